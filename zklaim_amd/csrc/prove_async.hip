// prove_async.hip — zkg_prover: Groth16 proofs of a resident key on the caller's stream, witnesses in device memory, proofs left in device
// memory, no host wait and no host arithmetic (include/zkg.h).
//
// A call composes the stream-ordered pieces the library already has — the QAP handle's launch sequence for coefficients_for_H, and three MSM
// jobs under msm_job_set_device_finish (H; A / B_1 / L in one launch over tables of the WHOLE witness queries; B_2) — and ends in the
// device epilogue below, which is assemble_proof's algebra (prover.hip) as kernels:
//   k_proof_comb      the key-only part: r delta_1, s alpha_1, r beta_1, rs delta_1 and s delta_2 from the key's fixed-base tables, one
//                     wavefront per product: 64 table picks and a lane tree.  Queued at the fork.
//   k_proof_g1_part   behind the G1 witness job's combine: the two variable-base products s (W_a + A_0) and r (W_b1 + B1_0) side by side
//                     (one DPP quad each, 4-bit windows, quad-cooperative additions and doublings), then the C sum without H and the
//                     finished A record.
//   k_proof_g2_part   behind the G2 job's combine: the B record.
//   k_proof_finish    behind H: C += H, one normalisation, the three records and the status word.
#include "common.hpp"
#include "proof_assemble.hpp"
#include "record.hip.hpp"
#include "../../include/zkg.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace zk {

// ---- the device epilogue -------------------------------------------------------------------------------------------------------------
// the key's points as the kernels take them (by value), and its four fixed-base tables in device memory (64 x 15 affine multiples each)
struct ProofKeyDev {
    G1Affine alpha, a0, b10; G2Affine beta2, b20;                 // alpha_1, A_query[0], B_g1[0]; beta_2, B_g2[0]
    const G1Affine *alpha1, *beta1, *delta1; const G2Affine *delta2;
};
static constexpr uint32_t G1_WORDS = 24, G2_WORDS = 48;           // a normalised point as msm_job_finish_dev stores it: X | Y | Z, Z = one or zero
static constexpr uint32_t PROOFS_PER_GROUP = 8;                   // k_proof_g1_part: a wavefront, two quads per proof
static constexpr uint32_t COMB_G1 = 4;                            // r delta_1 | s alpha_1 | r beta_1 | rs delta_1

ZK_D G1Affine load_point_g1(const uint32_t *in) {
    G1Affine a; Fq z;
    for (int i = 0; i < 8; ++i) { a.x.v[i] = in[i]; a.y.v[i] = in[8 + i]; z.v[i] = in[16 + i]; }
    return z.is_zero() ? G1Affine::inf() : a;
}
ZK_D G2Affine load_point_g2(const uint32_t *in) {
    G2Affine a; Fq2 z;
    for (int i = 0; i < 8; ++i) {
        a.x.c0.v[i] = in[i]; a.x.c1.v[i] = in[8 + i]; a.y.c0.v[i] = in[16 + i]; a.y.c1.v[i] = in[24 + i]; z.c0.v[i] = in[32 + i]; z.c1.v[i] = in[40 + i];
    }
    return z.is_zero() ? G2Affine::inf() : a;
}
ZK_D Fr load_fr(const uint64_t *in) { Fr r; for (int i = 0; i < 4; ++i) { r.v[2 * i] = (uint32_t)in[i]; r.v[2 * i + 1] = (uint32_t)(in[i] >> 32); } return r; }
ZK_D uint32_t nibble(const Fr &k, int j) { return (k.v[j >> 3] >> (4 * (j & 7))) & 15u; }

ZK_D Fq shfl_down(const Fq &a, int d) { Fq r; for (int i = 0; i < 8; ++i) r.v[i] = __shfl_down(a.v[i], d, 64); return r; }
ZK_D Fq2 shfl_down(const Fq2 &a, int d) { return {shfl_down(a.c0, d), shfl_down(a.c1, d)}; }
template <class F> ZK_D XYZZ<F> shfl_down(const XYZZ<F> &a, int d) { return {shfl_down(a.x, d), shfl_down(a.y, d), shfl_down(a.zz, d), shfl_down(a.zzz, d)}; }

// One wavefront per (proof, product): lane j picks digit j's multiple d 16^j P from the table, a tree of six additions sums the lanes.
// G1: blockIdx.y = 0 r delta_1, 1 s alpha_1, 2 r beta_1, 3 rs delta_1; G2: s delta_2.  out[proof * gridDim.y + product], as CombTable::mul gives it.
template <class F> __global__ __launch_bounds__(64) void k_proof_comb(const uint64_t *rs, ProofKeyDev key, XYZZ<F> *out) {
    const uint32_t p = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const Fr r = load_fr(rs + 8 * (size_t)p), s = load_fr(rs + 8 * (size_t)p + 4);
    Fr k; const Affine<F> *table;
    if constexpr (sizeof(F) == sizeof(Fq)) {
        k = c == 0 || c == 2 ? r : c == 1 ? s : r * s;
        table = c == 1 ? key.alpha1 : c == 2 ? key.beta1 : key.delta1;
    } else { k = s; table = key.delta2; }
    const uint32_t d = nibble(k.from_mont(), (int)lane);
    XYZZ<F> acc = XYZZ<F>::inf();
    if (d) acc = XYZZ<F>::from_affine(table[lane * 15 + d - 1]);
    for (int off = 32; off >= 1; off >>= 1) {
        const XYZZ<F> o = shfl_down(acc, off);
        if ((int)lane < off) acc.add_inl(o);
    }
    if (lane == 0) out[(size_t)p * gridDim.y + c] = acc.normalized();
}

// the doubling as a quad shares it (xyzz_add_quad's scheme, curve.hip.hpp): dbl-2008-s-1's nine products in three rounds and one
template <class F> ZK_D XYZZ<F> xyzz_dbl_quad(const XYZZ<F> &a, uint32_t q) {
    if (a.is_inf()) return a;                                                // quad-uniform
    const F U = a.y.dbl();
    const F m1 = quad_select(q, U, a.x, U, U) * quad_select(q, U, a.x, U, U);
    const F V = quad_bcast<0>(m1), xx = quad_bcast<1>(m1);
    const F m2 = quad_select(q, U, a.x, a.zz, a.zz) * V;
    const F W = quad_bcast<0>(m2), S = quad_bcast<1>(m2), ZZ3 = quad_bcast<2>(m2);
    const F M = xx.dbl() + xx;
    const F m3 = quad_select(q, M, W, W, W) * quad_select(q, M, a.y, a.zzz, a.zzz);
    const F X3 = quad_bcast<0>(m3) - S.dbl();
    const F Y3 = M * (S - X3) - quad_bcast<1>(m3);
    return {X3, Y3, ZZ3, quad_bcast<2>(m3)};
}

// Eight proofs per wavefront, two quads per proof: quad 0 computes s (W_a + A_0), quad 1 r (W_b1 + B1_0), each with a table of the 15 small
// multiples in LDS (every lane of a quad stores and reads its own identical copy: no barrier inside the ladder), 63 x 4 doublings and at most 64
// additions.  Then quad 0 sums what C has without H and quad 1 finishes A, record included.
// w1: per proof W_a | W_b1 | L (G1_WORDS each), w1_stride words apart; comb: k_proof_comb<Fq>'s output.
__global__ __launch_bounds__(64) void k_proof_g1_part(const uint64_t *rs, const uint32_t *w1, size_t w1_stride, const G1 *comb, ProofKeyDev key, uint32_t count,
                                                       G1 *c_part, uint8_t *a_rec) {
    __shared__ G1 tab[16][15];
    __shared__ G1 xch[16];
    const uint32_t lane = threadIdx.x, q = lane & 3, quad = lane >> 2, which = quad & 1, slot = lane >> 3;
    const uint32_t p = blockIdx.x * PROOFS_PER_GROUP + slot;
    const bool live = p < count;
    G1 wa = G1::inf();
    if (live) {
        const uint32_t *pts = w1 + (size_t)p * w1_stride;
        wa = G1::from_affine(load_point_g1(pts)); wa.madd(key.a0);                                   // the constant column first
        G1 base = wa;
        if (which) { base = G1::from_affine(load_point_g1(pts + G1_WORDS)); base.madd(key.b10); }
        const Fr k = load_fr(rs + 8 * (size_t)p + (which ? 0 : 4)).from_mont();                      // s for W_a, r for W_b1
        G1 t = base;
        tab[quad][0] = t;
        for (int d = 2; d <= 15; ++d) { xyzz_add_quad<Fq>(t, base, q); tab[quad][d - 1] = t; }
        G1 acc = G1::inf();
#pragma unroll 1
        for (int j = 63; j >= 0; --j) {
            if (j != 63) for (int i = 0; i < 4; ++i) acc = xyzz_dbl_quad<Fq>(acc, q);
            const uint32_t d = nibble(k, j);
            if (d) { const G1 e = tab[quad][d - 1]; xyzz_add_quad<Fq>(acc, e, q); }
        }
        xch[quad] = acc;
    }
    __syncthreads();
    if (!live) return;
    const G1 *cb = comb + (size_t)p * COMB_G1;
    if (which == 0) {                                                                                // s alpha + r beta_1 + rs delta + s W_a + r W_b1 + L
        G1 c = xch[quad];
        xyzz_add_quad<Fq>(c, xch[quad + 1], q);
        c.madd(load_point_g1(w1 + (size_t)p * w1_stride + 2 * G1_WORDS));
        for (int i = 1; i <= 3; ++i) xyzz_add_quad<Fq>(c, cb[i], q);
        if (q == 0) c_part[p] = c.normalized();
    } else {                                                                                         // alpha + r delta + W_a
        G1 a = G1::from_affine(key.alpha);
        xyzz_add_quad<Fq>(a, cb[0], q);
        xyzz_add_quad<Fq>(a, wa, q);
        const G1Affine aff = a.to_affine();
        if (q == 0) put_g1_record(a_rec + (size_t)p * 34, aff);
    }
}
// beta_2 + s delta_2 + W_b2 + B2_0, one lane per proof.  w2: per proof W_b2 (G2_WORDS), w2_stride words apart; comb: k_proof_comb<Fq2>'s output
__global__ __launch_bounds__(64) void k_proof_g2_part(const uint32_t *w2, size_t w2_stride, const G2 *comb, ProofKeyDev key, uint32_t count, uint8_t *b_rec) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count) return;
    G2 b = G2::from_affine(key.beta2);
    b.add_inl(comb[p]);
    b.madd(load_point_g2(w2 + (size_t)p * w2_stride));
    b.madd(key.b20);
    put_g2_record(b_rec + (size_t)p * 66, b.to_affine());
}
// C = c_part + H, the status word (unsat given: 2 where check and the word is set, else 0) and the proof's bytes — nothing for an unsatisfied
// item.  One lane per proof; byte stores, so no alignment is asked of `proofs`.
__global__ __launch_bounds__(64) void k_proof_finish(const G1 *c_part, const uint32_t *hpt, size_t h_stride, const uint8_t *a_rec, const uint8_t *b_rec,
                                                      const uint32_t *unsat /* or null */, int check, uint32_t count, uint8_t *proofs, size_t proof_stride, uint32_t *status /* or null */) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count) return;
    const bool refused = check && unsat && unsat[p] != 0;
    if (status) status[p] = refused ? ZKG_UNSATISFIED : ZKG_OK;
    if (refused) return;
    G1 c = c_part[p];
    c.madd(load_point_g1(hpt + (size_t)p * h_stride));
    uint8_t *o = proofs + (size_t)p * proof_stride;
    for (int i = 0; i < 34; ++i) o[i] = a_rec[(size_t)p * 34 + i];
    for (int i = 0; i < 66; ++i) o[34 + i] = b_rec[(size_t)p * 66 + i];
    put_g1_record(o + 100, c.to_affine());
}

// the epilogue's buffers for `cap` proofs
struct EpilogueWs {
    DevBuf comb1, comb2, c_part, a_rec, b_rec; size_t cap = 0;
    int reserve(size_t g) {
        if (g <= cap) return ZKG_OK;
        if (comb1.reserve(g * COMB_G1 * sizeof(G1)) || comb2.reserve(g * sizeof(G2)) || c_part.reserve(g * sizeof(G1)) || a_rec.reserve(g * 34 + 16) || b_rec.reserve(g * 66 + 16)) return ZKG_ERROR;
        cap = g;
        return ZKG_OK;
    }
    void release() { for (DevBuf *b : {&comb1, &comb2, &c_part, &a_rec, &b_rec}) b->release(); cap = 0; }
};
// The three stages' launches.  s_key: the key-only part; s_g1 / s_g2: the streams the witness points arrive on; s_fin: where H arrives.  The
// caller orders the streams (events) between the stages.
static void launch_key_part(const EpilogueWs &E, const ProofKeyDev &kd, const uint64_t *d_rs, uint32_t g, hipStream_t s) {
    hipLaunchKernelGGL(k_proof_comb<Fq>, dim3(g, COMB_G1), dim3(64), 0, s, d_rs, kd, E.comb1.as<G1>());
    hipLaunchKernelGGL(k_proof_comb<Fq2>, dim3(g, 1), dim3(64), 0, s, d_rs, kd, E.comb2.as<G2>());
}
static void launch_g1_part(const EpilogueWs &E, const ProofKeyDev &kd, const uint64_t *d_rs, const uint32_t *w1, size_t w1_stride, uint32_t g, hipStream_t s) {
    hipLaunchKernelGGL(k_proof_g1_part, dim3((g + PROOFS_PER_GROUP - 1) / PROOFS_PER_GROUP), dim3(64), 0, s, d_rs, w1, w1_stride, (const G1 *)E.comb1.as<G1>(), kd, g, E.c_part.as<G1>(), E.a_rec.as<uint8_t>());
}
static void launch_g2_part(const EpilogueWs &E, const ProofKeyDev &kd, const uint32_t *w2, size_t w2_stride, uint32_t g, hipStream_t s) {
    hipLaunchKernelGGL(k_proof_g2_part, dim3((g + 63) / 64), dim3(64), 0, s, w2, w2_stride, (const G2 *)E.comb2.as<G2>(), kd, g, E.b_rec.as<uint8_t>());
}
static void launch_finish(const EpilogueWs &E, const uint32_t *hpt, size_t h_stride, const uint32_t *unsat, int check, uint32_t g, uint8_t *proofs, size_t proof_stride, uint32_t *status, hipStream_t s) {
    hipLaunchKernelGGL(k_proof_finish, dim3((g + 63) / 64), dim3(64), 0, s, (const G1 *)E.c_part.as<G1>(), hpt, h_stride, (const uint8_t *)E.a_rec.as<uint8_t>(), (const uint8_t *)E.b_rec.as<uint8_t>(),
                       unsat, check, g, proofs, proof_stride, status);
}
// the key's tables and points into device memory (synchronous: a handle's construction, the test hook)
static int upload_key(const ProofKey &key, const G1Affine &a0, const G1Affine &b10, const G2Affine &b20, DevBuf &tables, ProofKeyDev &kd) {
    const size_t g1b = COMB_ENTRIES * sizeof(G1Affine), g2b = COMB_ENTRIES * sizeof(G2Affine);
    if (key.alpha1->t.size() != COMB_ENTRIES || key.beta1->t.size() != COMB_ENTRIES || key.delta1->t.size() != COMB_ENTRIES || key.delta2->t.size() != COMB_ENTRIES) { set_error("proof epilogue: the key has no fixed-base tables"); return ZKG_ERROR; }
    if (tables.reserve(3 * g1b + g2b)) return ZKG_ERROR;
    uint8_t *d = tables.as<uint8_t>();
    ZK_HIP(hipMemcpy(d, key.alpha1->t.data(), g1b, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(d + g1b, key.beta1->t.data(), g1b, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(d + 2 * g1b, key.delta1->t.data(), g1b, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(d + 3 * g1b, key.delta2->t.data(), g2b, hipMemcpyHostToDevice));
    kd.alpha = key.alpha_g1; kd.a0 = a0; kd.b10 = b10; kd.beta2 = key.beta_g2; kd.b20 = b20;
    kd.alpha1 = reinterpret_cast<const G1Affine *>(d); kd.beta1 = kd.alpha1 + COMB_ENTRIES; kd.delta1 = kd.beta1 + COMB_ENTRIES;
    kd.delta2 = reinterpret_cast<const G2Affine *>(d + 3 * g1b);
    return ZKG_OK;
}

}  // namespace zk

using namespace zk;

// ---- zkg_proof_assemble: the epilogue alone -------------------------------------------------------------------------------------------
static int proof_assemble_impl(const uint64_t *key_points, const uint64_t *points, const uint64_t *rs, size_t count, int where, uint8_t *proofs_out) {
    static const char *who = "zkg_proof_assemble";
    if (!key_points || (count && (!points || !rs || !proofs_out)) || count > ((size_t)1 << 16) || (where != 0 && where != 1)) {
        set_error(std::string(who) + ": bad argument (count <= 2^16, where 0 or 1)"); return ZKG_ERROR;
    }
    if (where == 1 && initialised_device() < 0) { set_error("zkg_init not called"); return ZKG_ERROR; }
    if (count == 0) return ZKG_OK;
    G1Affine g1[5]; G2Affine g2[3];                                        // alpha_1 beta_1 delta_1 A_0 B1_0 | beta_2 delta_2 B2_0
    memcpy(g1, key_points, sizeof g1); memcpy(g2, key_points + 40, sizeof g2);
    CombTable<Fq> alpha1, beta1, delta1; CombTable<Fq2> delta2;
    alpha1.build(g1[0]); beta1.build(g1[1]); delta1.build(g1[2]); delta2.build(g2[1]);
    ProofKey key; key.alpha_g1 = g1[0]; key.beta_g2 = g2[0]; key.alpha1 = &alpha1; key.beta1 = &beta1; key.delta1 = &delta1; key.delta2 = &delta2;
    if (where == 0) {
        for (size_t p = 0; p < count; ++p) {
            const uint64_t *pt = points + 72 * p;
            G1 W1[3] = {load_norm_g1(pt), load_norm_g1(pt + 12), load_norm_g1(pt + 24)}; const G1 Ht = load_norm_g1(pt + 36); G2 Wb2 = load_norm_g2(pt + 48);
            W1[0].madd(g1[3]); W1[1].madd(g1[4]); Wb2.madd(g2[2]);          // the constant column
            Fr r, s; memcpy(r.v, rs + 8 * p, 32); memcpy(s.v, rs + 8 * p + 4, 32);
            assemble_proof(key, r, s, W1, Wb2, Ht, proofs_out + p * ZKG_PROOF_BYTES);
        }
        return ZKG_OK;
    }
    ScopedDevBuf tables, d_points, d_rs, d_out; ProofKeyDev kd;
    struct Ws : EpilogueWs { ~Ws() { release(); } } E;
    if (upload_key(key, g1[3], g1[4], g2[2], tables, kd) || E.reserve(count) || d_points.reserve(count * 72 * 8) || d_rs.reserve(count * 64) || d_out.reserve(count * ZKG_PROOF_BYTES + 16)) return ZKG_ERROR;
    ZK_HIP(hipMemcpy(d_points.p, points, count * 72 * 8, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(d_rs.p, rs, count * 64, hipMemcpyHostToDevice));
    const uint32_t *pw = d_points.as<uint32_t>(); const uint32_t g = (uint32_t)count;
    launch_key_part(E, kd, d_rs.as<uint64_t>(), g, nullptr);
    launch_g1_part(E, kd, d_rs.as<uint64_t>(), pw, 144, g, nullptr);
    launch_g2_part(E, kd, pw + 96, 144, g, nullptr);
    launch_finish(E, pw + 72, 144, nullptr, 0, g, d_out.as<uint8_t>(), ZKG_PROOF_BYTES, nullptr, nullptr);
    if (hipGetLastError() != hipSuccess) { set_error(std::string(who) + ": kernel launch failed"); return ZKG_ERROR; }
    ZK_HIP(hipMemcpy(proofs_out, d_out.p, count * ZKG_PROOF_BYTES, hipMemcpyDeviceToHost));          // (waits for the null stream)
    return ZKG_OK;
}

// ---- the handle -----------------------------------------------------------------------------------------------------------------------
struct zkg_prover {
    zkg_crs *crs = nullptr; CrsProverView v; int device = 0; std::mutex mu; bool ref = false;
    zkg_qap *qap = nullptr;
    WindowTable tA, tB1, tL, tB2;                        // per-window tables over A[1..n], B_g1[1..n], L padded to n points, B_g2[1..n]
    MsmJob *job_w1 = nullptr, *job_w2 = nullptr, *job_h = nullptr;
    // s_h: mat-vec, transforms, H, finish — the critical path; s_w1 / s_w2: the witness jobs and their parts of the epilogue; s_key: the key-only part
    hipStream_t s_h = nullptr, s_w1 = nullptr, s_w2 = nullptr, s_key = nullptr;
    hipEvent_t ev_fork = nullptr, ev_key = nullptr, ev_w1 = nullptr, ev_w2 = nullptr, ev_fin = nullptr; bool fin_recorded = false;
    DevBuf key_tables; ProofKeyDev kd;
    DevBuf h, unsat, w1, w2, hpt; EpilogueWs E;          // a group's coefficients_for_H (m + 1 per proof), unsatisfied words, and the five points per proof
    size_t bmax_default = 1, bmax = 1;
};
static thread_local size_t t_prover_stats[3];

static void prover_drain(zkg_prover *p) { for (hipStream_t s : {p->s_h, p->s_w1, p->s_w2, p->s_key}) if (s) (void)hipStreamSynchronize(s); }
static void prover_destroy(zkg_prover *p) {
    int cur = 0; (void)hipGetDevice(&cur);
    if (cur != p->device) (void)hipSetDevice(p->device);                 // the handle's memory, streams and events live on the key's device
    prover_drain(p);
    if (p->qap) zkg_qap_free(p->qap);
    msm_job_destroy(p->job_w1); msm_job_destroy(p->job_w2); msm_job_destroy(p->job_h);
    for (hipStream_t *s : {&p->s_h, &p->s_w1, &p->s_w2, &p->s_key}) if (*s) (void)hipStreamDestroy(*s);
    for (hipEvent_t *e : {&p->ev_fork, &p->ev_key, &p->ev_w1, &p->ev_w2, &p->ev_fin}) if (*e) (void)hipEventDestroy(*e);
    for (WindowTable *t : {&p->tA, &p->tB1, &p->tL, &p->tB2}) t->release();
    for (DevBuf *b : {&p->key_tables, &p->h, &p->unsat, &p->w1, &p->w2, &p->hpt}) b->release();
    p->E.release();
    if (p->ref) (void)crs_prover_ref(p->crs, -1);
    if (cur != p->device) (void)hipSetDevice(cur);
    delete p;
}
// the constraint system back from the key's device copy, for the QAP handle (which keeps a device copy of its own)
static zkg_qap *qap_from_view(const CrsProverView &v) {
    std::vector<uint32_t> rp[3], col[3]; std::vector<uint64_t> val[3];
    for (int k = 0; k < 3; ++k) {
        rp[k].resize((size_t)v.C + 1); col[k].resize(v.nnz[k]); val[k].resize(v.nnz[k] * 4);
        if (!hip_ok(hipMemcpy(rp[k].data(), v.rp[k], rp[k].size() * 4, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__)) return nullptr;
        if (v.nnz[k] && (!hip_ok(hipMemcpy(col[k].data(), v.col[k], v.nnz[k] * 4, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__) ||
                         !hip_ok(hipMemcpy(val[k].data(), v.val[k], v.nnz[k] * 32, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__))) return nullptr;
    }
    zkg_r1cs cs; memset(&cs, 0, sizeof cs);
    cs.num_variables = v.n; cs.num_inputs = v.l; cs.num_constraints = v.C;
    cs.a_rowptr = rp[0].data(); cs.a_col = col[0].data(); cs.a_val = val[0].data();
    cs.b_rowptr = rp[1].data(); cs.b_col = col[1].data(); cs.b_val = val[1].data();
    cs.c_rowptr = rp[2].data(); cs.c_col = col[2].data(); cs.c_val = val[2].data();
    return zkg_qap_new(&cs);
}
static MsmBases table_set(const WindowTable &t) { MsmBases b; b.p = t.buf.p; b.g2 = t.g2; b.level_stride = t.n; b.p29 = t.rec29.p; return b; }

static zkg_prover *prover_new_impl(const zkg_crs *crs_c) {
    static const char *who = "zkg_prover_new";
    auto refuse = [&](const char *why) { set_error(std::string(who) + ": " + why); return (zkg_prover *)nullptr; };
    if (!crs_c) return refuse("null key");
    // before anything reads the key: without zkg_init no key can exist, so a pointer given here is not looked at (tests/test_prove_async_host.py
    // passes a buffer of zeros on a machine without a GPU)
    const int dev = initialised_device();
    if (dev < 0) { set_error("zkg_init not called"); return nullptr; }
    zkg_crs *crs = const_cast<zkg_crs *>(crs_c);                          // (the key's handle counter; the key's data is only read)
    std::unique_ptr<zkg_prover, void (*)(zkg_prover *)> p(new zkg_prover(), prover_destroy);
    p->crs = crs;
    crs_prover_view(crs, p->v);
    const CrsProverView &v = p->v;
    p->device = v.device;
    if (wrong_device_refused(who, v.device, "the key was uploaded on")) return nullptr;
    if (v.device != dev) return refuse("the key is not on the zkg_init device (the domain tables live there)");
    if (!crs_prover_ref(crs, +1)) return refuse("the key's H query is sharded over several devices");
    p->ref = true;
    const size_t n = v.n, m = v.m;
    if (!n || m < 2) return refuse("a key without variables");
    if (!(p->qap = qap_from_view(v))) return nullptr;
    if (zkg_qap_domain_size(p->qap) != m) return refuse("the key's domain is not get_evaluation_domain(C + l + 1)");
    // the tables over the whole witness queries; the G1 sets go through one launch of three sets, which reads no 29-bit records
    const int c_w = table_window_bits(n);
    {
        ScopedDevBuf lpad;
        if (lpad.reserve(n * sizeof(G1Affine))) return nullptr;
        if (!hip_ok(hipMemset(lpad.p, 0, (size_t)v.l * sizeof(G1Affine)), "hipMemset", __FILE__, __LINE__) ||
            (n > v.l && !hip_ok(hipMemcpy(lpad.as<G1Affine>() + v.l, v.L_query, (n - v.l) * sizeof(G1Affine), hipMemcpyDeviceToDevice), "D2D", __FILE__, __LINE__))) return nullptr;
        if (window_table_build_g1(p->tA, v.A_query + 1, n, c_w, nullptr) || window_table_build_g1(p->tB1, v.B_g1 + 1, n, c_w, nullptr) ||
            window_table_build_g1(p->tL, lpad.as<G1Affine>(), n, c_w, nullptr) || window_table_build_g2(p->tB2, v.B_g2 + 1, n, c_w, nullptr) ||
            !hip_ok(hipDeviceSynchronize(), "sync", __FILE__, __LINE__)) return nullptr;
    }
    G1Affine a0, b10; G2Affine b20;
    if (!hip_ok(hipMemcpy(&a0, v.A_query, sizeof a0, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__) || !hip_ok(hipMemcpy(&b10, v.B_g1, sizeof b10, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__) ||
        !hip_ok(hipMemcpy(&b20, v.B_g2, sizeof b20, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__) || upload_key(v.key, a0, b10, b20, p->key_tables, p->kd)) return nullptr;
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    bool ok = hip_ok(hipStreamCreateWithPriority(&p->s_h, hipStreamNonBlocking, prio_hi), "hipStreamCreate", __FILE__, __LINE__);
    for (hipStream_t *s : {&p->s_w1, &p->s_w2, &p->s_key}) ok = ok && hip_ok(hipStreamCreateWithPriority(s, hipStreamNonBlocking, prio_lo), "hipStreamCreate", __FILE__, __LINE__);
    for (hipEvent_t *e : {&p->ev_fork, &p->ev_key, &p->ev_w1, &p->ev_w2, &p->ev_fin}) ok = ok && hip_ok(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate", __FILE__, __LINE__);
    if (!ok) return nullptr;
    p->job_h = msm_job_create(p->s_h, false); p->job_w1 = msm_job_create(p->s_w1, false); p->job_w2 = msm_job_create(p->s_w2, false);
    if (!p->job_h || !p->job_w1 || !p->job_w2) return nullptr;
    msm_job_set_window(p->job_h, v.H->c); msm_job_set_row_merge(p->job_h, v.h_row_merge);
    for (MsmJob *j : {p->job_w1, p->job_w2}) { msm_job_set_window(j, c_w); msm_job_set_skewed(j, true); }     // a witness is mostly bits: the one-pass sort
    for (MsmJob *j : {p->job_h, p->job_w1, p->job_w2}) msm_job_set_device_finish(j, true);
    // proofs per launch sequence: what the three multi launches take, the QAP handle's group and the G2 job's bucket workspace (1 GiB)
    size_t g = std::min<size_t>(MSM_MULTI_MAX_VECTORS, std::max<size_t>(1, ((size_t)1 << 30) / msm_table_bucket_bytes(c_w, true)));
    while (g > 1 && !(msm_multi_supported(n, c_w, (uint32_t)g) && msm_multi_supported(m - 1, v.H->c, (uint32_t)g))) --g;
    p->bmax_default = p->bmax = std::max<size_t>(1, std::min(g, zkg_qap_batch_max(p->qap)));
    return p.release();
}

static bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}
// a table launch of `g` scalar vectors on the job's stream and its device epilogue into d_out; drains of the job's stream (a buffer that had to
// grow) are counted in waits
static int job_launch(MsmJob *job, const MsmBases *sets, int nsets, const uint32_t *sc, size_t n, size_t stride_words, uint32_t g, uint64_t *d_out, size_t &waits) {
    ReserveGuard guard(msm_job_stream(job));
    int rc = g > 1 ? msm_job_launch_multi(job, sets, nsets, sc, n, stride_words, g, true) : msm_job_launch(job, sets, nsets, sc, n, true, nullptr);
    if (rc == ZKG_OK) rc = msm_job_finish_dev(job, d_out);
    waits += guard.drains;
    return rc;
}
static int prover_prove_async_impl(zkg_prover *p, const void *d_witnesses, size_t stride, size_t count, const void *d_rs, int check_satisfied,
                                   void *d_proofs, size_t proof_stride, uint32_t *d_status, void *stream) {
    static const char *who = "zkg_prover_prove_async";
    for (size_t &x : t_prover_stats) x = 0;
    if (count == 0) return ZKG_OK;                                      // nothing to do, nothing touched
    if (initialised_device() < 0) { set_error("zkg_init not called"); return ZKG_ERROR; }
    if (!p || !d_witnesses || !d_rs || !d_proofs || !d_status) { set_error(std::string(who) + ": bad argument (null handle or pointer)"); return ZKG_ERROR; }
    const CrsProverView &v = p->v;
    const size_t n = v.n, m = v.m;
    if (proof_stride < ZKG_PROOF_BYTES || proof_stride > ZKG_MSM_ASYNC_MAX_STRIDE) { set_error(std::string(who) + ": proof_stride must be at least ZKG_PROOF_BYTES (and at most 2^32)"); return ZKG_ERROR; }
    if (async_vectors_refused(who, n, "n", stride, count, p->device, "the key was uploaded on")) return ZKG_ERROR;
    const size_t w_bytes = ((count - 1) * stride + n) * 32, rs_bytes = count * 64, pr_bytes = (count - 1) * proof_stride + ZKG_PROOF_BYTES, st_bytes = count * 4;
    if (dev_range_refused(d_witnesses, w_bytes, 16, p->device, who, "d_witnesses", "key") || dev_range_refused(d_rs, rs_bytes, 16, p->device, who, "d_rs", "key") ||
        dev_range_refused(d_proofs, pr_bytes, 1, p->device, who, "d_proofs", "key") || dev_range_refused(d_status, st_bytes, 4, p->device, who, "d_status", "key")) return ZKG_ERROR;
    const void *rg[4] = {d_witnesses, d_rs, d_proofs, d_status}; const size_t rb[4] = {w_bytes, rs_bytes, pr_bytes, st_bytes};
    for (int i = 0; i < 4; ++i) for (int j = i + 1; j < 4; ++j)
        if (ranges_overlap(rg[i], rb[i], rg[j], rb[j])) { set_error(std::string(who) + ": the input and output ranges overlap"); return ZKG_ERROR; }
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(p->mu);                              // held for the enqueue only: the handle's streams keep its calls in call order
    size_t waits = 0, groups = 0, done = 0;
    // the workspace of the call's largest group.  Growing frees: earlier calls may still be in it, so the handle's streams are drained first
    const size_t gmax = std::min(p->bmax, count);
    if (gmax > p->E.cap) {
        prover_drain(p); ++waits;
        if (p->h.reserve(gmax * (m + 1) * 32) || p->unsat.reserve(gmax * 4) || p->w1.reserve(gmax * 3 * G1_WORDS * 4) || p->w2.reserve(gmax * G2_WORDS * 4) ||
            p->hpt.reserve(gmax * G1_WORDS * 4) || p->E.reserve(gmax)) return ZKG_ERROR;
    }
    ZK_HIP(hipEventRecord(p->ev_fork, s));                              // behind the work that writes the witnesses and (r, s); nothing is enqueued yet
    for (hipStream_t hs : {p->s_h, p->s_w1, p->s_w2, p->s_key}) ZK_HIP(hipStreamWaitEvent(hs, p->ev_fork, 0));
    const MsmBases g1sets[3] = {table_set(p->tA), table_set(p->tB1), table_set(p->tL)}, g2set = table_set(p->tB2), hset = table_set(*v.H);
    const Fr *w = (const Fr *)d_witnesses; const uint64_t *rs = (const uint64_t *)d_rs; uint8_t *proofs = (uint8_t *)d_proofs;
    int rc = ZKG_OK;
    while (done < count && rc == ZKG_OK) {
        const uint32_t g = (uint32_t)std::min(p->bmax, count - done);
        const uint32_t *wg = reinterpret_cast<const uint32_t *>(w + done * stride); const uint64_t *rsg = rs + 8 * done;
        // the side streams reuse the group buffers: behind the finish of the group before (the last call's last group for the first)
        if (p->fin_recorded) for (hipStream_t hs : {p->s_w1, p->s_w2, p->s_key}) ZK_HIP(hipStreamWaitEvent(hs, p->ev_fin, 0));
        launch_key_part(p->E, p->kd, rsg, g, p->s_key);
        ZK_HIP(hipEventRecord(p->ev_key, p->s_key));
        // A, B_1, L: one launch of three sets over the witnesses themselves, then the ladder right behind its combine
        rc = job_launch(p->job_w1, g1sets, 3, wg, n, stride * 8, g, p->w1.as<uint64_t>(), waits);
        if (rc != ZKG_OK) break;
        ZK_HIP(hipStreamWaitEvent(p->s_w1, p->ev_key, 0));
        launch_g1_part(p->E, p->kd, rsg, p->w1.as<uint32_t>(), 3 * G1_WORDS, g, p->s_w1);
        ZK_HIP(hipEventRecord(p->ev_w1, p->s_w1));
        rc = job_launch(p->job_w2, &g2set, 1, wg, n, stride * 8, g, p->w2.as<uint64_t>(), waits);
        if (rc != ZKG_OK) break;
        ZK_HIP(hipStreamWaitEvent(p->s_w2, p->ev_key, 0));
        launch_g2_part(p->E, p->kd, p->w2.as<uint32_t>(), G2_WORDS, g, p->s_w2);
        ZK_HIP(hipEventRecord(p->ev_w2, p->s_w2));
        // coefficients_for_H and the unsatisfied words (the QAP handle's launch sequence), then H over them: m - 1 scalars at stride m + 1
        size_t qs[3] = {0, 0, 0};
        rc = qap_witness_h_enqueue(p->qap, wg, stride, g, p->h.p, m + 1, p->unsat.as<uint32_t>(), p->s_h, qs);
        waits += qs[2];
        if (rc != ZKG_OK) break;
        rc = job_launch(p->job_h, &hset, 1, p->h.as<uint32_t>(), m - 1, (m + 1) * 8, g, p->hpt.as<uint64_t>(), waits);
        if (rc != ZKG_OK) break;
        ZK_HIP(hipStreamWaitEvent(p->s_h, p->ev_w1, 0));
        ZK_HIP(hipStreamWaitEvent(p->s_h, p->ev_w2, 0));
        launch_finish(p->E, p->hpt.as<uint32_t>(), G1_WORDS, p->unsat.as<uint32_t>(), check_satisfied, g, proofs + done * proof_stride, proof_stride, d_status + done, p->s_h);
        if (hipGetLastError() != hipSuccess) { set_error(std::string(who) + ": kernel launch failed"); rc = ZKG_ERROR; break; }
        ZK_HIP(hipEventRecord(p->ev_fin, p->s_h));
        p->fin_recorded = true;
        done += g; ++groups;
    }
    // whatever the caller queues on `stream` after this call sees the proofs and the status — after a failure too: what was enqueued still runs
    bool ordered = true;
    if (rc == ZKG_OK) ordered = hip_ok(hipStreamWaitEvent(s, p->ev_fin, 0), "hipStreamWaitEvent", __FILE__, __LINE__);      // the last finish is behind everything of the call
    else for (hipStream_t hs : {p->s_h, p->s_w1, p->s_w2, p->s_key})                                                          // a broken group: every stream on its own
        ordered = hip_ok(hipEventRecord(p->ev_key, hs), "hipEventRecord", __FILE__, __LINE__) && hip_ok(hipStreamWaitEvent(s, p->ev_key, 0), "hipStreamWaitEvent", __FILE__, __LINE__) && ordered;
    t_prover_stats[0] = done; t_prover_stats[1] = groups; t_prover_stats[2] = waits;
    return rc == ZKG_OK && ordered ? ZKG_OK : ZKG_ERROR;
}

extern "C" {

int zkg_proof_assemble(const uint64_t *key_points, const uint64_t *points, const uint64_t *rs, size_t count, int where, uint8_t *proofs_out) {
    return c_boundary("zkg_proof_assemble", ZKG_ERROR, [&] { return proof_assemble_impl(key_points, points, rs, count, where, proofs_out); });
}
zkg_prover *zkg_prover_new(const zkg_crs *crs) { return c_boundary<zkg_prover *>("zkg_prover_new", nullptr, [&] { return prover_new_impl(crs); }); }
void zkg_prover_free(zkg_prover *p) {
    if (!p) return;
    c_boundary("zkg_prover_free", 0, [&] { prover_destroy(p); return 0; });
}
size_t zkg_prover_batch_max(const zkg_prover *p) {
    if (!p) return 0;
    return c_boundary<size_t>("zkg_prover_batch_max", 0, [&] { std::lock_guard<std::mutex> lk(const_cast<zkg_prover *>(p)->mu); return p->bmax; });
}
void zkg_prover_set_batch_max(zkg_prover *p, size_t k) {
    if (!p) return;
    c_boundary("zkg_prover_set_batch_max", 0, [&] { std::lock_guard<std::mutex> lk(p->mu); p->bmax = clamp_batch_max(k, p->bmax_default); return 0; });
}
int zkg_prover_prove_async(zkg_prover *p, const void *d_witnesses, size_t stride, size_t count, const void *d_rs, int check_satisfied,
                           void *d_proofs, size_t proof_stride, uint32_t *d_status, void *stream) {
    return c_boundary("zkg_prover_prove_async", ZKG_ERROR, [&] { return prover_prove_async_impl(p, d_witnesses, stride, count, d_rs, check_satisfied, d_proofs, proof_stride, d_status, stream); });
}
void zkg_prover_stats(size_t out[3]) { if (out) for (int i = 0; i < 3; ++i) out[i] = t_prover_stats[i]; }

}  // extern "C"
