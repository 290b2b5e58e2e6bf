// setup_verify.hip — Groth16 key generation and verification for the zklaim seam.
//
// Replaces r1cs_gg_ppzksnark_generator (/root/reference/zklaim/snark.cpp:91, reached from libsnark_trusted_setup,
// zklaim/libsnark_wrapper.cpp:195-215) and r1cs_gg_ppzksnark_verifier_strong_IC (snark.cpp:62, reached from libsnark_verify,
// libsnark_wrapper.cpp:252-276), plus the vk / pk blob export (libsnark_wrapper.cpp:122-157).
//
// Generator: swap A and B when B touches more variables (libsnark's swap_AB_if_beneficial: fewer G2 bases), evaluate the QAP
// at the trapdoor point t on the host (Lagrange coefficients in closed form with one batched inversion, then one pass over
// the non-zeros), and turn the ~4n + m scalars into curve points with the fixed-base kernels of msm.hip on the GPU — the part
// that dominates the reference's setup time.  Domain: libfqfft's get_evaluation_domain(C + l + 1) rule
// (evaluation_domain_shape, ntt.hip): basic_radix2_domain or step_radix2_domain, Lagrange coefficients from domain_lagrange.
// Verifier: host pairing (host/pairing.hpp); the public input is folded into gamma_ABC with host scalar multiplications.
#include "common.hpp"
#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <chrono>
#include "../../include/zkg.h"
#include "../../include/zklaim_abi.h"
#include "zklaim_public.hip.hpp"
#include "host/serialize.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <sys/random.h>

using namespace zk;
using zk::pairing::Fq12;
using zk::pairing::Fq6;

struct zkg_keypair {
    // the (possibly swapped) constraint system stored in the pk
    std::vector<uint32_t> rp[3], col[3]; std::vector<uint64_t> val[3];
    uint32_t n = 0, l = 0, C = 0, log_m = 0; size_t m = 0; bool swapped = false;
    ser::Bytes pk_blob; std::mutex blob_mu;            // serialised once, on first request
    G1Affine alpha_g1, beta_g1, delta_g1; G2Affine beta_g2, delta_g2, gamma_g2;
    std::vector<G1Affine> A_query, B_g1, H_query, L_query, IC;
    std::vector<G2Affine> B_g2;
    Fq12 alpha_beta;
    zkg_pk pk_view;
    // the resident generator (setup_resident_core) leaves the five queries on the DEVICE instead (they become the resident key of the proofs that
    // follow): the host vectors above stay empty, pk_view's query pointers are device pointers, b_idx lists the B query's non-zero entries
    // (host copy, for the blob's decimal text) and dBidx holds the same list on the device (for compress_kc_records)
    bool on_device = false; DevBuf dA, dB1, dB2, dH, dL, dBidx; std::vector<uint32_t> b_idx;
    ~zkg_keypair() { for (DevBuf *b : {&dA, &dB1, &dB2, &dH, &dL, &dBidx}) b->release(); }
};

namespace {

Fr fr_from_canonical(const uint64_t *limbs) { Fr x; memcpy(x.v, limbs, 32); return x.to_mont(); }

Fr random_fr() {
    std::random_device rd;                                   // the reference draws its toxic waste from std::random_device too
    for (;;) {
        Fr x;
        for (int i = 0; i < 8; ++i) x.v[i] = rd();
        x.v[7] &= 0x3fffffffu;
        bool lt = false;
        for (int i = 7; i >= 0; --i) { if (x.v[i] != FrParams::P[i]) { lt = x.v[i] < FrParams::P[i]; break; } }
        if (lt && !x.is_zero()) return x;                    // uniform in [1, r); reading it as a Montgomery residue keeps it uniform
    }
}

void copy_csr(std::vector<uint32_t> &rp, std::vector<uint32_t> &col, std::vector<uint64_t> &val, const uint32_t *s_rp, const uint32_t *s_col, const uint64_t *s_val, uint32_t rows) {
    rp.assign(s_rp, s_rp + rows + 1);
    size_t nnz = s_rp[rows];
    col.assign(s_col, s_col + nnz);
    val.assign(s_val, s_val + 4 * nnz);
}

// the scalars of one fixed-base batch: a host vector (uploaded by the batch), or n Montgomery Fr that already lie on the device
// (zkg_groth16_setup_dev: computed there by work queued on the null stream, which is where the batches run)
struct Scalars {
    const std::vector<Fr> *host = nullptr; const Fr *dev = nullptr; size_t n = 0;
    Scalars(const std::vector<Fr> &v) : host(&v), n(v.size()) {}
    Scalars(const Fr *d, size_t count) : dev(d), n(count) {}
    size_t size() const { return n; }
};

template <class A, class FN>
int batch_points(FN fixed_base_fn, const A &base, const Scalars &scalars, std::vector<A> &out) {
    size_t n = scalars.size();
    out.resize(n);
    if (!n) return ZKG_OK;
    static_assert(sizeof(Fr) == 32, "Fr is the 32-byte Montgomery element the kernel reads");
    DevBuf d_s, d_o;
    if ((scalars.host && d_s.reserve(n * 32)) || d_o.reserve(n * sizeof(A))) return ZKG_ERROR;
    int rc = ZKG_ERROR;                                    // Montgomery scalars go up as they are: the kernel converts (no host pass)
    if ((!scalars.host || hip_ok(hipMemcpy(d_s.p, scalars.host->data(), n * 32, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__)) &&
        fixed_base_fn(base, scalars.host ? d_s.as<uint32_t>() : reinterpret_cast<const uint32_t *>(scalars.dev), n, d_o.as<A>(), nullptr, true) == ZKG_OK &&
        hip_ok(hipMemcpy(out.data(), d_o.p, n * sizeof(A), hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__)) rc = ZKG_OK;
    d_s.release(); d_o.release();
    return rc;
}
template <class A, class FN>
int batch_points(FN fixed_base_fn, const A &base, const std::vector<Fr> &scalars, std::vector<A> &out) { return batch_points(fixed_base_fn, base, Scalars(scalars), out); }

// the same batch with its result left on the device; `uploaded` counts the scalars that came from host memory
template <class A, class FN>
int batch_points_dev(FN fixed_base_fn, const A &base, const Scalars &scalars, DevBuf &d_out, size_t &uploaded) {
    const size_t n = scalars.size();
    if (d_out.reserve(n * sizeof(A) + 16)) return ZKG_ERROR;
    if (!n) return ZKG_OK;
    if (!scalars.host) return fixed_base_fn(base, reinterpret_cast<const uint32_t *>(scalars.dev), n, d_out.as<A>(), nullptr, true);
    ScopedDevBuf d_s;
    if (d_s.reserve(n * 32) || !hip_ok(hipMemcpy(d_s.p, scalars.host->data(), n * 32, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__)) return ZKG_ERROR;
    uploaded += n;
    return fixed_base_fn(base, d_s.as<uint32_t>(), n, d_out.as<A>(), nullptr, true);
}

G1Affine g1_generator() { return {Fq::from_u64(1), Fq::from_u64(2)}; }
G2Affine g2_generator() {
    auto limbs = [](std::initializer_list<uint32_t> l) { Fq x; int i = 0; for (uint32_t v : l) x.v[i++] = v; return x; };
    return {{limbs({0x02bc2026u, 0x8e83b5d1u, 0x497b0172u, 0xdceb1935u, 0x97811adfu, 0xfbb82647u, 0xaf96503bu, 0x19573841u}),
             limbs({0xa84c6140u, 0xafb4737du, 0x5802d8c4u, 0x6043dd5au, 0x52a02f86u, 0x09e950fcu, 0x3aea7b6bu, 0x14fef083u})},
            {limbs({0x886be9f6u, 0x619dfa9du, 0xf59e9b78u, 0xfe7fd297u, 0x231b7dfeu, 0xff9e1a62u, 0xae9e4206u, 0x28fd7eebu}),
             limbs({0xc71856eeu, 0x64095b56u, 0x327d3cbbu, 0xdc57f922u, 0x33351076u, 0x55f935beu, 0x93fd6482u, 0x0da4a0e6u})}};
}
void fr_limbs(const Fr &x, uint32_t out[8]) { Fr c = x.from_mont(); memcpy(out, c.v, 32); }

// zkg_groth16_setup_dev: out[j] = (beta At[j] + alpha Bt[j] + Ct[j]) * (j <= l ? 1 / gamma : 1 / delta) over At | Bt | Ct, `stride` elements
// apart — the IC scalars, then the L query's, back to back
__global__ __launch_bounds__(256) void k_setup_abc_scalars(const Fr *abc, size_t stride, size_t cols, uint32_t l, Fr alpha, Fr beta, Fr ginv, Fr dinv, Fr *out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    const Fr v = beta * abc[j] + alpha * abc[stride + j] + abc[2 * stride + j];
    out[j] = (v * (j <= l ? ginv : dinv)).normalized();
}

// ---- the ordered non-zero index of an Fr vector (the B query's entries that are not the point at infinity): three dependent launches and
//      no wait between workgroups.  One element per thread: a wavefront takes NZ_WAVE elements and counts them with one ballot, a workgroup
//      takes NZ_BLOCK; k_nonzero_count leaves one count per workgroup, k_nonzero_scan — ONE workgroup that walks all the counts NZ_SCAN at a
//      time with a running carry, so the scan has no levels — turns them into offsets and the total, k_nonzero_scatter takes the ballots
//      again and writes each position at offset + waves before + lanes before.  Zero is the lazy layer's: 0 or r, nothing normalised.
constexpr unsigned NZ_WAVE = 64, NZ_BLOCK = 256, NZ_SCAN = 1024;
constexpr size_t NZ_MAX = (size_t)1 << 28;
__global__ __launch_bounds__(NZ_BLOCK) void k_nonzero_count(const Fr *v, size_t n, uint32_t *block_count) {
    __shared__ uint32_t wcnt[NZ_BLOCK / NZ_WAVE];
    const size_t i = (size_t)blockIdx.x * NZ_BLOCK + threadIdx.x;
    const bool nz = i < n && !v[i].is_zero();
    const unsigned long long mask = __ballot(nz);
    if ((threadIdx.x & (NZ_WAVE - 1)) == 0) wcnt[threadIdx.x / NZ_WAVE] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t c = 0; for (unsigned w = 0; w < NZ_BLOCK / NZ_WAVE; ++w) c += wcnt[w]; block_count[blockIdx.x] = c; }
}
__global__ __launch_bounds__(NZ_SCAN) void k_nonzero_scan(uint32_t *block_count, size_t nblocks, uint32_t *total) {   // counts -> exclusive offsets, in place
    __shared__ uint32_t wsum[NZ_SCAN / NZ_WAVE];
    const unsigned lane = threadIdx.x & (NZ_WAVE - 1), wave = threadIdx.x / NZ_WAVE;
    uint32_t carry = 0;
    for (size_t base = 0; base < nblocks; base += NZ_SCAN) {               // (the trip count is the same for every thread)
        const size_t i = base + threadIdx.x;
        const uint32_t c = i < nblocks ? block_count[i] : 0;
        uint32_t incl = c;
        for (unsigned d = 1; d < NZ_WAVE; d <<= 1) { const uint32_t up = __shfl_up(incl, d, NZ_WAVE); if (lane >= d) incl += up; }
        if (lane == NZ_WAVE - 1) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (unsigned w = 0; w < NZ_SCAN / NZ_WAVE; ++w) { const uint32_t s = wsum[w]; if (w < wave) before += s; all += s; }
        if (i < nblocks) block_count[i] = carry + before + incl - c;
        carry += all;
        __syncthreads();                                                   // wsum is written again by the next round
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(NZ_BLOCK) void k_nonzero_scatter(const Fr *v, size_t n, const uint32_t *block_offset, uint32_t *idx) {
    __shared__ uint32_t wcnt[NZ_BLOCK / NZ_WAVE];
    const size_t i = (size_t)blockIdx.x * NZ_BLOCK + threadIdx.x;
    const unsigned lane = threadIdx.x & (NZ_WAVE - 1), wave = threadIdx.x / NZ_WAVE;
    const bool nz = i < n && !v[i].is_zero();
    const unsigned long long mask = __ballot(nz);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (!nz) return;
    uint32_t at = block_offset[blockIdx.x] + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
    for (unsigned w = 0; w < wave; ++w) at += wcnt[w];
    idx[at] = (uint32_t)i;                                                  // at < the total <= n: idx holds n entries
}
// d_idx: n entries; d_count: one word; d_blocks: nonzero_index_blocks(n) words of workspace.  Queued on s, nothing waits.
size_t nonzero_index_blocks(size_t n) { return (n + NZ_BLOCK - 1) / NZ_BLOCK; }
int nonzero_index_dev(const Fr *d_v, size_t n, uint32_t *d_idx, uint32_t *d_count, uint32_t *d_blocks, hipStream_t s) {
    if (n > NZ_MAX) { set_error("nonzero index: more than 2^28 elements"); return ZKG_ERROR; }
    if (!n) { ZK_HIP(hipMemsetAsync(d_count, 0, 4, s)); return ZKG_OK; }
    const unsigned nblocks = (unsigned)nonzero_index_blocks(n);
    hipLaunchKernelGGL(k_nonzero_count, dim3(nblocks), dim3(NZ_BLOCK), 0, s, d_v, n, d_blocks);
    hipLaunchKernelGGL(k_nonzero_scan, dim3(1), dim3(NZ_SCAN), 0, s, d_blocks, (size_t)nblocks, d_count);
    hipLaunchKernelGGL(k_nonzero_scatter, dim3(nblocks), dim3(NZ_BLOCK), 0, s, d_v, n, (const uint32_t *)d_blocks, d_idx);
    if (hipGetLastError() != hipSuccess) { set_error("nonzero index: kernel launch failed"); return ZKG_ERROR; }
    return ZKG_OK;
}
// what the last generator of this thread that leaves its key on the device did (zkg_setup_resident_stats)
thread_local size_t t_setup_resident_stats[3] = {0, 0, 0};

}  // namespace

extern "C" {

// The generator proper.  The constraint system comes either as the ABI's view (copied) or — `owned` — as CSR vectors the caller gives up
// (the seam's circuit: 100 MB at 20 payloads that would otherwise be copied and then freed twice); `under_gpu` runs on a thread of its own
// while the GPU turns the scalars into points (the seam destroys its circuit there).
// mode: where the scalars are computed and where the queries end up (Resident: setup_resident_core below).
// after_csr(kp) runs when the generator's host loops are done and its GPU phase
// begins (kp holds the constraint system it will store) — the seam starts writing the pk blob's constraint rows there; before_delete()
// runs before a failing generator deletes kp (whatever after_csr started must have let go of it).
enum class SetupMode { Host,          // zkg_groth16_setup: scalars from the host loops, the key in host vectors
                       DevScalars,    // zkg_groth16_setup_dev: every scalar computed on the device, the key in host vectors
                       Resident };    // zkg_groth16_setup_resident, the seam: every scalar computed on the device, the queries left there
static zkg_keypair *groth16_setup_impl(const zkg_r1cs *cs, const uint64_t *trapdoor, OwnedCsr *owned, const std::function<void()> &under_gpu, SetupMode mode = SetupMode::Host,
                                       const std::function<void(zkg_keypair *)> &after_csr = nullptr, const std::function<void()> &before_delete = nullptr) {
    const bool dev_scalars = mode != SetupMode::Host, keep_on_device = mode == SetupMode::Resident;
    if (!cs || (!owned && (!cs->a_rowptr || !cs->b_rowptr || !cs->c_rowptr))) { set_error("zkg_groth16_setup: null constraint system"); return nullptr; }
    zkg_keypair *kp = new zkg_keypair();
    static const bool dbg = getenv("ZKG_DEBUG_TIMING") != nullptr;
    auto t_begin = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) { if (dbg) fprintf(stderr, "[zkg setup] %-28s %8.3f ms\n", what, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count()); };
    kp->n = cs->num_variables; kp->l = cs->num_inputs; kp->C = cs->num_constraints;
    const size_t n = kp->n, l = kp->l, C = kp->C;
    if (owned) {
        for (int k = 0; k < 3; ++k) { kp->rp[k].swap(owned->rp[k]); kp->col[k].swap(owned->col[k]); kp->val[k].swap(owned->val[k]); }
        for (int k = 0; k < 3; ++k)
            if (kp->rp[k].size() != C + 1 || kp->col[k].size() != kp->rp[k][C] || kp->val[k].size() != 4 * kp->col[k].size()) { set_error("zkg_groth16_setup: inconsistent CSR"); delete kp; return nullptr; }
    } else {
        copy_csr(kp->rp[0], kp->col[0], kp->val[0], cs->a_rowptr, cs->a_col, cs->a_val, kp->C);
        copy_csr(kp->rp[1], kp->col[1], kp->val[1], cs->b_rowptr, cs->b_col, cs->b_val, kp->C);
        copy_csr(kp->rp[2], kp->col[2], kp->val[2], cs->c_rowptr, cs->c_col, cs->c_val, kp->C);
    }
    {   // swap_AB_if_beneficial: count the variables each of A and B touches
        std::vector<char> ta(n + 1, 0), tb(n + 1, 0);
        for (uint32_t c : kp->col[0]) ta[c] = 1;
        for (uint32_t c : kp->col[1]) tb[c] = 1;
        size_t na = 0, nb = 0;
        for (size_t i = 0; i <= n; ++i) { na += ta[i]; nb += tb[i]; }
        if (nb > na) { kp->rp[0].swap(kp->rp[1]); kp->col[0].swap(kp->col[1]); kp->val[0].swap(kp->val[1]); kp->swapped = true; }
    }
    auto drop = [&]() -> zkg_keypair * { if (before_delete) before_delete(); delete kp; return nullptr; };
    DomainShape shape;                                                     // libfqfft get_evaluation_domain(C + l + 1)
    if (!evaluation_domain_shape(C + l + 1, shape)) { set_error("zkg_groth16_setup: system too large for the 2-adicity of Fr"); return drop(); }
    const unsigned log_m = shape.log_m;
    kp->log_m = log_m; kp->m = shape.m;
    const size_t m = shape.m;
    Fr t, alpha, beta, gamma, delta;
    if (trapdoor) { t = fr_from_canonical(trapdoor); alpha = fr_from_canonical(trapdoor + 4); beta = fr_from_canonical(trapdoor + 8); gamma = fr_from_canonical(trapdoor + 12); delta = fr_from_canonical(trapdoor + 16); }
    else { t = random_fr(); alpha = random_fr(); beta = random_fr(); gamma = random_fr(); delta = random_fr(); }
    lap("copy + swap");
    std::vector<Fr> At, Bt, Ct, Hs, Ls, ICs;                               // the scalars on the host ...
    ScopedDevBuf d_scalars;                                                // ... or (dev_scalars) on the device: At | Bt | Ct | t^i Z(t) / delta | IC, L
    if (dev_scalars) {
        // ---- zkg_groth16_setup_dev: the instance map on a zkg_qap handle over the system as it is stored (swapped or not), H's scalars from
        //      powers_table, IC's and L's from one kernel — all queued on the null stream, where the fixed-base batches follow them
        zkg_r1cs view; memset(&view, 0, sizeof(view));
        view.num_variables = kp->n; view.num_inputs = kp->l; view.num_constraints = kp->C;
        view.a_rowptr = kp->rp[0].data(); view.a_col = kp->col[0].data(); view.a_val = kp->val[0].data();
        view.b_rowptr = kp->rp[1].data(); view.b_col = kp->col[1].data(); view.b_val = kp->val[1].data();
        view.c_rowptr = kp->rp[2].data(); view.c_col = kp->col[2].data(); view.c_val = kp->val[2].data();
        std::unique_ptr<zkg_qap, void (*)(zkg_qap *)> qap(zkg_qap_new(&view), zkg_qap_free);
        if (!qap) return drop();
        lap("qap handle");
        if (d_scalars.reserve((4 * (n + 1) + (m - 1)) * sizeof(Fr))) return drop();
        Fr *d_abc = d_scalars.as<Fr>(), *d_h = d_abc + 3 * (n + 1), *d_icl = d_h + (m - 1);
        if (zkg_qap_instance_async(qap.get(), reinterpret_cast<const uint64_t *>(t.v), d_abc, n + 1, nullptr, nullptr)) return drop();   // refuses a t on the domain
        const Fr dinv = delta.inverse(), ginv = gamma.inverse(), zd = domain_vanishing_at(shape, t) * dinv;
        if (powers_table(d_h, m - 1, t, zd, nullptr)) { set_error("zkg_groth16_setup_dev: kernel launch failed"); return drop(); }   // t^i Z(t) / delta
        hipLaunchKernelGGL(k_setup_abc_scalars, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, nullptr, (const Fr *)d_abc, n + 1, n + 1, (uint32_t)l, alpha, beta, ginv, dinv, d_icl);
        if (hipGetLastError() != hipSuccess) { set_error("zkg_groth16_setup_dev: kernel launch failed"); return drop(); }
        // the B query's non-zero list, behind the instance map on the same stream: n + 1 indices | their count | the scan's workspace
        if (keep_on_device) {
            if (kp->dBidx.reserve((n + 2 + nonzero_index_blocks(n + 1)) * 4 + 16)) return drop();
            uint32_t *d_idx = kp->dBidx.as<uint32_t>();
            if (nonzero_index_dev(d_abc + (n + 1), n + 1, d_idx, d_idx + (n + 1), d_idx + (n + 2), nullptr)) return drop();
        }
        if (dbg) (void)hipStreamSynchronize(nullptr);                      // the lap then holds the kernels, not their enqueue
        lap("qap instance + scalars (device)");
    } else {
    // ---- Lagrange coefficients u_i = L_i(t) and Z(t) on the chosen domain (closed forms, one batched inversion)
    Fr Zt; std::vector<Fr> u;
    if (domain_lagrange(shape, t, u, Zt)) return drop();
    lap("lagrange");
    // ---- QAP polynomials at t (r1cs_to_qap_instance_map_with_evaluation)
    At.assign(n + 1, Fr::zero()); Bt.assign(n + 1, Fr::zero()); Ct.assign(n + 1, Fr::zero());
    for (size_t i = 0; i <= l; ++i) At[i] = u[C + i];
    std::vector<Fr> *dst[3] = {&At, &Bt, &Ct};
    host_parallel_for(3, [&](int k) {                                       // the three matrices accumulate into separate vectors
        const Fr one = Fr::one(), minus_one = Fr::one().neg();               // a gadget circuit's coefficients are mostly +-1: no product needed
        for (size_t i = 0; i < C; ++i)
            for (uint32_t e = kp->rp[k][i]; e < kp->rp[k][i + 1]; ++e) {
                Fr c; memcpy(c.v, &kp->val[k][4 * (size_t)e], 32);
                Fr &acc = (*dst[k])[kp->col[k][e]];
                if (c == one) acc += u[i]; else if (c == minus_one) acc -= u[i]; else acc += u[i] * c;
            }
    });
    Fr dinv = delta.inverse(), ginv = gamma.inverse();
    Hs.resize(m - 1); Ls.resize(n - l); ICs.resize(l + 1);
    auto chunked = [&](size_t count, const std::function<void(size_t, size_t)> &f) {           // [0, count) in chunks on the host pool
        const int chunks = (int)std::min<size_t>(64, (count + 8191) / 8192);
        if (chunks <= 1) { f(0, count); return; }
        host_parallel_for(chunks, [&](int c) { f(count * (size_t)c / chunks, count * (size_t)(c + 1) / chunks); });
    };
    {
        const Fr zd = Zt * dinv;
        chunked(m - 1, [&](size_t lo, size_t hi) { Fr ti = t.pow_u64(lo) * zd; for (size_t i = lo; i < hi; ++i) { Hs[i] = ti; ti = ti * t; } });   // t^i Z(t) / delta
    }
    chunked(n + 1, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            Fr abc = beta * At[i] + alpha * Bt[i] + Ct[i];
            if (i <= l) ICs[i] = abc * ginv; else Ls[i - l - 1] = abc * dinv;
        }
    });
    lap("qap evaluation + scalars");
    }
    // one batch's scalars from either side: the host vector, or `count` elements at `offset` of the device buffer (the layout above)
    auto scalars_of = [&](const std::vector<Fr> &host, size_t offset, size_t count) { return dev_scalars ? Scalars(d_scalars.as<Fr>() + offset, count) : Scalars(host); };
    const size_t h_at = 3 * (n + 1), icl_at = h_at + (m - 1);
    const Scalars sAt = scalars_of(At, 0, n + 1), sBt = scalars_of(Bt, n + 1, n + 1), sHs = scalars_of(Hs, h_at, m - 1), sICs = scalars_of(ICs, icl_at, l + 1),
                  sLs = scalars_of(Ls, icl_at + l + 1, n - l);
    // ---- scalars -> points (GPU fixed-base batches).  The host pool is free from here on: what after_csr starts (the seam: the pk blob's
    //      constraint rows) shares it with nothing but the short page pre-faulting below (started earlier it made the Lagrange and QAP
    //      loops above run inline on this thread: 37 -> 90 ms)
    if (after_csr) after_csr(kp);
    std::thread side;
    if (under_gpu) side = std::thread([&] { try { under_gpu(); } catch (...) {} });
    struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } join_side{side};
    G1Affine g1 = g1_generator(); G2Affine g2 = g2_generator();
    std::vector<G1Affine> small1; std::vector<G2Affine> small2;
    // the result vectors (250 MB at 20 payloads) get their pages on the pool, side by side, instead of one after the other inside the batches
    static const bool no_prefault = getenv("ZKG_NO_PREFAULT") != nullptr;
    if (keep_on_device) {
        // the seam: ~4n + m points computed into device buffers and left there; only the 8 key elements and the l + 1 points of the
        // verification key come back
        kp->on_device = true;
        size_t uploaded = 0;
        const bool okd = batch_points<G1Affine>(fixed_base_g1, g1, {alpha, beta, delta}, small1) == 0 && batch_points<G2Affine>(fixed_base_g2, g2, {beta, delta, gamma}, small2) == 0 &&
                         batch_points_dev<G1Affine>(fixed_base_g1, g1, sAt, kp->dA, uploaded) == 0 && batch_points_dev<G1Affine>(fixed_base_g1, g1, sBt, kp->dB1, uploaded) == 0 &&
                         batch_points_dev<G2Affine>(fixed_base_g2, g2, sBt, kp->dB2, uploaded) == 0 && batch_points_dev<G1Affine>(fixed_base_g1, g1, sHs, kp->dH, uploaded) == 0 &&
                         batch_points_dev<G1Affine>(fixed_base_g1, g1, sLs, kp->dL, uploaded) == 0 && batch_points<G1Affine>(fixed_base_g1, g1, sICs, kp->IC) == 0;
        if (!okd) return drop();
        // the B query's non-zero list (zero scalar <=> point at infinity): compress_kc_records reads it where k_nonzero_* left it, behind the
        // instance map and long finished by now; the blob's decimal text needs it on the host — its count and its entries come back here,
        // after the batches, so that this copy, the one host wait the device scalars cost, never holds the GPU's queue up
        const uint32_t *d_idx = kp->dBidx.as<uint32_t>();
        uint32_t count = 0;
        if (!hip_ok(hipMemcpy(&count, d_idx + (n + 1), 4, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__)) return drop();
        if (count > n + 1) { set_error("zkg_groth16_setup_resident: non-zero count above n + 1"); return drop(); }
        kp->b_idx.resize(count);
        if (count && !hip_ok(hipMemcpy(kp->b_idx.data(), d_idx, (size_t)count * 4, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__)) return drop();
        t_setup_resident_stats[0] = 1; t_setup_resident_stats[1] = count; t_setup_resident_stats[2] = uploaded;
    } else {
    if (!no_prefault) host_parallel_for(5, [&](int i) {
        if (i == 0) kp->B_g2.resize(sBt.size()); else if (i == 1) kp->A_query.resize(sAt.size()); else if (i == 2) kp->B_g1.resize(sBt.size());
        else if (i == 3) kp->H_query.resize(sHs.size()); else kp->L_query.resize(sLs.size());
    });
    bool ok = batch_points<G1Affine>(fixed_base_g1, g1, {alpha, beta, delta}, small1) == 0 && batch_points<G2Affine>(fixed_base_g2, g2, {beta, delta, gamma}, small2) == 0 &&
              batch_points<G1Affine>(fixed_base_g1, g1, sAt, kp->A_query) == 0 && batch_points<G1Affine>(fixed_base_g1, g1, sBt, kp->B_g1) == 0 &&
              batch_points<G2Affine>(fixed_base_g2, g2, sBt, kp->B_g2) == 0 && batch_points<G1Affine>(fixed_base_g1, g1, sHs, kp->H_query) == 0 &&
              batch_points<G1Affine>(fixed_base_g1, g1, sLs, kp->L_query) == 0 && batch_points<G1Affine>(fixed_base_g1, g1, sICs, kp->IC) == 0;
    if (!ok) return drop();
    }
    kp->alpha_g1 = small1[0]; kp->beta_g1 = small1[1]; kp->delta_g1 = small1[2];
    kp->beta_g2 = small2[0]; kp->delta_g2 = small2[1]; kp->gamma_g2 = small2[2];
    lap("fixed-base batches (GPU)");
    kp->alpha_beta = pairing::reduced_pairing(kp->alpha_g1, kp->beta_g2);
    lap("pairing");
    zkg_pk &v = kp->pk_view; memset(&v, 0, sizeof(v));
    v.cs.num_variables = kp->n; v.cs.num_inputs = kp->l; v.cs.num_constraints = kp->C;
    v.cs.a_rowptr = kp->rp[0].data(); v.cs.a_col = kp->col[0].data(); v.cs.a_val = kp->val[0].data();
    v.cs.b_rowptr = kp->rp[1].data(); v.cs.b_col = kp->col[1].data(); v.cs.b_val = kp->val[1].data();
    v.cs.c_rowptr = kp->rp[2].data(); v.cs.c_col = kp->col[2].data(); v.cs.c_val = kp->val[2].data();
    v.log_m = log_m; v.domain_size = (uint32_t)m;
    v.alpha_g1 = (const uint64_t *)&kp->alpha_g1; v.beta_g1 = (const uint64_t *)&kp->beta_g1; v.delta_g1 = (const uint64_t *)&kp->delta_g1;
    v.beta_g2 = (const uint64_t *)&kp->beta_g2; v.delta_g2 = (const uint64_t *)&kp->delta_g2;
    v.A_query = (const uint64_t *)kp->A_query.data(); v.B_g1 = (const uint64_t *)kp->B_g1.data(); v.B_g2 = (const uint64_t *)kp->B_g2.data();
    v.H_query = (const uint64_t *)kp->H_query.data(); v.L_query = (const uint64_t *)kp->L_query.data();
    if (kp->on_device) {                                                         // DEVICE pointers: for crs_upload_device_queries only
        v.A_query = kp->dA.as<uint64_t>(); v.B_g1 = kp->dB1.as<uint64_t>(); v.B_g2 = kp->dB2.as<uint64_t>(); v.H_query = kp->dH.as<uint64_t>(); v.L_query = kp->dL.as<uint64_t>();
    }
    return kp;
}
zkg_keypair *zkg_groth16_setup(const zkg_r1cs *cs, const uint64_t *trapdoor /* 5 x 4 canonical limbs: t, alpha, beta, gamma, delta; NULL = random */) {
    return groth16_setup_impl(cs, trapdoor, nullptr, nullptr);
}
// the same keypair with every scalar computed on the device (zkg_qap_instance_async, powers_table, k_setup_abc_scalars): no scalar vector on the host
zkg_keypair *zkg_groth16_setup_dev(const zkg_r1cs *cs, const uint64_t *trapdoor) {
    return c_boundary<zkg_keypair *>("zkg_groth16_setup_dev", nullptr, [&]() -> zkg_keypair * {
        if (initialised_device() < 0) { set_error("zkg_init not called"); return nullptr; }
        return groth16_setup_impl(cs, trapdoor, nullptr, nullptr, SetupMode::DevScalars);
    });
}

void zkg_keypair_free(zkg_keypair *kp) { delete kp; }
const zkg_pk *zkg_keypair_pk(const zkg_keypair *kp) { return kp && !kp->on_device ? &kp->pk_view : nullptr; }
int zkg_keypair_swapped(const zkg_keypair *kp) { return kp && kp->swapped ? 1 : 0; }

// operator<<(r1cs_gg_ppzksnark_proving_key), layout in codec.hip.  Built once per keypair (callers ask for the size first, then for
// the bytes); the fixed-size point records — 2.2 M of them at 20 payloads — are serialised on the host pool.
// the constraint rows of a pk blob (per row: a, b, c as #terms '\n' (index '\n' coefficient)*), in chunks written on the host pool
static void constraint_rows_text(const zkg_keypair *kp, std::vector<ser::Writer> &part) {
    const int chunks = (int)std::min<size_t>(64, ((size_t)kp->C + 4095) / 4096);
    part.assign(std::max(chunks, 1), ser::Writer());
    auto rows = [&](int ch) {
        ser::Writer &pw = part[ch];
        const uint32_t lo = (uint32_t)((size_t)kp->C * ch / std::max(chunks, 1)), hi = (uint32_t)((size_t)kp->C * (ch + 1) / std::max(chunks, 1));
        size_t terms = 0;
        for (int k = 0; k < 3; ++k) terms += kp->rp[k][hi] - kp->rp[k][lo];
        pw.buf.reserve(terms * 40 + (size_t)(hi - lo) * 8 + 64);
        for (uint32_t c = lo; c < hi; ++c)
            for (int k = 0; k < 3; ++k) {
                pw.dec(kp->rp[k][c + 1] - kp->rp[k][c]);
                for (uint32_t e = kp->rp[k][c]; e < kp->rp[k][c + 1]; ++e) { pw.dec(kp->col[k][e]); pw.raw(&kp->val[k][4 * (size_t)e], 32); }
            }
    };
    if (chunks <= 1) rows(0); else host_parallel_for(chunks, rows);
}
static void build_pk_blob(const zkg_keypair *kp, ser::Bytes &buf) {
    ser::Writer w;
    std::vector<size_t> idx;
    for (size_t i = 0; i < kp->B_g2.size(); ++i) if (!kp->B_g2[i].is_inf() || !kp->B_g1[i].is_inf()) idx.push_back(i);
    const size_t nterms = kp->col[0].size() + kp->col[1].size() + kp->col[2].size();
    w.buf.reserve((kp->A_query.size() + kp->H_query.size() + kp->L_query.size()) * 34 + idx.size() * 108 + nterms * 40 + (size_t)kp->C * 8 + 4096);
    // a run of fixed-size records: reserve the bytes, fill them in parallel
    auto records = [&](size_t count, size_t rec, const std::function<void(size_t, uint8_t *)> &put) {
        const size_t at = w.buf.size();
        w.buf.resize(at + count * rec);
        uint8_t *base = w.buf.data() + at;
        const int chunks = (int)std::min<size_t>(64, (count + 4095) / 4096);
        host_parallel_for(chunks, [&](int c) {
            size_t lo = count * (size_t)c / chunks, hi = count * (size_t)(c + 1) / chunks;
            for (size_t i = lo; i < hi; ++i) put(i, base + i * rec);
        });
    };
    w.g1(kp->alpha_g1); w.g1(kp->beta_g1); w.g2(kp->beta_g2); w.g1(kp->delta_g1); w.g2(kp->delta_g2);
    w.dec(kp->A_query.size()); records(kp->A_query.size(), 34, [&](size_t i, uint8_t *o) { ser::put_g1(o, kp->A_query[i]); });
    w.dec(kp->B_g2.size()); w.dec(idx.size()); for (size_t i : idx) w.dec(i);
    w.dec(idx.size()); records(idx.size(), 100, [&](size_t j, uint8_t *o) { ser::put_g2(o, kp->B_g2[idx[j]]); ser::put_g1(o + 66, kp->B_g1[idx[j]]); });
    w.dec(kp->H_query.size()); records(kp->H_query.size(), 34, [&](size_t i, uint8_t *o) { ser::put_g1(o, kp->H_query[i]); });
    w.dec(kp->L_query.size()); records(kp->L_query.size(), 34, [&](size_t i, uint8_t *o) { ser::put_g1(o, kp->L_query[i]); });
    w.dec(kp->l); w.dec(kp->n - kp->l); w.dec(kp->C);
    {   // the constraint system: variable-length records (decimal counts and indices), so each chunk of rows is written to a buffer of its
        // own on the pool and the buffers are then copied into place, also in parallel
        std::vector<ser::Writer> part;
        constraint_rows_text(kp, part);
        std::vector<size_t> at(part.size() + 1, w.buf.size());
        for (size_t i = 0; i < part.size(); ++i) at[i + 1] = at[i] + part[i].buf.size();
        w.buf.resize(at.back());
        host_parallel_for((int)part.size(), [&](int i) { if (!part[i].buf.empty()) memcpy(w.buf.data() + at[i], part[i].buf.data(), part[i].buf.size()); });
    }
    buf.swap(w.buf);
}
size_t zkg_keypair_pk_blob(const zkg_keypair *kp_, uint8_t *out, size_t cap) {
    zkg_keypair *kp = const_cast<zkg_keypair *>(kp_);
    if (!kp || kp->on_device) return 0;
    std::lock_guard<std::mutex> lk(kp->blob_mu);
    if (kp->pk_blob.empty()) build_pk_blob(kp, kp->pk_blob);
    if (out && cap >= kp->pk_blob.size()) {                                   // hundreds of MB into fresh pages: copy in parallel pieces
        const size_t len = kp->pk_blob.size(); const int chunks = (int)std::min<size_t>(32, (len >> 22) + 1);
        host_parallel_for(chunks, [&](int c) { size_t lo = len * (size_t)c / chunks, hi = len * (size_t)(c + 1) / chunks; memcpy(out + lo, kp->pk_blob.data() + lo, hi - lo); });
    }
    return kp->pk_blob.size();
}

// operator<<(r1cs_gg_ppzksnark_verification_key): alpha_g1_beta_g2 (GT, 384 B) | gamma_g2 | delta_g2 | gamma_ABC_g1 as an
// accumulation_vector: first (G1) then a sparse vector: domain '\n' #indices '\n' (index '\n')* #values '\n' (G1)*
size_t zkg_keypair_vk_blob(const zkg_keypair *kp, uint8_t *out, size_t cap) {
    if (!kp) return 0;
    ser::Writer w;
    uint8_t gt[384]; ser::put_fq12(gt, kp->alpha_beta); w.raw(gt, 384);
    w.g2(kp->gamma_g2); w.g2(kp->delta_g2);
    w.g1(kp->IC[0]);
    size_t rest = kp->IC.size() - 1;
    w.dec(rest); w.dec(rest); for (size_t i = 0; i < rest; ++i) w.dec(i);
    w.dec(rest); for (size_t i = 0; i < rest; ++i) w.g1(kp->IC[i + 1]);
    if (out && cap >= w.buf.size()) memcpy(out, w.buf.data(), w.buf.size());
    return w.buf.size();
}

// r1cs_gg_ppzksnark_verifier_strong_IC: 0 = proof valid, 1 = invalid (libsnark_verify returns !valid, libsnark_wrapper.cpp:269),
// 2 = malformed key / proof.  primary_input: n_inputs x 4 limbs, Montgomery Fr.
// What a verification key contributes to every verification, computed once per key: its points decompressed (one square root each —
// l + 3 of them) and every line of the Miller loops of gamma_g2 and delta_g2 (libsnark's r1cs_gg_ppzksnark_processed_verification_key;
// the reference's libsnark_verify re-parses and re-processes ctx->vk on every call, libsnark_wrapper.cpp:252-276).  Kept per vk blob —
// found by a 64-bit digest, confirmed byte for byte — for the last few keys.
struct PreparedVk {
    std::vector<uint8_t> blob;
    Fq12 alpha_beta; G2Affine gamma_g2, delta_g2; G1Affine ic0; size_t domain = 0;
    std::vector<size_t> idx; std::vector<G1Affine> ic;                          // gamma_ABC: indices and decompressed values
    std::vector<pairing::LineCoeff> gamma_lines, delta_lines;                   // empty when the point is infinity
    mutable std::once_flag batch_once; mutable bool batchable = false;          // vk_batchable, computed on the first batch call that meets the key
    // the key's bit table on the device (verify.hip, k_zklaim_ic_each), built by the first zkg_zklaim_verify_each that meets the key; it
    // lives as long as the cache entry and whatever call still holds the key, and goes in zkg_shutdown with the cache (verify_keys_release_all)
    mutable std::once_flag bits_once; mutable DevBuf bits; mutable int bits_device = -1; mutable bool bits_ok = false;
    PreparedVk() = default;
    PreparedVk(const PreparedVk &) = delete;
    PreparedVk &operator=(const PreparedVk &) = delete;
    ~PreparedVk() { bits.release(); }
};
static int prepare_vk(const uint8_t *vk_blob, size_t vk_len, PreparedVk &v) {   // 0, or 2 = malformed (message set)
    ser::Reader rd{vk_blob, vk_blob + vk_len};
    const uint8_t *gt = rd.take(384), *pg = rd.take(66), *pd = rd.take(66), *p0 = rd.take(34);
    if (!rd.ok) { set_error("vk blob truncated"); return 2; }
    ser::get_fq12(gt, v.alpha_beta);
    if (!ser::get_g2(pg, v.gamma_g2) || !ser::get_g2(pd, v.delta_g2) || !ser::get_g1(p0, v.ic0)) { set_error("vk blob: bad point"); return 2; }
    size_t domain = rd.dec(), nidx = rd.dec();
    // counts are bounded by the bytes that can still follow (an index takes >= 2 bytes, a value 34) before anything is sized by them
    if (!rd.ok || nidx > domain || nidx > (size_t)(rd.end - rd.p) / 2) { set_error("vk blob: bad gamma_ABC header"); return 2; }
    v.domain = domain; v.idx.resize(nidx);
    for (auto &i : v.idx) { i = rd.dec(); if (!rd.ok || i >= domain) { set_error("vk blob: bad index"); return 2; } }
    size_t nval = rd.dec();
    if (!rd.ok || nval != nidx || nval > (size_t)(rd.end - rd.p) / 34) { set_error("vk blob: bad gamma_ABC values"); return 2; }
    const uint8_t *vals = rd.take(nval * 34);
    if (!rd.ok) { set_error("vk blob: truncated gamma_ABC values"); return 2; }
    v.ic.resize(nidx);
    std::vector<char> bad(nidx, 0);
    host_parallel_for((int)nidx, [&](int k) { if (!ser::get_g1(vals + 34 * (size_t)k, v.ic[k])) bad[k] = 1; });
    for (char b : bad) if (b) { set_error("vk blob: bad gamma_ABC point"); return 2; }
    if (!v.gamma_g2.is_inf()) v.gamma_lines = pairing::miller_lines(v.gamma_g2);
    if (!v.delta_g2.is_inf()) v.delta_lines = pairing::miller_lines(v.delta_g2);
    v.blob.assign(vk_blob, vk_blob + vk_len);
    return 0;
}
static std::mutex g_vk_mu;
static std::map<uint64_t, std::shared_ptr<const PreparedVk>> g_vk_cache;
static uint64_t vk_digest(const uint8_t *p, size_t n) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ n; size_t i = 0;
    for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, p + i, 8); h = (h ^ w) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    for (; i < n; ++i) { h = (h ^ p[i]) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    return h;
}
static std::shared_ptr<const PreparedVk> prepared_vk(const uint8_t *vk_blob, size_t vk_len, int &rc) {
    const uint64_t key = vk_digest(vk_blob, vk_len);
    {
        std::lock_guard<std::mutex> lk(g_vk_mu);
        auto it = g_vk_cache.find(key);
        if (it != g_vk_cache.end() && it->second->blob.size() == vk_len && memcmp(it->second->blob.data(), vk_blob, vk_len) == 0) { rc = 0; return it->second; }
    }
    auto v = std::make_shared<PreparedVk>();
    rc = prepare_vk(vk_blob, vk_len, *v);
    if (rc) return nullptr;
    std::lock_guard<std::mutex> lk(g_vk_mu);
    if (g_vk_cache.size() >= 8) g_vk_cache.clear();
    g_vk_cache[key] = v;
    return v;
}
}  // extern "C"
// zkg_shutdown: the cached keys go, and their bit tables with them, while the device is still there
void zk::verify_keys_release_all() {
    std::lock_guard<std::mutex> lk(g_vk_mu);
    g_vk_cache.clear();
}
extern "C" {

// sum_k x_k * IC_k over the key's gamma_ABC entries (Montgomery scalars x_k from scalar_of(k, x)), in up to 16 chunks on the host pool.
// A chunk shares its doublings (Straus, one bit at a time: 254 doublings and on average 127 mixed additions per point instead of a
// double-and-add per point): 0.67 -> 0.3 ms at 20 payloads' 102 inputs.
static G1 ic_combination(const PreparedVk &vk, const std::function<void(size_t, Fr &)> &scalar_of) {
    const size_t nidx = vk.idx.size();
    const int chunks = (int)std::min<size_t>(16, nidx);
    std::vector<G1> part(std::max(chunks, 1), G1::inf());
    host_parallel_for(chunks, [&](int c) {
        const size_t lo = nidx * (size_t)c / chunks, hi = nidx * (size_t)(c + 1) / chunks, cnt = hi - lo;
        std::vector<uint32_t> e(8 * cnt);
        for (size_t k = lo; k < hi; ++k) { Fr x; scalar_of(k, x); fr_limbs(x, &e[8 * (k - lo)]); }
        const G1Affine *pt = vk.ic.data() + lo;
        G1 a = G1::inf();
        for (int bit = 255; bit >= 0; --bit) {
            a = a.dbl();
            for (size_t j = 0; j < cnt; ++j) if ((e[8 * j + (bit >> 5)] >> (bit & 31)) & 1u) a.madd(pt[j]);
        }
        part[c] = a;
    });
    G1 acc = G1::inf();
    for (int c = 0; c < chunks; ++c) acc.add(part[c]);
    return acc;
}

static int groth16_verify_impl(const uint8_t *vk_blob, size_t vk_len, const uint64_t *primary_input, size_t n_inputs, const uint8_t *proof, size_t proof_len) {
    if (!vk_blob || !proof || (n_inputs && !primary_input)) { set_error("zkg_groth16_verify: null argument"); return 2; }
    int rc = 0;
    const std::shared_ptr<const PreparedVk> vk = prepared_vk(vk_blob, vk_len, rc);
    if (!vk) return rc;
    if (vk->domain != n_inputs) return 1;                                       // strong input consistency: sizes must agree
    if (proof_len != ZKG_PROOF_BYTES) return 1;
    G1Affine pA, pC; G2Affine pB;
    if (!ser::get_g1(proof, pA) || !ser::get_g2(proof + 34, pB) || !ser::get_g1(proof + 100, pC)) return 1;     // is_well_formed
    // acc = IC_0 + sum_i input_i * IC_{i+1}
    G1 acc = G1::from_affine(vk->ic0);
    acc.add(ic_combination(*vk, [&](size_t k, Fr &x) { memcpy(x.v, primary_input + 4 * vk->idx[k], 32); }));
    // e(A, B) == e(alpha, beta) * e(acc, gamma) * e(C, delta)   <=>   FE( ML(A,B) * ML(-acc, gamma) * ML(-C, delta) ) == alpha_beta
    // (three loops in lock-step; the lines of gamma and delta come from the prepared key, only B's are computed here)
    G1Affine accA = acc.to_affine();
    std::vector<G1Affine> Ps; std::vector<G2Affine> Qs; std::vector<const std::vector<pairing::LineCoeff> *> prep;
    auto ml = [&](const G1Affine &P, const G2Affine &Q, const std::vector<pairing::LineCoeff> *lines) { if (!P.is_inf() && !Q.is_inf()) { Ps.push_back(P); Qs.push_back(Q); prep.push_back(lines); } };
    ml(pA, pB, nullptr); ml(accA.neg(), vk->gamma_g2, &vk->gamma_lines); ml(pC.neg(), vk->delta_g2, &vk->delta_lines);
    Fq12 f = Ps.empty() ? Fq12::one() : pairing::multi_miller_loop(Ps.data(), Qs.data(), (int)Ps.size(), prep.data());
    return pairing::final_exponentiation(f) == vk->alpha_beta ? 0 : 1;
}

int zkg_groth16_verify(const uint8_t *vk_blob, size_t vk_len, const uint64_t *primary_input, size_t n_inputs, const uint8_t *proof, size_t proof_len) {
    return c_boundary("zkg_groth16_verify", 2, [&] { return groth16_verify_impl(vk_blob, vk_len, primary_input, n_inputs, proof, proof_len); });
}

// ---- batch verification (zkg_groth16_verify_batch).  For the N proofs of one key, with fresh 128-bit weights r_i:
//   FE( prod_i ML(r_i A_i, B_i) * ML(-sum_i r_i acc_i, gamma) * ML(-sum_i r_i C_i, delta) ) == alpha_beta ^ (sum_i r_i),
//   sum_i r_i acc_i = (sum_i r_i) IC_0 + sum_j s_j IC_j,  s_j = sum_i r_i x_ij.
// The GPU (verify.hip) checks B_i in G2, computes r_i A_i and r_i C_i and the per-proof Miller values, and multiplies the Miller values of
// any index range; the host adds the r_i C_i, forms the s_j, runs the two Miller loops on the key's prepared lines, one final exponentiation
// and one GT power.  A failed range is halved until VERIFY_LEAF proofs or fewer are left, which zkg_groth16_verify's own code decides.
static constexpr size_t VERIFY_LEAF = 4;

static bool limbs_below(const uint32_t *x, const uint32_t *m) {            // x < m, 8 little-endian u32 limbs
    for (int i = 7; i >= 0; --i) if (x[i] != m[i]) return x[i] < m[i];
    return false;
}
static bool coords_canonical(const uint8_t *rec, int nfq) {                // the x coordinate's limbs of a compressed point are < q
    if (rec[0] == '1') return true;                                         // infinity: nothing else is read
    for (int k = 0; k < nfq; ++k) { uint32_t x[8]; memcpy(x, rec + 1 + 32 * k, 32); if (!limbs_below(x, FqParams::P)) return false; }
    return true;
}
// what the combination needs of a key beyond what the single verifier checks: gamma and delta in G2, alpha_beta of order r (then it lies
// in the cyclotomic subgroup, and alpha_beta^(sum r_i) can be taken with cyclotomic squarings)
static bool vk_limbs_canonical(const PreparedVk &vk) {
    auto canon = [](const Fq &x) { return limbs_below(x.v, FqParams::P); };  // the single verifier reads limbs >= q too; only canonical keys enter
    auto canon2 = [&](const Fq2 &x) { return canon(x.c0) && canon(x.c1); };
    for (const Fq6 *h : {&vk.alpha_beta.c0, &vk.alpha_beta.c1}) if (!canon2(h->c0) || !canon2(h->c1) || !canon2(h->c2)) return false;
    if (!canon2(vk.gamma_g2.x) || !canon2(vk.gamma_g2.y) || !canon2(vk.delta_g2.x) || !canon2(vk.delta_g2.y) || !canon(vk.ic0.x) || !canon(vk.ic0.y)) return false;
    for (const G1Affine &q : vk.ic) if (!canon(q.x) || !canon(q.y)) return false;
    return true;
}
static bool vk_batchable(const PreparedVk &vk) {
    const uint32_t *r = FrParams::P;
    if (!vk_limbs_canonical(vk)) return false;
    if (!G2::from_affine(vk.gamma_g2).mul(r, 8).is_inf() || !G2::from_affine(vk.delta_g2).mul(r, 8).is_inf()) return false;
    return vk.alpha_beta.pow(r, 8) == Fq12::one();
}

static bool vk_batchable_cached(const PreparedVk &vk) {
    std::call_once(vk.batch_once, [&] { vk.batchable = vk_batchable(vk); });
    return vk.batchable;
}

// 16 * n random bytes from the OS in as few requests as it allows (std::random_device on x86 issues one RDSEED per 32 bits: 4 per weight,
// ~0.1 ms per proof on a host whose cores share the RDSEED unit); std::random_device where getrandom is not available
static void draw_weights(uint32_t *w, size_t n) {
    uint8_t *p = reinterpret_cast<uint8_t *>(w);
    size_t left = 16 * n;
    while (left) {
        const ssize_t got = getrandom(p, left, 0);
        if (got <= 0) break;
        p += got; left -= (size_t)got;
    }
    if (left) { std::random_device rd; for (size_t i = 16 * n - left; i < 16 * n; i += 4) { uint32_t v = rd(); memcpy(reinterpret_cast<uint8_t *>(w) + i, &v, 4); } }
    for (size_t i = 0; i < n; ++i)                                              // nonzero weights (a zero draw has probability 2^-128)
        while (!(w[4 * i] | w[4 * i + 1] | w[4 * i + 2] | w[4 * i + 3])) { std::random_device rd; for (int j = 0; j < 4; ++j) w[4 * i + j] = rd(); }
}

// what the last zkg_groth16_verify_batch / zkg_zklaim_verify_batch call of this thread did (zkg_verify_batch_stats, zkg_zklaim_verify_batch_stats)
static thread_local size_t t_batch_stats[3] = {0, 0, 0};
static thread_local size_t t_seam_batch_stats[4] = {0, 0, 0, 0};

namespace {
struct BatchGroup {
    const uint8_t *blob; size_t len; uint64_t digest;
    std::shared_ptr<const PreparedVk> vk; bool batchable = false;
    std::vector<size_t> items;                                              // item indices, then the positions [lo, hi) of those that enter
    size_t lo = 0, hi = 0;
    uint32_t npl = 0; size_t pub_at = 0;                                    // the seam's device front end: payloads per item, where its records start
};
struct WorkspaceLease {                       // returned to the free list on every way out (after the call's streams are idle)
    VerifyWorkspace *w = nullptr;
    ~WorkspaceLease() { if (w) { (void)hipStreamSynchronize(w->s); (void)hipStreamSynchronize(w->s2); verify_workspace_release(w); } }
};
// ZKG_VERIFY_BATCH_LAPS=1: the host clock at the end of each stage, on stderr (where a batch's time goes)
struct BatchLaps {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::string line; size_t n;
    explicit BatchLaps(size_t count) : n(count) {}
    void operator()(const char *what) {
        static const bool laps = getenv("ZKG_VERIFY_BATCH_LAPS") && atoi(getenv("ZKG_VERIFY_BATCH_LAPS")) != 0;
        if (laps) line += std::string(" ") + what + "=" + std::to_string(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    ~BatchLaps() { if (!line.empty()) fprintf(stderr, "[verify_batch] n=%zu ms:%s\n", n, line.c_str()); }
};
struct BatchCounts { size_t combined = 0, alone = 0, outside_g2 = 0, from_device = 0; };
// where the core's arrays lie in a call's device workspace: N positions; o_flags: N bytes each of [B in G2 | B decoded | A decoded | C decoded
// | enters]; o_fe: the front end's own staging, directly behind the weights (o_w)
struct BatchLayout { uint8_t *d = nullptr; size_t N = 0, o_A = 0, o_C = 0, o_B = 0, o_w = 0, o_flags = 0, o_sums = 0, o_fe = 0; hipStream_t s = nullptr, s2 = nullptr; };

// What the batch core (verify_batch_core) asks of its caller: (a) the proofs' points, (b) the input sums, (c) the single verifier's arguments.
struct BatchFrontEnd {
    virtual ~BatchFrontEnd() = default;
    virtual bool on_device() const { return false; }                       // the points are decoded on the device, with a flag byte per position
    virtual size_t stage_bytes(size_t) const { return 0; }                 // device bytes behind the weights
    virtual size_t sum_elems() const { return 0; }                         // the most elements a key's sums have (device sums only)
    // (a) B of every position at d + o_B on s; then A, C and the weights (A and C back to back).  item_at[p]: the item at position p.
    virtual int stage_B(const BatchLayout &L, const std::vector<BatchGroup> &groups, const std::vector<size_t> &item_at, const uint32_t *w) = 0;
    virtual int stage_AC(const BatchLayout &L, const uint32_t *w) = 0;
    // (b) s_k = sum over positions p of [lo, hi) with in[p] of wm[p] * x_pk: sums_begin may start device work (in_dev: the mask on the device),
    // sums_ready waits for it, scalar_of(k) then gives the sum for the key's k-th gamma_ABC entry (called from the host pool)
    virtual int sums_begin(const BatchLayout &, const BatchGroup &, size_t, size_t) { return ZKG_OK; }
    virtual int sums_ready(const BatchLayout &) { return ZKG_OK; }
    virtual void scalar_of(const BatchGroup &G, const std::vector<size_t> &in, const std::vector<size_t> &item_at, const Fr *wm, size_t k, Fr &x) = 0;
    // (c) zkg_groth16_verify's own code on item i: 0 valid, 1 invalid, 2 malformed
    virtual int alone(size_t i) = 0;
};
}  // namespace

// steps 1 and 2 of a batch: group by the key's bytes; per key the prepared form (shared with zkg_groth16_verify's cache) and the checks
// the weights rely on, once per key.  blob_of(i, len): item i's key (null: the single verifier decides it).
// weights == false (zkg_groth16_verify_each draws none): only the canonical-limbs half of those checks.
static void batch_group_keys(size_t count, const std::function<const uint8_t *(size_t, size_t &)> &blob_of, std::vector<BatchGroup> &groups, std::vector<char> &own,
                             bool weights = true) {
    std::multimap<uint64_t, size_t> by_digest;
    for (size_t i = 0; i < count; ++i) {
        if (own[i]) continue;
        size_t len = 0;
        const uint8_t *blob = blob_of(i, len);
        if (!blob) { own[i] = 1; continue; }
        const uint64_t d = vk_digest(blob, len);
        size_t g = groups.size();
        for (auto r = by_digest.equal_range(d); r.first != r.second; ++r.first) {
            const BatchGroup &c = groups[r.first->second];
            if (c.len == len && memcmp(c.blob, blob, len) == 0) { g = r.first->second; break; }
        }
        if (g == groups.size()) { groups.push_back(BatchGroup{blob, len, d}); by_digest.emplace(d, g); }
        groups[g].items.push_back(i);
    }
    host_parallel_for((int)groups.size(), [&](int g) {
        BatchGroup &G = groups[g];
        try {
            int rc = 0;
            G.vk = prepared_vk(G.blob, G.len, rc);
            G.batchable = G.vk && (weights ? vk_batchable_cached(*G.vk) : vk_limbs_canonical(*G.vk));
        } catch (...) { G.vk = nullptr; G.batchable = false; }              // the single verifier decides these items (and meets the same failure)
    });
    for (const BatchGroup &G : groups) if (!G.batchable) for (size_t i : G.items) own[i] = 1;
}

// Steps 4 to 7 of a batch, shared by zkg_groth16_verify_batch (host front end) and zkg_zklaim_verify_batch (device front end): layout and
// weights, the GPU part, the combined check with bisection down to VERIFY_LEAF, the single verifier for whatever is left (own[i] != 0).
static int verify_batch_core(std::vector<BatchGroup> &groups, std::vector<char> &own, size_t count, BatchFrontEnd &fe, uint8_t *verdicts, BatchLaps &lap, BatchCounts &cnt) {
    // 4. layout: the entering proofs of each key at contiguous positions, a weight per position
    std::vector<size_t> item_at;
    for (BatchGroup &G : groups) {
        G.lo = item_at.size();
        for (size_t i : G.items) if (!own[i]) item_at.push_back(i);
        G.hi = item_at.size();
    }
    const size_t N = item_at.size();
    const bool dev = fe.on_device();
    std::vector<G1Affine> rC(N); std::vector<uint32_t> w(4 * N); std::vector<Fr> wm(N);
    draw_weights(w.data(), N);                                              // fresh on every call; no seed crosses the ABI
    for (size_t p = 0; p < N; ++p) { Fr x = Fr::zero(); memcpy(x.v, &w[4 * p], 16); wm[p] = x.to_mont(); }
    lap("weights");
    std::vector<uint8_t> flags((dev ? 4 : 1) * N, 1);                       // [B in G2 | B decoded | A decoded | C decoded]
    std::vector<uint8_t> in(N, 1);                                          // the position enters the sums
    std::vector<size_t> decide_alone;
    if (N) {
        // 5. the GPU part: B in G2 (second stream) beside r_i A_i and r_i C_i (one launch), then the Miller values
        const size_t ns = fe.sum_elems();
        const size_t o_A = 0, o_C = o_A + 64 * N, o_B = o_C + 64 * N, o_rA = o_B + 128 * N, o_rC = o_rA + 64 * N, o_M = o_rC + 64 * N,
                     o_part = o_M + 384 * N, o_out = o_part + 384 * VERIFY_PROD_BLOCKS, o_sums = o_out + 384, o_flags = o_sums + 32 * ns * (ZV_SUM_SLICES + 1),
                     o_w = (o_flags + 5 * N + 15) & ~(size_t)15, o_fe = o_w + 16 * N, total = o_fe + fe.stage_bytes(N) + 16;
        const size_t o_ok = o_flags, o_use = o_flags + 4 * N;
        WorkspaceLease lease;
        if (!(lease.w = verify_workspace_acquire()) || lease.w->buf.reserve(total)) return ZKG_ERROR;
        uint8_t *d = lease.w->buf.as<uint8_t>(); hipStream_t s = lease.w->s, s2 = lease.w->s2;
        BatchLayout L; L.d = d; L.N = N; L.o_A = o_A; L.o_C = o_C; L.o_B = o_B; L.o_w = o_w; L.o_flags = o_flags; L.o_sums = o_sums; L.o_fe = o_fe; L.s = s; L.s2 = s2;
        if (fe.stage_B(L, groups, item_at, w.data())) return ZKG_ERROR;
        ZK_HIP(hipEventRecord(lease.w->ev, s));
        ZK_HIP(hipStreamWaitEvent(s2, lease.w->ev, 0));
        if (verify_g2_subgroup((const G2Affine *)(d + o_B), N, d + o_ok, s2)) return ZKG_ERROR;
        ZK_HIP(hipEventRecord(lease.w->ev2, s2));
        if (fe.stage_AC(L, w.data())) return ZKG_ERROR;                     // A and C back to back: one launch for both
        if (verify_g1_mul128((const G1Affine *)(d + o_A), (const uint32_t *)(d + o_w), N, 2 * N, (G1Affine *)(d + o_rA), s)) return ZKG_ERROR;
        ZK_HIP(hipStreamWaitEvent(s, lease.w->ev2, 0));
        // a position whose points did not decode keeps its place with the Miller value 1, as one whose B is outside G2 does
        if (dev && verify_use_mask(N, d + o_ok, d + o_ok + N, d + o_ok + 2 * N, d + o_use, s)) return ZKG_ERROR;
        if (verify_miller((const G1Affine *)(d + o_rA), (const G2Affine *)(d + o_B), d + (dev ? o_use : o_ok), N, d + o_M, s)) return ZKG_ERROR;
        ZK_HIP(hipMemcpyAsync(flags.data(), d + o_ok, flags.size(), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipMemcpyAsync(rC.data(), d + o_rC, 64 * N, hipMemcpyDeviceToHost, s));
        lap("upload_launch");
        ZK_HIP(hipStreamSynchronize(s));
        lap("gpu");
        for (size_t p = 0; p < N; ++p) {                                    // its Miller value is 1: the ranges stay contiguous
            if (!flags[p]) ++cnt.outside_g2;
            in[p] = flags[p] && (!dev || (flags[N + p] && flags[2 * N + p] && flags[3 * N + p]));
            if (!in[p]) own[item_at[p]] = 1;
        }
        if (dev) cnt.from_device += N;
        // 6. one combined check per range; a failed range is halved
        auto combined = [&](const BatchGroup &G, size_t lo, size_t hi, bool &pass) -> int {
            Fq12 prod;
            if (verify_fq12_product(d + o_M, lo, hi, d + o_part, d + o_out, s)) return ZKG_ERROR;
            ZK_HIP(hipMemcpyAsync(&prod, d + o_out, 384, hipMemcpyDeviceToHost, s));
            if (fe.sums_begin(L, G, lo, hi)) return ZKG_ERROR;              // (beside the product, on the second stream)
            std::vector<size_t> inp;                                        // (the host work below runs while the product is computed)
            for (size_t p = lo; p < hi; ++p) if (in[p]) inp.push_back(p);
            Fr rsum = Fr::zero();
            for (size_t p : inp) rsum += wm[p];
            const int chunks = (int)std::min<size_t>(16, inp.size());
            std::vector<G1> part(std::max(chunks, 1), G1::inf());
            host_parallel_for(chunks, [&](int c) {
                G1 a = G1::inf();
                for (size_t t = inp.size() * c / chunks; t < inp.size() * (c + 1) / chunks; ++t) a.madd(rC[inp[t]]);
                part[c] = a;
            });
            G1 csum = G1::inf();
            for (const G1 &q : part) csum.add(q);
            const PreparedVk &vk = *G.vk;
            G1 acc = G1::from_affine(vk.ic0);
            { uint32_t e[8]; fr_limbs(rsum, e); acc = acc.mul(e, 8); }
            if (fe.sums_ready(L)) return ZKG_ERROR;
            acc.add(ic_combination(vk, [&](size_t k, Fr &x) { fe.scalar_of(G, inp, item_at, wm.data(), k, x); }));      // s_k = sum_i r_i x_ik
            std::vector<G1Affine> Ps; std::vector<G2Affine> Qs; std::vector<const std::vector<pairing::LineCoeff> *> prep;
            auto ml = [&](const G1Affine &P, const G2Affine &Q, const std::vector<pairing::LineCoeff> *lines) { if (!P.is_inf() && !Q.is_inf()) { Ps.push_back(P); Qs.push_back(Q); prep.push_back(lines); } };
            ml(acc.to_affine().neg(), vk.gamma_g2, &vk.gamma_lines); ml(csum.to_affine().neg(), vk.delta_g2, &vk.delta_lines);
            Fq12 f = Ps.empty() ? Fq12::one() : pairing::multi_miller_loop(Ps.data(), Qs.data(), (int)Ps.size(), prep.data());
            uint32_t e[8]; fr_limbs(rsum, e);
            const Fq12 rhs = vk.alpha_beta.cyclotomic_pow(e, 8);
            ZK_HIP(hipStreamSynchronize(s));
            pass = pairing::final_exponentiation(prod * f) == rhs;
            return ZKG_OK;
        };
        std::function<int(const BatchGroup &, size_t, size_t)> decide = [&](const BatchGroup &G, size_t lo, size_t hi) -> int {
            size_t n_in = 0;
            for (size_t p = lo; p < hi; ++p) n_in += in[p];
            if (!n_in) return ZKG_OK;
            bool pass = false;
            ++cnt.combined;
            if (int rc = combined(G, lo, hi, pass)) return rc;
            if (pass) { for (size_t p = lo; p < hi; ++p) if (in[p]) verdicts[item_at[p]] = 0; return ZKG_OK; }
            if (n_in <= VERIFY_LEAF) { for (size_t p = lo; p < hi; ++p) if (in[p]) own[item_at[p]] = 1; return ZKG_OK; }
            const size_t mid = lo + (hi - lo) / 2;
            if (int rc = decide(G, lo, mid)) return rc;
            return decide(G, mid, hi);
        };
        for (const BatchGroup &G : groups)
            if (G.hi > G.lo) if (int rc = decide(G, G.lo, G.hi)) return rc;
        lap("checks");
    }
    // 7. everything the combination did not decide: the single verifier's code, on the host pool
    for (size_t i = 0; i < count; ++i) if (own[i]) decide_alone.push_back(i);
    host_parallel_for((int)decide_alone.size(), [&](int t) {
        int v;
        try { v = fe.alone(decide_alone[t]); } catch (...) { v = 2; }
        verdicts[decide_alone[t]] = (uint8_t)v;
    });
    lap("alone");
    cnt.alone += decide_alone.size();
    return ZKG_OK;
}

namespace {
// the host front end: the caller's items, their points decoded on the host pool (step 3), the sums formed inside ic_combination's chunks
struct ItemFrontEnd : BatchFrontEnd {
    const zkg_verify_item *items; const G1Affine *hA, *hC; const G2Affine *hB;
    std::vector<G1Affine> pAC; std::vector<G2Affine> pB;
    ItemFrontEnd(const zkg_verify_item *it, const G1Affine *a, const G2Affine *b, const G1Affine *c) : items(it), hA(a), hC(c), hB(b) {}
    int stage_B(const BatchLayout &L, const std::vector<BatchGroup> &, const std::vector<size_t> &item_at, const uint32_t *) override {
        pAC.resize(2 * L.N); pB.resize(L.N);
        for (size_t p = 0; p < L.N; ++p) { pAC[p] = hA[item_at[p]]; pB[p] = hB[item_at[p]]; pAC[L.N + p] = hC[item_at[p]]; }
        ZK_HIP(hipMemcpyAsync(L.d + L.o_B, pB.data(), 128 * L.N, hipMemcpyHostToDevice, L.s));
        return ZKG_OK;
    }
    int stage_AC(const BatchLayout &L, const uint32_t *w) override {
        ZK_HIP(hipMemcpyAsync(L.d + L.o_A, pAC.data(), 64 * L.N, hipMemcpyHostToDevice, L.s));
        ZK_HIP(hipMemcpyAsync(L.d + L.o_C, pAC.data() + L.N, 64 * L.N, hipMemcpyHostToDevice, L.s));
        ZK_HIP(hipMemcpyAsync(L.d + L.o_w, w, 16 * L.N, hipMemcpyHostToDevice, L.s));
        return ZKG_OK;
    }
    void scalar_of(const BatchGroup &G, const std::vector<size_t> &in, const std::vector<size_t> &item_at, const Fr *wm, size_t k, Fr &x) override {
        Fr sk = Fr::zero();
        for (size_t p : in) { Fr xi; memcpy(xi.v, items[item_at[p]].primary_input + 4 * G.vk->idx[k], 32); sk += wm[p] * xi; }
        x = sk;
    }
    int alone(size_t i) override {
        const zkg_verify_item &it = items[i];
        return groth16_verify_impl(it.vk_blob, it.vk_len, it.primary_input, it.n_inputs, it.proof, it.proof_len);
    }
};
}  // namespace

// step 3 of a batch, per proof: sizes, encodings and inputs as the single verifier reads them; the proof's points decoded on the host pool.
// own[i] = 1 for every item that the single verifier's code has to decide.
static void decode_items(const zkg_verify_item *items, size_t count, const std::vector<BatchGroup> &groups, std::vector<char> &own,
                         std::vector<G1Affine> &hA, std::vector<G2Affine> &hB, std::vector<G1Affine> &hC) {
    std::vector<int> group_of(count, -1);
    for (size_t g = 0; g < groups.size(); ++g) for (size_t i : groups[g].items) group_of[i] = (int)g;
    host_parallel_for((int)std::min<size_t>(64, count), [&](int c) {
        for (size_t i = count * (size_t)c / std::min<size_t>(64, count); i < count * (size_t)(c + 1) / std::min<size_t>(64, count); ++i) {
            if (own[i]) continue;
            const zkg_verify_item &it = items[i];
            const BatchGroup &G = groups[group_of[i]];
            bool ok = it.proof && it.proof_len == ZKG_PROOF_BYTES && it.n_inputs == G.vk->domain && (!it.n_inputs || it.primary_input);
            for (size_t j = 0; ok && j < it.n_inputs; ++j) {
                uint32_t x[8]; memcpy(x, it.primary_input + 4 * j, 32);
                ok = limbs_below(x, FrParams::P);
            }
            ok = ok && coords_canonical(it.proof, 1) && coords_canonical(it.proof + 34, 2) && coords_canonical(it.proof + 100, 1) &&
                 ser::get_g1(it.proof, hA[i]) && ser::get_g2(it.proof + 34, hB[i]) && ser::get_g1(it.proof + 100, hC[i]);
            if (!ok) own[i] = 1;
        }
    });
}

// zkg_groth16_verify_batch without its thread's counters: what the entry and the seam's host leg share
static int verify_batch_items(const zkg_verify_item *items, size_t count, uint8_t *verdicts, BatchCounts &cnt) {
    BatchLaps lap(count);
    std::vector<char> own(count, 0);                                        // decided by the single verifier's code
    // 1, 2. group by the key's bytes; per key the prepared form and the checks the weights rely on
    std::vector<BatchGroup> groups;
    batch_group_keys(count, [&](size_t i, size_t &len) { len = items[i].vk_len; return items[i].vk_blob; }, groups, own);
    lap("keys");
    // 3. per proof: sizes, encodings, inputs, points
    std::vector<G1Affine> hA(count), hC(count); std::vector<G2Affine> hB(count);
    decode_items(items, count, groups, own, hA, hB, hC);
    lap("decode");
    ItemFrontEnd fe(items, hA.data(), hB.data(), hC.data());
    return verify_batch_core(groups, own, count, fe, verdicts, lap, cnt);
}

static int verify_batch_impl(const zkg_verify_item *items, size_t count, uint8_t *verdicts) {
    if (initialised_device() < 0) { set_error("zkg_groth16_verify_batch: zkg_init not called (no GPU: there is no CPU path)"); return ZKG_ERROR; }
    if (count && (!items || !verdicts)) { set_error("zkg_groth16_verify_batch: null argument"); return ZKG_ERROR; }
    t_batch_stats[0] = t_batch_stats[1] = t_batch_stats[2] = 0;
    if (!count) return ZKG_OK;
    BatchCounts cnt;
    if (int rc = verify_batch_items(items, count, verdicts, cnt)) return rc;
    t_batch_stats[0] = cnt.combined; t_batch_stats[1] = cnt.alone; t_batch_stats[2] = cnt.outside_g2;
    return ZKG_OK;
}

void zkg_verify_batch_stats(size_t out[3]) { if (out) for (int i = 0; i < 3; ++i) out[i] = t_batch_stats[i]; }

int zkg_groth16_verify_batch(const zkg_verify_item *items, size_t count, uint8_t *verdicts) {
    return c_boundary("zkg_groth16_verify_batch", ZKG_ERROR, [&] { return verify_batch_impl(items, count, verdicts); });
}

// ---- per-proof verification (zkg_groth16_verify_each).  Every item is decided by its own equation
//   FE( ML(A_i, B_i) * ML(-acc_i, gamma) * ML(-C_i, delta) ) == alpha_beta,   acc_i = IC_0 + sum_k x_ik IC_k,
// on the GPU, all items of a key side by side: k_ic_each forms -acc_i, k_miller runs over the 3 n pairs [A | -acc | -C] x [B | gamma.. | delta..],
// k_final_exp_check multiplies an item's three values, raises the product and compares it.  No weights are drawn, so nothing is asked of the
// key or of B beyond what the single verifier asks: a B outside G2, or a key whose gamma, delta or alpha_beta lie outside their groups, is
// decided here by the same field operations as on the host.  What the device does not take is what its arithmetic cannot read as the host's
// does: limbs >= q or >= r, and whatever the single verifier rejects before it computes (sizes, encodings, a malformed key).
// A key's points go up once per call; its positions are cut into rounds whose staging stays within VERIFY_EACH_STAGE_MAX.
static constexpr size_t VERIFY_EACH_STAGE_MAX = (size_t)64 << 20;
static std::atomic<size_t> g_each_chunk{0};                                 // zkg_verify_each_set_chunk: positions per round (0: by the staging limit)
static thread_local size_t t_each_stats[3] = {0, 0, 0};

static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
// positions per round of a key with nidx inputs; per position: P 3 x 64, Q 3 x 128, Miller values 3 x 384, inputs, slots, verdict
static size_t verify_each_round_positions(size_t nidx, size_t key_bytes) {
    if (const size_t forced = g_each_chunk.load()) return forced;
    const size_t per = 3 * 64 + 3 * 128 + 3 * 384 + 32 * nidx + verify_final_exp_ws_bytes(64) / 64 + 1;
    const size_t room = VERIFY_EACH_STAGE_MAX > key_bytes + 4096 ? VERIFY_EACH_STAGE_MAX - key_bytes - 4096 : 0;
    return std::max<size_t>(64, room / per / 64 * 64);
}

static int verify_each_impl(const zkg_verify_item *items, size_t count, uint8_t *verdicts) {
    if (initialised_device() < 0) { set_error("zkg_groth16_verify_each: zkg_init not called (no GPU: there is no CPU path)"); return ZKG_ERROR; }
    if (count && (!items || !verdicts)) { set_error("zkg_groth16_verify_each: null argument"); return ZKG_ERROR; }
    t_each_stats[0] = t_each_stats[1] = t_each_stats[2] = 0;
    if (!count) return ZKG_OK;
    std::vector<char> own(count, 0);                                        // decided by the single verifier's code
    std::vector<BatchGroup> groups;
    batch_group_keys(count, [&](size_t i, size_t &len) { len = items[i].vk_len; return items[i].vk_blob; }, groups, own, false);
    std::vector<G1Affine> hA(count), hC(count); std::vector<G2Affine> hB(count);
    decode_items(items, count, groups, own, hA, hB, hC);
    size_t on_device = 0, rounds = 0;
    WorkspaceLease lease;
    std::vector<G1Affine> pA, pC; std::vector<G2Affine> pB; std::vector<uint64_t> px; std::vector<uint8_t> v;
    for (const BatchGroup &G : groups) {
        std::vector<size_t> pos;
        for (size_t i : G.items) if (!own[i]) pos.push_back(i);
        if (pos.empty()) continue;
        const PreparedVk &vk = *G.vk;
        const size_t nidx = vk.ic.size();
        // the key: [alpha_beta 384 | gamma, delta 256 | IC_0 64 | IC 64 nidx]
        const size_t k_ab = 0, k_g2 = 384, k_ic0 = k_g2 + 256, k_ic = k_ic0 + 64, key_bytes = align16(k_ic + 64 * nidx);
        const size_t chunk = std::min(pos.size(), verify_each_round_positions(nidx, key_bytes));
        // a round of n <= chunk positions: [P 3 n x 64 | Q 3 n x 128 | M 3 n x 384 | x n nidx x 32 | slots | verdicts n]
        const size_t o_P = key_bytes, o_Q = o_P + 192 * chunk, o_M = o_Q + 384 * chunk, o_x = o_M + 1152 * chunk, o_ws = o_x + 32 * nidx * chunk,
                     o_v = o_ws + verify_final_exp_ws_bytes(chunk), total = o_v + chunk + 16;
        if (!lease.w && !(lease.w = verify_workspace_acquire())) return ZKG_ERROR;
        ZK_HIP(hipStreamSynchronize(lease.w->s));                           // (the previous key's rounds are done: the buffer may move)
        if (lease.w->buf.reserve(total)) return ZKG_ERROR;
        uint8_t *d = lease.w->buf.as<uint8_t>(); hipStream_t s = lease.w->s;
        const G2Affine key2[2] = {vk.gamma_g2, vk.delta_g2};
        ZK_HIP(hipMemcpyAsync(d + k_ab, &vk.alpha_beta, 384, hipMemcpyHostToDevice, s));
        ZK_HIP(hipMemcpyAsync(d + k_g2, key2, 256, hipMemcpyHostToDevice, s));
        ZK_HIP(hipMemcpyAsync(d + k_ic0, &vk.ic0, 64, hipMemcpyHostToDevice, s));
        if (nidx) ZK_HIP(hipMemcpyAsync(d + k_ic, vk.ic.data(), 64 * nidx, hipMemcpyHostToDevice, s));
        for (size_t lo = 0; lo < pos.size(); lo += chunk) {
            const size_t n = std::min(chunk, pos.size() - lo);
            pA.resize(n); pC.resize(n); pB.resize(n); px.resize(4 * nidx * n); v.assign(n, 0xFF);
            for (size_t t = 0; t < n; ++t) {
                const size_t i = pos[lo + t];
                pA[t] = hA[i]; pB[t] = hB[i]; pC[t] = hC[i].neg();
                for (size_t k = 0; k < nidx; ++k) memcpy(&px[4 * (t * nidx + k)], items[i].primary_input + 4 * vk.idx[k], 32);
            }
            G1Affine *dP = (G1Affine *)(d + o_P); G2Affine *dQ = (G2Affine *)(d + o_Q);
            ZK_HIP(hipMemcpyAsync(dP, pA.data(), 64 * n, hipMemcpyHostToDevice, s));
            ZK_HIP(hipMemcpyAsync(dP + 2 * n, pC.data(), 64 * n, hipMemcpyHostToDevice, s));
            ZK_HIP(hipMemcpyAsync(dQ, pB.data(), 128 * n, hipMemcpyHostToDevice, s));
            if (nidx) ZK_HIP(hipMemcpyAsync(d + o_x, px.data(), 32 * nidx * n, hipMemcpyHostToDevice, s));
            if (verify_g2_replicate((const G2Affine *)(d + k_g2), n, dQ, s) ||
                verify_ic_each((const G1Affine *)(d + k_ic0), (const G1Affine *)(d + k_ic), (uint32_t)nidx, d + o_x, n, dP + n, s) ||
                verify_miller(dP, dQ, nullptr, 3 * n, d + o_M, s) ||
                verify_final_exp_check(d + o_M, n, 3, d + o_ws, d + k_ab, d + o_v, nullptr, s)) return ZKG_ERROR;
            ZK_HIP(hipMemcpyAsync(v.data(), d + o_v, n, hipMemcpyDeviceToHost, s));
            ZK_HIP(hipStreamSynchronize(s));
            for (size_t t = 0; t < n; ++t) verdicts[pos[lo + t]] = v[t];
            ++rounds;
        }
        on_device += pos.size();
    }
    // everything else: the single verifier's code, on the host pool
    std::vector<size_t> decide_alone;
    for (size_t i = 0; i < count; ++i) if (own[i]) decide_alone.push_back(i);
    host_parallel_for((int)decide_alone.size(), [&](int t) {
        const zkg_verify_item &it = items[decide_alone[t]];
        int r;
        try { r = groth16_verify_impl(it.vk_blob, it.vk_len, it.primary_input, it.n_inputs, it.proof, it.proof_len); } catch (...) { r = 2; }
        verdicts[decide_alone[t]] = (uint8_t)r;
    });
    t_each_stats[0] = on_device; t_each_stats[1] = decide_alone.size(); t_each_stats[2] = rounds;
    return ZKG_OK;
}

int zkg_groth16_verify_each(const zkg_verify_item *items, size_t count, uint8_t *verdicts) {
    return c_boundary("zkg_groth16_verify_each", ZKG_ERROR, [&] { return verify_each_impl(items, count, verdicts); });
}
void zkg_verify_each_stats(size_t out[3]) { if (out) for (int i = 0; i < 3; ++i) out[i] = t_each_stats[i]; }
void zkg_verify_each_set_chunk(size_t positions) { g_each_chunk.store(positions); }

// ---- zkg_zklaim_verify_batch: many libsnark_verify calls in one.  The contexts of one key are one group of the batch above; by default its
// front end is the device's (ZKG_SEAM_GPU_VERIFY=0: the host's, zkg_zklaim_input_map per item and then zkg_groth16_verify_batch's path; a
// call that holds keys of both kinds runs the batch core once per front end).
// One upload per call, directly behind the core's weights:
//     [ weights 16 B x N | proof records 134 B x N | per group, per position: its payloads' public records, 80 B each (zklaim_public.hip.hpp) ]
// k_proof_decode turns the records into the points (B on the first stream in front of the event that releases the G2 test, A and C in one
// launch in front of k_g1_mul128), k_zklaim_input_sums forms the s_k of a range from the public records beside the range's Fq12 product.
// Neither the proofs' square roots nor a single public input exist on the host.
namespace {
static constexpr size_t SEAM_VERIFY_STAGE_MAX = (size_t)64 << 20;           // device staging of one call's device groups; beyond: the host front end

// payloads of a context as zkg_zklaim_input_map walks them, counted up to cap + 1
uint32_t payloads_walked(const zklaim_ctx *ctx, uint32_t cap) {
    uint32_t n = 0;
    for (const zklaim_wrap_payload_ctx *cur = ctx->pl_ctx_head; cur && n <= cap; cur = cur->next) ++n;
    return n;
}
void pack_public_records(const zklaim_ctx *ctx, uint32_t npl, uint8_t *out) {     // npl records (the list is at least that long)
    const zklaim_wrap_payload_ctx *cur = ctx->pl_ctx_head;
    for (uint32_t j = 0; j < npl; ++j, cur = cur->next, out += ZV_REC) {
        memcpy(out, cur->pl.hash, 32); memcpy(out + 32, cur->pl.data_ref, 40); memset(out + 72, 0, 8);
        for (int a = 0; a < 5; ++a) {
            uint8_t code = 0;
            switch ((int)cur->pl.data_op[a]) {                              // set_ops: which byte of the slot is set
            case zklaim_less: code = 1; break;          case zklaim_less_or_eq: code = 2; break;
            case zklaim_eq: code = 3; break;            case zklaim_greater_or_eq: code = 4; break;
            case zklaim_greater: code = 5; break;       case zklaim_not_eq: code = 6; break;
            case zklaim_noop: code = 7; break;          default: break;
            }
            out[72 + a] = code;
        }
    }
}
int verify_ctx_alone(const zklaim_ctx *c) {                                 // libsnark_verify's body
    const size_t n = zkg_zklaim_input_map(c, nullptr, 0);
    std::vector<uint64_t> input(4 * n + 4);
    zkg_zklaim_input_map(c, input.data(), n);
    return groth16_verify_impl(c->vk, c->vk_size, input.data(), n, c->proof, c->proof_size);
}

struct CtxFrontEnd : BatchFrontEnd {
    const zklaim_ctx *const *ctxs;
    std::vector<uint8_t> host;                                              // the upload
    size_t pub_bytes = 0, max_elems = 0;
    std::vector<Fr> sums;
    BatchLaps *lap = nullptr;
    explicit CtxFrontEnd(const zklaim_ctx *const *c) : ctxs(c) {}
    bool on_device() const override { return true; }
    size_t stage_bytes(size_t N) const override { return ((ZKG_PROOF_BYTES * N + 15) & ~(size_t)15) + pub_bytes; }
    size_t sum_elems() const override { return max_elems; }
    static size_t pub_at(size_t N) { return 16 * N + ((ZKG_PROOF_BYTES * N + 15) & ~(size_t)15); }
    int stage_B(const BatchLayout &L, const std::vector<BatchGroup> &groups, const std::vector<size_t> &item_at, const uint32_t *w) override {
        const size_t N = L.N;
        host.resize(16 * N + stage_bytes(N));
        memcpy(host.data(), w, 16 * N);
        std::vector<const BatchGroup *> group_at(N);
        for (const BatchGroup &G : groups) for (size_t p = G.lo; p < G.hi; ++p) group_at[p] = &G;
        const int chunks = (int)std::min<size_t>(64, N);
        host_parallel_for(chunks, [&](int c) {
            for (size_t p = N * (size_t)c / chunks; p < N * (size_t)(c + 1) / chunks; ++p) {
                const zklaim_ctx *ctx = ctxs[item_at[p]];
                const BatchGroup &G = *group_at[p];
                memcpy(host.data() + 16 * N + ZKG_PROOF_BYTES * p, ctx->proof, ZKG_PROOF_BYTES);
                pack_public_records(ctx, G.npl, host.data() + pub_at(N) + G.pub_at + (p - G.lo) * G.npl * ZV_REC);
            }
        });
        if (lap) (*lap)("decode");                                          // (the host's share of it: the records packed)
        ZK_HIP(hipMemcpyAsync(L.d + L.o_w, host.data(), host.size(), hipMemcpyHostToDevice, L.s));
        return verify_proof_decode_b(L.d + L.o_fe, N, (G2Affine *)(L.d + L.o_B), L.d + L.o_flags + N, L.s);
    }
    int stage_AC(const BatchLayout &L, const uint32_t *) override {
        return verify_proof_decode_ac(L.d + L.o_fe, L.N, (G1Affine *)(L.d + L.o_A), L.d + L.o_flags + 2 * L.N, L.s);
    }
    int sums_begin(const BatchLayout &L, const BatchGroup &G, size_t lo, size_t hi) override {
        const size_t l = zv_input_count(G.npl);
        sums.resize(l);
        uint8_t *d_out = L.d + L.o_sums, *d_part = d_out + 32 * max_elems;
        if (verify_zklaim_input_sums(L.d + L.o_w + pub_at(L.N) + G.pub_at, G.npl, G.lo, (const uint32_t *)(L.d + L.o_w), L.d + L.o_flags + 4 * L.N,
                                     lo, hi, d_part, d_out, L.s2)) return ZKG_ERROR;
        ZK_HIP(hipMemcpyAsync(sums.data(), d_out, 32 * l, hipMemcpyDeviceToHost, L.s2));
        return ZKG_OK;
    }
    int sums_ready(const BatchLayout &L) override { ZK_HIP(hipStreamSynchronize(L.s2)); return ZKG_OK; }
    void scalar_of(const BatchGroup &G, const std::vector<size_t> &, const std::vector<size_t> &, const Fr *, size_t k, Fr &x) override { x = sums[G.vk->idx[k]]; }
    int alone(size_t i) override { return verify_ctx_alone(ctxs[i]); }
};
}  // namespace

// which front end a key's group takes when ZKG_SEAM_GPU_VERIFY is not set: the device's wherever tools/seam_verify_batch_time.py found it
// no slower than hand-built items — every measured shape from 512 payload records (entering items x payloads) on; 64 one-payload items,
// the one shape below, lose 0.7 ms to the decode chains in front of the G2 test ("Seam entry and device front end")
static constexpr size_t SEAM_VERIFY_DEVICE_MIN_RECORDS = 512;
static bool seam_verify_device_default(uint32_t npl, size_t n_in) { return n_in * npl >= SEAM_VERIFY_DEVICE_MIN_RECORDS; }

// front_end: 0 the host's for every key, 1 the device's, anything else the default per group
static int seam_verify_batch_impl(const zklaim_ctx *const *ctxs, size_t count, int *rc, int front_end) {
    if (initialised_device() < 0) { set_error("zkg_zklaim_verify_batch: zkg_init not called (no GPU: there is no CPU path)"); return ZKG_ERROR; }
    BatchCounts cnt;
    std::vector<uint8_t> verdicts(count, 1);
    std::vector<char> own(count, 0), host_leg(count, 0);
    for (size_t i = 0; i < count; ++i) if (!ctxs[i] || !ctxs[i]->vk || !ctxs[i]->vk_size || !ctxs[i]->proof) own[i] = 2;       // rc 1, nothing to verify
    if (front_end == 0) { for (size_t i = 0; i < count; ++i) if (!own[i]) host_leg[i] = 1; }
    else {
        BatchLaps lap(count);
        std::vector<BatchGroup> groups;
        batch_group_keys(count, [&](size_t i, size_t &len) { len = ctxs[i]->vk_size; return (const uint8_t *)ctxs[i]->vk; }, groups, own);
        lap("keys");
        // a key's input count names its payload count (1280 bits per payload, 253 per input: the counts grow strictly); an item enters if
        // its proof has the size and its payload list, walked as zkg_zklaim_input_map walks it, has that many payloads
        CtxFrontEnd fe(ctxs);
        fe.lap = &lap;
        size_t entering = 0;
        for (BatchGroup &G : groups) {
            if (!G.batchable) continue;
            const size_t domain = G.vk->domain;
            const uint32_t npl = (uint32_t)std::min<size_t>(domain * ZV_FR_CAPACITY / (ZV_STRING_BYTES * 8), (size_t)1 << 20);
            G.npl = npl && zv_input_count(npl) == domain ? npl : 0;
            size_t n_in = 0;
            for (size_t i : G.items) if (G.npl && ctxs[i]->proof_size == ZKG_PROOF_BYTES && payloads_walked(ctxs[i], G.npl) == G.npl) ++n_in;
            const size_t grown = entering + n_in, staged = 16 * grown + ((ZKG_PROOF_BYTES * grown + 15) & ~(size_t)15) + fe.pub_bytes + n_in * G.npl * ZV_REC;
            if ((front_end != 1 && !seam_verify_device_default(G.npl, n_in)) || staged > SEAM_VERIFY_STAGE_MAX) {      // this key takes the host front end
                for (size_t i : G.items) host_leg[i] = 1;
                G.items.clear();
                continue;
            }
            for (size_t i : G.items) if (!(G.npl && ctxs[i]->proof_size == ZKG_PROOF_BYTES && payloads_walked(ctxs[i], G.npl) == G.npl)) own[i] = 1;
            G.pub_at = fe.pub_bytes;
            fe.pub_bytes += n_in * G.npl * ZV_REC;
            if (n_in) fe.max_elems = std::max(fe.max_elems, domain);
            entering += n_in;
        }
        for (size_t i = 0; i < count; ++i) if (own[i] == 2 || host_leg[i]) own[i] = 0;       // decided already, or the other leg's: not this core's
        if (int r = verify_batch_core(groups, own, count, fe, verdicts.data(), lap, cnt)) return r;
    }
    // the host front end: the input map of every context on the host pool, then zkg_groth16_verify_batch's own path
    std::vector<size_t> live;
    for (size_t i = 0; i < count; ++i) if (host_leg[i]) live.push_back(i);
    if (!live.empty()) {
        std::vector<std::vector<uint64_t>> inputs(live.size());
        std::vector<zkg_verify_item> items(live.size());
        const int chunks = (int)std::min<size_t>(64, live.size());
        host_parallel_for(chunks, [&](int c) {
            for (size_t t = live.size() * (size_t)c / chunks; t < live.size() * (size_t)(c + 1) / chunks; ++t) {
                const zklaim_ctx *x = ctxs[live[t]];
                const size_t n = zkg_zklaim_input_map(x, nullptr, 0);
                inputs[t].resize(4 * n + 4);
                zkg_zklaim_input_map(x, inputs[t].data(), n);
                items[t] = zkg_verify_item{x->vk, x->vk_size, inputs[t].data(), n, x->proof, x->proof_size};
            }
        });
        std::vector<uint8_t> v(live.size(), 1);
        BatchCounts host_cnt;
        if (int r = verify_batch_items(items.data(), live.size(), v.data(), host_cnt)) return r;
        for (size_t t = 0; t < live.size(); ++t) verdicts[live[t]] = v[t];
        cnt.combined += host_cnt.combined; cnt.alone += host_cnt.alone; cnt.outside_g2 += host_cnt.outside_g2;
    }
    for (size_t i = 0; i < count; ++i) rc[i] = verdicts[i] == 0 ? 0 : 1;
    t_seam_batch_stats[0] = cnt.combined; t_seam_batch_stats[1] = cnt.alone; t_seam_batch_stats[2] = cnt.outside_g2; t_seam_batch_stats[3] = cnt.from_device;
    return ZKG_OK;
}
}  // extern "C"
// compat.hip's entry: arguments checked, the seam's device bound; rc[i] is written for every i
int seam_verify_batch(const zklaim_ctx *const *ctxs, size_t count, int *rc, int front_end) {
    for (size_t i = 0; i < 4; ++i) t_seam_batch_stats[i] = 0;
    return seam_verify_batch_impl(ctxs, count, rc, front_end);
}
void seam_verify_batch_stats_clear() { for (size_t i = 0; i < 4; ++i) t_seam_batch_stats[i] = 0; }
extern "C" {

void zkg_zklaim_verify_batch_stats(size_t out[4]) { if (out) for (int i = 0; i < 4; ++i) out[i] = t_seam_batch_stats[i]; }

// ---- zkg_zklaim_verify_each: every context decided by its own equation, as zkg_groth16_verify_each decides its items, with the batch
// entry's device front end in front: per round one upload [key (first round) | proof records 134 B x n | public records 80 B x npl x n],
// k_proof_decode for A, B and C, and -acc_i from the key's bit table (k_zklaim_ic_each, which also turns C into -C), then k_g2_replicate,
// k_miller over [A | -acc | -C] x [B | gamma.. | delta..] and k_final_exp_check.  Neither a square root nor a public input exists on the
// host for an entering item.  The table build and the accumulator run on the workspace's second stream beside the decode of B; the
// Miller launch waits for them.  An item whose A, B or C did not decode is decided by the single verifier afterwards.
static thread_local size_t t_seam_each_stats[4] = {0, 0, 0, 0};

// positions per round of a key at npl payloads; per position: P 3 x 64, Q 3 x 128, Miller values 3 x 384, the proof record, the public
// records, slots, verdict and three flags
static size_t seam_each_round_positions(uint32_t npl) {
    if (const size_t forced = g_each_chunk.load()) return forced;
    const size_t per = 3 * 64 + 3 * 128 + 3 * 384 + ZKG_PROOF_BYTES + (size_t)ZV_REC * npl + verify_final_exp_ws_bytes(64) / 64 + 4;
    return std::max<size_t>(64, (VERIFY_EACH_STAGE_MAX - 4096) / per / 64 * 64);
}
// the key's bit table: built on s2 by the first call that meets the key (a second caller of the same key waits for that build), then read-only
static int seam_each_bit_table(const PreparedVk &vk, uint32_t npl, hipStream_t s2, size_t &built) {
    std::call_once(vk.bits_once, [&] {
        const uint32_t l = zv_input_count(npl);
        std::vector<G1Affine> dense(l, G1Affine::inf());                    // an absent index: infinity, its entries are skipped
        for (size_t j = 0; j < vk.idx.size(); ++j) dense[vk.idx[j]] = vk.ic[j];
        ScopedDevBuf d_ic, d_tmp;
        bool ok = !d_ic.reserve(64 * (size_t)l) && !d_tmp.reserve(zklaim_bit_table_tmp_bytes(npl)) && !vk.bits.reserve(64 * zklaim_bit_table_entries(npl)) &&
                  hip_ok(hipMemcpyAsync(d_ic.p, dense.data(), 64 * (size_t)l, hipMemcpyHostToDevice, s2), "H2D", __FILE__, __LINE__) &&
                  verify_zklaim_bit_table(d_ic.as<G1Affine>(), npl, d_tmp.p, vk.bits.as<G1Affine>(), s2) == ZKG_OK;
        ok = hip_ok(hipStreamSynchronize(s2), "sync", __FILE__, __LINE__) && ok;
        vk.bits_device = initialised_device(); vk.bits_ok = ok;
        if (ok) ++built;
    });
    if (!vk.bits_ok || vk.bits_device != initialised_device()) { set_error("zkg_zklaim_verify_each: the key's bit table is not on this device"); return ZKG_ERROR; }
    return ZKG_OK;
}

static int seam_verify_each_impl(const zklaim_ctx *const *ctxs, size_t count, int *rc) {
    if (initialised_device() < 0) { set_error("zkg_zklaim_verify_each: zkg_init not called (no GPU: there is no CPU path)"); return ZKG_ERROR; }
    std::vector<uint8_t> verdicts(count, 1);
    std::vector<char> own(count, 0);                                        // 1: decided by the single verifier's code
    for (size_t i = 0; i < count; ++i) if (!ctxs[i] || !ctxs[i]->vk || !ctxs[i]->vk_size || !ctxs[i]->proof) own[i] = 2;       // rc 1, nothing to verify
    std::vector<BatchGroup> groups;
    batch_group_keys(count, [&](size_t i, size_t &len) { len = ctxs[i]->vk_size; return (const uint8_t *)ctxs[i]->vk; }, groups, own, false);
    size_t on_device = 0, rounds = 0, built = 0;
    WorkspaceLease lease;
    std::vector<uint8_t> host, back;
    for (const BatchGroup &G : groups) {
        if (!G.batchable) continue;
        const PreparedVk &vk = *G.vk;
        // a key's input count names its payload count, as in seam_verify_batch_impl; the table takes one point per input element
        const size_t domain = vk.domain;
        uint32_t npl = (uint32_t)std::min<size_t>(domain * ZV_FR_CAPACITY / (ZV_STRING_BYTES * 8), (size_t)1 << 20);
        if (!npl || zv_input_count(npl) != domain) npl = 0;
        if (npl) { std::vector<char> seen(domain, 0); for (size_t k : vk.idx) { if (seen[k]) npl = 0; seen[k] = 1; } }
        std::vector<size_t> pos;
        for (size_t i : G.items) {
            if (npl && ctxs[i]->proof_size == ZKG_PROOF_BYTES && payloads_walked(ctxs[i], npl) == npl) pos.push_back(i); else own[i] = 1;
        }
        if (pos.empty()) continue;
        const size_t chunk = std::min(pos.size(), seam_each_round_positions(npl));
        // the key: [alpha_beta 384 | gamma, delta 256 | IC_0 64]; a round of n <= chunk positions: [records 134 n | public records 80 npl n]
        // behind the key (the upload), then [P 3 n x 64 | Q 3 n x 128 | M 3 n x 384 | slots | verdicts n, B decoded n, A decoded n, C decoded n]
        const size_t k_ab = 0, k_g2 = 384, k_ic0 = k_g2 + 256, o_rec = k_ic0 + 64, o_P = align16(o_rec + align16(ZKG_PROOF_BYTES * chunk) + (size_t)ZV_REC * npl * chunk),
                     o_Q = o_P + 192 * chunk, o_M = o_Q + 384 * chunk, o_ws = o_M + 1152 * chunk, o_v = o_ws + verify_final_exp_ws_bytes(chunk), total = o_v + 4 * chunk + 16;
        if (!lease.w && !(lease.w = verify_workspace_acquire())) return ZKG_ERROR;
        ZK_HIP(hipStreamSynchronize(lease.w->s));                           // (the previous key's rounds are done: the buffer may move)
        ZK_HIP(hipStreamSynchronize(lease.w->s2));
        if (lease.w->buf.reserve(total)) return ZKG_ERROR;
        uint8_t *d = lease.w->buf.as<uint8_t>(); hipStream_t s = lease.w->s, s2 = lease.w->s2;
        for (size_t lo = 0; lo < pos.size(); lo += chunk) {
            const size_t n = std::min(chunk, pos.size() - lo), up0 = lo ? o_rec : 0, o_pub = o_rec + align16(ZKG_PROOF_BYTES * n);
            host.assign(o_pub + (size_t)ZV_REC * npl * n, 0);
            if (!lo) {
                const G2Affine key2[2] = {vk.gamma_g2, vk.delta_g2};
                memcpy(host.data() + k_ab, &vk.alpha_beta, 384); memcpy(host.data() + k_g2, key2, 256); memcpy(host.data() + k_ic0, &vk.ic0, 64);
            }
            const int parts = (int)std::min<size_t>(64, n);
            host_parallel_for(parts, [&](int c) {
                for (size_t t = n * (size_t)c / parts; t < n * (size_t)(c + 1) / parts; ++t) {
                    const zklaim_ctx *ctx = ctxs[pos[lo + t]];
                    memcpy(host.data() + o_rec + ZKG_PROOF_BYTES * t, ctx->proof, ZKG_PROOF_BYTES);
                    pack_public_records(ctx, npl, host.data() + o_pub + t * npl * ZV_REC);
                }
            });
            G1Affine *dP = (G1Affine *)(d + o_P); G2Affine *dQ = (G2Affine *)(d + o_Q);
            ZK_HIP(hipMemcpyAsync(d + up0, host.data() + up0, host.size() - up0, hipMemcpyHostToDevice, s));
            if (verify_proof_decode_ac(d + o_rec, n, dP, d + o_v + 2 * n, s)) return ZKG_ERROR;        // A at 0, C at n (the accumulator moves it)
            ZK_HIP(hipEventRecord(lease.w->ev, s));
            if (verify_proof_decode_b(d + o_rec, n, dQ, d + o_v + n, s) || verify_g2_replicate((const G2Affine *)(d + k_g2), n, dQ, s)) return ZKG_ERROR;
            if (seam_each_bit_table(vk, npl, s2, built)) return ZKG_ERROR;
            ZK_HIP(hipStreamWaitEvent(s2, lease.w->ev, 0));
            if (verify_zklaim_ic_each((const G1Affine *)(d + k_ic0), vk.bits.as<G1Affine>(), d + o_pub, npl, n, dP + n, dP + n, dP + 2 * n, s2)) return ZKG_ERROR;
            ZK_HIP(hipEventRecord(lease.w->ev2, s2));
            ZK_HIP(hipStreamWaitEvent(s, lease.w->ev2, 0));
            if (verify_miller(dP, dQ, nullptr, 3 * n, d + o_M, s) ||
                verify_final_exp_check(d + o_M, n, 3, d + o_ws, d + k_ab, d + o_v, nullptr, s)) return ZKG_ERROR;
            back.assign(4 * n, 0xFF);
            ZK_HIP(hipMemcpyAsync(back.data(), d + o_v, 4 * n, hipMemcpyDeviceToHost, s));
            ZK_HIP(hipStreamSynchronize(s));
            for (size_t t = 0; t < n; ++t) {
                if (back[n + t] == 1 && back[2 * n + t] == 1 && back[3 * n + t] == 1) { verdicts[pos[lo + t]] = back[t]; ++on_device; }
                else own[pos[lo + t]] = 1;                                  // a point that did not decode: the single verifier says why
            }
            ++rounds;
        }
    }
    std::vector<size_t> decide_alone;
    for (size_t i = 0; i < count; ++i) if (own[i] == 1) decide_alone.push_back(i);
    host_parallel_for((int)decide_alone.size(), [&](int t) {
        int v;
        try { v = verify_ctx_alone(ctxs[decide_alone[t]]); } catch (...) { v = 2; }
        verdicts[decide_alone[t]] = (uint8_t)v;
    });
    for (size_t i = 0; i < count; ++i) rc[i] = verdicts[i] == 0 ? 0 : 1;
    t_seam_each_stats[0] = on_device; t_seam_each_stats[1] = decide_alone.size(); t_seam_each_stats[2] = rounds; t_seam_each_stats[3] = built;
    return ZKG_OK;
}
}  // extern "C"
// compat.hip's entry: arguments checked, the seam's device bound; rc[i] is written for every i
int seam_verify_each(const zklaim_ctx *const *ctxs, size_t count, int *rc) { return seam_verify_each_impl(ctxs, count, rc); }
void seam_verify_each_stats_clear() { for (size_t i = 0; i < 4; ++i) t_seam_each_stats[i] = 0; }
extern "C" {
void zkg_zklaim_verify_each_stats(size_t out[4]) { if (out) for (int i = 0; i < 4; ++i) out[i] = t_seam_each_stats[i]; }

// test hook of the accumulator (include/zkg.h)
static int zklaim_ic_each_impl(const uint64_t *ic0, const uint64_t *ic, const zklaim_ctx *const *ctxs, size_t count, int where, uint64_t *out) {
    if (where != 1 && where != 2) { set_error("zkg_zklaim_ic_each: where is 1 (GPU) or 2 (the device code on the host)"); return ZKG_ERROR; }
    if (where == 1 && initialised_device() < 0) { set_error("zkg_zklaim_ic_each: zkg_init not called (no GPU: the kernel has no CPU path)"); return ZKG_ERROR; }
    if (!ic0 || !ic || !ctxs || !count || !out) { set_error("zkg_zklaim_ic_each: bad argument"); return ZKG_ERROR; }
    size_t first = 0;
    while (first < count && !ctxs[first]) ++first;
    const uint32_t npl = first < count ? payloads_walked(ctxs[first], 4096) : 0;
    if (!npl || npl > 4096 || count > ((size_t)1 << 20)) { set_error("zkg_zklaim_ic_each: payload or context count out of range"); return ZKG_ERROR; }
    for (size_t i = 0; i < count; ++i)
        if (!ctxs[i] || payloads_walked(ctxs[i], npl) != npl) { set_error("zkg_zklaim_ic_each: a null context or another payload count"); return ZKG_ERROR; }
    const uint32_t l = zv_input_count(npl);
    std::vector<G1Affine> key(1 + (size_t)l);                               // IC_0, then the l points
    memcpy(&key[0], ic0, 64); memcpy(&key[1], ic, 64 * (size_t)l);
    for (const G1Affine &p : key)
        if (!limbs_below(p.x.v, FqParams::P) || !limbs_below(p.y.v, FqParams::P) || !pairing::on_curve_g1(p)) { set_error("zkg_zklaim_ic_each: a point is not on the curve"); return ZKG_ERROR; }
    const size_t pub = count * npl * ZV_REC;
    std::vector<uint8_t> host(pub);
    for (size_t i = 0; i < count; ++i) pack_public_records(ctxs[i], npl, host.data() + i * npl * ZV_REC);
    std::vector<G1Affine> res(count);
    if (where == 2) zklaim_ic_each_device_code_on_host(key[0], key.data() + 1, host.data(), npl, count, res.data());
    else {
        const size_t o_key = 0, o_T = align16(64 * key.size()), o_tmp = o_T + 64 * zklaim_bit_table_entries(npl), o_pub = align16(o_tmp + zklaim_bit_table_tmp_bytes(npl)),
                     o_out = align16(o_pub + pub), total = o_out + 64 * count + 16;
        WorkspaceLease lease;
        if (!(lease.w = verify_workspace_acquire()) || lease.w->buf.reserve(total)) return ZKG_ERROR;
        uint8_t *d = lease.w->buf.as<uint8_t>(); hipStream_t s = lease.w->s;
        ZK_HIP(hipMemcpyAsync(d + o_key, key.data(), 64 * key.size(), hipMemcpyHostToDevice, s));
        ZK_HIP(hipMemcpyAsync(d + o_pub, host.data(), pub, hipMemcpyHostToDevice, s));
        if (verify_zklaim_bit_table((const G1Affine *)(d + o_key) + 1, npl, d + o_tmp, (G1Affine *)(d + o_T), s) ||
            verify_zklaim_ic_each((const G1Affine *)(d + o_key), (const G1Affine *)(d + o_T), d + o_pub, npl, count, (G1Affine *)(d + o_out), nullptr, nullptr, s)) return ZKG_ERROR;
        ZK_HIP(hipMemcpyAsync(res.data(), d + o_out, 64 * count, hipMemcpyDeviceToHost, s));
        ZK_HIP(hipStreamSynchronize(s));
    }
    memcpy(out, res.data(), 64 * count);
    return ZKG_OK;
}
int zkg_zklaim_ic_each(const uint64_t *ic0, const uint64_t *ic, const zklaim_ctx *const *ctxs, size_t count, int where, uint64_t *out) {
    return c_boundary("zkg_zklaim_ic_each", ZKG_ERROR, [&] { return zklaim_ic_each_impl(ic0, ic, ctxs, count, where, out); });
}

// ---- test hooks of the device front end
static int proof_decode_gpu_impl(const uint8_t *proofs, size_t count, uint64_t *A, uint64_t *B, uint64_t *C, uint8_t *ok) {
    if (initialised_device() < 0) { set_error("zkg_proof_decode_gpu: zkg_init not called (no GPU: there is no CPU path)"); return ZKG_ERROR; }
    if (count && (!proofs || !A || !B || !C || !ok)) { set_error("zkg_proof_decode_gpu: null argument"); return ZKG_ERROR; }
    if (!count) return ZKG_OK;
    if (count > ((size_t)1 << 24)) { set_error("zkg_proof_decode_gpu: at most 2^24 proofs"); return ZKG_ERROR; }
    const size_t N = count, o_A = 0, o_C = 64 * N, o_B = 128 * N, o_dec = 256 * N, o_rec = (o_dec + 3 * N + 15) & ~(size_t)15, total = o_rec + ZKG_PROOF_BYTES * N + 16;
    WorkspaceLease lease;
    if (!(lease.w = verify_workspace_acquire()) || lease.w->buf.reserve(total)) return ZKG_ERROR;
    uint8_t *d = lease.w->buf.as<uint8_t>(); hipStream_t s = lease.w->s;
    std::vector<uint8_t> dec(3 * N);
    ZK_HIP(hipMemcpyAsync(d + o_rec, proofs, ZKG_PROOF_BYTES * N, hipMemcpyHostToDevice, s));
    if (verify_proof_decode_b(d + o_rec, N, (G2Affine *)(d + o_B), d + o_dec, s) ||
        verify_proof_decode_ac(d + o_rec, N, (G1Affine *)(d + o_A), d + o_dec + N, s)) return ZKG_ERROR;
    ZK_HIP(hipMemcpyAsync(A, d + o_A, 64 * N, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipMemcpyAsync(C, d + o_C, 64 * N, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipMemcpyAsync(B, d + o_B, 128 * N, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipMemcpyAsync(dec.data(), d + o_dec, 3 * N, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < N; ++i) ok[i] = (uint8_t)((dec[N + i] ? 1 : 0) | (dec[i] ? 2 : 0) | (dec[2 * N + i] ? 4 : 0));
    return ZKG_OK;
}
int zkg_proof_decode_gpu(const uint8_t *proofs, size_t count, uint64_t *A, uint64_t *B, uint64_t *C, uint8_t *ok) {
    return c_boundary("zkg_proof_decode_gpu", ZKG_ERROR, [&] { return proof_decode_gpu_impl(proofs, count, A, B, C, ok); });
}

static int input_sums_gpu_impl(const zklaim_ctx *const *ctxs, size_t count, const uint32_t *weights, const uint8_t *mask, size_t lo, size_t hi,
                               uint64_t *sums_out, size_t cap_elems, size_t *n_elems) {
    if (initialised_device() < 0) { set_error("zkg_zklaim_input_sums_gpu: zkg_init not called (no GPU: there is no CPU path)"); return ZKG_ERROR; }
    if (!ctxs || !count || !weights || !n_elems || lo > hi || hi > count) { set_error("zkg_zklaim_input_sums_gpu: bad argument"); return ZKG_ERROR; }
    if (!ctxs[0]) { set_error("zkg_zklaim_input_sums_gpu: null context"); return ZKG_ERROR; }
    const uint32_t npl = payloads_walked(ctxs[0], 4096);
    if (!npl || npl > 4096 || count > ((size_t)1 << 24)) { set_error("zkg_zklaim_input_sums_gpu: payload or context count out of range"); return ZKG_ERROR; }
    for (size_t i = 0; i < count; ++i)
        if (!ctxs[i] || payloads_walked(ctxs[i], npl) != npl) { set_error("zkg_zklaim_input_sums_gpu: a null context or another payload count"); return ZKG_ERROR; }
    const size_t l = zv_input_count(npl);
    *n_elems = l;
    if (!sums_out || cap_elems < l) { set_error("zkg_zklaim_input_sums_gpu: sums_out too small"); return ZKG_ERROR; }
    const size_t N = count, pub = N * npl * ZV_REC, o_w = 0, o_mask = 16 * N, o_pub = (o_mask + N + 15) & ~(size_t)15, o_out = (o_pub + pub + 31) & ~(size_t)31,
                 o_part = o_out + 32 * l, total = o_part + 32 * l * ZV_SUM_SLICES + 16;
    std::vector<uint8_t> host(o_pub + pub);
    memcpy(host.data() + o_w, weights, 16 * N);
    if (mask) memcpy(host.data() + o_mask, mask, N);
    for (size_t i = 0; i < N; ++i) pack_public_records(ctxs[i], npl, host.data() + o_pub + i * npl * ZV_REC);
    WorkspaceLease lease;
    if (!(lease.w = verify_workspace_acquire()) || lease.w->buf.reserve(total)) return ZKG_ERROR;
    uint8_t *d = lease.w->buf.as<uint8_t>(); hipStream_t s = lease.w->s;
    ZK_HIP(hipMemcpyAsync(d, host.data(), host.size(), hipMemcpyHostToDevice, s));
    if (verify_zklaim_input_sums(d + o_pub, npl, 0, (const uint32_t *)(d + o_w), mask ? d + o_mask : nullptr, lo, hi, d + o_part, d + o_out, s)) return ZKG_ERROR;
    ZK_HIP(hipMemcpyAsync(sums_out, d + o_out, 32 * l, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    return ZKG_OK;
}
int zkg_zklaim_input_sums_gpu(const zklaim_ctx *const *ctxs, size_t count, const uint32_t *weights, const uint8_t *mask, size_t lo, size_t hi,
                              uint64_t *sums_out, size_t cap_elems, size_t *n_elems) {
    return c_boundary("zkg_zklaim_input_sums_gpu", ZKG_ERROR, [&] { return input_sums_gpu_impl(ctxs, count, weights, mask, lo, hi, sums_out, cap_elems, n_elems); });
}

// the kernel's bit rule (zv_input_element) on the host: same outputs as zkg_zklaim_input_map
size_t zkg_zklaim_input_map_mirror(const zklaim_ctx *ctx, uint64_t *out, size_t cap_elems) {
    if (!ctx) return 0;
    try {
        uint32_t npl = 0;
        for (const zklaim_wrap_payload_ctx *cur = ctx->pl_ctx_head; cur; cur = cur->next) ++npl;
        const size_t n = zv_input_count(npl);
        if (!out || cap_elems < n) return n;
        std::vector<uint8_t> rec((size_t)npl * ZV_REC + 1);
        pack_public_records(ctx, npl, rec.data());
        for (size_t k = 0; k < n; ++k) { Fr x; zv_input_element(rec.data(), npl, (uint32_t)k, x.v); x = x.to_mont(); memcpy(out + 4 * k, x.v, 32); }
        return n;
    } catch (...) { return 0; }
}

static int pairing_product_impl(const uint64_t *g1_affine, const uint64_t *g2_affine, size_t n, uint8_t out[384]) {
    if (initialised_device() < 0) { set_error("zkg_pairing_product: zkg_init not called (no GPU: there is no CPU path)"); return ZKG_ERROR; }
    if (!out || (n && (!g1_affine || !g2_affine))) { set_error("zkg_pairing_product: null argument"); return ZKG_ERROR; }
    std::vector<G1Affine> P(n); std::vector<G2Affine> Q(n);
    if (n) { memcpy(P.data(), g1_affine, 64 * n); memcpy(Q.data(), g2_affine, 128 * n); }
    for (size_t i = 0; i < n; ++i) {
        const bool canon = limbs_below(P[i].x.v, FqParams::P) && limbs_below(P[i].y.v, FqParams::P) && limbs_below(Q[i].x.c0.v, FqParams::P) &&
                           limbs_below(Q[i].x.c1.v, FqParams::P) && limbs_below(Q[i].y.c0.v, FqParams::P) && limbs_below(Q[i].y.c1.v, FqParams::P);
        if (!canon || !pairing::on_curve_g1(P[i]) || !pairing::on_curve_g2(Q[i])) { set_error("zkg_pairing_product: point " + std::to_string(i) + " is not on its curve"); return ZKG_ERROR; }
    }
    Fq12 prod = Fq12::one();
    if (n) {
        const size_t o_P = 0, o_Q = 64 * n, o_M = o_Q + 128 * n, o_part = o_M + 384 * n, o_out = o_part + 384 * VERIFY_PROD_BLOCKS, total = o_out + 384;
        WorkspaceLease lease;
        if (!(lease.w = verify_workspace_acquire()) || lease.w->buf.reserve(total)) return ZKG_ERROR;
        uint8_t *d = lease.w->buf.as<uint8_t>(); hipStream_t s = lease.w->s;
        ZK_HIP(hipMemcpyAsync(d + o_P, P.data(), 64 * n, hipMemcpyHostToDevice, s));
        ZK_HIP(hipMemcpyAsync(d + o_Q, Q.data(), 128 * n, hipMemcpyHostToDevice, s));
        if (verify_miller((const G1Affine *)(d + o_P), (const G2Affine *)(d + o_Q), nullptr, n, d + o_M, s) ||
            verify_fq12_product(d + o_M, 0, n, d + o_part, d + o_out, s)) return ZKG_ERROR;
        ZK_HIP(hipMemcpyAsync(&prod, d + o_out, 384, hipMemcpyDeviceToHost, s));
        ZK_HIP(hipStreamSynchronize(s));
    }
    ser::put_fq12(out, pairing::final_exponentiation(prod));
    return ZKG_OK;
}

int zkg_pairing_product(const uint64_t *g1_affine, const uint64_t *g2_affine, size_t n, uint8_t out[384]) {
    return c_boundary("zkg_pairing_product", ZKG_ERROR, [&] { return pairing_product_impl(g1_affine, g2_affine, n, out); });
}

static bool point_pair_ok(const G1Affine &P, const G2Affine &Q) {             // canonical limbs, on the curves (zkg_pairing_product's rule)
    return limbs_below(P.x.v, FqParams::P) && limbs_below(P.y.v, FqParams::P) && limbs_below(Q.x.c0.v, FqParams::P) && limbs_below(Q.x.c1.v, FqParams::P) &&
           limbs_below(Q.y.c0.v, FqParams::P) && limbs_below(Q.y.c1.v, FqParams::P) && pairing::on_curve_g1(P) && pairing::on_curve_g2(Q);
}
static int pairing_each_impl(const uint64_t *g1_affine, const uint64_t *g2_affine, size_t items, size_t pairs, uint8_t *out) {
    if (initialised_device() < 0) { set_error("zkg_pairing_each: zkg_init not called (no GPU: there is no CPU path)"); return ZKG_ERROR; }
    if (items && (!out || (pairs && (!g1_affine || !g2_affine)))) { set_error("zkg_pairing_each: null argument"); return ZKG_ERROR; }
    if (!items) return ZKG_OK;
    if (pairs > 4096 || items > ((size_t)1 << 24)) { set_error("zkg_pairing_each: at most 2^24 items of 4096 pairs"); return ZKG_ERROR; }
    if (!pairs) { for (size_t i = 0; i < items; ++i) ser::put_fq12(out + 384 * i, Fq12::one()); return ZKG_OK; }
    const G1Affine *P = reinterpret_cast<const G1Affine *>(g1_affine); const G2Affine *Q = reinterpret_cast<const G2Affine *>(g2_affine);
    std::vector<G1Affine> tP; std::vector<G2Affine> tQ;
    for (size_t i = 0; i < items * pairs; ++i) {
        G1Affine p; G2Affine q; memcpy(&p, P + i, 64); memcpy(&q, Q + i, 128);
        if (!point_pair_ok(p, q)) { set_error("zkg_pairing_each: point " + std::to_string(i) + " is not on its curve"); return ZKG_ERROR; }
    }
    // rounds of `chunk` items within the staging limit; pair j of item t of a round at j n + t
    const size_t per = pairs * (64 + 128 + 384) + verify_final_exp_ws_bytes(64) / 64 + 384;
    const size_t chunk = std::min(items, std::max<size_t>(64, VERIFY_EACH_STAGE_MAX / per / 64 * 64));
    const size_t o_P = 0, o_Q = o_P + 64 * pairs * chunk, o_M = o_Q + 128 * pairs * chunk, o_ws = o_M + 384 * pairs * chunk,
                 o_gt = o_ws + verify_final_exp_ws_bytes(chunk), total = o_gt + 384 * chunk + 16;
    WorkspaceLease lease;
    if (!(lease.w = verify_workspace_acquire()) || lease.w->buf.reserve(total)) return ZKG_ERROR;
    uint8_t *d = lease.w->buf.as<uint8_t>(); hipStream_t s = lease.w->s;
    for (size_t lo = 0; lo < items; lo += chunk) {
        const size_t n = std::min(chunk, items - lo);
        tP.resize(pairs * n); tQ.resize(pairs * n);
        for (size_t t = 0; t < n; ++t) for (size_t j = 0; j < pairs; ++j) { memcpy(&tP[j * n + t], P + (lo + t) * pairs + j, 64); memcpy(&tQ[j * n + t], Q + (lo + t) * pairs + j, 128); }
        ZK_HIP(hipMemcpyAsync(d + o_P, tP.data(), 64 * pairs * n, hipMemcpyHostToDevice, s));
        ZK_HIP(hipMemcpyAsync(d + o_Q, tQ.data(), 128 * pairs * n, hipMemcpyHostToDevice, s));
        if (verify_miller((const G1Affine *)(d + o_P), (const G2Affine *)(d + o_Q), nullptr, pairs * n, d + o_M, s) ||
            verify_final_exp_check(d + o_M, n, (uint32_t)pairs, d + o_ws, nullptr, nullptr, d + o_gt, s)) return ZKG_ERROR;
        ZK_HIP(hipMemcpyAsync(out + 384 * lo, d + o_gt, 384 * n, hipMemcpyDeviceToHost, s));
        ZK_HIP(hipStreamSynchronize(s));
    }
    return ZKG_OK;
}
int zkg_pairing_each(const uint64_t *g1_affine, const uint64_t *g2_affine, size_t items, size_t pairs, uint8_t *out) {
    return c_boundary("zkg_pairing_each", ZKG_ERROR, [&] { return pairing_each_impl(g1_affine, g2_affine, items, pairs, out); });
}

static int final_exp_impl(const uint8_t *in, size_t n, int where, uint8_t *out) {
    if (where < 0 || where > 2) { set_error("zkg_final_exp: where is 0 (host), 1 (GPU) or 2 (the device code on the host)"); return ZKG_ERROR; }
    if (where == 1 && initialised_device() < 0) { set_error("zkg_final_exp: zkg_init not called (no GPU: the kernel has no CPU path)"); return ZKG_ERROR; }
    if (n && (!in || !out)) { set_error("zkg_final_exp: null argument"); return ZKG_ERROR; }
    if (n > ((size_t)1 << 20)) { set_error("zkg_final_exp: at most 2^20 elements"); return ZKG_ERROR; }
    for (size_t i = 0; i < n; ++i) {
        bool any = false;
        for (int k = 0; k < 12; ++k) {
            uint32_t x[8]; memcpy(x, in + 384 * i + 32 * k, 32);
            if (!limbs_below(x, FqParams::P)) { set_error("zkg_final_exp: element " + std::to_string(i) + " has a coefficient >= q"); return ZKG_ERROR; }
            for (int j = 0; j < 8; ++j) any = any || x[j];
        }
        if (!any) { set_error("zkg_final_exp: element " + std::to_string(i) + " is zero"); return ZKG_ERROR; }
    }
    if (!n) return ZKG_OK;
    if (where == 0) {
        for (size_t i = 0; i < n; ++i) { Fq12 f; ser::get_fq12(in + 384 * i, f); ser::put_fq12(out + 384 * i, pairing::final_exponentiation(f)); }
        return ZKG_OK;
    }
    if (where == 2) {
        for (size_t i = 0; i < n; ++i) final_exp_device_code_on_host(in + 384 * i, out + 384 * i);
        return ZKG_OK;
    }
    const size_t o_in = 0, o_ws = 384 * n, o_gt = o_ws + verify_final_exp_ws_bytes(n), total = o_gt + 384 * n + 16;
    WorkspaceLease lease;
    if (!(lease.w = verify_workspace_acquire()) || lease.w->buf.reserve(total)) return ZKG_ERROR;
    uint8_t *d = lease.w->buf.as<uint8_t>(); hipStream_t s = lease.w->s;
    ZK_HIP(hipMemcpyAsync(d + o_in, in, 384 * n, hipMemcpyHostToDevice, s));
    if (verify_final_exp_check(d + o_in, n, 1, d + o_ws, nullptr, nullptr, d + o_gt, s)) return ZKG_ERROR;
    ZK_HIP(hipMemcpyAsync(out, d + o_gt, 384 * n, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    return ZKG_OK;
}
int zkg_final_exp(const uint8_t *in, size_t n, int where, uint8_t *out) {
    return c_boundary("zkg_final_exp", ZKG_ERROR, [&] { return final_exp_impl(in, n, where, out); });
}

static int fq12_op_impl(int op, const uint32_t *a, const uint32_t *b, size_t n, int where, uint32_t *out) {
    if (op < 0 || op >= FQ12_OPS) { set_error("zkg_fq12_op: unknown operation"); return ZKG_ERROR; }
    if (where != 1 && where != 2) { set_error("zkg_fq12_op: where is 1 (GPU) or 2 (the device code on the host)"); return ZKG_ERROR; }
    if (where == 1 && initialised_device() < 0) { set_error("zkg_fq12_op: zkg_init not called (no GPU: the kernel has no CPU path)"); return ZKG_ERROR; }
    const bool binary = op == FQ12_MUL || op == FQ12_LINE;
    if (n && (!a || !out || (binary && !b))) { set_error("zkg_fq12_op: null argument"); return ZKG_ERROR; }
    if (n > ((size_t)1 << 20)) { set_error("zkg_fq12_op: at most 2^20 elements"); return ZKG_ERROR; }
    if (!n) return ZKG_OK;
    if (where == 2) {
        // the host build of fp.hip.hpp computes on canonical values: a coefficient >= q is refused, not reduced
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 12; ++k)
                if (!limbs_below(a + 96 * i + 8 * k, FqParams::P) || (binary && (op == FQ12_MUL || k < 6) && !limbs_below(b + 96 * i + 8 * k, FqParams::P))) {
                    set_error("zkg_fq12_op: element " + std::to_string(i) + " has a coefficient >= q (where = 2 takes canonical values)"); return ZKG_ERROR;
                }
        for (size_t i = 0; i < n; ++i) fq12_op_device_code_on_host(op, a + 96 * i, binary ? b + 96 * i : nullptr, out + 96 * i);
        return ZKG_OK;
    }
    const size_t o_a = 0, o_b = 384 * n, o_out = 2 * 384 * n, total = 3 * 384 * n;
    WorkspaceLease lease;
    if (!(lease.w = verify_workspace_acquire()) || lease.w->buf.reserve(total)) return ZKG_ERROR;
    uint8_t *d = lease.w->buf.as<uint8_t>(); hipStream_t s = lease.w->s;
    ZK_HIP(hipMemcpyAsync(d + o_a, a, 384 * n, hipMemcpyHostToDevice, s));
    if (binary) ZK_HIP(hipMemcpyAsync(d + o_b, b, 384 * n, hipMemcpyHostToDevice, s));
    if (verify_fq12_op(op, d + o_a, binary ? d + o_b : nullptr, n, d + o_out, s)) return ZKG_ERROR;
    ZK_HIP(hipMemcpyAsync(out, d + o_out, 384 * n, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    return ZKG_OK;
}
int zkg_fq12_op(int op, const uint32_t *a, const uint32_t *b, size_t n, int where, uint32_t *out) {
    return c_boundary("zkg_fq12_op", ZKG_ERROR, [&] { return fq12_op_impl(op, a, b, n, where, out); });
}

// bilinearity probe for the tests: writes e(a*G1, b*G2) (384 B) for canonical scalars a, b
int zkg_pairing_probe(const uint64_t a[4], const uint64_t b[4], uint8_t out[384]) {
    uint32_t ea[8], eb[8]; memcpy(ea, a, 32); memcpy(eb, b, 32);
    G1Affine P = G1::from_affine(g1_generator()).mul(ea, 8).to_affine();
    G2Affine Q = G2::from_affine(g2_generator()).mul(eb, 8).to_affine();
    ser::put_fq12(out, pairing::reduced_pairing(P, Q));
    return 0;
}

// test hook: 0 when (1) x -> x^(q^k) by coefficient maps equals square-and-multiply by q^k (k = 1, 2, 3) and (2) the last chunk of the
// final exponentiation equals square-and-multiply by the integer `e` (nlimbs x u32, little-endian) and (3) the projective and the
// affine Miller loops give the same reduced pairing products and (4) prepared lines give the same Miller value; bit flags otherwise
int zkg_pairing_selfcheck(const uint32_t *e, int nlimbs) {
    uint32_t k3[8] = {3}, k5[8] = {5};
    G1Affine P = G1::from_affine(g1_generator()).mul(k3, 8).to_affine();
    G2Affine Q = G2::from_affine(g2_generator()).mul(k5, 8).to_affine();
    Fq12 f = pairing::miller_loop(P, Q);
    int bad = 0;
    Fq12 x = f;
    for (int k = 1; k <= 3; ++k) { x = x.pow(FqParams::P, 8); if (!(x == pairing::frobenius(f, k))) bad |= 1 << (k - 1); }
    Fq12 g = pairing::final_exponentiation_first_chunk(f);
    if (!(g.conjugate() * g == Fq12::one())) bad |= 8;                        // in the cyclotomic subgroup: g^(q^6) = g^-1
    if (e && nlimbs > 0 && !(pairing::final_exponentiation_last_chunk(g) == g.pow(e, nlimbs))) bad |= 16;
    {   // the inversion-free lock-step Miller loop against the affine one of the definition: equal after the final exponentiation
        uint32_t k[6][8] = {{7}, {11}, {0x9e3779b9u, 0x7f4a7c15u, 0xf39cc060u, 5}, {13}, {0xdeadbeefu, 0x12345678u, 0xcafef00du, 0x0badc0deu, 0x31415926u, 0x27182818u, 0x16180339u, 0x1}, {17}};
        G1Affine Ps[3]; G2Affine Qs[3];
        for (int j = 0; j < 3; ++j) { Ps[j] = G1::from_affine(g1_generator()).mul(k[j], 8).to_affine(); Qs[j] = G2::from_affine(g2_generator()).mul(k[3 + j], 8).to_affine(); }
        for (int n = 1; n <= 3; ++n)
            if (!(pairing::final_exponentiation(pairing::multi_miller_loop(Ps, Qs, n)) == pairing::final_exponentiation(pairing::multi_miller_loop_affine(Ps, Qs, n)))) bad |= 32;
        // lines prepared ahead for two of the three pairs (a verification key's gamma and delta): the very same Miller value
        std::vector<pairing::LineCoeff> l1 = pairing::miller_lines(Qs[1]), l2 = pairing::miller_lines(Qs[2]);
        const std::vector<pairing::LineCoeff> *prep[3] = {nullptr, &l1, &l2};
        G2Affine unused[3] = {Qs[0], G2Affine::inf(), G2Affine::inf()};
        if (!(pairing::multi_miller_loop(Ps, unused, 3, prep) == pairing::multi_miller_loop(Ps, Qs, 3))) bad |= 64;
    }
    return bad;
}

}  // extern "C"

// the seam's entry (compat.hip): sizes in `cs`, the CSR arrays given up in `owned`
zkg_keypair *groth16_setup_owned(const zkg_r1cs *cs, zk::OwnedCsr *owned, const std::function<void()> &under_gpu) {
    return groth16_setup_impl(cs, nullptr, owned, under_gpu);
}

zkg_crs *crs_upload_device_queries(const zkg_pk *pk, const std::function<bool()> &constraint_system_ready);   // prover.hip

// a finished generator's keypair is destroyed on a thread of its own (one at a time: the next one, and seam_keygen_quiesce, wait for it)
// (the thread object lives on the heap and is never destroyed: a C caller that exits without zkg_shutdown must not meet the destructor of
//  a joinable std::thread; an atexit handler joins it before the runtime goes away)
static std::mutex &discard_mu() { static std::mutex *m = new std::mutex(); return *m; }
static std::thread &discard_thread() { static std::thread *t = new std::thread(); return *t; }
void seam_keygen_quiesce() {
    std::lock_guard<std::mutex> lk(discard_mu());
    if (discard_thread().joinable()) discard_thread().join();
}
static void keypair_discard(zkg_keypair *kp, int device) {
    static const bool registered = [] { return std::atexit(seam_keygen_quiesce) == 0; }();
    (void)registered;
    std::lock_guard<std::mutex> lk(discard_mu());
    if (discard_thread().joinable()) discard_thread().join();
    discard_thread() = std::thread([kp, device] { (void)hipSetDevice(device); delete kp; });
}

// The generator that leaves its key where it is made: zkg_groth16_setup_resident (a copied CSR, a trapdoor, no hooks) and
// libsnark_trusted_setup's generator (zklaim/libsnark_wrapper.cpp:195-215: an owned CSR, fresh randomness, under_gpu and on_blob) are this
// one function.  The reference's protocol is setup -> ONE prove -> verify per key (src/main_benchmark.c:113-148), so the key this call
// generates is the key the next proof needs: every scalar is computed on the device (as zkg_groth16_setup_dev computes them), the ~4n + m
// query points are computed into device buffers and stay there as the resident key (zkg_crs, H table included); the pk blob the caller
// receives is assembled from GPU-compressed records (34 / 100 bytes per point instead of 64 / 192 over PCIe, no host point vectors at
// all) around the constraint rows' text, which the host pool writes meanwhile.  Same bytes as zkg_keypair_pk_blob writes.
// pk / vk: malloc'd (the caller's to free).  crs_out NULL: no resident key is built.  on_blob runs on a thread of its own as soon as the pk
// blob is complete (the seam hashes it).
int setup_resident_core(const zkg_r1cs *cs, const uint64_t *trapdoor, zk::OwnedCsr *owned, const std::function<void()> &under_gpu,
                        unsigned char **pk_out, size_t *pk_len, unsigned char **vk_out, size_t *vk_len, zkg_crs **crs_out,
                        const std::function<void(const unsigned char *, size_t)> &on_blob) {
    static const bool dbg = getenv("ZKG_DEBUG_TIMING") != nullptr;
    auto t_begin = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) { if (dbg) fprintf(stderr, "[zkg seam keygen] %-26s %8.3f ms\n", what, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count()); };
    *pk_out = *vk_out = nullptr; if (crs_out) *crs_out = nullptr;
    t_setup_resident_stats[0] = t_setup_resident_stats[1] = t_setup_resident_stats[2] = 0;
    // ---- the constraint rows' text starts as soon as the generator has fixed the system it stores (a thread of its own that fans out over
    //      the host pool): it is the longest host-only part of the blob and needs nothing the GPU computes
    int device = 0; (void)hipGetDevice(&device);                               // threads started below bind to the caller's device
    std::unique_ptr<zkg_keypair> kp;                                            // (declared first: outlives every thread that reads it)
    std::vector<ser::Writer> rows_part; bool rows_ok = true;
    std::thread rows_thread;
    struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } join_rows{rows_thread};
    kp.reset(groth16_setup_impl(cs, trapdoor, owned, under_gpu, SetupMode::Resident,
        [&](zkg_keypair *k) { rows_thread = std::thread([&rows_part, &rows_ok, k] { try { constraint_rows_text(k, rows_part); } catch (...) { rows_ok = false; } }); },
        [&] { if (rows_thread.joinable()) rows_thread.join(); }));
    if (!kp) return ZKG_ERROR;
    lap("points on the device");
    // ---- the resident key is built from the device queries on a thread of its own (null stream: H table, constraint system upload, comb
    //      tables, domain, prover slot) while this thread turns the same queries into the blob's records on a stream of its own
    zkg_crs *crs = nullptr;
    std::thread crs_thread;
    if (crs_out) crs_thread = std::thread([&] { try { (void)hipSetDevice(device); crs = crs_upload_device_queries(&kp->pk_view, nullptr); } catch (...) { crs = nullptr; } });
    struct JoinCrs { std::thread &t; zkg_crs *&c; bool keep = false; ~JoinCrs() { if (t.joinable()) t.join(); if (!keep && c) { zkg_crs_free(c); c = nullptr; } } } join_crs{crs_thread, crs};
    // ---- layout: everything before the constraint rows has a known size
    const size_t nA = (size_t)kp->n + 1, nidx = kp->b_idx.size(), nH = kp->m - 1, nL = (size_t)kp->n - kp->l;
    ser::Writer seg[5];
    seg[0].g1(kp->alpha_g1); seg[0].g1(kp->beta_g1); seg[0].g2(kp->beta_g2); seg[0].g1(kp->delta_g1); seg[0].g2(kp->delta_g2); seg[0].dec(nA);
    seg[1].buf.reserve(nidx * 8 + 64);
    seg[1].dec(nA); seg[1].dec(nidx); for (uint32_t i : kp->b_idx) seg[1].dec(i); seg[1].dec(nidx);
    seg[2].dec(nH); seg[3].dec(nL); seg[4].dec(kp->l); seg[4].dec(kp->n - kp->l); seg[4].dec(kp->C);
    const size_t run[4] = {nA * 34, nidx * 100, nH * 34, nL * 34};
    size_t at_seg[5], at_run[4], pos = 0;
    for (int i = 0; i < 5; ++i) { at_seg[i] = pos; pos += seg[i].buf.size(); if (i < 4) { at_run[i] = pos; pos += run[i]; } }
    const size_t rows_at = pos;
    size_t terms = 0; for (int k = 0; k < 3; ++k) terms += kp->col[k].size();
    const size_t rows_bound = terms * 44 + (size_t)kp->C * 3 * 12 + 64;        // an index is at most 10 digits + '\n', a count likewise
    unsigned char *pk = (unsigned char *)malloc(rows_at + rows_bound);          // (untouched pages of the bound cost nothing; shrunk below)
    if (!pk) { set_error("resident generator: out of memory"); return ZKG_ERROR; }
    struct FreeOnExit { unsigned char *&p; ~FreeOnExit() { free(p); } } free_pk{pk};
    for (int i = 0; i < 5; ++i) memcpy(pk + at_seg[i], seg[i].buf.data(), seg[i].buf.size());
    // ---- the GPU compresses the points into the blob's records; they come back, run by run, straight into the blob
    {
        ScopedDevBuf d_rec;
        hipStream_t st = nullptr;
        if (!hip_ok(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate", __FILE__, __LINE__)) return ZKG_ERROR;
        struct DropStream { hipStream_t s; ~DropStream() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } drop_stream{st};
        size_t off[4], total = 0;
        for (int i = 0; i < 4; ++i) { off[i] = total; total += (run[i] + 15) & ~(size_t)15; }
        if (d_rec.reserve(total + 16)) return ZKG_ERROR;
        uint8_t *r = d_rec.as<uint8_t>();
        if (compress_g1_records(kp->dA.as<G1Affine>(), nA, r + off[0], st) || compress_kc_records(kp->dB2.as<G2Affine>(), kp->dB1.as<G1Affine>(), kp->dBidx.as<uint32_t>(), nidx, r + off[1], st) ||
            compress_g1_records(kp->dH.as<G1Affine>(), nH, r + off[2], st) || compress_g1_records(kp->dL.as<G1Affine>(), nL, r + off[3], st)) { set_error("resident generator: compression launch failed"); return ZKG_ERROR; }
        for (int i = 0; i < 4; ++i)
            if (run[i] && !hip_ok(hipMemcpyAsync(pk + at_run[i], r + off[i], run[i], hipMemcpyDeviceToHost, st), "D2H", __FILE__, __LINE__)) return ZKG_ERROR;
        if (!hip_ok(hipStreamSynchronize(st), "sync", __FILE__, __LINE__)) return ZKG_ERROR;
    }
    lap("records compressed + copied");
    rows_thread.join();
    size_t rows_len = 0;
    if (rows_ok) {
        std::vector<size_t> at(rows_part.size() + 1, rows_at);
        for (size_t i = 0; i < rows_part.size(); ++i) at[i + 1] = at[i] + rows_part[i].buf.size();
        rows_len = at.back() - rows_at;
        if (rows_len > rows_bound) rows_ok = false;
        else host_parallel_for((int)rows_part.size(), [&](int i) { if (!rows_part[i].buf.empty()) memcpy(pk + at[i], rows_part[i].buf.data(), rows_part[i].buf.size()); });
    }
    if (!rows_ok) { set_error("resident generator: constraint rows failed"); return ZKG_ERROR; }
    const size_t len = rows_at + rows_len;
    { unsigned char *shrunk = (unsigned char *)realloc(pk, len); if (shrunk) pk = shrunk; }
    lap("pk blob complete");
    std::thread blob_thread;
    if (on_blob) blob_thread = std::thread([&] { try { on_blob(pk, len); } catch (...) {} });
    struct Join2 { std::thread &t; ~Join2() { if (t.joinable()) t.join(); } } join_blob{blob_thread};
    // ---- vk (l + 1 points, host)
    const size_t vlen = zkg_keypair_vk_blob(kp.get(), nullptr, 0);
    unsigned char *vk = (unsigned char *)malloc(vlen);
    if (!vk || zkg_keypair_vk_blob(kp.get(), vk, vlen) != vlen) { free(vk); set_error("resident generator: vk blob failed"); return ZKG_ERROR; }
    if (crs_thread.joinable()) crs_thread.join();
    lap("resident key built");
    if (crs_out && !crs) { free(vk); return ZKG_ERROR; }
    if (blob_thread.joinable()) blob_thread.join();
    join_crs.keep = true;
    // the keypair's host vectors (the constraint system, 100 MB at 20 payloads) and device queries go back to their allocators on a thread
    // of their own: nothing below needs them
    keypair_discard(kp.release(), device);
    *pk_out = pk; *pk_len = len; *vk_out = vk; *vk_len = vlen; if (crs_out) *crs_out = crs;
    pk = nullptr;                                                               // handed over
    return ZKG_OK;
}

extern "C" {

int zkg_groth16_setup_resident(const zkg_r1cs *cs, const uint64_t *trapdoor, uint8_t **pk_blob, size_t *pk_len, uint8_t **vk_blob, size_t *vk_len, zkg_crs **crs) {
    return c_boundary("zkg_groth16_setup_resident", ZKG_ERROR, [&] {
        if (!cs || !pk_blob || !pk_len || !vk_blob || !vk_len) { set_error("zkg_groth16_setup_resident: null argument"); return ZKG_ERROR; }
        if (initialised_device() < 0) { set_error("zkg_groth16_setup_resident: zkg_init not called"); return ZKG_ERROR; }
        unsigned char *pk = nullptr, *vk = nullptr; size_t plen = 0, vlen = 0; zkg_crs *key = nullptr;
        if (setup_resident_core(cs, trapdoor, nullptr, nullptr, &pk, &plen, &vk, &vlen, crs ? &key : nullptr, nullptr) != ZKG_OK) {
            set_error(std::string("zkg_groth16_setup_resident: ") + zkg_last_error());       // the out-pointers are left alone
            return ZKG_ERROR;
        }
        *pk_blob = pk; *pk_len = plen; *vk_blob = vk; *vk_len = vlen;
        if (crs) *crs = key;
        return ZKG_OK;
    });
}
void zkg_free(void *p) { free(p); }
void zkg_setup_resident_stats(size_t out[3]) { if (out) for (int i = 0; i < 3; ++i) out[i] = t_setup_resident_stats[i]; }

// test hook: the generator's non-zero index (where 1) against a plain host loop (where 0) on raw limbs — any representative below 2r
int zkg_fr_nonzero_index(const uint64_t *fr, size_t n, int where, uint32_t *idx_out, size_t *count) {
    return c_boundary("zkg_fr_nonzero_index", ZKG_ERROR, [&] {
        if (!count || (n && (!fr || !idx_out)) || (where != 0 && where != 1)) { set_error("zkg_fr_nonzero_index: bad argument"); return ZKG_ERROR; }
        if (n > NZ_MAX) { set_error("zkg_fr_nonzero_index: more than 2^28 elements"); return ZKG_ERROR; }
        if (where == 0) {
            size_t c = 0;
            for (size_t i = 0; i < n; ++i) {
                uint32_t v[8]; memcpy(v, fr + 4 * i, 32);
                uint32_t o = 0, q = 0;
                for (int k = 0; k < 8; ++k) { o |= v[k]; q |= v[k] ^ FrParams::P[k]; }
                if (o != 0 && q != 0) idx_out[c++] = (uint32_t)i;
            }
            *count = c;
            return ZKG_OK;
        }
        if (initialised_device() < 0) { set_error("zkg_fr_nonzero_index: zkg_init not called"); return ZKG_ERROR; }
        if (!n) { *count = 0; return ZKG_OK; }
        // idx: n entries and a guard of 64 behind them, all ones before the kernels run — whatever lies behind the count must still be so
        const size_t guard = 64, words = n + guard;
        ScopedDevBuf d_v, d_w;
        if (d_v.reserve(n * 32) || d_w.reserve((words + 1 + nonzero_index_blocks(n)) * 4)) return ZKG_ERROR;
        uint32_t *d_idx = d_w.as<uint32_t>(), *d_count = d_idx + words, *d_blocks = d_count + 1;
        ZK_HIP(hipMemcpy(d_v.p, fr, n * 32, hipMemcpyHostToDevice));
        ZK_HIP(hipMemsetAsync(d_idx, 0xff, (words + 1) * 4, nullptr));
        if (nonzero_index_dev(d_v.as<Fr>(), n, d_idx, d_count, d_blocks, nullptr)) return ZKG_ERROR;
        std::vector<uint32_t> back(words + 1);
        ZK_HIP(hipMemcpy(back.data(), d_idx, (words + 1) * 4, hipMemcpyDeviceToHost));
        const size_t c = back[words];
        if (c > n) { set_error("zkg_fr_nonzero_index: count above n"); return ZKG_ERROR; }
        for (size_t i = c; i < words; ++i) if (back[i] != 0xffffffffu) { set_error("zkg_fr_nonzero_index: an entry behind the count was written"); return ZKG_ERROR; }
        memcpy(idx_out, back.data(), c * 4);
        *count = c;
        return ZKG_OK;
    });
}

}  // extern "C"
