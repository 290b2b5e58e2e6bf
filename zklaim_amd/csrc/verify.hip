// verify.hip — device kernels of the batch Groth16 verifier (zkg_groth16_verify_batch, zkg_pairing_product; host side in setup_verify.hip).
//
// Every kernel runs one independent item per lane:
//   k_g2_subgroup   [r]B == O for each proof's B (the random weights are sound only for B in G2; libsnark's is_well_formed checks
//                   the curve equation only)
//   k_g1_mul128     r_i * P_i for the 128-bit weights (A_i and C_i in one launch: lane i uses weight i mod nw), affine out
//   k_miller        ML(P_i, Q_i) (pairing.hip.hpp), 1 for a pair with a point at infinity or flagged out
//   k_fq12_prod     the product of the Miller values of an index range [lo, hi): per block a strided product and an LDS tree; a second
//                   launch of one block folds the block results
// the per-proof verifier (zkg_groth16_verify_each, zkg_pairing_each), which decides every item by its own equation:
//   k_ic_each           -(IC_0 + sum_k x_ik IC_k) per item: a block per item, lanes stride over k, an LDS tree adds the lanes
//   k_g2_replicate      the key's gamma and delta behind the proofs' B, so that k_miller runs over [A | -acc | -C] x [B | gamma.. | delta..]
//   k_final_exp_check   per lane the product of an item's Miller values and its final exponentiation (final_exp.hip.hpp); the verdict
//                       (== the key's alpha_beta) or the GT value itself
//   k_fq12_op           one operation of the tower per lane on raw, unnormalised limbs: the known-answer hook zkg_fq12_op, on no verifier's path
// and the device front end of the seam's batch entry (zkg_zklaim_verify_batch), which leaves the host neither square roots nor input sums:
//   k_proof_decode        a compressed point of a 134-byte proof record per lane -> the affine Montgomery point ser::get_g1 / ser::get_g2
//                         produce and a flag byte per item (the single verifier's acceptance rule and coords_canonical, bit for bit)
//   k_zklaim_input_sums   s_k = sum over the entering positions of a range of weight_p * x_pk, the public inputs x_pk assembled from the
//                         payloads' public bytes (zklaim_public.hip.hpp); a block per (element, slice), k_fr_fold adds the slices
// and the accumulator of the seam's per-proof entry (zkg_zklaim_verify_each), which works from the same public records:
//   k_zklaim_bit_chain, k_zklaim_bit_affine   per key, once: T[s] = 2^(s mod 253) IC_(s / 253) for every string bit s, affine
//   k_zklaim_ic_each      -(IC_0 + sum_k x_ik IC_k) per item as the sum of T over the string's set bits: a wavefront per item, the lanes
//                         stride over the string's bytes, an LDS tree adds the lanes; no doubling, no Fr
#include "common.hpp"
#include "pairing.hip.hpp"
#include "final_exp.hip.hpp"
#include "sqrt.hip.hpp"
#include "zklaim_public.hip.hpp"
#include "host/pairing.hpp"
#include "../../include/zkg.h"

namespace zk {
namespace {

constexpr int VB = 64;                                 // one wavefront per block: the lanes carry no shared state

// r, the order of G1 / G2 (FrParams::P), as 254 bits read from the top
__global__ __launch_bounds__(VB) void k_g2_subgroup(size_t n, const G2Affine *B, uint8_t *ok) {
    size_t i = (size_t)blockIdx.x * VB + threadIdx.x;
    if (i >= n) return;
    const G2Affine b = B[i];
    if (b.is_inf()) { ok[i] = 1; return; }
    G2 acc = G2::inf();
#pragma unroll 1
    for (int bit = 253; bit >= 0; --bit) {              // the same scalar in every lane: no divergence
        acc = acc.dbl();
        if ((FrParams::P[bit >> 5] >> (bit & 31)) & 1u) acc.madd(b);
    }
    ok[i] = acc.is_inf() ? 1 : 0;
}

__global__ __launch_bounds__(VB) void k_g1_mul128(size_t n, const G1Affine *in, const uint32_t *w, size_t nw, G1Affine *out) {
    size_t i = (size_t)blockIdx.x * VB + threadIdx.x;
    if (i >= n) return;
    const G1Affine a = in[i];
    const size_t wi = i % nw;
    const uint32_t k[4] = {w[4 * wi], w[4 * wi + 1], w[4 * wi + 2], w[4 * wi + 3]};
    G1 acc = G1::inf();
#pragma unroll 1
    for (int bit = 127; bit >= 0; --bit) {
        acc = acc.dbl();
        if ((k[bit >> 5] >> (bit & 31)) & 1u) acc.madd(a);
    }
    out[i] = acc.to_affine().normalized();
}

__global__ __launch_bounds__(VB) void k_miller(size_t n, const G1Affine *P, const G2Affine *Q, const uint8_t *use, MillerConsts kc, dev::Fq12 *out) {
    size_t i = (size_t)blockIdx.x * VB + threadIdx.x;
    if (i >= n) return;
    const G1Affine p = P[i]; const G2Affine q = Q[i];
    dev::Fq12 f = dev::Fq12::one();
    if ((!use || use[i]) && !p.is_inf() && !q.is_inf()) f = dev::miller_loop(p, q, kc);
    out[i] = f.normalized();
}

__global__ __launch_bounds__(VB) void k_fq12_prod(const dev::Fq12 *in, size_t lo, size_t hi, dev::Fq12 *out) {
    __shared__ dev::Fq12 sh[VB];
    const size_t n = hi - lo, b0 = lo + n * blockIdx.x / gridDim.x, b1 = lo + n * (blockIdx.x + 1) / gridDim.x;
    dev::Fq12 acc = dev::Fq12::one();
#pragma unroll 1
    for (size_t j = b0 + threadIdx.x; j < b1; j += VB) acc = acc * in[j];
    sh[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll 1
    for (int s = VB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] * sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0].normalized();
}

// out[i] = -(ic0 + sum_k x[i * nidx + k] * ic[k]), affine and canonical (infinity: all-zero).  x: Montgomery Fr, as the verifier's inputs are
// given.  One block per item; lane t takes the terms t, t + VB, ..: a 254-step double-and-add each (the scalars differ per lane, so the
// additions diverge), summed per lane, then an LDS tree over the lanes.
__global__ __launch_bounds__(VB) void k_ic_each(size_t n, uint32_t nidx, const G1Affine *ic0, const G1Affine *ic, const Fr *x, G1Affine *out) {
    __shared__ G1 sh[VB];
    const size_t i = blockIdx.x;                        // gridDim.x == n
    G1 sum = G1::inf();
#pragma unroll 1
    for (uint32_t k = threadIdx.x; k < nidx; k += VB) {
        const G1Affine b = ic[k];
        const Fr e = x[i * nidx + k].from_mont();
        G1 acc = G1::inf();
#pragma unroll 1
        for (int bit = 253; bit >= 0; --bit) {          // x < r < 2^254
            acc = acc.dbl();
            if ((e.v[bit >> 5] >> (bit & 31)) & 1u) acc.madd(b);
        }
        sum.add(acc);
    }
    sh[threadIdx.x] = sum;
    __syncthreads();
#pragma unroll 1
    for (int s = VB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { G1 a = sh[threadIdx.x]; a.add(sh[threadIdx.x + s]); sh[threadIdx.x] = a; }
        __syncthreads();
    }
    if (threadIdx.x == 0 && i < n) {
        G1 acc = G1::from_affine(*ic0);
        acc.add(sh[0]);
        out[i] = acc.neg().to_affine().normalized();
    }
}
// Q[n + i] = key[0], Q[2 n + i] = key[1] for i < n
__global__ __launch_bounds__(VB) void k_g2_replicate(size_t n, const G2Affine *key, G2Affine *Q) {
    const size_t i = (size_t)blockIdx.x * VB + threadIdx.x;
    if (i < 2 * n) Q[n + i] = key[i / n];
}
// lane i: f = M[i] M[n + i] .. M[(pairs - 1) n + i], then FE(f).  ab != null: verdict[i] = FE(f) == *ab ? 0 : 1 (ab canonical);
// gt != null: gt[i] = FE(f), canonical.  pairs >= 1.  ws: FE_SLOTS x 96 x stride words, stride >= n.
__global__ __launch_bounds__(VB) void k_final_exp_check(size_t n, const dev::Fq12 *M, uint32_t pairs, uint32_t *ws, size_t stride, FrobConsts fc,
                                                        const dev::Fq12 *ab, uint8_t *verdict, dev::Fq12 *gt) {
    // the Frobenius constants in LDS: as kernel arguments their 240 words are all loaded ahead of the chain's loop and spilled
    __shared__ FrobConsts sfc;
    for (uint32_t t = threadIdx.x; t < sizeof(FrobConsts) / 4; t += VB) reinterpret_cast<uint32_t *>(&sfc)[t] = reinterpret_cast<const uint32_t *>(&fc)[t];
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * VB + threadIdx.x;
    if (i >= n) return;
    const dev::FeSlots slots{ws, (uint32_t)i, stride};
    dev::Fq12 g = dev::final_exponentiation(M[i], (int)pairs - 1, [&](int j) { return M[(size_t)j * n + i]; }, sfc, slots).normalized();
    if (gt) gt[i] = g;
    if (ab) {
        const uint32_t *a = reinterpret_cast<const uint32_t *>(ab);
        uint32_t diff = 0;
        dev::FeSlots::each_fq(g, [&](Fq &c, int k) {
#pragma unroll
            for (int j = 0; j < 8; ++j) diff |= c.v[j] ^ a[8 * k + j];
        });
        verdict[i] = diff ? 1 : 0;
    }
}

// one operation of the tower on raw limbs (the known-answer hook zkg_fq12_op): the functions of pairing.hip.hpp and final_exp.hip.hpp
// themselves.  Nothing is normalised, so a caller sees the lazy representative the operation leaves.  b: the second factor (FQ12_MUL) or
// the line's a, b, c in its c0 (FQ12_LINE).
template <int OP> ZK_HD dev::Fq12 fq12_op_apply(const dev::Fq12 &a, const dev::Fq12 &b, const FrobConsts &fc) {
    if constexpr (OP == FQ12_MUL) return a * b;
    else if constexpr (OP == FQ12_SQR) return a.sqr();
    else if constexpr (OP == FQ12_LINE) return dev::mul_by_line2(a, b.c0.c0, b.c0.c1, b.c0.c2);
    else if constexpr (OP == FQ12_CSQR) return dev::cyclotomic_sqr(a);
    else if constexpr (OP == FQ12_INV) return dev::inverse(a);
    else if constexpr (OP == FQ12_CONJ) return dev::conjugate(a);
    else if constexpr (OP == FQ12_FROB1) return dev::frobenius<1>(a, fc);
    else if constexpr (OP == FQ12_FROB2) return dev::frobenius<2>(a, fc);
    else if constexpr (OP == FQ12_FROB3) return dev::frobenius<3>(a, fc);
    else return {a.c0.mul_by_v(), a.c1.mul_by_v()};
}
// lane i: out[i] = op(a[i], b[i]); b is read by the operations that have a second operand only
template <int OP> __global__ __launch_bounds__(VB) void k_fq12_op(size_t n, const dev::Fq12 *a, const dev::Fq12 *b, FrobConsts fc, dev::Fq12 *out) {
    const size_t i = (size_t)blockIdx.x * VB + threadIdx.x;
    if (i >= n) return;
    const dev::Fq12 x = a[i];
    out[i] = fq12_op_apply<OP>(x, (OP == FQ12_MUL || OP == FQ12_LINE) ? b[i] : x, fc);
}

// ---- the device front end (limbs_below_q, coords_canonical's test: sqrt.hip.hpp)
ZK_D bool decode_g1(const uint8_t *p, G1Affine &out) {   // ser::get_g1 && coords_canonical
    out = G1Affine::inf();
    if (p[0] == '1') return true;                       // infinity: nothing else is read
    if (p[0] != '0' || (p[33] != '0' && p[33] != '1')) return false;
    const Fq x = load_fq_bytes(p + 1);
    if (!limbs_below_q(x)) return false;
    const Fq rhs = x.sqr() * x + Fq::from_u64(3);
    Fq y = fq_sqrt_candidate(rhs);
    if (y.sqr() != rhs) return false;
    if (((y.from_mont().v[0] & 1u) != 0) != (p[33] == '1')) y = y.neg();
    out = G1Affine{x, y}.normalized();
    return true;
}
ZK_D bool decode_g2(const uint8_t *p, G2Affine &out) {   // ser::get_g2 && coords_canonical
    out = G2Affine::inf();
    if (p[0] == '1') return true;
    if (p[0] != '0' || (p[65] != '0' && p[65] != '1')) return false;
    const Fq2 x = {load_fq_bytes(p + 1), load_fq_bytes(p + 33)};
    if (!limbs_below_q(x.c0) || !limbs_below_q(x.c1)) return false;
    Fq2 b;                                              // the twist's coefficient 3 / (9 + u), Montgomery limbs
    { const uint32_t b0[8] = {0x77b802a8u, 0x3bf938e3u, 0x3633535du, 0x020b1b27u, 0x49755260u, 0x26b7edf0u, 0x4384a86du, 0x2514c632u};
      const uint32_t b1[8] = {0xd1dcff67u, 0x38e7ecccu, 0x93ce0d3eu, 0x65f0b37du, 0x22ac00aau, 0xd749d0ddu, 0x4a688d4du, 0x0141b9ceu};
      for (int k = 0; k < 8; ++k) { b.c0.v[k] = b0[k]; b.c1.v[k] = b1[k]; } }
    const Fq2 rhs = x.sqr() * x + b;
    Fq2 y;
    if (!fq2_sqrt(rhs, y)) return false;
    if (((y.c0.from_mont().v[0] & 1u) != 0) != (p[65] == '1')) y = y.neg();
    out = G2Affine{x, y}.normalized();
    return true;
}
// records of ZKG_PROOF_BYTES: A at 0, B at 34, C at 100.  g2 != 0: lane i decodes B of record i into out2[i].  g2 == 0: 2 n lanes, lane i < n
// decodes A of record i, lane n + i its C, into out1[lane] (A and C back to back, as k_g1_mul128 reads them).  dec[lane] = 1 iff the point
// decoded; a point that did not is stored as infinity (all-zero).
__global__ __launch_bounds__(VB) void k_proof_decode(const uint8_t *rec, size_t n, int g2, G1Affine *out1, G2Affine *out2, uint8_t *dec) {
    const size_t i = (size_t)blockIdx.x * VB + threadIdx.x;
    if (g2) {
        if (i >= n) return;
        G2Affine q;
        dec[i] = decode_g2(rec + i * ZKG_PROOF_BYTES + 34, q) ? 1 : 0;
        out2[i] = q;
    } else {
        if (i >= 2 * n) return;
        G1Affine p;
        dec[i] = decode_g1(i < n ? rec + i * ZKG_PROOF_BYTES : rec + (i - n) * ZKG_PROOF_BYTES + 100, p) ? 1 : 0;
        out1[i] = p;
    }
}
// use[i] = the item enters the combination: B in G2 and A, B, C decoded (dec_ac: n flags of A, then n of C)
__global__ __launch_bounds__(VB) void k_use_mask(size_t n, const uint8_t *in_g2, const uint8_t *dec_b, const uint8_t *dec_ac, uint8_t *use) {
    const size_t i = (size_t)blockIdx.x * VB + threadIdx.x;
    if (i < n) use[i] = in_g2[i] && dec_b[i] && dec_ac[i] && dec_ac[n + i] ? 1 : 0;
}

// block (k, slice): the slice's share of positions [lo, hi); position p reads its npl records at pub + (p - base) * npl * ZV_REC, its
// 128-bit weight at w + 4 p and mask[p] (optional).  The product of the two raw values is r x / R; R^2 twice on the block's sum makes it
// the Montgomery form of sum r x.  out[slice * l + k].
__global__ __launch_bounds__(VB) void k_zklaim_input_sums(const uint8_t *pub, uint32_t npl, size_t base, const uint32_t *w, const uint8_t *mask,
                                                          size_t lo, size_t hi, uint32_t l, Fr *out) {
    __shared__ Fr sh[VB];
    const uint32_t k = blockIdx.x;
    const size_t n = hi - lo, b0 = lo + n * blockIdx.y / gridDim.y, b1 = lo + n * (blockIdx.y + 1) / gridDim.y;
    Fr acc = Fr::zero();
#pragma unroll 1
    for (size_t p = b0 + threadIdx.x; p < b1; p += VB) {
        if (mask && !mask[p]) continue;
        Fr x, r = Fr::zero();
        zv_input_element(pub + (p - base) * npl * ZV_REC, npl, k, x.v);
#pragma unroll
        for (int j = 0; j < 4; ++j) r.v[j] = w[4 * p + j];
        acc += r * x;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll 1
    for (int s = VB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)blockIdx.y * l + k] = (sh[0] * Fr::r2() * Fr::r2()).normalized();
}
__global__ __launch_bounds__(VB) void k_fr_fold(const Fr *part, uint32_t l, uint32_t slices, Fr *out) {
    const uint32_t k = blockIdx.x * VB + threadIdx.x;
    if (k >= l) return;
    Fr acc = part[k];
#pragma unroll 1
    for (uint32_t s = 1; s < slices; ++s) acc += part[(size_t)s * l + k];
    out[k] = acc.normalized();
}

// ---- the seam's per-proof entry (zkg_zklaim_verify_each): -(IC_0 + sum_k x_ik IC_k) from the payloads' public records.  An input map is
// a bit string and element k holds its bits [253 k, 253 k + 253), so the sum is the sum of T[s] = 2^(s mod 253) IC_(s / 253) over the
// string's set bits s: a table per key, indexed by the string bit, and per item nothing but mixed additions.  The bodies are ZK_HD: the
// hook's where = 2 runs them on the host (zklaim_ic_each_device_code_on_host).
// the doubling chain of one element: tmp[b] = 2^b p, b < 253 (infinity stays infinity)
ZK_HD void zv_bit_table_chain(const G1Affine &p, G1 *tmp) {
    G1 a = G1::from_affine(p);
#pragma unroll 1
    for (uint32_t b = 0; b < ZV_FR_CAPACITY; ++b) { tmp[b] = a.normalized(); a = a.dbl(); }
}
// the stored form of a chain value: affine and canonical, all-zero for infinity (an inversion of its own: the entries are lanes)
ZK_HD G1Affine zv_bit_table_entry(const G1 &t) { return t.to_affine().normalized(); }
// what lane `lane` of an item's wavefront adds up: the table entries of the set bits of the string bytes lane, lane + VB, ..
// (zv_string_byte reverses a byte's bits, so bit j of its value is string bit 8 B + j).  madd is complete: an entry that meets the running
// sum itself, its negative or infinity comes out right.
ZK_HD G1 zv_ic_lane_sum(const G1Affine *T, const uint8_t *rec, uint32_t npl, uint32_t lane) {
    G1 sum = G1::inf();
#pragma unroll 1
    for (uint32_t B = lane; B < ZV_STRING_BYTES * npl; B += VB) {
        uint32_t v = zv_string_byte(rec, npl, B);
#pragma unroll 1
        while (v) {
            const uint32_t j = (uint32_t)__builtin_ctz(v);
            v &= v - 1u;
            sum.madd(T[8u * B + j]);
        }
    }
    return sum;
}
// -(ic0 + the lanes' sum), affine and canonical (infinity: all-zero)
ZK_HD G1Affine zv_ic_finish(const G1Affine &ic0, const G1 &lanes_sum) {
    G1 acc = G1::from_affine(ic0);
    acc.add(lanes_sum);
    return acc.neg().to_affine().normalized();
}

// lane k: the chain of element k into tmp + 253 k (tmp: 253 l XYZZ points)
__global__ __launch_bounds__(VB) void k_zklaim_bit_chain(uint32_t l, const G1Affine *ic, G1 *tmp) {
    const uint32_t k = blockIdx.x * VB + threadIdx.x;
    if (k < l) zv_bit_table_chain(ic[k], tmp + (size_t)ZV_FR_CAPACITY * k);
}
// lane s: T[s] for the string bits a payload can set, s < entries <= 253 l
__global__ __launch_bounds__(VB) void k_zklaim_bit_affine(size_t entries, const G1 *tmp, G1Affine *T) {
    const size_t s = (size_t)blockIdx.x * VB + threadIdx.x;
    if (s < entries) T[s] = zv_bit_table_entry(tmp[s]);
}
// out[i] = -(ic0 + sum_k x_ik IC_k) for the item whose npl public records lie at pub + i * npl * ZV_REC.  One wavefront per item
// (gridDim.x == n): the lanes' sums, an LDS tree over the lanes, lane 0 finishes.  c_in != null: the last lane also stores
// c_neg[i] = -c_in[i] (the proof's C behind the sums; c_in may be `out`: the lane reads before the first barrier, lane 0 writes after the last)
__global__ __launch_bounds__(VB) void k_zklaim_ic_each(size_t n, uint32_t npl, const G1Affine *ic0, const G1Affine *T, const uint8_t *pub, G1Affine *out,
                                                       const G1Affine *c_in, G1Affine *c_neg) {
    __shared__ G1 sh[VB];
    const size_t i = blockIdx.x;
    if (c_in && threadIdx.x == VB - 1 && i < n) {
        const G1Affine c = c_in[i];
        c_neg[i] = c.is_inf() ? G1Affine::inf() : c.neg().normalized();
    }
    sh[threadIdx.x] = zv_ic_lane_sum(T, pub + i * npl * ZV_REC, npl, threadIdx.x);
    __syncthreads();
#pragma unroll 1
    for (int s = VB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { G1 a = sh[threadIdx.x]; a.add(sh[threadIdx.x + s]); sh[threadIdx.x] = a; }
        __syncthreads();
    }
    if (threadIdx.x == 0 && i < n) out[i] = zv_ic_finish(*ic0, sh[0]);
}

unsigned blocks_for(size_t n) { return (unsigned)((n + VB - 1) / VB); }

}  // namespace

size_t zklaim_bit_table_entries(uint32_t npl) { return (size_t)ZV_STRING_BYTES * 8 * npl; }
size_t zklaim_bit_table_tmp_bytes(uint32_t npl) { return (size_t)ZV_FR_CAPACITY * zv_input_count(npl) * sizeof(G1); }
// d_ic: the l = zv_input_count(npl) points of the key, dense (infinity where the key has none); d_tmp: zklaim_bit_table_tmp_bytes(npl);
// d_T: zklaim_bit_table_entries(npl) affine points
int verify_zklaim_bit_table(const G1Affine *d_ic, uint32_t npl, void *d_tmp, G1Affine *d_T, hipStream_t s) {
    const uint32_t l = zv_input_count(npl);
    const size_t entries = zklaim_bit_table_entries(npl);
    if (!l) return ZKG_OK;
    hipLaunchKernelGGL(k_zklaim_bit_chain, dim3(blocks_for(l)), dim3(VB), 0, s, l, d_ic, (G1 *)d_tmp);
    ZK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_zklaim_bit_affine, dim3(blocks_for(entries)), dim3(VB), 0, s, entries, (const G1 *)d_tmp, d_T);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
// d_out[i] = -(ic0 + sum_k x_ik IC_k), i < n, from d_pub's n x npl public records; d_c (optional): d_negc[i] = -d_c[i]
int verify_zklaim_ic_each(const G1Affine *d_ic0, const G1Affine *d_T, const uint8_t *d_pub, uint32_t npl, size_t n, G1Affine *d_out,
                          const G1Affine *d_c, G1Affine *d_negc, hipStream_t s) {
    if (!n) return ZKG_OK;
    hipLaunchKernelGGL(k_zklaim_ic_each, dim3((unsigned)n), dim3(VB), 0, s, n, npl, d_ic0, d_T, d_pub, d_out, d_c, d_negc);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
// the same text on the host (zkg_zklaim_ic_each, where = 2): the table, then per item the VB lane sums, the tree in the kernel's order, the finish
void zklaim_ic_each_device_code_on_host(const G1Affine &ic0, const G1Affine *ic, const uint8_t *pub, uint32_t npl, size_t n, G1Affine *out) {
    const uint32_t l = zv_input_count(npl);
    std::vector<G1> tmp((size_t)ZV_FR_CAPACITY * l);
    for (uint32_t k = 0; k < l; ++k) zv_bit_table_chain(ic[k], tmp.data() + (size_t)ZV_FR_CAPACITY * k);
    std::vector<G1Affine> T(zklaim_bit_table_entries(npl));
    for (size_t s = 0; s < T.size(); ++s) T[s] = zv_bit_table_entry(tmp[s]);
    std::vector<G1> sh(VB);
    for (size_t i = 0; i < n; ++i) {
        for (int t = 0; t < VB; ++t) sh[t] = zv_ic_lane_sum(T.data(), pub + i * npl * ZV_REC, npl, (uint32_t)t);
        for (int s = VB / 2; s > 0; s >>= 1)
            for (int t = 0; t < s; ++t) { G1 a = sh[t]; a.add(sh[t + s]); sh[t] = a; }
        out[i] = zv_ic_finish(ic0, sh[0]);
    }
}

MillerConsts miller_consts() {
    static const MillerConsts k = [] {
        using namespace pairing;
        const Fq2 g1 = gamma1(), g2 = g1.sqr(), g3 = g2 * g1, n1 = g1 * conj(g1), n2 = n1.sqr(), n3 = n2 * n1;
        return MillerConsts{fq2(9, 0) * fq2_inverse_host(xi()), g2, g3, n2, n3};
    }();
    return k;
}

FrobConsts frob_consts() {
    static const FrobConsts k = [] {
        using namespace pairing;
        const Fq2 g1 = gamma1(), g2 = g1 * conj(g1), g3 = g2 * g1;
        FrobConsts c;
        const Fq2 *g[3] = {&g1, &g2, &g3};
        for (int j = 0; j < 3; ++j) { c.g[j][0] = *g[j]; for (int i = 1; i < 5; ++i) c.g[j][i] = c.g[j][i - 1] * *g[j]; }
        return c;
    }();
    return k;
}
size_t verify_final_exp_ws_bytes(size_t n) { return (size_t)dev::FE_SLOTS * dev::FE_WORDS * 4 * ((n + VB - 1) / VB * VB); }
// d_out[i] = -(ic0 + sum_k x_ik ic_k), i < n (d_x: n x nidx Montgomery Fr)
int verify_ic_each(const G1Affine *d_ic0, const G1Affine *d_ic, uint32_t nidx, const void *d_x, size_t n, G1Affine *d_out, hipStream_t s) {
    if (!n) return ZKG_OK;
    hipLaunchKernelGGL(k_ic_each, dim3((unsigned)n), dim3(VB), 0, s, n, nidx, d_ic0, d_ic, (const Fr *)d_x, d_out);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
int verify_g2_replicate(const G2Affine *d_key2, size_t n, G2Affine *d_Q, hipStream_t s) {
    if (!n) return ZKG_OK;
    hipLaunchKernelGGL(k_g2_replicate, dim3(blocks_for(2 * n)), dim3(VB), 0, s, n, d_key2, d_Q);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
// d_M: pairs x n Miller values (pair j of item i at j n + i); d_ws: verify_final_exp_ws_bytes(n); d_ab (verdicts) or d_gt (values) may be null
int verify_final_exp_check(const void *d_M, size_t n, uint32_t pairs, void *d_ws, const void *d_ab, uint8_t *d_verdict, void *d_gt, hipStream_t s) {
    if (!n) return ZKG_OK;
    hipLaunchKernelGGL(k_final_exp_check, dim3(blocks_for(n)), dim3(VB), 0, s, n, (const dev::Fq12 *)d_M, pairs, (uint32_t *)d_ws,
                       (size_t)blocks_for(n) * VB, frob_consts(), (const dev::Fq12 *)d_ab, d_verdict, (dev::Fq12 *)d_gt);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
// the device tower compiled for the host: final_exp.hip.hpp's text on one lane (zkg_final_exp, where = 2)
void final_exp_device_code_on_host(const uint8_t in[384], uint8_t out[384]) {
    static_assert(sizeof(dev::Fq12) == 384, "an Fq12 is 12 Fq");
    dev::Fq12 f;
    memcpy(&f, in, 384);
    std::vector<uint32_t> ws((size_t)dev::FE_SLOTS * dev::FE_WORDS);
    const dev::Fq12 g = dev::final_exponentiation(f, 0, [&](int) { return f; }, frob_consts(), dev::FeSlots{ws.data(), 0, 1}).normalized();
    memcpy(out, &g, 384);
}

// d_out[i] = op(d_a[i], d_b[i]) on raw 384-byte Fq12 (zkg_fq12_op, where = 1); d_b may be null for an operation without a second operand
int verify_fq12_op(int op, const void *d_a, const void *d_b, size_t n, void *d_out, hipStream_t s) {
    if (!n) return ZKG_OK;
    const dim3 g(blocks_for(n)), b(VB);
    const dev::Fq12 *A = (const dev::Fq12 *)d_a, *B = (const dev::Fq12 *)d_b; dev::Fq12 *O = (dev::Fq12 *)d_out;
    const FrobConsts fc = frob_consts();
    switch (op) {
#define ZK_FQ12_CASE(OP) case OP: hipLaunchKernelGGL(k_fq12_op<OP>, g, b, 0, s, n, A, B, fc, O); break;
    ZK_FQ12_CASE(FQ12_MUL) ZK_FQ12_CASE(FQ12_SQR) ZK_FQ12_CASE(FQ12_LINE) ZK_FQ12_CASE(FQ12_CSQR) ZK_FQ12_CASE(FQ12_INV) ZK_FQ12_CASE(FQ12_CONJ)
    ZK_FQ12_CASE(FQ12_FROB1) ZK_FQ12_CASE(FQ12_FROB2) ZK_FQ12_CASE(FQ12_FROB3) ZK_FQ12_CASE(FQ12_MUL_BY_V)
#undef ZK_FQ12_CASE
    default: return ZKG_ERROR;
    }
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
// the same text on the host, one element (zkg_fq12_op, where = 2): canonical values in, canonical values out
void fq12_op_device_code_on_host(int op, const uint32_t a[96], const uint32_t b[96], uint32_t out[96]) {
    dev::Fq12 x, y, r;
    memcpy(&x, a, 384); memcpy(&y, b ? b : a, 384);
    const FrobConsts fc = frob_consts();
    switch (op) {
#define ZK_FQ12_CASE(OP) case OP: r = fq12_op_apply<OP>(x, y, fc); break;
    ZK_FQ12_CASE(FQ12_MUL) ZK_FQ12_CASE(FQ12_SQR) ZK_FQ12_CASE(FQ12_LINE) ZK_FQ12_CASE(FQ12_CSQR) ZK_FQ12_CASE(FQ12_INV) ZK_FQ12_CASE(FQ12_CONJ)
    ZK_FQ12_CASE(FQ12_FROB1) ZK_FQ12_CASE(FQ12_FROB2) ZK_FQ12_CASE(FQ12_FROB3)
#undef ZK_FQ12_CASE
    default: r = fq12_op_apply<FQ12_MUL_BY_V>(x, y, fc); break;
    }
    memcpy(out, &r, 384);
}

int verify_g2_subgroup(const G2Affine *d_B, size_t n, uint8_t *d_ok, hipStream_t s) {
    if (!n) return ZKG_OK;
    hipLaunchKernelGGL(k_g2_subgroup, dim3(blocks_for(n)), dim3(VB), 0, s, n, d_B, d_ok);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
int verify_g1_mul128(const G1Affine *d_in, const uint32_t *d_w, size_t nw, size_t n, G1Affine *d_out, hipStream_t s) {
    if (!n || !nw) return ZKG_OK;
    hipLaunchKernelGGL(k_g1_mul128, dim3(blocks_for(n)), dim3(VB), 0, s, n, d_in, d_w, nw, d_out);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
int verify_miller(const G1Affine *d_P, const G2Affine *d_Q, const uint8_t *d_use, size_t n, void *d_out, hipStream_t s) {
    if (!n) return ZKG_OK;
    hipLaunchKernelGGL(k_miller, dim3(blocks_for(n)), dim3(VB), 0, s, n, d_P, d_Q, d_use, miller_consts(), (dev::Fq12 *)d_out);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
// d_partial: VERIFY_PROD_BLOCKS Fq12; the product lands in d_out[0] (lo == hi: one)
int verify_fq12_product(const void *d_in, size_t lo, size_t hi, void *d_partial, void *d_out, hipStream_t s) {
    const size_t n = hi - lo;
    const unsigned g = (unsigned)std::min<size_t>(VERIFY_PROD_BLOCKS, std::max<size_t>(1, n / VB));
    if (g == 1) {
        hipLaunchKernelGGL(k_fq12_prod, dim3(1), dim3(VB), 0, s, (const dev::Fq12 *)d_in, lo, hi, (dev::Fq12 *)d_out);
    } else {
        hipLaunchKernelGGL(k_fq12_prod, dim3(g), dim3(VB), 0, s, (const dev::Fq12 *)d_in, lo, hi, (dev::Fq12 *)d_partial);
        ZK_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_fq12_prod, dim3(1), dim3(VB), 0, s, (const dev::Fq12 *)d_partial, (size_t)0, (size_t)g, (dev::Fq12 *)d_out);
    }
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}

int verify_proof_decode_b(const uint8_t *d_rec, size_t n, G2Affine *d_B, uint8_t *d_dec, hipStream_t s) {
    if (!n) return ZKG_OK;
    hipLaunchKernelGGL(k_proof_decode, dim3(blocks_for(n)), dim3(VB), 0, s, d_rec, n, 1, (G1Affine *)nullptr, d_B, d_dec);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
int verify_proof_decode_ac(const uint8_t *d_rec, size_t n, G1Affine *d_AC, uint8_t *d_dec, hipStream_t s) {
    if (!n) return ZKG_OK;
    hipLaunchKernelGGL(k_proof_decode, dim3(blocks_for(2 * n)), dim3(VB), 0, s, d_rec, n, 0, d_AC, (G2Affine *)nullptr, d_dec);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
int verify_use_mask(size_t n, const uint8_t *d_in_g2, const uint8_t *d_dec_b, const uint8_t *d_dec_ac, uint8_t *d_use, hipStream_t s) {
    if (!n) return ZKG_OK;
    hipLaunchKernelGGL(k_use_mask, dim3(blocks_for(n)), dim3(VB), 0, s, n, d_in_g2, d_dec_b, d_dec_ac, d_use);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
unsigned zklaim_input_sums_slices(size_t n) { return (unsigned)std::min<size_t>(ZV_SUM_SLICES, std::max<size_t>(1, (n + 2 * VB - 1) / (2 * VB))); }
// d_part: ZV_SUM_SLICES x l Fr; the l sums land in d_out (lo == hi: zeros)
int verify_zklaim_input_sums(const uint8_t *d_pub, uint32_t npl, size_t base, const uint32_t *d_w, const uint8_t *d_mask, size_t lo, size_t hi,
                             void *d_part, void *d_out, hipStream_t s) {
    const uint32_t l = zv_input_count(npl);
    const unsigned g = zklaim_input_sums_slices(hi - lo);
    hipLaunchKernelGGL(k_zklaim_input_sums, dim3(l, g), dim3(VB), 0, s, d_pub, npl, base, d_w, d_mask, lo, hi, l, (Fr *)(g == 1 ? d_out : d_part));
    ZK_HIP(hipGetLastError());
    if (g > 1) {
        hipLaunchKernelGGL(k_fr_fold, dim3(blocks_for(l)), dim3(VB), 0, s, (const Fr *)d_part, l, g, (Fr *)d_out);
        ZK_HIP(hipGetLastError());
    }
    return ZKG_OK;
}

// grow-only workspaces of the batch entry points: one per call in flight, kept for the next call (no allocation, no hipFree and no stream
// creation on the way of a verification once a caller's sizes have been seen)
static std::mutex g_ws_mu;
static std::vector<VerifyWorkspace *> g_ws_free;
VerifyWorkspace *verify_workspace_acquire() {
    {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        if (!g_ws_free.empty()) { VerifyWorkspace *w = g_ws_free.back(); g_ws_free.pop_back(); return w; }
    }
    auto *w = new VerifyWorkspace();
    if (hip_ok(hipStreamCreateWithFlags(&w->s, hipStreamNonBlocking), "stream", __FILE__, __LINE__) &&
        hip_ok(hipStreamCreateWithFlags(&w->s2, hipStreamNonBlocking), "stream", __FILE__, __LINE__) &&
        hip_ok(hipEventCreateWithFlags(&w->ev, hipEventDisableTiming), "event", __FILE__, __LINE__) &&
        hip_ok(hipEventCreateWithFlags(&w->ev2, hipEventDisableTiming), "event", __FILE__, __LINE__)) return w;
    verify_workspace_destroy(w);
    return nullptr;
}
void verify_workspace_destroy(VerifyWorkspace *w) {
    if (w->s) (void)hipStreamSynchronize(w->s);
    if (w->s2) (void)hipStreamSynchronize(w->s2);
    w->buf.release();
    if (w->ev) (void)hipEventDestroy(w->ev);
    if (w->ev2) (void)hipEventDestroy(w->ev2);
    if (w->s) (void)hipStreamDestroy(w->s);
    if (w->s2) (void)hipStreamDestroy(w->s2);
    delete w;
}
void verify_workspace_release(VerifyWorkspace *w) {
    if (!w) return;
    if (initialised_device() < 0) { verify_workspace_destroy(w); return; }      // the library was shut down meanwhile
    std::lock_guard<std::mutex> lk(g_ws_mu);
    g_ws_free.push_back(w);
}
void verify_release_all() {
    std::vector<VerifyWorkspace *> ws;
    { std::lock_guard<std::mutex> lk(g_ws_mu); ws.swap(g_ws_free); }
    for (VerifyWorkspace *w : ws) verify_workspace_destroy(w);
}

}  // namespace zk
