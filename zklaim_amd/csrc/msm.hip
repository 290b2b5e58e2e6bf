// msm.hip — Pippenger multi-scalar multiplication over alt_bn128 G1 / G2 for gfx950.
//
// Replaces libff::multi_exp<G, Fr, multi_exp_method_BDLO12>, multi_exp_with_mixed_addition and
// kc_multi_exp_with_mixed_addition (the A/B/H/L query multi-exponentiations inside
// r1cs_gg_ppzksnark_prover, /root/reference/zklaim/snark.cpp:126).
//
// libff walks the c-bit windows serially and mixed-adds every base into buckets[digit].  EC addition is
// not atomic, so on the GPU the scatter is removed structurally — a counting sort by (window, bucket)
// followed by conflict-free accumulation:
//   1. k_digits        signed c-bit digits of every scalar, written window-major (4 B per digit)
//   2-4. the sort, in one of two forms (sort_digits picks):
//        two-pass (uniform scalars, 4096 <= n < 2^23, c >= 12): k_rx_count counts the coarse bins of buckets per
//                      window; k_rx_scatter splits each 16K-point slice into those bins inside LDS and writes every bin's run
//                      contiguously; k_rx_fine sorts one bin by the remaining bucket bits inside LDS and writes the final list and
//                      the bucket counts / offsets in order.  No single-word scatter to global memory anywhere.
//        one-pass (small or huge n, small c, ZKG_SCALARS_MOSTLY_BITS): k_hist — one workgroup per (window, 64K-point slice),
//                      histogram in LDS (2^(c-1) counters, up to 128 KiB of the CU's 160 KiB); k_colscan + block scan -> bucket
//                      offsets; k_place — bucket cursors staged in LDS, point indices (sign in bit 0) stored at their final
//                      position.  No global atomics, so skewed digits (bit witnesses) cost nothing extra.
//   5. k_order         bucket ids ordered by descending length, so the 64 lanes of a wavefront walk
//                      lists of (nearly) equal length
//   6. k_bucket_accum  one lane per bucket: sequential XYZZ mixed adds over its index list, next base
//                      prefetched (the dominant kernel: N*W mixed additions, 64/128 B gathers).
//                      Buckets longer than heavy_t leave this kernel: they are cut into 512-entry parts
//                      summed by one wavefront each (k_heavy_parts) and merged per bucket by an LDS tree
//                      (k_heavy_merge), so no lane ever walks a long list alone
//   7. k_bucket_reduce sum_b (b+1)*B_b per chunk of 128 ... 2048 buckets: per-lane running sums, then an LDS suffix
//                      scan + tree reduction across the workgroup; every addition is shared by a DPP quad
//   8. host            per-window chunk combine and the c-doublings Horner across windows
//   8'. k_msm_combine  the same combine on the device for a table launch (no Horner there): the points stay in device memory and the job
//                      ends without a host synchronisation (msm_job_finish_dev; zkg_msm_g1_resident_async at <Fq, 256>,
//                      zkg_msm_g2_resident_async at <Fq2, 128>)
// Zero scalars are dropped in step 1 and scalars equal to one simply land in bucket (window 0, digit 1),
// a "heavy" bucket: the effect of libff's multi_exp_with_mixed_addition prefilter without a special case.
//
// The prover's resident key adds two things (prover.hip drives them):
//   * per-window tables (window_table_build_*): level w holds 2^(c w) P_i, so a digit of any window weighs the same — step 6 gathers from
//     the digit's level, k_bucket_fold sums the W bucket sets bucket-wise (LDS tree over the windows), step 7 runs ONCE over 2^(c-1)
//     buckets and step 8 has no doubling left;
//   * the witness split (witness_classify, ones_sum_launch): multi_exp_with_mixed_addition as libff does it — zeros skipped, bases whose
//     scalar is one added flat (k_ones_sum, k_sum_partials), the remaining scalars through steps 1-8 as a gathered subset, several base
//     sets (A, B_g1, L) per launch (blockIdx.y).
// Also here: the generator's fixed-base batch (k_fixed_table, k_fixed_base: byte windows, in-lane batched normalisation).
#include "common.hpp"
#include "fq29.hip.hpp"
#include "host/horner_jac.hpp"
#include "../../include/zkg.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

// Register cap of one kernel.  gfx90a and later have one 512-entry file per lane for VGPRs and AGPRs, and LLVM doubles the attribute's
// value there before it compares it with the budget ("amdgpu-num-vgpr" counts the unified file): half the wanted number of VGPRs goes in.
#define ZK_VGPR_CAP(n) __attribute__((amdgpu_num_vgpr((n) / 2)))
static constexpr int ACC29_VGPRS = 192;
static constexpr int ACC29_WG = 64;          // threads per workgroup of k_bucket_accum29: one wavefront (see the kernel)

namespace zk {

static constexpr int SCALAR_BITS = 255;      // r < 2^254; one extra bit absorbs the signed-digit carry
// logical lanes per reduce workgroup, four physical lanes (one DPP quad) each.  G1: 128 (512 threads, 128-VGPR budget is enough for
// three 32-register points).  G2: 64 -> 256 threads, so that the compiler may use 256 VGPRs: the kernel holds three 64-register
// points and was spilling 1.4 KB per lane under the 128-register cap of a 512-thread workgroup.
template <class F> struct RedGeom { static constexpr int LANES_LOG = sizeof(F) == sizeof(Fq) ? 7 : 6, LANES = 1 << LANES_LOG, THREADS = 4 * LANES; };
// buckets per logical lane in the running-sum step, 2^L_LOG: the kernel is a dependency chain of 2(L-1) + 2 log2(128) + 2
// additions but does (2(L-1) + 14)/L additions per bucket, so small bucket sets (latency-bound: the prover's witness MSMs)
// take L = 4 and large ones (work-bound: 2^19 buckets at N = 2^20) take L = 16.
static constexpr int RED_L_LOG_TINY = 0, RED_L_LOG_SMALL = 2, RED_L_LOG_LARGE = 4;
// up to 2^16 buckets one bucket per logical lane still is a single round of workgroups (512 of them for G1): the chain is 2 log2(LANES) + 3
// additions, 17 instead of 23 for G1 — every table launch of the prover (one folded bucket set of <= 2^15 buckets) is in this class
static constexpr size_t RED_SMALL_BUCKETS = (size_t)1 << 16, RED_LARGE_BUCKETS = (size_t)1 << 18;
static constexpr int MAX_C = 16;             // LDS histogram: 2^(c-1) u32 counters <= 128 KiB
static constexpr uint32_t HEAVY_S = 512;     // entries per heavy part (one wavefront sums one part)
static constexpr uint32_t HEAVY_T_MAX = 1024;
static constexpr uint32_t CLASS_HIST_COPIES = 8;     // of the class histogram (HEAVY_T_MAX + 2 counters each), see rx_fine_offsets
static constexpr int HEAVY_PART_BLOCKS = 512, HEAVY_MERGE_BLOCKS = 128;
static constexpr int SORT_THREADS = 1024;
static constexpr int SCAN_ITEMS = 4;         // per thread in the block scan

// window bits, windows handled by this launch, buckets per window (2^(c-1)); the launch owns windows w0, w0 + ws, ... of the Wt
// windows of the scalar (w0 = 0, ws = 1: all of them; a window-sharded multi-GPU run gives rank g the set w0 = g, ws = G)
struct MsmGeom { uint32_t c, W, B, Wt, w0, ws; };
// How a sorted entry finds its base.  Plain set: bases[i].  Per-window table of a resident key (level w holds 2^(c w) P_i, built once by
// window_table_build): bases[w * level_stride + i], w = the window of the entry's bucket — every window's digit then weighs the same, so
// the W bucket sets are summed bucket-wise (k_bucket_fold) and reduced ONCE, and no doubling is left for the host.  `gather`: the scalars
// were a gathered subset (a witness' non-bit values); entry i stands for element gather[i] of the set.  `index_sub`: the set starts at
// that element (the L query starts behind the public inputs); entries below it belong to no base of this set.
// The base sets of one field in a launch are batched: every kernel below runs once for all of them, blockIdx.y = set, each set with its
// own accumulators, heavy lists and results laid out `set` strides apart (SetLayout), all walking the same sorted digit list.
struct SetLayout { size_t buckets, items, heavy, partials, folded, red_out; };     // elements per set in each per-set array
template <class F> struct BaseView {
    const Affine<F> *p; size_t level_stride; const uint32_t *gather; uint32_t index_sub, B; const uint32_t *remap;
    template <bool PLAIN = false> ZK_D Affine<F> load(uint32_t e, size_t gb) const {
        if constexpr (PLAIN) return p[e >> 1];            // a plain base set: nothing but the gather (the 2^20-point multi_exp's inner loop)
        uint32_t i = e >> 1;
        if (gather) i = gather[i];
        if (remap) i = remap[i];                          // a subset table: position of element i in it
        if (i < index_sub) return Affine<F>::inf();
        return p[(level_stride ? (gb / B) * level_stride : 0) + (i - index_sub)];
    }
};
template <class F> struct ViewSet { BaseView<F> v[MSM_MAX_SETS]; };
struct HeavyItem { uint32_t start, end, gb, single; };   // a part: range of the sorted index list, the bucket it belongs to, and whether it is that bucket's only part
struct HeavyBucket { uint32_t gb, first_item, nparts; };

// Window size.  Measured on MI355X with uniformly random scalars (tools/msm_c_sweep.py): the accumulation runs one lane per
// bucket, so it needs W * 2^(c-1) >> 64 K buckets to fill the chip, and that outweighs the extra bucket-reduction work down to
// 2^15 points: c = 16 there, 12 below, and small windows only for tiny inputs.  `window_hint` (the prover's witness
// multi-exponentiations, whose scalars are mostly 0/1 so that the bucket reduction dominates) overrides the rule.
static MsmGeom pick_geom(size_t n, int window_hint, uint32_t w0 = 0, uint32_t ws = 1) {
    int lg = 0; while (((size_t)1 << (lg + 1)) <= n) ++lg;
    int c = lg >= 15 ? 16 : lg >= 11 ? 12 : lg + 1;
    if (c < 4) c = 4;
    if (window_hint > 0) c = window_hint;
    static const char *force = getenv("ZKG_MSM_C");                          // tuning aid
    if (force && atoi(force) >= 2) c = atoi(force);
    if (c > MAX_C) c = MAX_C;
    MsmGeom g; g.c = c; g.Wt = (SCALAR_BITS + c - 1) / c; g.B = 1u << (c - 1);
    g.w0 = w0; g.ws = ws ? ws : 1; g.W = w0 < g.Wt ? (g.Wt - w0 + g.ws - 1) / g.ws : 0;
    return g;
}

// ---- 1. scalar -> signed digits -----------------------------------------------------------------
ZK_D uint32_t bits_at(const uint32_t v[8], uint32_t off, uint32_t c) {
    uint32_t limb = off >> 5, sh = off & 31;
    if (limb >= 8) return 0;
    uint64_t x = v[limb];
    if (limb + 1 < 8) x |= (uint64_t)v[limb + 1] << 32;
    return (uint32_t)(x >> sh) & ((1u << c) - 1);
}

// The digit sort's kernels raise their wavefronts' issue priority: in a piece-wise job they share SIMDs with the accumulation of the piece
// before (k_bucket_accum29 leaves them the registers, ACC29_VGPRS), whose older, multiply-bound wavefronts would otherwise win every
// arbitration — k_digits_c4 took 113 ... 183 us beside an accumulation, 10 us alone.  The sort is 5 % of the step's instructions and on its critical path.
ZK_D void sort_wave_priority() { __builtin_amdgcn_s_setprio(3); }


// digit code: 0 = no contribution; otherwise ((bucket + 1) << 1) | negative, bucket = |d| - 1
// The job's first kernel also clears the counters its later kernels accumulate into (coarse-bin counts, class histogram, heavy-bucket
// counters): three hipMemsetAsync fill launches per job were three more dependent launches on a proof's critical path.
struct ZeroList { uint32_t *p[4]; uint32_t words[4]; };
__global__ __launch_bounds__(256) void k_digits(const uint32_t *scalars, const uint32_t *gather, size_t n, int mont, MsmGeom g, uint32_t *digits, ZeroList zl) {
    sort_wave_priority();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) for (size_t z = i; z < zl.words[k]; z += lanes) zl.p[k][z] = 0;
    if (i >= n) return;
    Fr f;
    const uint4 *p = reinterpret_cast<const uint4 *>(scalars + 8 * (gather ? (size_t)gather[i] : i));
    uint4 a = p[0], b = p[1];
    f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
    if (mont) f = f.from_mont();
    uint32_t carry = 0;
    for (uint32_t w = 0, own = g.w0, slot = 0; w < g.Wt; ++w) {                 // the carry chain runs over every window; owned ones are stored
        uint32_t raw = bits_at(f.v, w * g.c, g.c) + carry, code = 0;
        if (raw > g.B) { uint32_t d = (1u << g.c) - raw; carry = 1; if (d) code = (d << 1) | 1u; }
        else { carry = 0; if (raw) code = raw << 1; }
        if (w == own) { digits[(size_t)slot * n + i] = code; ++slot; own += g.ws; }
    }
}

// The same with the window size known at compile time (16 and 12: every launch of the shipped geometry): the window loop unrolls, every limb
// index and shift is a constant, and the scalar stays in registers — the generic kernel indexes its limbs by a run-time window offset, which
// the compiler serves from an LDS copy of the scalar with two dependent reads per window (k_digits took 55 us at 2^20 points: 2.5 x what its
// 96 MB of traffic cost).
template <int C>
__global__ __launch_bounds__(256) void k_digits_c(const uint32_t *scalars, const uint32_t *gather, size_t n, int mont, MsmGeom g, uint32_t *digits, ZeroList zl) {
    sort_wave_priority();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) for (size_t z = i; z < zl.words[k]; z += lanes) zl.p[k][z] = 0;
    if (i >= n) return;
    Fr f;
    const uint4 *p = reinterpret_cast<const uint4 *>(scalars + 8 * (gather ? (size_t)gather[i] : i));
    uint4 a = p[0], b = p[1];
    f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
    if (mont) f = f.from_mont();
    constexpr int WT = (SCALAR_BITS + C - 1) / C;
    constexpr uint32_t B = 1u << (C - 1), MASK = (1u << C) - 1;
    uint32_t carry = 0, own = g.w0, slot = 0;
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        const int off = w * C, limb = off >> 5, sh = off & 31;
        uint32_t v = limb < 8 ? f.v[limb < 8 ? limb : 7] >> sh : 0u;
        if (sh + C > 32 && limb + 1 < 8) v |= f.v[limb + 1 < 8 ? limb + 1 : 7] << (32 - sh);
        const uint32_t raw = (v & MASK) + carry;
        const bool neg = raw > B;
        const uint32_t d = neg ? (1u << C) - raw : raw;                          // |digit|; 2^C - raw = 0 only for raw = 2^C (a pure carry)
        carry = neg ? 1u : 0u;
        const uint32_t code = d ? (d << 1) | (neg ? 1u : 0u) : 0u;
        if ((uint32_t)w == own) { digits[(size_t)slot * n + i] = code; ++slot; own += g.ws; }
    }
}

// Several scalar vectors over ONE table (msm_job_launch_multi: the H queries of a batch of proofs), blockIdx.y = vector.  The digit array gets
// a row per (window, vector), window-major: row (w / merge) * P * merge + p * merge + w % merge.  The rows of one window then lie side by side
// as ONE window of P * B buckets — an entry finds its level as bucket / (P * B), the fold over the windows leaves P bucket sets back to back,
// and every kernel behind this one runs unchanged on a geometry of W * P rows (with merged rows: a vector's `merge` consecutive windows stay adjacent).
template <int C>
__global__ __launch_bounds__(256) void k_digits_multi(const uint32_t *scalars, size_t scalar_stride /* words between vectors */, size_t n, int mont, uint32_t merge, uint32_t *digits, ZeroList zl) {
    sort_wave_priority();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
    if (blockIdx.y == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) for (size_t z = i; z < zl.words[k]; z += lanes) zl.p[k][z] = 0;
    }
    if (i >= n) return;
    const uint32_t p = blockIdx.y, P = gridDim.y;
    Fr f;
    const uint4 *src = reinterpret_cast<const uint4 *>(scalars + (size_t)p * scalar_stride + 8 * i);
    uint4 a = src[0], b = src[1];
    f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
    if (mont) f = f.from_mont();
    constexpr int WT = (SCALAR_BITS + C - 1) / C;
    constexpr uint32_t B = 1u << (C - 1), MASK = (1u << C) - 1;
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        const int off = w * C, limb = off >> 5, sh = off & 31;
        uint32_t v = limb < 8 ? f.v[limb < 8 ? limb : 7] >> sh : 0u;
        if (sh + C > 32 && limb + 1 < 8) v |= f.v[limb + 1 < 8 ? limb + 1 : 7] << (32 - sh);
        const uint32_t raw = (v & MASK) + carry;
        const bool neg = raw > B;
        const uint32_t d = neg ? (1u << C) - raw : raw;
        carry = neg ? 1u : 0u;
        const uint32_t code = d ? (d << 1) | (neg ? 1u : 0u) : 0u;
        const size_t row = ((size_t)((uint32_t)w / merge) * P + p) * merge + (uint32_t)w % merge;
        digits[row * n + i] = code;
    }
}

// the same for any window size (the witness tables': 10 ... 14 bits), as k_digits
__global__ __launch_bounds__(256) void k_digits_multi_any(const uint32_t *scalars, size_t scalar_stride, size_t n, int mont, MsmGeom g, uint32_t merge, uint32_t *digits, ZeroList zl) {
    sort_wave_priority();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
    if (blockIdx.y == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) for (size_t z = i; z < zl.words[k]; z += lanes) zl.p[k][z] = 0;
    }
    if (i >= n) return;
    const uint32_t p = blockIdx.y, P = gridDim.y;
    Fr f;
    const uint4 *src = reinterpret_cast<const uint4 *>(scalars + (size_t)p * scalar_stride + 8 * i);
    uint4 a = src[0], b = src[1];
    f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
    if (mont) f = f.from_mont();
    uint32_t carry = 0;
    for (uint32_t w = 0; w < g.Wt; ++w) {
        uint32_t raw = bits_at(f.v, w * g.c, g.c) + carry, code = 0;
        if (raw > g.B) { uint32_t d = (1u << g.c) - raw; carry = 1; if (d) code = (d << 1) | 1u; }
        else { carry = 0; if (raw) code = raw << 1; }
        const size_t row = ((size_t)(w / merge) * P + p) * merge + w % merge;
        digits[row * n + i] = code;
    }
}

// ... and four consecutive scalars per thread (no gather list, n a multiple of 4, every window owned): a window's four digits leave as ONE 16-byte
// store per lane — 1 KiB per wavefront instead of four 256-byte stores (the kernel is bound by its store instructions: 16.7 M four-byte stores at 2^20)
template <int C>
__global__ __launch_bounds__(256) void k_digits_c4(const uint32_t *scalars, size_t n, int mont, MsmGeom g, uint32_t *digits, ZeroList zl) {
    sort_wave_priority();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) for (size_t z = i; z < zl.words[k]; z += lanes) zl.p[k][z] = 0;
    if (4 * i >= n) return;
    Fr f[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 *p = reinterpret_cast<const uint4 *>(scalars + 8 * (4 * i + q));
        const uint4 a = p[0], b = p[1];
        f[q].v[0] = a.x; f[q].v[1] = a.y; f[q].v[2] = a.z; f[q].v[3] = a.w; f[q].v[4] = b.x; f[q].v[5] = b.y; f[q].v[6] = b.z; f[q].v[7] = b.w;
        if (mont) f[q] = f[q].from_mont();
    }
    constexpr int WT = (SCALAR_BITS + C - 1) / C;
    constexpr uint32_t B = 1u << (C - 1), MASK = (1u << C) - 1;
    uint32_t carry[4] = {0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < WT; ++w) {
        const int off = w * C, limb = off >> 5, sh = off & 31;
        uint32_t code[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t v = limb < 8 ? f[q].v[limb < 8 ? limb : 7] >> sh : 0u;
            if (sh + C > 32 && limb + 1 < 8) v |= f[q].v[limb + 1 < 8 ? limb + 1 : 7] << (32 - sh);
            const uint32_t raw = (v & MASK) + carry[q];
            const bool neg = raw > B;
            const uint32_t d = neg ? (1u << C) - raw : raw;
            carry[q] = neg ? 1u : 0u;
            code[q] = d ? (d << 1) | (neg ? 1u : 0u) : 0u;
        }
        *reinterpret_cast<uint4 *>(digits + (size_t)w * n + 4 * i) = make_uint4(code[0], code[1], code[2], code[3]);
    }
}

// ---- 2. per-(window, slice) histogram in LDS ---------------------------------------------------------
__global__ __launch_bounds__(SORT_THREADS) void k_hist(const uint32_t *digits, size_t n, uint32_t B, uint32_t S, uint32_t slice_len, uint32_t *hist) {
    extern __shared__ uint32_t lds_u32[];
    const uint32_t s = blockIdx.x, w = blockIdx.y, t = threadIdx.x;
    for (uint32_t b = t; b < B; b += SORT_THREADS) lds_u32[b] = 0;
    __syncthreads();
    size_t lo = (size_t)s * slice_len, hi = lo + slice_len < n ? lo + slice_len : n;
    const uint32_t *d = digits + (size_t)w * n;
    for (size_t i = lo + t; i < hi; i += SORT_THREADS) { uint32_t code = d[i]; if (code) atomicAdd(&lds_u32[(code >> 1) - 1], 1u); }
    __syncthreads();
    uint32_t *out = hist + ((size_t)w * S + s) * B;
    for (uint32_t b = t; b < B; b += SORT_THREADS) out[b] = lds_u32[b];
}

// ---- 3. per-bucket totals; hist becomes the slice-relative offset inside its bucket -----------------------
__global__ __launch_bounds__(256) void k_colscan(uint32_t *hist, uint32_t B, uint32_t S, size_t total, uint32_t *counts) {
    size_t gb = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gb >= total) return;
    uint32_t w = (uint32_t)(gb / B), b = (uint32_t)(gb % B), run = 0;
    uint32_t *col = hist + (size_t)w * S * B + b;
    for (uint32_t s = 0; s < S; ++s) { uint32_t v = col[(size_t)s * B]; col[(size_t)s * B] = run; run += v; }
    counts[gb] = run;
}

// block-wise exclusive scan (three launches): offsets[i] = sum counts[<i], offsets[total] = sum
__global__ __launch_bounds__(1024) void k_scan_blocks(const uint32_t *in, uint32_t *out, uint32_t *sums, size_t total) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x;
    size_t base = ((size_t)blockIdx.x * 1024 + t) * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS], s = 0;
    for (int j = 0; j < SCAN_ITEMS; ++j) { v[j] = base + j < total ? in[base + j] : 0; s += v[j]; }
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        uint32_t x = (t >= d) ? part[t - d] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (int j = 0; j < SCAN_ITEMS; ++j) { if (base + j < total) out[base + j] = run; run += v[j]; }
    if (t == 1023) sums[blockIdx.x] = part[1023];
}
__global__ __launch_bounds__(1024) void k_scan_sums(uint32_t *sums, uint32_t nblk, uint32_t *grand_total) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x;
    uint32_t s = t < nblk ? sums[t] : 0;
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        uint32_t x = (t >= d) ? part[t - d] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    if (t < nblk) sums[t] = part[t] - s;
    if (t == 1023) *grand_total = part[1023];
}
__global__ __launch_bounds__(1024) void k_scan_apply(uint32_t *out, const uint32_t *sums, size_t total) {
    size_t base = ((size_t)blockIdx.x * 1024 + threadIdx.x) * SCAN_ITEMS;
    uint32_t add = sums[blockIdx.x];
    for (int j = 0; j < SCAN_ITEMS; ++j) if (base + j < total) out[base + j] += add;
}

// ---- 4. placement: cursors of this (window, slice) staged in LDS -----------------------------------------
__global__ __launch_bounds__(SORT_THREADS) void k_place(const uint32_t *digits, size_t n, uint32_t B, uint32_t S, uint32_t slice_len,
                                                         const uint32_t *hist, const uint32_t *offsets, uint32_t *sorted) {
    extern __shared__ uint32_t lds_u32[];
    const uint32_t s = blockIdx.x, w = blockIdx.y, t = threadIdx.x;
    const uint32_t *rel = hist + ((size_t)w * S + s) * B, *off = offsets + (size_t)w * B;
    for (uint32_t b = t; b < B; b += SORT_THREADS) lds_u32[b] = off[b] + rel[b];
    __syncthreads();
    size_t lo = (size_t)s * slice_len, hi = lo + slice_len < n ? lo + slice_len : n;
    const uint32_t *d = digits + (size_t)w * n;
    for (size_t i = lo + t; i < hi; i += SORT_THREADS) {
        uint32_t code = d[i];
        if (code) { uint32_t pos = atomicAdd(&lds_u32[(code >> 1) - 1], 1u); sorted[pos] = ((uint32_t)i << 1) | (code & 1u); }
    }
}


// ---- 4b. two-pass sort (c >= 12, n < 2^22).  k_place's 4-byte stores each leave the L2 as their own 32-byte write (measured: 538 MB of
//      WRITE_SIZE for a 64 MiB list), so here no pass scatters single words to global memory: pass 1 splits a 16K-point slice into the
//      64 coarse bins of its window inside LDS and writes each bin's run contiguously; pass 2 takes one (window, coarse bin), sorts its
//      ~n/64 entries by the remaining bucket bits inside LDS and writes the final list — and the bucket counts and offsets — in order.
static constexpr uint32_t RX_MAX_CBITS = 10, RX_MAX_CB = 1u << RX_MAX_CBITS, RX_SLICE = 16384, RX_PER_THREAD = 16, RX_FINE_MAX = 8192, RX_BIN_AVG = 4096;
// temporary entry between the passes: fine bucket (fbits) in the top bits | point index << 1 | sign below.  cbits: log2 of the coarse bins
// per window, chosen on the host so that a bin averages <= 4096 entries, half of what the second pass holds in LDS (measured: 1365 ...
// 8192 all within 2 %).  The top window of a 254-bit scalar populates only 38 % of its buckets, so its bins are 2.65x as full and go to
// the streamed path of k_rx_fine (rx_fine_big_bin).
// Heavy threshold, computed on the device from the real list lengths: a lane walks its bucket's list alone (~7 us per G1
// addition at low occupancy), so the longest non-heavy list bounds the kernel's latency however little total work there is.
// Lists are cut at 4x the true average length + 32 (the partly filled top window of uniform scalars averages ~2.7x the other
// windows and stays on the lane-per-bucket path; a sparse bit-witness MSM gets a small threshold and a short tail).
ZK_D uint32_t heavy_threshold_dev(const uint32_t *offsets, size_t total_buckets, uint32_t divisor) {
    uint32_t entries = offsets[total_buckets];
    // the slack shrinks with the average: a sparse launch (a witness' few non-bit scalars over 2^19 buckets) is pure latency, and its
    // longest lane-walked list is its duration
    uint32_t avg6 = (uint32_t)(6 * (uint64_t)entries / total_buckets), slack = 8 + avg6 > 32 ? 32 : 8 + avg6;
    uint32_t t = (uint32_t)(4 * (uint64_t)entries / total_buckets) + slack;
    t = t > HEAVY_T_MAX ? HEAVY_T_MAX : t;
    t /= divisor;
    return t < 4 ? 4 : t;
}
// sum over the 64 lanes of a wavefront (every lane gets it)
ZK_D uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// The bin start positions are not laid out by a launch of their own: k_rx_count also adds every slice's entries to its window's total, wtot[w],
// and the workgroups of the two passes work out what they need from the counts — start of window w = sum of wtot below w, start of a bin = that
// plus the window's bin counts below it (rx_entries_before).  Each is a few hundred cached words per workgroup against one more dependent
// launch (a single workgroup, 10 us with its gap) at the head of every sort.
__global__ __launch_bounds__(1024) void k_rx_count(const uint32_t *digits, size_t n, uint32_t fbits, uint32_t cbits, uint32_t *cnt, uint32_t *wtot) {
    sort_wave_priority();
    __shared__ uint32_t c[RX_MAX_CB];
    __shared__ uint32_t tot;
    const uint32_t sl = blockIdx.x, w = blockIdx.y, t = threadIdx.x, CB = 1u << cbits;
    if (t < CB) c[t] = 0;
    if (t == 0) tot = 0;
    __syncthreads();
    size_t lo = (size_t)sl * RX_SLICE, hi = lo + RX_SLICE < n ? lo + RX_SLICE : n;
    const uint32_t *d = digits + (size_t)w * n;
    if ((n & 3) == 0) {                                                   // rows 16-byte aligned: four digits per load
        for (size_t i = lo + 4 * t; i < hi; i += 4096) {
            const uint4 q = *reinterpret_cast<const uint4 *>(d + i);     // (hi - lo is a multiple of 4 with n)
            if (q.x) atomicAdd(&c[((q.x >> 1) - 1) >> fbits], 1u);
            if (q.y) atomicAdd(&c[((q.y >> 1) - 1) >> fbits], 1u);
            if (q.z) atomicAdd(&c[((q.z >> 1) - 1) >> fbits], 1u);
            if (q.w) atomicAdd(&c[((q.w >> 1) - 1) >> fbits], 1u);
        }
    } else
    for (size_t i = lo + t; i < hi; i += 1024) { uint32_t code = d[i]; if (code) atomicAdd(&c[((code >> 1) - 1) >> fbits], 1u); }
    __syncthreads();
    if (t < CB) {                                                         // (CB >= 64: whole wavefronts)
        const uint32_t mine = c[t];
        if (mine) atomicAdd(&cnt[w * CB + t], mine);
        const uint32_t in_wave = wave_sum(mine);
        if ((t & 63) == 0 && in_wave) atomicAdd(&tot, in_wave);
    }
    __syncthreads();
    if (t == 0 && tot) atomicAdd(&wtot[w], tot);
}
// This thread's share of the entries that lie before bin (w, cb) in the list: the windows below w, and w's bins below cb.  Summed over the
// workgroup's threads (wave_sum, then one LDS atomic per wavefront) it is the bin's start; cb = 0: the window's.
ZK_D uint32_t rx_entries_before(const uint32_t *cnt, const uint32_t *wtot, uint32_t w, uint32_t cb, uint32_t cbits) {
    uint32_t v = 0;
    for (uint32_t i = threadIdx.x; i < w; i += blockDim.x) v += wtot[i];
    for (uint32_t b = threadIdx.x; b < cb; b += blockDim.x) v += cnt[(w << cbits) + b];
    return v;
}
// T threads per workgroup take a slice of 16 T digits.  T = 1024 (16K-digit slices, 64 KiB of LDS) when the sort has the chip to itself; T = 512 for
// the sorts of a piece-wise job, which run BESIDE the accumulation of the piece before: two wavefronts per SIMD of 56 registers fit into what
// k_bucket_accum29 leaves free (ACC29_VGPRS), four do not.
// The start of every bin of the window comes from an exclusive scan of the window's 2^cbits counts (it shares the barriers of the slice's own
// scan) on top of the window's start; `cursor` counts, per bin, the entries that the slices before this one (in atomic order) have reserved.
// Workgroup (0, 0) also stores the number of entries of the whole list, offsets[total buckets], for the kernels of the later launches.
template <int T>
__global__ __launch_bounds__(T) void k_rx_scatter(const uint32_t *digits, size_t n, uint32_t fbits, uint32_t cbits, const uint32_t *cnt, const uint32_t *wtot, uint32_t W,
                                                   uint32_t *cursor, uint32_t *tmp, uint32_t *grand_total) {
    sort_wave_priority();
    extern __shared__ uint32_t lds_u32[];
    constexpr uint32_t SLICE = RX_PER_THREAD * T;
    const uint32_t CB = 1u << cbits;
    uint32_t *stage = lds_u32, *c = lds_u32 + SLICE, *off = c + RX_MAX_CB, *gb = off + RX_MAX_CB + 1, *cur = gb + RX_MAX_CB, *wsum = cur + RX_MAX_CB;   // wsum[0]: start of the window, [1]: all entries
    const uint32_t sl = blockIdx.x, w = blockIdx.y, t = threadIdx.x;
    for (uint32_t b = t; b < CB; b += T) c[b] = 0;
    if (t < 2) wsum[t] = 0;
    __syncthreads();
    // a thread owns bins t and t + T (CB <= 1024 <= 2 T) in both scans
    const uint32_t b0 = t, b1 = t + T;
    const uint32_t g0 = b0 < CB ? cnt[w * CB + b0] : 0, g1 = b1 < CB ? cnt[w * CB + b1] : 0;
    {
        const uint32_t below = wave_sum(rx_entries_before(cnt, wtot, w, 0, cbits));
        if ((t & 63) == 0 && below) atomicAdd(&wsum[0], below);
        if (sl == 0 && w == 0) {                                          // (uniform across the workgroup)
            uint32_t all = 0;
            for (uint32_t i = t; i < W; i += T) all += wtot[i];
            all = wave_sum(all);
            if ((t & 63) == 0 && all) atomicAdd(&wsum[1], all);
        }
    }
    size_t lo = (size_t)sl * SLICE, hi = lo + SLICE < n ? lo + SLICE : n;
    const uint32_t *d = digits + (size_t)w * n;
    uint32_t code[RX_PER_THREAD];                                    // this thread's 16 digits stay in registers between the two passes
    // which element of the slice is this thread's j-th: four consecutive ones per 16-byte load when the rows are aligned (n a multiple of 4)
    const bool vec = (n & 3) == 0;
    auto elem = [&](uint32_t j) -> size_t { return vec ? lo + 4 * (size_t)t + (size_t)(j >> 2) * (4 * T) + (j & 3) : lo + t + (size_t)j * T; };
    if (vec) {
#pragma unroll
        for (uint32_t j = 0; j < RX_PER_THREAD; j += 4) {
            const size_t i = elem(j);
            uint4 q = make_uint4(0, 0, 0, 0);
            if (i < hi) q = *reinterpret_cast<const uint4 *>(d + i);
            code[j] = q.x; code[j + 1] = q.y; code[j + 2] = q.z; code[j + 3] = q.w;
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < RX_PER_THREAD; ++j) { const size_t i = elem(j); code[j] = i < hi ? d[i] : 0; }
    }
#pragma unroll
    for (uint32_t j = 0; j < RX_PER_THREAD; ++j) if (code[j]) atomicAdd(&c[((code[j] >> 1) - 1) >> fbits], 1u);
    __syncthreads();
    // exclusive scans of the slice's bin counts (off; off[CB] = entries of the slice) and of the window's (gb), Hillis-Steele side by side
    if (b0 < CB) { off[b0] = c[b0]; gb[b0] = g0; }
    if (b1 < CB) { off[b1] = c[b1]; gb[b1] = g1; }
    __syncthreads();
    for (uint32_t dd = 1; dd < CB; dd <<= 1) {
        const bool in0 = b0 < CB && b0 >= dd, in1 = b1 < CB && b1 >= dd;
        const uint32_t x0 = in0 ? off[b0 - dd] : 0, x1 = in1 ? off[b1 - dd] : 0, y0 = in0 ? gb[b0 - dd] : 0, y1 = in1 ? gb[b1 - dd] : 0;
        __syncthreads();
        if (b0 < CB) { off[b0] += x0; gb[b0] += y0; }
        if (b1 < CB) { off[b1] += x1; gb[b1] += y1; }
        __syncthreads();
    }
    if (t == 0) off[CB] = off[CB - 1];
    if (t == 0 && sl == 0 && w == 0) *grand_total = wsum[1];
    __syncthreads();
    const uint32_t wstart = wsum[0];
    if (b0 < CB) { off[b0] -= c[b0]; gb[b0] = c[b0] ? wstart + (gb[b0] - g0) + atomicAdd(&cursor[w * CB + b0], c[b0]) : 0; cur[b0] = 0; }
    if (b1 < CB) { off[b1] -= c[b1]; gb[b1] = c[b1] ? wstart + (gb[b1] - g1) + atomicAdd(&cursor[w * CB + b1], c[b1]) : 0; cur[b1] = 0; }
    __syncthreads();
    const uint32_t fmask = (1u << fbits) - 1;
#pragma unroll
    for (uint32_t j = 0; j < RX_PER_THREAD; ++j) {
        if (!code[j]) continue;
        uint32_t i = (uint32_t)elem(j), b = (code[j] >> 1) - 1, k = b >> fbits;
        uint32_t pos = off[k] + atomicAdd(&cur[k], 1u);
        stage[pos] = ((b & fmask) << (32 - fbits)) | (i << 1) | (code[j] & 1u);
    }
    __syncthreads();
    // runs go out contiguously, one wavefront per bin at a time (consecutive lanes -> consecutive addresses)
    const uint32_t wave = t >> 6, lane = t & 63;
    for (uint32_t k = wave; k < CB; k += T / 64) {
        const uint32_t a = off[k], b = off[k + 1], g = gb[k];
        for (uint32_t p = a + lane; p < b; p += 64) tmp[g + (p - a)] = stage[p];
    }
}
// shared by the two second-pass paths: exclusive scan of the FB <= 512 counters (Hillis-Steele in LDS), counts / offsets to global — and the
// bin's share of the class histogram (buckets per list length, k_class_hist's classes; h: heavy_t + 2 zeroed LDS counters), which the bucket
// order needs: the counts are in LDS here, so the two-pass sort has no k_class_hist launch
ZK_D void rx_fine_offsets(uint32_t *cf, uint32_t *of, uint32_t FB, uint32_t t, uint32_t start, size_t gb0, uint32_t *counts, uint32_t *offsets, uint32_t *h, uint32_t heavy_t,
                          uint32_t *class_hist) {
    const uint32_t T = blockDim.x;                                    // FB <= 512 <= T
    if (t < FB) { const uint32_t c = cf[t]; of[t] = c; atomicAdd(&h[c > heavy_t ? heavy_t + 1 : c], 1u); }
    __syncthreads();
    for (uint32_t d = 1; d < FB; d <<= 1) {
        uint32_t x = (t < FB && t >= d) ? of[t - d] : 0;
        __syncthreads();
        if (t < FB) of[t] += x;
        __syncthreads();
    }
    if (t < FB) of[t] -= cf[t];
    __syncthreads();
    for (uint32_t f = t; f < FB; f += T) { counts[gb0 + f] = cf[f]; offsets[gb0 + f] = start + of[f]; }
    // (every workgroup adds to the same few classes: the copies spread them over CLASS_HIST_COPIES times as many addresses, k_order_place sums them)
    uint32_t *copy = class_hist + ((blockIdx.x + blockIdx.y) % CLASS_HIST_COPIES) * (HEAVY_T_MAX + 2);
    for (uint32_t i = t; i < heavy_t + 2; i += T) if (h[i]) atomicAdd(&copy[i], h[i]);
}
// A bin with more entries than LDS holds, i.e. many equal digits (a 0/1 witness without ZKG_SCALARS_MOSTLY_BITS, adversarial input, the
// partly filled top window): the workgroup streams the bin twice; lanes of a wavefront that hold the same fine bucket share one LDS atomic
// and get consecutive positions, so the stores of the dominant bucket are coalesced.  (Round 2 ran this as a kernel of its own: one
// more launch per sort whose workgroups all returned at once for uniform scalars.)
ZK_D void rx_fine_big_bin(const uint32_t *tmp, uint32_t fbits, uint32_t start, uint32_t cnt, size_t gb0, uint32_t *cf, uint32_t *of, uint32_t *cur, uint32_t *counts,
                          uint32_t *offsets, uint32_t *sorted, uint32_t *h, uint32_t heavy_t, uint32_t *class_hist) {
    const uint32_t FB = 1u << fbits, sh = 32 - fbits, low = (1u << sh) - 1, t = threadIdx.x, T = blockDim.x;
    const bool giant = cnt > 8 * RX_FINE_MAX;                         // many equal digits; below that (a dense top window) plain atomics are faster
    if (!giant) {
        for (uint32_t p = t; p < cnt; p += T) atomicAdd(&cf[tmp[start + p] >> sh], 1u);
    } else
    for (uint32_t p0 = 0; p0 < cnt; p0 += T) {
        uint32_t p = p0 + t; bool live = p < cnt; uint32_t f = live ? tmp[start + p] >> sh : 0;
        while (__any(live)) {
            uint32_t lf = __shfl(f, __ffsll((long long)__ballot(live)) - 1, 64);
            unsigned long long same = __ballot(live && f == lf);
            if (live && f == lf) { if ((same & ((1ull << (threadIdx.x & 63)) - 1)) == 0) atomicAdd(&cf[lf], (uint32_t)__popcll(same)); live = false; }
        }
    }
    __syncthreads();
    rx_fine_offsets(cf, of, FB, t, start, gb0, counts, offsets, h, heavy_t, class_hist);
    if (!giant) {
        for (uint32_t p = t; p < cnt; p += T) { uint32_t e = tmp[start + p], f = e >> sh; sorted[start + of[f] + atomicAdd(&cur[f], 1u)] = e & low; }
        return;
    }
    for (uint32_t p0 = 0; p0 < cnt; p0 += T) {
        uint32_t p = p0 + t; bool live = p < cnt; uint32_t e = live ? tmp[start + p] : 0, f = e >> sh;
        while (__any(live)) {
            uint32_t lf = __shfl(f, __ffsll((long long)__ballot(live)) - 1, 64);
            unsigned long long same = __ballot(live && f == lf), below = same & ((1ull << (threadIdx.x & 63)) - 1);
            uint32_t basepos = 0;
            if (live && f == lf && below == 0) basepos = atomicAdd(&cur[lf], (uint32_t)__popcll(same));
            basepos = __shfl(basepos, __ffsll((long long)same) - 1, 64);
            if (live && f == lf) { sorted[start + of[lf] + basepos + (uint32_t)__popcll(below)] = e & low; live = false; }
        }
    }
}
// second pass, one workgroup per (window, coarse bin).  A bin whose entries fit LDS (every bin of uniformly random scalars): entries stay in
// registers between the count and the placement, the sorted bin is assembled in LDS and written out in order
// (T threads: 1024, or 512 beside a running accumulation — see k_rx_scatter; the bin size the workgroup holds is the same)
template <int T>
__global__ __launch_bounds__(T) void k_rx_fine(const uint32_t *tmp, uint32_t fbits, uint32_t cbits, uint32_t B, const uint32_t *bin_cnt, const uint32_t *wtot, uint32_t *counts,
                                                uint32_t *offsets, size_t total, uint32_t *class_hist, uint32_t *sorted) {
    sort_wave_priority();
    extern __shared__ uint32_t lds_u32[];
    const uint32_t FB = 1u << fbits, sh = 32 - fbits, low = (1u << sh) - 1;
    // (the class counters and the start's accumulator lie in bufB, which is filled only after them: 38 KiB with 512 fine buckets, four workgroups per CU)
    uint32_t *bufB = lds_u32, *cf = bufB + RX_FINE_MAX, *of = cf + FB, *cur = of + FB, *h = bufB, *before = h + HEAVY_T_MAX + 2;
    const uint32_t cb = blockIdx.x, w = blockIdx.y, t = threadIdx.x, bin = (w << cbits) + cb;
    const size_t gb0 = (size_t)w * B + (size_t)cb * FB;
    for (uint32_t f = t; f < FB; f += T) { cf[f] = 0; cur[f] = 0; }
    for (uint32_t i = t; i < HEAVY_T_MAX + 2; i += T) h[i] = 0;
    // (one thread works the threshold out for the workgroup: its two 64-bit divisions in every wavefront of every bin are issue slots
    //  taken from the accumulation this kernel runs beside)
    if (t == 0) { before[0] = 0; before[1] = heavy_threshold_dev(offsets, total, 1); }       // (offsets[total]: k_rx_scatter stored it)
    __syncthreads();
    {
        const uint32_t v = wave_sum(rx_entries_before(bin_cnt, wtot, w, cb, cbits));
        if ((t & 63) == 0 && v) atomicAdd(&before[0], v);
    }
    __syncthreads();
    const uint32_t start = before[0], heavy_t = before[1], cnt = bin_cnt[bin];
    if (cnt > RX_FINE_MAX) { rx_fine_big_bin(tmp, fbits, start, cnt, gb0, cf, of, cur, counts, offsets, sorted, h, heavy_t, class_hist); return; }     // (uniform across the workgroup)
    uint32_t ent[RX_FINE_MAX / T];
#pragma unroll
    for (uint32_t j = 0; j < RX_FINE_MAX / T; ++j) {
        uint32_t p = t + j * T;
        ent[j] = p < cnt ? tmp[start + p] : 0xffffffffu;
        if (p < cnt) atomicAdd(&cf[ent[j] >> sh], 1u);
    }
    __syncthreads();
    rx_fine_offsets(cf, of, FB, t, start, gb0, counts, offsets, h, heavy_t, class_hist);
    __syncthreads();                                                  // h (in bufB) has been flushed
#pragma unroll
    for (uint32_t j = 0; j < RX_FINE_MAX / T; ++j) {
        if (t + j * T >= cnt) continue;
        uint32_t e = ent[j], f = e >> sh;
        bufB[of[f] + atomicAdd(&cur[f], 1u)] = e & low;
    }
    __syncthreads();
    for (uint32_t p = t; p < cnt; p += T) sorted[start + p] = bufB[p];
}

// ---- 5. bucket order by descending length (classes 0..heavy_t, heavy_t+1 = heavy) ------------------------
// (the two-pass sort counts the classes in k_rx_fine, where the bucket counts are made: this launch is the one-pass sort's)
__global__ __launch_bounds__(1024) void k_class_hist(const uint32_t *counts, const uint32_t *offsets, size_t total, uint32_t *class_hist) {
    sort_wave_priority();
    __shared__ uint32_t h[HEAVY_T_MAX + 2];
    const uint32_t heavy_t = heavy_threshold_dev(offsets, total, 1);
    const uint32_t t = threadIdx.x, nc = heavy_t + 2;
    for (uint32_t i = t; i < nc; i += 1024) h[i] = 0;
    __syncthreads();
    size_t gb = (size_t)blockIdx.x * 1024 + t;
    if (gb < total) { uint32_t c = counts[gb]; atomicAdd(&h[c > heavy_t ? heavy_t + 1 : c], 1u); }
    __syncthreads();
    for (uint32_t i = t; i < nc; i += 1024) if (h[i]) atomicAdd(&class_hist[i], h[i]);
}
// Every workgroup works out where the classes start itself — longest first: class c is scanned at position nc - 1 - c, an exclusive scan of
// the <= 1026 class counts — where a single-workgroup launch between the histogram and this kernel used to; the ranges inside a class are
// reserved from class_cursor, which the job's first kernel zeroes with the histogram.  The kernel runs beside an accumulation in a piece-wise
// job, so the scan is kept off its issue slots: inside the wavefronts that hold classes (two positions per thread; a uniform 2^20-point job has
// ~50 classes: one wavefront), their totals through LDS, and one thread's threshold for all.
// heavy_out (may be null): a word of pinned host memory that gets the count of heavy buckets — class heavy_t + 1, the lists the accumulation
// hands to k_heavy_parts / k_heavy_merge under the same threshold — so that a host that paces the launches knows whether that pair has work
// (msm_g1_host_scalars).
// recs (may be null: no 29-bit accumulation reads this sort): beside order[p] = gb the kernel leaves a LaneRec at position p — the bucket, where
// its list starts, how long it is (bit 31: heavy, decided HERE under the threshold the class histogram was counted with) and the list's first
// entry — everything k_bucket_accum29's lane p needs before its first base, in one coalesced 16-byte load instead of the chain order[p] ->
// offsets[gb], offsets[gb + 1] -> sorted[start] behind a threshold worked out in every wavefront.  `sorted` is complete when this kernel
// starts (k_rx_fine / k_place run before it on the same stream).  One coalesced load (offsets[gb]), one gather (sorted[start], requested
// before the class scan and waited for after it) and one 16-byte store per bucket are all it adds.
struct alignas(16) LaneRec { uint32_t gb, start, len /* bit 31: heavy */, first /* sorted[start]; 0 for an empty list */; };
static constexpr uint32_t LANE_HEAVY = 0x80000000u;
__global__ __launch_bounds__(1024) void k_order_place(const uint32_t *counts, const uint32_t *offsets, size_t total, const uint32_t *class_hist, uint32_t *class_cursor,
                                                       uint32_t *order, uint32_t *heavy_out, const uint32_t *sorted, LaneRec *recs) {
    sort_wave_priority();
    __shared__ uint32_t h[HEAVY_T_MAX + 2], first[HEAVY_T_MAX + 2], wave_total[16], threshold;
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (uint32_t i = t; i < HEAVY_T_MAX + 2; i += 1024) h[i] = 0;
    if (t == 0) threshold = heavy_threshold_dev(offsets, total, 1);
    size_t gb = (size_t)blockIdx.x * 1024 + t;
    uint32_t c = 0, start = 0, head = 0;
    if (gb < total) {
        c = counts[gb];
        if (recs) { start = offsets[gb]; if (c) head = sorted[start]; }
    }
    __syncthreads();
    const uint32_t heavy_t = threshold, nc = heavy_t + 2;
    uint32_t cls = 0, rank = 0;
    if (gb < total) { cls = c > heavy_t ? heavy_t + 1 : c; rank = atomicAdd(&h[cls], 1u); }
    // HEAVY_T_MAX + 2 = 1026 classes at most: thread t takes positions 2t and 2t + 1 of the reversed order
    uint32_t v0 = 0, v1 = 0, incl = 0;
    if (128 * wave < nc) {                                              // (uniform in the wavefront)
        for (uint32_t k = 0; k < CLASS_HIST_COPIES; ++k) {
            const uint32_t *copy = class_hist + k * (HEAVY_T_MAX + 2);
            if (2 * t < nc) v0 += copy[nc - 1 - 2 * t];
            if (2 * t + 1 < nc) v1 += copy[nc - 2 - 2 * t];
        }
        if (heavy_out && blockIdx.x == 0 && t == 0) *heavy_out = v0;      // position 0 of the reversed order: class heavy_t + 1, summed over its copies
        incl = v0 + v1;
        for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(incl, d, 64); if (lane >= d) incl += y; }
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    if (128 * wave < nc) {
        uint32_t before = incl - v0 - v1;
        for (uint32_t k = 0; k < wave; ++k) before += wave_total[k];
        if (2 * t < nc) first[nc - 1 - 2 * t] = before;
        if (2 * t + 1 < nc) first[nc - 2 - 2 * t] = before + v0;
    }
    __syncthreads();
    for (uint32_t i = t; i < nc; i += 1024) if (h[i]) h[i] = first[i] + atomicAdd(&class_cursor[i], h[i]);      // reserve a range per class
    __syncthreads();
    if (gb < total) {
        const uint32_t p = h[cls] + rank;
        order[p] = (uint32_t)gb;
        if (recs) *reinterpret_cast<uint4 *>(recs + p) = make_uint4((uint32_t)gb, start, c | (c > heavy_t ? LANE_HEAVY : 0u), head);
    }
}

// ---- 6. bucket accumulation (dominant kernel) -------------------------------------------------------------
template <class F, bool PLAIN>
__global__ __launch_bounds__(256) void k_bucket_accum(const ViewSet<F> views, const uint32_t *sorted, const uint32_t *offsets, const uint32_t *order,
                                                       size_t lanes /* <= total buckets: the first `lanes` entries of order */, XYZZ<F> *buckets, HeavyItem *items,
                                                       HeavyBucket *heavy, uint32_t *counters /* per set: [0] items, [1] heavy buckets */, SetLayout L) {
    size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= lanes) return;
    const size_t total_buckets = L.buckets;
    const uint32_t set = blockIdx.y;
    const BaseView<F> bases = views.v[set];
    buckets += set * L.buckets; items += set * L.items; heavy += set * L.heavy; counters += 2 * set;
    const uint32_t heavy_t = heavy_threshold_dev(offsets, total_buckets, sizeof(F) > sizeof(Fq) ? 3 : 1);   // a G2 addition costs ~3x a G1 addition
    const uint32_t gb = order[tid];
    uint32_t k = offsets[gb], end = offsets[gb + 1];
    if (end - k > heavy_t) {
        uint32_t nparts = (end - k + HEAVY_S - 1) / HEAVY_S;
        uint32_t first = atomicAdd(&counters[0], nparts);
        for (uint32_t p = 0; p < nparts; ++p) { uint32_t a = k + p * HEAVY_S; items[first + p] = {a, a + HEAVY_S < end ? a + HEAVY_S : end, gb, nparts == 1}; }
        if (nparts > 1) heavy[atomicAdd(&counters[1], 1u)] = {gb, first, nparts};                   // a single part writes its bucket itself
        return;
    }
    XYZZ<F> acc = XYZZ<F>::inf();
    if (k < end) {
        // two loads deep (see k_bucket_accum29): the base of entry k + 1 and the index of entry k + 2 arrive under the addition of entry k
        uint32_t e = sorted[k], e_next = k + 1 < end ? sorted[k + 1] : 0;
        Affine<F> p = bases.template load<PLAIN>(e, gb);
        while (true) {
            Affine<F> cur = p; uint32_t ce = e;
            ++k;
            if (k < end) { e = e_next; p = bases.template load<PLAIN>(e, gb); if (k + 1 < end) e_next = sorted[k + 1]; }
            if (ce & 1u) cur.y = cur.y.neg();
            acc.madd(cur);
            if (k >= end) break;
        }
    }
    buckets[gb] = acc.normalized();
}

// ---- 6'. the same accumulation for a plain G1 base set on the 29-bit representation (fq29.hip.hpp): 10 products of 895 cycles instead of
//      1173 and carry-free additions per mixed addition.  The bases are converted once per launch into 64-byte packed records (Rec64, k_bases_to29: two
//      products per point against the 160 the point costs in the loop); an accumulator is converted back when its bucket is written, so
//      everything downstream (heavy parts, fold, reduction, host) sees the same XYZZ<Fq> buckets as before.
__global__ __launch_bounds__(256) void k_bases_to29(const Affine<Fq> *in, size_t n, Rec64 *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<Fq> a = in[i];
    store_rec64(out + i, f29::to29(a.x), f29::to29(a.y), a.is_inf());
}
ZK_D Affine29 load29(const Rec64 *bases, uint32_t e) { return load_rec64(bases + (e >> 1)); }
ZK_D Rec64 load29_raw(const Rec64 *bases, uint32_t e) { return load_rec64_raw(bases + (e >> 1)); }
// WAVES: wavefronts per SIMD the register allocation aims for (2: no spill in the loop; 3: 168 registers and a 232-byte spill frame)
// ACC29_VGPRS: left to itself the allocator spends all 256 registers two wavefronts per SIMD allow (253 for OUT29: loop-invariant constants
// parked in registers) and nothing else fits on the SIMD beside them.  Capped at 192 the addition's instruction stream is the same (2 281
// instructions, the spills all on the exceptional doubling path), and 128 registers per SIMD stay free: the digit sort of the NEXT piece of a
// piece-wise job (msm_g1_host_scalars) runs on the same compute units at once instead of waiting for accumulation workgroups to retire.
// level_stride != 0: `bases` is a per-window table (level w = 2^(c w) P_i, level_stride records apart) and a bucket reads its window's level
// OUT29: the buckets are Bucket29 records (the plain G1 path: the reduction reads them without conversion) instead of canonical XYZZ<Fq>
// (table launches: the fold in between works on 32-bit limbs).  resume (OUT29 only): the buckets hold the sums of the job's earlier pieces
// (piece-wise multi-exponentiation, msm_g1_host_scalars): a lane continues its bucket's accumulator, an empty list leaves it alone, and a
// heavy bucket's old value joins its parts in k_heavy_merge.
// A lane starts from its LaneRec (k_order_place): no threshold is worked out here (two 64-bit divisions in every wavefront, ~250 scalar
// instructions in front of the first load of order[]), and the chain order[] -> offsets[] -> sorted[] -> base, four round trips behind the
// one for the threshold, is two: the record, then the first base with the second index and the bucket.  Counters, one launch alone: 17 - 30 %
// fewer wave cycles spent waiting, 1 - 4 % fewer wave cycles; the launches' durations fall by 3 - 5 us each, not by the ~60 us per launch
// that a fit over the four pieces' durations leaves unexplained: the prologue was not that cost.
// ACC29_WG: the kernel has no LDS and no barrier, so a workgroup is only what the dispatcher hands out and takes back: with four wavefronts
// a slot is refilled once all four lists are done; one wavefront per workgroup refills each as it ends (traced: the four launches of a step
// 1366 -> 1292 us with the records, 1366 -> 1347 us without them).
template <int WAVES, bool OUT29>
__global__ __launch_bounds__(ACC29_WG, WAVES) ZK_VGPR_CAP(ACC29_VGPRS) void k_bucket_accum29(const Rec64 *bases, size_t level_stride, uint32_t B, const uint32_t *sorted, const LaneRec *recs,
                                                         size_t lanes, void *buckets_, HeavyItem *items, HeavyBucket *heavy, uint32_t *counters, int flags /* 1: resume, 2: critical path */) {
    crit_wave_priority(flags & 2);
    const int resume = flags & 1;
    size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= lanes) return;
    const uint4 rec = *reinterpret_cast<const uint4 *>(recs + tid);             // LaneRec {gb, start, len | heavy flag, first entry}: the lane's first memory instruction
    const uint32_t gb = rec.x, len = rec.z & ~LANE_HEAVY;
    if (level_stride) bases += (size_t)(gb / B) * level_stride;
    uint32_t k = rec.y, end = k + len;
    if (rec.z & LANE_HEAVY) {                                                   // as k_bucket_accum: long lists go to k_heavy_parts / k_heavy_merge (k_order_place applied the threshold)
        uint32_t nparts = (end - k + HEAVY_S - 1) / HEAVY_S;
        uint32_t first = atomicAdd(&counters[0], nparts);
        const bool single = nparts == 1 && !resume;                             // a lone part may write its bucket itself only when nothing is there yet
        for (uint32_t p = 0; p < nparts; ++p) { uint32_t a = k + p * HEAVY_S; items[first + p] = {a, a + HEAVY_S < end ? a + HEAVY_S : end, gb, single}; }
        if (!single) heavy[atomicAdd(&counters[1], 1u)] = {gb, first, nparts};
        return;
    }
    XYZZ29 acc; bool inf = true;
    acc.x = acc.y = acc.zz = acc.zzz = Fq29::zero();
    // Everything the first addition needs is requested on the record alone, before anything is waited for: the first entry came with the
    // record, so its base, the second index and, under resume, the bucket go out together — two round trips in front of the first addition
    // (the loop's first turn requests the third index before it waits for the second)
    uint32_t e = rec.w, e_next = 0;
    Rec64 p;                                                                    // (kept packed while in flight: unpacked when its addition starts)
    if (k < end) { if (k + 1 < end) e_next = sorted[k + 1]; p = load29_raw(bases, e); }
    if constexpr (OUT29) {
        if (resume) {
            if (k >= end) return;                                               // nothing of this piece lands here: the bucket keeps its sum
            const Bucket29 old = load_bucket29_raw(reinterpret_cast<const Bucket29 *>(buckets_) + gb);
            uint32_t any = 0;
#pragma unroll
            for (int j = 0; j < 9; ++j) { acc.x.v[j] = old.x[j]; acc.y.v[j] = old.y[j]; acc.zz.v[j] = old.zz[j]; acc.zzz.v[j] = old.zzz[j]; any |= old.zz[j]; }
            inf = any == 0;
        }
    }
    if (k < end) {
        // two loads deep: under the addition of entry k the base of entry k + 1 arrives (its address came from an index loaded one
        // addition earlier) and the index of entry k + 2 — neither the index nor the base is ever waited for right after it was requested
        while (true) {
            const Rec64 curw = p; const uint32_t ce = e;
            ++k;
            if (k < end) { e = e_next; p = load29_raw(bases, e); if (k + 1 < end) e_next = sorted[k + 1]; }
            const Affine29 cur = unpack_rec64(curw);
            if (!cur.inf) {
                Fq29 bx, by;
#pragma unroll
                for (int j = 0; j < 9; ++j) { bx.v[j] = cur.x[j]; by.v[j] = cur.y[j]; }
                if (ce & 1u) by = f29::neg(f29::S2_1, by);
                if (__builtin_expect(!acc.madd(bx, by, inf), 0)) {
                    // b == +-accumulator (a duplicated base under equal digits): the doubling / cancellation cases on the 32-bit path
                    // (These lines, down to the accumulator's new value, have a COPY in csrc/capi.hip, fq29_madd_fallback_copy, for the known-answer hook zkg_fq29_op: keep the two alike.)
                    XYZZ<Fq> a32 = {f29::from29(acc.x), f29::from29(acc.y), f29::from29(acc.zz), f29::from29(acc.zzz)};
                    a32.madd(Affine<Fq>{f29::from29(bx), f29::from29(f29::norm(by))});
                    if (a32.is_inf()) inf = true;
                    else { acc.x = f29::to29(a32.x.normalized()); acc.y = f29::to29(a32.y.normalized()); acc.zz = f29::to29(a32.zz.normalized()); acc.zzz = f29::to29(a32.zzz.normalized()); }
                }
            }
            if (k >= end) break;
        }
    }
    if constexpr (OUT29) store_bucket29(reinterpret_cast<Bucket29 *>(buckets_) + gb, acc, inf);
    else {
        XYZZ<Fq> *buckets = reinterpret_cast<XYZZ<Fq> *>(buckets_);
        if (inf) buckets[gb] = XYZZ<Fq>::inf().normalized();
        else buckets[gb] = XYZZ<Fq>{f29::from29(acc.x), f29::from29(acc.y), f29::from29(acc.zz), f29::from29(acc.zzz)};
    }
}

// A point in LDS, padded to 144 B (G1) / 272 B (G2): at the natural 128 / 256-byte stride consecutive points start on the same four banks.
// Measured effect: k_bucket_reduce 363 -> 354 us at 2^19 buckets — the kernels that use it are bound by the multiplications of their
// addition chains (two wavefronts per SIMD: 1.16 us per dependent product), not by the LDS port.
template <class F> struct alignas(16) LdsPoint {
    XYZZ<F> p; uint32_t pad[4];
    ZK_D LdsPoint &operator=(const XYZZ<F> &v) { p = v; return *this; }
    ZK_D operator const XYZZ<F> &() const { return p; }
    ZK_D XYZZ<F> normalized() const { return p.normalized(); }
};

// LDS tree reduction of seg[0..n) into seg[0] by `nthreads` threads (tid = 0..nthreads-1, n a power of two <= nthreads;
// every thread of the group must call it; barrier() synchronises the group).  Levels with at most nthreads/4 pairs share
// each addition across a DPP quad (nthreads is a multiple of 64, so quads never straddle groups).
template <class F, class Barrier>
ZK_D void lds_tree_reduce(LdsPoint<F> *seg, uint32_t n, uint32_t tid, uint32_t nthreads, Barrier barrier) {
    for (uint32_t d = n / 2; d >= 1; d >>= 1) {
        if (4 * d <= nthreads) {
            uint32_t t = tid >> 2, q = tid & 3;
            if (t < d) { XYZZ<F> a = seg[t]; xyzz_add_quad(a, seg[t + d].p, q); if (q == 0) seg[t] = a; }
        } else if (tid < d) { XYZZ<F> a = seg[tid]; a.add(seg[tid + d]); seg[tid] = a; }
        barrier();
    }
}

// one wavefront per heavy part: 64 lanes stride over <= HEAVY_S entries, then a 6-level LDS tree
// out29 (F = Fq only): the buckets are Bucket29 records (see k_bucket_accum29)
template <class F> ZK_D void put_bucket(XYZZ<F> *buckets, uint32_t gb, const XYZZ<F> &v, int out29) {
    if constexpr (sizeof(F) == sizeof(Fq)) { if (out29) { store_bucket29(reinterpret_cast<Bucket29 *>(buckets) + gb, v); return; } }
    buckets[gb] = v;
}
template <class F>
__global__ __launch_bounds__(256) void k_heavy_parts(const ViewSet<F> views, const uint32_t *sorted, const HeavyItem *items,
                                                      const uint32_t *counters, XYZZ<F> *partials, XYZZ<F> *buckets, SetLayout L, int out29) {
    extern __shared__ unsigned char red_smem[];
    LdsPoint<F> *sh = reinterpret_cast<LdsPoint<F> *>(red_smem);            // 256 points
    const uint32_t set = blockIdx.y;
    const BaseView<F> bases = views.v[set];
    items += set * L.items; partials += set * L.partials; buckets += set * L.buckets;          // (out29: one set per launch, no offset)
    const uint32_t n_items = counters[2 * set], t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (uint32_t base = blockIdx.x * 4; base < n_items; base += gridDim.x * 4) {      // uniform trip count per workgroup
        uint32_t it = base + wv;
        XYZZ<F> acc = XYZZ<F>::inf();
        if (it < n_items) {
            HeavyItem h = items[it];
            for (uint32_t k = h.start + lane; k < h.end; k += 64) {
                uint32_t e = sorted[k];
                Affine<F> p = bases.load(e, h.gb);
                if (e & 1u) p.y = p.y.neg();
                acc.madd(p);
            }
        }
        sh[t] = acc;
        __syncthreads();
        lds_tree_reduce<F>(sh + wv * 64, 64, lane, 64, [] { __syncthreads(); });      // the four wavefronts run their trees in step
        if (lane == 0 && it < n_items) { if (items[it].single) put_bucket<F>(buckets, items[it].gb, sh[t].normalized(), out29); else partials[it] = sh[t].normalized(); }
        __syncthreads();
    }
}

// one workgroup per heavy bucket: strided sum of its parts' partials, LDS tree, write the bucket
template <class F>
__global__ __launch_bounds__(256) void k_heavy_merge(const HeavyBucket *heavy, const uint32_t *counters, const XYZZ<F> *partials, XYZZ<F> *buckets, SetLayout L, int out29, int resume) {
    extern __shared__ unsigned char red_smem[];
    LdsPoint<F> *sh = reinterpret_cast<LdsPoint<F> *>(red_smem);
    const uint32_t set = blockIdx.y;
    heavy += set * L.heavy; partials += set * L.partials; buckets += set * L.buckets;
    const uint32_t n_heavy = counters[2 * set + 1], t = threadIdx.x;
    for (uint32_t hb = blockIdx.x; hb < n_heavy; hb += gridDim.x) {
        HeavyBucket h = heavy[hb];
        XYZZ<F> acc = XYZZ<F>::inf();
        for (uint32_t p = t; p < h.nparts; p += 256) acc.add(partials[h.first_item + p]);
        if constexpr (sizeof(F) == sizeof(Fq)) {
            if (resume && out29 && t == 255) acc.add(bucket29_to_xyzz(load_bucket29_raw(reinterpret_cast<const Bucket29 *>(buckets) + h.gb)));   // the earlier pieces' sum
        }
        sh[t] = acc;
        __syncthreads();
        lds_tree_reduce<F>(sh, 256, t, 256, [] { __syncthreads(); });
        if (t == 0) put_bucket<F>(buckets, h.gb, sh[0].normalized(), out29);
        __syncthreads();
    }
}

// ---- 7. bucket reduction: per chunk of RED_CHUNK buckets emit P = sum X_i and U = sum i*X_i (i 0-based in chunk).
//      RedGeom<F>::LANES logical lanes per workgroup, each played by the four lanes of a DPP quad (xyzz_add_quad): the kernel is a
//      dependency chain of 2(L-1) + 2 log2(LANES) + 2 additions, and the quad turns each addition's 14 dependent
//      multiplications into 4 rounds.
template <class F, int RED_L_LOG>
__global__ __launch_bounds__(RedGeom<F>::THREADS) void k_bucket_reduce(const XYZZ<F> *buckets, uint32_t B, uint32_t chunks_per_window, XYZZ<F> *out,
                                                                       size_t in_set_stride, size_t out_set_stride) {
    constexpr int RED_LANES = RedGeom<F>::LANES, RED_L = 1 << RED_L_LOG, RED_CHUNK = RED_LANES * RED_L;
    extern __shared__ unsigned char red_smem[];
    LdsPoint<F> *sh = reinterpret_cast<LdsPoint<F> *>(red_smem);              // 2 * RED_LANES points
    const uint32_t t = threadIdx.x >> 2, q = threadIdx.x & 3;          // logical lane, position in its quad
    const uint32_t w = blockIdx.x / chunks_per_window, ch = blockIdx.x % chunks_per_window;
    const XYZZ<F> *X = buckets + blockIdx.y * in_set_stride + (size_t)w * B;
    out += blockIdx.y * out_set_stride;
    const uint32_t base = ch * RED_CHUNK + t * RED_L;
    // lane-local running sums: S = sum_j X_j, T0 = sum_j j*X_j
    XYZZ<F> run = XYZZ<F>::inf(), T0 = XYZZ<F>::inf();
    XYZZ<F> cur = (base + RED_L - 1 < B) ? X[base + RED_L - 1] : XYZZ<F>::inf();
    for (int j = RED_L - 1; j >= 1; --j) {
        XYZZ<F> nxt = (base + j - 1 < B) ? X[base + j - 1] : XYZZ<F>::inf();      // next bucket arrives under the two additions
        xyzz_add_quad(run, cur, q);
        xyzz_add_quad(T0, run, q);
        cur = nxt;
    }
    xyzz_add_quad(run, cur, q);
    // inclusive suffix scan of S over logical lanes (Hillis-Steele through LDS): Q_t = sum_{u>=t} S_u
    XYZZ<F> Q = run;
    for (uint32_t d = 1; d < RED_LANES; d <<= 1) {
        if (q == 0) sh[t] = Q;
        __syncthreads();
        if (t + d < RED_LANES) xyzz_add_quad(Q, sh[t + d].p, q);
        __syncthreads();
    }
    // sum_t t*S_t = sum_{t>=1} Q_t ; tree-reduce Q (t>=1) in sh[0..), T0 in sh[RED_LANES..)
    XYZZ<F> P = Q;                                                  // logical lane 0: total of the chunk
    if (q == 0) { sh[t] = (t >= 1) ? Q : XYZZ<F>::inf(); sh[RED_LANES + t] = T0; }
    __syncthreads();
    for (uint32_t d = RED_LANES / 2; d >= 1; d >>= 1) {
        if (t < d) { XYZZ<F> a = sh[t]; xyzz_add_quad(a, sh[t + d].p, q); if (q == 0) sh[t] = a; }
        else if (t >= RED_LANES / 2 && t < RED_LANES / 2 + d) {
            uint32_t u = RED_LANES + (t - RED_LANES / 2);
            XYZZ<F> a = sh[u]; xyzz_add_quad(a, sh[u + d].p, q); if (q == 0) sh[u] = a;
        }
        __syncthreads();
    }
    if (t == 0) {
        XYZZ<F> E = sh[0];
        for (int i = 0; i < RED_L_LOG; ++i) E = E.dbl();            // * RED_L
        xyzz_add_quad(E, sh[RED_LANES].p, q);
        if (q == 0) { out[2 * (size_t)blockIdx.x] = P.normalized(); out[2 * (size_t)blockIdx.x + 1] = E.normalized(); }
    }
}

// ---- 7'. the same reduction for G1 on the 29-bit representation (fq29.hip.hpp, xyzz29_add_quad): the kernel is a chain of dependent
//      products at two wavefronts per SIMD, where a 29-bit product takes 930 cycles against 1293.  Buckets arrive as the accumulation wrote
//      them (canonical XYZZ<Fq>) and are converted on load, one coordinate per lane of the quad; the two chunk results leave as XYZZ<Fq>.
struct alignas(16) LdsPoint29 { XYZZ29q p; uint32_t pad[4]; };
template <bool IN29> ZK_D XYZZ29q load_bucket29(const void *X_, uint32_t i, uint32_t B, uint32_t q) {
    if (i >= B) return XYZZ29q::inf();
    if constexpr (IN29) {                                                        // as the accumulation left it: no conversion, every lane of the quad reads the record
        const Bucket29 b = load_bucket29_raw(reinterpret_cast<const Bucket29 *>(X_) + i);
        XYZZ29q r;
#pragma unroll
        for (int j = 0; j < 9; ++j) { r.x.v[j] = b.x[j]; r.y.v[j] = b.y[j]; r.zz.v[j] = b.zz[j]; r.zzz.v[j] = b.zzz[j]; }
        return r;
    } else {
        const XYZZ<Fq> b = reinterpret_cast<const XYZZ<Fq> *>(X_)[i];
        if (b.is_inf()) return XYZZ29q::inf();
        return quad_load29(b.x, b.y, b.zz, b.zzz, q);
    }
}
ZK_D XYZZ<Fq> store_point29(const XYZZ29q &p) {
    if (p.is_inf()) return XYZZ<Fq>::inf().normalized();
    return {f29::from29(p.x), f29::from29(p.y), f29::from29(p.zz), f29::from29(p.zzz)};
}
// (only RED_L_LOG_TINY is instantiated: the longer chains take the pair and lane kernels below)
template <int RED_L_LOG, bool IN29>
__global__ __launch_bounds__(RedGeom<Fq>::THREADS) void k_bucket_reduce29(const void *buckets, uint32_t B, uint32_t chunks_per_window, XYZZ<Fq> *out,
                                                                          size_t in_set_stride, size_t out_set_stride, int critical) {
    crit_wave_priority(critical);
    constexpr int RED_LANES = RedGeom<Fq>::LANES, RED_L = 1 << RED_L_LOG, RED_CHUNK = RED_LANES * RED_L;
    extern __shared__ unsigned char red_smem[];
    LdsPoint29 *sh = reinterpret_cast<LdsPoint29 *>(red_smem);             // 2 * RED_LANES points
    const uint32_t t = threadIdx.x >> 2, q = threadIdx.x & 3;
    const uint32_t w = blockIdx.x / chunks_per_window, ch = blockIdx.x % chunks_per_window;
    const size_t elem = IN29 ? sizeof(Bucket29) : sizeof(XYZZ<Fq>);
    const void *X = reinterpret_cast<const char *>(buckets) + (blockIdx.y * in_set_stride + (size_t)w * B) * elem;
    out += blockIdx.y * out_set_stride;
    const uint32_t base = ch * RED_CHUNK + t * RED_L;
    XYZZ29q run = XYZZ29q::inf(), T0 = XYZZ29q::inf();
    XYZZ29q cur = load_bucket29<IN29>(X, base + RED_L - 1, B, q);
    for (int j = RED_L - 1; j >= 1; --j) {
        const XYZZ29q nxt = load_bucket29<IN29>(X, base + j - 1, B, q);
        xyzz29_add_quad(run, cur, q);
        xyzz29_add_quad(T0, run, q);
        cur = nxt;
    }
    xyzz29_add_quad(run, cur, q);
    XYZZ29q Q = run;                                                     // inclusive suffix scan of the lane sums over logical lanes
    for (uint32_t d = 1; d < RED_LANES; d <<= 1) {
        if (q == 0) sh[t].p = Q;
        __syncthreads();
        if (t + d < RED_LANES) xyzz29_add_quad(Q, sh[t + d].p, q);
        __syncthreads();
    }
    const XYZZ29q P = Q;                                                 // logical lane 0: total of the chunk
    if (q == 0) { sh[t].p = (t >= 1) ? Q : XYZZ29q::inf(); sh[RED_LANES + t].p = T0; }
    __syncthreads();
    for (uint32_t d = RED_LANES / 2; d >= 1; d >>= 1) {
        if (t < d) { XYZZ29q a = sh[t].p; xyzz29_add_quad(a, sh[t + d].p, q); if (q == 0) sh[t].p = a; }
        else if (t >= RED_LANES / 2 && t < RED_LANES / 2 + d) {
            const uint32_t u = RED_LANES + (t - RED_LANES / 2);
            XYZZ29q a = sh[u].p; xyzz29_add_quad(a, sh[u + d].p, q); if (q == 0) sh[u].p = a;
        }
        __syncthreads();
    }
    if (t == 0) {
        XYZZ<Fq> E = store_point29(sh[0].p);
        for (int i = 0; i < RED_L_LOG; ++i) E = E.dbl();                 // * RED_L (RED_L_LOG doublings, once per workgroup: the 32-bit path)
        E.add(store_point29(sh[RED_LANES].p));
        if (q == 0) { out[2 * (size_t)blockIdx.x] = store_point29(P); out[2 * (size_t)blockIdx.x + 1] = E.normalized(); }
    }
}

// ---- 7''. the same reduction with every addition shared by a PAIR of lanes (fq29.hip.hpp xyzz29_add_pair): the quad kernel above is bound by
//      the quad addition's issue (2.8 us per wavefront-addition: 16 lane-products and as many operand moves again for the 14 products an addition
//      needs), a pair spends about half of that per addition at the same depth.  128 logical lanes = 256 threads, one wavefront per SIMD; same
//      chunks, same chain (running sums, suffix scan, two trees), same two results per chunk as k_bucket_reduce29.
ZK_D Half29 lds_load_half29(const LdsPoint29 *p, uint32_t r) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p) + 9 * r;
    Half29 h;
#pragma unroll
    for (int i = 0; i < 9; ++i) { h.c0.v[i] = w[i]; h.c1.v[i] = w[18 + i]; }
    return h;
}
ZK_D void lds_store_half29(LdsPoint29 *p, const Half29 &h, uint32_t r) {
    uint32_t *w = reinterpret_cast<uint32_t *>(p) + 9 * r;
#pragma unroll
    for (int i = 0; i < 9; ++i) { w[i] = h.c0.v[i]; w[18 + i] = h.c1.v[i]; }
}
template <bool IN29> ZK_D Half29 load_half29(const void *X_, uint32_t i, uint32_t B, uint32_t r) {
    if (i >= B) return Half29::inf();
    if constexpr (IN29) {                                                        // this lane's two coordinates of the 29-bit record
        const uint32_t *w = reinterpret_cast<const uint32_t *>(reinterpret_cast<const Bucket29 *>(X_) + i) + 9 * r;
        Half29 h;
#pragma unroll
        for (int j = 0; j < 9; ++j) { h.c0.v[j] = w[j]; h.c1.v[j] = w[18 + j]; }
        return h;
    } else {                                                                     // canonical XYZZ<Fq> (a table launch's folded buckets): two conversions per lane
        const Fq *f = reinterpret_cast<const Fq *>(reinterpret_cast<const XYZZ<Fq> *>(X_) + i);
        const Fq c0 = f[r], c1 = f[2 + r];
        if (c1.is_zero()) return Half29::inf();
        Fq29 to; for (int j = 0; j < 9; ++j) to.v[j] = f29::TO[j];
        Half29 h; f29::mul2(h.c0, h.c1, f29::unpack(c0), to, f29::unpack(c1), to);
        return h;
    }
}
template <int RED_L_LOG, bool IN29>
__global__ __launch_bounds__(2 * RedGeom<Fq>::LANES) void k_bucket_reduce29p(const void *buckets, uint32_t B, uint32_t chunks_per_window, XYZZ<Fq> *out,
                                                                             size_t in_set_stride, size_t out_set_stride, int critical) {
    crit_wave_priority(critical);
    constexpr int RED_LANES = RedGeom<Fq>::LANES, RED_L = 1 << RED_L_LOG, RED_CHUNK = RED_LANES * RED_L;
    extern __shared__ unsigned char red_smem[];
    LdsPoint29 *sh = reinterpret_cast<LdsPoint29 *>(red_smem);             // 2 * RED_LANES points
    const uint32_t t = threadIdx.x >> 1, r = threadIdx.x & 1;             // logical lane, place in its pair
    const uint32_t w = blockIdx.x / chunks_per_window, ch = blockIdx.x % chunks_per_window;
    const size_t elem = IN29 ? sizeof(Bucket29) : sizeof(XYZZ<Fq>);
    const void *X = reinterpret_cast<const char *>(buckets) + (blockIdx.y * in_set_stride + (size_t)w * B) * elem;
    out += blockIdx.y * out_set_stride;
    const uint32_t base = ch * RED_CHUNK + t * RED_L;
    Half29 run = Half29::inf(), T0 = Half29::inf();
    Half29 cur = load_half29<IN29>(X, base + RED_L - 1, B, r);
    for (int j = RED_L - 1; j >= 1; --j) {
        const Half29 nxt = load_half29<IN29>(X, base + j - 1, B, r);     // the next bucket arrives under the two additions
        xyzz29_add_pair(run, cur, r);
        xyzz29_add_pair(T0, run, r);
        cur = nxt;
    }
    xyzz29_add_pair(run, cur, r);
    Half29 Q = run;                                                      // inclusive suffix scan of the lane sums over logical lanes
    for (uint32_t d = 1; d < RED_LANES; d <<= 1) {
        lds_store_half29(sh + t, Q, r);
        __syncthreads();
        if (t + d < RED_LANES) xyzz29_add_pair(Q, lds_load_half29(sh + t + d, r), r);
        __syncthreads();
    }
    const Half29 P = Q;                                                  // logical lane 0: total of the chunk
    lds_store_half29(sh + t, t >= 1 ? Q : Half29::inf(), r); lds_store_half29(sh + RED_LANES + t, T0, r);
    __syncthreads();
    for (uint32_t d = RED_LANES / 2; d >= 1; d >>= 1) {
        if (t < d) { Half29 a = lds_load_half29(sh + t, r); xyzz29_add_pair(a, lds_load_half29(sh + t + d, r), r); lds_store_half29(sh + t, a, r); }
        else if (t >= RED_LANES / 2 && t < RED_LANES / 2 + d) {
            const uint32_t u = RED_LANES + (t - RED_LANES / 2);
            Half29 a = lds_load_half29(sh + u, r); xyzz29_add_pair(a, lds_load_half29(sh + u + d, r), r); lds_store_half29(sh + u, a, r);
        }
        __syncthreads();
    }
    if (t == 0) lds_store_half29(sh + 1, P, r);                          // (slot 1 is free once the trees are through)
    __syncthreads();
    if (threadIdx.x == 0) {
        XYZZ<Fq> E = store_point29(sh[0].p);
        for (int i = 0; i < RED_L_LOG; ++i) E = E.dbl();                 // * RED_L (RED_L_LOG doublings, once per workgroup: the 32-bit path)
        E.add(store_point29(sh[RED_LANES].p));
        out[2 * (size_t)blockIdx.x] = store_point29(sh[1].p); out[2 * (size_t)blockIdx.x + 1] = E.normalized();
    }
}

// ---- 7''. the large reduction with its first phase on single lanes.  k_bucket_reduce29p walks a logical lane's 16 buckets as 31 pair
//      additions in sequence — two thirds of its chain, at 126 ns of a SIMD per addition.  Here each of the workgroup's 256 THREADS takes 8
//      buckets alone (xyzz29_add_lane: 85 ns of a SIMD per addition, 64 additions per wavefront-step): 15 steps of 5.6 us instead of 31 of
//      4.7.  The 256 (sum, weighted sum) results go through LDS to the 128 pairs, two entries each, for the same scan and trees:
//          sum_b b B_b (b local, 8 i + j)  =  8 sum_i i R_i + sum_i T_i,      sum_i i R_i = sum_{i >= 1} (suffix sum of R at i),
//      a pair owning entries 2t, 2t + 1 adds four pair additions to the old chain (their sum for the scan, the odd entry's suffix, the
//      pair's two suffixes, the pair's two weighted sums).  Same chunks as the pair kernel; three results per chunk (see the end).
//      Bucket29 input only (the plain G1 path); the other shapes keep the pair / quad kernels.
__global__ __launch_bounds__(2 * RedGeom<Fq>::LANES) void k_bucket_reduce29l(const Bucket29 *buckets, uint32_t B, uint32_t chunks_per_window, XYZZ<Fq> *out,
                                                                             size_t in_set_stride, size_t out_set_stride, int critical) {
    crit_wave_priority(critical);
    constexpr int RED_LANES = RedGeom<Fq>::LANES, NT = 2 * RED_LANES, PER = 8, RED_CHUNK = NT * PER;      // = RED_LANES << RED_L_LOG_LARGE
    static_assert(RED_CHUNK == (RED_LANES << RED_L_LOG_LARGE), "the lane-form reduction keeps the large reduction's chunks");
    extern __shared__ unsigned char red_smem[];
    LdsPoint29 *sh = reinterpret_cast<LdsPoint29 *>(red_smem);             // 2 * NT points
    const uint32_t i = threadIdx.x;
    const uint32_t w = blockIdx.x / chunks_per_window, ch = blockIdx.x % chunks_per_window;
    const Bucket29 *X = buckets + blockIdx.y * in_set_stride + (size_t)w * B;
    out += blockIdx.y * out_set_stride;
    {   // phase 1: this thread's 8 buckets — run = their sum, T0 = sum_j j B_(base + j)
        const uint32_t base = ch * RED_CHUNK + i * PER;
        XYZZ29q run = XYZZ29q::inf(), T0 = XYZZ29q::inf();
        XYZZ29q cur = load_bucket29<true>(X, base + PER - 1, B, 0);
        for (int j = PER - 1; j >= 1; --j) {
            const XYZZ29q nxt = load_bucket29<true>(X, base + j - 1, B, 0);  // the next bucket arrives under the two additions
            xyzz29_add_lane(run, cur);
            xyzz29_add_lane(T0, run);
            cur = nxt;
        }
        xyzz29_add_lane(run, cur);
        sh[i].p = run; sh[NT + i].p = T0;
    }
    __syncthreads();
    // phase 2: pairs.  Pair t owns entries 2t and 2t + 1.
    const uint32_t t = i >> 1, r = i & 1;
    const Half29 R1 = lds_load_half29(sh + 2 * t + 1, r);
    Half29 Q = lds_load_half29(sh + 2 * t, r);
    xyzz29_add_pair(Q, R1, r);                                           // the pair's sum
    Half29 Tp = lds_load_half29(sh + NT + 2 * t, r);
    xyzz29_add_pair(Tp, lds_load_half29(sh + NT + 2 * t + 1, r), r);     // the pair's weighted sums
    __syncthreads();                                                     // (every entry has been read: the scan reuses the first RED_LANES slots)
    for (uint32_t d = 1; d < RED_LANES; d <<= 1) {                       // inclusive suffix scan of the pair sums
        lds_store_half29(sh + t, Q, r);
        __syncthreads();
        if (t + d < RED_LANES) xyzz29_add_pair(Q, lds_load_half29(sh + t + d, r), r);
        __syncthreads();
    }
    const Half29 P = Q;                                                  // pair 0: total of the chunk
    lds_store_half29(sh + t, Q, r);
    __syncthreads();
    Half29 V = t + 1 < RED_LANES ? lds_load_half29(sh + t + 1, r) : Half29::inf();     // the sum of everything above this pair
    xyzz29_add_pair(V, R1, r);                                           // suffix at entry 2t + 1
    if (t >= 1) xyzz29_add_pair(V, Q, r);                                // + suffix at entry 2t (entry 0 weighs nothing)
    __syncthreads();
    lds_store_half29(sh + t, V, r); lds_store_half29(sh + RED_LANES + t, Tp, r);
    __syncthreads();
    for (uint32_t d = RED_LANES / 2; d >= 1; d >>= 1) {                  // two trees side by side, as in the pair kernel
        if (t < d) { Half29 a = lds_load_half29(sh + t, r); xyzz29_add_pair(a, lds_load_half29(sh + t + d, r), r); lds_store_half29(sh + t, a, r); }
        else if (t >= RED_LANES / 2 && t < RED_LANES / 2 + d) {
            const uint32_t u = RED_LANES + (t - RED_LANES / 2);
            Half29 a = lds_load_half29(sh + u, r); xyzz29_add_pair(a, lds_load_half29(sh + u + d, r), r); lds_store_half29(sh + u, a, r);
        }
        __syncthreads();
    }
    if (t == 0) lds_store_half29(sh + 1, P, r);
    __syncthreads();
    // three results per chunk: the sum, sum_i T_i, sum_i i R_i.  The host adds the windows' chunks up anyway and multiplies the third by 8 (buckets
    // per thread) once per window: three doublings and an addition on ONE lane's 32-bit path here were 25 us at the end of every workgroup's chain.
    if (threadIdx.x < 3) out[3 * (size_t)blockIdx.x + threadIdx.x] = store_point29(threadIdx.x == 0 ? sh[1].p : threadIdx.x == 1 ? sh[RED_LANES].p : sh[0].p);
}


// ---- 7b'. the fold of a table launch's bucket rows on the 29-bit records: a pair of lanes per bucket adds its W rows in sequence (xyzz29_add_pair; rows
//      without entries were never written and are skipped by their length), Bucket29 in, Bucket29 out — the accumulation stores its accumulators as they
//      are and the reduction loads the folded set as it is: no conversion anywhere between the gathers and the chunk results.
__global__ __launch_bounds__(256) void k_bucket_fold29(const Bucket29 *buckets, const uint32_t *counts, uint32_t W, uint32_t B, Bucket29 *out, int critical) {
    crit_wave_priority(critical);
    const uint32_t b = (blockIdx.x * blockDim.x + threadIdx.x) >> 1, r = threadIdx.x & 1;
    if (b >= B) return;                                                         // (B is even: pairs stay whole)
    Half29 acc = Half29::inf();
    uint32_t w = 0;
    while (w < W && !counts[(size_t)w * B + b]) ++w;
    Half29 cur = w < W ? load_half29<true>(buckets + (size_t)w * B, b, B, r) : Half29::inf();
    while (w < W) {
        uint32_t nw = w + 1;
        while (nw < W && !counts[(size_t)nw * B + b]) ++nw;
        const Half29 nxt = nw < W ? load_half29<true>(buckets + (size_t)nw * B, b, B, r) : Half29::inf();   // the next row arrives under the addition
        xyzz29_add_pair(acc, cur, r);
        cur = nxt; w = nw;
    }
    uint32_t *o = reinterpret_cast<uint32_t *>(out + b) + 9 * r;
#pragma unroll
    for (int i = 0; i < 9; ++i) { o[i] = acc.c0.v[i]; o[18 + i] = acc.c1.v[i]; }
}

// ---- 7b. per-window tables: all W windows weigh the same, so their bucket sets are summed bucket-wise before the one reduction.
//      A workgroup takes FOLD_B buckets: its 256 threads load one accumulator each (window-major, so a wavefront reads FOLD_B
//      consecutive buckets of one window), then an LDS tree over the windows — ceil(log2 W) levels instead of a W-long chain, the upper
//      levels shared by DPP quads.  Empty accumulators (a sparse witness) cost nothing: additions with infinity return at once.
static constexpr uint32_t FOLD_THREADS = 256;
template <class F>
__global__ __launch_bounds__(FOLD_THREADS) void k_bucket_fold(const XYZZ<F> *buckets, const uint32_t *counts, uint32_t W, uint32_t B, uint32_t fold_b_log, XYZZ<F> *out, SetLayout L) {
    extern __shared__ unsigned char red_smem[];
    LdsPoint<F> *sh = reinterpret_cast<LdsPoint<F> *>(red_smem);            // FOLD_THREADS points: [window slot][bucket]
    const uint32_t t = threadIdx.x, FB = 1u << fold_b_log, slots = FOLD_THREADS >> fold_b_log;     // window slots held at once (a power of two)
    const uint32_t bl = t & (FB - 1), slot = t >> fold_b_log, b = blockIdx.x * FB + bl;
    buckets += blockIdx.y * L.buckets; out += blockIdx.y * L.folded;
    XYZZ<F> acc = XYZZ<F>::inf();
    // buckets without entries were never written (the accumulation is launched over the non-empty ones only): their length says so
    if (b < B) for (uint32_t w = slot; w < W; w += slots) if (counts[(size_t)w * B + b]) acc.add(buckets[(size_t)w * B + b]);   // W <= slots for the shipped window sizes: no addition
    sh[t] = acc;
    __syncthreads();
    for (uint32_t d = slots / 2; d >= 1; d >>= 1) {                    // tree over the window slots; pairs (slot, slot + d) of the same bucket
        const uint32_t pairs = d << fold_b_log;
        if (4 * pairs <= FOLD_THREADS) {
            const uint32_t u = t >> 2, q = t & 3;
            if (u < pairs) { XYZZ<F> a = sh[u]; xyzz_add_quad(a, sh[u + pairs].p, q); if (q == 0) sh[u] = a; }
        } else if (t < pairs) { XYZZ<F> a = sh[t]; a.add(sh[t + pairs]); sh[t] = a; }
        __syncthreads();
    }
    if (t < FB && b < B) out[b] = sh[t].normalized();
}

// 1 / x for the in-lane batched normalisations below.  Fq: through the 29-bit safegcd (f29::inverse: ~70 products' worth against the ~380 of the
// Fermat chain behind Fq::inverse(); two conversions); Fq2: the same on its norm.
template <class F> ZK_D F inverse_fast(const F &x) {
    if constexpr (std::is_same<F, Fq>::value) return f29::from29(f29::inverse(f29::to29(x.normalized())));
    else { const Fq d = inverse_fast<Fq>(x.c0.sqr() + x.c1.sqr()); return F{x.c0 * d, (x.c1 * d).neg()}; }      // (c0 - c1 u) / (c0^2 + c1^2), as Fq2::inverse()
}
// levels j+1 .. j+K of a window table from level j: level j+l = 2^(c l) * level j.  One lane walks a point through its K x c doublings in
// XYZZ and normalises the K results with ONE inversion (Montgomery's trick over their ZZZ): a level per launch spent 80 % of its
// time in the 380-product Fermat inversion of each point.  out points at level j+1; levels are n entries apart.
template <class F, int K>
__global__ __launch_bounds__(256) void k_table_levels(const Affine<F> *in, Affine<F> *out, size_t n, uint32_t c, int levels) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> a = in[i];
    if (a.is_inf()) { for (int l = 0; l < levels; ++l) out[(size_t)l * n + i] = a; return; }
    F x[K], y[K], zz[K], zzz[K];
    XYZZ<F> p = XYZZ<F>::dbl_affine_inl(a);
#pragma unroll
    for (int l = 0; l < K; ++l) {
        if (l < levels) {
            for (uint32_t k = (l == 0 ? 1u : 0u); k < c; ++k) p = p.dbl();
            x[l] = p.x; y[l] = p.y; zz[l] = p.zz; zzz[l] = p.zzz;
        } else { x[l] = F::zero(); y[l] = F::zero(); zz[l] = F::zero(); zzz[l] = F::zero(); }
    }
    // (a point of a prime-order group never doubles to infinity; a hostile key's small-order G2 point can: ZZZ = 0 is skipped and restored)
    F pre[K], run = F::one();
#pragma unroll
    for (int l = 0; l < K; ++l) { pre[l] = run; if (!zzz[l].is_zero()) run = run * zzz[l]; }
    F inv = inverse_fast(run);
#pragma unroll
    for (int l = K - 1; l >= 0; --l) {
        if (l >= levels) continue;
        if (zzz[l].is_zero()) { out[(size_t)l * n + i] = Affine<F>::inf(); continue; }
        F zi = inv * pre[l];                                                    // 1 / ZZZ_l
        inv = inv * zzz[l];
        F t = zi * zz[l];                                                       // ZZ / ZZZ = 1 / Z
        F zi2 = t.sqr();                                                        // 1 / ZZ
        out[(size_t)l * n + i] = Affine<F>{x[l] * zi2, y[l] * zi}.normalized();
    }
}

// ---- witness split (libff multi_exp_with_mixed_addition, reached from snark.cpp:126 for the A / B / L queries): a scalar that is 0 is
//      skipped, a scalar that is 1 adds its base directly, anything else is left to the bucket method.  k_classify tags every element
//      of z = [1 | w] (0 zero, 1 one, 2 other) and lists the indices of the others; k_ones_sum adds the bases tagged 1 (a flat sum: lanes
//      stride over the tags, LDS tree per workgroup, k_sum_partials finishes); the listed ones go through the digit sort as a gathered
//      subset.  Both parts are exact group sums, so their total is the same point the reference's loop produces.
__global__ __launch_bounds__(256) void k_classify(const Fr *z, size_t n1, uint8_t *tags, uint32_t *listed, uint32_t *count, const uint32_t *subset_pos) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t tag = 0;
    if (i < n1) {
        Fr v = z[i];
        uint32_t any = 0, diff = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { any |= v.v[j]; diff |= v.v[j] ^ FrParams::ONE[j]; }
        tag = any == 0 ? 0u : (diff == 0 ? 1u : 2u);
        tags[i] = (uint8_t)tag;
    }
    const unsigned long long mask = __ballot(tag == 2);
    if (!mask) return;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == (uint32_t)(__ffsll((long long)mask) - 1)) base = atomicAdd(count, (uint32_t)__popcll(mask));
    base = __shfl(base, __ffsll((long long)mask) - 1, 64);
    if (tag == 2) {
        listed[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = (uint32_t)i;
        if (subset_pos && subset_pos[i] == SUBSET_NONE) count[1] = 1;        // the witness tables do not cover this element (yet)
    }
}
template <class F>
__global__ __launch_bounds__(256) void k_gather_points(const Affine<F> *src, const uint32_t *idx, size_t count, uint32_t index_sub, Affine<F> *out) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const uint32_t i = idx[j];
    out[j] = i >= index_sub ? src[i - index_sub] : Affine<F>::inf();
}
template <class F>
__global__ __launch_bounds__(256) void k_scatter_points(const Affine<F> *src, const uint32_t *idx, size_t count, Affine<F> *out) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < count) out[idx[j]] = src[j];
}
// A workgroup owns `span` consecutive tags.  Its four wavefronts first list the positions tagged 1 in LDS (ballot + prefix count, a segment
// per wavefront: the order is the index order, nothing depends on timing), then all 256 lanes stride over the list — every lane of every
// addition is a real one.  (Round 2 strode over the tags themselves: with half the witness bits zero half of each wavefront's additions were
// masked off, the kernel's time was twice its work.)
template <class F>
__global__ __launch_bounds__(256) void k_ones_sum(const ViewSet<F> views, const uint8_t *tags, size_t n1, uint32_t span, XYZZ<F> *partials,
                                                   size_t tag_stride, size_t vec_stride /* blockIdx.z = witness of a batch (ones_sum_launch_multi): its tags and its partials */) {
    extern __shared__ unsigned char red_smem[];
    LdsPoint<F> *sh = reinterpret_cast<LdsPoint<F> *>(red_smem);            // 256 points
    uint32_t *list = reinterpret_cast<uint32_t *>(red_smem + 256 * sizeof(LdsPoint<F>));        // span positions, span / 4 per wavefront
    __shared__ uint32_t seg_count[4];
    const Affine<F> *bases = views.v[blockIdx.y].p; const uint32_t index_sub = views.v[blockIdx.y].index_sub;
    tags += (size_t)blockIdx.z * tag_stride;
    partials += (size_t)blockIdx.z * vec_stride + (size_t)blockIdx.y * (gridDim.x + 1);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cap = span >> 2;
    const size_t first = (size_t)blockIdx.x * span + (size_t)wv * cap;
    uint32_t count = 0;                                                       // uniform across the wavefront
    for (uint32_t o = 0; o < cap; o += 64) {
        const size_t i = first + o + lane;
        const bool one = i < n1 && i >= index_sub && tags[i] == 1;
        const unsigned long long mask = __ballot(one);
        if (one) list[wv * cap + count + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = (uint32_t)(i - index_sub);
        count += (uint32_t)__popcll(mask);
    }
    if (lane == 0) seg_count[wv] = count;
    __syncthreads();
    const uint32_t c0 = seg_count[0], c1 = c0 + seg_count[1], c2 = c1 + seg_count[2], total = c2 + seg_count[3];
    XYZZ<F> acc = XYZZ<F>::inf();
    for (uint32_t k = tid; k < total; k += 256) {
        const uint32_t seg = (k >= c0) + (k >= c1) + (k >= c2), off = seg == 0 ? 0u : (seg == 1 ? c0 : (seg == 2 ? c1 : c2));
        acc.madd(bases[list[seg * cap + (k - off)]]);
    }
    sh[tid] = acc;
    __syncthreads();
    lds_tree_reduce<F>(sh, 256, tid, 256, [] { __syncthreads(); });
    if (tid == 0) partials[blockIdx.x] = sh[0].normalized();
}
template <class F>
__global__ __launch_bounds__(256) void k_sum_partials(XYZZ<F> *partials_all, uint32_t count, size_t vec_stride) {        // per set (and witness, blockIdx.y): partials[0..count) -> partials[count]
    extern __shared__ unsigned char red_smem[];
    LdsPoint<F> *sh = reinterpret_cast<LdsPoint<F> *>(red_smem);
    XYZZ<F> *partials = partials_all + (size_t)blockIdx.y * vec_stride + (size_t)blockIdx.x * (count + 1), *out = partials + count;
    XYZZ<F> acc = XYZZ<F>::inf();
    for (uint32_t i = threadIdx.x; i < count; i += 256) acc.add(partials[i]);
    sh[threadIdx.x] = acc;
    __syncthreads();
    lds_tree_reduce<F>(sh, 256, threadIdx.x, 256, [] { __syncthreads(); });
    if (threadIdx.x == 0) out[0] = sh[0].normalized();
}

// ---- jobs: one MSM (or several base sets over one scalar vector) in flight on one stream ---------------------
struct MsmGroup {                   // the base sets of one field in a launch: accumulators and the host landing zone of their chunk results
    DevBuf buckets, folded, red_out, heavy_items, heavy_buckets, heavy_partials;
    DevBuf bases29;                                    // a plain G1 set's bases as 64-byte packed 29-bit records (Rec64, k_bases_to29), rebuilt per launch
    void *host_red = nullptr; size_t host_cap = 0; bool g2 = false, table = false; int nsets = 0;
    int out_index[MSM_MAX_SETS] = {0};                 // position of each set among the launch's sets of this field
    int red_slots = 2; size_t red_stride = 0;                                // results per chunk (k_bucket_reduce29l: 3, see there), elements per set in red_out
    uint32_t cpw = 0, red_windows = 0; size_t nred = 0; int chunk_log = 0;   // reduce geometry per set: chunks per window, windows reduced, chunk results, log2(buckets per chunk)
    int host_reserve(size_t bytes) {
        if (bytes <= host_cap) return 0;
        if (host_red) (void)hipHostFree(host_red);
        host_red = nullptr; host_cap = 0;
        if (!hip_ok(hipHostMalloc(&host_red, bytes + 4096, hipHostMallocDefault), "hipHostMalloc", __FILE__, __LINE__)) return 1;
        host_cap = bytes + 4096;
        return 0;
    }
    void release() {
        for (DevBuf *b : {&buckets, &folded, &red_out, &heavy_items, &heavy_buckets, &heavy_partials, &bases29}) b->release();
        if (host_red) (void)hipHostFree(host_red);
        host_red = nullptr; host_cap = 0;
    }
};
// What a digit sort writes and the accumulation behind it reads: the sorted entry list with its bucket offsets and order, the sort's scratch, and
// the heavy-list counters of the launch's two fields — the sort's first kernel clears them (ZeroList), so they go with the sort's buffers: a sort
// that runs beside the accumulation of the launch before it (msm_g1_host_scalars) must not clear the counters that one is filling.
struct MsmSortSpace {
    DevBuf digits, hist, counts, offsets, scan_sums, class_hist, order, lane_recs, sorted, rx_tmp, rx_meta, heavy_counters[2];
    bool has_lane_recs = false;        // the sort enqueued last wrote lane_recs (a lone G1 set: what k_bucket_accum29 can follow)
    void release() { for (DevBuf *b : {&digits, &hist, &counts, &offsets, &scan_sums, &class_hist, &order, &lane_recs, &sorted, &rx_tmp, &rx_meta, &heavy_counters[0], &heavy_counters[1]}) b->release(); }
};
// What belongs to ONE launch and not to the job: passed by value through both halves of a launch, nothing of it is kept on the job.
struct MsmLaunchMode {
    hipStream_t sort_stream = nullptr; // the digit sort's stream (high priority: its small kernels get the compute units an accumulation frees first); null: the job's own
    uint32_t *heavy_out = nullptr;     // where the sort's k_order_place stores its heavy-bucket count (pinned host memory); null: nowhere
    int window = 0;                    // > 0: this launch's window size, whatever the job's hint (the pieces of one multi-exponentiation share the whole job's)
    bool resume = false;               // the accumulation continues the buckets of the launch before it
    bool defer_reduce = false;         // more pieces follow: no reduction, nothing copied back
    bool heavy_pair = true;            // false: the caller has read the sort's heavy-bucket count (heavy_out) and found zero
    bool beside = false;               // something is meant to run beside the accumulation (the next piece's sort): two wavefronts per SIMD, see launch_accumulate
    bool timed = false;                // the launch feeds the kernel timer (the synchronous entry points' job)
    uint32_t *stream_waits = nullptr;  // counts the cross-stream waits the launch puts on job->stream (zkg_msm_host_scalars_stats); null: not counted
};
struct MsmJob {
    hipStream_t stream = nullptr; bool own_stream = false;
    MsmSortSpace space;
    MsmGroup group[2];                 // [0] the G1 sets, [1] the G2 sets of the launch
    MsmGeom g{}; size_t n = 0;         // of the launch whose sort was enqueued last (what msm_job_finish combines)
    int window_hint = 0;               // 0: pick_geom's rule
    // Table launches: every window's digit weighs the same, so f consecutive windows can share one row of buckets — a row is then a window
    // over the f n entries (level, point) of its levels, which lie back to back in the table.  Same sorted list (rows of the digit array
    // are simply read in pairs), W / f x B accumulators instead of W x B: the fold's additions shrink with it and chains get f times longer.
    uint32_t merge_hint = 1, merge = 1;
    // a plain G1 set's conversion to 29-bit records (k_bases_to29) runs on a stream of its own beside the digit sort, whose small launches
    // leave most of the chip idle: fork after everything queued before (the previous launch's accumulation still reads the records), join before the accumulation
    hipStream_t aux = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr; bool converted_aside = false;
    bool one_pass_sort = false;        // the caller knows the digits are skewed (a prover's 0/1 witness): skip the two-pass sort's attempt
    bool critical = false;                        // msm_job_set_critical: the accumulate / fold / reduce kernels raise their wavefronts' issue priority
    uint32_t w0 = 0, ws = 1;           // window subset of the next launches (window-sharded multi-GPU runs)
    bool empty = false;
    bool dev_finish = false;           // msm_job_set_device_finish: the next launches end in msm_job_finish_dev — their chunk records stay on the device
    // msm_job_launch_multi: `multi` scalar vectors, multi_stride words apart, over one table; the geometry then has W * multi rows (k_digits_multi)
    uint32_t multi = 1; size_t multi_stride = 0;
    std::mutex mu;
    // the side stream and its two events, all three or none
    int ensure_side() {
        if (aux) return ZKG_OK;
        if (hipStreamCreateWithFlags(&aux, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) == hipSuccess) return ZKG_OK;
        release_side(); set_error("msm: side stream"); return ZKG_ERROR;
    }
    void release_side() {
        if (aux) { (void)hipStreamSynchronize(aux); (void)hipStreamDestroy(aux); }
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        aux = nullptr; ev_fork = ev_join = nullptr;
    }
    // everything the job holds on the device but its own stream; the job can be used again afterwards (a later zkg_init may pick another device)
    void release_device() {
        space.release();
        for (MsmGroup &gr : group) gr.release();
        release_side();
    }
};
// What msm_job_enqueue_sort leaves for msm_job_enqueue_accumulate: the launch's base sets by field (level strides in merged rows), the geometry
// as the sorted list has it, and the workspace the sort wrote.
struct MsmLaunchSets { MsmBases by_field[2][MSM_MAX_SETS]; MsmGeom g{}; size_t n = 0; bool empty = false; MsmSortSpace *space = nullptr; };

template <class F>
static int launch_accumulate(MsmJob *job, MsmGroup &gr, const MsmLaunchSets &ls, const uint32_t *d_gather, const MsmLaunchMode &mode, bool time_it) {
    const MsmSortSpace &sp = *ls.space; const MsmBases *sets = ls.by_field[gr.g2 ? 1 : 0];
    const MsmGeom g = ls.g; const size_t n = ls.n, total_buckets = (size_t)g.W * g.B; const unsigned ns = (unsigned)gr.nsets;
    // a multi launch (msm_job_launch_multi): P vectors' rows side by side, a window is P * B buckets wide and the fold leaves P bucket sets
    const uint32_t P = job->multi, BP = g.B * P, Wp = g.W / P;
    hipStream_t s = job->stream;
    size_t n_entries_max = n * g.W;
    // worst case of the device-side threshold: a heavy bucket holds more than 8 entries (G1; 4 for G2), so there are fewer than
    // entries / 8 (entries / 4) of them and never more than there are buckets; each is cut into ceil(len / 512) parts
    const size_t max_heavy = std::min(total_buckets, n_entries_max / (sizeof(F) != sizeof(Fq) ? 4 : 8)) + 1,
                 max_items = max_heavy + n_entries_max / HEAVY_S + 1;
    typedef RedGeom<F> RG;
    gr.table = sets[0].level_stride != 0;
    gr.red_windows = gr.table ? P : g.W;                             // a table's windows are folded into one bucket set (per vector) first
    const size_t red_buckets = (size_t)gr.red_windows * g.B;
    static const char *force_l = getenv("ZKG_RED_L_LOG");                                                  // tuning aid: 0, 2 or 4
    const int red_l_log = force_l ? atoi(force_l) : red_buckets >= RED_LARGE_BUCKETS ? RED_L_LOG_LARGE : red_buckets > RED_SMALL_BUCKETS ? RED_L_LOG_SMALL : RED_L_LOG_TINY;
    gr.chunk_log = RG::LANES_LOG + red_l_log;
    gr.cpw = (g.B + (1u << gr.chunk_log) - 1) >> gr.chunk_log; gr.nred = (size_t)gr.red_windows * gr.cpw;
    gr.red_slots = 2;
    SetLayout L; L.buckets = total_buckets; L.items = max_items; L.heavy = max_heavy; L.partials = max_items; L.folded = BP; L.red_out = gr.nred * 3;      // two results per chunk, three from k_bucket_reduce29l (gr.red_slots)
    if (gr.heavy_items.reserve(ns * max_items * sizeof(HeavyItem)) || gr.heavy_buckets.reserve(ns * max_heavy * sizeof(HeavyBucket)) ||
        gr.heavy_partials.reserve(ns * max_items * sizeof(XYZZ<F>)) ||
        gr.buckets.reserve(ns * total_buckets * std::max(sizeof(XYZZ<F>), sizeof(Bucket29))) || (job->dev_finish && gr.red_out.reserve(ns * L.red_out * sizeof(XYZZ<F>))) || ((gr.red_stride = L.red_out), false) ||
        (gr.table && gr.folded.reserve(ns * (size_t)BP * std::max(sizeof(XYZZ<F>), sizeof(Bucket29)))) || (!job->dev_finish && gr.host_reserve(ns * L.red_out * sizeof(XYZZ<F>)))) return ZKG_ERROR;
    XYZZ<F> *buckets = gr.buckets.as<XYZZ<F>>();
    uint32_t *heavy_counters = sp.heavy_counters[gr.g2 ? 1 : 0].as<uint32_t>();      // (reserved and cleared by the sort's k_digits)
    ViewSet<F> views;
    for (unsigned i = 0; i < (unsigned)MSM_MAX_SETS; ++i) {
        const MsmBases &b = sets[i < ns ? i : 0];
        views.v[i] = BaseView<F>{reinterpret_cast<const Affine<F> *>(b.p), b.level_stride, d_gather, b.index_sub, BP, b.remap};
    }
    // `order` lists the buckets by descending length, the empty ones last.  A table launch folds through the bucket lengths and never reads
    // an empty bucket, so its accumulation covers at most one lane per entry: a witness' ~10^5 entries over 2^19 buckets would otherwise
    // dispatch 8 K wavefronts that find nothing to do — on a chip they share with the H multi-exponentiation.
    const size_t lanes = gr.table ? std::min(total_buckets, n_entries_max) : total_buckets;
    bool plain = !d_gather;
    for (unsigned i = 0; i < ns; ++i) plain = plain && sets[i].level_stride == 0 && sets[i].index_sub == 0 && !sets[i].remap;
    // a plain G1 set takes the 29-bit accumulation (several sets per launch keep the 8 x 32-bit kernel)
    bool use29 = false; const Rec64 *rec29 = nullptr; size_t stride29 = 0;
    if constexpr (sizeof(F) == sizeof(Fq)) {
        if (ns == 1 && plain) {
            use29 = true;
            if (sets[0].p29) rec29 = reinterpret_cast<const Rec64 *>(sets[0].p29);       // the caller made the records (a piece of a piece-wise job)
            else {
                ZK_HIP(hipStreamWaitEvent(s, job->ev_join, 0));                          // converted beside the sort (msm_job_enqueue_sort: the same conditions)
                if (mode.stream_waits) ++*mode.stream_waits;
                rec29 = gr.bases29.as<Rec64>();
            }
        } else if (ns == 1 && !d_gather && sets[0].p29 && !sets[0].remap && sets[0].index_sub == 0) {
            use29 = true; rec29 = reinterpret_cast<const Rec64 *>(sets[0].p29); stride29 = sets[0].level_stride;      // a resident table's records
        }
    }
    // plain G1 set on the 29-bit kernels: the buckets stay 29-bit records from the accumulation to the reduction
    // ... and so do a lone table set's (the prover's H query: accumulate -> k_bucket_fold29 -> reduce, all on the records)
    // — where the rows are few (8 after the row merge of the large tables: a bucket's rows are added in sequence, 4 us each; a one-payload key's 22
    // rows of 2048 buckets keep the 32-bit fold, a tree over the rows: 0.75 against 0.83 ms per proof)
    const bool out29 = use29 && (stride29 == 0 ? !gr.table : (gr.table && ns == 1 && Wp <= 8));
    if (use29 && !sp.has_lane_recs) { set_error("msm: the sort left no lane records for the 29-bit accumulation"); return ZKG_ERROR; }
    const int resume = mode.resume ? 1 : 0;                                   // (msm_g1_host_scalars' pieces: one plain G1 set with its records, so use29 and out29 hold)
    if (time_it) g_dominant_timer.begin(s);
    if constexpr (sizeof(F) == sizeof(Fq)) {
        // wavefronts per SIMD: three (168 registers; the loop has no spill either way) when the launch has the chip to itself — a plain set sorted on
        // the job's own stream: the resident call, 1.17 -> 1.14 ms alone — and two capped at ACC29_VGPRS where something is meant to run beside it: the
        // next piece's sort of a piece-wise job, the witness multi-exponentiations of a proof (table launches)
        static const int waves_env = getenv("ZKG_ACC29_WAVES") ? atoi(getenv("ZKG_ACC29_WAVES")) : 0;               // tuning aid: 2 or 3 everywhere
        // (the last piece of a piece-wise job has no sort beside it; three wavefronts for it alone were measured: 1.837 against 1.850 ms over three
        //  alternating runs each, one of the three pairs the other way round — inside the runs' own spread, so it keeps the two)
        const int waves29 = waves_env ? waves_env : (mode.beside || gr.table) ? 2 : 3;
        auto launch29 = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3((unsigned)((lanes + ACC29_WG - 1) / ACC29_WG)), dim3(ACC29_WG), 0, s, rec29, stride29, BP, sp.sorted.as<uint32_t>(),
                               sp.lane_recs.as<LaneRec>(), lanes, (void *)buckets, gr.heavy_items.as<HeavyItem>(),
                               gr.heavy_buckets.as<HeavyBucket>(), heavy_counters, resume | (job->critical ? 2 : 0));
        };
        if (use29 && waves29 == 3) { if (out29) launch29(k_bucket_accum29<3, true>); else launch29(k_bucket_accum29<3, false>); }
        else if (use29) { if (out29) launch29(k_bucket_accum29<2, true>); else launch29(k_bucket_accum29<2, false>); }
    }
    auto launch32 = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)((lanes + 255) / 256), ns), dim3(256), 0, s, views, sp.sorted.as<uint32_t>(), sp.offsets.as<uint32_t>(), sp.order.as<uint32_t>(),
                           lanes, buckets, gr.heavy_items.as<HeavyItem>(), gr.heavy_buckets.as<HeavyBucket>(), heavy_counters, L);
    };
    if (!use29) { if (plain) launch32(k_bucket_accum<F, true>); else launch32(k_bucket_accum<F, false>); }
    if (time_it) g_dominant_timer.end(s);
    // (counters == 0 and both kernels return at once where no list is above the threshold: 10 ... 15 us of dispatches per accumulation all the same)
    if (mode.heavy_pair) {
    hipLaunchKernelGGL(k_heavy_parts<F>, dim3(HEAVY_PART_BLOCKS, ns), dim3(256), 256 * sizeof(LdsPoint<F>), s,
                       views, sp.sorted.as<uint32_t>(), gr.heavy_items.as<HeavyItem>(), heavy_counters, gr.heavy_partials.as<XYZZ<F>>(), buckets, L, (int)out29);
    hipLaunchKernelGGL(k_heavy_merge<F>, dim3(HEAVY_MERGE_BLOCKS, ns), dim3(256), 256 * sizeof(LdsPoint<F>), s,
                       gr.heavy_buckets.as<HeavyBucket>(), heavy_counters, gr.heavy_partials.as<XYZZ<F>>(), buckets, L, (int)out29, resume);
    }
    if (mode.defer_reduce) {                                                    // a piece of a larger job: its buckets wait for the next piece
        if (hipGetLastError() != hipSuccess) { set_error("msm kernel launch failed"); return ZKG_ERROR; }
        return ZKG_OK;
    }
    const XYZZ<F> *red_in = buckets; size_t in_stride = L.buckets;
    // The chunk results of a job that finishes on the host are stored where host_combine reads them: gr.host_red is the library's own pinned
    // memory, so the reduction's few records cross the bus as the kernel's stores and no copy (its packet, and the gap in front of it) follows it.
    XYZZ<F> *red_dst = job->dev_finish ? gr.red_out.as<XYZZ<F>>() : reinterpret_cast<XYZZ<F> *>(gr.host_red);
    bool folded29 = false;
    if constexpr (sizeof(F) == sizeof(Fq)) {
        if (gr.table && out29) {
            hipLaunchKernelGGL(k_bucket_fold29, dim3((2 * BP + 255) / 256), dim3(256), 0, s, reinterpret_cast<const Bucket29 *>(buckets), sp.counts.as<uint32_t>(), Wp, BP,
                               gr.folded.as<Bucket29>(), job->critical ? 1 : 0);
            red_in = gr.folded.as<XYZZ<F>>(); in_stride = L.folded; folded29 = true;
        }
    }
    if (gr.table && !folded29) {
        uint32_t slots = 1; while (slots < Wp && slots < 32) slots <<= 1;                // window slots per workgroup: W rounded up to a power of two (<= 32)
        uint32_t fold_b_log = 0; while ((FOLD_THREADS >> (fold_b_log + 1)) >= slots) ++fold_b_log;
        hipLaunchKernelGGL(k_bucket_fold<F>, dim3((BP + (1u << fold_b_log) - 1) >> fold_b_log, ns), dim3(FOLD_THREADS), FOLD_THREADS * sizeof(LdsPoint<F>), s,
                           buckets, sp.counts.as<uint32_t>(), Wp, BP, fold_b_log, gr.folded.as<XYZZ<F>>(), L);
        red_in = gr.folded.as<XYZZ<F>>(); in_stride = L.folded;
    }
    if constexpr (sizeof(F) == sizeof(Fq)) {
        const size_t lds = 2 * RG::LANES * sizeof(LdsPoint29);
        const void *rin = red_in; XYZZ<Fq> *rout = reinterpret_cast<XYZZ<Fq> *>(red_dst);
        auto launch_red = [&](auto kern, unsigned threads) { hipLaunchKernelGGL(kern, dim3((unsigned)gr.nred, ns), dim3(threads), lds, s, rin, g.B, gr.cpw, rout, in_stride, L.red_out, job->critical ? 1 : 0); };
        if (out29 && red_l_log == RED_L_LOG_LARGE) {
            gr.red_slots = 3;
            hipLaunchKernelGGL(k_bucket_reduce29l, dim3((unsigned)gr.nred, ns), dim3(2 * RG::LANES), 4 * RG::LANES * sizeof(LdsPoint29), s,
                               reinterpret_cast<const Bucket29 *>(rin), g.B, gr.cpw, rout, in_stride, L.red_out, job->critical ? 1 : 0);
        } else if (red_l_log != RED_L_LOG_TINY) {
            if (red_l_log == RED_L_LOG_LARGE) launch_red(k_bucket_reduce29p<RED_L_LOG_LARGE, false>, 2 * RG::LANES);
            else if (out29) launch_red(k_bucket_reduce29p<RED_L_LOG_SMALL, true>, 2 * RG::LANES);
            else launch_red(k_bucket_reduce29p<RED_L_LOG_SMALL, false>, 2 * RG::LANES);
        } else {
            // one bucket per logical lane (a table launch's folded set: the prover): the chain is 17 steps either way and the quad kernel's two
            // wavefronts per SIMD hide its LDS rounds a little better (90 against 94 us); the pair form is for the long chains
            if (out29) launch_red(k_bucket_reduce29<RED_L_LOG_TINY, true>, RG::THREADS);
            else launch_red(k_bucket_reduce29<RED_L_LOG_TINY, false>, RG::THREADS);
        }
    } else {
        auto launch_red = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)gr.nred, ns), dim3(RG::THREADS), 2 * RG::LANES * sizeof(LdsPoint<F>), s, red_in, g.B, gr.cpw, red_dst, in_stride, L.red_out); };
        if (red_l_log == RED_L_LOG_LARGE) launch_red(k_bucket_reduce<F, RED_L_LOG_LARGE>);
        else if (red_l_log == RED_L_LOG_SMALL) launch_red(k_bucket_reduce<F, RED_L_LOG_SMALL>);
        else launch_red(k_bucket_reduce<F, RED_L_LOG_TINY>);
    }
    if (hipGetLastError() != hipSuccess) { set_error("msm kernel launch failed"); return ZKG_ERROR; }
    return ZKG_OK;                                                              // (msm_job_finish_dev reads gr.red_out, host_combine gr.host_red)
}

// host: window value V_w = sum_b (b+1) X_b = U_w + P_w, with chunk ch contributing U_ch + (ch*RED_CHUNK) * P_ch to U_w
// and P_ch to P_w; then Horner over windows (c doublings each).  A table set arrives as ONE window of weight 1: no doublings at all.
template <class F>
static XYZZ<F> host_combine(const MsmJob *job, const MsmGroup &gr, int set, int vec = 0 /* a multi launch: which scalar vector */) {
    const MsmGeom g = job->g; const uint32_t cpw = gr.cpw, W = gr.red_windows;
    const bool multi = gr.table && job->multi > 1;                              // msm_job_launch_multi: vector `vec` is window `vec` of the reduction
    const XYZZ<F> *red = reinterpret_cast<const XYZZ<F> *>(gr.host_red) + (size_t)set * gr.red_stride;
    const size_t sl = (size_t)gr.red_slots;                                     // 2: (P, U) per chunk; 3: (P, T, A) with U = T + 8 A (k_bucket_reduce29l)
    std::vector<XYZZ<F>> V(W);
    auto window = [&](int w) {
        XYZZ<F> Usum = XYZZ<F>::inf(), suffix = XYZZ<F>::inf(), weighted = XYZZ<F>::inf(), Asum = XYZZ<F>::inf();
        for (int ch = (int)cpw - 1; ch >= 0; --ch) {
            const XYZZ<F> &P = red[sl * ((size_t)w * cpw + ch)], &U = red[sl * ((size_t)w * cpw + ch) + 1];
            Usum.add(U);
            if (sl == 3) Asum.add(red[sl * ((size_t)w * cpw + ch) + 2]);
            if (ch >= 1) { suffix.add(P); weighted.add(suffix); }           // sum_ch ch * P_ch
            else suffix.add(P);                                             // suffix == P_w now
        }
        if (sl == 3 && !Asum.is_inf()) Usum.add(xyzz_times_pow2(Asum, 3));
        weighted = xyzz_times_pow2(weighted, (uint32_t)gr.chunk_log);                                     // * buckets per chunk (runs of doublings: host/horner_jac.hpp)
        Usum.add(weighted); Usum.add(suffix);
        V[w] = Usum;
    };
    if (multi) { window(vec); return V[vec]; }                                  // its folded bucket set: one window of weight 1
    if (gr.table) {                                                             // one window of weight 1; its chunks in segments on the host pool
        const int SEG = 16, nseg = ((int)cpw + SEG - 1) / SEG;
        if (nseg <= 1) { window(0); return V[0]; }
        // segment s = chunks [16 s, 16 s + 16): Usum_s = sum U, Psum_s = sum P, Wt_s = sum (ch - 16 s) P_ch; then
        // sum_ch ch P_ch = sum_s Wt_s + 16 * sum_s s Psum_s
        std::vector<XYZZ<F>> Us(nseg), Ps(nseg), Wt(nseg);
        host_parallel_for(nseg, [&](int sg) {
            XYZZ<F> Usum = XYZZ<F>::inf(), suffix = XYZZ<F>::inf(), weighted = XYZZ<F>::inf();
            const int lo = sg * SEG, hi = std::min<int>((int)cpw, lo + SEG);
            for (int ch = hi - 1; ch >= lo; --ch) {
                Usum.add(red[2 * (size_t)ch + 1]);
                suffix.add(red[2 * (size_t)ch]);
                if (ch > lo) weighted.add(suffix);
            }
            Us[sg] = Usum; Ps[sg] = suffix; Wt[sg] = weighted;
        });
        XYZZ<F> Usum = XYZZ<F>::inf(), suffix = XYZZ<F>::inf(), seg_weighted = XYZZ<F>::inf(), weighted = XYZZ<F>::inf();
        for (int sg = nseg - 1; sg >= 0; --sg) { Usum.add(Us[sg]); weighted.add(Wt[sg]); suffix.add(Ps[sg]); if (sg >= 1) seg_weighted.add(suffix); }
        weighted.add(xyzz_times_pow2(seg_weighted, 4));                                                   // * 16 chunks per segment
        weighted = xyzz_times_pow2(weighted, (uint32_t)gr.chunk_log);                                     // * buckets per chunk
        Usum.add(weighted); Usum.add(suffix);
        return Usum;
    }
    host_parallel_for((int)W, window);                                          // the windows are independent
    // sum_j 2^(c (w0 + j ws)) V_j: Horner with c*ws doublings per owned window, then the shift of the lowest one
    XYZZ<F> acc = XYZZ<F>::inf();
    for (int w = (int)W - 1; w >= 0; --w) {
        acc = xyzz_times_pow2(acc, g.c * g.ws);
        acc.add(V[w]);
    }
    return xyzz_times_pow2(acc, g.c * g.w0);
}

// ---- 8'. the same epilogue on the device for a TABLE launch of G1 sets, or of G2 sets (msm_job_finish_dev): host_combine's window(w), no Horner.
//      One workgroup per output point (blockIdx.x = the window of the reduction, i.e. the scalar vector of a multi launch; blockIdx.y = set).
//      A chunk's record is (P, U) — V = sum U_ch + 2^chunk_log sum ch P_ch + sum P_ch — or, from k_bucket_reduce29l (G1 only), (P, T, A) with
//      U = T + 8 A: `slots` says which.
//      Lanes own chunks: n = the power of two that covers cpw (THREADS at the most) lanes take 2^l consecutive chunks each and sum them as
//      host_combine's walk does (S = sum P, T0 = sum (ch - first) P, U, A).  sum_ch ch P_ch = 2^l sum_{t >= 1} Q_t + sum_t T0_t with Q the
//      inclusive suffix scan of S over the lanes (Hillis-Steele through LDS, as k_bucket_reduce's), so every lane weighs its own term —
//      2^chunk_log (2^l Q_t + T0_t), chunk_log + l doublings side by side — adds it to its U, lane 0 adds Q_0 = sum P, and ONE tree
//      (lds_tree_reduce) sums the lanes.  Chain: log2 n + 3 additions, chunk_log + l doublings, log2 n tree levels, one inversion.  Lane 0 stores
//      the point as store_norm does: X | Y | one, or (0, one, 0) for infinity.
//      G1 runs 256 lanes: one chunk per lane in every geometry a table produces (cpw <= 256).  G2 runs 128: an LdsPoint<Fq2> is 272 B, so 128
//      of them are 34 KiB — inside the 64 KiB a kernel gets without asking, where 256 lanes would need 68 KiB and a raised limit — and two
//      wavefronts leave each the whole register file; a lane takes 2^l consecutive chunks from cpw = 129 on (a lone vector at 16-bit windows
//      reduces to 512 chunks: l = 2).
//      A G2 point is 64 registers, so the live set is kept at three points plus one addition's temporaries: S is scanned in place (it IS Q), the
//      A term is finished (8 A added to U) straight behind the chunk loop and is dead before the scan, lane 0 adds Q_0 = sum P to its U BEFORE
//      the doublings and drops it, Q then becomes the weighted term itself (2^l Q, + T0 — T0 dies here — then chunk_log doublings) and is added
//      to U.  Sums in a group commute and the point leaves normalised, so the order changes no bit of it.
template <class F> constexpr int COMBINE_THREADS = 256;
template <> constexpr int COMBINE_THREADS<Fq2> = 128;
template <class F> constexpr int COMBINE_MAX_SLOTS = 3;                        // (P, T, A) records are k_bucket_reduce29l's: G1 only
template <> constexpr int COMBINE_MAX_SLOTS<Fq2> = 2;
template <class F> constexpr int POINT_WORDS = 3 * sizeof(F) / 4;              // a normalised point in the ABI's form: 24 words (G1), 48 (G2)
template <class F> static __host__ __device__ uint32_t combine_lanes(uint32_t cpw) { uint32_t n = 1; while (n < cpw && n < (uint32_t)COMBINE_THREADS<F>) n <<= 1; return n; }
template <class F> static size_t combine_lds_bytes(uint32_t cpw) { return combine_lanes<F>(cpw) * sizeof(LdsPoint<F>); }
// the limbs of a field element as the ABI lays them out: 8 words, c0 | c1 for Fq2
ZK_D void store_limbs(uint32_t *out, const Fq &a) { for (int i = 0; i < 8; ++i) out[i] = a.v[i]; }
ZK_D void store_limbs(uint32_t *out, const Fq2 &a) { store_limbs(out, a.c0); store_limbs(out + 8, a.c1); }
ZK_D void load_limbs(Fq &a, const uint32_t *in) { for (int i = 0; i < 8; ++i) a.v[i] = in[i]; }
ZK_D void load_limbs(Fq2 &a, const uint32_t *in) { load_limbs(a.c0, in); load_limbs(a.c1, in + 8); }
template <class F> ZK_D void store_norm_dev(uint32_t *out /* POINT_WORDS<F> */, const XYZZ<F> &v) {
    F X = F::zero(), Y = F::one(), Z = F::zero();
    if (!v.is_inf()) { const Affine<F> a = v.to_affine().normalized(); X = a.x; Y = a.y; Z = F::one(); }
    store_limbs(out, X); store_limbs(out + sizeof(F) / 4, Y); store_limbs(out + 2 * (sizeof(F) / 4), Z);
}
template <class F, int THREADS>
__global__ __launch_bounds__(THREADS) void k_msm_combine(const XYZZ<F> *red, uint32_t cpw, int slots, int chunk_log, size_t set_stride, uint32_t *out) {
    extern __shared__ unsigned char red_smem[];
    LdsPoint<F> *sh = reinterpret_cast<LdsPoint<F> *>(red_smem);              // n points
    const uint32_t t = threadIdx.x, w = blockIdx.x, set = blockIdx.y;
    const uint32_t n = combine_lanes<F>(cpw);
    int l_log = 0; while (((uint64_t)n << l_log) < cpw) ++l_log;
    const XYZZ<F> *rec = red + (size_t)set * set_stride + (size_t)slots * w * cpw;
    const uint64_t first = (uint64_t)t << l_log, end = first + ((uint64_t)1 << l_log) < cpw ? first + ((uint64_t)1 << l_log) : cpw;
    XYZZ<F> U = XYZZ<F>::inf(), Q = XYZZ<F>::inf(), T0 = XYZZ<F>::inf();
    {
        const bool has_a = COMBINE_MAX_SLOTS<F> == 3 && slots == 3;            // (no G2 reduction writes an A: that instantiation carries no code for it)
        XYZZ<F> A = XYZZ<F>::inf();
        for (uint64_t ch = end; ch > first; --ch) {                          // chunks end - 1 ... first (none for a lane behind the last chunk); Q = S here
            const XYZZ<F> *r = rec + (size_t)slots * (ch - 1);
            Q.add(r[0]); U.add(r[1]);
            if (has_a) A.add(r[2]);
            if (ch - 1 > first) T0.add(Q);
        }
        if (has_a) { for (int i = 0; i < 3; ++i) A = A.dbl(); U.add(A); }      // U = T + 8 A (k_bucket_reduce29l)
    }
    for (uint32_t d = 1; d < n; d <<= 1) {                                   // inclusive suffix scan of S over the lanes, in place
        if (t < n) sh[t] = Q;
        __syncthreads();
        if (t + d < n) Q.add(sh[t + d]);
        __syncthreads();
    }
    if (t == 0) { U.add(Q); Q = XYZZ<F>::inf(); }                            // Q_0 = sum_ch P_ch; lane 0 has no weighted term of the scan
    for (int i = 0; i < l_log; ++i) Q = Q.dbl();
    Q.add(T0);
    for (int i = 0; i < chunk_log; ++i) Q = Q.dbl();                         // * buckets per chunk (dbl() returns infinity as it is: lanes whose term is infinity idle through the loop, where host_combine skips it)
    U.add(Q);
    if (t < n) sh[t] = U;
    __syncthreads();
    lds_tree_reduce<F>(sh, n, t, THREADS, [] { __syncthreads(); });
    if (t == 0) store_norm_dev<F>(out + POINT_WORDS<F> * ((size_t)w * gridDim.y + set), sh[0]);
}
template <class F> static void launch_combine(dim3 grid, hipStream_t s, const XYZZ<F> *red, uint32_t cpw, int slots, int chunk_log, size_t set_stride, uint32_t *out) {
    hipLaunchKernelGGL((k_msm_combine<F, COMBINE_THREADS<F>>), grid, dim3(COMBINE_THREADS<F>), combine_lds_bytes<F>(cpw), s, red, cpw, slots, chunk_log, set_stride, out);
}
// an empty job's points (no window owned): the infinity encoding
template <class F> __global__ __launch_bounds__(64) void k_msm_store_inf(uint32_t *out, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) store_norm_dev(out + POINT_WORDS<F> * (size_t)i, XYZZ<F>::inf());
}
// the test hooks' records: normalised Jacobian points (X | Y | Z, Z = one or zero) -> the reduction's record form
template <class F> __global__ __launch_bounds__(256) void k_jac_to_records(const uint32_t *jac, size_t count, XYZZ<F> *rec) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t *in = jac + POINT_WORDS<F> * i;
    F X, Y, Z;
    load_limbs(X, in); load_limbs(Y, in + sizeof(F) / 4); load_limbs(Z, in + 2 * (sizeof(F) / 4));
    rec[i] = Z.is_zero() ? XYZZ<F>::inf() : XYZZ<F>{X, Y, F::one(), F::one()};
}

// the digit sort of one launch into ls.space, on mode.sort_stream (the job's own stream when that is null); leaves the sorted list's geometry in ls
static int sort_digits(MsmJob *job, MsmLaunchSets &ls, const uint32_t *d_scalars, bool mont, const uint32_t *d_gather, const MsmLaunchMode &mode) {
    MsmSortSpace &sp = *ls.space;
    const MsmGeom g0 = job->g; const size_t n0 = job->n;                        // as the scalars see them (k_digits)
    if (job->merge > 1) { job->g.W /= job->merge; job->g.Wt = job->g.W; job->n *= job->merge; }     // rows of the digit array read `merge` at a time from here on
    if (job->multi > 1) { job->g.W *= job->multi; job->g.Wt = job->g.W; }                           // ... and a row per (window, vector)
    const MsmGeom g = ls.g = job->g; const size_t n = ls.n = job->n;            // ... and as the sorted list and the accumulation do
    hipStream_t s = mode.sort_stream ? mode.sort_stream : job->stream;
    const size_t total = (size_t)g.W * g.B;
    uint32_t slice_len = (uint32_t)std::min<size_t>(65536, std::max<size_t>(4096, ((n + 15) / 16 + 1023) / 1024 * 1024));
    uint32_t S = (uint32_t)std::max<size_t>(1, (n + slice_len - 1) / slice_len);
    size_t nblk = (total + 1024 * SCAN_ITEMS - 1) / (1024 * SCAN_ITEMS);
    if (nblk > 1024) { set_error("msm: too many buckets for the block scan"); return ZKG_ERROR; }
    if (sp.digits.reserve(std::max<size_t>(1, n * g.W) * 4) || sp.hist.reserve((size_t)g.W * S * g.B * 4) || sp.counts.reserve(total * 4) ||
        sp.offsets.reserve((total + 1) * 4) || sp.scan_sums.reserve(1024 * 4) || sp.class_hist.reserve((CLASS_HIST_COPIES + 1) * (HEAVY_T_MAX + 2) * 4) ||
        sp.order.reserve(total * 4) || sp.sorted.reserve(std::max<size_t>(1, n * g.W) * 4)) return ZKG_ERROR;
    // a lone G1 set is what the 29-bit accumulation takes (launch_accumulate): only then does k_order_place write the lanes' records
    sp.has_lane_recs = job->group[0].nsets == 1;
    if (sp.has_lane_recs && sp.lane_recs.reserve(total * sizeof(LaneRec))) return ZKG_ERROR;
    uint32_t *digits = sp.digits.as<uint32_t>(), *hist = sp.hist.as<uint32_t>(), *counts = sp.counts.as<uint32_t>(),
             *offsets = sp.offsets.as<uint32_t>(), *sums = sp.scan_sums.as<uint32_t>(), *chist = sp.class_hist.as<uint32_t>();
    uint32_t cbits = 6;
    static const uint32_t bin_avg = getenv("ZKG_RX_AVG") ? (uint32_t)atoi(getenv("ZKG_RX_AVG")) : RX_BIN_AVG;     // tuning aid
    while (cbits < RX_MAX_CBITS && cbits + 1 < g.c - 1 && (n >> cbits) > bin_avg) ++cbits;  // bins average <= RX_BIN_AVG entries where possible, fbits >= 2
    // (below ~2^15.5 points the one-pass sort's six small launches beat the two-pass sort's eleven: a one-payload proof's H query, 2^15 - 1
    //  points, 0.657 -> 0.603 ms; equal at 2^16, the two-pass sort 5 % ahead at 2^17)
    const bool two_pass = !job->one_pass_sort && g.c >= 12 && n >= 49152 && (n >> cbits) <= RX_FINE_MAX && n <= ((size_t)1 << (31 - (g.c - 1 - cbits)));
    {
        ZeroList zl{};
        int k = 0;
        zl.p[k] = chist; zl.words[k++] = (CLASS_HIST_COPIES + 1) * (HEAVY_T_MAX + 2);     // the class histogram's copies and, behind them, k_order_place's cursors
        for (int f = 0; f < 2; ++f) if (job->group[f].nsets) {
            if (sp.heavy_counters[f].reserve(8 * MSM_MAX_SETS)) return ZKG_ERROR;
            zl.p[k] = sp.heavy_counters[f].as<uint32_t>(); zl.words[k++] = 2 * MSM_MAX_SETS;
        }
        if (two_pass) {
            const uint32_t nbins = g.W << cbits;
            if (sp.rx_meta.reserve((2 * (size_t)nbins + g.W) * 4)) return ZKG_ERROR;       // bin counts, bin cursors, window totals
            zl.p[k] = sp.rx_meta.as<uint32_t>(); zl.words[k++] = 2 * nbins + g.W;
        }
        const dim3 dg((unsigned)((n0 + 255) / 256));                                                     // n >= 1 (msm_job_launch)
        const bool four = !d_gather && (n0 & 3) == 0 && g0.w0 == 0 && g0.ws == 1 && g0.W == g0.Wt;      // every window stored, rows 16-byte aligned
        const dim3 dg4((unsigned)((n0 / 4 + 255) / 256));
        if (job->multi > 1) {
            const dim3 dgm(dg.x, job->multi);
            if (g0.c == 16) hipLaunchKernelGGL(k_digits_multi<16>, dgm, dim3(256), 0, s, d_scalars, job->multi_stride, n0, (int)mont, job->merge, digits, zl);
            else if (g0.c == 12) hipLaunchKernelGGL(k_digits_multi<12>, dgm, dim3(256), 0, s, d_scalars, job->multi_stride, n0, (int)mont, job->merge, digits, zl);
            else hipLaunchKernelGGL(k_digits_multi_any, dgm, dim3(256), 0, s, d_scalars, job->multi_stride, n0, (int)mont, g0, job->merge, digits, zl);
        }
        else if (four && g0.c == 16) hipLaunchKernelGGL(k_digits_c4<16>, dg4, dim3(256), 0, s, d_scalars, n0, (int)mont, g0, digits, zl);
        else if (four && g0.c == 12) hipLaunchKernelGGL(k_digits_c4<12>, dg4, dim3(256), 0, s, d_scalars, n0, (int)mont, g0, digits, zl);
        else if (g0.c == 16) hipLaunchKernelGGL(k_digits_c<16>, dg, dim3(256), 0, s, d_scalars, d_gather, n0, (int)mont, g0, digits, zl);
        else if (g0.c == 12) hipLaunchKernelGGL(k_digits_c<12>, dg, dim3(256), 0, s, d_scalars, d_gather, n0, (int)mont, g0, digits, zl);
        else hipLaunchKernelGGL(k_digits, dg, dim3(256), 0, s, d_scalars, d_gather, n0, (int)mont, g0, digits, zl);
    }
    if (two_pass) {
        // two-pass sort: 2^cbits coarse bins per window, then the remaining fbits inside LDS
        const uint32_t fbits = g.c - 1 - cbits, CB = 1u << cbits, nbins = g.W * CB, S1 = (uint32_t)((n + RX_SLICE - 1) / RX_SLICE);
        if (sp.rx_tmp.reserve(n * g.W * 4)) return ZKG_ERROR;
        uint32_t *cnt = sp.rx_meta.as<uint32_t>(), *cursor = cnt + nbins, *wtot = cursor + nbins, *tmp = sp.rx_tmp.as<uint32_t>();      // (zeroed by the digits kernel)
        const size_t fine_lds = (RX_FINE_MAX + 3 * (1u << fbits)) * 4;
        hipLaunchKernelGGL(k_rx_count, dim3(S1, g.W), dim3(1024), 0, s, digits, n, fbits, cbits, cnt, wtot);
        // (a sort on a stream of its own runs beside an accumulation: half-size workgroups fit into the registers that one leaves free)
        static const int wg_env = getenv("ZKG_SORT_WG") ? atoi(getenv("ZKG_SORT_WG")) : 0;                 // A/B switch: 512 / 1024 everywhere
        const bool half = (wg_env ? wg_env == 512 : mode.sort_stream != nullptr) && fbits <= 9;           // (k_rx_fine's scan: one fine bucket per thread)
        if (half) {
            const uint32_t S2 = (uint32_t)((n + 512 * RX_PER_THREAD - 1) / (512 * RX_PER_THREAD));
            hipLaunchKernelGGL(k_rx_scatter<512>, dim3(S2, g.W), dim3(512), (512 * RX_PER_THREAD + 4 * RX_MAX_CB + 8) * 4, s, digits, n, fbits, cbits, cnt, wtot, g.W, cursor, tmp, offsets + total);
            hipLaunchKernelGGL(k_rx_fine<512>, dim3(CB, g.W), dim3(512), fine_lds, s, tmp, fbits, cbits, g.B, cnt, wtot, counts, offsets, total, chist,
                               sp.sorted.as<uint32_t>());
        } else {
            hipLaunchKernelGGL(k_rx_scatter<1024>, dim3(S1, g.W), dim3(1024), (RX_SLICE + 4 * RX_MAX_CB + 8) * 4, s, digits, n, fbits, cbits, cnt, wtot, g.W, cursor, tmp, offsets + total);
            hipLaunchKernelGGL(k_rx_fine<1024>, dim3(CB, g.W), dim3(1024), fine_lds, s, tmp, fbits, cbits, g.B, cnt, wtot, counts, offsets, total, chist,
                               sp.sorted.as<uint32_t>());
        }
    } else {                                                                                    // one pass: histogram, scans, k_place
    hipLaunchKernelGGL(k_hist, dim3(S, g.W), dim3(SORT_THREADS), g.B * 4, s, digits, n, g.B, S, slice_len, hist);
    hipLaunchKernelGGL(k_colscan, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, hist, g.B, S, total, counts);
    hipLaunchKernelGGL(k_scan_blocks, dim3((unsigned)nblk), dim3(1024), 0, s, counts, offsets, sums, total);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, s, sums, (uint32_t)nblk, offsets + total);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nblk), dim3(1024), 0, s, offsets, sums, total);
    hipLaunchKernelGGL(k_place, dim3(S, g.W), dim3(SORT_THREADS), g.B * 4, s, digits, n, g.B, S, slice_len, hist, offsets, sp.sorted.as<uint32_t>());
    hipLaunchKernelGGL(k_class_hist, dim3((unsigned)((total + 1023) / 1024)), dim3(1024), 0, s, counts, offsets, total, chist);
    }
    hipLaunchKernelGGL(k_order_place, dim3((unsigned)((total + 1023) / 1024)), dim3(1024), 0, s, counts, offsets, total, chist, chist + CLASS_HIST_COPIES * (HEAVY_T_MAX + 2), sp.order.as<uint32_t>(), mode.heavy_out,
                       sp.sorted.as<uint32_t>(), sp.has_lane_recs ? sp.lane_recs.as<LaneRec>() : nullptr);
    if (hipGetLastError() != hipSuccess) { set_error("msm sort launch failed"); return ZKG_ERROR; }
    return ZKG_OK;
}

MsmJob *msm_job_create(hipStream_t s, bool own_stream, bool high_priority) {
    MsmJob *j = new MsmJob();
    j->stream = s;
    if (own_stream) {
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        if (!hip_ok(hipStreamCreateWithPriority(&j->stream, hipStreamNonBlocking, high_priority ? prio_hi : prio_lo), "hipStreamCreate", __FILE__, __LINE__)) { delete j; return nullptr; }
        j->own_stream = true;
    }
    return j;
}
void msm_job_set_window(MsmJob *j, int c) { if (j) j->window_hint = c; }
bool crit_priority_enabled() { static const bool on = !(getenv("ZKG_CRIT_PRIO") && atoi(getenv("ZKG_CRIT_PRIO")) == 0); return on; }
void msm_job_set_critical(MsmJob *j, bool critical) { if (j) j->critical = critical && crit_priority_enabled(); }
void msm_job_set_row_merge(MsmJob *j, uint32_t f) { if (j) j->merge_hint = f ? f : 1; }
void msm_job_set_skewed(MsmJob *j, bool skewed) { if (j) j->one_pass_sort = skewed; }
void msm_job_set_window_subset(MsmJob *j, uint32_t w0, uint32_t ws) { if (j) { j->w0 = w0; j->ws = ws ? ws : 1; } }
hipStream_t msm_job_stream(MsmJob *j) { return j->stream; }
void msm_job_destroy(MsmJob *j) {
    if (!j) return;
    j->release_device();
    if (j->own_stream) (void)hipStreamDestroy(j->stream);
    delete j;
}

static MsmJob g_default_job;          // the synchronous entry points share one job (serialised by its mutex); only it feeds the kernel timer
// what the last msm_g1_host_scalars did (zkg_msm_host_scalars_stats): pieces run, cross-stream waits put on the caller's stream, and per piece
// the heavy-bucket count the host read and whether the heavy pair was launched
struct HostScalarsStats { uint32_t pieces = 0, waits = 0, heavy[8] = {0}, pair[8] = {0}; };
// Everything msm_g1_host_scalars keeps between calls beside the default job (used under g_default_job's mutex): the device copy of the scalars,
// the copy stream with one event per piece and ev_caller (what the caller's stream held when the call began: the uploads wait for it), the high-priority stream the pieces' digit sorts run on, the second sort workspace — pieces
// alternate between the default job's and this one, [0] and [1] below — and per workspace ev_sorted (the sort into it has finished: the calling
// thread waits for it, then enqueues the accumulation) and ev_acc_done (the accumulation that read it has finished: the next sort into it waits
// for that on the device), eight words of pinned host memory, one per piece, for the sorts' heavy-bucket counts, and the stats record.
struct PieceStep {
    DevBuf scalars; MsmSortSpace space;
    hipStream_t copy = nullptr, sort = nullptr;
    hipEvent_t ev_piece[8] = {nullptr}, ev_sorted[2] = {nullptr}, ev_acc_done[2] = {nullptr}, ev_caller = nullptr;
    uint32_t *heavy_words = nullptr;
    HostScalarsStats stats;
    bool ready = false;                // streams, events and pinned words: all of them or none
    template <class Fn> void each_event(Fn f) { for (hipEvent_t &e : ev_piece) f(e); for (hipEvent_t &e : ev_sorted) f(e); for (hipEvent_t &e : ev_acc_done) f(e); f(ev_caller); }
    int ensure() {
        if (ready) return ZKG_OK;
        int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        // (confining the sort stream to 16 ... 128 compute units with a CU mask instead of the priority was measured: 2.11 -> 4.25 ... 2.70 ms — the sort needs the chip's width)
        bool ok = hipStreamCreateWithFlags(&copy, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithPriority(&sort, hipStreamNonBlocking, hi) == hipSuccess &&
                  hipHostMalloc(reinterpret_cast<void **>(&heavy_words), 8 * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
        // (ev_sorted / ev_acc_done without their system-scope fence — hipEventDisableSystemFence — were measured: 1.994 against 1.998 ms, nothing; an A/B on one box.
        //  Again for ev_acc_done alone once the host paced the accumulations: 1.7512 against 1.7549 ms over five alternating runs, nothing.  ev_sorted
        //  needs its fence in any case: the host reads the heavy word behind it.)
        each_event([&](hipEvent_t &e) { ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess; });
        if (!ok) { release(); set_error("msm: streams, events and pinned words of the piece-wise step"); return ZKG_ERROR; }
        ready = true;
        return ZKG_OK;
    }
    void release() {
        for (hipStream_t *s : {&sort, &copy}) if (*s) { (void)hipStreamSynchronize(*s); (void)hipStreamDestroy(*s); *s = nullptr; }
        each_event([](hipEvent_t &e) { if (e) { (void)hipEventDestroy(e); e = nullptr; } });
        if (heavy_words) { (void)hipHostFree(heavy_words); heavy_words = nullptr; }
        scalars.release(); space.release();
        ready = false;
    }
};
static PieceStep g_step;

// enqueue: one digit sort of the scalars (element d_gather[i] of d_scalars when a gather list is given), then one accumulate + reduce
// per base set
//
// A launch has two halves.  msm_job_enqueue_sort: the geometry, a plain G1 set's records on the side stream, and the digit sort into the
// workspace it is given, on mode.sort_stream.  msm_job_enqueue_accumulate: accumulate (+ reduce) per base set on job->stream.  msm_job_launch
// calls them back to back on one stream; a caller that takes them apart (msm_g1_host_scalars) orders the second behind the first itself.
// an error return after the fork must not leave the side stream reading the caller's bases (a synchronous caller may free them next)
static int msm_launch_failed(MsmJob *job) {
    if (job->converted_aside) { (void)hipStreamSynchronize(job->aux); job->converted_aside = false; }
    return ZKG_ERROR;
}
// The launch's base sets by field — ls.by_field, job->group[].nsets — and the row merge of a table launch (job->merge; ls.by_field's level strides
// are then in merged rows).  job->g is the launch's geometry as the scalars see it.
static void msm_job_split_sets(MsmJob *job, const MsmBases *sets, int nsets, size_t n, bool gathered, MsmLaunchSets &ls) {
    for (MsmGroup &gr : job->group) gr.nsets = 0;
    job->group[0].g2 = false; job->group[1].g2 = true;
    for (int i = 0; i < nsets; ++i) { MsmGroup &gr = job->group[sets[i].g2 ? 1 : 0]; ls.by_field[sets[i].g2 ? 1 : 0][gr.nsets] = sets[i]; gr.out_index[gr.nsets] = gr.nsets; ++gr.nsets; }
    bool merge = nsets > 0 && n > 0 && job->g.W > 0 && job->merge_hint > 1 && !gathered && job->g.W % job->merge_hint == 0 && (uint64_t)n * job->merge_hint < ((uint64_t)1 << 31);
    for (int i = 0; i < nsets; ++i) merge = merge && sets[i].level_stride == n && sets[i].index_sub == 0 && !sets[i].remap;      // a table's levels back to back, entry i = point i
    job->merge = merge ? job->merge_hint : 1;
    for (int k = 0; k < 2; ++k) for (int i = 0; i < job->group[k].nsets; ++i) ls.by_field[k][i].level_stride *= job->merge;
}
// A plain G1 set's 29-bit records (k_bases_to29 into group[0].bases29) on the job's side stream: forked behind everything queued on job->stream
// before (the work that made the bases; the previous launch's accumulation, which still reads the records), ev_join recorded behind it.
static int msm_job_convert_aside(MsmJob *job, const void *bases, size_t n) {
    if (job->ensure_side() || job->group[0].bases29.reserve(n * sizeof(Rec64))) return ZKG_ERROR;
    ZK_HIP(hipEventRecord(job->ev_fork, job->stream));
    ZK_HIP(hipStreamWaitEvent(job->aux, job->ev_fork, 0));
    hipLaunchKernelGGL(k_bases_to29, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, job->aux, reinterpret_cast<const Affine<Fq> *>(bases), n, job->group[0].bases29.as<Rec64>());
    ZK_HIP(hipEventRecord(job->ev_join, job->aux));
    return ZKG_OK;
}
static int msm_job_enqueue_sort(MsmJob *job, MsmSortSpace &space, const MsmBases *sets, int nsets, const uint32_t *d_scalars, size_t n, bool scalars_mont, const uint32_t *d_gather,
                                const MsmLaunchMode &mode, MsmLaunchSets &ls) {
    if (n >= ((size_t)1 << 31) || nsets < 0 || nsets > MSM_MAX_SETS) { set_error("msm: bad size"); return ZKG_ERROR; }
    const int window = mode.window > 0 ? mode.window : job->window_hint;
    bool any_table = false;
    for (int i = 0; i < nsets; ++i) any_table = any_table || sets[i].level_stride != 0;
    for (int i = 0; i < nsets; ++i) if ((sets[i].level_stride != 0) != any_table) { set_error("msm: table and plain base sets cannot share a launch"); return ZKG_ERROR; }
    if (any_table && (job->w0 != 0 || job->ws != 1 || window <= 0)) { set_error("msm: a table launch covers all windows at the table's window size"); return ZKG_ERROR; }
    job->g = pick_geom(n, window, job->w0, job->ws); job->n = n;
    job->empty = false; job->multi = 1;
    ls.space = &space; ls.empty = false;
    msm_job_split_sets(job, sets, nsets, n, d_gather != nullptr, ls);
    if (job->g.W == 0 || n == 0) { job->empty = ls.empty = true; return ZKG_OK; }        // no point, or this rank owns no window: the identity
    if ((uint64_t)n * job->g.W >= ((uint64_t)1 << 32)) { set_error("msm: n * windows exceeds the 32-bit index space of the sorted list (n < 2^28)"); return ZKG_ERROR; }
    job->converted_aside = false;
    const MsmBases &g1 = ls.by_field[0][0];
    if (!any_table && !d_gather && job->group[0].nsets == 1 && g1.index_sub == 0 && !g1.remap && !g1.p29) {
        if (msm_job_convert_aside(job, g1.p, n)) return ZKG_ERROR;
        job->converted_aside = true;
    }
    if (sort_digits(job, ls, d_scalars, scalars_mont, d_gather, mode)) return msm_launch_failed(job);
    return ZKG_OK;
}
static int msm_job_enqueue_accumulate(MsmJob *job, const MsmLaunchSets &ls, const uint32_t *d_gather, const MsmLaunchMode &mode) {
    if (ls.empty) return ZKG_OK;
    const bool timed_field_g2 = job->group[0].nsets == 0;                       // the kernel timer follows the first G1 launch (G2 when there is no G1 set)
    if (job->group[1].nsets && launch_accumulate<Fq2>(job, job->group[1], ls, d_gather, mode, mode.timed && timed_field_g2)) return msm_launch_failed(job);   // G2 first: the longer chains
    if (job->group[0].nsets && launch_accumulate<Fq>(job, job->group[0], ls, d_gather, mode, mode.timed)) return msm_launch_failed(job);
    return ZKG_OK;
}
static int msm_job_launch_as(MsmJob *job, const MsmBases *sets, int nsets, const uint32_t *d_scalars, size_t n, bool scalars_mont, const uint32_t *d_gather, const MsmLaunchMode &mode) {
    static const bool dbg = getenv("ZKG_DEBUG_TIMING") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *w) { if (dbg) fprintf(stderr, "[zkg]     %-18s %8.3f ms\n", w, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count()); };
    MsmLaunchSets ls;
    if (msm_job_enqueue_sort(job, job->space, sets, nsets, d_scalars, n, scalars_mont, d_gather, mode, ls)) return ZKG_ERROR;
    lap("sort enqueued");
    if (msm_job_enqueue_accumulate(job, ls, d_gather, mode)) return ZKG_ERROR;
    lap("accum enqueued");
    return ZKG_OK;
}
// the default mode: everything on the job's stream and in its own workspace, the chip to itself; the synchronous entry points' job feeds the kernel timer
int msm_job_launch(MsmJob *job, const MsmBases *sets, int nsets, const uint32_t *d_scalars, size_t n, bool scalars_mont, const uint32_t *d_gather) {
    MsmLaunchMode mode; mode.timed = job == &g_default_job;
    return msm_job_launch_as(job, sets, nsets, d_scalars, n, scalars_mont, d_gather, mode);
}
// The dual of a launch over several base sets: `count` scalar vectors of n elements, scalar_stride words apart, over the SAME table sets (all
// windows, no gather / remap / index_sub).  One digit sort, one accumulation, one fold and one reduction per field for all of them; the fold
// leaves a bucket set per (set, vector) and the reduction treats a set's as `count` windows (see k_digits_multi).
bool msm_multi_supported(size_t n, int c, uint32_t count) {
    const MsmGeom g = pick_geom(n, c);
    return c > 0 && count >= 1 && n >= 1 && (uint64_t)n * g.W * count < ((uint64_t)1 << 31) &&
           ((uint64_t)g.W * g.B * count + 1024 * SCAN_ITEMS - 1) / (1024 * SCAN_ITEMS) <= 1024;
}
int msm_job_launch_multi(MsmJob *job, const MsmBases *sets, int nsets, const uint32_t *d_scalars, size_t n, size_t scalar_stride, uint32_t count, bool scalars_mont) {
    bool ok = job->w0 == 0 && job->ws == 1 && nsets >= 1 && nsets <= MSM_MAX_SETS && msm_multi_supported(n, job->window_hint, count);
    for (int i = 0; i < nsets && ok; ++i) ok = sets[i].level_stride != 0 && !sets[i].remap && sets[i].index_sub == 0;
    if (!ok) { set_error("msm: unsupported multi launch"); return ZKG_ERROR; }
    job->g = pick_geom(n, job->window_hint); job->n = n;
    job->empty = false; job->converted_aside = false;
    MsmLaunchSets ls; ls.space = &job->space;
    msm_job_split_sets(job, sets, nsets, n, false, ls);
    job->multi = count; job->multi_stride = scalar_stride;
    const MsmLaunchMode mode;                                                   // the default; a multi launch never feeds the kernel timer
    if (sort_digits(job, ls, d_scalars, scalars_mont, nullptr, mode)) return ZKG_ERROR;
    return msm_job_enqueue_accumulate(job, ls, nullptr, mode);
}
// out_g1[p * (G1 sets) + k]: vector p over the k-th G1 set of the launch; out_g2 likewise
int msm_job_finish_multi(MsmJob *job, G1 *out_g1, G2 *out_g2) {
    ZK_HIP(hipStreamSynchronize(job->stream));
    const int n1 = job->group[0].nsets, n2 = job->group[1].nsets;
    host_parallel_for((int)job->multi, [&](int p) {
        for (int k = 0; k < n1; ++k) out_g1[p * n1 + k] = host_combine<Fq>(job, job->group[0], k, p);
        for (int k = 0; k < n2; ++k) out_g2[p * n2 + k] = host_combine<Fq2>(job, job->group[1], k, p);
    });
    return ZKG_OK;
}
// wait for the job's stream and finish on the host; outputs in launch order: out_g1[k] for the k-th G1 set, out_g2[k] for the k-th G2 set
int msm_job_finish(MsmJob *job, G1 *out_g1, G2 *out_g2) {
    static const bool dbg = getenv("ZKG_DEBUG_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    ZK_HIP(hipStreamSynchronize(job->stream));
    const auto t1 = std::chrono::steady_clock::now();
    struct Lap { bool on; std::chrono::steady_clock::time_point a, b; ~Lap() { if (on) fprintf(stderr, "[zkg]     job finish: waited %.3f ms, host combine %.3f ms\n", std::chrono::duration<float, std::milli>(b - a).count(), std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - b).count()); } } lap_{dbg, t0, t1};
    for (int k = 0; k < job->group[0].nsets; ++k) out_g1[k] = job->empty ? G1::inf() : host_combine<Fq>(job, job->group[0], k);
    for (int k = 0; k < job->group[1].nsets; ++k) out_g2[k] = job->empty ? G2::inf() : host_combine<Fq2>(job, job->group[1], k);
    return ZKG_OK;
}

void msm_job_set_device_finish(MsmJob *j, bool on) { if (j) j->dev_finish = on; }
// The device epilogue of a launch made under msm_job_set_device_finish: nothing is copied back and nothing is waited for.  k_msm_combine goes
// onto the job's stream behind the reduction with the launch's geometry by value, and writes the points of the launch's table sets where
// msm_job_finish / msm_job_finish_multi would return them — d_out[(p * sets + k) * 12 limbs] for G1 sets, 24 limbs for G2 sets, normalised as
// store_norm does.  The sets of a launch are all of one group: a launch of both is refused.
template <class F> static int finish_dev(MsmJob *job, const MsmGroup &gr, uint32_t *out) {
    const uint32_t vectors = job->multi > 1 ? job->multi : 1;
    if (job->empty) {
        const uint32_t count = vectors * (uint32_t)gr.nsets;
        hipLaunchKernelGGL(k_msm_store_inf<F>, dim3((count + 63) / 64), dim3(64), 0, job->stream, out, count);
    } else {
        if (!gr.table || gr.red_windows != vectors || gr.red_slots > COMBINE_MAX_SLOTS<F>) { set_error("msm_job_finish_dev: table sets only (a plain set's windows need the Horner doublings)"); return ZKG_ERROR; }
        launch_combine<F>(dim3(vectors, (unsigned)gr.nsets), job->stream, gr.red_out.as<XYZZ<F>>(), gr.cpw, gr.red_slots, gr.chunk_log, gr.red_stride, out);
    }
    if (hipGetLastError() != hipSuccess) { set_error("msm combine launch failed"); return ZKG_ERROR; }
    return ZKG_OK;
}
int msm_job_finish_dev(MsmJob *job, uint64_t *d_out) {
    const bool g2 = job->group[0].nsets == 0;
    const MsmGroup &gr = job->group[g2 ? 1 : 0];
    if (!job->dev_finish || (job->group[0].nsets && job->group[1].nsets) || gr.nsets < 1) { set_error("msm_job_finish_dev: a device-finish launch of G1 sets only, or of G2 sets only"); return ZKG_ERROR; }
    uint32_t *out = reinterpret_cast<uint32_t *>(d_out);
    return g2 ? finish_dev<Fq2>(job, gr, out) : finish_dev<Fq>(job, gr, out);
}
// zkg_msm_combine_gpu, zkg_msm_combine_g2_gpu: k_msm_combine alone on records the caller makes up.  records_jac: vectors x cpw x slots
// normalised points (12 limbs, 24 for G2) in the reduction's order (vector, chunk, slot); out_jac: one normalised point per vector.  Host
// pointers; synchronous.
template <class F> static int combine_records(const uint64_t *records_jac, size_t cpw, int slots, int chunk_log, size_t vectors, uint64_t *out_jac) {
    constexpr size_t point_bytes = POINT_WORDS<F> * 4;
    const size_t count = vectors * cpw * (size_t)slots;
    ScopedDevBuf in, rec, out;
    if (in.reserve(count * point_bytes) || rec.reserve(count * sizeof(XYZZ<F>)) || out.reserve(vectors * point_bytes)) return ZKG_ERROR;
    ZK_HIP(hipMemcpy(in.p, records_jac, count * point_bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_jac_to_records<F>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, nullptr, in.as<uint32_t>(), count, rec.as<XYZZ<F>>());
    launch_combine<F>(dim3((unsigned)vectors, 1), nullptr, rec.as<XYZZ<F>>(), (uint32_t)cpw, slots, chunk_log, (size_t)0, out.as<uint32_t>());
    if (hipGetLastError() != hipSuccess) { set_error("msm combine launch failed"); return ZKG_ERROR; }
    ZK_HIP(hipMemcpy(out_jac, out.p, vectors * point_bytes, hipMemcpyDeviceToHost));     // (waits for the null stream)
    return ZKG_OK;
}
int msm_combine_records(bool g2, const uint64_t *records_jac, size_t cpw, int slots, int chunk_log, size_t vectors, uint64_t *out_jac) {
    const bool args = records_jac && out_jac && cpw >= 1 && cpw <= ((size_t)1 << 16) && chunk_log >= 0 && chunk_log <= 24 && vectors >= 1 && vectors <= 1024;
    if (g2) {
        if (!args || slots != 2) { set_error("zkg_msm_combine_g2_gpu: bad argument (1 <= cpw <= 2^16, 0 <= chunk_log <= 24, 1 <= vectors <= 1024)"); return ZKG_ERROR; }
        return combine_records<Fq2>(records_jac, cpw, slots, chunk_log, vectors, out_jac);
    }
    if (!args || (slots != 2 && slots != 3)) { set_error("zkg_msm_combine_gpu: bad argument (1 <= cpw <= 2^16, slots 2 or 3, 0 <= chunk_log <= 24, 1 <= vectors <= 1024)"); return ZKG_ERROR; }
    return combine_records<Fq>(records_jac, cpw, slots, chunk_log, vectors, out_jac);
}
// what one scalar vector of a table launch asks of the bucket workspace (launch_accumulate: every window's bucket set, before the fold)
size_t msm_table_bucket_bytes(int c, bool g2) {
    const MsmGeom g = pick_geom(1, c);
    return (size_t)g.W * g.B * (g2 ? std::max(sizeof(XYZZ<Fq2>), sizeof(Bucket29)) : std::max(sizeof(XYZZ<Fq>), sizeof(Bucket29)));
}


int msm_shared(const G1Affine *const *d_g1_bases, int n_g1, const G2Affine *d_g2_bases, const uint32_t *d_scalars, size_t n,
               bool scalars_mont, G1 *out_g1, G2 *out_g2, hipStream_t s, uint32_t w0, uint32_t ws, bool mostly_bits) {
    if (n_g1 < 0 || n_g1 + (d_g2_bases ? 1 : 0) > MSM_MAX_SETS) { set_error("msm: too many base sets"); return ZKG_ERROR; }
    std::lock_guard<std::mutex> lk(g_default_job.mu);
    g_dominant_timer.new_call();
    g_default_job.stream = s; g_default_job.w0 = w0; g_default_job.ws = ws ? ws : 1; g_default_job.one_pass_sort = mostly_bits;
    MsmBases sets[MSM_MAX_SETS]; int nsets = 0;
    for (int i = 0; i < n_g1; ++i) { sets[nsets] = MsmBases(); sets[nsets].p = d_g1_bases[i]; ++nsets; }
    if (d_g2_bases) { sets[nsets] = MsmBases(); sets[nsets].p = d_g2_bases; sets[nsets].g2 = true; ++nsets; }
    // Above 2^23 points the job is cut into 2^23-point pieces run one after the other and summed on the host: the sort's 32-bit entry
    // space, its LDS bin sizes and the workspace (40 B per point and window) are sized for that, and per point a 2^26-point launch was
    // measured 2.2x slower than eight 2^23-point ones (275 ms against 8 x 15.3 ms).  Window-sharded launches keep their single pass.
    if (n >= ((size_t)1 << 28)) { set_error("msm: at most 2^28 - 1 points per call"); return ZKG_ERROR; }      // refused before a byte is touched
    const size_t PIECE = (size_t)1 << 23;
    if (n <= PIECE || w0 != 0 || g_default_job.ws != 1) {
        if (msm_job_launch(&g_default_job, sets, nsets, d_scalars, n, scalars_mont, nullptr)) return ZKG_ERROR;
        return msm_job_finish(&g_default_job, out_g1, out_g2);
    }
    G1 acc1[MSM_MAX_SETS]; G2 acc2[MSM_MAX_SETS];
    for (int i = 0; i < MSM_MAX_SETS; ++i) { acc1[i] = G1::inf(); acc2[i] = G2::inf(); }
    for (size_t lo = 0; lo < n; lo += PIECE) {
        const size_t cnt = std::min(PIECE, n - lo);
        MsmBases piece[MSM_MAX_SETS];
        for (int i = 0; i < nsets; ++i) { piece[i] = sets[i]; piece[i].p = (const char *)sets[i].p + lo * (sets[i].g2 ? sizeof(G2Affine) : sizeof(G1Affine)); }
        G1 p1[MSM_MAX_SETS]; G2 p2[MSM_MAX_SETS];
        if (msm_job_launch(&g_default_job, piece, nsets, d_scalars + 8 * lo, cnt, scalars_mont, nullptr) || msm_job_finish(&g_default_job, p1, p2)) return ZKG_ERROR;
        for (int i = 0; i < n_g1; ++i) acc1[i].add(p1[i]);
        if (d_g2_bases) acc2[0].add(p2[0]);
    }
    for (int i = 0; i < n_g1; ++i) out_g1[i] = acc1[i];
    if (d_g2_bases) out_g2[0] = acc2[0];
    return ZKG_OK;
}

// msm_g1_host_scalars' piece boundaries cut[0 .. P] (returns P): halves from the top, the lowest one split once more -> n/8, n/8, n/4, n/2 for four pieces
static int host_scalars_cuts(size_t n, int max_pieces, size_t cut[9]) {
    int P = max_pieces;
    cut[P] = n;
    for (int k = P - 1; k >= 1; --k) cut[k] = (cut[k + 1] / 2) & ~(size_t)255;
    cut[0] = 0;
    if (const char *e = getenv("ZKG_MSM_CUTS")) {                              // tuning aid: the piece boundaries in 64ths of n, e.g. "8,32" -> n/8, 3n/8, n/2
        int k = 1; const char *q = e;
        while (*q && k < 8) { const long v = strtol(q, const_cast<char **>(&q), 10); if (v <= 0 || v >= 64) break; cut[k++] = (n * (size_t)v / 64) & ~(size_t)255; if (*q == ',') ++q; }
        if (k > 1) { P = k; cut[P] = n; for (int i = 1; i < P; ++i) if (cut[i] < cut[i - 1]) cut[i] = cut[i - 1]; }
    }
    return P;
}
// Bases resident, scalars in HOST memory: SURVEY.md section 8(d)'s step ("wall clock around the call incl. H2D of scalars; bases resident") as
// one entry point.  The upload is 32 B x n over PCIe (0.6 ms at 2^20 points) against 1.9 ms of work that cannot start on a scalar it has not
// seen — so the job is cut by POINTS into pieces (1/8, 1/8, 1/4, 1/2 of them, host_scalars_cuts: a small first piece starts the chip early, and every later
// piece's upload is shorter than the work of the piece before it), each piece sorted and accumulated as it lands, all pieces into ONE set of
// buckets (k_bucket_accum29's `resume`: a lane picks its bucket's 29-bit accumulator up where the last piece left it), and one reduction at
// the end.  Same point as msm_g1 on the uploaded vector: the buckets hold the same sums, whatever the order of the additions.
int msm_g1_host_scalars(const G1Affine *d_bases, const uint32_t *h_scalars, size_t n, bool mont, G1 *out, hipStream_t s) {
    if (n >= ((size_t)1 << 28)) { set_error("msm: at most 2^28 - 1 points per call"); return ZKG_ERROR; }
    if (!n) { *out = G1::inf(); return ZKG_OK; }
    static const int max_pieces = getenv("ZKG_MSM_PIECES") ? std::max(1, std::min(8, atoi(getenv("ZKG_MSM_PIECES")))) : 4;        // tuning aid (1: one upload, one launch); 2^20 points, sorts beside the accumulation (ACC29_VGPRS, sort_wave_priority): 3 / 4 / 5 pieces 1.99 / 1.94 / 2.02 ms (before: 2.19 / 2.27 / 2.41)
    const bool pieces = max_pieces > 1 && n >= ((size_t)1 << 19) && n <= ((size_t)1 << 23);
    if (n > ((size_t)1 << 23)) {                                                // huge: one upload, then the resident path's own 2^23-point pieces
        ScopedDevBuf tmp;
        if (tmp.reserve(n * 32)) return ZKG_ERROR;
        ZK_HIP(hipMemcpyAsync(tmp.p, h_scalars, n * 32, hipMemcpyHostToDevice, s));
        return msm_g1(d_bases, tmp.as<uint32_t>(), n, mont, out, s, false);     // (returns after the stream has drained: tmp may go)
    }
    MsmJob &J = g_default_job; PieceStep &T = g_step;
    std::lock_guard<std::mutex> lk(J.mu);
    g_dominant_timer.new_call();
    if (T.scalars.reserve(n * 32)) return ZKG_ERROR;
    uint32_t *d_sc = T.scalars.as<uint32_t>();
    J.stream = s; J.w0 = 0; J.ws = 1; J.one_pass_sort = false;
    MsmBases set; set.p = d_bases;
    T.stats = HostScalarsStats();
    MsmLaunchMode mode; mode.timed = true; mode.stream_waits = &T.stats.waits;
    if (!pieces) {                                                              // small or switched off: one upload in stream order, one launch
        ZK_HIP(hipMemcpyAsync(d_sc, h_scalars, n * 32, hipMemcpyHostToDevice, s));
        if (msm_job_launch_as(&J, &set, 1, d_sc, n, mont, nullptr, mode)) return ZKG_ERROR;
        T.stats.pieces = 1; T.stats.heavy[0] = 0xffffffffu; T.stats.pair[0] = 1;     // (the pair goes out blind: nobody reads a count)
        return msm_job_finish(&J, out, nullptr);
    }
    if (T.ensure()) return ZKG_ERROR;
    size_t cut[9]; const int P = host_scalars_cuts(n, max_pieces, cut);
    // The uploads run on a stream of their own, and the contract is the single launch's, whose upload is on `s` itself: pinned scalars may be
    // written by work queued on `s` before the call.  So the copy stream waits for what `s` holds now — the copy stream, not the caller's: no
    // wait goes onto `s`.  A stream that has drained has nothing to wait for, and the first upload then starts without a wait in front of it.
    if (hipStreamQuery(s) != hipSuccess) {
        (void)hipGetLastError();                                                // (hipErrorNotReady is an answer, not a failure of the launches below)
        ZK_HIP(hipEventRecord(T.ev_caller, s));
        ZK_HIP(hipStreamWaitEvent(T.copy, T.ev_caller, 0));
    }
    for (int k = 0; k < P; ++k) {
        ZK_HIP(hipMemcpyAsync(d_sc + 8 * cut[k], h_scalars + 8 * cut[k], (cut[k + 1] - cut[k]) * 32, hipMemcpyHostToDevice, T.copy));
        ZK_HIP(hipEventRecord(T.ev_piece[k], T.copy));
    }
    // Pieces alternate between two sort workspaces — the default job's and the step's — over ONE set of buckets, all accumulations in order on the caller's stream —
    // and every piece's digit sort runs on a high-priority stream of its own beside the accumulation of the piece before it: the sort's
    // small dependent launches and single-workgroup scans stand a third of a step when alone and cost the accumulation little beside it
    // (without the priority they crawl: k_rx_count 134 us instead of 11; and they only run BESIDE it because the accumulation leaves a
    // quarter of each SIMD's registers free and the sort's wavefronts raise their own issue priority — ACC29_VGPRS, sort_wave_priority).  The bases' 29-bit records are made once for all pieces, on
    // the side stream, under the first upload.
    // all bases as 29-bit records, once, under the first piece's upload (the calling thread waits for ev_join before the first accumulation, below)
    if (msm_job_convert_aside(&J, d_bases, n)) return ZKG_ERROR;
    ZK_HIP(hipStreamWaitEvent(T.sort, J.ev_fork, 0));
    mode.sort_stream = T.sort; mode.beside = true;
    mode.window = (int)pick_geom(n, J.window_hint).c;                         // every piece under the whole job's window size
    // The calling thread paces the accumulations (it would only sleep in msm_job_finish otherwise): an accumulation is enqueued once the host has
    // seen its sort finish, so the caller's stream carries kernels and one event record per piece and no cross-stream wait — such a wait in front
    // of a kernel stood for 15 ... 23 us of idle chip even where the awaited sort had ended long before.  And the host then knows the piece's
    // heavy-bucket count (k_order_place's word, visible once ev_sorted has completed: the event keeps its system-scope fence): the heavy pair is
    // launched only where it has work.  Per piece: the NEXT piece's sort goes onto the sort stream first, with its waits for its upload and for the
    // accumulation that last read its buffers on the device — two pieces back: that accumulation's ev_acc_done was recorded in the round before —
    // then the host waits for this piece's sort, enqueues its accumulation and records ev_acc_done behind it.
    int run[8], R = 0;
    for (int k = 0; k < P; ++k) if (cut[k + 1] != cut[k] || k + 1 == P) run[R++] = k;      // (empty pieces are skipped; the last one always runs: it carries the reduction)
    MsmLaunchSets ls[2];
    int rc = ZKG_OK; bool used[2] = {false, false};
    // pieces alternate over the two workspaces by their position among the pieces that run; the last one sorts into the default job's own
    auto enqueue_sort = [&](int i) {
        const int k = run[i], which = (R - 1 - i) & 1;
        MsmBases piece = set; piece.p = reinterpret_cast<const char *>(d_bases) + cut[k] * sizeof(G1Affine);
        piece.p29 = J.group[0].bases29.as<Rec64>() + cut[k];
        mode.heavy_out = T.heavy_words + i;
        // after its scalars have landed, and after the accumulation that last read this workspace
        if (hipStreamWaitEvent(T.sort, T.ev_piece[k], 0) != hipSuccess) return ZKG_ERROR;
        if (used[which] && hipStreamWaitEvent(T.sort, T.ev_acc_done[which], 0) != hipSuccess) return ZKG_ERROR;
        if (msm_job_enqueue_sort(&J, which ? T.space : J.space, &piece, 1, d_sc + 8 * cut[k], cut[k + 1] - cut[k], mont, nullptr, mode, ls[which])) return ZKG_ERROR;
        return !ls[which].empty && hipEventRecord(T.ev_sorted[which], T.sort) != hipSuccess ? ZKG_ERROR : ZKG_OK;
    };
    rc = enqueue_sort(0);
    for (int i = 0; i < R && rc == ZKG_OK; ++i) {
        const int which = (R - 1 - i) & 1;
        if (i + 1 < R && (rc = enqueue_sort(i + 1)) != ZKG_OK) break;
        if (i == 0 && hipEventSynchronize(J.ev_join) != hipSuccess) { rc = ZKG_ERROR; break; }      // the bases' records
        uint32_t heavy = 0;
        if (!ls[which].empty) {
            if (hipEventSynchronize(T.ev_sorted[which]) != hipSuccess) { rc = ZKG_ERROR; break; }
            heavy = *static_cast<volatile const uint32_t *>(T.heavy_words + i);
        }
        mode.resume = i > 0; mode.defer_reduce = i + 1 < R; mode.heavy_pair = heavy != 0;
        rc = msm_job_enqueue_accumulate(&J, ls[which], nullptr, mode);
        if (rc == ZKG_OK && hipEventRecord(T.ev_acc_done[which], s) != hipSuccess) rc = ZKG_ERROR;
        used[which] = true;
        T.stats.heavy[i] = heavy; T.stats.pair[i] = heavy != 0; T.stats.pieces = (uint32_t)(i + 1);
    }
    if (rc != ZKG_OK) { (void)hipStreamSynchronize(T.copy); (void)hipStreamSynchronize(J.aux); (void)hipStreamSynchronize(T.sort); (void)hipStreamSynchronize(s); return ZKG_ERROR; }
    return msm_job_finish(&J, out, nullptr);
}
// out: pieces | stream waits | (heavy count, pair launched) per piece — at most n words; returns the words the record has (0: no call yet)
int msm_host_scalars_stats(uint32_t *out, int n) {
    std::lock_guard<std::mutex> lk(g_default_job.mu);
    const HostScalarsStats &st = g_step.stats;
    if (!st.pieces) return 0;
    uint32_t rec[2 + 2 * 8] = {st.pieces, st.waits};
    for (uint32_t k = 0; k < st.pieces; ++k) { rec[2 + 2 * k] = st.heavy[k]; rec[3 + 2 * k] = st.pair[k]; }
    const int words = 2 + 2 * (int)st.pieces;
    for (int i = 0; i < words && i < n; ++i) out[i] = rec[i];
    return words;
}

int msm_g1(const G1Affine *d_bases, const uint32_t *d_scalars, size_t n, bool mont, G1 *out, hipStream_t s, bool mostly_bits) {
    return msm_shared(&d_bases, 1, nullptr, d_scalars, n, mont, out, nullptr, s, 0, 1, mostly_bits);
}
int msm_g2(const G2Affine *d_bases, const uint32_t *d_scalars, size_t n, bool mont, G2 *out, hipStream_t s, bool mostly_bits) {
    return msm_shared(nullptr, 0, d_bases, d_scalars, n, mont, nullptr, out, s, 0, 1, mostly_bits);
}

// ---- per-window tables of a resident base set (built once per key) ------------------------------------------------
template <class F>
static int window_table_build_t(WindowTable &t, const Affine<F> *d_bases, size_t n, int c, hipStream_t s) {
    t.n = n; t.c = c; t.W = (SCALAR_BITS + c - 1) / c; t.g2 = sizeof(F) != sizeof(Fq);
    if (t.buf.reserve(std::max<size_t>(1, n) * t.W * sizeof(Affine<F>))) return ZKG_ERROR;
    if (!n) return ZKG_OK;
    Affine<F> *lv = t.buf.as<Affine<F>>();
    ZK_HIP(hipMemcpyAsync(lv, d_bases, n * sizeof(Affine<F>), hipMemcpyDeviceToDevice, s));
    constexpr int K = sizeof(F) != sizeof(Fq) ? 2 : 4;                          // levels per launch (the K results stay in registers)
    for (int w = 1; w < t.W; w += K)
        hipLaunchKernelGGL((k_table_levels<F, K>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lv + (size_t)(w - 1) * n, lv + (size_t)w * n, n, (uint32_t)c,
                           std::min(K, t.W - w));
    if (hipGetLastError() != hipSuccess) { set_error("window table launch failed"); return ZKG_ERROR; }
    return ZKG_OK;
}
int window_table_build_g1(WindowTable &t, const G1Affine *d_bases, size_t n, int c, hipStream_t s) { return window_table_build_t<Fq>(t, d_bases, n, c, s); }
int window_table_records29(WindowTable &t, hipStream_t s) {
    if (t.g2) { set_error("window_table_records29: G1 tables only"); return ZKG_ERROR; }
    const size_t total = t.n * (size_t)t.W;
    if (t.rec29.reserve(std::max<size_t>(1, total) * sizeof(Rec64))) return ZKG_ERROR;
    if (total) hipLaunchKernelGGL(k_bases_to29, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, t.buf.as<Affine<Fq>>(), total, t.rec29.as<Rec64>());
    if (hipGetLastError() != hipSuccess) { set_error("window table records launch failed"); return ZKG_ERROR; }
    return ZKG_OK;
}
int window_table_build_g2(WindowTable &t, const G2Affine *d_bases, size_t n, int c, hipStream_t s) { return window_table_build_t<Fq2>(t, d_bases, n, c, s); }

// ---- witness split: classification and the flat sum of the bases whose scalar is one ----------------------------------
int witness_classify(const Fr *d_z, size_t n1, uint8_t *d_tags, uint32_t *d_listed, uint32_t *d_count, hipStream_t s, const uint32_t *d_subset_pos) {
    ZK_HIP(hipMemsetAsync(d_count, 0, 8, s));
    if (n1) hipLaunchKernelGGL(k_classify, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, d_z, n1, d_tags, d_listed, d_count, d_subset_pos);
    return hipGetLastError() == hipSuccess ? ZKG_OK : ZKG_ERROR;
}
template <class F> static int gather_points_t(const Affine<F> *d_src, const uint32_t *d_idx, size_t count, uint32_t index_sub, Affine<F> *d_out, hipStream_t s) {
    if (count) hipLaunchKernelGGL(k_gather_points<F>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, d_src, d_idx, count, index_sub, d_out);
    return hipGetLastError() == hipSuccess ? ZKG_OK : ZKG_ERROR;
}
int gather_points_g1(const G1Affine *d_src, const uint32_t *d_idx, size_t count, uint32_t index_sub, G1Affine *d_out, hipStream_t s) { return gather_points_t<Fq>(d_src, d_idx, count, index_sub, d_out, s); }
int gather_points_g2(const G2Affine *d_src, const uint32_t *d_idx, size_t count, uint32_t index_sub, G2Affine *d_out, hipStream_t s) { return gather_points_t<Fq2>(d_src, d_idx, count, index_sub, d_out, s); }
template <class F> static int scatter_points_t(const Affine<F> *d_src, const uint32_t *d_idx, size_t count, Affine<F> *d_out, hipStream_t s) {
    if (count) hipLaunchKernelGGL(k_scatter_points<F>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, d_src, d_idx, count, d_out);
    return hipGetLastError() == hipSuccess ? ZKG_OK : ZKG_ERROR;
}
int scatter_points_g1(const G1Affine *d_src, const uint32_t *d_idx, size_t count, G1Affine *d_out, hipStream_t s) { return scatter_points_t<Fq>(d_src, d_idx, count, d_out, s); }
int scatter_points_g2(const G2Affine *d_src, const uint32_t *d_idx, size_t count, G2Affine *d_out, hipStream_t s) { return scatter_points_t<Fq2>(d_src, d_idx, count, d_out, s); }
template <class F>
static int ones_sum_launch_t(OnesSum &o, const MsmBases *sets, int nsets, const uint8_t *d_tags, size_t n1, hipStream_t s, size_t tag_stride = 0, uint32_t vecs = 1) {
    // per workgroup: list the positions tagged 1, lanes stride over the list, an 8-level LDS tree; one more workgroup per set sums the partials
    if (nsets < 1 || nsets > MSM_MAX_SETS) { set_error("ones-sum: bad set count"); return ZKG_ERROR; }
    // tags per workgroup: a 256th of the vector, at least 1024 (a short list per lane leaves only the trees) and at most 8192 (32 KiB of LDS list)
    const uint32_t span = (uint32_t)std::min<size_t>(8192, std::max<size_t>(1024, ((n1 + 255) / 256 + 255) / 256 * 256));
    const unsigned blocks = (unsigned)std::max<size_t>(1, (n1 + span - 1) / span);
    o.g2 = sizeof(F) != sizeof(Fq); o.nsets = nsets;
    const size_t vec_stride = (size_t)nsets * (blocks + 1), host_bytes = std::max<size_t>(MSM_MAX_SETS, (size_t)vecs * nsets) * sizeof(G2);
    if (o.partials.reserve(vecs * vec_stride * sizeof(XYZZ<F>))) return ZKG_ERROR;
    if (o.host_bytes < host_bytes) {
        if (o.host) (void)hipHostFree(o.host);
        o.host = nullptr; o.host_bytes = 0;
        if (!hip_ok(hipHostMalloc(&o.host, host_bytes, hipHostMallocDefault), "hipHostMalloc", __FILE__, __LINE__)) return ZKG_ERROR;
        o.host_bytes = host_bytes;
    }
    XYZZ<F> *part = o.partials.as<XYZZ<F>>();
    ViewSet<F> views;
    for (int i = 0; i < MSM_MAX_SETS; ++i) { const MsmBases &b = sets[i < nsets ? i : 0]; views.v[i] = BaseView<F>{reinterpret_cast<const Affine<F> *>(b.p), 0, nullptr, b.index_sub, 1, nullptr}; }
    hipLaunchKernelGGL(k_ones_sum<F>, dim3(blocks, (unsigned)nsets, vecs), dim3(256), 256 * sizeof(LdsPoint<F>) + (size_t)span * 4, s, views, d_tags, n1, span, part, tag_stride, vec_stride);
    hipLaunchKernelGGL(k_sum_partials<F>, dim3((unsigned)nsets, vecs), dim3(256), 256 * sizeof(LdsPoint<F>), s, part, blocks, vec_stride);
    if (hipGetLastError() != hipSuccess) { set_error("ones-sum launch failed"); return ZKG_ERROR; }
    if (vecs > 1) {                                                             // vecs x nsets results, (blocks + 1) points apart, in one strided copy
        ZK_HIP(hipMemcpy2DAsync(o.host, sizeof(XYZZ<F>), part + blocks, (blocks + 1) * sizeof(XYZZ<F>), sizeof(XYZZ<F>), (size_t)vecs * nsets, hipMemcpyDeviceToHost, s));
        return ZKG_OK;
    }
    for (int i = 0; i < nsets; ++i)
        ZK_HIP(hipMemcpyAsync((char *)o.host + (size_t)i * sizeof(XYZZ<F>), part + (size_t)i * (blocks + 1) + blocks, sizeof(XYZZ<F>), hipMemcpyDeviceToHost, s));
    return ZKG_OK;
}
int ones_sum_launch(OnesSum &o, const MsmBases *sets, int nsets, const uint8_t *d_tags, size_t n1, hipStream_t s) {
    for (int i = 1; i < nsets; ++i) if (sets[i].g2 != sets[0].g2) { set_error("ones-sum: one field per launch"); return ZKG_ERROR; }
    return sets[0].g2 ? ones_sum_launch_t<Fq2>(o, sets, nsets, d_tags, n1, s) : ones_sum_launch_t<Fq>(o, sets, nsets, d_tags, n1, s);
}
// the same for `count` witnesses' tag arrays, tag_stride bytes apart, as one launch pair: result of witness p, set i at index p * nsets + i
int ones_sum_launch_multi(OnesSum &o, const MsmBases *sets, int nsets, const uint8_t *d_tags, size_t tag_stride, size_t n1, uint32_t count, hipStream_t s) {
    for (int i = 1; i < nsets; ++i) if (sets[i].g2 != sets[0].g2) { set_error("ones-sum: one field per launch"); return ZKG_ERROR; }
    if (count < 1 || count > 65535) { set_error("ones-sum: bad witness count"); return ZKG_ERROR; }
    return sets[0].g2 ? ones_sum_launch_t<Fq2>(o, sets, nsets, d_tags, n1, s, tag_stride, count) : ones_sum_launch_t<Fq>(o, sets, nsets, d_tags, n1, s, tag_stride, count);
}
void OnesSum::release() { partials.release(); if (host) (void)hipHostFree(host); host = nullptr; host_bytes = 0; }

// ---- fixed-base batch: out[i] = k_i * base (libff batch_exp with a window table; libsnark's generator, snark.cpp:91) --------------
//      Table: entry [j][d-1] = d * 256^j * base (j < 32, d = 1..255), affine, 522 KB for G1: a scalar is 32 byte digits, i.e. at most
//      32 mixed additions and no doubling (the first build added bit by bit: 254 conditional additions).  A lane takes FB_K scalars and
//      keeps their results in registers, so that ONE field inversion (Montgomery's trick over ZZZ) normalises all of them: the kernel
//      writes each affine point once and nothing else (the first build's out-of-line to_affine spilt to scratch: 123x the output bytes).
static constexpr int FB_WINDOWS = 32, FB_DIGITS = 255, FB_K = 4;
template <class F>
__global__ __launch_bounds__(256) void k_fixed_table(const Affine<F> *rows /* 256^j * base */, Affine<F> *table) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= FB_WINDOWS * FB_DIGITS) return;
    const uint32_t j = t / FB_DIGITS, d = t % FB_DIGITS + 1;
    const Affine<F> r = rows[j];
    XYZZ<F> acc = XYZZ<F>::inf();
    for (int bit = 7; bit >= 0; --bit) { acc = acc.dbl(); if ((d >> bit) & 1u) acc.madd(r); }
    XYZZ<F> fin = acc;
    table[t] = fin.to_affine().normalized();
}
template <class F>
__global__ __launch_bounds__(256) void k_fixed_base(const Affine<F> *table, const uint32_t *scalars, size_t n, int mont, Affine<F> *out) {
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i0 = lane * FB_K;
    if (i0 >= n) return;
    F x[FB_K], y[FB_K], zz[FB_K], zzz[FB_K];
#pragma unroll
    for (int k = 0; k < FB_K; ++k) {
        XYZZ<F> acc = XYZZ<F>::inf();
        if (i0 + k < n) {
            Fr f;
            for (int j = 0; j < 8; ++j) f.v[j] = scalars[8 * (i0 + k) + j];
            if (mont) f = f.from_mont();                                        // the generator hands over Montgomery Fr; the ABI canonical limbs
            else f = f.normalized();
            for (int j = 0; j < FB_WINDOWS; ++j) {
                const uint32_t d = (f.v[j >> 2] >> (8 * (j & 3))) & 255u;
                if (d) acc.madd(table[j * FB_DIGITS + d - 1]);
            }
        }
        x[k] = acc.x; y[k] = acc.y; zz[k] = acc.zz; zzz[k] = acc.zzz;
    }
    // Montgomery's trick over the FB_K values of ZZZ (infinity: ZZZ = 0, replaced by one and restored below)
    F pre[FB_K], run = F::one();
#pragma unroll
    for (int k = 0; k < FB_K; ++k) { pre[k] = run; if (!zzz[k].is_zero()) run = run * zzz[k]; }
    F inv = inverse_fast(run);
#pragma unroll
    for (int k = FB_K - 1; k >= 0; --k) {
        if (i0 + k >= n) continue;
        if (zzz[k].is_zero()) { out[i0 + k] = Affine<F>::inf(); continue; }
        F zi = inv * pre[k];                                                    // 1 / ZZZ_k
        inv = inv * zzz[k];
        F t = zi * zz[k];                                                       // ZZ / ZZZ = 1 / Z
        F zi2 = t.sqr();                                                        // 1 / ZZ
        out[i0 + k] = Affine<F>{x[k] * zi2, y[k] * zi}.normalized();
    }
}

// table per base point, built once per process (the generator always uses the curve's generators)
template <class F> struct FixedTableCache { std::mutex mu; std::vector<std::pair<Affine<F>, DevBuf>> entries; };
template <class F> static FixedTableCache<F> &fixed_cache() { static FixedTableCache<F> c; return c; }
template <class F>
static const Affine<F> *fixed_table_for(const Affine<F> &base, hipStream_t s) {
    FixedTableCache<F> &c = fixed_cache<F>();
    std::lock_guard<std::mutex> lk(c.mu);
    for (auto &e : c.entries) if (memcmp(&e.first, &base, sizeof(base)) == 0) return e.second.template as<Affine<F>>();
    std::vector<Affine<F>> rows(FB_WINDOWS);
    XYZZ<F> cur = XYZZ<F>::from_affine(base);
    for (int j = 0; j < FB_WINDOWS; ++j) { rows[j] = cur.to_affine(); for (int k = 0; k < 8; ++k) cur = cur.dbl(); }
    DevBuf d_rows, d_table;
    if (d_rows.reserve(rows.size() * sizeof(Affine<F>)) || d_table.reserve((size_t)FB_WINDOWS * FB_DIGITS * sizeof(Affine<F>))) return nullptr;
    if (!hip_ok(hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * sizeof(Affine<F>), hipMemcpyHostToDevice, s), "H2D", __FILE__, __LINE__)) return nullptr;
    hipLaunchKernelGGL(k_fixed_table<F>, dim3((FB_WINDOWS * FB_DIGITS + 255) / 256), dim3(256), 0, s, d_rows.as<Affine<F>>(), d_table.as<Affine<F>>());
    const bool ok = hipGetLastError() == hipSuccess && hip_ok(hipStreamSynchronize(s), "sync", __FILE__, __LINE__);
    d_rows.release();
    if (!ok) { d_table.release(); set_error("fixed-base table build failed"); return nullptr; }
    c.entries.emplace_back(base, d_table);
    return c.entries.back().second.template as<Affine<F>>();
}
template <class F>
static int fixed_base(const Affine<F> &base, const uint32_t *d_scalars, size_t n, Affine<F> *d_out, hipStream_t s, bool mont) {
    const Affine<F> *table = fixed_table_for<F>(base, s);
    if (!table) return ZKG_ERROR;
    const size_t lanes = (n + FB_K - 1) / FB_K;
    if (n) hipLaunchKernelGGL(k_fixed_base<F>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, table, d_scalars, n, (int)mont, d_out);
    hipError_t e = hipGetLastError();
    ZK_HIP(hipStreamSynchronize(s));
    if (e != hipSuccess) { set_error("fixed_base launch failed"); return ZKG_ERROR; }
    return ZKG_OK;
}
int fixed_base_g1(const G1Affine &base, const uint32_t *d_scalars, size_t n, G1Affine *d_out, hipStream_t s, bool mont) { return fixed_base<Fq>(base, d_scalars, n, d_out, s, mont); }
int fixed_base_g2(const G2Affine &base, const uint32_t *d_scalars, size_t n, G2Affine *d_out, hipStream_t s, bool mont) { return fixed_base<Fq2>(base, d_scalars, n, d_out, s, mont); }
static void fixed_tables_release() {
    { auto &c = fixed_cache<Fq>(); std::lock_guard<std::mutex> lk(c.mu); for (auto &e : c.entries) e.second.release(); c.entries.clear(); }
    { auto &c = fixed_cache<Fq2>(); std::lock_guard<std::mutex> lk(c.mu); for (auto &e : c.entries) e.second.release(); c.entries.clear(); }
}

int msm_configure() {
    bool ok = hipFuncSetAttribute((const void *)k_bucket_reduce<Fq2, RED_L_LOG_SMALL>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * RedGeom<Fq2>::LANES * (int)sizeof(LdsPoint<Fq2>)) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_bucket_reduce<Fq2, RED_L_LOG_TINY>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * RedGeom<Fq2>::LANES * (int)sizeof(LdsPoint<Fq2>)) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_bucket_reduce<Fq2, RED_L_LOG_LARGE>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * RedGeom<Fq2>::LANES * (int)sizeof(LdsPoint<Fq2>)) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_heavy_parts<Fq2>, hipFuncAttributeMaxDynamicSharedMemorySize, 256 * (int)sizeof(LdsPoint<Fq2>)) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_heavy_merge<Fq2>, hipFuncAttributeMaxDynamicSharedMemorySize, 256 * (int)sizeof(LdsPoint<Fq2>)) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_bucket_fold<Fq2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FOLD_THREADS * (int)sizeof(LdsPoint<Fq2>)) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_ones_sum<Fq2>, hipFuncAttributeMaxDynamicSharedMemorySize, 256 * (int)sizeof(LdsPoint<Fq2>) + 8192 * 4) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_ones_sum<Fq>, hipFuncAttributeMaxDynamicSharedMemorySize, 256 * (int)sizeof(LdsPoint<Fq>) + 8192 * 4) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_sum_partials<Fq2>, hipFuncAttributeMaxDynamicSharedMemorySize, 256 * (int)sizeof(LdsPoint<Fq2>)) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (1 << (MAX_C - 1)) * 4) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_place, hipFuncAttributeMaxDynamicSharedMemorySize, (1 << (MAX_C - 1)) * 4) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_bucket_reduce29l, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * RedGeom<Fq>::LANES * (int)sizeof(LdsPoint29)) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_rx_scatter<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (RX_SLICE + 4 * RX_MAX_CB + 8) * 4) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_rx_scatter<512>, hipFuncAttributeMaxDynamicSharedMemorySize, (512 * RX_PER_THREAD + 4 * RX_MAX_CB + 8) * 4) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_rx_fine<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (RX_FINE_MAX + 3 * 1024) * 4) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)k_rx_fine<512>, hipFuncAttributeMaxDynamicSharedMemorySize, (RX_FINE_MAX + 3 * 1024) * 4) == hipSuccess;
    return ok ? ZKG_OK : ZKG_ERROR;
}
void msm_release_all() {
    fixed_tables_release();
    std::lock_guard<std::mutex> lk(g_default_job.mu);
    g_default_job.release_device();       // (every handle is null afterwards: a later zkg_init may pick another device and recreates them)
    g_step.release();
}

}  // namespace zk
