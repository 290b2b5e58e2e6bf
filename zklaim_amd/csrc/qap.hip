// qap.hip — zkg_qap: r1cs_to_qap_witness_map on device-resident witnesses, as a handle on a constraint system alone (include/zkg.h).
//
// The stage the prover runs per proof on its key (prover.hip, compute_h_matvec + compute_h_transforms: three sparse mat-vecs, three iFFT,
// three cosetFFT, (A.B - C)/Z on the coset, one icosetFFT), for `count` witnesses that already lie in device memory: the mat-vec reads every
// witness where it lies (the constant is supplied by the kernel: no [1 | w] copy), aA | aB | aC and the transforms' scratch are the handle's
// workspace, the pointwise step writes into the caller's buffer and the closing icosetFFT runs there in place.  Everything is queued on the
// caller's stream; nothing waits on the host.  The row kernels share their device functions with the prover's (r1cs.hip.hpp), the transforms
// are the prover's batched runners (ntt_run_ex, step_ntt_run) with 3 g vectors per launch: a witness's H has the limbs zkg_qap_witness_h gives.
// The same handle evaluates the QAP at a point (zkg_qap_instance_async, r1cs_to_qap_instance_map_with_evaluation): see "the instance map" below.
#include "common.hpp"
#include "r1cs.hip.hpp"
#include "../../include/zkg.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

namespace zk {

struct QapCsr { const uint32_t *a_rp, *a_col; const Fr *a_val; const uint32_t *b_rp, *b_col; const Fr *b_val; const uint32_t *c_rp, *c_col; const Fr *c_val; };

// witness p (blockIdx.y) of a group: n Fr at w + p * w_stride, read in place; its aA | aB | aC at aABC + 3 p m.  Rows C..C+l of aA carry z[i - C],
// the rows beyond are zero.  A lane that holds the three values of a row without a long side tests it there (unsat[p] |= 1); the rows with a
// long side are k_qap_long's, their test k_qap_check_rows'.
__global__ __launch_bounds__(256) void k_qap_eval(QapCsr M, const Fr *w, size_t w_stride, uint32_t C, uint32_t l, size_t m, Fr *aABC, uint32_t *unsat /* or null */) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; const uint32_t p = blockIdx.y;
    if (i >= m) return;
    const WitnessInPlace z{w + p * w_stride};
    Fr *aA = aABC + (size_t)3 * p * m, *aB = aA + m, *aC = aB + m;
    Fr a = Fr::zero(), b = Fr::zero(), c = Fr::zero();
    bool la = false, lb = false, lc = false;
    if (i < C) {
        a = row_dot_short(M.a_rp, M.a_col, M.a_val, z, i, la);
        b = row_dot_short(M.b_rp, M.b_col, M.b_val, z, i, lb);
        c = row_dot_short(M.c_rp, M.c_col, M.c_val, z, i, lc);
        if (unsat && !(la | lb | lc) && a * b != c) or_and_wait(unsat + p);
    } else if (i <= (size_t)C + l) {
        a = z[i - C];
    }
    aA[i] = a.normalized(); aB[i] = b.normalized(); aC[i] = c.normalized();
}
// the long rows: one wavefront per entry of the list, a launch of its own behind k_qap_eval
__global__ __launch_bounds__(256) void k_qap_long(const uint32_t *list, uint32_t n_long, QapCsr M, const Fr *w, size_t w_stride, size_t m, Fr *aABC) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63, p = blockIdx.y;
    if (wave >= n_long) return;
    Fr *aA = aABC + (size_t)3 * p * m;
    r1cs_long_entry(list[wave], lane, M.a_rp, M.a_col, M.a_val, M.b_rp, M.b_col, M.b_val, M.c_rp, M.c_col, M.c_val, WitnessInPlace{w + p * w_stride}, aA, aA + m, aA + 2 * m);
}
// the gate over the rows k_qap_long filled in, behind it in stream order (a row listed for two matrices is tested twice)
__global__ __launch_bounds__(256) void k_qap_check_rows(const uint32_t *list, uint32_t n_long, const Fr *aABC, size_t m, uint32_t *unsat) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    if (j >= n_long) return;
    const Fr *aA = aABC + (size_t)3 * p * m;
    const uint32_t row = list[j] & 0x3fffffffu;
    if (aA[row] * aA[m + row] != aA[2 * m + row]) or_and_wait(unsat + p);
}
// H_tmp = (aA . aB - aC) * Zinv out of the workspace into the caller's buffer (witness p at h + p * h_stride), and coefficients_for_H[m] = 0:
// the closing icosetFFT then runs in the caller's buffer, no copy follows it
__global__ __launch_bounds__(256) void k_qap_pointwise(const Fr *aABC, size_t m, Fr zinv, Fr *h, size_t h_stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    const Fr *aA = aABC + (size_t)3 * blockIdx.y * m;
    Fr *out = h + (size_t)blockIdx.y * h_stride;
    out[i] = (i == m ? Fr::zero() : (aA[i] * aA[m + i] - aA[2 * m + i]) * zinv).normalized();
}
// the same on a step_radix2_domain: Z(g x_i) takes big / small distinct values on the first big points and one on the rest (k_pointwise_h_step)
__global__ __launch_bounds__(256) void k_qap_pointwise_step(const Fr *aABC, size_t m, size_t big, const Fr *zinv, uint32_t period_mask, Fr zinv_small, Fr *h, size_t h_stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    const Fr *aA = aABC + (size_t)3 * blockIdx.y * m;
    Fr *out = h + (size_t)blockIdx.y * h_stride;
    if (i == m) { out[i] = Fr::zero().normalized(); return; }
    const Fr zi = i < big ? zinv[i & period_mask] : zinv_small;
    out[i] = ((aA[i] * aA[m + i] - aA[2 * m + i]) * zi).normalized();
}

// ---- the instance map (zkg_qap_instance_async): At | Bt | Ct = the columns of A, B, C against u = the Lagrange coefficients at t, a transposed
//      sparse mat-vec.  The handle holds the matrices by rows (CSR); the column-major index below is built from them on the device, once, by the
//      first instance call: per matrix n + 2 column pointers and, per entry, (row, position of the coefficient in the CSR val) — the 32-byte
//      values are not copied.  Degree count with atomics, exclusive scan, scatter through per-column cursors: the order of the entries inside a
//      column is whatever the atomics give, and the sums, exact in Fr and fully reduced on the way out, do not depend on it.
static constexpr uint32_t LONG_COLUMN = 24;          // columns above this many terms go one wavefront per segment (include/zkg.h names the number)
static constexpr uint32_t COLUMN_SEGMENT = 2048;     // terms per segment of such a column: 32 per lane
static constexpr uint32_t COLUMN_SEGMENT_MIN = 64;   // zkg_qap_set_column_segment: one term per lane at the least
struct ColSeg { uint32_t key /* matrix << 30 | column */, lo, hi /* entries [lo, hi) of the matrix's index */, nseg /* on a column's first segment: how many it has; else 0 */; };
struct QapCsc { const uint32_t *a_cp; const uint2 *a_ent; const Fr *a_val; const uint32_t *b_cp; const uint2 *b_ent; const Fr *b_val; const uint32_t *c_cp; const uint2 *c_ent; const Fr *c_val; };
template <class T> ZK_D T pick3(uint32_t k, T a, T b, T c) { return k == 0 ? a : k == 1 ? b : c; }

// one lane per row of matrix blockIdx.y: the degree of every column it touches
__global__ __launch_bounds__(256) void k_col_count(QapCsr M, uint32_t C, uint32_t *cnt_a, uint32_t *cnt_b, uint32_t *cnt_c) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= C) return;
    const uint32_t *rp = pick3(k, M.a_rp, M.b_rp, M.c_rp), *col = pick3(k, M.a_col, M.b_col, M.c_col);
    uint32_t *cnt = pick3(k, cnt_a, cnt_b, cnt_c);
    for (uint32_t e = rp[i]; e < rp[i + 1]; ++e) atomicAdd(cnt + col[e], 1u);
}
// one workgroup per matrix: cnt[0, cols) -> its exclusive prefix sums, in place and into the cursors, and the total at cnt[cols].  Every lane
// owns a run of consecutive columns; the 1024 run sums are scanned in LDS
__global__ __launch_bounds__(1024) void k_col_scan(uint32_t *cnt_a, uint32_t *cnt_b, uint32_t *cnt_c, uint32_t *cur, size_t cols) {
    __shared__ uint32_t sums[1024];
    const uint32_t tid = threadIdx.x, k = blockIdx.x;
    uint32_t *cnt = pick3(k, cnt_a, cnt_b, cnt_c);
    cur += k * cols;
    const size_t per = (cols + 1023) / 1024, lo = std::min((size_t)tid * per, cols), hi = std::min(lo + per, cols);
    uint32_t own = 0;
    for (size_t j = lo; j < hi; ++j) own += cnt[j];
    sums[tid] = own;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint32_t v = tid >= d ? sums[tid - d] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    uint32_t run = sums[tid] - own;
    for (size_t j = lo; j < hi; ++j) { const uint32_t c = cnt[j]; cnt[j] = run; cur[j] = run; run += c; }
    if (tid == 1023) cnt[cols] = sums[1023];
}
// the rows again: every entry takes the next place of its column
__global__ __launch_bounds__(256) void k_col_scatter(QapCsr M, uint32_t C, uint32_t *cur, size_t cols, uint2 *ent_a, uint2 *ent_b, uint2 *ent_c) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= C) return;
    const uint32_t *rp = pick3(k, M.a_rp, M.b_rp, M.c_rp), *col = pick3(k, M.a_col, M.b_col, M.c_col);
    uint2 *ent = pick3(k, ent_a, ent_b, ent_c);
    cur += k * cols;
    for (uint32_t e = rp[i]; e < rp[i + 1]; ++e) ent[atomicAdd(cur + col[e], 1u)] = make_uint2(i, e);
}
// the list of the long columns' segments: a column above LONG_COLUMN terms takes ceil(degree / seg) consecutive entries (`counter` hands them
// out: the list's order is the atomics' too).  Entry e's partial sum is partial e, a column's partials lie side by side.
__global__ __launch_bounds__(256) void k_col_segments(const uint32_t *cp_a, const uint32_t *cp_b, const uint32_t *cp_c, size_t cols, uint32_t seg, ColSeg *list, uint32_t cap, uint32_t *counter) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; const uint32_t k = blockIdx.y;
    if (j >= cols) return;
    const uint32_t *cp = pick3(k, cp_a, cp_b, cp_c);
    const uint32_t lo = cp[j], hi = cp[j + 1];
    if (hi - lo <= LONG_COLUMN) return;
    const uint32_t nseg = (hi - lo + seg - 1) / seg, base = atomicAdd(counter, nseg);
    for (uint32_t s = 0; s < nseg && base + s < cap; ++s)
        list[base + s] = ColSeg{(k << 30) | (uint32_t)j, lo + s * seg, std::min(lo + (s + 1) * seg, hi), s == 0 ? nseg : 0u};
}

ZK_D Fr wave_sum(Fr acc) {                            // the shuffle reduction of r1cs_long_entry: every lane ends with the wavefront's sum
    for (int d = 32; d >= 1; d >>= 1) {
        Fr o;
        for (int j = 0; j < 8; ++j) o.v[j] = __shfl_xor(acc.v[j], d, 64);
        acc += o;
    }
    return acc;
}
// one lane per column of matrix blockIdx.y (vector k at abc + k * stride); the columns above LONG_COLUMN terms are k_qap_columns_close's.  The
// input-consistency rows C .. C + l of A (one term each, u[C + j] into column j) are added here, not by a pass of their own.
__global__ __launch_bounds__(256) void k_qap_columns(QapCsc M, const Fr *u, size_t cols, uint32_t C, uint32_t l, Fr *abc, size_t stride) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; const uint32_t k = blockIdx.y;
    if (j >= cols) return;
    const uint32_t *cp = pick3(k, M.a_cp, M.b_cp, M.c_cp); const uint2 *ent = pick3(k, M.a_ent, M.b_ent, M.c_ent); const Fr *val = pick3(k, M.a_val, M.b_val, M.c_val);
    const uint32_t lo = cp[j], hi = cp[j + 1];
    if (hi - lo > LONG_COLUMN) return;
    Fr acc = (k == 0 && j <= l) ? u[C + j] : Fr::zero();
    for (uint32_t e = lo; e < hi; ++e) { const uint2 t = ent[e]; acc += val[t.y] * u[t.x]; }
    abc[k * stride + j] = acc.normalized();
}
// one wavefront per segment: lanes stride over its terms
__global__ __launch_bounds__(256) void k_qap_columns_long(const ColSeg *list, uint32_t n_seg, QapCsc M, const Fr *u, Fr *part) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_seg) return;
    const ColSeg g = list[wave]; const uint32_t k = g.key >> 30;
    const uint2 *ent = pick3(k, M.a_ent, M.b_ent, M.c_ent); const Fr *val = pick3(k, M.a_val, M.b_val, M.c_val);
    Fr acc = Fr::zero();
    for (uint32_t e = g.lo + lane; e < g.hi; e += 64) { const uint2 t = ent[e]; acc += val[t.y] * u[t.x]; }
    acc = wave_sum(acc);
    if (lane == 0) part[wave] = acc.normalized();
}
// the closing launch: one wavefront per long column (the list entry of its first segment) sums the column's partials, so no chain grows with
// the column; the entries of later segments have nothing to do
__global__ __launch_bounds__(256) void k_qap_columns_close(const ColSeg *list, uint32_t n_seg, const Fr *part, const Fr *u, uint32_t C, uint32_t l, Fr *abc, size_t stride) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_seg) return;
    const ColSeg g = list[wave];
    if (!g.nseg) return;
    Fr acc = Fr::zero();
    for (uint32_t s = lane; s < g.nseg; s += 64) acc += part[wave + s];
    acc = wave_sum(acc);
    const uint32_t k = g.key >> 30, j = g.key & 0x3fffffffu;
    if (lane != 0) return;
    if (k == 0 && j <= l) acc += u[C + j];
    abc[k * stride + j] = acc.normalized();
}

static constexpr size_t QAP_WORKSPACE_CAP = (size_t)1 << 30;                   // one launch group's workspace stays at or under this (one witness is always taken)
static constexpr size_t QAP_BYTES_PER_ELEMENT = 3 * sizeof(Fr) + 3 * NTT_SCRATCH_BYTES;   // aA | aB | aC and the scratch of their three transforms: 216
static constexpr size_t QAP_MAX_GROUP = 65535 / 3;                              // grid.y of the batched transforms carries 3 g vectors

}  // namespace zk

using namespace zk;

struct zkg_qap {
    DomainShape sh; int device = 0; std::mutex mu;
    uint32_t n = 0, l = 0, C = 0;
    DevBuf rp[3], col[3], val[3];
    DevBuf long_rows; uint32_t n_long = 0;          // (matrix << 30 | row) of every row with more than LONG_ROW terms
    DevBuf coset_over_m, coset_over_m29;            // g^i / m and its 29-bit records (radix-2 domains: iFFT's scaling fused with the cosetFFT's)
    Fr z_inv_coset;                                 // 1 / (g^m - 1) (radix-2 domains)
    DevBuf ws;                                      // a group's aA | aB | aC (3 g m Fr), then the transforms' scratch (3 g m records of 40 bytes)
    HandleOrder order;                              // its calls run in call order whatever streams they name (common.hpp)
    size_t bmax_default = 1, bmax = 1;
    // the instance map's column index, made by the first zkg_qap_instance_async: column pointers (n + 2) and (row, position in val) per entry
    size_t nnz[3] = {0, 0, 0};
    DevBuf cp[3], ent[3], seg_list, seg_counter; bool indexed = false;
    uint32_t seg_len = COLUMN_SEGMENT, seg_built = 0, n_seg = 0;   // the list holds n_seg segments of at most seg_built terms
    void release() {
        for (DevBuf *b : {&rp[0], &rp[1], &rp[2], &col[0], &col[1], &col[2], &val[0], &val[1], &val[2], &long_rows, &coset_over_m, &coset_over_m29, &ws,
                          &cp[0], &cp[1], &cp[2], &ent[0], &ent[1], &ent[2], &seg_list, &seg_counter}) b->release();
    }
};

static thread_local size_t t_qap_stats[3];
static thread_local size_t t_qap_instance_stats[2];

static int qap_upload(DevBuf &d, const void *src, size_t bytes) {
    if (d.reserve(bytes ? bytes : 16)) return ZKG_ERROR;
    if (bytes && !hip_ok(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__)) return ZKG_ERROR;
    return ZKG_OK;
}
static void qap_destroy(zkg_qap *q) {
    int cur = 0; (void)hipGetDevice(&cur);
    if (cur != q->device) (void)hipSetDevice(q->device);               // the buffers and the event live on the handle's device
    q->order.destroy();
    q->release();
    if (cur != q->device) (void)hipSetDevice(cur);
    delete q;
}
static zkg_qap *qap_new_impl(const zkg_r1cs *cs) {
    static const char *who = "zkg_qap_new";
    auto refuse = [&](const char *why) { set_error(std::string(who) + ": " + why); return (zkg_qap *)nullptr; };
    const int dev = initialised_device();
    if (dev < 0) { set_error("zkg_init not called"); return nullptr; }
    if (!cs) return refuse("null constraint system");
    const uint32_t n = cs->num_variables, l = cs->num_inputs, C = cs->num_constraints;
    if (!C || !n) return refuse("a system without constraints or without variables");
    if (l > n) return refuse("num_inputs exceeds num_variables");
    DomainShape sh;
    if (!evaluation_domain_shape((size_t)C + l + 1, sh)) return refuse("no radix-2 or step domain for C + l + 1 (get_evaluation_domain would fail)");
    const uint32_t *rps[3] = {cs->a_rowptr, cs->b_rowptr, cs->c_rowptr}, *cols[3] = {cs->a_col, cs->b_col, cs->c_col};
    const uint64_t *vals[3] = {cs->a_val, cs->b_val, cs->c_val};
    // the host check, once: the kernels walk the rows by these pointers and index z by these columns
    std::vector<uint32_t> lr;
    for (uint32_t mtx = 0; mtx < 3; ++mtx) {
        const uint32_t *rp = rps[mtx];
        if (!rp) return refuse("null CSR");
        if (rp[0] != 0) return refuse("a row pointer does not start at 0");
        for (uint32_t r = 0; r < C; ++r) {
            if (rp[r + 1] < rp[r]) return refuse("a row pointer decreases");
            if (rp[r + 1] - rp[r] > LONG_ROW) lr.push_back((mtx << 30) | r);
        }
        const size_t nnz = rp[C];
        if (nnz && (!cols[mtx] || !vals[mtx])) return refuse("null CSR");
        for (size_t k = 0; k < nnz; ++k) if (cols[mtx][k] > n) return refuse("a column index exceeds num_variables");
    }
    if (wrong_device_refused(who, dev, "zkg_init selected (the domain tables live there)")) return nullptr;
    std::unique_ptr<zkg_qap, void (*)(zkg_qap *)> q(new zkg_qap(), qap_destroy);
    q->sh = sh; q->device = dev; q->n = n; q->l = l; q->C = C;
    const size_t m = sh.m;
    q->bmax_default = q->bmax = std::max<size_t>(1, std::min(QAP_MAX_GROUP, QAP_WORKSPACE_CAP / (m * QAP_BYTES_PER_ELEMENT)));
    for (uint32_t mtx = 0; mtx < 3; ++mtx) {
        const size_t nnz = rps[mtx][C];
        q->nnz[mtx] = nnz;
        if (qap_upload(q->rp[mtx], rps[mtx], ((size_t)C + 1) * 4) || qap_upload(q->col[mtx], cols[mtx], nnz * 4) || qap_upload(q->val[mtx], vals[mtx], nnz * 32)) return nullptr;
    }
    q->n_long = (uint32_t)lr.size();
    if (qap_upload(q->long_rows, lr.data(), lr.size() * 4)) return nullptr;
    // the tables are built here, on the null stream, and waited for: no later call finds them missing or half made
    if (sh.step) {
        if (!step_domain(m, nullptr)) return nullptr;
    } else {
        NttDomain *nd = ntt_domain(sh.log_m, nullptr);
        if (!nd) return nullptr;
        const Fr g = Fr::from_u64(5);
        q->z_inv_coset = (g.pow_u64(m) - Fr::one()).inverse();           // basic_radix2_domain::divide_by_Z_on_coset
        if (q->coset_over_m.reserve(m * sizeof(Fr)) || powers_table(q->coset_over_m.as<Fr>(), m, g, nd->n_inv, nullptr) ||
            ntt_table29(q->coset_over_m29, q->coset_over_m.as<Fr>(), m, nullptr)) return nullptr;
    }
    if (!hip_ok(hipStreamSynchronize(nullptr), "hipStreamSynchronize", __FILE__, __LINE__) || q->order.create()) return nullptr;
    return q.release();
}

static bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}
static int qap_witness_h_async_impl(zkg_qap *q, const void *d_witnesses, size_t stride, size_t count, void *d_h, size_t h_stride, uint32_t *d_unsat, void *stream) {
    static const char *who = "zkg_qap_witness_h_async";
    for (size_t &v : t_qap_stats) v = 0;
    if (count == 0) return ZKG_OK;                                      // nothing to do, nothing touched
    if (initialised_device() < 0) { set_error("zkg_init not called"); return ZKG_ERROR; }
    if (!q || !d_witnesses || !d_h) { set_error(std::string(who) + ": bad argument (null handle or pointer)"); return ZKG_ERROR; }
    const size_t n = q->n, m = q->sh.m;
    if (h_stride < m + 1) { set_error(std::string(who) + ": h_stride must be at least m + 1"); return ZKG_ERROR; }
    if (async_vectors_refused(who, n, "n", stride, count, q->device, "the handle was made on") ||
        async_vectors_refused(who, m + 1, "m + 1", h_stride, count, q->device, "the handle was made on")) return ZKG_ERROR;
    const size_t w_bytes = ((count - 1) * stride + n) * 32, h_bytes = ((count - 1) * h_stride + m + 1) * 32, u_bytes = count * 4;
    if (dev_range_refused(d_witnesses, w_bytes, 16, q->device, who, "d_witnesses", "handle") || dev_range_refused(d_h, h_bytes, 16, q->device, who, "d_h", "handle") ||
        (d_unsat && dev_range_refused(d_unsat, u_bytes, 4, q->device, who, "d_unsat", "handle"))) return ZKG_ERROR;
    if (ranges_overlap(d_witnesses, w_bytes, d_h, h_bytes) ||
        (d_unsat && (ranges_overlap(d_unsat, u_bytes, d_witnesses, w_bytes) || ranges_overlap(d_unsat, u_bytes, d_h, h_bytes)))) {
        set_error(std::string(who) + ": the input and output ranges overlap"); return ZKG_ERROR;
    }
    size_t stats[3] = {0, 0, 0};
    const int rc = zk::qap_witness_h_enqueue(q, d_witnesses, stride, count, d_h, h_stride, d_unsat, (hipStream_t)stream, stats);
    for (int i = 0; i < 3; ++i) t_qap_stats[i] = stats[i];
    return rc;
}
// The launch sequence alone, for arguments that have been checked: zkg_qap_witness_h_async behind its refusals, and the prover handle
// (prove_async.hip) on buffers of its own.  stats: witnesses enqueued, launch groups, host waits; no thread-local counter is touched.
int zk::qap_witness_h_enqueue(zkg_qap *q, const void *d_witnesses, size_t stride, size_t count, void *d_h, size_t h_stride, uint32_t *d_unsat, hipStream_t s, size_t stats[3]) {
    static const char *who = "zkg_qap_witness_h_async";
    const size_t m = q->sh.m, u_bytes = count * 4;
    std::lock_guard<std::mutex> lk(q->mu);                              // held for the enqueue only
    NttDomain *nd = nullptr; StepDomain *sd = nullptr;                  // looked up per call (a map find): zkg_shutdown releases them under a live handle
    if (q->sh.step) sd = step_domain(m, s); else nd = ntt_domain(q->sh.log_m, s);
    if (!nd && !sd) return ZKG_ERROR;
    size_t waits = 0, groups = 0, done = 0;
    // the workspace of the call's largest group.  Growing it frees it: earlier calls may still be in it, so the handle's event is waited for first
    const size_t need = std::min(q->bmax, count) * m * QAP_BYTES_PER_ELEMENT;
    if (q->order.grow(q->ws, need, waits) || q->order.order_behind(s)) return ZKG_ERROR;
    const QapCsr M = {q->rp[0].as<uint32_t>(), q->col[0].as<uint32_t>(), q->val[0].as<Fr>(), q->rp[1].as<uint32_t>(), q->col[1].as<uint32_t>(), q->val[1].as<Fr>(),
                      q->rp[2].as<uint32_t>(), q->col[2].as<uint32_t>(), q->val[2].as<Fr>()};
    const Fr *w = (const Fr *)d_witnesses; Fr *h = (Fr *)d_h;
    const unsigned grid_m = (unsigned)((m + 255) / 256), grid_h = (unsigned)((m + 1 + 255) / 256);
    bool enqueued = false;
    int rc = ZKG_OK;
    if (d_unsat) { rc = hip_ok(hipMemsetAsync(d_unsat, 0, u_bytes, s), "hipMemsetAsync", __FILE__, __LINE__) ? ZKG_OK : ZKG_ERROR; enqueued = rc == ZKG_OK; }
    while (done < count && rc == ZKG_OK) {
        const unsigned g = (unsigned)std::min(q->bmax, count - done);
        Fr *aABC = q->ws.as<Fr>(), *scr = aABC + (size_t)3 * g * m;
        const Fr *wg = w + done * stride; Fr *hg = h + done * h_stride;
        uint32_t *ug = d_unsat ? d_unsat + done : nullptr;
        const hipEvent_t ev = done + g == count ? q->order.ev : nullptr;     // the call's last group ends in the handle's event
        enqueued = true;
        hipLaunchKernelGGL(k_qap_eval, dim3(grid_m, g), dim3(256), 0, s, M, wg, stride, q->C, q->l, m, aABC, ug);
        if (q->n_long) {
            hipLaunchKernelGGL(k_qap_long, dim3((q->n_long + 3) / 4, g), dim3(256), 0, s, q->long_rows.as<uint32_t>(), q->n_long, M, wg, stride, m, aABC);
            if (ug) hipLaunchKernelGGL(k_qap_check_rows, dim3((q->n_long + 255) / 256, g), dim3(256), 0, s, q->long_rows.as<uint32_t>(), q->n_long, (const Fr *)aABC, m, ug);
        }
        if (hipGetLastError() != hipSuccess) { set_error(std::string(who) + ": kernel launch failed"); rc = ZKG_ERROR; break; }
        // the transforms as batches of 3 g and g vectors (witness p's aA | aB | aC are vectors 3 p .. 3 p + 2), the sequence of the prover's chunk
        if (nd) {
            rc = ntt_run_ex(nd, aABC, true, nullptr, q->coset_over_m.as<Fr>(), nullptr, s, scr, 3 * g, 0, nullptr, q->coset_over_m29.p);   // iFFT x 3 g, g^i / m fused
            if (rc == ZKG_OK) rc = ntt_run_ex(nd, aABC, false, nullptr, nullptr, nullptr, s, scr, 3 * g);                                  // the cosetFFT's transform
            if (rc != ZKG_OK) break;
            hipLaunchKernelGGL(k_qap_pointwise, dim3(grid_h, g), dim3(256), 0, s, (const Fr *)aABC, m, q->z_inv_coset, hg, h_stride);
            rc = ntt_run_ex(nd, hg, true, nullptr, nd->icoset_post.as<Fr>(), nullptr, s, scr, g, h_stride, nullptr, nullptr, m, ev);       // icosetFFT x g, in the caller's buffer
        } else {
            rc = step_ntt_run(sd, aABC, true, false, s, scr, 3 * g, m);                                                                    // iFFT x 3 g
            if (rc == ZKG_OK) rc = step_ntt_run(sd, aABC, false, true, s, scr, 3 * g, m);                                                  // cosetFFT x 3 g
            if (rc != ZKG_OK) break;
            hipLaunchKernelGGL(k_qap_pointwise_step, dim3(grid_h, g), dim3(256), 0, s, (const Fr *)aABC, m, sd->shape.big, sd->zinv.as<Fr>(),
                               (uint32_t)(sd->shape.big / sd->shape.small - 1), sd->zinv_small, hg, h_stride);
            rc = step_ntt_run(sd, hg, true, true, s, scr, g, h_stride, m, ev);                                                             // icosetFFT x g
        }
        if (rc == ZKG_OK && hipGetLastError() != hipSuccess) { set_error(std::string(who) + ": kernel launch failed"); rc = ZKG_ERROR; }
        if (rc == ZKG_OK) { done += g; ++groups; }
    }
    stats[0] = done; stats[1] = groups; stats[2] = waits;
    if (rc == ZKG_OK) { q->order.carried(s); return ZKG_OK; }
    if (enqueued) q->order.record(s);                                   // a failure: what was enqueued before it still runs
    return ZKG_ERROR;
}

// The column index and the segment list, on s, under the handle's mutex.  The first call builds both and waits for them once (the list's length
// comes back with that wait); a call after zkg_qap_set_column_segment rebuilds the list alone, behind the handle's pending work (which reads it).
static int qap_index(zkg_qap *q, hipStream_t s, size_t &builds, size_t &waits) {
    static const char *who = "zkg_qap_instance_async";
    if (q->indexed && q->seg_built == q->seg_len) return ZKG_OK;
    const size_t cols = (size_t)q->n + 1; const uint32_t C = q->C;
    const QapCsr M = {q->rp[0].as<uint32_t>(), q->col[0].as<uint32_t>(), q->val[0].as<Fr>(), q->rp[1].as<uint32_t>(), q->col[1].as<uint32_t>(), q->val[1].as<Fr>(),
                      q->rp[2].as<uint32_t>(), q->col[2].as<uint32_t>(), q->val[2].as<Fr>()};
    ScopedDevBuf cur;                                                   // the scatter's cursors: gone after the wait below
    const bool build = !q->indexed;
    if (build) {
        if (cur.reserve(3 * cols * 4) || q->seg_counter.reserve(4)) return ZKG_ERROR;
        for (int k = 0; k < 3; ++k) {
            if (q->cp[k].reserve((cols + 1) * 4) || q->ent[k].reserve(std::max<size_t>(q->nnz[k], 1) * sizeof(uint2))) return ZKG_ERROR;
            ZK_HIP(hipMemsetAsync(q->cp[k].p, 0, (cols + 1) * 4, s));
        }
        const dim3 rows((C + 255) / 256, 3);
        hipLaunchKernelGGL(k_col_count, rows, dim3(256), 0, s, M, C, q->cp[0].as<uint32_t>(), q->cp[1].as<uint32_t>(), q->cp[2].as<uint32_t>());
        hipLaunchKernelGGL(k_col_scan, dim3(3), dim3(1024), 0, s, q->cp[0].as<uint32_t>(), q->cp[1].as<uint32_t>(), q->cp[2].as<uint32_t>(), cur.as<uint32_t>(), cols);
        hipLaunchKernelGGL(k_col_scatter, rows, dim3(256), 0, s, M, C, cur.as<uint32_t>(), cols, q->ent[0].as<uint2>(), q->ent[1].as<uint2>(), q->ent[2].as<uint2>());
    } else if (q->order.wait_host()) {
        return ZKG_ERROR;
    }
    // a long column has more than LONG_COLUMN terms and ceil(degree / seg) <= degree / seg + 1 segments
    size_t cap = 0;
    for (int k = 0; k < 3; ++k) cap += q->nnz[k] / (LONG_COLUMN + 1) + q->nnz[k] / q->seg_len;
    if (cap >= ((size_t)1 << 31)) { set_error(std::string(who) + ": too many column segments"); return ZKG_ERROR; }
    uint32_t n_seg = 0;
    if (q->seg_list.reserve(std::max<size_t>(cap, 1) * sizeof(ColSeg))) return ZKG_ERROR;
    ZK_HIP(hipMemsetAsync(q->seg_counter.p, 0, 4, s));
    hipLaunchKernelGGL(k_col_segments, dim3((unsigned)((cols + 255) / 256), 3), dim3(256), 0, s, q->cp[0].as<uint32_t>(), q->cp[1].as<uint32_t>(), q->cp[2].as<uint32_t>(), cols,
                       q->seg_len, q->seg_list.as<ColSeg>(), (uint32_t)cap, q->seg_counter.as<uint32_t>());
    if (hipGetLastError() != hipSuccess) { set_error(std::string(who) + ": kernel launch failed"); (void)hipStreamSynchronize(s); return ZKG_ERROR; }
    const bool landed = hip_ok(hipMemcpyAsync(&n_seg, q->seg_counter.p, 4, hipMemcpyDeviceToHost, s), "D2H", __FILE__, __LINE__);
    if (!hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize", __FILE__, __LINE__) || !landed) return ZKG_ERROR;   // the cursors are freed behind this
    ++waits;
    if (n_seg > cap) { set_error(std::string(who) + ": the segment list overran its bound"); return ZKG_ERROR; }
    if (build) { q->indexed = true; ++builds; }
    q->n_seg = n_seg; q->seg_built = q->seg_len;
    return ZKG_OK;
}
static int qap_instance_async_impl(zkg_qap *q, const uint64_t *t, void *d_abc, size_t stride, void *d_z, void *stream) {
    static const char *who = "zkg_qap_instance_async";
    for (size_t &v : t_qap_instance_stats) v = 0;
    if (initialised_device() < 0) { set_error("zkg_init not called"); return ZKG_ERROR; }
    if (!q || !t || !d_abc) { set_error(std::string(who) + ": bad argument (null handle or pointer)"); return ZKG_ERROR; }
    const size_t cols = (size_t)q->n + 1, m = q->sh.m;
    if (cols >= ((size_t)1 << 30)) { set_error(std::string(who) + ": too many variables"); return ZKG_ERROR; }
    if (async_vectors_refused(who, cols, "n + 1", stride, 3, q->device, "the handle was made on")) return ZKG_ERROR;
    const size_t abc_bytes = (2 * stride + cols) * 32;
    if (dev_range_refused(d_abc, abc_bytes, 16, q->device, who, "d_abc", "handle") || (d_z && dev_range_refused(d_z, 32, 16, q->device, who, "d_z", "handle"))) return ZKG_ERROR;
    if (d_z && ranges_overlap(d_abc, abc_bytes, d_z, 32)) { set_error(std::string(who) + ": the output ranges overlap"); return ZKG_ERROR; }
    Fr tf; memcpy(tf.v, t, 32);                                         // read now: the caller may reuse t on return
    if (domain_vanishing_at(q->sh, tf).is_zero()) { set_error(std::string(who) + ": t is a domain point (Z(t) = 0)"); return ZKG_ERROR; }
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(q->mu);                              // held for the enqueue (and the first call's one wait)
    size_t builds = 0, waits = 0;
    auto leave = [&](int rc) { t_qap_instance_stats[0] = builds; t_qap_instance_stats[1] = waits; return rc; };
    if (qap_index(q, s, builds, waits)) return leave(ZKG_ERROR);
    // u (m Fr), then the segments' partial sums, in the workspace the H calls use: grown and ordered by their rules
    const size_t need = (m + q->n_seg) * sizeof(Fr);
    if (q->order.grow(q->ws, need, waits) || q->order.order_behind(s)) return leave(ZKG_ERROR);
    Fr *u = q->ws.as<Fr>(), *part = u + m, *abc = (Fr *)d_abc;
    if (domain_lagrange_dev(q->sh, tf, u, (Fr *)d_z, s)) return leave(ZKG_ERROR);
    const QapCsc M = {q->cp[0].as<uint32_t>(), q->ent[0].as<uint2>(), q->val[0].as<Fr>(), q->cp[1].as<uint32_t>(), q->ent[1].as<uint2>(), q->val[1].as<Fr>(),
                      q->cp[2].as<uint32_t>(), q->ent[2].as<uint2>(), q->val[2].as<Fr>()};
    hipLaunchKernelGGL(k_qap_columns, dim3((unsigned)((cols + 255) / 256), 3), dim3(256), 0, s, M, (const Fr *)u, cols, q->C, q->l, abc, stride);
    if (q->n_seg) {
        const dim3 waves((q->n_seg + 3) / 4);
        hipLaunchKernelGGL(k_qap_columns_long, waves, dim3(256), 0, s, q->seg_list.as<ColSeg>(), q->n_seg, M, (const Fr *)u, part);
        hipLaunchKernelGGL(k_qap_columns_close, waves, dim3(256), 0, s, q->seg_list.as<ColSeg>(), q->n_seg, (const Fr *)part, (const Fr *)u, q->C, q->l, abc, stride);
    }
    const bool launched = hipGetLastError() == hipSuccess;
    q->order.record(s);                                                 // whatever was enqueued still runs
    if (!launched) { set_error(std::string(who) + ": kernel launch failed"); return leave(ZKG_ERROR); }
    return leave(ZKG_OK);
}

extern "C" {

zkg_qap *zkg_qap_new(const zkg_r1cs *cs) { return c_boundary<zkg_qap *>("zkg_qap_new", nullptr, [&] { return qap_new_impl(cs); }); }
void zkg_qap_free(zkg_qap *q) {
    if (!q) return;
    c_boundary("zkg_qap_free", 0, [&] { qap_destroy(q); return 0; });
}
size_t zkg_qap_domain_size(const zkg_qap *q) { return q ? q->sh.m : 0; }
uint32_t zkg_qap_num_variables(const zkg_qap *q) { return q ? q->n : 0; }
size_t zkg_qap_batch_max(const zkg_qap *q) { return q ? q->bmax : 0; }
void zkg_qap_set_batch_max(zkg_qap *q, size_t k) {
    if (!q) return;
    c_boundary("zkg_qap_set_batch_max", 0, [&] { std::lock_guard<std::mutex> lk(q->mu); q->bmax = clamp_batch_max(k, q->bmax_default); return 0; });
}
int zkg_qap_witness_h_async(zkg_qap *q, const void *d_witnesses, size_t stride, size_t count, void *d_h, size_t h_stride, uint32_t *d_unsat, void *stream) {
    return c_boundary("zkg_qap_witness_h_async", ZKG_ERROR, [&] { return qap_witness_h_async_impl(q, d_witnesses, stride, count, d_h, h_stride, d_unsat, stream); });
}
void zkg_qap_stats(size_t out[3]) { if (out) for (int i = 0; i < 3; ++i) out[i] = t_qap_stats[i]; }
int zkg_qap_instance_async(zkg_qap *q, const uint64_t t[4], void *d_abc, size_t stride, void *d_z, void *stream) {
    return c_boundary("zkg_qap_instance_async", ZKG_ERROR, [&] { return qap_instance_async_impl(q, t, d_abc, stride, d_z, stream); });
}
void zkg_qap_set_column_segment(zkg_qap *q, size_t k) {
    if (!q) return;
    c_boundary("zkg_qap_set_column_segment", 0, [&] {
        std::lock_guard<std::mutex> lk(q->mu);
        q->seg_len = k == 0 ? COLUMN_SEGMENT : (uint32_t)std::min<size_t>(std::max<size_t>(k, COLUMN_SEGMENT_MIN), (size_t)1 << 20);
        return 0;
    });
}
void zkg_qap_instance_stats(size_t out[2]) { if (out) for (int i = 0; i < 2; ++i) out[i] = t_qap_instance_stats[i]; }

}  // extern "C"
