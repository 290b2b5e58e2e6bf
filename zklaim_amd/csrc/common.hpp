// common.hpp — host-side plumbing shared by the HIP translation units of libzkg.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include <functional>
#include <map>
#include <mutex>
#include "curve.hip.hpp"
#include "c_boundary.hpp"                // set_error, c_boundary

struct zklaim_ctx;                       // include/zklaim_abi.h

namespace zk {

bool hip_ok(hipError_t e, const char *what, const char *file, int line);
#define ZK_HIP(expr) do { if (!::zk::hip_ok((expr), #expr, __FILE__, __LINE__)) return ZKG_ERROR; } while (0)
#define ZK_HIP_V(expr) do { if (!::zk::hip_ok((expr), #expr, __FILE__, __LINE__)) return; } while (0)

// grow-only device buffer (workspaces are allocated outside the timed path and reused)
struct DevBuf {
    void *p = nullptr; size_t cap = 0;
    int reserve(size_t bytes);
    void release();
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// While one is alive on a thread, every DevBuf::reserve of that thread that has to GROW (free and reallocate) first waits for `stream`: for
// workspaces that asynchronous work queued on that stream may still read (zkg_msm_g1_resident_async).  drains counts those waits.
struct ReserveGuard;
extern thread_local ReserveGuard *t_reserve_guard;
struct ReserveGuard {
    hipStream_t stream; size_t drains = 0; ReserveGuard *prev;
    explicit ReserveGuard(hipStream_t s) : stream(s), prev(t_reserve_guard) { t_reserve_guard = this; }
    ReserveGuard(const ReserveGuard &) = delete;
    ReserveGuard &operator=(const ReserveGuard &) = delete;
    ~ReserveGuard() { t_reserve_guard = prev; }
};

// a DevBuf that lives for one scope (staging of a key load, of a table build): released on every way out, an exception's included.
// DevBuf itself has no destructor on purpose — resident buffers are members of objects with explicit lifetimes and are copied into caches.
struct ScopedDevBuf : DevBuf {
    ScopedDevBuf() = default;
    ScopedDevBuf(const ScopedDevBuf &) = delete;
    ScopedDevBuf &operator=(const ScopedDevBuf &) = delete;
    ~ScopedDevBuf() { release(); }
};

// The call order of a handle that queues its work on the caller's streams and owns one workspace (zkg_domain, zkg_qap): its calls run in call
// order whatever streams they name.  One event completes with the last call's last kernel; a call on another stream than that one's waits for
// it on the device before anything of its own — that is what keeps two streams out of the one workspace — and the host waits for it before the
// workspace is freed.  Used under the handle's mutex (capi.hip).
struct HandleOrder {
    hipEvent_t ev = nullptr; bool pending = false; hipStream_t last = nullptr;
    int create();
    int order_behind(hipStream_t s);                          // s waits (on the device) for the last call, unless that was on s itself
    int wait_host();                                          // the host waits for the last call
    int grow(DevBuf &ws, size_t need, size_t &waits);         // ws to `need` bytes: growing frees it, so wait_host first; counted in waits
    // The event of a call: its last launch carries ev as its completion (ZK_LAUNCH_DONE, ntt.hip).  Behind a lone transform that costs 2.0 us of
    // device time where a hipEventRecord behind the kernel costs 2.9 and no event nothing (profiles/ntt_batch_time.json, "event_cost"); a
    // device-scope release (hipEventReleaseToDevice) changes neither.  record() is the plain way, for a call that failed after it had enqueued
    // something (that still runs) or whose last launch cannot carry it.
    void carried(hipStream_t s) { pending = true; last = s; }
    void record(hipStream_t s);
    void destroy();                                           // wait_host, then the event goes (on the handle's device)
};
inline size_t clamp_batch_max(size_t k, size_t dflt) { return k == 0 || k > dflt ? dflt : k; }   // zkg_*_set_batch_max: 0 or too many = the default

// HIP-event timing of the dominant kernel (bench.py's roofline.achieved), on the launch stream
struct KernelTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs; size_t used = 0; bool enabled = true, pending = false;
    // The two event records around a launch are not free on the stream they sit on (traced: the four accumulation launches of a 2^20-point
    // step lose 38 us to them, 2 % of the step), so only every `stride`-th CALL of an entry point is timed — all of its launches, so that the
    // pieces of a piece-wise call weigh what they weigh — and drain() scales the launch count back up (ZKG_KERNEL_TIMER_STRIDE, default 4; 1: all).
    size_t calls = 0, calls_seen = 0, calls_timed = 0; bool sample = true;
    void new_call();                  // an entry point that launches the dominant kernel starts (under its job's mutex)
    void begin(hipStream_t s); void end(hipStream_t s);
    float drain(int *launches);       // average ms per launch over the timed calls since the last reset (synchronises the events); *launches: the
                                      // launches of ALL calls since then (timed launches x calls / timed calls)
    void reset();
};
extern KernelTimer g_dominant_timer;

// small persistent host thread pool (the per-window tails of the MSMs are independent; see msm.hip host_combine)
// host_parallel_for: a caller that finds the pool busy runs its tasks inline (short loops on a proof's latency path);
// host_parallel_for_wait: queues behind the running loop (bulk work that must be parallel: hashing a 200 MB key blob)
void host_parallel_for(int n, const std::function<void(int)> &fn);
void host_parallel_for_wait(int n, const std::function<void(int)> &fn);
void host_parallel_for_spawn(int n, const std::function<void(int)> &fn);   // the pool if it is free, threads of its own if not (heavy loops only)

// ---------------- NTT (ntt.hip) ----------------
struct NttDomain {
    unsigned logn = 0;
    DevBuf tw_fwd, tw_inv;        // omega^i, omega^-i, i < N/2
    DevBuf coset_pre;             // g^i               (cosetFFT pre-multiplication)
    DevBuf icoset_post;           // g^-i / N          (icosetFFT post-multiplication, 1/N folded in)
    DevBuf tw_fwd29, tw_inv29, coset_pre29, icoset_post29;   // the same tables as 40-byte 29-bit records (fr29.hip.hpp), read by k_ntt_pass29
    DevBuf scratch;               // N elements (40-byte records: the 29-bit passes' form between passes)
    Fr n_inv;                     // 1/N
    std::mutex mu; bool first_stream_set = false; hipStream_t first_stream = nullptr;
    std::map<hipStream_t, DevBuf> stream_scratch;
    Fr *scratch_for(hipStream_t s);
    int init(unsigned logn, hipStream_t s);
    void release();
};
NttDomain *ntt_domain(unsigned logn, hipStream_t s);     // cached per size
// mode: inverse / coset as in zkg_ntt.  extra_post (device, N Fr, optional) replaces the default
// post table: the prover fuses iFFT's 1/N with the following cosetFFT's g^i through it.
int ntt_run(NttDomain *d, Fr *d_a, int inverse, int coset, hipStream_t s, Fr *scratch = nullptr, unsigned batch = 1, size_t batch_stride = 0,
            size_t scratch_stride = 0, hipEvent_t done = nullptr);      // the batch arguments of ntt_run_ex (below)
// batch > 1: `batch` vectors, batch_stride elements apart (0 = N: back to back) in d_a and in `scratch` (which must then be given),
// one launch per pass
// pre29 / post29: the 29-bit twins of a caller's own pre / post table (ntt_table29); without them such a call takes the 32-bit pass.
// A caller's scratch holds 40 bytes per element (NTT_SCRATCH_BYTES).  scratch_stride (0 = batch_stride): elements between the vectors' areas in
// `scratch`, for vectors that lie further apart than their scratch has to.  done (optional): an event that completes with the transform's
// last kernel, carried by that launch itself (cheaper on the device than a record behind it).
static constexpr size_t NTT_SCRATCH_BYTES = 40;
int ntt_run_ex(NttDomain *d, Fr *d_a, bool inverse, const Fr *pre, const Fr *post, const Fr *post_scalar, hipStream_t s, Fr *scratch = nullptr,
               unsigned batch = 1, size_t batch_stride = 0, const void *pre29 = nullptr, const void *post29 = nullptr, size_t scratch_stride = 0, hipEvent_t done = nullptr);
int ntt_table29(DevBuf &out, const Fr *d_in, size_t n, hipStream_t s);       // a table in libff's form -> its 29-bit records

// libfqfft get_evaluation_domain(min_size) for min_size <= 2^28: basic_radix2_domain (m = 2^k) or step_radix2_domain (m = big + small,
// big = 2^(ceil_log2(m)-1), small = 2^b < big).  zklaim's circuits land on a step domain for 11 of the 20 payload counts.
struct DomainShape { size_t m = 0, big = 0, small = 0; bool step = false; unsigned log_m = 0; /* ceil(log2 m) */ };
bool evaluation_domain_shape(size_t min_size, DomainShape &d);
bool domain_shape_of(size_t m, DomainShape &d);           // m must be a size the rule maps to itself
Fr fr_root_of_unity_pow2(unsigned logn);                  // libff::get_root_of_unity(2^logn)
// evaluate_all_lagrange_polynomials(t) and compute_vanishing_polynomial(t) of the domain (host, one batched inversion)
int domain_lagrange(const DomainShape &d, const Fr &t, std::vector<Fr> &u, Fr &Zt);
Fr domain_vanishing_at(const DomainShape &d, const Fr &t);    // Z(t) alone, as both of them compute it (host)
// the same values from one kernel queued on s (k_lagrange): d_u (device, m Fr) and, if given, d_z (device, one Fr), canonical limbs.  Z(t) is
// computed on the host first: ZKG_ERROR before any launch when t is a domain point.  No host wait once the domain's tables exist.
int domain_lagrange_dev(const DomainShape &d, const Fr &t, Fr *d_u, Fr *d_z, hipStream_t s, hipEvent_t done = nullptr);   // done: as in ntt_run_ex

// step_radix2_domain on the device: FFT = fold (mod x^big - 1 | x -> omega x, mod x^small - 1) + one radix-2 transform of each size
struct StepDomain {
    DomainShape shape;
    NttDomain *dbig = nullptr, *dsmall = nullptr;
    DevBuf w;                     // omega^i, i < big          (omega = root of unity of order 2 big)
    DevBuf winv_half;             // omega^-i / 2, i < small
    DevBuf g_pow, ginv_pow;       // g^i, g^-i, i < m          (coset variants)
    DevBuf zinv;                  // 1 / Z(g x_i) for i < big: period big/small entries (divide_by_Z_on_coset)
    Fr zinv_small;                // 1 / Z(g x_i), i >= big
    Fr big_inv, small_inv, half;
    int init(const DomainShape &sh, hipStream_t s);
    void release();
};
StepDomain *step_domain(size_t m, hipStream_t s);         // cached per size
// a: batch vectors of m elements, batch_stride apart; scratch: same shape, or scratch_stride (>= m) elements of 40 bytes apart when given
int step_ntt_run(StepDomain *d, Fr *d_a, bool inverse, bool coset, hipStream_t s, Fr *scratch, unsigned batch = 1, size_t batch_stride = 0,
                 size_t scratch_stride = 0, hipEvent_t done = nullptr);
int powers_table(Fr *d_out, size_t n, const Fr &base, const Fr &scale, hipStream_t s);   // out[i] = scale * base^i
void ntt_release_all();
int ntt_configure();

// ---------------- MSM (msm.hip) ----------------
static constexpr int MSM_MAX_SETS = 4;                      // base sets sharing one digit sort (the prover: A, B_g1, L and B_g2 over one witness)
// one base set of a launch.  level_stride > 0: a per-window table (window_table_build_*): level w of the table, at p + w * level_stride
// elements, holds 2^(c w) P_i, so every window shares one bucket set and the host has no doublings left.  index_sub: entry i of the
// scalars stands for element i - index_sub of the set (the L query starts behind the constant and the public inputs); smaller i: no base.
// remap (optional, device): element i of the scalars stands for entry remap[i] of the set — a table that holds only a subset of the key's
// elements (the prover's witness tables cover the non-bit variables only).
// p29 (optional, G1 only): the same points, every level, as the 64-byte packed 29-bit records (Rec64) of fq29.hip.hpp (window_table_records29): a launch of
// this set alone, without gather / remap / index_sub, then accumulates on the 29-bit representation without converting anything per call.
struct MsmBases { const void *p = nullptr; bool g2 = false; size_t level_stride = 0; uint32_t index_sub = 0; const uint32_t *remap = nullptr; const void *p29 = nullptr; };
// CSR matrices A, B, C handed from a circuit to the key generator without a copy
struct OwnedCsr { std::vector<uint32_t> rp[3], col[3]; std::vector<uint64_t> val[3]; };
struct WindowTable { DevBuf buf, rec29; size_t n = 0; int c = 0, W = 0; bool g2 = false; void release() { buf.release(); rec29.release(); n = 0; } };
int window_table_records29(WindowTable &t, hipStream_t s);                // rec29 <- every level of a built G1 table as 29-bit records
int window_table_build_g1(WindowTable &t, const G1Affine *d_bases, size_t n, int c, hipStream_t s);
int table_window_bits(size_t n);                          // window size of a query's table, by the size of the query (prover.hip)
int window_table_build_g2(WindowTable &t, const G2Affine *d_bases, size_t n, int c, hipStream_t s);
struct MsmJob;                                             // one MSM in flight: stream, workspace, pinned landing zone
MsmJob *msm_job_create(hipStream_t s, bool own_stream, bool high_priority = false);
hipStream_t msm_job_stream(MsmJob *j);
void msm_job_set_window_subset(MsmJob *j, uint32_t w0, uint32_t ws);   // the job computes sum over windows w0, w0+ws, ... of 2^(cw) V_w only
void msm_job_set_skewed(MsmJob *j, bool skewed);            // scalars known to be mostly equal (0/1 witness): use the one-pass sort directly
void msm_job_set_row_merge(MsmJob *j, uint32_t f);        // table launches without a gather list: f consecutive windows share a row of buckets (1 = off)
void msm_job_set_window(MsmJob *j, int c);                 // window bits for the next launches (0 = the size-based rule)
void msm_job_set_critical(MsmJob *j, bool critical);   // the job is on its caller's critical path: its accumulate / fold / reduce wavefronts raise their issue priority (crit_wave_priority)
static constexpr unsigned CRIT_PRIORITY_MIN_LOG = 20;     // ... from this domain size on (tools/r4_crit_prio_ab.sh, sparse-witness proofs, off -> on: 37 payloads / 2^20: 3.14 -> 3.07 ms; 20 payloads / 2^19 + 2^18: 2.13 -> 2.16; 8 payloads / 2^18: 1.12 -> 1.23)
bool crit_priority_for(int part, unsigned log_m);        // part 1: matrix-vector + pointwise, 2: transforms, 4: the H job; tuning aids ZKG_CRIT_PRIO_PARTS (mask, default 7), ZKG_CRIT_PRIO_MIN_LOG
bool crit_priority_enabled();                           // ZKG_CRIT_PRIO=0 switches the raised priorities of the critical-path kernels off (A/B)
void msm_job_destroy(MsmJob *j);
// d_gather (optional, n entries): scalar i is d_scalars[d_gather[i]] and stands for element d_gather[i] of every base set
int msm_job_launch(MsmJob *job, const MsmBases *sets, int nsets, const uint32_t *d_scalars, size_t n, bool scalars_mont, const uint32_t *d_gather = nullptr);
int msm_job_finish(MsmJob *job, G1 *out_g1, G2 *out_g2);   // out_g1[k]: k-th G1 set of the launch, out_g2[k]: k-th G2 set
// the dual: `count` scalar vectors of n elements, scalar_stride 32-bit words apart, over the same table sets (all windows, no gather /
// remap / index_sub), as one launch sequence; out_g1[p * (G1 sets) + k] = vector p over the k-th G1 set, out_g2 likewise
bool msm_multi_supported(size_t n, int c, uint32_t count);
static constexpr uint32_t MSM_MULTI_MAX_VECTORS = 16;       // the largest `count` a caller passes: the batched prover's chunk, zkg_msm_g1_resident_batch_max
static constexpr size_t ZKG_MSM_ASYNC_MAX_COUNT = (size_t)1 << 24, ZKG_MSM_ASYNC_MAX_STRIDE = (size_t)1 << 32;   // zkg_msm_g1_resident_async: vectors per call, elements between vectors
int msm_job_launch_multi(MsmJob *job, const MsmBases *sets, int nsets, const uint32_t *d_scalars, size_t n, size_t scalar_stride, uint32_t count, bool scalars_mont);
int msm_job_finish_multi(MsmJob *job, G1 *out_g1, G2 *out_g2);
// The asynchronous end of a TABLE launch of G1 sets, or of G2 sets (not both).  msm_job_set_device_finish(job, true) before the launch: its chunk
// records are not copied to the host.  msm_job_finish_dev then queues the epilogue kernel (k_msm_combine) on the job's stream and
// returns without synchronising: d_out (device, 12 limbs per G1 point, 24 per G2 point, normalised as store_norm writes them) gets point
// (p * sets + k) for vector p and the k-th set.
void msm_job_set_device_finish(MsmJob *j, bool on);
int msm_job_finish_dev(MsmJob *job, uint64_t *d_out);
int msm_combine_records(bool g2, const uint64_t *records_jac, size_t cpw, int slots, int chunk_log, size_t vectors, uint64_t *out_jac);   // zkg_msm_combine_gpu, zkg_msm_combine_g2_gpu (slots 2)
size_t msm_table_bucket_bytes(int c, bool g2);             // bucket workspace of ONE scalar vector of a table launch at window size c (every window's set)
// the multi_exp_with_mixed_addition split of a witness z = [1 | w] (n1 elements, Montgomery): tags (0 zero, 1 one, 2 other), the
// indices of the others and their count; and the flat sum of the bases tagged one (result lands in pinned host memory)
// d_count: two words, [0] the number of listed elements, [1] set to 1 when a listed element has no entry in d_subset_pos (optional: position of
// every element in the subset the witness tables were built for, SUBSET_NONE = absent)
static constexpr uint32_t SUBSET_NONE = 0xffffffffu;
int witness_classify(const Fr *d_z, size_t n1, uint8_t *d_tags, uint32_t *d_listed, uint32_t *d_count, hipStream_t s, const uint32_t *d_subset_pos = nullptr);
// out[j] = idx[j] >= index_sub ? src[idx[j] - index_sub] : infinity   (level 0 of a subset table)
int gather_points_g1(const G1Affine *d_src, const uint32_t *d_idx, size_t count, uint32_t index_sub, G1Affine *d_out, hipStream_t s);
int gather_points_g2(const G2Affine *d_src, const uint32_t *d_idx, size_t count, uint32_t index_sub, G2Affine *d_out, hipStream_t s);
// out[idx[j]] = src[j] (a sparse vector's values into their dense places; out must be zero-filled = all infinity)
int scatter_points_g1(const G1Affine *d_src, const uint32_t *d_idx, size_t count, G1Affine *d_out, hipStream_t s);
int scatter_points_g2(const G2Affine *d_src, const uint32_t *d_idx, size_t count, G2Affine *d_out, hipStream_t s);
struct OnesSum {                                            // results: nsets points (G1 or G2, XYZZ) back to back in pinned host memory
    DevBuf partials; void *host = nullptr; size_t host_bytes = 0; bool g2 = false; int nsets = 0; void release();
    const G1 &g1(int i) const { return reinterpret_cast<const G1 *>(host)[i]; }
    const G2 &g2pt(int i) const { return reinterpret_cast<const G2 *>(host)[i]; }
};
// level 0 of each set (its plain bases) and its index_sub are read; all sets of one field
int ones_sum_launch(OnesSum &o, const MsmBases *sets, int nsets, const uint8_t *d_tags, size_t n1, hipStream_t s);
// `count` witnesses' tag arrays, tag_stride bytes apart, in one launch pair (blockIdx.z = witness): result of witness p, set i at index p * nsets + i
int ones_sum_launch_multi(OnesSum &o, const MsmBases *sets, int nsets, const uint8_t *d_tags, size_t tag_stride, size_t n1, uint32_t count, hipStream_t s);
// scalars: n x 8 u32 (canonical, or Montgomery when scalars_mont).  Zero scalars are dropped and ones land in
// one heavy bucket, which is what libff's multi_exp_with_mixed_addition prefilter achieves.
int msm_g1(const G1Affine *d_bases, const uint32_t *d_scalars, size_t n, bool scalars_mont, G1 *out, hipStream_t s, bool mostly_bits = false);
int msm_g2(const G2Affine *d_bases, const uint32_t *d_scalars, size_t n, bool scalars_mont, G2 *out, hipStream_t s, bool mostly_bits = false);
int msm_g1_host_scalars(const G1Affine *d_bases, const uint32_t *h_scalars, size_t n, bool scalars_mont, G1 *out, hipStream_t s);   // bases resident, scalars uploaded in pieces under the work
int msm_host_scalars_stats(uint32_t *out, int n);         // zkg_msm_host_scalars_stats: the last msm_g1_host_scalars' pieces, heavy counts, heavy launches and stream waits
// one digit/sort pass shared by several base sets (A, B_g1, B_g2 queries use the same scalars)
int msm_shared(const G1Affine *const *d_g1_bases, int n_g1, const G2Affine *d_g2_bases, const uint32_t *d_scalars, size_t n,
               bool scalars_mont, G1 *out_g1, G2 *out_g2, hipStream_t s, uint32_t w0 = 0, uint32_t ws = 1,   // w0, ws: window subset (see MsmGeom)
               bool mostly_bits = false);                 // the multi_exp_with_mixed_addition case: scalars mostly 0/1 -> one-pass sort
int fixed_base_g1(const G1Affine &base, const uint32_t *d_scalars, size_t n, G1Affine *d_out, hipStream_t s, bool scalars_mont = false);
int fixed_base_g2(const G2Affine &base, const uint32_t *d_scalars, size_t n, G2Affine *d_out, hipStream_t s, bool scalars_mont = false);
void msm_release_all();
int msm_configure();

// ---------------- the QAP handle's launch sequence without its argument checks (qap.hip) ----------------
// zkg_qap_witness_h_async for a caller inside the library whose buffers are its own: same launches, same ordering and growth; stats receives
// witnesses enqueued, launch groups and host waits, and the calling thread's zkg_qap_stats stay as they are.
}  // namespace zk
struct zkg_qap;
namespace zk {
int qap_witness_h_enqueue(zkg_qap *q, const void *d_witnesses, size_t stride, size_t count, void *d_h, size_t h_stride, uint32_t *d_unsat, hipStream_t s, size_t stats[3]);

// ---------------- key blobs (codec.hip) ----------------
// affine points on the device -> the pk blob's compressed records (34 bytes per G1; 100 per knowledge commitment G2 | G1 of the sparse
// B query, entry idx[j]); d_out: 16-byte aligned device staging for n x 34 (nidx x 100) bytes
int compress_g1_records(const G1Affine *d_in, size_t n, uint8_t *d_out, hipStream_t s);
int compress_kc_records(const G2Affine *d_g2, const G1Affine *d_g1, const uint32_t *d_idx, size_t nidx, uint8_t *d_out, hipStream_t s);

// ---------------- batch verification kernels (verify.hip) ----------------
// one lane per item.  ok[i] = 1 iff [r]B_i == O; out[i] = w_i P_i (w: n x 4 u32, 128-bit weights, little-endian) in affine form;
// Miller values ML(P_i, Q_i) as 384-byte Fq12 (1 where a point is infinity or use[i] == 0; use optional)
static constexpr size_t VERIFY_PROD_BLOCKS = 64;         // the range product's first launch: at most this many partial Fq12
int verify_g2_subgroup(const G2Affine *d_B, size_t n, uint8_t *d_ok, hipStream_t s);
int verify_g1_mul128(const G1Affine *d_in, const uint32_t *d_w, size_t nw, size_t n, G1Affine *d_out, hipStream_t s);   // lane i: weight i mod nw
int verify_miller(const G1Affine *d_P, const G2Affine *d_Q, const uint8_t *d_use, size_t n, void *d_out, hipStream_t s);
int verify_fq12_product(const void *d_in, size_t lo, size_t hi, void *d_partial, void *d_out, hipStream_t s);   // d_out[0] = prod d_in[lo, hi)
// the seam's device front end.  Proof records of ZKG_PROOF_BYTES -> B (n lanes), A and C back to back in d_AC (2 n lanes): affine Montgomery
// points as ser::get_g1 / ser::get_g2 give them, infinity where the record is infinity or does not decode; d_dec: a byte per lane, 1 = decoded
// by the single verifier's rule with canonical limbs.  use[i] = in_g2[i] && dec_b[i] && dec_ac[i] && dec_ac[n + i].
int verify_proof_decode_b(const uint8_t *d_rec, size_t n, G2Affine *d_B, uint8_t *d_dec, hipStream_t s);
int verify_proof_decode_ac(const uint8_t *d_rec, size_t n, G1Affine *d_AC, uint8_t *d_dec, hipStream_t s);
int verify_use_mask(size_t n, const uint8_t *d_in_g2, const uint8_t *d_dec_b, const uint8_t *d_dec_ac, uint8_t *d_use, hipStream_t s);
// d_out[k] = sum over positions lo <= p < hi with d_mask[p] (optional) of weight_p * x_pk, Montgomery Fr, k < zv_input_count(npl); position p
// has its npl public records (zklaim_public.hip.hpp) at d_pub + (p - base) * npl * 80 and its weight at d_w + 4 p; d_part: ZV_SUM_SLICES x l Fr
static constexpr size_t ZV_SUM_SLICES = 16;
int verify_zklaim_input_sums(const uint8_t *d_pub, uint32_t npl, size_t base, const uint32_t *d_w, const uint8_t *d_mask, size_t lo, size_t hi,
                             void *d_part, void *d_out, hipStream_t s);
// the seam's per-proof entry (zkg_zklaim_verify_each): a key's bit table T[s] = 2^(s mod 253) IC_(s / 253), s < zklaim_bit_table_entries(npl)
// (the string bits npl payloads can set), built from the key's l = zv_input_count(npl) dense IC points (infinity where the key has none);
// then d_out[i] = -(ic0 + sum_k x_ik IC_k) from item i's npl public records at d_pub + i * npl * 80, and (d_c given) d_negc[i] = -d_c[i]
size_t zklaim_bit_table_entries(uint32_t npl);
size_t zklaim_bit_table_tmp_bytes(uint32_t npl);         // the build's XYZZ staging
int verify_zklaim_bit_table(const G1Affine *d_ic, uint32_t npl, void *d_tmp, G1Affine *d_T, hipStream_t s);
int verify_zklaim_ic_each(const G1Affine *d_ic0, const G1Affine *d_T, const uint8_t *d_pub, uint32_t npl, size_t n, G1Affine *d_out,
                          const G1Affine *d_c, G1Affine *d_negc, hipStream_t s);
void zklaim_ic_each_device_code_on_host(const G1Affine &ic0, const G1Affine *ic, const uint8_t *pub, uint32_t npl, size_t n, G1Affine *out);
void verify_keys_release_all();                          // zkg_shutdown: the prepared keys and their bit tables (setup_verify.hip)
int initialised_device();                                // the device zkg_init selected, -1 before (capi.hip)
// ZKG_ERROR (message "<who>: <what> ...") unless d is `bytes` of device memory of `device`, aligned to `align` (capi.hip); owner: "key", "handle"
int dev_range_refused(const void *d, size_t bytes, size_t align, int device, const char *who, const char *what, const char *owner);
// the rules the *_async entries share (capi.hip): the calling thread is on `device` ("<who>: the calling thread's device is not the one <made>");
// `count` vectors of n elements lie `stride` elements apart, within ZKG_MSM_ASYNC_MAX_COUNT / _STRIDE
int wrong_device_refused(const char *who, int device, const char *made);
int async_vectors_refused(const char *who, size_t n, const char *n_name, size_t stride, size_t count, int device, const char *made);
// the per-proof verifier (zkg_groth16_verify_each, zkg_pairing_each, zkg_final_exp)
int verify_ic_each(const G1Affine *d_ic0, const G1Affine *d_ic, uint32_t nidx, const void *d_x, size_t n, G1Affine *d_out, hipStream_t s);
int verify_g2_replicate(const G2Affine *d_key2, size_t n, G2Affine *d_Q, hipStream_t s);     // d_Q[n + i] = key2[0], d_Q[2 n + i] = key2[1]
size_t verify_final_exp_ws_bytes(size_t n);              // the slot workspace of n lanes
int verify_final_exp_check(const void *d_M, size_t n, uint32_t pairs, void *d_ws, const void *d_ab, uint8_t *d_verdict, void *d_gt, hipStream_t s);
void final_exp_device_code_on_host(const uint8_t in[384], uint8_t out[384]);
// the known-answer hook of the device tower (zkg_fq12_op): the operation numbers of include/zkg.h; raw 96-word Fq12, nothing normalised
enum { FQ12_MUL = 0, FQ12_SQR, FQ12_LINE, FQ12_CSQR, FQ12_INV, FQ12_CONJ, FQ12_FROB1, FQ12_FROB2, FQ12_FROB3, FQ12_MUL_BY_V, FQ12_OPS };
int verify_fq12_op(int op, const void *d_a, const void *d_b, size_t n, void *d_out, hipStream_t s);      // k_fq12_op; d_b: FQ12_MUL and FQ12_LINE only
void fq12_op_device_code_on_host(int op, const uint32_t a[96], const uint32_t b[96], uint32_t out[96]);  // the same text on the host, one element
// a batch call's device workspace: grow-only buffer, two streams (the subgroup check runs beside the scalar multiplications), two events
struct VerifyWorkspace { DevBuf buf; hipStream_t s = nullptr, s2 = nullptr; hipEvent_t ev = nullptr, ev2 = nullptr; };
VerifyWorkspace *verify_workspace_acquire();             // a free one or a new one; null on a HIP failure (message set)
void verify_workspace_release(VerifyWorkspace *w);       // back to the free list (null: nothing)
void verify_workspace_destroy(VerifyWorkspace *w);
void verify_release_all();                               // zkg_shutdown: the free workspaces' buffers, streams and events

// ---------------- zklaim witnesses on the device (zklaim_witness.hip) ----------------
// The generator derives the sparse witness of every context of a chunk (tags, listed indices and values) from a 128-byte record per
// payload and writes it in the packed form the batched prover's split reads: [descriptors | values | indices | tags].
struct ZwPlan { uint32_t k = 0, per = 0, n = 0, cap = 0; };          // payloads, variables per payload sub-circuit, variables, listed slots per item
uint32_t zklaim_payload_vars_host();                               // zklaim_circuit.hip: what the host pass measures per payload
// the plan for k payloads, or for the key with n variables; false (message set) when the generator's own count of a payload's variables
// disagrees with the host pass's, or no payload count gives n: the caller then keeps the host witnesses
bool zklaim_witness_plan(uint32_t k, ZwPlan &pl);
bool zklaim_witness_plan_for_n(size_t n, ZwPlan &pl);
size_t zklaim_witness_input_bytes(const ZwPlan &pl, uint32_t P);  // [error word | table of 1/1 .. 1/64 | P x k records], one upload
// fills the input block; ok[p] = 0 for a null context, a payload count other than k or a broken payload list (nothing is written for it)
void zklaim_witness_pack(const ZwPlan &pl, const struct ::zklaim_ctx *const *ctxs, uint32_t P, uint8_t *host_in, uint8_t *ok);
// desc: P (offset, count) pairs; item p's listed slots are pl.cap entries from p * pl.cap.  d_in[0] is non-zero afterwards if a cursor went astray.
extern thread_local size_t t_zklaim_witness_stats[2];          // prover.hip; the seam adds its groups up in it
extern thread_local size_t t_prove_zklaim_stats[2];            // prover.hip: zkg_prove_zklaim_stats; libsnark_prove's host pass reports itself here
int zklaim_witness_launch(const ZwPlan &pl, uint32_t P, uint8_t *d_in, uint32_t *d_desc, Fr *d_vals, uint32_t *d_idx, uint8_t *d_tags, size_t tag_stride, hipStream_t s);
// The same contract on k_zklaim_witness_par, the generator shaped for one proof's latency: its input block is [error word | P x k records]
// only — the 1 / c table and the slices' plan are resident on the device, uploaded by the first launch there.  _ready: the slices' plan
// (derived from the mirror's trace) ends where the payload's does; false (message set): the caller keeps the host witness.
bool zklaim_witness_par_ready(const ZwPlan &pl);
size_t zklaim_witness_par_input_bytes(const ZwPlan &pl, uint32_t P);
void zklaim_witness_par_pack(const ZwPlan &pl, const struct ::zklaim_ctx *const *ctxs, uint32_t P, uint8_t *host_in, uint8_t *ok);
int zklaim_witness_par_launch(const ZwPlan &pl, uint32_t P, uint8_t *d_in, uint32_t *d_desc, Fr *d_vals, uint32_t *d_idx, uint8_t *d_tags, size_t tag_stride, hipStream_t s);
void zklaim_witness_release_all();                              // zkg_shutdown: the resident tables

// ---------------- ABI encodings (capi.cpp) ----------------
void store_norm(uint64_t *out, const G1 &p);   // normalised jac, 12 limbs
void store_norm(uint64_t *out, const G2 &p);   // 24 limbs
G1 load_norm_g1(const uint64_t *in);
G2 load_norm_g2(const uint64_t *in);

}  // namespace zk
