// prover.hip — Groth16 prover pipeline on a device-resident proving key.
//
// Replaces libsnark's r1cs_gg_ppzksnark_prover<ppT>(pk, primary_input, auxiliary_input), the call at
// /root/reference/zklaim/snark.cpp:126, including r1cs_to_qap_witness_map (3 sparse mat-vecs, 3 iFFT,
// 3 cosetFFT, pointwise H = (A.B - C)/Z on the coset, 1 icosetFFT) and the four multi-exponentiations
// (A query; B query in G2 and G1; H query; L query), and the proof serialisation operator<< reached from
// zklaim/libsnark_wrapper.cpp:170-181.
//
// What differs from the reference by design: the pk is parsed and uploaded ONCE (zkg_crs_upload) instead
// of on every call (libsnark_wrapper.cpp:230 + the by-value copy at snark.cpp:107-109); iFFT's 1/m and
// the following cosetFFT's g^i are one fused table multiplication; the H query and the witness queries' non-bit elements live on
// the device as per-window tables (2^(c w) P_i), so a multi-exponentiation is one bucket set, one reduction and no host doublings; the witness queries are split
// as multi_exp_with_mixed_addition splits them (zeros skipped, ones summed flat, the rest through the bucket method, A / B_g1 / L
// sharing one digit sort); the prover randomness (r, s) is an explicit input.
#include "common.hpp"
#include "r1cs.hip.hpp"
#include "proof_assemble.hpp"
#include "../../include/zkg.h"
#include "../../include/zklaim_abi.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <functional>
#include <condition_variable>
#include <thread>
#include <vector>

namespace zk {

struct DevCsr { DevBuf rowptr, col, val; size_t nnz = 0; };
thread_local size_t t_zklaim_witness_stats[2] = {0, 0};      // zkg_zklaim_witness_stats: items whose witness the GPU made, the host made
thread_local size_t t_prove_zklaim_stats[2] = {0, 0};        // zkg_prove_zklaim_stats: the last single credential's witness came from the GPU, from the host
thread_local size_t t_prove_dev_stats[2] = {0, 0};           // zkg_prove_dev_stats: witnesses split on the device from the caller's buffer, staged through host memory

}  // namespace zk

// Everything one proof in flight needs on top of the shared key: its [1 | w], the three evaluation vectors, the transform
// scratch, a stream for the mat-vec / NTT pipeline, three MSM jobs (stream + workspace + pinned landing zone each) and the
// events that order them.  Up to three per key for small domains, created when callers overlap (see zkg_crs): a large proof's
// concurrent MSMs already fill the chip, a small one leaves room.
// One persistent helper thread per prover slot: it queues the witness streams' work while the calling thread queues the critical path, and
// later computes one of the two variable-base products of the assembly.  (std::async spawned a thread for each: 30-50 us apiece on every
// proof, and the occasional multi-millisecond outlier when the spawn was slow.)
struct Helper {
    std::thread th; std::mutex mu; std::condition_variable cv;
    std::function<int()> task; bool has_task = false, done = true, stop = false; int result = 0;
    int device = 0;                       // the key's device: a new thread starts on device 0, and this one launches kernels on the slot's streams
    void start() { (void)hipGetDevice(&device); th = std::thread([this] { loop(); }); }
    void loop() {
        (void)hipSetDevice(device);
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return has_task || stop; });
            if (stop) return;
            std::function<int()> t = std::move(task); has_task = false;
            lk.unlock();
            int r = ZKG_ERROR;
            try { r = t(); } catch (...) { r = ZKG_ERROR; }
            lk.lock();
            result = r; done = true;
            cv.notify_all();
        }
    }
    void submit(std::function<int()> f) { std::lock_guard<std::mutex> lk(mu); task = std::move(f); has_task = true; done = false; cv.notify_all(); }
    int wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return done; }); return result; }
    void shutdown() { if (!th.joinable()) return; { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); th.join(); }
};

struct ProverSlot {
    zk::DevBuf z, aABC, flag, up_tags, up_idx, up_vals;    // up_*: staging of a sparse witness                   // [1 | w] and aA | aB | aC back to back (batched NTTs)
    zk::DevBuf ntt_scratch;                     // inter-pass scratch, 3 m elements
    zk::DevBuf wtags, wlisted, wcount;          // the witness split: tag per element of z, indices of the non-bit elements, their count
    // a zklaim credential whose witness the device generates (zkg_groth16_prove_zklaim): its records packed in pinned memory, their place on
    // the device ([error word | records | descriptor]), and what became of it (ZW_*: prove_enqueue's error is the context's, or the generator's)
    uint8_t *zw_stage = nullptr; size_t zw_stage_cap = 0; zk::DevBuf zw_in; int zw_state = 0;
    hipStream_t stream = nullptr;               // upload + split + mat-vec + NTT stream
    // witness multi-exponentiations: one job for the three G1 queries (A, B_g1, L share the digit sort), one for B_g2; H on its own
    zk::MsmJob *job_w1 = nullptr, *job_w2 = nullptr, *job_h = nullptr;
    // H sharded over several devices (zkg_crs_shard_h): this slot's job, scalar slice and "slice copied" event on every shard's device
    struct HShardRun { int device = 0; zk::MsmJob *job = nullptr; zk::DevBuf scalars; };
    std::vector<HShardRun> h_runs; uint64_t h_epoch = 0;                       // h_epoch: the sharding (zkg_crs::h_epoch) these were made for
    zk::OnesSum ones_g1, ones_g2;               // flat sums of the bases whose witness element is one: (A, B_g1, L) and B_g2, on streams of their own
    std::vector<uint8_t> scan_tags; std::vector<uint32_t> scan_idx; std::vector<uint64_t> scan_vals;    // a dense witness rewritten as tags + listed values (witness_to_sparse)
    hipStream_t stream_o = nullptr;
    Helper helper;
    hipEvent_t ev[20]; bool ev_ok = false, ready = false;
    float stage_ms[8] = {0};
    // the proof in flight between prove_enqueue and prove_finish
    uint32_t *flag_host = nullptr;              // pinned: [0] lands the satisfiability flag, [1] the count of non-bit witness elements, [4] the witness generator's error word
    bool check = false; zk::Fr r, s;
    std::chrono::steady_clock::time_point t0;
};

// The workspace of zkg_groth16_prove_batch: one chunk of up to P proofs of the key in flight as ONE launch sequence.  Proof p's vectors lie
// p strides apart in every buffer (z: n + 1 elements; aABC: aA | aB | aC, 3 m; the transform scratch the same shape), so that the kernels
// take the proof as blockIdx.y and the transforms see a batch of 3 P (then P) vectors.  The multi-exponentiations are multi launches
// (msm_job_launch_multi: P scalar vectors over one table): H over coefficients_for_H, the witness queries over wscal — every proof's values
// at the elements the witness tables cover, zero where this witness has a bit there — one job for A / B_1 / L and one for B_2, on streams of
// their own.  The flat sums over the ones take the proof as blockIdx.z (ones_sum_launch_multi), on two more streams.  Kept with the key, reused
// by every call, freed with it.
struct BatchWs {
    uint32_t P = 0; bool ready = false;
    zk::DevBuf z, aABC, scratch, wtags, wlisted, words, stage, wscal;
    uint8_t *host_stage = nullptr; size_t host_cap = 0;      // pinned: the chunk's witnesses, packed (one upload)
    uint32_t *host_words = nullptr;                          // pinned: P x BATCH_WORDS after the split, then P x BATCH_WORDS after the mat-vec, then the witness generator's error word
    hipStream_t stream = nullptr, wst[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_in = nullptr;                              // zkg_groth16_prove_batch_dev: the caller's stream at the time of the call; `stream` waits for it
    zk::MsmJob *job_h = nullptr, *job_w1 = nullptr, *job_w2 = nullptr; zk::OnesSum ones_g1, ones_g2;
    hipEvent_t ev_split = nullptr, ev_flags = nullptr, ev_gathered = nullptr;      // the split's words landed; the mat-vec's flags landed; the witness jobs' scalars gathered
};

// (CombTable, the fixed-base tables of alpha_1, beta_1, delta_1, delta_2: proof_assemble.hpp, shared with prove_async.hip)
struct zkg_crs {
    uint32_t n = 0, l = 0, C = 0, log_m = 0; size_t m = 0;
    zk::DevCsr A, B, Cm;
    // Per-window tables (level w = 2^(c w) P_i, level 0 = the query itself): windows share one bucket set, one reduction per
    // multi-exponentiation and no doubling on the host.  The H query gets one over all of its m - 1 points (its scalars are dense).
    // The witness queries stay as uploaded (the flat sums over the ones read them) and get tables over a SUBSET of their elements only:
    // the bucket method sees the non-bit variables of a witness, ~3 % of a credential's, and the same ones proof after proof.
    zk::WindowTable H_query;
    // One proof's H query over several GPUs ("the four MSMs are mutually independent -> task-parallel across GPUs first,
    // then point-sharding"): H is the largest of the four (m - 1 uniformly random scalars, 40 - 50 % of a proof's critical path at
    // m >= 2^18) and shards by points exactly like the plain multi-exponentiation: shard i holds the per-window table of its contiguous
    // slice of the query on devices[i]; a proof copies that slice of coefficients_for_H to it (32 B per point: 4 MiB per shard at m = 2^20
    // over eight devices), every shard runs the single-GPU table launch on a stream of its own, and the partial points are added on the host.
    struct HShard { int device = 0; size_t first = 0, n = 0; zk::WindowTable table; };
    std::vector<HShard> h_shards; int home_device = 0; uint64_t h_epoch = 0;
    zk::DevBuf A_query, B_g1, B_g2, L_query;    // n + 1, n + 1, n + 1 (G2), n - l affine points
    struct SubsetTables {
        std::vector<uint8_t> member;            // host: is element i of z = [1 | w] covered
        zk::DevBuf pos, idx;                    // device: position of every element in the subset (SUBSET_NONE = absent); the covered elements, ascending
        size_t count = 0; uint32_t rebuilds = 0;
        zk::WindowTable A, B1, B2, L;           // count points per level; the L table holds infinity for the constant and the public inputs
    } sub;
    int c_w = 8, c_w_forced = 0;                // window bits of the witness tables (set when they are built), ZKG_TABLE_C_W override
    zk::G1Affine alpha_g1, beta_g1, delta_g1; zk::G2Affine beta_g2, delta_g2;
    zk::CombTable<zk::Fq> alpha1_comb, beta1_comb, delta1_comb; zk::CombTable<zk::Fq2> delta2_comb;
    zk::NttDomain *dom = nullptr;               // basic_radix2_domain (m = 2^log_m) ...
    zk::StepDomain *sdom = nullptr;             // ... or step_radix2_domain (m = 2^(log_m-1) + 2^b); exactly one is set
    zk::DevBuf coset_over_m, coset_over_m29;    // g^i / m : iFFT post-scale fused with the next cosetFFT's pre-scale (and its 29-bit records)
    zk::DevBuf long_rows; uint32_t n_long = 0;  // (matrix << 30 | row) of every row with more than LONG_ROW terms
    zk::Fr z_inv_coset;                         // 1 / (g^m - 1)
    // Prover slots.  A lone caller only ever uses slot 0 (created with the key).  When callers arrive on several threads, a second and a
    // third slot are created on first need: from 8 payloads up one proof fills the chip and a second in flight adds 4 %, but a one-payload
    // proof is latency chains and three in flight give 1.6x the proofs per second (tools/prove_throughput.py).  The witness tables are
    // shared: a proof that has to extend them waits, holding its slot, until every other proof in flight has either finished or is waiting
    // for the same reason, and no new proof starts meanwhile (`extending`, `waiting_ext`).
    static constexpr int MAX_SLOTS = 3;
    ProverSlot slot[MAX_SLOTS];
    float stage_ms[8] = {0};
    std::mutex mu; std::condition_variable cv;
    bool busy[MAX_SLOTS] = {false, false, false}; int leases = 0, waiting_ext = 0; bool extending = false;
    // zkg_groth16_prove_batch: one chunk workspace per key; batch callers take turns on it (batch_mu, always taken BEFORE a slot lease)
    BatchWs batch; std::mutex batch_mu;
    int device = 0;                             // the device the key was uploaded on (the *_dev prove entries refuse a caller on another one)
    int provers = 0;                            // live zkg_prover handles (under mu): they hold H_query, so zkg_crs_shard_h refuses while there is one
};

namespace zk {

// row_dot_short, r1cs_long_entry, or_and_wait and LONG_ROW: r1cs.hip.hpp (shared with the QAP handle's kernels, qap.hip)
// flag (or null): the satisfiability gate for rows without a long side, see below.
__global__ __launch_bounds__(256) void k_r1cs_eval(const uint32_t *a_rp, const uint32_t *a_col, const Fr *a_val,
                                                    const uint32_t *b_rp, const uint32_t *b_col, const Fr *b_val,
                                                    const uint32_t *c_rp, const uint32_t *c_col, const Fr *c_val,
                                                    const Fr *z, uint32_t C, uint32_t l, size_t m, Fr *aA, Fr *aB, Fr *aC, int critical, uint32_t *flag /* or null */) {
    crit_wave_priority(critical);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    if (i < C) {
        bool la = false, lb = false, lc = false;
        const Fr a = row_dot_short(a_rp, a_col, a_val, z, i, la);
        const Fr b = row_dot_short(b_rp, b_col, b_val, z, i, lb);
        const Fr c = row_dot_short(c_rp, c_col, c_val, z, i, lc);
        // the satisfiability gate (snark.cpp:121-124) for this row, here where its three values are in registers: a kernel of its own over
        // the stored vectors stood 14 us (8 payloads) ... 53 us (37) in front of the transforms.  Rows with a long side: k_r1cs_check_rows.
        if (flag && !(la | lb | lc) && a * b != c) or_and_wait(flag);
        aA[i] = a.normalized();
        aB[i] = b.normalized();
        aC[i] = c.normalized();
    } else {
        aA[i] = (i <= (size_t)C + l ? z[i - C] : Fr::zero()).normalized();
        aB[i] = Fr::zero().normalized();
        aC[i] = Fr::zero().normalized();
    }
}
// the long rows, a launch of their own behind k_r1cs_eval (see compute_h_matvec)
__global__ __launch_bounds__(256) void k_r1cs_long(const uint32_t *list, uint32_t n_long,
                                                    const uint32_t *a_rp, const uint32_t *a_col, const Fr *a_val,
                                                    const uint32_t *b_rp, const uint32_t *b_col, const Fr *b_val,
                                                    const uint32_t *c_rp, const uint32_t *c_col, const Fr *c_val,
                                                    const Fr *z, Fr *aA, Fr *aB, Fr *aC) {
    uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_long) return;
    r1cs_long_entry(list[wave], lane, a_rp, a_col, a_val, b_rp, b_col, b_val, c_rp, c_col, c_val, z, aA, aB, aC);
}
// flag[0] |= 1 when a row violates <A,z><B,z> = <C,z>: the pb.is_satisfied() gate of snark.cpp:121-124.  The gate over the rows k_r1cs_long
// filled in (entries of its list; a row listed twice is checked twice), behind it in stream order — k_r1cs_eval has tested every other row.
// The last workgroup to finish (ticket in flag[1]) writes the verdict straight into the caller's pinned word: no copy launch between the
// mat-vec and the transforms.
__global__ __launch_bounds__(256) void k_r1cs_check_rows(const uint32_t *list, uint32_t n_long, const Fr *aA, const Fr *aB, const Fr *aC, uint32_t *flag, uint32_t *host_flag) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_long) { const uint32_t row = list[j] & 0x3fffffffu; if (aA[row] * aB[row] != aC[row]) or_and_wait(flag); }
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(flag + 1, 1u) == gridDim.x - 1) host_flag[0] = atomicOr(flag, 0u);
}

// the same on a step_radix2_domain: Z(g x_i) takes big/small distinct values on the first big points and one on the rest
__global__ __launch_bounds__(256) void k_pointwise_h_step(Fr *aA, const Fr *aB, const Fr *aC, size_t m, size_t big, const Fr *zinv, uint32_t period_mask, Fr zinv_small, int critical) {
    crit_wave_priority(critical);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    Fr zi = i < big ? zinv[i & period_mask] : zinv_small;
    aA[i] = ((aA[i] * aB[i] - aC[i]) * zi).normalized();
}

__global__ void k_set_one(Fr *z) { if (threadIdx.x == 0 && blockIdx.x == 0) z[0] = Fr::one(); }

// Sparse witness upload: a credential's witness is ~97 % zeros and ones, so the host sends one tag byte per variable (0 zero, 1 one,
// 2 listed) and the listed values as (index, value) records — 0.5 MB instead of 17.5 MB at 20 payloads.  The two kernels also ARE the
// multi_exp_with_mixed_addition split of z = [1 | w] (what k_classify derives from a dense witness): k_expand_tags writes the constant,
// the zeros and ones and their tags and clears the proof's counters, k_scatter_full writes the listed values, tags each by its VALUE (a
// listed 0 or 1 is a bit like any other), lists the others and tells the host how many there are — the last workgroup to finish writes
// into the pinned words, so no fill, classify or copy launch stands between the upload and the mat-vec.
// words: [0] satisfiability flag, [1] k_r1cs_check_rows' ticket, [2] k_scatter_full's ticket, [3] bad listed entry; count: [0] listed, [1] a listed element misses the witness tables
static constexpr uint32_t TAG_UNCLAIMED = 3;
__global__ __launch_bounds__(256) void k_expand_tags(const uint8_t *tags, size_t n, Fr *z /* z[0] is the constant */, uint8_t *wtags, uint32_t *words, uint32_t *count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { z[0] = Fr::one(); wtags[0] = 1; words[0] = 0; words[1] = 0; words[2] = 0; words[3] = 0; count[0] = 0; count[1] = 0; }
    if (i >= n) return;
    const bool one = tags[i] == 1;
    z[i + 1] = one ? Fr::one() : Fr::zero();                                   // listed entries are overwritten by k_scatter_full
    wtags[i + 1] = one ? 1 : (tags[i] == 2 ? TAG_UNCLAIMED : 0);               // a tag-2 variable waits for its one listing (never listed: counts as zero; no consumer reads 3 as a bit)
}
// A listed variable's tag byte goes from TAG_UNCLAIMED to the tag of its value exactly once: the second listing of an index finds the byte
// taken and fails the call (it used to put the position into the gather list twice: A / B / L counted z[pos] twice while H saw it once —
// ZKG_OK with an invalid proof).  Byte-wide compare-and-swap on the containing word; the neighbours' bytes may change under it.
ZK_D bool claim_listed_tag(uint8_t *wtags, uint32_t pos, uint32_t tag) {
    uint32_t *w = reinterpret_cast<uint32_t *>(wtags + (pos & ~3u)); const uint32_t sh = 8 * (pos & 3u);
    uint32_t old = atomicOr(w, 0u);
    for (;;) {
        if (((old >> sh) & 0xffu) != TAG_UNCLAIMED) return false;
        const uint32_t want = (old & ~(0xffu << sh)) | (tag << sh), prev = atomicCAS(w, old, want);
        if (prev == old) return true;
        old = prev;
    }
}
// the tag of an element by its VALUE: 0 zero, 1 one, 2 anything else (k_classify in msm.hip keeps a copy of this rule, and records a subset miss with a plain store)
ZK_D uint32_t tag_by_value(const Fr &v) {
    uint32_t any = 0, diff = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { any |= v.v[j]; diff |= v.v[j] ^ FrParams::ONE[j]; }
    return any == 0 ? 0u : (diff == 0 ? 1u : 2u);
}
// Every lane of the wavefront arrives here; those with is_listed append pos to listed[] — a ballot, ONE atomicAdd on count[0] by the leader, the
// base handed round by a shuffle (unordered across wavefronts) — and raise count[1] when the witness tables do not cover pos (yet).
ZK_D void wave_list_append(bool is_listed, uint32_t pos, uint32_t *listed, uint32_t *count, const uint32_t *subset_pos) {
    const unsigned long long mask = __ballot(is_listed);
    if (!mask) return;
    const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(mask));
    base = __shfl(base, leader, 64);
    if (is_listed) {
        listed[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = pos;
        if (subset_pos && subset_pos[pos] == SUBSET_NONE) or_and_wait(count + 1);
    }
}
// The last workgroup to finish (ticket) hands the split's counts to the pinned words: [1] listed, [2] a listed element misses the witness tables,
// and [3] bad listed entry / [4] the witness generator's error word where the kernel has one: no copy launch between the split and the mat-vec.
ZK_D void publish_split_words(uint32_t *ticket, uint32_t *count, uint32_t *host_words, uint32_t *bad /* or null */, const uint32_t *gen_err /* or null */) {
    __syncthreads();
    if (threadIdx.x != 0 || atomicAdd(ticket, 1u) != gridDim.x - 1) return;
    host_words[1] = atomicOr(count, 0u); host_words[2] = atomicOr(count + 1, 0u);
    if (bad) host_words[3] = atomicOr(bad, 0u);
    if (gen_err) host_words[4] = *gen_err;
}
// entry i of one witness' listing (every lane of the wavefront takes part: the list positions come from a ballot); bad: the call's "bad listed entry" word
ZK_D void scatter_full_entry(size_t i, const uint32_t *idx, const Fr *vals, size_t cnt, size_t n, Fr *z, const uint8_t *tags, uint8_t *wtags,
                             uint32_t *listed, uint32_t *count, uint32_t *bad, const uint32_t *subset_pos) {
    uint32_t tag = 0, pos = 0;
    if (i < cnt) {
        const uint32_t v = idx[i];
        if (v >= n || tags[v] != 2) or_and_wait(bad);                          // a listed index must be in range and tagged 2 (and listed once)
        else {
            const Fr val = vals[i];
            tag = tag_by_value(val);
            pos = v + 1;
            if (claim_listed_tag(wtags, pos, tag)) z[pos] = val;
            else { or_and_wait(bad); tag = 0; }                                 // listed twice: the call fails (words[3]), nothing is listed again
        }
    }
    wave_list_append(tag == 2, pos, listed, count, subset_pos);
}
__global__ __launch_bounds__(256) void k_scatter_full(const uint32_t *idx, const Fr *vals, size_t cnt, size_t n, Fr *z, const uint8_t *tags, uint8_t *wtags,
                                                      uint32_t *listed, uint32_t *count, uint32_t *words, const uint32_t *subset_pos, uint32_t *host_words) {
    scatter_full_entry((size_t)blockIdx.x * blockDim.x + threadIdx.x, idx, vals, cnt, n, z, tags, wtags, listed, count, words + 3, subset_pos);
    publish_split_words(words + 2, count, host_words, words + 3, nullptr);
}

// the same for a listing made on the device (k_zklaim_witness_par): its length is desc[1], known there only, so the launch covers the
// listing's capacity; the last workgroup also hands the generator's error word to the host
__global__ __launch_bounds__(256) void k_scatter_full_counted(const uint32_t *desc, const uint32_t *idx, const Fr *vals, size_t cap, size_t n, Fr *z, const uint8_t *tags, uint8_t *wtags,
                                                              uint32_t *listed, uint32_t *count, uint32_t *words, const uint32_t *subset_pos, uint32_t *host_words, const uint32_t *gen_err) {
    const size_t cnt = desc[1] < cap ? desc[1] : cap;
    scatter_full_entry((size_t)blockIdx.x * blockDim.x + threadIdx.x, idx + desc[0], vals + desc[0], cnt, n, z, tags, wtags, listed, count, words + 3, subset_pos);
    publish_split_words(words + 2, count, host_words, words + 3, gen_err);
}

// Witnesses ALREADY on the device (zkg_groth16_prove_dev, zkg_groth16_prove_batch_dev): this kernel is the whole way in — no staging, no tags
// from the host, no upload.  blockIdx.y = proof; proof p reads the caller's vector at src + p * src_stride (n elements; what lies between n and
// the stride is never read) and writes z_p = [1 | w], the tag of every element by its VALUE (k_classify's rule), the listing of the non-bit
// positions (ballot + one atomic per wavefront, unordered like k_scatter_full's), their count in count[0] and "one of them misses the witness
// tables" in count[1] — each where the next stage reads it: a slot's z / wtags / wlisted / wcount (P = 1, the strides unused) or proof p's
// strides of the batch workspace, count = the proof's words + 4.  count[0..1] and the ticket words[2] are zero when the launch starts (a memset in
// front of it: one launch cannot both clear a counter and count into it).  host_words (single proof): the last workgroup to finish writes the two
// counts into the pinned words, as k_scatter_full does; null (batch): the chunk's one copy of its words carries them.
__global__ __launch_bounds__(256) void k_split_dev(const Fr *src, size_t src_stride, size_t n, Fr *z, uint8_t *wtags, size_t wtag_stride, uint32_t *listed,
                                                   uint32_t *words, uint32_t *count, uint32_t word_stride, const uint32_t *subset_pos, uint32_t *host_words /* or null */) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n1 = n + 1; const uint32_t p = blockIdx.y;
    src += p * src_stride; z += p * n1; wtags += p * wtag_stride; listed += p * n1; words += (size_t)p * word_stride; count += (size_t)p * word_stride;
    uint32_t tag = 0;
    if (i < n1) {
        const Fr v = i ? src[i - 1] : Fr::one();
        tag = tag_by_value(v);
        z[i] = v; wtags[i] = (uint8_t)tag;
    }
    wave_list_append(tag == 2, (uint32_t)i, listed, count, subset_pos);
    if (host_words) publish_split_words(words + 2, count, host_words, nullptr, nullptr);
}

// H_tmp = (aA . aB - aC) * Zinv  (divide_by_Z_on_coset fused with the pointwise product)
__global__ __launch_bounds__(256) void k_pointwise_h(Fr *aA, const Fr *aB, const Fr *aC, size_t m, Fr zinv, int critical) {
    crit_wave_priority(critical);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    aA[i] = ((aA[i] * aB[i] - aC[i]) * zinv).normalized();
}

// ---- the same steps for a chunk of proofs of one key (zkg_groth16_prove_batch): blockIdx.y = proof, proof p's vectors p strides apart.
// Every witness arrives in the sparse form (the host rewrites a dense one), packed into one staging buffer: desc[p] = where its listing
// starts among the chunk's (index, value) records and how long it is.  words: BATCH_WORDS per proof — [0] satisfiability flag, [3] bad listed
// entry, [4] listed (non-bit) elements, [5] one of them misses the witness tables; the host reads all proofs' words in one copy.
static constexpr uint32_t BATCH_WORDS = 8;
struct BatchDesc { uint32_t off, cnt; };
__global__ __launch_bounds__(256) void k_expand_tags_batch(const uint8_t *tags, size_t tag_stride, size_t n, Fr *z, uint8_t *wtags, size_t wtag_stride, uint32_t *words) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; const uint32_t p = blockIdx.y;
    tags += p * tag_stride; z += p * (n + 1); wtags += p * wtag_stride; words += p * BATCH_WORDS;
    if (i == 0) { z[0] = Fr::one(); wtags[0] = 1; for (uint32_t k = 0; k < BATCH_WORDS; ++k) words[k] = 0; }
    if (i >= n) return;
    const bool one = tags[i] == 1;
    z[i + 1] = one ? Fr::one() : Fr::zero();
    wtags[i + 1] = one ? 1 : (tags[i] == 2 ? TAG_UNCLAIMED : 0);
}
__global__ __launch_bounds__(256) void k_scatter_full_batch(const BatchDesc *desc, const uint32_t *idx, const Fr *vals, const uint8_t *tags, size_t tag_stride, size_t n, Fr *z,
                                                            uint8_t *wtags, size_t wtag_stride, uint32_t *listed, uint32_t *words, const uint32_t *subset_pos) {
    const uint32_t p = blockIdx.y; const BatchDesc d = desc[p];
    if ((size_t)blockIdx.x * blockDim.x >= d.cnt) return;                       // (uniform per workgroup: the ballot below sees whole wavefronts)
    uint32_t *w = words + p * BATCH_WORDS;
    scatter_full_entry((size_t)blockIdx.x * blockDim.x + threadIdx.x, idx + d.off, vals + d.off, d.cnt, n, z + p * (n + 1), tags + p * tag_stride, wtags + p * wtag_stride,
                       listed + p * (n + 1), w + 4, w + 3, subset_pos);
}
// proof p: aA | aB | aC at aABC + 3 p m.  The long rows are k_r1cs_long_batch's, their satisfiability k_r1cs_check_rows_batch's (as the single proof's default sequence)
__global__ __launch_bounds__(256) void k_r1cs_eval_batch(const uint32_t *a_rp, const uint32_t *a_col, const Fr *a_val, const uint32_t *b_rp, const uint32_t *b_col, const Fr *b_val,
                                                          const uint32_t *c_rp, const uint32_t *c_col, const Fr *c_val, const Fr *z, size_t z_stride, uint32_t C, uint32_t l, size_t m,
                                                          Fr *aABC, uint32_t *words /* or null */) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; const uint32_t p = blockIdx.y;
    if (i >= m) return;
    z += p * z_stride;
    Fr *aA = aABC + (size_t)3 * p * m, *aB = aA + m, *aC = aB + m;
    Fr a = Fr::zero(), b = Fr::zero(), c = Fr::zero();
    bool la = false, lb = false, lc = false;
    if (i < C) {
        a = row_dot_short(a_rp, a_col, a_val, z, i, la);
        b = row_dot_short(b_rp, b_col, b_val, z, i, lb);
        c = row_dot_short(c_rp, c_col, c_val, z, i, lc);
        if (words && !(la | lb | lc) && a * b != c) or_and_wait(words + p * BATCH_WORDS);
    } else if (i <= (size_t)C + l) {
        a = z[i - C];
    }
    aA[i] = a.normalized(); aB[i] = b.normalized(); aC[i] = c.normalized();
}
__global__ __launch_bounds__(256) void k_r1cs_long_batch(const uint32_t *list, uint32_t n_long, const uint32_t *a_rp, const uint32_t *a_col, const Fr *a_val,
                                                          const uint32_t *b_rp, const uint32_t *b_col, const Fr *b_val, const uint32_t *c_rp, const uint32_t *c_col, const Fr *c_val,
                                                          const Fr *z, size_t z_stride, size_t m, Fr *aABC) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63, p = blockIdx.y;
    if (wave >= n_long) return;
    Fr *aA = aABC + (size_t)3 * p * m;
    r1cs_long_entry(list[wave], lane, a_rp, a_col, a_val, b_rp, b_col, b_val, c_rp, c_col, c_val, z + p * z_stride, aA, aA + m, aA + 2 * m);
}
__global__ __launch_bounds__(256) void k_r1cs_check_rows_batch(const uint32_t *list, uint32_t n_long, const Fr *aABC, size_t m, uint32_t *words) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    if (j >= n_long) return;
    const Fr *aA = aABC + (size_t)3 * p * m;
    const uint32_t row = list[j] & 0x3fffffffu;
    if (aA[row] * aA[m + row] != aA[2 * m + row]) or_and_wait(words + p * BATCH_WORDS);
}
// the witness jobs' scalars: out[p][j] = z_p[idx[j]] where witness p has a non-bit value at element idx[j] of the witness tables' subset, else 0
// (its zeros contribute nothing and its ones belong to the flat sum)
__global__ __launch_bounds__(256) void k_gather_nonbits_batch(const Fr *z, const uint8_t *wtags, size_t n1, size_t wtag_stride, const uint32_t *idx, size_t count, Fr *out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; const uint32_t p = blockIdx.y;
    if (j >= count) return;
    const uint32_t e = idx[j];
    out[p * count + j] = (e < n1 && wtags[p * wtag_stride + e] == 2) ? z[p * n1 + e] : Fr::zero();
}
__global__ __launch_bounds__(256) void k_pointwise_h_batch(Fr *aABC, size_t m, Fr zinv) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    Fr *aA = aABC + (size_t)3 * blockIdx.y * m;
    aA[i] = ((aA[i] * aA[m + i] - aA[2 * m + i]) * zinv).normalized();
}

// the same on a step_radix2_domain (k_pointwise_h_step's arithmetic, the proof as blockIdx.y)
__global__ __launch_bounds__(256) void k_pointwise_h_step_batch(Fr *aABC, size_t m, size_t big, const Fr *zinv, uint32_t period_mask, Fr zinv_small) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    Fr *aA = aABC + (size_t)3 * blockIdx.y * m;
    const Fr zi = i < big ? zinv[i & period_mask] : zinv_small;
    aA[i] = ((aA[i] * aA[m + i] - aA[2 * m + i]) * zi).normalized();
}

static int upload(DevBuf &d, const void *src, size_t bytes) {
    if (d.reserve(bytes ? bytes : 16)) return ZKG_ERROR;
    if (bytes && !hip_ok(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__)) return ZKG_ERROR;
    return ZKG_OK;
}
static int upload_csr(DevCsr &d, const uint32_t *rp, const uint32_t *col, const uint64_t *val, uint32_t rows) {
    if (!rp) { set_error("crs: null CSR"); return ZKG_ERROR; }
    d.nnz = rp[rows];
    if (upload(d.rowptr, rp, (size_t)(rows + 1) * 4) || upload(d.col, col, d.nnz * 4) || upload(d.val, val, d.nnz * 32)) return ZKG_ERROR;
    return ZKG_OK;
}

// ---- host-side proof assembly ---------------------------------------------------------------------
static void canonical_limbs(const Fr &x, uint32_t out[8]) { Fr c = x.from_mont(); for (int i = 0; i < 8; ++i) out[i] = c.v[i]; }
static bool canonical_lsb(const Fq &y) { return y.from_mont().v[0] & 1u; }
static size_t ser_g1(uint8_t *out, const G1 &p) {        // libff operator<<(alt_bn128_G1): binary, Montgomery, compressed
    G1Affine a = p.to_affine(); bool inf = p.is_inf();
    Fq x = inf ? Fq::zero() : a.x, y = inf ? Fq::one() : a.y;
    out[0] = inf ? '1' : '0'; memcpy(out + 1, x.v, 32); out[33] = canonical_lsb(y) ? '1' : '0';
    return 34;
}
static size_t ser_g2(uint8_t *out, const G2 &p) {
    G2Affine a = p.to_affine(); bool inf = p.is_inf();
    Fq2 x = inf ? Fq2::zero() : a.x, y = inf ? Fq2::one() : a.y;
    out[0] = inf ? '1' : '0'; memcpy(out + 1, x.c0.v, 32); memcpy(out + 33, x.c1.v, 32); out[65] = canonical_lsb(y.c0) ? '1' : '0';
    return 66;
}

struct WitnessSrc {                           // dense: n x 4 limbs; or sparse: tags[n] + (idx[count], vals[count x 4 limbs]); or a zklaim context and its plan; or n elements on the device
    const uint64_t *dense = nullptr;
    const Fr *dev = nullptr;
    const uint8_t *tags = nullptr; const uint32_t *idx = nullptr; const uint64_t *vals = nullptr; size_t count = 0;
    const zklaim_ctx *ctx = nullptr; const ZwPlan *plan = nullptr;
};
enum { ZW_NONE = 0, ZW_BAD_CONTEXT = 1, ZW_GENERATOR_ERROR = 2 };
// phase 1 of r1cs_to_qap_witness_map: z = [1 | w] resident and split, the three mat-vecs, the satisfiability flag
static unsigned floor_log2(size_t x) { unsigned r = 0; while (x >>= 1) ++r; return r; }
static int compute_h_matvec(zkg_crs *crs, ProverSlot &S, const WitnessSrc &W, bool want_flag) {
    const int crit = crit_priority_for(1, floor_log2(crs->m)) ? 1 : 0;   // (see ntt_run_ex)
    hipStream_t s = S.stream; uint32_t *flag_out = S.flag_host;
    const size_t m = crs->m;
    Fr *z = S.z.as<Fr>(), *aA = S.aABC.as<Fr>(), *aB = aA + m, *aC = aA + 2 * m;
    uint32_t *words = S.flag.as<uint32_t>(), *count = S.wcount.as<uint32_t>();
    const uint32_t *subset_pos = crs->sub.count ? crs->sub.pos.as<uint32_t>() : nullptr;
    if (W.plan) {
        // the credential goes up as 128 bytes per payload in ONE copy; k_zklaim_witness_par writes the sparse form into the slot's staging, the split follows
        // in stream order.  The listing's length stays on the device (the descriptor), nothing here waits for anything.
        const ZwPlan &pl = *W.plan; const size_t n = crs->n, in_bytes = zklaim_witness_par_input_bytes(pl, 1), o_desc = (in_bytes + 63) / 64 * 64;
        if (pl.n != n) { set_error("zkg_groth16_prove_zklaim: plan does not fit the key"); return ZKG_ERROR; }
        if (S.zw_stage_cap < in_bytes) {
            if (S.zw_stage) (void)hipHostFree(S.zw_stage);
            S.zw_stage = nullptr; S.zw_stage_cap = 0;
            ZK_HIP(hipHostMalloc((void **)&S.zw_stage, in_bytes, hipHostMallocDefault));
            S.zw_stage_cap = in_bytes;
        }
        if (S.zw_in.reserve(o_desc + 64) || S.up_tags.reserve(n) || S.up_idx.reserve((size_t)pl.cap * 4 + 16) || S.up_vals.reserve((size_t)pl.cap * 32 + 16)) return ZKG_ERROR;
        uint8_t ok = 0;
        zklaim_witness_par_pack(pl, &W.ctx, 1, S.zw_stage, &ok);
        if (!ok) { S.zw_state = ZW_BAD_CONTEXT; set_error("zkg_groth16_prove_zklaim: broken payload list or a payload count other than the key's"); return ZKG_ERROR; }
        uint8_t *d_in = S.zw_in.as<uint8_t>(); uint32_t *desc = reinterpret_cast<uint32_t *>(d_in + o_desc);
        ZK_HIP(hipMemcpyAsync(d_in, S.zw_stage, in_bytes, hipMemcpyHostToDevice, s));
        if (zklaim_witness_par_launch(pl, 1, d_in, desc, S.up_vals.as<Fr>(), S.up_idx.as<uint32_t>(), S.up_tags.as<uint8_t>(), n, s)) return ZKG_ERROR;
        hipLaunchKernelGGL(k_expand_tags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, S.up_tags.as<uint8_t>(), n, z, S.wtags.as<uint8_t>(), words, count);
        hipLaunchKernelGGL(k_scatter_full_counted, dim3((unsigned)((pl.cap + 255) / 256)), dim3(256), 0, s, desc, S.up_idx.as<uint32_t>(), S.up_vals.as<Fr>(), (size_t)pl.cap, n, z,
                           S.up_tags.as<uint8_t>(), S.wtags.as<uint8_t>(), S.wlisted.as<uint32_t>(), count, words, subset_pos, S.flag_host, reinterpret_cast<const uint32_t *>(d_in));
    } else if (W.dev) {
        // the caller's device buffer (zkg_groth16_prove_dev; the slot's stream already waits for the caller's): k_split_dev reads it in place, and its
        // last workgroup hands the counts to the pinned words.  The two memsets are the host-dense branch's.
        ZK_HIP(hipMemsetAsync(words, 0, 16, s));
        ZK_HIP(hipMemsetAsync(count, 0, 8, s));
        hipLaunchKernelGGL(k_split_dev, dim3((unsigned)(((size_t)crs->n + 256) / 256), 1), dim3(256), 0, s, W.dev, (size_t)0, (size_t)crs->n, z, S.wtags.as<uint8_t>(), (size_t)0,
                           S.wlisted.as<uint32_t>(), words, count, 0u, subset_pos, S.flag_host);
    } else if (W.dense || !crs->n) {
        hipLaunchKernelGGL(k_set_one, dim3(1), dim3(64), 0, s, z);
        if (crs->n) ZK_HIP(hipMemcpyAsync(z + 1, W.dense, (size_t)crs->n * 32, hipMemcpyHostToDevice, s));
        ZK_HIP(hipMemsetAsync(words, 0, 16, s));
        // the multi_exp_with_mixed_addition split of z: tags, the indices of the non-bit elements, and their count (read by the host)
        // (and whether every one of them has its place in the witness tables: flag_host[2])
        if (witness_classify(z, (size_t)crs->n + 1, S.wtags.as<uint8_t>(), S.wlisted.as<uint32_t>(), count, s, subset_pos)) return ZKG_ERROR;
        ZK_HIP(hipMemcpyAsync(S.flag_host + 1, count, 8, hipMemcpyDeviceToHost, s));
    } else {
        const size_t n = crs->n, cnt = W.count;
        if (S.up_tags.reserve(n) || S.up_idx.reserve(cnt * 4 + 16) || S.up_vals.reserve(cnt * 32 + 16)) return ZKG_ERROR;
        ZK_HIP(hipMemcpyAsync(S.up_tags.p, W.tags, n, hipMemcpyHostToDevice, s));
        if (cnt) {
            ZK_HIP(hipMemcpyAsync(S.up_idx.p, W.idx, cnt * 4, hipMemcpyHostToDevice, s));
            ZK_HIP(hipMemcpyAsync(S.up_vals.p, W.vals, cnt * 32, hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(k_expand_tags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, S.up_tags.as<uint8_t>(), n, z, S.wtags.as<uint8_t>(), words, count);
        if (cnt) hipLaunchKernelGGL(k_scatter_full, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, S.up_idx.as<uint32_t>(), S.up_vals.as<Fr>(), cnt, n, z,
                                    S.up_tags.as<uint8_t>(), S.wtags.as<uint8_t>(), S.wlisted.as<uint32_t>(), count, words, subset_pos, S.flag_host);
    }
    if (S.ev_ok) (void)hipEventRecord(S.ev[0], s);                      // z = [1 | w] is resident and split from here on
    // The long rows are a launch of their own.  With their workgroups leading k_r1cs_eval's grid instead the stage got shorter (8 payloads
    // 0.069 -> 0.055 ms, 37 payloads 0.18 -> 0.13) and the proof did not: at 8 payloads it got LONGER (1.13 -> 1.15 ms, three alternating runs) — the
    // witness jobs' first small kernels slip onto the chip during the short launches in front of the first transform, and then found
    // its workgroups holding every CU's LDS — and at 37 payloads it was inside the noise (3.06 against 3.08).
    hipLaunchKernelGGL(k_r1cs_eval, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s,
                       crs->A.rowptr.as<uint32_t>(), crs->A.col.as<uint32_t>(), crs->A.val.as<Fr>(),
                       crs->B.rowptr.as<uint32_t>(), crs->B.col.as<uint32_t>(), crs->B.val.as<Fr>(),
                       crs->Cm.rowptr.as<uint32_t>(), crs->Cm.col.as<uint32_t>(), crs->Cm.val.as<Fr>(),
                       z, crs->C, crs->l, m, aA, aB, aC, crit, want_flag ? words : nullptr);
    if (crs->n_long)
        hipLaunchKernelGGL(k_r1cs_long, dim3((crs->n_long + 3) / 4), dim3(256), 0, s, crs->long_rows.as<uint32_t>(), crs->n_long,
                           crs->A.rowptr.as<uint32_t>(), crs->A.col.as<uint32_t>(), crs->A.val.as<Fr>(),
                           crs->B.rowptr.as<uint32_t>(), crs->B.col.as<uint32_t>(), crs->B.val.as<Fr>(),
                           crs->Cm.rowptr.as<uint32_t>(), crs->Cm.col.as<uint32_t>(), crs->Cm.val.as<Fr>(), z, aA, aB, aC);
    if (want_flag) {
        if (crs->C) hipLaunchKernelGGL(k_r1cs_check_rows, dim3(std::max<uint32_t>(1, (crs->n_long + 255) / 256)), dim3(256), 0, s, crs->long_rows.as<uint32_t>(), crs->n_long, aA, aB, aC, words, flag_out);
        if (S.ev_ok) (void)hipEventRecord(S.ev[3], s);
    }
    if (S.ev_ok) (void)hipEventRecord(S.ev[1], s);
    if (hipGetLastError() != hipSuccess) { set_error("prover kernel launch failed"); return ZKG_ERROR; }
    return ZKG_OK;
}
// phase 2: the seven transforms and the pointwise step -> coefficients_for_H in aA
static int compute_h_transforms(zkg_crs *crs, ProverSlot &S) {
    const int crit = crit_priority_for(1, floor_log2(crs->m)) ? 1 : 0;   // (see ntt_run_ex)
    hipStream_t s = S.stream;
    const size_t m = crs->m;
    Fr *aA = S.aABC.as<Fr>(), *aB = aA + m, *aC = aA + 2 * m;
    Fr *scr = S.ntt_scratch.as<Fr>();
    const unsigned grid_m = (unsigned)((m + 255) / 256);
    if (crs->dom) {
        // iFFT then cosetFFT of aA, aB, aC as ONE batch of three (a single 2^18 transform fills half the chip; three fill it):
        // inverse transform with the fused post table g^i/m, then a plain forward transform
        const Fr *fused = crs->coset_over_m.as<Fr>();
        if (ntt_run_ex(crs->dom, aA, true, nullptr, fused, nullptr, s, scr, 3, 0, nullptr, crs->coset_over_m29.p)) return ZKG_ERROR;
        if (ntt_run_ex(crs->dom, aA, false, nullptr, nullptr, nullptr, s, scr, 3)) return ZKG_ERROR;
        hipLaunchKernelGGL(k_pointwise_h, dim3(grid_m), dim3(256), 0, s, aA, aB, aC, m, crs->z_inv_coset, crit);
        if (ntt_run_ex(crs->dom, aA, true, nullptr, crs->dom->icoset_post.as<Fr>(), nullptr, s, scr)) return ZKG_ERROR;   // icosetFFT -> coefficients_for_H[0..m)
    } else {
        // step_radix2_domain: the same four steps, each transform a fold/unfold pass around a 2^a and a 2^b radix-2 transform
        StepDomain *sd = crs->sdom;
        if (step_ntt_run(sd, aA, true, false, s, scr, 3, m)) return ZKG_ERROR;                     // iFFT  x3
        if (step_ntt_run(sd, aA, false, true, s, scr, 3, m)) return ZKG_ERROR;                     // cosetFFT x3
        hipLaunchKernelGGL(k_pointwise_h_step, dim3(grid_m), dim3(256), 0, s, aA, aB, aC, m, sd->shape.big, sd->zinv.as<Fr>(),
                           (uint32_t)(sd->shape.big / sd->shape.small - 1), sd->zinv_small, crit);
        if (step_ntt_run(sd, aA, true, true, s, scr, 1, m)) return ZKG_ERROR;                      // icosetFFT
    }
    if (S.ev_ok) (void)hipEventRecord(S.ev[2], s);
    if (hipGetLastError() != hipSuccess) { set_error("prover kernel launch failed"); return ZKG_ERROR; }
    return ZKG_OK;
}

static constexpr size_t H_ROW_MERGE_MIN = 49152;                               // points from which H's windows share rows of buckets in pairs (slot_create)
int table_window_bits(size_t n) {                                    // window size of a query's table, by the size of the query
    int lg = 0; while (((size_t)1 << (lg + 1)) <= n) ++lg;
    // (re-measured in round 3 with the 29-bit kernels, tools/ch_sweep.sh + tools/prove_throughput.py: one payload, 2^15 - 1 points: c = 12 / 13 / 15 / 16
    //  -> 0.75 / 0.71 / 0.67 / 0.71 ms for a lone caller but 1907 / 1874 / 1632 / 1539 proofs/s with three callers, and no difference through
    //  the seam, whose witness pass dominates there: 17 windows x 2^14 buckets cost chip time that other proofs could use.  12 stays.)
    return lg >= 15 ? 16 : lg >= 9 ? 12 : 8;
}
static uint32_t h_row_merge(const zkg_crs *crs) {                             // (ZKG_H_ROW_MERGE: tuning aid)
    static const int force = getenv("ZKG_H_ROW_MERGE") ? atoi(getenv("ZKG_H_ROW_MERGE")) : 0;
    return force ? (uint32_t)force : (crs->H_query.n >= H_ROW_MERGE_MIN ? 2u : 1u);
}
static int slot_create(zkg_crs *crs, ProverSlot &S) {
    if (S.ready) return ZKG_OK;
    const size_t n = crs->n, m = crs->m;
    bool ok = S.z.reserve((n + 1) * 32) == 0 && S.aABC.reserve(3 * m * 32) == 0 && S.flag.reserve(16) == 0 && S.ntt_scratch.reserve(3 * m * NTT_SCRATCH_BYTES) == 0 &&
              S.wtags.reserve(n + 8) == 0 && S.wlisted.reserve((n + 1) * 4) == 0 && S.wcount.reserve(8) == 0 &&
              hip_ok(hipHostMalloc((void **)&S.flag_host, 64, hipHostMallocDefault), "hipHostMalloc", __FILE__, __LINE__);
    if (ok) {
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);             // numerically lower = higher priority
        // Four streams, so that each can have a hardware queue (a compute pipe) of its own — with more, two streams share a pipe and a
        // small kernel waits until every workgroup of the other stream's big kernel has been dispatched (seen in the kernel trace: the G1
        // witness job started 1.3 ms into a 1.9 ms proof):
        //   stream    upload, split, mat-vec, 7 NTTs and the H multi-exponentiation (H needs the NTTs anyway): the critical path
        //   job_w2    B_g2 over the non-bit witness elements (the longest latency chain)
        //   job_w1    A, B_g1 and L over the same elements, batched
        //   stream_o  the flat sums over the ones: B_g2, then A / B_g1 / L batched
        // ZKG_PRIO (tuning aid): bit 0 = `stream` high priority, bit 1 = witness jobs high, bit 2 = ones-sums high.
        static const char *pe = getenv("ZKG_PRIO");
        const int pr = pe ? atoi(pe) : 1;
        auto prio = [&](int bit) { return (pr >> bit) & 1 ? prio_hi : prio_lo; };
        ok = hip_ok(hipStreamCreateWithPriority(&S.stream, hipStreamNonBlocking, prio(0)), "hipStreamCreate", __FILE__, __LINE__);
        S.job_w1 = msm_job_create(nullptr, true, prio(1) == prio_hi); S.job_w2 = msm_job_create(nullptr, true, prio(1) == prio_hi);
        S.job_h = ok ? msm_job_create(S.stream, false) : nullptr;
        ok = ok && S.job_w1 && S.job_w2 && S.job_h &&
             hip_ok(hipStreamCreateWithPriority(&S.stream_o, hipStreamNonBlocking, prio(2)), "hipStreamCreate", __FILE__, __LINE__);
        if (ok) {                                                            // a table launch runs at the table's window size
            msm_job_set_window(S.job_w1, crs->c_w); msm_job_set_window(S.job_w2, crs->c_w); msm_job_set_window(S.job_h, crs->H_query.c);
            msm_job_set_critical(S.job_h, crit_priority_for(4, floor_log2(crs->m)));                              // the H query's multi-exponentiation ends the proof; the witness jobs beside it have slack
            // H: sixteen windows in eight rows of buckets from 49152 points on — where the unmerged launch already takes the two-pass sort
            // (2 / 4 / 8 payloads: 0.78 -> 0.72, 0.93 -> 0.88, 1.22 -> 1.17 ms; four rows at 8 payloads: 1.26 — one round of lanes, the
            // longest chain sets the time; one payload, 2^15 points: 0.75 -> 0.89, the doubled rows leave the one-pass sort's range)
            msm_job_set_row_merge(S.job_h, h_row_merge(crs));
        }
    }
    if (ok) {
        S.ev_ok = true;
        for (auto &e : S.ev) if (hipEventCreate(&e) != hipSuccess) S.ev_ok = false;
        if (!S.ev_ok) { set_error("hipEventCreate failed"); ok = false; }
    }
    if (ok) S.helper.start();
    S.ready = ok;
    return ok ? ZKG_OK : ZKG_ERROR;
}
static void slot_destroy(ProverSlot &S) {
    S.helper.shutdown();
    for (DevBuf *b : {&S.z, &S.aABC, &S.flag, &S.ntt_scratch, &S.up_tags, &S.up_idx, &S.up_vals, &S.wtags, &S.wlisted, &S.wcount, &S.zw_in}) b->release();
    if (S.zw_stage) (void)hipHostFree(S.zw_stage);
    S.zw_stage = nullptr; S.zw_stage_cap = 0;
    msm_job_destroy(S.job_w1); msm_job_destroy(S.job_w2); msm_job_destroy(S.job_h);
    S.job_w1 = S.job_w2 = S.job_h = nullptr;
    for (OnesSum *o : {&S.ones_g1, &S.ones_g2}) o->release();
    for (hipStream_t *st : {&S.stream, &S.stream_o}) { if (*st) (void)hipStreamDestroy(*st); *st = nullptr; }
    if (S.ev_ok) for (auto &e : S.ev) (void)hipEventDestroy(e);
    S.ev_ok = false;
    if (S.flag_host) (void)hipHostFree(S.flag_host);
    S.flag_host = nullptr; S.ready = false;
}

// proof bytes from the four multi-exponentiations' results (W1: A, B_1, L over the whole witness; the same algebra as prove_finish); proof_assemble.hpp
void assemble_proof(const ProofKey &key, const Fr &r, const Fr &s, const G1 W1[3], const G2 &Wb2, const G1 &Ht, uint8_t *out) {
    uint32_t rc[8], sc[8], rsc[8];
    canonical_limbs(r, rc); canonical_limbs(s, sc); canonical_limbs(r * s, rsc);
    G1 gA = G1::from_affine(key.alpha_g1); gA.add(key.delta1->mul(rc)); gA.add(W1[0]);                   // alpha + r delta + W_a
    G2 gB2 = G2::from_affine(key.beta_g2); gB2.add(key.delta2->mul(sc)); gB2.add(Wb2);                   // beta + s delta + W_b
    G1 gC = key.alpha1->mul(sc); gC.add(key.beta1->mul(rc)); gC.add(key.delta1->mul(rsc));               // s alpha + r beta_1 + rs delta
    gC.add(W1[0].mul(sc, 8)); gC.add(W1[1].mul(rc, 8)); gC.add(W1[2]); gC.add(Ht);                       // + s W_a + r W_b + L + H
    size_t off = ser_g1(out, gA);
    off += ser_g2(out + off, gB2);
    ser_g1(out + off, gC);
}
static ProofKey proof_key_of(const zkg_crs *crs) {
    ProofKey k; k.alpha_g1 = crs->alpha_g1; k.beta_g2 = crs->beta_g2;
    k.alpha1 = &crs->alpha1_comb; k.beta1 = &crs->beta1_comb; k.delta1 = &crs->delta1_comb; k.delta2 = &crs->delta2_comb;
    return k;
}
// ---- what a zkg_prover handle (prove_async.hip) borrows from the key
void crs_prover_view(const zkg_crs *crs, CrsProverView &v) {
    v.n = crs->n; v.l = crs->l; v.C = crs->C; v.m = crs->m; v.device = crs->device; v.h_sharded = !crs->h_shards.empty();
    const DevCsr *mtx[3] = {&crs->A, &crs->B, &crs->Cm};
    for (int k = 0; k < 3; ++k) { v.rp[k] = mtx[k]->rowptr.as<uint32_t>(); v.col[k] = mtx[k]->col.as<uint32_t>(); v.val[k] = mtx[k]->val.as<uint64_t>(); v.nnz[k] = mtx[k]->nnz; }
    v.H = &crs->H_query; v.h_row_merge = h_row_merge(crs);
    v.A_query = crs->A_query.as<G1Affine>(); v.B_g1 = crs->B_g1.as<G1Affine>(); v.L_query = crs->L_query.as<G1Affine>(); v.B_g2 = crs->B_g2.as<G2Affine>();
    v.key = proof_key_of(crs);
}
bool crs_prover_ref(zkg_crs *crs, int delta) {
    std::lock_guard<std::mutex> lk(crs->mu);
    if (delta > 0 && !crs->h_shards.empty()) return false;
    crs->provers += delta;
    return true;
}

}  // namespace zk

using namespace zk;

extern "C" {

static zkg_crs *zkg_crs_upload_impl(const zkg_pk *pk, bool queries_on_device = false, const std::function<bool()> &constraint_system_ready = nullptr) {
    if (!pk) { set_error("zkg_crs_upload: null pk"); return nullptr; }
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("zkg_crs_upload: no HIP device (call zkg_init)"); return nullptr; }
    const zkg_r1cs &cs = pk->cs;
    DomainShape shape;
    if (pk->log_m > 28 || !domain_shape_of(pk->domain_size ? (size_t)pk->domain_size : ((size_t)1 << pk->log_m), shape) || shape.log_m != pk->log_m ||
        ((size_t)cs.num_constraints + cs.num_inputs + 1) > shape.m || cs.num_inputs > cs.num_variables) {
        set_error("zkg_crs_upload: inconsistent sizes (domain must be 2^log_m or a step_radix2 size 2^(log_m-1) + 2^b)"); return nullptr;
    }
    auto t_begin = std::chrono::steady_clock::now();
    static const bool dbg_timing = getenv("ZKG_DEBUG_TIMING") != nullptr;
    auto lap = [&](const char *what) { if (dbg_timing) fprintf(stderr, "[zkg key upload] %-24s %8.3f ms\n", what, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count()); };
    zkg_crs *crs = new zkg_crs();
    crs->device = dev;
    crs->n = cs.num_variables; crs->l = cs.num_inputs; crs->C = cs.num_constraints; crs->log_m = pk->log_m; crs->m = shape.m;
    const size_t n = crs->n, l = crs->l, m = crs->m;
    bool ok = true;
    {
        // H becomes a per-window table (level 0 is the query as uploaded); A, B_g1, B_g2 and L go up as they are — their tables are built
        // over the elements the first proofs list (subset_extend).  They are indexed by the same witness and share one digit sort per
        // proof, so they share one window size; H has its own.
        static const char *cw = getenv("ZKG_TABLE_C_W"), *ch = getenv("ZKG_TABLE_C_H");                  // tuning aids
        // The witness tables' window is chosen when they are built, from the number of elements they cover (subset_extend); 0 = that rule.
        const int c_w = cw ? atoi(cw) : 0, c_h = ch ? atoi(ch) : table_window_bits(m - 1);
        crs->c_w_forced = c_w;
        // a query: from the host (zkg_pk as the ABI hands it over) or already on the device (the blob path decompresses there)
        auto query = [&](DevBuf &q, const uint64_t *src, size_t count, bool g2) {
            const size_t bytes = count * (g2 ? 128 : 64);
            if (q.reserve(bytes + 16)) return false;
            return !bytes || hip_ok(hipMemcpy(q.p, src, bytes, queries_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice), "query upload", __FILE__, __LINE__);
        };
        ok = (c_w == 0 || (c_w >= 2 && c_w <= 16)) && c_h >= 2 && c_h <= 16 &&
             query(crs->A_query, pk->A_query, n + 1, false) && query(crs->B_g1, pk->B_g1, n + 1, false) && query(crs->B_g2, pk->B_g2, n + 1, true) &&
             query(crs->L_query, pk->L_query, n - l, false);
        if (ok) {
            DevBuf stage; const G1Affine *h_dev = (const G1Affine *)pk->H_query;
            if (!queries_on_device) { ok = upload(stage, pk->H_query, (m - 1) * 64) == 0; h_dev = stage.as<G1Affine>(); }
            ok = ok && window_table_build_g1(crs->H_query, h_dev, m - 1, c_h, nullptr) == 0 && window_table_records29(crs->H_query, nullptr) == 0 &&
                 hip_ok(hipDeviceSynchronize(), "sync", __FILE__, __LINE__);
            stage.release();
        }
    }
    lap("queries up, H table built");
    if (ok) {
        memcpy(&crs->alpha_g1, pk->alpha_g1, 64); memcpy(&crs->beta_g1, pk->beta_g1, 64); memcpy(&crs->delta_g1, pk->delta_g1, 64);
        memcpy(&crs->beta_g2, pk->beta_g2, 128); memcpy(&crs->delta_g2, pk->delta_g2, 128);
        host_parallel_for(4, [&](int i) {
            if (i == 0) crs->delta2_comb.build(crs->delta_g2); else if (i == 1) crs->delta1_comb.build(crs->delta_g1);
            else if (i == 2) crs->alpha1_comb.build(crs->alpha_g1); else crs->beta1_comb.build(crs->beta_g1);
        });
        if (shape.step) crs->sdom = step_domain(shape.m, nullptr); else crs->dom = ntt_domain(pk->log_m, nullptr);
        ok = crs->dom != nullptr || crs->sdom != nullptr;
    }
    if (ok && crs->dom) {
        Fr g = Fr::from_u64(5);
        crs->z_inv_coset = (g.pow_u64(m) - Fr::one()).inverse();           // basic_radix2_domain::divide_by_Z_on_coset
        ok = crs->coset_over_m.reserve(m * 32) == 0 && powers_table(crs->coset_over_m.as<Fr>(), m, g, crs->dom->n_inv, nullptr) == 0 &&
             ntt_table29(crs->coset_over_m29, crs->coset_over_m.as<Fr>(), m, nullptr) == 0;
    }
    lap("comb tables + domain");
    ok = ok && hip_ok(hipDeviceSynchronize(), "sync", __FILE__, __LINE__) && slot_create(crs, crs->slot[0]) == ZKG_OK;
    lap("prover slot created");
    // the constraint system last — behind the comb tables, the domain and the prover slot, which do not need it: the blob path parses it on another
    // thread meanwhile (8 payloads: the parse ends 2.4 ms after the H table stands; what used to follow it was 4.8 ms, now 1.2)
    if (ok && constraint_system_ready && !constraint_system_ready()) ok = false;
    ok = ok && upload_csr(crs->A, cs.a_rowptr, cs.a_col, cs.a_val, crs->C) == 0 && upload_csr(crs->B, cs.b_rowptr, cs.b_col, cs.b_val, crs->C) == 0 &&
         upload_csr(crs->Cm, cs.c_rowptr, cs.c_col, cs.c_val, crs->C) == 0;
    if (ok) {                                                                // rows left to the wavefront-per-row kernel
        std::vector<uint32_t> lr;
        const uint32_t *rps[3] = {cs.a_rowptr, cs.b_rowptr, cs.c_rowptr};
        for (uint32_t mtx = 0; mtx < 3; ++mtx)
            for (uint32_t r = 0; r < crs->C; ++r) if (rps[mtx][r + 1] - rps[mtx][r] > LONG_ROW) lr.push_back((mtx << 30) | r);
        crs->n_long = (uint32_t)lr.size();
        ok = crs->C < (1u << 30) && upload(crs->long_rows, lr.data(), lr.size() * 4) == 0;
    }
    ok = ok && hip_ok(hipDeviceSynchronize(), "sync", __FILE__, __LINE__);
    lap("constraint system up");
    if (!ok) { zkg_crs_free(crs); return nullptr; }
    return crs;
}
zkg_crs *zkg_crs_upload(const zkg_pk *pk) { return c_boundary<zkg_crs *>("zkg_crs_upload", nullptr, [&] { return zkg_crs_upload_impl(pk); }); }

static void slot_release_h_runs(ProverSlot &S) {                              // leaves the current device changed; callers restore it
    for (auto &r : S.h_runs) {
        (void)hipSetDevice(r.device);
        if (r.job) { (void)hipStreamSynchronize(msm_job_stream(r.job)); msm_job_destroy(r.job); }
        r.scalars.release();
    }
    S.h_runs.clear();
}
static void batch_destroy(BatchWs &B);
void zkg_crs_free(zkg_crs *crs) {
    if (!crs) return;
    for (DevBuf *b : {&crs->A.rowptr, &crs->A.col, &crs->A.val, &crs->B.rowptr, &crs->B.col, &crs->B.val, &crs->Cm.rowptr, &crs->Cm.col, &crs->Cm.val,
                      &crs->coset_over_m, &crs->coset_over_m29, &crs->long_rows})
        b->release();
    for (WindowTable *t : {&crs->H_query, &crs->sub.A, &crs->sub.B1, &crs->sub.B2, &crs->sub.L}) t->release();
    for (DevBuf *b : {&crs->A_query, &crs->B_g1, &crs->B_g2, &crs->L_query, &crs->sub.pos, &crs->sub.idx}) b->release();
    int cur = 0; (void)hipGetDevice(&cur);
    for (ProverSlot &S : crs->slot) slot_release_h_runs(S);
    for (auto &sh : crs->h_shards) { (void)hipSetDevice(sh.device); sh.table.release(); }
    (void)hipSetDevice(cur);
    for (ProverSlot &S : crs->slot) slot_destroy(S);
    batch_destroy(crs->batch);
    delete crs;
}

uint32_t zkg_crs_num_variables(const zkg_crs *crs) { return crs ? crs->n : 0; }

// the largest number of proofs any one key has had in flight at once since the last reset (zkg_prover_peak_in_flight): what a test of
// "callers run side by side" can assert without a stopwatch
static std::atomic<int> g_peak_in_flight{0};
// A caller's hold on one prover slot of a key (see zkg_crs): blocks until a slot is free and no table extension is pending.
struct SlotLease {
    zkg_crs *crs; int i = -1;
    explicit SlotLease(zkg_crs *c) : crs(c) {
        // how many proofs of this key may be in flight: measured proofs per second with 1 / 2 / 3 callers — one payload (m = 2^15) 1069 /
        // 1142 / 1706, eight payloads (2^18) 609 / 698 / 576, 37 payloads (2^20) 250 / 247.  ZKG_PROVER_SLOTS caps it (1 = callers queue).
        static const int env_slots = [] { const char *e = getenv("ZKG_PROVER_SLOTS"); int v = e ? atoi(e) : zkg_crs::MAX_SLOTS; return v < 1 ? 1 : v > zkg_crs::MAX_SLOTS ? zkg_crs::MAX_SLOTS : v; }();
        const int max_slots = std::min(env_slots, c->m < ((size_t)1 << 18) ? 3 : c->m < ((size_t)1 << 19) ? 2 : 1);
        std::unique_lock<std::mutex> lk(crs->mu);
        for (;;) {
            if (!crs->extending && crs->waiting_ext == 0) {
                int pick = -1;
                for (int k = 0; k < max_slots && pick < 0; ++k) if (!crs->busy[k] && crs->slot[k].ready) pick = k;
                for (int k = 0; k < max_slots && pick < 0; ++k) if (!crs->busy[k]) pick = k;              // not created yet
                if (pick >= 0) {
                    crs->busy[pick] = true; ++crs->leases;
                    { int seen = g_peak_in_flight.load(std::memory_order_relaxed); while (crs->leases > seen && !g_peak_in_flight.compare_exchange_weak(seen, crs->leases)) {} }
                    if (crs->slot[pick].ready) { i = pick; return; }
                    lk.unlock();
                    const int rc = slot_create(crs, crs->slot[pick]);                                     // device allocations: outside the lock
                    lk.lock();
                    if (rc == ZKG_OK) { i = pick; return; }
                    slot_destroy(crs->slot[pick]);
                    crs->busy[pick] = false; --crs->leases; crs->cv.notify_all();
                    if (pick == 0) return;                                                                // not even one slot: give up (i stays -1)
                    // no memory for another slot: wait for one of the existing ones
                    crs->cv.wait(lk, [&] { for (int k = 0; k < max_slots; ++k) if (!crs->busy[k] && crs->slot[k].ready) return true; return false; });
                    continue;
                }
            }
            crs->cv.wait(lk);
        }
    }
    ~SlotLease() {
        if (i < 0) return;
        std::lock_guard<std::mutex> lk(crs->mu);
        crs->busy[i] = false; --crs->leases; crs->cv.notify_all();
    }
    bool ok() const { return i >= 0; }
    ProverSlot &S() { return crs->slot[i]; }
};

static int zkg_qap_witness_h_impl(const zkg_crs *crs_, const uint64_t *witness, uint64_t *h_out) {
    zkg_crs *crs = const_cast<zkg_crs *>(crs_);
    if (!crs || !h_out || (crs->n && !witness)) { set_error("zkg_qap_witness_h: bad argument"); return ZKG_ERROR; }
    SlotLease lease(crs);
    if (!lease.ok()) return ZKG_ERROR;
    ProverSlot &S = lease.S();
    WitnessSrc W; W.dense = witness;
    if (compute_h_matvec(crs, S, W, false) || compute_h_transforms(crs, S)) return ZKG_ERROR;
    ZK_HIP(hipStreamSynchronize(S.stream));
    ZK_HIP(hipMemcpy(h_out, S.aABC.p, crs->m * 32, hipMemcpyDeviceToHost));
    memset(h_out + 4 * crs->m, 0, 32);                                      // coefficients_for_H[m] = 0
    return ZKG_OK;
}
int zkg_qap_witness_h(const zkg_crs *crs, const uint64_t *witness, uint64_t *h_out) {
    return c_boundary("zkg_qap_witness_h", ZKG_ERROR, [&] { return zkg_qap_witness_h_impl(crs, witness, h_out); });
}

// ---- one proof = prove_enqueue (everything the GPU does, queued without waiting) + prove_finish (host tails, assembly, bytes)
static const bool g_dbg_timing = getenv("ZKG_DEBUG_TIMING") != nullptr, g_serial_msm = getenv("ZKG_SERIAL_MSM") != nullptr;
// ZKG_WITNESS_START (tuning aid): which event the witness streams wait for — 0 the split (default), 1 the mat-vec, 2 the transforms
static const int g_witness_start = [] { const char *e = getenv("ZKG_WITNESS_START"); int v = e ? atoi(e) : 0; return v >= 0 && v <= 2 ? v : 0; }();
static void lap(const ProverSlot &S, const char *what) {
    if (g_dbg_timing) fprintf(stderr, "[zkg] %-22s %8.3f ms\n", what, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - S.t0).count());
}
static MsmBases table_set(const WindowTable &t, bool g2, uint32_t index_sub, const uint32_t *remap = nullptr) {       // (a table not built yet is empty, not G1)
    MsmBases b; b.p = t.buf.p; b.g2 = g2; b.level_stride = t.n; b.index_sub = index_sub; b.remap = remap; b.p29 = t.rec29.p; return b;
}
static MsmBases query_set(const DevBuf &q, bool g2, uint32_t index_sub) { MsmBases b; b.p = q.p; b.g2 = g2; b.index_sub = index_sub; return b; }

// The witness tables grow to cover `listed` more elements (the first proof on a key; later only when a witness has a non-bit value where
// every earlier one had a bit).  Host: membership -> ascending element list and positions; device: level 0 gathered from the queries, then
// the levels.  Runs on the helper thread with the ones-sum stream, which has nothing of this proof queued yet.
static int subset_extend(zkg_crs *crs, ProverSlot &S, size_t listed, const std::vector<uint32_t> *listed_host /* a batch: the union of its witnesses' lists; or null: the slot's list */) {
    zkg_crs::SubsetTables &T = crs->sub;
    const size_t n1 = (size_t)crs->n + 1; hipStream_t s = S.stream_o;
    // From here until one of the two success exits the key has NO witness tables: pos / idx / the tables / the window size are rewritten
    // below in several steps, and a failure between them (a device allocation under memory pressure) must leave a state the next proof
    // recognises — count == 0 sends it back here — instead of old tables under a new position map.
    T.count = 0;
    const auto t_ext0 = std::chrono::steady_clock::now();
    auto ext_lap = [&](const char *w) { if (g_dbg_timing) fprintf(stderr, "[zkg]       subset_extend %-28s %8.3f ms\n", w, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_ext0).count()); };
    std::vector<uint32_t> li;
    if (listed_host) li = *listed_host;
    else {
        li.resize(listed);
        ZK_HIP(hipMemcpyAsync(li.data(), S.wlisted.p, listed * 4, hipMemcpyDeviceToHost, s));
        ZK_HIP(hipStreamSynchronize(s));
    }
    if (T.member.empty()) T.member.assign(n1, 0);
    for (uint32_t i : li) { if (i >= n1) { set_error("prover: witness split out of range"); return ZKG_ERROR; } T.member[i] = 1; }
    std::vector<uint32_t> pos(n1, SUBSET_NONE), idx;
    idx.reserve(listed + T.count);
    for (size_t i = 0; i < n1; ++i) if (T.member[i]) { pos[i] = (uint32_t)idx.size(); idx.push_back((uint32_t)i); }
    const size_t count = idx.size();
    ext_lap("listed read, positions built");
    if (T.pos.reserve(n1 * 4) || T.idx.reserve(count * 4 + 16)) return ZKG_ERROR;
    ZK_HIP(hipMemcpyAsync(T.pos.p, pos.data(), n1 * 4, hipMemcpyHostToDevice, s));
    ZK_HIP(hipMemcpyAsync(T.idx.p, idx.data(), count * 4, hipMemcpyHostToDevice, s));
    // Window size: only the non-bit elements of a witness reach the bucket method — a credential's values, packings and public inputs,
    // ~30 per payload, a thousand of a million variables at 37 payloads — so the window is sized for `count` entries per window, about one
    // per bucket: c = log2(count) + 2 within [10, 14] (measured flat between 10 and 14 at 8 and 37 payloads, 3 - 5 % slower at 16).  Small
    // bucket sets keep this latency-bound work light: the digit sort's LDS histogram is 2^(c-1) counters, the fold and the reduction
    // shrink with it.
    int lg_count = 0; while (((size_t)1 << (lg_count + 1)) <= count) ++lg_count;
    const int c_new = crs->c_w_forced ? crs->c_w_forced : std::min(14, std::max(10, lg_count + 2));     // becomes crs->c_w once the tables stand
    ScopedDevBuf stage, stage2;                                                                       // released on every way out
    if (stage.reserve(3 * count * sizeof(G1Affine) + 16) || stage2.reserve(count * sizeof(G2Affine) + 16)) return ZKG_ERROR;
    const uint32_t *d_idx = T.idx.as<uint32_t>();
    static const size_t host_limit = getenv("ZKG_SUBSET_HOST_LIMIT") ? (size_t)atoi(getenv("ZKG_SUBSET_HOST_LIMIT")) : 1024;   // tuning aid
    if (count <= host_limit) {
        // A small subset (every credential size zklaim's benchmark covers): on the GPU each table is a chain of 254 doublings and W / 4
        // inversions per lane whatever the count — 10 ms for 22 points; the host pool walks the same chains at 0.08 ms per G1 point (0.25 ms
        // per G2 point), a task per (table, point), and uploads the finished levels.  Same-box A/B: 8 ms less at 12 payloads (324
        // elements), 6 ms less at 20 (552); the costs meet around a thousand elements.
        G1Affine *d1 = stage.as<G1Affine>();
        int rc = gather_points_g1(crs->A_query.as<G1Affine>(), d_idx, count, 0, d1, s) || gather_points_g1(crs->B_g1.as<G1Affine>(), d_idx, count, 0, d1 + count, s) ||
                 gather_points_g1(crs->L_query.as<G1Affine>(), d_idx, count, (uint32_t)(crs->l + 1), d1 + 2 * count, s) ||
                 gather_points_g2(crs->B_g2.as<G2Affine>(), d_idx, count, 0, stage2.as<G2Affine>(), s);
        std::vector<G1Affine> p1(3 * count); std::vector<G2Affine> p2(count);
        const bool got = !rc && hip_ok(hipMemcpyAsync(p1.data(), d1, 3 * count * sizeof(G1Affine), hipMemcpyDeviceToHost, s), "D2H", __FILE__, __LINE__) &&
                         hip_ok(hipMemcpyAsync(p2.data(), stage2.p, count * sizeof(G2Affine), hipMemcpyDeviceToHost, s), "D2H", __FILE__, __LINE__) &&
                         hip_ok(hipStreamSynchronize(s), "sync", __FILE__, __LINE__);
        stage.release(); stage2.release();
        if (!got) return ZKG_ERROR;
        ext_lap("points gathered and read back");
        const int c = c_new, W = (254 + c) / c;                               // = (SCALAR_BITS + c - 1) / c of window_table_build
        std::vector<G1Affine> t1((size_t)3 * W * count); std::vector<G2Affine> t2((size_t)W * count);
        auto levels = [&](auto base, auto *out /* level w of this point at out[w * count] */) {
            typedef decltype(base.x) F;
            if (base.is_inf()) { for (int w = 0; w < W; ++w) out[(size_t)w * count] = base; return; }
            std::vector<XYZZ<F>> lv(W);
            XYZZ<F> p = XYZZ<F>::from_affine(base);
            for (int w = 1; w < W; ++w) { for (int k = 0; k < c; ++k) p = p.dbl(); lv[w] = p; }
            std::vector<F> pre(W); F run = F::one();
            for (int w = 1; w < W; ++w) { pre[w] = run; if (!lv[w].is_inf()) run = run * lv[w].zzz; }
            F inv = run.inverse();
            out[0] = base;
            for (int w = W - 1; w >= 1; --w) {
                if (lv[w].is_inf()) { out[(size_t)w * count] = decltype(base)::inf(); continue; }
                F zi = inv * pre[w]; inv = inv * lv[w].zzz;
                F z1 = zi * lv[w].zz, zi2 = z1.sqr();
                out[(size_t)w * count] = {lv[w].x * zi2, lv[w].y * zi};
            }
        };
        host_parallel_for_wait((int)(4 * count), [&](int task) {
            const size_t tb = (size_t)task / count, i = (size_t)task % count;
            if (tb < 3) levels(p1[tb * count + i], &t1[tb * (size_t)W * count + i]); else levels(p2[i], &t2[i]);
        });
        ext_lap("levels on the host pool");
        WindowTable *g1t[3] = {&T.A, &T.B1, &T.L};
        bool up = true;
        for (int tb = 0; tb < 3 && up; ++tb) {
            WindowTable &t = *g1t[tb]; t.n = count; t.c = c; t.W = W; t.g2 = false;
            up = t.buf.reserve((size_t)W * count * sizeof(G1Affine)) == 0 &&
                 hip_ok(hipMemcpyAsync(t.buf.p, &t1[tb * (size_t)W * count], (size_t)W * count * sizeof(G1Affine), hipMemcpyHostToDevice, s), "H2D", __FILE__, __LINE__);
        }
        T.B2.n = count; T.B2.c = c; T.B2.W = W; T.B2.g2 = true;
        up = up && T.B2.buf.reserve((size_t)W * count * sizeof(G2Affine)) == 0 &&
             hip_ok(hipMemcpyAsync(T.B2.buf.p, t2.data(), (size_t)W * count * sizeof(G2Affine), hipMemcpyHostToDevice, s), "H2D", __FILE__, __LINE__);
        up = hip_ok(hipStreamSynchronize(s), "sync", __FILE__, __LINE__) && up;          // (host vectors go out of scope)
        if (!up) return ZKG_ERROR;
        ext_lap("tables uploaded");
        crs->c_w = c_new; T.count = count; ++T.rebuilds;
        if (g_dbg_timing) fprintf(stderr, "[zkg]     witness tables over %zu of %zu elements (rebuild %u, levels on the host)\n", count, n1, T.rebuilds);
        return ZKG_OK;
    }
    // the G2 table on the B_g2 job's stream (idle as well), beside the three G1 tables: a few thousand points per launch are latency chains
    hipStream_t s2 = msm_job_stream(S.job_w2);
    bool ok = hip_ok(hipEventRecord(S.ev[11], s), "event", __FILE__, __LINE__) && hip_ok(hipStreamWaitEvent(s2, S.ev[11], 0), "wait", __FILE__, __LINE__);   // idx is up
    int rc = !ok || gather_points_g2(crs->B_g2.as<G2Affine>(), d_idx, count, 0, stage2.as<G2Affine>(), s2) || window_table_build_g2(T.B2, stage2.as<G2Affine>(), count, c_new, s2) ||
             gather_points_g1(crs->A_query.as<G1Affine>(), d_idx, count, 0, stage.as<G1Affine>(), s) || window_table_build_g1(T.A, stage.as<G1Affine>(), count, c_new, s) ||
             gather_points_g1(crs->B_g1.as<G1Affine>(), d_idx, count, 0, stage.as<G1Affine>(), s) || window_table_build_g1(T.B1, stage.as<G1Affine>(), count, c_new, s) ||
             gather_points_g1(crs->L_query.as<G1Affine>(), d_idx, count, (uint32_t)(crs->l + 1), stage.as<G1Affine>(), s) || window_table_build_g1(T.L, stage.as<G1Affine>(), count, c_new, s);
    const bool synced1 = hip_ok(hipStreamSynchronize(s), "sync", __FILE__, __LINE__), synced2 = hip_ok(hipStreamSynchronize(s2), "sync", __FILE__, __LINE__);
    const bool synced = synced1 && synced2;                                     // (both streams waited for: host vectors and staging go out of scope)
    stage.release(); stage2.release();
    if (rc || !synced) return ZKG_ERROR;
    crs->c_w = c_new; T.count = count; ++T.rebuilds;
    if (g_dbg_timing) fprintf(stderr, "[zkg]     witness tables over %zu of %zu elements (rebuild %u)\n", count, n1, T.rebuilds);
    return ZKG_OK;
}
// subset_extend under the key's protocol (see zkg_crs): the tables are shared by the key's slots, so the caller — holding its lease — waits until
// every other proof in flight has finished or waits here too, extends alone, and lets the others go on.  No new proof starts meanwhile.
static int extend_tables_exclusive(zkg_crs *crs, ProverSlot &S, size_t listed, const std::vector<uint32_t> *host_list) {
    std::unique_lock<std::mutex> lk(crs->mu);
    ++crs->waiting_ext; crs->cv.notify_all();
    crs->cv.wait(lk, [&] { return !crs->extending && crs->leases - crs->waiting_ext == 0; });
    --crs->waiting_ext; crs->extending = true;
    lk.unlock();
    int rc = ZKG_ERROR;
    try { rc = subset_extend(crs, S, listed, host_list); } catch (...) { set_error("prover: witness table extension failed"); }   // the flag below must be cleared whatever happens
    lk.lock();
    crs->extending = false; crs->cv.notify_all();
    return rc;
}
// ---- H over several devices: launch (after the transforms, in the slot's stream order) and finish
static int h_shards_launch(zkg_crs *crs, ProverSlot &S) {
    int cur = 0; (void)hipGetDevice(&cur);
    struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{cur};
    if (S.h_epoch != crs->h_epoch) {                                       // this slot's first proof under this sharding: a job and a buffer per shard
        slot_release_h_runs(S);
        S.h_runs.resize(crs->h_shards.size());
        for (size_t i = 0; i < crs->h_shards.size(); ++i) {
            ProverSlot::HShardRun &run = S.h_runs[i];
            run.device = crs->h_shards[i].device;
            ZK_HIP(hipSetDevice(run.device));
            run.job = msm_job_create(nullptr, true);
            if (!run.job || run.scalars.reserve(crs->h_shards[i].n * 32 + 16)) { set_error("prover: H shard workspace"); return ZKG_ERROR; }
            msm_job_set_window(run.job, crs->h_shards[i].table.c); msm_job_set_row_merge(run.job, crs->h_shards[i].n >= H_ROW_MERGE_MIN ? 2u : 1u);
        }
        S.h_epoch = crs->h_epoch;
    }
    // ev[2]: coefficients_for_H complete on the slot's stream (recorded by compute_h_transforms)
    const Fr *coeff = S.aABC.as<Fr>();
    for (size_t i = 0; i < crs->h_shards.size(); ++i) {
        const zkg_crs::HShard &sh = crs->h_shards[i]; ProverSlot::HShardRun &run = S.h_runs[i];
        ZK_HIP(hipSetDevice(sh.device));
        hipStream_t st = msm_job_stream(run.job);
        ZK_HIP(hipStreamWaitEvent(st, S.ev[2], 0));
        ZK_HIP(hipMemcpyAsync(run.scalars.p, coeff + sh.first, sh.n * 32, hipMemcpyDefault, st));       // peer copy over xGMI (or a device copy on one GPU)
        const MsmBases h = table_set(sh.table, false, 0);
        if (msm_job_launch(run.job, &h, 1, run.scalars.as<uint32_t>(), sh.n, true)) return ZKG_ERROR;
    }
    return ZKG_OK;
}
static int h_shards_finish(zkg_crs *crs, ProverSlot &S, G1 &out) {
    int cur = 0; (void)hipGetDevice(&cur);
    struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{cur};
    out = G1::inf();
    for (size_t i = 0; i < crs->h_shards.size(); ++i) {
        ZK_HIP(hipSetDevice(crs->h_shards[i].device));
        G1 part;
        if (msm_job_finish(S.h_runs[i].job, &part, nullptr)) return ZKG_ERROR;
        out.add(part);
    }
    return ZKG_OK;
}

// event slots: 0 witness resident + split done, 1 mat-vec done, 2 H coefficients done, 3 satisfiability flag landed,
//              4-5 G1 witness job, 6-7 G2 witness job, 8-9 H job, 10 G2 ones-sum landed, 11 table extension, 12 the caller's stream (zkg_groth16_prove_dev)
static int prove_enqueue(zkg_crs *crs, ProverSlot &S, const WitnessSrc &witness, const uint64_t r_[4], const uint64_t s_[4], bool check) {
    S.t0 = std::chrono::steady_clock::now();
    S.check = check; memcpy(S.r.v, r_, 32); memcpy(S.s.v, s_, 32);
    S.flag_host[0] = 0; S.flag_host[1] = 0; S.flag_host[2] = 0; S.flag_host[3] = 0; S.flag_host[4] = 0; S.zw_state = ZW_NONE;
    if (compute_h_matvec(crs, S, witness, check)) return ZKG_ERROR;
    lap(S, "upload + mat-vec enqueued");
    const size_t n = crs->n, l = crs->l, m = crs->m;
    // The witness queries (libff multi_exp_with_mixed_addition): zeros skipped, ones summed flat, the rest — 0.1 % of a credential's
    // witness — through the bucket method as a gathered subset.  The count of "the rest" sizes the launches, so a helper thread waits
    // for the split (event 0), reads it and queues the four witness streams' work while this thread queues the critical path.
    auto witness_fn = [&]() -> int {
        ZK_HIP(hipEventSynchronize(S.ev[0]));
        lap(S, "  (helper) split landed");
        const size_t listed = S.flag_host[1];
        if (witness.plan && S.flag_host[4]) { S.zw_state = ZW_GENERATOR_ERROR; set_error("zklaim witness generator: a cursor left its range (the host witness is used)"); return ZKG_ERROR; }
        if (S.flag_host[3]) { set_error("prover: a listed witness index is out of range, not tagged 2 or listed twice"); return ZKG_ERROR; }
        if (listed > n + 1) { set_error("prover: witness split out of range"); return ZKG_ERROR; }
        const uint8_t *tags = S.wtags.as<uint8_t>(); const uint32_t *gather = S.wlisted.as<uint32_t>(), *z = S.z.as<uint32_t>();
        if (listed && (S.flag_host[2] || !crs->sub.count) && extend_tables_exclusive(crs, S, listed, nullptr)) return ZKG_ERROR;
        msm_job_set_window(S.job_w1, crs->c_w); msm_job_set_window(S.job_w2, crs->c_w);   // (another slot's proof may have built the tables)
        const uint32_t *pos = crs->sub.pos.as<uint32_t>();
        // bucket method: the subset tables, addressed through the element positions; flat sums over the ones: the queries as uploaded
        const MsmBases g1[3] = {table_set(crs->sub.A, false, 0, pos), table_set(crs->sub.B1, false, 0, pos), table_set(crs->sub.L, false, 0, pos)}, b2 = table_set(crs->sub.B2, true, 0, pos);
        const MsmBases o1[3] = {query_set(crs->A_query, false, 0), query_set(crs->B_g1, false, 0), query_set(crs->L_query, false, (uint32_t)(l + 1))},
                       o2 = query_set(crs->B_g2, true, 0);
        // ZKG_WITNESS_START (tuning aid): which event the witness streams wait for — 0 the split (default), 1 the mat-vec, 2 the transforms
        hipEvent_t go = S.ev[g_witness_start];
        {
            hipStream_t js = msm_job_stream(S.job_w2);                         // G2 first: the longest chains
            ZK_HIP(hipStreamWaitEvent(S.stream_o, go, 0));
            if (ones_sum_launch(S.ones_g2, &o2, 1, tags, n + 1, S.stream_o)) return ZKG_ERROR;
            lap(S, "  (helper) G2 ones-sum enqueued");
            (void)hipEventRecord(S.ev[10], S.stream_o);                        // the G2 sum has landed (the G1 sums follow on the same stream)
            if (g_serial_msm) (void)hipStreamSynchronize(S.stream_o);          // (profiling aid: the flat sum alone on the chip, then the job's kernels)
            ZK_HIP(hipStreamWaitEvent(js, go, 0));
            (void)hipEventRecord(S.ev[6], js);
            if (msm_job_launch(S.job_w2, &b2, 1, z, listed, true, gather)) return ZKG_ERROR;
            lap(S, "  (helper) G2 job enqueued");
            (void)hipEventRecord(S.ev[7], js);
            if (g_serial_msm) { (void)hipStreamSynchronize(S.stream_o); (void)hipStreamSynchronize(js); }
        }
        {
            hipStream_t js = msm_job_stream(S.job_w1);
            if (ones_sum_launch(S.ones_g1, o1, 3, tags, n + 1, S.stream_o)) return ZKG_ERROR;
            lap(S, "  (helper) G1 ones-sums enqueued");
            if (g_serial_msm) (void)hipStreamSynchronize(S.stream_o);
            ZK_HIP(hipStreamWaitEvent(js, go, 0));
            (void)hipEventRecord(S.ev[4], js);
            if (msm_job_launch(S.job_w1, g1, 3, z, listed, true, gather)) return ZKG_ERROR;
            (void)hipEventRecord(S.ev[5], js);
            if (g_serial_msm) { (void)hipStreamSynchronize(S.stream_o); (void)hipStreamSynchronize(js); }
        }
        return ZKG_OK;
    };
    const bool helper = !g_serial_msm && g_witness_start == 0;                  // a later start event must have been recorded before it is waited for
    if (helper) S.helper.submit(witness_fn);
    int rc = compute_h_transforms(crs, S);
    lap(S, "transforms enqueued");
    // H: uniformly random scalars, follows the transforms in stream order
    if (rc == ZKG_OK) {
        hipStream_t js = msm_job_stream(S.job_h);                              // == S.stream
        (void)hipEventRecord(S.ev[8], js);
        if (!crs->h_shards.empty()) rc = h_shards_launch(crs, S);
        else {
        const MsmBases h = table_set(crs->H_query, false, 0);
        rc = msm_job_launch(S.job_h, &h, 1, S.aABC.as<uint32_t>(), m - 1, true);
        }
        (void)hipEventRecord(S.ev[9], js);
        if (g_serial_msm) (void)hipStreamSynchronize(js);
    }
    const int rc_w = helper ? S.helper.wait() : witness_fn();          // (profiling aid: every job alone on the chip, one after the other)
    lap(S, "msm jobs enqueued");
    return rc == ZKG_OK ? rc_w : rc;
}
static void slot_drain(const zkg_crs *, ProverSlot &S) {                      // after an error: nothing of this slot may still be running
    (void)hipStreamSynchronize(S.stream);
    for (MsmJob *j : {S.job_w1, S.job_w2, S.job_h}) if (j) (void)hipStreamSynchronize(msm_job_stream(j));
    if (S.stream_o) (void)hipStreamSynchronize(S.stream_o);
    for (auto &r : S.h_runs) if (r.job) (void)hipStreamSynchronize(msm_job_stream(r.job));
}
static int prove_finish(zkg_crs *crs, ProverSlot &S, uint8_t *proof_out, size_t *proof_len) {
    hipStream_t s = S.stream;
    G1 W1[3]; G2 Bt2; G1 Ht;
    // host work that needs only the key and (r, s), from the fixed-base tables: overlaps the GPU.
    //   A = alpha + W_a + r delta,  B = beta + W_b + s delta (in G2, and its copy B_1 in G1),
    //   C = H + L + s A + r B_1 - rs delta = H + L + (s alpha + r beta_1 + rs delta) + s W_a + r W_b
    // (W_a, W_b, L, H: the four multi-exponentiations).  The same group elements as libsnark's expression order gives; bytes identical.
    uint32_t rc[8], sc[8], rsc[8];
    canonical_limbs(S.r, rc); canonical_limbs(S.s, sc); canonical_limbs(S.r * S.s, rsc);
    G1 gA = G1::from_affine(crs->alpha_g1); gA.add(crs->delta1_comb.mul(rc));                          // alpha + r delta
    G1 c_fixed = crs->alpha1_comb.mul(sc); c_fixed.add(crs->beta1_comb.mul(rc)); c_fixed.add(crs->delta1_comb.mul(rsc));   // s alpha + r beta_1 + rs delta
    G2 gB2 = G2::from_affine(crs->beta_g2); gB2.add(crs->delta2_comb.mul(sc));                         // beta + s delta
    lap(S, "key-only host products");
    if (S.check) {
        ZK_HIP(hipEventSynchronize(S.ev[3]));
        if (S.flag_host[0]) {                                                // drain the speculative MSMs, then refuse like snark.cpp:121-124
            slot_drain(crs, S);
            set_error("constraint system not satisfied; not creating proof"); return ZKG_UNSATISFIED;
        }
    }
    // ---- finish + assembly (host), ordered so that nothing the GPU has already delivered waits for what it is still computing
    if (msm_job_finish(S.job_w1, W1, nullptr) || !hip_ok(hipStreamSynchronize(S.stream_o), "sync", __FILE__, __LINE__)) { slot_drain(crs, S); return ZKG_ERROR; }
    lap(S, "A, B_1, L landed");
    for (int i = 0; i < 3; ++i) W1[i].add(S.ones_g1.g1(i));                   // bucket method over the non-bit elements + flat sum over the ones
    // the two variable-base products s W_a and r W_b: the second one on a helper thread
    G1 rWb;
    S.helper.submit([&]() -> int { rWb = W1[1].mul(rc, 8); return ZKG_OK; });
    G1 gC = W1[0].mul(sc, 8);
    gA.add(W1[0]);
    size_t off = 0;
    off += ser_g1(proof_out + off, gA);
    (void)S.helper.wait();
    gC.add(rWb); gC.add(c_fixed); gC.add(W1[2]);
    lap(S, "A serialised, s*Wa + r*Wb + L");
    if (msm_job_finish(S.job_w2, nullptr, &Bt2) || !hip_ok(hipEventSynchronize(S.ev[10]), "sync", __FILE__, __LINE__)) { slot_drain(crs, S); return ZKG_ERROR; }
    lap(S, "B_2 landed");
    Bt2.add(S.ones_g2.g2pt(0));
    gB2.add(Bt2);
    off += ser_g2(proof_out + off, gB2);
    lap(S, "B serialised");
    if (crs->h_shards.empty() ? msm_job_finish(S.job_h, &Ht, nullptr) : h_shards_finish(crs, S, Ht)) { slot_drain(crs, S); return ZKG_ERROR; }
    lap(S, "H landed");
    gC.add(Ht);                                                             // C = H_t + L_t + s A + r B_1 - rs delta
    off += ser_g1(proof_out + off, gC);
    *proof_len = off;
    lap(S, "assembled+serialised");
    ZK_HIP(hipStreamSynchronize(s));
    {
        float t;
        auto el = [&](int a, int b) { return hipEventElapsedTime(&t, S.ev[a], S.ev[b]) == hipSuccess ? t : -1.f; };
        S.stage_ms[0] = el(0, 1); S.stage_ms[1] = el(1, 2); S.stage_ms[2] = el(4, 5); S.stage_ms[3] = 0.f; S.stage_ms[4] = el(6, 7);
        S.stage_ms[5] = el(8, 9); S.stage_ms[6] = 0.f;
        S.stage_ms[7] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - S.t0).count();
        for (int i = 0; i < 8; ++i) crs->stage_ms[i] = S.stage_ms[i];
    }
    return ZKG_OK;
}

// A dense witness whose variables are mostly bits (a credential circuit's: 97 %) is cheaper to SCAN on the host pool than to upload: 32 bytes per
// variable over PCIe (0.58 ms at 2^20 variables) against a read of the same bytes from host memory in 32 chunks (~0.2 ms) and an upload of one tag byte per
// variable plus the listed values — the sparse form zkg_groth16_prove_sparse takes, built here for callers of the dense entry point.  Gives up (false: the
// dense upload) as soon as more than 1/16 of the variables are not bits, and below 2^19 variables, where waking the pool costs what the upload did
// (measured, dense upload -> scan: 37 payloads / 2^20 domain 3.78 -> 3.53 ms, 8 payloads 1.29 -> 1.32, 2 payloads 0.78 -> 0.83).
static bool witness_to_sparse(const uint64_t *w, size_t n, std::vector<uint8_t> &tags, std::vector<uint32_t> &idx, std::vector<uint64_t> &vals) {
    if (n < ((size_t)1 << 19)) return false;
    const Fr one_fr = Fr::one();
    uint64_t one[4]; memcpy(one, one_fr.v, 32);
    const size_t cap = n / 16;
    tags.resize(n);
    const int chunks = (int)std::min<size_t>(32, n / 32768 + 1);
    std::vector<std::vector<uint32_t>> found((size_t)chunks);
    std::atomic<bool> over{false};
    uint8_t *t = tags.data();
    zk::host_parallel_for(chunks, [&](int ch) {
        const size_t lo = n * (size_t)ch / (size_t)chunks, hi = n * (size_t)(ch + 1) / (size_t)chunks;
        std::vector<uint32_t> &f = found[(size_t)ch];
        for (size_t v = lo; v < hi; ++v) {
            const uint64_t *e = w + 4 * v;
            if ((e[0] | e[1] | e[2] | e[3]) == 0) t[v] = 0;
            else if (e[0] == one[0] && e[1] == one[1] && e[2] == one[2] && e[3] == one[3]) t[v] = 1;
            else { t[v] = 2; f.push_back((uint32_t)v); if (f.size() > cap) { over.store(true); return; } }
        }
    });
    if (over.load()) return false;
    size_t total = 0;
    for (auto &f : found) total += f.size();
    if (total > cap) return false;
    idx.clear(); idx.reserve(total);
    for (auto &f : found) idx.insert(idx.end(), f.begin(), f.end());
    vals.resize(4 * total);
    for (size_t i = 0; i < total; ++i) memcpy(&vals[4 * i], w + 4 * (size_t)idx[i], 32);
    return true;
}
// The body of every single-proof entry: a slot lease, prove_enqueue (nothing of the slot is left running when it fails), prove_finish (which writes
// `out` as the pieces land: see prove_single_staged).  A dense host witness goes up sparse where that pays.  A device witness is ordered behind `caller`,
// the stream whose queued work wrote it (unused otherwise): the proof runs on the slot's own (non-blocking) streams, and the call returns after the proof
// has landed, so nothing of it is left running for the caller to order after.
struct SingleOutcome { bool enqueued = false; int zw_state = ZW_NONE; };     // prove_enqueue succeeded; what became of a generated witness (ZW_*)
static int prove_single(zkg_crs *crs, const WitnessSrc &witness, const uint64_t r_[4], const uint64_t s_[4], bool check, hipStream_t caller, uint8_t *out, size_t *len,
                        SingleOutcome *outcome = nullptr) {
    SlotLease lease(crs);
    if (!lease.ok()) return ZKG_ERROR;
    ProverSlot &S = lease.S();
    WitnessSrc W = witness;
    if (W.dense && witness_to_sparse(W.dense, crs->n, S.scan_tags, S.scan_idx, S.scan_vals)) {
        W.dense = nullptr; W.tags = S.scan_tags.data(); W.idx = S.scan_idx.data(); W.vals = S.scan_vals.data(); W.count = S.scan_idx.size();
    }
    if (W.dev) { ZK_HIP(hipEventRecord(S.ev[12], caller)); ZK_HIP(hipStreamWaitEvent(S.stream, S.ev[12], 0)); }
    const int rc = prove_enqueue(crs, S, W, r_, s_, check);
    if (outcome) { outcome->enqueued = rc == ZKG_OK; outcome->zw_state = S.zw_state; }
    if (rc) { slot_drain(crs, S); return ZKG_ERROR; }
    return prove_finish(crs, S, out, len);
}
// the same with the proof staged: nothing is written unless the proof is made
static int prove_single_staged(zkg_crs *crs, const WitnessSrc &W, const uint64_t r_[4], const uint64_t s_[4], bool check, hipStream_t caller, uint8_t *proof_out, size_t *proof_len,
                               SingleOutcome *outcome = nullptr) {
    uint8_t buf[256]; size_t len = 0;
    const int rc = prove_single(crs, W, r_, s_, check, caller, buf, &len, outcome);
    if (rc == ZKG_OK) { memcpy(proof_out, buf, len); *proof_len = len; }
    return rc;
}
static int groth16_prove_impl(const zkg_crs *crs_, const uint64_t *witness, const uint64_t r_[4], const uint64_t s_[4], int check_satisfied,
                              uint8_t *proof_out, size_t *proof_len) {
    zkg_crs *crs = const_cast<zkg_crs *>(crs_);
    if (!crs || !r_ || !s_ || !proof_out || !proof_len || (crs->n && !witness)) { set_error("zkg_groth16_prove: bad argument"); return ZKG_ERROR; }
    WitnessSrc W; W.dense = witness;
    return prove_single(crs, W, r_, s_, check_satisfied != 0, nullptr, proof_out, proof_len);
}

// the same proof from a sparse description of the witness: tags[n] (0 = zero, 1 = one, 2 = listed) and `count` listed variables as
// (index among the n variables, value as 4 Montgomery limbs).  What a witness generator that knows its bits hands over: the upload
// shrinks ~30x (see k_expand_tags).  Identical proof bytes to zkg_groth16_prove on the expanded vector.
static int groth16_prove_sparse_impl(const zkg_crs *crs_, const uint8_t *tags, const uint32_t *full_index, const uint64_t *full_values, size_t count,
                                     const uint64_t r_[4], const uint64_t s_[4], int check_satisfied, uint8_t *proof_out, size_t *proof_len) {
    zkg_crs *crs = const_cast<zkg_crs *>(crs_);
    if (!crs || !r_ || !s_ || !proof_out || !proof_len || (crs->n && !tags) || (count && (!full_index || !full_values)) || count > crs->n) {
        set_error("zkg_groth16_prove_sparse: bad argument"); return ZKG_ERROR;
    }
    WitnessSrc W; W.tags = tags; W.idx = full_index; W.vals = full_values; W.count = count;
    return prove_single(crs, W, r_, s_, check_satisfied != 0, nullptr, proof_out, proof_len);
}

// ---- zkg_groth16_prove_zklaim: one credential of a resident key, its witness generated on the device (k_zklaim_witness_par, launched by
// compute_h_matvec in front of the split).  Every key the single path serves.  A key the generator's plan does not fit, a plan that
// disagrees with the host pass, or a generator that raised its error word: the host witness and groth16_prove_sparse_impl.
static int prove_zklaim_host_witness(zkg_crs *crs, const zklaim_ctx *ctx, const uint64_t r_[4], const uint64_t s_[4], int check_satisfied, uint8_t *proof_out, size_t *proof_len) {
    zkg_circuit *ck = zkg_zklaim_witness_new(ctx);
    if (!ck) return ZKG_ERROR;
    struct Free { zkg_circuit *c; ~Free() { zkg_circuit_free(c); } } free_ck{ck};
    const uint8_t *tags = nullptr; const uint32_t *fidx = nullptr; const uint64_t *fval = nullptr; size_t nfull = 0;
    if (zkg_circuit_num_variables(ck) != crs->n) { set_error("zkg_groth16_prove_zklaim: broken payload list or a payload count other than the key's"); return ZKG_ERROR; }
    if (zkg_circuit_sparse_witness(ck, &tags, &fidx, &fval, &nfull) != ZKG_OK) { set_error("zkg_groth16_prove_zklaim: no witness"); return ZKG_ERROR; }
    t_prove_zklaim_stats[1] = 1;
    return groth16_prove_sparse_impl(crs, tags, fidx, fval, nfull, r_, s_, check_satisfied, proof_out, proof_len);   // (zkg_last_error keeps what sent the call here)
}
static int groth16_prove_zklaim_impl(const zkg_crs *crs_, const zklaim_ctx *ctx, const uint64_t r_[4], const uint64_t s_[4], int check_satisfied, uint8_t *proof_out, size_t *proof_len) {
    t_prove_zklaim_stats[0] = t_prove_zklaim_stats[1] = 0;
    zkg_crs *crs = const_cast<zkg_crs *>(crs_);
    if (initialised_device() < 0) { set_error("zkg_groth16_prove_zklaim: zkg_init has not been called"); return ZKG_ERROR; }
    if (!crs || !ctx || !r_ || !s_ || !proof_out || !proof_len) { set_error("zkg_groth16_prove_zklaim: bad argument"); return ZKG_ERROR; }
    ZwPlan pl;
    if (zklaim_witness_plan_for_n(crs->n, pl) && zklaim_witness_par_ready(pl)) {
        WitnessSrc W; W.ctx = ctx; W.plan = &pl;
        SingleOutcome outcome;
        const int rc = prove_single_staged(crs, W, r_, s_, check_satisfied != 0, nullptr, proof_out, proof_len, &outcome);
        if (rc == ZKG_OK || rc == ZKG_UNSATISFIED) t_prove_zklaim_stats[0] = 1;
        if (outcome.zw_state != ZW_GENERATOR_ERROR) return rc;                  // (the generator's error: the host witness below)
    }
    return prove_zklaim_host_witness(crs, ctx, r_, s_, check_satisfied, proof_out, proof_len);
}

// ---- zkg_groth16_prove_batch: P proofs of one key per launch sequence -----------------------------------------------------------
// Proofs per chunk, 0 = the key takes the single-proof path inside the call: domains below 2^18 without H shards run batched (up to seven
// payloads: a lone proof leaves most of the chip idle there), radix-2 and step_radix2 alike; a larger domain (one proof fills the chip) or a
// sharded H query do not.  16 proofs up to m = 2^15, 8 above: the H launch's P x W x B buckets stay within the block scan of the digit sort.
static uint32_t batch_chunk_for(const zkg_crs *crs) {
    if ((!crs->dom && !crs->sdom) || crs->m >= ((size_t)1 << 18) || crs->m < 2 || !crs->n || !crs->h_shards.empty()) return 0;
    const uint32_t P = (crs->m <= ((size_t)1 << 15) && crs->c_w_forced < 15) ? MSM_MULTI_MAX_VECTORS : MSM_MULTI_MAX_VECTORS / 2;               // (a forced 15- or 16-bit witness window: as the large H windows)
    return msm_multi_supported(crs->m - 1, crs->H_query.c, P) ? P : 0;
}
static void batch_destroy(BatchWs &B) {
    for (DevBuf *b : {&B.z, &B.aABC, &B.scratch, &B.wtags, &B.wlisted, &B.words, &B.stage, &B.wscal}) b->release();
    msm_job_destroy(B.job_h); msm_job_destroy(B.job_w1); msm_job_destroy(B.job_w2); B.job_h = B.job_w1 = B.job_w2 = nullptr;
    B.ones_g1.release(); B.ones_g2.release();
    if (B.stream) (void)hipStreamDestroy(B.stream);
    B.stream = nullptr;
    for (hipStream_t &st : B.wst) { if (st) (void)hipStreamDestroy(st); st = nullptr; }
    for (hipEvent_t *e : {&B.ev_split, &B.ev_flags, &B.ev_gathered, &B.ev_in}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
    if (B.host_stage) (void)hipHostFree(B.host_stage);
    if (B.host_words) (void)hipHostFree(B.host_words);
    B.host_stage = nullptr; B.host_words = nullptr; B.host_cap = 0; B.ready = false; B.P = 0;
}
static size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static int batch_create(zkg_crs *crs, BatchWs &B, uint32_t P) {
    if (B.ready) return ZKG_OK;
    const size_t n1 = (size_t)crs->n + 1, m = crs->m;
    bool ok = B.z.reserve(P * n1 * 32) == 0 && B.aABC.reserve((size_t)P * 3 * m * 32) == 0 && B.scratch.reserve((size_t)P * 3 * m * NTT_SCRATCH_BYTES) == 0 &&
              B.wtags.reserve(P * round_up(n1, 16)) == 0 && B.wlisted.reserve(P * n1 * 4) == 0 && B.words.reserve((size_t)P * BATCH_WORDS * 4) == 0 &&
              hip_ok(hipHostMalloc((void **)&B.host_words, ((size_t)2 * P * BATCH_WORDS + 16) * 4, hipHostMallocDefault), "hipHostMalloc", __FILE__, __LINE__);
    if (ok) {
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        // the chunk's critical path (upload, split, mat-vec, transforms, H) on one stream, as a slot's; wst[0] the B_2 job, wst[1] the A / B_1 / L job, wst[2..3] the flat sums
        ok = hip_ok(hipStreamCreateWithPriority(&B.stream, hipStreamNonBlocking, prio_hi), "hipStreamCreate", __FILE__, __LINE__);
        for (hipStream_t &st : B.wst) ok = ok && hip_ok(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio_lo), "hipStreamCreate", __FILE__, __LINE__);
        ok = ok && hip_ok(hipEventCreateWithFlags(&B.ev_split, hipEventDisableTiming), "hipEventCreate", __FILE__, __LINE__) &&
             hip_ok(hipEventCreateWithFlags(&B.ev_flags, hipEventDisableTiming), "hipEventCreate", __FILE__, __LINE__) &&
             hip_ok(hipEventCreateWithFlags(&B.ev_gathered, hipEventDisableTiming), "hipEventCreate", __FILE__, __LINE__) &&
             hip_ok(hipEventCreateWithFlags(&B.ev_in, hipEventDisableTiming), "hipEventCreate", __FILE__, __LINE__);
        B.job_h = ok ? msm_job_create(B.stream, false) : nullptr;
        B.job_w2 = ok ? msm_job_create(B.wst[0], false) : nullptr; B.job_w1 = ok ? msm_job_create(B.wst[1], false) : nullptr;
        ok = ok && B.job_h && B.job_w1 && B.job_w2;
        if (ok) { msm_job_set_window(B.job_h, crs->H_query.c); msm_job_set_row_merge(B.job_h, h_row_merge(crs)); }
    }
    if (!ok) { batch_destroy(B); return ZKG_ERROR; }
    B.P = P; B.ready = true;
    return ZKG_OK;
}
static void batch_drain(BatchWs &B) {
    (void)hipStreamSynchronize(B.stream);
    for (hipStream_t st : B.wst) (void)hipStreamSynchronize(st);
}
// a dense witness in the sparse form: tag per variable, the variables that are neither 0 nor 1 listed (idx / vals null: count only)
static size_t dense_to_sparse(const uint64_t *w, size_t n, uint8_t *tags, uint32_t *idx, uint64_t *vals) {
    const Fr one_fr = Fr::one();
    uint64_t one[4]; memcpy(one, one_fr.v, 32);
    size_t cnt = 0;
    for (size_t v = 0; v < n; ++v) {
        const uint64_t *e = w + 4 * v;
        uint8_t t = 2;
        if ((e[0] | e[1] | e[2] | e[3]) == 0) t = 0;
        else if (e[0] == one[0] && e[1] == one[1] && e[2] == one[2] && e[3] == one[3]) t = 1;
        if (tags) tags[v] = t;
        if (t == 2) { if (idx) { idx[cnt] = (uint32_t)v; memcpy(vals + 4 * cnt, e, 32); } ++cnt; }
    }
    return cnt;
}
static thread_local size_t t_batch_stats[3] = {0, 0, 0};

// Where a batch's witnesses come from (what WitnessSrc is to a single proof), one kind per entry:
//   HOST_ITEMS  zkg_groth16_prove_batch: items[p], a dense or a sparse witness and its (r, s); packed on the host, one upload per chunk
//   ZKLAIM      zkg_groth16_prove_batch_zklaim: ctxs[p], credentials of the key's payload count; a few bytes each go up and k_zklaim_witness
//               writes the same packed form into the device stage
//   DEVICE      zkg_groth16_prove_batch_dev: dense witnesses already in device memory, item p at dev + p * stride, behind the caller's `stream`;
//               split in place by k_split_dev, nothing is packed, staged or uploaded
struct ChunkSource {
    enum Kind { HOST_ITEMS, ZKLAIM, DEVICE } kind = HOST_ITEMS;
    const zkg_prove_item *items = nullptr;
    const zklaim_ctx *const *ctxs = nullptr; const ZwPlan *plan = nullptr;
    const Fr *dev = nullptr; size_t stride = 0; hipStream_t stream = nullptr;
    const uint64_t *rs = nullptr;                                             // ZKLAIM, DEVICE: 8 limbs per item, r | s
    const uint64_t *r(size_t p) const { return kind == HOST_ITEMS ? items[p].r : rs + 8 * p; }
    const uint64_t *s(size_t p) const { return kind == HOST_ITEMS ? items[p].s : rs + 8 * p + 4; }
    ChunkSource from(size_t first) const {                                    // the same source, item `first` as item 0
        ChunkSource c = *this;
        if (items) c.items += first; if (ctxs) c.ctxs += first; if (dev) c.dev += first * stride; if (rs) c.rs += 8 * first;
        return c;
    }
};
enum { CHUNK_CURSOR_ERROR = -1 };             // prove_chunk (ZKLAIM): the generator raised its cursor error; the chunk's witnesses have to come from the host

// one chunk: P <= B.P items 0 .. P of `src`, under the batch mutex and a slot lease (the lease is the chunk's place in the key's extension protocol;
// its slot lends the streams of a table extension).  The source's kind decides how the stage is built, which split is launched and where (r, s) are
// read; from the split on the three are one.
static int prove_chunk(zkg_crs *crs, BatchWs &B, ProverSlot &S, const ChunkSource &src, uint32_t P, bool check, uint8_t *proofs_out, int *status) {
    const size_t n = crs->n, n1 = n + 1, m = crs->m, l = crs->l, tag_stride = round_up(n, 16), wtag_stride = round_up(n1, 16);
    hipStream_t s = B.stream;
    const auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) { if (g_dbg_timing) fprintf(stderr, "[zkg batch] %-28s %8.3f ms\n", what, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count()); };
    auto host_stage_for = [&](size_t bytes) {
        if (bytes <= B.host_cap) return ZKG_OK;
        if (B.host_stage) (void)hipHostFree(B.host_stage);
        B.host_stage = nullptr; B.host_cap = 0;
        ZK_HIP(hipHostMalloc((void **)&B.host_stage, bytes + bytes / 2, hipHostMallocDefault));
        B.host_cap = bytes + bytes / 2;
        return ZKG_OK;
    };
    // ---- 1. the chunk's witnesses in the device stage: [desc | values | indices | tags]
    std::vector<uint32_t> cnt(P, 0); std::vector<uint8_t> skip(P, 0);
    std::vector<uint32_t> off(P + 1, 0);
    size_t o_vals = round_up((size_t)P * sizeof(BatchDesc), 64), o_idx = 0, o_tags = 0, o_gen = 0;
    uint32_t max_cnt = 0;
    switch (src.kind) {
    case ChunkSource::DEVICE: o_vals = 0; break;                                 // resident already: no stage (the offsets below stay 0)
    case ChunkSource::HOST_ITEMS: {                                              // packed on the host, one upload
        const zkg_prove_item *items = src.items;
        host_parallel_for((int)P, [&](int p) {
            const zkg_prove_item &it = items[p];
            if (!it.r || !it.s) skip[p] = 1;
            else if (it.witness) cnt[p] = (uint32_t)dense_to_sparse(it.witness, n, nullptr, nullptr, nullptr);
            else if (!it.tags || (it.count && (!it.full_index || !it.full_values)) || it.count > n) skip[p] = 1;
            else cnt[p] = (uint32_t)it.count;
        });
        for (uint32_t p = 0; p < P; ++p) off[p + 1] = off[p] + cnt[p];
        const size_t total = off[P];
        o_idx = o_vals + total * 32; o_tags = round_up(o_idx + total * 4, 64);
        const size_t bytes = o_tags + P * tag_stride;
        if (host_stage_for(bytes) || B.stage.reserve(bytes)) return ZKG_ERROR;
        uint8_t *hs = B.host_stage;
        host_parallel_for((int)P, [&](int p) {
            const zkg_prove_item &it = items[p];
            BatchDesc *d = reinterpret_cast<BatchDesc *>(hs) + p; d->off = off[p]; d->cnt = cnt[p];
            uint8_t *tags = hs + o_tags + (size_t)p * tag_stride; uint32_t *idx = reinterpret_cast<uint32_t *>(hs + o_idx) + off[p]; uint64_t *vals = reinterpret_cast<uint64_t *>(hs + o_vals) + 4 * (size_t)off[p];
            if (skip[p]) memset(tags, 0, n);
            else if (it.witness) (void)dense_to_sparse(it.witness, n, tags, idx, vals);
            else { memcpy(tags, it.tags, n); if (cnt[p]) { memcpy(idx, it.full_index, (size_t)cnt[p] * 4); memcpy(vals, it.full_values, (size_t)cnt[p] * 32); } }
        });
        lap("witnesses packed");
        ZK_HIP(hipMemcpyAsync(B.stage.p, hs, bytes, hipMemcpyHostToDevice, s));
        max_cnt = *std::max_element(cnt.begin(), cnt.end());
        break;
    }
    case ChunkSource::ZKLAIM: {                                                  // generated in place: fixed-capacity listed slots per item, counts made on the device
        const ZwPlan &pl = *src.plan;
        if (pl.n != n) { set_error("zkg_groth16_prove_batch_zklaim: plan does not fit the key"); return ZKG_ERROR; }
        const size_t total = (size_t)P * pl.cap, in_bytes = zklaim_witness_input_bytes(pl, P);
        o_idx = o_vals + total * 32; o_tags = round_up(o_idx + total * 4, 64); o_gen = round_up(o_tags + P * tag_stride, 64);
        if (host_stage_for(in_bytes) || B.stage.reserve(o_gen + in_bytes)) return ZKG_ERROR;
        zklaim_witness_pack(pl, src.ctxs, P, B.host_stage, skip.data());
        for (uint32_t p = 0; p < P; ++p) skip[p] = !skip[p];                      // (pack reports the good ones)
        lap("credentials packed");
        uint8_t *st = B.stage.as<uint8_t>();
        ZK_HIP(hipMemcpyAsync(st + o_gen, B.host_stage, in_bytes, hipMemcpyHostToDevice, s));
        if (zklaim_witness_launch(pl, P, st + o_gen, reinterpret_cast<uint32_t *>(st), reinterpret_cast<Fr *>(st + o_vals), reinterpret_cast<uint32_t *>(st + o_idx), st + o_tags, tag_stride, s)) return ZKG_ERROR;
        max_cnt = pl.cap;
        break;
    }
    }
    const uint8_t *st = B.stage.as<uint8_t>();
    const BatchDesc *d_desc = reinterpret_cast<const BatchDesc *>(st); const Fr *d_vals = reinterpret_cast<const Fr *>(st + o_vals);
    const uint32_t *d_idx = reinterpret_cast<const uint32_t *>(st + o_idx); const uint8_t *d_tags = st + o_tags;
    Fr *z = B.z.as<Fr>(), *aABC = B.aABC.as<Fr>(), *scr = B.scratch.as<Fr>();
    uint8_t *wtags = B.wtags.as<uint8_t>(); uint32_t *wlisted = B.wlisted.as<uint32_t>(), *words = B.words.as<uint32_t>();
    uint32_t *hw_split = B.host_words, *hw_flags = B.host_words + (size_t)B.P * BATCH_WORDS;
    const uint32_t *subset_pos = crs->sub.count ? crs->sub.pos.as<uint32_t>() : nullptr;
    uint32_t *hw_gen = B.host_words + (size_t)2 * B.P * BATCH_WORDS;
    // ---- 2. split, mat-vec, transforms, H: one launch sequence for the chunk
    if (src.kind == ChunkSource::DEVICE) {
        ZK_HIP(hipMemsetAsync(words, 0, (size_t)P * BATCH_WORDS * 4, s));
        hipLaunchKernelGGL(k_split_dev, dim3((unsigned)((n1 + 255) / 256), P), dim3(256), 0, s, src.dev, src.stride, n, z, wtags, wtag_stride, wlisted, words, words + 4, BATCH_WORDS,
                           subset_pos, (uint32_t *)nullptr);
    } else {
        hipLaunchKernelGGL(k_expand_tags_batch, dim3((unsigned)((n + 255) / 256), P), dim3(256), 0, s, d_tags, tag_stride, n, z, wtags, wtag_stride, words);
        if (max_cnt) hipLaunchKernelGGL(k_scatter_full_batch, dim3((max_cnt + 255) / 256, P), dim3(256), 0, s, d_desc, d_idx, d_vals, d_tags, tag_stride, n, z, wtags, wtag_stride, wlisted, words, subset_pos);
    }
    ZK_HIP(hipMemcpyAsync(hw_split, words, (size_t)P * BATCH_WORDS * 4, hipMemcpyDeviceToHost, s));
    if (src.kind == ChunkSource::ZKLAIM) ZK_HIP(hipMemcpyAsync(hw_gen, st + o_gen, 4, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipEventRecord(B.ev_split, s));
    const unsigned grid_m = (unsigned)((m + 255) / 256);
    hipLaunchKernelGGL(k_r1cs_eval_batch, dim3(grid_m, P), dim3(256), 0, s, crs->A.rowptr.as<uint32_t>(), crs->A.col.as<uint32_t>(), crs->A.val.as<Fr>(),
                       crs->B.rowptr.as<uint32_t>(), crs->B.col.as<uint32_t>(), crs->B.val.as<Fr>(), crs->Cm.rowptr.as<uint32_t>(), crs->Cm.col.as<uint32_t>(), crs->Cm.val.as<Fr>(),
                       z, n1, crs->C, crs->l, m, aABC, check ? words : nullptr);
    if (crs->n_long) {
        hipLaunchKernelGGL(k_r1cs_long_batch, dim3((crs->n_long + 3) / 4, P), dim3(256), 0, s, crs->long_rows.as<uint32_t>(), crs->n_long,
                           crs->A.rowptr.as<uint32_t>(), crs->A.col.as<uint32_t>(), crs->A.val.as<Fr>(), crs->B.rowptr.as<uint32_t>(), crs->B.col.as<uint32_t>(), crs->B.val.as<Fr>(),
                           crs->Cm.rowptr.as<uint32_t>(), crs->Cm.col.as<uint32_t>(), crs->Cm.val.as<Fr>(), z, n1, m, aABC);
        if (check) hipLaunchKernelGGL(k_r1cs_check_rows_batch, dim3((crs->n_long + 255) / 256, P), dim3(256), 0, s, crs->long_rows.as<uint32_t>(), crs->n_long, aABC, m, words);
    }
    if (check) { ZK_HIP(hipMemcpyAsync(hw_flags, words, (size_t)P * BATCH_WORDS * 4, hipMemcpyDeviceToHost, s)); ZK_HIP(hipEventRecord(B.ev_flags, s)); }
    // the transforms as batches of 3 P and P vectors (proof p's aA | aB | aC are vectors 3 p .. 3 p + 2; its aA alone 3 m apart)
    if (crs->dom) {
        if (ntt_run_ex(crs->dom, aABC, true, nullptr, crs->coset_over_m.as<Fr>(), nullptr, s, scr, 3 * P, 0, nullptr, crs->coset_over_m29.p)) return ZKG_ERROR;
        if (ntt_run_ex(crs->dom, aABC, false, nullptr, nullptr, nullptr, s, scr, 3 * P)) return ZKG_ERROR;
        hipLaunchKernelGGL(k_pointwise_h_batch, dim3(grid_m, P), dim3(256), 0, s, aABC, m, crs->z_inv_coset);
        if (ntt_run_ex(crs->dom, aABC, true, nullptr, crs->dom->icoset_post.as<Fr>(), nullptr, s, scr, P, 3 * m)) return ZKG_ERROR;
    } else {
        // step_radix2_domain: compute_h_transforms' four steps with the proof dimension.  Every vector's partial sums (32-byte elements) and
        // transform scratch (40-byte records, the small transform's behind the big one's) stay inside its own stride of the P x 3 m scratch:
        // 32 big + 40 small <= 40 m bytes
        StepDomain *sd = crs->sdom;
        if (step_ntt_run(sd, aABC, true, false, s, scr, 3 * P, m)) return ZKG_ERROR;                 // iFFT x 3 P
        if (step_ntt_run(sd, aABC, false, true, s, scr, 3 * P, m)) return ZKG_ERROR;                 // cosetFFT x 3 P
        hipLaunchKernelGGL(k_pointwise_h_step_batch, dim3(grid_m, P), dim3(256), 0, s, aABC, m, sd->shape.big, sd->zinv.as<Fr>(),
                           (uint32_t)(sd->shape.big / sd->shape.small - 1), sd->zinv_small);
        if (step_ntt_run(sd, aABC, true, true, s, scr, P, 3 * m)) return ZKG_ERROR;                  // icosetFFT x P
    }
    if (hipGetLastError() != hipSuccess) { set_error("prover kernel launch failed"); return ZKG_ERROR; }
    const MsmBases h = table_set(crs->H_query, false, 0);
    if (msm_job_launch_multi(B.job_h, &h, 1, B.aABC.as<uint32_t>(), m - 1, 3 * m * 8, P, true)) return ZKG_ERROR;
    lap("chunk stream enqueued");
    // ---- 3. the split has landed: per-item verdicts, the witness tables, the witness jobs
    ZK_HIP(hipEventSynchronize(B.ev_split));
    lap("split landed");
    if (src.kind == ChunkSource::ZKLAIM && *hw_gen) { set_error("zklaim witness generator: a cursor left its range (host witnesses are used)"); return CHUNK_CURSOR_ERROR; }
    std::vector<uint8_t> good(P, 0);
    bool extend = false;
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t *w = hw_split + (size_t)p * BATCH_WORDS;
        status[p] = ZKG_ERROR;
        if (skip[p]) { set_error("zkg_groth16_prove_batch: bad item"); continue; }
        if (w[3]) { set_error("prover: a listed witness index is out of range, not tagged 2 or listed twice"); continue; }
        if (w[4] > n1) { set_error("prover: witness split out of range"); continue; }
        good[p] = 1;
        extend = extend || (w[4] && (w[5] || !crs->sub.count));
    }
    if (extend) {
        // ONE extension for the union of the chunk's non-bit elements, under the key's protocol (see zkg_crs): no other proof in flight meanwhile
        std::vector<uint32_t> li;
        for (uint32_t p = 0; p < P; ++p) if (good[p]) {
            const size_t k = hw_split[(size_t)p * BATCH_WORDS + 4], at = li.size();
            li.resize(at + k);
            if (k) ZK_HIP(hipMemcpy(li.data() + at, wlisted + (size_t)p * n1, k * 4, hipMemcpyDeviceToHost));
        }
        if (extend_tables_exclusive(crs, S, li.size(), &li)) return ZKG_ERROR;
    }
    // bucket method: every proof's non-bit values over the subset tables, two multi launches; flat sums over the ones: the queries as uploaded, per proof
    const size_t sub_n = crs->sub.count;
    bool any_listed = false;
    for (uint32_t p = 0; p < P; ++p) any_listed = any_listed || (good[p] && hw_split[(size_t)p * BATCH_WORDS + 4]);
    const bool jobs = any_listed && sub_n;                                   // (no table yet and nothing listed: the witness queries are flat sums only)
    if (jobs) {
        if (!msm_multi_supported(sub_n, crs->c_w, P) || B.wscal.reserve((size_t)P * sub_n * 32)) { set_error("prover: witness tables too large for a batched launch"); return ZKG_ERROR; }
        hipStream_t s2 = msm_job_stream(B.job_w2), s1 = msm_job_stream(B.job_w1);
        hipLaunchKernelGGL(k_gather_nonbits_batch, dim3((unsigned)((sub_n + 255) / 256), P), dim3(256), 0, s2, z, wtags, n1, wtag_stride, crs->sub.idx.as<uint32_t>(), sub_n, B.wscal.as<Fr>());
        ZK_HIP(hipEventRecord(B.ev_gathered, s2)); ZK_HIP(hipStreamWaitEvent(s1, B.ev_gathered, 0));
        const MsmBases g1[3] = {table_set(crs->sub.A, false, 0), table_set(crs->sub.B1, false, 0), table_set(crs->sub.L, false, 0)}, b2 = table_set(crs->sub.B2, true, 0);
        msm_job_set_window(B.job_w1, crs->c_w); msm_job_set_window(B.job_w2, crs->c_w);
        if (msm_job_launch_multi(B.job_w2, &b2, 1, B.wscal.as<uint32_t>(), sub_n, sub_n * 8, P, true) ||
            msm_job_launch_multi(B.job_w1, g1, 3, B.wscal.as<uint32_t>(), sub_n, sub_n * 8, P, true)) return ZKG_ERROR;
    }
    const MsmBases o1[3] = {query_set(crs->A_query, false, 0), query_set(crs->B_g1, false, 0), query_set(crs->L_query, false, (uint32_t)(l + 1))}, o2 = query_set(crs->B_g2, true, 0);
    // (the split is complete: nothing to wait for on these streams)
    if (ones_sum_launch_multi(B.ones_g2, &o2, 1, wtags, wtag_stride, n1, P, B.wst[2]) || ones_sum_launch_multi(B.ones_g1, o1, 3, wtags, wtag_stride, n1, P, B.wst[3])) return ZKG_ERROR;
    lap("witness jobs enqueued");
    // ---- 4. results: H for the whole chunk, then the proofs' host work side by side on the host pool
    std::vector<G1> Ht(P), Wg1((size_t)3 * P, G1::inf()); std::vector<G2> Wg2(P, G2::inf());
    if (msm_job_finish_multi(B.job_h, Ht.data(), nullptr)) return ZKG_ERROR;     // (waits for the chunk's stream: the flags have landed too)
    lap("H landed");
    for (hipStream_t w : B.wst) ZK_HIP(hipStreamSynchronize(w));
    if (jobs && (msm_job_finish_multi(B.job_w1, Wg1.data(), nullptr) || msm_job_finish_multi(B.job_w2, nullptr, Wg2.data()))) return ZKG_ERROR;
    lap("witness jobs landed");
    const ProofKey pkey = proof_key_of(crs);
    host_parallel_for((int)P, [&](int p) {
        if (!good[p]) return;
        if (check && hw_flags[(size_t)p * BATCH_WORDS]) { status[p] = ZKG_UNSATISFIED; return; }
        G1 W1[3] = {Wg1[3 * (size_t)p], Wg1[3 * (size_t)p + 1], Wg1[3 * (size_t)p + 2]}; G2 Wb2 = Wg2[p];
        for (int i = 0; i < 3; ++i) W1[i].add(B.ones_g1.g1(3 * p + i));
        Wb2.add(B.ones_g2.g2pt(p));
        Fr r, sv; memcpy(r.v, src.r((size_t)p), 32); memcpy(sv.v, src.s((size_t)p), 32);
        assemble_proof(pkey, r, sv, W1, Wb2, Ht[p], proofs_out + (size_t)p * ZKG_PROOF_BYTES);
        status[p] = ZKG_OK;
    });
    lap("proofs assembled");
    for (uint32_t p = 0; p < P; ++p) if (status[p] == ZKG_UNSATISFIED) set_error("constraint system not satisfied; not creating proof");
    return ZKG_OK;
}
// one proof from n elements at d_w, behind `stream`; counts into t_prove_dev_stats (the entries reset it)
static int prove_dev_one(zkg_crs *crs, const Fr *d_w, const uint64_t r_[4], const uint64_t s_[4], int check_satisfied, uint8_t *proof_out, size_t *proof_len, hipStream_t stream) {
    WitnessSrc W; W.dev = d_w;
    SingleOutcome outcome;
    const int rc = prove_single_staged(crs, W, r_, s_, check_satisfied != 0, stream, proof_out, proof_len, &outcome);
    if (outcome.enqueued) ++t_prove_dev_stats[0];
    return rc;
}

// ---- the one driver of the batch entries: `count` items of `src` as chunks of the key's workspace, or — a key whose proofs do not batch — item by
// item through the single-proof path.  Counts into t_batch_stats (the entries reset it): items proved in chunks, items proved singly, chunks.
struct BatchHooks {                                                          // what an entry adds to the chunk loop
    std::function<int(BatchWs &)> before_chunks;                             // under the batch mutex, the workspace standing, in front of the first chunk
    size_t *chunk_items = nullptr;                                           // the entry's own counter of items proved in chunks
    std::vector<std::pair<size_t, uint32_t>> *redo = nullptr;                // chunks (first, P) that ended in CHUNK_CURSOR_ERROR are listed here and the call goes on
};
static int prove_batch_chunks(zkg_crs *crs, const ChunkSource &src, size_t count, int check_satisfied, uint8_t *proofs_out, int *status, const BatchHooks &hooks) {
    const uint32_t chunk = batch_chunk_for(crs);
    if (!chunk) {                                                            // this key's proofs do not batch: the single-proof path of the same source, item by item
        for (size_t i = 0; i < count; ++i) {
            uint8_t buf[256]; size_t len = 0;
            switch (src.kind) {
            case ChunkSource::HOST_ITEMS: {
                const zkg_prove_item &it = src.items[i];
                status[i] = it.witness ? groth16_prove_impl(crs, it.witness, it.r, it.s, check_satisfied, buf, &len)
                                       : groth16_prove_sparse_impl(crs, it.tags, it.full_index, it.full_values, it.count, it.r, it.s, check_satisfied, buf, &len);
                break;
            }
            case ChunkSource::DEVICE: status[i] = prove_dev_one(crs, src.dev + i * src.stride, src.r(i), src.s(i), check_satisfied, buf, &len, src.stream); break;
            case ChunkSource::ZKLAIM: set_error("prover: contexts on a key that does not batch"); return ZKG_ERROR;   // (the entry sends such a key to host witnesses: items by the time they are here)
            }
            if (status[i] == ZKG_OK) memcpy(proofs_out + i * ZKG_PROOF_BYTES, buf, ZKG_PROOF_BYTES);
            ++t_batch_stats[1];
        }
        return ZKG_OK;
    }
    std::lock_guard<std::mutex> batch_lock(crs->batch_mu);
    BatchWs &B = crs->batch;
    if (batch_create(crs, B, chunk)) return ZKG_ERROR;
    if (hooks.before_chunks && hooks.before_chunks(B)) return ZKG_ERROR;
    for (size_t first = 0; first < count; first += chunk) {
        const uint32_t P = (uint32_t)std::min<size_t>(chunk, count - first);
        SlotLease lease(crs);                                                // per chunk: between chunks other callers may extend the witness tables
        if (!lease.ok()) return ZKG_ERROR;
        // nothing of the chunk may still be running when the workspace changes hands: drained on every way out but success, a throw included
        struct Drain { BatchWs &B; bool armed; ~Drain() { if (armed) batch_drain(B); } } drain{B, true};
        const int rc = prove_chunk(crs, B, lease.S(), src.from(first), P, check_satisfied != 0, proofs_out + first * ZKG_PROOF_BYTES, status + first);
        if (rc == CHUNK_CURSOR_ERROR && hooks.redo) { hooks.redo->push_back({first, P}); continue; }
        if (rc) return ZKG_ERROR;
        drain.armed = false;
        t_batch_stats[0] += P; ++t_batch_stats[2];
        if (hooks.chunk_items) *hooks.chunk_items += P;
    }
    return ZKG_OK;
}
static int groth16_prove_batch_impl(const zkg_crs *crs_, const zkg_prove_item *items, size_t count, int check_satisfied, uint8_t *proofs_out, int *status) {
    t_batch_stats[0] = t_batch_stats[1] = t_batch_stats[2] = 0;
    if (!count) return ZKG_OK;
    zkg_crs *crs = const_cast<zkg_crs *>(crs_);
    if (!crs || !items || !proofs_out || !status) { set_error("zkg_groth16_prove_batch: bad argument"); return ZKG_ERROR; }
    ChunkSource src; src.kind = ChunkSource::HOST_ITEMS; src.items = items;
    return prove_batch_chunks(crs, src, count, check_satisfied, proofs_out, status, BatchHooks{});
}

// ---- zkg_groth16_prove_dev / zkg_groth16_prove_batch_dev: witnesses that are already in device memory.  The refusals come first, before any
// launch: the calling thread on another device than the key's, a pointer that is not device memory of that device (pinned, managed and
// unregistered host memory included), a range that runs past the end of its allocation (best effort: where the runtime knows the allocation).
static int dev_witness_refused(const zkg_crs *crs, const void *d, size_t elems, const char *who) {
    auto refuse = [&](const char *why) { set_error(std::string(who) + ": " + why); return ZKG_ERROR; };
    if (initialised_device() < 0) return refuse("zkg_init has not been called");
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != crs->device) { (void)hipGetLastError(); return refuse("the calling thread's device is not the key's"); }
    if (!elems) return ZKG_OK;                                                  // (a key without variables: nothing is read)
    return dev_range_refused(d, elems * 32, alignof(Fr), crs->device, who, "the witness", "key");
}
static int groth16_prove_dev_impl(const zkg_crs *crs_, const void *d_witness, const uint64_t r_[4], const uint64_t s_[4], int check_satisfied,
                                  uint8_t *proof_out, size_t *proof_len, void *stream) {
    t_prove_dev_stats[0] = t_prove_dev_stats[1] = 0;
    zkg_crs *crs = const_cast<zkg_crs *>(crs_);
    if (!crs || !d_witness || !r_ || !s_ || !proof_out || !proof_len) { set_error("zkg_groth16_prove_dev: bad argument"); return ZKG_ERROR; }
    if (dev_witness_refused(crs, d_witness, crs->n, "zkg_groth16_prove_dev")) return ZKG_ERROR;
    return prove_dev_one(crs, static_cast<const Fr *>(d_witness), r_, s_, check_satisfied, proof_out, proof_len, (hipStream_t)stream);
}
static int groth16_prove_batch_dev_impl(const zkg_crs *crs_, const void *d_witnesses, size_t stride, size_t count, const uint64_t *rs, int check_satisfied,
                                        uint8_t *proofs_out, int *status, void *stream) {
    t_batch_stats[0] = t_batch_stats[1] = t_batch_stats[2] = 0; t_prove_dev_stats[0] = t_prove_dev_stats[1] = 0;
    if (!count) return ZKG_OK;
    zkg_crs *crs = const_cast<zkg_crs *>(crs_);
    if (!crs || !d_witnesses || !rs || !proofs_out || !status) { set_error("zkg_groth16_prove_batch_dev: bad argument"); return ZKG_ERROR; }
    if (stride < crs->n) { set_error("zkg_groth16_prove_batch_dev: stride is shorter than the witness"); return ZKG_ERROR; }
    if (stride && count - 1 > (SIZE_MAX / 64 - crs->n) / stride) { set_error("zkg_groth16_prove_batch_dev: count x stride out of range"); return ZKG_ERROR; }
    if (dev_witness_refused(crs, d_witnesses, crs->n ? (count - 1) * stride + crs->n : 0, "zkg_groth16_prove_batch_dev")) return ZKG_ERROR;
    ChunkSource src; src.kind = ChunkSource::DEVICE; src.dev = static_cast<const Fr *>(d_witnesses); src.stride = stride; src.stream = (hipStream_t)stream; src.rs = rs;
    BatchHooks hooks; hooks.chunk_items = &t_prove_dev_stats[0];
    // every chunk runs on the workspace's stream, in order: ONE wait puts the whole call behind the caller's stream
    hooks.before_chunks = [&](BatchWs &B) -> int { ZK_HIP(hipEventRecord(B.ev_in, src.stream)); ZK_HIP(hipStreamWaitEvent(B.stream, B.ev_in, 0)); return ZKG_OK; };
    return prove_batch_chunks(crs, src, count, check_satisfied, proofs_out, status, hooks);
}

// ---- zkg_groth16_prove_batch_zklaim: the same chunks, their witnesses generated on the device from the contexts
// host witnesses for ctxs[0 .. count) through zkg_groth16_prove_batch (which takes the single-proof path for keys that do not batch)
static int prove_zklaim_host_witnesses(const zkg_crs *crs, const zklaim_ctx *const *ctxs, size_t count, const uint64_t *rs, int check_satisfied, uint8_t *proofs_out, int *status) {
    std::vector<zkg_circuit *> cks(count, nullptr);
    struct FreeAll { std::vector<zkg_circuit *> &v; ~FreeAll() { for (zkg_circuit *c : v) if (c) zkg_circuit_free(c); } } free_all{cks};
    std::vector<zkg_prove_item> items(count); std::vector<uint8_t> ok(count, 0);
    host_parallel_for((int)count, [&](int i) {
        try {
            zkg_prove_item &it = items[i]; it = zkg_prove_item{};
            if (!ctxs[i]) return;
            cks[i] = zkg_zklaim_witness_new(ctxs[i]);
            ok[i] = cks[i] && zkg_circuit_num_variables(cks[i]) == crs->n && zkg_circuit_sparse_witness(cks[i], &it.tags, &it.full_index, &it.full_values, &it.count) == ZKG_OK;
            it.r = rs + 8 * (size_t)i; it.s = it.r + 4;
        } catch (...) { ok[i] = 0; }
    });
    std::vector<zkg_prove_item> batch; std::vector<size_t> which;
    for (size_t i = 0; i < count; ++i) {
        status[i] = ZKG_ERROR;
        if (ok[i]) { batch.push_back(items[i]); which.push_back(i); }
        else set_error("zkg_groth16_prove_batch_zklaim: null context, broken payload list or a payload count other than the key's");
    }
    zk::t_zklaim_witness_stats[1] += which.size();
    const size_t before[3] = {t_batch_stats[0], t_batch_stats[1], t_batch_stats[2]};
    std::vector<uint8_t> out(batch.size() * ZKG_PROOF_BYTES); std::vector<int> st(batch.size(), ZKG_ERROR);
    const int rc = c_boundary("zkg_groth16_prove_batch", ZKG_ERROR, [&] { return groth16_prove_batch_impl(crs, batch.data(), batch.size(), check_satisfied, out.data(), st.data()); });
    for (int j = 0; j < 3; ++j) t_batch_stats[j] += before[j];
    if (rc != ZKG_OK) return rc;
    for (size_t j = 0; j < which.size(); ++j) { status[which[j]] = st[j]; if (st[j] == ZKG_OK) memcpy(proofs_out + which[j] * ZKG_PROOF_BYTES, out.data() + j * ZKG_PROOF_BYTES, ZKG_PROOF_BYTES); }
    return ZKG_OK;
}
static int groth16_prove_batch_zklaim_impl(const zkg_crs *crs_, const zklaim_ctx *const *ctxs, size_t count, const uint64_t *rs, int check_satisfied, uint8_t *proofs_out, int *status) {
    t_batch_stats[0] = t_batch_stats[1] = t_batch_stats[2] = 0; zk::t_zklaim_witness_stats[0] = zk::t_zklaim_witness_stats[1] = 0;
    if (!count) return ZKG_OK;
    zkg_crs *crs = const_cast<zkg_crs *>(crs_);
    if (!crs || !ctxs || !rs || !proofs_out || !status) { set_error("zkg_groth16_prove_batch_zklaim: bad argument"); return ZKG_ERROR; }
    ZwPlan pl;
    // a key that does not batch, or a generator that disagrees with the host pass about the circuit: host witnesses, the existing paths
    if (!batch_chunk_for(crs) || !zklaim_witness_plan_for_n(crs->n, pl)) return prove_zklaim_host_witnesses(crs, ctxs, count, rs, check_satisfied, proofs_out, status);
    std::vector<std::pair<size_t, uint32_t>> redo;                            // chunks whose generator reported a stray cursor
    ChunkSource src; src.kind = ChunkSource::ZKLAIM; src.ctxs = ctxs; src.plan = &pl; src.rs = rs;
    BatchHooks hooks; hooks.chunk_items = &zk::t_zklaim_witness_stats[0]; hooks.redo = &redo;
    if (prove_batch_chunks(crs, src, count, check_satisfied, proofs_out, status, hooks)) return ZKG_ERROR;
    // (the batch mutex is free again: the host witnesses go through zkg_groth16_prove_batch's path, which takes it)
    for (auto &c : redo)
        if (prove_zklaim_host_witnesses(crs, ctxs + c.first, c.second, rs + 8 * c.first, check_satisfied, proofs_out + c.first * ZKG_PROOF_BYTES, status + c.first)) return ZKG_ERROR;
    return ZKG_OK;
}

// helper threads and host containers are used below these: nothing may propagate through the C boundary
int zkg_groth16_prove(const zkg_crs *crs, const uint64_t *witness, const uint64_t r[4], const uint64_t s[4], int check_satisfied,
                      uint8_t *proof_out, size_t *proof_len) {
    return c_boundary("zkg_groth16_prove", ZKG_ERROR, [&] { return groth16_prove_impl(crs, witness, r, s, check_satisfied, proof_out, proof_len); });
}
int zkg_groth16_prove_sparse(const zkg_crs *crs, const uint8_t *tags, const uint32_t *full_index, const uint64_t *full_values, size_t count,
                             const uint64_t r[4], const uint64_t s[4], int check_satisfied, uint8_t *proof_out, size_t *proof_len) {
    return c_boundary("zkg_groth16_prove_sparse", ZKG_ERROR, [&] { return groth16_prove_sparse_impl(crs, tags, full_index, full_values, count, r, s, check_satisfied, proof_out, proof_len); });
}
int zkg_groth16_prove_zklaim(const zkg_crs *crs, const struct zklaim_ctx *ctx, const uint64_t r[4], const uint64_t s[4], int check_satisfied, uint8_t *proof_out, size_t *proof_len) {
    return c_boundary("zkg_groth16_prove_zklaim", ZKG_ERROR, [&] { return groth16_prove_zklaim_impl(crs, ctx, r, s, check_satisfied, proof_out, proof_len); });
}
void zkg_prove_zklaim_stats(size_t out[2]) { if (out) { out[0] = zk::t_prove_zklaim_stats[0]; out[1] = zk::t_prove_zklaim_stats[1]; } }
int zkg_groth16_prove_batch(const zkg_crs *crs, const zkg_prove_item *items, size_t count, int check_satisfied, uint8_t *proofs_out, int *status) {
    return c_boundary("zkg_groth16_prove_batch", ZKG_ERROR, [&] { return groth16_prove_batch_impl(crs, items, count, check_satisfied, proofs_out, status); });
}
int zkg_groth16_prove_dev(const zkg_crs *crs, const void *d_witness, const uint64_t r[4], const uint64_t s[4], int check_satisfied, uint8_t *proof_out, size_t *proof_len, void *stream) {
    return c_boundary("zkg_groth16_prove_dev", ZKG_ERROR, [&] { return groth16_prove_dev_impl(crs, d_witness, r, s, check_satisfied, proof_out, proof_len, stream); });
}
int zkg_groth16_prove_batch_dev(const zkg_crs *crs, const void *d_witnesses, size_t stride, size_t count, const uint64_t *rs, int check_satisfied, uint8_t *proofs_out, int *status, void *stream) {
    return c_boundary("zkg_groth16_prove_batch_dev", ZKG_ERROR, [&] { return groth16_prove_batch_dev_impl(crs, d_witnesses, stride, count, rs, check_satisfied, proofs_out, status, stream); });
}
void zkg_prove_dev_stats(size_t out[2]) { if (out) { out[0] = zk::t_prove_dev_stats[0]; out[1] = zk::t_prove_dev_stats[1]; } }
int zkg_groth16_prove_batch_zklaim(const zkg_crs *crs, const struct zklaim_ctx *const *ctxs, size_t count, const uint64_t *rs, int check_satisfied, uint8_t *proofs_out, int *status) {
    return c_boundary("zkg_groth16_prove_batch_zklaim", ZKG_ERROR, [&] { return groth16_prove_batch_zklaim_impl(crs, ctxs, count, rs, check_satisfied, proofs_out, status); });
}
void zkg_zklaim_witness_stats(size_t out[2]) { if (out) { out[0] = zk::t_zklaim_witness_stats[0]; out[1] = zk::t_zklaim_witness_stats[1]; } }
void zkg_prove_batch_stats(size_t out[3]) { if (out) for (int i = 0; i < 3; ++i) out[i] = t_batch_stats[i]; }
size_t zkg_prove_batch_chunk(const zkg_crs *crs) { return crs ? batch_chunk_for(crs) : 0; }

// Shards the H query of a resident key over `ndev` devices (a device may be listed more than once: how a one-GPU box rehearses the
// path).  No proof of this key may be in flight.  The key's own device keeps everything else (witness queries, transforms, assembly).
static int crs_shard_h_impl(zkg_crs *crs, const int *devices, int ndev) {
    if (!crs || !devices || ndev < 1 || ndev > 64) { set_error("zkg_crs_shard_h: bad argument"); return ZKG_ERROR; }
    int count = 0; (void)hipGetDeviceCount(&count);
    for (int i = 0; i < ndev; ++i) if (devices[i] < 0 || devices[i] >= count) { set_error("zkg_crs_shard_h: bad device index"); return ZKG_ERROR; }
    std::unique_lock<std::mutex> lk(crs->mu);
    if (crs->leases) { set_error("zkg_crs_shard_h: a proof of this key is in flight"); return ZKG_ERROR; }
    if (crs->provers) { set_error("zkg_crs_shard_h: the key has a live zkg_prover handle (it holds the H table); free it first"); return ZKG_ERROR; }
    int cur = 0; (void)hipGetDevice(&cur);
    struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{cur};
    crs->home_device = cur;
    const size_t n = crs->H_query.n; const int c = crs->H_query.c;
    const G1Affine *level0 = crs->H_query.buf.as<G1Affine>();                 // level 0 of the table is the query as uploaded
    std::vector<zkg_crs::HShard> shards; shards.reserve((size_t)ndev);
    bool ok = true;
    for (int i = 0; i < ndev && ok; ++i) {
        const size_t first = n * (size_t)i / (size_t)ndev, count = n * (size_t)(i + 1) / (size_t)ndev - first;
        if (!count) continue;                                                  // more shards than points
        shards.emplace_back();
        zkg_crs::HShard &sh = shards.back();
        sh.device = devices[i]; sh.first = first; sh.n = count;
        ok = hipSetDevice(sh.device) == hipSuccess;
        if (ok && sh.device != cur) { int can = 0; if (hipDeviceCanAccessPeer(&can, sh.device, cur) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(cur, 0); (void)hipGetLastError(); }
        ScopedDevBuf slice;
        ok = ok && slice.reserve(sh.n * sizeof(G1Affine) + 16) == 0 &&
             hip_ok(hipMemcpy(slice.p, level0 + sh.first, sh.n * sizeof(G1Affine), hipMemcpyDefault), "H shard copy", __FILE__, __LINE__) &&
             window_table_build_g1(sh.table, slice.as<G1Affine>(), sh.n, c, nullptr) == 0 && window_table_records29(sh.table, nullptr) == 0 &&
             hip_ok(hipDeviceSynchronize(), "sync", __FILE__, __LINE__);
    }
    if (!ok) { for (auto &sh : shards) { (void)hipSetDevice(sh.device); sh.table.release(); } return ZKG_ERROR; }
    crs->h_shards.swap(shards); ++crs->h_epoch;                               // slots rebuild their per-shard jobs at their next proof
    for (auto &sh : shards) { (void)hipSetDevice(sh.device); sh.table.release(); }     // a previous sharding's tables
    return ZKG_OK;
}
int zkg_crs_shard_h(zkg_crs *crs, const int *devices, int ndev) { return c_boundary("zkg_crs_shard_h", ZKG_ERROR, [&] { return crs_shard_h_impl(crs, devices, ndev); }); }

int zkg_prover_peak_in_flight(int reset) {
    const int v = g_peak_in_flight.load();
    if (reset) g_peak_in_flight.store(0);
    return v;
}
int zkg_prove_stage_ms(const zkg_crs *crs, float ms[8]) {
    if (!crs || !ms) return ZKG_ERROR;
    for (int i = 0; i < 8; ++i) ms[i] = crs->stage_ms[i];
    return ZKG_OK;
}

}  // extern "C"

// the blob path (codec.hip): queries already on the device, constraint system possibly still being parsed
zkg_crs *crs_upload_device_queries(const zkg_pk *pk, const std::function<bool()> &constraint_system_ready) {
    return zkg_crs_upload_impl(pk, true, constraint_system_ready);
}
