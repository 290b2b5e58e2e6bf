// zklaim_witness.hip — the witness of zklaim's credential circuit generated on the device, for the batched prover.
//
// A chunk's contexts go up as 128 bytes per payload (pre-image, hash, reference values, ops); k_zklaim_witness writes what the host pass
// (zkg_zklaim_witness_new + zkg_circuit_sparse_witness) produces for each of them — the tag of every variable and the listed variables in
// ascending order with their Montgomery values — in the packed form the prover's split kernels read.  What allocates which variable is
// host/zklaim_witness_mirror.hpp, compiled here for both sides: the device runs it per payload, the host runs it to count a payload's
// variables (compared with the host pass before anything is launched) and for zkg_zklaim_witness_mirror.
//
// k_zklaim_witness_par is the same generator shaped for one proof's latency (zkg_groth16_prove_zklaim): the serial part of a payload is a
// plain SHA-256 compression on one lane, then one thread per slice of the mirror's trace writes that slice's records at the places a plan
// names.  The plan (cursors, record indices, operand masks) is derived on the host from the mirror's own trace and lives on the device
// beside the 1 / c table, uploaded once per device.
#include "common.hpp"
#include "../../include/zkg.h"
#include "../../include/zklaim_abi.h"
#include "host/zklaim_witness_mirror.hpp"
#include <array>
#include <cstring>
#include <map>
#include <mutex>

using namespace zk;
using namespace zk::zwm;

namespace {

constexpr size_t ZW_TABLE_OFF = 64, ZW_TABLE_BYTES = 65 * 32 + 32, ZW_RECS_OFF = ZW_TABLE_OFF + ZW_TABLE_BYTES;     // input block: [error word | 1 / c table | records]
constexpr size_t ZW_PAR_RECS_OFF = 64;                                      // k_zklaim_witness_par's input block: [error word | records]; its table and plan are resident
constexpr uint32_t ZW_MAX_RECORDS = 1024;                                   // a payload's trace leaves ~800

struct LRec { uint32_t base, v0, m0, v1, m1; };
struct LdsSink {
    LRec *r; uint32_t n;
    ZK_HD void put(uint32_t base, uint32_t v0, uint32_t m0, uint32_t v1, uint32_t m1) {
        if (n < ZW_MAX_RECORDS) { LRec x; x.base = base; x.v0 = v0; x.m0 = m0; x.v1 = v1; x.m1 = m1; r[n] = x; }
        ++n;
    }
};

// the item workgroup of both kernels: one thread per candidate (public-input packings, data, plvars, refvals, alpha_packed, inv): value,
// to_mont, the 0 / 1 / 2 tag, and the listed ones compacted in candidate (= index) order
ZK_D void item_candidates(const Rec *mine, const Fr *inv_table, uint32_t *err, const Layout &L, uint32_t p, uint32_t *desc, Fr *vals, uint32_t *idx, uint8_t *t, bool skip, uint32_t *wcnt /* LDS, 4 */) {
    const uint32_t tid = threadIdx.x, slot = p * L.cap;
    if (skip) { if (tid == 0) { desc[2 * p] = slot; desc[2 * p + 1] = 0; } return; }
    const uint32_t lane = tid & 63, wave = tid >> 6;
    uint32_t listed = 0;
    for (uint32_t q0 = 0; q0 < L.cap; q0 += 256) {
        const uint32_t q = q0 + tid;
        uint32_t tag = 0, pos = 0; Fr val = Fr::zero();
        if (q < L.cap) {
            uint32_t raw[8]; bool is_inv;
            pos = candidate(L, mine, q, raw, is_inv);
            tag = candidate_value(raw, is_inv, inv_table, val);
            if (pos < L.n) t[pos] = (uint8_t)tag; else { atomicOr(err, 2u); tag = 0; }
        }
        const unsigned long long mask = __ballot(tag == 2);
        if (lane == 0) wcnt[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t rank = listed + (uint32_t)__popcll(mask & ((1ull << lane) - 1)), total = 0;
        for (uint32_t w = 0; w < 4; ++w) { if (w < wave) rank += wcnt[w]; total += wcnt[w]; }
        if (tag == 2 && rank < L.cap) { idx[slot + rank] = pos; vals[slot + rank] = val; }
        listed += total;
        __syncthreads();
    }
    if (tid == 0) { desc[2 * p] = slot; desc[2 * p + 1] = listed < L.cap ? listed : L.cap; }
}

// blockIdx.y = item; blockIdx.x < k: that payload's sub-circuit and public bits, blockIdx.x == k: the item's field-element variables.
//   payload: lane 0 runs the mirror's trace on native words and leaves one record per word operation in LDS (the gates' control flow and
//   cursor do not depend on the values: every item takes the same path); the second wavefront writes the payload's public bits meanwhile;
//   then all 256 threads expand the records into tag bytes.  Writes stay inside the payload's own range whatever the cursor does.
//   item: one thread per candidate (public-input packings, data, plvars, refvals, alpha_packed, inv): value, to_mont, the 0 / 1 / 2 tag, and
//   the listed ones compacted in candidate (= index) order.
__global__ __launch_bounds__(256) void k_zklaim_witness(const Rec *recs, const Fr *inv_table, uint32_t *err, Layout L, uint32_t *desc, Fr *vals, uint32_t *idx,
                                                         uint8_t *tags, size_t tag_stride) {
    const uint32_t p = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const Rec *mine = recs + (size_t)p * L.k;
    uint8_t *t = tags + (size_t)p * tag_stride;
    const bool skip = mine[0].skip != 0;
    if (part < L.k) {
        if (skip) return;
        __shared__ LRec lrec[ZW_MAX_RECORDS];
        __shared__ Wd W[64];
        __shared__ Rec rec;
        __shared__ uint32_t nrec;
        if (tid < sizeof(Rec) / 4) reinterpret_cast<uint32_t *>(&rec)[tid] = reinterpret_cast<const uint32_t *>(mine + part)[tid];
        __syncthreads();
        const uint32_t seg = L.o_seg + L.per * part, seg_end = seg + L.per;
        if (tid == 0) {
            LdsSink s; s.r = lrec; s.n = 0;
            const uint32_t end = payload_trace(rec, seg, W, s);
            uint32_t n = s.n;
            if (end != seg_end || n > ZW_MAX_RECORDS) { atomicOr(err, 1u); n = 0; }             // the host compared the counts before the launch: not expected
            nrec = n;
        } else if (tid >= 64 && tid - 64 < ZW_PUBLIC_RECORDS) {
            uint32_t base, v, m;
            public_record(L, rec, part, tid - 64, base, v, m);
            expand(t, L.o_seg, base, v, m, 0, 0);
        }
        __syncthreads();
        for (uint32_t q = tid; q < nrec; q += 256) { const LRec x = lrec[q]; expand(t, seg_end, x.base, x.v0, x.m0, x.v1, x.m1); }
        return;
    }
    __shared__ uint32_t wcnt[4];
    item_candidates(mine, inv_table, err, L, p, desc, vals, idx, t, skip, wcnt);
}

// The generator for one proof's latency.  Same grid, same outputs as k_zklaim_witness; a payload workgroup works in three steps:
//   1. lane 0 computes the plain SHA-256 compression of the padded pre-image and leaves W[0 .. 63] and the state at the entry of every
//      round in LDS (2.3 KB); the third wavefront writes the payload's public bits meanwhile;
//   2. thread q < ZW_SLICES runs slice q of the mirror's trace on those values and the plan's masks, from the plan's cursor, and writes
//      its records at the plan's indices (never past the next slice's first); a slice that ends off the next one's cursor, or leaves
//      another number of records than planned, raises the error word and the payload expands nothing;
//   3. all 256 threads expand the records into tag bytes, inside the payload's own range whatever the cursors were.
__global__ __launch_bounds__(256) void k_zklaim_witness_par(const Rec *recs, const Fr *inv_table, const SlicePlan *plan, uint32_t *err, Layout L, uint32_t *desc, Fr *vals,
                                                             uint32_t *idx, uint8_t *tags, size_t tag_stride) {
    const uint32_t p = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const Rec *mine = recs + (size_t)p * L.k;
    uint8_t *t = tags + (size_t)p * tag_stride;
    const bool skip = mine[0].skip != 0;
    if (part < L.k) {
        if (skip) return;
        __shared__ SliceRec lrec[ZW_MAX_RECORDS];
        __shared__ uint32_t shaW[64], shaS[ZW_SHA_STATE_WORDS];
        __shared__ Rec rec;
        __shared__ uint32_t bad;
        if (tid < sizeof(Rec) / 4) reinterpret_cast<uint32_t *>(&rec)[tid] = reinterpret_cast<const uint32_t *>(mine + part)[tid];
        if (tid == 255) bad = 0;
        __syncthreads();
        const uint32_t seg = L.o_seg + L.per * part, seg_end = seg + L.per;
        if (tid == 0) sha_values(rec, shaW, shaS);
        else if (tid >= 128 && tid - 128 < ZW_PUBLIC_RECORDS) {
            uint32_t base, v, m;
            public_record(L, rec, part, tid - 128, base, v, m);
            expand(t, L.o_seg, base, v, m, 0, 0);
        }
        __syncthreads();
        const uint32_t nrec = plan->e[ZW_SLICES].rec;
        if (tid < ZW_SLICES) {
            const SliceEntry e = plan->e[tid];
            const uint32_t next_cur = plan->e[tid + 1].cur, next_rec = plan->e[tid + 1].rec;
            SliceSink s; s.r = lrec; s.at = e.rec; s.end = next_rec < ZW_MAX_RECORDS ? next_rec : ZW_MAX_RECORDS;
            const uint32_t end = slice_run(rec, e, tid, shaW, shaS, seg, s);
            if (end != next_cur || s.at != next_rec) bad = 1;                               // the host compared the plan with the host pass before the launch: not expected
        } else if (tid == 255 && (plan->e[ZW_SLICES].cur != L.per || nrec > ZW_MAX_RECORDS)) bad = 1;
        __syncthreads();
        if (bad) { if (tid == 0) atomicOr(err, 1u); return; }
        for (uint32_t q = tid; q < nrec; q += 256) { const SliceRec x = lrec[q]; expand(t, seg_end, x.base, x.v0, x.m0, x.v1, x.m1); }
        return;
    }
    __shared__ uint32_t wcnt[4];
    item_candidates(mine, inv_table, err, L, p, desc, vals, idx, t, skip, wcnt);
}

// the generator's own count of a payload's variables (value-independent: any record gives it)
uint32_t mirror_payload_vars() {
    static const uint32_t per = [] { Rec r; memset(&r, 0, sizeof(r)); std::array<Wd, 64> W; CountSink s; return payload_trace(r, 0, W.data(), s); }();
    return per;
}
const Fr *inv_table_host() {
    static const std::array<Fr, 65> tab = [] { std::array<Fr, 65> t; t[0] = Fr::zero(); for (uint64_t i = 1; i <= 64; ++i) t[i] = Fr::from_u64(i).inverse(); return t; }();
    return tab.data();
}
uint8_t op_slot(int op) {                                                  // set_zklaim_ops: which byte of the 8-byte slot is 1
    switch (op) {
    case zklaim_less: return 0;          case zklaim_less_or_eq: return 1;   case zklaim_eq: return 2;        case zklaim_greater_or_eq: return 3;
    case zklaim_greater: return 4;       case zklaim_not_eq: return 5;       case zklaim_noop: return 6;      default: return 0xff;
    }
}
// a context's payloads as records; false: the payload list is not k long
bool pack_ctx(const zklaim_ctx *ctx, uint32_t k, Rec *out) {
    memset(out, 0, (size_t)k * sizeof(Rec));
    if (!ctx || ctx->num_of_payloads != k) return false;
    uint32_t i = 0;
    for (const zklaim_wrap_payload_ctx *cur = ctx->pl_ctx_head; cur; cur = cur->next, ++i) {
        if (i >= k) return false;
        Rec &r = out[i]; const zklaim_payload &pl = cur->pl;
        memcpy(r.pre, pl.pre, 48); memcpy(r.hash, pl.hash, 32);
        for (int j = 0; j < 5; ++j) { r.ref[j] = pl.data_ref[j]; r.op[j] = op_slot(pl.data_op[j]); }
    }
    return i == k;
}

const SlicePlan &slice_plan_host() {
    static const SlicePlan plan = [] { SlicePlan p; slice_plan_derive(p); return p; }();
    return plan;
}
// what k_zklaim_witness_par reads besides the records, resident once per device: [1 / c table | slice plan]
std::mutex g_consts_mu;
std::map<int, void *> g_consts;
const uint8_t *device_consts() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_consts_mu);
    auto it = g_consts.find(dev);
    if (it != g_consts.end()) return static_cast<const uint8_t *>(it->second);
    std::vector<uint8_t> host(ZW_TABLE_BYTES + sizeof(SlicePlan), 0);
    memcpy(host.data(), inv_table_host(), 65 * 32);
    memcpy(host.data() + ZW_TABLE_BYTES, &slice_plan_host(), sizeof(SlicePlan));
    void *d = nullptr;
    if (!hip_ok(hipMalloc(&d, host.size()), "hipMalloc", __FILE__, __LINE__)) return nullptr;
    if (!hip_ok(hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__)) { (void)hipFree(d); return nullptr; }
    g_consts[dev] = d;
    return static_cast<const uint8_t *>(d);
}

}  // namespace

namespace zk {

bool zklaim_witness_plan(uint32_t k, ZwPlan &pl) {
    const uint32_t per = mirror_payload_vars(), host_per = zklaim_payload_vars_host();
    if (!k || per != host_per) {
        set_error("zklaim witness generator: a payload's sub-circuit has " + std::to_string(per) + " variables here, the host pass measures " + std::to_string(host_per) + " (host witnesses are used)");
        return false;
    }
    const Layout L = layout_of(k, per);
    pl.k = k; pl.per = per; pl.n = L.n; pl.cap = L.cap;
    return true;
}
bool zklaim_witness_plan_for_n(size_t n, ZwPlan &pl) {
    const uint32_t per = mirror_payload_vars();
    for (uint32_t k = 1; k <= 64; ++k) {
        const uint32_t nk = layout_of(k, per).n;
        if (nk == n) return zklaim_witness_plan(k, pl);
        if (nk > n) break;
    }
    set_error("zklaim witness generator: no payload count gives the key's " + std::to_string(n) + " variables (host witnesses are used)");
    return false;
}
size_t zklaim_witness_input_bytes(const ZwPlan &pl, uint32_t P) { return ZW_RECS_OFF + (size_t)P * pl.k * sizeof(Rec); }
void zklaim_witness_pack(const ZwPlan &pl, const ::zklaim_ctx *const *ctxs, uint32_t P, uint8_t *host_in, uint8_t *ok) {
    memset(host_in, 0, ZW_TABLE_OFF);
    memset(host_in + ZW_TABLE_OFF, 0, ZW_TABLE_BYTES);
    memcpy(host_in + ZW_TABLE_OFF, inv_table_host(), 65 * 32);
    Rec *recs = reinterpret_cast<Rec *>(host_in + ZW_RECS_OFF);
    for (uint32_t p = 0; p < P; ++p) {
        Rec *r = recs + (size_t)p * pl.k;
        ok[p] = pack_ctx(ctxs[p], pl.k, r) ? 1 : 0;
        if (!ok[p]) { memset(r, 0, (size_t)pl.k * sizeof(Rec)); r[0].skip = 1; }
    }
}
int zklaim_witness_launch(const ZwPlan &pl, uint32_t P, uint8_t *d_in, uint32_t *d_desc, Fr *d_vals, uint32_t *d_idx, uint8_t *d_tags, size_t tag_stride, hipStream_t s) {
    const Layout L = layout_of(pl.k, pl.per);
    if (!P || L.n != pl.n || tag_stride < L.n) { set_error("zklaim witness generator: bad launch"); return ZKG_ERROR; }
    ZK_HIP(hipMemsetAsync(d_tags, 0, (size_t)P * tag_stride, s));
    hipLaunchKernelGGL(k_zklaim_witness, dim3(pl.k + 1, P), dim3(256), 0, s, reinterpret_cast<const Rec *>(d_in + ZW_RECS_OFF), reinterpret_cast<const Fr *>(d_in + ZW_TABLE_OFF),
                       reinterpret_cast<uint32_t *>(d_in), L, d_desc, d_vals, d_idx, d_tags, tag_stride);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
// the plan of the slices agrees with the plan of the payload: same segment size, records within the kernel's LDS
bool zklaim_witness_par_ready(const ZwPlan &pl) {
    const SliceEntry &last = slice_plan_host().e[ZW_SLICES];
    if (last.cur != pl.per || last.rec > ZW_MAX_RECORDS) { set_error("zklaim witness generator: the slices' plan does not end at the payload's size (host witnesses are used)"); return false; }
    return true;
}
size_t zklaim_witness_par_input_bytes(const ZwPlan &pl, uint32_t P) { return ZW_PAR_RECS_OFF + (size_t)P * pl.k * sizeof(Rec); }
void zklaim_witness_par_pack(const ZwPlan &pl, const ::zklaim_ctx *const *ctxs, uint32_t P, uint8_t *host_in, uint8_t *ok) {
    memset(host_in, 0, ZW_PAR_RECS_OFF);
    Rec *recs = reinterpret_cast<Rec *>(host_in + ZW_PAR_RECS_OFF);
    for (uint32_t p = 0; p < P; ++p) {
        Rec *r = recs + (size_t)p * pl.k;
        ok[p] = pack_ctx(ctxs[p], pl.k, r) ? 1 : 0;
        if (!ok[p]) { memset(r, 0, (size_t)pl.k * sizeof(Rec)); r[0].skip = 1; }
    }
}
int zklaim_witness_par_launch(const ZwPlan &pl, uint32_t P, uint8_t *d_in, uint32_t *d_desc, Fr *d_vals, uint32_t *d_idx, uint8_t *d_tags, size_t tag_stride, hipStream_t s) {
    const Layout L = layout_of(pl.k, pl.per);
    if (!P || P > 65535 || L.n != pl.n || tag_stride < L.n || !zklaim_witness_par_ready(pl)) { set_error("zklaim witness generator: bad launch"); return ZKG_ERROR; }
    const uint8_t *consts = device_consts();
    if (!consts) return ZKG_ERROR;
    ZK_HIP(hipMemsetAsync(d_tags, 0, (size_t)P * tag_stride, s));
    hipLaunchKernelGGL(k_zklaim_witness_par, dim3(pl.k + 1, P), dim3(256), 0, s, reinterpret_cast<const Rec *>(d_in + ZW_PAR_RECS_OFF), reinterpret_cast<const Fr *>(consts),
                       reinterpret_cast<const SlicePlan *>(consts + ZW_TABLE_BYTES), reinterpret_cast<uint32_t *>(d_in), L, d_desc, d_vals, d_idx, d_tags, tag_stride);
    ZK_HIP(hipGetLastError());
    return ZKG_OK;
}
void zklaim_witness_release_all() {
    std::lock_guard<std::mutex> lk(g_consts_mu);
    int cur = 0; (void)hipGetDevice(&cur);
    for (auto &c : g_consts) { if (hipSetDevice(c.first) == hipSuccess) (void)hipFree(c.second); }
    g_consts.clear();
    (void)hipSetDevice(cur);
}

}  // namespace zk

static size_t round_up64(size_t x) { return (x + 63) / 64 * 64; }

extern "C" {

size_t zkg_zklaim_witness_size(size_t payloads, size_t *cap_listed) {
    if (!payloads || payloads > 64) return 0;
    const Layout L = layout_of((uint32_t)payloads, mirror_payload_vars());
    if (cap_listed) *cap_listed = L.cap;
    return L.n;
}

static int witness_mirror_impl(const zklaim_ctx *ctx, uint8_t *tags_out, uint32_t *index_out, uint64_t *values_out, size_t cap_listed, size_t *listed_count, bool par) {
    {
        if (!ctx || !tags_out || !listed_count || (cap_listed && (!index_out || !values_out))) { set_error("zkg_zklaim_witness_mirror: null argument"); return ZKG_ERROR; }
        const size_t k = ctx->num_of_payloads;
        if (!k || k > 64) { set_error("zkg_zklaim_witness_mirror: payload count out of range"); return ZKG_ERROR; }
        std::vector<Rec> recs(k);
        if (!pack_ctx(ctx, (uint32_t)k, recs.data())) { set_error("zkg_zklaim_witness_mirror: num_of_payloads disagrees with the payload list"); return ZKG_ERROR; }
        const uint32_t per = mirror_payload_vars();
        const Layout L = layout_of((uint32_t)k, per);
        memset(tags_out, 0, L.n);
        std::array<Wd, 64> W;
        for (uint32_t i = 0; i < k; ++i) {
            const uint32_t seg = L.o_seg + per * i;
            if (par) {
                // the device path's three steps: the value pass, every slice on its own (last one first: none may lean on another), the expansion
                const SlicePlan &plan = slice_plan_host();
                const uint32_t nrec = plan.e[ZW_SLICES].rec;
                if (plan.e[ZW_SLICES].cur != per || nrec > ZW_MAX_RECORDS) { set_error("zkg_zklaim_witness_mirror_parallel: the slices' plan does not end at the payload's size"); return ZKG_ERROR; }
                std::array<uint32_t, 64> shaW; std::array<uint32_t, ZW_SHA_STATE_WORDS> shaS;
                sha_values(recs[i], shaW.data(), shaS.data());
                std::vector<SliceRec> lrec(nrec);
                for (uint32_t q = ZW_SLICES; q-- > 0;) {
                    SliceSink s; s.r = lrec.data(); s.at = plan.e[q].rec; s.end = plan.e[q + 1].rec;
                    const uint32_t end = slice_run(recs[i], plan.e[q], q, shaW.data(), shaS.data(), seg, s);
                    if (end != plan.e[q + 1].cur || s.at != plan.e[q + 1].rec) { set_error("zkg_zklaim_witness_mirror_parallel: a slice ended off its planned cursor"); return ZKG_ERROR; }
                }
                for (const SliceRec &x : lrec) expand(tags_out, seg + per, x.base, x.v0, x.m0, x.v1, x.m1);
            } else {
                TagSink s; s.tags = tags_out; s.limit = seg + per;
                if (payload_trace(recs[i], seg, W.data(), s) != seg + per) { set_error("zkg_zklaim_witness_mirror: payload sub-circuits differ in size"); return ZKG_ERROR; }
            }
            for (uint32_t q = 0; q < ZW_PUBLIC_RECORDS; ++q) { uint32_t base, v, m; public_record(L, recs[i], i, q, base, v, m); expand(tags_out, L.o_seg, base, v, m, 0, 0); }
        }
        size_t cnt = 0;
        for (uint32_t q = 0; q < L.cap; ++q) {
            uint32_t raw[8]; bool is_inv; Fr val;
            const uint32_t pos = candidate(L, recs.data(), q, raw, is_inv);
            const uint8_t tag = candidate_value(raw, is_inv, inv_table_host(), val);
            if (pos >= L.n) { set_error("zkg_zklaim_witness_mirror: variable out of range"); return ZKG_ERROR; }
            tags_out[pos] = tag;
            if (tag != 2) continue;
            if (cnt >= cap_listed) { set_error("zkg_zklaim_witness_mirror: cap_listed too small"); return ZKG_ERROR; }
            index_out[cnt] = pos; memcpy(values_out + 4 * cnt, val.v, 32); ++cnt;
        }
        *listed_count = cnt;
        return ZKG_OK;
    }
}
int zkg_zklaim_witness_mirror(const zklaim_ctx *ctx, uint8_t *tags_out, uint32_t *index_out, uint64_t *values_out, size_t cap_listed, size_t *listed_count) {
    return c_boundary("zkg_zklaim_witness_mirror", ZKG_ERROR, [&] { return witness_mirror_impl(ctx, tags_out, index_out, values_out, cap_listed, listed_count, false); });
}
int zkg_zklaim_witness_mirror_parallel(const zklaim_ctx *ctx, uint8_t *tags_out, uint32_t *index_out, uint64_t *values_out, size_t cap_listed, size_t *listed_count) {
    return c_boundary("zkg_zklaim_witness_mirror_parallel", ZKG_ERROR, [&] { return witness_mirror_impl(ctx, tags_out, index_out, values_out, cap_listed, listed_count, true); });
}

static int witness_gpu_impl(const zklaim_ctx *const *ctxs, size_t count, uint8_t *tags_out, uint32_t *index_out, uint64_t *values_out, size_t cap_listed, size_t *listed_counts, bool par) {
    if (!count) return ZKG_OK;
    if (!ctxs || !tags_out || !listed_counts || (cap_listed && (!index_out || !values_out))) { set_error("zkg_zklaim_witness_gpu: null argument"); return ZKG_ERROR; }
    if (initialised_device() < 0) { set_error("zkg_zklaim_witness_gpu: zkg_init has not been called"); return ZKG_ERROR; }
    if (count > 65535) { set_error("zkg_zklaim_witness_gpu: too many contexts"); return ZKG_ERROR; }
    size_t k = 0;
    for (size_t i = 0; i < count && !k; ++i) if (ctxs[i]) k = ctxs[i]->num_of_payloads;
    ZwPlan pl;
    if (!k || k > 64 || !zklaim_witness_plan((uint32_t)k, pl)) { if (!k || k > 64) set_error("zkg_zklaim_witness_gpu: no context with a payload count in range"); return ZKG_ERROR; }
    const uint32_t P = (uint32_t)count;
    const size_t n = pl.n, tag_stride = (n + 15) / 16 * 16, total = (size_t)P * pl.cap;
    const size_t o_vals = round_up64((size_t)P * 8), o_idx = o_vals + total * 32, o_tags = round_up64(o_idx + total * 4), o_in = round_up64(o_tags + P * tag_stride),
                 in_bytes = par ? zklaim_witness_par_input_bytes(pl, P) : zklaim_witness_input_bytes(pl, P), bytes = o_in + in_bytes;
    std::vector<uint8_t> host(bytes), ok(P);
    if (par) zklaim_witness_par_pack(pl, ctxs, P, host.data() + o_in, ok.data()); else zklaim_witness_pack(pl, ctxs, P, host.data() + o_in, ok.data());
    ScopedDevBuf dev;
    if (dev.reserve(bytes)) return ZKG_ERROR;
    uint8_t *d = dev.as<uint8_t>();
    ZK_HIP(hipMemcpy(d + o_in, host.data() + o_in, in_bytes, hipMemcpyHostToDevice));
    if ((par ? zklaim_witness_par_launch : zklaim_witness_launch)(pl, P, d + o_in, reinterpret_cast<uint32_t *>(d), reinterpret_cast<Fr *>(d + o_vals), reinterpret_cast<uint32_t *>(d + o_idx), d + o_tags, tag_stride, nullptr)) return ZKG_ERROR;
    ZK_HIP(hipStreamSynchronize(nullptr));
    ZK_HIP(hipMemcpy(host.data(), d, o_in + 64, hipMemcpyDeviceToHost));
    uint32_t err; memcpy(&err, host.data() + o_in, 4);
    if (err) { set_error("zkg_zklaim_witness_gpu: the generator's cursor left its range"); return ZKG_ERROR; }
    for (uint32_t p = 0; p < P; ++p) {
        uint32_t dsc[2]; memcpy(dsc, host.data() + 8 * (size_t)p, 8);
        memcpy(tags_out + (size_t)p * n, host.data() + o_tags + (size_t)p * tag_stride, n);
        if (!ok[p]) { listed_counts[p] = (size_t)-1; continue; }
        if (dsc[1] > cap_listed) { set_error("zkg_zklaim_witness_gpu: cap_listed too small"); return ZKG_ERROR; }
        listed_counts[p] = dsc[1];
        if (dsc[1]) {
            memcpy(index_out + (size_t)p * cap_listed, host.data() + o_idx + 4 * (size_t)dsc[0], 4 * (size_t)dsc[1]);
            memcpy(values_out + 4 * (size_t)p * cap_listed, host.data() + o_vals + 32 * (size_t)dsc[0], 32 * (size_t)dsc[1]);
        }
    }
    return ZKG_OK;
}
int zkg_zklaim_witness_gpu(const zklaim_ctx *const *ctxs, size_t count, uint8_t *tags_out, uint32_t *index_out, uint64_t *values_out, size_t cap_listed, size_t *listed_counts) {
    return c_boundary("zkg_zklaim_witness_gpu", ZKG_ERROR, [&] { return witness_gpu_impl(ctxs, count, tags_out, index_out, values_out, cap_listed, listed_counts, false); });
}
int zkg_zklaim_witness_gpu_parallel(const zklaim_ctx *const *ctxs, size_t count, uint8_t *tags_out, uint32_t *index_out, uint64_t *values_out, size_t cap_listed, size_t *listed_counts) {
    return c_boundary("zkg_zklaim_witness_gpu_parallel", ZKG_ERROR, [&] { return witness_gpu_impl(ctxs, count, tags_out, index_out, values_out, cap_listed, listed_counts, true); });
}

}  // extern "C"
