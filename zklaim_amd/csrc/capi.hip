// capi.hip — the C ABI of include/zkg.h over the HIP kernels (host code only).
//
// This is the thin shim the reference's C/C++ front-end binds instead of libsnark: the entry
// points sit directly below r1cs_gg_ppzksnark_prover (/root/reference/zklaim/snark.cpp:126).
// There is no CPU fallback: every entry point fails with ZKG_ERROR when no HIP device is usable.
#include "common.hpp"
#include "fq29.hip.hpp"
#include "fr29.hip.hpp"
#include "../../include/zkg.h"
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <dlfcn.h>
#include <rccl/rccl.h>                  // types and prototypes only: the library is opened at run time (rccl_api), never linked

namespace zk {

static thread_local std::string t_error;
static std::string g_error;
static std::mutex g_err_mu;
void set_error(const std::string &msg) { t_error = msg; std::lock_guard<std::mutex> lk(g_err_mu); g_error = msg; }
bool hip_ok(hipError_t e, const char *what, const char *file, int line) {
    if (e == hipSuccess) return true;
    set_error(std::string(what) + ": " + hipGetErrorString(e) + " at " + file + ":" + std::to_string(line));
    return false;
}

thread_local ReserveGuard *t_reserve_guard = nullptr;
int DevBuf::reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    // growing frees the buffer: under a ReserveGuard (work of earlier calls may still read it) the guarded stream is drained first
    if (t_reserve_guard) { (void)hip_ok(hipStreamSynchronize(t_reserve_guard->stream), "hipStreamSynchronize", __FILE__, __LINE__); ++t_reserve_guard->drains; }
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    size_t want = bytes + bytes / 8 + 256;
    if (!hip_ok(hipMalloc(&p, want), "hipMalloc", __FILE__, __LINE__)) { p = nullptr; return 1; }
    cap = want;
    return 0;
}
void DevBuf::release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }

int HandleOrder::create() { ZK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); return ZKG_OK; }
int HandleOrder::order_behind(hipStream_t s) { if (pending && s != last) ZK_HIP(hipStreamWaitEvent(s, ev, 0)); return ZKG_OK; }
int HandleOrder::wait_host() { if (pending) ZK_HIP(hipEventSynchronize(ev)); return ZKG_OK; }
int HandleOrder::grow(DevBuf &ws, size_t need, size_t &waits) {
    if (need <= ws.cap) return ZKG_OK;
    if (wait_host() || ws.reserve(need)) return ZKG_ERROR;               // earlier calls may still be in it
    ++waits;
    return ZKG_OK;
}
void HandleOrder::record(hipStream_t s) { if (hipEventRecord(ev, s) == hipSuccess) carried(s); }
void HandleOrder::destroy() { if (ev) { if (pending) (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); ev = nullptr; pending = false; } }

KernelTimer g_dominant_timer;
bool crit_priority_for(int part, unsigned log_m) {
    static const int parts = getenv("ZKG_CRIT_PRIO_PARTS") ? atoi(getenv("ZKG_CRIT_PRIO_PARTS")) : 7;
    static const unsigned min_log = getenv("ZKG_CRIT_PRIO_MIN_LOG") ? (unsigned)atoi(getenv("ZKG_CRIT_PRIO_MIN_LOG")) : CRIT_PRIORITY_MIN_LOG;
    return crit_priority_enabled() && (parts & part) && log_m >= min_log;
}
static std::mutex g_timer_mu;
static constexpr size_t TIMER_MAX_PAIRS = 4096;              // a long-running host that never drains the timer stops recording here
void KernelTimer::new_call() {
    static const size_t stride = getenv("ZKG_KERNEL_TIMER_STRIDE") ? (size_t)std::max(1, atoi(getenv("ZKG_KERNEL_TIMER_STRIDE"))) : 4;
    std::lock_guard<std::mutex> lk(g_timer_mu);
    sample = (calls++ % stride) == 0;
    ++calls_seen; if (sample) ++calls_timed;
}
void KernelTimer::begin(hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_timer_mu);
    pending = false;
    if (!sample) return;
    static const bool off = getenv("ZKG_KERNEL_TIMER") && atoi(getenv("ZKG_KERNEL_TIMER")) == 0;      // A/B switch: what the two event records per launch cost the step
    if (off || !enabled || used >= TIMER_MAX_PAIRS) return;
    // (timing only: no system-scope fence — the write-back of whatever the kernel before left dirty would be timed and would delay the kernel behind)
    static const unsigned tf = hipEventDisableSystemFence;
    if (used == pairs.size()) { hipEvent_t a, b; if (hipEventCreateWithFlags(&a, tf) != hipSuccess || hipEventCreateWithFlags(&b, tf) != hipSuccess) { enabled = false; return; } pairs.push_back({a, b}); }
    (void)hipEventRecord(pairs[used].first, s);
    pending = true;
}
void KernelTimer::end(hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_timer_mu);
    if (!pending) return;
    (void)hipEventRecord(pairs[used].second, s); ++used; pending = false;
}
float KernelTimer::drain(int *launches) {
    std::lock_guard<std::mutex> lk(g_timer_mu);
    float total = 0; int n = 0;
    for (size_t i = 0; i < used; ++i) {
        float ms = 0;
        if (hipEventSynchronize(pairs[i].second) == hipSuccess && hipEventElapsedTime(&ms, pairs[i].first, pairs[i].second) == hipSuccess) { total += ms; ++n; }
    }
    if (launches) *launches = calls_timed ? (int)((size_t)n * calls_seen / calls_timed) : n;
    return n ? total / n : 0.f;
}
void KernelTimer::reset() { std::lock_guard<std::mutex> lk(g_timer_mu); used = 0; pending = false; calls = 0; calls_seen = 0; calls_timed = 0; sample = true; }

// ---- host thread pool -------------------------------------------------------------------------------------
namespace {
struct Run {                                   // one parallel_for: workers that wake late see next >= n and touch nothing else
    std::function<void(int)> fn; int n = 0; std::atomic<int> next{0}, done{0};
};
struct Pool {
    std::vector<std::thread> workers;
    std::mutex mu; std::condition_variable cv_work, cv_done;
    std::shared_ptr<Run> cur; uint64_t epoch = 0; bool stop = false;
    std::mutex run_mu;                         // one parallel_for at a time
    Pool() {
        unsigned hw = std::thread::hardware_concurrency();
        int nw = (int)(hw > 16 ? 15 : (hw > 1 ? hw - 1 : 0));
        for (int i = 0; i < nw; ++i) workers.emplace_back([this] { loop(); });
    }
    ~Pool() {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv_work.notify_all();
        for (auto &t : workers) t.join();
    }
    void drain(Run &r) {
        for (int i; (i = r.next.fetch_add(1)) < r.n;) {
            r.fn(i);
            if (r.done.fetch_add(1) + 1 == r.n) { std::lock_guard<std::mutex> lk(mu); cv_done.notify_all(); }
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            std::shared_ptr<Run> r;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return stop || epoch != seen; });
                if (stop) return;
                seen = epoch; r = cur;
            }
            drain(*r);
        }
    }
    bool try_run(int count, const std::function<void(int)> &f) {              // the pool's turn if it is free; false (nothing done) if it is busy
        if (workers.empty()) return false;
        std::unique_lock<std::mutex> rl(run_mu, std::defer_lock);
        if (!rl.try_lock()) return false;
        auto r = std::make_shared<Run>(); r->fn = f; r->n = count;
        { std::lock_guard<std::mutex> lk(mu); cur = r; ++epoch; }
        cv_work.notify_all();
        drain(*r);
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return r->done.load() == r->n; });
        return true;
    }
    void run(int count, const std::function<void(int)> &f, bool wait_for_pool) {
        if (count <= 1 || workers.empty()) { for (int i = 0; i < count; ++i) f(i); return; }
        // the pool runs one loop at a time; a caller that finds it busy (the seam's key-digest thread hashing 200 MB, say) does its own
        // few tasks inline rather than queueing behind it — these loops sit on the latency path of a proof
        std::unique_lock<std::mutex> rl(run_mu, std::defer_lock);
        if (wait_for_pool) rl.lock();
        else if (!rl.try_lock()) { for (int i = 0; i < count; ++i) f(i); return; }
        auto r = std::make_shared<Run>(); r->fn = f; r->n = count;
        { std::lock_guard<std::mutex> lk(mu); cur = r; ++epoch; }
        cv_work.notify_all();
        drain(*r);
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return r->done.load() == r->n; });
    }
};
}  // namespace
static Pool &host_pool() { static Pool pool; return pool; }
void host_parallel_for(int n, const std::function<void(int)> &fn) { host_pool().run(n, fn, false); }
void host_parallel_for_wait(int n, const std::function<void(int)> &fn) { host_pool().run(n, fn, true); }
// heavy loops (tens of milliseconds of work: a credential circuit's synthesis with its constraints) that find the pool busy — the key loader hashing and
// parsing a blob, in the same first libsnark_prove — neither run inline (28 ms on one thread instead of 5) nor queue behind it: they get threads of
// their own for the call.  Creating them costs ~0.3 ms; not for the short loops of a proof's latency path.
void host_parallel_for_spawn(int n, const std::function<void(int)> &fn) {
    if (n <= 1) { for (int i = 0; i < n; ++i) fn(i); return; }
    if (host_pool().try_run(n, fn)) return;
    const int nt = std::min(n, 15);
    std::atomic<int> next{0};
    std::vector<std::thread> th; th.reserve((size_t)nt);
    auto work = [&] { for (int i; (i = next.fetch_add(1)) < n;) fn(i); };
    for (int t = 0; t < nt - 1; ++t) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}

// ---- ABI point encodings -----------------------------------------------------------------------
static void put(uint64_t *out, const Fq &a) { memcpy(out, a.v, 32); }
static Fq get(const uint64_t *in) { Fq r; memcpy(r.v, in, 32); return r; }
void store_norm(uint64_t *out, const G1 &p) {
    G1Affine a = p.to_affine();
    if (p.is_inf()) { put(out, Fq::zero()); put(out + 4, Fq::one()); put(out + 8, Fq::zero()); }
    else { put(out, a.x); put(out + 4, a.y); put(out + 8, Fq::one()); }
}
void store_norm(uint64_t *out, const G2 &p) {
    G2Affine a = p.to_affine();
    if (p.is_inf()) { put(out, Fq::zero()); put(out + 4, Fq::zero()); put(out + 8, Fq::one()); put(out + 12, Fq::zero()); put(out + 16, Fq::zero()); put(out + 20, Fq::zero()); }
    else { put(out, a.x.c0); put(out + 4, a.x.c1); put(out + 8, a.y.c0); put(out + 12, a.y.c1); put(out + 16, Fq::one()); put(out + 20, Fq::zero()); }
}
G1 load_norm_g1(const uint64_t *in) {
    Fq z = get(in + 8);
    if (z.is_zero()) return G1::inf();
    return {get(in), get(in + 4), Fq::one(), Fq::one()};           // normalised: Z == 1
}
G2 load_norm_g2(const uint64_t *in) {
    Fq2 z = {get(in + 16), get(in + 20)};
    if (z.is_zero()) return G2::inf();
    return {{get(in), get(in + 4)}, {get(in + 8), get(in + 12)}, Fq2::one(), Fq2::one()};
}

// ---- device field arithmetic, element-wise (the known-answer hook behind zkg_field_op) ---------------------------
template <class F> ZK_D F field_apply(int op, const F &x, const F &y) {
    switch (op) {
    case 0: return x * y;   case 1: return x + y;   case 2: return x - y;   case 3: return x.inverse();
    case 6: return x.neg(); case 7: return x.sqr();
    case 8: return x.dbl();
    default: return x;
    }
}
// ops 20-28 and 40-42: the stores stay RAW (no normalized()), so the representative an operator leaves in [0, 2p) is what the caller reads
template <class F> ZK_D F field_apply_raw(int op, const F &x, const F &y) {
    switch (op) {
    case 20: return x * y;   case 21: return x + y;   case 22: return x - y;
    case 26: return x.neg(); case 27: return x.sqr(); case 28: return x.dbl();
    case 40: return ((x * y) - x) * (x + y);
    case 41: { F t = x; for (int k = 0; k < 8; ++k) t = (t + t) - y; return t; }
    default: { F xx = x.sqr(), M = xx.dbl() + xx; return M.sqr() - (x * y).dbl(); }         // 42: the shape dbl_inl builds
    }
}
template <class F> ZK_D F field_flag(bool f) {
    F r = F::zero();
    if constexpr (sizeof(F) == sizeof(Fq)) r.v[0] = f ? 1u : 0u; else r.c0.v[0] = f ? 1u : 0u;
    return r;
}
template <class F> __global__ __launch_bounds__(64) void k_field_op(int op, const F *a, const F *b, size_t n, F *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F x = a[i], y = b ? b[i] : x;
    if constexpr (sizeof(F) == sizeof(Fq)) {
        if (op == 4) { out[i] = x.to_mont().normalized(); return; }
        if (op == 5) { out[i] = x.from_mont(); return; }
    }
    if constexpr (std::is_same<F, Fq>::value) {
        // the 29-bit representation of the accumulation kernel (fq29.hip.hpp), entered and left through its own conversions
        if (op >= 10 && op <= 15) {
            const Fq29 xa = f29::to29(x), yb = f29::to29(y);
            Fq29 r = xa;
            if (op == 10) r = f29::mul(xa, yb);
            else if (op == 15) r = f29::inverse(f29::norm(f29::add(f29::add(xa, xa), xa)));      // 1 / (3 a): an unreduced sum as input
            else if (op == 11) r = f29::norm(f29::add(xa, yb));
            else if (op == 12) r = f29::norm(f29::sub(xa, f29::S2_1, yb));
            else if (op == 14) {                 // a chain as the mixed addition builds them: unnormalised differences into products
                const Fq29 d = f29::sub(xa, f29::S6_1, yb), e = f29::norm(f29::sub(yb, f29::S4_1, xa));
                r = f29::norm(f29::sub(f29::mul(e, d), f29::S4_3, f29::add(f29::mul(e, e), f29::dbl(f29::mul(xa, yb)))));      // (b-a)(a-b) - (b-a)^2 - 2ab
            }
            Fq o = f29::from29(r);
            if (op == 13 && f29::is_zero_mod_p(f29::norm(f29::sub(xa, f29::S2_1, yb)))) o = Fq::zero();                          // zero test: out = 0 iff a == b
            out[i] = o; return;
        }
    }
    if (op >= 20) {
        if (op == 30) out[i] = field_flag<F>(x.is_zero());
        else if (op == 31) out[i] = field_flag<F>(x == y);
        else out[i] = field_apply_raw(op, x, y);
        return;
    }
    out[i] = field_apply(op, x, y).normalized();
}
template <class F> static int field_op_run(int op, const uint64_t *a, const uint64_t *b, size_t n, uint64_t *out) {
    DevBuf da, db, dout;
    const size_t bytes = n * sizeof(F);
    int rc = ZKG_ERROR;
    if (!da.reserve(bytes) && !dout.reserve(bytes) && (!b || !db.reserve(bytes)) &&
        hip_ok(hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__) &&
        (!b || hip_ok(hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__))) {
        hipLaunchKernelGGL(k_field_op<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, op, da.as<F>(), b ? db.as<F>() : (const F *)nullptr, n, dout.as<F>());
        if (hipGetLastError() == hipSuccess && hip_ok(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__)) rc = ZKG_OK;
    }
    da.release(); db.release(); dout.release();
    return rc;
}

// ---- the NTT's 29-bit Fr arithmetic on raw limbs (the known-answer hook behind zkg_fr29_op): one lane per element, k vectors of nine
//      limbs in, m out.
// COPIES of the radix-4 step and of the odd-R tail step of k_ntt_pass29_r4 (csrc/ntt.hip), from the loaded records to the stored ones — the
// kernel keeps its own text (moving the body into a shared function changed its register allocation): keep the two alike, line by line.
ZK_D void fr29_r4_step_copy(Fr29 &r0, Fr29 &r1, Fr29 &r2, Fr29 &r3, const Fr29 &wa, const Fr29 &wb, const Fr29 &wc, bool product, bool norm_stores) {
    Fr29 x0 = r0, x2 = r2;
    if (!norm_stores) { x0 = fr29::norm(x0); x2 = fr29::norm(x2); }
    Fr29 t1 = r1, t3 = r3;
    if (product) { fr29::mul2(t1, t3, t1, wa, t3, wa); }
    else if (!norm_stores) { t1 = fr29::norm(t1); t3 = fr29::norm(t3); }      // (stage 0 has no product to bring them back to digits)
    const Fr29 y0 = fr29::add_lazy(x0, t1), y1 = fr29::sub_lazy(x0, t1), y2 = fr29::add_lazy(x2, t3), y3 = fr29::sub_lazy(x2, t3);
    Fr29 u2, u3;
    fr29::mul2(u2, u3, y2, wb, y3, wc);
    if (norm_stores) {
        r0 = fr29::norm(fr29::add_lazy(y0, u2));
        r2 = fr29::norm(fr29::sub_lazy(y0, u2));
        r1 = fr29::norm(fr29::add_lazy(y1, u3));
        r3 = fr29::norm(fr29::sub_lazy(y1, u3));
    } else {
        r0 = fr29::add_lazy(y0, u2);
        r2 = fr29::sub_lazy(y0, u2);
        r1 = fr29::add_lazy(y1, u3);
        r3 = fr29::sub_lazy(y1, u3);
    }
}
ZK_D void fr29_r2_tail_copy(Fr29 &r0, Fr29 &r1, const Fr29 &w, bool product) {
    const Fr29 u = fr29::norm(r0);
    Fr29 v = r1;
    if (product) v = fr29::mul(v, w);
    else v = fr29::norm(v);
    r0 = fr29::add_norm(u, v);
    r1 = fr29::sub_norm(u, v);
}
static constexpr int FR29_OPS = 15;
static const int FR29_K[FR29_OPS] = {2, 4, 1, 2, 2, 2, 2, 1, 1, 7, 7, 7, 7, 3, 3};
static const int FR29_M[FR29_OPS] = {1, 2, 1, 1, 1, 1, 1, 1, 1, 4, 4, 4, 4, 2, 2};
__global__ __launch_bounds__(64) void k_fr29_op(int op, int k, int m, const uint32_t *in, size_t n, uint32_t *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr29 x[7], y[4];
    for (int j = 0; j < 7; ++j) for (int l = 0; l < 9; ++l) x[j].v[l] = j < k ? in[(i * k + j) * 9 + l] : 0u;
    for (int j = 0; j < 4; ++j) for (int l = 0; l < 9; ++l) y[j].v[l] = 0u;
    switch (op) {
    case 0: y[0] = fr29::mul(x[0], x[1]); break;
    case 1: fr29::mul2(y[0], y[1], x[0], x[1], x[2], x[3]); break;
    case 2: y[0] = fr29::norm(x[0]); break;
    case 3: y[0] = fr29::add_norm(x[0], x[1]); break;
    case 4: y[0] = fr29::sub_norm(x[0], x[1]); break;
    case 5: y[0] = fr29::add_lazy(x[0], x[1]); break;
    case 6: y[0] = fr29::sub_lazy(x[0], x[1]); break;
    case 7: { Fr f; for (int l = 0; l < 8; ++l) f.v[l] = x[0].v[l]; y[0] = fr29::slice(f); break; }
    case 8: { const Fr f = fr29::unslice_reduce(x[0]); for (int l = 0; l < 8; ++l) y[0].v[l] = f.v[l]; break; }
    case 9: case 10: case 11: case 12:
        fr29_r4_step_copy(x[0], x[1], x[2], x[3], x[4], x[5], x[6], op == 9 || op == 11, op >= 11);
        y[0] = x[0]; y[1] = x[1]; y[2] = x[2]; y[3] = x[3];
        break;
    default:
        fr29_r2_tail_copy(x[0], x[1], x[2], op == 13);
        y[0] = x[0]; y[1] = x[1];
        break;
    }
    for (int j = 0; j < m; ++j) for (int l = 0; l < 9; ++l) out[(i * m + j) * 9 + l] = y[j].v[l];
}
static int fr29_op_run(int op, const uint32_t *in, size_t n, uint32_t *out) {
    DevBuf din, dout;
    const int k = FR29_K[op], m = FR29_M[op];
    const size_t in_bytes = n * k * 9 * sizeof(uint32_t), out_bytes = n * m * 9 * sizeof(uint32_t);
    int rc = ZKG_ERROR;
    if (!din.reserve(in_bytes) && !dout.reserve(out_bytes) && hip_ok(hipMemcpy(din.p, in, in_bytes, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__)) {
        hipLaunchKernelGGL(k_fr29_op, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, op, k, m, din.as<uint32_t>(), n, dout.as<uint32_t>());
        if (hipGetLastError() == hipSuccess && hip_ok(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__)) rc = ZKG_OK;
    }
    din.release(); dout.release();
    return rc;
}

// known-answer hook for the 29-bit group law of the reduction kernels (fq29.hip.hpp xyzz29_add_quad): out[i] = a[i] + b[i], one DPP quad
// per pair, points as XYZZ<Fq> in and out (converted by the same quad_load29 / from29 the kernels use)
__global__ __launch_bounds__(64) void k_add_quad29(const XYZZ<Fq> *a, const XYZZ<Fq> *b, size_t n, int chain, XYZZ<Fq> *out) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2; const uint32_t q = threadIdx.x & 3;
    if (i >= n) return;
    const XYZZ<Fq> pa = a[i], pb = b[i];
    XYZZ29q x = pa.is_inf() ? XYZZ29q::inf() : quad_load29(pa.x, pa.y, pa.zz, pa.zzz, q);
    const XYZZ29q y = pb.is_inf() ? XYZZ29q::inf() : quad_load29(pb.x, pb.y, pb.zz, pb.zzz, q);
    if (chain < 0) xyzz29_add_lane(x, y); else
    xyzz29_add_quad(x, y, q);
    for (int k = 0; k < chain; ++k) { XYZZ29q z = x; xyzz29_add_quad(x, y, q); xyzz29_add_quad(x, z, q); }     // sums of sums: the invariants across additions
    if (q == 0) out[i] = x.is_inf() ? XYZZ<Fq>::inf().normalized() : XYZZ<Fq>{f29::from29(x.x), f29::from29(x.y), f29::from29(x.zz), f29::from29(x.zzz)};
}

// ---- the multi-exponentiation's 29-bit Fq arithmetic on raw limbs (the known-answer hook behind zkg_fq29_op): k vectors of nine limbs
//      in, m out, no to29 on the way in and no from29 on the way out, so that a caller can place limbs and values AT the lazy bounds the
//      comments of fq29.hip.hpp state.  One lane per element; the pair and quad additions take 2 and 4 lanes per element.
// COPY of the exceptional path of k_bucket_accum29 (csrc/msm.hip), from the false return of XYZZ29::madd to the accumulator's new value —
// the kernel keeps its own text (its register allocation is tuned: ACC29_VGPRS): keep the two alike, line by line.
ZK_D void fq29_madd_fallback_copy(XYZZ29 &acc, const Fq29 &bx, const Fq29 &by, bool &inf) {
    XYZZ<Fq> a32 = {f29::from29(acc.x), f29::from29(acc.y), f29::from29(acc.zz), f29::from29(acc.zzz)};
    a32.madd(Affine<Fq>{f29::from29(bx), f29::from29(f29::norm(by))});
    if (a32.is_inf()) inf = true;
    else { acc.x = f29::to29(a32.x.normalized()); acc.y = f29::to29(a32.y.normalized()); acc.zz = f29::to29(a32.zz.normalized()); acc.zzz = f29::to29(a32.zzz.normalized()); }
}
enum { FQ29_MUL, FQ29_MUL2, FQ29_SQR, FQ29_SQR2, FQ29_NORM, FQ29_ADD, FQ29_DBL, FQ29_SUB_S2_1, FQ29_SUB_S4_1, FQ29_SUB_S6_1, FQ29_SUB_S4_3, FQ29_NEG_S2_1, FQ29_IS_ZERO,
       FQ29_UNPACK, FQ29_TO29, FQ29_FROM29, FQ29_REC64, FQ29_BUCKET29, FQ29_INVERSE, FQ29_MADD, FQ29_ADD_LANE, FQ29_ADD_PAIR, FQ29_ADD_QUAD, FQ29_OPS };
static const int FQ29_K[FQ29_OPS] = {2, 4, 1, 2, 1, 2, 1, 2, 2, 2, 2, 1, 1, 1, 1, 1, 3, 5, 1, 7, 8, 8, 8};
static const int FQ29_M[FQ29_OPS] = {1, 2, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3, 4, 1, 5, 4, 4, 4};
ZK_D Fq29 fq29_load(const uint32_t *p) { Fq29 r; for (int l = 0; l < 9; ++l) r.v[l] = p[l]; return r; }
ZK_D void fq29_store(uint32_t *p, const Fq29 &a) { for (int l = 0; l < 9; ++l) p[l] = a.v[l]; }
// `records`: room for n Bucket29 (ops rec64 and bucket29 store their record there, Rec64 or Bucket29, and load it back)
__global__ __launch_bounds__(64) void k_fq29_op(int op, int k, int m, int chain, const uint32_t *in, size_t n, uint32_t *out, void *records) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    if (!live && op != FQ29_INVERSE) return;             // (the inversion's early exit is a wavefront vote: a tail lane inverts the integer 1 and writes nothing)
    Fq29 x[8], y[5];
    for (int j = 0; j < 8; ++j) for (int l = 0; l < 9; ++l) x[j].v[l] = live ? (j < k ? in[(i * k + j) * 9 + l] : 0u) : (l == 0 ? 1u : 0u);
    for (int j = 0; j < 5; ++j) y[j] = Fq29::zero();
    switch (op) {
    case FQ29_MUL: y[0] = f29::mul(x[0], x[1]); break;
    case FQ29_MUL2: f29::mul2(y[0], y[1], x[0], x[1], x[2], x[3]); break;
    case FQ29_SQR: y[0] = f29::sqr(x[0]); break;
    case FQ29_SQR2: f29::sqr2(y[0], y[1], x[0], x[1]); break;
    case FQ29_NORM: y[0] = f29::norm(x[0]); break;
    case FQ29_ADD: y[0] = f29::add(x[0], x[1]); break;
    case FQ29_DBL: y[0] = f29::dbl(x[0]); break;
    case FQ29_SUB_S2_1: y[0] = f29::sub(x[0], f29::S2_1, x[1]); break;
    case FQ29_SUB_S4_1: y[0] = f29::sub(x[0], f29::S4_1, x[1]); break;
    case FQ29_SUB_S6_1: y[0] = f29::sub(x[0], f29::S6_1, x[1]); break;
    case FQ29_SUB_S4_3: y[0] = f29::sub(x[0], f29::S4_3, x[1]); break;
    case FQ29_NEG_S2_1: y[0] = f29::neg(f29::S2_1, x[0]); break;
    case FQ29_IS_ZERO: y[0].v[0] = f29::is_zero_mod_p(x[0]) ? 1u : 0u; break;
    case FQ29_UNPACK: { Fq f; for (int l = 0; l < 8; ++l) f.v[l] = x[0].v[l]; y[0] = f29::unpack(f); break; }
    case FQ29_TO29: { Fq f; for (int l = 0; l < 8; ++l) f.v[l] = x[0].v[l]; y[0] = f29::to29(f); break; }
    case FQ29_FROM29: { const Fq f = f29::from29(x[0]); for (int l = 0; l < 8; ++l) y[0].v[l] = f.v[l]; break; }
    case FQ29_REC64: {
        Rec64 *rec = reinterpret_cast<Rec64 *>(records) + i;
        store_rec64(rec, x[0], x[1], (x[2].v[0] & 1u) != 0);
        const Affine29 a = load_rec64(rec);
        for (int l = 0; l < 9; ++l) { y[0].v[l] = a.x[l]; y[1].v[l] = a.y[l]; }
        y[2].v[0] = a.inf;
        break;
    }
    case FQ29_BUCKET29: {
        XYZZ29 a; a.x = x[0]; a.y = x[1]; a.zz = x[2]; a.zzz = x[3];
        Bucket29 *rec = reinterpret_cast<Bucket29 *>(records) + i;
        store_bucket29(rec, a, (x[4].v[0] & 1u) != 0);
        const Bucket29 b = load_bucket29_raw(rec);
        for (int l = 0; l < 9; ++l) { y[0].v[l] = b.x[l]; y[1].v[l] = b.y[l]; y[2].v[l] = b.zz[l]; y[3].v[l] = b.zzz[l]; }
        break;
    }
    case FQ29_INVERSE: y[0] = f29::inverse(x[0]); break;
    case FQ29_MADD: {                                     // 1 + chain times acc <- acc + b, each as k_bucket_accum29 does it
        XYZZ29 acc; acc.x = x[0]; acc.y = x[1]; acc.zz = x[2]; acc.zzz = x[3];
        bool inf = (x[6].v[0] & 1u) != 0, ok = true;
        for (int s = 0; s <= chain; ++s) {
            ok = acc.madd(x[4], x[5], inf);
            if (!ok) fq29_madd_fallback_copy(acc, x[4], x[5], inf);
        }
        if (!inf) { y[0] = acc.x; y[1] = acc.y; y[2] = acc.zz; y[3] = acc.zzz; }               // (infinity: all zero, as store_bucket29 writes it)
        y[4].v[0] = inf ? 1u : 0u; y[4].v[1] = ok ? 1u : 0u;
        break;
    }
    default: {                                            // FQ29_ADD_LANE: a + b, then `chain` rounds of x <- 2x + b
        XYZZ29q a, b; a.x = x[0]; a.y = x[1]; a.zz = x[2]; a.zzz = x[3]; b.x = x[4]; b.y = x[5]; b.zz = x[6]; b.zzz = x[7];
        xyzz29_add_lane(a, b);
        for (int s = 0; s < chain; ++s) { const XYZZ29q z = a; xyzz29_add_lane(a, b); xyzz29_add_lane(a, z); }
        y[0] = a.x; y[1] = a.y; y[2] = a.zz; y[3] = a.zzz;
        break;
    }
    }
    if (!live) return;
    for (int j = 0; j < m; ++j) for (int l = 0; l < 9; ++l) out[(i * m + j) * 9 + l] = y[j].v[l];
}
// the pair form: lane r of a pair loads (X, ZZ) or (Y, ZZZ) of both points, as k_add_pair29 does, and writes its own two coordinates of the
// sum — no exchange outside xyzz29_add_pair, inside which the whole pair is active (a pair leaves together: i is the pair's)
__global__ __launch_bounds__(64) void k_fq29_add_pair(int chain, const uint32_t *in, size_t n, uint32_t *out) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1; const uint32_t r = threadIdx.x & 1;
    if (i >= n) return;
    const uint32_t *p = in + i * 72; uint32_t *o = out + i * 36;
    Half29 a, b; a.c0 = fq29_load(p + 9 * r); a.c1 = fq29_load(p + 9 * (2 + r)); b.c0 = fq29_load(p + 9 * (4 + r)); b.c1 = fq29_load(p + 9 * (6 + r));
    xyzz29_add_pair(a, b, r);
    for (int s = 0; s < chain; ++s) { const Half29 z = a; xyzz29_add_pair(a, b, r); xyzz29_add_pair(a, z, r); }
    fq29_store(o + 9 * r, a.c0); fq29_store(o + 9 * (2 + r), a.c1);
}
// the quad form: every lane of a quad holds both points whole; lane q writes coordinate q of ITS copy of the sum (the four copies must agree)
__global__ __launch_bounds__(64) void k_fq29_add_quad(int chain, const uint32_t *in, size_t n, uint32_t *out) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2; const uint32_t q = threadIdx.x & 3;
    if (i >= n) return;
    const uint32_t *p = in + i * 72;
    XYZZ29q a, b; a.x = fq29_load(p); a.y = fq29_load(p + 9); a.zz = fq29_load(p + 18); a.zzz = fq29_load(p + 27);
    b.x = fq29_load(p + 36); b.y = fq29_load(p + 45); b.zz = fq29_load(p + 54); b.zzz = fq29_load(p + 63);
    xyzz29_add_quad(a, b, q);
    for (int s = 0; s < chain; ++s) { const XYZZ29q z = a; xyzz29_add_quad(a, b, q); xyzz29_add_quad(a, z, q); }
    fq29_store(out + i * 36 + 9 * q, quad_select29(q, a.x, a.y, a.zz, a.zzz));
}
static int fq29_op_run(int op, int chain, const uint32_t *in, size_t n, uint32_t *out) {
    DevBuf din, dout, drec;
    const int k = FQ29_K[op], m = FQ29_M[op];
    const size_t in_bytes = n * k * 9 * sizeof(uint32_t), out_bytes = n * m * 9 * sizeof(uint32_t);
    const bool records = op == FQ29_REC64 || op == FQ29_BUCKET29;
    int rc = ZKG_ERROR;
    if (!din.reserve(in_bytes) && !dout.reserve(out_bytes) && (!records || !drec.reserve(n * sizeof(Bucket29))) &&
        hip_ok(hipMemcpy(din.p, in, in_bytes, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__)) {
        if (op == FQ29_ADD_PAIR) hipLaunchKernelGGL(k_fq29_add_pair, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, nullptr, chain, din.as<uint32_t>(), n, dout.as<uint32_t>());
        else if (op == FQ29_ADD_QUAD) hipLaunchKernelGGL(k_fq29_add_quad, dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, nullptr, chain, din.as<uint32_t>(), n, dout.as<uint32_t>());
        else hipLaunchKernelGGL(k_fq29_op, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, op, k, m, chain, din.as<uint32_t>(), n, dout.as<uint32_t>(), records ? drec.p : (void *)nullptr);
        if (hipGetLastError() == hipSuccess && hip_ok(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__)) rc = ZKG_OK;
    }
    din.release(); dout.release(); drec.release();
    return rc;
}

static std::mutex g_init_mu;
static std::atomic<int> g_device{-1};                     // written under g_init_mu, read by entry points on any thread
int initialised_device() { return g_device.load(); }
// the pointer rule of the *_dev entries (zkg_groth16_prove_dev, zkg_msm_g1_resident_async): `what` must be device memory of `device` (pinned,
// managed and unregistered host memory are refused), aligned, and `bytes` long inside its allocation where the runtime knows the allocation
int dev_range_refused(const void *d, size_t bytes, size_t align, int device, const char *who, const char *what, const char *owner) {
    auto refuse = [&](const std::string &why) { set_error(std::string(who) + ": " + what + " " + why); return ZKG_ERROR; };
    if (reinterpret_cast<uintptr_t>(d) % align) return refuse("must be aligned to " + std::to_string(align) + " bytes");
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, d) != hipSuccess) { (void)hipGetLastError(); return refuse("is not device memory"); }
    if (at.type != hipMemoryTypeDevice || at.isManaged || at.device != device) return refuse(std::string("is not device memory of the ") + owner + "'s device");
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d) != hipSuccess) { (void)hipGetLastError(); return ZKG_OK; }
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base), at_d = reinterpret_cast<uintptr_t>(d);
    if (at_d < lo || at_d - lo > size || bytes > size - (at_d - lo)) return refuse("runs past the end of its allocation");
    return ZKG_OK;
}
// the rules the *_async entries share (zkg_msm_g1_resident_async, zkg_domain_*_async): the caller is on the handle's device (`made`: "the
// bases were uploaded on"), and `count` vectors of n elements lie `stride` elements apart
int wrong_device_refused(const char *who, int device, const char *made) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device) return ZKG_OK;
    (void)hipGetLastError();
    set_error(std::string(who) + ": the calling thread's device is not the one " + made);
    return ZKG_ERROR;
}
int async_vectors_refused(const char *who, size_t n, const char *n_name, size_t stride, size_t count, int device, const char *made) {
    if (stride < n) { set_error(std::string(who) + ": stride must be at least " + n_name); return ZKG_ERROR; }
    if (count > ZKG_MSM_ASYNC_MAX_COUNT || stride > ZKG_MSM_ASYNC_MAX_STRIDE) { set_error(std::string(who) + ": at most 2^24 vectors, at most 2^32 elements apart"); return ZKG_ERROR; }
    return wrong_device_refused(who, device, made);
}
// ---- the 32-bit device group law of curve.hip.hpp, element-wise (the known-answer hook behind zkg_curve_op): RAW records in, exactly as the
//      device structs lay them out and with no load_norm or normalized() before the operation, so a caller can place any representative
//      below 2p in any coordinate (ZZ != 1, infinity as ZZ = p, the affine infinity as x = y = p).  Results leave through normalized().
enum { CURVE_MADD, CURVE_ADD, CURVE_ADD_QUAD, CURVE_DBL, CURVE_DBL_AFFINE, CURVE_TO_AFFINE, CURVE_MUL, CURVE_OPS };
template <class F, int OP> __global__ __launch_bounds__(64) void k_curve_op(const void *a, const void *b, const uint32_t *k, size_t n, int chain, void *out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = OP == CURVE_ADD_QUAD ? t >> 2 : t;                       // the quad form: four lanes per element, identical copies
    if (i >= n) return;
    if constexpr (OP == CURVE_MADD) {
        XYZZ<F> x = ((const XYZZ<F> *)a)[i]; const Affine<F> y = ((const Affine<F> *)b)[i];
        x.madd(y);
        for (int c = 0; c < chain; ++c) { const XYZZ<F> z = x; x.add_inl(z); x.madd(y); }
        ((XYZZ<F> *)out)[i] = x.normalized();
    } else if constexpr (OP == CURVE_ADD) {
        XYZZ<F> x = ((const XYZZ<F> *)a)[i]; const XYZZ<F> y = ((const XYZZ<F> *)b)[i];
        x.add_inl(y);
        for (int c = 0; c < chain; ++c) { const XYZZ<F> z = x; x.add_inl(z); x.add_inl(y); }
        ((XYZZ<F> *)out)[i] = x.normalized();
    } else if constexpr (OP == CURVE_ADD_QUAD) {
        const uint32_t q = threadIdx.x & 3;
        XYZZ<F> x = ((const XYZZ<F> *)a)[i]; const XYZZ<F> y = ((const XYZZ<F> *)b)[i];
        xyzz_add_quad<F>(x, y, q);
        for (int c = 0; c < chain; ++c) { const XYZZ<F> z = x; xyzz_add_quad<F>(x, z, q); xyzz_add_quad<F>(x, y, q); }
        ((XYZZ<F> *)out)[4 * i + q] = x.normalized();                         // every lane's copy: the caller checks that the four agree
    } else if constexpr (OP == CURVE_DBL) {
        ((XYZZ<F> *)out)[i] = ((const XYZZ<F> *)a)[i].dbl_inl().normalized();
    } else if constexpr (OP == CURVE_DBL_AFFINE) {
        ((XYZZ<F> *)out)[i] = XYZZ<F>::dbl_affine_inl(((const Affine<F> *)a)[i]).normalized();
    } else if constexpr (OP == CURVE_TO_AFFINE) {
        ((Affine<F> *)out)[i] = ((const XYZZ<F> *)a)[i].to_affine().normalized();
    } else {
        uint32_t s[8];
        for (int j = 0; j < 8; ++j) s[j] = k[8 * i + j];
        ((XYZZ<F> *)out)[i] = ((const XYZZ<F> *)a)[i].mul(s, 8).normalized();
    }
}
template <class F, int OP> static int curve_op_run(const uint32_t *a, const uint32_t *b, const uint32_t *k, size_t n, int chain, uint32_t *out) {
    const size_t a_bytes = n * (OP == CURVE_DBL_AFFINE ? sizeof(Affine<F>) : sizeof(XYZZ<F>));
    const size_t b_bytes = OP == CURVE_MADD ? n * sizeof(Affine<F>) : OP == CURVE_ADD || OP == CURVE_ADD_QUAD ? n * sizeof(XYZZ<F>) : 0;
    const size_t k_bytes = OP == CURVE_MUL ? n * 8 * sizeof(uint32_t) : 0;
    const size_t out_bytes = OP == CURVE_TO_AFFINE ? n * sizeof(Affine<F>) : (OP == CURVE_ADD_QUAD ? 4 : 1) * n * sizeof(XYZZ<F>);
    const size_t lanes = OP == CURVE_ADD_QUAD ? 4 * n : n;
    ScopedDevBuf da, db, dk, dout;
    if (da.reserve(a_bytes) || dout.reserve(out_bytes) || (b_bytes && db.reserve(b_bytes)) || (k_bytes && dk.reserve(k_bytes))) return ZKG_ERROR;
    ZK_HIP(hipMemcpy(da.p, a, a_bytes, hipMemcpyHostToDevice));
    if (b_bytes) ZK_HIP(hipMemcpy(db.p, b, b_bytes, hipMemcpyHostToDevice));
    if (k_bytes) ZK_HIP(hipMemcpy(dk.p, k, k_bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_curve_op<F, OP>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, nullptr, (const void *)da.p, (const void *)db.p, dk.as<uint32_t>(), n, chain, dout.p);
    if (hipGetLastError() != hipSuccess) { set_error("zkg_curve_op: launch failed"); return ZKG_ERROR; }
    ZK_HIP(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
    return ZKG_OK;
}
template <class F> static int curve_op_group(int op, const uint32_t *a, const uint32_t *b, const uint32_t *k, size_t n, int chain, uint32_t *out) {
    switch (op) {
    case CURVE_MADD: return curve_op_run<F, CURVE_MADD>(a, b, k, n, chain, out);
    case CURVE_ADD: return curve_op_run<F, CURVE_ADD>(a, b, k, n, chain, out);
    case CURVE_ADD_QUAD: return curve_op_run<F, CURVE_ADD_QUAD>(a, b, k, n, chain, out);
    case CURVE_DBL: return curve_op_run<F, CURVE_DBL>(a, b, k, n, chain, out);
    case CURVE_DBL_AFFINE: return curve_op_run<F, CURVE_DBL_AFFINE>(a, b, k, n, chain, out);
    case CURVE_TO_AFFINE: return curve_op_run<F, CURVE_TO_AFFINE>(a, b, k, n, chain, out);
    default: return curve_op_run<F, CURVE_MUL>(a, b, k, n, chain, out);
    }
}
static void kernels_configure() { (void)ntt_configure(); (void)msm_configure(); }

}  // namespace zk

void seam_keygen_quiesce();          // setup_verify.hip

using namespace zk;

extern "C" {

int zkg_init(int device) {
    std::lock_guard<std::mutex> lk(g_init_mu);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { set_error("zkg_init: no HIP device visible (this library has no CPU fallback)"); return ZKG_ERROR; }
    if (device < 0 || device >= count) { set_error("zkg_init: bad device index"); return ZKG_ERROR; }
    ZK_HIP(hipSetDevice(device));
    g_device = device;
    kernels_configure();
    return ZKG_OK;
}
void zkg_shutdown(void) {
    seam_keygen_quiesce();
    std::lock_guard<std::mutex> lk(g_init_mu);
    if (g_device < 0) return;
    (void)hipDeviceSynchronize();
    ntt_release_all();
    msm_release_all();
    verify_keys_release_all();
    verify_release_all();
    zklaim_witness_release_all();
    g_device = -1;
}
const char *zkg_last_error(void) { std::lock_guard<std::mutex> lk(g_err_mu); static std::string copy; copy = g_error; return copy.c_str(); }

int zkg_device_info(char *name, size_t name_len, int *compute_units) {
    if (g_device < 0) { set_error("zkg_init not called"); return ZKG_ERROR; }
    hipDeviceProp_t prop;
    ZK_HIP(hipGetDeviceProperties(&prop, g_device));
    if (name && name_len) { strncpy(name, prop.gcnArchName, name_len - 1); name[name_len - 1] = 0; }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    return ZKG_OK;
}

#define REQUIRE_INIT() do { if (g_device < 0) { set_error("zkg_init not called"); return ZKG_ERROR; } } while (0)

int zkg_ntt_dev(void *d_a, unsigned logN, int inverse, int coset, void *stream) {
    REQUIRE_INIT();
    if (logN > 28) { set_error("zkg_ntt: logN exceeds the 2-adicity (28) of Fr"); return ZKG_ERROR; }
    hipStream_t s = (hipStream_t)stream;
    NttDomain *d = ntt_domain(logN, s);
    if (!d) return ZKG_ERROR;
    return ntt_run(d, (Fr *)d_a, inverse, coset, s);
}
// The host-pointer transforms run on the null stream with the domain's shared inter-pass scratch: callers on several threads take turns
// (device-pointer callers pass their own stream and get a scratch vector per stream, NttDomain::scratch_for).
static std::mutex g_host_ntt_mu;
int zkg_ntt(uint64_t *a, unsigned logN, int inverse, int coset) {
    REQUIRE_INIT();
    if (!a || logN > 28) { set_error("zkg_ntt: bad argument"); return ZKG_ERROR; }
    std::lock_guard<std::mutex> lk(g_host_ntt_mu);
    size_t bytes = ((size_t)1 << logN) * 32;
    DevBuf buf;
    if (buf.reserve(bytes)) return ZKG_ERROR;
    int rc = ZKG_ERROR;
    if (hip_ok(hipMemcpy(buf.p, a, bytes, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__) &&
        zkg_ntt_dev(buf.p, logN, inverse, coset, nullptr) == ZKG_OK &&
        hip_ok(hipDeviceSynchronize(), "sync", __FILE__, __LINE__) &&
        hip_ok(hipMemcpy(a, buf.p, bytes, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__)) rc = ZKG_OK;
    buf.release();
    return rc;
}

int zkg_evaluation_domain_size(size_t min_size, size_t *m, int *is_step) {
    DomainShape sh;
    if (!evaluation_domain_shape(min_size, sh)) { set_error("zkg_evaluation_domain_size: no radix-2 or step domain for that size"); return ZKG_ERROR; }
    if (m) *m = sh.m;
    if (is_step) *is_step = sh.step ? 1 : 0;
    return ZKG_OK;
}
int zkg_ntt_domain_dev(void *d_a, size_t m, int inverse, int coset, void *stream) {
    REQUIRE_INIT();
    DomainShape sh;
    if (!domain_shape_of(m, sh)) { set_error("zkg_ntt_domain: m is neither 2^k nor 2^a + 2^b (get_evaluation_domain would not return it)"); return ZKG_ERROR; }
    if (!sh.step) return zkg_ntt_dev(d_a, sh.log_m, inverse, coset, stream);
    hipStream_t s = (hipStream_t)stream;
    StepDomain *d = step_domain(m, s);
    if (!d) return ZKG_ERROR;
    DevBuf scratch;                                           // one-off call: the prover keeps its own
    if (scratch.reserve(m * NTT_SCRATCH_BYTES)) return ZKG_ERROR;
    int rc = step_ntt_run(d, (Fr *)d_a, inverse != 0, coset != 0, s, scratch.as<Fr>());
    if (!hip_ok(hipStreamSynchronize(s), "sync", __FILE__, __LINE__)) rc = ZKG_ERROR;
    scratch.release();
    return rc;
}
int zkg_ntt_domain(uint64_t *a, size_t m, int inverse, int coset) {
    REQUIRE_INIT();
    if (!a || m < 2) { set_error("zkg_ntt_domain: bad argument"); return ZKG_ERROR; }
    std::lock_guard<std::mutex> lk(g_host_ntt_mu);
    size_t bytes = m * 32;
    DevBuf buf;
    if (buf.reserve(bytes)) return ZKG_ERROR;
    int rc = ZKG_ERROR;
    if (hip_ok(hipMemcpy(buf.p, a, bytes, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__) &&
        zkg_ntt_domain_dev(buf.p, m, inverse, coset, nullptr) == ZKG_OK &&
        hip_ok(hipDeviceSynchronize(), "sync", __FILE__, __LINE__) &&
        hip_ok(hipMemcpy(a, buf.p, bytes, hipMemcpyDeviceToHost), "D2H", __FILE__, __LINE__)) rc = ZKG_OK;
    buf.release();
    return rc;
}

// ---- zkg_domain: one evaluation domain as a handle — batched transforms and the Lagrange coefficients, queued on the caller's stream with no
//      wait on the host (include/zkg.h).  The twiddle and coset tables are the shared ones of ntt_domain / step_domain; the handle owns the
//      inter-pass scratch of its batches (packed: m records per vector of a group, however far apart the vectors lie) and one event.
static constexpr size_t DOMAIN_WORKSPACE_CAP = (size_t)1 << 30;          // the scratch of one launch group stays below this (one vector is always taken)
static constexpr size_t DOMAIN_MAX_GROUP = 65535;                        // grid.y
struct zkg_domain {
    DomainShape sh; int device = 0; std::mutex mu;
    DevBuf scratch;
    HandleOrder order;                                                  // its calls run in call order whatever streams they name (common.hpp)
    size_t bmax_default = 1, bmax = 1;
};
static thread_local size_t t_domain_stats[3];
static zkg_domain *domain_new_impl(size_t m) {
    if (g_device < 0) { set_error("zkg_init not called"); return nullptr; }
    DomainShape sh;
    if (m < 2 || !domain_shape_of(m, sh)) { set_error("zkg_domain_new: m is neither 2^k (k <= 28) nor 2^a + 2^b (get_evaluation_domain would not return it)"); return nullptr; }
    if (wrong_device_refused("zkg_domain_new", g_device, "zkg_init selected (the domain tables live there)")) return nullptr;
    std::unique_ptr<zkg_domain> d(new zkg_domain());
    d->sh = sh; d->device = g_device;
    d->bmax_default = d->bmax = std::max<size_t>(1, std::min(DOMAIN_MAX_GROUP, DOMAIN_WORKSPACE_CAP / (m * NTT_SCRATCH_BYTES)));
    // the tables are built here, on the null stream, and waited for: no later call finds them missing or half made
    const bool tables = sh.step ? step_domain(m, nullptr) != nullptr : ntt_domain(sh.log_m, nullptr) != nullptr;
    if (!tables || !hip_ok(hipStreamSynchronize(nullptr), "hipStreamSynchronize", __FILE__, __LINE__) || d->order.create()) return nullptr;
    return d.release();
}
static int domain_ntt_async_impl(zkg_domain *d, void *d_a, size_t stride, size_t count, int inverse, int coset, void *stream) {
    static const char *who = "zkg_domain_ntt_async";
    for (size_t &v : t_domain_stats) v = 0;
    if (count == 0) return ZKG_OK;                                      // nothing to do, nothing touched
    REQUIRE_INIT();
    if (!d || !d_a) { set_error(std::string(who) + ": bad argument (null handle or pointer)"); return ZKG_ERROR; }
    const size_t m = d->sh.m;
    if (async_vectors_refused(who, m, "m", stride, count, d->device, "the handle was made on") ||
        dev_range_refused(d_a, ((count - 1) * stride + m) * 32, 16, d->device, who, "d_a", "handle")) return ZKG_ERROR;
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(d->mu);                              // held for the enqueue only
    NttDomain *nd = nullptr; StepDomain *sd = nullptr;                  // looked up per call (a map find): zkg_shutdown releases them under a live handle
    if (d->sh.step) sd = step_domain(m, s); else nd = ntt_domain(d->sh.log_m, s);
    if (!nd && !sd) return ZKG_ERROR;
    size_t waits = 0, groups = 0, done = 0;
    // the scratch of the call's largest group.  Growing it frees it: earlier calls may still be in it, so the handle's event is waited for first
    const size_t need = std::min(d->bmax, count) * m * NTT_SCRATCH_BYTES;
    if (d->order.grow(d->scratch, need, waits) || d->order.order_behind(s)) return ZKG_ERROR;
    Fr *a = (Fr *)d_a;
    int rc = ZKG_OK;
    while (done < count && rc == ZKG_OK) {
        const size_t g = std::min(d->bmax, count - done);
        Fr *ag = a + done * stride;
        const hipEvent_t ev = done + g == count ? d->order.ev : nullptr;     // the call's last group ends in the handle's event
        rc = sd ? step_ntt_run(sd, ag, inverse != 0, coset != 0, s, d->scratch.as<Fr>(), (unsigned)g, stride, m, ev)
                : ntt_run(nd, ag, inverse, coset, s, d->scratch.as<Fr>(), (unsigned)g, stride, m, ev);
        if (rc == ZKG_OK) { done += g; ++groups; }
    }
    t_domain_stats[0] = done; t_domain_stats[1] = groups; t_domain_stats[2] = waits;
    if (rc == ZKG_OK) { d->order.carried(s); return ZKG_OK; }
    d->order.record(s);                                                 // a failure: the groups enqueued before it still run
    return ZKG_ERROR;
}
static int domain_lagrange_async_impl(zkg_domain *d, const uint64_t t[4], void *d_u, void *d_z, void *stream) {
    static const char *who = "zkg_domain_lagrange_async";
    REQUIRE_INIT();
    if (!d || !t || !d_u) { set_error(std::string(who) + ": bad argument (null handle or pointer)"); return ZKG_ERROR; }
    if (wrong_device_refused(who, d->device, "the handle was made on") || dev_range_refused(d_u, d->sh.m * 32, 16, d->device, who, "d_u", "handle") ||
        (d_z && dev_range_refused(d_z, 32, 16, d->device, who, "d_z", "handle"))) return ZKG_ERROR;
    Fr tf; memcpy(tf.v, t, 32);                                         // read now: the caller may reuse t on return
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(d->mu);
    if (d->order.order_behind(s) || domain_lagrange_dev(d->sh, tf, (Fr *)d_u, (Fr *)d_z, s, d->order.ev)) return ZKG_ERROR;
    d->order.carried(s);
    return ZKG_OK;
}
zkg_domain *zkg_domain_new(size_t m) { return c_boundary<zkg_domain *>("zkg_domain_new", nullptr, [&] { return domain_new_impl(m); }); }
void zkg_domain_free(zkg_domain *d) {
    if (!d) return;
    c_boundary("zkg_domain_free", 0, [&] {
        int cur = 0; (void)hipGetDevice(&cur);
        if (cur != d->device) (void)hipSetDevice(d->device);           // the scratch and the event live on the handle's device
        d->order.destroy();
        d->scratch.release();
        if (cur != d->device) (void)hipSetDevice(cur);
        delete d;
        return 0;
    });
}
size_t zkg_domain_size(const zkg_domain *d) { return d ? d->sh.m : 0; }
size_t zkg_domain_batch_max(const zkg_domain *d) { return d ? d->bmax : 0; }
void zkg_domain_set_batch_max(zkg_domain *d, size_t k) {
    if (!d) return;
    c_boundary("zkg_domain_set_batch_max", 0, [&] { std::lock_guard<std::mutex> lk(d->mu); d->bmax = clamp_batch_max(k, d->bmax_default); return 0; });
}
int zkg_domain_ntt_async(zkg_domain *d, void *d_a, size_t stride, size_t count, int inverse, int coset, void *stream) {
    return c_boundary("zkg_domain_ntt_async", ZKG_ERROR, [&] { return domain_ntt_async_impl(d, d_a, stride, count, inverse, coset, stream); });
}
int zkg_domain_lagrange_async(zkg_domain *d, const uint64_t t[4], void *d_u, void *d_z, void *stream) {
    return c_boundary("zkg_domain_lagrange_async", ZKG_ERROR, [&] { return domain_lagrange_async_impl(d, t, d_u, d_z, stream); });
}
void zkg_domain_stats(size_t out[3]) { if (out) for (int i = 0; i < 3; ++i) out[i] = t_domain_stats[i]; }

int zkg_msm_g1_dev(const void *d_bases, const void *d_scalars, size_t n, int scalars_mont, uint64_t out_jac[12], void *stream) {
    REQUIRE_INIT();
    G1 r;
    if (msm_g1((const G1Affine *)d_bases, (const uint32_t *)d_scalars, n, (scalars_mont & ZKG_SCALARS_MONT) != 0, &r, (hipStream_t)stream, (scalars_mont & ZKG_SCALARS_MOSTLY_BITS) != 0)) return ZKG_ERROR;
    store_norm(out_jac, r);
    return ZKG_OK;
}
int zkg_msm_g1_host_scalars(const void *d_bases, const uint64_t *scalars, size_t n, int scalars_mont, uint64_t out_jac[12], void *stream) {
    REQUIRE_INIT();
    if (!out_jac || (n && (!d_bases || !scalars))) { set_error("zkg_msm_g1_host_scalars: bad argument"); return ZKG_ERROR; }
    G1 r;
    if (msm_g1_host_scalars((const G1Affine *)d_bases, (const uint32_t *)scalars, n, (scalars_mont & ZKG_SCALARS_MONT) != 0, &r, (hipStream_t)stream)) return ZKG_ERROR;
    store_norm(out_jac, r);
    return ZKG_OK;
}
int zkg_msm_host_scalars_stats(uint32_t *out, int n) { return out && n >= 0 ? msm_host_scalars_stats(out, n) : 0; }
int zkg_msm_g1_windows_dev(const void *d_bases, const void *d_scalars, size_t n, int scalars_mont, unsigned first_window, unsigned window_stride,
                           uint64_t out_jac[12], void *stream) {
    REQUIRE_INIT();
    if (!window_stride) { set_error("zkg_msm_g1_windows_dev: window_stride must be positive"); return ZKG_ERROR; }
    G1 r; const G1Affine *b = (const G1Affine *)d_bases;
    if (msm_shared(&b, 1, nullptr, (const uint32_t *)d_scalars, n, (scalars_mont & ZKG_SCALARS_MONT) != 0, &r, nullptr, (hipStream_t)stream, first_window, window_stride,
                   (scalars_mont & ZKG_SCALARS_MOSTLY_BITS) != 0)) return ZKG_ERROR;
    store_norm(out_jac, r);
    return ZKG_OK;
}
// ---- fixed bases kept resident with their per-window tables (what the prover's H query gets; a Groth16 B query for G2): include/zkg.h.
//      One implementation for both groups.  A handle owns its table, one job on a stream of its own, and the two events that tie that stream
//      to the caller's.  The groups differ in what MsmResidentG1 / MsmResidentG2 say and in two places marked below: G1 also builds the 29-bit
//      records and merges rows, G2 caps a group by its bucket workspace.
struct MsmResident { WindowTable table; MsmJob *job = nullptr; std::mutex mu; int device = 0; hipEvent_t ev_in = nullptr, ev_out = nullptr; };
struct zkg_msm_bases : MsmResident {};
struct zkg_msm_g2_bases : MsmResident {};
struct MsmResidentG1 { using Handle = zkg_msm_bases; using Point = G1; static constexpr bool g2 = false; static constexpr size_t limbs = 12; static constexpr unsigned n_log = 27; static constexpr const char *prefix = "zkg_msm_g1"; };
struct MsmResidentG2 { using Handle = zkg_msm_g2_bases; using Point = G2; static constexpr bool g2 = true; static constexpr size_t limbs = 24; static constexpr unsigned n_log = 25; static constexpr const char *prefix = "zkg_msm_g2"; };
static constexpr size_t G2_RESIDENT_BUCKET_CAP = (size_t)1 << 30;       // one group's bucket workspace (zkg_msm_g2_resident_batch_max)

extern "C++" {                                                          // (templates: this file's entries sit in one extern "C" block)
static void resident_free(MsmResident *h) {
    int cur = 0; (void)hipGetDevice(&cur);
    if (cur != h->device) (void)hipSetDevice(h->device);               // the handle's memory, stream and events live on the device it was made on
    if (h->job) { (void)hipStreamSynchronize(msm_job_stream(h->job)); msm_job_destroy(h->job); }
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_out) (void)hipEventDestroy(h->ev_out);
    h->table.release();
    if (cur != h->device) (void)hipSetDevice(cur);
}
template <class G> static typename G::Handle *resident_upload(const void *d_bases, size_t n) {
    const std::string who = std::string(G::prefix) + "_bases_upload";
    if (g_device < 0) { set_error("zkg_init not called"); return nullptr; }
    if (!d_bases || n == 0 || n >= ((size_t)1 << G::n_log)) { set_error(who + ": bad argument (1 <= n < 2^" + std::to_string(G::n_log) + ")"); return nullptr; }
    typename G::Handle *h = new (std::nothrow) typename G::Handle();
    if (!h) { set_error(who + ": out of memory"); return nullptr; }
    (void)hipGetDevice(&h->device);
    h->job = msm_job_create(nullptr, true);
    bool ok = h->job != nullptr && hip_ok(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming), "hipEventCreate", __FILE__, __LINE__) &&
              hip_ok(hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming), "hipEventCreate", __FILE__, __LINE__);
    if constexpr (G::g2) ok = ok && window_table_build_g2(h->table, (const G2Affine *)d_bases, n, table_window_bits(n), nullptr) == 0;
    else ok = ok && window_table_build_g1(h->table, (const G1Affine *)d_bases, n, table_window_bits(n), nullptr) == 0 && window_table_records29(h->table, nullptr) == 0;
    if (!ok || !hip_ok(hipDeviceSynchronize(), "sync", __FILE__, __LINE__)) { resident_free(h); delete h; return nullptr; }   // (the failing step has set the message)
    msm_job_set_window(h->job, h->table.c);
    if constexpr (!G::g2) msm_job_set_row_merge(h->job, n >= 49152 ? 2u : 1u);  // (G2 rows are not merged: the job's default, 1)
    return h;
}
// the handle's table as a launch's one base set (rec29 is null where no 29-bit records were built: G2)
static MsmBases resident_table_set(const MsmResident *h) { MsmBases b; b.p = h->table.buf.p; b.g2 = h->table.g2; b.level_stride = h->table.n; b.p29 = h->table.rec29.p; return b; }
template <class G> static int resident_sync(MsmResident *h, const void *d_scalars, size_t n, int scalars_mont, uint64_t *out_jac, void *stream) {
    const std::string who = std::string(G::prefix) + "_resident";
    REQUIRE_INIT();
    if (!h || !d_scalars || !out_jac || n != h->table.n) { set_error(who + ": bad argument (n must be the handle's point count)"); return ZKG_ERROR; }
    if (wrong_device_refused(who.c_str(), h->device, "the bases were uploaded on")) return ZKG_ERROR;
    std::lock_guard<std::mutex> lk(h->mu);                              // the handle owns one job: calls take turns
    // the job runs on the handle's own (non-blocking) stream: order it behind whatever the caller queued on `stream` (the work that
    // produces d_scalars).  The call returns after the result has landed, so nothing of it is left running for the caller to order after.
    ZK_HIP(hipEventRecord(h->ev_in, (hipStream_t)stream));
    ZK_HIP(hipStreamWaitEvent(msm_job_stream(h->job), h->ev_in, 0));
    const MsmBases b = resident_table_set(h);
    typename G::Point r;
    msm_job_set_device_finish(h->job, false);
    int rc;
    {   // asynchronous calls may still be running on the handle's stream: a buffer this launch has to grow is freed only after they have drained
        ReserveGuard guard(msm_job_stream(h->job));
        rc = msm_job_launch(h->job, &b, 1, (const uint32_t *)d_scalars, n, (scalars_mont & ZKG_SCALARS_MONT) != 0, nullptr);
    }
    if constexpr (G::g2) rc = rc || msm_job_finish(h->job, nullptr, &r); else rc = rc || msm_job_finish(h->job, &r, nullptr);
    if (rc) return ZKG_ERROR;
    store_norm(out_jac, r);
    return ZKG_OK;
}
// ---- zkg_msm_g1_resident_async, zkg_msm_g2_resident_async: the same multi-exponentiation for `count` scalar vectors, the points left in
//      DEVICE memory, no host wait.
static thread_local size_t t_resident_async_stats[3];
// Vectors per launch: what msm_multi_supported allows (the sort's 32-bit index space and its 2^22-bucket scan), and never more than
// MSM_MULTI_MAX_VECTORS, the largest batch the prover runs through msm_job_launch_multi — the workspace grows linearly with the group (at 2^12-bit
// windows of 5000 points 128 vectors would ask for 0.6 GB of buckets for a 0.6 MB scalar batch) and nothing above that size is exercised.
// G2, whose buckets are twice the size, also keeps one group's bucket workspace below G2_RESIDENT_BUCKET_CAP.
template <class G> static size_t resident_batch_max(const MsmResident *h) {
    size_t p = MSM_MULTI_MAX_VECTORS;
    if constexpr (G::g2) p = std::min<size_t>(p, std::max<size_t>(1, G2_RESIDENT_BUCKET_CAP / msm_table_bucket_bytes(h->table.c, true)));
    while (p > 1 && !msm_multi_supported(h->table.n, h->table.c, (uint32_t)p)) --p;
    return p;
}
template <class G> static int resident_async(MsmResident *h, const void *d_scalars, size_t n, size_t stride, size_t count, int scalars_mont, void *d_out_jac, void *stream) {
    const std::string who_s = std::string(G::prefix) + "_resident_async"; const char *who = who_s.c_str();
    for (size_t &v : t_resident_async_stats) v = 0;
    if (count == 0) return ZKG_OK;                                      // nothing to do, nothing touched
    REQUIRE_INIT();
    if (!h || !d_scalars || !d_out_jac || n != h->table.n) { set_error(who_s + ": bad argument (n must be the handle's point count)"); return ZKG_ERROR; }
    if (async_vectors_refused(who, n, "n", stride, count, h->device, "the bases were uploaded on")) return ZKG_ERROR;
    if (dev_range_refused(d_scalars, ((count - 1) * stride + n) * 32, 16, h->device, who, "d_scalars", "handle") ||
        dev_range_refused(d_out_jac, count * G::limbs * 8, 8, h->device, who, "d_out_jac", "handle")) return ZKG_ERROR;
    const size_t bmax = resident_batch_max<G>(h);
    const bool mont = (scalars_mont & ZKG_SCALARS_MONT) != 0;
    const uint32_t *sc = (const uint32_t *)d_scalars; uint64_t *out = (uint64_t *)d_out_jac;
    std::lock_guard<std::mutex> lk(h->mu);                              // held for the enqueue only: calls on one handle run in call order on its stream
    hipStream_t js = msm_job_stream(h->job);
    ZK_HIP(hipEventRecord(h->ev_in, (hipStream_t)stream));              // behind the work that writes d_scalars (nothing is enqueued yet)
    ZK_HIP(hipStreamWaitEvent(js, h->ev_in, 0));
    const MsmBases b = resident_table_set(h);
    msm_job_set_device_finish(h->job, true);
    int rc = ZKG_OK;
    size_t groups = 0, waits = 0, done = 0;
    while (done < count && rc == ZKG_OK) {
        const size_t g = std::min(bmax, count - done);
        // The job's buffers only grow, but which of them a group needs more of does not follow from its size alone (the reduction's chunk records
        // shrink as the group grows): every reserve that has to grow drains the handle's stream before it frees the buffer — earlier groups and
        // earlier calls may still read it — and is counted.  A launch whose buffers all suffice allocates nothing and waits for nothing.
        ReserveGuard guard(js);
        const uint32_t *sg = sc + done * stride * 8;
        rc = g > 1 ? msm_job_launch_multi(h->job, &b, 1, sg, n, stride * 8, (uint32_t)g, mont) : msm_job_launch(h->job, &b, 1, sg, n, mont, nullptr);
        if (rc == ZKG_OK) rc = msm_job_finish_dev(h->job, out + done * G::limbs);
        waits += guard.drains;
        if (rc == ZKG_OK) { done += g; ++groups; }
    }
    // whatever the caller queues on `stream` after this call sees the points — after a failure too: the groups enqueued before it still write theirs
    const bool ordered = hip_ok(hipEventRecord(h->ev_out, js), "hipEventRecord", __FILE__, __LINE__) &&
                         hip_ok(hipStreamWaitEvent((hipStream_t)stream, h->ev_out, 0), "hipStreamWaitEvent", __FILE__, __LINE__);
    t_resident_async_stats[0] = done; t_resident_async_stats[1] = groups; t_resident_async_stats[2] = waits;
    return rc == ZKG_OK && ordered ? ZKG_OK : ZKG_ERROR;
}
}  // extern "C++"
void zkg_msm_resident_async_stats(size_t out[3]) { if (out) for (int i = 0; i < 3; ++i) out[i] = t_resident_async_stats[i]; }
// the twelve entries: five per group and the two hooks that run the device epilogue (k_msm_combine, msm.hip) alone
#define ZKG_RESIDENT_ENTRIES(NAME, G)                                                                                                                       \
    G::Handle *NAME##_bases_upload(const void *d_bases, size_t n) {                                                                                         \
        return c_boundary<G::Handle *>(#NAME "_bases_upload", nullptr, [&] { return resident_upload<G>(d_bases, n); });                                    \
    }                                                                                                                                                       \
    void NAME##_bases_free(G::Handle *h) {                                                                                                                  \
        if (h) c_boundary(#NAME "_bases_free", 0, [&] { resident_free(h); delete h; return 0; });                                                           \
    }                                                                                                                                                       \
    int NAME##_resident(G::Handle *h, const void *d_scalars, size_t n, int scalars_mont, uint64_t *out_jac, void *stream) {                                \
        return c_boundary(#NAME "_resident", ZKG_ERROR, [&] { return resident_sync<G>(h, d_scalars, n, scalars_mont, out_jac, stream); });                  \
    }                                                                                                                                                       \
    int NAME##_resident_async(G::Handle *h, const void *d_scalars, size_t n, size_t stride, size_t count, int scalars_mont, void *d_out_jac, void *stream) { \
        return c_boundary(#NAME "_resident_async", ZKG_ERROR, [&] { return resident_async<G>(h, d_scalars, n, stride, count, scalars_mont, d_out_jac, stream); }); \
    }                                                                                                                                                       \
    size_t NAME##_resident_batch_max(const G::Handle *h) {                                                                                                  \
        return h ? c_boundary<size_t>(#NAME "_resident_batch_max", 0, [&] { return resident_batch_max<G>(h); }) : 0;                                        \
    }
ZKG_RESIDENT_ENTRIES(zkg_msm_g1, MsmResidentG1)
ZKG_RESIDENT_ENTRIES(zkg_msm_g2, MsmResidentG2)
#undef ZKG_RESIDENT_ENTRIES
int zkg_msm_combine_gpu(const uint64_t *records_jac, size_t cpw, int slots, int chunk_log, size_t vectors, uint64_t *out_jac) {
    return c_boundary("zkg_msm_combine_gpu", ZKG_ERROR, [&]() -> int { REQUIRE_INIT(); return msm_combine_records(false, records_jac, cpw, slots, chunk_log, vectors, out_jac); });
}
int zkg_msm_combine_g2_gpu(const uint64_t *records_jac, size_t cpw, int chunk_log, size_t vectors, uint64_t *out_jac) {
    return c_boundary("zkg_msm_combine_g2_gpu", ZKG_ERROR, [&]() -> int { REQUIRE_INIT(); return msm_combine_records(true, records_jac, cpw, 2, chunk_log, vectors, out_jac); });
}
int zkg_msm_g2_dev(const void *d_bases, const void *d_scalars, size_t n, int scalars_mont, uint64_t out_jac[24], void *stream) {
    REQUIRE_INIT();
    G2 r;
    if (msm_g2((const G2Affine *)d_bases, (const uint32_t *)d_scalars, n, (scalars_mont & ZKG_SCALARS_MONT) != 0, &r, (hipStream_t)stream, (scalars_mont & ZKG_SCALARS_MOSTLY_BITS) != 0)) return ZKG_ERROR;
    store_norm(out_jac, r);
    return ZKG_OK;
}
static int msm_host(const uint64_t *bases, const uint64_t *scalars, size_t n, uint64_t *out, int g2) {
    REQUIRE_INIT();
    if (n && (!bases || !scalars)) { set_error("zkg_msm: null input"); return ZKG_ERROR; }
    size_t bb = n * (g2 ? 128 : 64), sb = n * 32;
    DevBuf db, ds;
    if (db.reserve(bb + 16) || ds.reserve(sb + 16)) return ZKG_ERROR;
    int rc = ZKG_ERROR;
    if ((!n || (hip_ok(hipMemcpy(db.p, bases, bb, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__) &&
                hip_ok(hipMemcpy(ds.p, scalars, sb, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__))))
        rc = g2 ? zkg_msm_g2_dev(db.p, ds.p, n, 0, out, nullptr) : zkg_msm_g1_dev(db.p, ds.p, n, 0, out, nullptr);
    db.release(); ds.release();
    return rc;
}
int zkg_msm_g1(const uint64_t *bases, const uint64_t *scalars, size_t n, uint64_t out_jac[12]) { return msm_host(bases, scalars, n, out_jac, 0); }
int zkg_msm_g2(const uint64_t *bases, const uint64_t *scalars, size_t n, uint64_t out_jac[24]) { return msm_host(bases, scalars, n, out_jac, 1); }

int zkg_g1_sum(const uint64_t *points_jac, size_t count, uint64_t out_jac[12]) {
    G1 acc = G1::inf();
    for (size_t i = 0; i < count; ++i) acc.add(load_norm_g1(points_jac + 12 * i));
    store_norm(out_jac, acc);
    return ZKG_OK;
}
// out[i] = a[i] + b[i] (then `chain` rounds of x <- 2x + b) on the GPU through the 29-bit quad addition; normalised Jacobian in and out
int zkg_g1_add_quad29(const uint64_t *a_jac, const uint64_t *b_jac, size_t n, int chain, uint64_t *out_jac) {
    REQUIRE_INIT();
    if (!a_jac || !b_jac || !out_jac || chain < -1 || chain > 64) { set_error("zkg_g1_add_quad29: bad argument"); return ZKG_ERROR; }
    if (!n) return ZKG_OK;
    std::vector<G1> ha(n), hb(n), ho(n);
    for (size_t i = 0; i < n; ++i) { ha[i] = load_norm_g1(a_jac + 12 * i).normalized(); hb[i] = load_norm_g1(b_jac + 12 * i).normalized(); }
    ScopedDevBuf da, db, dout;
    if (da.reserve(n * sizeof(G1)) || db.reserve(n * sizeof(G1)) || dout.reserve(n * sizeof(G1))) return ZKG_ERROR;
    ZK_HIP(hipMemcpy(da.p, ha.data(), n * sizeof(G1), hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(db.p, hb.data(), n * sizeof(G1), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_add_quad29, dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, nullptr, da.as<G1>(), db.as<G1>(), n, chain, dout.as<G1>());
    if (hipGetLastError() != hipSuccess) { set_error("zkg_g1_add_quad29: launch failed"); return ZKG_ERROR; }
    ZK_HIP(hipMemcpy(ho.data(), dout.p, n * sizeof(G1), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) store_norm(out_jac + 12 * i, ho[i]);
    return ZKG_OK;
}
// the same hook for the pair form (fq29.hip.hpp xyzz29_add_pair): one pair of lanes per point pair, lane 0 holding (X, ZZ), lane 1 (Y, ZZZ)
__global__ __launch_bounds__(64) void k_add_pair29(const XYZZ<Fq> *a, const XYZZ<Fq> *b, size_t n, int chain, XYZZ<Fq> *out) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1; const uint32_t r = threadIdx.x & 1;
    if (i >= n) return;
    auto half = [&](const XYZZ<Fq> &p) {
        Half29 h = Half29::inf();
        if (!p.is_inf()) { h.c0 = f29::to29(r ? p.y : p.x); h.c1 = f29::to29(r ? p.zzz : p.zz); }
        return h;
    };
    Half29 x = half(a[i]); const Half29 y = half(b[i]);
    xyzz29_add_pair(x, y, r);
    for (int k = 0; k < chain; ++k) { const Half29 z = x; xyzz29_add_pair(x, y, r); xyzz29_add_pair(x, z, r); }
    // both halves through a scratch record in LDS, then lane 0 converts and writes
    __shared__ uint32_t rec[32][36];
    uint32_t *w = rec[threadIdx.x >> 1] + 9 * r;
    for (int j = 0; j < 9; ++j) { w[j] = x.c0.v[j]; w[18 + j] = x.c1.v[j]; }
    __syncthreads();
    if (r == 0) {
        Fq29 c[4]; const uint32_t *q = rec[threadIdx.x >> 1]; uint32_t any = 0;
        for (int k = 0; k < 4; ++k) for (int j = 0; j < 9; ++j) c[k].v[j] = q[9 * k + j];
        for (int j = 0; j < 9; ++j) any |= c[2].v[j];
        out[i] = any ? XYZZ<Fq>{f29::from29(c[0]), f29::from29(c[1]), f29::from29(c[2]), f29::from29(c[3])} : XYZZ<Fq>::inf().normalized();
    }
}
int zkg_g1_add_pair29(const uint64_t *a_jac, const uint64_t *b_jac, size_t n, int chain, uint64_t *out_jac) {
    REQUIRE_INIT();
    if (!a_jac || !b_jac || !out_jac || chain < 0 || chain > 64) { set_error("zkg_g1_add_pair29: bad argument"); return ZKG_ERROR; }
    if (!n) return ZKG_OK;
    std::vector<G1> ha(n), hb(n), ho(n);
    for (size_t i = 0; i < n; ++i) { ha[i] = load_norm_g1(a_jac + 12 * i).normalized(); hb[i] = load_norm_g1(b_jac + 12 * i).normalized(); }
    ScopedDevBuf da, db, dout;
    if (da.reserve(n * sizeof(G1)) || db.reserve(n * sizeof(G1)) || dout.reserve(n * sizeof(G1))) return ZKG_ERROR;
    ZK_HIP(hipMemcpy(da.p, ha.data(), n * sizeof(G1), hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(db.p, hb.data(), n * sizeof(G1), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_add_pair29, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, nullptr, da.as<G1>(), db.as<G1>(), n, chain, dout.as<G1>());
    if (hipGetLastError() != hipSuccess) { set_error("zkg_g1_add_pair29: launch failed"); return ZKG_ERROR; }
    ZK_HIP(hipMemcpy(ho.data(), dout.p, n * sizeof(G1), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) store_norm(out_jac + 12 * i, ho[i]);
    return ZKG_OK;
}
int zkg_g2_sum(const uint64_t *points_jac, size_t count, uint64_t out_jac[24]) {
    G2 acc = G2::inf();
    for (size_t i = 0; i < count; ++i) acc.add(load_norm_g2(points_jac + 24 * i));
    store_norm(out_jac, acc);
    return ZKG_OK;
}

int zkg_curve_op(int group, int op, const uint32_t *a, const uint32_t *b, const uint32_t *k, size_t n, int chain, uint32_t *out) {
    REQUIRE_INIT();
    const bool binary = op == CURVE_MADD || op == CURVE_ADD || op == CURVE_ADD_QUAD;
    if (group < 0 || group > 1 || op < 0 || op >= CURVE_OPS || !a || !out || (binary && !b) || (op == CURVE_MUL && !k) || n > ((size_t)1 << 20) ||
        chain < 0 || chain > 64 || (chain && !binary)) { set_error("zkg_curve_op: bad argument"); return ZKG_ERROR; }
    if (!n) return ZKG_OK;
    return group == 0 ? curve_op_group<Fq>(op, a, b, k, n, chain, out) : curve_op_group<Fq2>(op, a, b, k, n, chain, out);
}

int zkg_g1_fixed_base_dev(const uint64_t base[8], const void *d_scalars, size_t n, void *d_out_affine, void *stream) {
    REQUIRE_INIT();
    G1Affine b; memcpy(&b, base, 64);
    return fixed_base_g1(b, (const uint32_t *)d_scalars, n, (G1Affine *)d_out_affine, (hipStream_t)stream);
}
int zkg_g2_fixed_base_dev(const uint64_t base[16], const void *d_scalars, size_t n, void *d_out_affine, void *stream) {
    REQUIRE_INIT();
    G2Affine b; memcpy(&b, base, 128);
    return fixed_base_g2(b, (const uint32_t *)d_scalars, n, (G2Affine *)d_out_affine, (hipStream_t)stream);
}

int zkg_field_op(int field, int op, const uint64_t *a, const uint64_t *b, size_t n, uint64_t *out) {
    REQUIRE_INIT();
    const bool binary = (op >= 0 && op <= 2) || (op >= 10 && op <= 14 && field == 0) || (op >= 20 && op <= 22) || op == 31 || (op >= 40 && op <= 42);
    const bool known = binary || op == 3 || (op >= 6 && op <= 8) || (op == 15 && field == 0) || ((op == 4 || op == 5) && field != 2) || (op >= 26 && op <= 28) || op == 30;
    if (!known || field < 0 || field > 2 || !a || !out || (binary && !b)) { set_error("zkg_field_op: bad argument"); return ZKG_ERROR; }
    if (!n) return ZKG_OK;
    if (field == 0) return field_op_run<Fq>(op, a, binary ? b : nullptr, n, out);
    if (field == 1) return field_op_run<Fr>(op, a, binary ? b : nullptr, n, out);
    return field_op_run<Fq2>(op, a, binary ? b : nullptr, n, out);
}

int zkg_fr29_op(int op, const uint32_t *in, size_t n, uint32_t *out) {
    REQUIRE_INIT();
    if (op < 0 || op >= FR29_OPS || !in || !out || n > ((size_t)1 << 24)) { set_error("zkg_fr29_op: bad argument"); return ZKG_ERROR; }
    if (!n) return ZKG_OK;
    return fr29_op_run(op, in, n, out);
}

int zkg_fq29_op_chain(int op, int chain, const uint32_t *in, size_t n, uint32_t *out) {
    REQUIRE_INIT();
    const bool chained = op == FQ29_MADD || op == FQ29_ADD_LANE || op == FQ29_ADD_PAIR || op == FQ29_ADD_QUAD;
    if (op < 0 || op >= FQ29_OPS || !in || !out || n > ((size_t)1 << 24) || chain < 0 || chain > 64 || (chain && !chained)) { set_error("zkg_fq29_op: bad argument"); return ZKG_ERROR; }
    if (!n) return ZKG_OK;
    return fq29_op_run(op, chain, in, n, out);
}
int zkg_fq29_op(int op, const uint32_t *in, size_t n, uint32_t *out) { return zkg_fq29_op_chain(op, 0, in, n, out); }

// ---- one process, several GPUs: the G1 multi-exponentiation sharded by points.  Every shard is a resident slice of
//      the bases on one device with its own stream and workspace; a call hands each shard its slice of the scalars on a host thread of
//      its own (hipSetDevice is per thread), the shards run the complete single-GPU Pippenger concurrently, and the partial points — 96
//      bytes each — are added on the host.  There is no data-path collective: RCCL has no elliptic-curve reduction, and a sum of
//      ndev points is not worth a kernel.  (The one-process-per-GPU form of the same exchange is zklaim_amd/dist.py over RCCL.)
namespace { struct JoinAll { std::vector<std::thread> &t; ~JoinAll() { for (auto &x : t) if (x.joinable()) x.join(); } }; }   // also on an exception
// RCCL for the exchange of the shards' partial points (ZKG_MULTI_RCCL=1; BASELINE.json north_star: "RCCL ... of partial ... sums over xGMI").
// One process drives every GPU, so the communicators come from ncclCommInitAll and the all-gather of the 96-byte partials is one group call.
// The library is dlopen'ed on first use (a process that already holds PyTorch's copy gets that one): libzkg.so itself links no RCCL, and the
// single-GPU entry points never touch it.
extern "C++" {
namespace {
struct RcclApi {
    void *lib = nullptr; bool tried = false;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool ok() const { return CommInitAll && CommDestroy && AllGather && GroupStart && GroupEnd; }
};
RcclApi &rccl_api() {
    static RcclApi a; static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (!a.tried) {
        a.tried = true;
        for (const char *name : {"librccl.so.1", "librccl.so"}) { a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (a.lib) break; }
        if (a.lib) {
            a.CommInitAll = (decltype(a.CommInitAll))dlsym(a.lib, "ncclCommInitAll"); a.CommDestroy = (decltype(a.CommDestroy))dlsym(a.lib, "ncclCommDestroy");
            a.AllGather = (decltype(a.AllGather))dlsym(a.lib, "ncclAllGather"); a.GroupStart = (decltype(a.GroupStart))dlsym(a.lib, "ncclGroupStart");
            a.GroupEnd = (decltype(a.GroupEnd))dlsym(a.lib, "ncclGroupEnd"); a.GetErrorString = (decltype(a.GetErrorString))dlsym(a.lib, "ncclGetErrorString");
        }
    }
    return a;
}
}  // namespace
}  // extern "C++"
struct zkg_msm_shards {
    struct Shard { int device = 0; size_t first = 0, n = 0; DevBuf bases, scalars; MsmJob *job = nullptr; DevBuf xsend, xrecv; ncclComm_t comm = nullptr; };
    std::vector<Shard> shards; size_t n = 0;
    std::mutex mu;                       // a call owns every shard's scalar buffer, job workspace and stream: callers of one handle take turns
    int rccl_state = 0;                  // 0 not tried, 1 communicators up, -1 unavailable (no library, a device listed twice, init failed): host exchange
    uint64_t *pinned = nullptr;          // ndev x 12 words: the partials on their way to the devices, and the gathered set coming back
};
// the shards' communicators, on first use: one rank per shard, which RCCL only allows on distinct devices
static bool shards_rccl_ready(zkg_msm_shards *h) {
    if (h->rccl_state) return h->rccl_state > 0;
    h->rccl_state = -1;
    const size_t ns = h->shards.size();
    for (size_t i = 0; i < ns; ++i) for (size_t j = i + 1; j < ns; ++j) if (h->shards[i].device == h->shards[j].device) return false;   // (the single-GPU rehearsal lists a device twice)
    RcclApi &R = rccl_api();
    if (!R.ok()) return false;
    std::vector<int> devs(ns); std::vector<ncclComm_t> comms(ns, nullptr);
    for (size_t i = 0; i < ns; ++i) devs[i] = h->shards[i].device;
    int cur = 0; (void)hipGetDevice(&cur);
    bool ok = R.CommInitAll(comms.data(), (int)ns, devs.data()) == ncclSuccess;
    for (size_t i = 0; ok && i < ns; ++i) {
        zkg_msm_shards::Shard &sh = h->shards[i];
        sh.comm = comms[i];
        ok = hipSetDevice(sh.device) == hipSuccess && !sh.xsend.reserve(96) && !sh.xrecv.reserve(ns * 96);
    }
    ok = ok && hipHostMalloc((void **)&h->pinned, 2 * ns * 96, hipHostMallocDefault) == hipSuccess;
    (void)hipSetDevice(cur);
    if (!ok) { for (size_t i = 0; i < ns; ++i) if (comms[i]) { (void)R.CommDestroy(comms[i]); h->shards[i].comm = nullptr; } return false; }
    h->rccl_state = 1;
    return true;
}

int zkg_init_multi(const int *devices, int ndev) {
    if (!devices || ndev < 1) { set_error("zkg_init_multi: bad argument"); return ZKG_ERROR; }
    if (zkg_init(devices[0])) return ZKG_ERROR;                                   // also the calling thread's device for the single-GPU entry points
    std::lock_guard<std::mutex> lk(g_init_mu);
    int count = 0;
    (void)hipGetDeviceCount(&count);
    for (int i = 1; i < ndev; ++i) {
        if (devices[i] < 0 || devices[i] >= count) { set_error("zkg_init_multi: bad device index"); return ZKG_ERROR; }
        ZK_HIP(hipSetDevice(devices[i]));
        kernels_configure();                                                      // kernel attributes are per device
    }
    ZK_HIP(hipSetDevice(devices[0]));
    return ZKG_OK;
}

static zkg_msm_shards *zkg_msm_g1_shards_upload_impl(const uint64_t *bases, size_t n, const int *devices, int ndev) {
    if (g_device < 0) { set_error("zkg_init not called"); return nullptr; }
    if ((n && !bases) || !devices || ndev < 1 || ndev > 64) { set_error("zkg_msm_g1_shards_upload: bad argument"); return nullptr; }
    std::unique_ptr<zkg_msm_shards, void (*)(zkg_msm_shards *)> holder(new zkg_msm_shards(), zkg_msm_g1_shards_free);   // released on every early exit
    zkg_msm_shards *h = holder.get();
    h->n = n; h->shards.resize((size_t)ndev);
    std::vector<int> rc((size_t)ndev, ZKG_OK);
    std::vector<std::thread> th;
    {
    JoinAll join_guard{th};
    for (int i = 0; i < ndev; ++i) {
        zkg_msm_shards::Shard &sh = h->shards[(size_t)i];
        sh.device = devices[i]; sh.first = n * (size_t)i / (size_t)ndev; sh.n = n * (size_t)(i + 1) / (size_t)ndev - sh.first;
        th.emplace_back([&sh, &rc, i, bases] {
            if (hipSetDevice(sh.device) != hipSuccess) { set_error("zkg_msm_g1_shards_upload: hipSetDevice failed"); rc[(size_t)i] = ZKG_ERROR; return; }
            sh.job = msm_job_create(nullptr, true);
            if (!sh.job || sh.bases.reserve(sh.n * 64 + 16) || sh.scalars.reserve(sh.n * 32 + 16) ||
                (sh.n && !hip_ok(hipMemcpy(sh.bases.p, bases + 8 * sh.first, sh.n * 64, hipMemcpyHostToDevice), "H2D", __FILE__, __LINE__))) rc[(size_t)i] = ZKG_ERROR;
        });
    }
    }
    for (int r : rc) if (r) return nullptr;
    return holder.release();
}
zkg_msm_shards *zkg_msm_g1_shards_upload(const uint64_t *bases, size_t n, const int *devices, int ndev) {
    return zk::c_boundary<zkg_msm_shards *>("zkg_msm_g1_shards_upload", nullptr, [&] { return zkg_msm_g1_shards_upload_impl(bases, n, devices, ndev); });
}

void zkg_msm_g1_shards_free(zkg_msm_shards *h) {
    if (!h) return;
    int cur = 0; (void)hipGetDevice(&cur);
    for (auto &sh : h->shards) {
        (void)hipSetDevice(sh.device); msm_job_destroy(sh.job); sh.bases.release(); sh.scalars.release(); sh.xsend.release(); sh.xrecv.release();
        if (sh.comm) (void)rccl_api().CommDestroy(sh.comm);
    }
    if (h->pinned) (void)hipHostFree(h->pinned);
    (void)hipSetDevice(cur);
    delete h;
}
size_t zkg_msm_g1_shards_count(const zkg_msm_shards *h, size_t *points) { if (points) *points = h ? h->n : 0; return h ? h->shards.size() : 0; }

static std::atomic<unsigned> g_multi_rccl_calls{0};                                // zkg_msm_g1_multi calls that exchanged over RCCL (zkg_multi_rccl_calls)
unsigned zkg_multi_rccl_calls(void) { return g_multi_rccl_calls.load(); }
static int zkg_msm_g1_multi_impl(const zkg_msm_shards *h_, const uint64_t *scalars, uint64_t out_jac[12], uint64_t *partials_jac) {
    zkg_msm_shards *h = const_cast<zkg_msm_shards *>(h_);
    if (!h || !out_jac || (h->n && !scalars)) { set_error("zkg_msm_g1_multi: bad argument"); return ZKG_ERROR; }
    std::lock_guard<std::mutex> calls_take_turns(h->mu);
    const size_t ns = h->shards.size();
    std::vector<G1> part(ns, G1::inf()); std::vector<int> rc(ns, ZKG_OK);
    auto run = [&](size_t i) {
        zkg_msm_shards::Shard &sh = h->shards[i];
        if (hipSetDevice(sh.device) != hipSuccess) { set_error("zkg_msm_g1_multi: hipSetDevice failed"); rc[i] = ZKG_ERROR; return; }
        hipStream_t st = msm_job_stream(sh.job);
        MsmBases set; set.p = sh.bases.p;
        if ((sh.n && !hip_ok(hipMemcpyAsync(sh.scalars.p, scalars + 4 * sh.first, sh.n * 32, hipMemcpyHostToDevice, st), "H2D", __FILE__, __LINE__)) ||
            msm_job_launch(sh.job, &set, 1, sh.scalars.as<uint32_t>(), sh.n, false) || msm_job_finish(sh.job, &part[i], nullptr)) rc[i] = ZKG_ERROR;
    };
    std::vector<std::thread> th;
    {
        JoinAll join_guard{th};
        for (size_t i = 1; i < ns; ++i) th.emplace_back(run, i);
        int cur = 0; (void)hipGetDevice(&cur);
        run(0);                                                                   // shard 0 on the calling thread
        (void)hipSetDevice(cur);
    }
    for (int r : rc) if (r) return ZKG_ERROR;
    // the exchange.  Default: the partials are already on the host (each shard's finish step lands its chunk sums there), so they are simply
    // added.  ZKG_MULTI_RCCL=1: every device all-gathers the normalised partials over RCCL (xGMI) first and the sum is taken over what device 0
    // received — the collective form of the same 96-byte-per-GPU exchange (one more round trip; the points must agree with the host's copies).
    const bool want_rccl = getenv("ZKG_MULTI_RCCL") != nullptr;                  // (read per call: the tests switch it inside one process)
    if (want_rccl && shards_rccl_ready(h)) {
        RcclApi &R = rccl_api();
        int cur = 0; (void)hipGetDevice(&cur);
        bool ok = true;
        for (size_t i = 0; i < ns && ok; ++i) {
            store_norm(h->pinned + 12 * i, part[i]);
            ok = hipSetDevice(h->shards[i].device) == hipSuccess &&
                 hipMemcpyAsync(h->shards[i].xsend.p, h->pinned + 12 * i, 96, hipMemcpyHostToDevice, msm_job_stream(h->shards[i].job)) == hipSuccess;
        }
        ok = ok && R.GroupStart() == ncclSuccess;
        for (size_t i = 0; i < ns && ok; ++i)
            ok = hipSetDevice(h->shards[i].device) == hipSuccess &&
                 R.AllGather(h->shards[i].xsend.p, h->shards[i].xrecv.p, 12, ncclUint64, h->shards[i].comm, msm_job_stream(h->shards[i].job)) == ncclSuccess;
        ok = R.GroupEnd() == ncclSuccess && ok;
        uint64_t *got = h->pinned + 12 * ns;
        ok = ok && hipSetDevice(h->shards[0].device) == hipSuccess &&
             hipMemcpyAsync(got, h->shards[0].xrecv.p, ns * 96, hipMemcpyDeviceToHost, msm_job_stream(h->shards[0].job)) == hipSuccess;
        for (size_t i = 0; i < ns && ok; ++i) ok = hipSetDevice(h->shards[i].device) == hipSuccess && hipStreamSynchronize(msm_job_stream(h->shards[i].job)) == hipSuccess;
        (void)hipSetDevice(cur);
        if (!ok) { set_error("zkg_msm_g1_multi: the RCCL exchange failed"); return ZKG_ERROR; }
        if (memcmp(got, h->pinned, ns * 96) != 0) { set_error("zkg_msm_g1_multi: the gathered partials differ from the shards' own"); return ZKG_ERROR; }
        G1 acc = G1::inf();
        for (size_t i = 0; i < ns; ++i) { if (partials_jac) memcpy(partials_jac + 12 * i, got + 12 * i, 96); acc.add(load_norm_g1(got + 12 * i)); }
        store_norm(out_jac, acc);
        g_multi_rccl_calls.fetch_add(1);
        return ZKG_OK;
    }
    G1 acc = G1::inf();
    for (size_t i = 0; i < ns; ++i) { if (partials_jac) store_norm(partials_jac + 12 * i, part[i]); acc.add(part[i]); }
    store_norm(out_jac, acc);
    return ZKG_OK;
}
int zkg_msm_g1_multi(const zkg_msm_shards *h_, const uint64_t *scalars, uint64_t out_jac[12], uint64_t *partials_jac) {
    return zk::c_boundary("zkg_msm_g1_multi", ZKG_ERROR, [&] { return zkg_msm_g1_multi_impl(h_, scalars, out_jac, partials_jac); });
}


void zkg_timing_reset(void) { g_dominant_timer.reset(); }
float zkg_timing_dominant_ms(int *launches) { return g_dominant_timer.drain(launches); }

}  // extern "C"
