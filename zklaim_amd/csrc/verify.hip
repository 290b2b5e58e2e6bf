// verify.hip — device kernels of the batch Groth16 verifier (zkg_groth16_verify_batch, zkg_pairing_product; host side in setup_verify.hip).
//
// Every kernel runs one independent item per lane:
//   k_g2_subgroup   [r]B == O for each proof's B (the random weights are sound only for B in G2; libsnark's is_well_formed checks
//                   the curve equation only)
//   k_g1_mul128     r_i * P_i for the 128-bit weights (A_i and C_i in one launch: lane i uses weight i mod nw), affine out
//   k_miller        ML(P_i, Q_i) (pairing.hip.hpp), 1 for a pair with a point at infinity or flagged out
//   k_fq12_prod     the product of the Miller values of an index range [lo, hi): per block a strided product and an LDS tree; a second
//                   launch of one block folds the block results
#include "common.hpp"
#include "pairing.hip.hpp"
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

unsigned blocks_for(size_t n) { return (unsigned)((n + VB - 1) / VB); }

}  // namespace

MillerConsts miller_consts() {
    static const MillerConsts k = [] {
        using namespace pairing;
        const Fq2 g1 = gamma1(), g2 = g1.sqr(), g3 = g2 * g1, n1 = g1 * conj(g1), n2 = n1.sqr(), n3 = n2 * n1;
        return MillerConsts{fq2(9, 0) * fq2_inverse_host(xi()), g2, g3, n2, n3};
    }();
    return k;
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
