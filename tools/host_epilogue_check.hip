// host_epilogue_check.hip — the MSM's host epilogue, old against new, on the CPU (no GPU is touched: host code only).
//   * fq_sqr_host(a) against a * a on edge values and random ones;
//   * xyzz_times_pow2 (Jacobian run of doublings) against n XYZZ doublings on random points in random representations, for every n the
//     epilogue uses, infinity included;
//   * Horner's rule over 16 random window values with 16 doublings per window, both ways, the results compared as affine points, and timed.
// Build and run (host pass only is enough):
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/host_epilogue_check.hip -o build_variants/host_epilogue_check && build_variants/host_epilogue_check
//   and the same with -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined
#include "../zklaim_amd/csrc/host/horner_jac.hpp"
#include <chrono>
#include <cstdio>
#include <vector>

using namespace zk;

static uint64_t g_state = 0x5A4B4C41494D0003ull;
static uint64_t next64() {                                     // SplitMix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static Fq random_fq() {                                        // 253 random bits: below p
    Fq r;
    for (int i = 0; i < 4; ++i) { const uint64_t w = next64(); r.v[2 * i] = (uint32_t)w; r.v[2 * i + 1] = (uint32_t)(w >> 32); }
    r.v[7] &= 0x1fffffffu;
    return r;
}
static XYZZ<Fq> random_point() {                               // k G in a random representation (x l^2, y l^3, l^2, l^3)
    const XYZZ<Fq> g = XYZZ<Fq>::from_affine(Affine<Fq>{Fq::from_u64(1), Fq::from_u64(2)});
    uint32_t k[8];
    for (int i = 0; i < 8; ++i) k[i] = (uint32_t)next64();
    k[7] &= 0x0fffffffu;
    const Affine<Fq> a = g.mul(k, 8).to_affine();
    Fq l = random_fq();
    if (l.is_zero()) l = Fq::one();
    const Fq l2 = l.sqr(), l3 = l2 * l;
    return {a.x * l2, a.y * l3, l2, l3};
}
static bool same_point(const XYZZ<Fq> &a, const XYZZ<Fq> &b) {
    const Affine<Fq> p = a.to_affine(), q = b.to_affine();
    return p.x == q.x && p.y == q.y;
}
static XYZZ<Fq> dbl_n_old(XYZZ<Fq> p, uint32_t n) { for (uint32_t i = 0; i < n; ++i) p = p.dbl(); return p; }

template <class Dbl> static XYZZ<Fq> horner(const std::vector<XYZZ<Fq>> &V, uint32_t c, Dbl dbl_n) {
    XYZZ<Fq> acc = XYZZ<Fq>::inf();
    for (int w = (int)V.size() - 1; w >= 0; --w) {
        if (!acc.is_inf()) acc = dbl_n(acc, c);
        acc.add(V[w]);
    }
    return acc;
}

int main() {
    int bad = 0;
    // squaring: edge values, then random ones
    std::vector<Fq> edge;
    edge.push_back(Fq::zero()); edge.push_back(Fq::one()); edge.push_back(Fq::zero() - Fq::one());          // 0, R mod p, p - R mod p
    { Fq t = Fq::zero(); t.v[0] = 1; edge.push_back(t); edge.push_back(Fq::zero() - t); }                    // limbs 1 and p - 1
    { Fq t; for (int i = 0; i < 8; ++i) t.v[i] = 0xffffffffu; t.v[7] = 0x2fffffffu; edge.push_back(t); }     // all-ones limbs below p
    { Fq t = Fq::zero(); t.v[1] = 0xffffffffu; t.v[3] = 0xffffffffu; t.v[5] = 0xffffffffu; edge.push_back(t); }
    for (const Fq &a : edge) if (!(fq_sqr_host(a) == a * a)) { ++bad; fprintf(stderr, "square differs on an edge value\n"); }
    for (int i = 0; i < 200000; ++i) { const Fq a = random_fq(); if (!(fq_sqr_host(a) == a * a)) { ++bad; fprintf(stderr, "square differs on random value %d\n", i); break; } }
    // runs of doublings
    for (uint32_t n : {0u, 1u, 2u, 3u, 4u, 11u, 12u, 16u, 48u})
        for (int i = 0; i < 8; ++i) {
            const XYZZ<Fq> p = random_point();
            if (!same_point(xyzz_times_pow2(p, n), dbl_n_old(p, n))) { ++bad; fprintf(stderr, "2^%u P differs\n", n); }
        }
    if (!xyzz_times_pow2(XYZZ<Fq>::inf(), 16).is_inf()) { ++bad; fprintf(stderr, "2^16 * infinity is not infinity\n"); }
    // Horner over 16 windows of 16 bits, some of them infinity, old against new
    double t_old = 0, t_new = 0;
    const int rounds = 50;
    for (int r = 0; r < rounds; ++r) {
        std::vector<XYZZ<Fq>> V(16);
        for (auto &v : V) v = random_point();
        if (r % 5 == 1) { V[15] = XYZZ<Fq>::inf(); V[3] = XYZZ<Fq>::inf(); }
        if (r % 5 == 2) V[7] = V[8];
        const auto a = std::chrono::steady_clock::now();
        const XYZZ<Fq> o = horner(V, 16, dbl_n_old);
        const auto b = std::chrono::steady_clock::now();
        const XYZZ<Fq> n = horner(V, 16, [](const XYZZ<Fq> &p, uint32_t k) { return xyzz_times_pow2(p, k); });
        const auto c = std::chrono::steady_clock::now();
        t_old += std::chrono::duration<double, std::micro>(b - a).count(); t_new += std::chrono::duration<double, std::micro>(c - b).count();
        if (!same_point(o, n)) { ++bad; fprintf(stderr, "Horner differs in round %d\n", r); }
    }
    printf("Horner, 16 windows x 16 doublings: XYZZ %.1f us, Jacobian %.1f us (mean of %d)\n", t_old / rounds, t_new / rounds, rounds);
    printf(bad ? "FAILED: %d differences\n" : "ok: squares, runs of doublings and Horner agree\n", bad);
    return bad ? 1 : 0;
}
