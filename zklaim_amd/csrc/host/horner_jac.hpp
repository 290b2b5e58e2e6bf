// horner_jac.hpp — runs of doublings on the host for the MSM's epilogue (host_combine: c doublings per window in Horner's rule, the chunk
// weights inside a window).  Host code only.
//
// An XYZZ doubling is 6M + 3S, and the host's squaring is its general product.  A run of n doublings goes through Jacobian coordinates
// instead — (x, y, zz, zzz) -> (X, Y, Z) = (x zz, y zzz, zz): X / Z^2 = x / zz and Y / Z^3 = y zzz / zz^3 = y / zzz — where a doubling on
// y^2 = x^3 + b costs 2M + 5S (dbl-2009-l), with a squaring of its own (ten 64 x 64 products and a separate Montgomery reduction, 26
// against the interleaved product's 32), and back: (X, Y, Z^2, Z^3).  Group elements are exact: the point is the same, its
// representative differs, and every result leaves the library normalised.
#pragma once
#include "../curve.hip.hpp"
#include <cstring>

namespace zk {

// Montgomery square a^2 R^-1 mod p of a canonical value, canonical result (what a * a returns)
static inline Fq fq_sqr_host(const Fq &a) {
    typedef unsigned __int128 u128;
    constexpr uint64_t P4[4] = {Fq::p64(0), Fq::p64(1), Fq::p64(2), Fq::p64(3)};
    uint64_t A[4], r[8];
    memcpy(A, a.v, 32);
    // the six cross products, once: r[1 .. 6]
    u128 x = (u128)A[0] * A[1];                r[1] = (uint64_t)x; uint64_t c = (uint64_t)(x >> 64);
    x = (u128)A[0] * A[2] + c;                 r[2] = (uint64_t)x; c = (uint64_t)(x >> 64);
    x = (u128)A[0] * A[3] + c;                 r[3] = (uint64_t)x; r[4] = (uint64_t)(x >> 64);
    x = (u128)A[1] * A[2] + r[3];              r[3] = (uint64_t)x; c = (uint64_t)(x >> 64);
    x = (u128)A[1] * A[3] + r[4] + c;          r[4] = (uint64_t)x; r[5] = (uint64_t)(x >> 64);
    x = (u128)A[2] * A[3] + r[5];              r[5] = (uint64_t)x; r[6] = (uint64_t)(x >> 64);
    // twice that (a < 2^254: a^2, which bounds it, is below 2^508 and nothing leaves r[7]) ...
    r[7] = r[6] >> 63;
    for (int j = 6; j >= 2; --j) r[j] = (r[j] << 1) | (r[j - 1] >> 63);
    r[1] <<= 1;
    // ... plus the four squares on the diagonal (a product and two words never exceed 2^128 - 1)
    x = (u128)A[0] * A[0];                     r[0] = (uint64_t)x; c = (uint64_t)(x >> 64);
    x = (u128)r[1] + c;                        r[1] = (uint64_t)x; c = (uint64_t)(x >> 64);
    x = (u128)A[1] * A[1] + r[2] + c;          r[2] = (uint64_t)x; c = (uint64_t)(x >> 64);
    x = (u128)r[3] + c;                        r[3] = (uint64_t)x; c = (uint64_t)(x >> 64);
    x = (u128)A[2] * A[2] + r[4] + c;          r[4] = (uint64_t)x; c = (uint64_t)(x >> 64);
    x = (u128)r[5] + c;                        r[5] = (uint64_t)x; c = (uint64_t)(x >> 64);
    x = (u128)A[3] * A[3] + r[6] + c;          r[6] = (uint64_t)x; c = (uint64_t)(x >> 64);
    r[7] += c;
    // Montgomery reduction, one limb per round: r + m p has limb i zero; `top` is the carry out of limb i + 4, taken in by the next round
    uint64_t top = 0;
    for (int i = 0; i < 4; ++i) {
        const uint64_t m = r[i] * FqParams::INV64;
        c = 0;
        for (int j = 0; j < 4; ++j) { x = (u128)m * P4[j] + r[i + j] + c; r[i + j] = (uint64_t)x; c = (uint64_t)(x >> 64); }
        x = (u128)r[i + 4] + c + top; r[i + 4] = (uint64_t)x; top = (uint64_t)(x >> 64);
    }
    // (a < p: (a^2 + m p) / R < 2p < 2^255, so top is zero here) r[4 .. 7] < 2p: one conditional subtraction
    uint64_t s[4]; unsigned long long br = 0;
    for (int j = 0; j < 4; ++j) s[j] = __builtin_subcll(r[4 + j], P4[j], br, &br);
    const uint64_t keep = 0ull - (uint64_t)br;                                   // borrowed: below p already
    for (int j = 0; j < 4; ++j) s[j] ^= (s[j] ^ r[4 + j]) & keep;
    Fq out; memcpy(out.v, s, 32);
    return out;
}

// 2^n P.  Fq: through Jacobian coordinates as above; any other field (G2): n XYZZ doublings
template <class F> static inline XYZZ<F> xyzz_times_pow2(const XYZZ<F> &p, uint32_t n) {
    if (p.is_inf() || n == 0) return p;
    if constexpr (std::is_same<F, Fq>::value) {
        if (n >= 3) {                                                           // (below that the conversions' four products outweigh the gain)
            Fq X = p.x * p.zz, Y = p.y * p.zzz, Z = p.zz;
            for (uint32_t i = 0; i < n; ++i) {                                  // dbl-2009-l, a = 0
                const Fq A = fq_sqr_host(X), B = fq_sqr_host(Y), C = fq_sqr_host(B);
                const Fq D = (fq_sqr_host(X + B) - A - C).dbl(), E = A.dbl() + A, E2 = fq_sqr_host(E);
                Z = (Y * Z).dbl();
                X = E2 - D.dbl();
                Y = E * (D - X) - C.dbl().dbl().dbl();
            }
            if (Z.is_zero()) return XYZZ<Fq>::inf();                            // (a point of order two: none on this curve)
            const Fq zz = fq_sqr_host(Z);
            return {X, Y, zz, zz * Z};
        }
    }
    XYZZ<F> r = p;
    for (uint32_t i = 0; i < n; ++i) r = r.dbl();
    return r;
}

}  // namespace zk
