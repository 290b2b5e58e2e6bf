// sqrt.hip.hpp — square roots in Fq and Fq2 on the device, and the limb loader of a compressed point's coordinate: what decompressing
// a libff point costs (codec.hip's k_decompress_g1 / k_decompress_g2 for key blobs, verify.hip's k_proof_decode for proofs).
#pragma once
#include "curve.hip.hpp"

namespace zk {

// q = 3 mod 4: sqrt(a) = a^((q+1)/4) when a is a square
ZK_D Fq fq_sqrt_candidate(const Fq &a) {
    // (q + 1) / 4
    const uint32_t e[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
    return a.pow(e, 8);
}
// complex method in Fq2 = Fq[u]/(u^2+1): returns false when a is not a square
ZK_D bool fq2_sqrt(const Fq2 &a, Fq2 &out) {
    if (a.c1.is_zero()) {                               // a in Fq: sqrt is either in Fq or purely imaginary
        Fq s = fq_sqrt_candidate(a.c0);
        if (s.sqr() == a.c0) { out = {s, Fq::zero()}; return true; }
        Fq t = fq_sqrt_candidate(a.c0.neg());
        if (t.sqr() == a.c0.neg()) { out = {Fq::zero(), t}; return true; }
        return false;
    }
    Fq norm = a.c0.sqr() + a.c1.sqr();
    Fq s = fq_sqrt_candidate(norm);
    if (s.sqr() != norm) return false;
    Fq two_inv = Fq::from_u64(2).inverse();
    Fq d = (a.c0 + s) * two_inv;
    Fq c0 = fq_sqrt_candidate(d);
    if (c0.sqr() != d) { d = (a.c0 - s) * two_inv; c0 = fq_sqrt_candidate(d); if (c0.sqr() != d) return false; }
    Fq c1 = a.c1 * (c0.dbl()).inverse();
    out = {c0, c1};
    return true;
}

ZK_D Fq load_fq_bytes(const uint8_t *p) {
    Fq r;
    for (int i = 0; i < 8; ++i) r.v[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
    return r;
}
// the stored limbs of a coordinate are a canonical value, x < q: asked of every encoded point before any arithmetic touches it (the
// device's lazy range is [0, 2q), and a second encoding of one point is refused).  Host and device: the host decoders ask the same.
ZK_HD bool limbs_below_q(const Fq &x) {
    for (int i = 7; i >= 0; --i) if (x.v[i] != FqParams::P[i]) return x.v[i] < FqParams::P[i];
    return false;
}

}  // namespace zk
