// record.hip.hpp — an affine point as its compressed record (libff operator<< under libsnark's defaults: binary, Montgomery, compressed), on the
// device.  Shared by the key-blob encoder (codec.hip) and the proof epilogue (prove_async.hip).
#pragma once
#include "curve.hip.hpp"

namespace zk {

ZK_D void put_fq_bytes(uint8_t *p, const Fq &x) {
    for (int i = 0; i < 8; ++i) { p[4 * i] = (uint8_t)x.v[i]; p[4 * i + 1] = (uint8_t)(x.v[i] >> 8); p[4 * i + 2] = (uint8_t)(x.v[i] >> 16); p[4 * i + 3] = (uint8_t)(x.v[i] >> 24); }
}
ZK_D void put_g1_record(uint8_t *o, const G1Affine &a) {                  // ser::put_g1
    const bool inf = a.is_inf();
    const Fq x = inf ? Fq::zero() : a.x.normalized(), y = inf ? Fq::one() : a.y;
    o[0] = inf ? '1' : '0'; put_fq_bytes(o + 1, x); o[33] = (y.from_mont().v[0] & 1u) ? '1' : '0';
}
ZK_D void put_g2_record(uint8_t *o, const G2Affine &a) {                  // ser::put_g2
    const bool inf = a.is_inf();
    const Fq2 x = inf ? Fq2::zero() : a.x.normalized(); const Fq y0 = inf ? Fq::one() : a.y.c0;
    o[0] = inf ? '1' : '0'; put_fq_bytes(o + 1, x.c0); put_fq_bytes(o + 33, x.c1); o[65] = (y0.from_mont().v[0] & 1u) ? '1' : '0';
}

}  // namespace zk
