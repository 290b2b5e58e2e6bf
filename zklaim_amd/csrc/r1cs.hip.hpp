// r1cs.hip.hpp — the device functions of the R1CS mat-vec, shared by the prover's kernels (prover.hip) and the QAP handle's (qap.hip).
#pragma once
#include "curve.hip.hpp"

namespace zk {

// <A_i,z>, <B_i,z>, <C_i,z> for every constraint row.  Rows are short (1-3 terms) except packing and 32-bit-addition rows
// (up to 253 terms): a lane walking such a row alone would set the latency of the whole stage, so rows longer than
// LONG_ROW terms are left to k_r1cs_long (one wavefront per row, lanes stride over the terms, shuffle reduction).
// Rows C..C+l of aA carry the input-consistency terms (r1cs_to_qap_witness_map).
static constexpr uint32_t LONG_ROW = 24;

// z = [1 | w] read from the caller's witness where it lies (zkg_qap_witness_h_async): column 0 is the constant, column c element c - 1 of w.
// The prover's kernels index a resident copy of z through a plain pointer; both forms go through the same functions below.
struct WitnessInPlace {
    const Fr *w;
    ZK_D Fr operator[](size_t c) const { return c ? w[c - 1] : Fr::one(); }
};

template <class Z> ZK_D Fr row_dot_short(const uint32_t *rp, const uint32_t *col, const Fr *val, Z z, size_t i, bool &is_long) {
    Fr acc = Fr::zero();
    uint32_t k = rp[i], e = rp[i + 1];
    if (e - k > LONG_ROW) { is_long = true; return acc; }  // filled in by k_r1cs_long
    for (; k < e; ++k) acc += val[k] * z[col[k]];
    return acc;
}
// Device-scope atomics only (no fence: a release fence writes back the XCD's whole L2, and one per workgroup behind the mat-vec's 96 MB of
// fresh output doubled that stage at 2^20): the OR returns its old value and the lane waits for it, so it has been performed before the
// workgroup's barrier and ticket.
ZK_D void or_and_wait(uint32_t *word) { const uint32_t old = atomicOr(word, 1u); asm volatile("" : : "v"(old) : "memory"); }
// one wavefront per long row entry ((matrix << 30) | row): lanes stride over the terms, shuffle reduction
template <class Z> ZK_D void r1cs_long_entry(uint32_t e, uint32_t lane, const uint32_t *a_rp, const uint32_t *a_col, const Fr *a_val, const uint32_t *b_rp, const uint32_t *b_col,
                                             const Fr *b_val, const uint32_t *c_rp, const uint32_t *c_col, const Fr *c_val, Z z, Fr *aA, Fr *aB, Fr *aC) {
    const uint32_t mtx = e >> 30, row = e & 0x3fffffffu;
    const uint32_t *rp = mtx == 0 ? a_rp : mtx == 1 ? b_rp : c_rp, *col = mtx == 0 ? a_col : mtx == 1 ? b_col : c_col;
    const Fr *val = mtx == 0 ? a_val : mtx == 1 ? b_val : c_val;
    Fr acc = Fr::zero();
    for (uint32_t k = rp[row] + lane; k < rp[row + 1]; k += 64) acc += val[k] * z[col[k]];
    for (int d = 32; d >= 1; d >>= 1) {
        Fr o;
        for (int j = 0; j < 8; ++j) o.v[j] = __shfl_xor(acc.v[j], d, 64);
        acc += o;
    }
    if (lane == 0) (mtx == 0 ? aA : mtx == 1 ? aB : aC)[row] = acc.normalized();
}

}  // namespace zk
