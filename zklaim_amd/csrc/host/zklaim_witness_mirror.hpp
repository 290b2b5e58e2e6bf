// zklaim_witness_mirror.hpp — the witness of zklaim's credential circuit derived from ~130 bytes per payload, in plain host / device code.
//
// The witness-only pass of build_zklaim (zklaim_circuit.hip) over the gadgets of gadgets.hpp writes one value per allocated variable, in
// allocation order, and which gate allocates never depends on the values.  This file mirrors exactly that: a word is a (32-bit value,
// 32-bit "is a variable" mask) pair, every gate computes its result word and hands the variables it allocates to a sink as one record
// (base cursor, up to two value words with their allocation masks, emitted most significant bit first, word 0's bit before word 1's).
// Nothing here knows an offset: the layout is the allocation order of build_zklaim restated as arithmetic on the payload count, and the
// size of a payload's sub-circuit is whatever cursor the trace ends at (the callers compare it with what the host pass measures).
// The same code runs on the host (zkg_zklaim_witness_mirror, the tests' reference point without a GPU) and inside k_zklaim_witness; the
// trace is cut into slices that k_zklaim_witness_par (and zkg_zklaim_witness_mirror_parallel on the host) run independently of each other.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../fp.hip.hpp"

namespace zk { namespace zwm {

#define ZW_HD ZK_HD

// what the generator reads per (context, payload)
struct Rec {
    uint8_t pre[48];                     // the pre-image: five little-endian u64 attributes and the salt
    uint8_t hash[32];
    uint64_t ref[5];                     // data_ref
    uint8_t op[5];                       // position of the op's one-hot byte inside its 8-byte slot (set_zklaim_ops), 0xff: none
    uint8_t skip;                        // the context is not part of the batch (null, wrong payload count): nothing is written for it
    uint8_t pad[2];
};
static_assert(sizeof(Rec) == 128, "one record per payload, 128 bytes");

// ---- the variable layout: build_zklaim's allocation order (tag index = variable index - 1)
struct Layout {
    uint32_t k, per, n_inputs;
    uint32_t o_zero, o_dll, o_pl, o_ref, o_ops, o_pub, o_r, o_seg, n;
    uint32_t cap;                        // the variables whose value is a field element rather than a bit: the most an item can list
};
ZW_HD Layout layout_of(uint32_t k, uint32_t per) {
    Layout L; L.k = k; L.per = per;
    L.n_inputs = (256u * 5u * k + 252u) / 253u;             // input_fe: 253 bits per element
    uint32_t c = L.n_inputs;
    L.o_zero = c; c += 1;                                   // zero
    L.o_dll = c; c += 15 * k;                               // (data, less, less_or_eq) x 5 per payload
    L.o_pl = c; c += 6 * k;                                 // plvars
    L.o_ref = c; c += 8 * k;                                // refvals
    L.o_ops = c; c += 64 * k;                               // opsvals
    L.o_pub = c; c += (256 + 512 + 512) * k;                // h_bits | ref_bits | ops_bits per payload
    L.o_r = c; c += 384 * k;                                // r_bits per payload
    L.o_seg = c; c += per * k;                              // the payload sub-circuits
    L.n = c;
    L.cap = L.n_inputs + 29 * k;                            // input_fe; data 5, plvars 6, refvals 8, alpha_packed 5, inv 5 per payload
    return L;
}

// ---- bytes of the payload's public data: hash (32) | refs (64) | ops (64), as payload_public_bytes lays them out
ZW_HD uint32_t pub_byte(const Rec &r, uint32_t at) {
    if (at < 32) return r.hash[at];
    at -= 32;
    if (at < 64) return at < 40 ? (uint32_t)(r.ref[at >> 3] >> (8 * (at & 7))) & 0xffu : 0u;
    at -= 64;
    return (at < 40 && r.op[at >> 3] == (at & 7)) ? 1u : 0u;
}
ZW_HD uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
ZW_HD uint64_t le64(const uint8_t *p) { uint64_t x = 0; for (int i = 7; i >= 0; --i) x = x << 8 | p[i]; return x; }

// ---- a record's variables into the tag array; positions outside [0, limit) are dropped, never written
ZW_HD void expand(uint8_t *tags, uint32_t limit, uint32_t base, uint32_t v0, uint32_t m0, uint32_t v1, uint32_t m1) {
    uint32_t pos = base;
    for (int i = 31; i >= 0 && ((m0 | m1) << (31 - i)); --i) {
        if ((m0 >> i) & 1) { if (pos < limit) tags[pos] = (v0 >> i) & 1; ++pos; }
        if ((m1 >> i) & 1) { if (pos < limit) tags[pos] = (v1 >> i) & 1; ++pos; }
    }
}

// ---- words and gates (gadgets.hpp: bit_xor, bit_choice, bit_majority, add_mod32 on 32 bits at once)
struct Wd { uint32_t v, m; };
ZW_HD uint32_t rr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
ZW_HD Wd rotr(Wd w, int n) { Wd o; o.v = rr(w.v, n); o.m = rr(w.m, n); return o; }
ZW_HD Wd shr(Wd w, int n) { Wd o; o.v = w.v >> n; o.m = w.m >> n; return o; }
ZW_HD Wd konst(uint32_t x) { Wd o; o.v = x; o.m = 0; return o; }
ZW_HD uint32_t popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

template <class Sink> ZW_HD void emit(Sink &s, uint32_t &cur, uint32_t v0, uint32_t m0, uint32_t v1, uint32_t m1) {
    if (!(m0 | m1)) return;
    s.put(cur, v0, m0, v1, m1);
    cur += popc(m0) + popc(m1);
}
// a xor b xor c as two xor steps: each allocates where both of its operands are variables
template <class Sink> ZW_HD Wd xor3(Sink &s, uint32_t &cur, Wd a, Wd b, Wd c) {
    const uint32_t tv = a.v ^ b.v, tm = a.m | b.m;
    Wd o; o.v = tv ^ c.v; o.m = tm | c.m;
    emit(s, cur, tv, a.m & b.m, o.v, tm & c.m);
    return o;
}
// e ? f : g: nothing when e is constant, or when f and g both are (then the result is a constant, e or its negation)
template <class Sink> ZW_HD Wd choice(Sink &s, uint32_t &cur, Wd e, Wd f, Wd g) {
    Wd o; o.v = (e.v & f.v) | (~e.v & g.v);
    const uint32_t fg = f.m | g.m;
    o.m = (~e.m & ((e.v & f.m) | (~e.v & g.m))) | (e.m & (fg | (f.v ^ g.v)));
    emit(s, cur, o.v, e.m & fg, 0, 0);
    return o;
}
// majority: with a constant operand (the first of a, b, c that is one) an AND (constant 0) or an OR (constant 1) of the other two, which
// allocates where both are variables — the OR as the AND of the negations, so its variable holds NOT (x OR y); otherwise t = a AND b, then r
template <class Sink> ZW_HD Wd majority(Sink &s, uint32_t &cur, Wd a, Wd b, Wd c) {
    const uint32_t selA = ~a.m, selC = a.m & b.m & ~c.m, selN = a.m & b.m & c.m;
    const uint32_t kv = (selA & a.v) | (a.m & ~b.m & b.v) | (selC & c.v);                          // the constant operand, where there is one
    Wd x, y;
    x.v = (selA & b.v) | (~selA & a.v); x.m = (selA & b.m) | (~selA & a.m);                        // the other two: (b, c), (a, c) or (a, b)
    y.v = (selC & b.v) | (~selC & c.v); y.m = (selC & b.m) | (~selC & c.m);
    const uint32_t both = x.m & y.m & ~selN;
    const uint32_t gate = (kv & ~(x.v | y.v)) | (~kv & x.v & y.v);
    const uint32_t m_and = (x.m & ~y.m & y.v) | (y.m & ~x.m & x.v), m_or = (x.m & ~y.m & ~y.v) | (y.m & ~x.m & ~x.v);
    Wd o; o.v = (a.v & b.v) | (c.v & (a.v ^ b.v));
    o.m = selN | both | (~selN & ((kv & m_or) | (~kv & m_and)));
    emit(s, cur, (selN & a.v & b.v) | (~selN & gate), selN | both, o.v, selN);
    return o;
}
// sum of words + constant mod 2^32: nothing when every operand is constant and there is no `out`; otherwise the 32 result bits (unless
// they are `out`, variables that exist already) and the carry bits, least significant first
template <class Sink> ZW_HD Wd add(Sink &s, uint32_t &cur, const Wd *terms, int nterms, uint32_t k, bool has_out) {
    uint64_t sum = k; uint32_t any = 0;
    for (int i = 0; i < nterms; ++i) { sum += terms[i].v; any |= terms[i].m; }
    if (!any && !has_out) return konst((uint32_t)sum);
    int extra = 0; while (((uint64_t)(nterms + 1) << 32) > ((uint64_t)1 << (32 + extra))) ++extra;
    if (!has_out) emit(s, cur, (uint32_t)sum, 0xffffffffu, 0, 0);
    emit(s, cur, __builtin_bitreverse32((uint32_t)(sum >> 32)), 0xffffffffu << (32 - extra), 0, 0);
    Wd o; o.v = (uint32_t)sum; o.m = 0xffffffffu;
    return o;
}

#define ZW_SHA256_K_LIST \
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, \
    0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, \
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, \
    0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, \
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, \
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2
#define ZW_SHA256_IV_LIST 0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19
static const uint32_t ZW_K_HOST[64] = {ZW_SHA256_K_LIST};
static const uint32_t ZW_IV_HOST[8] = {ZW_SHA256_IV_LIST};
#if defined(__HIPCC__)
__constant__ static const uint32_t ZW_K_DEV[64] = {ZW_SHA256_K_LIST};
__constant__ static const uint32_t ZW_IV_DEV[8] = {ZW_SHA256_IV_LIST};
#endif
ZW_HD uint32_t sha_k(int t) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ZW_K_DEV[t];
#else
    return ZW_K_HOST[t];
#endif
}
ZW_HD uint32_t sha_iv(int j) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ZW_IV_DEV[j];
#else
    return ZW_IV_HOST[j];
#endif
}

// alpha = 2^64 + ref - attr as 65 bits (comparison_witness)
struct Alpha { uint64_t lo; uint32_t hi, cnt; };
ZW_HD Alpha alpha_of(uint64_t attr, uint64_t ref) {
    Alpha a; a.lo = ref - attr; a.hi = ref >= attr ? 1u : 0u;
    a.cnt = popc((uint32_t)a.lo) + popc((uint32_t)(a.lo >> 32));
    return a;
}

// ---- the sub-circuit of one payload (payload_gadgets of build_zklaim): five comparisons, then sha256_compress_from_iv of the padded
// block with the digest written into h_bits (which carry the context's hash already: only the carries are new) — as ZW_SLICES slices that
// each take their operands as words and advance the cursor: comparison j, schedule step t = 16 .. 63, round t = 0 .. 63, final addition j.
// What a slice allocates depends on its operands' masks only; its values on the plain SHA-256 words of the step it stands for.
static constexpr uint32_t ZW_SL_SCHED = 5, ZW_SL_ROUND = ZW_SL_SCHED + 48, ZW_SL_FINAL = ZW_SL_ROUND + 64, ZW_SLICES = ZW_SL_FINAL + 8;
static constexpr int ZW_SLICE_OPERANDS = 9;                                     // a round's: the eight state words and W[t]

// 64 alpha bits (least significant first), alpha_packed, not_all_zeros, inv
template <class Sink> ZW_HD void slice_compare(const Rec &r, int j, uint32_t &cur, Sink &s) {
    const Alpha a = alpha_of(le64(r.pre + 8 * j), r.ref[j]);
    s.put(cur, __builtin_bitreverse32((uint32_t)a.lo), 0xffffffffu, 0, 0);
    s.put(cur + 32, __builtin_bitreverse32((uint32_t)(a.lo >> 32)), 0xffffffffu, 0, 0);
    s.put(cur + 65, a.cnt ? 0x80000000u : 0u, 0x80000000u, 0, 0);
    cur += 67;
}
// in: W[t - 16], W[t - 15], W[t - 7], W[t - 2] -> W[t]
template <class Sink> ZW_HD Wd slice_schedule(const Wd *in, uint32_t &cur, Sink &s) {
    const Wd s0 = xor3(s, cur, rotr(in[1], 7), rotr(in[1], 18), shr(in[1], 3));
    const Wd s1 = xor3(s, cur, rotr(in[3], 17), rotr(in[3], 19), shr(in[3], 10));
    const Wd terms[4] = {in[0], s0, in[2], s1};
    return add(s, cur, terms, 4, 0, false);
}
// st: a .. h at the round's entry, replaced by the state at its exit
template <class Sink> ZW_HD void slice_round(Wd *st, Wd w, int t, uint32_t &cur, Sink &s) {
    const Wd a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    const Wd S1 = xor3(s, cur, rotr(e, 6), rotr(e, 11), rotr(e, 25));
    const Wd ch = choice(s, cur, e, f, g);
    const Wd S0 = xor3(s, cur, rotr(a, 2), rotr(a, 13), rotr(a, 22));
    const Wd mj = majority(s, cur, a, b, c);
    const Wd te[5] = {d, h, S1, ch, w};
    const Wd new_e = add(s, cur, te, 5, sha_k(t), false);
    const Wd ta[6] = {h, S1, ch, w, S0, mj};
    const Wd new_a = add(s, cur, ta, 6, sha_k(t), false);
    st[7] = g; st[6] = f; st[5] = e; st[4] = new_e; st[3] = c; st[2] = b; st[1] = a; st[0] = new_a;
}
// word j of the state after the last round + IV[j] = the digest word that h_bits hold already: the carries only
template <class Sink> ZW_HD void slice_final(Wd x, int j, uint32_t &cur, Sink &s) { (void)add(s, cur, &x, 1, sha_iv(j), true); }

// The serial composition.  W: storage for the 64 message words (the schedule is allocated in full before the rounds, so all of them live
// at once).  Returns the cursor behind the last variable; base: tag index of the sub-circuit's first variable.  The observer is shown
// every slice as it is entered: its cursor relative to base and its operands (slice_plan_derive keeps them; payload_trace looks away).
struct NoObserver { ZW_HD void slice(uint32_t, uint32_t, const Wd *, int) {} };
template <class Sink, class Obs> ZW_HD uint32_t payload_trace_observed(const Rec &r, uint32_t base, Wd *W, Sink &s, Obs &o) {
    uint32_t cur = base;
    for (int j = 0; j < 5; ++j) { o.slice((uint32_t)j, cur - base, nullptr, 0); slice_compare(r, j, cur, s); }
    for (int t = 0; t < 12; ++t) { W[t].v = be32(r.pre + 4 * t); W[t].m = 0xffffffffu; }
    W[12] = konst(0x80000000u); W[13] = konst(0); W[14] = konst(0); W[15] = konst(0x180u);     // the padding of a 48-byte message
    for (int t = 16; t < 64; ++t) {
        const Wd in[4] = {W[t - 16], W[t - 15], W[t - 7], W[t - 2]};
        o.slice(ZW_SL_SCHED + (uint32_t)(t - 16), cur - base, in, 4);
        W[t] = slice_schedule(in, cur, s);
    }
    Wd st[ZW_SLICE_OPERANDS];
    for (int j = 0; j < 8; ++j) st[j] = konst(sha_iv(j));
    for (int t = 0; t < 64; ++t) {
        st[8] = W[t];
        o.slice(ZW_SL_ROUND + (uint32_t)t, cur - base, st, 9);
        slice_round(st, W[t], t, cur, s);
    }
    for (int j = 0; j < 8; ++j) { o.slice(ZW_SL_FINAL + (uint32_t)j, cur - base, &st[j], 1); slice_final(st[j], j, cur, s); }
    return cur;
}
template <class Sink> ZW_HD uint32_t payload_trace(const Rec &r, uint32_t base, Wd *W, Sink &s) { NoObserver o; return payload_trace_observed(r, base, W, s, o); }

// ---- the slices on their own (k_zklaim_witness_par, zkg_zklaim_witness_mirror_parallel).  The plan: for every slice the cursor it is
// entered at (relative to the payload's segment), the index of its first record and its operands' masks; entry ZW_SLICES closes the
// list with the segment's size and the record count.  Derived by running the serial trace on a zero record, never written down.
struct SliceEntry { uint32_t cur, rec, m[ZW_SLICE_OPERANDS]; };
struct SlicePlan { SliceEntry e[ZW_SLICES + 1]; };
// the plain SHA-256 compression of the padded 48-byte pre-image: W[0 .. 63] and the state at the entry of round t in st[8 t .. 8 t + 7]
// (t = 64: after the last round, before the IV is added) — the values of every slice's operands
static constexpr uint32_t ZW_SHA_STATE_WORDS = 65 * 8;
ZW_HD void sha_values(const Rec &r, uint32_t *W, uint32_t *st) {
    for (int t = 0; t < 12; ++t) W[t] = be32(r.pre + 4 * t);
    W[12] = 0x80000000u; W[13] = 0; W[14] = 0; W[15] = 0x180u;
    for (int t = 16; t < 64; ++t) {
        const uint32_t x = W[t - 15], y = W[t - 2];
        W[t] = W[t - 16] + (rr(x, 7) ^ rr(x, 18) ^ (x >> 3)) + W[t - 7] + (rr(y, 17) ^ rr(y, 19) ^ (y >> 10));
    }
    uint32_t a = sha_iv(0), b = sha_iv(1), c = sha_iv(2), d = sha_iv(3), e = sha_iv(4), f = sha_iv(5), g = sha_iv(6), h = sha_iv(7);
    for (int t = 0; t <= 64; ++t) {
        uint32_t *o = st + 8 * t;
        o[0] = a; o[1] = b; o[2] = c; o[3] = d; o[4] = e; o[5] = f; o[6] = g; o[7] = h;
        if (t == 64) break;
        const uint32_t t1 = h + (rr(e, 6) ^ rr(e, 11) ^ rr(e, 25)) + ((e & f) | (~e & g)) + sha_k(t) + W[t];
        const uint32_t t2 = (rr(a, 2) ^ rr(a, 13) ^ rr(a, 22)) + ((a & b) | (c & (a ^ b)));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
}
// slice q of a payload whose plain SHA-256 words are (W, st): its records go to the sink, the cursor it ends at (relative to base) comes back
template <class Sink> ZW_HD uint32_t slice_run(const Rec &r, const SliceEntry &e, uint32_t q, const uint32_t *W, const uint32_t *st, uint32_t base, Sink &s) {
    uint32_t cur = base + e.cur;
    if (q < ZW_SL_SCHED) slice_compare(r, (int)q, cur, s);
    else if (q < ZW_SL_ROUND) {
        const int t = 16 + (int)(q - ZW_SL_SCHED);
        Wd in[4];
        in[0].v = W[t - 16]; in[1].v = W[t - 15]; in[2].v = W[t - 7]; in[3].v = W[t - 2];
        for (int j = 0; j < 4; ++j) in[j].m = e.m[j];
        (void)slice_schedule(in, cur, s);
    } else if (q < ZW_SL_FINAL) {
        const int t = (int)(q - ZW_SL_ROUND);
        Wd x[8], w;
        for (int j = 0; j < 8; ++j) { x[j].v = st[8 * t + j]; x[j].m = e.m[j]; }
        w.v = W[t]; w.m = e.m[8];
        slice_round(x, w, t, cur, s);
    } else if (q < ZW_SLICES) {
        const int j = (int)(q - ZW_SL_FINAL);
        Wd x; x.v = st[8 * 64 + j]; x.m = e.m[0];
        slice_final(x, j, cur, s);
    }
    return cur - base;
}

// ---- the payload's bits outside its sub-circuit, as records at their places: record q of ZW_PUBLIC_RECORDS
static constexpr uint32_t ZW_PUBLIC_RECORDS = 12 + 40 + 5 + 2;
ZW_HD void public_record(const Layout &L, const Rec &r, uint32_t i, uint32_t q, uint32_t &base, uint32_t &v, uint32_t &m) {
    m = 0xffffffffu;
    if (q < 12) { base = L.o_r + 384 * i + 32 * q; v = be32(r.pre + 4 * q); return; }                      // r_bits: memtobv of the pre-image
    q -= 12;
    if (q < 40) {                                                                                              // h_bits | ref_bits | ops_bits
        base = L.o_pub + 1280 * i + 32 * q;
        v = pub_byte(r, 4 * q) << 24 | pub_byte(r, 4 * q + 1) << 16 | pub_byte(r, 4 * q + 2) << 8 | pub_byte(r, 4 * q + 3);
        return;
    }
    q -= 40;
    if (q < 5) {                                                                                               // less, less_or_eq of attribute q
        const Alpha a = alpha_of(le64(r.pre + 8 * q), r.ref[q]);
        base = L.o_dll + 3 * (5 * i + q) + 1; m = 0xc0000000u;
        v = ((a.hi && a.cnt) ? 0x80000000u : 0u) | (a.hi ? 0x40000000u : 0u);
        return;
    }
    q -= 5;                                                                                                    // opsvals: the 64 one-hot bytes, 8 bits each: 0 or 1
    base = L.o_ops + 64 * i + 32 * q; v = 0;
    for (uint32_t c = 0; c < 32; ++c) v |= pub_byte(r, 96 + 32 * q + c) << (31 - c);
}

// ---- the variables that hold a field element, in ascending index order: candidate q < L.cap.  raw: the integer (below 2^253), or for the
// comparisons' inverses the number of set alpha bits with is_inv set (the value is 1 / that number).  Returns the variable's tag index.
ZW_HD uint32_t candidate(const Layout &L, const Rec *recs /* k */, uint32_t q, uint32_t raw[8], bool &is_inv) {
    for (int j = 0; j < 8; ++j) raw[j] = 0;
    is_inv = false;
    const uint32_t k = L.k;
    if (q < L.n_inputs) {                                                     // 253 bits of hash || refs || ops over the payloads, memtobv order
        const uint32_t lo = 253 * q, hi = (lo + 253 < 1280 * k) ? lo + 253 : 1280 * k;
#pragma unroll
        for (int w = 0; w < 8; ++w) {                                         // (limb by limb: raw stays in registers on the device)
            uint32_t x = 0;
            for (uint32_t c = 0; c < 32; ++c) {
                const uint32_t b = lo + 32 * (uint32_t)w + c;
                if (b >= hi) break;
                const uint32_t i = b / 1280, off = b % 1280;
                x |= ((pub_byte(recs[i], off >> 3) >> (7 - (off & 7))) & 1u) << c;
            }
            raw[w] = x;
        }
        return q;
    }
    q -= L.n_inputs;
    uint64_t x;
    if (q < 5 * k) { x = le64(recs[q / 5].pre + 8 * (q % 5)); raw[0] = (uint32_t)x; raw[1] = (uint32_t)(x >> 32); return L.o_dll + 3 * q; }       // data
    q -= 5 * k;
    if (q < 6 * k) { x = le64(recs[q / 6].pre + 8 * (q % 6)); raw[0] = (uint32_t)x; raw[1] = (uint32_t)(x >> 32); return L.o_pl + q; }            // plvars
    q -= 6 * k;
    if (q < 8 * k) { x = (q % 8) < 5 ? recs[q / 8].ref[q % 8] : 0; raw[0] = (uint32_t)x; raw[1] = (uint32_t)(x >> 32); return L.o_ref + q; }      // refvals
    q -= 8 * k;
    const uint32_t i = q / 10, j = (q % 10) >> 1;
    const Alpha a = alpha_of(le64(recs[i].pre + 8 * j), recs[i].ref[j]);
    const uint32_t at = L.o_seg + L.per * i + 67 * j;
    if (q & 1) { raw[0] = a.cnt; is_inv = true; return at + 66; }                                                                                 // inv
    raw[0] = (uint32_t)a.lo; raw[1] = (uint32_t)(a.lo >> 32); raw[2] = a.hi;                                                                      // alpha_packed
    return at + 64;
}
// the tag Builder::set gives the value, and the value in Montgomery form (inv_table: 1 / c for c <= 64, Montgomery, [0] = 0)
ZW_HD uint8_t candidate_value(const uint32_t raw[8], bool is_inv, const Fr *inv_table, Fr &out) {
    uint32_t rest = 0;
    for (int j = 1; j < 8; ++j) rest |= raw[j];
    const uint8_t tag = rest ? 2 : (raw[0] == 0 ? 0 : (raw[0] == 1 ? 1 : 2));
    if (is_inv) { out = inv_table[raw[0] <= 64 ? raw[0] : 0]; return tag; }
    Fr x; for (int j = 0; j < 8; ++j) x.v[j] = raw[j];
    out = x.to_mont().normalized();
    return tag;
}

// sinks: count only (the cursor is the result), and straight into a tag array
struct CountSink { uint32_t records = 0; ZW_HD void put(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) { ++records; } };
struct TagSink { uint8_t *tags; uint32_t limit; ZW_HD void put(uint32_t base, uint32_t v0, uint32_t m0, uint32_t v1, uint32_t m1) { expand(tags, limit, base, v0, m0, v1, m1); } };
// one record per put, as the expansion reads them; a slice's records lie at [at, end) of the payload's list, `at` counts on past `end`
struct SliceRec { uint32_t base, v0, m0, v1, m1; };
struct SliceSink {
    SliceRec *r; uint32_t at, end;
    ZW_HD void put(uint32_t base, uint32_t v0, uint32_t m0, uint32_t v1, uint32_t m1) {
        if (at < end) { SliceRec x; x.base = base; x.v0 = v0; x.m0 = m0; x.v1 = v1; x.m1 = m1; r[at] = x; }
        ++at;
    }
};

// the plan: the serial trace of a zero record, watched (host, once per process)
struct PlanObserver {
    SlicePlan *p; const CountSink *s;
    ZW_HD void slice(uint32_t q, uint32_t cur, const Wd *ops, int n) {
        SliceEntry &e = p->e[q];
        e.cur = cur; e.rec = s->records;
        for (int j = 0; j < ZW_SLICE_OPERANDS; ++j) e.m[j] = j < n ? ops[j].m : 0;
    }
};
inline void slice_plan_derive(SlicePlan &p) {
    Rec r;
    for (size_t i = 0; i < sizeof(Rec); ++i) reinterpret_cast<uint8_t *>(&r)[i] = 0;
    Wd W[64]; CountSink s; PlanObserver o; o.p = &p; o.s = &s;
    SliceEntry &last = p.e[ZW_SLICES];
    last.cur = payload_trace_observed(r, 0, W, s, o); last.rec = s.records;
    for (int j = 0; j < ZW_SLICE_OPERANDS; ++j) last.m[j] = 0;
}

}}  // namespace zk::zwm
