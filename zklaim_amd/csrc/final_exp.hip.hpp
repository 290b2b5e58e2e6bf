// final_exp.hip.hpp — the final exponentiation of the pairing on the device (one lane per value), for zkg_groth16_verify_each,
// zkg_pairing_each and zkg_final_exp (kernel k_final_exp_check, verify.hip).
//
// A transcription of host/pairing.hpp's final_exponentiation, which is the specification: first chunk conjugate x inverse, then
// frobenius(., 2) x .; last chunk the Fuentes-Castaneda chain A .. U with exp_by_neg_z (z = 0x44e992b44a6909f1, Granger-Scott cyclotomic
// squarings) and the Frobenius maps 1, 2, 3.  Values are lazy ([0, 2p)) inside the lane.  The powers of gamma_1, gamma_2, gamma_3 that the
// Frobenius maps multiply by are computed on the host once and passed by value (FrobConsts), as MillerConsts is.
//
// An Fq12 is 96 registers and the chain keeps five named values alive besides the one being raised, so no Fq12 lives in registers across
// two operations here: every value of the chain lives in a per-lane slot array in global memory.  FeSlots addresses word w of slot s of
// lane i at ((s * 96 + w) * stride + i), so the 64 lanes of a wavefront read and write 64 consecutive words.  The chain itself is a table of
// operations from slots to a slot (FeProgram, built at compile time: 292 entries, the three exponentiations unrolled into it), and
// final_exponentiation is one loop over that table around one switch: each operation's code exists once, nothing but the table index lives
// across two operations, and nothing is called (an out-of-line Fq12 product saves and restores hundreds of registers through scratch).  The
// same table entry is read by every lane, so the switch does not diverge.
// Everything is host and device code: zkg_final_exp(where = 2) runs this text on the host, with one lane and stride 1.
#pragma once
#include "pairing.hip.hpp"

namespace zk {

struct FrobConsts { Fq2 g[3][5]; };                    // g[k - 1][i - 1] = gamma_k^i, gamma_k = xi^((q^k - 1)/6), k = 1..3, i = 1..5

namespace dev {

ZK_HD Fq6 neg(const Fq6 &a) { return {a.c0.neg(), a.c1.neg(), a.c2.neg()}; }
ZK_HD Fq fq_inverse_inline(const Fq &x) {                                      // Fermat, x^(q - 2), as Fq::inverse but without its call
    Fq r = Fq::one();
#pragma unroll 1
    for (int i = 255; i >= 0; --i) {
        r = r.sqr();
        if (((FqParams::P[i >> 5] - (i < 32 ? 2u : 0u)) >> (i & 31)) & 1u) r = r * x;      // P[0] ends in ..47: no borrow
    }
    return r;
}
ZK_HD Fq2 fq2_inverse_inline(const Fq2 &a) { Fq d = fq_inverse_inline(a.c0.sqr() + a.c1.sqr()); return {a.c0 * d, (a.c1 * d).neg()}; }
ZK_HD Fq6 inverse(const Fq6 &a) {                                              // host Fq6::inverse
    Fq2 t0 = a.c0.sqr() - mul_xi(a.c1 * a.c2), t1 = mul_xi(a.c2.sqr()) - a.c0 * a.c1, t2 = a.c1.sqr() - a.c0 * a.c2;
    Fq2 d = (a.c0 * t0 + mul_xi(a.c2 * t1) + mul_xi(a.c1 * t2));
    d = fq2_inverse_inline(d);
    return {t0 * d, t1 * d, t2 * d};
}
ZK_HD Fq12 conjugate(const Fq12 &x) { return {x.c0, neg(x.c1)}; }              // = x^(q^6)
ZK_HD Fq12 inverse(const Fq12 &x) { Fq6 d = inverse(x.c0 * x.c0 - (x.c1 * x.c1).mul_by_v()); return {x.c0 * d, neg(x.c1 * d)}; }
ZK_HD void fq4_sqr(const Fq2 &a, const Fq2 &b, Fq2 &r0, Fq2 &r1) {             // (a + b y)^2 with y^2 = xi
    Fq2 ab = a * b;
    r0 = (a + b) * (a + mul_xi(b)) - ab - mul_xi(ab); r1 = ab + ab;
}
ZK_HD Fq12 cyclotomic_sqr(const Fq12 &x) {                                     // Granger-Scott (host Fq12::cyclotomic_sqr)
    Fq2 z0 = x.c0.c0, z4 = x.c0.c1, z3 = x.c0.c2, z2 = x.c1.c0, z1 = x.c1.c1, z5 = x.c1.c2;
    Fq2 t0, t1, t2, t3, t4, t5;
    fq4_sqr(z0, z1, t0, t1); fq4_sqr(z2, z3, t2, t3); fq4_sqr(z4, z5, t4, t5);
    z0 = t0 - z0; z0 = z0 + z0 + t0;
    z1 = t1 + z1; z1 = z1 + z1 + t1;
    Fq2 x5 = mul_xi(t5);
    z2 = x5 + z2; z2 = z2 + z2 + x5;
    z3 = t4 - z3; z3 = z3 + z3 + t4;
    z4 = t2 - z4; z4 = z4 + z4 + t2;
    z5 = t3 + z5; z5 = z5 + z5 + t3;
    return {{z0, z4, z3}, {z2, z1, z5}};
}
// x -> x^(q^k): the coefficient a_i of w^i goes to conj^k(a_i) gamma_k^i (host frobenius); c0 = (w^0, w^2, w^4), c1 = (w^1, w^3, w^5)
template <int K> ZK_HD Fq12 frobenius(const Fq12 &x, const FrobConsts &fc) {
    auto m = [&](const Fq2 &a, int i) { return ((K & 1) ? conj(a) : a) * fc.g[K - 1][i - 1]; };
    return {{(K & 1) ? conj(x.c0.c0) : x.c0.c0, m(x.c0.c1, 2), m(x.c0.c2, 4)}, {m(x.c1.c0, 1), m(x.c1.c1, 3), m(x.c1.c2, 5)}};
}

// the slots of one lane: the named intermediates of the chain (a slot is reused once its value is dead) and a working slot
enum { FE_ELT = 0, FE_B_L = 1, FE_D_R = 2, FE_E = 3, FE_F_K = 4, FE_T = 5, FE_SLOTS = 6 };
constexpr int FE_WORDS = 96;                           // u32 words of an Fq12
struct FeSlots {
    uint32_t *p; uint32_t lane; size_t stride;         // p: word 0 of slot 0 of lane 0 (the same in every lane: a scalar base, the lane a 32-bit offset)
    template <class Fn> static ZK_HD void each_fq(Fq12 &f, Fn fn) {
        fn(f.c0.c0.c0, 0); fn(f.c0.c0.c1, 1); fn(f.c0.c1.c0, 2); fn(f.c0.c1.c1, 3); fn(f.c0.c2.c0, 4); fn(f.c0.c2.c1, 5);
        fn(f.c1.c0.c0, 6); fn(f.c1.c0.c1, 7); fn(f.c1.c1.c0, 8); fn(f.c1.c1.c1, 9); fn(f.c1.c2.c0, 10); fn(f.c1.c2.c1, 11);
    }
    ZK_HD Fq12 load(int s) const {
        Fq12 f;
        const uint32_t *q = p + (size_t)s * FE_WORDS * stride;
        each_fq(f, [&](Fq &x, int i) {
#pragma unroll
            for (int j = 0; j < 8; ++j) x.v[j] = q[(size_t)(8 * i + j) * stride + lane];
        });
        return f;
    }
    ZK_HD void store(int s, const Fq12 &v) const {
        Fq12 f = v;
        uint32_t *q = p + (size_t)s * FE_WORDS * stride;
        each_fq(f, [&](Fq &x, int i) {
#pragma unroll
            for (int j = 0; j < 8; ++j) q[(size_t)(8 * i + j) * stride + lane] = x.v[j];
        });
    }
};

// slot d = op(slot a, slot b); d may be a or b
enum : uint8_t { FE_OP_MUL, FE_OP_MUL_CONJ /* a * conjugate(b) */, FE_OP_CSQR, FE_OP_INV, FE_OP_COPY, FE_OP_CONJ, FE_OP_FROB1, FE_OP_FROB2, FE_OP_FROB3 };
struct FeOp { uint8_t op, d, a, b; };
struct FeProgram { FeOp ops[304]; int n; };
constexpr void fe_emit(FeProgram &p, uint8_t op, uint8_t d, uint8_t a, uint8_t b = 0) { p.ops[p.n].op = op; p.ops[p.n].d = d; p.ops[p.n].a = a; p.ops[p.n].b = b; ++p.n; }
// d = s^z, z = 0x44e992b44a6909f1 (63 bits), s in the cyclotomic subgroup; d != s
constexpr void fe_emit_exp_by_z(FeProgram &p, uint8_t d, uint8_t s) {
    constexpr uint64_t Z = 0x44e992b44a6909f1ull;
    fe_emit(p, FE_OP_COPY, d, s);
    for (int i = 61; i >= 0; --i) {
        fe_emit(p, FE_OP_CSQR, d, d);
        if ((Z >> i) & 1) fe_emit(p, FE_OP_MUL, d, d, s);
    }
}
// host final_exponentiation of the value in FE_T, the result in FE_T
constexpr FeProgram fe_make_program() {
    FeProgram p = {};
    // first chunk: f^((q^6 - 1)(q^2 + 1))
    fe_emit(p, FE_OP_INV, FE_F_K, FE_T);
    fe_emit(p, FE_OP_MUL_CONJ, FE_F_K, FE_F_K, FE_T);                          // a = conjugate(f) * inverse(f)
    fe_emit(p, FE_OP_FROB2, FE_T, FE_F_K);
    fe_emit(p, FE_OP_MUL, FE_ELT, FE_T, FE_F_K);                               // elt = frobenius(a, 2) * a
    // last chunk; the names are the specification's
    fe_emit_exp_by_z(p, FE_T, FE_ELT);
    fe_emit(p, FE_OP_CONJ, FE_T, FE_T);                                        // A = exp_by_neg_z(elt)
    fe_emit(p, FE_OP_CSQR, FE_B_L, FE_T);                                      // B
    fe_emit(p, FE_OP_CSQR, FE_T, FE_B_L);                                      // C
    fe_emit(p, FE_OP_MUL, FE_D_R, FE_T, FE_B_L);                               // D = C B
    fe_emit_exp_by_z(p, FE_T, FE_D_R);
    fe_emit(p, FE_OP_CONJ, FE_E, FE_T);                                        // E = exp_by_neg_z(D)
    fe_emit(p, FE_OP_CSQR, FE_F_K, FE_E);                                      // F
    fe_emit_exp_by_z(p, FE_T, FE_F_K);                                         // I = conjugate(G), G = exp_by_neg_z(F): F^z itself
    fe_emit(p, FE_OP_MUL, FE_T, FE_T, FE_E);                                   // J = I E
    fe_emit(p, FE_OP_MUL_CONJ, FE_F_K, FE_T, FE_D_R);                          // K = J H, H = conjugate(D)
    fe_emit(p, FE_OP_MUL, FE_B_L, FE_F_K, FE_B_L);                             // L = K B
    fe_emit(p, FE_OP_MUL, FE_T, FE_F_K, FE_E);                                 // M = K E
    fe_emit(p, FE_OP_MUL, FE_T, FE_T, FE_ELT);                                 // N = M elt
    fe_emit(p, FE_OP_FROB1, FE_E, FE_B_L);                                     // O = frobenius(L, 1)
    fe_emit(p, FE_OP_MUL, FE_T, FE_E, FE_T);                                   // P = O N
    fe_emit(p, FE_OP_FROB2, FE_E, FE_F_K);                                     // Q = frobenius(K, 2)
    fe_emit(p, FE_OP_MUL, FE_D_R, FE_E, FE_T);                                 // R = Q P
    fe_emit(p, FE_OP_MUL_CONJ, FE_T, FE_B_L, FE_ELT);                          // T = S L, S = conjugate(elt)
    fe_emit(p, FE_OP_FROB3, FE_E, FE_T);                                       // U = frobenius(T, 3)
    fe_emit(p, FE_OP_MUL, FE_T, FE_E, FE_D_R);                                 // U R
    return p;
}
struct FeChain { static constexpr FeProgram prog = fe_make_program(); };
static_assert(FeChain::prog.n == 292, "4 + 3 x (1 + 62 + 27) + 18 operations");

// host final_exponentiation(f_0 f_1 .. f_npre), f_0 = f and f_j = more(j) for 1 <= j <= npre; the result is lazy (normalise it where it
// leaves the lane).  The products in front run through the same switch as the chain.
template <class More> ZK_HD Fq12 final_exponentiation(const Fq12 &f, int npre, More more, const FrobConsts &fc, FeSlots ws) {
    ws.store(FE_T, f);
#pragma unroll 1
    for (int pc = -npre; pc < FeChain::prog.n; ++pc) {
        // the stride is made unknown once per operation: the 96 word addresses of a slot are otherwise computed ahead of the loop for
        // every slot and kept (and spilled) across it
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(ws.stride));
#else
        asm volatile("" : "+r"(ws.stride));
#endif
        FeOp o = {FE_OP_MUL, FE_T, FE_T, FE_E};
        if (pc < 0) ws.store(FE_E, more(npre + pc + 1)); else o = FeChain::prog.ops[pc];
        switch (o.op) {
        case FE_OP_MUL:
        case FE_OP_MUL_CONJ: {
            Fq12 y = ws.load(o.b);
            if (o.op == FE_OP_MUL_CONJ) y.c1 = neg(y.c1);
            ws.store(o.d, ws.load(o.a) * y);
            break;
        }
        case FE_OP_CSQR: ws.store(o.d, cyclotomic_sqr(ws.load(o.a))); break;
        case FE_OP_INV: ws.store(o.d, inverse(ws.load(o.a))); break;
        case FE_OP_COPY:
        case FE_OP_CONJ: {
            Fq12 y = ws.load(o.a);
            if (o.op == FE_OP_CONJ) y.c1 = neg(y.c1);
            ws.store(o.d, y);
            break;
        }
        case FE_OP_FROB1: ws.store(o.d, frobenius<1>(ws.load(o.a), fc)); break;
        case FE_OP_FROB2: ws.store(o.d, frobenius<2>(ws.load(o.a), fc)); break;
        default: ws.store(o.d, frobenius<3>(ws.load(o.a), fc)); break;
        }
    }
    return ws.load(FE_T);
}

}  // namespace dev
}  // namespace zk
