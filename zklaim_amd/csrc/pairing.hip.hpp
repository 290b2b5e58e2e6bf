// pairing.hip.hpp — the optimal-ate Miller loop on the device (one lane per pair), for the batch verifier (verify.hip).
//
// A transcription of host/pairing.hpp, which is the specification: the same tower (xi = 9 + u, v^3 = xi, w^2 = v; an Fq12 is
// c0 + c1 w with c0 = (w^0, w^2, w^4), c1 = (w^1, w^3, w^5) coefficients), the inversion-free projective steps of LineWalker, the
// 6z+2 schedule of miller_schedule and the Frobenius addends of miller_addends.  Values are lazy ([0, 2p), fp.hip.hpp) inside a
// lane and normalised when they leave it, so the host reads the same canonical limbs its own loop would produce.
// The constants that the host derives by inversion or exponentiation (3b', gamma_1^2, gamma_1^3, N^2, N^3) are computed there once and
// passed in MillerConsts.
// The tower is host and device code (ZK_HD), as fp.hip.hpp's field operations are: compiled for the host it computes on canonical values,
// which is how the final exponentiation built on it (final_exp.hip.hpp) is checked against the specification without a GPU.
#pragma once
#include "curve.hip.hpp"

namespace zk {

struct MillerConsts { Fq2 b3, g2, g3, n2, n3; };      // 3b' = 9 / xi;  pi(Q) = (conj(x) g2, conj(y) g3);  pi^2(Q) = (x n2, y n3)

namespace dev {

ZK_HD Fq2 mul_xi(const Fq2 &a) {                           // (9 + u)(a0 + a1 u) = (9 a0 - a1) + (9 a1 + a0) u
    Fq2 a8 = a.dbl().dbl().dbl();
    return {a8.c0 + a.c0 - a.c1, a8.c1 + a.c1 + a.c0};
}
ZK_HD Fq2 conj(const Fq2 &a) { return {a.c0, a.c1.neg()}; }
ZK_HD Fq2 scale(const Fq2 &a, const Fq &s) { return {a.c0 * s, a.c1 * s}; }

struct Fq6 {
    Fq2 c0, c1, c2;
    static ZK_HD Fq6 zero() { return {Fq2::zero(), Fq2::zero(), Fq2::zero()}; }
    static ZK_HD Fq6 one() { return {Fq2::one(), Fq2::zero(), Fq2::zero()}; }
    friend ZK_HD Fq6 operator+(const Fq6 &a, const Fq6 &b) { return {a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2}; }
    friend ZK_HD Fq6 operator-(const Fq6 &a, const Fq6 &b) { return {a.c0 - b.c0, a.c1 - b.c1, a.c2 - b.c2}; }
    friend ZK_HD Fq6 operator*(const Fq6 &a, const Fq6 &o) {                     // schoolbook with v^3 = xi (host Fq6::operator*)
        Fq2 a0 = a.c0 * o.c0, a1 = a.c1 * o.c1, a2 = a.c2 * o.c2;
        Fq2 t0 = a0 + mul_xi((a.c1 + a.c2) * (o.c1 + o.c2) - a1 - a2);
        Fq2 t1 = (a.c0 + a.c1) * (o.c0 + o.c1) - a0 - a1 + mul_xi(a2);
        Fq2 t2 = (a.c0 + a.c2) * (o.c0 + o.c2) - a0 - a2 + a1;
        return {t0, t1, t2};
    }
    ZK_HD Fq6 mul_by_v() const { return {mul_xi(c2), c0, c1}; }
    ZK_HD Fq6 normalized() const { return {c0.normalized(), c1.normalized(), c2.normalized()}; }
};

struct Fq12 {
    Fq6 c0, c1;
    static ZK_HD Fq12 one() { return {Fq6::one(), Fq6::zero()}; }
    friend ZK_HD Fq12 operator*(const Fq12 &x, const Fq12 &o) {
        Fq6 a = x.c0 * o.c0, b = x.c1 * o.c1;
        return {a + b.mul_by_v(), (x.c0 + x.c1) * (o.c0 + o.c1) - a - b};
    }
    ZK_HD Fq12 sqr() const {                                                     // complex squaring (host Fq12::sqr)
        Fq6 ab = c0 * c1;
        return {(c0 + c1) * (c0 + c1.mul_by_v()) - ab - ab.mul_by_v(), ab + ab};
    }
    ZK_HD Fq12 normalized() const { return {c0.normalized(), c1.normalized()}; }
};

// f * (a + b w + c w^3), a, b, c in Fq2 (host mul_by_line2)
ZK_HD Fq12 mul_by_line2(const Fq12 &f, const Fq2 &a, const Fq2 &b, const Fq2 &c) {
    auto sparse = [](const Fq6 &x, const Fq2 &b_, const Fq2 &c_) {             // x * (b_ + c_ v)
        Fq2 x0b = x.c0 * b_, x1c = x.c1 * c_;
        Fq2 mid = (x.c0 + x.c1) * (b_ + c_) - x0b - x1c;
        return Fq6{x0b + mul_xi(x.c2 * c_), mid, x1c + x.c2 * b_};
    };
    Fq6 f0A = {f.c0.c0 * a, f.c0.c1 * a, f.c0.c2 * a}, f1B = sparse(f.c1, b, c);
    return {f0A + f1B.mul_by_v(), sparse(f.c0 + f.c1, a + b, c) - f0A - f1B};
}

// host LineWalker: homogeneous projective T = (X : Y : Z) on the twist; each step returns its line (a, b, c) and moves T
struct LineWalker {
    Fq2 X, Y, Z;
    ZK_HD void dbl(const Fq2 &b3, Fq2 &la, Fq2 &lb, Fq2 &lc) {
        Fq2 B = Y.sqr(), C = Z.sqr(), E = C * b3, F = E.dbl() + E, H = (Y + Z).sqr() - B - C, J = X.sqr();
        la = H; lb = J.dbl() + J; lc = B - E;
        Fq2 E2 = E.sqr(), E4 = E2.dbl().dbl();
        Fq2 X3 = ((X * Y) * (B - F)).dbl(), Y3 = (B + F).sqr() - (E4.dbl() + E4), Z3 = (B * H).dbl().dbl();
        X = X3; Y = Y3; Z = Z3;
    }
    ZK_HD void add(const G2Affine &R, Fq2 &la, Fq2 &lb, Fq2 &lc) {
        Fq2 theta = Y - R.y * Z, mu = X - R.x * Z;
        la = mu; lb = theta; lc = theta * R.x - mu * R.y;
        Fq2 C = theta.sqr(), D = mu.sqr(), E = mu * D, F = Z * C, G = X * D, H = E + F - G.dbl();
        Fq2 X3 = mu * H, Y3 = theta * (G - H) - E * Y, Z3 = Z * E;
        X = X3; Y = Y3; Z = Z3;
    }
};

// ML(P, Q) of one finite pair: miller_schedule's 64 doublings of 6z + 2 = 2^64 + 0x9d797039be763ba8, an addition of Q after each
// doubling whose bit is set, then the additions of pi(Q) and -pi^2(Q) (miller_addends)
ZK_HD Fq12 miller_loop(const G1Affine &P, const G2Affine &Q, const MillerConsts &k) {
    constexpr uint64_t S_LO = 0x9d797039be763ba8ull;
    Fq12 f = Fq12::one();
    LineWalker T{Q.x, Q.y, Fq2::one()};
    const Fq nx = P.x.neg();
    Fq2 la, lb, lc;
#pragma unroll 1
    for (int i = 63; i >= 0; --i) {
        f = f.sqr();
        T.dbl(k.b3, la, lb, lc);
        f = mul_by_line2(f, scale(la, P.y), scale(lb, nx), lc);
        if ((S_LO >> i) & 1) {                                                  // the same bit in every lane: no divergence
            T.add(Q, la, lb, lc);
            f = mul_by_line2(f, scale(la, P.y), scale(lb, nx), lc);
        }
    }
    const G2Affine q1 = {conj(Q.x) * k.g2, conj(Q.y) * k.g3};
    T.add(q1, la, lb, lc);
    f = mul_by_line2(f, scale(la, P.y), scale(lb, nx), lc);
    const G2Affine q2 = {Q.x * k.n2, (Q.y * k.n3).neg()};
    T.add(q2, la, lb, lc);
    return mul_by_line2(f, scale(la, P.y), scale(lb, nx), lc);
}

}  // namespace dev
}  // namespace zk
