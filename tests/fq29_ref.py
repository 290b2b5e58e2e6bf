"""CPU reference of the multi-exponentiation's 29-bit Fq arithmetic (zklaim_amd/csrc/fq29.hip.hpp), shared by the CPU and GPU tests of that file.

Plain Python integers on value(l) = sum l_i 2^(29 i).  Two levels, as in tests/fr29_ref.py: `sim_mul` / `sim_mul2` / `sim_sqr` / `sim_sqr2`
interpret the generated streams themselves (tools/gen_mont_asm.py gen_f29 / gen_f29_dual with the default modulus, through simulate_f29):
the exact limbs the hardware must produce.  `mont` / `sqr` are the same column algorithm written out (the tests check them limb for limb
against the simulator) with the simulator's bound (a column never reaches 2^64), and the rest mirrors the header function by function: the
limb-wise operations, the zero test, the conversions and records, XYZZ29::madd with the exceptional path of k_bucket_accum29, and the
general addition in its three lane layouts.  A `Bounds` object passed to the mirrors asserts every range the comments of fq29.hip.hpp
state and keeps the peaks.  The group law is checked against affine arithmetic on y^2 = x^3 + 3 in integers."""
import os
import re

from fr29_ref import M29, M32, ROOT, Rng, gen, limbs9, value, norm  # noqa: F401  (modulus-independent helpers)

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
RHO = pow(1 << 261, -1, Q)                         # a product's Montgomery factor: mul(a, b) = a b RHO mod q
P = [(Q >> (29 * i)) & M29 for i in range(9)]
INV = (-pow(Q, -1, 1 << 29)) % (1 << 29)
PINV = pow(Q, -1, 1 << 29)
ONE = (1 << 261) % Q
TO = (32 << 261) % Q
FROM = (1 << 256) % Q
R3 = pow(1 << 261, 3, Q)
Q30 = [(Q >> (30 * i)) & ((1 << 30) - 1) if i < 8 else Q >> 240 for i in range(9)]
Q30_INV = pow(Q, -1, 1 << 30)
_QINV261 = pow(Q, -1, 1 << 261)
POINTS_SEED = 0x29F9                              # the oracle points both suites build their addition cases from
T_LIMB = int(2 ** 30.6)                            # "T's limbs below 2^30.6"


def spread(k, d):
    """k q with d 2^29 lent from every limb to the one below (f29::S{k}_{d}): every lower limb is at least d (2^29 - 1)"""
    t = limbs9(k * Q)
    return [t[0] + (d << 29)] + [t[i] + (d << 29) - d for i in range(1, 8)] + [t[8] - d]


S2_1, S4_1, S6_1, S4_3 = spread(2, 1), spread(4, 1), spread(6, 1), spread(4, 3)
SPREADS = {"S2_1": (S2_1, 2, 1), "S4_1": (S4_1, 4, 1), "S6_1": (S6_1, 6, 1), "S4_3": (S4_3, 4, 3)}


def header_constants():
    """the constants as csrc/fq29.hip.hpp states them: the nine-limb tables as lists, INV / PINV / Q30_INV as integers"""
    src = open(os.path.join(ROOT, "zklaim_amd", "csrc", "fq29.hip.hpp")).read()
    out = {}
    for name in ("P", "ONE", "TO", "FROM", "R3", "Q30", "S2_1", "S4_1", "S6_1", "S4_3"):
        out[name] = [int(x, 16) for x in re.findall(r"0x([0-9a-f]+)", re.search(r"\b" + name + r"\[9\] = \{([^}]*)\}", src).group(1))]
    for name in ("INV", "PINV", "Q30_INV"):
        out[name] = int(re.search(r"\b" + name + r" = 0x([0-9a-f]+)u", src).group(1), 16)
    return out


# ---- the streams, interpreted -----------------------------------------------------------------------------------------------------------
_streams = {}


def _stream(square, dual):
    if (square, dual) not in _streams:
        _streams[square, dual] = gen().gen_f29_dual(square) if dual else gen().gen_f29(square)
    return _streams[square, dual]


def _ops(base, l):
    return {base + i: int(x) for i, x in enumerate(l)}


def _dbl32(a):
    return [(2 * x) & M32 for x in a]


def sim_mul(a, b):
    return gen().simulate_f29(_stream(False, False), {**_ops(9, a), **_ops(18, b)})


def sim_sqr(a):
    return gen().simulate_f29(_stream(True, False), {**_ops(9, a), **_ops(18, _dbl32(a))})


def sim_mul2(a, b, c, d):
    r = gen().simulate_f29(_stream(False, True), {**_ops(18, a), **_ops(27, b), **_ops(36, c), **_ops(45, d)}, 18)
    return r[:9], r[9:]


def sim_sqr2(a, c):
    r = gen().simulate_f29(_stream(True, True), {**_ops(18, a), **_ops(27, _dbl32(a)), **_ops(36, c), **_ops(45, _dbl32(c))}, 18)
    return r[:9], r[9:]


# ---- the stated ranges ------------------------------------------------------------------------------------------------------------------
def is_digits(l):
    return max(l[:8]) <= M29 and 0 <= l[8] <= M32


class Bounds:
    """the ranges the comments of fq29.hip.hpp state, asserted while a mirror runs; `peak` keeps the largest figures seen (values in
    units of q where the comment gives them so)"""

    def __init__(self):
        self.peak = {"Pd": 0, "Rd": 0, "X": 0, "Y": 0, "ZZ": 0, "X3": 0, "Y3": 0, "ZZ3": 0, "T_limb": 0, "column": 0, "limb": 0, "product": 0}

    def _up(self, k, v):
        if v > self.peak[k]:
            self.peak[k] = v

    def limb(self, x, what):
        assert 0 <= x <= M32, f"{what}: a limb leaves [0, 2^32) ({x:#x})"
        self._up("limb", x)

    def column(self, c):
        assert c < 1 << 64, "column overflow"
        self._up("column", c)

    def product(self, a, b, what):
        la, lb = max(a) + 1, max(b) + 1
        assert 9 * la * lb + 9 * (1 << 58) + (1 << 36) < 1 << 64, f"{what}: operand limbs outside 9 La Lb + 9 2^58 + 2^36 < 2^64 ({la:#x}, {lb:#x})"
        assert value(a) * value(b) < 169 * Q * Q, f"{what}: a b >= 169 q^2"
        self._up("product", value(a) * value(b))

    def pd(self, l):
        assert is_digits(l) and value(l) < 7.1 * Q, f"Pd = {value(l) / Q:.3f} q"
        self._up("Pd", value(l))

    def rd(self, l):
        assert is_digits(l) and value(l) < 5.1 * Q, f"Rd = {value(l) / Q:.3f} q"
        self._up("Rd", value(l))

    def t(self, l):
        assert max(l) < T_LIMB and value(l) < 7.1 * Q, f"T: limb {max(l):#x}, value {value(l) / Q:.3f} q"
        self._up("T_limb", max(l))

    def stored(self, x, y, zz, zzz, computed=False):
        """a point as it is kept between additions; computed: an addition's result (its peaks are kept apart from the operands')"""
        assert all(is_digits(c) for c in (x, y, zz, zzz)), "a stored coordinate is not digits"
        assert value(x) < 5.3 * Q and value(y) < 3.4 * Q and value(zz) < 1.1 * Q and value(zzz) < 1.1 * Q, \
            f"stored point outside the invariants: X {value(x) / Q:.3f} Y {value(y) / Q:.3f} ZZ {value(zz) / Q:.3f} ZZZ {value(zzz) / Q:.3f} (units of q)"
        k = "3" if computed else ""
        self._up("X" + k, value(x)); self._up("Y" + k, value(y)); self._up("ZZ" + k, max(value(zz), value(zzz)))

    def zero_test(self, l):
        assert is_digits(l) and value(l) < 16 * Q, "is_zero_mod_p: argument is not digits below 16 q"

    def from29(self, l):
        assert is_digits(l) and value(l) < 13 * Q, "from29: argument is not digits below 13 q"

    def show(self):
        u = lambda k: f"{self.peak[k] / Q:.3f} q"
        return {"Pd": u("Pd"), "Rd": u("Rd"), "X in": u("X"), "Y in": u("Y"), "ZZ/ZZZ in": u("ZZ"), "X3": u("X3"), "Y3": u("Y3"), "ZZ3/ZZZ3": u("ZZ3"), "T limb": f"2^{_log2(self.peak['T_limb']):.2f}",
                "column": f"2^{_log2(self.peak['column']):.2f}", "limb": f"2^{_log2(self.peak['limb']):.2f}", "product": f"{self.peak['product'] / Q / Q:.1f} q^2"}


def _log2(x):
    import math
    return math.log2(x) if x else 0.0


# ---- products ---------------------------------------------------------------------------------------------------------------------------
def _reduce_columns(terms, bounds):
    """the streams' column algorithm: terms(k) gives column k's operand products; 17 columns of 29 bits in one 64-bit accumulator, nine
    quotient digits"""
    col = 0; m = []; out = [0] * 9; peak = 0
    for k in range(17):
        col += terms(k)
        if k < 9:
            for i in range(k):
                col += m[i] * P[k - i]
            m.append((((col & M32) * INV) & M32) & M29)
            col += m[k] * P[0]
        else:
            for i in range(k - 8, 9):
                col += m[i] * P[k - i]
            out[k - 9] = col & M29
        peak = max(peak, col)
        assert col < 1 << 64, "column overflow"
        col >>= 29
    assert col <= M32
    out[8] = col
    if bounds:
        bounds.column(peak)
    return out


def mont(a, b, bounds=None, what="mul"):
    """f29::mul: same limbs as sim_mul (and as either half of sim_mul2)"""
    if bounds:
        bounds.product(a, b, what)
    return _reduce_columns(lambda k: sum(a[i] * b[k - i] for i in range(max(0, k - 8), min(k, 8) + 1)), bounds)


def sqr(a, bounds=None, what="sqr"):
    """f29::sqr: the cross products once, against the doubled limb (doubled in 32 bits: limbs below 2^31); same limbs as sim_sqr"""
    if bounds:
        bounds.product(a, a, what)
        assert max(a) < 1 << 31, "sqr: a doubled limb leaves 32 bits"
    d = _dbl32(a)
    return _reduce_columns(lambda k: sum(d[i] * a[k - i] for i in range(max(0, k - 8), min(k, 8) + 1) if i < k - i) + (a[k // 2] ** 2 if k % 2 == 0 else 0), bounds)


def mont_value(av, bv):
    """the value a product returns, in closed form: (a b + m q) / 2^261 with m = -a b / q mod 2^261"""
    t = av * bv
    return (t + ((-t * _QINV261) % (1 << 261)) * Q) >> 261


# ---- limb-wise operations ---------------------------------------------------------------------------------------------------------------
def add(a, b, bounds=None):
    r = [x + y for x, y in zip(a, b)]
    if bounds:
        for x in r:
            bounds.limb(x, "add")
    return [x & M32 for x in r]


def dbl(a, bounds=None):
    return add(a, a, bounds)


def sub(a, S, b, bounds=None):
    """a + S - b, unnormalised (f29::sub); under bounds no limb may borrow or leave 32 bits"""
    r = [x + s - y for x, s, y in zip(a, S, b)]
    if bounds:
        for x in r:
            bounds.limb(x, "sub")
    return [x & M32 for x in r]


def neg(S, b, bounds=None):
    return sub([0] * 9, S, b, bounds)


def is_zero_mod_p(a, bounds=None):
    if bounds:
        bounds.zero_test(a)
    k = (a[0] * PINV) & M29
    if k > 15:
        return False
    return [int(x) for x in a] == limbs9(k * Q)


# ---- conversions and records ------------------------------------------------------------------------------------------------------------
def words8(v):
    return [(v >> (32 * i)) & M32 for i in range(8)]


def unpack(w):
    """eight 32-bit words -> nine limbs by bit position (f29::unpack)"""
    return limbs9(sum(int(x) << (32 * i) for i, x in enumerate(w)))


def unpack8(w):
    """the same behind a Rec64: bit 255 is not part of the value"""
    r = unpack(w)
    return r[:8] + [r[8] & 0x7FFFFF]


def pack8(t):
    """digits -> 32-bit words, with the header's shifts and ORs (f29::pack8, and from29 behind its product)"""
    w = []
    for l in range(8):
        i = (32 * l) // 29; s = 32 * l - 29 * i
        v = t[i] >> s
        if i + 1 < 9:
            v |= t[i + 1] << (29 - s)
        if s > 26 and i + 2 < 9:
            v |= t[i + 2] << (58 - s)
        w.append(v & M32)
    return w


def to29(w, bounds=None):
    return mont(unpack(w), limbs9(TO), bounds, "to29")


def from29(a, bounds=None):
    """-> eight 32-bit words, canonical (Fq::reduce_once behind the product by FROM)"""
    if bounds:
        bounds.from29(a)
    t = mont(a, limbs9(FROM), bounds, "from29")
    v = sum(x << (32 * i) for i, x in enumerate(pack8(t)))
    return words8(v - Q if v >= Q else v)


def rec64(x, y, inf):
    """store_rec64 -> load_rec64: (x, y, inf) as they come back"""
    xw, yw = pack8(x), pack8(y)
    if inf:
        xw[7] |= 1 << 31
    return unpack8(xw), unpack8(yw), xw[7] >> 31


def bucket29(x, y, zz, zzz, inf):
    return [[0] * 9] * 4 if inf else [list(x), list(y), list(zz), list(zzz)]


def inverse(a):
    """f29::inverse: the canonical inverse of the value, times R'^2 through the product by R3; a multiple of q gives zero limbs"""
    v = value(a) % Q
    return mont(limbs9(pow(v, -1, Q) if v else 0), limbs9(R3))


# ---- field values and the curve in integers ---------------------------------------------------------------------------------------------
def fv(l):
    """the field element a limb vector stands for"""
    return value(l) * RHO % Q


def rep(x):
    """the canonical digits that represent the field element x"""
    return limbs9(x * ONE % Q)


def to29_of(x):
    """to29 of the field element x in libff's memory form (the limbs the 32-bit path's results come back as)"""
    return to29(words8(x * FROM % Q))


def ec_add(p, s):
    """affine addition on y^2 = x^3 + 3; None is infinity"""
    if p is None:
        return s
    if s is None:
        return p
    (x1, y1), (x2, y2) = p, s
    if x1 == x2:
        if (y1 + y2) % Q == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, Q) % Q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return x3, (lam * (x1 - x3) - y1) % Q


def ec_neg(p):
    return None if p is None else (p[0], (-p[1]) % Q)


def is_point(c, p):
    """do the four coordinates (limb vectors; ZZ == 0: infinity) stand for the affine point p?  By cross-multiplication."""
    x, y, zz, zzz = (fv(v) for v in c)
    if p is None:
        return zz == 0
    return zz != 0 and pow(zz, 3, Q) == zzz * zzz % Q and x == p[0] * zz % Q and y == p[1] * zzz % Q


def scaled(p, z):
    """the affine point p as XYZZ coordinates with ZZ = z^2, ZZZ = z^3, canonical digits"""
    return [rep(p[0] * z * z % Q), rep(p[1] * z * z * z % Q), rep(z * z % Q), rep(z * z * z % Q)]


INF4 = [[0] * 9 for _ in range(4)]


# ---- XYZZ29::madd and the exceptional path of k_bucket_accum29 --------------------------------------------------------------------------
def _dbl32bit(x, y, zz, zzz):
    """XYZZ<Fq>::dbl_inl (dbl-2008-s-1) on field elements"""
    U = 2 * y % Q; V = U * U % Q; W = U * V % Q; S = x * V % Q
    M = 3 * x * x % Q
    X3 = (M * M - 2 * S) % Q
    return X3, (M * (S - X3) - W * y) % Q, V * zz % Q, W * zzz % Q


def madd(acc, bx, by, inf, bounds=None, info=None):
    """XYZZ29::madd, then — on a false return — what k_bucket_accum29 does.  acc: [x, y, zz, zzz].  Returns (acc, inf, ok); info (a dict)
    receives Pd."""
    if inf:
        one = limbs9(ONE)
        return [list(bx), norm(by, bounds), one, list(one)], False, True
    x, y, zz, zzz = acc
    if bounds:
        bounds.stored(x, y, zz, zzz)
    U2, S2 = mont(bx, zz, bounds, "bx zz"), mont(by, zzz, bounds, "by zzz")
    Pd = norm(sub(U2, S6_1, x, bounds), bounds)
    Rd = norm(sub(S2, S4_1, y, bounds), bounds)
    if bounds:
        bounds.pd(Pd); bounds.rd(Rd)
    if info is not None:
        info["Pd"] = Pd
    if is_zero_mod_p(Pd, bounds):
        # from29 -> XYZZ<Fq>::madd -> to29: with b == +-accumulator the 32-bit path doubles the affine b (mdbl-2008-s-1) or returns infinity
        for c in (x, y, zz, zzz, bx):
            from29(c, bounds)
        yb = norm(by, bounds); from29(yb, bounds)
        X, Y, ZZ, ZZZ, BX, BY = fv(x), fv(y), fv(zz), fv(zzz), fv(bx), fv(yb)
        assert (BX * ZZ - X) % Q == 0
        if (BY * ZZZ - Y) % Q:
            return acc, True, False
        return [to29_of(v) for v in _dbl32bit(BX, BY, 1, 1)], False, False
    PP, RR = sqr(Pd, bounds, "Pd^2"), sqr(Rd, bounds, "Rd^2")
    PPP, Qq = mont(Pd, PP, bounds, "Pd PP"), mont(x, PP, bounds, "x PP")
    D = add(PPP, dbl(Qq, bounds), bounds)
    x3 = norm(sub(RR, S4_3, D, bounds), bounds)
    T = sub(Qq, S6_1, x3, bounds)
    if bounds:
        bounds.t(T)
    RT, YP = mont(Rd, T, bounds, "Rd T"), mont(y, PPP, bounds, "y PPP")
    y3 = norm(sub(RT, S2_1, YP, bounds), bounds)
    z2, z3 = mont(zz, PP, bounds, "zz PP"), mont(zzz, PPP, bounds, "zzz PPP")
    if bounds:
        bounds.stored(x3, y3, z2, z3, True)
    return [x3, y3, z2, z3], False, True


def madd_out(acc, inf, ok):
    """the hook's five output vectors"""
    return ([[0] * 9] * 4 if inf else [list(c) for c in acc]) + [[int(inf), int(ok)] + [0] * 7]


# ---- the general addition: xyzz29_add_lane, and the pair and quad forms of the same arithmetic ------------------------------------------
def add_general(a, b, form="lane", bounds=None):
    """a + b on [x, y, zz, zzz] limb vectors; infinity: all zero.  The three forms compute the same columns — the pair form squares
    through the product stream (mul2(D, D, ..)), the quad form runs every product through the single stream — so one mirror serves them;
    `form` only selects how the squares are taken, and the CPU suite asserts that the limbs agree."""
    if not any(b[2]) and (form != "pair" or not any(b[3])):
        return [list(c) for c in a]
    if not any(a[2]) and (form != "pair" or not any(a[3])):
        return [list(c) for c in b]
    if bounds:
        bounds.stored(*a); bounds.stored(*b)
    U1, U2 = mont(a[0], b[2], bounds, "U1"), mont(b[0], a[2], bounds, "U2")
    S1, S2 = mont(a[1], b[3], bounds, "S1"), mont(b[1], a[3], bounds, "S2")
    Pv, Rv = norm(sub(U2, S2_1, U1, bounds), bounds), norm(sub(S2, S2_1, S1, bounds), bounds)
    p_zero, r_zero = is_zero_mod_p(Pv, bounds), is_zero_mod_p(Rv, bounds)      # (the pair form takes both verdicts up front, the others R's when P's is true)
    if p_zero:
        if not r_zero:
            return [[0] * 9 for _ in range(4)]
        for c in a:
            from29(c, bounds)
        return [to29_of(v) for v in _dbl32bit(*(fv(c) for c in a))]
    if form == "lane":
        PP, RR = sqr(Pv, bounds, "P^2"), sqr(Rv, bounds, "R^2")
    else:
        PP, RR = mont(Pv, Pv, bounds, "P P"), mont(Rv, Rv, bounds, "R R")
    ZZ12, ZZZ12 = mont(a[2], b[2], bounds, "ZZ12"), mont(a[3], b[3], bounds, "ZZZ12")
    PPP, Qq = mont(Pv, PP, bounds, "P PP"), mont(U1, PP, bounds, "U1 PP")
    X3 = norm(sub(RR, S4_3, add(PPP, dbl(Qq, bounds), bounds), bounds), bounds)
    T = sub(Qq, S6_1, X3, bounds)
    if bounds:
        bounds.t(T)
    RT, SP = mont(T, Rv, bounds, "T R"), mont(PPP, S1, bounds, "PPP S1")
    Y3 = norm(sub(RT, S2_1, SP, bounds), bounds)
    out = [X3, Y3, mont(ZZ12, PP, bounds, "ZZ3"), mont(ZZZ12, PPP, bounds, "ZZZ3")]
    if bounds:
        bounds.stored(*out, computed=True)
    return out


def add_chain(a, b, rounds, form="lane", bounds=None):
    """a + b, then `rounds` times x <- 2x + b, as the hooks chain them (x <- x + b, then x <- x + the old x)"""
    x = add_general(a, b, form, bounds)
    for _ in range(rounds):
        z = x
        x = add_general(x, b, form, bounds)
        x = add_general(x, z, form, bounds)
    return x


# ---- representatives and case families shared by the CPU and GPU tests ------------------------------------------------------------------
def reps(l, bound):
    """every representative value(l) + j q below bound (a float, units of q), as digits"""
    v = value(l)
    return [limbs9(v + j * Q) for j in range(8) if v + j * Q < bound * Q]


def worst_rep(l, bound):
    return reps(l, bound)[-1]


def worst_point(c):
    """the largest representatives of a point's coordinates that the stored invariants admit"""
    return [worst_rep(c[0], 5.3), worst_rep(c[1], 3.4), worst_rep(c[2], 1.1), worst_rep(c[3], 1.1)]


def affine_points(oracle, n, seed):
    """n affine points k G as (x, y) integers, from the oracle's fixed-base multiplication"""
    from util import ints, random_fr_canonical
    pts = oracle.g1_fixed_base(oracle.g1_generator(), random_fr_canonical(n, seed))
    v = ints(pts, Q)
    return [(v[2 * i], v[2 * i + 1]) for i in range(n)]


def small_z(rng, both=True, tries=20000):
    """a z whose ZZ = z^2 (and ZZZ = z^3) have representations below 0.1 q: the only ones with a second representative below 1.1 q"""
    for _ in range(tries):
        z = 1 + rng.below(Q - 1)
        if value(rep(z * z % Q)) < Q // 10 and (not both or value(rep(z * z * z % Q)) < Q // 10):
            return z
    raise AssertionError("no small z found")


ALL_MAX_13 = [M29] * 8 + [(13 * Q - 1) >> 232]    # eight limbs at 2^29 - 1, the top limb as for 13 q - 1
ALL_MAX_8 = [M29] * 8 + [((8 * Q) >> 232) - 1]    # ... below 8 q (the squarings' range)


def lazy_T(rng):
    """a T = Q + S6_1 - X3 as madd feeds it to a product: Q digits below 2 q, X3 digits below 5.3 q"""
    return sub(limbs9(rng.below(2 * Q)), S6_1, limbs9(rng.below(int(5.3 * Q))))


def lazy_negy(rng):
    """a by = S2_1 - y of a negated base: y digits below 1.01 q"""
    return neg(S2_1, limbs9(rng.below(int(1.01 * Q))))


N_PRODUCTS = 2048


def product_operands():
    """(a, b) of the GPU mul test: digits x digits with every edge against every edge, then one side lazy as madd feeds it (T against
    Rd below 5.1 q; a negated by against ZZZ), then random digits below 13 q"""
    rng = Rng(0xF929)
    edge = [ALL_MAX_13, [0] * 9] + [limbs9(v) for v in (1, Q - 1, Q, 13 * Q - 1)]
    t_max = sub([M29] * 8 + [(2 * Q) >> 232], S6_1, [0] * 9)                       # Q all-maximal below 2 q, X3 = 0: T's largest limbs
    y_max = neg(S2_1, [0] * 9)
    out = [(x, y) for x in edge for y in edge]
    out += [(t_max, ALL_MAX_13[:8] + [(5 * Q) >> 232]), (y_max, [M29] * 8 + [Q >> 232])]
    while len(out) < N_PRODUCTS:
        k = len(out) % 4
        if k == 0:
            out.append((lazy_T(rng), limbs9(rng.below(int(5.1 * Q)))))
        elif k == 1:
            out.append((lazy_negy(rng), limbs9(rng.below(int(1.1 * Q)))))
        elif k == 2:
            out.append((limbs9(rng.below(int(1.1 * Q))), lazy_T(rng)))                # the lazy side second (madd: Rd T; add_lane: T R)
        else:
            out.append((limbs9(rng.below(13 * Q)), limbs9(rng.below(13 * Q))))
    return out


def product_quads():
    pairs = product_operands(); n = len(pairs)
    return [(pairs[i][0], pairs[i][1], pairs[(i + 5) % n][0], pairs[(i + 5) % n][1]) for i in range(n)]


def square_operands():
    """digits up to 8 q: the edges, then random"""
    rng = Rng(0x5929)
    out = [ALL_MAX_8, [0] * 9] + [limbs9(v) for v in (1, Q - 1, Q, 8 * Q - 1, int(7.1 * Q))]
    while len(out) < N_PRODUCTS:
        out.append(limbs9(rng.below(8 * Q)))
    return out


def square_pairs():
    a = square_operands(); n = len(a)
    return [(a[i], a[(i + 3) % n]) for i in range(n)]


# ---- the addition case families (CPU and GPU tests run the same ones) --------------------------------------------------------------------
def _pick(seq, j):
    return seq[j % len(seq)]


def base_points(pts):
    """the points whose x (resp. y) representation lies below 0.01 q — the only bases with a second representative below 1.01 q — first"""
    small = [p for p in pts if value(rep(p[0])) < Q // 100 or value(rep(p[1])) < Q // 100]
    return small + [p for p in pts if p not in small]


def madd_cases(pts, pairs=64, full=8):
    """(acc, bx, by, inf, expected point) for XYZZ29::madd: per pair of points every representative of X below 5.3 q and of Y below 3.4 q
    (the full cross of the two on the first `full` pairs), ZZ / ZZZ + q where below 1.1 q (every fourth pair has a z that allows it),
    bx / by + q where below 1.01 q, by negated as S2_1 - y or not, and the accumulator at infinity"""
    rng = Rng(0xADD29)
    bases = base_points(pts[pairs:])
    out = []
    for i in range(pairs):
        A, B = pts[i], bases[i]
        z = small_z(rng, both=i % 8 == 0) if i % 4 == 0 else 1 + rng.below(Q - 1)
        c = scaled(A, z)
        xs, ys, zzs, zzzs = reps(c[0], 5.3), reps(c[1], 3.4), reps(c[2], 1.1), reps(c[3], 1.1)
        bxs, bys = reps(rep(B[0]), 1.01), reps(rep(B[1]), 1.01)
        for negated in (False, True):
            want = ec_add(A, ec_neg(B) if negated else B)
            by_of = lambda y: neg(S2_1, y) if negated else y
            sel = [(j, j) for j in range(len(xs))] + [(j + 1, j) for j in range(len(ys))]
            if i < full:
                sel = [(jx, jy) for jx in range(len(xs)) for jy in range(len(ys))]
            for n, (jx, jy) in enumerate(sel):
                out.append(([_pick(xs, jx), _pick(ys, jy), _pick(zzs, n), _pick(zzzs, n // 2)], _pick(bxs, n), by_of(_pick(bys, n // 2)), False, want))
            out.append(([[0] * 9] * 4, _pick(bxs, i), by_of(_pick(bys, i // 2)), True, ec_neg(B) if negated else B))
    return out


def madd_exceptional_cases(pts, pairs=64):
    """b == the accumulator for every representative of X (Pd = k q) and two of Y, and b == minus the accumulator, the negation written
    both ways (S2_1 - y of the base, and the base -P itself)"""
    rng = Rng(0xE29)
    out = []
    for i in range(pairs):
        B = pts[i]
        z = 1 + rng.below(Q - 1)
        c = scaled(B, z)
        xs, ys = reps(c[0], 5.3), reps(c[1], 3.4)
        bx, by = rep(B[0]), rep(B[1])
        for j, x in enumerate(xs):
            out.append(([x, _pick(ys, j), c[2], c[3]], bx, by, False, ec_add(B, B)))
        out.append(([_pick(xs, i), _pick(ys, i), c[2], c[3]], bx, neg(S2_1, by), False, None))
        out.append(([_pick(xs, i + 1), _pick(ys, i + 1), c[2], c[3]], bx, rep(-B[1] % Q), False, None))
        n = scaled(ec_neg(B), z)
        out.append(([n[0], worst_rep(n[1], 3.4), n[2], n[3]], bx, neg(S2_1, by), False, ec_add(ec_neg(B), ec_neg(B))))     # -P + (S2_1 - y: -P): the doubling
    return out


def stored_reps(c, j):
    """one choice of representatives of a stored point, rotating with j"""
    return [_pick(reps(c[0], 5.3), j), _pick(reps(c[1], 3.4), j // 2), _pick(reps(c[2], 1.1), j), _pick(reps(c[3], 1.1), j // 2)]


def add_cases(pts, pairs=64):
    """(a, b, expected point) for the general addition: both operands stored points, six rotations of representatives per pair; P + P for
    every representative of either side's X; P + (-P); infinity on either side and both"""
    rng = Rng(0xA29)
    out = []
    for i in range(pairs):
        A, B = pts[i], pts[pairs + i]
        za = small_z(rng, both=i % 8 == 0) if i % 4 == 0 else 1 + rng.below(Q - 1)
        zb = small_z(rng, both=i % 8 == 2) if i % 4 == 2 else 1 + rng.below(Q - 1)
        a, b = scaled(A, za), scaled(B, zb)
        for j in range(6):
            out.append((stored_reps(a, j), stored_reps(b, j + 1), ec_add(A, B)))
        a2 = scaled(A, zb)                                                        # the same point under another scaling
        for j in range(6):
            out.append((stored_reps(a, j), stored_reps(a2, 5 - j), ec_add(A, A)))
        out.append((stored_reps(a, i), stored_reps(a, i + 3), ec_add(A, A)))     # ... and under the same
        if i < 4:
            # P = U2 + 2 q - U1 is q (resp. 3 q) only when U1 (resp. U2) comes back above q, U1 = c + q: a product is below q + a b / R',
            # so c = x za^2 zb^2 R' mod q must be small (below 0.005 q) and a b large (X at its largest representative, ZZ above q / 2)
            while True:
                zc = 1 + rng.below(Q - 1)
                if value(rep(A[0] * za * za * zc * zc % Q)) < Q // 200 and value(rep(zc * zc % Q)) > Q // 2:
                    break
            a3 = scaled(A, zc)
            big = [worst_rep(a[0], 5.3)] + a[1:]
            out.append((big, a3, ec_add(A, A))); out.append((a3, big, ec_add(A, A)))
        m = scaled(ec_neg(A), zb)
        out.append((stored_reps(a, i), stored_reps(m, i + 1), None))
        out.append((stored_reps(m, i + 2), stored_reps(a, i), None))
        out.append((INF4, stored_reps(b, i), B)); out.append((stored_reps(a, i), INF4, A))
    out.append((INF4, INF4, None))
    return out


def chain_points(pts, n):
    """n (a, b, A, B) for the chains: both operands at the worst representatives, every other element with a z that admits ZZ + q"""
    rng = Rng(0xC29)
    out = []
    for i in range(n):
        A, B = pts[i], pts[n + i]
        za = small_z(rng) if i % 2 == 0 else 1 + rng.below(Q - 1)
        zb = small_z(rng) if i % 2 == 0 else 1 + rng.below(Q - 1)
        out.append((worst_point(scaled(A, za)), worst_point(scaled(B, zb)), A, B))
    return out


def add_chain_point(A, B, rounds):
    p = ec_add(A, B)
    for _ in range(rounds):
        p = ec_add(ec_add(p, p), B)
    return p


def madd_chain(acc, bx, by, steps, bounds=None, lift=False):
    """`steps` times acc <- acc + b from a finite accumulator; lift: every step starts from the worst representatives its result admits"""
    inf = False
    for _ in range(steps):
        if lift and not inf:
            acc = worst_point(acc)
        acc, inf, ok = madd(acc, bx, by, inf, bounds)
    return acc, inf, ok
