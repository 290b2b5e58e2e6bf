"""Reference and operand families for the 32-bit device layer (csrc/fp.hip.hpp, csrc/mont_asm.inc, the device compile of csrc/curve.hip.hpp).

On the device a field value is ANY representative in [0, 2p): zero is 0 or p, add / sub fold once with 2p, products skip the final
subtraction, and the exceptional branches of the group law test is_zero() of unnormalised differences.  This module restates that layer on
plain Python integers in two forms that must agree:
  * the COMMITTED instruction streams of csrc/mont_asm.inc, read back from the file and interpreted by tools/gen_mont_asm.py
    (decode / simulate for the product, simulate_addsub for add and sub): `Lazy(fp, sim=True)`;
  * their closed forms: (ab + (ab * -1/p mod 2^256) p) / 2^256, a + b folded once with 2p, a - b plus 2p after a borrow: `Lazy(fp)`.
    tests/test_fp32_mirror.py holds the two against each other on every family below, so the GPU tests may use the fast one on every
    element and the interpreter on the edge families and on the first N_SIM elements of the random ones.
Exact results are integers mod p (`Exact`, and oracle/pyref.py's f2_* / ec_add / ec_mul for Fq2 and the groups).
Every family has a fixed seed.  tests/test_gpu_fp32.py and tests/test_gpu_curve32.py run them on the GPU."""
import functools
import importlib.util
import os
import random
import re

import numpy as np

import pyref
from util import Q, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR = 1 << 256
M32 = 0xFFFFFFFF
N_SIM = 64            # elements per random family that also go through the stream interpreter (0.2 ms a product, 0.1 ms an add); edge families: all


def _load_gen():
    spec = importlib.util.spec_from_file_location("gen_mont_asm", os.path.join(ROOT, "tools", "gen_mont_asm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _load_gen()


@functools.lru_cache(None)
def committed_streams():
    """macro name -> instruction texts, read from the committed csrc/mont_asm.inc (what hipcc compiles, not what the generator would emit)"""
    txt = open(os.path.join(ROOT, "zklaim_amd", "csrc", "mont_asm.inc")).read()
    out = {}
    for m in re.finditer(r'#define (ZK_\w+_ASM_\w+) \\\n((?:    ".*" \\\n)+)    ""', txt):
        out[m.group(1)] = re.findall(r'"(.*?)\\n\\t"', m.group(2))
    return out


class Fp32:
    """one prime field's 32-bit layer: sim_* interpret the committed streams, mul / add / sub are the closed forms they must equal"""

    def __init__(self, name, p):
        key = name.upper()
        P, inv32 = GEN.FIELDS[key]
        assert sum(x << (32 * i) for i, x in enumerate(P)) == p
        s = committed_streams()
        self.name, self.p, self.inv32, self.P = name, p, inv32, P
        self.ninv = (-pow(p, -1, RR)) % RR
        self.rinv = pow(RR, -1, p)
        self.one = RR % p
        self._mul = GEN.decode([GEN.Ins(t) for t in s[f"ZK_MONT_MUL_ASM_{key}"]])
        self._add, self._sub = s[f"ZK_FP_ADD_ASM_{key}"], s[f"ZK_FP_SUB_ASM_{key}"]

    def sim_mul(self, a, b): return self._mul(a, b)
    def sim_add(self, a, b): return GEN.simulate_addsub(self._add, a, b)
    def sim_sub(self, a, b): return GEN.simulate_addsub(self._sub, a, b)

    def mul(self, a, b):
        t = a * b
        return (t + (t * self.ninv % RR) * self.p) >> 256

    def add(self, a, b):
        t = a + b
        return t - 2 * self.p if t >= 2 * self.p else t

    def sub(self, a, b):
        t = a - b
        return t + 2 * self.p if t < 0 else t

    def quotient_digits(self, a, b):
        """the eight reduction factors m_k of the product scanning (the v_mul_lo_u32 of each column): the digits of ab * (-1/p) mod 2^256"""
        m = a * b * self.ninv % RR
        return [(m >> (32 * k)) & M32 for k in range(8)]


FQ, FR = Fp32("fq", Q), Fp32("fr", R)
FIELDS = {"fq": FQ, "fr": FR}


class Lazy:
    """device semantics of Fp<PR> on integers in [0, 2p): every operand and every result is asserted to lie below 2p"""
    width = 1

    def __init__(self, fp, sim=False):
        self.fp, self.p = fp, fp.p
        self._m, self._a, self._s = (fp.sim_mul, fp.sim_add, fp.sim_sub) if sim else (fp.mul, fp.add, fp.sub)
        self.zero, self.one = 0, fp.one

    def _chk(self, x):
        assert 0 <= x < 2 * self.p, "left the lazy range"
        return x

    def mul(self, a, b): self._chk(a); self._chk(b); return self._chk(self._m(a, b))
    def add(self, a, b): self._chk(a); self._chk(b); return self._chk(self._a(a, b))
    def sub(self, a, b): self._chk(a); self._chk(b); return self._chk(self._s(a, b))
    def neg(self, a): return self.sub(0, a)
    def sqr(self, a): return self.mul(a, a)
    def dbl(self, a): return self.add(a, a)
    def is_zero(self, a): return a == 0 or a == self.p
    def eq(self, a, b): return self.is_zero(self.sub(a, b))
    def norm(self, a): return a - self.p if a >= self.p else a
    def value(self, a): return a * self.fp.rinv % self.p                 # the field element a Montgomery representative stands for
    def flat(self, a): return [a]
    def unflat(self, l): return l[0]
    def rand(self, rnd): return rnd.randrange(self.p)


class Lazy2:
    """device semantics of Fq2 (fp.hip.hpp) over a Lazy Fq, operation order as written there"""
    width = 2

    def __init__(self, f):
        self.f, self.p = f, f.p
        self.zero, self.one = (0, 0), (f.one, 0)

    def mul(self, a, b):
        f = self.f
        aa, bb = f.mul(a[0], b[0]), f.mul(a[1], b[1])
        return (f.sub(aa, bb), f.sub(f.sub(f.mul(f.add(a[0], a[1]), f.add(b[0], b[1])), aa), bb))

    def sqr(self, a):
        f = self.f
        ab = f.mul(a[0], a[1])
        return (f.mul(f.add(a[0], a[1]), f.sub(a[0], a[1])), f.add(ab, ab))

    def add(self, a, b): return (self.f.add(a[0], b[0]), self.f.add(a[1], b[1]))
    def sub(self, a, b): return (self.f.sub(a[0], b[0]), self.f.sub(a[1], b[1]))
    def neg(self, a): return (self.f.neg(a[0]), self.f.neg(a[1]))
    def dbl(self, a): return (self.f.dbl(a[0]), self.f.dbl(a[1]))
    def is_zero(self, a): return self.f.is_zero(a[0]) and self.f.is_zero(a[1])
    def eq(self, a, b): return self.f.eq(a[0], b[0]) and self.f.eq(a[1], b[1])
    def norm(self, a): return (self.f.norm(a[0]), self.f.norm(a[1]))
    def value(self, a): return (self.f.value(a[0]), self.f.value(a[1]))
    def flat(self, a): return [a[0], a[1]]
    def unflat(self, l): return (l[0], l[1])
    def rand(self, rnd): return (self.f.rand(rnd), self.f.rand(rnd))


class Exact:
    """the field itself: integers mod p"""

    def __init__(self, p): self.p = p
    def mul(self, a, b): return a * b % self.p
    def add(self, a, b): return (a + b) % self.p
    def sub(self, a, b): return (a - b) % self.p
    def neg(self, a): return -a % self.p
    def sqr(self, a): return a * a % self.p
    def dbl(self, a): return 2 * a % self.p
    def inv(self, a): return pow(a, -1, self.p) if a else 0


class Exact2:
    """Fq2 by oracle/pyref.py"""
    mul, add, sub, neg = map(staticmethod, (pyref.f2_mul, pyref.f2_add, pyref.f2_sub, pyref.f2_neg))
    sqr = staticmethod(lambda a: pyref.f2_mul(a, a))
    dbl = staticmethod(lambda a: pyref.f2_add(a, a))
    inv = staticmethod(lambda a: pyref.f2_inv(a) if a != (0, 0) else (0, 0))


def lazy_field(field, sim=False):
    """field 0 Fq, 1 Fr, 2 Fq2 (zkg_field_op's numbering) -> (device semantics, exact field)"""
    if field == 2:
        return Lazy2(Lazy(FQ, sim)), Exact2
    fp = FR if field == 1 else FQ
    return Lazy(fp, sim), Exact(fp.p)


# ---- the ops of zkg_field_op on any of the three interfaces above (the chains exactly as include/zkg.h fixes their text) ---------------
def chain40(F, a, b): return F.mul(F.sub(F.mul(a, b), a), F.add(a, b))


def chain41(F, a, b):
    x = a
    for _ in range(8):
        x = F.sub(F.add(x, x), b)
    return x


def chain42(F, a, b):
    xx = F.sqr(a)
    M = F.add(F.dbl(xx), xx)
    return F.sub(F.sqr(M), F.dbl(F.mul(a, b)))


OPS = {"mul": lambda F, a, b: F.mul(a, b), "add": lambda F, a, b: F.add(a, b), "sub": lambda F, a, b: F.sub(a, b), "neg": lambda F, a, b: F.neg(a),
       "sqr": lambda F, a, b: F.sqr(a), "dbl": lambda F, a, b: F.dbl(a), "chain40": chain40, "chain41": chain41, "chain42": chain42}
RAW_OP = {"mul": 20, "add": 21, "sub": 22, "neg": 26, "sqr": 27, "dbl": 28, "chain40": 40, "chain41": 41, "chain42": 42}       # zkg_field_op numbers
NORM_OP = {"mul": 0, "add": 1, "sub": 2, "neg": 6, "sqr": 7, "dbl": 8}
OP_IS_ZERO, OP_EQ, OP_INVERSE = 30, 31, 3


# ---- operand families: name -> (A, B, edge) with A[i], B[i] integers below 2p; edge families are interpreted whole --------------------
def limbs32(x): return [(x >> (32 * i)) & M32 for i in range(8)]
def from_limbs32(l): return sum(int(v) << (32 * i) for i, v in enumerate(l))


def value_edges(p):
    v = [0, 1, p - 1, p, p + 1, 2 * p - 1, (p - 1) // 2, (p + 1) // 2]
    for k in range(256):
        v += [x for x in (1 << k, (1 << k) - 1) if x < 2 * p]
    return sorted(set(v))


def limb_edges(p):
    P = limbs32(p)
    v = []
    for mask in range(128):                                  # every pattern of the low seven limbs in {0, 0xFFFFFFFF}
        low = sum(M32 << (32 * j) for j in range(7) if mask >> j & 1)
        for top in (0, P[7], (2 * p - 1 - low) >> 224):      # ... under a top limb of 0, of p's, and the largest that stays below 2p
            v.append(low | top << 224)
    ones = (1 << 256) - 1
    for j in range(8):
        v += [M32 << (32 * j), ones ^ (M32 << (32 * j))]      # one limb of 0xFFFFFFFF among zeros, and the reverse
        for base in (p, 2 * p):
            v += [base + (1 << (32 * j)), base - (1 << (32 * j))]      # p and 2p with one limb moved by +-1
    return sorted(set(x for x in v if 0 <= x < 2 * p))


def fold_edges(p, rnd):
    """pairs around the single fold of add (a + b against 2p) and the single borrow of sub (a - b against 0)"""
    A, B = [], []
    picks = [0, 1, p - 1, p, p + 1, 2 * p - 1] + [rnd.randrange(2 * p) for _ in range(26)]
    for s in (2 * p - 1, 2 * p, 2 * p + 1, 4 * p - 2):
        for a in picks:
            if 0 <= s - a < 2 * p:
                A.append(a); B.append(s - a)
    for d in (0, -1, 1, -(2 * p - 1), p, -p):
        for a in picks:
            if 0 <= a - d < 2 * p:
                A.append(a); B.append(a - d)
    return A, B


def product_edges(fp, rnd):
    """(2p - 1)^2; operands that drive the reduction factor m_k of a column (m_k = low word of the column * INV32) to 0 or 0xFFFFFFFF: the
    factors are the digits of ab * (-1/p) mod 2^256, so for an odd a and a wanted digit string m, b = -m p / a mod 2^256 (redrawn until it
    lies below 2p); b = 1 and b = R mod p as raw limbs"""
    p = fp.p
    assert fp.inv32 == (-pow(p, -1, 1 << 32)) % (1 << 32) == fp.ninv & M32
    A, B = [2 * p - 1, 2 * p - 1, p, p], [2 * p - 1, p, p, 2 * p - 1]
    wanted = [0, RR - 1]                                                     # every column 0 (b = 0), every column 0xFFFFFFFF
    for k in range(8):
        for d in (0, M32):
            for _ in range(4):
                wanted.append(rnd.randrange(RR) & ~(M32 << (32 * k)) | d << (32 * k))
            wanted.append(d << (32 * k) | (RR - 1 if not d else 0) & ~(M32 << (32 * k)))      # the odd one out
    for m in wanted:
        while True:
            a = rnd.randrange(2 * p) | 1
            b = -m * p * pow(a, -1, RR) % RR
            if b < 2 * p:
                break
        assert fp.quotient_digits(a, b) == limbs32(m)
        A.append(a); B.append(b)
    for a in value_edges(p)[::9] + [rnd.randrange(2 * p) for _ in range(16)]:
        A += [a, a]; B += [1, fp.one]
    return A, B


def paired(vals, rnd):
    """a list of single values as pairs: with itself, with its neighbour, with 2p - 1 - itself and with a random member"""
    A, B = [], []
    top = max(vals)
    for i, v in enumerate(vals):
        A += [v, v, v, v]; B += [v, vals[(i + 1) % len(vals)], min(top, max(0, top - v)), rnd.choice(vals)]
    return A, B


@functools.lru_cache(None)
def field_families(name):
    fp = FIELDS[name]; p = fp.p
    rnd = random.Random({"fq": 0xF32A, "fr": 0xF32B}[name])
    fam = {}
    fam["value_edges"] = paired(value_edges(p), rnd) + (True,)
    fam["limb_edges"] = paired(limb_edges(p), rnd) + (True,)
    fam["fold_edges"] = fold_edges(p, rnd) + (True,)
    fam["product_edges"] = product_edges(fp, rnd) + (True,)
    c = [(rnd.randrange(p), rnd.randrange(p)) for _ in range(256)]       # both representatives of every canonical value, all four combinations
    fam["both_representatives"] = ([x + da for x, _ in c for da in (0, p) for _ in (0, 1)], [y + db for _, y in c for _ in (0, 1) for db in (0, p)], False)
    fam["random"] = ([rnd.randrange(2 * p) for _ in range(2048)], [rnd.randrange(2 * p) for _ in range(2048)], False)
    for A, B, _ in fam.values():
        assert len(A) == len(B) and all(0 <= x < 2 * p for x in A) and all(0 <= x < 2 * p for x in B)
    return fam


@functools.lru_cache(None)
def fq2_families():
    """Fq2 operands with components over the Fq families (a second component from elsewhere in the same family), and the corners of the
    Karatsuba sums (c0 + c1)(d0 + d1) - aa - bb and (c0 + c1)(c0 - c1) at 2p - 1"""
    rnd = random.Random(0xF32C)
    e = [0, 1, Q - 1, Q, Q + 1, 2 * Q - 1]
    corners = [((a0, a1), (b0, b1)) for a0 in e for a1 in e for b0 in (0, Q, 2 * Q - 1) for b1 in (1, Q - 1, 2 * Q - 1)]
    fam = {"karatsuba_corners": ([a for a, _ in corners], [b for _, b in corners], True)}
    for key, (A, B, edge) in field_families("fq").items():
        n = len(A); step = 4 if edge and n > 600 else 1              # the large edge families thinned: every fourth pair, still whole in Fq
        idx = list(range(0, n, step))
        fam[key] = ([(A[i], A[rnd.randrange(n)]) for i in idx], [(B[i], B[rnd.randrange(n)]) for i in idx], False)
    return fam


def sim_indices(families, thin=1):
    """per family the elements that also go through the interpreter: all of an edge family (thin > 1: every thin-th of one with more than
    256 elements), the first N_SIM of the others"""
    return {k: range(0, len(A), thin if len(A) > 256 else 1) if edge else range(min(N_SIM, len(A))) for k, (A, B, edge) in families.items()}


# ---- limb arrays ----------------------------------------------------------------------------------------------------------------------
def pack64(vals, width=1):
    """integers (width 1) or tuples of them -> (n, 4 * width) uint64 as zkg_field_op takes them: raw limbs, nothing converted"""
    flat = vals if width == 1 else [c for v in vals for c in v]
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in flat), np.uint64).reshape(len(vals), 4 * width).copy()


def unpack64(a, width=1):
    b = np.ascontiguousarray(a, np.uint64).tobytes()
    flat = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
    return flat if width == 1 else [tuple(flat[i:i + width]) for i in range(0, len(flat), width)]


# ---- the group law: XYZZ<F> of curve.hip.hpp (device compile) over a Lazy field, line by line ----------------------------------------------
def x_inf(F): return (F.zero, F.one, F.zero, F.zero)
def x_is_inf(F, a): return F.is_zero(a[2])


def x_dbl_affine(F, b):
    x, y = b
    U = F.dbl(y); V = F.sqr(U); W = F.mul(U, V); S = F.mul(x, V)
    xx = F.sqr(x); M = F.add(F.dbl(xx), xx)
    X3 = F.sub(F.sqr(M), F.dbl(S))
    Y3 = F.sub(F.mul(M, F.sub(S, X3)), F.mul(W, y))
    return (X3, Y3, V, W)


def x_dbl(F, a):
    if x_is_inf(F, a):
        return a
    X3, Y3, V, W = x_dbl_affine(F, (a[0], a[1]))
    return (X3, Y3, F.mul(V, a[2]), F.mul(W, a[3]))


def madd_differences(F, a, b):
    """the unnormalised P = U2 - U1 and R = S2 - S1 of XYZZ::madd"""
    return F.sub(F.mul(b[0], a[2]), a[0]), F.sub(F.mul(b[1], a[3]), a[1])


def add_differences(F, a, b):
    """the same for add_inl and xyzz_add_quad (lane k of the quad forms the k-th of these four products)"""
    U1, U2, S1, S2 = F.mul(a[0], b[2]), F.mul(b[0], a[2]), F.mul(a[1], b[3]), F.mul(b[1], a[3])
    return F.sub(U2, U1), F.sub(S2, S1)


def x_madd(F, a, b):
    if F.is_zero(b[0]) and F.is_zero(b[1]):
        return a
    if x_is_inf(F, a):
        return (b[0], b[1], F.one, F.one)
    P, Rr = madd_differences(F, a, b)
    if F.is_zero(P):
        return x_dbl_affine(F, b) if F.is_zero(Rr) else x_inf(F)
    PP = F.sqr(P); PPP = F.mul(P, PP); Qq = F.mul(a[0], PP)
    X3 = F.sub(F.sub(F.sqr(Rr), PPP), F.dbl(Qq))
    Y3 = F.sub(F.mul(Rr, F.sub(Qq, X3)), F.mul(a[1], PPP))
    return (X3, Y3, F.mul(a[2], PP), F.mul(a[3], PPP))


def x_add(F, a, b):
    if x_is_inf(F, b):
        return a
    if x_is_inf(F, a):
        return b
    U1, S1 = F.mul(a[0], b[2]), F.mul(a[1], b[3])
    P, Rr = add_differences(F, a, b)
    if F.is_zero(P):
        return x_dbl(F, a) if F.is_zero(Rr) else x_inf(F)
    PP = F.sqr(P); PPP = F.mul(P, PP); Qq = F.mul(U1, PP)
    X3 = F.sub(F.sub(F.sqr(Rr), PPP), F.dbl(Qq))
    Y3 = F.sub(F.mul(Rr, F.sub(Qq, X3)), F.mul(S1, PPP))
    return (X3, Y3, F.mul(F.mul(a[2], b[2]), PP), F.mul(F.mul(a[3], b[3]), PPP))


def x_normalized(F, a): return tuple(F.norm(c) for c in a)


def group_fields(group):
    """group 0 G1, 1 G2 -> (device field, exact field, pyref's curve field)"""
    return (Lazy2(Lazy(FQ)), Exact2, pyref.Field2) if group else (Lazy(FQ), Exact(Q), pyref.Field1)


def affine_value(group, a):
    """a raw XYZZ record -> the affine point (field values, out of Montgomery form) it stands for, None for infinity; also checks ZZ^3 = ZZZ^2"""
    F, E, _ = group_fields(group)
    if x_is_inf(F, a):
        return None
    x, y, zz, zzz = (F.value(c) for c in a)
    assert E.mul(E.sqr(zz), zz) == E.sqr(zzz), "ZZ^3 != ZZZ^2"
    return (E.mul(x, E.inv(zz)), E.mul(y, E.inv(zzz)))


def affine_point_value(group, b):
    F = group_fields(group)[0]
    return None if F.is_zero(b[0]) and F.is_zero(b[1]) else (F.value(b[0]), F.value(b[1]))


def chain_expected(CF, A, B, chain):
    """x <- A + B, then `chain` rounds of x <- 2x + B, by pyref.ec_add on affine values"""
    x = pyref.ec_add(CF, A, B)
    for _ in range(chain):
        x = pyref.ec_add(CF, pyref.ec_add(CF, x, x), B)
    return x


class Case:
    """one pair of operands: kind, the raw records a (XYZZ), bx (the second operand as XYZZ, ZZ != 1) and ba (as affine)"""

    def __init__(self, kind, a, bx, ba):
        self.kind, self.a, self.bx, self.ba = kind, a, bx, ba


N_GENERAL, N_DOUBLE, N_CANCEL, N_VARIANTS = 14, 28, 12, 5
CHAINS = (0, 1, 5, 16, 64)
SCALARS = [0, 1, 2, R - 1, R, R + 1, (1 << 256) - 1]


@functools.lru_cache(None)
def group_points(group, n):
    """n points k_i G of seeded scalars from the CPU oracle's fixed-base multiplication, as canonical Montgomery coordinates"""
    import zkoracle
    from util import random_fr_canonical
    zkoracle.build()
    ks = random_fr_canonical(n, 0xC32 + group)
    if group:
        rows = unpack64(zkoracle.g2_fixed_base(zkoracle.g2_generator(), ks), 4)
        return [((r[0], r[1]), (r[2], r[3])) for r in rows]
    return [tuple(r) for r in unpack64(zkoracle.g1_fixed_base(zkoracle.g1_generator(), ks), 2)]


def lift(F, rec, mask):
    """every Fq component of a canonical record independently as c (bit clear) or c + p (bit set)"""
    flat = [c for e in rec for c in F.flat(e)]
    flat = [c + (F.p if mask >> i & 1 else 0) for i, c in enumerate(flat)]
    return tuple(F.unflat(flat[i:i + F.width]) for i in range(0, len(flat), F.width))


@functools.lru_cache(None)
def group_cases(group):
    """The operand pairs of madd / add / add_quad: P + S in general position, P + P (the doubling branch), P + (-P), infinity on either side
    and on both — each in both orders, every non-infinite XYZZ operand re-scaled by its own random Z (ZZ = Z^2, ZZZ = Z^3), infinity as
    ZZ = 0 with the coordinates of XYZZ::inf() or with arbitrary ones, the affine infinity as x = y = 0.  Every pair then appears
    N_VARIANTS times: every Fq component as c, every one as c + p (so ZZ = p, x = y = p), and seeded independent choices per component.
    y = 0 has no stand-in: a point with y = 0 would have order 2, and the groups here have odd prime order r."""
    F, E, CF = group_fields(group)
    rnd = random.Random(0xC320 + group)
    pts = group_points(group, 2 * max(N_GENERAL, N_DOUBLE, N_CANCEL))
    half = len(pts) // 2
    neg = lambda P: (P[0], F.norm(F.neg(P[1])))

    def xyzz(P, junk):
        if P is None:
            return (F.rand(rnd), F.rand(rnd), F.zero, F.rand(rnd)) if junk else x_inf(F)
        z = F.rand(rnd)
        while F.is_zero(z):
            z = F.rand(rnd)
        zz = F.norm(F.sqr(z)); zzz = F.norm(F.mul(zz, z))
        return (F.norm(F.mul(P[0], zz)), F.norm(F.mul(P[1], zzz)), zz, zzz)

    abstract = []
    for i in range(N_GENERAL):
        abstract += [("general", pts[i], pts[half + i]), ("general", pts[half + i], pts[i])]
    for i in range(N_DOUBLE):
        abstract.append(("double", pts[i], pts[i]))                                     # both orders: the two sides carry different Z
    for i in range(N_CANCEL):
        abstract += [("cancel", pts[i], neg(pts[i])), ("cancel", neg(pts[half + i]), pts[half + i])]
    abstract += [("inf_a", None, pts[0]), ("inf_b", pts[1], None), ("inf_both", None, None)]
    cases = []
    for kind, A, B in abstract:
        for v in range(N_VARIANTS):
            a, bx = xyzz(A, v & 1), xyzz(B, v & 1)
            ba = (F.zero, F.zero) if B is None else B
            bits = 4 * F.width
            masks = [0, 0, 0] if v == 0 else [(1 << bits) - 1] * 3 if v == 1 else [rnd.getrandbits(bits) for _ in range(3)]
            cases.append(Case(kind, lift(F, a, masks[0]), lift(F, bx, masks[1]), lift(F, ba, masks[2])))
    assert len(cases) <= 512
    return cases


def chain_subset(cases):
    """the first four cases of every kind: the chains run on these"""
    seen, out = {}, []
    for i, c in enumerate(cases):
        if seen.setdefault(c.kind, 0) < 4:
            seen[c.kind] += 1; out.append(i)
    return out


def difference_census(group, op):
    """Over the doubling and cancellation cases, with the INTERPRETED streams: how often the raw P = U2 - U1 and (doubling only) the raw
    R = S2 - S1 come out as 0 and as p — per Fq component, so G2 reports c0 and c1 separately, and the mixed zeros (0, p) / (p, 0) too."""
    F = Lazy2(Lazy(FQ, sim=True)) if group else Lazy(FQ, sim=True)
    count = {}
    for c in group_cases(group):
        if c.kind not in ("double", "cancel"):
            continue
        P, Rr = madd_differences(F, c.a, c.ba) if op == "madd" else add_differences(F, c.a, c.bx)
        assert F.is_zero(P) and F.is_zero(Rr) == (c.kind == "double")
        for name, d in (("P", P), ("R", Rr)) if c.kind == "double" else (("P", P),):
            comps = F.flat(d)
            for j, x in enumerate(comps):
                key = f"{name}.c{j}={'0' if x == 0 else 'p'}"
                count[key] = count.get(key, 0) + 1
            if len(comps) == 2 and (comps[0] == 0) != (comps[1] == 0):
                count[f"{name} mixed"] = count.get(f"{name} mixed", 0) + 1
    return count


def census_keys(group):
    keys = [f"{n}.c{j}={z}" for n in "PR" for j in range(2 if group else 1) for z in "0p"]
    return keys + (["P mixed", "R mixed"] if group else [])


@functools.lru_cache(None)
def mul_cases(group):
    """(raw XYZZ record, scalar): the scalars 0, 1, 2, r - 1, r, r + 1, 2^256 - 1 and 32 (G2: 16) random 256-bit ones, each on its own point
    with its own Z and representatives; the last special scalar multiplies infinity as well"""
    F, E, CF = group_fields(group)
    rnd = random.Random(0xC32A + group)
    ks = SCALARS + [rnd.getrandbits(256) for _ in range(16 if group else 32)]
    pts = group_points(group, 2 * max(N_GENERAL, N_DOUBLE, N_CANCEL))
    src = [c.a for c in group_cases(group) if c.kind in ("general", "double")]
    recs = [src[(7 * i) % len(src)] for i in range(len(ks))]
    ks.append(ks[6]); recs.append(lift(F, x_inf(F), 0b0100 if not group else 0b00110000))       # infinity with ZZ = p
    assert len(ks) <= 64 and pts
    return recs, ks


# ---- raw records for zkg_curve_op: (n, coordinates, 8 or 16) uint32 ------------------------------------------------------------------------
def pack_records(F, recs):
    flat = [c for r in recs for e in r for c in F.flat(e)]
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in flat), np.uint32).reshape(len(recs), len(recs[0]), 8 * F.width).copy()


def unpack_records(F, a):
    a = np.ascontiguousarray(a, np.uint32)
    coords = a.shape[-2]
    b = a.tobytes()
    flat = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
    elems = [F.unflat(flat[i:i + F.width]) for i in range(0, len(flat), F.width)]
    return [tuple(elems[i:i + coords]) for i in range(0, len(elems), coords)]
