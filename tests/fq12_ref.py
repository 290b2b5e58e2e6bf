"""Shared by tests/test_pairing_reference.py (CPU) and tests/test_gpu_pairing_reference.py (GPU): the raw-limb side of zkg_fq12_op and its
expected values from oracle/pyref.py's polynomial Fq12 (12 integers modulo w^12 - 18 w^6 + 82), which shares no structure with the tower.

A raw element is twelve integers in [0, 2^256), the tower's Fq coefficients in FeSlots::each_fq order (c0.c0.c0, c0.c0.c1, .. c1.c2.c1), each
a Montgomery-form word taken as given: it stands for raw * 2^-256 mod q whatever representative of that residue it is."""
import random

import numpy as np

import pyref as P
from util import MONT, Q

RINV = pow(MONT, -1, Q)
EDGES = (0, Q, 1, Q - 1, Q + 1, 2 * Q - 1)              # the ends of the lazy range [0, 2q); q is the lazy zero
OPS = ("mul", "sqr", "mul_by_line2", "cyclotomic_sqr", "inverse", "conjugate", "frobenius1", "frobenius2", "frobenius3", "mul_by_v")
N_LANES = 65                                            # one full wavefront and a last block with one live lane


def words(raws):
    """raw elements (lists of 12 ints) -> (n, 96) uint32"""
    return np.frombuffer(b"".join(int(c).to_bytes(32, "little") for e in raws for c in e), np.uint32).reshape(len(raws), 96).copy()


def unwords(a):
    """(n, 96) uint32 -> raw elements"""
    b = np.ascontiguousarray(a, dtype=np.uint32).tobytes()
    return [[int.from_bytes(b[384 * i + 32 * k:384 * i + 32 * k + 32], "little") for k in range(12)] for i in range(len(a))]


def fq2s_to_poly(v):
    """twelve Fq VALUES in the tower's order -> the polynomial: a_i = alpha + beta u is the coefficient of w^i and u = w^6 - 9"""
    p = [0] * 12
    for pos, i in enumerate(P.GT_ORDER):
        p = P.p_add(p, P.p_from_f2((v[2 * pos], v[2 * pos + 1]), i))
    return p


def raw_to_poly(raw):
    return fq2s_to_poly([c * RINV % Q for c in raw])


def poly_to_raw(p):
    """the canonical raw element of a polynomial"""
    b = P.ser_gt(p)
    return [int.from_bytes(b[32 * k:32 * k + 32], "little") for k in range(12)]


def other_representative(raw):
    """the same residues written the other way: x + q below q, x - q from q on (both stay inside [0, 2q))"""
    return [c + Q if c < Q else c - Q for c in raw]


def line_to_poly(raw6):
    """mul_by_line2's second operand: the line a + b w + c w^3 with a, b, c in Fq2 (six raw words)"""
    v = [c * RINV % Q for c in raw6]
    out = P.p_from_f2((v[0], v[1]), 0)
    out = P.p_add(out, P.p_from_f2((v[2], v[3]), 1))
    return P.p_add(out, P.p_from_f2((v[4], v[5]), 3))


def conj_poly(p):
    """x^(q^6): w -> -w (test_pairing_reference.py checks this against pow(x, q^6) itself)"""
    return [c if i % 2 == 0 else (-c) % Q for i, c in enumerate(p)]


_FROB_BASIS = {}


def frobenius_poly(p, k):
    """pow(x, q^k) through its Fq-linearity: x = sum x_i w^i with x_i in Fq gives x^(q^k) = sum x_i (w^i)^(q^k).  The twelve images of the
    basis are pyref.frobenius_ref's, computed once; the tests compare a few whole elements with frobenius_ref(x, k) itself as well."""
    if k not in _FROB_BASIS:
        _FROB_BASIS[k] = [P.frobenius_ref([1 if j == i else 0 for j in range(12)], k) for i in range(12)]
    out = [0] * 12
    for c, img in zip(p, _FROB_BASIS[k]):
        if c:
            out = [(o + c * m) % Q for o, m in zip(out, img)]
    return out


W2 = [0, 0, 1] + [0] * 9                                # v = w^2


def lazy_pool(seed, n=N_LANES):
    """n distinct raw elements over the lazy range: the named edge cases first, then seeded mixtures.  Distinct as values, not
    only as words, so a lane that used its neighbour's operand would not pass."""
    rng = random.Random(seed)
    lo = lambda: rng.randrange(Q)                       # noqa: E731
    hi = lambda: Q + rng.randrange(Q)                   # noqa: E731
    pool = [[Q] * 12]                                                                       # every coefficient the lazy zero
    pool += [[EDGES[(j + k) % 6] for j in range(12)] for k in range(6)]                     # nothing but the ends of the range
    pool += [[lo() for _ in range(6)] + [Q] * 6, [hi() for _ in range(6)] + [Q] * 6]        # an element of Fq6, its c1 written as q
    pool += [[lo() for _ in range(6)] + [0] * 6]                                            # and as 0
    for k in (0, 1, 7, 11):                                                                 # one non-zero coefficient
        pool += [[0] * k + [lo() or 1] + [0] * (11 - k), [Q] * k + [hi()] + [Q] * (11 - k)]
    pool += [[lo() for _ in range(12)], [hi() for _ in range(12)], [2 * Q - 1] * 12, [Q + 1] * 12]
    while len(pool) < n:
        pool.append([rng.choice((lo, hi, lambda: rng.choice(EDGES)))() for _ in range(12)])
    assert len(pool) == n and len({tuple(c % Q for c in e) for e in pool}) == n and all(0 <= c < 2 * Q for e in pool for c in e)
    return pool


def line_pool(seed, n=N_LANES):
    """n raw second operands of mul_by_line2: the line in the first six words (a = 0 and c = 0 written as 0 and as q first), the other six
    words arbitrary (the operation must not read them)"""
    rng = random.Random(seed)
    pool = lazy_pool(seed ^ 0x11, n)
    junk = [[rng.randrange(Q) for _ in range(6)] for _ in range(n)]
    lines = [e[:6] for e in pool]
    for t, (zero, at) in enumerate(((0, 0), (Q, 0), (0, 4), (Q, 4), (0, 2), (Q, 2))):       # a, c (and b) = 0, written both ways
        lines[t] = [rng.randrange(2 * Q) for _ in range(6)]
        lines[t][at] = lines[t][at + 1] = zero
    return [l + j for l, j in zip(lines, junk)]


def cyclotomic_pool(seed, n=N_LANES):
    """n distinct polynomials in the cyclotomic subgroup: four values x^((q^6 - 1)(q^2 + 1)) by the reference's pow, then products of them
    (the subgroup is a group)"""
    rng = random.Random(seed)
    gens = [P.p_pow([rng.randrange(Q) for _ in range(12)], (Q ** 6 - 1) * (Q ** 2 + 1)) for _ in range(4)]
    out = [gens[0]]
    while len(out) < n:
        out.append(P.p_mul(out[-1], gens[len(out) % 4]))
    assert len({tuple(p) for p in out}) == n
    return out


def lazy_representatives(polys, seed):
    """canonical raw elements of the polynomials with seeded coefficients re-expressed as value + q (element 0 stays canonical, element 1
    has every coefficient raised)"""
    rng = random.Random(seed)
    out = []
    for t, p in enumerate(polys):
        raw = poly_to_raw(p)
        out.append([c + Q if (t == 1 or (t > 1 and rng.random() < 0.5)) else c for c in raw])
    return out


def expected(op, a_raw, b_raw=None):
    """the polynomial the operation must produce; for 'inverse' of a non-zero element the caller checks x * out = 1 instead of a value"""
    x = raw_to_poly(a_raw)
    if op == "mul":
        return P.p_mul(x, raw_to_poly(b_raw))
    if op in ("sqr", "cyclotomic_sqr"):
        return P.p_mul(x, x)
    if op == "mul_by_line2":
        return P.p_mul(x, line_to_poly(b_raw[:6]))
    if op == "conjugate":
        return conj_poly(x)
    if op.startswith("frobenius"):
        return frobenius_poly(x, int(op[-1]))
    if op == "mul_by_v":
        return P.p_mul(x, W2)
    raise ValueError(op)


def check_outputs(op, a_raws, b_raws, out_words, lazy):
    """every output coefficient inside the range (below 2q from the device, below q from the host build) and the output, reduced mod q,
    equal to the reference's value.  Returns the outputs as polynomials."""
    outs = unwords(out_words)
    assert len(outs) == len(a_raws)
    polys = []
    for t, (a, o) in enumerate(zip(a_raws, outs)):
        bound = 2 * Q if lazy else Q
        assert all(c < bound for c in o), (op, t, [hex(c) for c in o if c >= bound])
        got = raw_to_poly(o)
        if op == "inverse":
            x = raw_to_poly(a)
            assert P.p_mul(x, got) == (P.P_ONE if any(x) else [0] * 12), (op, t)
        else:
            assert got == expected(op, a, b_raws[t] if b_raws is not None else None), (op, t)
        polys.append(got)
    return polys
