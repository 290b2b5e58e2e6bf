"""GPU known-answer test of the 32-bit device group law (csrc/curve.hip.hpp as the device compiles it: madd, add_inl, xyzz_add_quad, dbl_inl,
dbl_affine_inl, to_affine, mul over lazy values in [0, 2p)) through zkg_curve_op, for G1 and G2.  Operands are RAW records: XYZZ points
re-scaled by random Z (ZZ != 1), every coordinate as c or as c + p, infinity as ZZ = 0 and as ZZ = p, the affine infinity as x = y = 0 and
x = y = p; the cases of tests/fp32_ref.py (P + S, P + P, P + (-P), infinity on either side and on both, both orders) hold at least 16
doubling / cancellation pairs for each way the unnormalised differences P and R come out (0 or p; tests/test_fp32_mirror.py asserts it).
Everything is exact: results brought to affine integers equal oracle/pyref.py's ec_add / ec_mul, a result at infinity has ZZ = 0 in
canonical limbs, the four lanes of add_quad agree, and for the single operations the XYZZ limbs equal the mirror's, line by line."""
import functools

import pytest

import fp32_ref as ref
import pyref
from gpu_util import zkg  # noqa: F401

pytestmark = pytest.mark.gpu
GROUPS = pytest.mark.parametrize("group", [0, 1], ids=["g1", "g2"])
MIRROR = {"madd": ref.x_madd, "add": ref.x_add, "add_quad": ref.x_add}


@functools.lru_cache(None)
def values(group):
    """per case the affine values (A, B) its records stand for: computed once, shared by every test"""
    return [(ref.affine_value(group, c.a), ref.affine_value(group, c.bx)) for c in ref.group_cases(group)]


@functools.lru_cache(None)
def expected_sum(group, chain, i):
    A, B = values(group)[i]
    return ref.chain_expected(ref.group_fields(group)[2], A, B, chain)


def check_point(group, rec, exp, tag):
    """a normalised XYZZ record from the GPU against an affine value (None: infinity)"""
    F = ref.group_fields(group)[0]
    assert all(x < F.p for e in rec for x in F.flat(e)), (tag, "not canonical")
    assert ref.affine_value(group, rec) == exp, tag
    if exp is None:
        assert rec[2] == F.zero, (tag, "infinity must leave as ZZ = 0")


@GROUPS
@pytest.mark.parametrize("op", ["madd", "add", "add_quad"])
def test_additions(zkg, group, op):
    F = ref.group_fields(group)[0]
    cases = ref.group_cases(group)
    a = ref.pack_records(F, [c.a for c in cases]); b = ref.pack_records(F, [c.ba if op == "madd" else c.bx for c in cases])
    got = ref.unpack_records(F, zkg.curve_op(group, op, a, b))
    if op == "add_quad":
        for i in range(len(cases)):
            assert got[4 * i] == got[4 * i + 1] == got[4 * i + 2] == got[4 * i + 3], (i, cases[i].kind, "the four lanes differ")
        got = got[::4]
    assert len(got) == len(cases)
    for i, (c, g) in enumerate(zip(cases, got)):
        check_point(group, g, expected_sum(group, 0, i), (op, i, c.kind))
        assert g == ref.x_normalized(F, MIRROR[op](F, c.a, c.ba if op == "madd" else c.bx)), (op, i, c.kind, "limbs differ from the mirror")


@GROUPS
@pytest.mark.parametrize("op", ["madd", "add", "add_quad"])
def test_addition_chains(zkg, group, op):
    """x <- a + b, then x <- 2x + b 1, 5, 16 and 64 times on the device (2x = x + x takes the doubling branch), on four cases of every kind"""
    F = ref.group_fields(group)[0]
    cases = ref.group_cases(group)
    sub = ref.chain_subset(cases)
    a = ref.pack_records(F, [cases[i].a for i in sub]); b = ref.pack_records(F, [cases[i].ba if op == "madd" else cases[i].bx for i in sub])
    for chain in ref.CHAINS[1:]:
        got = ref.unpack_records(F, zkg.curve_op(group, op, a, b, chain=chain))
        if op == "add_quad":
            assert all(got[4 * j] == got[4 * j + 1] == got[4 * j + 2] == got[4 * j + 3] for j in range(len(sub))), (chain, "the four lanes differ")
            got = got[::4]
        for i, g in zip(sub, got):
            check_point(group, g, expected_sum(group, chain, i), (op, chain, i, cases[i].kind))


@GROUPS
def test_doublings_and_to_affine(zkg, group):
    F, E, CF = ref.group_fields(group)
    cases = ref.group_cases(group)
    recs = [c.a for c in cases]; vals = [v[0] for v in values(group)]
    packed = ref.pack_records(F, recs)
    for g, rec, A, c in zip(ref.unpack_records(F, zkg.curve_op(group, "dbl", packed)), recs, vals, cases):
        check_point(group, g, pyref.ec_add(CF, A, A), ("dbl", c.kind))
        assert g == ref.x_normalized(F, ref.x_dbl(F, rec)), ("dbl", c.kind, "limbs differ from the mirror")
    for g, A, c in zip(ref.unpack_records(F, zkg.curve_op(group, "to_affine", packed)), vals, cases):
        assert all(x < F.p for e in g for x in F.flat(e)), ("to_affine", c.kind, "not canonical")
        assert (None if g == (F.zero, F.zero) else (F.value(g[0]), F.value(g[1]))) == A, ("to_affine", c.kind)
    aff = [c.ba for c in cases if c.kind not in ("inf_b", "inf_both")]          # dbl_affine_inl makes no infinity check: its callers do
    for g, b in zip(ref.unpack_records(F, zkg.curve_op(group, "dbl_affine", ref.pack_records(F, aff))), aff):
        B = ref.affine_point_value(group, b)
        check_point(group, g, pyref.ec_add(CF, B, B), "dbl_affine")
        assert g == ref.x_normalized(F, ref.x_dbl_affine(F, b)), ("dbl_affine", "limbs differ from the mirror")


@GROUPS
def test_scalar_multiplication(zkg, group):
    """a.mul(k, 8) with the raw scalars 0, 1, 2, r - 1, r, r + 1, 2^256 - 1 and random 256-bit ones (unreduced: k P = (k mod r) P)"""
    F, E, CF = ref.group_fields(group)
    recs, ks = ref.mul_cases(group)
    k = ref.np.array([ref.limbs32(x) for x in ks], ref.np.uint32)
    got = ref.unpack_records(F, zkg.curve_op(group, "mul", ref.pack_records(F, recs), k=k))
    for g, rec, x in zip(got, recs, ks):
        A = ref.affine_value(group, rec)
        check_point(group, g, pyref.ec_mul(CF, x, A), ("mul", hex(x)))
    assert ref.affine_value(group, got[4]) is None and ref.affine_value(group, got[0]) is None           # r P and 0 P
