"""CPU suite: the mirror of the 32-bit device layer that tests/test_gpu_fp32.py and tests/test_gpu_curve32.py compare the GPU with
(tests/fp32_ref.py).  The committed streams of csrc/mont_asm.inc, interpreted by tools/gen_mont_asm.py, on every operand family: results
below 2p, congruent to the integer result, add and sub exactly the single fold; the chains composed from the interpreter with every
intermediate below 2p; the conditions the families must meet (sizes, distinctness, the edges they claim, and at least 16 doubling /
cancellation cases for each way the unnormalised differences P and R can come out); the mirror's XYZZ formulas against pyref.ec_add."""
import pytest

import fp32_ref as ref
import pyref
from fp32_ref import FIELDS, M32


@pytest.mark.parametrize("name", ["fq", "fr"])
def test_streams_on_every_family(name):
    fp = FIELDS[name]; p = fp.p
    for fam, (A, B, edge) in ref.field_families(name).items():
        for a, b in zip(A, B):
            t = fp.sim_mul(a, b)
            assert t < 2 * p and t % p == a * b * fp.rinv % p and t == fp.mul(a, b), (fam, "mul", a, b)
            t = fp.sim_mul(a, a)
            assert t < 2 * p and t % p == a * a * fp.rinv % p and t == fp.mul(a, a), (fam, "sqr", a)
            t = fp.sim_add(a, b)
            assert t == (a + b - 2 * p if a + b >= 2 * p else a + b) == fp.add(a, b), (fam, "add", a, b)      # exactly the single fold
            t = fp.sim_sub(a, b)
            assert t == (a - b + 2 * p if a < b else a - b) == fp.sub(a, b), (fam, "sub", a, b)
            t = fp.sim_sub(0, a)
            assert t == (2 * p - a if a else 0), (fam, "neg", a)


@pytest.mark.parametrize("field", [0, 1, 2])
def test_chains_composed_from_the_interpreter(field):
    """ops 40-42 on the interpreter (Lazy asserts every operand and intermediate below 2p), against the closed forms and the integers: every
    eighth element of the edge families (test_streams_on_every_family runs each single operation on all of them), N_SIM of the others"""
    S, E = ref.lazy_field(field, sim=True)
    F, _ = ref.lazy_field(field)
    fams = ref.fq2_families() if field == 2 else ref.field_families("fr" if field == 1 else "fq")
    for fam, idx in ref.sim_indices(fams, thin=8).items():
        A, B, _ = fams[fam]
        for i in idx:
            for op in ("chain40", "chain41", "chain42"):
                got = ref.OPS[op](S, A[i], B[i])
                assert got == ref.OPS[op](F, A[i], B[i]), (fam, op, i)
                assert S.value(got) == ref.OPS[op](E, S.value(A[i]), S.value(B[i])), (fam, op, i)


def test_fq2_mirror_against_pyref():
    S, E = ref.lazy_field(2, sim=True)
    F, _ = ref.lazy_field(2)
    fams = ref.fq2_families()
    for fam, idx in ref.sim_indices(fams).items():
        A, B, _ = fams[fam]
        for i in idx:
            for op in ("mul", "add", "sub", "neg", "sqr", "dbl"):
                got = ref.OPS[op](S, A[i], B[i])
                assert got == ref.OPS[op](F, A[i], B[i]), (fam, op, i)
                assert S.value(got) == ref.OPS[op](E, S.value(A[i]), S.value(B[i])), (fam, op, i)


@pytest.mark.parametrize("name", ["fq", "fr"])
def test_field_family_conditions(name):
    fp = FIELDS[name]; p = fp.p
    fam = ref.field_families(name)
    ve = set(ref.value_edges(p))
    assert {0, 1, p - 1, p, p + 1, 2 * p - 1, (p - 1) // 2, (p + 1) // 2, 1 << 254, (1 << 254) - 1, 1 << 32, (1 << 32) - 1} <= ve and max(ve) < 2 * p
    le = ref.limb_edges(p)
    assert len(le) == len(set(le)) and max(le) < 2 * p
    for top in (0, fp.P[7]):
        assert sum(1 for x in le if x >> 224 == top and all(l in (0, M32) for l in ref.limbs32(x)[:7])) >= 128
    # the largest top limb: one more would reach 2p
    assert sum(1 for x in le if all(l in (0, M32) for l in ref.limbs32(x)[:7]) and x + (1 << 224) >= 2 * p) >= 128
    assert {M32 << (32 * j) for j in range(7)} <= set(le) and {p + 1, p - 1, 2 * p - 1, p + (1 << 224), p - (1 << 224), 2 * p - (1 << 224)} <= set(le)
    A, B, _ = fam["fold_edges"]
    sums, diffs = {a + b for a, b in zip(A, B)}, {a - b for a, b in zip(A, B)}
    assert {2 * p - 1, 2 * p, 2 * p + 1, 4 * p - 2} <= sums and {0, -1, 1, -(2 * p - 1), p, -p} <= diffs
    A, B, _ = fam["product_edges"]
    digits = [fp.quotient_digits(a, b) for a, b in zip(A, B)]
    assert (2 * p - 1, 2 * p - 1) in set(zip(A, B)) and 1 in B and fp.one in B
    for k in range(8):                                       # every column's reduction factor at both ends, and all columns at once
        assert sum(1 for d in digits if d[k] == 0) >= 4 and sum(1 for d in digits if d[k] == M32) >= 4, k
    assert [M32] * 8 in digits and [0] * 8 in digits
    A, B, _ = fam["both_representatives"]
    assert len(A) == 1024 and all(len({(A[i + j] % p, B[i + j] % p) for j in range(4)}) == 1 for i in range(0, 1024, 4))
    assert all({(A[i + j] >= p, B[i + j] >= p) for j in range(4)} == {(x, y) for x in (False, True) for y in (False, True)} for i in range(0, 1024, 4))
    A, B, _ = fam["random"]
    assert len(A) == 2048 and len(set(A)) == 2048 and len(set(B)) == 2048
    assert ref.field_families(name) is fam                  # one fixed family per session (seeded, cached)


@pytest.mark.parametrize("group", [0, 1])
def test_group_family_conditions(group):
    """at least 16 doubling / cancellation cases for each of: P raw = 0, P raw = p, R raw = 0, R raw = p — for madd and for add (add_quad
    forms the same four products), in G1 and per Fq2 component in G2, where a zero of mixed representatives (0, p) must occur as well.
    The raw differences come from the interpreted streams."""
    cases = ref.group_cases(group)
    assert len(cases) <= 512
    kinds = {}
    for c in cases:
        kinds[c.kind] = kinds.get(c.kind, 0) + 1
    assert set(kinds) == {"general", "double", "cancel", "inf_a", "inf_b", "inf_both"}
    F = ref.group_fields(group)[0]
    p = F.p
    flat = lambda rec: [x for e in rec for x in F.flat(e)]
    assert all(x < 2 * p for c in cases for rec in (c.a, c.bx, c.ba) for x in flat(rec))
    assert any(all(x >= p for x in flat(c.a)) for c in cases) and any(all(x < p for x in flat(c.a)) for c in cases)
    assert any(c.kind == "inf_a" and all(z == p for z in F.flat(c.a[2])) for c in cases), "the XYZZ infinity with ZZ = p"
    assert any(c.kind == "inf_b" and all(z == p for z in flat(c.ba)) for c in cases), "the affine infinity x = y = p"
    assert all(F.norm(c.a[2]) != F.one for c in cases if c.kind == "general"), "ZZ != 1"
    for op in ("madd", "add"):
        census = ref.difference_census(group, op)
        for key in ref.census_keys(group):
            assert census.get(key, 0) >= 16, (op, key, census)


@pytest.mark.parametrize("group", [0, 1])
def test_group_mirror_against_pyref(group):
    """the mirror's XYZZ formulas (madd, add, dbl, dbl_affine) on every case, brought to affine values, against pyref.ec_add"""
    F, E, CF = ref.group_fields(group)
    for i, c in enumerate(ref.group_cases(group)):
        A, B = ref.affine_value(group, c.a), ref.affine_value(group, c.bx)
        assert B == ref.affine_point_value(group, c.ba), i
        exp = pyref.ec_add(CF, A, B)
        assert ref.affine_value(group, ref.x_madd(F, c.a, c.ba)) == exp, (i, c.kind, "madd")
        assert ref.affine_value(group, ref.x_add(F, c.a, c.bx)) == exp, (i, c.kind, "add")
        assert ref.affine_value(group, ref.x_dbl(F, c.a)) == pyref.ec_add(CF, A, A), (i, c.kind, "dbl")
        if B is not None:
            assert ref.affine_value(group, ref.x_dbl_affine(F, c.ba)) == pyref.ec_add(CF, B, B), (i, c.kind, "dbl_affine")
            assert pyref.on_curve(CF, B)
