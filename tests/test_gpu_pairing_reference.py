"""GPU suite: the device pairing against the independent reference of oracle/pyref.py (polynomial Fq12, affine Miller loop, one pow), exactly.
The tower's operations are fed raw limbs at the bounds of the lazy range [0, 2q) through zkg_fq12_op(where=1); the final exponentiation
kernel, the Miller kernel with both product paths and the two batch verifiers are compared with the reference's values, which come from
tests/golden/pairing.json (the reference's known-answer record, re-derived in tests/test_oracle_golden.py) or are computed once per module.
There is no tolerance anywhere: raw outputs are compared modulo q together with the range invariant, everything else byte for byte."""
import random

import numpy as np
import pytest

import fq12_ref as F
import pyref as P
from gpu_util import zkg  # noqa: F401
from r1cs_util import golden_case_arrays
from test_final_exp_host import ONE, final_exp_inputs
from test_verifier import CASES, build_vk
from util import Q, arr, golden, h

pytestmark = pytest.mark.gpu

GOLD = golden("pairing.json")


# ---- 1. the tower at the bounds of the lazy range ----------------------------------------------------------------------------------
START = {1: 40, 64: 1, 65: 0}                            # which lanes of the 65-element pools a shape takes: one, a full wavefront, 64 + 1


@pytest.fixture(scope="module")
def pools():
    return dict(a=F.lazy_pool(0xA0), b=F.lazy_pool(0xB0)[::-1], line=F.line_pool(0xC0))


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("op", [o for o in F.OPS if o != "cyclotomic_sqr"])
def test_tower_operation_at_the_lazy_bounds(zkg, pools, op, n):
    s = START[n]
    a = pools["a"][s:s + n]
    b = {"mul": pools["b"], "mul_by_line2": pools["line"]}.get(op)
    b = None if b is None else b[s:s + n]
    out = zkg.fq12_op(op, F.words(a), None if b is None else F.words(b))
    got = F.check_outputs(op, a, b, out, lazy=True)
    # the same values written with the other representative of every coefficient: the same results modulo q
    a2 = [F.other_representative(e) for e in a]
    b2 = None if b is None else [F.other_representative(e[:6]) + e[6:] if op == "mul_by_line2" else F.other_representative(e) for e in b]
    out2 = zkg.fq12_op(op, F.words(a2), None if b2 is None else F.words(b2))
    assert F.check_outputs(op, a2, b2, out2, lazy=True) == got
    if op.startswith("frobenius") and n == 65:           # whole elements against pow(x, q^k) itself, not through its linearity
        for t in (0, 5, 30, 64):
            assert got[t] == P.frobenius_ref(F.raw_to_poly(a[t]), int(op[-1])), t


@pytest.fixture(scope="module")
def cyclotomic():
    return F.cyclotomic_pool(0xD0)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_cyclotomic_squaring_at_the_lazy_bounds(zkg, cyclotomic, n):
    """inputs from the cyclotomic subgroup only (the operation is not specified outside it), some coefficients written as value + q:
    the result is the plain square"""
    s = START[n]
    polys = cyclotomic[s:s + n]
    canon = [F.poly_to_raw(p) for p in polys]
    lazy = F.lazy_representatives(polys, 0xD1)
    assert lazy != canon or n == 1
    got = F.check_outputs("cyclotomic_sqr", lazy, None, zkg.fq12_op("cyclotomic_sqr", F.words(lazy)), lazy=True)
    assert got == [P.p_mul(p, p) for p in polys]
    for raws in (canon, [F.other_representative(e) for e in canon]):
        assert F.check_outputs("cyclotomic_sqr", raws, None, zkg.fq12_op("cyclotomic_sqr", F.words(raws)), lazy=True) == got


def test_tower_hook_arguments(zkg):
    a = F.words(F.lazy_pool(0xA0)[:2])
    assert zkg.fq12_op("sqr", np.zeros((0, 96), np.uint32)).shape == (0, 96)
    with pytest.raises(zkg.ZkgError):
        zkg.fq12_op("sqr", a, where=0)
    import ctypes as C
    L = zkg.lib()
    L.zkg_fq12_op.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out = np.zeros((2, 96), np.uint32); p = lambda x: x.ctypes.data_as(C.c_void_p)       # noqa: E731
    assert L.zkg_fq12_op(10, p(a), p(a), 2, 1, p(out)) == zkg.ERROR and L.zkg_fq12_op(0, p(a), None, 2, 1, p(out)) == zkg.ERROR
    assert L.zkg_fq12_op(1, p(a), None, (1 << 20) + 1, 1, p(out)) == zkg.ERROR and not out.any()


# ---- 2. the final exponentiation kernel --------------------------------------------------------------------------------------------
def test_final_exp_on_the_device_equals_the_reference(zkg):
    pool = final_exp_inputs()
    ref = [P.ser_gt(P.final_exp_ref(P.parse_gt(v))) for v in pool]            # 18 pows
    assert len(pool) == 18 and len(set(pool)) == 18
    vals = [pool[i % 18] for i in range(65)]             # no two adjacent lanes hold the same value
    got = zkg.final_exp(vals, 1)
    for i, g in enumerate(got):
        assert g == ref[i % 18], i
    assert ref[0] == ONE
    # and the recorded known answers
    rec = GOLD["final_exp"]
    assert zkg.final_exp([bytes.fromhex(c["in_hex"]) for c in rec], 1) == [bytes.fromhex(c["out_hex"]) for c in rec]


# ---- 3. single pairings and products -----------------------------------------------------------------------------------------------
def g1_limbs(p):
    return np.zeros(8, np.uint64) if p is None else arr([p[0], p[1]], Q).reshape(8)


def g2_limbs(s):
    return np.zeros(16, np.uint64) if s is None else arr([s[0][0], s[0][1], s[1][0], s[1][1]], Q).reshape(16)


@pytest.fixture(scope="module")
def records():
    """the recorded reference pairings with their points, which pyref computes itself (not the library's fixed-base kernel): the inputs are
    independent too"""
    out = []
    for c in GOLD["pairing"]:
        a, b = h(c["a"]), h(c["b"])
        p, s = P.g1_mul(a), P.g2_mul(b)
        out.append(dict(a=a, b=b, P=g1_limbs(p), Q=g2_limbs(s), gt=bytes.fromhex(c["gt_hex"])))
    assert P.g1_mul(out[0]["a"]) == (1, 2) and P.g1_mul(out[4]["a"]) == (1, Q - 2)         # G1 itself and -G1
    return out


def test_single_pairings_equal_the_reference(zkg, records):
    for r in records:
        assert zkg.pairing_product(r["P"][None], r["Q"][None]) == r["gt"], (hex(r["a"]), hex(r["b"]))
    got = zkg.pairing_each(np.array([r["P"] for r in records]), np.array([r["Q"] for r in records]), 1)
    assert got == [r["gt"] for r in records]
    inf = [r for r in records if r["a"] == 0 or r["b"] == 0]
    assert len(inf) == 2 and all(r["gt"] == ONE for r in inf) and sum(r["gt"] == ONE for r in records) == 2
    assert not inf[0]["P"].any() and inf[0]["Q"].any() and inf[1]["P"].any() and not inf[1]["Q"].any()


@pytest.fixture(scope="module")
def pool8(records):
    """eight reference pairings, none of them 1, as (points, polynomial)"""
    pick = [r for r in records if r["gt"] != ONE][:4] + records[-4:]
    assert len({r["gt"] for r in pick}) == 8
    return [(r["P"], r["Q"], P.parse_gt(r["gt"])) for r in pick]


@pytest.mark.parametrize("items", [1, 2, 65])
def test_pairing_each_products_equal_the_reference(zkg, pool8, items):
    rng = random.Random(0xEAC4 + items)
    choice = [rng.sample(range(8), 3) for _ in range(items)]                   # a seeded arrangement per item
    assert all(x != y for x, y in zip(choice, choice[1:]))
    g1 = np.array([pool8[k][0] for c in choice for k in c]); g2 = np.array([pool8[k][1] for c in choice for k in c])
    got = zkg.pairing_each(g1, g2, 3)
    for i, c in enumerate(choice):
        assert got[i] == P.ser_gt(P.p_mul(P.p_mul(pool8[c[0]][2], pool8[c[1]][2]), pool8[c[2]][2])), (i, c)


@pytest.mark.parametrize("n", [127, 128, 130])
def test_pairing_product_equals_the_reference(zkg, pool8, n):
    """k_fq12_prod runs one block up to 127 values and from 128 on (n / 64 >= 2) several blocks and a second launch that folds them;
    130 splits unevenly over the lanes"""
    rng = random.Random(0x9D0D + n)
    idx = [rng.randrange(8) for _ in range(n)]
    acc = P.P_ONE
    for k in idx:
        acc = P.p_mul(acc, pool8[k][2])
    got = zkg.pairing_product(np.array([pool8[k][0] for k in idx]), np.array([pool8[k][1] for k in idx]))
    assert got == P.ser_gt(acc) and acc != P.P_ONE


# ---- 4. end to end: keys whose alpha_g1_beta_g2 comes from the reference -----------------------------------------------------------
def reference_gt(alpha, beta):
    return P.ser_gt(P.pairing(P.g1_mul(alpha), P.g2_mul(beta)))


@pytest.mark.parametrize("case", CASES[:2], ids=[c["tag"] for c in CASES[:2]])
def test_verifiers_accept_a_key_with_the_reference_pairing(zkg, oracle, case):
    keep = []
    vk, x = build_vk(oracle, case, keep, gt_source=reference_gt)
    proof = bytes.fromhex(case["proof_hex"])
    bad = bytearray(vk); bad[32 * 7] ^= 1                # another GT value: the key is still well formed
    items = [(vk, x, proof), (bytes(bad), x, proof)]
    single = [zkg.groth16_verify(*it) for it in items]
    assert single == [0, 1]
    assert list(zkg.groth16_verify_each(items)) == single
    assert list(zkg.groth16_verify_batch(items)) == single                    # the documented contract: the single verifier's verdict
    # the key zkg_groth16_setup itself issues starts with the reference's 384 bytes
    A, B, C, pts, w, r, s = golden_case_arrays(case)
    cs = zkg.make_r1cs(case["num_variables"], case["num_inputs"], A, B, C, keep)
    kp = zkg.Keypair(cs, arr([h(case["trapdoor"][k]) for k in ("t", "alpha", "beta", "gamma", "delta")]))
    try:
        issued = kp.vk_blob()
    finally:
        kp.free()
    assert issued[:384] == vk[:384] == reference_gt(h(case["trapdoor"]["alpha"]), h(case["trapdoor"]["beta"]))
