"""CPU suite: the pairing pinned to an independent reference.  oracle/pyref.py's pairing is plain integers from the definition (Fq12 as
polynomials modulo w^12 - 18 w^6 + 82, an affine Miller loop, one pow for the final exponentiation); it is checked here against
mathematics alone, and then the host pairing (zkg_pairing_probe), both final exponentiations that run without a GPU (zkg_final_exp,
where 0 and 2), the device tower compiled for the host (zkg_fq12_op, where 2) and a verification key's first 384 bytes are compared with
it, byte for byte.  The GPU side of the same comparison is tests/test_gpu_pairing_reference.py."""
import random

import numpy as np
import pytest

import fq12_ref as F
import pyref as P
import zklaim_amd as zkg
from test_final_exp_host import final_exp_inputs
from test_verifier import CASES, build_vk
from util import Q, R, golden, h, limbs

GOLD = golden("pairing.json")
SCALARS = [(h(c["a"]), h(c["b"])) for c in GOLD["pairing"]]


@pytest.fixture(scope="module")
def lib():
    from zklaim_amd import build
    build.build()
    return zkg


@pytest.fixture(scope="module")
def ref_pairings():
    """the reference pairing of every scalar pair, from points the reference computed itself"""
    return {(a, b): P.pairing(P.g1_mul(a), P.g2_mul(b)) for a, b in SCALARS}


# ---- 1. the reference against mathematics only ------------------------------------------------------------------------------------
def test_reference_field_is_a_field_extension_of_the_tower():
    """w^6 = 9 + u with u^2 = -1, the conjugation and the Frobenius helper of fq12_ref against pow itself"""
    w6 = P.p_pow([0, 1] + [0] * 10, 6)
    u = [(c - 9) % Q if i == 0 else c for i, c in enumerate(w6)]
    assert P.p_mul(u, u) == [Q - 1] + [0] * 11
    assert P.p_from_f2((0, 1), 0) == u and P.p_from_f2((5, 7), 3) == P.p_mul(P.p_add([5] + [0] * 11, [7 * c % Q for c in u]), [0, 0, 0, 1] + [0] * 8)
    rng = random.Random(0xF1E1D)
    x = [rng.randrange(Q) for _ in range(12)]
    assert P.p_mul(x, P.p_inv(x)) == P.P_ONE
    assert F.conj_poly(x) == P.frobenius_ref(x, 6)
    for k in (1, 2, 3):
        assert F.frobenius_poly(x, k) == P.frobenius_ref(x, k)
    assert P.parse_gt(P.ser_gt(x)) == x and F.raw_to_poly(F.poly_to_raw(x)) == x
    assert F.raw_to_poly(F.other_representative(F.poly_to_raw(x))) == x


def test_reference_pairing_is_bilinear_of_order_r_and_nondegenerate(ref_pairings):
    e11 = ref_pairings[(1, 1)]
    assert e11 != P.P_ONE and P.p_pow(e11, R) == P.P_ONE
    for (a, b), e in ref_pairings.items():
        assert e == P.p_pow(e11, a * b % R), (a, b)                           # e(aP, bQ) = e(P, Q)^(ab), by the reference's own product and pow
    assert ref_pairings[(0, 5)] == P.P_ONE == ref_pairings[(5, 0)]
    assert P.p_mul(ref_pairings[(R - 1, 1)], e11) == P.P_ONE                  # P = -G1 = (1, q - 2)
    assert P.g1_mul(R - 1) == (1, Q - 2) and P.g1_mul(1) == (1, 2)


def test_reference_pairing_is_the_cofactor_power_of_the_ate_pairing():
    """which of the valid pairings is meant: libff's last chunk raises to 2z(6z^2 + 3z + 1) times the exact hard exponent
    (test_verifier.py's pairing_selfcheck(hard) == 16 is the library's side of the same statement)"""
    z = P.ATE_Z
    assert 36 * z**4 + 36 * z**3 + 24 * z**2 + 6 * z + 1 == Q and 36 * z**4 + 36 * z**3 + 18 * z**2 + 6 * z + 1 == R
    assert P.GT_COFACTOR == 2 * z * (6 * z * z + 3 * z + 1) and P.GT_COFACTOR % R != 0 and (Q ** 12 - 1) % R == 0
    p, s = P.g1_mul(2), P.g2_mul(3)
    ate = P.pairing(p, s, cofactor=1)
    full = P.pairing(p, s)
    assert full == P.p_pow(ate, P.GT_COFACTOR) and full != ate and ate != P.P_ONE and P.p_pow(ate, R) == P.P_ONE


def test_reference_frobenius_addends_are_on_the_twist():
    for k in (1, 5, R - 2):
        s = P.g2_mul(k)
        q1, q2 = P.miller_addends(s)
        assert P.on_curve(P.Field2, q1) and P.on_curve(P.Field2, q2) and q1 != s and q2 != s
        assert P.ec_mul(P.Field2, R, q1) is None and P.ec_mul(P.Field2, R, q2) is None      # and in G2
        # pi(Q) = [q]Q on G2 (the trace-zero subgroup): the addends are q Q and -q^2 Q
        assert q1 == P.g2_mul(Q % R, s) and q2 == P.ec_neg(P.Field2, P.g2_mul(Q * Q % R, s))


# ---- 2. the host pairing against the reference ------------------------------------------------------------------------------------
def test_scalars_cover_the_named_cases():
    want = {(a, b) for a in (1, 2, R - 1, R - 2) for b in (1, R - 1)} | {(0, 5), (5, 0)}
    assert want <= set(SCALARS) and len(set(SCALARS) - want) == 4


def test_pairing_probe_equals_the_reference(lib, ref_pairings):
    for (a, b), e in ref_pairings.items():
        assert lib.pairing_probe(limbs(a), limbs(b)) == P.ser_gt(e), (hex(a), hex(b))


@pytest.fixture(scope="module")
def fe_reference():
    vals = final_exp_inputs()
    return vals, [P.ser_gt(P.final_exp_ref(P.parse_gt(v))) for v in vals]


@pytest.mark.parametrize("where", [0, 2])
def test_final_exp_equals_the_reference(lib, fe_reference, ref_pairings, where):
    vals, ref = fe_reference
    got = lib.final_exp(vals, where)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g == r, k
    # the reference's own Miller value of one pair, before the final exponentiation: the result is the reference pairing
    a, b = SCALARS[-1]
    f = P.miller(P.g1_mul(a), P.g2_mul(b))
    assert lib.final_exp([P.ser_gt(f)], where) == [P.ser_gt(ref_pairings[(a, b)])]


# ---- 3. the device tower compiled for the host, on the canonical subset ------------------------------------------------------------
def canonical(raws):
    return [[c % Q for c in e] for e in raws]


@pytest.mark.parametrize("op", [o for o in F.OPS if o != "cyclotomic_sqr"])
def test_tower_operation_on_the_host_equals_the_reference(lib, op):
    """zkg_fq12_op(where=2): the text the kernels run, on canonical values.  A failure here is in the text, not in the lazy range."""
    a = canonical(F.lazy_pool(0xA0))
    b = None
    if op == "mul":
        b = canonical(F.lazy_pool(0xB0))[::-1]
    elif op == "mul_by_line2":
        b = canonical(F.line_pool(0xC0))
    out = lib.fq12_op(op, F.words(a), None if b is None else F.words(b), where=2)
    F.check_outputs(op, a, b, out, lazy=False)
    if op.startswith("frobenius"):                       # whole elements against pow(x, q^k) itself
        for t in (7, 20, 64):
            assert F.raw_to_poly(F.unwords(out[t:t + 1])[0]) == P.frobenius_ref(F.raw_to_poly(a[t]), int(op[-1])), t
    # one element at a time gives the same
    assert np.array_equal(lib.fq12_op(op, F.words(a[20:21]), None if b is None else F.words(b[20:21]), where=2), out[20:21])


def test_cyclotomic_squaring_on_the_host_equals_the_reference(lib):
    polys = F.cyclotomic_pool(0xD0)
    a = [F.poly_to_raw(p) for p in polys]
    assert all(P.p_mul(p, F.conj_poly(p)) == P.P_ONE for p in polys[:4])      # x^(q^6) = x^-1 there
    F.check_outputs("cyclotomic_sqr", a, None, lib.fq12_op("cyclotomic_sqr", F.words(a), where=2), lazy=False)


def test_tower_hook_refuses_what_it_cannot_run(lib):
    a = F.words(canonical(F.lazy_pool(0xA0))[:2])
    with pytest.raises(lib.ZkgError):
        lib.fq12_op("mul", F.words([[Q] * 12]), F.words([[1] * 12]), where=2)   # a coefficient >= q on the host build
    with pytest.raises(lib.ZkgError):
        lib.fq12_op("mul", a, F.words([[1] * 12, [0] * 11 + [Q]]), where=2)
    line = [1] * 6 + [2 * Q - 1] * 6                    # the words behind the line are not read, whatever they hold
    assert lib.fq12_op("mul_by_line2", a[:1], F.words([line]), where=2).shape == (1, 96)
    with pytest.raises(lib.ZkgError):
        lib.fq12_op("mul_by_line2", a[:1], F.words([[1] * 5 + [Q] + [0] * 6]), where=2)
    with pytest.raises(lib.ZkgError):
        lib.fq12_op("sqr", a, where=0)
    with pytest.raises(lib.ZkgError):
        lib.fq12_op("sqr", a, where=3)
    L = lib.lib()
    import ctypes as C
    L.zkg_fq12_op.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out = np.zeros((2, 96), np.uint32); p = lambda x: x.ctypes.data_as(C.c_void_p)       # noqa: E731
    assert L.zkg_fq12_op(10, p(a), p(a), 2, 2, p(out)) == lib.ERROR and L.zkg_fq12_op(-1, p(a), p(a), 2, 2, p(out)) == lib.ERROR
    assert L.zkg_fq12_op(0, p(a), None, 2, 2, p(out)) == lib.ERROR and L.zkg_fq12_op(1, None, None, 2, 2, p(out)) == lib.ERROR
    assert L.zkg_fq12_op(1, p(a), None, 2, 2, None) == lib.ERROR
    assert L.zkg_fq12_op(1, p(a), None, (1 << 20) + 1, 2, p(out)) == lib.ERROR             # refused before anything is read
    assert L.zkg_fq12_op(1, None, None, 0, 2, None) == lib.OK
    assert lib.fq12_op("sqr", np.zeros((0, 96), np.uint32), where=2).shape == (0, 96)


def test_tower_hook_on_the_device_needs_a_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(lib.ZkgError):
        lib.fq12_op("sqr", F.words([[1] * 12]), where=1)
    with pytest.raises(lib.ZkgError):
        lib.fq12_op("sqr", np.zeros((0, 96), np.uint32), where=1)


# ---- 4. a verification key whose first 384 bytes come from the reference ----------------------------------------------------------
def reference_gt(alpha, beta):
    return P.ser_gt(P.pairing(P.g1_mul(alpha), P.g2_mul(beta)))


@pytest.mark.parametrize("case", CASES[:2], ids=[c["tag"] for c in CASES[:2]])
def test_a_key_with_the_reference_pairing_verifies(oracle, lib, case):
    keep = []
    vk, x = build_vk(oracle, case, keep, gt_source=reference_gt)
    assert vk[:384] == reference_gt(h(case["trapdoor"]["alpha"]), h(case["trapdoor"]["beta"]))
    proof = bytes.fromhex(case["proof_hex"])
    assert lib.groth16_verify(vk, x, proof) == 0
    assert vk == build_vk(oracle, case, keep)[0]                              # the key the library's own pairing gives: the same bytes
    for pos in (0, 160, 352):                                                 # another GT value: well formed, and the proof fails
        bad = bytearray(vk); bad[pos] ^= 1
        assert lib.groth16_verify(bytes(bad), x, proof) == 1, pos
