"""CPU suite: the reference the GPU test of the multi-exponentiation's 29-bit Fq arithmetic compares with (tests/fq29_ref.py) is itself
checked here — its constants against csrc/fq29.hip.hpp, its column algorithm limb for limb against the interpreted streams on the very
operands the GPU product tests use, its mixed and general additions against affine integer arithmetic on every case family of the GPU
test, and chains of additions from the worst representatives inside every bound the header's comments state — before any of it is used as
a yardstick for the hardware."""
import pytest

import fq29_ref as F
from fq29_ref import Q, M29, limbs9, value


@pytest.fixture(scope="module")
def pts(oracle):
    return F.affine_points(oracle, 1024, F.POINTS_SEED)


def test_constants_match_the_header():
    h = F.header_constants()
    assert h["P"] == F.P and value(F.P) == Q
    assert h["INV"] == F.INV and h["PINV"] == F.PINV and (F.INV * Q + 1) % (1 << 29) == 0 and F.PINV * Q % (1 << 29) == 1
    assert h["ONE"] == limbs9(F.ONE) and h["TO"] == limbs9(F.TO) and h["FROM"] == limbs9(F.FROM) and h["R3"] == limbs9(F.R3)
    assert h["Q30"] == F.Q30 and sum(x << (30 * i) for i, x in enumerate(F.Q30)) == Q and h["Q30_INV"] == F.Q30_INV
    for name, (S, k, d) in F.SPREADS.items():
        assert h[name] == S and value(S) == k * Q and min(S[:8]) >= d * M29 and S[8] >= 0, name


def test_column_mirror_equals_the_interpreted_streams_on_the_gpu_tests_operands():
    """every operand set the GPU product tests compare with fq29_ref.mont / sqr is interpreted instruction by instruction here (the single
    streams on all of them, the interleaved pairs on the first 1024), so that on the GPU the mirror stands for the simulator"""
    for i, (a, b) in enumerate(F.product_operands()):
        assert F.mont(a, b) == F.sim_mul(a, b) == limbs9(F.mont_value(value(a), value(b))), i
    for i, a in enumerate(F.square_operands()):
        assert F.sqr(a) == F.sim_sqr(a) == F.mont(a, a), i
    for i, (a, b, c, d) in enumerate(F.product_quads()[:1024]):
        assert (F.mont(a, b), F.mont(c, d)) == F.sim_mul2(a, b, c, d), i
    for i, (a, c) in enumerate(F.square_pairs()[:1024]):
        assert (F.sqr(a), F.sqr(c)) == F.sim_sqr2(a, c), i


def test_conversions_and_records_round_trip():
    rng = F.Rng(0xC0)
    for v in [0, 1, Q - 1, 1 << 253, (1 << 232) - 1, (1 << 232) + 1, (1 << 29) - 1, 1 << 29] + [rng.below(Q) for _ in range(200)]:
        t = F.to29(F.words8(v))
        assert value(t) % Q == v * 32 % Q and value(t) < 2 * Q and F.is_digits(t)                                # x 2^256 -> x 2^261
        assert F.from29(t) == F.words8(v)
        for j in range(1, 12):
            assert F.from29(limbs9(value(t) + j * Q), F.Bounds()) == F.words8(v)
        assert F.pack8(limbs9(v)) == F.words8(v) and F.unpack8(F.words8(v)) == limbs9(v)
    for x in (0, Q - 1, int(1.01 * Q), 1 << 254):
        for inf in (0, 1):
            assert F.rec64(limbs9(x), limbs9(Q - 1), inf) == (limbs9(x), limbs9(Q - 1), inf)


def test_zero_test_mirror():
    for k in range(16):
        assert F.is_zero_mod_p(limbs9(k * Q), F.Bounds())
        if k:
            for d in (1, -1, 1 << 29, 1 << 232):
                assert not F.is_zero_mod_p(limbs9(k * Q + d))


def test_madd_mirror_is_the_group_law_inside_the_stated_bounds(pts):
    b = F.Bounds()
    cases = F.madd_cases(pts)
    assert len(cases) >= 64 * 20
    for i, (acc, bx, by, inf, want) in enumerate(cases):
        out, oinf, ok = F.madd(acc, bx, by, inf, b)
        assert ok and not oinf and F.is_point(out, want), i
    ks = set()
    for i, (acc, bx, by, inf, want) in enumerate(F.madd_exceptional_cases(pts)):
        info = {}
        out, oinf, ok = F.madd(acc, bx, by, inf, b, info)
        assert not ok and value(info["Pd"]) % Q == 0, i
        ks.add(value(info["Pd"]) // Q)
        assert (oinf and want is None) or (not oinf and F.is_point(out, want)), i
    assert ks >= set(range(1, 7)), ks                          # Pd = k q for every k = 1 .. 6
    print("madd cases:", b.show())


def test_general_addition_mirror_is_the_group_law_and_its_three_forms_agree(pts):
    b = F.Bounds()
    ks = set()
    for i, (x, y, want) in enumerate(F.add_cases(pts)):
        out = F.add_general(x, y, "lane", b)
        assert F.is_point(out, want), i
        assert out == F.add_general(x, y, "pair") == F.add_general(x, y, "quad"), i
        if want is not None and any(x[2]) and any(y[2]) and F.fv(x[0]) * F.fv(y[2]) % Q == F.fv(y[0]) * F.fv(x[2]) % Q:
            pv = F.norm(F.sub(F.mont(y[0], x[2]), F.S2_1, F.mont(x[0], y[2])))
            assert value(pv) % Q == 0
            ks.add(value(pv) // Q)
    assert ks >= {1, 2}, ks                                    # P + P with P = q and P = 2 q
    print("general addition cases:", b.show())


def test_chains_from_the_worst_representatives_stay_inside_the_stated_bounds(pts):
    """64 mixed additions per element, every step re-entered at the largest representatives the invariants admit (X + j q below 5.3 q,
    Y + j q below 3.4 q, ZZ / ZZZ + q below 1.1 q) with by negated on every other element, and 33 rounds of x <- 2x + b (67 general
    additions) from the worst representatives: the mirror asserts every stated range at every operation.  The peaks are printed; the
    comments' figures are Pd < 7.1, Rd < 5.1, X < 5.3, Y < 3.4, ZZ / ZZZ < 1.1 (units of q), T's limbs < 2^30.6, a column < 2^64."""
    b = F.Bounds()
    for i, (a, bb, A, B) in enumerate(F.chain_points(pts, 12)):
        bx, by = F.rep(B[0]), F.rep(B[1])
        if i % 2:
            by = F.neg(F.S2_1, by); B = F.ec_neg(B)
        for lift in (False, True):
            acc, inf, ok = F.madd_chain(a, bx, by, 64, b, lift)
            want = A
            for _ in range(64):
                want = F.ec_add(want, B)
            assert ok and not inf and F.is_point(acc, want), (i, lift)
    print("madd chains:", b.show())
    assert b.peak["Pd"] < 7.1 * Q and b.peak["Rd"] < 5.1 * Q and b.peak["T_limb"] < F.T_LIMB and b.peak["column"] < 1 << 64
    g = F.Bounds()
    for i, (a, bb, A, B) in enumerate(F.chain_points(pts[100:], 6)):
        out = F.add_chain(a, bb, 33, "lane", g)
        assert F.is_point(out, F.add_chain_point(A, B, 33)), i
    print("general addition chains:", g.show())
    assert g.peak["X3"] < 5.3 * Q and g.peak["Y3"] < 3.4 * Q and g.peak["ZZ3"] < 1.1 * Q
