"""CPU suite: the reference the GPU test of the NTT's 29-bit Fr arithmetic compares with (tests/fr29_ref.py) is itself checked here — its
constants against csrc/fr29.hip.hpp, its column algorithm limb for limb against the interpreted streams, and the 14-step chain of radix-4
steps inside every bound the code's comments state, before any of it is used as a yardstick for the hardware."""
import fr29_ref as F
from fr29_ref import R, M29, P, S2_1, limbs9, value, data_side_cases, table_side_cases


def test_constants_match_the_header():
    h = F.header_constants()
    assert h["P"] == P and value(P) == R
    assert h["ONE"] == limbs9(F.ONE)
    assert h["S2_1"] == S2_1 and value(S2_1) == 2 * R and min(S2_1[:8]) >= M29


def test_column_mirror_equals_the_interpreted_streams():
    rng = F.Rng(0x29)
    a = data_side_cases(rng, 160); b = table_side_cases(rng, 160)
    b = b[:3] * 4 + b[3:]                                             # the table edges against the data edges too
    for i, x in enumerate(a):
        y = b[(i * 7) % len(b)]
        t = F.mont(x, y)
        assert t == F.sim_mul(x, y), i
        assert value(t) % R == value(x) * value(y) * F.RHO % R and value(t) < 2 * R and max(t[:8]) <= M29
    for i in range(0, 80, 2):
        r0, r1 = F.sim_mul2(a[i], b[i], a[i + 1], b[i + 1])
        assert r0 == F.mont(a[i], b[i]) and r1 == F.mont(a[i + 1], b[i + 1]), i


def test_column_mirror_equals_the_interpreted_streams_on_the_gpu_tests_operands():
    """every operand pair the GPU product test compares with fr29_ref.mont is interpreted instruction by instruction here (the single
    stream on all 4096, the interleaved pair on the first 1024 quads), so that on the GPU mont stands for the simulator"""
    for i, (x, y) in enumerate(F.product_operands()):
        assert F.mont(x, y) == F.sim_mul(x, y), i
    for i, (a, b, c, d) in enumerate(F.product_quads()[:1024]):
        assert (F.mont(a, b), F.mont(c, d)) == F.sim_mul2(a, b, c, d), i


def test_radix4_step_and_tail_are_the_two_stage_butterfly():
    rng = F.Rng(0x44)
    for i in range(60):
        x = [limbs9(rng.below(50 * R)) for _ in range(4)]
        wa, wb, wc = (limbs9(rng.below(R)) for _ in range(3))
        small = [limbs9(value(v) % (2 * R - (1 << 232))) for v in x]    # a stage without a product takes its subtrahends as they are: below 2r - 2^232
        for product, ns in ((True, False), (False, False), (True, True), (False, True)):
            xs = x if product else small
            o = [value(v) % R for v in F.r4_step(*xs, wa, wb, wc, product, ns, F.Bounds())]
            a = value(wa) * F.RHO % R if product else 1
            b, c = value(wb) * F.RHO % R, value(wc) * F.RHO % R
            v0, v1, v2, v3 = (value(v) for v in xs)
            assert o == [(v0 + a * v1 + b * (v2 + a * v3)) % R, (v0 - a * v1 + c * (v2 - a * v3)) % R,
                         (v0 + a * v1 - b * (v2 + a * v3)) % R, (v0 - a * v1 - c * (v2 - a * v3)) % R], (i, product, ns)
        for product in (True, False):
            xs = x if product else small
            o = [value(v) % R for v in F.r2_tail_step(xs[0], xs[1], wa, product, F.Bounds())]
            a = value(wa) * F.RHO % R if product else 1
            assert o == [(value(xs[0]) + a * value(xs[1])) % R, (value(xs[0]) - a * value(xs[1])) % R]


def test_chain_of_14_steps_stays_inside_the_stated_bounds():
    """28 stages from the all-maximal digits with twiddles picked to keep the products large: the mirror asserts at every operation that no
    limb leaves 32 bits, every product's data operand has limbs below 2.5 x 2^30 and a value below 60 r, and every subtrahend's top limb
    stays below S2_1's.  The peaks: limbs stay below 2.5 x 2^30 and the values below 40 r (a product is below 1.36 r, not 2 r, so row 0
    gains at most 2.72 r per step)."""
    for ns in (False, True):
        b = F.run_chain(48, 0x5A4B0029, ns)
        print("norm_stores", ns, {k: (f"{v / R:.2f} r" if k == "data_value" else hex(v)) for k, v in b.peak.items()})
        assert b.peak["limb"] < F.LAZY_LIMB and b.peak["data_value"] < 40 * R
