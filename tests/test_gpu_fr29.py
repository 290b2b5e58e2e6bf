"""GPU known-answer test of the NTT's 29-bit Fr arithmetic (zklaim_amd/csrc/fr29.hip.hpp) through zkg_fr29_op, on raw limbs: the
generated product streams, the lazy limb-wise operations, the conversions, and the radix-4 step and odd-R tail of k_ntt_pass29_r4 (the
hook's marked copy of the kernel's step bodies), with limbs placed AT the lazy bounds — which a transform of random values reaches with probability
2^-29 per limb.  References, both CPU-only (tests/fr29_ref.py, itself checked by tests/test_fr29_mirror.py): plain Python integers on
value(l) = sum l_i 2^(29 i), and tools/gen_mont_asm.py's interpreter on the very streams.  Everything is limb-exact; no tolerances."""
import numpy as np
import pytest

import fr29_ref as F
from fr29_ref import R, M29, M32, S2_1, limbs9, value
from gpu_util import zkg  # noqa: F401

pytestmark = pytest.mark.gpu

N = F.N_PRODUCTS            # elements per launch
N_SIM = 768                 # ... of which this many (the edges and every family) are interpreted instruction by instruction here (2 ms each); the CPU
#                             suite interprets ALL of the mul operands and the first 1024 mul2 quads against fr29_ref.mont (tests/test_fr29_mirror.py)


def u32(x):
    return np.array(x, dtype=np.uint32)


def rows(a):
    return [[int(v) for v in r] for r in a]


def check_product(t, a, b, tag):
    assert value(t) % R == value(a) * value(b) * F.RHO % R and value(t) < 2 * R and max(t[:8]) <= M29, tag


def test_mul_vs_simulator_and_integers(zkg):
    pairs = F.product_operands()
    got = rows(zkg.fr29_op("mul", u32([[a, b] for a, b in pairs]))[:, 0])
    for i, (a, b) in enumerate(pairs):
        assert got[i] == F.mont(a, b), i
        check_product(got[i], a, b, i)
        if i < N_SIM:
            assert got[i] == F.sim_mul(a, b), i


def test_mul2_vs_simulator_and_integers(zkg):
    quads = F.product_quads()
    got = zkg.fr29_op("mul2", u32(quads))
    for i, (a, b, c, d) in enumerate(quads):
        g0, g1 = rows(got[i])
        assert g0 == F.mont(a, b) and g1 == F.mont(c, d), i
        check_product(g0, a, b, i); check_product(g1, c, d, i)
        if i < N_SIM // 2:
            assert (g0, g1) == F.sim_mul2(a, b, c, d), i


T_MAX = [M29] * 8 + [S2_1[8]]                                    # the largest subtrahend the spread of 2r covers


def lazy_operands():
    """(u, t): u digits or lazy limbs (two lazy stages: up to 2^31 above a digit), t digits whose top limb stays below S2_1's —
    with u = 0, t = 0, t at its maximum, and t = 2r - 2^232 - 1 (the bound sub_norm's comment states)"""
    rng = F.Rng(0x1A27)
    us = [[0] * 9, list(F.ALL_MAX), [M29] * 8 + [0], [x + (1 << 31) for x in F.ALL_MAX[:8]] + [F.ALL_MAX[8]]]
    ts = [[0] * 9, list(T_MAX), limbs9(2 * R - (1 << 232) - 1), limbs9(R - 1), limbs9(1)]
    out = [(u, t) for u in us for t in ts]
    while len(out) < N:
        u = limbs9(rng.below(58 * R)); t = limbs9(rng.below(2 * R - (1 << 232)))
        if len(out) % 2:
            u = [x + rng.choice((0, 1 << 29, 1 << 30, 3 << 29, 1 << 31)) if i < 8 else x for i, x in enumerate(u)]
        out.append((u, t))
    return out


def test_lazy_additions_and_subtractions(zkg):
    ops = lazy_operands()
    x = u32([[u, t] for u, t in ops])
    add, sub = rows(zkg.fr29_op("add_lazy", x)[:, 0]), rows(zkg.fr29_op("sub_lazy", x)[:, 0])
    b = F.Bounds()
    for i, (u, t) in enumerate(ops):
        assert add[i] == F.add_lazy(u, t, b) == [p + q for p, q in zip(u, t)], i
        assert sub[i] == F.sub_lazy(u, t, b) == [p + s - q for p, s, q in zip(u, S2_1, t)], i       # no limb borrows: the spread covers t
        assert value(add[i]) == value(u) + value(t) and value(sub[i]) == value(u) + 2 * R - value(t)
    assert sub[0] == S2_1 and sub[1] == [s - q for s, q in zip(S2_1, T_MAX)] and sub[1][8] == 0          # u = 0: the spread itself, and all of it used
    # digits in, digits out: the carried forms
    dig = [(limbs9(value(u) % (58 * R)) if max(u[:8]) > M29 else u, t) for u, t in ops]
    x = u32([[u, t] for u, t in dig])
    addn, subn = rows(zkg.fr29_op("add_norm", x)[:, 0]), rows(zkg.fr29_op("sub_norm", x)[:, 0])
    for i, (u, t) in enumerate(dig):
        assert addn[i] == F.add_norm(u, t, b) == limbs9(value(u) + value(t)), i
        assert subn[i] == F.sub_norm(u, t, b) == limbs9(value(u) + 2 * R - value(t)), i


def test_norm_preserves_the_value_and_returns_digits(zkg):
    rng = F.Rng(0x9027)
    top = (1 << 32) - 8                                            # a limb plus the carry into it (at most 7) must not wrap
    cases = [[0] * 9, [top] * 9, [M32] + [top] * 8, [M32] + [0] * 8, [M29] * 9, [(5 << 29) - 1] * 8 + [1 << 27]]
    while len(cases) < N:
        k = len(cases) % 3
        cases.append([rng.below(top + 1) for _ in range(9)] if k == 0 else
                     [x + rng.choice((0, 1 << 30, 3 << 29, 1 << 31)) if i < 8 else x for i, x in enumerate(limbs9(rng.below(60 * R)))] if k == 1 else
                     [rng.choice((0, 1, M29, 1 << 29, top, top - 1)) for _ in range(9)])
    # (beyond that bound norm is out of contract: the carry into a limb at 2^32 - 1 wraps it.  Not pinned here.)
    got = rows(zkg.fr29_op("norm", u32([[c] for c in cases]))[:, 0])
    b = F.Bounds()
    for i, a in enumerate(cases):
        assert got[i] == F.norm(a, b), i
        assert value(got[i]) == value(a) and max(got[i][:8]) <= M29, i


def test_slice_and_unslice_reduce(zkg):
    rng = F.Rng(0x511CE)
    canon = [0, 1, R - 1, 1 << 253, (1 << 232) - 1, (1 << 232) + 1, 1 << 232, (1 << 29) - 1, 1 << 29, (1 << 253) - 1]
    canon += [rng.below(R) for _ in range(N - len(canon))]
    words = lambda v: [(v >> (32 * i)) & M32 for i in range(8)] + [0]
    other = [(1 << 256) - 1, R, 2 * R - 1, (1 << 255) + 12345]                     # not canonical: slicing is by bit position all the same
    sl = rows(zkg.fr29_op("slice", u32([[words(v)] for v in canon + other]))[:, 0])
    for i, v in enumerate(canon + other):
        assert sl[i] == limbs9(v) == F.slice256(words(v)[:8]), i
    back = rows(zkg.fr29_op("unslice_reduce", u32([[s] for s in sl[: len(canon)]]))[:, 0])
    for i, v in enumerate(canon):
        assert back[i] == words(v), i
    above = [R, R + 1, 2 * R - 1, R + (1 << 232), R + (1 << 253)] + [R + rng.below(R) for _ in range(1024)]
    red = rows(zkg.fr29_op("unslice_reduce", u32([[limbs9(v)] for v in above]))[:, 0])
    for i, v in enumerate(above):
        assert red[i] == words(v - R) == F.unslice_reduce(limbs9(v)) + [0], i


def lazy(rng, v, adds=(0, 1 << 30, 3 << 29, 1 << 31)):
    return [x + rng.choice(adds) if i < 8 else x for i, x in enumerate(limbs9(v))]


def step_inputs(n, product, norm_stores, seed):
    """n x (x0, x1, x2, x3, wa, wb, wc) inside the step's contract: rows that get carried on load (x0, x2; every row at stage 0) hold lazy
    limbs — digits under norm_stores, whose records hold digits; rows that go into a product hold lazy limbs up to 2.5 x 2^30 and values
    up to 50 r; rows that are subtracted as they are (stage 0) stay below 2r - 2^232.  Twiddles: digits below r, with 0, one and r - 1."""
    rng = F.Rng(seed)
    small = 2 * R - (6 << 232)                                      # (lazy limbs add up to 4.01 x 2^232 to the value: the carried top limb stays below S2_1's)
    out = []
    tw_edges = [limbs9(0), limbs9(F.ONE), limbs9(R - 1)]
    for e in range(n):
        form = (lambda v: limbs9(v)) if norm_stores or e % 4 == 0 else (lambda v: lazy(rng, v))
        big = lambda: rng.below(50 * R)
        x0, x2 = form(big()), form(big())
        x1, x3 = (form(big()), form(big())) if product else (form(rng.below(small)), form(rng.below(small)))
        if e < 4:
            x0 = x1 = x2 = x3 = list(F.ALL_MAX) if e % 2 == 0 else [0] * 9
        tw = [tw_edges[(e + k) % 3] if e < 9 else limbs9(rng.below(R)) for k in range(3)]
        out.append([x0, x1, x2, x3] + tw)
    return out


@pytest.mark.parametrize("name,product,norm_stores", [("r4", True, False), ("r4_stage0", False, False), ("r4_norm_stores", True, True),
                                                       ("r4_stage0_norm_stores", False, True)])
def test_radix4_step_vs_mirror_and_two_stage_butterfly(zkg, name, product, norm_stores):
    ins = step_inputs(1024, product, norm_stores, 0x44 + zkg.FR29_OPS[name][0])
    got = zkg.fr29_op(name, u32(ins))
    b = F.Bounds()
    for i, x in enumerate(ins):
        g = rows(got[i])
        assert g == F.r4_step(*x, product, norm_stores, b), (name, i)
        v0, v1, v2, v3, wa, wb, wc = (value(v) for v in x)
        a = wa * F.RHO % R if product else 1
        bb, c = wb * F.RHO % R, wc * F.RHO % R
        assert [value(v) % R for v in g] == [(v0 + a * v1 + bb * (v2 + a * v3)) % R, (v0 - a * v1 + c * (v2 - a * v3)) % R,
                                             (v0 + a * v1 - bb * (v2 + a * v3)) % R, (v0 - a * v1 - c * (v2 - a * v3)) % R], (name, i)
        if norm_stores:
            assert all(max(v[:8]) <= M29 for v in g)


@pytest.mark.parametrize("name,product", [("r2_tail", True), ("r2_tail_stage0", False)])
def test_odd_tail_step_vs_mirror_and_butterfly(zkg, name, product):
    ins = [[x[0], x[1], x[4]] for x in step_inputs(1024, product, False, 0x7A11 + product)]
    got = zkg.fr29_op(name, u32(ins))
    b = F.Bounds()
    for i, (u, v, w) in enumerate(ins):
        g = rows(got[i])
        assert g == F.r2_tail_step(u, v, w, product, b), (name, i)
        a = value(w) * F.RHO % R if product else 1
        assert [value(x) % R for x in g] == [(value(u) + a * value(v)) % R, (value(u) - a * value(v)) % R], (name, i)
        assert all(max(x[:8]) <= M29 for x in g)


@pytest.mark.parametrize("norm_stores", [False, True])
def test_chain_of_14_radix4_steps_at_the_bounds(zkg, norm_stores):
    """Each step's four stored rows are the next step's loaded rows, 14 steps = 28 stages (the field's 2-adicity): step 0 in the stage-0
    form, the rest with products.  Row 0 is never multiplied and accumulates the growth (the comments allow 2 r a stage, 60 r in all; a
    product is in fact below 1.36 r and the chain peaks below 40 r); the twiddles of every step are the ones, out of six random table
    values each, that make t1 + t3, u2 and u3 largest; the first eight elements start from the all-maximal digits.  The GPU's limbs equal
    the mirror's at every step, and the mirror asserts the stated bounds at every operation (tests/fr29_ref.py Bounds)."""
    op = ("r4_norm_stores", "r4_stage0_norm_stores") if norm_stores else ("r4", "r4_stage0")

    def on_step(step, ins, outs):
        got = zkg.fr29_op(op[1] if step == 0 else op[0], u32(ins))
        assert np.array_equal(got, u32(outs)), (step, np.argwhere((got != u32(outs)).any(axis=(1, 2)))[:4].tolist())

    b = F.run_chain(256, 0x5A4B0029, norm_stores, on_step=on_step)
    print("chain peaks", {k: (f"{v / R:.2f} r" if k == "data_value" else hex(v)) for k, v in b.peak.items()})
    assert b.peak["limb"] < F.LAZY_LIMB and b.peak["data_value"] < 40 * R
