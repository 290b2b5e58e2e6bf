"""GPU known-answer test of the multi-exponentiation's 29-bit Fq arithmetic (zklaim_amd/csrc/fq29.hip.hpp) through zkg_fq29_op, on raw
limbs: the generated product and squaring streams, the lazy limb-wise operations with their spread constants, the zero test, the
conversions and records, the inversion, XYZZ29::madd with the exceptional path of k_bucket_accum29, and the general addition in its lane,
pair and quad forms — with limbs and values placed AT the bounds the header's comments state, which canonical inputs (zkg_field_op ops
10-15, zkg_g1_add_quad29 / _pair29, whole multi-exponentiations) reach with probability 2^-29 per limb.  References, both CPU-only
(tests/fq29_ref.py, itself checked by tests/test_fq29_mirror.py): plain Python integers, and tools/gen_mont_asm.py's interpreter on the very
streams.  Everything is limb-exact; no tolerances."""
import numpy as np
import pytest

import fq29_ref as F
from fq29_ref import Q, M29, M32, limbs9, value
from gpu_util import zkg  # noqa: F401

pytestmark = pytest.mark.gpu

N_SIM = 768                 # the first results of every product test (the edges and every family) are also interpreted instruction by instruction here;
#                             the CPU suite interprets ALL single-stream operands and the first 1024 of the interleaved ones (tests/test_fq29_mirror.py)


@pytest.fixture(scope="module")
def pts(oracle):
    return F.affine_points(oracle, 1024, F.POINTS_SEED)


def u32(x):
    return np.array(x, dtype=np.uint32)


def rows(a):
    return [[int(v) for v in r] for r in a]


def run(zkg, name, elems, chain=0):
    """elems: n x k limb vectors -> n x m limb vectors as lists"""
    return [rows(e) for e in zkg.fq29_op(name, u32(elems), chain)]


def check_product(t, a, b, tag):
    assert value(t) % Q == value(a) * value(b) * F.RHO % Q and F.is_digits(t), tag
    if value(a) * value(b) < 169 * Q * Q:
        assert value(t) < 2 * Q, tag


# ---- products ---------------------------------------------------------------------------------------------------------------------------
def test_mul_vs_simulator_and_integers(zkg):
    pairs = F.product_operands()
    got = run(zkg, "mul", [[a, b] for a, b in pairs])
    for i, (a, b) in enumerate(pairs):
        assert got[i][0] == F.mont(a, b), i
        check_product(got[i][0], a, b, i)
        if i < N_SIM:
            assert got[i][0] == F.sim_mul(a, b), i


def test_mul2_vs_simulator_and_integers(zkg):
    quads = F.product_quads()
    got = run(zkg, "mul2", quads)
    for i, (a, b, c, d) in enumerate(quads):
        assert got[i] == [F.mont(a, b), F.mont(c, d)], i
        check_product(got[i][0], a, b, i); check_product(got[i][1], c, d, i)
        if i < N_SIM:
            assert tuple(got[i]) == F.sim_mul2(a, b, c, d), i


def test_sqr_vs_simulator_and_integers(zkg):
    ops = F.square_operands()
    got = run(zkg, "sqr", [[a] for a in ops])
    for i, a in enumerate(ops):
        assert got[i][0] == F.sqr(a), i
        check_product(got[i][0], a, a, i)
        if i < N_SIM:
            assert got[i][0] == F.sim_sqr(a), i


def test_sqr2_vs_simulator_and_integers(zkg):
    ops = F.square_pairs()[:2047]                                  # (a launch that is not whole wavefronts)
    got = run(zkg, "sqr2", ops)
    for i, (a, c) in enumerate(ops):
        assert got[i] == [F.sqr(a), F.sqr(c)], i
        check_product(got[i][0], a, a, i); check_product(got[i][1], c, c, i)
        if i < N_SIM:
            assert tuple(got[i]) == F.sim_sqr2(a, c), i


# ---- carries and limb-wise operations ---------------------------------------------------------------------------------------------------
def test_norm_preserves_the_value_and_returns_digits(zkg):
    rng = F.Rng(0x9029)
    top = (1 << 32) - 8                                            # a limb plus the carry into it (at most 7) must not wrap
    cases = [[0] * 9, [top] * 9, [M32] + [top] * 8, [M32] + [0] * 8, [M29] * 9, [(5 << 29) - 1] * 8 + [1 << 27]]
    while len(cases) < 1000:
        k = len(cases) % 3
        cases.append([rng.below(top + 1) for _ in range(9)] if k == 0 else
                     [x + rng.choice((0, 1 << 30, 3 << 29, 1 << 31)) if i < 8 else x for i, x in enumerate(limbs9(rng.below(13 * Q)))] if k == 1 else
                     [rng.choice((0, 1, M29, 1 << 29, top, top - 1)) for _ in range(9)])
    got = run(zkg, "norm", [[c] for c in cases])
    b = F.Bounds()
    for i, a in enumerate(cases):
        assert got[i][0] == F.norm(a, b), i
        assert value(got[i][0]) == value(a) and max(got[i][0][:8]) <= M29, i


def test_add_and_dbl(zkg):
    rng = F.Rng(0xADD)
    cases = [([0] * 9, [0] * 9), (F.ALL_MAX_13, F.ALL_MAX_13), ([3 * M29] * 9, [M29] * 9), ([(1 << 31) - 1] * 9, [(1 << 31) - 1] * 9)]
    cases += [(limbs9(rng.below(13 * Q)), [x + rng.choice((0, 1 << 29, 1 << 30)) for x in limbs9(rng.below(2 * Q))]) for _ in range(300)]
    add = run(zkg, "add", [[a, b] for a, b in cases]); dbl = run(zkg, "dbl", [[a] for a, _ in cases])
    bnd = F.Bounds()
    for i, (a, b) in enumerate(cases):
        assert add[i][0] == F.add(a, b, bnd) == [x + y for x, y in zip(a, b)], i
        assert dbl[i][0] == F.dbl(a, bnd) == [2 * x for x in a], i


# the largest subtrahend value each use site of a spread constant states (units of q).  Under S2_1 the subtrahends are products (below
# 1.04 q where the comments give a figure, below 2 q by the streams' contract); the constant's top limb covers values up to 2 q - 2^232, and
# that is what stands for "2 q" here: the digits of 2 q - 1 already have a top limb one above S2_1's.
USE_SITE = {"S6_1": lambda: limbs9(int(5.3 * Q) - 1), "S4_1": lambda: limbs9(int(3.4 * Q) - 1), "S2_1": lambda: limbs9(2 * Q - (1 << 232) - 1),
            "S4_3": lambda: [3 * M29] * 8 + [(int(3.2 * Q) >> 232) - 3]}


@pytest.mark.parametrize("name", ["S2_1", "S4_1", "S6_1", "S4_3"])
def test_subtractions_never_borrow_up_to_what_the_spread_covers(zkg, name):
    S, K, d = F.SPREADS[name]
    rng = F.Rng(0x5B + K * 8 + d)
    covered = [d * M29] * 8 + [S[8]]                                 # the largest subtrahend the constant covers: the result's top limb is 0
    site = USE_SITE[name]()
    assert value(site) <= value(covered) and all(x <= c for x, c in zip(site, covered))
    subs = [[0] * 9, covered, site, limbs9(Q - 1), limbs9(1)]
    if name == "S4_3":
        subs.append(F.add(limbs9(int(1.06 * Q)), F.dbl(limbs9(int(1.06 * Q)))))         # PPP + 2 Q as madd forms it
    mins = [[0] * 9, [M29] * 8 + [(2 * Q) >> 232], limbs9(2 * Q - 1)]
    cases = [(a, b) for a in mins for b in subs]
    while len(cases) < 515:
        b = limbs9(rng.below(value(site)))
        if d > 1:
            b = [x + rng.choice((0, 1 << 29, M29 * (d - 1))) if i < 8 else x for i, x in enumerate(limbs9(rng.below(value(site) - (3 << 232))))]
        cases.append((limbs9(rng.below(2 * Q)), b))
    got = run(zkg, "sub_" + name, [[a, b] for a, b in cases])
    bnd = F.Bounds()
    for i, (a, b) in enumerate(cases):
        assert got[i][0] == F.sub(a, S, b, bnd) == [x + s - y for x, s, y in zip(a, S, b)], i      # exact integers: no limb borrows
        assert value(got[i][0]) == value(a) + K * Q - value(b), i
    assert got[0][0] == S and got[1][0][8] == 0 and min(got[1][0]) >= 0
    if name == "S2_1":
        ng = run(zkg, "neg_S2_1", [[b] for _, b in cases])
        for i, (_, b) in enumerate(cases):
            assert ng[i][0] == F.neg(S, b, bnd) == [s - y for s, y in zip(S, b)] and value(ng[i][0]) == 2 * Q - value(b), i


# ---- the zero test ----------------------------------------------------------------------------------------------------------------------
def test_is_zero_accepts_every_multiple_and_rejects_its_neighbours(zkg):
    yes = [limbs9(k * Q) for k in range(16)]
    near, deep = [], []                                             # deep: limb 0 intact, so the low-limb filter passes and the comparison must reject
    for k in range(1, 16):
        near += [limbs9(k * Q + 1), limbs9(k * Q - 1)]
        deep += [limbs9(k * Q + (1 << 29)), limbs9(k * Q + (1 << 232))]
        for i in range(1, 9):
            t = limbs9(k * Q); t[i] ^= 1 << (i % 23); deep.append(t)
    deep += [[0] * i + [1] + [0] * (8 - i) for i in range(1, 9)]    # k = 0 with one other limb set
    deep = [t for t in deep if value(t) < 16 * Q]
    assert len(deep) >= 15 * 9 and all(((t[0] * F.PINV) & M29) <= 15 for t in deep)
    no = near + deep
    got = run(zkg, "is_zero", [[t] for t in yes + no])
    bnd = F.Bounds()
    for i, t in enumerate(yes + no):
        assert got[i][0] == [int(i < len(yes))] + [0] * 8 and F.is_zero_mod_p(t, bnd) == (i < len(yes)), (i, t)
    rng = F.Rng(0x15E0)
    rnd = [limbs9(rng.below(16 * Q)) for _ in range(4096)]
    got = run(zkg, "is_zero", [[t] for t in rnd])
    for i, t in enumerate(rnd):
        assert got[i][0][0] == int(F.is_zero_mod_p(t, bnd)) == int(value(t) % Q == 0), i


# ---- conversions and records ------------------------------------------------------------------------------------------------------------
def test_unpack_to29_from29(zkg):
    rng = F.Rng(0xC0429)
    canon = [0, 1, Q - 1, 1 << 253, (1 << 232) - 1, (1 << 232) + 1, 1 << 232, (1 << 29) - 1, 1 << 29, (1 << 253) - 1]
    canon += [rng.below(Q) for _ in range(1013 - len(canon))]
    words = lambda v: F.words8(v) + [0]
    un = run(zkg, "unpack", [[words(v)] for v in canon + [(1 << 256) - 1, (1 << 255) + 12345]])
    for i, v in enumerate(canon + [(1 << 256) - 1, (1 << 255) + 12345]):
        assert un[i][0] == limbs9(v) == F.unpack(F.words8(v)), i                      # by bit position, whatever the value
    to = run(zkg, "to29", [[words(v)] for v in canon])
    for i, v in enumerate(canon):
        assert to[i][0] == F.to29(F.words8(v)) and value(to[i][0]) % Q == 32 * v % Q and value(to[i][0]) < 2 * Q and F.is_digits(to[i][0]), i
    back = run(zkg, "from29", [[t[0]] for t in to])
    for i, v in enumerate(canon):
        assert back[i][0] == words(v), i                                              # from29 o to29
    # from29 on every representative up to 13 q - 1 returns the canonical value
    lifted = [limbs9(value(to[i][0]) + (i % 12) * Q) for i in range(len(canon))] + [limbs9(13 * Q - 1), limbs9(12 * Q), F.ALL_MAX_13[:8] + [F.ALL_MAX_13[8] - 1]]
    bnd = F.Bounds()
    fr = run(zkg, "from29", [[t] for t in lifted])
    for i, t in enumerate(lifted):
        assert fr[i][0] == F.from29(t, bnd) + [0] == words(value(t) * F.RHO * F.FROM % Q), i
    again = run(zkg, "to29", [[w[0]] for w in fr])                                   # to29 o from29: the same field element, canonical digits of it or + q
    for i, t in enumerate(lifted):
        assert again[i][0] == F.to29(fr[i][0][:8]) and value(again[i][0]) % Q == value(t) % Q, i


def test_rec64_round_trip_keeps_the_flag_out_of_x(zkg):
    vals = [0, Q - 1, int(1.01 * Q), (1 << 254) + 1, (1 << 255) - 1]                # the last two: bit 254 set (beyond 1.01 q: the field is 255 bits wide)
    cases = [(limbs9(x), limbs9(y), inf) for x in vals for y in vals for inf in (0, 1)]
    got = run(zkg, "rec64", [[x, y, [inf] + [0] * 8] for x, y, inf in cases])
    for i, (x, y, inf) in enumerate(cases):
        assert got[i] == [x, y, [inf] + [0] * 8], i
        assert tuple(got[i][:2]) + (inf,) == F.rec64(x, y, inf), i


def test_bucket29_round_trip(zkg, pts):
    pt = [F.worst_point(F.scaled(pts[i], F.small_z(F.Rng(i)))) for i in range(6)]
    pt.append([limbs9(int(5.3 * Q) - 1), limbs9(int(3.4 * Q) - 1), limbs9(int(1.1 * Q) - 1), limbs9(int(1.1 * Q) - 1)])
    pt.append([[M29] * 8 + [(5 * Q) >> 232], [M29] * 8 + [(3 * Q) >> 232], [M29] * 8 + [Q >> 232], [M29] * 8 + [(Q >> 232) - 1]])
    bnd = F.Bounds()
    for p in pt:
        bnd.stored(*p)
    got = run(zkg, "bucket29", [p + [[inf] + [0] * 8] for p in pt for inf in (0, 1)])
    for i, p in enumerate(pt):
        assert got[2 * i] == p == F.bucket29(*p, 0) and got[2 * i + 1] == F.INF4 == F.bucket29(*p, 1), i


# ---- the inversion ----------------------------------------------------------------------------------------------------------------------
def test_inverse(zkg):
    rng = F.Rng(0x1297)
    ins = [[M29] * 9] + [limbs9(k * Q) for k in range(9)] + [limbs9(v) for v in (1, Q - 1, Q + 1)]
    ins += [limbs9(rng.below(1 << 261)) for _ in range(2048)]      # 2061 elements: the launch's tail lanes are given the value 1 by the hook
    got = run(zkg, "inverse", [[a] for a in ins])
    for i, a in enumerate(ins):
        g = got[i][0]
        if value(a) % Q == 0:
            assert g == [0] * 9, i
        else:
            assert value(g) * value(a) % Q == pow(1 << 261, 2, Q) and F.is_digits(g) and value(g) < 2 * Q, i
        assert g == F.inverse(a), i


# ---- XYZZ29::madd -----------------------------------------------------------------------------------------------------------------------
def flag(inf):
    return [int(inf)] + [0] * 8


def test_madd_on_every_representative(zkg, pts):
    cases = F.madd_cases(pts)
    assert 64 * 20 <= len(cases) <= 4096
    got = run(zkg, "madd", [acc + [bx, by, flag(inf)] for acc, bx, by, inf, _ in cases])
    bnd = F.Bounds()
    for i, (acc, bx, by, inf, want) in enumerate(cases):
        out, oinf, ok = F.madd(acc, bx, by, inf, bnd)
        assert got[i] == F.madd_out(out, oinf, ok) and ok and not oinf, i
        assert F.is_point(got[i][:4], want), i
        bnd.stored(*got[i][:4])
    print("madd peaks", bnd.show())


def test_madd_exceptional_cases_take_the_fallback(zkg, pts):
    cases = F.madd_exceptional_cases(pts)
    got = run(zkg, "madd", [acc + [bx, by, flag(inf)] for acc, bx, by, inf, _ in cases])
    bnd = F.Bounds(); ks = set()
    for i, (acc, bx, by, inf, want) in enumerate(cases):
        info = {}
        out, oinf, ok = F.madd(acc, bx, by, inf, bnd, info)
        ks.add(value(info["Pd"]) // Q)
        assert not ok and value(info["Pd"]) % Q == 0 and got[i] == F.madd_out(out, oinf, ok), i
        assert got[i][4][:2] == [int(want is None), 0] and F.is_point(got[i][:4], want), i         # madd returned false; the doubling resp. infinity
    assert ks >= set(range(1, 7)), ks                                # Pd = k q for every k = 1 .. 6, from the mirror's Pd


def test_madd_chain_of_64_steps(zkg, pts):
    start = F.chain_points(pts, 40)
    ins, exp = [], []
    bnd = F.Bounds()
    for i, (a, _, A, B) in enumerate(start):
        bx, by = F.rep(B[0]), F.rep(B[1])
        if i % 2:
            by = F.neg(F.S2_1, by); B = F.ec_neg(B)
        ins.append(a + [bx, by, flag(False)])
        acc, inf, ok = F.madd_chain(a, bx, by, 64, bnd)
        want = A
        for _ in range(64):
            want = F.ec_add(want, B)
        assert F.is_point(acc, want)
        exp.append(F.madd_out(acc, inf, ok))
    got = run(zkg, "madd", ins, chain=63)
    assert got == exp, [i for i in range(len(exp)) if got[i] != exp[i]][:4]
    print("madd chain peaks", bnd.show())


# ---- the general addition: one lane, a pair of lanes, a quad ------------------------------------------------------------------------------
FORMS = ("add_lane", "add_pair", "add_quad")


def test_general_addition_three_forms_on_every_case(zkg, pts):
    cases = F.add_cases(pts)
    assert len(cases) % 2 == 1 and len(cases) <= 4096              # an odd count: the last wavefront holds a lone pair / quad
    ins = [a + b for a, b, _ in cases]
    got = {f: run(zkg, f, ins) for f in FORMS}
    bnd = F.Bounds()
    for i, (a, b, want) in enumerate(cases):
        exp = F.add_general(a, b, "lane", bnd)
        for f in FORMS:
            assert got[f][i] == exp, (f, i)
        assert F.is_point(exp, want), i
    print("general addition peaks", bnd.show())


@pytest.mark.parametrize("rounds,n", [(1, 33), (5, 33), (33, 9)])
def test_general_addition_chains_from_the_worst_representatives(zkg, pts, rounds, n):
    start = F.chain_points(pts[200:], n)
    bnd = F.Bounds()
    exp = [F.add_chain(a, b, rounds, "lane", bnd) for a, b, _, _ in start]
    for i, (_, _, A, B) in enumerate(start):
        assert F.is_point(exp[i], F.add_chain_point(A, B, rounds)), i
    for f in FORMS:
        got = run(zkg, f, [a + b for a, b, _, _ in start], chain=rounds)
        assert got == exp, (f, [i for i in range(n) if got[i] != exp[i]][:4])


def test_hook_refuses_bad_arguments(zkg):
    with pytest.raises(zkg.ZkgError):
        zkg.fq29_op("mul", np.zeros((4, 3, 9), np.uint32))
    with pytest.raises(zkg.ZkgError):
        zkg.fq29_op("mul", np.zeros((4, 2, 9), np.uint32), chain=1)                  # only madd and the additions chain
    with pytest.raises(zkg.ZkgError):
        zkg.fq29_op("madd", np.zeros((4, 7, 9), np.uint32), chain=65)
    import ctypes as C
    z = np.zeros(18, np.uint32); p = z.ctypes.data_as(C.c_void_p)
    lib = zkg.lib()
    assert lib.zkg_fq29_op(99, p, C.c_size_t(1), p) == zkg.ERROR and lib.zkg_fq29_op(-1, p, C.c_size_t(1), p) == zkg.ERROR
    assert lib.zkg_fq29_op(0, None, C.c_size_t(1), p) == zkg.ERROR and lib.zkg_fq29_op(0, p, C.c_size_t(1), None) == zkg.ERROR
    assert lib.zkg_fq29_op(0, p, C.c_size_t((1 << 24) + 1), p) == zkg.ERROR                      # refused before anything is read
