"""GPU known-answer test of the 32-bit field layer AT its lazy bounds (csrc/fp.hip.hpp, the generated streams of csrc/mont_asm.inc), for Fq, Fr
and Fq2.  tests/test_gpu_field.py feeds zkg_field_op canonical operands only; here every operand is a raw representative in [0, 2p) from
the families of tests/fp32_ref.py (value edges, limbs of 0 and 0xFFFFFFFF, the fold of add and the borrow of sub, reduction factors of 0
and 0xFFFFFFFF, both representatives of a value, random), nothing is normalised on the way in, and the raw ops (20-28, 40-42) show the
limbs an operator leaves.  Everything is exact: the GPU's limbs equal the closed forms on EVERY element and the interpreted committed
streams on every element of the edge families and the first N_SIM = 64 of the others (tests/test_fp32_mirror.py, without a GPU, holds the
closed forms against the interpreter on all of them); values equal Python integers mod p, for Fq2 oracle/pyref.py's f2_*."""
import pytest

import fp32_ref as ref
from gpu_util import zkg  # noqa: F401

pytestmark = pytest.mark.gpu
FIELD_IDS = {0: "fq", 1: "fr", 2: "fq2"}


@pytest.fixture(scope="module", params=[0, 1, 2], ids=FIELD_IDS.get)
def operands(request):
    """field -> (field, all families end to end as A, B, the indices that also go through the interpreter, per-family offsets)"""
    field = request.param
    fams = ref.fq2_families() if field == 2 else ref.field_families(FIELD_IDS[field])
    A, B, sim, sim_thin, where = [], [], [], [], {}
    for (name, (a, b, _)), idx, idx_thin in zip(fams.items(), ref.sim_indices(fams).values(), ref.sim_indices(fams, thin=8).values()):
        where[name] = len(A)
        sim += [len(A) + i for i in idx]; sim_thin += [len(A) + i for i in idx_thin]
        A += a; B += b
    return field, A, B, sim, sim_thin, where


def run(zkg, field, op, A, B=None):
    w = 2 if field == 2 else 1
    out = zkg.field_op(field, op, ref.pack64(A, w), None if B is None else ref.pack64(B, w))
    return ref.unpack64(out, w)


def family_of(where, i):
    return max((o, n) for n, o in where.items() if o <= i)[1]


@pytest.mark.parametrize("op", ["mul", "add", "sub", "neg", "sqr", "dbl", "chain40", "chain41", "chain42"])
def test_raw_ops(zkg, operands, op):
    """ops 20-28 and the chains 40-42: the limbs the device leaves, without normalized()"""
    field, A, B, sim, sim_thin, where = operands
    F, E = ref.lazy_field(field)
    S, _ = ref.lazy_field(field, sim=True)
    f = ref.OPS[op]
    unary = op in ("neg", "sqr", "dbl")
    got = run(zkg, field, ref.RAW_OP[op], A, None if unary else B)
    assert len(got) == len(A)
    for i, (a, b, g) in enumerate(zip(A, B, got)):
        assert all(c < 2 * F.p for c in F.flat(g)), (family_of(where, i), i, "result not below 2p")
        assert g == f(F, a, b), (family_of(where, i), i, "limbs differ from the closed form")
        assert F.value(g) == f(E, F.value(a), F.value(b)), (family_of(where, i), i, "value differs from the integers")
    for i in (sim_thin if op.startswith("chain") else sim):
        assert got[i] == f(S, A[i], B[i]), (family_of(where, i), i, "limbs differ from the interpreted stream")


@pytest.mark.parametrize("op", ["mul", "add", "sub", "neg", "sqr", "dbl"])
def test_normalising_ops_on_raw_operands(zkg, operands, op):
    """the ops tests/test_gpu_field.py runs on canonical operands, on representatives anywhere below 2p: the canonical result"""
    field, A, B, _, _, where = operands
    F, E = ref.lazy_field(field)
    f = ref.OPS[op]
    got = run(zkg, field, ref.NORM_OP[op], A, None if op in ("neg", "sqr", "dbl") else B)
    for i, (a, b, g) in enumerate(zip(A, B, got)):
        assert all(c < F.p for c in F.flat(g)), (family_of(where, i), i, "not canonical")
        assert g == F.norm(f(F, a, b)) and F.value(g) == f(E, F.value(a), F.value(b)), (family_of(where, i), i)


def test_predicates(zkg, operands):
    """is_zero is 1 exactly for 0 and p (Fq2: in both components); == is 1 exactly when a = b in the field, whatever the representatives"""
    field, A, B, _, _, where = operands
    F, _ = ref.lazy_field(field)
    p = F.p
    flag = lambda x: [x] + [0] * (F.width - 1)
    zeros = [F.unflat(list(z)) for z in ((0, 0), (p, p), (0, p), (p, 0))][: 4 if field == 2 else 2]
    near = [F.unflat([x] * F.width) for x in (1, p - 1, p + 1, 2 * p - 1)] + ([(0, 1), (p, 1), (1, p), (p + 1, 0)] if field == 2 else [])
    X = zeros + near + A
    got = run(zkg, field, ref.OP_IS_ZERO, X)
    for i, (x, g) in enumerate(zip(X, got)):
        assert F.flat(g) == flag(int(all(c in (0, p) for c in F.flat(x)))), ("is_zero", i, x)
    assert [F.flat(g)[0] for g in got[: len(zeros) + len(near)]] == [1] * len(zeros) + [0] * len(near)
    # ==: the families (fold_edges holds differences of 0, p and -p; both_representatives every combination for unequal values) and 256
    # equal values in all four combinations of representatives, per component
    rnd = ref.random.Random(0xE0 + field)
    same = [[rnd.randrange(p) for _ in range(F.width)] for _ in range(256)]
    XA = A + [F.unflat([c + (p if m >> j & 1 else 0) for j, c in enumerate(s)]) for s in same for m in range(4) for _ in range(4)]
    XB = B + [F.unflat([c + (p if m >> j & 1 else 0) for j, c in enumerate(s)]) for s in same for _ in range(4) for m in range(4)]
    got = run(zkg, field, ref.OP_EQ, XA, XB)
    n_equal = 0
    for i, (a, b, g) in enumerate(zip(XA, XB, got)):
        equal = all((x - y) % p == 0 for x, y in zip(F.flat(a), F.flat(b)))
        n_equal += equal
        assert F.flat(g) == flag(int(equal)), ("==", i, a, b)
    assert n_equal >= 4096 and len(XA) - n_equal >= 4096


def test_inverse_of_both_representatives(zkg, operands):
    """op 3 on c and on c + p (Fq2: the four combinations), 256 values: the same canonical inverse; the inverse of every zero is 0"""
    field, _, _, _, _, _ = operands
    F, E = ref.lazy_field(field)
    p = F.p
    rnd = ref.random.Random(0x1A + field)
    c = [[rnd.randrange(p) for _ in range(F.width)] for _ in range(256)]
    c[:4] = [[1] * F.width, [p - 1] * F.width, [F.f.one if field == 2 else F.one] * F.width, [2] + [0] * (F.width - 1)]
    outs = []
    for m in range(2 ** F.width):
        X = [F.unflat([x + (p if m >> j & 1 else 0) for j, x in enumerate(v)]) for v in c]
        outs.append(run(zkg, field, ref.OP_INVERSE, X))
        for v, g in zip(c, outs[-1]):
            assert all(x < p for x in F.flat(g)) and F.value(g) == E.inv(F.value(F.unflat(v))), (m, v)
    assert all(o == outs[0] for o in outs)
    zeros = [F.unflat(list(z)) for z in ((0, 0), (p, p), (0, p), (p, 0))][: 4 if field == 2 else 2]
    assert run(zkg, field, ref.OP_INVERSE, zeros) == [F.zero] * len(zeros)
