"""The cases of the key blob's point codec, shared by tests/test_point_codec_host.py (where = 0: the host's ser::get_* / put_*) and
tests/test_gpu_point_codec.py (where = 1: the loader's k_decompress_g1 / k_decompress_g2 and the key writer's k_compress_records).
Every expected value comes from oracle/pyref.py's deser_g1 / deser_g2 / ser_g1 / ser_g2: Python integers, the decoding rule restated.

The pool: POOL knowledge commitments (k_i G2, k_i G1) from the oracle's fixed-base tables, their records and the reference's decoding of
those records, computed once per session."""
import numpy as np

import pyref
from pyref import Q, REFUSED
from util import MONT, arr, ints, random_fr_canonical

COUNTS = [1, 255, 256, 257, 513]        # one lane; a partial workgroup; an exact one; one lane into the second; a third, odd (34 n = 2 mod 4)
POOL = 600
GUARD = bytes(range(0xC0, 0xD0))
# (name, g2, stride, offset): the four layouts the loader decompresses
LAYOUTS = [("g1_34", 0, 34, 0), ("g2_66", 1, 66, 0), ("kc_g2_100", 1, 100, 0), ("kc_g1_100", 0, 100, 66)]
LAYOUT_IDS = [l[0] for l in LAYOUTS]

_pool = None


def limbs_g1(P):
    """the reference's point -> 8 Montgomery limbs; infinity and a refusal are all-zero, as the hooks store them"""
    return np.zeros(8, np.uint64) if P is None or P == REFUSED else arr([P[0], P[1]], Q).reshape(8)


def limbs_g2(P):
    return np.zeros(16, np.uint64) if P is None or P == REFUSED else arr([P[0][0], P[0][1], P[1][0], P[1][1]], Q).reshape(16)


class Pool:
    pass


def pool(oracle):
    global _pool
    if _pool is None:
        p = Pool()
        ks = random_fr_canonical(POOL, 0xC0DEC)
        p.g1 = oracle.g1_fixed_base(oracle.g1_generator(), ks)
        p.g2 = oracle.g2_fixed_base(oracle.g2_generator(), ks)
        p.P1, p.P2, p.rec1, p.rec2 = [], [], [], []
        for i in range(POOL):
            a = ints(p.g1[i], Q); b = ints(p.g2[i], Q)
            p.P1.append((a[0], a[1])); p.P2.append(((b[0], b[1]), (b[2], b[3])))
            p.rec1.append(pyref.ser_g1(p.P1[-1])); p.rec2.append(pyref.ser_g2(p.P2[-1]))
        assert {P[1] & 1 for P in p.P1} == {0, 1} and {P[1][0] & 1 for P in p.P2} == {0, 1}       # both parities of y and of y.c0 occur
        # the reference's decoding of every record: what the decompression is compared with.  (That it gives the oracle's points back
        # pins deser_* to ser_* and to the oracle's tables.)
        p.ref1 = np.stack([limbs_g1(pyref.deser_g1(r)) for r in p.rec1])
        p.ref2 = np.stack([limbs_g2(pyref.deser_g2(r)) for r in p.rec2])
        assert np.array_equal(p.ref1, p.g1) and np.array_equal(p.ref2, p.g2)
        _pool = p
    return _pool


def run_of(p, layout, n, replace=None):
    """n records of the layout from the pool's first n commitments; replace: {position: the point's record bytes} -> (bytes, expected limbs)"""
    name, g2, stride, off = layout
    replace = replace or {}
    recs, exp = [], []
    for i in range(n):
        own = replace.get(i, p.rec2[i] if g2 else p.rec1[i])
        assert len(own) == (66 if g2 else 34)
        if stride == 100:
            recs.append(own + p.rec1[i] if g2 else p.rec2[i] + own)
        else:
            recs.append(own)
        if i in replace:
            exp.append(limbs_g2(pyref.deser_g2(own)) if g2 else limbs_g1(pyref.deser_g1(own)))
        else:
            exp.append(p.ref2[i] if g2 else p.ref1[i])
    blob = b"".join(recs)
    assert len(blob) == n * stride
    return blob, np.stack(exp)


def edge_positions(n):
    return sorted({q for q in (0, 255, 256, n - 1) if q < n})


# ---- decompression against deser_* ---------------------------------------------------------------------------------------------------
def check_decompress(zkg, p, layout, n, where):
    name, g2, stride, off = layout
    blob, exp = run_of(p, layout, n)
    got, flag = zkg.point_decompress(blob, stride, off, n, g2, where)
    assert flag == 0 and np.array_equal(got, exp), (name, n)
    # infinity records: '1', then bytes that no rule accepts (x >= q, a parity byte '9'): nothing behind the flag may be read
    inf = b"1" + b"\xff" * (64 if g2 else 32) + b"9"
    planted = edge_positions(n)
    blob, exp = run_of(p, layout, n, {q: inf for q in planted})
    assert not exp[planted].any()
    got, flag = zkg.point_decompress(blob, stride, off, n, g2, where)
    assert flag == 0 and np.array_equal(got, exp), (name, n, "infinity")


# ---- the a.c1 == 0 branch of fq2_sqrt ------------------------------------------------------------------------------------------------
def mont_bytes(v):
    return (v * MONT % Q).to_bytes(32, "little")


def g2_record(x, parity):
    return b"0" + mont_bytes(x[0]) + mont_bytes(x[1]) + parity


def twist_rhs(x):
    return pyref.f2_add(pyref.f2_mul(pyref.f2_mul(x, x), x), pyref.G2_B)


def real_rhs_points():
    """x = (a, c) on the twist with Im(x^3 + b') = 0, i.e. a^2 = (c^3 - b'_1) / (3 c), for small c: -> (an x whose right-hand side is a
    square in Fq: y real; an x whose right-hand side is a non-residue: y purely imaginary)"""
    real = imag = None
    for c in range(1, 64):
        a = pyref.fq_sqrt((c ** 3 - pyref.G2_B[1]) * pyref.inv(3 * c, Q) % Q)
        if a is None:
            continue
        for x in ((a, c), ((-a) % Q, c)):
            rhs = twist_rhs(x)
            assert rhs[1] == 0
            if rhs[0] == 0:
                continue
            if pyref.fq_sqrt(rhs[0]) is not None:
                real = real or x
            else:
                imag = imag or x
    assert real is not None and imag is not None          # one of each kind (c = 2 and c = 7)
    return real, imag


def sqrt_branch_records():
    """G2 records that reach the branches random points never reach: [(name, 66 bytes, the reference's verdict)]"""
    real, imag = real_rhs_points()
    out = []
    for name, x in (("real_root", real), ("imaginary_root", imag)):
        for parity in (b"0", b"1"):
            rec = g2_record(x, parity)
            P = pyref.deser_g2(rec)
            assert P not in (None, REFUSED) and pyref.on_curve(pyref.Field2, P)
            assert (P[1][1] == 0 and P[1][0] != 0) if name == "real_root" else (P[1][0] == 0 and P[1][1] != 0)
            out.append((name + "_" + parity.decode(), rec, P))
        a, b = pyref.deser_g2(g2_record(x, b"0")), pyref.deser_g2(g2_record(x, b"1"))
        assert a[1] == pyref.f2_neg(b[1])                                     # the two parity bytes give the two roots
    # false on the first level: the norm of x^3 + b' is a non-residue of Fq
    x = next((k, 1) for k in range(1, 200) if twist_rhs((k, 1))[1] != 0 and
             pyref.fq_sqrt(sum(v * v for v in twist_rhs((k, 1))) % Q) is None)
    for parity in (b"0", b"1"):
        out.append(("nonresidue_norm_" + parity.decode(), g2_record(x, parity), REFUSED))
    # x = 0: the right-hand side is b' itself, not a square of Fq2 either (its c1 is not zero: the general branch)
    assert pyref.G2_B[1] != 0 and pyref.f2_sqrt(pyref.G2_B) is None
    for parity in (b"0", b"1"):
        out.append(("x_zero_" + parity.decode(), g2_record((0, 0), parity), REFUSED))
    for name, rec, P in out:
        assert pyref.deser_g2(rec) == P, name
    return out


def g1_x_zero_records():
    """G1 x = 0, y^2 = 3, with both parity bytes: [(34 bytes, the reference's verdict)]"""
    return [(b"0" + bytes(32) + parity, pyref.deser_g1(b"0" + bytes(32) + parity)) for parity in (b"0", b"1")]


def check_sqrt_branches(zkg, p, where):
    cases = sqrt_branch_records()
    for stride, layout in ((66, LAYOUTS[1]), (100, LAYOUTS[2])):
        n = len(cases) + 2                                                   # a pool record on either side
        blob, exp = run_of(p, layout, n, {1 + j: rec for j, (_, rec, _) in enumerate(cases)})
        for j, (name, rec, P) in enumerate(cases):
            assert np.array_equal(exp[1 + j], limbs_g2(P)), name
        got, flag = zkg.point_decompress(blob, stride, 0, n, 1, where)
        for j, (name, rec, P) in enumerate(cases):
            assert np.array_equal(got[1 + j], exp[1 + j]), (name, stride)
        assert np.array_equal(got, exp) and flag == 1
        # without the refused ones the flag stays clear
        good = [c for c in cases if c[2] != REFUSED]
        blob, exp = run_of(p, layout, len(good), {j: rec for j, (_, rec, _) in enumerate(good)})
        got, flag = zkg.point_decompress(blob, stride, 0, len(good), 1, where)
        assert np.array_equal(got, exp) and flag == 0 and exp.any(axis=1).all()
    g1 = g1_x_zero_records()
    for layout in (LAYOUTS[0], LAYOUTS[3]):
        blob, exp = run_of(p, layout, 4, {1: g1[0][0], 2: g1[1][0]})
        got, flag = zkg.point_decompress(blob, layout[2], layout[3], 4, 0, where)
        assert np.array_equal(got, exp) and flag == (1 if g1[0][1] == REFUSED else 0)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def fq_nonresidue_x():
    return next(x for x in range(1, 1000) if pyref.fq_sqrt((x ** 3 + 3) % Q) is None)


def _put(rec, at, value):
    return rec[:at] + value + rec[at + len(value):]


def _shift_x(rec, at, by):
    """the 32 limb bytes at `at` plus `by` (q or 2 q): the same residue under another encoding"""
    v = int.from_bytes(rec[at:at + 32], "little") + by
    assert v < 1 << 256
    return _put(rec, at, v.to_bytes(32, "little"))


def refusal_variants(g2):
    """[(name, record -> malformed record)]: what the rule of pyref.deser_* refuses"""
    last = 65 if g2 else 33
    v = [("flag_2", lambda r: _put(r, 0, b"2")), ("parity_7", lambda r: _put(r, last, b"7")), ("parity_nul", lambda r: _put(r, last, b"\0"))]
    if g2:
        x = next((k, 1) for k in range(1, 200) if pyref.f2_sqrt(twist_rhs((k, 1))) is None)
        v.append(("nonresidue_x", lambda r: _put(r, 1, mont_bytes(x[0]) + mont_bytes(x[1]))))
    else:
        v.append(("nonresidue_x", lambda r: _put(r, 1, mont_bytes(fq_nonresidue_x()))))
    for cname, at in (("c0", 1), ("c1", 33)) if g2 else (("x", 1),):
        v.append((cname + "_plus_q", lambda r, at=at: _shift_x(r, at, Q)))
        v.append((cname + "_plus_2q", lambda r, at=at: _shift_x(r, at, 2 * Q)))
        v.append((cname + "_all_ones", lambda r, at=at: _put(r, at, b"\xff" * 32)))
    return v


def decode_reducing_x(rec, g2):
    """the rule before the canonical check: the stored limbs are taken modulo q"""
    for at in (1, 33) if g2 else (1,):
        rec = _put(rec, at, (int.from_bytes(rec[at:at + 32], "little") % Q).to_bytes(32, "little"))
    return pyref.deser_g2(rec) if g2 else pyref.deser_g1(rec)


def planted_refusals(p, layout, n, variant, positions):
    name, g2, stride, off = layout
    vname, mutate = variant
    replace = {}
    for q in positions:
        orig = p.rec2[q] if g2 else p.rec1[q]
        bad = mutate(orig)
        assert (pyref.deser_g2(bad) if g2 else pyref.deser_g1(bad)) == REFUSED, vname        # the verdict is the reference's
        if vname.endswith("_plus_q"):                                        # a second encoding of the SAME point, accepted before the check
            assert decode_reducing_x(bad, g2) == (p.P2[q] if g2 else p.P1[q])
        replace[q] = bad
    return run_of(p, layout, n, replace)


def check_refusals_planted(zkg, p, layout, where):
    """each malformed record at positions 0, 255, 256 (= last) of a 257-record run: the flag is set, exactly the planted outputs are
    all-zero and every neighbour is the reference's point"""
    name, g2, stride, off = layout
    n = 257
    planted = edge_positions(n)
    for variant in refusal_variants(g2):
        blob, exp = planted_refusals(p, layout, n, variant, planted)
        got, flag = zkg.point_decompress(blob, stride, off, n, g2, where)
        zero = np.flatnonzero(~got.any(axis=1)).tolist()
        assert flag != 0 and zero == planted, (name, variant[0], flag, zero)
        assert np.array_equal(got, exp), (name, variant[0])


def check_refusals_side_by_side(zkg, p, layout, where):
    """every malformed record once, side by side in one call, a valid record between any two"""
    name, g2, stride, off = layout
    variants = refusal_variants(g2)
    n = 2 * len(variants) + 1
    replace = {}
    for j, (vname, mutate) in enumerate(variants):
        bad = mutate(p.rec2[2 * j + 1] if g2 else p.rec1[2 * j + 1])
        assert (pyref.deser_g2(bad) if g2 else pyref.deser_g1(bad)) == REFUSED, vname
        replace[2 * j + 1] = bad
    blob, exp = run_of(p, layout, n, replace)
    got, flag = zkg.point_decompress(blob, stride, off, n, g2, where)
    bad_rows = [vname for j, (vname, _) in enumerate(variants) if got[2 * j + 1].any()]
    assert flag != 0 and not bad_rows, (name, "accepted:", bad_rows)
    assert np.array_equal(got, exp), name
    # and each alone in a run of valid records sets the flag by itself
    for vname, mutate in variants:
        blob1, exp1 = run_of(p, layout, 3, {1: mutate(p.rec2[1] if g2 else p.rec1[1])})
        got1, flag1 = zkg.point_decompress(blob1, stride, off, 3, g2, where)
        assert flag1 != 0 and not got1[1].any() and np.array_equal(got1, exp1), (name, vname, "alone")


# ---- compression against ser_* -------------------------------------------------------------------------------------------------------
def check_compress_g1(zkg, p, n, where):
    g1 = p.g1[:n].copy()
    inf = edge_positions(n)
    g1[inf] = 0
    exp = b"".join(pyref.ser_g1(None) if i in inf else p.rec1[i] for i in range(n))
    got, guard = zkg.point_compress(g1, rec=34, where=where, guard=GUARD)
    assert got == exp, n
    assert guard == GUARD, "bytes behind the run were written"
    # fewer records than points: the run ends at n, not at the input's end
    if n > 1:
        got, guard = zkg.point_compress(p.g1[:n], rec=34, where=where, n=n - 1, guard=GUARD)
        assert got == b"".join(p.rec1[:n - 1]) and guard == GUARD, n


def gapped_indices(n, seed):
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(POOL, n, replace=False)).astype(np.uint32)
    assert (np.diff(idx.astype(np.int64)) > 0).all() and (n == 1 or (np.diff(idx.astype(np.int64)) > 1).any())     # increasing, with gaps
    return idx


def check_compress_kc(zkg, p, n, where):
    idx = gapped_indices(n, 100 + n)
    g1 = p.g1.copy(); g2 = p.g2.copy()
    inf = {int(idx[q]) for q in edge_positions(n)} if n > 1 else set()       # infinity commitments at the edges (n = 1 keeps its point)
    for e in inf:
        g1[e] = 0; g2[e] = 0
    exp = b"".join(pyref.ser_g2(None) + pyref.ser_g1(None) if int(e) in inf else p.rec2[e] + p.rec1[e] for e in idx)
    got, guard = zkg.point_compress(g1, g2, idx, rec=100, where=where, guard=GUARD)
    assert got == exp, n
    assert guard == GUARD, "bytes behind the run were written"


def check_compress_kc_permuted(zkg, p, where):
    """the gather reads idx[i], not i"""
    n = 257
    idx = np.random.default_rng(7).permutation(n).astype(np.uint32)
    assert (idx != np.arange(n)).sum() > n // 2
    got, guard = zkg.point_compress(p.g1[:n], p.g2[:n], idx, rec=100, where=where, guard=GUARD)
    assert got == b"".join(p.rec2[e] + p.rec1[e] for e in idx) and guard == GUARD


def check_round_trip(zkg, p, where):
    """decompress(compress(P)) == P over the whole pool, through both record sizes"""
    rec, _ = zkg.point_compress(p.g1, rec=34, where=where)
    got, flag = zkg.point_decompress(rec, 34, 0, POOL, 0, where)
    assert flag == 0 and np.array_equal(got, p.g1)
    rec, _ = zkg.point_compress(p.g1, p.g2, np.arange(POOL, dtype=np.uint32), rec=100, where=where)
    got2, flag2 = zkg.point_decompress(rec, 100, 0, POOL, 1, where)
    got1, flag1 = zkg.point_decompress(rec, 100, 66, POOL, 0, where)
    assert flag1 == 0 and flag2 == 0 and np.array_equal(got2, p.g2) and np.array_equal(got1, p.g1)


# ---- pk blobs: where the sections lie (the format of csrc/codec.hip's header comment) ----------------------------------------------------
def blob_sections(blob):
    """-> dict: A (offset of the A query's first record, count), idx (offset of the first index, end of the list, the indices),
    B (offset of the first 100-byte value, count)"""
    def dec(at):
        nl = blob.index(b"\n", at)
        return int(blob[at:nl]), nl + 1
    at = 34 + 34 + 66 + 34 + 66
    nA, at = dec(at)
    out = {"A": (at, nA)}
    at += 34 * nA
    domain, at = dec(at)
    nidx, at = dec(at)
    first = at
    idx = []
    for _ in range(nidx):
        v, at = dec(at)
        idx.append(v)
    out["idx"] = (first, at, idx)
    nval, at = dec(at)
    assert domain == nA and nval == nidx
    out["B"] = (at, nval)
    return out


def with_index_list(blob, idx):
    first, end, old = blob_sections(blob)["idx"]
    assert len(idx) == len(old)
    return blob[:first] + b"".join(b"%d\n" % v for v in idx) + blob[end:]


def damaged_point_blobs(blob):
    """one A-query record, then one B-query G2 record, each as x + q, x + 2q and with the parity byte '7': [(name, blob)]"""
    sec = blob_sections(blob)
    out = []
    for qname, (at, count), stride, g2 in (("A", sec["A"], 34, 0), ("B_g2", sec["B"], 100, 1)):
        k = next(i for i in range(count) if blob[at + i * stride:at + i * stride + 1] == b"0")       # a record that is not infinity
        o = at + k * stride
        size = 66 if g2 else 34
        rec = blob[o:o + size]
        assert (pyref.deser_g2(rec) if g2 else pyref.deser_g1(rec)) not in (None, REFUSED)
        for vname, bad in (("plus_q", _shift_x(rec, 1, Q)), ("plus_2q", _shift_x(rec, 1, 2 * Q)), ("parity_7", _put(rec, size - 1, b"7"))):
            assert (pyref.deser_g2(bad) if g2 else pyref.deser_g1(bad)) == REFUSED
            out.append((qname + "_" + vname, blob[:o] + bad + blob[o + size:]))
            assert len(out[-1][1]) == len(blob)
    return out


def disordered_index_blobs(blob):
    """the B query's index list with one index repeated, and with two neighbours swapped: [(name, blob)]"""
    idx = blob_sections(blob)["idx"][2]
    assert len(idx) >= 3 and all(a < b for a, b in zip(idx, idx[1:]))        # libsnark's sparse_vector: strictly increasing
    rep = list(idx); rep[2] = rep[1]
    swp = list(idx); swp[1], swp[2] = swp[2], swp[1]
    return [("repeated", with_index_list(blob, rep)), ("swapped", with_index_list(blob, swp))]
