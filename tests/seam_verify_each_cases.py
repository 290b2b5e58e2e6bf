"""Cases of the seam's per-item input accumulator (zkg_zklaim_ic_each), shared by the host and the GPU tests.

A case is a key IC_k = c_k G for scalars the case chooses and a list of contexts; the accumulator's output for a context with input map x is
then -(c_0 + sum_k x_k c_k mod r) G, one g1_mul of oracle/pyref.py per item.  A context's public bytes are written directly: pl.hash,
pl.data_ref, pl.data_op.

The input string of a context is, per payload, 32 hash bytes, 64 reference bytes (five little-endian u64, three zero slots) and 64 op bytes
(a byte of value 1 per 8-byte slot), every byte read most significant bit first; string bit s goes to element s // 253 with weight
2^(s % 253).  So string bit s = 1280 p + 8 B + t is bit 7 - t of byte B of payload p."""
import functools

import numpy as np

from util import Q, R, arr, ints

OP_NAMES = ["less", "less_or_eq", "eq", "greater_or_eq", "greater", "not_eq", "noop"]     # the byte set_ops sets in a slot, in order
NO_OP = 1000                                                                         # outside the enum: no byte set
CASE_NAMES = ["random_1", "zero_and_full_1", "random_3", "zero_and_full_3", "random_13", "zero_and_full_13", "one_hot", "relations", "sum_is_infinity"]
PAYLOAD_COUNTS = (1, 3, 13)                                                          # l = 6, 16, 66 (more elements than lanes)


def input_count(npl):
    return (1280 * npl + 252) // 253


def ctx_from_fields(zkg, fields, keep):
    """fields: per payload (hash bytes[32], refs [5 u64], ops [5 enum values])"""
    ctx = zkg.make_ctx([dict(attrs=[0] * 5, refs=[0] * 5, ops=["noop"] * 5, salt=0, hash=b"\1" * 32) for _ in fields], keep)
    node = ctx.pl_ctx_head
    for h, refs, ops in fields:
        pl = node.contents.pl
        pl.hash[:] = list(bytes(h))
        for j in range(5):
            pl.data_ref[j] = int(refs[j]); pl.data_op[j] = int(ops[j])
        node = node.contents.next
    return ctx


def ctx_from_bits(zkg, npl, bits, keep):
    """the context whose input string has exactly the string bits `bits` set (each must be a bit a payload can set)"""
    fields = [(bytearray(32), [0] * 5, [NO_OP] * 5) for _ in range(npl)]
    for s in bits:
        p, o = divmod(s, 1280); B, t = divmod(o, 8)
        h, refs, ops = fields[p]
        if B < 32:
            h[B] |= 0x80 >> t
        elif B < 72:
            a, i = divmod(B - 32, 8)
            refs[a] |= (0x80 >> t) << (8 * i)
        else:
            a, i = divmod(B - 96, 8)
            assert 96 <= B < 136 and t == 7 and i < 7 and ops[a] == NO_OP, ("not a settable bit", s)
            ops[a] = zkg.OPS[OP_NAMES[i]]
    return ctx_from_fields(zkg, fields, keep)


def op_bit(p, slot, i):
    """the string bit that op OP_NAMES[i] in slot `slot` of payload p sets"""
    return 1280 * p + 8 * (96 + 8 * slot + i) + 7


def random_ctx(zkg, npl, rng, keep):
    fields = []
    for _ in range(npl):
        refs = [int(v) for v in rng.integers(0, 1 << 63, 5, dtype=np.int64)]
        refs[int(rng.integers(5))] = (1 << 64) - 1
        fields.append((bytes(rng.integers(0, 256, 32, dtype=np.uint8)), refs, [zkg.OPS[OP_NAMES[int(v)]] for v in rng.integers(0, 7, 5)]))
    return ctx_from_fields(zkg, fields, keep)


def scalars(npl, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % (R - 1) + 1 for _ in range(input_count(npl) + 1)]


def key_points(c):
    """(ic0 (8,), ic (l, 8)) affine Montgomery limbs of c_k G; c_k = 0: infinity, all-zero"""
    import pyref
    pts = np.zeros((len(c), 8), np.uint64)
    for k, v in enumerate(c):
        if v % R:
            pts[k] = arr(list(pyref.g1_mul(v)), Q).reshape(8)
    return pts[0], pts[1:]


def expected(zkg, c, ctxs):
    """-(c_0 + sum_k x_k c_k) G per context, as the hook writes it"""
    import pyref
    out = np.zeros((len(ctxs), 8), np.uint64)
    for i, ctx in enumerate(ctxs):
        x = ints(zkg.zklaim_input_map(ctx), R)
        assert len(x) == len(c) - 1
        s = (c[0] + sum(a * b for a, b in zip(x, c[1:]))) % R
        if s:
            px, py = pyref.g1_mul(s)
            out[i] = arr([px, (Q - py) % Q], Q).reshape(8)
    return out


def one_hot_bits():
    """one payload: the two bits on each side of the element boundaries that fall in hash or reference bytes (253 in the hash's last byte,
    506 in the fourth reference value; 759 and 1265 lie in the string's constant zeros, 1012 in an op byte's upper bits), the first and the
    last bit of a byte in the hash and in a reference value, one op bit per slot"""
    return [252, 253, 505, 506, 0, 7, 248, 255, 256, 263, 568, 575] + [op_bit(0, a, (2 * a + 1) % 7) for a in range(5)]


def relation_scalars():
    """three payloads (l = 16).  With e_k the scalar of input element k (the list's entry 1 + k; entry 0 is IC_0's): e_1 = e_2 = a,
    e_3 = r - a, e_4 = 0 (infinity), e_5 = 2 a, so T[253 * 5 + b] = T[253 * 1 + b + 1]; and e_7 = 2 a as well, which puts an entry equal to
    a lane's running sum into that lane"""
    c = scalars(3, 0x4E1)
    a = c[1 + 1]
    c[1 + 2] = a; c[1 + 3] = R - a; c[1 + 4] = 0; c[1 + 5] = 2 * a % R; c[1 + 7] = 2 * a % R
    return c


def relation_bit_sets():
    """string bits set together, by what they make the accumulator meet (lane = string byte mod 64)"""
    c = relation_scalars()

    def t(s):                                            # the scalar of table entry s
        return c[1 + s // 253] * (1 << (s % 253)) % R
    sets = {}
    # equal entries in different lanes: the tree adds a point to itself (elements 1 and 2, the same bit b)
    sets["tree_doubling"] = [253 + 40, 506 + 40]
    assert t(293) == t(546) and (293 // 8) % 64 != (546 // 8) % 64
    # opposite entries in different lanes: the tree's sum is infinity (element 1 against element 3, an op bit)
    s3 = op_bit(0, 1, 2)
    sets["tree_cancel"] = [s3 - 506, s3]
    assert (t(s3 - 506) + t(s3)) % R == 0 and ((s3 - 506) // 8) % 64 != (s3 // 8) % 64
    # opposite entries in one lane: an op byte of payload 0 and the hash byte of payload 1 that lies 64 string bytes behind it
    s5 = s3 + 505
    sets["lane_cancel"] = [s3, s5]
    assert (t(s3) + t(s5)) % R == 0 and s5 // 8 - s3 // 8 == 64
    # a lane's running sum meets itself: hash byte 0 of payload 1 (element 5) and, 64 string bytes on, a reference byte (element 7)
    sets["lane_doubling"] = [1280 + 6, 1792]
    assert t(1286) == t(1792) and 1792 // 8 - 1286 // 8 == 64
    # T[253 * 5 + b] and T[253 * 1 + b + 1] together, and with a third bit so that the doubled point is added to
    sets["shifted_collision"] = [1265 + 20, 253 + 21, 300]
    assert t(1285) == t(274)
    # infinity entries (element 4) are skipped: alone (the sum is IC_0) and beside others
    inf4 = [op_bit(0, 4, i) for i in (0, 3)]
    assert all(s // 253 == 4 and t(s) == 0 for s in inf4)
    sets["infinity_alone"] = inf4[:1]
    sets["infinity_beside"] = inf4[1:] + [10, 300]
    sets["everything"] = sorted({s for v in sets.values() for s in v} - {inf4[0]})
    return sets


@functools.lru_cache(maxsize=None)
def cases(n_random=5):
    """[(name, npl, c, contexts, expected (n, 8))], built once per process; keep-alive objects ride along in the tuple's last slot"""
    import zklaim_amd as zkg
    keep = []
    out = []

    def add(name, npl, c, ctxs):
        out.append((name, npl, c, ctxs, expected(zkg, c, ctxs)))
    for npl in PAYLOAD_COUNTS:
        c = scalars(npl, 0xC0 + npl)
        rng = np.random.default_rng(0x1C + npl)
        zero = ctx_from_fields(zkg, [(bytes(32), [0] * 5, [NO_OP, 0, -5, 256 + 1, 4]) for _ in range(npl)], keep)
        full = ctx_from_fields(zkg, [(b"\xff" * 32, [(1 << 64) - 1] * 5, [zkg.OPS[OP_NAMES[(p + j) % 7]] for j in range(5)]) for p in range(npl)], keep)
        add("random_%d" % npl, npl, c, [random_ctx(zkg, npl, rng, keep) for _ in range(n_random)])
        add("zero_and_full_%d" % npl, npl, c, [zero, full])
        assert np.array_equal(out[-1][4][0][:4], key_points(c[:1])[0][:4])              # the all-zero string: acc = IC_0, same x
    c1 = scalars(1, 0xC1)
    add("one_hot", 1, c1, [ctx_from_bits(zkg, 1, [s], keep) for s in one_hot_bits()])
    for s, ctx in zip(one_hot_bits(), out[-1][3]):
        x = ints(zkg.zklaim_input_map(ctx), R)
        assert x == [(1 << (s % 253)) if k == s // 253 else 0 for k in range(6)], s
    rel = relation_scalars()
    sets = relation_bit_sets()
    add("relations", 3, rel, [ctx_from_bits(zkg, 3, bits, keep) for bits in sets.values()])
    # c_0 chosen so that the whole sum is infinity: the output is all-zero
    rng = np.random.default_rng(0x1F)
    ctx = random_ctx(zkg, 3, rng, keep)
    c = scalars(3, 0xC9)
    c[0] = -sum(a * b for a, b in zip(ints(zkg.zklaim_input_map(ctx), R), c[1:])) % R
    add("sum_is_infinity", 3, c, [ctx, random_ctx(zkg, 3, rng, keep)])
    assert not out[-1][4][0].any() and out[-1][4][1].any()
    assert [c[0] for c in out] == CASE_NAMES
    out.append(keep)
    return out
