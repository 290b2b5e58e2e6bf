"""CPU suite: the seam's batch verification entry exists in the header, the library and the binding; count == 0, the null-argument contract and
"a ctx without a key or a proof is rc 1" are decided before any GPU call, so they hold with no GPU in the machine; and the bit rule the
device front end assembles public inputs with (zkg_zklaim_input_map_mirror: k_zklaim_input_sums' code compiled for the host) equals
zkg_zklaim_input_map."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from util import MONT, R, from_limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "zkg_zklaim_verify_batch"
HOOKS = ["zkg_zklaim_verify_batch_stats", "zkg_proof_decode_gpu", "zkg_zklaim_input_sums_gpu", "zkg_zklaim_input_map_mirror"]
OP_NAMES = ["less", "less_or_eq", "eq", "greater_or_eq", "greater", "not_eq", "noop"]


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_zklaim_verify_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    return zklaim_amd, L


def _plain_ctx(zklaim_amd, keep):
    return zklaim_amd.make_ctx([dict(attrs=[1, 2, 3, 4, 5], refs=[1, 2, 3, 4, 5], ops=["eq"] * 5, salt=1)], keep)


def test_header_declares_and_library_exports_the_seam_verify_batch():
    zklaim_amd, L = _lib()
    header = open(os.path.join(ROOT, "include", "zkg.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*struct zklaim_ctx \*const \*ctxs, size_t count, int \*rc\)" % NAME, header)
    for name in [NAME] + HOOKS:
        assert name in zklaim_amd.DECLARED_SYMBOLS and hasattr(L, name), name
    for fn in ("zklaim_verify_batch", "zklaim_verify_batch_stats", "proof_decode_gpu", "zklaim_input_sums_gpu", "zklaim_input_map_mirror"):
        assert callable(getattr(zklaim_amd, fn)), fn


def test_count_zero_touches_nothing():
    zklaim_amd, L = _lib()
    rc = (C.c_int * 2)(-7, -7)
    assert L.zkg_zklaim_verify_batch(None, 0, None) == zklaim_amd.OK
    assert L.zkg_zklaim_verify_batch(None, 0, rc) == zklaim_amd.OK and list(rc) == [-7, -7]
    assert zklaim_amd.zklaim_verify_batch([]) == []


def test_null_arguments_are_an_error():
    zklaim_amd, L = _lib()
    keep = []
    ctx = _plain_ctx(zklaim_amd, keep)
    ptrs = (C.c_void_p * 1)(C.addressof(ctx))
    rc = (C.c_int * 1)(-7)
    assert L.zkg_zklaim_verify_batch(None, 1, rc) == zklaim_amd.ERROR and rc[0] == -7
    assert L.zkg_zklaim_verify_batch(ptrs, 1, None) == zklaim_amd.ERROR


def test_ctx_without_a_key_or_a_proof_is_rc_1():
    zklaim_amd, L = _lib()
    keep = []
    no_vk = _plain_ctx(zklaim_amd, keep)
    proof = (C.c_ubyte * 134)()
    no_vk.proof = C.addressof(proof); no_vk.proof_size = 134
    no_proof = _plain_ctx(zklaim_amd, keep)
    vk = (C.c_ubyte * 64)()
    no_proof.vk = C.addressof(vk); no_proof.vk_size = 64
    assert zklaim_amd.zklaim_verify_batch([no_vk, None, no_proof]) == [1, 1, 1]
    assert zklaim_amd.zklaim_verify_batch_stats() == (0, 0, 0, 0)
    # a vk pointer without a size is no key either
    no_size = _plain_ctx(zklaim_amd, keep)
    no_size.vk = C.addressof(vk); no_size.vk_size = 0
    no_size.proof = C.addressof(proof); no_size.proof_size = 134
    assert zklaim_amd.zklaim_verify_batch([no_size]) == [1]
    assert [zklaim_amd.libsnark_verify(c) for c in (no_vk, no_proof)] == [1, 1]


def _payloads(k, rng, variant):
    """k payloads: random hashes; reference values with 0 and 2^64 - 1 among them; every op in turn"""
    out = []
    for i in range(k):
        refs = [int(v) for v in rng.integers(0, 1 << 63, 5, dtype=np.int64)]
        refs[(i + variant) % 5] = 0
        refs[(i + variant + 2) % 5] = (1 << 64) - 1
        if variant == 2:
            refs = [(1 << 64) - 1] * 5
        ops = [OP_NAMES[(i + j + variant) % 7] for j in range(5)]
        out.append(dict(attrs=[0] * 5, refs=refs, ops=ops, salt=0, hash=bytes(rng.integers(0, 256, 32, dtype=np.uint8)) if variant else b"\xff" * 32))
    return out


def _python_input_map(ctx):
    """the bit rule on Python integers: per payload 256 hash bits, 512 reference bits, 512 op bits, every byte most significant bit first;
    bit b of the whole goes to element b // 253 with weight 2^(b % 253)"""
    import zklaim_amd
    slot = {v: i for i, v in enumerate(zklaim_amd.OPS[n] for n in OP_NAMES)}
    bits = []
    node = ctx.pl_ctx_head
    while node:
        pl = node.contents.pl
        data = bytearray(bytes(pl.hash))
        refs = bytearray(64); ops = bytearray(64)
        for j in range(5):
            refs[8 * j:8 * j + 8] = int(pl.data_ref[j]).to_bytes(8, "little")
            if int(pl.data_op[j]) in slot:
                ops[8 * j + slot[int(pl.data_op[j])]] = 1
        data += refs + ops
        for byte in data:
            bits += [(byte >> (7 - t)) & 1 for t in range(8)]
        node = node.contents.next
    n = (len(bits) + 252) // 253
    return [sum(b << t for t, b in enumerate(bits[253 * c:253 * c + 253])) for c in range(n)]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 20])
def test_mirror_equals_the_input_map(k):
    """element boundaries (bits 253 c of the string, 1280 bits per payload) fall inside the hash (253), inside a reference value (506: the
    fourth), inside an op slot (1012: the fourth) and, from two payloads on, elements span two payloads (element 5: bits 1265 .. 1517);
    with more payloads the boundaries move through every field"""
    zklaim_amd, L = _lib()
    for variant in range(3):
        keep = []
        ctx = zklaim_amd.make_ctx(_payloads(k, np.random.default_rng(100 * k + variant), variant), keep)
        ref = zklaim_amd.zklaim_input_map(ctx)
        assert ref.shape[0] == (1280 * k + 252) // 253
        assert zklaim_amd.zklaim_input_map_mirror(ctx, count_only=True) == ref.shape[0]
        got = zklaim_amd.zklaim_input_map_mirror(ctx)
        assert got.tobytes() == ref.tobytes()


def test_mirror_with_an_out_of_range_op():
    """set_ops' default: an enum value outside the seven sets no byte"""
    zklaim_amd, L = _lib()
    keep = []
    ctx = zklaim_amd.make_ctx(_payloads(2, np.random.default_rng(7), 1), keep)
    node = ctx.pl_ctx_head.contents
    node.pl.data_op[1] = 1000; node.pl.data_op[3] = 0; node.pl.data_op[4] = -5
    node.next.contents.pl.data_op[0] = 256 + 1                  # low byte is zklaim_less: still no op
    ref = zklaim_amd.zklaim_input_map(ctx)
    assert zklaim_amd.zklaim_input_map_mirror(ctx).tobytes() == ref.tobytes()
    exp = _python_input_map(ctx)
    assert [from_limbs(r) for r in zklaim_amd.zklaim_input_map_mirror(ctx)] == [v * MONT % R for v in exp]


def test_mirror_against_the_bit_rule_on_python_integers():
    zklaim_amd, L = _lib()
    keep = []
    ctx = zklaim_amd.make_ctx(_payloads(3, np.random.default_rng(11), 1), keep)
    exp = _python_input_map(ctx)
    got = zklaim_amd.zklaim_input_map_mirror(ctx)
    assert len(exp) == 16 and got.shape == (16, 4)
    assert [from_limbs(r) for r in got] == [v * MONT % R for v in exp]
    assert max(exp) < 1 << 253 and any(v >> 252 for v in exp)


def test_mirror_of_a_null_and_of_an_empty_context():
    zklaim_amd, L = _lib()
    L.zkg_zklaim_input_map_mirror.restype = C.c_size_t
    L.zkg_zklaim_input_map_mirror.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    assert L.zkg_zklaim_input_map_mirror(None, None, 0) == 0
    keep = []
    ctx = zklaim_amd.make_ctx([], keep)
    assert zklaim_amd.zklaim_input_map_mirror(ctx, count_only=True) == 0 == zklaim_amd.zklaim_input_map(ctx).shape[0]
