"""CPU suite: the seam's batch entry exists in the header, the library and the binding; count == 0, the null-argument contract and "a
ctx without a key is rc 1" are decided before any GPU call, so they hold with no GPU in the machine."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "zkg_zklaim_prove_batch"


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_zklaim_prove_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    return zklaim_amd, L


def test_header_declares_and_library_exports_the_seam_batch():
    zklaim_amd, L = _lib()
    header = open(os.path.join(ROOT, "include", "zkg.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*struct zklaim_ctx \*const \*ctxs, size_t count, int \*rc\)" % NAME, header)
    assert NAME in zklaim_amd.DECLARED_SYMBOLS
    assert hasattr(L, NAME)
    assert callable(zklaim_amd.zklaim_prove_batch)


def test_count_zero_touches_nothing():
    zklaim_amd, L = _lib()
    rc = (C.c_int * 2)(-7, -7)
    assert L.zkg_zklaim_prove_batch(None, 0, None) == zklaim_amd.OK
    assert L.zkg_zklaim_prove_batch(None, 0, rc) == zklaim_amd.OK and list(rc) == [-7, -7]
    assert zklaim_amd.zklaim_prove_batch([]) == []


def test_null_arguments_are_an_error():
    zklaim_amd, L = _lib()
    keep = []
    ctx = zklaim_amd.make_ctx([dict(attrs=[1, 2, 3, 4, 5], refs=[1, 2, 3, 4, 5], ops=["eq"] * 5, salt=1)], keep)
    ptrs = (C.c_void_p * 1)(C.addressof(ctx))
    rc = (C.c_int * 1)(-7)
    assert L.zkg_zklaim_prove_batch(None, 1, rc) == zklaim_amd.ERROR and rc[0] == -7
    assert L.zkg_zklaim_prove_batch(ptrs, 1, None) == zklaim_amd.ERROR


def test_ctx_without_a_key_is_rc_1():
    zklaim_amd, L = _lib()
    keep = []
    ctx = zklaim_amd.make_ctx([dict(attrs=[1, 2, 3, 4, 5], refs=[1, 2, 3, 4, 5], ops=["eq"] * 5, salt=1)], keep)
    assert zklaim_amd.zklaim_prove_batch([ctx, None, ctx]) == [1, 1, 1]
    assert not ctx.proof and ctx.proof_size == 0
    # a pk pointer without a size is no key either
    buf = (C.c_ubyte * 16)()
    ctx.pk = C.addressof(buf); ctx.pk_size = 0
    assert zklaim_amd.zklaim_prove_batch([ctx]) == [1]
