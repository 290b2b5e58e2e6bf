"""CPU suite: the zkg_domain entry points exist in the header, the library and the binding, and the argument rules that need no GPU hold:
without zkg_init no handle is made and the error is named, a null handle has no size and takes no vectors, freeing it returns."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkg_domain_new", "zkg_domain_free", "zkg_domain_size", "zkg_domain_batch_max", "zkg_domain_set_batch_max", "zkg_domain_ntt_async",
         "zkg_domain_lagrange_async", "zkg_domain_stats")


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_domain_new.restype = C.c_void_p
    L.zkg_domain_new.argtypes = [C.c_size_t]
    L.zkg_domain_free.argtypes = [C.c_void_p]
    L.zkg_domain_size.restype = L.zkg_domain_batch_max.restype = C.c_size_t
    L.zkg_domain_size.argtypes = L.zkg_domain_batch_max.argtypes = [C.c_void_p]
    L.zkg_domain_set_batch_max.argtypes = [C.c_void_p, C.c_size_t]
    L.zkg_domain_ntt_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.zkg_domain_lagrange_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return zklaim_amd, L


def test_header_declares_and_library_exports_the_domain_handle():
    zkg, L = _lib()
    header = open(os.path.join(ROOT, "include", "zkg.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in zkg.DECLARED_SYMBOLS
        assert hasattr(L, name), name
    assert callable(zkg.domain_stats)
    for method in ("ntt_async", "lagrange_async", "batch_max", "set_batch_max", "size", "free"):
        assert callable(getattr(zkg.Domain, method)), method


def test_no_handle_without_zkg_init_and_the_error_says_so():
    from zklaim_amd import api
    zkg, L = _lib()
    if api._initialised:                                            # a GPU box with the library already initialised by an earlier test: the rule
        return                                                      # cannot be seen from this process any more
    assert L.zkg_domain_new(1 << 10) is None
    msg = L.zkg_last_error().decode()
    assert msg and "zkg_init" in msg
    try:
        zkg.Domain(24)
    except zkg.ZkgError as e:
        assert "zkg_init" in str(e)
    else:
        raise AssertionError("Domain(24) was made without zkg_init")


def test_a_null_handle_has_no_size_takes_no_vectors_and_is_freed():
    zkg, L = _lib()
    assert L.zkg_domain_size(None) == 0 and L.zkg_domain_batch_max(None) == 0
    L.zkg_domain_free(None)
    L.zkg_domain_set_batch_max(None, 3)
    a = np.full(8, 0xA5A5A5A5A5A5A5A5, np.uint64)
    assert L.zkg_domain_ntt_async(None, a.ctypes.data, 2, 1, 0, 0, None) == zkg.ERROR
    assert L.zkg_last_error().decode()
    assert zkg.domain_stats() == (0, 0, 0)
    t = np.zeros(4, np.uint64)
    assert L.zkg_domain_lagrange_async(None, t.ctypes.data, a.ctypes.data, None, None) == zkg.ERROR
    assert L.zkg_last_error().decode()
    assert (a == 0xA5A5A5A5A5A5A5A5).all()
    # an empty batch is ZKG_OK whatever the handle: nothing to do, nothing touched
    assert L.zkg_domain_ntt_async(None, None, 0, 0, 0, 0, None) == zkg.OK
    assert zkg.domain_stats() == (0, 0, 0)
