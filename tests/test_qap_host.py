"""CPU suite: the zkg_qap entry points exist in the header, the library and the binding, and the argument rules that need no GPU hold:
without zkg_init no handle is made and the error is named, a null handle has no size, no variables and no batch, takes no witnesses and
writes nothing, freeing it returns, and an empty batch is ZKG_OK."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkg_qap_new", "zkg_qap_free", "zkg_qap_domain_size", "zkg_qap_num_variables", "zkg_qap_batch_max", "zkg_qap_set_batch_max",
         "zkg_qap_witness_h_async", "zkg_qap_stats")
FILL = 0xA5A5A5A5A5A5A5A5


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_qap_new.restype = C.c_void_p
    L.zkg_qap_new.argtypes = [C.c_void_p]
    L.zkg_qap_free.argtypes = [C.c_void_p]
    L.zkg_qap_domain_size.restype = L.zkg_qap_batch_max.restype = C.c_size_t
    L.zkg_qap_num_variables.restype = C.c_uint32
    L.zkg_qap_domain_size.argtypes = L.zkg_qap_batch_max.argtypes = L.zkg_qap_num_variables.argtypes = [C.c_void_p]
    L.zkg_qap_set_batch_max.argtypes = [C.c_void_p, C.c_size_t]
    L.zkg_qap_witness_h_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return zklaim_amd, L


def _tiny_system(zkg, keep):
    """x * x = y over two variables: one row per matrix"""
    one = np.array([[1, 0, 0, 0]], np.uint64)                        # any limbs: the system is never evaluated here
    rp = np.array([0, 1], np.uint32)
    return zkg.make_r1cs(2, 1, (rp, np.array([1], np.uint32), one), (rp, np.array([1], np.uint32), one), (rp, np.array([2], np.uint32), one), keep)


def test_header_declares_and_library_exports_the_qap_handle():
    zkg, L = _lib()
    header = open(os.path.join(ROOT, "include", "zkg.h")).read()
    assert re.search(r"typedef\s+struct\s+zkg_qap\s+zkg_qap\s*;", header)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in zkg.DECLARED_SYMBOLS
        assert hasattr(L, name), name
    assert callable(zkg.qap_stats)
    for method in ("witness_h_async", "domain_size", "num_variables", "batch_max", "set_batch_max", "free"):
        assert callable(getattr(zkg.Qap, method)), method


def test_no_handle_without_zkg_init_and_the_error_says_so():
    from zklaim_amd import api
    zkg, L = _lib()
    if api._initialised:                                            # a GPU box with the library already initialised by an earlier test: the rule
        return                                                      # cannot be seen from this process any more
    keep = []
    cs = _tiny_system(zkg, keep)
    assert L.zkg_qap_new(C.byref(cs)) is None
    msg = L.zkg_last_error().decode()
    assert msg and "zkg_init" in msg
    try:
        zkg.Qap(cs)
    except zkg.ZkgError as e:
        assert "zkg_init" in str(e)
    else:
        raise AssertionError("Qap(cs) was made without zkg_init")


def test_a_null_handle_has_no_size_takes_no_witnesses_and_is_freed():
    zkg, L = _lib()
    assert L.zkg_qap_domain_size(None) == 0 and L.zkg_qap_num_variables(None) == 0 and L.zkg_qap_batch_max(None) == 0
    L.zkg_qap_free(None)
    L.zkg_qap_set_batch_max(None, 3)
    w = np.full((2, 4), FILL, np.uint64); hh = np.full((5, 4), FILL, np.uint64); flags = np.full(2, 0xA5A5A5A5, np.uint32)
    assert L.zkg_qap_witness_h_async(None, w.ctypes.data, 2, 1, hh.ctypes.data, 5, flags.ctypes.data, None) == zkg.ERROR
    assert L.zkg_last_error().decode()
    assert zkg.qap_stats() == (0, 0, 0)
    assert (w == FILL).all() and (hh == FILL).all() and (flags == 0xA5A5A5A5).all()


def test_an_empty_batch_is_ok_whatever_the_handle():
    zkg, L = _lib()
    hh = np.full((5, 4), FILL, np.uint64)
    assert L.zkg_qap_witness_h_async(None, None, 0, 0, hh.ctypes.data, 0, None, None) == zkg.OK
    assert zkg.qap_stats() == (0, 0, 0)
    assert (hh == FILL).all()
