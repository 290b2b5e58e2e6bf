"""CPU suite: the device-witness prove entries exist in the header, the library and the binding; without a GPU there is no key, and the
argument rules that need neither hold: a null key is ZKG_ERROR, an empty batch is ZKG_OK and touches nothing."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkg_groth16_prove_dev", "zkg_groth16_prove_batch_dev", "zkg_prove_dev_stats")


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_groth16_prove_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.zkg_groth16_prove_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return zklaim_amd, L


def test_header_declares_and_library_exports_the_device_witness_prover():
    zkg, L = _lib()
    header = open(os.path.join(ROOT, "include", "zkg.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in zkg.DECLARED_SYMBOLS
        assert hasattr(L, name), name
    for name in ("prove_dev_stats", "groth16_prove_batch_dev"):
        assert callable(getattr(zkg, name))
    assert callable(zkg.Crs.prove_dev) and callable(zkg.Crs.prove_batch_dev)


def test_null_key_is_an_error_and_writes_nothing():
    zkg, L = _lib()
    rs = np.ones(8, np.uint64); out = np.zeros(256, np.uint8); ln = C.c_size_t(77); status = np.full(2, -1, np.int32)
    somewhere = np.zeros(64, np.uint64)                                          # never read: the null key is refused first
    assert L.zkg_groth16_prove_dev(None, somewhere.ctypes.data, rs.ctypes.data, rs[4:].ctypes.data, 1, out.ctypes.data, C.byref(ln), None) == zkg.ERROR
    assert L.zkg_groth16_prove_batch_dev(None, somewhere.ctypes.data, 16, 2, rs.ctypes.data, 1, out.ctypes.data, status.ctypes.data, None) == zkg.ERROR
    assert not out.any() and ln.value == 77 and list(status) == [-1, -1]
    assert zkg.prove_dev_stats() == (0, 0)
    rc, got = zkg.groth16_prove_batch_dev(None, somewhere.ctypes.data, 16, 1, [(rs[:4], rs[4:])])
    assert rc == zkg.ERROR and got == [(-1, None)]


def test_empty_batch_is_ok_and_touches_nothing():
    zkg, L = _lib()
    out = np.full(134, 0xA5, np.uint8); status = np.full(1, -1, np.int32)
    assert L.zkg_groth16_prove_batch_dev(None, None, 0, 0, None, 1, out.ctypes.data, status.ctypes.data, None) == zkg.OK
    assert (out == 0xA5).all() and status[0] == -1
    assert zkg.groth16_prove_batch_dev(None, 0, 0, 0, []) == (zkg.OK, [])
    assert zkg.prove_dev_stats() == (0, 0) and zkg.prove_batch_stats() == (0, 0, 0)
