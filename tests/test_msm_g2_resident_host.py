"""CPU suite: the resident G2 multi-exponentiation's entry points exist in the header, the library and the binding, and the argument rules
that need no GPU hold: without zkg_init the call is ZKG_ERROR with a message, a null handle takes no vectors, an empty batch is OK."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the six new entries and the statistics hook they share with the G1 call
NAMES = ("zkg_msm_g2_bases_upload", "zkg_msm_g2_bases_free", "zkg_msm_g2_resident", "zkg_msm_g2_resident_async", "zkg_msm_g2_resident_batch_max",
         "zkg_msm_combine_g2_gpu", "zkg_msm_resident_async_stats")
FILL = 0xA5A5A5A5A5A5A5A5


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_msm_g2_resident_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.zkg_msm_g2_resident_batch_max.restype = C.c_size_t
    L.zkg_msm_g2_resident_batch_max.argtypes = [C.c_void_p]
    L.zkg_msm_combine_g2_gpu.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p]
    return zklaim_amd, L


def test_header_declares_and_library_exports_the_resident_g2_msm():
    zkg, L = _lib()
    header = open(os.path.join(ROOT, "include", "zkg.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in zkg.DECLARED_SYMBOLS
        assert hasattr(L, name), name
    assert "typedef struct zkg_msm_g2_bases zkg_msm_g2_bases;" in header
    assert callable(zkg.msm_combine_g2_gpu)
    for method in ("msm", "msm_async", "batch_max", "free"):
        assert callable(getattr(zkg.ResidentBasesG2, method)), method


def test_the_call_is_an_error_with_a_message_before_zkg_init_and_writes_nothing():
    import torch
    zkg, L = _lib()
    scalars = np.zeros(4, np.uint64); out = np.full(24, FILL, np.uint64)
    # (no handle can exist without a GPU: the null one is refused as a bad argument where zkg_init has been called, and before that the
    #  missing zkg_init is reported first)
    assert L.zkg_msm_g2_resident_async(None, scalars.ctypes.data, 1, 1, 1, 0, out.ctypes.data, None) == zkg.ERROR
    msg = L.zkg_last_error().decode()
    assert msg
    if not torch.cuda.is_available():
        assert "zkg_init" in msg
    assert (out == FILL).all()
    assert zkg.msm_resident_async_stats() == (0, 0, 0)


def test_a_null_handle_takes_no_vectors_and_an_empty_batch_is_ok():
    zkg, L = _lib()
    assert L.zkg_msm_g2_resident_batch_max(None) == 0
    out = np.full(24, FILL, np.uint64)
    assert L.zkg_msm_g2_resident_async(None, None, 0, 0, 0, 0, out.ctypes.data, None) == zkg.OK
    assert (out == FILL).all()
    assert zkg.msm_resident_async_stats() == (0, 0, 0)


def test_the_epilogue_hook_is_an_error_without_a_gpu():
    import torch
    zkg, L = _lib()
    if torch.cuda.is_available():
        return                                                          # (with a GPU the hook is tests/test_gpu_msm_g2_resident.py's business)
    rec = np.zeros(2 * 24, np.uint64); out = np.full(24, FILL, np.uint64)
    assert L.zkg_msm_combine_g2_gpu(rec.ctypes.data, 1, 0, 1, out.ctypes.data) == zkg.ERROR
    assert L.zkg_last_error().decode()
    assert (out == FILL).all()
