"""CPU suite: the asynchronous resident multi-exponentiation's entry points exist in the header, the library and the binding, and the
argument rules that need no GPU hold: without zkg_init the call is ZKG_ERROR with a message, a null handle takes no vectors."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkg_msm_g1_resident_async", "zkg_msm_g1_resident_batch_max", "zkg_msm_resident_async_stats", "zkg_msm_combine_gpu")


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_msm_g1_resident_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.zkg_msm_g1_resident_batch_max.restype = C.c_size_t
    L.zkg_msm_g1_resident_batch_max.argtypes = [C.c_void_p]
    L.zkg_msm_g2_resident_async.argtypes = L.zkg_msm_g1_resident_async.argtypes
    return zklaim_amd, L


def test_header_declares_and_library_exports_the_async_resident_msm():
    zkg, L = _lib()
    header = open(os.path.join(ROOT, "include", "zkg.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in zkg.DECLARED_SYMBOLS
        assert hasattr(L, name), name
    for name in ("msm_resident_async_stats", "msm_combine_gpu"):
        assert callable(getattr(zkg, name))
    assert callable(zkg.ResidentBases.msm_async) and callable(zkg.ResidentBases.batch_max)


def test_the_call_is_an_error_with_a_message_before_zkg_init_and_writes_nothing():
    import torch
    zkg, L = _lib()
    scalars = np.zeros(4, np.uint64); out = np.full(12, 0xA5A5A5A5A5A5A5A5, np.uint64)
    # (no handle can exist without a GPU: the null one is refused as a bad argument where zkg_init has been called, and before that the
    #  missing zkg_init is reported first)
    assert L.zkg_msm_g1_resident_async(None, scalars.ctypes.data, 1, 1, 1, 0, out.ctypes.data, None) == zkg.ERROR
    msg = L.zkg_last_error().decode()
    assert msg
    if not torch.cuda.is_available():
        assert "zkg_init" in msg
    assert (out == 0xA5A5A5A5A5A5A5A5).all()
    assert zkg.msm_resident_async_stats() == (0, 0, 0)


def test_a_null_handle_takes_no_vectors_and_an_empty_batch_is_ok():
    zkg, L = _lib()
    assert L.zkg_msm_g1_resident_batch_max(None) == 0
    out = np.full(12, 0xA5A5A5A5A5A5A5A5, np.uint64)
    assert L.zkg_msm_g1_resident_async(None, None, 0, 0, 0, 0, out.ctypes.data, None) == zkg.OK
    assert (out == 0xA5A5A5A5A5A5A5A5).all()
    assert zkg.msm_resident_async_stats() == (0, 0, 0)


def test_upload_returns_null_with_a_message_before_zkg_init_for_a_null_pointer_and_for_no_points():
    import torch
    zkg, L = _lib()
    L.zkg_msm_g1_bases_upload.restype = C.c_void_p
    L.zkg_msm_g1_bases_upload.argtypes = [C.c_void_p, C.c_size_t]
    points = np.zeros(8, np.uint64)
    cases = [(None, 1), (points.ctypes.data, 0)]
    if not torch.cuda.is_available():
        cases.append((points.ctypes.data, 1))                            # nothing wrong but the missing zkg_init (which no machine without a GPU can make)
    for d_bases, n in cases:
        assert L.zkg_msm_g2_resident_async(None, points.ctypes.data, 1, 1, 1, 0, points.ctypes.data, None) == zkg.ERROR   # another entry's message first
        assert "zkg_msm_g1_bases_upload" not in L.zkg_last_error().decode()
        assert L.zkg_msm_g1_bases_upload(d_bases, n) is None
        msg = L.zkg_last_error().decode()
        # (before zkg_init that is what is missing, whatever the arguments; after it the entry names itself)
        assert "zkg_init" in msg or "zkg_msm_g1_bases_upload" in msg, msg
        if not torch.cuda.is_available():
            assert "zkg_init" in msg
    assert (points == 0).all()


def test_the_synchronous_call_on_a_null_handle_is_an_error_with_a_message_and_writes_nothing():
    zkg, L = _lib()
    L.zkg_msm_g1_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    scalars = np.zeros(4, np.uint64); out = np.full(12, 0xA5A5A5A5A5A5A5A5, np.uint64)
    assert L.zkg_msm_g1_resident(None, scalars.ctypes.data, 1, 0, out.ctypes.data, None) == zkg.ERROR
    msg = L.zkg_last_error().decode()
    assert "zkg_init" in msg or "zkg_msm_g1_resident" in msg, msg
    assert (out == 0xA5A5A5A5A5A5A5A5).all()


def test_the_epilogue_hook_is_an_error_without_a_gpu():
    import torch
    zkg, L = _lib()
    if torch.cuda.is_available():
        return                                                          # (with a GPU the hook is tests/test_gpu_msm_resident_async.py's business)
    L.zkg_msm_combine_gpu.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
    rec = np.zeros(2 * 12, np.uint64); out = np.full(12, 0xA5A5A5A5A5A5A5A5, np.uint64)
    assert L.zkg_msm_combine_gpu(rec.ctypes.data, 1, 2, 0, 1, out.ctypes.data) == zkg.ERROR
    assert L.zkg_last_error().decode()
    assert (out == 0xA5A5A5A5A5A5A5A5).all()
