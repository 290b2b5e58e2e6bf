"""CPU suite: the stream-ordered prover's names exist in the header, the library and the binding; zkg_proof_assemble(where=0) — the host's
proof assembly, the specification the epilogue kernels are compared with — gives the oracle prover's bytes from the five points of a proof;
and the handle's argument rules that need no GPU hold."""
import ctypes as C
import os
import re

import numpy as np

from prove_async_cases import five_points, key_points, oracle_key
from util import R, random_fr_canonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkg_prover_new", "zkg_prover_free", "zkg_prover_batch_max", "zkg_prover_set_batch_max", "zkg_prover_prove_async", "zkg_prover_stats",
         "zkg_proof_assemble")


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_prover_new.restype = C.c_void_p
    L.zkg_prover_new.argtypes = [C.c_void_p]
    L.zkg_prover_free.argtypes = [C.c_void_p]
    L.zkg_prover_batch_max.restype = C.c_size_t
    L.zkg_prover_batch_max.argtypes = [C.c_void_p]
    L.zkg_prover_set_batch_max.argtypes = [C.c_void_p, C.c_size_t]
    L.zkg_prover_prove_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    return zklaim_amd, L


def test_names_are_declared_exported_and_bound():
    zkg, L = _lib()
    header = open(os.path.join(ROOT, "include", "zkg.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in zkg.DECLARED_SYMBOLS
        assert hasattr(L, name), name
    for name in ("Prover", "prover_stats", "proof_assemble"):
        assert callable(getattr(zkg, name))
    for name in ("prove_async", "batch_max", "set_batch_max", "free"):
        assert callable(getattr(zkg.Prover, name))


def test_host_assembly_gives_the_oracle_provers_bytes(oracle):
    """n = 40: the five points from the oracle's multi-exponentiations over [1 | w] and its coefficients_for_H, the constant column's points
    subtracted; three (r, s) pairs, the zero pair among them"""
    zkg, _ = _lib()
    keep = []
    ocs, opk, arrays, _ = oracle_key(oracle, 40, 0xA51, keep)
    rng = np.random.default_rng(7)
    vals = [int(rng.integers(0, 2)) if i % 3 else int.from_bytes(rng.bytes(31), "little") % (R - 2) + 2 for i in range(40)]
    pts = five_points(oracle, ocs, arrays, vals)
    from util import arr
    w = arr(vals, R)
    rss = np.concatenate([random_fr_canonical(4, 0xA52).reshape(2, 8), np.zeros((1, 8), np.uint64)])
    got = zkg.proof_assemble(key_points(arrays), np.tile(pts, (3, 1)), rss, 0)
    for k in range(3):
        rc, proof = oracle.groth16_prove(opk, w, rss[k, :4], rss[k, 4:])
        assert rc == 0 and len(proof) == 134
        assert got[k].tobytes() == proof, k
    assert len({got[k].tobytes() for k in range(3)}) == 3


def test_assemble_refuses_bad_arguments_and_an_empty_call_touches_nothing():
    zkg, L = _lib()
    L.zkg_proof_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    kp = np.zeros(88, np.uint64); pts = np.zeros(72, np.uint64); rs = np.zeros(8, np.uint64); out = np.full(134, 0xA5, np.uint8)
    assert L.zkg_proof_assemble(kp.ctypes.data, pts.ctypes.data, rs.ctypes.data, 0, 0, out.ctypes.data) == zkg.OK
    assert L.zkg_proof_assemble(None, pts.ctypes.data, rs.ctypes.data, 1, 0, out.ctypes.data) == zkg.ERROR
    assert L.zkg_proof_assemble(kp.ctypes.data, None, rs.ctypes.data, 1, 0, out.ctypes.data) == zkg.ERROR
    assert L.zkg_proof_assemble(kp.ctypes.data, pts.ctypes.data, rs.ctypes.data, 1, 2, out.ctypes.data) == zkg.ERROR
    assert L.zkg_proof_assemble(kp.ctypes.data, pts.ctypes.data, rs.ctypes.data, (1 << 16) + 1, 0, out.ctypes.data) == zkg.ERROR
    assert (out == 0xA5).all()


def test_handle_rules_that_need_no_gpu():
    import torch
    zkg, L = _lib()
    assert L.zkg_prover_new(None) is None
    assert b"null key" in L.zkg_last_error()
    if not torch.cuda.is_available():                                            # (with a GPU the session may have called zkg_init: the key would be read)
        fake = np.zeros(64, np.uint64)
        assert L.zkg_prover_new(fake.ctypes.data) is None
        assert b"zkg_init not called" in L.zkg_last_error()
    assert L.zkg_prover_batch_max(None) == 0
    L.zkg_prover_free(None)
    L.zkg_prover_set_batch_max(None, 3)
    # an empty call is ZKG_OK whatever else it is given, and touches nothing
    status = np.full(1, 7, np.uint32)
    assert L.zkg_prover_prove_async(None, None, 0, 0, None, 1, None, 0, status.ctypes.data, None) == zkg.OK
    assert status[0] == 7 and zkg.prover_stats() == (0, 0, 0)
