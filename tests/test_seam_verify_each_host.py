"""CPU suite: the seam's per-proof verification entry (zkg_zklaim_verify_each) exists in the header, the library and the binding; count == 0
and the null-argument contract are decided before any GPU call; without a GPU the entry fails loudly; and the accumulator the entry puts in
front of the Miller loops, -(IC_0 + sum_k x_ik IC_k) as a sum of bit-table entries, is checked through its hook with the kernel's code
compiled for the host (zkg_zklaim_ic_each, where = 2) against oracle/pyref.py: one g1_mul per item."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import seam_verify_each_cases as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["zkg_zklaim_verify_each", "zkg_zklaim_verify_each_stats", "zkg_zklaim_ic_each"]


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_zklaim_verify_each.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    return zklaim_amd, L


def _plain_ctx(zklaim_amd, keep):
    return zklaim_amd.make_ctx([dict(attrs=[1, 2, 3, 4, 5], refs=[1, 2, 3, 4, 5], ops=["eq"] * 5, salt=1)], keep)


def test_header_declares_and_library_exports_the_seam_verify_each():
    zklaim_amd, L = _lib()
    header = open(os.path.join(ROOT, "include", "zkg.h")).read()
    assert re.search(r"\bint\s+zkg_zklaim_verify_each\s*\(\s*struct zklaim_ctx \*const \*ctxs, size_t count, int \*rc\)", header)
    assert re.search(r"\bvoid\s+zkg_zklaim_verify_each_stats\s*\(\s*size_t out\[4\]\)", header)
    assert re.search(r"\bint\s+zkg_zklaim_ic_each\s*\(\s*const uint64_t \*ic0, const uint64_t \*ic, const struct zklaim_ctx \*const \*ctxs, "
                     r"size_t count, int where, uint64_t \*out\)", header)
    for name in NAMES:
        assert name in zklaim_amd.DECLARED_SYMBOLS and hasattr(L, name), name
    for fn in ("zklaim_verify_each", "zklaim_verify_each_stats", "zklaim_ic_each"):
        assert callable(getattr(zklaim_amd, fn)), fn


def test_count_zero_and_null_arguments():
    zklaim_amd, L = _lib()
    rc = (C.c_int * 2)(-7, -7)
    assert L.zkg_zklaim_verify_each(None, 0, None) == zklaim_amd.OK
    assert L.zkg_zklaim_verify_each(None, 0, rc) == zklaim_amd.OK and list(rc) == [-7, -7]
    assert zklaim_amd.zklaim_verify_each([]) == []
    keep = []
    ctx = _plain_ctx(zklaim_amd, keep)
    ptrs = (C.c_void_p * 1)(C.addressof(ctx))
    assert L.zkg_zklaim_verify_each(None, 1, rc) == zklaim_amd.ERROR and list(rc) == [-7, -7]
    assert L.zkg_zklaim_verify_each(ptrs, 1, None) == zklaim_amd.ERROR
    assert zklaim_amd.zklaim_verify_each_stats() == (0, 0, 0, 0)


def test_ctx_without_a_key_or_a_proof_is_rc_1_before_any_gpu_call():
    zklaim_amd, L = _lib()
    keep = []
    no_vk = _plain_ctx(zklaim_amd, keep)
    proof = (C.c_ubyte * 134)()
    no_vk.proof = C.addressof(proof); no_vk.proof_size = 134
    no_proof = _plain_ctx(zklaim_amd, keep)
    vk = (C.c_ubyte * 64)()
    no_proof.vk = C.addressof(vk); no_proof.vk_size = 64
    no_size = _plain_ctx(zklaim_amd, keep)
    no_size.vk = C.addressof(vk); no_size.vk_size = 0
    no_size.proof = C.addressof(proof); no_size.proof_size = 134
    assert zklaim_amd.zklaim_verify_each([no_vk, None, no_proof, no_size]) == [1, 1, 1, 1]
    assert zklaim_amd.zklaim_verify_each_stats() == (0, 0, 0, 0)


def test_without_a_gpu_the_entry_is_an_error():
    import torch
    zklaim_amd, L = _lib()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    keep = []
    ctx = _plain_ctx(zklaim_amd, keep)
    vk = (C.c_ubyte * 600)(); proof = (C.c_ubyte * 134)()
    ctx.vk = C.addressof(vk); ctx.vk_size = 600
    ctx.proof = C.addressof(proof); ctx.proof_size = 134
    ptrs = (C.c_void_p * 2)(C.addressof(ctx), None)
    rc = (C.c_int * 2)(-7, -7)
    assert L.zkg_zklaim_verify_each(ptrs, 2, rc) == zklaim_amd.ERROR and list(rc) == [-7, -7]
    with pytest.raises(zklaim_amd.ZkgError):
        zklaim_amd.zklaim_verify_each([ctx])
    assert zklaim_amd.zklaim_verify_each_stats() == (0, 0, 0, 0)
    assert zklaim_amd.libsnark_verify(ctx) == 1                             # the host verifier is what decides without a GPU
    with pytest.raises(zklaim_amd.ZkgError):                                # the hook's kernel leg has no CPU path either
        zklaim_amd.zklaim_ic_each(np.zeros(8, np.uint64), np.zeros((6, 8), np.uint64), [ctx], where=1)


@pytest.mark.parametrize("name", cs.CASE_NAMES)
def test_ic_each_device_code_on_host_against_pyref(name):
    """every case of seam_verify_each_cases: payload counts 1, 3 and 13; random credentials, the all-zero and the fullest string; one-hot
    strings at the element and byte boundaries; a key whose table entries coincide, cancel and are infinity; a sum that is infinity"""
    zklaim_amd, L = _lib()
    case = {c[0]: c for c in cs.cases()[:-1]}[name]
    _, npl, c, ctxs, exp = case
    ic0, ic = cs.key_points(c)
    assert ic.shape[0] == cs.input_count(npl)
    got = zklaim_amd.zklaim_ic_each(ic0, ic, ctxs, where=2)
    assert got.shape == exp.shape
    assert np.array_equal(got, exp), [i for i in range(len(ctxs)) if not np.array_equal(got[i], exp[i])]


def test_ic_each_refuses_a_null_context_and_another_payload_count():
    zklaim_amd, L = _lib()
    keep = []
    rng = np.random.default_rng(5)
    one = cs.random_ctx(zklaim_amd, 1, rng, keep)
    three = cs.random_ctx(zklaim_amd, 3, rng, keep)
    ic0, ic = cs.key_points(cs.scalars(1, 0xC1))
    assert zklaim_amd.zklaim_ic_each(ic0, ic, [one, one], where=2).shape == (2, 8)
    for bad in ([one, None], [None, one], [one, three]):
        with pytest.raises(zklaim_amd.ZkgError):
            zklaim_amd.zklaim_ic_each(ic0, ic, bad, where=2)
    with pytest.raises(zklaim_amd.ZkgError):                                # where is 1 or 2
        zklaim_amd.zklaim_ic_each(ic0, ic, [one], where=0)
