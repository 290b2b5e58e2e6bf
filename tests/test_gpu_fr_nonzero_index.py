"""GPU parity: the generator's ordered non-zero index (k_nonzero_count / k_nonzero_scan / k_nonzero_scatter behind zkg_fr_nonzero_index,
where 1) against the host loop (where 0) and against the mask the vector was built from.  The sizes are the kernels' own geometry: one
element per thread, 64 per wavefront, 256 per workgroup, and a scan workgroup that takes 1024 workgroup counts (262144 elements) per round
with a carry — one less than, exactly and one more than each, n = 1, and 2^17 + 3.  The count word and every index are compared; the words
behind idx_out[count] must keep what the caller left there (the hook itself refuses a device list with an entry written behind its count)."""
import ctypes as C

import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from util import MONT, R, limbs

pytestmark = pytest.mark.gpu

WAVE, BLOCK, SCAN_ROUND = 64, 256, 1024 * 256
SIZES = [1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5, SCAN_ROUND - 1, SCAN_ROUND, SCAN_ROUND + 1, (1 << 17) + 3]
GUARD, SENTINEL = 64, 0x5A5A5A5A
R_ROW = np.array(limbs(R), np.uint64)
NONZERO = np.array([limbs(v) for v in (1, R - 1, R + 1, 2 * R - 1, MONT % R, 2, R + MONT % R)], np.uint64)   # every one of them != 0 mod r


def masks(n):
    """name -> bool[n], True where the element is non-zero"""
    rng = np.random.default_rng(n)
    i = np.arange(n)
    first = np.zeros(n, bool); first[0] = True
    last = np.zeros(n, bool); last[-1] = True
    return {"all_zero": np.zeros(n, bool), "all_nonzero": np.ones(n, bool), "first_only": first, "last_only": last,
            "empty_workgroups": (i // BLOCK) % 3 == 0, "alternating": i % 2 == 1, "density_3pct": rng.random(n) < 0.03}


def vector(mask, zero_as_r, seed):
    """raw limbs: non-zero representatives (below and above r) where mask, else 0 — or r"""
    rng = np.random.default_rng(seed)
    fr = NONZERO[rng.integers(0, len(NONZERO), mask.size)]
    fr[~mask] = R_ROW if zero_as_r else 0
    return np.ascontiguousarray(fr)


def raw_index(zkg, fr, where):
    """the C entry on a buffer with a guard behind it -> (indices, the whole buffer)"""
    L = zkg.lib()
    L.zkg_fr_nonzero_index.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    n = fr.shape[0]
    buf = np.full(n + GUARD, SENTINEL, np.uint32); count = C.c_size_t(1 << 40)
    rc = L.zkg_fr_nonzero_index(fr.ctypes.data, n, where, buf.ctypes.data, C.byref(count))
    assert rc == 0, L.zkg_last_error().decode()
    return buf[:count.value].copy(), buf, count.value


@pytest.mark.parametrize("n", SIZES)
def test_device_index_equals_the_host_loop_and_the_mask(zkg, n):
    for name, mask in masks(n).items():
        for zero_as_r in (False, True):                              # every zero written as r instead of 0
            fr = vector(mask, zero_as_r, n + 7)
            want = np.nonzero(mask)[0].astype(np.uint32)
            host, _, _ = raw_index(zkg, fr, 0)
            dev, buf, count = raw_index(zkg, fr, 1)
            assert count == want.size, (name, zero_as_r, count, want.size)
            assert np.array_equal(host, want), (name, zero_as_r)
            assert np.array_equal(dev, want), (name, zero_as_r)
            assert (buf[count:] == SENTINEL).all(), (name, zero_as_r)
            assert np.array_equal(zkg.fr_nonzero_index(fr), want)    # the binding (where=1 is its default)


def test_mixed_representatives_and_n_zero(zkg):
    values = [0, R, 1, R - 1, R + 1, 2 * R - 1, MONT % R] * 41      # 287 elements: past one workgroup
    fr = np.array([limbs(v) for v in values], np.uint64)
    want = [i for i, v in enumerate(values) if v % R != 0]
    assert zkg.fr_nonzero_index(fr, where=1).tolist() == want == zkg.fr_nonzero_index(fr, where=0).tolist()
    assert zkg.fr_nonzero_index(np.zeros((0, 4), np.uint64), where=1).size == 0
