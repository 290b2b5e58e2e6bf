"""The digit sort without its single-workgroup scan launches (msm.hip: k_rx_count's window totals, the bin starts worked out inside
k_rx_scatter / k_rx_fine, the class histogram made in k_rx_fine, the class starts scanned inside k_order_place) and the reduction's chunk
results stored straight into the host landing zone: every path that runs the changed kernels returns the oracle's point, bit for bit."""
import numpy as np
import pytest

from gpu_util import dev_bases_g1, to_dev, zkg  # noqa: F401
from util import R, limbs, random_fr_canonical

pytestmark = pytest.mark.gpu

N_EDGE = 70000                 # c = 16, two-pass sort, 64 coarse bins per window, 5 slices of 16K digits (the last one partial)


def _oracle_msm(oracle, bases, sc):
    return oracle.msm_g1(bases, sc, oracle.BDLO12, oracle.num_threads())


@pytest.fixture(scope="module")
def edge_bases(zkg):
    d_bases, bases, _ = dev_bases_g1(zkg, N_EDGE, 0x50A7)
    return d_bases, bases


@pytest.mark.parametrize("n", [49152, 49156])
def test_two_pass_sort_at_its_smallest_size(zkg, oracle, n):
    """49152 points: the first size that takes the two-pass sort (three full slices); 49156: a fourth slice of four digits"""
    d_bases, bases, _ = dev_bases_g1(zkg, n, 0x50A0 + n)
    sc = random_fr_canonical(n, 0x50A1 + n)
    d_sc = to_dev(sc)
    assert np.array_equal(zkg.msm_g1_dev(d_bases.data_ptr(), d_sc.data_ptr(), n), _oracle_msm(oracle, bases, sc))


def _edge_scalars(kind):
    n = N_EDGE
    rng = np.random.default_rng(0x50A8)
    if kind == "equal":                       # one bucket per window holds every entry: a giant bin, a heavy class, every other class empty
        return np.tile(random_fr_canonical(1, 0x50A9), (n, 1))
    if kind == "zero":                        # no entry at all: every window total, bin count and class but class 0 is zero
        return np.zeros((n, 4), np.uint64)
    if kind == "r-1":
        return np.tile(np.array(limbs(R - 1), np.uint64), (n, 1))
    if kind == "top_window":                  # windows 0 ... 14 empty: the top window starts at entry 0 behind fifteen zero totals
        sc = np.zeros((n, 4), np.uint64)
        sc[:, 3] = rng.integers(1, (R >> 240), n).astype(np.uint64) << np.uint64(48)       # bits 240 ... 253, below r's own
        return sc
    if kind == "half_one_digit":              # half of window 0's entries in one bucket, the rest uniform
        sc = random_fr_canonical(n, 0x50AA)
        half = rng.random(n) < 0.5
        sc[half, 0] = (sc[half, 0] & ~np.uint64(0xFFFF)) | np.uint64(0x1234)
        return sc
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["equal", "zero", "r-1", "top_window", "half_one_digit"])
def test_two_pass_sort_skewed_digits(zkg, oracle, edge_bases, kind):
    d_bases, bases = edge_bases
    sc = np.ascontiguousarray(_edge_scalars(kind))
    d_sc = to_dev(sc)
    assert np.array_equal(zkg.msm_g1_dev(d_bases.data_ptr(), d_sc.data_ptr(), N_EDGE), _oracle_msm(oracle, bases, sc))


def test_one_pass_sort_orders_buckets_with_the_new_placement(zkg, oracle):
    """20000 points stay on the one-pass sort: k_class_hist, then k_order_place's own scan of the classes"""
    n = 20000
    d_bases, bases, _ = dev_bases_g1(zkg, n, 0x50AB)
    sc = random_fr_canonical(n, 0x50AC)
    sc[::3] = sc[0]                                           # a heavy class beside the short ones
    d_sc = to_dev(sc)
    assert np.array_equal(zkg.msm_g1_dev(d_bases.data_ptr(), d_sc.data_ptr(), n), _oracle_msm(oracle, bases, sc))


def test_resident_table_launch_keeps_empty_buckets_last(zkg, oracle, edge_bases):
    """a table launch accumulates only the first `lanes` < buckets entries of the bucket order: a non-empty bucket ordered behind an empty
    one would be lost"""
    d_bases, bases = edge_bases
    sc = random_fr_canonical(N_EDGE, 0x50AD)
    d_sc = to_dev(sc)
    h = zkg.ResidentBases(d_bases.data_ptr(), N_EDGE)
    try:
        got = h.msm(d_sc.data_ptr())
        again = h.msm(d_sc.data_ptr())
    finally:
        h.free()
    exp = _oracle_msm(oracle, bases, sc)
    assert np.array_equal(got, exp) and np.array_equal(again, exp)


def test_piece_wise_step_twice_from_pinned_and_pageable_memory(zkg):
    """2^19 + 256 points: the smallest piece-wise job (its first pieces of n/8 are two-pass sorts beside an accumulation, 512-thread workgroups),
    called twice in a row from pinned and from pageable memory: the resident call's point every time"""
    import torch
    n = (1 << 19) + 256
    d_bases, _, _ = dev_bases_g1(zkg, n, 0x50AE)
    sc = random_fr_canonical(n, 0x50AF)
    d_sc = to_dev(sc)
    h_sc = torch.from_numpy(sc.view(np.int64)).pin_memory()
    exp = zkg.msm_g1_dev(d_bases.data_ptr(), d_sc.data_ptr(), n)
    for _ in range(2):
        assert np.array_equal(zkg.msm_g1_host_scalars(d_bases.data_ptr(), h_sc.data_ptr(), n), exp)
    for _ in range(2):
        assert np.array_equal(zkg.msm_g1_host_scalars(d_bases.data_ptr(), sc.ctypes.data, n), exp)
