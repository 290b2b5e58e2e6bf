"""GPU: k_zklaim_witness alone (zkg_zklaim_witness_gpu) against the host witness pass — tags, listed indices and listed values byte for
byte, for every credential of zklaim_witness_cases, in batches of 1, 3 and 16 contexts.  From nine payloads up (KS_LARGE) the item
workgroup compacts its candidates in two to nine rounds of 256: there both kernels (k_zklaim_witness and k_zklaim_witness_par share the
item workgroup, not the place they read the 1 / c table from) run the credentials whose rounds differ from each other and the sweeps
over all 65 entries of the table; the host passes are zklaim_witness_cases.large_cases', computed once."""
import ctypes as C

import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from zklaim_witness_cases import KS_LARGE, N_SPECS, assert_same_witness, candidate_positions, host_pass, large_cases, payloads

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 8]
ENTRIES = ["zklaim_witness_gpu", "zklaim_witness_gpu_parallel"]


@pytest.mark.parametrize("k", KS)
def test_generator_equals_host_pass(zkg, k):
    keep = []
    ctxs = [zkg.make_ctx(payloads(k, j % N_SPECS, j // N_SPECS), keep) for j in range(16)]
    want = [host_pass(zkg, c) for c in ctxs]
    assert len({w[1].size for w in want}) >= 2
    for batch in ([9], [0, 7, 8], [3], list(range(16))):                      # 1, 3, 1 and 16 contexts: every spec is in one of them
        got = zkg.zklaim_witness_gpu([ctxs[j] for j in batch])
        assert len(got) == len(batch)
        for j, g in zip(batch, got):
            assert_same_witness(g, want[j], (k, j, len(batch)))
    for j in range(N_SPECS):                                                   # and every spec alone
        assert_same_witness(zkg.zklaim_witness_gpu([ctxs[j]])[0], want[j], (k, j, "alone"))


@pytest.mark.parametrize("k", [1, 3])
def test_bad_contexts_fail_alone(zkg, k):
    keep = []
    good = [zkg.make_ctx(payloads(k, j), keep) for j in range(4)]
    other = zkg.make_ctx(payloads(k + 1, 2), keep)                             # another payload count than the batch's
    broken = zkg.make_ctx(payloads(k, 5), keep)
    broken.pl_ctx_head = None                                                  # the list is shorter than num_of_payloads says
    batch = [good[0], None, good[1], other, good[2], broken, good[3]]
    got = zkg.zklaim_witness_gpu(batch)
    assert [g is None for g in got] == [False, True, False, True, False, True, False]
    for j, at in enumerate((0, 2, 4, 6)):
        assert_same_witness(got[at], host_pass(zkg, good[j]), (k, j))


# ---- more than one round of candidates: 9 .. 64 payloads, both kernels

@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("k", KS_LARGE)
def test_large_counts_equal_host_pass(zkg, k, entry):
    """one batch of every large credential with a null context and one of k + 1 payloads (65 at the upper limit) in the middle: the two fail
    alone and write no tag, their neighbours equal the host pass; then one credential alone, another one per count and kernel"""
    generate = getattr(zkg, entry)
    cases = large_cases(zkg, k)
    names = list(cases)
    assert {"mixed0", "random", "ones", "banded1"} <= set(names)
    keep = []
    batch = [cases[name][0] for name in names]
    batch[2:2] = [None, zkg.make_ctx(payloads(k + 1, 2), keep)]
    got = generate(batch)                                                      # (raises if a failed context's tags are not all zero)
    assert len(got) == len(batch) and got[2] is None and got[3] is None
    del got[2:4]
    for name, g in zip(names, got):
        assert_same_witness(g, cases[name][1], (entry, k, name, "batch"))
    alone = names[(KS_LARGE.index(k) + ENTRIES.index(entry)) % 4]
    assert_same_witness(generate([cases[alone][0]])[0], cases[alone][1], (entry, k, alone, "alone"))


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_of_the_inverse_table_is_read(zkg, entry):
    """the two sweeps alone and together: 65 comparisons whose inv variables are the table's entries 0 .. 64 and 64 .. 0.  That the host pass
    lists 63 distinct inverses is test_zklaim_witness_mirror_host's; here the device's listing holds them at the same places."""
    generate = getattr(zkg, entry)
    cases = large_cases(zkg, 13)
    both = [cases["sweep"], cases["sweep_reversed"]]
    for j, (ctx, want) in enumerate(both):
        pos, inv = candidate_positions(13, want[0].size)
        listed = pos[inv][want[0][pos[inv]] == 2]
        assert len(listed) == 63 and len({v.tobytes() for v in want[2][np.searchsorted(want[1], listed)]}) == 63
        got = generate([ctx])[0]
        assert_same_witness(got, want, (entry, j, "alone"))
        assert got[2][np.searchsorted(got[1], listed)].tobytes() == want[2][np.searchsorted(want[1], listed)].tobytes()
    for g, (_, want) in zip(generate([both[1][0], both[0][0]]), both[::-1]):
        assert_same_witness(g, want, (entry, "together"))


def test_more_than_64_payloads_are_refused_before_anything_is_launched(zkg):
    keep = []
    ctx = zkg.make_ctx(payloads(65, 0), keep)
    with pytest.raises(zkg.ZkgError):
        zkg.zklaim_witness_size(65)
    L = zkg.lib()
    ptrs = (C.c_void_p * 2)(None, C.addressof(ctx))
    for entry in ENTRIES:
        with pytest.raises(zkg.ZkgError):
            getattr(zkg, entry)([ctx])
        fn = getattr(L, "zkg_" + entry)
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        tags = np.full((2, 64), 0xAB, np.uint8); idx = np.full((2, 8), 0xABABABAB, np.uint32); vals = np.full((2, 8, 4), 0xAB, np.uint64)
        counts = (C.c_size_t * 2)(0xDEAD, 0xDEAD)
        assert fn(ptrs, 2, tags.ctypes.data, idx.ctypes.data, vals.ctypes.data, 8, counts) == zkg.ERROR
        assert b"no context with a payload count in range" in L.zkg_last_error()          # the argument check's message: no plan, no buffer, no launch
        assert (tags == 0xAB).all() and (idx == 0xABABABAB).all() and (vals == 0xAB).all() and list(counts) == [0xDEAD, 0xDEAD]
    good = large_cases(zkg, 64)["mixed0"]                                      # and the generator still serves the upper limit afterwards
    assert_same_witness(zkg.zklaim_witness_gpu([good[0]])[0], good[1], "64 after 65")
