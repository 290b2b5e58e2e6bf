"""CPU suite: the device witness generator's gate-by-gate mirror, compiled for the host (zkg_zklaim_witness_mirror), against the host
witness pass (zkg_zklaim_witness_new + zkg_circuit_sparse_witness): tags, listed indices and listed values byte for byte.  From nine
payloads up (KS_LARGE) the candidates take more than one round of 256 on the device: the layout that puts the rounds' boundaries where they
are, the credentials whose rounds differ and the sweep over the 1 / c table are checked here from the host pass alone, and the mirror runs
them all, so that an error in the code it shares with the device shows without a GPU."""
import ctypes as C

import numpy as np
import pytest

from util import R, ints
from zklaim_witness_cases import (BOUNDARIES, KS_LARGE, N_SPECS, ROUND, assert_same_witness, boundary_classes, candidate_classes, candidate_positions,
                                  honest_payloads, host_pass, large_cases, listed_per_round, payloads)

KS = [1, 2, 3, 5, 8]
# k -> n_inputs and the cumulative ends of data, plvars, refvals and alpha / inv (= the most an item lists)
CLASS_ENDS = {9: (46, 91, 145, 217, 307), 13: (66, 131, 209, 313, 443), 20: (102, 202, 322, 482, 682), 37: (188, 373, 595, 891, 1261), 64: (324, 644, 1028, 1540, 2180)}


def _zkg():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    zklaim_amd.lib()
    return zklaim_amd


def test_names_are_declared_and_exported():
    zkg = _zkg()
    for name in ("zkg_groth16_prove_batch_zklaim", "zkg_zklaim_witness_gpu", "zkg_zklaim_witness_mirror", "zkg_zklaim_witness_stats", "zkg_zklaim_witness_size"):
        assert name in zkg.DECLARED_SYMBOLS and hasattr(zkg.lib(), name), name
    for name in ("zklaim_witness_gpu", "zklaim_witness_mirror", "zklaim_witness_stats"):
        assert callable(getattr(zkg, name))
    assert callable(zkg.Crs.prove_batch_zklaim)


@pytest.mark.parametrize("k", KS)
def test_mirror_equals_host_pass(k):
    zkg = _zkg()
    keep = []
    listed = set()
    for spec in range(N_SPECS):
        ctx = zkg.make_ctx(payloads(k, spec), keep)
        want = host_pass(zkg, ctx)
        got = zkg.zklaim_witness_mirror(ctx)
        assert zkg.zklaim_witness_size(k)[0] == want[0].size
        assert_same_witness(got, want, (k, spec))
        assert want[1].size <= zkg.zklaim_witness_size(k)[1]
        listed.add(int(want[1].size))
    assert len(listed) >= 2, "the value-dependent tagging (a packed 0 or 1 is not listed) was not exercised"


@pytest.mark.parametrize("k", KS)
def test_serial_host_pass_gives_the_same(k, monkeypatch):
    zkg = _zkg()
    keep = []
    for spec in (0, 3, 7, 8, 9):
        ctx = zkg.make_ctx(payloads(k, spec), keep)
        got = zkg.zklaim_witness_mirror(ctx)
        assert_same_witness(got, host_pass(zkg, ctx), (k, spec, "pool"))
        monkeypatch.setenv("ZKG_SERIAL_CIRCUIT", "1")
        assert_same_witness(got, host_pass(zkg, ctx), (k, spec, "serial"))
        assert_same_witness(zkg.zklaim_witness_mirror(ctx), got, (k, spec, "mirror under serial"))
        monkeypatch.delenv("ZKG_SERIAL_CIRCUIT")


def test_broken_payload_list_is_an_error():
    zkg = _zkg()
    keep = []
    ctx = zkg.make_ctx(payloads(2, 0), keep)
    ctx.num_of_payloads = 3
    with pytest.raises(zkg.ZkgError):
        zkg.zklaim_witness_mirror(ctx)


# ---- more than one round of candidates: 9 .. 64 payloads

@pytest.mark.parametrize("k", KS_LARGE)
def test_round_boundaries_fall_where_the_large_counts_were_chosen_for(k):
    zkg = _zkg()
    n, cap = zkg.zklaim_witness_size(k)
    ends = candidate_classes(k)
    assert tuple(ends.values()) == CLASS_ENDS[k]
    assert ends["input_fe"] == -(-1280 * k // 253) and cap == ends["alpha_inv"] == ends["input_fe"] + 29 * k
    assert boundary_classes(k) == BOUNDARIES[k]
    assert len(BOUNDARIES[k]) == (cap - 1) // ROUND and (k <= 9 or len(BOUNDARIES[k]) >= 1)
    pos, inv = candidate_positions(k, n)                                      # the positions follow from n alone; every host pass below lists nothing else
    assert len(pos) == cap and len(pos[inv]) == 5 * k and pos[-1] < n
    assert {c for ks in BOUNDARIES.values() for c in ks} == set(ends)        # every class holds a boundary at some count


def test_payload_count_limits():
    zkg = _zkg()
    assert zkg.zklaim_witness_size(64)[1] == CLASS_ENDS[64][-1]
    L = zkg.lib()
    L.zkg_zklaim_witness_size.restype = C.c_size_t
    L.zkg_zklaim_witness_size.argtypes = [C.c_size_t, C.c_void_p]
    for k in (0, 65, 66, 1 << 32):
        with pytest.raises(zkg.ZkgError):
            zkg.zklaim_witness_size(k)
        cap = C.c_size_t(0xDEAD)
        assert L.zkg_zklaim_witness_size(k, C.byref(cap)) == 0 and cap.value == 0xDEAD
    keep = []
    ctx = zkg.make_ctx(payloads(65, 0), keep)
    for name in ("zkg_zklaim_witness_mirror", "zkg_zklaim_witness_mirror_parallel"):
        fn = getattr(L, name)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        tags = np.full(64, 0xAB, np.uint8); idx = np.full(8, 0xABABABAB, np.uint32); vals = np.full((8, 4), 0xAB, np.uint64); cnt = C.c_size_t(0xDEAD)
        assert fn(C.addressof(ctx), tags.ctypes.data, idx.ctypes.data, vals.ctypes.data, 8, C.byref(cnt)) == zkg.ERROR
        assert b"payload count out of range" in L.zkg_last_error()
        assert (tags == 0xAB).all() and (idx == 0xABABABAB).all() and (vals == 0xAB).all() and cnt.value == 0xDEAD


def test_rounds_of_the_large_credentials_differ():
    """a condition on the inputs, read off the host pass: rounds and wavefronts that list nothing between rounds that list nearly all 256"""
    zkg = _zkg()
    k = KS_LARGE[-1]
    cases = large_cases(zkg, k)
    for name in ("banded0", "banded1"):
        rounds, fewest, most = listed_per_round(k, cases[name][1])
        print(name, rounds, fewest, most)
        assert len(rounds) == 9 and fewest == 0 and most > 200, (name, rounds, fewest, most)
        assert rounds[0] > 200 and 0 < rounds[-1] < ROUND, (name, rounds)
    rounds0, rounds1 = listed_per_round(k, cases["banded0"][1])[0], listed_per_round(k, cases["banded1"][1])[0]
    assert rounds0.count(0) >= 2 and rounds0 != rounds1                      # whole rounds list nothing, not the first and not the last one
    assert ROUND in listed_per_round(k, cases["random"][1])[0]               # and in the same batch a round lists all 256
    pos, _ = candidate_positions(k, cases["banded0"][1][0].size)
    waves = (cases["banded0"][1][0][pos] == 2)[:8 * ROUND].reshape(8, 4, 64).sum(2)       # the eight whole rounds by wavefront
    assert any(0 in w and max(w) > 32 for w in waves.tolist()), waves         # a round in which one wavefront lists nothing and another most of its 64
    for kk in KS_LARGE:                                                        # the mixed credentials: neither all nor none in any round
        rounds, _, _ = listed_per_round(kk, large_cases(zkg, kk)["mixed0"][1])
        full = [ROUND] * (len(rounds) - 1) + [candidate_classes(kk)["alpha_inv"] - ROUND * (len(rounds) - 1)]
        assert all(0 < r for r in rounds) and any(r < f for r, f in zip(rounds, full)), (kk, rounds)


def test_the_sweep_reads_every_entry_of_the_inverse_table():
    """from the host pass alone: the 65 comparisons' inv variables are 1 / c for c = 0 .. 64 in turn, 0 and 1 by tag and 63 listed values"""
    zkg = _zkg()
    cases = large_cases(zkg, 13)
    expect = [c and pow(c, -1, R) for c in range(65)]
    seen = {}
    for name, order in (("sweep", list(range(65))), ("sweep_reversed", list(range(64, -1, -1)))):
        tags, idx, vals = cases[name][1]
        pos, inv = candidate_positions(13, tags.size)
        inv_pos = pos[inv]
        assert len(inv_pos) == 65
        assert [int(t) for t in tags[inv_pos]] == [min(c, 2) for c in order]
        listed = [p for p, c in zip(inv_pos, order) if c >= 2]
        at = np.searchsorted(idx, listed)
        assert np.array_equal(idx[at], listed)
        got = vals[at]
        assert len(got) == 63 and len({v.tobytes() for v in got}) == 63
        assert ints(got, R) == [expect[c] for c in order if c >= 2]
        assert all(c * e % R == 1 for c, e in enumerate(expect) if c)
        seen[name] = got
    assert seen["sweep"].tobytes() == seen["sweep_reversed"][::-1].tobytes()  # the same 63 values from other payload slots


@pytest.mark.parametrize("k", KS_LARGE)
def test_mirror_equals_host_pass_at_large_counts(k):
    zkg = _zkg()
    cases = large_cases(zkg, k)
    assert len(cases) >= 4 and len({w[1].size for _, w in cases.values()}) >= 2
    for name, (ctx, want) in cases.items():
        assert want[0].size == zkg.zklaim_witness_size(k)[0] and want[1].size <= zkg.zklaim_witness_size(k)[1]
        assert_same_witness(zkg.zklaim_witness_mirror(ctx), want, (k, name))


def test_full_circuit_anchors_the_host_pass_at_nine_payloads():
    """the witness-only pass is the reference of everything above: once above eight payloads it is held against the circuit builder itself"""
    zkg = _zkg()
    keep = []
    ctx = zkg.make_ctx(honest_payloads(9), keep)
    ck = zkg.ZklaimCircuit(ctx)
    wo = zkg.ZklaimCircuit(ctx, witness_only=True)
    try:
        assert ck.is_satisfied(), ck.first_unsatisfied()
        assert ck.r1cs.num_inputs == CLASS_ENDS[9][0] and ck.r1cs.num_variables == wo.r1cs.num_variables == zkg.zklaim_witness_size(9)[0]
        w = ck.witness()
        assert np.array_equal(wo.witness(), w)
        want = wo.sparse_witness()
        assert_same_witness(ck.sparse_witness(), want, "full circuit")
        assert np.array_equal(zkg.zklaim_input_map(ctx), w[:CLASS_ENDS[9][0]])
    finally:
        ck.free(); wo.free()
    rounds, _, _ = listed_per_round(9, want)
    assert len(rounds) == 2 and rounds[1] > 0
    assert_same_witness(zkg.zklaim_witness_mirror(ctx), want, "mirror")
    assert_same_witness(zkg.zklaim_witness_mirror_parallel(ctx), want, "parallel mirror")
    ctx.pl_ctx_head.contents.pl.data_ref[1] = 1                               # attribute 1 of payload 0 is 0, "eq": the statement no longer holds
    bad = zkg.ZklaimCircuit(ctx)
    try:
        assert not bad.is_satisfied()
    finally:
        bad.free()
