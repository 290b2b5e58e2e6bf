"""GPU parity: zkg_prover (proofs queued on the caller's stream, witnesses, (r, s), proofs and status all in device memory) against the
oracle's r1cs_gg_ppzksnark_prover and against zkg_groth16_prove_dev / _batch_dev on the same buffers.  Proof bytes are deterministic given
(key, witness, r, s), so every comparison is byte for byte; groups and host waits are asserted through zkg_prover_stats, not a stopwatch.
Device buffers are torch tensors."""
import threading

import numpy as np
import pytest

from gpu_util import credential_payloads, oracle_pk_from_keypair, zkg  # noqa: F401
from test_gpu_prove_batch import _synthetic_key, _witness
from test_gpu_prove_dev import _dev, _edge_witnesses
from util import R, random_fr_canonical

pytestmark = pytest.mark.gpu
N_TINY = 300              # 8-bit tables; C + l + 1 = 302 lands on the step domain 256 + 64
N_TINY_RADIX2 = 400       # 8-bit tables, m = 512
N_SMALL = 1900            # 12-bit tables, m = 2048
N_STEP = 2500             # step domain 2048 + 512
FILL = 0xA5
FF = np.uint64(0xFFFFFFFFFFFFFFFF)


def _edges(n, seed):
    """test_gpu_prove_dev._edge_witnesses where its positions fit; below that the shapes that do: bits only, no bits, the lane and workgroup edges"""
    if n > 701:
        return _edge_witnesses(n, seed)
    rng = np.random.default_rng(seed)
    return {"mixed": _witness(rng, n, list(range(7, 3 * n // 4, 11))), "bits_only": _witness(rng, n, []), "no_bits": _witness(rng, n, list(range(n))),
            "lane_and_workgroup_edges": _witness(rng, n, [0, 62, 63, 254, 255, n - 1]),
            "full_wavefront_beside_an_empty_one": _witness(rng, n, list(range(127, 191)))}


def _rs_array(rss):
    return np.ascontiguousarray(np.concatenate([np.concatenate([r, s]) for r, s in rss]), np.uint64).reshape(len(rss), 8)


def _prove(prover, ws, rss, stride=None, proof_stride=134, check=True, stream=0, d_w=None):
    """one call and a synchronise -> (status (count,), proofs (count, proof_stride) with the gaps as pre-filled)"""
    import torch
    count, n = len(ws), ws[0].shape[0]
    stride = stride or n
    if d_w is None:
        buf = np.full((count, stride, 4), FF, np.uint64)                         # the padding between n and the stride is never read
        for j, w in enumerate(ws):
            buf[j, :n] = w
        d_w = _dev(buf)
    d_rs = _dev(_rs_array(rss))
    d_pr = torch.full((count * proof_stride,), FILL, dtype=torch.uint8, device="cuda")
    d_st = torch.full((count,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    prover.prove_async(d_w.data_ptr(), stride, count, d_rs.data_ptr(), d_pr.data_ptr(), proof_stride, d_st.data_ptr(), check, stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_pr.cpu().numpy().reshape(count, proof_stride)


@pytest.mark.parametrize("n", [N_TINY, N_TINY_RADIX2, N_SMALL, N_STEP])
def test_single_keys_bytes_vs_oracle_and_prove_dev(zkg, oracle, n):
    keep = []
    crs, opk = _synthetic_key(zkg, oracle, n, 0xA500 + n, keep)
    assert zkg.evaluation_domain_size(n + 2) == {N_TINY: (320, True), N_TINY_RADIX2: (512, False), N_SMALL: (2048, False), N_STEP: (2560, True)}[n]
    prover = zkg.Prover(crs)
    try:
        assert prover.batch_max() >= 1
        ws = _edges(n, 0xA0 + n)
        names = list(ws)
        rss = [tuple(random_fr_canonical(2, 0xA600 + 16 * (n % 251) + j)) for j in range(len(names))]
        status, proofs = _prove(prover, [ws[k] for k in names], rss)
        assert zkg.prover_stats()[0] == len(names)
        for j, name in enumerate(names):
            rc_o, proof_o = oracle.groth16_prove(opk, ws[name], rss[j][0], rss[j][1])
            assert rc_o == 0 and status[j] == 0, name
            assert proofs[j].tobytes() == proof_o, name
            d = _dev(ws[name])
            assert crs.prove_dev(d.data_ptr(), rss[j][0], rss[j][1]) == (0, proof_o), name
        # one proof per call: the single-vector launches
        status, proofs1 = _prove(prover, [ws[names[0]]], rss[:1])
        assert status[0] == 0 and proofs1[0].tobytes() == proofs[0].tobytes()
    finally:
        prover.free(); crs.free()


@pytest.fixture(scope="module")
def small(zkg, oracle):
    """one key (n = 1900) with a prover handle, nine witnesses and their prove_batch_dev proofs"""
    keep = []
    crs, opk = _synthetic_key(zkg, oracle, N_SMALL, 0xA5B1, keep)
    rng = np.random.default_rng(59)
    ws = [_witness(rng, N_SMALL, list(range(5 * j, 1500, 9 + j)) if j != 4 else []) for j in range(9)]
    rss = [tuple(random_fr_canonical(2, 0xA5B200 + j)) for j in range(9)]
    d = _dev(np.stack(ws))
    rc, want = crs.prove_batch_dev(d.data_ptr(), N_SMALL, 9, rss)
    assert rc == 0 and all(st == 0 for st, _ in want)
    rc_o, proof_o = oracle.groth16_prove(opk, ws[0], rss[0][0], rss[0][1])
    assert rc_o == 0 and want[0][1] == proof_o
    prover = zkg.Prover(crs)
    yield crs, prover, ws, rss, [p for _, p in want]
    prover.free(); crs.free()


@pytest.mark.parametrize("count", [1, 3, 4, 9])
def test_batches_in_groups_of_three(zkg, small, count):
    crs, prover, ws, rss, want = small
    n = N_SMALL
    prover.set_batch_max(3)
    assert prover.batch_max() == 3
    try:
        for stride, proof_stride in ((n, 134), (n + 5, 160)):
            status, proofs = _prove(prover, ws[:count], rss[:count], stride, proof_stride)
            done, groups, _ = zkg.prover_stats()
            assert (done, groups) == (count, -(-count // 3))
            assert list(status) == [0] * count
            for j in range(count):
                assert proofs[j, :134].tobytes() == want[j], (count, j)
            assert (proofs[:, 134:] == FILL).all()                               # bytes between ZKG_PROOF_BYTES and proof_stride are never written
        _prove(prover, ws[:count], rss[:count])
        assert zkg.prover_stats() == (count, -(-count // 3), 0)                  # a group size the handle has served: no host wait
    finally:
        prover.set_batch_max(0)
    assert prover.batch_max() >= 3


def test_the_call_stays_on_the_callers_stream_and_does_not_wait_on_the_host(zkg, small):
    """witnesses and (r, s) are written by copies queued on a side stream behind ~0.1 s of queued work; the call returns while that stream is
    still busy, having waited for nothing, and copies queued on the same stream afterwards see proofs and status"""
    import torch
    crs, prover, ws, rss, want = small
    count = 2
    src_w = _dev(np.stack(ws[:count])); src_rs = _dev(_rs_array(rss[:count]))
    _prove(prover, ws[:count], rss[:count])                                     # warm: this group size is served
    side = torch.cuda.Stream()
    d_w = torch.zeros_like(src_w); d_rs = torch.zeros_like(src_rs)
    d_pr = torch.full((count * 134,), FILL, dtype=torch.uint8, device="cuda"); d_st = torch.full((count,), 7, dtype=torch.int32, device="cuda")
    h_pr = torch.empty((count * 134,), dtype=torch.uint8).pin_memory(); h_st = torch.empty((count,), dtype=torch.int32).pin_memory()
    torch.cuda.synchronize()
    can_sleep = hasattr(torch.cuda, "_sleep")
    if can_sleep:                                                               # cycles per millisecond of the sleep kernel's counter, measured on a short one
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            e0.record(); torch.cuda._sleep(2_000_000); e1.record()
        side.synchronize()
        per_ms = 2_000_000 / max(e0.elapsed_time(e1), 1e-3)
    with torch.cuda.stream(side):
        if can_sleep:
            torch.cuda._sleep(int(100 * per_ms))
        d_w.copy_(src_w, non_blocking=True); d_rs.copy_(src_rs, non_blocking=True)
    prover.prove_async(d_w.data_ptr(), N_SMALL, count, d_rs.data_ptr(), d_pr.data_ptr(), 134, d_st.data_ptr(), True, side.cuda_stream)
    busy = not side.query()
    stats = zkg.prover_stats()
    with torch.cuda.stream(side):
        h_pr.copy_(d_pr, non_blocking=True); h_st.copy_(d_st, non_blocking=True)
    side.synchronize()
    if can_sleep:
        assert busy, "the call returned only after the side stream had drained"
    assert stats == (count, 1, 0)
    assert list(h_st.numpy()) == [0] * count
    assert [h_pr.numpy().reshape(count, 134)[j].tobytes() for j in range(count)] == want[:count]


def test_two_streams_on_one_handle_and_a_synchronous_prove_beside_them(zkg, small):
    import torch
    crs, prover, ws, rss, want = small
    _prove(prover, ws[:3], rss[:3])                                             # warm
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    picks = [[0, 1, 2], [5, 6, 7]]
    bufs = []
    for pick in picks:
        bufs.append((_dev(np.stack([ws[j] for j in pick])), _dev(_rs_array([rss[j] for j in pick])),
                     torch.full((3 * 134,), FILL, dtype=torch.uint8, device="cuda"), torch.full((3,), 7, dtype=torch.int32, device="cuda")))
    d8 = _dev(ws[8])
    torch.cuda.synchronize()
    beside = []
    th = threading.Thread(target=lambda: beside.append(crs.prove_dev(d8.data_ptr(), rss[8][0], rss[8][1])))
    th.start()
    for st, (dw, drs, dpr, dst) in zip(streams, bufs):
        prover.prove_async(dw.data_ptr(), N_SMALL, 3, drs.data_ptr(), dpr.data_ptr(), 134, dst.data_ptr(), True, st.cuda_stream)
    th.join()
    for st in streams:
        st.synchronize()
    assert beside == [(0, want[8])]
    for pick, (_, _, dpr, dst) in zip(picks, bufs):
        assert list(dst.cpu().numpy()) == [0, 0, 0]
        got = dpr.cpu().numpy().reshape(3, 134)
        assert [got[k].tobytes() for k in range(3)] == [want[j] for j in pick]


@pytest.fixture(scope="module")
def cred1(zkg):
    """a one-payload credential key (12-bit tables, m = 2^15), four credentials, a prover handle"""
    keep = []
    cks = [zkg.ZklaimCircuit(zkg.make_ctx([dict(credential_payloads(1)[0], salt=0x3700 + v)], keep)) for v in range(4)]
    kp = zkg.Keypair(cks[0].r1cs, random_fr_canonical(5, 0xA5E1))
    assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == 1 << 15
    crs = zkg.Crs(kp.pk)
    prover = zkg.Prover(crs)
    yield crs, prover, kp, cks, [ck.witness() for ck in cks], [tuple(random_fr_canonical(2, 0xA5E200 + v)) for v in range(4)], keep
    prover.free(); crs.free(); kp.free()
    for c in cks:
        c.free()


def test_one_payload_credentials(zkg, oracle, cred1):
    crs, prover, kp, cks, ws, rss, keep = cred1
    nv, l = cks[0].r1cs.num_variables, cks[0].r1cs.num_inputs
    d = _dev(np.stack(ws))
    rc, want = crs.prove_batch_dev(d.data_ptr(), nv, 4, rss)
    assert rc == 0
    status, proofs = _prove(prover, ws, rss)
    assert list(status) == [0] * 4 and zkg.prover_stats()[:2] == (4, 1)
    assert [(0, proofs[v].tobytes()) for v in range(4)] == want
    _, opk, m = oracle_pk_from_keypair(oracle, kp, cks[0].csr(), nv, l, keep)
    rc_o, proof_o = oracle.groth16_prove(opk, ws[1], rss[1][0], rss[1][1], True, oracle.num_threads())
    assert rc_o == 0 and proofs[1].tobytes() == proof_o


def test_unsatisfied_item_fails_alone(zkg, cred1):
    """one limb of item 2's last variable is flipped on the device copy: status 2, its proof bytes stay as pre-filled, the neighbours' are
    prove_dev's; without the check the bytes are prove_dev's without the check"""
    import torch
    crs, prover, kp, cks, ws, rss, keep = cred1
    nv = cks[0].r1cs.num_variables
    d = _dev(np.stack(ws))
    d[2, nv - 1, 0] ^= 1
    torch.cuda.synchronize()
    bad = ws[2].copy(); bad[nv - 1, 0] ^= np.uint64(1)
    assert np.array_equal(d[2].cpu().numpy().view(np.uint64), bad)
    status, proofs = _prove(prover, ws, rss, proof_stride=160, d_w=d)
    assert list(status) == [0, 0, zkg.UNSATISFIED, 0]
    assert (proofs[2] == FILL).all()                                             # nothing is written for the failed item
    for v in (0, 1, 3):
        assert crs.prove_dev(d[v].data_ptr(), rss[v][0], rss[v][1]) == (0, proofs[v, :134].tobytes()), v
    status, proofs = _prove(prover, ws, rss, check=False, d_w=d)
    assert list(status) == [0, 0, 0, 0]
    assert crs.prove_dev(d[2].data_ptr(), rss[2][0], rss[2][1], check_satisfied=False) == (0, proofs[2].tobytes())


def test_two_payload_credentials_at_the_default_group(zkg):
    """16-bit tables, H's windows merged in pairs (65535 points), m = 2^16"""
    keep = []
    cks = []
    for v in range(2):
        pls = credential_payloads(2)
        pls[0] = dict(pls[0], salt=0x3800 + v)
        cks.append(zkg.ZklaimCircuit(zkg.make_ctx(pls, keep)))
    kp = zkg.Keypair(cks[0].r1cs, random_fr_canonical(5, 0xA5F1))
    assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == 1 << 16
    crs = zkg.Crs(kp.pk)
    prover = zkg.Prover(crs)
    try:
        nv = cks[0].r1cs.num_variables
        assert nv >= 1 << 15 and prover.batch_max() >= 2
        ws = [ck.witness() for ck in cks]
        rss = [tuple(random_fr_canonical(2, 0xA5F200 + v)) for v in range(2)]
        d = _dev(np.stack(ws))
        rc, want = crs.prove_batch_dev(d.data_ptr(), nv, 2, rss)
        assert rc == 0
        status, proofs = _prove(prover, ws, rss)
        assert list(status) == [0, 0] and zkg.prover_stats()[:2] == (2, 1)
        assert [(0, proofs[v].tobytes()) for v in range(2)] == want
    finally:
        prover.free(); crs.free(); kp.free()
        for c in cks:
            c.free()


def test_refusals_write_nothing(zkg, small):
    import torch
    crs, prover, ws, rss, want = small
    n = N_SMALL
    d_w = _dev(np.stack(ws[:2])); d_rs = _dev(_rs_array(rss[:2]))
    d_pr = torch.full((2 * 134 + 64,), FILL, dtype=torch.uint8, device="cuda"); d_st = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    h_w = np.ascontiguousarray(np.stack(ws[:2])); h_pinned = torch.zeros((2 * n * 4,), dtype=torch.int64).pin_memory()
    wp, rp, pp, sp = d_w.data_ptr(), d_rs.data_ptr(), d_pr.data_ptr(), d_st.data_ptr()

    def refused(*args):
        with pytest.raises(zkg.ZkgError):
            prover.prove_async(*args)
        torch.cuda.synchronize()
        assert (d_pr == FILL).all() and (d_st == 7).all()
        assert zkg.prover_stats() == (0, 0, 0)

    refused(0, n, 2, rp, pp, 134, sp)                                           # null arguments
    refused(wp, n, 2, 0, pp, 134, sp)
    refused(wp, n, 2, rp, 0, 134, sp)
    refused(wp, n, 2, rp, pp, 134, 0)
    refused(wp, n - 1, 2, rp, pp, 134, sp)                                      # stride < n
    refused(wp, n, 2, rp, pp, 133, sp)                                          # proof_stride < ZKG_PROOF_BYTES
    refused(wp, n, (1 << 24) + 1, rp, pp, 134, sp)                              # too many items
    refused(wp, (1 << 32) + 1, 2, rp, pp, 134, sp)                              # stride above 2^32
    refused(h_w.ctypes.data, n, 2, rp, pp, 134, sp)                             # host memory, pinned memory
    refused(h_pinned.data_ptr(), n, 2, rp, pp, 134, sp)
    refused(wp, n, 2, h_w.ctypes.data, pp, 134, sp)
    refused(wp, n, 2, rp, h_pinned.data_ptr(), 134, sp)
    refused(wp, n, 2, rp, pp, 134, h_pinned.data_ptr())
    refused(wp + 8, n, 1, rp, pp, 134, sp)                                      # misaligned: 16 bytes for witnesses and (r, s), 4 for the status
    refused(wp, n, 2, rp + 8, pp, 134, sp)
    refused(wp, n, 2, rp, pp, 134, sp + 2)
    refused(wp, 1 << 31, 2, rp, pp, 134, sp)                                    # the second witness lies beyond the allocation
    # (r, s), proofs and status that run past an allocation of their own (12 MiB is a size the caching allocator neither rounds nor, with its
    # cache emptied, carves out of a larger block)
    torch.cuda.empty_cache()
    big = torch.full((12 << 20,), FILL, dtype=torch.uint8, device="cuda")
    end = big.data_ptr() + (12 << 20)
    refused(wp, n, 2, end - 64, pp, 134, sp)
    refused(wp, n, 2, rp, end - 200, 134, sp)
    refused(wp, n, 2, rp, pp, 134, end - 4)
    assert (big == FILL).all()
    del big
    refused(wp, n, 2, wp + n * 32, pp, 134, sp)                                 # overlapping ranges
    refused(wp, n, 2, rp, wp + 64, 134, sp)
    refused(wp, n, 2, rp, pp, 134, pp + 200)
    if torch.cuda.device_count() > 1:                                           # a calling thread on another device than the key's
        torch.cuda.set_device(1)
        try:
            refused(wp, n, 2, rp, pp, 134, sp)
        finally:
            torch.cuda.set_device(0)
    prover.prove_async(wp, n, 0, rp, pp, 134, sp)                               # an empty call is fine and touches nothing
    torch.cuda.synchronize()
    assert (d_pr == FILL).all() and (d_st == 7).all()
    d_pr1 = torch.full((2 * 134 + 1,), FILL, dtype=torch.uint8, device="cuda")  # no alignment is asked of d_proofs
    torch.cuda.synchronize()
    prover.prove_async(wp, n, 2, rp, d_pr1.data_ptr() + 1, 134, sp)
    torch.cuda.synchronize()
    got = d_pr1.cpu().numpy()
    assert got[0] == FILL and [got[1 + 134 * j:1 + 134 * (j + 1)].tobytes() for j in range(2)] == want[:2]
    assert list(d_st.cpu().numpy()[:2]) == [0, 0]


def test_h_shards_and_prover_handles_exclude_each_other(zkg, oracle):
    keep = []
    crs, _ = _synthetic_key(zkg, oracle, N_TINY, 0xA5C1, keep)
    prover = zkg.Prover(crs)
    with pytest.raises(zkg.ZkgError, match="live zkg_prover"):
        crs.shard_h([0, 0])
    prover.free()
    crs.shard_h([0, 0])                                                         # the handle is gone: the key may be sharded
    with pytest.raises(zkg.ZkgError, match="sharded"):
        zkg.Prover(crs)
    crs.free()
