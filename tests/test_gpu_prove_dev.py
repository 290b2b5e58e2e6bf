"""GPU parity: zkg_groth16_prove_dev / zkg_groth16_prove_batch_dev (witnesses that are already in device memory, split there by k_split_dev)
against the oracle's r1cs_gg_ppzksnark_prover and against the host-witness entries on a host copy of the same vector.  Proof bytes are
deterministic given (key, witness, r, s), so every comparison is byte for byte; which path served a call is asserted through
zkg_prove_dev_stats and zkg_prove_batch_stats, not through a stopwatch.  Device buffers are torch int64 tensors."""
import ctypes as C
import threading

import numpy as np
import pytest

from gpu_util import credential_payloads, zkg  # noqa: F401
from test_gpu_prove_batch import _synthetic_key, _to_sparse, _witness
from util import R, arr, random_fr_canonical
from zklaim_witness_cases import host_pass

pytestmark = pytest.mark.gpu
N_BATCH = 3200            # m = 4096, radix-2, batched: z has 3201 elements, one lane in the last wavefront
N_SMALL = 1900            # m = 2048: 1901 = 29 x 64 + 45
N_STEP = 2500             # step domain 2048 + 512
FF = np.uint64(0xFFFFFFFFFFFFFFFF)


def _dev(a):
    """a numpy uint64 array as a torch int64 tensor on the GPU (as gpu_util makes its device buffers)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _raw_single(zkg, crs, d_ptr, r, s, check=1, stream=0):
    L = zkg.lib()
    L.zkg_groth16_prove_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    out = np.zeros(256, np.uint8); ln = C.c_size_t(0)
    rc = L.zkg_groth16_prove_dev(C.c_void_p(crs._h), C.c_void_p(d_ptr), r.ctypes.data, s.ctypes.data, check, out.ctypes.data, C.byref(ln), C.c_void_p(stream))
    return rc, out, ln.value


def _raw_batch(zkg, crs, d_ptr, stride, count, rs, check=1, proofs=True, status=True, stream=0):
    """the C entry with the caller's own output arrays: -> (rc, proofs (count x 134), status)"""
    L = zkg.lib()
    L.zkg_groth16_prove_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    out = np.zeros((count, 134), np.uint8); st = np.full(count, -1, np.int32)
    rs_a = None if rs is None else np.ascontiguousarray(np.concatenate([np.concatenate([r, s]) for r, s in rs]), np.uint64)
    rc = L.zkg_groth16_prove_batch_dev(C.c_void_p(crs._h), C.c_void_p(d_ptr), stride, count, None if rs_a is None else rs_a.ctypes.data, check,
                                       out.ctypes.data if proofs else None, st.ctypes.data if status else None, C.c_void_p(stream))
    return rc, out, st


def _edge_witnesses(n, seed):
    """name -> witness: the split kernel's lane, wavefront and workgroup edges, and the values its tag rule must not take for a bit"""
    rng = np.random.default_rng(seed)
    one = arr([1], R)[0]
    ws = {}
    ws["mixed"] = _witness(rng, n, list(range(7, 3 * n // 4, 11)))
    ws["mixed_dense_head"] = _witness(rng, n, list(range(100, 400, 3)))
    ws["bits_only"] = _witness(rng, n, [])
    ws["no_bits"] = _witness(rng, n, list(range(n)))
    # z position = variable + 1: these sit on both sides of z positions 63 | 64 and 255 | 256, at the first variable and at the last
    ws["lane_and_workgroup_edges"] = _witness(rng, n, [0, 62, 63, 254, 255, n - 1])
    # z positions 128 .. 191 (one whole wavefront) are non-bits, z positions 192 .. 255 (the next one) hold bits only
    ws["full_wavefront_beside_an_empty_one"] = _witness(rng, n, list(range(127, 191)))
    w = _witness(rng, n, [])
    w[700] = [0, 0, 0, 1]                                                        # only the top limb is non-zero: below r, neither 0 nor 1
    w[701] = one; w[701, 3] ^= np.uint64(1)                                      # Montgomery one with bit 0 of its top limb flipped: below r, not 1
    assert w[701, 3] < np.uint64(0x30644e72e131a029)
    ws["values_that_are_almost_bits"] = w
    return ws


@pytest.mark.parametrize("n", [N_BATCH, N_SMALL, N_STEP])
def test_single_bytes_vs_oracle_and_host_entry(zkg, oracle, n):
    """a fresh key each (its first call is a prove_dev that has to build the witness tables), every edge witness: the oracle's bytes, the
    host entry's bytes on the host copy, and the counters say the caller's buffer was split in place"""
    keep = []
    crs, opk = _synthetic_key(zkg, oracle, n, 0x5D00 + n, keep)
    assert zkg.evaluation_domain_size(n + 2) == {N_BATCH: (4096, False), N_SMALL: (2048, False), N_STEP: (2560, True)}[n]
    for j, (name, w) in enumerate(_edge_witnesses(n, 0xD0 + n).items()):
        r, s = random_fr_canonical(2, 0x5E00 + 16 * (n % 251) + j)
        rc_o, proof_o = oracle.groth16_prove(opk, w, r, s)
        assert rc_o == 0, name
        d = _dev(w)
        got = crs.prove_dev(d.data_ptr(), r, s)
        assert zkg.prove_dev_stats() == (1, 0), name
        assert got == (0, proof_o), name
        assert crs.prove(w, r, s) == (0, proof_o), name
    crs.free()


@pytest.fixture(scope="module")
def synth(zkg, oracle):
    """one synthetic key (n = 3200, m = 4096) and 16 distinct witnesses with distinct (r, s) and their oracle proofs; the key's first proof
    is whichever test below runs first"""
    keep = []
    crs, opk = _synthetic_key(zkg, oracle, N_BATCH, 0x5DB1, keep)
    rng = np.random.default_rng(53)
    cases = []
    for j in range(16):
        shape = list(range(7 * j, 2400, 11 + j)) if j % 4 else list(range(100 + j, 400, 3))
        w = _witness(rng, N_BATCH, shape if j != 5 else [])                      # (one witness of bits only)
        rs = random_fr_canonical(2, 0x5DB200 + j)
        rc_o, proof_o = oracle.groth16_prove(opk, w, rs[0], rs[1])
        assert rc_o == 0
        cases.append((w, rs, proof_o))
    yield crs, opk, cases, keep
    crs.free()


@pytest.mark.parametrize("size", ["1", "3", "chunk", "chunk+1", "2*chunk+3"])
def test_batch_bytes_vs_host_batch_and_oracle(zkg, synth, size):
    crs, _, cases, _ = synth
    n = N_BATCH
    chunk = crs.prove_batch_chunk()
    assert chunk > 0
    P = {"1": 1, "3": 3, "chunk": chunk, "chunk+1": chunk + 1, "2*chunk+3": 2 * chunk + 3}[size]
    ws = [cases[j % 16][0] for j in range(P)]
    rss = [cases[j][1] if j < 16 else random_fr_canonical(2, 0x5DC000 + j) for j in range(P)]
    results = []
    for stride in (n, n + 5):
        buf = np.full((P, stride, 4), FF, np.uint64)                             # the padding between n and the stride is never read
        for j, w in enumerate(ws):
            buf[j, :n] = w
        d = _dev(buf)
        rc, got = crs.prove_batch_dev(d.data_ptr(), stride, P, [(rs[0], rs[1]) for rs in rss])
        assert rc == 0
        assert zkg.prove_batch_stats() == (P, 0, -(-P // chunk))
        assert zkg.prove_dev_stats() == (P, 0)
        results.append(got)
    assert results[0] == results[1]
    host = crs.prove_batch([(w, rs[0], rs[1]) for w, rs in zip(ws, rss)])
    assert [g[0] for g in host] == [0] * P
    assert results[0] == host
    for j in range(min(P, 16)):
        assert results[0][j] == (0, cases[j][2]), j


def test_batch_unsatisfied_item_fails_alone(zkg):
    """four credentials of one one-payload key; one limb of item 2's last variable is flipped on the device copy"""
    import torch
    keep = []
    cks = [zkg.ZklaimCircuit(zkg.make_ctx([dict(credential_payloads(1)[0], salt=0x3500 + v)], keep)) for v in range(4)]
    kp = zkg.Keypair(cks[0].r1cs, random_fr_canonical(5, 0x5DE1))
    crs = zkg.Crs(kp.pk)
    nv = cks[0].r1cs.num_variables
    ws = [ck.witness() for ck in cks]
    rss = [random_fr_canonical(2, 0x5DE200 + v) for v in range(4)]
    d = _dev(np.stack(ws))
    d[2, nv - 1, 0] ^= 1
    torch.cuda.synchronize()
    bad = ws[2].copy(); bad[nv - 1, 0] ^= np.uint64(1)
    assert np.array_equal(d[2].cpu().numpy().view(np.uint64), bad)
    rc, proofs, status = _raw_batch(zkg, crs, d.data_ptr(), nv, 4, rss)
    assert rc == 0 and list(status) == [0, 0, zkg.UNSATISFIED, 0]
    assert not proofs[2].any()                                                   # nothing is written for the failed item
    assert zkg.prove_dev_stats() == (4, 0)
    for v in (0, 1, 3):
        assert crs.prove(ws[v], rss[v][0], rss[v][1]) == (0, proofs[v].tobytes()), v
    rc, got = crs.prove_batch_dev(d.data_ptr(), nv, 4, rss, check_satisfied=False)
    assert rc == 0 and got[2] == crs.prove(bad, rss[2][0], rss[2][1], check_satisfied=False) and got[2][0] == 0
    assert [g[1] for g in got[:2] + got[3:]] == [proofs[v].tobytes() for v in (0, 1, 3)]
    rc1, out1, ln1 = _raw_single(zkg, crs, d[2].data_ptr(), rss[2][0], rss[2][1])      # the single entry refuses it the same way
    assert rc1 == zkg.UNSATISFIED and ln1 == 0 and not out1.any()
    crs.free(); kp.free()
    for c in cks:
        c.free()


def test_three_sources_one_driver_across_a_chunk_boundary(zkg):
    """chunk + 1 credentials of a one-payload key (m = 2^15, the smallest zklaim key that batches): two chunks, the second of one item.  The
    same credentials and the same (r, s) through prove_batch (host sparse witnesses), prove_batch_zklaim (contexts, witnesses generated on
    the device) and prove_batch_dev (the mirror's witnesses, expanded and copied to the device): one chunk driver, three sources, the
    same bytes and the same chunk counts"""
    keep = []
    payloads = lambda v: [dict(credential_payloads(1)[0], salt=0x3600 + v)]      # noqa: E731
    ck = zkg.ZklaimCircuit(zkg.make_ctx(payloads(0), keep))
    kp = zkg.Keypair(ck.r1cs, random_fr_canonical(5, 0x5DF1))
    assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == 1 << 15
    crs = zkg.Crs(kp.pk)
    chunk = crs.prove_batch_chunk()
    assert chunk > 0
    P, n = chunk + 1, ck.r1cs.num_variables
    ctxs = [zkg.make_ctx(payloads(v), keep) for v in range(P)]
    rss = [tuple(random_fr_canonical(2, 0x5DF200 + v)) for v in range(P)]
    host = crs.prove_batch([(*host_pass(zkg, c), r, s) for c, (r, s) in zip(ctxs, rss)])
    assert zkg.prove_batch_stats() == (P, 0, 2)
    assert all(g[0] == 0 and len(g[1]) == 134 for g in host)
    gen = crs.prove_batch_zklaim(ctxs, rss)
    assert zkg.prove_batch_stats() == (P, 0, 2) and zkg.zklaim_witness_stats() == (P, 0)
    dense = np.zeros((P, n, 4), np.uint64)
    for j, c in enumerate(ctxs):
        tags, idx, vals = zkg.zklaim_witness_mirror(c)
        dense[j, tags == 1] = arr([1], R)[0]
        dense[j, idx] = vals
    d = _dev(dense)
    rc, dev = crs.prove_batch_dev(d.data_ptr(), n, P, rss)
    assert rc == 0 and zkg.prove_batch_stats() == (P, 0, 2) and zkg.prove_dev_stats() == (P, 0)
    assert gen == host and dev == host
    crs.free(); kp.free(); ck.free()


def test_batch_on_keys_that_do_not_batch(zkg, oracle):
    """an 8-payload key (m = 2^18: one proof fills the chip, the items go through the single _dev path) and the step-domain key: the same
    contract, whatever path serves it"""
    keep = []
    cks = [zkg.ZklaimCircuit(zkg.make_ctx([dict(p, salt=p["salt"] + 0x100 * v) for p in credential_payloads(8)], keep)) for v in range(3)]
    kp = zkg.Keypair(cks[0].r1cs, random_fr_canonical(5, 0x5DA7))
    assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == 1 << 18
    big = zkg.Crs(kp.pk)
    step, _ = _synthetic_key(zkg, oracle, N_STEP, 0x5DA8, keep)
    rng = np.random.default_rng(59)
    step_ws = [_witness(rng, N_STEP, sh) for sh in (list(range(0, 2500, 9)), [], [0, 63, 2499])]
    for crs, ws in ((big, [ck.witness() for ck in cks]), (step, step_ws)):
        n = ws[0].shape[0]
        rss = [random_fr_canonical(2, 0x5DA900 + 8 * (n % 97) + v) for v in range(3)]
        d = _dev(np.stack(ws))
        rc, got = crs.prove_batch_dev(d.data_ptr(), n, 3, rss)
        st = zkg.prove_batch_stats()
        assert rc == 0 and st[0] + st[1] == 3 and zkg.prove_dev_stats() == (3, 0)
        if crs.prove_batch_chunk() == 0:
            assert st == (0, 3, 0)
        for v in range(3):
            assert got[v] == crs.prove(ws[v], rss[v][0], rss[v][1]) and got[v][0] == 0, (n, v)
    assert big.prove_batch_chunk() == 0
    big.free(); step.free(); kp.free()
    for c in cks:
        c.free()


def test_ordering_behind_the_callers_stream(zkg, synth):
    """six witnesses through ONE device buffer: each is filled by a non-blocking copy from pinned memory on a side stream whose handle the
    call gets, and the buffer is refilled as soon as the call returns; then the same on the null stream"""
    import torch
    crs, _, cases, _ = synth
    pinned = [torch.from_numpy(w.view(np.int64)).pin_memory() for w, _, _ in cases[:6]]
    d = torch.zeros((N_BATCH, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for j in range(6):
        with torch.cuda.stream(side):
            d.copy_(pinned[j], non_blocking=True)
        r, s = cases[j][1]
        assert crs.prove_dev(d.data_ptr(), r, s, stream=side.cuda_stream) == (0, cases[j][2]), j
    side.synchronize()
    for j in (3, 0, 5):
        d.copy_(pinned[j], non_blocking=True)                                    # torch's current stream here is the null stream
        torch.cuda.synchronize()
        r, s = cases[j][1]
        assert crs.prove_dev(d.data_ptr(), r, s, stream=0) == (0, cases[j][2]), j
    # and the batch entry: two items written on the side stream
    d2 = torch.zeros((2, N_BATCH, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d2[0].copy_(pinned[4], non_blocking=True); d2[1].copy_(pinned[1], non_blocking=True)
    rc, got = crs.prove_batch_dev(d2.data_ptr(), N_BATCH, 2, [cases[4][1], cases[1][1]], stream=side.cuda_stream)
    assert rc == 0 and got == [(0, cases[4][2]), (0, cases[1][2])]
    side.synchronize()


def test_refusals_that_cannot_fault(zkg, synth):
    """every refusal here is decided before a launch, and none of the pointers could fault if the check were missing: pinned memory is
    readable by the GPU"""
    import torch
    crs, _, cases, _ = synth
    w, rs, proof = cases[0]
    n = N_BATCH
    pinned = torch.from_numpy(np.stack([w, w]).view(np.int64)).pin_memory()
    rc, out, ln = _raw_single(zkg, crs, pinned.data_ptr(), rs[0], rs[1])
    assert rc == zkg.ERROR and ln == 0 and not out.any()
    assert zkg.prove_dev_stats() == (0, 0)
    rc, proofs, status = _raw_batch(zkg, crs, pinned.data_ptr(), n, 2, [rs, rs])
    assert rc == zkg.ERROR and not proofs.any() and list(status) == [-1, -1]
    d = _dev(np.stack([w, w]))
    rc, proofs, status = _raw_batch(zkg, crs, d.data_ptr(), n - 1, 2, [rs, rs])   # stride < n
    assert rc == zkg.ERROR and not proofs.any() and list(status) == [-1, -1]
    for kw in (dict(rs=None), dict(rs=[rs, rs], status=False), dict(rs=[rs, rs], proofs=False)):
        rc, proofs, status = _raw_batch(zkg, crs, d.data_ptr(), n, 2, kw.pop("rs"), **kw)
        assert rc == zkg.ERROR and not proofs.any() and list(status) == [-1, -1]
    assert _raw_batch(zkg, crs, 0, n, 2, [rs, rs])[0] == zkg.ERROR                # a null witness pointer
    L = zkg.lib()
    out = np.zeros(256, np.uint8); ln = C.c_size_t(0)
    for args in ((None, rs[1].ctypes.data, out.ctypes.data, C.byref(ln)), (rs[0].ctypes.data, None, out.ctypes.data, C.byref(ln)),
                 (rs[0].ctypes.data, rs[1].ctypes.data, None, C.byref(ln)), (rs[0].ctypes.data, rs[1].ctypes.data, out.ctypes.data, None)):
        assert L.zkg_groth16_prove_dev(C.c_void_p(crs._h), C.c_void_p(d.data_ptr()), args[0], args[1], 1, args[2], args[3], None) == zkg.ERROR
    assert not out.any() and ln.value == 0
    # and the buffer itself is fine
    rc, proofs, status = _raw_batch(zkg, crs, d.data_ptr(), n, 2, [rs, rs])
    assert rc == 0 and list(status) == [0, 0] and proofs[0].tobytes() == proof and proofs[1].tobytes() == proof


def test_dev_entries_beside_other_callers(zkg, oracle):
    """one thread proves device batches, one proves sparse host witnesses, one proves device witnesses one by one, on ONE fresh key, with
    witnesses whose non-bit positions force table extensions from every side"""
    import torch
    rng = np.random.default_rng(61)
    n = N_SMALL
    keep = []
    crs, opk = _synthetic_key(zkg, oracle, n, 0x5D91, keep)
    assert crs.prove_batch_chunk() > 0
    shapes = [list(range(a, b, st)) for a, b, st in ((0, 90, 3), (100, 400, 5), (400, 1200, 11), (3, 1100, 13), (50, 60, 1), (600, 1199, 2))]
    cases = []
    for j, shape in enumerate(shapes):
        w = _witness(rng, n, shape); rs = random_fr_canonical(2, 0x5D92 + j)
        rc_o, proof_o = oracle.groth16_prove(opk, w, rs[0], rs[1])
        assert rc_o == 0
        cases.append((w, rs, proof_o))
    d_all = _dev(np.stack([c[0] for c in cases]))
    orders = ([0, 1, 2], [5, 3, 1, 4, 2, 0], [4, 5], [2, 4, 0, 5, 1, 3])
    d_orders = [d_all[torch.tensor(order, device="cuda")].contiguous() for order in orders]
    torch.cuda.synchronize()
    errors = []

    def batch_caller():
        try:
            for order, d in zip(orders, d_orders):
                rc, got = crs.prove_batch_dev(d.data_ptr(), n, len(order), [cases[j][1] for j in order])
                if rc != 0:
                    errors.append(("batch", rc))
                for j, g in zip(order, got):
                    if g != (0, cases[j][2]):
                        errors.append(("batch", j, g[0]))
        except Exception as e:                                   # noqa: BLE001
            errors.append(repr(e))

    def single_caller(order, dev):
        try:
            for rep in range(3):
                for j in order:
                    w, rs, expect = cases[j]
                    rc, proof = crs.prove_dev(d_all[j].data_ptr(), rs[0], rs[1]) if dev else crs.prove_sparse(*_to_sparse(w), rs[0], rs[1])
                    if rc != 0 or proof != expect:
                        errors.append(("dev" if dev else "sparse", j, rc))
        except Exception as e:                                   # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=batch_caller), threading.Thread(target=single_caller, args=([5, 3, 1, 4, 2, 0], False)),
               threading.Thread(target=single_caller, args=([2, 4, 0, 5, 1, 3], True))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in threads), "a caller is stuck"
    assert not errors, errors[:5]
    crs.free()
