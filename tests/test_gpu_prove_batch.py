"""GPU parity: zkg_groth16_prove_batch (many proofs of one resident key as one launch sequence per chunk) against the oracle's
r1cs_gg_ppzksnark_prover and against the single-proof entry points.  Proof bytes are deterministic given (key, witness, r, s), so every
comparison is byte for byte; what ran batched is asserted through zkg_prove_batch_stats, not through a stopwatch."""
import threading

import numpy as np
import pytest

from gpu_util import credential_payloads, oracle_pk_from_keypair, zkg  # noqa: F401
from test_gpu_groth16 import _trivial_system
from util import R, arr, random_fr_canonical

pytestmark = pytest.mark.gpu
N_SYNTH = 3200            # C + l + 1 = 3202 -> basic_radix2_domain(4096), the batched path (2502 would be the step domain 2048 + 512: a key that falls back)


def _witness(rng, n, nonbit_positions):
    vals = [int(x) for x in rng.integers(0, 2, n)]
    for p_ in nonbit_positions:
        vals[p_] = int.from_bytes(rng.bytes(31), "little") % (R - 2) + 2
    return arr(vals, R)


def _synthetic_key(zkg, oracle, n, seed, keep):
    n_, l, A, B, C, _ = _trivial_system([0] * n)
    ocs = oracle.make_r1cs(n, l, A, B, C, keep)
    crs_arrays = oracle.groth16_setup(ocs, random_fr_canonical(5, seed))
    opk = oracle.make_pk(ocs, crs_arrays)
    m = crs_arrays["m"]
    crs = zkg.Crs(zkg.make_pk(zkg.make_r1cs(n, l, A, B, C, keep), crs_arrays, (m - 1).bit_length(), keep, domain_size=m))
    return crs, opk


def _to_sparse(w):
    """a dense witness in the form zkg_groth16_prove_sparse takes"""
    one = arr([1], R)[0]
    zero = ~w.any(axis=1); is_one = (w == one).all(axis=1)
    tags = np.where(zero, 0, np.where(is_one, 1, 2)).astype(np.uint8)
    idx = np.nonzero(tags == 2)[0].astype(np.uint32)
    return tags, idx, w[idx].copy()


@pytest.fixture(scope="module")
def synth(zkg, oracle):
    """one synthetic key (n = 3200, m = 4096) and 16 distinct witnesses with distinct (r, s) and their oracle proofs"""
    keep = []
    crs, opk = _synthetic_key(zkg, oracle, N_SYNTH, 0xB1, keep)
    assert zkg.evaluation_domain_size(N_SYNTH + 2) == (4096, False)
    rng = np.random.default_rng(41)
    cases = []
    for j in range(16):
        shape = list(range(7 * j, 2400, 11 + j)) if j % 4 else list(range(100 + j, 400, 3))
        w = _witness(rng, N_SYNTH, shape if j != 5 else [])                      # (one witness of bits only)
        rs = random_fr_canonical(2, 0xB200 + j)
        rc_o, proof_o = oracle.groth16_prove(opk, w, rs[0], rs[1])
        assert rc_o == 0
        cases.append((w, rs, proof_o))
    yield crs, opk, cases, keep
    crs.free()


@pytest.mark.parametrize("P", [1, 2, 3, 7, 16])
def test_batch_bytes_vs_oracle_synthetic(zkg, synth, P):
    crs, _, cases, _ = synth
    assert crs.prove_batch_chunk() > 0
    got = crs.prove_batch([(w, rs[0], rs[1]) for w, rs, _ in cases[:P]])
    assert [g[0] for g in got] == [0] * P
    for k, (g, c) in enumerate(zip(got, cases)):
        assert g[1] == c[2], k
    assert zkg.prove_batch_stats() == (P, 0, 1)


def test_batch_bytes_vs_oracle_credentials(zkg, oracle):
    """one real one-payload key, four credentials that differ in attributes and salt: the oracle's bytes, and the batch verifier accepts"""
    keep = []
    variants = [[dict(attrs=[1990 + 3 * v, 7 + v, 42 + v, v, 5 + v], refs=[2100, 7 + v, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x1000 + 77 * v)]
                for v in range(4)]
    cks = [zkg.ZklaimCircuit(zkg.make_ctx(pl, keep)) for pl in variants]
    assert all(ck.is_satisfied() for ck in cks)
    ck = cks[0]
    nv, l = ck.r1cs.num_variables, ck.r1cs.num_inputs
    kp = zkg.Keypair(ck.r1cs, random_fr_canonical(5, 0xC1))
    ocs, opk, m = oracle_pk_from_keypair(oracle, kp, ck.csr(), nv, l, keep)
    assert m == 1 << 15
    crs = zkg.Crs(kp.pk)
    ws = [c.witness() for c in cks]
    assert len({w.tobytes() for w in ws}) == 4 and len({w[:l].tobytes() for w in ws}) == 4
    rss = [random_fr_canonical(2, 0xC200 + v) for v in range(4)]
    got = crs.prove_batch([(w, rs[0], rs[1]) for w, rs in zip(ws, rss)])
    assert zkg.prove_batch_stats() == (4, 0, 1)
    for v in range(4):
        rc_o, proof_o = oracle.groth16_prove(opk, ws[v], rss[v][0], rss[v][1], True, oracle.num_threads())
        assert rc_o == 0 and got[v] == (0, proof_o), v
    vk = kp.vk_blob()
    assert list(zkg.groth16_verify_batch([(vk, ws[v][:l], got[v][1]) for v in range(4)])) == [0, 0, 0, 0]
    crs.free(); kp.free()
    for c in cks:
        c.free()


@pytest.mark.parametrize("k", [1, 2, 4])
def test_batch_bytes_vs_single_path_credentials(zkg, k):
    """k payloads (m = 2^15, 2^16, 2^17), eight items, dense and sparse mixed in one call"""
    keep = []
    cks = []
    for v in range(8):
        pls = credential_payloads(k)
        pls[0] = dict(pls[0], attrs=[1980 + v, 0, 42 + v, 0, 5], salt=0x2000 + v)
        cks.append(zkg.ZklaimCircuit(zkg.make_ctx(pls, keep)))
    assert all(ck.is_satisfied() for ck in cks)
    kp = zkg.Keypair(cks[0].r1cs, random_fr_canonical(5, 0xD1 + k))
    assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == 1 << (14 + k.bit_length())
    crs = zkg.Crs(kp.pk)
    assert crs.prove_batch_chunk() > 0
    rss = [random_fr_canonical(2, 0xD200 + 16 * k + v) for v in range(8)]
    items, expect = [], []
    for v, ck in enumerate(cks):
        r, s = rss[v]
        if v % 2:
            t, i, vals = ck.sparse_witness()
            items.append((t, i, vals, r, s)); expect.append(crs.prove_sparse(t, i, vals, r, s))
        else:
            w = ck.witness()
            items.append((w, r, s)); expect.append(crs.prove(w, r, s))
    assert all(e[0] == 0 and len(e[1]) == 134 for e in expect)
    got = crs.prove_batch(items)
    st = zkg.prove_batch_stats()
    assert st[0] == 8 and st[1] == 0
    assert got == expect
    crs.free(); kp.free()
    for c in cks:
        c.free()


def test_batch_per_item_failures(zkg):
    """an unsatisfied witness at position 2, a sparse item with a duplicated index at position 4: only they fail; a clean batch follows"""
    keep = []
    cks = [zkg.ZklaimCircuit(zkg.make_ctx([dict(credential_payloads(1)[0], salt=0x3000 + v)], keep)) for v in range(6)]
    kp = zkg.Keypair(cks[0].r1cs, random_fr_canonical(5, 0xE1))
    crs = zkg.Crs(kp.pk)
    nv = cks[0].r1cs.num_variables
    rss = [random_fr_canonical(2, 0xE200 + v) for v in range(6)]
    items = []
    for v, ck in enumerate(cks):
        r, s = rss[v]
        if v == 2:
            bad = ck.witness(); bad[nv - 1, 0] ^= np.uint64(1)
            items.append((bad, r, s))
        elif v == 4:
            t, i, vals = ck.sparse_witness()
            items.append((t, np.concatenate([i, i[:1]]), np.concatenate([vals, vals[:1]]), r, s))
        elif v % 2:
            items.append(ck.sparse_witness() + (r, s))
        else:
            items.append((ck.witness(), r, s))
    got = crs.prove_batch(items)
    assert [g[0] for g in got] == [0, 0, zkg.UNSATISFIED, 0, zkg.ERROR, 0]
    assert got[2][1] is None and got[4][1] is None
    single = {v: (crs.prove_sparse(*items[v]) if len(items[v]) == 5 else crs.prove(*items[v])) for v in (0, 1, 3, 5)}
    for v in (0, 1, 3, 5):
        assert got[v] == single[v], v
    clean = [items[v] for v in (5, 3, 1, 0)]
    assert crs.prove_batch(clean) == [single[v] for v in (5, 3, 1, 0)]
    assert crs.prove_batch(items, check_satisfied=False)[2][0] == 0               # without the gate the witness at 2 is proved like any other
    crs.free(); kp.free()
    for c in cks:
        c.free()


def test_batch_extends_the_witness_tables_once(zkg, oracle):
    """first call on a fresh key: a batch whose items have disjoint sets of non-bit positions; then their union and bits-only witnesses"""
    keep = []
    crs, opk = _synthetic_key(zkg, oracle, N_SYNTH, 0xF1, keep)
    rng = np.random.default_rng(43)
    first = list(range(100, 400, 3)); second = list(range(1000, 1900, 7)); third = [0, 1, N_SYNTH - 1]
    for call, shapes in enumerate(([first, second, third], [first + second + third, [], second, []])):
        ws = [_witness(rng, N_SYNTH, sh) for sh in shapes]
        rss = [random_fr_canonical(2, 0xF200 + 8 * call + j) for j in range(len(ws))]
        got = crs.prove_batch([(w, rs[0], rs[1]) for w, rs in zip(ws, rss)])
        assert zkg.prove_batch_stats() == (len(ws), 0, 1)
        for j, (w, rs) in enumerate(zip(ws, rss)):
            rc_o, proof_o = oracle.groth16_prove(opk, w, rs[0], rs[1])
            assert rc_o == 0 and got[j] == (0, proof_o), (call, j)
    crs.free()


def test_batch_is_cut_into_chunks(zkg, synth):
    crs, _, cases, _ = synth
    chunk = crs.prove_batch_chunk()
    P = 2 * chunk + 3
    items = []
    for j in range(P):
        w = cases[j % len(cases)][0]
        r, s = random_fr_canonical(2, 0xA100 + j)
        items.append(_to_sparse(w) + (r, s) if j % 3 == 1 else (w, r, s))
    got = crs.prove_batch(items)
    assert zkg.prove_batch_stats() == (P, 0, 3)
    for j, it in enumerate(items):
        assert got[j] == (crs.prove_sparse(*it) if len(it) == 5 else crs.prove(*it)), j


def test_batch_on_keys_that_fall_back(zkg):
    """an 8-payload key (m = 2^18) and a step-domain key (three payloads, m = 2^16 + 2^15): the same contract, whatever path serves it"""
    for k in (8, 3):
        keep = []
        cks = [zkg.ZklaimCircuit(zkg.make_ctx([dict(p, salt=p["salt"] + 0x100 * v) for p in credential_payloads(k)], keep)) for v in range(3)]
        kp = zkg.Keypair(cks[0].r1cs, random_fr_canonical(5, 0xA7 + k))
        m = kp.pk.domain_size or (1 << kp.pk.log_m)
        assert m == (1 << 18 if k == 8 else (1 << 16) + (1 << 15))
        crs = zkg.Crs(kp.pk)
        items = []
        for v, ck in enumerate(cks):
            r, s = random_fr_canonical(2, 0xA800 + 8 * k + v)
            items.append(ck.sparse_witness() + (r, s) if v == 1 else (ck.witness(), r, s))
        got = crs.prove_batch(items)
        st = zkg.prove_batch_stats()
        assert st[0] + st[1] == 3
        if crs.prove_batch_chunk() == 0:
            assert st == (0, 3, 0)
        for v, it in enumerate(items):
            assert got[v] == (crs.prove_sparse(*it) if len(it) == 5 else crs.prove(*it)), (k, v)
            assert got[v][0] == 0
        crs.free(); kp.free()
        for c in cks:
            c.free()


def test_batch_beside_other_callers(zkg, oracle):
    """one thread proves batches, two prove sparse witnesses one by one, on ONE fresh key, with witnesses whose non-bit positions force
    table extensions from both sides"""
    rng = np.random.default_rng(47)
    n = 1900                                                                     # (m = 2048, radix-2: the batches run batched)
    keep = []
    crs, opk = _synthetic_key(zkg, oracle, n, 0x91, keep)
    assert crs.prove_batch_chunk() > 0
    shapes = [list(range(a, b, st)) for a, b, st in ((0, 90, 3), (100, 400, 5), (400, 1200, 11), (3, 1100, 13), (50, 60, 1), (600, 1199, 2))]
    cases = []
    for j, shape in enumerate(shapes):
        w = _witness(rng, n, shape); rs = random_fr_canonical(2, 0x92 + j)
        rc_o, proof_o = oracle.groth16_prove(opk, w, rs[0], rs[1])
        assert rc_o == 0
        cases.append((w, rs, proof_o))
    errors = []

    def batch_caller():
        try:
            for order in ([0, 1, 2], [5, 3, 1, 4, 2, 0], [4, 5], [2, 4, 0, 5, 1, 3]):
                got = crs.prove_batch([(cases[j][0], cases[j][1][0], cases[j][1][1]) for j in order])
                for j, g in zip(order, got):
                    if g != (0, cases[j][2]):
                        errors.append(("batch", j, g[0]))
        except Exception as e:                                   # noqa: BLE001
            errors.append(repr(e))

    def single_caller(order):
        try:
            for rep in range(3):
                for j in order:
                    w, rs, expect = cases[j]
                    rc, proof = crs.prove_sparse(*_to_sparse(w), rs[0], rs[1])
                    if rc != 0 or proof != expect:
                        errors.append(("single", j, rc))
        except Exception as e:                                   # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=batch_caller), threading.Thread(target=single_caller, args=([5, 3, 1, 4, 2, 0],)),
               threading.Thread(target=single_caller, args=([2, 4, 0, 5, 1, 3],))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in threads), "a caller is stuck"
    assert not errors, errors[:5]
    crs.free()


def test_batch_argument_contract(zkg, synth):
    import ctypes as C
    crs, _, cases, _ = synth
    w, rs, proof = cases[0]
    assert crs.prove_batch([]) == [] and zkg.prove_batch_stats() == (0, 0, 0)     # count == 0: ZKG_OK, nothing touched
    L = zkg.lib()
    assert L.zkg_groth16_prove_batch(None, None, 0, 1, None, None) == zkg.OK
    out = np.zeros(134, np.uint8); status = np.full(1, -1, np.int32)
    item = zkg.api.ProveItem(w.ctypes.data, None, None, None, 0, rs.ctypes.data, rs[1:].ctypes.data)
    for args in ((None, C.byref(item), out.ctypes.data, status.ctypes.data), (C.c_void_p(crs._h), None, out.ctypes.data, status.ctypes.data),
                 (C.c_void_p(crs._h), C.byref(item), None, status.ctypes.data), (C.c_void_p(crs._h), C.byref(item), out.ctypes.data, None)):
        assert L.zkg_groth16_prove_batch(args[0], args[1], 1, 1, args[2], args[3]) == zkg.ERROR
    assert status[0] == -1 and not out.any()
    with pytest.raises(zkg.ZkgError):
        zkg.groth16_prove_batch(None, [(w, rs[0], rs[1])])
    with pytest.raises(zkg.ZkgError):
        crs.prove_batch([(w[:-1], rs[0], rs[1])])                                # a witness of the wrong length
    with pytest.raises(zkg.ZkgError):
        crs.prove_batch([(w, rs[0])])
    t, i, v = _to_sparse(w)
    with pytest.raises(zkg.ZkgError):
        crs.prove_batch([(t[:-1], i, v, rs[0], rs[1])])
    # a null (r, s) inside an item fails that item alone
    items = (zkg.api.ProveItem * 2)(zkg.api.ProveItem(w.ctypes.data, None, None, None, 0, None, None), item)
    out2 = np.zeros((2, 134), np.uint8); st2 = np.full(2, -1, np.int32)
    assert L.zkg_groth16_prove_batch(C.c_void_p(crs._h), C.cast(items, C.c_void_p), 2, 1, out2.ctypes.data, st2.ctypes.data) == zkg.OK
    assert list(st2) == [zkg.ERROR, zkg.OK] and out2[1].tobytes() == proof and not out2[0].any()
