"""GPU parity: zkg_groth16_prove_batch on keys whose evaluation domain is a step_radix2_domain (m = 2^a + 2^b < 2^18).  The chunk's
transforms are the fold / unfold passes around a 2^a and a 2^b radix-2 transform, with the proof dimension, and the H launch runs over
m - 1 scalars that are not 2^k - 1.  Proof bytes are deterministic given (key, witness, r, s): every comparison is byte for byte against
the oracle's prover or the single-proof entry points, and what ran batched is asserted through zkg_prove_batch_stats, never a clock."""
import threading

import numpy as np
import pytest

from gpu_util import credential_payloads, oracle_pk_from_keypair, zkg  # noqa: F401
from test_gpu_prove_batch import _synthetic_key, _to_sparse, _witness
from util import random_fr_canonical

pytestmark = pytest.mark.gpu

# n variables of _trivial_system give C + l + 1 = n + 2 -> (domain, big / small)
SYNTH_SHAPES = {2500: (2048 + 512, 4), 3000: (2048 + 1024, 2), 4200: (4096 + 128, 32)}      # 32 > 16: the chunked fold / unfold
STEP_PAYLOADS = {3: (1 << 16) + (1 << 15), 5: (1 << 17) + (1 << 13), 6: (1 << 17) + (1 << 16), 7: (1 << 17) + (1 << 16)}
N_CASES = 19                                                                                 # chunk + 3 at the chunk of these sizes (16)


@pytest.fixture(scope="module", params=sorted(SYNTH_SHAPES))
def synth_step(request, zkg, oracle):
    """one synthetic step-domain key and 19 distinct witnesses with distinct (r, s) and their oracle proofs"""
    n = request.param
    m, compr = SYNTH_SHAPES[n]
    assert zkg.evaluation_domain_size(n + 2) == (m, True)
    keep = []
    crs, opk = _synthetic_key(zkg, oracle, n, 0x51 + n, keep)
    assert crs.m == m
    rng = np.random.default_rng(53 + n)
    cases = []
    for j in range(N_CASES):
        shape = list(range(7 * j, n - 100, 11 + j)) if j % 4 else list(range(100 + j, 400, 3))   # distinct non-bit positions per item
        w = _witness(rng, n, shape if j != 5 else [])                                            # (one witness of bits only)
        rs = random_fr_canonical(2, 0x5200 + 32 * (n % 97) + j)
        rc_o, proof_o = oracle.groth16_prove(opk, w, rs[0], rs[1])
        assert rc_o == 0
        cases.append((w, rs, proof_o))
    yield crs, n, cases, keep
    crs.free()


@pytest.mark.parametrize("which", ["1", "2", "3", "chunk", "chunk+3"])
def test_step_batch_bytes_vs_oracle_synthetic(zkg, synth_step, which):
    crs, n, cases, _ = synth_step
    chunk = crs.prove_batch_chunk()
    assert chunk > 0
    P = {"1": 1, "2": 2, "3": 3, "chunk": chunk, "chunk+3": chunk + 3}[which]
    assert P <= len(cases)
    items = [(_to_sparse(w) + (rs[0], rs[1])) if j % 3 == 1 else (w, rs[0], rs[1]) for j, (w, rs, _) in enumerate(cases[:P])]   # dense and sparse mixed
    got = crs.prove_batch(items)
    st = zkg.prove_batch_stats()
    assert [g[0] for g in got] == [0] * P
    for k, (g, c) in enumerate(zip(got, cases)):
        assert g[1] == c[2], (n, k)
    assert st == (P, 0, -(-P // chunk))


@pytest.mark.parametrize("k", sorted(STEP_PAYLOADS))
def test_step_batch_bytes_vs_single_path_credentials(zkg, oracle, k):
    """k payloads on a step domain below 2^18, eight items, dense and sparse alternating; at three payloads also the oracle's bytes and
    the batch verifier's verdict"""
    keep = []
    cks = []
    for v in range(8):
        pls = credential_payloads(k)
        pls[0] = dict(pls[0], attrs=[1980 + v, 0, 42 + v, 0, 5], salt=0x2000 + v)
        cks.append(zkg.ZklaimCircuit(zkg.make_ctx(pls, keep)))
    assert all(ck.is_satisfied() for ck in cks)
    kp = zkg.Keypair(cks[0].r1cs, random_fr_canonical(5, 0x5D1 + k))
    assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == STEP_PAYLOADS[k]
    crs = zkg.Crs(kp.pk)
    assert crs.prove_batch_chunk() > 0
    rss = [random_fr_canonical(2, 0x5D200 + 16 * k + v) for v in range(8)]
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
    if k == 3:
        nv, l = cks[0].r1cs.num_variables, cks[0].r1cs.num_inputs
        ocs, opk, m = oracle_pk_from_keypair(oracle, kp, cks[0].csr(), nv, l, keep)
        ws = [ck.witness() for ck in cks]
        for v in range(8):
            rc_o, proof_o = oracle.groth16_prove(opk, ws[v], rss[v][0], rss[v][1], True, oracle.num_threads())
            assert rc_o == 0 and got[v] == (0, proof_o), v
        vk = kp.vk_blob()
        assert list(zkg.groth16_verify_batch([(vk, ws[v][:l], got[v][1]) for v in range(8)])) == [0] * 8
    crs.free(); kp.free()
    for c in cks:
        c.free()


def test_step_batch_per_item_failures(zkg):
    """three payloads: the witness of a false statement at position 2, a sparse item with a duplicated index at position 4: only they fail; a
    clean batch follows"""
    keep = []
    cks = []
    for v in range(6):
        pls = [dict(p, salt=0x3000 + 16 * v + i) for i, p in enumerate(credential_payloads(3))]
        if v == 2:
            pls[1] = dict(pls[1], ops=["greater", "eq", "greater", "noop", "greater_or_eq"])          # 1991 > 2100 is false
        cks.append(zkg.ZklaimCircuit(zkg.make_ctx(pls, keep)))
    assert [ck.is_satisfied() for ck in cks] == [True, True, False, True, True, True]
    kp = zkg.Keypair(cks[0].r1cs, random_fr_canonical(5, 0x5E1))
    assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == STEP_PAYLOADS[3]
    crs = zkg.Crs(kp.pk)
    assert crs.prove_batch_chunk() > 0
    rss = [random_fr_canonical(2, 0x5E200 + v) for v in range(6)]
    items = []
    for v, ck in enumerate(cks):
        r, s = rss[v]
        if v == 4:
            t, i, vals = ck.sparse_witness()
            items.append((t, np.concatenate([i, i[:1]]), np.concatenate([vals, vals[:1]]), r, s))
        elif v % 2:
            items.append(ck.sparse_witness() + (r, s))
        else:
            items.append((ck.witness(), r, s))
    got = crs.prove_batch(items)
    assert zkg.prove_batch_stats()[:2] == (6, 0)
    assert [g[0] for g in got] == [0, 0, zkg.UNSATISFIED, 0, zkg.ERROR, 0]
    assert got[2][1] is None and got[4][1] is None
    single = {v: (crs.prove_sparse(*items[v]) if len(items[v]) == 5 else crs.prove(*items[v])) for v in (0, 1, 3, 5)}
    for v in (0, 1, 3, 5):
        assert single[v][0] == 0 and got[v] == single[v], v
    clean = [items[v] for v in (5, 3, 1, 0)]
    assert crs.prove_batch(clean) == [single[v] for v in (5, 3, 1, 0)]
    assert zkg.prove_batch_stats()[:2] == (4, 0)
    crs.free(); kp.free()
    for c in cks:
        c.free()


def test_step_batch_beside_other_callers(zkg, oracle):
    """one thread proves batches, two prove sparse witnesses one by one, on ONE fresh step-domain key, with witnesses whose non-bit
    positions force table extensions from both sides"""
    rng = np.random.default_rng(59)
    n = 2500                                                                     # (m = 2048 + 512: the batches run batched)
    keep = []
    assert zkg.evaluation_domain_size(n + 2) == (2560, True)
    crs, opk = _synthetic_key(zkg, oracle, n, 0x591, keep)
    assert crs.prove_batch_chunk() > 0
    shapes = [list(range(a, b, st)) for a, b, st in ((0, 90, 3), (100, 400, 5), (400, 1200, 11), (3, 1100, 13), (50, 60, 1), (600, 2399, 2))]
    cases = []
    for j, shape in enumerate(shapes):
        w = _witness(rng, n, shape); rs = random_fr_canonical(2, 0x592 + j)
        rc_o, proof_o = oracle.groth16_prove(opk, w, rs[0], rs[1])
        assert rc_o == 0
        cases.append((w, rs, proof_o))
    errors = []
    batched = []

    def batch_caller():
        try:
            for order in ([0, 1, 2], [5, 3, 1, 4, 2, 0], [4, 5], [2, 4, 0, 5, 1, 3]):
                got = crs.prove_batch([(cases[j][0], cases[j][1][0], cases[j][1][1]) for j in order])
                batched.append(zkg.prove_batch_stats()[:2] == (len(order), 0))
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
    assert batched == [True] * 4
    crs.free()


def test_eight_payloads_still_fall_back(zkg):
    """m = 2^18: one proof fills the chip, the key reports chunk 0 and its items take the single-proof path"""
    keep = []
    cks = [zkg.ZklaimCircuit(zkg.make_ctx([dict(p, salt=p["salt"] + 0x100 * v) for p in credential_payloads(8)], keep)) for v in range(3)]
    kp = zkg.Keypair(cks[0].r1cs, random_fr_canonical(5, 0x5A7))
    assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == 1 << 18
    crs = zkg.Crs(kp.pk)
    assert crs.prove_batch_chunk() == 0
    items = []
    for v, ck in enumerate(cks):
        r, s = random_fr_canonical(2, 0x5A800 + v)
        items.append(ck.sparse_witness() + (r, s) if v == 1 else (ck.witness(), r, s))
    got = crs.prove_batch(items)
    assert zkg.prove_batch_stats() == (0, 3, 0)
    for v, it in enumerate(items):
        assert got[v] == (crs.prove_sparse(*it) if len(it) == 5 else crs.prove(*it)), v
        assert got[v][0] == 0
    crs.free(); kp.free()
    for c in cks:
        c.free()
