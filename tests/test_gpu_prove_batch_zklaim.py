"""GPU: zkg_groth16_prove_batch_zklaim — credentials of one resident key proved as batches whose witnesses the GPU generates.  Proof bytes
are deterministic given (key, witness, r, s): every proof is compared byte for byte with zkg_groth16_prove_sparse on the host witness
of the same context, and who made the witnesses is asserted through zkg_zklaim_witness_stats / zkg_prove_batch_stats, never a clock."""
import json
import os
import subprocess
import sys

import pytest

from gpu_util import credential_payloads, zkg  # noqa: F401
from util import random_fr_canonical
from zklaim_witness_cases import host_pass

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOMAINS = {1: 1 << 15, 3: (1 << 16) + (1 << 15), 4: 1 << 17}


def _payloads(k, v, wrong_hash=False):
    pls = [dict(p, salt=0x6000 + 0x40 * k + 0x100 * v + i) for i, p in enumerate(credential_payloads(k))]
    pls[0] = dict(pls[0], attrs=[1970 + v, 0, 42 + v, 0, 5])
    if wrong_hash:
        pls[-1] = dict(pls[-1], hash=bytes((0x3C + b) & 0xFF for b in range(32)))
    return pls


@pytest.fixture(scope="module", params=sorted(DOMAINS))
def keyed(request, zkg):
    """a k-payload key from zkg_groth16_setup with a fixed trapdoor, chunk + 3 credentials with (r, s) and their single-path proofs"""
    k = request.param
    keep = []
    ck = zkg.ZklaimCircuit(zkg.make_ctx(_payloads(k, 0), keep))
    kp = zkg.Keypair(ck.r1cs, random_fr_canonical(5, 0x6A1 + k))
    assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == DOMAINS[k]
    crs = zkg.Crs(kp.pk)
    chunk = crs.prove_batch_chunk()
    assert chunk == (16 if k == 1 else 8)
    ctxs = [zkg.make_ctx(_payloads(k, v), keep) for v in range(chunk + 3)]
    rss = [tuple(random_fr_canonical(2, 0x6A200 + 64 * k + v)) for v in range(chunk + 3)]
    expect = [crs.prove_sparse(*host_pass(zkg, c), r, s) for c, (r, s) in zip(ctxs, rss)]
    assert all(e[0] == 0 and len(e[1]) == 134 for e in expect)
    yield k, crs, kp, chunk, ctxs, rss, expect, keep
    crs.free(); kp.free(); ck.free()


@pytest.mark.parametrize("which", ["1", "chunk", "chunk+3"])
def test_bytes_equal_the_single_path(zkg, keyed, which):
    k, crs, kp, chunk, ctxs, rss, expect, _ = keyed
    P = {"1": 1, "chunk": chunk, "chunk+3": chunk + 3}[which]
    first = 2 if which == "1" else 0
    got = crs.prove_batch_zklaim(ctxs[first:first + P], rss[first:first + P])
    ws, st = zkg.zklaim_witness_stats(), zkg.prove_batch_stats()
    assert got == expect[first:first + P]
    assert ws == (P, 0) and st == (P, 0, -(-P // chunk))
    vk = kp.vk_blob()
    for c, g in zip(ctxs[first:first + P], got):
        assert zkg.groth16_verify(vk, zkg.zklaim_input_map(c), g[1]) == 0


def test_failures_stay_with_their_item(zkg, keyed):
    k, crs, kp, chunk, ctxs, rss, expect, keep = keyed
    false_hash = zkg.make_ctx(_payloads(k, 40, wrong_hash=True), keep)
    other_count = zkg.make_ctx(_payloads(k + 1, 41), keep)
    batch = [ctxs[0], false_hash, ctxs[1], other_count, None, ctxs[2]]
    rs = [rss[0], rss[5], rss[1], rss[6], rss[7], rss[2]]
    got = crs.prove_batch_zklaim(batch, rs)
    assert [g[0] for g in got] == [0, zkg.UNSATISFIED, 0, zkg.ERROR, zkg.ERROR, 0]
    assert got[1][1] is None and got[3][1] is None and got[4][1] is None
    assert [got[0], got[2], got[5]] == expect[:3]
    assert zkg.zklaim_witness_stats() == (6, 0) and zkg.prove_batch_stats()[:2] == (6, 0)
    # the single path agrees about the false credential
    assert crs.prove_sparse(*host_pass(zkg, false_hash), *rss[5])[0] == zkg.UNSATISFIED
    assert crs.prove_batch_zklaim([], []) == []


def test_eight_payloads_take_host_witnesses_and_the_single_path(zkg):
    keep = []
    ctxs = [zkg.make_ctx(_payloads(8, v), keep) for v in range(3)]
    ck = zkg.ZklaimCircuit(ctxs[0])
    kp = zkg.Keypair(ck.r1cs, random_fr_canonical(5, 0x6B7))
    assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == 1 << 18
    crs = zkg.Crs(kp.pk)
    assert crs.prove_batch_chunk() == 0
    rss = [tuple(random_fr_canonical(2, 0x6B800 + v)) for v in range(3)]
    other_count = zkg.make_ctx(_payloads(1, 50), keep)
    got = crs.prove_batch_zklaim(ctxs + [other_count], rss + [rss[0]])
    assert zkg.zklaim_witness_stats() == (0, 3) and zkg.prove_batch_stats() == (0, 3, 0)
    assert got[3] == (zkg.ERROR, None)
    for c, (r, s), g in zip(ctxs, rss, got):
        assert g[0] == 0 and g == crs.prove_sparse(*host_pass(zkg, c), r, s)
        assert zkg.groth16_verify(kp.vk_blob(), zkg.zklaim_input_map(c), g[1]) == 0
    crs.free(); kp.free(); ck.free()


SEAM_SCRIPT = r"""
import json, sys
sys.path[:0] = [%r, %r]
import zklaim_amd as zkg
from test_gpu_prove_batch_zklaim import seam_run
zkg.init(0)
print("RESULT " + json.dumps(seam_run(zkg)))
zkg.shutdown()
"""


def seam_run(zkg):
    """16 one-payload contexts and a false one through zkg_zklaim_prove_batch on a key that ARRIVES AS A BLOB: the key the setup left
    resident is dropped first, so the batch parses ctx->pk itself, confirms nothing by digest and meets a key that has proved nothing yet
    (no witness tables: the chunk's extension branch).  Beside it, libsnark_prove on fresh copies of all 17 contexts."""
    keep = []
    owner = zkg.make_ctx(_payloads(1, 0), keep)
    assert zkg.libsnark_trusted_setup(owner) == 0 and owner.pk_size > 0
    zkg.lib().zkg_compat_reset()                                               # the prover holds the blob only

    def contexts():
        out = []
        for v in range(17):
            c = zkg.make_ctx(_payloads(1, v, wrong_hash=(v == 11)), keep)
            c.pk, c.pk_size, c.vk, c.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
            out.append(c)
        return out
    ctxs = contexts()
    rc = zkg.zklaim_prove_batch(ctxs)
    ws, st = zkg.zklaim_witness_stats(), zkg.prove_batch_stats()
    verdicts = [zkg.libsnark_verify(c) if c.proof else None for c in ctxs]
    again = zkg.zklaim_prove_batch(contexts())                                 # the key is resident now: the digest-confirmed path
    ws2 = zkg.zklaim_witness_stats()
    single = [zkg.libsnark_prove(c) for c in contexts()]
    zkg.lib().zkg_compat_reset()
    return dict(rc=rc, witness_stats=list(ws), batch_stats=list(st), verdicts=verdicts, again=again, witness_stats_again=list(ws2), single=single)


def test_seam_uses_gpu_witnesses_and_the_switch_keeps_the_host_ones(zkg):
    here = seam_run(zkg)
    want_rc = [1 if v == 11 else 0 for v in range(17)]
    assert here["single"] == want_rc                                           # what libsnark_prove gives for each of them
    assert here["rc"] == here["single"] and here["again"] == here["single"]
    assert here["verdicts"] == [None if v == 11 else 0 for v in range(17)]
    assert here["witness_stats"] == [17, 0] and here["batch_stats"][:2] == [17, 0] and here["witness_stats_again"] == [17, 0]
    env = dict(os.environ, ZKG_SEAM_GPU_WITNESS="0")
    out = subprocess.run([sys.executable, "-c", SEAM_SCRIPT % (ROOT, os.path.join(ROOT, "tests"))], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert child["single"] == want_rc and child["rc"] == child["single"] and child["again"] == child["single"]
    assert child["verdicts"] == here["verdicts"]
    assert child["witness_stats"] == [0, 17] and child["batch_stats"][:2] == [17, 0] and child["witness_stats_again"] == [0, 17]
