"""GPU: zkg_groth16_prove_zklaim — ONE credential of a resident key proved with its witness generated on the GPU by k_zklaim_witness_par,
on every class of key the single-proof path serves.  Proof bytes are deterministic given (key, witness, r, s): every proof is compared byte
for byte with zkg_groth16_prove_sparse on the host witness of the same context, and who made the witness is asserted through
zkg_prove_zklaim_stats, never a clock."""
import json
import os
import subprocess
import sys
import threading

import pytest

from gpu_util import credential_payloads, zkg  # noqa: F401
from util import random_fr_canonical
from zklaim_witness_cases import N_SPECS, assert_same_witness, host_pass, payloads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOMAINS = {1: 1 << 15, 3: (1 << 16) + (1 << 15), 8: 1 << 18}      # radix-2; step domain; the class the batch leaves to the host


def _payloads(k, v, wrong_hash=False):
    pls = [dict(p, salt=0x7000 + 0x40 * k + 0x100 * v + i) for i, p in enumerate(credential_payloads(k))]
    pls[0] = dict(pls[0], attrs=[1970 + v, 0, 42 + v, 0, 5])
    if wrong_hash:
        pls[-1] = dict(pls[-1], hash=bytes((0x3C + b) & 0xFF for b in range(32)))
    return pls


# ---- the generator alone

@pytest.mark.parametrize("k,specs", [(1, range(N_SPECS)), (3, range(N_SPECS)), (8, [4])])
def test_parallel_generator_equals_host_pass(zkg, k, specs):
    keep = []
    good = [zkg.make_ctx(payloads(k, j), keep) for j in specs]
    batch = list(good)
    if len(good) > 1:                                                          # a null context and another payload count in the middle
        batch[5:5] = [None, zkg.make_ctx(payloads(k + 1, 2), keep)]
    got = zkg.zklaim_witness_gpu_parallel(batch)                               # (raises if a failed context's tags are not all zero)
    assert len(got) == len(batch)
    if len(good) > 1:
        assert got[5] is None and got[6] is None
        del got[5:7]
    listed = set()
    for j, c, g in zip(specs, good, got):
        want = host_pass(zkg, c)
        assert_same_witness(g, want, (k, j))
        listed.add(int(want[1].size))
    assert len(good) == 1 or len(listed) >= 2


# ---- proofs

_KEYS = {}


def _keyed(zkg, k):
    """a k-payload key with a fixed trapdoor, four credentials with (r, s), and what the single path gives for them on a SECOND Crs of the same
    key — the Crs under test has proved nothing when its first test reaches it.  Made once per module."""
    if k not in _KEYS:
        keep = []
        ck = zkg.ZklaimCircuit(zkg.make_ctx(_payloads(k, 0), keep))
        kp = zkg.Keypair(ck.r1cs, random_fr_canonical(5, 0x7A1 + k))
        assert (kp.pk.domain_size or (1 << kp.pk.log_m)) == DOMAINS[k]
        ctxs = [zkg.make_ctx(_payloads(k, v), keep) for v in range(4)]
        rss = [tuple(random_fr_canonical(2, 0x7A200 + 64 * k + v)) for v in range(4)]
        ref = zkg.Crs(kp.pk)
        expect = [ref.prove_sparse(*host_pass(zkg, c), r, s) for c, (r, s) in zip(ctxs, rss)]
        ref.free()
        assert all(e[0] == 0 and len(e[1]) == 134 for e in expect)
        crs = zkg.Crs(kp.pk)
        assert (crs.prove_batch_chunk() == 0) == (k == 8)
        _KEYS[k] = (crs, kp, ctxs, rss, expect, keep, ck)
    return _KEYS[k][:6]


@pytest.fixture(scope="module", autouse=True)
def _free_keys():
    yield
    for crs, kp, _, _, _, _, ck in _KEYS.values():
        crs.free(); kp.free(); ck.free()
    _KEYS.clear()


@pytest.mark.parametrize("k", sorted(DOMAINS))
def test_bytes_equal_the_single_path_on_the_host_witness(zkg, k):
    """first test on the fresh Crs: credential 0 is the first proof it ever makes (no witness tables yet: the extension branch)"""
    crs, kp, ctxs, rss, expect, _ = _keyed(zkg, k)
    vk = kp.vk_blob()
    for c, (r, s), e in list(zip(ctxs, rss, expect))[:3]:
        got = crs.prove_zklaim(c, r, s)
        assert zkg.prove_zklaim_stats() == (1, 0)
        assert got == e and len(got[1]) == 134
        assert got == crs.prove_sparse(*host_pass(zkg, c), r, s)
        assert zkg.groth16_verify(vk, zkg.zklaim_input_map(c), got[1]) == 0


@pytest.mark.parametrize("k", [1, 8])
def test_failures(zkg, k):
    crs, kp, ctxs, rss, expect, keep = _keyed(zkg, k)
    r, s = rss[3]
    false_hash = zkg.make_ctx(_payloads(k, 40, wrong_hash=True), keep)
    assert crs.prove_zklaim(false_hash, r, s) == (zkg.UNSATISFIED, None)
    assert zkg.prove_zklaim_stats() == (1, 0)
    assert crs.prove_sparse(*host_pass(zkg, false_hash), r, s)[0] == zkg.UNSATISFIED
    assert crs.prove_zklaim(zkg.make_ctx(_payloads(k + 1, 41), keep), r, s) == (zkg.ERROR, None)
    assert zkg.prove_zklaim_stats() == (0, 0)
    assert crs.prove_zklaim(None, r, s) == (zkg.ERROR, None)
    broken = zkg.make_ctx(_payloads(k, 42), keep)
    broken.pl_ctx_head = None                                                  # the list is shorter than num_of_payloads says
    assert crs.prove_zklaim(broken, r, s) == (zkg.ERROR, None)
    assert crs.prove_zklaim(ctxs[3], r, s) == expect[3] and zkg.prove_zklaim_stats() == (1, 0)


def test_three_callers_at_once(zkg):
    """the k = 1 key has three prover slots: three threads, four credentials each"""
    crs, kp, ctxs, rss, expect, _ = _keyed(zkg, 1)
    got = [[None] * 4 for _ in range(3)]

    def caller(t):
        for j in range(4):
            v = (t + j) % 4
            got[t][j] = (v, crs.prove_zklaim(ctxs[v], *rss[v]), zkg.prove_zklaim_stats())
    threads = [threading.Thread(target=caller, args=(t,)) for t in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    for row in got:
        for v, proof, stats in row:
            assert proof == expect[v] and stats == (1, 0)


def test_h_query_sharded(zkg):
    """zkg_crs_shard_h with device 0 listed twice rehearses the sharded H path on the k = 1 key"""
    crs, kp, ctxs, rss, expect, _ = _keyed(zkg, 1)
    crs.shard_h([0, 0])
    for v in (1, 2):
        assert crs.prove_zklaim(ctxs[v], *rss[v]) == expect[v] and zkg.prove_zklaim_stats() == (1, 0)
    crs.shard_h([0])
    assert crs.prove_zklaim(ctxs[0], *rss[0]) == expect[0]


# ---- the seam

SEAM_SCRIPT = r"""
import json, sys
sys.path[:0] = [%r, %r]
import zklaim_amd as zkg
from test_gpu_prove_zklaim import seam_run
zkg.init(0)
print("RESULT " + json.dumps(seam_run(zkg)))
zkg.shutdown()
"""


def seam_run(zkg):
    """libsnark_prove at k = 1 and k = 8 on a key that ARRIVES AS A BLOB (the key the setup left resident is dropped first): a good and a false
    context each, the good one's proof verified, and who made its witness"""
    out = {}
    for k in (1, 8):
        keep = []
        owner = zkg.make_ctx(_payloads(k, 0), keep)
        assert zkg.libsnark_trusted_setup(owner) == 0 and owner.pk_size > 0
        zkg.lib().zkg_compat_reset()                                           # the prover holds the blob only
        good, false = zkg.make_ctx(_payloads(k, 1), keep), zkg.make_ctx(_payloads(k, 2, wrong_hash=True), keep)
        for c in (good, false):
            c.pk, c.pk_size, c.vk, c.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
        rc_good = zkg.libsnark_prove(good)
        stats = zkg.prove_zklaim_stats()
        verdict = zkg.libsnark_verify(good) if good.proof else None
        rc_false = zkg.libsnark_prove(false)
        again = zkg.libsnark_prove(good)                                       # the key is resident now: the digest-confirmed path
        out[str(k)] = dict(rc=[rc_good, rc_false, again], verdict=verdict, stats=list(stats), stats_again=list(zkg.prove_zklaim_stats()), false_has_proof=bool(false.proof))
        zkg.lib().zkg_compat_reset()
    return out


def test_seam_makes_the_witness_on_the_gpu_and_the_switch_keeps_the_host_pass(zkg):
    here = seam_run(zkg)
    for k in ("1", "8"):
        assert here[k] == dict(rc=[0, 1, 0], verdict=0, stats=[1, 0], stats_again=[1, 0], false_has_proof=False), k
    env = dict(os.environ, ZKG_SEAM_GPU_WITNESS="0")
    out = subprocess.run([sys.executable, "-c", SEAM_SCRIPT % (ROOT, os.path.join(ROOT, "tests"))], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    for k in ("1", "8"):
        assert child[k] == dict(rc=[0, 1, 0], verdict=0, stats=[0, 1], stats_again=[0, 1], false_has_proof=False), k
