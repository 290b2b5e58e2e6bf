"""GPU: libsnark_trusted_setup generates through zkg_groth16_setup_resident's core with every scalar computed on the device.  On a
one-payload context (m = 2^15) and a three-payload one (step domain, m = 2^16 + 2^15): the counters say device scalars and nothing
uploaded; the B query's non-zero count is the blob's and is min(columns A touches, columns B touches) of the circuit (the generator stores
the smaller side in B; a touched column summing to zero at a random t has negligible probability); the seam proves and verifies; the blob
loaded afresh proves the host witness; and an issuer-only child process produces blobs with the same counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import credential_payloads, zkg  # noqa: F401
from util import random_fr_canonical

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOMAIN = {1: 1 << 15, 3: (1 << 16) + (1 << 15)}


def seam_setup(zkg, k, keep):
    """-> (ctx after libsnark_trusted_setup, its counters, what pk_blob_inspect says of ctx.pk)"""
    ctx = zkg.make_ctx(credential_payloads(k), keep)
    assert zkg.libsnark_trusted_setup(ctx) == 0 and ctx.pk_size > 0 and ctx.vk_size > 0
    return ctx, zkg.setup_resident_stats(), zkg.pk_blob_inspect(zkg.ctx_blob(ctx, "pk"))


ISSUER_SCRIPT = r"""
import json, sys
sys.path[:0] = [%r, %r]
import zklaim_amd as zkg
from test_gpu_seam_keygen_dev import seam_setup
zkg.init(0)
out = {}
for k in (1, 3):
    keep = []
    ctx, stats, info = seam_setup(zkg, k, keep)
    out[str(k)] = dict(stats=stats, info=info, vk_size=ctx.vk_size)
print("RESULT " + json.dumps(out))
zkg.shutdown()
"""


@pytest.fixture(scope="module")
def seam_keys(zkg):
    keep, out = [], {}
    for k in (1, 3):
        out[k] = seam_setup(zkg, k, keep)
    yield out
    zkg.lib().zkg_compat_reset()


@pytest.mark.parametrize("k", [1, 3])
def test_the_seam_generates_with_device_scalars(zkg, seam_keys, k):
    ctx, stats, info = seam_keys[k]
    assert info["domain_size"] == DOMAIN[k]
    assert stats[0] == 1 and stats[2] == 0
    assert stats[1] == info["B_values"]
    ck = zkg.ZklaimCircuit(ctx)
    try:
        A, B, _ = ck.csr()
        assert stats[1] == min(np.unique(A[1]).size, np.unique(B[1]).size)       # column 0 counts like any other
        assert zkg.libsnark_prove(ctx) == 0 and ctx.proof_size == 134
        assert zkg.libsnark_verify(ctx) == 0
        fresh = zkg.Crs(blob=zkg.ctx_blob(ctx, "pk"))
        try:
            rs = random_fr_canonical(2, 0x5EA + k)
            rc, proof = fresh.prove(ck.witness(), rs[0], rs[1])
            assert rc == 0
            assert zkg.groth16_verify(zkg.ctx_blob(ctx, "vk"), zkg.zklaim_input_map(ctx), proof) == 0
        finally:
            fresh.free()
    finally:
        ck.free()


def test_an_issuer_only_process_produces_the_blobs_with_the_same_counters(zkg, seam_keys):
    env = dict(os.environ, ZKG_SEAM_ISSUER_ONLY="1")
    out = subprocess.run([sys.executable, "-c", ISSUER_SCRIPT % (ROOT, os.path.join(ROOT, "tests"))], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    for k in (1, 3):
        ctx, stats, info = seam_keys[k]
        assert child[str(k)] == dict(stats=stats, info=info, vk_size=ctx.vk_size), k
