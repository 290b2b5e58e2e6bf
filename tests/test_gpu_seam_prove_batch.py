"""GPU: zkg_zklaim_prove_batch, many libsnark_prove calls in one.  Contexts of one key become one zkg_groth16_prove_batch; proofs draw
fresh (r, s), so the checks are return codes, libsnark_verify's verdicts and the batch counters (zkg_prove_batch_stats), as the
reference's own tests check the seam."""
import ctypes as C

import pytest

from gpu_util import credential_payloads, zkg  # noqa: F401

pytestmark = pytest.mark.gpu


def _payloads(k, v, ok=True):
    """k satisfiable payloads that differ per v in attributes and salt; ok=False: the first statement (attr0 < 2100) is false"""
    pls = credential_payloads(k)
    pls[0] = dict(pls[0], attrs=[(1980 if ok else 2200) + v, 0, 42 + v, 0, 5], salt=0x7000 + 0x10 * k + v)
    return pls


def _key(zkg, k, keep):
    """libsnark_trusted_setup on a k-payload ctx -> that ctx (it owns pk / vk)"""
    ctx = zkg.make_ctx(_payloads(k, 0), keep)
    assert zkg.libsnark_trusted_setup(ctx) == 0 and ctx.pk_size > 0 and ctx.vk_size > 0
    return ctx


def _ctx_on(zkg, owner, pls, keep):
    """a ctx of its own (own payloads, own ctx->proof) sharing the owner's pk / vk"""
    c = zkg.make_ctx(pls, keep)
    c.pk, c.pk_size, c.vk, c.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
    return c


def _swap_public(a, b):
    """exchange the proofs of two contexts"""
    a.proof, b.proof = b.proof, a.proof


@pytest.mark.parametrize("k", [3, 1])
def test_six_contexts_of_one_key(zkg, k):
    """k = 3: a step domain (2^16 + 2^15); k = 1: radix-2 (2^15)"""
    keep = []
    owner = _key(zkg, k, keep)
    ctxs = [_ctx_on(zkg, owner, _payloads(k, v), keep) for v in range(6)]
    rc = zkg.zklaim_prove_batch(ctxs)
    st = zkg.prove_batch_stats()
    assert rc == [0] * 6
    assert st[0] == 6 and st[1] == 0
    assert all(c.proof_size == 134 and c.proof for c in ctxs)
    assert len({zkg.ctx_blob(c, "proof") for c in ctxs}) == 6
    for c in ctxs:
        assert zkg.libsnark_verify(c) == 0
    for i, j in ((0, 1), (2, 5), (4, 3)):                                         # ctx i's proof under ctx j's public values: rejected
        _swap_public(ctxs[i], ctxs[j])
        assert zkg.libsnark_verify(ctxs[i]) != 0 and zkg.libsnark_verify(ctxs[j]) != 0
        _swap_public(ctxs[i], ctxs[j])
        assert zkg.libsnark_verify(ctxs[i]) == 0 and zkg.libsnark_verify(ctxs[j]) == 0
    zkg.lib().zkg_compat_reset()


def test_failures_stay_with_their_item(zkg):
    """an unsatisfied credential in the middle, a ctx whose pk was made for another payload count, a ctx without a key"""
    keep = []
    owner3 = _key(zkg, 3, keep)
    owner1 = _key(zkg, 1, keep)
    good = [_ctx_on(zkg, owner3, _payloads(3, v), keep) for v in range(4)]
    false_claim = _ctx_on(zkg, owner3, _payloads(3, 9, ok=False), keep)
    wrong_key = _ctx_on(zkg, owner1, _payloads(3, 10), keep)                      # three payloads under the one-payload key
    no_key = zkg.make_ctx(_payloads(3, 11), keep)
    ctxs = [good[0], good[1], false_claim, good[2], wrong_key, no_key, good[3]]
    rc = zkg.zklaim_prove_batch(ctxs)
    assert rc == [0, 0, 1, 0, 1, 1, 0]
    for c in (false_claim, wrong_key, no_key):
        assert not c.proof and c.proof_size == 0
    for c in good:
        assert c.proof_size == 134 and zkg.libsnark_verify(c) == 0
    assert zkg.libsnark_prove(false_claim) == 1                                   # the single call agrees
    zkg.lib().zkg_compat_reset()


def test_two_keys_interleaved(zkg):
    """1- and 3-payload contexts alternating in one call: every proof verifies under its own vk"""
    keep = []
    owners = {1: _key(zkg, 1, keep), 3: _key(zkg, 3, keep)}
    ctxs = [_ctx_on(zkg, owners[k], _payloads(k, v), keep) for v, k in enumerate((1, 3, 1, 3, 1, 3, 1, 3))]
    assert zkg.zklaim_prove_batch(ctxs) == [0] * 8
    for c in ctxs:
        assert c.proof_size == 134 and zkg.libsnark_verify(c) == 0
    zkg.lib().zkg_compat_reset()


def test_argument_contract(zkg):
    keep = []
    L = zkg.lib()
    L.zkg_zklaim_prove_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    assert zkg.zklaim_prove_batch([]) == []
    rc = (C.c_int * 2)(-7, -7)
    assert L.zkg_zklaim_prove_batch(None, 0, None) == zkg.OK and L.zkg_zklaim_prove_batch(None, 0, rc) == zkg.OK and list(rc) == [-7, -7]
    ctx = zkg.make_ctx(_payloads(1, 0), keep)
    ptrs = (C.c_void_p * 2)(C.addressof(ctx), None)
    assert L.zkg_zklaim_prove_batch(None, 2, rc) == zkg.ERROR and list(rc) == [-7, -7]
    assert L.zkg_zklaim_prove_batch(ptrs, 2, None) == zkg.ERROR
    assert L.zkg_zklaim_prove_batch(ptrs, 2, rc) == zkg.OK and list(rc) == [1, 1]   # no key, and a null entry
    assert not ctx.proof and ctx.proof_size == 0
