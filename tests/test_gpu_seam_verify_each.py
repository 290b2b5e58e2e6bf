"""GPU: zkg_zklaim_verify_each, many libsnark_verify calls in one with every context decided by its own pairing equation on the device, and
the accumulator in front of its Miller loops (the per-key bit table and k_zklaim_ic_each) through its hook.
The contract: rc[i] equals libsnark_verify(ctxs[i]) whatever the mix of keys, sizes, encodings and bad proofs, in however many rounds; the
counters say who decided; the kernel gives, limb for limb, what its own code compiled for the host gives (which test_seam_verify_each_host.py
holds against oracle/pyref.py)."""
import ctypes as C
import threading

import numpy as np
import pytest

import seam_verify_each_cases as cs
from gpu_util import credential_payloads, zkg  # noqa: F401

pytestmark = pytest.mark.gpu


# ---- 1. the accumulator's hook: the GPU against the same code on the host ----------------------------------------------------------------
@pytest.mark.parametrize("name", cs.CASE_NAMES)
def test_ic_each_gpu_equals_the_device_code_on_host(zkg, name):
    _, npl, c, ctxs, exp = {c[0]: c for c in cs.cases()[:-1]}[name]
    ic0, ic = cs.key_points(c)
    host = zkg.zklaim_ic_each(ic0, ic, ctxs, where=2)
    gpu = zkg.zklaim_ic_each(ic0, ic, ctxs, where=1)
    assert np.array_equal(gpu, host), [i for i in range(len(ctxs)) if not np.array_equal(gpu[i], host[i])]
    assert np.array_equal(gpu, exp)


@pytest.mark.parametrize("npl", cs.PAYLOAD_COUNTS)
def test_ic_each_batch_sizes(zkg, npl):
    """1, 64 and 65 items: one block, as many blocks as a wavefront has lanes, one more"""
    keep = []
    rng = np.random.default_rng(0xB5 + npl)
    ctxs = [cs.random_ctx(zkg, npl, rng, keep) for _ in range(65)]
    ic0, ic = cs.key_points(cs.scalars(npl, 0xC0 + npl))
    host = zkg.zklaim_ic_each(ic0, ic, ctxs, where=2)
    assert len({host[i].tobytes() for i in range(65)}) == 65
    for n in (1, 64, 65):
        assert np.array_equal(zkg.zklaim_ic_each(ic0, ic, ctxs[:n], where=1), host[:n]), n
    with pytest.raises(zkg.ZkgError):
        zkg.zklaim_ic_each(ic0, ic, [ctxs[0], None], where=1)


# ---- 2. the seam entry -------------------------------------------------------------------------------------------------------------------
N1, N3 = 130, 9


def _payloads(k, v):
    pls = credential_payloads(k)
    pls[0] = dict(pls[0], attrs=[1980 + v % 100, v // 100, 42 + v, 0, 5], refs=[2100, v // 100, 41, 0, 5], salt=0x8100 + 0x1000 * k + v)
    return pls


def _ctx_on(zkg, owner, pls, keep):
    """a ctx of its own (own payloads, own ctx->proof) sharing the owner's pk / vk"""
    c = zkg.make_ctx(pls, keep)
    c.pk, c.pk_size, c.vk, c.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
    return c


def _with_proof(zkg, owner, pls, proof_of, keep, mutate=None, size=None):
    """a ctx on the owner's key carrying (a mutated copy of) another context's proof"""
    c = _ctx_on(zkg, owner, pls, keep)
    buf = bytearray(zkg.ctx_blob(proof_of, "proof"))
    if mutate:
        mutate(buf)
    held = (C.c_ubyte * len(buf))(*buf); keep.append(held)
    c.proof, c.proof_size = C.addressof(held), len(buf) if size is None else size
    return c


@pytest.fixture(scope="module")
def seam(zkg):
    """a key at one payload (radix-2 domain) and at three (a step domain); 130 proved presentations of the first, nine of the second"""
    keep = []
    owners, ctxs = {}, {}
    for k, n in ((1, N1), (3, N3)):
        owner = zkg.make_ctx(_payloads(k, 0), keep)
        assert zkg.libsnark_trusted_setup(owner) == 0
        owners[k] = owner
        ctxs[k] = [_ctx_on(zkg, owner, _payloads(k, v), keep) for v in range(n)]
        assert zkg.zklaim_prove_batch(ctxs[k]) == [0] * n
    yield zkg, owners, ctxs, keep
    zkg.lib().zkg_compat_reset()


def _single(zkg, ctxs):
    return [1 if c is None else zkg.libsnark_verify(c) for c in ctxs]


def _forged(zkg, owners, ctxs, k, v, keep):
    """presentation v's proof under another public reference value"""
    c = _with_proof(zkg, owners[k], _payloads(k, v), ctxs[k][v], keep)
    c.pl_ctx_head.contents.pl.data_ref[0] = 1000
    return c


def test_the_first_call_that_meets_a_key_builds_its_table(seam):
    zkg, owners, ctxs, keep = seam
    owner = zkg.make_ctx(_payloads(1, 500), keep)                           # a key no call has met
    assert zkg.libsnark_trusted_setup(owner) == 0
    two = [_ctx_on(zkg, owner, _payloads(1, 500 + v), keep) for v in range(2)]
    assert zkg.zklaim_prove_batch(two) == [0, 0]
    assert zkg.zklaim_verify_each(two) == [0, 0] and zkg.zklaim_verify_each_stats() == (2, 0, 1, 1)
    assert zkg.zklaim_verify_each(two) == [0, 0] and zkg.zklaim_verify_each_stats() == (2, 0, 1, 0)
    assert zkg.zklaim_verify_each(two + [ctxs[1][0]])[:2] == [0, 0] and zkg.zklaim_verify_each_stats()[:3] == (3, 0, 2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_valid_queues(seam, n):
    zkg, owners, ctxs, keep = seam
    rc = zkg.zklaim_verify_each(ctxs[1][:n])
    st = zkg.zklaim_verify_each_stats()
    assert rc == [0] * n == _single(zkg, ctxs[1][:n])
    assert st[:3] == (n, 0, 1) and st[3] in (0, 1)
    assert zkg.zklaim_verify_each(ctxs[1][:n]) == [0] * n and zkg.zklaim_verify_each_stats() == (n, 0, 1, 0)


def test_valid_three_payload_queue(seam):
    zkg, owners, ctxs, keep = seam
    assert zkg.zklaim_verify_each(ctxs[3]) == [0] * N3 == _single(zkg, ctxs[3])
    assert zkg.zklaim_verify_each_stats()[:3] == (N3, 0, 1)


def test_all_invalid(seam):
    """the sign byte of A, B or C flipped: the point still decodes, the equation fails"""
    zkg, owners, ctxs, keep = seam

    def flip(at):
        def f(b):
            b[at] ^= 1                                                      # '0' <-> '1'
        return f
    batch = [_with_proof(zkg, owners[1], _payloads(1, j), ctxs[1][j], keep, flip((33, 99, 133)[j % 3])) for j in range(65)]
    zkg.zklaim_verify_each(ctxs[1][:1])                                     # (the key's table is there)
    rc = zkg.zklaim_verify_each(batch)
    assert rc == [1] * 65 == _single(zkg, batch)
    assert zkg.zklaim_verify_each_stats() == (65, 0, 1, 0)


def test_bad_items_stay_with_their_item(seam):
    zkg, owners, ctxs, keep = seam
    good1, good3 = ctxs[1], ctxs[3]

    def set_byte(at, v):
        def f(b):
            b[at] = v
        return f

    def xor(at, v):
        def f(b):
            b[at] ^= v
        return f
    forged = _forged(zkg, owners, ctxs, 1, 1, keep)
    flipped = [_with_proof(zkg, owners[1], _payloads(1, 2 + j), good1[2 + j], keep, xor(50 + j, 4)) for j in range(3)]      # a bit of B's x
    short = _with_proof(zkg, owners[1], _payloads(1, 5), good1[5], keep, size=133)
    other_vk = _with_proof(zkg, owners[1], _payloads(3, 4), good3[4], keep)                                # three payloads under the one-payload key
    longer = _with_proof(zkg, owners[1], _payloads(1, 6) + credential_payloads(1), good1[6], keep)         # one payload more than the key takes
    no_proof = _ctx_on(zkg, owners[1], _payloads(1, 7), keep)
    inf_a = _with_proof(zkg, owners[1], _payloads(1, 8), good1[8], keep, set_byte(0, ord("1")))
    inf_c = _with_proof(zkg, owners[1], _payloads(1, 9), good1[9], keep, set_byte(100, ord("1")))
    batch = list(good1)
    placed = {0: forged, 63: short, 64: inf_a, N1 - 1: flipped[0], 1: other_vk, 31: longer, 65: None, 100: no_proof, 128: inf_c, 62: flipped[1], 66: flipped[2]}
    for at, c in placed.items():
        batch[at] = c
    ref = _single(zkg, batch)
    assert all(ref[at] == 1 for at in placed) and sum(ref) == len(placed)
    rc = zkg.zklaim_verify_each(batch)
    st = zkg.zklaim_verify_each_stats()
    assert rc == ref
    assert st[0] + st[1] == N1 - 2                                          # every item that has a key and a proof was decided by one of the two
    # the forged item, the infinity items and every flipped B that still decodes were decided by the device equation
    decodes = sum(1 for c in flipped if zkg.proof_decode_gpu(np.frombuffer(zkg.ctx_blob(c, "proof"), np.uint8))[3][0] == 7)
    assert st[0] == (N1 - len(placed)) + 3 + decodes and st[1] == 3 + (3 - decodes)
    assert st[2] == 1


def test_rounds(seam):
    zkg, owners, ctxs, keep = seam
    batch = list(ctxs[1])
    for at in (0, 63, 64, N1 - 1):
        batch[at] = _forged(zkg, owners, ctxs, 1, at, keep)
    expect = [1 if at in (0, 63, 64, N1 - 1) else 0 for at in range(N1)]
    one = zkg.zklaim_verify_each(batch)
    assert zkg.zklaim_verify_each_stats()[:3] == (N1, 0, 1)
    try:
        zkg.verify_each_set_chunk(64)
        three = zkg.zklaim_verify_each(batch)
        assert zkg.zklaim_verify_each_stats()[:3] == (N1, 0, 3)
    finally:
        zkg.verify_each_set_chunk(0)
    assert one == three == expect == _single(zkg, batch)


def test_two_keys_interleaved(seam):
    zkg, owners, ctxs, keep = seam
    batch = [ctxs[k][v] for v in range(N3) for k in (1, 3)]
    assert zkg.zklaim_verify_each(batch) == [0] * (2 * N3)
    assert zkg.zklaim_verify_each_stats()[:3] == (2 * N3, 0, 2)
    batch[6] = _with_proof(zkg, owners[1], _payloads(1, 2), ctxs[1][3], keep)      # presentation 2's public values with presentation 3's proof
    rc = zkg.zklaim_verify_each(batch)
    assert rc == _single(zkg, batch) and rc[6] == 1 and sum(rc) == 1
    assert zkg.zklaim_verify_each_stats()[:3] == (2 * N3, 0, 2)


def test_two_threads_on_the_same_contexts(seam):
    zkg, owners, ctxs, keep = seam
    batches = [ctxs[3] + ctxs[1][:20] + [None], ctxs[1][:70]]
    refs = [_single(zkg, b) for b in batches]
    errs = []

    def run(b, ref, n_dev):
        try:
            for _ in range(3):
                assert zkg.zklaim_verify_each(b) == ref
                assert zkg.zklaim_verify_each_stats()[:2] == (n_dev, 0)     # the counters are the calling thread's
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(batches[0], refs[0], N3 + 20)), threading.Thread(target=run, args=(batches[1], refs[1], 70)),
          threading.Thread(target=run, args=(batches[0], refs[0], N3 + 20))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


def test_agreement_with_the_other_gpu_verifiers(seam):
    zkg, owners, ctxs, keep = seam
    queue = [ctxs[k][v] for v in range(N3) for k in (1, 3)] + ctxs[1][N3:40]
    queue[4] = _forged(zkg, owners, ctxs, 1, 2, keep)
    queue[11] = _forged(zkg, owners, ctxs, 3, 5, keep)
    rc = zkg.zklaim_verify_each(queue)
    assert sum(rc) == 2 and rc[4] == rc[11] == 1
    assert zkg.zklaim_verify_batch(queue) == rc
    items = [(zkg.ctx_blob(c, "vk"), zkg.zklaim_input_map(c), zkg.ctx_blob(c, "proof")) for c in queue]
    assert [int(v) for v in zkg.groth16_verify_each(items)] == rc


def test_argument_contract_with_a_gpu(seam):
    zkg, owners, ctxs, keep = seam
    L = zkg.lib()
    L.zkg_zklaim_verify_each.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    rc = (C.c_int * 2)(-7, -7)
    ptrs = (C.c_void_p * 2)(C.addressof(ctxs[1][0]), None)
    assert L.zkg_zklaim_verify_each(None, 0, rc) == zkg.OK and list(rc) == [-7, -7]
    assert L.zkg_zklaim_verify_each(None, 2, rc) == zkg.ERROR and list(rc) == [-7, -7]
    assert L.zkg_zklaim_verify_each(ptrs, 2, None) == zkg.ERROR
    assert L.zkg_zklaim_verify_each(ptrs, 2, rc) == zkg.OK and list(rc) == [0, 1]
    assert zkg.zklaim_verify_each_stats()[:3] == (1, 0, 1)
