"""GPU: zkg_zklaim_verify_batch, many libsnark_verify calls in one, and the two kernels of its device front end through their hooks.
The contract: rc[i] equals libsnark_verify(ctxs[i]) whatever the mix of keys, sizes, encodings and bad proofs; k_proof_decode gives the
points and flags the single verifier's decoding gives; k_zklaim_input_sums gives sum w_p x_pk mod r over the public inputs of
zkg_zklaim_input_map."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from gpu_util import credential_payloads, zkg  # noqa: F401
from util import MONT, Q, R, from_limbs, ints, random_fr_canonical

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The library reads ZKG_SEAM_GPU_VERIFY at its first zkg_zklaim_verify_batch that reaches the GPU.  Groups as small as these tests' take the
# host front end by default (the device's wins from 512 payload records on), so this process asks for the device's for every group: the
# entry's contract is the same on either, and the device front end is what is new.  The other two settings run in child processes below.
os.environ["ZKG_SEAM_GPU_VERIFY"] = "1"


# ---- 1. k_proof_decode ---------------------------------------------------------------------------------------------------------------
def mont_bytes(v):
    return (v * MONT % Q).to_bytes(32, "little")


def fq_nonresidue_x():
    for x in range(1, 1000):
        if pow((x ** 3 + 3) % Q, (Q - 1) // 2, Q) == Q - 1:
            return x
    raise AssertionError


# (name, slot whose flag bit the host rule clears or None, mutation of the 134-byte record): the malformed encodings of
# test_gpu_verify_batch.invalid_variants, per slot, and infinity in each slot (accepted: the point is all-zero, nothing else is read)
def _set(at, value):
    def f(b):
        b[at:at + len(value)] = value
    return f


MALFORMED = [
    ("flag_2_A", 0, _set(0, b"2")),
    ("parity_7_B", 1, _set(99, b"7")),
    ("parity_0_C", 2, _set(133, b"\0")),
    ("nonresidue_x_A", 0, _set(0, b"0" + mont_bytes(fq_nonresidue_x()))),
    ("x_ge_q_A", 0, _set(1, (Q + 5).to_bytes(32, "little"))),
    ("x_c0_ge_q_B", 1, _set(35, (Q + 1).to_bytes(32, "little"))),
    ("x_c1_ge_q_B", 1, _set(67, (Q + 1).to_bytes(32, "little"))),
    ("x_ge_q_C", 2, _set(101, (Q + 1).to_bytes(32, "little"))),
    ("infinity_A", None, _set(0, b"1")),
    ("infinity_B", None, _set(34, b"1")),
    ("infinity_C", None, _set(100, b"1")),
]
INF_SLOT = {"infinity_A": 0, "infinity_B": 1, "infinity_C": 2}
DECODE_COUNTS = [1, 64, 65, 257]


@pytest.fixture(scope="module")
def decode_pool(oracle):
    """257 records (a_i G1, b_i G2, c_i G1) serialised by the oracle's own writer, and the oracle's affine Montgomery limbs"""
    import pyref
    n = max(DECODE_COUNTS)
    ks = random_fr_canonical(3 * n, 0xD0)
    A = oracle.g1_fixed_base(oracle.g1_generator(), ks[:n]); B = oracle.g2_fixed_base(oracle.g2_generator(), ks[n:2 * n])
    Cc = oracle.g1_fixed_base(oracle.g1_generator(), ks[2 * n:])
    recs = np.zeros((n, 134), np.uint8)
    par_y, par_y0 = set(), set()
    for i in range(n):
        a = ints(A[i], Q); b = ints(B[i], Q); c = ints(Cc[i], Q)
        rec = pyref.ser_g1((a[0], a[1])) + pyref.ser_g2(((b[0], b[1]), (b[2], b[3]))) + pyref.ser_g1((c[0], c[1]))
        assert len(rec) == 134
        recs[i] = np.frombuffer(rec, np.uint8)
        par_y.add(a[1] & 1); par_y0.add(b[2] & 1)
    assert par_y == {0, 1} and par_y0 == {0, 1}                             # both parities of y and of y.c0 occur
    return recs, A, B, Cc


@pytest.mark.parametrize("n", DECODE_COUNTS)
def test_proof_decode_matches_the_oracle(zkg, decode_pool, n):
    recs, A, B, Cc = decode_pool
    gA, gB, gC, ok = zkg.proof_decode_gpu(recs[:n])
    assert np.array_equal(gA, A[:n]) and np.array_equal(gB, B[:n]) and np.array_equal(gC, Cc[:n])
    assert (ok == 7).all()


@pytest.mark.parametrize("n", DECODE_COUNTS)
def test_proof_decode_flags_follow_the_host_rule(zkg, decode_pool, n):
    """malformed records at positions 0, 63, 64 and last: the flag bits are the host rule's (ser::get_g1 / get_g2 with coords_canonical),
    a point that does not decode or is infinity is all-zero, the record's other points and every neighbour are untouched"""
    recs, A, B, Cc = decode_pool
    proofs = recs[:n].copy()
    exp = [A[:n].copy(), B[:n].copy(), Cc[:n].copy()]
    exp_ok = np.full(n, 7, np.uint8)
    start = 4 * DECODE_COUNTS.index(n)
    planted = sorted({p for p in (0, 63, 64, n - 1) if p < n})
    for j, pos in enumerate(planted):
        name, bad_slot, mutate = MALFORMED[(start + j) % len(MALFORMED)]
        b = bytearray(proofs[pos].tobytes()); mutate(b)
        proofs[pos] = np.frombuffer(bytes(b), np.uint8)
        slot = bad_slot if bad_slot is not None else INF_SLOT[name]
        exp[slot][pos] = 0
        if bad_slot is not None:
            exp_ok[pos] &= np.uint8(~(1 << bad_slot) & 7)
    gA, gB, gC, ok = zkg.proof_decode_gpu(proofs)
    assert np.array_equal(ok, exp_ok), (planted, ok[planted], exp_ok[planted])
    assert np.array_equal(gA, exp[0]) and np.array_equal(gB, exp[1]) and np.array_equal(gC, exp[2])


def test_proof_decode_every_malformed_variant(zkg, decode_pool):
    """every variant once, side by side in one call (the per-count test above plants four per count)"""
    recs, A, B, Cc = decode_pool
    n = len(MALFORMED)
    proofs = recs[:n].copy()
    exp = [A[:n].copy(), B[:n].copy(), Cc[:n].copy()]
    exp_ok = np.full(n, 7, np.uint8)
    for pos, (name, bad_slot, mutate) in enumerate(MALFORMED):
        b = bytearray(proofs[pos].tobytes()); mutate(b)
        proofs[pos] = np.frombuffer(bytes(b), np.uint8)
        exp[bad_slot if bad_slot is not None else INF_SLOT[name]][pos] = 0
        if bad_slot is not None:
            exp_ok[pos] &= np.uint8(~(1 << bad_slot) & 7)
    gA, gB, gC, ok = zkg.proof_decode_gpu(proofs)
    assert np.array_equal(ok, exp_ok)
    assert np.array_equal(gA, exp[0]) and np.array_equal(gB, exp[1]) and np.array_equal(gC, exp[2])


# ---- 2. k_zklaim_input_sums ------------------------------------------------------------------------------------------------------------
OP_NAMES = ["less", "less_or_eq", "eq", "greater_or_eq", "greater", "not_eq", "noop"]


def _random_public(k, rng):
    out = []
    for i in range(k):
        refs = [int(v) for v in rng.integers(0, 1 << 63, 5, dtype=np.int64)]
        refs[int(rng.integers(5))] = (1 << 64) - 1
        out.append(dict(attrs=[0] * 5, refs=refs, ops=[OP_NAMES[int(v)] for v in rng.integers(0, 7, 5)], salt=0, hash=bytes(rng.integers(0, 256, 32, dtype=np.uint8))))
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 20])
def test_input_sums(zkg, k):
    """l = 6, 11, 16, 102 elements; N = 1, 65, 300 (one lane, a second pass of the wavefront, three slices and their fold); whole, inner,
    one-position and empty ranges; a mask with zeros at a block's first and last lane; weights 1, 2^128 - 1 and random"""
    rng = np.random.default_rng(0x5EA + k)
    keep = []
    ctxs = [zkg.make_ctx(_random_public(k, rng), keep) for _ in range(300)]
    x = [[v for v in ints(zkg.zklaim_input_map(c), R)] for c in ctxs]
    l = (1280 * k + 252) // 253
    assert all(len(row) == l for row in x)
    for n in (1, 65, 300):
        w = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
        w[0] = [1, 0, 0, 0]
        if n > 1:
            w[n - 1] = [0xFFFFFFFF] * 4
        wi = [sum(int(v) << (32 * j) for j, v in enumerate(row)) for row in w]
        mask = np.ones(n, np.uint8)
        for z in (0, 63, 64, 100, 299):                                     # first and last lane of a block's first pass, the next pass, the second slice, the end
            if z < n and n > 1:
                mask[z] = 0
        ranges = [(0, n), (1, 64), (64, 65), (n, n), (0, 0)]
        for lo, hi in ranges:
            if hi > n:
                continue
            for m in (None, mask):
                got = zkg.zklaim_input_sums_gpu(ctxs[:n], w, m, lo, hi)
                assert got.shape == (l, 4)
                exp = [sum(wi[p] * x[p][e] for p in range(lo, hi) if m is None or m[p]) % R for e in range(l)]
                assert [from_limbs(r) for r in got] == [v * MONT % R for v in exp], (k, n, lo, hi, m is not None)
    with pytest.raises(zkg.ZkgError):                                       # another payload count among the contexts
        zkg.zklaim_input_sums_gpu([ctxs[0], zkg.make_ctx(_random_public(k + 1, rng), keep)], np.ones((2, 4), np.uint32))
    with pytest.raises(zkg.ZkgError):
        zkg.zklaim_input_sums_gpu([ctxs[0], None], np.ones((2, 4), np.uint32))


# ---- 3. the seam entry -------------------------------------------------------------------------------------------------------------------
def _payloads(k, v):
    pls = credential_payloads(k)
    pls[0] = dict(pls[0], attrs=[1980 + v, 0, 42 + v, 0, 5], salt=0x7100 + 0x10 * k + v)
    return pls


def _ctx_on(zkg, owner, pls, keep):
    """a ctx of its own (own payloads, own ctx->proof) sharing the owner's pk / vk"""
    c = zkg.make_ctx(pls, keep)
    c.pk, c.pk_size, c.vk, c.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
    return c


@pytest.fixture(scope="module")
def seam(zkg):
    """a key at one payload (radix-2 domain) and at three (a step domain), nine proved presentations of each"""
    keep = []
    owners, ctxs = {}, {}
    for k in (1, 3):
        owner = zkg.make_ctx(_payloads(k, 0), keep)
        assert zkg.libsnark_trusted_setup(owner) == 0
        owners[k] = owner
        ctxs[k] = [_ctx_on(zkg, owner, _payloads(k, v), keep) for v in range(9)]
        assert zkg.zklaim_prove_batch(ctxs[k]) == [0] * 9
    yield zkg, owners, ctxs, keep
    zkg.lib().zkg_compat_reset()


def _single(zkg, ctxs):
    return [1 if c is None else zkg.libsnark_verify(c) for c in ctxs]


@pytest.mark.parametrize("k", [1, 3])
def test_nine_valid_presentations(seam, k):
    zkg, owners, ctxs, keep = seam
    rc = zkg.zklaim_verify_batch(ctxs[k])
    st = zkg.zklaim_verify_batch_stats()
    assert rc == [0] * 9 == _single(zkg, ctxs[k])
    assert st == (1, 0, 0, 9)                                               # one combined check, no single decision, all nine from the device


def test_bad_items_stay_with_their_item(seam):
    zkg, owners, ctxs, keep = seam
    good = ctxs[3]
    forged = _ctx_on(zkg, owners[3], _payloads(3, 1), keep)                 # presentation 1's proof under another public reference value
    forged.proof, forged.proof_size = good[1].proof, good[1].proof_size
    forged.pl_ctx_head.contents.pl.data_ref[0] = 1000
    flipped = _ctx_on(zkg, owners[3], _payloads(3, 2), keep)
    buf = bytearray(zkg.ctx_blob(good[2], "proof")); buf[50] ^= 4
    flipped_buf = (C.c_ubyte * 134)(*buf); keep.append(flipped_buf)
    flipped.proof, flipped.proof_size = C.addressof(flipped_buf), 134
    short = _ctx_on(zkg, owners[3], _payloads(3, 3), keep)
    short.proof, short.proof_size = good[3].proof, 133
    other_vk = _ctx_on(zkg, owners[1], _payloads(3, 4), keep)               # three payloads and their proof under the one-payload key
    other_vk.proof, other_vk.proof_size = good[4].proof, good[4].proof_size
    longer = _ctx_on(zkg, owners[3], _payloads(3, 5) + credential_payloads(1), keep)     # one payload more than the key takes
    longer.proof, longer.proof_size = good[5].proof, good[5].proof_size
    no_proof = _ctx_on(zkg, owners[3], _payloads(3, 6), keep)
    batch = [good[0], forged, good[1], flipped, good[2], short, other_vk, good[3], longer, None, good[4], no_proof, good[5], good[0], good[6], good[7], good[8]]
    expect = [0, 1, 0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0]
    ref = _single(zkg, batch)
    assert ref == expect
    rc = zkg.zklaim_verify_batch(batch)
    st = zkg.zklaim_verify_batch_stats()
    assert rc == ref
    assert st[0] > 1 and st[1] > 0                                          # the forged item forces a bisection; it and the misfits go to the single verifier
    assert st[3] == 12                                                      # ten valid, the forged and the flipped one entered through the device


def test_two_keys_interleaved(seam):
    zkg, owners, ctxs, keep = seam
    batch = [ctxs[k][v] for v in range(9) for k in (1, 3)]
    assert zkg.zklaim_verify_batch(batch) == [0] * 18
    assert zkg.zklaim_verify_batch_stats() == (2, 0, 0, 18)
    swapped = _ctx_on(zkg, owners[1], _payloads(1, 2), keep)                # presentation 2's public values with presentation 3's proof
    swapped.proof, swapped.proof_size = ctxs[1][3].proof, ctxs[1][3].proof_size
    batch[6] = swapped
    rc = zkg.zklaim_verify_batch(batch)
    assert rc == _single(zkg, batch) and rc[6] == 1 and sum(rc) == 1


def test_two_threads_on_the_same_contexts(seam):
    zkg, owners, ctxs, keep = seam
    batch = ctxs[3] + ctxs[1] + [None]
    ref = _single(zkg, batch)
    errs = []

    def run():
        try:
            for _ in range(3):
                assert zkg.zklaim_verify_batch(batch) == ref
                assert zkg.zklaim_verify_batch_stats()[3] == 18             # the counters are the calling thread's
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run) for _ in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs


def test_argument_contract_with_a_gpu(seam):
    zkg, owners, ctxs, keep = seam
    L = zkg.lib()
    L.zkg_zklaim_verify_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    rc = (C.c_int * 2)(-7, -7)
    ptrs = (C.c_void_p * 2)(C.addressof(ctxs[1][0]), None)
    assert L.zkg_zklaim_verify_batch(None, 0, rc) == zkg.OK and list(rc) == [-7, -7]
    assert L.zkg_zklaim_verify_batch(None, 2, rc) == zkg.ERROR and list(rc) == [-7, -7]
    assert L.zkg_zklaim_verify_batch(ptrs, 2, None) == zkg.ERROR
    assert L.zkg_zklaim_verify_batch(ptrs, 2, rc) == zkg.OK and list(rc) == [0, 1]


HOST_LEG = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import zklaim_amd as zkg
from gpu_util import credential_payloads
keep = []
owner = zkg.make_ctx(credential_payloads(1), keep)
assert zkg.libsnark_trusted_setup(owner) == 0
ctxs = []
for v in range(6):
    pls = credential_payloads(1); pls[0] = dict(pls[0], attrs=[1980 + v, 0, 42 + v, 0, 5], salt=0x7200 + v)
    c = zkg.make_ctx(pls, keep)
    c.pk, c.pk_size, c.vk, c.vk_size = owner.pk, owner.pk_size, owner.vk, owner.vk_size
    ctxs.append(c)
assert zkg.zklaim_prove_batch(ctxs) == [0] * 6
ctxs[2].pl_ctx_head.contents.pl.data_ref[0] = 1000
rc = zkg.zklaim_verify_batch(ctxs + [None])
st = zkg.zklaim_verify_batch_stats()
assert rc == [zkg.libsnark_verify(c) for c in ctxs] + [1] == [0, 0, 1, 0, 0, 0, 1], rc
assert st[0] >= 1 and st[1] >= 1 and st[3] == 0, st
big = [ctxs[v % 2] for v in range(int(sys.argv[2]))]
assert zkg.zklaim_verify_batch(big) == [0] * len(big)
assert zkg.zklaim_verify_batch_stats() == (1, 0, 0, int(sys.argv[3])), zkg.zklaim_verify_batch_stats()
zkg.lib().zkg_compat_reset()
zkg.shutdown()
print("host leg ok")
"""


@pytest.mark.parametrize("setting", ["0", None])
def test_host_front_end_in_a_child_process(zkg, setting):
    """ZKG_SEAM_GPU_VERIFY is read once per process.  "0": the host front end for every group; not set: the default, the host front end for a
    group of seven one-payload items and the device's for one of 512.  Same return codes, and the counters say which front end ran."""
    env = dict(os.environ)
    env.pop("ZKG_SEAM_GPU_VERIFY")
    if setting is not None:
        env["ZKG_SEAM_GPU_VERIFY"] = setting
    out = subprocess.run([sys.executable, "-c", HOST_LEG, ROOT, "512", "0" if setting == "0" else "512"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "host leg ok" in out.stdout, out.stderr[-2000:]
