"""GPU suite: per-proof verification on the device (zkg_groth16_verify_each), the per-item pairing product (zkg_pairing_each) and the
final exponentiation kernel (zkg_final_exp, where=1).  The contract: every verdict equals zkg_groth16_verify's for the same item, exactly,
and every GT value equals the host's, byte for byte."""
import threading

import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from test_final_exp_host import ONE, final_exp_inputs
from test_gpu_verify_batch import CASES, WideKey, fixed_base, golden_key, invalid_variants, single
from util import R, arr, limbs, random_fr_canonical

pytestmark = pytest.mark.gpu

POOL = 140          # proofs of the 48-variable system (key 1); the tests below slice it


@pytest.fixture(scope="module")
def wide(zkg):
    k1, k2 = WideKey(zkg, 0xE1), WideKey(zkg, 0xE2)
    pool = [k1.proof() for _ in range(POOL)]
    yield k1, k2, pool
    k1.free(); k2.free()


def check_each(zkg, items, stats=None):
    got = zkg.groth16_verify_each(items)
    st = zkg.verify_each_stats()
    ref = single(zkg, items)
    assert got.dtype == np.uint8 and got.shape == (len(items),)
    assert np.array_equal(got, ref), (np.flatnonzero(got != ref), got[got != ref], ref[got != ref])
    if stats is not None:
        assert st == stats
    return got


# ---- 1. the final exponentiation on the device -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fe_cases(zkg):
    vals = final_exp_inputs(n_random=40)                 # 50 values: one, random, c1 = 0, c0 = 0, single coefficients, limbs q - 1
    gt = zkg.final_exp(vals[:15], 0)                     # and 15 values that are in GT already
    vals = vals + gt
    assert len(vals) == 65
    return vals, zkg.final_exp(vals, 0)


@pytest.mark.parametrize("n", [1, 64, 65])               # 65: the last block has one live lane
def test_final_exp_on_the_device(zkg, fe_cases, n):
    vals, spec = fe_cases
    assert zkg.final_exp(vals[:n], 1) == spec[:n]
    assert zkg.final_exp(vals[65 - n:], 1) == spec[65 - n:]
    assert spec[0] == ONE


def test_final_exp_refuses_bad_elements_on_the_device(zkg, fe_cases):
    vals, _ = fe_cases
    with pytest.raises(zkg.ZkgError):
        zkg.final_exp([vals[1], b"\0" * 384], 1)
    with pytest.raises(zkg.ZkgError):
        zkg.final_exp([b"\xff" * 384], 1)
    assert zkg.final_exp([], 1) == []


# ---- 2. pairing_each ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def points(zkg):
    n = 65 * 3
    a = random_fr_canonical(n, 0xD1); b = random_fr_canonical(n, 0xD2)
    return a, b, fixed_base(zkg, False, a), fixed_base(zkg, True, b)


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("items", [1, 2, 65])
def test_pairing_each_equals_pairing_product_per_item(zkg, points, pairs, items):
    a, b, P, Qs = points
    n = items * pairs
    got = zkg.pairing_each(P[:n], Qs[:n], pairs)
    assert len(got) == items
    for i in range(items):
        assert got[i] == zkg.pairing_product(P[i * pairs:(i + 1) * pairs], Qs[i * pairs:(i + 1) * pairs]), i
    if pairs == 1:
        for i in range(min(items, 3)):
            assert got[i] == zkg.pairing_probe(a[i], b[i]), i


def test_pairing_each_bilinear(zkg):
    """e([a]G1, [b]G2) == e([ab]G1, G2), both sides through the device-only path"""
    a = random_fr_canonical(4, 0xD3); b = random_fr_canonical(4, 0xD4)
    ai = [sum(int(v) << (64 * k) for k, v in enumerate(x)) for x in a]; bi = [sum(int(v) << (64 * k) for k, v in enumerate(x)) for x in b]
    ab = np.array([limbs(x * y % R) for x, y in zip(ai, bi)], np.uint64)
    one = np.tile(np.array(limbs(1), np.uint64), (4, 1))
    lhs = zkg.pairing_each(fixed_base(zkg, False, a), fixed_base(zkg, True, b), 1)
    rhs = zkg.pairing_each(fixed_base(zkg, False, ab), fixed_base(zkg, True, one), 1)
    assert lhs == rhs and len(set(lhs)) == 4 and ONE not in lhs


def test_pairing_each_infinity_and_bad_points(zkg, points):
    _, _, P, Qs = points
    P3 = P[:9].copy(); Q3 = Qs[:9].copy()
    P3[1] = 0                                            # item 0: its second pair has P at infinity
    Q3[5] = 0                                            # item 1: its third pair has Q at infinity
    P3[6] = 0; Q3[7] = 0; P3[8] = 0; Q3[8] = 0           # item 2: every pair has a point at infinity
    got = zkg.pairing_each(P3, Q3, 3)
    assert got[0] == zkg.pairing_product(P[[0, 2]], Qs[[0, 2]])
    assert got[1] == zkg.pairing_product(P[3:5], Qs[3:5])
    assert got[2] == ONE
    assert zkg.pairing_each(np.zeros((2, 8), np.uint64), np.zeros((2, 16), np.uint64), 1) == [ONE, ONE]
    assert zkg.pairing_each(np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64), 3) == []
    bad = P[:3].copy(); bad[2, 4] ^= np.uint64(1)        # off the curve: refused
    with pytest.raises(zkg.ZkgError):
        zkg.pairing_each(bad, Qs[:3], 3)
    badq = Qs[:3].copy(); badq[0, 9] ^= np.uint64(1)
    with pytest.raises(zkg.ZkgError):
        zkg.pairing_each(P[:3], badq, 1)


# ---- 3. verdicts equal the single verifier's ---------------------------------------------------------------------------------------
def test_golden_proofs(zkg):
    items = []
    for case in CASES:
        vk, x, pr = golden_key(zkg, case)
        bad = bytearray(pr); bad[50] ^= 4
        flip = bytearray(pr); flip[33] ^= 1              # -A: decodes, so the device decides it
        items += [(vk, x, pr), (vk, x, bytes(bad)), (vk, x, bytes(flip))]
    got = check_each(zkg, items)
    assert not got[0::3].any() and got[1::3].all() and got[2::3].all()
    st = zkg.verify_each_stats()
    assert st[0] + st[1] == len(items) and st[0] >= 2 * len(CASES) and st[2] == len(CASES)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_valid_batches(zkg, wide, n):
    _, _, pool = wide
    got = check_each(zkg, pool[:n], stats=(n, 0, 1))
    assert not got.any()
    assert len({it[1].tobytes() for it in pool[:n]}) == n                      # public inputs differ per proof


def test_all_invalid_batch(zkg, wide):
    """the case the entry exists for: nothing is bisected, every proof is rejected by its own equation in the one round"""
    _, _, pool = wide
    items = []
    for j, (vk, x, pr) in enumerate(pool[:65]):
        b = bytearray(pr); b[(33, 99, 133)[j % 3]] ^= 1  # the sign of A, B or C
        items.append((vk, x, bytes(b)))
    got = check_each(zkg, items, stats=(65, 0, 1))
    assert got.all() and (got == 1).all()


HOST_VARIANTS = {"bad_flag_A", "bad_flag_B", "bad_flag_C", "nonresidue_x", "x_limbs_ge_q", "C_x_limbs_ge_q", "input_ge_r", "long_proof", "short_proof",
                 "few_inputs", "malformed_vk"}


def test_invalid_variants_element_by_element(zkg, wide):
    _, _, pool = wide
    variants = invalid_variants(wide)
    n = 130
    slots = [0, n - 1, 63, 64, 65, 127, 128, 1, 62, 66, 126, 31, 32, 100, 10]   # first, last, both sides of the wavefront boundaries
    assert len(slots) == len(set(slots)) >= len(variants)
    items = list(pool[:n])
    for s_, (name, it, v) in zip(slots, variants):
        items[s_] = it
    on_host = sum(name in HOST_VARIANTS for name, _, _ in variants)
    assert on_host == len(HOST_VARIANTS)
    got = check_each(zkg, items, stats=(n - on_host, on_host, 1))
    for s_, (name, it, v) in zip(slots, variants):
        if v is not None:
            assert got[s_] == v, name
    assert not np.delete(got, slots[:len(variants)]).any()
    # every variant on its own: which path decides it
    for name, it, v in variants:
        check_each(zkg, [it], stats=(0, 1, 0) if name in HOST_VARIANTS else (1, 0, 1))
    # nothing but invalid items
    check_each(zkg, [it for _, it, _ in variants] * 3, stats=(3 * (len(variants) - on_host), 3 * on_host, 1))


# ---- 4. the input-count geometries of k_ic_each ------------------------------------------------------------------------------------
class GeoKey:
    """the shape of wide_system (x_i * 1 = x_i, any assignment satisfies it) with npub public inputs of npub + 8 variables"""

    def __init__(self, zkg, npub, seed):
        self.keep = []; self.npub = npub; self.n = n = npub + 8
        rp = np.arange(n + 1, dtype=np.uint32); cols = np.arange(1, n + 1, dtype=np.uint32)
        one = np.tile(arr([1], R), (n, 1))
        cs = zkg.make_r1cs(n, npub, (rp, cols, one), (rp, np.zeros(n, np.uint32), one), (rp, cols, one), self.keep)
        self.kp = zkg.Keypair(cs, random_fr_canonical(5, seed))
        self.vk = self.kp.vk_blob()
        self.crs = zkg.Crs(self.kp.pk)
        self.rng = np.random.default_rng(seed)

    def proof(self):
        w = arr([int.from_bytes(self.rng.bytes(31), "little") % R for _ in range(self.n)], R)
        rs = random_fr_canonical(2, int(self.rng.integers(1 << 62)))
        rc, pr = self.crs.prove(w, rs[0], rs[1])
        assert rc == 0
        return self.vk, w[:self.npub].copy(), pr

    def free(self):
        self.crs.free(); self.kp.free()


@pytest.mark.parametrize("npub", [1, 40, 70])            # one term, fewer than a wavefront, more than a wavefront
def test_input_counts(zkg, npub):
    k = GeoKey(zkg, npub, 0xF0 + npub)
    try:
        items = [k.proof() for _ in range(3)]
        for pos in sorted({0, npub // 2, npub - 1}):     # one changed input: the first, a middle one, the last (lane 5 of the second pass at 70)
            vk, x, pr = items[0]
            x2 = x.copy(); x2[pos] = arr([777 + pos], R)[0]
            items.append((vk, x2, pr))
        zero = (items[1][0], np.zeros_like(items[1][1]), items[1][2])          # every input 0: acc = IC_0
        items.append(zero)
        got = check_each(zkg, items, stats=(len(items), 0, 1))
        assert list(got) == [0, 0, 0] + [1] * (len(items) - 3)
    finally:
        k.free()


def test_input_count_of_a_golden_key(zkg):
    vk, x, pr = golden_key(zkg, CASES[3])
    assert x.shape[0] == 6
    x2 = x.copy(); x2[5] = arr([5], R)[0]
    assert list(check_each(zkg, [(vk, x, pr), (vk, x2, pr)], stats=(2, 0, 1))) == [0, 1]


# ---- 5. rounds, several keys, threads, nothing -------------------------------------------------------------------------------------
def test_rounds(zkg, wide):
    _, _, pool = wide
    items = list(pool[:130])
    for s_ in (0, 63, 64, 129):
        vk, x, pr = items[s_]
        b = bytearray(pr); b[133] ^= 1
        items[s_] = (vk, x, bytes(b))
    whole = check_each(zkg, items, stats=(130, 0, 1))
    try:
        zkg.verify_each_set_chunk(64)
        cut = check_each(zkg, items, stats=(130, 0, 3))
    finally:
        zkg.verify_each_set_chunk(0)
    assert np.array_equal(whole, cut) and list(np.flatnonzero(cut)) == [0, 63, 64, 129]
    check_each(zkg, items, stats=(130, 0, 1))


def test_two_keys_interleaved(zkg, wide):
    _, k2, pool = wide
    other = [k2.proof() for _ in range(5)]
    gold = golden_key(zkg, CASES[1])
    items = []
    for j in range(5):
        items += [pool[j], other[j], gold]
    items[4] = (pool[4][0],) + other[1][1:]              # key 1's blob with key 2's input and proof
    bad = bytearray(gold[2]); bad[133] ^= 1
    items[8] = (gold[0], gold[1], bytes(bad))
    got = check_each(zkg, items, stats=(15, 0, 3))
    assert list(np.flatnonzero(got)) == [4, 8]


def test_two_threads(zkg, wide):
    _, _, pool = wide
    variants = invalid_variants(wide)
    lists = [list(pool[:70]), list(pool[70:140])]
    lists[0][17] = variants[0][1]; lists[1][3] = variants[1][1]; lists[1][69] = variants[14][1]
    refs = [single(zkg, lst) for lst in lists]
    assert refs[0].sum() == 1 and refs[1].sum() == 2
    errs = []

    def run(k):
        try:
            for _ in range(3):
                assert np.array_equal(zkg.groth16_verify_each(lists[k]), refs[k])
                assert zkg.verify_each_stats() == (70, 0, 1)                   # the counters are the calling thread's
                if k:
                    assert np.array_equal(zkg.groth16_verify_batch(lists[k]), refs[k])       # beside the other verify entries
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs


def test_count_zero(zkg, wide):
    _, _, pool = wide
    zkg.groth16_verify_each(pool[:2])
    got = zkg.groth16_verify_each([])
    assert got.shape == (0,) and zkg.verify_each_stats() == (0, 0, 0)
