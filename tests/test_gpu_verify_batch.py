"""GPU suite: batched Groth16 verification (zkg_groth16_verify_batch) and the device pairing product (zkg_pairing_product).
The contract: every verdict equals zkg_groth16_verify's for the same item, whatever the mix of keys, sizes, encodings and bad proofs."""
import threading

import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from r1cs_util import golden_case_arrays
from util import MONT, Q, R, arr, golden, h, limbs, random_fr_canonical

pytestmark = pytest.mark.gpu
CASES = golden("groth16.json")

G1_GEN = [0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f,
          0xa6ba871b8b1e1b3a, 0x14f1d651eb8e167b, 0xccdd46def0f28c58, 0x1c14ef83340fbe5e]
_G2_U32 = [[0x02bc2026, 0x8e83b5d1, 0x497b0172, 0xdceb1935, 0x97811adf, 0xfbb82647, 0xaf96503b, 0x19573841],
           [0xa84c6140, 0xafb4737d, 0x5802d8c4, 0x6043dd5a, 0x52a02f86, 0x09e950fc, 0x3aea7b6b, 0x14fef083],
           [0x886be9f6, 0x619dfa9d, 0xf59e9b78, 0xfe7fd297, 0x231b7dfe, 0xff9e1a62, 0xae9e4206, 0x28fd7eeb],
           [0xc71856ee, 0x64095b56, 0x327d3cbb, 0xdc57f922, 0x33351076, 0x55f935be, 0x93fd6482, 0x0da4a0e6]]
G2_GEN = [c[2 * i] | (c[2 * i + 1] << 32) for c in _G2_U32 for i in range(4)]          # Montgomery limbs, x.c0 x.c1 y.c0 y.c1


def fixed_base(zkg, g2, ks):
    import torch
    n = ks.shape[0]
    d_k = torch.from_numpy(np.ascontiguousarray(ks).view(np.int64)).cuda()
    d_out = torch.empty((n, 16 if g2 else 8), dtype=torch.int64, device="cuda")
    (zkg.fixed_base_g2_dev if g2 else zkg.fixed_base_g1_dev)(np.array(G2_GEN if g2 else G1_GEN, np.uint64), d_k.data_ptr(), n, d_out.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64).copy()


def single(zkg, items):
    return np.array([zkg.groth16_verify(*it) for it in items], np.uint8)


def check_batch(zkg, items, expect=None):
    got = zkg.groth16_verify_batch(items)
    ref = single(zkg, items)
    assert got.dtype == np.uint8 and got.shape == (len(items),)
    assert np.array_equal(got, ref), (np.flatnonzero(got != ref), got[got != ref], ref[got != ref])
    if expect is not None:
        assert np.array_equal(ref, np.asarray(expect, np.uint8))
    return got


# ---- 1. pairing product ------------------------------------------------------------------------------------------------------------
def test_pairing_product_single_pairs(zkg):
    ab = random_fr_canonical(10, 0xB1)
    P = fixed_base(zkg, False, ab[:5]); Qs = fixed_base(zkg, True, ab[5:])
    for j in range(5):
        assert zkg.pairing_product(P[j:j + 1], Qs[j:j + 1]) == zkg.pairing_probe(ab[j], ab[5 + j]), j


def test_pairing_product_bilinear_sum(zkg):
    n = 300
    a = random_fr_canonical(n, 0xB2); b = random_fr_canonical(n, 0xB3)
    P = fixed_base(zkg, False, a); Qs = fixed_base(zkg, True, b)
    ai = [sum(int(v) << (64 * k) for k, v in enumerate(x)) for x in a]; bi = [sum(int(v) << (64 * k) for k, v in enumerate(x)) for x in b]
    total = sum(x * y for x, y in zip(ai, bi)) % R
    expect = zkg.pairing_probe(np.array(limbs(total), np.uint64), np.array(limbs(1), np.uint64))
    assert zkg.pairing_product(P, Qs) == expect
    # a pair with a point at infinity contributes 1
    P2 = np.vstack([P, np.zeros((1, 8), np.uint64), P[:1]]); Q2 = np.vstack([Qs, Qs[:1], np.zeros((1, 16), np.uint64)])
    assert zkg.pairing_product(P2, Q2) == expect
    # n = 0: GT's one
    one = zkg.pairing_product(np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64))
    assert one == zkg.pairing_probe(np.zeros(4, np.uint64), np.array(limbs(1), np.uint64))
    assert one[:32] == bytes(np.array(limbs(MONT % Q), np.uint64).view(np.uint8)) and not any(one[32:])
    bad = P[:1].copy(); bad[0, 4] ^= np.uint64(1)                     # off the curve: refused
    with pytest.raises(zkg.ZkgError):
        zkg.pairing_product(bad, Qs[:1])


# ---- key / proof factories ---------------------------------------------------------------------------------------------------------
NPUB = 40


def wide_system(zkg, keep):
    """x_i * 1 = x_i for 48 variables, 40 of them public: any assignment satisfies it, so the public inputs differ per proof"""
    n = 48
    rp = np.arange(n + 1, dtype=np.uint32); cols = np.arange(1, n + 1, dtype=np.uint32)
    one = np.tile(arr([1], R), (n, 1))
    return zkg.make_r1cs(n, NPUB, (rp, cols, one), (rp, np.zeros(n, np.uint32), one), (rp, cols, one), keep), n


class WideKey:
    def __init__(self, zkg, seed):
        self.keep = []
        cs, self.n = wide_system(zkg, self.keep)
        self.kp = zkg.Keypair(cs, random_fr_canonical(5, seed))
        self.vk = self.kp.vk_blob()
        self.crs = zkg.Crs(self.kp.pk)
        self.rng = np.random.default_rng(seed)

    def proof(self, w=None):
        if w is None:
            w = arr([int.from_bytes(self.rng.bytes(31), "little") % R for _ in range(self.n)], R)
        rs = random_fr_canonical(2, int(self.rng.integers(1 << 62)))
        rc, pr = self.crs.prove(w, rs[0], rs[1])
        assert rc == 0
        return self.vk, w[:NPUB].copy(), pr

    def free(self):
        self.crs.free(); self.kp.free()


@pytest.fixture(scope="module")
def wide(zkg):
    k1, k2 = WideKey(zkg, 0xC1), WideKey(zkg, 0xC2)
    pool = [k1.proof() for _ in range(1000)]
    yield k1, k2, pool
    k1.free(); k2.free()


def golden_key(zkg, case):
    A, B, C, pts, w, r, s = golden_case_arrays(case)
    keep = []
    cs = zkg.make_r1cs(case["num_variables"], case["num_inputs"], A, B, C, keep)
    td = arr([h(case["trapdoor"][k]) for k in ("t", "alpha", "beta", "gamma", "delta")])
    kp = zkg.Keypair(cs, td)
    vk = kp.vk_blob()
    kp.free()
    return vk, w[:case["num_inputs"]].copy(), bytes.fromhex(case["proof_hex"])


# ---- 2. golden keys ----------------------------------------------------------------------------------------------------------------
def test_golden_proofs(zkg):
    items = []
    for case in CASES:
        vk, x, pr = golden_key(zkg, case)
        bad = bytearray(pr); bad[50] ^= 4
        items += [(vk, x, pr), (vk, x, bytes(bad))]
    got = check_batch(zkg, items)
    assert not got[0::2].any() and got[1::2].all()


# ---- 3. valid batches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000])
def test_valid_batches(zkg, wide, n):
    _, _, pool = wide
    got = zkg.groth16_verify_batch(pool[:n])
    assert not got.any()
    assert np.array_equal(got, single(zkg, pool[:n]))
    assert len({it[1].tobytes() for it in pool[:n]}) == n                  # public inputs differ per proof


# ---- 4. mixed batches against the single verifier ----------------------------------------------------------------------------------
def fq2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def twist_point_outside_g2():
    """an x in Fq2 whose x^3 + b' is a square (norm's Legendre symbol), b' = 3 / (9 + u): a point on the twist that is not in G2
    (the twist's group order is r times a cofactor of ~2^254, so a point found this way lies in G2 with negligible probability)"""
    inv = pow(81 + 1, Q - 2, Q)
    bp = fq2_mul((3, 0), (9 * inv % Q, (-inv) % Q))
    for x0 in range(1, 1000):
        x = (x0, 1)
        rhs = fq2_mul(fq2_mul(x, x), x); rhs = ((rhs[0] + bp[0]) % Q, (rhs[1] + bp[1]) % Q)
        norm = (rhs[0] * rhs[0] + rhs[1] * rhs[1]) % Q
        if pow(norm, (Q - 1) // 2, Q) == 1:
            return x
    raise AssertionError("no x found")


def mont_bytes(v):
    return (v * MONT % Q).to_bytes(32, "little")


def fq_nonresidue_x():
    for x in range(1, 1000):
        if pow((x ** 3 + 3) % Q, (Q - 1) // 2, Q) == Q - 1:
            return x
    raise AssertionError


def invalid_variants(wide_keys):
    """(name, item, expected verdict) for every kind of item the combination must not take, or must reject"""
    k1, k2, pool = wide_keys
    vk, x, pr = pool[0]
    out = []
    x2 = x.copy(); x2[3] = arr([12345], R)[0]
    out.append(("wrong_input", (vk, x2, pr), 1))
    out.append(("other_key", (vk,) + k2.proof()[1:], 1))
    b = bytearray(pr); b[0] = ord("2"); out.append(("bad_flag_A", (vk, x, bytes(b)), 1))
    b = bytearray(pr); b[99] = ord("7"); out.append(("bad_flag_B", (vk, x, bytes(b)), 1))
    b = bytearray(pr); b[100] = 0; out.append(("bad_flag_C", (vk, x, bytes(b)), 1))
    b = bytearray(pr); b[0] = ord("0"); b[1:33] = mont_bytes(fq_nonresidue_x()); out.append(("nonresidue_x", (vk, x, bytes(b)), 1))
    b = bytearray(pr); b[1:33] = (Q + 5).to_bytes(32, "little"); out.append(("x_limbs_ge_q", (vk, x, bytes(b)), None))
    b = bytearray(pr); b[101:133] = (Q + 1).to_bytes(32, "little"); out.append(("C_x_limbs_ge_q", (vk, x, bytes(b)), None))
    x3 = x.copy(); x3[5] = np.array(limbs(R + 3), np.uint64); out.append(("input_ge_r", (vk, x3, pr), None))
    out.append(("long_proof", (vk, x, pr + b"\0"), 1))
    out.append(("short_proof", (vk, x, pr[:-1]), 1))
    out.append(("few_inputs", (vk, x[:-1], pr), 1))
    out.append(("malformed_vk", (vk[:200], x, pr), 2))
    b = bytearray(pr); b[0] = ord("1"); out.append(("A_infinity", (vk, x, bytes(b)), None))
    xt = twist_point_outside_g2()
    b = bytearray(pr); b[34] = ord("0"); b[35:67] = mont_bytes(xt[0]); b[67:99] = mont_bytes(xt[1]); b[99] = ord("0")
    out.append(("B_outside_G2", (vk, x, bytes(b)), 1))
    return out


def test_mixed_batch_element_by_element(zkg, wide):
    _, _, pool = wide
    variants = invalid_variants(wide)
    n = 300
    slots = [0, n - 1, 64, 65, 127, 128, 200, 201, 202, 10, 31, 32, 250, 260, 290]      # first, last, adjacent, several wavefronts
    assert len(slots) >= len(variants)
    items = list(pool[:n]); expect = [0] * n
    for s_, (name, it, v) in zip(slots, variants):
        items[s_] = it
        expect[s_] = v
    got = check_batch(zkg, items)
    for s_, (name, it, v) in zip(slots, variants):
        if v is not None:
            assert got[s_] == v, name
    assert not np.delete(got, slots[:len(variants)]).any()
    # every variant on its own, and a batch of nothing but invalid items (the bisection's worst case)
    for name, it, v in variants:
        check_batch(zkg, [it])
    check_batch(zkg, [it for _, it, _ in variants] * 3)


def test_mixed_batch_random_positions(zkg, wide):
    _, _, pool = wide
    variants = invalid_variants(wide)
    rng = np.random.default_rng(5)
    items = list(pool[300:557])
    for pos in rng.choice(len(items), 20, replace=False):
        items[pos] = variants[int(rng.integers(len(variants)))][1]
    check_batch(zkg, items)


# ---- 5. the weights are used -------------------------------------------------------------------------------------------------------
def test_swapped_c_points_are_rejected(zkg, wide):
    k1, _, pool = wide
    w = arr([int(v) for v in range(7, 7 + k1.n)], R)
    (vk, x, p1), (_, _, p2) = k1.proof(w), k1.proof(w)
    assert p1 != p2 and p1[100:] != p2[100:]
    s1 = p1[:100] + p2[100:]; s2 = p2[:100] + p1[100:]
    got = check_batch(zkg, [(vk, x, s1), (vk, x, s2)], expect=[1, 1])
    assert list(got) == [1, 1]
    got = check_batch(zkg, list(pool[:40]) + [(vk, x, s1), (vk, x, s2)] + list(pool[40:80]))
    assert got[40] == 1 and got[41] == 1 and got.sum() == 2


# ---- 6 and 7. several keys interleaved; credentials through the seam ---------------------------------------------------------------
def credential_items(zkg, k, presentations, keep):
    pls = [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i)
           for i in range(k)]
    ctx = zkg.make_ctx(pls, keep)
    keep.append(ctx)
    assert zkg.libsnark_trusted_setup(ctx) == 0
    items = []
    for _ in range(presentations):
        assert zkg.libsnark_prove(ctx) == 0
        assert zkg.libsnark_verify(ctx) == 0
        items.append((zkg.ctx_blob(ctx, "vk"), zkg.zklaim_input_map(ctx), zkg.ctx_blob(ctx, "proof")))
    # the verifier's view with a forged public reference value: rejected, as libsnark_verify rejects it
    head = ctx.pl_ctx_head.contents
    head.pl.data_ref[0] = 1000
    assert zkg.libsnark_verify(ctx) != 0
    forged = (zkg.ctx_blob(ctx, "vk"), zkg.zklaim_input_map(ctx), zkg.ctx_blob(ctx, "proof"))
    head.pl.data_ref[0] = 2100
    return items, forged


def test_credentials_through_the_seam(zkg):
    keep = []
    for k in (1, 8):
        items, forged = credential_items(zkg, k, 4, keep)
        check_batch(zkg, items, expect=[0] * len(items))
        got = check_batch(zkg, items[:2] + [forged] + items[2:])
        assert list(got) == [0, 0, 1, 0, 0]
    zkg.lib().zkg_compat_reset()


def test_several_keys_interleaved(zkg, wide):
    keep = []
    cred1, forged1 = credential_items(zkg, 1, 3, keep)
    cred8, _ = credential_items(zkg, 8, 3, keep)
    gold = [golden_key(zkg, c) for c in CASES[:3]]
    _, _, pool = wide
    sources = [cred1, cred8, [gold[0]] * 3, [gold[1]] * 3, [gold[2]] * 3, pool[:3]]
    items = []
    for j in range(3):
        for src in sources:
            items.append(src[j])
    bad = bytearray(gold[1][2]); bad[40] ^= 1
    items.insert(4, forged1); items.insert(9, (gold[1][0], gold[1][1], bytes(bad))); items.append((gold[2][0], gold[0][1], gold[0][2]))
    got = check_batch(zkg, items)
    assert got[4] == 1 and got[9] != 0 and got[-1] != 0 and (got == 0).sum() == len(items) - 3
    zkg.lib().zkg_compat_reset()


# ---- 8. two threads at once --------------------------------------------------------------------------------------------------------
def test_two_threads(zkg, wide):
    _, _, pool = wide
    variants = invalid_variants(wide)
    lists = [list(pool[:200]), list(pool[200:450])]
    lists[0][17] = variants[0][1]; lists[1][100] = variants[1][1]; lists[1][249] = variants[14][1]
    refs = [single(zkg, lst) for lst in lists]
    out = [None, None]; errs = []

    def run(k):
        try:
            for _ in range(3):
                got = zkg.groth16_verify_batch(lists[k])
                assert np.array_equal(got, refs[k])
            out[k] = True
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs and out == [True, True]
