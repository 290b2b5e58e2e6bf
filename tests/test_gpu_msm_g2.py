"""GPU parity of the G2 multi-exponentiation at the geometry only it has: c = 16 from 2^15 points on, so k_bucket_reduce<Fq2, LARGE> with 64
logical lanes (chunks of 1024 buckets, lane-local running sums whose `T0 += run` doubles), the 2^15-counter one-pass sort and the two-pass
sort from 49 152 points, heavy buckets cut into parts of 512 and merged by a strided sum and an LDS tree.  Two references, both independent
of the code under test: the oracle's BDLO12 restatement on distinct bases, and — where all bases are P, -P or infinity — the one scalar
multiplication (sum eps_i s_i mod r) * P, the sum formed with Python integers.  The same one-point construction runs the heavy path of the
G1 kernels.  Every comparison is bit-exact on the normalised point."""
import numpy as np
import pytest

from gpu_util import ONE_POINT_PATTERNS, adversarial_scalars, dev_bases_g1, g2_jac_of_affine, neg_affine, one_point_case, to_dev, zkg  # noqa: F401
from util import R, arr, g1_jac_expected, g2_jac_expected, limbs, random_fr_canonical

pytestmark = pytest.mark.gpu

POOL = 49152


@pytest.fixture(scope="module")
def pool(oracle):
    """49 152 distinct G2 bases k_i * G, shared (read-only) by every test that needs distinct bases"""
    bases = oracle.g2_fixed_base(oracle.g2_generator(), random_fr_canonical(POOL, 0x62A5E5))
    bases.setflags(write=False)
    return bases


def _oracle_g2(oracle, bases, sc, method=None):
    return oracle.msm_g2(bases, sc, oracle.BDLO12 if method is None else method, oracle.num_threads())


def _dev_g2(zkg, bases, sc, **kw):
    d_b, d_s = to_dev(bases), to_dev(sc)
    return zkg.msm_g2_dev(d_b.data_ptr(), d_s.data_ptr(), len(sc), **kw)


# ---- 1. size classes: c = 4 ... 10 -> 12 -> 16, TINY -> LARGE reduction, one-pass -> two-pass sort -----------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 32767, 32768, 49151, 49152])
def test_msm_g2_size_classes_vs_oracle(zkg, oracle, pool, n):
    bases = np.ascontiguousarray(pool[:n])
    sc = random_fr_canonical(n, 0x62000000 + n)
    exp = _oracle_g2(oracle, bases, sc)
    assert np.array_equal(zkg.msm_g2(bases, sc), exp)
    if n in (2048, 32768, 49152):
        assert np.array_equal(_dev_g2(zkg, bases, sc), exp)
    if n == 32768:                                                   # the scalars as a witness vector keeps them: Montgomery form
        sc_m = np.ascontiguousarray(zkg.field_op(1, 4, sc))
        assert np.array_equal(_dev_g2(zkg, bases, sc_m, scalars_mont=True), exp)


# ---- 2. digit distributions on distinct bases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3000, 32768])
@pytest.mark.parametrize("name", ["same", "two", "tiny", "pow2", "r-1"])
def test_msm_g2_adversarial_scalar_distributions(zkg, oracle, pool, n, name):
    """every scalar equal, two distinct scalars, tiny scalars, 2^k, all r - 1: at 32 768 points most buckets of the large reduction are empty
    and most of its lanes add equal running sums"""
    bases = np.ascontiguousarray(pool[:n])
    sc = adversarial_scalars(n, 0x62100000 + n)[name]
    assert np.array_equal(zkg.msm_g2(bases, sc), _oracle_g2(oracle, bases, sc))


# ---- 3. one-point bases: equal and opposite operands in the accumulation, the heavy parts, the merge, the scan and the trees ------------
@pytest.fixture(scope="module")
def point_g2(oracle):
    return oracle.g2_fixed_base(oracle.g2_generator(), random_fr_canonical(1, 0x62200001))[0]


@pytest.fixture(scope="module")
def point_g1(oracle):
    return oracle.g1_fixed_base(oracle.g1_generator(), random_fr_canonical(1, 0x62200002))[0]


def _one_point_expected_g2(oracle, p, S):
    return g2_jac_of_affine(oracle.g2_fixed_base(p, arr([S]))[0]) if S else g2_jac_expected(None)


@pytest.mark.parametrize("n", [4096, 32768, 150000])
@pytest.mark.parametrize("pattern", ONE_POINT_PATTERNS)
def test_msm_g2_one_point_bases(zkg, oracle, point_g2, n, pattern):
    """sum s_i (eps_i P) = (sum eps_i s_i mod r) P.  At 150 000 points `equal` puts 293 parts into one bucket per window: the second trip of
    k_heavy_merge's strided loop, and tree levels that are all doublings"""
    bases, sc, S = one_point_case(point_g2, n, pattern, 0x62300000 + n)
    if pattern == "zero_sum" or (pattern.startswith("alt") and n % (2 * int(pattern[3:])) == 0):
        assert S == 0
    assert np.array_equal(zkg.msm_g2(bases, sc), _one_point_expected_g2(oracle, point_g2, S))


@pytest.mark.parametrize("n", [4096, 150000])
@pytest.mark.parametrize("pattern", ONE_POINT_PATTERNS)
def test_msm_g1_one_point_bases(zkg, oracle, point_g1, n, pattern):
    """the same for G1 through the host and the device-pointer entry (the 29-bit plain path and its heavy kernels)"""
    bases, sc, S = one_point_case(point_g1, n, pattern, 0x62400000 + n)
    exp = oracle.g1_scalar_mul(point_g1, np.array(limbs(S), np.uint64)) if S else g1_jac_expected(None)
    assert np.array_equal(zkg.msm_g1(bases, sc), exp)
    d_b, d_s = to_dev(bases), to_dev(sc)
    assert np.array_equal(zkg.msm_g1_dev(d_b.data_ptr(), d_s.data_ptr(), n), exp)


# ---- 4. exceptional pairs in lane-walked lists ------------------------------------------------------------------------------------------
def test_msm_g2_exceptional_pairs_in_bucket_lists_match_the_oracle(zkg, oracle, pool):
    """groups of four equal scalars land in one bucket; their bases make neighbours in the bucket's list equal (tangent), opposite, or put
    infinity in as an operand or as the running sum — test_exceptional_pairs_in_bucket_lists_match_the_oracle on Fq2"""
    n = 8192
    bases = pool[:n].copy()
    sc = np.repeat(random_fr_canonical(n // 4, 0x62500001), 4, axis=0)
    for g in range(n // 4):
        p, q_ = bases[4 * g].copy(), bases[4 * g + 1].copy()
        kind = g % 4
        if kind == 0:
            bases[4 * g: 4 * g + 4] = p
        elif kind == 1:
            bases[4 * g + 1] = neg_affine(p); bases[4 * g + 2] = q_; bases[4 * g + 3] = 0
        elif kind == 2:
            bases[4 * g + 1] = q_; bases[4 * g + 2] = neg_affine(q_); bases[4 * g + 3] = neg_affine(p)
        else:
            bases[4 * g] = 0; bases[4 * g + 1] = 0; bases[4 * g + 2] = p; bases[4 * g + 3] = p
    assert np.array_equal(zkg.msm_g2(bases, sc), _oracle_g2(oracle, bases, sc))


# ---- 5. heavy buckets among ordinary ones -----------------------------------------------------------------------------------------------
def _heavy_among_ordinary(bases, seed):
    """n = 4096: the first 1536 entries share one scalar (three heavy parts per window: 512 x P, 512 x P / -P in turn, 512 x Q), the rest is
    uniform on distinct bases"""
    n = 4096
    bases = bases[:n].copy()
    p, q_ = bases[0].copy(), bases[1].copy()
    bases[:512] = p
    bases[512:1024:2] = p; bases[513:1024:2] = neg_affine(p)
    bases[1024:1536] = q_
    sc = random_fr_canonical(n, seed)
    sc[:1536] = sc[0]
    return bases, sc


def test_msm_g2_heavy_bucket_of_equal_and_opposite_points(zkg, oracle, pool):
    bases, sc = _heavy_among_ordinary(pool, 0x62600001)
    assert np.array_equal(zkg.msm_g2(bases, sc), _oracle_g2(oracle, bases, sc))


def test_msm_g1_heavy_bucket_of_equal_and_opposite_points(zkg, oracle):
    _, all_bases, _ = dev_bases_g1(zkg, 4096, 0x62600002)
    bases, sc = _heavy_among_ordinary(all_bases, 0x62600003)
    assert np.array_equal(zkg.msm_g1(bases, sc), oracle.msm_g1(bases, sc, oracle.BDLO12, oracle.num_threads()))


# ---- 6. witness-like scalars at the two-pass size ---------------------------------------------------------------------------------------
def test_msm_g2_mostly_bits_flag_does_not_change_the_result(zkg, oracle, pool):
    """n = 50 000 (c = 16, two-pass sort by default), 97 % of the scalars 0 or 1: ZKG_SCALARS_MOSTLY_BITS selects the one-pass sort and the
    point stays the oracle's.  The bases past the pool's end repeat its first ones (848 duplicated bases under different scalars)."""
    n = 50000
    bases = np.ascontiguousarray(pool[np.arange(n) % POOL])
    sc = random_fr_canonical(n, 0x62700001)
    rng = np.random.default_rng(5)
    bits = rng.random(n) < 0.97
    sc[bits] = 0; sc[bits, 0] = rng.integers(0, 2, int(bits.sum())).astype(np.uint64)
    exp = _oracle_g2(oracle, bases, sc, oracle.MIXED)
    d_b, d_s = to_dev(bases), to_dev(sc)
    assert np.array_equal(zkg.msm_g2_dev(d_b.data_ptr(), d_s.data_ptr(), n), exp)
    assert np.array_equal(zkg.msm_g2_dev(d_b.data_ptr(), d_s.data_ptr(), n, mostly_bits=True), exp)


# ---- 7. the two helpers no test called --------------------------------------------------------------------------------------------------
def test_g2_sum_matches_oracle(zkg, oracle, pool):
    n = 300
    aff = pool[1000:1000 + n].copy()
    aff[10] = aff[11]                                                # P next to P
    aff[20] = neg_affine(aff[21])                                    # -P next to P
    aff[0] = aff[1]; aff[2] = aff[3] = neg_affine(aff[1])            # the running sum doubles, then cancels to infinity
    aff[30] = 0; aff[31] = 0; aff[299] = 0                           # infinities, two of them neighbours
    pts = np.stack([g2_jac_of_affine(a) for a in aff])
    assert np.array_equal(zkg.g2_sum(pts), oracle.g2_sum(pts))
    assert np.array_equal(zkg.g2_sum(pts[:4]), g2_jac_expected(None))
    assert np.array_equal(zkg.g2_sum(pts[:0]), g2_jac_expected(None))                    # empty
    assert np.array_equal(zkg.g2_sum(pts[5:6]), pts[5])                                  # one point
    assert np.array_equal(zkg.g2_sum(pts[30:31]), g2_jac_expected(None))                 # one point, at infinity


def test_fixed_base_g2_matches_oracle(zkg, oracle):
    import torch
    n = 300
    ks = random_fr_canonical(n, 0x62800001)
    ks[0] = 0; ks[1] = limbs(1); ks[2] = limbs(2); ks[3] = limbs(R - 1)
    d_k = to_dev(ks)
    d_out = torch.empty((n, 16), dtype=torch.int64, device="cuda")
    zkg.fixed_base_g2_dev(oracle.g2_generator(), d_k.data_ptr(), n, d_out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), oracle.g2_fixed_base(oracle.g2_generator(), ks))


# ---- 8. the SMALL reduction for Fq2: no natural size selects it (c = 12 stays below 2^16 buckets, c = 16 jumps to 2^19) -------------------
def test_msm_g2_small_reduction_form(zkg, oracle, point_g2):
    """k_bucket_reduce<Fq2, SMALL> (four buckets per logical lane) through the tuning switch ZKG_RED_L_LOG=2, in a process of its own (the
    switch is read once): 4096 one-point bases, uniform scalars, against the one-point reference"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import zklaim_amd as zkg
from gpu_util import one_point_case
zkg.init(0)
p = np.frombuffer(bytes.fromhex(sys.argv[2]), np.uint64)
bases, sc, _ = one_point_case(p, 4096, "uniform", 0x62900001)
print(zkg.msm_g2(bases, sc).tobytes().hex())
'''
    r = subprocess.run([sys.executable, "-c", code, root, point_g2.tobytes().hex()], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ZKG_RED_L_LOG="2"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.frombuffer(bytes.fromhex(r.stdout.strip().splitlines()[-1]), np.uint64)
    _, _, S = one_point_case(point_g2, 4096, "uniform", 0x62900001)
    assert np.array_equal(got, _one_point_expected_g2(oracle, point_g2, S))
