"""GPU suite: which path decided the verdicts of zkg_groth16_verify_batch (zkg_verify_batch_stats).  Equal verdicts alone cannot tell the
GPU's combined check from a fall-back to the single verifier: a batch of valid proofs must take exactly one combined check and no single
decision, a B outside G2 must be sent to the single verifier by the GPU's membership test, and a B inside G2 must pass that test."""
import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from test_gpu_verify_batch import WideKey, fixed_base, invalid_variants
from util import MONT, Q, R, arr, random_fr_canonical

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wide(zkg):
    k1, k2 = WideKey(zkg, 0xD1), WideKey(zkg, 0xD2)
    pool = [k1.proof() for _ in range(1000)]
    yield k1, k2, pool
    k1.free(); k2.free()


def batch(zkg, items):
    got = zkg.groth16_verify_batch(items)
    stats = zkg.verify_batch_stats()
    ref = np.array([zkg.groth16_verify(*it) for it in items], np.uint8)
    assert np.array_equal(got, ref)
    return got, stats


@pytest.mark.parametrize("n", [1, 64, 1000])
def test_valid_batch_is_one_combined_check(zkg, wide, n):
    got, stats = batch(zkg, wide[2][:n])
    assert not got.any()
    assert stats == (1, 0, 0)                                  # no single-verifier decision, no B refused by k_g2_subgroup


def test_invalid_proof_is_found_by_bisection(zkg, wide):
    _, _, pool = wide
    x = pool[5][1].copy(); x[2] = arr([99], R)[0]
    items = list(pool[:64]); items[37] = (pool[5][0], x, pool[5][2])
    got, (checks, alone, outside) = batch(zkg, items)
    assert got[37] == 1 and got.sum() == 1
    assert 1 < checks <= 2 * 6 and 1 <= alone <= 4 and outside == 0


def test_b_outside_g2_is_refused_by_the_gpu_test(zkg, wide):
    _, _, pool = wide
    outside = [it for name, it, _ in invalid_variants(wide) if name == "B_outside_G2"][0]
    got, stats = batch(zkg, [outside])
    assert list(got) == [1] and stats == (0, 1, 1)
    got, stats = batch(zkg, list(pool[:100]) + [outside] + list(pool[100:130]))
    assert got[100] == 1 and got.sum() == 1 and stats == (1, 1, 1)    # the others still pass as one combination


def compress_g2(pt):
    """libsnark's compressed G2 record of an affine point given as 16 Montgomery limbs"""
    v = [sum(int(pt[4 * c + k]) << (64 * k) for k in range(4)) for c in range(4)]
    y0 = v[2] * pow(MONT, -1, Q) % Q
    return b"0" + b"".join(x.to_bytes(32, "little") for x in v[:2]) + (b"1" if y0 & 1 else b"0")


def test_b_inside_g2_passes_the_gpu_test(zkg, wide):
    """B replaced by multiples of the G2 generator: wrong proofs, but every B is in G2, so none is refused by k_g2_subgroup"""
    _, _, pool = wide
    Bs = fixed_base(zkg, True, random_fr_canonical(6, 0xD3))
    items = [(vk, x, pr[:34] + compress_g2(Bs[j]) + pr[100:]) for j, (vk, x, pr) in enumerate(pool[200:206])]
    got, (checks, alone, outside) = batch(zkg, list(pool[:40]) + items)
    assert got[40:].all() and not got[:40].any()
    assert outside == 0 and alone >= 6 and checks >= 2


def test_swapped_c_points_fail_the_combination(zkg, wide):
    k1, _, pool = wide
    w = arr(list(range(3, 3 + k1.n)), R)
    (vk, x, p1), (_, _, p2) = k1.proof(w), k1.proof(w)
    got, (checks, alone, outside) = batch(zkg, [(vk, x, p1[:100] + p2[100:]), (vk, x, p2[:100] + p1[100:])])
    assert list(got) == [1, 1] and checks == 1 and alone == 2 and outside == 0
