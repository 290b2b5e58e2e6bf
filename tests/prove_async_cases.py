"""Shared by the zkg_prover tests: a synthetic key as test_gpu_prove_batch._synthetic_key builds its own, and the inputs of zkg_proof_assemble
(the key's points, the five points of a proof) computed with the oracle."""
import numpy as np

from util import Q, R, arr, from_limbs, limbs, random_fr_canonical

G1_INF_JAC = arr([0, 1, 0], Q).reshape(12)
G2_INF_JAC = arr([0, 0, 1, 0, 0, 0], Q).reshape(24)


def trivial_system(n):
    """x_i * 1 = x_i for every variable: satisfied by ANY assignment (one public input); test_gpu_groth16._trivial_system without the GPU imports"""
    rp = np.arange(n + 1, dtype=np.uint32); cols = np.arange(1, n + 1, dtype=np.uint32)
    one = np.tile(arr([1], R), (n, 1))
    return n, 1, (rp, cols, one), (rp, np.zeros(n, np.uint32), one), (rp, cols, one)


def oracle_key(oracle, n, seed, keep):
    """(oracle constraint system, oracle pk, key arrays) of the trivial system over n variables"""
    n_, l, A, B, C = trivial_system(n)
    ocs = oracle.make_r1cs(n, l, A, B, C, keep)
    arrays = oracle.groth16_setup(ocs, random_fr_canonical(5, seed))
    return ocs, oracle.make_pk(ocs, arrays), arrays, (n, l, A, B, C)


def neg_affine(b):
    out = np.array(b, np.uint64).copy()
    for k in range(out.size // 2, out.size, 4):
        out[k:k + 4] = limbs((Q - from_limbs(out[k:k + 4])) % Q)
    return out


def affine_of_jac(p):
    """a normalised point (12 / 24 limbs) as the affine one (8 / 16 limbs, all-zero = infinity)"""
    p = np.asarray(p, np.uint64).reshape(-1)
    k = p.size // 3
    return np.zeros(2 * k, np.uint64) if not p[2 * k:].any() else p[:2 * k].copy()


def jac_of_affine(a):
    a = np.asarray(a, np.uint64).reshape(-1)
    if not a.any():
        return (G1_INF_JAC if a.size == 8 else G2_INF_JAC).copy()
    return np.concatenate([a, arr([1], Q).reshape(4) if a.size == 8 else arr([1, 0], Q).reshape(8)])


def key_points(arrays):
    """alpha_g1 | beta_g1 | delta_g1 | A_0 | B1_0 | beta_g2 | delta_g2 | B2_0: 88 limbs"""
    return np.concatenate([arrays["alpha_g1"], arrays["beta_g1"], arrays["delta_g1"], arrays["A_query"][0], arrays["B_g1"][0],
                           arrays["beta_g2"], arrays["delta_g2"], arrays["B_g2"][0]]).astype(np.uint64)


def five_points(oracle, ocs, arrays, vals):
    """W_a | W_b1 | L | H | W_b2 of the witness `vals` (ints): the sums over [1 | w] with the constant column's point subtracted — 72 limbs"""
    n, l, m = len(vals), ocs.num_inputs, arrays["m"]
    z = arr([1] + [int(v) for v in vals])                                    # canonical scalars
    wa = oracle.g1_add(affine_of_jac(oracle.msm_g1(arrays["A_query"], z)), neg_affine(arrays["A_query"][0]))
    wb1 = oracle.g1_add(affine_of_jac(oracle.msm_g1(arrays["B_g1"], z)), neg_affine(arrays["B_g1"][0]))
    wb2 = oracle.g2_add(affine_of_jac(oracle.msm_g2(arrays["B_g2"], z)), neg_affine(arrays["B_g2"][0]))
    lq = oracle.msm_g1(arrays["L_query"], z[l + 1:]) if n > l else G1_INF_JAC
    h = oracle.qap_witness_h(ocs, arr(vals, R), m)                           # Montgomery coefficients
    h_can = arr([x for x in _from_mont(h[:m - 1])])
    hp = oracle.msm_g1(arrays["H_query"], h_can)
    return np.concatenate([wa, wb1, lq, hp, wb2]).astype(np.uint64)


def _from_mont(a):
    rinv = pow(1 << 256, -1, R)
    return [from_limbs(r) * rinv % R for r in np.asarray(a, np.uint64).reshape(-1, 4)]
