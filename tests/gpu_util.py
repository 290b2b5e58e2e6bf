"""Shared fixtures for the -m gpu parity tests (HIP path through the C ABI vs the CPU oracle)."""
import numpy as np
import pytest

import zklaim_amd
from util import random_fr_canonical


@pytest.fixture(scope="session")
def zkg():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from zklaim_amd import build
    build.build()
    zklaim_amd.init(0)
    yield zklaim_amd
    zklaim_amd.shutdown()


def dev_bases_g1(zkg, n, seed):
    """n synthetic G1 bases k_i*G generated ON DEVICE by the product's fixed-base kernel; returns (torch tensor, numpy copy)."""
    import torch
    ks = random_fr_canonical(n, seed)
    d_k = torch.from_numpy(ks.view(np.int64)).cuda()
    d_out = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    g1 = np.zeros(8, np.uint64)
    g1[:4] = [0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f]
    g1[4:] = [0xa6ba871b8b1e1b3a, 0x14f1d651eb8e167b, 0xccdd46def0f28c58, 0x1c14ef83340fbe5e]
    zkg.fixed_base_g1_dev(g1, d_k.data_ptr(), n, d_out.data_ptr())
    torch.cuda.synchronize()
    return d_out, d_out.cpu().numpy().view(np.uint64), ks


def to_dev(a):
    """a uint64 limb array as a device tensor (the *_dev entry points take its data_ptr())"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a if a.flags.writeable else a.copy()).view(np.int64)).cuda()


def neg_affine(b):
    """-P of an affine point of 8 (G1) or 16 (G2) Montgomery limbs: (x, -y), for G2 on both Fq2 coefficients; infinity stays infinity"""
    from util import Q, from_limbs, limbs
    out = np.array(b, np.uint64).copy()
    for k in range(out.size // 2, out.size, 4):
        out[k:k + 4] = limbs((Q - from_limbs(out[k:k + 4])) % Q)
    return out


def g2_jac_of_affine(a):
    """the normalised 24-limb point the ABI returns for a 16-limb affine one (all-zero = infinity)"""
    from util import Q, arr, g2_jac_expected
    a = np.asarray(a, np.uint64).reshape(16)
    if not a.any():
        return g2_jac_expected(None)
    return np.concatenate([a, arr([1, 0], Q).reshape(8)])


def r_minus(sc):
    """r - s for canonical scalars 0 < s < r, limb-wise with borrow"""
    from util import R_LIMBS
    out = np.empty_like(sc); borrow = np.zeros(len(sc), np.uint64)
    with np.errstate(over="ignore"):
        for j in range(4):
            d = R_LIMBS[j] - sc[:, j]
            out[:, j] = d - borrow
            borrow = ((R_LIMBS[j] < sc[:, j]) | (d < borrow)).astype(np.uint64)
    assert not borrow.any()
    return out


def signed_scalar_sum(sc, eps):
    """sum eps_i * s_i mod r with Python integers (eps_i in {-1, 0, 1}; the 32-bit halves of every limb column are summed exactly in int64)"""
    from util import R
    eps = np.asarray(eps, np.int64); tot = 0
    for j in range(4):
        lo = (sc[:, j] & np.uint64(0xFFFFFFFF)).astype(np.int64); hi = (sc[:, j] >> np.uint64(32)).astype(np.int64)
        tot += (int((lo * eps).sum()) + (int((hi * eps).sum()) << 32)) << (64 * j)
    return tot % R


ONE_POINT_PATTERNS = ("uniform", "equal", "alt1", "alt2", "alt64", "zero_sum", "third_inf")


def one_point_case(p, n, pattern, seed):
    """An MSM whose bases are all P, -P or infinity, so that it equals S * P with S = sum eps_i s_i mod r: -> (bases, scalars, S).
    uniform: all P, uniform scalars (every bucket a small multiple of P); equal: all P, one scalar (one bucket per window holds everything);
    altK: P and -P in runs of K under one scalar; zero_sum: all P, the second half of the scalars r - the first half (S = 0);
    third_inf: infinity, P, -P in turn, uniform scalars.  n is even."""
    p = np.asarray(p, np.uint64).reshape(-1)
    eps = np.ones(n, np.int64)
    if pattern == "uniform":
        sc = random_fr_canonical(n, seed)
    elif pattern == "equal":
        sc = np.tile(random_fr_canonical(1, seed), (n, 1))
    elif pattern.startswith("alt"):
        sc = np.tile(random_fr_canonical(1, seed), (n, 1))
        eps = np.where((np.arange(n) // int(pattern[3:])) % 2 == 0, 1, -1)
    elif pattern == "zero_sum":
        half = random_fr_canonical(n // 2, seed)
        sc = np.concatenate([half, r_minus(half)])
    elif pattern == "third_inf":
        sc = random_fr_canonical(n, seed)
        eps = np.array([0, 1, -1])[np.arange(n) % 3]
    else:
        raise ValueError(pattern)
    bases = np.zeros((n, p.size), np.uint64)
    bases[eps == 1] = p; bases[eps == -1] = neg_affine(p)
    return bases, np.ascontiguousarray(sc), signed_scalar_sum(sc, eps)


def adversarial_scalars(n, seed):
    """the five digit distributions of test_msm_adversarial_scalar_distributions: name -> (n, 4) canonical scalars"""
    from util import R, limbs
    rng = np.random.default_rng(seed)
    tiny = np.zeros((n, 4), np.uint64); tiny[:, 0] = rng.integers(0, 1000, n).astype(np.uint64)
    k = rng.integers(0, 253, n)
    pow2 = np.zeros((n, 4), np.uint64); pow2[np.arange(n), k // 64] = np.uint64(1) << (k % 64).astype(np.uint64)
    return {"same": np.tile(random_fr_canonical(1, seed + 1), (n, 1)), "two": np.ascontiguousarray(random_fr_canonical(2, seed + 2)[rng.integers(0, 2, n)]),
            "tiny": tiny, "pow2": pow2, "r-1": np.tile(np.array(limbs(R - 1), np.uint64), (n, 1))}


def credential_payloads(k):
    """k satisfiable payloads (the workload of bench.py's prove legs)"""
    return [dict(attrs=[1990 + i, 7 * i, 42, i, 5], refs=[2100, 7 * i, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=0x5A4B + i)
            for i in range(k)]


def oracle_pk_from_keypair(oracle, kp, csr, nv, l, keep):
    """the oracle's view of a key made by the product's generator: same arrays, A and B exchanged back when the generator swapped them"""
    A, B, C = csr
    if kp.swapped:
        A, B = B, A
    ocs = oracle.make_r1cs(nv, l, A, B, C, keep)
    m = kp.pk.domain_size or (1 << kp.pk.log_m)
    arrays = {name: kp.array(name, cnt, lim) for name, cnt, lim in (("A_query", nv + 1, 8), ("B_g1", nv + 1, 8), ("B_g2", nv + 1, 16), ("H_query", m - 1, 8),
              ("L_query", nv - l, 8), ("alpha_g1", 1, 8), ("beta_g1", 1, 8), ("delta_g1", 1, 8), ("beta_g2", 1, 16), ("delta_g2", 1, 16))}
    arrays["m"] = m
    keep.append(arrays)
    return ocs, oracle.make_pk(ocs, arrays), m
