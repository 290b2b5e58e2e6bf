"""GPU parity: the proof epilogue kernels (zkg_proof_assemble, where = 1) against the host's assembly (where = 0, which
test_prove_async_host pins to the oracle prover), on points that are oracle multiples of the generators — so that the exceptional sums
(infinity, the doubling branch of an addition, A = O, C = O) can be placed by their discrete logarithms."""
import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from prove_async_cases import jac_of_affine
from util import R, arr, random_fr_canonical

pytestmark = pytest.mark.gpu
PROOFS_PER_GROUP = 8          # k_proof_g1_part: proofs one workgroup takes
LANES = 64                    # k_proof_g2_part, k_proof_finish: one lane per proof


def _ints(a):
    return [sum(int(v) << (64 * i) for i, v in enumerate(r)) for r in np.asarray(a, np.uint64).reshape(-1, 4)]


class Points:
    """k G1 / k G2 for every k asked, through ONE oracle fixed-base call per group at the end"""

    def __init__(self, oracle):
        self.oracle, self.k1, self.k2 = oracle, [], []

    def g1(self, k):
        self.k1.append(k % R); return len(self.k1) - 1

    def g2(self, k):
        self.k2.append(k % R); return len(self.k2) - 1

    def resolve(self):
        o = self.oracle
        self.p1 = o.g1_fixed_base(o.g1_generator(), arr(self.k1)) if self.k1 else np.zeros((0, 8), np.uint64)
        self.p2 = o.g2_fixed_base(o.g2_generator(), arr(self.k2)) if self.k2 else np.zeros((0, 16), np.uint64)
        for k, p in zip(self.k1, self.p1):
            assert p.any() == (k != 0)


@pytest.fixture(scope="module")
def cases(oracle):
    """the key's discrete logarithms, and a pool of proofs (W_a, W_b1, L, H, W_b2, r, s as scalars) — built once, shared by the tests"""
    key = [int(x) for x in _ints(random_fr_canonical(8, 0xE1))]               # alpha beta1 delta1 a0 b10 | beta2 delta2 b20
    al, be1, de1, a0, b10, be2, de2, b20 = key
    rnd = iter(_ints(random_fr_canonical(400, 0xE2)))
    edge = [0, 1, R - 1, next(rnd)]
    pool = []
    for r in edge:                                                            # r, s in {0, 1, r_mod - 1, random}: all sixteen pairs
        for s in edge:
            pool.append(dict(wa=next(rnd), wb1=next(rnd), l=next(rnd), h=next(rnd), wb2=next(rnd), r=r, s=s))
    r, s = next(rnd), next(rnd)
    u, v = next(rnd), next(rnd)
    c_fixed = lambda r_, s_: (s_ * al + r_ * be1 + r_ * s_ * de1) % R       # s alpha + r beta_1 + rs delta
    pool.append(dict(wa=-a0, wb1=next(rnd), l=next(rnd), h=next(rnd), wb2=next(rnd), r=r, s=s))                     # W_a = -A_0: the sum is infinity
    pool.append(dict(wa=None, wb1=None, l=None, h=None, wb2=None, r=r, s=s))                                         # every point infinity
    pool.append(dict(wa=None, wb1=None, l=None, h=None, wb2=None, r=0, s=0))
    v0 = (-s * u) * pow(r, -1, R) % R
    pool.append(dict(wa=u - a0, wb1=v0 - b10, l=next(rnd), h=next(rnd), wb2=next(rnd), r=r, s=s))                  # s W_a' + r W_b1' = O
    v1 = s * u * pow(r, -1, R) % R
    pool.append(dict(wa=u - a0, wb1=v1 - b10, l=next(rnd), h=next(rnd), wb2=next(rnd), r=r, s=s))                  # s W_a' = r W_b1': the addition doubles
    lk = next(rnd)
    pool.append(dict(wa=u - a0, wb1=v - b10, l=lk, h=c_fixed(r, s) + s * u + r * v + lk, wb2=next(rnd), r=r, s=s))  # H = the rest of C: the last addition doubles
    pool.append(dict(wa=(al + r * de1) - a0, wb1=v - b10, l=lk, h=next(rnd), wb2=be2 + s * de2 - b20, r=r, s=s))   # W_a' = alpha + r delta, W_b2' = beta + s delta_2: A and B double
    ua = -(al + r * de1) % R
    pool.append(dict(wa=ua - a0, wb1=v - b10, l=lk, h=-(c_fixed(r, s) + s * ua + r * v + lk), wb2=-(be2 + s * de2) - b20, r=r, s=s))   # A = O, B = O, C = O: three '1' records
    pool.append(dict(wa=u - a0, wb1=v - b10, l=None, h=-(c_fixed(r, s) + s * u + r * v), wb2=next(rnd), r=r, s=s))  # L = O and C = O
    pts = Points(oracle)
    kidx = [pts.g1(k) for k in key[:5]] + [pts.g2(k) for k in key[5:]]
    for c in pool:
        for name in ("wa", "wb1", "l", "h"):
            c[name + "_i"] = None if c[name] is None else pts.g1(c[name])
        c["wb2_i"] = None if c["wb2"] is None else pts.g2(c["wb2"])
    pts.resolve()
    key_points = np.concatenate([pts.p1[i] for i in kidx[:5]] + [pts.p2[i] for i in kidx[5:]])
    rows, rs = [], []
    for c in pool:
        g1 = [jac_of_affine(np.zeros(8, np.uint64) if c[n + "_i"] is None else pts.p1[c[n + "_i"]]) for n in ("wa", "wb1", "l", "h")]
        g2 = jac_of_affine(np.zeros(16, np.uint64) if c["wb2_i"] is None else pts.p2[c["wb2_i"]])
        rows.append(np.concatenate(g1 + [g2])); rs.append(np.concatenate([arr([c["r"]], R)[0], arr([c["s"]], R)[0]]))
    return key_points, np.array(rows, np.uint64), np.array(rs, np.uint64)


def test_the_pool_holds_the_records_it_is_meant_to(zkg, cases):
    """the specification's own bytes: where the cases place infinity the record is '1', elsewhere '0'"""
    kp, pts, rs = cases
    want = zkg.proof_assemble(kp, pts, rs, 0)
    flags = [(chr(p[0]), chr(p[34]), chr(p[100])) for p in want]
    assert flags[:16] == [("0", "0", "0")] * 16
    assert flags[-2] == ("1", "1", "1") and flags[-1] == ("0", "0", "1")
    assert len({p.tobytes() for p in want}) == len(want)                  # all distinct: no case degenerates into another


@pytest.mark.parametrize("count", [1, PROOFS_PER_GROUP - 1, PROOFS_PER_GROUP, PROOFS_PER_GROUP + 1, LANES - 1, LANES, LANES + 1])
def test_kernels_equal_the_host_assembly(zkg, cases, count):
    kp, pts, rs = cases
    n = len(pts)
    pick = [(3 * count + j) % n for j in range(count)] if count < n else list(range(n)) + [(7 * j) % n for j in range(count - n)]
    want = zkg.proof_assemble(kp, pts[pick], rs[pick], 0)
    got = zkg.proof_assemble(kp, pts[pick], rs[pick], 1)
    for j in range(count):
        assert got[j].tobytes() == want[j].tobytes(), (j, pick[j])


def test_every_case_of_the_pool(zkg, cases):
    kp, pts, rs = cases
    want = zkg.proof_assemble(kp, pts, rs, 0)
    got = zkg.proof_assemble(kp, pts, rs, 1)
    for j in range(len(pts)):
        assert got[j].tobytes() == want[j].tobytes(), j


def test_a_key_of_infinities(zkg, cases):
    """every key point and every input infinity: three '1' records; and the pool under a key whose constant column is empty"""
    kp, pts, rs = cases
    zero_key = np.zeros(88, np.uint64)
    got = zkg.proof_assemble(zero_key, pts[17:18], rs[17:18], 1)              # (case 17: every point infinity)
    assert got[0].tobytes() == zkg.proof_assemble(zero_key, pts[17:18], rs[17:18], 0)[0].tobytes()
    assert (chr(got[0][0]), chr(got[0][34]), chr(got[0][100])) == ("1", "1", "1")
    kp2 = kp.copy(); kp2[24:40] = 0; kp2[72:88] = 0                           # A_0 = B1_0 = B2_0 = O
    n = len(pts)
    assert zkg.proof_assemble(kp2, pts, rs, 1).tobytes() == zkg.proof_assemble(kp2, pts, rs, 0).tobytes()
    assert n > 20
