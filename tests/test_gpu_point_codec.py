"""GPU: the point codec of the proving-key blob.  k_decompress_g1 / k_decompress_g2 through the loader's own decompress_dev
(zkg_point_decompress, where = 1) against oracle/pyref.py's deser_g1 / deser_g2, k_compress_records<34> / <100> through the key writer's
compress_g1_records / compress_kc_records (zkg_point_compress, where = 1) against ser_g1 / ser_g2, and the same rule through the whole
loader (zkg_crs_upload_blob) and through the proof decoder's k_proof_decode, which shares the square roots.  The cases are
tests/point_codec_cases.py's; tests/test_point_codec_host.py runs them on the host's decoder and writer.

The rule (pyref.deser_*): '1' first is infinity and nothing else is read; otherwise the flag is '0', the parity byte '0' or '1', every x
coordinate's limbs are below q, x^3 + b is a square, and y is the root whose canonical lsb is the parity byte.  Before the kernels asked
for the parity byte and for x < q, they took any parity byte but '1' as '0' and an x in [q, 2q) as a second encoding of x - q; for
x in [2q, 2^256) they computed outside the lazy range of csrc/fp.hip.hpp.  Measured on those kernels with these cases (eight pool records
per variant): the parity bytes '7' and NUL and x + q were accepted in every layout (flag 0); x + 2q was accepted in G1 and on G2's c0 and
stored the point with limbs >= q; on G2's c1 it was refused for six records of eight and gave another point with limbs >= q for two;
2^256 - 1 was refused in G1 and gave such a point in G2 for three (c0) and five (c1) records of eight."""
import numpy as np
import pytest

import point_codec_cases as pc
import pyref
from gpu_util import zkg  # noqa: F401
from r1cs_util import golden_case_arrays
from util import golden

pytestmark = pytest.mark.gpu
GPU = 1


@pytest.fixture(scope="module")
def pool(oracle):
    return pc.pool(oracle)


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
@pytest.mark.parametrize("n", pc.COUNTS)
def test_decompress_matches_the_reference(zkg, pool, layout, n):
    pc.check_decompress(zkg, pool, layout, n, GPU)


def test_square_root_branches_random_points_never_reach(zkg, pool):
    """fq2_sqrt's a.c1 == 0 branch (a real root, a purely imaginary one, both parity bytes), a non-residue norm, x = 0 in G2 and in G1,
    through k_decompress_g2 / k_decompress_g1"""
    pc.check_sqrt_branches(zkg, pool, GPU)


def test_square_root_branches_through_the_proof_decoder(zkg, pool):
    """the same G2 records as a proof's B, through k_proof_decode (it shares csrc/sqrt.hip.hpp): bit 1 of the flag byte is the
    reference's verdict, the point the reference's, A and C untouched"""
    cases = pc.sqrt_branch_records()
    n = len(cases)
    proofs = np.stack([np.frombuffer(pool.rec1[i] + rec + pool.rec1[n + i], np.uint8) for i, (_, rec, _) in enumerate(cases)])
    A, B, Cc, ok = zkg.proof_decode_gpu(proofs)
    for i, (name, rec, P) in enumerate(cases):
        assert np.array_equal(B[i], pc.limbs_g2(P)), name
        assert ok[i] == (5 if P == pyref.REFUSED else 7), name
    assert np.array_equal(A, pool.ref1[:n]) and np.array_equal(Cc, pool.ref1[n:2 * n])
    g1 = pc.g1_x_zero_records()
    proofs = np.stack([np.frombuffer(rec + pool.rec2[i] + pool.rec1[i], np.uint8) for i, (rec, _) in enumerate(g1)])
    A, B, Cc, ok = zkg.proof_decode_gpu(proofs)
    for i, (rec, P) in enumerate(g1):
        assert np.array_equal(A[i], pc.limbs_g1(P)) and ok[i] == (6 if P == pyref.REFUSED else 7)


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
def test_refusals_planted_at_the_edges(zkg, pool, layout):
    pc.check_refusals_planted(zkg, pool, layout, GPU)


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
def test_refusals_side_by_side(zkg, pool, layout):
    pc.check_refusals_side_by_side(zkg, pool, layout, GPU)


@pytest.mark.parametrize("n", pc.COUNTS)
def test_compress_g1_records(zkg, pool, n):
    pc.check_compress_g1(zkg, pool, n, GPU)


@pytest.mark.parametrize("n", pc.COUNTS)
def test_compress_commitment_records(zkg, pool, n):
    pc.check_compress_kc(zkg, pool, n, GPU)


def test_compress_commitments_through_a_permutation(zkg, pool):
    pc.check_compress_kc_permuted(zkg, pool, GPU)


def test_round_trip(zkg, pool):
    pc.check_round_trip(zkg, pool, GPU)


def test_host_and_device_write_the_same_records(zkg, pool):
    assert zkg.point_compress(pool.g1, rec=34, where=GPU) == zkg.point_compress(pool.g1, rec=34, where=0)
    idx = pc.gapped_indices(513, 9)
    assert zkg.point_compress(pool.g1, pool.g2, idx, rec=100, where=GPU) == zkg.point_compress(pool.g1, pool.g2, idx, rec=100, where=0)


# ---- through the loader ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_blob(oracle):
    case = golden("groth16.json")[1]
    A, B, C, pts, w, r, s = golden_case_arrays(case)
    keep = []
    ocs = oracle.make_r1cs(case["num_variables"], case["num_inputs"], A, B, C, keep)
    return case, oracle.pk_write_blob(oracle.make_pk(ocs, pts)), (w, r, s), keep


def _proves_the_golden_proof(zkg, case, blob, wrs):
    crs = zkg.Crs(blob=blob, m=case["m"])
    rc, proof = crs.prove(*wrs)
    crs.free()
    return rc == 0 and proof.hex() == case["proof_hex"]


def test_loader_refuses_malformed_points(zkg, golden_blob):
    """one A-query record, then one B-query G2 record, as x + q, x + 2q and with the parity byte '7': no key, and the loader still
    works afterwards"""
    case, blob, wrs, _ = golden_blob
    assert _proves_the_golden_proof(zkg, case, blob, wrs)
    for name, bad in pc.damaged_point_blobs(blob):
        with pytest.raises(zkg.ZkgError, match="malformed or not on the curve"):
            zkg.Crs(blob=bad, m=case["m"])
    assert _proves_the_golden_proof(zkg, case, blob, wrs)


def test_loader_refuses_a_disordered_index_list(zkg, golden_blob):
    case, blob, wrs, _ = golden_blob
    for name, bad in pc.disordered_index_blobs(blob):
        with pytest.raises(zkg.ZkgError, match="B_query index"):
            zkg.Crs(blob=bad, m=case["m"])
    assert _proves_the_golden_proof(zkg, case, blob, wrs)
