"""CPU suite: the point codec of the proving-key blob on the host (zkg_point_decompress / zkg_point_compress with where = 0: ser::get_g1 /
get_g2 with the canonical check, ser::put_g1 / put_g2) against oracle/pyref.py's deser_* / ser_*, the hooks' argument contract, and the
index-list order zkg_pk_blob_inspect's walk asks for.  The cases are tests/point_codec_cases.py's, the ones tests/test_gpu_point_codec.py
runs on the loader's and the key writer's kernels: one rule, the same verdicts."""
import ctypes as C

import numpy as np
import pytest

import point_codec_cases as pc
import pyref
import zklaim_amd as zkg
from r1cs_util import golden_case_arrays
from util import golden

HOST = 0


@pytest.fixture(scope="module")
def pool(oracle):
    return pc.pool(oracle)


def test_reference_square_roots():
    """pyref.f2_sqrt against squares and non-squares built from the definition"""
    rng = np.random.default_rng(3)
    for _ in range(20):
        a = (int.from_bytes(rng.bytes(32), "little") % pyref.Q, int.from_bytes(rng.bytes(32), "little") % pyref.Q)
        sq = pyref.f2_mul(a, a)
        r = pyref.f2_sqrt(sq)
        assert r in (a, pyref.f2_neg(a))
        # xi = 9 + u is a non-residue of Fq2 (the tower is built on it): xi a^2 has no root
        assert pyref.f2_sqrt(pyref.f2_mul((9, 1), sq)) is None
    assert pyref.f2_sqrt((4, 0)) in ((2, 0), (pyref.Q - 2, 0)) and pyref.f2_sqrt((pyref.Q - 4, 0)) in ((0, 2), (0, pyref.Q - 2))


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
@pytest.mark.parametrize("n", pc.COUNTS)
def test_decompress_matches_the_reference(pool, layout, n):
    pc.check_decompress(zkg, pool, layout, n, HOST)


def test_square_root_branches_random_points_never_reach(pool):
    pc.check_sqrt_branches(zkg, pool, HOST)


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
def test_refusals_planted_at_the_edges(pool, layout):
    pc.check_refusals_planted(zkg, pool, layout, HOST)


@pytest.mark.parametrize("layout", pc.LAYOUTS, ids=pc.LAYOUT_IDS)
def test_refusals_side_by_side(pool, layout):
    pc.check_refusals_side_by_side(zkg, pool, layout, HOST)


@pytest.mark.parametrize("n", pc.COUNTS)
def test_compress_g1_records(pool, n):
    pc.check_compress_g1(zkg, pool, n, HOST)


@pytest.mark.parametrize("n", pc.COUNTS)
def test_compress_commitment_records(pool, n):
    pc.check_compress_kc(zkg, pool, n, HOST)


def test_compress_commitments_through_a_permutation(pool):
    pc.check_compress_kc_permuted(zkg, pool, HOST)


def test_round_trip(pool):
    pc.check_round_trip(zkg, pool, HOST)


def test_hooks_refuse_bad_arguments(pool):
    L = zkg.lib()
    L.zkg_point_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.zkg_point_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rec = np.frombuffer(b"".join(pool.rec2[i] + pool.rec1[i] for i in range(4)), np.uint8).copy()
    out = np.zeros((4, 16), np.uint64); flag = C.c_uint32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(rc, word):
        assert rc == zkg.ERROR and word in L.zkg_last_error().decode(), L.zkg_last_error()

    for where in (0, 1):                                     # (where = 1 is refused for its arguments before any GPU is asked for, or for the missing zkg_init)
        for args in ((None, 34, 0, 4, 0, where, p(out), C.byref(flag)), (p(rec), 34, 0, 4, 0, where, None, C.byref(flag)), (p(rec), 34, 0, 4, 0, where, p(out), None)):
            assert L.zkg_point_decompress(*args) == zkg.ERROR
    refused(L.zkg_point_decompress(p(rec), 34, 0, 4, 0, 2, p(out), C.byref(flag)), "where")
    for stride, off, g2 in ((35, 0, 0), (66, 0, 0), (34, 0, 1), (100, 34, 0), (100, 66, 1), (100, 67, 0), (0, 0, 0), (100, 0, 2)):
        refused(L.zkg_point_decompress(p(rec), stride, off, 1, g2, HOST, p(out), C.byref(flag)), "layouts")
    refused(L.zkg_point_decompress(p(rec), 34, 0, (1 << 20) + 1, 0, HOST, p(out), C.byref(flag)), "2^20")
    assert L.zkg_point_decompress(None, 34, 0, 0, 0, HOST, None, C.byref(flag)) == zkg.OK and flag.value == 0       # nothing to do

    g1 = pool.g1[:4].copy(); g2 = pool.g2[:4].copy(); idx = np.arange(4, dtype=np.uint32); rout = np.zeros(400, np.uint8)
    for bad_rec in (0, 33, 35, 66, 99, 134):
        refused(L.zkg_point_compress(p(g1), p(g2), p(idx), 4, 4, bad_rec, HOST, p(rout), None), "34 bytes")
    refused(L.zkg_point_compress(p(g1), p(g2), p(idx), 4, 4, 34, 2, p(rout), None), "where")
    refused(L.zkg_point_compress(None, None, None, 4, 4, 34, HOST, p(rout), None), "null")
    refused(L.zkg_point_compress(p(g1), None, None, 4, 4, 34, HOST, None, None), "null")
    refused(L.zkg_point_compress(p(g1), None, p(idx), 4, 4, 100, HOST, p(rout), None), "null")
    refused(L.zkg_point_compress(p(g1), p(g2), None, 4, 4, 100, HOST, p(rout), None), "null")
    refused(L.zkg_point_compress(p(g1), None, None, 4, 5, 34, HOST, p(rout), None), "more records than points")
    for at in (0, 3):
        far = idx.copy(); far[at] = 4
        refused(L.zkg_point_compress(p(g1), p(g2), p(far), 4, 4, 100, HOST, p(rout), None), "beyond")
    refused(L.zkg_point_compress(p(g1), None, None, (1 << 20) + 1, 4, 34, HOST, p(rout), None), "2^20")
    refused(L.zkg_point_compress(p(g1), p(g2), p(idx), 4, (1 << 20) + 1, 100, HOST, p(rout), None), "2^20")
    assert L.zkg_point_compress(p(g1), None, None, 4, 0, 34, HOST, None, None) == zkg.OK                              # nothing to do
    # and the wrappers still work afterwards
    assert zkg.point_compress(g1, rec=34, where=HOST)[0] == b"".join(pool.rec1[:4])


# ---- the loader's host walk ------------------------------------------------------------------------------------------------------------
def _blob(oracle, case, keep):
    A, B, C_, pts, w, r, s = golden_case_arrays(case)
    ocs = oracle.make_r1cs(case["num_variables"], case["num_inputs"], A, B, C_, keep)
    return oracle.pk_write_blob(oracle.make_pk(ocs, pts))


def test_index_list_must_be_strictly_increasing(oracle):
    """a repeated index would make the loader's scatter write one slot of the dense B query from two lanes; libsnark's sparse_vector is
    strictly increasing by construction, so the walk refuses every other order"""
    keep = []
    blob = _blob(oracle, golden("groth16.json")[1], keep)
    ok = zkg.pk_blob_inspect(blob)
    for name, bad in pc.disordered_index_blobs(blob):
        with pytest.raises(zkg.ZkgError, match="B_query index"):
            zkg.pk_blob_inspect(bad)
    assert zkg.pk_blob_inspect(pc.with_index_list(blob, pc.blob_sections(blob)["idx"][2])) == ok       # the rebuilt list itself is the blob's
    assert zkg.pk_blob_inspect(blob) == ok


def test_damaged_point_records_keep_the_sections(oracle):
    """the point damages of the loader test leave the host walk's view alone: what refuses them is the decompression"""
    keep = []
    blob = _blob(oracle, golden("groth16.json")[1], keep)
    ok = zkg.pk_blob_inspect(blob)
    cases = pc.damaged_point_blobs(blob)
    assert [n for n, _ in cases] == ["A_plus_q", "A_plus_2q", "A_parity_7", "B_g2_plus_q", "B_g2_plus_2q", "B_g2_parity_7"]
    for name, bad in cases:
        assert zkg.pk_blob_inspect(bad) == ok, name
