"""The piece-wise step with the host pacing its accumulations (msm.hip, msm_g1_host_scalars): an accumulation is enqueued once the calling
thread has seen its sort finish, and k_heavy_parts / k_heavy_merge follow it only where the count of heavy buckets that k_order_place stored
into pinned host memory is not zero.  n = 2^19 is the smallest size that takes the piece-wise path: c = 16, 16 windows of 2^15 buckets, pieces
[0, 65536), [65536, 131072), [131072, 262144), [262144, 524288).  Every result is compared with zkg_msm_g1_dev on the same inputs, bit for bit,
and zkg_msm_host_scalars_stats says what the host read and launched."""
import numpy as np
import pytest

from bench import splitmix_fr
from gpu_util import dev_bases_g1, to_dev, zkg  # noqa: F401
from util import R, limbs

pytestmark = pytest.mark.gpu

N = 1 << 19
PIECES = [(0, 65536), (65536, 131072), (131072, 262144), (262144, 524288)]
BLOCK = 4096
# sixteen non-zero 16-bit digits, none of them with its top bit set (no carry between signed digits), the top one below r's own 0x3064:
# 4096 copies put 4096 entries into one bucket of every window of a piece.  The accumulation's threshold (heavy_threshold_dev: four times the
# piece's average list length plus a slack of at most 32) is 63 or 64 in the last piece (average 8) and 28 in the first two (average 2); a
# uniform piece's longest list stays below it — the part-filled top window of the last piece is the closest, a Poisson mean of 21 over 12 388
# buckets against 64: about 10^-9 for any of them to pass.
EQUAL = np.array([0x1234123412341234] * 4, np.uint64)


def _with_block(sc, pieces):
    out = sc.copy()
    for p in pieces:
        lo, hi = PIECES[p]
        start = lo + (hi - lo) // 3
        out[start:start + BLOCK] = EQUAL
    return out


class _Inputs:
    def __init__(self, zkg):
        import torch
        self.zkg = zkg
        self.n_max = N + 256
        self.d_bases, self.bases, _ = dev_bases_g1(zkg, self.n_max, 0x9ACE)
        self.uniform = splitmix_fr(self.n_max, 0x9ACF)
        # the existing piece-wise test's edge inputs on top of a block in every piece: zeros, r - 1, a duplicated base and a base at infinity
        sc = _with_block(self.uniform[:N], [0, 1, 2, 3])
        kind = np.random.default_rng(0x9AD0).integers(0, 100, N)
        zero = kind < 7
        zero[[N - 1, N // 2]] = False
        sc[zero] = 0
        sc[N - 1] = limbs(R - 1); sc[N // 2] = limbs(R - 1)
        self.edge = np.ascontiguousarray(sc)
        bases = self.bases[:N].copy()
        bases[N // 2] = bases[N - 1]; bases[5] = 0
        self.edge_bases = bases
        self.d_edge_bases = torch.from_numpy(bases.view(np.int64)).cuda()
        self._pinned = {}
        self._expected = {}

    def expected(self, key, d_bases, sc, n):
        if key not in self._expected:
            d_sc = to_dev(sc[:n])
            self._expected[key] = self.zkg.msm_g1_dev(d_bases.data_ptr(), d_sc.data_ptr(), n)
        return self._expected[key]

    def oracle_uniform(self, oracle):
        """the oracle's point for the uniform scalars at N, computed once for the tests that compare with it"""
        if "oracle" not in self._expected:
            self._expected["oracle"] = oracle.msm_g1(self.bases[:N], self.uniform[:N], oracle.BDLO12, oracle.num_threads())
        return self._expected["oracle"]

    def pinned(self, key, sc):
        import torch
        if key not in self._pinned:
            self._pinned[key] = torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).pin_memory()
        return self._pinned[key]

    def run_uniform(self, n=N):
        sc = self.uniform[:n]
        got = self.zkg.msm_g1_host_scalars(self.d_bases.data_ptr(), self.pinned(("uniform", n), sc).data_ptr(), n)
        return got, self.expected(("uniform", n), self.d_bases, sc, n), self.zkg.msm_host_scalars_stats()

    def run_edge(self):
        got = self.zkg.msm_g1_host_scalars(self.d_edge_bases.data_ptr(), self.edge.ctypes.data, N)            # pageable memory
        return got, self.expected("edge", self.d_edge_bases, self.edge, N), self.zkg.msm_host_scalars_stats()


@pytest.fixture(scope="module")
def inputs(zkg):
    return _Inputs(zkg)


def _assert_uniform_stats(st):
    assert st["pieces"] == 4 and st["heavy"] == [0, 0, 0, 0] and st["pair"] == [False] * 4 and st["stream_waits"] == 0, st


def _assert_edge_stats(st):
    assert st["pieces"] == 4 and all(h >= 16 for h in st["heavy"]) and st["pair"] == [True] * 4 and st["stream_waits"] == 0, st


def test_uniform_scalars_launch_no_heavy_pair(inputs, oracle):
    got, exp, st = inputs.run_uniform()
    print("stats:", st)
    assert np.array_equal(got, exp)
    assert np.array_equal(got, inputs.oracle_uniform(oracle))
    _assert_uniform_stats(st)


@pytest.mark.parametrize("piece", [3, 1])
def test_equal_block_in_one_piece_launches_the_pair_there_only(inputs, piece):
    """piece 3: the last accumulation alone gets the pair; piece 1: the pieces after it resume the block's buckets as ordinary lanes"""
    zkg = inputs.zkg
    sc = _with_block(inputs.uniform[:N], [piece])
    got = zkg.msm_g1_host_scalars(inputs.d_bases.data_ptr(), inputs.pinned(("block", piece), sc).data_ptr(), N)
    st = zkg.msm_host_scalars_stats()
    print("stats:", st)
    assert np.array_equal(got, inputs.expected(("block", piece), inputs.d_bases, sc, N))
    assert st["pieces"] == 4 and st["stream_waits"] == 0, st
    assert st["pair"] == [k == piece for k in range(4)], st
    assert st["heavy"][piece] >= 16 and all(st["heavy"][k] == 0 for k in range(4) if k != piece), st      # one bucket in each of the 16 windows


def test_block_in_every_piece_with_edge_inputs_from_pageable_memory(inputs):
    got, exp, st = inputs.run_edge()
    print("stats:", st)
    assert np.array_equal(got, exp)
    _assert_edge_stats(st)


def test_three_calls_in_a_row_alternating_inputs(inputs):
    """the second and third call reuse ev_acc_done, both sets of sort buffers and the pinned words of the call before"""
    for k in range(3):
        got, exp, st = inputs.run_edge() if k == 1 else inputs.run_uniform()
        assert np.array_equal(got, exp), k
        (_assert_edge_stats if k == 1 else _assert_uniform_stats)(st)


def test_sizes_around_the_piece_wise_threshold(inputs):
    got, exp, st = inputs.run_uniform(N + 256)
    assert np.array_equal(got, exp)
    _assert_uniform_stats(st)
    got, exp, st = inputs.run_uniform(N - 256)                 # the single-launch path: one piece, no count read, the pair launched as before
    assert np.array_equal(got, exp)
    assert st["pieces"] == 1 and st["heavy"] == [None] and st["pair"] == [True], st


def test_launch_modes_do_not_leak_between_entries(inputs, oracle):
    """What a piece-wise call sets for its launches — the sort stream and its 512-thread sort form, two wavefronts per SIMD, resumed buckets, no
    reduction, the heavy count's address, the window size — holds for those launches alone: the resident entries that follow it on the same
    job (a plain G1 set with its side-stream conversion, the three-wave form and the one-launch sort at 4096 points; the two-pass sort at 2^19;
    a G2 set), the single-launch form of the entry itself and a second piece-wise call return what they returned before the first one."""
    import torch
    zkg = inputs.zkg
    n_small, n_g2, n_single = 4096, 2048, N - 256
    d_small, d_big = to_dev(inputs.uniform[:n_small]), to_dev(inputs.uniform[:N])
    d_k = to_dev(inputs.uniform[:n_g2])
    d_g2 = torch.empty((n_g2, 16), dtype=torch.int64, device="cuda")
    zkg.fixed_base_g2_dev(oracle.g2_generator(), d_k.data_ptr(), n_g2, d_g2.data_ptr())
    torch.cuda.synchronize()
    g2_bases = d_g2.cpu().numpy().view(np.uint64)
    sc_g2 = np.ascontiguousarray(inputs.uniform[n_g2:2 * n_g2])
    d_sc_g2 = to_dev(sc_g2)

    def entries():
        return [zkg.msm_g1_dev(inputs.d_bases.data_ptr(), d_small.data_ptr(), n_small),
                zkg.msm_g1_dev(inputs.d_bases.data_ptr(), d_big.data_ptr(), N),
                zkg.msm_g2_dev(d_g2.data_ptr(), d_sc_g2.data_ptr(), n_g2)]

    before = entries()
    before_single = inputs.expected(("uniform", n_single), inputs.d_bases, inputs.uniform, n_single)
    assert np.array_equal(before[1], inputs.expected(("uniform", N), inputs.d_bases, inputs.uniform, N))
    assert np.array_equal(before[0], oracle.msm_g1(inputs.bases[:n_small], inputs.uniform[:n_small], oracle.BDLO12, oracle.num_threads()))
    assert np.array_equal(before[1], inputs.oracle_uniform(oracle))
    assert np.array_equal(before[2], oracle.msm_g2(g2_bases, sc_g2, oracle.BDLO12, oracle.num_threads()))

    got, exp, st = inputs.run_uniform()                                                       # 1. piece-wise
    print("stats:", st)
    assert np.array_equal(got, before[1]) and np.array_equal(got, exp)
    _assert_uniform_stats(st)
    after = entries()                                                                         # 2. - 4.
    for k in range(3):
        assert np.array_equal(after[k], before[k]), k
    got, _, st = inputs.run_uniform(n_single)                                                 # 5. the entry's single launch
    print("stats:", st)
    assert np.array_equal(got, before_single)
    assert st["pieces"] == 1, st
    got, _, st = inputs.run_uniform()                                                         # 6. piece-wise again
    print("stats:", st)
    assert np.array_equal(got, before[1])
    _assert_uniform_stats(st)


def test_release_and_recreate_in_one_process():
    """zkg_shutdown releases everything the piece-wise step and the default job hold, and a later zkg_init starts from nothing: init, piece-wise
    call, shutdown, init, the same call, the resident call, shutdown — in a process of its own.  The three points are equal, the second
    piece-wise call ran four pieces without a cross-stream wait on the caller's stream, and the process ends cleanly."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import zklaim_amd as zkg
from bench import splitmix_fr
from gpu_util import dev_bases_g1
n = 1 << 19
zkg.init(0)
d_bases, _, _ = dev_bases_g1(zkg, n, 0x9AE0)
sc = splitmix_fr(n, 0x9AE1)
h_sc = torch.from_numpy(sc.view(np.int64)).pin_memory()
first = zkg.msm_g1_host_scalars(d_bases.data_ptr(), h_sc.data_ptr(), n)
zkg.shutdown()
zkg.init(0)
second = zkg.msm_g1_host_scalars(d_bases.data_ptr(), h_sc.data_ptr(), n)
st = zkg.msm_host_scalars_stats()
d_sc = h_sc.cuda()
third = zkg.msm_g1_dev(d_bases.data_ptr(), d_sc.data_ptr(), n)
zkg.shutdown()
print(json.dumps({"points": [p.tobytes().hex() for p in (first, second, third)], "stats": st}))
'''
    r = subprocess.run([sys.executable, "-c", code, root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    print("stats:", rec["stats"])
    assert rec["points"][0] == rec["points"][1] == rec["points"][2] and any(c != "0" for c in rec["points"][0])
    assert rec["stats"]["pieces"] == 4 and rec["stats"]["stream_waits"] == 0, rec["stats"]
