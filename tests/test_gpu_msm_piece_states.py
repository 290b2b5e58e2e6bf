"""What a bucket goes through from piece to piece in zkg_msm_g1_host_scalars (msm.hip, msm_g1_host_scalars), chosen instead of left to the
inputs: msm_piece_cases.py builds scalar vectors in which every bucket's list has a given class — empty, walked by one lane, heavy with one
part, heavy with several parts — in every piece, so that every sequence of classes over the four pieces occurs, and vectors in which every
kind of join of a piece's list with the earlier pieces' sum (the lane walk's resume, k_heavy_merge with one and with several parts, the first
piece's `single`) meets a sum at infinity, an incoming infinity, an equal and an opposite sum and a base at infinity.  Then the driver's forms
with other piece counts (ZKG_MSM_PIECES, ZKG_MSM_CUTS, in processes of their own) and the stream order of pinned scalars.  n = 2^19, the
smallest size that takes the piece-wise path.  Every comparison is bit for bit on the normalised point."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msm_piece_cases as mc
from bench import splitmix_fr
from gpu_util import dev_bases_g1, to_dev, zkg  # noqa: F401
from util import g1_jac_expected, random_fr_canonical

pytestmark = pytest.mark.gpu

N = mc.N
UNIFORM_COPIES = {"E": 0, "L": 3, "S": 200, "M": 2000}


class _State:
    """bases, vectors and reference points, each made once and left unchanged"""

    def __init__(self, zkg, oracle):
        self.zkg, self.oracle = zkg, oracle
        self.d_bases, self.bases, _ = dev_bases_g1(zkg, N + 256, 0x9B00)
        self._made = {}

    def once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    @property
    def seq(self):
        return self.once("seq", mc.build_sequences)

    @property
    def joins(self):
        return self.once("joins", mc.build_joins)

    @property
    def join_bases(self):
        """-> (host, device): the first 2^19 bases with the join vector's plan applied"""
        def make():
            import torch
            b = mc.apply_base_plan(self.oracle, self.bases[:N].copy(), self.joins.plan)
            return b, torch.from_numpy(b.view(np.int64)).cuda()
        return self.once("join_bases", make)

    def pinned(self, sc):
        import torch
        return torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).pin_memory()

    def host_scalars(self, d_bases, sc, n=N):
        h_sc = self.pinned(sc)
        got = self.zkg.msm_g1_host_scalars(d_bases.data_ptr(), h_sc.data_ptr(), n)
        return got, self.zkg.msm_host_scalars_stats()

    def resident(self, d_bases, sc, n=N):
        d_sc = to_dev(sc)
        return self.zkg.msm_g1_dev(d_bases.data_ptr(), d_sc.data_ptr(), n)

    def oracle_msm(self, bases, sc):
        return self.oracle.msm_g1(bases, sc, self.oracle.BDLO12, self.oracle.num_threads())

    def seq_points(self):
        """the 256-sequence vector's point by the piece-wise entry (with its stats), the resident entry and the oracle"""
        def make():
            got, st = self.host_scalars(self.d_bases, self.seq.scalars)
            return got, st, self.resident(self.d_bases, self.seq.scalars), self.oracle_msm(self.bases[:N], self.seq.scalars)
        return self.once("seq_points", make)

    def join_points(self):
        def make():
            b, d_b = self.join_bases
            got, st = self.host_scalars(d_b, self.joins.scalars)
            return got, st, self.resident(d_b, self.joins.scalars), self.oracle_msm(b, self.joins.scalars)
        return self.once("join_points", make)


@pytest.fixture(scope="module")
def state(zkg, oracle):
    return _State(zkg, oracle)


def _hex(p):
    return np.asarray(p, np.uint64).tobytes().hex()


def _assert_stats(st, heavy, pieces=4):
    assert st["pieces"] == pieces and st["stream_waits"] == 0, st
    assert st["heavy"] == list(heavy) and st["pair"] == [h > 0 for h in heavy], (st, heavy)


def test_every_sequence_of_list_classes_over_the_four_pieces(state):
    """All 4^4 sequences of classes in one vector over zero scalars: 64 x (3 + 40 + 600) copies in every piece, 658 432 entries over 2^19
    buckets, a threshold of 20 in every piece (mirrored, not assumed), so 128 sequences x 16 windows = 2048 heavy buckets per piece."""
    got, st, dev, ref = state.seq_points()
    print("point:", _hex(got)); print("stats:", st)
    assert np.array_equal(got, ref) and np.array_equal(dev, ref)
    assert state.seq.thresholds == [20] * 4 and state.seq.heavy == [2048] * 4
    _assert_stats(st, [2048] * 4)
    again, st2 = state.host_scalars(state.d_bases, state.seq.scalars)            # the same call twice in a row
    assert np.array_equal(again, got)
    _assert_stats(st2, [2048] * 4)


def test_every_join_at_its_exceptional_cases(state):
    got, st, dev, ref = state.join_points()
    print("point:", _hex(got)); print("stats:", st)
    assert np.array_equal(got, ref) and np.array_equal(dev, ref)
    _assert_stats(st, state.joins.heavy)
    assert np.array_equal(state.host_scalars(state.join_bases[1], state.joins.scalars)[0], got)


def test_every_join_on_its_own(state):
    """The sharper diagnostic: the multi-exponentiation restricted to one sequence's indices, every other scalar zero (alone in the vector the
    sequence keeps its classes: test_msm_piece_cases_host.py), equals the sequence's scalar times the oracle's own sum of its bases."""
    import torch
    zkg, oracle = state.zkg, state.oracle
    b, d_b = state.join_bases
    h_sc = torch.zeros((N, 4), dtype=torch.int64).pin_memory()
    view = h_sc.numpy().view(np.uint64)
    wrong = []
    for m in state.joins.members:
        idx = m.all_indices
        view[idx] = m.scalar
        got = zkg.msm_g1_host_scalars(d_b.data_ptr(), h_sc.data_ptr(), N)
        st = zkg.msm_host_scalars_stats()
        view[idx] = 0
        exp = oracle.g1_scalar_mul(mc.affine_sum(oracle, b[idx]), m.scalar)
        heavy = [16 if c in "SM" else 0 for c in m.classes]
        if not np.array_equal(got, exp) or st["heavy"] != heavy or st["stream_waits"] != 0:
            wrong.append((m.name, m.classes, m.recipes, st["heavy"]))
    assert not wrong, wrong


@pytest.mark.parametrize("empty", [(0,), (2,), (3,), (0, 1, 2, 3)], ids=["first", "third", "last", "all"])
def test_pieces_without_a_single_entry(state, empty):
    """all-zero scalars in a whole piece: its sort has no entry, its accumulation nothing to add (the first piece's still writes every bucket's
    infinity), and the last piece still carries the reduction"""
    vec = state.once(("empty", empty), lambda: mc.build_sequences(empty_pieces=empty))
    got, st = state.host_scalars(state.d_bases, vec.scalars)
    print("stats:", st)
    assert np.array_equal(got, state.resident(state.d_bases, vec.scalars))
    if len(empty) == 4:
        assert np.array_equal(got, g1_jac_expected(None))
    else:
        assert not np.array_equal(got, g1_jac_expected(None))
    assert vec.heavy == [0 if k in empty else 2048 for k in range(4)]
    _assert_stats(st, vec.heavy)


def test_sequences_of_classes_over_a_uniform_background(state):
    """Uniform scalars everywhere but at the sequences' copies, 200 copies for a one-part and 2000 for a several-part list.  All 256 sequences at
    3 + 200 + 2000 copies do not fit a piece of 65 536 points (64 x 2203 = 140 992), so the vector holds 64 of them: every triple of classes
    in the first three pieces, the fourth class chosen so that every ordered pair of classes occurs at every join (COVERING_SEQUENCES).
    The bound, exact for this seed from the mirrored digits and thresholds (the builder asserts it, test_msm_piece_cases_host.py states
    it): thresholds 26, 26, 46 and 63 in the four pieces; the longest list of the background alone 10, 13, 19 and 36; a sequence's bucket
    holds its copies plus at most 31 background entries — 3 ... 31 for a lane's list, 200 ... 226 for one part (above 63, below 512),
    2000 ... 2024 for several — so no random entry moves a list across a class boundary, and 32 sequences x 16 windows = 512 buckets are
    heavy in every piece."""
    vec = state.once("uniform", lambda: mc.build_sequences(copies=UNIFORM_COPIES, sequences=mc.COVERING_SEQUENCES, background=splitmix_fr(N, 0x9B01)))
    assert vec.thresholds == [26, 26, 46, 63] and vec.heavy == [512] * 4
    got, st = state.host_scalars(state.d_bases, vec.scalars)
    print("stats:", st)
    assert np.array_equal(got, state.resident(state.d_bases, vec.scalars))
    assert np.array_equal(got, state.oracle_msm(state.bases[:N], vec.scalars))
    _assert_stats(st, [512] * 4)


def _forty_copies(n, sequences, seed):
    """zero scalars but `sequences` random ones, 40 copies each at scattered indices: every window in which such a scalar has a digit gets a
    list of 40 (80 where two of them share the digit)"""
    sc = np.zeros((n, 4), np.uint64)
    where = np.random.default_rng(seed).permutation(n)[:40 * sequences].reshape(sequences, 40)
    for s, v in zip(where, random_fr_canonical(sequences, seed + 1)):
        sc[s] = v
    return sc


@pytest.mark.parametrize("entry, n", [("g2", 4096), ("table", 4096), ("table", 33000), ("g1", 4096)])
def test_one_part_heavy_lists_on_the_other_accumulation_kernels(state, entry, n):
    """Lists of 40 over zero scalars are heavy with one part on the kernels the piece-wise step does not use — k_bucket_accum<Fq2, true>
    (zkg_msm_g2_dev), k_bucket_accum29 on a resident table (a launch over per-window levels, at two table sizes) and the three-wavefront
    form of the plain G1 launch: the part's `single` flag lets k_heavy_parts write the bucket itself.  Four scalars x 40 copies x at most 22
    windows are at most 3520 entries; over the 2048 buckets of even one window of the smallest geometry here (c = 12) the threshold is at
    most 24 (6 + 18), a third of it for G2 — below 40, and 80 stays below HEAVY_S.  (No entry point reaches the gathered 32-bit form without
    a prover's key; it is left out.)"""
    import torch
    zkg, oracle = state.zkg, state.oracle
    assert mc.heavy_threshold(4 * 40 * 22, 2048) == 24 < 40 and 2 * 40 <= mc.HEAVY_S
    sc = _forty_copies(n, 4, 0x9B20 + n)
    d_sc = to_dev(sc)
    if entry == "g2":
        d_k = to_dev(random_fr_canonical(n, 0x9B22))
        d_g2 = torch.empty((n, 16), dtype=torch.int64, device="cuda")
        zkg.fixed_base_g2_dev(oracle.g2_generator(), d_k.data_ptr(), n, d_g2.data_ptr())
        torch.cuda.synchronize()
        got = zkg.msm_g2_dev(d_g2.data_ptr(), d_sc.data_ptr(), n)
        exp = oracle.msm_g2(d_g2.cpu().numpy().view(np.uint64), sc, oracle.BDLO12, oracle.num_threads())
    elif entry == "table":
        h = zkg.ResidentBases(state.d_bases.data_ptr(), n)
        try:
            got = h.msm(d_sc.data_ptr())
        finally:
            h.free()
        exp = state.oracle_msm(state.bases[:n], sc)
    else:
        got = zkg.msm_g1_dev(state.d_bases.data_ptr(), d_sc.data_ptr(), n)
        exp = state.oracle_msm(state.bases[:n], sc)
    assert np.array_equal(got, exp)


_OTHER_PIECES = r'''
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import zklaim_amd as zkg
zkg.init(0)
out = {}
for name in ("seq", "joins"):
    d_bases = torch.from_numpy(np.load(sys.argv[2] + "/" + name + "_bases.npy").view(np.int64)).cuda()
    h_sc = torch.from_numpy(np.load(sys.argv[2] + "/" + name + "_scalars.npy").view(np.int64)).pin_memory()
    n = h_sc.shape[0]
    first = zkg.msm_g1_host_scalars(d_bases.data_ptr(), h_sc.data_ptr(), n)
    second = zkg.msm_g1_host_scalars(d_bases.data_ptr(), h_sc.data_ptr(), n)
    out[name] = {"points": [first.tobytes().hex(), second.tobytes().hex()], "stats": zkg.msm_host_scalars_stats()}
zkg.shutdown()
print(json.dumps(out))
'''


@pytest.fixture(scope="module")
def vector_files(state, tmp_path_factory):
    d = tmp_path_factory.mktemp("piece_vectors")
    np.save(d / "seq_bases.npy", state.bases[:N]); np.save(d / "seq_scalars.npy", state.seq.scalars)
    np.save(d / "joins_bases.npy", state.join_bases[0]); np.save(d / "joins_scalars.npy", state.joins.scalars)
    return str(d)


def _halvings(pieces):
    """host_scalars_cuts: halves from the top"""
    return [0] + [N >> k for k in range(pieces - 1, -1, -1)]


@pytest.mark.parametrize("env, cuts", [({"ZKG_MSM_PIECES": "3"}, _halvings(3)), ({"ZKG_MSM_PIECES": "5"}, _halvings(5)), ({"ZKG_MSM_PIECES": "8"}, _halvings(8)),
                                       ({"ZKG_MSM_PIECES": "1"}, [0, N]), ({"ZKG_MSM_CUTS": "8,8,32"}, [0, N // 8, N // 2, N])],
                         ids=["three", "five", "eight", "one", "empty_middle_cut"])
def test_other_piece_counts_give_the_same_points(state, vector_files, env, cuts):
    """The driver's forms that four pieces never take, in a process of their own (the switches are read once): an odd count of pieces over the
    two sort workspaces (which = (R - 1 - i) & 1 with R = 3 and 5), eight pieces of 4096 points and more, one piece (the single launch), and
    cuts at n/8, n/8, n/2 — a zero-length second piece that the run[] list skips, three pieces run.  The lists' classes change with the
    cuts — the heavy counts the host reads are the mirror's for these cuts; the two points do not."""
    pieces = len(cuts) - 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _OTHER_PIECES, root, vector_files], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    print("stats:", {k: v["stats"] for k, v in rec.items()})
    for name, vec, ours in (("seq", state.seq, state.seq_points()[0]), ("joins", state.joins, state.join_points()[0])):
        assert rec[name]["points"] == [_hex(ours)] * 2, name
        st = rec[name]["stats"]
        assert st["pieces"] == pieces, st
        if pieces > 1:
            heavy = [p.heavy for p in mc.piece_profiles(vec.scalars, list(zip(cuts[:-1], cuts[1:])))]
            assert any(heavy) and st["stream_waits"] == 0 and st["heavy"] == heavy and st["pair"] == [h > 0 for h in heavy], (st, heavy)
        else:
            assert st["heavy"] == [None] and st["pair"] == [True], st


@pytest.mark.parametrize("n", [N + 256, N - 256], ids=["piece_wise", "single_launch"])
def test_pinned_scalars_written_by_work_queued_on_the_stream(state, n):
    """zkg.h: pinned scalars may be produced by work queued on `stream` before the call — on both sides of the piece-wise threshold.  The pinned
    buffer starts as zeros; ~1 GB of traffic and then the copy that fills it are queued on a side stream, and the call names that stream.
    The piece-wise path uploads on a stream of its own, which has to be ordered behind the caller's (without a wait on the caller's: the
    stats say so); the single launch uploads on the caller's stream itself.  Four fresh side streams in turn: streams share a few hardware
    queues, and a caller's stream that happens to share the copy stream's is ordered by that accident — without the order the first side stream
    of a process got the right point and the next five the point at infinity, the sum over the zeros the buffer still held."""
    import torch
    zkg = state.zkg
    sc = splitmix_fr(n, 0x9B30 + (n & 1023))
    d_sc = to_dev(sc)
    exp = zkg.msm_g1_dev(state.d_bases.data_ptr(), d_sc.data_ptr(), n)
    # a first call at this size from memory that is ready: the step's streams, events and buffers exist afterwards, so the call below starts its
    # uploads at once and not after the milliseconds their creation takes (which would hide a missing order when this test runs alone)
    assert np.array_equal(state.host_scalars(state.d_bases, sc, n)[0], exp)
    junk = torch.empty(32 << 20, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for k in range(4):
        h_sc = torch.zeros((n, 4), dtype=torch.int64).pin_memory()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(4):
                junk.add_(1)                                           # ~1 GB of traffic queued ahead of the copy
            h_sc.copy_(d_sc, non_blocking=True)
        got = zkg.msm_g1_host_scalars(state.d_bases.data_ptr(), h_sc.data_ptr(), n, stream=side.cuda_stream)
        st = zkg.msm_host_scalars_stats()
        side.synchronize()
        print("point:", _hex(got)); print("stats:", st)
        assert np.array_equal(h_sc.numpy().view(np.uint64), sc)
        assert np.array_equal(got, exp), k
    assert st["pieces"] == (4 if n >= N else 1), st
    if n >= N:
        assert st["stream_waits"] == 0, st
