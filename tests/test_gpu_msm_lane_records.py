"""The lane records of the 29-bit accumulation (msm.hip: k_order_place writes one LaneRec {bucket, start, length | heavy flag, first entry}
per position of the bucket order, k_bucket_accum29 starts from it and from nothing else): lists whose lengths, signs and first bases are
chosen, not left to the inputs, on both sort forms and every launch kind that reaches the kernel.  Every comparison is bit for bit on the
normalised point, with the oracle or with an entry that the suite checks against the oracle on the same inputs.

A planted list is made of scalars with ONE chosen signed digit: d << (c w) puts an entry into bucket d - 1 of window w; 2^(c (w + 1)) -
(d << (c w)) puts a NEGATIVE entry there (and its carry, digit 1, into bucket 0 of window w + 1).  All other scalars are zero and give no
entry, so every list is exactly what was planted; `digits_of` mirrors the device's recoding (k_digits: raw = c bits + carry, above 2^(c-1)
it becomes 2^c - raw, negative, with a carry) for any window size and is checked against msm_piece_cases.signed_digits at c = 16; the
threshold is msm_piece_cases.heavy_threshold on the mirrored entry count.  Which entry of a list the sort puts first is not fixed (its
placement uses atomics), so a list that needs a property in its first entry has it in all of them.

The last bucket of the last window, whose old lane read offsets[total], is empty in every launch over canonical scalars (the top digit of
r is 3 at c = 12 and 0x3064 at c = 16): it is the last record of every order here.  The window-subset launch makes it non-empty: its last
owned window is an ordinary one."""
import numpy as np
import pytest

import msm_piece_cases as mc
from gpu_util import dev_bases_g1, to_dev, zkg  # noqa: F401
from util import R, arr, from_limbs, random_fr_canonical

pytestmark = pytest.mark.gpu

N = mc.N
SCALAR_BITS = 255


def geometry(n):
    """msm.hip, pick_geom: -> (c, windows, buckets per window)"""
    lg = n.bit_length() - 1
    c = 16 if lg >= 15 else 12 if lg >= 11 else max(lg + 1, 4)
    return c, (SCALAR_BITS + c - 1) // c, 1 << (c - 1)


def digits_of(value, c, windows):
    """the signed digits of one scalar as k_digits makes them"""
    out, carry = [], 0
    for w in range(windows):
        raw = ((value >> (c * w)) & ((1 << c) - 1)) + carry
        if raw > 1 << (c - 1):
            out.append(raw - (1 << c)); carry = 1
        else:
            out.append(raw); carry = 0
    assert not carry
    return out


class Planted:
    """n scalars, zero but for the planted lists: name -> (window, digit, count, negative); `where[name]` the indices of a list's scalars"""

    def __init__(self, n, lists):
        self.n = n
        self.c, self.windows, self.B = geometry(n)
        values, self.where = [], {}
        for name, (w, d, count, negative) in lists.items():
            assert 0 < d <= self.B and not (negative and d == self.B)
            v = ((1 << self.c) - d << (self.c * w)) if negative else d << (self.c * w)
            assert 0 < v < R, name
            self.where[name] = np.arange(len(values), len(values) + count)
            values += [v] * count
        assert len(values) <= n
        # scattered over the index range: a list's entries come from more than one slice of the sort
        self.perm = np.random.default_rng(n).permutation(n)[:len(values)]
        self.where = {k: self.perm[v] for k, v in self.where.items()}
        self.scalars = np.zeros((n, 4), np.uint64)
        self.scalars[self.perm] = arr(values)
        self.lengths = np.zeros((self.windows, self.B + 1), np.int64)
        self.negatives = np.zeros((self.windows, self.B + 1), np.int64)
        for v, cnt in zip(*np.unique(np.array(values, object), return_counts=True)):
            for w, d in enumerate(digits_of(int(v), self.c, self.windows)):
                if d:
                    self.lengths[w, abs(d)] += cnt
                    self.negatives[w, abs(d)] += cnt * (d < 0)
        self.entries = int(self.lengths.sum())
        self.threshold = mc.heavy_threshold(self.entries, self.windows * self.B)
        if self.c == 16:
            mirror = mc.signed_digits(self.scalars[self.perm])
            for w in range(16):
                assert np.array_equal(np.bincount(mirror[:, w], minlength=self.B + 1)[1:], self.lengths[w, 1:])

    def length(self, name, lists):
        w, d = lists[name][:2]
        return int(self.lengths[w, d])


def planted_lists(n, t):
    """the cases of one shape under threshold t"""
    c, windows, B = geometry(n)
    top = R >> (c * (windows - 1))                                         # the largest digit the top window can hold
    return {
        "bucket0_one": (0, 1, 1, False),                                   # bucket 0 of the whole launch, one entry: nothing to prefetch
        "one": (1, 700, 1, False), "two": (1, 701, 2, False), "three": (1, 702, 3, False),
        "one_neg": (3, 800, 1, True), "two_neg": (3, 801, 2, True), "three_neg": (3, 802, 3, True),   # carries: six entries in bucket 0 of window 4
        "one_inf": (6, 900, 1, False), "two_inf": (6, 901, 2, False), "three_inf": (6, 902, 3, False), "three_one_inf": (6, 903, 3, False),
        "last_of_window": (7, B, 2, False),                                # the last bucket of a window: the next window's first starts where it ends
        "top_window": (windows - 1, top, 3, False),                       # the last bucket of the last window that a canonical scalar reaches
        "at_threshold": (9, 1000, t, False), "above_threshold": (9, 1001, t + 1, False),
        "at_threshold_neg": (11, 1000, t, True), "above_threshold_neg": (11, 1001, t + 1, True),     # carries: 2 t + 1 in bucket 0 of window 12, heavy
    }


INF_LISTS = ("one_inf", "two_inf", "three_inf")


class _State:
    """bases and vectors, each made once and left unchanged"""

    def __init__(self, zkg, oracle):
        self.zkg, self.oracle = zkg, oracle
        self.d_bases, self.bases, _ = dev_bases_g1(zkg, N, 0x1A00)
        self._made = {}

    def once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    def oracle_msm(self, bases, sc):
        return self.oracle.msm_g1(bases, sc, self.oracle.BDLO12, self.oracle.num_threads())


@pytest.fixture(scope="module")
def state(zkg, oracle):
    return _State(zkg, oracle)


@pytest.mark.parametrize("n", [3000, 49152, 49156])
def test_planted_lists_on_both_sorts(state, n):
    """n = 3000: c = 12, the one-pass sort (k_place, k_class_hist); 49152 and 49156: c = 16, the smallest two-pass sort (k_rx_fine's class
    histogram), rows 16-byte aligned and not.  Over zero scalars the threshold is 8 (mirrored): lists of 8 stay on their lane, lists of 9
    carry the flag; 0, 1, 2 and 3 entries; all-negative lists; lists of bases at infinity; bucket 0; a window's last bucket."""
    t = 8
    lists = planted_lists(n, t)
    v = Planted(n, lists)
    assert v.threshold == t and v.c == (12 if n < 32768 else 16)
    for name, (w, d, count, negative) in lists.items():
        assert v.lengths[w, d] == count and v.negatives[w, d] == (count if negative else 0), name
    assert v.lengths[4, 1] == 6 and v.lengths[12, 1] == 2 * t + 1 and v.negatives[4, 1] == 0      # the carries' lists
    assert int((v.lengths > t).sum()) == 3 and int((v.lengths == t).sum()) == 2                     # the flag on both sides of the boundary
    assert v.lengths[v.windows - 1, v.B] == 0                                                      # the launch's last bucket: always empty
    assert {int(x) for x in np.unique(v.lengths)} >= {0, 1, 2, 3, t, t + 1}
    bases = state.bases[:n].copy()
    for name in INF_LISTS:
        bases[v.where[name]] = 0
    bases[v.where["three_one_inf"][:1]] = 0
    d_b = to_dev(bases)
    d_sc = to_dev(v.scalars)
    got = state.zkg.msm_g1_dev(d_b.data_ptr(), d_sc.data_ptr(), n)
    assert np.array_equal(got, state.oracle_msm(bases, v.scalars))
    assert np.array_equal(state.zkg.msm_g1_dev(d_b.data_ptr(), d_sc.data_ptr(), n), got)             # the same workspace again


@pytest.mark.parametrize("n", [3000, 49152, 49156])
def test_uniform_scalars_on_both_sorts(state, n):
    """lists as uniform scalars make them (lengths 0 ... ~10 around an average of 1.5), every record of the order in use"""
    sc = random_fr_canonical(n, 0x1A10 + n)
    d_sc = to_dev(sc)
    assert np.array_equal(state.zkg.msm_g1_dev(state.d_bases.data_ptr(), d_sc.data_ptr(), n), state.oracle_msm(state.bases[:n], sc))


def _sparse(n, nonzero, seed):
    sc = np.zeros((n, 4), np.uint64)
    sc[np.random.default_rng(seed).permutation(n)[:nonzero]] = random_fr_canonical(nonzero, seed + 1)
    return sc


@pytest.mark.parametrize("n, nonzero", [(5000, 5000), (5000, 37), (2999, 2999)])
def test_resident_table_launch(state, n, nonzero):
    """A launch over per-window tables covers one lane per possible entry at the most: fewer lanes than buckets, the records behind the
    last lane are written and never read — with every scalar set, and with 37 of them (nearly every lane's list is empty)."""
    sc = _sparse(n, nonzero, 0x1A20 + nonzero)
    d_sc = to_dev(sc)
    h = state.zkg.ResidentBases(state.d_bases.data_ptr(), n)
    try:
        got = h.msm(d_sc.data_ptr())
        again = h.msm(d_sc.data_ptr())
    finally:
        h.free()
    assert np.array_equal(got, state.oracle_msm(state.bases[:n], sc)) and np.array_equal(again, got)


@pytest.mark.parametrize("count", [2, 3])
def test_multi_launch(state, count):
    """two and three vectors over one table in one launch (rows per window and vector): a uniform vector, a sparse one, a zero one"""
    import torch
    n, stride = 5000, 5008
    vectors = [random_fr_canonical(n, 0x1A30), _sparse(n, 37, 0x1A31), np.zeros((n, 4), np.uint64)][:count]
    buf = np.full((count, stride, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    for i, v in enumerate(vectors):
        buf[i, :n] = v
    d_sc = to_dev(buf)
    d_out = torch.zeros((count, 12), dtype=torch.int64, device="cuda")
    h = state.zkg.ResidentBases(state.d_bases.data_ptr(), n)
    try:
        assert h.batch_max() >= count
        h.msm_async(d_sc.data_ptr(), d_out.data_ptr(), count=count, stride=stride)
        torch.cuda.synchronize()
    finally:
        h.free()
    got = d_out.cpu().numpy().view(np.uint64)
    for i, v in enumerate(vectors):
        assert np.array_equal(got[i], state.oracle_msm(state.bases[:n], v)), i


def test_window_subset_launch_fills_the_last_bucket(state):
    """msm_g1_windows_dev at 40000 points, every third window: the rank that starts at window 1 owns 1, 4, 7, 10, 13, and a digit of 2^15 in
    window 13 lands in the last bucket of its last row — the record whose list ends at offsets[total].  The three ranks' points add up to
    the whole multi-exponentiation, which is the oracle's."""
    n, ws = 40000, 3
    c, windows, B = geometry(n)
    assert (c, windows) == (16, 16)
    sc = random_fr_canonical(n, 0x1A40)
    sc[[5, 17000, 39999]] = arr([B << (c * 13)] * 3)
    assert [digits_of(from_limbs(sc[5]), c, windows)[w] for w in (12, 13, 14)] == [0, B, 0]
    d_sc = to_dev(sc)
    d_b = state.d_bases.data_ptr()
    parts = np.stack([state.zkg.msm_g1_windows_dev(d_b, d_sc.data_ptr(), n, g, ws) for g in range(ws)])
    full = state.oracle_msm(state.bases[:n], sc)
    assert np.array_equal(state.zkg.g1_sum(parts), full)
    assert np.array_equal(state.zkg.msm_g1_dev(d_b, d_sc.data_ptr(), n), full)


LANE_JOINS = ("lane_over_lane_cancelled", "lane_incoming_infinity", "lane_equals_lane", "lane_negates_lane_then_lane", "lane_infinity_base")


def test_piece_wise_resume_from_the_record(state):
    """n = 2^19, four pieces over one set of buckets: the lane joins of msm_piece_cases.JOINS alone in the vector (every other scalar zero, so
    no list is heavy: threshold 8, mirrored).  lane_equals_lane: empty in the third piece and resumed in the fourth, and in the second
    piece all three incoming entries equal the accumulator, so the first addition after the record takes the 32-bit fallback;
    lane_negates_lane_then_lane: the one incoming entry cancels the accumulator, and the next piece resumes an infinity;
    lane_incoming_infinity and lane_infinity_base: a piece whose list sums to nothing, and first entries that are bases at infinity."""
    import torch
    joins = state.once("joins", mc.build_joins)
    keep = [m for m in joins.members if m.name in LANE_JOINS]
    assert len(keep) == len(LANE_JOINS)
    sc = np.zeros((N, 4), np.uint64)
    for m in keep:
        sc[m.all_indices] = m.scalar
    profiles = mc.piece_profiles(sc)
    assert [p.threshold for p in profiles] == [8] * 4 and [p.heavy for p in profiles] == [0] * 4
    by_name = {m.name: m for m in keep}
    for m in keep:
        for k, p in enumerate(profiles):
            assert p.classes_of(m.digit) == {m.classes[k]}, (m.name, k)
    assert by_name["lane_equals_lane"].classes == ("L", "L", "E", "L") and by_name["lane_equals_lane"].recipes[1] == "eq"
    assert by_name["lane_negates_lane_then_lane"].recipes[:3] == ("fresh", "neg", "fresh")
    used = np.concatenate([m.all_indices for m in keep])
    plan = [op for op in joins.plan if np.isin(op[1], used).all()]          # the other joins' scalars are zero: their bases stay as they are
    assert {op[0] for op in plan} == {"neg", "sum", "inf"}
    bases = mc.apply_base_plan(state.oracle, state.bases.copy(), plan)
    d_b = to_dev(bases)
    h_sc = torch.from_numpy(sc.view(np.int64)).pin_memory()
    got = state.zkg.msm_g1_host_scalars(d_b.data_ptr(), h_sc.data_ptr(), N)
    st = state.zkg.msm_host_scalars_stats()
    assert st["pieces"] == 4 and st["heavy"] == [0] * 4 and st["pair"] == [False] * 4, st
    assert np.array_equal(got, state.oracle_msm(bases, sc))
    assert np.array_equal(state.zkg.msm_g1_host_scalars(d_b.data_ptr(), h_sc.data_ptr(), N), got)
