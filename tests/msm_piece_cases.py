"""Scalar vectors that choose what every bucket of the piece-wise multi-exponentiation (msm.hip, msm_g1_host_scalars) goes through from piece
to piece.  n = 2^19 is the smallest size that takes the piece-wise path: c = 16, 16 windows of 2^15 buckets, pieces [0, 65536),
[65536, 131072), [131072, 262144), [262144, 524288).  In each piece a bucket's list is empty (E), walked by one lane (L: at most the piece's
heavy threshold), heavy with one part (S: above the threshold, at most HEAVY_S = 512 entries) or heavy with several parts (M).

A "sequence" is one scalar whose sixteen 16-bit digits are all d: no digit has its top bit set, so no signed-digit carry occurs, the top digit
is below r's own 0x3064, so the scalar is below r, and every copy lands in bucket d - 1 of all 16 windows.  The number of copies inside a
piece's index range gives the bucket its class there.  Pure numpy: the mirror of the device's threshold (heavy_threshold) and of its signed
digits (signed_digits) give every list's exact length, whatever the background, and the builders assert the classes against them."""
import itertools

import numpy as np

N = 1 << 19
PIECES = ((0, 65536), (65536, 131072), (131072, 262144), (262144, 524288))
WINDOWS, WINDOW_BUCKETS = 16, 1 << 15
TOTAL_BUCKETS = WINDOWS * WINDOW_BUCKETS
HEAVY_T_MAX, HEAVY_S = 1024, 512
COPIES = {"E": 0, "L": 3, "S": 40, "M": 600}
R_TOP_DIGIT = 0x3064                      # r >> 240


def heavy_threshold(entries, total_buckets, divisor=1):
    """msm.hip, heavy_threshold_dev: four times the average list length plus a slack of 8 + 6 x the average, at most 32; at most
    HEAVY_T_MAX; divided by `divisor` (3 for G2); at least 4.  A list is heavy when it is LONGER than this."""
    avg6 = 6 * entries // total_buckets
    slack = 32 if 8 + avg6 > 32 else 8 + avg6
    t = 4 * entries // total_buckets + slack
    t = min(t, HEAVY_T_MAX) // divisor
    return max(t, 4)


def list_class(length, threshold):
    return "E" if length == 0 else "L" if length <= threshold else "S" if length <= HEAVY_S else "M"


def sequence_scalar(j):
    d = 0x0100 + j
    assert 0 < d < R_TOP_DIGIT and not d & 0x8000
    return np.array([d * 0x0001000100010001] * 4, np.uint64)


def signed_digits(sc):
    """|digit| of the 16 windows of canonical scalars at c = 16 as k_digits_c<16> makes them (0: no entry; otherwise the entry goes to
    bucket |digit| - 1): raw = 16 bits + carry, above 2^15 it becomes 2^16 - raw with a carry into the next window."""
    sc = np.ascontiguousarray(sc, np.uint64)
    raw16 = sc.view("<u2").reshape(len(sc), 16).astype(np.int64)
    out = np.empty_like(raw16)
    carry = np.zeros(len(sc), np.int64)
    for w in range(16):
        raw = raw16[:, w] + carry
        neg = raw > 0x8000
        out[:, w] = np.where(neg, 0x10000 - raw, raw)
        carry = neg.astype(np.int64)
    assert not carry.any(), "a scalar of 2^256 or more"
    return out


class PieceProfile:
    """entries, threshold and every list's length — lengths[w, d] for digit d of window w — of one piece"""

    def __init__(self, digits):
        self.entries = int(np.count_nonzero(digits))
        self.threshold = heavy_threshold(self.entries, TOTAL_BUCKETS)
        self.lengths = np.stack([np.bincount(digits[:, w], minlength=WINDOW_BUCKETS + 1) for w in range(WINDOWS)])
        self.lengths[:, 0] = 0
        self.heavy = int((self.lengths > self.threshold).sum())

    def classes_of(self, d):
        """the classes of digit d's bucket in the 16 windows, as a set"""
        return {list_class(int(v), self.threshold) for v in self.lengths[:, d]}


def piece_profiles(scalars, pieces=PIECES):
    digits = signed_digits(scalars)
    return [PieceProfile(digits[lo:hi]) for lo, hi in pieces]


class Member:
    """one sequence: its digit and scalar, its class in every piece and the indices of its copies there"""

    def __init__(self, name, j, classes):
        self.name, self.j, self.digit, self.scalar, self.classes = name, j, 0x0100 + j, sequence_scalar(j), tuple(classes)
        self.indices = [np.zeros(0, np.int64) for _ in PIECES]

    @property
    def all_indices(self):
        return np.concatenate(self.indices)


class PieceVector:
    def __init__(self, scalars, members, plan=(), noisy=False):
        self.scalars, self.members, self.plan = np.ascontiguousarray(scalars), members, list(plan)
        self.profiles = piece_profiles(self.scalars)
        self.heavy = [p.heavy for p in self.profiles]
        self.thresholds = [p.threshold for p in self.profiles]
        # every bucket of the sequence, in all 16 windows, has the class it was given (over a background that is not zero a bucket without a
        # copy holds what the background gives it: nothing, or a lane's walk)
        for m in members:
            for k, prof in enumerate(self.profiles):
                allowed = {"E", "L"} if noisy and m.classes[k] == "E" else {m.classes[k]}
                assert prof.classes_of(m.digit) <= allowed, (m.name, k, prof.classes_of(m.digit), m.classes[k], prof.threshold)


def _place(members_counts, background):
    """copies of every member back to back from the start of each piece: -> scalars; members' indices filled in"""
    scalars = np.zeros((N, 4), np.uint64) if background is None else np.array(background[:N], np.uint64)
    cursor = [lo for lo, _ in PIECES]
    for m, counts in members_counts:
        for k, cnt in enumerate(counts):
            assert cursor[k] + cnt <= PIECES[k][1], "the piece has no room for its copies"
            m.indices[k] = np.arange(cursor[k], cursor[k] + cnt, dtype=np.int64)
            scalars[m.indices[k]] = m.scalar
            cursor[k] += cnt
    return scalars


ALL_SEQUENCES = tuple(itertools.product("ELSM", repeat=4))
# 64 of them: every triple of classes in the first three pieces, the last piece's class chosen so that every ordered pair of classes occurs at
# every one of the three joins and every class 16 times in every piece
COVERING_SEQUENCES = tuple(s for s in ALL_SEQUENCES if "ELSM".index(s[3]) == sum("ELSM".index(c) for c in s[:3]) % 4)


def build_sequences(copies=COPIES, sequences=ALL_SEQUENCES, background=None, empty_pieces=()):
    """Sequence j (digit 0x0100 + j) has class sequences[j][k] in piece k: copies[class] copies of its scalar there.  background: the other
    scalars (None: zero, which gives no entry, so that every list is exactly what is put there).  empty_pieces: pieces whose scalars are all
    zeroed afterwards (their classes become E)."""
    members = [Member("".join(s), j, s) for j, s in enumerate(sequences)]
    scalars = _place([(m, [copies[c] for c in m.classes]) for m in members], background)
    for k in empty_pieces:
        scalars[PIECES[k][0]:PIECES[k][1]] = 0
        for m in members:
            m.classes = m.classes[:k] + ("E",) + m.classes[k + 1:]
            m.indices[k] = np.zeros(0, np.int64)
    return PieceVector(scalars, members, noisy=background is not None)


# ---- the joins ------------------------------------------------------------------------------------------------------------------------------
# A join is where a piece's list meets the sum of the earlier pieces: the lane walk (k_bucket_accum29's resume: load_bucket29_raw, then madd),
# k_heavy_merge with one part (a lone part of a later piece: `single` is forced off) and with several parts (thread 255 adds the old bucket),
# and the first piece's `single` (k_heavy_parts writes the bucket itself).  The record a later piece resumes from was written by the lane
# walk (store_bucket29: lazy digits) or by put_bucket (from a canonical XYZZ), the infinity form by either.  Per piece: (class, recipe).
#   fresh     distinct bases, as they come
#   pairs     P, -P, Q, -Q, ...: the piece's sum is infinity (and additions cancel on the way)
#   eq        the piece's sum equals the old sum T: for L three entries that ARE T (the first incoming entry equals the accumulator whatever the
#             order of the list: the madd fallback under resume); for S and M the entry T and pairs
#   neg       the piece's sum is -T: for L the one entry -T; for S and M the entry -T and pairs.  The bucket is infinity afterwards.
#   dup       the bases of the sequence's last non-empty piece again (equal sums through duplicated bases)
#   inf       fresh, two of them replaced by the point at infinity
JOIN_COUNTS = {("L", "fresh"): 3, ("L", "pairs"): 4, ("L", "eq"): 3, ("L", "neg"): 1, ("L", "inf"): 3,
               ("S", "fresh"): 40, ("S", "pairs"): 40, ("S", "eq"): 41, ("S", "neg"): 41, ("S", "dup"): 40, ("S", "inf"): 40,
               ("M", "fresh"): 600, ("M", "pairs"): 600, ("M", "eq"): 601, ("M", "neg"): 601, ("M", "dup"): 600, ("M", "inf"): 600}
_ = None
JOINS = (
    # lane resume (incoming L) ...
    ("lane_over_lane_cancelled", [("L", "pairs"), ("L", "fresh"), _, _]),                 # ... of an infinity the lane walk stored
    ("lane_over_single_cancelled", [("S", "pairs"), ("L", "fresh"), _, _]),               # ... of an infinity the first piece's single stored
    ("lane_over_merge_cancelled", [("M", "pairs"), _, ("L", "fresh"), _]),                # ... of an infinity k_heavy_merge stored
    ("lane_incoming_infinity", [("L", "fresh"), ("L", "pairs"), ("L", "fresh"), _]),
    ("lane_equals_lane", [("L", "fresh"), ("L", "eq"), _, ("L", "fresh")]),               # accumulator in lazy digits
    ("lane_equals_single", [("S", "fresh"), ("L", "eq"), _, ("L", "fresh")]),             # accumulator from put_bucket
    ("lane_equals_merge", [("M", "fresh"), ("L", "eq"), ("L", "fresh"), _]),
    ("lane_negates_lane_then_lane", [("L", "fresh"), ("L", "neg"), ("L", "fresh"), _]),
    ("lane_negates_single_then_single", [("S", "fresh"), ("L", "neg"), _, ("S", "fresh")]),
    ("lane_negates_lane_then_merge", [_, ("L", "fresh"), ("L", "neg"), ("M", "fresh")]),
    ("lane_infinity_base", [("L", "fresh"), ("L", "inf"), _, _]),
    # k_heavy_merge with one part (incoming S in a later piece)
    ("one_part_over_lane_cancelled", [("L", "pairs"), ("S", "fresh"), _, _]),
    ("one_part_over_single_cancelled", [("S", "pairs"), _, ("S", "fresh"), _]),
    ("one_part_incoming_infinity", [("L", "fresh"), ("S", "pairs"), ("L", "fresh"), _]),
    ("one_part_equals_lane", [("L", "fresh"), ("S", "eq"), _, ("L", "fresh")]),
    ("one_part_duplicates_single", [("S", "fresh"), ("S", "dup"), _, _]),
    ("one_part_negates_lane_then_lane", [("L", "fresh"), ("S", "neg"), ("L", "fresh"), _]),
    ("one_part_negates_merge_then_one_part", [("M", "fresh"), ("S", "neg"), ("S", "fresh"), _]),
    ("one_part_infinity_base", [("L", "fresh"), _, _, ("S", "inf")]),
    # k_heavy_merge with several parts (incoming M)
    ("parts_over_lane_cancelled", [("L", "pairs"), ("M", "fresh"), _, _]),
    ("parts_over_merge_cancelled", [("M", "pairs"), ("M", "fresh"), _, _]),
    ("parts_incoming_infinity", [("L", "fresh"), ("M", "pairs"), _, ("L", "fresh")]),
    ("parts_duplicate_merge", [("M", "fresh"), _, ("M", "dup"), _]),
    ("parts_equal_single", [("S", "fresh"), ("M", "eq"), _, _]),
    ("parts_negate_lane_then_parts", [("L", "fresh"), ("M", "neg"), ("M", "fresh"), _]),
    ("parts_negate_single_then_lane", [("S", "fresh"), _, ("M", "neg"), ("L", "fresh")]),
    ("parts_infinity_base", [("L", "fresh"), ("M", "inf"), _, _]),
    # the first piece's single
    ("single_cancelled_then_one_part", [("S", "pairs"), _, _, ("S", "fresh")]),
    ("single_infinity_base_then_lane", [("S", "inf"), ("L", "fresh"), _, _]),
    ("single_then_nothing_then_lane", [("S", "fresh"), _, _, ("L", "fresh")]),
    ("first_parts_infinity_base_then_lane", [("M", "inf"), ("L", "fresh"), _, _]),
)


def build_joins():
    """-> PieceVector whose `plan` makes the bases: ("neg", dst, src), ("dup", dst, src), ("inf", dst) and ("sum", dst, srcs, sign) — the bases
    at dst become sign x the sum of the bases at srcs — over index arrays, to be applied in order (apply_base_plan)."""
    members, counts, recipes = [], [], []
    for j, (name, spec) in enumerate(JOINS):
        members.append(Member(name, j, [s[0] if s else "E" for s in spec]))
        counts.append([JOIN_COUNTS[s] if s else 0 for s in spec])
        recipes.append([s[1] if s else None for s in spec])
    scalars = _place(list(zip(members, counts)), None)
    plan = []
    for m, rec in zip(members, recipes):
        m.recipes = tuple(rec)
        for k, recipe in enumerate(rec):
            idx = m.indices[k]
            earlier = [m.indices[q] for q in range(k) if len(m.indices[q])]
            old = np.concatenate(earlier) if earlier else np.zeros(0, np.int64)

            def pairs(ix):
                assert len(ix) % 2 == 0
                plan.append(("neg", ix[len(ix) // 2:], ix[:len(ix) // 2]))
            if recipe == "pairs":
                pairs(idx)
            elif recipe in ("eq", "neg"):
                assert len(old)
                own = idx if m.classes[k] == "L" else idx[:1]
                plan.append(("sum", own, old, 1 if recipe == "eq" else -1))
                if m.classes[k] != "L":
                    pairs(idx[1:])
            elif recipe == "dup":
                assert len(earlier[-1]) == len(idx)
                plan.append(("dup", idx, earlier[-1]))
            elif recipe == "inf":
                plan.append(("inf", idx[[1, len(idx) - 1]]))
    return PieceVector(scalars, members, plan)


def running_sum_is_infinity(m):
    """for a member of build_joins: per piece, whether its bucket is at infinity after that piece (None where nothing has landed yet)"""
    out, state = [], None
    for recipe in m.recipes:
        if recipe in ("fresh", "inf", "dup", "eq"):
            state = False
        elif recipe == "pairs":
            state = True if state is None else state
        elif recipe == "neg":
            state = True
        out.append(state)
    return out


def affine_sum(oracle, bases):
    """the oracle's sum of affine G1 points (n, 8) -> 8 affine limbs (all-zero: infinity)"""
    from util import Q, arr
    bases = np.asarray(bases, np.uint64).reshape(-1, 8)
    jac = np.zeros((len(bases), 12), np.uint64)
    jac[:, :8] = bases
    finite = bases.any(axis=1)
    jac[finite, 8:] = arr([1], Q).reshape(4)
    jac[~finite, 4:8] = arr([1], Q).reshape(4)                    # (0, 1, 0)
    s = oracle.g1_sum(jac)
    return s[:8].copy() if s[8:].any() else np.zeros(8, np.uint64)


def apply_base_plan(oracle, bases, plan):
    from gpu_util import neg_affine
    for op in plan:
        if op[0] == "neg":
            for d, s in zip(op[1], op[2]):
                bases[d] = neg_affine(bases[s])
        elif op[0] == "dup":
            bases[op[1]] = bases[op[2]]
        elif op[0] == "inf":
            bases[op[1]] = 0
        elif op[0] == "sum":
            t = affine_sum(oracle, bases[op[2]])
            bases[op[1]] = t if op[3] > 0 else neg_affine(t)
        else:
            raise ValueError(op[0])
    return bases
