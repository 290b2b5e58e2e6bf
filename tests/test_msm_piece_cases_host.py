"""The vectors of msm_piece_cases.py do what they say (no GPU): every scalar is canonical and carry-free, every piece holds the copies it should,
every bucket has its class under the mirrored threshold, the heavy counts follow — and the mirror of heavy_threshold_dev itself gives the
values worked out by hand from msm.hip's formula."""
import numpy as np
import pytest

import msm_piece_cases as mc
from util import R, from_limbs


@pytest.mark.parametrize("entries, total, divisor, expected", [
    # t = min(4 e / total + min(32, 8 + 6 e / total), 1024) / divisor, at least 4 (integer divisions)
    (0, 1 << 19, 1, 8),                      # no entry: the slack's own 8
    (0, 1 << 19, 3, 4),                      # 8 / 3 = 2: the `min 4` clamp (G2)
    (1, 45056, 3, 4),
    (658432, 1 << 19, 1, 20),                # the 256-sequence vector's pieces: 4 e / total = 5, 6 e / total = 7, slack 15
    ((1 << 19) - 1, 1 << 19, 1, 16),         # just below an average of one: 3 + (8 + 5)
    (1 << 19, 1 << 19, 1, 18),               # an average of one: 4 + (8 + 6)
    (2 << 19, 1 << 19, 1, 28),               # two: 8 + (8 + 12)
    (4 << 19, 1 << 19, 1, 48),               # four: 16 + 32, the slack's clamp reached exactly (8 + 24)
    (8 << 19, 1 << 19, 1, 64),               # eight: 32 + 32, the slack clamped (8 + 48 > 32)
    (8 << 19, 1 << 19, 3, 21),
    (248 << 19, 1 << 19, 1, 1024),           # 992 + 32: HEAVY_T_MAX reached exactly
    (300 << 19, 1 << 19, 1, 1024),           # 1200 + 32: clamped
    (300 << 19, 1 << 19, 3, 341),            # the clamp comes before the division
    (0xFFFFFFFF, 1 << 19, 1, 1024),          # the largest entry count a 32-bit offset holds: the device's 64-bit products do not wrap
])
def test_threshold_mirror_against_hand_computed_values(entries, total, divisor, expected):
    assert mc.heavy_threshold(entries, total, divisor) == expected
    assert (mc.HEAVY_T_MAX, mc.HEAVY_S) == (1024, 512)


def test_signed_digits_mirror():
    sc = np.zeros((5, 4), np.uint64)
    sc[1, 0] = 0x8000                        # exactly 2^15: stays positive (raw > B is the test)
    sc[2, 0] = 0x8001                        # 2^16 - 0x8001 = 0x7FFF, carry into window 1
    sc[3, 0] = 0xFFFF                        # digit 1 (negative), carry
    sc[4, 0] = 0xFFFF_FFFF                   # window 0: 1 with a carry; window 1: 0xFFFF + 1 = 2^16 -> digit 0, no entry, carry; window 2: 1
    d = mc.signed_digits(sc)
    assert d[0].tolist() == [0] * 16
    assert d[1].tolist() == [0x8000] + [0] * 15
    assert d[2].tolist() == [0x7FFF, 1] + [0] * 14
    assert d[3].tolist() == [1, 1] + [0] * 14
    assert d[4].tolist() == [1, 0, 1] + [0] * 13


def _check_scalars(vec):
    """every scalar below r; the members' scalars carry-free with sixteen equal digits, and exactly at their indices"""
    from util import R_LIMBS
    lt = np.zeros(mc.N, bool); eq = np.ones(mc.N, bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (vec.scalars[:, i] < R_LIMBS[i]); eq &= vec.scalars[:, i] == R_LIMBS[i]
    assert lt.all() and R >> 240 == mc.R_TOP_DIGIT
    owned = np.zeros(mc.N, bool)
    for m in vec.members:
        assert from_limbs(m.scalar) < R
        raw = m.scalar.view("<u2")
        assert (raw == m.digit).all() and m.digit < 0x8000                       # no top bit: no carry
        assert (mc.signed_digits(m.scalar.reshape(1, 4)) == m.digit).all()
        for k, (lo, hi) in enumerate(mc.PIECES):
            idx = m.indices[k]
            assert ((idx >= lo) & (idx < hi)).all() and not owned[idx].any()
            owned[idx] = True
            assert (vec.scalars[idx] == m.scalar).all()
    return owned


def test_sequence_vector_invariants():
    vec = mc.build_sequences()
    assert len(vec.members) == 256 and len({m.classes for m in vec.members}) == 256 and len({m.digit for m in vec.members}) == 256
    owned = _check_scalars(vec)
    assert not vec.scalars[~owned].any()                                        # the background is zero: no entry
    for k, (lo, hi) in enumerate(mc.PIECES):
        for c in "ELSM":
            assert sum(m.classes[k] == c for m in vec.members) == 64
        for m in vec.members:
            assert len(m.indices[k]) == mc.COPIES[m.classes[k]]
        assert int(owned[lo:hi].sum()) == 64 * 643 == 41152
        prof = vec.profiles[k]
        assert prof.entries == 16 * 41152 == 658432 and prof.threshold == 20
        assert mc.COPIES["L"] <= prof.threshold < mc.COPIES["S"] <= mc.HEAVY_S < mc.COPIES["M"]
        for m in vec.members:
            assert prof.classes_of(m.digit) == {m.classes[k]}
    assert vec.heavy == [128 * 16] * 4 == [2048] * 4


@pytest.mark.parametrize("empty", [(0,), (2,), (3,), (0, 1, 2, 3)])
def test_vectors_with_pieces_without_entries(empty):
    vec = mc.build_sequences(empty_pieces=empty)
    for k, (lo, hi) in enumerate(mc.PIECES):
        if k in empty:
            assert not vec.scalars[lo:hi].any() and vec.profiles[k].entries == 0 and vec.heavy[k] == 0 and vec.thresholds[k] == 8
        else:
            assert vec.heavy[k] == 2048 and vec.thresholds[k] == 20


def test_sequences_over_a_uniform_background_keep_their_classes():
    from bench import splitmix_fr
    vec = mc.build_sequences(copies={"E": 0, "L": 3, "S": 200, "M": 2000}, sequences=mc.COVERING_SEQUENCES, background=splitmix_fr(mc.N, 0x9B01))
    assert len(vec.members) == 64
    _check_scalars(vec)
    for a in range(3):                                                          # every ordered pair of classes at every join
        assert {(m.classes[a], m.classes[a + 1]) for m in vec.members} == {(x, y) for x in "ELSM" for y in "ELSM"}
    for k, prof in enumerate(vec.profiles):
        others = prof.lengths.copy()
        others[:, [m.digit for m in vec.members]] = 0
        assert others.max() <= prof.threshold                                   # no list of the background is heavy
        assert vec.heavy[k] == 32 * 16
        for m in vec.members:
            lens = prof.lengths[:, m.digit]
            if m.classes[k] == "S":
                assert prof.threshold < lens.min() and lens.max() <= mc.HEAVY_S
            elif m.classes[k] == "M":
                assert lens.min() > mc.HEAVY_S
            else:
                assert lens.max() <= prof.threshold


def test_join_vector_invariants():
    vec = mc.build_joins()
    owned = _check_scalars(vec)
    assert not vec.scalars[~owned].any()
    names = [m.name for m in vec.members]
    assert len(set(names)) == len(names) >= 24
    for m in vec.members:
        for k, prof in enumerate(vec.profiles):
            assert prof.classes_of(m.digit) == {m.classes[k]}
            assert len(m.indices[k]) == (mc.JOIN_COUNTS[(m.classes[k], m.recipes[k])] if m.recipes[k] else 0)
        # alone in the vector (the per-sequence comparison zeroes every other scalar) the classes are the same
        assert [mc.list_class(len(ix), mc.heavy_threshold(16 * len(ix), mc.TOTAL_BUCKETS)) for ix in m.indices] == list(m.classes)
    assert vec.heavy == [16 * sum(m.classes[k] in "SM" for m in vec.members) for k in range(4)] and all(vec.heavy)
    # every kind of join meets every exceptional case
    joins = {}
    for m in vec.members:
        inf_after = mc.running_sum_is_infinity(m)
        for k in range(4):
            if m.recipes[k] is None:
                continue
            before = [q for q in range(k) if m.recipes[q] is not None]
            kind = "first_" + m.classes[k] if not before else m.classes[k]
            joins.setdefault(kind, set()).add((m.recipes[k], inf_after[before[-1]] if before else None))
    for kind in "LSM":
        cases = joins[kind]
        assert ("fresh", True) in cases, kind                                   # the old sum is infinity
        assert ("pairs", False) in cases, kind                                  # the incoming sum is infinity
        assert ("eq", False) in cases or ("dup", False) in cases, kind          # the incoming sum equals the old one
        assert ("neg", False) in cases, kind                                    # ... or cancels it
        assert ("inf", False) in cases, kind                                    # a base at infinity in the list
    assert {("pairs", None), ("inf", None), ("fresh", None)} <= joins["first_S"]
    # ... and after every cancellation a later piece resumes from the infinity, through each kind of join
    after_neg = {m.classes[k2] for m in vec.members for k in range(4) if m.recipes[k] == "neg"
                 for k2 in range(k + 1, 4) if m.recipes[k2] is not None}
    assert after_neg == {"L", "S", "M"}


def test_join_plan_makes_the_sums_it_promises(oracle):
    """the base plan applied to bases made by the oracle: after every piece a sequence's running sum is at infinity exactly where the recipe says,
    `eq` doubles the old sum (an L list: three more of it) and `dup` doubles it too"""
    from util import random_fr_canonical
    vec = mc.build_joins()
    used = np.concatenate([m.all_indices for m in vec.members])
    bases = np.zeros((mc.N, 8), np.uint64)
    bases[used] = oracle.g1_fixed_base(oracle.g1_generator(), random_fr_canonical(len(used), 0x9B10))
    mc.apply_base_plan(oracle, bases, vec.plan)
    for m in vec.members:
        inf_after = mc.running_sum_is_infinity(m)
        old = None
        for k in range(4):
            if m.recipes[k] is None:
                continue
            now = mc.affine_sum(oracle, bases[np.concatenate(m.indices[:k + 1])])
            assert (not now.any()) == inf_after[k], (m.name, k)
            if m.recipes[k] in ("eq", "dup"):
                times = 4 if (m.classes[k], m.recipes[k]) == ("L", "eq") else 2
                assert np.array_equal(now, mc.affine_sum(oracle, np.tile(old, (times, 1)))), (m.name, k)
            if m.recipes[k] == "inf":
                assert int((~bases[m.indices[k]].any(axis=1)).sum()) == 2
            old = now
