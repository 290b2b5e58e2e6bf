"""GPU parity: zkg_msm_g1_resident_async (batched resident multi-exponentiation whose points stay in device memory, finished by the
one-workgroup epilogue kernel k_msm_combine) against zkg_msm_g1_resident and the oracle, bit for bit on the normalised point; its
stream-order contract, its refusals, and the epilogue kernel alone (zkg_msm_combine_gpu) against the chunk-sum formula on oracle points."""
import numpy as np
import pytest

from gpu_util import dev_bases_g1, zkg  # noqa: F401
from util import Q, R, arr, limbs, random_fr_canonical

pytestmark = pytest.mark.gpu

INF = arr([0, 1, 0], Q).reshape(12)                     # the normalised encoding of infinity: (0, one, 0)
ONE = np.array([1, 0, 0, 0], np.uint64)
FILL = 0x5A5A5A5A5A5A5A5A


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


class Bases:
    """a resident handle of n bases (a duplicated base and a base at infinity from 300 points on) with the scalar vectors the tests share and
    the synchronous call's point for each of them, computed once"""

    def __init__(self, zkg, n):
        import torch
        self.zkg, self.n = zkg, n
        self.d_bases, self.bases, _ = dev_bases_g1(zkg, n, 0xA51C + n)
        if n >= 300:
            self.bases[7] = self.bases[8]; self.bases[9] = 0
            self.d_bases = torch.from_numpy(self.bases.view(np.int64)).cuda()
        self.h = zkg.ResidentBases(self.d_bases.data_ptr(), n)
        self._vec, self._sync = {}, {}

    def vector(self, kind):
        if kind not in self._vec:
            n = self.n
            if kind == "zero":
                sc = np.zeros((n, 4), np.uint64)
            elif kind == "bits":                                       # mostly 0 / 1, with r - 1 (on the duplicated pair too)
                sc = random_fr_canonical(n, 0xB175 + n); rng = np.random.default_rng(n); k = rng.integers(0, 100, n)
                sc[k < 45] = 0; sc[(k >= 45) & (k < 90), :] = ONE; sc[0] = limbs(R - 1)
                if n >= 300:
                    sc[7] = sc[8] = limbs(R - 1)
            else:                                                      # "u0", "u1", ...: uniform
                sc = random_fr_canonical(n, 0xC0FFEE + 977 * int(kind[1:]) + n)
            self._vec[kind] = sc
        return self._vec[kind]

    def sync(self, kind):
        if kind not in self._sync:
            self._sync[kind] = self.h.msm(_dev(self.vector(kind)).data_ptr())
        return self._sync[kind]

    def run_async(self, kinds, stride=None, mont=False):
        """one asynchronous call on the null stream over the vectors `kinds`, `stride` elements apart with 0xFF.. in the gaps"""
        import torch
        n = self.n; stride = n if stride is None else stride
        buf = np.full((len(kinds), stride, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
        for i, kind in enumerate(kinds):
            v = self.vector(kind)
            buf[i, :n] = arr([x for x in _ints(v)], R) if mont else v
        d_sc = _dev(buf)
        d_out = torch.full((len(kinds), 12), FILL, dtype=torch.int64, device="cuda")
        self.h.msm_async(d_sc.data_ptr(), d_out.data_ptr(), count=len(kinds), stride=stride, scalars_mont=mont)
        stats = self.zkg.msm_resident_async_stats()
        torch.cuda.synchronize()
        return _host(d_out), stats


def _ints(a):
    return [sum(int(v) << (64 * i) for i, v in enumerate(r)) for r in a]


@pytest.fixture(scope="module")
def resident(zkg):
    made = {}

    def get(n):
        if n not in made:
            made[n] = Bases(zkg, n)
        return made[n]
    yield get
    for b in made.values():
        b.h.free()


@pytest.mark.parametrize("n", [1, 300, 5000, 32768, 70000])
def test_single_vectors_equal_the_synchronous_call_bit_for_bit(zkg, oracle, resident, n):
    """every table window size (8 / 12 / 16 bits) and the row merge from 49152 points on; uniform scalars, mostly-bit scalars with r - 1, and
    an all-zero vector, whose point is the (0, one, 0) encoding"""
    b = resident(n)
    for kind in ("u0", "bits", "zero"):
        got, stats = b.run_async([kind])
        assert stats[:2] == (1, 1)
        assert np.array_equal(got[0], b.sync(kind)), kind
        if n <= 5000:
            assert np.array_equal(got[0], oracle.msm_g1(b.bases, b.vector(kind))), kind
    assert np.array_equal(b.sync("zero"), INF) and np.array_equal(b.run_async(["zero"])[0][0], INF)


@pytest.mark.parametrize("gap", [0, 3])
@pytest.mark.parametrize("count", [2, 5])
@pytest.mark.parametrize("n", [300, 5000, 32768])
def test_batches_equal_the_synchronous_call_on_each_vector(zkg, resident, n, count, gap):
    """count vectors through ONE launch sequence, contiguous and with a gap of three 0xFF.. elements that must never be read.  Five vectors:
    a uniform one twice, an all-zero one, a mostly-bit one, another uniform one.  Two vectors cannot hold both an all-zero and an identical
    pair: (uniform, zero) without the gap, the same uniform vector twice with it."""
    b = resident(n)
    kinds = ["u0", "zero", "bits", "u0", "u1"] if count == 5 else (["u0", "zero"] if gap == 0 else ["u0", "u0"])
    got, stats = b.run_async(kinds, stride=n + gap)
    assert stats[:2] == (count, 1)
    for i, kind in enumerate(kinds):
        assert np.array_equal(got[i], b.sync(kind)), (i, kind)


def test_a_batch_of_montgomery_scalars(zkg, resident):
    b = resident(5000)
    kinds = ["u0", "zero", "bits", "u0", "u1"]
    got, _ = b.run_async(kinds, stride=5003, mont=True)
    for i, kind in enumerate(kinds):
        assert np.array_equal(got[i], b.sync(kind)), (i, kind)


def test_more_vectors_than_one_launch_takes_are_split_into_two_groups(zkg, resident):
    """batch_max() + 1 vectors at 70000 points (16-bit windows, merged rows): two launch groups, the second of one vector through the
    single-vector launch; at a shape the handle has served the call makes no host wait"""
    b = resident(70000)
    bmax = b.h.batch_max()
    assert 1 <= bmax <= 32
    cycle = ["u0", "zero", "bits", "u1"]
    kinds = [cycle[i % 4] for i in range(bmax + 1)]
    b.run_async(kinds)                                                  # the first call at this shape may grow the workspace
    got, stats = b.run_async(kinds)
    for i, kind in enumerate(kinds):
        assert np.array_equal(got[i], b.sync(kind)), (i, kind)
    assert stats == (bmax + 1, 2, 0)


def test_a_smaller_group_after_a_full_one_on_a_fresh_handle_drains_before_it_grows_a_buffer(zkg):
    """16-bit windows: the reduction's chunk records SHRINK as the group grows (eight vectors: 16 chunks each, 384 records; three: 64
    chunks, 576; one: 256 chunks, 768), so on a handle whose first launch is a full group every smaller group still has a buffer to grow —
    while the launches before it may be reading it.  Calls on a fresh handle: a full group; a group of three; a full group and a group of
    one in ONE call; a group of three again.  Right points everywhere, the waits of the first three counted, none in the fourth."""
    b = Bases(zkg, 32768)
    try:
        bmax = b.h.batch_max()
        assert bmax == 8
        cycle = ["u0", "bits", "u1", "zero"]
        calls = [[cycle[i % 4] for i in range(bmax)], ["u1", "u0", "bits"], [cycle[(i + 1) % 4] for i in range(bmax + 1)], ["bits", "u1", "u0"]]
        results = [b.run_async(kinds) for kinds in calls]
        stats = [st for _, st in results]
        assert stats[0][:2] == (bmax, 1) and stats[0][2] >= 1           # the fresh workspace
        assert stats[1][:2] == (3, 1) and stats[1][2] >= 1              # 576 records where 384 were reserved
        assert stats[2][:2] == (bmax + 1, 2) and stats[2][2] >= 1       # the group of one: 768 records
        assert stats[3] == (3, 1, 0)
        for kinds, (got, _) in zip(calls, results):
            for i, kind in enumerate(kinds):
                assert np.array_equal(got[i], b.sync(kind)), (kinds, i)
    finally:
        b.h.free()


def test_the_call_stays_on_the_callers_stream_and_does_not_wait_on_the_host(zkg, resident):
    """the scalars are produced on a side stream behind ~0.3 s of queued work; the call returns while that stream is still busy, having
    waited for nothing, and a copy queued on the same stream afterwards sees the point"""
    import torch
    b = resident(5000)
    want = b.sync("u1")
    src = _dev(b.vector("u1"))
    b.run_async(["u0"])                                                 # warm: this shape is served
    side = torch.cuda.Stream()
    d_out = torch.full((1, 12), FILL, dtype=torch.int64, device="cuda")
    h_out = torch.empty((1, 12), dtype=torch.int64).pin_memory()
    d_late = torch.zeros_like(src)
    torch.cuda.synchronize()
    can_sleep = hasattr(torch.cuda, "_sleep")
    if can_sleep:                                                       # cycles per millisecond of the sleep kernel's counter, measured on a short one
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            e0.record(); torch.cuda._sleep(2_000_000); e1.record()
        side.synchronize()
        per_ms = 2_000_000 / max(e0.elapsed_time(e1), 1e-3)
    with torch.cuda.stream(side):
        if can_sleep:
            torch.cuda._sleep(int(300 * per_ms))
        else:
            junk = torch.empty(32 << 20, dtype=torch.int64, device="cuda")
            for _ in range(4):
                junk.add_(1)
        d_late.copy_(src, non_blocking=True)
    b.h.msm_async(d_late.data_ptr(), d_out.data_ptr(), stream=side.cuda_stream)
    busy = not side.query()
    stats = zkg.msm_resident_async_stats()
    with torch.cuda.stream(side):
        h_out.copy_(d_out, non_blocking=True)
    side.synchronize()
    if can_sleep:
        assert busy, "the call returned only after the side stream had drained"
    assert stats == (1, 1, 0)
    assert np.array_equal(h_out.numpy().view(np.uint64)[0], want)


def test_calls_back_to_back_and_a_synchronous_call_beside_them(zkg, resident):
    """three asynchronous calls with their own scalars and outputs, nothing synchronised in between, then the synchronous entry on the same
    handle, then one synchronisation: four right points"""
    import torch
    b = resident(5000)
    kinds = ["u0", "bits", "u1"]
    want = [b.sync(k) for k in kinds] + [b.sync("u2")]
    d_sc = [_dev(b.vector(k)) for k in kinds]; d_last = _dev(b.vector("u2"))
    d_out = [torch.full((1, 12), FILL, dtype=torch.int64, device="cuda") for _ in kinds]
    torch.cuda.synchronize()
    for s, o in zip(d_sc, d_out):
        b.h.msm_async(s.data_ptr(), o.data_ptr())
    last = b.h.msm(d_last.data_ptr())
    torch.cuda.synchronize()
    for o, w in zip(d_out, want):
        assert np.array_equal(_host(o)[0], w)
    assert np.array_equal(last, want[3])


def test_refusals_write_nothing(zkg, resident):
    import torch
    b = resident(300); n = 300
    d_sc = _dev(np.stack([b.vector("u0"), b.vector("u1")]))
    d_out = torch.full((2, 12), FILL, dtype=torch.int64, device="cuda")
    h_sc = np.ascontiguousarray(b.vector("u0")); h_out = np.full((2, 12), FILL, np.uint64)
    sp, op = d_sc.data_ptr(), d_out.data_ptr()

    def refused(call):
        with pytest.raises(zkg.ZkgError):
            call()
        torch.cuda.synchronize()
        assert (_host(d_out) == FILL).all() and (h_out == FILL).all()

    refused(lambda: b.h.msm_async(0, op))                               # null arguments
    refused(lambda: b.h.msm_async(sp, 0))
    null = zkg.ResidentBases.__new__(zkg.ResidentBases); null._h = None; null.n = n
    refused(lambda: null.msm_async(sp, op))
    b.h.n = n + 1                                                       # not the handle's point count
    try:
        refused(lambda: b.h.msm_async(sp, op))
    finally:
        b.h.n = n
    refused(lambda: b.h.msm_async(sp, op, count=2, stride=n - 1))       # vectors that overlap
    refused(lambda: b.h.msm_async(h_sc.ctypes.data, op))                # host memory
    refused(lambda: b.h.msm_async(sp, h_out.ctypes.data))
    b.h.msm_async(sp, op, count=0)                                      # an empty batch: OK, nothing touched
    assert zkg.msm_resident_async_stats() == (0, 0, 0)
    torch.cuda.synchronize()
    assert (_host(d_out) == FILL).all()
    b.h.msm_async(sp, op, count=2)                                      # and the handle still works
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_out)[0], b.sync("u0")) and np.array_equal(_host(d_out)[1], b.sync("u1"))


# ---- the epilogue kernel alone -------------------------------------------------------------------------------------------------------
def _records(oracle, mult):
    """small multiples of the generator as normalised Jacobian records (0 -> infinity); also the affine points"""
    gen = oracle.g1_generator()
    aff = oracle.g1_fixed_base(gen, arr([m % R for m in mult])).reshape(-1, 8)
    jac = np.zeros((len(mult), 12), np.uint64)
    jac[:, :8] = aff; jac[:, 8:] = arr([1], Q).reshape(4)
    for i, m in enumerate(mult):
        if m % R == 0:
            jac[i] = INF
    return aff, jac


def _combine_case(zkg, oracle, mult, cpw, slots, chunk_log, vectors):
    """mult: vectors x cpw x slots integers.  Expected per vector, on the oracle's points: V = sum U_ch [+ 8 sum A_ch, T in U's place]
    + 2^chunk_log sum ch P_ch + sum P_ch — every record times its weight (g1_scalar_mul), summed (g1_sum); the same in integers as a
    check of the test's own arithmetic"""
    flat = [int(m) for m in np.asarray(mult, dtype=object).reshape(-1)]
    aff, jac = _records(oracle, flat)
    got = zkg.msm_combine_gpu(jac, cpw, slots, chunk_log, vectors)
    gen = oracle.g1_generator()
    for v in range(vectors):
        terms, total = [], 0
        for ch in range(cpw):
            for s in range(slots):
                i = (v * cpw + ch) * slots + s
                weight = ((ch << chunk_log) + 1) if s == 0 else (1 if s == 1 else 8)
                terms.append(oracle.g1_scalar_mul(aff[i], np.array(limbs(weight), np.uint64)))
                total += weight * flat[i]
        want = oracle.g1_sum(np.array(terms))
        assert np.array_equal(want, oracle.g1_scalar_mul(gen, np.array(limbs(total % R), np.uint64)))
        assert np.array_equal(got[v], want), (cpw, slots, chunk_log, vectors, v)
    return got


@pytest.mark.parametrize("vectors", [1, 3])
@pytest.mark.parametrize("chunk_log", [0, 5])
@pytest.mark.parametrize("slots", [2, 3])
@pytest.mark.parametrize("cpw", [1, 2, 16, 17, 64, 128, 129, 256, 257, 600])
def test_the_epilogue_kernel_matches_the_chunk_sum_formula(zkg, oracle, cpw, slots, chunk_log, vectors):
    """cpw up to 256: one chunk per lane at 1 ... 256 lanes (128 | 129: the step from 128 lanes to 256; 256: the last one-chunk-per-lane
    shape); 257 and 600: two and four chunks per lane (more chunks than the kernel has lanes).
    Records are multiples -40 ... 40 of the generator with about one in six at infinity."""
    rng = np.random.default_rng(1000 * cpw + 100 * slots + 10 * chunk_log + vectors)
    mult = rng.integers(-40, 41, (vectors, cpw, slots))
    mult[rng.integers(0, 6, mult.shape) == 0] = 0
    _combine_case(zkg, oracle, mult, cpw, slots, chunk_log, vectors)


def test_the_epilogue_kernel_on_equal_and_cancelling_records(zkg, oracle):
    # every P_ch (and every U_ch) the same point: the scan's and the tree's additions meet equal operands and must double
    _combine_case(zkg, oracle, np.full((1, 16, 2), 5), 16, 2, 0, 1)
    _combine_case(zkg, oracle, np.full((2, 64, 3), 3), 64, 3, 5, 2)
    # records that cancel: P alternates +7 / -7 (suffix sums pass through infinity), and U_0 takes away what is left
    cpw, cl = 16, 5
    mult = np.zeros((1, cpw, 2), dtype=object)
    for ch in range(cpw):
        mult[0, ch, 0] = 7 if ch % 2 == 0 else -7
    mult[0, 0, 1] = -sum(((ch << cl) + 1) * int(mult[0, ch, 0]) for ch in range(cpw))
    got = _combine_case(zkg, oracle, mult, cpw, 2, cl, 1)
    assert np.array_equal(got[0], INF)
    # an all-infinity vector beside a live one
    mult = np.zeros((2, 17, 3), dtype=object); mult[1, 16, 2] = 1
    got = _combine_case(zkg, oracle, mult, 17, 3, 0, 2)
    assert np.array_equal(got[0], INF) and not np.array_equal(got[1], INF)


@pytest.mark.parametrize("live", ["P and T", "A"])
def test_the_A_term_is_neither_lost_nor_counted_twice(zkg, oracle, live):
    """three-slot records at cpw 17 (a 32-lane workgroup with lanes behind the last chunk): the kernel finishes 8 A behind its chunk loop,
    before the scan.  Every A at infinity: the point is the two-slot one.  Only A live: the point is 8 sum A."""
    cpw, cl = 17, 5
    rng = np.random.default_rng(317)
    mult = rng.integers(1, 41, (2, cpw, 3))
    if live == "A":
        mult[:, :, :2] = 0
        got = _combine_case(zkg, oracle, mult, cpw, 3, cl, 2)
        for v in range(2):
            total = 8 * int(mult[v, :, 2].sum())
            assert np.array_equal(got[v], oracle.g1_scalar_mul(oracle.g1_generator(), np.array(limbs(total % R), np.uint64)))
    else:
        mult[:, :, 2] = 0
        got = _combine_case(zkg, oracle, mult, cpw, 3, cl, 2)
        assert np.array_equal(got, _combine_case(zkg, oracle, mult[:, :, :2], cpw, 2, cl, 2))
