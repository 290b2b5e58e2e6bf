"""GPU parity: zkg_msm_g2_resident / zkg_msm_g2_resident_async (fixed G2 bases kept with their per-window tables; batched, the points left in
device memory by the one-workgroup epilogue kernel k_msm_combine<Fq2, 128>) against zkg_msm_g2_dev on the plain bases and the oracle, bit for bit on
the normalised point; the stream-order contract, the refusals, and the epilogue kernel alone (zkg_msm_combine_g2_gpu) against the chunk-sum
formula in integers and one oracle scalar multiplication."""
import numpy as np
import pytest

from gpu_util import g2_jac_of_affine, to_dev, zkg  # noqa: F401
from util import R, arr, g2_jac_expected, limbs, random_fr_canonical

pytestmark = pytest.mark.gpu

POOL = 32768
INF = g2_jac_expected(None)                             # the normalised encoding of infinity: (0, one, 0) with one = (Montgomery one, 0)
ONE = np.array([1, 0, 0, 0], np.uint64)
FILL = 0x5A5A5A5A5A5A5A5A


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _ints(a):
    return [sum(int(v) << (64 * i) for i, v in enumerate(r)) for r in a]


@pytest.fixture(scope="module")
def pool(oracle):
    """32 768 distinct G2 bases k_i * G, shared (read-only) by every handle"""
    bases = oracle.g2_fixed_base(oracle.g2_generator(), random_fr_canonical(POOL, 0x62A5E5))
    bases.setflags(write=False)
    return bases


class Bases:
    """a resident handle of the pool's first n bases (a duplicated base and a base at infinity from 300 points on) with the scalar vectors the
    tests share and, computed once per vector, the synchronous call's point and zkg_msm_g2_dev's on the plain bases"""

    def __init__(self, zkg, pool, n):
        self.zkg, self.n = zkg, n
        self.bases = np.ascontiguousarray(pool[:n]).copy()
        if n >= 300:
            self.bases[7] = self.bases[8]; self.bases[9] = 0
        self.d_bases = to_dev(self.bases)
        self.h = zkg.ResidentBasesG2(self.d_bases.data_ptr(), n)
        self._vec, self._sync, self._plain = {}, {}, {}

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
            self._sync[kind] = self.h.msm(to_dev(self.vector(kind)).data_ptr())
        return self._sync[kind]

    def plain(self, kind):
        if kind not in self._plain:
            self._plain[kind] = self.zkg.msm_g2_dev(self.d_bases.data_ptr(), to_dev(self.vector(kind)).data_ptr(), self.n)
        return self._plain[kind]

    def run_async(self, kinds, stride=None, mont=False):
        """one asynchronous call on the null stream over the vectors `kinds`, `stride` elements apart with 0xFF.. in the gaps"""
        import torch
        n = self.n; stride = n if stride is None else stride
        buf = np.full((len(kinds), stride, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
        for i, kind in enumerate(kinds):
            v = self.vector(kind)
            buf[i, :n] = arr(_ints(v), R) if mont else v
        d_sc = to_dev(buf)
        d_out = torch.full((len(kinds), 24), FILL, dtype=torch.int64, device="cuda")
        self.h.msm_async(d_sc.data_ptr(), d_out.data_ptr(), count=len(kinds), stride=stride, scalars_mont=mont)
        stats = self.zkg.msm_resident_async_stats()
        torch.cuda.synchronize()
        return _host(d_out), stats


@pytest.fixture(scope="module")
def resident(zkg, pool):
    made = {}

    def get(n):
        if n not in made:
            made[n] = Bases(zkg, pool, n)
        return made[n]
    yield get
    for b in made.values():
        b.h.free()


# ---- 1. single vectors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 300, 5000, 32768])
def test_single_vectors_equal_the_synchronous_call_and_the_plain_path_bit_for_bit(zkg, oracle, resident, n):
    """every table window size (8 / 12 / 16 bits); uniform scalars, mostly-bit scalars with r - 1, and an all-zero vector, whose point is the
    (0, one, 0) encoding from both entries"""
    b = resident(n)
    for kind in ("u0", "bits", "zero"):
        got, stats = b.run_async([kind])
        assert stats[:2] == (1, 1)
        assert np.array_equal(got[0], b.sync(kind)), kind
        assert np.array_equal(got[0], b.plain(kind)), kind
        if n <= 5000:
            assert np.array_equal(got[0], oracle.msm_g2(b.bases, b.vector(kind), oracle.BDLO12, oracle.num_threads())), kind
    assert np.array_equal(b.sync("zero"), INF) and np.array_equal(b.run_async(["zero"])[0][0], INF)


# ---- 2. batches -----------------------------------------------------------------------------------------------------------------------
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


# ---- 3. Montgomery scalars --------------------------------------------------------------------------------------------------------------
def test_a_batch_of_montgomery_scalars(zkg, resident):
    b = resident(5000)
    kinds = ["u0", "zero", "bits", "u0", "u1"]
    got, _ = b.run_async(kinds, stride=5003, mont=True)
    for i, kind in enumerate(kinds):
        assert np.array_equal(got[i], b.sync(kind)), (i, kind)


# ---- 4. more vectors than one launch takes ----------------------------------------------------------------------------------------------
def test_more_vectors_than_one_launch_takes_are_split_into_two_groups(zkg, resident):
    """batch_max() + 1 vectors at 32768 points (16-bit windows): two launch groups, the second of one vector through the single-vector
    launch; at a shape the handle has served the call makes no host wait"""
    b = resident(32768)
    bmax = b.h.batch_max()
    assert 1 <= bmax <= 16
    cycle = ["u0", "zero", "bits", "u1"]
    kinds = [cycle[i % 4] for i in range(bmax + 1)]
    b.run_async(kinds)                                                  # the first call at this shape may grow the workspace
    got, stats = b.run_async(kinds)
    for i, kind in enumerate(kinds):
        assert np.array_equal(got[i], b.sync(kind)), (i, kind)
    assert stats == (bmax + 1, 2, 0)


# ---- 5. a smaller group after a full one ------------------------------------------------------------------------------------------------
def test_a_smaller_group_after_a_full_one_on_a_fresh_handle(zkg, pool):
    """the reduction's chunk records shrink as the group grows, so a smaller group may still have a buffer to grow while the launches before
    it read it.  Calls on a fresh handle: a full group; a group of three; a full group and a group of one in ONE call; a group of three
    again.  Right points everywhere and no wait in the fourth call; which of the earlier calls grow which buffer is not pinned here."""
    b = Bases(zkg, pool, 32768)
    try:
        bmax = b.h.batch_max()
        cycle = ["u0", "bits", "u1", "zero"]
        calls = [[cycle[i % 4] for i in range(bmax)], ["u1", "u0", "bits"], [cycle[(i + 1) % 4] for i in range(bmax + 1)], ["bits", "u1", "u0"]]
        results = [b.run_async(kinds) for kinds in calls]
        stats = [st for _, st in results]
        three = -(-3 // bmax)                                           # groups that three vectors make
        assert stats[0][:2] == (bmax, 1)
        assert stats[1][:2] == (3, three)
        assert stats[2][:2] == (bmax + 1, 2)
        assert stats[3] == (3, three, 0)
        for kinds, (got, _) in zip(calls, results):
            for i, kind in enumerate(kinds):
                assert np.array_equal(got[i], b.sync(kind)), (kinds, i)
    finally:
        b.h.free()


# ---- 6. stream order --------------------------------------------------------------------------------------------------------------------
def test_the_call_stays_on_the_callers_stream_and_does_not_wait_on_the_host(zkg, resident):
    """the scalars are produced on a side stream behind ~0.3 s of queued work; the call returns while that stream is still busy, having
    waited for nothing, and a copy queued on the same stream afterwards sees the point"""
    import torch
    b = resident(5000)
    want = b.sync("u1")
    src = to_dev(b.vector("u1"))
    b.run_async(["u0"])                                                 # warm: this shape is served
    side = torch.cuda.Stream()
    d_out = torch.full((1, 24), FILL, dtype=torch.int64, device="cuda")
    h_out = torch.empty((1, 24), dtype=torch.int64).pin_memory()
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


# ---- 7. ordering on one handle ----------------------------------------------------------------------------------------------------------
def test_calls_back_to_back_and_a_synchronous_call_beside_them(zkg, resident):
    """three asynchronous calls with their own scalars and outputs, nothing synchronised in between, then the synchronous entry on the same
    handle, then one synchronisation: four right points"""
    import torch
    b = resident(5000)
    kinds = ["u0", "bits", "u1"]
    want = [b.sync(k) for k in kinds] + [b.sync("u2")]
    d_sc = [to_dev(b.vector(k)) for k in kinds]; d_last = to_dev(b.vector("u2"))
    d_out = [torch.full((1, 24), FILL, dtype=torch.int64, device="cuda") for _ in kinds]
    torch.cuda.synchronize()
    for s, o in zip(d_sc, d_out):
        b.h.msm_async(s.data_ptr(), o.data_ptr())
    last = b.h.msm(d_last.data_ptr())
    torch.cuda.synchronize()
    for o, w in zip(d_out, want):
        assert np.array_equal(_host(o)[0], w)
    assert np.array_equal(last, want[3])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(zkg, resident):
    import torch
    b = resident(300); n = 300
    want = [b.sync("u0"), b.sync("u1")]
    d_sc = to_dev(np.stack([b.vector("u0"), b.vector("u1")]))
    d_out = torch.full((2, 24), FILL, dtype=torch.int64, device="cuda")
    h_sc = np.ascontiguousarray(b.vector("u0")); h_out = np.full((2, 24), FILL, np.uint64)
    sp, op = d_sc.data_ptr(), d_out.data_ptr()

    def refused(call):
        with pytest.raises(zkg.ZkgError):
            call()
        torch.cuda.synchronize()
        assert (_host(d_out) == FILL).all() and (h_out == FILL).all()

    refused(lambda: b.h.msm_async(0, op))                               # null arguments
    refused(lambda: b.h.msm_async(sp, 0))
    null = zkg.ResidentBasesG2.__new__(zkg.ResidentBasesG2); null._h = None; null.n = n
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
    assert np.array_equal(_host(d_out)[0], want[0]) and np.array_equal(_host(d_out)[1], want[1])


# ---- 9. the epilogue kernel alone ---------------------------------------------------------------------------------------------------------
class Multiples(dict):
    """k -> k * G2 as a normalised 24-limb record (0: infinity); -40 ... 40 computed once, any other k when it is first asked for"""

    def __init__(self, oracle):
        super().__init__()
        self.oracle = oracle
        self.add(range(-40, 41))

    def add(self, ks):
        ks = [int(k) for k in ks]
        aff = self.oracle.g2_fixed_base(self.oracle.g2_generator(), arr([k % R for k in ks]))
        for i, k in enumerate(ks):
            self[k] = g2_jac_of_affine(aff[i]) if k % R else INF

    def __missing__(self, k):
        self.add([k])
        return self[k]


@pytest.fixture(scope="module")
def multiples(oracle):
    return Multiples(oracle)


def _combine_case(zkg, oracle, multiples, mult, cpw, chunk_log, vectors):
    """mult: vectors x cpw x 2 integers in [-40, 40].  Expected per vector: (T mod r) * G2 with T = sum over the records of weight * k, weight
    (ch << chunk_log) + 1 for P and 1 for U — integers and one oracle scalar multiplication, nothing of the code under test"""
    mult = np.asarray(mult, dtype=object).reshape(vectors, cpw, 2)
    jac = np.array([multiples[int(m)] for m in mult.reshape(-1)], np.uint64)
    got = zkg.msm_combine_g2_gpu(jac, cpw, chunk_log, vectors)
    totals = [sum((((ch << chunk_log) + 1) * int(mult[v, ch, 0]) + int(mult[v, ch, 1])) for ch in range(cpw)) % R for v in range(vectors)]
    want = oracle.g2_fixed_base(oracle.g2_generator(), arr(totals))
    for v in range(vectors):
        exp = g2_jac_of_affine(want[v]) if totals[v] else INF
        assert np.array_equal(got[v], exp), (cpw, chunk_log, vectors, v)
    return got


@pytest.mark.parametrize("vectors", [1, 3])
@pytest.mark.parametrize("chunk_log", [0, 5])
@pytest.mark.parametrize("cpw", [1, 2, 16, 17, 64, 128, 129, 257, 600])
def test_the_epilogue_kernel_matches_the_chunk_sum_formula(zkg, oracle, multiples, cpw, chunk_log, vectors):
    """cpw up to 128: one chunk per lane at 1 ... 128 of the kernel's 128 lanes (128: the last such shape); 129, 257 and 600: two, four and
    eight chunks per lane (more chunks than the kernel has lanes).  Records are multiples -40 ... 40 of the generator with about one in six at infinity."""
    rng = np.random.default_rng(1000 * cpw + 10 * chunk_log + vectors)
    mult = rng.integers(-40, 41, (vectors, cpw, 2))
    mult[rng.integers(0, 6, mult.shape) == 0] = 0
    _combine_case(zkg, oracle, multiples, mult, cpw, chunk_log, vectors)


def test_the_epilogue_kernel_on_equal_and_cancelling_records(zkg, oracle, multiples):
    # every P_ch and every U_ch the same point: the scan's and the tree's additions meet equal operands and must double
    _combine_case(zkg, oracle, multiples, np.full((1, 16, 2), 5), 16, 0, 1)
    _combine_case(zkg, oracle, multiples, np.full((2, 64, 2), 3), 64, 5, 2)
    # records that cancel: P alternates +7 / -7 (suffix sums pass through infinity), and U_0 takes away what is left
    cpw, cl = 16, 5
    mult = np.zeros((1, cpw, 2), dtype=object)
    for ch in range(cpw):
        mult[0, ch, 0] = 7 if ch % 2 == 0 else -7
    mult[0, 0, 1] = -sum(((ch << cl) + 1) * int(mult[0, ch, 0]) for ch in range(cpw))
    got = _combine_case(zkg, oracle, multiples, mult, cpw, cl, 1)
    assert np.array_equal(got[0], INF)
    # an all-infinity vector beside a live one
    mult = np.zeros((2, 17, 2), dtype=object); mult[1, 16, 1] = 1
    got = _combine_case(zkg, oracle, multiples, mult, 17, 0, 2)
    assert np.array_equal(got[0], INF) and not np.array_equal(got[1], INF)
