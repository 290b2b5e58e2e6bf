"""GPU parity: zkg_qap_instance_async, the QAP polynomials at a point t on the zkg_qap handle.  At | Bt | Ct and Z(t) against the oracle's
generator (oracle.groth16_setup emits them for a known trapdoor), bit for bit: radix-2 and step domains, a column of hundreds of terms in each
of the three matrix positions, segment lengths that cut it into several partial sums, column degrees at the LONG_COLUMN threshold, columns no
row touches, strides with gaps that must stay untouched, the ordering rule across streams and against zkg_qap_witness_h_async on the one
workspace, the index-build counter and the refusals.  The instance map is defined for any matrices: no satisfying witness is needed."""
import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from qap_instance_systems import log10_system, step_system
from r1cs_util import golden_case_arrays
from util import R, arr, from_limbs, golden, random_fr_canonical

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A5A5A5A5A
GOLDEN = [(c, False) for c in golden("groth16.json")] + [(c, True) for c in golden("groth16_step.json")]
LONG_COLUMN = 24                                             # columns above this many terms go one wavefront per segment (include/zkg.h)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def mont_t(td):
    """the trapdoor's t (canonical limbs, as the oracle takes it) in the Montgomery limbs the instance call takes"""
    return arr([from_limbs(td[0])], R)[0]


def degrees(M, n):
    return np.bincount(M[1].astype(np.int64), minlength=n + 1)


class System:
    """a constraint system with its handle and, per trapdoor seed, the oracle's At | Bt | Ct | Zt computed once"""

    def __init__(self, zkg, oracle, n, l, A, B, C):
        self.zkg, self.oracle, self.n, self.l, self.A, self.B, self.C = zkg, oracle, n, l, A, B, C
        self.keep = []
        self.ocs = oracle.make_r1cs(n, l, A, B, C, self.keep)
        self.cs = zkg.make_r1cs(n, l, A, B, C, self.keep)
        self.qap = zkg.Qap(self.cs)
        self.m = self.qap.domain_size()
        self._want = {}

    def td(self, seed):
        return random_fr_canonical(5, seed)

    def want(self, seed):
        if seed not in self._want:
            key = self.oracle.groth16_setup(self.ocs, self.td(seed))
            assert key["m"] == self.m
            self._want[seed] = (np.stack([key["At"], key["Bt"], key["Ct"]]), key["Zt"].copy())
        return self._want[seed]

    def buffers(self, stride):
        import torch
        d_abc = torch.full((3 * stride + 2, 4), FILL, dtype=torch.int64, device="cuda")      # two elements behind the third vector's stride
        d_z = torch.full((3, 4), FILL, dtype=torch.int64, device="cuda")                     # Z(t) goes into the middle one
        return d_abc, d_z

    def check(self, seed, stride, d_abc, d_z):
        """both buffers against the oracle, every gap and tail against the fill"""
        n = self.n
        abc, z = self.want(seed)
        got = _host(d_abc)
        for k in range(3):
            assert np.array_equal(got[k * stride:k * stride + n + 1], abc[k]), "ABC"[k]
            assert (got[k * stride + n + 1:(k + 1) * stride] == FILL).all(), "ABC"[k]
        assert (got[2 * stride + n + 1:] == FILL).all()
        if d_z is not None:
            gz = _host(d_z)
            assert np.array_equal(gz[1], z) and (gz[0] == FILL).all() and (gz[2] == FILL).all()
        return got

    def run(self, seed, stride=None, stream=0, with_z=True):
        import torch
        stride = self.n + 1 if stride is None else stride
        d_abc, d_z = self.buffers(stride)
        self.qap.instance_async(mont_t(self.td(seed)), d_abc.data_ptr(), stride, d_z.data_ptr() + 32 if with_z else 0, stream)
        stats = self.zkg.qap_instance_stats()
        torch.cuda.synchronize()
        if not with_z:
            assert (_host(d_z) == FILL).all()
        return self.check(seed, stride, d_abc, d_z if with_z else None), stats


_SYSTEMS = {}


@pytest.fixture(scope="module")
def systems(zkg, oracle):
    def get(kind):
        if kind not in _SYSTEMS:
            if kind == "step":
                n, l, A, B, C, _ = step_system()
            else:                                                       # "log10", "log10-BCA", "log10-CAB": the long column in B, A, C
                n, l, A, B, C, _ = log10_system()
                if kind == "log10-BCA":
                    A, B, C = B, C, A
                elif kind == "log10-CAB":
                    A, B, C = C, A, B
            _SYSTEMS[kind] = System(zkg, oracle, n, l, A, B, C)
        return _SYSTEMS[kind]
    yield get
    for s in _SYSTEMS.values():
        s.qap.free()
    _SYSTEMS.clear()


@pytest.mark.parametrize("case,step", GOLDEN, ids=[c["tag"] for c, _ in GOLDEN])
def test_golden_systems_equal_the_oracle_at_two_strides(zkg, oracle, case, step):
    """m = 8 ... 64 on radix-2 domains and the step domains of the golden file: At | Bt | Ct and Z(t), packed and with a gap of four"""
    A, B, C, pts, w, r, s = golden_case_arrays(case)
    assert (case.get("domain") == "step") == step
    sy = System(zkg, oracle, case["num_variables"], case["num_inputs"], A, B, C)
    try:
        assert sy.m == case["m"]
        first, _ = sy.run(0x51)
        second, _ = sy.run(0x51, stride=sy.n + 5)
        n = sy.n
        for k in range(3):
            assert np.array_equal(first[k * (n + 1):(k + 1) * (n + 1)], second[k * (n + 5):k * (n + 5) + n + 1])
    finally:
        sy.qap.free()


@pytest.mark.parametrize("kind,pos", [("log10", 1), ("log10-BCA", 0), ("log10-CAB", 2)])
def test_a_column_of_403_terms_in_each_matrix_position_whole_and_in_four_segments(zkg, systems, kind, pos):
    """m = 2^10, n = 1065: the constant's column holds a term of every bitness row (403), every other column at most 20, and hundreds of
    columns are touched by no row.  The matrices as given and in the rotations (B, C, A) and (C, A, B); at the default segment length (one
    segment) and at 128 (four, the last of 19 terms): equal to each other and to the oracle"""
    s = systems(kind)
    n = s.n
    assert n == 1065 and s.m == 1 << 10
    deg = [degrees(M, n) for M in (s.A, s.B, s.C)]
    assert deg[pos][0] == 403 and deg[pos][1:].max() <= 20 and all(d.max() <= 20 for k, d in enumerate(deg) if k != pos)
    untouched = sorted(int((d == 0).sum()) for d in deg)
    assert untouched == sorted([251, 468, 245])
    whole, _ = s.run(0x61)
    s.qap.set_column_segment(128)
    try:
        cut, stats = s.run(0x61, stride=n + 3)
        assert stats[0] == 0                                            # the segment list is rebuilt, the index is not
    finally:
        s.qap.set_column_segment(0)
    again, _ = s.run(0x61)
    assert np.array_equal(whole, again)
    for k in range(3):
        assert np.array_equal(whole[k * (n + 1):(k + 1) * (n + 1)], cut[k * (n + 3):k * (n + 3) + n + 1])
        zero = np.nonzero(deg[k] == 0)[0]
        zero = zero[zero > s.l] if k == 0 else zero                     # columns 0 .. l of A carry u[C + j]
        assert not whole[k * (n + 1) + zero].any()                      # a column no row touches is exactly zero


def test_column_degrees_at_the_threshold(zkg, oracle):
    """single-term rows appended to A of that system so that one column holds exactly LONG_COLUMN terms (the last a lane walks alone) and
    another LONG_COLUMN + 1 (the first that goes to a wavefront): both, and a column no row touches, equal the oracle's"""
    n, l, A, B, C, _ = log10_system()
    deg = degrees(A, n)
    x, y = (int(v) for v in np.nonzero((deg > 0) & (deg <= 20) & (np.arange(n + 1) > l))[0][:2])
    z = int(np.nonzero((deg == 0) & (np.arange(n + 1) > l))[0][0])
    cols = np.array([x] * (LONG_COLUMN - int(deg[x])) + [y] * (LONG_COLUMN + 1 - int(deg[y])), np.uint32)
    rng = random_fr_canonical(len(cols), 0x71)                          # any coefficients: read as Montgomery limbs
    A = (np.concatenate([A[0], A[0][-1] + np.arange(1, len(cols) + 1, dtype=np.uint32)]), np.concatenate([A[1], cols]), np.concatenate([A[2], rng]))
    B = (np.concatenate([B[0], np.full(len(cols), B[0][-1], np.uint32)]), B[1], B[2])
    C = (np.concatenate([C[0], np.full(len(cols), C[0][-1], np.uint32)]), C[1], C[2])
    deg = degrees(A, n)
    assert deg[x] == LONG_COLUMN and deg[y] == LONG_COLUMN + 1 and deg[z] == 0
    s = System(zkg, oracle, n, l, A, B, C)
    try:
        got, _ = s.run(0x72)
        want = s.want(0x72)[0][0]
        for j in (x, y, z):
            assert np.array_equal(got[j], want[j]), j
        assert want[x].any() and want[y].any() and not got[z].any()
    finally:
        s.qap.free()


def test_step_domain_with_a_column_of_1466_terms(zkg, systems):
    """m = 2^12 + 2^6: column 0 of B has 1466 terms, A has five columns of 25 - 27 and the constant's of 48 (one wavefront, one segment
    each)"""
    s = systems("step")
    assert s.m == (1 << 12) + (1 << 6)
    da, db = degrees(s.A, s.n), degrees(s.B, s.n)
    assert db[0] == 1466
    long_a = da[1:][da[1:] > LONG_COLUMN]
    assert len(long_a) == 5 and long_a.min() >= 25 and long_a.max() <= 27
    assert da[0] == 8 + 40                                              # the constant's column of A: the padding rows 1 * 0 = 0 on top of its own 8
    s.run(0x81, stride=s.n + 2)
    s.qap.set_column_segment(512)                                       # three segments, the last of 442
    try:
        s.run(0x81)
    finally:
        s.qap.set_column_segment(0)


def test_two_calls_on_two_streams_follow_each_other(zkg, systems):
    """one handle, one workspace (u lies there): a call behind a large junk kernel on one stream and a second with another t on another
    stream, nothing synchronised in between — the second stream waits for the first call's event, and both results stand"""
    import torch
    s = systems("log10")
    s.run(0x61)                                                          # the index exists from here on: no call below waits on the host
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    junk = torch.zeros(8 << 20, dtype=torch.int64, device="cuda")
    stride = s.n + 1
    abc1, z1 = s.buffers(stride); abc2, z2 = s.buffers(stride)
    s.want(0x61), s.want(0x62)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            junk.add_(1)
    s.qap.instance_async(mont_t(s.td(0x61)), abc1.data_ptr(), stride, z1.data_ptr() + 32, s1.cuda_stream)
    assert zkg.qap_instance_stats() == (0, 0)
    s.qap.instance_async(mont_t(s.td(0x62)), abc2.data_ptr(), stride, z2.data_ptr() + 32, s2.cuda_stream)
    assert zkg.qap_instance_stats() == (0, 0)
    s2.synchronize()
    s.check(0x62, stride, abc2, z2)
    s.check(0x61, stride, abc1, z1)
    torch.cuda.synchronize()


def test_an_h_call_between_two_instance_calls_shares_the_workspace(zkg, oracle, systems):
    """instance, witness_h, instance on one handle over three streams: the H call's aA | aB | aC overwrite u, so each call must run behind
    the one before it.  H equals the oracle's, both instances are right"""
    import torch
    s = systems("log10")
    n, m = s.n, s.m
    w = log10_system()[5]
    assert oracle.r1cs_is_satisfied(s.ocs, w)
    want_h = oracle.qap_witness_h(s.ocs, w, m)
    s.want(0x61), s.want(0x62)
    d_w = _dev(w)
    d_h = torch.full((m + 3, 4), FILL, dtype=torch.int64, device="cuda")
    streams = [torch.cuda.Stream() for _ in range(3)]
    stride = n + 1
    abc1, z1 = s.buffers(stride); abc2, z2 = s.buffers(stride)
    torch.cuda.synchronize()
    s.qap.instance_async(mont_t(s.td(0x61)), abc1.data_ptr(), stride, z1.data_ptr() + 32, streams[0].cuda_stream)
    s.qap.witness_h_async(d_w.data_ptr(), 1, n, d_h.data_ptr(), m + 3, 0, streams[1].cuda_stream)
    s.qap.instance_async(mont_t(s.td(0x62)), abc2.data_ptr(), stride, z2.data_ptr() + 32, streams[2].cuda_stream)
    streams[2].synchronize()
    got_h = _host(d_h)
    assert np.array_equal(got_h[:m + 1], want_h) and (got_h[m + 1:] == FILL).all()
    s.check(0x61, stride, abc1, z1)
    s.check(0x62, stride, abc2, z2)
    torch.cuda.synchronize()


def test_the_index_is_built_by_the_first_call_only(zkg, oracle):
    case = golden("groth16.json")[0]
    A, B, C, pts, w, r, s_ = golden_case_arrays(case)
    s = System(zkg, oracle, case["num_variables"], case["num_inputs"], A, B, C)
    try:
        _, first = s.run(0xB1)
        assert first[0] == 1 and first[1] >= 1                          # one index build, waited for
        _, second = s.run(0xB1)
        assert second == (0, 0)
        _, third = s.run(0xB2, stride=s.n + 4, with_z=False)             # another t, a gap, no Z(t) asked for
        assert third == (0, 0)
    finally:
        s.qap.free()


def test_refusals_write_nothing(zkg, systems):
    import torch
    s = systems("log10")
    q, n = s.qap, s.n
    stride = n + 1
    s.run(0x61)
    d_abc, d_z = s.buffers(stride)
    h_abc = np.full((3 * stride, 4), FILL, np.uint64); h_z = np.full((1, 4), FILL, np.uint64)
    t = mont_t(s.td(0x61))
    pa, pz = d_abc.data_ptr(), d_z.data_ptr() + 32

    def refused(call):
        with pytest.raises(zkg.ZkgError) as e:
            call()
        assert "zkg_qap_instance_async" in str(e.value) and zkg.lib().zkg_last_error().decode()
        assert zkg.qap_instance_stats() == (0, 0)
        torch.cuda.synchronize()
        assert (_host(d_abc) == FILL).all() and (_host(d_z) == FILL).all() and (h_abc == FILL).all() and (h_z == FILL).all()

    null = zkg.Qap.__new__(zkg.Qap); null._h = None; null.n = n
    refused(lambda: null.instance_async(t, pa, stride, pz))             # a null handle, t, d_abc
    refused(lambda: q.instance_async(None, pa, stride, pz))
    refused(lambda: q.instance_async(t, 0, stride, pz))
    refused(lambda: q.instance_async(t, pa, n, pz))                      # vectors that overlap
    refused(lambda: q.instance_async(t, pa, (1 << 32) + 1, pz))
    refused(lambda: q.instance_async(t, h_abc.ctypes.data, stride, pz))  # host memory
    refused(lambda: q.instance_async(t, pa, stride, h_z.ctypes.data))
    refused(lambda: q.instance_async(t, pa + 8, stride, pz))             # misaligned
    refused(lambda: q.instance_async(t, pa, stride, pz + 8))
    refused(lambda: q.instance_async(t, pa, 1 << 31, pz))                # the second vector lies beyond the allocation
    # a d_abc that is one stride short of its allocation: an allocation of its own (12 MiB is a size the caching allocator neither rounds nor,
    # with its cache emptied, carves out of a larger block), three vectors 2^17 apart starting one stride into it
    torch.cuda.empty_cache()
    big_stride = 1 << 17
    big = torch.full((3 * big_stride, 4), FILL, dtype=torch.int64, device="cuda")
    refused(lambda: q.instance_async(t, big.data_ptr() + big_stride * 32, big_stride, pz))
    assert (_host(big) == FILL).all()
    del big
    refused(lambda: q.instance_async(t, pa, stride, pa + stride * 32))   # Z(t) inside the vectors' range
    refused(lambda: q.instance_async(arr([1], R)[0], pa, stride, pz))    # t = 1: a point of the domain, Z(t) = 0
    if torch.cuda.device_count() > 1:                                   # a calling thread on another device than the handle's
        torch.cuda.set_device(1)
        try:
            refused(lambda: q.instance_async(t, pa, stride, pz))
        finally:
            torch.cuda.set_device(0)
    q.instance_async(t, pa, stride, pz)                                  # and the handle still works
    torch.cuda.synchronize()
    s.check(0x61, stride, d_abc, d_z)
