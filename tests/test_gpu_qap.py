"""GPU parity: the zkg_qap handle.  coefficients_for_H of device-resident witnesses (zkg_qap_witness_h_async) against the golden values, the
oracle's r1cs_to_qap_witness_map and the key-bound entry zkg_qap_witness_h, byte for byte: radix-2 and step domains, long rows in all three
matrices, batches cut into groups, strides with gaps that must stay untouched, the per-witness unsatisfied flag, the ordering rule across
streams, the composition with zkg_msm_g1_resident_async on one stream, the counters and the refusals."""
import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from r1cs_util import golden_case_arrays
from util import R, arr, golden, h, ints, random_fr_canonical

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A5A5A5A5A
FLAG_FILL = 0x5A5A5A5A
GOLDEN = [(c, False) for c in golden("groth16.json")] + [(c, True) for c in golden("groth16_step.json")]
LONG_ROW = 24                                                # rows above this many terms go one wavefront per row


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _terms(M, vals, r):
    return [(int(M[1][k]), vals[k]) for k in range(int(M[0][r]), int(M[0][r + 1]))]


def solve_witness(n, l, A, B, C, seed):
    """another satisfying witness of a zklaim_shaped system: the rows are walked in order, a variable first met in A or B is drawn (a bit
    in a bitness row b * (1 - b) = 0, 248 bits elsewhere) and the one variable of C not met before is solved for"""
    rng = np.random.default_rng(seed)
    va, vb, vc = (ints(M[2], R) for M in (A, B, C))
    z = [None] * (n + 1)
    z[0] = 1
    for i in range(1, l + 1):
        z[i] = int.from_bytes(rng.bytes(31), "little")
    dot = lambda row: sum(c * z[v] for v, c in row) % R
    for r in range(len(A[0]) - 1):
        ra, rb, rc = _terms(A, va, r), _terms(B, vb, r), _terms(C, vc, r)
        bitness = len(ra) == 1 and len(rb) == 2 and not rc and rb[0][0] == 0 and rb[1][0] == ra[0][0]
        for v, _ in ra + rb:
            if z[v] is None:
                z[v] = int(rng.integers(0, 2)) if bitness else int.from_bytes(rng.bytes(31), "little")
        new = [(v, c) for v, c in rc if z[v] is None]
        assert len(new) <= 1
        if new:
            v, c = new[0]
            rest = sum(c_ * z[v_] for v_, c_ in rc if v_ != v) % R
            z[v] = (dot(ra) * dot(rb) - rest) * pow(c, -1, R) % R
    assert all(x is not None for x in z)
    return arr(z[1:], R)


def with_long_rows_everywhere(A, B, C):
    """the last row of a zklaim_shaped system is the padding row 1 * 0 = 0; it becomes the padding row 1 * S = S with S the sum of the first
    30 variables, satisfied by every witness: B and C then hold a row above LONG_ROW terms as A (the packing rows) does, and C + l + 1 stays"""
    assert A[0][-1] - A[0][-2] == 1 and A[1][-1] == 0 and B[0][-1] == B[0][-2] and C[0][-1] == C[0][-2]
    cols = np.arange(1, 31, dtype=np.uint32); ones = np.tile(arr([1], R), (30, 1))
    grow = lambda M: (np.concatenate([M[0][:-1], [M[0][-1] + 30]]).astype(np.uint32), np.concatenate([M[1], cols]), np.concatenate([M[2], ones]))
    return A, grow(B), grow(C)


class System:
    """a constraint system with its handle, satisfying witnesses under several seeds and the oracle's H of every witness asked for, computed once"""

    def __init__(self, zkg, oracle, n, l, A, B, C, w):
        self.zkg, self.oracle, self.n, self.l, self.A, self.B, self.C = zkg, oracle, n, l, A, B, C
        self.keep = []
        self.ocs = oracle.make_r1cs(n, l, A, B, C, self.keep)
        self.cs = zkg.make_r1cs(n, l, A, B, C, self.keep)
        self.qap = zkg.Qap(self.cs)
        self.m = self.qap.domain_size()
        self._w = {0: w}
        self._h = {}
        self._key = None

    def witness(self, name):
        """0: the generator's own; k > 0: solved under seed k; ("bad", k): witness k with its last element changed; ("pack", k): witness k with
        the value of the last packing row changed (only a long row is violated)"""
        if name not in self._w:
            if isinstance(name, tuple):
                w = self.witness(name[1]).copy()
                if name[0] == "bad":
                    w[-1, 0] ^= np.uint64(1)
                else:
                    long_a = np.nonzero(np.diff(self.A[0].astype(np.int64)) > LONG_ROW)[0]
                    w[int(self.C[1][self.C[0][long_a[-1]]]) - 1, 0] ^= np.uint64(1)
                self._w[name] = w
            else:
                self._w[name] = solve_witness(self.n, self.l, self.A, self.B, self.C, name)
                assert self.oracle.r1cs_is_satisfied(self.ocs, self._w[name])
        return self._w[name]

    def want(self, name):
        if name not in self._h:
            self._h[name] = self.oracle.qap_witness_h(self.ocs, self.witness(name), self.m)
        return self._h[name]

    def key(self):
        if self._key is None:
            self._key = self.oracle.groth16_setup(self.ocs, random_fr_canonical(5, 0x0A9))
            assert self._key["m"] == self.m
        return self._key

    def run(self, names, stride=None, h_stride=None, stream=0, flags=True):
        """one call over the witnesses `names` with FILL in every gap -> (H buffer (count, h_stride, 4), the flag words and the three behind them)"""
        import torch
        n, m = self.n, self.m
        stride = n if stride is None else stride; h_stride = m + 1 if h_stride is None else h_stride
        buf = np.full((len(names), stride, 4), FILL, np.uint64)
        for i, name in enumerate(names):
            buf[i, :n] = self.witness(name)
        d_w = _dev(buf)
        d_h = torch.full((len(names), h_stride, 4), FILL, dtype=torch.int64, device="cuda")
        d_f = torch.full((len(names) + 3,), FLAG_FILL, dtype=torch.int32, device="cuda")
        self.qap.witness_h_async(d_w.data_ptr(), len(names), stride, d_h.data_ptr(), h_stride, d_f.data_ptr() if flags else 0, stream)
        stats = self.zkg.qap_stats()
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_w).reshape(buf.shape), buf)                       # read in place, never written: the tails hold the fill
        got = _host(d_h).reshape(len(names), h_stride, 4)
        assert (got[:, m + 1:] == FILL).all()
        return got, d_f.cpu().numpy().view(np.uint32), stats


_SYSTEMS = {}


@pytest.fixture(scope="module")
def systems(zkg, oracle):
    def get(kind):
        if kind not in _SYSTEMS:
            from zklaim_amd import synth
            if kind == "log10":                                         # m = 2^10: four workgroups per vector, long rows in A, B and C
                n, l, A, B, C, w = synth.zklaim_shaped(10, num_inputs=5, seed=0x0A)
                A, B, C = with_long_rows_everywhere(A, B, C)
            else:                                                       # "step": the padded system of test_prove_step_domain_with_large_ratio, m = 2^12 + 2^6
                n, l, A, B, C, w = synth.zklaim_shaped(12, num_inputs=5, seed=19)
                pad = 40
                A = (np.concatenate([A[0], A[0][-1] + np.arange(1, pad + 1, dtype=np.uint32)]), np.concatenate([A[1], np.zeros(pad, np.uint32)]),
                     np.concatenate([A[2], np.tile(arr([1], R), (pad, 1))]))                                 # 1 * 0 = 0
                B = (np.concatenate([B[0], np.full(pad, B[0][-1], np.uint32)]), B[1], B[2])
                C = (np.concatenate([C[0], np.full(pad, C[0][-1], np.uint32)]), C[1], C[2])
            _SYSTEMS[kind] = System(zkg, oracle, n, l, A, B, C, w)
            assert oracle.r1cs_is_satisfied(_SYSTEMS[kind].ocs, w)
        return _SYSTEMS[kind]
    yield get
    for s in _SYSTEMS.values():
        s.qap.free()
    _SYSTEMS.clear()


@pytest.mark.parametrize("case,step", GOLDEN, ids=[c["tag"] for c, _ in GOLDEN])
def test_h_equals_the_golden_coefficients(zkg, case, step):
    """m = 8 ... 64 on radix-2 domains, 10, 17, 24 and 48 on step domains: H is the case's "h", the flag 0, the zero stands at index m"""
    import torch
    A, B, C, pts, w, r, s = golden_case_arrays(case)
    keep = []
    n, m = case["num_variables"], case["m"]
    qap = zkg.Qap(zkg.make_r1cs(n, case["num_inputs"], A, B, C, keep))
    try:
        assert (case.get("domain") == "step") == step
        assert qap.domain_size() == m and qap.num_variables() == n == len(w)
        assert qap.batch_max() == max(1, min(65535 // 3, (1 << 30) // (m * 216)))
        d_w = _dev(w)
        d_h = torch.full((m + 3, 4), FILL, dtype=torch.int64, device="cuda")
        d_f = torch.full((2,), FLAG_FILL, dtype=torch.int32, device="cuda")
        qap.witness_h_async(d_w.data_ptr(), 1, n, d_h.data_ptr(), m + 3, d_f.data_ptr())
        assert zkg.qap_stats()[:2] == (1, 1)
        torch.cuda.synchronize()
        got = _host(d_h)
        assert ints(got[:m + 1], R) == [h(x) for x in case["h"]]
        assert not got[m].any() and (got[m + 1:] == FILL).all()
        assert d_f.cpu().numpy().view(np.uint32).tolist() == [0, FLAG_FILL]
    finally:
        qap.free()


def test_long_rows_in_every_matrix_over_several_workgroups_equal_the_oracle(zkg, oracle, systems):
    """m = 2^10, rows above 24 terms in A, B and C (one wavefront per row); a witness that violates only a long row is flagged by the pass over
    the long rows, and its H is the oracle's all the same; without flag words the same H"""
    s = systems("log10")
    assert s.m == 1 << 10
    for M in (s.A, s.B, s.C):
        assert (np.diff(M[0].astype(np.int64)) > LONG_ROW).any()
    got, flags, stats = s.run([0])
    assert stats[:2] == (1, 1)
    assert np.array_equal(got[0, :s.m + 1], s.want(0)) and not got[0, s.m].any()
    assert flags.tolist() == [0] + [FLAG_FILL] * 3
    assert not oracle.r1cs_is_satisfied(s.ocs, s.witness(("pack", 0)))
    got, flags, _ = s.run([("pack", 0), 0])
    assert flags.tolist() == [1, 0] + [FLAG_FILL] * 3
    assert np.array_equal(got[0, :s.m + 1], s.want(("pack", 0))) and np.array_equal(got[1, :s.m + 1], s.want(0))
    got, flags, _ = s.run([("pack", 0)], flags=False)
    assert np.array_equal(got[0, :s.m + 1], s.want(("pack", 0))) and (flags == FLAG_FILL).all()


def test_five_witnesses_in_groups_of_two_with_gaps_and_flags(zkg, systems):
    """five different witnesses, two of them with their last element changed, stride n + 3 and h_stride m + 6, groups of two (three launch
    sequences): every H equals that witness run alone and the oracle's, the flags are 0 1 0 1 0, every gap, input tail and the words behind
    the fifth flag hold the fill; the same call again makes no host wait"""
    s = systems("log10")
    n, m = s.n, s.m
    names = [0, ("bad", 1), 1, ("bad", 0), 2]
    alone = {}
    for name in names:
        got, flags, stats = s.run([name])
        assert stats[:2] == (1, 1)
        alone[name] = (got[0, :m + 1].copy(), int(flags[0]))
    default = s.qap.batch_max()
    s.qap.set_batch_max(default + 7)
    assert s.qap.batch_max() == default                                  # clamped
    s.qap.set_batch_max(2)
    try:
        assert s.qap.batch_max() == 2
        got, flags, first = s.run(names, stride=n + 3, h_stride=m + 6)
        assert first[:2] == (5, 3) and first[2] <= 1
        assert flags.tolist() == [0, 1, 0, 1, 0] + [FLAG_FILL] * 3
        for i, name in enumerate(names):
            assert np.array_equal(got[i, :m + 1], alone[name][0]), name
            assert np.array_equal(got[i, :m + 1], s.want(name)), name
            assert int(flags[i]) == alone[name][1], name
            assert not got[i, m].any()
        got2, flags2, second = s.run(names, stride=n + 3, h_stride=m + 6)
        assert second == (5, 3, 0)
        assert np.array_equal(got2, got) and np.array_equal(flags2, flags)
    finally:
        s.qap.set_batch_max(0)
    assert s.qap.batch_max() == default


def test_step_domain_with_the_chunked_fold_two_witnesses(zkg, systems):
    """m = 2^12 + 2^6 (big / small = 64: the fold and unfold walks are cut into chunks with a summing pass), two witnesses in one call"""
    s = systems("step")
    assert s.m == (1 << 12) + (1 << 6) and zkg.evaluation_domain_size(len(s.A[0]) - 1 + s.l + 1) == (s.m, True)
    got, flags, stats = s.run([0, 1], h_stride=s.m + 2)
    assert stats[:2] == (2, 1)
    assert flags.tolist() == [0, 0] + [FLAG_FILL] * 3
    for i in range(2):
        assert np.array_equal(got[i, :s.m + 1], s.want(i)), i


def test_the_key_bound_entry_gives_the_same_bytes(zkg, systems):
    """zkg_qap_witness_h on a key over the same system (host witness, slot lease, copy back) against the handle's output"""
    s = systems("log10")
    crs = zkg.Crs(zkg.make_pk(s.cs, s.key(), 10, s.keep))
    try:
        for name in (0, 1):
            got, _, _ = s.run([name])
            assert got[0, :s.m + 1].tobytes() == crs.qap_witness_h(s.witness(name)).tobytes(), name
    finally:
        crs.free()


def test_h_goes_straight_into_the_resident_msm_on_one_stream(zkg, oracle, systems):
    """witness_h_async for two witnesses and zkg_msm_g1_resident_async over d_h (n = m - 1, stride = h_stride, Montgomery scalars) queued back
    to back on one side stream, one synchronise at the end: both points are the oracle's multi-exponentiation of the key's H query"""
    import torch
    s = systems("log10")
    m = s.m
    h_query = np.ascontiguousarray(s.key()["H_query"])
    assert h_query.shape == (m - 1, 8)
    d_bases = _dev(h_query)
    bases = zkg.ResidentBases(d_bases.data_ptr(), m - 1)
    try:
        h_stride = m + 4
        d_w = _dev(np.stack([s.witness(0), s.witness(2)]))
        d_h = torch.full((2, h_stride, 4), FILL, dtype=torch.int64, device="cuda")
        d_out = torch.full((2, 12), FILL, dtype=torch.int64, device="cuda")
        side = torch.cuda.Stream()
        s.run([0, 2])                                                    # the handle has served a group of two from here on
        s.qap.witness_h_async(d_w.data_ptr(), 2, s.n, d_h.data_ptr(), h_stride, 0, side.cuda_stream)
        assert zkg.qap_stats() == (2, 1, 0)                              # the group size has been served: no wait, no allocation
        bases.msm_async(d_h.data_ptr(), d_out.data_ptr(), count=2, stride=h_stride, scalars_mont=True, stream=side.cuda_stream)
        side.synchronize()
        got = _host(d_out)
        for i, name in enumerate((0, 2)):
            assert np.array_equal(got[i], oracle.msm_g1(h_query, arr(ints(s.want(name)[:m - 1], R)))), name
    finally:
        bases.free()


def test_two_calls_on_two_streams_follow_each_other(zkg, systems):
    """one handle, one workspace: a call on a busy stream and a second on another stream with nothing synchronised in between — the second
    stream is made to wait for the first call's event, so after synchronising IT both results stand"""
    import torch
    s = systems("log10")
    n, m = s.n, s.m
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    junk = torch.zeros(8 << 20, dtype=torch.int64, device="cuda")
    first, second = [0, 1], [2, ("bad", 0)]
    src1, src2 = _dev(np.stack([s.witness(k) for k in first])), _dev(np.stack([s.witness(k) for k in second]))
    d_w1 = torch.full_like(src1, FILL)
    d_h1 = torch.full((2, m + 1, 4), FILL, dtype=torch.int64, device="cuda"); d_h2 = torch.full_like(d_h1, FILL)
    d_f = torch.full((4,), FLAG_FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            junk.add_(1)
        d_w1.copy_(src1, non_blocking=True)                              # the witnesses themselves arrive on the stream the call names
    s.qap.witness_h_async(d_w1.data_ptr(), 2, n, d_h1.data_ptr(), m + 1, d_f.data_ptr(), s1.cuda_stream)
    s.qap.witness_h_async(src2.data_ptr(), 2, n, d_h2.data_ptr(), m + 1, d_f.data_ptr() + 8, s2.cuda_stream)
    s2.synchronize()
    for i, name in enumerate(first):
        assert np.array_equal(_host(d_h1)[i], s.want(name)), name
    for i, name in enumerate(second):
        assert np.array_equal(_host(d_h2)[i], s.want(name)), name
    assert d_f.cpu().numpy().view(np.uint32).tolist() == [0, 0, 0, 1]
    torch.cuda.synchronize()


def test_a_call_on_a_second_stream_that_grows_the_workspace_waits_once(zkg, oracle):
    """a fresh handle: one witness on one stream, then two on another — a larger group, so the workspace the first call may still be in is
    freed and made anew behind one host wait.  Both calls give what they give alone on one stream, and the oracle's H"""
    import torch
    from qap_instance_systems import log10_system
    s = System(zkg, oracle, *log10_system())
    try:
        n, m = s.n, s.m
        names = [0, ("bad", 0)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        src1, src2 = _dev(s.witness(0)), _dev(np.stack([s.witness(k) for k in names]))
        d_h1 = torch.full((1, m + 1, 4), FILL, dtype=torch.int64, device="cuda"); d_h2 = torch.full((2, m + 1, 4), FILL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        s.qap.witness_h_async(src1.data_ptr(), 1, n, d_h1.data_ptr(), m + 1, 0, s1.cuda_stream)
        s.qap.witness_h_async(src2.data_ptr(), 2, n, d_h2.data_ptr(), m + 1, 0, s2.cuda_stream)
        assert zkg.qap_stats() == (2, 1, 1)
        s2.synchronize()
        got1, got2 = _host(d_h1).reshape(1, m + 1, 4), _host(d_h2).reshape(2, m + 1, 4)
        torch.cuda.synchronize()
        alone, _, stats = s.run(names)
        assert stats == (2, 1, 0)
        assert np.array_equal(got1[0], alone[0]) and np.array_equal(got2, alone)
        for i, name in enumerate(names):
            assert np.array_equal(got2[i], s.want(name)), name
    finally:
        s.qap.free()


def test_refusals_write_nothing(zkg, systems):
    import torch
    s = systems("log10")
    q, n, m = s.qap, s.n, s.m
    w2 = np.stack([s.witness(0), s.witness(1)])
    d_w = _dev(w2)
    d_h = torch.full((2 * (m + 1), 4), FILL, dtype=torch.int64, device="cuda")
    d_f = torch.full((4,), FLAG_FILL, dtype=torch.int32, device="cuda")
    both = torch.full((2 * n + 2 * (m + 1), 4), FILL, dtype=torch.int64, device="cuda")
    h_w = w2.copy(); h_h = np.full((2 * (m + 1), 4), FILL, np.uint64); h_f = np.full(4, FLAG_FILL, np.uint32)
    pw, ph, pf = d_w.data_ptr(), d_h.data_ptr(), d_f.data_ptr()

    def refused(call):
        with pytest.raises(zkg.ZkgError) as e:
            call()
        assert "zkg_qap_witness_h_async" in str(e.value) and zkg.lib().zkg_last_error().decode()
        assert zkg.qap_stats() == (0, 0, 0)
        torch.cuda.synchronize()
        assert (_host(d_h) == FILL).all() and (d_f.cpu().numpy().view(np.uint32) == FLAG_FILL).all() and (_host(both) == FILL).all()
        assert np.array_equal(_host(d_w).reshape(w2.shape), w2) and (h_h == FILL).all() and (h_f == FLAG_FILL).all() and np.array_equal(h_w, w2)

    null = zkg.Qap.__new__(zkg.Qap); null._h = None
    refused(lambda: null.witness_h_async(pw, 2, n, ph, m + 1, pf))       # a null handle, null pointers
    refused(lambda: q.witness_h_async(0, 2, n, ph, m + 1, pf))
    refused(lambda: q.witness_h_async(pw, 2, n, 0, m + 1, pf))
    refused(lambda: q.witness_h_async(pw, 2, n - 1, ph, m + 1, pf))      # witnesses that overlap, outputs that overlap
    refused(lambda: q.witness_h_async(pw, 2, n, ph, m, pf))
    refused(lambda: q.witness_h_async(pw, (1 << 24) + 1, n, ph, m + 1, pf))   # too many witnesses, too far apart
    refused(lambda: q.witness_h_async(pw, 2, (1 << 32) + 1, ph, m + 1, pf))
    refused(lambda: q.witness_h_async(pw, 2, n, ph, (1 << 32) + 1, pf))
    refused(lambda: q.witness_h_async(h_w.ctypes.data, 2, n, ph, m + 1, pf))   # host memory for each of the three buffers
    refused(lambda: q.witness_h_async(pw, 2, n, h_h.ctypes.data, m + 1, pf))
    refused(lambda: q.witness_h_async(pw, 2, n, ph, m + 1, h_f.ctypes.data))
    refused(lambda: q.witness_h_async(pw + 8, 1, n, ph, m + 1, pf))      # misaligned: 16 bytes for the vectors, 4 for the flags
    refused(lambda: q.witness_h_async(pw, 2, n, ph + 8, m + 1, pf))
    refused(lambda: q.witness_h_async(pw, 2, n, ph, m + 1, pf + 2))
    refused(lambda: q.witness_h_async(pw, 2, n, ph, 1 << 31, pf))        # the second output lies beyond the allocation
    refused(lambda: q.witness_h_async(pw, 2, 1 << 31, ph, m + 1, pf))
    pb = both.data_ptr()
    refused(lambda: q.witness_h_async(pb, 2, n, pb + n * 32, m + 1, pf))               # the output starts inside the second witness
    refused(lambda: q.witness_h_async(pb + (m + 1) * 32, 2, n, pb, m + 1, pf))         # the witnesses start inside the first output
    if torch.cuda.device_count() > 1:                                   # a calling thread on another device than the handle's
        torch.cuda.set_device(1)
        try:
            refused(lambda: q.witness_h_async(pw, 2, n, ph, m + 1, pf))
        finally:
            torch.cuda.set_device(0)
    q.witness_h_async(pw, 2, n, ph, m + 1, pf)                           # and the handle still works
    torch.cuda.synchronize()
    got = _host(d_h).reshape(2, m + 1, 4)
    assert np.array_equal(got[0], s.want(0)) and np.array_equal(got[1], s.want(1))
    assert d_f.cpu().numpy().view(np.uint32).tolist() == [0, 0, FLAG_FILL, FLAG_FILL]


def test_a_broken_constraint_system_makes_no_handle(zkg):
    """checked on the host, once: the kernels index z by the columns and walk the rows by the row pointers"""
    case = golden("groth16.json")[0]
    A, B, C, pts, w, r, s = golden_case_arrays(case)
    n, l = case["num_variables"], case["num_inputs"]

    def refused(n_, l_, A_, B_, C_, what):
        keep = []
        with pytest.raises(zkg.ZkgError) as e:
            zkg.Qap(zkg.make_r1cs(n_, l_, A_, B_, C_, keep))
        assert "zkg_qap_new" in str(e.value) and what in str(e.value), str(e.value)

    col = B[1].copy(); col[-1] = n + 1
    refused(n, l, A, (B[0], col, B[2]), C, "column")                    # a column index above n
    col = C[1].copy(); col[0] = 0xFFFFFFFF
    refused(n, l, A, B, (C[0], col, C[2]), "column")
    rp = A[0].copy(); rp[-2] = rp[-1] + 1
    refused(n, l, (rp, A[1], A[2]), B, C, "decreases")             # a decreasing row pointer
    rp = A[0].copy(); rp[0] = 1
    refused(n, l, (rp, A[1], A[2]), B, C, "start at 0")
    refused(n, n + 1, A, B, C, "num_inputs")
    empty = (np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 4), np.uint64))
    refused(n, l, empty, empty, empty, "without constraints")
    keep = []
    zkg.Qap(zkg.make_r1cs(n, l, A, B, C, keep)).free()                   # the system as it is makes one
