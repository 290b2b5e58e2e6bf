"""GPU parity: the zkg_domain handle.  Batched, stream-ordered transforms (zkg_domain_ntt_async) against the oracle's fft on every vector,
radix-2 and step sizes, all four variants, strides with gaps that must stay untouched, groups cut by batch_max; the ordering rule across
streams; the counters; the refusals; the Lagrange kernel (zkg_domain_lagrange_async) against the golden values and the oracle, byte for
byte; and the two halves against each other (sum u_i a_i = the interpolated polynomial at t)."""
import math

import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from util import R, arr, golden, h, ints, limbs, random_fr_canonical

pytestmark = pytest.mark.gpu

MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]                    # (inverse, coset)
FILL = 0x5A5A5A5A5A5A5A5A
LARGE = 1 << 18                                              # from here on at most two vectors per call
RADIX2 = [2, 1 << 9, 1 << 10, 1 << 18]
STEPS = [3, 24, (1 << 10) + (1 << 7), (1 << 10) + (1 << 5), (1 << 18) + (1 << 17)]
STEP = golden("step_domain.json")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


_REF = {}


def reference(oracle, m):
    """the vectors of size m the tests share (three, two from 2^18 on) and the oracle's transform of each in every variant, computed once"""
    if m not in _REF:
        vecs = [random_fr_canonical(m, 0xD0A1 + 31 * m + i) for i in range(2 if m >= LARGE else 3)]
        _REF[m] = (vecs, {mode: [oracle.fft(v, inverse=mode[0], coset=mode[1]) for v in vecs] for mode in MODES})
    return _REF[m]


@pytest.fixture(scope="module")
def domains(zkg):
    made = {}

    def get(m):
        if m not in made:
            made[m] = zkg.Domain(m)
        return made[m]
    yield get
    for d in made.values():
        d.free()


def _run(dom, picks, vecs, stride, mode, stream=0):
    """one call over the vectors vecs[picks[i]], `stride` elements apart with FILL in the gaps -> the buffer afterwards, (count, stride, 4)"""
    import torch
    m = dom.m
    buf = np.full((len(picks), stride, 4), FILL, np.uint64)
    for i, p in enumerate(picks):
        buf[i, :m] = vecs[p]
    d = _dev(buf)
    dom.ntt_async(d.data_ptr(), count=len(picks), stride=stride, inverse=mode[0], coset=mode[1], stream=stream)
    torch.cuda.synchronize()
    return _host(d).reshape(len(picks), stride, 4)


@pytest.mark.parametrize("m", RADIX2 + STEPS)
def test_every_vector_of_a_batch_equals_the_oracle(zkg, oracle, domains, m):
    """counts 1, 2, 3 (1, 2 from 2^18 on) at stride m and m + 5, and five vectors in groups of two (three launch sequences) up to 2^10 + 2^7"""
    dom = domains(m)
    assert dom.size() == m and dom.batch_max() == max(1, min(65535, (1 << 30) // (m * 40)))
    vecs, want = reference(oracle, m)
    cases = [(list(range(c)), 0) for c in ((1, 2) if m >= LARGE else (1, 2, 3))]
    if m <= (1 << 10) + (1 << 7):
        cases.append(([0, 1, 2, 0, 1], 2))
    for picks, bmax in cases:
        dom.set_batch_max(bmax)
        for stride in (m, m + 5):
            for mode in MODES:
                got = _run(dom, picks, vecs, stride, mode)
                assert zkg.domain_stats()[:2] == (len(picks), math.ceil(len(picks) / dom.batch_max())), (m, picks, stride, mode)
                for i, p in enumerate(picks):
                    assert np.array_equal(got[i, :m], want[mode][p]), (m, picks, stride, mode, i)
                assert (got[:, m:] == FILL).all(), (m, picks, stride, mode)
    dom.set_batch_max(0)


@pytest.mark.parametrize("m", [1 << 10, (1 << 10) + (1 << 7)])
def test_calls_follow_their_stream_and_each_other_across_streams(zkg, oracle, domains, m):
    """the vectors are written by a copy queued on a busy side stream and the call follows on that stream with nothing synchronised in
    between; then a forward call on one stream and its inverse on another through the one handle: the second stream is made to wait for
    the first call's event, so after synchronising IT the data is the input again — plain pair and coset pair"""
    import torch
    dom = domains(m)
    vecs, want = reference(oracle, m)
    src = _dev(np.stack(vecs))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    junk = torch.zeros(8 << 20, dtype=torch.int64, device="cuda")
    for coset in (0, 1):
        d = torch.full_like(src, FILL)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            for _ in range(4):
                junk.add_(1)
            d.copy_(src, non_blocking=True)
        dom.ntt_async(d.data_ptr(), count=3, coset=coset, stream=s1.cuda_stream)
        s1.synchronize()
        for i in range(3):
            assert np.array_equal(_host(d)[i], want[(0, coset)][i]), (m, coset, i)
        d.copy_(src)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            for _ in range(4):
                junk.add_(1)
        dom.ntt_async(d.data_ptr(), count=3, coset=coset, stream=s1.cuda_stream)
        dom.ntt_async(d.data_ptr(), count=3, inverse=True, coset=coset, stream=s2.cuda_stream)
        s2.synchronize()
        assert np.array_equal(_host(d), np.stack(vecs)), (m, coset)
        torch.cuda.synchronize()


def test_a_call_on_a_second_stream_that_grows_the_scratch_waits_once(zkg, oracle):
    """m = 8, a fresh handle: one vector on one stream, then three on another — a larger group, so the scratch the first call may still be in
    is freed and made anew behind one host wait.  Both calls give what they give alone on one stream"""
    import torch
    m = 8
    vecs, want = reference(oracle, m)
    dom = zkg.Domain(m)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        d1, d3 = _dev(vecs[0]), _dev(np.stack(vecs))
        torch.cuda.synchronize()
        dom.ntt_async(d1.data_ptr(), count=1, stream=s1.cuda_stream)
        dom.ntt_async(d3.data_ptr(), count=3, stream=s2.cuda_stream)
        assert zkg.domain_stats() == (3, 1, 1)
        s2.synchronize()
        got1, got3 = _host(d1), _host(d3)
        torch.cuda.synchronize()
        alone = _run(dom, [0, 1, 2], vecs, m, (0, 0))
        assert zkg.domain_stats() == (3, 1, 0)
        assert np.array_equal(got1, alone[0]) and np.array_equal(got3, alone)
        assert np.array_equal(got3, np.stack(want[(0, 0)]))
    finally:
        dom.free()


def test_counters_groups_and_the_empty_batch(zkg, oracle):
    """on a fresh handle the first call at a group size may wait (it allocates the scratch); the same call again does not; the groups are
    ceil(count / batch_max); an empty batch is ZKG_OK and touches nothing"""
    import torch
    m = (1 << 10) + (1 << 7)
    vecs, want = reference(oracle, m)
    dom = zkg.Domain(m)
    try:
        default = dom.batch_max()
        assert default == (1 << 30) // (m * 40)
        dom.set_batch_max(default + 7)
        assert dom.batch_max() == default                               # clamped
        dom.set_batch_max(2)
        assert dom.batch_max() == 2
        picks = [0, 1, 2, 0, 1]
        got = _run(dom, picks, vecs, m, (0, 0))
        first = zkg.domain_stats()
        assert first[:2] == (5, 3) and first[2] <= 1
        got = _run(dom, picks, vecs, m, (0, 0))
        assert zkg.domain_stats() == (5, 3, 0)
        for i, p in enumerate(picks):
            assert np.array_equal(got[i, :m], want[(0, 0)][p])
        dom.set_batch_max(0)
        assert dom.batch_max() == default
        _run(dom, picks, vecs, m, (1, 1))                               # one group of five: more scratch than two vectors took
        assert zkg.domain_stats()[:2] == (5, 1)
        _run(dom, picks, vecs, m, (1, 1))
        assert zkg.domain_stats() == (5, 1, 0)
        _run(dom, [0, 1], vecs, m, (0, 1))                              # a smaller group fits the scratch that is there
        assert zkg.domain_stats() == (2, 1, 0)
        canary = torch.full((m, 4), FILL, dtype=torch.int64, device="cuda")
        dom.ntt_async(canary.data_ptr(), count=0)
        assert zkg.domain_stats() == (0, 0, 0)
        torch.cuda.synchronize()
        assert (_host(canary) == FILL).all()
    finally:
        dom.free()


def test_refusals_write_nothing(zkg, oracle, domains):
    import torch
    m = 24
    dom = domains(m)
    vecs, want = reference(oracle, m)
    d = torch.full((2 * m + 1, 4), FILL, dtype=torch.int64, device="cuda")
    h_buf = np.full((2 * m, 4), FILL, np.uint64)
    pinned = torch.full((2 * m, 4), FILL, dtype=torch.int64).pin_memory()
    t = arr([7], R)[0]
    p = d.data_ptr()

    def refused(call, who="zkg_domain_ntt_async"):
        with pytest.raises(zkg.ZkgError) as e:
            call()
        assert who in str(e.value) and zkg.lib().zkg_last_error().decode()
        torch.cuda.synchronize()
        assert (_host(d) == FILL).all() and (h_buf == FILL).all() and (pinned.numpy().view(np.uint64) == FILL).all()

    null = zkg.Domain.__new__(zkg.Domain); null._h = None; null.m = m
    refused(lambda: null.ntt_async(p))                                  # a null handle, a null pointer
    refused(lambda: dom.ntt_async(0))
    refused(lambda: dom.ntt_async(p, count=2, stride=m - 1))            # vectors that overlap
    refused(lambda: dom.ntt_async(p, count=(1 << 24) + 1))              # too many vectors, too far apart
    refused(lambda: dom.ntt_async(p, count=2, stride=(1 << 32) + 1))
    refused(lambda: dom.ntt_async(h_buf.ctypes.data))                   # plain host memory, pinned host memory
    refused(lambda: dom.ntt_async(pinned.data_ptr()))
    refused(lambda: dom.ntt_async(p + 8))                               # misaligned
    refused(lambda: dom.ntt_async(p, count=2, stride=1 << 31))          # the second vector lies beyond the allocation
    if torch.cuda.device_count() > 1:                                   # a calling thread on another device than the handle's
        torch.cuda.set_device(1)
        try:
            refused(lambda: dom.ntt_async(p))
            refused(lambda: dom.lagrange_async(t, p), "zkg_domain_lagrange_async")
        finally:
            torch.cuda.set_device(0)
    who = "zkg_domain_lagrange_async"                                   # the Lagrange entry: the same rules for d_u and d_z
    refused(lambda: null.lagrange_async(t, p), who)
    refused(lambda: dom.lagrange_async(t, 0), who)
    refused(lambda: dom.lagrange_async(t, h_buf.ctypes.data), who)
    refused(lambda: dom.lagrange_async(t, pinned.data_ptr()), who)
    refused(lambda: dom.lagrange_async(t, p + 8), who)
    refused(lambda: dom.lagrange_async(t, p, h_buf.ctypes.data), who)   # d_z in host memory, misaligned
    refused(lambda: dom.lagrange_async(t, p, p + m * 32 + 8), who)
    d[:m].copy_(_dev(vecs[0])); d[m:2 * m].copy_(_dev(vecs[1]))         # and the handle still works
    dom.ntt_async(p, count=2)
    torch.cuda.synchronize()
    assert np.array_equal(_host(d)[:m], want[(0, 0)][0]) and np.array_equal(_host(d)[m:2 * m], want[(0, 0)][1])


def _root_of_unity(n):
    """the root of unity of order n (a power of two) the domains use: 5^((r - 1) / n)"""
    return pow(5, (R - 1) // n, R)


def _lagrange(dom, t_int, with_z=True):
    """-> (u as (m, 4) limbs, Z as 4 limbs or None) for the canonical integer t"""
    import torch
    d_u = torch.full((dom.m, 4), FILL, dtype=torch.int64, device="cuda")
    d_z = torch.full((1, 4), FILL, dtype=torch.int64, device="cuda")
    dom.lagrange_async(arr([t_int], R)[0], d_u.data_ptr(), d_z.data_ptr() if with_z else 0)
    torch.cuda.synchronize()
    if not with_z:
        assert (_host(d_z) == FILL).all()
    return _host(d_u), (_host(d_z)[0] if with_z else None)


@pytest.mark.parametrize("case", STEP["lagrange"], ids=[str(c["m"]) for c in STEP["lagrange"]])
def test_lagrange_equals_the_golden_values_byte_for_byte(zkg, domains, case):
    """step sizes 3 ... 48: the small segment of one element, both segments inside one lane's run, the segments' border between two lanes"""
    dom = domains(case["m"])
    u, z = _lagrange(dom, h(case["t"]))
    assert np.array_equal(u, arr([h(x) for x in case["u"]], R))
    assert np.array_equal(z, arr([h(case["Z"])], R)[0])


@pytest.mark.parametrize("m", [2, 8, 1 << 10, 1 << 13, (1 << 9) + (1 << 3), (1 << 10) + (1 << 5), (1 << 13) + (1 << 10)])
def test_lagrange_equals_the_oracle_byte_for_byte(zkg, oracle, domains, m):
    """a random t, t = 0 and t = 5; sizes below one lane's run, several workgroups, a last workgroup that is not full; Z(t) optional"""
    dom = domains(m)
    for t in (int(ints(random_fr_canonical(1, 0x1A6 + m))[0]), 0, 5):
        want_u, want_z = oracle.domain_lagrange(m, np.array(limbs(t), np.uint64))
        u, z = _lagrange(dom, t)
        assert np.array_equal(u, want_u) and np.array_equal(z, want_z), (m, t)
    u, _ = _lagrange(dom, 5, with_z=False)
    assert np.array_equal(u, want_u), m


def test_lagrange_refuses_a_domain_point_before_any_launch(zkg, domains):
    import torch
    points = {8: [pow(_root_of_unity(8), 3, R)]}
    for c in STEP["fft"]:
        if c["m"] == 24:
            points[24] = [h(c["points"][3]), h(c["points"][c["big"] + 1])]      # one of each segment
    assert len(points[24]) == 2
    for m, ts in points.items():
        dom = domains(m)
        d_u = torch.full((m, 4), FILL, dtype=torch.int64, device="cuda")
        d_z = torch.full((1, 4), FILL, dtype=torch.int64, device="cuda")
        for t in ts:
            with pytest.raises(zkg.ZkgError) as e:
                dom.lagrange_async(arr([t], R)[0], d_u.data_ptr(), d_z.data_ptr())
            assert "domain point" in str(e.value)
            torch.cuda.synchronize()
            assert (_host(d_u) == FILL).all() and (_host(d_z) == FILL).all()


@pytest.mark.parametrize("m", [1 << 10, (1 << 10) + (1 << 7)])
def test_the_two_halves_meet(zkg, domains, m):
    """a: the values of a polynomial on the domain.  Its coefficients come from the handle's inverse transform, the Lagrange coefficients
    from the handle's kernel: sum u_i a_i, in Python integers, is the polynomial at t (Horner on the coefficients)"""
    import torch
    dom = domains(m)
    a = random_fr_canonical(m, 0x7A1 + m)                   # Montgomery representations of some values
    t = int(ints(random_fr_canonical(1, 0x7A2 + m))[0])
    d = _dev(a)
    dom.ntt_async(d.data_ptr(), inverse=True)
    torch.cuda.synchronize()
    coeffs = ints(_host(d), R)
    u, _ = _lagrange(dom, t)
    lhs = sum(x * y for x, y in zip(ints(u, R), ints(a, R))) % R
    rhs = 0
    for c in reversed(coeffs):
        rhs = (rhs * t + c) % R
    assert lhs == rhs
