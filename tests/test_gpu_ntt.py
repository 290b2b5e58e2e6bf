"""GPU parity: zkg_ntt (HIP) vs the oracle's libfqfft restatement and the golden DFT vectors.  Bit-exact."""
import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from ntt_vectors import C0, LARGE_SUBSET, MODES, oracle_many, single, structured
from util import R, arr, golden, h, ints, random_fr_canonical

pytestmark = pytest.mark.gpu


def test_ntt_golden(zkg):
    for c in golden("ntt.json"):
        a = arr([h(x) for x in c["a"]], R)
        for inv in (0, 1):
            for coset in (0, 1):
                out = zkg.ntt(a, inverse=inv, coset=coset)
                assert ints(out, R) == [h(x) for x in c[f"out_inv{inv}_coset{coset}"]], (c["logn"], inv, coset)


@pytest.mark.parametrize("logn", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 21])
def test_ntt_vs_oracle(zkg, oracle, logn):
    a = random_fr_canonical(1 << logn, 0x5A4B4C41494D0003 + logn)       # any 4-limb values < r are valid Montgomery residues
    for inv in (0, 1):
        for coset in (0, 1):
            got = zkg.ntt(a, inverse=inv, coset=coset)
            exp = oracle.fft(a, inverse=inv, coset=coset)
            assert np.array_equal(got, exp), (logn, inv, coset)


def test_ntt_full_size_properties(zkg, oracle):
    """BASELINE config 3 size (2^20): round trips, linearity, and a spot-check of outputs against the definition."""
    n = 1 << 20
    a = random_fr_canonical(n, 0x5A4B4C41494D0003)
    b = random_fr_canonical(n, 0x5A4B4C41494D0013)
    fa = zkg.ntt(a)
    assert np.array_equal(zkg.ntt(fa, inverse=True), a)
    assert np.array_equal(zkg.ntt(zkg.ntt(a, coset=True), inverse=True, coset=True), a)
    sel = np.arange(0, n, n // 64)
    fb = zkg.ntt(b)
    # definition check on a 2^12 transform: out[k] = sum_j a[j] w^(jk), Horner in Python ints
    from util import from_limbs, MONT
    rinv = pow(MONT, -1, R)
    ai = [from_limbs(x) * rinv % R for x in a[: 1 << 12]]
    sub = zkg.ntt(a[: 1 << 12].copy())
    w12 = pow(pow(5, (R - 1) >> 28, R), 1 << 16, R)
    for k in (0, 1, 77, 4095):
        acc = 0
        for x in reversed(ai):
            acc = (acc * pow(w12, k, R) + x) % R
        assert from_limbs(sub[k]) * rinv % R == acc
    # full size against the oracle (serial radix-2, ~2 s)
    assert np.array_equal(fa, oracle.fft(a))
    assert np.array_equal(fb[sel], oracle.fft(b)[sel])


@pytest.mark.parametrize("logn", list(range(1, 21)))
def test_ntt_structured_inputs(zkg, oracle, logn):
    """The prover's kind of input, which uniformly random vectors never are: zeros (the output must be canonical zeros, never r), all r - 1,
    all Montgomery one, single entries at 0, 1, N/2 and N - 1, alternating 0 and r - 1, 0/1 bits, every 29-bit digit at its maximum, the
    top digit alone (tests/ntt_vectors.py), all four modes, bit-exact.  Reference: the definition on Python integers (oracle/pyref.py
    domain_fft) up to 2^12, the oracle's transform above; above 2^16 zeros plus the three of LARGE_SUBSET (all r - 1, the 0/1 bits, the
    digits of 2^253 - 1)."""
    import pyref
    n = 1 << logn
    vecs = structured(n)
    if logn > 16:
        vecs = {k: v for k, v in vecs.items() if k in LARGE_SUBSET or k == "zeros"}
    jobs = [(name, v, inv, coset) for name, v in vecs.items() for inv, coset in MODES]
    jobs = [j for j in jobs if j[0] != "zeros"] + [j for j in jobs if j[0] == "zeros"]
    todo = [j for j in jobs if j[0] != "zeros"]                      # (the transform of zeros needs no reference)
    if logn <= 12:
        exp = [arr(pyref.domain_fft(ints(v), inverse=bool(inv), coset=bool(coset))) for _, v, inv, coset in todo]
    else:
        exp = oracle_many(oracle, [(v, inv, coset) for _, v, inv, coset in todo])
    exp += [j[1] for j in jobs[len(todo):]]
    for (name, v, inv, coset), e in zip(jobs, exp):
        got = zkg.ntt(v, inverse=inv, coset=coset)
        if name == "zeros":
            assert not got.any(), (logn, inv, coset)
        assert np.array_equal(got, e), (logn, name, inv, coset)


# ---- 2^22, 2^23, 2^24: the splits with R = 8 in the radix-4 kernel.  The oracle's serial transform is too slow there; each property below
#      pins the whole output or samples of it to something already checked.
def _large_random(n, seed):
    a = np.random.default_rng(seed).integers(0, 1 << 63, (n, 4), dtype=np.uint64)        # uniform below 2^252 < r
    a[:, 3] >>= np.uint64(3)
    return a


def _omega(logn):
    return pow(pow(5, (R - 1) >> 28, R), 1 << (28 - logn), R)


def _closed_form(logn, j0, k, inv, coset, c=C0):
    """output k of the transform of c e_j0 (raw limbs in, raw out: the transform is linear)"""
    n = 1 << logn
    w = _omega(logn)
    if not inv:
        return c * pow(5, j0 * coset, R) * pow(w, j0 * k, R) % R
    return c * pow(w, -j0 * k, R) * pow(n, -1, R) * pow(5, -k * coset, R) % R


@pytest.mark.parametrize("logn", [22, 23, 24])
def test_ntt_large_single_entries_closed_form(zkg, logn):
    n = 1 << logn
    ks = sorted(set(int(x) for x in np.random.default_rng(logn).integers(0, n, 60)) | {0, 1, n // 2, n - 1})
    for j0 in (0, 1, n // 2, n - 1):
        a = single(n, j0)
        for inv, coset in MODES:
            got = zkg.ntt(a, inverse=inv, coset=coset)
            assert ints(got[ks]) == [_closed_form(logn, j0, k, inv, coset) for k in ks], (logn, j0, inv, coset)


@pytest.mark.parametrize("logn", [22, 23, 24])
def test_ntt_large_round_trips(zkg, logn):
    a = _large_random(1 << logn, 0x5A4B0000 + logn)
    assert np.array_equal(zkg.ntt(zkg.ntt(a), inverse=True), a)
    assert np.array_equal(zkg.ntt(zkg.ntt(a, coset=True), inverse=True, coset=True), a)


def _powers(zkg, base, count):
    """base^j for j < count (a power of two) as Montgomery limbs, by doubling on the 32-bit Fr path (zkg.field_op)"""
    out = arr([1], R)
    while out.shape[0] < count:
        m = out.shape[0]
        out = np.concatenate([out, zkg.field_op(1, 0, out, np.tile(arr([pow(base, m, R)], R), (m, 1)))])
    return out


@pytest.mark.parametrize("logn", [22, 23, 24])
def test_ntt_large_decimation_identity(zkg, logn):
    """The even and odd outputs of the size-2^n transform are the size-2^(n-1) transforms of (a_j + a_(j+N/2)) and (a_j - a_(j+N/2)) w^j —
    over the whole output, for the plain, the coset (a_(j+N/2) scaled by g^(N/2) first), the inverse (w^-1, halved) and the inverse coset
    transform (the inverse's halves, whose outputs the half-size transform scales by g^-k where the full one has g^-2k, g^-(2k+1)).  The
    halves are formed on the 32-bit Fr path; the smaller size is pinned by the oracle (2^21) or by this test one size down."""
    n = 1 << logn; hn = n >> 1
    a = _large_random(n, 0x5A4B1000 + logn)
    lo, hi = a[:hn], a[hn:]
    w = _omega(logn)
    wj = _powers(zkg, w, hn)
    ginv = pow(5, -1, R)
    gk = _powers(zkg, ginv, hn)                                                                   # g^-k: icoset's output scaling, g^-2k on the even outputs
    for inv, coset in MODES:
        hi_s = zkg.field_op(1, 0, hi, np.tile(arr([pow(5, hn, R)], R), (hn, 1))) if coset and not inv else hi
        tw = wj if not inv else np.concatenate([wj[:1], zkg.field_op(1, 6, wj[:0:-1])])          # w^-j = -w^(N/2 - j)
        s = zkg.field_op(1, 1, lo, hi_s); d = zkg.field_op(1, 0, zkg.field_op(1, 2, lo, hi_s), tw)
        if inv:
            half = np.tile(arr([pow(2, -1, R)], R), (hn, 1))
            s = zkg.field_op(1, 0, s, half); d = zkg.field_op(1, 0, d, half)
        full = zkg.ntt(a, inverse=inv, coset=coset)
        even, odd = zkg.ntt(s, inverse=inv, coset=coset), zkg.ntt(d, inverse=inv, coset=coset)
        if inv and coset:                                  # g^-2k = g^-k g^-k and g^-(2k+1) = g^-1 g^-k g^-k: one g^-k comes with the half-size transform
            even = zkg.field_op(1, 0, even, gk); odd = zkg.field_op(1, 0, zkg.field_op(1, 0, odd, gk), np.tile(arr([ginv], R), (hn, 1)))
        assert np.array_equal(full[0::2], even), (logn, inv, coset, "even")
        assert np.array_equal(full[1::2], odd), (logn, inv, coset, "odd")


_dense22 = {}


def _dense_2p22():
    """the random 2^22 vector of the round-trip test and its values as Python integers (made once)"""
    if not _dense22:
        a = _large_random(1 << 22, 0x5A4B0000 + 22)
        raw = a.tobytes()
        _dense22["a"] = a; _dense22["ints"] = [int.from_bytes(raw[32 * j:32 * j + 32], "little") for j in range(1 << 22)]
    return _dense22["a"], _dense22["ints"]


@pytest.mark.parametrize("inv,coset", MODES)
def test_ntt_2p22_outputs_by_definition(zkg, inv, coset):
    """two outputs of the 2^22 transform of a dense random vector against the definition, by Horner on Python integers: out[k] = sum_j a_j x^j
    at x = w^k (g w^k on the coset; w^-k, scaled by 1/N and g^-k, for the inverses)"""
    logn = 22; n = 1 << logn
    a, vals = _dense_2p22()
    w = _omega(logn); ninv = pow(n, -1, R)
    got = zkg.ntt(a, inverse=inv, coset=coset)
    for k in (1, 0x2A5F31):
        x = pow(w, -k if inv else k, R) * (pow(5, coset, R) if not inv else 1) % R
        acc = 0
        for v in reversed(vals):
            acc = (acc * x + v) % R
        if inv:
            acc = acc * ninv * pow(5, -k * coset, R) % R
        assert ints(got[k:k + 1])[0] == acc, (inv, coset, k)


def test_ntt_switches_agree_with_the_default_path(zkg):
    """ntt.hip keeps A/B switches (ZKG_NTT_32: the whole 32-bit kernel; ZKG_NTT_RADIX2; ZKG_NTT_NORM_STORES; ZKG_NTT_XCD; ZKG_NTT29_PAD) and
    two geometry aids (ZKG_NTT_TILE_LOG, ZKG_NTT_MAX_R), all read once.  Forced each way in a process of its own, the transforms of fixed
    vectors (a random one and the 0/1 bits) for n in 1..12, 18, 20 in all four modes are byte-identical (SHA-256 of the output bytes) to this
    process's default path, which the tests above pin to the oracle.  Every forced geometry was checked from ntt_run_ex for each listed n:
    the stage counts sum to n, rows x columns x tiles = N, the largest LDS tile is 80 KiB (ZKG_NTT29_PAD=1 at 2^20) under the 128 KiB that
    ntt_configure sets.  The last environment gives passes of at most 3 stages on 32-element tiles: multi-pass radix-4 with the odd tail."""
    import hashlib, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import hashlib, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import zklaim_amd as zkg
from ntt_vectors import MODES, bits
from util import random_fr_canonical
zkg.init(0)
for logn in list(range(1, 13)) + [18, 20]:
    for a in (random_fr_canonical(1 << logn, 0x5117C4 + logn), bits(1 << logn, logn)):
        for inv, coset in MODES:
            print("digest", logn, inv, coset, hashlib.sha256(zkg.ntt(a, inverse=inv, coset=coset).tobytes()).hexdigest())
zkg.shutdown()
'''
    from ntt_vectors import bits
    want = []
    for logn in list(range(1, 13)) + [18, 20]:
        for a in (random_fr_canonical(1 << logn, 0x5117C4 + logn), bits(1 << logn, logn)):
            for inv, coset in MODES:
                want.append(f"digest {logn} {inv} {coset} " + hashlib.sha256(zkg.ntt(a, inverse=inv, coset=coset).tobytes()).hexdigest())
    envs = [{"ZKG_NTT_32": "1"}, {"ZKG_NTT_RADIX2": "1"}, {"ZKG_NTT_RADIX2": "0"}, {"ZKG_NTT_NORM_STORES": "1"}, {"ZKG_NTT_XCD": "0"}, {"ZKG_NTT29_PAD": "1"},
            {"ZKG_NTT_MAX_R": "8", "ZKG_NTT_TILE_LOG": "9", "ZKG_NTT_RADIX2": "1", "ZKG_NTT_XCD": "0"},          # round 2's shape
            {"ZKG_NTT_MAX_R": "3", "ZKG_NTT_TILE_LOG": "5", "ZKG_NTT_RADIX2": "0"}]
    for env in envs:                                                     # one at a time; the first that fails ends the test
        r = subprocess.run([sys.executable, "-c", code, root], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
        assert r.returncode == 0, (env, r.stderr[-2000:])
        got = [l for l in r.stdout.splitlines() if l.startswith("digest ")]
        assert got == want, (env, [g for g, e in zip(got, want) if g != e][:4])
