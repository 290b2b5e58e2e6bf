"""Credentials for the witness-generator tests: every op, attribute / reference pairs at the edges of the 64-bit range, an all-zero
pre-image and a hash that is not the pre-image's.  The witness passes do not ask whether the statement holds, so most of these are
false statements: what is compared is the witness, variable by variable.

Above eight payloads the item workgroup compacts its candidates in more than one round of 256 (KS_LARGE): mixed_payloads and
banded_payloads make credentials whose rounds differ from each other, cnt_sweep_payloads reads every entry of the 1 / c table, and
large_cases keeps each of those credentials with its host pass for every test module of the run."""
import numpy as np

M = 2 ** 64 - 1
H = 2 ** 63
OPS7 = ["less", "less_or_eq", "eq", "greater_or_eq", "greater", "not_eq", "noop"]
# (attribute, reference): 0, 1, 2^63, 2^64 - 1, equal, off by one in both directions, far apart
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1), (H, H), (H, H - 1), (H - 1, H), (M, M), (M, M - 1), (M - 1, M), (0, M), (M, 0), (H, 0), (1, H), (5, 5), (6, 5), (2, 1), (1, 2)]
N_SPECS = 12
SPEC_ZERO, SPEC_RANDOM, SPEC_ONES = 7, 10, 11
# payload counts that put a boundary between two rounds of 256 candidates inside every class of candidate (candidate_classes)
KS_LARGE = [9, 13, 20, 37, 64]
ROUND = 256                                                        # candidates per round of the item workgroup


def payload(i, spec, variant=0):
    """payload i of credential `spec` (0 .. N_SPECS - 1); variant changes the salts only (spec SPEC_RANDOM: all of the pre-image)"""
    salt = 0x9000 + 0x100 * spec + 0x10 * variant + i
    if spec < 7:                                                   # every op on every kind of pair, rotating over attributes and payloads
        pairs = [PAIRS[(5 * spec + 7 * i + 3 * j) % len(PAIRS)] for j in range(5)]
        return dict(attrs=[a for a, _ in pairs], refs=[r for _, r in pairs], ops=[OPS7[(spec + i + j) % 7] for j in range(5)], salt=salt)
    if spec == SPEC_ZERO:                                          # all-zero pre-image (salt included), references zero: nothing but bits and zeros
        return dict(attrs=[0] * 5, refs=[0] * 5, ops=["eq"] * 5, salt=0)
    if spec == 8:                                                  # a hash that is not SHA-256(pre), on the first payload
        pl = dict(attrs=[1990 + i, 7, 42, i, 5], refs=[2100, 7, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=salt)
        if i == 0:
            pl["hash"] = bytes((0xA5 + b) & 0xFF for b in range(32))
        return pl
    if spec == 9:                                                  # attributes and references that are 0 or 1: packed values tagged 0 / 1, not listed
        return dict(attrs=[1, 0, 1, 0, 1], refs=[1, 1, 0, 0, 1], ops=["eq", "less", "greater", "eq", "less_or_eq"], salt=salt)
    if spec == SPEC_RANDOM:                                        # full-width attributes, references and salt: no byte of the pre-image is zero by design
        x = [int(v) for v in np.random.default_rng([0x2C1A, variant, i]).integers(0, 2 ** 64, 11, dtype=np.uint64)]
        return dict(attrs=x[:5], refs=x[5:10], ops=[OPS7[(i + j) % 7] for j in range(5)], salt=x[10])
    assert spec == SPEC_ONES                                       # every bit of the pre-image set; references on both sides of it
    return dict(attrs=[M] * 5, refs=[M, 0, M - 1, H, 1], ops=[OPS7[(i + 2 * j) % 7] for j in range(5)], salt=M)


def payloads(k, spec, variant=0):
    """k payloads of credential `spec`"""
    return [payload(i, spec, variant) for i in range(k)]


def mixed_payloads(k, variant=0):
    """payload i takes spec (i + variant) % N_SPECS: neighbouring candidates of one class come from different specs, so listed and
    unlisted ones alternate in runs of a few inside every wavefront"""
    return [payload(i, (i + variant) % N_SPECS, variant) for i in range(k)]


def banded_payloads(k, variant=0):
    """three quarters of the payloads are the all-zero one (the last ones for variant 0, the first ones for variant 1), the rest rotate as
    in mixed_payloads.  An all-zero payload lists nothing among data, plvars and refvals: at 37 payloads whole wavefronts, and at 64 whole
    rounds, list nothing between rounds that list most of their candidates."""
    band = range(k // 4, k) if variant % 2 == 0 else range(0, k - k // 4)
    return [payload(i, SPEC_ZERO if i in band else (i + variant) % N_SPECS, variant) for i in range(k)]


def cnt_sweep_payloads(reverse=False):
    """13 payloads whose 65 (attribute, reference) pairs give popcount((ref - attr) mod 2^64) = 0, 1, .., 64 (64, .., 0 if reverse): the
    comparisons' inv variables are the entries 0 .. 64 of the 1 / c table, each read once"""
    pairs = [(0, 2 ** c - 1) for c in range(64)] + [(1, 0)]
    assert [bin((r - a) % 2 ** 64).count("1") for a, r in pairs] == list(range(65))
    if reverse:
        pairs.reverse()
    return [dict(attrs=[a for a, _ in pairs[5 * i:5 * i + 5]], refs=[r for _, r in pairs[5 * i:5 * i + 5]], ops=[OPS7[(5 * i + j) % 7] for j in range(5)],
                 salt=0xC0DE00 + i) for i in range(13)]


def honest_payloads(k):
    """k payloads whose statements all hold, every op among them, with full-width attributes and salts"""
    out = []
    for i in range(k):
        a = [H + 1990 + i, 7 * i, M - i, i, 5]
        refs = [M, 7 * i, M - i - 1, 0, 5]; ops = ["less", "eq", "greater", "noop", "greater_or_eq"]
        if i % 2:
            refs = [a[0], 7 * i + 1, M - i - 1, 12345, 5]; ops = ["less_or_eq", "not_eq", "greater_or_eq", "noop", "eq"]
        out.append(dict(attrs=a, refs=refs, ops=ops, salt=M - 0x5A4B * (i + 1)))
    return out


def host_pass(zkg, ctx):
    """zkg_zklaim_witness_new + zkg_circuit_sparse_witness"""
    ck = zkg.ZklaimCircuit(ctx, witness_only=True)
    try:
        return ck.sparse_witness()
    finally:
        ck.free()


def assert_same_witness(got, want, what):
    assert got is not None, what
    for name, g, w in zip(("tags", "listed indices", "listed values"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, np.flatnonzero(np.asarray(g).reshape(len(g), -1) != np.asarray(w).reshape(len(w), -1))[:8])


# ---- the candidates of a k-payload credential, from the circuit's allocation order alone (nothing here reads the generator's header)

def candidate_classes(k):
    """the cumulative ends of the candidate classes in index order: input_fe, data, plvars, refvals, alpha_packed / inv"""
    n_inputs = -(-1280 * k // 253)
    return dict(input_fe=n_inputs, data=n_inputs + 5 * k, plvars=n_inputs + 11 * k, refvals=n_inputs + 19 * k, alpha_inv=n_inputs + 29 * k)


# k -> the classes that hold a candidate q = 256 j, j >= 1 (a class that holds two of them is named twice)
BOUNDARIES = {9: ["alpha_inv"], 13: ["refvals"], 20: ["plvars", "alpha_inv"], 37: ["data", "plvars", "refvals", "alpha_inv"],
              64: ["input_fe", "data", "plvars", "plvars", "refvals", "refvals", "alpha_inv", "alpha_inv"]}


def boundary_classes(k):
    ends = candidate_classes(k)
    return [next(name for name, end in ends.items() if q < end) for q in range(ROUND, ends["alpha_inv"], ROUND)]


def candidate_positions(k, n):
    """the tag index of every candidate of a k-payload circuit of n variables, in candidate order (ascending), and the slice of the inv ones"""
    e = candidate_classes(k)
    fixed = e["input_fe"] + 1 + (15 + 6 + 8 + 64 + 1280 + 384) * k            # inputs, zero, (data, less, less_or_eq), plvars, refvals, opsvals, public bits, r_bits
    per, rest = divmod(n - fixed, k)
    assert rest == 0 and per > 5 * 67, (k, n)
    o_dll = e["input_fe"] + 1; o_pl = o_dll + 15 * k; o_ref = o_pl + 6 * k; o_seg = fixed
    cmp_at = (o_seg + per * np.arange(k)[:, None] + 67 * np.arange(5)[None, :]).reshape(-1)        # comparison j of payload i: 64 bits, packed, not_all_zeros, inv
    pos = np.concatenate([np.arange(e["input_fe"]), o_dll + 3 * np.arange(5 * k), o_pl + np.arange(6 * k), o_ref + np.arange(8 * k),
                          np.stack([cmp_at + 64, cmp_at + 66], 1).reshape(-1)])
    assert len(pos) == e["alpha_inv"] and (np.diff(pos) > 0).all()
    return pos, slice(e["refvals"] + 1, None, 2)


def listed_per_round(k, want):
    """how many candidates each round of 256 lists, and the fewest / most that any window of 256 consecutive candidates lists"""
    pos, _ = candidate_positions(k, want[0].size)
    is_listed = want[0][pos] == 2
    assert int(is_listed.sum()) == want[1].size and np.array_equal(pos[is_listed], want[1])      # nothing but candidates is listed
    c = np.concatenate([[0], np.cumsum(is_listed)])
    windows = c[ROUND:] - c[:-ROUND]
    return [int(is_listed[q:q + ROUND].sum()) for q in range(0, len(pos), ROUND)], int(windows.min()), int(windows.max())


_LARGE = {}


def large_cases(zkg, k):
    """name -> (context, host pass) of the k-payload credentials the large-count tests share; each host pass is computed once per run.
    Nobody writes to what this returns."""
    if k not in _LARGE:
        keep = []
        made = dict(mixed0=mixed_payloads(k, 0), random=payloads(k, SPEC_RANDOM, k), ones=payloads(k, SPEC_ONES), banded1=banded_payloads(k, 1))
        if k == 13:
            made.update(sweep=cnt_sweep_payloads(), sweep_reversed=cnt_sweep_payloads(reverse=True))
        if k == KS_LARGE[-1]:
            made.update(banded0=banded_payloads(k, 0))
        out = {}
        for name, pls in made.items():
            ctx = zkg.make_ctx(pls, keep)
            out[name] = (ctx, host_pass(zkg, ctx))
        _LARGE[k] = (out, keep)
    return _LARGE[k][0]
