"""Credentials for the witness-generator tests: every op, attribute / reference pairs at the edges of the 64-bit range, an all-zero
pre-image and a hash that is not the pre-image's.  The witness passes do not ask whether the statement holds, so most of these are
false statements: what is compared is the witness, variable by variable."""
import numpy as np

M = 2 ** 64 - 1
H = 2 ** 63
OPS7 = ["less", "less_or_eq", "eq", "greater_or_eq", "greater", "not_eq", "noop"]
# (attribute, reference): 0, 1, 2^63, 2^64 - 1, equal, off by one in both directions, far apart
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1), (H, H), (H, H - 1), (H - 1, H), (M, M), (M, M - 1), (M - 1, M), (0, M), (M, 0), (H, 0), (1, H), (5, 5), (6, 5), (2, 1), (1, 2)]
N_SPECS = 10


def payloads(k, spec, variant=0):
    """k payloads of credential `spec` (0 .. N_SPECS - 1); variant changes the salts only"""
    out = []
    for i in range(k):
        salt = 0x9000 + 0x100 * spec + 0x10 * variant + i
        if spec < 7:                                               # every op on every kind of pair, rotating over attributes and payloads
            pairs = [PAIRS[(5 * spec + 7 * i + 3 * j) % len(PAIRS)] for j in range(5)]
            pl = dict(attrs=[a for a, _ in pairs], refs=[r for _, r in pairs], ops=[OPS7[(spec + i + j) % 7] for j in range(5)], salt=salt)
        elif spec == 7:                                            # all-zero pre-image (salt included), references zero: nothing but bits and zeros
            pl = dict(attrs=[0] * 5, refs=[0] * 5, ops=["eq"] * 5, salt=0)
        elif spec == 8:                                            # a hash that is not SHA-256(pre), on the first payload
            pl = dict(attrs=[1990 + i, 7, 42, i, 5], refs=[2100, 7, 41, 0, 5], ops=["less", "eq", "greater", "noop", "greater_or_eq"], salt=salt)
            if i == 0:
                pl["hash"] = bytes((0xA5 + b) & 0xFF for b in range(32))
        else:                                                      # attributes and references that are 0 or 1: packed values tagged 0 / 1, not listed
            pl = dict(attrs=[1, 0, 1, 0, 1], refs=[1, 1, 0, 0, 1], ops=["eq", "less", "greater", "eq", "less_or_eq"], salt=salt)
        out.append(pl)
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
