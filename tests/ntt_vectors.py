"""Structured NTT inputs shared by the GPU transform tests, and the oracle's transforms of several vectors side by side.

The prover's transform inputs are the A, B, C evaluations of a SHA-256 circuit: almost all Montgomery zeros and ones, nothing like the
uniformly random vectors.  Vectors here are raw ABI limbs ((n, 4) uint64, any value below r is a valid Montgomery residue); the transforms
are linear, so a reference on Python integers takes the raw values as they are."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from util import R, MONT, arr

MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]                     # (inverse, coset)
ONE = MONT % R                                               # Montgomery one, raw
ALL_DIGITS_232 = (1 << 232) - 1                              # every 29-bit digit below the top one at its maximum
ALL_DIGITS_253 = (1 << 253) - 1                              # ... and the top digit's 21 low bits too (the largest such value below r)
TOP_DIGIT = ((R >> 232) - 1) << 232                          # only the top digit set, as large as it gets below r
C0 = 0x1d2c3b4a5968778695a4b3c2d1e0f00112233445566778899aabbccddeeff123 % R     # the single entries' value
BIT_DENSITY = 0.25                                           # share of ones in the 0/1 vector.  Measured on the one-payload credential circuit (27653 rows, its
#                                                              own witness): ones are 23 % of the A, 49 % of the B and 4 % of the C evaluations (zeros 54 %, 48 %, 83 %;
#                                                              the rest other values) - a quarter on average


def fill(n, v):
    return np.tile(arr([v]), (n, 1))


def bits(n, seed):
    out = np.zeros((n, 4), np.uint64)
    out[np.random.default_rng(seed).random(n) < BIT_DENSITY] = arr([ONE])[0]
    return out


def single(n, j, v=C0):
    out = np.zeros((n, 4), np.uint64)
    out[j] = arr([v])[0]
    return out


def structured(n):
    """name -> vector, every family of the list"""
    alt = fill(n, R - 1); alt[0::2] = 0
    v = {"zeros": fill(n, 0), "all r-1": fill(n, R - 1), "all one": fill(n, ONE), "alternating 0, r-1": alt, "bits": bits(n, 0xB175 + n),
         "digits 2^232-1": fill(n, ALL_DIGITS_232), "digits 2^253-1": fill(n, ALL_DIGITS_253), "top digit": fill(n, TOP_DIGIT)}
    for j in sorted({0, 1, n // 2, n - 1}):
        v[f"single at {j}"] = single(n, j)
    return v


LARGE_SUBSET = ("all r-1", "bits", "digits 2^253-1")         # above 2^16: the three that put the most limbs at their bounds, and the prover's kind


def oracle_many(oracle, jobs, workers=12):
    """[(vector, inverse, coset)] -> the oracle's transforms, several at a time (the library call releases the interpreter lock)"""
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(lambda j: oracle.fft(j[0], inverse=j[1], coset=j[2]), jobs))
