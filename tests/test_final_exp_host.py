"""CPU suite: the device's final exponentiation (csrc/final_exp.hip.hpp) compiled for the host, zkg_final_exp(where=2), against its
specification, host/pairing.hpp's final_exponentiation (where=0): byte for byte.  Neither needs a GPU or zkg_init.  The kernel itself
(where=1), zkg_groth16_verify_each and zkg_pairing_each have no CPU path: without a GPU they fail loudly."""
import random

import numpy as np
import pytest

from util import MONT, Q

ONE = (MONT % Q).to_bytes(32, "little") + b"\0" * 352


def fq12_bytes(coeffs):
    """12 canonical Montgomery limbs values (ints < q), in the tower's order c0.c0.c0, c0.c0.c1, c0.c1.c0, .. c1.c2.c1"""
    assert len(coeffs) == 12
    return b"".join(int(c).to_bytes(32, "little") for c in coeffs)


def final_exp_inputs(n_random=8, seed=0xFE):
    rng = random.Random(seed)
    rnd = lambda: rng.randrange(Q)                                              # noqa: E731
    vals = [ONE]
    vals += [fq12_bytes([rnd() for _ in range(12)]) for _ in range(n_random)]
    vals += [fq12_bytes([rnd() for _ in range(6)] + [0] * 6) for _ in range(3)]            # c1 = 0 (an element of Fq6)
    vals += [fq12_bytes([0] * 6 + [rnd() for _ in range(6)])]                              # c0 = 0
    vals += [fq12_bytes([0] * k + [rnd()] + [0] * (11 - k)) for k in (0, 1, 7, 11)]        # one coefficient
    vals += [fq12_bytes([Q - 1] * 12)]                                                      # the largest canonical limbs
    return vals


@pytest.fixture(scope="module")
def zk():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    return zklaim_amd


def test_device_code_on_host_equals_the_specification(zk):
    vals = final_exp_inputs()
    spec = zk.final_exp(vals, 0)
    assert zk.final_exp(vals, 2) == spec
    assert spec[0] == ONE                                                       # FE(1) = 1
    assert all(v != ONE for v in spec[1:9])
    assert spec[9:12] == [ONE] * 3                                              # x in Fq6: x^(q^6 - 1) = 1
    # values that are already in GT (outputs of the specification): raised once more
    assert zk.final_exp(spec, 2) == zk.final_exp(spec, 0)
    # one at a time gives the same as all at once
    assert [zk.final_exp([v], 2)[0] for v in vals[:4]] == spec[:4]
    assert zk.final_exp([], 0) == [] and zk.final_exp([], 2) == []


def test_a_value_does_not_depend_on_its_neighbours(zk):
    vals = final_exp_inputs(3, 0xA1)
    a = zk.final_exp(vals, 2)
    b = zk.final_exp(list(reversed(vals)), 2)
    assert a == list(reversed(b))


@pytest.mark.parametrize("where", [0, 2])
def test_bad_elements_are_refused(zk, where):
    good = final_exp_inputs(1)[1]
    with pytest.raises(zk.ZkgError):
        zk.final_exp([b"\0" * 384], where)                                      # zero has no inverse
    with pytest.raises(zk.ZkgError):
        zk.final_exp([good, b"\0" * 384], where)
    for k in (0, 5, 11):
        bad = bytearray(good); bad[32 * k:32 * k + 32] = Q.to_bytes(32, "little")          # a coefficient == q
        with pytest.raises(zk.ZkgError):
            zk.final_exp([bytes(bad)], where)
        bad[32 * k:32 * k + 32] = b"\xff" * 32
        with pytest.raises(zk.ZkgError):
            zk.final_exp([bytes(bad)], where)
    with pytest.raises(zk.ZkgError):
        zk.final_exp([good], 3)
    with pytest.raises(zk.ZkgError):
        zk.final_exp([good[:-1]], where)


def test_device_entries_need_a_gpu(zk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(zk.ZkgError):
        zk.init(0)
    with pytest.raises(zk.ZkgError):
        zk.final_exp([ONE], 1)
    with pytest.raises(zk.ZkgError):
        zk.final_exp([], 1)
    with pytest.raises(zk.ZkgError):
        zk.groth16_verify_each([(b"\0" * 600, np.zeros((1, 4), np.uint64), b"\0" * 134)])
    with pytest.raises(zk.ZkgError):
        zk.groth16_verify_each([])
    with pytest.raises(zk.ZkgError):
        zk.pairing_each(np.zeros((1, 8), np.uint64), np.zeros((1, 16), np.uint64), 1)
    with pytest.raises(zk.ZkgError):
        zk.pairing_each(np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64), 1)
    assert zk.verify_each_stats() == (0, 0, 0)
