"""GPU parity: zkg_groth16_setup_dev, the generator whose scalars stay on the device (zkg_qap_instance_async at t, the powers kernel for
t^i Z(t) / delta, one kernel for the IC and L combinations).  Against the oracle's generator on a radix-2 and a step system, swap flag both
ways; against zkg_groth16_setup under the same trapdoor, arrays and blobs byte for byte (the check on IC and gamma, which live in the vk), on
those systems and a real one-payload zklaim circuit; a proof under the device-made key; a trapdoor whose t lies on the domain."""
import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from qap_instance_systems import log10_system, step_system
from util import limbs, random_fr_canonical

pytestmark = pytest.mark.gpu

TD = random_fr_canonical(5, 0x5E7)
_CACHE = {}


def pk_arrays(kp, n, l, m):
    return {name: kp.array(name, count, lim) for name, count, lim in (("A_query", n + 1, 8), ("B_g1", n + 1, 8), ("B_g2", n + 1, 16), ("H_query", m - 1, 8),
            ("L_query", n - l, 8), ("alpha_g1", 1, 8), ("beta_g1", 1, 8), ("delta_g1", 1, 8), ("beta_g2", 1, 16), ("delta_g2", 1, 16))}


def system(kind):
    """(n, l, A, B, C, witness), made once"""
    if kind not in _CACHE:
        _CACHE[kind] = log10_system() if kind == "log10" else step_system()
    return _CACHE[kind]


@pytest.mark.parametrize("kind", ["log10", "step"])
def test_dev_key_equals_the_oracle_and_swaps_as_the_generator_does(zkg, oracle, kind):
    """A of these systems touches more variables than B: as given nothing is exchanged, with A and B exchanged the generator swaps them back —
    either way the key is the oracle's on the system with the larger side in A"""
    n, l, A, B, C, _ = system(kind)
    keep = []
    want = oracle.groth16_setup(oracle.make_r1cs(n, l, A, B, C, keep), TD)
    m = want["m"]
    assert m == ((1 << 10) if kind == "log10" else (1 << 12) + (1 << 6))
    for a, b, swapped in ((A, B, False), (B, A, True)):
        kp = zkg.Keypair(zkg.make_r1cs(n, l, a, b, C, keep), TD, dev=True)
        try:
            assert kp.swapped == swapped
            for name, got in pk_arrays(kp, n, l, m).items():
                assert np.array_equal(got.reshape(-1), want[name].reshape(-1)), (name, swapped)
        finally:
            kp.free()


def _same_key(zkg, cs, n, l):
    host, dev = zkg.Keypair(cs, TD), zkg.Keypair(cs, TD, dev=True)
    try:
        m = host.pk.domain_size
        assert dev.pk.domain_size == m and dev.pk.log_m == host.pk.log_m and dev.swapped == host.swapped
        want = pk_arrays(host, n, l, m)
        for name, got in pk_arrays(dev, n, l, m).items():
            assert np.array_equal(got, want[name]), name
        assert dev.vk_blob() == host.vk_blob()                          # gamma_g2 and the IC points live here alone
        assert dev.pk_blob() == host.pk_blob()
        return m
    finally:
        host.free(); dev.free()


@pytest.mark.parametrize("kind", ["log10", "step"])
def test_dev_key_equals_the_existing_generator(zkg, kind):
    n, l, A, B, C, _ = system(kind)
    keep = []
    _same_key(zkg, zkg.make_r1cs(n, l, A, B, C, keep), n, l)
    _same_key(zkg, zkg.make_r1cs(n, l, B, A, C, keep), n, l)            # the swapping side


def test_dev_key_equals_the_existing_generator_on_a_zklaim_circuit(zkg):
    """one payload: 27.7k constraints, m = 2^15, packing rows of 253 terms and the constant's column with a term of every bitness row"""
    keep = []
    ck = zkg.ZklaimCircuit(zkg.make_ctx([dict(attrs=[5, 6, 7, 8, 9], refs=[5, 0, 0, 0, 0], ops=["eq", "noop", "noop", "noop", "noop"], salt=9)], keep))
    assert _same_key(zkg, ck.r1cs, ck.r1cs.num_variables, ck.r1cs.num_inputs) == 1 << 15


def test_a_proof_under_the_dev_key_is_accepted(zkg):
    n, l, A, B, C, w = system("log10")
    keep = []
    kp = zkg.Keypair(zkg.make_r1cs(n, l, A, B, C, keep), TD, dev=True)
    crs = zkg.Crs(blob=kp.pk_blob(), m=kp.pk.domain_size)
    try:
        rs = random_fr_canonical(2, 0x5E8)
        rc, proof = crs.prove(w, rs[0], rs[1])
        assert rc == 0
        assert zkg.groth16_verify(kp.vk_blob(), w[:l], proof) == 0
        bad = bytearray(proof); bad[50] ^= 4
        assert zkg.groth16_verify(kp.vk_blob(), w[:l], bytes(bad)) != 0
    finally:
        crs.free(); kp.free()


def test_a_trapdoor_with_t_on_the_domain_makes_no_key(zkg):
    n, l, A, B, C, _ = system("log10")
    keep = []
    td = TD.copy(); td[0] = limbs(1)                                    # t = 1 = omega^0
    with pytest.raises(zkg.ZkgError) as e:
        zkg.Keypair(zkg.make_r1cs(n, l, A, B, C, keep), td, dev=True)
    assert "zkg_groth16_setup_dev" in str(e.value) and "domain point" in str(e.value)
    assert zkg.lib().zkg_last_error().decode()
