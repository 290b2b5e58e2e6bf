"""GPU parity: zkg_groth16_setup_resident, the generator that leaves its key on the device.  Under a fixed trapdoor its blobs are the host
generator's byte for byte (radix-2 and step domain, swap both ways, a real one-payload zklaim circuit, a system without an L query, a B that
touches the constant alone); its counters say that every scalar was made on the device and nothing was uploaded; the zkg_crs it returns
proves byte for byte what the key loaded from the blob and the key uploaded from host arrays prove; a t on the domain makes no key and
leaves the out-pointers alone; two threads generate at once."""
import ctypes as C
import threading

import numpy as np
import pytest

from gpu_util import zkg  # noqa: F401
from qap_instance_systems import log10_system, step_system
from util import R, arr, limbs, random_fr_canonical

pytestmark = pytest.mark.gpu

TD = random_fr_canonical(5, 0x5E7)
RS = random_fr_canonical(2, 0x5E8)
_BASES, _SYSTEMS, _HOST = {}, {}, {}
KINDS = ["log10", "log10_swapped", "step", "step_swapped", "zklaim"]


def system(zkg, kind):
    """(cs, n, l, witness, keep), made once"""
    if kind not in _SYSTEMS:
        keep = []
        if kind == "zklaim":
            ck = zkg.ZklaimCircuit(zkg.make_ctx([dict(attrs=[5, 6, 7, 8, 9], refs=[5, 0, 0, 0, 0], ops=["eq", "noop", "noop", "noop", "noop"], salt=9)], keep))
            keep.append(ck)
            _SYSTEMS[kind] = (ck.r1cs, ck.r1cs.num_variables, ck.r1cs.num_inputs, ck.witness(), keep)
        else:
            base = kind.split("_")[0]
            if base not in _BASES:
                _BASES[base] = log10_system() if base == "log10" else step_system()
            n, l, A, B, Cm, w = _BASES[base]
            if kind == "log10_no_l":                                    # every variable an input: n = l, the L query is empty
                l = n
            elif kind == "log10_b_constant":                            # B = the constant in every row: its non-zero list is [0]
                rows = len(B[0]) - 1
                B = (np.arange(rows + 1, dtype=np.uint32), np.zeros(rows, np.uint32), np.tile(arr([1], R), (rows, 1)))
            elif kind.endswith("_swapped"):
                A, B = B, A
            _SYSTEMS[kind] = (zkg.make_r1cs(n, l, A, B, Cm, keep), n, l, w, keep)
    return _SYSTEMS[kind]


def host_key(zkg, kind):
    """the host generator's (pk_blob, vk_blob, swapped) under TD, made once"""
    if kind not in _HOST:
        kp = zkg.Keypair(system(zkg, kind)[0], TD)
        try:
            _HOST[kind] = (kp.pk_blob(), kp.vk_blob(), kp.swapped)
        finally:
            kp.free()
    return _HOST[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_blobs_stats_and_the_returned_key(zkg, kind):
    cs, n, l, w, _ = system(zkg, kind)
    want_pk, want_vk, swapped = host_key(zkg, kind)
    assert swapped == (kind.endswith("_swapped") or kind == "zklaim")  # (the gadget circuit's B touches more variables than its A)
    pk_blob, vk_blob, crs = zkg.groth16_setup_resident(cs, TD)
    stats = zkg.setup_resident_stats()
    try:
        assert vk_blob == want_vk
        assert pk_blob == want_pk
        info = zkg.pk_blob_inspect(pk_blob)
        assert info["domain_size"] == {"log10": 1 << 10, "step": (1 << 12) + (1 << 6), "zklaim": 1 << 15}[kind.split("_")[0]]
        assert stats == [1, info["B_values"], 0] and 0 < info["B_values"] < n + 1
        # the resident key against the same key loaded from the blob and uploaded from the host generator's arrays
        rc, proof = crs.prove(w, RS[0], RS[1])
        assert rc == 0 and len(proof) == 134
        loaded = zkg.Crs(blob=pk_blob)
        try:
            assert loaded.prove(w, RS[0], RS[1]) == (0, proof)
        finally:
            loaded.free()
        kp = zkg.Keypair(cs, TD)
        try:
            uploaded = zkg.Crs(pk=kp.pk)
            try:
                assert uploaded.prove(w, RS[0], RS[1]) == (0, proof)
            finally:
                uploaded.free()
        finally:
            kp.free()
        assert zkg.groth16_verify(vk_blob, w[:l], proof) == 0
        bad = bytearray(proof); bad[50] ^= 4
        assert zkg.groth16_verify(vk_blob, w[:l], bytes(bad)) != 0
    finally:
        crs.free()


def test_without_a_handle_the_blobs_are_the_same(zkg):
    cs = system(zkg, "step")[0]
    pk_blob, vk_blob, crs = zkg.groth16_setup_resident(cs, TD, want_crs=False)
    assert crs is None
    assert (pk_blob, vk_blob) == host_key(zkg, "step")[:2]
    assert zkg.setup_resident_stats() == [1, zkg.pk_blob_inspect(pk_blob)["B_values"], 0]


def test_a_trapdoor_with_t_on_the_domain_makes_no_key(zkg):
    cs = system(zkg, "log10")[0]
    td = TD.copy(); td[0] = limbs(1)                                    # t = 1 = omega^0
    L = zkg.lib()
    L.zkg_groth16_setup_resident.argtypes = [C.c_void_p] * 7
    pk = C.c_void_p(None); vk = C.c_void_p(None); crs = C.c_void_p(None); pk_len = C.c_size_t(0); vk_len = C.c_size_t(0)
    assert L.zkg_groth16_setup_resident(C.byref(cs), td.ctypes.data, C.byref(pk), C.byref(pk_len), C.byref(vk), C.byref(vk_len), C.byref(crs)) == zkg.ERROR
    msg = L.zkg_last_error().decode()
    assert "zkg_groth16_setup_resident" in msg and "domain point" in msg
    assert not pk.value and not vk.value and not crs.value and pk_len.value == 0 and vk_len.value == 0
    with pytest.raises(zkg.ZkgError) as e:
        zkg.groth16_setup_resident(cs, td)
    assert "zkg_groth16_setup_resident" in str(e.value)
    pk_blob, _, _ = zkg.groth16_setup_resident(cs, TD, want_crs=False)      # and the next call is not disturbed
    assert pk_blob == host_key(zkg, "log10")[0]


@pytest.mark.parametrize("kind", ["log10_no_l", "log10_b_constant"])
def test_an_empty_l_query_and_a_b_that_touches_the_constant_alone(zkg, kind):
    cs, n, l, _, _ = system(zkg, kind)
    pk_blob, vk_blob, _ = zkg.groth16_setup_resident(cs, TD, want_crs=False)
    stats = zkg.setup_resident_stats()
    assert (pk_blob, vk_blob) == host_key(zkg, kind)[:2]
    info = zkg.pk_blob_inspect(pk_blob)
    if kind == "log10_no_l":
        assert n == l and info["L_query"] == 0
    else:
        assert not host_key(zkg, kind)[2] and info["B_values"] == 1
    assert stats == [1, info["B_values"], 0]


def test_two_threads_generate_different_systems_at_once(zkg):
    kinds = ("log10", "step")
    want = {k: host_key(zkg, k) for k in kinds}
    systems = {k: system(zkg, k) for k in kinds}
    zkg.lib().zkg_prover_peak_in_flight(1)
    got, errors = {}, []
    barrier = threading.Barrier(2)

    def run(kind):
        try:
            cs, n, l, w, _ = systems[kind]
            barrier.wait(timeout=60)
            out = []
            for _ in range(2):                                          # the second one meets the first one's keypair on the discard thread
                pk_blob, vk_blob, crs = zkg.groth16_setup_resident(cs, TD)
                stats = zkg.setup_resident_stats()                      # the calling thread's own
                try:
                    rc, proof = crs.prove(w, RS[0], RS[1])
                finally:
                    crs.free()
                out.append((pk_blob, vk_blob, stats, rc, zkg.groth16_verify(vk_blob, w[:l], proof)))
            got[kind] = out
        except Exception as e:  # noqa: BLE001
            errors.append((kind, repr(e)))

    threads = [threading.Thread(target=run, args=(k,)) for k in kinds]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors and not any(t.is_alive() for t in threads), errors
    for k in kinds:
        for pk_blob, vk_blob, stats, rc, verdict in got[k]:
            assert (pk_blob, vk_blob) == want[k][:2], k
            assert stats == [1, zkg.pk_blob_inspect(pk_blob)["B_values"], 0] and rc == 0 and verdict == 0, k
    assert zkg.lib().zkg_prover_peak_in_flight(1) == 1                  # each key only ever had its own caller's one proof in flight
