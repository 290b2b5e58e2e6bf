"""CPU suite: the single-proof zklaim entry without a GPU.  k_zklaim_witness_par's device code compiled for the host
(zkg_zklaim_witness_mirror_parallel: the plain SHA-256 value pass, then every slice of the trace on its own from the derived plan, last
slice first) against the host witness pass and the serial mirror, byte for byte, up to the 64 payloads the generator serves; and
zkg_groth16_prove_zklaim's argument failures."""
import ctypes as C

import numpy as np
import pytest

from zklaim_witness_cases import KS_LARGE, N_SPECS, assert_same_witness, host_pass, large_cases, payloads


def _zkg():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    zklaim_amd.lib()
    return zklaim_amd


def test_names_are_declared_and_exported():
    zkg = _zkg()
    for name in ("zkg_groth16_prove_zklaim", "zkg_prove_zklaim_stats", "zkg_zklaim_witness_gpu_parallel", "zkg_zklaim_witness_mirror_parallel"):
        assert name in zkg.DECLARED_SYMBOLS and hasattr(zkg.lib(), name), name
    for name in ("prove_zklaim_stats", "zklaim_witness_gpu_parallel", "zklaim_witness_mirror_parallel"):
        assert callable(getattr(zkg, name))
    assert callable(zkg.Crs.prove_zklaim)


@pytest.mark.parametrize("k,specs", [(1, range(N_SPECS)), (3, range(N_SPECS)), (8, [0])])
def test_slices_in_reverse_order_equal_the_host_pass_and_the_serial_mirror(k, specs):
    zkg = _zkg()
    keep = []
    for spec in specs:
        ctx = zkg.make_ctx(payloads(k, spec), keep)
        got = zkg.zklaim_witness_mirror_parallel(ctx)
        assert_same_witness(got, host_pass(zkg, ctx), (k, spec, "host pass"))
        assert_same_witness(got, zkg.zklaim_witness_mirror(ctx), (k, spec, "serial mirror"))


@pytest.mark.parametrize("k", KS_LARGE)
def test_slices_equal_the_host_pass_at_large_counts(k):
    """more than one round of candidates (the mixed and banded credentials, the full-width pre-images, at 13 the sweeps over the 1 / c table)"""
    zkg = _zkg()
    cases = large_cases(zkg, k)
    assert {"mixed0", "random", "ones", "banded1"} <= set(cases) and (k != 13 or {"sweep", "sweep_reversed"} <= set(cases))
    for name, (ctx, want) in cases.items():
        got = zkg.zklaim_witness_mirror_parallel(ctx)
        assert_same_witness(got, want, (k, name, "host pass"))
        assert_same_witness(got, zkg.zklaim_witness_mirror(ctx), (k, name, "serial mirror"))


def test_broken_payload_list_is_an_error():
    zkg = _zkg()
    keep = []
    ctx = zkg.make_ctx(payloads(2, 0), keep)
    ctx.num_of_payloads = 3
    with pytest.raises(zkg.ZkgError):
        zkg.zklaim_witness_mirror_parallel(ctx)


def test_prove_zklaim_refuses_without_init_and_null_arguments():
    """no zkg_init in this process: whatever the arguments are, ZKG_ERROR, a message, and neither the proof nor its length is touched"""
    zkg = _zkg()
    L = zkg.lib()
    L.zkg_groth16_prove_zklaim.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    keep = []
    ctx = zkg.make_ctx(payloads(1, 0), keep)
    r = np.arange(1, 5, dtype=np.uint64); s = np.arange(5, 9, dtype=np.uint64)
    fake_crs = np.zeros(64, np.uint64)                                         # never dereferenced: the call stops at "not initialised"
    good = dict(crs=fake_crs.ctypes.data, ctx=C.addressof(ctx), r=r.ctypes.data, s=s.ctypes.data)
    for null in (None, "crs", "ctx", "r", "s", "out", "len"):
        out = np.full(256, 0xAB, np.uint8); ln = C.c_size_t(0xDEAD)
        a = dict(good, out=out.ctypes.data, len=C.addressof(ln))
        if null:
            a[null] = None
        L.zkg_last_error.restype = C.c_char_p
        rc = L.zkg_groth16_prove_zklaim(a["crs"], a["ctx"], a["r"], a["s"], 1, a["out"], a["len"])
        assert rc == zkg.ERROR, null
        assert b"zkg_groth16_prove_zklaim" in L.zkg_last_error(), null
        assert (out == 0xAB).all() and ln.value == 0xDEAD, null
        assert zkg.prove_zklaim_stats() == (0, 0)
