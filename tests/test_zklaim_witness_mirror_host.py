"""CPU suite: the device witness generator's gate-by-gate mirror, compiled for the host (zkg_zklaim_witness_mirror), against the host
witness pass (zkg_zklaim_witness_new + zkg_circuit_sparse_witness): tags, listed indices and listed values byte for byte."""
import pytest

from zklaim_witness_cases import N_SPECS, assert_same_witness, host_pass, payloads

KS = [1, 2, 3, 5, 8]


def _zkg():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    zklaim_amd.lib()
    return zklaim_amd


def test_names_are_declared_and_exported():
    zkg = _zkg()
    for name in ("zkg_groth16_prove_batch_zklaim", "zkg_zklaim_witness_gpu", "zkg_zklaim_witness_mirror", "zkg_zklaim_witness_stats", "zkg_zklaim_witness_size"):
        assert name in zkg.DECLARED_SYMBOLS and hasattr(zkg.lib(), name), name
    for name in ("zklaim_witness_gpu", "zklaim_witness_mirror", "zklaim_witness_stats"):
        assert callable(getattr(zkg, name))
    assert callable(zkg.Crs.prove_batch_zklaim)


@pytest.mark.parametrize("k", KS)
def test_mirror_equals_host_pass(k):
    zkg = _zkg()
    keep = []
    listed = set()
    for spec in range(N_SPECS):
        ctx = zkg.make_ctx(payloads(k, spec), keep)
        want = host_pass(zkg, ctx)
        got = zkg.zklaim_witness_mirror(ctx)
        assert zkg.zklaim_witness_size(k)[0] == want[0].size
        assert_same_witness(got, want, (k, spec))
        assert want[1].size <= zkg.zklaim_witness_size(k)[1]
        listed.add(int(want[1].size))
    assert len(listed) >= 2, "the value-dependent tagging (a packed 0 or 1 is not listed) was not exercised"


@pytest.mark.parametrize("k", KS)
def test_serial_host_pass_gives_the_same(k, monkeypatch):
    zkg = _zkg()
    keep = []
    for spec in (0, 3, 7, 8, 9):
        ctx = zkg.make_ctx(payloads(k, spec), keep)
        got = zkg.zklaim_witness_mirror(ctx)
        assert_same_witness(got, host_pass(zkg, ctx), (k, spec, "pool"))
        monkeypatch.setenv("ZKG_SERIAL_CIRCUIT", "1")
        assert_same_witness(got, host_pass(zkg, ctx), (k, spec, "serial"))
        assert_same_witness(zkg.zklaim_witness_mirror(ctx), got, (k, spec, "mirror under serial"))
        monkeypatch.delenv("ZKG_SERIAL_CIRCUIT")


def test_broken_payload_list_is_an_error():
    zkg = _zkg()
    keep = []
    ctx = zkg.make_ctx(payloads(2, 0), keep)
    ctx.num_of_payloads = 3
    with pytest.raises(zkg.ZkgError):
        zkg.zklaim_witness_mirror(ctx)
