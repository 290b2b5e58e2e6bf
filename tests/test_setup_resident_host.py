"""CPU suite: zkg_fr_nonzero_index's host side (where 0) against value % r != 0 on raw limbs, its edge arguments, and what
zkg_groth16_setup_resident, zkg_free and zkg_setup_resident_stats promise without a GPU: a refusal with a message and out-pointers left alone."""
import ctypes as C

import numpy as np

from util import MONT, R, arr

FILL = 0xA5A5A5A5


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_fr_nonzero_index.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.zkg_groth16_setup_resident.argtypes = [C.c_void_p] * 7
    L.zkg_free.argtypes = [C.c_void_p]; L.zkg_free.restype = None
    return zklaim_amd, L


def _tiny_system(zkg, keep):
    """x * x = y over two variables: one row per matrix"""
    one = np.array([[1, 0, 0, 0]], np.uint64)
    rp = np.array([0, 1], np.uint32)
    return zkg.make_r1cs(2, 1, (rp, np.array([1], np.uint32), one), (rp, np.array([1], np.uint32), one), (rp, np.array([2], np.uint32), one), keep)


def test_the_new_entries_are_declared_and_bound():
    zkg, L = _lib()
    for name in ("zkg_groth16_setup_resident", "zkg_free", "zkg_setup_resident_stats", "zkg_fr_nonzero_index"):
        assert name in zkg.DECLARED_SYMBOLS and hasattr(L, name), name
    assert callable(zkg.groth16_setup_resident) and callable(zkg.setup_resident_stats) and callable(zkg.fr_nonzero_index)


def test_host_index_is_value_mod_r_on_every_representative():
    zkg, _ = _lib()
    values = [0, R, 1, R - 1, R + 1, 2 * R - 1, MONT % R, 0, R, 5, R, 0, R + MONT % R, 7]
    fr = arr(values)                                                 # raw limbs, nothing reduced
    want = [i for i, v in enumerate(values) if v % R != 0]
    assert want == [2, 3, 4, 5, 6, 9, 12, 13]
    assert zkg.fr_nonzero_index(fr, where=0).tolist() == want
    rng = np.random.default_rng(0x5E7)                               # and a longer vector: 0 and r scattered among random limbs
    n = 1000
    big = rng.integers(0, 1 << 62, (n, 4), dtype=np.uint64)
    kind = rng.integers(0, 3, n)
    big[kind == 0] = 0
    big[kind == 1] = arr([R])[0]
    assert zkg.fr_nonzero_index(big, where=0).tolist() == np.nonzero(kind == 2)[0].tolist()


def test_host_index_edges_and_null_arguments():
    zkg, L = _lib()
    out = np.full(8, FILL, np.uint32); count = C.c_size_t(77)
    assert L.zkg_fr_nonzero_index(None, 0, 0, out.ctypes.data, C.byref(count)) == zkg.OK         # n = 0: count 0, nothing written
    assert count.value == 0 and (out == FILL).all()
    assert L.zkg_fr_nonzero_index(None, 0, 0, None, C.byref(count)) == zkg.OK and count.value == 0
    fr = arr([1, 0, 2])
    count = C.c_size_t(77)
    assert L.zkg_fr_nonzero_index(fr.ctypes.data, 3, 0, out.ctypes.data, C.byref(count)) == zkg.OK
    assert count.value == 2 and out[:2].tolist() == [0, 2] and (out[2:] == FILL).all()           # nothing behind idx_out[count]
    for args in ((None, 3, 0, out.ctypes.data, C.byref(count)), (fr.ctypes.data, 3, 0, None, C.byref(count)), (fr.ctypes.data, 3, 0, out.ctypes.data, None),
                 (fr.ctypes.data, 3, 2, out.ctypes.data, C.byref(count))):
        assert L.zkg_fr_nonzero_index(*args) == zkg.ERROR
        assert "zkg_fr_nonzero_index" in L.zkg_last_error().decode()
    assert L.zkg_fr_nonzero_index(fr.ctypes.data, (1 << 28) + 1, 0, out.ctypes.data, C.byref(count)) == zkg.ERROR     # refused before anything is read


def test_setup_resident_refuses_without_init_and_null_out_pointers_and_writes_nothing():
    from zklaim_amd import api
    zkg, L = _lib()
    keep = []
    cs = _tiny_system(zkg, keep)
    td = np.arange(1, 21, dtype=np.uint64).reshape(5, 4) & np.uint64(0xFFFF)
    mark = 0x1234
    pk = C.c_void_p(mark); vk = C.c_void_p(mark); crs = C.c_void_p(mark); pk_len = C.c_size_t(mark); vk_len = C.c_size_t(mark)
    full = [C.byref(cs), td.ctypes.data, C.byref(pk), C.byref(pk_len), C.byref(vk), C.byref(vk_len), C.byref(crs)]

    def untouched():
        return pk.value == mark and vk.value == mark and crs.value == mark and pk_len.value == mark and vk_len.value == mark

    for hole in (0, 2, 3, 4, 5):                                     # a null cs, pk_blob, pk_len, vk_blob, vk_len
        args = list(full); args[hole] = None
        assert L.zkg_groth16_setup_resident(*args) == zkg.ERROR
        assert "zkg_groth16_setup_resident" in L.zkg_last_error().decode() and untouched(), hole
    if not api._initialised:                                         # (a process an earlier test initialised cannot show this rule any more)
        assert L.zkg_groth16_setup_resident(*full) == zkg.ERROR
        msg = L.zkg_last_error().decode()
        assert "zkg_groth16_setup_resident" in msg and "zkg_init" in msg and untouched()
        try:
            zkg.groth16_setup_resident(cs, td)
        except zkg.ZkgError as e:
            assert "zkg_groth16_setup_resident" in str(e) and "zkg_init" in str(e)
        else:
            raise AssertionError("groth16_setup_resident made a key without zkg_init")
        assert zkg.fr_nonzero_index(arr([1, 0]), where=0).tolist() == [0]                         # the host loop needs no zkg_init ...
        try:
            zkg.fr_nonzero_index(arr([1, 0]), where=1)                                            # ... the kernels do
        except zkg.ZkgError as e:
            assert "zkg_init" in str(e)
        else:
            raise AssertionError("fr_nonzero_index(where=1) ran without zkg_init")
    L.zkg_free(None)                                                 # accepted
    assert len(zkg.setup_resident_stats()) == 3


def test_crs_wraps_a_handle_it_did_not_create(monkeypatch):
    from zklaim_amd import api
    zkg, _ = _lib()
    freed = []

    class Fake:
        def zkg_crs_free(self, h):
            freed.append(h.value)

    monkeypatch.setattr(api, "lib", lambda: Fake())
    crs = zkg.Crs(handle=0xBEEF, m=1024)
    assert crs._h == 0xBEEF and crs.m == 1024
    crs.free(); crs.free()
    assert freed == [0xBEEF]                                         # owned: freed once
