"""CPU suite: zkg_qap_instance_async, zkg_qap_set_column_segment, zkg_qap_instance_stats and zkg_groth16_setup_dev exist in the header, the
library and the binding with the documented signatures; without zkg_init the two entries fail with a message and write nothing; and
Keypair(..., dev=False) — the default — goes through zkg_groth16_setup alone."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkg_qap_instance_async", "zkg_qap_set_column_segment", "zkg_qap_instance_stats", "zkg_groth16_setup_dev")
FILL = 0xA5A5A5A5A5A5A5A5


def _lib():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    L = zklaim_amd.lib()
    L.zkg_qap_instance_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.zkg_qap_set_column_segment.argtypes = [C.c_void_p, C.c_size_t]
    L.zkg_groth16_setup_dev.restype = C.c_void_p
    L.zkg_groth16_setup_dev.argtypes = [C.c_void_p, C.c_void_p]
    return zklaim_amd, L


def _tiny_system(zkg, keep):
    """x * x = y over two variables: one row per matrix"""
    one = np.array([[1, 0, 0, 0]], np.uint64)
    rp = np.array([0, 1], np.uint32)
    return zkg.make_r1cs(2, 1, (rp, np.array([1], np.uint32), one), (rp, np.array([1], np.uint32), one), (rp, np.array([2], np.uint32), one), keep)


def test_header_library_and_binding_have_the_new_entries():
    zkg, L = _lib()
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "zkg.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", header)
    assert re.search(r"int zkg_qap_instance_async\( ?zkg_qap \*q, const uint64_t t\[4\] , void \*d_abc , size_t stride , void \*d_z , void \*stream\);", flat)
    assert re.search(r"void zkg_qap_set_column_segment\(zkg_qap \*q, size_t k\);", flat)
    assert re.search(r"void zkg_qap_instance_stats\(size_t out\[2\]\);", flat)
    assert re.search(r"zkg_keypair \*zkg_groth16_setup_dev\(const zkg_r1cs \*cs, const uint64_t \*trapdoor ?\);", flat)
    for name in NAMES:
        assert name in zkg.DECLARED_SYMBOLS and hasattr(L, name), name
    assert list(inspect.signature(zkg.Qap.instance_async).parameters) == ["self", "t", "d_abc_ptr", "stride", "d_z_ptr", "stream"]
    assert [p.default for p in inspect.signature(zkg.Qap.instance_async).parameters.values()][3:] == [None, 0, 0]
    assert list(inspect.signature(zkg.Qap.set_column_segment).parameters) == ["self", "k"]
    assert callable(zkg.qap_instance_stats)
    params = inspect.signature(zkg.Keypair.__init__).parameters
    assert list(params) == ["self", "r1cs", "trapdoor", "dev"] and params["trapdoor"].default is None and params["dev"].default is False


def test_without_zkg_init_both_entries_fail_with_a_message_and_write_nothing():
    from zklaim_amd import api
    zkg, L = _lib()
    if api._initialised:                                            # a GPU box with the library already initialised by an earlier test: the rule
        return                                                      # cannot be seen from this process any more
    keep = []
    cs = _tiny_system(zkg, keep)
    t = np.array([1, 2, 3, 4], np.uint64); abc = np.full((9, 4), FILL, np.uint64); z = np.full((1, 4), FILL, np.uint64)
    assert L.zkg_qap_instance_async(None, t.ctypes.data, abc.ctypes.data, 3, z.ctypes.data, None) == zkg.ERROR
    assert "zkg_init" in L.zkg_last_error().decode()
    assert zkg.qap_instance_stats() == (0, 0)
    assert (abc == FILL).all() and (z == FILL).all()
    L.zkg_qap_set_column_segment(None, 128)                         # a null handle: nothing happens
    td = np.arange(1, 21, dtype=np.uint64).reshape(5, 4) & np.uint64(0xFFFF)
    assert L.zkg_groth16_setup_dev(C.byref(cs), td.ctypes.data) is None
    assert "zkg_init" in L.zkg_last_error().decode()
    assert L.zkg_groth16_setup_dev(None, None) is None and L.zkg_last_error().decode()
    try:
        zkg.Keypair(cs, td, dev=True)
    except zkg.ZkgError as e:
        assert "zkg_groth16_setup_dev" in str(e) and "zkg_init" in str(e)
    else:
        raise AssertionError("Keypair(cs, td, dev=True) was made without zkg_init")


class _Entry:
    def __init__(self, log, name, result):
        self.log, self.name, self.result = log, name, result
        self.restype = self.argtypes = None

    def __call__(self, *args):
        self.log.append(self.name)
        return self.result


class _RecordingLib:
    """stands in for libzkg.so: every entry can be called, the calls are written down"""

    def __init__(self):
        self.calls, self._entries = [], {}

    def __getattr__(self, name):
        if name.startswith("_") or name == "calls":
            raise AttributeError(name)
        if name not in self._entries:
            result = {"zkg_keypair_pk": C.pointer(__import__("zklaim_amd").PK()), "zkg_keypair_swapped": 0}.get(name, 1)
            self._entries[name] = _Entry(self.calls, name, result)
        return self._entries[name]


def test_keypair_without_dev_takes_the_old_entry_alone(monkeypatch):
    from zklaim_amd import api
    zkg, _ = _lib()
    keep = []
    cs = _tiny_system(zkg, keep)
    td = np.ones((5, 4), np.uint64)
    for kwargs, used, unused in (({}, "zkg_groth16_setup", "zkg_groth16_setup_dev"), ({"dev": False}, "zkg_groth16_setup", "zkg_groth16_setup_dev"),
                                 ({"dev": True}, "zkg_groth16_setup_dev", "zkg_groth16_setup")):
        fake = _RecordingLib()
        monkeypatch.setattr(api, "lib", lambda fake=fake: fake)
        kp = zkg.Keypair(cs, td, **kwargs)
        kp.free()
        assert used in fake.calls and unused not in fake.calls, kwargs
        assert not [c for c in fake.calls if c.startswith("zkg_qap")], kwargs
