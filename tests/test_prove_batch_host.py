"""CPU suite: the batch prover's entry points exist in the header, the library and the binding; without a GPU there is no key to prove
on and every misuse of the binding fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zkg_groth16_prove_batch", "zkg_prove_batch_stats", "zkg_prove_batch_chunk")


def test_header_declares_and_library_exports_the_batch_prover():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    header = open(os.path.join(ROOT, "include", "zkg.h")).read()
    L = zklaim_amd.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in zklaim_amd.DECLARED_SYMBOLS
        assert hasattr(L, name), name
    assert "typedef struct zkg_prove_item" in header
    # the binding's item mirrors the header's struct: seven pointer-sized fields
    assert C.sizeof(zklaim_amd.api.ProveItem) == 7 * C.sizeof(C.c_void_p)


def test_batch_prover_without_a_key():
    import zklaim_amd
    from zklaim_amd import build
    build.build()
    w = np.zeros((3, 4), np.uint64); r = np.zeros(4, np.uint64)
    with pytest.raises(zklaim_amd.ZkgError):
        zklaim_amd.groth16_prove_batch(None, [(w, r, r)])                        # no key: a null crs is ZKG_ERROR
    with pytest.raises(zklaim_amd.ZkgError):
        zklaim_amd.groth16_prove_batch(None, [(w, r)])                           # not an item
    with pytest.raises(zklaim_amd.ZkgError):
        zklaim_amd.groth16_prove_batch(None, [(w, r[:3], r)])                    # r must be 4 limbs
    assert zklaim_amd.groth16_prove_batch(None, []) == []                        # count == 0 is ZKG_OK and touches nothing
    assert zklaim_amd.prove_batch_stats() == (0, 0, 0)
    L = zklaim_amd.lib()
    L.zkg_prove_batch_chunk.restype = C.c_size_t
    L.zkg_prove_batch_chunk.argtypes = [C.c_void_p]
    assert L.zkg_prove_batch_chunk(None) == 0
