"""CPU suite: the batch verifier and the pairing product have no CPU path — without a GPU both fail loudly."""
import numpy as np
import pytest


def test_batch_entry_points_need_a_gpu():
    import torch
    import zklaim_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from zklaim_amd import build
    build.build()
    with pytest.raises(zklaim_amd.ZkgError):
        zklaim_amd.init(0)
    with pytest.raises(zklaim_amd.ZkgError):
        zklaim_amd.groth16_verify_batch([(b"\0" * 600, np.zeros((1, 4), np.uint64), b"\0" * 134)])
    with pytest.raises(zklaim_amd.ZkgError):
        zklaim_amd.groth16_verify_batch([])
    with pytest.raises(zklaim_amd.ZkgError):
        zklaim_amd.pairing_product(np.zeros((1, 8), np.uint64), np.zeros((1, 16), np.uint64))
    with pytest.raises(zklaim_amd.ZkgError):
        zklaim_amd.pairing_product(np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64))
