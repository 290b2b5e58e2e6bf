"""CPU suite: zkg_groth16_verify_each has no CPU path.  Without a GPU the entry fails loudly whatever it is given and whatever its test hook
was set to, writes no verdict and leaves its counters at zero; the single verifier beside it keeps working."""
import numpy as np
import pytest

from util import golden


def test_verify_each_needs_a_gpu_whatever_the_round_size():
    import torch
    import zklaim_amd as zk
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from zklaim_amd import build
    build.build()
    case = golden("groth16.json")[0]
    item = (b"\0" * 600, np.zeros((case["num_inputs"], 4), np.uint64), bytes.fromhex(case["proof_hex"]))
    try:
        for chunk in (0, 1, 64):
            zk.verify_each_set_chunk(chunk)
            for items in ([item], [item] * 3, []):
                with pytest.raises(zk.ZkgError) as e:
                    zk.groth16_verify_each(items)
                assert "zkg_groth16_verify_each" in str(e.value) and "no CPU path" in str(e.value)
                assert zk.verify_each_stats() == (0, 0, 0)
    finally:
        zk.verify_each_set_chunk(0)
    assert zk.groth16_verify(*item) == 2                                        # the host verifier is what decides without a GPU
