"""The two synthetic constraint systems the instance-map and device-generator tests share: -> (n, l, A, B, C, witness)."""
import numpy as np

from util import R, arr


def log10_system():
    from zklaim_amd import synth
    n, l, A, B, C, w = synth.zklaim_shaped(10, num_inputs=5, seed=0x0A)
    return n, l, A, B, C, w


def step_system():
    """zklaim_shaped(12) padded by 40 rows 1 * 0 = 0 as in test_gpu_qap.py: m = 2^12 + 2^6"""
    from zklaim_amd import synth
    n, l, A, B, C, w = synth.zklaim_shaped(12, num_inputs=5, seed=19)
    pad = 40
    A = (np.concatenate([A[0], A[0][-1] + np.arange(1, pad + 1, dtype=np.uint32)]), np.concatenate([A[1], np.zeros(pad, np.uint32)]),
         np.concatenate([A[2], np.tile(arr([1], R), (pad, 1))]))
    B = (np.concatenate([B[0], np.full(pad, B[0][-1], np.uint32)]), B[1], B[2])
    C = (np.concatenate([C[0], np.full(pad, C[0][-1], np.uint32)]), C[1], C[2])
    return n, l, A, B, C, w
