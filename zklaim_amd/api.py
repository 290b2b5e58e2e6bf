"""ctypes binding of include/zkg.h (the drop-in boundary below snark.cpp:126 of the reference).

Array conventions are those of zkg.h: numpy uint64 arrays of little-endian limbs, Montgomery form
unless stated, G1 affine 8 limbs, G2 affine 16 limbs, normalised "jac" outputs 12 / 24 limbs.
*_dev functions take raw device pointers (e.g. ``torch.Tensor.data_ptr()``) and a HIP stream handle.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libzkg.so")

DECLARED_SYMBOLS = [
    "zkg_init", "zkg_shutdown", "zkg_last_error", "zkg_device_info", "zkg_ntt", "zkg_ntt_dev", "zkg_evaluation_domain_size", "zkg_ntt_domain", "zkg_ntt_domain_dev", "zkg_msm_g1", "zkg_msm_g2",
    "zkg_msm_g1_dev", "zkg_msm_g2_dev", "zkg_msm_g1_windows_dev", "zkg_g1_sum", "zkg_g2_sum", "zkg_g1_fixed_base_dev", "zkg_g2_fixed_base_dev",
    "zkg_groth16_prove_batch_zklaim", "zkg_zklaim_witness_stats", "zkg_zklaim_witness_size", "zkg_zklaim_witness_gpu", "zkg_zklaim_witness_mirror",
    "zkg_crs_upload", "zkg_crs_upload_blob", "zkg_pk_blob_inspect", "zkg_crs_free", "zkg_crs_num_variables", "zkg_groth16_prove", "zkg_groth16_prove_sparse", "zkg_circuit_sparse_witness", "zkg_qap_witness_h", "zkg_prove_stage_ms", "zkg_timing_reset",
    "zkg_timing_dominant_ms", "zkg_zklaim_circuit_new", "zkg_zklaim_witness_new", "zkg_circuit_num_variables", "zkg_circuit_free", "zkg_circuit_r1cs", "zkg_circuit_witness",
    "zkg_circuit_is_satisfied", "zkg_circuit_first_unsatisfied", "zkg_zklaim_input_map", "zkg_groth16_setup", "zkg_keypair_free",
    "zkg_keypair_pk", "zkg_keypair_swapped", "zkg_keypair_pk_blob", "zkg_keypair_vk_blob", "zkg_groth16_verify", "zkg_pairing_probe", "zkg_pairing_selfcheck",
    "zkg_compat_reset", "zkg_field_op", "zkg_init_multi", "zkg_msm_g1_shards_upload", "zkg_msm_g1_shards_free", "zkg_msm_g1_shards_count",
    "zkg_msm_g1_multi", "zkg_g1_add_quad29", "zkg_crs_shard_h", "zkg_msm_g1_bases_upload", "zkg_msm_g1_resident", "zkg_msm_g1_bases_free",
    "zkg_prover_peak_in_flight", "zkg_msm_g1_host_scalars", "zkg_multi_rccl_calls", "zkg_g1_add_pair29",
    "zkg_groth16_verify_batch", "zkg_pairing_product", "zkg_verify_batch_stats",
    "zkg_groth16_prove_batch", "zkg_prove_batch_stats", "zkg_prove_batch_chunk", "zkg_zklaim_prove_batch",
    "zkg_groth16_prove_zklaim", "zkg_prove_zklaim_stats", "zkg_zklaim_witness_gpu_parallel", "zkg_zklaim_witness_mirror_parallel",
    "zkg_fr29_op", "zkg_fq29_op", "zkg_fq29_op_chain",
    "zkg_zklaim_verify_batch", "zkg_zklaim_verify_batch_stats", "zkg_proof_decode_gpu", "zkg_zklaim_input_sums_gpu", "zkg_zklaim_input_map_mirror",
    "zkg_groth16_prove_dev", "zkg_groth16_prove_batch_dev", "zkg_prove_dev_stats",
    "zkg_msm_g1_resident_async", "zkg_msm_g1_resident_batch_max", "zkg_msm_resident_async_stats", "zkg_msm_combine_gpu",
    "zkg_groth16_verify_each", "zkg_verify_each_stats", "zkg_verify_each_set_chunk", "zkg_pairing_each", "zkg_final_exp",
    "zkg_fq12_op", "zkg_point_decompress", "zkg_point_compress",
    "zkg_zklaim_verify_each", "zkg_zklaim_verify_each_stats", "zkg_zklaim_ic_each",
    "zkg_curve_op",
    "zkg_domain_new", "zkg_domain_free", "zkg_domain_size", "zkg_domain_batch_max", "zkg_domain_set_batch_max", "zkg_domain_ntt_async",
    "zkg_domain_lagrange_async", "zkg_domain_stats",
    "zkg_msm_g2_bases_upload", "zkg_msm_g2_bases_free", "zkg_msm_g2_resident", "zkg_msm_g2_resident_async", "zkg_msm_g2_resident_batch_max",
    "zkg_msm_combine_g2_gpu",
    "zkg_qap_new", "zkg_qap_free", "zkg_qap_domain_size", "zkg_qap_num_variables", "zkg_qap_batch_max", "zkg_qap_set_batch_max",
    "zkg_qap_witness_h_async", "zkg_qap_stats",
    "zkg_qap_instance_async", "zkg_qap_set_column_segment", "zkg_qap_instance_stats", "zkg_groth16_setup_dev",
    "zkg_msm_host_scalars_stats",
    "zkg_groth16_setup_resident", "zkg_free", "zkg_setup_resident_stats", "zkg_fr_nonzero_index",
    "zkg_prover_new", "zkg_prover_free", "zkg_prover_batch_max", "zkg_prover_set_batch_max", "zkg_prover_prove_async", "zkg_prover_stats",
    "zkg_proof_assemble",
]
# the reference's own seam, exported with its original names (zklaim.h:257-259)
COMPAT_SYMBOLS = ["libsnark_trusted_setup", "libsnark_prove", "libsnark_verify"]


OK, ERROR, UNSATISFIED = 0, 1, 2          # include/zkg.h


class ZkgError(RuntimeError):
    pass


class R1CS(C.Structure):
    _fields_ = [("num_variables", C.c_uint32), ("num_inputs", C.c_uint32), ("num_constraints", C.c_uint32), ("reserved", C.c_uint32)] + \
        [(f"{m}_{f}", C.c_void_p) for m in "abc" for f in ("rowptr", "col", "val")]


class PK(C.Structure):
    _fields_ = [("cs", R1CS), ("log_m", C.c_uint32), ("domain_size", C.c_uint32)] + \
        [(k, C.c_void_p) for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "A_query", "B_g1", "B_g2", "H_query", "L_query")]


_lib = None


def lib():
    """Loads libzkg.so.  Fails loudly when it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise ZkgError(f"{_SO} is missing: build it with `python -m zklaim_amd.build` (hipcc, gfx950)")
        # One ROCm stack per process: PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64.  If libzkg.so pulled in the
        # system copies first and torch loaded afterwards, two HSA runtimes would coexist and device discovery fails.  When torch
        # is installed, let it load its runtime first; libzkg.so's libamdhip64.so.7 dependency then resolves to the same objects.
        if "torch" not in sys.modules and not os.environ.get("ZKG_NO_TORCH"):
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        _lib = C.CDLL(_SO)
        _lib.zkg_last_error.restype = C.c_char_p
        _lib.zkg_timing_dominant_ms.restype = C.c_float
        _lib.zkg_crs_upload.restype = C.c_void_p
        _lib.zkg_crs_upload.argtypes = [C.c_void_p]
        _lib.zkg_crs_upload_blob.restype = C.c_void_p
        _lib.zkg_crs_upload_blob.argtypes = [C.c_void_p, C.c_size_t]
        _lib.zkg_crs_free.argtypes = [C.c_void_p]
    return _lib


def _check(rc, what):
    if rc != 0:
        raise ZkgError(f"{what} failed (rc={rc}): {lib().zkg_last_error().decode()}")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _vp(x):
    return C.c_void_p(int(x) if x else 0)


_initialised = False


def init(device=0):
    global _initialised
    _check(lib().zkg_init(int(device)), "zkg_init")
    _initialised = True


def shutdown():
    global _initialised
    if _initialised:
        lib().zkg_shutdown()
    _initialised = False


def device_info():
    name = C.create_string_buffer(128); cus = C.c_int(0)
    _check(lib().zkg_device_info(name, C.c_size_t(128), C.byref(cus)), "zkg_device_info")
    return name.value.decode(), cus.value


def field_op(field, op, a, b=None):
    """element-wise device arithmetic (zkg_field_op): field 0 Fq, 1 Fr, 2 Fq2; op 0 mul 1 add 2 sub 3 inv 4 to_mont 5 from_mont 6 neg 7 sqr;
    Fq only: 10-15 the 29-bit representation of the accumulation kernel (mul, add, sub, zero test, composite, inverse of 3a) entered through
    to29 on canonical values: a smoke of that code on digits below 1.01 q.  Its lazy bounds are tested on raw limbs through fq29_op
    (tests/test_gpu_fq29.py).
    The lazy range of the 32-bit layer (no input is normalised: any representative below 2p may be passed): 8 dbl; raw stores 20 mul 21 add
    22 sub 26 neg 27 sqr 28 dbl; predicates (0 or 1 in the low word) 30 is_zero 31 ==; raw chains 40 ((ab) - a)(a + b), 41 x <- a then eight
    times x <- (x + x) - b, 42 M = 3 a^2, M^2 - 2ab (tests/test_gpu_fp32.py)."""
    a = _u64(a); limbs = 8 if field == 2 else 4
    out = np.zeros_like(a)
    bb = None if b is None else _u64(b)
    _check(lib().zkg_field_op(int(field), int(op), _p(a), _p(bb), C.c_size_t(a.size // limbs), _p(out)), "zkg_field_op")
    return out


FR29_OPS = {"mul": (0, 2, 1), "mul2": (1, 4, 2), "norm": (2, 1, 1), "add_norm": (3, 2, 1), "sub_norm": (4, 2, 1), "add_lazy": (5, 2, 1), "sub_lazy": (6, 2, 1),
            "slice": (7, 1, 1), "unslice_reduce": (8, 1, 1), "r4": (9, 7, 4), "r4_stage0": (10, 7, 4), "r4_norm_stores": (11, 7, 4),
            "r4_stage0_norm_stores": (12, 7, 4), "r2_tail": (13, 3, 2), "r2_tail_stage0": (14, 3, 2)}          # name -> (op, k, m) of zkg_fr29_op


def fr29_op(name, x):
    """the NTT's 29-bit Fr arithmetic on raw limbs (zkg_fr29_op): x is (n, k, 9) uint32, the result (n, m, 9) uint32"""
    op, k, m = FR29_OPS[name]
    x = np.ascontiguousarray(x, dtype=np.uint32)
    if x.ndim != 3 or x.shape[1:] != (k, 9):
        raise ZkgError(f"fr29_op {name}: input must be (n, {k}, 9), got {x.shape}")
    out = np.zeros((x.shape[0], m, 9), np.uint32)
    _check(lib().zkg_fr29_op(int(op), _p(x), C.c_size_t(x.shape[0]), _p(out)), "zkg_fr29_op")
    return out


FQ29_OPS = {"mul": (0, 2, 1), "mul2": (1, 4, 2), "sqr": (2, 1, 1), "sqr2": (3, 2, 2), "norm": (4, 1, 1), "add": (5, 2, 1), "dbl": (6, 1, 1),
            "sub_S2_1": (7, 2, 1), "sub_S4_1": (8, 2, 1), "sub_S6_1": (9, 2, 1), "sub_S4_3": (10, 2, 1), "neg_S2_1": (11, 1, 1), "is_zero": (12, 1, 1),
            "unpack": (13, 1, 1), "to29": (14, 1, 1), "from29": (15, 1, 1), "rec64": (16, 3, 3), "bucket29": (17, 5, 4), "inverse": (18, 1, 1),
            "madd": (19, 7, 5), "add_lane": (20, 8, 4), "add_pair": (21, 8, 4), "add_quad": (22, 8, 4)}           # name -> (op, k, m) of zkg_fq29_op


def fq29_op(name, x, chain=0):
    """the multi-exponentiation's 29-bit Fq arithmetic on raw limbs (zkg_fq29_op, zkg_fq29_op_chain): x is (n, k, 9) uint32, the result
    (n, m, 9) uint32; chain (madd and the three additions only): that many further steps on the device"""
    op, k, m = FQ29_OPS[name]
    x = np.ascontiguousarray(x, dtype=np.uint32)
    if x.ndim != 3 or x.shape[1:] != (k, 9):
        raise ZkgError(f"fq29_op {name}: input must be (n, {k}, 9), got {x.shape}")
    out = np.zeros((x.shape[0], m, 9), np.uint32)
    _check(lib().zkg_fq29_op_chain(int(op), int(chain), _p(x), C.c_size_t(x.shape[0]), _p(out)), "zkg_fq29_op")
    return out


def g1_add_quad29(a_jac, b_jac, chain=0):
    """out[i] = a[i] + b[i] (then `chain` rounds of x <- 2x + b[i]) on the GPU through the 29-bit quad addition of the reduction kernels"""
    a = _u64(a_jac); b = _u64(b_jac); out = np.zeros_like(a)
    _check(lib().zkg_g1_add_quad29(_p(a), _p(b), C.c_size_t(a.size // 12), int(chain), _p(out)), "zkg_g1_add_quad29")
    return out.reshape(-1, 12)


def g1_add_pair29(a_jac, b_jac, chain=0):
    """the same through the pair form of the addition (xyzz29_add_pair, the bucket reduction's since round 4)"""
    a = _u64(a_jac); b = _u64(b_jac); out = np.zeros_like(a)
    _check(lib().zkg_g1_add_pair29(_p(a), _p(b), C.c_size_t(a.size // 12), int(chain), _p(out)), "zkg_g1_add_pair29")
    return out.reshape(-1, 12)


CURVE_OPS = {"madd": 0, "add": 1, "add_quad": 2, "dbl": 3, "dbl_affine": 4, "to_affine": 5, "mul": 6}          # name -> op of zkg_curve_op


def curve_op(group, name, a, b=None, k=None, chain=0):
    """the 32-bit device group law on raw records (zkg_curve_op): group 0 G1, 1 G2; a, b (n, coordinates, w) uint32 with w = 8 (G1) or 16 (G2)
    limbs per coordinate, XYZZ records of 4 coordinates and affine ones of 2 (b of madd, a of dbl_affine); k (n, 8) uint32 scalars for mul.
    Returns (n, 4, w), for to_affine (n, 2, w), for add_quad (n, 4 lanes, 4, w)."""
    op = CURVE_OPS[name]; w = 16 if group else 8
    a = np.ascontiguousarray(a, dtype=np.uint32)
    need_a = 2 if name == "dbl_affine" else 4
    if a.ndim != 3 or a.shape[1:] != (need_a, w):
        raise ZkgError(f"curve_op {name}: a must be (n, {need_a}, {w}), got {a.shape}")
    n = a.shape[0]
    if name in ("madd", "add", "add_quad"):
        need_b = 2 if name == "madd" else 4
        b = np.ascontiguousarray(b, dtype=np.uint32)
        if b.shape != (n, need_b, w):
            raise ZkgError(f"curve_op {name}: b must be ({n}, {need_b}, {w}), got {b.shape}")
    else:
        b = None
    if name == "mul":
        k = np.ascontiguousarray(k, dtype=np.uint32)
        if k.shape != (n, 8):
            raise ZkgError(f"curve_op mul: k must be ({n}, 8), got {k.shape}")
    else:
        k = None
    shape = (n, 2, w) if name == "to_affine" else (n, 4, 4, w) if name == "add_quad" else (n, 4, w)
    out = np.zeros(shape, np.uint32)
    _check(lib().zkg_curve_op(int(group), int(op), _p(a), _p(b), _p(k), C.c_size_t(n), int(chain), _p(out)), "zkg_curve_op")
    return out


# ---- NTT (libfqfft basic_radix2_domain FFT/iFFT/cosetFFT/icosetFFT) -------------------------------
def ntt(a, inverse=False, coset=False):
    """FFT / iFFT / cosetFFT / icosetFFT on the domain get_evaluation_domain(len(a)) names: a power of two
    (basic_radix2_domain, zkg_ntt) or 2^a + 2^b (step_radix2_domain, zkg_ntt_domain)"""
    a = _u64(a).copy(); n = a.size // 4
    logn = n.bit_length() - 1
    if n == 0:
        raise ZkgError("ntt: empty input")
    if (1 << logn) == n:
        _check(lib().zkg_ntt(_p(a), C.c_uint(logn), int(inverse), int(coset)), "zkg_ntt")
    else:
        _check(lib().zkg_ntt_domain(_p(a), C.c_size_t(n), int(inverse), int(coset)), "zkg_ntt_domain")
    return a.reshape(n, 4)


def pk_blob_inspect(blob):
    """host-only walk of a pk blob (zkg_pk_blob_inspect): dict of its sizes, or ZkgError"""
    out = np.zeros(8, np.uint64)
    buf = (C.c_ubyte * len(blob)).from_buffer_copy(blob) if len(blob) else None
    L = lib()
    L.zkg_pk_blob_inspect.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    _check(L.zkg_pk_blob_inspect(C.cast(buf, C.c_void_p) if buf is not None else None, C.c_size_t(len(blob)), _p(out)), "zkg_pk_blob_inspect")
    names = ("A_query", "B_values", "H_query", "L_query", "num_inputs", "num_constraints", "terms", "domain_size")
    return {k: int(v) for k, v in zip(names, out)}


def evaluation_domain_size(min_size):
    """libfqfft get_evaluation_domain(min_size) -> (m, is_step)"""
    m = C.c_size_t(0); st = C.c_int(0)
    _check(lib().zkg_evaluation_domain_size(C.c_size_t(min_size), C.byref(m), C.byref(st)), "zkg_evaluation_domain_size")
    return m.value, bool(st.value)


def ntt_dev(d_ptr, logn, inverse=False, coset=False, stream=0):
    _check(lib().zkg_ntt_dev(_vp(d_ptr), C.c_uint(logn), int(inverse), int(coset), _vp(stream)), "zkg_ntt_dev")


class Domain:
    """zkg_domain: the evaluation domain of size m (2^k or 2^a + 2^b) as a handle — batched transforms and the Lagrange coefficients on
    device memory, queued on the caller's stream without a wait on the host"""

    def __init__(self, m):
        L = lib()
        L.zkg_domain_new.restype = C.c_void_p
        L.zkg_domain_new.argtypes = [C.c_size_t]
        L.zkg_domain_free.argtypes = [C.c_void_p]
        for name in ("zkg_domain_size", "zkg_domain_batch_max"):
            getattr(L, name).restype = C.c_size_t
            getattr(L, name).argtypes = [C.c_void_p]
        L.zkg_domain_set_batch_max.argtypes = [C.c_void_p, C.c_size_t]
        L.zkg_domain_ntt_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        L.zkg_domain_lagrange_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._h = L.zkg_domain_new(C.c_size_t(m))
        if not self._h:
            raise ZkgError("zkg_domain_new failed: " + L.zkg_last_error().decode())
        self.m = m

    def ntt_async(self, d_ptr, count=1, stride=None, inverse=False, coset=False, stream=0):
        """zkg_domain_ntt_async: `count` in-place transforms of m Fr each, `stride` elements apart (default m), at the device address d_ptr.
        Returns without waiting: synchronise `stream` before reading the result on the host."""
        _check(lib().zkg_domain_ntt_async(C.c_void_p(self._h), _vp(d_ptr), C.c_size_t(self.m if stride is None else stride), C.c_size_t(count),
                                          int(inverse), int(coset), _vp(stream)), "zkg_domain_ntt_async")

    def lagrange_async(self, t, d_u_ptr, d_z_ptr=0, stream=0):
        """zkg_domain_lagrange_async: t (4 Montgomery limbs, host) -> evaluate_all_lagrange_polynomials(t) at the device address d_u_ptr
        (m Fr) and, if d_z_ptr is given, Z(t) there (one Fr)"""
        t = _u64(t).reshape(4)
        _check(lib().zkg_domain_lagrange_async(C.c_void_p(self._h), _p(t), _vp(d_u_ptr), _vp(d_z_ptr), _vp(stream)), "zkg_domain_lagrange_async")

    def batch_max(self):
        return int(lib().zkg_domain_batch_max(C.c_void_p(self._h)))

    def set_batch_max(self, k):
        """test hook: k vectors per launch sequence from now on (0: the default; a larger k is clamped to it)"""
        lib().zkg_domain_set_batch_max(C.c_void_p(self._h), C.c_size_t(k))

    def size(self):
        return int(lib().zkg_domain_size(C.c_void_p(self._h)))

    def free(self):
        if self._h:
            lib().zkg_domain_free(C.c_void_p(self._h)); self._h = None


def domain_stats():
    """(vectors, launch groups, host waits) of the calling thread's last Domain.ntt_async"""
    out = (C.c_size_t * 3)()
    lib().zkg_domain_stats(out)
    return tuple(int(v) for v in out)


class Qap:
    """zkg_qap: r1cs_to_qap_witness_map on device-resident witnesses as a handle on a constraint system alone (cs: make_r1cs's struct, host
    CSR, copied to the device) — coefficients_for_H of many witnesses per call, queued on the caller's stream without a wait on the host"""

    def __init__(self, cs):
        L = lib()
        L.zkg_qap_new.restype = C.c_void_p
        L.zkg_qap_new.argtypes = [C.c_void_p]
        L.zkg_qap_free.argtypes = [C.c_void_p]
        for name in ("zkg_qap_domain_size", "zkg_qap_batch_max"):
            getattr(L, name).restype = C.c_size_t
            getattr(L, name).argtypes = [C.c_void_p]
        L.zkg_qap_num_variables.restype = C.c_uint32
        L.zkg_qap_num_variables.argtypes = [C.c_void_p]
        L.zkg_qap_set_batch_max.argtypes = [C.c_void_p, C.c_size_t]
        L.zkg_qap_witness_h_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.zkg_qap_instance_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.zkg_qap_set_column_segment.argtypes = [C.c_void_p, C.c_size_t]
        self._h = L.zkg_qap_new(C.byref(cs))
        if not self._h:
            raise ZkgError("zkg_qap_new failed: " + L.zkg_last_error().decode())
        self.m, self.n = self.domain_size(), self.num_variables()

    def witness_h_async(self, d_w_ptr, count, stride, d_h_ptr, h_stride, d_unsat_ptr=0, stream=0):
        """zkg_qap_witness_h_async: `count` witnesses of n Montgomery Fr, `stride` elements apart at the device address d_w_ptr, read in place ->
        coefficients_for_H (m + 1 Fr each, `h_stride` apart) at d_h_ptr and, if d_unsat_ptr is given, one 32-bit word per witness there (1: the
        witness violates the system).  Returns without waiting: synchronise `stream` before reading the result on the host."""
        _check(lib().zkg_qap_witness_h_async(C.c_void_p(self._h), _vp(d_w_ptr), C.c_size_t(stride), C.c_size_t(count), _vp(d_h_ptr), C.c_size_t(h_stride),
                                             _vp(d_unsat_ptr), _vp(stream)), "zkg_qap_witness_h_async")

    def instance_async(self, t, d_abc_ptr, stride=None, d_z_ptr=0, stream=0):
        """zkg_qap_instance_async: the QAP polynomials at t (4 Montgomery limbs, host) -> At | Bt | Ct, n + 1 Montgomery Fr each, `stride`
        elements apart (default n + 1) at the device address d_abc_ptr and, if d_z_ptr is given, Z(t) there.  The first call on a handle builds
        the column index and waits for it; later calls return without waiting: synchronise `stream` before reading the result on the host."""
        tt = None if t is None else _u64(t).reshape(-1)
        if tt is not None and tt.size != 4:
            raise ZkgError("zkg_qap_instance_async: t is 4 limbs")
        _check(lib().zkg_qap_instance_async(C.c_void_p(self._h), _p(tt), _vp(d_abc_ptr), C.c_size_t(self.n + 1 if stride is None else stride), _vp(d_z_ptr),
                                            _vp(stream)), "zkg_qap_instance_async")

    def set_column_segment(self, k):
        """test hook: long columns are cut into segments of k terms from the next instance call on (0: the default)"""
        lib().zkg_qap_set_column_segment(C.c_void_p(self._h), C.c_size_t(k))

    def domain_size(self):
        return int(lib().zkg_qap_domain_size(C.c_void_p(self._h)))

    def num_variables(self):
        return int(lib().zkg_qap_num_variables(C.c_void_p(self._h)))

    def batch_max(self):
        return int(lib().zkg_qap_batch_max(C.c_void_p(self._h)))

    def set_batch_max(self, k):
        """test hook: k witnesses per launch sequence from now on (0: the default; a larger k is clamped to it)"""
        lib().zkg_qap_set_batch_max(C.c_void_p(self._h), C.c_size_t(k))

    def free(self):
        if self._h:
            lib().zkg_qap_free(C.c_void_p(self._h)); self._h = None


def qap_stats():
    """(witnesses, launch groups, host waits) of the calling thread's last Qap.witness_h_async"""
    out = (C.c_size_t * 3)()
    lib().zkg_qap_stats(out)
    return tuple(int(v) for v in out)


class Prover:
    """zkg_prover: proofs of a resident key on the caller's stream — witnesses in device memory in, 134-byte proofs in device memory out, no wait
    on the host.  The handle borrows `crs` (a Crs, or a raw zkg_crs pointer): free the prover before the key."""

    def __init__(self, crs):
        L = lib()
        L.zkg_prover_new.restype = C.c_void_p
        L.zkg_prover_new.argtypes = [C.c_void_p]
        L.zkg_prover_free.argtypes = [C.c_void_p]
        L.zkg_prover_batch_max.restype = C.c_size_t
        L.zkg_prover_batch_max.argtypes = [C.c_void_p]
        L.zkg_prover_set_batch_max.argtypes = [C.c_void_p, C.c_size_t]
        L.zkg_prover_prove_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        self._crs = crs                                       # keeps the key alive while the handle lives
        self._h = L.zkg_prover_new(C.c_void_p(getattr(crs, "_h", crs) or 0))
        if not self._h:
            raise ZkgError("zkg_prover_new failed: " + L.zkg_last_error().decode())

    def prove_async(self, d_ptr, stride, count, d_rs, d_proofs, proof_stride, d_status, check_satisfied=True, stream=0):
        """zkg_prover_prove_async: `count` witnesses of n Montgomery Fr, `stride` elements apart at the device address d_ptr, and (r, s) per item
        at d_rs (8 limbs: r | s) -> proof i at d_proofs + i * proof_stride and its status word at d_status + 4 i, all DEVICE addresses.  Returns
        without waiting: synchronise `stream` before reading the result on the host."""
        _check(lib().zkg_prover_prove_async(C.c_void_p(self._h), _vp(d_ptr), C.c_size_t(stride), C.c_size_t(count), _vp(d_rs), 1 if check_satisfied else 0,
                                            _vp(d_proofs), C.c_size_t(proof_stride), _vp(d_status), _vp(stream)), "zkg_prover_prove_async")

    def batch_max(self):
        return int(lib().zkg_prover_batch_max(C.c_void_p(self._h)))

    def set_batch_max(self, k):
        """test hook: k proofs per launch sequence from now on (0: the default; a larger k is clamped to it)"""
        lib().zkg_prover_set_batch_max(C.c_void_p(self._h), C.c_size_t(k))

    def free(self):
        if self._h:
            lib().zkg_prover_free(C.c_void_p(self._h)); self._h = None


def prover_stats():
    """(proofs enqueued, launch groups, host waits) of the calling thread's last Prover.prove_async"""
    out = (C.c_size_t * 3)()
    lib().zkg_prover_stats(out)
    return tuple(int(v) for v in out)


def proof_assemble(key_points, points, rs, where):
    """zkg_proof_assemble: the proof epilogue alone.  key_points: 88 limbs (alpha_g1 | beta_g1 | delta_g1 | A_0 | B1_0 | beta_g2 | delta_g2 | B2_0,
    affine); points: count x 72 limbs (W_a | W_b1 | L | H normalised jac, W_b2); rs: count x 8 limbs.  where 0: the host's assemble_proof (no
    GPU), 1: the epilogue kernels.  Returns count x 134 bytes."""
    kp, pt, r = _u64(key_points).reshape(-1), _u64(points).reshape(-1, 72), _u64(rs).reshape(-1, 8)
    if kp.size != 88 or pt.shape[0] != r.shape[0]:
        raise ZkgError("zkg_proof_assemble: key_points is 88 limbs, points and rs one row per proof")
    out = np.zeros((pt.shape[0], 134), np.uint8)
    L = lib()
    L.zkg_proof_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    _check(L.zkg_proof_assemble(_p(kp), _p(pt), _p(r), C.c_size_t(pt.shape[0]), int(where), _p(out)), "zkg_proof_assemble")
    return out


def qap_instance_stats():
    """(column indexes built, host waits) of the calling thread's last Qap.instance_async"""
    out = (C.c_size_t * 2)()
    lib().zkg_qap_instance_stats(out)
    return tuple(int(v) for v in out)


# ---- MSM (libff multi_exp / multi_exp_with_mixed_addition) -----------------------------------------
def msm_g1(bases, scalars):
    bases = _u64(bases); scalars = _u64(scalars); out = np.zeros(12, np.uint64)
    _check(lib().zkg_msm_g1(_p(bases), _p(scalars), C.c_size_t(scalars.size // 4), _p(out)), "zkg_msm_g1")
    return out


def msm_g2(bases, scalars):
    bases = _u64(bases); scalars = _u64(scalars); out = np.zeros(24, np.uint64)
    _check(lib().zkg_msm_g2(_p(bases), _p(scalars), C.c_size_t(scalars.size // 4), _p(out)), "zkg_msm_g2")
    return out


def init_multi(devices):
    global _initialised
    d = (C.c_int * len(devices))(*devices)
    _check(lib().zkg_init_multi(d, len(devices)), "zkg_init_multi")
    _initialised = True


class MsmShards:
    """G1 bases sharded by points over several devices of this process (zkg_msm_g1_shards_upload); msm() = zkg_msm_g1_multi"""

    def __init__(self, bases, devices):
        bases = _u64(bases)
        L = lib()
        L.zkg_msm_g1_shards_upload.restype = C.c_void_p
        L.zkg_msm_g1_shards_upload.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
        L.zkg_msm_g1_shards_free.argtypes = [C.c_void_p]
        L.zkg_msm_g1_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        d = (C.c_int * len(devices))(*devices)
        self.n = bases.size // 8; self.ndev = len(devices)
        self._h = L.zkg_msm_g1_shards_upload(_p(bases), self.n, d, len(devices))
        if not self._h:
            raise ZkgError("zkg_msm_g1_shards_upload failed: " + L.zkg_last_error().decode())

    def msm(self, scalars, with_partials=False):
        scalars = _u64(scalars); out = np.zeros(12, np.uint64); parts = np.zeros((self.ndev, 12), np.uint64)
        assert scalars.size // 4 == self.n
        _check(lib().zkg_msm_g1_multi(C.c_void_p(self._h), _p(scalars), _p(out), _p(parts)), "zkg_msm_g1_multi")
        return (out, parts) if with_partials else out

    def free(self):
        if self._h:
            lib().zkg_msm_g1_shards_free(C.c_void_p(self._h)); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


SCALARS_MONT, SCALARS_MOSTLY_BITS = 1, 2


def msm_g1_dev(d_bases, d_scalars, n, scalars_mont=False, stream=0, mostly_bits=False):
    out = np.zeros(12, np.uint64)
    flags = (SCALARS_MONT if scalars_mont else 0) | (SCALARS_MOSTLY_BITS if mostly_bits else 0)
    _check(lib().zkg_msm_g1_dev(_vp(d_bases), _vp(d_scalars), C.c_size_t(n), flags, _p(out), _vp(stream)), "zkg_msm_g1_dev")
    return out


def msm_g1_host_scalars(d_bases, scalars_host_ptr, n, scalars_mont=False, stream=0):
    """zkg_msm_g1_host_scalars: bases resident (device pointer), scalars at a HOST address (pinned memory lets the upload overlap the work)"""
    out = np.zeros(12, np.uint64)
    lib().zkg_msm_g1_host_scalars.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    _check(lib().zkg_msm_g1_host_scalars(_vp(d_bases), _vp(scalars_host_ptr), C.c_size_t(n), SCALARS_MONT if scalars_mont else 0, _p(out), _vp(stream)), "zkg_msm_g1_host_scalars")
    return out


def msm_host_scalars_stats():
    """zkg_msm_host_scalars_stats: the last msm_g1_host_scalars as a dict — pieces, stream_waits (cross-stream waits on the caller's stream),
    heavy (per piece: the heavy-bucket count the host read, None where it read none) and pair (per piece: the heavy kernels were launched)"""
    out = (C.c_uint32 * 18)()
    words = lib().zkg_msm_host_scalars_stats(out, 18)
    if words < 2:
        return None
    pieces = int(out[0])
    return {"pieces": pieces, "stream_waits": int(out[1]),
            "heavy": [None if out[2 + 2 * k] == 0xFFFFFFFF else int(out[2 + 2 * k]) for k in range(pieces)],
            "pair": [bool(out[3 + 2 * k]) for k in range(pieces)]}


class _ResidentBases:
    """zkg_msm_<group>_bases_upload / _resident / _resident_async / _resident_batch_max / _bases_free behind one class: _PREFIX is the entries'
    common prefix (zkg_msm_g1, zkg_msm_g2), _LIMBS the 64-bit limbs of a normalised point (12, 24)"""
    _PREFIX = None
    _LIMBS = 0

    def _fn(self, suffix, argtypes, restype=C.c_int):
        fn = getattr(lib(), self._PREFIX + suffix)
        fn.argtypes = argtypes; fn.restype = restype
        return fn

    def __init__(self, d_bases, n):
        self._h = self._fn("_bases_upload", [C.c_void_p, C.c_size_t], C.c_void_p)(_vp(d_bases), C.c_size_t(n))
        if not self._h:
            raise ZkgError(self._PREFIX + "_bases_upload failed: " + last_error())
        self.n = n

    def msm(self, d_scalars, scalars_mont=False, stream=0):
        """`stream`: the HIP stream whose queued work produced d_scalars (0 = the null stream); the job is ordered behind it"""
        out = np.zeros(self._LIMBS, np.uint64)
        fn = self._fn("_resident", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p])
        _check(fn(C.c_void_p(self._h), _vp(d_scalars), C.c_size_t(self.n), SCALARS_MONT if scalars_mont else 0, _p(out), _vp(stream)), self._PREFIX + "_resident")
        return out

    def msm_async(self, d_scalars_ptr, d_out_ptr, count=1, stride=None, scalars_mont=False, stream=0):
        """zkg_msm_g1_resident_async / zkg_msm_g2_resident_async: `count` vectors of n Fr, `stride` elements apart (default n), at the device
        address d_scalars_ptr; the normalised points (12 limbs each for G1, 24 for G2) are written to the device address d_out_ptr by work that
        `stream` is made to wait for.  Returns without waiting: synchronise `stream` before reading the points on the host."""
        fn = self._fn("_resident_async", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p])
        _check(fn(C.c_void_p(self._h), _vp(d_scalars_ptr), C.c_size_t(self.n), C.c_size_t(self.n if stride is None else stride),
                  C.c_size_t(count), SCALARS_MONT if scalars_mont else 0, _vp(d_out_ptr), _vp(stream)), self._PREFIX + "_resident_async")

    def batch_max(self):
        """zkg_msm_g1_resident_batch_max / zkg_msm_g2_resident_batch_max: scalar vectors that share one launch sequence on this handle"""
        return int(self._fn("_resident_batch_max", [C.c_void_p], C.c_size_t)(C.c_void_p(self._h)))

    def free(self):
        if self._h:
            self._fn("_bases_free", [C.c_void_p], None)(C.c_void_p(self._h)); self._h = None


class ResidentBases(_ResidentBases):
    """zkg_msm_g1_bases_upload / zkg_msm_g1_resident: fixed G1 bases (device pointer, n affine points) kept with their per-window tables"""
    _PREFIX = "zkg_msm_g1"
    _LIMBS = 12


class ResidentBasesG2(_ResidentBases):
    """zkg_msm_g2_bases_upload / zkg_msm_g2_resident: fixed G2 bases (device pointer, n affine points of 16 limbs) kept with their per-window tables"""
    _PREFIX = "zkg_msm_g2"
    _LIMBS = 24


def msm_resident_async_stats():
    """(vectors, launch groups, host waits) of the calling thread's last ResidentBases.msm_async"""
    out = (C.c_size_t * 3)()
    lib().zkg_msm_resident_async_stats(out)
    return tuple(int(v) for v in out)


def _msm_combine(name, limbs, records_jac, cpw, slots, chunk_log, vectors, slot_args):
    rec = _u64(records_jac)
    if rec.size != vectors * cpw * slots * limbs:
        raise ZkgError("%s: records_jac must hold vectors x cpw x %s points of %d limbs" % (name, "slots" if slot_args else slots, limbs))
    out = np.zeros((vectors, limbs), np.uint64)
    fn = getattr(lib(), "zkg_" + name)
    fn.argtypes = [C.c_void_p, C.c_size_t] + [C.c_int] * len(slot_args) + [C.c_int, C.c_size_t, C.c_void_p]
    _check(fn(_p(rec), C.c_size_t(cpw), *slot_args, int(chunk_log), C.c_size_t(vectors), _p(out)), "zkg_" + name)
    return out


def msm_combine_gpu(records_jac, cpw, slots, chunk_log, vectors=1):
    """zkg_msm_combine_gpu: the MSM's device epilogue alone.  records_jac: vectors x cpw x slots normalised G1 points (12 limbs) in the order
    vector, chunk, slot; returns (vectors, 12) normalised points."""
    return _msm_combine("msm_combine_gpu", 12, records_jac, cpw, slots, chunk_log, vectors, [int(slots)])


def msm_combine_g2_gpu(records_jac, cpw, chunk_log, vectors=1):
    """zkg_msm_combine_g2_gpu: the G2 MSM's device epilogue alone.  records_jac: vectors x cpw x 2 normalised G2 points (24 limbs) in the order
    vector, chunk, (P, U); returns (vectors, 24) normalised points."""
    return _msm_combine("msm_combine_g2_gpu", 24, records_jac, cpw, 2, chunk_log, vectors, [])


def msm_g1_windows_dev(d_bases, d_scalars, n, first_window, window_stride, scalars_mont=False, stream=0):
    """partial MSM over the Pippenger windows first_window, first_window + window_stride, ... (window-sharded multi-GPU variant)"""
    out = np.zeros(12, np.uint64)
    _check(lib().zkg_msm_g1_windows_dev(_vp(d_bases), _vp(d_scalars), C.c_size_t(n), int(scalars_mont), C.c_uint(first_window), C.c_uint(window_stride),
                                        _p(out), _vp(stream)), "zkg_msm_g1_windows_dev")
    return out


def msm_g2_dev(d_bases, d_scalars, n, scalars_mont=False, stream=0, mostly_bits=False):
    out = np.zeros(24, np.uint64)
    flags = (SCALARS_MONT if scalars_mont else 0) | (SCALARS_MOSTLY_BITS if mostly_bits else 0)
    _check(lib().zkg_msm_g2_dev(_vp(d_bases), _vp(d_scalars), C.c_size_t(n), flags, _p(out), _vp(stream)), "zkg_msm_g2_dev")
    return out


def g1_sum(points_jac):
    pts = _u64(points_jac); out = np.zeros(12, np.uint64)
    _check(lib().zkg_g1_sum(_p(pts), C.c_size_t(pts.size // 12), _p(out)), "zkg_g1_sum")
    return out


def g2_sum(points_jac):
    pts = _u64(points_jac); out = np.zeros(24, np.uint64)
    _check(lib().zkg_g2_sum(_p(pts), C.c_size_t(pts.size // 24), _p(out)), "zkg_g2_sum")
    return out


def fixed_base_g1_dev(base, d_scalars, n, d_out, stream=0):
    base = _u64(base)
    _check(lib().zkg_g1_fixed_base_dev(_p(base), _vp(d_scalars), C.c_size_t(n), _vp(d_out), _vp(stream)), "zkg_g1_fixed_base_dev")


def fixed_base_g2_dev(base, d_scalars, n, d_out, stream=0):
    base = _u64(base)
    _check(lib().zkg_g2_fixed_base_dev(_p(base), _vp(d_scalars), C.c_size_t(n), _vp(d_out), _vp(stream)), "zkg_g2_fixed_base_dev")


def timing_reset():
    lib().zkg_timing_reset()


def timing_dominant_ms():
    n = C.c_int(0)
    ms = lib().zkg_timing_dominant_ms(C.byref(n))
    return float(ms), n.value


# ---- Groth16 (r1cs_gg_ppzksnark_prover, snark.cpp:126) ---------------------------------------------
def make_r1cs(n, l, A, B, Cm, keep):
    """A, B, Cm = (rowptr uint32[C+1], col uint32[nnz], val uint64[nnz,4] Montgomery Fr); `keep` pins the arrays."""
    cs = R1CS()
    cs.num_variables, cs.num_inputs, cs.num_constraints = n, l, len(A[0]) - 1
    for name, (rp, col, val) in zip("abc", (A, B, Cm)):
        rp = np.ascontiguousarray(rp, np.uint32); col = np.ascontiguousarray(col, np.uint32); val = _u64(val)
        keep += [rp, col, val]
        setattr(cs, f"{name}_rowptr", rp.ctypes.data); setattr(cs, f"{name}_col", col.ctypes.data); setattr(cs, f"{name}_val", val.ctypes.data)
    return cs


def make_pk(cs, arrays, log_m, keep, domain_size=0):
    """domain_size: m when it is a step_radix2 size 2^(log_m-1) + 2^b; 0 for m = 2^log_m"""
    pk = PK(); pk.cs = cs; pk.log_m = log_m; pk.domain_size = domain_size
    for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "A_query", "B_g1", "B_g2", "H_query", "L_query"):
        a = _u64(arrays[k]); keep.append(a)
        setattr(pk, k, a.ctypes.data)
    return pk


class Crs:
    """Device-resident proving key (zkg_crs_upload): parsed once, reused for every proof."""

    def __init__(self, pk=None, blob=None, m=None, handle=None):
        """from a zkg_pk struct of flat arrays, from a libsnark pk byte blob (ctx->pk), or around a zkg_crs handle made elsewhere
        (groth16_setup_resident), which this object then owns"""
        if handle is not None:
            self._h = int(handle)
            self.m = m
        elif blob is not None:
            buf = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
            self._h = lib().zkg_crs_upload_blob(C.cast(buf, C.c_void_p), C.c_size_t(len(blob)))
            self.m = m
        else:
            self._h = lib().zkg_crs_upload(C.byref(pk))
            self.m = pk.domain_size or (1 << pk.log_m)
        if not self._h:
            raise ZkgError("zkg_crs_upload failed: " + lib().zkg_last_error().decode())

    def prove(self, witness, r, s, check_satisfied=True):
        """-> (rc, proof bytes); rc == UNSATISFIED (2): the gate of snark.cpp:121-124 refused the witness (libsnark_prove returns 1 there)."""
        out = np.zeros(256, np.uint8); ln = C.c_size_t(0)
        rc = lib().zkg_groth16_prove(C.c_void_p(self._h), _p(_u64(witness)), _p(_u64(r)), _p(_u64(s)), int(check_satisfied), _p(out), C.byref(ln))
        if rc not in (OK, UNSATISFIED):
            _check(rc, "zkg_groth16_prove")
        return rc, bytes(out[:ln.value])

    def prove_sparse(self, tags, full_index, full_values, r, s, check_satisfied=True):
        """zkg_groth16_prove_sparse: tags uint8[n] (0 zero, 1 one, 2 listed), listed variables as (index, 4 Montgomery limbs)"""
        tags = np.ascontiguousarray(tags, np.uint8); full_index = np.ascontiguousarray(full_index, np.uint32); full_values = _u64(full_values)
        out = np.zeros(256, np.uint8); ln = C.c_size_t(0)
        rc = lib().zkg_groth16_prove_sparse(C.c_void_p(self._h), _p(tags), _p(full_index), _p(full_values), C.c_size_t(full_index.size), _p(_u64(r)), _p(_u64(s)),
                                            int(check_satisfied), _p(out), C.byref(ln))
        if rc not in (OK, UNSATISFIED):
            _check(rc, "zkg_groth16_prove_sparse")
        return rc, bytes(out[:ln.value])

    def prove_batch(self, items, check_satisfied=True):
        """zkg_groth16_prove_batch: items are (witness, r, s) or (tags, full_index, full_values, r, s); -> [(status, proof bytes or None)]"""
        return groth16_prove_batch(self, items, check_satisfied)

    def prove_batch_zklaim(self, ctxs, rs, check_satisfied=True):
        """zkg_groth16_prove_batch_zklaim: credentials (ZklaimCtx, None: a null entry) of this key, witnesses made on the GPU; rs: (r, s) pairs of
        4 Montgomery limbs each -> [(status, proof bytes or None)]"""
        return groth16_prove_batch_zklaim(self, ctxs, rs, check_satisfied)

    def prove_zklaim(self, ctx, r, s, check_satisfied=True):
        """zkg_groth16_prove_zklaim: one credential (ZklaimCtx, None: a null context) of this key, its witness made on the GPU -> (rc, proof
        bytes or None): what prove_sparse gives on the host witness of ctx, ERROR included (no exception: the failures are the contract)"""
        L = lib()
        L.zkg_groth16_prove_zklaim.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        out = np.zeros(256, np.uint8); ln = C.c_size_t(0)
        rc = L.zkg_groth16_prove_zklaim(C.c_void_p(self._h), None if ctx is None else C.addressof(ctx), _p(_u64(r)), _p(_u64(s)), int(check_satisfied), _p(out), C.byref(ln))
        return rc, (bytes(out[:ln.value]) if rc == OK else None)

    def prove_dev(self, d_ptr, r, s, check_satisfied=True, stream=0):
        """zkg_groth16_prove_dev: the witness (n x 4 Montgomery limbs) at the raw DEVICE pointer d_ptr, proved behind what is queued on `stream`
        (a HIP stream handle, 0: the null stream) -> (rc, proof bytes or None): what prove gives on a host copy, ERROR included (no exception:
        the refusals are the contract)"""
        L = lib()
        L.zkg_groth16_prove_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        out = np.zeros(256, np.uint8); ln = C.c_size_t(0)
        rc = L.zkg_groth16_prove_dev(C.c_void_p(self._h), _vp(d_ptr), _p(_u64(r)), _p(_u64(s)), int(check_satisfied), _p(out), C.byref(ln), _vp(stream))
        return rc, (bytes(out[:ln.value]) if rc == OK else None)

    def prove_batch_dev(self, d_ptr, stride, count, rs, check_satisfied=True, stream=0):
        """zkg_groth16_prove_batch_dev: `count` witnesses at the raw DEVICE pointer d_ptr, `stride` Fr elements apart; rs: (r, s) pairs of 4
        Montgomery limbs each -> (rc, [(status, proof bytes or None)]): rc ERROR is a refused call (nothing was written)"""
        return groth16_prove_batch_dev(self, d_ptr, stride, count, rs, check_satisfied, stream)

    def prove_batch_chunk(self):
        """proofs per batched chunk for this key; 0: prove_batch takes the single-proof path"""
        lib().zkg_prove_batch_chunk.restype = C.c_size_t
        lib().zkg_prove_batch_chunk.argtypes = [C.c_void_p]
        return int(lib().zkg_prove_batch_chunk(C.c_void_p(self._h)))

    def shard_h(self, devices):
        """zkg_crs_shard_h: the H query's tables sharded by points over `devices` (one GPU listed several times rehearses the path)"""
        d = (C.c_int * len(devices))(*devices)
        lib().zkg_crs_shard_h.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _check(lib().zkg_crs_shard_h(C.c_void_p(self._h), d, len(devices)), "zkg_crs_shard_h")

    def qap_witness_h(self, witness):
        out = np.zeros((self.m + 1, 4), np.uint64)
        _check(lib().zkg_qap_witness_h(C.c_void_p(self._h), _p(_u64(witness)), _p(out)), "zkg_qap_witness_h")
        return out

    def stage_ms(self):
        ms = (C.c_float * 8)()
        _check(lib().zkg_prove_stage_ms(C.c_void_p(self._h), ms), "zkg_prove_stage_ms")
        return list(ms)

    def free(self):
        if self._h:
            lib().zkg_crs_free(C.c_void_p(self._h)); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- zklaim front-end structures (include/zklaim_abi.h) and the credential circuit --------------------------------
class ZklaimPayload(C.Structure):
    _fields_ = [("data_ref", C.c_uint64 * 5), ("data_op", C.c_int * 5), ("salt", C.c_uint64), ("hash", C.c_ubyte * 32), ("priv", C.c_uint8),
                ("pre", C.c_ubyte * 48)]


class ZklaimWrapPayload(C.Structure):
    pass


ZklaimWrapPayload._fields_ = [("next", C.POINTER(ZklaimWrapPayload)), ("pl", ZklaimPayload)]


class ZklaimCtx(C.Structure):
    _fields_ = [("num_of_payloads", C.c_size_t), ("pl_ctx_head", C.POINTER(ZklaimWrapPayload)), ("pk_size", C.c_size_t), ("pk", C.c_void_p),
                ("vk_size", C.c_size_t), ("vk", C.c_void_p), ("proof_size", C.c_size_t), ("proof", C.c_void_p), ("pub_key", C.c_ubyte * 32),
                ("signature", C.c_ubyte * 64)]


OPS = dict(less=1, less_or_eq=3, eq=2, greater_or_eq=10, greater=8, not_eq=9, noop=99)


def make_ctx(payloads, keep):
    """payloads: list of dicts(attrs=[5 u64], refs=[5 u64], ops=[5 names], salt=u64, hash=bytes|None).  hash None -> SHA-256(pre),
    as zklaim_hash_pl computes it (zklaim.c:114-121)."""
    import hashlib
    import struct
    ctx = ZklaimCtx()
    ctx.num_of_payloads = len(payloads)
    nodes = []
    for p in payloads:
        node = ZklaimWrapPayload()
        pre = struct.pack("<5QQ", *p["attrs"], p.get("salt", 0))
        node.pl.pre[:] = list(pre)
        for j in range(5):
            node.pl.data_ref[j] = p["refs"][j]
            node.pl.data_op[j] = OPS[p["ops"][j]]
        node.pl.salt = p.get("salt", 0)
        h = p.get("hash") or hashlib.sha256(pre).digest()
        node.pl.hash[:] = list(h)
        nodes.append(node)
    for a, b in zip(nodes, nodes[1:]):
        a.next = C.pointer(b)
    if nodes:
        ctx.pl_ctx_head = C.pointer(nodes[0])
    keep.append(nodes)
    return ctx


class ZklaimCircuit:
    """R1CS (+ witness) of zklaim_gadget for a zklaim_ctx, built on the host by libzkg.so"""

    def __init__(self, ctx, with_witness=True, witness_only=False, reference_quirk=False):
        L = lib()
        L.zkg_zklaim_circuit_new.restype = C.c_void_p
        L.zkg_zklaim_circuit_new.argtypes = [C.c_void_p, C.c_int]
        L.zkg_zklaim_witness_new.restype = C.c_void_p
        L.zkg_zklaim_witness_new.argtypes = [C.c_void_p]
        L.zkg_circuit_num_variables.restype = C.c_uint32
        L.zkg_circuit_num_variables.argtypes = [C.c_void_p]
        L.zkg_circuit_witness.restype = C.c_void_p
        L.zkg_circuit_first_unsatisfied.restype = C.c_long
        for f in (L.zkg_circuit_free, L.zkg_circuit_witness, L.zkg_circuit_is_satisfied, L.zkg_circuit_first_unsatisfied):
            f.argtypes = [C.c_void_p]
        L.zkg_circuit_r1cs.argtypes = [C.c_void_p, C.c_void_p]
        if witness_only:
            self._h = L.zkg_zklaim_witness_new(C.cast(C.pointer(ctx), C.c_void_p))
        else:
            self._h = L.zkg_zklaim_circuit_new(C.cast(C.pointer(ctx), C.c_void_p), (1 if with_witness else 0) | (2 if reference_quirk else 0))
        if not self._h:
            raise ZkgError("zkg_zklaim_circuit_new failed: " + L.zkg_last_error().decode())
        self.r1cs = R1CS()
        _check(L.zkg_circuit_r1cs(self._h, C.byref(self.r1cs)), "zkg_circuit_r1cs")
        if witness_only:
            self.r1cs.num_variables = L.zkg_circuit_num_variables(self._h)
        self.with_witness = with_witness

    def witness(self):
        p = lib().zkg_circuit_witness(self._h)
        if not p:
            return None
        n = self.r1cs.num_variables
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(n, 4)).copy()

    def sparse_witness(self):
        """-> (tags uint8[n], full_index uint32[count], full_values uint64[count,4]): the witness as zkg_groth16_prove_sparse takes it"""
        tags = C.POINTER(C.c_uint8)(); idx = C.POINTER(C.c_uint32)(); vals = C.POINTER(C.c_uint64)(); cnt = C.c_size_t(0)
        _check(lib().zkg_circuit_sparse_witness(C.c_void_p(self._h), C.byref(tags), C.byref(idx), C.byref(vals), C.byref(cnt)), "zkg_circuit_sparse_witness")
        n, c = self.r1cs.num_variables, cnt.value
        t = np.ctypeslib.as_array(tags, shape=(n,)).copy()
        i = np.ctypeslib.as_array(idx, shape=(c,)).copy() if c else np.zeros(0, np.uint32)
        v = np.ctypeslib.as_array(vals, shape=(c, 4)).copy() if c else np.zeros((0, 4), np.uint64)
        return t, i, v

    def is_satisfied(self):
        return bool(lib().zkg_circuit_is_satisfied(self._h))

    def first_unsatisfied(self):
        return int(lib().zkg_circuit_first_unsatisfied(self._h))

    def csr(self):
        """numpy copies of the three CSR matrices: (rowptr, col, val) x 3"""
        out = []
        C_ = self.r1cs.num_constraints
        for m in "abc":
            rp = np.ctypeslib.as_array(C.cast(getattr(self.r1cs, m + "_rowptr"), C.POINTER(C.c_uint32)), shape=(C_ + 1,)).copy()
            nnz = int(rp[-1])
            col = np.ctypeslib.as_array(C.cast(getattr(self.r1cs, m + "_col"), C.POINTER(C.c_uint32)), shape=(max(nnz, 1),))[:nnz].copy()
            val = np.ctypeslib.as_array(C.cast(getattr(self.r1cs, m + "_val"), C.POINTER(C.c_uint64)), shape=(max(nnz, 1), 4))[:nnz].copy()
            out.append((rp, col, val))
        return out

    def free(self):
        if self._h:
            lib().zkg_circuit_free(self._h); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def zklaim_input_map(ctx):
    L = lib()
    L.zkg_zklaim_input_map.restype = C.c_size_t
    L.zkg_zklaim_input_map.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    n = L.zkg_zklaim_input_map(C.cast(C.pointer(ctx), C.c_void_p), None, 0)
    out = np.zeros((n, 4), np.uint64)
    L.zkg_zklaim_input_map(C.cast(C.pointer(ctx), C.c_void_p), _p(out), n)
    return out


# ---- key generation / verification (r1cs_gg_ppzksnark_generator, r1cs_gg_ppzksnark_verifier_strong_IC) ------------------
class Keypair:
    def __init__(self, r1cs, trapdoor=None, dev=False):
        """dev: zkg_groth16_setup_dev, the generator whose scalars never leave the device (the same keypair byte for byte)"""
        L = lib()
        L.zkg_groth16_setup.restype = C.c_void_p
        L.zkg_groth16_setup.argtypes = [C.c_void_p, C.c_void_p]
        L.zkg_keypair_pk.restype = C.POINTER(PK)
        for f in (L.zkg_keypair_pk, L.zkg_keypair_free, L.zkg_keypair_swapped):
            f.argtypes = [C.c_void_p]
        for f in (L.zkg_keypair_pk_blob, L.zkg_keypair_vk_blob):
            f.restype = C.c_size_t; f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        td = None if trapdoor is None else _u64(trapdoor)
        entry = "zkg_groth16_setup_dev" if dev else "zkg_groth16_setup"
        if dev:
            L.zkg_groth16_setup_dev.restype = C.c_void_p
            L.zkg_groth16_setup_dev.argtypes = [C.c_void_p, C.c_void_p]
        self._h = getattr(L, entry)(C.byref(r1cs), _p(td))
        if not self._h:
            raise ZkgError(entry + " failed: " + L.zkg_last_error().decode())
        self.pk = L.zkg_keypair_pk(self._h).contents
        self.swapped = bool(L.zkg_keypair_swapped(self._h))

    def _blob(self, fn):
        n = fn(self._h, None, 0)
        out = np.zeros(n, np.uint8)
        assert fn(self._h, _p(out), n) == n
        return out.tobytes()

    def pk_blob(self): return self._blob(lib().zkg_keypair_pk_blob)
    def vk_blob(self): return self._blob(lib().zkg_keypair_vk_blob)

    def array(self, name, count, limbs):
        return np.ctypeslib.as_array(C.cast(getattr(self.pk, name), C.POINTER(C.c_uint64)), shape=(count, limbs)).copy()

    def free(self):
        if self._h:
            lib().zkg_keypair_free(self._h); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def groth16_setup_resident(cs, trapdoor=None, want_crs=True):
    """zkg_groth16_setup_resident: the key generated on the device and left there -> (pk_blob, vk_blob, Crs or None); the blobs are
    Keypair(cs, trapdoor)'s byte for byte, the Crs is the key Crs(blob=pk_blob) would load"""
    L = lib()
    L.zkg_groth16_setup_resident.argtypes = [C.c_void_p] * 7
    L.zkg_free.argtypes = [C.c_void_p]; L.zkg_free.restype = None
    td = None if trapdoor is None else _u64(trapdoor)
    pk = C.c_void_p(None); vk = C.c_void_p(None); crs = C.c_void_p(None); pk_len = C.c_size_t(0); vk_len = C.c_size_t(0)
    rc = L.zkg_groth16_setup_resident(C.byref(cs), _p(td), C.byref(pk), C.byref(pk_len), C.byref(vk), C.byref(vk_len), C.byref(crs) if want_crs else None)
    if rc != OK:
        assert not pk.value and not vk.value and not crs.value, "a failed zkg_groth16_setup_resident wrote an out-pointer"
        _check(rc, "zkg_groth16_setup_resident")
    try:
        blobs = C.string_at(pk.value, pk_len.value), C.string_at(vk.value, vk_len.value)
    finally:
        L.zkg_free(pk); L.zkg_free(vk)
    return blobs[0], blobs[1], (Crs(handle=crs.value, m=pk_blob_inspect(blobs[0])["domain_size"]) if want_crs else None)


def setup_resident_stats():
    """[scalars computed on the device (1 / 0), entries of the B query's non-zero list, Fr scalars uploaded for the query batches] of this
    thread's last groth16_setup_resident or libsnark_trusted_setup"""
    out = (C.c_size_t * 3)()
    lib().zkg_setup_resident_stats.argtypes = [C.c_void_p]
    lib().zkg_setup_resident_stats(out)
    return [int(v) for v in out]


def fr_nonzero_index(fr, where=1):
    """zkg_fr_nonzero_index: ascending positions of the elements of fr (raw limbs, any representative below 2r) that are not zero mod r;
    where 0: a host loop, 1: the generator's kernels"""
    fr = _u64(fr).reshape(-1, 4); n = fr.shape[0]
    out = np.zeros(max(n, 1), np.uint32); count = C.c_size_t(0)
    L = lib()
    L.zkg_fr_nonzero_index.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    _check(L.zkg_fr_nonzero_index(_p(fr) if n else None, C.c_size_t(n), int(where), _p(out), C.byref(count)), "zkg_fr_nonzero_index")
    return out[:count.value].copy()


def groth16_verify(vk_blob, primary_input, proof):
    """0 valid, 1 invalid, 2 malformed (host pairing; no GPU needed)"""
    L = lib()
    L.zkg_groth16_verify.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    vk = np.frombuffer(vk_blob, np.uint8).copy(); pr = np.frombuffer(proof, np.uint8).copy()
    x = _u64(primary_input)
    return L.zkg_groth16_verify(_p(vk), vk.size, _p(x) if x.size else None, x.size // 4, _p(pr), pr.size)


def pairing_probe(a, b):
    out = np.zeros(384, np.uint8)
    lib().zkg_pairing_probe(_p(_u64(a)), _p(_u64(b)), _p(out))
    return out.tobytes()


class VerifyItem(C.Structure):
    _fields_ = [("vk_blob", C.c_void_p), ("vk_len", C.c_size_t), ("primary_input", C.c_void_p), ("n_inputs", C.c_size_t),
                ("proof", C.c_void_p), ("proof_len", C.c_size_t)]


def groth16_verify_batch(items):
    """items: (vk_blob, primary_input, proof) triples.  Returns a uint8 array: verdicts[i] == groth16_verify(*items[i]) (0 valid,
    1 invalid, 2 malformed key), checked on the GPU as random linear combinations per key.  Raises ZkgError when the call fails."""
    L = lib()
    L.zkg_groth16_verify_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    arr = (VerifyItem * max(1, len(items)))()
    keep = []
    for k, (vk_blob, primary_input, proof) in enumerate(items):
        vk = np.frombuffer(bytes(vk_blob), np.uint8); pr = np.frombuffer(bytes(proof), np.uint8); x = _u64(primary_input)
        keep += [vk, pr, x]
        arr[k] = VerifyItem(vk.ctypes.data if vk.size else None, vk.size, x.ctypes.data if x.size else None, x.size // 4,
                            pr.ctypes.data if pr.size else None, pr.size)
    verdicts = np.full(max(1, len(items)), 0xFF, np.uint8)
    _check(L.zkg_groth16_verify_batch(C.cast(arr, C.c_void_p), len(items), _p(verdicts)), "zkg_groth16_verify_batch")
    return verdicts[:len(items)]


def verify_batch_stats():
    """(combined checks, items decided by the single verifier's code, of those: B outside G2) of this thread's last groth16_verify_batch"""
    out = (C.c_size_t * 3)()
    lib().zkg_verify_batch_stats(out)
    return tuple(int(v) for v in out)


def groth16_verify_each(items):
    """items: (vk_blob, primary_input, proof) triples.  Returns a uint8 array: verdicts[i] == groth16_verify(*items[i]) exactly, every
    item decided by its own pairing equation on the GPU (no weights, no bisection).  Raises ZkgError when the call fails."""
    L = lib()
    L.zkg_groth16_verify_each.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    arr = (VerifyItem * max(1, len(items)))()
    keep = []
    for k, (vk_blob, primary_input, proof) in enumerate(items):
        vk = np.frombuffer(bytes(vk_blob), np.uint8); pr = np.frombuffer(bytes(proof), np.uint8); x = _u64(primary_input)
        keep += [vk, pr, x]
        arr[k] = VerifyItem(vk.ctypes.data if vk.size else None, vk.size, x.ctypes.data if x.size else None, x.size // 4,
                            pr.ctypes.data if pr.size else None, pr.size)
    verdicts = np.full(max(1, len(items)), 0xFF, np.uint8)
    _check(L.zkg_groth16_verify_each(C.cast(arr, C.c_void_p), len(items), _p(verdicts)), "zkg_groth16_verify_each")
    return verdicts[:len(items)]


def verify_each_stats():
    """(items decided by the device equation, items decided by the single verifier's code, device rounds) of this thread's last groth16_verify_each"""
    out = (C.c_size_t * 3)()
    lib().zkg_verify_each_stats(out)
    return tuple(int(v) for v in out)


def verify_each_set_chunk(positions):
    """test hook: positions per device round of groth16_verify_each; 0 restores the default"""
    L = lib()
    L.zkg_verify_each_set_chunk.argtypes = [C.c_size_t]
    L.zkg_verify_each_set_chunk.restype = None
    L.zkg_verify_each_set_chunk(int(positions))


def pairing_each(g1, g2, pairs):
    """FE(prod_j ML(g1[i * pairs + j], g2[i * pairs + j])) per item i, Miller loops and final exponentiation on the GPU: g1 (items * pairs, 8),
    g2 (items * pairs, 16) affine Montgomery limbs (all-zero = infinity) -> a list of 384-byte values as pairing_probe's"""
    a = _u64(g1).reshape(-1, 8); b = _u64(g2).reshape(-1, 16)
    pairs = int(pairs)
    if a.shape[0] != b.shape[0] or pairs < 1 or a.shape[0] % pairs:
        raise ZkgError("pairing_each: g1 and g2 must hold items * pairs points each")
    items = a.shape[0] // pairs
    out = np.zeros((max(1, items), 384), np.uint8)
    L = lib()
    L.zkg_pairing_each.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    _check(L.zkg_pairing_each(_p(a) if a.size else None, _p(b) if b.size else None, items, pairs, _p(out)), "zkg_pairing_each")
    return [out[i].tobytes() for i in range(items)]


def final_exp(values, where):
    """the final exponentiation of serialised Fq12 values (384 bytes each) -> a list of 384-byte values.  where 0: the host's (the
    specification), 1: the GPU kernel, 2: the kernel's device code compiled for the host"""
    vals = [bytes(v) for v in values]
    if any(len(v) != 384 for v in vals):
        raise ZkgError("final_exp: every value is 384 bytes")
    buf = np.frombuffer(b"".join(vals), np.uint8).copy() if vals else np.zeros(0, np.uint8)
    out = np.zeros((max(1, len(vals)), 384), np.uint8)
    L = lib()
    L.zkg_final_exp.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    _check(L.zkg_final_exp(_p(buf) if buf.size else None, len(vals), int(where), _p(out)), "zkg_final_exp")
    return [out[i].tobytes() for i in range(len(vals))]


FQ12_OPS = {"mul": 0, "sqr": 1, "mul_by_line2": 2, "cyclotomic_sqr": 3, "inverse": 4, "conjugate": 5, "frobenius1": 6, "frobenius2": 7,
            "frobenius3": 8, "mul_by_v": 9}                                                                     # name -> op of zkg_fq12_op


def fq12_op(name, a, b=None, where=1):
    """one operation of the pairing's device tower on raw limbs (zkg_fq12_op): a is (n, 96) uint32, twelve Fq of eight little-endian words in
    the tower's order, taken as given; b likewise for "mul", and for "mul_by_line2" the line's three Fq2 in its first 48 words.  The
    result is (n, 96) uint32, not normalised.  where 1: the GPU kernel, 2: the same text on the host (canonical inputs only)"""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.ndim != 2 or a.shape[1] != 96:
        raise ZkgError(f"fq12_op {name}: a must be (n, 96), got {a.shape}")
    bb = None
    if name in ("mul", "mul_by_line2"):
        bb = np.ascontiguousarray(b, dtype=np.uint32)
        if bb.shape != a.shape:
            raise ZkgError(f"fq12_op {name}: b must be {a.shape}, got {bb.shape}")
    out = np.zeros((max(1, a.shape[0]), 96), np.uint32)
    L = lib()
    L.zkg_fq12_op.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    _check(L.zkg_fq12_op(FQ12_OPS[name], _p(a) if a.size else None, _p(bb) if bb is not None and bb.size else None, a.shape[0], int(where), _p(out)),
           "zkg_fq12_op")
    return out[:a.shape[0]]


class ProveItem(C.Structure):
    _fields_ = [("witness", C.c_void_p), ("tags", C.c_void_p), ("full_index", C.c_void_p), ("full_values", C.c_void_p), ("count", C.c_size_t),
                ("r", C.c_void_p), ("s", C.c_void_p)]


def groth16_prove_batch(crs, items, check_satisfied=True):
    """Proves every item on one resident key in one call (Crs.prove_batch).  items: (witness, r, s) for a dense witness of n x 4 limbs, or
    (tags, full_index, full_values, r, s) for the sparse form.  Returns [(status, proof bytes or None)]: status OK / UNSATISFIED / ERROR per
    item, as Crs.prove / Crs.prove_sparse would give for it alone.  Raises ZkgError when an item is malformed or the call itself fails."""
    L = lib()
    L.zkg_groth16_prove_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.zkg_crs_num_variables.argtypes = [C.c_void_p]
    L.zkg_crs_num_variables.restype = C.c_uint32
    handle = crs._h if crs is not None else None
    n = int(L.zkg_crs_num_variables(C.c_void_p(handle))) if handle else None
    arr = (ProveItem * max(1, len(items)))()
    keep = []

    def fr(x, what, k):
        a = _u64(x).reshape(-1)
        if a.size != 4:
            raise ZkgError(f"prove_batch: item {k}: {what} must be 4 limbs")
        return a
    for k, it in enumerate(items):
        if len(it) == 3:
            w = _u64(it[0]).reshape(-1, 4) if np.size(it[0]) % 4 == 0 else None
            if w is None or (n is not None and w.shape[0] != n):
                raise ZkgError(f"prove_batch: item {k}: the witness must be n x 4 limbs" + (f" (n = {n})" if n is not None else ""))
            r, s = fr(it[1], "r", k), fr(it[2], "s", k)
            keep += [w, r, s]
            arr[k] = ProveItem(w.ctypes.data if w.size else None, None, None, None, 0, r.ctypes.data, s.ctypes.data)
        elif len(it) == 5:
            tags = np.ascontiguousarray(it[0], np.uint8).reshape(-1); idx = np.ascontiguousarray(it[1], np.uint32).reshape(-1); vals = _u64(it[2]).reshape(-1, 4)
            if (n is not None and tags.size != n) or vals.shape[0] != idx.size:
                raise ZkgError(f"prove_batch: item {k}: tags must have n entries and every listed index its value")
            r, s = fr(it[3], "r", k), fr(it[4], "s", k)
            keep += [tags, idx, vals, r, s]
            arr[k] = ProveItem(None, tags.ctypes.data if tags.size else None, idx.ctypes.data if idx.size else None, vals.ctypes.data if vals.size else None,
                               idx.size, r.ctypes.data, s.ctypes.data)
        else:
            raise ZkgError(f"prove_batch: item {k}: (witness, r, s) or (tags, full_index, full_values, r, s)")
    proofs = np.zeros((max(1, len(items)), 134), np.uint8)
    status = np.full(max(1, len(items)), -1, np.int32)
    _check(L.zkg_groth16_prove_batch(C.c_void_p(handle), C.cast(arr, C.c_void_p), len(items), int(check_satisfied), _p(proofs), _p(status)), "zkg_groth16_prove_batch")
    return [(int(status[k]), proofs[k].tobytes() if status[k] == OK else None) for k in range(len(items))]


def _ctx_ptrs(ctxs):
    return (C.c_void_p * max(1, len(ctxs)))(*[None if c is None else C.addressof(c) for c in ctxs])


def groth16_prove_batch_zklaim(crs, ctxs, rs, check_satisfied=True):
    """Crs.prove_batch_zklaim.  Status per item as Crs.prove_sparse on the host witness of that context would give."""
    L = lib()
    L.zkg_groth16_prove_batch_zklaim.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    n = len(ctxs)
    rs_a = np.zeros((max(1, n), 8), np.uint64)
    if len(rs) != n:
        raise ZkgError("prove_batch_zklaim: one (r, s) per context")
    for k, (r, s) in enumerate(rs):
        r = _u64(r).reshape(-1); s = _u64(s).reshape(-1)
        if r.size != 4 or s.size != 4:
            raise ZkgError(f"prove_batch_zklaim: item {k}: r and s must be 4 limbs")
        rs_a[k, :4] = r; rs_a[k, 4:] = s
    proofs = np.zeros((max(1, n), 134), np.uint8)
    status = np.full(max(1, n), -1, np.int32)
    ptrs = _ctx_ptrs(ctxs)
    handle = crs._h if crs is not None else None
    _check(L.zkg_groth16_prove_batch_zklaim(C.c_void_p(handle), ptrs, n, _p(rs_a), int(check_satisfied), _p(proofs), _p(status)), "zkg_groth16_prove_batch_zklaim")
    return [(int(status[k]), proofs[k].tobytes() if status[k] == OK else None) for k in range(n)]


def groth16_prove_batch_dev(crs, d_ptr, stride, count, rs, check_satisfied=True, stream=0):
    """Crs.prove_batch_dev.  Pointer level: d_ptr is a device address (e.g. ``torch.Tensor.data_ptr()``), stream a HIP stream handle.  Status per
    item as Crs.prove on a host copy of that item would give."""
    L = lib()
    L.zkg_groth16_prove_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    count = int(count)
    if len(rs) != count:
        raise ZkgError("prove_batch_dev: one (r, s) per item")
    rs_a = np.zeros((max(1, count), 8), np.uint64)
    for k, (r, s) in enumerate(rs):
        r = _u64(r).reshape(-1); s = _u64(s).reshape(-1)
        if r.size != 4 or s.size != 4:
            raise ZkgError(f"prove_batch_dev: item {k}: r and s must be 4 limbs")
        rs_a[k, :4] = r; rs_a[k, 4:] = s
    proofs = np.zeros((max(1, count), 134), np.uint8)
    status = np.full(max(1, count), -1, np.int32)
    handle = crs._h if crs is not None else None
    rc = L.zkg_groth16_prove_batch_dev(C.c_void_p(handle), _vp(d_ptr), int(stride), count, _p(rs_a), int(check_satisfied), _p(proofs), _p(status), _vp(stream))
    return rc, [(int(status[k]), proofs[k].tobytes() if status[k] == OK else None) for k in range(count)]


def prove_dev_stats():
    """(witnesses split on the device from the caller's buffer, witnesses staged through host memory: always 0) of this thread's last
    Crs.prove_dev / Crs.prove_batch_dev"""
    out = (C.c_size_t * 2)()
    lib().zkg_prove_dev_stats(out)
    return tuple(int(v) for v in out)


def zklaim_witness_stats():
    """(items whose witness the GPU made, items whose witness the host made) of this thread's last prove_batch_zklaim / zklaim_prove_batch"""
    out = (C.c_size_t * 2)()
    lib().zkg_zklaim_witness_stats(out)
    return tuple(int(v) for v in out)


def zklaim_witness_size(payloads):
    """(variables, most listed per witness) of the credential circuit with that many payloads, as the generator counts them"""
    L = lib()
    L.zkg_zklaim_witness_size.restype = C.c_size_t
    L.zkg_zklaim_witness_size.argtypes = [C.c_size_t, C.c_void_p]
    cap = C.c_size_t(0)
    n = int(L.zkg_zklaim_witness_size(payloads, C.byref(cap)))
    if not n:
        raise ZkgError("zklaim_witness_size: payload count out of range")
    return n, int(cap.value)


def _witness_mirror(ctx, name):
    fn = getattr(lib(), name)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    n, cap = zklaim_witness_size(int(ctx.num_of_payloads))
    tags = np.zeros(n, np.uint8); idx = np.zeros(cap, np.uint32); vals = np.zeros((cap, 4), np.uint64); cnt = C.c_size_t(0)
    _check(fn(C.addressof(ctx), _p(tags), _p(idx), _p(vals), cap, C.byref(cnt)), name)
    return tags, idx[:cnt.value].copy(), vals[:cnt.value].copy()


def zklaim_witness_mirror(ctx):
    """zkg_zklaim_witness_mirror (no GPU): -> (tags uint8[n], full_index uint32[count], full_values uint64[count, 4]) as ZklaimCircuit.sparse_witness"""
    return _witness_mirror(ctx, "zkg_zklaim_witness_mirror")


def zklaim_witness_mirror_parallel(ctx):
    """zkg_zklaim_witness_mirror_parallel (no GPU): the same from k_zklaim_witness_par's code on the host, its slices run last one first"""
    return _witness_mirror(ctx, "zkg_zklaim_witness_mirror_parallel")


def prove_zklaim_stats():
    """(1 if the GPU made the witness, 1 if the host did) of this thread's last Crs.prove_zklaim / libsnark_prove"""
    out = (C.c_size_t * 2)()
    lib().zkg_prove_zklaim_stats(out)
    return tuple(int(v) for v in out)


def zklaim_witness_gpu_parallel(ctxs):
    """zkg_zklaim_witness_gpu_parallel: zklaim_witness_gpu on k_zklaim_witness_par"""
    return zklaim_witness_gpu(ctxs, "zkg_zklaim_witness_gpu_parallel")


def zklaim_witness_gpu(ctxs, name="zkg_zklaim_witness_gpu"):
    """zkg_zklaim_witness_gpu: the generator alone for contexts of one payload count (None: a null entry) -> one (tags, full_index, full_values)
    per context, or None where the context failed alone"""
    L = lib()
    fn = getattr(L, name)
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    k = next((int(c.num_of_payloads) for c in ctxs if c is not None), 0)
    if not k:
        raise ZkgError("zklaim_witness_gpu: no context")
    n, cap = zklaim_witness_size(k)
    cnt = len(ctxs)
    tags = np.zeros((cnt, n), np.uint8); idx = np.zeros((cnt, cap), np.uint32); vals = np.zeros((cnt, cap, 4), np.uint64)
    counts = (C.c_size_t * cnt)()
    _check(fn(_ctx_ptrs(ctxs), cnt, _p(tags), _p(idx), _p(vals), cap, counts), name)
    bad = C.c_size_t(-1).value
    if any(counts[i] == bad and tags[i].any() for i in range(cnt)):
        raise ZkgError(name + ": tags written for a context that failed")
    return [None if counts[i] == bad else (tags[i].copy(), idx[i, :counts[i]].copy(), vals[i, :counts[i]].copy()) for i in range(cnt)]


def prove_batch_stats():
    """(items through batched launches, items through the single-proof path, batched chunks) of this thread's last prove_batch"""
    out = (C.c_size_t * 3)()
    lib().zkg_prove_batch_stats(out)
    return tuple(int(v) for v in out)


def pairing_product(g1, g2):
    """FE(prod_i ML(g1[i], g2[i])): g1 (n, 8), g2 (n, 16) affine Montgomery limbs (all-zero = infinity); 384 bytes as pairing_probe"""
    a = _u64(g1).reshape(-1, 8); b = _u64(g2).reshape(-1, 16)
    if a.shape[0] != b.shape[0]:
        raise ZkgError("pairing_product: g1 and g2 differ in length")
    out = np.zeros(384, np.uint8)
    L = lib()
    L.zkg_pairing_product.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    _check(L.zkg_pairing_product(_p(a) if a.size else None, _p(b) if b.size else None, a.shape[0], _p(out)), "zkg_pairing_product")
    return out.tobytes()


def pairing_selfcheck(exponent):
    """0 when the Frobenius maps and the final exponentiation's last chunk agree with square-and-multiply (exponent: Python int)"""
    n = (exponent.bit_length() + 31) // 32
    e = np.array([(exponent >> (32 * i)) & 0xFFFFFFFF for i in range(n)], np.uint32)
    return lib().zkg_pairing_selfcheck(e.ctypes.data_as(C.c_void_p), n)


def libsnark_trusted_setup(ctx): return lib().libsnark_trusted_setup(C.byref(ctx))
def libsnark_prove(ctx): return lib().libsnark_prove(C.byref(ctx))
def libsnark_verify(ctx): return lib().libsnark_verify(C.byref(ctx))


def zklaim_prove_batch(ctxs):
    """zkg_zklaim_prove_batch: one libsnark_prove per ZklaimCtx (None: a null entry), grouped by key and batched -> [rc, ...]"""
    L = lib()
    L.zkg_zklaim_prove_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    n = len(ctxs)
    ptrs = (C.c_void_p * max(1, n))(*[None if c is None else C.addressof(c) for c in ctxs])
    rc = (C.c_int * max(1, n))(*([-1] * max(1, n)))
    _check(L.zkg_zklaim_prove_batch(ptrs, n, rc), "zkg_zklaim_prove_batch")
    return [int(rc[i]) for i in range(n)]


def zklaim_verify_batch(ctxs):
    """zkg_zklaim_verify_batch: one libsnark_verify per ZklaimCtx (None: a null entry), grouped by key and combined on the GPU -> [rc, ...]"""
    L = lib()
    L.zkg_zklaim_verify_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    n = len(ctxs)
    ptrs = _ctx_ptrs(ctxs)
    rc = (C.c_int * max(1, n))(*([-1] * max(1, n)))
    _check(L.zkg_zklaim_verify_batch(ptrs, n, rc), "zkg_zklaim_verify_batch")
    return [int(rc[i]) for i in range(n)]


def zklaim_verify_batch_stats():
    """(combined checks, items decided by the single verifier's code, items whose B is outside G2, items whose points and inputs the device
    front end produced) of this thread's last zklaim_verify_batch"""
    out = (C.c_size_t * 4)()
    lib().zkg_zklaim_verify_batch_stats(out)
    return tuple(int(v) for v in out)


def zklaim_verify_each(ctxs):
    """zkg_zklaim_verify_each: one libsnark_verify per ZklaimCtx (None: a null entry), every context by its own equation on the GPU -> [rc, ...]"""
    L = lib()
    L.zkg_zklaim_verify_each.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    n = len(ctxs)
    ptrs = _ctx_ptrs(ctxs)
    rc = (C.c_int * max(1, n))(*([-1] * max(1, n)))
    _check(L.zkg_zklaim_verify_each(ptrs, n, rc), "zkg_zklaim_verify_each")
    return [int(rc[i]) for i in range(n)]


def zklaim_verify_each_stats():
    """(items decided by the device equation, items decided by the single verifier's code, device rounds, key bit tables built) of this
    thread's last zklaim_verify_each"""
    out = (C.c_size_t * 4)()
    lib().zkg_zklaim_verify_each_stats(out)
    return tuple(int(v) for v in out)


def zklaim_ic_each(ic0, ic, ctxs, where=1):
    """zkg_zklaim_ic_each: ic0 (8,), ic (l, 8) affine Montgomery limbs (all-zero = infinity), contexts of one payload count ->
    (n, 8) limbs of -(IC_0 + sum_k x_ik IC_k).  where 1: the GPU's table build and k_zklaim_ic_each, 2: the same code on the host"""
    a0 = _u64(ic0).reshape(8); a = _u64(ic).reshape(-1, 8)
    k = next((int(c.num_of_payloads) for c in ctxs if c is not None), 0)
    if a.shape[0] != (1280 * k + 252) // 253:
        raise ZkgError("zklaim_ic_each: one IC point per input element of the first context")
    n = len(ctxs)
    out = np.zeros((max(1, n), 8), np.uint64)
    L = lib()
    L.zkg_zklaim_ic_each.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    _check(L.zkg_zklaim_ic_each(_p(a0), _p(a) if a.size else None, _ctx_ptrs(ctxs), n, int(where), _p(out)), "zkg_zklaim_ic_each")
    return out[:n]


def proof_decode_gpu(proofs):
    """zkg_proof_decode_gpu: proofs (n, 134) uint8 -> A (n, 8), B (n, 16), C (n, 8) affine Montgomery limbs and ok (n,) flag bytes
    (bit 0 A, bit 1 B, bit 2 C decoded)"""
    pr = np.ascontiguousarray(proofs, np.uint8).reshape(-1, 134)
    n = pr.shape[0]
    A = np.zeros((n, 8), np.uint64); B = np.zeros((n, 16), np.uint64); Cc = np.zeros((n, 8), np.uint64); ok = np.zeros(n, np.uint8)
    L = lib()
    L.zkg_proof_decode_gpu.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(L.zkg_proof_decode_gpu(_p(pr), n, _p(A), _p(B), _p(Cc), _p(ok)), "zkg_proof_decode_gpu")
    return A, B, Cc, ok


def point_decompress(records, stride, offset, n, g2, where=1):
    """zkg_point_decompress: n compressed records `stride` bytes apart, the point `offset` bytes into its record -> ((n, 8) or (n, 16)
    affine Montgomery limbs, flag word).  where 1: the key loader's kernels, 0: the host's decoder.  A refused record is all-zero and
    sets the flag."""
    buf = np.frombuffer(bytes(records), np.uint8)
    n = int(n)
    if buf.size < n * int(stride):
        raise ZkgError("point_decompress: fewer than n * stride bytes")
    out = np.zeros((max(1, n), 16 if g2 else 8), np.uint64); flag = C.c_uint32(0xFFFFFFFF)
    L = lib()
    L.zkg_point_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _check(L.zkg_point_decompress(_p(buf) if buf.size else None, int(stride), int(offset), n, int(g2), int(where), _p(out), C.byref(flag)), "zkg_point_decompress")
    return out[:n], int(flag.value)


def point_compress(g1, g2=None, idx=None, rec=34, where=1, n=None, guard=None):
    """zkg_point_compress: rec 34: G1 points (npoints, 8) -> n records of 34 bytes (n defaults to all); rec 100: record i = G2 g2[idx[i]]
    then G1 g1[idx[i]].  -> (n * rec bytes, the 16 guard bytes as they were found behind the run afterwards).  where 1: the key writer's
    kernels, 0: the host's writer."""
    a = _u64(g1).reshape(-1, 8); npoints = a.shape[0]
    b = None if g2 is None else _u64(g2).reshape(-1, 16)
    ix = None if idx is None else np.ascontiguousarray(idx, np.uint32).reshape(-1)
    if b is not None and b.shape[0] != npoints:
        raise ZkgError("point_compress: as many G2 points as G1 points")
    n = (npoints if ix is None else ix.size) if n is None else int(n)
    if ix is not None and ix.size < n:
        raise ZkgError("point_compress: fewer than n indices")
    out = np.zeros(max(1, n * int(rec)), np.uint8)
    g = np.frombuffer(bytes(guard) if guard is not None else bytes(16), np.uint8).copy()
    if g.size != 16:
        raise ZkgError("point_compress: the guard is 16 bytes")
    L = lib()
    L.zkg_point_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _check(L.zkg_point_compress(_p(a) if a.size else None, _p(b) if b is not None and b.size else None, _p(ix) if ix is not None and ix.size else None,
                                npoints, n, int(rec), int(where), _p(out), _p(g)), "zkg_point_compress")
    return out[:n * int(rec)].tobytes(), g.tobytes()


def zklaim_input_sums_gpu(ctxs, weights, mask=None, lo=0, hi=None):
    """zkg_zklaim_input_sums_gpu: contexts of one payload count, weights (n, 4) uint32, mask (n,) uint8 or None -> (l, 4) Montgomery Fr sums"""
    n = len(ctxs)
    hi = n if hi is None else hi
    w = np.ascontiguousarray(weights, np.uint32).reshape(-1, 4)
    if w.shape[0] != n:
        raise ZkgError("zklaim_input_sums_gpu: one weight per context")
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    if m is not None and m.size != n:
        raise ZkgError("zklaim_input_sums_gpu: one mask byte per context")
    k = next((int(c.num_of_payloads) for c in ctxs if c is not None), 1)
    cap = (1280 * max(k, 1) + 252) // 253 + 8
    out = np.zeros((cap, 4), np.uint64); cnt = C.c_size_t(0)
    L = lib()
    L.zkg_zklaim_input_sums_gpu.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    _check(L.zkg_zklaim_input_sums_gpu(_ctx_ptrs(ctxs), n, _p(w), _p(m), lo, hi, _p(out), cap, C.byref(cnt)), "zkg_zklaim_input_sums_gpu")
    return out[:cnt.value].copy()


def zklaim_input_map_mirror(ctx, count_only=False):
    """zkg_zklaim_input_map_mirror (no GPU): the device's bit rule on the host -> (l, 4) Montgomery Fr as zklaim_input_map; count_only: l"""
    L = lib()
    L.zkg_zklaim_input_map_mirror.restype = C.c_size_t
    L.zkg_zklaim_input_map_mirror.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    n = int(L.zkg_zklaim_input_map_mirror(C.addressof(ctx), None, 0))
    if count_only:
        return n
    out = np.zeros((n, 4), np.uint64)
    assert L.zkg_zklaim_input_map_mirror(C.addressof(ctx), _p(out), n) == n
    return out


def ctx_blob(ctx, which):
    size = getattr(ctx, which + "_size"); ptr = getattr(ctx, which)
    return C.string_at(ptr, size) if ptr and size else b""
