"""zklaim_amd — MI355X-native Groth16 prover hot path behind zklaim's C front-end.

The product is ``libzkg.so`` (hand-written HIP for gfx950 + the C ABI of ``include/zkg.h``).
This package is the thin ctypes mirror used by the tests and ``bench.py``; the arithmetic lives
in ``csrc/``.  There is no CPU fallback: importing works anywhere, but every compute entry point
raises unless the HIP library is built and a GPU is visible.
"""
from .api import (ZkgError, device_info, evaluation_domain_size, fixed_base_g1_dev, fixed_base_g2_dev, g1_sum, g2_sum, init, lib, msm_g1, msm_g1_dev, msm_g1_windows_dev,  # noqa: F401
                  msm_g2, msm_g2_dev, ntt, ntt_dev, shutdown, timing_dominant_ms, timing_reset, Crs, PK, R1CS, make_r1cs, make_pk,
                  DECLARED_SYMBOLS, Prover, prover_stats, proof_assemble, ZklaimCircuit, ZklaimCtx, make_ctx, zklaim_input_map, OPS, Keypair, groth16_verify, groth16_verify_batch, verify_batch_stats, groth16_prove_batch, prove_batch_stats, groth16_prove_batch_dev, prove_dev_stats, groth16_prove_batch_zklaim, zklaim_witness_stats, zklaim_witness_size, zklaim_witness_mirror, zklaim_witness_gpu, zklaim_witness_mirror_parallel, zklaim_witness_gpu_parallel, prove_zklaim_stats, pairing_product, pairing_probe, pairing_selfcheck,
                  libsnark_trusted_setup, libsnark_prove, libsnark_verify, zklaim_prove_batch, zklaim_verify_batch, zklaim_verify_batch_stats, proof_decode_gpu, zklaim_input_sums_gpu, zklaim_input_map_mirror, ctx_blob, COMPAT_SYMBOLS, field_op, fr29_op, FR29_OPS, fq29_op, FQ29_OPS, g1_add_quad29, g1_add_pair29, curve_op, CURVE_OPS, OK, ERROR, UNSATISFIED, init_multi, MsmShards, pk_blob_inspect, ResidentBases, msm_g1_host_scalars, msm_host_scalars_stats, msm_resident_async_stats, msm_combine_gpu, ResidentBasesG2, msm_combine_g2_gpu,
                  groth16_verify_each, verify_each_stats, verify_each_set_chunk, pairing_each, final_exp, fq12_op, FQ12_OPS,
                  point_decompress, point_compress, zklaim_verify_each, zklaim_verify_each_stats, zklaim_ic_each,
                  Domain, domain_stats, Qap, qap_stats, qap_instance_stats,
                  groth16_setup_resident, setup_resident_stats, fr_nonzero_index)
