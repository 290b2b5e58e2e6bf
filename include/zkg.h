/*
 * zkg.h — C ABI of the MI355X-native Groth16 prover hot path (alt_bn128).
 *
 * This is the drop-in boundary below zklaim's prover call
 *     r1cs_gg_ppzksnark_prover<ppT>(proving_key, primary_input, auxiliary_input)
 * at /root/reference/zklaim/snark.cpp:126 (reached from libsnark_prove,
 * zklaim/libsnark_wrapper.cpp:218-249, reached from zklaim_proof_generate,
 * zklaim/zklaim.c:77-80).  Everything above that call stays host C/C++; everything
 * below it is hand-written HIP for gfx950 behind the functions declared here.
 * Each entry point names the libsnark / libff / libfqfft function it replaces; those
 * live in the un-vendored submodule lib/libsnark (.gitmodules:1-6) and are cited by
 * the reference call site that reaches them.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types; never throws; 0 == success
 *     (ZKLAIM_OK, zklaim/zklaim.h:38), non-zero == failure (ZKLAIM_ERROR semantics).
 *   - Field element (Fq or Fr): 4 x uint64_t little-endian limbs, MONTGOMERY form with
 *     R = 2^256 — the in-memory form of libff's Fp_model<4,...> — unless a parameter
 *     says "canonical".
 *   - G1 affine: 8 limbs  X||Y.   G2 affine: 16 limbs  X.c0||X.c1||Y.c0||Y.c1.
 *     The point at infinity is encoded as all-zero limbs ((0,0) is not on either curve).
 *   - "jac" outputs: X||Y||Z, NORMALISED (Z == Montgomery one) or infinity == (0, one, 0),
 *     i.e. what libff's to_affine_coordinates() leaves behind.  Normalised output is what
 *     makes results byte-comparable between the HIP path and the CPU oracle.
 *   - *_dev entry points take DEVICE pointers (hipMalloc'd, or torch tensor data_ptr())
 *     and a hipStream_t passed as void*; all others take HOST pointers and stage
 *     internally.
 */
#ifndef ZKG_H
#define ZKG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKG_OK 0
#define ZKG_ERROR 1          /* generic failure (bad argument, HIP error)            */
#define ZKG_UNSATISFIED 2    /* zkg_groth16_prove*: the witness violates the constraint
                                system and no proof was made.  A code of its own, so that
                                callers never have to tell it from ZKG_ERROR by the error
                                text; the seam maps it to the reference's return value 1
                                (libsnark_prove, zklaim/libsnark_wrapper.cpp:233-240)   */
#define ZKG_PROOF_BYTES 134  /* G1(34) || G2(66) || G1(34), see zkg_groth16_prove    */

/* ---- R1CS in CSR form (three matrices).  Column 0 is the constant ONE, columns
 *      1..num_inputs the primary input, the rest the auxiliary input: the layout of
 *      libsnark's r1cs_constraint_system + variable indices (used through
 *      pb.get_constraint_system(), snark.cpp:87).                                    */
typedef struct zkg_r1cs {
    uint32_t num_variables;    /* n, excluding the constant                           */
    uint32_t num_inputs;       /* l                                                   */
    uint32_t num_constraints;  /* C                                                   */
    uint32_t reserved;
    const uint32_t *a_rowptr, *a_col; const uint64_t *a_val;   /* rowptr[C+1], col[nnz], val[nnz*4] (Fr) */
    const uint32_t *b_rowptr, *b_col; const uint64_t *b_val;
    const uint32_t *c_rowptr, *c_col; const uint64_t *c_val;
} zkg_r1cs;

/* ---- Proving key material as flat host arrays: the fields of
 *      r1cs_gg_ppzksnark_proving_key<ppT> (imported at libsnark_wrapper.cpp:160-168).
 *      B_query is libsnark's sparse knowledge_commitment_vector<G2,G1> densified:
 *      absent entries are infinity.                                                   */
typedef struct zkg_pk {
    zkg_r1cs cs;               /* the (possibly A/B-swapped) system stored in the pk   */
    uint32_t log_m;            /* ceil(log2 m) of the evaluation domain size m         */
    uint32_t domain_size;      /* m as libfqfft's get_evaluation_domain(C+l+1) picks it:
                                  2^log_m (basic_radix2_domain; 0 means the same) or
                                  2^(log_m-1) + 2^b, b < log_m-1 (step_radix2_domain)   */
    const uint64_t *alpha_g1, *beta_g1, *delta_g1;   /* 8 limbs each                   */
    const uint64_t *beta_g2, *delta_g2;              /* 16 limbs each                  */
    const uint64_t *A_query;   /* (n+1) x 8                                            */
    const uint64_t *B_g1;      /* (n+1) x 8                                            */
    const uint64_t *B_g2;      /* (n+1) x 16                                           */
    const uint64_t *H_query;   /* (m-1) x 8                                            */
    const uint64_t *L_query;   /* (n-l) x 8                                            */
} zkg_pk;

typedef struct zkg_crs zkg_crs;   /* opaque: device-resident proving key + domain tables */

/* ---- lifecycle -------------------------------------------------------------------- */
/* Replaces ppT::init_public_params() (libsnark_wrapper.cpp:204,227,259).  Selects HIP
 * device `device` (>=0) for the calling process (one process per GPU), uploads constant
 * tables.  Re-entrant; fails (non-zero) if no HIP device is usable — there is no CPU
 * fallback behind this ABI.                                                            */
int  zkg_init(int device);
void zkg_shutdown(void);
const char *zkg_last_error(void);
/* number of compute units / device name of the device zkg_init selected (diagnostics) */
int  zkg_device_info(char *name, size_t name_len, int *compute_units);

/* ---- NTT: libfqfft basic_radix2_domain<Fr>::FFT / iFFT / cosetFFT / icosetFFT
 *      (reached from r1cs_to_qap_witness_map inside the call at snark.cpp:126).
 *      a: N = 2^logN Fr elements, Montgomery, natural order in and out, in place.
 *      inverse: 0 forward, 1 inverse (includes the 1/N scaling).
 *      coset:   0 plain, 1 coset with g = Fr::multiplicative_generator (= 5).         */
int zkg_ntt(uint64_t *a, unsigned logN, int inverse, int coset);
int zkg_ntt_dev(void *d_a, unsigned logN, int inverse, int coset, void *stream);

/* ---- Domain choice and the non-power-of-two case.
 *      zkg_evaluation_domain_size: libfqfft::get_evaluation_domain(min_size) as
 *      r1cs_to_qap_instance_map / _witness_map call it with min_size = C + l + 1
 *      (inside snark.cpp:91 and :126): *m = the domain size, *is_step = 1 when it is a
 *      step_radix2_domain (m = 2^a + 2^b, b < a) instead of a basic_radix2_domain.
 *      zklaim's circuit lands on a step domain for 11 of its 20 payload counts
 *      (e.g. 3 payloads: m = 2^16 + 2^15).
 *      zkg_ntt_domain: the same four transforms as zkg_ntt on the domain of size m,
 *      m = 2^k or 2^a + 2^b: libfqfft step_radix2_domain<Fr>::FFT / iFFT / cosetFFT /
 *      icosetFFT for the latter.  a: m Fr elements, Montgomery, in place.             */
int zkg_evaluation_domain_size(size_t min_size, size_t *m, int *is_step);
int zkg_ntt_domain(uint64_t *a, size_t m, int inverse, int coset);
int zkg_ntt_domain_dev(void *d_a, size_t m, int inverse, int coset, void *stream);

/* ---- One evaluation domain as a handle: many transforms per call and the Lagrange coefficients, on the caller's stream.
 *      zkg_domain_new(m): m as zkg_ntt_domain takes it (2^k, k <= 28, or 2^a + 2^b; m >= 2).  The handle lives on the calling thread's device,
 *      which must be the zkg_init device (the twiddle and coset tables are the process-wide ones zkg_ntt* use; they are built here if they
 *      are not there yet).  NULL on failure, with zkg_last_error set.  zkg_domain_free waits for the handle's pending work; NULL is accepted.
 *      zkg_domain_size: m (0 for NULL).
 *      zkg_domain_ntt_async: `count` in-place transforms.  Vector i is m Fr elements, Montgomery, at d_a + i * stride * 32 bytes, stride >= m,
 *      the base aligned to 16 bytes; what lies between m and the stride is never read or written.  inverse / coset as in zkg_ntt_domain.
 *      Once the work has run every vector holds exactly what zkg_ntt_domain_dev writes for that vector alone, bit for bit (the same kernels,
 *      with the vectors of a group in grid.y).  The vectors are cut into groups of at most zkg_domain_batch_max, one launch sequence each;
 *      the default is min(65535, 1 GiB / (m * 40 bytes)), at least 1.
 *      Ordering: the kernels are queued on `stream` (NULL: the null stream) behind everything already there, and the call does not wait on
 *      the host: synchronise `stream` before the host reads the result.  A handle serves its calls in call order whatever streams they name:
 *      each call leaves the handle's event behind its last kernel (that launch carries it as its completion), and a later call on another
 *      stream makes that stream wait for it first — this is what keeps two streams out of the handle's one scratch buffer.  The handle owns that inter-pass scratch (40 bytes per element of a
 *      group, packed whatever the stride); it only grows.  A call that needs more of it waits for the handle's event, reallocates and counts
 *      one host wait; a call at a group size the handle has served neither waits nor allocates.
 *      Refused with ZKG_ERROR before any launch, nothing written: a null handle or pointer; stride < m; more than 2^24 vectors or a stride
 *      above 2^32 elements; a calling thread whose current device is not the handle's; a pointer that hipPointerGetAttributes does not
 *      report as device memory of that device (pinned, managed and unregistered host memory are all refused), that is misaligned, or whose
 *      range runs past the end of its allocation where hipMemGetAddressRange knows it.  count == 0 is ZKG_OK and touches nothing.
 *      zkg_domain_lagrange_async: libfqfft evaluate_all_lagrange_polynomials(t) into d_u (DEVICE, m Fr) and, where d_z is not NULL,
 *      compute_vanishing_polynomial(t) into d_z (DEVICE, one Fr): fully reduced Montgomery limbs, the values the key generator's host loop
 *      computes, from one kernel (Montgomery's trick per lane over a run of consecutive elements).  t: Montgomery Fr in HOST memory, read
 *      during the call.  Z(t) is computed on the host first: for a domain point (Z(t) = 0) the call is ZKG_ERROR before any launch.
 *      Ordering and refusals as above; the call makes no host wait.                                                                       */
typedef struct zkg_domain zkg_domain;
zkg_domain *zkg_domain_new(size_t m);
void   zkg_domain_free(zkg_domain *d);
size_t zkg_domain_size(const zkg_domain *d);
size_t zkg_domain_batch_max(const zkg_domain *d);   /* vectors one launch sequence takes; >= 1, 0 for NULL */
void   zkg_domain_set_batch_max(zkg_domain *d, size_t k);   /* test hook: k vectors per launch sequence from now on; 0 restores the default, a larger k is clamped to it */
int zkg_domain_ntt_async(zkg_domain *d, void *d_a, size_t stride /* Fr elements between vectors, >= m */, size_t count,
                         int inverse, int coset, void *stream);
int zkg_domain_lagrange_async(zkg_domain *d, const uint64_t t[4], void *d_u, void *d_z, void *stream);
/* test hook: the calling thread's last zkg_domain_ntt_async — out[0] vectors enqueued, out[1] launch groups, out[2] host waits the entry
 * made.  Counters, not clocks.                                                                                                           */
void zkg_domain_stats(size_t out[3]);

/* ---- r1cs_to_qap_witness_map on device-resident witnesses, as a handle on a constraint system alone (no proving key): three mat-vecs, three
 *      iFFT, three cosetFFT, (A.B - C)/Z on the coset and the icosetFFT, for many witnesses per call, on the caller's stream.
 *      zkg_qap_new(cs): the CSR matrices in HOST memory, copied to the device; the domain is get_evaluation_domain(C + l + 1).  The handle lives
 *      on the zkg_init device, which must be the calling thread's; the domain tables are built as zkg_domain_new builds them, with the fused
 *      g^i / m table of a radix-2 domain and the list of the rows above 24 terms (one wavefront per row).  NULL, with zkg_last_error set: no
 *      zkg_init; a null CSR; num_constraints == 0 or num_variables == 0; num_inputs > num_variables; C + l + 1 with no radix-2 or step domain;
 *      a row pointer that does not start at 0 or decreases; a column index above num_variables (checked here, on the host, once: the kernels
 *      index z by it).  The system is taken as given: there is no swap_AB_if_beneficial (H does not depend on the swap).
 *      zkg_qap_free waits for the handle's pending work; NULL is accepted; callable from any device.
 *      zkg_qap_domain_size: m.  zkg_qap_num_variables: n.  Both 0 for NULL.
 *      zkg_qap_witness_h_async: witness i is n Fr, Montgomery, at d_witnesses + i * stride * 32 bytes, stride >= n — the layout
 *      zkg_groth16_prove_dev takes.  It is read in place: the constant z[0] = 1 is supplied by the kernel, and what lies between n and the stride
 *      is never read.  coefficients_for_H of witness i, m + 1 Fr, goes to d_h + i * h_stride * 32 bytes, h_stride >= m + 1: the limbs
 *      zkg_qap_witness_h writes for a host copy of that witness on a key over the same system, bit for bit, coefficients_for_H[m] = 0 included;
 *      what lies between m + 1 and h_stride is never written.  d_unsat (DEVICE, `count` 32-bit words, or NULL): every word is written — 0 for
 *      a satisfied witness, 1 where some row has <A,z><B,z> != <C,z> (the pb.is_satisfied() gate).  H is written for such a witness all the same
 *      (the map is defined on it) and the other witnesses of the call are not affected.
 *      The witnesses are cut into groups of at most zkg_qap_batch_max, one launch sequence each (mat-vec with the witness in grid.y, the seven
 *      transforms as batches of 3 g and g vectors, the pointwise step writing into d_h, the icosetFFT in place there).  A group's workspace is
 *      3 m Fr of aA | aB | aC plus the transforms' 40 bytes per element, 216 m bytes per witness; the default group is
 *      max(1, min(65535 / 3, 1 GiB / (m * 216 bytes))) — 65535 / 3 because grid.y of the batched transforms carries 3 g vectors.
 *      Ordering is zkg_domain's: the kernels are queued on `stream` behind everything already there and the call makes no host wait; a handle
 *      serves its calls in call order whatever streams they name (one workspace: each call leaves the handle's event in its last launch, and a
 *      later call on another stream makes that stream wait for it first).  The workspace only grows; a call that needs more of it waits for
 *      the handle's event, reallocates and counts one host wait; a call at a group size the handle has served neither waits nor allocates.
 *      Refused with ZKG_ERROR before any launch, nothing written: a null handle or pointer (d_unsat may be NULL); stride < n or
 *      h_stride < m + 1; more than 2^24 witnesses or a stride above 2^32 elements; a calling thread on another device than the handle's; a
 *      pointer that is not device memory of that device, is misaligned (16 bytes; 4 for d_unsat) or runs past the end of its allocation
 *      (zkg_domain_ntt_async's rules); ranges of d_witnesses, d_h and d_unsat that overlap.  count == 0 is ZKG_OK and touches nothing.       */
typedef struct zkg_qap zkg_qap;
zkg_qap *zkg_qap_new(const zkg_r1cs *cs);
void     zkg_qap_free(zkg_qap *q);
size_t   zkg_qap_domain_size(const zkg_qap *q);
uint32_t zkg_qap_num_variables(const zkg_qap *q);
size_t   zkg_qap_batch_max(const zkg_qap *q);     /* witnesses one launch sequence takes; >= 1, 0 for NULL */
void     zkg_qap_set_batch_max(zkg_qap *q, size_t k);   /* test hook: k witnesses per launch sequence from now on; 0 restores the default, a larger k is clamped to it */
int      zkg_qap_witness_h_async(zkg_qap *q, const void *d_witnesses, size_t stride /* Fr elements between witnesses, >= n */, size_t count,
                                 void *d_h, size_t h_stride /* Fr elements between outputs, >= m + 1 */, uint32_t *d_unsat /* DEVICE, count words, or NULL */,
                                 void *stream);
/* test hook: the calling thread's last zkg_qap_witness_h_async — out[0] witnesses enqueued, out[1] launch groups, out[2] host waits the entry
 * made.  Counters, not clocks.                                                                                                           */
void     zkg_qap_stats(size_t out[3]);
/* ---- the other half of the QAP reduction on the same handle: r1cs_to_qap_instance_map_with_evaluation, the QAP polynomials at a point t.
 *      With u = evaluate_all_lagrange_polynomials(t) on the handle's domain: At[j] = sum_i u[i] A[i][j] (+ u[C + j] for j <= l, the
 *      input-consistency rows), Bt[j] = sum_i u[i] B[i][j], Ct[j] = sum_i u[i] C[i][j], j = 0 .. n with column 0 the constant — for the system as
 *      the handle holds it (no swap_AB_if_beneficial).  t: 4 limbs in HOST memory, Montgomery, read during the call.  Vector k of At | Bt | Ct,
 *      n + 1 Fr, goes to d_abc + k * stride * 32 bytes, stride >= n + 1; d_z (or NULL) receives Z(t).  Everything written is a fully reduced
 *      Montgomery element; a column no row touches is exactly zero; what lies between n + 1 and the stride is never written.
 *      It is a transposed sparse mat-vec, so the handle needs its matrices by columns.  That index — per matrix n + 2 column pointers and, per
 *      entry, the row and the position of its coefficient in the row-major values the handle already holds (the 32-byte values are not copied)
 *      — is built on the device by the FIRST instance call of a handle, which waits for it once on the host (zkg_qap_instance_stats counts
 *      both); zkg_qap_new and handles used for H alone pay nothing.  It is made with atomics (degree count, exclusive scan, scatter through
 *      per-column cursors), so the order of the entries inside a column differs from build to build; the sums are exact in Fr and every result
 *      is reduced to [0, r) on the way out, so the output does not depend on that order.
 *      A call queues: the Lagrange kernel (u into the handle's workspace, m Fr), one lane per column over the three matrices (the u[C + j] term
 *      added there), and — when some column has more than LONG_COLUMN = 24 terms — one wavefront per segment of such a column (lanes stride
 *      over the terms, shuffle reduction; a column is cut into segments of 2048 terms, zklaim's constant column in B holds a term of every
 *      bitness row) and a closing launch that sums a column's partial sums, one wavefront per column.  Ordering, the event and the grow-only
 *      workspace are zkg_qap_witness_h_async's: instance and H calls on one handle run in call order whatever streams they name.
 *      Refused with ZKG_ERROR before any launch, nothing written: a null handle, t or d_abc; stride < n + 1 or above 2^32; a calling thread on
 *      another device than the handle's; d_abc or d_z that is not device memory of that device, is not 16-byte aligned or runs past the end of
 *      its allocation; d_z inside d_abc's range; a t with Z(t) = 0 (a point of the domain).                                                  */
int      zkg_qap_instance_async(zkg_qap *q, const uint64_t t[4] /* HOST, Montgomery */, void *d_abc /* DEVICE: At | Bt | Ct */,
                                size_t stride /* Fr elements between the three vectors, >= n + 1 */, void *d_z /* DEVICE, one Fr, or NULL */, void *stream);
/* test hook: long columns are cut into segments of k terms from the next instance call on (which rebuilds the segment list behind the handle's
 * pending work and counts one host wait); 0 restores the default 2048, k below 64 is taken as 64, above 2^20 as 2^20                        */
void     zkg_qap_set_column_segment(zkg_qap *q, size_t k);
/* test hook: the calling thread's last zkg_qap_instance_async — out[0] column indexes built (1 on a handle's first call), out[1] host waits */
void     zkg_qap_instance_stats(size_t out[2]);

/* ---- MSM: libff::multi_exp<G1,Fr,multi_exp_method_BDLO12> and
 *      multi_exp_with_mixed_addition (A/H/L queries), and the G2 half of
 *      kc_multi_exp_with_mixed_addition (B query); reached from snark.cpp:126.
 *      bases: affine Montgomery; scalars: N x 4 limbs, CANONICAL (as_bigint()) values
 *      in [0, r).  out: normalised jac.                                               */
int zkg_msm_g1(const uint64_t *bases, const uint64_t *scalars, size_t n, uint64_t out_jac[12]);
int zkg_msm_g2(const uint64_t *bases, const uint64_t *scalars, size_t n, uint64_t out_jac[24]);
/* device-resident inputs.  scalars_mont is a set of flags:
 *   ZKG_SCALARS_MONT         the scalars are Montgomery Fr (a witness vector), converted on the fly;
 *   ZKG_SCALARS_MOSTLY_BITS  the caller knows most scalars are 0 or 1 — libff's
 *                            multi_exp_with_mixed_addition case (A / B / L queries over a witness), as opposed to plain multi_exp
 *                            (H query): the digits are then sorted in one pass; the two-pass sort that is faster for uniformly
 *                            random scalars degrades when half of them share a digit.  The result never depends on the flag.
 * The result is written to HOST memory (out_jac) after the stream is synchronised.     */
#define ZKG_SCALARS_MONT 1
#define ZKG_SCALARS_MOSTLY_BITS 2
int zkg_msm_g1_dev(const void *d_bases, const void *d_scalars, size_t n, int scalars_mont,
                   uint64_t out_jac[12], void *stream);
int zkg_msm_g2_dev(const void *d_bases, const void *d_scalars, size_t n, int scalars_mont,
                   uint64_t out_jac[24], void *stream);
/* Bases resident on the device, scalars in HOST memory: the step SURVEY.md section 8(d) times ("wall clock around the call incl. H2D of
 * scalars; bases resident") — what a prover with a resident key does per proof when the scalars come from the host.  `scalars`: n x 4
 * canonical limbs (or Montgomery with ZKG_SCALARS_MONT) in host memory; page-locked memory (hipHostMalloc / hipHostRegister) lets the upload
 * run under the work: from 2^19 points on the job is cut by points into four pieces whose uploads overlap the sort and accumulation of the
 * pieces before them, all accumulating into one set of buckets (pageable memory works, without the overlap).  Same point as zkg_msm_g1_dev on
 * the uploaded vector, bit for bit.  `stream` as in zkg_msm_g1_dev; the result is in out_jac when the call returns.  The calling thread
 * is busy for the length of the call: it enqueues each piece's accumulation once that piece's sort has finished.
 * Ordering of `scalars`: page-locked scalars may be produced by work queued on `stream` before the call (a device-to-host copy, say) — at
 * every n the uploads are ordered behind that work, and no wait is put on `stream` for it.  Pageable memory is read at call time, as
 * hipMemcpyAsync reads it: it must hold the scalars when the call is made.                                                              */
int zkg_msm_g1_host_scalars(const void *d_bases, const uint64_t *scalars, size_t n, int scalars_mont, uint64_t out_jac[12], void *stream);
/* test hook: what the last zkg_msm_g1_host_scalars of the process did.  The calling thread paces a piece-wise job: it enqueues an accumulation
 * only once that piece's digit sort has finished, and reads the piece's count of heavy buckets (lists above the accumulation's threshold) from
 * a word the sort stored in the library's pinned memory — the two heavy-bucket kernels are launched behind an accumulation only where that
 * count is not zero.  out[0]: pieces run (1: the single-launch path); out[1]: cross-stream waits enqueued on the caller's stream (0 for a
 * piece-wise job); then per piece k, out[2 + 2k]: the heavy-bucket count the host read (0xffffffff where it reads none: the single-launch path
 * launches the pair blind) and out[3 + 2k]: 1 if the pair was launched.  At most n words are written; returns the words the record has
 * (2 + 2 * pieces; 0 before the first call or for a null `out`).  Counters, not clocks.                                                      */
int zkg_msm_host_scalars_stats(uint32_t *out, int n);
/* Fixed bases kept resident WITH their per-window tables (level w = 2^(c w) P_i; c = 16 from 2^15 points on: 16 x the bases' memory plus the
 * same again as 29-bit records) — what the prover builds for a key's H query, offered for any fixed G1 base set (libff has no counterpart; its
 * multi_exp takes the bases as they are).  Every window's digit then weighs the same: one bucket set, one reduction, no doublings on the
 * host.  zkg_msm_g1_bases_upload reads n affine points from DEVICE memory (the layout zkg_msm_g1_dev takes) and builds the tables once;
 * zkg_msm_g1_resident computes sum scalars[i] * P_i for n DEVICE scalars (n = the handle's point count) — the same point as
 * zkg_msm_g1_dev, bit for bit.  Calls on one handle take turns.  Ordering: the job runs on a stream of the handle's own, behind everything
 * queued on `stream` (NULL: the null stream) at the time of the call — the work that wrote d_scalars — and the call returns when the result
 * is in out_jac.  The calling thread's current device must be the one the handle was made on (otherwise ZKG_ERROR); zkg_msm_g1_bases_free
 * may be called from any device.  bench.py reports it as a SECOND figure (extras.msm_resident_tables); the headline stays the plain path.                                                                                                  */
typedef struct zkg_msm_bases zkg_msm_bases;
zkg_msm_bases *zkg_msm_g1_bases_upload(const void *d_bases, size_t n);
int zkg_msm_g1_resident(zkg_msm_bases *bases, const void *d_scalars, size_t n, int scalars_mont, uint64_t out_jac[12], void *stream);
void zkg_msm_g1_bases_free(zkg_msm_bases *bases);
/* The same multi-exponentiation for a caller that stays on its stream: `count` scalar vectors over the handle's bases, the points left in
 * DEVICE memory, no wait on the host.  Vector i is n Fr elements (n = the handle's point count) at d_scalars + i * stride * 32 bytes,
 * stride >= n, aligned to 16 bytes; what lies between n and the stride is never read.  Point i lands at d_out_jac + i * 12 limbs, normalised
 * exactly as zkg_msm_g1_resident returns it (X | Y | one, or (0, one, 0) for infinity): the same bytes, bit for bit.  The vectors are cut
 * into groups of at most zkg_msm_g1_resident_batch_max; a group of several shares ONE sort, accumulation, fold and reduction (what
 * zkg_groth16_prove_batch does with the H queries of its proofs), and a one-workgroup kernel per point (k_msm_combine) finishes the
 * reduction's chunk sums and normalises on the device — the epilogue zkg_msm_g1_resident runs on the host.
 * Ordering: the work runs on the handle's own stream, behind everything queued on `stream` (NULL: the null stream) at the time of the call —
 * the work that writes d_scalars.  Before it returns the call records an event behind its last kernel and makes `stream` wait for it, so
 * whatever the caller queues on `stream` afterwards sees the points; the host has to synchronise `stream` (or an event on it) before IT
 * reads them.  The call itself does not wait: the caller keeps d_scalars and d_out_jac alive and unchanged until that later work has run.
 * Calls on one handle run in call order; zkg_msm_g1_resident on the same handle stays correct beside them (it drains them first), and
 * zkg_msm_g1_bases_free waits for the handle's stream.  The handle's workspace only grows.  A launch that needs more of any of its buffers
 * than the handle holds — the first at a group size, and sometimes a SMALLER group after a larger one: the reduction's chunk records shrink
 * as the group grows — waits for the handle's stream before that buffer is freed (earlier calls may still read it) and allocates, and may
 * block; a call whose group sizes the handle has served before does neither.  zkg_msm_g1_resident takes the same care beside pending calls.
 * Refused with ZKG_ERROR before any launch, nothing written: a null argument; n other than the handle's point count; stride < n; more
 * than 2^24 vectors or a stride above 2^32 elements; a calling thread whose current device is not the handle's; d_scalars or d_out_jac that hipPointerGetAttributes does not report as device memory of
 * the handle's device (pinned, managed and unregistered host memory are all refused), that is misaligned (16 / 8 bytes), or whose range runs
 * past the end of its allocation where hipMemGetAddressRange knows it.  count == 0 is ZKG_OK and touches nothing.                          */
int zkg_msm_g1_resident_async(zkg_msm_bases *bases, const void *d_scalars, size_t n, size_t stride /* Fr elements between vectors, >= n */, size_t count,
                              int scalars_mont, void *d_out_jac /* count x 12 limbs, DEVICE */, void *stream);
size_t zkg_msm_g1_resident_batch_max(const zkg_msm_bases *bases);   /* vectors one launch takes: what the sort's index space and bucket scan allow, at most 16 (the batched prover's largest launch; the workspace grows with it); >= 1, 0 for NULL */
/* test hook: the calling thread's last zkg_msm_g1_resident_async or zkg_msm_g2_resident_async — out[0] vectors enqueued, out[1] launch groups, out[2] host waits the
 * entry made (one per buffer it had to grow: a stream drain and an allocation; 0 where nothing grew).  Counters, not clocks.                                  */
void zkg_msm_resident_async_stats(size_t out[3]);
/* test hook: the epilogue kernel alone, on chunk records the caller makes up.  records_jac (HOST): vectors x cpw x slots normalised points
 * (12 limbs, infinity allowed) in the reduction's order — vector, chunk, slot; slots == 2: (P, U) per chunk, slots == 3: (P, T, A) with
 * U = T + 8 A.  out_jac (HOST): per vector V = sum U_ch + 2^chunk_log * sum ch * P_ch + sum P_ch, normalised.  This reaches geometries a
 * handle does not produce at test sizes (three slots, more chunks than the kernel has lanes).  Synchronous.                               */
int zkg_msm_combine_gpu(const uint64_t *records_jac, size_t cpw, int slots /* 2|3 */, int chunk_log, size_t vectors, uint64_t *out_jac);
/* The same for a fixed G2 base set (a Groth16 B query): per-window tables of n affine G2 points read from DEVICE memory (the layout
 * zkg_msm_g2_dev takes: 16 limbs per point, all-zero = infinity), window size table_window_bits(n) — 8, 12 or 16 bits; at 16 bits 16 levels
 * of 128 bytes per point.  1 <= n < 2^25; NULL with zkg_last_error set for a bad argument or a failed allocation.  No subgroup or on-curve
 * check is made, as for G1.  The contract of every entry is its G1 sibling's above:
 * zkg_msm_g2_resident: sum scalars[i] * P_i for n DEVICE scalars (n = the handle's point count), the same normalised 24 limbs as
 * zkg_msm_g2_dev over the same bases, bit for bit.  Calls on one handle take turns, run on the handle's own stream behind everything queued
 * on `stream` at the time of the call, and the call returns when the point is in out_jac.
 * zkg_msm_g2_resident_async: `count` vectors, vector i at d_scalars + i * stride * 32 bytes (stride >= n, 16-byte aligned; what lies between
 * n and the stride is never read), point i at d_out_jac + i * 24 limbs, normalised exactly as zkg_msm_g2_resident returns it: X | Y | one,
 * or (0, one, 0) for infinity, with one = (Montgomery one, 0).  The vectors are cut into groups of at most zkg_msm_g2_resident_batch_max; a
 * group shares one sort, accumulation, fold and reduction, and a one-workgroup kernel per point (k_msm_combine) sums the reduction's chunk
 * records and normalises on the device.  The call records an event behind its last kernel and makes `stream` wait for it; it makes no
 * host wait at a group size the handle has served before.  A buffer that must grow is freed only after the handle's stream has drained, and
 * each such drain is counted (zkg_msm_resident_async_stats); zkg_msm_g2_resident beside pending asynchronous calls takes the same care;
 * zkg_msm_g2_bases_free waits for the handle's stream and may be called from any device.
 * Refused with ZKG_ERROR before any launch, nothing written: a null argument; n other than the handle's point count; stride < n; more than
 * 2^24 vectors or a stride above 2^32 elements; a calling thread on another device; d_scalars or d_out_jac that is not device memory of the
 * handle's device, is misaligned (16 / 8 bytes) or runs past its allocation.  count == 0 is ZKG_OK and touches nothing.                    */
typedef struct zkg_msm_g2_bases zkg_msm_g2_bases;
zkg_msm_g2_bases *zkg_msm_g2_bases_upload(const void *d_bases /* DEVICE, n x 16 limbs affine Montgomery, all-zero = infinity */, size_t n);
void   zkg_msm_g2_bases_free(zkg_msm_g2_bases *bases);
int    zkg_msm_g2_resident(zkg_msm_g2_bases *bases, const void *d_scalars, size_t n, int scalars_mont, uint64_t out_jac[24], void *stream);
int    zkg_msm_g2_resident_async(zkg_msm_g2_bases *bases, const void *d_scalars, size_t n, size_t stride, size_t count,
                                 int scalars_mont, void *d_out_jac /* count x 24 limbs, DEVICE */, void *stream);
/* vectors one launch takes: the largest p <= 16 (MSM_MULTI_MAX_VECTORS, the batched prover's largest launch) that the sort's index space and
 * bucket scan allow AND whose bucket workspace, p x windows x 2^(c-1) buckets of 256 bytes (an XYZZ<Fq2>, four times G1's), stays at or under
 * 1 GiB: 8 at 16-bit windows (128 MiB per vector), 16 below.  >= 1, 0 for NULL.                                                            */
size_t zkg_msm_g2_resident_batch_max(const zkg_msm_g2_bases *bases);
/* test hook: the G2 epilogue kernel alone.  records_jac (HOST): vectors x cpw x 2 normalised G2 points (24 limbs, infinity allowed) in order
 * vector, chunk, (P, U); out_jac (HOST): per vector V = sum U_ch + 2^chunk_log * sum ch * P_ch + sum P_ch, normalised.  Bounds as
 * zkg_msm_combine_gpu: 1 <= cpw <= 2^16, 0 <= chunk_log <= 24, 1 <= vectors <= 1024.  Synchronous.                                         */
int    zkg_msm_combine_g2_gpu(const uint64_t *records_jac, size_t cpw, int chunk_log, size_t vectors, uint64_t *out_jac);
/* Window-sharded variant for multi-GPU runs where every GPU holds every base: the partial
 * sum over the Pippenger windows first_window, first_window + window_stride, ... only, each
 * already weighted by 2^(c w) — the partials of ranks g = 0..G-1 (first_window = g,
 * window_stride = G) add up to zkg_msm_g1_dev's result (zkg_g1_sum).                      */
int zkg_msm_g1_windows_dev(const void *d_bases, const void *d_scalars, size_t n, int scalars_mont,
                           unsigned first_window, unsigned window_stride, uint64_t out_jac[12], void *stream);
/* Sum of `count` normalised-jac G1 (G2) points held in HOST memory: the combine step after
 * the per-GPU partial MSMs have been all-gathered (RCCL has no elliptic-curve reduce op). */
int zkg_g1_sum(const uint64_t *points_jac, size_t count, uint64_t out_jac[12]);
int zkg_g2_sum(const uint64_t *points_jac, size_t count, uint64_t out_jac[24]);

/* ---- several GPUs in ONE process: the G1 multi-exponentiation sharded by points.
 *      zkg_init_multi: zkg_init(devices[0]) plus the per-device kernel setup of the other devices.  A device may be listed more
 *      than once (two shards on one GPU: how a single-GPU box rehearses the path).
 *      zkg_msm_g1_shards_upload: splits n affine bases (HOST pointer) into ndev contiguous shards, shard i resident on devices[i]
 *      with its own stream and workspace.
 *      zkg_msm_g1_multi: scalars n x 4 canonical limbs (HOST pointer).  One host thread per shard uploads that shard's scalar
 *      slice and runs the complete single-GPU Pippenger; the ndev partial points are added on the host (RCCL has no elliptic-curve
 *      reduction; the exchange is 96 bytes per GPU).  partials_jac (optional, ndev x 12 limbs) receives the per-shard results.
 *      Result == zkg_msm_g1 on the same inputs, bit for bit.  Calls on one handle take turns (a mutex inside the handle: a call owns
 *      every shard's scalar buffer, workspace and stream); different handles run side by side.                                */
typedef struct zkg_msm_shards zkg_msm_shards;
int zkg_init_multi(const int *devices, int ndev);
zkg_msm_shards *zkg_msm_g1_shards_upload(const uint64_t *bases, size_t n, const int *devices, int ndev);
void zkg_msm_g1_shards_free(zkg_msm_shards *shards);
size_t zkg_msm_g1_shards_count(const zkg_msm_shards *shards, size_t *points);
int zkg_msm_g1_multi(const zkg_msm_shards *shards, const uint64_t *scalars, uint64_t out_jac[12], uint64_t *partials_jac);
/* With ZKG_MULTI_RCCL=1 in the environment zkg_msm_g1_multi exchanges the shards' partial points with an RCCL all-gather (one
 * communicator per shard from ncclCommInitAll, one group call per multi-exponentiation, 96 bytes per GPU over xGMI) before the sum; the
 * library is opened at run time.  Needs every shard on its own device (RCCL refuses a device listed twice: such a handle keeps the host
 * exchange).  zkg_multi_rccl_calls: how many calls of this process went through the collective.                                      */
unsigned zkg_multi_rccl_calls(void);

/* ---- fixed-base batch: out[i] = scalars[i] * base (affine out).  The batch_exp of
 *      libsnark's generator (snark.cpp:91); used here to build synthetic bases on device. */
int zkg_g1_fixed_base_dev(const uint64_t base[8], const void *d_scalars, size_t n, void *d_out_affine, void *stream);
int zkg_g2_fixed_base_dev(const uint64_t base[16], const void *d_scalars, size_t n, void *d_out_affine, void *stream);

/* ---- CRS residency: parse once, keep on device (removes the per-call pk re-parse of
 *      libsnark_wrapper.cpp:230 and the by-value pk copy of snark.cpp:107-109).        */
zkg_crs *zkg_crs_upload(const zkg_pk *pk);
/* Same, from the byte blob zklaim keeps in ctx->pk (written by libsnark_export_pk, libsnark_wrapper.cpp:146-157, i.e.
 * operator<<(r1cs_gg_ppzksnark_proving_key) under libsnark's default flags: binary, Montgomery, compressed points).
 * Replaces libsnark_import_pk (libsnark_wrapper.cpp:160-168); the ~4n+m point decompressions (one square root each) run
 * on the GPU.  The domain is recovered from |H_query| + 1 (2^k, or a step_radix2 size 2^a + 2^b).  Counts inside the blob are
 * bounded by the bytes that follow them before anything is sized by them: a malformed blob is an error return, never a fault. */
zkg_crs *zkg_crs_upload_blob(const void *pk_blob, size_t len);
/* The host half of that loader alone (no GPU, no zkg_init): walks the sections, the sparse B index list and every constraint's terms of
 * a pk blob and reports its sizes — out[8] (optional): A_query entries, B_query values, H_query entries, L_query entries, public inputs,
 * constraints, terms in A + B + C, evaluation domain size.  ZKG_OK / ZKG_ERROR; what the reference's libsnark_import_pk would have
 * thrown on (libsnark_wrapper.cpp:160-168) is an error return here. */
int zkg_pk_blob_inspect(const void *pk_blob, size_t len, uint64_t out[8]);
void     zkg_crs_free(zkg_crs *crs);
/* One proof over several GPUs of ONE process: shards the H query of a resident key — the largest of the prover's
 * four multi-exponentiations, m - 1 uniformly random scalars — by points over `ndev` devices (call zkg_init_multi first; a device may be
 * listed more than once, which is how a one-GPU box rehearses the path).  Shard i keeps the per-window table of its slice on devices[i];
 * every later proof copies that slice of coefficients_for_H there (32 bytes per point, peer-to-peer), runs the shards side by side and adds
 * the partial points on the host.  Everything else of the proof stays on the key's own device.  Proof bytes are unchanged.
 * No proof of this key may be in flight during the call.                                                                         */
int zkg_crs_shard_h(zkg_crs *crs, const int *devices, int ndev);
uint32_t zkg_crs_num_variables(const zkg_crs *crs);   /* n of the resident key (the witness length zkg_groth16_prove expects) */

/* ---- Groth16 prove: r1cs_gg_ppzksnark_prover (snark.cpp:126) with the prover
 *      randomness (r, s) as explicit inputs (libsnark draws them internally).
 *      witness: n x 4 limbs Montgomery Fr = primary_input || auxiliary_input.
 *      r, s: Montgomery Fr.  proof_out: >= ZKG_PROOF_BYTES; layout = libsnark
 *      operator<<(proof) under its default flags (binary, Montgomery, compressed):
 *      g_A (34 B) || g_B (66 B) || g_C (34 B) (exported at libsnark_wrapper.cpp:170-181).
 *      check_satisfied != 0 reproduces the gate of snark.cpp:121-124 and returns
 *      ZKG_UNSATISFIED without proving.                                                */
int zkg_groth16_prove(const zkg_crs *crs, const uint64_t *witness, const uint64_t r[4],
                      const uint64_t s[4], int check_satisfied, uint8_t *proof_out, size_t *proof_len);
/* The same proof from a sparse description of the witness: tags[n] (0 = zero, 1 = one, 2 = listed) and `count` listed variables
 * as (index in 0..n-1, value as 4 Montgomery limbs).  For witness generators that know their bits (zkg_circuit_sparse_witness): the
 * host-to-device upload shrinks ~30x.  Proof bytes are identical to zkg_groth16_prove on the expanded vector.
 * Every listed index must be in range, tagged 2 and listed once (a listed VALUE may be anything, 0 and 1 included); a tag-2 variable that
 * is not listed counts as zero.  An index out of range, not tagged 2 or listed twice is ZKG_ERROR (detected on the device: each listed
 * variable's tag byte is claimed once; no proof is written). */
int zkg_groth16_prove_sparse(const zkg_crs *crs, const uint8_t *tags, const uint32_t *full_index, const uint64_t *full_values, size_t count,
                             const uint64_t r[4], const uint64_t s[4], int check_satisfied, uint8_t *proof_out, size_t *proof_len);
/* ---- many proofs of ONE resident key in one call.  An item is one zkg_groth16_prove (witness != NULL) or one zkg_groth16_prove_sparse
 *      (witness == NULL) call with its own (r, s); status[i] and the ZKG_PROOF_BYTES at proofs_out + i * ZKG_PROOF_BYTES are exactly what that
 *      call returns and writes for item i alone — proof bytes are deterministic given (key, witness, r, s).  An unsatisfied witness (with
 *      check_satisfied) is ZKG_UNSATISFIED for that item only, a bad sparse listing or a null pointer inside an item ZKG_ERROR for that item
 *      only; the other items are still proved and nothing is written for a failed one.  Keys on a domain below 2^18 (radix-2 up to 2^17
 *      and every step_radix2 size under 2^18: one to seven zklaim payloads) without H shards are proved in chunks of zkg_prove_batch_chunk
 *      items whose GPU work is ONE launch sequence (the kernels carry a proof dimension; the H multi-exponentiations of a chunk share one
 *      sort, accumulation, fold and reduction); other keys go through the single-proof path item by item.  Synchronous; host pointers; safe from several threads and beside zkg_groth16_prove* on the same key.
 *      Returns ZKG_OK when every status was written (count == 0 included: nothing is touched), ZKG_ERROR for a null argument or a HIP failure. */
typedef struct zkg_prove_item {
    const uint64_t *witness;                 /* dense form: n x 4 limbs as zkg_groth16_prove, or NULL for the sparse form */
    const uint8_t  *tags; const uint32_t *full_index; const uint64_t *full_values; size_t count;   /* as zkg_groth16_prove_sparse */
    const uint64_t *r, *s;                   /* 4 limbs each, Montgomery Fr */
} zkg_prove_item;
int zkg_groth16_prove_batch(const zkg_crs *crs, const zkg_prove_item *items, size_t count, int check_satisfied,
                            uint8_t *proofs_out /* count x ZKG_PROOF_BYTES */, int *status /* count entries */);
/* test hook: what the calling thread's last zkg_groth16_prove_batch did — out[0] items that went through batched launches, out[1] items
 * that went through the single-proof path, out[2] batched chunks launched.  Counters, not clocks. */
void zkg_prove_batch_stats(size_t out[3]);
size_t zkg_prove_batch_chunk(const zkg_crs *crs);   /* proofs per batched chunk for this key; 0 = this key takes the single-proof path */
/* ---- proofs from witnesses that are ALREADY in device memory (a torch computation's output, the caller's own witness kernel): the *_dev form of
 *      zkg_groth16_prove and zkg_groth16_prove_batch.  d_witness: n x 4 limbs Montgomery Fr in DEVICE memory, the layout zkg_groth16_prove takes
 *      on the host, aligned to 16 bytes; item i of d_witnesses starts `stride` Fr elements (32 bytes each) after item i - 1, stride >= n, and what
 *      lies between n and the stride is never read.  rs, proofs_out and status are HOST pointers: (r, s) per item as 8 limbs r | s.  Status
 *      and proof bytes are exactly those of zkg_groth16_prove on a host copy of the same vector with the same (r, s), ZKG_UNSATISFIED
 *      included; for the batch the per-item rules of zkg_groth16_prove_batch hold (a failed item fails alone, nothing is written for it;
 *      count == 0 is ZKG_OK and touches nothing).  One kernel (k_split_dev, the proof as its second grid dimension) reads the caller's
 *      buffer in place and writes [1 | w], the tags, the non-bit listing and its counts where the mat-vec and the witness jobs read them: no
 *      staging buffer, no scan on the host, no host-to-device copy of witness data.
 *      Ordering (zkg_msm_g1_resident's contract): the work runs on the library's own streams, behind everything queued on `stream` (NULL: the
 *      null stream) at the time of the call — the work that wrote the witness — and the call returns when the proofs are in host memory,
 *      so the caller may overwrite the buffer as soon as it returns.
 *      Refused with ZKG_ERROR before any launch, nothing written: a null argument; stride < n; a calling thread whose current device is not
 *      the key's; a pointer that hipPointerGetAttributes does not report as device memory of the key's device (pinned, managed and
 *      unregistered host memory are all refused); a range that runs past the end of its allocation where hipMemGetAddressRange knows it
 *      (best effort: a sub-range of a caching allocator's block is checked against that block).
 *      zkg_groth16_prove_dev serves every key the single-proof path serves (radix-2 and step domains, m >= 2^18, H shards);
 *      zkg_groth16_prove_batch_dev cuts the items into zkg_prove_batch_chunk chunks and sets zkg_prove_batch_stats exactly as
 *      zkg_groth16_prove_batch does, and goes item by item through the single _dev path for a key whose chunk is 0.  Safe from several
 *      threads and beside every other prove entry on the same key. */
int zkg_groth16_prove_dev(const zkg_crs *crs, const void *d_witness, const uint64_t r[4], const uint64_t s[4], int check_satisfied,
                          uint8_t *proof_out, size_t *proof_len, void *stream);
int zkg_groth16_prove_batch_dev(const zkg_crs *crs, const void *d_witnesses, size_t stride /* Fr elements between items, >= n */, size_t count,
                                const uint64_t *rs /* count x 8 limbs: r | s, host */, int check_satisfied,
                                uint8_t *proofs_out /* count x ZKG_PROOF_BYTES, host */, int *status /* count entries, host */, void *stream);
/* the calling thread's last zkg_groth16_prove_dev / zkg_groth16_prove_batch_dev: out[0] witnesses split on the device from the caller's buffer,
 * out[1] witnesses staged through host memory (0 on every path).  Counters, not clocks. */
void zkg_prove_dev_stats(size_t out[2]);
/* ---- proofs that stay on the caller's stream and on the device: a prover handle on a resident key.  One call takes `count` witnesses in DEVICE
 *      memory and leaves `count` proofs of ZKG_PROOF_BYTES in DEVICE memory, queued behind the caller's stream with no wait on the host and no
 *      arithmetic on the host; the bytes are those of zkg_groth16_prove_dev for the same (key, witness, r, s).  The synchronous entries above
 *      keep their own tuned paths (subset tables, flat sums over the ones, host finish) and remain the default.
 *      zkg_prover_new(crs): from a resident key of any source (zkg_crs_upload, zkg_crs_upload_blob, zkg_groth16_setup_resident), on the calling
 *      thread's device, which must be the key's and the zkg_init device.  The handle BORROWS the key — its H per-window table, its queries, its
 *      domain tables: free the prover before the key.  A key whose H query is sharded (zkg_crs_shard_h) is refused, and zkg_crs_shard_h refuses
 *      a key that has a live prover handle.  NULL on failure, with zkg_last_error set (no zkg_init, a null key, a failed allocation).
 *      What the handle builds once: a QAP handle over a device copy of the key's constraint system; per-window tables over the WHOLE witness
 *      queries — A[1..n], B_g1[1..n], L padded to n points (infinity for the l public inputs, so that the three G1 sets share indices) and
 *      B_g2[1..n], window size by n (8, 12 or 16 bits); three multi-exponentiation jobs with a device epilogue (one launch for the three G1 sets,
 *      one for G2, one for H); the constant column's points A[0], B_g1[0], B_g2[0] and alpha, beta; the fixed-base tables of alpha_1, beta_1,
 *      delta_1, delta_2 (64 x 15 affine multiples each) in device memory.  Memory beside the key: 64 B x levels x n per G1 table (these launches
 *      read no 29-bit records, so none are built) and 128 B x levels x n for G2 — 320 B x 16 x n at 16-bit windows, 1.1 GB for an
 *      eight-payload credential key (n = 219 338) — plus per proof of a group 32 (m + 1) B of coefficients, the QAP handle's 216 m B and the
 *      jobs' buckets: at 16-bit windows 128 MiB for the G2 job (the capped one: 1 GiB for a group of 8), 3 x 64 MiB for the three G1 sets
 *      of the A / B_1 / L job (1.5 GiB for a group of 8) and 32 MiB for H, whose rows are merged in pairs (0.25 GiB); at 12-bit windows a sixteenth of that per proof.
 *      zkg_prover_free waits for the handle's pending work; NULL is accepted; callable from any device.
 *      zkg_prover_prove_async: witness i is n Montgomery Fr at d_witnesses + i * stride * 32 bytes, stride >= n (zkg_groth16_prove_batch_dev's
 *      layout), read in place; what lies between n and the stride is never read.  d_rs: (r, s) of item i as 8 limbs r | s, Montgomery Fr, in
 *      DEVICE memory.  Proof i goes to d_proofs + i * proof_stride; bytes between ZKG_PROOF_BYTES and proof_stride are never written and no
 *      alignment is asked of d_proofs.  Every word of d_status is written: ZKG_OK, or ZKG_UNSATISFIED when check_satisfied != 0 and the witness
 *      violates a row — nothing is then written at that item's proof position and the other items are not affected; with check_satisfied == 0
 *      the proof is written as zkg_groth16_prove_dev writes it.
 *      The items are cut into groups of at most zkg_prover_batch_max — the largest p <= 16 that the three multi launches' sort geometry allows,
 *      capped by the QAP handle's group and by 1 GiB of G2 buckets (zkg_msm_g2_resident_batch_max's rule).  Per group: the QAP handle's launch
 *      sequence (coefficients_for_H and the unsatisfied words) and H over it on the handle's main stream; beside it, from the call's fork event,
 *      the A / B_1 / L launch, the B_2 launch and the key-only part of the epilogue on three more streams; then the epilogue (three stages:
 *      the products with r, s, rs from the fixed-base tables; s (W_a + A_0) and r (W_b1 + B1_0) as 4-bit windowed ladders side by side, behind
 *      the G1 job; the sums, one normalisation per point and the three records).
 *      Ordering: everything is ordered behind what is on `stream` (NULL: the null stream) at the time of the call, and before returning the call
 *      makes `stream` wait for its last kernel: later work on `stream` sees proofs and status, and the host synchronises `stream` before it reads
 *      them.  The caller keeps all four buffers alive and unchanged until then.  A handle serves its calls in call order whatever streams they
 *      name (the enqueue is under the handle's mutex, on the handle's own streams).  The workspace only grows: a call that needs more of it
 *      drains the handle's work first and counts one host wait per buffer set that grew; a call at a group size the handle has served makes no
 *      host wait and no allocation.
 *      Refused with ZKG_ERROR before any launch, nothing written: a null argument; stride < n or proof_stride < ZKG_PROOF_BYTES; more than 2^24
 *      items, or a stride (either) above 2^32; a calling thread on another device than the key's; any of the four pointers that is not device
 *      memory of that device, is misaligned (16 bytes for d_witnesses and d_rs, 4 for d_status) or runs past its allocation; ranges that
 *      overlap.  count == 0 is ZKG_OK and touches nothing.  Safe from several threads, and beside every synchronous prove entry on the same key
 *      (it shares only read-only key data).                                                                                                  */
typedef struct zkg_prover zkg_prover;
zkg_prover *zkg_prover_new(const zkg_crs *crs);
void   zkg_prover_free(zkg_prover *p);
size_t zkg_prover_batch_max(const zkg_prover *p);         /* proofs one launch sequence takes; >= 1, 0 for NULL */
void   zkg_prover_set_batch_max(zkg_prover *p, size_t k); /* test hook: k proofs per launch sequence from now on; 0 restores the default, a larger k is clamped to it */
int    zkg_prover_prove_async(zkg_prover *p, const void *d_witnesses, size_t stride /* Fr elements between items, >= n */, size_t count,
                              const void *d_rs /* DEVICE, count x 8 limbs: r | s */, int check_satisfied,
                              void *d_proofs /* DEVICE */, size_t proof_stride /* bytes, >= ZKG_PROOF_BYTES */,
                              uint32_t *d_status /* DEVICE, count words */, void *stream);
/* test hook: the calling thread's last zkg_prover_prove_async — out[0] proofs enqueued, out[1] launch groups, out[2] host waits.  Counters, not clocks. */
void   zkg_prover_stats(size_t out[3]);
/* test hook: the proof epilogue alone, on points the caller makes up.  key_points: alpha_g1 | beta_g1 | delta_g1 | A_0 | B1_0 (8 limbs each) |
 * beta_g2 | delta_g2 | B2_0 (16 each), affine Montgomery, all-zero = infinity.  points: per proof W_a | W_b1 | L | H (12 limbs each, normalised
 * jac) | W_b2 (24 limbs) — the sums over the witness WITHOUT the constant column, which the epilogue adds; rs: per proof r | s.  HOST pointers;
 * proofs_out: count x ZKG_PROOF_BYTES.  where 0: the host's assembly (no GPU, no zkg_init) — the specification; 1: the epilogue kernels (needs
 * zkg_init).  count <= 2^16.  Synchronous.                                                                                                 */
int    zkg_proof_assemble(const uint64_t *key_points, const uint64_t *points, const uint64_t *rs, size_t count, int where, uint8_t *proofs_out);
/* ---- many zklaim credentials of ONE resident key, their witnesses generated on the GPU.  ctxs[i] is a zklaim_ctx (include/zklaim_abi.h) whose
 *      payload count is the key's; rs holds (r, s) per item, 8 limbs: r | s, Montgomery Fr.  status[i] and the proof bytes are exactly those of
 *      zkg_groth16_prove_sparse on the host witness of ctxs[i] (zkg_zklaim_witness_new + zkg_circuit_sparse_witness) with the same (r, s).
 *      Per chunk, 128 bytes per payload go up (pre-image, hash, reference values, ops) and one kernel writes every variable's tag and the
 *      listed values into the chunk's device stage; everything from the split on is zkg_groth16_prove_batch's.  A null context, a broken
 *      payload list or a payload count other than the key's is ZKG_ERROR for that item only, an unsatisfied credential ZKG_UNSATISFIED for
 *      that item only.  For a key that does not batch (zkg_prove_batch_chunk == 0) the witnesses are made on the host and the existing
 *      paths are taken: same bytes.  The generator counts a payload's variables itself; if that count ever disagrees with the host pass's,
 *      or with the key's variable count, the call keeps the host witnesses and zkg_last_error says so.  Returns as zkg_groth16_prove_batch. */
struct zklaim_ctx;
int zkg_groth16_prove_batch_zklaim(const zkg_crs *crs, const struct zklaim_ctx *const *ctxs, size_t count, const uint64_t *rs /* count x 8 limbs */,
                                   int check_satisfied, uint8_t *proofs_out /* count x ZKG_PROOF_BYTES */, int *status /* count entries */);
/* what the calling thread's last zkg_groth16_prove_batch_zklaim or zkg_zklaim_prove_batch did: out[0] items whose witness the GPU made,
 * out[1] items whose witness the host made.  Counters, not clocks. */
void zkg_zklaim_witness_stats(size_t out[2]);
/* Variables of the credential circuit with `payloads` payloads (0: out of range), and optionally the most one witness can list, as the
 * generator counts them.  No GPU, no zkg_init. */
size_t zkg_zklaim_witness_size(size_t payloads, size_t *cap_listed);
/* test hook: the generator alone.  Contexts of ONE payload count (that of the first non-null one), n = zkg_zklaim_witness_size of it:
 * tags_out[i * n ..] the tag of every variable (0 zero, 1 one, 2 listed), index_out[i * cap_listed ..] / values_out[4 * i * cap_listed ..]
 * the listed variables in ascending order with their Montgomery values, listed_counts[i] how many.  A null context, a broken payload list or
 * another payload count fails alone: listed_counts[i] = (size_t)-1, its tags zero.  Needs zkg_init, no key. */
int zkg_zklaim_witness_gpu(const struct zklaim_ctx *const *ctxs, size_t count, uint8_t *tags_out /* count x n */, uint32_t *index_out,
                           uint64_t *values_out, size_t cap_listed /* per item */, size_t *listed_counts);
/* the same outputs for one context from the generator's code compiled for the host.  No GPU, no zkg_init (as zkg_pk_blob_inspect). */
int zkg_zklaim_witness_mirror(const struct zklaim_ctx *ctx, uint8_t *tags_out /* n */, uint32_t *index_out, uint64_t *values_out, size_t cap_listed,
                              size_t *listed_count);
/* ---- ONE zklaim credential of a resident key, its witness generated on the GPU: status and proof bytes are exactly those of
 *      zkg_groth16_prove_sparse on the host witness of ctx (zkg_zklaim_witness_new + zkg_circuit_sparse_witness) with the same (r, s).
 *      Every key the single-proof path serves: radix-2 and step domains, m >= 2^18, H shards.  128 bytes per payload go up in one copy and
 *      k_zklaim_witness_par — a plain SHA-256 per payload, then one thread per slice of the circuit's trace — writes tags and listed values in
 *      front of the split, on the proof's own stream; nothing waits on the host for it.  A null context, a broken payload list or a payload
 *      count other than the key's: ZKG_ERROR; an unsatisfied credential: ZKG_UNSATISFIED; nothing is written in either case.  If the
 *      generator's plan does not fit the key, disagrees with the host pass about a payload's variables, or the kernel raises its error word,
 *      the witness is made on the host and zkg_groth16_prove_sparse's path is taken: same bytes, zkg_last_error says why. */
int zkg_groth16_prove_zklaim(const zkg_crs *crs, const struct zklaim_ctx *ctx, const uint64_t r[4], const uint64_t s[4],
                             int check_satisfied, uint8_t *proof_out, size_t *proof_len);
/* the calling thread's last zkg_groth16_prove_zklaim / libsnark_prove: out[0] = 1 if the GPU made the witness, out[1] = 1 if the host did */
void zkg_prove_zklaim_stats(size_t out[2]);
/* test hooks: zkg_zklaim_witness_gpu's contract on k_zklaim_witness_par; and zkg_zklaim_witness_mirror's on that kernel's device code
 * compiled for the host — the value pass, then every slice on its own, last one first (no GPU, no zkg_init) */
int zkg_zklaim_witness_gpu_parallel(const struct zklaim_ctx *const *ctxs, size_t count, uint8_t *tags_out /* count x n */, uint32_t *index_out,
                                    uint64_t *values_out, size_t cap_listed /* per item */, size_t *listed_counts);
int zkg_zklaim_witness_mirror_parallel(const struct zklaim_ctx *ctx, uint8_t *tags_out /* n */, uint32_t *index_out, uint64_t *values_out,
                                       size_t cap_listed, size_t *listed_count);
/* coefficients_for_H (m+1 Fr, Montgomery) of r1cs_to_qap_witness_map, for parity tests */
int zkg_qap_witness_h(const zkg_crs *crs, const uint64_t *witness, uint64_t *h_out);
/* per-stage device milliseconds of the last zkg_groth16_prove on this crs (the stages run on their own streams, so the entries
 * overlap and do not add up to the total): [0] R1CS mat-vec, [1] 7 NTTs + pointwise, [2] A / B(G1) / L over the non-bit witness
 * elements (one batched job), [3] unused, [4] B(G2) over the same elements, [5] H, [6] unused, [7] wall-clock total incl. host
 * assembly.  The flat sums over the witness elements equal to one run beside [2] and [4] on a stream of their own.               */
int zkg_prove_stage_ms(const zkg_crs *crs, float ms[8]);
/* the largest number of proofs one resident key has had in flight at once (callers on several threads share a key's prover slots: up
 * to three below m = 2^18, two at 2^18, one above) since the last call with reset != 0.  A counter, not a clock: what the concurrency
 * tests assert instead of wall-clock ratios. */
int zkg_prover_peak_in_flight(int reset);

/* ---- zklaim's credential circuit on the host: replaces protoboard + zklaim_gadget construction,
 *      generate_r1cs_constraints and generate_r1cs_witness (snark.cpp:113-118, zklaim_gadget.cpp:153-784) and
 *      zklaim_input_map (zklaim_gadget.cpp:115-150).  `ctx` is zklaim's own zklaim_ctx (include/zklaim_abi.h).           */
struct zklaim_ctx;
typedef struct zkg_circuit zkg_circuit;
/* flags: ZKG_CIRCUIT_WITH_WITNESS assigns the variables from ctx (generate_r1cs_witness);
 *        ZKG_CIRCUIT_REFERENCE_QUIRK leaves the pack_PL / pack_REF / pack_OPS packings unconstrained as the reference does
 *        (zklaim_gadget.cpp:583-699 never generates them): refvals / opsvals / plvars are then free witness variables and the
 *        proof only binds SHA256(pre) == hash.  Default (flag clear): the packings are enforced (78 constraints per payload). */
#define ZKG_CIRCUIT_WITH_WITNESS 1
#define ZKG_CIRCUIT_REFERENCE_QUIRK 2
zkg_circuit *zkg_zklaim_circuit_new(const struct zklaim_ctx *ctx, int flags);
zkg_circuit *zkg_zklaim_witness_new(const struct zklaim_ctx *ctx);   /* witness only: no constraints, no CSR (prover with a resident key) */
uint32_t zkg_circuit_num_variables(const zkg_circuit *c);
void zkg_circuit_free(zkg_circuit *c);
int zkg_circuit_r1cs(const zkg_circuit *c, zkg_r1cs *out);        /* pointers stay valid until zkg_circuit_free            */
const uint64_t *zkg_circuit_witness(const zkg_circuit *c);        /* num_variables x 4 limbs (NULL without witness)        */
int zkg_circuit_sparse_witness(const zkg_circuit *c, const uint8_t **tags, const uint32_t **full_index, const uint64_t **full_values, size_t *count);
int zkg_circuit_is_satisfied(const zkg_circuit *c);               /* pb.is_satisfied() (snark.cpp:121)                     */
long zkg_circuit_first_unsatisfied(const zkg_circuit *c);         /* index of the first violated constraint, -1 if none    */
size_t zkg_zklaim_input_map(const struct zklaim_ctx *ctx, uint64_t *out, size_t cap_elems);   /* returns the element count */

/* ---- key generation and verification.
 *      zkg_groth16_setup replaces r1cs_gg_ppzksnark_generator (snark.cpp:91): trapdoor = 5 x 4 canonical limbs
 *      (t, alpha, beta, gamma, delta) or NULL for fresh randomness; the fixed-base exponentiations run on the GPU.
 *      The blobs follow libsnark's operator<< layout for pk / vk (exported at libsnark_wrapper.cpp:122-157).
 *      zkg_groth16_verify replaces r1cs_gg_ppzksnark_verifier_strong_IC (snark.cpp:62): 0 valid, 1 invalid, 2 malformed.   */
typedef struct zkg_keypair zkg_keypair;
zkg_keypair *zkg_groth16_setup(const zkg_r1cs *cs, const uint64_t *trapdoor);
/* The same keypair, byte for byte under the same trapdoor (pk arrays, swap flag, pk and vk blobs), with no scalar vector on the host: after the
 * swap decision a zkg_qap handle over the stored system runs zkg_qap_instance_async at t, t^i Z(t) / delta comes from the powers kernel, the
 * (beta At + alpha Bt + Ct) / gamma and / delta combinations from one kernel, and the fixed-base batches read those device buffers.  NULL with
 * zkg_last_error set: no zkg_init, a system zkg_qap_new refuses, a trapdoor whose t lies on the evaluation domain.                            */
zkg_keypair *zkg_groth16_setup_dev(const zkg_r1cs *cs, const uint64_t *trapdoor /* as zkg_groth16_setup; NULL = random */);
/* r1cs_gg_ppzksnark_generator with the key left where it is made.  trapdoor as zkg_groth16_setup (NULL: fresh randomness).
 * *pk_blob / *vk_blob: the bytes zkg_keypair_pk_blob / zkg_keypair_vk_blob write for zkg_groth16_setup under the same trapdoor, byte for byte,
 * malloc'ed (zkg_free).  *crs (optional, NULL: an issuer that keeps nothing on the GPU): the resident key, ready for every zkg_groth16_prove*
 * entry, the same key zkg_crs_upload_blob(*pk_blob) would load — proofs are byte-identical.  No scalar vector and no query point exists on
 * the host: the scalars are computed as zkg_groth16_setup_dev computes them, the B query's non-zero list by a ballot / scan / scatter of
 * three launches over the device Bt, and the points come back only as the blob's compressed records.  ZKG_ERROR with zkg_last_error set and
 * nothing allocated (the out-pointers are left alone): no zkg_init; a null cs, pk_blob, pk_len, vk_blob or vk_len; a system zkg_qap_new
 * refuses; a trapdoor whose t lies on the evaluation domain.  Safe to call from several threads at once. */
int  zkg_groth16_setup_resident(const zkg_r1cs *cs, const uint64_t *trapdoor, uint8_t **pk_blob, size_t *pk_len,
                                uint8_t **vk_blob, size_t *vk_len, zkg_crs **crs);
void zkg_free(void *p);
/* the calling thread's last zkg_groth16_setup_resident or libsnark_trusted_setup: out[0] 1 if the scalars were computed on the device,
 * out[1] entries of the B query's non-zero list, out[2] Fr scalars uploaded from host memory for the query batches (0 on the device path).
 * Counters, not clocks. */
void zkg_setup_resident_stats(size_t out[3]);
/* test hook: positions of the non-zero elements of n raw Fr (HOST pointer, 4 limbs each, any representative below 2r, nothing normalised),
 * ascending.  where 0: a plain host loop (no GPU, no zkg_init); 1: the generator's kernels.  idx_out holds up to n entries; only *count of
 * them are written.  n <= 2^28. */
int zkg_fr_nonzero_index(const uint64_t *fr, size_t n, int where, uint32_t *idx_out, size_t *count);
void zkg_keypair_free(zkg_keypair *kp);
const zkg_pk *zkg_keypair_pk(const zkg_keypair *kp);               /* flat arrays, valid until zkg_keypair_free              */
int zkg_keypair_swapped(const zkg_keypair *kp);                    /* 1 if swap_AB_if_beneficial exchanged A and B          */
size_t zkg_keypair_pk_blob(const zkg_keypair *kp, uint8_t *out, size_t cap);   /* returns the size needed / written       */
size_t zkg_keypair_vk_blob(const zkg_keypair *kp, uint8_t *out, size_t cap);
int zkg_groth16_verify(const uint8_t *vk_blob, size_t vk_len, const uint64_t *primary_input, size_t n_inputs,
                       const uint8_t *proof, size_t proof_len);
int zkg_pairing_probe(const uint64_t a[4], const uint64_t b[4], uint8_t out[384]);   /* e(a*G1, b*G2), for bilinearity tests */
/* ---- batch verification on the GPU.  One item = one zkg_groth16_verify call; items may name different keys (grouped by the
 *      vk's bytes).  verdicts[i] = what zkg_groth16_verify would return for items[i] (0 valid, 1 invalid, 2 malformed vk), except
 *      with probability at most (number of combined checks) * 2^-128: the proofs of one key are checked together as one random
 *      linear combination (128-bit weights drawn from std::random_device on every call), a failed combination is bisected, and
 *      whatever the combination cannot decide soundly (malformed or unusual keys, wrong sizes, bad encodings, B outside G2) goes
 *      through zkg_groth16_verify's own code.  Synchronous; host pointers; safe to call from several threads at once.
 *      Returns ZKG_OK when every verdict was written, ZKG_ERROR on a null argument, a HIP failure or no GPU (zkg_init).    */
typedef struct zkg_verify_item {
    const uint8_t  *vk_blob;       size_t vk_len;      /* as zkg_groth16_verify                          */
    const uint64_t *primary_input; size_t n_inputs;    /* n_inputs x 4 limbs, Montgomery Fr              */
    const uint8_t  *proof;         size_t proof_len;   /* ZKG_PROOF_BYTES, libsnark compressed layout    */
} zkg_verify_item;
int zkg_groth16_verify_batch(const zkg_verify_item *items, size_t count, uint8_t *verdicts);
/* test hook: what the calling thread's last zkg_groth16_verify_batch did — out[0] combined checks, out[1] items decided by
 * zkg_groth16_verify's own code, out[2] of those, items whose B failed the GPU's G2 membership test ([r]B == O)                  */
void zkg_verify_batch_stats(size_t out[3]);
/* reduced pairing product FE(prod_i ML(g1[i], g2[i])) of n affine pairs (8 / 16 Montgomery limbs each, all-zero = infinity, which
 * contributes 1), serialised as zkg_pairing_probe's output.  Miller loops and their product on the GPU, the final exponentiation on
 * the host.  ZKG_ERROR for a point off its curve or a coordinate >= q.                                                          */
int zkg_pairing_product(const uint64_t *g1_affine, const uint64_t *g2_affine, size_t n, uint8_t out[384]);
/* ---- per-proof verification on the GPU: every item decided by its OWN equation
 *      FE(ML(A,B) ML(-acc,gamma) ML(-C,delta)) == alpha_beta, Miller loops and final exponentiation on the GPU, all items side by side.
 *      verdicts[i] == zkg_groth16_verify(items[i]) exactly (0 / 1 / 2): no random weights, no bisection, no probability attached, and a
 *      cost that does not depend on how many proofs are bad.  Nothing is asked of B or of the key's gamma, delta and alpha_beta beyond
 *      what zkg_groth16_verify asks (no subgroup tests).  The device decides an item whose key parses and holds canonical limbs, whose
 *      sizes fit and whose points and inputs are canonical and decode; everything else goes through zkg_groth16_verify's own code on the
 *      host pool.  Synchronous; host pointers; safe from several threads at once and beside the other verify entries.  ZKG_OK when every
 *      verdict was written; count == 0 and null arguments behave as zkg_groth16_verify_batch's do.                                      */
int  zkg_groth16_verify_each(const zkg_verify_item *items, size_t count, uint8_t *verdicts);
/* the calling thread's last zkg_groth16_verify_each: out[0] items decided by the device equation, out[1] items decided by the single
 * verifier's code, out[2] device rounds (chunks launched) */
void zkg_verify_each_stats(size_t out[3]);
/* test hook: positions per device round of zkg_groth16_verify_each and of zkg_zklaim_verify_each (process-wide); 0 restores the default
 * (64 MiB of staging, worked out for each entry's own layout) */
void zkg_verify_each_set_chunk(size_t positions);
/* reduced pairing product per ITEM, Miller loops AND final exponentiation on the GPU: item i uses pairs i*pairs .. i*pairs+pairs-1
 * (layouts and infinity rule as zkg_pairing_product); out: items x 384 bytes, each as zkg_pairing_probe writes one.  ZKG_ERROR for a
 * point off its curve or a coordinate >= q, and without a GPU (zkg_init).                                                       */
int  zkg_pairing_each(const uint64_t *g1_affine, const uint64_t *g2_affine, size_t items, size_t pairs, uint8_t *out);
/* test hook: the final exponentiation alone on n serialised Fq12 (384 bytes each, canonical coefficients, non-zero element; else
 * ZKG_ERROR).  where 0: the host's final_exponentiation (the specification; no GPU, no zkg_init); 1: the kernel k_final_exp_check;
 * 2: the kernel's device code compiled for the host (no GPU, no zkg_init).                                                        */
int  zkg_final_exp(const uint8_t *in, size_t n, int where, uint8_t *out);
/* test hook: Frobenius maps and the last chunk of the final exponentiation against plain square-and-multiply by q^k and by
 * the integer e (nlimbs x u32, little-endian); 0 = all agree */
int zkg_pairing_selfcheck(const uint32_t *e, int nlimbs);

/* ---- the reference's own seam (zklaim.h:257-259, libsnark_wrapper.cpp:195-276), same names and return codes, on
 *      zklaim's zklaim_ctx (include/zklaim_abi.h): the three functions zklaim.c:77-91 calls.                               */
int libsnark_trusted_setup(struct zklaim_ctx *ctx);
int libsnark_prove(struct zklaim_ctx *ctx);
int libsnark_verify(struct zklaim_ctx *ctx);
void zkg_compat_reset(void);
/* ---- many libsnark_prove calls in one (no counterpart in the reference, hence the prefix).
 * rc[i] = what libsnark_prove(ctxs[i]) returns: 0 (ZKLAIM_OK) with ctxs[i]->proof / proof_size set (malloc'ed, ZKG_PROOF_BYTES), 1 for an
 * unsatisfied credential or any other failure (the reference's two codes coincide).  A failed item leaves its ctx untouched and does
 * not disturb the others; a null ctx or one without a key is rc 1, decided before any GPU call.  Contexts are grouped by their key, every
 * group resolves its resident key once and is one zkg_groth16_prove_batch_zklaim with fresh (r, s) per item when its key batches (the
 * witnesses are generated on the GPU; ZKG_SEAM_GPU_WITNESS=0, read once, keeps the host passes), otherwise the witnesses are generated
 * side by side on the host pool and the group is one zkg_groth16_prove_batch.  Returns ZKG_OK when every rc[i] was written (count == 0: nothing is touched),
 * ZKG_ERROR for a null ctxs or rc.  Safe beside libsnark_prove on the same key from other threads. */
int zkg_zklaim_prove_batch(struct zklaim_ctx *const *ctxs, size_t count, int *rc);
/* ---- many libsnark_verify calls in one (no counterpart in the reference, hence the prefix).
 * rc[i] = what libsnark_verify(ctxs[i]) returns: 0 valid, 1 otherwise — except with probability at most (combined checks) * 2^-128, as
 * zkg_groth16_verify_batch documents.  A null ctx, or one without vk / vk_size or without proof, is rc 1, decided before any GPU call.
 * count == 0 touches nothing and returns ZKG_OK; a null ctxs or rc with count > 0 is ZKG_ERROR and nothing is written.  The same context may
 * appear more than once: verification writes nothing into a ctx.  Synchronous; host pointers; safe from several threads at once and beside
 * libsnark_verify, libsnark_prove and zkg_zklaim_prove_batch; the calling thread is bound to the seam's device (ZKG_DEVICE) as the prove
 * entries bind it; a HIP failure returns ZKG_ERROR.
 * Contexts are grouped by the bytes of ctx->vk and every group is one random linear combination on the GPU, as in zkg_groth16_verify_batch.
 * An item enters its key's combination only if proof_size == ZKG_PROOF_BYTES and its payload list (walked as zkg_zklaim_input_map walks it;
 * num_of_payloads is not trusted) yields as many inputs as the key takes; everything else — malformed or unusual keys, wrong sizes, points
 * that do not decode, non-canonical limbs, B outside G2 — goes through the single verifier's own code on the host pool, with that item's
 * input map computed on the host.  The device can do the front end too: per call, 134 bytes per proof and 80 bytes per payload go up,
 * k_proof_decode takes the square roots and k_zklaim_input_sums forms the combination's input sums from the payloads' public bytes, so no
 * public input exists on the host.  That is the default for a key's group of at least 512 payload records (entering items x payloads),
 * where it was measured no slower than hand-built items; smaller groups, and a call whose device staging would exceed 64 MiB, take the
 * host front end: zkg_zklaim_input_map per item on the host pool, then zkg_groth16_verify_batch's path.  ZKG_SEAM_GPU_VERIFY (read once
 * per process) = 0 keeps the host front end for every group, = 1 the device's.  ZKG_VERIFY_BATCH_LAPS=1 prints that entry's lap line. */
int zkg_zklaim_verify_batch(struct zklaim_ctx *const *ctxs, size_t count, int *rc);
/* what the calling thread's last zkg_zklaim_verify_batch did: out[0] combined checks, out[1] items decided by the single verifier's code,
 * out[2] items whose B failed the G2 test, out[3] items whose points and inputs the device front end produced.  Counters, not clocks. */
void zkg_zklaim_verify_batch_stats(size_t out[4]);
/* test hooks of the device front end.
 * proofs: count x 134 bytes.  A / C: count x 8 limbs, B: count x 16 limbs (affine Montgomery, all-zero = infinity), ok: count bytes
 * (bit 0 A, bit 1 B, bit 2 C decoded).  On the GPU; host pointers; needs zkg_init, no key. */
int zkg_proof_decode_gpu(const uint8_t *proofs, size_t count, uint64_t *A, uint64_t *B, uint64_t *C, uint8_t *ok);
/* contexts of ONE payload count; weights: count x 4 u32 (128-bit, as the verifier draws them); mask: count bytes or NULL (all ones);
 * sums_out: l x 4 limbs Montgomery Fr = sum over positions lo <= p < hi with mask[p] of weight_p * x_p; returns l through *n_elems.
 * On the GPU (k_zklaim_input_sums); a null context or another payload count is ZKG_ERROR. */
int zkg_zklaim_input_sums_gpu(const struct zklaim_ctx *const *ctxs, size_t count, const uint32_t *weights, const uint8_t *mask,
                              size_t lo, size_t hi, uint64_t *sums_out, size_t cap_elems, size_t *n_elems);
/* the kernel's bit rule compiled for the host: same outputs as zkg_zklaim_input_map.  No GPU, no zkg_init. */
size_t zkg_zklaim_input_map_mirror(const struct zklaim_ctx *ctx, uint64_t *out, size_t cap_elems);
/* ---- many libsnark_verify calls in one, every context decided by its OWN pairing equation on the GPU (zkg_groth16_verify_each's kernels
 * behind zkg_zklaim_verify_batch's device front end).  rc[i] == libsnark_verify(ctxs[i]) exactly: 0 valid, 1 otherwise.  No weights, no
 * bisection, no probability attached, no G2 test, and a cost that does not depend on how many proofs are bad.
 * A null ctx, or one without vk / vk_size or without proof, is rc 1, decided before any GPU call.  count == 0 touches nothing and returns
 * ZKG_OK; a null ctxs or rc with count > 0 is ZKG_ERROR and nothing is written; no GPU is ZKG_ERROR.  Synchronous; host pointers; the
 * calling thread is bound to the seam's device as zkg_zklaim_verify_batch binds it; safe from several threads at once and beside every
 * other verify and prove entry; the same context may appear more than once; nothing is written into a ctx.
 * Contexts are grouped by the bytes of ctx->vk.  A group goes to the device when its key parses, holds canonical limbs and takes
 * zv_input_count(npl) inputs for some payload count npl; an item of it enters when proof_size == ZKG_PROOF_BYTES and its payload list
 * (walked as zkg_zklaim_input_map walks it; num_of_payloads is not trusted) has npl payloads.  Per round 134 bytes per proof and 80 bytes
 * per payload go up; A, B and C are decoded on the device, and -(IC_0 + sum_k x_ik IC_k) is the sum, over the set bits of the item's input
 * string, of the entries of a per-key table T[253 k + b] = 2^b IC_k that the first call meeting the key builds on the device (it stays with
 * the verifier's cached key, at most 8 keys, about 82 KB per payload).  Everything else, and an entering item whose A, B or C does not
 * decode, is decided by the single verifier's own code on the host pool.  Rounds follow zkg_verify_each_set_chunk.                      */
int  zkg_zklaim_verify_each(struct zklaim_ctx *const *ctxs, size_t count, int *rc);
/* the calling thread's last zkg_zklaim_verify_each: out[0] items decided by the device equation, out[1] items decided by the single
 * verifier's code, out[2] device rounds, out[3] key bit tables this call had to build.  Counters, not clocks. */
void zkg_zklaim_verify_each_stats(size_t out[4]);
/* test hook of the accumulator.
 * out[i] = -(IC_0 + sum_k x_ik IC_k), affine Montgomery, all-zero = infinity; x_i = the input map of ctxs[i].
 * ic0: 8 limbs; ic: l x 8 limbs affine (all-zero = infinity), l = zv_input_count(payloads of the first non-null ctx);
 * a null ctx or another payload count: ZKG_ERROR.  where 1: table build + k_zklaim_ic_each on the GPU (needs zkg_init);
 * where 2: the same device text compiled for the host (no GPU, no zkg_init). */
int zkg_zklaim_ic_each(const uint64_t *ic0, const uint64_t *ic, const struct zklaim_ctx *const *ctxs, size_t count, int where, uint64_t *out);

/* ---- test hooks of the key blob's point codec (csrc/codec.hip).  The decoding rule of a compressed point, shared by the key loader, the
 *      proof decoder, the host's decoder and the single verifier: '1' first is infinity and nothing else is read; otherwise the flag is
 *      '0', the parity byte '0' or '1', every x coordinate's limbs are below q, x^3 + b is a square, and y is the root whose canonical lsb
 *      (of y.c0 in G2) is the parity byte.  Anything else is refused.
 * zkg_point_decompress: n records `stride` bytes apart, the point `offset` bytes into its record, in the loader's layouts: G1 (g2 = 0)
 *   at stride 34 offset 0 or stride 100 offset 66, G2 (g2 = 1) at stride 66 or 100, offset 0.  out: n x 8 (G2: 16) limbs, affine Montgomery,
 *   all-zero for infinity AND for a refused record; *flag: non-zero iff a record was refused.
 *   where 1: the loader's own path (decompress_dev with k_decompress_g1 / k_decompress_g2; needs zkg_init); 0: the host's ser::get_g1 /
 *   get_g2 with the canonical check (no GPU, no zkg_init).
 * zkg_point_compress: rec 34: record i = G1 g1[i], i < n <= npoints.  rec 100: record i = G2 g2[idx[i]] then G1 g1[idx[i]], idx[i] <
 *   npoints (a knowledge commitment of the sparse B query; g2 and idx are read for rec 100 only).  Points as above.  out: n x rec bytes.
 *   guard (optional): 16 bytes placed behind the run before it is written and read back afterwards: a writer that stays inside its run
 *   leaves them as they were.  where 1: compress_g1_records / compress_kc_records into 16-byte aligned device staging, as the key
 *   writer of libsnark_trusted_setup calls them (needs zkg_init); 0: the host's ser::put_g1 / put_g2.
 * Both: ZKG_ERROR for a null argument, another layout or record size, an index beyond the points, n (or npoints) above 2^20. */
int zkg_point_decompress(const uint8_t *records, size_t stride, size_t offset, size_t n, int g2, int where, uint64_t *out, uint32_t *flag);
int zkg_point_compress(const uint64_t *g1, const uint64_t *g2, const uint32_t *idx, size_t npoints, size_t n, int rec, int where, uint8_t *out,
                       uint8_t guard[16]);

/* ---- known-answer hook for the device arithmetic (libff Fp_model<4,...>::mul_reduce, Fp2_model —
 *      here the generated v_mad_u64_u32 streams of csrc/mont_asm.inc).  Element-wise ON THE GPU, host pointers:
 *      field 0 = Fq, 1 = Fr (4 limbs per element), 2 = Fq2 (8 limbs);  op 0 mul, 1 add, 2 sub, 3 inverse, 4 to Montgomery form,
 *      5 from Montgomery form, 6 negate, 7 square (4 and 5: Fq / Fr only).  Inputs and outputs are Montgomery limbs except op 4's
 *      input and op 5's output (canonical); outputs are fully reduced.  b is read by ops 0-2 only.
 *      Fq only, ops 10-14: the same arithmetic on the 9 x 29-bit representation of the bucket-accumulation kernel (csrc/fq29.hip.hpp),
 *      entered and left through its conversions: 10 mul, 11 add, 12 sub, 13 a if a != b else 0 (its zero test), 14 the composite
 *      (b-a)(a-b) - (b-a)^2 - 2ab with unnormalised intermediate sums, as the mixed addition chains them, 15 the inverse of 3a
 *      (safegcd divsteps on 30-bit limbs, f29::inverse: what the table levels and fixed-base batches normalise through; 0 -> 0).
 *      The lazy range of the 32-bit layer, all three fields.  On the device a value is any representative in [0, 2p) (Fq2: per component), and
 *      NO input of any op is normalised before the operation, so a caller may pass limbs anywhere below 2p.
 *      8 dbl(a), fully reduced like ops 0-7.
 *      RAW stores (the result leaves WITHOUT normalized(): the limbs are the operator's own, in [0, 2p)):
 *      20 mul, 21 add, 22 sub, 26 negate, 27 square, 28 dbl  (ops 0, 1, 2, 6, 7, 8 plus 20).
 *      40  ((a*b) - a) * (a + b)
 *      41  x <- a; 8 times: x <- (x + x) - b
 *      42  M = a.sqr().dbl() + a.sqr();  M.sqr() - (a*b).dbl()          (the shape XYZZ::dbl_inl builds)
 *      with no normalisation between the steps of 40-42.
 *      Predicates, the integer 0 or 1 in 32-bit limb 0 of the result (all other limbs 0):  30 a.is_zero(), 31 a == b
 *      (Fq2: both components take part).  b is read by ops 0-2, 20-22, 31 and 40-42.                                                       */
int zkg_field_op(int field, int op, const uint64_t *a, const uint64_t *b, size_t n, uint64_t *out);

/* known-answer hook for the NTT's 29-bit Fr arithmetic (csrc/fr29.hip.hpp: Fr as nine 29-bit limbs, R' = 2^261, lazy limb-wise sums).
 * Element-wise ON THE GPU, one lane per element, host pointers, RAW limbs: element i reads k vectors of nine 32-bit limbs at
 * in + 9 k i and writes m vectors at out + 9 m i, so a caller can place limbs at the lazy bounds.  No input is range-checked.
 *   op  0  mul(a, b)                      k 2, m 1     the single product stream (a: data side, b: table side)
 *       1  mul2(a, b, c, d)               k 4, m 2     the interleaved pair: a b and c d
 *       2  norm(a)                        k 1, m 1     carry propagation
 *       3  add_norm(a, b)   4  sub_norm(a, b)   5  add_lazy(a, b)   6  sub_lazy(a, b)          k 2, m 1     (subtractions: a + 2r - b)
 *       7  slice(x)                       k 1, m 1     x: eight 32-bit words of libff's form in the first eight slots (the ninth is ignored)
 *       8  unslice_reduce(a)              k 1, m 1     out: eight 32-bit words, the ninth slot zero
 *       9  the radix-4 step of k_ntt_pass29_r4, a stage with a product: in x0 x1 x2 x3 wa wb wc, out the four stored rows       k 7, m 4
 *      10  the same at stage 0 (wa unused)     11  op 9 with the carry propagations on the stores (ZKG_NTT_NORM_STORES)     12  op 10 likewise
 *      13  the radix-2 step that ends an odd R: in u v w, out the two stored rows       k 3, m 2          14  the same at stage 0 (w unused)
 * Ops 9-14 run a copy of the kernel's step bodies (csrc/capi.hip, marked at both places): the kernel keeps its own text.  n at most 2^24. */
int zkg_fr29_op(int op, const uint32_t *in, size_t n, uint32_t *out);

/* known-answer hook for the multi-exponentiation's 29-bit Fq arithmetic (csrc/fq29.hip.hpp: Fq as nine 29-bit limbs, R' = 2^261, values kept
 * lazily above q, subtractions through spread multiples of q): the functions of that file themselves, ON THE GPU, host pointers, RAW limbs
 * (no to29 on the way in, no from29 on the way out), so a caller can place limbs and values at the bounds the file's comments state.
 * Element i reads k vectors of nine 32-bit limbs at in + 9 k i and writes m vectors at out + 9 m i.  No input is range-checked.
 *   op  0  mul(a, b)         k 2, m 1         1  mul2(a, b, c, d): a b and c d   k 4, m 2
 *       2  sqr(a)            k 1, m 1         3  sqr2(a, c): a^2 and c^2         k 2, m 2
 *       4  norm(a)   6  dbl(a)   11  S2_1 - a                                    k 1, m 1
 *       5  add(a, b)   7 - 10  a + S - b for S = S2_1, S4_1, S6_1, S4_3, unnormalised, as f29::sub returns it          k 2, m 1
 *      12  is_zero_mod_p(a): limb 0 of the result is 0 or 1                     k 1, m 1
 *      13  unpack   14  to29: eight 32-bit words of libff's form in the first eight slots (the ninth is ignored)       k 1, m 1
 *      15  from29: out eight 32-bit words, the ninth slot zero                  k 1, m 1
 *      16  x, y, flag (limb 0: infinity) -> store_rec64 -> load_rec64 -> x, y, flag                                    k 3, m 3
 *      17  x, y, zz, zzz, flag -> store_bucket29 -> load_bucket29_raw -> x, y, zz, zzz                                 k 5, m 4
 *      18  inverse(a) (a launch's tail lanes invert 1: the early exit is a wavefront vote)                             k 1, m 1
 *      19  XYZZ29::madd: in x, y, zz, zzz, bx, by, flag (limb 0: the accumulator is infinity); out x, y, zz, zzz (all zero for infinity),
 *          flag (limb 0: infinity, limb 1: what madd returned).  A false return continues as k_bucket_accum29 does (from29, the 32-bit
 *          madd, to29 — a copy of the kernel's lines, csrc/capi.hip, marked at both places).                           k 7, m 5
 *      20  xyzz29_add_lane   21  xyzz29_add_pair (2 lanes per element)   22  xyzz29_add_quad (4 lanes per element): in two points of four
 *          coordinates, infinity all zero; out the sum's four coordinates                                              k 8, m 4
 * zkg_fq29_op_chain: ops 19-22 with 0 <= chain <= 64.  19: 1 + chain times acc <- acc + b (the flag is the last step's);  20-22: a + b, then
 * `chain` rounds of x <- 2x + b, so stored invariants are re-entered without leaving the device.  Other ops take chain 0.  n at most 2^24. */
int zkg_fq29_op(int op, const uint32_t *in, size_t n, uint32_t *out);
int zkg_fq29_op_chain(int op, int chain, const uint32_t *in, size_t n, uint32_t *out);

/* known-answer hook for the pairing's device tower (csrc/pairing.hip.hpp, csrc/final_exp.hip.hpp: Fq12 over Fq6 over Fq2 on values kept lazily
 * in [0, 2q)): the functions of those files themselves on RAW limbs.  An element is 96 32-bit words, the twelve Fq coefficients in the order
 * c0.c0.c0, c0.c0.c1, c0.c1.c0 .. c1.c2.c1 (FeSlots::each_fq), eight little-endian words of Montgomery form each; element i of a, b and out
 * is at word 96 i.  No word is normalised on the way in or out, so a caller can place coefficients anywhere in the lazy range and sees the
 * representative an operation leaves.  b is read by ops 0 and 2 only.
 *   op  0  a * b (Fq12 operator*)          1  a.sqr() (complex squaring)          2  mul_by_line2(a, l0, l1, l2): the line's three Fq2 in the
 *       first 48 words of b's element      3  cyclotomic_sqr(a) (specified in the cyclotomic subgroup only)      4  inverse(a) (0 -> 0)
 *       5  conjugate(a)      6 - 8  frobenius<1>, <2>, <3>(a) with the verifier's FrobConsts      9  Fq6::mul_by_v on both halves of a
 * where 1: one lane per element on the GPU (kernel k_fq12_op; needs zkg_init); 2: the same text compiled for the host, which computes on
 * canonical values: a coefficient >= q is ZKG_ERROR.  n at most 2^20.                                                                   */
int zkg_fq12_op(int op, const uint32_t *a, const uint32_t *b, size_t n, int where, uint32_t *out);

/* known-answer hook for the 29-bit group law of the bucket-reduction kernels (csrc/fq29.hip.hpp, xyzz29_add_quad): on the GPU,
 * out[i] = a[i] + b[i], then `chain` rounds of x <- 2x + b[i]; points as normalised Jacobian (12 limbs), host pointers.          */
int zkg_g1_add_quad29(const uint64_t *a_jac, const uint64_t *b_jac, size_t n, int chain, uint64_t *out_jac);
/* the same for the pair form the bucket reduction uses since round 4 (xyzz29_add_pair: lane 0 of a pair holds (X, ZZ), lane 1 (Y, ZZZ)) */
int zkg_g1_add_pair29(const uint64_t *a_jac, const uint64_t *b_jac, size_t n, int chain, uint64_t *out_jac);

/* known-answer hook for the 32-bit device group law (csrc/curve.hip.hpp as the device compiles it: lazy values in [0, 2p), zero as 0 or p):
 * element-wise ON THE GPU, host pointers.  group 0 = G1 over Fq, 1 = G2 over Fq2.  Inputs are RAW records of 32-bit limbs exactly as the
 * device structs lay them out — XYZZ<F> = x, y, zz, zzz and Affine<F> = x, y, each coordinate 8 (Fq) or 16 (Fq2: c0 then c1) little-endian
 * limbs of Montgomery form — and nothing is normalised on the way in, so a caller can place any representative below 2p in any coordinate,
 * ZZ != 1 included; infinity is ZZ == 0 (XYZZ) and x == y == 0 (affine), in either representative of zero.  No input is range-checked.
 * Outputs are XYZZ<F>::normalized() (op 5: Affine<F>::normalized()).
 *   op 0  madd        a.madd(b)                 a XYZZ, b affine
 *      1  add         a.add_inl(b)              a, b XYZZ
 *      2  add_quad    xyzz_add_quad<F>(a, b, lane & 3): four lanes per element hold identical copies; out holds all FOUR lanes' results,
 *                     4 n XYZZ records, element i's at 4 i .. 4 i + 3 (they must be equal)
 *      3  dbl         a.dbl_inl()               a XYZZ
 *      4  dbl_affine  XYZZ::dbl_affine_inl(a)   a affine (no infinity check there: the callers make it)
 *      5  to_affine   a.to_affine()             a XYZZ, out affine
 *      6  mul         a.mul(k, 8)               a XYZZ, k eight raw 32-bit limbs per element (any 256-bit value)
 * chain (ops 0-2 only, 0 .. 64; otherwise 0): x <- a + b, then `chain` rounds of x <- 2x + b with 2x = x.add_inl(x) (op 2: xyzz_add_quad(x, x)),
 * which takes the doubling branch, and + b the op itself.  b is read by ops 0-2, k by op 6.  n at most 2^20. */
int zkg_curve_op(int group, int op, const uint32_t *a, const uint32_t *b, const uint32_t *k, size_t n, int chain, uint32_t *out);

/* kernel-only timing hooks for bench.py (HIP events on the stream the kernels run on): average device ms per launch of the dominant kernel
 * since the last reset.  Every fourth call of an MSM entry point is timed, with all of its launches (the event records cost the stream they
 * sit on: 2 % of a 2^20-point step when every launch carries them; ZKG_KERNEL_TIMER_STRIDE=1 times every call); *launches is the launch
 * count of ALL calls since the reset, so that average x launches / calls is the kernel's time per call. */
void  zkg_timing_reset(void);
float zkg_timing_dominant_ms(int *launches);

#ifdef __cplusplus
}
#endif
#endif /* ZKG_H */
