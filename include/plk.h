/*
 * plk.h — C ABI of the MI355X PLONK hot path (BLS12-381 Fr NTT family + G1 MSM/KZG commit).
 *
 * This is the drop-in boundary. In the reference the path sits behind Rust generic
 * structs of un-vendored crates (no FFI exists there); each entry point
 * below replaces one of those calls. The host-side mirror that calls this ABI with the
 * reference's names is dusk-plonk_amd/plonk.py + dusk-plonk_amd/prover.py (Python, used by
 * the tests and bench.py); the C++ prover behind plk_prove is dusk-plonk_amd/csrc/prover.hip
 * (composer: composer.hip, proving key: key.hip, commits: commit.hip).
 * INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *  - plk_fr is BlsScalar exactly as the reference stores it: 4 little-endian u64 limbs
 *    in Montgomery form with R = 2^256 (pinned by /root/reference/src/lib.rs:583-588).
 *  - plk_g1 is G1Affine: x, y as 6 LE u64 limbs of Montgomery Fp (R = 2^384), plus an
 *    infinity flag (0/1) widened to u64. Outputs are canonical (fully reduced, and the
 *    point at infinity is written as x = y = 0, infinity = 1).
 *  - Host pointers are caller-owned; in-place use (same in/out) is allowed.
 *    Entry points with the _dev suffix take device pointers and a hipStream_t (passed as
 *    void*, NULL = the context's stream) and are stream-ordered.
 *  - Every entry point returns a plk_status; nothing throws or aborts across the ABI.
 *  - One plk_ctx per GPU. A context may be used from one thread at a time; concurrent
 *    streams must pass their own scratch buffers (plk_ntt_dev) / workspaces.
 */
#ifndef PLK_H
#define PLK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLK_ABI_VERSION 2

typedef struct { uint64_t l[4]; } plk_fr;                          /* 32 bytes  */
typedef struct { uint64_t x[6]; uint64_t y[6]; uint64_t infinity; } plk_g1; /* 104 bytes */

typedef enum {
  PLK_OK = 0,
  PLK_E_DEGREE = 1,   /* commit: polynomial (trailing zeros stripped) longer than the SRS
                         — zksnarks PlonkParams::commit error path (prover.rs:133-452) */
  PLK_E_ARG = 2,      /* bad argument (null pointer, length > domain, bad log_n, ...) */
  PLK_E_DEVICE = 3,   /* HIP runtime error */
  PLK_E_OOM = 4,      /* device allocation failed */
  PLK_E_NODEV = 5,    /* no GPU visible / HIP unavailable */
  PLK_E_UNSUPPORTED = 6 /* reserved: a feature this backend does not implement */
} plk_status;

typedef struct plk_ctx plk_ctx;
typedef struct plk_domain plk_domain;
typedef struct plk_srs plk_srs;
typedef struct plk_composer plk_composer;
typedef struct plk_key plk_key;

/* ---- library / context ------------------------------------------------------------- */
int plk_abi_version(void);
const char* plk_status_str(int status);
/* Build provenance (no reference counterpart): "src=<16 hex> flags=<16 hex> variant=<name>",
 * src = a hash of csrc/ *.hip, csrc/ *.hpp and this header as they were compiled, flags = a hash
 * of the hipcc flags (build_ext.py source_id / flags_id). The Python mirror refuses a library
 * whose src differs from the tree it is loaded from (plonk.check_build). */
const char* plk_build_info(void);
/* Number of visible GPUs (0 when no GPU; never fails for lack of one). */
int plk_device_count(int* out);
int plk_ctx_create(int device, plk_ctx** out);
int plk_ctx_destroy(plk_ctx* ctx);
/* The context's default stream (hipStream_t) — for callers that chain _dev calls. */
int plk_ctx_stream(plk_ctx* ctx, void** stream_out);
int plk_ctx_synchronize(plk_ctx* ctx);

/* ---- evaluation domains: poly_commit::Fft<Fr> -------------------------------------- */
/* Fft::new(k) (prover.rs:88, quotient_poly.rs:52, key.rs:83,222). Cached per ctx and k:
 * w = ROOT_OF_UNITY^(2^(32-k)), coset shift g = 7, tables resident in HBM. 0 <= k <= 27. */
int plk_domain_get(plk_ctx* ctx, uint32_t log_n, plk_domain** out);
/* Fft::size(), generator() (= w), generator_inv(), size_inv(), and the coset shift g, g^-1.
 * Any output pointer may be NULL. (prover.rs:252,446; key.rs:205-207) */
int plk_domain_info(const plk_domain* d, uint64_t* size, plk_fr* generator,
                    plk_fr* generator_inv, plk_fr* size_inv, plk_fr* coset, plk_fr* coset_inv);
/* Fft.elements: out[i] = w^i, i < n (permutation.rs:148,246). */
int plk_domain_elements(const plk_domain* d, plk_fr* out);
/* Fft::compute_vanishing_poly_over_coset(poly_degree) (key.rs:291):
 * out[i] = (g * w^i)^poly_degree - 1, i < n. */
int plk_domain_vanishing_over_coset(const plk_domain* d, uint64_t poly_degree, plk_fr* out);

/* ---- the NTT family (host buffers) --------------------------------------------------
 * dir = +1: Fft::dft (coset = 0) / Fft::coset_dft (coset = 1)
 *           input: len_in <= n coefficients (zero-padded to n); output: n evaluations.
 *           (permutation.rs:232; quotient_poly.rs:54-58,145,237; key.rs:226-245)
 * dir = -1: Fft::idft (coset = 0) / Fft::coset_idft (coset = 1)
 *           input: len_in <= n evaluations (zero-padded); output: n coefficients.
 *           (prover.rs:121-124,192,229; quotient_poly.rs:115,271; permutation.rs:194-197;
 *            key.rs:121-131)
 * `inout` must hold n elements; natural order in and out. */
int plk_ntt(plk_domain* d, plk_fr* inout, size_t len_in, int dir, int coset);
/* plk_ntt on the caller's stream (hipStream_t as void*, NULL = the context's stream), the
 * signature of SURVEY §8b: same semantics, host buffer in and out, returns once `inout`
 * holds the result (the reference's Fft calls block). Staging and scratch are stream-ordered
 * allocations of its own, so callers on different streams may share one domain. */
int plk_ntt_stream(plk_domain* d, plk_fr* inout, size_t len_in, int dir, int coset, void* stream);
/* Device-pointer variant: d_in -> d_out (may alias; both hold n elements). d_scratch is
 * NULL (use the domain's scratch — then calls on one domain must share one stream) or a
 * device buffer of 2*n elements owned by the caller. */
int plk_ntt_dev(plk_domain* d, const plk_fr* d_in, plk_fr* d_out, size_t len_in, int dir,
                int coset, plk_fr* d_scratch, void* stream);
/* Batched device variant: `count` independent vectors, vector v at d_inout + v*n. */
int plk_ntt_batch_dev(plk_domain* d, plk_fr* d_inout, size_t count, int dir, int coset,
                      void* stream);

/* ---- SRS and KZG commit: zksnarks::plonk::PlonkParams<TatePairing> ------------------ */
/* PlonkParams::setup(k, rng) restated with an explicit secret tau (Montgomery Fr):
 * g1[i] = [tau^i]G1 for i < n_points, generated on the GPU. If out_points != NULL the
 * points are also copied to the host. The returned SRS is resident and MSM-ready. */
int plk_srs_setup(plk_ctx* ctx, const plk_fr* tau, size_t n_points, plk_g1* out_points,
                  plk_srs** out);
/* The slice [start, start + n_points) of the same SRS (g1[i] = [tau^i]G1 for i in the
 * range): the per-GPU shard of a sharded MSM. */
int plk_srs_setup_range(plk_ctx* ctx, const plk_fr* tau, uint64_t start, size_t n_points,
                        plk_g1* out_points, plk_srs** out);
/* Load an existing SRS (e.g. a trimmed PlonkParams) from host affine points. The points are
 * taken on faith: plk_srs_verify (below) checks them and their structure against an opening key. */
int plk_srs_load(plk_ctx* ctx, const plk_g1* points, size_t n_points, plk_srs** out);
/* The Lagrange-basis SRS of the 2^log_n-point domain, computed from the first 2^log_n + 3
 * points of `srs` alone (an inverse DFT over G1): point i < n is [L_i(tau)]G1, and points
 * n, n + 1, n + 2 are [tau^(n+t)]G1 - [tau^t]G1, t = 0, 1, 2. A commit of the scalars
 * [p(omega^0) .. p(omega^(n-1)) | b_0 b_1 b_2] on it is the commit of p(X) + b(X)(X^n - 1) on
 * `srs`. An ordinary SRS (plk_commit, plk_srs_points, ...) that the caller destroys; points at
 * infinity occur when tau is an n-th root of unity. PLK_E_ARG when `srs` has fewer than
 * n + 3 points. plk_key_compile builds the key's own (round 1 commits the wire polynomials
 * from their values on it) unless PLK_LAGRANGE_COMMIT=0 is set in the environment. */
int plk_srs_lagrange(plk_srs* srs, uint32_t log_n, plk_srs** out);
int plk_srs_destroy(plk_srs* srs);
int plk_srs_len(const plk_srs* srs, size_t* n_points);
/* Copy SRS points [start, start+count) back to the host. */
int plk_srs_points(const plk_srs* srs, size_t start, size_t count, plk_g1* out);

/* Raw MSM: out = sum_{i<len} scalars[i] * g1[i], len <= n_points (msm_curve_addition,
 * proof.rs:507; the inner loop of commit). */
int plk_msm(plk_srs* srs, const plk_fr* scalars, size_t len, plk_g1* out);
/* PlonkParams::commit(&Coefficients) (prover.rs:133-136,194,262-265,440,452;
 * key.rs:138-159): strips trailing zeros; PLK_E_DEGREE if the rest is longer than the
 * SRS; otherwise out = MSM over the SRS prefix. */
int plk_commit(plk_srs* srs, const plk_fr* coeffs, size_t len, plk_g1* out);
/* Device-pointer commit (coefficients already in HBM, e.g. straight from plk_ntt_dev). */
int plk_commit_dev(plk_srs* srs, const plk_fr* d_coeffs, size_t len, plk_g1* out,
                   void* stream);

/* Batched device commit: `count` independent polynomials (d_coeffs[k], lens[k]) committed
 * as one GPU batch (their kernels share launches; the latency-bound reduction tails of the
 * batch overlap). Used for the prover's independent commit groups: the 4 wire commits
 * (prover.rs:133-136), the 4 quotient chunks (:262-265) and the 2 openings (:440,452).
 * statuses (nullable) gets each commit's status; returns PLK_E_DEGREE if any failed. */
int plk_commit_batch_dev(plk_srs* srs, const plk_fr* const* d_coeffs, const size_t* lens,
                         size_t count, plk_g1* outs, int* statuses, void* stream);

/* Bucket-range part of plk_commit_batch_dev (round 5; SURVEY §8e, the north star's "partial
 * bucket sums for a single large MSM"): the same commits, but only the Pippenger buckets of
 * part `part` of `parts` (parts a power of two): bucket range [part, part + 1) x 2^(c-1) /
 * parts of the SRS's window size c. outs[k] is that range's share sum_{b in range} (b + 1) S_b
 * of commit k; the shares of parts 0 .. parts-1 sum (plk_g1_sum) to plk_commit_batch_dev's
 * outputs. Every part reads all scalars and the whole window table, sorts and accumulates
 * only its buckets' entries and reduces only its buckets: one GPU per part, each doing
 * ~1/parts of the accumulation AND of the bucket reduction (the SRS-slice split,
 * plk_prover_shard / plk_msm_sharded, divides only the accumulation). The degree check runs
 * in every part (same status everywhere). PLK_E_ARG unless 2^(c-1) > 32768 (a wide bucket
 * set, c >= 17: SRS >= 2^16 points) and 2^(c-1) / parts >= 2^14. */
int plk_commit_batch_dev_part(plk_srs* srs, const plk_fr* const* d_coeffs, const size_t* lens,
                              size_t count, uint32_t part, uint32_t parts, plk_g1* outs,
                              int* statuses, void* stream);

/* PlonkParams::compute_aggregate_witness(&[p_0..p_(k-1)], &point, &v) (prover.rs:422-438,
 * 444-450): W(X) = (sum_i v^i p_i(X)) / (X - point), the remainder dropped (Ruffini). The
 * k polynomials (d_polys[i], lens[i] coefficients) are device pointers; d_out receives
 * *out_len = max(lens) - 1 coefficients (0 when every polynomial is constant or empty),
 * stream-ordered. point and v must be canonical (PLK_E_ARG otherwise). The same division
 * plk_prove runs for its two openings; exported so the primitive itself can be replaced. */
int plk_aggregate_witness_dev(plk_ctx* ctx, const plk_fr* const* d_polys, const size_t* lens,
                              size_t count, const plk_fr* point, const plk_fr* v,
                              plk_fr* d_out, size_t* out_len, void* stream);
/* Host-buffer variant on the context's stream; returns when `out` holds the result. */
int plk_aggregate_witness(plk_ctx* ctx, const plk_fr* const* polys, const size_t* lens,
                          size_t count, const plk_fr* point, const plk_fr* v, plk_fr* out,
                          size_t* out_len);

/* Host-side sum of n affine points (canonical affine out): the local fold after the RCCL
 * all-gather of per-GPU partial commitments of a sharded MSM. Needs no GPU. */
int plk_g1_sum(const plk_g1* points, size_t n, plk_g1* out);

/* One large MSM split over the GPUs of a node from ONE process:
 * per_gpu[i] holds the SRS points following those of per_gpu[0..i-1] (e.g.
 * plk_srs_setup_range on consecutive ranges, one slice per device). Each slice's MSM of its
 * scalar slice runs concurrently (one host thread per slice, each on its own device and
 * stream) and the partial points are folded on the host (plk_g1_sum):
 * out = sum_{i<len} scalars[i] * g1[i], len <= total points. The multi-process form (one
 * rank per GPU, RCCL all-gather of the partials) is dusk-plonk_amd/parallel.py. */
int plk_msm_sharded(plk_srs* const* per_gpu, int n_gpu, const plk_fr* scalars, size_t len,
                    plk_g1* out);

/* msm_curve_addition(points, scalars) for arbitrary affine points (proof.rs:507): canonical
 * affine out. Variable-base Pippenger (csrc/msm_var.hip): no precomputed window table, the
 * points are used once. Host buffers; n = 0 gives the identity. Identity inputs (infinity = 1)
 * are legal and skipped; a finite point with a coordinate >= p or off y^2 = x^3 + 4, or an
 * infinity word other than 0 / 1, gives PLK_E_ARG. Subgroup membership is not checked here:
 * screen points with plk_g1_subgroup_check_batch (or decode them with plk_g1_decompress_batch /
 * plk_proofs_ingest, which check it). One call at a time per context. */
int plk_msm_points(plk_ctx* ctx, const plk_g1* points, const plk_fr* scalars, size_t n, plk_g1* out);
/* Several sums over disjoint index ranges of ONE point array as one GPU batch:
 * outs[k] = sum_{i in [starts[k], starts[k] + lens[k])} scalars[i] * points[i], k < count <= 16,
 * every range inside [0, n). What plk_verifier_fold runs for its two sums. */
int plk_msm_points_ranges(plk_ctx* ctx, const plk_g1* points, const plk_fr* scalars, size_t n,
                          const size_t* starts, const size_t* lens, size_t count, plk_g1* outs);

/* ---- instrumentation (bench / profiling) ------------------------------------------- */
/* Milliseconds of the dominant kernel of the most recent plk_commit/plk_msm on this SRS
 * (bucket accumulation), measured with HIP events on the launching stream; and the
 * number of bucket-accumulation point additions it performed. */
int plk_srs_last_msm_stats(const plk_srs* srs, float* accumulate_ms, uint64_t* point_adds,
                           uint32_t* window_bits);
/* Cumulative accumulation statistics since the last reset (measurement only): summed
 * k_accumulate time (HIP events on the MSM's stream), launches, point additions and MSM
 * points (scalar counts over all slots). */
int plk_srs_msm_stats_reset(plk_srs* srs);
int plk_srs_cum_msm_stats(const plk_srs* srs, double* accumulate_ms, uint64_t* launches,
                          uint64_t* point_adds, uint64_t* points);
/* The layout of this SRS's MSM table: naf = 1 for the row table (a row 2^p P for every bit position
 * p < rows = 255, scalars recoded as a signed sliding window), 0 for the window table (rows = the
 * window count); table_bytes = device memory of the table and its infinity flags. */
int plk_srs_table_layout(const plk_srs* srs, uint32_t* naf, uint32_t* rows, uint64_t* table_bytes);
/* The layout an SRS of n_points at window_bits would be set up with, before the allocation is
 * tried (no GPU needed): PLK_MSM_NAF = 1 / 0 asks for / forbids the row table, which only bucket
 * sets of window_bits >= 17 support; c_from_env: the window size came from PLK_MSM_C. A row table
 * above PLK_MSM_TABLE_CAP bytes (when set) counts as one that cannot be allocated: the window
 * table then, as after a failed allocation. */
int plk_msm_table_policy(uint64_t n_points, uint32_t window_bits, int c_from_env, uint32_t* naf,
                         uint64_t* table_bytes);

/* ---- prover: Plonk composer, PlonkKey::compile, Prover::create_proof --------------------
 * The callers of the hot path, restated on the C++ host with every O(n) step
 * on the GPU. A constraint is one width-4 gate
 *   q_m a b + q_l a + q_r b + q_o o + q_4 d + q_c + PI = 0   (src/lib.rs:546) plus the
 * widget selectors; a, b, o, d are witness indices. Field order follows
 * zksnarks::Constraint. */
typedef struct {
  plk_fr q_m, q_l, q_r, q_o, q_4, q_c, q_arith, q_range, q_logic, q_fixed_group_add,
      q_variable_group_add;
  uint32_t a, b, o, d;
  uint32_t has_public, _pad;
  plk_fr public_input;
} plk_constraint;

/* zksnarks Proof (src/prover/proof.rs:36-66) with ProofEvaluations in construction order
 * (src/prover/linearization_poly.rs:117-134). */
typedef struct {
  plk_g1 a_comm, b_comm, c_comm, d_comm, z_comm, t_low_comm, t_mid_comm, t_high_comm, t_4_comm,
      w_z_chall_comm, w_z_chall_w_comm;
  plk_fr a_eval, b_eval, c_eval, d_eval, a_next_eval, b_next_eval, d_next_eval, q_arith_eval,
      q_c_eval, q_l_eval, q_r_eval, s_sigma_1_eval, s_sigma_2_eval, s_sigma_3_eval, r_poly_eval,
      perm_eval;
} plk_proof;

/* Plonk::initialize (src/lib.rs:121-134): zero/one witnesses, their constant gates and
 * two rounds of dummy gates. */
int plk_composer_create(plk_composer** out);
int plk_composer_destroy(plk_composer* c);
int plk_composer_size(const plk_composer* c, size_t* gates, size_t* witnesses);
int plk_composer_append_witness(plk_composer* c, const plk_fr* value, uint32_t* wire);
int plk_composer_witness_value(const plk_composer* c, uint32_t wire, plk_fr* value);
int plk_composer_set_witness(plk_composer* c, uint32_t wire, const plk_fr* value);
/* append_public (lib.rs:708-719) */
int plk_composer_append_public(plk_composer* c, const plk_fr* value, uint32_t* wire);
/* append_gate (lib.rs:546-550, q_arith = 1) / append_custom_gate (lib.rs:224-240) */
int plk_composer_append_gate(plk_composer* c, const plk_constraint* s);
int plk_composer_append_custom_gate(plk_composer* c, const plk_constraint* s);
/* gate_add / gate_mul (lib.rs:1169-1197): q_o = -1, output evaluated and appended */
int plk_composer_gate_eval(plk_composer* c, const plk_constraint* s, uint32_t* out_wire);
int plk_composer_assert_equal(plk_composer* c, uint32_t a, uint32_t b);            /* :721 */
int plk_composer_assert_equal_constant(plk_composer* c, uint32_t a, const plk_fr* constant,
                                       const plk_fr* public_input /* nullable */);  /* :766 */
int plk_composer_component_boolean(plk_composer* c, uint32_t a);                   /* :859 */
/* component_range (lib.rs:1066-1163): constrain `a` to num_bits (<= 256) bits with the
 * range widget; an out-of-range value makes create_proof fail (tests/range.rs:82-84). */
int plk_composer_component_range(plk_composer* c, uint32_t a, size_t num_bits);
/* The bench circuit: `gates` chained gates x' = x*y + x (q_m = q_l = 1, q_o = -1). */
int plk_composer_synthetic_chain(plk_composer* c, size_t gates, uint64_t seed);
/* Plonk::instance(): public inputs sorted by gate index, and their indexes. */
int plk_composer_public_inputs(const plk_composer* c, plk_fr* values, uint64_t* indexes,
                               size_t cap, size_t* count);
/* The circuit as the composer holds it (Plonk::constraints and the witness vector,
 * lib.rs:103-115): gates[i] for i < min(cap, m) and witness[j] for j < min(wcap, #witness);
 * *m / *nw receive the full sizes. For external checkers and serialisation. */
int plk_composer_export(const plk_composer* c, plk_constraint* gates, size_t cap,
                        plk_fr* witness, size_t wcap, size_t* m, size_t* nw);

/* PlonkKey::compile_with_circuit (src/key.rs:63-327): device-resident proving key for the
 * circuit's structure, committed against `srs` (trimmed to next_pow2(m + 6) + 8 points).
 * All five widgets are proven: arithmetic, range, logic, fixed-base scalar multiplication
 * and variable-base addition (quotient_poly.rs:128-262, linearization_poly.rs:136-225). */
int plk_key_compile(plk_srs* srs, const plk_composer* circuit, const char* label, plk_key** out);
int plk_key_destroy(plk_key* key);
/* n (padded domain), m (gates) and the 15 verifier-key commitments in transcript order
 * q_m q_l q_r q_o q_c q_4 q_arith q_range q_logic q_fixed_group_add q_variable_group_add
 * s_sigma_1..4. */
int plk_key_info(const plk_key* key, uint64_t* n, uint64_t* m, plk_g1* commitments);
/* Prover::create_proof (src/prover.rs:67-474) for a circuit with the key's structure and
 * its own witness values. Blinding randomness comes from `seed` (SplitMix64). Fails with
 * PLK_E_DEGREE exactly where the reference's commit fails for an unsatisfied circuit, and
 * with PLK_E_ARG when the circuit's structure (gates, wires, selectors, public-input
 * positions) differs from the one the key was compiled from or its witness vector is too
 * short for the key's wires. */
int plk_prove(plk_key* key, const plk_composer* circuit, uint64_t seed, plk_proof* proof,
              plk_fr* public_inputs, size_t pi_cap, size_t* pi_count);

/* ---- prover lanes: several proofs in flight over one key ----------------------------
 * Prover: Clone + create_proof(&self) may run concurrently in the reference.
 * A plk_prover is one such concurrent prover: its own HIP stream, MSM workspace, NTT
 * scratch and per-proof buffers, sharing the key's device-resident tables and the SRS
 * window table read-only (one copy per GPU however many proofs are in flight). Provers of
 * one key may run plk_prover_prove from different threads at the same time. Destroy every
 * prover of a key before the key. plk_prove(key, ...) is plk_prover_prove on a default
 * prover the key owns (on the context's stream); it is thread-safe, but concurrent
 * plk_prove calls on one key are serialised on that prover — use plk_prover_create for
 * proofs in parallel. */
typedef struct plk_prover plk_prover;
int plk_prover_create(plk_key* key, plk_prover** out);
int plk_prover_destroy(plk_prover* p);
/* The prover's stream (hipStream_t). */
int plk_prover_stream(plk_prover* p, void** stream_out);
/* Prover::create_proof (prover.rs:67-474) on this prover; arguments as plk_prove. */
int plk_prover_prove(plk_prover* p, const plk_composer* circuit, uint64_t seed, plk_proof* proof,
                     plk_fr* public_inputs, size_t pi_cap, size_t* pi_count);
/* k_accumulate statistics of this prover's MSMs (see plk_srs_cum_msm_stats); reset != 0
 * clears the cumulative figures after reading them. Any output may be NULL. */
int plk_prover_msm_stats(plk_prover* p, int reset, double* accumulate_ms, uint64_t* launches,
                         uint64_t* point_adds, uint64_t* points);
/* The four wire commits (a, b, o, d) of this prover's last proof: basis[c] = 1 when wire c was
 * committed from its Lagrange values on the key's Lagrange-basis SRS, 0 from its coefficients
 * (no Lagrange SRS, a sharded prover, or a wire whose values crowd one MSM bucket);
 * entries[c] = the MSM entries (point additions) of that commit, 0 for a sharded prover.
 * Either output may be NULL. */
int plk_prover_commit_info(const plk_prover* p, int basis[4], uint64_t entries[4]);

/* ---- circuit check: which gates a witness fails -------------------------------------------
 * Every gate identity of the quotient's numerator evaluated on its own at the gate (not folded
 * with separation challenges): the job of a mock prover. The permutation terms are left out:
 * wires are witness indices, so copy constraints hold by construction. A circuit passes exactly
 * when no bit is set on any gate, which is when plk_prove succeeds (up to the negligible chance
 * that a random challenge cancels a non-zero term). The next row of gate i is gate i + 1, of the
 * last gate the all-zero row. Mask bits of a gate (a bit is set when the term is non-zero):
 *   PLK_GATE_ARITH       q_arith (q_m a b + q_l a + q_r b + q_o o + q_4 d + q_c) + PI, always
 *                        evaluated; its value is the reported residual
 *   PLK_GATE_RANGE(j)    j < 4, q_range != 0:  delta(o - 4d), delta(b - 4o), delta(a - 4b),
 *                        delta(d' - 4a), delta(f) = f (f - 1)(f - 2)(f - 3)
 *   PLK_GATE_LOGIC(j)    j < 5, q_logic != 0, on the quads qa = a' - 4a, qb = b' - 4b,
 *                        qd = d' - 4d and w = o: delta(qa), delta(qb), delta(qd), w - qa qb, and
 *                        the xor / and identity selected by q_c
 *   PLK_GATE_FIXED(j)    j < 4, q_fixed_group_add != 0, bit = d' - 2d: bit (bit - 1)(bit + 1),
 *                        bit q_c - o, the x check, the y check
 *   PLK_GATE_VAR(j)      j < 3, q_variable_group_add != 0: x1 y2 - d', the x3 check, the y3 check */
#define PLK_GATE_ARITH 0x1u
#define PLK_GATE_RANGE(j) (1u << (4 + (j)))
#define PLK_GATE_LOGIC(j) (1u << (8 + (j)))
#define PLK_GATE_FIXED(j) (1u << (16 + (j)))
#define PLK_GATE_VAR(j) (1u << (20 + (j)))
typedef struct { uint64_t gate; uint32_t mask; uint32_t _pad; plk_fr residual; } plk_gate_failure;
/* by_class: gates failing a term of the arithmetic, range, logic, fixed-base, variable-base class */
typedef struct { uint64_t gates, failing, by_class[5]; } plk_check_summary;
/* A failing circuit is a verdict, not an error: all three return PLK_OK, summary->failing counts
 * the failing gates, failures[0 .. min(cap, failing)) are the failing gates with the smallest
 * indices in ascending order and *count (nullable) their number; cap = 0 with failures = NULL is
 * a count-only call. PLK_E_ARG only for a NULL summary / circuit / p / key (and, for the two
 * diagnoses, when there is no witness to check).
 *
 * plk_composer_check needs no key: the witness and the composer's compact gate records are
 * uploaded and one kernel (k_gate_check) checks a gate per lane; a satisfied circuit reads back
 * the summary alone. ctx = NULL evaluates the same per-gate function in a host loop, no GPU. */
int plk_composer_check(plk_ctx* ctx, const plk_composer* circuit, plk_check_summary* summary,
                       plk_gate_failure* failures, size_t cap, size_t* count);
/* The same check of the witness and public inputs of this prover's most recent plk_prover_prove,
 * whether it succeeded or failed with PLK_E_DEGREE: the witness is still on the device, so it
 * costs one kernel on the prover's stream and no upload, against the gate table the key keeps.
 * PLK_E_ARG when no witness has been uploaded yet (a plk_prover_prove refused with PLK_E_ARG
 * counts as none). The prover is not disturbed: its next proof is what a fresh prover's would
 * be. plk_key_diagnose is the same on the prover behind plk_prove. */
int plk_prover_diagnose(plk_prover* p, plk_check_summary* summary,
                        plk_gate_failure* failures, size_t cap, size_t* count);
int plk_key_diagnose(plk_key* key, plk_check_summary* summary,
                     plk_gate_failure* failures, size_t cap, size_t* count);
/* HIP-event milliseconds of k_gate_check in the most recent plk_composer_check on this context
 * or diagnosis of a key of this context (measurement only). */
int plk_check_last_ms(plk_ctx* ctx, float* kernel_ms);

/* ---- sharded commits: one proof, its MSMs split over the GPUs of a node ------------------
 * BASELINE configs[4] / SURVEY §8e. One process (rank) per GPU proves the SAME circuit with
 * the same seed; every rank runs the NTT / elementwise rounds on its own GPU (replicas, they
 * are a minority of the proof) and each commit — the 4 wire commits (prover.rs:133-136),
 * z (:194), the 4 quotient chunks (:262-265) and the 2 openings (:440,452) — is split by
 * SRS index: rank r runs the Pippenger over its slice [slice_start, slice_start +
 * slice_len) of every polynomial against `slice` (plk_srs_setup_range on the same tau), then
 * the ranks exchange their partial points (13 words + a status word per commit) with ONE
 * all-gather per commit group and each folds them on the host (plk_g1_sum order: rank 0
 * first). Proofs are byte-identical to the unsharded plk_prove on any rank.
 * The all-gather is the caller's (RCCL over xGMI under torch.distributed in
 * dusk-plonk_amd/parallel.py): `allgather(user, send, bytes, recv)` must place every rank's
 * `bytes` of `send` at recv + rank * bytes and return 0 (non-zero: PLK_E_DEVICE). Slices
 * must tile [0, N) in rank order with N >= the key's trimmed SRS; every rank calls
 * plk_prover_prove for every proof, in the same order (the exchange is a collective).
 * world = 1 with a slice and an all-gather runs the same exchange path with one rank (the
 * sharded code path on one GPU); world = 1 with slice = allgather = NULL is unsharded. */
typedef int (*plk_allgather_fn)(void* user, const void* send, size_t bytes, void* recv);
int plk_prover_shard(plk_prover* p, plk_srs* slice, uint64_t slice_start, int rank, int world,
                     plk_allgather_fn allgather, void* user);
/* The same sharded proof with each commit split by BUCKET RANGE instead of SRS slice (round 6;
 * the north star's "partial bucket sums"): every rank keeps the key's whole SRS and window
 * table and runs every commit of the group over all of its points, sorting, accumulating and
 * reducing only bucket range `rank` of `world` (plk_commit_batch_dev_part's split, so each rank
 * also does 1/world of the bucket reduction, which the slice split repeats on every rank); the
 * shares go through the same all-gather and fold, so proofs are byte-identical. PLK_E_ARG
 * unless `world` is a power of two and the key's SRS has a wide bucket set with >= 2^14
 * buckets per part (c >= 17: SRS >= 2^16 points; c = 20 from 2^20 points: world <= 32) — the
 * caller then keeps plk_prover_shard's slices. Undone by plk_prover_shard. */
int plk_prover_shard_buckets(plk_prover* p, int rank, int world, plk_allgather_fn allgather,
                             void* user);

/* ---- verifier: Verifier::new, Verifier::verify ------------------------------------------
 * plk_verifier_fold returns the two G1 points of the final KZG check; all proofs of the batch
 * are valid  <=>  e(c, H) == e(w, [tau]H)  (up to the soundness error of the random weights,
 * 2^-128). The pairing check itself is plk_pairing_check / plk_pairing_check_batch against a
 * plk_opening_key (H, [tau]H), and plk_verifier_verify / plk_verifier_verify_each below give the
 * verdicts: the fold stays available for callers with a pairing library of their own.
 * Points are checked to be on the curve (identity commitments are legal: selector commitments
 * of unused widgets, w_z_chall_w_comm of trivial circuits). Subgroup membership is NOT checked
 * here: as in the reference (proof.rs:77, Proof holds decoded G1Affine values) it is the duty
 * of whoever decoded the proof bytes into points. The ingest stage below is that decoder:
 * plk_proofs_ingest / plk_proof_decode_compact check it for compact proofs,
 * plk_g1_subgroup_check_batch for points that arrived through the SCALE route, and
 * plk_verifier_verify_each_bytes runs ingest and the verdicts in one call. */
typedef struct plk_verifier plk_verifier;
typedef struct { plk_g1 c, w; } plk_kzg_pair;

/* Verifier::new (verifier.rs:25-43). Host only, needs no GPU. n: the padded domain size (a
 * power of two, 2 <= n <= 2^27), m: the gate count the transcript is seeded with,
 * commitments: the 15 key commitments in plk_key_info order, pi_indexes: pi_count strictly
 * increasing gate indexes < n (NULL when pi_count = 0). */
int plk_verifier_create(const char* label, uint64_t n, uint64_t m, const plk_g1 commitments[15],
                        const uint64_t* pi_indexes, size_t pi_count, plk_verifier** out);
int plk_verifier_destroy(plk_verifier* v);

/* The transcript replay of Proof::verify (proof.rs:87-178, 213-295, 344-376) for one proof.
 * Host only. out[0..10] = beta, gamma, alpha, range / logic / fixed / variable separation, z,
 * v (aggregate), v (shifted), u (batch). public_inputs: the verifier's pi_count values.
 * PLK_E_ARG: a non-canonical evaluation or public input, z_h(z) = 0 or z = 1 (the reference
 * panics there). Points are compressed as given (x and the sign of y), not curve-checked. */
int plk_verifier_challenges(const plk_verifier* v, const plk_proof* proof, const plk_fr* public_inputs,
                            plk_fr out[11]);

/* Everything of Verifier::verify (verifier.rs:46-81) up to the pairing, for `count` proofs of
 * this verifier's circuit: out = (sum_j rho_j C_j, sum_j rho_j W_j), where (C_j, W_j) is
 * exactly batch_check's pair (commitment_scheme.rs:24-66) for proof j. public_inputs holds
 * count * pi_count values. weights: `count` canonical scalars, or NULL. On NULL: rho_0 = 1 and
 * rho_j = 128-bit values drawn from a merlin transcript over every proof's u challenge plus
 * 32 bytes of OS entropy. The NULL form is the sound one; explicit weights exist for tests and
 * for callers with their own Fiat-Shamir. The transcripts are replayed on the host (up to 16
 * threads), every proof's scalars are derived and both sums run on the GPU as one
 * plk_msm_points_ranges batch over 16 + 11 count and 2 count points.
 * PLK_E_ARG: count = 0, a non-canonical evaluation / public input / weight, a finite point off
 * the curve, z_h(z) = 0 or z = 1. One call at a time per context. */
int plk_verifier_fold(plk_ctx* ctx, plk_verifier* v, const plk_proof* proofs,
                      const plk_fr* public_inputs, size_t count, const plk_fr* weights,
                      plk_kzg_pair* out);
/* Timing of the most recent plk_verifier_fold on this verifier (measurement only): host
 * milliseconds of the transcript replays (and the weights), and milliseconds between two HIP
 * events on the context's stream, one before the upload of the points and one after the MSM
 * has returned: the scalar kernels, the MSM's kernels and its host Horner tail. */
int plk_verifier_last_fold_stats(const plk_verifier* v, double* replay_ms, float* gpu_ms);

/* Where plk_verifier_fold replays the transcripts. PLK_REPLAY_HOST (the default): on up to 16
 * host threads, as described above. PLK_REPLAY_DEVICE: on the GPU, one proof per lane
 * (csrc/verifier_replay.hip); the host keeps the canonical-form checks, the uploads and, for
 * weights = NULL, one sequential hash. With explicit weights the pair is byte-identical in both
 * modes. z_h(z) = 0 and z = 1 are detected on the device and refused with PLK_E_ARG all the same.
 * Device mode refuses verifiers with more than 2^16 public inputs (PLK_E_ARG): its compiled
 * schedule grows with them.
 * weights = NULL in device mode draws the weights differently (same soundness in the random-
 * oracle model: independent 128-bit values bound to every proof's u and unknown to whoever
 * chose the proofs): the host hashes root = Transcript("plk-verifier-fold"), append_u64("count",
 * count), append_scalar("u", u_j) for every j, append_message("entropy", 32 OS bytes); rho_0 = 1
 * and rho_j = the 128-bit little-endian value of challenge_bytes("rho", 16) taken from a clone
 * of root after append_u64("index", j), one lane per proof. Host mode squeezes count - 1 times
 * from one transcript instead.
 * In device mode plk_verifier_last_fold_stats reports as replay_ms the host time before and
 * inside the GPU phase (canonical checks, the weights root), and gpu_ms also spans the replay
 * kernels. Host only; PLK_E_ARG on another mode. */
#define PLK_REPLAY_HOST 0
#define PLK_REPLAY_DEVICE 1
int plk_verifier_set_replay(plk_verifier* v, int mode);
/* The device replay alone, whatever the verifier's mode: out[11 j .. 11 j + 10] = the challenges
 * of proof j in plk_verifier_challenges order. public_inputs: count * pi_count values.
 * PLK_E_ARG: as plk_verifier_challenges, count = 0, or more than 2^16 public inputs. */
int plk_verifier_challenges_batch(plk_ctx* ctx, plk_verifier* v, const plk_proof* proofs,
                                  const plk_fr* public_inputs, size_t count, plk_fr* out);
/* Milliseconds between two HIP events around the replay kernels of the most recent device-mode
 * plk_verifier_fold or plk_verifier_challenges_batch; 0 after a host-mode fold. */
int plk_verifier_last_replay_ms(const plk_verifier* v, float* kernel_ms);

/* ---- opening key and pairing check: the G2 half of EvaluationKey, TatePairing ---------------
 * plk_g2 is a G2 point on the twist y^2 = x^3 + 4 (1 + u) over Fp2 = Fp[u] / (u^2 + 1): x.c0,
 * x.c1, y.c0, y.c1 as 6 LE u64 Montgomery Fp limbs each, then the infinity flag. ASSUMED
 * (parity unpinned, like the SCALE codec below): the field order of zkcrypto's G2Affine; the
 * reference's pairing crate is not vendored and no fixture of it holds a G2 point.
 * An opening key holds H and beta_h = [tau]H and, prepared once on the host, the 68 line
 * coefficients per point that the Miller loop consumes (csrc/pairing.hpp); no G2 arithmetic
 * runs on the GPU. The prepared lines are uploaded to a context's device on first device use;
 * a key serves one device. */
typedef struct { uint64_t x[12]; uint64_t y[12]; uint64_t infinity; } plk_g2; /* 200 bytes */
typedef struct plk_opening_key plk_opening_key;
/* H = the standard G2 generator, beta_h = [tau]H (tau: canonical Montgomery Fr, not zero). Host
 * only: the counterpart of plk_srs_setup's explicit trapdoor. */
int plk_opening_key_setup(const plk_fr* tau, plk_opening_key** out);
/* An existing key. PLK_E_ARG for either point: a limb >= p, a point off the twist, a point not
 * of order r (one host scalar multiplication each), the point at infinity. */
int plk_opening_key_load(const plk_g2* h, const plk_g2* beta_h, plk_opening_key** out);
int plk_opening_key_points(const plk_opening_key* key, plk_g2* h, plk_g2* beta_h);
int plk_opening_key_destroy(plk_opening_key* key);

/* *ok = 1 iff e(pair.c, H) == e(pair.w, beta_h): ML(c, H) ML(-w, beta_h) final-exponentiates
 * to 1 (one shared Miller loop, as the reference's multi_miller_loop). Host only, needs no GPU.
 * Finite points must be canonical and on the curve (PLK_E_ARG otherwise, as in plk_msm_points);
 * subgroup membership is not checked (plk_verifier_fold's contract; plk_g1_subgroup_check_batch
 * is the screen). A point at infinity
 * contributes the factor 1: (inf, inf) is accepted, (finite, inf) and (inf, finite) rejected. */
int plk_pairing_check(const plk_opening_key* key, const plk_kzg_pair* pair, int* ok);
/* The same check for `count` pairs on the GPU, one pair per lane (csrc/pairing.hip): ok[j] =
 * 0 / 1. Host buffers; one malformed point makes the whole call PLK_E_ARG. One call at a time
 * per context and per key. */
int plk_pairing_check_batch(plk_ctx* ctx, plk_opening_key* key, const plk_kzg_pair* pairs,
                            size_t count, uint8_t* ok);
/* Milliseconds of the pairing kernel of the most recent device check on this key (HIP events
 * around the kernel; measurement only). */
int plk_opening_key_last_pairing_ms(const plk_opening_key* key, float* kernel_ms);

/* (C_j, W_j) of every proof: out[j] is exactly plk_verifier_fold(count = 1, weight 1) of proof
 * j, bit for bit, for `count` proofs in one GPU pass (csrc/verifier.hip k_proof_pairs: half a
 * wave per proof, one point and scalar per lane). Both replay modes feed it. PLK_E_ARG as the
 * fold: one malformed proof refuses the whole call. One call at a time per context. */
int plk_verifier_pairs(plk_ctx* ctx, plk_verifier* v, const plk_proof* proofs,
                       const plk_fr* public_inputs, size_t count, plk_kzg_pair* out);
/* Verifier::verify (verifier.rs:46-81) to its end, for a batch: plk_verifier_fold (weights =
 * NULL: the sound random weights; or explicit) plus one host plk_pairing_check. *ok = 1: every
 * proof of the batch is valid; 0: the reference's Err(PairingCheckFailure). Malformed input
 * (whatever the fold refuses) is PLK_E_ARG, not a verdict. */
int plk_verifier_verify(plk_ctx* ctx, plk_verifier* v, const plk_opening_key* key,
                        const plk_proof* proofs, const plk_fr* public_inputs, size_t count,
                        const plk_fr* weights, int* ok);
/* One verdict per proof on the GPU: plk_verifier_pairs, then the batched pairing kernel on the
 * pairs where they lie (no host round trip): ok[j] = 0 / 1. A malformed proof anywhere in the
 * batch makes the whole call PLK_E_ARG and leaves ok untouched — it never hides as ok = 0 and
 * never lets the other verdicts pass silently; decode and screen proofs first
 * (plk_proof_decode, or the batched plk_proofs_ingest) when single malformed ones must be told
 * apart; plk_verifier_verify_each_bytes does both and gives one verdict per proof. */
int plk_verifier_verify_each(plk_ctx* ctx, plk_verifier* v, plk_opening_key* key,
                             const plk_proof* proofs, const plk_fr* public_inputs, size_t count,
                             uint8_t* ok);
/* Milliseconds of the two GPU phases of the most recent plk_verifier_pairs /
 * plk_verifier_verify_each on this verifier (HIP events around each kernel): the per-proof pairs
 * kernel and, for verify_each, the pairing kernel (0 after plk_verifier_pairs). */
int plk_verifier_last_each_stats(const plk_verifier* v, float* pairs_ms, float* pairing_ms);

/* ---- Proof wire format (SCALE, src/prover/proof.rs:11,36) ---------------------------------
 * The reference derives parity-scale-codec Encode/Decode for Proof: fields in declaration
 * order, 11 Commitment<G1Affine> then ProofEvaluations. The element encodings live in the
 * un-vendored bls-12-381 / zksnarks crates; ASSUMED here (parity unpinned): G1Affine as its
 * fields x, y (Fq = [u64; 6] Montgomery limbs, LE) and is_infinity (bool, 1 byte) = 97 B;
 * Fr as [u64; 4] Montgomery limbs, LE = 32 B; ProofEvaluations in plk_proof order. Total
 * PLK_PROOF_SCALE_BYTES. Decode rejects (PLK_E_ARG) a wrong length, a non-boolean flag,
 * limbs >= the modulus, and finite points not on y^2 = x^3 + 4. The identity (ASSUMED
 * encoding) is written as x = 0, y = 0, is_infinity = 1; decode takes is_infinity = 1 with
 * (x, y) = (0, 0) or zkcrypto's (0, one) as the identity and returns it as (0, 0, 1); other
 * coordinates under the flag are rejected. DELIBERATE DIVERGENCE (parity unpinned): a
 * derived SCALE Decode plus zkcrypto's flag-only is_identity would accept ANY (x, y) under
 * is_infinity = 1 as the identity; this decoder is strict so that one proof has one byte
 * string (a verifier hashing proof bytes sees no malleable identity encodings). No fixture
 * in the reference covers either behaviour. */
#define PLK_PROOF_SCALE_BYTES (11 * 97 + 16 * 32)
int plk_proof_encode(const plk_proof* proof, uint8_t* out, size_t cap, size_t* len);
int plk_proof_decode(const uint8_t* in, size_t len, plk_proof* proof);

/* ---- Compact proofs and the ingest stage (csrc/ingest.hip) -------------------------------
 * The compact form of a proof, the shape of upstream dusk-plonk's Proof::to_bytes: the 11
 * commitments in plk_proof order as zkcrypto's 48-byte compressed G1, then the 16 evaluations as
 * 32 canonical little-endian bytes each (NOT Montgomery), PLK_PROOF_COMPACT_BYTES in all. ASSUMED,
 * parity unpinned, as the SCALE codec above: the element crates are not vendored. A point is
 * exactly what the transcript hashes (csrc/transcript.hpp g1_compress): x big-endian, and in byte
 * 0 bit 7 = compressed (always set), bit 6 = infinity, bit 5 = y is the larger root (y > (p-1)/2);
 * infinity is 0xc0 and 47 zero bytes. A scalar is what the transcript's append_scalar writes.
 * Decoding is strict, so that one proof has one byte string. It rejects: bit 7 clear; the
 * infinity bit with any other bit or byte set; x >= p; x^3 + 4 not a square; a scalar >= r; and,
 * with check_subgroup != 0, a curve point outside G1 (not of order r). Reading a point back costs
 * one Fp square root, y = (x^3 + 4)^((p+1)/4), and the subgroup check two multiplications by
 * x0 = 0xd201000000010000 (the endomorphism test of Scott, eprint 2021/1130 section 6, what
 * zkcrypto's is_torsion_free does): P in G1  <=>  (beta x, y) == -[x0^2]P. */
#define PLK_PROOF_COMPACT_BYTES (11 * 48 + 16 * 32)
/* Host only. out = NULL: a size query. PLK_E_ARG: cap too small, a non-canonical field. */
int plk_proof_encode_compact(const plk_proof* proof, uint8_t* out, size_t cap, size_t* len);
/* Host only, one proof: the single-proof path, and the independent check of the kernels below.
 * PLK_E_ARG for a wrong length and for every rejection listed above; *out is then untouched. */
int plk_proof_decode_compact(const uint8_t* in, size_t len, plk_proof* out, int check_subgroup);

/* Per-item status of the batched calls, one byte each; the first failure wins (for a point in
 * the order of the list; for a proof over its 27 fields in order). */
#define PLK_INGEST_OK 0
#define PLK_INGEST_ENCODING 1   /* flag bits / infinity form */
#define PLK_INGEST_RANGE 2      /* x >= p or a scalar >= r */
#define PLK_INGEST_OFF_CURVE 3  /* x^3 + 4 has no square root */
#define PLK_INGEST_SUBGROUP 4   /* on the curve, not of order r */

/* The batched calls below run on the GPU, one point per lane. Host buffers. The content of the
 * bytes never makes them fail: only a NULL pointer or a zero count is PLK_E_ARG (and
 * plk_g1_subgroup_check_batch's malformed points, see there). One call at a time per context. */
/* n compressed points (48 n bytes) -> out[i] (canonical; all zero bytes when status[i] != 0) and
 * status[i]. check_subgroup = 0 skips the membership test. */
int plk_g1_decompress_batch(plk_ctx* ctx, const uint8_t* in48, size_t n, int check_subgroup,
                            plk_g1* out, uint8_t* status);
/* ok[i] = 1 iff points[i] is in G1 (the identity is), for points already in ABI form, e.g. of
 * proofs that arrived through the SCALE route. PLK_E_ARG for a non-canonical or off-curve finite
 * point or an infinity word other than 0 / 1, as plk_msm_points. */
int plk_g1_subgroup_check_batch(plk_ctx* ctx, const plk_g1* points, size_t n, uint8_t* ok);
/* `count` compact proofs (count * PLK_PROOF_COMPACT_BYTES bytes) -> out[j], status[j]. An accepted
 * proof is byte for byte what plk_proof_decode_compact gives. out[j] of a rejected proof is all
 * zero bytes: finite points off the curve, which plk_verifier_fold refuses should it ever be
 * passed on by mistake. */
int plk_proofs_ingest(plk_ctx* ctx, const uint8_t* in, size_t count, int check_subgroup,
                      plk_proof* out, uint8_t* status);
/* Milliseconds of the two kernels of the most recent batched call above on this context (HIP
 * events around each; measurement only). subgroup_ms is 0 when that kernel did not run. */
int plk_ingest_last_ms(plk_ctx* ctx, float* decompress_ms, float* subgroup_ms);
/* plk_proofs_ingest, then plk_verifier_verify_each on the accepted proofs and their public
 * inputs (compacted through host memory), verdicts scattered back: verdict[j] = 1 valid, 0
 * well-formed but the pairing check fails, 0x10 | status when ingest rejected proof j.
 * public_inputs holds count * pi_count values, those of rejected proofs are skipped. When every
 * proof is rejected, plk_verifier_verify_each is not called. Both replay modes work. What
 * plk_verifier_verify_each still refuses in a well-formed proof (a non-canonical public input,
 * z_h(z) = 0) is PLK_E_ARG for the call, as there. */
int plk_verifier_verify_each_bytes(plk_ctx* ctx, plk_verifier* v, plk_opening_key* key,
                                   const uint8_t* in, const plk_fr* public_inputs, size_t count,
                                   int check_subgroup, uint8_t* verdict);

/* ---- An SRS from bytes, and its verification (csrc/srs_io.hip) ---------------------------
 * A ceremony's SRS comes as bare arrays of points in zkcrypto's byte forms. ASSUMED, parity
 * unpinned, as the compact proof above: the element crates are not vendored.
 *  - PLK_G1_COMPRESSED, 48 B: exactly the form of plk_g1_decompress_batch (and of the compact
 *    proof's commitments), with its strict rules.
 *  - PLK_G1_UNCOMPRESSED, 96 B: x big-endian then y big-endian; in byte 0 bit 7 = 0 (not
 *    compressed), bit 6 = infinity, bit 5 = 0. Infinity is 0x40 and 95 zero bytes. Decoding is
 *    strict: bit 7 or bit 5 set, or any other bit or byte under the infinity bit, is
 *    PLK_INGEST_ENCODING; x >= p or y >= p PLK_INGEST_RANGE; y^2 != x^3 + 4 PLK_INGEST_OFF_CURVE.
 *  - G2 (the opening key): compressed 96 B = x.c1 big-endian then x.c0, the G1 flag bits in byte
 *    0, the sort bit set when y is the lexicographically larger of +-y (y.c1 > (p-1)/2, or y.c1 =
 *    0 and y.c0 > (p-1)/2); uncompressed 192 B = x.c1, x.c0, y.c1, y.c0. */
#define PLK_G1_COMPRESSED 0
#define PLK_G1_UNCOMPRESSED 1
/* n_points points in `format` (48 n / 96 n bytes, a host buffer) -> an SRS, as plk_srs_load gives
 * for the same points. The bytes are uploaded and decoded on the GPU, one point per lane,
 * straight into the SRS's device arrays; with check_subgroup != 0 every point is also tested for
 * order r. Infinity encodings are accepted (a Lagrange-basis SRS holds them legitimately). One
 * rejected point makes the call PLK_E_ARG with *out = NULL and no table built; *bad_index
 * (nullable) is then the smallest rejected index and *bad_status (nullable) its PLK_INGEST_*
 * code, found by a reduction on the device. The SRS remembers that its points are canonical and
 * on the curve and whether they passed the subgroup test (plk_srs_verify skips what is known). */
int plk_srs_load_bytes(plk_ctx* ctx, const uint8_t* in, size_t n_points, int format,
                       int check_subgroup, plk_srs** out, uint64_t* bad_index, uint8_t* bad_status);
/* Points [start, start + count) in `format` (48 / 96 bytes each), encoded on the GPU: out of
 * Montgomery form, big-endian, the sort bit from y > (p-1)/2. A compressed export followed by
 * plk_srs_load_bytes reproduces plk_srs_points bit for bit. PLK_E_ARG for a range outside the SRS
 * or an unknown format. */
int plk_srs_export_bytes(const plk_srs* srs, size_t start, size_t count, int format, uint8_t* out);
/* Milliseconds of the decode and subgroup kernels of the most recent plk_srs_load_bytes on this
 * context (HIP events around each; measurement only; 0 for a kernel that did not run). */
int plk_srs_last_load_ms(plk_ctx* ctx, float* decode_ms, float* subgroup_ms);

/* The structure check's fold. With weights rho_i, i < n - 1 (rho_0 = 1, the others independent
 * 128-bit values):  out.c = sum rho_i g1[i+1],  out.w = sum rho_i g1[i].  On points of order r,
 * g1[i+1] = tau g1[i] for every i  <=>  e(c, H) = e(w, [tau]H), except with probability 2^-128
 * over the weights. The weights are derived on the device, one lane per index, from
 * one merlin root over a domain label, n and the seed: rho_i = challenge_bytes("rho", 16) of a
 * clone after append_u64("index", i), the pattern of the verifier's fold. seed = NULL takes 32
 * bytes from getrandom and is the sound form; an explicit seed is for tests. Both sums run as one
 * batch of two MSMs on the SRS's own table. n = 1 gives (inf, inf), which plk_pairing_check
 * accepts. One call at a time per SRS. */
int plk_srs_fold(plk_srs* srs, const uint8_t seed[32], plk_kzg_pair* out);
#define PLK_SRS_OK 0
#define PLK_SRS_POINT 1     /* non-canonical limb or off the curve (an SRS from plk_srs_load) */
#define PLK_SRS_SUBGROUP 2  /* a point not of order r */
#define PLK_SRS_INFINITY 3  /* a power of tau is never the identity */
#define PLK_SRS_GENERATOR 4 /* g1[0] is not the standard generator */
#define PLK_SRS_CHAIN 5     /* the pairing check of the fold fails */
/* Is this SRS ([tau^i]G)_i for the tau of `key`? In order: the canonical / on-curve pass over the
 * device points (skipped for an SRS from plk_srs_load_bytes), the subgroup kernel (skipped when
 * already passed), the infinity scan, g1[0] == G, plk_srs_fold, one host plk_pairing_check.
 * *verdict is the first failing class or PLK_SRS_OK; *bad_index (nullable) the smallest offending
 * index for PLK_SRS_POINT / _SUBGROUP / _INFINITY, untouched otherwise. Without the generator
 * test a uniformly scaled SRS would pass. A bad SRS is a verdict, not an error: only NULL
 * pointers or an SRS of another context are PLK_E_ARG. seed as in plk_srs_fold. */
int plk_srs_verify(plk_ctx* ctx, plk_srs* srs, const plk_opening_key* key, const uint8_t seed[32],
                   int* verdict, uint64_t* bad_index);
/* Milliseconds of the most recent plk_srs_verify on this SRS that reached the fold: the fold
 * (weights and both MSMs, host wall time) and the host pairing check (measurement only). */
int plk_srs_last_verify_ms(const plk_srs* srs, double* fold_ms, double* pairing_ms);

/* The opening key in zkcrypto's G2 byte forms (above): `format` PLK_G1_COMPRESSED = 96 bytes per
 * point, PLK_G1_UNCOMPRESSED = 192. Host only. Decoding is strict and mirrors the G1 rules (flag
 * bits, every coefficient < p, x^3 + 4 (1 + u) a square in Fp2 / the twist equation); then every
 * check of plk_opening_key_load applies: order r, not infinity. PLK_E_ARG otherwise. */
int plk_opening_key_load_bytes(const uint8_t* h, const uint8_t* beta_h, int format,
                               plk_opening_key** out);
int plk_opening_key_to_bytes(const plk_opening_key* key, int format, uint8_t* h, uint8_t* beta_h);

/* ---- Updating an SRS (csrc/g1_mul.hip, csrc/srs_io.hip) ------------------------------------
 * PLONK's reference string is updatable: anyone may multiply a fresh secret s into it, g1'[i] =
 * [s^i] g1[i] and beta_h' = [s] beta_h, and the result is sound if one contributor was honest. The
 * contributor publishes the witness [s]H (the shape of the Ethereum KZG ceremony's pot_pubkey),
 * from which anyone can check that the new string is the old one times the witness's secret.
 *
 * The primitive under it is a batched variable-base scalar multiplication, one point and one
 * scalar per lane: the scalar is split on the device into two positive 128-bit halves by the
 * endomorphism of the subgroup test, and one chain of 128 doublings and at most 128
 * mixed additions runs on the redundant-limb field. The split is only valid on G1. */
/* out[i] = [scalars[i]] points[i], canonical affine; host buffers, one call at a time per context;
 * n = 0 is PLK_OK. Scalars are Montgomery Fr, a scalar >= r is PLK_E_ARG. Points follow the rules
 * of plk_msm_points: a non-canonical or off-curve finite point or an infinity word other than
 * 0 / 1 is PLK_E_ARG. assume_subgroup = 0 runs the subgroup kernel first
 * (plk_g1_subgroup_check_batch) and refuses a non-member with PLK_E_ARG; assume_subgroup = 1: the
 * caller vouches for membership (for a point outside G1 the result is then unspecified). Identity
 * inputs and zero scalars are legal and give the identity (x = y = 0, infinity = 1). */
int plk_g1_mul_batch(plk_ctx* ctx, const plk_g1* points, const plk_fr* scalars, size_t n,
                     int assume_subgroup, plk_g1* out);
/* HIP events around the multiplication kernel of the last plk_g1_mul_batch or plk_srs_update on
 * this context (milliseconds; measurement only). */
int plk_g1_mul_last_ms(plk_ctx* ctx, float* kernel_ms);
/* Host only. A new key with the same H and beta_h' = [s] beta_h; *witness = [s]H. s = 0 or s >= r
 * (Montgomery form) is PLK_E_ARG. */
int plk_opening_key_update(const plk_opening_key* key, const plk_fr* s, plk_opening_key** out,
                           plk_g2* witness);
/* A NEW SRS on the context of `srs` with g1'[0] = G and g1'[i] = [s^i] g1[i], MSM-ready as one from
 * plk_srs_load, with the updated opening key and the witness; the input SRS and key are untouched.
 * The powers s^i are formed on the device. s = NULL draws 64 bytes from getrandom, reduces them
 * mod r and redraws on 0: the form meant for use, the secret never leaves the library. The secret
 * and what is derived from it are wiped on a BEST EFFORT basis before the call returns: the host
 * copies with explicit_bzero, the device array of powers with hipMemsetAsync before it is freed;
 * registers, kernel arguments and the allocator's pages are beyond the library's reach. An
 * explicit s is for tests and callers with their own entropy. The new SRS is known to be
 * canonical, on the curve and in G1 (its plk_srs_verify skips those passes). When the input SRS
 * is not known to be in G1 (one from plk_srs_load or plk_srs_setup), the canonical / on-curve pass
 * and the subgroup kernel run first: a bad point is PLK_E_ARG with *out_srs = NULL and *bad_index
 * (nullable) the smallest offending index, as plk_srs_load_bytes. PLK_E_ARG also for fewer than 2
 * points, s = 0 and s >= r. One call at a time per context. */
int plk_srs_update(plk_srs* srs, const plk_opening_key* key, const plk_fr* s, plk_srs** out_srs,
                   plk_opening_key** out_key, plk_g2* witness, uint64_t* bad_index);
#define PLK_SRS_WITNESS 6 /* the witness is malformed, outside the r-torsion or the identity */
#define PLK_SRS_LINK 7    /* e(new g1[1], H) != e(prev g1[1], witness), or a bad prev g1[1] */
/* Is new_srs with new_key a well-formed SRS whose tau is (the previous string's tau) * s for the s
 * behind `witness`? prev_tau_g1 is g1[1] of the string that was updated. In order: the witness is
 * canonical, on the twist, of order r and not the identity (else PLK_SRS_WITNESS); every class of
 * plk_srs_verify(new_srs, new_key, seed) with its verdicts and *bad_index; one host
 * plk_pairing_check of e(new g1[1], H) = e(prev_tau_g1, witness) on the temporary key (H,
 * witness), where a malformed, non-member or identity prev_tau_g1 is PLK_SRS_LINK too. The first
 * failing class wins. A bad update is a verdict, not an error: only NULL pointers, fewer than 2
 * points or an SRS of another context are PLK_E_ARG. */
int plk_srs_verify_update(plk_ctx* ctx, const plk_g1* prev_tau_g1, plk_srs* new_srs,
                          const plk_opening_key* new_key, const plk_g2* witness,
                          const uint8_t seed[32], int* verdict, uint64_t* bad_index);
/* One bare G2 point (a witness) in zkcrypto's byte forms, as the opening key's: 96 bytes
 * compressed, 192 uncompressed. Host only; decoding is strict (the subgroup check is the
 * consumer's: plk_srs_verify_update makes it). */
int plk_g2_to_bytes(const plk_g2* q, int format, uint8_t* out);
int plk_g2_from_bytes(const uint8_t* in, int format, plk_g2* out);

/* ---- KZG openings (csrc/kzg.hip, csrc/g1_ntt.hip) --------------------------------------------
 * The scheme's other operations beside plk_commit (the reference's src/commitment_scheme.rs and
 * docs/notes-KZG10.md: open, check, batch check). The witness of f at z is the commitment to
 * (f(X) - f(z)) / (X - z); the opening (C, z, y, W) holds iff e(C - y g + z W, H) = e(W, [tau]H).
 * Scalars are Montgomery Fr, canonical (a value >= r is PLK_E_ARG); host buffers; one call at a
 * time per SRS. */
/* Opens one polynomial at `count` arbitrary points: values[k] = f(points[k]), witnesses[k] the
 * witness there. The polynomial is uploaded once; per point one evaluation and one Ruffini
 * division on the device, the quotients committed 16 at a time through the SRS's batch MSM.
 * PLK_E_DEGREE when the polynomial (trailing zeros ignored) has more coefficients than the SRS
 * points, as plk_commit. len <= 1 gives the value f_0 (or 0) and the identity. */
int plk_kzg_open(plk_srs* srs, const plk_fr* coeffs, size_t len, const plk_fr* points, size_t count,
                 plk_fr* values, plk_g1* witnesses);
/* Opens one polynomial of len <= n = 2^log_n coefficients at all n points of the domain, entry i
 * for omega^i (omega = plk_domain_info's generator): values[i] = f(omega^i) and witnesses[i],
 * the same points plk_kzg_open returns, from three transforms over G1 and 2n scalar
 * multiplications (Feist-Khovratovich) instead of n divisions and n MSMs. 1 <= log_n <= 20,
 * len > n is PLK_E_ARG, an SRS of fewer than n points PLK_E_DEGREE.
 * The first call per (SRS, log_n) builds a table of 2n affine points, the transform of the
 * reversed SRS prefix: 2n * 97 bytes of device memory (194 MiB at log_n = 20), kept in the SRS
 * and freed with it. Before the first build the first n SRS points pass the canonical / on-curve
 * and subgroup kernels unless the SRS is known to be in G1 (plk_srs_setup, plk_srs_load_bytes
 * with check_subgroup, plk_srs_update, a passed plk_srs_verify): the multiplication's scalar
 * split is valid on G1 only. A bad point is PLK_E_ARG with *bad_index (nullable) the smallest
 * offending index, as plk_srs_load_bytes reports; otherwise *bad_index = UINT64_MAX. */
int plk_kzg_open_domain(plk_srs* srs, uint32_t log_n, const plk_fr* coeffs, size_t len, plk_fr* values,
                        plk_g1* witnesses, uint64_t* bad_index);
/* HIP-event milliseconds of the most recent plk_kzg_open_domain on this context (measurement
 * only): the transforms (Fr and G1), the pointwise multiplication (with its batch inversion),
 * and the table build (0 when the table was cached). Each pointer nullable. */
int plk_kzg_last_open_ms(plk_ctx* ctx, float* transform_ms, float* mul_ms, float* table_ms);
/* Folds `count` openings (commitments[k], points[k], values[k], witnesses[k]) of commitments
 * made on the base point g (g1[0] of the SRS) into one pair with weights rho_k:
 *   C = sum rho_k (C_k - y_k g + z_k W_k),   W = sum rho_k W_k.
 * All the openings hold iff e(C, H) = e(W, [tau]H) (plk_pairing_check), up to 2^-128 for random
 * weights. One plk_msm_points_ranges batch: 2 count + 1 points for C (sum rho_k y_k accumulated
 * on the scalar side) and count for W. weights = NULL: rho_0 = 1 and 128-bit rho_k from a merlin
 * transcript over the count, every z_k and y_k and 32 bytes of OS entropy (the verifier fold's
 * derivation; the sound form). Explicit weights (count of them) serve callers with their own
 * Fiat-Shamir; count = 1 with weight 1 gives (C - y g + z W, W), the opening's own pair, so
 * per-opening verdicts come from plk_pairing_check_batch over such pairs.
 * PLK_E_ARG: count = 0, a non-canonical scalar, a finite point off the curve or not canonical,
 * an infinity word other than 0 / 1. Subgroup membership is the caller's (plk_verifier_fold's
 * contract). One call at a time per context. */
int plk_kzg_fold(plk_ctx* ctx, const plk_g1* g, const plk_g1* commitments, const plk_fr* points,
                 const plk_fr* values, const plk_g1* witnesses, size_t count, const plk_fr* weights,
                 plk_kzg_pair* out);
/* Opens one polynomial of len <= n = 2^log_n coefficients on every coset of l = 2^log_l points of
 * the domain (a KZG multiproof per coset; the second half of Feist-Khovratovich). With r = n / l,
 * coset j < r is omega^j <omega^r>, its vanishing polynomial X^l - omega^(l j), and witnesses[j]
 * (r entries) the commitment to f(X) div (X^l - omega^(l j)). values holds the n entries
 * f(omega^i) in the domain's natural order, as plk_kzg_open_domain returns them: the i-th value
 * of coset j is entry j + r i. The same 2n scalar multiplications as plk_kzg_open_domain, then a
 * column sum over the l residues and G1 transforms of 2r and r points instead of 2n and n.
 * log_l = log_n gives the one witness O; log_l = 0 gives plk_kzg_open_domain's output byte for
 * byte and shares its table. Arguments, refusals, the table per (SRS, log_n, log_l) of 2n affine
 * points, the G1 test of the SRS prefix and *bad_index as plk_kzg_open_domain; log_l > log_n is
 * PLK_E_ARG. plk_kzg_last_open_ms reports the most recent open of either kind. */
int plk_kzg_open_cosets(plk_srs* srs, uint32_t log_n, uint32_t log_l, const plk_fr* coeffs, size_t len,
                        plk_fr* values, plk_g1* witnesses, uint64_t* bad_index);
/* Folds `count` coset openings (commitments[k], shifts[k], the l = 2^log_l values of row k,
 * witnesses[k]) into one pair. Row k holds v_(k,i) = f(z_k w^i), i < l, w the generator of the
 * l-point domain and z_k = shifts[k] any non-zero scalar. With c_k = IDFT_l(row k), the
 * interpolant of opening k is I_k = sum_i c_(k,i) z_k^-i X^i, and the opening holds iff
 * e(C_k - [I_k(tau)]G + z_k^l W_k, H) = e(W_k, [tau^l]H). The fold with weights rho_k is
 *   C = sum rho_k (C_k + z_k^l W_k) - sum_{i<l} P_i g1[i],   W = sum rho_k W_k,
 *   P_i = sum_k rho_k z_k^-i c_(k,i),
 * to be checked with plk_pairing_check against the opening key of tau^l (plk_opening_key_setup
 * (tau^l), or a ceremony's l-th G2 power through plk_opening_key_load), not the key of tau. The
 * inverse transforms of the rows and the reduction to P run on the device, C and W are one
 * plk_msm_points_ranges batch with the first l SRS points as variable-base points. weights = NULL:
 * rho_0 = 1 and 128-bit rho_k from a merlin transcript (label "plk-kzg-fold-cosets") over count,
 * log_l, every shift, every value and 32 bytes of OS entropy. At log_l = 0 with explicit weights
 * the pair is plk_kzg_fold's byte for byte. PLK_E_ARG: count = 0, log_l > 20, a zero shift, a
 * non-canonical scalar, a bad point by plk_kzg_fold's rules, an SRS of fewer than l points. One
 * call at a time per SRS. */
int plk_kzg_fold_cosets(plk_srs* srs, uint32_t log_l, const plk_g1* commitments, const plk_fr* shifts,
                        const plk_fr* values, const plk_g1* witnesses, size_t count,
                        const plk_fr* weights, plk_kzg_pair* out);

/* ---- test support ---------------------------------------------------------------- */
/* `batch` independent transforms of 2^log_n points each, laid out one after the other, through
 * the batched launcher of csrc/g1_ntt.hip (one launch per level over all of them); otherwise as
 * plk_debug_g1_ntt. batch >= 1, batch * 2^log_n <= 2^20. */
int plk_debug_g1_ntt_batch(plk_ctx* ctx, const plk_g1* in, uint32_t log_n, size_t batch, int dir,
                           plk_g1* out);
/* The column sum over G1 of csrc/g1_colsum.hip through the product's own launcher: out[t] =
 * sum_{a < rows} points[a * cols + t], t < cols, as affine ABI points. Points follow
 * plk_msm_points' rules (PLK_E_ARG otherwise); they need not lie in G1. rows, cols >= 1,
 * rows * cols <= 2^21. */
int plk_debug_g1_colsum(plk_ctx* ctx, const plk_g1* points, size_t rows, size_t cols, plk_g1* out);
/* The transform over G1 of csrc/g1_ntt.hip through the product's own launcher: out_i = sum_j
 * omega^(dir ij) in_j over the 2^log_n domain (log_n <= 20), natural order, dir = +1 / -1, the
 * inverse with n^-1. Points follow plk_msm_points' rules (PLK_E_ARG otherwise); they need not
 * lie in G1. */
int plk_debug_g1_ntt(plk_ctx* ctx, const plk_g1* in, uint32_t log_n, int dir, plk_g1* out);
/* The scalar split of csrc/g1_mul.hip: out[4 i .. 4 i + 3] = a_lo, a_hi, b_lo, b_hi of scalar i
 * (canonical Montgomery; otherwise PLK_E_ARG) with a = z - (k mod z), b = floor(k / z) + 1.
 * ctx = NULL: the host mirror; otherwise the device function the kernel calls. */
int plk_debug_glv_split(plk_ctx* ctx, const plk_fr* s, size_t n, uint64_t* out);
/* out[i] = the weight rho_i of plk_srs_fold for an SRS of n points and this seed, i < n - 1
 * (canonical Montgomery). ctx = NULL: computed on the host (the mirror of the kernel). */
int plk_debug_srs_weights(plk_ctx* ctx, const uint8_t seed[32], size_t n, plk_fr* out);
/* One host Fp2 square root (csrc/pairing_host.hpp f2_sqrt): a = (c0, c1) as 12 Montgomery limbs;
 * *is_square = 1 and out = a root, or *is_square = 0. Needs no GPU. */
int plk_debug_f2_sqrt(const uint64_t* a, uint64_t* out, int* is_square);
/* Elementwise device field arithmetic on host arrays (used by the parity tests to pin the
 * gfx950 multiplier against the oracle): field 0 = Fr (4 limbs), 1 = Fp (6 limbs);
 * op 0 = a*b, 1 = a+b, 2 = a-b, 3 = a^2, 4 = a^-1 (Montgomery form in and out). */
int plk_debug_field_op(plk_ctx* ctx, int field, int op, const uint64_t* a, const uint64_t* b,
                       uint64_t* out, size_t n);
/* The redundant-limb field of the hot loops (csrc/ffr.hpp) on raw limb rows: field 0 = Fr
 * (L = 9 limbs of 29 bits), 1 = Fp (L = 13 limbs of 30 bits). Operands a, b, c, d are n rows of L
 * uint32 limbs each; a thread copies its rows into Rx values unchanged (nothing is unpacked,
 * reduced or normalised) and writes each result's limbs back raw: out holds n x (outputs of the
 * op) rows, row i * outputs + j = output j of input row i. Operands an op does not read may be
 * NULL. Ops (outputs; (A) marks the form with its columns as inline-asm statements):
 *    0 rx_mul a b                  1 rx_sqr a                 2 rx_mul_add a b + c d
 *    3 rx_mul2 (a b, c d)          4 rx_mul2 (A)              5 rx_sqr2 (a^2, b^2)
 *    6 rx_sqr2 (A), Fp only        7 rx_mul_add_mul2 (a b + c d, a d, c b)
 *    8 rx_mul_add_mul2 (A), Fp only                           9 rx_mul3 (a b, c d, d a)
 *   10 rx_add a + b               11 rx_sub a - b            12 rx_sub_lazy a - b
 *   13 rx_sub2_n<6> a + 6p - b - 2c                          14, 15 rx_small_mul_n<2>, <3> a
 *   16 rx_canon a                 17 rx_is_zero a            18 rx_is_zero_u a
 *   19 (rx_unpack a, rx_pack of that): a's first 8 (Fr) / 12 (Fp) words are a packed value;
 *      output 0 its limbs, output 1 the words packed back (the rest of the row 0)
 *   100 + CP rx_sub_u<CP> a + CP p - b, 200 + CP rx_sub_n<CP>: CP in 3, 5, 6 and for Fp 4, 10
 * The two tests write 0 / 1 into limb 0 of an otherwise zero row. Other codes: PLK_E_ARG. */
int plk_debug_rx_op(plk_ctx* ctx, int field, int op, const uint32_t* a, const uint32_t* b,
                    const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n);
/* The lazy butterfly helpers of the NTT pass kernel (csrc/ntt.hip), the functions k_ntt_pass
 * calls, on raw Fr limb rows (9 uint32 each, copied into the kernel's values unchanged). in holds
 * n cases of (operand rows of the op) rows, out n cases of (outputs) rows; a twiddle t is an
 * R'-domain limb row that the hook stages in LDS where the helper reads it. Ops (operands ->
 * outputs):
 *    0 reduce_q a                              1 add_u a + b            2 sub_u a + 3r - b
 *    3 sub_u2<11> a + 11r - b, the raw unnormalised limbs
 *    4 r4_math<false> x0 x1 x2 x3, t(r s1) t((r + h) s1) t(r s2) -> o0 o1 o2 o3
 *    5 r4_math<true> x0 x1 x2 x3, t -> o0 o1 o2 o3
 *    6 the first stage of an odd radix: a v t -> reduce_q(add_u(a, v)), twmul(sub_u(a, v), t)
 *    7 the last stage of an odd radix: a c -> reduce_q(add_u(a, c)), reduce_q(rx_sub_u<6>(a, c))
 *    8 the store without a scale (POST 0): v -> rx_pack_canonical(reduce_q(v))
 *    9 the store with the scalar (POST 1): v s -> rx_pack_canonical(rx_mul(v, rx_unpack(s))); s is
 *      the kernel argument, taken from case 0 for all cases
 *   10 the store with the scale table (POST 2): the same with each case's own s
 * s is a packed canonical R'-domain value in the first 8 words of its row; the stores return the
 * packed word the same way (word 8 is 0). Other codes, a NULL argument: PLK_E_ARG. */
int plk_debug_ntt_lazy_op(plk_ctx* ctx, int op, const uint32_t* in, uint32_t* out, size_t n);
/* The XYZZ group law over that field (csrc/g1r.hpp) on raw limb rows: p, q and out are rows of
 * 4 x 13 limbs (X, Y, ZZ, ZZZ; R' = 2^390 domain), an affine q uses X and Y only. Bit 0 of
 * flags[i] (flags may be NULL) negates q: the lazy 4p - Y (rx_neg_lazy) for the lazy ops,
 * rx_neg for the others. Ops:
 *    0..3 g1r_madd_lazy_sl<GROUPED, ASM, PAIRS> as (0,0,0), (1,0,0), (1,1,0), (1,1,1), in the
 *         sequence of k_accumulate: the flag's rx_neg_lazy, the straight-line addition, and on a
 *         zero ZZ g1r_madd_lazy_fix with the canonical (negated) point
 *    4 g1r_madd_lazy      5 g1r_add_lazy
 *    6 g1r_add_quad: every row runs on the four lanes of a quad and out holds 4 n rows, row
 *      4 i + l = lane l's result
 *    7 g1r_dbl_lazy p     8 g1r_lazy_finish p        9 g1r_add        10 g1r_add_affine
 *   11 g1r_dbl p         12 g1r_dbl_affine of (p.X, p.Y)
 * q may be NULL for the ops of p alone. */
int plk_debug_g1r_op(plk_ctx* ctx, int op, const uint32_t* p, const uint32_t* q,
                     const uint32_t* flags, uint32_t* out, size_t n);
/* The prover's forward block transform: the polynomial of `len` <= n + 8 coefficients
 * (Montgomery form) evaluated on the blocks of the key's quotient domain, the cosets
 * g w_8n^m H_n, m < blocks (5; 6 for n = 8): out[m * n + u] = p(g w_8n^m w_n^u), the point
 * 8u + m of the reference's g H_8n. out holds blocks * n values; *blocks_out (may be NULL)
 * receives the block count. out == NULL only reports the block count. (The prover's round 3
 * itself uses the first four of these cosets for n >= 16; this call evaluates on five.) */
int plk_debug_block_eval(plk_key* key, const uint64_t* coef, size_t len, uint64_t* out,
                         size_t out_cap, int* blocks_out);
/* One stage of the prover's rounds on caller arrays: the arrays are copied to the device, the
 * pk_* launcher the prover calls for that stage runs on them (csrc/prover_kernels.hip; nothing is
 * computed on the host beyond what the launcher itself does), and the result is copied back.
 * in[k] holds in_len[k] field elements (4 uint64 each, Montgomery form unless noted), scalars are
 * Montgomery-form plk_fr, out takes out_cap elements. Stages (inputs; scalars; params -> out):
 *   0 pk_perm_numden: wires (4 columns of `stride`), sigmas (4 x n), elements (n); beta gamma k1
 *     k2 k3; n, stride >= n -> num (n) then den (n)
 *   1 pk_scan: data (n); -; flags 1 multiply (else add) | 2 suffix | 4 exclusive | 8 in place ->
 *     the n outputs, then the grand total the prover reads at tmp[blocks]
 *   2 pk_quotient: a b c d z pi l1 sel sigma elements exactly as k_quotient reads them: nq =
 *     blocks * n points each, sel 11 rows and sigma 4 rows of nq, elements n; the wires at exponent
 *     -1 (the values times 2^5), pi at +1 (times 2^-5; length 0: no public inputs), the rest plain;
 *     alpha beta gamma range_sep logic_sep fixed_sep var_sep, s_m[blocks], vh_inv[blocks];
 *     log2 n, blocks (5 or 6), 1 has_range | 2 has_logic | 4 has_fixed | 8 has_var -> t (nq).
 *     The constants come from the function the prover fills its QuotientArgs with.
 *   3 pk_pi_sparse: l1 (nq); the values; log2 n, then one gate index per value -> the PI row (nq)
 *   4 pk_pi_coef: tw_inv (n; w^-e times 2^261, the domain's inverse table); value / n per input;
 *     one gate index per input -> the coefficients (n)
 *   5 pk_coset_combine: blocks x n coefficients; the blocks^2 matrix entries (times 2^5, row
 *     major); blocks -> blocks x n
 *   6 pk_eval: up to 28 polynomials; one point each; - -> one value each
 *   7 pk_lincomb: up to 24 terms; one scalar each; len_out -> len_out
 *   8 pk_scale_powers: c; x; shift -> c_j x^(j + shift)
 *   9 pk_ruffini: c (len); z (not 0); - -> the len - 1 coefficients of (c(X) - c(z)) / (X - z)
 *  10 quotient_top (host code, ctx may be NULL): the top seven coefficients, in ascending order, of
 *     the wires (4 x 7: n-5 .. n+1), z (7: n-4 .. n+2), the selectors (11 x 7, gate order: n-7 ..
 *     n-1), the sigmas (4 x 7) and L1 (7); alpha beta gamma range_sep logic_sep fixed_sep var_sep,
 *     omega, then the public-input values; log2 n (>= 4), the has_* flags as in stage 2, then one
 *     gate index per public input -> t[4n .. 4n + 6], the numerator's coefficients 5n .. 5n + 6
 *  11 pk_coset_combine_top: 4 x n coefficients (the inverse block transforms); the 16 matrix
 *     entries (times 2^5, row major), t[4n .. 4n + 6], then p_0 .. p_4 with prod_{m<4} (Y - c_m) =
 *     sum p_l Y^l; - -> the 4n + 8 coefficients of t
 * PLK_E_ARG: an unknown stage, a NULL array of non-zero length, lengths that do not fit together,
 * out_cap too small, and whatever the launcher itself refuses. A zero-length problem is PLK_OK and
 * writes nothing. */
int plk_debug_prover_stage(plk_ctx* ctx, int stage, const uint64_t* const* in, const size_t* in_len,
                           size_t n_in, const plk_fr* scalars, size_t n_scalars,
                           const uint64_t* params, size_t n_params, uint64_t* out, size_t out_cap);
/* The polynomials of the prover's last round 3, Montgomery form: alpha beta gamma range_sep
 * logic_sep fixed_sep var_sep, the 11 selectors' n coefficients each (gate order), the 4 sigmas',
 * the 4 blinded wires' n + 2, z's n + 3 and t's 4n + 8: 24n + 26 elements. PLK_E_ARG unless the
 * prover's last plk_prover_prove reached round 3 on a key with n >= 16, or out_cap is too small. */
int plk_debug_prover_round3(plk_prover* p, uint64_t* out, size_t out_cap);
/* The device-mode fold weights (plk_verifier_set_replay) from given entropy and u challenges
 * (Montgomery form): out[j] = rho_j, j < count. ctx = NULL: the host mirror, no GPU; otherwise
 * the kernel the fold runs. PLK_E_ARG: a NULL argument, count = 0, a non-canonical u. */
int plk_debug_fold_weights(plk_ctx* ctx, const uint8_t entropy[32], const plk_fr* u, size_t count,
                           plk_fr* out);
/* out[72 i ..] = ML(p_i, q)^(3 (p^12 - 1) / r) = e(p_i, q)^3 as 12 Fp values (6 LE u64 Montgomery
 * limbs each): the coefficient of w^k, k < 6, of Fp12 = Fp2[w] / (w^6 - (1 + u)) as (c0, c1). A p_i
 * at infinity gives one. ctx = NULL: the host code; otherwise the kernel. This project's own
 * coefficient order and power (the cube), not a reference-compatible Gt encoding. q: finite,
 * canonical, on the twist, of order r; n <= 4096. */
int plk_debug_pairing(plk_ctx* ctx, const plk_g1* p, const plk_g2* q, size_t n, uint64_t* out);
/* One operation of the pairing's tower (csrc/pairing.hpp) on n rows of plk_debug_pairing's layout
 * (72 u64: the six Fp2 coefficients of w^0 .. w^5 as (c0, c1) Montgomery limbs): out row i =
 * op(a row i, b row i). ctx = NULL: the host slot store; otherwise one lane per row over the
 * kernel's wave-tiled workspace. Ops:
 *    0 f2_mul a b      1 f2_sqr a      2 f2_inv a      3 f2_mul_xi a: the Fp2 function applied to
 *      each of the six coefficients (of a and b pairwise)
 *    4 f12_mul a b     5 f12_sqr a     6 f12_cyc_sqr a (a in the cyclotomic subgroup; undefined
 *      elsewhere)      7 f12_inv_even a (a in Fp6: even coefficients; the odd ones return zero)
 *    8 f12_conj a      9 f12_frob a^p                 10 f12_frob a^(p^2)
 *      each out of place, or with PLK_F12_IN_PLACE added to the op on the operand's own slot
 *   11 f12_mul_line a (c0 + c2 w^2 + y w^3): b row = c0 (limbs 0..11), c2 (12..23), y (24..29)
 *   12 f12_final_exp a: a^(3 (p^12 - 1) / r)
 * The operands of an Fp12 operation sit in distinct slots and the result in a third, as the
 * functions require. b may be NULL for the ops of a alone (it is not read). PLK_E_ARG: another op,
 * PLK_F12_IN_PLACE on an op other than 8..10, a NULL a / out / needed b, a limb row of a or of a
 * needed b (all 72 limbs) that is not canonical, n = 0, n > 4096. */
#define PLK_F12_IN_PLACE 0x100
int plk_debug_f12_op(plk_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n,
                     uint64_t* out);
/* out[72 i ..] = the raw Miller value, before the final exponentiation, in the same layout.
 * p1 = NULL: ML(p0_i, q0), what plk_debug_pairing raises to its power (q1 is not read). Otherwise
 * ML(p0_i, q0) ML(-p1_i, q1) with the squarings shared, exactly the value plk_pairing_check[_batch]
 * computes for the pair (C, W) = (p0_i, p1_i) against (H, beta_h) = (q0, q1). A point at infinity
 * contributes the factor one. ctx = NULL: the host code; otherwise a kernel that makes k_pairing's
 * call. p0, p1: plk_g1 rules of plk_msm_points (on the curve; the subgroup is not checked); q0, q1:
 * finite, canonical, on the twist, of order r; n <= 4096. */
int plk_debug_miller(plk_ctx* ctx, const plk_g1* p0, const plk_g2* q0, const plk_g1* p1,
                     const plk_g2* q1, size_t n, uint64_t* out);

/* What one batch of the fixed-base MSM leaves in its workspace, stage by stage (test support). The
 * call makes a workspace of its own, sets its accumulation form (shared_chip: the prover lanes'
 * grouped k_accumulate instead of the lone form) and the reduction trees' form (tail_quad 0 / 1 /
 * 2, as PLK_TAIL_QUAD), runs the library's own batch on `count` <= 16 slots of host scalars
 * exactly as plk_commit_batch_dev_part does (slot k: lens[k] Montgomery scalars, the first
 * min(lens[k], SRS length) of them committed, the rest required to be zero), and copies the
 * workspace out. No kernel and no launch differs from plk_commit_batch_dev_part's.
 *
 * hdr (PLK_MSM_SNAPSHOT_HDR words): B W narrow c chunk rb fb NC NR G nbits nout wide sort_one hold
 * task_stride sorted_stride max_tasks_used b_lo n_srs gen part parts has_inf — the bucket count of
 * the call (a part's range for parts > 1), the window count and the number of narrow top windows,
 * the window size, the task length, the run, fine-bin, coarse-bin and group figures of the
 * reduction, the number of bit sums (nbits) and of readback rows (nout), which sort ran, the
 * workspace strides, the bound on a slot's tasks, the part's first bucket, the SRS length, and the
 * batch's generation number (a degree-check flag equal to it is set).
 *
 * Per slot k, each buffer optional (NULL: not copied); 32-bit words:
 *   offsets, task_off   [k (B + 1) ..]: B + 1 words each
 *   sorted              [k cap_sorted ..]: the offsets[B] entry codes, w n_srs + i | sign << 31
 *   tasks               [2 k cap_tasks ..]: n_tasks[k] = task_off[B] records {first entry, partial
 *                       index | (length - 1) << 26}: full tasks in bucket order, then tails grouped
 *                       by length, longest first
 *   partials            [48 k cap_tasks ..]: n_tasks[k] packed R'-domain XYZZ rows of 48 words
 *   bsum                [48 k B ..]: B rows (narrow bucket sets, B <= 32768; untouched otherwise)
 *   rsum                [48 k B ..]: B rows; ys, zs [48 k NR ..]: NR rows (wide sets only)
 *   bits                [48 k nout ..]: the nout readback rows T_j
 *   readback            [3 k ..]: flag, entries, max_count (max_count only with guard_limit)
 * then outs[k] and statuses[k] as plk_commit_batch_dev_part gives them.
 * PLK_E_ARG: a NULL srs / lens / hdr / outs / statuses, count = 0 or > 16, a slot with scalars NULL
 * and a length, tail_quad outside 0..2, parts the SRS does not take, a sorted or tasks capacity
 * too small for a slot (nothing is written past a capacity). Otherwise the batch's status:
 * PLK_OK, or PLK_E_DEGREE when a slot failed its degree check (the buffers are still filled). */
#define PLK_MSM_SNAPSHOT_HDR 24
typedef struct plk_msm_snapshot {
  uint32_t shared_chip, tail_quad, part, parts, guard_limit, reserved;
  uint64_t cap_sorted, cap_tasks; /* per-slot capacities: entries, task records */
  uint32_t *offsets, *task_off, *sorted, *tasks, *partials, *bsum, *rsum, *ys, *zs, *bits;
  uint32_t* readback;
  uint64_t hdr[PLK_MSM_SNAPSHOT_HDR];
  uint32_t n_tasks[16];
} plk_msm_snapshot;
int plk_debug_msm_snapshot(plk_srs* s, const plk_fr* const* scalars, const size_t* lens,
                           size_t count, plk_msm_snapshot* snap, plk_g1* outs, int* statuses);

#ifdef __cplusplus
}
#endif
#endif /* PLK_H */
