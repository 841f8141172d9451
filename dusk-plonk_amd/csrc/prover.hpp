// prover.hpp — proving key and prover objects behind the plk_key / plk_prove entry points of
// include/plk.h (key.hip, commit.hip, prover.hip; the composer is composer.hpp), and the
// kernel-argument structs of prover_kernels.hip.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "composer.hpp"
#include "internal.hpp"
#include "protocol.hpp"
#include "quotient_top.hpp"

// return a PLK_* status other than PLK_OK to the caller
#define TRY(...)                   \
  do {                             \
    int _st = (__VA_ARGS__);       \
    if (_st != PLK_OK) return _st; \
  } while (0)

namespace plk {

// ---- kernel arguments --------------------------------------------------------------
struct BlindArgs {
  Fr r[4];
  uint32_t count;
};
// PI(X) of a few public inputs straight from its definition (pk_pi_coef)
constexpr int kPiDirect = 16;
struct PiDirect {
  uint64_t idx[kPiDirect];  // gate index of each public input
  Fr c[kPiDirect];          // its value times n^-1 (R domain)
  uint32_t count;
};
// the blinding of up to 4 polynomials in one launch (round 1's four wires)
struct BlindBatch {
  Fr* poly[4];
  Fr* lag[4];  // when set: the blinders also go to lag[p][n + i], after the n Lagrange values
  BlindArgs b[4];
  uint32_t npoly;
};

// The quotient domain (round 3). The reference evaluates the quotient over the coset g H_8n
// (quotient_poly.rs:52-58,115). The numerator N (z times four wire factors, degree <= 5n + 6) is
// never interpolated: k_quotient evaluates t(x) = N(x) / Z_H(x) exactly at each point from
// exact evaluations of the factors, and only t is interpolated. t is unique (degree <= 4n + 6),
// so however its coefficients are found, commitments and proofs are the same bit for bit. The
// points are cosets of the n-domain itself, s_m H_n with s_m = g w_8n^m: every point is point
// 8u + m of the reference's own g H_8n, and every block transform is an n-point one (key->dom).
// Every quotient-domain vector is laid out in blocks of n (block m = coset m, natural order in
// u): evaluation point x(m, u) = s_m w_n^u, the next row (w_n x) is u + 1 in the same block, and
// v_h(x) = x^n - 1 = c_m - 1 with c_m = s_m^n = g^n w_8^m is constant per block (distinct values,
// none equal to 1).
//
// Inverse: the inverse block transform m gives r_m = t mod (X^n - c_m), r_m[k] = sum_l c_m^l
// t_l[k] for the n-coefficient chunks t_l of t; the chunks come back through the inverse
// Vandermonde matrix of the c_m (pk_coset_combine; the matrix is computed once per key).
//
// n >= 16: kQBlocksTop = 4 blocks and the top seven coefficients in closed form. 4n points do
// not determine the 4n + 7 coefficients of t, but the seven that do not fit are known without
// any transform: t = N / (X^n - 1) with deg N <= 5n + 6 gives t[4n + j] = N[5n + j], j < 7, and
// the top seven coefficients of a product depend only on the top seven coefficients of its
// factors (quotient_top.hpp: the widget and permutation formulas of protocol.hpp on a
// seven-term power series in 1 / X). The factors' top coefficients are seven field elements
// each: cached per key for the selectors, the sigmas and L1, read back with the round-1 and
// round-2 commits for the wires and z, computed from the public inputs for PI. With
// Q(X) = sum_j t[4n + j] X^j, the four blocks give T_4 = t mod P(X^n), P(Y) = prod_{m<4}
// (Y - c_m) = sum_l p_l Y^l, and t = T_4 + Q(X) P(X^n): the combine adds p_l Q[j] to
// t[l n + j] (l < 4) and writes Q at 4n (pk_coset_combine_top). This is exact for every circuit.
//
// Unsatisfied circuits, n >= 16: N = q Z_H + rho with rho != 0, the four blocks leave no spare
// coefficient to test, and the prover would hand out some polynomial t' of degree <= 4n + 6
// that is not N / Z_H. So after round 4 the prover derives, from the evaluations it is about to
// publish, the quotient value the verifier will derive (proof_at_z, protocol.hpp: N(zeta) /
// Z_H(zeta)) and compares it with t'(zeta) from its own coefficients: unequal is PLK_E_DEGREE,
// the status such a circuit always had. For a satisfied circuit the two are equal by
// construction; for an unsatisfied one N - t' Z_H is a non-zero polynomial of degree <= 5n + 6
// and zeta, drawn after t' is committed, is a root of it with probability about 5n / |Fr|.
//
// n = 8 (the smallest composer) keeps kQBlocksSmall = 6 blocks and the deterministic check:
// the interpolant over B blocks is q + rho(X) A(X^n), A of degree <= B - 1 with
// A(c_m) = 1 / (c_m - 1), whose leading coefficient kappa is not zero (else A(c)(c - 1) - 1, of
// degree <= B - 1, would vanish at B points and hence at c = 1, where it is -1); q has degree
// <= 4n + 6, so the coefficients [40, 48) are kappa rho and the zero check of t_4 past its
// n + 8 committed points (prover.hip round3_quotient) fails there. kQBlocks = 5 is the smallest count that
// determines t for n >= 16 without the closed form: the stage tests and plk_debug_block_eval
// still run it.
constexpr int kQBlocksTop = 4, kQBlocks = 5, kQBlocksSmall = 6, kQBlocksMax = 6;
static_assert(kQBlocksTop == kTopBlocks, "quotient_top.hpp patches a four-block combine");
inline int q_blocks(uint64_t n) { return n >= 16 ? kQBlocksTop : kQBlocksSmall; }
// PI over the quotient domain from at most kPiSparse public inputs as rotated reads of the
// key's L1 table (pk_pi_sparse): L_i(X) = L_0(w^-i X), so PI(s_m w^u) = sum_i pi_i
// l1q[m][(u - i) mod n] — one product per point and public input, no pk_pi_coef, idft or coset
// transform. (Inside k_quotient the loop cost 2 spilled VGPRs at its 168-VGPR, 3-wave budget,
// so it is a kernel of its own that fills the PI row k_quotient reads.)
constexpr int kPiSparse = 4;
struct PiSparse {
  uint32_t count;
  uint32_t idx[kPiSparse];  // gate index of each public input
  Fr v[kPiSparse];          // its value (R domain)
};

struct QuotientArgs {
  const Fr *a, *b, *c, *d, *z, *pi, *l1, *sel, *sigma, *elements;  // pi null: no public inputs
  Fr* out;
  uint64_t nq;        // quotient-domain points: q_blocks(n) blocks of n
  uint32_t log_blk;   // log2(n)
  Fr g, alpha, alpha2, beta, gamma, k1, k2, k3;
  Fr range_sep, kappa, kappa2, kappa3;
  Fr logic_sep, lk, lk2, lk3, lk4;  // logic separation challenge and its kappa powers
  Fr fixed_sep, fk, fk2, fk3;        // fixed-base scalar mul: sep, kappa = sep^2, ^2, ^3
  Fr var_sep, vk, vk2;               // variable-base addition: sep, kappa = sep^2, ^2
  Fr edwards_d;                      // JubJub d (protocol.hpp edwards_d)
  int has_range, has_logic, has_fixed, has_var;
  Fr vh_inv[kQBlocksMax];  // 1 / v_h of block m
  // k_quotient runs in the redundant form (ffr.hpp): a value with exponent e is stored as
  // x R 2^(-5e) (e = 0: the R domain; e = -1: the R' domain) and rx_mul adds exponents
  // plus one. Wire evaluations arrive at e = -1 (coset table scaled by 2^5), public
  // inputs at e = +1, z / selectors / sigmas / L1 / elements at e = 0; these constants are
  // pre-scaled so every term meets at e = 1 and num / v_h lands at e = 0 (the R domain).
  Fr rx_bg[kQBlocksMax], rx_beta, rx_gamma;  // beta s_m and beta at e = -2, gamma at e = -1
  Fr rx_one_w, rx_two_w, rx_three_w;    // 1, 2, 3 at e = -1 (range widget deltas)
  Fr rx_kappa, rx_kappa2, rx_kappa3;    // range kappa powers at e = -1
  Fr rx_alpha2;                         // alpha^2 at e = -1 (alpha and range_sep at e = 0)
  Fr rx_vh[kQBlocksMax];                // 1 / v_h at e = -2
  Fr rx_inv32, rx_32;                   // 2^-5 and 2^5 (R domain): k_quotient_ext converts
};

// The transcript challenges k_quotient / k_quotient_ext take (R domain)
struct QuotientChallenges {
  Fr alpha, beta, gamma, range_sep, logic_sep, fixed_sep, var_sep;
};
// Every field of qa that is neither an array pointer nor a size (nq, log_blk, g): the
// challenges, K1..K3, the kappa powers, the has_* flags, vh_inv[] and the exponent-scaled
// constants, from the challenges and the key's s_m[] / vh_inv[] (`blocks` entries each).
// Host code (prover.hip); the prover and plk_debug_prover_stage both fill QuotientArgs here.
void quotient_constants(QuotientArgs& qa, const QuotientChallenges& ch, const Fr* s_m,
                        const Fr* vh_inv, int blocks, bool has_range, bool has_logic,
                        bool has_fixed, bool has_var);

constexpr int kMaxEval = 28;  // 16 proof evaluations + the linearisation terms at z
struct EvalBatch {
  const Fr* poly[kMaxEval];
  uint64_t len[kMaxEval];
  Fr x[kMaxEval];
};

constexpr int kMaxTerms = 24;  // the opening aggregate with r(X) expanded in place
struct LinComb {
  const Fr* p[kMaxTerms];
  uint64_t len[kMaxTerms];
  Fr s[kMaxTerms];
  uint32_t terms;
};

// out[col * stride + i] (col < 4, i < n): the wire's witness, zero for i >= m
int pk_gather_wires(const Fr* witness, const uint32_t* idx, uint64_t m, uint64_t n, Fr* out,
                    uint64_t stride, hipStream_t s);
int pk_blind(Fr* poly, uint64_t n, const BlindArgs& b, hipStream_t s);
int pk_blind_batch(const BlindBatch& bb, uint64_t n, hipStream_t s);
// coefficients of PI(X) = idft(public-input vector) for at most kPiDirect public inputs:
// out[j] = sum_k c_k w^(-idx_k j), w^-e from the domain's R'-domain table tw_inv
int pk_pi_coef(const PiDirect& pd, const Fr* tw_inv, uint64_t n, Fr* out, hipStream_t s);
// out[m n + u] = sum_k v_k l1[m n + ((u - idx_k) mod n)] at exponent +1, over nq = blocks * n points
int pk_pi_sparse(const PiSparse& ps, const Fr* l1, uint32_t log_n, uint64_t nq, Fr* out,
                 hipStream_t s);
int pk_fill(Fr* out, const Fr& v, uint64_t n, hipStream_t s);
int pk_perm_numden(const Fr* wires, uint64_t wire_stride, const Fr* sigmas, const Fr* elements,
                   uint64_t n, const Fr& beta, const Fr& gamma, const Fr& k1, const Fr& k2, const Fr& k3,
                   Fr* num, Fr* den, hipStream_t s);
int pk_mul3(const Fr* a, const Fr* b, const Fr& c, Fr* out, uint64_t n, hipStream_t s);
uint64_t pk_scan_tmp_elems(uint64_t n);
int pk_scan(const Fr* in, Fr* out, uint64_t n, bool mul, bool suffix, bool exclusive, Fr* tmp,
            hipStream_t s);
int pk_quotient(const QuotientArgs& q, hipStream_t s);
// t coefficients from the `blocks` inverse block transforms r_m (n coefficients each, in + m n):
// out[k + l n] = sum_m mat[l * blocks + m] r_m[k] for l, m < blocks; mat: the inverse
// Vandermonde matrix of the c_m (prover.hpp top), R'-domain constants
struct CombineMat {
  Fr m[kQBlocksMax * kQBlocksMax];
};
int pk_coset_combine(const Fr* in, uint64_t n, int blocks, const CombineMat& mat, Fr* out,
                     hipStream_t s);
// the same over kQBlocksTop blocks (mat: 4 x 4), then t = T_4 + Q(X) P(X^n) (prover.hpp top):
// out[l n + j] += patch.v[l][j] for l < 4 and out[4n + j] = patch.v[4][j], j < 8 (R domain);
// out holds 4n + 8 coefficients, n >= 8
int pk_coset_combine_top(const Fr* in, uint64_t n, const CombineMat& mat,
                         const QuotientPatch& patch, Fr* out, hipStream_t s);
// out[j] = in[j] * c (packed Montgomery product), j < n
int pk_scale_copy(const Fr* in, const Fr& c, Fr* out, uint64_t n, hipStream_t s);
uint32_t pk_eval_max_blocks(uint64_t max_len);
int pk_eval(const EvalBatch& e, uint32_t count, uint64_t max_len, Fr* partial, Fr* d_out,
            hipStream_t s);
int pk_lincomb(const LinComb& lc, Fr* out, uint64_t len_out, hipStream_t s);
int pk_scale_powers(const Fr* c, uint64_t len, const Fr& x, uint64_t shift, Fr* y, hipStream_t s);
int pk_ruffini(const Fr* c, uint64_t len, const Fr& z, Fr* q, Fr* tmp, Fr* scan_tmp,
               hipStream_t s);

struct CheckWs;  // circuit_check.hpp

// ---- the quotient domain's block transforms (key.hip) ------------------------------
// s_m[m] = g w_8n^m, m < blocks: the shifts of the cosets s_m H_n of dom
PLK_LOCAL void coset_shifts(const plk_domain* dom, int blocks, Fr* s_m);
// The forward coset transforms of one polynomial (len <= n + 8 coefficients, folded onto the
// block) onto `blocks` cosets in one launch per pass: block m to out + m n, pre-multiplied by
// row m of `table` (rows of n + 8: s_m^j, scaled or not). Key compilation, the prover's
// round 3 and plk_debug_block_eval all transform through here.
PLK_LOCAL int coset_blocks_fwd(plk_domain* dom, const Fr* in, Fr* out, uint64_t len,
                               const Fr* table, int blocks, Fr* scratch, hipStream_t s);
// out[0 .. count] = the coefficients of prod_{j < count} (X - c[j]), lowest first
PLK_LOCAL void poly_from_roots(const Fr* c, int count, Fr* out);

}  // namespace plk

struct plk_key {
  plk_ctx* ctx = nullptr;
  plk_srs* srs = nullptr;
  std::string label;
  uint64_t m = 0, n = 0, n_trim = 0;
  uint32_t k = 0;
  plk_domain* dom = nullptr;   // n (also the blocks of the quotient domain, prover.hpp top)
  // the Lagrange-basis SRS of the domain (lagrange.hip; owned): [L_i(tau)]_1, i < n, then the
  // three blinder points, with the SRS's window size. Round 1 commits the wires from their
  // values on it. Null when PLK_LAGRANGE_COMMIT=0 or the SRS has fewer than n + 3 points.
  plk_srs* lag = nullptr;
  int qb = 0;                  // q_blocks(n)
  bool has_range = false, has_logic = false, has_fixed = false, has_var = false;
  // device-resident proving key
  plk::DevBuf q_coef;       // 11 x n selector coefficient polys
  plk::DevBuf selq;         // SEL_COUNTQ x qb n quotient-domain evaluations
  plk::DevBuf sigma_coef;   // 4 x n
  plk::DevBuf sigma_lag;    // 4 x n Lagrange values (= dft of sigma_coef, cached)
  plk::DevBuf sigmaq;       // 4 x qb n
  plk::DevBuf l1q;          // L1 over the quotient domain: coset_dft(idft(e_0)) (quotient_poly.rs:264-272)
  // forward coset tables, qb rows of n + 8 (R' domain): s_m^j for selectors, sigmas,
  // L1 and z; 2^5 s_m^j for the wires (evaluations at e = -1); 2^-5 s_m^j for PI (e = +1)
  plk::DevBuf coset_s, coset_w, coset_pi;
  plk::DevBuf icoset_q;     // qb rows of n: n^-1 s_m^-k (R'), inverse blocks
  plk::Fr s_m[plk::kQBlocksMax];  // g w_8n^m (R domain)
  plk::Fr c_m[plk::kQBlocksMax];  // s_m^n (R domain)
  plk::CombineMat comb;     // pk_coset_combine's matrix (R')
  plk::DevBuf wire_idx;     // 4 x n witness indices per gate (u32)
  // the compact gate table of plk_prover_diagnose (circuit_check.hpp): the composer's m gate
  // records and its pooled constants, a public-input slot holding the gate's ordinal among the
  // public inputs in place of the compile-time value
  plk::DevBuf gate_recs, gate_consts;
  plk::Fr vh_inv[plk::kQBlocksMax];
  // the closed-form top of t (prover.hpp top; qb == kQBlocksTop): the top seven coefficients of
  // the selectors, the sigmas and L1 (wire and z rows are filled per proof), the coefficients
  // p_l of prod_{m<4} (Y - c_m), and w^i / w^-i of every public-input row i (PI's top
  // coefficients; the self-check at zeta)
  plk::QuotientTopIn top_in;
  plk::Fr top_p[plk::kQBlocksTop + 1];
  std::vector<plk::Fr> pi_w, pi_winv;
  plk_g1 comms[15];         // q_m q_l q_r q_o q_c q_4 q_arith q_range q_logic q_fixed q_var s1..s4
  // the circuit the key was compiled from: plk_prove refuses a circuit whose structure hash
  // differs or whose witness vector does not cover the largest wire index (prover.rs:114-119
  // reads the wires of the proving circuit; the key's gather indices must be valid for it)
  uint64_t struct_hash = 0;
  uint32_t max_wire = 0;
  // the prover behind plk_prove(key, ...) (context stream), created on first use
  std::mutex def_mu;
  std::unique_ptr<plk_prover> def_prover;
  ~plk_key();
};

// One concurrent prover over a key (include/plk.h plk_prover): stream, MSM workspace, NTT
// scratch and per-proof buffers of its own; the key and the SRS window table are shared
// read-only by every prover of the key.
struct plk_prover {
  plk_key* key = nullptr;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  plk::MsmWorkspace* ws = nullptr;  // owned (msm_workspace_new)
  // sharded commits (plk_prover_shard): this rank's SRS slice and the all-gather
  plk_srs* shard = nullptr;
  uint64_t shard_lo = 0;
  // plk_prover_shard_buckets (round 6): every commit on the key's own (whole) SRS, this rank
  // keeping bucket range `rank` of `world` (msm_run_batch part / parts) instead of a slice
  bool shard_buckets = false;
  int rank = 0, world = 1;
  plk_allgather_fn allgather = nullptr;
  void* allgather_user = nullptr;
  // per-proof scratch
  plk::PinnedBuf pin_witness, pin_small;  // host staging of the witness upload / small readbacks
  // the wires' coefficients n-5 .. n+1 (4 x 7) and z's n-4 .. n+2, copied back behind the
  // round-1 and round-2 commits (quotient_top.hpp)
  plk::PinnedBuf pin_top;
  // plk_debug_prover_round3: the last proof's alpha, beta, gamma and separation challenges, set
  // once its t_coef is queued
  plk::Fr last_ch[7];
  bool have_round3 = false;
  // the round-4 evaluations: coherent mapped host memory that k_eval_final writes directly
  plk::PinnedBuf eval_out;
  void* eval_dev = nullptr;  // eval_out's device address
  // the last proof's wire commits (plk_prover_commit_info): basis (0 coefficients, 1
  // Lagrange values) and MSM entry count per wire
  int commit_basis[4] = {0, 0, 0, 0};
  uint64_t commit_entries[4] = {0, 0, 0, 0};
  // plk_prover_diagnose: whether `witness` holds the most recent plk_prover_prove's upload, that
  // proof's public-input values in gate order (host, and their device copy), and the check's own
  // buffers, made on first use
  bool have_witness = false;
  std::vector<plk::Fr> last_pi;
  plk::DevBuf pi_vals;
  plk::CheckWs* check_ws = nullptr;
  plk::DevBuf witness, wires_lag, wires_coef, z_lag, z_coef, num, den, tmp_a, scan_tmp, pi_lag,
      pi_coef, evq, quotq, t_coef, agg, agg2, w_coef, eval_partial, ntt_scratch;
  ~plk_prover();
};

// ---- commit paths (commit.hip) -----------------------------------------------------
namespace plk {
// commit a batch of device polys against the key's trimmed SRS (key.rs:81-82): a poly whose
// non-zero part is longer than the trimmed SRS fails with PLK_E_DEGREE. `ws` / `s`: the
// calling prover's MSM workspace and stream. cap: commit at most `cap` points, the rest of each
// polynomial must be zero (else PLK_E_DEGREE) — the quotient chunks' bound
PLK_LOCAL int key_commit(plk_key* key, MsmWorkspace& ws, const std::vector<const Fr*>& ptrs,
                         const std::vector<size_t>& lens, plk_g1* outs, int* statuses,
                         hipStream_t s, size_t cap = SIZE_MAX, MsmSlotInfo* info = nullptr);
// the same for a prover: over the ranks of a sharded one, else key_commit on its stream
PLK_LOCAL int prover_commit(plk_prover* P, const std::vector<const Fr*>& ptrs,
                            const std::vector<size_t>& lens, plk_g1* outs, int* statuses,
                            size_t cap = SIZE_MAX);
// Round 1's four wire commits, each from its Lagrange values [w(omega^i) | b_0 b_1] (lag + c
// stride) unless that wire is hot, else from its blinded coefficients (coef + c stride); fills
// P->commit_basis / commit_entries
PLK_LOCAL int commit_wires(plk_prover* P, const Fr* lag, const Fr* coef, uint64_t stride,
                           plk_g1 out[4]);
}  // namespace plk
