// prover.hip — host orchestration of Prover::create_proof (src/prover.rs:67-474) on the GPU: one
// function per round over a ProofRun, every O(n) step on the device (ntt.hip, msm.hip,
// prover_kernels.hip; the commits through commit.hip) and only the transcript and O(1) scalar
// algebra on the host. The composer is composer.hip, the proving key key.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "ffr.hpp"
#include "msm_common.hpp"
#include "prover.hpp"
#include "transcript.hpp"

using namespace plk;

namespace plk {
void quotient_constants(QuotientArgs& qa, const QuotientChallenges& ch, const Fr* s_m,
                        const Fr* vh_inv, int blocks, bool has_range, bool has_logic,
                        bool has_fixed, bool has_var) {
  const Fr alpha2 = fe_sqr(ch.alpha);
  qa.alpha2 = alpha2;
  qa.alpha = ch.alpha;
  qa.beta = ch.beta;
  qa.gamma = ch.gamma;
  qa.k1 = perm_k(1);
  qa.k2 = perm_k(2);
  qa.k3 = perm_k(3);
  const SepPowers rk = sep_powers(ch.range_sep), lk = sep_powers(ch.logic_sep),
                  fk = sep_powers(ch.fixed_sep), vk = sep_powers(ch.var_sep);
  qa.range_sep = ch.range_sep;
  qa.kappa = rk.k, qa.kappa2 = rk.k2, qa.kappa3 = rk.k3;
  qa.has_range = has_range ? 1 : 0;
  qa.logic_sep = ch.logic_sep;
  qa.lk = lk.k, qa.lk2 = lk.k2, qa.lk3 = lk.k3, qa.lk4 = lk.k4;
  qa.has_logic = has_logic ? 1 : 0;
  qa.fixed_sep = ch.fixed_sep;
  qa.fk = fk.k, qa.fk2 = fk.k2, qa.fk3 = fk.k3;
  qa.var_sep = ch.var_sep;
  qa.vk = vk.k, qa.vk2 = vk.k2;
  qa.edwards_d = edwards_d();
  qa.has_fixed = has_fixed ? 1 : 0;
  qa.has_var = has_var ? 1 : 0;
  for (int j = 0; j < blocks; ++j) qa.vh_inv[j] = vh_inv[j];
  // exponent-scaled constants for k_quotient (x[e] = x R 2^(-5e); [-1] = R' domain)
  auto em1 = [](const Fr& x) { return fe_to_rx_domain(x); };
  auto em2 = [](const Fr& x) { return fe_to_rx_domain(fe_to_rx_domain(x)); };
  const Fr one = fe_one<FrCfg>(), two = fe_dbl(one);
  for (int mb = 0; mb < blocks; ++mb) qa.rx_bg[mb] = em2(fe_mul(ch.beta, s_m[mb]));
  qa.rx_beta = em2(ch.beta);
  qa.rx_gamma = em1(ch.gamma);
  qa.rx_one_w = em1(one);
  qa.rx_two_w = em1(two);
  qa.rx_three_w = em1(fe_add(two, one));
  qa.rx_kappa = em1(qa.kappa);
  qa.rx_kappa2 = em1(qa.kappa2);
  qa.rx_kappa3 = em1(qa.kappa3);
  qa.rx_alpha2 = em1(alpha2);
  for (int j = 0; j < blocks; ++j) qa.rx_vh[j] = em2(vh_inv[j]);
  qa.rx_32 = fr_u64(32);
  qa.rx_inv32 = fe_inv(qa.rx_32);
}
}  // namespace plk

namespace {

enum { QM = SEL_QM, QL = SEL_QL, QR = SEL_QR, QO = SEL_QO, Q4 = SEL_Q4, QC = SEL_QC,
       QARITH = SEL_QARITH, QRANGE = SEL_QRANGE, QLOGIC = SEL_QLOGIC, QFIXED = SEL_QFIXED,
       QVAR = SEL_QVAR };  // the selector rows (protocol.hpp), short

Fr d2h_fr(const Fr* p, hipStream_t s) {
  thread_local PinnedBuf pin;
  if (pin.alloc(sizeof(Fr)) != PLK_OK) return fe_zero<FrCfg>();
  (void)hipMemcpyAsync(pin.ptr, p, sizeof(Fr), hipMemcpyDeviceToHost, s);
  (void)stream_wait(s);
  return *pin.as<Fr>();
}

// quotient_numerator's widget flags of a key
unsigned top_flags(const plk_key* key) {
  return (key->has_range ? 1u : 0u) | (key->has_logic ? 2u : 0u) | (key->has_fixed ? 4u : 0u) |
         (key->has_var ? 8u : 0u);
}

// r(X) = sum_t s_t p_t(X) (arithmetic / range / logic / curve widgets' linearize and the
// permutation's): its polynomials p_t are known before round 4, its scalars s_t only from the
// evaluations. So r is never formed: its terms' values at z join the batch of the 16
// proof evaluations (one launch, one read-back), r(z) = sum_t s_t p_t(z) is taken on the
// host — the same field element — and the opening aggregate carries v s_t p_t itself.
struct RTerm {
  const Fr* p;
  uint64_t len;
  int ev;   // index of p(z) in the evaluation batch
  int lin;  // its scalar s_t: the term of linearisation_scalars (protocol.hpp)
};

// PI(X) = idft of the public-input vector (prover.rs:229) onto the quotient domain: without
// public inputs PI = 0 and the term is skipped; at most kPiSparse, no PI polynomial at all but
// rotated rows of the key's L1 table; at most kPiDirect, the coefficients straight from the
// definition, one product per input and coefficient (no upload, no transform); otherwise the
// vector is uploaded and transformed
enum PiPath { PI_NONE, PI_SPARSE, PI_DIRECT, PI_TRANSFORM };
PiPath pi_path(size_t count) {
  return count == 0 ? PI_NONE : count <= (size_t)kPiSparse ? PI_SPARSE
       : count <= (size_t)kPiDirect ? PI_DIRECT : PI_TRANSFORM;
}

// What one proof shares across its rounds
struct ProofRun {
  plk_prover* P;
  plk_key* key;
  const plk_composer* cs;
  hipStream_t s;
  uint64_t n, S, nq;  // S: padded poly stride; nq: quotient domain, QB blocks of n (prover.hpp)
  int QB;
  bool top4;       // four blocks and the closed-form top (prover.hpp)
  uint64_t t_cap;  // t: at most 4n + 7 coefficients
  Rng rng;
  Transcript tr;
  std::vector<std::pair<uint64_t, Fr>> pis;  // (gate, value) of the public inputs (prover.rs:90-105)
  Fr ch[CH_COUNT] = {};
  // device: wires' values and coefficients (4 x S), z's and t's coefficients, the six polynomials
  // over the quotient domain, NTT and scan scratch, the key's selector and sigma coefficients
  Fr *wl = nullptr, *wc = nullptr, *zc = nullptr, *tc = nullptr, *ev = nullptr, *nsc = nullptr,
     *st = nullptr;
  const Fr *qc = nullptr, *sc = nullptr;
  plk_g1 com[PC_COUNT];  // the proof's commitments so far, in plk_proof order (ProofComm)
  uint64_t t4_len = 0;  // t and t_4 end at 3n + t4_len
  // round 4's results: the batch of evaluations (the proof's 16 first), t(z), z^n and L1(z),
  // r's terms and their scalars
  Fr evs[kMaxEval], t_eval;
  AtZ at;
  std::vector<RTerm> rt;
  std::vector<Fr> rs;

  // transcript seeded like Prover::new (prover.rs:54-55): Transcript::base(label, vk, m)
  ProofRun(plk_prover* P_, const plk_composer* cs_, uint64_t seed)
      : P(P_), key(P_->key), cs(cs_), s(P_->stream), n(key->n), S(n + 8), nq((uint64_t)key->qb * n),
        QB(key->qb), top4(key->qb == kQBlocksTop), t_cap(std::max<uint64_t>(nq, 4 * n + 8)),
        rng{seed}, tr(Transcript::base(key->label, key->comms, key->m)) {
    for (uint64_t i = 0; i < key->m; ++i)
      if (cs->gates[i].code & kPiBit) pis.emplace_back(i, gate_unpack(cs, i).pi);
  }
};

// scratch (allocated once per prover): every allocation of a proof, before anything is queued
int reserve_scratch(ProofRun& R) {
  plk_prover* P = R.P;
  const uint64_t n = R.n, S = R.S, nq = R.nq;
  TRY(P->witness.alloc(std::max<size_t>(R.cs->witness.size(), 1) * sizeof(Fr)));
  TRY(P->wires_lag.alloc(4 * S * sizeof(Fr)));  // per wire: n values, then its blinders
  TRY(P->wires_coef.alloc(4 * S * sizeof(Fr)));
  TRY(P->z_lag.alloc(n * sizeof(Fr)));
  TRY(P->z_coef.alloc(S * sizeof(Fr)));
  TRY(P->num.alloc(n * sizeof(Fr)));
  TRY(P->den.alloc(n * sizeof(Fr)));
  TRY(P->scan_tmp.alloc((pk_scan_tmp_elems(5 * n) + 1) * sizeof(Fr)));
  TRY(P->pi_lag.alloc(n * sizeof(Fr)));
  TRY(P->pi_coef.alloc(n * sizeof(Fr)));
  TRY(P->evq.alloc(6 * nq * sizeof(Fr)));
  TRY(P->quotq.alloc(nq * sizeof(Fr)));
  TRY(P->t_coef.alloc(R.t_cap * sizeof(Fr)));
  TRY(P->pin_top.alloc(5 * kTop * sizeof(Fr)));
  TRY(P->agg.alloc(5 * n * sizeof(Fr)));
  TRY(P->agg2.alloc(S * sizeof(Fr)));
  TRY(P->w_coef.alloc((5 * n + S) * sizeof(Fr)));
  TRY(P->tmp_a.alloc(5 * n * sizeof(Fr)));
  TRY(P->eval_partial.alloc((size_t)kMaxEval * pk_eval_max_blocks(R.t_cap) * sizeof(Fr)));
  if (!P->eval_out.ptr) {
    TRY(P->eval_out.alloc(kMaxEval * sizeof(Fr),
                          hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable));
    PLK_HIP_TRY(hipHostGetDevicePointer(&P->eval_dev, P->eval_out.ptr, 0));
  }
  // 4 nq: the four wires' 4 QB coset blocks transform in one batch (4 QB n of scratch: the
  // output doubles as the other ping-pong buffer, ntt_run_batch)
  TRY(P->ntt_scratch.alloc(4 * nq * sizeof(Fr)));
  // host staging: the witness upload, and the PI values round 3 uploads (sized once: queued
  // copies keep pointing into it)
  TRY(P->pin_witness.alloc(R.cs->witness.size() * sizeof(Fr)));
  TRY(P->pin_small.alloc(std::max<size_t>(R.pis.size(), 1) * sizeof(Fr)));
  R.wl = P->wires_lag.as<Fr>();
  R.wc = P->wires_coef.as<Fr>();
  R.zc = P->z_coef.as<Fr>();
  R.tc = P->t_coef.as<Fr>();
  R.ev = P->evq.as<Fr>();  // z, a, b, c, d, pi, nq points each
  R.nsc = P->ntt_scratch.as<Fr>();
  R.st = P->scan_tmp.as<Fr>();
  R.qc = R.key->q_coef.as<Fr>();
  R.sc = R.key->sigma_coef.as<Fr>();
  return PLK_OK;
}

// witness upload through pinned staging, in chunks: the CPU copy of chunk i+1 overlaps the DMA
// of chunk i (the previous proof's DMA finished at its last wait)
int upload_witness(ProofRun& R) {
  plk_prover* P = R.P;
  const size_t bytes = R.cs->witness.size() * sizeof(Fr);
  const size_t chunk = 8u << 20;
  const char* src = reinterpret_cast<const char*>(R.cs->witness.data());
  char* pin = P->pin_witness.as<char>();
  char* dst = P->witness.as<char>();
  for (size_t off = 0; off < bytes; off += chunk) {
    const size_t len = std::min(chunk, bytes - off);
    std::memcpy(pin + off, src + off, len);
    PLK_HIP_TRY(hipMemcpyAsync(dst + off, pin + off, len, hipMemcpyHostToDevice, R.s));
  }
  // what plk_prover_diagnose checks: this witness with this proof's public inputs
  P->last_pi.resize(R.pis.size());
  for (size_t i = 0; i < R.pis.size(); ++i) P->last_pi[i] = R.pis[i].second;
  P->have_witness = true;
  return PLK_OK;
}

// round 1: wires -> idft -> blind(1) -> commit (prover.rs:107-158)
int round1_wires(ProofRun& R) {
  plk_prover* P = R.P;
  plk_key* key = R.key;
  hipStream_t s = R.s;
  const uint64_t n = R.n, S = R.S;
  Fr *wl = R.wl, *wc = R.wc;
  TRY(pk_gather_wires(P->witness.as<Fr>(), key->wire_idx.as<uint32_t>(), key->m, n, wl, S, s));
  {  // the four wire idfts as one batch (one launch per pass instead of four)
    NttBatch b;
    b.in_stride = S;
    b.out_stride = S;
    TRY(ntt_run_batch(key->dom, wl, wc, n, -1, 0, R.nsc, s, 4, b));
  }
  BlindBatch bb{};
  bb.npoly = 4;
  for (int c = 0; c < 4; ++c) {
    bb.poly[c] = wc + c * S;  // blind(1): b(X)(X^n - 1)
    bb.lag[c] = wl + c * S;
    bb.b[c].count = 2;
    // randomness: two blinders per wire, in wire order, before z's three; nothing else draws
    bb.b[c].r[0] = R.rng.fr();
    bb.b[c].r[1] = R.rng.fr();
  }
  TRY(pk_blind_batch(bb, n, s));
  // the wires' coefficients n-5 .. n+1 for round 3's closed-form top. Stream order: queued
  // before the commits, whose read-back is what completes the copy
  if (R.top4)
    PLK_HIP_TRY(hipMemcpy2DAsync(P->pin_top.ptr, kTop * sizeof(Fr), wc + (n + 2 - kTop),
                                 S * sizeof(Fr), kTop * sizeof(Fr), 4, hipMemcpyDeviceToHost, s));
  // each wire from its values or its coefficients (commit.hip); the coefficients are needed by
  // rounds 3-5 either way
  TRY(commit_wires(P, wl, wc, S, R.com + PC_A));
  R.tr.append_commitment("a_w", R.com[PC_A]);  // transcript: after the PIs
  R.tr.append_commitment("b_w", R.com[PC_B]);
  R.tr.append_commitment("c_w", R.com[PC_C]);
  R.tr.append_commitment("d_w", R.com[PC_D]);
  return PLK_OK;
}

// round 2: permutation grand product z (prover.rs:160-199)
int round2_permutation(ProofRun& R) {
  plk_prover* P = R.P;
  plk_key* key = R.key;
  hipStream_t s = R.s;
  const uint64_t n = R.n;
  // transcript: beta (appended back), then gamma
  const Fr beta = R.ch[CH_BETA] = R.tr.challenge_scalar("beta");
  R.tr.append_scalar("beta", beta);
  const Fr gamma = R.ch[CH_GAMMA] = R.tr.challenge_scalar("gamma");
  Fr* num = P->num.as<Fr>();
  Fr* den = P->den.as<Fr>();
  TRY(pk_perm_numden(R.wl, R.S, key->sigma_lag.as<Fr>(), key->dom->tw_fwd.as<Fr>(), n, beta, gamma,
                     perm_k(1), perm_k(2), perm_k(3), num, den, s));
  TRY(pk_scan(num, num, n, true, false, true, R.st, s));   // N_i = prod_{j<i} num_j
  TRY(pk_scan(den, den, n, true, true, false, R.st, s));   // S_i = prod_{j>=i} den_j
  const uint64_t nb = pk_scan_tmp_elems(n) - 1;
  const Fr dtot = d2h_fr(R.st + nb, s);                    // prod of all den_j
  TRY(pk_mul3(num, den, fe_inv(dtot), P->z_lag.as<Fr>(), n, s));
  Fr* zc = R.zc;
  TRY(ntt_run(key->dom, P->z_lag.as<Fr>(), zc, n, -1, 0, R.nsc, s, 1));
  {
    BlindArgs b{};
    b.count = 3;
    for (int i = 0; i < 3; ++i) b.r[i] = R.rng.fr();  // randomness: z's three, after the wires'
    TRY(pk_blind(zc, n, b, s));
  }
  // z's coefficients n-4 .. n+2. Stream order: queued before z's commit, complete behind its
  // read-back
  if (R.top4)
    PLK_HIP_TRY(hipMemcpyAsync(P->pin_top.as<Fr>() + 4 * kTop, zc + (n + 3 - kTop),
                               kTop * sizeof(Fr), hipMemcpyDeviceToHost, s));
  TRY(prover_commit(P, {zc}, {n + 3}, R.com + PC_Z, nullptr));
  R.tr.append_commitment("z", R.com[PC_Z]);
  return PLK_OK;
}

// PI's coefficients, where the path has any: queued before z's and the wires' block transforms
int pi_coefficients(ProofRun& R, PiPath path) {
  plk_prover* P = R.P;
  plk_key* key = R.key;
  const uint64_t n = R.n;
  const auto& pis = R.pis;
  if (path == PI_DIRECT) {
    PiDirect pd{};
    pd.count = (uint32_t)pis.size();
    for (size_t i = 0; i < pis.size(); ++i) {
      pd.idx[i] = pis[i].first;
      pd.c[i] = fe_mul(pis[i].second, key->dom->n_inv);
    }
    TRY(pk_pi_coef(pd, key->dom->tw_inv.as<Fr>(), n, P->pi_coef.as<Fr>(), R.s));
  } else if (path == PI_TRANSFORM) {
    Fr* pil = P->pi_lag.as<Fr>();
    PLK_HIP_TRY(hipMemsetAsync(pil, 0, n * sizeof(Fr), R.s));
    for (size_t i = 0; i < pis.size(); ++i) {
      P->pin_small.as<Fr>()[i] = pis[i].second;
      PLK_HIP_TRY(hipMemcpyAsync(pil + pis[i].first, P->pin_small.as<Fr>() + i, sizeof(Fr),
                                 hipMemcpyHostToDevice, R.s));
    }
    TRY(ntt_run(key->dom, pil, P->pi_coef.as<Fr>(), n, -1, 0, R.nsc, R.s, 1));
  }
  return PLK_OK;
}

// PI over the quotient domain (at exponent +1), queued after the wires' block transforms
int pi_on_quotient_domain(ProofRun& R, PiPath path, Fr* out) {
  plk_key* key = R.key;
  if (path == PI_SPARSE) {
    PiSparse ps{};
    ps.count = (uint32_t)R.pis.size();
    for (size_t i = 0; i < R.pis.size(); ++i) {
      ps.idx[i] = (uint32_t)R.pis[i].first;
      ps.v[i] = R.pis[i].second;
    }
    return pk_pi_sparse(ps, key->l1q.as<Fr>(), key->k, R.nq, out, R.s);
  }
  if (path == PI_NONE) return PLK_OK;
  return coset_blocks_fwd(key->dom, R.P->pi_coef.as<Fr>(), out, R.n, key->coset_pi.as<Fr>(), R.QB,
                          R.nsc, R.s);
}

// round 3: quotient (prover.rs:201-287, quotient_poly.rs)
int round3_quotient(ProofRun& R) {
  plk_prover* P = R.P;
  plk_key* key = R.key;
  hipStream_t s = R.s;
  const uint64_t n = R.n, S = R.S, nq = R.nq;
  const int QB = R.QB;
  Fr* ch = R.ch;
  // transcript: alpha, then the four separation challenges
  ch[CH_ALPHA] = R.tr.challenge_scalar("alpha");
  ch[CH_RANGE] = R.tr.challenge_scalar("range separation challenge");
  ch[CH_LOGIC] = R.tr.challenge_scalar("logic separation challenge");
  ch[CH_FIXED] = R.tr.challenge_scalar("fixed base separation challenge");
  ch[CH_VAR] = R.tr.challenge_scalar("variable base separation challenge");
  // the six polynomials over the quotient domain (quotient_poly.rs:54-58,145 over g H_8n
  // there): each a batch of the QB coset blocks (prover.hpp) in one launch per pass; z and the
  // wires are longer than n and fold onto the block (ntt_run_batch)
  Fr* ev = R.ev;
  const PiPath pi = pi_path(R.pis.size());
  TRY(pi_coefficients(R, pi));
  TRY(coset_blocks_fwd(key->dom, R.zc, ev + 0 * nq, n + 3, key->coset_s.as<Fr>(), QB, R.nsc, s));
  // wire evaluations at exponent -1 and PI at +1 for k_quotient's redundant-form
  // arithmetic (QuotientArgs): scaled coset tables, no extra pass
  {  // the four wires' coset blocks as ONE batch of 4 QB (NttBatch::group: wire c, block m)
    NttBatch b;
    b.group = QB;
    b.in_stride = 0;
    b.in_group_stride = S;
    b.out_stride = n;
    b.pre = key->coset_w.as<Fr>();
    b.pre_stride = S;
    TRY(ntt_run_batch(key->dom, R.wc, ev + nq, n + 2, 1, 1, R.nsc, s, 4 * QB, b));
  }
  TRY(pi_on_quotient_domain(R, pi, ev + 5 * nq));
  QuotientArgs qa{};
  qa.z = ev;
  qa.a = ev + nq;
  qa.b = ev + 2 * nq;
  qa.c = ev + 3 * nq;
  qa.d = ev + 4 * nq;
  qa.pi = pi == PI_NONE ? nullptr : ev + 5 * nq;
  qa.l1 = key->l1q.as<Fr>();
  qa.sel = key->selq.as<Fr>();
  qa.sigma = key->sigmaq.as<Fr>();
  qa.elements = key->dom->tw_fwd.as<Fr>();
  qa.out = P->quotq.as<Fr>();
  qa.nq = nq;
  qa.log_blk = key->k;
  qa.g = key->dom->g;
  // the challenges, their powers and the exponent-scaled constants (shared with
  // plk_debug_prover_stage, debug.hip)
  quotient_constants(qa, QuotientChallenges{ch[CH_ALPHA], ch[CH_BETA], ch[CH_GAMMA], ch[CH_RANGE],
                                            ch[CH_LOGIC], ch[CH_FIXED], ch[CH_VAR]},
                     key->s_m, key->vh_inv, QB, key->has_range, key->has_logic, key->has_fixed,
                     key->has_var);
  TRY(pk_quotient(qa, s));
  Fr* tc = R.tc;
  {  // t = coset_idft over the quotient domain (quotient_poly.rs:115): the QB blocks' inverse
     // transforms (post-scaled by n^-1 s_m^-k) in place give t mod (X^n - c_m), then the
     // combine into the QB n coefficients (t has at most 4n + 7; the rest are zero)
    NttBatch b;
    b.in_stride = b.out_stride = n;
    b.post = key->icoset_q.as<Fr>();
    b.post_stride = n;
    TRY(ntt_run_batch(key->dom, P->quotq.as<Fr>(), P->quotq.as<Fr>(), n, -1, 1, R.nsc, s, QB, b));
    if (!R.top4) {
      TRY(pk_coset_combine(P->quotq.as<Fr>(), n, QB, key->comb, tc, s));
    } else {
      // t[4n .. 4n + 6] (quotient_top.hpp), then the combine that also places them. Stream order:
      // on the host after the inverse transforms are queued, while the stream runs them, and
      // before the combine
      QuotientTopIn ti = key->top_in;
      std::memcpy(ti.wire, P->pin_top.ptr, 4 * kTop * sizeof(Fr));
      std::memcpy(ti.z, P->pin_top.as<Fr>() + 4 * kTop, kTop * sizeof(Fr));
      const Top pit = top_public_inputs(P->last_pi.data(), key->pi_w.data(), R.pis.size(),
                                        key->dom->n_inv, n);
      Fr q_top[kTop];
      quotient_top(ti, pit, n, key->dom->omega, key->dom->omega_inv, ch, top_flags(key), q_top);
      QuotientPatch patch;
      quotient_patch(q_top, key->top_p, patch);
      TRY(pk_coset_combine_top(P->quotq.as<Fr>(), n, key->comb, patch, tc, s));
    }
  }
  {  // flags: have_round3 once t is queued, before the t commits can refuse
    const Fr lc[7] = {ch[CH_ALPHA], ch[CH_BETA], ch[CH_GAMMA], ch[CH_RANGE], ch[CH_LOGIC],
                      ch[CH_FIXED], ch[CH_VAR]};
    std::memcpy(P->last_ch, lc, sizeof lc);
    P->have_round3 = true;
  }
  // split into t_low, t_mid, t_high (n each) and t_4 = t[3n..] (prover.rs:252-265).
  // t_4 is t[3n..8n) in the reference (prover.rs:259) and t[3n..QB n) here. For a satisfied
  // circuit t has degree <= 4n + 6 on either domain (prover.hpp), so t_4 ends below n + 8:
  // committing at most n + 8 points changes no commitment, and the zero check of the rest
  // fails for an unsatisfied circuit (its interpolant does not vanish there, prover.hpp)
  // where the reference's commit fails (t_4 past the trimmed SRS, prover.rs:262-265) —
  // including tiny circuits whose trimmed SRS covers all of t[3n..QB n)
  // (n >= 16: t_coef holds exactly 4n + 8 coefficients, nothing is left to check here, and
  // the self-check at zeta in round 4 refuses an unsatisfied circuit)
  TRY(prover_commit(P, {tc, tc + n, tc + 2 * n, tc + 3 * n}, {n, n, n, R.t_cap - 3 * n},
                    R.com + PC_T_LOW, nullptr, n + 8));
  // its commit succeeded, so everything past the committed prefix is zero: t and t_4 end at
  // 3n + t4_len for the evaluation and the opening
  R.t4_len = std::min<uint64_t>(n + 8, std::min<uint64_t>(key->srs->n, key->n_trim));
  R.tr.append_commitment("t_low", R.com[PC_T_LOW]);
  R.tr.append_commitment("t_mid", R.com[PC_T_MID]);
  R.tr.append_commitment("t_high", R.com[PC_T_HIGH]);
  R.tr.append_commitment("t_4", R.com[PC_T_4]);
  return PLK_OK;
}

// round 4: evaluations and linearization (linearization_poly.rs:22-134)
int round4_evaluations(ProofRun& R) {
  plk_prover* P = R.P;
  plk_key* key = R.key;
  const uint64_t n = R.n, S = R.S, t_len = 3 * n + R.t4_len;
  const Fr *wc = R.wc, *qc = R.qc, *sc = R.sc;
  Fr* ch = R.ch;
  const Fr zeta = ch[CH_Z] = R.tr.challenge_scalar("z_challenge");  // transcript: after t_low..t_4
  const Fr zw = fe_mul(zeta, key->dom->omega);
  EvalBatch eb{};
  // the batch begins with the proof's 16 evaluations in plk_proof order (Eval); r's place holds
  // t(z) until r(z) is formed from the others
  const Fr* polys[EV_COUNT] = {wc, wc + S, wc + 2 * S, wc + 3 * S, wc, wc + S, wc + 3 * S,
                               qc + QARITH * n, qc + QC * n, qc + QL * n, qc + QR * n,
                               sc, sc + n, sc + 2 * n, R.tc, R.zc};
  const uint64_t lens[EV_COUNT] = {n + 2, n + 2, n + 2, n + 2, n + 2, n + 2, n + 2, n, n, n, n,
                                   n, n, n, t_len, n + 3};
  uint32_t ne = 0;
  for (int i = 0; i < EV_COUNT; ++i, ++ne) {
    eb.poly[i] = polys[i];
    eb.len[i] = lens[i];
    eb.x[i] = i == EV_A_NEXT || i == EV_B_NEXT || i == EV_D_NEXT || i == EV_PERM ? zw : zeta;
  }
  auto rterm = [&](const Fr* p, uint64_t len, int lin, int have = -1) {
    if (have < 0) {  // a new evaluation at z
      eb.poly[ne] = p;
      eb.len[ne] = len;
      eb.x[ne] = zeta;
      have = (int)ne++;
    }
    R.rt.push_back(RTerm{p, len, have, lin});
  };
  rterm(qc + QM * n, n, KC_QM);
  rterm(qc + QL * n, n, KC_QL, EV_Q_L);
  rterm(qc + QR * n, n, KC_QR, EV_Q_R);
  rterm(qc + QO * n, n, KC_QO);
  rterm(qc + Q4 * n, n, KC_Q4);
  rterm(qc + QC * n, n, KC_QC, EV_Q_C);
  if (key->has_range) rterm(qc + QRANGE * n, n, KC_QRANGE);
  if (key->has_logic) rterm(qc + QLOGIC * n, n, KC_QLOGIC);
  if (key->has_fixed) rterm(qc + QFIXED * n, n, KC_QFIXED);
  if (key->has_var) rterm(qc + QVAR * n, n, KC_QVAR);
  rterm(R.zc, n + 3, LIN_Z);
  rterm(sc + 3 * n, n, KC_S4);
  // the evaluations land in host memory (no copy dispatch): read once the stream is done
  TRY(pk_eval(eb, ne, t_len, P->eval_partial.as<Fr>(), static_cast<Fr*>(P->eval_dev), R.s));
  Fr* evs = R.evs;
  PLK_HIP_TRY(stream_wait(R.s));
  std::memcpy(evs, P->eval_out.ptr, ne * sizeof(Fr));
  R.t_eval = evs[EV_R];
  // the scalars s_t of r(X) = arithmetic::linearize + range::linearize + ... + permutation,
  // those of the terms this key has, in the terms' order
  (void)at_z(zeta, key->k, key->dom->n_inv, fe_one<FrCfg>(), R.at);  // z^n and L1(z)
  Fr lin[LIN_Z + 1];
  linearisation_scalars(evs, ch, R.at.l1, edwards_d(), [&](int t, const Fr& v) { lin[t] = v; });
  for (const RTerm& t : R.rt) R.rs.push_back(lin[t.lin]);
  Fr r_e = fe_zero<FrCfg>();  // r(z) = sum_t s_t p_t(z)
  for (size_t t = 0; t < R.rt.size(); ++t) r_e = fe_add(r_e, fe_mul(R.rs[t], evs[R.rt[t].ev]));
  evs[EV_R] = r_e;  // evs[0 .. EV_COUNT) are the proof's evaluations from here on
  {  // The self-check at zeta (prover.hpp): the quotient value a verifier derives from these
     // evaluations against t(zeta) from the prover's own coefficients. They differ exactly when
     // t Z_H is not the numerator, an unsatisfied circuit (up to ~5n / |Fr| over zeta).
     // Flags: the refusal leaves have_round3 and the witness in place for plk_prover_diagnose
    Fr zn_v, l1_v, t_v;
    const bool ok = proof_at_z(evs, ch, zeta, key->k, key->dom->n_inv, P->last_pi.data(),
                               key->pi_winv.data(), (uint32_t)R.pis.size(), zn_v, l1_v, t_v);
    if (ok && !fe_eq(t_v, R.t_eval)) return PLK_E_DEGREE;
  }
  for (const Step& st : kScript)  // transcript: the evaluations in kScript's order
    if (st.kind == STEP_EVAL) R.tr.append_scalar(st.label, evs[st.id]);
    else if (st.kind == STEP_T_EVAL) R.tr.append_scalar(st.label, R.t_eval);
  return PLK_OK;
}

// round 5: openings (prover.rs:407-452)
int round5_openings(ProofRun& R) {
  plk_prover* P = R.P;
  hipStream_t s = R.s;
  const uint64_t n = R.n, S = R.S, t4_len = R.t4_len;
  const Fr *wc = R.wc, *sc = R.sc, *tc = R.tc, *zc = R.zc;
  const Fr one = fe_one<FrCfg>(), zeta = R.ch[CH_Z];
  // transcript: both v challenges precede both opening commits
  const Fr v1 = R.tr.challenge_scalar("v_challenge");
  const Fr v2 = R.tr.challenge_scalar("v_challenge");
  const Fr zn = R.at.zn, z2n = fe_sqr(zn), z3n = fe_mul(z2n, zn);
  // W(X) = (sum v1^i p_i(X)) / (X - z), p = [quot, r, a, b, c, d, s1, s2, s3]
  // with quot = t_low + z^n t_mid + z^2n t_high + z^3n t_4 and r = sum_t s_t p_t expanded
  // in place (scalars v1 s_t)
  LinComb la{}, lb{};
  auto lt = [](LinComb& lc, const Fr* p, uint64_t len, const Fr& sc_) {
    lc.p[lc.terms] = p;
    lc.len[lc.terms] = len;
    lc.s[lc.terms] = sc_;
    ++lc.terms;
  };
  if (4 + R.rt.size() + 7 > (size_t)kMaxTerms) return PLK_E_DEVICE;
  // the aggregate and its quotient by (X - z) stop where t_4 does (same polynomials,
  // same commits)
  const uint64_t agg_len = std::max<uint64_t>(n + 3, t4_len);
  lt(la, tc, n, one);
  lt(la, tc + n, n, zn);
  lt(la, tc + 2 * n, n, z2n);
  lt(la, tc + 3 * n, t4_len, z3n);
  Fr vp = v1;
  for (size_t t = 0; t < R.rt.size(); ++t) lt(la, R.rt[t].p, R.rt[t].len, fe_mul(vp, R.rs[t]));
  for (int c = 0; c < 4; ++c) {
    vp = fe_mul(vp, v1);
    lt(la, wc + c * S, n + 2, vp);
  }
  for (int c = 0; c < 3; ++c) {
    vp = fe_mul(vp, v1);
    lt(la, sc + c * n, n, vp);
  }
  Fr* ag = P->agg.as<Fr>();
  TRY(pk_lincomb(la, ag, agg_len, s));
  Fr* w1 = P->w_coef.as<Fr>();
  Fr* w2 = w1 + 5 * n;
  TRY(pk_ruffini(ag, agg_len, zeta, w1, P->tmp_a.as<Fr>(), R.st, s));
  // W'(X) = (z + v2 a + v2^2 b + v2^3 d) / (X - z w)
  const Fr v2_2 = fe_sqr(v2);
  lt(lb, zc, n + 3, one);
  lt(lb, wc, n + 2, v2);
  lt(lb, wc + S, n + 2, v2_2);
  lt(lb, wc + 3 * S, n + 2, fe_mul(v2_2, v2));
  Fr* ag2 = P->agg2.as<Fr>();
  TRY(pk_lincomb(lb, ag2, n + 3, s));
  TRY(pk_ruffini(ag2, n + 3, fe_mul(zeta, R.key->dom->omega), w2, P->tmp_a.as<Fr>(), R.st, s));
  return prover_commit(P, {w1, w2}, {agg_len - 1, n + 2}, R.com + PC_W_Z, nullptr);
}

// proof (proof.rs:36-66)
void write_proof(const ProofRun& R, plk_proof* proof) {
  plk_g1* pc = &proof->a_comm;  // ProofComm and Eval are plk_proof's order (protocol.hpp)
  for (int i = 0; i < PC_COUNT; ++i) pc[i] = R.com[i];
  plk_fr* pev = &proof->a_eval;
  for (int i = 0; i < EV_COUNT; ++i) pev[i] = fr_to_abi(R.evs[i]);
}

}  // namespace

extern "C" {

int plk_prover_create(plk_key* key, plk_prover** out) {
  PLK_API_BEGIN
    if (!key || !out) return PLK_E_ARG;
    *out = nullptr;
    DeviceGuard guard(key->ctx->device);
    std::unique_ptr<plk_prover> p(new plk_prover());
    p->key = key;
    p->ws = msm_workspace_new();
    // a lane shares the chip with other lanes' proofs: the reduction trees' form by circuit
    // size (msm_common.hpp lane_tail_policy, with the measured rows)
    if (!p->ws->tail_forced) p->ws->tail_quad = lane_tail_policy(key->n);
    p->ws->shared_chip = true;
    PLK_HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    p->own_stream = true;
    *out = p.release();
    return PLK_OK;
  PLK_API_END
}

int plk_prover_destroy(plk_prover* p) {
  if (!p) return PLK_E_ARG;
  DeviceGuard g(p->key->ctx->device);
  (void)stream_wait(p->stream);
  delete p;
  return PLK_OK;
}

int plk_prover_stream(plk_prover* p, void** stream_out) {
  if (!p || !stream_out) return PLK_E_ARG;
  *stream_out = p->stream;
  return PLK_OK;
}

int plk_prover_msm_stats(plk_prover* p, int reset, double* accumulate_ms, uint64_t* launches,
                         uint64_t* point_adds, uint64_t* points) {
  if (!p) return PLK_E_ARG;
  MsmStats& st = msm_workspace_stats(*p->ws);
  if (accumulate_ms) *accumulate_ms = st.cum_accumulate_ms;
  if (launches) *launches = st.cum_launches;
  if (point_adds) *point_adds = st.cum_point_adds;
  if (points) *points = st.cum_points;
  if (reset) st.reset_cum();
  return PLK_OK;
}

int plk_prover_shard(plk_prover* p, plk_srs* slice, uint64_t slice_start, int rank, int world,
                     plk_allgather_fn allgather, void* user) {
  if (!p || world < 1 || rank < 0 || rank >= world) return PLK_E_ARG;
  // world 1 with a slice and an all-gather still takes the exchange path (one slice covering
  // the SRS, one rank's partials exchanged): the whole sharded code path on one GPU. World 1
  // without them is the unsharded prover.
  const bool sharded = world > 1 || (slice && allgather);
  if (sharded && (!slice || !allgather || slice->ctx->device != p->key->ctx->device))
    return PLK_E_ARG;
  p->shard = sharded ? slice : nullptr;
  p->shard_lo = sharded ? slice_start : 0;
  p->shard_buckets = false;
  p->rank = rank;
  p->world = world;
  p->allgather = sharded ? allgather : nullptr;
  p->allgather_user = user;
  return PLK_OK;
}

int plk_prover_shard_buckets(plk_prover* p, int rank, int world, plk_allgather_fn allgather,
                             void* user) {
  if (!p || !allgather || world < 1 || rank < 0 || rank >= world) return PLK_E_ARG;
  // msm_run_batch's part conditions (a power of two; a wide bucket set, c >= 17, with >= 2^14
  // buckets per part); otherwise the caller keeps SRS slices (parallel.shard_prover_lane
  // mode "auto")
  if (!msm_parts_ok(p->key->srs, (uint32_t)world)) return PLK_E_ARG;
  p->shard = nullptr;
  p->shard_lo = 0;
  p->shard_buckets = true;
  p->rank = rank;
  p->world = world;
  p->allgather = allgather;
  p->allgather_user = user;
  return PLK_OK;
}

int plk_prove(plk_key* key, const plk_composer* cs, uint64_t seed, plk_proof* proof,
              plk_fr* public_inputs, size_t pi_cap, size_t* pi_count) {
  PLK_API_BEGIN
  if (!key) return PLK_E_ARG;
  // the default prover's scratch, workspace and stream serve one proof at a time: concurrent
  // plk_prove calls on one key run one after the other (plk_prover_create gives parallel lanes)
  std::lock_guard<std::mutex> lk(key->def_mu);
  if (!key->def_prover) {
    std::unique_ptr<plk_prover> d(new plk_prover());
    d->key = key;
    d->ws = msm_workspace_new();
    d->stream = key->ctx->stream;  // the context's stream, not owned
    key->def_prover = std::move(d);
  }
  return plk_prover_prove(key->def_prover.get(), cs, seed, proof, public_inputs, pi_cap, pi_count);
  PLK_API_END
}

// Every launch and async copy of a proof is issued on P->stream in the order of the steps below
// and, within a step, of its lines; a status other than PLK_OK from any step is the call's.
int plk_prover_prove(plk_prover* P, const plk_composer* cs, uint64_t seed, plk_proof* proof,
                     plk_fr* public_inputs, size_t pi_cap, size_t* pi_count) {
  PLK_API_BEGIN
    if (!P) return PLK_E_ARG;
    P->have_witness = false;  // plk_prover_diagnose: a refused call leaves no witness to check
    P->have_round3 = false;
    if (!cs || !proof) return PLK_E_ARG;
    plk_key* key = P->key;
    // the proving circuit must have the key's structure (prover.rs:114-119 gathers the
    // wires of this circuit; the key's gather indices stand for them)
    if (cs->gates.size() != key->m || cs->struct_hash != key->struct_hash) return PLK_E_ARG;
    if (cs->witness.size() <= key->max_wire) return PLK_E_ARG;
    DeviceGuard guard(key->ctx->device);
    ProofRun R(P, cs, seed);
    TRY(reserve_scratch(R));  // a failed allocation refuses before any work is queued
    // transcript: the public inputs first (prover.rs:90-105)
    for (auto& p : R.pis) R.tr.append_scalar("pi", p.second);
    if (pi_count) *pi_count = R.pis.size();
    if (public_inputs)
      for (size_t i = 0; i < R.pis.size() && i < pi_cap; ++i) public_inputs[i] = fr_to_abi(R.pis[i].second);
    TRY(upload_witness(R));  // flags: have_witness from here on
    TRY(round1_wires(R));
    TRY(round2_permutation(R));
    TRY(round3_quotient(R));  // flags: have_round3, last_ch
    TRY(round4_evaluations(R));  // PLK_E_DEGREE from the self-check at zeta
    TRY(round5_openings(R));  // PLK_E_DEVICE past kMaxTerms
    write_proof(R, proof);
    return PLK_OK;
  PLK_API_END
}

int plk_prover_commit_info(const plk_prover* p, int basis[4], uint64_t entries[4]) {
  if (!p) return PLK_E_ARG;
  for (int c = 0; c < 4; ++c) {
    if (basis) basis[c] = p->commit_basis[c];
    if (entries) entries[c] = p->commit_entries[c];
  }
  return PLK_OK;
}

}  // extern "C"

plk_prover::~plk_prover() {
  if (own_stream && stream) (void)hipStreamDestroy(stream);
  plk::msm_workspace_delete(ws);
  plk::check_ws_delete(check_ws);
}
