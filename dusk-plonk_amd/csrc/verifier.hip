// verifier.hip — Verifier::new and everything of Verifier::verify up to the pairing
// (/root/reference/src/verifier.rs:25-81, src/prover/proof.rs:70-591,
// commitment_scheme.rs:24-152), batched over many proofs of one circuit.
//
// One proof's check is e(C, H) == e(W, [tau]H) with C and W linear combinations of the 15 key
// commitments, the generator and the proof's 11 commitments. Any number of proofs fold into
// one such pair with random weights rho_j: (sum_j rho_j C_j, sum_j rho_j W_j).
// The protocol itself — the transcript's order, t_eval and the scalars of the linearisation — is
// stated in protocol.hpp; this file walks it.
//  1. Host: the merlin replay of every proof (transcript.hpp over protocol.hpp's kScript), spread
//     over up to 16 threads. t_eval is absorbed in mid-replay, so the host computes it
//     (proof_at_z: Z_H(z), L_1(z) and the barycentric PI(z) with one inversion per proof).
//  2. GPU, k_fold_scalars: one lane per proof expands C_j and W_j into scalars on the points
//     — t_comm, r_comm, both AggregateProof::flatten sums and the u batching flattened, so no
//     intermediate point is formed. k_fold_shared sums the 16 shared scalars (key commitments
//     and generator) over the proofs.
//  3. GPU: both sums as one variable-base MSM batch (msm_var.hip) over 16 + 11 count and
//     2 count points.
// The fold's pair goes to the pairing check of pairing.hip (plk_verifier_verify), or to the
// caller's own pairing library.
//
// Per-proof verdicts (plk_verifier_pairs, plk_verifier_verify_each): k_proof_pairs forms every
// proof's OWN pair (C_j, W_j) from the scalars of step 2 at rho = 1 — half a wave per proof, one
// point and scalar per lane, a 255-bit double-and-add and a segmented shuffle tree — and the
// batched pairing kernel checks the pairs where they lie.
//
// Device replay (plk_verifier_set_replay, PLK_REPLAY_DEVICE): step 1 runs on the GPU as well
// (verifier_replay.hip). The host keeps the canonical-form checks, the uploads and, for random
// weights, one sequential hash over the batch's u challenges (fold_device below).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "internal.hpp"
#include "msm_common.hpp"
#include "transcript.hpp"
#include "verifier_replay.hpp"

using namespace plk;

namespace plk {
namespace {

constexpr int kShared = KC_COUNT + 1;  // 15 key commitments + the generator
constexpr int kGenerator = KC_COUNT;
constexpr int kPerProof = PC_COUNT;

struct FoldConst {
  Fr omega, ed;  // the domain generator; edwards_d()
};

// The scalars of rho (C_j, W_j) on the points (tests/verifier_pair.py states the same algebra):
// shared[KC_*] on the key commitments, shared[kGenerator] on the generator, pr[PC_*] on the
// proof's commitments, ws[0..1] on (w_z_chall_comm, w_z_chall_w_comm) for W.
PLK_HD void fold_scalars(const FoldIn& in, const FoldConst& k, Fr* shared, size_t shared_stride,
                        Fr* pr, Fr* ws) {
#define M fe_mul
#define A fe_add
  const Fr &z = in.ch[CH_Z], &va = in.ch[CH_VA], &vb = in.ch[CH_VB], &u = in.ch[CH_U];
  const Fr* e = in.ev;
  // every scalar leaves through these, times the proof's weight
  auto SH = [&](int i, const Fr& val) { shared[(size_t)i * shared_stride] = fe_mul(val, in.rho); };
  auto PR = [&](int i, const Fr& val) { pr[i] = fe_mul(val, in.rho); };
  // r_comm (proof.rs:459-527), every term times va (its place in the aggregate): on the key
  // commitments, but for z's scalar, which joins z_comm's below
  Fr zc;
  linearisation_scalars(e, in.ch, in.l1, k.ed, [&](int term, const Fr& val) {
    if (term == LIN_Z)
      zc = val;
    else
      SH(term, M(va, val));
  });
  const Fr va2 = M(va, va), va3 = M(va2, va), va4 = M(va2, va2), va5 = M(va4, va), va6 = M(va3, va3),
           va7 = M(va6, va), va8 = M(va4, va4);
  const Fr vb2 = M(vb, vb), vb3 = M(vb2, vb);
  SH(KC_S1, va6);
  SH(KC_S2, va7);
  SH(KC_S3, va8);
  // the evaluations of both flattened aggregates go on the generator, negated
  Fr eva = A(in.t_eval, M(va, e[EV_R]));
  eva = A(eva, M(va2, e[EV_A]));
  eva = A(eva, M(va3, e[EV_B]));
  eva = A(eva, M(va4, e[EV_C]));
  eva = A(eva, M(va5, e[EV_D]));
  eva = A(eva, M(va6, e[EV_S1]));
  eva = A(eva, M(va7, e[EV_S2]));
  eva = A(eva, M(va8, e[EV_S3]));
  Fr evb = A(e[EV_PERM], M(vb, e[EV_A_NEXT]));
  evb = A(evb, M(vb2, e[EV_B_NEXT]));
  evb = A(evb, M(vb3, e[EV_D_NEXT]));
  SH(kGenerator, fe_neg(A(eva, M(u, evb))));
  const Fr zn2 = M(in.zn, in.zn);
  PR(PC_A, A(va2, M(u, vb)));
  PR(PC_B, A(va3, M(u, vb2)));
  PR(PC_C, va4);
  PR(PC_D, A(va5, M(u, vb3)));
  PR(PC_Z, A(M(va, zc), u));
  PR(PC_T_LOW, fe_one<FrCfg>());  // t_low .. t_4: [t] = sum_i z^(i n) t_i, times va^0
  PR(PC_T_MID, in.zn);
  PR(PC_T_HIGH, zn2);
  PR(PC_T_4, M(zn2, in.zn));
  PR(PC_W_Z, z);                       // at z
  PR(PC_W_ZW, M(u, M(z, k.omega)));    // at z omega, times u
  ws[0] = in.rho;
  ws[1] = M(u, in.rho);
#undef M
#undef A
}

// scalars: [16 shared][11 per proof][2 per proof]; tmp[k * count + j] = proof j's share of
// shared scalar k
__global__ void __launch_bounds__(128) k_fold_scalars(const FoldIn* __restrict__ in, FoldConst k,
                                                      uint32_t count, Fr* __restrict__ scalars,
                                                      Fr* __restrict__ tmp) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  fold_scalars(in[j], k, tmp + j, count, scalars + kShared + (size_t)kPerProof * j,
               scalars + kShared + (size_t)kPerProof * count + 2 * (size_t)j);
}

// scalars[k] = sum_j tmp[k * count + j], k = blockIdx.x
__global__ void __launch_bounds__(256) k_fold_shared(const Fr* __restrict__ tmp, uint32_t count,
                                                     Fr* __restrict__ scalars) {
  __shared__ Fr sh[256];
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  Fr acc = fe_zero<FrCfg>();
  for (uint32_t j = t; j < count; j += 256) acc = fe_add(acc, tmp[(size_t)k * count + j]);
  sh[t] = acc;
  __syncthreads();
  for (uint32_t h = 128; h >= 1; h >>= 1) {
    if (t < h) sh[t] = fe_add(sh[t], sh[t + h]);
    __syncthreads();
  }
  if (t == 0) scalars[k] = sh[0];
}

// ---- per-proof pairs ---------------------------------------------------------------------------
constexpr int kPairLanes = 32;  // half a wave per proof
constexpr int kPairC = kShared + kPerProof;  // lanes [0, 27): the terms of C; 27, 28: of W

__device__ __forceinline__ G1xyzz xyzz_shfl_down(const G1xyzz& p, int off) {
  G1xyzz r;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    r.X.v[i] = __shfl_down(p.X.v[i], off, kPairLanes);
    r.Y.v[i] = __shfl_down(p.Y.v[i], off, kPairLanes);
    r.ZZ.v[i] = __shfl_down(p.ZZ.v[i], off, kPairLanes);
    r.ZZZ.v[i] = __shfl_down(p.ZZZ.v[i], off, kPairLanes);
  }
  return r;
}

// (C_j, W_j) of proof j = the fold of that proof alone at weight 1, as canonical affine points.
// points / scalars: the fold's layout ([16 shared][11 per proof][2 per proof]); the proof's own
// share of the 16 shared scalars is tmp[k * count + j] (k_fold_scalars at rho = 1). Lane l of the
// proof's 32: l < 16 a shared point, 16 <= l < 27 one of the proof's commitments, 27 and 28 the
// two terms of W, 29 .. 31 idle. Each lane multiplies its point by its scalar (double-and-add
// over all 256 bits, g1.hpp's complete operations: identity points, zero scalars and equal
// operands are ordinary inputs), a shuffle tree segmented at lane 27 leaves C in lane 0 and W in
// lane 27, and lane 0 brings both to affine with one shared inversion. g1.hpp's packed XYZZ is
// used, not g1r.hpp's redundant-limb form: the points stay in the ABI's Montgomery domain from
// load to store and the operations are host-and-device code the host tail of the MSM already runs.
// A point g1_load<true> refuses sets *bad (the call fails with PLK_E_ARG) and counts as the
// identity.
__global__ void __launch_bounds__(128) k_proof_pairs(const plk_g1* __restrict__ points,
                                                     const Fr* __restrict__ scalars,
                                                     const Fr* __restrict__ tmp, uint32_t count,
                                                     plk_kzg_pair* __restrict__ out,
                                                     uint32_t* __restrict__ bad) {
  const uint32_t j = (blockIdx.x * blockDim.x + threadIdx.x) / kPairLanes;
  const int l = (int)(threadIdx.x % kPairLanes);
  if (j >= count) return;  // whole lane groups leave together
  const size_t n_c = kShared + (size_t)kPerProof * count;
  G1xyzz acc = xyzz_infinity();
  if (l < kPairC + 2) {
    size_t pi, si;
    const Fr* sp = scalars;
    if (l < kShared) {
      pi = (size_t)l;
      sp = tmp;
      si = (size_t)l * count + j;
    } else if (l < kPairC) {
      pi = si = kShared + (size_t)kPerProof * j + (size_t)(l - kShared);
    } else {
      pi = si = n_c + 2 * (size_t)j + (size_t)(l - kPairC);
    }
    const G1Abi p = g1_load<true>(&points[pi]);
    if (!p.ok) *bad = 1;
    Fr s = fe_from_mont(sp[si]);
    if (!p.inf && p.ok) {
#pragma nounroll
      for (int i = 0; i < 256; ++i) {
        acc = xyzz_dbl(acc);
        const uint32_t top = s.v[7] >> 31;
#pragma unroll
        for (int k = 7; k > 0; --k) s.v[k] = (s.v[k] << 1) | (s.v[k - 1] >> 31);
        s.v[0] <<= 1;
        if (top) acc = xyzz_add_affine(acc, p.x, p.y);
      }
    }
  }
  // lane l takes lane l + off's partial sum while both lie in one segment ([0, 27) or [27, 29)):
  // after the last round lane 0 holds C and lane 27 holds W
#pragma nounroll
  for (int off = 1; off < kPairLanes; off <<= 1) {
    const G1xyzz other = xyzz_shfl_down(acc, off);
    const int src = l + off;
    if (src < kPairC + 2 && (l < kPairC) == (src < kPairC)) acc = xyzz_add(acc, other);
  }
  const G1xyzz w = xyzz_shfl_down(acc, kPairC);  // lane 0 reads lane 27
  if (l != 0) return;
  const bool fc = !xyzz_is_inf(acc), fw = !xyzz_is_inf(w);
  const Fp zc = fc ? acc.ZZZ : fe_one<FpCfg>(), zw = fw ? w.ZZZ : fe_one<FpCfg>();
  const Fp inv = fe_inv(fe_mul(zc, zw));
  const Fp ic = fe_mul(inv, zw), iw = fe_mul(inv, zc);  // 1 / ZZZ; 1 / ZZ = (ZZ / ZZZ)^2
  g1_store(fe_mul(acc.X, fe_sqr(fe_mul(acc.ZZ, ic))), fe_mul(acc.Y, ic), fc, &out[j].c);
  g1_store(fe_mul(w.X, fe_sqr(fe_mul(w.ZZ, iw))), fe_mul(w.Y, iw), fw, &out[j].w);
}

}  // namespace
}  // namespace plk

struct plk_verifier {
  std::string label;
  uint64_t n = 0, m = 0;
  uint32_t log_n = 0;
  plk_g1 comms[15];
  std::vector<uint64_t> pi_idx;
  std::vector<Fr> pi_winv;  // omega^-index per public input
  Fr omega, n_inv;
  FoldConst consts;
  Transcript base{""};  // Transcript::base(label, vk, m): what every proof's replay starts from
  double replay_ms = 0.0;
  float gpu_ms = 0.f;
  // fold buffers (device), kept between calls
  DevBuf d_points, d_scalars, d_in, d_tmp;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int device = -1;
  // device replay: the mode, the compiled schedule (made on first use) and its buffers
  int replay_mode = PLK_REPLAY_HOST;
  float replay_kernel_ms = 0.f;
  bool plan_ready = false, plan_on_device = false;
  ReplayPlan plan;
  DevBuf d_sched, d_winv, d_evals, d_pi, d_weights, d_vals, d_u, d_status, d_rho_sched;
  hipEvent_t e2 = nullptr, e3 = nullptr;
  // per-proof pairs (plk_verifier_pairs / plk_verifier_verify_each)
  DevBuf d_pairs, d_pair_bad, d_ok;
  hipEvent_t e4 = nullptr, e5 = nullptr;
  float pairs_ms = 0.f, pairing_ms = 0.f;
};

namespace plk {
size_t verifier_pi_count(const plk_verifier* v) { return v->pi_idx.size(); }

namespace {

// The transcript replay of Proof::verify for one proof: the 11 challenges and what the scalar
// kernel needs besides (t_eval, L_1(z), z^n). PLK_E_ARG on a non-canonical value, z_h(z) = 0 or
// z = 1.
int replay(const plk_verifier* v, const plk_proof& p, const plk_fr* pis, FoldIn& o) {
  const plk_fr* evals = &p.a_eval;
  const plk_g1* comms = &p.a_comm;
  for (int i = 0; i < EV_COUNT; ++i) {
    if (!abi_canonical<FrCfg>(evals[i].l)) return PLK_E_ARG;
    o.ev[i] = fr_from_abi(evals[i]);
  }
  const size_t npi = v->pi_idx.size();
  std::vector<Fr> pi(npi);
  for (size_t i = 0; i < npi; ++i) {
    if (!abi_canonical<FrCfg>(pis[i].l)) return PLK_E_ARG;
    pi[i] = fr_from_abi(pis[i]);
  }
  Transcript t = v->base;
  for (const Step& st : kScript) switch (st.kind) {
      case STEP_PI:
        for (size_t i = 0; i < npi; ++i) t.append_scalar(st.label, pi[i]);
        break;
      case STEP_COMM: t.append_commitment(st.label, comms[st.id]); break;
      case STEP_CHAL:
        o.ch[st.id] = t.challenge_scalar(st.label);
        if (st.id == CH_Z &&
            !proof_at_z(o.ev, o.ch, o.ch[CH_Z], v->log_n, v->n_inv, pi.data(), v->pi_winv.data(),
                        (uint32_t)npi, o.zn, o.l1, o.t_eval))
          return PLK_E_ARG;
        break;
      case STEP_BETA: t.append_scalar(st.label, o.ch[CH_BETA]); break;
      case STEP_EVAL: t.append_scalar(st.label, o.ev[st.id]); break;
      case STEP_T_EVAL: t.append_scalar(st.label, o.t_eval); break;
    }
  o.rho = fe_one<FrCfg>();
  return PLK_OK;
}

// The G1 generator in the ABI layout
plk_g1 g1_generator_abi() {
  Fp x, y;
  g1_generator(x, y);
  plk_g1 g;
  g1_store(x, y, true, &g);
  return g;
}

// rho_0 = 1, rho_j = 128 bits of a merlin transcript over every proof's u challenge and 32 bytes
// of OS entropy: nobody who fixed the proofs beforehand knows the weights
int random_weights(std::vector<FoldIn>& in) {
  uint8_t seed[32];
  os_entropy(seed);
  Transcript t("plk-verifier-fold");
  t.append_u64("count", in.size());
  for (const FoldIn& f : in) t.append_scalar("u", f.ch[CH_U]);
  t.append_message("entropy", seed, sizeof seed);
  for (size_t j = 1; j < in.size(); ++j) {
    uint8_t b[16];
    t.challenge_bytes("rho", b, 16);
    Fr r = fe_zero<FrCfg>();
    for (int i = 0; i < 4; ++i)
      r.v[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
               ((uint32_t)b[4 * i + 3] << 24);
    in[j].rho = fe_to_mont(r);
  }
  return PLK_OK;
}

// The transcript replays of a whole batch on up to 16 host threads: in[j] for every proof, at
// rho = 1. The first failing proof's status, or PLK_OK.
int replay_host_batch(const plk_verifier* v, const plk_proof* proofs, const plk_fr* public_inputs,
                      size_t count, std::vector<FoldIn>& in) {
  const size_t npi = v->pi_idx.size();
  in.resize(count);
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const size_t nth = std::min<size_t>({16, hw, (count + 7) / 8});
  std::vector<int> status(std::max<size_t>(nth, 1), PLK_OK);
  auto work = [&](size_t th) {
    for (size_t j = th; j < count; j += std::max<size_t>(nth, 1)) {
      const int st = replay(v, proofs[j], public_inputs ? public_inputs + j * npi : nullptr, in[j]);
      if (st != PLK_OK) {
        status[th] = st;
        return;
      }
    }
  };
  if (nth <= 1) {
    work(0);
  } else {
    std::vector<std::thread> workers;
    workers.reserve(nth);
    try {
      for (size_t th = 0; th < nth; ++th) workers.emplace_back(work, th);
    } catch (...) {
      for (auto& w : workers) w.join();
      throw;
    }
    for (auto& w : workers) w.join();
  }
  for (int st : status)
    if (st != PLK_OK) return st;
  return PLK_OK;
}

// The points of a batch in the fold's layout: [15 key commitments, generator][11 per proof]
// [w_z, w_z_w per proof]
std::vector<plk_g1> batch_points(const plk_verifier* v, const plk_proof* proofs, size_t count) {
  const size_t n_c = kShared + (size_t)kPerProof * count;
  std::vector<plk_g1> pts(n_c + 2 * count);
  std::memcpy(pts.data(), v->comms, sizeof v->comms);
  pts[kGenerator] = g1_generator_abi();
  for (size_t j = 0; j < count; ++j) {
    std::memcpy(&pts[kShared + kPerProof * j], &proofs[j].a_comm, kPerProof * sizeof(plk_g1));
    pts[n_c + 2 * j] = proofs[j].w_z_chall_comm;
    pts[n_c + 2 * j + 1] = proofs[j].w_z_chall_w_comm;
  }
  return pts;
}

}  // namespace
}  // namespace plk

// ---- device replay ------------------------------------------------------------------------
namespace plk {
namespace {

// the schedule holds about a quarter of a block (1 KiB) per public input
constexpr size_t kMaxDevicePi = 1u << 16;

// Device-mode weights: the sequential part that binds the batch stays on the host — the root
// transcript over the count, every proof's u and the entropy. rho_j is then drawn from a clone
// of the root after append_u64("index", j), one lane per proof (k_fold_rho / rho_host).
void fold_weights_root(const uint8_t entropy[32], const Fr* u, size_t count, RhoPlan& plan) {
  Transcript t("plk-verifier-fold");
  t.append_u64("count", count);
  for (size_t j = 0; j < count; ++j) t.append_scalar("u", u[j]);
  t.append_message("entropy", entropy, 32);
  const Strobe128& s = t.strobe();
  rho_plan_compile(s.state(), s.pos(), s.pos_begin(), plan);
}

// The canonical-form checks of replay(), for the whole batch, before any upload.
int check_canonical(const plk_verifier* v, const plk_proof* proofs, const plk_fr* pis, size_t count) {
  const size_t npi = v->pi_idx.size();
  for (size_t j = 0; j < count; ++j) {
    const plk_fr* evals = &proofs[j].a_eval;
    for (int i = 0; i < EV_COUNT; ++i)
      if (!abi_canonical<FrCfg>(evals[i].l)) return PLK_E_ARG;
  }
  for (size_t i = 0; i < npi * count; ++i)
    if (!abi_canonical<FrCfg>(pis[i].l)) return PLK_E_ARG;
  return PLK_OK;
}

// Uploads the points (the layout of the fold's MSM), the evaluations, the public inputs and
// the weights, and queues the replay kernels on the context's stream between the events e2 and
// e3 (e0 goes before the uploads). On return d_in holds every proof's FoldIn (rho = its weight,
// or one) and d_u the u challenges, stream-ordered. The caller holds the device guard.
int replay_on_device(plk_ctx* ctx, plk_verifier* v, const plk_proof* proofs, const plk_fr* pis,
                     size_t count, const plk_fr* weights) {
  const size_t npi = v->pi_idx.size();
  if (npi > kMaxDevicePi) return PLK_E_ARG;
  hipStream_t s = ctx->stream;
  if (v->device >= 0 && v->device != ctx->device) return PLK_E_ARG;  // one GPU per verifier
  v->device = ctx->device;
  for (hipEvent_t* e : {&v->e0, &v->e1, &v->e2, &v->e3})
    if (!*e) PLK_HIP_TRY(hipEventCreate(e));
  int st;
  if (!v->plan_ready) {
    const Strobe128& b = v->base.strobe();
    replay_plan_compile(b.state(), b.pos(), b.pos_begin(), (uint32_t)npi, v->plan);
    v->plan_ready = true;
  }
  if (!v->plan_on_device) {
    if ((st = v->d_sched.alloc(v->plan.sched.size() * sizeof(uint32_t)))) return st;
    if ((st = v->d_winv.alloc(std::max<size_t>(npi, 1) * sizeof(Fr)))) return st;
    if ((st = v->d_status.alloc(sizeof(uint32_t)))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(v->d_sched.ptr, v->plan.sched.data(), v->plan.sched.size() * sizeof(uint32_t),
                               hipMemcpyHostToDevice, s));
    if (npi)
      PLK_HIP_TRY(hipMemcpyAsync(v->d_winv.ptr, v->pi_winv.data(), npi * sizeof(Fr), hipMemcpyHostToDevice, s));
    PLK_HIP_TRY(stream_wait(s));
    v->plan_on_device = true;
  }
  // the points: [15 key commitments, generator][11 per proof][w_z, w_z_w per proof]
  const size_t n_c = kShared + (size_t)kPerProof * count, n_pts = n_c + 2 * count;
  std::vector<plk_g1> pts(n_pts);
  std::memcpy(pts.data(), v->comms, sizeof v->comms);
  pts[kGenerator] = g1_generator_abi();
  std::vector<plk_fr> evals(16 * count);
  for (size_t j = 0; j < count; ++j) {
    std::memcpy(&pts[kShared + kPerProof * j], &proofs[j].a_comm, kPerProof * sizeof(plk_g1));
    pts[n_c + 2 * j] = proofs[j].w_z_chall_comm;
    pts[n_c + 2 * j + 1] = proofs[j].w_z_chall_w_comm;
    std::memcpy(&evals[16 * j], &proofs[j].a_eval, 16 * sizeof(plk_fr));
  }
  if ((st = v->d_points.alloc(n_pts * sizeof(plk_g1)))) return st;
  if ((st = v->d_scalars.alloc(n_pts * sizeof(Fr)))) return st;
  if ((st = v->d_in.alloc(count * sizeof(FoldIn)))) return st;
  if ((st = v->d_tmp.alloc((size_t)kShared * count * sizeof(Fr)))) return st;
  if ((st = v->d_evals.alloc(16 * count * sizeof(Fr)))) return st;
  if ((st = v->d_pi.alloc(std::max<size_t>(npi * count, 1) * sizeof(Fr)))) return st;
  if ((st = v->d_weights.alloc(count * sizeof(Fr)))) return st;
  if ((st = v->d_u.alloc(count * sizeof(Fr)))) return st;
  if ((st = v->d_vals.alloc((size_t)v->plan.lay.rows() * count * sizeof(uint32_t)))) return st;
  PLK_HIP_TRY(hipEventRecord(v->e0, s));
  PLK_HIP_TRY(hipMemcpyAsync(v->d_points.ptr, pts.data(), n_pts * sizeof(plk_g1), hipMemcpyHostToDevice, s));
  PLK_HIP_TRY(hipMemcpyAsync(v->d_evals.ptr, evals.data(), 16 * count * sizeof(Fr), hipMemcpyHostToDevice, s));
  if (npi)
    PLK_HIP_TRY(hipMemcpyAsync(v->d_pi.ptr, pis, npi * count * sizeof(Fr), hipMemcpyHostToDevice, s));
  if (weights)
    PLK_HIP_TRY(hipMemcpyAsync(v->d_weights.ptr, weights, count * sizeof(Fr), hipMemcpyHostToDevice, s));
  ReplayLaunch l;
  l.d_sched = v->d_sched.as<uint32_t>();
  l.blocks = v->plan.blocks;
  l.lay = v->plan.lay;
  l.base = v->plan.base;
  l.n_inv = v->n_inv;
  l.log_n = v->log_n;
  l.count = (uint32_t)count;
  l.d_comms = v->d_points.as<plk_g1>() + kShared;
  l.d_evals = v->d_evals.as<Fr>();
  l.d_pi = v->d_pi.as<Fr>();
  l.d_winv = v->d_winv.as<Fr>();
  l.d_weights = weights ? v->d_weights.as<Fr>() : nullptr;
  l.d_vals = v->d_vals.as<uint32_t>();
  l.d_in = v->d_in.as<FoldIn>();
  l.d_u = v->d_u.as<Fr>();
  l.d_status = v->d_status.as<uint32_t>();
  PLK_HIP_TRY(hipEventRecord(v->e2, s));
  if ((st = replay_launch(s, l))) return st;
  PLK_HIP_TRY(hipEventRecord(v->e3, s));
  return PLK_OK;
}

// plk_verifier_fold in device mode (the arguments are checked)
int fold_device(plk_ctx* ctx, plk_verifier* v, const plk_proof* proofs, const plk_fr* public_inputs,
                size_t count, const plk_fr* weights, plk_kzg_pair* out) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  int st;
  if ((st = check_canonical(v, proofs, public_inputs, count))) return st;
  double host_ms = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  if ((st = replay_on_device(ctx, v, proofs, public_inputs, count, weights))) return st;
  uint32_t status = 0;
  if (!weights) {
    std::vector<Fr> u(count);
    PLK_HIP_TRY(hipMemcpyAsync(u.data(), v->d_u.ptr, count * sizeof(Fr), hipMemcpyDeviceToHost, s));
    PLK_HIP_TRY(hipMemcpyAsync(&status, v->d_status.ptr, sizeof status, hipMemcpyDeviceToHost, s));
    PLK_HIP_TRY(stream_wait(s));
    if (status) return PLK_E_ARG;  // z_h(z) = 0 or z = 1 in some proof
    const auto t1 = clock::now();
    uint8_t seed[32];
    os_entropy(seed);
    RhoPlan rho;
    fold_weights_root(seed, u.data(), count, rho);
    host_ms += std::chrono::duration<double, std::milli>(clock::now() - t1).count();
    if ((st = v->d_rho_sched.alloc(rho.sched.size() * sizeof(uint32_t)))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(v->d_rho_sched.ptr, rho.sched.data(), rho.sched.size() * sizeof(uint32_t),
                               hipMemcpyHostToDevice, s));
    if ((st = rho_launch(s, rho.root, v->d_rho_sched.as<uint32_t>(), rho.blocks, (uint32_t)count,
                         &v->d_in.as<FoldIn>()->rho, (uint32_t)(sizeof(FoldIn) / sizeof(Fr)))))
      return st;
    // the schedule is read by the kernel: keep it alive until the stream has passed it
    PLK_HIP_TRY(stream_wait(s));
  }
  v->replay_ms = host_ms;
  hipLaunchKernelGGL(k_fold_scalars, dim3(cdiv(count, 128)), dim3(128), 0, s,
                     (const FoldIn*)v->d_in.as<FoldIn>(), v->consts, (uint32_t)count,
                     v->d_scalars.as<Fr>(), v->d_tmp.as<Fr>());
  hipLaunchKernelGGL(k_fold_shared, dim3(kShared), dim3(256), 0, s, (const Fr*)v->d_tmp.as<Fr>(),
                     (uint32_t)count, v->d_scalars.as<Fr>());
  PLK_HIP_TRY(hipGetLastError());
  const size_t n_c = kShared + (size_t)kPerProof * count, n_pts = n_c + 2 * count;
  const size_t starts[2] = {0, n_c}, lens[2] = {n_c, 2 * count};
  plk_g1 res[2];
  st = msm_var_run(ctx, v->d_points.as<plk_g1>(), v->d_scalars.as<Fr>(), n_pts, starts, lens, 2, res, s);
  PLK_HIP_TRY(hipEventRecord(v->e1, s));
  if (weights)
    PLK_HIP_TRY(hipMemcpyAsync(&status, v->d_status.ptr, sizeof status, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  if (st != PLK_OK) return st;
  if (status) return PLK_E_ARG;
  (void)hipEventElapsedTime(&v->gpu_ms, v->e0, v->e1);
  (void)hipEventElapsedTime(&v->replay_kernel_ms, v->e2, v->e3);
  out->c = res[0];
  out->w = res[1];
  return PLK_OK;
}

// Every proof's own pair (k_proof_pairs) into v->d_pairs, queued on the context's stream, in the
// verifier's replay mode. The caller holds the device guard, has checked the arguments, and
// reads the verdict of pairs_status once the stream has passed.
int pairs_on_device(plk_ctx* ctx, plk_verifier* v, const plk_proof* proofs, const plk_fr* public_inputs,
                    size_t count) {
  hipStream_t s = ctx->stream;
  int st;
  if ((st = check_canonical(v, proofs, public_inputs, count))) return st;
  const size_t n_c = kShared + (size_t)kPerProof * count, n_pts = n_c + 2 * count;
  if (v->replay_mode == PLK_REPLAY_DEVICE) {
    if ((st = replay_on_device(ctx, v, proofs, public_inputs, count, nullptr))) return st;  // rho = 1
  } else {
    std::vector<FoldIn> in;
    if ((st = replay_host_batch(v, proofs, public_inputs, count, in))) return st;
    const std::vector<plk_g1> pts = batch_points(v, proofs, count);
    if (v->device >= 0 && v->device != ctx->device) return PLK_E_ARG;  // one GPU per verifier
    v->device = ctx->device;
    if ((st = v->d_points.alloc(n_pts * sizeof(plk_g1)))) return st;
    if ((st = v->d_scalars.alloc(n_pts * sizeof(Fr)))) return st;
    if ((st = v->d_in.alloc(count * sizeof(FoldIn)))) return st;
    if ((st = v->d_tmp.alloc((size_t)kShared * count * sizeof(Fr)))) return st;
    if ((st = v->d_status.alloc(sizeof(uint32_t)))) return st;
    PLK_HIP_TRY(hipMemsetAsync(v->d_status.ptr, 0, sizeof(uint32_t), s));
    PLK_HIP_TRY(hipMemcpyAsync(v->d_points.ptr, pts.data(), n_pts * sizeof(plk_g1), hipMemcpyHostToDevice, s));
    PLK_HIP_TRY(hipMemcpyAsync(v->d_in.ptr, in.data(), count * sizeof(FoldIn), hipMemcpyHostToDevice, s));
    PLK_HIP_TRY(stream_wait(s));  // pts and in leave scope
  }
  if (!v->e4) PLK_HIP_TRY(hipEventCreate(&v->e4));
  if (!v->e5) PLK_HIP_TRY(hipEventCreate(&v->e5));
  if ((st = v->d_pairs.alloc(count * sizeof(plk_kzg_pair)))) return st;
  if ((st = v->d_pair_bad.alloc(sizeof(uint32_t)))) return st;
  PLK_HIP_TRY(hipMemsetAsync(v->d_pair_bad.ptr, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_fold_scalars, dim3(cdiv(count, 128)), dim3(128), 0, s,
                     (const FoldIn*)v->d_in.as<FoldIn>(), v->consts, (uint32_t)count,
                     v->d_scalars.as<Fr>(), v->d_tmp.as<Fr>());
  PLK_HIP_TRY(hipEventRecord(v->e4, s));
  hipLaunchKernelGGL(k_proof_pairs, dim3(cdiv(count * kPairLanes, 128)), dim3(128), 0, s,
                     (const plk_g1*)v->d_points.as<plk_g1>(), (const Fr*)v->d_scalars.as<Fr>(),
                     (const Fr*)v->d_tmp.as<Fr>(), (uint32_t)count, v->d_pairs.as<plk_kzg_pair>(),
                     v->d_pair_bad.as<uint32_t>());
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipEventRecord(v->e5, s));
  return PLK_OK;
}

// After the stream has passed pairs_on_device: PLK_E_ARG when a point was malformed or, in device
// mode, some proof had z_h(z) = 0 or z = 1. Takes the kernel's time.
int pairs_status(plk_ctx* ctx, plk_verifier* v) {
  uint32_t bad[2] = {0, 0};
  hipStream_t s = ctx->stream;
  PLK_HIP_TRY(hipMemcpyAsync(&bad[0], v->d_pair_bad.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(hipMemcpyAsync(&bad[1], v->d_status.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  (void)hipEventElapsedTime(&v->pairs_ms, v->e4, v->e5);
  return (bad[0] || bad[1]) ? PLK_E_ARG : PLK_OK;
}

}  // namespace
}  // namespace plk

extern "C" {

int plk_verifier_create(const char* label, uint64_t n, uint64_t m, const plk_g1 commitments[15],
                        const uint64_t* pi_indexes, size_t pi_count, plk_verifier** out) {
  PLK_API_BEGIN
  if (!out) return PLK_E_ARG;
  *out = nullptr;
  if (!label || !commitments || (pi_count && !pi_indexes)) return PLK_E_ARG;
  if (n < 2 || n > (1ull << 27) || (n & (n - 1)) || pi_count > n) return PLK_E_ARG;
  for (size_t i = 0; i < pi_count; ++i)
    if (pi_indexes[i] >= n || (i && pi_indexes[i] <= pi_indexes[i - 1])) return PLK_E_ARG;
  std::unique_ptr<plk_verifier> v(new plk_verifier());
  v->label = label;
  v->n = n;
  v->m = m;
  v->log_n = (uint32_t)__builtin_ctzll(n);
  std::memcpy(v->comms, commitments, sizeof v->comms);
  v->pi_idx.assign(pi_indexes, pi_indexes + pi_count);
  fr_root_of_unity(v->log_n, v->omega);
  const Fr winv = fe_inv(v->omega);
  v->pi_winv.resize(pi_count);
  for (size_t i = 0; i < pi_count; ++i) v->pi_winv[i] = fe_pow_u64(winv, pi_indexes[i]);
  v->n_inv = fe_inv(fr_small((uint32_t)n));
  v->consts.omega = v->omega;
  v->consts.ed = edwards_d();
  v->base = Transcript::base(v->label, v->comms, m);
  *out = v.release();
  return PLK_OK;
  PLK_API_END
}

int plk_verifier_destroy(plk_verifier* v) {
  PLK_API_BEGIN
  if (!v) return PLK_E_ARG;
  if (v->device >= 0) {
    DeviceGuard g(v->device);
    if (v->e0) (void)hipEventDestroy(v->e0);
    if (v->e1) (void)hipEventDestroy(v->e1);
    if (v->e2) (void)hipEventDestroy(v->e2);
    if (v->e3) (void)hipEventDestroy(v->e3);
    if (v->e4) (void)hipEventDestroy(v->e4);
    if (v->e5) (void)hipEventDestroy(v->e5);
    delete v;  // frees the device buffers on their device
    return PLK_OK;
  }
  delete v;
  return PLK_OK;
  PLK_API_END
}

int plk_verifier_challenges(const plk_verifier* v, const plk_proof* proof, const plk_fr* public_inputs,
                            plk_fr out[11]) {
  PLK_API_BEGIN
  if (!v || !proof || !out || (!public_inputs && !v->pi_idx.empty())) return PLK_E_ARG;
  FoldIn in;
  const int st = replay(v, *proof, public_inputs, in);
  if (st != PLK_OK) return st;
  for (int i = 0; i < CH_COUNT; ++i) out[i] = fr_to_abi(in.ch[i]);
  return PLK_OK;
  PLK_API_END
}

int plk_verifier_fold(plk_ctx* ctx, plk_verifier* v, const plk_proof* proofs,
                      const plk_fr* public_inputs, size_t count, const plk_fr* weights,
                      plk_kzg_pair* out) {
  PLK_API_BEGIN
  if (!ctx || !v || !proofs || !out || count == 0 || count > (1u << 24)) return PLK_E_ARG;
  const size_t npi = v->pi_idx.size();
  if (npi && !public_inputs) return PLK_E_ARG;
  if (weights)
    for (size_t j = 0; j < count; ++j)
      if (!abi_canonical<FrCfg>(weights[j].l)) return PLK_E_ARG;
  if (v->replay_mode == PLK_REPLAY_DEVICE)
    return fold_device(ctx, v, proofs, public_inputs, count, weights, out);
  v->replay_kernel_ms = 0.f;
  // 1. the transcript replays, on up to 16 host threads
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<FoldIn> in;
  {
    const int rst = replay_host_batch(v, proofs, public_inputs, count, in);
    if (rst != PLK_OK) return rst;
  }
  if (weights) {
    for (size_t j = 0; j < count; ++j) in[j].rho = fr_from_abi(weights[j]);
  } else {
    random_weights(in);
  }
  v->replay_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  // 2. the points: [15 key commitments, generator][11 per proof][w_z, w_z_w per proof]
  const size_t n_c = kShared + (size_t)kPerProof * count, n_pts = n_c + 2 * count;
  const std::vector<plk_g1> pts = batch_points(v, proofs, count);
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  if (v->device >= 0 && v->device != ctx->device) return PLK_E_ARG;  // one GPU per verifier
  v->device = ctx->device;
  if (!v->e0) PLK_HIP_TRY(hipEventCreate(&v->e0));
  if (!v->e1) PLK_HIP_TRY(hipEventCreate(&v->e1));
  int st;
  if ((st = v->d_points.alloc(n_pts * sizeof(plk_g1)))) return st;
  if ((st = v->d_scalars.alloc(n_pts * sizeof(Fr)))) return st;
  if ((st = v->d_in.alloc(count * sizeof(FoldIn)))) return st;
  if ((st = v->d_tmp.alloc((size_t)kShared * count * sizeof(Fr)))) return st;
  PLK_HIP_TRY(hipEventRecord(v->e0, s));
  PLK_HIP_TRY(hipMemcpyAsync(v->d_points.ptr, pts.data(), n_pts * sizeof(plk_g1), hipMemcpyHostToDevice, s));
  PLK_HIP_TRY(hipMemcpyAsync(v->d_in.ptr, in.data(), count * sizeof(FoldIn), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_fold_scalars, dim3(cdiv(count, 128)), dim3(128), 0, s,
                     (const FoldIn*)v->d_in.as<FoldIn>(), v->consts, (uint32_t)count,
                     v->d_scalars.as<Fr>(), v->d_tmp.as<Fr>());
  hipLaunchKernelGGL(k_fold_shared, dim3(kShared), dim3(256), 0, s, (const Fr*)v->d_tmp.as<Fr>(),
                     (uint32_t)count, v->d_scalars.as<Fr>());
  PLK_HIP_TRY(hipGetLastError());
  // 3. both sums as one variable-base MSM batch
  const size_t starts[2] = {0, n_c}, lens[2] = {n_c, 2 * count};
  plk_g1 res[2];
  st = msm_var_run(ctx, v->d_points.as<plk_g1>(), v->d_scalars.as<Fr>(), n_pts, starts, lens, 2, res, s);
  PLK_HIP_TRY(hipEventRecord(v->e1, s));
  PLK_HIP_TRY(stream_wait(s));
  if (st != PLK_OK) return st;
  (void)hipEventElapsedTime(&v->gpu_ms, v->e0, v->e1);
  out->c = res[0];
  out->w = res[1];
  return PLK_OK;
  PLK_API_END
}

int plk_verifier_pairs(plk_ctx* ctx, plk_verifier* v, const plk_proof* proofs,
                       const plk_fr* public_inputs, size_t count, plk_kzg_pair* out) {
  PLK_API_BEGIN
  if (!ctx || !v || !proofs || !out || count == 0 || count > (1u << 24)) return PLK_E_ARG;
  if (!public_inputs && !v->pi_idx.empty()) return PLK_E_ARG;
  DeviceGuard g(ctx->device);
  int st;
  if ((st = pairs_on_device(ctx, v, proofs, public_inputs, count))) return st;
  std::vector<plk_kzg_pair> res(count);
  PLK_HIP_TRY(hipMemcpyAsync(res.data(), v->d_pairs.ptr, count * sizeof(plk_kzg_pair), hipMemcpyDeviceToHost,
                             ctx->stream));
  if ((st = pairs_status(ctx, v))) return st;
  v->pairing_ms = 0.f;
  std::memcpy(out, res.data(), count * sizeof(plk_kzg_pair));
  return PLK_OK;
  PLK_API_END
}

int plk_verifier_verify(plk_ctx* ctx, plk_verifier* v, const plk_opening_key* key,
                        const plk_proof* proofs, const plk_fr* public_inputs, size_t count,
                        const plk_fr* weights, int* ok) {
  if (!key || !ok) return PLK_E_ARG;
  plk_kzg_pair pair;
  const int st = plk_verifier_fold(ctx, v, proofs, public_inputs, count, weights, &pair);
  if (st != PLK_OK) return st;
  return plk_pairing_check(key, &pair, ok);
}

int plk_verifier_verify_each(plk_ctx* ctx, plk_verifier* v, plk_opening_key* key,
                             const plk_proof* proofs, const plk_fr* public_inputs, size_t count,
                             uint8_t* ok) {
  PLK_API_BEGIN
  if (!ctx || !v || !key || !proofs || !ok || count == 0 || count > (1u << 24)) return PLK_E_ARG;
  if (!public_inputs && !v->pi_idx.empty()) return PLK_E_ARG;
  DeviceGuard g(ctx->device);
  int st;
  if ((st = pairs_on_device(ctx, v, proofs, public_inputs, count))) return st;
  if ((st = v->d_ok.alloc(count))) return st;
  // a malformed point counts as the identity in k_proof_pairs, so the pairs are well-formed
  // points whatever pairs_status says afterwards
  if ((st = pairing_check_dev(ctx, key, v->d_pairs.as<plk_kzg_pair>(), count, v->d_ok.as<uint8_t>())))
    return st;
  std::vector<uint8_t> res(count);
  PLK_HIP_TRY(hipMemcpyAsync(res.data(), v->d_ok.ptr, count, hipMemcpyDeviceToHost, ctx->stream));
  if ((st = pairs_status(ctx, v))) return st;
  pairing_last_ms(key, &v->pairing_ms);
  std::memcpy(ok, res.data(), count);
  return PLK_OK;
  PLK_API_END
}

int plk_verifier_last_each_stats(const plk_verifier* v, float* pairs_ms, float* pairing_ms) {
  if (!v) return PLK_E_ARG;
  if (pairs_ms) *pairs_ms = v->pairs_ms;
  if (pairing_ms) *pairing_ms = v->pairing_ms;
  return PLK_OK;
}

int plk_verifier_set_replay(plk_verifier* v, int mode) {
  if (!v || (mode != PLK_REPLAY_HOST && mode != PLK_REPLAY_DEVICE)) return PLK_E_ARG;
  v->replay_mode = mode;
  return PLK_OK;
}

int plk_verifier_challenges_batch(plk_ctx* ctx, plk_verifier* v, const plk_proof* proofs,
                                  const plk_fr* public_inputs, size_t count, plk_fr* out) {
  PLK_API_BEGIN
  if (!ctx || !v || !proofs || !out || count == 0 || count > (1u << 24)) return PLK_E_ARG;
  if (!public_inputs && !v->pi_idx.empty()) return PLK_E_ARG;
  int st;
  if ((st = check_canonical(v, proofs, public_inputs, count))) return st;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  if ((st = replay_on_device(ctx, v, proofs, public_inputs, count, nullptr))) return st;
  std::vector<FoldIn> in(count);
  uint32_t status = 0;
  PLK_HIP_TRY(hipMemcpyAsync(in.data(), v->d_in.ptr, count * sizeof(FoldIn), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(hipMemcpyAsync(&status, v->d_status.ptr, sizeof status, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  (void)hipEventElapsedTime(&v->replay_kernel_ms, v->e2, v->e3);
  if (status) return PLK_E_ARG;  // z_h(z) = 0 or z = 1 in some proof
  for (size_t j = 0; j < count; ++j)
    for (int i = 0; i < CH_COUNT; ++i) out[CH_COUNT * j + i] = fr_to_abi(in[j].ch[i]);
  return PLK_OK;
  PLK_API_END
}

int plk_verifier_last_replay_ms(const plk_verifier* v, float* kernel_ms) {
  if (!v || !kernel_ms) return PLK_E_ARG;
  *kernel_ms = v->replay_kernel_ms;
  return PLK_OK;
}

int plk_debug_fold_weights(plk_ctx* ctx, const uint8_t entropy[32], const plk_fr* u, size_t count,
                           plk_fr* out) {
  PLK_API_BEGIN
  if (!entropy || !u || !out || count == 0 || count > (1u << 24)) return PLK_E_ARG;
  std::vector<Fr> um(count);
  for (size_t j = 0; j < count; ++j) {
    if (!abi_canonical<FrCfg>(u[j].l)) return PLK_E_ARG;
    um[j] = fr_from_abi(u[j]);
  }
  RhoPlan rho;
  fold_weights_root(entropy, um.data(), count, rho);
  if (!ctx) {
    for (size_t j = 0; j < count; ++j) out[j] = fr_to_abi(rho_host(rho, (uint32_t)j));
    return PLK_OK;
  }
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  DevBuf d_sched, d_out;
  int st;
  if ((st = d_sched.alloc(rho.sched.size() * sizeof(uint32_t)))) return st;
  if ((st = d_out.alloc(count * sizeof(Fr)))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(d_sched.ptr, rho.sched.data(), rho.sched.size() * sizeof(uint32_t),
                             hipMemcpyHostToDevice, s));
  if ((st = rho_launch(s, rho.root, d_sched.as<uint32_t>(), rho.blocks, (uint32_t)count, d_out.as<Fr>(), 1)))
    return st;
  PLK_HIP_TRY(hipMemcpyAsync(um.data(), d_out.ptr, count * sizeof(Fr), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  for (size_t j = 0; j < count; ++j) out[j] = fr_to_abi(um[j]);
  return PLK_OK;
  PLK_API_END
}

int plk_verifier_last_fold_stats(const plk_verifier* v, double* replay_ms, float* gpu_ms) {
  if (!v) return PLK_E_ARG;
  if (replay_ms) *replay_ms = v->replay_ms;
  if (gpu_ms) *gpu_ms = v->gpu_ms;
  return PLK_OK;
}

}  // extern "C"
