// verifier_replay.hip — the merlin replay of Proof::verify (protocol.hpp's kScript, which
// verifier.hip replay() walks on the host) for a batch of proofs of one circuit, one proof per
// lane, and the fold weights.
//
// The schedule is the same for every proof (transcript_dev.hpp), so the control flow is
// wave-uniform: a loop over the compiled rate blocks, each XORed into the 25 state lanes held in
// registers, one Keccak-f[1600], and where the block says so a challenge taken from the state.
//  k_replay_prep: one thread per (proof, value) serialises what the transcript absorbs into the
//    value stream [row][proof] — compressed commitments, canonical evaluations and public
//    inputs — and fills FoldIn.ev and FoldIn.rho.
//  k_replay: one lane per proof, a workgroup of one wave. After z it computes z^n, L_1(z) and
//    t_eval (protocol.hpp proof_at_z: no per-lane array for any pi_count); beta and t_eval go
//    back into the lane's own column of the value stream, from where the following blocks absorb
//    them.
//  k_fold_rho: one lane per proof, the weight of a random fold.
#include <hip/hip_runtime.h>

#include <cstring>

#include "verifier_replay.hpp"

using namespace plk;

namespace plk {
namespace {

constexpr uint32_t kItems = PC_COUNT + EV_COUNT + 1;  // per proof besides its public inputs: + rho

struct PrepArgs {
  ReplayLayout lay;
  uint32_t count;
  const plk_g1* comms;
  const Fr* evals;
  const Fr* pi;
  const Fr* weights;
  uint32_t* vals;
  FoldIn* in;
};

__global__ void __launch_bounds__(256) k_replay_prep(PrepArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t item = t / a.count;
  const uint32_t j = (uint32_t)(t % a.count);
  if (item >= kItems + a.lay.npi) return;
  if (item < PC_COUNT) {
    const plk_g1* p = a.comms + (size_t)PC_COUNT * j + item;
    const G1Abi c = g1_load<false>(p);
    uint32_t w[12];
    g1_compress_words(c.x, c.y, c.inf, w);
#pragma unroll
    for (int i = 0; i < 12; ++i)
      a.vals[((size_t)a.lay.comm((uint32_t)item) / 4u + 1u + i) * a.count + j] = w[i];
  } else if (item < PC_COUNT + EV_COUNT) {
    const uint32_t e = (uint32_t)item - PC_COUNT;
    const Fr v = a.evals[(size_t)EV_COUNT * j + e];
    a.in[j].ev[e] = v;
    const Fr c = fe_from_mont(v);
#pragma unroll
    for (int i = 0; i < 8; ++i) a.vals[((size_t)a.lay.eval(e) / 4u + 1u + i) * a.count + j] = c.v[i];
  } else if (item == PC_COUNT + EV_COUNT) {
    a.in[j].rho = a.weights ? a.weights[j] : fe_one<FrCfg>();
  } else {
    const uint32_t i0 = (uint32_t)(item - kItems);
    const Fr c = fe_from_mont(a.pi[(size_t)a.lay.npi * j + i0]);
#pragma unroll
    for (int i = 0; i < 8; ++i) a.vals[((size_t)a.lay.pi(i0) / 4u + 1u + i) * a.count + j] = c.v[i];
  }
}

struct ReplayArgs {
  KeccakState base;
  Fr n_inv;
  ReplayLayout lay;
  uint32_t log_n, count, blocks;
  uint32_t* vals;
  FoldIn* in;
  Fr* u;
  uint32_t* status;
};

__device__ __forceinline__ void put_scalar(const ReplayArgs& a, uint32_t j, uint32_t stream, const Fr& mont) {
  const Fr c = fe_from_mont(mont);
#pragma unroll
  for (int i = 0; i < 8; ++i) a.vals[((size_t)stream / 4u + 1u + i) * a.count + j] = c.v[i];
}

// Between the z challenge and the evaluations: t_eval, L_1(z), z^n (protocol.hpp).
__device__ __forceinline__ void replay_mid(const ReplayArgs& a, const Fr* __restrict__ pi,
                                           const Fr* __restrict__ winv, uint32_t j, const Fr& z) {
  FoldIn* o = a.in + j;
  Fr zn, l1, t_eval;
  // as in replay(): z_h(z) = 0 or z = 1 refuses the batch (the host turns the word into PLK_E_ARG)
  if (!proof_at_z(o->ev, o->ch, z, a.log_n, a.n_inv, pi + (size_t)a.lay.npi * j, winv, a.lay.npi,
                  zn, l1, t_eval))
    atomicOr(a.status, 1u);
  o->t_eval = t_eval;
  o->l1 = l1;
  o->zn = zn;
  put_scalar(a, j, a.lay.t_eval(), t_eval);
}

// sched, pi and winv are only read: as restrict parameters their (wave-uniform) words come
// through the scalar cache
__global__ void __launch_bounds__(64) k_replay(ReplayArgs a, const uint32_t* __restrict__ sched,
                                               const Fr* __restrict__ pi,
                                               const Fr* __restrict__ winv) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.count) return;
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) s[i] = a.base.s[i];
  const uint32_t* vals = a.vals;
  const uint32_t count = a.count;
  for (uint32_t b = 0; b < a.blocks; ++b) {
    const uint32_t* blk = sched + (size_t)b * kBlockWords;
    sched_absorb(s, blk, [&](uint32_t row) { return vals[(size_t)row * count + j]; });
    keccak_f1600(s);
    const uint32_t take = blk[0];  // the same for every proof
    if (take != kNoTake) {
      const Fr c = sched_take_scalar(s);
      a.in[j].ch[take] = c;
      if (take == CH_BETA) put_scalar(a, j, a.lay.beta(), c);
      if (take == CH_Z) replay_mid(a, pi, winv, j, c);
      if (take == CH_U) a.u[j] = c;
    }
  }
}

PLK_HD Fr rho_one(const KeccakState& root, const uint32_t* sched, uint32_t blocks, uint32_t j) {
  Fr r = fe_one<FrCfg>();
  if (j == 0) return r;
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) s[i] = root.s[i];
  for (uint32_t b = 0; b < blocks; ++b) {
    const uint32_t* blk = sched + (size_t)b * kBlockWords;
    // the value stream is the index as a little-endian u64: row 1 = j, row 2 = 0
    sched_absorb(s, blk, [&](uint32_t row) { return row == 1 ? j : 0u; });
    keccak_f1600(s);
    if (blk[0] != kNoTake) r = sched_take_u128(s);
  }
  return r;
}

__global__ void __launch_bounds__(64) k_fold_rho(KeccakState root, const uint32_t* __restrict__ sched,
                                                 uint32_t blocks, uint32_t count, Fr* __restrict__ out,
                                                 uint32_t stride) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  out[(size_t)j * stride] = rho_one(root, sched, blocks, j);
}

void state_from_bytes(const uint8_t state[200], KeccakState& k) { std::memcpy(k.s, state, 200); }

}  // namespace

void replay_plan_compile(const uint8_t state[200], uint8_t pos, uint8_t pos_begin, uint32_t npi,
                         ReplayPlan& plan) {
  const ReplayLayout lay{npi};
  ReplaySchedule t(pos, pos_begin);
  for (const Step& st : kScript) switch (st.kind) {
      case STEP_PI:
        for (uint32_t i = 0; i < npi; ++i) t.append_value(st.label, lay.pi(i), 32);
        break;
      case STEP_COMM: t.append_value(st.label, lay.comm(st.id), 48); break;
      case STEP_CHAL: t.challenge(st.label, 64, st.id); break;
      case STEP_BETA: t.append_value(st.label, lay.beta(), 32); break;
      case STEP_EVAL: t.append_value(st.label, lay.eval(st.id), 32); break;
      case STEP_T_EVAL: t.append_value(st.label, lay.t_eval(), 32); break;
    }
  plan.sched = t.words();
  plan.blocks = t.blocks();
  plan.lay = lay;
  state_from_bytes(state, plan.base);
}

void rho_plan_compile(const uint8_t state[200], uint8_t pos, uint8_t pos_begin, RhoPlan& plan) {
  ReplaySchedule t(pos, pos_begin);
  t.append_value("index", 0, 8);
  t.challenge("rho", 16, 0);
  plan.sched = t.words();
  plan.blocks = t.blocks();
  state_from_bytes(state, plan.root);
}

Fr rho_host(const RhoPlan& plan, uint32_t j) {
  return rho_one(plan.root, plan.sched.data(), plan.blocks, j);
}

int replay_launch(hipStream_t s, const ReplayLaunch& l) {
  const uint64_t threads = (uint64_t)(kItems + l.lay.npi) * l.count;
  if (l.count == 0 || threads > (1ull << 38)) return PLK_E_ARG;
  PLK_HIP_TRY(hipMemsetAsync(l.d_status, 0, sizeof(uint32_t), s));
  PrepArgs p{l.lay, l.count, l.d_comms, l.d_evals, l.d_pi, l.d_weights, l.d_vals, l.d_in};
  hipLaunchKernelGGL(k_replay_prep, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s, p);
  ReplayArgs r{l.base, l.n_inv, l.lay, l.log_n, l.count, l.blocks, l.d_vals, l.d_in, l.d_u, l.d_status};
  hipLaunchKernelGGL(k_replay, dim3((l.count + 63) / 64), dim3(64), 0, s, r, l.d_sched, l.d_pi,
                     l.d_winv);
  PLK_HIP_TRY(hipGetLastError());
  return PLK_OK;
}

int rho_launch(hipStream_t s, const KeccakState& root, const uint32_t* d_sched, uint32_t blocks,
               uint32_t count, Fr* out, uint32_t stride) {
  if (count == 0) return PLK_E_ARG;
  hipLaunchKernelGGL(k_fold_rho, dim3((count + 63) / 64), dim3(64), 0, s, root, d_sched, blocks,
                     count, out, stride);
  PLK_HIP_TRY(hipGetLastError());
  return PLK_OK;
}

}  // namespace plk
