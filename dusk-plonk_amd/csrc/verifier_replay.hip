// verifier_replay.hip — the merlin replay of Proof::verify (verifier.hip replay(), the
// contract) for a batch of proofs of one circuit, one proof per lane, and the fold weights.
//
// The schedule is the same for every proof (transcript_dev.hpp), so the control flow is
// wave-uniform: a loop over the compiled rate blocks, each XORed into the 25 state lanes held in
// registers, one Keccak-f[1600], and where the block says so a challenge taken from the state.
//  k_replay_prep: one thread per (proof, value) serialises what the transcript absorbs into the
//    value stream [row][proof] — compressed commitments, canonical evaluations and public
//    inputs — and fills FoldIn.ev and FoldIn.rho.
//  k_replay: one lane per proof, a workgroup of one wave. After z it computes z^n, Z_H(z),
//    L_1(z), PI(z) and t_eval; beta and t_eval go back into the lane's own column of the value
//    stream, from where the following blocks absorb them.
//  k_fold_rho: one lane per proof, the weight of a random fold.
// PI(z) = Z_H(z) / n  sum_i pi_i / (omega^-i z - 1) is summed as ONE fraction: per non-zero
// input num = num d_i + pi_i den, den = den d_i (four products), and den joins Z_H(z) and z - 1
// in the proof's single Fermat inversion. No per-lane array for any pi_count.
#include <hip/hip_runtime.h>

#include <cstring>

#include "verifier_replay.hpp"

using namespace plk;

namespace plk {
namespace {

constexpr uint32_t kItems = 11 + 16 + 1;  // per proof besides its public inputs: + rho

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
  if (item < 11) {
    const plk_g1* p = a.comms + (size_t)11 * j + item;
    const G1Abi c = g1_load<false>(p);
    uint32_t w[12];
    g1_compress_words(c.x, c.y, c.inf, w);
#pragma unroll
    for (int i = 0; i < 12; ++i)
      a.vals[((size_t)a.lay.comm((uint32_t)item) / 4u + 1u + i) * a.count + j] = w[i];
  } else if (item < 27) {
    const uint32_t e = (uint32_t)item - 11;
    const Fr v = a.evals[(size_t)16 * j + e];
    a.in[j].ev[e] = v;
    const Fr c = fe_from_mont(v);
#pragma unroll
    for (int i = 0; i < 8; ++i) a.vals[((size_t)a.lay.eval(e) / 4u + 1u + i) * a.count + j] = c.v[i];
  } else if (item == 27) {
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

// What replay() computes between the z challenge and the evaluations: t_eval, L_1(z), z^n.
__device__ __forceinline__ void replay_mid(const ReplayArgs& a, const Fr* __restrict__ pi,
                                           const Fr* __restrict__ winv, uint32_t j, const Fr& z) {
  FoldIn* o = a.in + j;
  const Fr one = fe_one<FrCfg>();
  Fr zn = z;
  for (uint32_t i = 0; i < a.log_n; ++i) zn = fe_sqr(zn);
  const Fr z_h = fe_sub(zn, one), zm1 = fe_sub(z, one);
  // as in replay(): z_h(z) = 0 or z = 1 refuses the batch (the host turns the word into PLK_E_ARG)
  if (fe_is_zero(z_h) || fe_is_zero(zm1)) atomicOr(a.status, 1u);
  // the barycentric sum as one fraction; zero public inputs are skipped, as in the reference
  Fr num = fe_zero<FrCfg>(), den = one;
  for (uint32_t i = 0; i < a.lay.npi; ++i) {
    const Fr p = pi[(size_t)a.lay.npi * j + i];
    if (!fe_is_zero(p)) {
      const Fr d = fe_sub(fe_mul(winv[i], z), one);
      num = fe_add(fe_mul(num, d), fe_mul(p, den));
      den = fe_mul(den, d);
    }
  }
  // one inversion for z_h, z - 1 and den
  const Fr ab = fe_mul(z_h, zm1);
  const Fr inv = fe_inv(fe_mul(ab, den));
  const Fr den_inv = fe_mul(inv, ab);
  const Fr inv_den = fe_mul(inv, den);
  const Fr zm1_inv = fe_mul(inv_den, z_h), zh_inv = fe_mul(inv_den, zm1);
  const Fr zh_n = fe_mul(z_h, a.n_inv);
  const Fr l1 = fe_mul(zh_n, zm1_inv);  // z_h / (n (z - 1))
  const Fr pi_eval = fe_mul(fe_mul(num, den_inv), zh_n);
  // t_eval (proof.rs:386-440)
  const Fr beta = o->ch[0], gamma = o->ch[1], alpha = o->ch[2];
  const Fr b0 = fe_add(fe_add(o->ev[0], fe_mul(beta, o->ev[11])), gamma);
  const Fr b1 = fe_add(fe_add(o->ev[1], fe_mul(beta, o->ev[12])), gamma);
  const Fr b2 = fe_add(fe_add(o->ev[2], fe_mul(beta, o->ev[13])), gamma);
  const Fr b3 = fe_mul(fe_mul(fe_add(o->ev[3], gamma), o->ev[15]), alpha);
  const Fr b_term = fe_mul(fe_mul(b0, b1), fe_mul(b2, b3));
  const Fr c_term = fe_mul(l1, fe_mul(alpha, alpha));
  const Fr t_eval = fe_mul(fe_sub(fe_sub(fe_add(o->ev[14], pi_eval), b_term), c_term), zh_inv);
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
      if (take == 0) put_scalar(a, j, a.lay.beta(), c);
      if (take == 7) replay_mid(a, pi, winv, j, c);
      if (take == 10) a.u[j] = c;
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
  auto comm = [&](const char* label, uint32_t c) { t.append_value(label, lay.comm(c), 48); };
  auto eval = [&](const char* label, uint32_t e) { t.append_value(label, lay.eval(e), 32); };
  auto chal = [&](const char* label, uint32_t id) { t.challenge(label, 64, id); };
  // the order of replay() in verifier.hip
  for (uint32_t i = 0; i < npi; ++i) t.append_value("pi", lay.pi(i), 32);
  comm("a_w", 0);
  comm("b_w", 1);
  comm("c_w", 2);
  comm("d_w", 3);
  chal("beta", 0);
  t.append_value("beta", lay.beta(), 32);
  chal("gamma", 1);
  comm("z", 4);
  chal("alpha", 2);
  chal("range separation challenge", 3);
  chal("logic separation challenge", 4);
  chal("fixed base separation challenge", 5);
  chal("variable base separation challenge", 6);
  comm("t_low", 5);
  comm("t_mid", 6);
  comm("t_high", 7);
  comm("t_4", 8);
  chal("z_challenge", 7);
  eval("a_eval", 0);
  eval("b_eval", 1);
  eval("c_eval", 2);
  eval("d_eval", 3);
  eval("a_next_eval", 4);
  eval("b_next_eval", 5);
  eval("d_next_eval", 6);
  eval("s_sigma_1_eval", 11);
  eval("s_sigma_2_eval", 12);
  eval("s_sigma_3_eval", 13);
  eval("q_arith_eval", 7);
  eval("q_c_eval", 8);
  eval("q_l_eval", 9);
  eval("q_r_eval", 10);
  eval("perm_eval", 15);
  t.append_value("t_eval", lay.t_eval(), 32);
  eval("r_eval", 14);
  chal("v_challenge", 8);
  chal("v_challenge", 9);
  comm("w_z", 9);
  comm("w_z_w", 10);
  chal("batch", 10);
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
