// verifier_replay.hpp — the batch verifier's transcript replay on the GPU (verifier_replay.hip),
// one proof per lane, and the per-proof fold weights. protocol.hpp states what is replayed: the
// host's replay() (verifier.hip) and the compiled schedule here walk the same kScript.
#pragma once
#include <vector>

#include "internal.hpp"
#include "protocol.hpp"
#include "transcript_dev.hpp"

namespace plk {

// What the replay hands to the scalar kernel for one proof (Montgomery form).
struct FoldIn {
  Fr ev[EV_COUNT];  // indexed by Eval (plk_proof order)
  Fr ch[CH_COUNT];  // indexed by Chal
  Fr t_eval, l1, zn, rho;
};

// The value stream of one proof (bytes; transcript_dev.hpp): the public inputs, the 11
// commitments compressed, beta (absorbed again after it is drawn), the 16 evaluations, t_eval.
struct ReplayLayout {
  uint32_t npi;
  PLK_HD uint32_t pi(uint32_t i) const { return 32u * i; }
  PLK_HD uint32_t comm(uint32_t c) const { return 32u * npi + 48u * c; }
  PLK_HD uint32_t beta() const { return comm(PC_COUNT); }
  PLK_HD uint32_t eval(uint32_t e) const { return beta() + 32u + 32u * e; }
  PLK_HD uint32_t t_eval() const { return eval(EV_COUNT); }
  PLK_HD uint32_t rows() const { return (t_eval() + 32u) / 4u + 2u; }  // a padding row at either end
};

// One verifier's replay, compiled from its base transcript (host).
struct ReplayPlan {
  std::vector<uint32_t> sched;
  uint32_t blocks = 0;
  ReplayLayout lay{0};
  KeccakState base;
};
void replay_plan_compile(const uint8_t state[200], uint8_t pos, uint8_t pos_begin, uint32_t npi,
                         ReplayPlan& plan);

// The fold weights: rho_j = challenge_bytes("rho", 16) of a clone of the root transcript after
// append_u64("index", j); rho_0 = 1.
struct RhoPlan {
  std::vector<uint32_t> sched;
  uint32_t blocks = 0;
  KeccakState root;
};
void rho_plan_compile(const uint8_t state[200], uint8_t pos, uint8_t pos_begin, RhoPlan& plan);
Fr rho_host(const RhoPlan& plan, uint32_t j);  // the host mirror of k_fold_rho

struct ReplayLaunch {
  const uint32_t* d_sched;  // the plan's blocks
  uint32_t blocks;
  ReplayLayout lay;
  KeccakState base;
  Fr n_inv;
  uint32_t log_n, count;
  const plk_g1* d_comms;    // proof j's 11 commitments at d_comms[11 j ..], plk_proof order
  const Fr* d_evals;        // count x 16, Montgomery
  const Fr* d_pi;           // count x npi, Montgomery
  const Fr* d_winv;         // omega^-index per public input
  const Fr* d_weights;      // count, or nullptr: rho = 1 (k_fold_rho may follow)
  uint32_t* d_vals;         // lay.rows() x count words
  FoldIn* d_in;
  Fr* d_u;                  // count: the u challenges, contiguous
  uint32_t* d_status;       // one word, cleared here; non-zero: z = 1 or z_h(z) = 0 somewhere
};
// the preparation and replay kernels, stream-ordered
int replay_launch(hipStream_t s, const ReplayLaunch& a);
// out[j * stride] = rho_j, j < count
int rho_launch(hipStream_t s, const KeccakState& root, const uint32_t* d_sched, uint32_t blocks,
               uint32_t count, Fr* out, uint32_t stride);

}  // namespace plk
