// msm_common.hpp — what the MSM's translation units share: device load/store helpers, the
// sort / accumulate contract, the shape constants and the batch plan, the per-SRS workspace
// and the stage launchers (msm_sort.hip, msm_acc.hip, msm_reduce.hip) the driver (msm.hip) calls.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "ffr.hpp"
#include "internal.hpp"

namespace plk {

#ifndef PLK_CHUNK_MAX
#define PLK_CHUNK_MAX 64
#endif
#ifndef PLK_CHUNK_MIN
#define PLK_CHUNK_MIN 16
#endif
constexpr uint32_t kChunkMin = PLK_CHUNK_MIN;  // points per accumulation task (bounds)
// small batches (the one-dispatch sort's: B <= 4 096, <= 8 192 scalars per slot) take tasks
// of down to 8 points: their latency-bound accumulation chains halve (round 4: 2^12 proofs
// +7 %; 8 everywhere cost the 2^14 / 2^16 proofs and the lone 2^16 MSM 1-3 %)
#ifndef PLK_CHUNK_SMALL
#define PLK_CHUNK_SMALL 8
#endif
constexpr uint32_t kChunkSmall = PLK_CHUNK_SMALL;
constexpr uint32_t kChunkMax = PLK_CHUNK_MAX;
// task record .y = partial index | (length - 1) << kTaskShift
constexpr uint32_t kTaskShift = 32 - (kChunkMax <= 64 ? 6 : 7);
static_assert(kChunkMax <= 128, "task length field");
// The contract between the sorts (msm_sort.hip, msm_var.hip) and k_accumulate (msm_acc.hip),
// stated once. An entry of the sorted digit list is a table row with the digit's sign on top;
// a task is {first entry, partial index | (length - 1) << kTaskShift}: 1 .. kChunkMax
// same-bucket entries whose sum goes to partials[partial index] (< kTaskIndexEnd).
constexpr uint32_t kEntryNeg = 0x80000000u;  // the entry's point is subtracted
constexpr uint32_t kTaskIndexEnd = 1u << kTaskShift;
__device__ __forceinline__ uint32_t entry_code(uint32_t row, bool neg) { return row | (neg ? kEntryNeg : 0u); }
__device__ __forceinline__ uint32_t entry_row(uint32_t code) { return code & ~kEntryNeg; }
__device__ __forceinline__ bool entry_neg(uint32_t code) { return code & kEntryNeg; }
__device__ __forceinline__ uint2 task_record(uint32_t first, uint32_t partial, uint32_t len) {
  return make_uint2(first, partial | ((len - 1) << kTaskShift));
}
__device__ __forceinline__ uint32_t task_len(const uint2& t) { return (t.y >> kTaskShift) + 1; }
__device__ __forceinline__ uint32_t task_partial(const uint2& t) { return t.y & (kTaskIndexEnd - 1); }
constexpr uint32_t kBatchAff = 32;  // points per batch-inversion chunk
constexpr uint32_t kMaxSlots = 16;  // independent MSMs per batch

struct MsmCfg {
  uint32_t c, W, B;
  uint32_t narrow;  // plk_srs::narrow: the top `narrow` windows are c - 1 bits, digits x 2
  // bucket range of a part (msm_run_batch parts > 1: the wide-set sort keeps only digits of
  // buckets [b_lo, b_lo + B), renumbered from 0); b_lo = 0 for a whole MSM
  uint32_t b_lo;
};

// Kernel-argument view of one batch of independent MSMs (slot = blockIdx.y).
struct MsmBatch {
  const Fr* scalars[kMaxSlots];
  uint32_t len[kMaxSlots];
  uint64_t check_len[kMaxSlots];
};

__device__ __forceinline__ void ld_fp(const uint32_t* p, Fp& r) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    uint4 a = q[i];
    r.v[4 * i] = a.x; r.v[4 * i + 1] = a.y; r.v[4 * i + 2] = a.z; r.v[4 * i + 3] = a.w;
  }
}

__device__ __forceinline__ void st_fp(uint32_t* p, const Fp& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = make_uint4(v.v[4 * i], v.v[4 * i + 1], v.v[4 * i + 2], v.v[4 * i + 3]);
}

__device__ __forceinline__ void ld_aff(const G1Affine* p, Fp& x, Fp& y) {
  ld_fp(reinterpret_cast<const uint32_t*>(p), x);
  ld_fp(reinterpret_cast<const uint32_t*>(p) + 12, y);
}

__device__ __forceinline__ void st_aff(G1Affine* p, const Fp& x, const Fp& y) {
  st_fp(reinterpret_cast<uint32_t*>(p), x);
  st_fp(reinterpret_cast<uint32_t*>(p) + 12, y);
}

__device__ __forceinline__ void ld_xyzz(const G1xyzz* p, G1xyzz& r) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
  ld_fp(q, r.X); ld_fp(q + 12, r.Y); ld_fp(q + 24, r.ZZ); ld_fp(q + 36, r.ZZZ);
}

__device__ __forceinline__ void st_xyzz(G1xyzz* p, const G1xyzz& r) {
  uint32_t* q = reinterpret_cast<uint32_t*>(p);
  st_fp(q, r.X); st_fp(q + 12, r.Y); st_fp(q + 24, r.ZZ); st_fp(q + 36, r.ZZZ);
}

__device__ __forceinline__ Fr ld_fr(const Fr* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  Fr r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  return r;
}

// Head of a batch's readback record (MsmWorkspace::host_out, written by the kernels straight
// into mapped host memory, the bit sums after it): per slot the degree-check flag (stamped
// with the batch's generation number by k_any_nonzero) and the entry count (point
// additions, written by k_bitsum2), and for a guarded batch (MsmGuard) the slot's largest
// bucket count (k_guard). A multiple of 16 bytes, so the G1xyzz records after it stay aligned.
struct ReadbackHeader {
  uint32_t flag[kMaxSlots];
  uint32_t entries[kMaxSlots];
  uint32_t max_count[kMaxSlots];
};
static_assert(sizeof(ReadbackHeader) % 16 == 0, "alignment of the bit sums");

// ---- the constants the plan (msm.hip) and the kernels (msm_sort.hip, msm_reduce.hip) share
#ifndef PLK_LANE_PARTIALS
#define PLK_LANE_PARTIALS 4  // bucket partials per k_bucket_sum lane aimed at (only c <= 15, SRS < 2^16: 8 -> 4 gave 2^12 3.74 -> 3.93 M constraints/s, tools/gpu_ab_quick.sh)
#endif
#ifndef PLK_CHUNK_TARGET
#define PLK_CHUNK_TARGET 262144  // accumulation tasks aimed at per batch (chunk = entries / this)
#endif
constexpr uint32_t kHistBlocksMax = 256;  // histogram / scatter workgroups per slot
// LDS histograms cover at most kLdsBuckets buckets (128 KiB); larger bucket sets (c = 17)
// are processed in bucket windows, each a fresh pass over the workgroup's scalars.
constexpr uint32_t kLdsBuckets = 32768;
// small bucket sets (the 2^12-size commits, c <= 13): k_sort_small / k_sort_one hold the
// bucket counts in LDS (msm_sort.hip)
constexpr uint32_t kSortSmallMax = 4096;
constexpr uint32_t kSortOneMax = 8192;  // scalars per slot held in registers
// workgroups per slot, each taking 1/kSortOneParts of the buckets (round 5, three interleaved
// runs against one workgroup, profiles/r05_sort_one_parts_ab.jsonl: lone 2^12 MSM 0.394 ->
// 0.347 ms, 2^12 proofs 8.81 -> 9.10 M, 2^13 within noise; 8 workgroups the same as 4)
constexpr uint32_t kSortOneParts = 4;
// HOLD: the slot's scalars (<= kSortOneMax) stay in registers between the histogram and the
// scatter; otherwise (<= kSortOneBig, the 2^14-size commits at c = 13) both passes read them
// from memory, 4 ahead per thread (for_scalars)
constexpr uint32_t kSortOneBig = 32768;
constexpr uint32_t kFineBits = 10;  // 2^10 buckets per coarse bin = threads of k_fine
// A bucket-range part (parts > 1) of 2^(c-1) / parts buckets keeps >= 256 coarse bins (k_fine
// / k_make_tasks_wide workgroups) with bins of 2^FB buckets, FB = max(8, 10 - log2 parts)
constexpr uint32_t kFineBitsMin = 8;
constexpr uint32_t kCoarseMax = 4096;        // coarse bins (B <= 2^22, c <= 23)
// bucket reduction: runs of K = 2^rb buckets per lane. Batches of several MSMs (the
// prover's commit groups, with other proofs' kernels beside them) take 16. A lone MSM's
// run-sum chains are latency-bound with the chip otherwise idle, so its rb is the largest
// rb <= kRunBits that still gives kRunLanes run lanes: K = 8 at 2^20, 2 at 2^16 (lone
// 2^16 MSM 1.14 -> 1.01 ms in round 2). Applied to batches too it cost the 2^16 proof
// 22 -> 18 M constraints/s (more bit-sum groups, NR / 256, in every commit group).
constexpr uint32_t kRunBits = 4, kRunBitsMin = 1;
// run lanes aimed at: 65536 (one wave per SIMD) — with the 4-lane k_bitsum1 a lone 2^20
// MSM then runs rb = 3, 256 bit-sum groups: 3.44 -> 3.34 ms (131072: rb = 2, 512 groups)
constexpr size_t kRunLanes = 65536;
constexpr uint32_t kBitsumOut = 10;  // k_bitsum1's records per group of 256 (msm_reduce.hip)
// k_bitsum1 folds k_bitsum2 in when a slot has at most this many bit-sum groups (msm_reduce.hip)
constexpr uint32_t kFoldMaxGroups = 16;
// kRunLanes, or PLK_RUN_LANES from the environment (sweeps)
PLK_LOCAL inline size_t run_lanes() {
  static const size_t v = [] {
    const char* e = getenv("PLK_RUN_LANES");
    const long long x = e ? atoll(e) : 0;
    return x > 0 ? (size_t)x : kRunLanes;
  }();
  return v;
}
// a batch's rb: kRunBits, or PLK_RUN_BITS_BATCH from the environment (sweeps; 1 .. 8)
PLK_LOCAL inline uint32_t batch_run_bits() {
  static const uint32_t v = [] {
    const char* e = getenv("PLK_RUN_BITS_BATCH");
    const int x = e ? atoi(e) : 0;
    return x >= 1 && x <= 8 ? (uint32_t)x : kRunBits;
  }();
  return v;
}
PLK_LOCAL inline uint32_t run_bits(uint32_t B, uint32_t slots) {
  if (slots > 1) return std::min<uint32_t>(batch_run_bits(), 31 - __builtin_clz(B));
  uint32_t rb = kRunBits;
  while (rb > kRunBitsMin && (size_t)(B >> rb) < run_lanes()) --rb;
  return rb;
}
// wide bucket sets (2^(c-1) > kLdsBuckets, c >= 17): two-level sort and run-sum reduction
PLK_LOCAL inline bool is_wide(uint32_t c) { return (1u << (c - 1)) > kLdsBuckets; }
// small shapes (the 2^12-size proofs' commits: k_sort_one with the scalars held in registers)
// may run tasks of kChunkSmall points; ws_reserve sizes the task buffers for them
PLK_LOCAL inline bool is_small_shape(uint32_t c, size_t len) {
  return !is_wide(c) && (1u << (c - 1)) <= kSortSmallMax && len <= kSortOneMax;
}

// Everything one batch's launches follow from, derived once by msm_plan (msm.hip) from the SRS
// shape, the slots' lengths, part / parts and the workspace's policy, before any kernel runs.
// msm_sort, launch_accumulate and msm_reduce read it, and MsmWorkspace::last keeps the most
// recent one for plk_debug_msm_snapshot (debug.hip).
struct MsmPlan {
  uint32_t slots = 0, part = 0, parts = 1;
  uint32_t c = 0, W = 0, narrow = 0;  // the SRS's windows (plk_srs)
  bool naf = false;                   // the SRS's row-table layout (plk_srs::naf, msm_digits.hpp)
  uint64_t n_srs = 0;
  bool has_inf = false;
  uint32_t B = 0, b_lo = 0;  // the buckets this call reduces: all 2^(c-1), or a part's range
  bool wide = false;         // is_wide(c)
  size_t max_len = 0, max_tail = 0, total_entries = 0;  // over the slots
  bool sort_one = false, hold = false;  // k_sort_one, with the scalars held in registers
  bool small_sort = false;              // k_sort_small after k_hist (B <= kSortSmallMax)
  uint32_t hist_blocks = 0;             // histogram / scatter workgroups per slot
  uint32_t fb = 0, NC = 0;              // wide sets: bins of 2^fb buckets, NC of them
  uint32_t chunk = 0;                   // points per accumulation task
  uint64_t max_tasks_used = 0;          // bound on a slot's tasks
  uint32_t acc_blocks = 0;              // k_accumulate's grid.x (256 task lanes each)
  bool lone = false;                    // k_accumulate's LONE form (!shared_chip)
  uint32_t rb = 0, NR = 0;              // runs of 2^rb buckets, NR of them per slot
  uint32_t lp = 0;                      // narrow sets: 2^lp k_bucket_sum lanes per bucket
  uint32_t G = 0, nbits = 0, nout = 0;  // bit-sum groups (a power of two), T_j count, outputs
  bool fold = false;                    // k_bitsum2 folded into k_bitsum1 (G <= kFoldMaxGroups)
  int tail_quad = 0;                    // MsmWorkspace::tail_quad
  uint32_t guard_limit = 0;             // hot-bucket guard (k_guard), 0: off
  uint32_t gen = 0;                     // the batch's generation stamp (set by msm_run_batch)
  MsmCfg cfg() const { return MsmCfg{c, W, B, narrow, b_lo}; }
};

struct MsmWorkspace {
  MsmPlan last;
  DevBuf counts, blockhist, offsets, task_off, full_off, len_cur, sorted, tasks, partials, bsum, bits1;
  // wide bucket sets only (msm_sort.hip: two-level sort; msm_reduce.hip: run-sum reduction)
  DevBuf tmp, task_rel, bin_tot, len_fill, coarse_off, rsum, ys, zs;
  DevBuf naf;   // row-table layout: the scalars' digit words, W per scalar (k_chist_naf)
  DevBuf done;  // k_bitsum1's per-slot arrival counters (its fold of k_bitsum2)
  DevBuf guard;  // k_guard's per-slot running maxima and arrival counters (2 kMaxSlots words)
  // the readback record (ReadbackHeader + bit sums): coherent host memory mapped into the
  // device's address space, written by the kernels themselves (no copy dispatch per batch)
  PinnedBuf host_out;
  void* out_dev = nullptr;  // host_out's device address
  uint32_t gen = 0;    // generation number of the last batch (degree-check flag stamps)
  size_t cap_len = 0, task_stride = 0, sorted_stride = 0, naf_stride = 0;
  uint32_t cap_slots = 0;
  // the SRS shape the buffers and strides were sized for: a workspace moves between SRSs
  // (a prover's key SRS, then a shard slice with another window size), and every size
  // above depends on c and the window count
  uint32_t cap_c = 0, cap_windows = 0;
  uint32_t cap_chunk_min = kChunkMin;  // the task-length floor the buffers were sized for
  // the bit-sum trees' additions: 1 quad-cooperative (g1r_add_quad, lower latency, the lone
  // call's choice), 0 one lane each (fewer issue slots per addition, for prover lanes that
  // share the chip with other proofs), 2 quads in k_bitsum2 only (lane_tail_policy).
  // PLK_TAIL_QUAD (experiments, tests) forces a form for every workspace created while it is
  // set: read once here, never per batch (a getenv in the hot path raced the tests' setenv)
  int tail_quad = 1;
  bool tail_forced = false;
  // the chip is shared with other proofs' kernels (prover lanes): k_accumulate's grouped form
  // at 2 waves per SIMD; otherwise (lone commits, plk_prove) the LONE form (msm_acc.hip)
  bool shared_chip = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  MsmStats stats;
  MsmWorkspace() {
    if (const char* e = getenv("PLK_TAIL_QUAD")) {
      const int v = atoi(e);
      if (v >= 0 && v <= 2) {
        tail_quad = v;
        tail_forced = true;
      }
    }
  }
  ~MsmWorkspace() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

int ws_reserve(plk_srs* s, MsmWorkspace& w, size_t len, uint32_t slots, hipStream_t stream);

// The reduction trees' form for a prover lane of an n-row circuit (plk_prover_create; lone
// commits and plk_prove's default prover keep 1). A lane shares the chip with other lanes'
// proofs, so issue slots per addition count more than a tree level's latency, except where
// the reduction tails stay latency-bound. Measured, prover lanes at the bench's lane counts,
// interleaved on one box (constraints/s, 0 / 1 / 2):
//   2^12  7.61-7.80 / 8.26-8.65 / —          -> 1 (profiles/r04_tail_quad_ab.jsonl, r04p)
//   2^14  15.1-15.6 / 15.2-15.5 / +3 %        -> 2 (profiles/r04_tail_mode2_ab.jsonl,
//                                                   r04_tail_modes_small_ab.jsonl)
//   2^16  26.2-26.9 / 24.1-26.2 / -3 % vs 0   -> 0
//   2^20  32.5-32.7 / 32.1-32.3 / +0.6 % vs 0 -> 2
// and, round 5 (profiles/r05_small_and_tail_policy_ab.jsonl, two interleaved runs each):
//   2^15  21.2-21.4 / 20.3-20.9 / 21.3-21.5   -> 0 (2 within noise)
//   2^17  29.1-29.2 / 28.5-28.5 / 29.0-29.2   -> 0
//   2^18  29.6-29.8 / 29.0-29.2 / 29.5-29.6   -> 0
// 2^19 and up as 2^20. Re-measured after 2^13 / 2^14 moved to c = 12 / 13 (round 5,
// profiles/r05_tail_forms_new_c_ab.jsonl, three interleaved runs): 2^13 12.71 / 13.17 / 12.74 M
// -> 1 stays, 2^14 16.87 / 16.18 / 17.37 M -> 2 stays.
inline int lane_tail_policy(uint64_t n) {
  if (n <= (1ull << 13)) return 1;
  if (n == (1ull << 14)) return 2;
  if (n >= (1ull << 19)) return 2;
  return 0;
}

// R'-domain [0, 2p) packed XYZZ coordinates (ffr.hpp), as the reduction kernels store them ->
// canonical R-domain (msm.hip): what the host tails read back
G1xyzz rx_to_r_domain(const G1xyzz& p);
// One coordinate of it, for a value already below p (the host reduces a packed [0, 2p) value once,
// a kernel packs with rx_pack_canonical): x * 2^-SH (SH = BL - 384 = 6) as the R-domain product
// x * 2^(384 - SH) / 2^384.
PLK_HD Fp fp_rx_to_r(const Fp& x) {
  constexpr int SH = RxShape<FpCfg>::B * RxShape<FpCfg>::L - 32 * FpCfg::N;
  static_assert(SH > 0 && SH < 32, "R' / R shift");
  Fp k = fe_zero<FpCfg>();
  k.v[11] = 1u << (32 - SH);  // 2^(384 - SH) (< p)
  return fe_mul(x, k);
}

// The batch's sort (msm_sort.hip): the commit degree check, the path the plan chose (one
// dispatch, LDS histogram or two-level wide) and the hot-bucket guard, leaving offsets, sorted,
// task_off and tasks in the workspace. The launches only, stream-ordered.
PLK_LOCAL int msm_sort(const MsmPlan& p, const MsmBatch& batch, MsmWorkspace& w, hipStream_t stream);
// The sort kernels' dynamic-LDS limits for window size c, once per workspace shape (ws_reserve)
PLK_LOCAL int msm_sort_prepare(uint32_t c);
// The batch's bucket reduction (msm_reduce.hip): bucket sums or run sums, then the bit sums and
// the entry counts into the workspace's readback record. The launches only, stream-ordered.
PLK_LOCAL void msm_reduce(const MsmPlan& p, MsmWorkspace& w, hipStream_t stream);

// k_accumulate (msm_acc.hip) over grid.x * 256 task lanes per slot (grid.y = slots), stamped
// with the start / stop events ev0 / ev1 by the dispatch itself
void launch_accumulate(bool has_inf, bool lone, dim3 grid, hipStream_t stream, hipEvent_t ev0,
                       hipEvent_t ev1, const uint2* tasks, const uint32_t* task_off, uint32_t B,
                       uint64_t task_stride, const uint32_t* sorted, uint64_t sorted_stride,
                       const G1Affine* table, const uint8_t* table_inf, G1xyzz* partials);

}  // namespace plk
