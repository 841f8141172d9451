// msm.hip — G1 multi-scalar multiplication behind KZG commit on gfx950: the design, the
// batch plan and the host driver. The kernels live in msm_sort.hip (recoding in msm_digits.hpp),
// msm_acc.hip and msm_reduce.hip, behind the launchers msm_common.hpp declares.
//
// Replaces msm_curve_addition inside zksnarks PlonkParams::commit (un-vendored; called at
// prover.rs:133-136,194,262-265,440,452 and key.rs:138-159).
//
// Design (fixed-base Pippenger, all windows folded into one bucket set):
//  * SRS load (srs.hip): table[w][i] = 2^(c*w) * P_i in affine form, w < W, resident in
//    HBM (W * n * 96 B: 1.6 GB at n = 2^20, c = 16, W = 16). Commit bases are always an
//    SRS prefix, so the table is built once.
//  * Per MSM: each scalar s is first brought to [0, (r-1)/2] (s or r - s with the signs
//    flipped, scalar_half), then recoded into W = ceil(255/c) signed c-bit digits
//    |d| <= 2^(c-1); digit (i, w) sends +-table[w][i] to bucket |d|-1: ONE set of
//    B = 2^(c-1) buckets and no per-window doubling chain.
//  * Counting sort by bucket: per-workgroup LDS histograms (windows of 32 K buckets =
//    128 KiB; c = 17 takes two) written whole, a per-bucket scan over the workgroups
//    (k_block_scan) instead of global atomics, then LDS atomics place each digit. Order
//    inside a bucket is irrelevant: group addition is exact and the canonical affine
//    output is unique.
//  * Bucket accumulation in chunks of CH points (one thread per chunk, XYZZ mixed adds):
//    the dominant kernel, integer-VALU bound.
//  * Bucket reduction sum_b (b+1) S_b = sum_j 2^j T_j (T_j: sums of buckets selected by the
//    bits of their weight, see k_bitsum1): two shallow tree kernels give the c points T_j and
//    the CPU runs the 2c-op Horner tail and the single inversion to canonical affine.
//  * Up to kMaxSlots independent MSMs run as ONE batch (blockIdx.y = slot): the prover's
//    commits come in independent groups (4 wires, 4 quotient chunks, 2 openings), and the
//    latency-bound tail kernels of a batch then cost about what one MSM's tail costs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "internal.hpp"
#include "msm_common.hpp"

namespace plk {

// R'-domain [0, 2p) packed coordinates (ffr.hpp) -> canonical R-domain
G1xyzz rx_to_r_domain(const G1xyzz& p) {
  G1xyzz r = p;
  for (Fp* c : {&r.X, &r.Y, &r.ZZ, &r.ZZZ}) {
    fe_reduce_once(*c);
    *c = fp_rx_to_r(*c);
  }
  return r;
}

bool msm_parts_ok(const plk_srs* s, uint32_t parts) {
  if (parts == 0 || (parts & (parts - 1))) return false;
  // a part's bucket range stays a wide set's (two-level sort, run sums): >= 2^14 buckets
  return parts == 1 || (is_wide(s->c) && ((1u << (s->c - 1)) / parts) >= (1u << 14));
}

// The plan of one batch: the SRS shape, the slots' lengths (batch), part / parts and the
// workspace's policy (tail_quad, shared_chip, cap_chunk_min) in, every shape value the sort,
// the accumulation and the reduction launch with out. No HIP call, no buffer touched.
// PLK_E_DEVICE: a part's run count is not 256 G (the part offset's Horner seed, host_tail).
static int msm_plan(const plk_srs* s, const MsmWorkspace& w, const MsmBatch& batch, uint32_t slots,
                    size_t max_len, uint32_t part, uint32_t parts, uint32_t guard_limit, MsmPlan& p) {
  p = MsmPlan{};
  p.slots = slots;
  p.part = part;
  p.parts = parts;
  p.c = s->c;
  p.W = s->windows;
  p.narrow = s->narrow;
  p.naf = s->naf;
  p.n_srs = s->n;
  p.has_inf = s->has_inf;
  p.guard_limit = guard_limit;
  p.tail_quad = w.tail_quad;
  p.lone = !w.shared_chip;
  p.max_len = max_len;  // over the slots, as ws_reserve was sized (msm_run_batch)
  for (uint32_t k = 0; k < slots; ++k) {
    const size_t len = batch.len[k];
    if (batch.check_len[k] > len) p.max_tail = std::max<size_t>(p.max_tail, batch.check_len[k] - len);
    p.total_entries += (size_t)p.W * len;
  }
  // B: the buckets this call reduces (all 2^(c-1), or a part's range of them)
  const uint32_t B_all = 1u << (p.c - 1), B = B_all / parts;
  p.B = B;
  p.b_lo = part * B;
  // wide bucket sets: two-level sort and run-sum reduction; the bit sums then run over the
  // NR = B / 2^rb runs instead of the buckets
  p.wide = is_wide(p.c);
  p.rb = run_bits(B, slots);
  // coarse-bin width (wide sets): 2^10 buckets, finer for a part's narrower range
  p.fb = kFineBits;
  while (p.fb > kFineBitsMin && (1u << (kFineBits - p.fb)) < parts) --p.fb;
  p.NC = B >> p.fb;
  p.NR = B >> p.rb;
  p.G = cdiv(p.wide ? p.NR : B, 256);  // a power of two
  if (parts > 1 && p.NR != 256u * p.G) return PLK_E_DEVICE;  // the part offset's Horner seed (host_tail)
  p.nbits = 8 + (uint32_t)__builtin_ctz(p.G);  // T_0..T_7 of u, one per bit of g
  p.nout = p.nbits + (p.wide ? 2u : 0u);       // + sum_r T_r, sum_r Y_r
  p.fold = p.G <= kFoldMaxGroups;  // k_bitsum2 folded into k_bitsum1 when the slots have few groups
  // chunk so that the accumulation grid holds ~2 waves of the chip's resident threads. Wide
  // sets in a batch have few entries per bucket and enough tasks anyway: one task per bucket.
  // A lone wide MSM below ~2^18 points (configs[2]-style commits at 2^16) would leave one
  // task of ~15-35 dependent additions per bucket on a half-empty chip: it takes the chunk
  // formula too (16 at 2^16, 52 at 2^20)
  const bool small_batch = is_small_shape(p.c, p.max_len);
  // the task-length floor: kChunkSmall for small batches when the workspace was sized for it
  const uint32_t chunk_floor = small_batch ? std::max(kChunkSmall, w.cap_chunk_min) : kChunkMin;
  const uint32_t chunk_fit = (uint32_t)std::min<size_t>(
      kChunkMax, std::max<size_t>(chunk_floor, p.total_entries / parts / PLK_CHUNK_TARGET));
  p.chunk = p.wide && slots > 1 ? kChunkMax : chunk_fit;
  p.max_tasks_used = (size_t)p.W * p.max_len / p.chunk + B;
  p.acc_blocks = cdiv(p.max_tasks_used, 256);
  // 256 workgroups per slot: fewer give longer per-bucket write runs in k_scatter but lose
  // more parallelism than they gain (measured 2.77 / 2.79 / 3.02 / 4.52 ms per proof at
  // 256 / 128 / 64 / 32, tools/gpu_hist_sweep.sh)
  p.hist_blocks = std::max<uint32_t>(1, std::min<uint32_t>(kHistBlocksMax, cdiv(p.max_len, 512)));
  // small batches: the whole sort (and the degree check) in one dispatch (k_sort_one,
  // msm_sort.hip), up to kSortOneBig scalars; up to kSortOneMax of them held in registers
  p.small_sort = !p.wide && B <= kSortSmallMax;
  p.sort_one = p.small_sort && p.max_len <= kSortOneBig;
  p.hold = p.sort_one && p.max_len <= kSortOneMax;
  if (!p.wide) {
    // lanes per bucket: until each lane adds ~PLK_LANE_PARTIALS partials (partials per bucket = entries /
    // chunk + 1 tail) or the grid holds 2^17 lanes (the tree levels cost a full addition
    // per lane, so an already full chip gains nothing from more lanes per bucket)
    const size_t per_bucket = cdiv(p.total_entries, (size_t)p.chunk * B * slots) + 1;
    while (p.lp < 4 && ((size_t)PLK_LANE_PARTIALS << p.lp) < per_bucket && (((size_t)B * slots) << p.lp) < 131072) ++p.lp;
  }
  return PLK_OK;
}

int ws_reserve(plk_srs* s, MsmWorkspace& w, size_t len, uint32_t slots, hipStream_t stream) {
  // (a workspace sized on a window table meets a row table: the digit words are still to come)
  const bool same_shape = w.cap_c == s->c && w.cap_windows == s->windows && (!s->naf || w.naf.ptr);
  if (same_shape && len <= w.cap_len && slots <= w.cap_slots && w.cap_len) return PLK_OK;
  // buffers only ever grow (DevBuf::alloc), so re-sizing for another shape keeps the larger
  // of the old and new needs; the strides below always match the current shape
  len = std::max(len, w.cap_len);
  slots = std::max(slots, w.cap_slots);
  const size_t B = (size_t)1 << (s->c - 1);
  const bool wide = is_wide(s->c);
  const size_t NC = B >> kFineBits;
  // runs over all slots of a batch (run_bits: a batch runs B >> kRunBits per slot, a lone
  // MSM fewer than 2 kRunLanes unless rb = kRunBits)
  const size_t max_runs =
      std::max<size_t>(slots * (B >> std::min(kRunBits, batch_run_bits())), B >> kRunBitsMin);
  if (wide && NC > kCoarseMax) return PLK_E_ARG;
  const size_t entries = (size_t)s->windows * len;
  // small shapes (k_sort_one's) may run tasks of kChunkSmall points (msm_plan)
  const uint32_t chunk_min = is_small_shape(s->c, len) ? kChunkSmall : kChunkMin;
  const size_t max_tasks = entries / chunk_min + B + 1;
  const size_t groups = wide ? (max_runs + 255) / 256 : slots * ((B + 255) / 256);
  if (max_tasks >= kTaskIndexEnd) return PLK_E_ARG;  // task records: partial index bits
  int st;
  const size_t hb = wide ? NC : B;  // histogram bins: coarse bins or buckets
  if ((st = w.counts.alloc(slots * hb * 4))) return st;
  if ((st = w.offsets.alloc(slots * (B + 1) * 4))) return st;
  if ((st = w.task_off.alloc(slots * (B + 1) * 4))) return st;
  if ((st = w.blockhist.alloc(slots * kHistBlocksMax * hb * 4))) return st;
  if ((st = w.full_off.alloc(slots * B * 4))) return st;
  if ((st = w.len_cur.alloc(slots * kChunkMax * 4))) return st;
  if ((st = w.sorted.alloc(slots * (entries + 1) * 4))) return st;
  if ((st = w.tasks.alloc(slots * max_tasks * sizeof(uint2)))) return st;
  if ((st = w.partials.alloc(slots * max_tasks * sizeof(G1xyzz)))) return st;
  if (wide) {
    if ((st = w.tmp.alloc(slots * entries * sizeof(uint2)))) return st;
    if (s->naf && (st = w.naf.alloc(slots * entries * 4))) return st;
    if ((st = w.task_rel.alloc(slots * B * 4))) return st;
    if ((st = w.bin_tot.alloc(slots * 2 * NC * 4))) return st;
    if ((st = w.len_fill.alloc(slots * kChunkMax * 4))) return st;
    if ((st = w.coarse_off.alloc(slots * (NC + 1) * 4))) return st;
    if ((st = w.rsum.alloc(slots * B * sizeof(G1xyzz)))) return st;
    if ((st = w.ys.alloc(max_runs * sizeof(G1xyzz)))) return st;
    if ((st = w.zs.alloc(max_runs * sizeof(G1xyzz)))) return st;
  } else {
    if ((st = w.bsum.alloc(slots * B * sizeof(G1xyzz)))) return st;
  }
  if ((st = w.bits1.alloc(groups * kBitsumOut * sizeof(G1xyzz)))) return st;
  {  // k_bitsum1's fold counters: zero between batches (the last workgroup resets its slot's)
    void* before = w.done.ptr;
    if ((st = w.done.alloc(kMaxSlots * sizeof(uint32_t)))) return st;
    if (w.done.ptr != before) PLK_HIP_TRY(hipMemsetAsync(w.done.ptr, 0, kMaxSlots * sizeof(uint32_t), stream));
  }
  if (!w.guard.ptr) {  // k_guard's state: zero between batches
    if ((st = w.guard.alloc(2 * kMaxSlots * sizeof(uint32_t)))) return st;
    PLK_HIP_TRY(hipMemsetAsync(w.guard.ptr, 0, 2 * kMaxSlots * sizeof(uint32_t), stream));
  }
  {  // readback record: header (flags, entry counts) then the bit sums (nout <= 32 per slot),
     // in coherent mapped host memory (round 5: the per-batch copy dispatch it replaces cost
     // small proofs a dispatch per commit group). The previous batch has completed (every
     // batch ends with a host wait), so the host may clear it.
    void* before = w.host_out.ptr;
    if ((st = w.host_out.alloc(sizeof(ReadbackHeader) + (size_t)kMaxSlots * 32 * sizeof(G1xyzz),
                               hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable)))
      return st;
    if (w.host_out.ptr != before) {  // fresh memory: the flags start at generation 0
      std::memset(w.host_out.ptr, 0, sizeof(ReadbackHeader));
      w.gen = 0;
      PLK_HIP_TRY(hipHostGetDevicePointer(&w.out_dev, w.host_out.ptr, 0));
    }
  }
  if (!w.ev0) PLK_HIP_TRY(hipEventCreate(&w.ev0));
  if (!w.ev1) PLK_HIP_TRY(hipEventCreate(&w.ev1));
  if ((st = msm_sort_prepare(s->c))) return st;
  w.cap_len = len;
  w.cap_slots = slots;
  w.cap_chunk_min = chunk_min;
  w.cap_c = s->c;
  w.cap_windows = s->windows;
  w.task_stride = max_tasks;
  w.sorted_stride = entries + 1;
  w.naf_stride = entries;
  return PLK_OK;
}

// host tail: sum_j 2^j T_j (Horner) over a slot's nout bit sums T, then canonical affine. The
// device stages work in the R' domain (ffr.hpp) with values in [0, 2p): reduce and map back to
// R first.
static void host_tail(const MsmPlan& p, const G1xyzz* T, plk_g1* out) {
  const uint32_t nbits = p.nbits;
  G1xyzz acc = xyzz_infinity();
  // a part (b_lo = part B = part NR K, NR = 2^nbits runs): its buckets weigh b_lo + 1 + b',
  // i.e. + b_lo sum_b S_b = K 2^nbits part sum_r Y_r — part sum_r Y_r seeds the Horner
  // below, whose nbits doublings and the K below scale it
  if (p.wide && p.part) {
    const G1xyzz ysum = rx_to_r_domain(T[nbits + 1]);
    for (int i = 31 - __builtin_clz(p.part); i >= 0; --i) {
      acc = xyzz_dbl(acc);
      if ((p.part >> i) & 1u) acc = xyzz_add(acc, ysum);
    }
  }
  for (int j = (int)nbits - 1; j >= 0; --j) {
    acc = xyzz_dbl(acc);
    acc = xyzz_add(acc, rx_to_r_domain(T[j]));
  }
  if (p.wide) {  // over the runs: K (sum_r (r + 1) Y_r - sum_r Y_r) + sum_r T_r (k_runsum2)
    G1xyzz a = rx_to_r_domain(T[nbits + 1]);
    a.Y = fe_neg(a.Y);
    acc = xyzz_add(acc, a);
    for (uint32_t i = 0; i < p.rb; ++i) acc = xyzz_dbl(acc);
    acc = xyzz_add(acc, rx_to_r_domain(T[nbits]));
  }
  // row-table layout (wide sets only): bucket k holds the digits +-(2 k + 1), so the sum is
  // sum_k (2 (k + 1) - 1) B_k = 2 acc - sum_r Y_r, for a part over its own buckets alike
  if (p.naf) {
    G1xyzz y = rx_to_r_domain(T[nbits + 1]);
    y.Y = fe_neg(y.Y);
    acc = xyzz_add(xyzz_dbl(acc), y);
  }
  Fp x, y;
  const bool fin = xyzz_to_affine(acc, x, y);
  g1_store(x, y, fin, out);
}

// Runs `count` independent MSMs on the same SRS as one batch. For slot k: scalars
// d_scalars[k][0 .. lens[k]) (lens[k] <= n_srs) against the SRS prefix, and if
// check_lens[k] > lens[k] the tail [lens[k], check_lens[k]) must be zero (else that slot
// reports PLK_E_DEGREE). statuses[k] receives each slot's status.
int msm_run_batch(plk_srs* s, MsmWorkspace& w, const Fr* const* d_scalars, const size_t* lens,
                  const size_t* check_lens, size_t count, plk_g1* outs, int* statuses,
                  hipStream_t stream, uint32_t part, uint32_t parts, uint32_t guard_limit,
                  MsmSlotInfo* info) {
  if (count == 0) return PLK_OK;
  if (count > kMaxSlots) return PLK_E_ARG;
  if (!msm_parts_ok(s, parts) || part >= parts) return PLK_E_ARG;
  const uint32_t slots = (uint32_t)count;
  size_t max_len = 0;
  MsmBatch batch{};
  for (size_t k = 0; k < count; ++k) {
    if (lens[k] > s->n) return PLK_E_ARG;
    batch.scalars[k] = d_scalars[k];
    batch.len[k] = (uint32_t)lens[k];
    batch.check_len[k] = check_lens ? check_lens[k] : lens[k];
    max_len = std::max(max_len, lens[k]);
  }
  // the workspace first: the plan's task-length floor is the one its buffers were sized for
  int st;
  if ((st = ws_reserve(s, w, max_len ? max_len : 1, slots, stream))) return st;
  MsmPlan p;
  if ((st = msm_plan(s, w, batch, slots, max_len, part, parts, guard_limit, p))) return st;
  if (p.max_tasks_used + 1 > w.task_stride) return PLK_E_DEVICE;  // sizing invariant (ws_reserve)

  if (++w.gen == 0xFFFFFFFFu) {  // wrap: clear the stamps once every 2^32 - 1 batches
    std::memset(w.host_out.ptr, 0, sizeof(ReadbackHeader));
    w.gen = 1;
  }
  const uint32_t gen = p.gen = w.gen;
  w.last = p;

  if ((st = msm_sort(p, batch, w, stream))) return st;
  // start / stop events stamped by the dispatch itself (its execution, as rocprofv3 times
  // it), not by the stream: with several lanes on the GPU a stream event would also count
  // the time the kernel waits behind other lanes' kernels
  launch_accumulate(p.has_inf, p.lone, dim3(p.acc_blocks, slots), stream, w.ev0, w.ev1,
                    w.tasks.as<uint2>(), w.task_off.as<uint32_t>(), p.B, (uint64_t)w.task_stride,
                    w.sorted.as<uint32_t>(), (uint64_t)w.sorted_stride, s->table.as<G1Affine>(),
                    s->table_inf.as<uint8_t>(), w.partials.as<G1xyzz>());
  msm_reduce(p, w, stream);
  PLK_HIP_TRY(hipGetLastError());

  // the readback record (flags, entry counts, then the slots' bit sums) is in host memory
  // once the batch's kernels have completed
  const ReadbackHeader* hdr = w.host_out.as<ReadbackHeader>();
  const G1xyzz* T = reinterpret_cast<const G1xyzz*>(hdr + 1);
  PLK_HIP_TRY(stream_wait(stream));
  const uint32_t* ent = hdr->entries;
  uint32_t flag[kMaxSlots];
  for (uint32_t k = 0; k < slots; ++k) flag[k] = hdr->flag[k] == gen ? 1u : 0u;
  MsmStats& stt = w.stats;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, w.ev0, w.ev1) == hipSuccess) stt.last_accumulate_ms = ms;
  // a guarded slot over the limit ran no additions (k_guard cleared its tasks); its output is void
  bool hot[kMaxSlots] = {};
  for (uint32_t k = 0; k < slots; ++k) {
    hot[k] = guard_limit && hdr->max_count[k] > guard_limit;
    if (info) info[k] = MsmSlotInfo{ent[k], guard_limit ? hdr->max_count[k] : 0u, hot[k]};
  }
  stt.last_point_adds = 0;
  for (uint32_t k = 0; k < slots; ++k) stt.last_point_adds += hot[k] ? 0u : ent[k];
  stt.last_slots = slots;
  stt.cum_accumulate_ms += stt.last_accumulate_ms;
  stt.cum_launches += 1;
  stt.cum_point_adds += stt.last_point_adds;
  for (uint32_t k = 0; k < slots; ++k) stt.cum_points += batch.len[k];

  int overall = PLK_OK;
  for (uint32_t k = 0; k < slots; ++k) {
    plk_g1* out = &outs[k];
    if (flag[k]) {
      *out = plk_g1{};
      if (statuses) statuses[k] = PLK_E_DEGREE;
      if (overall == PLK_OK) overall = PLK_E_DEGREE;
      continue;
    }
    if (hot[k]) {  // the caller commits this slot another way (info[k].hot)
      *out = plk_g1{};
      if (statuses) statuses[k] = PLK_OK;
      continue;
    }
    host_tail(p, &T[(size_t)k * p.nout], out);
    if (statuses) statuses[k] = PLK_OK;
  }
  return overall;
}

int msm_run(plk_srs* s, const Fr* d_scalars, size_t len, size_t check_len, plk_g1* out,
            hipStream_t stream) {
  return msm_run_batch(s, *s->ws, &d_scalars, &len, &check_len, 1, out, nullptr, stream);
}

MsmWorkspace* msm_workspace_new() { return new MsmWorkspace(); }
void msm_workspace_delete(MsmWorkspace* w) { delete w; }
const MsmStats& msm_workspace_stats(const MsmWorkspace& w) { return w.stats; }
MsmStats& msm_workspace_stats(MsmWorkspace& w) { return w.stats; }

}  // namespace plk

plk_srs::plk_srs() = default;
plk_srs::~plk_srs() = default;
