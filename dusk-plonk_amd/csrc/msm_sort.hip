// msm_sort.hip — the fixed-base MSM's counting sort by bucket (design: msm.hip): every digit
// of a batch's scalars becomes an entry code in bucket order (`sorted`, `offsets`), and the
// buckets are cut into k_accumulate's task records (`tasks`, `task_off`). Three paths, chosen
// by the batch's plan (msm_plan, msm.hip): one dispatch for small batches (k_sort_one), LDS
// histograms for narrow bucket sets, a two-level radix sort for wide ones; k_block_scan serves
// the last two. Beside them the commit degree check (k_any_nonzero) and the hot-bucket guard
// (k_guard). msm_sort() at the end launches a batch's sort.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "internal.hpp"
#include "msm_common.hpp"
#include "msm_digits.hpp"

namespace plk {

namespace {

constexpr uint32_t kHistThreads = 1024;

// Pass 1: LDS histogram of this workgroup's digits, written whole to
// blockhist[slot][blk][b] (no global atomics).
template <uint32_t C>
__global__ void __launch_bounds__(kHistThreads) k_hist(MsmBatch batch, MsmCfg cfg,
                                                       uint32_t* __restrict__ blockhist) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
  const uint32_t slot = blockIdx.y, B = cfg.B;
  uint32_t i0, i1;
  slot_range(batch.len[slot], i0, i1);
  const Fr* sc = batch.scalars[slot];
  uint32_t* out = blockhist + ((size_t)slot * gridDim.x + blockIdx.x) * B;
  for (uint32_t b0 = 0; b0 < B; b0 += kLdsBuckets) {
    const uint32_t nb = min(kLdsBuckets, B - b0);
    for (uint32_t b = threadIdx.x; b < nb; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    for_scalars(sc, i0, i1, threadIdx.x, blockDim.x, [&](uint32_t, const Fr& s, bool) {
      each_digit<C>(s, cfg, [&](uint32_t, int d) {
        const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u - b0;  // wraps for d == 0
        if (d != 0 && b < nb) atomicAdd(&hist[b], 1u);
      });
    });
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nb; b += blockDim.x) out[b0 + b] = hist[b];
    __syncthreads();
  }
}

// Inclusive scan over the workgroup's nt threads of the three per-thread sums the task layout
// needs (entries, tasks, full tasks), in place in LDS; both barriers inside every step.
__device__ __forceinline__ void scan3_incl(uint32_t* s_c, uint32_t* s_t, uint32_t* s_f, uint32_t tid,
                                           uint32_t nt) {
  for (uint32_t off = 1; off < nt; off <<= 1) {
    const uint32_t a = tid >= off ? s_c[tid - off] : 0, t = tid >= off ? s_t[tid - off] : 0;
    const uint32_t f = tid >= off ? s_f[tid - off] : 0;
    __syncthreads();
    s_c[tid] += a;
    s_t[tid] += t;
    s_f[tid] += f;
    __syncthreads();
  }
}

// Per bucket, over the histogram workgroups: blockhist becomes the exclusive running count
// (each workgroup's first position inside the bucket) and counts[b] the bucket total.
// Workgroup (0, slot) also clears the slot's kChunkMax-word counters zero_a / zero_b when
// given (the wide path's tail-length counters, used by k_fine and k_make_tasks_wide) — two
// memset dispatches fewer per batch.
__global__ void k_block_scan(uint32_t* __restrict__ blockhist, uint32_t nblk, uint32_t B,
                             uint32_t* __restrict__ counts, uint32_t* __restrict__ zero_a,
                             uint32_t* __restrict__ zero_b) {
  const uint32_t slot = blockIdx.y;
  if (blockIdx.x == 0 && zero_a) {  // a loop: kChunkMax (PLK_CHUNK_MAX) may exceed the block
    for (uint32_t l = threadIdx.x; l < (uint32_t)kChunkMax; l += blockDim.x) {
      zero_a[(size_t)slot * kChunkMax + l] = 0;
      zero_b[(size_t)slot * kChunkMax + l] = 0;
    }
  }
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  uint32_t* h = blockhist + (size_t)slot * nblk * B + b;
  uint32_t run = 0, k = 0;
  for (; k + 8 <= nblk; k += 8) {  // 8 loads in flight before the stores
    uint32_t v[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) v[u] = h[(size_t)(k + u) * B];
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
      h[(size_t)(k + u) * B] = run;
      run += v[u];
    }
  }
  for (; k < nblk; ++k) {
    const uint32_t v = h[(size_t)k * B];
    h[(size_t)k * B] = run;
    run += v;
  }
  counts[(size_t)slot * B + b] = run;
}

// single workgroup per slot: offsets = exclusive scan(counts),
// task_off = exclusive scan(ceil(count / CH)) (where each bucket's partial sums go), and the
// EXECUTION order of the tasks: all full tasks (CH entries) first in bucket order, then the
// partial tails grouped by length, longest first, so that a wavefront's lanes run tasks of
// (nearly) the same length. len_cur[slot][l] = first execution slot of the tails of length l.
// The counts are staged in LDS first (dynamic, B words; one coalesced pass): the two walks
// over each thread's contiguous buckets then read LDS instead of issuing one dependent
// global load per bucket.
__global__ void __launch_bounds__(1024) k_scan_buckets(const uint32_t* __restrict__ counts_g,
                                                       uint32_t B, uint32_t chunk,
                                                       uint32_t* __restrict__ offsets,
                                                       uint32_t* __restrict__ task_off,
                                                       uint32_t* __restrict__ full_off,
                                                       uint32_t* __restrict__ len_cur) {
  __shared__ uint32_t s_cnt[1024], s_tsk[1024], s_full[1024], s_len[kChunkMax];
  extern __shared__ __attribute__((aligned(16))) uint32_t counts[];
  const uint32_t slot = blockIdx.y;
  counts_g += (size_t)slot * B;
  for (uint32_t b = threadIdx.x; b < B; b += blockDim.x) counts[b] = counts_g[b];
  offsets += (size_t)slot * (B + 1);
  task_off += (size_t)slot * (B + 1);
  full_off += (size_t)slot * B;
  len_cur += (size_t)slot * kChunkMax;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  if (tid < kChunkMax) s_len[tid] = 0;
  __syncthreads();
  const uint32_t per = (B + nt - 1) / nt;
  const uint32_t b0 = tid * per;
  uint32_t c_sum = 0, t_sum = 0, f_sum = 0;
  for (uint32_t b = b0; b < b0 + per && b < B; ++b) {
    const uint32_t c = counts[b];
    c_sum += c;
    t_sum += (c + chunk - 1) / chunk;
    f_sum += c / chunk;
    if (c % chunk) atomicAdd(&s_len[c % chunk], 1u);
  }
  s_cnt[tid] = c_sum;
  s_tsk[tid] = t_sum;
  s_full[tid] = f_sum;
  __syncthreads();
  scan3_incl(s_cnt, s_tsk, s_full, tid, nt);
  uint32_t c_run = s_cnt[tid] - c_sum, t_run = s_tsk[tid] - t_sum, f_run = s_full[tid] - f_sum;
  for (uint32_t b = b0; b < b0 + per && b < B; ++b) {
    offsets[b] = c_run;
    task_off[b] = t_run;
    full_off[b] = f_run;
    c_run += counts[b];
    t_run += (counts[b] + chunk - 1) / chunk;
    f_run += counts[b] / chunk;
  }
  if (tid == nt - 1) {
    offsets[B] = s_cnt[tid];
    task_off[B] = s_tsk[tid];
  }
  if (tid == 0) {  // tails after the full tasks, longest first
    uint32_t run = s_full[nt - 1];
    for (uint32_t l = chunk - 1; l >= 1; --l) {
      len_cur[l] = run;
      run += s_len[l];
    }
  }
}

// Pass 2: this workgroup's positions start at offsets[b] + blockhist[slot][blk][b]; each
// digit takes the next one with an LDS atomic (bucket windows as in k_hist).
template <uint32_t C>
__global__ void __launch_bounds__(kHistThreads) k_scatter(MsmBatch batch, MsmCfg cfg,
                                                          uint64_t n_srs,
                                                          const uint32_t* __restrict__ offsets,
                                                          const uint32_t* __restrict__ blockhist,
                                                          uint32_t* __restrict__ sorted,
                                                          uint64_t sorted_stride) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
  const uint32_t slot = blockIdx.y, B = cfg.B;
  const uint32_t* off = offsets + (size_t)slot * (B + 1);
  const uint32_t* bh = blockhist + ((size_t)slot * gridDim.x + blockIdx.x) * B;
  uint32_t i0, i1;
  slot_range(batch.len[slot], i0, i1);
  const Fr* sc = batch.scalars[slot];
  uint32_t* out = sorted + (size_t)slot * sorted_stride;
  for (uint32_t b0 = 0; b0 < B; b0 += kLdsBuckets) {
    const uint32_t nb = min(kLdsBuckets, B - b0);
    for (uint32_t b = threadIdx.x; b < nb; b += blockDim.x) hist[b] = off[b0 + b] + bh[b0 + b];
    __syncthreads();
    for_scalars(sc, i0, i1, threadIdx.x, blockDim.x, [&](uint32_t i, const Fr& s, bool neg) {
      each_digit<C>(s, cfg, [&](uint32_t w, int d) {
        const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u - b0;
        if (d != 0 && b < nb) {
          const uint32_t pos = atomicAdd(&hist[b], 1u);
          out[pos] = entry_code((uint32_t)(w * n_srs + i), (d < 0) != neg);
        }
      });
    });
    __syncthreads();
  }
}

// Task t of bucket b covers sorted[offsets[b] + t*CH, ...+CH) and writes its partial sum to
// partials[task_off[b] + t]; its execution slot is full_off[b] + t for a full task, or the
// next slot of its length class for the tail. tasks[slot] = task_record(first entry, partial
// index, length) (msm_common.hpp).
__global__ void k_make_tasks(const uint32_t* __restrict__ offsets,
                             const uint32_t* __restrict__ task_off,
                             const uint32_t* __restrict__ full_off, uint32_t* __restrict__ len_cur,
                             uint32_t B, uint32_t chunk, uint2* __restrict__ tasks,
                             uint64_t task_stride) {
  // tails: ranks inside the workgroup from LDS atomics, one global atomic per (workgroup,
  // length) for the base
  __shared__ uint32_t s_cnt[kChunkMax], s_base[kChunkMax];
  const uint32_t slot = blockIdx.y, tid = threadIdx.x;
  const uint32_t b = blockIdx.x * blockDim.x + tid;
  for (uint32_t l = tid; l < kChunkMax; l += blockDim.x) s_cnt[l] = 0;
  __syncthreads();
  offsets += (size_t)slot * (B + 1);
  task_off += (size_t)slot * (B + 1);
  tasks += (size_t)slot * task_stride;
  uint32_t start = 0, t0 = 0, nfull = 0, tail = 0, rank = 0;
  if (b < B) {
    start = offsets[b];
    const uint32_t cnt = offsets[b + 1] - start;
    t0 = task_off[b];
    nfull = cnt / chunk;
    tail = cnt - nfull * chunk;
    if (tail) rank = atomicAdd(&s_cnt[tail], 1u);
  }
  __syncthreads();
  for (uint32_t l = tid; l < kChunkMax; l += blockDim.x)
    if (s_cnt[l]) s_base[l] = atomicAdd(&len_cur[(size_t)slot * kChunkMax + l], s_cnt[l]);
  __syncthreads();
  if (b >= B) return;
  uint32_t x = full_off[(size_t)slot * B + b];
  for (uint32_t t = 0; t < nfull; ++t, ++x) tasks[x] = task_record(start + t * chunk, t0 + t, chunk);
  if (tail) tasks[s_base[tail] + rank] = task_record(start + nfull * chunk, t0 + nfull, tail);
}

// Small bucket sets (B <= kSortSmallMax: the 2^12-size commits, c <= 13) in ONE dispatch per
// batch instead of three: k_block_scan + k_scan_buckets + k_make_tasks on one workgroup per
// slot (the bucket counts and the tail-length cursors in LDS, so the tail ranks need no global
// atomics). Small proofs are bound by the rate at which the command processor takes
// dispatches, not by these kernels' work. The task layout is k_make_tasks' (full
// tasks in bucket order, then the tails grouped by length, longest first).
__global__ void __launch_bounds__(1024) k_sort_small(uint32_t* __restrict__ blockhist, uint32_t nblk,
                                                     uint32_t B, uint32_t chunk,
                                                     uint32_t* __restrict__ offsets,
                                                     uint32_t* __restrict__ task_off,
                                                     uint2* __restrict__ tasks, uint64_t task_stride) {
  __shared__ uint32_t s_count[kSortSmallMax];
  __shared__ uint32_t s_c[1024], s_t[1024], s_f[1024], s_len[kChunkMax], s_cur[kChunkMax];
  const uint32_t slot = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  blockhist += (size_t)slot * nblk * B;
  offsets += (size_t)slot * (B + 1);
  task_off += (size_t)slot * (B + 1);
  tasks += (size_t)slot * task_stride;
  if (tid < kChunkMax) s_len[tid] = 0;
  // per bucket, over the histogram workgroups: exclusive running counts (k_block_scan)
  for (uint32_t b = tid; b < B; b += nt) {
    uint32_t* h = blockhist + b;
    uint32_t run = 0, k = 0;
    for (; k + 8 <= nblk; k += 8) {
      uint32_t v[8];
#pragma unroll
      for (uint32_t u = 0; u < 8; ++u) v[u] = h[(size_t)(k + u) * B];
#pragma unroll
      for (uint32_t u = 0; u < 8; ++u) {
        h[(size_t)(k + u) * B] = run;
        run += v[u];
      }
    }
    for (; k < nblk; ++k) {
      const uint32_t v = h[(size_t)k * B];
      h[(size_t)k * B] = run;
      run += v;
    }
    s_count[b] = run;
  }
  __syncthreads();
  // offsets / task offsets / full-task offsets over each thread's contiguous buckets
  // (k_scan_buckets)
  const uint32_t per = (B + nt - 1) / nt;
  const uint32_t b0 = min(tid * per, B), b1 = min(b0 + per, B);
  uint32_t c_sum = 0, t_sum = 0, f_sum = 0;
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t c = s_count[b];
    c_sum += c;
    t_sum += (c + chunk - 1) / chunk;
    f_sum += c / chunk;
    if (c % chunk) atomicAdd(&s_len[c % chunk], 1u);
  }
  s_c[tid] = c_sum;
  s_t[tid] = t_sum;
  s_f[tid] = f_sum;
  __syncthreads();
  for (uint32_t off = 1; off < nt; off <<= 1) {
    const uint32_t a = tid >= off ? s_c[tid - off] : 0, t = tid >= off ? s_t[tid - off] : 0;
    const uint32_t f = tid >= off ? s_f[tid - off] : 0;
    __syncthreads();
    s_c[tid] += a;
    s_t[tid] += t;
    s_f[tid] += f;
    __syncthreads();
  }
  if (tid == 0) {  // tails after the full tasks, longest first
    uint32_t run = s_f[nt - 1];
    for (uint32_t l = chunk - 1; l >= 1; --l) {
      s_cur[l] = run;
      run += s_len[l];
    }
    offsets[B] = s_c[nt - 1];
    task_off[B] = s_t[nt - 1];
  }
  __syncthreads();
  // the task records (k_make_tasks), tail ranks from LDS cursors
  uint32_t c_run = s_c[tid] - c_sum, t_run = s_t[tid] - t_sum, f_run = s_f[tid] - f_sum;
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t cnt = s_count[b];
    offsets[b] = c_run;
    task_off[b] = t_run;
    const uint32_t nfull = cnt / chunk, tail = cnt - nfull * chunk;
    for (uint32_t t = 0; t < nfull; ++t) tasks[f_run + t] = task_record(c_run + t * chunk, t_run + t, chunk);
    if (tail) tasks[atomicAdd(&s_cur[tail], 1u)] = task_record(c_run + nfull * chunk, t_run + nfull, tail);
    c_run += cnt;
    t_run += (cnt + chunk - 1) / chunk;
    f_run += nfull;
  }
}

// Small batches (B <= kSortSmallMax and at most kSortOneMax scalars per slot: the 2^12-size
// proofs' commits) sorted in ONE dispatch (round 4: one workgroup per slot; round 5: a few,
// split by bucket range, below) instead of three (k_hist,
// k_sort_small, k_scatter) or four (with k_any_nonzero): the commit degree check, an LDS
// histogram over all of the slot's digits, the scans and task records of k_sort_small, then
// the scatter with LDS cursors. Small proofs are bound by the command processor's dispatch
// rate, so the dispatches matter more than the single workgroup's latency. The
// order of the entries inside a bucket differs from the multi-workgroup sort; the bucket's
// sum (exact XYZZ arithmetic, canonical affine result) does not.
// Measured (profiles/r04_sortone_runsum_shoup_ab.jsonl, one box, interleaved): 2^12 proofs
// 7.48 / 7.84 against 7.05 / 7.45 M constraints/s with the multi-dispatch sort.
// Round 4 also measured the 2^14-size proofs' commits (c = 15: 2^14 buckets, ~2^14 scalars
// per slot) through one workgroup re-reading the scalars for the scatter: no faster
// (profiles/r04_sort_one_big_ab.jsonl; removed in round 5).
// kSortOneMax, kSortOneParts and kSortOneBig (HOLD's bounds): msm_common.hpp.
template <uint32_t C, bool HOLD>
__global__ void __launch_bounds__(1024) k_sort_one(MsmBatch batch, MsmCfg cfg, uint64_t n_srs,
                                                   uint32_t chunk, uint32_t* __restrict__ sorted,
                                                   uint64_t sorted_stride,
                                                   uint32_t* __restrict__ offsets,
                                                   uint32_t* __restrict__ task_off,
                                                   uint2* __restrict__ tasks, uint64_t task_stride,
                                                   uint32_t* __restrict__ flag, uint32_t gen) {
  // Workgroup x of the slot's gridDim.x owns buckets [bl, bh): every workgroup histograms ALL
  // the slot's digits (LDS atomics; the offsets of its range follow from the counts below it,
  // so no workgroup waits for another), then writes the task records and scatters the
  // entries of its own range only — the scattered 4-byte stores, which one CU's memory path
  // took most of the kernel's time for, spread over gridDim.x CUs.
  __shared__ uint32_t s_count[kSortSmallMax];
  __shared__ uint32_t s_c[1024], s_t[1024], s_f[1024], s_len[kChunkMax], s_cur[kChunkMax],
      s_pre[kChunkMax];
  const uint32_t slot = blockIdx.y, tid = threadIdx.x, nt = 1024, B = cfg.B;  // blockDim.x
  const uint32_t bpart = B / gridDim.x;  // B and gridDim.x powers of two, B >= gridDim.x
  const uint32_t bl = blockIdx.x * bpart, bh = bl + bpart;
  const uint32_t len = batch.len[slot];
  const Fr* sc = batch.scalars[slot];
  offsets += (size_t)slot * (B + 1);
  task_off += (size_t)slot * (B + 1);
  tasks += (size_t)slot * task_stride;
  uint32_t* out = sorted + (size_t)slot * sorted_stride;
  // the commit's degree check (k_any_nonzero): a nonzero scalar in [len, check_len)
  if (blockIdx.x == 0)
    for (uint64_t i = (uint64_t)len + tid; i < batch.check_len[slot]; i += nt)
      if (!fe_is_zero(ld_fr(&sc[i]))) flag[slot] = gen;  // every writer stores the same value
  for (uint32_t b = tid; b < B; b += nt) s_count[b] = 0;
  for (uint32_t l = tid; l < kChunkMax; l += nt) s_len[l] = s_pre[l] = 0;
  __syncthreads();
  // HOLD: this thread's scalars (i = tid + k nt, at most kSortOneMax / 1024 of them), brought
  // to [0, (r-1)/2] once and kept in registers for both passes
  constexpr uint32_t kPer = HOLD ? kSortOneMax / 1024 : 1;
  Fr sv[kPer];
  bool sneg[kPer];
  auto hist_digits = [&](const Fr& x) {
    each_digit<C>(x, cfg, [&](uint32_t, int d) {
      if (d != 0) atomicAdd(&s_count[(uint32_t)(d < 0 ? -d : d) - 1u], 1u);
    });
  };
  if constexpr (HOLD) {
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t i = tid + k * nt;
      sneg[k] = false;
      if (i < len) sv[k] = scalar_half(&sc[i], sneg[k]);
    }
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {  // histogram of every digit of the slot
      if (tid + k * nt >= len) break;
      hist_digits(sv[k]);
    }
  } else {
    for_scalars(sc, 0, len, tid, nt, [&](uint32_t, const Fr& x, bool) { hist_digits(x); });
  }
  __syncthreads();
  // offsets / task offsets / full-task offsets over each thread's contiguous buckets (all B:
  // every workgroup derives the same global layout), the tail-length counts over all buckets
  // and over the buckets below this workgroup's range (its tail ranks start after those)
  const uint32_t per = (B + nt - 1) / nt;
  const uint32_t b0 = min(tid * per, B), b1 = min(b0 + per, B);
  uint32_t c_sum = 0, t_sum = 0, f_sum = 0;
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t c = s_count[b];
    c_sum += c;
    t_sum += (c + chunk - 1) / chunk;
    f_sum += c / chunk;
    if (c % chunk) {
      atomicAdd(&s_len[c % chunk], 1u);
      if (b < bl) atomicAdd(&s_pre[c % chunk], 1u);
    }
  }
  s_c[tid] = c_sum;
  s_t[tid] = t_sum;
  s_f[tid] = f_sum;
  __syncthreads();
  scan3_incl(s_c, s_t, s_f, tid, nt);
  if (tid == 0) {  // tails after the full tasks, longest first; this range's after those below
    uint32_t run = s_f[nt - 1];
    for (uint32_t l = chunk - 1; l >= 1; --l) {
      s_cur[l] = run + s_pre[l];
      run += s_len[l];
    }
    if (blockIdx.x == 0) {
      offsets[B] = s_c[nt - 1];
      task_off[B] = s_t[nt - 1];
    }
  }
  __syncthreads();
  uint32_t c_run = s_c[tid] - c_sum, t_run = s_t[tid] - t_sum, f_run = s_f[tid] - f_sum;
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t cnt = s_count[b];
    if (b >= bl && b < bh) {
      s_count[b] = c_run;
      offsets[b] = c_run;
      task_off[b] = t_run;
      const uint32_t nfull = cnt / chunk, tail = cnt - nfull * chunk;
      for (uint32_t t = 0; t < nfull; ++t) tasks[f_run + t] = task_record(c_run + t * chunk, t_run + t, chunk);
      if (tail) tasks[atomicAdd(&s_cur[tail], 1u)] = task_record(c_run + nfull * chunk, t_run + nfull, tail);
    }
    c_run += cnt;
    t_run += (cnt + chunk - 1) / chunk;
    f_run += cnt / chunk;
  }
  __syncthreads();
  auto scatter_digits = [&](const Fr& x, bool neg, uint32_t i) {
    each_digit<C>(x, cfg, [&](uint32_t w, int d) {
      const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u;  // d = 0: wraps past bh
      if (b - bl < bpart) {
        const uint32_t pos = atomicAdd(&s_count[b], 1u);
        out[pos] = entry_code((uint32_t)(w * n_srs + i), (d < 0) != neg);
      }
    });
  };
  if constexpr (HOLD) {
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {  // scatter (k_scatter) of this workgroup's buckets
      const uint32_t i = tid + k * nt;
      if (i >= len) break;
      scatter_digits(sv[k], sneg[k], i);
    }
  } else {
    for_scalars(sc, 0, len, tid, nt,
                [&](uint32_t i, const Fr& x, bool neg) { scatter_digits(x, neg, i); });
  }
}

// ---- wide bucket sets (B > kLdsBuckets, c >= 17): two-level radix sort ----------------
// One LDS histogram cannot hold the buckets, and per-(workgroup, bucket) runs of ~1 entry
// make a direct scatter write-amplified. Instead: (1) coarse bins of kFine consecutive
// buckets — per-workgroup LDS histograms, a per-bin scan over the workgroups and a scatter
// of (code, bucket) pairs into bin order (runs of ~100 entries per (workgroup, bin));
// (2) one workgroup per bin counting-sorts its entries by bucket inside the bin's own
// region (LDS counters, writes that stay in one L2), emitting the bucket offsets and the
// per-bucket task counts on the way; (3) the task records, as k_make_tasks does.
// kFineBits, kFineBitsMin and kCoarseMax: msm_common.hpp.

// Exclusive scan over the workgroup of K values per thread (wave shuffles, then the wave
// totals through LDS); tot = the workgroup totals. sh: K * 32 words.
template <int K>
__device__ __forceinline__ void block_scan_excl(uint32_t (&v)[K], uint32_t (&tot)[K], uint32_t* sh) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint32_t inc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) inc[k] = v[k];
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t t = __shfl_up(inc[k], o, 64);
      if (lane >= o) inc[k] += t;
    }
  }
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k * 32 + wid] = inc[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    uint32_t base = 0, total = 0;
    for (uint32_t w = 0; w < nw; ++w) {
      const uint32_t s = sh[k * 32 + w];
      base += w < wid ? s : 0u;
      total += s;
    }
    v[k] = base + inc[k] - v[k];
    tot[k] = total;
  }
  __syncthreads();
}

// Wide pass 1: per-workgroup histogram of the coarse bins (bucket >> kFineBits), written whole
template <uint32_t C>
__global__ void __launch_bounds__(kHistThreads) k_chist(MsmBatch batch, MsmCfg cfg, uint32_t NC,
                                                        uint32_t fb, uint32_t* __restrict__ blockhist) {
  __shared__ uint32_t hist[kCoarseMax];
  const uint32_t slot = blockIdx.y;
  uint32_t i0, i1;
  slot_range(batch.len[slot], i0, i1);
  const Fr* sc = batch.scalars[slot];
  for (uint32_t b = threadIdx.x; b < NC; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  for_scalars(sc, i0, i1, threadIdx.x, blockDim.x, [&](uint32_t, const Fr& s, bool) {
    each_digit<C>(s, cfg, [&](uint32_t, int d) {
      const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u - cfg.b_lo;  // d = 0: wraps past B
      if (b < cfg.B) atomicAdd(&hist[b >> fb], 1u);
    });
  });
  __syncthreads();
  uint32_t* out = blockhist + ((size_t)slot * gridDim.x + blockIdx.x) * NC;
  for (uint32_t b = threadIdx.x; b < NC; b += blockDim.x) out[b] = hist[b];
}

// Wide pass 2 (after k_block_scan over the bins): every workgroup scans the bin totals into
// bin offsets (workgroup 0 also stores them), then each digit's (code, bucket) takes the next
// slot of its bin in this workgroup's range.
template <uint32_t C>
__global__ void __launch_bounds__(kHistThreads) k_cscatter(MsmBatch batch, MsmCfg cfg, uint32_t NC,
                                                           uint32_t fb, uint64_t n_srs,
                                                           const uint32_t* __restrict__ ccounts,
                                                           const uint32_t* __restrict__ blockhist,
                                                           uint32_t* __restrict__ coarse_off,
                                                           uint2* __restrict__ tmp, uint64_t tmp_stride) {
  __shared__ uint32_t hist[kCoarseMax];
  __shared__ uint32_t sh[32];
  const uint32_t slot = blockIdx.y, tid = threadIdx.x;
  const uint32_t* cc = ccounts + (size_t)slot * NC;
  const uint32_t* bh = blockhist + ((size_t)slot * gridDim.x + blockIdx.x) * NC;
  uint32_t* co = coarse_off + (size_t)slot * (NC + 1);
  uint32_t loc[4], v[1], tot[1];
  v[0] = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t b = 4 * tid + q;
    loc[q] = b < NC ? cc[b] : 0u;
    v[0] += loc[q];
  }
  block_scan_excl<1>(v, tot, sh);
  uint32_t run = v[0];
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t b = 4 * tid + q;
    if (b < NC) {
      if (blockIdx.x == 0) co[b] = run;
      hist[b] = run + bh[b];
    }
    run += loc[q];
  }
  if (blockIdx.x == 0 && tid == 0) co[NC] = tot[0];
  __syncthreads();
  uint32_t i0, i1;
  slot_range(batch.len[slot], i0, i1);
  const Fr* sc = batch.scalars[slot];
  uint2* out = tmp + (size_t)slot * tmp_stride;
  for_scalars(sc, i0, i1, tid, blockDim.x, [&](uint32_t i, const Fr& s, bool neg) {
    each_digit<C>(s, cfg, [&](uint32_t w, int d) {
      const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u - cfg.b_lo;  // d = 0: wraps past B
      if (b < cfg.B) {
        const uint32_t pos = atomicAdd(&hist[b >> fb], 1u);
        out[pos] = make_uint2(entry_code((uint32_t)(w * n_srs + i), (d < 0) != neg), b);
      }
    });
  });
}

// Wide pass 1 and 2 of the row-table layout (MsmPlan::naf; msm_digits.hpp naf_walk). Each scalar
// is recoded ONCE: k_chist_naf walks it, counts its digits' bins and leaves the digit words in
// naf[j * len + i] (W words per scalar, kNafNone after the last digit); k_cscatter_naf reads them
// back (the scalars not at all) and scatters (pos * n_srs + i | sign, bucket). A part keeps the
// digits of its bucket range, as the window layout's kernels do.
__global__ void __launch_bounds__(kHistThreads) k_chist_naf(MsmBatch batch, MsmCfg cfg, uint32_t NC,
                                                            uint32_t fb, uint32_t* __restrict__ blockhist,
                                                            uint32_t* __restrict__ naf, uint64_t naf_stride) {
  __shared__ uint32_t hist[kCoarseMax];
  const uint32_t slot = blockIdx.y, len = batch.len[slot];
  uint32_t i0, i1;
  slot_range(len, i0, i1);
  const Fr* sc = batch.scalars[slot];
  uint32_t* words = naf + (size_t)slot * naf_stride;
  for (uint32_t b = threadIdx.x; b < NC; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  for_scalars(sc, i0, i1, threadIdx.x, blockDim.x, [&](uint32_t i, const Fr& s, bool neg) {
    const uint32_t m = naf_walk(s, cfg, [&](uint32_t j, uint32_t word) {
      words[(size_t)j * len + i] = neg ? word ^ 0x80000000u : word;
      const uint32_t b = naf_bucket(word) - cfg.b_lo;  // below the part's range: wraps past B
      if (b < cfg.B) atomicAdd(&hist[b >> fb], 1u);
    });
    for (uint32_t j = m; j < cfg.W; ++j) words[(size_t)j * len + i] = kNafNone;
  });
  __syncthreads();
  uint32_t* out = blockhist + ((size_t)slot * gridDim.x + blockIdx.x) * NC;
  for (uint32_t b = threadIdx.x; b < NC; b += blockDim.x) out[b] = hist[b];
}

__global__ void __launch_bounds__(kHistThreads) k_cscatter_naf(MsmBatch batch, MsmCfg cfg, uint32_t NC,
                                                               uint32_t fb, uint64_t n_srs,
                                                               const uint32_t* __restrict__ ccounts,
                                                               const uint32_t* __restrict__ blockhist,
                                                               uint32_t* __restrict__ coarse_off,
                                                               uint2* __restrict__ tmp, uint64_t tmp_stride,
                                                               const uint32_t* __restrict__ naf,
                                                               uint64_t naf_stride) {
  __shared__ uint32_t hist[kCoarseMax];
  __shared__ uint32_t sh[32];
  const uint32_t slot = blockIdx.y, tid = threadIdx.x, len = batch.len[slot];
  const uint32_t* cc = ccounts + (size_t)slot * NC;
  const uint32_t* bh = blockhist + ((size_t)slot * gridDim.x + blockIdx.x) * NC;
  uint32_t* co = coarse_off + (size_t)slot * (NC + 1);
  uint32_t loc[4], v[1], tot[1];
  v[0] = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {  // the bin offsets, as k_cscatter
    const uint32_t b = 4 * tid + q;
    loc[q] = b < NC ? cc[b] : 0u;
    v[0] += loc[q];
  }
  block_scan_excl<1>(v, tot, sh);
  uint32_t run = v[0];
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t b = 4 * tid + q;
    if (b < NC) {
      if (blockIdx.x == 0) co[b] = run;
      hist[b] = run + bh[b];
    }
    run += loc[q];
  }
  if (blockIdx.x == 0 && tid == 0) co[NC] = tot[0];
  __syncthreads();
  uint32_t i0, i1;
  slot_range(len, i0, i1);
  const uint32_t* words = naf + (size_t)slot * naf_stride;
  uint2* out = tmp + (size_t)slot * tmp_stride;
  for (uint32_t i = i0 + tid; i < i1; i += blockDim.x) {
    uint32_t wv[kNafMaxW];  // every load in flight before the first atomic
#pragma unroll
    for (uint32_t j = 0; j < kNafMaxW; ++j) wv[j] = j < cfg.W ? words[(size_t)j * len + i] : kNafNone;
#pragma unroll
    for (uint32_t j = 0; j < kNafMaxW; ++j) {
      const uint32_t word = wv[j];
      const uint32_t b = naf_bucket(word) - cfg.b_lo;
      if (word != kNafNone && b < cfg.B) {
        const uint32_t pos = atomicAdd(&hist[b >> fb], 1u);
        out[pos] = make_uint2(entry_code((uint32_t)(naf_pos(word) * n_srs + i), naf_neg(word)), b);
      }
    }
  }
}

// Wide pass 3: one workgroup per (bin, slot), one thread per bucket of the bin. Counting sort
// of the bin's entries by bucket into its own region of `sorted`; bucket offsets (global),
// per-bucket task and full-task offsets relative to the bin, the bin's totals and the
// global histogram of tail lengths (for the execution order of the tasks).
// loads in flight per thread and pass (8 measured no faster in round 5:
// profiles/r05_sort_prefetch_readback_ab.jsonl)
constexpr uint32_t kFineLoads = 4;
template <uint32_t FB>
__global__ void __launch_bounds__(1u << FB) k_fine(uint32_t B, uint32_t NC, uint32_t chunk,
                                                const uint32_t* __restrict__ coarse_off,
                                                const uint2* __restrict__ tmp, uint64_t tmp_stride,
                                                uint32_t* __restrict__ sorted, uint64_t sorted_stride,
                                                uint32_t* __restrict__ offsets,
                                                uint32_t* __restrict__ task_rel,
                                                uint32_t* __restrict__ full_rel,
                                                uint32_t* __restrict__ bin_tot,
                                                uint32_t* __restrict__ len_count) {
  constexpr uint32_t kFine = 1u << FB;
  __shared__ uint32_t cnt[kFine];
  __shared__ uint32_t s_len[kChunkMax];
  __shared__ uint32_t sh[3 * 32];
  const uint32_t slot = blockIdx.y, bin = blockIdx.x, tid = threadIdx.x;
  const uint32_t lo = coarse_off[(size_t)slot * (NC + 1) + bin];
  const uint32_t hi = coarse_off[(size_t)slot * (NC + 1) + bin + 1];
  const uint2* in = tmp + (size_t)slot * tmp_stride;
  cnt[tid] = 0;
  if (tid < kChunkMax) s_len[tid] = 0;
  __syncthreads();
  {  // kFineLoads loads in flight per thread, then their atomics
    uint32_t e = lo + tid;
    for (; e + (kFineLoads - 1) * kFine < hi; e += kFineLoads * kFine) {
      uint32_t k[kFineLoads];
#pragma unroll
      for (uint32_t u = 0; u < kFineLoads; ++u) k[u] = in[e + u * kFine].y;
#pragma unroll
      for (uint32_t u = 0; u < kFineLoads; ++u) atomicAdd(&cnt[k[u] & (kFine - 1)], 1u);
    }
    for (; e < hi; e += kFine) atomicAdd(&cnt[in[e].y & (kFine - 1)], 1u);
  }
  __syncthreads();
  const uint32_t c = cnt[tid];
  if (c % chunk) atomicAdd(&s_len[c % chunk], 1u);
  uint32_t v[3] = {c, (c + chunk - 1) / chunk, c / chunk}, tot[3];
  block_scan_excl<3>(v, tot, sh);  // its barriers also order the s_len atomics and cnt reads
  const uint32_t b = bin * kFine + tid;  // B = NC * kFine
  offsets[(size_t)slot * (B + 1) + b] = lo + v[0];
  task_rel[(size_t)slot * B + b] = v[1];
  full_rel[(size_t)slot * B + b] = v[2];
  if (tid == 0) {
    bin_tot[(size_t)slot * 2 * NC + bin] = tot[1];
    bin_tot[(size_t)slot * 2 * NC + NC + bin] = tot[2];
    if (bin == NC - 1) offsets[(size_t)slot * (B + 1) + B] = hi;
  }
  if (tid < kChunkMax && s_len[tid]) atomicAdd(&len_count[(size_t)slot * kChunkMax + tid], s_len[tid]);
  cnt[tid] = v[0];  // cursor of bucket tid, relative to lo
  __syncthreads();
  uint32_t* out = sorted + (size_t)slot * sorted_stride + lo;
  uint32_t e = lo + tid;
  for (; e + (kFineLoads - 1) * kFine < hi; e += kFineLoads * kFine) {
    uint2 x[kFineLoads];
    uint32_t pos[kFineLoads];
#pragma unroll
    for (uint32_t u = 0; u < kFineLoads; ++u) x[u] = in[e + u * kFine];
#pragma unroll
    for (uint32_t u = 0; u < kFineLoads; ++u) pos[u] = atomicAdd(&cnt[x[u].y & (kFine - 1)], 1u);
#pragma unroll
    for (uint32_t u = 0; u < kFineLoads; ++u) out[pos[u]] = x[u].x;
  }
  for (; e < hi; e += kFine) {
    const uint2 x = in[e];
    out[atomicAdd(&cnt[x.y & (kFine - 1)], 1u)] = x.x;
  }
}

// Wide pass 4: task records in the layout of k_make_tasks (full tasks first, bucket order;
// tails grouped by length, longest first). Bin bases are sums of the bin totals below.
template <uint32_t FB>
__global__ void __launch_bounds__(1u << FB) k_make_tasks_wide(uint32_t B, uint32_t NC, uint32_t chunk,
                                                           const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ task_rel,
                                                           const uint32_t* __restrict__ full_rel,
                                                           const uint32_t* __restrict__ bin_tot,
                                                           const uint32_t* __restrict__ len_count,
                                                           uint32_t* __restrict__ len_fill,
                                                           uint32_t* __restrict__ task_off,
                                                           uint2* __restrict__ tasks,
                                                           uint64_t task_stride) {
  __shared__ uint32_t s_cnt[kChunkMax], s_base[kChunkMax], s_lc[kChunkMax], sh[4 * 32];
  const uint32_t slot = blockIdx.y, bin = blockIdx.x, tid = threadIdx.x;
  const uint32_t* bt = bin_tot + (size_t)slot * 2 * NC;
  uint32_t v[4] = {0, 0, 0, 0}, tot[4];
  for (uint32_t q = tid; q < NC; q += blockDim.x) {
    const uint32_t a = bt[q], f = bt[NC + q];
    v[0] += q < bin ? a : 0u;
    v[1] += q < bin ? f : 0u;
    v[2] += a;
    v[3] += f;
  }
  if (tid < kChunkMax) {
    s_cnt[tid] = 0;
    s_lc[tid] = len_count[(size_t)slot * kChunkMax + tid];
  }
  block_scan_excl<4>(v, tot, sh);
  const uint32_t task_base = tot[0], full_base = tot[1], task_total = tot[2], full_total = tot[3];
  const uint32_t b = (bin << FB) + tid;
  const uint32_t* off = offsets + (size_t)slot * (B + 1);
  const uint32_t start = off[b], cnt = off[b + 1] - start;
  const uint32_t t0 = task_base + task_rel[(size_t)slot * B + b];
  const uint32_t f0 = full_base + full_rel[(size_t)slot * B + b];
  task_off[(size_t)slot * (B + 1) + b] = t0;
  if (b == B - 1) task_off[(size_t)slot * (B + 1) + B] = task_total;
  const uint32_t nfull = cnt / chunk, tail = cnt - nfull * chunk;
  uint32_t rank = 0;
  if (tail) rank = atomicAdd(&s_cnt[tail], 1u);
  __syncthreads();
  if (tid < kChunkMax && s_cnt[tid]) {
    uint32_t base = full_total;  // tails of length l start after all longer tails
    for (uint32_t l = tid + 1; l < kChunkMax; ++l) base += s_lc[l];
    s_base[tid] = base + atomicAdd(&len_fill[(size_t)slot * kChunkMax + tid], s_cnt[tid]);
  }
  __syncthreads();
  tasks += (size_t)slot * task_stride;
  for (uint32_t t = 0; t < nfull; ++t) tasks[f0 + t] = task_record(start + t * chunk, t0 + t, chunk);
  if (tail) tasks[s_base[tail] + rank] = task_record(start + nfull * chunk, t0 + nfull, tail);
}

// flag[slot] = gen if any scalar in [len, check_len) is nonzero (commit degree check). The
// flags are stamped with the batch's generation number instead of being cleared per batch:
// a stale flag holds an older generation, so no memset dispatch is needed. Every writer
// stores the same value, so a plain store does (no atomic: the flags live in mapped host
// memory, where an atomic would need the platform's PCIe atomics).
__global__ void k_any_nonzero(MsmBatch batch, uint32_t* __restrict__ flag, uint32_t gen) {
  const uint32_t slot = blockIdx.y;
  const uint64_t i = (uint64_t)batch.len[slot] + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch.check_len[slot]) return;
  if (!fe_is_zero(ld_fr(&batch.scalars[slot][i]))) flag[slot] = gen;
}

// Hot-bucket guard (msm_run_batch's guard_limit), after the sort and before the accumulation:
// max_out[slot] = the slot's largest bucket count, and a slot above `limit` loses its tasks
// (task_off cleared: the accumulation and the reductions of that slot then see empty buckets
// and cost what a near-empty slot costs; its output is not used). k_runsum1 / k_bucket_sum walk
// a bucket's partials one after the other in a single lane, so n equal small scalars (one bucket
// of n entries) would make a reduction of n / chunk dependent additions.
// state[slot] = running maximum, state[kMaxSlots + slot] = arrival counter, both zero between
// batches (the slot's last workgroup resets them). max_out: mapped host memory, plain store.
__global__ void __launch_bounds__(256) k_guard(const uint32_t* __restrict__ offsets,
                                               uint32_t* __restrict__ task_off, uint32_t B,
                                               uint32_t limit, uint32_t* __restrict__ state,
                                               uint32_t* __restrict__ max_out) {
  __shared__ uint32_t s_max, s_last;
  const uint32_t slot = blockIdx.y, tid = threadIdx.x;
  const uint32_t* off = offsets + (size_t)slot * (B + 1);
  if (tid == 0) s_max = 0;
  __syncthreads();
  uint32_t m = 0;
  for (uint32_t b = blockIdx.x * blockDim.x + tid; b < B; b += gridDim.x * blockDim.x)
    m = max(m, off[b + 1] - off[b]);
  if (m) atomicMax(&s_max, m);
  __syncthreads();
  if (tid == 0) {
    if (s_max) atomicMax(&state[slot], s_max);
    __threadfence();
    s_last = atomicAdd(&state[kMaxSlots + slot], 1u) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  if (tid == 0) {
    __threadfence();
    s_max = atomicMax(&state[slot], 0u);  // the other workgroups' maxima included
    max_out[slot] = s_max;
    state[slot] = 0;  // ready for the next batch (stream order)
    state[kMaxSlots + slot] = 0;
  }
  __syncthreads();
  if (s_max > limit) {
    uint32_t* to = task_off + (size_t)slot * (B + 1);
    for (uint32_t b = tid; b <= B; b += blockDim.x) to[b] = 0;
  }
}

// f(std::integral_constant<uint32_t, CC>) with CC = c as a compile-time constant when c is one
// of Cs (each_digit's unrolled form; the sizes choose_c picks), CC = 0 (the run-time layout,
// right for any c) otherwise. Each kernel lists only the window sizes that can reach it.
template <uint32_t... Cs>
struct CList {};
template <uint32_t... Cs, class F>
void by_c(CList<Cs...>, uint32_t c, F&& f) {
  const bool hit = ((c == Cs ? (f(std::integral_constant<uint32_t, Cs>{}), true) : false) || ...);
  if (!hit) f(std::integral_constant<uint32_t, 0>{});
}
using CSmall = CList<10, 12, 13>;       // k_sort_one, under k_sort_small's bound: B <= kSortSmallMax, c <= 13
using CNarrow = CList<10, 12, 13, 15>;  // k_hist / k_scatter: B <= kLdsBuckets, c <= 16
using CWide = CList<17, 20>;            // k_chist / k_cscatter: c >= 17

// small batches: the whole sort (and the degree check) in one dispatch per batch
// (the chunk floor stays small_batch's: more scalars than kSortOneMax keep kChunkMin tasks).
// Round 5: up to kSortOneBig scalars too (the 2^14-size commits at c = 13) instead of
// k_hist + k_sort_small + k_scatter: 2^14 proofs 16.77 -> 17.33 M, 2^13 / 2^12 within noise
// (profiles/r05_sort_one_big_c13_ab.jsonl; round 4's single-workgroup form at c = 15 did
// not pay, profiles/r04_sort_one_big_ab.jsonl)
template <bool HOLD>
void sort_one(const MsmPlan& p, const MsmBatch& batch, MsmWorkspace& w, uint32_t* flag,
              hipStream_t stream) {
  by_c(CSmall{}, p.c, [&](auto cc) {
    hipLaunchKernelGGL((k_sort_one<decltype(cc)::value, HOLD>), dim3(std::min(kSortOneParts, p.B), p.slots),
                       dim3(1024), 0, stream, batch, p.cfg(), p.n_srs, p.chunk,
                       w.sorted.as<uint32_t>(), (uint64_t)w.sorted_stride,
                       w.offsets.as<uint32_t>(), w.task_off.as<uint32_t>(),
                       w.tasks.as<uint2>(), (uint64_t)w.task_stride, flag, p.gen);
  });
}

// narrow bucket sets: LDS histograms, the scans, the scatter, the task records
int sort_narrow(const MsmPlan& p, const MsmBatch& batch, MsmWorkspace& w, hipStream_t stream) {
  const uint32_t B = p.B, slots = p.slots, hist_blocks = p.hist_blocks;
  const MsmCfg cfg = p.cfg();
  const size_t lds = (size_t)std::min<uint32_t>(B, kLdsBuckets) * 4;
  if (p.max_len) {
    by_c(CNarrow{}, p.c, [&](auto cc) {
      hipLaunchKernelGGL(k_hist<decltype(cc)::value>, dim3(hist_blocks, slots), dim3(kHistThreads), lds,
                         stream, batch, cfg, w.blockhist.as<uint32_t>());
    });
  } else {
    PLK_HIP_TRY(hipMemsetAsync(w.blockhist.ptr, 0, (size_t)slots * hist_blocks * B * 4, stream));
  }
  if (p.small_sort) {
    hipLaunchKernelGGL(k_sort_small, dim3(1, slots), dim3(1024), 0, stream,
                       w.blockhist.as<uint32_t>(), hist_blocks, B, p.chunk, w.offsets.as<uint32_t>(),
                       w.task_off.as<uint32_t>(), w.tasks.as<uint2>(), (uint64_t)w.task_stride);
  } else {
    hipLaunchKernelGGL(k_block_scan, dim3(cdiv(B, 256), slots), dim3(256), 0, stream,
                       w.blockhist.as<uint32_t>(), hist_blocks, B, w.counts.as<uint32_t>(),
                       (uint32_t*)nullptr, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_scan_buckets, dim3(1, slots), dim3(1024), (size_t)B * 4, stream,
                       w.counts.as<uint32_t>(), B, p.chunk, w.offsets.as<uint32_t>(),
                       w.task_off.as<uint32_t>(), w.full_off.as<uint32_t>(),
                       w.len_cur.as<uint32_t>());
  }
  if (p.max_len) {
    by_c(CNarrow{}, p.c, [&](auto cc) {
      hipLaunchKernelGGL(k_scatter<decltype(cc)::value>, dim3(hist_blocks, slots), dim3(kHistThreads),
                         lds, stream, batch, cfg, p.n_srs,
                         w.offsets.as<uint32_t>(), w.blockhist.as<uint32_t>(),
                         w.sorted.as<uint32_t>(), (uint64_t)w.sorted_stride);
    });
  }
  if (!p.small_sort) {
    hipLaunchKernelGGL(k_make_tasks, dim3(cdiv(B, 256), slots), dim3(256), 0, stream,
                       w.offsets.as<uint32_t>(), w.task_off.as<uint32_t>(),
                       w.full_off.as<uint32_t>(), w.len_cur.as<uint32_t>(), B, p.chunk,
                       w.tasks.as<uint2>(), (uint64_t)w.task_stride);
  }
  return PLK_OK;
}

// wide pass 3 and 4 on bins of 2^FB buckets
template <uint32_t FB>
void sort_fine(const MsmPlan& p, MsmWorkspace& w, hipStream_t stream) {
  const uint32_t B = p.B, NC = p.NC, slots = p.slots;
  hipLaunchKernelGGL(k_fine<FB>, dim3(NC, slots), dim3(1u << FB), 0, stream, B, NC, p.chunk,
                     (const uint32_t*)w.coarse_off.as<uint32_t>(), (const uint2*)w.tmp.as<uint2>(),
                     (uint64_t)(w.sorted_stride - 1), w.sorted.as<uint32_t>(),
                     (uint64_t)w.sorted_stride, w.offsets.as<uint32_t>(),
                     w.task_rel.as<uint32_t>(), w.full_off.as<uint32_t>(),
                     w.bin_tot.as<uint32_t>(), w.len_cur.as<uint32_t>());
  hipLaunchKernelGGL(k_make_tasks_wide<FB>, dim3(NC, slots), dim3(1u << FB), 0, stream, B, NC,
                     p.chunk, (const uint32_t*)w.offsets.as<uint32_t>(),
                     (const uint32_t*)w.task_rel.as<uint32_t>(),
                     (const uint32_t*)w.full_off.as<uint32_t>(),
                     (const uint32_t*)w.bin_tot.as<uint32_t>(),
                     (const uint32_t*)w.len_cur.as<uint32_t>(), w.len_fill.as<uint32_t>(),
                     w.task_off.as<uint32_t>(), w.tasks.as<uint2>(), (uint64_t)w.task_stride);
}

// wide bucket sets: the two-level sort
int sort_wide(const MsmPlan& p, const MsmBatch& batch, MsmWorkspace& w, hipStream_t stream) {
  const uint32_t NC = p.NC, fb = p.fb, slots = p.slots, hist_blocks = p.hist_blocks;
  const MsmCfg cfg = p.cfg();
  if (p.max_len && p.naf) {
    hipLaunchKernelGGL(k_chist_naf, dim3(hist_blocks, slots), dim3(kHistThreads), 0, stream, batch,
                       cfg, NC, fb, w.blockhist.as<uint32_t>(), w.naf.as<uint32_t>(),
                       (uint64_t)w.naf_stride);
  } else if (p.max_len) {
    by_c(CWide{}, p.c, [&](auto cc) {
      hipLaunchKernelGGL(k_chist<decltype(cc)::value>, dim3(hist_blocks, slots), dim3(kHistThreads), 0,
                         stream, batch, cfg, NC, fb, w.blockhist.as<uint32_t>());
    });
  } else {
    PLK_HIP_TRY(hipMemsetAsync(w.blockhist.ptr, 0, (size_t)slots * hist_blocks * NC * 4, stream));
  }
  hipLaunchKernelGGL(k_block_scan, dim3(cdiv(NC, 256), slots), dim3(256), 0, stream,
                     w.blockhist.as<uint32_t>(), hist_blocks, NC, w.counts.as<uint32_t>(),
                     w.len_cur.as<uint32_t>(), w.len_fill.as<uint32_t>());
  if (p.naf) {
    hipLaunchKernelGGL(k_cscatter_naf, dim3(hist_blocks, slots), dim3(kHistThreads), 0, stream, batch,
                       cfg, NC, fb, p.n_srs, (const uint32_t*)w.counts.as<uint32_t>(),
                       (const uint32_t*)w.blockhist.as<uint32_t>(), w.coarse_off.as<uint32_t>(),
                       w.tmp.as<uint2>(), (uint64_t)(w.sorted_stride - 1),
                       (const uint32_t*)w.naf.as<uint32_t>(), (uint64_t)w.naf_stride);
  } else by_c(CWide{}, p.c, [&](auto cc) {
    hipLaunchKernelGGL(k_cscatter<decltype(cc)::value>, dim3(hist_blocks, slots), dim3(kHistThreads),
                       0, stream, batch, cfg, NC, fb, p.n_srs,
                       (const uint32_t*)w.counts.as<uint32_t>(),
                       (const uint32_t*)w.blockhist.as<uint32_t>(),
                       w.coarse_off.as<uint32_t>(), w.tmp.as<uint2>(),
                       (uint64_t)(w.sorted_stride - 1));
  });
  if (fb == 10) sort_fine<10>(p, w, stream);
  else if (fb == 9) sort_fine<9>(p, w, stream);
  else sort_fine<8>(p, w, stream);
  return PLK_OK;
}

}  // namespace

int msm_sort_prepare(uint32_t c) {
  if (is_wide(c)) return PLK_OK;  // the wide kernels' LDS is static
  // k_scan_buckets stages the B counts (narrow sets: B <= kLdsBuckets)
  const int lds = (int)((1u << (c - 1)) * 4);
  PLK_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_scan_buckets),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  int st = PLK_OK;
  by_c(CNarrow{}, c, [&](auto cc) {
    st = [&]() -> int {
      PLK_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hist<decltype(cc)::value>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      PLK_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_scatter<decltype(cc)::value>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      return PLK_OK;
    }();
  });
  return st;
}

int msm_sort(const MsmPlan& p, const MsmBatch& batch, MsmWorkspace& w, hipStream_t stream) {
  ReadbackHeader* hdr_dev = static_cast<ReadbackHeader*>(w.out_dev);
  int st = PLK_OK;
  if (p.max_tail && !p.sort_one) {
    hipLaunchKernelGGL(k_any_nonzero, dim3(cdiv(p.max_tail, 256), p.slots), dim3(256), 0, stream,
                       batch, hdr_dev->flag, p.gen);
  }
  if (p.wide) st = sort_wide(p, batch, w, stream);
  else if (!p.sort_one) st = sort_narrow(p, batch, w, stream);
  else if (p.hold) sort_one<true>(p, batch, w, hdr_dev->flag, stream);
  else sort_one<false>(p, batch, w, hdr_dev->flag, stream);
  if (st) return st;
  if (p.guard_limit) {
    hipLaunchKernelGGL(k_guard, dim3(std::min<uint32_t>(64, cdiv(p.B, 1024)), p.slots), dim3(256), 0, stream,
                       (const uint32_t*)w.offsets.as<uint32_t>(), w.task_off.as<uint32_t>(), p.B,
                       p.guard_limit, w.guard.as<uint32_t>(), hdr_dev->max_count);
  }
  return PLK_OK;
}

}  // namespace plk
