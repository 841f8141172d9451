// msm_var.hip — variable-base G1 multi-scalar multiplication on gfx950: msm_curve_addition
// (&[G1Affine], &[Fr]) for points seen once (zksnarks, un-vendored; called at
// /root/reference/src/prover/proof.rs:507). The SRS MSM (msm.hip) runs over a
// window table table[w][i] = 2^(cw) P_i that costs a 255-doubling chain per point; a verifier's
// points (proof commitments) are used once, so this one has no table:
//
//  * k_var_prepare: the caller's ABI points -> R'-domain affine (ffr.hpp, what k_accumulate
//    reads), with the curve check y^2 = x^3 + 4 and the canonical-limb check; identity inputs
//    are flagged and emit no entries at all.
//  * Classic per-window bucket sets: scalar s -> [0, (r-1)/2] (s or r - s with the signs flipped),
//    W = ceil(255 / c) signed c-bit digits |d| <= 2^(c-1); entry (i, w) with digit d goes to bucket
//    w 2^(c-1) + |d| - 1 with code i | sign << 31. The accumulation gathers straight from the
//    converted points.
//  * Counting sort by bucket: k_var_count (global atomics: N W <= ~2e7 entries, not the SRS
//    sizes), k_var_scan (one workgroup per output: bucket offsets and the accumulation tasks of
//    <= chunk same-bucket entries), k_var_scatter.
//  * Accumulation: msm_acc.hip's k_accumulate, unchanged (launch_accumulate), without its
//    identity path.
//  * Reduction sum_w 2^(cw) sum_b (b + 1) S_(w,b) = sum_j 2^j T_j: T_(cw+k) = the sum of window
//    w's buckets with bit k of b + 1 set (b + 1 <= 2^(c-1) has c bits, so every j belongs to one
//    window). k_var_bucket_sum folds a bucket's task partials, k_var_bitsum gives the W c points
//    T_j, the host runs the Horner tail and the single inversion.
//  * Up to kMaxSlots outputs over disjoint index ranges of one point array run as one batch
//    (blockIdx.y = output): the verifier's fold needs two.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "internal.hpp"
#include "msm_common.hpp"
#include "g1r.hpp"

namespace plk {

struct VarMsmWs {
  DevBuf pts, inf, counts, offsets, cursor, task_off, sorted, tasks, partials, bsum, tout, bad;
  PinnedBuf host_out;
  TimingEvents<2> ev;
};

void msm_var_ws_delete(VarMsmWs* w) { delete w; }

namespace {

struct VarBatch {
  uint32_t start[kMaxSlots], len[kMaxSlots];
};

// ABI point i -> pts[i] (R' domain) and inf[i]; *bad = 1 for a point g1_load<true> refuses, which
// is kept out of the sums (flagged as identity) while the call fails with PLK_E_ARG
__global__ void __launch_bounds__(256) k_var_prepare(const plk_g1* __restrict__ in, uint32_t n,
                                                     G1Affine* __restrict__ pts,
                                                     uint8_t* __restrict__ inf,
                                                     uint32_t* __restrict__ bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1Abi p = g1_load<true>(&in[i]);
  if (!p.ok) *bad = 1;
  const bool keep = p.ok && !p.inf;
  Fp x = fe_zero<FpCfg>(), y = fe_zero<FpCfg>();
  if (keep) {
    x = fe_to_rx_domain(p.x);
    y = fe_to_rx_domain(p.y);
  }
  st_aff(&pts[i], x, y);
  inf[i] = keep ? 0 : 1;
}

// Canonical scalar in [0, (r-1)/2]: s, or r - s with the digit signs flipped (msm_digits.hpp
// scalar_half_v: the same recoding, s < 2^254 needs W = ceil(255 / c) windows)
__device__ __forceinline__ Fr var_scalar_half(const Fr& raw, bool& neg) {
  const Fr s = fe_from_mont(raw);
  const Fr t = fe_neg(s);
  bool lt = false;  // t < s
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    if (t.v[k] != s.v[k]) {
      lt = t.v[k] < s.v[k];
      break;
    }
  }
  neg = lt;
  return lt ? t : s;
}

// f(w, d) for the W signed c-bit digits of s (msm_digits.hpp each_digit's recoding with plain c-bit
// windows: d in [-2^(c-1) + 1, 2^(c-1)], the carry threaded upwards). The scalar is shifted
// down by c bits per window, so no word of it is indexed at run time (no scratch).
template <class F>
__device__ __forceinline__ void var_digits(Fr s, uint32_t c, uint32_t W, F&& f) {
  const uint32_t mask = (1u << c) - 1u, half = 1u << (c - 1);
  uint32_t carry = 0;
  for (uint32_t w = 0; w < W; ++w) {
    const uint32_t val = (s.v[0] & mask) + carry;
    int d;
    if (val > half) {
      d = (int)val - (int)(1u << c);
      carry = 1;
    } else {
      d = (int)val;
      carry = 0;
    }
    f(w, d);
#pragma unroll
    for (int k = 0; k < 7; ++k) s.v[k] = (s.v[k] >> c) | (s.v[k + 1] << (32 - c));
    s.v[7] >>= c;
  }
}

__global__ void __launch_bounds__(256) k_var_count(VarBatch batch, const Fr* __restrict__ scalars,
                                                   const uint8_t* __restrict__ inf, uint32_t c,
                                                   uint32_t W, uint32_t NB,
                                                   uint32_t* __restrict__ counts) {
  const uint32_t slot = blockIdx.y;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= batch.len[slot]) return;
  const uint32_t i = batch.start[slot] + t;
  if (inf[i]) return;
  bool neg;
  const Fr s = var_scalar_half(ld_fr(&scalars[i]), neg);
  uint32_t* cnt = counts + (size_t)slot * (NB + 1);
  const uint32_t Bw = 1u << (c - 1);
  var_digits(s, c, W, [&](uint32_t w, int d) {
    if (d == 0) return;
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    atomicAdd(&cnt[w * Bw + a - 1], 1u);
  });
}

// One workgroup per output: offsets[b] = entries before bucket b (offsets[NB] = all), cursor = a
// copy for the scatter, task_off[b] = tasks before bucket b, and the task records of
// k_accumulate (msm_acc.hip): task_record(first entry, partial index, length) of msm_common.hpp,
// bucket b's tasks at task_off[b] .. task_off[b + 1], each of <= chunk entries.
__global__ void __launch_bounds__(1024) k_var_scan(const uint32_t* __restrict__ counts, uint32_t NB,
                                                   uint32_t chunk, uint32_t* __restrict__ offsets,
                                                   uint32_t* __restrict__ cursor,
                                                   uint32_t* __restrict__ task_off,
                                                   uint2* __restrict__ tasks, uint64_t task_stride) {
  __shared__ uint32_t sh_e[1024], sh_t[1024];
  const uint32_t slot = blockIdx.y, t = threadIdx.x;
  counts += (size_t)slot * (NB + 1);
  offsets += (size_t)slot * (NB + 1);
  cursor += (size_t)slot * (NB + 1);
  task_off += (size_t)slot * (NB + 1);
  tasks += (size_t)slot * task_stride;
  const uint32_t per = (NB + 1023) / 1024;
  const uint32_t b0 = min(NB, t * per), b1 = min(NB, b0 + per);
  uint32_t e = 0, k = 0;
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t n = counts[b];
    e += n;
    k += (n + chunk - 1) / chunk;
  }
  sh_e[t] = e;
  sh_t[t] = k;
  __syncthreads();
  for (uint32_t h = 1; h < 1024; h <<= 1) {  // inclusive scan
    const uint32_t ae = t >= h ? sh_e[t - h] : 0u, at = t >= h ? sh_t[t - h] : 0u;
    __syncthreads();
    sh_e[t] += ae;
    sh_t[t] += at;
    __syncthreads();
  }
  uint32_t eo = sh_e[t] - e, to = sh_t[t] - k;  // exclusive
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t n = counts[b];
    offsets[b] = eo;
    cursor[b] = eo;
    task_off[b] = to;
    for (uint32_t done = 0; done < n; done += chunk) {
      const uint32_t len = min(chunk, n - done);
      if (to < task_stride) tasks[to] = task_record(eo + done, to, len);
      ++to;
    }
    eo += n;
  }
  if (t == 1023) {
    offsets[NB] = eo;
    task_off[NB] = to;
  }
}

__global__ void __launch_bounds__(256) k_var_scatter(VarBatch batch, const Fr* __restrict__ scalars,
                                                     const uint8_t* __restrict__ inf, uint32_t c,
                                                     uint32_t W, uint32_t NB,
                                                     uint32_t* __restrict__ cursor,
                                                     uint32_t* __restrict__ sorted,
                                                     uint64_t sorted_stride) {
  const uint32_t slot = blockIdx.y;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= batch.len[slot]) return;
  const uint32_t i = batch.start[slot] + t;
  if (inf[i]) return;
  bool neg;
  const Fr s = var_scalar_half(ld_fr(&scalars[i]), neg);
  uint32_t* cur = cursor + (size_t)slot * (NB + 1);
  uint32_t* out = sorted + (size_t)slot * sorted_stride;
  const uint32_t Bw = 1u << (c - 1);
  var_digits(s, c, W, [&](uint32_t w, int d) {
    if (d == 0) return;
    const uint32_t a = (uint32_t)(d < 0 ? -d : d);
    const uint32_t pos = atomicAdd(&cur[w * Bw + a - 1], 1u);
    // the same digits as k_var_count counted, so pos stays inside the bucket's range
    if (pos < sorted_stride) out[pos] = entry_code(i, (d < 0) != neg);
  });
}

// bsum[b] = the sum of bucket b's task partials (the identity for an empty bucket)
__global__ void __launch_bounds__(256) k_var_bucket_sum(const uint32_t* __restrict__ task_off,
                                                        uint32_t NB, uint64_t task_stride,
                                                        const G1xyzz* __restrict__ partials,
                                                        G1xyzz* __restrict__ bsum) {
  const uint32_t slot = blockIdx.y;
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= NB) return;
  task_off += (size_t)slot * (NB + 1);
  partials += (size_t)slot * task_stride;
  G1R acc = g1r_infinity();
  for (uint32_t t = task_off[b]; t < task_off[b + 1]; ++t) acc = g1r_add(acc, ld_g1r(&partials[t]));
  st_g1r(&bsum[(size_t)slot * NB + b], acc);
}

__device__ __forceinline__ G1R var_shfl_down(const G1R& v, uint32_t h) {
  G1R o;
  Fp x;
#define PLK_VAR_SHFL(F)                                              \
  x = rx_pack(v.F);                                                  \
  _Pragma("unroll") for (int i = 0; i < 12; ++i) x.v[i] = __shfl_down(x.v[i], h, 64); \
  o.F = rx_unpack(x);
  PLK_VAR_SHFL(X)
  PLK_VAR_SHFL(Y)
  PLK_VAR_SHFL(ZZ)
  PLK_VAR_SHFL(ZZZ)
#undef PLK_VAR_SHFL
  return o;
}

// out[j], j = c w + k = blockIdx.x: the sum of window w's buckets b with bit k of b + 1 set
__global__ void __launch_bounds__(256) k_var_bitsum(const G1xyzz* __restrict__ bsum, uint32_t c,
                                                    uint32_t W, G1xyzz* __restrict__ out) {
  __shared__ G1xyzz sh[4];
  const uint32_t slot = blockIdx.y, j = blockIdx.x, w = j / c, k = j % c;
  const uint32_t Bw = 1u << (c - 1), NB = W * Bw;
  bsum += (size_t)slot * NB + (size_t)w * Bw;
  G1R acc = g1r_infinity();
  for (uint32_t b = threadIdx.x; b < Bw; b += 256)
    if (((b + 1) >> k) & 1u) acc = g1r_add(acc, ld_g1r(&bsum[b]));
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t h = 32; h >= 1; h >>= 1) {
    const G1R o = var_shfl_down(acc, h);
    if (lane < h) acc = g1r_add(acc, o);
  }
  if (lane == 0) st_g1r(&sh[threadIdx.x >> 6], acc);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t v = 1; v < 4; ++v) acc = g1r_add(acc, ld_g1r(&sh[v]));
    st_g1r(&out[(size_t)slot * (W * c) + j], acc);
  }
}

// Window size for an output of n points. Cost in point additions (the model choose_c states for
// the SRS MSM, with this file's reduction): n W mixed additions, W 2^(c-1) to fold the task
// partials, and W c 2^(c-2) full additions (~1.5 mixed ones) in the bit sums.
uint32_t choose_c_var(size_t n) {
  uint32_t best = 3;
  double best_cost = 0;
  for (uint32_t c = 3; c <= 16; ++c) {
    const double W = (double)((255 + c - 1) / c);
    const double cost = (double)n * W + W * (double)(1u << (c - 1)) + 1.5 * W * c * (double)(1u << (c - 2));
    if (c == 3 || cost < best_cost) {
      best = c;
      best_cost = cost;
    }
  }
  return best;
}

}  // namespace

int msm_var_run(plk_ctx* ctx, const plk_g1* d_points, const Fr* d_scalars, size_t n,
                const size_t* starts, const size_t* lens, size_t count, plk_g1* outs,
                hipStream_t stream) {
  if (count == 0) return PLK_OK;
  if (count > kMaxSlots || n >= (1ull << 31)) return PLK_E_ARG;
  VarBatch batch{};
  size_t max_len = 0;
  for (size_t k = 0; k < count; ++k) {
    if (starts[k] > n || lens[k] > n - starts[k]) return PLK_E_ARG;
    batch.start[k] = (uint32_t)starts[k];
    batch.len[k] = (uint32_t)lens[k];
    max_len = std::max(max_len, lens[k]);
  }
  const uint32_t slots = (uint32_t)count;
  if (n == 0 || max_len == 0) {
    for (size_t k = 0; k < count; ++k) {
      outs[k] = plk_g1{};
      outs[k].infinity = 1;
    }
    return PLK_OK;
  }
  if (!ctx->var_ws) ctx->var_ws = new VarMsmWs();
  VarMsmWs& w = *ctx->var_ws;
  const uint32_t c = choose_c_var(max_len), W = (255 + c - 1) / c;
  const uint32_t Bw = 1u << (c - 1), NB = W * Bw, NT = W * c;
  const size_t E = (size_t)W * max_len;  // entries per output at most
  if (E >= (1ull << 31)) return PLK_E_ARG;
  const uint32_t chunk = E < (1u << 20) ? kChunkMin : kChunkMax;
  const size_t task_stride = std::min<size_t>(E, E / chunk + NB) + 1;
  if (task_stride >= kTaskIndexEnd) return PLK_E_ARG;
  int st;
  if ((st = w.pts.alloc(n * sizeof(G1Affine)))) return st;
  if ((st = w.inf.alloc(n))) return st;
  if ((st = w.counts.alloc((size_t)slots * (NB + 1) * 4))) return st;
  if ((st = w.offsets.alloc((size_t)slots * (NB + 1) * 4))) return st;
  if ((st = w.cursor.alloc((size_t)slots * (NB + 1) * 4))) return st;
  if ((st = w.task_off.alloc((size_t)slots * (NB + 1) * 4))) return st;
  if ((st = w.sorted.alloc((size_t)slots * E * 4))) return st;
  if ((st = w.tasks.alloc((size_t)slots * task_stride * sizeof(uint2)))) return st;
  if ((st = w.partials.alloc((size_t)slots * task_stride * sizeof(G1xyzz)))) return st;
  if ((st = w.bsum.alloc((size_t)slots * NB * sizeof(G1xyzz)))) return st;
  const size_t out_bytes = (size_t)slots * NT * sizeof(G1xyzz);
  if ((st = w.tout.alloc(out_bytes + 16))) return st;  // the T_j, then the curve-check flag
  if ((st = w.host_out.alloc(out_bytes + 16))) return st;
  if ((st = w.ev.create())) return st;
  uint32_t* bad = reinterpret_cast<uint32_t*>(w.tout.as<uint8_t>() + out_bytes);

  PLK_HIP_TRY(hipMemsetAsync(bad, 0, 16, stream));
  PLK_HIP_TRY(hipMemsetAsync(w.counts.ptr, 0, (size_t)slots * (NB + 1) * 4, stream));
  hipLaunchKernelGGL(k_var_prepare, dim3(cdiv(n, 256)), dim3(256), 0, stream, d_points, (uint32_t)n,
                     w.pts.as<G1Affine>(), w.inf.as<uint8_t>(), bad);
  hipLaunchKernelGGL(k_var_count, dim3(cdiv(max_len, 256), slots), dim3(256), 0, stream, batch,
                     d_scalars, (const uint8_t*)w.inf.as<uint8_t>(), c, W, NB, w.counts.as<uint32_t>());
  hipLaunchKernelGGL(k_var_scan, dim3(1, slots), dim3(1024), 0, stream,
                     (const uint32_t*)w.counts.as<uint32_t>(), NB, chunk, w.offsets.as<uint32_t>(),
                     w.cursor.as<uint32_t>(), w.task_off.as<uint32_t>(), w.tasks.as<uint2>(),
                     (uint64_t)task_stride);
  hipLaunchKernelGGL(k_var_scatter, dim3(cdiv(max_len, 256), slots), dim3(256), 0, stream, batch,
                     d_scalars, (const uint8_t*)w.inf.as<uint8_t>(), c, W, NB, w.cursor.as<uint32_t>(),
                     w.sorted.as<uint32_t>(), (uint64_t)E);
  PLK_HIP_TRY(hipGetLastError());
  // identity inputs emit no entries, so k_accumulate runs without its identity path
  launch_accumulate(false, true, dim3(cdiv(task_stride, 256), slots), stream, w.ev.e[0], w.ev.e[1],
                    w.tasks.as<uint2>(), w.task_off.as<uint32_t>(), NB, (uint64_t)task_stride,
                    w.sorted.as<uint32_t>(), (uint64_t)E, w.pts.as<G1Affine>(),
                    w.inf.as<uint8_t>(), w.partials.as<G1xyzz>());
  hipLaunchKernelGGL(k_var_bucket_sum, dim3(cdiv(NB, 256), slots), dim3(256), 0, stream,
                     (const uint32_t*)w.task_off.as<uint32_t>(), NB, (uint64_t)task_stride,
                     (const G1xyzz*)w.partials.as<G1xyzz>(), w.bsum.as<G1xyzz>());
  hipLaunchKernelGGL(k_var_bitsum, dim3(NT, slots), dim3(256), 0, stream,
                     (const G1xyzz*)w.bsum.as<G1xyzz>(), c, W, w.tout.as<G1xyzz>());
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipMemcpyAsync(w.host_out.ptr, w.tout.ptr, out_bytes + 16, hipMemcpyDeviceToHost, stream));
  PLK_HIP_TRY(stream_wait(stream));
  const G1xyzz* T = w.host_out.as<G1xyzz>();
  const uint32_t bad_host = *reinterpret_cast<const uint32_t*>(w.host_out.as<uint8_t>() + out_bytes);
  if (bad_host) return PLK_E_ARG;
  // host tail: sum_j 2^j T_j (Horner), then canonical affine
  for (uint32_t k = 0; k < slots; ++k) {
    G1xyzz acc = xyzz_infinity();
    for (int j = (int)NT - 1; j >= 0; --j) {
      acc = xyzz_dbl(acc);
      acc = xyzz_add(acc, rx_to_r_domain(T[(size_t)k * NT + j]));
    }
    Fp x, y;
    const bool fin = xyzz_to_affine(acc, x, y);
    g1_store(x, y, fin, &outs[k]);
  }
  return PLK_OK;
}

}  // namespace plk

using namespace plk;

extern "C" {

int plk_msm_points_ranges(plk_ctx* ctx, const plk_g1* points, const plk_fr* scalars, size_t n,
                          const size_t* starts, const size_t* lens, size_t count, plk_g1* outs) {
  PLK_API_BEGIN
  if (!ctx || !outs || count == 0 || count > kMaxSlots || !starts || !lens ||
      (n && (!points || !scalars)))
    return PLK_E_ARG;
  for (size_t k = 0; k < count; ++k)
    if (starts[k] > n || lens[k] > n - starts[k]) return PLK_E_ARG;
  for (size_t a = 0; a < count; ++a)  // disjoint ranges
    for (size_t b = a + 1; b < count; ++b)
      if (lens[a] && lens[b] && starts[a] < starts[b] + lens[b] && starts[b] < starts[a] + lens[a])
        return PLK_E_ARG;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  DevBuf dp, ds;
  int st;
  if (n) {
    if ((st = dp.alloc(n * sizeof(plk_g1)))) return st;
    if ((st = ds.alloc(n * sizeof(Fr)))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(dp.ptr, points, n * sizeof(plk_g1), hipMemcpyHostToDevice, s));
    PLK_HIP_TRY(hipMemcpyAsync(ds.ptr, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, s));
  }
  st = msm_var_run(ctx, dp.as<plk_g1>(), ds.as<Fr>(), n, starts, lens, count, outs, s);
  (void)stream_wait(s);  // dp / ds are freed on return
  return st;
  PLK_API_END
}

int plk_msm_points(plk_ctx* ctx, const plk_g1* points, const plk_fr* scalars, size_t n, plk_g1* out) {
  const size_t start = 0;
  return plk_msm_points_ranges(ctx, points, scalars, n, &start, &n, 1, out);
}

}  // extern "C"
