// msm_digits.hpp — the fixed-base MSM's device-side scalar recoding: the canonical half of a
// scalar, its signed c-bit digits, and the sort passes' walk over a slot's scalars (msm_sort.hip).
#pragma once
#include "msm_common.hpp"

namespace plk {

// signed digit w of canonical scalar s (carry threaded through the caller): windows
// 0 .. W - narrow - 1 take c bits, the top `narrow` ones c - 1 bits (plk_srs::narrow), their
// digits (|d| <= 2^(c-2)) scaled by 2 so that they span the bucket range too
__device__ __forceinline__ int digit_at(const Fr& s, uint32_t w, const MsmCfg& cfg, uint32_t& carry) {
  const uint32_t wn = cfg.W - cfg.narrow;  // first narrow window
  const bool nar = w >= wn;
  const uint32_t c = cfg.c - (nar ? 1u : 0u);
  const uint32_t o = nar ? wn * cfg.c + (w - wn) * c : w * cfg.c;
  uint32_t val = 0;
  if (o < 256) {
    // words wd, wd + 1 by a 3-level select tree: indexing s.v with a run-time wd put the
    // scalar in scratch memory (k_sort_one: 272 B per lane, k_hist / k_scatter: 48)
    const uint32_t wd = o >> 5, sh = o & 31;
    const bool b0 = wd & 1, b1 = wd & 2, b2 = wd & 4;
    uint64_t p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // pair (2k + b0, 2k + b0 + 1)
      const uint32_t lo = b0 ? s.v[2 * k + 1] : s.v[2 * k];
      const uint32_t hi = b0 ? (k < 3 ? s.v[2 * k + 2] : 0u) : s.v[2 * k + 1];
      p[k] = ((uint64_t)hi << 32) | lo;
    }
    const uint64_t q0 = b1 ? p[1] : p[0], q1 = b1 ? p[3] : p[2];
    const uint64_t two = b2 ? q1 : q0;
    val = (uint32_t)(two >> sh) & ((1u << c) - 1u);
  }
  int d = (int)(val + carry);
  if (d > (int)(1u << (c - 1))) {
    d -= (int)(1u << c);
    carry = 1;
  } else {
    carry = 0;
  }
  return nar ? d * 2 : d;
}

// Every digit of s, f(w, d) for w = 0 .. W-1 in order. C = 0: digit_at with the run-time
// window layout. C = the SRS's c (10, 12, 13, 15, 17, 20 — the window sizes choose_c picks): the
// layout is a compile-time constant, the loop unrolls and each digit is a funnel shift
// (v_alignbit_b32) of two known words, a mask and the carry test — ~6 instructions instead
// of digit_at's ~25 (word select tree, 64-bit shift). The sort kernels extract every digit of
// every scalar twice (histogram and scatter); k_sort_one does it for a whole commit on one
// workgroup.
template <uint32_t C, class F>
__device__ __forceinline__ void each_digit(const Fr& s, const MsmCfg& cfg, F&& f) {
  if constexpr (C == 0) {
    uint32_t carry = 0;
    for (uint32_t w = 0; w < cfg.W; ++w) f(w, digit_at(s, w, cfg, carry));
  } else {
    constexpr uint32_t W = (255 + C - 1) / C, NAR = C * W - 255, WN = W - NAR;
    static_assert(NAR < W, "balanced windows need (C - 1) W <= 255");
    uint32_t carry = 0;
#pragma unroll
    for (uint32_t w = 0; w < W; ++w) {
      const bool nar = w >= WN;
      const uint32_t cw = nar ? C - 1 : C;
      const uint32_t o = nar ? WN * C + (w - WN) * (C - 1) : w * C;
      const uint32_t wd = o >> 5, sh = o & 31;
      uint32_t val = sh == 0 ? s.v[wd]
                             : __builtin_amdgcn_alignbit(wd + 1 < 8 ? s.v[wd + 1 < 8 ? wd + 1 : 7] : 0u,
                                                         s.v[wd], sh);
      val &= (1u << cw) - 1u;
      int d = (int)(val + carry);
      if (d > (int)(1u << (cw - 1))) {
        d -= (int)(1u << cw);
        carry = 1;
      } else {
        carry = 0;
      }
      f(w, nar ? d * 2 : d);
    }
  }
}

__device__ __forceinline__ void slot_range(uint32_t len, uint32_t& i0, uint32_t& i1) {
  const uint32_t per = (len + gridDim.x - 1) / gridDim.x;
  i0 = blockIdx.x * per;
  i1 = min(len, i0 + per);
}

// Canonical scalar in [0, (r-1)/2]: s, or r - s with the digit signs flipped (s P = (r - s)(-P)).
// With s < 2^254 the signed c-bit recoding needs W = ceil(255 / c) windows (c = 17: 15).
__device__ __forceinline__ Fr scalar_half_v(const Fr& raw, bool& neg) {
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
__device__ __forceinline__ Fr scalar_half(const Fr* p, bool& neg) { return scalar_half_v(ld_fr(p), neg); }

// f(i, canonical half of scalar i, its sign flip) for i = i0 + t, i0 + t + step, ... < i1 in
// order, with kScalarLoads scalars loaded before the first is processed: the sort passes are
// bound by load latency (one scalar in flight per thread before), not by bytes
constexpr uint32_t kScalarLoads = 4;
template <class F>
__device__ __forceinline__ void for_scalars(const Fr* __restrict__ sc, uint32_t i0, uint32_t i1,
                                            uint32_t t, uint32_t step, F&& f) {
  uint32_t i = i0 + t;
  for (; i + (kScalarLoads - 1) * step < i1; i += kScalarLoads * step) {
    Fr raw[kScalarLoads];
#pragma unroll
    for (uint32_t u = 0; u < kScalarLoads; ++u) raw[u] = ld_fr(&sc[i + u * step]);
#pragma unroll
    for (uint32_t u = 0; u < kScalarLoads; ++u) {
      bool neg;
      const Fr s = scalar_half_v(raw[u], neg);
      f(i + u * step, s, neg);
    }
  }
  for (; i < i1; i += step) {
    bool neg;
    const Fr s = scalar_half_v(ld_fr(&sc[i]), neg);
    f(i, s, neg);
  }
}

}  // namespace plk
