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

// ---- row-table layout (plk_srs::naf): a signed sliding window over the canonical half --------
// The table has a row 2^p P for every bit position p, so a digit may start at any bit: a window
// starts at a set bit of the running value (its digit is odd), the zeros after it cost nothing,
// and with windows of up to c + 1 bits the odd digits |d| < 2^c fill the same 2^(c-1) buckets,
// bucket (|d| - 1) / 2 weighing |d|. A uniform 254-bit half gives 255 / (c + 2) + ~0.4 digits
// (c = 20: 11.98) instead of the fixed grid's W = 13, never more than ceil(255 / (c + 1)) <= W.
//
// The half stays in its registers: the walk keeps a bit position and a borrow (the running
// value is (s >> pos) + borrow), and a window starts at the first bit >= pos that differs from
// the borrow. Pass 1 is the greedy walk, all windows c + 1 bits, counting its digits m. Greedy's
// top digit takes the few bits left over, whose values crowd the lowest buckets (9 % of all
// scalars in bucket 0), so pass 2 spreads the bits over the same m digits: with rho bits still
// to cover (one more for the borrow) and k digits to emit, a window is
// min(c + 1, max(ceil(rho / k) - 1, rho - (c + 1)(k - 1), 2)) bits; the middle term keeps the
// rest coverable. tests/msm_naf_ref.py states both forms, tests/test_msm_naf_cpu.py the conditions.

// bits [o, o + 33) of s at least (64 taken, sh <= 31 shifted out), zero from bit 256 on
__device__ __forceinline__ uint64_t bits_at(const Fr& s, uint32_t o) {
  if (o >= 256) return 0;
  const uint32_t wd = o >> 5, sh = o & 31;
  const bool b0 = wd & 1, b1 = wd & 2, b2 = wd & 4;
  uint64_t p[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // pair (2k + b0, 2k + b0 + 1), as digit_at
    const uint32_t lo = b0 ? s.v[2 * k + 1] : s.v[2 * k];
    const uint32_t hi = b0 ? (k < 3 ? s.v[2 * k + 2] : 0u) : s.v[2 * k + 1];
    p[k] = ((uint64_t)hi << 32) | lo;
  }
  const uint64_t q0 = b1 ? p[1] : p[0], q1 = b1 ? p[3] : p[2];
  return (b2 ? q1 : q0) >> sh;
}

__device__ __forceinline__ uint32_t fr_bit_length(const Fr& s) {
  uint32_t len = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (s.v[k]) len = 32u * k + 32u - (uint32_t)__builtin_clz(s.v[k]);
  return len;
}

// One walk over s (bit length len): EMIT = false counts the greedy digits, EMIT = true emits
// f(pos, d) for the k digits of pass 2. Returns the digit count. At most `cap` windows whatever
// the input (the callers' buffers hold cap words per scalar).
template <bool EMIT, class F>
__device__ __forceinline__ uint32_t naf_pass(const Fr& s, uint32_t len, uint32_t c, uint32_t k,
                                             uint32_t cap, F&& f) {
  const uint32_t w = c + 1;
  // a window read from one bits_at: its start at most `skip` bits in, skip + w <= 33
  const uint32_t skip = 33 - w;
  uint32_t pos = 0, carry = 0, n = 0;
  while (n < cap) {
    if (!carry && pos >= len) break;
    const uint64_t x = bits_at(s, pos);
    const uint32_t differ = (uint32_t)x ^ (0u - carry);  // bits that differ from the borrow
    const uint32_t tz = (uint32_t)__builtin_ctz(differ | (1u << skip));
    if (tz == skip && !((differ >> skip) & 1u)) {  // a longer run: look again from its end
      pos += skip;
      continue;
    }
    pos += tz;
    uint32_t wd = w;
    if (EMIT && k > 1) {
      const uint32_t rho = (len > pos ? len - pos : 1u) + 1u;
      const uint32_t even = (rho + k - 1) / k - 1, rest = w * (k - 1);
      wd = min(w, max(max(even, rho > rest ? rho - rest : 0u), 2u));
    }
    const uint32_t val = ((uint32_t)(x >> tz) & ((1u << wd) - 1u)) + carry;
    carry = val >> (wd - 1) ? 1u : 0u;  // val odd: never 2^(wd-1) itself
    if (EMIT) f(pos, (int)val - (int)(carry << wd));
    pos += wd;
    --k;
    ++n;
  }
  return n;
}

// A scalar's digits as words: bucket (|d| - 1) / 2 | position << 22 | (d < 0) << 31. Positions
// stop at 254, so kNafNone (position 255) marks a word that holds no digit.
constexpr uint32_t kNafNone = 0xFFFFFFFFu;
constexpr uint32_t kNafMaxW = 15;  // digits per scalar at most: W of the wide sets (c >= 17)
constexpr uint32_t kNafPosShift = 22;
__device__ __forceinline__ uint32_t naf_word(uint32_t pos, int d) {
  const uint32_t a = (uint32_t)(d < 0 ? -d : d);
  return ((a - 1u) >> 1) | (pos << kNafPosShift) | (d < 0 ? 0x80000000u : 0u);
}
__device__ __forceinline__ uint32_t naf_bucket(uint32_t word) { return word & ((1u << kNafPosShift) - 1u); }
__device__ __forceinline__ uint32_t naf_pos(uint32_t word) { return (word >> kNafPosShift) & 255u; }
__device__ __forceinline__ bool naf_neg(uint32_t word) { return word >> 31; }

// Both passes: f(j, word) for j = 0 .. digits - 1 in order of position. Returns the count (<= W).
template <class F>
__device__ __forceinline__ uint32_t naf_walk(const Fr& s, const MsmCfg& cfg, F&& f) {
  const uint32_t len = fr_bit_length(s);
  const uint32_t m = naf_pass<false>(s, len, cfg.c, 0, cfg.W, [](uint32_t, int) {});
  uint32_t j = 0;
  naf_pass<true>(s, len, cfg.c, m, cfg.W, [&](uint32_t pos, int d) { f(j++, naf_word(pos, d)); });
  return m;
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
