// ingest_math.hpp — the per-point math of the ingest stage, shared by ingest.hip (compact proofs)
// and srs_io.hip (an SRS from bytes): PLK_HD code on the packed field of ff.hpp / g1.hpp, so the
// kernels of both units and the host decoders run the same functions.
//
//  - g1_decompress_words: parse, range-check x, y = (x^3 + 4)^((p+1)/4) (p = 3 mod 4), verify
//    y^2 = x^3 + 4, pick the root by the sort bit.
//  - g1_in_subgroup: P in G1  <=>  (beta x, y) == -[x0^2] P with x0 = 0xd201000000010000 (Scott,
//    eprint 2021/1130 section 6; zkcrypto's is_torsion_free).
//  - fr_decode_words: range check and Montgomery form.
// The limb and byte conversions, the canonical test, the curve constants and the curve equation
// are abi.hpp's.
//
// The square root's exponent is fixed: a sliding window of 3 bits over it with the odd powers
// x, x^3, x^5, x^7 held in registers (48 VGPRs) costs 379 squarings and about 100 products. The
// exponent's bits are wave-uniform, so the window logic is scalar control flow and the table is
// selected with compile-time indices: no stack array, no LDS, no scratch.
#pragma once
#include <stdint.h>

#include "../../include/plk.h"
#include "abi.hpp"
#include "g1.hpp"

namespace plk {

// word i (little-endian) of (p + 1) / 4: 379 bits, Hamming weight 229
PLK_HD uint32_t sqrt_exp_word(int i) {
  switch (i) {
    case 0: return 0xffffeaabu;
    case 1: return 0xee7fbfffu;
    case 2: return 0xac54ffffu;
    case 3: return 0x07aaffffu;
    case 4: return 0x3dac3d89u;
    case 5: return 0xd9cc34a8u;
    case 6: return 0x3ce144afu;
    case 7: return 0xd91dd2e1u;
    case 8: return 0x90d2eb35u;
    case 9: return 0x92c6e9edu;
    case 10: return 0x8e5ff9a6u;
    default: return 0x0680447au;
  }
}
constexpr int kSqrtExpBits = 379;
PLK_HD uint32_t sqrt_exp_bit(int i) { return (sqrt_exp_word(i >> 5) >> (i & 31)) & 1u; }

// a > b as integers
PLK_HD bool fp_gt(const Fp& a, const Fp& b) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const uint64_t t = (uint64_t)b.v[i] - a.v[i] - borrow;
    borrow = (uint32_t)(t >> 63);
  }
  return borrow != 0;  // b - a < 0
}

// one of the four odd powers by a wave-uniform index (compile-time indices into t)
PLK_HD Fp fp_sel4(const Fp (&t)[4], uint32_t k) {
  Fp r = t[0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
#pragma unroll
    for (int i = 0; i < 12; ++i) r.v[i] = k == (uint32_t)j ? t[j].v[i] : r.v[i];
  }
  return r;
}

// a^((p+1)/4): the square root of a when a is a square (the caller verifies). Sliding window of
// up to 3 bits, MSB first, over the fixed exponent.
PLK_HD Fp fp_sqrt_candidate(const Fp& a) {
  Fp t[4];
  const Fp a2 = fe_sqr(a);
  t[0] = a;
  t[1] = fe_mul(t[0], a2);
  t[2] = fe_mul(t[1], a2);
  t[3] = fe_mul(t[2], a2);
  Fp r = a;
  bool started = false;
  int i = kSqrtExpBits - 1;
  while (i >= 0) {
    if (!sqrt_exp_bit(i)) {  // the top bit is set, so r has started here
      r = fe_sqr(r);
      --i;
      continue;
    }
    int len = i >= 2 ? 3 : i + 1;
    while (!sqrt_exp_bit(i - len + 1)) --len;  // the window ends on a set bit
    uint32_t val = 0;
    for (int k = 0; k < len; ++k) val = (val << 1) | sqrt_exp_bit(i - k);
    const Fp m = fp_sel4(t, val >> 1);
    if (started) {
      for (int k = 0; k < len; ++k) r = fe_sqr(r);
      r = fe_mul(r, m);
    } else {
      r = m;
      started = true;
    }
    i -= len;
  }
  return r;
}

// 48 compressed bytes as the 12 words read little-endian from memory -> Montgomery (x, y) or
// the identity. Returns a PLK_INGEST_* code; x, y are zero unless it is OK and finite.
PLK_HD uint8_t g1_decompress_words(const uint32_t (&w)[12], Fp& x, Fp& y, bool& inf) {
  x = fe_zero<FpCfg>();
  y = fe_zero<FpCfg>();
  inf = false;
  const uint32_t b0 = w[0] & 0xffu;
  if (!(b0 & 0x80u)) return PLK_INGEST_ENCODING;
  if (b0 & 0x40u) {  // infinity: 0xc0 and 47 zero bytes, nothing else
    uint32_t rest = w[0] ^ 0xc0u;
#pragma unroll
    for (int i = 1; i < 12; ++i) rest |= w[i];
    if (rest) return PLK_INGEST_ENCODING;
    inf = true;
    return PLK_INGEST_OK;
  }
  const bool sort = (b0 & 0x20u) != 0;
  Fp xc = fp_of_be_words(w);  // x is big-endian over the 48 bytes
  xc.v[11] &= 0x1fffffffu;
  if (!fe_canonical(xc)) return PLK_INGEST_RANGE;
  const Fp xm = fe_to_mont(xc);
  const Fp rhs = fe_add(fe_mul(fe_sqr(xm), xm), fp_four());
  Fp ym = fp_sqrt_candidate(rhs);
  if (!fe_eq(fe_sqr(ym), rhs)) return PLK_INGEST_OFF_CURVE;
  // the sort bit: y is the larger of (y, p - y) as integers. y = 0 does not occur: the curve's
  // order is odd, so it has no point of order 2.
  const Fp yc = fe_from_mont(ym);
  const Fp nyc = fe_neg(yc);
  if (fp_gt(yc, nyc) != sort) ym = fe_neg(ym);
  x = xm;
  y = ym;
  return PLK_INGEST_OK;
}

// acc = [x0] base for x0 = 0xd201000000010000, MSB first: 63 doublings and 5 additions; Add is
// the complete addition of the base (g1.hpp handles P = +-Q and the identity explicitly)
constexpr uint64_t kX0 = 0xd201000000010000ull;
template <class Add>
PLK_HD G1xyzz g1_mul_x0(G1xyzz acc, Add add_base) {
  for (int b = 62; b >= 0; --b) {
    acc = xyzz_dbl(acc);
    if ((kX0 >> b) & 1ull) acc = add_base(acc);
  }
  return acc;
}

// (x, y): a finite point on the curve, Montgomery form. True iff it has order r.
PLK_HD bool g1_in_subgroup(const Fp& x, const Fp& y) {
  G1Affine p;
  p.x = x;
  p.y = y;
  const G1xyzz q1 = g1_mul_x0(xyzz_from_affine(p), [&](const G1xyzz& a) { return xyzz_add_affine(a, x, y); });
  const G1xyzz q2 = g1_mul_x0(q1, [&](const G1xyzz& a) { return xyzz_add(a, q1); });
  if (xyzz_is_inf(q2)) return false;  // (beta x, y) is finite
  // -q2 == (beta x, y):  X2 == beta x ZZ2  and  Y2 + y ZZZ2 == 0
  const Fp bx = fe_mul(fp_beta(), x);
  return fe_eq(q2.X, fe_mul(bx, q2.ZZ)) && fe_is_zero(fe_add(q2.Y, fe_mul(y, q2.ZZZ)));
}

// 32 little-endian bytes as 8 words -> Montgomery scalar
PLK_HD uint8_t fr_decode_words(const uint32_t (&w)[8], Fr& out) {
  Fr c;
#pragma unroll
  for (int i = 0; i < 8; ++i) c.v[i] = w[i];
  out = fe_zero<FrCfg>();
  if (!fe_canonical(c)) return PLK_INGEST_RANGE;
  out = fe_to_mont(c);
  return PLK_INGEST_OK;
}

}  // namespace plk
