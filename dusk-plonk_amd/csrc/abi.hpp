// abi.hpp — the values at the C-ABI boundary (include/plk.h): how plk_fr / plk_g1 limbs, the
// big-endian bytes of the compressed encodings and the items of a byte buffer become field
// elements and points, and back. Every translation unit that meets caller data goes through here,
// so a change of an encoding or of a validation rule is made once.
//
// PLK_HD code on the packed field of ff.hpp only: kernels and host code run the same functions,
// and the header compiles without HIP (tools/*_selftest.cpp reach it through pairing_host.hpp).
//
// The rules for a plk_g1 from a caller (g1_load<true>, plk_msm_points' contract):
//  - the infinity word is 0 or 1;
//  - a finite point has canonical limbs (< p) and lies on y^2 = x^3 + 4;
//  - under infinity = 1 the coordinate words are not looked at; the point loads as (0, 0).
// g1_load<false> is the plain load for points that were validated before (or are taken on faith):
// any non-zero infinity word means the identity.
#pragma once
#include <stdint.h>

#include "../../include/plk.h"
#include "ff.hpp"

namespace plk {

// ---- limbs <-> elements: N / 2 little-endian u64 limbs are the memory image of Fe<C> ------------
template <class C>
PLK_HD Fe<C> fe_of_abi(const uint64_t* l) {
  Fe<C> r;
#pragma unroll
  for (int i = 0; i < C::N / 2; ++i) {
    r.v[2 * i] = (uint32_t)l[i];
    r.v[2 * i + 1] = (uint32_t)(l[i] >> 32);
  }
  return r;
}
template <class C>
PLK_HD void fe_to_abi(const Fe<C>& a, uint64_t* l) {
#pragma unroll
  for (int i = 0; i < C::N / 2; ++i) l[i] = (uint64_t)a.v[2 * i] | ((uint64_t)a.v[2 * i + 1] << 32);
}

// a < modulus, for a value in plain 32-bit words
template <class C>
PLK_HD bool fe_canonical(const Fe<C>& a) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < C::N; ++i) {
    const uint64_t t = (uint64_t)a.v[i] - C::P[i] - borrow;
    borrow = (uint32_t)(t >> 63);
  }
  return borrow != 0;
}
template <class C>
PLK_HD bool abi_canonical(const uint64_t* l) {
  return fe_canonical(fe_of_abi<C>(l));
}

PLK_HD Fr fr_from_abi(const plk_fr& a) { return fe_of_abi<FrCfg>(a.l); }
PLK_HD plk_fr fr_to_abi(const Fr& a) {
  plk_fr r;
  fe_to_abi(a, r.l);
  return r;
}

// ---- curve constants and the curve equation ----------------------------------------------------
PLK_HD Fp fp_const(const uint32_t (&w)[12]) {
  Fp r;
#pragma unroll
  for (int i = 0; i < 12; ++i) r.v[i] = w[i];
  return r;
}
// 4 and beta in Montgomery form; beta = 0x5f19672f...fffefffe, the cube root of unity with
// (beta x, y) = [-x0^2] (x, y) on G1
struct FpFour {
  static constexpr uint32_t W[12] = {0x000cfff3u, 0xaa270000u, 0xfc34000au, 0x53cc0032u,
                                     0x6b0a807fu, 0x478fe97au, 0xe6ba24d7u, 0xb1d37ebeu,
                                     0xbf78ab2fu, 0x8ec9733bu, 0x3d83de7eu, 0x09d64551u};
};
PLK_HD Fp fp_four() {
  Fp r;
#pragma unroll
  for (int i = 0; i < 12; ++i) r.v[i] = FpFour::W[i];
  return r;
}
PLK_HD Fp fp_beta() {
  const uint32_t w[12] = {0x798a64e8u, 0x30f1361bu, 0x7ece5a2au, 0xf3b8ddabu, 0xc61577f7u, 0x16a8ca3au,
                          0x74fd029bu, 0xc26a2ff8u, 0x60701c6eu, 0x3636b766u, 0x241b6160u, 0x051ba4abu};
  return fp_const(w);
}
// the one value of 4: fp_four() is the field's own one doubled twice
constexpr bool fp_four_is_one_doubled_twice() {
  uint32_t a[12] = {};
  for (int i = 0; i < 12; ++i) a[i] = FpCfg::ONE[i];
  for (int rep = 0; rep < 2; ++rep) {  // a = 2 a mod p (2 a < 2^384)
    uint32_t d[12] = {}, e[12] = {};
    uint64_t carry = 0, borrow = 0;
    for (int i = 0; i < 12; ++i) {
      const uint64_t t = 2 * (uint64_t)a[i] + carry;
      d[i] = (uint32_t)t;
      carry = t >> 32;
    }
    for (int i = 0; i < 12; ++i) {
      const uint64_t t = (uint64_t)d[i] - FpCfg::P[i] - borrow;
      e[i] = (uint32_t)t;
      borrow = t >> 63;
    }
    for (int i = 0; i < 12; ++i) a[i] = borrow ? d[i] : e[i];
  }
  for (int i = 0; i < 12; ++i)
    if (a[i] != FpFour::W[i]) return false;
  return true;
}
static_assert(fp_four_is_one_doubled_twice(), "fp_four() == fe_dbl(fe_dbl(fe_one))");

PLK_HD bool g1_on_curve(const Fp& x, const Fp& y) {
  Fp t = fe_sqr(x);  // x^3 + 4 before y^2: k_var_prepare, which keeps x and y, needs 36 VGPRs fewer
  t = fe_mul(t, x);
  t = fe_add(t, fp_four());
  return fe_is_zero(fe_sub(fe_sqr(y), t));
}
// the coordinates of a finite point as they arrive: canonical and on the curve
PLK_HD bool g1_coords_valid(const Fp& x, const Fp& y) {
  // both range tests without a branch between them: k_g1_validate keeps 5 waves per SIMD
  const bool canonical = fe_canonical(x) & fe_canonical(y);
  return canonical && g1_on_curve(x, y);
}

// the standard generator, Montgomery form: the one table of its words
PLK_HD void g1_generator(Fp& x, Fp& y) {
  const uint32_t gx[12] = {0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu,
                           0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u};
  const uint32_t gy[12] = {0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu,
                           0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u};
  x = fe_to_mont(fp_const(gx));
  y = fe_to_mont(fp_const(gy));
}

// ---- plk_g1 <-> (x, y, identity) ---------------------------------------------------------------
struct G1Abi {
  Fp x, y;   // Montgomery form; zero for an identity loaded with validate
  bool inf;  // the identity
  bool ok;   // validate: the rules at the head of this file hold; otherwise true
};

template <bool validate>
PLK_HD G1Abi g1_load(const plk_g1* p) {
  G1Abi r;
  const uint64_t flag = p->infinity;
  r.inf = flag != 0;
  r.ok = !validate || flag <= 1;
  r.x = r.y = fe_zero<FpCfg>();
  if (!validate || !r.inf) {
    r.x = fe_of_abi<FpCfg>(p->x);
    r.y = fe_of_abi<FpCfg>(p->y);
    if (validate) r.ok = g1_coords_valid(r.x, r.y);
  }
  return r;
}

// zeros and infinity = 1 for the identity
PLK_HD void g1_store(const Fp& x, const Fp& y, bool finite, plk_g1* out) {
  const Fp zero = fe_zero<FpCfg>();
  fe_to_abi(finite ? x : zero, out->x);
  fe_to_abi(finite ? y : zero, out->y);
  out->infinity = finite ? 0 : 1;
}

// ---- big-endian words: 48 big-endian bytes read from memory as 12 little-endian words ----------
PLK_HD uint32_t bswap32(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
}
// the value's words, plain (word i of the value is the byte-swapped word 11 - i)
PLK_HD Fp fp_of_be_words(const uint32_t* w) {
  Fp r;
#pragma unroll
  for (int i = 0; i < 12; ++i) r.v[i] = bswap32(w[11 - i]);
  return r;
}
// Montgomery value -> the 12 words of its 48 big-endian bytes
PLK_HD void fp_to_be_words(const Fp& a_mont, uint32_t* out) {
  const Fp a = fe_from_mont(a_mont);
#pragma unroll
  for (int k = 0; k < 12; ++k) out[k] = bswap32(a.v[11 - k]);
}

// zkcrypto's compressed G1 as the 12 words of its 48 bytes. x, y: Montgomery form.
PLK_HD void g1_compress_words(const Fp& x_mont, const Fp& y_mont, bool infinity, uint32_t out[12]) {
  const Fp y = fe_from_mont(y_mont), ny = fe_neg(y);
  // sort flag: y is the larger of y, -y. Decided at the highest differing word.
  bool larger = false, decided = false;
#pragma unroll
  for (int i = 11; i >= 0; --i) {
    if (!decided && y.v[i] != ny.v[i]) {
      larger = y.v[i] > ny.v[i];
      decided = true;
    }
  }
  fp_to_be_words(x_mont, out);
#pragma unroll
  for (int k = 0; k < 12; ++k) out[k] = infinity ? 0u : out[k];
  out[0] |= infinity ? 0xc0u : (0x80u | (larger ? 0x20u : 0u));
}

// ---- items of a byte buffer as words -----------------------------------------------------------
// N words of a 16-byte aligned item, by 16-byte vector loads
typedef uint32_t abi_u32x4 __attribute__((vector_size(16)));
template <int N>
PLK_HD void ld_words(const uint8_t* p, uint32_t (&w)[N]) {
  static_assert(N % 4 == 0, "whole 16-byte vectors");
  const abi_u32x4* src = reinterpret_cast<const abi_u32x4*>(p);
#pragma unroll
  for (int i = 0; i < N / 4; ++i) {
    const abi_u32x4 q = src[i];
    w[4 * i] = q[0];
    w[4 * i + 1] = q[1];
    w[4 * i + 2] = q[2];
    w[4 * i + 3] = q[3];
  }
}
// the host twin: no alignment asked
template <int N>
inline void words_of_bytes(const uint8_t* b, uint32_t (&w)[N]) {
  for (int i = 0; i < N; ++i)
    w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
           ((uint32_t)b[4 * i + 3] << 24);
}
template <int N>
inline void bytes_of_words(const uint32_t (&w)[N], uint8_t* b) {
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < 4; ++k) b[4 * i + k] = (uint8_t)(w[i] >> (8 * k));
}

// the 48 bytes of zkcrypto's compressed G1 (host): the one byte serializer on top of the words
inline void g1_compress_bytes(const Fp& x_mont, const Fp& y_mont, bool infinity, uint8_t out[48]) {
  uint32_t w[12];
  g1_compress_words(x_mont, y_mont, infinity, w);
  bytes_of_words(w, out);
}

}  // namespace plk
