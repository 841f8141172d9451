// pairing_host.hpp — the host-only half of the pairing: affine G2 arithmetic (one Fp2 inversion
// per step; it runs once per key), the preparation of a G2 point into its Miller-loop lines, the
// ABI conversions (on abi.hpp) and the host pairing check. Plain C++ (no HIP): pairing.hip includes it, and so
// does tools/pairing_selftest.cpp, which runs it under the host sanitizers.
#pragma once
#include <string.h>

#include <vector>

#include "../../include/plk.h"
#include "abi.hpp"
#include "pairing.hpp"

namespace plk {

struct G2Aff {
  Fp2 x, y;
  bool inf;
};

struct G1In {
  Fp x, y;
  bool inf;
};

inline Fp fp_from_words(const uint32_t* w) {
  Fp r;
  for (int i = 0; i < 12; ++i) r.v[i] = w[i];
  return r;
}

inline Fp2 f2_from_words(const uint32_t (*w)[12]) { return {fp_from_words(w[0]), fp_from_words(w[1])}; }

// xi^(i (p - 1) / 6), i < 6, then xi^(i (p^2 - 1) / 6), i < 6 (f12_final_exp's table)
inline void frob_table(Fp2 out[12]) {
  for (int i = 0; i < 6; ++i) {
    out[i] = f2_from_words(pairing_consts::kFrob1[i]);
    out[6 + i] = f2_from_words(pairing_consts::kFrob2[i]);
  }
}

inline G2Aff g2_generator() {
  return {f2_from_words(pairing_consts::kG2Gen[0]), f2_from_words(pairing_consts::kG2Gen[1]), false};
}

inline G2Aff g2_infinity() { return {f2_zero(), f2_zero(), true}; }

// y^2 = x^3 + 4 xi
inline bool g2_on_curve(const G2Aff& q) {
  if (q.inf) return true;
  const Fp2 b = f2_mul_xi({fp_four(), fe_zero<FpCfg>()});
  return f2_eq(f2_sqr(q.y), f2_add(f2_mul(f2_sqr(q.x), q.x), b));
}

// a + b, every case; *lam (optional) receives the slope when both are finite and the sum is
inline G2Aff g2_add(const G2Aff& a, const G2Aff& b, Fp2* lam_out = nullptr) {
  if (a.inf) return b;
  if (b.inf) return a;
  Fp2 lam;
  if (f2_eq(a.x, b.x)) {
    if (!f2_eq(a.y, b.y) || f2_is_zero(a.y)) return g2_infinity();
    const Fp2 xx = f2_sqr(a.x);
    lam = f2_mul(f2_add(f2_dbl(xx), xx), f2_inv(f2_dbl(a.y)));
  } else {
    lam = f2_mul(f2_sub(b.y, a.y), f2_inv(f2_sub(b.x, a.x)));
  }
  G2Aff r;
  r.x = f2_sub(f2_sub(f2_sqr(lam), a.x), b.x);
  r.y = f2_sub(f2_mul(lam, f2_sub(a.x, r.x)), a.y);
  r.inf = false;
  if (lam_out) *lam_out = lam;
  return r;
}

// [e] q for a little-endian exponent of `words` 32-bit words (plain integers, not Montgomery)
inline G2Aff g2_mul(const G2Aff& q, const uint32_t* e, int words) {
  G2Aff acc = g2_infinity();
  for (int w = words - 1; w >= 0; --w)
    for (int b = 31; b >= 0; --b) {
      acc = g2_add(acc, acc);
      if ((e[w] >> b) & 1u) acc = g2_add(acc, q);
    }
  return acc;
}

inline bool g2_in_subgroup(const G2Aff& q) { return g2_mul(q, FrCfg::P, 8).inf; }

// The kMillerLines (lam xT - yT, lam) pairs of q in the order miller_loop consumes them. False
// when a step meets infinity (q at infinity or of small order): such a point has no table.
inline bool g2_prepare(const G2Aff& q, Fp2* out) {
  if (q.inf) return false;
  G2Aff t = q;
  int idx = 0;
  for (int b = 62; b >= 0; --b) {
    const int steps = 1 + (int)((pairing_consts::kXAbs >> b) & 1ull);
    for (int s = 0; s < steps; ++s, ++idx) {
      Fp2 lam;
      const G2Aff n = g2_add(t, s ? q : t, &lam);
      if (n.inf) return false;
      out[2 * idx] = f2_sub(f2_mul(lam, t.x), t.y);
      out[2 * idx + 1] = lam;
      t = n;
    }
  }
  return idx == kMillerLines;
}

// ---- ABI conversions (abi.hpp) ----------------------------------------------------------------
// PLK_E_ARG for a point g1_load<true> refuses (plk_msm_points' contract)
inline int g1_from_abi(const plk_g1& p, G1In& o) {
  const G1Abi a = g1_load<true>(&p);
  o = {a.x, a.y, a.inf};
  return a.ok ? PLK_OK : PLK_E_ARG;
}

// PLK_E_ARG unless q is finite, canonical and on the twist (the subgroup check is the caller's)
inline int g2_from_abi(const plk_g2& q, G2Aff& o) {
  if (q.infinity != 0) return PLK_E_ARG;
  o.x = {fe_of_abi<FpCfg>(q.x), fe_of_abi<FpCfg>(q.x + 6)};
  o.y = {fe_of_abi<FpCfg>(q.y), fe_of_abi<FpCfg>(q.y + 6)};
  o.inf = false;
  if (!fe_canonical(o.x.c0) || !fe_canonical(o.x.c1) || !fe_canonical(o.y.c0) || !fe_canonical(o.y.c1))
    return PLK_E_ARG;
  return g2_on_curve(o) ? PLK_OK : PLK_E_ARG;
}

inline void g2_to_abi(const G2Aff& q, plk_g2* o) {
  memset(o, 0, sizeof *o);
  if (q.inf) {
    o->infinity = 1;
    return;
  }
  fe_to_abi(q.x.c0, o->x);
  fe_to_abi(q.x.c1, o->x + 6);
  fe_to_abi(q.y.c0, o->y);
  fe_to_abi(q.y.c1, o->y + 6);
}

// ---- zkcrypto's G2 byte forms (include/plk.h "An SRS from bytes") -----------------------------
// a^e for a little-endian exponent of 12 words (a plain integer)
inline Fp2 f2_pow(const Fp2& a, const uint32_t* e) {
  Fp2 r = f2_one();
  for (int w = 11; w >= 0; --w)
    for (int b = 31; b >= 0; --b) {
      r = f2_sqr(r);
      if ((e[w] >> b) & 1u) r = f2_mul(r, a);
    }
  return r;
}

// A square root of a in Fp2, p = 3 mod 4 (Adj, Rodriguez-Henriquez, eprint 2012/685 algorithm 9,
// two exponentiations): a1 = a^((p-3)/4), x0 = a1 a, alpha = a1 x0 = a^((p-1)/2). alpha = -1:
// the root is u x0; else (1 + alpha)^((p-1)/2) x0. The candidate is verified by squaring, so a
// non-square gives false whatever the branches computed.
inline bool f2_sqrt(const Fp2& a, Fp2& out) {
  out = f2_zero();
  if (f2_is_zero(a)) return true;
  uint32_t e1[12], e2[12];  // (p - 3) / 4 and (p - 1) / 2
  for (int i = 0; i < 12; ++i) {
    const uint32_t hi = i < 11 ? FpCfg::P[i + 1] : 0u;
    e1[i] = (FpCfg::P[i] >> 2) | (hi << 30);  // p = 3 mod 4: floor(p / 4) = (p - 3) / 4
    e2[i] = (FpCfg::P[i] >> 1) | (hi << 31);  // p odd: floor(p / 2) = (p - 1) / 2
  }
  const Fp2 a1 = f2_pow(a, e1);
  const Fp2 x0 = f2_mul(a1, a);
  const Fp2 alpha = f2_mul(a1, x0);
  Fp2 x;
  if (f2_eq(alpha, f2_neg(f2_one()))) {
    x = {fe_neg(x0.c1), x0.c0};  // u x0
  } else {
    x = f2_mul(f2_pow(f2_add(f2_one(), alpha), e2), x0);
  }
  if (!f2_eq(f2_sqr(x), a)) return false;
  out = x;
  return true;
}

// 48 big-endian bytes -> a plain (not Montgomery) value; the caller masks flag bits first
inline Fp fp_from_be(const uint8_t* b) {
  Fp r;
  for (int i = 0; i < 12; ++i) {
    const uint8_t* q = b + 44 - 4 * i;
    r.v[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
  return r;
}

// Montgomery value -> 48 big-endian bytes
inline void fp_to_be(const Fp& a_mont, uint8_t* b) {
  const Fp a = fe_from_mont(a_mont);
  for (int i = 0; i < 12; ++i)
    for (int k = 0; k < 4; ++k) b[47 - (4 * i + k)] = (uint8_t)(a.v[i] >> (8 * k));
}

// a > (p - 1) / 2 for a Montgomery value, i.e. a > -a as integers
inline bool fp_is_larger_half(const Fp& a_mont) {
  const Fp a = fe_from_mont(a_mont), na = fe_from_mont(fe_neg(a_mont));
  for (int i = 11; i >= 0; --i)
    if (a.v[i] != na.v[i]) return a.v[i] > na.v[i];
  return false;
}

// the sort bit of a G2 point: y is the lexicographically larger of +-y, c1 first
inline bool g2_y_is_larger(const Fp2& y) {
  return fe_is_zero(y.c1) ? fp_is_larger_half(y.c0) : fp_is_larger_half(y.c1);
}

// compressed (96 B) or uncompressed (192 B) -> a point on the twist or the identity. PLK_E_ARG
// for every strict rejection; the subgroup check is the caller's.
inline int g2_from_bytes(const uint8_t* in, bool compressed, G2Aff& o) {
  const size_t len = compressed ? 96 : 192;
  const uint8_t flags = in[0] & 0xe0;
  o = g2_infinity();
  if (((flags & 0x80) != 0) != compressed) return PLK_E_ARG;
  if (flags & 0x40) {  // infinity: the flag byte alone
    if (in[0] != (compressed ? 0xc0 : 0x40)) return PLK_E_ARG;
    for (size_t i = 1; i < len; ++i)
      if (in[i]) return PLK_E_ARG;
    return PLK_OK;
  }
  if (!compressed && (flags & 0x20)) return PLK_E_ARG;
  uint8_t first[48];
  memcpy(first, in, 48);
  first[0] &= 0x1f;
  const Fp xc1 = fp_from_be(first), xc0 = fp_from_be(in + 48);
  if (!fe_canonical(xc1) || !fe_canonical(xc0)) return PLK_E_ARG;
  o.x = {fe_to_mont(xc0), fe_to_mont(xc1)};
  o.inf = false;
  if (compressed) {
    const Fp2 rhs = f2_add(f2_mul(f2_sqr(o.x), o.x), f2_mul_xi({fp_four(), fe_zero<FpCfg>()}));
    Fp2 y;
    if (!f2_sqrt(rhs, y)) return PLK_E_ARG;
    if (g2_y_is_larger(y) != ((flags & 0x20) != 0)) y = f2_neg(y);
    o.y = y;
    return PLK_OK;
  }
  const Fp yc1 = fp_from_be(in + 96), yc0 = fp_from_be(in + 144);
  if (!fe_canonical(yc1) || !fe_canonical(yc0)) return PLK_E_ARG;
  o.y = {fe_to_mont(yc0), fe_to_mont(yc1)};
  return g2_on_curve(o) ? PLK_OK : PLK_E_ARG;
}

inline void g2_to_bytes(const G2Aff& q, bool compressed, uint8_t* out) {
  memset(out, 0, compressed ? 96 : 192);
  if (q.inf) {
    out[0] = compressed ? 0xc0 : 0x40;
    return;
  }
  fp_to_be(q.x.c1, out);
  fp_to_be(q.x.c0, out + 48);
  if (compressed) {
    out[0] |= 0x80 | (g2_y_is_larger(q.y) ? 0x20 : 0);
    return;
  }
  fp_to_be(q.y.c1, out + 96);
  fp_to_be(q.y.c0, out + 144);
}

// slot 0 of m = ML(c, Q0) ML(-w, Q1): the value the check raises to the final power (and what
// plk_debug_miller returns)
inline void miller_check_host(F12Host& m, const Fp2* lines0, const Fp2* lines1, const G1In& c,
                              const G1In& w) {
  miller_loop(m, lines0, !c.inf, c.x, c.y, true, lines1, !w.inf, w.x, fe_neg(w.y));
}

// e(c, Q0) == e(w, Q1), as ML(c, Q0) ML(-w, Q1) -> final exponentiation == 1. lines0 / lines1:
// the prepared tables of Q0 / Q1; frob: frob_table.
inline bool pairing_check_host(const Fp2* lines0, const Fp2* lines1, const Fp2* frob, const G1In& c,
                               const G1In& w) {
  F12Host m;
  miller_check_host(m, lines0, lines1, c, w);
  const int r = f12_final_exp(m, frob);
  return f12_is_one(m, r);
}

// slot 0 of m = ML(p, Q), one pair
inline void miller_value_host(F12Host& m, const Fp2* lines, const G1In& p) {
  miller_loop(m, lines, !p.inf, p.x, p.y, false, lines, false, p.x, p.y);
}

// out[72] = ML(p, Q)^(3 (p^12 - 1) / r), the six coefficients as (c0, c1) Montgomery limbs
inline void pairing_value_host(const Fp2* lines, const Fp2* frob, const G1In& p, uint64_t* out) {
  F12Host m;
  miller_value_host(m, lines, p);
  const int r = f12_final_exp(m, frob);
  for (int i = 0; i < 6; ++i) {
    const Fp2 a = m.ld(r, i);
    fe_to_abi(a.c0, out + 12 * i);
    fe_to_abi(a.c1, out + 12 * i + 6);
  }
}

}  // namespace plk
