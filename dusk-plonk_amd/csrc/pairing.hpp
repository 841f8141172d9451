// pairing.hpp — the BLS12-381 optimal ate pairing over ff.hpp's packed Fp, one source for host
// and device (the reference ends Verifier::verify in multi_miller_loop(..).final_exp() of its
// un-vendored pairing crate, commitment_scheme.rs:24-66).
//
// Tower: Fp2 = Fp[u] / (u^2 + 1); Fp12 = Fp2[w] / (w^6 - xi), xi = 1 + u, as the six Fp2
// coefficients of w^0 .. w^5 (no Fp6 layer: products are the 6 x 6 convolution folded by xi).
//
// An Fp12 value is 144 words: a lane cannot hold two of them in registers. Every Fp12 value
// therefore lives in a MEMORY SLOT and the operations below take slot numbers; only Fp2
// operands are live in registers. The slot store M provides
//     Fp2  ld(int slot, int i) const;      // coefficient of w^i
//     void st(int slot, int i, const Fp2&);
// F12Host is a plain array; pairing.hip's device store is a workspace tiled by wave and laid out
// [slot][coefficient][32-bit word][lane] inside a tile. The loops over coefficients, over the bits of |x| and over the
// Miller steps are real loops (no unrolling): the code stays small.
//
// Lines: the twist y^2 = x^3 + 4 xi is of M type, (x, y) -> (x / w^2, y / w^3). The line through
// T with slope lam at P = (xP, yP), scaled by w^3 (a factor of Fp4, killed by the final
// exponentiation), is (lam xT - yT) + (-lam xP) w^2 + yP w^3. G2 points are prepared on the
// host into their kMillerLines = 68 (lam xT - yT, lam) pairs (63 doublings, 5 additions, in the
// order the loop consumes them); the loop itself never touches G2.
//
// Final exponentiation: 3 (p^4 - p^2 + 1) / r = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3, so the
// result is the CUBE of the plain power (p^12 - 1) / r; gcd(3, r) = 1 keeps "== 1" intact.
#pragma once
#include "ff.hpp"
#include "pairing_consts.hpp"

namespace plk {

#if defined(__HIPCC__)
#define PLK_NOUNROLL _Pragma("nounroll")
#else
#define PLK_NOUNROLL
#endif

constexpr int kMillerLines = 68;  // per G2 point: 63 doublings + 5 additions
constexpr int kF12Slots = 5;      // what miller + final exponentiation need

// ----------------------------------------------------------------------------- Fp2
struct Fp2 {
  Fp c0, c1;
};

PLK_HD Fp2 f2_zero() { return {fe_zero<FpCfg>(), fe_zero<FpCfg>()}; }
PLK_HD Fp2 f2_one() { return {fe_one<FpCfg>(), fe_zero<FpCfg>()}; }
PLK_HD bool f2_is_zero(const Fp2& a) { return fe_is_zero(a.c0) && fe_is_zero(a.c1); }
PLK_HD bool f2_eq(const Fp2& a, const Fp2& b) { return fe_eq(a.c0, b.c0) && fe_eq(a.c1, b.c1); }
PLK_HD Fp2 f2_add(const Fp2& a, const Fp2& b) { return {fe_add(a.c0, b.c0), fe_add(a.c1, b.c1)}; }
PLK_HD Fp2 f2_sub(const Fp2& a, const Fp2& b) { return {fe_sub(a.c0, b.c0), fe_sub(a.c1, b.c1)}; }
PLK_HD Fp2 f2_neg(const Fp2& a) { return {fe_neg(a.c0), fe_neg(a.c1)}; }
PLK_HD Fp2 f2_dbl(const Fp2& a) { return {fe_dbl(a.c0), fe_dbl(a.c1)}; }
PLK_HD Fp2 f2_conj(const Fp2& a) { return {a.c0, fe_neg(a.c1)}; }
// a (1 + u)
PLK_HD Fp2 f2_mul_xi(const Fp2& a) { return {fe_sub(a.c0, a.c1), fe_add(a.c0, a.c1)}; }
PLK_HD Fp2 f2_mul_fp(const Fp2& a, const Fp& k) { return {fe_mul(a.c0, k), fe_mul(a.c1, k)}; }

// Karatsuba: three Fp products
PLK_HD Fp2 f2_mul(const Fp2& a, const Fp2& b) {
  const Fp t0 = fe_mul(a.c0, b.c0), t1 = fe_mul(a.c1, b.c1);
  const Fp t2 = fe_mul(fe_add(a.c0, a.c1), fe_add(b.c0, b.c1));
  return {fe_sub(t0, t1), fe_sub(fe_sub(t2, t0), t1)};
}

// complex squaring: two Fp products
PLK_HD Fp2 f2_sqr(const Fp2& a) {
  const Fp t = fe_mul(a.c0, a.c1);
  return {fe_mul(fe_add(a.c0, a.c1), fe_sub(a.c0, a.c1)), fe_dbl(t)};
}

// one Fp inversion (Fermat); the inverse of zero is zero
PLK_HD Fp2 f2_inv(const Fp2& a) {
  const Fp d = fe_inv(fe_add(fe_sqr(a.c0), fe_sqr(a.c1)));
  return {fe_mul(a.c0, d), fe_neg(fe_mul(a.c1, d))};
}

// Keeps the compiler from forwarding values stored to a slot into later loads of it: the
// point of the slots is that those values leave the registers.
PLK_HD void f12_fence() {
#if defined(__HIP_DEVICE_COMPILE__) || defined(__GNUC__)
  __asm__ volatile("" ::: "memory");
#endif
}

// ----------------------------------------------------------------------------- Fp12 in slots
struct F12Host {
  Fp2 v[kF12Slots][6];
  Fp2 ld(int slot, int i) const { return v[slot][i]; }
  void st(int slot, int i, const Fp2& a) { v[slot][i] = a; }
};

template <class M>
PLK_HD void f12_set_one(M& m, int d) {
  m.st(d, 0, f2_one());
  PLK_NOUNROLL
  for (int i = 1; i < 6; ++i) m.st(d, i, f2_zero());
}

template <class M>
PLK_HD void f12_copy(M& m, int d, int a) {
  PLK_NOUNROLL
  for (int i = 0; i < 6; ++i) m.st(d, i, m.ld(a, i));
}

// a^(p^6): w -> -w. d == a allowed.
template <class M>
PLK_HD void f12_conj(M& m, int d, int a) {
  PLK_NOUNROLL
  for (int i = 0; i < 6; ++i) {
    const Fp2 x = m.ld(a, i);
    m.st(d, i, (i & 1) ? f2_neg(x) : x);
  }
}

// a^p (second = false; coef = xi^(i (p - 1) / 6)) or a^(p^2) (second = true; coef =
// xi^(i (p^2 - 1) / 6)); coef: six Fp2 values. d == a allowed.
template <class M>
PLK_HD void f12_frob(M& m, int d, int a, const Fp2* coef, bool second) {
  PLK_NOUNROLL
  for (int i = 0; i < 6; ++i) {
    Fp2 x = m.ld(a, i);
    if (!second) x = f2_conj(x);
    m.st(d, i, f2_mul(x, coef[i]));
  }
}

template <class M>
PLK_HD bool f12_is_one(const M& m, int a) {
  bool ok = f2_eq(m.ld(a, 0), f2_one());
  PLK_NOUNROLL
  for (int i = 1; i < 6; ++i) ok = ok && f2_is_zero(m.ld(a, i));
  return ok;
}

// d = a b (d differs from a and b): c_k = sum_{i+j=k} a_i b_j + xi sum_{i+j=k+6} a_i b_j,
// 36 Fp2 products, one output coefficient in registers at a time
template <class M>
PLK_HD void f12_mul(M& m, int d, int a, int b) {
  PLK_NOUNROLL
  for (int k = 0; k < 6; ++k) {
    Fp2 lo = f2_zero(), hi = f2_zero();
    PLK_NOUNROLL
    for (int i = 0; i < 6; ++i) {
      const bool wrap = i > k;
      const int j = wrap ? k + 6 - i : k - i;
      const Fp2 t = f2_mul(m.ld(a, i), m.ld(b, j));
      if (wrap)
        hi = f2_add(hi, t);
      else
        lo = f2_add(lo, t);
    }
    m.st(d, k, f2_add(lo, f2_mul_xi(hi)));
  }
  f12_fence();
}

// d = a^2 (d differs from a): the symmetric half of the convolution, 15 products + 6 squares
template <class M>
PLK_HD void f12_sqr(M& m, int d, int a) {
  PLK_NOUNROLL
  for (int k = 0; k < 6; ++k) {
    Fp2 lo = f2_zero(), hi = f2_zero();
    PLK_NOUNROLL
    for (int i = 0; i < 6; ++i) {
      const bool wrap = i > k;
      const int j = wrap ? k + 6 - i : k - i;
      if (i > j) continue;
      const Fp2 x = m.ld(a, i);
      const Fp2 t = (i == j) ? f2_sqr(x) : f2_dbl(f2_mul(x, m.ld(a, j)));
      if (wrap)
        hi = f2_add(hi, t);
      else
        lo = f2_add(lo, t);
    }
    m.st(d, k, f2_add(lo, f2_mul_xi(hi)));
  }
  f12_fence();
}

// d = a (c0 + c2 w^2 + y w^3), the sparse line product (d differs from a): 2 Fp2 products and
// one Fp2-by-Fp product per coefficient
template <class M>
PLK_HD void f12_mul_line(M& m, int d, int a, const Fp2& c0, const Fp2& c2, const Fp& y) {
  PLK_NOUNROLL
  for (int k = 0; k < 6; ++k) {
    const int i2 = k < 2 ? k + 4 : k - 2, i3 = k < 3 ? k + 3 : k - 3;
    Fp2 u = f2_mul(m.ld(a, i2), c2);
    if (k < 2) u = f2_mul_xi(u);
    Fp2 v = f2_mul_fp(m.ld(a, i3), y);
    if (k < 3) v = f2_mul_xi(v);
    m.st(d, k, f2_add(f2_add(f2_mul(m.ld(a, k), c0), u), v));
  }
  f12_fence();
}

// d = a^2 for a in the cyclotomic subgroup (a^(p^4 - p^2 + 1) = 1), d differs from a.
// Granger-Scott over Fp4 = Fp2[s], s = w^3, s^2 = xi: a = A + B w + C w^2 with A = (a0, a3),
// B = (a1, a4), C = (a2, a5) in Fp4, and
//   a^2 = (3 A^2 - 2 conj A) + (3 s C^2 + 2 conj B) w + (3 B^2 - 2 conj C) w^2,
// conj (x + y s) = x - y s. Three Fp4 squarings of three Fp2 squarings each: 18 Fp products.
template <class M>
PLK_HD void f12_cyc_sqr(M& m, int d, int a) {
  PLK_NOUNROLL
  for (int t = 0; t < 3; ++t) {
    const Fp2 x = m.ld(a, t), y = m.ld(a, t + 3);
    const Fp2 xx = f2_sqr(x), yy = f2_sqr(y);
    Fp2 s0 = f2_add(xx, f2_mul_xi(yy));                        // (x + y s)^2 = s0 + s1 s
    Fp2 s1 = f2_sub(f2_sub(f2_sqr(f2_add(x, y)), xx), yy);
    const int o = t == 0 ? 0 : (t == 1 ? 2 : 1);  // A^2 -> w^0, B^2 -> w^2, C^2 -> w^1
    if (t == 2) {                                  // times s
      const Fp2 n0 = f2_mul_xi(s1);
      s1 = s0;
      s0 = n0;
    }
    const Fp2 g0 = f2_dbl(m.ld(a, o)), g1 = f2_dbl(m.ld(a, o + 3));
    const Fp2 h0 = f2_add(f2_dbl(s0), s0), h1 = f2_add(f2_dbl(s1), s1);
    if (t == 2) {
      m.st(d, o, f2_add(h0, g0));
      m.st(d, o + 3, f2_sub(h1, g1));
    } else {
      m.st(d, o, f2_sub(h0, g0));
      m.st(d, o + 3, f2_add(h1, g1));
    }
  }
  f12_fence();
}

// t = N^-1 in place for N in Fp6 = Fp2[v], v = w^2 (even coefficients of t; the odd ones are
// overwritten and left zero): the cubic-extension formula with one Fp2 (hence one Fp) inversion.
// With N = a conj(a) this gives a^-1 = conj(a) N^-1. The inverse of zero is zero.
template <class M>
PLK_HD void f12_inv_even(M& m, int t) {
  // the cofactors go to the odd coefficients; operands are loaded where they are used
  m.st(t, 1, f2_sub(f2_sqr(m.ld(t, 0)), f2_mul_xi(f2_mul(m.ld(t, 2), m.ld(t, 4)))));
  f12_fence();
  m.st(t, 3, f2_sub(f2_mul_xi(f2_sqr(m.ld(t, 4))), f2_mul(m.ld(t, 0), m.ld(t, 2))));
  f12_fence();
  m.st(t, 5, f2_sub(f2_sqr(m.ld(t, 2)), f2_mul(m.ld(t, 0), m.ld(t, 4))));
  f12_fence();
  Fp2 s = f2_mul(m.ld(t, 4), m.ld(t, 3));
  f12_fence();
  s = f2_add(s, f2_mul(m.ld(t, 2), m.ld(t, 5)));
  f12_fence();
  const Fp2 di = f2_inv(f2_add(f2_mul(m.ld(t, 0), m.ld(t, 1)), f2_mul_xi(s)));
  PLK_NOUNROLL
  for (int i = 0; i < 3; ++i) {
    m.st(t, 2 * i, f2_mul(m.ld(t, 2 * i + 1), di));
    m.st(t, 2 * i + 1, f2_zero());
  }
  f12_fence();
}

// The final exponentiation as a program for a small sequencer: each Fp12 primitive is inlined
// ONCE into the loop below whatever the number of steps (25 steps and five exponentiations by
// x would otherwise be ~140 inlined Fp products). Instruction: op | d << 4 | a << 7 | b << 10.
enum : uint32_t { kOpEnd, kOpConj, kOpMul, kOpFrob1, kOpFrob2, kOpExpX, kOpCycSqr, kOpInvEven, kOpCopy };
#define PLK_F12_INS(op, d, a, b) ((uint16_t)((op) | ((d) << 4) | ((a) << 7) | ((b) << 10)))
// Slot 0 = f. Easy part: m = f^((p^6 - 1)(p^2 + 1)) = frob^2(g) g with g = conj(f) / f. Hard
// part: t0 = m^x conj(m), t1 = t0^x conj(t0), t2 = t1^x frob(t1),
// t3 = (t2^x)^x frob^2(t2) conj(t2); result t3 m^3, left in slot 3. ExpX d a b: d = a^x, b scratch.
static constexpr uint16_t kFinalExpProg[] = {
    PLK_F12_INS(kOpConj, 2, 0, 0),     // conj(f)
    PLK_F12_INS(kOpMul, 3, 0, 2),      // N = f conj(f)
    PLK_F12_INS(kOpInvEven, 3, 0, 0),  // N^-1
    PLK_F12_INS(kOpMul, 1, 2, 3),      // f^-1
    PLK_F12_INS(kOpMul, 3, 2, 1),      // g = f^(p^6 - 1)
    PLK_F12_INS(kOpFrob2, 2, 3, 0),
    PLK_F12_INS(kOpMul, 0, 2, 3),      // m
    PLK_F12_INS(kOpExpX, 1, 0, 2),
    PLK_F12_INS(kOpConj, 2, 0, 0),
    PLK_F12_INS(kOpMul, 3, 1, 2),      // t0
    PLK_F12_INS(kOpExpX, 1, 3, 2),
    PLK_F12_INS(kOpConj, 2, 3, 0),
    PLK_F12_INS(kOpMul, 4, 1, 2),      // t1
    PLK_F12_INS(kOpExpX, 1, 4, 2),
    PLK_F12_INS(kOpFrob1, 2, 4, 0),
    PLK_F12_INS(kOpMul, 3, 1, 2),      // t2
    PLK_F12_INS(kOpExpX, 1, 3, 2),
    PLK_F12_INS(kOpExpX, 4, 1, 2),     // (t2^x)^x
    PLK_F12_INS(kOpFrob2, 2, 3, 0),
    PLK_F12_INS(kOpMul, 1, 4, 2),
    PLK_F12_INS(kOpConj, 2, 3, 0),
    PLK_F12_INS(kOpMul, 4, 1, 2),      // t3
    PLK_F12_INS(kOpCycSqr, 1, 0, 0),
    PLK_F12_INS(kOpMul, 2, 1, 0),      // m^3
    PLK_F12_INS(kOpMul, 3, 4, 2),      // t3 m^3
    PLK_F12_INS(kOpEnd, 0, 0, 0),
};
constexpr int kFinalExpSlot = 3;

// Slot 0 -> (slot 0)^(3 (p^12 - 1) / r) in slot kFinalExpSlot. frob: 12 Fp2 values,
// xi^(i (p - 1) / 6) then xi^(i (p^2 - 1) / 6), i < 6. Uses all kF12Slots slots.
// d = a^x = conj(a^|x|) (a in the cyclotomic subgroup) runs as micro-steps of the same loop:
// d = a; per bit of |x| below the top one b = d^2 (cyclotomic), then d = b a or d = b; d = conj d.
template <class M>
PLK_HD int f12_final_exp(M& m, const Fp2* frob) {
  int pc = 0, bit = -1, phase = 0;  // bit: -1 outside an ExpX, -2 its closing conjugation
  PLK_NOUNROLL
  for (;;) {
    const uint32_t ins = kFinalExpProg[pc];
    uint32_t op = ins & 15u;
    int d = (int)((ins >> 4) & 7u), a = (int)((ins >> 7) & 7u), b = (int)((ins >> 10) & 7u);
    if (op == kOpEnd) break;
    if (op == kOpExpX) {
      if (bit == -1) {
        op = kOpCopy;
        bit = 62;
        phase = 0;
      } else if (bit == -2) {
        op = kOpConj;
        a = d;
        bit = -1;
        ++pc;
      } else if (phase == 0) {
        op = kOpCycSqr;
        a = d;
        d = b;
        phase = 1;
      } else {
        const bool set = (pairing_consts::kXAbs >> bit) & 1ull;
        op = set ? kOpMul : kOpCopy;
        const int src = a;
        a = b;
        b = src;
        phase = 0;
        if (--bit < 0) bit = -2;
      }
    } else {
      ++pc;
    }
    switch (op) {
      case kOpConj: f12_conj(m, d, a); break;
      case kOpMul: f12_mul(m, d, a, b); break;
      case kOpFrob1: f12_frob(m, d, a, frob, false); break;
      case kOpFrob2: f12_frob(m, d, a, frob + 6, true); break;
      case kOpCycSqr: f12_cyc_sqr(m, d, a); break;
      case kOpInvEven: f12_inv_even(m, d); break;
      default: f12_copy(m, d, a); break;
    }
    f12_fence();
  }
  return kFinalExpSlot;
}

// Slot 0 = ML(P0, Q0) [ML(P1, Q1)] with the squarings shared (the reference's multi_miller_loop),
// conjugated for the negative x. tab0 / tab1: the prepared lines of Q0 / Q1 (kMillerLines pairs
// (lam xT - yT, lam)); on0 / on1 false: P at infinity, the factor one. two = false leaves the
// second pair out altogether (uniform). Uses slots 0 and 1.
template <class M>
PLK_HD void miller_loop(M& m, const Fp2* tab0, bool on0, const Fp& x0, const Fp& y0, bool two,
                        const Fp2* tab1, bool on1, const Fp& x1, const Fp& y1) {
  int f = 0, t = 1;
  f12_set_one(m, f);
  f12_fence();
  int idx = 0;
  PLK_NOUNROLL
  for (int b = 62; b >= 0; --b) {
    f12_sqr(m, t, f);
    { const int s = f; f = t; t = s; }
    const int steps = 1 + (int)((pairing_consts::kXAbs >> b) & 1ull);
    PLK_NOUNROLL
    for (int s = 0; s < steps; ++s, ++idx) {
      PLK_NOUNROLL
      for (int q = 0; q < (two ? 2 : 1); ++q) {
        const Fp2* row = (q ? tab1 : tab0) + 2 * idx;
        const bool on = q ? on1 : on0;
        if (on) {
          const Fp2 c2 = f2_neg(f2_mul_fp(row[1], q ? x1 : x0));
          f12_mul_line(m, t, f, row[0], c2, q ? y1 : y0);
        } else {
          f12_copy(m, t, f);
          f12_fence();
        }
        { const int sw = f; f = t; t = sw; }
      }
    }
  }
  f12_conj(m, 0, f);
  f12_fence();
}

}  // namespace plk
