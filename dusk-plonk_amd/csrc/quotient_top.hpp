// quotient_top.hpp — the top seven coefficients of the quotient numerator in closed form
// (prover.hpp, "The quotient domain"). Top is a polynomial known only by a degree bound D and
// its coefficients D-6 .. D: a power series in 1/X truncated after kTop terms. The top kTop
// coefficients of a sum or a product depend only on the top kTop coefficients of the operands,
// so the widget and permutation formulas of protocol.hpp, instantiated on Top, give
// N[5n .. 5n + 6] = t[4n .. 4n + 6] from a handful of field elements per factor polynomial.
//
// PLK_HD code like protocol.hpp: no HIP calls, no allocation, and plain g++ compiles it.
#pragma once
#include <stdint.h>

#include "protocol.hpp"

namespace plk {

constexpr int kTop = 7;

struct Top {
  int64_t deg;  // degree bound D: no coefficient above X^D
  Fr c[kTop];   // c[i]: the coefficient of X^(D - i); zero where D - i < 0
  PLK_HD Top() : deg(0) {
    for (int i = 0; i < kTop; ++i) c[i] = fe_zero<FrCfg>();
  }
  PLK_HD Top(const Fr& k) : deg(0) {  // the constant k
    c[0] = k;
    for (int i = 1; i < kTop; ++i) c[i] = fe_zero<FrCfg>();
  }
};

// from the coefficients D-6 .. D in ascending order, as a coefficient array holds them
PLK_HD Top top_from_coeffs(const Fr* asc, int64_t deg) {
  Top r;
  r.deg = deg;
  for (int i = 0; i < kTop; ++i) r.c[i] = deg - i >= 0 ? asc[kTop - 1 - i] : fe_zero<FrCfg>();
  return r;
}

// the coefficient of X^k (zero above the degree bound; below D - 6 it is not known: the caller
// asks only for k >= deg - 6)
PLK_HD Fr top_coeff(const Top& p, int64_t k) {
  const int64_t i = p.deg - k;
  return i >= 0 && i < kTop ? p.c[i] : fe_zero<FrCfg>();
}

// Sums align by degree: a term whose degree is lower by kTop or more drops out
PLK_HD Top top_axpy(const Top& a, const Top& b, bool sub) {
  const Top& hi = a.deg >= b.deg ? a : b;
  const Top& lo = a.deg >= b.deg ? b : a;
  const bool hi_is_a = a.deg >= b.deg;
  const int64_t shift = hi.deg - lo.deg;
  Top r;
  r.deg = hi.deg;
  for (int i = 0; i < kTop; ++i) {
    const Fr h = hi.c[i];
    const Fr l = i >= shift ? lo.c[i - shift] : fe_zero<FrCfg>();
    const Fr x = hi_is_a ? h : l, y = hi_is_a ? l : h;  // x from a, y from b
    r.c[i] = sub ? fe_sub(x, y) : fe_add(x, y);
  }
  return r;
}
PLK_HD Top fe_add(const Top& a, const Top& b) { return top_axpy(a, b, false); }
PLK_HD Top fe_sub(const Top& a, const Top& b) { return top_axpy(a, b, true); }
PLK_HD Top fe_dbl(const Top& a) {
  Top r = a;
  for (int i = 0; i < kTop; ++i) r.c[i] = fe_dbl(a.c[i]);
  return r;
}
PLK_HD Top fe_neg(const Top& a) {
  Top r = a;
  for (int i = 0; i < kTop; ++i) r.c[i] = fe_neg(a.c[i]);
  return r;
}
PLK_HD Top fe_mul(const Top& a, const Fr& k) {
  Top r = a;
  for (int i = 0; i < kTop; ++i) r.c[i] = fe_mul(a.c[i], k);
  return r;
}
PLK_HD Top fe_mul(const Fr& k, const Top& a) { return fe_mul(a, k); }
// X^(Da + Db - k) collects a[i] b[k - i]
PLK_HD Top fe_mul(const Top& a, const Top& b) {
  Top r;
  r.deg = a.deg + b.deg;
  for (int k = 0; k < kTop; ++k) {
    Fr s = fe_zero<FrCfg>();
    for (int i = 0; i <= k; ++i) s = fe_add(s, fe_mul(a.c[i], b.c[k - i]));
    r.c[k] = s;
  }
  return r;
}
PLK_HD Top fe_sqr(const Top& a) { return fe_mul(a, a); }

// p(w X): coefficient k times w^k (w_inv = 1 / w)
PLK_HD Top top_rotate(const Top& p, const Fr& w, const Fr& w_inv) {
  Top r = p;
  Fr s = fe_pow_u64(w, p.deg < 0 ? 0 : (uint64_t)p.deg);
  for (int i = 0; i < kTop; ++i) {
    r.c[i] = fe_mul(p.c[i], s);
    s = fe_mul(s, w_inv);
  }
  return r;
}

// X
PLK_HD Top top_x() {
  Top r(fe_one<FrCfg>());
  r.deg = 1;
  return r;
}

// PI(X) = sum_i pi_i L_i(X) with L_i(X) = n^-1 sum_k (w^-i X)^k: the coefficient of X^(n - 1 - t)
// is n^-1 sum_i pi_i (w^i)^(t + 1). w_i[i] = w^index_i.
PLK_HD Top top_public_inputs(const Fr* pi, const Fr* w_i, size_t npi, const Fr& n_inv, uint64_t n) {
  Top r;
  r.deg = (int64_t)n - 1;
  for (size_t i = 0; i < npi; ++i) {
    Fr p = fe_mul(pi[i], n_inv);
    for (int t = 0; t < kTop; ++t) {
      p = fe_mul(p, w_i[i]);
      r.c[t] = fe_add(r.c[t], p);
    }
  }
  return r;
}

// What round 3 knows of the factor polynomials, each as seven coefficients in ascending order:
// the blinded wires' n-5 .. n+1, z's n-4 .. n+2, the selectors' (SEL_* order), the sigmas' and
// L1's n-7 .. n-1.
struct QuotientTopIn {
  Fr wire[4][kTop], z[kTop], sel[SEL_COUNTQ][kTop], sigma[4][kTop], l1[kTop];
};

// q[j] = N[5n + j] = t[4n + j], j < kTop, for the numerator N of protocol.hpp quotient_numerator:
// the same text on Top. pi: PI's top (top_public_inputs, or Top() without public inputs);
// ch: beta, gamma, alpha and the separation challenges; flags as quotient_numerator's.
PLK_HD void quotient_top(const QuotientTopIn& in, const Top& pi, uint64_t n, const Fr& omega,
                         const Fr& omega_inv, const Fr* ch, unsigned flags, Fr* q) {
  const int64_t N = (int64_t)n;
  Top w[4], wn[4], sel[SEL_COUNTQ], sigma[4];
  for (int c = 0; c < 4; ++c) {
    w[c] = top_from_coeffs(in.wire[c], N + 1);
    wn[c] = top_rotate(w[c], omega, omega_inv);
    sigma[c] = top_from_coeffs(in.sigma[c], N - 1);
  }
  for (int s = 0; s < SEL_COUNTQ; ++s) sel[s] = top_from_coeffs(in.sel[s], N - 1);
  const Top z = top_from_coeffs(in.z, N + 2), zn = top_rotate(z, omega, omega_inv);
  const Top l1 = top_from_coeffs(in.l1, N - 1);
  const Top num = quotient_numerator(w, wn, z, zn, sel, sigma, l1, pi, top_x(), ch, edwards_d(), flags);
  for (int j = 0; j < kTop; ++j) q[j] = top_coeff(num, 5 * N + j);
}

// t from four blocks (prover.hpp): with c_m = s_m^n and P(Y) = prod_{m<4} (Y - c_m) =
// sum_l p_l Y^l (p_4 = 1), t = T_4 + Q(X) P(X^n): v[l][j] is what t[l n + j] gains, l < 4, and
// what t[4n + j] is, l = 4; v[l][7] = 0.
constexpr int kTopBlocks = 4;
struct QuotientPatch {
  Fr v[kTopBlocks + 1][kTop + 1];
};
PLK_HD void quotient_patch(const Fr* q, const Fr* p, QuotientPatch& o) {
  for (int l = 0; l <= kTopBlocks; ++l) {
    for (int j = 0; j < kTop; ++j) o.v[l][j] = fe_mul(p[l], q[j]);
    o.v[l][kTop] = fe_zero<FrCfg>();
  }
}

}  // namespace plk
