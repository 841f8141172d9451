// protocol.hpp — the PLONK protocol, stated once for the prover (key.hip, prover.hip, prover_kernels.hip),
// the verifier (verifier.hip) and the device replay (verifier_replay.hip): the names of a proof's
// evaluations, challenges and commitments, the shared constants, the widgets, the scalars of the
// linearisation polynomial r, the values at z that enter the transcript, and the order in which
// everything enters it. A change to a widget, a challenge or the transcript is made here.
//
// PLK_HD code on the packed field of ff.hpp, like abi.hpp: no HIP calls, no allocation, and plain
// g++ compiles it. Every value is a canonical field element in Montgomery form.
#pragma once
#include <stddef.h>

#include "abi.hpp"

namespace plk {

// ---- names ------------------------------------------------------------------------------------
// the 16 evaluations, in plk_proof order
enum Eval { EV_A = 0, EV_B, EV_C, EV_D, EV_A_NEXT, EV_B_NEXT, EV_D_NEXT, EV_Q_ARITH, EV_Q_C, EV_Q_L,
            EV_Q_R, EV_S1, EV_S2, EV_S3, EV_R, EV_PERM, EV_COUNT };
// the 11 challenges, in the order they are drawn
enum Chal { CH_BETA = 0, CH_GAMMA, CH_ALPHA, CH_RANGE, CH_LOGIC, CH_FIXED, CH_VAR, CH_Z, CH_VA,
            CH_VB, CH_U, CH_COUNT };
// the proof's 11 commitments, in plk_proof order
enum ProofComm { PC_A = 0, PC_B, PC_C, PC_D, PC_Z, PC_T_LOW, PC_T_MID, PC_T_HIGH, PC_T_4, PC_W_Z,
                 PC_W_ZW, PC_COUNT };
// the key's 15 commitments, in the order the base transcript absorbs them (key.rs:138-159)
enum KeyComm { KC_QM = 0, KC_QL, KC_QR, KC_QO, KC_QC, KC_Q4, KC_QARITH, KC_QRANGE, KC_QLOGIC,
               KC_QFIXED, KC_QVAR, KC_S1, KC_S2, KC_S3, KC_S4, KC_COUNT };
// the selector rows of the prover's tables and of a gate (zksnarks::Constraint order)
enum { SEL_QM = 0, SEL_QL, SEL_QR, SEL_QO, SEL_Q4, SEL_QC, SEL_QARITH, SEL_QRANGE, SEL_QLOGIC,
       SEL_QFIXED, SEL_QVAR, SEL_COUNTQ };
// kKeyCommSel[KC_*] = the selector row behind that commitment: the two orders differ in q_4 / q_c
constexpr int kKeyCommSel[SEL_COUNTQ] = {SEL_QM, SEL_QL, SEL_QR, SEL_QO, SEL_QC, SEL_Q4, SEL_QARITH,
                                         SEL_QRANGE, SEL_QLOGIC, SEL_QFIXED, SEL_QVAR};
static_assert(kKeyCommSel[KC_QC] == SEL_QC && kKeyCommSel[KC_Q4] == SEL_Q4 && KC_QC == SEL_Q4 &&
                  KC_Q4 == SEL_QC && kKeyCommSel[KC_QVAR] == SEL_QVAR,
              "key commitments: selector order with q_4 and q_c swapped");
constexpr const char* kKeyCommLabel[KC_COUNT] = {
    "q_m", "q_l", "q_r", "q_o", "q_c", "q_4", "q_arith", "q_range", "q_logic", "q_fixed_group_add",
    "q_variable_group_add", "s_sigma_1", "s_sigma_2", "s_sigma_3", "s_sigma_4"};

#define PLK_AT(field, first, idx, T) \
  static_assert(offsetof(plk_proof, field) == offsetof(plk_proof, first) + (idx) * sizeof(T), #field)
PLK_AT(a_eval, a_eval, EV_A, plk_fr);
PLK_AT(b_eval, a_eval, EV_B, plk_fr);
PLK_AT(c_eval, a_eval, EV_C, plk_fr);
PLK_AT(d_eval, a_eval, EV_D, plk_fr);
PLK_AT(a_next_eval, a_eval, EV_A_NEXT, plk_fr);
PLK_AT(b_next_eval, a_eval, EV_B_NEXT, plk_fr);
PLK_AT(d_next_eval, a_eval, EV_D_NEXT, plk_fr);
PLK_AT(q_arith_eval, a_eval, EV_Q_ARITH, plk_fr);
PLK_AT(q_c_eval, a_eval, EV_Q_C, plk_fr);
PLK_AT(q_l_eval, a_eval, EV_Q_L, plk_fr);
PLK_AT(q_r_eval, a_eval, EV_Q_R, plk_fr);
PLK_AT(s_sigma_1_eval, a_eval, EV_S1, plk_fr);
PLK_AT(s_sigma_2_eval, a_eval, EV_S2, plk_fr);
PLK_AT(s_sigma_3_eval, a_eval, EV_S3, plk_fr);
PLK_AT(r_poly_eval, a_eval, EV_R, plk_fr);
PLK_AT(perm_eval, a_eval, EV_PERM, plk_fr);
PLK_AT(a_comm, a_comm, PC_A, plk_g1);
PLK_AT(b_comm, a_comm, PC_B, plk_g1);
PLK_AT(c_comm, a_comm, PC_C, plk_g1);
PLK_AT(d_comm, a_comm, PC_D, plk_g1);
PLK_AT(z_comm, a_comm, PC_Z, plk_g1);
PLK_AT(t_low_comm, a_comm, PC_T_LOW, plk_g1);
PLK_AT(t_mid_comm, a_comm, PC_T_MID, plk_g1);
PLK_AT(t_high_comm, a_comm, PC_T_HIGH, plk_g1);
PLK_AT(t_4_comm, a_comm, PC_T_4, plk_g1);
PLK_AT(w_z_chall_comm, a_comm, PC_W_Z, plk_g1);
PLK_AT(w_z_chall_w_comm, a_comm, PC_W_ZW, plk_g1);
#undef PLK_AT
static_assert(sizeof(plk_proof) == PC_COUNT * sizeof(plk_g1) + EV_COUNT * sizeof(plk_fr), "plk_proof");

// ---- the transcript after Transcript::base (transcript.hpp), step by step -----------------------
// (prover.rs:99-452, proof.rs:88-384). The verifier's two replays walk the whole table; the prover
// makes its commitment and challenge calls where its rounds are and walks the evaluations.
enum StepKind : uint8_t {
  STEP_PI,      // every public input
  STEP_COMM,    // the proof's commitment `id` (ProofComm)
  STEP_CHAL,    // challenge `id` (Chal) is drawn
  STEP_BETA,    // beta, absorbed back
  STEP_EVAL,    // evaluation `id` (Eval)
  STEP_T_EVAL,  // t(z), which the verifier computes (proof_at_z)
};
struct Step {
  StepKind kind;
  uint8_t id;
  const char* label;
};
constexpr Step kScript[] = {
    {STEP_PI, 0, "pi"},
    {STEP_COMM, PC_A, "a_w"},
    {STEP_COMM, PC_B, "b_w"},
    {STEP_COMM, PC_C, "c_w"},
    {STEP_COMM, PC_D, "d_w"},
    {STEP_CHAL, CH_BETA, "beta"},
    {STEP_BETA, 0, "beta"},
    {STEP_CHAL, CH_GAMMA, "gamma"},
    {STEP_COMM, PC_Z, "z"},
    {STEP_CHAL, CH_ALPHA, "alpha"},
    {STEP_CHAL, CH_RANGE, "range separation challenge"},
    {STEP_CHAL, CH_LOGIC, "logic separation challenge"},
    {STEP_CHAL, CH_FIXED, "fixed base separation challenge"},
    {STEP_CHAL, CH_VAR, "variable base separation challenge"},
    {STEP_COMM, PC_T_LOW, "t_low"},
    {STEP_COMM, PC_T_MID, "t_mid"},
    {STEP_COMM, PC_T_HIGH, "t_high"},
    {STEP_COMM, PC_T_4, "t_4"},
    {STEP_CHAL, CH_Z, "z_challenge"},
    {STEP_EVAL, EV_A, "a_eval"},
    {STEP_EVAL, EV_B, "b_eval"},
    {STEP_EVAL, EV_C, "c_eval"},
    {STEP_EVAL, EV_D, "d_eval"},
    {STEP_EVAL, EV_A_NEXT, "a_next_eval"},
    {STEP_EVAL, EV_B_NEXT, "b_next_eval"},
    {STEP_EVAL, EV_D_NEXT, "d_next_eval"},
    {STEP_EVAL, EV_S1, "s_sigma_1_eval"},
    {STEP_EVAL, EV_S2, "s_sigma_2_eval"},
    {STEP_EVAL, EV_S3, "s_sigma_3_eval"},
    {STEP_EVAL, EV_Q_ARITH, "q_arith_eval"},
    {STEP_EVAL, EV_Q_C, "q_c_eval"},
    {STEP_EVAL, EV_Q_L, "q_l_eval"},
    {STEP_EVAL, EV_Q_R, "q_r_eval"},
    {STEP_EVAL, EV_PERM, "perm_eval"},
    {STEP_T_EVAL, 0, "t_eval"},
    {STEP_EVAL, EV_R, "r_eval"},
    {STEP_CHAL, CH_VA, "v_challenge"},
    {STEP_CHAL, CH_VB, "v_challenge"},
    {STEP_COMM, PC_W_Z, "w_z"},
    {STEP_COMM, PC_W_ZW, "w_z_w"},
    {STEP_CHAL, CH_U, "batch"},
};

// ---- constants and small helpers ----------------------------------------------------------------
PLK_HD Fr fr_small(uint32_t k) {
  Fr r = fe_zero<FrCfg>();
  r.v[0] = k;
  return fe_to_mont(r);
}

// JubJub's twisted-Edwards d = -10240 / 10241 mod r
PLK_HD Fr edwards_d() {
  Fr x;
  x.v[0] = 0xd6343eb1u; x.v[1] = 0x01065fd6u; x.v[2] = 0x37579d26u; x.v[3] = 0x292d7f6du;
  x.v[4] = 0xe6bd7fd4u; x.v[5] = 0xf5fd9207u; x.v[6] = 0x4bfa2b48u; x.v[7] = 0x2a9318e7u;
  return fe_to_mont(x);
}

// the coset representatives K1, K2, K3 of the wire columns b, c, d (permutation.rs:28-30)
PLK_HD Fr perm_k(int i) { return fr_small(i == 1 ? 7u : i == 2 ? 13u : 17u); }

// The widgets and the quotient numerator are templates on the scalar type T: Fr for a row's
// values (k_quotient_ext, the verifier's linearisation, the circuit check) and Top
// (quotient_top.hpp) for the top coefficients of the polynomials themselves (the prover's round
// 3). Constants (kappa powers, edwards d, small integers) stay Fr; T supplies fe_add / fe_sub /
// fe_mul / fe_sqr / fe_dbl among T and with an Fr.

// f (f - 1)(f - 2)(f - 3): zero exactly on a quad
template <class T>
PLK_HD T fr_delta(const T& f) {
  const Fr one = fe_one<FrCfg>();
  const T f1 = fe_sub(f, one), f2 = fe_sub(f1, one), f3 = fe_sub(f2, one);
  return fe_mul(fe_mul(f, f1), fe_mul(f2, f3));
}

template <class T>
PLK_HD T fe_quad(const T& x) { return fe_dbl(fe_dbl(x)); }

// A widget's terms are separated by the powers of kappa = sep^2
struct SepPowers {
  Fr k, k2, k3, k4;
};
PLK_HD SepPowers sep_powers(const Fr& sep) {
  SepPowers p;
  p.k = fe_sqr(sep);
  p.k2 = fe_sqr(p.k);
  p.k3 = fe_mul(p.k2, p.k);
  p.k4 = fe_sqr(p.k2);
  return p;
}

// ---- the widgets: a gate's row (and the next row's), then the kappa powers ----------------------
// Arithmetic: q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c), q in SEL_* order
template <class T>
PLK_HD T widget_arith(const T* q, const T& a, const T& b, const T& c, const T& d) {
  T t = fe_mul(fe_mul(q[SEL_QM], a), b);
  t = fe_add(t, fe_mul(q[SEL_QL], a));
  t = fe_add(t, fe_mul(q[SEL_QR], b));
  t = fe_add(t, fe_mul(q[SEL_QO], c));
  t = fe_add(t, fe_mul(q[SEL_Q4], d));
  t = fe_add(t, q[SEL_QC]);
  return fe_mul(q[SEL_QARITH], t);
}

// Range: D(c - 4d) + D(b - 4c) k + D(a - 4b) k^2 + D(d_next - 4a) k^3
template <class T>
PLK_HD T widget_range(const T& a, const T& b, const T& c, const T& d, const T& d_n,
                      const Fr& k, const Fr& k2, const Fr& k3) {
  T r = fr_delta(fe_sub(c, fe_quad(d)));
  r = fe_add(r, fe_mul(fr_delta(fe_sub(b, fe_quad(c))), k));
  r = fe_add(r, fe_mul(fr_delta(fe_sub(a, fe_quad(b))), k2));
  return fe_add(r, fe_mul(fr_delta(fe_sub(d_n, fe_quad(a))), k3));
}

// delta_xor_and: 3(a + b + c) - 2 f + q_c (9c - 3(a + b)) with
// f = w (w (4w - 18(a + b) + 81) + 18(a^2 + b^2) - 81(a + b) + 83) = 6 (a AND b) for quads
template <class T>
PLK_HD T logic_xor_and(const T& a, const T& b, const T& w, const T& c, const T& qc) {
  const T ab = fe_add(a, b);
  T f = fe_sub(fe_quad(w), fe_mul(fr_small(18), ab));
  f = fe_add(f, fr_small(81));
  f = fe_mul(w, f);
  f = fe_add(f, fe_mul(fr_small(18), fe_add(fe_sqr(a), fe_sqr(b))));
  f = fe_sub(f, fe_mul(fr_small(81), ab));
  f = fe_add(f, fr_small(83));
  f = fe_mul(w, f);
  const T e = fe_sub(fe_mul(fr_small(3), fe_add(ab, c)), fe_dbl(f));
  const T bb = fe_mul(qc, fe_sub(fe_mul(fr_small(9), c), fe_mul(fr_small(3), ab)));
  return fe_add(bb, e);
}

// Logic (dusk-plonk logic gate; zksnarks, un-vendored): quads qa = a_next - 4a, qb = b_next - 4b,
// qd = d_next - 4d, w = c:  D(qa) + D(qb) k + D(qd) k^2 + (w - qa qb) k^3 + xor_and k^4
template <class T>
PLK_HD T widget_logic(const T& a, const T& a_n, const T& b, const T& b_n, const T& c,
                      const T& d, const T& d_n, const T& q_c, const Fr& k, const Fr& k2,
                      const Fr& k3, const Fr& k4) {
  const T qa = fe_sub(a_n, fe_quad(a)), qb = fe_sub(b_n, fe_quad(b)), qd = fe_sub(d_n, fe_quad(d));
  T r = fr_delta(qa);
  r = fe_add(r, fe_mul(fr_delta(qb), k));
  r = fe_add(r, fe_mul(fr_delta(qd), k2));
  r = fe_add(r, fe_mul(fe_sub(c, fe_mul(qa, qb)), k3));
  return fe_add(r, fe_mul(logic_xor_and(qa, qb, c, qd, q_c), k4));
}

// Fixed-base scalar multiplication widget (dusk-plonk ecc/scalar_mul/fixed_base; zksnarks
// curve_scalar, un-vendored): accumulators (a, b) = point, d = scalar accumulator,
// c = xy_alpha, q_l / q_r / q_c = x_beta / y_beta / x_beta y_beta of the gate's multiple.
//   bit = d' - 2d;  bit (bit - 1)(bit + 1) + (bit q_c - c) k + x-check k^2 + y-check k^3
template <class T>
PLK_HD T widget_fixed_base(const T& ax, const T& ax_n, const T& ay, const T& ay_n,
                           const T& xy_alpha, const T& acc, const T& acc_n,
                           const T& x_beta, const T& y_beta, const T& xy_beta, const Fr& k,
                           const Fr& k2, const Fr& k3, const Fr& d) {
  const Fr one = fe_one<FrCfg>();
  const T bit = fe_sub(acc_n, fe_dbl(acc));
  const T bit_consistency = fe_mul(fe_mul(bit, fe_sub(bit, one)), fe_add(bit, one));
  const T y_alpha = fe_add(fe_mul(fe_sqr(bit), fe_sub(y_beta, one)), one);
  const T x_alpha = fe_mul(x_beta, bit);
  const T xy_consistency = fe_mul(fe_sub(fe_mul(bit, xy_beta), xy_alpha), k);
  const T prod = fe_mul(fe_mul(fe_mul(xy_alpha, ax), ay), d);
  const T x_lhs = fe_add(ax_n, fe_mul(ax_n, prod));
  const T x_rhs = fe_add(fe_mul(ax, y_alpha), fe_mul(ay, x_alpha));
  const T y_lhs = fe_sub(ay_n, fe_mul(ay_n, prod));
  const T y_rhs = fe_add(fe_mul(ay, y_alpha), fe_mul(ax, x_alpha));
  T id = fe_add(bit_consistency, xy_consistency);
  id = fe_add(id, fe_mul(fe_sub(x_lhs, x_rhs), k2));
  id = fe_add(id, fe_mul(fe_sub(y_lhs, y_rhs), k3));
  return id;
}

// Variable-base addition widget (dusk-plonk ecc/curve_addition; zksnarks curve_addtion):
// gate (x1, y1, x2, y2), next row (x3, y3, ., x1 y2):
//   (x1 y2 - x1y2') + (x1y2' + y1 x2 - x3 (1 + d x1y2' y1 x2)) k
//                   + (y1 y2 + x1 x2 - y3 (1 - d x1y2' y1 x2)) k^2
template <class T>
PLK_HD T widget_var_base(const T& x1, const T& x3, const T& y1, const T& y3, const T& x2,
                         const T& y2, const T& x1y2, const Fr& k, const Fr& k2, const Fr& d) {
  const T xy_consistency = fe_sub(fe_mul(x1, y2), x1y2);
  const T y1x2 = fe_mul(y1, x2);
  const T y1y2 = fe_mul(y1, y2);
  const T x1x2 = fe_mul(x1, x2);
  const T dprod = fe_mul(fe_mul(d, x1y2), y1x2);
  const T x3c = fe_sub(fe_add(x1y2, y1x2), fe_add(x3, fe_mul(x3, dprod)));
  const T y3c = fe_sub(fe_add(y1y2, x1x2), fe_sub(y3, fe_mul(y3, dprod)));
  return fe_add(fe_add(xy_consistency, fe_mul(x3c, k)), fe_mul(y3c, k2));
}

// ---- the quotient numerator N = t Z_H (quotient_poly.rs:74-114,122-262) ------------------------
// What k_quotient evaluates point by point in the redundant form, stated once on T: the row's
// wires w[4] and the next row's wn[4], z and z_next, the 11 selectors q (SEL_* order), the four
// sigmas, L1, PI and x (the point X itself). ch: alpha .. var separation are read (not z).
// flags: has_range | 2 has_logic | 4 has_fixed | 8 has_var, the widgets the key carries.
//   q_arith (...) + PI + sum_widgets sep q_w widget
//   + alpha [ z prod_c (w_c + beta K_c X + gamma) - z_next prod_c (w_c + beta sigma_c + gamma) ]
//   + alpha^2 (z - 1) L1
template <class T>
PLK_HD T quotient_numerator(const T* w, const T* wn, const T& z, const T& z_next, const T* q,
                            const T* sigma, const T& l1, const T& pi, const T& x, const Fr* ch,
                            const Fr& ed, unsigned flags) {
  const T &a = w[0], &b = w[1], &c = w[2], &d = w[3], &an = wn[0], &bn = wn[1], &dn = wn[3];
  const Fr &beta = ch[CH_BETA], &gamma = ch[CH_GAMMA], &alpha = ch[CH_ALPHA];
  T t = fe_add(widget_arith(q, a, b, c, d), pi);
  if (flags & 1u) {
    const SepPowers k = sep_powers(ch[CH_RANGE]);
    t = fe_add(t, fe_mul(fe_mul(widget_range(a, b, c, d, dn, k.k, k.k2, k.k3), q[SEL_QRANGE]),
                         ch[CH_RANGE]));
  }
  if (flags & 2u) {
    const SepPowers k = sep_powers(ch[CH_LOGIC]);
    t = fe_add(t, fe_mul(fe_mul(widget_logic(a, an, b, bn, c, d, dn, q[SEL_QC], k.k, k.k2, k.k3,
                                             k.k4), q[SEL_QLOGIC]), ch[CH_LOGIC]));
  }
  if (flags & 4u) {
    const SepPowers k = sep_powers(ch[CH_FIXED]);
    t = fe_add(t, fe_mul(fe_mul(widget_fixed_base(a, an, b, bn, c, d, dn, q[SEL_QL], q[SEL_QR],
                                                  q[SEL_QC], k.k, k.k2, k.k3, ed), q[SEL_QFIXED]),
                         ch[CH_FIXED]));
  }
  if (flags & 8u) {
    const SepPowers k = sep_powers(ch[CH_VAR]);
    t = fe_add(t, fe_mul(fe_mul(widget_var_base(a, an, b, bn, c, d, dn, k.k, k.k2, ed),
                                q[SEL_QVAR]), ch[CH_VAR]));
  }
  const T bx = fe_mul(x, beta);
  T id = fe_mul(fe_add(fe_add(a, bx), gamma), fe_add(fe_add(b, fe_mul(bx, perm_k(1))), gamma));
  id = fe_mul(id, fe_add(fe_add(c, fe_mul(bx, perm_k(2))), gamma));
  id = fe_mul(id, fe_add(fe_add(d, fe_mul(bx, perm_k(3))), gamma));
  id = fe_mul(id, z);
  T cp = fe_mul(fe_add(fe_add(a, fe_mul(sigma[0], beta)), gamma),
                fe_add(fe_add(b, fe_mul(sigma[1], beta)), gamma));
  cp = fe_mul(cp, fe_add(fe_add(c, fe_mul(sigma[2], beta)), gamma));
  cp = fe_mul(cp, fe_add(fe_add(d, fe_mul(sigma[3], beta)), gamma));
  cp = fe_mul(cp, z_next);
  t = fe_add(t, fe_mul(fe_sub(id, cp), alpha));
  return fe_add(t, fe_mul(fe_mul(fe_sub(z, fe_one<FrCfg>()), l1), fe_sqr(alpha)));
}

// ---- the linearisation polynomial r (linearization_poly.rs:22-134, proof.rs:459-527) ------------
// r(X) = sum_t s_t p_t(X) over the 11 selectors, z and sigma_4. A term is named by its key
// commitment (KC_QM .. KC_QVAR, KC_S4), or LIN_Z for z. put(term, s_t) receives the 13 scalars one
// at a time, so that a kernel need not hold them together. ev: the 16 evaluations, ch: the
// challenges (beta .. z are read), l1 = L_1(z), ed = edwards_d().
constexpr int LIN_Z = KC_COUNT;
template <class Put>
PLK_HD void linearisation_scalars(const Fr* ev, const Fr* ch, const Fr& l1, const Fr& ed, Put&& put) {
  const Fr &a = ev[EV_A], &b = ev[EV_B], &c = ev[EV_C], &d = ev[EV_D], &an = ev[EV_A_NEXT],
           &bn = ev[EV_B_NEXT], &dn = ev[EV_D_NEXT], &qar = ev[EV_Q_ARITH];
  const Fr &beta = ch[CH_BETA], &gamma = ch[CH_GAMMA], &alpha = ch[CH_ALPHA];
  // arithmetic::linearize: q_arith(z) (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c)
  put(KC_QM, fe_mul(qar, fe_mul(a, b)));
  put(KC_QL, fe_mul(qar, a));
  put(KC_QR, fe_mul(qar, b));
  put(KC_QO, fe_mul(qar, c));
  put(KC_QC, qar);
  put(KC_Q4, fe_mul(qar, d));
  put(KC_QARITH, fe_zero<FrCfg>());
  {  // range, logic, curve_scalar (fixed base) and curve_addition (variable base) ::linearize
    const SepPowers k = sep_powers(ch[CH_RANGE]);
    put(KC_QRANGE, fe_mul(widget_range(a, b, c, d, dn, k.k, k.k2, k.k3), ch[CH_RANGE]));
  }
  {
    const SepPowers k = sep_powers(ch[CH_LOGIC]);
    put(KC_QLOGIC, fe_mul(widget_logic(a, an, b, bn, c, d, dn, ev[EV_Q_C], k.k, k.k2, k.k3, k.k4),
                          ch[CH_LOGIC]));
  }
  {
    const SepPowers k = sep_powers(ch[CH_FIXED]);
    put(KC_QFIXED, fe_mul(widget_fixed_base(a, an, b, bn, c, d, dn, ev[EV_Q_L], ev[EV_Q_R],
                                            ev[EV_Q_C], k.k, k.k2, k.k3, ed),
                          ch[CH_FIXED]));
  }
  {
    const SepPowers k = sep_powers(ch[CH_VAR]);
    put(KC_QVAR, fe_mul(widget_var_base(a, an, b, bn, c, d, dn, k.k, k.k2, ed), ch[CH_VAR]));
  }
  // permutation::linearize:
  // z(X) [(a + b z + g)(b + b K1 z + g)(c + b K2 z + g)(d + b K3 z + g) alpha + L1(z) alpha^2]
  const Fr bz = fe_mul(beta, ch[CH_Z]);
  Fr x = fe_mul(fe_add(fe_add(a, bz), gamma), fe_add(fe_add(b, fe_mul(perm_k(1), bz)), gamma));
  x = fe_mul(x, fe_add(fe_add(c, fe_mul(perm_k(2), bz)), gamma));
  x = fe_mul(x, fe_add(fe_add(d, fe_mul(perm_k(3), bz)), gamma));
  x = fe_mul(x, alpha);
  put(LIN_Z, fe_add(x, fe_mul(l1, fe_sqr(alpha))));
  // -sigma_4(X) (a + b s1 + g)(b + b s2 + g)(c + b s3 + g) beta perm_eval alpha
  const Fr b0 = fe_add(fe_add(a, fe_mul(beta, ev[EV_S1])), gamma);
  const Fr b1 = fe_add(fe_add(b, fe_mul(beta, ev[EV_S2])), gamma);
  const Fr b2 = fe_add(fe_add(c, fe_mul(beta, ev[EV_S3])), gamma);
  put(KC_S4, fe_neg(fe_mul(fe_mul(fe_mul(b0, b1), fe_mul(b2, beta)), fe_mul(ev[EV_PERM], alpha))));
}

// ---- the values at z -----------------------------------------------------------------------------
// z^n, Z_H(z) / n, and the inverses of Z_H(z) and of `den` (a further denominator, or one) from
// ONE inversion shared with z - 1; L_1(z) = Z_H(z) / (n (z - 1)). False when Z_H(z) = 0 or z = 1
// (the values are then meaningless): a verifier refuses such a proof.
struct AtZ {
  Fr zn, zh_n, zh_inv, den_inv, l1;
};
PLK_HD bool at_z(const Fr& z, uint32_t log_n, const Fr& n_inv, const Fr& den, AtZ& o) {
  const Fr one = fe_one<FrCfg>();
  o.zn = z;
  for (uint32_t i = 0; i < log_n; ++i) o.zn = fe_sqr(o.zn);
  const Fr z_h = fe_sub(o.zn, one), zm1 = fe_sub(z, one);
  const Fr ab = fe_mul(z_h, zm1);
  const Fr inv = fe_inv(fe_mul(ab, den));
  o.den_inv = fe_mul(inv, ab);
  const Fr inv_den = fe_mul(inv, den);
  o.zh_inv = fe_mul(inv_den, zm1);
  o.zh_n = fe_mul(z_h, n_inv);
  o.l1 = fe_mul(o.zh_n, fe_mul(inv_den, z_h));
  return !(fe_is_zero(z_h) || fe_is_zero(zm1));
}

// What a verifier computes between the z challenge and the evaluations: z^n, L_1(z) and t(z)
// (proof.rs:386-440). PI(z) = Z_H(z) / n sum_i pi_i / (omega^-i z - 1) over the npi public inputs
// (winv[i] = omega^-index) is summed as ONE fraction: per non-zero input num = num d_i + pi_i den,
// den = den d_i, and den joins at_z's inversion; zero inputs are skipped, as in the reference
// (proof.rs:558). No allocation for any npi. Returns at_z's verdict.
PLK_HD bool proof_at_z(const Fr* ev, const Fr* ch, const Fr& z, uint32_t log_n, const Fr& n_inv,
                       const Fr* pi, const Fr* winv, uint32_t npi, Fr& zn, Fr& l1, Fr& t_eval) {
  const Fr one = fe_one<FrCfg>();
  Fr num = fe_zero<FrCfg>(), den = one;
  for (uint32_t i = 0; i < npi; ++i) {
    const Fr p = pi[i];
    if (!fe_is_zero(p)) {
      const Fr d = fe_sub(fe_mul(winv[i], z), one);
      num = fe_add(fe_mul(num, d), fe_mul(p, den));
      den = fe_mul(den, d);
    }
  }
  AtZ o;
  const bool ok = at_z(z, log_n, n_inv, den, o);
  const Fr pi_eval = fe_mul(fe_mul(num, o.den_inv), o.zh_n);
  const Fr beta = ch[CH_BETA], gamma = ch[CH_GAMMA], alpha = ch[CH_ALPHA];
  const Fr b0 = fe_add(fe_add(ev[EV_A], fe_mul(beta, ev[EV_S1])), gamma);
  const Fr b1 = fe_add(fe_add(ev[EV_B], fe_mul(beta, ev[EV_S2])), gamma);
  const Fr b2 = fe_add(fe_add(ev[EV_C], fe_mul(beta, ev[EV_S3])), gamma);
  const Fr b3 = fe_mul(fe_mul(fe_add(ev[EV_D], gamma), ev[EV_PERM]), alpha);
  const Fr b_term = fe_mul(fe_mul(b0, b1), fe_mul(b2, b3));
  const Fr c_term = fe_mul(o.l1, fe_mul(alpha, alpha));
  t_eval = fe_mul(fe_sub(fe_sub(fe_add(ev[EV_R], pi_eval), b_term), c_term), o.zh_inv);
  l1 = o.l1;
  zn = o.zn;
  return ok;
}

}  // namespace plk
