// circuit_check.hpp — the per-gate check behind plk_composer_check / plk_prover_diagnose
// (include/plk.h): every summand of the quotient's numerator (tests/prover_stage_ref.quotient)
// evaluated on its own at one gate, from the composer's compact gate records. One definition:
// k_gate_check (circuit_check.hip) and the host mirror both call gate_check_at.
#pragma once
#include "prover.hpp"

namespace plk {

struct GateVerdict {
  uint32_t mask;  // PLK_GATE_* bits of the non-zero terms
  Fr residual;    // the arithmetic term's value (R domain)
};

// failing gates of a class: any bit of the class's mask (summary order: arith range logic fixed var)
constexpr uint32_t kClassMask[5] = {0x1u, 0xfu << 4, 0x1fu << 8, 0xfu << 16, 0x7u << 20};

// 32 bytes as two 16-byte loads on the device (the gathers bind the kernel, not the products)
PLK_HD Fr ld_fr(const Fr* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  Fr r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  return r;
#else
  return *p;
#endif
}

// delta(f) = f (f - 1)(f - 2)(f - 3) != 0
PLK_HD bool delta_nonzero(const Fr& f) {
  const Fr one = fe_one<FrCfg>();
  const Fr f1 = fe_sub(f, one), f2 = fe_sub(f1, one), f3 = fe_sub(f2, one);
  // a product in a field vanishes exactly when a factor does
  return !(fe_is_zero(f) || fe_is_zero(f1) || fe_is_zero(f2) || fe_is_zero(f3));
}

// The gate's 11 selectors q (SEL_* order), its own wire values a b c (= o) d, the next row's
// an bn cn dn and its public input pi (0 without one). cn enters no identity; it is taken so
// that the call names the whole next row.
PLK_HD GateVerdict gate_check(const Fr* q, const Fr& a, const Fr& b, const Fr& c, const Fr& d,
                              const Fr& an, const Fr& bn, const Fr& cn, const Fr& dn,
                              const Fr& pi) {
  (void)cn;
  GateVerdict v;
  v.mask = 0;
  {  // q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c) + PI
    v.residual = fe_add(widget_arith(q, a, b, c, d), pi);
    if (!fe_is_zero(v.residual)) v.mask |= PLK_GATE_ARITH;
  }
  if (!fe_is_zero(q[SEL_QRANGE])) {
    if (delta_nonzero(fe_sub(c, fe_quad(d)))) v.mask |= PLK_GATE_RANGE(0);
    if (delta_nonzero(fe_sub(b, fe_quad(c)))) v.mask |= PLK_GATE_RANGE(1);
    if (delta_nonzero(fe_sub(a, fe_quad(b)))) v.mask |= PLK_GATE_RANGE(2);
    if (delta_nonzero(fe_sub(dn, fe_quad(a)))) v.mask |= PLK_GATE_RANGE(3);
  }
  if (!fe_is_zero(q[SEL_QLOGIC])) {
    const Fr qa = fe_sub(an, fe_quad(a)), qb = fe_sub(bn, fe_quad(b)), qd = fe_sub(dn, fe_quad(d));
    if (delta_nonzero(qa)) v.mask |= PLK_GATE_LOGIC(0);
    if (delta_nonzero(qb)) v.mask |= PLK_GATE_LOGIC(1);
    if (delta_nonzero(qd)) v.mask |= PLK_GATE_LOGIC(2);
    if (!fe_eq(c, fe_mul(qa, qb))) v.mask |= PLK_GATE_LOGIC(3);
    if (!fe_is_zero(logic_xor_and(qa, qb, c, qd, q[SEL_QC]))) v.mask |= PLK_GATE_LOGIC(4);
  }
  if (!fe_is_zero(q[SEL_QFIXED])) {
    // (a, b) the point accumulator, d the scalar accumulator, c = xy_alpha,
    // (q_l, q_r, q_c) = (x_beta, y_beta, x_beta y_beta) of the gate's multiple
    const Fr one = fe_one<FrCfg>();
    const Fr bit = fe_sub(dn, fe_dbl(d));
    if (!(fe_is_zero(bit) || fe_eq(bit, one) || fe_is_zero(fe_add(bit, one))))
      v.mask |= PLK_GATE_FIXED(0);
    if (!fe_eq(fe_mul(bit, q[SEL_QC]), c)) v.mask |= PLK_GATE_FIXED(1);
    const Fr y_alpha = fe_add(fe_mul(fe_sqr(bit), fe_sub(q[SEL_QR], one)), one);
    const Fr x_alpha = fe_mul(q[SEL_QL], bit);
    const Fr prod = fe_mul(fe_mul(fe_mul(c, a), b), edwards_d());
    const Fr x_lhs = fe_add(an, fe_mul(an, prod));
    const Fr x_rhs = fe_add(fe_mul(a, y_alpha), fe_mul(b, x_alpha));
    if (!fe_eq(x_lhs, x_rhs)) v.mask |= PLK_GATE_FIXED(2);
    const Fr y_lhs = fe_sub(bn, fe_mul(bn, prod));
    const Fr y_rhs = fe_add(fe_mul(b, y_alpha), fe_mul(a, x_alpha));
    if (!fe_eq(y_lhs, y_rhs)) v.mask |= PLK_GATE_FIXED(3);
  }
  if (!fe_is_zero(q[SEL_QVAR])) {
    // gate (x1, y1, x2, y2) = (a, b, c, d), next row (x3, y3, ., x1 y2)
    if (!fe_eq(fe_mul(a, d), dn)) v.mask |= PLK_GATE_VAR(0);
    const Fr y1x2 = fe_mul(b, c);
    const Fr dprod = fe_mul(fe_mul(edwards_d(), dn), y1x2);
    if (!fe_eq(fe_add(dn, y1x2), fe_add(an, fe_mul(an, dprod)))) v.mask |= PLK_GATE_VAR(1);
    if (!fe_eq(fe_add(fe_mul(b, d), fe_mul(a, c)), fe_sub(bn, fe_mul(bn, dprod))))
      v.mask |= PLK_GATE_VAR(2);
  }
  return v;
}

// Gate i of a table of m compact records: the selectors decoded (0, 1, -1 without a load,
// pooled ones from consts[ext + k]), the gate's wires and the next row's gathered from the
// witness array (the row after the last gate is the zero row, as k_gather_wires pads it), then
// gate_check. pi_vals null: the public input is the value pooled after the gate's selectors
// (a composer's table). pi_vals set: that slot holds, in its first word, the gate's ordinal
// among the circuit's public inputs, and the value is pi_vals[ordinal] (a key's table: the
// values belong to the proof, not to the key).
PLK_HD GateVerdict gate_check_at(const GateRec* gates, const Fr* consts, const Fr* witness,
                                 const Fr* pi_vals, uint64_t m, uint64_t i) {
  const GateRec r = gates[i];
  const Fr zero = fe_zero<FrCfg>(), one = fe_one<FrCfg>(), minus_one = fe_neg(one);
  Fr q[SEL_COUNTQ];
  uint32_t e = r.ext;
#pragma unroll
  for (int k = 0; k < SEL_COUNTQ; ++k) {
    const uint32_t code = sel_code(r.code, k);
    if (code == kSelPooled)
      q[k] = ld_fr(&consts[e++]);
    else
      q[k] = code == kSelOne ? one : code == kSelMinusOne ? minus_one : zero;
  }
  Fr pi = zero;
  if (r.code & kPiBit) {
    pi = ld_fr(&consts[e]);
    if (pi_vals) pi = ld_fr(&pi_vals[pi.v[0]]);
  }
  const Fr a = ld_fr(&witness[r.w[0]]), b = ld_fr(&witness[r.w[1]]);
  const Fr c = ld_fr(&witness[r.w[2]]), d = ld_fr(&witness[r.w[3]]);
  Fr an = zero, bn = zero, cn = zero, dn = zero;
  if (i + 1 < m) {
    const GateRec& nx = gates[i + 1];
    an = ld_fr(&witness[nx.w[0]]);
    bn = ld_fr(&witness[nx.w[1]]);
    cn = ld_fr(&witness[nx.w[2]]);
    dn = ld_fr(&witness[nx.w[3]]);
  }
  return gate_check(q, a, b, c, d, an, bn, cn, dn, pi);
}

// ---- the device check (circuit_check.hip) --------------------------------------------
// What k_gate_check reduces on the device. first_inv holds ~gate of the smallest failing gate
// (largest wins), so that a zeroed record means no failing gate.
struct CheckCounters {
  unsigned long long failing, by_class[5], first_inv;
};

// One checker's buffers and events (a context's, for plk_composer_check, or a prover's): the
// gate table and witness are passed in, so a prover checks what it already holds.
// summary / failures / cap / count: the contract of include/plk.h. Waits for the stream.
int check_run(CheckWs*& ws, plk_ctx* ctx, hipStream_t s, const GateRec* d_gates, const Fr* d_consts,
              const Fr* d_witness, const Fr* d_pi_vals, uint64_t m, plk_check_summary* summary,
              plk_gate_failure* failures, size_t cap, size_t* count);

}  // namespace plk
