// composer.hip — the composer (restating the reference's Plonk<C>, src/lib.rs):
// the compact gate records, the structure hash, the gadgets and every plk_composer_* entry point.
// Host code only.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "composer.hpp"
#include "protocol.hpp"

using namespace plk;

namespace {

bool fr_eq(const Fr& a, const Fr& b) { return fe_eq(a, b); }

enum { QM = SEL_QM, QL = SEL_QL, QR = SEL_QR, QO = SEL_QO, Q4 = SEL_Q4, QC = SEL_QC,
       QARITH = SEL_QARITH, QRANGE = SEL_QRANGE };  // the selector rows (protocol.hpp), short

Gate default_gate() {
  Gate g;
  for (auto& q : g.q) q = fe_zero<FrCfg>();
  for (auto& w : g.w) w = 0;  // Plonk::ZERO
  g.has_pi = false;
  g.pi = fe_zero<FrCfg>();
  return g;
}

uint32_t append_witness(plk_composer* c, const Fr& v) {
  c->witness.push_back(v);
  c->wire_head.push_back(plk_composer::kNoWire);
  c->wire_tail.push_back(plk_composer::kNoWire);
  return (uint32_t)(c->witness.size() - 1);
}

// Montgomery images of the selector codes kSelZero / kSelOne / kSelMinusOne
struct SelConsts {
  Fr v[3];
  SelConsts() {
    v[0] = fe_zero<FrCfg>();
    v[1] = fe_one<FrCfg>();
    v[2] = fe_neg(v[1]);
  }
};
const SelConsts& sel_consts() {
  static const SelConsts k;
  return k;
}

}  // namespace

namespace plk {
GateRec gate_pack(plk_composer* c, const Gate& g) {
  const SelConsts& k = sel_consts();
  GateRec r;
  std::memcpy(r.w, g.w, sizeof r.w);
  r.code = 0;
  r.ext = (uint32_t)c->consts.size();
  for (int q = 0; q < 11; ++q) {
    uint32_t code = kSelPooled;
    for (uint32_t j = 0; j < 3; ++j)
      if (fe_eq(g.q[q], k.v[j])) {
        code = j;
        break;
      }
    if (code == kSelPooled) c->consts.push_back(g.q[q]);
    r.code |= code << (2 * q);
  }
  if (g.has_pi) {
    r.code |= kPiBit;
    c->consts.push_back(g.pi);
  }
  return r;
}

Gate gate_unpack(const plk_composer* c, size_t i) {
  const SelConsts& k = sel_consts();
  const GateRec& r = c->gates[i];
  Gate g;
  std::memcpy(g.w, r.w, sizeof g.w);
  uint32_t e = r.ext;
  for (int q = 0; q < 11; ++q) {
    const uint32_t code = sel_code(r.code, q);
    g.q[q] = code == kSelPooled ? c->consts[e++] : k.v[code];
  }
  g.has_pi = (r.code & kPiBit) != 0;
  g.pi = g.has_pi ? c->consts[e] : fe_zero<FrCfg>();
  return g;
}
}  // namespace plk

namespace {

inline uint64_t hash_mix(uint64_t h, uint64_t v) {
  h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
  return h * 0xff51afd7ed558ccdull;
}

int push_gate(plk_composer* c, const GateRec& g) {
  for (int k = 0; k < 4; ++k)
    if (g.w[k] >= c->witness.size()) return PLK_E_ARG;  // permutation.rs:98 assert
  const uint32_t n = (uint32_t)c->gates.size();
  c->gates.push_back(g);
  {  // structure hash: wires, selector codes (incl. the PI bit) and pooled selector values
    uint64_t h = hash_mix(c->struct_hash, (uint64_t)g.w[0] | ((uint64_t)g.w[1] << 32));
    h = hash_mix(h, (uint64_t)g.w[2] | ((uint64_t)g.w[3] << 32));
    h = hash_mix(h, g.code);
    uint32_t e = g.ext;
    for (int q = 0; q < 11; ++q)
      if (sel_code(g.code, q) == kSelPooled) {
        const Fr& v = c->consts[e++];
        for (int i = 0; i < 8; i += 2) h = hash_mix(h, (uint64_t)v.v[i] | ((uint64_t)v.v[i + 1] << 32));
      }
    c->struct_hash = h;
  }
  for (int k = 0; k < 4; ++k) {  // add_witnesses_to_map (permutation.rs:72-91)
    const uint32_t wire = 4 * n + k, wit = g.w[k];
    c->wire_next.push_back(plk_composer::kNoWire);
    if (c->wire_tail[wit] == plk_composer::kNoWire)
      c->wire_head[wit] = wire;
    else
      c->wire_next[c->wire_tail[wit]] = wire;
    c->wire_tail[wit] = wire;
  }
  return PLK_OK;
}

int append_custom_gate(plk_composer* c, const Gate& g) {
  for (int k = 0; k < 4; ++k)
    if (g.w[k] >= c->witness.size()) return PLK_E_ARG;
  return push_gate(c, gate_pack(c, g));
}

int append_gate(plk_composer* c, Gate g) {  // Constraint::arithmetic
  g.q[QARITH] = fe_one<FrCfg>();
  return append_custom_gate(c, g);
}

// append_evaluated_output (lib.rs:555-600): o = -(q_m a b + q_l a + q_r b + q_4 d + q_c + PI) / q_o
bool evaluated_output(plk_composer* c, const Gate& s, uint32_t& out) {
  const Fr a = c->witness[s.w[0]], b = c->witness[s.w[1]], d = c->witness[s.w[3]];
  Fr x = fe_mul(fe_mul(s.q[QM], a), b);
  x = fe_add(x, fe_mul(s.q[QL], a));
  x = fe_add(x, fe_mul(s.q[QR], b));
  x = fe_add(x, fe_mul(s.q[Q4], d));
  x = fe_add(x, s.q[QC]);
  if (s.has_pi) x = fe_add(x, s.pi);
  const Fr y = s.q[QO];
  if (fe_is_zero(y)) return false;
  Fr o;
  if (fr_eq(y, fe_one<FrCfg>()))
    o = fe_neg(x);
  else if (fr_eq(y, fe_neg(fe_one<FrCfg>())))
    o = x;
  else
    o = fe_mul(x, fe_neg(fe_inv(y)));
  out = append_witness(c, o);
  return true;
}

void assert_equal_constant(plk_composer* c, uint32_t a, const Fr& constant, const Fr* pi) {
  Gate g = default_gate();
  g.q[QL] = fe_one<FrCfg>();
  g.q[QC] = fe_neg(constant);
  g.w[0] = a;
  if (pi) {
    g.has_pi = true;
    g.pi = *pi;
  }
  (void)append_gate(c, g);
}

// lib.rs:606-640
void append_dummy_gates(plk_composer* c) {
  const uint32_t six = append_witness(c, fr_u64(6));
  const uint32_t one = append_witness(c, fr_u64(1));
  const uint32_t seven = append_witness(c, fr_u64(7));
  const uint32_t min_twenty = append_witness(c, fe_neg(fr_u64(20)));
  Gate g = default_gate();
  g.q[QM] = fr_u64(1);
  g.q[QL] = fr_u64(2);
  g.q[QR] = fr_u64(3);
  g.q[Q4] = fr_u64(1);
  g.q[QC] = fr_u64(4);
  g.q[QO] = fr_u64(4);
  g.w[0] = six;
  g.w[1] = seven;
  g.w[3] = one;
  g.w[2] = min_twenty;
  (void)append_gate(c, g);
  Gate h = default_gate();
  h.q[QM] = fr_u64(1);
  h.q[QL] = fr_u64(1);
  h.q[QR] = fr_u64(1);
  h.q[QC] = fr_u64(127);
  h.q[QO] = fr_u64(1);
  h.w[0] = min_twenty;
  h.w[1] = six;
  h.w[2] = seven;
  (void)append_gate(c, h);
}

Gate gate_from(const plk_constraint* s) {
  Gate g = default_gate();
  const plk_fr* qs[11] = {&s->q_m, &s->q_l, &s->q_r, &s->q_o, &s->q_4, &s->q_c, &s->q_arith,
                          &s->q_range, &s->q_logic, &s->q_fixed_group_add, &s->q_variable_group_add};
  for (int i = 0; i < 11; ++i) g.q[i] = fr_from_abi(*qs[i]);
  g.w[0] = s->a;
  g.w[1] = s->b;
  g.w[2] = s->o;
  g.w[3] = s->d;
  g.has_pi = s->has_public != 0;
  g.pi = fr_from_abi(s->public_input);
  return g;
}

}  // namespace

extern "C" {

// Composer storage pool: a proof server synthesizes a fresh composer per proof (as
// create_proof does, prover.rs:76-78); reusing the vectors of destroyed composers (clear()
// keeps capacity) avoids re-faulting ~120 bytes of fresh pages per gate every proof.
namespace {
std::mutex g_pool_mu;
std::vector<std::unique_ptr<plk_composer>> g_pool;
constexpr size_t kPoolMax = 2;

std::unique_ptr<plk_composer> composer_from_pool() {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (!g_pool.empty()) {
      std::unique_ptr<plk_composer> c = std::move(g_pool.back());
      g_pool.pop_back();
      return c;
    }
  }
  return std::unique_ptr<plk_composer>(new plk_composer());
}
}  // namespace

int plk_composer_create(plk_composer** out) {
  try {
    if (!out) return PLK_E_ARG;
    std::unique_ptr<plk_composer> c = composer_from_pool();
    // Plonk::initialize (lib.rs:121-134)
    const uint32_t zero = append_witness(c.get(), fe_zero<FrCfg>());
    const uint32_t one = append_witness(c.get(), fe_one<FrCfg>());
    assert_equal_constant(c.get(), zero, fe_zero<FrCfg>(), nullptr);
    assert_equal_constant(c.get(), one, fe_one<FrCfg>(), nullptr);
    append_dummy_gates(c.get());
    append_dummy_gates(c.get());
    *out = c.release();
    return PLK_OK;
  } catch (...) {
    return PLK_E_OOM;
  }
}

int plk_composer_destroy(plk_composer* c) {
  if (!c) return PLK_OK;
  std::unique_ptr<plk_composer> h(c);
  h->witness.clear();
  h->gates.clear();
  h->consts.clear();
  h->wire_head.clear();
  h->wire_tail.clear();
  h->wire_next.clear();
  h->struct_hash = plk_composer::kHashInit;
  std::lock_guard<std::mutex> lk(g_pool_mu);
  if (g_pool.size() < kPoolMax) g_pool.push_back(std::move(h));
  return PLK_OK;
}

int plk_composer_size(const plk_composer* c, size_t* gates, size_t* witnesses) {
  if (!c) return PLK_E_ARG;
  if (gates) *gates = c->gates.size();
  if (witnesses) *witnesses = c->witness.size();
  return PLK_OK;
}

int plk_composer_append_witness(plk_composer* c, const plk_fr* v, uint32_t* wire) {
  if (!c || !v || !wire) return PLK_E_ARG;
  *wire = append_witness(c, fr_from_abi(*v));
  return PLK_OK;
}

int plk_composer_witness_value(const plk_composer* c, uint32_t wire, plk_fr* v) {
  if (!c || !v || wire >= c->witness.size()) return PLK_E_ARG;
  *v = fr_to_abi(c->witness[wire]);
  return PLK_OK;
}

// lib.rs:708-719: witness + assert_equal_constant(w, 0, Some(-public))
int plk_composer_append_public(plk_composer* c, const plk_fr* v, uint32_t* wire) {
  if (!c || !v || !wire) return PLK_E_ARG;
  const Fr val = fr_from_abi(*v);
  *wire = append_witness(c, val);
  const Fr neg = fe_neg(val);
  assert_equal_constant(c, *wire, fe_zero<FrCfg>(), &neg);
  return PLK_OK;
}

int plk_composer_append_gate(plk_composer* c, const plk_constraint* s) {
  if (!c || !s) return PLK_E_ARG;
  return append_gate(c, gate_from(s));
}

int plk_composer_append_custom_gate(plk_composer* c, const plk_constraint* s) {
  if (!c || !s) return PLK_E_ARG;
  return append_custom_gate(c, gate_from(s));
}

// lib.rs:1169-1197: q_o = -1, o := evaluated output, append
int plk_composer_gate_eval(plk_composer* c, const plk_constraint* s, uint32_t* out) {
  if (!c || !s || !out) return PLK_E_ARG;
  Gate g = gate_from(s);
  g.q[QARITH] = fe_one<FrCfg>();
  g.q[QO] = fe_neg(fe_one<FrCfg>());
  for (int k = 0; k < 4; ++k)
    if (g.w[k] >= c->witness.size() && k != 2) return PLK_E_ARG;
  uint32_t o;
  if (!evaluated_output(c, g, o)) return PLK_E_ARG;
  g.w[2] = o;
  *out = o;
  return append_gate(c, g);
}

int plk_composer_assert_equal(plk_composer* c, uint32_t a, uint32_t b) {
  if (!c || a >= c->witness.size() || b >= c->witness.size()) return PLK_E_ARG;
  Gate g = default_gate();  // lib.rs:721-730
  g.q[QL] = fe_one<FrCfg>();
  g.q[QR] = fe_neg(fe_one<FrCfg>());
  g.w[0] = a;
  g.w[1] = b;
  return append_gate(c, g);
}

int plk_composer_assert_equal_constant(plk_composer* c, uint32_t a, const plk_fr* constant,
                                       const plk_fr* public_input) {
  if (!c || !constant || a >= c->witness.size()) return PLK_E_ARG;
  const Fr pi = public_input ? fr_from_abi(*public_input) : fe_zero<FrCfg>();
  assert_equal_constant(c, a, fr_from_abi(*constant), public_input ? &pi : nullptr);
  return PLK_OK;
}

// component_range (lib.rs:1066-1163): base-4 accumulators over the witness's canonical bits
// (LSB first), 4 quads per width-4 gate with q_range = 1 (d, o, b, a order within a gate,
// the next gate's d closing the chain), a final zero-selector gate carrying the last
// accumulator, and the last accumulator asserted equal to the witness.
int plk_composer_component_range(plk_composer* c, uint32_t witness, size_t num_bits) {
  if (!c || witness >= c->witness.size() || num_bits > 256) return PLK_E_ARG;
  try {
    const Fr canon = fe_from_mont(c->witness[witness]);
    auto bit = [&](size_t i) -> uint32_t { return (canon.v[i / 32] >> (i % 32)) & 1u; };
    size_t num_gates = num_bits >> 3;
    if (num_bits % 8 != 0) ++num_gates;
    const size_t num_quads = num_gates * 4;
    const size_t pad = 1 + (((num_quads << 1) - num_bits) >> 1);
    Gate base = default_gate();
    base.q[QRANGE] = fe_one<FrCfg>();  // Constraint::range
    std::vector<Gate> cons(num_gates + 1, base);
    std::vector<uint32_t> accs;
    const Fr four = fr_u64(4);
    Fr acc = fe_zero<FrCfg>();
    for (size_t i = pad; i <= num_quads; ++i) {
      const size_t bi = (num_quads - i) << 1;
      const uint32_t quad = (bi < 256 ? bit(bi) : 0u) + 2 * (bi + 1 < 256 ? bit(bi + 1) : 0u);
      acc = fe_add(fe_mul(four, acc), fr_u64(quad));
      const uint32_t w = append_witness(c, acc);
      accs.push_back(w);
      Gate& g = cons[i / 4];
      switch (i % 4) {
        case 0: g.w[3] = w; break;
        case 1: g.w[2] = w; break;
        case 2: g.w[1] = w; break;
        default: g.w[0] = w; break;
      }
    }
    cons.back() = default_gate();
    if (!accs.empty()) cons.back().w[3] = accs.back();
    for (const Gate& g : cons)
      if (append_custom_gate(c, g) != PLK_OK) return PLK_E_ARG;
    if (!accs.empty()) return plk_composer_assert_equal(c, accs.back(), witness);
    return PLK_OK;
  } catch (...) {
    return PLK_E_OOM;
  }
}

int plk_composer_component_boolean(plk_composer* c, uint32_t a) {
  if (!c || a >= c->witness.size()) return PLK_E_ARG;
  Gate g = default_gate();  // lib.rs:859-872
  g.q[QM] = fe_one<FrCfg>();
  g.q[QO] = fe_neg(fe_one<FrCfg>());
  g.w[0] = a;
  g.w[1] = a;
  g.w[2] = a;
  g.w[3] = 0;
  return append_gate(c, g);
}

// The bench circuit: `gates` arithmetic gates of the chain
// x_{i+1} = x_i * y_i + x_i via gate_mul-style gates (q_m = 1, q_l = 1, q_o = -1) whose
// outputs feed the next gate's a-wire (non-trivial copy constraints); y_i from SplitMix64.
int plk_composer_synthetic_chain(plk_composer* c, size_t gates, uint64_t seed) {
  if (!c) return PLK_E_ARG;
  try {
    Rng rng{seed};
    uint32_t x = append_witness(c, rng.fr_mont());
    c->witness.reserve(c->witness.size() + 2 * gates);
    c->wire_head.reserve(c->wire_head.size() + 2 * gates);
    c->wire_tail.reserve(c->wire_tail.size() + 2 * gates);
    c->wire_next.reserve(c->wire_next.size() + 4 * gates);
    c->gates.reserve(c->gates.size() + gates);
    GateRec g;
    g.code = (kSelOne << (2 * QM)) | (kSelOne << (2 * QL)) | (kSelMinusOne << (2 * QO)) |
             (kSelOne << (2 * QARITH));
    g.ext = (uint32_t)c->consts.size();
    g.w[3] = 0;  // Plonk::ZERO
    for (size_t i = 0; i < gates; ++i) {
      const uint32_t y = append_witness(c, rng.fr_mont());
      const Fr& xv = c->witness[x];
      const Fr o = fe_add(fe_mul(xv, c->witness[y]), xv);
      g.w[0] = x;
      g.w[1] = y;
      g.w[2] = append_witness(c, o);
      if (push_gate(c, g) != PLK_OK) return PLK_E_ARG;
      x = g.w[2];
    }
    return PLK_OK;
  } catch (...) {
    return PLK_E_OOM;
  }
}

// Overwrite witness values (a new instance of the same circuit, as create_proof
// re-synthesizes the circuit with new witnesses, prover.rs:76-78).
int plk_composer_set_witness(plk_composer* c, uint32_t wire, const plk_fr* v) {
  if (!c || !v || wire >= c->witness.size()) return PLK_E_ARG;
  c->witness[wire] = fr_from_abi(*v);
  return PLK_OK;
}

// public inputs, sorted by gate index (Plonk::instance, lib.rs:182-196)
int plk_composer_public_inputs(const plk_composer* c, plk_fr* values, uint64_t* indexes,
                               size_t cap, size_t* count) {
  if (!c || !count) return PLK_E_ARG;
  size_t k = 0;
  for (size_t i = 0; i < c->gates.size(); ++i) {
    if (!(c->gates[i].code & kPiBit)) continue;
    if (k < cap) {
      if (values) values[k] = fr_to_abi(gate_unpack(c, i).pi);
      if (indexes) indexes[k] = i;
    }
    ++k;
  }
  *count = k;
  return PLK_OK;
}

int plk_composer_export(const plk_composer* c, plk_constraint* gates, size_t cap,
                        plk_fr* witness, size_t wcap, size_t* m, size_t* nw) {
  if (!c) return PLK_E_ARG;
  if (m) *m = c->gates.size();
  if (nw) *nw = c->witness.size();
  if (gates) {
    const size_t cnt = std::min(cap, c->gates.size());
    for (size_t i = 0; i < cnt; ++i) {
      const Gate g = gate_unpack(c, i);
      plk_constraint& o = gates[i];
      plk_fr* qs[11] = {&o.q_m,     &o.q_l,   &o.q_r,     &o.q_o,
                        &o.q_4,     &o.q_c,   &o.q_arith, &o.q_range,
                        &o.q_logic, &o.q_fixed_group_add, &o.q_variable_group_add};
      for (int q = 0; q < 11; ++q) *qs[q] = fr_to_abi(g.q[q]);
      o.a = g.w[0];
      o.b = g.w[1];
      o.o = g.w[2];
      o.d = g.w[3];
      o.has_public = g.has_pi ? 1u : 0u;
      o._pad = 0;
      o.public_input = fr_to_abi(g.pi);
    }
  }
  if (witness) {
    const size_t cnt = std::min(wcap, c->witness.size());
    for (size_t j = 0; j < cnt; ++j) witness[j] = fr_to_abi(c->witness[j]);
  }
  return PLK_OK;
}

}  // extern "C"
