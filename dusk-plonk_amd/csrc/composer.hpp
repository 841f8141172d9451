// composer.hpp — the composer object behind the plk_composer_* entry points of include/plk.h
// (composer.hip, host only) and the gate records that key.hip, prover.hip and circuit_check.hip
// read from it.
#pragma once
#include <vector>

#include "internal.hpp"

namespace plk {

PLK_LOCAL inline Fr fr_u64(uint64_t v) {
  Fr x = fe_zero<FrCfg>();
  x.v[0] = (uint32_t)v;
  x.v[1] = (uint32_t)(v >> 32);
  return fe_to_mont(x);
}

// SplitMix64 -> uniform Fr (4 words, top masked to 255 bits, rejection), Montgomery out.
// The prover's randomness (blinding scalars) comes from an explicit seed so the CPU and
// GPU paths can consume identical randomness (SURVEY §7 hard part 5).
struct PLK_LOCAL Rng {
  uint64_t s;
  uint64_t next() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  // 255 random bits below r, as they come (rejection)
  Fr below_r() {
    for (;;) {
      const uint64_t w[4] = {next(), next(), next(), next()};
      Fr c = fe_of_abi<FrCfg>(w);
      c.v[7] &= 0x7fffffffu;
      if (fe_canonical(c)) return c;
    }
  }
  Fr fr() { return fe_to_mont(below_r()); }
  // uniform Fr drawn directly as its Montgomery image (x -> xR is a bijection of Fr), so no
  // multiply: used for the synthetic circuit's witnesses
  Fr fr_mont() { return below_r(); }
};

// One width-4 gate: q_m a b + q_l a + q_r b + q_o o + q_4 d + q_c + PI = 0 (lib.rs:546)
struct Gate {
  Fr q[11];  // q_m q_l q_r q_o q_4 q_c q_arith q_range q_logic q_fixed_group_add q_variable_group_add
  uint32_t w[4];  // a, b, o, d witness indices
  bool has_pi;
  Fr pi;
};

// The composer stores a gate as 24 bytes instead of Gate's 416: the four wires, a 2-bit
// code per selector (kSelZero / kSelOne / kSelMinusOne / kSelPooled) with bit kPiBit set
// when the gate carries a public input, and `ext`, the index in plk_composer::consts of
// the gate's pooled selectors (in selector order) followed by its PI value. Circuits are
// dominated by 0/±1 selectors, so synthesis writes ~17x fewer bytes per gate.
enum : uint32_t { kSelZero = 0, kSelOne = 1, kSelMinusOne = 2, kSelPooled = 3 };
constexpr uint32_t kPiBit = 1u << 22;
struct GateRec {
  uint32_t w[4];
  uint32_t code;
  uint32_t ext;
};
PLK_HD uint32_t sel_code(uint32_t code, int q) { return (code >> (2 * q)) & 3u; }

}  // namespace plk

struct plk_composer {
  std::vector<plk::Fr> witness;
  std::vector<plk::GateRec> gates;
  std::vector<plk::Fr> consts;  // pooled selector / PI values (see GateRec)
  // witness -> its wires in insertion order (permutation.rs:21-25,72-104), wire = 4*gate+col,
  // as flat singly linked lists (no per-witness allocation): head/tail per witness, next
  // per wire; kNoWire terminates.
  static constexpr uint32_t kNoWire = 0xffffffffu;
  std::vector<uint32_t> wire_head, wire_tail, wire_next;
  // running hash of the circuit's structure (every gate's wires, selector codes, pooled
  // selector values and public-input position — not witness or public-input values),
  // updated as gates are appended: plk_prove compares it with the key's in O(1)
  static constexpr uint64_t kHashInit = 0x6a09e667f3bcc908ull;
  uint64_t struct_hash = kHashInit;
};

namespace plk {
// Gate <-> GateRec (composer.hip): packing appends the gate's pooled values to c->consts
PLK_LOCAL GateRec gate_pack(plk_composer* c, const Gate& g);
PLK_LOCAL Gate gate_unpack(const plk_composer* c, size_t i);
}  // namespace plk
