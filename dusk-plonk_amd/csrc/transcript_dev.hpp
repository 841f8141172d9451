// transcript_dev.hpp — a merlin transcript with a fixed schedule, for host and device.
//
// Every proof of one verifier walks the same transcript: the labels, the lengths, the order of
// the operations and so the sponge position at every byte are the same, only the values differ.
// ReplaySchedule replays the STROBE-128 / merlin framing of transcript.hpp ONCE on the host,
// with placeholders for the values, and compiles it into a list of 166-byte rate blocks. A block
// is what one Keccak-f[1600] call absorbs:
//   - per 32-bit word of the rate (42 words, 168 bytes: the rate and the two bytes of padding
//     behind it) a constant to XOR — operation headers, labels, length prefixes, the run_f
//     padding — and up to two value parts: a row of the per-proof value stream, a byte shift
//     and a byte mask (a word holds bytes of at most two values: any two are separated by
//     at least one operation header and a label);
//   - whether a PRF output (challenge_bytes) is taken after the permutation, and which. Every
//     challenge_bytes begins with a forced permutation (or lands on one), so a PRF always reads
//     the state from byte 0.
// sched_absorb / keccak_f1600 run a block for one proof with the 25 lanes of the state in
// statically indexed registers: no byte-addressed state, no scratch memory. The value stream is
// a table of 32-bit rows [row][proof]; row r holds the stream bytes 4 (r - 1) .. 4 (r - 1) + 3,
// row 0 and the row behind the last one are padding the masks never let through.
#pragma once
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "abi.hpp"

namespace plk {

constexpr int kRateWords = 42;                       // 166 bytes of rate + 2 of padding
constexpr int kBlockWords = 2 + 6 * kRateWords;      // take, take_len, then 6 words per rate word
constexpr uint32_t kNoTake = 0xffffffffu;

struct KeccakState {
  uint64_t s[25];
};

struct KeccakCfg {
  static constexpr uint64_t RC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull,
      0x000000000000808Bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
      0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
      0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull,
      0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
};

PLK_HD uint64_t rol64(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }

// Keccak-f[1600] on s[x + 5 y], every index a constant
PLK_HD void keccak_f1600(uint64_t (&s)[25]) {
#pragma unroll
  for (int r = 0; r < 24; ++r) {
    uint64_t c[5];
#pragma unroll
    for (int x = 0; x < 5; ++x) c[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];
#pragma unroll
    for (int x = 0; x < 5; ++x) {
      const uint64_t d = c[(x + 4) % 5] ^ rol64(c[(x + 1) % 5], 1);
#pragma unroll
      for (int y = 0; y < 25; y += 5) s[y + x] ^= d;
    }
    // rho and pi along the single cycle of the lane permutation
    uint64_t t = s[1], b;
#define PLK_RP(j, n) \
  b = s[j];          \
  s[j] = rol64(t, n); \
  t = b;
    PLK_RP(10, 1) PLK_RP(7, 3) PLK_RP(11, 6) PLK_RP(17, 10) PLK_RP(18, 15) PLK_RP(3, 21)
    PLK_RP(5, 28) PLK_RP(16, 36) PLK_RP(8, 45) PLK_RP(21, 55) PLK_RP(24, 2) PLK_RP(4, 14)
    PLK_RP(15, 27) PLK_RP(23, 41) PLK_RP(19, 56) PLK_RP(13, 8) PLK_RP(12, 25) PLK_RP(2, 43)
    PLK_RP(20, 62) PLK_RP(14, 18) PLK_RP(22, 39) PLK_RP(9, 61) PLK_RP(6, 20) PLK_RP(1, 44)
#undef PLK_RP
#pragma unroll
    for (int y = 0; y < 25; y += 5) {
#pragma unroll
      for (int x = 0; x < 5; ++x) c[x] = s[y + x];
#pragma unroll
      for (int x = 0; x < 5; ++x) s[y + x] = c[x] ^ (~c[(x + 1) % 5] & c[(x + 2) % 5]);
    }
    s[0] ^= KeccakCfg::RC[r];
  }
}

// XOR one compiled block into the rate. blk: the block's kBlockWords words; load(row): the
// proof's value stream row.
template <class Load>
PLK_HD void sched_absorb(uint64_t (&s)[25], const uint32_t* blk, Load load) {
#pragma unroll
  for (int d = 0; d < kRateWords; ++d) {
    const uint32_t* w = blk + 2 + 6 * d;
    uint32_t x = w[0];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const uint32_t mask = w[2 + 2 * e];
      if (mask) {  // the same for every proof
        const uint32_t row = w[1 + 2 * e], sh = (w[5] >> (8 * e)) & 0xffu;
        const uint64_t two = (uint64_t)load(row) | ((uint64_t)load(row + 1) << 32);
        x ^= (uint32_t)(two >> sh) & mask;
      }
    }
    s[d / 2] ^= (uint64_t)x << (32 * (d & 1));
  }
}

// Fr::from_bytes_wide of the first 64 bytes of the state (Montgomery form out), which the
// PRF then clears. (lo + hi 2^256) mod r as lo R^2 / R + hi R^3 / R.
PLK_HD Fr sched_take_scalar(uint64_t (&s)[25]) {
  Fr lo, hi, r2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lo.v[2 * i] = (uint32_t)s[i];
    lo.v[2 * i + 1] = (uint32_t)(s[i] >> 32);
    hi.v[2 * i] = (uint32_t)s[4 + i];
    hi.v[2 * i + 1] = (uint32_t)(s[4 + i] >> 32);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s[i] = 0;
    r2.v[i] = FrCfg::R2[i];
  }
  // the spare-bit Montgomery multiply needs canonical inputs: 2^256 < 3 r
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    fe_reduce_once(lo);
    fe_reduce_once(hi);
  }
  const Fr r3 = fe_mul(r2, r2);
  return fe_add(fe_mul(lo, r2), fe_mul(hi, r3));
}

// The first 16 bytes of the state as a 128-bit little-endian value (Montgomery form out)
PLK_HD Fr sched_take_u128(uint64_t (&s)[25]) {
  Fr r = fe_zero<FrCfg>();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    r.v[2 * i] = (uint32_t)s[i];
    r.v[2 * i + 1] = (uint32_t)(s[i] >> 32);
    s[i] = 0;
  }
  return fe_to_mont(r);
}

// The host's recording STROBE: Strobe128 / Transcript of transcript.hpp with positions only.
class ReplaySchedule {
 public:
  // continue from a transcript whose sponge stands at (pos, pos_begin)
  ReplaySchedule(uint8_t pos, uint8_t pos_begin) : pos_(pos), pos_begin_(pos_begin) { fresh(); }

  // Transcript::append_message of n value bytes at byte `stream` of the value stream
  void append_value(const char* label, uint32_t stream, uint32_t n) {
    frame(label, n);
    begin_op(kA);
    for (uint32_t i = 0; i < n; ++i) value_byte(stream + i);
  }
  // Transcript::challenge_bytes of n < 166 bytes, reported as take `id`
  void challenge(const char* label, uint32_t n, uint32_t id) {
    frame(label, n);
    begin_op(kI | kA | kC);
    if (pos_ != 0 || blocks_ == 0 || n >= kR) throw std::logic_error("replay schedule: prf");
    uint32_t* last = words_.data() + (size_t)(blocks_ - 1) * kBlockWords;
    if (last[0] != kNoTake) throw std::logic_error("replay schedule: two takes in a block");
    last[0] = id;
    last[1] = n;
    pos_ = (uint8_t)n;  // the PRF cleared and passed bytes 0 .. n - 1
  }
  // the compiled blocks; what stands in the open block behind the last take is never run
  const std::vector<uint32_t>& words() const { return words_; }
  uint32_t blocks() const { return blocks_; }

 private:
  static constexpr uint8_t kI = 1, kA = 2, kC = 4, kM = 16, kK = 32;
  static constexpr uint8_t kR = 166;
  uint8_t pos_, pos_begin_;
  uint8_t k_[4 * kRateWords];
  uint32_t cur_[kBlockWords];
  std::vector<uint32_t> words_;
  uint32_t blocks_ = 0;

  void fresh() {
    for (uint8_t& b : k_) b = 0;
    for (uint32_t& w : cur_) w = 0;
    cur_[0] = kNoTake;
  }
  void run_f() {
    k_[pos_] ^= pos_begin_;
    k_[pos_ + 1] ^= 0x04;
    k_[kR + 1] ^= 0x80;
    for (int d = 0; d < kRateWords; ++d)
      cur_[2 + 6 * d] = (uint32_t)k_[4 * d] | ((uint32_t)k_[4 * d + 1] << 8) |
                        ((uint32_t)k_[4 * d + 2] << 16) | ((uint32_t)k_[4 * d + 3] << 24);
    words_.insert(words_.end(), cur_, cur_ + kBlockWords);
    ++blocks_;
    fresh();
    pos_ = 0;
    pos_begin_ = 0;
  }
  void const_byte(uint8_t b) {
    k_[pos_] ^= b;
    if (++pos_ == kR) run_f();
  }
  void value_byte(uint32_t stream) {
    const uint32_t d = pos_ / 4u, b = pos_ % 4u;
    // the word's byte 0 would be stream byte s0 (as low as -3): row = floor(s0 / 4) + 1
    const int64_t s0 = (int64_t)stream - b;
    const uint32_t row = (uint32_t)((s0 + 4) / 4), sh = 8u * (uint32_t)((s0 + 4) % 4);
    uint32_t* w = cur_ + 2 + 6 * d;
    int e = 0;
    for (; e < 2; ++e) {
      const bool same = w[2 + 2 * e] && w[1 + 2 * e] == row && ((w[5] >> (8 * e)) & 0xffu) == sh;
      if (same || !w[2 + 2 * e]) break;
    }
    if (e == 2) throw std::logic_error("replay schedule: three values in a word");
    w[1 + 2 * e] = row;
    w[2 + 2 * e] |= 0xffu << (8 * b);
    w[5] = (w[5] & ~(0xffu << (8 * e))) | (sh << (8 * e));
    if (++pos_ == kR) run_f();
  }
  void begin_op(uint8_t flags) {
    const uint8_t old_begin = pos_begin_;
    pos_begin_ = pos_ + 1;
    const_byte(old_begin);
    const_byte(flags);
    if ((flags & (kC | kK)) && pos_ != 0) run_f();
  }
  // meta_ad(label) and meta_ad(le32(n), more)
  void frame(const char* label, uint32_t n) {
    begin_op(kM | kA);
    for (const char* c = label; *c; ++c) const_byte((uint8_t)*c);
    for (int i = 0; i < 4; ++i) const_byte((uint8_t)(n >> (8 * i)));
  }
};

}  // namespace plk
