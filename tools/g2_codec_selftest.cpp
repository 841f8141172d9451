// g2_codec_selftest.cpp — the opening key's byte codec and the Fp2 square root
// (csrc/pairing_host.hpp g2_from_bytes, g2_to_bytes, f2_sqrt) as a stand-alone program, for a
// sanitizer run on the CPU. No GPU, no HIP:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/g2_codec_selftest.cpp -o g2_codec_selftest && ./g2_codec_selftest
//
// Round trips H, [tau]H and -[tau]H through both forms, squares and re-roots a chain of Fp2
// values (real, imaginary and mixed), and walks the strict rejections: flag bits, a coefficient
// >= p, an x without a root, a y off the twist, bytes under the infinity bit. Buffers are
// heap-allocated at their exact sizes so that a read or write past 96 / 192 bytes is caught.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../dusk-plonk_amd/csrc/g1.hpp"
#include "../dusk-plonk_amd/csrc/pairing_host.hpp"

using namespace plk;

static int failures = 0;
static void expect(bool cond, const char* what) {
  printf("%-52s %s\n", what, cond ? "ok" : "FAILED");
  if (!cond) ++failures;
}

static bool g2_same(const G2Aff& a, const G2Aff& b) {
  if (a.inf || b.inf) return a.inf == b.inf;
  return f2_eq(a.x, b.x) && f2_eq(a.y, b.y);
}

static bool round_trip(const G2Aff& q, bool compressed) {
  std::vector<uint8_t> buf(compressed ? 96 : 192);
  g2_to_bytes(q, compressed, buf.data());
  G2Aff back;
  if (g2_from_bytes(buf.data(), compressed, back) != PLK_OK) return false;
  std::vector<uint8_t> again(buf.size());
  g2_to_bytes(back, compressed, again.data());
  return g2_same(q, back) && buf == again;
}

static bool refused(const std::vector<uint8_t>& buf, bool compressed) {
  G2Aff o;
  return g2_from_bytes(buf.data(), compressed, o) == PLK_E_ARG;
}

int main() {
  const uint32_t tau[8] = {0x9e3779b9u, 0x7f4a7c15u, 0xbf58476du, 0x1ce4e5b9u, 0x94d049bbu, 0x133111ebu, 0x12345678u, 0x0badc0deu};
  const G2Aff h = g2_generator();
  const G2Aff bh = g2_mul(h, tau, 8);
  G2Aff nbh = bh;
  nbh.y = f2_neg(bh.y);
  for (int c = 0; c < 2; ++c) {
    expect(round_trip(h, c != 0), c ? "H, compressed" : "H, uncompressed");
    expect(round_trip(bh, c != 0), c ? "[tau]H, compressed" : "[tau]H, uncompressed");
    expect(round_trip(nbh, c != 0), c ? "-[tau]H, compressed" : "-[tau]H, uncompressed");
    expect(round_trip(g2_infinity(), c != 0), c ? "infinity, compressed" : "infinity, uncompressed");
  }
  expect(g2_y_is_larger(bh.y) != g2_y_is_larger(nbh.y), "one of +-y is the larger");

  // square roots: a chain of values, their squares re-rooted up to sign
  bool roots_ok = true, none_ok = true;
  int non_squares = 0;
  Fp2 v = bh.x;
  const Fp three = fe_add(fe_dbl(fe_one<FpCfg>()), fe_one<FpCfg>());
  for (int i = 0; i < 24; ++i) {
    Fp2 s = v;
    if (i % 6 == 4) s.c1 = fe_zero<FpCfg>();  // real
    if (i % 6 == 5) s.c0 = fe_zero<FpCfg>();  // imaginary
    const Fp2 sq = f2_sqr(s);
    Fp2 r;
    roots_ok = roots_ok && f2_sqrt(sq, r) && (f2_eq(r, s) || f2_eq(r, f2_neg(s)));
    if (!f2_sqrt(v, r)) {  // about half of the chain: no root, and the output is zero
      ++non_squares;
      none_ok = none_ok && f2_is_zero(r);
    } else {
      none_ok = none_ok && f2_eq(f2_sqr(r), v);
    }
    v = f2_add(f2_mul(v, bh.y), {three, fe_one<FpCfg>()});
  }
  Fp2 r;
  roots_ok = roots_ok && f2_sqrt(f2_zero(), r) && f2_is_zero(r);
  roots_ok = roots_ok && f2_sqrt(f2_neg(f2_one()), r) && f2_eq(f2_sqr(r), f2_neg(f2_one()));  // -1 = u^2
  expect(roots_ok, "sqrt(s^2) = +-s, sqrt(0), sqrt(-1)");
  expect(none_ok && non_squares > 0, "non-squares give no root");

  // strict rejections
  std::vector<uint8_t> c(96), u(192);
  g2_to_bytes(bh, true, c.data());
  g2_to_bytes(bh, false, u.data());
  auto with0 = [](std::vector<uint8_t> b, uint8_t v0) {
    b[0] = v0;
    return b;
  };
  expect(refused(with0(c, c[0] & 0x7f), true), "compressed: bit 7 clear");
  expect(refused(with0(c, c[0] | 0x40), true), "compressed: infinity bit on a point");
  expect(refused(with0(u, u[0] | 0x80), false), "uncompressed: bit 7 set");
  expect(refused(with0(u, u[0] | 0x20), false), "uncompressed: sort bit set");
  std::vector<uint8_t> inf_c(96, 0), inf_u(192, 0);
  inf_c[0] = 0xc0;
  inf_u[0] = 0x40;
  inf_c[95] = 1;
  inf_u[191] = 1;
  expect(refused(inf_c, true) && refused(inf_u, false), "a byte under the infinity bit");
  std::vector<uint8_t> big = c;  // x.c0 = 2^384 - 1 >= p
  memset(big.data() + 48, 0xff, 48);
  expect(refused(big, true), "x.c0 >= p");
  big = c;
  memset(big.data() + 1, 0xff, 47);
  big[0] |= 0x1f;  // x.c1 = 2^381 - 1 >= p
  expect(refused(big, true), "x.c1 >= p");
  big = u;
  memset(big.data() + 144, 0xff, 48);
  expect(refused(big, false), "y.c0 >= p");
  std::vector<uint8_t> off = u;
  off[191] ^= 1;
  expect(refused(off, false), "y off the twist");
  // an x without a root: walk x.c0 until the decoder refuses (about every second x)
  std::vector<uint8_t> walk = c;
  bool met = false;
  for (int i = 0; i < 64 && !met; ++i) {
    walk[95] = (uint8_t)(c[95] + i);
    met = refused(walk, true);
  }
  expect(met, "an x with no point on the twist");
  printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
