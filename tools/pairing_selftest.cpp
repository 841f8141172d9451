// pairing_selftest.cpp — the host pairing (csrc/pairing.hpp, csrc/pairing_host.hpp) as a
// stand-alone program, for a sanitizer run of the G2 preparation and the pairing check on the
// CPU. No GPU, no HIP:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/pairing_selftest.cpp -o pairing_selftest && ./pairing_selftest
//
// Checks e(tau s G, H) == e(s G, [tau]H) (accept), the two reject cases (tau s G + G, s G) and
// (tau s G, -s G), the infinity rules, and that [r]H is the identity. `--dump` also prints
// e(G, H)^3 as 72 hex words (Montgomery limbs, plk_debug_pairing's layout).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../dusk-plonk_amd/csrc/g1.hpp"
#include "../dusk-plonk_amd/csrc/pairing_host.hpp"

using namespace plk;

static G1In g1_gen() {
  // the G1 generator, plain integers (little-endian 32-bit words)
  static const uint32_t gx[12] = {0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu,
                                  0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u};
  static const uint32_t gy[12] = {0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu,
                                  0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u};
  return {fe_to_mont(fp_from_words(gx)), fe_to_mont(fp_from_words(gy)), false};
}

static G1In g1_mul(const G1In& p, const uint32_t* e, int words) {
  G1xyzz acc = xyzz_infinity();
  for (int w = words - 1; w >= 0; --w)
    for (int b = 31; b >= 0; --b) {
      acc = xyzz_dbl(acc);
      if (!p.inf && ((e[w] >> b) & 1u)) acc = xyzz_add_affine(acc, p.x, p.y);
    }
  G1In r;
  r.inf = !xyzz_to_affine(acc, r.x, r.y);
  return r;
}

static G1In g1_add(const G1In& a, const G1In& b) {
  if (a.inf) return b;
  if (b.inf) return a;
  G1In r;
  r.inf = !xyzz_to_affine(xyzz_add_affine(xyzz_from_affine({a.x, a.y}), b.x, b.y), r.x, r.y);
  return r;
}

static int failures = 0;
static void expect(bool cond, const char* what) {
  printf("%-44s %s\n", what, cond ? "ok" : "FAILED");
  if (!cond) ++failures;
}

int main(int argc, char** argv) {
  const uint32_t tau[8] = {0x9e3779b9u, 0x7f4a7c15u, 0xbf58476du, 0x1ce4e5b9u, 0x94d049bbu, 0x133111ebu, 0x12345678u, 0x0badc0deu};
  const uint32_t s[8] = {0xdeadbeefu, 0x01234567u, 0x89abcdefu, 0x0f1e2d3cu, 0x4b5a6978u, 0x8796a5b4u, 0xc3d2e1f0u, 0x01020304u};
  Fp2 frob[12];
  frob_table(frob);
  const G2Aff h = g2_generator();
  expect(g2_on_curve(h), "H on the twist");
  expect(g2_in_subgroup(h), "[r]H is the identity");
  const G2Aff bh = g2_mul(h, tau, 8);
  std::vector<Fp2> lh(2 * kMillerLines), lb(2 * kMillerLines);
  expect(g2_prepare(h, lh.data()), "prepare H");
  expect(g2_prepare(bh, lb.data()), "prepare [tau]H");
  expect(!g2_prepare(g2_infinity(), lb.data() /* untouched */), "infinity has no table");
  expect(g2_prepare(bh, lb.data()), "prepare [tau]H again");

  const G1In g = g1_gen();
  const G1In w = g1_mul(g, s, 8);
  const G1In c = g1_mul(w, tau, 8);
  G1In wn = w;
  wn.y = fe_neg(w.y);
  const G1In inf = {fe_zero<FpCfg>(), fe_zero<FpCfg>(), true};
  expect(pairing_check_host(lh.data(), lb.data(), frob, c, w), "accepts (tau s G, s G)");
  expect(!pairing_check_host(lh.data(), lb.data(), frob, g1_add(c, g), w), "rejects (tau s G + G, s G)");
  expect(!pairing_check_host(lh.data(), lb.data(), frob, c, wn), "rejects (tau s G, -s G)");
  expect(pairing_check_host(lh.data(), lb.data(), frob, inf, inf), "accepts (inf, inf)");
  expect(!pairing_check_host(lh.data(), lb.data(), frob, g, inf), "rejects (G, inf)");
  expect(!pairing_check_host(lh.data(), lb.data(), frob, inf, g), "rejects (inf, G)");
  if (argc > 1 && !strcmp(argv[1], "--dump")) {
    uint64_t out[72];
    pairing_value_host(lh.data(), frob, g, out);
    for (int i = 0; i < 72; ++i) printf("%016llx\n", (unsigned long long)out[i]);
  }
  printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
