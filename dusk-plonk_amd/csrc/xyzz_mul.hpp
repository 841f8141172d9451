// xyzz_mul.hpp — windowed scalar multiplication on packed XYZZ points, shared by the transforms
// over G1 (lagrange.hip, g1_ntt.hip). Exact for every point of the curve (no endomorphism), with
// every exceptional case of the group law handled by xyzz_add / xyzz_dbl.
#pragma once
#include <hip/hip_runtime.h>

#include "g1.hpp"

namespace plk {

__device__ __forceinline__ G1xyzz xyzz_sel(bool c, const G1xyzz& a, const G1xyzz& b) {
  G1xyzz r;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    r.X.v[i] = c ? a.X.v[i] : b.X.v[i];
    r.Y.v[i] = c ? a.Y.v[i] : b.Y.v[i];
    r.ZZ.v[i] = c ? a.ZZ.v[i] : b.ZZ.v[i];
    r.ZZZ.v[i] = c ? a.ZZZ.v[i] : b.ZZZ.v[i];
  }
  return r;
}

// s P for a canonical (non-Montgomery) scalar s < 2^255: 2-bit windows from the top set pair
__device__ __forceinline__ G1xyzz xyzz_mul(const G1xyzz& p, const Fr& s) {
  int top = -1;  // highest nonzero 2-bit digit
#pragma unroll
  for (int k = 7; k >= 0; --k)
    if (top < 0 && s.v[k]) top = 16 * k + ((31 - __clz(s.v[k])) >> 1);
  G1xyzz acc = xyzz_infinity();
  if (top < 0 || xyzz_is_inf(p)) return acc;
  const G1xyzz p2 = xyzz_dbl(p), p3 = xyzz_add(p2, p);
  for (int i = top; i >= 0; --i) {
    acc = xyzz_dbl(xyzz_dbl(acc));
    // word (i >> 4) by a select tree: a run-time index would put the scalar in scratch memory
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) w = (i >> 4) == k ? s.v[k] : w;
    const uint32_t d = (w >> (2 * (i & 15))) & 3u;
    if (d) acc = xyzz_add(acc, xyzz_sel(d == 1, p, xyzz_sel(d == 2, p2, p3)));
  }
  return acc;
}

}  // namespace plk
