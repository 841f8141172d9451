// g1_mul.hip — batched variable-base scalar multiplication on G1, one point and one 255-bit
// scalar per lane (include/plk.h "Updating an SRS"): out[i] = [k_i] P_i.
//
// The endomorphism of the subgroup test (ingest_math.hpp g1_in_subgroup, beta from abi.hpp):
// psi(x, y) = (beta x, y) = [-z] P on G1
// with z = x0^2 = 0xac45a4010001a4020000000100000000 and r = z^2 - z + 1. For k in [0, r):
//     a = z - (k mod z)  in [1, z],    b = floor(k / z) + 1  in [1, z]   ((r - 1) / z = z - 1),
//     a - b z = -k,  so  [k] P = -(a P + b psi P) = a (-P) + b (-psi P).
// Both halves fit 128 bits and are positive, so the split is one division of k by the constant z:
// no inversion mod r, no rounding, no signs. The chain is 128 doublings with one mixed addition
// each from the table {-P, -psi P, -(P + psi P)} = {(x, -y), (beta x, -y), (beta^2 x, y)}: the
// third entry is free because 1 + psi + psi^2 = 0, i.e. P + psi P = -psi^2 P = (beta^2 x, -y).
// Forming the table costs the two products beta x, beta^2 x.
//
//  - The chain runs on the redundant-limb lazy law of g1r.hpp (g1r_dbl_lazy, g1r_madd_lazy_sl +
//    g1r_madd_lazy_fix, g1r_lazy_finish) in the R' domain; the point enters through
//    fe_to_rx_domain and the result leaves as packed canonical R-domain XYZZ for srs.hip's batch
//    inversion (srs_batch_affine).
//  - The addend is chosen with lane-wise selects between the entries held in registers, and the
//    digit's bits are shifted out of the two 128-bit halves: nothing is indexed at run time, so
//    there is no scratch object and no LDS table.
//  - Every addition is executed by the whole wave (some lane of 64 almost always has a non-zero
//    digit); a lane with the digit 0 is masked off by the branch around it.
//  - Exceptional additions: the accumulator is the identity until the first non-zero digit; on
//    G1 the only other cases are in the LAST addition: k = 0 (a = z, b = 1) ends on z P' + psi P' =
//    O, and k = 2 z (a = z, b = 3) on psi P' + psi P', a doubling. Both give ZZ3 = 0 in the
//    straight-line formula and are finished by g1r_madd_lazy_fix, as in k_accumulate.
//  - The split is only valid on G1 (off it psi is not multiplication by -z): callers check
//    membership or vouch for it.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "g1r.hpp"
#include "internal.hpp"
#include "msm_common.hpp"

using namespace plk;

namespace plk {

int srs_batch_affine(const G1xyzz* temp, uint64_t n, Fp* pref, G1Affine* out, uint8_t* out_inf,
                     hipStream_t stream);

namespace {

constexpr int kBlock = 64;  // one wave per block, as the ingest kernels
constexpr uint64_t kZLo = 0x0000000100000000ull, kZHi = 0xac45a4010001a402ull;  // z = x0^2
constexpr size_t kMaxBatch = (size_t)1 << 26;

// k: a canonical scalar in plain form (not Montgomery). a = z - (k mod z), b = floor(k / z) + 1,
// each as (lo, hi) 64-bit words. k < r < 2^255 and z > 2^127, so the top 127 bits of k are already
// a remainder below z; the other 128 bits come in by restoring division, one quotient bit each
// (no quotient-digit estimate that could be off by one). The remainder is kept in 128 bits with
// the bit shifted out of it as the 129th.
PLK_HD void glv_split(const Fr& k, uint64_t (&a)[2], uint64_t (&b)[2]) {
  uint64_t lo = (uint64_t)k.v[0] | ((uint64_t)k.v[1] << 32), hi = (uint64_t)k.v[2] | ((uint64_t)k.v[3] << 32);
  uint64_t r0 = (uint64_t)k.v[4] | ((uint64_t)k.v[5] << 32), r1 = (uint64_t)k.v[6] | ((uint64_t)k.v[7] << 32);
  uint64_t q0 = 0, q1 = 0;
  for (int i = 0; i < 128; ++i) {
    const uint64_t top = r1 >> 63;
    r1 = (r1 << 1) | (r0 >> 63);
    r0 = (r0 << 1) | (hi >> 63);
    hi = (hi << 1) | (lo >> 63);
    lo <<= 1;
    const uint64_t d0 = r0 - kZLo, br = r0 < kZLo ? 1u : 0u;
    const uint64_t d1 = r1 - kZHi - br;
    const bool below = r1 < kZHi || (r1 == kZHi && r0 < kZLo);  // r < z as 128-bit values
    const bool ge = top != 0 || !below;
    r0 = ge ? d0 : r0;
    r1 = ge ? d1 : r1;
    q1 = (q1 << 1) | (q0 >> 63);
    q0 = (q0 << 1) | (ge ? 1u : 0u);
  }
  a[0] = kZLo - r0;
  a[1] = kZHi - r1 - (kZLo < r0 ? 1u : 0u);
  b[0] = q0 + 1;
  b[1] = q1 + (b[0] == 0 ? 1u : 0u);
}

// ---- kernels ----------------------------------------------------------------------------------
__device__ __forceinline__ RFp rfp_select(bool c, const RFp& a, const RFp& b) {
  RFp r;
#pragma unroll
  for (int i = 0; i < RxShape<FpCfg>::L; ++i) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// an R'-domain value in [0, 2p) -> canonical packed R-domain
__device__ __forceinline__ Fp rfp_to_r(const RFp& v) { return fp_rx_to_r(rx_pack_canonical(v)); }

// temp[t] = [scalars[t]] pts[t] (XYZZ, canonical R-domain; ZZ = 0 for the identity). pts: affine
// R-domain points of G1, inf their identity flags, scalars canonical Montgomery.
// 2 waves per SIMD: the accumulator (52 limbs), the table (x, beta x, beta^2 x, y: 52) and the
// two halves stay live across the addition's ~100 temporaries.
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2)))
    k_g1_mul(const G1Affine* __restrict__ pts, const uint8_t* __restrict__ inf, const Fr* __restrict__ scalars,
             uint64_t n, G1xyzz* __restrict__ temp) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  uint64_t a[2], b[2];
  glv_split(fe_from_mont(ld_fr(&scalars[t])), a, b);
  Fp x, y;
  ld_aff(&pts[t], x, y);
  const bool is_inf = inf[t] != 0;
  const RFp x1 = rx_unpack(fe_to_rx_domain(x));
  const RFp yp = rx_unpack(fe_to_rx_domain(y));
  const RFp beta = rx_unpack(fe_to_rx_domain(fp_beta()));
  const RFp x2 = rx_mul(x1, beta), x3 = rx_mul(x2, beta);
  uint64_t a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
  G1R acc = g1r_infinity();
#pragma unroll 1
  for (int i = 0; i < 128; ++i) {
    acc = g1r_dbl_lazy(acc);
    const uint32_t d = (uint32_t)(a1 >> 63) | ((uint32_t)(b1 >> 63) << 1);
    a1 = (a1 << 1) | (a0 >> 63);
    a0 <<= 1;
    b1 = (b1 << 1) | (b0 >> 63);
    b0 <<= 1;
    // digit 1: -P, 2: -psi P, 3: -(P + psi P). A lane with the digit 0 sits the addition out under
    // the branch's mask: a select of the old accumulator would keep 52 more limbs live.
    if (d != 0) {
      const RFp xs = rfp_select(d == 1, x1, rfp_select(d == 2, x2, x3));
      // -y is formed here from an opaque copy: hoisted out of the loop it would hold 13 more
      // registers across every doubling and addition (the idiom of g1r_add_lazy_fix)
      uint32_t zero = 0;
      __asm__ volatile(";; plk loop-variant zero" : "+v"(zero));
      RFp yv = yp;
      yv.v[0] += zero;
      const RFp ys = rfp_select(d == 3, yv, rx_neg(yv));
      const bool was_inf = g1r_is_inf(acc);
      G1R r = g1r_madd_lazy_sl<true, true, true>(acc, xs, ys);
      if (rx_is_zero(r.ZZ)) r = g1r_madd_lazy_fix(was_inf, r, xs, ys);  // rare
      acc = r;
    }
  }
  acc = g1r_lazy_finish(acc);
  G1xyzz o;
  o.X = rfp_to_r(acc.X);
  o.Y = rfp_to_r(acc.Y);
  o.ZZ = rfp_to_r(acc.ZZ);
  o.ZZZ = rfp_to_r(acc.ZZZ);
  if (is_inf) o = xyzz_infinity();
  st_xyzz(&temp[t], o);
}

// ABI points -> the affine layout and identity flags; *bad = 1 for a point g1_load<true> refuses
__global__ void __launch_bounds__(kBlock) k_g1_mul_load(const plk_g1* __restrict__ in, uint64_t n,
                                                        G1Affine* __restrict__ pts, uint8_t* __restrict__ inf,
                                                        uint32_t* __restrict__ bad) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const G1Abi p = g1_load<true>(in + t);
  st_aff(&pts[t], p.x, p.y);
  inf[t] = p.inf ? 1 : 0;
  if (!p.ok) *bad = 1;
}

// out[i] = s^i (Montgomery), i < n
__global__ void __launch_bounds__(256) k_fr_powers(Fr s, uint64_t n, Fr* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Fr v = fe_pow_u64(s, i);
  uint4* dst = reinterpret_cast<uint4*>(&out[i]);
  dst[0] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  dst[1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
}

// out[4 i ..] = a_lo, a_hi, b_lo, b_hi of the Montgomery scalar i (plk_debug_glv_split)
__global__ void __launch_bounds__(kBlock) k_glv_split(const Fr* __restrict__ scalars, uint64_t n,
                                                      uint64_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  uint64_t a[2], b[2];
  glv_split(fe_from_mont(ld_fr(&scalars[t])), a, b);
  out[4 * t] = a[0];
  out[4 * t + 1] = a[1];
  out[4 * t + 2] = b[0];
  out[4 * t + 3] = b[1];
}

}  // namespace

// out[i] = [scal[i]] pts[i] in canonical affine form with identity flags; every pointer a device
// array of n entries, pts in G1 (the caller's check). Waits for the stream; the multiplication
// kernel's time goes to ctx->g1_mul_ms.
int g1_mul_dev(plk_ctx* ctx, const G1Affine* pts, const uint8_t* inf, const Fr* scal, uint64_t n,
               G1Affine* out, uint8_t* out_inf, hipStream_t s) {
  DevBuf temp, pref;
  TimingEvents<2> ev;
  int st;
  if ((st = temp.alloc(n * sizeof(G1xyzz)))) return st;
  if ((st = pref.alloc(n * sizeof(Fp)))) return st;
  if ((st = ev.create())) return st;
  // the events are stamped by the dispatch itself (as k_accumulate's): the kernel alone
  hipExtLaunchKernelGGL(k_g1_mul, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, ev.e[0], ev.e[1], 0, pts, inf, scal, n,
                        temp.as<G1xyzz>());
  PLK_HIP_TRY(hipGetLastError());
  if ((st = srs_batch_affine(temp.as<G1xyzz>(), n, pref.as<Fp>(), out, out_inf, s))) return st;
  PLK_HIP_TRY(stream_wait(s));
  ctx->g1_mul_ms = 0.f;
  (void)hipEventElapsedTime(&ctx->g1_mul_ms, ev.e[0], ev.e[1]);
  return PLK_OK;
}

// d_out[i] = s^i, i < n (Montgomery), stream-ordered
int fr_powers_dev(const Fr& s_mont, uint64_t n, Fr* d_out, hipStream_t s) {
  hipLaunchKernelGGL(k_fr_powers, dim3(cdiv(n, 256)), dim3(256), 0, s, s_mont, n, d_out);
  PLK_HIP_TRY(hipGetLastError());
  return PLK_OK;
}

}  // namespace plk

extern "C" {

int plk_g1_mul_batch(plk_ctx* ctx, const plk_g1* points, const plk_fr* scalars, size_t n, int assume_subgroup,
                     plk_g1* out) {
  PLK_API_BEGIN
  if (!ctx || n > kMaxBatch) return PLK_E_ARG;
  if (n == 0) return PLK_OK;
  if (!points || !scalars || !out) return PLK_E_ARG;
  for (size_t i = 0; i < n; ++i)
    if (!abi_canonical<FrCfg>(scalars[i].l)) return PLK_E_ARG;
  int st;
  if (!assume_subgroup) {  // the split is only valid on G1
    std::vector<uint8_t> ok(n);
    if ((st = plk_g1_subgroup_check_batch(ctx, points, n, ok.data()))) return st;
    for (size_t i = 0; i < n; ++i)
      if (!ok[i]) return PLK_E_ARG;
  }
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  DevBuf d_in, d_scal, d_pts, d_inf, d_out, d_oinf, d_bad;
  if ((st = d_in.alloc(n * sizeof(plk_g1)))) return st;
  if ((st = d_scal.alloc(n * sizeof(Fr)))) return st;
  if ((st = d_pts.alloc(n * sizeof(G1Affine)))) return st;
  if ((st = d_inf.alloc(n))) return st;
  if ((st = d_out.alloc(n * sizeof(G1Affine)))) return st;
  if ((st = d_oinf.alloc(n))) return st;
  if ((st = d_bad.alloc(sizeof(uint32_t)))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(d_in.ptr, points, n * sizeof(plk_g1), hipMemcpyHostToDevice, s));
  PLK_HIP_TRY(hipMemcpyAsync(d_scal.ptr, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, s));
  PLK_HIP_TRY(hipMemsetAsync(d_bad.ptr, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_g1_mul_load, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, (const plk_g1*)d_in.as<plk_g1>(),
                     (uint64_t)n, d_pts.as<G1Affine>(), d_inf.as<uint8_t>(), d_bad.as<uint32_t>());
  PLK_HIP_TRY(hipGetLastError());
  uint32_t bad = 0;
  PLK_HIP_TRY(hipMemcpyAsync(&bad, d_bad.ptr, sizeof bad, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  if (bad) return PLK_E_ARG;
  if ((st = g1_mul_dev(ctx, d_pts.as<G1Affine>(), d_inf.as<uint8_t>(), d_scal.as<Fr>(), n, d_out.as<G1Affine>(),
                       d_oinf.as<uint8_t>(), s)))
    return st;
  std::vector<G1Affine> res(n);
  std::vector<uint8_t> rinf(n);
  PLK_HIP_TRY(hipMemcpyAsync(res.data(), d_out.ptr, n * sizeof(G1Affine), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(hipMemcpyAsync(rinf.data(), d_oinf.ptr, n, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  for (size_t i = 0; i < n; ++i) g1_store(res[i].x, res[i].y, !rinf[i], &out[i]);
  return PLK_OK;
  PLK_API_END
}

int plk_g1_mul_last_ms(plk_ctx* ctx, float* kernel_ms) {
  if (!ctx || !kernel_ms) return PLK_E_ARG;
  *kernel_ms = ctx->g1_mul_ms;
  return PLK_OK;
}

int plk_debug_glv_split(plk_ctx* ctx, const plk_fr* s, size_t n, uint64_t* out) {
  PLK_API_BEGIN
  if (n > kMaxBatch) return PLK_E_ARG;
  if (n == 0) return PLK_OK;
  if (!s || !out) return PLK_E_ARG;
  for (size_t i = 0; i < n; ++i)
    if (!abi_canonical<FrCfg>(s[i].l)) return PLK_E_ARG;
  if (!ctx) {
    for (size_t i = 0; i < n; ++i) {
      uint64_t a[2], b[2];
      glv_split(fe_from_mont(fr_from_abi(s[i])), a, b);
      out[4 * i] = a[0];
      out[4 * i + 1] = a[1];
      out[4 * i + 2] = b[0];
      out[4 * i + 3] = b[1];
    }
    return PLK_OK;
  }
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  DevBuf d_s, d_out;
  int r;
  if ((r = d_s.alloc(n * sizeof(Fr)))) return r;
  if ((r = d_out.alloc(n * 4 * sizeof(uint64_t)))) return r;
  PLK_HIP_TRY(hipMemcpyAsync(d_s.ptr, s, n * sizeof(Fr), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_glv_split, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, st, (const Fr*)d_s.as<Fr>(), (uint64_t)n,
                     d_out.as<uint64_t>());
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipMemcpyAsync(out, d_out.ptr, n * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  PLK_HIP_TRY(stream_wait(st));
  return PLK_OK;
  PLK_API_END
}

}  // extern "C"
