// lagrange.hip — the Lagrange-basis SRS of an n-point domain, from the SRS points alone.
//
// A polynomial given by its values v_i = w(omega^i) commits to sum_i v_i [L_i(tau)]_1, and
//   P_i = [L_i(tau)]_1 = n^-1 sum_j omega^(-ij) [tau^j]_1,
// the inverse DFT of the first n SRS points taken over G1. A column that is zero (or sparse) in
// the evaluation basis then costs the MSM nothing (msm_sort.hip emits no entry for a zero digit),
// where its n dense coefficients cost a full MSM. Three more points carry a blinder
// b(X)(X^n - 1), b of degree <= 2, in the same MSM:
//   Z_t = [tau^(n+t)]_1 - [tau^t]_1  (t < 3),   commit = sum_i v_i P_i + sum_t b_t Z_t
// over the contiguous scalars [values | b_0 b_1 b_2]. The result is an ordinary plk_srs of
// n + 3 points (batch-affine, window table, table_inf), so msm_run_batch takes it unchanged.
//
// The transform is a radix-2 decimation-in-frequency pass per level, one thread per butterfly
// (u, v) -> (u + v, omega_len^-j (u - v)), in place on XYZZ points in the packed R-domain
// arithmetic of g1.hpp (exact, with every exceptional case of the group law: an SRS whose tau
// is an n-th root of unity sends all but one P_i, and Z_0, to infinity). The twiddle is a
// 255-bit scalar multiplication (2-bit fixed windows); the last level has none. Then the
// bit-reversal, the n^-1 scale and the Z_t in one kernel. Cost: (n / 2)(log n - 1) + n scalar
// multiplications, once per key.
#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "msm_common.hpp"
#include "xyzz_mul.hpp"

namespace plk {

namespace {

__device__ __forceinline__ G1xyzz ld_point(const G1Affine* __restrict__ pts,
                                           const uint8_t* __restrict__ inf, uint64_t i) {
  if (inf[i]) return xyzz_infinity();
  Fp x, y;
  ld_aff(&pts[i], x, y);
  return xyzz_from_affine(G1Affine{x, y});
}

__global__ void __launch_bounds__(256) k_ec_load(const G1Affine* __restrict__ pts,
                                                 const uint8_t* __restrict__ inf, uint64_t n,
                                                 G1xyzz* __restrict__ a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) st_xyzz(&a[i], ld_point(pts, inf, i));
}

// One level of the inverse transform over blocks of len = 2^log_len: butterfly t of n / 2.
// tw_fwd: omega^e, e < n (R domain), so omega_len^-j = tw_fwd[(n - j n / len) mod n].
__global__ void __launch_bounds__(128) k_ec_dif(G1xyzz* __restrict__ a, uint64_t n, uint32_t log_len,
                                                const Fr* __restrict__ tw_fwd) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n / 2) return;
  const uint64_t half = 1ull << (log_len - 1), j = t & (half - 1);
  const uint64_t i0 = ((t >> (log_len - 1)) << log_len) + j, i1 = i0 + half;
  G1xyzz u, v;
  ld_xyzz(&a[i0], u);
  ld_xyzz(&a[i1], v);
  st_xyzz(&a[i0], xyzz_add(u, v));
  G1xyzz d = xyzz_add(u, xyzz_neg(v));
  if (log_len > 1) {  // uniform: the last level's twiddles are all 1
    const uint64_t e = j * (n >> log_len);
    d = xyzz_mul(d, fe_from_mont(ld_fr(&tw_fwd[(n - e) & (n - 1)])));
  }
  st_xyzz(&a[i1], d);
}

// out[i] = n^-1 a[bitrev(i)] (i < n), out[n + t] = S[n + t] - S[t] (t < 3)
__global__ void __launch_bounds__(128) k_ec_finish(const G1xyzz* __restrict__ a, uint64_t n, uint32_t log_n,
                                                   Fr n_inv, const G1Affine* __restrict__ pts,
                                                   const uint8_t* __restrict__ inf,
                                                   G1xyzz* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n + 3) return;
  if (i >= n) {
    st_xyzz(&out[i], xyzz_add(ld_point(pts, inf, i), xyzz_neg(ld_point(pts, inf, i - n))));
    return;
  }
  const uint64_t r = log_n ? __brevll(i) >> (64 - log_n) : 0;
  G1xyzz p;
  ld_xyzz(&a[r], p);
  st_xyzz(&out[i], xyzz_mul(p, n_inv));
}

}  // namespace

// srs.hip
int srs_batch_affine(const G1xyzz* temp, uint64_t n, Fp* pref, G1Affine* out, uint8_t* out_inf,
                     hipStream_t stream);

int srs_lagrange_build(plk_srs* src, plk_domain* dom, bool own_ws, plk_srs** out) {
  *out = nullptr;
  const uint64_t n = dom->n;
  if (!src || n < 2 || src->n < n + 3 || src->ctx != dom->ctx) return PLK_E_ARG;
  hipStream_t stream = src->ctx->stream;
  std::unique_ptr<plk_srs> s(new plk_srs());
  s->ctx = src->ctx;
  s->n = n + 3;
  int st;
  if ((st = s->points.alloc(s->n * sizeof(G1Affine)))) return st;
  if ((st = s->inf.alloc(s->n))) return st;
  DevBuf a, b, pref;
  if ((st = a.alloc(n * sizeof(G1xyzz)))) return st;
  if ((st = b.alloc(s->n * sizeof(G1xyzz)))) return st;
  if ((st = pref.alloc(s->n * sizeof(Fp)))) return st;
  const G1Affine* pts = src->points.as<G1Affine>();
  const uint8_t* inf = src->inf.as<uint8_t>();
  hipLaunchKernelGGL(k_ec_load, dim3(cdiv(n, 256)), dim3(256), 0, stream, pts, inf, n, a.as<G1xyzz>());
  for (uint32_t ll = dom->log_n; ll >= 1; --ll)
    hipLaunchKernelGGL(k_ec_dif, dim3(cdiv(n / 2, 128)), dim3(128), 0, stream, a.as<G1xyzz>(), n, ll,
                       (const Fr*)dom->tw_fwd.as<Fr>());
  hipLaunchKernelGGL(k_ec_finish, dim3(cdiv(n + 3, 128)), dim3(128), 0, stream,
                     (const G1xyzz*)a.as<G1xyzz>(), n, dom->log_n, fe_from_mont(dom->n_inv), pts, inf,
                     b.as<G1xyzz>());
  PLK_HIP_TRY(hipGetLastError());
  if ((st = srs_batch_affine(b.as<G1xyzz>(), s->n, pref.as<Fp>(), s->points.as<G1Affine>(),
                             s->inf.as<uint8_t>(), stream)))
    return st;
  std::vector<uint8_t> flags(s->n);
  PLK_HIP_TRY(hipMemcpyAsync(flags.data(), s->inf.ptr, s->n, hipMemcpyDeviceToHost, stream));
  PLK_HIP_TRY(stream_wait(stream));
  s->has_inf = false;
  for (uint8_t f : flags) s->has_inf |= f != 0;
  a = DevBuf();
  b = DevBuf();
  pref = DevBuf();
  // the key SRS's window size and table layout: one workspace shape serves both bases
  if ((st = msm_prepare_srs(s.get(), stream, src->c, own_ws, src->naf ? 1 : 0))) return st;
  *out = s.release();
  return PLK_OK;
}

}  // namespace plk
