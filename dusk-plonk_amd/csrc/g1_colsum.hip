// g1_colsum.hip — the two column reductions of the coset openings (kzg.hip, plk_kzg_open_cosets and
// plk_kzg_fold_cosets):
//   g1_colsum_dev:        out_t = sum_{a < rows} in[a][t]               over G1,
//   fr_interp_reduce_dev: P_i   = sum_{k < count} rho_k z_k^-i c[k][i]  over Fr.
// Both read a row-major matrix with the column index fastest, so a wave reads consecutive columns.
//
// The G1 sum takes affine points with identity flags (what g1_mul_dev leaves) and writes XYZZ,
// straight into the inverse transform of g1_ntt.hip. Every addition is xyzz_add, the complete
// group law: equal addends double, opposite ones give the identity, identities pass through. That
// is needed, not caution: whoever knows tau (every test SRS) can choose f so that two products of
// one column coincide or cancel.
//
// What was chosen: a split of the rows over `split` lanes per column and a second pass, not an LDS
// tree. A column is a chain of rows - 1 dependent additions; with cols = 2r lanes alone a 2^12
// domain in cosets of 64 would run 128 lanes, each 63 additions deep. So lane (s, t) of the first
// pass sums the rows s, s + split, .. of column t into partial[s][t], and the second pass sums the
// `split` partials of a column the same way (its rows are XYZZ). split = min(rows, 64,
// ceil(65536 / cols)): once the columns alone fill the chip (some 64 Ki lanes) it is 1 and the
// first pass writes the result itself. A second pass costs one launch and split additions per
// column; an LDS tree would tie a column's lanes to one workgroup, give up the coalesced reads
// (the stride between a column's rows is cols points), and hold 192-byte points in LDS for a
// saving of a few additions. The same kernel serves both passes and every split, so there is one
// code path, with or without partials.
//
// A fused form (one shared doubling chain per column instead of one per product) was not built:
// the products go through g1_mul_dev, whose chain on the endomorphism split is the measured one.
//
// The Fr reduction is the same two-pass shape. Lane (s, i) of the first pass takes the rows k = s,
// s + split, .. and keeps z_k^-i by square-and-multiply on i (at most 20 bits), so a row costs
// about 2 log2(l) multiplications however long the column; split = min(count, 1024,
// ceil(65536 / l)), so 65 536 openings of one point and one opening of 2^20 points both run on
// some 64 Ki lanes or more.
#include <hip/hip_runtime.h>

#include <vector>

#include "internal.hpp"
#include "msm_common.hpp"

namespace plk {

int srs_batch_affine(const G1xyzz* temp, uint64_t n, Fp* pref, G1Affine* out, uint8_t* out_inf,
                     hipStream_t stream);

namespace {

constexpr uint64_t kFillLanes = 65536;  // lanes that fill the chip: 256 CUs x 4 SIMDs x 64
constexpr uint64_t kMaxSplitG1 = 64, kMaxSplitFr = 1024;

uint64_t split_of(uint64_t rows, uint64_t cols, uint64_t cap) {
  uint64_t s = (kFillLanes + cols - 1) / cols;
  if (s > cap) s = cap;
  if (s > rows) s = rows;
  return s ? s : 1;
}

// AFFINE: row a of column t is (pts, inf)[a * cols + t]; otherwise xyzz[a * cols + t].
// out[s * cols + t] = the sum of the rows a = s, s + split, .. < rows of column t.
template <bool AFFINE>
__global__ void __launch_bounds__(64) k_g1_colsum(const G1Affine* __restrict__ pts, const uint8_t* __restrict__ inf,
                                                  const G1xyzz* __restrict__ xyzz, uint64_t rows, uint64_t cols,
                                                  uint64_t split, G1xyzz* __restrict__ out) {
  const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= split * cols) return;
  const uint64_t s = lane / cols, t = lane - s * cols;
  G1xyzz acc = xyzz_infinity();
  for (uint64_t a = s; a < rows; a += split) {
    const uint64_t k = a * cols + t;
    G1xyzz p;
    if (AFFINE) {
      if (inf[k]) continue;
      Fp x, y;
      ld_aff(&pts[k], x, y);
      p = xyzz_from_affine(G1Affine{x, y});
    } else {
      ld_xyzz(&xyzz[k], p);
    }
    acc = xyzz_add(acc, p);
  }
  st_xyzz(&out[lane], acc);
}

__device__ __forceinline__ void st_fr(Fr* p, const Fr& r) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
  q[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}

// WEIGHTED: out[s * l + i] = sum over k = s, s + split, .. < count of rho[k] zinv[k]^i c[k * l + i];
// otherwise the plain sum of c[k * l + i] over the same rows (the second pass).
template <bool WEIGHTED>
__global__ void __launch_bounds__(256) k_fr_colsum(const Fr* __restrict__ c, const Fr* __restrict__ rho,
                                                   const Fr* __restrict__ zinv, uint64_t count, uint64_t l,
                                                   uint64_t split, Fr* __restrict__ out) {
  const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= split * l) return;
  const uint64_t s = lane / l, i = lane - s * l;
  Fr acc = fe_zero<FrCfg>();
  for (uint64_t k = s; k < count; k += split) {
    Fr v = ld_fr(&c[k * l + i]);
    if (WEIGHTED) {
      Fr w = ld_fr(&rho[k]);
      if (i) {  // z_k^-i, i < 2^20
        Fr b = ld_fr(&zinv[k]);
        for (uint64_t e = i; e; e >>= 1) {
          if (e & 1) w = fe_mul(w, b);
          b = fe_sqr(b);
        }
      }
      v = fe_mul(v, w);
    }
    acc = fe_add(acc, v);
  }
  st_fr(&out[lane], acc);
}

// ABI points -> affine with flags; *bad = 1 for a point g1_load<true> refuses
__global__ void __launch_bounds__(256) k_colsum_load_abi(const plk_g1* __restrict__ in, uint64_t n,
                                                         G1Affine* __restrict__ out, uint8_t* __restrict__ out_inf,
                                                         uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1Abi p = g1_load<true>(in + i);
  if (!p.ok) *bad = 1;
  const bool inf = p.inf || !p.ok;
  out_inf[i] = inf ? 1 : 0;
  st_aff(&out[i], inf ? fe_zero<FpCfg>() : p.x, inf ? fe_zero<FpCfg>() : p.y);
}

}  // namespace

int g1_colsum_dev(const G1Affine* pts, const uint8_t* inf, uint64_t rows, uint64_t cols, G1xyzz* out,
                  hipStream_t stream) {
  if (!pts || !inf || !out || rows == 0 || cols == 0) return PLK_E_ARG;
  const uint64_t split = split_of(rows, cols, kMaxSplitG1);
  if (split == 1) {
    hipLaunchKernelGGL(k_g1_colsum<true>, dim3(cdiv(cols, 64)), dim3(64), 0, stream, pts, inf,
                       (const G1xyzz*)nullptr, rows, cols, split, out);
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
  }
  AsyncBuf partial;
  int st;
  if ((st = partial.alloc(split * cols * sizeof(G1xyzz), stream))) return st;
  hipLaunchKernelGGL(k_g1_colsum<true>, dim3(cdiv(split * cols, 64)), dim3(64), 0, stream, pts, inf,
                     (const G1xyzz*)nullptr, rows, cols, split, partial.as<G1xyzz>());
  hipLaunchKernelGGL(k_g1_colsum<false>, dim3(cdiv(cols, 64)), dim3(64), 0, stream, (const G1Affine*)nullptr,
                     (const uint8_t*)nullptr, (const G1xyzz*)partial.as<G1xyzz>(), split, cols, (uint64_t)1, out);
  PLK_HIP_TRY(hipGetLastError());
  return PLK_OK;
}

int fr_interp_reduce_dev(const Fr* c, const Fr* rho, const Fr* zinv, uint64_t count, uint64_t l, Fr* out,
                         hipStream_t stream) {
  if (!c || !rho || !zinv || !out || count == 0 || l == 0) return PLK_E_ARG;
  const uint64_t split = split_of(count, l, kMaxSplitFr);
  if (split == 1) {
    hipLaunchKernelGGL(k_fr_colsum<true>, dim3(cdiv(l, 256)), dim3(256), 0, stream, c, rho, zinv, count, l, split,
                       out);
    PLK_HIP_TRY(hipGetLastError());
    return PLK_OK;
  }
  AsyncBuf partial;
  int st;
  if ((st = partial.alloc(split * l * sizeof(Fr), stream))) return st;
  hipLaunchKernelGGL(k_fr_colsum<true>, dim3(cdiv(split * l, 256)), dim3(256), 0, stream, c, rho, zinv, count, l,
                     split, partial.fr());
  hipLaunchKernelGGL(k_fr_colsum<false>, dim3(cdiv(l, 256)), dim3(256), 0, stream, (const Fr*)partial.fr(),
                     (const Fr*)nullptr, (const Fr*)nullptr, split, l, (uint64_t)1, out);
  PLK_HIP_TRY(hipGetLastError());
  return PLK_OK;
}

}  // namespace plk

using namespace plk;

extern "C" {

int plk_debug_g1_colsum(plk_ctx* ctx, const plk_g1* points, size_t rows, size_t cols, plk_g1* out) {
  PLK_API_BEGIN
  if (!ctx || !points || !out || rows == 0 || cols == 0) return PLK_E_ARG;
  if (rows > ((size_t)1 << 21) || cols > ((size_t)1 << 21) || rows * cols > ((size_t)1 << 21)) return PLK_E_ARG;
  const uint64_t n = (uint64_t)rows * cols;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  AsyncBuf abi, aff, inf, sum, pref, res, rinf, bad;
  int st;
  if ((st = abi.alloc(n * sizeof(plk_g1), s))) return st;
  if ((st = aff.alloc(n * sizeof(G1Affine), s))) return st;
  if ((st = inf.alloc(n, s))) return st;
  if ((st = sum.alloc(cols * sizeof(G1xyzz), s))) return st;
  if ((st = pref.alloc(cols * sizeof(Fp), s))) return st;
  if ((st = res.alloc(cols * sizeof(G1Affine), s))) return st;
  if ((st = rinf.alloc(cols, s))) return st;
  if ((st = bad.alloc(16, s))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(abi.ptr, points, n * sizeof(plk_g1), hipMemcpyHostToDevice, s));
  PLK_HIP_TRY(hipMemsetAsync(bad.ptr, 0, 16, s));
  hipLaunchKernelGGL(k_colsum_load_abi, dim3(cdiv(n, 256)), dim3(256), 0, s, (const plk_g1*)abi.as<plk_g1>(), n,
                     aff.as<G1Affine>(), inf.as<uint8_t>(), bad.as<uint32_t>());
  PLK_HIP_TRY(hipGetLastError());
  if ((st = g1_colsum_dev(aff.as<G1Affine>(), inf.as<uint8_t>(), rows, cols, sum.as<G1xyzz>(), s))) return st;
  if ((st = srs_batch_affine(sum.as<G1xyzz>(), cols, pref.as<Fp>(), res.as<G1Affine>(), rinf.as<uint8_t>(), s)))
    return st;
  std::vector<G1Affine> h(cols);
  std::vector<uint8_t> hinf(cols);
  uint32_t hbad = 0;
  PLK_HIP_TRY(hipMemcpyAsync(h.data(), res.ptr, cols * sizeof(G1Affine), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(hipMemcpyAsync(hinf.data(), rinf.ptr, cols, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(hipMemcpyAsync(&hbad, bad.ptr, sizeof hbad, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  if (hbad) return PLK_E_ARG;
  for (size_t i = 0; i < cols; ++i) g1_store(h[i].x, h[i].y, !hinf[i], &out[i]);
  return PLK_OK;
  PLK_API_END
}

}  // extern "C"
