// g1_ntt.hip — the discrete Fourier transform over G1 at any power-of-two size, both directions:
//   out_i = sum_j omega^(+-ij) P_j   (natural order in and out; the inverse carries n^-1),
// omega the generator of the 2^log_n domain (ntt.hip; the twiddles are the domain's own tw_fwd).
//
// A radix-2 decimation-in-frequency pass per level, one lane per butterfly
//   (u, v) -> (u + v, w (u - v)),   w = omega_len^(+-j),
// in place on packed XYZZ points in the R-domain arithmetic of g1.hpp, then the bit-reversal as
// swaps in place and, for the inverse, one multiplication by n^-1 per point. xyzz_add is the
// complete group law (u = v doubles, u = -v gives the identity, identities pass through). A
// butterfly whose twiddle is 1 (j = 0 at every level, the whole last level) does no
// multiplication: (n / 2)(log n - 2) + 1 twiddle multiplications, + n for the inverse's scale.
//
// Two forms of the multiplication (G1NttForm), the same results bit for bit:
//  - kXyzz: inside the butterfly, lagrange.hip's 255-bit windowed xyzz_mul. No endomorphism, so
//    exact for any points of the curve, and stream-ordered. One wave per SIMD (256 VGPRs and 228
//    spilled to AGPRs): a level is one 255-step chain deep.
//  - kGlv: the differences leave the butterfly for a compact array, one batch inversion makes them
//    affine and g1_mul.hip's 128-step chain on the endomorphism split multiplies them (g1_mul_dev,
//    with its own batch inversion). Valid on G1 only: the caller's guarantee.
// Measured inside plk_kzg_open_domain (profiles/kzg_open.jsonl): a forward transform
// of 2^17 points takes 125.4 ms as kXyzz and 119.2 ms as kGlv, 127.6 and 121.2 ns per twiddle
// multiplication; at 2^13 and 2^9 points 91.9 / 60.6 ms and 60.7 / 44.3 ms. Up to 2^17 points
// both are bound by the depth of one multiplication chain per level (some 7.5 and 5.5 ms a level),
// not by throughput, so neither reaches its kernel's rate at scale (127 and 32 ns).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "internal.hpp"
#include "msm_common.hpp"
#include "prover.hpp"
#include "xyzz_mul.hpp"

namespace plk {

int srs_batch_affine(const G1xyzz* temp, uint64_t n, Fp* pref, G1Affine* out, uint8_t* out_inf,
                     hipStream_t stream);

namespace {

constexpr uint32_t kMaxLog = 27;  // plk_domain_get's range

// One level over blocks of len = 2^log_len: butterfly t of total / 2, total = batch n points (the
// transforms lie one after the other, and len divides n, so a block never straddles two of them).
// tw_fwd: omega^e, e < n (R domain, Montgomery), so omega_len^j = tw_fwd[j n / len] and
// omega_len^-j = tw_fwd[(n - j n / len) mod n].
__global__ void __launch_bounds__(128) k_g1_dif(G1xyzz* __restrict__ a, uint64_t total, uint64_t n, uint32_t log_len,
                                                const Fr* __restrict__ tw_fwd, int inverse) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total / 2) return;
  const uint64_t half = 1ull << (log_len - 1), j = t & (half - 1);
  const uint64_t i0 = ((t >> (log_len - 1)) << log_len) + j, i1 = i0 + half;
  G1xyzz u, v;
  ld_xyzz(&a[i0], u);
  ld_xyzz(&a[i1], v);
  st_xyzz(&a[i0], xyzz_add(u, v));
  G1xyzz d = xyzz_add(u, xyzz_neg(v));
  if (j != 0) {  // j = 0: the twiddle is 1
    const uint64_t e = j * (n >> log_len);
    d = xyzz_mul(d, fe_from_mont(ld_fr(&tw_fwd[inverse ? (n - e) & (n - 1) : e])));
  }
  st_xyzz(&a[i1], d);
}

// a[i] <-> a[bitrev(i)] inside every transform of 2^log_n points, the lane of the smaller index swaps
__global__ void __launch_bounds__(256) k_g1_bitrev(G1xyzz* __restrict__ a, uint64_t total, uint32_t log_n) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint64_t i = g & ((1ull << log_n) - 1);
  const uint64_t r = __brevll(i) >> (64 - log_n);
  if (r <= i) return;
  a += g - i;
  G1xyzz p, q;
  ld_xyzz(&a[i], p);
  ld_xyzz(&a[r], q);
  st_xyzz(&a[i], q);
  st_xyzz(&a[r], p);
}

// a[i] = [s] a[i], s canonical (not Montgomery)
__global__ void __launch_bounds__(128) k_g1_scale(G1xyzz* __restrict__ a, uint64_t n, Fr s) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1xyzz p;
  ld_xyzz(&a[i], p);
  st_xyzz(&a[i], xyzz_mul(p, s));
}

// out[i] = pts[rev ? first - i : first + i] for i < m, the identity for m <= i < n
__global__ void __launch_bounds__(256) k_g1_load(const G1Affine* __restrict__ pts, const uint8_t* __restrict__ inf,
                                                 uint64_t first, int rev, uint64_t m, uint64_t n,
                                                 G1xyzz* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1xyzz p = xyzz_infinity();
  if (i < m) {
    const uint64_t k = rev ? first - i : first + i;
    if (!inf[k]) {
      Fp x, y;
      ld_aff(&pts[k], x, y);
      p = xyzz_from_affine(G1Affine{x, y});
    }
  }
  st_xyzz(&out[i], p);
}

// ---- the affine-between-levels form ("glv") ------------------------------------------------------
// The same butterfly with the multiplication taken out of it: u + v goes to a[i0] and u - v, for
// j = 0 (twiddle 1), to a[i1]; every other difference goes to the compact array d with its twiddle
// beside it, block b's differences j = 1 .. half - 1 at b (half - 1) + j - 1. One batch inversion
// brings d to affine form, k_g1_mul (g1_mul.hip: the 128-step chain on the endomorphism split)
// multiplies, and k_g1_scatter puts the products back. The split is valid on G1 only.
__global__ void __launch_bounds__(128) k_g1_bfly_split(G1xyzz* __restrict__ a, uint64_t total, uint64_t n,
                                                       uint32_t log_len, const Fr* __restrict__ tw_fwd, int inverse,
                                                       G1xyzz* __restrict__ d, Fr* __restrict__ tw) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total / 2) return;
  const uint64_t half = 1ull << (log_len - 1), j = t & (half - 1), blk = t >> (log_len - 1);
  const uint64_t i0 = (blk << log_len) + j, i1 = i0 + half;
  G1xyzz u, v;
  ld_xyzz(&a[i0], u);
  ld_xyzz(&a[i1], v);
  st_xyzz(&a[i0], xyzz_add(u, v));
  const G1xyzz diff = xyzz_add(u, xyzz_neg(v));
  if (j == 0) {
    st_xyzz(&a[i1], diff);
    return;
  }
  const uint64_t k = blk * (half - 1) + j - 1, e = j * (n >> log_len);
  st_xyzz(&d[k], diff);
  const uint4* src = reinterpret_cast<const uint4*>(&tw_fwd[inverse ? (n - e) & (n - 1) : e]);
  uint4* dst = reinterpret_cast<uint4*>(&tw[k]);
  dst[0] = src[0];
  dst[1] = src[1];
}

// a[i1] = the product of butterfly t's difference (j != 0), from the compact affine array
__global__ void __launch_bounds__(256) k_g1_scatter(const G1Affine* __restrict__ prod,
                                                    const uint8_t* __restrict__ prod_inf, uint64_t total,
                                                    uint32_t log_len, G1xyzz* __restrict__ a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total / 2) return;
  const uint64_t half = 1ull << (log_len - 1), j = t & (half - 1), blk = t >> (log_len - 1);
  if (j == 0) return;
  const uint64_t k = blk * (half - 1) + j - 1;
  G1xyzz p = xyzz_infinity();
  if (!prod_inf[k]) {
    Fp x, y;
    ld_aff(&prod[k], x, y);
    p = xyzz_from_affine(G1Affine{x, y});
  }
  st_xyzz(&a[(blk << log_len) + j + half], p);
}

// ABI points -> XYZZ; *bad = 1 for a point g1_load<true> refuses
__global__ void __launch_bounds__(256) k_g1_load_abi(const plk_g1* __restrict__ in, uint64_t n,
                                                     G1xyzz* __restrict__ out, uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1Abi p = g1_load<true>(in + i);
  if (!p.ok) *bad = 1;
  st_xyzz(&out[i], p.inf || !p.ok ? xyzz_infinity() : xyzz_from_affine(G1Affine{p.x, p.y}));
}

// The glv form of g1_ntt_run_batch on points of G1: the differences of all `batch` transforms go
// through one batch inversion and one multiplication per level. g1_mul_dev waits for the stream at
// every level.
int run_glv(plk_ctx* ctx, plk_domain* dom, G1xyzz* points, uint64_t batch, int dir, hipStream_t s, bool scale) {
  const uint64_t n = dom->n, total = batch * n, cap = total;  // the levels need total / 2 slots, the scale pass total
  const uint32_t log_n = dom->log_n;
  AsyncBuf d, tw, aff, inf, pref, prod, prod_inf;
  int st;
  if ((st = d.alloc(cap * sizeof(G1xyzz), s))) return st;
  if ((st = tw.alloc(cap * sizeof(Fr), s))) return st;
  if ((st = aff.alloc(cap * sizeof(G1Affine), s))) return st;
  if ((st = inf.alloc(cap, s))) return st;
  if ((st = pref.alloc(cap * sizeof(Fp), s))) return st;
  if ((st = prod.alloc(cap * sizeof(G1Affine), s))) return st;
  if ((st = prod_inf.alloc(cap, s))) return st;
  for (uint32_t ll = log_n; ll >= 1; --ll) {
    hipLaunchKernelGGL(k_g1_bfly_split, dim3(cdiv(total / 2, 128)), dim3(128), 0, s, points, total, n, ll,
                       (const Fr*)dom->tw_fwd.as<Fr>(), dir < 0 ? 1 : 0, d.as<G1xyzz>(), tw.fr());
    PLK_HIP_TRY(hipGetLastError());
    const uint64_t m = total / 2 - (total >> ll);  // the butterflies with j != 0
    if (m == 0) continue;
    if ((st = srs_batch_affine(d.as<G1xyzz>(), m, pref.as<Fp>(), aff.as<G1Affine>(), inf.as<uint8_t>(), s))) return st;
    if ((st = g1_mul_dev(ctx, aff.as<G1Affine>(), inf.as<uint8_t>(), tw.fr(), m, prod.as<G1Affine>(),
                         prod_inf.as<uint8_t>(), s)))
      return st;
    hipLaunchKernelGGL(k_g1_scatter, dim3(cdiv(total / 2, 256)), dim3(256), 0, s, (const G1Affine*)prod.as<G1Affine>(),
                       (const uint8_t*)prod_inf.as<uint8_t>(), total, ll, points);
    PLK_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_g1_bitrev, dim3(cdiv(total, 256)), dim3(256), 0, s, points, total, log_n);
  PLK_HIP_TRY(hipGetLastError());
  if (dir < 0 && scale) {
    if ((st = srs_batch_affine(points, total, pref.as<Fp>(), aff.as<G1Affine>(), inf.as<uint8_t>(), s))) return st;
    if ((st = pk_fill(tw.fr(), dom->n_inv, total, s))) return st;
    if ((st = g1_mul_dev(ctx, aff.as<G1Affine>(), inf.as<uint8_t>(), tw.fr(), total, prod.as<G1Affine>(),
                         prod_inf.as<uint8_t>(), s)))
      return st;
    if ((st = g1_xyzz_load(prod.as<G1Affine>(), prod_inf.as<uint8_t>(), 0, false, total, total, points, s))) return st;
  }
  return PLK_OK;
}

// PLK_G1_NTT_FORM (experiments, tools/kzg_open_bench.py): "xyzz" or "glv" instead of the default
G1NttForm chosen_form(G1NttForm form) {
  if (const char* e = getenv("PLK_G1_NTT_FORM")) {
    if (!strcmp(e, "xyzz")) return G1NttForm::kXyzz;
    if (!strcmp(e, "glv")) return G1NttForm::kGlv;
  }
  return form;
}

}  // namespace

// The transform of the 2^log_n device-resident points, in place and stream-ordered; dir = +1
// forward, -1 inverse. scale = false leaves the inverse's n^-1 to the caller. form: kXyzz is exact
// for any points of the curve; kGlv asks for points of G1 (the caller's check).
int g1_ntt_run(plk_ctx* ctx, G1xyzz* points, uint32_t log_n, int dir, hipStream_t stream, bool scale,
               G1NttForm form) {
  return g1_ntt_run_batch(ctx, points, log_n, 1, dir, stream, scale, form);
}

// `batch` transforms of 2^log_n points each, one after the other in `points`: every level, the bit
// reversal and the scale are one launch over all batch 2^log_n points, so the batch is as deep as
// one transform. The kernels index a butterfly's block across the whole array and take only the
// twiddle from the transform's own size; batch = 1 is the single transform, launch for launch.
int g1_ntt_run_batch(plk_ctx* ctx, G1xyzz* points, uint32_t log_n, uint64_t batch, int dir, hipStream_t stream,
                     bool scale, G1NttForm form) {
  if (!ctx || !points || log_n > kMaxLog || (dir != 1 && dir != -1)) return PLK_E_ARG;
  if (batch == 0 || batch > (1ull << kMaxLog) >> log_n) return PLK_E_ARG;
  if (log_n == 0) return PLK_OK;
  plk_domain* dom = nullptr;
  int st;
  if ((st = plk_domain_get(ctx, log_n, &dom))) return st;
  const uint64_t n = dom->n, total = batch * n;
  if (chosen_form(form) == G1NttForm::kGlv) return run_glv(ctx, dom, points, batch, dir, stream, scale);
  for (uint32_t ll = log_n; ll >= 1; --ll)
    hipLaunchKernelGGL(k_g1_dif, dim3(cdiv(total / 2, 128)), dim3(128), 0, stream, points, total, n, ll,
                       (const Fr*)dom->tw_fwd.as<Fr>(), dir < 0 ? 1 : 0);
  hipLaunchKernelGGL(k_g1_bitrev, dim3(cdiv(total, 256)), dim3(256), 0, stream, points, total, log_n);
  if (dir < 0 && scale)
    hipLaunchKernelGGL(k_g1_scale, dim3(cdiv(total, 128)), dim3(128), 0, stream, points, total,
                       fe_from_mont(dom->n_inv));
  PLK_HIP_TRY(hipGetLastError());
  return PLK_OK;
}

// out[i] = pts[first +- i] (i < m) as XYZZ, identities up to n; stream-ordered
int g1_xyzz_load(const G1Affine* pts, const uint8_t* inf, uint64_t first, bool rev, uint64_t m, uint64_t n,
                 G1xyzz* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_g1_load, dim3(cdiv(n, 256)), dim3(256), 0, stream, pts, inf, first, rev ? 1 : 0, m, n, out);
  PLK_HIP_TRY(hipGetLastError());
  return PLK_OK;
}

}  // namespace plk

using namespace plk;

extern "C" {

int plk_debug_g1_ntt(plk_ctx* ctx, const plk_g1* in, uint32_t log_n, int dir, plk_g1* out) {
  return plk_debug_g1_ntt_batch(ctx, in, log_n, 1, dir, out);
}

int plk_debug_g1_ntt_batch(plk_ctx* ctx, const plk_g1* in, uint32_t log_n, size_t batch, int dir, plk_g1* out) {
  PLK_API_BEGIN
  if (!ctx || !in || !out || log_n > 20 || (dir != 1 && dir != -1)) return PLK_E_ARG;
  if (batch == 0 || batch > ((size_t)1 << 20) >> log_n) return PLK_E_ARG;
  const uint64_t n = (uint64_t)batch << log_n;  // all the points
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  void* buf = nullptr;  // the ABI points, the XYZZ points, the affine results, prefix products, flags
  const size_t o_x = (n * sizeof(plk_g1) + 15) & ~(size_t)15, o_a = o_x + n * sizeof(G1xyzz), o_p = o_a + n * sizeof(G1Affine),
               o_f = o_p + n * sizeof(Fp), o_b = o_f + ((n + 15) & ~(size_t)15), total = o_b + 16;
  if (hipMallocAsync(&buf, total, s) != hipSuccess) return PLK_E_OOM;
  uint8_t* base = static_cast<uint8_t*>(buf);
  G1xyzz* pts = reinterpret_cast<G1xyzz*>(base + o_x);
  uint32_t bad = 0;
  std::vector<G1Affine> res(n);
  std::vector<uint8_t> rinf(n);
  int st = PLK_OK;
  hipError_t e = hipMemcpyAsync(base, in, n * sizeof(plk_g1), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(base + o_b, 0, 16, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_g1_load_abi, dim3(cdiv(n, 256)), dim3(256), 0, s, (const plk_g1*)base, n, pts,
                       reinterpret_cast<uint32_t*>(base + o_b));
    st = g1_ntt_run_batch(ctx, pts, log_n, batch, dir, s, true);
    if (st == PLK_OK)
      st = srs_batch_affine(pts, n, reinterpret_cast<Fp*>(base + o_p), reinterpret_cast<G1Affine*>(base + o_a),
                            base + o_f, s);
  }
  if (e == hipSuccess && st == PLK_OK)
    e = hipMemcpyAsync(res.data(), base + o_a, n * sizeof(G1Affine), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && st == PLK_OK) e = hipMemcpyAsync(rinf.data(), base + o_f, n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && st == PLK_OK) e = hipMemcpyAsync(&bad, base + o_b, sizeof bad, hipMemcpyDeviceToHost, s);
  (void)hipFreeAsync(buf, s);
  if (e == hipSuccess) e = stream_wait(s);
  if (e != hipSuccess) {
    last_hip_error() = e;
    return PLK_E_DEVICE;
  }
  if (st != PLK_OK) return st;
  if (bad) return PLK_E_ARG;
  for (uint64_t i = 0; i < n; ++i) g1_store(res[i].x, res[i].y, !rinf[i], &out[i]);
  return PLK_OK;
  PLK_API_END
}

}  // extern "C"
