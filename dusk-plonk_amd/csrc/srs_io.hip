// srs_io.hip — an SRS from bytes and its verification (include/plk.h "An SRS from bytes").
//
//  - plk_srs_load_bytes: the ceremony's bytes are uploaded and decoded one point per lane straight
//    into the SRS's device arrays (G1Affine limbs and the infinity bytes). The compressed form is
//    k_g1_decompress's per-lane function (ingest_math.hpp g1_decompress_words) in the SRS's layout;
//    the uncompressed form is g1_decode_raw_words: strict flags, then abi.hpp's byte swap, range
//    test and curve equation, Montgomery form. The item loads and the encoder's words are abi.hpp's. The subgroup test is g1_in_subgroup, as k_g1_subgroup.
//  - No status array: a rejecting lane folds (index << 8 | status) into one 64-bit word with an
//    atomic minimum, so the host reads 8 bytes whatever n is, and the smallest index wins. A
//    rejected point gets the infinity byte kRejected, which keeps the later kernels of the same
//    call off it.
//  - plk_srs_export_bytes: the inverse, k_srs_encode.
//  - plk_srs_fold / plk_srs_verify: weights from the verifier's rho kernel (verifier_replay.hip
//    k_fold_rho) on a root transcript of this unit, the two sums as one batch of two MSMs on the
//    SRS's own table (msm_run_batch), one host pairing check. No new MSM or pairing kernel.
//  - The opening key from bytes: host only, pairing_host.hpp g2_from_bytes / g2_to_bytes, then
//    plk_opening_key_load with all its checks.
//  - plk_srs_update / plk_srs_verify_update (include/plk.h "Updating an SRS"): the powers s^i on
//    the device, one scalar multiplication per point (g1_mul.hip), the opening key and the witness
//    [s]H on the host (g2_mul); the verification is plk_srs_verify plus one host pairing check on
//    the temporary key (H, witness).
#include <chrono>
#include <cstring>
#include <new>
#include <vector>

#include "ingest_math.hpp"
#include "internal.hpp"
#include "msm_common.hpp"
#include "pairing_host.hpp"
#include "transcript.hpp"
#include "verifier_replay.hpp"

using namespace plk;

namespace plk {
namespace {

constexpr size_t kG1Comp = 48, kG1Raw = 96;
constexpr size_t kMaxPoints = (size_t)1 << 26;  // plk_srs_load's bound
constexpr int kBlock = 64;                      // one wave, as the ingest kernels
constexpr uint8_t kRejected = 2;                // infinity byte of a point the decoder refused
constexpr uint8_t kBadPoint = 0xff;             // k_srs_validate's status (ingest.hip k_g1_validate)
constexpr unsigned long long kNoBad = ~0ull;

static_assert(sizeof(G1Affine) == 96, "SRS point layout");

// ---- shared math ------------------------------------------------------------------------------
// 96 uncompressed bytes as the 24 words read little-endian from memory -> Montgomery (x, y) or
// the identity. Returns a PLK_INGEST_* code; x, y are zero unless it is OK and finite.
PLK_HD uint8_t g1_decode_raw_words(const uint32_t (&w)[24], Fp& x, Fp& y, bool& inf) {
  x = fe_zero<FpCfg>();
  y = fe_zero<FpCfg>();
  inf = false;
  const uint32_t b0 = w[0] & 0xffu;
  if (b0 & 0xa0u) return PLK_INGEST_ENCODING;  // compressed bit or sort bit
  if (b0 & 0x40u) {  // infinity: 0x40 and 95 zero bytes, nothing else
    uint32_t rest = w[0] ^ 0x40u;
#pragma unroll
    for (int i = 1; i < 24; ++i) rest |= w[i];
    if (rest) return PLK_INGEST_ENCODING;
    inf = true;
    return PLK_INGEST_OK;
  }
  const Fp xc = fp_of_be_words(w), yc = fp_of_be_words(w + 12);  // the flag bits are all clear
  if (!fe_canonical(xc) || !fe_canonical(yc)) return PLK_INGEST_RANGE;
  const Fp xm = fe_to_mont(xc), ym = fe_to_mont(yc);
  if (!g1_on_curve(xm, ym)) return PLK_INGEST_OFF_CURVE;
  x = xm;
  y = ym;
  return PLK_INGEST_OK;
}

// ---- kernels ----------------------------------------------------------------------------------
__device__ __forceinline__ void report(unsigned long long* bad, uint64_t index, uint8_t status) {
  atomicMin(bad, (unsigned long long)((index << 8) | status));
}

__device__ __forceinline__ void st_decoded(uint64_t t, uint8_t st, const Fp& x, const Fp& y, bool is_inf,
                                           G1Affine* pts, uint8_t* inf, unsigned long long* bad) {
  st_aff(&pts[t], x, y);
  inf[t] = st != PLK_INGEST_OK ? kRejected : (is_inf ? 1 : 0);
  if (st != PLK_INGEST_OK) report(bad, t, st);
}

__global__ void __launch_bounds__(kBlock) k_srs_decompress(const uint8_t* __restrict__ in, uint64_t n,
                                                           G1Affine* __restrict__ pts,
                                                           uint8_t* __restrict__ inf,
                                                           unsigned long long* __restrict__ bad) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  uint32_t w[12];
  ld_words(in + t * kG1Comp, w);  // 16-B aligned: 48 t of a hipMalloc
  Fp x, y;
  bool is_inf;
  const uint8_t st = g1_decompress_words(w, x, y, is_inf);
  st_decoded(t, st, x, y, is_inf, pts, inf, bad);
}

__global__ void __launch_bounds__(kBlock) k_srs_decode_raw(const uint8_t* __restrict__ in, uint64_t n,
                                                           G1Affine* __restrict__ pts,
                                                           uint8_t* __restrict__ inf,
                                                           unsigned long long* __restrict__ bad) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  uint32_t w[24];
  ld_words(in + t * kG1Raw, w);
  Fp x, y;
  bool is_inf;
  const uint8_t st = g1_decode_raw_words(w, x, y, is_inf);
  st_decoded(t, st, x, y, is_inf, pts, inf, bad);
}

// finite points on the curve: a non-member reports PLK_INGEST_SUBGROUP; identities and rejected
// points are passed over
__global__ void __launch_bounds__(kBlock) k_srs_subgroup(const G1Affine* __restrict__ pts,
                                                         const uint8_t* __restrict__ inf, uint64_t n,
                                                         unsigned long long* __restrict__ bad) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n || inf[t] != 0) return;
  Fp x, y;
  ld_aff(&pts[t], x, y);
  if (!g1_in_subgroup(x, y)) report(bad, t, PLK_INGEST_SUBGROUP);
}

// the points of an SRS that came through plk_srs_load: a finite point with a non-canonical limb
// or off the curve reports kBadPoint (k_g1_validate's test)
__global__ void __launch_bounds__(kBlock) k_srs_validate(const G1Affine* __restrict__ pts,
                                                         const uint8_t* __restrict__ inf, uint64_t n,
                                                         unsigned long long* __restrict__ bad) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n || inf[t] != 0) return;
  Fp x, y;
  ld_aff(&pts[t], x, y);
  if (!g1_coords_valid(x, y)) report(bad, t, kBadPoint);
}

__global__ void __launch_bounds__(256) k_srs_scan_inf(const uint8_t* __restrict__ inf, uint64_t n,
                                                      unsigned long long* __restrict__ bad) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  if (inf[t] != 0) report(bad, t, 0);
}

// out of Montgomery, big-endian; compressed: abi.hpp g1_compress_words (the sort bit
// from y > (p-1)/2), uncompressed: x then y with 0x40 alone for the identity
__global__ void __launch_bounds__(kBlock) k_srs_encode(const G1Affine* __restrict__ pts,
                                                       const uint8_t* __restrict__ inf, uint64_t count,
                                                       int compressed, uint8_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= count) return;
  Fp x, y;
  ld_aff(&pts[t], x, y);
  const bool is_inf = inf[t] != 0;
  uint32_t w[24];
  if (compressed) {
    g1_compress_words(x, y, is_inf, w);
  } else {
    fp_to_be_words(x, w);
    fp_to_be_words(y, w + 12);
#pragma unroll
    for (int i = 0; i < 24; ++i) w[i] = is_inf ? (i == 0 ? 0x40u : 0u) : w[i];
  }
  uint4* dst = reinterpret_cast<uint4*>(out + t * (compressed ? kG1Comp : kG1Raw));
#pragma unroll
  for (int i = 0; i < 3; ++i) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
  if (!compressed) {
#pragma unroll
    for (int i = 3; i < 6; ++i) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
  }
}

// ---- host side --------------------------------------------------------------------------------
// the reduction word: cleared before a pass, read after it (the stream has been waited for)
struct BadWord {
  DevBuf d;
  int reset(hipStream_t s) {
    int st;
    if ((st = d.alloc(sizeof(unsigned long long)))) return st;
    PLK_HIP_TRY(hipMemsetAsync(d.ptr, 0xff, sizeof(unsigned long long), s));
    return PLK_OK;
  }
  unsigned long long* dev() const { return d.as<unsigned long long>(); }
  // false: nothing was reported
  int read(hipStream_t s, bool* any, uint64_t* index, uint8_t* status) {
    unsigned long long v = kNoBad;
    PLK_HIP_TRY(hipMemcpyAsync(&v, d.ptr, sizeof v, hipMemcpyDeviceToHost, s));
    PLK_HIP_TRY(stream_wait(s));
    *any = v != kNoBad;
    *index = (uint64_t)(v >> 8);
    *status = (uint8_t)(v & 0xff);
    return PLK_OK;
  }
};

// The root of the fold's weights: binds the label, the number of points and the seed. rho_i is
// drawn from a clone after append_u64("index", i) (k_fold_rho / rho_host; rho_0 = 1).
void fold_root(const uint8_t seed[32], uint64_t n, RhoPlan& plan) {
  Transcript t("plk-srs-fold");
  t.append_u64("n", n);
  t.append_message("seed", seed, 32);
  const Strobe128& s = t.strobe();
  rho_plan_compile(s.state(), s.pos(), s.pos_begin(), plan);
}

// the caller holds the device guard
int fold_run(plk_srs* s, const uint8_t* seed_or_null, plk_kzg_pair* out) {
  const size_t n = s->n;
  if (n == 1) {
    g1_store(fe_zero<FpCfg>(), fe_zero<FpCfg>(), false, &out->c);
    out->w = out->c;
    return PLK_OK;
  }
  uint8_t seed[32];
  if (seed_or_null) {
    std::memcpy(seed, seed_or_null, 32);
  } else {
    os_entropy(seed);
  }
  RhoPlan rho;
  fold_root(seed, n, rho);
  hipStream_t st = s->ctx->stream;
  // [0, rho_0 .. rho_(n-2), 0]: the first n are c's scalars (on g1[1 ..]), the last n are w's
  DevBuf d_sched, d_scal;
  int r;
  if ((r = d_sched.alloc(rho.sched.size() * sizeof(uint32_t)))) return r;
  if ((r = d_scal.alloc((n + 1) * sizeof(Fr)))) return r;
  PLK_HIP_TRY(hipMemcpyAsync(d_sched.ptr, rho.sched.data(), rho.sched.size() * sizeof(uint32_t),
                             hipMemcpyHostToDevice, st));
  PLK_HIP_TRY(hipMemsetAsync(d_scal.ptr, 0, (n + 1) * sizeof(Fr), st));
  if ((r = rho_launch(st, rho.root, d_sched.as<uint32_t>(), rho.blocks, (uint32_t)(n - 1),
                      d_scal.as<Fr>() + 1, 1)))
    return r;
  const Fr* ptrs[2] = {d_scal.as<Fr>(), d_scal.as<Fr>() + 1};
  const size_t lens[2] = {n, n};
  plk_g1 outs[2];
  int statuses[2] = {PLK_OK, PLK_OK};
  if ((r = msm_run_batch(s, *s->ws, ptrs, lens, lens, 2, outs, statuses, st))) return r;
  PLK_HIP_TRY(stream_wait(st));  // d_sched / d_scal are freed on return
  out->c = outs[0];
  out->w = outs[1];
  return PLK_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---- updating an SRS --------------------------------------------------------------------------
// s: canonical Montgomery, not zero
bool update_scalar_ok(const Fr& s) { return fe_canonical(s) && !fe_is_zero(s); }

// 64 bytes of OS entropy reduced mod r (Montgomery form), redrawn on zero
void fr_from_entropy(Fr& out) {
  uint8_t buf[64];
  Fr lo, hi;
  do {
    os_entropy(buf);
    os_entropy(buf + 32);
    for (int i = 0; i < 8; ++i) {
      std::memcpy(&lo.v[i], buf + 4 * i, 4);
      std::memcpy(&hi.v[i], buf + 32 + 4 * i, 4);
    }
    fe_reduce_once(lo);  // 2^256 < 3 r: two subtractions bring a 256-bit value below r
    fe_reduce_once(lo);
    fe_reduce_once(hi);
    fe_reduce_once(hi);
    // lo + hi 2^256: fe_one's words are 2^256 mod r as a plain value
    out = fe_add(fe_to_mont(lo), fe_mul(fe_to_mont(hi), fe_to_mont(fe_one<FrCfg>())));
  } while (fe_is_zero(out));
  explicit_bzero(buf, sizeof buf);
  explicit_bzero(&lo, sizeof lo);
  explicit_bzero(&hi, sizeof hi);
}

// a device array that held secrets: overwritten before it is freed (best effort)
struct SecretDevBuf {
  DevBuf d;
  hipStream_t s = nullptr;
  ~SecretDevBuf() {
    if (!d.ptr) return;
    (void)hipMemsetAsync(d.ptr, 0, d.bytes, s);
    (void)stream_wait(s);
  }
};

struct KeyHolder {  // destroys the key unless it was released
  plk_opening_key* k = nullptr;
  ~KeyHolder() {
    if (k) (void)plk_opening_key_destroy(k);
  }
  plk_opening_key* release() {
    plk_opening_key* r = k;
    k = nullptr;
    return r;
  }
};

// the canonical / on-curve pass and the subgroup kernel over an SRS not yet known to be in G1
// (plk_srs_verify's first two steps): *any with the smallest offending index, flags set on success
int srs_ensure_g1(plk_srs* srs, bool* any, uint64_t* idx) {
  hipStream_t s = srs->ctx->stream;
  const uint64_t n = srs->n;
  const G1Affine* pts = srs->points.as<G1Affine>();
  const uint8_t* inf = srs->inf.as<uint8_t>();
  BadWord bad;
  uint8_t code;
  int st;
  *any = false;
  if (!srs->points_checked) {
    if ((st = bad.reset(s))) return st;
    hipLaunchKernelGGL(k_srs_validate, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, pts, inf, n, bad.dev());
    PLK_HIP_TRY(hipGetLastError());
    if ((st = bad.read(s, any, idx, &code))) return st;
    if (*any) return PLK_OK;
    srs->points_checked = true;
  }
  if (!srs->subgroup_checked) {
    if ((st = bad.reset(s))) return st;
    hipLaunchKernelGGL(k_srs_subgroup, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, pts, inf, n, bad.dev());
    PLK_HIP_TRY(hipGetLastError());
    if ((st = bad.read(s, any, idx, &code))) return st;
    if (*any) return PLK_OK;
    srs->subgroup_checked = true;
  }
  return PLK_OK;
}

}  // namespace

// The same two passes over the first n points only (plk_kzg_open_domain, which reads no others).
// A clean pass is recorded in g1_prefix; the flags of the whole SRS are srs_ensure_g1's.
int srs_ensure_g1_prefix(plk_srs* srs, uint64_t n, bool* any, uint64_t* idx) {
  *any = false;
  if (srs->subgroup_checked || srs->g1_prefix >= n) return PLK_OK;
  if (n > srs->n) return PLK_E_ARG;
  hipStream_t s = srs->ctx->stream;
  const G1Affine* pts = srs->points.as<G1Affine>();
  const uint8_t* inf = srs->inf.as<uint8_t>();
  BadWord bad;
  uint8_t code;
  int st;
  if (!srs->points_checked) {
    if ((st = bad.reset(s))) return st;
    hipLaunchKernelGGL(k_srs_validate, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, pts, inf, n, bad.dev());
    PLK_HIP_TRY(hipGetLastError());
    if ((st = bad.read(s, any, idx, &code))) return st;
    if (*any) return PLK_OK;
  }
  if ((st = bad.reset(s))) return st;
  hipLaunchKernelGGL(k_srs_subgroup, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, pts, inf, n, bad.dev());
  PLK_HIP_TRY(hipGetLastError());
  if ((st = bad.read(s, any, idx, &code))) return st;
  if (*any) return PLK_OK;
  srs->g1_prefix = n;
  return PLK_OK;
}

}  // namespace plk

extern "C" {

int plk_srs_load_bytes(plk_ctx* ctx, const uint8_t* in, size_t n_points, int format, int check_subgroup,
                       plk_srs** out, uint64_t* bad_index, uint8_t* bad_status) {
  PLK_API_BEGIN
  if (!out) return PLK_E_ARG;
  *out = nullptr;
  if (!ctx || !in || n_points == 0 || n_points > kMaxPoints) return PLK_E_ARG;
  if (format != PLK_G1_COMPRESSED && format != PLK_G1_UNCOMPRESSED) return PLK_E_ARG;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const uint64_t n = n_points;
  const size_t bytes = n_points * (format == PLK_G1_COMPRESSED ? kG1Comp : kG1Raw);
  std::unique_ptr<plk_srs> srs;
  TimingEvents<4> ev;
  BadWord bad;
  int st;
  if ((st = srs_new(ctx, n_points, srs))) return st;
  if ((st = ev.create())) return st;
  {
    DevBuf d_in;  // freed before the table is built
    if ((st = d_in.alloc(bytes))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(d_in.ptr, in, bytes, hipMemcpyHostToDevice, s));
    if ((st = bad.reset(s))) return st;
    G1Affine* pts = srs->points.as<G1Affine>();
    uint8_t* inf = srs->inf.as<uint8_t>();
    PLK_HIP_TRY(hipEventRecord(ev.e[0], s));
    if (format == PLK_G1_COMPRESSED) {
      hipLaunchKernelGGL(k_srs_decompress, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s,
                         (const uint8_t*)d_in.as<uint8_t>(), n, pts, inf, bad.dev());
    } else {
      hipLaunchKernelGGL(k_srs_decode_raw, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s,
                         (const uint8_t*)d_in.as<uint8_t>(), n, pts, inf, bad.dev());
    }
    PLK_HIP_TRY(hipEventRecord(ev.e[1], s));
    if (check_subgroup) {
      PLK_HIP_TRY(hipEventRecord(ev.e[2], s));
      hipLaunchKernelGGL(k_srs_subgroup, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, (const G1Affine*)pts,
                         (const uint8_t*)inf, n, bad.dev());
      PLK_HIP_TRY(hipEventRecord(ev.e[3], s));
    }
    PLK_HIP_TRY(hipGetLastError());
    bool any;
    uint64_t idx;
    uint8_t code;
    if ((st = bad.read(s, &any, &idx, &code))) return st;
    ctx->srs_decode_ms = ctx->srs_subgroup_ms = 0.f;
    (void)hipEventElapsedTime(&ctx->srs_decode_ms, ev.e[0], ev.e[1]);
    if (check_subgroup) (void)hipEventElapsedTime(&ctx->srs_subgroup_ms, ev.e[2], ev.e[3]);
    if (any) {
      if (bad_index) *bad_index = idx;
      if (bad_status) *bad_status = code;
      return PLK_E_ARG;
    }
  }
  srs->points_checked = true;
  srs->subgroup_checked = check_subgroup != 0;
  if ((st = srs_complete(srs.get()))) return st;
  *out = srs.release();
  return PLK_OK;
  PLK_API_END
}

int plk_srs_last_load_ms(plk_ctx* ctx, float* decode_ms, float* subgroup_ms) {
  if (!ctx) return PLK_E_ARG;
  if (decode_ms) *decode_ms = ctx->srs_decode_ms;
  if (subgroup_ms) *subgroup_ms = ctx->srs_subgroup_ms;
  return PLK_OK;
}

int plk_srs_export_bytes(const plk_srs* srs, size_t start, size_t count, int format, uint8_t* out) {
  PLK_API_BEGIN
  if (!srs || (!out && count) || start > srs->n || count > srs->n - start) return PLK_E_ARG;
  if (format != PLK_G1_COMPRESSED && format != PLK_G1_UNCOMPRESSED) return PLK_E_ARG;
  if (!count) return PLK_OK;
  DeviceGuard g(srs->ctx->device);
  hipStream_t s = srs->ctx->stream;
  const size_t bytes = count * (format == PLK_G1_COMPRESSED ? kG1Comp : kG1Raw);
  DevBuf d_out;
  int st;
  if ((st = d_out.alloc(bytes))) return st;
  hipLaunchKernelGGL(k_srs_encode, dim3(cdiv(count, kBlock)), dim3(kBlock), 0, s,
                     (const G1Affine*)srs->points.as<G1Affine>() + start,
                     (const uint8_t*)srs->inf.as<uint8_t>() + start, (uint64_t)count,
                     format == PLK_G1_COMPRESSED ? 1 : 0, d_out.as<uint8_t>());
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipMemcpyAsync(out, d_out.ptr, bytes, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  return PLK_OK;
  PLK_API_END
}

int plk_srs_fold(plk_srs* srs, const uint8_t seed[32], plk_kzg_pair* out) {
  PLK_API_BEGIN
  if (!srs || !out) return PLK_E_ARG;
  DeviceGuard g(srs->ctx->device);
  return fold_run(srs, seed, out);
  PLK_API_END
}

int plk_srs_verify(plk_ctx* ctx, plk_srs* srs, const plk_opening_key* key, const uint8_t seed[32],
                   int* verdict, uint64_t* bad_index) {
  PLK_API_BEGIN
  if (!ctx || !srs || !key || !verdict || srs->ctx != ctx) return PLK_E_ARG;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const uint64_t n = srs->n;
  const G1Affine* pts = srs->points.as<G1Affine>();
  const uint8_t* inf = srs->inf.as<uint8_t>();
  BadWord bad;
  bool any;
  uint64_t idx;
  uint8_t code;
  int st;
  auto fail = [&](int cls) {
    *verdict = cls;
    if (bad_index) *bad_index = idx;
    return PLK_OK;
  };
  if (!srs->points_checked) {
    if ((st = bad.reset(s))) return st;
    hipLaunchKernelGGL(k_srs_validate, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, pts, inf, n, bad.dev());
    PLK_HIP_TRY(hipGetLastError());
    if ((st = bad.read(s, &any, &idx, &code))) return st;
    if (any) return fail(PLK_SRS_POINT);
    srs->points_checked = true;
  }
  if (!srs->subgroup_checked) {
    if ((st = bad.reset(s))) return st;
    hipLaunchKernelGGL(k_srs_subgroup, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, pts, inf, n, bad.dev());
    PLK_HIP_TRY(hipGetLastError());
    if ((st = bad.read(s, &any, &idx, &code))) return st;
    if (any) return fail(PLK_SRS_SUBGROUP);
    srs->subgroup_checked = true;
  }
  if (srs->has_inf) {  // srs_finish's flag: no identity anywhere otherwise
    if ((st = bad.reset(s))) return st;
    hipLaunchKernelGGL(k_srs_scan_inf, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, inf, n, bad.dev());
    PLK_HIP_TRY(hipGetLastError());
    if ((st = bad.read(s, &any, &idx, &code))) return st;
    if (any) return fail(PLK_SRS_INFINITY);
  }
  G1Affine first;
  PLK_HIP_TRY(hipMemcpyAsync(&first, pts, sizeof first, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  G1Affine gen;
  g1_generator(gen.x, gen.y);
  if (!fe_eq(first.x, gen.x) || !fe_eq(first.y, gen.y)) {
    *verdict = PLK_SRS_GENERATOR;
    return PLK_OK;
  }
  plk_kzg_pair pair;
  auto t0 = std::chrono::steady_clock::now();
  if ((st = fold_run(srs, seed, &pair))) return st;
  srs->verify_fold_ms = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  int ok = 0;
  if ((st = plk_pairing_check(key, &pair, &ok))) return st;
  srs->verify_pairing_ms = ms_since(t0);
  *verdict = ok ? PLK_SRS_OK : PLK_SRS_CHAIN;
  return PLK_OK;
  PLK_API_END
}

int plk_srs_last_verify_ms(const plk_srs* srs, double* fold_ms, double* pairing_ms) {
  if (!srs) return PLK_E_ARG;
  if (fold_ms) *fold_ms = srs->verify_fold_ms;
  if (pairing_ms) *pairing_ms = srs->verify_pairing_ms;
  return PLK_OK;
}

int plk_debug_srs_weights(plk_ctx* ctx, const uint8_t seed[32], size_t n, plk_fr* out) {
  PLK_API_BEGIN
  if (!seed || n == 0 || n > kMaxPoints || (!out && n > 1)) return PLK_E_ARG;
  if (n == 1) return PLK_OK;
  const size_t count = n - 1;
  RhoPlan rho;
  fold_root(seed, n, rho);
  std::vector<Fr> w(count);
  if (!ctx) {
    for (size_t i = 0; i < count; ++i) w[i] = rho_host(rho, (uint32_t)i);
  } else {
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    DevBuf d_sched, d_out;
    int st;
    if ((st = d_sched.alloc(rho.sched.size() * sizeof(uint32_t)))) return st;
    if ((st = d_out.alloc(count * sizeof(Fr)))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(d_sched.ptr, rho.sched.data(), rho.sched.size() * sizeof(uint32_t),
                               hipMemcpyHostToDevice, s));
    if ((st = rho_launch(s, rho.root, d_sched.as<uint32_t>(), rho.blocks, (uint32_t)count, d_out.as<Fr>(), 1)))
      return st;
    PLK_HIP_TRY(hipMemcpyAsync(w.data(), d_out.ptr, count * sizeof(Fr), hipMemcpyDeviceToHost, s));
    PLK_HIP_TRY(stream_wait(s));
  }
  for (size_t i = 0; i < count; ++i) out[i] = fr_to_abi(w[i]);
  return PLK_OK;
  PLK_API_END
}

// ---- the opening key from bytes (host only) ---------------------------------------------------
int plk_opening_key_load_bytes(const uint8_t* h, const uint8_t* beta_h, int format, plk_opening_key** out) {
  PLK_API_BEGIN
  if (!out) return PLK_E_ARG;
  *out = nullptr;
  if (!h || !beta_h || (format != PLK_G1_COMPRESSED && format != PLK_G1_UNCOMPRESSED)) return PLK_E_ARG;
  const bool comp = format == PLK_G1_COMPRESSED;
  G2Aff a, b;
  int st;
  if ((st = g2_from_bytes(h, comp, a)) || (st = g2_from_bytes(beta_h, comp, b))) return st;
  plk_g2 pa, pb;  // an identity goes on as infinity = 1, which plk_opening_key_load refuses
  g2_to_abi(a, &pa);
  g2_to_abi(b, &pb);
  return plk_opening_key_load(&pa, &pb, out);
  PLK_API_END
}

int plk_opening_key_to_bytes(const plk_opening_key* key, int format, uint8_t* h, uint8_t* beta_h) {
  PLK_API_BEGIN
  if (!key || (format != PLK_G1_COMPRESSED && format != PLK_G1_UNCOMPRESSED)) return PLK_E_ARG;
  const bool comp = format == PLK_G1_COMPRESSED;
  plk_g2 pa, pb;
  int st;
  if ((st = plk_opening_key_points(key, &pa, &pb))) return st;
  G2Aff a, b;
  if ((st = g2_from_abi(pa, a)) || (st = g2_from_abi(pb, b))) return st;
  if (h) g2_to_bytes(a, comp, h);
  if (beta_h) g2_to_bytes(b, comp, beta_h);
  return PLK_OK;
  PLK_API_END
}

int plk_debug_f2_sqrt(const uint64_t* a, uint64_t* out, int* is_square) {
  PLK_API_BEGIN
  if (!a || !out || !is_square) return PLK_E_ARG;
  const Fp2 v = {fe_of_abi<FpCfg>(a), fe_of_abi<FpCfg>(a + 6)};
  if (!fe_canonical(v.c0) || !fe_canonical(v.c1)) return PLK_E_ARG;
  Fp2 r;
  *is_square = f2_sqrt(v, r) ? 1 : 0;
  fe_to_abi(r.c0, out);
  fe_to_abi(r.c1, out + 6);
  return PLK_OK;
  PLK_API_END
}

// ---- updating an SRS --------------------------------------------------------------------------
int plk_opening_key_update(const plk_opening_key* key, const plk_fr* s, plk_opening_key** out, plk_g2* witness) {
  PLK_API_BEGIN
  if (!out) return PLK_E_ARG;
  *out = nullptr;
  if (!key || !s || !witness) return PLK_E_ARG;
  const Fr sm = fr_from_abi(*s);
  if (!update_scalar_ok(sm)) return PLK_E_ARG;
  plk_g2 ph, pb;
  G2Aff h, bh;
  int st;
  if ((st = plk_opening_key_points(key, &ph, &pb))) return st;
  if ((st = g2_from_abi(ph, h)) || (st = g2_from_abi(pb, bh))) return st;
  Fr plain = fe_from_mont(sm);
  const G2Aff nb = g2_mul(bh, plain.v, 8), w = g2_mul(h, plain.v, 8);
  explicit_bzero(&plain, sizeof plain);
  plk_g2 pnb;
  g2_to_abi(nb, &pnb);
  if ((st = plk_opening_key_load(&ph, &pnb, out))) return st;
  g2_to_abi(w, witness);
  return PLK_OK;
  PLK_API_END
}

int plk_srs_update(plk_srs* srs, const plk_opening_key* key, const plk_fr* s, plk_srs** out_srs,
                   plk_opening_key** out_key, plk_g2* witness, uint64_t* bad_index) {
  PLK_API_BEGIN
  if (!out_srs || !out_key) return PLK_E_ARG;
  *out_srs = nullptr;
  *out_key = nullptr;
  if (!srs || !key || !witness || srs->n < 2) return PLK_E_ARG;
  Fr sm;
  if (s) {
    sm = fr_from_abi(*s);
    if (!update_scalar_ok(sm)) return PLK_E_ARG;
  } else {
    fr_from_entropy(sm);
  }
  struct Wipe {  // the host copies of the secret, on every way out
    Fr& a;
    plk_fr& b;
    ~Wipe() {
      explicit_bzero(&a, sizeof a);
      explicit_bzero(&b, sizeof b);
    }
  };
  plk_fr s_abi;
  Wipe wipe{sm, s_abi};
  s_abi = fr_to_abi(sm);
  plk_ctx* ctx = srs->ctx;
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const uint64_t n = srs->n;
  int r;
  bool any;
  uint64_t idx;
  if ((r = srs_ensure_g1(srs, &any, &idx))) return r;  // the split of g1_mul.hip holds on G1 only
  if (any) {
    if (bad_index) *bad_index = idx;
    return PLK_E_ARG;
  }
  KeyHolder nk;
  if ((r = plk_opening_key_update(key, &s_abi, &nk.k, witness))) return r;
  std::unique_ptr<plk_srs> ns;
  if ((r = srs_new(ctx, srs->n, ns))) return r;
  {
    SecretDevBuf pow;  // s^i, i < n
    pow.s = st;
    if ((r = pow.d.alloc(n * sizeof(Fr)))) return r;
    if ((r = fr_powers_dev(sm, n, pow.d.as<Fr>(), st))) return r;
    if ((r = g1_mul_dev(ctx, srs->points.as<G1Affine>(), srs->inf.as<uint8_t>(), pow.d.as<Fr>(), n,
                        ns->points.as<G1Affine>(), ns->inf.as<uint8_t>(), st)))
      return r;
  }
  ns->points_checked = ns->subgroup_checked = true;  // multiples of points of G1
  if ((r = srs_complete(ns.get()))) return r;
  *out_srs = ns.release();
  *out_key = nk.release();
  return PLK_OK;
  PLK_API_END
}

int plk_srs_verify_update(plk_ctx* ctx, const plk_g1* prev_tau_g1, plk_srs* new_srs, const plk_opening_key* new_key,
                          const plk_g2* witness, const uint8_t seed[32], int* verdict, uint64_t* bad_index) {
  PLK_API_BEGIN
  if (!ctx || !prev_tau_g1 || !new_srs || !new_key || !witness || !verdict) return PLK_E_ARG;
  if (new_srs->ctx != ctx || new_srs->n < 2) return PLK_E_ARG;
  // the witness as the beta_h of a temporary key on the same H: plk_opening_key_load refuses what
  // is not canonical, off the twist, outside the r-torsion or the identity
  plk_g2 ph;
  KeyHolder tk;
  int st;
  if ((st = plk_opening_key_points(new_key, &ph, nullptr))) return st;
  st = plk_opening_key_load(&ph, witness, &tk.k);
  if (st == PLK_E_ARG) {
    *verdict = PLK_SRS_WITNESS;
    return PLK_OK;
  }
  if (st) return st;
  int v = PLK_SRS_OK;
  if ((st = plk_srs_verify(ctx, new_srs, new_key, seed, &v, bad_index))) return st;
  if (v != PLK_SRS_OK) {
    *verdict = v;
    return PLK_OK;
  }
  // e(new g1[1], H) == e(prev g1[1], [s]H)
  *verdict = PLK_SRS_LINK;
  G1In prev;
  if (g1_from_abi(*prev_tau_g1, prev) != PLK_OK || prev.inf || !g1_in_subgroup(prev.x, prev.y)) return PLK_OK;
  plk_kzg_pair pair;
  if ((st = plk_srs_points(new_srs, 1, 1, &pair.c))) return st;
  pair.w = *prev_tau_g1;
  int ok = 0;
  if ((st = plk_pairing_check(tk.k, &pair, &ok))) return st;
  if (ok) *verdict = PLK_SRS_OK;
  return PLK_OK;
  PLK_API_END
}

int plk_g2_to_bytes(const plk_g2* q, int format, uint8_t* out) {
  PLK_API_BEGIN
  if (!q || !out || (format != PLK_G1_COMPRESSED && format != PLK_G1_UNCOMPRESSED)) return PLK_E_ARG;
  G2Aff a = g2_infinity();
  int st;
  if (q->infinity != 1 && (st = g2_from_abi(*q, a))) return st;
  g2_to_bytes(a, format == PLK_G1_COMPRESSED, out);
  return PLK_OK;
  PLK_API_END
}

int plk_g2_from_bytes(const uint8_t* in, int format, plk_g2* out) {
  PLK_API_BEGIN
  if (!in || !out || (format != PLK_G1_COMPRESSED && format != PLK_G1_UNCOMPRESSED)) return PLK_E_ARG;
  G2Aff a;
  int st;
  if ((st = g2_from_bytes(in, format == PLK_G1_COMPRESSED, a))) return st;
  g2_to_abi(a, out);
  return PLK_OK;
  PLK_API_END
}

}  // extern "C"
