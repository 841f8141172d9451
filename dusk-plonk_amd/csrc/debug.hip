// debug.hip — test hooks: elementwise device arithmetic on host arrays for the parity tests.
// plk_debug_field_op: the packed field of ff.hpp; plk_debug_rx_op: the redundant-limb field of
// ffr.hpp on raw limb rows; plk_debug_ntt_lazy_op: the NTT pass' lazy butterfly helpers (the
// kernel is in ntt.hip); plk_debug_g1r_op: the XYZZ group law of g1r.hpp on raw limb rows;
// plk_debug_block_eval: the prover's forward block transform onto a key's quotient domain;
// plk_debug_prover_stage: one pk_* launcher of prover_kernels.hip on caller arrays;
// plk_debug_msm_snapshot: one fixed-base MSM batch and what it left in its workspace.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "g1r.hpp"
#include "internal.hpp"
#include "msm_common.hpp"
#include "prover.hpp"

namespace plk {
namespace {

template <class C>
__global__ void k_field_op(int op, const Fe<C>* __restrict__ a, const Fe<C>* __restrict__ b,
                           Fe<C>* __restrict__ out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe<C> x = a[i], y = b[i];
  Fe<C> r;
  switch (op) {
    case 0: r = fe_mul(x, y); break;
    case 1: r = fe_add(x, y); break;
    case 2: r = fe_sub(x, y); break;
    case 3: r = fe_sqr(x); break;
    default: r = fe_inv(x); break;
  }
  out[i] = r;
}

template <class C>
int run(plk_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  const size_t bytes = n * sizeof(Fe<C>);
  DevBuf da, db, dout;
  int st;
  if ((st = da.alloc(bytes)) || (st = db.alloc(bytes)) || (st = dout.alloc(bytes))) return st;
  hipStream_t s = ctx->stream;
  PLK_HIP_TRY(hipMemcpyAsync(da.ptr, a, bytes, hipMemcpyHostToDevice, s));
  PLK_HIP_TRY(hipMemcpyAsync(db.ptr, b ? b : a, bytes, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_field_op<C>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, op,
                     da.as<Fe<C>>(), db.as<Fe<C>>(), dout.as<Fe<C>>(), (uint64_t)n);
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipMemcpyAsync(out, dout.ptr, bytes, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  return PLK_OK;
}

// ---- plk_debug_rx_op: ffr.hpp on raw limb rows ------------------------------------------
// One kernel instantiation per op (the op is a template argument: a run-time switch over
// values of this size is merged through a scratch object, ntt.hip r4_math). Op codes as in
// include/plk.h; 100 + CP: rx_sub_u<CP>, 200 + CP: rx_sub_n<CP>.
enum : int {
  kOpMul = 0, kOpSqr, kOpMulAdd, kOpMul2, kOpMul2Asm, kOpSqr2, kOpSqr2Asm, kOpMulAddMul2,
  kOpMulAddMul2Asm, kOpMul3, kOpAdd, kOpSub, kOpSubLazy, kOpSub2N6, kOpSmall2, kOpSmall3,
  kOpCanon, kOpIsZero, kOpIsZeroU, kOpUnpackPack, kOpSubU = 100, kOpSubN = 200
};

constexpr int rx_op_nin(int op) {
  if (op >= kOpSubU) return 2;
  switch (op) {
    case kOpSqr: case kOpSmall2: case kOpSmall3: case kOpCanon: case kOpIsZero: case kOpIsZeroU:
    case kOpUnpackPack: return 1;
    case kOpMul: case kOpSqr2: case kOpSqr2Asm: case kOpAdd: case kOpSub: case kOpSubLazy: return 2;
    case kOpSub2N6: return 3;
    default: return 4;
  }
}
constexpr int rx_op_nout(int op) {
  switch (op) {
    case kOpMul2: case kOpMul2Asm: case kOpSqr2: case kOpSqr2Asm: case kOpUnpackPack: return 2;
    case kOpMulAddMul2: case kOpMulAddMul2Asm: case kOpMul3: return 3;
    default: return 1;
  }
}

template <class C>
__device__ __forceinline__ Rx<C> ld_row(const uint32_t* __restrict__ p, uint64_t i) {
  Rx<C> r;
#pragma unroll
  for (int k = 0; k < RxShape<C>::L; ++k) r.v[k] = p[i * RxShape<C>::L + k];
  return r;
}
template <class C>
__device__ __forceinline__ void st_row(uint32_t* __restrict__ p, uint64_t i, const Rx<C>& r) {
#pragma unroll
  for (int k = 0; k < RxShape<C>::L; ++k) p[i * RxShape<C>::L + k] = r.v[k];
}
template <class C>
__device__ __forceinline__ Rx<C> rx_flag(bool f) {
  Rx<C> r = rx_zero<C>();
  r.v[0] = f ? 1u : 0u;
  return r;
}

template <class C, int OP>
__global__ void __launch_bounds__(256)
    k_rx_op(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
            const uint32_t* __restrict__ c, const uint32_t* __restrict__ d,
            uint32_t* __restrict__ out, uint64_t n) {
  constexpr int NIN = rx_op_nin(OP), NOUT = rx_op_nout(OP);
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Rx<C> x0 = ld_row<C>(a, i);
  const Rx<C> x1 = NIN > 1 ? ld_row<C>(b, i) : rx_zero<C>();
  const Rx<C> x2 = NIN > 2 ? ld_row<C>(c, i) : rx_zero<C>();
  const Rx<C> x3 = NIN > 3 ? ld_row<C>(d, i) : rx_zero<C>();
  Rx<C> o0 = rx_zero<C>(), o1 = rx_zero<C>(), o2 = rx_zero<C>();
  if constexpr (OP == kOpMul) o0 = rx_mul(x0, x1);
  else if constexpr (OP == kOpSqr) o0 = rx_sqr(x0);
  else if constexpr (OP == kOpMulAdd) o0 = rx_mul_add(x0, x1, x2, x3);
  else if constexpr (OP == kOpMul2) rx_mul2<C, false>(x0, x1, x2, x3, o0, o1);
  else if constexpr (OP == kOpMul2Asm) rx_mul2<C, true>(x0, x1, x2, x3, o0, o1);
  else if constexpr (OP == kOpSqr2) rx_sqr2<C, false>(x0, x1, o0, o1);
  else if constexpr (OP == kOpSqr2Asm) rx_sqr2<C, true>(x0, x1, o0, o1);
  else if constexpr (OP == kOpMulAddMul2) rx_mul_add_mul2<C, false>(x0, x1, x2, x3, x0, x3, x2, x1, o0, o1, o2);
  else if constexpr (OP == kOpMulAddMul2Asm) rx_mul_add_mul2<C, true>(x0, x1, x2, x3, x0, x3, x2, x1, o0, o1, o2);
  else if constexpr (OP == kOpMul3) rx_mul3<C>(x0, x1, x2, x3, x3, x0, o0, o1, o2);
  else if constexpr (OP == kOpAdd) o0 = rx_add(x0, x1);
  else if constexpr (OP == kOpSub) o0 = rx_sub(x0, x1);
  else if constexpr (OP == kOpSubLazy) o0 = rx_sub_lazy(x0, x1);
  else if constexpr (OP == kOpSub2N6) o0 = rx_sub2_n<C, 6>(x0, x1, x2);
  else if constexpr (OP == kOpSmall2) o0 = rx_small_mul_n<C, 2>(x0);
  else if constexpr (OP == kOpSmall3) o0 = rx_small_mul_n<C, 3>(x0);
  else if constexpr (OP == kOpCanon) o0 = rx_canon(x0);
  else if constexpr (OP == kOpIsZero) o0 = rx_flag<C>(rx_is_zero(x0));
  else if constexpr (OP == kOpIsZeroU) o0 = rx_flag<C>(rx_is_zero_u(x0));
  else if constexpr (OP == kOpUnpackPack) {
    Fe<C> w;
#pragma unroll
    for (int k = 0; k < C::N; ++k) w.v[k] = x0.v[k];
    o0 = rx_unpack(w);
    w = rx_pack(o0);
#pragma unroll
    for (int k = 0; k < C::N; ++k) o1.v[k] = w.v[k];
  } else if constexpr (OP >= kOpSubN) o0 = rx_sub_n<C, OP - kOpSubN>(x0, x1);
  else o0 = rx_sub_u<C, OP - kOpSubU>(x0, x1);
  st_row<C>(out, i * NOUT, o0);
  if constexpr (NOUT > 1) st_row<C>(out, i * NOUT + 1, o1);
  if constexpr (NOUT > 2) st_row<C>(out, i * NOUT + 2, o2);
}

using RxKernel = void (*)(const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                          uint32_t*, uint64_t);
#define PLK_RX_CASE(C, OP) \
  case OP: return k_rx_op<C, OP>;
#define PLK_RX_COMMON(C)                                                                       \
  PLK_RX_CASE(C, kOpMul) PLK_RX_CASE(C, kOpSqr) PLK_RX_CASE(C, kOpMulAdd) PLK_RX_CASE(C, kOpMul2) \
  PLK_RX_CASE(C, kOpMul2Asm) PLK_RX_CASE(C, kOpSqr2) PLK_RX_CASE(C, kOpMulAddMul2)             \
  PLK_RX_CASE(C, kOpMul3) PLK_RX_CASE(C, kOpAdd) PLK_RX_CASE(C, kOpSub) PLK_RX_CASE(C, kOpSubLazy) \
  PLK_RX_CASE(C, kOpSub2N6) PLK_RX_CASE(C, kOpSmall2) PLK_RX_CASE(C, kOpSmall3)                \
  PLK_RX_CASE(C, kOpCanon) PLK_RX_CASE(C, kOpIsZero) PLK_RX_CASE(C, kOpIsZeroU)                \
  PLK_RX_CASE(C, kOpUnpackPack) PLK_RX_CASE(C, kOpSubU + 3) PLK_RX_CASE(C, kOpSubU + 5)        \
  PLK_RX_CASE(C, kOpSubU + 6) PLK_RX_CASE(C, kOpSubN + 3) PLK_RX_CASE(C, kOpSubN + 5)          \
  PLK_RX_CASE(C, kOpSubN + 6)
RxKernel rx_kernel(int field, int op) {
  if (field == 0) {
    switch (op) {
      PLK_RX_COMMON(FrCfg)
      default: return nullptr;
    }
  }
  switch (op) {
    PLK_RX_COMMON(FpCfg)
    PLK_RX_CASE(FpCfg, kOpSqr2Asm) PLK_RX_CASE(FpCfg, kOpMulAddMul2Asm)
    PLK_RX_CASE(FpCfg, kOpSubU + 4) PLK_RX_CASE(FpCfg, kOpSubU + 10)
    PLK_RX_CASE(FpCfg, kOpSubN + 4) PLK_RX_CASE(FpCfg, kOpSubN + 10)
    default: return nullptr;
  }
}
#undef PLK_RX_COMMON
#undef PLK_RX_CASE

// ---- plk_debug_g1r_op: g1r.hpp on raw XYZZ limb rows -------------------------------------
enum : int {
  kG1Madd000 = 0, kG1Madd100, kG1Madd110, kG1Madd111, kG1MaddLazy, kG1AddLazy, kG1AddQuad,
  kG1DblLazy, kG1LazyFinish, kG1Add, kG1AddAffine, kG1Dbl, kG1DblAffine, kG1OpCount
};
constexpr int kG1Row = 4 * RxShape<FpCfg>::L;
constexpr bool g1_op_needs_q(int op) {
  return !(op == kG1DblLazy || op == kG1LazyFinish || op == kG1Dbl || op == kG1DblAffine);
}

__device__ __forceinline__ G1R ld_g1row(const uint32_t* __restrict__ p, uint64_t i) {
  G1R r;
  r.X = ld_row<FpCfg>(p, 4 * i);
  r.Y = ld_row<FpCfg>(p, 4 * i + 1);
  r.ZZ = ld_row<FpCfg>(p, 4 * i + 2);
  r.ZZZ = ld_row<FpCfg>(p, 4 * i + 3);
  return r;
}

// k_accumulate's sequence around the straight-line mixed addition (msm_acc.hip)
template <bool GROUPED, bool ASM, bool PAIRS>
__device__ __forceinline__ G1R madd_as_accumulate(const G1R& acc, const G1R& q, bool neg) {
  RFp y = q.Y;
  if (neg) y = rx_neg_lazy(y);
  const bool was_inf = g1r_is_inf(acc);
  G1R r = g1r_madd_lazy_sl<GROUPED, ASM, PAIRS>(acc, q.X, y);
  if (rx_is_zero(r.ZZ)) {
    RFp yr = q.Y;
    if (neg) yr = rx_neg(yr);
    r = g1r_madd_lazy_fix(was_inf, r, q.X, yr);
  }
  return r;
}

template <int OP>
__global__ void __launch_bounds__(256)
    k_g1r_op(const uint32_t* __restrict__ p, const uint32_t* __restrict__ q,
             const uint32_t* __restrict__ flags, uint32_t* __restrict__ out, uint64_t n) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i = OP == kG1AddQuad ? t >> 2 : t;  // a quad shares one row: uniform per quad
  if (i >= n) return;
  const G1R a = ld_g1row(p, i);
  G1R b = g1_op_needs_q(OP) ? ld_g1row(q, i) : a;
  const bool neg = g1_op_needs_q(OP) && flags && (flags[i] & 1u);
  G1R r;
  if constexpr (OP == kG1Madd000) r = madd_as_accumulate<false, false, false>(a, b, neg);
  else if constexpr (OP == kG1Madd100) r = madd_as_accumulate<true, false, false>(a, b, neg);
  else if constexpr (OP == kG1Madd110) r = madd_as_accumulate<true, true, false>(a, b, neg);
  else if constexpr (OP == kG1Madd111) r = madd_as_accumulate<true, true, true>(a, b, neg);
  else if constexpr (OP == kG1MaddLazy) r = g1r_madd_lazy(a, b.X, neg ? rx_neg_lazy(b.Y) : b.Y);
  else if constexpr (OP == kG1AddLazy || OP == kG1AddQuad) {
    if (neg) b.Y = rx_neg_lazy(b.Y);  // 4p - Y, normalised
    if constexpr (OP == kG1AddLazy) r = g1r_add_lazy(a, b);
    else r = g1r_add_quad(a, b, threadIdx.x & 3u);
  } else if constexpr (OP == kG1DblLazy) r = g1r_dbl_lazy(a);
  else if constexpr (OP == kG1LazyFinish) r = g1r_lazy_finish(a);
  else if constexpr (OP == kG1Add) r = g1r_add(a, neg ? g1r_neg(b) : b);
  else if constexpr (OP == kG1AddAffine) r = g1r_add_affine(a, b.X, neg ? rx_neg(b.Y) : b.Y);
  else if constexpr (OP == kG1Dbl) r = g1r_dbl(a);
  else r = g1r_dbl_affine(a.X, a.Y);
  st_row<FpCfg>(out, 4 * t, r.X);
  st_row<FpCfg>(out, 4 * t + 1, r.Y);
  st_row<FpCfg>(out, 4 * t + 2, r.ZZ);
  st_row<FpCfg>(out, 4 * t + 3, r.ZZZ);
}

using G1Kernel = void (*)(const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint64_t);
G1Kernel g1r_kernel(int op) {
  switch (op) {
#define PLK_G1_CASE(OP) \
  case OP: return k_g1r_op<OP>;
    PLK_G1_CASE(kG1Madd000) PLK_G1_CASE(kG1Madd100) PLK_G1_CASE(kG1Madd110)
    PLK_G1_CASE(kG1Madd111) PLK_G1_CASE(kG1MaddLazy) PLK_G1_CASE(kG1AddLazy)
    PLK_G1_CASE(kG1AddQuad) PLK_G1_CASE(kG1DblLazy) PLK_G1_CASE(kG1LazyFinish)
    PLK_G1_CASE(kG1Add) PLK_G1_CASE(kG1AddAffine) PLK_G1_CASE(kG1Dbl) PLK_G1_CASE(kG1DblAffine)
#undef PLK_G1_CASE
    default: return nullptr;
  }
}

// host arrays of uint32 rows in, one launch of `threads` threads, rows out
struct RowArg {
  const uint32_t* host;
  size_t bytes;
};
template <class K, size_t NA>
int run_rows(plk_ctx* ctx, K kern, const RowArg (&in)[NA], uint32_t* out, size_t out_bytes,
             uint64_t threads, uint64_t n) {
  DevBuf din[NA], dout;
  int st;
  hipStream_t s = ctx->stream;
  for (size_t k = 0; k < NA; ++k) {
    if (!in[k].host) continue;
    if ((st = din[k].alloc(in[k].bytes))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(din[k].ptr, in[k].host, in[k].bytes, hipMemcpyHostToDevice, s));
  }
  if ((st = dout.alloc(out_bytes))) return st;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  const uint32_t* dp[NA];
  for (size_t k = 0; k < NA; ++k) dp[k] = static_cast<const uint32_t*>(din[k].ptr);
  uint32_t* const dres = static_cast<uint32_t*>(dout.ptr);
  if constexpr (NA == 4)
    hipLaunchKernelGGL(kern, grid, block, 0, s, dp[0], dp[1], dp[2], dp[3], dres, n);
  else
    hipLaunchKernelGGL(kern, grid, block, 0, s, dp[0], dp[1], dp[2], dres, n);
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipMemcpyAsync(out, dout.ptr, out_bytes, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  return PLK_OK;
}


// ---- plk_debug_prover_stage: the prover's pk_* launchers on caller arrays ----------------
enum : int {
  kStPermNumDen = 0, kStScan, kStQuotient, kStPiSparse, kStPiCoef, kStCosetCombine, kStEval,
  kStLinComb, kStScalePowers, kStRuffini, kStQuotientTop, kStCosetCombineTop, kStCount
};

struct StageCall {
  int stage;
  const uint64_t* const* in;
  const size_t* len;  // Fr elements per input array
  size_t n_in;
  const plk_fr* sc;
  size_t n_sc;
  const uint64_t* par;
  size_t n_par;
  uint64_t* out;
  size_t out_cap;  // Fr elements
};

// The stage's launcher on device copies of c.in; PLK_E_ARG unless the array lengths are the
// ones the kernels index (every read and write of a launch lies inside an array checked here).
int run_stage(plk_ctx* ctx, const StageCall& c) {
  hipStream_t s = ctx->stream;
  int st;
  std::vector<DevBuf> d(c.n_in);
  for (size_t k = 0; k < c.n_in; ++k) {
    if (c.len[k] == 0) continue;
    if ((st = d[k].alloc(c.len[k] * sizeof(Fr)))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(d[k].ptr, c.in[k], c.len[k] * sizeof(Fr), hipMemcpyHostToDevice, s));
  }
  auto in = [&](size_t k) { return d[k].as<Fr>(); };
  auto sc = [&](size_t k) { return fr_from_abi(c.sc[k]); };
  DevBuf dout;
  auto finish = [&](const Fr* res, size_t count) -> int {
    if (count) PLK_HIP_TRY(hipMemcpyAsync(c.out, res, count * sizeof(Fr), hipMemcpyDeviceToHost, s));
    PLK_HIP_TRY(stream_wait(s));
    return PLK_OK;
  };
  switch (c.stage) {
    case kStPermNumDen: {  // in: wires (4 x stride), sigmas (4 x n), elements; sc: beta gamma k1 k2 k3
      if (c.n_in != 3 || c.n_sc != 5 || c.n_par != 2) return PLK_E_ARG;
      const uint64_t n = c.par[0], ws = c.par[1];
      if (n == 0) return PLK_OK;
      if (ws < n || c.len[0] != 4 * ws || c.len[1] != 4 * n || c.len[2] != n || c.out_cap < 2 * n)
        return PLK_E_ARG;
      if ((st = dout.alloc(2 * n * sizeof(Fr)))) return st;
      if ((st = pk_perm_numden(in(0), ws, in(1), in(2), n, sc(0), sc(1), sc(2), sc(3), sc(4),
                               dout.as<Fr>(), dout.as<Fr>() + n, s)))
        return st;
      return finish(dout.as<Fr>(), 2 * n);
    }
    case kStScan: {  // par: flags (1 mul, 2 suffix, 4 exclusive, 8 in place); out: n values, tmp[nb]
      if (c.n_in != 1 || c.n_par != 1 || c.par[0] > 15) return PLK_E_ARG;
      const uint64_t n = c.len[0], f = c.par[0];
      if (n == 0) return PLK_OK;
      if (c.out_cap < n + 1) return PLK_E_ARG;
      const uint64_t nt = pk_scan_tmp_elems(n);
      DevBuf tmp;
      if ((st = tmp.alloc(nt * sizeof(Fr)))) return st;
      Fr* res = in(0);
      if (!(f & 8)) {
        if ((st = dout.alloc(n * sizeof(Fr)))) return st;
        res = dout.as<Fr>();
      }
      if ((st = pk_scan(in(0), res, n, f & 1, f & 2, f & 4, tmp.as<Fr>(), s))) return st;
      PLK_HIP_TRY(hipMemcpyAsync(c.out + 4 * n, tmp.as<Fr>() + (nt - 1), sizeof(Fr),
                                 hipMemcpyDeviceToHost, s));
      return finish(res, n);
    }
    case kStQuotient: {
      // in: a b c d z pi l1 sel sigma elements, as k_quotient reads them (QuotientArgs; pi of
      // length 0: no public inputs); sc: alpha beta gamma range_sep logic_sep fixed_sep var_sep,
      // s_m[blocks], vh_inv[blocks]; par: log2 n, blocks, has_range | 2 has_logic | 4 has_fixed |
      // 8 has_var
      if (c.n_in != 10 || c.n_par != 3 || c.par[0] > 24 || c.par[2] > 15) return PLK_E_ARG;
      const uint64_t blocks = c.par[1], n = 1ull << c.par[0], nq = blocks * n;
      if ((blocks != kQBlocks && blocks != kQBlocksSmall) || c.n_sc != 7 + 2 * blocks) return PLK_E_ARG;
      for (int k = 0; k < 7; ++k)
        if (c.len[k] != nq && !(k == 5 && c.len[k] == 0)) return PLK_E_ARG;
      if (c.len[7] != SEL_COUNTQ * nq || c.len[8] != 4 * nq || c.len[9] != n || c.out_cap < nq)
        return PLK_E_ARG;
      if ((st = dout.alloc(nq * sizeof(Fr)))) return st;
      QuotientArgs qa{};
      qa.a = in(0), qa.b = in(1), qa.c = in(2), qa.d = in(3), qa.z = in(4);
      qa.pi = c.len[5] ? in(5) : nullptr;
      qa.l1 = in(6), qa.sel = in(7), qa.sigma = in(8), qa.elements = in(9);
      qa.out = dout.as<Fr>();
      qa.nq = nq;
      qa.log_blk = (uint32_t)c.par[0];
      Fr s_m[kQBlocksMax], vh[kQBlocksMax];
      for (uint64_t m = 0; m < blocks; ++m) s_m[m] = sc(7 + m), vh[m] = sc(7 + blocks + m);
      const uint64_t f = c.par[2];
      quotient_constants(qa, QuotientChallenges{sc(0), sc(1), sc(2), sc(3), sc(4), sc(5), sc(6)}, s_m,
                         vh, (int)blocks, f & 1, f & 2, f & 4, f & 8);
      if ((st = pk_quotient(qa, s))) return st;
      return finish(dout.as<Fr>(), nq);
    }
    case kStPiSparse: {  // in: l1 (nq); sc: the values; par: log2 n, then the gate indices
      if (c.n_in != 1 || c.n_par != 1 + c.n_sc || c.par[0] > 24) return PLK_E_ARG;
      const uint64_t nq = c.len[0];
      if (nq == 0) return PLK_OK;
      if (nq & ((1ull << c.par[0]) - 1) || c.out_cap < nq) return PLK_E_ARG;
      PiSparse ps{};
      ps.count = (uint32_t)c.n_sc;  // 0 or more than kPiSparse: pk_pi_sparse refuses
      for (size_t k = 0; k < c.n_sc && k < (size_t)kPiSparse; ++k) {
        ps.idx[k] = (uint32_t)c.par[1 + k];
        ps.v[k] = sc(k);
      }
      if ((st = dout.alloc(nq * sizeof(Fr)))) return st;
      if ((st = pk_pi_sparse(ps, in(0), (uint32_t)c.par[0], nq, dout.as<Fr>(), s))) return st;
      return finish(dout.as<Fr>(), nq);
    }
    case kStPiCoef: {  // in: tw_inv (n, R'); sc: value n^-1 per input; par: the gate indices
      if (c.n_in != 1 || c.n_par != c.n_sc) return PLK_E_ARG;
      const uint64_t n = c.len[0];
      if (n == 0) return PLK_OK;
      if (c.out_cap < n) return PLK_E_ARG;
      PiDirect pd{};
      pd.count = (uint32_t)c.n_sc;  // more than kPiDirect: pk_pi_coef refuses
      for (size_t k = 0; k < c.n_sc && k < (size_t)kPiDirect; ++k) {
        pd.idx[k] = c.par[k];
        pd.c[k] = sc(k);
      }
      if ((st = dout.alloc(n * sizeof(Fr)))) return st;
      if ((st = pk_pi_coef(pd, in(0), n, dout.as<Fr>(), s))) return st;
      return finish(dout.as<Fr>(), n);
    }
    case kStCosetCombine: {  // in: blocks x n coefficients; sc: blocks^2 matrix entries (R'); par: blocks
      if (c.n_in != 1 || c.n_par != 1) return PLK_E_ARG;
      const uint64_t blocks = c.par[0];
      if (blocks == 0 || blocks > 64 || c.n_sc != blocks * blocks || c.len[0] % blocks) return PLK_E_ARG;
      const uint64_t n = c.len[0] / blocks;
      if (n == 0) return PLK_OK;
      if (c.out_cap < blocks * n) return PLK_E_ARG;
      CombineMat mat{};
      for (size_t k = 0; k < c.n_sc && k < (size_t)(kQBlocksMax * kQBlocksMax); ++k) mat.m[k] = sc(k);
      if ((st = dout.alloc(blocks * n * sizeof(Fr)))) return st;
      if ((st = pk_coset_combine(in(0), n, (int)blocks, mat, dout.as<Fr>(), s))) return st;
      return finish(dout.as<Fr>(), blocks * n);
    }
    case kStEval: {  // in: the polynomials; sc: one point each
      if (c.n_in > (size_t)kMaxEval || c.n_sc != c.n_in || c.n_par != 0) return PLK_E_ARG;
      const uint32_t count = (uint32_t)c.n_in;
      if (count == 0) return PLK_OK;
      if (c.out_cap < count) return PLK_E_ARG;
      EvalBatch eb{};
      uint64_t max_len = 0;
      for (uint32_t k = 0; k < count; ++k) {
        eb.poly[k] = in(k);
        eb.len[k] = c.len[k];
        eb.x[k] = sc(k);
        max_len = std::max<uint64_t>(max_len, c.len[k]);
      }
      DevBuf partial;
      const size_t mb = pk_eval_max_blocks(max_len ? max_len : 1);
      if ((st = partial.alloc(mb * count * sizeof(Fr))) || (st = dout.alloc(count * sizeof(Fr))))
        return st;
      if ((st = pk_eval(eb, count, max_len, partial.as<Fr>(), dout.as<Fr>(), s))) return st;
      return finish(dout.as<Fr>(), count);
    }
    case kStLinComb: {  // in: the terms; sc: one scalar each; par: len_out
      if (c.n_in > (size_t)kMaxTerms || c.n_sc != c.n_in || c.n_par != 1) return PLK_E_ARG;
      const uint64_t len_out = c.par[0];
      if (len_out == 0) return PLK_OK;
      if (c.out_cap < len_out) return PLK_E_ARG;
      LinComb lc{};
      lc.terms = (uint32_t)c.n_in;
      for (uint32_t t = 0; t < lc.terms; ++t) {
        lc.p[t] = in(t);
        lc.len[t] = c.len[t];
        lc.s[t] = sc(t);
      }
      if ((st = dout.alloc(len_out * sizeof(Fr)))) return st;
      if ((st = pk_lincomb(lc, dout.as<Fr>(), len_out, s))) return st;
      return finish(dout.as<Fr>(), len_out);
    }
    case kStScalePowers: {  // in: c; sc: x; par: shift
      if (c.n_in != 1 || c.n_sc != 1 || c.n_par != 1) return PLK_E_ARG;
      const uint64_t len = c.len[0];
      if (len == 0) return PLK_OK;
      if (c.out_cap < len) return PLK_E_ARG;
      if ((st = dout.alloc(len * sizeof(Fr)))) return st;
      if ((st = pk_scale_powers(in(0), len, sc(0), c.par[0], dout.as<Fr>(), s))) return st;
      return finish(dout.as<Fr>(), len);
    }
    case kStRuffini: {  // in: c; sc: z (not 0); out: len - 1 quotient coefficients
      if (c.n_in != 1 || c.n_sc != 1 || c.n_par != 0) return PLK_E_ARG;
      const uint64_t len = c.len[0];
      if (len <= 1) return PLK_OK;
      if (c.out_cap < len - 1 || fe_is_zero(sc(0))) return PLK_E_ARG;
      DevBuf tmp, scan;  // as the prover: tmp_a and scan_tmp beside the aggregate and w
      if ((st = dout.alloc((len - 1) * sizeof(Fr))) || (st = tmp.alloc(len * sizeof(Fr))) ||
          (st = scan.alloc(pk_scan_tmp_elems(len) * sizeof(Fr))))
        return st;
      if ((st = pk_ruffini(in(0), len, sc(0), dout.as<Fr>(), tmp.as<Fr>(), scan.as<Fr>(), s))) return st;
      return finish(dout.as<Fr>(), len - 1);
    }
    case kStCosetCombineTop: {
      // in: 4 x n coefficients (the inverse block transforms); sc: the 16 matrix entries (R', row
      // major), Q[7], p_0 .. p_4 (quotient_top.hpp quotient_patch) -> 4n + 8 coefficients of t
      if (c.n_in != 1 || c.n_par != 0 || c.n_sc != 16 + kTop + kQBlocksTop + 1 || c.len[0] % kQBlocksTop)
        return PLK_E_ARG;
      const uint64_t n = c.len[0] / kQBlocksTop;
      if (n == 0) return PLK_OK;
      if (n <= (uint64_t)kTop || c.out_cap < 4 * n + 8) return PLK_E_ARG;
      CombineMat mat{};
      for (int k = 0; k < 16; ++k) mat.m[k] = sc(k);
      Fr q[kTop], p[kQBlocksTop + 1];
      for (int j = 0; j < kTop; ++j) q[j] = sc(16 + j);
      for (int l = 0; l <= kQBlocksTop; ++l) p[l] = sc(16 + kTop + l);
      QuotientPatch patch;
      quotient_patch(q, p, patch);
      if ((st = dout.alloc((4 * n + 8) * sizeof(Fr)))) return st;
      if ((st = pk_coset_combine_top(in(0), n, mat, patch, dout.as<Fr>(), s))) return st;
      return finish(dout.as<Fr>(), 4 * n + 8);
    }
    default: return PLK_E_ARG;
  }
}

// Stage kStQuotientTop, host code only (no context): quotient_top (quotient_top.hpp) on the
// caller's top coefficients. in: wires (4 x 7), z (7), selectors (11 x 7, SEL_* order), sigmas
// (4 x 7), L1 (7), each row seven coefficients in ascending order; sc: alpha beta gamma range_sep
// logic_sep fixed_sep var_sep, omega, then the public-input values; par: log2 n, the has_* flags,
// then one gate index per public input -> Q[7] = t[4n .. 4n + 6]
int run_quotient_top(const StageCall& c) {
  const size_t want[5] = {4 * kTop, kTop, SEL_COUNTQ * kTop, 4 * kTop, kTop};
  if (c.n_in != 5 || c.n_sc < 8 || c.n_par != 2 + (c.n_sc - 8) || c.out_cap < (size_t)kTop)
    return PLK_E_ARG;
  for (int k = 0; k < 5; ++k)
    if (c.len[k] != want[k]) return PLK_E_ARG;
  if (c.par[0] < 4 || c.par[0] > 27 || c.par[1] > 15) return PLK_E_ARG;
  const uint64_t n = 1ull << c.par[0];
  const size_t npi = c.n_sc - 8;
  QuotientTopIn ti;
  Fr* rows[5] = {&ti.wire[0][0], ti.z, &ti.sel[0][0], &ti.sigma[0][0], ti.l1};
  for (int k = 0; k < 5; ++k) std::memcpy(rows[k], c.in[k], want[k] * sizeof(Fr));
  Fr ch[CH_COUNT] = {};
  ch[CH_ALPHA] = fr_from_abi(c.sc[0]), ch[CH_BETA] = fr_from_abi(c.sc[1]);
  ch[CH_GAMMA] = fr_from_abi(c.sc[2]), ch[CH_RANGE] = fr_from_abi(c.sc[3]);
  ch[CH_LOGIC] = fr_from_abi(c.sc[4]), ch[CH_FIXED] = fr_from_abi(c.sc[5]);
  ch[CH_VAR] = fr_from_abi(c.sc[6]);
  const Fr omega = fr_from_abi(c.sc[7]);
  if (fe_is_zero(omega)) return PLK_E_ARG;
  Fr nf = fe_zero<FrCfg>();
  nf.v[0] = (uint32_t)n;
  const Fr n_inv = fe_inv(fe_to_mont(nf));
  std::vector<Fr> pi(npi), wi(npi);
  for (size_t i = 0; i < npi; ++i) {
    if (c.par[2 + i] >= n) return PLK_E_ARG;
    pi[i] = fr_from_abi(c.sc[8 + i]);
    wi[i] = fe_pow_u64(omega, c.par[2 + i]);
  }
  const Top pit = top_public_inputs(pi.data(), wi.data(), npi, n_inv, n);
  Fr q[kTop];
  quotient_top(ti, pit, n, omega, fe_inv(omega), ch, (unsigned)c.par[1], q);
  std::memcpy(c.out, q, sizeof q);
  return PLK_OK;
}

}  // namespace
}  // namespace plk

extern "C" int plk_debug_rx_op(plk_ctx* ctx, int field, int op, const uint32_t* a,
                               const uint32_t* b, const uint32_t* c, const uint32_t* d,
                               uint32_t* out, size_t n) {
  try {
    if (!ctx || !out || (field != 0 && field != 1)) return PLK_E_ARG;
    const plk::RxKernel kern = plk::rx_kernel(field, op);
    if (!kern) return PLK_E_ARG;
    const uint32_t* rows[4] = {a, b, c, d};
    const int nin = plk::rx_op_nin(op);
    for (int k = 0; k < nin; ++k)
      if (!rows[k]) return PLK_E_ARG;
    if (n == 0) return PLK_OK;
    const size_t row = (field == 0 ? 9 : 13) * sizeof(uint32_t);
    plk::RowArg in[4];
    for (int k = 0; k < 4; ++k) in[k] = {k < nin ? rows[k] : nullptr, n * row};
    plk::DeviceGuard g(ctx->device);
    return plk::run_rows(ctx, kern, in, out, n * row * plk::rx_op_nout(op), n, n);
  } catch (...) {
    return PLK_E_DEVICE;
  }
}

extern "C" int plk_debug_ntt_lazy_op(plk_ctx* ctx, int op, const uint32_t* in, uint32_t* out,
                                     size_t n) {
  try {
    if (!ctx || !in || !out) return PLK_E_ARG;
    plk::DeviceGuard g(ctx->device);
    return plk::ntt_lazy_op(ctx, op, in, out, n);
  } catch (...) {
    return PLK_E_DEVICE;
  }
}

extern "C" int plk_debug_g1r_op(plk_ctx* ctx, int op, const uint32_t* p, const uint32_t* q,
                                const uint32_t* flags, uint32_t* out, size_t n) {
  try {
    if (!ctx || !p || !out) return PLK_E_ARG;
    const plk::G1Kernel kern = plk::g1r_kernel(op);
    if (!kern || (plk::g1_op_needs_q(op) && !q)) return PLK_E_ARG;
    if (n == 0) return PLK_OK;
    const size_t row = plk::kG1Row * sizeof(uint32_t);
    const uint64_t threads = op == plk::kG1AddQuad ? 4 * (uint64_t)n : n;
    const plk::RowArg in[3] = {{p, n * row},
                               {plk::g1_op_needs_q(op) ? q : nullptr, n * row},
                               {flags, n * sizeof(uint32_t)}};
    plk::DeviceGuard g(ctx->device);
    return plk::run_rows(ctx, kern, in, out, threads * row, threads, n);
  } catch (...) {
    return PLK_E_DEVICE;
  }
}

extern "C" int plk_debug_field_op(plk_ctx* ctx, int field, int op, const uint64_t* a,
                                  const uint64_t* b, uint64_t* out, size_t n) {
  try {
    if (!ctx || !a || !out || op < 0 || op > 4 || (field != 0 && field != 1)) return PLK_E_ARG;
    if (n == 0) return PLK_OK;
    plk::DeviceGuard g(ctx->device);
    return field == 0 ? plk::run<plk::FrCfg>(ctx, op, a, b, out, n)
                      : plk::run<plk::FpCfg>(ctx, op, a, b, out, n);
  } catch (...) {
    return PLK_E_DEVICE;
  }
}

// the same call the prover makes for z and PI and key compilation for its tables (key.hip
// coset_blocks_fwd)
extern "C" int plk_debug_block_eval(plk_key* key, const uint64_t* coef, size_t len, uint64_t* out,
                                    size_t out_cap, int* blocks_out) {
  using plk::last_hip_error;
  try {
    if (!key) return PLK_E_ARG;
    // the cosets m < 5 (6 for n = 8), whatever number of them the prover's round 3 uses: a coset
    // table of this call's own, made as the key's is (key.hip)
    const int blocks = key->n >= 16 ? plk::kQBlocks : plk::kQBlocksSmall;
    if (blocks_out) *blocks_out = blocks;
    if (!out) return PLK_OK;
    const uint64_t n = key->n, total = (uint64_t)blocks * n;
    if (!coef || len == 0 || len > n + 8 || out_cap < total) return PLK_E_ARG;
    plk::DeviceGuard g(key->ctx->device);
    hipStream_t s = key->ctx->stream;
    plk::DevBuf din, dout, table;
    int st;
    if ((st = din.alloc(len * sizeof(plk::Fr))) || (st = dout.alloc(total * sizeof(plk::Fr))) ||
        (st = table.alloc(blocks * (n + 8) * sizeof(plk::Fr))))
      return st;
    PLK_HIP_TRY(hipMemcpyAsync(din.ptr, coef, len * sizeof(plk::Fr), hipMemcpyHostToDevice, s));
    plk::Fr sm[plk::kQBlocksMax];
    plk::coset_shifts(key->dom, blocks, sm);
    for (int mb = 0; mb < blocks; ++mb)
      if ((st = plk::ntt_power_table(table.as<plk::Fr>() + mb * (n + 8), sm[mb],
                                     plk::fe_one<plk::FrCfg>(), n + 8, true, s)))
        return st;
    if ((st = plk::coset_blocks_fwd(key->dom, din.as<plk::Fr>(), dout.as<plk::Fr>(), len,
                                    table.as<plk::Fr>(), blocks, nullptr, s)))
      return st;
    PLK_HIP_TRY(hipMemcpyAsync(out, dout.ptr, total * sizeof(plk::Fr), hipMemcpyDeviceToHost, s));
    PLK_HIP_TRY(plk::stream_wait(s));
    return PLK_OK;
  } catch (...) {
    return PLK_E_DEVICE;
  }
}

// the pk_* launcher the prover calls for `stage`, on device copies of the caller's arrays
extern "C" int plk_debug_prover_stage(plk_ctx* ctx, int stage, const uint64_t* const* in,
                                      const size_t* in_len, size_t n_in, const plk_fr* scalars,
                                      size_t n_scalars, const uint64_t* params, size_t n_params,
                                      uint64_t* out, size_t out_cap) {
  try {
    if (stage < 0 || stage >= plk::kStCount) return PLK_E_ARG;
    if ((n_in && (!in || !in_len)) || (n_scalars && !scalars) || (n_params && !params) ||
        (out_cap && !out) || n_in > 32)
      return PLK_E_ARG;
    for (size_t k = 0; k < n_in; ++k)
      if (in_len[k] > ((size_t)1 << 28) || (in_len[k] && !in[k])) return PLK_E_ARG;
    const plk::StageCall c{stage, in, in_len, n_in, scalars, n_scalars, params, n_params, out, out_cap};
    if (stage == plk::kStQuotientTop) return plk::run_quotient_top(c);  // host only: ctx unused
    if (!ctx) return PLK_E_ARG;
    plk::DeviceGuard g(ctx->device);
    return plk::run_stage(ctx, c);
  } catch (...) {
    return PLK_E_DEVICE;
  }
}

// The polynomials of the prover's last round 3 (test support): out = alpha beta gamma range_sep
// logic_sep fixed_sep var_sep | the 11 selectors' n coefficients (SEL_* order) | the 4 sigmas' |
// the 4 blinded wires' n + 2 | z's n + 3 | t's 4n + 8 — 24n + 26 elements. PLK_E_ARG unless the
// prover's last plk_prover_prove reached round 3 on a key with n >= 16.
extern "C" int plk_debug_prover_round3(plk_prover* p, uint64_t* out, size_t out_cap) {
  using plk::Fr;
  using plk::last_hip_error;
  try {
    if (!p || !out || !p->have_round3 || p->key->qb != plk::kQBlocksTop) return PLK_E_ARG;
    const plk_key* key = p->key;
    const uint64_t n = key->n, S = n + 8;
    if (out_cap < 24 * n + 26) return PLK_E_ARG;
    plk::DeviceGuard g(key->ctx->device);
    hipStream_t s = p->stream;
    Fr* o = reinterpret_cast<Fr*>(out);
    std::memcpy(o, p->last_ch, sizeof p->last_ch);
    o += 7;
    auto d2h = [&](const Fr* src, uint64_t count) {
      const hipError_t e = hipMemcpyAsync(o, src, count * sizeof(Fr), hipMemcpyDeviceToHost, s);
      o += count;
      return e;
    };
    // q_coef rows are in the gate's selector order, which is SEL_* order
    PLK_HIP_TRY(d2h(key->q_coef.as<Fr>(), 11 * n));
    PLK_HIP_TRY(d2h(key->sigma_coef.as<Fr>(), 4 * n));
    for (int c = 0; c < 4; ++c) PLK_HIP_TRY(d2h(p->wires_coef.as<Fr>() + c * S, n + 2));
    PLK_HIP_TRY(d2h(p->z_coef.as<Fr>(), n + 3));
    PLK_HIP_TRY(d2h(p->t_coef.as<Fr>(), 4 * n + 8));
    PLK_HIP_TRY(plk::stream_wait(s));
    return PLK_OK;
  } catch (...) {
    return PLK_E_DEVICE;
  }
}

// One batch of the fixed-base MSM on a workspace of this call's own, then the workspace's buffers
// as the batch left them (include/plk.h). msm_run_batch is the library's, unchanged: it reports
// the batch's plan in MsmWorkspace::last.
extern "C" int plk_debug_msm_snapshot(plk_srs* s, const plk_fr* const* scalars, const size_t* lens,
                                      size_t count, plk_msm_snapshot* snap, plk_g1* outs,
                                      int* statuses) {
  using namespace plk;
  try {
    if (!s || !lens || !snap || !outs || !statuses || count == 0 || count > kMaxSlots ||
        (!scalars && count) || snap->tail_quad > 2)
      return PLK_E_ARG;
    for (size_t k = 0; k < count; ++k)
      if (!scalars[k] && lens[k]) return PLK_E_ARG;
    DeviceGuard g(s->ctx->device);
    hipStream_t st = s->ctx->stream;
    DevBuf dsc[kMaxSlots];
    const Fr* ptrs[kMaxSlots];
    size_t use[kMaxSlots], chk[kMaxSlots];
    int r;
    for (size_t k = 0; k < count; ++k) {
      if ((r = dsc[k].alloc(std::max<size_t>(lens[k], 1) * sizeof(Fr)))) return r;
      if (lens[k])
        PLK_HIP_TRY(hipMemcpyAsync(dsc[k].ptr, scalars[k], lens[k] * sizeof(Fr), hipMemcpyHostToDevice, st));
      ptrs[k] = dsc[k].as<Fr>();
      chk[k] = lens[k];
      use[k] = std::min(lens[k], s->n);
    }
    struct WsDelete {
      void operator()(MsmWorkspace* w) const { msm_workspace_delete(w); }
    };
    std::unique_ptr<MsmWorkspace, WsDelete> ws(msm_workspace_new());
    MsmWorkspace& w = *ws;
    w.shared_chip = snap->shared_chip != 0;
    w.tail_quad = (int)snap->tail_quad;
    r = msm_run_batch(s, w, ptrs, use, chk, count, outs, statuses, st, snap->part, snap->parts,
                      snap->guard_limit);
    if (r != PLK_OK && r != PLK_E_DEGREE) return r;
    const MsmPlan& d = w.last;
    const uint64_t hdr[PLK_MSM_SNAPSHOT_HDR] = {
        d.B, d.W, d.narrow, d.c, d.chunk, d.rb, d.fb, d.NC, d.NR, d.G, d.nbits, d.nout, d.wide,
        d.sort_one, d.hold, w.task_stride, w.sorted_stride, d.max_tasks_used, d.b_lo, s->n, d.gen,
        snap->part, snap->parts, s->has_inf ? 1u : 0u};
    std::memcpy(snap->hdr, hdr, sizeof hdr);
    const size_t B = d.B, row = sizeof(G1xyzz);
    static_assert(sizeof(G1xyzz) == 48 * 4, "packed XYZZ row");
    auto d2h = [&](uint32_t* dst, const void* src, size_t off_bytes, size_t bytes) -> hipError_t {
      if (!dst || !bytes) return hipSuccess;
      return hipMemcpy(dst, static_cast<const uint8_t*>(src) + off_bytes, bytes, hipMemcpyDeviceToHost);
    };
    const ReadbackHeader* rh = w.host_out.as<ReadbackHeader>();
    const G1xyzz* T = reinterpret_cast<const G1xyzz*>(rh + 1);
    for (size_t k = 0; k < count; ++k) {
      // the slot's entry and task counts first: they bound the copies below
      uint32_t ends[2] = {0, 0};
      PLK_HIP_TRY(hipMemcpy(&ends[0], w.offsets.as<uint32_t>() + k * (B + 1) + B, 4, hipMemcpyDeviceToHost));
      PLK_HIP_TRY(hipMemcpy(&ends[1], w.task_off.as<uint32_t>() + k * (B + 1) + B, 4, hipMemcpyDeviceToHost));
      const size_t n_ent = ends[0], n_task = ends[1];
      if (n_ent + 1 > w.sorted_stride || n_task > w.task_stride) return PLK_E_DEVICE;
      if ((snap->sorted && n_ent > snap->cap_sorted) ||
          ((snap->tasks || snap->partials) && n_task > snap->cap_tasks))
        return PLK_E_ARG;
      snap->n_tasks[k] = (uint32_t)n_task;
      PLK_HIP_TRY(d2h(snap->offsets ? snap->offsets + k * (B + 1) : nullptr, w.offsets.ptr, k * (B + 1) * 4, (B + 1) * 4));
      PLK_HIP_TRY(d2h(snap->task_off ? snap->task_off + k * (B + 1) : nullptr, w.task_off.ptr, k * (B + 1) * 4, (B + 1) * 4));
      PLK_HIP_TRY(d2h(snap->sorted ? snap->sorted + k * snap->cap_sorted : nullptr, w.sorted.ptr,
                      k * w.sorted_stride * 4, n_ent * 4));
      PLK_HIP_TRY(d2h(snap->tasks ? snap->tasks + 2 * k * snap->cap_tasks : nullptr, w.tasks.ptr,
                      k * w.task_stride * sizeof(uint2), n_task * sizeof(uint2)));
      PLK_HIP_TRY(d2h(snap->partials ? snap->partials + 48 * k * snap->cap_tasks : nullptr, w.partials.ptr,
                      k * w.task_stride * row, n_task * row));
      if (d.wide) {
        PLK_HIP_TRY(d2h(snap->rsum ? snap->rsum + 48 * k * B : nullptr, w.rsum.ptr, k * B * row, B * row));
        PLK_HIP_TRY(d2h(snap->ys ? snap->ys + 48 * k * d.NR : nullptr, w.ys.ptr, k * d.NR * row, d.NR * row));
        PLK_HIP_TRY(d2h(snap->zs ? snap->zs + 48 * k * d.NR : nullptr, w.zs.ptr, k * d.NR * row, d.NR * row));
      } else {
        PLK_HIP_TRY(d2h(snap->bsum ? snap->bsum + 48 * k * B : nullptr, w.bsum.ptr, k * B * row, B * row));
      }
      if (snap->bits) std::memcpy(snap->bits + 48 * k * d.nout, &T[k * d.nout], d.nout * row);
      if (snap->readback) {
        snap->readback[3 * k] = rh->flag[k];
        snap->readback[3 * k + 1] = rh->entries[k];
        snap->readback[3 * k + 2] = rh->max_count[k];
      }
    }
    return r;
  } catch (const std::bad_alloc&) {
    return PLK_E_OOM;
  } catch (...) {
    return PLK_E_DEVICE;
  }
}
