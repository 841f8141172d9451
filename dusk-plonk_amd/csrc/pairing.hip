// pairing.hip — the opening key (the G2 half of EvaluationKey), the host pairing check and the
// batched pairing kernel: e(C, H) == e(W, [tau]H) for one pair per lane
// (the reference's commitment_scheme.rs:24-66 ends in multi_miller_loop(..).final_exp()).
//
// The arithmetic is csrc/pairing.hpp, the same source on host and device. On the device a
// lane's Fp12 values live in a workspace tiled by wave, [slot][coefficient][32-bit word][lane]
// inside a tile (coalesced: the lanes of a wave read one 256-byte row per word); only Fp2
// operands are in registers, so the kernel owns no scratch object. Both Miller loops of a pair share their 63 squarings, and both
// line tables are read at lane-uniform addresses. G2 points are prepared on the host
// (pairing_host.hpp); no G2 arithmetic runs here.
//
// Test support at the end of each part: plk_debug_pairing (a pairing value), plk_debug_f12_op (one
// operation of the tower, host slots or k_f12_op over the same tiles) and plk_debug_miller (the
// raw Miller value, host or k_miller_value).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "internal.hpp"
#include "pairing_host.hpp"

using namespace plk;

struct plk_opening_key {
  G2Aff h, bh;
  // [0, 136): the lines of H; [136, 272): of beta_h; [272, 284): frob_table
  std::vector<Fp2> tab;
  int device = -1;
  DevBuf d_tab, d_ws, d_pts, d_ok, d_out;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float kernel_ms = 0.f;
};

namespace plk {
namespace {

constexpr int kTabH = 0, kTabB = 2 * kMillerLines, kTabFrob = 4 * kMillerLines;
constexpr int kTabLen = kTabFrob + 12;
constexpr uint32_t kF12Words = 144;  // one Fp12 value

// A lane's Fp12 slots. The workspace is tiled by wave: tile t (the 64 lanes of block t) holds
// [slot][coefficient][word][lane], so a wave reads one 256-byte row per word and every word's
// offset from the coefficient's row is a compile-time constant (no address arithmetic in
// registers beyond the row's).
constexpr size_t kTileWords = (size_t)kF12Slots * kF12Words * 64;
struct F12Dev {
  uint32_t* base;  // the tile, already offset by the lane
  __device__ __forceinline__ Fp2 ld(int slot, int i) const {
    const uint32_t* p = base + (slot * 6 + i) * (24 * 64);
    Fp2 r;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      r.c0.v[k] = p[k * 64];
      r.c1.v[k] = p[(12 + k) * 64];
    }
    return r;
  }
  __device__ __forceinline__ void st(int slot, int i, const Fp2& a) {
    uint32_t* p = base + (slot * 6 + i) * (24 * 64);
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      p[k * 64] = a.c0.v[k];
      p[(12 + k) * 64] = a.c1.v[k];
    }
  }
};

// pairs != 0: lane j checks (pts[2 j], pts[2 j + 1]) = (C, W) against (tab H, tab beta_h) and
// writes ok[j]. pairs == 0: lane j writes ML(pts[j], Q)^(3 (p^12 - 1) / r) to out[72 j ..], Q's
// lines at tab[0 ..]. ws: one tile of kTileWords words per block of 64 lanes.
__global__ void __launch_bounds__(64) k_pairing(const plk_g1* __restrict__ pts, uint32_t count,
                                                int pairs, const Fp2* __restrict__ tab,
                                                uint32_t* __restrict__ ws,
                                                uint8_t* __restrict__ ok, uint64_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  F12Dev m{ws + (size_t)blockIdx.x * kTileWords + threadIdx.x};
  // the points were validated by the caller (pairing_check_dev): the plain load
  const G1Abi p0 = g1_load<false>(pairs ? &pts[2 * (size_t)j] : &pts[j]);
  G1Abi p1 = p0;
  bool on1 = false;
  if (pairs) {
    p1 = g1_load<false>(&pts[2 * (size_t)j + 1]);
    on1 = !p1.inf;
    p1.y = fe_neg(p1.y);
  }
  miller_loop(m, tab + kTabH, !p0.inf, p0.x, p0.y, pairs != 0, tab + kTabB, on1, p1.x, p1.y);
  const int r = f12_final_exp(m, tab + kTabFrob);
  if (pairs) {
    ok[j] = f12_is_one(m, r) ? 1 : 0;
  } else {
    for (int i = 0; i < 6; ++i) {
      const Fp2 a = m.ld(r, i);
      fe_to_abi(a.c0, out + 72 * (size_t)j + 12 * i);
      fe_to_abi(a.c1, out + 72 * (size_t)j + 12 * i + 6);
    }
  }
}

// ---- test support: the tower one operation at a time (plk_debug_f12_op) and the raw Miller value
// (plk_debug_miller). Rows are plk_debug_pairing's: 72 u64, the coefficient of w^i as (c0, c1).
enum : int {
  kDbgF2Mul, kDbgF2Sqr, kDbgF2Inv, kDbgF2MulXi, kDbgMul, kDbgSqr, kDbgCycSqr, kDbgInvEven,
  kDbgConj, kDbgFrob1, kDbgFrob2, kDbgMulLine, kDbgFinalExp, kDbgOps
};
constexpr int kDbgInPlace = 0x100;  // conj, frob1, frob2 with d == a

// the ops that read row b; all but mul_line take it as an Fp12 value in slot 1
PLK_HD bool dbg_reads_b(int op) { return op == kDbgF2Mul || op == kDbgMul || op == kDbgMulLine; }

PLK_HD Fp2 f2_of_abi(const uint64_t* l) { return {fe_of_abi<FpCfg>(l), fe_of_abi<FpCfg>(l + 6)}; }

template <class M>
PLK_HD void f12_load_row(M& m, int slot, const uint64_t* row) {
  PLK_NOUNROLL
  for (int i = 0; i < 6; ++i) m.st(slot, i, f2_of_abi(row + 12 * i));
  f12_fence();
}

template <class M>
PLK_HD void f12_store_row(const M& m, int slot, uint64_t* row) {
  PLK_NOUNROLL
  for (int i = 0; i < 6; ++i) {
    const Fp2 a = m.ld(slot, i);
    fe_to_abi(a.c0, row + 12 * i);
    fe_to_abi(a.c1, row + 12 * i + 6);
  }
}

// One operation on the rows of one lane: a -> slot 0, b (an Fp12 operand) -> slot 1, the result in
// slot 2 unless the operation is in place or names its own slot. Returns the result's slot. The
// operands of every Fp12 operation are in distinct slots, as the contracts in pairing.hpp ask.
template <class M>
PLK_HD int f12_debug_op(M& m, int op, bool in_place, const uint64_t* a, const uint64_t* b,
                        const Fp2* frob) {
  f12_load_row(m, 0, a);
  if (dbg_reads_b(op) && op != kDbgMulLine) f12_load_row(m, 1, b);
  const int d = in_place ? 0 : 2;
  switch (op) {
    case kDbgF2Mul:
      PLK_NOUNROLL
      for (int i = 0; i < 6; ++i) m.st(2, i, f2_mul(m.ld(0, i), m.ld(1, i)));
      return 2;
    case kDbgF2Sqr:
      PLK_NOUNROLL
      for (int i = 0; i < 6; ++i) m.st(2, i, f2_sqr(m.ld(0, i)));
      return 2;
    case kDbgF2Inv:
      PLK_NOUNROLL
      for (int i = 0; i < 6; ++i) m.st(2, i, f2_inv(m.ld(0, i)));
      return 2;
    case kDbgF2MulXi:
      PLK_NOUNROLL
      for (int i = 0; i < 6; ++i) m.st(2, i, f2_mul_xi(m.ld(0, i)));
      return 2;
    case kDbgMul: f12_mul(m, 2, 0, 1); return 2;
    case kDbgSqr: f12_sqr(m, 2, 0); return 2;
    case kDbgCycSqr: f12_cyc_sqr(m, 2, 0); return 2;
    case kDbgInvEven: f12_inv_even(m, 0); return 0;
    case kDbgConj: f12_conj(m, d, 0); return d;
    case kDbgFrob1: f12_frob(m, d, 0, frob, false); return d;
    case kDbgFrob2: f12_frob(m, d, 0, frob + 6, true); return d;
    case kDbgMulLine:
      f12_mul_line(m, 2, 0, f2_of_abi(b), f2_of_abi(b + 12), fe_of_abi<FpCfg>(b + 24));
      return 2;
    default: return f12_final_exp(m, frob);  // kDbgFinalExp
  }
}

// lane j: out row j = op(a row j, b row j); frob: frob_table; ws as k_pairing's
__global__ void __launch_bounds__(64) k_f12_op(int op, int in_place, const uint64_t* __restrict__ a,
                                               const uint64_t* __restrict__ b, uint32_t count,
                                               const Fp2* __restrict__ frob,
                                               uint32_t* __restrict__ ws, uint64_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  F12Dev m{ws + (size_t)blockIdx.x * kTileWords + threadIdx.x};
  const int r = f12_debug_op(m, op, in_place != 0, a + 72 * (size_t)j,
                             b ? b + 72 * (size_t)j : nullptr, frob);
  f12_fence();
  f12_store_row(m, r, out + 72 * (size_t)j);
}

// lane j: out row j = the Miller value k_pairing hands to the final exponentiation, for p0[j]
// alone (p1 == nullptr, the pairs == 0 form) or for the pair (p0[j], p1[j]) (pairs != 0)
__global__ void __launch_bounds__(64) k_miller_value(const plk_g1* __restrict__ p0,
                                                     const plk_g1* __restrict__ p1, uint32_t count,
                                                     const Fp2* __restrict__ tab,
                                                     uint32_t* __restrict__ ws,
                                                     uint64_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  F12Dev m{ws + (size_t)blockIdx.x * kTileWords + threadIdx.x};
  const G1Abi a = g1_load<false>(&p0[j]);
  G1Abi c = a;
  bool on1 = false;
  if (p1) {
    c = g1_load<false>(&p1[j]);
    on1 = !c.inf;
    c.y = fe_neg(c.y);
  }
  miller_loop(m, tab + kTabH, !a.inf, a.x, a.y, p1 != nullptr, tab + kTabB, on1, c.x, c.y);
  f12_store_row(m, 0, out + 72 * (size_t)j);
}

int key_build(const G2Aff& h, const G2Aff& bh, plk_opening_key** out) {
  std::unique_ptr<plk_opening_key> k(new plk_opening_key());
  k->h = h;
  k->bh = bh;
  k->tab.resize(kTabLen);
  if (!g2_prepare(h, &k->tab[kTabH]) || !g2_prepare(bh, &k->tab[kTabB])) return PLK_E_ARG;
  frob_table(&k->tab[kTabFrob]);
  *out = k.release();
  return PLK_OK;
}

// the table on the context's device (uploaded once) and the events
int key_on_device(plk_ctx* ctx, plk_opening_key* key, const Fp2* tab, DevBuf& d_tab, bool cache) {
  if (key) {
    if (key->device >= 0 && key->device != ctx->device) return PLK_E_ARG;  // one GPU per key
    key->device = ctx->device;
    if (!key->e0) PLK_HIP_TRY(hipEventCreate(&key->e0));
    if (!key->e1) PLK_HIP_TRY(hipEventCreate(&key->e1));
  }
  if (cache && d_tab.ptr) return PLK_OK;
  int st;
  if ((st = d_tab.alloc(kTabLen * sizeof(Fp2)))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(d_tab.ptr, tab, kTabLen * sizeof(Fp2), hipMemcpyHostToDevice, ctx->stream));
  PLK_HIP_TRY(stream_wait(ctx->stream));
  return PLK_OK;
}

size_t ws_tiles(size_t count) { return (count + 63) / 64; }

}  // namespace

// d_pairs: `count` pairs on the device; d_ok: `count` bytes on the device. Stream-ordered on the
// context's stream; the kernel sits between the key's events e0 and e1.
int pairing_check_dev(plk_ctx* ctx, plk_opening_key* key, const plk_kzg_pair* d_pairs, size_t count,
                      uint8_t* d_ok) {
  if (count == 0 || count > (1u << 24)) return PLK_E_ARG;
  int st;
  if ((st = key_on_device(ctx, key, key->tab.data(), key->d_tab, true))) return st;
  const size_t tiles = ws_tiles(count);
  if ((st = key->d_ws.alloc(tiles * kTileWords * sizeof(uint32_t)))) return st;
  hipStream_t s = ctx->stream;
  PLK_HIP_TRY(hipEventRecord(key->e0, s));
  hipLaunchKernelGGL(k_pairing, dim3((unsigned)tiles), dim3(64), 0, s,
                     reinterpret_cast<const plk_g1*>(d_pairs), (uint32_t)count, 1,
                     (const Fp2*)key->d_tab.as<Fp2>(), key->d_ws.as<uint32_t>(), d_ok,
                     (uint64_t*)nullptr);
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipEventRecord(key->e1, s));
  return PLK_OK;
}

int pairing_last_ms(plk_opening_key* key, float* ms) {
  *ms = 0.f;
  if (!key->e0 || !key->e1) return PLK_OK;
  (void)hipEventElapsedTime(ms, key->e0, key->e1);
  key->kernel_ms = *ms;
  return PLK_OK;
}

}  // namespace plk

extern "C" {

int plk_opening_key_setup(const plk_fr* tau, plk_opening_key** out) {
  PLK_API_BEGIN
  if (!out) return PLK_E_ARG;
  *out = nullptr;
  if (!tau) return PLK_E_ARG;
  const Fr t = fr_from_abi(*tau);
  if (!fe_canonical(t) || fe_is_zero(t)) return PLK_E_ARG;
  const Fr plain = fe_from_mont(t);
  const G2Aff h = g2_generator();
  return key_build(h, g2_mul(h, plain.v, 8), out);
  PLK_API_END
}

int plk_opening_key_load(const plk_g2* h, const plk_g2* beta_h, plk_opening_key** out) {
  PLK_API_BEGIN
  if (!out) return PLK_E_ARG;
  *out = nullptr;
  if (!h || !beta_h) return PLK_E_ARG;
  G2Aff a, b;
  int st;
  if ((st = g2_from_abi(*h, a)) || (st = g2_from_abi(*beta_h, b))) return st;
  if (!g2_in_subgroup(a) || !g2_in_subgroup(b)) return PLK_E_ARG;
  return key_build(a, b, out);
  PLK_API_END
}

int plk_opening_key_points(const plk_opening_key* key, plk_g2* h, plk_g2* beta_h) {
  if (!key) return PLK_E_ARG;
  if (h) g2_to_abi(key->h, h);
  if (beta_h) g2_to_abi(key->bh, beta_h);
  return PLK_OK;
}

int plk_opening_key_destroy(plk_opening_key* key) {
  PLK_API_BEGIN
  if (!key) return PLK_E_ARG;
  if (key->device >= 0) {
    DeviceGuard g(key->device);
    if (key->e0) (void)hipEventDestroy(key->e0);
    if (key->e1) (void)hipEventDestroy(key->e1);
    delete key;  // frees the device buffers on their device
    return PLK_OK;
  }
  delete key;
  return PLK_OK;
  PLK_API_END
}

int plk_pairing_check(const plk_opening_key* key, const plk_kzg_pair* pair, int* ok) {
  PLK_API_BEGIN
  if (!key || !pair || !ok) return PLK_E_ARG;
  G1In c, w;
  int st;
  if ((st = g1_from_abi(pair->c, c)) || (st = g1_from_abi(pair->w, w))) return st;
  *ok = pairing_check_host(&key->tab[kTabH], &key->tab[kTabB], &key->tab[kTabFrob], c, w) ? 1 : 0;
  return PLK_OK;
  PLK_API_END
}

int plk_pairing_check_batch(plk_ctx* ctx, plk_opening_key* key, const plk_kzg_pair* pairs,
                            size_t count, uint8_t* ok) {
  PLK_API_BEGIN
  if (!ctx || !key || !pairs || !ok || count == 0 || count > (1u << 24)) return PLK_E_ARG;
  for (size_t j = 0; j < count; ++j) {
    G1In t;
    if (g1_from_abi(pairs[j].c, t) || g1_from_abi(pairs[j].w, t)) return PLK_E_ARG;
  }
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  int st;
  if ((st = key->d_pts.alloc(count * sizeof(plk_kzg_pair)))) return st;
  if ((st = key->d_ok.alloc(count))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(key->d_pts.ptr, pairs, count * sizeof(plk_kzg_pair), hipMemcpyHostToDevice, s));
  if ((st = pairing_check_dev(ctx, key, key->d_pts.as<plk_kzg_pair>(), count, key->d_ok.as<uint8_t>())))
    return st;
  PLK_HIP_TRY(hipMemcpyAsync(ok, key->d_ok.ptr, count, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  float ms;
  pairing_last_ms(key, &ms);
  return PLK_OK;
  PLK_API_END
}

int plk_opening_key_last_pairing_ms(const plk_opening_key* key, float* kernel_ms) {
  if (!key || !kernel_ms) return PLK_E_ARG;
  *kernel_ms = key->kernel_ms;
  return PLK_OK;
}

int plk_debug_pairing(plk_ctx* ctx, const plk_g1* p, const plk_g2* q, size_t n, uint64_t* out) {
  PLK_API_BEGIN
  if (!p || !q || !out || n == 0 || n > 4096) return PLK_E_ARG;
  G2Aff qa;
  int st;
  if ((st = g2_from_abi(*q, qa))) return st;
  if (!g2_in_subgroup(qa)) return PLK_E_ARG;
  std::vector<Fp2> tab(kTabLen);
  if (!g2_prepare(qa, &tab[kTabH])) return PLK_E_ARG;
  std::memcpy(&tab[kTabB], &tab[kTabH], 2 * kMillerLines * sizeof(Fp2));
  frob_table(&tab[kTabFrob]);
  std::vector<G1In> pts(n);
  for (size_t i = 0; i < n; ++i)
    if ((st = g1_from_abi(p[i], pts[i]))) return st;
  if (!ctx) {
    for (size_t i = 0; i < n; ++i) pairing_value_host(&tab[kTabH], &tab[kTabFrob], pts[i], out + 72 * i);
    return PLK_OK;
  }
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  DevBuf d_tab, d_ws, d_pts, d_out;
  if ((st = key_on_device(ctx, nullptr, tab.data(), d_tab, false))) return st;
  const size_t tiles = ws_tiles(n);
  if ((st = d_ws.alloc(tiles * kTileWords * sizeof(uint32_t)))) return st;
  if ((st = d_pts.alloc(n * sizeof(plk_g1)))) return st;
  if ((st = d_out.alloc(n * 72 * sizeof(uint64_t)))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(d_pts.ptr, p, n * sizeof(plk_g1), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_pairing, dim3((unsigned)tiles), dim3(64), 0, s,
                     (const plk_g1*)d_pts.as<plk_g1>(), (uint32_t)n, 0, (const Fp2*)d_tab.as<Fp2>(),
                     d_ws.as<uint32_t>(), (uint8_t*)nullptr, d_out.as<uint64_t>());
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipMemcpyAsync(out, d_out.ptr, n * 72 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  return PLK_OK;
  PLK_API_END
}

int plk_debug_f12_op(plk_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n,
                     uint64_t* out) {
  PLK_API_BEGIN
  if (op < 0 || !a || !out || n == 0 || n > 4096) return PLK_E_ARG;
  const bool in_place = (op & kDbgInPlace) != 0;
  const int code = op & ~kDbgInPlace;
  if (code >= kDbgOps) return PLK_E_ARG;
  if (in_place && code != kDbgConj && code != kDbgFrob1 && code != kDbgFrob2) return PLK_E_ARG;
  const bool reads_b = dbg_reads_b(code);
  if (reads_b && !b) return PLK_E_ARG;
  for (size_t i = 0; i < 12 * n; ++i)
    if (!abi_canonical<FpCfg>(a + 6 * i) || (reads_b && !abi_canonical<FpCfg>(b + 6 * i))) return PLK_E_ARG;
  Fp2 frob[12];
  frob_table(frob);
  if (!ctx) {
    for (size_t j = 0; j < n; ++j) {
      F12Host m;
      const int r = f12_debug_op(m, code, in_place, a + 72 * j, reads_b ? b + 72 * j : nullptr, frob);
      f12_store_row(m, r, out + 72 * j);
    }
    return PLK_OK;
  }
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const size_t bytes = n * 72 * sizeof(uint64_t);
  DevBuf d_a, d_b, d_frob, d_ws, d_out;
  int st;
  if ((st = d_a.alloc(bytes)) || (st = d_out.alloc(bytes)) || (st = d_frob.alloc(sizeof frob))) return st;
  if ((st = d_ws.alloc(ws_tiles(n) * kTileWords * sizeof(uint32_t)))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(d_a.ptr, a, bytes, hipMemcpyHostToDevice, s));
  PLK_HIP_TRY(hipMemcpyAsync(d_frob.ptr, frob, sizeof frob, hipMemcpyHostToDevice, s));
  if (reads_b) {
    if ((st = d_b.alloc(bytes))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(d_b.ptr, b, bytes, hipMemcpyHostToDevice, s));
  }
  hipLaunchKernelGGL(k_f12_op, dim3((unsigned)ws_tiles(n)), dim3(64), 0, s, code, in_place ? 1 : 0,
                     (const uint64_t*)d_a.as<uint64_t>(), (const uint64_t*)d_b.as<uint64_t>(),
                     (uint32_t)n, (const Fp2*)d_frob.as<Fp2>(), d_ws.as<uint32_t>(),
                     d_out.as<uint64_t>());
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipMemcpyAsync(out, d_out.ptr, bytes, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));  // frob and the buffers live until here
  return PLK_OK;
  PLK_API_END
}

int plk_debug_miller(plk_ctx* ctx, const plk_g1* p0, const plk_g2* q0, const plk_g1* p1,
                     const plk_g2* q1, size_t n, uint64_t* out) {
  PLK_API_BEGIN
  if (!p0 || !q0 || (p1 && !q1) || !out || n == 0 || n > 4096) return PLK_E_ARG;
  const bool two = p1 != nullptr;
  std::vector<Fp2> tab(kTabLen);
  int st;
  for (int k = 0; k < (two ? 2 : 1); ++k) {
    G2Aff qa;
    if ((st = g2_from_abi(k ? *q1 : *q0, qa))) return st;
    if (!g2_in_subgroup(qa) || !g2_prepare(qa, &tab[k ? kTabB : kTabH])) return PLK_E_ARG;
  }
  if (!two) std::memcpy(&tab[kTabB], &tab[kTabH], 2 * kMillerLines * sizeof(Fp2));
  frob_table(&tab[kTabFrob]);
  std::vector<G1In> c(n), w(two ? n : 0);
  for (size_t i = 0; i < n; ++i)
    if ((st = g1_from_abi(p0[i], c[i])) || (two && (st = g1_from_abi(p1[i], w[i])))) return st;
  if (!ctx) {
    for (size_t i = 0; i < n; ++i) {
      F12Host m;
      if (two)  // pairing_check_host's call
        miller_check_host(m, &tab[kTabH], &tab[kTabB], c[i], w[i]);
      else  // pairing_value_host's
        miller_value_host(m, &tab[kTabH], c[i]);
      f12_store_row(m, 0, out + 72 * i);
    }
    return PLK_OK;
  }
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  DevBuf d_tab, d_ws, d_p0, d_p1, d_out;
  if ((st = key_on_device(ctx, nullptr, tab.data(), d_tab, false))) return st;
  if ((st = d_ws.alloc(ws_tiles(n) * kTileWords * sizeof(uint32_t)))) return st;
  if ((st = d_p0.alloc(n * sizeof(plk_g1))) || (st = d_out.alloc(n * 72 * sizeof(uint64_t)))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(d_p0.ptr, p0, n * sizeof(plk_g1), hipMemcpyHostToDevice, s));
  if (two) {
    if ((st = d_p1.alloc(n * sizeof(plk_g1)))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(d_p1.ptr, p1, n * sizeof(plk_g1), hipMemcpyHostToDevice, s));
  }
  hipLaunchKernelGGL(k_miller_value, dim3((unsigned)ws_tiles(n)), dim3(64), 0, s,
                     (const plk_g1*)d_p0.as<plk_g1>(), (const plk_g1*)d_p1.as<plk_g1>(), (uint32_t)n,
                     (const Fp2*)d_tab.as<Fp2>(), d_ws.as<uint32_t>(), d_out.as<uint64_t>());
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipMemcpyAsync(out, d_out.ptr, n * 72 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  return PLK_OK;
  PLK_API_END
}

}  // extern "C"
