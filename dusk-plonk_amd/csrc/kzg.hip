// kzg.hip — KZG openings as public operations (include/plk.h "KZG openings"): open one polynomial
// at arbitrary points, open it at every point of a domain, and fold openings into one pairing
// check. The reference describes the four operations of the scheme in src/commitment_scheme.rs
// and docs/notes-KZG10.md (commit, open, check, batch check).
//
// plk_kzg_open: per point the value (pk_eval) and the Ruffini quotient (pk_ruffini), the
// quotients committed kMaxSlots at a time through the SRS's own batch MSM.
//
// plk_kzg_open_domain (Feist-Khovratovich): with n = 2^log_n, omega the domain's generator and
// s_m = g1[m], the witness at omega^i is pi_i = sum_k omega^(ik) h_k with
//   h_k = sum_{m=0}^{n-2-k} f_{m+k+1} s_m  (k <= n - 2),  h_{n-1} = O,
// and the h_k are the upper half of one cyclic convolution of length 2n:
//   a_i = s_{n-1-i} (i < n), O otherwise;  b_j = f_j (j < n), 0 otherwise;  h_k = (a * b)_{n+k}.
//  1. A = G1-DFT_2n(a): the SRS's table for log_n, built on first use (KzgTable, affine form);
//  2. B = (2n)^-1 DFT_2n(b): the zero-padding Fr transform, the inverse's scale folded in;
//  3. U_t = [B_t] A_t: the batched GLV multiplication of g1_mul.hip (valid on G1: the SRS
//     prefix is tested once unless it is known to be in G1);
//  4. c = unscaled G1-IDFT_2n(U);  5. h = c[n, 2n);  6. pi = G1-DFT_n(h)  (g1_ntt.hip, the
//     affine-between-levels form: all these points lie in G1);
//  7. one batch inversion to the affine ABI form;  8. the values are DFT_n(f).
//
// plk_kzg_open_cosets (the same paper's multiproofs): with l = 2^log_l, r = n / l and psi = omega^l,
// the witness of the coset omega^j <omega^r> is pi_j = [f div (X^l - psi^j)](tau) = sum_k psi^(jk) H_k,
//   H_k = sum_{a<l} sum_{b=0}^{r-2-k} f_(a+(b+k+1)l) s_(a+bl)  (k <= r - 2),  H_(r-1) = O:
// for every residue a the sum above with n -> r on f^(a)_c = f_(a+cl) and s^(a)_b = s_(a+bl).
//  1. Table[a] = G1-DFT_2r(s^(a)_(r-1), .., s^(a)_0, O, .., O), a < l: l transforms as one batch
//     (g1_ntt_run_batch), 2n affine points in [a][t] layout, kept beside open_domain's tables;
//  2. B^(a) = (2r)^-1 DFT_2r(f^(a) zero-padded): one batched Fr transform;
//  3. the 2n products [B^(a)_t] Table[a]_t, then U_t = their sum over a (g1_colsum.hip);
//  4. c = unscaled G1-IDFT_2r(U);  H = c[r, 2r);  pi = G1-DFT_r(H);  5. one batch inversion.
// The multiplications are open_domain's 2n; the G1 transforms have log 2r and log r levels
// instead of log 2n and log n, and a level costs one multiplication chain whatever its width.
// plk_kzg_fold_cosets: the verifier's side, see include/plk.h.
// This file's scratch is stream-ordered (hipMallocAsync / hipFreeAsync); g1_mul_dev, under step 3
// and under every level of the transforms, brings its own buffers and waits for the stream.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ffr.hpp"
#include "internal.hpp"
#include "msm_common.hpp"
#include "prover.hpp"
#include "transcript.hpp"

using namespace plk;

namespace plk {
int srs_batch_affine(const G1xyzz* temp, uint64_t n, Fp* pref, G1Affine* out, uint8_t* out_inf,
                     hipStream_t stream);
}

namespace {

constexpr uint32_t kMaxLogOpen = 20;
// The transforms' form: every point they meet is a multiple of SRS points known to be in G1, so the
// affine-between-levels form with the endomorphism split applies. Measured against the XYZZ form
// inside open_domain at 2^8 / 2^12 / 2^16 (profiles/kzg_open.jsonl): 85 / 120 / 191 ms
// against 117 / 181 / 250 ms warm.
constexpr G1NttForm kForm = G1NttForm::kGlv;
constexpr size_t kMaxFold = (size_t)1 << 24;

bool all_canonical(const plk_fr* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!abi_canonical<FrCfg>(v[i].l)) return false;
  return true;
}

plk_g1 g1_identity_abi() {
  plk_g1 p;
  g1_store(fe_zero<FpCfg>(), fe_zero<FpCfg>(), false, &p);
  return p;
}

// the affine device points [0, n) -> host ABI points
int download_points(const G1Affine* d_pts, const uint8_t* d_inf, size_t n, plk_g1* out, hipStream_t s) {
  std::vector<G1Affine> res(n);
  std::vector<uint8_t> rinf(n);
  PLK_HIP_TRY(hipMemcpyAsync(res.data(), d_pts, n * sizeof(G1Affine), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(hipMemcpyAsync(rinf.data(), d_inf, n, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  for (size_t i = 0; i < n; ++i) g1_store(res[i].x, res[i].y, !rinf[i], &out[i]);
  return PLK_OK;
}

// The table of (srs, log_n): A = G1-DFT_2n(s_{n-1}, .., s_0, O, .., O) in affine form.
int build_table(plk_srs* srs, uint32_t log_n, KzgTable& tab, hipStream_t s) {
  const uint64_t n = 1ull << log_n, n2 = 2 * n;
  int st;
  if ((st = tab.points.alloc(n2 * sizeof(G1Affine)))) return st;
  if ((st = tab.inf.alloc(n2))) return st;
  AsyncBuf a, pref;
  if ((st = a.alloc(n2 * sizeof(G1xyzz), s))) return st;
  if ((st = pref.alloc(n2 * sizeof(Fp), s))) return st;
  if ((st = g1_xyzz_load(srs->points.as<G1Affine>(), srs->inf.as<uint8_t>(), n - 1, true, n, n2, a.as<G1xyzz>(), s)))
    return st;
  if ((st = g1_ntt_run(srs->ctx, a.as<G1xyzz>(), log_n + 1, 1, s, true, kForm))) return st;
  return srs_batch_affine(a.as<G1xyzz>(), n2, pref.as<Fp>(), tab.points.as<G1Affine>(), tab.inf.as<uint8_t>(), s);
}

// 128-bit weights for a fold, rho_0 = 1: the verifier's derivation (verifier.hip random_weights) —
// a merlin transcript over the count, every opening's point and value, and 32 bytes of OS entropy,
// so nobody who fixed the openings beforehand knows the weights
void random_weights(const plk_fr* points, const plk_fr* values, size_t count, std::vector<Fr>& rho) {
  uint8_t seed[32];
  os_entropy(seed);
  Transcript t("plk-kzg-fold");
  t.append_u64("count", count);
  for (size_t k = 0; k < count; ++k) {
    t.append_scalar("z", fr_from_abi(points[k]));
    t.append_scalar("y", fr_from_abi(values[k]));
  }
  t.append_message("entropy", seed, sizeof seed);
  rho.assign(count, fe_one<FrCfg>());
  for (size_t j = 1; j < count; ++j) {
    uint8_t b[16];
    t.challenge_bytes("rho", b, 16);
    Fr r = fe_zero<FrCfg>();
    for (int i = 0; i < 4; ++i)
      r.v[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
               ((uint32_t)b[4 * i + 3] << 24);
    rho[j] = fe_to_mont(r);
  }
}

// ---- coset openings --------------------------------------------------------------------------
constexpr uint32_t kNttChunk = 32768;  // transforms per ntt_run_batch call (the grid's y extent)

// out[a 2r + i] = s_(a + (r - 1 - i) l) for i < r, the identity for r <= i < 2r; a < l
__global__ void __launch_bounds__(256) k_coset_srs_load(const G1Affine* __restrict__ pts,
                                                        const uint8_t* __restrict__ inf, uint32_t log_l,
                                                        uint32_t log_r, G1xyzz* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >> (log_l + log_r + 1)) return;
  const uint64_t r = 1ull << log_r, a = g >> (log_r + 1), i = g & (2 * r - 1);
  G1xyzz p = xyzz_infinity();
  if (i < r) {
    const uint64_t k = a + ((r - 1 - i) << log_l);
    if (!inf[k]) {
      Fp x, y;
      ld_aff(&pts[k], x, y);
      p = xyzz_from_affine(G1Affine{x, y});
    }
  }
  st_xyzz(&out[g], p);
}

// out[a r + c] = f_(a + c l), zero from len on; a < l, c < r
__global__ void __launch_bounds__(256) k_coset_coeffs(const Fr* __restrict__ f, uint64_t len, uint32_t log_l,
                                                      uint32_t log_r, Fr* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >> (log_l + log_r)) return;
  const uint64_t a = g >> log_r, c = g & ((1ull << log_r) - 1), k = a + (c << log_l);
  uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
  if (k < len) {
    const uint4* src = reinterpret_cast<const uint4*>(&f[k]);
    lo = src[0];
    hi = src[1];
  }
  uint4* dst = reinterpret_cast<uint4*>(&out[g]);
  dst[0] = lo;
  dst[1] = hi;
}

// `count` transforms of d->n points, vector v from in + v in_stride (len_in values) to out + v d->n,
// at most kNttChunk per launch; scratch: 2 d->n min(count, kNttChunk) elements
int ntt_many(plk_domain* d, const Fr* in, uint64_t in_stride, size_t len_in, Fr* out, int dir, uint64_t count,
             Fr* scratch, hipStream_t s) {
  NttBatch b;
  b.in_stride = in_stride;
  b.out_stride = d->n;
  for (uint64_t v = 0; v < count; v += kNttChunk) {
    const uint32_t m = (uint32_t)(count - v < kNttChunk ? count - v : kNttChunk);
    const int st = ntt_run_batch(d, in + v * in_stride, out + v * d->n, len_in, dir, 0, scratch, s, m, b);
    if (st) return st;
  }
  return PLK_OK;
}

// The table of (srs, log_n, log_l), l > 1: residue a's transform at [a 2r, (a + 1) 2r), affine.
int build_coset_table(plk_srs* srs, uint32_t log_n, uint32_t log_l, KzgTable& tab, hipStream_t s) {
  const uint64_t n2 = 2ull << log_n;
  const uint32_t log_r = log_n - log_l;
  int st;
  if ((st = tab.points.alloc(n2 * sizeof(G1Affine)))) return st;
  if ((st = tab.inf.alloc(n2))) return st;
  AsyncBuf a, pref;
  if ((st = a.alloc(n2 * sizeof(G1xyzz), s))) return st;
  if ((st = pref.alloc(n2 * sizeof(Fp), s))) return st;
  hipLaunchKernelGGL(k_coset_srs_load, dim3(cdiv(n2, 256)), dim3(256), 0, s, (const G1Affine*)srs->points.as<G1Affine>(),
                     (const uint8_t*)srs->inf.as<uint8_t>(), log_l, log_r, a.as<G1xyzz>());
  PLK_HIP_TRY(hipGetLastError());
  if ((st = g1_ntt_run_batch(srs->ctx, a.as<G1xyzz>(), log_r + 1, 1ull << log_l, 1, s, true, kForm))) return st;
  return srs_batch_affine(a.as<G1xyzz>(), n2, pref.as<Fp>(), tab.points.as<G1Affine>(), tab.inf.as<uint8_t>(), s);
}

// the weights of plk_kzg_fold_cosets, as random_weights with a label of its own
void random_coset_weights(uint32_t log_l, const plk_fr* shifts, const plk_fr* values, size_t count,
                          std::vector<Fr>& rho) {
  uint8_t seed[32];
  os_entropy(seed);
  const size_t l = (size_t)1 << log_l;
  Transcript t("plk-kzg-fold-cosets");
  t.append_u64("count", count);
  t.append_u64("log_l", log_l);
  for (size_t k = 0; k < count; ++k) {
    t.append_scalar("z", fr_from_abi(shifts[k]));
    for (size_t i = 0; i < l; ++i) t.append_scalar("y", fr_from_abi(values[k * l + i]));
  }
  t.append_message("entropy", seed, sizeof seed);
  rho.assign(count, fe_one<FrCfg>());
  for (size_t j = 1; j < count; ++j) {
    uint8_t b[16];
    t.challenge_bytes("rho", b, 16);
    Fr r = fe_zero<FrCfg>();
    for (int i = 0; i < 4; ++i)
      r.v[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
               ((uint32_t)b[4 * i + 3] << 24);
    rho[j] = fe_to_mont(r);
  }
}

}  // namespace

extern "C" {

int plk_kzg_open(plk_srs* srs, const plk_fr* coeffs, size_t len, const plk_fr* points, size_t count,
                 plk_fr* values, plk_g1* witnesses) {
  PLK_API_BEGIN
  if (!srs || (!coeffs && len) || (count && (!points || !values || !witnesses))) return PLK_E_ARG;
  if (!all_canonical(coeffs, len) || !all_canonical(points, count)) return PLK_E_ARG;
  // Coefficients::degree() ignores trailing zeros; as plk_commit, the polynomial must fit the SRS
  size_t eff = len;
  while (eff > 0) {
    const plk_fr& c = coeffs[eff - 1];
    if (c.l[0] | c.l[1] | c.l[2] | c.l[3]) break;
    --eff;
  }
  if (eff > srs->n) return PLK_E_DEGREE;
  if (count == 0) return PLK_OK;
  if (eff <= 1) {  // a constant: its own value everywhere, the zero quotient
    const plk_fr zero = fr_to_abi(fe_zero<FrCfg>());
    for (size_t k = 0; k < count; ++k) {
      values[k] = eff ? coeffs[0] : zero;
      witnesses[k] = g1_identity_abi();
    }
    return PLK_OK;
  }
  plk_ctx* ctx = srs->ctx;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  const size_t qlen = eff - 1;
  AsyncBuf f, q, tmp, scan, partial, vals;
  int st;
  if ((st = f.alloc(eff * sizeof(Fr), s))) return st;
  if ((st = q.alloc((size_t)kMaxSlots * qlen * sizeof(Fr), s))) return st;
  if ((st = tmp.alloc(eff * sizeof(Fr), s))) return st;
  if ((st = scan.alloc(pk_scan_tmp_elems(eff) * sizeof(Fr), s))) return st;
  if ((st = partial.alloc((size_t)kMaxSlots * pk_eval_max_blocks(eff) * sizeof(Fr), s))) return st;
  if ((st = vals.alloc(kMaxSlots * sizeof(Fr), s))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(f.ptr, coeffs, eff * sizeof(Fr), hipMemcpyHostToDevice, s));
  static_assert(kMaxSlots <= (uint32_t)kMaxEval, "one evaluation batch per commit batch");
  for (size_t base = 0; base < count; base += kMaxSlots) {
    const size_t m = count - base < kMaxSlots ? count - base : kMaxSlots;
    EvalBatch eb{};
    const Fr* ptrs[kMaxSlots];
    size_t lens[kMaxSlots];
    for (size_t k = 0; k < m; ++k) {
      const Fr z = fr_from_abi(points[base + k]);
      eb.poly[k] = f.fr();
      eb.len[k] = eff;
      eb.x[k] = z;
      Fr* qk = q.fr() + k * qlen;
      ptrs[k] = qk;
      lens[k] = qlen;
      if (fe_is_zero(z)) {  // division by X: q_k = c_(k+1), as opening.hip
        PLK_HIP_TRY(hipMemcpyAsync(qk, f.fr() + 1, qlen * sizeof(Fr), hipMemcpyDeviceToDevice, s));
      } else if ((st = pk_ruffini(f.fr(), eff, z, qk, tmp.fr(), scan.fr(), s))) {
        return st;
      }
    }
    if ((st = pk_eval(eb, (uint32_t)m, eff, partial.fr(), vals.fr(), s))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(values + base, vals.ptr, m * sizeof(Fr), hipMemcpyDeviceToHost, s));
    int sts[kMaxSlots];
    if ((st = msm_run_batch(srs, *srs->ws, ptrs, lens, lens, m, witnesses + base, sts, s))) return st;
    PLK_HIP_TRY(stream_wait(s));
  }
  return PLK_OK;
  PLK_API_END
}

int plk_kzg_open_domain(plk_srs* srs, uint32_t log_n, const plk_fr* coeffs, size_t len, plk_fr* values,
                        plk_g1* witnesses, uint64_t* bad_index) {
  PLK_API_BEGIN
  if (bad_index) *bad_index = ~0ull;
  if (!srs || (!coeffs && len) || !values || !witnesses) return PLK_E_ARG;
  if (log_n < 1 || log_n > kMaxLogOpen) return PLK_E_ARG;
  const uint64_t n = 1ull << log_n, n2 = 2 * n;
  if (len > n || !all_canonical(coeffs, len)) return PLK_E_ARG;
  if (srs->n < n) return PLK_E_DEGREE;
  plk_ctx* ctx = srs->ctx;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  plk_domain *dom = nullptr, *dom2 = nullptr;
  int st;
  if ((st = plk_domain_get(ctx, log_n, &dom))) return st;
  if ((st = plk_domain_get(ctx, log_n + 1, &dom2))) return st;
  TimingEvents<5> ev;
  if ((st = ev.create())) return st;
  PLK_HIP_TRY(hipEventRecord(ev.e[0], s));
  auto it = srs->kzg_tables.find(log_n);
  const bool fresh = it == srs->kzg_tables.end();
  if (fresh) {
    bool any = false;
    uint64_t idx = 0;
    if ((st = srs_ensure_g1_prefix(srs, n, &any, &idx))) return st;
    if (any) {
      if (bad_index) *bad_index = idx;
      return PLK_E_ARG;
    }
    KzgTable tab;
    if ((st = build_table(srs, log_n, tab, s))) return st;
    it = srs->kzg_tables.emplace(log_n, std::move(tab)).first;
  }
  const KzgTable& tab = it->second;
  PLK_HIP_TRY(hipEventRecord(ev.e[1], s));
  const size_t flen = len ? len : 1;  // the zero polynomial as one zero coefficient
  AsyncBuf f, bsc, vals, ntt_tmp, upts, uinf, c, pref, wpts, winf;
  if ((st = f.alloc(flen * sizeof(Fr), s))) return st;
  if ((st = bsc.alloc(n2 * sizeof(Fr), s))) return st;
  if ((st = vals.alloc(n * sizeof(Fr), s))) return st;
  if ((st = ntt_tmp.alloc(2 * n2 * sizeof(Fr), s))) return st;
  if ((st = upts.alloc(n2 * sizeof(G1Affine), s))) return st;
  if ((st = uinf.alloc(n2, s))) return st;
  if ((st = c.alloc(n2 * sizeof(G1xyzz), s))) return st;
  if ((st = pref.alloc(n * sizeof(Fp), s))) return st;
  if ((st = wpts.alloc(n * sizeof(G1Affine), s))) return st;
  if ((st = winf.alloc(n, s))) return st;
  if (len)
    PLK_HIP_TRY(hipMemcpyAsync(f.ptr, coeffs, len * sizeof(Fr), hipMemcpyHostToDevice, s));
  else
    PLK_HIP_TRY(hipMemsetAsync(f.ptr, 0, sizeof(Fr), s));
  // the values, and B with the 2n-point inverse's scale
  if ((st = ntt_run(dom, f.fr(), vals.fr(), flen, 1, 0, ntt_tmp.fr(), s, 1))) return st;
  if ((st = ntt_run(dom2, f.fr(), bsc.fr(), flen, 1, 0, ntt_tmp.fr(), s, 1))) return st;
  if ((st = pk_scale_copy(bsc.fr(), dom2->n_inv, bsc.fr(), n2, s))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(values, vals.ptr, n * sizeof(Fr), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(hipEventRecord(ev.e[2], s));
  // U_t = [B_t] A_t
  if ((st = g1_mul_dev(ctx, tab.points.as<G1Affine>(), tab.inf.as<uint8_t>(), bsc.fr(), n2, upts.as<G1Affine>(),
                       uinf.as<uint8_t>(), s)))
    return st;
  PLK_HIP_TRY(hipEventRecord(ev.e[3], s));
  // c = IDFT_2n(U), h = c[n, 2n), pi = DFT_n(h)
  if ((st = g1_xyzz_load(upts.as<G1Affine>(), uinf.as<uint8_t>(), 0, false, n2, n2, c.as<G1xyzz>(), s))) return st;
  if ((st = g1_ntt_run(ctx, c.as<G1xyzz>(), log_n + 1, -1, s, false, kForm))) return st;
  G1xyzz* h = c.as<G1xyzz>() + n;
  if ((st = g1_ntt_run(ctx, h, log_n, 1, s, true, kForm))) return st;
  if ((st = srs_batch_affine(h, n, pref.as<Fp>(), wpts.as<G1Affine>(), winf.as<uint8_t>(), s))) return st;
  PLK_HIP_TRY(hipEventRecord(ev.e[4], s));
  if ((st = download_points(wpts.as<G1Affine>(), winf.as<uint8_t>(), n, witnesses, s))) return st;
  float t01 = 0.f, t12 = 0.f, t23 = 0.f, t34 = 0.f;
  (void)hipEventElapsedTime(&t01, ev.e[0], ev.e[1]);
  (void)hipEventElapsedTime(&t12, ev.e[1], ev.e[2]);
  (void)hipEventElapsedTime(&t23, ev.e[2], ev.e[3]);
  (void)hipEventElapsedTime(&t34, ev.e[3], ev.e[4]);
  ctx->kzg_table_ms = fresh ? t01 : 0.f;
  ctx->kzg_transform_ms = t12 + t34;
  ctx->kzg_mul_ms = t23;
  return PLK_OK;
  PLK_API_END
}

int plk_kzg_open_cosets(plk_srs* srs, uint32_t log_n, uint32_t log_l, const plk_fr* coeffs, size_t len,
                        plk_fr* values, plk_g1* witnesses, uint64_t* bad_index) {
  PLK_API_BEGIN
  if (bad_index) *bad_index = ~0ull;
  if (!srs || (!coeffs && len) || !values || !witnesses) return PLK_E_ARG;
  if (log_n < 1 || log_n > kMaxLogOpen || log_l > log_n) return PLK_E_ARG;
  const uint64_t n = 1ull << log_n, n2 = 2 * n, l = 1ull << log_l;
  const uint32_t log_r = log_n - log_l;
  const uint64_t r = 1ull << log_r, r2 = 2 * r;
  if (len > n || !all_canonical(coeffs, len)) return PLK_E_ARG;
  if (srs->n < n) return PLK_E_DEGREE;
  plk_ctx* ctx = srs->ctx;
  DeviceGuard g(ctx->device);
  hipStream_t s = ctx->stream;
  plk_domain *dom = nullptr, *dom2 = nullptr;
  int st;
  if ((st = plk_domain_get(ctx, log_n, &dom))) return st;
  if ((st = plk_domain_get(ctx, log_r + 1, &dom2))) return st;
  TimingEvents<5> ev;
  if ((st = ev.create())) return st;
  PLK_HIP_TRY(hipEventRecord(ev.e[0], s));
  // log_l = 0 is open_domain's table under open_domain's key; r = 1 needs none
  const uint32_t key = log_n | (log_l << 8);
  auto it = srs->kzg_tables.find(key);
  const bool fresh = it == srs->kzg_tables.end();
  if (fresh) {
    bool any = false;
    uint64_t idx = 0;
    if ((st = srs_ensure_g1_prefix(srs, n, &any, &idx))) return st;
    if (any) {
      if (bad_index) *bad_index = idx;
      return PLK_E_ARG;
    }
    if (r > 1) {
      KzgTable tab;
      if ((st = log_l ? build_coset_table(srs, log_n, log_l, tab, s) : build_table(srs, log_n, tab, s))) return st;
      it = srs->kzg_tables.emplace(key, std::move(tab)).first;
    }
  }
  PLK_HIP_TRY(hipEventRecord(ev.e[1], s));
  const size_t flen = len ? len : 1;  // the zero polynomial as one zero coefficient
  AsyncBuf f, fa, bsc, vals, ntt_tmp, upts, uinf, c, pref, wpts, winf;
  if ((st = f.alloc(flen * sizeof(Fr), s))) return st;
  if ((st = vals.alloc(n * sizeof(Fr), s))) return st;
  if ((st = ntt_tmp.alloc(2 * n2 * sizeof(Fr), s))) return st;
  if (len)
    PLK_HIP_TRY(hipMemcpyAsync(f.ptr, coeffs, len * sizeof(Fr), hipMemcpyHostToDevice, s));
  else
    PLK_HIP_TRY(hipMemsetAsync(f.ptr, 0, sizeof(Fr), s));
  if ((st = ntt_run(dom, f.fr(), vals.fr(), flen, 1, 0, ntt_tmp.fr(), s, 1))) return st;
  PLK_HIP_TRY(hipMemcpyAsync(values, vals.ptr, n * sizeof(Fr), hipMemcpyDeviceToHost, s));
  if (r == 1) {  // one coset, the whole domain: f = I, the quotient is zero
    PLK_HIP_TRY(hipEventRecord(ev.e[2], s));
    PLK_HIP_TRY(stream_wait(s));
    witnesses[0] = g1_identity_abi();
    float t12 = 0.f;
    (void)hipEventElapsedTime(&t12, ev.e[1], ev.e[2]);
    ctx->kzg_table_ms = 0.f;
    ctx->kzg_transform_ms = t12;
    ctx->kzg_mul_ms = 0.f;
    return PLK_OK;
  }
  const KzgTable& tab = it->second;
  if ((st = fa.alloc(n * sizeof(Fr), s))) return st;
  if ((st = bsc.alloc(n2 * sizeof(Fr), s))) return st;
  if ((st = upts.alloc(n2 * sizeof(G1Affine), s))) return st;
  if ((st = uinf.alloc(n2, s))) return st;
  if ((st = c.alloc(r2 * sizeof(G1xyzz), s))) return st;
  if ((st = pref.alloc(r * sizeof(Fp), s))) return st;
  if ((st = wpts.alloc(r * sizeof(G1Affine), s))) return st;
  if ((st = winf.alloc(r, s))) return st;
  // B^(a), a < l, with the 2r-point inverse's scale: row a at [a 2r, (a + 1) 2r)
  hipLaunchKernelGGL(k_coset_coeffs, dim3(cdiv(n, 256)), dim3(256), 0, s, (const Fr*)f.fr(), (uint64_t)len, log_l,
                     log_r, fa.fr());
  PLK_HIP_TRY(hipGetLastError());
  if ((st = ntt_many(dom2, fa.fr(), r, r, bsc.fr(), 1, l, ntt_tmp.fr(), s))) return st;
  if ((st = pk_scale_copy(bsc.fr(), dom2->n_inv, bsc.fr(), n2, s))) return st;
  PLK_HIP_TRY(hipEventRecord(ev.e[2], s));
  // the 2n products [B^(a)_t] Table[a]_t
  if ((st = g1_mul_dev(ctx, tab.points.as<G1Affine>(), tab.inf.as<uint8_t>(), bsc.fr(), n2, upts.as<G1Affine>(),
                       uinf.as<uint8_t>(), s)))
    return st;
  PLK_HIP_TRY(hipEventRecord(ev.e[3], s));
  // U = their sum over a; c = IDFT_2r(U), H = c[r, 2r), pi = DFT_r(H)
  if ((st = g1_colsum_dev(upts.as<G1Affine>(), uinf.as<uint8_t>(), l, r2, c.as<G1xyzz>(), s))) return st;
  if ((st = g1_ntt_run(ctx, c.as<G1xyzz>(), log_r + 1, -1, s, false, kForm))) return st;
  G1xyzz* h = c.as<G1xyzz>() + r;
  if ((st = g1_ntt_run(ctx, h, log_r, 1, s, true, kForm))) return st;
  if ((st = srs_batch_affine(h, r, pref.as<Fp>(), wpts.as<G1Affine>(), winf.as<uint8_t>(), s))) return st;
  PLK_HIP_TRY(hipEventRecord(ev.e[4], s));
  if ((st = download_points(wpts.as<G1Affine>(), winf.as<uint8_t>(), r, witnesses, s))) return st;
  float t01 = 0.f, t12 = 0.f, t23 = 0.f, t34 = 0.f;
  (void)hipEventElapsedTime(&t01, ev.e[0], ev.e[1]);
  (void)hipEventElapsedTime(&t12, ev.e[1], ev.e[2]);
  (void)hipEventElapsedTime(&t23, ev.e[2], ev.e[3]);
  (void)hipEventElapsedTime(&t34, ev.e[3], ev.e[4]);
  ctx->kzg_table_ms = fresh ? t01 : 0.f;
  ctx->kzg_transform_ms = t12 + t34;
  ctx->kzg_mul_ms = t23;
  return PLK_OK;
  PLK_API_END
}

int plk_kzg_fold_cosets(plk_srs* srs, uint32_t log_l, const plk_g1* commitments, const plk_fr* shifts,
                        const plk_fr* values, const plk_g1* witnesses, size_t count, const plk_fr* weights,
                        plk_kzg_pair* out) {
  PLK_API_BEGIN
  if (!srs || !commitments || !shifts || !values || !witnesses || !out) return PLK_E_ARG;
  if (count == 0 || count > kMaxFold || log_l > kMaxLogOpen) return PLK_E_ARG;
  const size_t l = (size_t)1 << log_l;
  if (count > kMaxFold >> log_l || srs->n < l) return PLK_E_ARG;
  const size_t cells = count * l;
  if (!all_canonical(shifts, count) || !all_canonical(values, cells)) return PLK_E_ARG;
  if (weights && !all_canonical(weights, count)) return PLK_E_ARG;
  for (size_t k = 0; k < count; ++k)
    if (!(shifts[k].l[0] | shifts[k].l[1] | shifts[k].l[2] | shifts[k].l[3])) return PLK_E_ARG;
  std::vector<Fr> rho;
  if (weights) {
    rho.resize(count);
    for (size_t k = 0; k < count; ++k) rho[k] = fr_from_abi(weights[k]);
  } else {
    random_coset_weights(log_l, shifts, values, count, rho);
  }
  // z_k^-1 by one inversion (prefix products), z_k^l by log_l squarings
  std::vector<Fr> z(count), zinv(count), zl(count);
  Fr acc = fe_one<FrCfg>();
  for (size_t k = 0; k < count; ++k) {
    z[k] = fr_from_abi(shifts[k]);
    zinv[k] = acc;
    acc = fe_mul(acc, z[k]);
    zl[k] = z[k];
    for (uint32_t b = 0; b < log_l; ++b) zl[k] = fe_sqr(zl[k]);
  }
  acc = fe_inv(acc);
  for (size_t k = count; k-- > 0;) {
    zinv[k] = fe_mul(zinv[k], acc);
    acc = fe_mul(acc, z[k]);
  }
  plk_ctx* ctx = srs->ctx;
  std::vector<Fr> p(l);
  {
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    AsyncBuf v, c, tmp, d_rho, d_zinv, d_p;
    int st;
    if ((st = v.alloc(cells * sizeof(Fr), s))) return st;
    if ((st = d_rho.alloc(count * sizeof(Fr), s))) return st;
    if ((st = d_zinv.alloc(count * sizeof(Fr), s))) return st;
    if ((st = d_p.alloc(l * sizeof(Fr), s))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(v.ptr, values, cells * sizeof(Fr), hipMemcpyHostToDevice, s));
    PLK_HIP_TRY(hipMemcpyAsync(d_rho.ptr, rho.data(), count * sizeof(Fr), hipMemcpyHostToDevice, s));
    PLK_HIP_TRY(hipMemcpyAsync(d_zinv.ptr, zinv.data(), count * sizeof(Fr), hipMemcpyHostToDevice, s));
    const Fr* rows = v.fr();
    if (log_l) {  // c_k = IDFT_l(row k); at l = 1 the row is its own interpolant
      plk_domain* dom = nullptr;
      if ((st = plk_domain_get(ctx, log_l, &dom))) return st;
      const size_t chunk = count < kNttChunk ? count : kNttChunk;
      if ((st = c.alloc(cells * sizeof(Fr), s))) return st;
      if ((st = tmp.alloc(2 * l * chunk * sizeof(Fr), s))) return st;
      if ((st = ntt_many(dom, v.fr(), l, l, c.fr(), -1, count, tmp.fr(), s))) return st;
      rows = c.fr();
    }
    if ((st = fr_interp_reduce_dev(rows, d_rho.fr(), d_zinv.fr(), count, l, d_p.fr(), s))) return st;
    PLK_HIP_TRY(hipMemcpyAsync(p.data(), d_p.ptr, l * sizeof(Fr), hipMemcpyDeviceToHost, s));
    PLK_HIP_TRY(stream_wait(s));
  }
  // C = sum rho_k C_k + sum (rho_k z_k^l) W_k - sum P_i g1[i] over 2 count + l points, and
  // W = sum rho_k W_k over count more: one batch of two ranges
  const size_t n_c = 2 * count + l, total = n_c + count;
  std::vector<plk_g1> pts(total);
  std::vector<plk_fr> sc(total);
  for (size_t k = 0; k < count; ++k) {
    pts[k] = commitments[k];
    sc[k] = fr_to_abi(rho[k]);
    pts[count + k] = witnesses[k];
    sc[count + k] = fr_to_abi(fe_mul(rho[k], zl[k]));
    pts[n_c + k] = witnesses[k];
    sc[n_c + k] = sc[k];
  }
  int st;
  if ((st = plk_srs_points(srs, 0, l, pts.data() + 2 * count))) return st;
  for (size_t i = 0; i < l; ++i) sc[2 * count + i] = fr_to_abi(fe_neg(p[i]));
  const size_t starts[2] = {0, n_c}, lens[2] = {n_c, count};
  plk_g1 res[2];
  if ((st = plk_msm_points_ranges(ctx, pts.data(), sc.data(), total, starts, lens, 2, res))) return st;
  out->c = res[0];
  out->w = res[1];
  return PLK_OK;
  PLK_API_END
}

int plk_kzg_last_open_ms(plk_ctx* ctx, float* transform_ms, float* mul_ms, float* table_ms) {
  if (!ctx) return PLK_E_ARG;
  if (transform_ms) *transform_ms = ctx->kzg_transform_ms;
  if (mul_ms) *mul_ms = ctx->kzg_mul_ms;
  if (table_ms) *table_ms = ctx->kzg_table_ms;
  return PLK_OK;
}

int plk_kzg_fold(plk_ctx* ctx, const plk_g1* g, const plk_g1* commitments, const plk_fr* points,
                 const plk_fr* values, const plk_g1* witnesses, size_t count, const plk_fr* weights,
                 plk_kzg_pair* out) {
  PLK_API_BEGIN
  if (!ctx || !g || !commitments || !points || !values || !witnesses || !out) return PLK_E_ARG;
  if (count == 0 || count > kMaxFold) return PLK_E_ARG;
  if (!all_canonical(points, count) || !all_canonical(values, count)) return PLK_E_ARG;
  if (weights && !all_canonical(weights, count)) return PLK_E_ARG;
  std::vector<Fr> rho;
  if (weights) {
    rho.resize(count);
    for (size_t k = 0; k < count; ++k) rho[k] = fr_from_abi(weights[k]);
  } else {
    random_weights(points, values, count, rho);
  }
  // C = sum rho_k C_k + sum (rho_k z_k) W_k - (sum rho_k y_k) g over 2 count + 1 points, and
  // W = sum rho_k W_k over count more: one batch of two ranges
  const size_t n_c = 2 * count + 1, total = n_c + count;
  std::vector<plk_g1> pts(total);
  std::vector<plk_fr> sc(total);
  Fr ysum = fe_zero<FrCfg>();
  for (size_t k = 0; k < count; ++k) {
    pts[k] = commitments[k];
    sc[k] = fr_to_abi(rho[k]);
    pts[count + k] = witnesses[k];
    sc[count + k] = fr_to_abi(fe_mul(rho[k], fr_from_abi(points[k])));
    ysum = fe_add(ysum, fe_mul(rho[k], fr_from_abi(values[k])));
    pts[n_c + k] = witnesses[k];
    sc[n_c + k] = sc[k];
  }
  pts[2 * count] = *g;
  sc[2 * count] = fr_to_abi(fe_neg(ysum));
  const size_t starts[2] = {0, n_c}, lens[2] = {n_c, count};
  plk_g1 res[2];
  // refuses a finite point that is off the curve or not canonical, and an infinity word above 1
  const int st = plk_msm_points_ranges(ctx, pts.data(), sc.data(), total, starts, lens, 2, res);
  if (st != PLK_OK) return st;
  out->c = res[0];
  out->w = res[1];
  return PLK_OK;
  PLK_API_END
}

}  // extern "C"
