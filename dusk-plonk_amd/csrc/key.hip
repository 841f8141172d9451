// key.hip — the proving key: PlonkKey::compile_with_circuit (src/key.rs:63-327) as one function
// per step, each filling fields of the plk_key under construction, and the quotient domain's
// block transforms that key compilation, the prover's round 3 and plk_debug_block_eval share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "ffr.hpp"
#include "prover.hpp"

namespace plk {

void coset_shifts(const plk_domain* dom, int blocks, Fr* s_m) {
  Fr w8n;
  fr_root_of_unity(dom->log_n + 3, w8n);
  s_m[0] = dom->g;
  for (int m = 1; m < blocks; ++m) s_m[m] = fe_mul(s_m[m - 1], w8n);
}

int coset_blocks_fwd(plk_domain* dom, const Fr* in, Fr* out, uint64_t len, const Fr* table,
                     int blocks, Fr* scratch, hipStream_t s) {
  const uint64_t n = dom->n;
  NttBatch b;
  b.in_stride = 0;  // the same coefficients for every block
  b.out_stride = n;
  b.pre = table;
  b.pre_stride = n + 8;
  return ntt_run_batch(dom, in, out, len, 1, 1, scratch, s, (uint32_t)blocks, b);
}

void poly_from_roots(const Fr* c, int count, Fr* out) {
  out[0] = fe_one<FrCfg>();
  for (int j = 0; j < count; ++j) {  // times (X - c_j)
    out[j + 1] = fe_zero<FrCfg>();
    for (int l = j + 1; l >= 1; --l) out[l] = fe_sub(out[l - 1], fe_mul(out[l], c[j]));
    out[0] = fe_neg(fe_mul(out[0], c[j]));
  }
}

namespace {

uint32_t log2_ceil(uint64_t x) {
  uint32_t k = 0;
  while ((1ull << k) < x) ++k;
  return k;
}

// sigma values k_col(next) * w^gate(next) from wire codes (4*gate + col)
__global__ void k_sigma_values(const uint32_t* __restrict__ codes, const Fr* __restrict__ el,
                               uint64_t n, Fr k1, Fr k2, Fr k3, Fr* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * n) return;
  const uint32_t code = codes[i];
  const uint32_t g = code >> 2, col = code & 3;
  Fr v = el[g];
  if (col == 1) v = fe_mul(v, k1);
  if (col == 2) v = fe_mul(v, k2);
  if (col == 3) v = fe_mul(v, k3);
  out[i] = v;
}

// One key compilation: the key under construction, its circuit and stream, and the host and
// device staging that queued copies and kernels read until the final wait. Every transform here
// runs without scratch of its own (ntt_run with nullptr), unlike the prover's.
struct KeyBuild {
  plk_key* key;
  const plk_composer* cs;
  hipStream_t s;
  std::vector<Fr> sel_host, gate_consts;
  std::vector<uint32_t> sigma_codes, wire_idx;
  DevBuf d_sigma_codes;
};

// 1. selectors padded to n (key.rs:89-119) -> idft (key.rs:121-131)
int compile_selectors(KeyBuild& kb) {
  plk_key* key = kb.key;
  const uint64_t n = key->n, m = key->m;
  kb.sel_host.assign(11 * n, fe_zero<FrCfg>());
  for (uint64_t i = 0; i < m; ++i) {
    const Gate g = gate_unpack(kb.cs, i);
    for (int q = 0; q < 11; ++q) kb.sel_host[q * n + i] = g.q[q];
  }
  TRY(key->q_coef.alloc(11 * n * sizeof(Fr)));
  PLK_HIP_TRY(hipMemcpyAsync(key->q_coef.ptr, kb.sel_host.data(), 11 * n * sizeof(Fr),
                             hipMemcpyHostToDevice, kb.s));
  Fr* qc = key->q_coef.as<Fr>();
  for (int q = 0; q < 11; ++q) TRY(ntt_run(key->dom, qc + q * n, qc + q * n, n, -1, 0, nullptr, kb.s, 1));
  return PLK_OK;
}

// 2. sigma permutations (permutation.rs:108-141) and Lagrange encodings (:143-168)
int compile_sigmas(KeyBuild& kb) {
  plk_key* key = kb.key;
  const plk_composer* cs = kb.cs;
  const uint64_t n = key->n;
  std::vector<uint32_t>& codes = kb.sigma_codes;
  codes.resize(4 * n);
  for (uint64_t i = 0; i < n; ++i)
    for (uint32_t col = 0; col < 4; ++col) codes[col * n + i] = (uint32_t)(4 * i + col);
  // each witness's wires form a cycle in insertion order: wire -> next, last -> first
  for (size_t wit = 0; wit < cs->wire_head.size(); ++wit)
    for (uint32_t cur = cs->wire_head[wit]; cur != plk_composer::kNoWire; cur = cs->wire_next[cur]) {
      const uint32_t nx = cs->wire_next[cur];
      const uint32_t nxt = nx == plk_composer::kNoWire ? cs->wire_head[wit] : nx;
      codes[(cur & 3) * n + (cur >> 2)] = nxt;
    }
  TRY(kb.d_sigma_codes.alloc(4 * n * 4));
  PLK_HIP_TRY(hipMemcpyAsync(kb.d_sigma_codes.ptr, codes.data(), 4 * n * 4, hipMemcpyHostToDevice, kb.s));
  TRY(key->sigma_lag.alloc(4 * n * sizeof(Fr)));
  hipLaunchKernelGGL(k_sigma_values, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, kb.s,
                     kb.d_sigma_codes.as<uint32_t>(), key->dom->tw_fwd.as<Fr>(), n, perm_k(1),
                     perm_k(2), perm_k(3), key->sigma_lag.as<Fr>());
  PLK_HIP_TRY(hipGetLastError());
  TRY(key->sigma_coef.alloc(4 * n * sizeof(Fr)));
  Fr* sc = key->sigma_coef.as<Fr>();
  for (int c = 0; c < 4; ++c)
    TRY(ntt_run(key->dom, key->sigma_lag.as<Fr>() + c * n, sc + c * n, n, -1, 0, nullptr, kb.s, 1));
  return PLK_OK;
}

// 3. commitments (key.rs:138-159): selectors swallow errors, sigmas propagate
int compile_commitments(KeyBuild& kb) {
  plk_key* key = kb.key;
  const uint64_t n = key->n;
  std::vector<const Fr*> ptrs;
  std::vector<size_t> lens;
  for (int q : kKeyCommSel) {
    ptrs.push_back(key->q_coef.as<Fr>() + q * n);
    lens.push_back(n);
  }
  for (int c = 0; c < 4; ++c) {
    ptrs.push_back(key->sigma_coef.as<Fr>() + c * n);
    lens.push_back(n);
  }
  int sts[15];
  const int r = key_commit(key, *key->srs->ws, ptrs, lens, key->comms, sts, kb.s);
  if (r != PLK_OK && r != PLK_E_DEGREE) return r;
  for (int i = 0; i < 11; ++i)
    if (sts[i] != PLK_OK) key->comms[i] = plk_g1{{0}, {0}, 1};  // unwrap_or_default
  for (int i = 11; i < 15; ++i)
    if (sts[i] != PLK_OK) return sts[i];
  return PLK_OK;
}

// 4. quotient-domain evaluations (key.rs:220-245 over g H_8n there; its cosets g w_8n^m H_n,
// m < qb, here, see prover.hpp) and v_h over them (key.rs:291)
int compile_quotient_tables(KeyBuild& kb) {
  plk_key* key = kb.key;
  hipStream_t s = kb.s;
  const uint64_t n = key->n;
  const int QB = key->qb;
  const uint64_t nq = (uint64_t)QB * n;
  const Fr one = fe_one<FrCfg>();
  const uint64_t rowc = n + 8;  // coset table row: the transforms read <= n + 8 inputs
  TRY(key->coset_s.alloc(QB * rowc * sizeof(Fr)));
  TRY(key->coset_w.alloc(QB * rowc * sizeof(Fr)));
  TRY(key->coset_pi.alloc(QB * rowc * sizeof(Fr)));
  TRY(key->icoset_q.alloc(QB * n * sizeof(Fr)));
  const Fr c32 = fr_u64(32);
  coset_shifts(key->dom, QB, key->s_m);
  for (int mb = 0; mb < QB; ++mb) {
    const Fr sm = key->s_m[mb];
    TRY(ntt_power_table(key->coset_s.as<Fr>() + mb * rowc, sm, one, rowc, true, s));
    TRY(ntt_power_table(key->coset_w.as<Fr>() + mb * rowc, sm, c32, rowc, true, s));
    TRY(ntt_power_table(key->coset_pi.as<Fr>() + mb * rowc, sm, fe_inv(c32), rowc, true, s));
    TRY(ntt_power_table(key->icoset_q.as<Fr>() + mb * n, fe_inv(sm), key->dom->n_inv, n, true, s));
  }
  // c_m = s_m^n = g^n w_8^m; v_h(s_m w_n^u) = c_m - 1 on the whole block
  const Fr* cm = key->c_m;
  for (int mb = 0; mb < QB; ++mb) {
    key->c_m[mb] = fe_pow_u64(key->s_m[mb], n);
    key->vh_inv[mb] = fe_inv(fe_sub(cm[mb], one));
  }
  // pk_coset_combine: the inverse of V[m][l] = c_m^l. Its column m holds the coefficients
  // of the Lagrange polynomial prod_{j != m} (x - c_j) / (c_m - c_j)
  for (int mb = 0; mb < QB; ++mb) {
    Fr others[kQBlocksMax], poly[kQBlocksMax + 1];
    Fr den = one;
    int cnt = 0;
    for (int j = 0; j < QB; ++j) {
      if (j == mb) continue;
      others[cnt++] = cm[j];
      den = fe_mul(den, fe_sub(cm[mb], cm[j]));
    }
    poly_from_roots(others, cnt, poly);
    const Fr dinv = fe_inv(den);
    for (int l = 0; l < QB; ++l) key->comb.m[l * QB + mb] = fe_to_rx_domain(fe_mul(poly[l], dinv));
  }
  // forward coset transforms of n-coefficient polys onto the QB blocks in one launch
  auto coset_fwd = [&](const Fr* in, Fr* out) {
    return coset_blocks_fwd(key->dom, in, out, n, key->coset_s.as<Fr>(), QB, nullptr, s);
  };
  TRY(key->selq.alloc(SEL_COUNTQ * nq * sizeof(Fr)));
  const bool sel_used[SEL_COUNTQ] = {true, true, true, true, true, true, true, key->has_range,
                                     key->has_logic, key->has_fixed, key->has_var};
  for (int j = 0; j < SEL_COUNTQ; ++j)  // SEL_* rows; unused widget selectors are never read
    if (sel_used[j]) TRY(coset_fwd(key->q_coef.as<Fr>() + j * n, key->selq.as<Fr>() + j * nq));
  TRY(key->sigmaq.alloc(4 * nq * sizeof(Fr)));
  for (int c = 0; c < 4; ++c)
    TRY(coset_fwd(key->sigma_coef.as<Fr>() + c * n, key->sigmaq.as<Fr>() + c * nq));
  // L1 over the quotient domain, shared by every proof: idft(e_0) = n^-1 in every coefficient
  TRY(key->l1q.alloc(nq * sizeof(Fr)));
  DevBuf tmp;
  TRY(tmp.alloc(n * sizeof(Fr)));
  TRY(pk_fill(tmp.as<Fr>(), key->dom->n_inv, n, s));
  TRY(coset_fwd(tmp.as<Fr>(), key->l1q.as<Fr>()));
  PLK_HIP_TRY(stream_wait(s));
  return PLK_OK;
}

// 4b. the closed-form top of t (prover.hpp): the key's share of quotient_top's inputs, and
// w^i / w^-i of the public-input rows (PI's top coefficients; proof_at_z's winv)
int compile_top_inputs(KeyBuild& kb) {
  plk_key* key = kb.key;
  const uint64_t n = key->n, m = key->m;
  if (key->qb == kQBlocksTop) {
    // coefficients n-7 .. n-1 of the 11 selectors and the 4 sigmas
    std::vector<Fr> top(15 * kTop);
    PLK_HIP_TRY(hipMemcpy2DAsync(top.data(), kTop * sizeof(Fr), key->q_coef.as<Fr>() + (n - kTop),
                                 n * sizeof(Fr), kTop * sizeof(Fr), 11, hipMemcpyDeviceToHost, kb.s));
    PLK_HIP_TRY(hipMemcpy2DAsync(top.data() + 11 * kTop, kTop * sizeof(Fr),
                                 key->sigma_coef.as<Fr>() + (n - kTop), n * sizeof(Fr),
                                 kTop * sizeof(Fr), 4, hipMemcpyDeviceToHost, kb.s));
    PLK_HIP_TRY(stream_wait(kb.s));
    for (int j = 0; j < SEL_COUNTQ; ++j)
      for (int i = 0; i < kTop; ++i) key->top_in.sel[j][i] = top[j * kTop + i];
    for (int c = 0; c < 4; ++c)
      for (int i = 0; i < kTop; ++i) key->top_in.sigma[c][i] = top[(11 + c) * kTop + i];
    for (int i = 0; i < kTop; ++i) key->top_in.l1[i] = key->dom->n_inv;  // idft(e_0)
    poly_from_roots(key->c_m, key->qb, key->top_p);  // P(Y) = prod_{m<4} (Y - c_m)
  }
  for (uint64_t i = 0; i < m; ++i)
    if (kb.cs->gates[i].code & kPiBit) {
      key->pi_w.push_back(fe_pow_u64(key->dom->omega, i));
      key->pi_winv.push_back(fe_pow_u64(key->dom->omega_inv, i));
    }
  return PLK_OK;
}

// 5. wire indices for the per-proof gather (prover.rs:114-119)
int compile_wire_index(KeyBuild& kb) {
  plk_key* key = kb.key;
  const plk_composer* cs = kb.cs;
  const uint64_t n = key->n;
  kb.wire_idx.assign(4 * n, 0);
  for (uint64_t i = 0; i < key->m; ++i)
    for (int c = 0; c < 4; ++c) {
      kb.wire_idx[c * n + i] = cs->gates[i].w[c];
      key->max_wire = std::max(key->max_wire, cs->gates[i].w[c]);
    }
  key->struct_hash = cs->struct_hash;
  TRY(key->wire_idx.alloc(4 * n * 4));
  PLK_HIP_TRY(hipMemcpyAsync(key->wire_idx.ptr, kb.wire_idx.data(), 4 * n * 4, hipMemcpyHostToDevice,
                             kb.s));
  return PLK_OK;
}

// 6. the gate table of plk_prover_diagnose: the compact records and pooled constants as the
// composer holds them, a public-input slot carrying the gate's ordinal (prover.hpp)
int compile_gate_table(KeyBuild& kb) {
  plk_key* key = kb.key;
  const plk_composer* cs = kb.cs;
  const uint64_t m = key->m;
  std::vector<Fr>& consts = kb.gate_consts;
  consts = cs->consts;
  uint32_t ordinal = 0;
  for (uint64_t i = 0; i < m; ++i) {
    const GateRec& g = cs->gates[i];
    if (!(g.code & kPiBit)) continue;
    uint32_t e = g.ext;
    for (int q = 0; q < 11; ++q) e += sel_code(g.code, q) == kSelPooled;
    consts[e] = fe_zero<FrCfg>();
    consts[e].v[0] = ordinal++;
  }
  TRY(key->gate_recs.alloc(std::max<size_t>(m, 1) * sizeof(GateRec)));
  TRY(key->gate_consts.alloc(std::max<size_t>(consts.size(), 1) * sizeof(Fr)));
  PLK_HIP_TRY(hipMemcpyAsync(key->gate_recs.ptr, cs->gates.data(), m * sizeof(GateRec),
                             hipMemcpyHostToDevice, kb.s));
  if (!consts.empty())
    PLK_HIP_TRY(hipMemcpyAsync(key->gate_consts.ptr, consts.data(), consts.size() * sizeof(Fr),
                               hipMemcpyHostToDevice, kb.s));
  return PLK_OK;
}

// PLK_LAGRANGE_COMMIT=0: keys compiled while it is set carry no Lagrange-basis SRS, and round 1
// commits their wires from the coefficients (the A/B switch). Read at key compile, never per
// proof.
bool lagrange_commit_enabled() {
  const char* e = getenv("PLK_LAGRANGE_COMMIT");
  return !(e && e[0] == '0' && e[1] == 0);
}

}  // namespace
}  // namespace plk

using namespace plk;

extern "C" {

int plk_key_compile(plk_srs* srs, const plk_composer* cs, const char* label, plk_key** out) {
  PLK_API_BEGIN
    if (!srs || !cs || !out) return PLK_E_ARG;
    *out = nullptr;
    plk_ctx* ctx = srs->ctx;
    DeviceGuard guard(ctx->device);
    std::unique_ptr<plk_key> key(new plk_key());
    key->ctx = ctx;
    key->srs = srs;
    key->label = label ? label : "plonk";
    const uint64_t m = cs->gates.size();
    const uint32_t k = log2_ceil(m);
    const uint64_t n = 1ull << k;
    key->m = m;
    key->n = n;
    key->k = k;
    // keypair.trim(additional_n) with additional_n = next_pow2(m + 6) (key.rs:81-82); the
    // trimmed SRS keeps PlonkParams' slack of 8 points
    key->n_trim = (1ull << log2_ceil(m + 6)) + 8;
    if (k + 1 > 27) return PLK_E_ARG;
    for (uint64_t i = 0; i < m; ++i) {
      const Gate g = gate_unpack(cs, i);
      if (!fe_is_zero(g.q[SEL_QRANGE])) key->has_range = true;
      if (!fe_is_zero(g.q[SEL_QLOGIC])) key->has_logic = true;
      if (!fe_is_zero(g.q[SEL_QFIXED])) key->has_fixed = true;
      if (!fe_is_zero(g.q[SEL_QVAR])) key->has_var = true;
    }
    TRY(plk_domain_get(ctx, k, &key->dom));
    // the Lagrange-basis SRS (round 1's wire commits): needs [tau^n .. tau^(n+2)] for the blinders
    if (lagrange_commit_enabled() && srs->n >= n + 3) TRY(srs_lagrange_build(srs, key->dom, false, &key->lag));
    key->qb = q_blocks(n);
    // the steps queue on the context's stream in this order; the staging they read lives in kb
    // until the last wait
    KeyBuild kb{key.get(), cs, ctx->stream};
    TRY(compile_selectors(kb));
    TRY(compile_sigmas(kb));
    TRY(compile_commitments(kb));
    TRY(compile_quotient_tables(kb));
    TRY(compile_top_inputs(kb));
    TRY(compile_wire_index(kb));
    TRY(compile_gate_table(kb));
    PLK_HIP_TRY(stream_wait(kb.s));
    *out = key.release();
    return PLK_OK;
  PLK_API_END
}

int plk_key_destroy(plk_key* key) {
  if (!key) return PLK_E_ARG;
  DeviceGuard g(key->ctx->device);
  (void)stream_wait(key->ctx->stream);
  delete key;
  return PLK_OK;
}

int plk_key_info(const plk_key* key, uint64_t* n, uint64_t* m, plk_g1* commitments) {
  if (!key) return PLK_E_ARG;
  if (n) *n = key->n;
  if (m) *m = key->m;
  if (commitments) std::memcpy(commitments, key->comms, sizeof key->comms);
  return PLK_OK;
}

}  // extern "C"

plk_key::~plk_key() { delete lag; }
