// circuit_check.hip — which gates a witness fails (include/plk.h, "circuit check"): k_gate_check
// evaluates every gate identity of circuit_check.hpp, one gate per lane, on the composer's
// compact gate records, and reduces the verdict on the device; plk_composer_check uploads a
// composer and runs it (or, without a context, the same function in a host loop);
// plk_prover_diagnose / plk_key_diagnose run it on the witness a prover already holds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "circuit_check.hpp"
#include "internal.hpp"
#include "prover.hpp"

namespace plk {

constexpr uint32_t kCheckBlock = 256, kCheckWaves = kCheckBlock / 64;

struct GateCheckArgs {
  const GateRec* gates;
  const Fr* consts;
  const Fr* witness;
  const Fr* pi_vals;  // null: a composer's table (gate_check_at)
  uint64_t m;
  // The sweep (list null, count = m): lane t checks gate t, mask[t] is its mask, and the counters
  // take the failing gates. The listing (after a failing sweep): lane t checks gate list[t],
  // t < count, and stores mask[t] and residual[t]; no counters.
  const uint32_t* list;
  uint64_t count;
  uint32_t* mask;
  Fr* residual;
  CheckCounters* counters;
};

__global__ void __launch_bounds__(kCheckBlock) k_gate_check(GateCheckArgs A) {
  const uint64_t t = (uint64_t)blockIdx.x * kCheckBlock + threadIdx.x;
  uint32_t mask = 0;
  if (t < A.count) {
    const uint64_t i = A.list ? A.list[t] : t;
    const GateVerdict v = gate_check_at(A.gates, A.consts, A.witness, A.pi_vals, A.m, i);
    mask = v.mask;
    A.mask[t] = mask;
    if (A.residual) {
      uint4* o = reinterpret_cast<uint4*>(&A.residual[t]);
      o[0] = make_uint4(v.residual.v[0], v.residual.v[1], v.residual.v[2], v.residual.v[3]);
      o[1] = make_uint4(v.residual.v[4], v.residual.v[5], v.residual.v[6], v.residual.v[7]);
    }
  }
  if (!A.counters) return;  // uniform over the launch
  // per wave: the failing gates, the five class counts and the smallest failing lane; per block:
  // their sums, then one atomic per counter that has something to add
  __shared__ uint32_t cnt[kCheckWaves][6];
  __shared__ uint32_t first[kCheckWaves];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long fail = __ballot(mask != 0);
  unsigned long long cls[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) cls[k] = __ballot((mask & kClassMask[k]) != 0);
  if (lane == 0) {
    cnt[wave][0] = (uint32_t)__popcll(fail);
#pragma unroll
    for (int k = 0; k < 5; ++k) cnt[wave][1 + k] = (uint32_t)__popcll(cls[k]);
    first[wave] = fail ? wave * 64 + (uint32_t)__ffsll((long long)fail) - 1 : 0xffffffffu;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < kCheckWaves; ++w) sum += cnt[w][threadIdx.x];
    unsigned long long* dst = threadIdx.x == 0 ? &A.counters->failing
                                               : &A.counters->by_class[threadIdx.x - 1];
    if (sum) atomicAdd(dst, (unsigned long long)sum);
  } else if (threadIdx.x == 6) {
    uint32_t lo = 0xffffffffu;
#pragma unroll
    for (uint32_t w = 0; w < kCheckWaves; ++w) lo = min(lo, first[w]);
    if (lo != 0xffffffffu)
      atomicMax(&A.counters->first_inv, ~((unsigned long long)blockIdx.x * kCheckBlock + lo));
  }
}

struct CheckWs {
  DevBuf mask, counters, list, list_mask, list_res;
  PinnedBuf pin_counters;
  // plk_composer_check's upload: witness | gate records | pooled constants, staged through pin_up
  DevBuf up;
  PinnedBuf pin_up;
  TimingEvents<2> ev;
};
void check_ws_delete(CheckWs* w) { delete w; }

namespace {

void summary_add(plk_check_summary& s, uint32_t mask) {
  if (!mask) return;
  ++s.failing;
  for (int k = 0; k < 5; ++k) s.by_class[k] += (mask & kClassMask[k]) != 0;
}

}  // namespace

int check_run(CheckWs*& ws, plk_ctx* ctx, hipStream_t s, const GateRec* d_gates, const Fr* d_consts,
              const Fr* d_witness, const Fr* d_pi_vals, uint64_t m, plk_check_summary* summary,
              plk_gate_failure* failures, size_t cap, size_t* count) {
  if (!ws) ws = new CheckWs();
  CheckWs& w = *ws;
  TRY(w.ev.create());
  TRY(w.mask.alloc(std::max<uint64_t>(m, 1) * sizeof(uint32_t)));
  TRY(w.counters.alloc(sizeof(CheckCounters)));
  TRY(w.pin_counters.alloc(sizeof(CheckCounters)));
  GateCheckArgs A{};
  A.gates = d_gates;
  A.consts = d_consts;
  A.witness = d_witness;
  A.pi_vals = d_pi_vals;
  A.m = m;
  A.count = m;
  A.mask = w.mask.as<uint32_t>();
  A.counters = w.counters.as<CheckCounters>();
  PLK_HIP_TRY(hipMemsetAsync(w.counters.ptr, 0, sizeof(CheckCounters), s));
  PLK_HIP_TRY(hipEventRecord(w.ev.e[0], s));
  if (m) hipLaunchKernelGGL(k_gate_check, dim3(cdiv(m, kCheckBlock)), dim3(kCheckBlock), 0, s, A);
  PLK_HIP_TRY(hipEventRecord(w.ev.e[1], s));
  PLK_HIP_TRY(hipGetLastError());
  PLK_HIP_TRY(hipMemcpyAsync(w.pin_counters.ptr, w.counters.ptr, sizeof(CheckCounters),
                             hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  (void)hipEventElapsedTime(&ctx->check_ms, w.ev.e[0], w.ev.e[1]);
  const CheckCounters c = *w.pin_counters.as<CheckCounters>();
  std::memset(summary, 0, sizeof *summary);
  summary->gates = m;
  summary->failing = c.failing;
  for (int k = 0; k < 5; ++k) summary->by_class[k] = c.by_class[k];
  const size_t want = failures ? (size_t)std::min<uint64_t>(cap, c.failing) : 0;
  if (count) *count = want;
  if (!want) return PLK_OK;
  // the first `want` failing gates: the masks from the smallest failing gate on, a stretch at
  // a time, until they are found
  std::vector<uint32_t> list, masks, buf;
  const uint64_t stretch = 1u << 20;
  for (uint64_t lo = ~c.first_inv; lo < m && list.size() < want; lo += stretch) {
    const uint64_t len = std::min(stretch, m - lo);
    buf.resize(len);
    PLK_HIP_TRY(hipMemcpyAsync(buf.data(), w.mask.as<uint32_t>() + lo, len * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, s));
    PLK_HIP_TRY(stream_wait(s));
    for (uint64_t j = 0; j < len && list.size() < want; ++j)
      if (buf[j]) {
        list.push_back((uint32_t)(lo + j));
        masks.push_back(buf[j]);
      }
  }
  if (list.size() != want) return PLK_E_DEVICE;  // the counters and the masks disagree
  // their residuals: the same kernel over the listed gates
  TRY(w.list.alloc(want * sizeof(uint32_t)));
  TRY(w.list_mask.alloc(want * sizeof(uint32_t)));
  TRY(w.list_res.alloc(want * sizeof(Fr)));
  PLK_HIP_TRY(hipMemcpyAsync(w.list.ptr, list.data(), want * sizeof(uint32_t),
                             hipMemcpyHostToDevice, s));
  A.list = w.list.as<uint32_t>();
  A.count = want;
  A.mask = w.list_mask.as<uint32_t>();
  A.residual = w.list_res.as<Fr>();
  A.counters = nullptr;
  hipLaunchKernelGGL(k_gate_check, dim3(cdiv(want, kCheckBlock)), dim3(kCheckBlock), 0, s, A);
  PLK_HIP_TRY(hipGetLastError());
  std::vector<Fr> res(want);
  PLK_HIP_TRY(hipMemcpyAsync(res.data(), w.list_res.ptr, want * sizeof(Fr), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  for (size_t j = 0; j < want; ++j) {
    failures[j].gate = list[j];
    failures[j].mask = masks[j];
    failures[j]._pad = 0;
    failures[j].residual = fr_to_abi(res[j]);
  }
  return PLK_OK;
}

}  // namespace plk

using namespace plk;

extern "C" {

int plk_composer_check(plk_ctx* ctx, const plk_composer* cs, plk_check_summary* summary,
                       plk_gate_failure* failures, size_t cap, size_t* count) {
  PLK_API_BEGIN
    if (!cs || !summary) return PLK_E_ARG;
    const uint64_t m = cs->gates.size();
    if (!ctx) {  // the host mirror: the kernel's per-gate function in a loop
      std::memset(summary, 0, sizeof *summary);
      summary->gates = m;
      size_t listed = 0;
      for (uint64_t i = 0; i < m; ++i) {
        const GateVerdict v = gate_check_at(cs->gates.data(), cs->consts.data(), cs->witness.data(),
                                            nullptr, m, i);
        if (!v.mask) continue;
        summary_add(*summary, v.mask);
        if (failures && listed < cap) {
          plk_gate_failure& f = failures[listed++];
          f.gate = i;
          f.mask = v.mask;
          f._pad = 0;
          f.residual = fr_to_abi(v.residual);
        }
      }
      if (count) *count = listed;
      return PLK_OK;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);  // one check at a time on the context's buffers
    DeviceGuard guard(ctx->device);
    hipStream_t s = ctx->stream;
    if (!ctx->check_ws) ctx->check_ws = new CheckWs();
    CheckWs& w = *ctx->check_ws;
    // witness | gate records | pooled constants through pinned staging, in chunks: the CPU copy
    // of chunk i + 1 overlaps the DMA of chunk i
    const void* src[3] = {cs->witness.data(), cs->gates.data(), cs->consts.data()};
    const size_t len[3] = {cs->witness.size() * sizeof(Fr), cs->gates.size() * sizeof(GateRec),
                           cs->consts.size() * sizeof(Fr)};
    size_t off[3], total = 0;
    for (int k = 0; k < 3; ++k) {
      off[k] = total;
      total += (len[k] + 31) & ~(size_t)31;
    }
    TRY(w.up.alloc(std::max<size_t>(total, 32)));
    TRY(w.pin_up.alloc(std::max<size_t>(total, 32)));
    const size_t chunk = 8u << 20;
    for (int k = 0; k < 3; ++k)
      for (size_t o = 0; o < len[k]; o += chunk) {
        const size_t n = std::min(chunk, len[k] - o);
        std::memcpy(w.pin_up.as<char>() + off[k] + o, static_cast<const char*>(src[k]) + o, n);
        PLK_HIP_TRY(hipMemcpyAsync(w.up.as<char>() + off[k] + o, w.pin_up.as<char>() + off[k] + o, n,
                                   hipMemcpyHostToDevice, s));
      }
    const char* d = w.up.as<char>();
    return check_run(ctx->check_ws, ctx, s, reinterpret_cast<const GateRec*>(d + off[1]),
                     reinterpret_cast<const Fr*>(d + off[2]), reinterpret_cast<const Fr*>(d + off[0]),
                     nullptr, m, summary, failures, cap, count);
  PLK_API_END
}

int plk_prover_diagnose(plk_prover* P, plk_check_summary* summary, plk_gate_failure* failures,
                        size_t cap, size_t* count) {
  PLK_API_BEGIN
    if (!P || !summary || !P->have_witness) return PLK_E_ARG;
    plk_key* key = P->key;
    DeviceGuard guard(key->ctx->device);
    hipStream_t s = P->stream;
    // this proof's public inputs, by their ordinal (the key's table names the ordinal)
    TRY(P->pi_vals.alloc(std::max<size_t>(P->last_pi.size(), 1) * sizeof(Fr)));
    if (!P->last_pi.empty())
      PLK_HIP_TRY(hipMemcpyAsync(P->pi_vals.ptr, P->last_pi.data(), P->last_pi.size() * sizeof(Fr),
                                 hipMemcpyHostToDevice, s));
    return check_run(P->check_ws, key->ctx, s, key->gate_recs.as<GateRec>(),
                     key->gate_consts.as<Fr>(), P->witness.as<Fr>(), P->pi_vals.as<Fr>(), key->m,
                     summary, failures, cap, count);
  PLK_API_END
}

int plk_key_diagnose(plk_key* key, plk_check_summary* summary, plk_gate_failure* failures,
                     size_t cap, size_t* count) {
  PLK_API_BEGIN
    if (!key || !summary) return PLK_E_ARG;
    std::lock_guard<std::mutex> lk(key->def_mu);
    if (!key->def_prover) return PLK_E_ARG;  // plk_prove has not run: no witness
    return plk_prover_diagnose(key->def_prover.get(), summary, failures, cap, count);
  PLK_API_END
}

int plk_check_last_ms(plk_ctx* ctx, float* kernel_ms) {
  if (!ctx || !kernel_ms) return PLK_E_ARG;
  *kernel_ms = ctx->check_ms;
  return PLK_OK;
}

}  // extern "C"
