// ingest.hip — the ingest stage in front of the batch verifier (include/plk.h "Compact proofs
// and the ingest stage"): compact proof bytes in, decoded proofs and one status per proof out.
//
//  - The compact format: 11 commitments as zkcrypto's 48-byte compressed G1 (exactly what
//    Transcript::g1_compress writes), then 16 scalars as 32 canonical little-endian bytes.
//    ASSUMED, parity unpinned: the element crates are not vendored.
//  - k_g1_decompress, one point per lane: parse, range-check x, y = (x^3 + 4)^((p+1)/4)
//    (p = 3 mod 4), verify y^2 = x^3 + 4, pick the root by the sort bit.
//  - k_g1_subgroup, one point per lane: P in G1  <=>  (beta x, y) == -[x0^2] P with
//    x0 = 0xd201000000010000 (Scott, eprint 2021/1130 section 6; zkcrypto's is_torsion_free).
//  - k_fr_decode, one scalar per lane: range check and Montgomery form.
//
// The math (ingest_math.hpp, shared with srs_io.hip) and the conversions at the boundary (abi.hpp:
// item loads, limbs, the byte serializer) are PLK_HD code on the packed field of ff.hpp / g1.hpp,
// so the host decode
// (plk_proof_decode_compact, the single-proof path) and the kernels run the same functions; the
// tests hold both against a pure-Python reference. The packed form, not the redundant-limb one
// (ffr.hpp): both kernels are one long dependent chain of products per lane with canonical
// comparisons in between (y^2 == x^3 + 4, the group law's P == Q tests on adversarial low-order
// inputs), which the packed field's always-canonical values give for free, and g1.hpp's group
// law handles doubling and the identity explicitly.
//
// The square root's exponent is fixed: a sliding window of 3 bits over it with the odd powers
// x, x^3, x^5, x^7 held in registers (48 VGPRs) costs 379 squarings and about 100 products. The
// exponent's bits are wave-uniform, so the window logic is scalar control flow and the table is
// selected with compile-time indices: no stack array, no LDS, no scratch.
#include <cstring>
#include <new>
#include <vector>

#include "ingest_math.hpp"
#include "internal.hpp"

using namespace plk;

namespace plk {
namespace {

constexpr size_t kG1Bytes = 48, kFrBytes = 32, kComms = 11, kEvals = 16, kFields = kComms + kEvals;
static_assert(PLK_PROOF_COMPACT_BYTES == kComms * kG1Bytes + kEvals * kFrBytes, "layout");
static_assert(sizeof(plk_proof) == kComms * sizeof(plk_g1) + kEvals * sizeof(plk_fr), "no padding");
static_assert(sizeof(plk_g1) == 104 && sizeof(plk_fr) == 32, "ABI");

// ---- kernels --------------------------------------------------------------------------
// Items are addressed in groups so that the same kernels serve a flat array of points (per = 1)
// and the fields of an array of proofs (per = 11 points / 16 scalars per proof): item t is field
// t % per of group t / per, its input at in + group * in_stride + field * item bytes, its output
// at out + group * out_stride + field * item size, its status at status + group * st_stride +
// field. All strides in bytes.
struct Layout {
  uint32_t per;
  uint64_t in_stride, out_stride, st_stride;
};

constexpr int kBlock = 64;  // one wave: a small batch still spreads over the CUs

__global__ void __launch_bounds__(kBlock) k_g1_decompress(const uint8_t* __restrict__ in, uint64_t n, Layout L,
                                                          uint8_t* __restrict__ out,
                                                          uint8_t* __restrict__ status) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const uint64_t g = t / L.per, f = t % L.per;
  uint32_t w[12];
  ld_words(in + g * L.in_stride + f * kG1Bytes, w);  // 16-B aligned
  Fp x, y;
  bool inf;
  const uint8_t st = g1_decompress_words(w, x, y, inf);  // x = y = 0 unless finite and accepted
  plk_g1* dst = reinterpret_cast<plk_g1*>(out + g * L.out_stride + f * sizeof(plk_g1));
  fe_to_abi(x, dst->x);
  fe_to_abi(y, dst->y);
  dst->infinity = inf ? 1 : 0;
  status[g * L.st_stride + f] = st;
}

// points in ABI form (canonical, on the curve) with status 0: a non-member gets
// PLK_INGEST_SUBGROUP; identities and items with a status stay as they are
__global__ void __launch_bounds__(kBlock) k_g1_subgroup(const uint8_t* __restrict__ pts, uint64_t n, Layout L,
                                                        uint8_t* __restrict__ status) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const uint64_t g = t / L.per, f = t % L.per;
  uint8_t* st = status + g * L.st_stride + f;
  const plk_g1* src = reinterpret_cast<const plk_g1*>(pts + g * L.out_stride + f * sizeof(plk_g1));
  if (*st != PLK_INGEST_OK || src->infinity != 0) return;
  const G1Abi p = g1_load<false>(src);
  if (!g1_in_subgroup(p.x, p.y)) *st = PLK_INGEST_SUBGROUP;
}

// ABI points from the caller: status 0xff for a point g1_load<true> refuses
// (plk_g1_subgroup_check_batch refuses the call), else 0
constexpr uint8_t kBadPoint = 0xff;
__global__ void __launch_bounds__(kBlock) k_g1_validate(const plk_g1* __restrict__ pts, uint64_t n,
                                                        uint8_t* __restrict__ status) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  status[t] = g1_load<true>(pts + t).ok ? PLK_INGEST_OK : kBadPoint;
}

__global__ void __launch_bounds__(kBlock) k_fr_decode(const uint8_t* __restrict__ in, uint64_t n, Layout L,
                                                      uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const uint64_t g = t / L.per, f = t % L.per;
  uint32_t w[8];
  ld_words(in + g * L.in_stride + f * kFrBytes, w);  // 16-B aligned
  Fr s;
  const uint8_t st = fr_decode_words(w, s);
  fe_to_abi(s, reinterpret_cast<uint64_t*>(out + g * L.out_stride + f * sizeof(plk_fr)));
  status[g * L.st_stride + f] = st;
}

// ---- host codec -----------------------------------------------------------------------
// field order of proof.rs:39-66 / plk_proof: the 11 commitments, then the 16 evaluations
const plk_g1* comm(const plk_proof* p, size_t i) { return &p->a_comm + i; }
plk_g1* comm(plk_proof* p, size_t i) { return &p->a_comm + i; }
const plk_fr* eval(const plk_proof* p, size_t i) { return &p->a_eval + i; }
plk_fr* eval(plk_proof* p, size_t i) { return &p->a_eval + i; }

// the 48 bytes Transcript::g1_compress writes, for a point with canonical limbs (the curve
// equation is not asked for: an encoder, not a validator)
bool g1_compress_host(const plk_g1& p, uint8_t* out) {
  const G1Abi a = g1_load<false>(&p);
  if (p.infinity > 1 || (!a.inf && !(fe_canonical(a.x) && fe_canonical(a.y)))) return false;
  g1_compress_bytes(a.x, a.y, a.inf, out);
  return true;
}

// one compressed point on the host: the kernels' math. Returns a PLK_INGEST_* code.
uint8_t g1_decompress_host(const uint8_t* in, int check_subgroup, plk_g1* out) {
  uint32_t w[12];
  words_of_bytes(in, w);
  Fp x, y;
  bool inf;
  uint8_t st = g1_decompress_words(w, x, y, inf);
  if (st == PLK_INGEST_OK && !inf && check_subgroup && !g1_in_subgroup(x, y)) st = PLK_INGEST_SUBGROUP;
  std::memset(out, 0, sizeof *out);
  if (st == PLK_INGEST_OK) g1_store(x, y, !inf, out);
  return st;
}

}  // namespace

struct IngestWs {
  DevBuf d_in, d_out, d_status;
  TimingEvents<4> ev;
  float decompress_ms = 0.f, subgroup_ms = 0.f;
};
void ingest_ws_delete(IngestWs* w) { delete w; }

namespace {

int ingest_ws(plk_ctx* ctx, IngestWs** out) {
  if (!ctx->ingest_ws) ctx->ingest_ws = new IngestWs();
  IngestWs& w = *ctx->ingest_ws;
  *out = &w;
  return w.ev.create();
}

// the timed kernels of one batched call on the context's stream: decompression of n_pts points
// (skipped when `decompress` is false: the points are already in d_out) and the subgroup test
int run_point_kernels(plk_ctx* ctx, IngestWs& w, uint64_t n_pts, const Layout& L, bool decompress,
                      bool subgroup) {
  hipStream_t s = ctx->stream;
  if (decompress) {
    PLK_HIP_TRY(hipEventRecord(w.ev.e[0], s));
    hipLaunchKernelGGL(k_g1_decompress, dim3(cdiv(n_pts, kBlock)), dim3(kBlock), 0, s,
                       (const uint8_t*)w.d_in.as<uint8_t>(), n_pts, L, w.d_out.as<uint8_t>(),
                       w.d_status.as<uint8_t>());
    PLK_HIP_TRY(hipEventRecord(w.ev.e[1], s));
  }
  if (subgroup) {
    PLK_HIP_TRY(hipEventRecord(w.ev.e[2], s));
    hipLaunchKernelGGL(k_g1_subgroup, dim3(cdiv(n_pts, kBlock)), dim3(kBlock), 0, s,
                       (const uint8_t*)w.d_out.as<uint8_t>(), n_pts, L, w.d_status.as<uint8_t>());
    PLK_HIP_TRY(hipEventRecord(w.ev.e[3], s));
  }
  PLK_HIP_TRY(hipGetLastError());
  return PLK_OK;
}

void read_timings(IngestWs& w, bool decompress, bool subgroup) {
  w.decompress_ms = w.subgroup_ms = 0.f;
  if (decompress) (void)hipEventElapsedTime(&w.decompress_ms, w.ev.e[0], w.ev.e[1]);
  if (subgroup) (void)hipEventElapsedTime(&w.subgroup_ms, w.ev.e[2], w.ev.e[3]);
}

}  // namespace
}  // namespace plk

extern "C" {

int plk_proof_encode_compact(const plk_proof* proof, uint8_t* out, size_t cap, size_t* len) {
  if (!proof) return PLK_E_ARG;
  if (len) *len = PLK_PROOF_COMPACT_BYTES;
  if (!out) return PLK_OK;  // size query
  if (cap < PLK_PROOF_COMPACT_BYTES) return PLK_E_ARG;
  uint8_t buf[PLK_PROOF_COMPACT_BYTES];
  uint8_t* o = buf;
  for (size_t i = 0; i < kComms; ++i, o += kG1Bytes)
    if (!g1_compress_host(*comm(proof, i), o)) return PLK_E_ARG;
  for (size_t i = 0; i < kEvals; ++i, o += kFrBytes) {
    if (!abi_canonical<FrCfg>(eval(proof, i)->l)) return PLK_E_ARG;
    bytes_of_words(fe_from_mont(fr_from_abi(*eval(proof, i))).v, o);
  }
  std::memcpy(out, buf, sizeof buf);
  return PLK_OK;
}

int plk_proof_decode_compact(const uint8_t* in, size_t len, plk_proof* out, int check_subgroup) {
  if (!in || !out || len != PLK_PROOF_COMPACT_BYTES) return PLK_E_ARG;
  plk_proof p;
  std::memset(&p, 0, sizeof p);
  const uint8_t* q = in;
  for (size_t i = 0; i < kComms; ++i, q += kG1Bytes)
    if (g1_decompress_host(q, check_subgroup, comm(&p, i)) != PLK_INGEST_OK) return PLK_E_ARG;
  for (size_t i = 0; i < kEvals; ++i, q += kFrBytes) {
    uint32_t w[8];
    words_of_bytes(q, w);
    Fr s;
    if (fr_decode_words(w, s) != PLK_INGEST_OK) return PLK_E_ARG;
    *eval(&p, i) = fr_to_abi(s);
  }
  *out = p;
  return PLK_OK;
}

int plk_g1_decompress_batch(plk_ctx* ctx, const uint8_t* in48, size_t n, int check_subgroup, plk_g1* out,
                            uint8_t* status) {
  PLK_API_BEGIN
  if (!ctx || !in48 || !out || !status || n == 0 || n > (1u << 28)) return PLK_E_ARG;
  DeviceGuard g(ctx->device);
  IngestWs* w;
  int st;
  if ((st = ingest_ws(ctx, &w))) return st;
  if ((st = w->d_in.alloc(n * kG1Bytes))) return st;
  if ((st = w->d_out.alloc(n * sizeof(plk_g1)))) return st;
  if ((st = w->d_status.alloc(n))) return st;
  hipStream_t s = ctx->stream;
  PLK_HIP_TRY(hipMemcpyAsync(w->d_in.ptr, in48, n * kG1Bytes, hipMemcpyHostToDevice, s));
  const Layout L = {1, kG1Bytes, sizeof(plk_g1), 1};
  if ((st = run_point_kernels(ctx, *w, n, L, true, check_subgroup != 0))) return st;
  std::vector<plk_g1> pts(n);
  std::vector<uint8_t> sts(n);
  PLK_HIP_TRY(hipMemcpyAsync(pts.data(), w->d_out.ptr, n * sizeof(plk_g1), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(hipMemcpyAsync(sts.data(), w->d_status.ptr, n, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  read_timings(*w, true, check_subgroup != 0);
  for (size_t i = 0; i < n; ++i)
    if (sts[i] != PLK_INGEST_OK) std::memset(&pts[i], 0, sizeof(plk_g1));
  std::memcpy(out, pts.data(), n * sizeof(plk_g1));
  std::memcpy(status, sts.data(), n);
  return PLK_OK;
  PLK_API_END
}

int plk_g1_subgroup_check_batch(plk_ctx* ctx, const plk_g1* points, size_t n, uint8_t* ok) {
  PLK_API_BEGIN
  if (!ctx || !points || !ok || n == 0 || n > (1u << 28)) return PLK_E_ARG;
  DeviceGuard g(ctx->device);
  IngestWs* w;
  int st;
  if ((st = ingest_ws(ctx, &w))) return st;
  if ((st = w->d_out.alloc(n * sizeof(plk_g1)))) return st;
  if ((st = w->d_status.alloc(n))) return st;
  hipStream_t s = ctx->stream;
  PLK_HIP_TRY(hipMemcpyAsync(w->d_out.ptr, points, n * sizeof(plk_g1), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_g1_validate, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s,
                     (const plk_g1*)w->d_out.as<plk_g1>(), (uint64_t)n, w->d_status.as<uint8_t>());
  const Layout L = {1, kG1Bytes, sizeof(plk_g1), 1};
  if ((st = run_point_kernels(ctx, *w, n, L, false, true))) return st;
  std::vector<uint8_t> sts(n);
  PLK_HIP_TRY(hipMemcpyAsync(sts.data(), w->d_status.ptr, n, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  read_timings(*w, false, true);
  for (size_t i = 0; i < n; ++i)
    if (sts[i] == kBadPoint) return PLK_E_ARG;
  for (size_t i = 0; i < n; ++i) ok[i] = sts[i] == PLK_INGEST_OK ? 1 : 0;
  return PLK_OK;
  PLK_API_END
}

int plk_proofs_ingest(plk_ctx* ctx, const uint8_t* in, size_t count, int check_subgroup, plk_proof* out,
                      uint8_t* status) {
  PLK_API_BEGIN
  if (!ctx || !in || !out || !status || count == 0 || count > (1u << 24)) return PLK_E_ARG;
  DeviceGuard g(ctx->device);
  IngestWs* w;
  int st;
  if ((st = ingest_ws(ctx, &w))) return st;
  if ((st = w->d_in.alloc(count * PLK_PROOF_COMPACT_BYTES))) return st;
  if ((st = w->d_out.alloc(count * sizeof(plk_proof)))) return st;
  if ((st = w->d_status.alloc(count * kFields))) return st;
  hipStream_t s = ctx->stream;
  PLK_HIP_TRY(hipMemcpyAsync(w->d_in.ptr, in, count * PLK_PROOF_COMPACT_BYTES, hipMemcpyHostToDevice, s));
  // the points of proof j: fields 0..10 of group j; its scalars: the 16 fields after them
  const Layout LP = {(uint32_t)kComms, PLK_PROOF_COMPACT_BYTES, sizeof(plk_proof), kFields};
  if ((st = run_point_kernels(ctx, *w, count * kComms, LP, true, check_subgroup != 0))) return st;
  const Layout LS = {(uint32_t)kEvals, PLK_PROOF_COMPACT_BYTES, sizeof(plk_proof), kFields};
  hipLaunchKernelGGL(k_fr_decode, dim3(cdiv(count * kEvals, kBlock)), dim3(kBlock), 0, s,
                     (const uint8_t*)w->d_in.as<uint8_t>() + kComms * kG1Bytes, (uint64_t)(count * kEvals), LS,
                     w->d_out.as<uint8_t>() + kComms * sizeof(plk_g1), w->d_status.as<uint8_t>() + kComms);
  PLK_HIP_TRY(hipGetLastError());
  std::vector<plk_proof> res(count);
  std::vector<uint8_t> sts(count * kFields);
  PLK_HIP_TRY(hipMemcpyAsync(res.data(), w->d_out.ptr, count * sizeof(plk_proof), hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(hipMemcpyAsync(sts.data(), w->d_status.ptr, count * kFields, hipMemcpyDeviceToHost, s));
  PLK_HIP_TRY(stream_wait(s));
  read_timings(*w, true, check_subgroup != 0);
  for (size_t j = 0; j < count; ++j) {
    uint8_t code = PLK_INGEST_OK;  // the first failing field's code
    for (size_t f = 0; f < kFields && code == PLK_INGEST_OK; ++f) code = sts[j * kFields + f];
    if (code != PLK_INGEST_OK) std::memset(&res[j], 0, sizeof(plk_proof));
    status[j] = code;
  }
  std::memcpy(out, res.data(), count * sizeof(plk_proof));
  return PLK_OK;
  PLK_API_END
}

int plk_ingest_last_ms(plk_ctx* ctx, float* decompress_ms, float* subgroup_ms) {
  if (!ctx) return PLK_E_ARG;
  const IngestWs* w = ctx->ingest_ws;
  if (decompress_ms) *decompress_ms = w ? w->decompress_ms : 0.f;
  if (subgroup_ms) *subgroup_ms = w ? w->subgroup_ms : 0.f;
  return PLK_OK;
}

int plk_verifier_verify_each_bytes(plk_ctx* ctx, plk_verifier* v, plk_opening_key* key, const uint8_t* in,
                                   const plk_fr* public_inputs, size_t count, int check_subgroup,
                                   uint8_t* verdict) {
  PLK_API_BEGIN
  if (!ctx || !v || !key || !in || !verdict || count == 0 || count > (1u << 24)) return PLK_E_ARG;
  const size_t npi = verifier_pi_count(v);
  if (npi && !public_inputs) return PLK_E_ARG;
  std::vector<plk_proof> proofs(count);
  std::vector<uint8_t> status(count);
  int st;
  if ((st = plk_proofs_ingest(ctx, in, count, check_subgroup, proofs.data(), status.data()))) return st;
  // compact the accepted proofs and their public inputs (through host memory)
  std::vector<size_t> where;
  for (size_t j = 0; j < count; ++j)
    if (status[j] == PLK_INGEST_OK) where.push_back(j);
  std::vector<plk_fr> pis(where.size() * npi);
  for (size_t k = 0; k < where.size(); ++k) {
    if (where[k] != k) proofs[k] = proofs[where[k]];
    if (npi) std::memcpy(&pis[k * npi], public_inputs + where[k] * npi, npi * sizeof(plk_fr));
  }
  std::vector<uint8_t> ok(where.size());
  if (!where.empty() &&
      (st = plk_verifier_verify_each(ctx, v, key, proofs.data(), npi ? pis.data() : nullptr, where.size(),
                                     ok.data())))
    return st;
  for (size_t j = 0; j < count; ++j) verdict[j] = (uint8_t)(0x10 | status[j]);
  for (size_t k = 0; k < where.size(); ++k) verdict[where[k]] = ok[k];
  return PLK_OK;
  PLK_API_END
}

}  // extern "C"
