// internal.hpp — shared runtime objects behind the C ABI (include/plk.h).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/plk.h"
#include "abi.hpp"
#include "g1.hpp"

namespace plk {

#define PLK_HIP_TRY(expr)                                        \
  do {                                                           \
    hipError_t _e = (expr);                                      \
    if (_e != hipSuccess) {                                      \
      last_hip_error() = _e;                                     \
      return (_e == hipErrorOutOfMemory) ? PLK_E_OOM : PLK_E_DEVICE; \
    }                                                            \
  } while (0)

// Around the body of every extern "C" entry point that can throw: no C++ exception crosses the
// boundary, it comes back as a plk_status.
#define PLK_API_BEGIN try {
#define PLK_API_END                 \
  }                                 \
  catch (const std::bad_alloc&) {   \
    return PLK_E_OOM;               \
  }                                 \
  catch (...) {                     \
    return PLK_E_DEVICE;            \
  }

hipError_t& last_hip_error();

// a function shared by translation units of the library and not part of what it exports
#define PLK_LOCAL __attribute__((visibility("hidden")))

// blocks of b threads for a items
inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// 32 bytes from the OS (getrandom, std::random_device behind it); api.hip
void os_entropy(uint8_t seed[32]);

// N timing events, created on first use and destroyed with their holder
template <int N>
struct TimingEvents {
  hipEvent_t e[N] = {};
  TimingEvents() = default;
  TimingEvents(const TimingEvents&) = delete;
  TimingEvents& operator=(const TimingEvents&) = delete;
  ~TimingEvents() {
    for (hipEvent_t ev : e)
      if (ev) (void)hipEventDestroy(ev);
  }
  int create() {
    for (hipEvent_t& ev : e)
      if (!ev) PLK_HIP_TRY(hipEventCreate(&ev));
    return PLK_OK;
  }
};

// Device buffer owned by a context object.
struct DevBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) {
    o.ptr = nullptr;
    o.bytes = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      if (ptr) (void)hipFree(ptr);
      ptr = o.ptr;
      bytes = o.bytes;
      o.ptr = nullptr;
      o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() {
    if (ptr) (void)hipFree(ptr);
  }
  int alloc(size_t b) {
    if (ptr && bytes >= b) return PLK_OK;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
    if (b == 0) return PLK_OK;
    hipError_t e = hipMalloc(&ptr, b);
    if (e != hipSuccess) {
      ptr = nullptr;
      last_hip_error() = e;
      return e == hipErrorOutOfMemory ? PLK_E_OOM : PLK_E_DEVICE;
    }
    bytes = b;
    return PLK_OK;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(ptr);
  }
};

// Stream-ordered scratch freed on the same stream when the scope ends.
struct AsyncBuf {
  void* ptr = nullptr;
  hipStream_t s = nullptr;
  AsyncBuf() = default;
  AsyncBuf(const AsyncBuf&) = delete;
  AsyncBuf& operator=(const AsyncBuf&) = delete;
  int alloc(size_t bytes, hipStream_t st) {
    s = st;
    if (hipMallocAsync(&ptr, bytes > 32 ? bytes : 32, st) != hipSuccess) {
      ptr = nullptr;
      return PLK_E_OOM;
    }
    return PLK_OK;
  }
  ~AsyncBuf() {
    if (ptr) (void)hipFreeAsync(ptr, s);
  }
  Fr* fr() const { return static_cast<Fr*>(ptr); }
  template <class T>
  T* as() const {
    return static_cast<T*>(ptr);
  }
};

struct NttPass {
  uint32_t lp, lr, lt;  // log2 of: sub-transform length so far, radix, columns per block
};

}  // namespace plk

struct plk_domain {
  plk_ctx* ctx = nullptr;
  uint32_t log_n = 0;
  uint64_t n = 0;
  plk::Fr omega, omega_inv, n_inv, g, g_inv;  // Montgomery form (host copies)
  plk::DevBuf tw_fwd;        // w^e, e < n (R domain: the domain elements)
  plk::DevBuf tw_fwd_rx;     // w^e, R' domain (ffr.hpp), read by the NTT passes
  plk::DevBuf tw_inv;        // w^-e, e < n (R' domain)
  plk::DevBuf coset_pow;     // g^e, e < n (R' domain)
  plk::DevBuf icoset_scale;  // n^-1 * g^-e, e < n (R' domain)
  std::vector<plk::DevBuf> pass_tw_fwd, pass_tw_inv;  // per pass q > 0: w_{Rp}^{jk} [j][k] (R')
  // the inverse direction's last pass table times n^-1: a plain idft's scaling rides on the
  // inter-pass twiddle instead of a product per output (multi-pass plans only)
  plk::DevBuf pass_tw_inv_last;
  plk::DevBuf scratch;       // 2n elements (default scratch for plk_ntt_dev)
  plk::DevBuf io;            // n elements (host-buffer entry points stage through it)
  std::vector<plk::NttPass> plan;
  uint32_t le = 10;          // log2 elements per workgroup
};

namespace plk {
struct MsmWorkspace;
// Bucket-accumulation statistics of one MSM workspace (measurement only): the most recent
// batch and the cumulative figures since the last reset — k_accumulate time from
// dispatch-stamped events, launches, point additions and MSM points (scalar counts).
struct MsmStats {
  float last_accumulate_ms = 0.f;
  uint64_t last_point_adds = 0;
  uint32_t last_slots = 0;
  double cum_accumulate_ms = 0.0;
  uint64_t cum_launches = 0, cum_point_adds = 0, cum_points = 0;
  void reset_cum() {
    cum_accumulate_ms = 0.0;
    cum_launches = cum_point_adds = cum_points = 0;
  }
};
}

namespace plk {
struct KzgTable {
  DevBuf points, inf;  // G1Affine / uint8, 2n entries
};
}

struct plk_srs {
  plk_ctx* ctx = nullptr;
  size_t n = 0;              // number of SRS points
  uint32_t c = 16;           // window bits
  uint32_t windows = 16;     // ceil(256 / c)
  // balanced windows (round 5): when c does not divide 255, the top `narrow` windows are
  // c - 1 bits wide (narrow = c W - 255) and their digits come scaled by 2, their table rows
  // pre-divided by 2 (msm_prepare_srs, msm_digits.hpp digit_at): every window spreads over the whole
  // bucket range, without the short top window whose few digit values piled extra entries
  // onto a few hot buckets
  uint32_t narrow = 0;
  // row-table layout (msm_prepare_srs, msm_digits.hpp naf_walk): the table holds a row 2^p P for
  // every bit position p < rows = 255 instead of one per window (rows = windows otherwise), and a
  // scalar is recoded as a signed sliding window, <= windows odd digits. c and windows keep their
  // meaning: 2^(c-1) buckets, at most `windows` entries per scalar
  bool naf = false;
  uint32_t rows = 16;
  plk::DevBuf points;       // affine, plk::G1Affine (96 B), n entries; inf flags separate
  plk::DevBuf inf;           // uint8 per point
  plk::DevBuf table;         // precomputed 2^(c*w) * P_i, affine, windows * n entries
  plk::DevBuf table_inf;     // uint8, windows * n
  bool has_inf = false;      // any point at infinity in the SRS (slow-path flag checks)
  // what is known of the points (srs_io.hip): canonical and on the curve / of order r. Set by
  // plk_srs_load_bytes and by a plk_srs_verify that got past the step; plk_srs_load and
  // plk_srs_setup leave both false, so plk_srs_verify runs every step on their SRS
  bool points_checked = false, subgroup_checked = false;
  double verify_fold_ms = 0.0, verify_pairing_ms = 0.0;  // the most recent plk_srs_verify
  // the leading points known to lie in G1 without a test (plk_srs_setup computes multiples of the
  // generator) or by the prefix test of plk_kzg_open_domain; subgroup_checked covers every point
  size_t g1_prefix = 0;
  // plk_kzg_open_domain's tables, one per log_n (kzg.hip): the 2n-point transform of the reversed,
  // identity-padded SRS prefix in affine form, 2n * 97 bytes each, built on first use. The tables
  // of plk_kzg_open_cosets sit beside them under log_n | log_l << 8: 2^log_l transforms of 2r
  // points, residue a's at [a 2r, (a + 1) 2r); log_l = 0 is open_domain's own table
  std::map<uint32_t, plk::KzgTable> kzg_tables;
  plk::DevBuf staging;       // host-scalar entry points stage through it
  // the workspace of the SRS's own entry points (plk_msm / plk_commit*: one thread at a
  // time); concurrent provers sharing this SRS each bring their own (plk_prover)
  std::unique_ptr<plk::MsmWorkspace> ws;
  plk_srs();
  ~plk_srs();
};

namespace plk {
struct VarMsmWs;
struct IngestWs;
struct CheckWs;
}

struct plk_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::map<uint32_t, std::unique_ptr<plk_domain>> domains;
  std::mutex mu;
  // workspace of the variable-base MSM (msm_var.hip), made on first use, freed with the context
  plk::VarMsmWs* var_ws = nullptr;
  // buffers, events and timings of the ingest stage (ingest.hip), made on first use
  plk::IngestWs* ingest_ws = nullptr;
  // kernel times of the most recent plk_srs_load_bytes (srs_io.hip; measurement only)
  float srs_decode_ms = 0.f, srs_subgroup_ms = 0.f;
  // kernel time of the most recent scalar multiplication batch (g1_mul.hip; measurement only)
  float g1_mul_ms = 0.f;
  // buffers of plk_composer_check (circuit_check.hip), made on first use, and the kernel time of
  // the most recent check or diagnosis on this context (measurement only)
  plk::CheckWs* check_ws = nullptr;
  float check_ms = 0.f;
  // HIP-event times of the most recent plk_kzg_open_domain / _cosets (kzg.hip; measurement only): the
  // transforms, the pointwise multiplication, the table build (0 when the table was cached)
  float kzg_transform_ms = 0.f, kzg_mul_ms = 0.f, kzg_table_ms = 0.f;
};

namespace plk {
// Page-locked host buffer: the prover's host<->device transfers go through these. A
// pageable hipMemcpy pins and unpins its pages on every call, and the page-table and
// TLB-shootdown work that comes with it slowed a concurrent composer synthesis ~1.6x.
struct PinnedBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() {
    if (ptr) (void)hipHostFree(ptr);
  }
  int alloc(size_t b, unsigned flags = hipHostMallocDefault) {
    if (ptr && bytes >= b) return PLK_OK;
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    bytes = 0;
    if (b == 0) return PLK_OK;
    const hipError_t e = hipHostMalloc(&ptr, b, flags);
    if (e != hipSuccess) {
      ptr = nullptr;
      last_hip_error() = e;
      return e == hipErrorOutOfMemory ? PLK_E_OOM : PLK_E_DEVICE;
    }
    bytes = b;
    return PLK_OK;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(ptr);
  }
};

// Host wait for all work queued on `s`, blocking in the driver instead of spinning: the
// prover's host thread waits at every commitment, and a spinning wait steals the core a
// concurrent composer synthesis (or any other host work) runs on. One event per thread.
inline hipError_t stream_wait(hipStream_t s) {
  thread_local hipEvent_t ev = nullptr;
  if (!ev) {
    const hipError_t e = hipEventCreateWithFlags(&ev, hipEventBlockingSync | hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  const hipError_t e = hipEventRecord(ev, s);
  if (e != hipSuccess) return e;
  return hipEventSynchronize(ev);
}

// RAII device guard
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
  }
};

int ntt_build_domain(plk_domain* d);
// Per-launch strides of a batch of `count` transforms (vector v: in + v * in_stride, out + v *
// out_stride, pre-scale table pre + v * pre_stride, post-scale table post + v * post_stride;
// a stride of 0 shares one input / table between the vectors). pre / post: R'-domain tables
// replacing the domain's g^j (forward coset) / n^-1 g^-j (inverse coset) tables.
struct NttBatch {
  uint64_t in_stride = 0, out_stride = 0;
  const Fr* pre = nullptr;
  uint64_t pre_stride = 0;
  const Fr* post = nullptr;
  uint64_t post_stride = 0;
  // group > 0: vector v = g * group + m reads in + g * in_group_stride + m * in_stride and its
  // pre / post tables at m * pre_stride / m * post_stride (several polynomials' coset blocks in
  // one launch); outputs stay at v * out_stride
  uint32_t group = 0;
  uint64_t in_group_stride = 0;
};
struct NttStrides {  // kernel-side view
  uint64_t in, out, pre, post, in_group;
  uint32_t group_in, group_post;  // grouping of the first pass' inputs / the last pass' post table
};
int ntt_run_batch(plk_domain* d, const Fr* in, Fr* out, size_t len_in, int dir, int coset,
                  Fr* scratch, hipStream_t stream, uint32_t count, const NttBatch& b);
// pre_table (forward coset transforms only): R'-domain multipliers for the len_in inputs
// in place of the domain's g^j table — a scaled table (c g^j) yields the evaluations of c p
int ntt_run(plk_domain* d, const Fr* in, Fr* out, size_t len_in, int dir, int coset,
            Fr* scratch, hipStream_t stream, uint32_t count, const Fr* pre_table = nullptr);
// An SRS object with its point and infinity arrays allocated (api.hip srs_alloc), and what every
// loader ends with once they are filled: the has_inf scan and the MSM table (srs_finish).
int srs_new(plk_ctx* ctx, size_t n, std::unique_ptr<plk_srs>& s);
int srs_complete(plk_srs* s);
// force_naf (with force_c): the table layout of the SRS whose c is taken, 1 row table, 0 window table
int msm_prepare_srs(plk_srs* s, hipStream_t stream, uint32_t force_c = 0, bool own_ws = true,
                    int force_naf = -1);
// The table layout msm_prepare_srs gives an SRS of n points at window size c (PLK_MSM_NAF, the
// default for large SRSs, wide sets only) before it tries the allocation, and whether a table of
// `bytes` may be tried at all (PLK_MSM_TABLE_CAP, bytes: a cap on the row table, 0 = none)
bool msm_naf_policy(size_t n, uint32_t c, bool c_from_env);
bool msm_naf_table_allowed(size_t bytes);
// The Lagrange-basis SRS of `dom` from the first dom->n + 3 points of `src` (lagrange.hip):
// [L_i(tau)]_1 for i < n, then [tau^(n+t)]_1 - [tau^t]_1 for t < 3; an ordinary SRS with src's
// window size. PLK_E_ARG when src has fewer than n + 3 points.
int srs_lagrange_build(plk_srs* src, plk_domain* dom, bool own_ws, plk_srs** out);
int msm_run(plk_srs* s, const Fr* d_scalars, size_t len, size_t check_len, plk_g1* out,
            hipStream_t stream);
// The SRS (window table) is only read: any number of threads may run batches on one SRS
// concurrently, each with its own workspace `w` and stream.
// part / parts (parts a power of two, 1 = the whole MSM): only the buckets of the part's
// range [part, part + 1) * 2^(c-1) / parts (wide bucket sets, 2^(c-1) / parts >= 2^14); the
// parts' outputs sum to the whole MSM's (one large MSM split over GPUs by bucket
// range, each GPU's reduction over its own buckets only).
// guard_limit > 0: a slot whose largest bucket holds more than guard_limit entries is not
// accumulated or reduced (msm_sort.hip k_guard); info[k].hot reports it and outs[k] is void. info
// (optional, `count` records): each slot's entry count and, for a guarded batch, its largest
// bucket count.
struct MsmSlotInfo {
  uint32_t entries, max_count;
  bool hot;
};
int msm_run_batch(plk_srs* s, MsmWorkspace& w, const Fr* const* d_scalars, const size_t* lens,
                  const size_t* check_lens, size_t count, plk_g1* outs, int* statuses,
                  hipStream_t stream, uint32_t part = 0, uint32_t parts = 1,
                  uint32_t guard_limit = 0, MsmSlotInfo* info = nullptr);
// whether msm_run_batch accepts `parts` bucket ranges on this SRS (a power of two; for
// parts > 1 a wide bucket set, 2^(c-1) above the LDS histogram's range, and >= 2^14 buckets
// per part)
bool msm_parts_ok(const plk_srs* s, uint32_t parts);
// Variable-base MSM (msm_var.hip), device pointers, on `stream`: outs[k] = sum over
// i in [starts[k], starts[k] + lens[k]) of scalars[i] * points[i], k < count <= kMaxSlots, as one
// batch. d_points: n points in the ABI layout (plk_g1), d_scalars: n Montgomery scalars. The
// kernels are stream-ordered; the call returns after the host tail (it waits for the stream).
// PLK_E_ARG when a finite point is off the curve or not canonical.
int msm_var_run(plk_ctx* ctx, const plk_g1* d_points, const Fr* d_scalars, size_t n,
                const size_t* starts, const size_t* lens, size_t count, plk_g1* outs,
                hipStream_t stream);
void msm_var_ws_delete(VarMsmWs* w);
void ingest_ws_delete(IngestWs* w);
void check_ws_delete(CheckWs* w);  // circuit_check.hip
// the number of public inputs a verifier was created with (verifier.hip)
size_t verifier_pi_count(const plk_verifier* v);
// The batched pairing check (pairing.hip) on device buffers, stream-ordered on the context's
// stream: d_ok[j] = 1 iff e(d_pairs[j].c, H) == e(d_pairs[j].w, beta_h). The points must be
// canonical and on the curve (the caller's check). pairing_last_ms: the kernel's time once the
// stream has passed it.
int pairing_check_dev(plk_ctx* ctx, plk_opening_key* key, const plk_kzg_pair* d_pairs, size_t count,
                      uint8_t* d_ok);
int pairing_last_ms(plk_opening_key* key, float* ms);
MsmWorkspace* msm_workspace_new();
void msm_workspace_delete(MsmWorkspace* w);
const MsmStats& msm_workspace_stats(const MsmWorkspace& w);
MsmStats& msm_workspace_stats(MsmWorkspace& w);
void fr_root_of_unity(uint32_t log_n, Fr& omega);
int ntt_vanishing(plk_domain* d, uint64_t deg, Fr* d_out, hipStream_t s);
// plk_debug_ntt_lazy_op (include/plk.h): the pass kernel's lazy butterfly helpers on host rows
int ntt_lazy_op(plk_ctx* ctx, int op, const uint32_t* in, uint32_t* out, size_t n);
// out[e] = base^e * scale, e < n (R domain; to_rx: converted to the R' domain)
int ntt_power_table(Fr* out, const Fr& base, const Fr& scale, uint64_t n, bool to_rx,
                    hipStream_t s);
int srs_generate(plk_srs* s, const Fr& tau_mont, uint64_t start, hipStream_t stream);
// Batched scalar multiplication (g1_mul.hip): out[i] = [scal[i]] pts[i] in canonical affine form
// with identity flags; device arrays of n entries, the points in G1 (the caller's check), the
// scalars canonical Montgomery. Waits for the stream.
int g1_mul_dev(plk_ctx* ctx, const G1Affine* pts, const uint8_t* inf, const Fr* scal, uint64_t n,
               G1Affine* out, uint8_t* out_inf, hipStream_t s);
// The transform over G1 of 2^log_n device-resident XYZZ points (g1_ntt.hip), in place, natural
// order in and out: dir = +1 forward, -1 inverse (with n^-1 unless scale is false). kXyzz: the
// twiddle multiplication inside the butterfly on XYZZ points, stream-ordered, exact for any points
// of the curve. kGlv: affine between the levels, the multiplications through g1_mul_dev (waits for
// the stream at every level); the points must lie in G1.
enum class G1NttForm { kXyzz, kGlv };
int g1_ntt_run(plk_ctx* ctx, G1xyzz* points, uint32_t log_n, int dir, hipStream_t stream, bool scale = true,
               G1NttForm form = G1NttForm::kXyzz);
// `batch` independent transforms of 2^log_n points each, one after the other in `points`: one launch
// per level over all of them, so the batch is one multiplication chain per level deep, not `batch`.
// batch = 1 is g1_ntt_run.
int g1_ntt_run_batch(plk_ctx* ctx, G1xyzz* points, uint32_t log_n, uint64_t batch, int dir, hipStream_t stream,
                     bool scale = true, G1NttForm form = G1NttForm::kXyzz);
// out[t] = sum_{a < rows} pts[a * cols + t] as XYZZ, by the complete group law (g1_colsum.hip);
// stream-ordered with its own stream-ordered scratch
int g1_colsum_dev(const G1Affine* pts, const uint8_t* inf, uint64_t rows, uint64_t cols, G1xyzz* out,
                  hipStream_t stream);
// out[i] = sum_{k < count} rho[k] zinv[k]^i c[k * l + i], i < l (g1_colsum.hip): the fold of coset
// interpolants (kzg.hip); Montgomery scalars on the device, stream-ordered
int fr_interp_reduce_dev(const Fr* c, const Fr* rho, const Fr* zinv, uint64_t count, uint64_t l, Fr* out,
                         hipStream_t stream);
// out[i] = pts[first + i] (rev: pts[first - i]) for i < m as XYZZ, the identity for m <= i < n
int g1_xyzz_load(const G1Affine* pts, const uint8_t* inf, uint64_t first, bool rev, uint64_t m, uint64_t n,
                 G1xyzz* out, hipStream_t stream);
// The canonical / on-curve pass and the subgroup kernel over the first n points of an SRS not yet
// known to be in G1 there (srs_io.hip): *any with the smallest offending index; the SRS's flags
// (or g1_prefix, for n < srs->n) record a clean pass.
int srs_ensure_g1_prefix(plk_srs* srs, uint64_t n, bool* any, uint64_t* idx);
// d_out[i] = s^i, i < n (Montgomery), stream-ordered
int fr_powers_dev(const Fr& s_mont, uint64_t n, Fr* d_out, hipStream_t s);
}  // namespace plk
