// commit.hip — the commit paths of key compilation and the prover (prover.hpp): a batch of
// polynomials against the key's trimmed SRS, the same split over the ranks of a sharded prover,
// and round 1's choice of basis per wire.
#include <algorithm>
#include <cstring>
#include <vector>

#include "msm_common.hpp"
#include "prover.hpp"

namespace plk {

int key_commit(plk_key* key, MsmWorkspace& ws, const std::vector<const Fr*>& ptrs,
               const std::vector<size_t>& lens, plk_g1* outs, int* statuses, hipStream_t s,
               size_t cap, MsmSlotInfo* info) {
  const size_t max_points = std::min<size_t>(std::min<size_t>(key->srs->n, key->n_trim), cap);
  std::vector<size_t> use(lens.size());
  for (size_t i = 0; i < lens.size(); ++i) use[i] = std::min(lens[i], max_points);
  int overall = PLK_OK;
  for (size_t base = 0; base < ptrs.size(); base += kMaxSlots) {
    const size_t m = std::min<size_t>(kMaxSlots, ptrs.size() - base);
    const int r = msm_run_batch(key->srs, ws, ptrs.data() + base, use.data() + base,
                                lens.data() + base, m, outs + base,
                                statuses ? statuses + base : nullptr, s, 0, 1, 0,
                                info ? info + base : nullptr);
    if (r != PLK_OK && r != PLK_E_DEGREE) return r;
    if (r != PLK_OK) overall = r;
  }
  return overall;
}

namespace {

// Round 1's guard on a Lagrange-basis wire commit: the most entries one bucket may hold. n equal
// small values put n entries into one bucket, and the bucket reduction walks a bucket's partials
// in a single lane. The bound is a fixed number of accumulation tasks per bucket whatever n,
// 4 kChunkMax entries (a dense random column at c = 20 averages 26 per bucket), and never
// below 4 times what a dense column of this length puts into every bucket, W len / 2^(c-1):
// that is what the coefficient commit, the alternative, runs at anyway (n = 2^12 at c = 10:
// 208 per bucket).
uint32_t lagrange_bucket_max(const plk_srs* s, size_t len) {
  // (row-table layout: a random scalar gives 255 / (c + 2) + ~0.4 digits, not `windows`)
  const size_t per = s->naf ? 255 / (s->c + 2) + 1 : s->windows;
  const size_t dense = per * len >> (s->c - 1);
  return (uint32_t)std::max<size_t>(4 * kChunkMax, 4 * dense);
}

// The same commit group split over the ranks of a sharded prover (plk_prover_shard, SURVEY
// §8e): this rank's MSMs over its SRS slice [lo, hi) of every polynomial, one all-gather
// of (13 point words + status) per commit, and the fold of the partial points in rank order.
// The last rank also checks the tail [max_points, len) for the degree error, wherever that
// tail starts relative to its slice (an SRS longer than the circuit's trimmed one puts the
// last slice past it). Every rank takes part in the exchange even when its own MSMs failed,
// so no rank waits forever on a collective the others left.
// Bucket-range form (plk_prover_shard_buckets, round 6): every rank holds the key's whole SRS
// and window table and runs each commit of the group over ALL of its points, keeping only the
// digits of bucket range `rank` of `world` (msm_run_batch part / parts: its sort, accumulation
// and run-sum / bit-sum reduction cover 1/world of the 2^(c-1) buckets); its outputs are that
// range's shares, and the same exchange and fold give the commitments. Every part checks the
// degree tail itself, so every rank sees the same status.
int shard_commit(plk_prover* P, const std::vector<const Fr*>& ptrs,
                 const std::vector<size_t>& lens, plk_g1* outs, int* statuses, size_t cap) {
  plk_key* key = P->key;
  const size_t cnt = ptrs.size();
  const size_t max_points = std::min<size_t>(std::min<size_t>(key->srs->n, key->n_trim), cap);
  const bool buckets = P->shard_buckets;
  plk_srs* srs = buckets ? key->srs : P->shard;
  const uint64_t lo = buckets ? 0 : P->shard_lo, hi = buckets ? key->srs->n : lo + P->shard->n;
  const bool last = buckets || P->rank == P->world - 1;
  const uint32_t part = buckets ? (uint32_t)P->rank : 0, parts = buckets ? (uint32_t)P->world : 1;
  std::vector<const Fr*> lp(cnt);
  std::vector<size_t> luse(cnt), lchk(cnt);
  int local = PLK_OK;
  if (last && hi < max_points) local = PLK_E_ARG;  // the slices do not cover the trimmed SRS
  for (size_t i = 0; i < cnt; ++i) {
    const size_t use = std::min(lens[i], max_points);
    luse[i] = use > lo ? (size_t)(std::min<uint64_t>(use, hi) - lo) : 0;
    lchk[i] = luse[i];
    lp[i] = ptrs[i] + lo;
    if (last && lens[i] > use) {
      if (use >= lo) {
        lchk[i] = lens[i] - lo;  // the tail follows this slice's own points
      } else {
        // nothing of this polynomial falls in the slice: an empty MSM whose base is the
        // start of the tail, so the degree check reads [use, lens) (no SRS point is read)
        lp[i] = ptrs[i] + use;
        lchk[i] = lens[i] - use;
      }
    }
  }
  std::vector<plk_g1> shares(cnt, plk_g1{});
  std::vector<int> pst(cnt, PLK_OK);
  for (size_t base = 0; local == PLK_OK && base < cnt; base += kMaxSlots) {
    const size_t m = std::min<size_t>(kMaxSlots, cnt - base);
    const int r = msm_run_batch(srs, *P->ws, lp.data() + base, luse.data() + base,
                                lchk.data() + base, m, shares.data() + base, pst.data() + base,
                                P->stream, part, parts);
    if (r != PLK_OK && r != PLK_E_DEGREE) local = r;
  }
  // payload per commit: x[6], y[6], infinity, status
  constexpr size_t kWords = 14;
  std::vector<uint64_t> send(cnt * kWords), recv((size_t)P->world * cnt * kWords);
  for (size_t i = 0; i < cnt; ++i) {
    uint64_t* w = &send[i * kWords];
    std::memcpy(w, &shares[i], sizeof(plk_g1));
    w[13] = (uint64_t)(local != PLK_OK ? local : pst[i]);
  }
  if (P->allgather(P->allgather_user, send.data(), send.size() * 8, recv.data()) != 0)
    return PLK_E_DEVICE;
  int overall = PLK_OK;
  std::vector<plk_g1> pts((size_t)P->world);
  for (size_t i = 0; i < cnt; ++i) {
    int st = PLK_OK;
    for (int r = 0; r < P->world; ++r) {
      const uint64_t* w = &recv[((size_t)r * cnt + i) * kWords];
      std::memcpy(&pts[r], w, sizeof(plk_g1));
      if (w[13] != PLK_OK && (st == PLK_OK || st == PLK_E_DEGREE)) st = (int)w[13];
    }
    if (st != PLK_OK && st != PLK_E_DEGREE) return st;  // a rank's device / argument error
    if (statuses) statuses[i] = st;
    if (st != PLK_OK) {
      outs[i] = plk_g1{};
      overall = PLK_E_DEGREE;
      continue;
    }
    const int r = plk_g1_sum(pts.data(), pts.size(), &outs[i]);
    if (r != PLK_OK) return r;
  }
  return overall;
}

bool sharded(const plk_prover* P) { return P->shard || P->shard_buckets; }

}  // namespace

int prover_commit(plk_prover* P, const std::vector<const Fr*>& ptrs,
                  const std::vector<size_t>& lens, plk_g1* outs, int* statuses, size_t cap) {
  if (sharded(P)) return shard_commit(P, ptrs, lens, outs, statuses, cap);
  return key_commit(P->key, *P->ws, ptrs, lens, outs, statuses, P->stream, cap);
}

// From the Lagrange values on the key's Lagrange-basis SRS (the same group element as the commit
// of the blinded coefficients; a zero or sparse column, the bench chain's fourth wire, then has
// next to no MSM entries), guarded: a wire whose values pile more than lagrange_bucket_max
// entries onto one bucket (small equal values, a wire of bits) would run a single-lane chain in
// the bucket reduction, and is committed from its coefficients instead, like every wire of a
// sharded prover or of a key without the Lagrange SRS.
int commit_wires(plk_prover* P, const Fr* lag, const Fr* coef, uint64_t stride, plk_g1 out[4]) {
  plk_key* key = P->key;
  const size_t len = key->n + 2;
  bool hot[4] = {true, true, true, true};  // hot, or never tried: from the coefficients
  for (int c = 0; c < 4; ++c) P->commit_basis[c] = 0, P->commit_entries[c] = 0;
  if (key->lag && !sharded(P)) {
    const Fr* ptrs[4] = {lag, lag + stride, lag + 2 * stride, lag + 3 * stride};
    const size_t lens[4] = {len, len, len, len};
    MsmSlotInfo info[4];
    const int r = msm_run_batch(key->lag, *P->ws, ptrs, lens, lens, 4, out, nullptr, P->stream, 0,
                                1, lagrange_bucket_max(key->lag, len), info);
    if (r != PLK_OK) return r;
    for (int c = 0; c < 4; ++c) {
      hot[c] = info[c].hot;
      if (!hot[c]) P->commit_basis[c] = 1, P->commit_entries[c] = info[c].entries;
    }
  }
  std::vector<const Fr*> cp;
  std::vector<size_t> cl;
  int which[4];
  for (int c = 0; c < 4; ++c)
    if (hot[c]) which[cp.size()] = c, cp.push_back(coef + c * stride), cl.push_back(len);
  if (cp.empty()) return PLK_OK;
  plk_g1 cc[4];
  MsmSlotInfo info[4] = {};  // a sharded commit counts no entries
  const int r = sharded(P) ? shard_commit(P, cp, cl, cc, nullptr, SIZE_MAX)
                           : key_commit(key, *P->ws, cp, cl, cc, nullptr, P->stream, SIZE_MAX, info);
  if (r != PLK_OK) return r;
  for (size_t i = 0; i < cp.size(); ++i) {
    out[which[i]] = cc[i];
    P->commit_entries[which[i]] = info[i].entries;
  }
  return PLK_OK;
}

}  // namespace plk
