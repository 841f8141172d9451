// msm_reduce.hip — the fixed-base MSM's bucket reduction (design: msm.hip): from the
// accumulation partials to the few points T_j the host's Horner tail reads back. Narrow bucket
// sets sum each bucket (k_bucket_sum), wide ones form run suffix sums (k_runsum1/2); both end in
// the bit-sum trees (k_bitsum1, k_bitsum2). msm_reduce() at the end launches a batch's reduction.
#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "msm_common.hpp"
#include "g1r.hpp"

namespace plk {

namespace {

// Bucket sums S_b = sum of bucket b's accumulation partials (task_off[b] .. task_off[b+1]):
// 2^lp lanes per bucket (consecutive lanes of one wave, 2^lp <= 16), each adding every
// 2^lp-th partial, then a tree over the lanes through cross-lane shuffles of the packed
// point (no LDS: these long add chains would otherwise hold 48 KiB of a CU's LDS per
// workgroup while other proofs' kernels wait for it). 2^lp is sized on the host to the
// partials per bucket, so the sequential chain stays ~PLK_LANE_PARTIALS additions at every
// MSM size, unless the grid is already full.
__device__ __forceinline__ RFp shfl_down_rfp(const RFp& v, uint32_t h) {
  Fp x = rx_pack(v);
#pragma unroll
  for (int i = 0; i < 12; ++i) x.v[i] = __shfl_down(x.v[i], h, 64);
  return rx_unpack(x);
}

__device__ __forceinline__ G1R shfl_down_g1r(const G1R& v, uint32_t h) {
  G1R o;
  o.X = shfl_down_rfp(v.X, h);
  o.Y = shfl_down_rfp(v.Y, h);
  o.ZZ = shfl_down_rfp(v.ZZ, h);
  o.ZZZ = shfl_down_rfp(v.ZZZ, h);
  return o;
}

// The trees' addition. LAZY: g1r_add_lazy
// (straight-line, exceptional cases repaired after; ~275 VGPRs) or the branching g1r_add
// (~205 VGPRs: two waves per SIMD). One dependent addition costs a lone wave 12.5 / 14.3 us
// (tools/ubench_tail.hip, profiles/r03_ubench_tail.txt).
template <bool LAZY>
__device__ __forceinline__ G1R g1r_add_t(const G1R& a, const G1R& b) {
  return LAZY ? g1r_add_lazy(a, b) : g1r_add(a, b);
}

// QUAD: every "lane" of the reduction trees (k_bucket_sum, k_bitsum1/2) is a quad of 4 lanes
// holding the same values, adding with g1r_add_quad (g1r.hpp: one product per lane, ~3.5
// products issued per addition instead of ~15) — these trees are a chain of dependent
// additions on a few waves, so their time is one wave's issue of each level. Shuffles move by
// whole quads. Which form a batch takes: MsmWorkspace::tail_quad.
template <bool QUAD>
struct TailUnit {
  static constexpr uint32_t S = QUAD ? 4 : 1;  // lanes per unit
  uint32_t u, l;                               // unit index, lane in the unit
  __device__ explicit TailUnit(uint32_t tid) : u(tid / S), l(tid % S) {}
  template <bool LAZY>
  __device__ __forceinline__ G1R add(const G1R& a, const G1R& b) const {
    if constexpr (QUAD) return g1r_add_quad(a, b, l);
    else return g1r_add_t<LAZY>(a, b);
  }
  __device__ __forceinline__ G1R down(const G1R& v, uint32_t h) const { return shfl_down_g1r(v, h * S); }
  // sum over groups of w consecutive units (w a power of two, groups aligned, inside one wave;
  // e = unit index in the group): unit e = 0 of each group ends with the group's sum
  template <bool LAZY>
  __device__ __forceinline__ G1R tree(G1R acc, uint32_t e, uint32_t w) const {
    for (uint32_t h = w >> 1; h >= 1; h >>= 1) {
      const G1R o = down(acc, h);
      if (e < h) acc = add<LAZY>(acc, o);
    }
    return acc;
  }
};

// k_bitsum1: the branching addition (single-lane form) at two waves per SIMD (2 workgroups of
// 256 per CU: a lone 2^20 MSM's 512 groups in one round instead of two)
#ifndef PLK_BITSUM_WAVES
#define PLK_BITSUM_WAVES 2
#endif

template <bool QUAD>
__global__ void __launch_bounds__(256) k_bucket_sum(const uint32_t* __restrict__ task_off,
                                                    uint32_t B, uint32_t lp, uint64_t task_stride,
                                                    const G1xyzz* __restrict__ partials,
                                                    G1xyzz* __restrict__ bsum) {
  const uint32_t slot = blockIdx.y;
  const TailUnit<QUAD> T(blockIdx.x * 256 + threadIdx.x);  // unit = one lane of the bucket's 2^lp
  const uint32_t P = 1u << lp, s = T.u & (P - 1);
  const uint32_t b = T.u >> lp;
  task_off += (size_t)slot * (B + 1);
  partials += (size_t)slot * task_stride;
  // the branching g1r_add here: ~200 VGPRs (2 waves per SIMD) against ~325 for the lazy form
  G1R acc = g1r_infinity();
  if (b < B)
    for (uint32_t t = task_off[b] + s; t < task_off[b + 1]; t += P) acc = T.template add<false>(acc, ld_g1r(&partials[t]));
  acc = T.template tree<false>(acc, s, P);  // units s < h add unit s + h (same bucket)
  if (s == 0 && T.l == 0 && b < B) st_g1r(&bsum[(size_t)slot * B + b], QUAD ? g1r_lazy_finish(acc) : acc);
}

#ifndef PLK_RUNSUM_WAVES
#define PLK_RUNSUM_WAVES 1  // ~270 VGPRs; a 2-wave cap spills in the loop (runsum1 3.43 -> 3.07 ms per proof uncapped)
#endif
// Wide bucket sets, reduction: runs of K = 2^rb consecutive buckets b = rK + t.
//   sum_b (b + 1) S_b = sum_r (T_r + rK Y_r) = K (sum_r (r + 1) Y_r - sum_r Y_r) + sum_r T_r,
//   R_(r,t) = sum_(t' >= t) S_(rK+t') (suffix sums), Y_r = R_(r,0), T_r = sum_t R_(r,t).
// 2 additions per bucket with every lane busy (the bit-sum trees over 2^19 buckets left most
// lanes idle); the weighted sum over the runs is the bit-sum reduction, sum_r Y_r (its A)
// and sum_r T_r extra outputs of it, the host multiplies by K. Two kernels with ONE
// accumulator each (both chains in one lane need 3 live points: over 256 VGPRs).
// kRunBits, kRunBitsMin, kRunLanes and run_bits(): msm_common.hpp.
//
// Step 1, lane r: the suffix sums R_(r,t), t = K-1 .. 0, straight from the bucket's
// accumulation partials (S_b is never formed: R += S_b is the same sum taken partial by
// partial), stored lazily (X < 8p, Y < 4p fit the packed layout) to rsum[b].
__global__ void __launch_bounds__(256, PLK_RUNSUM_WAVES) k_runsum1(const uint32_t* __restrict__ task_off, uint32_t B, uint32_t rb,
                                                 uint64_t task_stride,
                                                 const G1xyzz* __restrict__ partials,
                                                 G1xyzz* __restrict__ rsum) {
  const uint32_t K = 1u << rb;
  const uint32_t slot = blockIdx.y, NR = B >> rb;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= NR) return;
  task_off += (size_t)slot * (B + 1);
  partials += (size_t)slot * task_stride;
  rsum += (size_t)slot * B;
  // the rare path's copy of the accumulator waits in LDS, not in 56 live registers
  __shared__ G1xyzz s_prev[256];
  G1xyzz* prev = &s_prev[threadIdx.x];
  G1R R = g1r_infinity();
  uint32_t pe = task_off[r * K + K];
  for (uint32_t t = K; t-- > 0;) {
    const uint32_t b = r * K + t;
    const uint32_t p0 = task_off[b];
    for (uint32_t p = p0; p < pe; ++p) {
      st_g1r(prev, R);
      G1R c = g1r_add_lazy_sl(R, ld_g1r(&partials[p]));
      if (rx_is_zero(c.ZZ)) c = g1r_add_lazy_fix(ld_g1r(prev), ld_g1r(&partials[p]), c.X);  // rare
      R = c;
    }
    pe = p0;
    st_g1r(&rsum[b], R);
  }
}

// Step 2, lane r: T_r = sum_t R_(r,t) and Y_r = R_(r,0) (canonical [0, 2p) coordinates for
// the bit sums).
__global__ void __launch_bounds__(256, PLK_RUNSUM_WAVES) k_runsum2(uint32_t B, uint32_t rb, const G1xyzz* __restrict__ rsum,
                                                 G1xyzz* __restrict__ ys, G1xyzz* __restrict__ ts) {
  const uint32_t K = 1u << rb;
  const uint32_t slot = blockIdx.y, NR = B >> rb;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= NR) return;
  rsum += (size_t)slot * B + (size_t)r * K;
  __shared__ G1xyzz s_prev[256];  // as in k_runsum1
  G1xyzz* prev = &s_prev[threadIdx.x];
  G1R T = ld_g1r(&rsum[0]);
  for (uint32_t t = 1; t < K; ++t) {
    // the suffix sums past a run's last filled bucket are infinity: a near-empty slot (a
    // sparse Lagrange-basis column) pays a load and a test per step, not an addition and its
    // repair path
    const G1R v = ld_g1r(&rsum[t]);
    if (g1r_is_inf(v)) continue;
    st_g1r(prev, T);
    G1R c = g1r_add_lazy_sl(T, v);
    if (rx_is_zero(c.ZZ)) c = g1r_add_lazy_fix(ld_g1r(prev), ld_g1r(&rsum[t]), c.X);  // rare
    T = c;
  }
  st_g1r(&ys[(size_t)slot * NR + r], g1r_lazy_finish(ld_g1r(&rsum[0])));
  st_g1r(&ts[(size_t)slot * NR + r], g1r_lazy_finish(T));
}

// Bucket reduction sum_b (b+1) S_b, split per workgroup g of 256 buckets b = 256g + u,
// u = 16a + c (a, c < 16):
//   sum_u (256g + u + 1) S_(g,u) = sum_(j<8) 2^j T_j(g) + (256g + 1) A_g,
//   T_j(g) = sum of S_(g,u) over u with bit j set,  A_g = sum_u S_(g,u).
// With row sums Row_a = sum_c S_(g,16a+c) and column sums Col_c = sum_a S_(g,16a+c), T_j for
// j < 4 is a sum of the 8 columns with bit j of c set and T_(4+i) a sum of the 8 rows with
// bit i of a set; A_g is the sum of the rows: 480 + 71 additions per 256 buckets instead of
// the 1 144 of bit sums taken over the buckets themselves.
// k_bitsum1 (one workgroup per g): the bucket sums S (k_bucket_sum), the 32
// row / column sums (8 consecutive lanes each: one addition, then a 3-level shuffle tree),
// then the 9 outputs from them (wave 0). out[slot][g][0..7] = T_j(g), [8] = A_g; with `zin`
// (wide bucket sets) also [9] = the plain sum of the group's 256 Z values (k_runsum):
// kBitsumOut = 10 records per group (msm_common.hpp).

// k_bitsum1's fold of k_bitsum2 (done == nullptr: off): per-slot arrival counters (zero
// between batches), the readback record's bit sums and entry counts, as k_bitsum2 takes them
struct BitsumFold {
  uint32_t* done;
  G1xyzz* out2;
  const uint32_t* offsets;
  uint32_t* entries;
  uint32_t B, nbits, nout;
};

// k-th of the 8 indices in [0, 16) with bit j set
__device__ __forceinline__ uint32_t with_bit(uint32_t k, uint32_t j) {
  return ((k >> j) << (j + 1)) | (1u << j) | (k & ((1u << j) - 1u));
}

// threads of k_bitsum1: 4 units per row / column sum, 1 or 4 lanes per unit. Quads stay at 8
// waves per workgroup (2 per SIMD: the quad addition needs ~250 VGPRs), so with Z (48 sums) the
// group takes TWO workgroups (blockIdx.z = role): the 32 row / column sums and their outputs
// 0..8, and the 16 plain-sum rows and output 9, side by side instead of 8-member chains
constexpr uint32_t bitsum1_threads(bool z, bool quad) {
  return quad ? 512 : (z ? 192 : 128);
}
template <bool Z, bool QUAD>
__global__ void __launch_bounds__(bitsum1_threads(Z, QUAD), PLK_BITSUM_WAVES) k_bitsum1(uint32_t B, const G1xyzz* __restrict__ bsum,
                                                                           const G1xyzz* __restrict__ zin,
                                                                           G1xyzz* __restrict__ out,
                                                                           BitsumFold fold) {
  // the group's values (buckets or run sums Y; with Z also the 256 plain-sum values) are
  // read straight from HBM and the trees run over cross-lane shuffles: LDS holds only the
  // NS row / column sums (9 KiB instead of 105 — a resident k_bitsum1 used to keep the other
  // proofs' NTT passes off its CU).
  // The NS sums of 16 take 4 consecutive units each, and each unit first adds its 4 members
  // in sequence (every unit busy), then a 2-level shuffle tree: 3 + 2 levels on NS / 16 waves.
  // The tree kernels are issue-bound — a wave issues the whole addition however few of its
  // lanes are active — so units idle in a shuffle level cost as much as busy ones: 8 units
  // per sum with 2 members each (3-level tree) issued twice the wave-additions (round 3:
  // 8 waves x 4 levels + 4 against 3 waves x 5 levels + 4 per group).
  constexpr uint32_t NS = Z ? 48 : 32;
  constexpr bool SPLIT = Z && QUAD;  // two workgroups per group (bitsum1_threads)
  constexpr uint32_t NSU = 4, MEM = 16 / NSU;  // units per sum, members per unit
  constexpr uint32_t NU = bitsum1_threads(Z, QUAD) / TailUnit<QUAD>::S;  // units
  constexpr bool LZ = false;
  __shared__ G1xyzz sh[NS];
  const uint32_t slot = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const uint32_t role = SPLIT ? blockIdx.z : 0;
  const TailUnit<QUAD> T(tid);
  out += ((size_t)slot * gridDim.x + g) * kBitsumOut;
  auto value = [&](uint32_t x) -> G1R {  // x < 256: bsum, else zin; past B: infinity
    const uint32_t b = g * 256 + (x & 255);
    const G1xyzz* src = x < 256 ? bsum : zin;
    return b < B ? ld_g1r(&src[(size_t)slot * B + b]) : g1r_infinity();
  };
  {  // sum q < 16: row a = q (members 16q + c); 16 <= q < 32: column c = q - 16 (members
     // c + 16a); q >= 32 (Z): row q - 32 of the plain-sum values. Unit e < NSU of the sum's
     // NSU takes members MEM e .. MEM e + MEM - 1 of its row / column.
    const uint32_t q = T.u / NSU + (role ? 32 : 0), e = T.u % NSU;
    auto member = [&](uint32_t i) {  // i-th member of sum q, i < 16
      return q < 16 ? 16 * q + i : q < 32 ? (q - 16) + 16 * i : 256 + 16 * (q - 32) + i;
    };
    if (q < NS && (!SPLIT || role || q < 32)) {  // uniform per sum (its NSU units)
      G1R acc = value(member(MEM * e));
#pragma unroll 1
      for (uint32_t i = 1; i < MEM; ++i) acc = T.template add<LZ>(acc, value(member(MEM * e + i)));
      acc = T.template tree<LZ>(acc, e, NSU);
      if (e == 0 && T.l == 0) st_g1r(&sh[q], acc);
    }
  }
  __syncthreads();
  // units 0..31 = T_0..T_7, 4 units each (2 terms per unit); units 32..39 = A_g, 8 units
  // (rows 2e, 2e + 1); with Z units 40..47 = the plain sum (its rows 2e, 2e + 1); then trees
  // (unit groups never straddle a wave: 4 or 8 units of 1 or 4 lanes, aligned)
  if (T.u < 64) {
    // (SPLIT: role 0 the units 0..39, role 1 the plain sum as units 40..47)
    const uint32_t t = role ? 40 + T.u : T.u;
    const bool on = role ? T.u < 8 : t < (Z && !SPLIT ? 48u : 40u);
    const uint32_t s = t < 32 ? t >> 2 : t < 40 ? 8 : 9, e = t < 32 ? t & 3 : (t - 32) & 7;
    const uint32_t w = t < 32 ? 4 : 8;
    uint32_t i0 = 0, i1 = 0;
    if (s < 4) {  // columns c with bit s
      i0 = 16 + with_bit(2 * e, s);
      i1 = 16 + with_bit(2 * e + 1, s);
    } else if (s < 8) {  // rows a with bit s - 4
      i0 = with_bit(2 * e, s - 4);
      i1 = with_bit(2 * e + 1, s - 4);
    } else if (on) {  // all rows (A_g) / all plain-sum rows
      i0 = (s == 8 ? 0 : 32) + 2 * e;
      i1 = i0 + 1;
    }
    G1R acc = g1r_infinity();
    if (on) acc = T.template add<LZ>(ld_g1r(&sh[i0]), ld_g1r(&sh[i1]));
    for (uint32_t h = 4; h >= 1; h >>= 1) {  // groups of w consecutive units
      const G1R o = T.down(acc, h);
      if (on && e < h && h < w) acc = T.template add<LZ>(acc, o);
    }
    if (on && e == 0 && T.l == 0) st_g1r(&out[s], acc);
  }
  if (!fold.done) return;
  // few groups (G <= kFoldMaxGroups): the slot's last workgroup to finish runs k_bitsum2's sums
  // here (one dispatch fewer per batch; small proofs are dispatch-rate bound). Release this
  // group's outputs, count it in, and the last one acquires the others' before reading them.
  __shared__ uint32_t s_last;
  __threadfence();
  __syncthreads();
  if (tid == 0) s_last = atomicAdd(&fold.done[slot], 1u) == gridDim.x * gridDim.z - 1 ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  const G1xyzz* in = out - (size_t)g * kBitsumOut;  // this slot's groups
  const uint32_t e = T.u & 7, G = gridDim.x;
  for (uint32_t j0 = 0; j0 < fold.nout; j0 += NU / 8) {  // uniform trip count: the trees shuffle
    const uint32_t j = j0 + (T.u >> 3);
    G1R acc = g1r_infinity();
    if (j < fold.nout) {  // output j: 8 units, unit e takes the groups g = e mod 8
      for (uint32_t gg = e; gg < G; gg += 8) {
        const G1xyzz* v = &in[(size_t)gg * kBitsumOut];
        if (j >= fold.nbits) {  // wide sets: the plain sums (j = nbits) and the A_g (nbits + 1)
          acc = T.template add<LZ>(acc, ld_g1r(&v[j == fold.nbits ? 9 : 8]));
        } else if (j < 8) {
          acc = T.template add<LZ>(acc, ld_g1r(&v[j]));
          if (j == 0) acc = T.template add<LZ>(acc, ld_g1r(&v[8]));
        } else if ((gg >> (j - 8)) & 1u) {
          acc = T.template add<LZ>(acc, ld_g1r(&v[8]));
        }
      }
    }
    acc = T.template tree<LZ>(acc, e, 8);
    if (j < fold.nout && e == 0 && T.l == 0) st_g1r(&fold.out2[(size_t)slot * fold.nout + j], g1r_lazy_finish(acc));
  }
  if (tid == 0) {
    fold.entries[slot] = fold.offsets[(size_t)slot * (fold.B + 1) + fold.B];
    fold.done[slot] = 0;  // ready for the next batch (stream order)
  }
}

// Workgroup j of slot: T_j = sum_g T_j(g) for 0 < j < 8; T_0 = sum_g (T_0(g) + A_g);
// T_(8+i) = sum_(g: bit i of g) A_g; wide bucket sets: j = nbits sum_g of the plain sums,
// j = nbits + 1 sum_g A_g.
// Also the batch's readback record (ReadbackHeader): workgroup (0, slot) copies the slot's
// entry count (its point additions, offsets[B]) next to the flags k_any_nonzero stamped, so
// the host reads flags, counts and bit sums with ONE copy.
// k_bitsum2's additions: lazy (the branching g1r_add measured no faster, round 2)
// QUAD: 128 units of 4 lanes (8 waves, 2 per SIMD: the quad addition's ~250 VGPRs)
constexpr uint32_t kBitsum2Units(bool quad) { return quad ? 128 : 256; }
template <bool QUAD>
__global__ void __launch_bounds__(QUAD ? 512 : 256) k_bitsum2(const G1xyzz* __restrict__ in, uint32_t G,
                                                 uint32_t nbits, uint32_t nout,
                                                 G1xyzz* __restrict__ out,
                                                 const uint32_t* __restrict__ offsets, uint32_t B,
                                                 uint32_t* __restrict__ entries) {
  constexpr uint32_t UPW = QUAD ? 16 : 64;  // units per wave
  constexpr bool LZ = true;
  __shared__ G1xyzz sh[16];
  const uint32_t slot = blockIdx.y, tid = threadIdx.x, j = blockIdx.x;
  const TailUnit<QUAD> T(tid);
  if (j == 0 && tid == 0) entries[slot] = offsets[(size_t)slot * (B + 1) + B];
  in += (size_t)slot * G * kBitsumOut;
  // lazy additions (one wave per SIMD is all this narrow kernel runs); the stored totals are
  // finished to [0, 2p) for the host. A unit's first term is taken as is (adding it to
  // infinity would run the repair path).
  G1R acc = g1r_infinity();
  bool have = false;
  for (uint32_t g = T.u; g < G; g += kBitsum2Units(QUAD)) {
    const G1xyzz* e = &in[(size_t)g * kBitsumOut];
    // wide sets: j = nbits sums the plain sums, nbits + 1 the A_g
    uint32_t i0 = kBitsumOut, i1 = kBitsumOut;  // kBitsumOut: none
    if (j >= nbits) i0 = j == nbits ? 9 : 8;
    else if (j < 8) i0 = j, i1 = j == 0 ? 8 : kBitsumOut;
    else if ((g >> (j - 8)) & 1u) i0 = 8;
    for (uint32_t i : {i0, i1}) {
      if (i == kBitsumOut) continue;
      const G1R v = ld_g1r(&e[i]);
      if (have) acc = T.template add<LZ>(acc, v);
      else acc = v;
      have = true;
    }
  }
  // units >= G hold infinity: a shuffle tree over each wave's min(G, UPW) units, then the
  // wave totals (up to 4 / 8) through LDS
  uint32_t w0 = 1;
  while (w0 < min(G, UPW)) w0 <<= 1;
  acc = T.template tree<LZ>(acc, T.u % UPW, w0);
  const uint32_t gu = min(G, kBitsum2Units(QUAD)), nw = gu > UPW ? (gu + UPW - 1) / UPW : 1;  // waves holding values
  if (T.u % UPW == 0 && T.l == 0 && T.u / UPW < nw) st_g1r(&sh[T.u / UPW], acc);
  __syncthreads();
  if (T.u < UPW) {  // wave 0: unit e < nw/2 adds a pair of wave totals, then a tree
    const uint32_t e = T.u, np = (nw + 1) / 2;
    acc = g1r_infinity();
    if (e < np) {
      acc = ld_g1r(&sh[2 * e]);
      if (2 * e + 1 < nw) acc = T.template add<LZ>(acc, ld_g1r(&sh[2 * e + 1]));
    }
    uint32_t w = 1;
    while (w < np) w <<= 1;
    acc = T.template tree<LZ>(acc, e, w);
    if (e == 0 && T.l == 0) st_g1r(&out[(size_t)slot * nout + j], g1r_lazy_finish(acc));
  }
}

// the bit-sum kernels of one batch (k_bitsum2 folded into k_bitsum1 when fold.done is set)
template <bool QUAD, bool QUAD2>
void bitsum_launch(const MsmPlan& p, MsmWorkspace& w, const BitsumFold& fold, G1xyzz* bits_dev,
                   ReadbackHeader* hdr_dev, hipStream_t stream) {
  const uint32_t G = p.G, slots = p.slots;
  if (p.wide) {
    hipLaunchKernelGGL((k_bitsum1<true, QUAD>), dim3(G, slots, QUAD ? 2 : 1), dim3(bitsum1_threads(true, QUAD)), 0, stream, p.NR,
                       (const G1xyzz*)w.ys.as<G1xyzz>(), (const G1xyzz*)w.zs.as<G1xyzz>(),
                       w.bits1.as<G1xyzz>(), fold);
  } else {
    hipLaunchKernelGGL((k_bitsum1<false, QUAD>), dim3(G, slots), dim3(bitsum1_threads(false, QUAD)), 0, stream, p.B,
                       (const G1xyzz*)w.bsum.as<G1xyzz>(), (const G1xyzz*)nullptr,
                       w.bits1.as<G1xyzz>(), fold);
  }
  if (!fold.done) {
    hipLaunchKernelGGL(k_bitsum2<QUAD2>, dim3(p.nout, slots), dim3(kBitsum2Units(QUAD2) * TailUnit<QUAD2>::S), 0, stream, w.bits1.as<G1xyzz>(),
                       G, p.nbits, p.nout, bits_dev, (const uint32_t*)w.offsets.as<uint32_t>(), p.B,
                       hdr_dev->entries);
  }
}

}  // namespace

void msm_reduce(const MsmPlan& p, MsmWorkspace& w, hipStream_t stream) {
  const uint32_t B = p.B, slots = p.slots;
  ReadbackHeader* hdr_dev = static_cast<ReadbackHeader*>(w.out_dev);
  G1xyzz* bits_dev = reinterpret_cast<G1xyzz*>(hdr_dev + 1);
  // 0: single-lane trees, 1: quad trees, 2: quad k_bitsum2 only (its few workgroups are
  // latency-bound at any load); chosen when the workspace is made (msm_common.hpp)
  const int tail = p.tail_quad;
  const bool quad = tail == 1;
  if (p.wide) {
    hipLaunchKernelGGL(k_runsum1, dim3(cdiv(p.NR, 256), slots), dim3(256), 0, stream,
                       (const uint32_t*)w.task_off.as<uint32_t>(), B, p.rb, (uint64_t)w.task_stride,
                       (const G1xyzz*)w.partials.as<G1xyzz>(), w.rsum.as<G1xyzz>());
    hipLaunchKernelGGL(k_runsum2, dim3(cdiv(p.NR, 256), slots), dim3(256), 0, stream, B, p.rb,
                       (const G1xyzz*)w.rsum.as<G1xyzz>(), w.ys.as<G1xyzz>(), w.zs.as<G1xyzz>());
  } else if (quad) {  // 2^lp lanes per bucket (msm_plan)
    hipLaunchKernelGGL(k_bucket_sum<true>, dim3(cdiv(((size_t)B << p.lp) * 4, 256), slots), dim3(256), 0, stream,
                       w.task_off.as<uint32_t>(), B, p.lp, (uint64_t)w.task_stride,
                       w.partials.as<G1xyzz>(), w.bsum.as<G1xyzz>());
  } else {
    hipLaunchKernelGGL(k_bucket_sum<false>, dim3(cdiv((size_t)B << p.lp, 256), slots), dim3(256), 0, stream,
                       w.task_off.as<uint32_t>(), B, p.lp, (uint64_t)w.task_stride,
                       w.partials.as<G1xyzz>(), w.bsum.as<G1xyzz>());
  }
  BitsumFold fold{};  // k_bitsum2 folded into k_bitsum1 when the slots have few groups
  if (p.fold) {
    fold.done = w.done.as<uint32_t>();
    fold.out2 = bits_dev;
    fold.offsets = w.offsets.as<uint32_t>();
    fold.entries = hdr_dev->entries;
    fold.B = B;
    fold.nbits = p.nbits;
    fold.nout = p.nout;
  }
  if (quad) bitsum_launch<true, true>(p, w, fold, bits_dev, hdr_dev, stream);
  else if (tail == 2) bitsum_launch<false, true>(p, w, fold, bits_dev, hdr_dev, stream);
  else bitsum_launch<false, false>(p, w, fold, bits_dev, hdr_dev, stream);
}

}  // namespace plk
