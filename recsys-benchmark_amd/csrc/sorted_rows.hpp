// sorted_rows.hpp — the sorted-segment walker of the row-sparse optimizer steps (optim.hip: Adam and the coalesce store;
// adagrad.hip: Adagrad and row-wise Adagrad), parametrised by a row rule.
//
// Input: the row ids of a row-form gradient sorted ascending (rows), the permutation that sorted them (perm: sorted
// position -> original entry) and the values vals[n, D] in original order.  Every run of equal ids is one table row; the
// walker sums the run's gradient rows in a FIXED order (no atomics: equal bits on every run) and hands the TOTAL to the
// rule exactly once per row.  Ids outside [0, N) are skipped.
//
// A rule is a struct passed by value to the kernels:
//     void begin();                                              once per thread, before the walk (device-side scalars)
//     template <int D> void row(row, q, const Vec<VW> &G) const; the LPR kernels: lane q of the row's LPR lanes holds
//                                                                G[q*VW .. q*VW+VW); ALL LPR lanes of the group are
//                                                                active and convergent at the call (see below)
//     void row_any(int64_t row, int D, int lane, Sum sum) const; the any-D kernel: the whole wave is at the call,
//                                                                sum(d) returns G[d] (d < D) for the calling lane
// The rule never sees a partial sum: a run that spans passes leaves its per-pass pieces in acc through the walker's own
// stores, the join kernel adds them, and only that total reaches row().  There is no other call site of row(), and the
// rule has no access to acc — which is what lets a rule that squares G (Adagrad) share the walker.
//
// Where a rule may reduce over a row (row-wise Adagrad's sum of squares): in k_rows_pass the LPR lanes of one position
// share r and therefore every branch up to the call; in k_rows_join the call sits under `r == 0`, i.e. lanes 0..LPR-1,
// one whole group.  An xor tree over masks 1..LPR/2 therefore reads active lanes only.  In k_rows_any the lanes stride d
// and would leave a `d < D` loop at different trips, so row_any() is called wave-uniformly and the rule loops itself.
#pragma once
#include "common.hpp"

namespace mi {

struct SortedRows {
  const int64_t *rows;   // sorted
  const int64_t *perm;   // sorted position -> original entry
  const float *vals;     // [n, D] original order
  float *acc;            // [n, D] scratch: per-pass pieces of the segments longer than one pass
  int64_t n, N;
};

// VW consecutive floats of a row held by one lane: float4 (VW = 4) or a scalar (VW = 1: the [N,1] first-order table)
template <int VW> struct Vec;
template <> struct Vec<4> {
  float4 v;
  static __device__ __forceinline__ Vec load(const float *p) { return {ld4(p)}; }
  __device__ __forceinline__ void store(float *p) const { st4(p, v); }
  __device__ __forceinline__ void add(const Vec &o) { v.x += o.v.x; v.y += o.v.y; v.z += o.v.z; v.w += o.v.w; }
  __device__ __forceinline__ Vec down(int d) const {
    return {float4{__shfl_down(v.x, d), __shfl_down(v.y, d), __shfl_down(v.z, d), __shfl_down(v.w, d)}};
  }
  __device__ __forceinline__ Vec across(int m) const {
    return {float4{__shfl_xor(v.x, m), __shfl_xor(v.y, m), __shfl_xor(v.z, m), __shfl_xor(v.w, m)}};
  }
  static __device__ __forceinline__ Vec zero() { return {float4{0.f, 0.f, 0.f, 0.f}}; }
};
template <> struct Vec<1> {
  float v;
  static __device__ __forceinline__ Vec load(const float *p) { return {*p}; }
  __device__ __forceinline__ void store(float *p) const { *p = v; }
  __device__ __forceinline__ void add(const Vec &o) { v += o.v; }
  __device__ __forceinline__ Vec down(int d) const { return {__shfl_down(v, d)}; }
  __device__ __forceinline__ Vec across(int m) const { return {__shfl_xor(v, m)}; }
  static __device__ __forceinline__ Vec zero() { return {0.f}; }
};

// A pass = RS consecutive sorted positions, LPR lanes (VW floats each, D = LPR*VW) per position.  Every position loads
// its gradient row (no serial walk over duplicates); a segmented suffix sum over the pass (log2 RS shuffle steps: the
// keys are sorted, so "position i+s has my row" means everything between has it too) leaves each segment's in-pass
// total with its first position in the pass.  A segment that lies inside one pass is applied at once; one that spans
// passes leaves a piece per pass in acc[that first position] (plain stores: every slot has one writer) and
// k_rows_join adds the pieces in a fixed order — no atomics, so the step is deterministic.
template <int LPR, int VW, class Rule>
__global__ __launch_bounds__(kBlock) void k_rows_pass(SortedRows a, Rule rule) {
  rule.begin();
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * VW;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const int64_t ntiles = (a.n + RS - 1) / RS;
  for (int64_t t = wave0; t < ntiles; t += nwaves) {
    const int64_t i = t * RS + r;
    const bool live = i < a.n;
    const int64_t row = live ? a.rows[i] : (int64_t)-1 - r;          // dead positions: keys nobody shares
    Vec<VW> g = live ? Vec<VW>::load(a.vals + a.perm[i] * D + q * VW) : Vec<VW>::zero();
#pragma unroll
    for (int s = 1; s < RS; s <<= 1) {
      const int64_t nrow = __shfl_down(row, s * LPR);
      const Vec<VW> ng = g.down(s * LPR);
      if (r + s < RS && nrow == row) g.add(ng);
    }
    if (!live || (uint64_t)row >= (uint64_t)a.N) continue;
    const bool before = i > 0 && a.rows[i - 1] == row;
    if (r > 0 && before) continue;                                   // not the first of its segment in this pass
    const int64_t pe = t * RS + RS;                                  // first position after the pass
    const bool after = pe < a.n && a.rows[pe] == row;
    if (!before && !after) rule.template row<D>(row, q, g);
    else g.store(a.acc + i * D + q * VW);
  }
}

// second kernel of the pair: the wave that holds the first position of a segment running past its pass gathers the
// pieces — acc[first position], then acc[start of each following pass] while that pass still begins with the row —
// its RS lane groups striding over them, joined by a fixed shuffle tree.
template <int LPR, int VW, class Rule>
__global__ __launch_bounds__(kBlock) void k_rows_join(SortedRows a, Rule rule) {
  rule.begin();
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * VW;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const int64_t ntiles = (a.n + RS - 1) / RS;
  for (int64_t t = wave0; t < ntiles; t += nwaves) {
    const int64_t i = t * RS + r, pe = t * RS + RS;
    if (pe >= a.n) break;                                            // the last pass has nothing after it (wave-uniform)
    const int64_t row = a.rows[i];
    const bool head = (uint64_t)row < (uint64_t)a.N && a.rows[pe] == row && !(i > 0 && a.rows[i - 1] == row);
    uint64_t todo = __ballot(head && q == 0);
    while (todo) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const int64_t hrow = __shfl(row, src), hi = __shfl(i, src);
      Vec<VW> sum = Vec<VW>::zero();
      for (int64_t k = r;; k += RS) {
        const int64_t pos = k == 0 ? hi : pe + (k - 1) * RS;
        if (pos >= a.n || a.rows[pos] != hrow) break;
        sum.add(Vec<VW>::load(a.acc + pos * D + q * VW));
      }
#pragma unroll
      for (int m = LPR; m < kWave; m <<= 1) sum.add(sum.across(m));
      if (r == 0) rule.template row<D>(hrow, q, sum);
    }
  }
}

// any D: one wave per sorted position, lanes stride the row; the first position of a row walks its duplicates
template <class Rule>
__global__ __launch_bounds__(kBlock) void k_rows_any(SortedRows a, Rule rule, int D) {
  rule.begin();
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t i = wave0; i < a.n; i += nwaves) {
    const int64_t row = a.rows[i];
    if ((uint64_t)row >= (uint64_t)a.N) continue;
    if (i > 0 && a.rows[i - 1] == row) continue;
    rule.row_any(row, D, lane, [&](int d) {
      float g = a.vals[a.perm[i] * D + d];
      for (int64_t j = i + 1; j < a.n && a.rows[j] == row; ++j) g += a.vals[a.perm[j] * D + d];
      return g;
    });
  }
}

// The width dispatch of every sorted-row step: D = 1 and D = 2 the scalar forms, D/4 a power of two up to 64 the float4
// forms when `aligned` (every pointer the kernels touch with float4 accesses is 16-byte aligned), else the any-D kernel.
template <class Rule>
inline int launch_sorted_rows(const char *name, const char *name_join, SortedRows a, Rule rule, int32_t D, bool aligned,
                              void *stream) {
  const int64_t n = a.n;
#define MI_ROWS_CALL(LPR, VW)                                                                     \
  do {                                                                                            \
    const int grid = grid_for_waves((n + (kWave / LPR) - 1) / (kWave / LPR));                     \
    MI_LAUNCH(name, (k_rows_pass<LPR, VW, Rule>), grid, kBlock, stream, a, rule);                 \
    MI_LAUNCH(name_join, (k_rows_join<LPR, VW, Rule>), grid, kBlock, stream, a, rule);            \
  } while (0)
  if (D == 1) {
    MI_ROWS_CALL(1, 1);
  } else if (D == 2) {
    MI_ROWS_CALL(2, 1);
  } else if (vec_ok(D) && aligned && aligned16(a.vals) && aligned16(a.acc)) {
#define MI_ROWS_CALL4(LPR) MI_ROWS_CALL(LPR, 4)
    MI_DISPATCH_LPR(D / 4, MI_ROWS_CALL4)
#undef MI_ROWS_CALL4
  } else {
    MI_LAUNCH(name, (k_rows_any<Rule>), grid_for_waves(n), kBlock, stream, a, rule, D);
  }
#undef MI_ROWS_CALL
  return launch_status();
}

}  // namespace mi
