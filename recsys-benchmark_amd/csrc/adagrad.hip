// adagrad.hip — Adagrad and exact row-wise Adagrad on row-form (COO, possibly uncoalesced) gradients, and dense Adagrad
// over a list of tensors.  The sparse steps are two rules on the sorted-segment walker of sorted_rows.hpp (the one the
// Adam step runs on): the walker sums every duplicate of a row first, in a fixed order, and hands the rule the total G —
// so both are the EXACT forms, (sum g_i)^2, not the sum of g_i^2 an atomic scatter would give.
//
//   Adagrad (torch.optim.Adagrad on a sparse gradient: coalesce, touched rows only; clr = lr / (1 + (t-1) lr_decay)):
//       s = state_sum[row,d] + G_d*G_d;  state_sum[row,d] = s;  W[row,d] -= clr * (G_d / (sqrtf(s) + eps))
//   row-wise Adagrad (one fp32 accumulator per table row):
//       s = row_sum[row] + (sum_d G_d^2) / D;  row_sum[row] = s;  W[row,d] -= clr * (G_d / (sqrtf(s) + eps))
//   sum_d in a fixed order: a lane adds the squares of its own VW elements in index order, then the LPR lanes of the row
//   are joined by an xor tree (masks 1, 2, .. LPR/2); the any-D kernel: a lane adds d = lane, lane+64, .. in that order,
//   then the 64 lanes are joined by an xor tree (masks 32 .. 1).
#include "common.hpp"
#include "sorted_rows.hpp"

namespace {
using namespace mi;

__device__ __forceinline__ float adagrad_step(float clr, float eps, float g, float s) { return clr * (g / (sqrtf(s) + eps)); }

struct AdagradRule {
  float *W, *S;          // W [N, ldw-strided rows]; S = state_sum [N, D] contiguous
  int64_t ldw;
  float clr, eps;

  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ float one(float g, float &s) const {
    s += g * g;
    return adagrad_step(clr, eps, g, s);
  }
  template <int D>
  __device__ __forceinline__ void row(int64_t row, int q, const Vec<4> &g) const {
    const int64_t o = row * D + q * 4, ow = row * ldw + q * 4;
    float4 s = ld4(S + o), w = ld4(W + ow);
    w.x -= one(g.v.x, s.x);
    w.y -= one(g.v.y, s.y);
    w.z -= one(g.v.z, s.z);
    w.w -= one(g.v.w, s.w);
    st4(S + o, s);
    st4(W + ow, w);
  }
  template <int D>
  __device__ __forceinline__ void row(int64_t row, int q, const Vec<1> &g) const {
    const int64_t o = row * D + q;
    float s = S[o];
    W[row * ldw + q] -= one(g.v, s);
    S[o] = s;
  }
  template <class Sum>
  __device__ __forceinline__ void row_any(int64_t row, int D, int lane, Sum sum) const {
    for (int d = lane; d < D; d += kWave) {
      const float g = sum(d);
      const int64_t o = row * D + d;
      float s = S[o];
      W[row * ldw + d] -= one(g, s);
      S[o] = s;
    }
  }
};

struct RowwiseRule {
  float *W, *R;          // R = row_sum [N]
  int64_t ldw;
  float clr, eps;

  __device__ __forceinline__ void begin() {}
  // the LPR lanes of a row are all here (sorted_rows.hpp): the xor tree stays inside the group
  template <int LPR>
  __device__ __forceinline__ float finish(int64_t row, int q, float ss, float inv_d) const {
#pragma unroll
    for (int m = 1; m < LPR; m <<= 1) ss += __shfl_xor(ss, m);
    const float s = R[row] + ss * inv_d;
    if (q == 0) R[row] = s;                      // (every lane of the group loaded R[row] before this store: one wave)
    return s;
  }
  template <int D>
  __device__ __forceinline__ void row(int64_t row, int q, const Vec<4> &g) const {
    float ss = g.v.x * g.v.x;
    ss += g.v.y * g.v.y;
    ss += g.v.z * g.v.z;
    ss += g.v.w * g.v.w;
    const float s = finish<D / 4>(row, q, ss, 1.f / D);
    const int64_t ow = row * ldw + q * 4;
    float4 w = ld4(W + ow);
    w.x -= adagrad_step(clr, eps, g.v.x, s);
    w.y -= adagrad_step(clr, eps, g.v.y, s);
    w.z -= adagrad_step(clr, eps, g.v.z, s);
    w.w -= adagrad_step(clr, eps, g.v.w, s);
    st4(W + ow, w);
  }
  template <int D>
  __device__ __forceinline__ void row(int64_t row, int q, const Vec<1> &g) const {
    const float s = finish<D>(row, q, g.v * g.v, 1.f / D);
    W[row * ldw + q] -= adagrad_step(clr, eps, g.v, s);
  }
  // the lanes stride d and D % 64 may be anything: the squares are gathered in a loop whose trip count is the same for
  // every lane, joined across the wave, and only then is the row updated in a second walk over d
  template <class Sum>
  __device__ __forceinline__ void row_any(int64_t row, int D, int lane, Sum sum) const {
    float ss = 0.f;
    for (int d0 = 0; d0 < D; d0 += kWave) {
      const int d = d0 + lane;
      const float g = d < D ? sum(d) : 0.f;
      ss += g * g;
    }
    ss = wave_sum(ss);
    const float s = R[row] + ss / (float)D;
    for (int d = lane; d < D; d += kWave) W[row * ldw + d] -= adagrad_step(clr, eps, sum(d), s);
    if (lane == 0) R[row] = s;
  }
};

// ---- dense Adagrad over a list of tensors (torch.optim.Adagrad, L2 weight decay, lr_decay = 0) ---------------------------
// k_adam_dense's layout: one launch updates up to kAdagradTensors tensors, workgroup c owns one 4096-element chunk of one
// tensor (chunk counts are prefix-summed in the table), every thread four float4 groups with all loads issued before the
// arithmetic — 5 streams (p, g, s in; p, s out).  No step count enters the rule, so there is no counter and no ticket.
constexpr int kAdagradTensors = 24;
constexpr int kAdagradChunk = kBlock * 16;
struct AdagradDenseTable {
  float *p[kAdagradTensors];
  const float *g[kAdagradTensors];
  float *s[kAdagradTensors];
  int64_t numel[kAdagradTensors];
  int64_t chunk_end[kAdagradTensors];   // prefix sum of ceil(numel / kAdagradChunk)
  int32_t count;
  uint32_t vec_ok;                      // bit k: all three pointers of tensor k are 16-byte aligned
};

__device__ __forceinline__ void adagrad_dense1(float &p, float g, float &s, float lr, float eps, float wd) {
  g += wd * p;
  s += g * g;
  p -= lr * (g / (sqrtf(s) + eps));
}

__global__ __launch_bounds__(kBlock) void k_adagrad_dense(AdagradDenseTable t, float lr, float eps, float wd) {
  int k = 0;
  while (k + 1 < t.count && (int64_t)blockIdx.x >= t.chunk_end[k]) ++k;
  const int64_t chunk = (int64_t)blockIdx.x - (k ? t.chunk_end[k - 1] : 0);
  float *P = t.p[k], *S = t.s[k];
  const float *G = t.g[k];
  const int64_t n = t.numel[k], base = chunk * kAdagradChunk;
  if (((t.vec_ok >> k) & 1u) && base + kAdagradChunk <= n) {
    float4 p[4], g[4], s[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t e = base + (int64_t)(u * kBlock + threadIdx.x) * 4;
      p[u] = ld4(P + e); g[u] = ld4(G + e); s[u] = ld4(S + e);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      adagrad_dense1(p[u].x, g[u].x, s[u].x, lr, eps, wd);
      adagrad_dense1(p[u].y, g[u].y, s[u].y, lr, eps, wd);
      adagrad_dense1(p[u].z, g[u].z, s[u].z, lr, eps, wd);
      adagrad_dense1(p[u].w, g[u].w, s[u].w, lr, eps, wd);
      const int64_t e = base + (int64_t)(u * kBlock + threadIdx.x) * 4;
      st4(P + e, p[u]); st4(S + e, s[u]);
    }
  } else {                                         // a tensor's last chunk, or unaligned views
    for (int64_t e = base + threadIdx.x; e < n && e < base + kAdagradChunk; e += kBlock) {
      float p = P[e], s = S[e];
      adagrad_dense1(p, G[e], s, lr, eps, wd);
      P[e] = p; S[e] = s;
    }
  }
}

}  // namespace

extern "C" {

int mi_sparse_adagrad_sorted_ld(const int64_t *rows_sorted, const int64_t *perm, const float *vals, float *W, int64_t ldw,
                                float *state_sum, float *acc, int64_t n, int32_t D, int64_t N, float clr, float eps,
                                void *stream) {
  if (n < 0 || D <= 0 || N < 0 || ldw < D) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!rows_sorted || !perm || !vals || !W || !state_sum || !acc) return MI_ERR_INVALID_ARG;
  if (vec_ok(D) && (ldw & 3) != 0) return MI_ERR_UNSUPPORTED;   // float4 row accesses need 16-byte aligned rows
  const SortedRows a{rows_sorted, perm, vals, acc, n, N};
  const AdagradRule rule{W, state_sum, ldw, clr, eps};
  return launch_sorted_rows("sparse_adagrad", "sparse_adagrad_long", a, rule, D, all_aligned16(W, state_sum), stream);
}

int mi_rowwise_adagrad_sorted_ld(const int64_t *rows_sorted, const int64_t *perm, const float *vals, float *W, int64_t ldw,
                                 float *row_sum, float *acc, int64_t n, int32_t D, int64_t N, float clr, float eps,
                                 void *stream) {
  if (n < 0 || D <= 0 || N < 0 || ldw < D) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!rows_sorted || !perm || !vals || !W || !row_sum || !acc) return MI_ERR_INVALID_ARG;
  if (vec_ok(D) && (ldw & 3) != 0) return MI_ERR_UNSUPPORTED;
  const SortedRows a{rows_sorted, perm, vals, acc, n, N};
  const RowwiseRule rule{W, row_sum, ldw, clr, eps};
  return launch_sorted_rows("rowwise_adagrad", "rowwise_adagrad_long", a, rule, D, aligned16(W), stream);
}

int mi_adagrad_dense_multi(float *const *params, const float *const *grads, float *const *state_sums, const int64_t *numels,
                           int32_t count, float lr, float eps, float weight_decay, void *stream) {
  if (count < 0) return MI_ERR_INVALID_ARG;
  if (count == 0) return MI_OK;
  if (!params || !grads || !state_sums || !numels) return MI_ERR_INVALID_ARG;
  // zero-element entries are skipped, so a launch may consume more than kAdagradTensors entries: the next one starts at
  // the entry where this one stopped
  for (int32_t i = 0; i < count;) {
    AdagradDenseTable t{};
    int64_t chunks = 0;
    for (; i < count && t.count < kAdagradTensors; ++i) {
      if (numels[i] < 0) return MI_ERR_INVALID_ARG;
      if (numels[i] == 0) continue;
      if (!params[i] || !grads[i] || !state_sums[i]) return MI_ERR_INVALID_ARG;
      const int k = t.count++;
      t.p[k] = params[i]; t.g[k] = grads[i]; t.s[k] = state_sums[i];
      t.numel[k] = numels[i];
      chunks += (numels[i] + kAdagradChunk - 1) / kAdagradChunk;
      t.chunk_end[k] = chunks;
      if (all_aligned16(params[i], grads[i], state_sums[i])) t.vec_ok |= 1u << k;
    }
    if (t.count == 0) continue;
    if (chunks > 0x7fffffff) return MI_ERR_UNSUPPORTED;
    MI_LAUNCH("adagrad_dense", k_adagrad_dense, (int)chunks, kBlock, stream, t, lr, eps, weight_decay);
  }
  return launch_status();
}

}  // extern "C"
