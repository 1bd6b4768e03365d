// optim.hip — fused row-sparse optimizer steps on row-form (COO, possibly uncoalesced) gradients.
// SURVEY.md §8f rank 1; reference: get_optimizers' sparse branch (src/models/deepfm.py:163-184:
// torch.optim.SparseAdam on model.embedding.parameters(), no weight decay), and the SGD branch.
//
// torch.optim.SparseAdam semantics (torch/optim/sparse_adam.py, _single_tensor_sparse_adam):
// coalesce the gradient (duplicates SUMMED), then for the touched rows only
//     m += (1-b1)(g - m);  v += (1-b2)(g*g - v);  p -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
// Here the caller sorts the row ids once (torch.sort: no host sync, no dynamic shape); every
// sorted position whose predecessor holds a different row is a segment head: it sums the
// gradient rows of its segment and applies the update — one pass, traffic ~ B*F rows, not N.
#include "common.hpp"
#include "sorted_rows.hpp"

namespace {
using namespace mi;

// torch.optim.SparseAdam on one coalesced row (sorted_rows.hpp: the walker hands over the run's total, once per row)
struct AdamRule {
  float *W, *M, *V;      // [N, D]; M, V contiguous
  int64_t ldw;           // floats between consecutive rows of W (D, or the row stride of a packed table)
  float step_size, omb1, omb2, eps;   // omb = 1 - beta, formed in double by the host (1.f - 0.999f is off by 1.3e-5)
  const float *step_size_dev;   // when given: the step size lives on the device (mi_adam_tick), hipGraph replays

  __device__ __forceinline__ void begin() {
    if (step_size_dev) step_size = step_size_dev[0];
  }
  __device__ __forceinline__ float one(float g, float &m, float &v) const {
    m += omb1 * (g - m);
    v += omb2 * (g * g - v);
    return step_size * (m / (sqrtf(v) + eps));
  }
  template <int D>
  __device__ __forceinline__ void row(int64_t row, int q, const Vec<4> &g) const {
    const int64_t o = row * D + q * 4, ow = row * ldw + q * 4;
    float4 m = ld4(M + o), v = ld4(V + o), w = ld4(W + ow);
    w.x -= one(g.v.x, m.x, v.x);
    w.y -= one(g.v.y, m.y, v.y);
    w.z -= one(g.v.z, m.z, v.z);
    w.w -= one(g.v.w, m.w, v.w);
    st4(M + o, m);
    st4(V + o, v);
    st4(W + ow, w);
  }
  template <int D>
  __device__ __forceinline__ void row(int64_t row, int q, const Vec<1> &g) const {
    const int64_t o = row * D + q;
    float m = M[o], v = V[o];
    W[row * ldw + q] -= one(g.v, m, v);
    M[o] = m;
    V[o] = v;
  }
  template <class Sum>
  __device__ __forceinline__ void row_any(int64_t row, int D_, int lane, Sum sum) const {
    for (int d = lane; d < D_; d += kWave) {
      const float g = sum(d);
      const int64_t o = row * D_ + d;
      float m = M[o], v = V[o];
      W[row * ldw + d] -= one(g, m, v);
      M[o] = m;
      V[o] = v;
    }
  }
};

// the coalesce store: no update — the coalesced gradient row is STORED to G[row] (mi_coalesce_rows_sorted)
struct CoalesceRule {
  float *G;              // [N, D]
  __device__ __forceinline__ void begin() {}
  template <int D>
  __device__ __forceinline__ void row(int64_t row, int q, const Vec<4> &g) const { st4(G + row * D + q * 4, g.v); }
  template <int D>
  __device__ __forceinline__ void row(int64_t row, int q, const Vec<1> &g) const { G[row * D + q] = g.v; }
  template <class Sum>
  __device__ __forceinline__ void row_any(int64_t row, int D_, int lane, Sum sum) const {
    for (int d = lane; d < D_; d += kWave) G[row * D_ + d] = sum(d);
  }
};

// t += 1; step_size = lr * sqrt(1 - b2^t) / (1 - b1^t) in double, like the host computes it in the eager path
constexpr int kTickSlots = 8;
struct TickTable {
  float *step[kTickSlots];
  float *step_size[kTickSlots];
  int count;
};
__global__ void k_adam_tick(TickTable tt, double lr, double beta1, double beta2) {
  const int i = threadIdx.x;
  if (i >= tt.count) return;
  const double t = (double)tt.step[i][0] + 1.0;
  tt.step[i][0] = (float)t;
  tt.step_size[i][0] = (float)(lr * sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t)));
}

// ---- dense Adam over a list of tensors (torch.optim.Adam, L2 weight decay) --------------------------------------
// One launch updates up to kAdamTensors tensors: workgroup c owns one 4096-element chunk of one tensor (chunk counts are
// prefix-summed in the table), every thread four float4 groups with all loads issued before the arithmetic — 7 streams
// (p, g, m, v in; p, m, v out), HBM-bound for the big tables and one launch instead of a 40 us multi_tensor_apply for the
// MLP's 0.5 M parameters.  The step count is a device float per tensor (torch's capturable layout): this kernel reads
// t = step + 1, k_adam_steps_inc advances the counters afterwards.
constexpr int kAdamTensors = 24;
constexpr int kAdamChunk = kBlock * 16;
struct AdamDenseTable {
  float *p[kAdamTensors];
  const float *g[kAdamTensors];
  float *m[kAdamTensors];
  float *v[kAdamTensors];
  float *step[kAdamTensors];
  int64_t numel[kAdamTensors];
  int64_t chunk_end[kAdamTensors];   // prefix sum of ceil(numel / kAdamChunk)
  int32_t count;
  uint32_t vec_ok;                   // bit k: all four pointers of tensor k are 16-byte aligned
  unsigned *ticket;                  // when given: the last workgroup to finish advances the step counts (no second launch)
};

__device__ __forceinline__ void adam_dense1(float &p, float g, float &m, float &v, float omb1, float b2, float omb2, float wd,
                                            float step_size, float inv_bc2s, float eps) {
  g += wd * p;
  m += omb1 * (g - m);                             // m.lerp_(g, 1 - b1)
  v = b2 * v + omb2 * g * g;
  p -= step_size * (m / (sqrtf(v) * inv_bc2s + eps));
}

__global__ __launch_bounds__(kBlock) void k_adam_dense(AdamDenseTable t, float lr, double beta1, double beta2, float eps,
                                                       float wd) {
  __shared__ float s_step_size, s_inv_bc2s;
  int k = 0;
  while (k + 1 < t.count && (int64_t)blockIdx.x >= t.chunk_end[k]) ++k;
  const int64_t chunk = (int64_t)blockIdx.x - (k ? t.chunk_end[k - 1] : 0);
  if (threadIdx.x == 0) {
    const double tt = (double)t.step[k][0] + 1.0;
    s_step_size = (float)((double)lr / (1.0 - pow(beta1, tt)));
    s_inv_bc2s = (float)(1.0 / sqrt(1.0 - pow(beta2, tt)));
  }
  __syncthreads();
  const float step_size = s_step_size, inv_bc2s = s_inv_bc2s;
  const float omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
  float *P = t.p[k], *M = t.m[k], *V = t.v[k];
  const float *G = t.g[k];
  const int64_t n = t.numel[k], base = chunk * kAdamChunk;
  if (((t.vec_ok >> k) & 1u) && base + kAdamChunk <= n) {
    float4 p[4], g[4], m[4], v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t e = base + (int64_t)(u * kBlock + threadIdx.x) * 4;
      p[u] = ld4(P + e); g[u] = ld4(G + e); m[u] = ld4(M + e); v[u] = ld4(V + e);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      adam_dense1(p[u].x, g[u].x, m[u].x, v[u].x, omb1, b2, omb2, wd, step_size, inv_bc2s, eps);
      adam_dense1(p[u].y, g[u].y, m[u].y, v[u].y, omb1, b2, omb2, wd, step_size, inv_bc2s, eps);
      adam_dense1(p[u].z, g[u].z, m[u].z, v[u].z, omb1, b2, omb2, wd, step_size, inv_bc2s, eps);
      adam_dense1(p[u].w, g[u].w, m[u].w, v[u].w, omb1, b2, omb2, wd, step_size, inv_bc2s, eps);
      const int64_t e = base + (int64_t)(u * kBlock + threadIdx.x) * 4;
      st4(P + e, p[u]); st4(M + e, m[u]); st4(V + e, v[u]);
    }
  } else {                                         // a tensor's last chunk, or unaligned views
    for (int64_t e = base + threadIdx.x; e < n && e < base + kAdamChunk; e += kBlock) {
      float p = P[e], m = M[e], v = V[e];
      adam_dense1(p, G[e], m, v, omb1, b2, omb2, wd, step_size, inv_bc2s, eps);
      P[e] = p; M[e] = m; V[e] = v;
    }
  }
  if (t.ticket) {
    // every workgroup read its tensor's step count before doing anything else, so once all of them have finished the
    // counts may advance: the last one to take a ticket does it (and re-arms the ticket for the next launch)
    __syncthreads();
    if (threadIdx.x == 0 &&
        __hip_atomic_fetch_add(t.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
      for (int i = 0; i < t.count; ++i) t.step[i][0] += 1.f;
      __hip_atomic_store(t.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void k_adam_steps_inc(AdamDenseTable t) {
  if ((int)threadIdx.x < t.count) t.step[threadIdx.x][0] += 1.f;
}

// W[idx[i], :] += alpha * g[i, :]   (row-sparse SGD: linear, so duplicates need no coalescing)
__global__ __launch_bounds__(kBlock) void k_scatter_axpy(const int64_t *__restrict__ idx, const float *__restrict__ g,
                                                         float alpha, float *__restrict__ W, int64_t n, int D,
                                                         int64_t N) {
  const int64_t total = n * D;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx[e / D];
    if ((uint64_t)row < (uint64_t)N) atomicAdd(W + row * D + e % D, alpha * g[e]);
  }
}

}  // namespace

extern "C" {

int mi_sparse_adam_sorted_ld(const int64_t *rows_sorted, const int64_t *perm, const float *vals, float *W, int64_t ldw,
                             float *exp_avg, float *exp_avg_sq, float *acc, int64_t n, int32_t D, int64_t N,
                             float step_size, const float *step_size_dev, double beta1, double beta2, float eps,
                             void *stream) {
  if (n < 0 || D <= 0 || N < 0 || ldw < D) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!rows_sorted || !perm || !vals || !W || !exp_avg || !exp_avg_sq || !acc) return MI_ERR_INVALID_ARG;
  if (vec_ok(D) && (ldw & 3) != 0) return MI_ERR_UNSUPPORTED;   // float4 row accesses need 16-byte aligned rows
  const SortedRows a{rows_sorted, perm, vals, acc, n, N};
  const AdamRule rule{W, exp_avg, exp_avg_sq, ldw, step_size, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, step_size_dev};
  return launch_sorted_rows("sparse_adam", "sparse_adam_long", a, rule, D, all_aligned16(W, exp_avg, exp_avg_sq), stream);
}

int mi_sparse_adam_sorted(const int64_t *rows_sorted, const int64_t *perm, const float *vals, float *W,
                          float *exp_avg, float *exp_avg_sq, float *acc, int64_t n, int32_t D, int64_t N,
                          float step_size, const float *step_size_dev, double beta1, double beta2, float eps,
                          void *stream) {
  return mi_sparse_adam_sorted_ld(rows_sorted, perm, vals, W, D, exp_avg, exp_avg_sq, acc, n, D, N, step_size, step_size_dev,
                                  beta1, beta2, eps, stream);
}

// The same segmented sums, stored instead of applied: G[row, :] = sum of vals[perm[i], :] over the sorted positions i with
// rows_sorted[i] == row, added in a FIXED order (no atomics) — a bit-reproducible dense gradient out of row-form values.
// Rows that do not occur are not written: the caller zero-fills G.
int mi_coalesce_rows_sorted(const int64_t *rows_sorted, const int64_t *perm, const float *vals, float *G, float *acc,
                            int64_t n, int32_t D, int64_t N, void *stream) {
  if (n < 0 || D <= 0 || N < 0) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!rows_sorted || !perm || !vals || !G || !acc) return MI_ERR_INVALID_ARG;
  const SortedRows a{rows_sorted, perm, vals, acc, n, N};
  return launch_sorted_rows("sparse_adam", "sparse_adam_long", a, CoalesceRule{G}, D, aligned16(G), stream);
}

int mi_adam_tick(float *step, float *step_size, double lr, double beta1, double beta2, void *stream) {
  if (!step || !step_size) return MI_ERR_INVALID_ARG;
  TickTable tt{};
  tt.step[0] = step; tt.step_size[0] = step_size; tt.count = 1;
  MI_LAUNCH("adam_tick", k_adam_tick, 1, kWave, stream, tt, lr, beta1, beta2);
  return launch_status();
}

int mi_adam_tick_multi(float *const *steps, float *const *step_sizes, int32_t count, double lr, double beta1, double beta2,
                       void *stream) {
  if (count < 0 || (count > 0 && (!steps || !step_sizes))) return MI_ERR_INVALID_ARG;
  for (int32_t first = 0; first < count; first += kTickSlots) {
    TickTable tt{};
    for (int32_t i = first; i < count && tt.count < kTickSlots; ++i) {
      if (!steps[i] || !step_sizes[i]) return MI_ERR_INVALID_ARG;
      tt.step[tt.count] = steps[i];
      tt.step_size[tt.count++] = step_sizes[i];
    }
    MI_LAUNCH("adam_tick", k_adam_tick, 1, kWave, stream, tt, lr, beta1, beta2);
  }
  return launch_status();
}

int mi_adam_dense_multi(float *const *params, const float *const *grads, float *const *exp_avgs,
                        float *const *exp_avg_sqs, float *const *steps, const int64_t *numels, int32_t count, float lr,
                        double beta1, double beta2, float eps, float weight_decay, uint32_t *tickets, void *stream) {
  if (count < 0) return MI_ERR_INVALID_ARG;
  if (count == 0) return MI_OK;
  if (!params || !grads || !exp_avgs || !exp_avg_sqs || !steps || !numels) return MI_ERR_INVALID_ARG;
  int launch = 0;
  // zero-element entries are skipped (nothing to update, their step counts stay), so a launch may consume more than
  // kAdamTensors entries: the next one starts at the entry where this one stopped
  for (int32_t i = 0; i < count;) {
    AdamDenseTable t{};
    int64_t chunks = 0;
    for (; i < count && t.count < kAdamTensors; ++i) {
      if (numels[i] < 0) return MI_ERR_INVALID_ARG;
      if (numels[i] == 0) continue;
      if (!params[i] || !grads[i] || !exp_avgs[i] || !exp_avg_sqs[i] || !steps[i]) return MI_ERR_INVALID_ARG;
      const int k = t.count++;
      t.p[k] = params[i]; t.g[k] = grads[i]; t.m[k] = exp_avgs[i]; t.v[k] = exp_avg_sqs[i]; t.step[k] = steps[i];
      t.numel[k] = numels[i];
      chunks += (numels[i] + kAdamChunk - 1) / kAdamChunk;
      t.chunk_end[k] = chunks;
      if (aligned16(params[i]) && aligned16(grads[i]) && aligned16(exp_avgs[i]) && aligned16(exp_avg_sqs[i]))
        t.vec_ok |= 1u << k;
    }
    if (t.count == 0) continue;
    if (chunks > 0x7fffffff) return MI_ERR_UNSUPPORTED;
    t.ticket = tickets ? tickets + launch++ : nullptr;
    MI_LAUNCH("adam_dense", k_adam_dense, (int)chunks, kBlock, stream, t, lr, beta1, beta2, eps, weight_decay);
    if (!tickets) MI_LAUNCH("adam_steps_inc", k_adam_steps_inc, 1, kWave, stream, t);
  }
  return launch_status();
}

int mi_scatter_axpy_rows(const int64_t *idx, const float *g, float alpha, float *W, int64_t n, int32_t D, int64_t N,
                         void *stream) {
  if (n < 0 || D <= 0 || N < 0) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!idx || !g || !W) return MI_ERR_INVALID_ARG;
  int64_t gsz = (n * D + kBlock - 1) / kBlock;
  if (gsz > kMaxGrid) gsz = kMaxGrid;
  MI_LAUNCH("scatter_axpy_rows", k_scatter_axpy, (int)gsz, kBlock, stream, idx, g, alpha, W, n, D, N);
  return launch_status();
}

}  // extern "C"
