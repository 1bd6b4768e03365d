// optembed_cf.hip — OptEmbed supernet for the CF tables (LightGCN / SingleLightGCN / NeuMF):
// OptEmbed.get_weight of src/models/embeddings/lightgcn_opt_embed.py:121-177 with _MaskEmbeddingModule, BinaryStep
// (optembed_utils.py:25-86) and the dimension draws of _sampling_by_weight (optembed_utils.py:181-202) and of the
// field mode (lightgcn_opt_embed.py:138-152).  Table form: row r of W gives row r of the output, no index array.
//
//   out[r, j] = W[r, j] * s_r * [j <= k_r],   s_r = [ ||W[r]||_p - t(r) > 0 ],  p = 1 or 2
//   t(r): one threshold per field (field = row range of field_off) or per row; t NULL = no row mask.
//   k_r : given per row / per field, drawn here (written to k, one per row or one per field), or NULL = all dims.
//   backward:  G = g * [j <= k_r],  c_r = sum_j G_j W_j,  u_r = ||W[r]||_p - t(r)
//              dW[r] = G * s_r + c_r * a(u_r) * d||W[r]||_p / dW[r]      (one plain store per element)
//              dt    = -c_r * a(u_r): per row directly; per field through a row workspace and one fixed-order fold.
//   a(u) = BinaryStep's surrogate (2 - 4|u| for |u| <= 0.4, 0.4 for |u| <= 1, else 0); d||w||_1 = sign(w),
//   d||w||_2 = w / ||w|| (0 at ||w|| = 0, as torch).
//
// Layout: a group of LPR lanes owns a row; with D % 4 == 0 each lane moves float4s (D = 64: 16 lanes, four rows per
// wave).  Norms and c_r are group reductions by xor shuffles in a fixed order, so results do not depend on the run.
//
// Draws: counter-based, bits = mix(seed[0], salt, key) with key = row (or field).  seed[0] is read from the device and
// bumped by the launch itself: every workgroup reads it once (thread 0, through LDS), then takes a ticket in seed[1];
// the workgroup whose ticket comes back last writes seed[0] + 1 and resets the ticket with plain vector stores.  A
// captured graph therefore draws a fresh mask on every replay without host work.
#include "common.hpp"

namespace {
using namespace mi;

constexpr int kMaxChunks = 4;     // float4 (or float) chunks a lane holds: D <= 1024 (vector path), D <= 256 (scalar)

__device__ __forceinline__ float surrogate(float u) {
  const float a = fabsf(u);
  return a > 1.f ? 0.f : (a > 0.4f ? 0.4f : 2.f - 4.f * a);
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// one draw of the last kept dimension: law 0 uniform on [0, hi), law 1 inverse CDF (cdf[D], float64, last entry 1)
__device__ __forceinline__ int64_t draw_k(uint64_t seed, uint64_t salt, uint64_t key, int law, int hi, const double *cdf,
                                          int D) {
  const uint64_t bits = mix64(mix64(seed + 0x9E3779B97F4A7C15ull * (salt + 1)) + 0xD1B54A32D192ED03ull * (key + 1));
  if (law == 0) return (int64_t)(((bits >> 32) * (uint64_t)hi) >> 32);
  const double u = (double)(bits >> 11) * 0x1.0p-53;
  int lo = 0, up = D - 1;                 // smallest j with u < cdf[j]
  while (lo < up) {
    const int mid = (lo + up) >> 1;
    if (u < cdf[mid]) up = mid; else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ int field_of(const int64_t *off, int F, int64_t r) {
  int lo = 0, up = F - 1;                 // last f with off[f] <= r
  while (lo < up) {
    const int mid = (lo + up + 1) >> 1;
    if (off[mid] <= r) lo = mid; else up = mid - 1;
  }
  return lo;
}

template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

struct CfArgs {
  const float *W;          // [N, D] (NULL: draw only)
  const float *t;          // thresholds, per field or per row (NULL: no row mask)
  int t_field;
  const int64_t *off;      // [F + 1] field row offsets (needed when anything is per field)
  int F;
  int64_t *k;              // [N] or [F] last kept dims (NULL: all)
  int k_field;
  int draw;                // k is written here
  int law, hi;
  const double *cdf;
  int64_t *seed;           // [2]: seed word, ticket
  int64_t salt;
  int norm;
  int64_t N;
  int D;
};

// VW = 4: lane q of a group holds float4 chunks at columns 4 * (q + i * LPR); VW = 1: floats at q + i * LPR
template <int LPR, int VW>
struct Row {
  float v[kMaxChunks * VW];
  __device__ __forceinline__ static bool has(int q, int i, int D) { return (q + i * LPR) * VW < D; }
  __device__ __forceinline__ void load(const float *p, int q, int D) {
#pragma unroll
    for (int i = 0; i < kMaxChunks; ++i) {
      if (!has(q, i, D)) {
#pragma unroll
        for (int e = 0; e < VW; ++e) v[i * VW + e] = 0.f;
        continue;
      }
      if constexpr (VW == 4) {
        const float4 x = ld4(p + 4 * (q + i * LPR));
        v[i * 4] = x.x; v[i * 4 + 1] = x.y; v[i * 4 + 2] = x.z; v[i * 4 + 3] = x.w;
      } else {
        v[i] = p[q + i * LPR];
      }
    }
  }
  __device__ __forceinline__ void store(float *p, int q, int D) const {
#pragma unroll
    for (int i = 0; i < kMaxChunks; ++i) {
      if (!has(q, i, D)) continue;
      if constexpr (VW == 4) st4(p + 4 * (q + i * LPR), make_float4(v[i * 4], v[i * 4 + 1], v[i * 4 + 2], v[i * 4 + 3]));
      else p[q + i * LPR] = v[i];
    }
  }
  __device__ __forceinline__ static int col(int q, int i, int e) { return (q + i * LPR) * VW + e; }
};

template <int LPR>
__device__ __forceinline__ float norm_of(const float *v, int n, int p) {
  float acc = 0.f;
  for (int e = 0; e < n; ++e) acc += p == 1 ? fabsf(v[e]) : v[e] * v[e];
  acc = group_sum<LPR>(acc);
  return p == 1 ? acc : sqrtf(acc);
}

template <int LPR, int VW>
__global__ __launch_bounds__(kBlock) void k_optembed_cf_fwd(CfArgs a, float *__restrict__ out, int *err) {
  __shared__ int64_t s_seed;
  const int q = threadIdx.x % LPR;
  const int64_t gid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LPR;
  const int64_t ngroups = (int64_t)gridDim.x * kBlock / LPR;
  if (a.draw) {
    if (threadIdx.x == 0) s_seed = a.seed[0];
    __syncthreads();
  }
  const uint64_t seed = a.draw ? (uint64_t)s_seed : 0ull;
  int bad = 0;
  if (a.draw && a.k_field) {              // one width per field, written once; every row of the field recomputes it
    for (int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x; f < a.F; f += (int64_t)gridDim.x * kBlock)
      a.k[f] = draw_k(seed, (uint64_t)a.salt, (uint64_t)f, a.law, a.hi, a.cdf, a.D);
  }
  for (int64_t r = gid; r < a.N; r += ngroups) {
    const bool need_f = (a.t && a.t_field) || (a.k && a.k_field);
    const int f = need_f ? field_of(a.off, a.F, r) : 0;
    int64_t kr = a.D - 1;
    if (a.k) {
      if (a.draw) {
        kr = draw_k(seed, (uint64_t)a.salt, (uint64_t)(a.k_field ? f : r), a.law, a.hi, a.cdf, a.D);
        if (!a.k_field && q == 0) a.k[r] = kr;
      } else {
        kr = a.k[a.k_field ? f : r];
        bad |= (uint64_t)kr >= (uint64_t)a.D;
      }
    }
    if (!a.W) continue;
    Row<LPR, VW> w;
    w.load(a.W + r * a.D, q, a.D);
    float s = 1.f;
    if (a.t) {
      const float nrm = norm_of<LPR>(w.v, kMaxChunks * VW, a.norm);
      s = (nrm - a.t[a.t_field ? f : r]) > 0.f ? 1.f : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kMaxChunks; ++i)
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        const int j = Row<LPR, VW>::col(q, i, e);
        w.v[i * VW + e] = j <= kr ? w.v[i * VW + e] * s : 0.f;
      }
    w.store(out + r * a.D, q, a.D);
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
  if (a.draw) {                           // the last workgroup to finish bumps the seed word
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long *ticket = reinterpret_cast<unsigned long long *>(a.seed + 1);
      const unsigned long long n = __hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (n == (unsigned long long)gridDim.x - 1) {
        a.seed[1] = 0;
        a.seed[0] = (int64_t)seed + 1;
      }
    }
  }
}

template <int LPR, int VW>
__global__ __launch_bounds__(kBlock) void k_optembed_cf_bwd(CfArgs a, const float *__restrict__ g, float *__restrict__ dW,
                                                            float *__restrict__ dt_out) {
  const int q = threadIdx.x % LPR;
  const int64_t gid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LPR;
  const int64_t ngroups = (int64_t)gridDim.x * kBlock / LPR;
  for (int64_t r = gid; r < a.N; r += ngroups) {
    const bool need_f = (a.t && a.t_field) || (a.k && a.k_field);
    const int f = need_f ? field_of(a.off, a.F, r) : 0;
    const int64_t kr = a.k ? a.k[a.k_field ? f : r] : (int64_t)a.D - 1;
    Row<LPR, VW> gg;
    gg.load(g + r * a.D, q, a.D);
#pragma unroll
    for (int i = 0; i < kMaxChunks; ++i)
#pragma unroll
      for (int e = 0; e < VW; ++e)
        if (Row<LPR, VW>::col(q, i, e) > kr) gg.v[i * VW + e] = 0.f;       // G = g * [j <= k_r]
    if (!a.t) {
      if (dW) gg.store(dW + r * a.D, q, a.D);
      continue;
    }
    Row<LPR, VW> w;
    w.load(a.W + r * a.D, q, a.D);
    float c = 0.f;
#pragma unroll
    for (int e = 0; e < kMaxChunks * VW; ++e) c += gg.v[e] * w.v[e];
    c = group_sum<LPR>(c);
    const float nrm = norm_of<LPR>(w.v, kMaxChunks * VW, a.norm);
    const float u = nrm - a.t[a.t_field ? f : r];
    const float s = u > 0.f ? 1.f : 0.f;
    const float ca = c * surrogate(u);
    if (dt_out && q == 0) dt_out[r] = -ca;
    if (dW) {
#pragma unroll
      for (int e = 0; e < kMaxChunks * VW; ++e) {
        const float x = w.v[e];
        const float dn = a.norm == 1 ? (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f)) : (nrm > 0.f ? x / nrm : 0.f);
        gg.v[e] = gg.v[e] * s + ca * dn;
      }
      gg.store(dW + r * a.D, q, a.D);
    }
  }
}

// dt[f] = sum over the rows of field f of dt_rows, in a fixed order: thread i sums rows i, i + 256, ... in turn, then a
// fixed tree over the block.  One workgroup per field.
__global__ __launch_bounds__(kBlock) void k_optembed_cf_fold(const float *__restrict__ dt_rows, const int64_t *off,
                                                             float *__restrict__ dt) {
  __shared__ float part[kBlock];
  const int f = blockIdx.x;
  float acc = 0.f;
  for (int64_t r = off[f] + threadIdx.x; r < off[f + 1]; r += kBlock) acc += dt_rows[r];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) dt[f] = part[0];
}

inline int rows_grid(int64_t N, int lpr) {
  const int64_t groups_per_block = kBlock / lpr;
  int64_t g = (N + groups_per_block - 1) / groups_per_block;
  if (g < 1) g = 1;
  if (g > kMaxGrid) g = kMaxGrid;
  return (int)g;
}

// lanes per row: the power of two that covers a row in at most kMaxChunks chunks
inline int lanes_per_row(int D, int vw) {
  const int chunks = (D + vw - 1) / vw;
  int l = 1;
  while (l < kWave && l < chunks) l <<= 1;
  return l;
}

inline bool vector_ok(const CfArgs &a, const void *p0, const void *p1, const void *p2) {
  return a.D % 4 == 0 && (!p0 || aligned16(p0)) && (!p1 || aligned16(p1)) && (!p2 || aligned16(p2));
}

inline bool shape_ok(int D, bool vec) { return D >= 1 && D <= kWave * kMaxChunks * (vec ? 4 : 1); }

#define MI_CF_DISPATCH(KERNEL, NAME, STREAM, ...)                                                                  \
  do {                                                                                                             \
    switch (lpr * 8 + vw) {                                                                                        \
      case 1 * 8 + 4: MI_LAUNCH(NAME, (KERNEL<1, 4>), rows_grid(a.N, 1), kBlock, STREAM, __VA_ARGS__); break;      \
      case 2 * 8 + 4: MI_LAUNCH(NAME, (KERNEL<2, 4>), rows_grid(a.N, 2), kBlock, STREAM, __VA_ARGS__); break;      \
      case 4 * 8 + 4: MI_LAUNCH(NAME, (KERNEL<4, 4>), rows_grid(a.N, 4), kBlock, STREAM, __VA_ARGS__); break;      \
      case 8 * 8 + 4: MI_LAUNCH(NAME, (KERNEL<8, 4>), rows_grid(a.N, 8), kBlock, STREAM, __VA_ARGS__); break;      \
      case 16 * 8 + 4: MI_LAUNCH(NAME, (KERNEL<16, 4>), rows_grid(a.N, 16), kBlock, STREAM, __VA_ARGS__); break;   \
      case 32 * 8 + 4: MI_LAUNCH(NAME, (KERNEL<32, 4>), rows_grid(a.N, 32), kBlock, STREAM, __VA_ARGS__); break;   \
      case 64 * 8 + 4: MI_LAUNCH(NAME, (KERNEL<64, 4>), rows_grid(a.N, 64), kBlock, STREAM, __VA_ARGS__); break;   \
      default: MI_LAUNCH(NAME, (KERNEL<64, 1>), rows_grid(a.N, 64), kBlock, STREAM, __VA_ARGS__); break;           \
    }                                                                                                              \
  } while (0)

inline int fill(CfArgs &a, const float *W, const float *t, int32_t t_per_field, const int64_t *field_off, int32_t F,
                int64_t *k, int32_t k_per_field, int32_t norm, int64_t N, int32_t D) {
  if (N < 0 || D < 1 || (norm != 1 && norm != 2) || F < 1) return MI_ERR_INVALID_ARG;
  if (((t && t_per_field) || (k && k_per_field)) && !field_off) return MI_ERR_INVALID_ARG;
  a.W = W; a.t = t; a.t_field = t_per_field != 0; a.off = field_off; a.F = F; a.k = k; a.k_field = k_per_field != 0;
  a.draw = 0; a.law = 0; a.hi = D; a.cdf = nullptr; a.seed = nullptr; a.salt = 0; a.norm = norm; a.N = N; a.D = D;
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_optembed_cf_fwd(const float *W, const float *t, int32_t t_per_field, const int64_t *field_off, int32_t F,
                       int64_t *k, int32_t k_per_field, int32_t draw, int32_t law, int32_t law_hi, const double *cdf,
                       int64_t *seed, int64_t salt, int32_t norm, float *out, int64_t N, int32_t D, int32_t *err,
                       void *stream) {
  CfArgs a;
  const int rc = fill(a, W, t, t_per_field, field_off, F, k, k_per_field, norm, N, D);
  if (rc != MI_OK) return rc;
  if (draw) {
    if (!k || !seed || (law != 0 && law != 1)) return MI_ERR_INVALID_ARG;
    if (law == 0 && (law_hi < 1 || law_hi > D)) return MI_ERR_INVALID_ARG;
    if (law == 1 && !cdf) return MI_ERR_INVALID_ARG;
    a.draw = 1; a.law = law; a.hi = law_hi; a.cdf = cdf; a.seed = seed; a.salt = salt;
  }
  if (!W && !draw) return MI_ERR_INVALID_ARG;
  if (W && !out) return MI_ERR_INVALID_ARG;
  if (N == 0 && !(draw && k_per_field)) return MI_OK;
  const int vw = vector_ok(a, W, out, nullptr) ? 4 : 1;
  if (W && !shape_ok(D, vw == 4)) return MI_ERR_INVALID_ARG;
  const int lpr = vw == 4 ? lanes_per_row(D, 4) : 64;
  MI_CF_DISPATCH(k_optembed_cf_fwd, "optembed_cf_fwd", stream, a, out, err);
  return launch_status();
}

int mi_optembed_cf_bwd(const float *W, const float *t, int32_t t_per_field, const int64_t *field_off, int32_t F,
                       const int64_t *k, int32_t k_per_field, int32_t norm, const float *g, float *dW, float *dt,
                       float *dt_rows, int64_t N, int32_t D, void *stream) {
  CfArgs a;
  const int rc = fill(a, W, t, t_per_field, field_off, F, const_cast<int64_t *>(k), k_per_field, norm, N, D);
  if (rc != MI_OK) return rc;
  if (!g || (t && !W)) return MI_ERR_INVALID_ARG;
  const bool fold = t && dt && t_per_field;
  if (fold && (!dt_rows || !field_off)) return MI_ERR_INVALID_ARG;
  if (N == 0) {                           // fields with no rows: the fold writes zeros
    if (fold) MI_LAUNCH("optembed_cf_fold", k_optembed_cf_fold, F, kBlock, stream, dt_rows, field_off, dt);
    return launch_status();
  }
  const int vw = vector_ok(a, W, g, dW) ? 4 : 1;
  if (!shape_ok(D, vw == 4)) return MI_ERR_INVALID_ARG;
  const int lpr = vw == 4 ? lanes_per_row(D, 4) : 64;
  float *dt_out = !(t && dt) ? nullptr : (fold ? dt_rows : dt);
  MI_CF_DISPATCH(k_optembed_cf_bwd, "optembed_cf_bwd", stream, a, g, dW, dt_out);
  if (fold) MI_LAUNCH("optembed_cf_fold", k_optembed_cf_fold, F, kBlock, stream, dt_rows, field_off, dt);
  return launch_status();
}

}  // extern "C"
