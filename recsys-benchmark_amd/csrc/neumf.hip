// neumf.hip — NeuMF (GMF + MLP) lookup, backward and all-items scoring (src/models/mlp.py:11-344).
//
// mi_neumf_fwd: four row gathers per sample, the GMF score and the MLP tower's input row [mu ; mi].
// mi_neumf_bwd: the four tables' gradients (dense by float atomics, or row form) and gmf_fc's, the latter reduced in a
//   fixed order (per-workgroup partials, then one finishing workgroup) so they are reproducible in every mode.
// mi_neumf_score_all: every (user, item) pair of a user batch through the whole model.  Layer 1 comes in split
//   (P = U W1_u^T, Q = I W1_i^T + b1, two GEMMs of the library); the kernel builds relu(P[b] + Q[i]) straight into the
//   B operand of v_mfma_f32_16x16x4_f32 and runs the remaining hidden layers transposed (features on the rows, pairs on
//   the columns), so that one layer's accumulator registers are the next layer's B operand with no lane movement.
#include "common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxD = 256;                   // row width (emb_size / 2) the lookup kernels take
constexpr int kMaxJ = kMaxD / mi::kWave;     // k slots per lane at 64 lanes per sample

__device__ __forceinline__ bool in_range(int64_t v, int64_t n) { return v >= 0 && v < n; }

template <int LPS>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = 1; m < LPS; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// LPS lanes per sample; lane q of a sample handles k = q, q + LPS, ...
template <int LPS>
__global__ void __launch_bounds__(mi::kBlock) k_neumf_fwd(const int64_t *__restrict__ users, const int64_t *__restrict__ items,
                                                          int64_t S, const float *__restrict__ GU, const float *__restrict__ GI,
                                                          const float *__restrict__ MU, const float *__restrict__ MI, int D,
                                                          int64_t nU, int64_t nI, const float *__restrict__ w,
                                                          const float *__restrict__ b, float *__restrict__ y,
                                                          float *__restrict__ X0, int32_t *err) {
  const int q = threadIdx.x % LPS;
  const int64_t per_block = mi::kBlock / LPS;
  for (int64_t s = blockIdx.x * per_block + threadIdx.x / LPS; s < S; s += (int64_t)gridDim.x * per_block) {
    const int64_t u = users[s], it = items[s];
    const bool ok = in_range(u, nU) && in_range(it, nI);
    if (!ok && q == 0 && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
    float acc = 0.f;
    for (int k = q; k < D; k += LPS) {
      if (y) {
        const float gu = ok ? GU[u * D + k] : 0.f, gi = ok ? GI[it * D + k] : 0.f;
        acc = fmaf(gu * gi, w[k], acc);
      }
      if (X0) {
        X0[s * 2 * D + k] = ok ? MU[u * D + k] : 0.f;
        X0[s * 2 * D + D + k] = ok ? MI[it * D + k] : 0.f;
      }
    }
    if (y) {
      acc = group_sum<LPS>(acc);
      if (q == 0) y[s] = acc + b[0];
    }
  }
}

// mode 0: out* are dense [n, D] tables (caller-zeroed), float atomics; mode 1: out* are row-form [S, D] values.
// part: [gridDim.x, D + 1] per-workgroup sums of dy (gu . gi) and dy (only when dy is given).
template <int LPS>
__global__ void __launch_bounds__(mi::kBlock) k_neumf_bwd(const int64_t *__restrict__ users, const int64_t *__restrict__ items,
                                                          int64_t S, const float *__restrict__ GU, const float *__restrict__ GI,
                                                          int D, int64_t nU, int64_t nI, const float *__restrict__ w,
                                                          const float *__restrict__ dy, const float *__restrict__ dX0, int mode,
                                                          float *oGU, float *oGI, float *oMU, float *oMI,
                                                          float *__restrict__ part) {
  constexpr int kSub = mi::kBlock / LPS;
  constexpr int kJ = LPS == mi::kWave ? kMaxJ : 1;     // lanes_per_sample: LPS < 64 only for D <= LPS
  __shared__ float red[kSub][kMaxD + 1];
  const int q = threadIdx.x % LPS, sub = threadIdx.x / LPS;
  float dw[kJ];
#pragma unroll
  for (int j = 0; j < kJ; ++j) dw[j] = 0.f;
  float db = 0.f;
  for (int64_t s = blockIdx.x * kSub + sub; s < S; s += (int64_t)gridDim.x * kSub) {
    const int64_t u = users[s], it = items[s];
    const bool ok = in_range(u, nU) && in_range(it, nI);
    const float g = dy ? dy[s] : 0.f;
    db += g;
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
      const int k = q + j * LPS;
      if (k >= D) break;
      if (dy) {
        const float gu = ok ? GU[u * D + k] : 0.f, gi = ok ? GI[it * D + k] : 0.f;
        const float gw = g * w[k];
        dw[j] = fmaf(g, gu * gi, dw[j]);
        if (mode == 0) {
          if (ok) {
            unsafeAtomicAdd(oGU + u * D + k, gw * gi);
            unsafeAtomicAdd(oGI + it * D + k, gw * gu);
          }
        } else {
          oGU[s * D + k] = gw * gi;
          oGI[s * D + k] = gw * gu;
        }
      }
      if (dX0) {
        const float a = dX0[s * 2 * D + k], c = dX0[s * 2 * D + D + k];
        if (mode == 0) {
          if (ok) {
            unsafeAtomicAdd(oMU + u * D + k, a);
            unsafeAtomicAdd(oMI + it * D + k, c);
          }
        } else {
          oMU[s * D + k] = ok ? a : 0.f;
          oMI[s * D + k] = ok ? c : 0.f;
        }
      }
    }
  }
  if (!dy) return;
#pragma unroll
  for (int j = 0; j < kJ; ++j) {
    const int k = q + j * LPS;
    if (k < D) red[sub][k] = dw[j];
  }
  if (q == 0) red[sub][D] = db;
  __syncthreads();
  for (int k = threadIdx.x; k <= D; k += mi::kBlock) {   // subgroups joined in index order: fixed summation order
    float t = 0.f;
    for (int r = 0; r < kSub; ++r) t += red[r][k];
    part[(int64_t)blockIdx.x * (D + 1) + k] = t;
  }
}

__global__ void __launch_bounds__(mi::kBlock) k_neumf_bwd_finish(const float *__restrict__ part, int nparts, int D,
                                                                 float *__restrict__ dw, float *__restrict__ db) {
  for (int k = threadIdx.x; k <= D; k += mi::kBlock) {
    float t = 0.f;
    for (int p = 0; p < nparts; ++p) t += part[(int64_t)p * (D + 1) + k];
    if (k < D)
      dw[k] = t;
    else
      db[0] = t;
  }
}

// ---- all-items scoring ------------------------------------------------------------------------------------------
constexpr int kMaxHidden = 4;                 // hidden layers (hidden_sizes entries)
constexpr int kScoreUsers = 64;               // users per workgroup (each wave walks them for its 16 items)
constexpr int kScoreItems = 16 * mi::kWavesPerBlock;
constexpr int kMaxScoreD = 128;               // GMF row width held in registers: kMaxScoreD / 4 per lane
constexpr int kMaxLdsFloats = 16384;          // permuted hidden weights + biases + mlp_fc + gmf_fc weights (64 KiB)

struct ScoreArgs {
  const float *P, *Q;                          // [B, h0] and [N, h0] (b1 folded into Q)
  const int64_t *users;                        // [B] ids into GU
  const float *GU, *GI, *wg, *bg;              // GMF tables, gmf_fc weight [D] / bias [1]
  const float *W[kMaxHidden - 1], *bias[kMaxHidden - 1];   // layers 2..nl: [h_l, h_{l-1}], [h_l]
  const float *wf, *bf;                        // mlp_fc weight [h_{nl-1}] / bias [1]
  float *scores;
  int64_t B, N, nU, ld;
  int32_t *err;
  int h[kMaxHidden];
  int nl, D, flags;
  int w_off[kMaxHidden - 1], b_off[kMaxHidden - 1], wf_off, wg_off;   // LDS offsets (floats)
};

__host__ __device__ __forceinline__ int tiles16(int n) { return (n + 15) >> 4; }

// T: 16-feature tiles per lane held for a layer (widths <= 16 T).
template <int T>
__global__ void __launch_bounds__(mi::kBlock) k_neumf_score(ScoreArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int il = lane & 15, g = lane >> 4;
  const bool mlp = a.flags & 1, gmf = a.flags & 2;

  // prologue: hidden weights in A-operand order (see the header comment of this file), zero-padded to whole tiles
  if (mlp) {
    for (int l = 1; l < a.nl; ++l) {
      const int hin = a.h[l - 1], hout = a.h[l], ti = tiles16(hin), to = tiles16(hout);
      const int n = to * ti * 4 * 64;
      for (int e = threadIdx.x; e < n; e += mi::kBlock) {
        const int ln = e & 63, r = (e >> 6) & 3, blk = e >> 8, t = blk % ti, o = blk / ti;
        const int f = 16 * o + (ln & 15), k = 16 * t + 4 * (ln >> 4) + r;
        lds[a.w_off[l - 1] + e] = (f < hout && k < hin) ? a.W[l - 1][(int64_t)f * hin + k] : 0.f;
      }
      for (int e = threadIdx.x; e < 16 * to; e += mi::kBlock) lds[a.b_off[l - 1] + e] = e < hout ? a.bias[l - 1][e] : 0.f;
    }
    const int hl = a.h[a.nl - 1];
    for (int e = threadIdx.x; e < 16 * tiles16(hl); e += mi::kBlock) lds[a.wf_off + e] = e < hl ? a.wf[e] : 0.f;
  }
  if (gmf)
    for (int e = threadIdx.x; e < a.D; e += mi::kBlock) lds[a.wg_off + e] = a.wg[e];
  __syncthreads();

  const int64_t i = (int64_t)blockIdx.x * kScoreItems + 16 * wave + il;
  const bool vi = i < a.N;
  const int h0 = a.h[0], t0 = tiles16(h0);
  float q[T][4];                               // this lane's item: Q[i][16t + 4g + r]
  float gi[kMaxScoreD / 4];                    // GI[i][4j + g]
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 16 * t + 4 * g + r;
      q[t][r] = (mlp && vi && f < h0) ? a.Q[i * h0 + f] : 0.f;
    }
#pragma unroll
  for (int j = 0; j < kMaxScoreD / 4; ++j) {
    const int k = 4 * j + g;
    gi[j] = (gmf && vi && k < a.D) ? a.GI[i * a.D + k] : 0.f;
  }
  const float tail_bias = (mlp ? a.bf[0] : 0.f) + (gmf ? a.bg[0] : 0.f);

  const int64_t b_end = min((int64_t)(blockIdx.y + 1) * kScoreUsers, a.B);
  for (int64_t b = (int64_t)blockIdx.y * kScoreUsers; b < b_end; ++b) {
    float part = 0.f;
    if (mlp) {
      f32x4 x[T];
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 16 * t + 4 * g + r;
          x[t][r] = (t < t0 && f < h0) ? fmaxf(a.P[b * h0 + f] + q[t][r], 0.f) : 0.f;
        }
      int tin = t0;
#pragma unroll
      for (int l = 1; l < kMaxHidden; ++l) {
        if (l >= a.nl) continue;
        const int tout = tiles16(a.h[l]);
        const float *wl = lds + a.w_off[l - 1];
        const float *bl = lds + a.b_off[l - 1];
        f32x4 y[T];
#pragma unroll
        for (int o = 0; o < T; ++o)
#pragma unroll
          for (int r = 0; r < 4; ++r) y[o][r] = o < tout ? bl[16 * o + 4 * g + r] : 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t) {
          if (t < tin) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int o = 0; o < T; ++o)
                if (o < tout) {
                  const float w = wl[((o * tin + t) * 4 + r) * 64 + lane];
                  y[o] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, x[t][r], y[o], 0, 0, 0);
                }
          }
        }
#pragma unroll
        for (int o = 0; o < T; ++o)
#pragma unroll
          for (int r = 0; r < 4; ++r) x[o][r] = o < tout ? fmaxf(y[o][r], 0.f) : 0.f;
        tin = tout;
      }
      const float *wf = lds + a.wf_off;
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (t < tin) {
#pragma unroll
          for (int r = 0; r < 4; ++r) part = fmaf(wf[16 * t + 4 * g + r], x[t][r], part);
        }
    }
    if (gmf) {
      const int64_t u = a.users[b];
      const bool ok = in_range(u, a.nU);
      if (!ok && lane == 0 && a.err) atomicOr(a.err, MI_IDX_OUT_OF_RANGE);
      const float *wg = lds + a.wg_off;
#pragma unroll
      for (int j = 0; j < kMaxScoreD / 4; ++j) {
        const int k = 4 * j + g;
        if (4 * j < a.D) {
          const float gu = (ok && k < a.D) ? a.GU[u * a.D + k] : 0.f;
          part = fmaf(gu * (k < a.D ? wg[k] : 0.f), gi[j], part);
        }
      }
    }
    part += __shfl_xor(part, 16);
    part += __shfl_xor(part, 32);
    if (g == 0 && vi) a.scores[b * a.ld + i] = part + tail_bias;
  }
}

template <int LPS>
int launch_fwd(const int64_t *users, const int64_t *items, int64_t S, const float *GU, const float *GI, const float *MU,
               const float *MI, int D, int64_t nU, int64_t nI, const float *w, const float *b, float *y, float *X0,
               int32_t *err, void *stream) {
  const int grid = mi::grid_for_waves((S * LPS + mi::kWave - 1) / mi::kWave);
  MI_LAUNCH("k_neumf_fwd", k_neumf_fwd<LPS>, grid, mi::kBlock, stream, users, items, S, GU, GI, MU, MI, D, nU, nI, w, b, y,
            X0, err);
  return mi::launch_status();
}

template <int LPS>
int launch_bwd(const int64_t *users, const int64_t *items, int64_t S, const float *GU, const float *GI, int D, int64_t nU,
               int64_t nI, const float *w, const float *dy, const float *dX0, int mode, float *oGU, float *oGI, float *oMU,
               float *oMI, float *part, int grid, void *stream) {
  MI_LAUNCH("k_neumf_bwd", k_neumf_bwd<LPS>, grid, mi::kBlock, stream, users, items, S, GU, GI, D, nU, nI, w, dy, dX0, mode,
            oGU, oGI, oMU, oMI, part);
  return mi::launch_status();
}

int lanes_per_sample(int D) { return D <= 16 ? 16 : D <= 32 ? 32 : 64; }

}  // namespace

extern "C" {

MI_API int mi_neumf_fwd(const int64_t *users, const int64_t *items, int64_t S, const float *GU, const float *GI,
                        const float *MU, const float *MI, int32_t D, int64_t nU, int64_t nI, const float *w, const float *b,
                        int32_t flags, float *y_gmf, float *X0, int32_t *err, void *stream) {
  const bool mlp = flags & 1, gmf = flags & 2;
  if (S < 0 || D <= 0 || D > kMaxD || (flags & ~3) || !(mlp || gmf)) return MI_ERR_INVALID_ARG;
  if (S == 0) return MI_OK;
  if (!users || !items || (gmf && (!GU || !GI || !w || !b || !y_gmf)) || (mlp && (!MU || !MI || !X0)))
    return MI_ERR_INVALID_ARG;
  float *y = gmf ? y_gmf : nullptr;
  float *x = mlp ? X0 : nullptr;
  switch (lanes_per_sample(D)) {
    case 16: return launch_fwd<16>(users, items, S, GU, GI, MU, MI, D, nU, nI, w, b, y, x, err, stream);
    case 32: return launch_fwd<32>(users, items, S, GU, GI, MU, MI, D, nU, nI, w, b, y, x, err, stream);
    default: return launch_fwd<64>(users, items, S, GU, GI, MU, MI, D, nU, nI, w, b, y, x, err, stream);
  }
}

MI_API int mi_neumf_bwd_parts(int64_t S, int32_t D) {
  const int lps = lanes_per_sample(D);
  const int64_t sub = mi::kBlock / lps;
  int64_t g = (S + sub - 1) / sub;
  if (g < 1) g = 1;
  if (g > mi::kMaxGrid) g = mi::kMaxGrid;
  return (int)g;
}

MI_API int mi_neumf_bwd(const int64_t *users, const int64_t *items, int64_t S, const float *GU, const float *GI, int32_t D,
                        int64_t nU, int64_t nI, const float *w, int32_t flags, const float *dy, const float *dX0, int32_t mode,
                        float *dGU, float *dGI, float *dMU, float *dMI, float *dw, float *db, float *workspace,
                        void *stream) {
  const bool mlp = flags & 1, gmf = flags & 2;
  if (S < 0 || D <= 0 || D > kMaxD || (flags & ~3) || !(mlp || gmf) || (mode != 0 && mode != 1)) return MI_ERR_INVALID_ARG;
  if (!users || !items || (gmf && (!GU || !GI || !w || !dy || !dGU || !dGI || !dw || !db || !workspace)) ||
      (mlp && (!dX0 || !dMU || !dMI)))
    return MI_ERR_INVALID_ARG;
  const int grid = mi_neumf_bwd_parts(S, D);
  const float *g = gmf ? dy : nullptr;
  const float *x = mlp ? dX0 : nullptr;
  int rc;
  switch (lanes_per_sample(D)) {
    case 16: rc = launch_bwd<16>(users, items, S, GU, GI, D, nU, nI, w, g, x, mode, dGU, dGI, dMU, dMI, workspace, grid, stream); break;
    case 32: rc = launch_bwd<32>(users, items, S, GU, GI, D, nU, nI, w, g, x, mode, dGU, dGI, dMU, dMI, workspace, grid, stream); break;
    default: rc = launch_bwd<64>(users, items, S, GU, GI, D, nU, nI, w, g, x, mode, dGU, dGI, dMU, dMI, workspace, grid, stream); break;
  }
  if (rc != MI_OK || !gmf) return rc;
  MI_LAUNCH("k_neumf_bwd_finish", k_neumf_bwd_finish, 1, mi::kBlock, stream, (const float *)workspace, grid, (int)D, dw, db);
  return mi::launch_status();
}

MI_API int mi_neumf_score_supported(int32_t nhidden, const int32_t *hidden, int32_t D, int32_t flags) {
  const bool mlp = flags & 1, gmf = flags & 2;
  if ((flags & ~3) || !(mlp || gmf)) return 0;
  if (gmf && (D <= 0 || D > kMaxScoreD)) return 0;
  if (!mlp) return 1;
  if (nhidden < 1 || nhidden > kMaxHidden || !hidden) return 0;
  int64_t lds = 0;
  for (int l = 0; l < nhidden; ++l) {
    if (hidden[l] <= 0 || hidden[l] > 128) return 0;
    if (l > 0) lds += 256LL * tiles16(hidden[l]) * tiles16(hidden[l - 1]) + 16 * tiles16(hidden[l]);
  }
  lds += 16 * tiles16(hidden[nhidden - 1]) + kMaxScoreD;
  return lds <= kMaxLdsFloats;
}

MI_API int mi_neumf_score_all(const float *P, const float *Q, int64_t B, int64_t N, int32_t nhidden, const int32_t *hidden,
                              const float *const *W, const float *const *bias, const float *wf, const float *bf,
                              const int64_t *users, const float *GU, const float *GI, int32_t D, int64_t nU, const float *wg,
                              const float *bg, int32_t flags, float *scores, int64_t ld, int32_t *err, void *stream) {
  const bool mlp = flags & 1, gmf = flags & 2;
  if (B < 0 || N < 0 || ld < N || !scores) return MI_ERR_INVALID_ARG;
  if (!mi_neumf_score_supported(nhidden, hidden, D, flags)) return MI_ERR_UNSUPPORTED;
  if (mlp && (!P || !Q || !wf || !bf)) return MI_ERR_INVALID_ARG;
  if (gmf && (!users || !GU || !GI || !wg || !bg)) return MI_ERR_INVALID_ARG;
  if (B == 0 || N == 0) return MI_OK;
  if ((B + kScoreUsers - 1) / kScoreUsers > 65535) return MI_ERR_UNSUPPORTED;
  ScoreArgs a{};
  a.P = P; a.Q = Q; a.users = users; a.GU = GU; a.GI = GI; a.wg = wg; a.bg = bg; a.wf = wf; a.bf = bf;
  a.scores = scores; a.B = B; a.N = N; a.nU = nU; a.ld = ld; a.err = err; a.D = gmf ? D : 0; a.flags = flags;
  a.nl = mlp ? nhidden : 1;
  int off = 0, tmax = 1;
  for (int l = 0; l < kMaxHidden; ++l) a.h[l] = (mlp && l < nhidden) ? hidden[l] : 0;
  if (mlp) {
    for (int l = 0; l < nhidden; ++l) tmax = tiles16(hidden[l]) > tmax ? tiles16(hidden[l]) : tmax;
    for (int l = 1; l < nhidden; ++l) {
      if (!W || !bias || !W[l - 1] || !bias[l - 1]) return MI_ERR_INVALID_ARG;
      a.W[l - 1] = W[l - 1];
      a.bias[l - 1] = bias[l - 1];
      a.w_off[l - 1] = off;
      off += 256 * tiles16(hidden[l]) * tiles16(hidden[l - 1]);
      a.b_off[l - 1] = off;
      off += 16 * tiles16(hidden[l]);
    }
    a.wf_off = off;
    off += 16 * tiles16(hidden[nhidden - 1]);
  }
  a.wg_off = off;
  off += gmf ? D : 0;
  const size_t lds = (size_t)(off > 0 ? off : 1) * sizeof(float);
  const dim3 grid((unsigned)((N + kScoreItems - 1) / kScoreItems), (unsigned)((B + kScoreUsers - 1) / kScoreUsers));
  if (tmax <= 4)
    hipLaunchKernelGGL(k_neumf_score<4>, grid, dim3(mi::kBlock), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_neumf_score<8>, grid, dim3(mi::kBlock), lds, (hipStream_t)stream, a);
  return mi::launch_status();
}

}  // extern "C"
