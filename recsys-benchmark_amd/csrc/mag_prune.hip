// mag_prune.hip — global magnitude pruning of a trained table (src/utils.py:8-34 `prune`) as a k-th element selection,
// and the CSR of the pruned table (what PrunedEmbedding serves) without the dense pruned table being written.
//
//   key(w)  = bits(|w|) (31 bits, monotone in |w|; +0.0 and -0.0 share key 0)
//   row cut = per row the m-th largest key and the column up to which equals of it are protected (8 bytes per row);
//             D = 64 one wave per row (bitwise search by ballots), D = 8 / 16 / 32 several rows per wave, else generic
//   select  = radix select, most significant digit first (11 + 11 + 9 bits of the 31-bit key), of the k-th smallest
//             unprotected key T; integer histograms only (LDS adds per wave, integer global adds per workgroup), the
//             bucket choice is recomputed by every workgroup of the NEXT launch from the finished histogram — no host
//             read-back, no cross-workgroup hand-off inside a launch
//   apply   = out = (unprotected && key < T) ? +0 : w; equals of T: all or none, or — only when the cut falls inside a
//             run of equal keys — the first `prune_eq` of them in flat order (chunk counts, then a ranked pass).
//             The chunk counts are one more read of the whole table (k_finish): five table passes in the plain case,
//             six in this one, which is the normal one for a table of hundreds of millions of values
//   CSR     = per-row counts -> chunk scan -> row scan (crow) -> ballot/popcount compaction (col, values)
#include "common.hpp"

namespace mi {
namespace {

constexpr uint32_t kAbs = 0x7fffffffu;
constexpr int kBins0 = 2048, kBins1 = 2048, kBins2 = 512;     // digits: key[30:20], key[19:9], key[8:0]
constexpr int kShift0 = 20, kShift1 = 9;
constexpr int kMaxChunks = 8192;
constexpr int kHistUnroll = 4, kHistTilesPerBlock = 8, kHistMaxGrid = 1024;
// workspace words (uint32)
constexpr int kH0 = 0, kH1 = kH0 + kBins0, kH2 = kH1 + kBins1, kSt = kH2 + kBins2;
// state: [0] b0 [1] k1 | [2] prefix22 [3] k2 | [4] T [5] n_less [6] n_equal [7] prune_equal
constexpr int kStWords = 8;
constexpr int kChunk = kSt + kStWords;                          // kMaxChunks chunk counts of equals (tie path)
constexpr int kHeadWords = kChunk + kMaxChunks;                 // then the row cuts, uint2 per row
constexpr int64_t kHeadBytes = ((int64_t)kHeadWords * 4 + 15) / 16 * 16;

struct Geo {
  int64_t ldw;
  uint32_t total;      // N * D
  uint32_t D;
  int shift;           // log2(D) when D is a power of two, else -1
};

__device__ __forceinline__ void row_col(const Geo &g, uint32_t e, uint32_t &r, uint32_t &c) {
  if (g.shift >= 0) {
    r = e >> g.shift;
    c = e & (g.D - 1);
  } else {
    r = e / g.D;
    c = e - r * g.D;
  }
}

__device__ __forceinline__ bool is_protected(const uint2 *cut, uint32_t r, uint32_t c, uint32_t key) {
  if (cut == nullptr) return false;
  uint2 q = cut[r];
  return key > q.x || (key == q.x && c <= q.y);
}

// The bucket of `hist` (BINS bins) that holds the krem-th smallest element (1-based) and the rank inside it:
// res[0] = bucket, res[1] = krem - (elements below the bucket), res[2] = hist[bucket].  krem == 0 gives (0, 0, hist[0]).
// Every thread of the workgroup calls it; the result is in res[] (LDS, 3 words) after the call.
template <int BINS>
__device__ __forceinline__ void pick_bucket(const uint32_t *hist, uint32_t krem, uint32_t *sm, uint32_t *res) {
  constexpr int PER = BINS / kBlock;
  uint32_t h[PER], s = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    h[i] = hist[threadIdx.x * PER + i];
    s += h[i];
  }
  if (threadIdx.x == 0) {
    res[0] = 0;
    res[1] = 0;
    res[2] = h[0];
  }
  uint32_t tot;
  uint32_t below = block_excl_scan(s, sm, &tot);     // (barriers inside order the defaults before the winner's store)
  if (krem > below && krem - below <= s) {
    uint32_t rem = krem - below;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (rem != 0) {
        if (rem <= h[i]) {
          res[0] = threadIdx.x * PER + i;
          res[1] = rem;
          res[2] = h[i];
          rem = 0;
        } else {
          rem -= h[i];
        }
      }
    }
  }
  __syncthreads();
}

// ---- row cut ---------------------------------------------------------------------------------------------------------
// D a power of two < 64: D lanes per row, 64 / D rows per wave, ranks by D shuffles.
template <int D>
__global__ __launch_bounds__(kBlock) void k_row_cut_pow2(const float *__restrict__ W, int64_t ldw, int64_t N, int m,
                                                         uint2 *__restrict__ cut) {
  constexpr int RPW = kWave / D;
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane / D, col = lane % D;
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t wv = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); wv * RPW < N; wv += nwaves) {
    const int64_t row = wv * RPW + sub;
    const bool live = row < N;
    uint32_t key = live ? (__float_as_uint(W[row * ldw + col]) & kAbs) : 0u;
    int rank = 0;
#pragma unroll
    for (int f = 0; f < D; ++f) {
      uint32_t kf = __shfl(key, f, D);
      rank += (kf > key || (kf == key && f < col)) ? 1 : 0;
    }
    if (live && rank == m - 1) cut[row] = make_uint2(key, (uint32_t)col);
  }
}

// D = 64: one wave per row, one lane per element.  The m-th largest key by a bitwise search (31 ballots: the largest t
// with at least m keys >= t), then the column of the last protected equal of it from the ballot of the equals.
__global__ __launch_bounds__(kBlock) void k_row_cut_64(const float *__restrict__ W, int64_t ldw, int64_t N, int m,
                                                       uint2 *__restrict__ cut) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t row = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); row < N; row += nwaves) {
    const uint32_t key = __float_as_uint(W[row * ldw + lane]) & kAbs;
    uint32_t t = 0;
#pragma unroll
    for (int b = 30; b >= 0; --b) {
      const uint32_t cand = t | (1u << b);
      if (__popcll(__ballot(key >= cand)) >= m) t = cand;
    }
    const int need = m - __popcll(__ballot(key > t));          // >= 1 equals of t are protected
    const uint64_t eq = __ballot(key == t);
    if (key == t && __popcll(eq & below) == need - 1) cut[row] = make_uint2(t, (uint32_t)lane);
  }
}

// any D <= 1024: one wave per row, the keys staged in LDS, ranks by D broadcast reads per element
__global__ __launch_bounds__(kBlock) void k_row_cut_any(const float *__restrict__ W, int64_t ldw, int64_t N, int D, int m,
                                                        uint2 *__restrict__ cut) {
  __shared__ uint32_t keys[kWavesPerBlock][1024];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  uint32_t *kw = keys[wave];
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  // (a wave only ever reads its own LDS slice: wave-synchronous, the barriers below are per-iteration safety for the
  //  compiler's reordering, and every wave of the workgroup runs the same number of iterations)
  const int64_t iters = (N + nwaves - 1) / nwaves;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t row = it * nwaves + (int64_t)blockIdx.x * kWavesPerBlock + wave;
    const bool live = row < N;
    __syncthreads();
    if (live)
      for (int c = lane; c < D; c += kWave) kw[c] = __float_as_uint(W[row * ldw + c]) & kAbs;
    __syncthreads();
    if (live) {
      for (int c = lane; c < D; c += kWave) {
        const uint32_t key = kw[c];
        int rank = 0;
        for (int f = 0; f < D; ++f) {
          uint32_t kf = kw[f];
          rank += (kf > key || (kf == key && f < c)) ? 1 : 0;
        }
        if (rank == m - 1) cut[row] = make_uint2(key, (uint32_t)c);
      }
    }
  }
}

// ---- select: one histogram pass per digit --------------------------------------------------------------------------------
template <int PASS, int VEC>
__global__ __launch_bounds__(kBlock) void k_hist(const float *__restrict__ W, Geo g, const uint2 *__restrict__ cut,
                                                 uint32_t *__restrict__ ws, uint32_t k) {
  constexpr int BINS = PASS == 0 ? kBins0 : (PASS == 1 ? kBins1 : kBins2);
  constexpr int OFF = PASS == 0 ? kH0 : (PASS == 1 ? kH1 : kH2);
  constexpr int SH = PASS == 0 ? kShift0 : (PASS == 1 ? kShift1 : 0);
  constexpr int PSH = PASS == 1 ? kShift0 : kShift1;           // key >> PSH must equal the prefix (PASS > 0)
  __shared__ uint32_t h[kWavesPerBlock][BINS];
  __shared__ uint32_t sm[kWavesPerBlock], res[3];
  uint32_t prefix = 0;
  if (PASS == 1) {
    pick_bucket<kBins0>(ws + kH0, k, sm, res);
    prefix = res[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      ws[kSt + 0] = res[0];
      ws[kSt + 1] = res[1];
    }
  } else if (PASS == 2) {
    const uint32_t b0 = ws[kSt + 0], k1 = ws[kSt + 1];
    pick_bucket<kBins1>(ws + kH1, k1, sm, res);
    prefix = (b0 << (kShift0 - kShift1)) | res[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      ws[kSt + 2] = prefix;
      ws[kSt + 3] = res[1];
    }
  }
  for (int i = threadIdx.x; i < kWavesPerBlock * BINS; i += kBlock) (&h[0][0])[i] = 0;
  __syncthreads();
  uint32_t *hw = h[threadIdx.x >> 6];
  // kHistUnroll tiles per trip, their loads issued before the first LDS add: a workgroup covers many tiles (few
  // workgroups = few global merges onto the same few words), so the trips must not each wait out a load
  const uint64_t stride = (uint64_t)gridDim.x * kBlock * VEC;
  for (uint64_t e0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * VEC; e0 < g.total; e0 += stride * kHistUnroll) {
    uint32_t key[kHistUnroll][VEC], c[kHistUnroll];
    uint2 q[kHistUnroll];
    bool live[kHistUnroll];
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      const uint64_t e64 = e0 + stride * u;
      live[u] = e64 < g.total;
      q[u] = make_uint2(0, 0);
      c[u] = 0;
#pragma unroll
      for (int i = 0; i < VEC; ++i) key[u][i] = 0;
      if (live[u]) {
        uint32_t r;
        row_col(g, (uint32_t)e64, r, c[u]);
        const float *p = W + (int64_t)r * g.ldw + c[u];
        if (VEC == 4) {
          float4 v = ld4(p);
          key[u][0] = __float_as_uint(v.x) & kAbs;
          key[u][1 % VEC] = __float_as_uint(v.y) & kAbs;
          key[u][2 % VEC] = __float_as_uint(v.z) & kAbs;
          key[u][3 % VEC] = __float_as_uint(v.w) & kAbs;
        } else {
          key[u][0] = __float_as_uint(*p) & kAbs;
        }
        if (cut != nullptr) q[u] = cut[r];
      }
    }
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const uint32_t ky = key[u][i];
        const bool prot = cut != nullptr && (ky > q[u].x || (ky == q[u].x && c[u] + i <= q[u].y));
        const bool in = PASS == 0 || (ky >> PSH) == prefix;
        if (live[u] && !prot && in) atomicAdd(&hw[(ky >> SH) & (BINS - 1)], 1u);
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < BINS; b += kBlock) {
    uint32_t s = h[0][b] + h[1][b] + h[2][b] + h[3][b];
    if (s != 0) atomicAdd(ws + OFF + b, s);
  }
}

// ---- finish the select; on the tie path count the equals of T per chunk -------------------------------------------------
// chunk c = flat elements [c * CH, (c + 1) * CH); CH a multiple of 256 * VEC
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_finish(const float *__restrict__ W, Geo g, const uint2 *__restrict__ cut,
                                                   uint32_t *__restrict__ ws, uint32_t k, uint32_t CH) {
  __shared__ uint32_t sm[kWavesPerBlock], res[3];
  const uint32_t prefix = ws[kSt + 2], k2 = ws[kSt + 3];
  pick_bucket<kBins2>(ws + kH2, k2, sm, res);
  const uint32_t T = (prefix << kShift1) | res[0], n_eq = res[2], prune_eq = res[1];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ws[kSt + 4] = T;
    ws[kSt + 5] = k - prune_eq;
    ws[kSt + 6] = n_eq;
    ws[kSt + 7] = prune_eq;
  }
  if (prune_eq == 0 || prune_eq == n_eq) return;        // all or none of the equals go: no order needed
  const uint64_t lo = (uint64_t)blockIdx.x * CH;
  uint64_t hi = lo + CH;
  if (hi > g.total) hi = g.total;
  uint32_t n = 0;
  for (uint64_t e64 = lo + (uint64_t)threadIdx.x * VEC; e64 < hi; e64 += (uint64_t)kBlock * VEC) {
    uint32_t r, c;
    row_col(g, (uint32_t)e64, r, c);
    const float *p = W + (int64_t)r * g.ldw + c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      uint32_t key = __float_as_uint(p[i]) & kAbs;
      n += (key == T && !is_protected(cut, r, c + i, key)) ? 1u : 0u;
    }
  }
  uint32_t tot;
  block_excl_scan(n, sm, &tot);
  if (threadIdx.x == 0) ws[kChunk + blockIdx.x] = tot;
}

// ---- apply --------------------------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_apply(const float *W, Geo g, float *out, int64_t ldo,
                                                  const uint2 *__restrict__ cut, const uint32_t *__restrict__ ws,
                                                  uint32_t CH) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const uint32_t T = ws[kSt + 4], n_eq = ws[kSt + 6], prune_eq = ws[kSt + 7];
  const bool ties = prune_eq != 0 && prune_eq != n_eq;
  uint32_t rank0 = 0;                                    // equals of T in flat order before this chunk (tie path)
  if (ties) {
    uint32_t s = 0;
    for (uint32_t c = threadIdx.x; c < blockIdx.x; c += kBlock) s += ws[kChunk + c];
    uint32_t tot;
    block_excl_scan(s, sm, &tot);
    rank0 = tot;
  }
  const uint64_t lo = (uint64_t)blockIdx.x * CH;
  uint64_t hi = lo + CH;
  if (hi > g.total) hi = g.total;
  for (uint64_t t64 = lo; t64 < hi; t64 += (uint64_t)kBlock * VEC) {     // uniform trip count: barriers inside
    const uint64_t e64 = t64 + (uint64_t)threadIdx.x * VEC;
    const bool live = e64 < hi;
    uint32_t r = 0, c = 0;
    float v[VEC];
    uint32_t key[VEC];
    bool eq[VEC], prot[VEC];
    uint32_t neq = 0;
    if (live) {
      row_col(g, (uint32_t)e64, r, c);
      const float *p = W + (int64_t)r * g.ldw + c;
      if (VEC == 4) {
        float4 x = ld4(p);
        v[0] = x.x;
        v[1 % VEC] = x.y;
        v[2 % VEC] = x.z;
        v[3 % VEC] = x.w;
      } else {
        v[0] = *p;
      }
      uint2 q = make_uint2(0, 0);
      if (cut != nullptr) q = cut[r];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        key[i] = __float_as_uint(v[i]) & kAbs;
        prot[i] = cut != nullptr && (key[i] > q.x || (key[i] == q.x && c + i <= q.y));
        eq[i] = !prot[i] && key[i] == T;
        neq += eq[i] ? 1u : 0u;
      }
    }
    uint32_t rank = 0;
    if (ties) {
      uint32_t tot;
      rank = rank0 + block_excl_scan(neq, sm, &tot);
      rank0 += tot;
    }
    if (live) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        bool cutit;
        if (prot[i]) cutit = false;
        else if (eq[i]) {
          cutit = ties ? rank < prune_eq : prune_eq != 0;
          ++rank;
        } else cutit = key[i] < T;
        if (cutit) v[i] = 0.0f;
      }
      float *o = out + (int64_t)r * ldo + c;
      if (VEC == 4) st4(o, make_float4(v[0], v[1 % VEC], v[2 % VEC], v[3 % VEC]));
      else *o = v[0];
    }
  }
}

// ---- CSR ----------------------------------------------------------------------------------------------------------------
// csr workspace words: A[kMaxChunks] E[kMaxChunks] Ebase[kMaxChunks] NNZbase[kMaxChunks], then uint2 (a, e) per row.
constexpr int kCA = 0, kCE = kMaxChunks, kCEb = 2 * kMaxChunks, kCNb = 3 * kMaxChunks, kCsrHeadWords = 4 * kMaxChunks;

struct Sel {
  uint32_t T, prune_eq;
};
__device__ __forceinline__ Sel load_sel(const uint32_t *ws) {
  Sel s = {0u, 0u};
  if (ws != nullptr) {
    s.T = ws[kSt + 4];
    s.prune_eq = ws[kSt + 7];
  }
  return s;
}

// per row: a = non-zero elements that survive if no equal of T is pruned, e = unprotected equals of T
__global__ __launch_bounds__(kBlock) void k_csr_rowcount(const float *__restrict__ W, int64_t ldw, int64_t N, int D,
                                                         const uint2 *__restrict__ cut, const uint32_t *__restrict__ ws,
                                                         uint32_t *__restrict__ cw, uint2 *__restrict__ rowtmp,
                                                         int64_t RCH) {
  __shared__ uint32_t sa[kWavesPerBlock], se[kWavesPerBlock];
  const Sel s = load_sel(ws);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t lo = (int64_t)blockIdx.x * RCH;
  const int64_t hi = lo + RCH < N ? lo + RCH : N;
  uint32_t ta = 0, te = 0;
  for (int64_t row = lo + wave; row < hi; row += kWavesPerBlock) {
    uint32_t a = 0, e = 0;
    for (int c0 = 0; c0 < D; c0 += kWave) {
      const int c = c0 + lane;
      bool keep = false, eq = false;
      if (c < D) {
        const uint32_t key = __float_as_uint(W[row * ldw + c]) & kAbs;
        const bool prot = is_protected(cut, (uint32_t)row, (uint32_t)c, key);
        eq = !prot && key == s.T;
        keep = key != 0 && (prot || key >= s.T);
      }
      a += __popcll(__ballot(keep));
      e += __popcll(__ballot(eq));
    }
    if (lane == 0) rowtmp[row] = make_uint2(a, e);
    ta += a;
    te += e;
  }
  if (lane == 0) {
    sa[wave] = ta;
    se[wave] = te;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    cw[kCA + blockIdx.x] = sa[0] + sa[1] + sa[2] + sa[3];
    cw[kCE + blockIdx.x] = se[0] + se[1] + se[2] + se[3];
  }
}

__device__ __forceinline__ uint32_t pruned_equals(const Sel &s, uint32_t ebase, uint32_t e) {
  if (s.T == 0 || s.prune_eq <= ebase) return 0;        // equals of key 0 are zeros: never stored anyway
  uint32_t left = s.prune_eq - ebase;
  return left < e ? left : e;
}

// one workgroup: chunk totals -> chunk bases; crow[N] = number of stored elements
__global__ __launch_bounds__(kBlock) void k_csr_chunkscan(const uint32_t *__restrict__ ws, uint32_t *__restrict__ cw,
                                                          int nchunks, int64_t *__restrict__ crow, int64_t N) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const Sel s = load_sel(ws);
  uint32_t carry_e = 0, carry_n = 0;
  for (int c0 = 0; c0 < nchunks; c0 += kBlock) {
    const int c = c0 + threadIdx.x;
    const uint32_t a = c < nchunks ? cw[kCA + c] : 0u, e = c < nchunks ? cw[kCE + c] : 0u;
    uint32_t tot;
    const uint32_t eb = carry_e + block_excl_scan(e, sm, &tot);
    carry_e += tot;
    const uint32_t nn = a - pruned_equals(s, eb, e);
    const uint32_t nb = carry_n + block_excl_scan(nn, sm, &tot);
    carry_n += tot;
    if (c < nchunks) {
      cw[kCEb + c] = eb;
      cw[kCNb + c] = nb;
    }
  }
  if (threadIdx.x == 0) crow[N] = (int64_t)carry_n;
}

// rows of chunk c in order: crow[r], and rowtmp[r].y := equals of T in flat order before row r
__global__ __launch_bounds__(kBlock) void k_csr_rowscan(const uint32_t *__restrict__ ws, const uint32_t *__restrict__ cw,
                                                        uint2 *__restrict__ rowtmp, int64_t *__restrict__ crow, int64_t N,
                                                        int64_t RCH) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const Sel s = load_sel(ws);
  const int64_t lo = (int64_t)blockIdx.x * RCH;
  const int64_t hi = lo + RCH < N ? lo + RCH : N;
  uint32_t carry_e = cw[kCEb + blockIdx.x], carry_n = cw[kCNb + blockIdx.x];
  for (int64_t r0 = lo; r0 < hi; r0 += kBlock) {
    const int64_t r = r0 + threadIdx.x;
    uint2 ae = make_uint2(0, 0);
    if (r < hi) ae = rowtmp[r];
    uint32_t tot;
    const uint32_t eb = carry_e + block_excl_scan(ae.y, sm, &tot);
    carry_e += tot;
    const uint32_t nn = ae.x - pruned_equals(s, eb, ae.y);
    const uint32_t nb = carry_n + block_excl_scan(nn, sm, &tot);
    carry_n += tot;
    if (r < hi) {
      crow[r] = (int64_t)nb;
      rowtmp[r] = make_uint2(ae.x, eb);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_csr_fill(const float *__restrict__ W, int64_t ldw, int64_t N, int D,
                                                     const uint2 *__restrict__ cut, const uint32_t *__restrict__ ws,
                                                     const uint2 *__restrict__ rowtmp, const int64_t *__restrict__ crow,
                                                     int64_t *__restrict__ col, float *__restrict__ values) {
  const Sel s = load_sel(ws);
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t row = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); row < N; row += nwaves) {
    int64_t pos = crow[row];
    uint32_t erank = rowtmp[row].y;
    for (int c0 = 0; c0 < D; c0 += kWave) {
      const int c = c0 + lane;
      bool keep = false, eq = false;
      float w = 0.0f;
      if (c < D) {
        w = W[row * ldw + c];
        const uint32_t key = __float_as_uint(w) & kAbs;
        const bool prot = is_protected(cut, (uint32_t)row, (uint32_t)c, key);
        eq = !prot && key == s.T;
        keep = key != 0 && (prot || key >= s.T);
      }
      const uint64_t meq = __ballot(eq);
      if (eq && s.T != 0 && erank + (uint32_t)__popcll(meq & below) < s.prune_eq) keep = false;
      erank += __popcll(meq);
      const uint64_t mk = __ballot(keep);
      if (keep) {
        const int64_t o = pos + __popcll(mk & below);
        col[o] = c;
        values[o] = w;
      }
      pos += __popcll(mk);
    }
  }
}

int ilog2_or_neg(uint32_t d) {
  if ((d & (d - 1)) != 0) return -1;
  int s = 0;
  while ((1u << s) < d) ++s;
  return s;
}

// chunk length (flat elements) of the apply / tie passes: at most kMaxChunks chunks, a multiple of one workgroup tile
uint32_t chunk_len(uint64_t total, int vec) {
  const uint64_t tile = (uint64_t)kBlock * vec;
  uint64_t ch = (total + kMaxChunks - 1) / kMaxChunks;
  ch = (ch + tile - 1) / tile * tile;
  if (ch < tile) ch = tile;
  return (uint32_t)ch;
}

int64_t row_chunk(int64_t N) {
  int64_t r = (N + kMaxChunks - 1) / kMaxChunks;
  r = (r + kWave - 1) / kWave * kWave;
  return r < kWave ? kWave : r;
}

int table_check(const float *W, int64_t ldw, int64_t N, int32_t D) {
  if (W == nullptr || N < 1 || D < 1 || ldw < D || (uint64_t)N > 0xffffffffull / (uint64_t)D) return MI_ERR_INVALID_ARG;
  return D <= 1024 ? MI_OK : MI_ERR_UNSUPPORTED;
}

}  // namespace
}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_mag_prune_workspace_bytes(int64_t N) { return N < 0 ? 0 : kHeadBytes + 8 * N; }

int mi_mag_prune(const float *W, int64_t ldw, float *out, int64_t ldo, int64_t N, int32_t D, int64_t k, int32_t m,
                 void *workspace, void *stream) {
  if (int rc = table_check(W, ldw, N, D)) return rc;
  if (workspace == nullptr || k < 0 || m < 0 || m > D) return MI_ERR_INVALID_ARG;
  if (out != nullptr && ldo < D) return MI_ERR_INVALID_ARG;
  const uint64_t total = (uint64_t)N * D;
  if ((uint64_t)N * (uint64_t)m + (uint64_t)k > total) return MI_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  uint32_t *ws = (uint32_t *)workspace;
  uint2 *cut = m > 0 ? (uint2 *)((char *)workspace + kHeadBytes) : nullptr;
  if (hipMemsetAsync(ws, 0, (size_t)(kSt + kStWords) * 4, st) != hipSuccess) return MI_ERR_LAUNCH;
  if (m > 0) {
    const int rpw = (D <= 64 && (D & (D - 1)) == 0 && D >= 8) ? 64 / D : 1;
    const int grid = grid_for_waves((N + rpw - 1) / rpw);
    switch (rpw == 1 && D != 64 ? 0 : D) {
      case 8: MI_LAUNCH("mag_row_cut", k_row_cut_pow2<8>, grid, kBlock, st, W, ldw, N, (int)m, cut); break;
      case 16: MI_LAUNCH("mag_row_cut", k_row_cut_pow2<16>, grid, kBlock, st, W, ldw, N, (int)m, cut); break;
      case 32: MI_LAUNCH("mag_row_cut", k_row_cut_pow2<32>, grid, kBlock, st, W, ldw, N, (int)m, cut); break;
      case 64: MI_LAUNCH("mag_row_cut", k_row_cut_64, grid, kBlock, st, W, ldw, N, (int)m, cut); break;
      default: MI_LAUNCH("mag_row_cut", k_row_cut_any, grid, kBlock, st, W, ldw, N, (int)D, (int)m, cut); break;
    }
  }
  Geo g = {ldw, (uint32_t)total, (uint32_t)D, ilog2_or_neg((uint32_t)D)};
  const bool vec = D % 4 == 0 && ldw % 4 == 0 && aligned16(W) &&
                   (out == nullptr || (ldo % 4 == 0 && aligned16(out)));
  const int V = vec ? 4 : 1;
  int64_t tiles = ((int64_t)total + (int64_t)kBlock * V - 1) / ((int64_t)kBlock * V);
  int64_t hblocks = (tiles + kHistTilesPerBlock - 1) / kHistTilesPerBlock;
  const int hgrid = (int)(hblocks < kHistMaxGrid ? hblocks : kHistMaxGrid);
  const uint32_t CH = chunk_len(total, V);
  const int cgrid = (int)((total + CH - 1) / CH);
  const uint32_t k32 = (uint32_t)k;
  if (vec) {
    MI_LAUNCH("mag_hist0", (k_hist<0, 4>), hgrid, kBlock, st, W, g, cut, ws, k32);
    MI_LAUNCH("mag_hist1", (k_hist<1, 4>), hgrid, kBlock, st, W, g, cut, ws, k32);
    MI_LAUNCH("mag_hist2", (k_hist<2, 4>), hgrid, kBlock, st, W, g, cut, ws, k32);
    MI_LAUNCH("mag_finish", k_finish<4>, cgrid, kBlock, st, W, g, cut, ws, k32, CH);
    if (out != nullptr) MI_LAUNCH("mag_apply", k_apply<4>, cgrid, kBlock, st, W, g, out, ldo, cut, ws, CH);
  } else {
    MI_LAUNCH("mag_hist0", (k_hist<0, 1>), hgrid, kBlock, st, W, g, cut, ws, k32);
    MI_LAUNCH("mag_hist1", (k_hist<1, 1>), hgrid, kBlock, st, W, g, cut, ws, k32);
    MI_LAUNCH("mag_hist2", (k_hist<2, 1>), hgrid, kBlock, st, W, g, cut, ws, k32);
    MI_LAUNCH("mag_finish", k_finish<1>, cgrid, kBlock, st, W, g, cut, ws, k32, CH);
    if (out != nullptr) MI_LAUNCH("mag_apply", k_apply<1>, cgrid, kBlock, st, W, g, out, ldo, cut, ws, CH);
  }
  return launch_status();
}

int mi_mag_prune_result(const void *workspace, uint32_t *result4, void *stream) {
  if (workspace == nullptr || result4 == nullptr) return MI_ERR_INVALID_ARG;
  if (hipMemcpyAsync(result4, (const uint32_t *)workspace + kSt + 4, 16, hipMemcpyDeviceToDevice,
                     (hipStream_t)stream) != hipSuccess)
    return MI_ERR_LAUNCH;
  return MI_OK;
}

int64_t mi_mag_csr_workspace_bytes(int64_t N) { return N < 0 ? 0 : (int64_t)kCsrHeadWords * 4 + 8 * N; }

int mi_mag_csr_count(const float *W, int64_t ldw, int64_t N, int32_t D, const void *prune_ws, int32_t m,
                     void *csr_ws, int64_t *crow, void *stream) {
  if (int rc = table_check(W, ldw, N, D)) return rc;
  if (csr_ws == nullptr || crow == nullptr || m < 0 || (prune_ws == nullptr && m != 0))
    return MI_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t *ws = (const uint32_t *)prune_ws;
  const uint2 *cut = m > 0 ? (const uint2 *)((const char *)prune_ws + kHeadBytes) : nullptr;
  uint32_t *cw = (uint32_t *)csr_ws;
  uint2 *rowtmp = (uint2 *)(cw + kCsrHeadWords);
  const int64_t RCH = row_chunk(N);
  const int nchunks = (int)((N + RCH - 1) / RCH);
  MI_LAUNCH("mag_csr_rowcount", k_csr_rowcount, nchunks, kBlock, st, W, ldw, N, (int)D, cut, ws, cw, rowtmp, RCH);
  MI_LAUNCH("mag_csr_chunkscan", k_csr_chunkscan, 1, kBlock, st, ws, cw, nchunks, crow, N);
  MI_LAUNCH("mag_csr_rowscan", k_csr_rowscan, nchunks, kBlock, st, ws, (const uint32_t *)cw, rowtmp, crow, N, RCH);
  return launch_status();
}

int mi_mag_csr_fill(const float *W, int64_t ldw, int64_t N, int32_t D, const void *prune_ws, int32_t m,
                    const void *csr_ws, const int64_t *crow, int64_t *col, float *values, void *stream) {
  if (int rc = table_check(W, ldw, N, D)) return rc;
  if (csr_ws == nullptr || crow == nullptr || m < 0 || (prune_ws == nullptr && m != 0))
    return MI_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t *ws = (const uint32_t *)prune_ws;
  const uint2 *cut = m > 0 ? (const uint2 *)((const char *)prune_ws + kHeadBytes) : nullptr;
  const uint2 *rowtmp = (const uint2 *)((const uint32_t *)csr_ws + kCsrHeadWords);
  MI_LAUNCH("mag_csr_fill", k_csr_fill, grid_for_waves(N), kBlock, st, W, ldw, N, (int)D, cut, ws, rowtmp, crow, col,
            values);
  return launch_status();
}

}  // extern "C"
