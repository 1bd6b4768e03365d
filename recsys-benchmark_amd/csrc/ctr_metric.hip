// ctr_metric.hip — the CTR validation metric on the device (src/trainer/deepfm.py:96-139 `validate_epoch`:
// sklearn.metrics.roc_auc_score and log_loss over the whole validation set).
//
//   AUC   = S / (2 P N),  S = sum over the positives p of  #{negatives below p} + #{negatives not above p}
//           (= sum over groups of equal score of pos_g * (2 * neg_below_g + neg_g): the Mann-Whitney statistic with ties
//           sharing their average rank, doubled so that it is an integer)
//   key   = monotone map of the float32 bits, -0.0 folded onto +0.0; +-inf ordinary; NaN counted, outside the order
//   sort  = stable least-significant-digit radix sort of the NEGATIVES' keys, 4 passes of 8 bits; a positive travels as
//           the key 0xffffffff (above every ordinary key), so the sorted negatives are the first N words and the sort
//           needs no compaction and no label payload.  Per pass: per-tile digit counts (LDS integer adds) -> one
//           workgroup per digit scans its row of tile counts -> scatter with a stable in-tile rank (digit match by
//           ballots inside a wave, wave-private LDS counters across a wave's rounds, waves in order)
//   count = every positive does a lower- and an upper-bound search in the sorted negatives; integer sums per workgroup,
//           one 64-bit integer global add each: no float atomics, nothing depends on the order of arrival
//   append= one launch per validation batch: logits and label bytes into the epoch buffers, the batch's
//           BCE-with-logits sum (float64 terms, block partials joined by the last workgroup in index order) onto a
//           device double
#include "common.hpp"

namespace mi {
namespace {

constexpr int kDigits = 256, kDigitBits = 8, kPasses = 4;
constexpr int kItems = 4;                                 // keys per thread and tile
constexpr int kTile = kBlock * kItems;                    // 1024 keys per workgroup
constexpr uint32_t kPosKey = 0xffffffffu;                 // what a positive (or a label outside {0, 1}) sorts as
constexpr int kCountMaxGrid = 2048;
constexpr int kAppendMaxGrid = 1024;

struct Rec {                    // mi_binary_auc's result record (48 bytes)
  unsigned long long S;
  unsigned long long P, N, n_nan, n_bad;
  double auc;
};

__device__ __forceinline__ uint32_t score_key(float s, bool *nan) {
  uint32_t b = __float_as_uint(s);
  *nan = (b & 0x7fffffffu) > 0x7f800000u;
  if ((b << 1) == 0) b = 0;                                // -0.0 == +0.0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

inline int64_t pad16(int64_t bytes) { return (bytes + 15) / 16 * 16; }
inline int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

// ---- per-tile digit counts: hist[digit * T + tile] ---------------------------------------------------------------------
// FIRST: the keys are made here from (score, label), written to keys_out, and P / N / NaN / bad labels are counted.
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void k_auc_hist(const float *__restrict__ score, const uint8_t *__restrict__ label,
                                                     const uint32_t *__restrict__ keys_in, uint32_t *__restrict__ keys_out,
                                                     int64_t n, int64_t T, int shift, uint32_t *__restrict__ hist,
                                                     Rec *__restrict__ rec) {
  __shared__ uint32_t h[kDigits];
  __shared__ uint32_t cnt[kWavesPerBlock][4];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kTile;
  uint32_t c_pos = 0, c_neg = 0, c_nan = 0, c_bad = 0;     // wave-uniform
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + r * kBlock + threadIdx.x;
    const bool live = i < n;
    uint32_t key = 0;
    bool pos = false, neg = false, nan = false, bad = false;
    if (live) {
      if (FIRST) {
        const uint8_t y = label[i];
        key = score_key(score[i], &nan);
        pos = y == 1;
        neg = y == 0;
        bad = y > 1;
        if (!neg) key = kPosKey;
        keys_out[i] = key;
      } else {
        key = keys_in[i];
      }
      atomicAdd(&h[(key >> shift) & (kDigits - 1)], 1u);
    }
    if (FIRST) {
      c_pos += __popcll(__ballot(pos));
      c_neg += __popcll(__ballot(neg));
      c_nan += __popcll(__ballot(nan));
      c_bad += __popcll(__ballot(bad));
    }
  }
  if (FIRST && (threadIdx.x & (kWave - 1)) == 0) {
    uint32_t *c = cnt[threadIdx.x >> 6];
    c[0] = c_pos;
    c[1] = c_neg;
    c[2] = c_nan;
    c[3] = c_bad;
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * T + blockIdx.x] = h[threadIdx.x];
  if (FIRST && threadIdx.x < 4) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) s += cnt[w][threadIdx.x];
    unsigned long long *dst = threadIdx.x == 0 ? &rec->P : (threadIdx.x == 1 ? &rec->N : (threadIdx.x == 2 ? &rec->n_nan : &rec->n_bad));
    if (s != 0) atomicAdd(dst, (unsigned long long)s);
  }
}

// one workgroup per digit: its row of T tile counts becomes their exclusive running sum, tot[digit] = the row's sum
__global__ __launch_bounds__(kBlock) void k_auc_scan(uint32_t *__restrict__ hist, int64_t T, uint32_t *__restrict__ tot) {
  __shared__ uint32_t sm[kWavesPerBlock];
  uint32_t *row = hist + (int64_t)blockIdx.x * T;
  uint32_t carry = 0;
  for (int64_t t0 = 0; t0 < T; t0 += kBlock * 4) {        // uniform trip count: barriers inside
    const int64_t t = t0 + (int64_t)threadIdx.x * 4;
    uint32_t v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = t + j < T ? row[t + j] : 0u;
      s += v[j];
    }
    uint32_t total;
    uint32_t ex = carry + block_excl_scan(s, sm, &total);
    carry += total;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (t + j < T) row[t + j] = ex;
      ex += v[j];
    }
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// stable scatter of one tile.  Order inside the tile = (wave, round, lane), which is the order of the input index.
__global__ __launch_bounds__(kBlock) void k_auc_scatter(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, int64_t n,
                                                        int64_t T, int shift, const uint32_t *__restrict__ hist,
                                                        const uint32_t *__restrict__ tot) {
  __shared__ uint32_t cnt[kWavesPerBlock][kDigits];
  __shared__ uint32_t sm[kWavesPerBlock];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
#pragma unroll
  for (int w = 0; w < kWavesPerBlock; ++w) cnt[w][threadIdx.x] = 0;
  uint32_t all;
  const uint32_t dbase = block_excl_scan(tot[threadIdx.x], sm, &all);     // keys of lower digits, all tiles (barriers inside)
  const int64_t base = (int64_t)blockIdx.x * kTile + wave * (kItems * kWave);
  uint32_t key[kItems], loc[kItems];
  bool live[kItems];
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    const int64_t i = base + r * kWave + lane;
    live[r] = i < n;
    key[r] = live[r] ? in[i] : 0u;
    const uint32_t d = (key[r] >> shift) & (kDigits - 1);
    uint64_t peers = __ballot(live[r]);                     // live lanes of this wave with my digit
#pragma unroll
    for (int b = 0; b < kDigitBits; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    // cnt[wave] is touched by this wave only, and a wave's LDS instructions complete in program order: the round's reads
    // come before its one write per digit, that write before the next round's reads.  The fences keep the compiler from
    // moving them across each other; no workgroup barrier is needed until the waves read each other's counters.
    const uint32_t pre = cnt[wave][d];                      // my digit in this wave's earlier rounds
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    loc[r] = pre + (uint32_t)__popcll(peers & below);
    if (live[r] && (peers & below) == 0) cnt[wave][d] = pre + (uint32_t)__popcll(peers);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {  // thread = digit: the waves' counts become the waves' first output positions
    uint32_t run = dbase + hist[(int64_t)threadIdx.x * T + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) {
      const uint32_t c = cnt[w][threadIdx.x];
      cnt[w][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kItems; ++r) {
    if (live[r]) {
      const int64_t o = (int64_t)cnt[wave][(key[r] >> shift) & (kDigits - 1)] + loc[r];
      if (o < n) out[o] = key[r];                           // (always true for counts made from these keys)
    }
  }
}

// #{sorted[0, N) < key} + #{sorted[0, N) <= key}: the lower- and the upper-bound search side by side, so that their two
// loads per step are in flight together and the lanes of a wave keep one trip count (a walk shared until a probe hits an
// equal of key, then two searches, was measured: 17 % faster on distinct scores, 54 % slower on 1 000 levels, where every
// lane leaves the shared walk at another step)
__device__ __forceinline__ int64_t rank_sum(const uint32_t *__restrict__ sorted, int64_t N, uint32_t key) {
  int64_t lo1 = 0, hi1 = N, lo2 = 0, hi2 = N;
  while (lo1 < hi1 || lo2 < hi2) {
    const bool go1 = lo1 < hi1, go2 = lo2 < hi2;
    const int64_t m1 = lo1 + ((hi1 - lo1) >> 1), m2 = lo2 + ((hi2 - lo2) >> 1);
    const uint32_t v1 = go1 ? sorted[m1] : 0u, v2 = go2 ? sorted[m2] : 0u;
    if (go1) {
      if (v1 < key) lo1 = m1 + 1;
      else hi1 = m1;
    }
    if (go2) {
      if (v2 <= key) lo2 = m2 + 1;
      else hi2 = m2;
    }
  }
  return lo1 + lo2;
}

__global__ __launch_bounds__(kBlock) void k_auc_count(const float *__restrict__ score, const uint8_t *__restrict__ label, int64_t n,
                                                      const uint32_t *__restrict__ sorted, Rec *rec) {
  __shared__ unsigned long long red[kWavesPerBlock];
  int64_t N = (int64_t)rec->N;                             // finished by the first launch
  if (N > n) N = n;
  unsigned long long s = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    if (label[i] != 1) continue;
    bool nan;
    const uint32_t key = score_key(score[i], &nan);
    if (nan) continue;
    s += (unsigned long long)rank_sum(sorted, N, key);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = red[0] + red[1] + red[2] + red[3];
    if (s != 0) atomicAdd(&rec->S, s);
  }
}

__global__ void k_auc_final(Rec *rec) {
  const unsigned long long P = rec->P, N = rec->N;
  double auc = __longlong_as_double(0x7ff8000000000000ll);
  if (rec->n_nan == 0 && P != 0 && N != 0) auc = (double)rec->S / (double)(2ull * P * N);
  rec->auc = auc;
}

// ---- append ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// v summed over the workgroup in a fixed tree (wave sums, then thread 0 adds the waves in order); valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double *red) {
  v = wave_sum_f64(v);
  __syncthreads();                                          // red may still be read from an earlier call
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = 0.0;
    for (int w = 0; w < kWavesPerBlock; ++w) v += red[w];
  }
  return v;
}

// ws: part double[kAppendMaxGrid], then the arrival ticket (zero on entry, zero again on exit) — grid_join of common.hpp
// in float64
template <class L>
__global__ __launch_bounds__(kBlock) void k_ctr_append(const float *__restrict__ logit, const L *__restrict__ lab, int64_t b,
                                                       float *__restrict__ score, uint8_t *__restrict__ lbl,
                                                       double *loss_sum, double *part, unsigned *ticket) {
  __shared__ double red[kWavesPerBlock];
  __shared__ bool last;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < b; i += (int64_t)gridDim.x * kBlock) {
    const float x = logit[i];
    const L y = lab[i];
    score[i] = x;
    lbl[i] = y == (L)1 ? 1 : (y == (L)0 ? 0 : 2);
    const double xd = (double)x, yd = (double)y;
    acc += fmax(xd, 0.0) - xd * yd + log1p(exp(-fabs(xd)));
  }
  double v = block_sum_f64(acc, red);
  if (threadIdx.x == 0) {
    __hip_atomic_store(part + blockIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  v = 0.0;
  for (unsigned j = threadIdx.x; j < gridDim.x; j += kBlock)
    v += __hip_atomic_load(part + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  v = block_sum_f64(v, red);
  if (threadIdx.x == 0) {
    *loss_sum += v;
    *ticket = 0;
  }
}

}  // namespace
}  // namespace mi

using namespace mi;

extern "C" {

int64_t mi_binary_auc_workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return 2 * pad16(4 * n) + pad16(4 * (int64_t)kDigits * tiles_of(n)) + 4 * kDigits;
}

int mi_binary_auc(const float *score, const uint8_t *label, int64_t n, void *workspace, void *result, void *stream) {
  if (result == nullptr || n < 0) return MI_ERR_INVALID_ARG;
  if (n > 0 && (score == nullptr || label == nullptr || workspace == nullptr)) return MI_ERR_INVALID_ARG;
  if (n > 0x7fffffffll) return MI_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Rec *rec = (Rec *)result;
  if (hipMemsetAsync(rec, 0, sizeof(Rec), st) != hipSuccess) return MI_ERR_LAUNCH;
  if (n > 0) {
    const int64_t T = tiles_of(n);
    uint32_t *a = (uint32_t *)workspace;
    uint32_t *b = (uint32_t *)((char *)workspace + pad16(4 * n));
    uint32_t *hist = (uint32_t *)((char *)workspace + 2 * pad16(4 * n));
    uint32_t *tot = hist + pad16(4 * (int64_t)kDigits * T) / 4;
    const int grid = (int)T;
    for (int p = 0; p < kPasses; ++p) {                      // a -> b -> a -> b -> a
      const int shift = p * kDigitBits;
      if (p == 0)
        MI_LAUNCH("auc_hist_first", k_auc_hist<true>, grid, kBlock, st, score, label, (const uint32_t *)nullptr, a, n, T,
                  shift, hist, rec);
      else
        MI_LAUNCH("auc_hist", k_auc_hist<false>, grid, kBlock, st, (const float *)nullptr, (const uint8_t *)nullptr,
                  (const uint32_t *)a, (uint32_t *)nullptr, n, T, shift, hist, rec);
      MI_LAUNCH("auc_scan", k_auc_scan, kDigits, kBlock, st, hist, T, tot);
      MI_LAUNCH("auc_scatter", k_auc_scatter, grid, kBlock, st, (const uint32_t *)a, b, n, T, shift, (const uint32_t *)hist,
                (const uint32_t *)tot);
      uint32_t *t = a;
      a = b;
      b = t;
    }
    int64_t cgrid = (n + kBlock - 1) / kBlock;
    if (cgrid > kCountMaxGrid) cgrid = kCountMaxGrid;
    MI_LAUNCH("auc_count", k_auc_count, (int)cgrid, kBlock, st, score, label, n, (const uint32_t *)a, rec);
  }
  MI_LAUNCH("auc_final", k_auc_final, 1, 1, st, rec);
  return launch_status();
}

int64_t mi_ctr_metric_append_workspace_bytes(void) { return 8 * (int64_t)kAppendMaxGrid + 16; }

int mi_ctr_metric_append(const float *logits, const void *labels, int32_t label_kind, int64_t b, int64_t at, float *score_buf,
                         uint8_t *label_buf, int64_t cap, double *loss_sum, void *workspace, void *stream) {
  if (b < 0 || at < 0 || cap < 0 || at > cap || b > cap - at) return MI_ERR_INVALID_ARG;
  if (label_kind != MI_CTR_LABEL_INT64 && label_kind != MI_CTR_LABEL_FLOAT32) return MI_ERR_INVALID_ARG;
  if (b == 0) return MI_OK;
  if (logits == nullptr || labels == nullptr || score_buf == nullptr || label_buf == nullptr || loss_sum == nullptr ||
      workspace == nullptr)
    return MI_ERR_INVALID_ARG;
  int64_t grid = (b + kBlock - 1) / kBlock;
  if (grid > kAppendMaxGrid) grid = kAppendMaxGrid;
  double *part = (double *)workspace;
  unsigned *ticket = (unsigned *)(part + kAppendMaxGrid);
  if (label_kind == MI_CTR_LABEL_INT64)
    MI_LAUNCH("ctr_append", k_ctr_append<int64_t>, (int)grid, kBlock, stream, logits, (const int64_t *)labels, b, score_buf + at,
              label_buf + at, loss_sum, part, ticket);
  else
    MI_LAUNCH("ctr_append", k_ctr_append<float>, (int)grid, kBlock, stream, logits, (const float *)labels, b, score_buf + at,
              label_buf + at, loss_sum, part, ticket);
  return launch_status();
}

}  // extern "C"
