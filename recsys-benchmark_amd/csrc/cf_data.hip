// cf_data.hip — the two ends of a collaborative-filtering loop on the device: the epoch's (user, positive, K negatives)
// triples (reference: CFGraphDataset.__getitem__ / _sample_negative / _get_uniform, src/dataset/cf_graph_dataset.py:
// 128-168) and NDCG / recall per user (get_ndcg_recall, src/metrics.py:70-108).
//
// Sampler.  One thread per sample, no loop whose trip count depends on a draw.  The reference rejects candidates until
// one is outside the user's items and outside the earlier picks; the law of that loop is "uniform over the items the
// user has not interacted with, the K of a sample pairwise distinct", and that law is drawn directly here:
//   t-th negative: a rank r uniform in [0, num_items - deg - t) among the non-positives not picked yet,
//   bumped past the earlier picks (their ranks, kept ascending in registers: r += 1 for every earlier rank <= r, in
//   ascending order), then mapped to its item by ONE binary search over g(j) = pos_col[j] - j, which is non-decreasing
//   for a distinct ascending row: item = r + j for the smallest j in [0, deg] with g(j) > r (j = deg when none is).
// At most K * ceil(log2(deg + 1)) reads of pos_col per sample, whatever share of the items the user holds.
//
// Random numbers are counter-based and stateless (mix64 = the splitmix64 finaliser the library uses elsewhere):
//   base       = mix64(seed + 0x9E3779B97F4A7C15 * (epoch + 1))
//   key(i)     = mix64(base + 0xD1B54A32D192ED03 * (i + 1))              i = the sample's index in the EPOCH
//   bits(i, d) = mix64(key(i) + 0x9E3779B97F4A7C15 * (d + 1))            d = 0: the positive; d = 1 + t: negative t
//   value      = high 64 bits of bits(i, d) * range                     (all of it modulo 2^64)
// so a sub-range of an epoch holds the bits the whole epoch holds there, for any grid.  The multiply-high reduction is
// biased by at most range / 2^64 per value (< 2^-33 for ranges below 2^31): accepted.
//
// Stores are plain vector stores; the only atomic is the OR into the error word, on the error path.  A sample that
// cannot be drawn (pair index or user out of range, no stored item, deg + K > num_items) writes -1 to its outputs and
// reads nothing further: every subscript below is checked against the array lengths the caller passed.
#include "common.hpp"

namespace {
using namespace mi;

constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kSalt = 0xD1B54A32D192ED03ull;

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t draw(uint64_t key, uint64_t d, uint64_t range) {
  return __umul64hi(mix64(key + kGold * (d + 1)), range);
}

struct SampleArgs {
  const int64_t *pair_user, *pair_item, *pair_crow, *pos_crow;
  const int32_t *pos_col;
  const int64_t *order;
  int64_t P, pos_nnz, U, num_items, per_user_num, first, n;
  uint64_t base;
  int mode, K;
  int64_t *users, *pos, *neg;
  int *err;
};

// KCAP: the capacity of the sorted rank array (K <= KCAP); every index into it is a compile-time constant, so it
// stays in registers (a runtime subscript would send it to scratch).
template <int KCAP>
__global__ __launch_bounds__(kBlock) void k_sample_triples(SampleArgs a) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
    const uint64_t key = mix64(a.base + kSalt * ((uint64_t)(a.first + i) + 1));
    int64_t u = -1, item = -1;
    if (a.mode == MI_CF_SAMPLE_POPULARITY) {
      const int64_t p = a.order ? a.order[i] : a.first + i;
      if (p >= 0 && p < a.P) {
        u = a.pair_user[p];
        item = a.pair_item[p];
      }
    } else {
      u = (a.first + i) / a.per_user_num;
      if (u < a.U) {
        const int64_t s0 = a.pair_crow[u], s1 = a.pair_crow[u + 1];
        if (s0 >= 0 && s1 > s0 && s1 <= a.P) item = a.pair_item[s0 + (int64_t)draw(key, 0, (uint64_t)(s1 - s0))];
      }
    }
    bool ok = u >= 0 && u < a.U && item >= 0;
    int64_t c0 = 0, deg = 0;
    if (ok) {
      c0 = a.pos_crow[u];
      deg = a.pos_crow[u + 1] - c0;
      ok = c0 >= 0 && deg >= 0 && c0 + deg <= a.pos_nnz && deg + a.K <= a.num_items;
    }
    a.users[i] = ok ? u : -1;
    a.pos[i] = ok ? item : -1;
    if (!ok) {
      for (int t = 0; t < a.K; ++t) a.neg[(int64_t)t * a.n + i] = -1;
      if (a.err) atomicOr(a.err, MI_IDX_OUT_OF_RANGE);
      continue;
    }
    const int32_t *row = a.pos_col + c0;
    const int32_t d32 = (int32_t)deg;
    const int32_t free_items = (int32_t)(a.num_items - deg);
    int32_t picked[KCAP];
    for (int t = 0; t < a.K; ++t) {
      int32_t r = (int32_t)draw(key, 1 + t, (uint64_t)(free_items - t));
      if (KCAP > 1) {
#pragma unroll
        for (int j = 0; j < KCAP; ++j)
          if (j < t && r >= picked[j]) ++r;
        int32_t carry = r;                       // insert, keeping picked[0..t] ascending
#pragma unroll
        for (int j = 0; j < KCAP; ++j) {
          if (j < t) {
            if (picked[j] > carry) {
              const int32_t x = picked[j];
              picked[j] = carry;
              carry = x;
            }
          } else if (j == t) {
            picked[j] = carry;
          }
        }
      }
      int32_t lo = 0, hi = d32;                  // smallest j with row[j] - j > r
      while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (row[mid] - mid > r) hi = mid; else lo = mid + 1;
      }
      a.neg[(int64_t)t * a.n + i] = (int64_t)r + lo;
    }
  }
}

// One thread per row of pred: k binary searches in the user's truth row, DCG in ascending j.
__global__ __launch_bounds__(kBlock) void k_ndcg_recall_rows(const int64_t *__restrict__ pred, int64_t ld,
                                                             const int64_t *__restrict__ users, int64_t n, int k,
                                                             const int64_t *__restrict__ crow,
                                                             const int64_t *__restrict__ col, int64_t U, int64_t nnz,
                                                             const double *__restrict__ weight,
                                                             const double *__restrict__ ideal, double *__restrict__ ndcg,
                                                             double *__restrict__ recall, int *err) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int64_t u = users[i];
    int64_t c0 = 0, len = -1;
    if (u >= 0 && u < U) {
      c0 = crow[u];
      len = crow[u + 1] - c0;
      if (c0 < 0 || len < 0 || c0 + len > nnz) len = -1;
    }
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (len <= 0) {                              // 0: the reference's 0 / 0; < 0: no such user
      ndcg[i] = nan;
      recall[i] = nan;
      if (len < 0 && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
      continue;
    }
    const int64_t *row = col + c0;
    double dcg = 0.0;
    int hits = 0;
    for (int j = 0; j < k; ++j) {
      const int64_t v = pred[i * ld + j];
      int64_t lo = 0, hi = len;                  // first entry >= v
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row[mid] < v) lo = mid + 1; else hi = mid;
      }
      if (lo < len && row[lo] == v) {
        dcg += weight[j];
        ++hits;
      }
    }
    const int64_t length = len < k ? len : k;
    ndcg[i] = dcg / ideal[length - 1];
    recall[i] = (double)hits / (double)length;
  }
}

inline int grid_for_threads(int64_t n) {
  int64_t g = (n + kBlock - 1) / kBlock;
  return (int)(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));
}

}  // namespace

extern "C" {

int mi_cf_sample_triples(const int64_t *pair_user, const int64_t *pair_item, const int64_t *pair_crow, int64_t P,
                         const int64_t *pos_crow, const int32_t *pos_col, int64_t pos_nnz, int64_t U, int64_t num_items,
                         int32_t mode, int64_t per_user_num, int32_t K, const int64_t *order, int64_t seed, int64_t epoch,
                         int64_t first, int64_t n, int64_t *users, int64_t *pos, int64_t *neg, int *err, void *stream) {
  if (mode != MI_CF_SAMPLE_UNIFORM && mode != MI_CF_SAMPLE_POPULARITY) return MI_ERR_INVALID_ARG;
  if (P < 0 || pos_nnz < 0 || U < 0 || num_items < 0 || K < 1 || first < 0 || n < 0) return MI_ERR_INVALID_ARG;
  if (K > MI_CF_MAX_NEG || num_items > INT32_MAX) return MI_ERR_UNSUPPORTED;
  if (n == 0) return MI_OK;
  if (!pair_item || !pos_crow || !users || !pos || !neg) return MI_ERR_INVALID_ARG;
  if (pos_nnz > 0 && !pos_col) return MI_ERR_INVALID_ARG;
  if (mode == MI_CF_SAMPLE_POPULARITY ? !pair_user : (!pair_crow || per_user_num < 1)) return MI_ERR_INVALID_ARG;
  SampleArgs a;
  a.pair_user = pair_user; a.pair_item = pair_item; a.pair_crow = pair_crow; a.pos_crow = pos_crow; a.pos_col = pos_col;
  a.order = mode == MI_CF_SAMPLE_POPULARITY ? order : nullptr;
  a.P = P; a.pos_nnz = pos_nnz; a.U = U; a.num_items = num_items; a.per_user_num = per_user_num; a.first = first; a.n = n;
  a.base = mix64((uint64_t)seed + kGold * ((uint64_t)epoch + 1));
  a.mode = mode; a.K = K;
  a.users = users; a.pos = pos; a.neg = neg; a.err = err;
  const int grid = grid_for_threads(n);
  if (K == 1) MI_LAUNCH("cf_sample_triples", k_sample_triples<1>, grid, kBlock, stream, a);
  else if (K <= 8) MI_LAUNCH("cf_sample_triples", k_sample_triples<8>, grid, kBlock, stream, a);
  else MI_LAUNCH("cf_sample_triples", k_sample_triples<MI_CF_MAX_NEG>, grid, kBlock, stream, a);
  return launch_status();
}

int mi_ndcg_recall_rows(const int64_t *pred, int64_t ld, const int64_t *users, int64_t n, int32_t k, const int64_t *crow,
                        const int64_t *col, int64_t U, int64_t nnz, const double *weight, const double *ideal,
                        double *ndcg, double *recall, int *err, void *stream) {
  if (n < 0 || k < 1 || ld < k || U < 0 || nnz < 0) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!pred || !users || !crow || !weight || !ideal || !ndcg || !recall || (nnz > 0 && !col)) return MI_ERR_INVALID_ARG;
  MI_LAUNCH("ndcg_recall_rows", k_ndcg_recall_rows, grid_for_threads(n), kBlock, stream, pred, ld, users, n, (int)k, crow,
            col, U, nnz, weight, ideal, ndcg, recall, err);
  return launch_status();
}

}  // extern "C"
