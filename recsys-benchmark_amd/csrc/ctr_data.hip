// ctr_data.hip — click-through data on the device: the vocabulary rule of the reference's Criteo dataset
// (__get_feat_mapper / __yield_buffer, src/dataset/criteo/criteo_torchfm.py:114-161) over one SORTED column, and the
// (x, y) batch a DataLoader would have collated, read from the resident uint32 [n, 1 + F] record array in one launch.
//
// Vocabulary (mi_ctr_vocab_field).  The caller sorts the column's int64 keys (stable) and hands over the sorted keys and
// the permutation.  A key seen at least `threshold` times is kept; kept keys are numbered 0 .. kept-1 in ascending key
// order, every other key gets the id `kept`.  Three launches, integer adds only, plain vector stores:
//   mark     element i finds how far its run of equal keys reaches on either side, by two binary searches inside the
//            window [i - (T-1), i + (T-1)] (a run is kept exactly when back + forward + 1 >= T, so nothing outside that
//            window matters and a run of millions costs what a run of T costs); it writes one flag byte
//            (bit 0: run kept, bit 1: i is its run's head) and the tile's number of kept heads;
//   scan     one workgroup turns the tiles' counts into exclusive offsets (block_excl_scan with a carry) and writes the
//            total, num_kept, to the caller's device word;
//   scatter  the kept heads at or before i, less one, is the id of a kept element (its own head is the latest of them);
//            out[perm[i] * stride] = kept ? id : num_kept.
// No arrival order enters any value: reruns give the same bits.
//
// Batch (mi_ctr_batch).  One lane per output element, flat over count * (1 + F), so the lanes of a record read
// consecutive dwords (the record stride, 4 (1 + F) bytes, is in general no multiple of 8: dword loads).  The sample at
// epoch position j is record row index[p(j)] (p(j) without an index); p is the identity, or the keyed bijection of
// [0, n) spelled out in include/mi355x_recsys.h: a six-round Feistel network over 2k bits walked until it lands below
// n.  Every lane of a record walks the same p(j): redundant integer work, no cross-lane traffic, no second launch.
//
// The only atomic is the OR into the error word, on the error path; every subscript is checked against the lengths the
// caller passed before it is used.
#include "common.hpp"

namespace {
using namespace mi;

constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kSalt = 0xD1B54A32D192ED03ull;
constexpr int kRounds = 6;

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {        // the splitmix64 finaliser, as in cf_data.hip
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

constexpr uint8_t kKept = 1, kHead = 2;

inline int64_t tiles_of(int64_t n) { return (n + kBlock - 1) / kBlock; }
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

inline int grid_for_tiles(int64_t tiles) { return (int)(tiles < 1 ? 1 : (tiles > kMaxGrid ? kMaxGrid : tiles)); }

// T is in [1, n + 1] (the entry point clamps it), so i + (T - 1) cannot overflow.
__global__ __launch_bounds__(kBlock) void k_vocab_mark(const int64_t *__restrict__ keys, int64_t n, int64_t T,
                                                       uint8_t *__restrict__ flags, uint32_t *__restrict__ tile_sums) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const int64_t tiles = (n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i = t * kBlock + threadIdx.x;
    uint32_t kept_head = 0;
    if (i < n) {
      const int64_t key = keys[i];
      const bool head = i == 0 || keys[i - 1] != key;
      int64_t lo = i - (T - 1) < 0 ? 0 : i - (T - 1), hi = i;          // lowest j in the window with keys[j] == key
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] == key) hi = mid; else lo = mid + 1;
      }
      const int64_t back = i - lo;
      lo = i;                                                           // highest j in the window with keys[j] == key
      hi = i + (T - 1) > n - 1 ? n - 1 : i + (T - 1);
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (keys[mid] == key) lo = mid; else hi = mid - 1;
      }
      const bool kept = back + (lo - i) + 1 >= T;
      flags[i] = (uint8_t)((kept ? kKept : 0) | (head ? kHead : 0));
      kept_head = kept && head;
    }
    uint32_t total;
    block_excl_scan(kept_head, sm, &total);
    if (threadIdx.x == 0) tile_sums[t] = total;
  }
}

// one workgroup: tile_sums becomes the exclusive scan of itself, *num_kept the total
__global__ __launch_bounds__(kBlock) void k_vocab_scan_tiles(uint32_t *__restrict__ tile_sums, int64_t tiles,
                                                             int64_t *__restrict__ num_kept) {
  __shared__ uint32_t sm[kWavesPerBlock];
  uint32_t carry = 0;
  for (int64_t base = 0; base < tiles; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < tiles ? tile_sums[i] : 0u;
    uint32_t total;
    const uint32_t before = block_excl_scan(v, sm, &total);
    if (i < tiles) tile_sums[i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) *num_kept = (int64_t)carry;
}

__global__ __launch_bounds__(kBlock) void k_vocab_scatter(const uint8_t *__restrict__ flags, const int64_t *__restrict__ perm,
                                                          int64_t n, const uint32_t *__restrict__ tile_off,
                                                          const int64_t *__restrict__ num_kept, uint32_t *__restrict__ out,
                                                          int64_t stride, int *err) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const int64_t tiles = (n + kBlock - 1) / kBlock;
  const uint32_t oov = (uint32_t)*num_kept;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i = t * kBlock + threadIdx.x;
    const uint8_t f = i < n ? flags[i] : (uint8_t)0;
    const uint32_t kept_head = f == (kKept | kHead);
    uint32_t total;
    const uint32_t before = block_excl_scan(kept_head, sm, &total);
    if (i < n) {
      const uint32_t id = (f & kKept) ? tile_off[t] + before + kept_head - 1u : oov;
      const int64_t p = perm[i];
      if (p >= 0 && p < n) out[p * stride] = id;
      else if (err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
    }
  }
}

struct BatchArgs {
  const uint32_t *records;
  const int64_t *index;
  int64_t n_records, n, first, count;
  uint64_t key[kRounds], mask;
  int F, k, shuffle;
  int64_t *x;
  float *y;
  int *err;
};

__device__ __forceinline__ uint64_t feistel(const BatchArgs &a, uint64_t x) {
  uint64_t L = x >> a.k, R = x & a.mask;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t t = L ^ (mix64(a.key[r] + R) & a.mask);
    L = R;
    R = t;
  }
  return (L << a.k) | R;
}

__global__ __launch_bounds__(kBlock) void k_ctr_batch(BatchArgs a) {
  const int64_t w = a.F + 1, total = a.count * w;
  const bool narrow = total <= (int64_t)UINT32_MAX;                      // wave-uniform: the 32-bit divide is a few instructions
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    int64_t s;
    int c;
    if (narrow) {
      const uint32_t q = (uint32_t)e / (uint32_t)w;
      s = q;
      c = (int)((uint32_t)e - q * (uint32_t)w);
    } else {
      s = e / w;
      c = (int)(e - s * w);
    }
    uint64_t pos = (uint64_t)(a.first + s);                              // < n: the entry point checked first + count <= n
    if (a.shuffle) {
      do pos = feistel(a, pos);
      while (pos >= (uint64_t)a.n);
    }
    const int64_t row = a.index ? a.index[pos] : (int64_t)pos;
    const bool ok = row >= 0 && row < a.n_records;
    const uint32_t v = ok ? a.records[row * w + c] : 0u;
    if (c == 0) a.y[s] = ok ? (float)v : __int_as_float(0x7FC00000);
    else a.x[s * a.F + (c - 1)] = ok ? (int64_t)v : -1;
    if (!ok && a.err) atomicOr(a.err, MI_IDX_OUT_OF_RANGE);
  }
}

}  // namespace

extern "C" {

int64_t mi_ctr_vocab_workspace_bytes(int64_t n) {
  if (n <= 0) return 16;
  return align16(tiles_of(n) * (int64_t)sizeof(uint32_t)) + align16(n);
}

int mi_ctr_vocab_field(const int64_t *sorted_keys, const int64_t *perm, int64_t n, int64_t threshold, uint32_t *out,
                       int64_t stride, int64_t *num_kept, void *workspace, int *err, void *stream) {
  if (n < 0 || threshold < 1 || stride < 1 || !num_kept || !workspace) return MI_ERR_INVALID_ARG;
  if (n > (int64_t)INT32_MAX || stride > (int64_t)INT32_MAX) return MI_ERR_UNSUPPORTED;   // ids and n * stride stay exact
  if (n > 0 && (!sorted_keys || !perm || !out)) return MI_ERR_INVALID_ARG;
  const int64_t tiles = tiles_of(n);
  uint32_t *tile_sums = static_cast<uint32_t *>(workspace);
  uint8_t *flags = static_cast<uint8_t *>(workspace) + align16(tiles * (int64_t)sizeof(uint32_t));
  const int64_t T = threshold > n + 1 ? n + 1 : threshold;
  const int grid = grid_for_tiles(tiles);
  if (n > 0) MI_LAUNCH("ctr_vocab_mark", k_vocab_mark, grid, kBlock, stream, sorted_keys, n, T, flags, tile_sums);
  MI_LAUNCH("ctr_vocab_scan_tiles", k_vocab_scan_tiles, 1, kBlock, stream, tile_sums, tiles, num_kept);
  if (n > 0)
    MI_LAUNCH("ctr_vocab_scatter", k_vocab_scatter, grid, kBlock, stream, (const uint8_t *)flags, perm, n,
              (const uint32_t *)tile_sums, (const int64_t *)num_kept, out, stride, err);
  return launch_status();
}

int mi_ctr_batch(const uint32_t *records, int64_t n_records, int32_t F, const int64_t *index, int64_t n, int32_t shuffle,
                 int64_t seed, int64_t epoch, int64_t first, int64_t count, int64_t *x, float *y, int *err, void *stream) {
  if (n_records < 0 || F < 1 || n < 0 || first < 0 || count < 0 || count > n || first > n - count) return MI_ERR_INVALID_ARG;
  const int64_t w = (int64_t)F + 1;
  if (n_records > INT64_MAX / (4 * w) || count > INT64_MAX / (8 * w) || n > ((int64_t)1 << 62)) return MI_ERR_UNSUPPORTED;
  if (!index && n != n_records) return MI_ERR_INVALID_ARG;
  if (count == 0) return MI_OK;
  if (!records || !x || !y) return MI_ERR_INVALID_ARG;
  BatchArgs a;
  a.records = records; a.index = index; a.n_records = n_records; a.n = n; a.first = first; a.count = count;
  a.F = F; a.shuffle = shuffle != 0;
  int bits = 0;
  for (uint64_t v = (uint64_t)(n - 1); v; v >>= 1) ++bits;
  if (bits < 2) bits = 2;
  a.k = (bits + 1) / 2;
  a.mask = ((uint64_t)1 << a.k) - 1;
  const uint64_t base = mix64((uint64_t)seed + kGold * ((uint64_t)epoch + 1));
  for (int r = 0; r < kRounds; ++r) a.key[r] = mix64(base + kSalt * (uint64_t)(r + 1));
  a.x = x; a.y = y; a.err = err;
  const int64_t blocks = (count * w + kBlock - 1) / kBlock;
  MI_LAUNCH("ctr_batch", k_ctr_batch, (int)(blocks > kMaxGrid ? kMaxGrid : blocks), kBlock, stream, a);
  return launch_status();
}

}  // extern "C"
