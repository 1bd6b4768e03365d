// gather_fm_csr.hip — the CTR models served from a CSR-pruned table (PrunedEmbedding; inference only, as in the reference:
// src/models/embeddings/pruned_embedding.py:136-204 under src/models/deepfm.py:88-98 and scripts/deepfm/infer_deepfm.py).
//   mi_gather_fm_csr_fwd:   row = idx[b, f] + offsets[f],  emb[b, f, :] = the densified CSR row,  y_fm as the other fused
//                           lookups form it — DeepFM's lookup in ONE launch;
//   mi_csr_rows_typed_fwd:  the densify alone over flat ids (PrunedEmbedding.forward, DCN's lookup with x + offsets inside).
// Both take the row pointers as int32 or int64 and the columns as one byte or int64: a compact table (D <= 256,
// nnz < 2^31) holds 5 bytes per stored element + 4 per row instead of 12 + 8.
//
// The row walk is slot-cooperative.  k_csr_rows (embed.hip) has every one of a row's D lanes scan the row's whole column
// list; here the LPR = D / 4 lanes of a row slot (gather_fm.hip's mapping: lane q holds columns 4q .. 4q+3) load the
// row's entries ONCE, lane q entry lo + t LPR + q of trip t — the first kTrips = 4 trips issued together, which covers the
// D entries a row without duplicates can hold — and pass them round the slot by shuffles in ascending entry order.  A lane
// keeps an entry whose col >> 2 is its q, in component col & 3: "a later duplicate wins" is decided by that order alone
// (registers, no LDS or global write race), a column outside [0, D) matches no lane.  The pass stops, wave-uniformly, at
// the longest row of the wave-instruction; past 4 LPR entries a wave-uniform loop loads and passes LPR more at a time
// while any slot still has some.  emb then has the bits mi_csr_rows_fwd writes.
//
// Dependent round trips per sample: ids -> row pointers (+ the first-order weight) -> entries: one more than the dense
// lookup's two.  No float atomics (the only atomic is the err OR), no LDS.
// sum e^2, |S|^2 and 0.5 t + lin are written as explicit fused multiply-adds: the four index-type instantiations of a
// form then cannot differ in how the compiler contracts them, and y_fm of a compact table has the wide table's bits.
#include "common.hpp"
#include "gather_fm_walk.hpp"

namespace {
using namespace mi;

constexpr int kTrips = 4;      // entry trips of a row slot whose loads are in flight together: kTrips * LPR = D entries

template <class CR>
__device__ __forceinline__ int64_t ld_crow(const void *__restrict__ crow, int64_t i) {
  return (int64_t) reinterpret_cast<const CR *>(crow)[i];
}
// the column of entry j as an int, -1 when it lies outside [0, D) (it then matches no lane)
template <class CO>
__device__ __forceinline__ int ld_col(const void *__restrict__ col, int64_t j, int D) {
  if constexpr (sizeof(CO) == 1) {
    const int c = (int) reinterpret_cast<const uint8_t *>(col)[j];
    return c < D ? c : -1;
  } else {
    const int64_t c = reinterpret_cast<const int64_t *>(col)[j];
    return (uint64_t)c < (uint64_t)D ? (int)c : -1;
  }
}
// number of entries of the row [lo, hi) (the triple is trusted as mi_csr_rows_fwd trusts it)
__device__ __forceinline__ int row_len(int64_t lo, int64_t hi) {
  const int64_t n = hi - lo;
  return n <= 0 ? 0 : (n > 0x7fffffff ? 0x7fffffff : (int)n);
}

// what lane q of a row slot holds of the row's first kTrips * LPR entries
struct Ent {
  int c[kTrips];
  float v[kTrips];
};

template <int LPR, class CO>
__device__ __forceinline__ void load_entries(Ent &e, const float *__restrict__ values, const void *__restrict__ col,
                                             int64_t lo, int len, int q) {
#pragma unroll
  for (int t = 0; t < kTrips; ++t) {
    const int i = t * LPR + q;
    const bool in = i < len;
    e.c[t] = in ? ld_col<CO>(col, lo + i, LPR * 4) : -1;
    e.v[t] = in ? values[lo + i] : 0.f;
  }
}

__device__ __forceinline__ void keep_entry(float4 &o, int c, float v, int q) {
  const bool hit = (c >> 2) == q;      // (c = -1: no lane)
  const int k = c & 3;
  o.x = (hit && k == 0) ? v : o.x;
  o.y = (hit && k == 1) ? v : o.y;
  o.z = (hit && k == 2) ? v : o.z;
  o.w = (hit && k == 3) ? v : o.w;
}

// the lane's four columns of the densified row.  Every lane of the wave calls it (len = 0 for a slot without a row):
// the loops' bounds are wave-uniform.
template <int LPR, class CO>
__device__ __forceinline__ float4 densify(const Ent &e, const float *__restrict__ values, const void *__restrict__ col,
                                          int64_t lo, int len, int lane, int q) {
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  const int src0 = lane - q;
#pragma unroll
  for (int t = 0; t < kTrips; ++t) {
    for (int s = 0; s < LPR; ++s) {
      if (__ballot(t * LPR + s < len) == 0) break;
      keep_entry(o, __shfl(e.c[t], src0 + s), __shfl(e.v[t], src0 + s), q);
    }
  }
  for (int b = kTrips * LPR; __ballot(b < len) != 0; b += LPR) {      // rows longer than D entries: duplicates
    const int i = b + q;
    const bool in = i < len;
    const int c = in ? ld_col<CO>(col, lo + i, LPR * 4) : -1;
    const float v = in ? values[lo + i] : 0.f;
    for (int s = 0; s < LPR; ++s) {
      if (__ballot(b + s < len) == 0) break;
      keep_entry(o, __shfl(c, src0 + s), __shfl(v, src0 + s), q);
    }
  }
  return o;
}

__device__ __forceinline__ float sumsq4(float4 v, float acc) {
  return fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, acc))));
}

// column d of the densified row [lo, hi) for every lane of a wave (the scalar forms: all 64 lanes walk ONE row, 64
// entries per trip, passed round in ascending order; d may lie past D, such a lane matches nothing it stores)
template <class CO>
__device__ __forceinline__ float densify_col(const float *__restrict__ values, const void *__restrict__ col, int64_t lo,
                                             int64_t hi, int lane, int d, int D) {
  float o = 0.f;
  for (int64_t j0 = lo; j0 < hi; j0 += kWave) {
    const int64_t j = j0 + lane;
    const bool in = j < hi;
    const int c = in ? ld_col<CO>(col, j, D) : -1;
    const float v = in ? values[j] : 0.f;
    const int cnt = hi - j0 < kWave ? (int)(hi - j0) : kWave;
    for (int s = 0; s < cnt; ++s) {
      const int cc = __shfl(c, s);
      const float vv = __shfl(v, s);
      o = cc == d ? vv : o;
    }
  }
  return o;
}

// ---------------------------------------------------------------- lookup + FM ----
// NIT > 0 (F <= 64): the ids by one coalesced load + shuffles; then the row pointers and first-order weights of the NIT
// steps in flight together, then their entries, then the passes.  NIT = 0: one step at a time, any F.
template <int LPR, int NIT, class CR, class CO>
__global__ __launch_bounds__(kBlock) void k_gather_fm_csr_fwd(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets, const float *__restrict__ values,
    const void *__restrict__ crow, const void *__restrict__ col, const float *__restrict__ w1, int64_t ldw1,
    const float *__restrict__ bias, float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int64_t N, int *err) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const float bv = bias ? bias[0] : 0.f;
  int bad = 0;
  int64_t myoff = 0;
  if constexpr (NIT > 0) myoff = (offsets && lane < F) ? offsets[lane] : 0;

  for (int64_t b = wave0; b < B; b += nwaves) {
    float4 S = make_float4(0.f, 0.f, 0.f, 0.f);
    float ss = 0.f, lin = 0.f;
    const int64_t base = b * F;
    if constexpr (NIT > 0) {
      bool act[NIT];
      int64_t lo[NIT];
      int len[NIT];
      float l[NIT];
      Ent e[NIT];
      const int64_t mine = lane < F ? idx[base + lane] + myoff : 0;
      if (rows_out && lane < F) rows_out[base + lane] = mine;
#pragma unroll
      for (int k = 0; k < NIT; ++k) {
        const int f = r + k * RS;
        act[k] = f < F;
        const int64_t row = __shfl(mine, f & 63);
        const bool ok = act[k] && (uint64_t)row < (uint64_t)N;
        bad |= (act[k] && !ok);
        lo[k] = ok ? ld_crow<CR>(crow, row) : 0;
        const int64_t hi = ok ? ld_crow<CR>(crow, row + 1) : 0;
        len[k] = row_len(lo[k], hi);
        l[k] = (ok && q == 0) ? w1[row * ldw1] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < NIT; ++k) load_entries<LPR, CO>(e[k], values, col, lo[k], len[k], q);
#pragma unroll
      for (int k = 0; k < NIT; ++k) {
        const int f = r + k * RS;
        const float4 v = densify<LPR, CO>(e[k], values, col, lo[k], len[k], lane, q);
        if (act[k]) st4_nt(emb + (base + f) * D + q * 4, v);
        S.x += v.x; S.y += v.y; S.z += v.z; S.w += v.w;
        ss = sumsq4(v, ss);
        lin += l[k];
      }
    } else {
      for (int f0 = 0; f0 < F; f0 += RS) {
        const int f = f0 + r;
        const bool act = f < F;
        const int64_t row = act ? idx[base + f] + (offsets ? offsets[f] : 0) : 0;
        const bool ok = act && (uint64_t)row < (uint64_t)N;
        bad |= (act && !ok);
        const int64_t lo = ok ? ld_crow<CR>(crow, row) : 0;
        const int64_t hi = ok ? ld_crow<CR>(crow, row + 1) : 0;
        const int len = row_len(lo, hi);
        if (ok && q == 0) lin += w1[row * ldw1];
        Ent e;
        load_entries<LPR, CO>(e, values, col, lo, len, q);
        const float4 v = densify<LPR, CO>(e, values, col, lo, len, lane, q);
        if (act) {
          st4_nt(emb + (base + f) * D + q * 4, v);
          if (rows_out && q == 0) rows_out[base + f] = row;
        }
        S.x += v.x; S.y += v.y; S.z += v.z; S.w += v.w;
        ss = sumsq4(v, ss);
      }
    }
    S = slot_sum<LPR>(S);
    float t = (r == 0 ? sumsq4(S, 0.f) : 0.f) - ss;
    t = wave_sum(fmaf(0.5f, t, lin));
    if (lane == 0) yfm[b] = t + bv;
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// any D (scalar accesses): wave per sample, lanes stride over d
template <class CR, class CO>
__global__ __launch_bounds__(kBlock) void k_gather_fm_csr_fwd_anyD(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets, const float *__restrict__ values,
    const void *__restrict__ crow, const void *__restrict__ col, const float *__restrict__ w1, int64_t ldw1,
    const float *__restrict__ bias, float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int D, int64_t N, int *err) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const float bv = bias ? bias[0] : 0.f;
  int bad = 0;
  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    float t = 0.f;
    for (int d0 = 0; d0 < D; d0 += kWave) {
      const int d = d0 + lane;
      float S = 0.f, ss = 0.f;
      for (int f = 0; f < F; ++f) {
        const int64_t row = idx[base + f] + (offsets ? offsets[f] : 0);
        const bool ok = (uint64_t)row < (uint64_t)N;
        bad |= !ok;
        if (d0 == 0 && lane == 0) {
          if (ok) t += w1[row * ldw1];
          if (rows_out) rows_out[base + f] = row;
        }
        const int64_t lo = ok ? ld_crow<CR>(crow, row) : 0;
        const int64_t hi = ok ? ld_crow<CR>(crow, row + 1) : 0;
        const float v = densify_col<CO>(values, col, lo, hi, lane, d, D);
        if (d < D) {
          emb[(base + f) * D + d] = v;
          S += v;
          ss = fmaf(v, v, ss);
        }
      }
      t += 0.5f * (S * S - ss);
    }
    t = wave_sum(t);
    if (lane == 0) yfm[b] = t + bv;
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// ---------------------------------------------------------------- the densify alone ----
// one id per row slot and trip: RS ids per wave-instruction
template <int LPR, class CR, class CO>
__global__ __launch_bounds__(kBlock) void k_csr_rows_typed(
    const float *__restrict__ values, const void *__restrict__ crow, const void *__restrict__ col,
    const int64_t *__restrict__ ids, const int64_t *__restrict__ offsets, int F, int64_t *__restrict__ rows_out,
    float *__restrict__ out, int64_t n, int64_t N, int *err) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  int bad = 0;
  for (int64_t i0 = wave0 * RS; i0 < n; i0 += nwaves * RS) {
    const int64_t i = i0 + r;
    const bool act = i < n;
    const int64_t row = act ? ids[i] + (offsets ? offsets[i % F] : 0) : 0;
    const bool ok = act && (uint64_t)row < (uint64_t)N;
    bad |= (act && !ok);
    const int64_t lo = ok ? ld_crow<CR>(crow, row) : 0;
    const int64_t hi = ok ? ld_crow<CR>(crow, row + 1) : 0;
    const int len = row_len(lo, hi);
    Ent e;
    load_entries<LPR, CO>(e, values, col, lo, len, q);
    const float4 v = densify<LPR, CO>(e, values, col, lo, len, lane, q);
    if (act) {
      st4_nt(out + i * D + q * 4, v);
      if (rows_out && q == 0) rows_out[i] = row;
    }
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// any D: wave per id
template <class CR, class CO>
__global__ __launch_bounds__(kBlock) void k_csr_rows_typed_anyD(
    const float *__restrict__ values, const void *__restrict__ crow, const void *__restrict__ col,
    const int64_t *__restrict__ ids, const int64_t *__restrict__ offsets, int F, int64_t *__restrict__ rows_out,
    float *__restrict__ out, int64_t n, int D, int64_t N, int *err) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  int bad = 0;
  for (int64_t i = wave0; i < n; i += nwaves) {
    const int64_t row = ids[i] + (offsets ? offsets[i % F] : 0);
    const bool ok = (uint64_t)row < (uint64_t)N;
    bad |= !ok;
    if (rows_out && lane == 0) rows_out[i] = row;
    const int64_t lo = ok ? ld_crow<CR>(crow, row) : 0;
    const int64_t hi = ok ? ld_crow<CR>(crow, row + 1) : 0;
    for (int d0 = 0; d0 < D; d0 += kWave) {
      const int d = d0 + lane;
      const float v = densify_col<CO>(values, col, lo, hi, lane, d, D);
      if (d < D) out[i * D + d] = v;
    }
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

template <class CR, class CO>
int launch_fm_csr(const int64_t *idx, const int64_t *offsets, const float *values, const void *crow, const void *col,
                  const float *w1, int64_t ldw1, const float *bias, float *emb, float *yfm, int64_t *rows_out, int64_t B,
                  int F, int D, int64_t N, int *err, void *stream) {
  const int grid = grid_for_waves(B);
  if (vec_ok(D) && aligned16(emb)) {
    const int lpr = D / 4, nit = F <= kWave ? nit_for(F, lpr) : 0;
#define CALL(LPR, NIT)                                                                                              \
  MI_LAUNCH("gather_fm_csr_fwd", (k_gather_fm_csr_fwd<LPR, NIT, CR, CO>), grid, kBlock, stream, idx, offsets, values, \
            crow, col, w1, ldw1, bias, emb, yfm, rows_out, B, F, N, err)
    MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
  } else {
    MI_LAUNCH("gather_fm_csr_fwd", (k_gather_fm_csr_fwd_anyD<CR, CO>), grid, kBlock, stream, idx, offsets, values, crow,
              col, w1, ldw1, bias, emb, yfm, rows_out, B, F, D, N, err);
  }
  return launch_status();
}

template <class CR, class CO>
int launch_rows_typed(const float *values, const void *crow, const void *col, const int64_t *ids, const int64_t *offsets,
                      int F, int64_t *rows_out, float *out, int64_t n, int D, int64_t N, int *err, void *stream) {
  if (vec_ok(D) && aligned16(out)) {
    const int lpr = D / 4, rs = kWave / lpr;
    const int grid = grid_for_waves((n + rs - 1) / rs);
#define CALL(LPR)                                                                                                      \
  MI_LAUNCH("csr_rows_typed", (k_csr_rows_typed<LPR, CR, CO>), grid, kBlock, stream, values, crow, col, ids, offsets, F, \
            rows_out, out, n, N, err)
    MI_DISPATCH_LPR(lpr, CALL)
#undef CALL
  } else {
    MI_LAUNCH("csr_rows_typed", (k_csr_rows_typed_anyD<CR, CO>), grid_for_waves(n), kBlock, stream, values, crow, col, ids,
              offsets, F, rows_out, out, n, D, N, err);
  }
  return launch_status();
}

inline bool widths_ok(int32_t crow_bytes, int32_t col_bytes) {
  return (crow_bytes == 4 || crow_bytes == 8) && (col_bytes == 1 || col_bytes == 8);
}

}  // namespace

// Expands `CALL(CR, CO)` with the index types the two run-time widths name (widths_ok has passed).
#define MI_DISPATCH_CSR_TYPES(crow_bytes, col_bytes, CALL)  \
  if (crow_bytes == 8) {                                    \
    if (col_bytes == 8) return CALL(int64_t, int64_t);      \
    return CALL(int64_t, uint8_t);                          \
  }                                                         \
  if (col_bytes == 8) return CALL(int32_t, int64_t);        \
  return CALL(int32_t, uint8_t);

extern "C" {

int mi_gather_fm_csr_fwd(const int64_t *idx, const int64_t *offsets, const float *values, const void *crow,
                         int32_t crow_bytes, const void *col, int32_t col_bytes, const float *w1, int64_t ldw1,
                         const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out, int64_t B, int32_t F,
                         int32_t D, int64_t N, int32_t *err, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0 || ldw1 < 1 || !widths_ok(crow_bytes, col_bytes)) return MI_ERR_INVALID_ARG;
  if (B == 0) return MI_OK;
  if (!idx || !crow || !w1 || !emb_out || !yfm_out) return MI_ERR_INVALID_ARG;      // (values / col: null when nnz = 0)
#define CALL(CR, CO) \
  launch_fm_csr<CR, CO>(idx, offsets, values, crow, col, w1, ldw1, bias, emb_out, yfm_out, rows_out, B, F, D, N, err, stream)
  MI_DISPATCH_CSR_TYPES(crow_bytes, col_bytes, CALL)
#undef CALL
}

int mi_csr_rows_typed_fwd(const float *values, const void *crow, int32_t crow_bytes, const void *col, int32_t col_bytes,
                          const int64_t *ids, const int64_t *offsets, int32_t F, int64_t *rows_out, float *out, int64_t n,
                          int32_t D, int64_t N, int32_t *err, void *stream) {
  if (n < 0 || D <= 0 || N < 0 || !widths_ok(crow_bytes, col_bytes) || (offsets && F < 1)) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!crow || !ids || !out || (offsets && n % F != 0)) return MI_ERR_INVALID_ARG;
#define CALL(CR, CO) launch_rows_typed<CR, CO>(values, crow, col, ids, offsets, F, rows_out, out, n, D, N, err, stream)
  MI_DISPATCH_CSR_TYPES(crow_bytes, col_bytes, CALL)
#undef CALL
}

}  // extern "C"
