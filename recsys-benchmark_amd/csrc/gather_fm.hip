// gather_fm.hip — DeepFM's embedding gather fused with the FM second-order term
// and the first-order (EmbeddingBag(N,1,sum)) term, forward and backward.
//
// Reference arithmetic: src/models/deepfm.py:88-98 and
// src/models/embeddings/base.py:74-75 (see include/mi355x_recsys.h).
//
// Mapping (CDNA4, wave = 64): ONE WAVE PER SAMPLE.  A row of D = 4*LPR floats is
// read by LPR adjacent lanes as one float4 each (16 B per lane, the widest
// coalesced access), so a wave-instruction moves RS = 64/LPR rows = 1 KiB.
// lane = r*LPR + q  (r = row slot, q = which float4 of the row).  The F rows of
// the sample are covered in NIT = ceil(F/RS) unrolled steps whose loads are all
// issued before the first use, so each wave has NIT row gathers in flight.
// sum_f e (per d) is a shuffle-xor reduction over the r bits of the lane id;
// the per-sample scalar is one 64-lane reduction.  emb[b] is F*D contiguous
// floats, so the stores of a step are one contiguous <=1 KiB run.
//
// HBM-bound integer/copy work: no LDS staging is needed in the forward (each
// byte is used once); the dense backward stages a 1 KiB tile per wave in LDS to
// turn 16-B-strided float4 fragments into 256-B contiguous atomic instructions.
#include <type_traits>

#include "common.hpp"
#include "dual_xform.hpp"
#include "gather_fm_walk.hpp"
#include "prefetch_rows.hpp"
#include "tail_masks.hpp"

namespace {
using namespace mi;

// ------------------------------------------------------------ small helpers ----
// (fm_grad_row, keep_prefix, imin, the Xform operand with thr4 / soft4 / mask4 / keep_bytes, bias_grad_block:
// gather_fm_walk.hpp)
// SLOT = false: gvals[i,:] / g1vals[i] in lookup order (the reference's COO values), i = b*F + f.
// SLOT = true : the row goes to gvals + slot[i]*(D+4), its first-order gradient into column D of
//               the same packed row; slots >= nslot (the dump slot of route.hip) are skipped.
template <int LPR, bool SLOT>
__device__ __forceinline__ void store_grad_row(float *__restrict__ gvals, float *__restrict__ g1vals,
                                               const int64_t *__restrict__ slot, int64_t nslot, int64_t i, int q,
                                               float4 o4, float gy) {
  constexpr int D = LPR * 4;
  if constexpr (SLOT) {
    const int64_t s = slot[i];
    if ((uint64_t)s < (uint64_t)nslot) {
      st4(gvals + s * (D + 4) + q * 4, o4);
      if (q == 0) st4(gvals + s * (D + 4) + D, make_float4(gy, 0.f, 0.f, 0.f));
    }
  } else {
    st4(gvals + i * D + q * 4, o4);
    if (q == 0) g1vals[i] = gy;
  }
}

// The masked lookups (mi_gather_fm_masked_*) keep a PREFIX of every looked-up row:
//   kept(b, f) = min(keep ? keep[row] : D, fwidth ? fwidth[f] : D),   emb[b, f, d] = d < kept ? W[row, d] : +0
// keep uint8[N] (0 = a dead row), fwidth int32[F]; a value above D acts as D (d never reaches it), a negative fwidth as 0.
// the kept width of lookup i (field f) in the backward: `rows` is the forward's rows_out; a row it flagged keeps nothing
__device__ __forceinline__ int kept_width(const int64_t *__restrict__ rows, const uint8_t *__restrict__ keep,
                                          const int32_t *__restrict__ fwidth, int64_t i, int f, int64_t N, int D) {
  int kw = fwidth ? fwidth[f] : D;
  if (keep) {
    const int64_t row = rows[i];
    kw = (uint64_t)row < (uint64_t)N ? imin(kw, (int)keep[row]) : 0;
  }
  return kw;
}
struct KeptWidths {      // (the same operands as one kernel argument)
  const int64_t *rows;
  const uint8_t *keep;
  const int32_t *fwidth;
  int64_t N;
};
__device__ __forceinline__ int kept_width(KeptWidths m, int64_t i, int f, int D) {
  return kept_width(m.rows, m.keep, m.fwidth, i, f, m.N, D);
}

// ---------------------------------------------------------------- forward ----
// gather_fm_fwd_blocks / gather_fm_fwd_anyD_blocks, the walk over a sample's fields, are gather_fm_walk.hpp's; these are
// the kernels around them.
template <int LPR, int NIT, bool SHFL>
__global__ __launch_bounds__(kBlock) void k_gather_fm_fwd(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets,
    const float *__restrict__ W, const float *__restrict__ w1, const float *__restrict__ bias,
    float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int64_t N, int64_t ldw, int64_t ldw1, int *err, float *__restrict__ sum_out) {
  gather_fm_fwd_blocks<LPR, NIT, SHFL>(idx, offsets, W, w1, bias, emb, yfm, rows_out, B, F, N, ldw, ldw1, err, sum_out,
                                       (int)blockIdx.x, (int)gridDim.x);
}
template <int LPR, int NIT, bool SHFL>
__global__ __launch_bounds__(kBlock) void k_gather_fm_fwd_masked(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets,
    const float *__restrict__ W, const float *__restrict__ w1, const float *__restrict__ bias,
    float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int64_t N, int64_t ldw, int64_t ldw1, int *err, float *__restrict__ sum_out,
    const uint8_t *__restrict__ keep, const int32_t *__restrict__ fwidth) {
  gather_fm_fwd_blocks<LPR, NIT, SHFL, true>(idx, offsets, W, w1, bias, emb, yfm, rows_out, B, F, N, ldw, ldw1, err, sum_out,
                                             (int)blockIdx.x, (int)gridDim.x, keep, fwidth);
}
template <int LPR, int NIT, bool SHFL, int XF>
__global__ __launch_bounds__(kBlock) void k_gather_fm_fwd_xform(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets,
    const float *__restrict__ W, const float *__restrict__ w1, const float *__restrict__ bias,
    float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int64_t N, int64_t ldw, int64_t ldw1, int *err, float *__restrict__ sum_out, Xform xf) {
  gather_fm_fwd_blocks<LPR, NIT, SHFL, false, XF>(idx, offsets, W, w1, bias, emb, yfm, rows_out, B, F, N, ldw, ldw1, err,
                                                  sum_out, (int)blockIdx.x, (int)gridDim.x, nullptr, nullptr, xf);
}
// The same launch carrying the MLP tail's dropout keep bits and the zero fill of its accumulation buffer in workgroups
// past the first `ngather` (tail_masks.hpp): in DeepFM's fused step this kernel is the first of the step, every reader of
// the bits and every adder into the buffer comes later, and the mask work (~1 us spread over the chip, all ALU) runs
// beside a gather that waits on memory — one launch less per step.  The extra workgroups sit at the END of the grid: the
// gather's are dispatched first.
template <int LPR, int NIT>
__global__ __launch_bounds__(kBlock) void k_gather_fm_fwd_ride(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets,
    const float *__restrict__ W, const float *__restrict__ w1, const float *__restrict__ bias,
    float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int64_t N, int64_t ldw, int64_t ldw1, int *err, float *__restrict__ sum_out, int ngather, MaskRide ride) {
  if ((int)blockIdx.x >= ngather) {
    const int rb = (int)blockIdx.x - ngather;
    if (rb < ride.mask_blocks) mask_blocks(ride.j, ride.seed, ride.zero4, ride.nzero4, rb, ride.mask_blocks);
    else affine_consts_blocks(ride.aff, rb - ride.mask_blocks, (int)gridDim.x - ngather - ride.mask_blocks);
    return;
  }
  // every workgroup of the launch is resident at once (1 024 + ~200 of the chip's 2 048 slots): the gather's waves wait on
  // memory most of the time and should win the issue slot against the mask work's 64-bit multiplies whenever they are ready
  __builtin_amdgcn_s_setprio(2);
  gather_fm_fwd_blocks<LPR, NIT, true>(idx, offsets, W, w1, bias, emb, yfm, rows_out, B, F, N, ldw, ldw1, err, sum_out,
                                       (int)blockIdx.x, ngather);
}

__global__ __launch_bounds__(kBlock) void k_mask_job(MaskRide ride) {
  const int rb = (int)blockIdx.x;
  if (rb < ride.mask_blocks) mask_blocks(ride.j, ride.seed, ride.zero4, ride.nzero4, rb, ride.mask_blocks);
  else affine_consts_blocks(ride.aff, rb - ride.mask_blocks, (int)gridDim.x - ride.mask_blocks);
}

__global__ __launch_bounds__(kBlock) void k_gather_fm_fwd_anyD(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets,
    const float *__restrict__ W, const float *__restrict__ w1, const float *__restrict__ bias,
    float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int D, int64_t N, int *err, float *__restrict__ sum_out) {
  gather_fm_fwd_anyD_blocks<false>(idx, offsets, W, w1, bias, emb, yfm, rows_out, B, F, D, N, err, sum_out);
}
__global__ __launch_bounds__(kBlock) void k_gather_fm_fwd_anyD_masked(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets,
    const float *__restrict__ W, const float *__restrict__ w1, const float *__restrict__ bias,
    float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int D, int64_t N, int *err, float *__restrict__ sum_out,
    const uint8_t *__restrict__ keep, const int32_t *__restrict__ fwidth) {
  gather_fm_fwd_anyD_blocks<true>(idx, offsets, W, w1, bias, emb, yfm, rows_out, B, F, D, N, err, sum_out, keep, fwidth);
}
template <int XF>
__global__ __launch_bounds__(kBlock) void k_gather_fm_fwd_anyD_xform(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets,
    const float *__restrict__ W, const float *__restrict__ w1, const float *__restrict__ bias,
    float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int D, int64_t N, int *err, float *__restrict__ sum_out, Xform xf) {
  gather_fm_fwd_anyD_blocks<false, XF>(idx, offsets, W, w1, bias, emb, yfm, rows_out, B, F, D, N, err, sum_out, nullptr,
                                       nullptr, xf);
}

// ----------------------------------------------------- backward, row form ----
// e[k] / ge[k] = the lane's float4 of emb / g_emb (zeros without one) at field f + k*RS of the sample at `base`; zeros past F
template <int LPR, int NSTEP>
__device__ __forceinline__ void load_chunk(const float *__restrict__ emb, const float *__restrict__ g_emb, int64_t base, int f,
                                           int F, int q, float4 (&e)[NSTEP], float4 (&ge)[NSTEP]) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < NSTEP; ++k, f += kWave / LPR) {
    const bool act = f < F;
    const int64_t o = (base + f) * (LPR * 4) + q * 4;
    e[k] = act ? ld4(emb + o) : z;
    ge[k] = (act && g_emb) ? ld4(g_emb + o) : z;
  }
}

// The gradient rows, stored by store_grad_row in either form.  NIT > 0: e[] and g_emb's rows are read once, all NIT loads
// in flight, and e[] stays in registers between the sum over the fields and the write; NIT = 0: one-step chunks, e read
// again in the second walk.
// The masked form (mi_gather_fm_masked_bwd_rows) is this kernel with ONE more argument, a KeptWidths, as the pack M
// (empty otherwise: the plain kernel's arguments and code are what they were): columns at or past the lookup's kept
// width are stored as exact zeros (emb holds zeros there already, so S needs nothing).
template <int LPR, int NIT, bool SLOT, class... M>
__global__ __launch_bounds__(kBlock) void k_gather_fm_bwd_rows(
    const float *__restrict__ emb, const float *__restrict__ g_y,
    const float *__restrict__ g_emb, float *__restrict__ gvals, float *__restrict__ g1vals,
    int64_t B, int F, const int64_t *__restrict__ slot, int64_t nslot, float *__restrict__ gbias, M... m) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  constexpr int NSTEP = NIT > 0 ? NIT : 1;
  constexpr bool MASK = sizeof...(M) > 0;
  static_assert(sizeof...(M) <= 1 && (std::is_same_v<M, KeptWidths> && ...), "the pack is empty or one KeptWidths");
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blk * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const int fend = NIT > 0 ? 1 : F;      // (NIT > 0: the chunk loops below run once)

  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    const float gy = g_y[b];
    float4 S = z;
    float4 e[NSTEP], ge[NSTEP];
    int kw[NSTEP];      // (MASK only)
    if constexpr (MASK && NIT > 0) {      // the ids and their bytes travel with the rows of e / g_emb
#pragma unroll
      for (int k = 0; k < NSTEP; ++k) {
        const int f = r + k * RS;
        kw[k] = f < F ? kept_width(m..., base + f, f, D) : 0;
      }
    }
    for (int f0 = 0; f0 < fend; f0 += NSTEP * RS) {
      load_chunk<LPR, NSTEP>(emb, NIT > 0 ? g_emb : nullptr, base, f0 + r, F, q, e, ge);
#pragma unroll
      for (int k = 0; k < NSTEP; ++k) acc4(S, e[k]);
    }
    S = slot_sum<LPR>(S);
    for (int f0 = 0; f0 < fend; f0 += NSTEP * RS) {
      if constexpr (NIT == 0) load_chunk<LPR, NSTEP>(emb, g_emb, base, f0 + r, F, q, e, ge);
#pragma unroll
      for (int k = 0; k < NSTEP; ++k) {
        const int f = f0 + r + k * RS;
        if (f < F) {
          float4 o4 = fm_grad_row(ge[k], gy, S, e[k]);
          if constexpr (MASK) {
            if constexpr (NIT == 0) kw[k] = kept_width(m..., base + f, f, D);
            o4 = keep_prefix(o4, q, kw[k]);
          }
          store_grad_row<LPR, SLOT>(gvals, g1vals, slot, nslot, base + f, q, o4, gy);
        }
      }
    }
  }
}

template <bool MASK>
__device__ __forceinline__ void gather_fm_bwd_rows_anyD_blocks(
    const float *__restrict__ emb, const float *__restrict__ g_y,
    const float *__restrict__ g_emb, float *__restrict__ gvals, float *__restrict__ g1vals,
    int64_t B, int F, int D, int blk, int nblk, const int64_t *__restrict__ rows = nullptr,
    const uint8_t *__restrict__ keep = nullptr, const int32_t *__restrict__ fwidth = nullptr, int64_t N = 0) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blk * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    const float gy = g_y[b];
    for (int f = lane; f < F; f += kWave) g1vals[base + f] = gy;
    for (int d = lane; d < D; d += kWave) {
      float S = 0.f;
      for (int f = 0; f < F; ++f) S += emb[(base + f) * D + d];
      for (int f = 0; f < F; ++f) {
        const int64_t o = (base + f) * D + d;
        float g = (g_emb ? g_emb[o] : 0.f) + gy * (S - emb[o]);
        if constexpr (MASK) g = d < kept_width(rows, keep, fwidth, base + f, f, N, D) ? g : 0.f;
        gvals[o] = g;
      }
    }
  }
}
__global__ __launch_bounds__(kBlock) void k_gather_fm_bwd_rows_anyD(
    const float *__restrict__ emb, const float *__restrict__ g_y,
    const float *__restrict__ g_emb, float *__restrict__ gvals, float *__restrict__ g1vals,
    int64_t B, int F, int D, float *__restrict__ gbias) {
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  gather_fm_bwd_rows_anyD_blocks<false>(emb, g_y, g_emb, gvals, g1vals, B, F, D, blk, nblk);
}
__global__ __launch_bounds__(kBlock) void k_gather_fm_bwd_rows_anyD_masked(
    const float *__restrict__ emb, const float *__restrict__ g_y,
    const float *__restrict__ g_emb, float *__restrict__ gvals, float *__restrict__ g1vals,
    int64_t B, int F, int D, float *__restrict__ gbias, const int64_t *__restrict__ rows,
    const uint8_t *__restrict__ keep, const int32_t *__restrict__ fwidth, int64_t N) {
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  gather_fm_bwd_rows_anyD_blocks<true>(emb, g_y, g_emb, gvals, g1vals, B, F, D, blk, nblk, rows, keep, fwidth, N);
}

// ------------------------------------- backward, row form, PEP transforms ----
// mi_gather_fm_soft_bwd_rows / mi_gather_fm_elemmask_bwd_rows: the walk of k_gather_fm_bwd_rows over the SAVED emb (W is
// not read again), with dE = g_emb + g_y (S_b - e) as there, and
//   XF_SOFT: gvals = dE [e != 0],   svals = -dE sign(e) sigma(s) (1 - sigma(s))     (sign(0) = 0 carries the [e != 0])
//            [e != 0] IS the reference's relu derivative here: e = sign(w) u with u = relu(|w| - sigma(s)), so e is
//            non-zero exactly when |w| - sigma(s) > 0 (then |w| > sigma(s) >= 0 and sign(w) != 0).
//   XF_MASK: gvals = dE where M[row, d] — the mask from M, not from e: a kept element may hold exactly 0.
// svals by the threshold's strides: (D,1) one row [D] per lookup; (1,0) one float per lookup, summed over d across the
// row's LPR lanes; (0,1) / (0,0) every thread adds its lookups' values up per column and column_join sums the grid.
constexpr int kJoinMaxD = 256;
struct SoftGrad {
  float *svals;      // [B*F, D], [B*F], [D] or [1]
  float *part;       // (0,*) forms: nblk x D partial column sums
  unsigned *ticket;  // (0,*) forms: zero on entry, zero again on exit
};

// Column sums over the grid without float atomics, block_join's hand-off (common.hpp) with D values per workgroup:
// red[w][c] holds wave w's sum of column c.  Wave 0 adds the waves in order and publishes the workgroup's D sums (sc1
// stores), waits for them (s_waitcnt vmcnt(0) covers every store the wave issued), then its lane 0 takes the ticket.  The
// workgroup whose ticket came back last adds all workgroups' sums: thread (g, c) those of workgroups g, g + G, ... in
// that order, then thread c the G group sums in order — a fixed tree, so reruns give the same bits.  total: the [1]
// threshold, the D column sums added in column order.
__device__ __forceinline__ void column_join(float (*red)[kJoinMaxD], int D, float *__restrict__ part, unsigned *ticket,
                                            float *__restrict__ out, bool total, int blk, int nblk) {
  __shared__ bool last;
  __shared__ float grp[kBlock];
  const int lane = threadIdx.x & 63;
  __syncthreads();
  if (threadIdx.x < kWave) {
    for (int c = lane; c < D; c += kWave) {
      float t = 0.f;
      for (int j = 0; j < kWavesPerBlock; ++j) t += red[j][c];
      __hip_atomic_store(part + (int64_t)blk * D + c, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nblk - 1;
  }
  __syncthreads();
  if (!last) return;
  const int G = kBlock / D;      // (D <= kJoinMaxD = kBlock: at least one group)
  const int c = threadIdx.x % D, g = threadIdx.x / D;
  float t = 0.f;
  if (g < G)
    for (int j = g; j < nblk; j += G) t += __hip_atomic_load(part + (int64_t)j * D + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  grp[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x < D) {
    t = 0.f;
    for (int j = 0; j < G; ++j) t += grp[j * D + threadIdx.x];
    if (!total) out[threadIdx.x] = t;
    red[0][threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (total) {
      t = 0.f;
      for (int j = 0; j < D; ++j) t += red[0][j];
      out[0] = t;
    }
    *ticket = 0;
  }
}

__device__ __forceinline__ float dsigmoid_(float s) {
  const float t = sigmoidf_(s);
  return t * (1.f - t);
}

template <int LPR, int NIT, int XF>
__global__ __launch_bounds__(kBlock) void k_gather_fm_xform_bwd_rows(
    const int64_t *__restrict__ rows, const float *__restrict__ emb, const float *__restrict__ g_y,
    const float *__restrict__ g_emb, float *__restrict__ gvals, float *__restrict__ g1vals,
    int64_t B, int F, int64_t N, float *__restrict__ gbias, Xform xf, SoftGrad sg) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  constexpr int NSTEP = NIT > 0 ? NIT : 1;
  __shared__ __align__(16) float red[XF == XF_SOFT ? kWavesPerBlock : 1][kJoinMaxD];      // (written with st4)
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blk * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const int fend = NIT > 0 ? 1 : F;      // (NIT > 0: the chunk loops below run once)
  const bool joined = XF == XF_SOFT && xf.srs == 0;
  float4 cs = z;      // (XF_SOFT, srs == 0) this thread's column sums of svals

  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    const float gy = g_y[b];
    float4 S = z;
    float4 e[NSTEP], ge[NSTEP];
    for (int f0 = 0; f0 < fend; f0 += NSTEP * RS) {
      load_chunk<LPR, NSTEP>(emb, NIT > 0 ? g_emb : nullptr, base, f0 + r, F, q, e, ge);
#pragma unroll
      for (int k = 0; k < NSTEP; ++k) acc4(S, e[k]);
    }
    S = slot_sum<LPR>(S);
    for (int f0 = 0; f0 < fend; f0 += NSTEP * RS) {
      if constexpr (NIT == 0) load_chunk<LPR, NSTEP>(emb, g_emb, base, f0 + r, F, q, e, ge);
#pragma unroll
      for (int k = 0; k < NSTEP; ++k) {
        const int f = f0 + r + k * RS;
        const bool act = f < F;
        const int64_t i = base + f;
        const int64_t row = act ? rows[i] : -1;
        const bool ok = (uint64_t)row < (uint64_t)N;      // (a row the forward flagged: emb is zero, its gradients too)
        const float4 dE = fm_grad_row(ge[k], gy, S, e[k]);
        float4 o4 = z;
        if constexpr (XF == XF_MASK) {
          o4 = keep_bytes(dE, ok ? mask4(xf.M, row * D + q * 4) : 0u);
        } else {
          const float4 ev = e[k];
          o4 = make_float4(ev.x != 0.f ? dE.x : 0.f, ev.y != 0.f ? dE.y : 0.f, ev.z != 0.f ? dE.z : 0.f,
                           ev.w != 0.f ? dE.w : 0.f);
          float4 sv = z;
          if (ok) {
            const float4 s4 = thr4(xf, row, q);
            sv = make_float4(-o4.x * signf_(ev.x) * dsigmoid_(s4.x), -o4.y * signf_(ev.y) * dsigmoid_(s4.y),
                             -o4.z * signf_(ev.z) * dsigmoid_(s4.z), -o4.w * signf_(ev.w) * dsigmoid_(s4.w));
          }
          if (joined) {
            acc4(cs, sv);
          } else if (xf.scs) {
            if (act) st4(sg.svals + i * D + q * 4, sv);
          } else {
            float t = (sv.x + sv.y) + (sv.z + sv.w);
#pragma unroll
            for (int m = 1; m < LPR; m <<= 1) t += __shfl_xor(t, m);
            if (act && q == 0) sg.svals[i] = t;
          }
        }
        if (act) store_grad_row<LPR, false>(gvals, g1vals, nullptr, 0, i, q, o4, gy);
      }
    }
  }
  if constexpr (XF == XF_SOFT) {
    if (joined) {      // (uniform over the grid: every workgroup but the bias one arrives here)
      cs = slot_sum<LPR>(cs);
      if (lane < LPR) st4(&red[threadIdx.x >> 6][lane * 4], cs);
      column_join(red, D, sg.part, sg.ticket, sg.svals, xf.scs == 0, blk, nblk);
    }
  }
}

// any D <= kJoinMaxD (scalar accesses): wave per sample, lanes stride over d
template <int XF>
__global__ __launch_bounds__(kBlock) void k_gather_fm_xform_bwd_rows_anyD(
    const int64_t *__restrict__ rows, const float *__restrict__ emb, const float *__restrict__ g_y,
    const float *__restrict__ g_emb, float *__restrict__ gvals, float *__restrict__ g1vals,
    int64_t B, int F, int D, int64_t N, float *__restrict__ gbias, Xform xf, SoftGrad sg) {
  __shared__ __align__(16) float red[XF == XF_SOFT ? kWavesPerBlock : 1][kJoinMaxD];      // (written with st4)
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blk * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
  const bool joined = XF == XF_SOFT && xf.srs == 0;
  float cs[kJoinMaxD / kWave] = {0.f, 0.f, 0.f, 0.f};      // column lane + 64 j
  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    const float gy = g_y[b];
    for (int f = lane; f < F; f += kWave) g1vals[base + f] = gy;
#pragma unroll
    for (int j = 0; j < kJoinMaxD / kWave; ++j) {
      const int d = lane + j * kWave;
      if (d >= D) continue;
      float S = 0.f;
      for (int f = 0; f < F; ++f) S += emb[(base + f) * D + d];
      for (int f = 0; f < F; ++f) {
        const int64_t o = (base + f) * D + d;
        const int64_t row = rows[base + f];
        const bool ok = (uint64_t)row < (uint64_t)N;
        const float ev = emb[o];
        const float dE = (g_emb ? g_emb[o] : 0.f) + gy * (S - ev);
        if constexpr (XF == XF_MASK) {
          gvals[o] = (ok && xf.M[row * D + d]) ? dE : 0.f;
        } else {
          const float g = ev != 0.f ? dE : 0.f;
          gvals[o] = g;
          const float sv = ok ? -g * signf_(ev) * dsigmoid_(xf.S[row * xf.srs + d * xf.scs]) : 0.f;
          if (joined) cs[j] += sv;
          else if (xf.scs) sg.svals[o] = sv;
        }
      }
    }
    if (XF == XF_SOFT && !joined && xf.scs == 0) {      // feature: one value per lookup, its columns summed over the wave
      for (int f = 0; f < F; ++f) {
        const int64_t row = rows[base + f];
        const bool ok = (uint64_t)row < (uint64_t)N;
        const float ds = ok ? dsigmoid_(xf.S[row * xf.srs]) : 0.f;
        float t = 0.f;
        for (int d = lane; d < D; d += kWave) {
          const int64_t o = (base + f) * D + d;
          t += -gvals[o] * signf_(emb[o]) * ds;      // (gvals[o]: this lane's own store above)
        }
        t = wave_sum(t);
        if (lane == 0) sg.svals[base + f] = t;
      }
    }
  }
  if constexpr (XF == XF_SOFT) {
    if (joined) {
      for (int j = 0; j < kJoinMaxD / kWave; ++j) red[threadIdx.x >> 6][lane + j * kWave] = cs[j];
      column_join(red, D, sg.part, sg.ticket, sg.svals, xf.scs == 0, blk, nblk);
    }
  }
}

// ------------------------------------------- backward, summed per slot ----
// The de-duplicated sharded lookup (route.hip, mi_route_buckets_unique) lets many lookups share one slot, so the slot
// backward cannot store: every slot needs the SUM of its lookups' gradient rows.  Store pass + per-destination sum pass
// (no float atomics): k_gather_fm_bwd_rows<SLOT=false> writes the per-lookup rows, then this kernel PULLS — slot s adds
// rows order[begin_s .. end_s) in that order, which routing made the ascending flat lookup index.
//   phase 1: LPR lanes per slot, for the slots of up to kLongSeg lookups (nearly all of them);
//   phase 2: a whole wave per LONG slot (a field with fewer values than B / kLongSeg has only long ones; so has a hot
//            value).  Wave w takes the slots = w modulo the number of waves, so the neighbouring long slots of a small
//            field go to different waves.  Per round the wave fetches RS*U rows at once into its LDS slab and one lane
//            per column adds them in order: the chain of adds stays serial, the loads do not.  Rows past the end are
//            staged as zeros (x + 0 = x), which keeps the adding loop's trip count fixed.
constexpr int kLongSeg = 32;

// slot s's lookups are order[beg .. end); an empty range for a slot past the last one or with bounds outside [0, n]
__device__ __forceinline__ void seg_range(const int32_t *__restrict__ seg, int64_t s, int64_t nslot, int64_t n, int &beg,
                                          int &end) {
  beg = end = 0;
  if (s < nslot) {
    beg = seg[2 * s];
    end = seg[2 * s + 1];
    if (beg < 0 || end > n || end < beg) beg = end = 0;
  }
}

template <int LPR>
__global__ __launch_bounds__(kBlock) void k_segment_sum(const int32_t *__restrict__ seg,
                                                        const float *__restrict__ gvals,
                                                        const float *__restrict__ g1vals,
                                                        float *__restrict__ gbuf, int64_t nslot, int64_t n) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  constexpr int LD = D + 4;
  constexpr int U = LPR >= 4 ? 8 : 4;            // row fetches in flight per lane in phase 2
  constexpr int ROWS = RS * U;                   // rows per round
  constexpr int NC = (LD + kWave - 1) / kWave;   // columns per lane when one lane adds one column
  __shared__ float slab[kWavesPerBlock][ROWS * LD];
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + wib;
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const int32_t *__restrict__ order = seg + 2 * nslot;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float *my = slab[wib];
  // ---- phase 1 (+1: the dump row nslot is written as zeros, nobody's gradient)
  for (int64_t tile = wave0; tile * RS < nslot + 1; tile += nwaves) {
    const int64_t s = tile * RS + r;
    int beg, end;
    seg_range(seg, s, nslot, n, beg, end);
    if (s > nslot || end - beg > kLongSeg) continue;
    float4 acc = z;
    float a1 = 0.f;
    for (int t = beg; t < end; t += 4) {
      int i[4];
      float4 v[4];
      float l[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) i[u] = t + u < end ? order[t + u] : -1;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool ok = (uint64_t)(uint32_t)i[u] < (uint64_t)n;
        v[u] = ok ? ld4(gvals + (int64_t)i[u] * D + q * 4) : z;
        l[u] = (ok && q == 0) ? g1vals[i[u]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (t + u < end) {
          acc4(acc, v[u]);
          a1 += l[u];
        }
      }
    }
    st4(gbuf + s * LD + q * 4, acc);
    if (q == 0) st4(gbuf + s * LD + D, make_float4(a1, 0.f, 0.f, 0.f));
  }
  // ---- phase 2: lane k looks at slot base + k * nwaves + wave0, the wave then takes its long ones in turn
  for (int64_t base = 0; base < nslot; base += (int64_t)kWave * nwaves) {
    const int64_t sl = base + (int64_t)lane * nwaves + wave0;
    int lb, le;
    seg_range(seg, sl, nslot, n, lb, le);
    unsigned long long m = __ballot(le - lb > kLongSeg);
    while (m) {
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int b0 = __shfl(lb, src), e0 = __shfl(le, src);
      const int64_t s0 = base + (int64_t)src * nwaves + wave0;
      float c[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) c[k] = 0.f;
      int inext[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = b0 + u * RS + r;
        inext[u] = t < e0 ? order[t] : -1;
      }
      for (int t0 = b0; t0 < e0; t0 += ROWS) {
        float4 v[U];
        float l[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool ok = (uint64_t)(uint32_t)inext[u] < (uint64_t)n;
          v[u] = ok ? ld4(gvals + (int64_t)inext[u] * D + q * 4) : z;
          l[u] = (ok && q == 0) ? g1vals[inext[u]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {             // the next round's indices travel while this round is added up
          const int t = t0 + ROWS + u * RS + r;
          inext[u] = t < e0 ? order[t] : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          st4(my + (u * RS + r) * LD + q * 4, v[u]);
          if (q == 0) st4(my + (u * RS + r) * LD + D, make_float4(l[u], 0.f, 0.f, 0.f));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          const int col = lane + k * kWave;
          if (col < LD) {
#pragma unroll 16
            for (int j = 0; j < ROWS; ++j) c[k] += my[j * LD + col];
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int col = lane + k * kWave;
        if (col < LD) gbuf[s0 * LD + col] = c[k];
      }
    }
  }
}

// --------------------------------------------------- backward, dense form ----
// Same gradient rows, scatter-added into gW / gw1.  The wave's RS x D tile of a
// step (256 floats = the lanes' float4 fragments back to back) goes through a
// wave-private 1 KiB LDS slab so that each of the 4 atomic wave-instructions
// covers 64 CONSECUTIVE floats of the tile: whole 256-B runs per row (D >= 64)
// or 64/D whole rows (D < 64) — the shape global float atomics run fastest at
// (MI355X_MICROARCH.md, "Global float atomics").
// MASK (mi_gather_fm_masked_bwd_dense): an element at or past its row's kept width issues NO atomic — gW stays the
// caller's zero there, and a table kept to a fifth sends a fifth of the atomic traffic.  The first-order adds are unmasked.
// (slab: the workgroup's kWavesPerBlock x 256 floats of LDS, declared by the kernel)
template <int LPR, int NIT, bool MASK = false>
__device__ __forceinline__ void gather_fm_bwd_dense_blocks(
    const int64_t *__restrict__ rows, const float *__restrict__ emb,
    const float *__restrict__ g_y, const float *__restrict__ g_emb,
    float *__restrict__ gW, float *__restrict__ gw1, int64_t B, int F, int64_t N, float (*slab)[kWave * 4], int blk, int nblk,
    const uint8_t *__restrict__ keep = nullptr, const int32_t *__restrict__ fwidth = nullptr) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blk * kWavesPerBlock + wib;
  const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float *my = slab[wib];
  constexpr int NSTEP = NIT > 0 ? NIT : 1;

  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    const float gy = g_y[b];
    float4 S = z;
    for (int f = r; f < F; f += RS) {
      const float4 e = ld4(emb + (base + f) * D + q * 4);
      acc4(S, e);
    }
    S = slot_sum<LPR>(S);
    const int nsteps = NIT > 0 ? NSTEP : (F + RS - 1) / RS;
    for (int k = 0; k < nsteps; ++k) {
      const int f = r + k * RS;
      const bool act = f < F;
      int64_t row = -1;
      float4 o4 = z;
      int kw = 0;      // (MASK only)
      if (act) {
        const int64_t o = (base + f) * D + q * 4;
        const float4 e = ld4(emb + o);
        const float4 ge = g_emb ? ld4(g_emb + o) : z;
        row = rows[base + f];
        if ((uint64_t)row >= (uint64_t)N) row = -1;
        if constexpr (MASK) {
          kw = fwidth ? fwidth[f] : D;
          if (keep && row >= 0) kw = imin(kw, (int)keep[row]);
        }
        o4 = fm_grad_row(ge, gy, S, e);
        if (q == 0 && row >= 0) atomicAdd(gw1 + row, gy);
      }
      st4(my + lane * 4, o4);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int el = j * kWave + lane;  // element of the RS x D tile
        const int tr = el / D, tc = el % D;
        const int64_t trow = __shfl(row, tr * LPR);
        const float val = my[el];
        if constexpr (MASK) {
          const int tkw = __shfl(kw, tr * LPR);
          if (trow >= 0 && tc < tkw) atomicAdd(gW + trow * D + tc, val);
        } else {
          if (trow >= 0) atomicAdd(gW + trow * D + tc, val);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}
template <int LPR, int NIT>
__global__ __launch_bounds__(kBlock) void k_gather_fm_bwd_dense(
    const int64_t *__restrict__ rows, const float *__restrict__ emb,
    const float *__restrict__ g_y, const float *__restrict__ g_emb,
    float *__restrict__ gW, float *__restrict__ gw1, int64_t B, int F, int64_t N, float *__restrict__ gbias) {
  __shared__ float slab[kWavesPerBlock][kWave * 4];
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  gather_fm_bwd_dense_blocks<LPR, NIT>(rows, emb, g_y, g_emb, gW, gw1, B, F, N, slab, blk, nblk);
}
template <int LPR, int NIT>
__global__ __launch_bounds__(kBlock) void k_gather_fm_bwd_dense_masked(
    const int64_t *__restrict__ rows, const float *__restrict__ emb,
    const float *__restrict__ g_y, const float *__restrict__ g_emb,
    float *__restrict__ gW, float *__restrict__ gw1, int64_t B, int F, int64_t N, float *__restrict__ gbias,
    const uint8_t *__restrict__ keep, const int32_t *__restrict__ fwidth) {
  __shared__ float slab[kWavesPerBlock][kWave * 4];
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  gather_fm_bwd_dense_blocks<LPR, NIT, true>(rows, emb, g_y, g_emb, gW, gw1, B, F, N, slab, blk, nblk, keep, fwidth);
}

template <bool MASK>
__device__ __forceinline__ void gather_fm_bwd_dense_anyD_blocks(
    const int64_t *__restrict__ rows, const float *__restrict__ emb,
    const float *__restrict__ g_y, const float *__restrict__ g_emb,
    float *__restrict__ gW, float *__restrict__ gw1, int64_t B, int F, int D, int64_t N, int blk, int nblk,
    const uint8_t *__restrict__ keep = nullptr, const int32_t *__restrict__ fwidth = nullptr) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blk * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    const float gy = g_y[b];
    for (int f = lane; f < F; f += kWave) {
      const int64_t row = rows[base + f];
      if ((uint64_t)row < (uint64_t)N) atomicAdd(gw1 + row, gy);
    }
    for (int d = lane; d < D; d += kWave) {
      float S = 0.f;
      for (int f = 0; f < F; ++f) S += emb[(base + f) * D + d];
      for (int f = 0; f < F; ++f) {
        const int64_t o = (base + f) * D + d;
        const int64_t row = rows[base + f];
        bool add = (uint64_t)row < (uint64_t)N;
        if constexpr (MASK) add = add && d < kept_width(rows, keep, fwidth, base + f, f, N, D);
        if (add) atomicAdd(gW + row * D + d, (g_emb ? g_emb[o] : 0.f) + gy * (S - emb[o]));
      }
    }
  }
}
__global__ __launch_bounds__(kBlock) void k_gather_fm_bwd_dense_anyD(
    const int64_t *__restrict__ rows, const float *__restrict__ emb,
    const float *__restrict__ g_y, const float *__restrict__ g_emb,
    float *__restrict__ gW, float *__restrict__ gw1, int64_t B, int F, int D, int64_t N, float *__restrict__ gbias) {
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  gather_fm_bwd_dense_anyD_blocks<false>(rows, emb, g_y, g_emb, gW, gw1, B, F, D, N, blk, nblk);
}
__global__ __launch_bounds__(kBlock) void k_gather_fm_bwd_dense_anyD_masked(
    const int64_t *__restrict__ rows, const float *__restrict__ emb,
    const float *__restrict__ g_y, const float *__restrict__ g_emb,
    float *__restrict__ gW, float *__restrict__ gw1, int64_t B, int F, int D, int64_t N, float *__restrict__ gbias,
    const uint8_t *__restrict__ keep, const int32_t *__restrict__ fwidth) {
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  gather_fm_bwd_dense_anyD_blocks<true>(rows, emb, g_y, g_emb, gW, gw1, B, F, D, N, blk, nblk, keep, fwidth);
}

// ------------------------------------------------- next batch's table lines ----
// Touches the table rows the NEXT batch's lookup will gather (one dword per row is enough: the 128-byte line — a whole
// packed row — comes into the Infinity Cache), so that the next step's forward finds them on-die instead of in HBM.  Meant
// to run on a side stream under an MFMA-bound kernel of the CURRENT step (the tail's weight gradients leave the HBM idle for
// ~45 us).  `sink` is never non-null in practice; it keeps the loads alive.
__global__ __launch_bounds__(kBlock) void k_prefetch_rows(PrefetchJob j, float *__restrict__ sink) {
  prefetch_rows_blocks(j, (int)blockIdx.x, (int)gridDim.x, sink);
}

// ------------------------------------------------------- plain row gather ----
template <int LPR>
__global__ __launch_bounds__(kBlock) void k_gather_rows(
    const int64_t *__restrict__ idx, const float *__restrict__ W, float *__restrict__ out,
    int64_t n, int64_t N, int *err) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  constexpr int U = 4;  // row gathers in flight per lane
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const int64_t ntiles = (n + (int64_t)RS * U - 1) / ((int64_t)RS * U);
  int bad = 0;
  for (int64_t t = wave0; t < ntiles; t += nwaves) {
    int64_t row[U];
    bool act[U], ok[U];
    float4 v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = (t * U + k) * RS + r;
      act[k] = i < n;
      row[k] = act[k] ? idx[i] : 0;
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      ok[k] = act[k] && (uint64_t)row[k] < (uint64_t)N;
      bad |= (act[k] && !ok[k]);
      v[k] = ok[k] ? ld4(W + row[k] * D + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = (t * U + k) * RS + r;
      if (act[k]) st4(out + i * D + q * 4, v[k]);
    }
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

__global__ __launch_bounds__(kBlock) void k_gather_rows_anyD(
    const int64_t *__restrict__ idx, const float *__restrict__ W, float *__restrict__ out,
    int64_t n, int D, int64_t N, int *err) {
  // one thread per output element: coalesced for any D (D = 1 included)
  const int64_t total = n * D;
  int bad = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx[e / D];
    const bool ok = (uint64_t)row < (uint64_t)N;
    bad |= !ok;
    out[e] = ok ? W[row * D + e % D] : 0.f;
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// gW[idx[i],:] += g[i,:]; same LDS re-tiling as the dense FM backward.
template <int LPR>
__global__ __launch_bounds__(kBlock) void k_scatter_add_rows(
    const int64_t *__restrict__ idx, const float *__restrict__ g, float *__restrict__ gW,
    int64_t n, int64_t N) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  __shared__ float slab[kWavesPerBlock][kWave * 4];
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const int r = lane / LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + wib;
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const int64_t ntiles = (n + RS - 1) / RS;
  float *my = slab[wib];
  for (int64_t t = wave0; t < ntiles; t += nwaves) {
    const int64_t i = t * RS + r;
    int64_t row = -1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) {
      row = idx[i];
      if ((uint64_t)row >= (uint64_t)N) row = -1;
      // the tile's rows are consecutive in g: lane*4 floats from the tile start
      v = ld4(g + t * RS * D + lane * 4);
    }
    st4(my + lane * 4, v);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int el = j * kWave + lane;
      const int tr = el / D, tc = el % D;
      const int64_t trow = __shfl(row, tr * LPR);
      const float val = my[el];
      if (trow >= 0) atomicAdd(gW + trow * D + tc, val);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ __launch_bounds__(kBlock) void k_scatter_add_rows_anyD(
    const int64_t *__restrict__ idx, const float *__restrict__ g, float *__restrict__ gW,
    int64_t n, int D, int64_t N) {
  const int64_t total = n * D;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx[e / D];
    if ((uint64_t)row < (uint64_t)N) atomicAdd(gW + row * D + e % D, g[e]);
  }
}

// ------------------------------------------------------------- dispatch ------
// ---- the forward's one launcher ----
// the operands the float4 forward takes (the others go to the scalar kernel, or are refused)
inline bool fwd_float4_ok(int D, const float *W, int64_t ldw, const float *emb_out) {
  return vec_ok(D) && aligned16(W) && (ldw & 3) == 0 && aligned16(emb_out);
}
inline bool fwd_shfl(int F, int nit) { return nit > 0 && F <= kWave; }

// Chooses (LPR, NIT, SHFL), or the scalar kernel, and launches; the entry point has checked its arguments.  offsets == nullptr
// (the ids are row numbers) is for the float4 form only: k_gather_fm_fwd_anyD reads offsets[f] unconditionally.
// MASK: the kept-width kernels of the same (LPR, NIT, SHFL) choice, with keep / fwidth behind the common operands.
// XF: the PEP transforms, xf their operand; a threshold with columns (or a mask) the float4 loads cannot take sends the
// call to the scalar kernel.
inline bool xform_float4_ok(int XF, const Xform &xf) {
  if (XF == XF_SOFT) return xf.scs == 0 || (aligned16(xf.S) && (xf.srs & 3) == 0);
  if (XF == XF_MASK) return (reinterpret_cast<uintptr_t>(xf.M) & 3u) == 0;
  return true;
}
template <bool MASK = false, int XF = XF_NONE>
int launch_gather_fm_fwd(const char *name, const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw,
                         const float *w1, int64_t ldw1, const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out,
                         float *sum_out, int64_t B, int F, int D, int64_t N, int *err, void *stream,
                         const uint8_t *keep = nullptr, const int32_t *fwidth = nullptr, Xform xf = {}) {
  if (B == 0) return MI_OK;
  const int grid = grid_for_waves(B);
  if (fwd_float4_ok(D, W, ldw, emb_out) && xform_float4_ok(XF, xf)) {
    const int lpr = D / 4, nit = nit_for(F, lpr);
    const bool shfl = fwd_shfl(F, nit);
    if constexpr (XF != XF_NONE) {
      decltype(&k_gather_fm_fwd_xform<1, 0, false, XF>) kernel = nullptr;
#define CALL(LPR, NIT) kernel = shfl ? k_gather_fm_fwd_xform<LPR, NIT, true, XF> : k_gather_fm_fwd_xform<LPR, NIT, false, XF>
      MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
      MI_LAUNCH(name, kernel, grid, kBlock, stream, idx, offsets, W, w1, bias, emb_out, yfm_out, rows_out, B, F, N, ldw, ldw1,
                err, sum_out, xf);
    } else if constexpr (MASK) {
      decltype(&k_gather_fm_fwd_masked<1, 0, false>) kernel = nullptr;
#define CALL(LPR, NIT) kernel = shfl ? k_gather_fm_fwd_masked<LPR, NIT, true> : k_gather_fm_fwd_masked<LPR, NIT, false>
      MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
      MI_LAUNCH(name, kernel, grid, kBlock, stream, idx, offsets, W, w1, bias, emb_out, yfm_out, rows_out, B, F, N, ldw, ldw1,
                err, sum_out, keep, fwidth);
    } else {
      decltype(&k_gather_fm_fwd<1, 0, false>) kernel = nullptr;
#define CALL(LPR, NIT) kernel = shfl ? k_gather_fm_fwd<LPR, NIT, true> : k_gather_fm_fwd<LPR, NIT, false>
      MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
      MI_LAUNCH(name, kernel, grid, kBlock, stream, idx, offsets, W, w1, bias, emb_out, yfm_out, rows_out, B, F, N, ldw, ldw1,
                err, sum_out);
    }
  } else {
    if (!offsets) return MI_ERR_INVALID_ARG;
    if (ldw != D || ldw1 != 1) return MI_ERR_UNSUPPORTED;      // the scalar fallback reads the reference's two tensors only
    if constexpr (XF != XF_NONE)
      MI_LAUNCH(name, k_gather_fm_fwd_anyD_xform<XF>, grid, kBlock, stream, idx, offsets, W, w1, bias, emb_out, yfm_out,
                rows_out, B, F, D, N, err, sum_out, xf);
    else if constexpr (MASK)
      MI_LAUNCH(name, k_gather_fm_fwd_anyD_masked, grid, kBlock, stream, idx, offsets, W, w1, bias, emb_out, yfm_out, rows_out,
                B, F, D, N, err, sum_out, keep, fwidth);
    else
      MI_LAUNCH(name, k_gather_fm_fwd_anyD, grid, kBlock, stream, idx, offsets, W, w1, bias, emb_out, yfm_out, rows_out, B, F,
                D, N, err, sum_out);
  }
  return launch_status();
}

// mi_gather_fm_fwd_sum: its argument checks, then the launcher (also where mi_gather_fm_fwd_ride ends without a ride)
int gather_fm_fwd_sum(const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw, const float *w1, int64_t ldw1,
                      const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out, float *sum_out, int64_t B, int F,
                      int D, int64_t N, int *err, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0 || ldw < D || ldw1 < 1) return MI_ERR_INVALID_ARG;
  if (B > 0 && (!idx || !W || !w1 || !emb_out || !yfm_out)) return MI_ERR_INVALID_ARG;
  return launch_gather_fm_fwd("gather_fm_fwd", idx, offsets, W, ldw, w1, ldw1, bias, emb_out, yfm_out, rows_out, sum_out, B, F,
                              D, N, err, stream);
}

// the four threshold layouts of mi_xform_gather_*
inline bool soft_strides_ok(int64_t srs, int64_t scs, int D) {
  return (srs == 0 && (scs == 0 || scs == 1)) || (srs == 1 && scs == 0) || (srs == D && scs == 1);
}

template <int XF>
int gather_fm_xform_bwd_rows(const char *name, const int64_t *rows, const float *emb, const float *g_y, const float *g_emb,
                             float *gvals, float *g1vals, float *gbias, int64_t B, int F, int D, int64_t N, Xform xf,
                             SoftGrad sg, void *stream) {
  const int grid = grid_for_waves(B) + (gbias ? 1 : 0);      // + the workgroup that only sums the bias gradient
  if (vec_ok(D) && all_aligned16(emb, gvals, g_emb) && xform_float4_ok(XF, xf) &&
      (XF != XF_SOFT || xf.srs == 0 || xf.scs == 0 || aligned16(sg.svals))) {
    const int lpr = D / 4, nit = nit_for(F, lpr);
#define CALL(LPR, NIT)                                                                                              \
  MI_LAUNCH(name, (k_gather_fm_xform_bwd_rows<LPR, NIT, XF>), grid, kBlock, stream, rows, emb, g_y, g_emb, gvals, g1vals, B, \
            F, N, gbias, xf, sg)
    MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
  } else {
    MI_LAUNCH(name, k_gather_fm_xform_bwd_rows_anyD<XF>, grid, kBlock, stream, rows, emb, g_y, g_emb, gvals, g1vals, B, F, D,
              N, gbias, xf, sg);
  }
  return launch_status();
}
}  // namespace

extern "C" {

int mi_gather_fm_fwd_sum(const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw, const float *w1,
                         int64_t ldw1, const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out, float *sum_out,
                         int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err, void *stream) {
  return gather_fm_fwd_sum(idx, offsets, W, ldw, w1, ldw1, bias, emb_out, yfm_out, rows_out, sum_out, B, F, D, N, err, stream);
}

int mi_gather_fm_fwd_ride(const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw, const float *w1,
                          int64_t ldw1, const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out, float *sum_out,
                          int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err, const mi_tail_mask_ride *ride,
                          void *stream) {
  if (!ride) return gather_fm_fwd_sum(idx, offsets, W, ldw, w1, ldw1, bias, emb_out, yfm_out, rows_out, sum_out, B, F, D, N, err, stream);
  if (B < 0 || F < 0 || D <= 0 || N < 0 || ldw < D || ldw1 < 1) return MI_ERR_INVALID_ARG;
  MaskRide r;
  int64_t extra = 0;
  const int rc = mask_job(ride->seed, ride->nlayers, ride->salts, ride->ps, ride->lds, ride->bits, ride->M, ride->zero_buf,
                          ride->zero_floats, r.j, &extra);
  if (rc != MI_OK) return rc;
  r.seed = ride->seed;
  r.zero4 = reinterpret_cast<float4 *>(ride->zero_buf);
  r.nzero4 = ride->zero_floats / 4;
  r.aff.nl = 0;
  int aff_blocks = 0;
  if (ride->affine) {
    const mi_tail_affine_job *q = ride->affine;
    const int rc2 = affine_job(q->nlayers, q->widths, q->gamma, q->beta, q->running_mean, q->running_var, q->bias, q->eps, q->mu,
                               q->sc, q->be, q->rstd, r.aff, &aff_blocks);
    if (rc2 != MI_OK) return rc2;
  }
  const int lpr = D / 4, nit = vec_ok(D) ? nit_for(F, lpr) : 0;
  const bool fits = B > 0 && idx && W && w1 && emb_out && yfm_out && fwd_float4_ok(D, W, ldw, emb_out) &&
                    fwd_shfl(F, nit);      // (offsets may be NULL: slot lookups, mi_slot_fm_fwd's operands)
  // (mask workgroups: a quarter of what the job would take alone — each walks four strides — so the launch stays one wave
  //  of workgroups over the chip's slots)
  int nmask = (int)((extra + 3) / 4);
  if (nmask > 1024) nmask = 1024;
  r.mask_blocks = nmask;
  if (nmask + aff_blocks == 0 || !fits) {      // nothing to carry, or a gather form without the extra workgroups: two launches
    if (nmask + aff_blocks > 0) {
      MI_LAUNCH("tail_dropout_masks", k_mask_job, nmask + aff_blocks, kBlock, stream, r);
      const int st = launch_status();
      if (st != MI_OK) return st;
    }
    return gather_fm_fwd_sum(idx, offsets, W, ldw, w1, ldw1, bias, emb_out, yfm_out, rows_out, sum_out, B, F, D, N, err, stream);
  }
  const int ngather = grid_for_waves(B);
#define CALL(LPR, NIT)                                                                                         \
  MI_LAUNCH("gather_fm_fwd_ride", (k_gather_fm_fwd_ride<LPR, NIT>), ngather + nmask + aff_blocks, kBlock, stream, idx, offsets, \
            W, w1, bias, emb_out, yfm_out, rows_out, B, F, N, ldw, ldw1, err, sum_out, ngather, r)
  MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
  return launch_status();
}

int mi_gather_fm_fwd_ld(const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw, const float *w1,
                        int64_t ldw1, const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out,
                        int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err, void *stream) {
  return mi_gather_fm_fwd_sum(idx, offsets, W, ldw, w1, ldw1, bias, emb_out, yfm_out, rows_out, nullptr, B, F, D, N, err, stream);
}

int mi_gather_fm_fwd(const int64_t *idx, const int64_t *offsets, const float *W, const float *w1,
                     const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out,
                     int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err, void *stream) {
  return mi_gather_fm_fwd_ld(idx, offsets, W, D, w1, 1, bias, emb_out, yfm_out, rows_out, B, F, D, N, err, stream);
}

int mi_gather_fm_bwd_rows(const float *emb, const float *g_y, const float *g_emb, float *gvals,
                          float *g1vals, float *gbias, int64_t B, int32_t F, int32_t D, void *stream) {
  if (B < 0 || F < 0 || D <= 0) return MI_ERR_INVALID_ARG;
  if (B == 0) return MI_OK;
  if (!emb || !g_y || !gvals || !g1vals) return MI_ERR_INVALID_ARG;
  const int grid = grid_for_waves(B) + (gbias ? 1 : 0);      // + the workgroup that only sums the bias gradient
  if (vec_ok(D) && aligned16(emb) && aligned16(gvals) && (!g_emb || aligned16(g_emb))) {
    const int lpr = D / 4, nit = nit_for(F, lpr);
#define CALL(LPR, NIT)                                                                      \
  MI_LAUNCH("gather_fm_bwd_rows", (k_gather_fm_bwd_rows<LPR, NIT, false>), grid, kBlock, stream, \
            emb, g_y, g_emb, gvals, g1vals, B, F, (const int64_t *)nullptr, (int64_t)0, gbias)
    MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
  } else {
    MI_LAUNCH("gather_fm_bwd_rows", k_gather_fm_bwd_rows_anyD, grid, kBlock, stream, emb, g_y,
              g_emb, gvals, g1vals, B, F, D, gbias);
  }
  return launch_status();
}

int mi_gather_fm_bwd_dense(const int64_t *rows, const float *emb, const float *g_y,
                           const float *g_emb, float *gW, float *gw1, float *gbias, int64_t B,
                           int32_t F, int32_t D, int64_t N, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0) return MI_ERR_INVALID_ARG;
  if (B == 0) return MI_OK;
  if (!rows || !emb || !g_y || !gW || !gw1) return MI_ERR_INVALID_ARG;
  const int grid = grid_for_waves(B) + (gbias ? 1 : 0);      // + the workgroup that only sums the bias gradient
  if (vec_ok(D) && aligned16(emb) && (!g_emb || aligned16(g_emb))) {
    const int lpr = D / 4, nit = nit_for(F, lpr);
#define CALL(LPR, NIT)                                                                         \
  MI_LAUNCH("gather_fm_bwd_dense", (k_gather_fm_bwd_dense<LPR, NIT>), grid, kBlock, stream, rows, \
            emb, g_y, g_emb, gW, gw1, B, F, N, gbias)
    MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
  } else {
    MI_LAUNCH("gather_fm_bwd_dense", k_gather_fm_bwd_dense_anyD, grid, kBlock, stream, rows, emb,
              g_y, g_emb, gW, gw1, B, F, D, N, gbias);
  }
  return launch_status();
}

// ---- the kept-width forms (DeepFM on OptEmbed: a search candidate's eval lookup, the retraining table) ----
int mi_gather_fm_masked_fwd(const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw, const float *w1,
                            int64_t ldw1, const float *bias, const uint8_t *keep, const int32_t *fwidth, float *emb_out,
                            float *yfm_out, int64_t *rows_out, int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err,
                            void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0 || ldw < D || ldw1 < 1) return MI_ERR_INVALID_ARG;
  if (D > MI_GATHER_FM_MASKED_MAX_D) return MI_ERR_UNSUPPORTED;      // a kept width is one byte
  if (B > 0 && (!idx || !W || !w1 || !emb_out || !yfm_out)) return MI_ERR_INVALID_ARG;
  return launch_gather_fm_fwd<true>("gather_fm_masked_fwd", idx, offsets, W, ldw, w1, ldw1, bias, emb_out, yfm_out, rows_out,
                                    nullptr, B, F, D, N, err, stream, keep, fwidth);
}

int mi_gather_fm_masked_bwd_rows(const int64_t *rows, const uint8_t *keep, const int32_t *fwidth, const float *emb,
                                 const float *g_y, const float *g_emb, float *gvals, float *g1vals, float *gbias, int64_t B,
                                 int32_t F, int32_t D, int64_t N, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0) return MI_ERR_INVALID_ARG;
  if (D > MI_GATHER_FM_MASKED_MAX_D) return MI_ERR_UNSUPPORTED;
  if (B == 0) return MI_OK;
  if (!emb || !g_y || !gvals || !g1vals || (keep && !rows)) return MI_ERR_INVALID_ARG;
  const int grid = grid_for_waves(B) + (gbias ? 1 : 0);      // + the workgroup that only sums the bias gradient
  const KeptWidths kept = {rows, keep, fwidth, N};
  if (vec_ok(D) && aligned16(emb) && aligned16(gvals) && (!g_emb || aligned16(g_emb))) {
    const int lpr = D / 4, nit = nit_for(F, lpr);
#define CALL(LPR, NIT)                                                                                      \
  MI_LAUNCH("gather_fm_masked_bwd_rows", (k_gather_fm_bwd_rows<LPR, NIT, false, KeptWidths>), grid, kBlock, stream, emb, \
            g_y, g_emb, gvals, g1vals, B, F, (const int64_t *)nullptr, (int64_t)0, gbias, kept)
    MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
  } else {
    MI_LAUNCH("gather_fm_masked_bwd_rows", k_gather_fm_bwd_rows_anyD_masked, grid, kBlock, stream, emb, g_y, g_emb, gvals,
              g1vals, B, F, D, gbias, rows, keep, fwidth, N);
  }
  return launch_status();
}

int mi_gather_fm_masked_bwd_dense(const int64_t *rows, const uint8_t *keep, const int32_t *fwidth, const float *emb,
                                  const float *g_y, const float *g_emb, float *gW, float *gw1, float *gbias, int64_t B,
                                  int32_t F, int32_t D, int64_t N, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0) return MI_ERR_INVALID_ARG;
  if (D > MI_GATHER_FM_MASKED_MAX_D) return MI_ERR_UNSUPPORTED;
  if (B == 0) return MI_OK;
  if (!rows || !emb || !g_y || !gW || !gw1) return MI_ERR_INVALID_ARG;
  const int grid = grid_for_waves(B) + (gbias ? 1 : 0);      // + the workgroup that only sums the bias gradient
  if (vec_ok(D) && aligned16(emb) && (!g_emb || aligned16(g_emb))) {
    const int lpr = D / 4, nit = nit_for(F, lpr);
#define CALL(LPR, NIT)                                                                                        \
  MI_LAUNCH("gather_fm_masked_bwd_dense", (k_gather_fm_bwd_dense_masked<LPR, NIT>), grid, kBlock, stream, rows, \
            emb, g_y, g_emb, gW, gw1, B, F, N, gbias, keep, fwidth)
    MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
  } else {
    MI_LAUNCH("gather_fm_masked_bwd_dense", k_gather_fm_bwd_dense_anyD_masked, grid, kBlock, stream, rows, emb, g_y, g_emb,
              gW, gw1, B, F, D, N, gbias, keep, fwidth);
  }
  return launch_status();
}

// ---- the PEP forms (DeepFM on PepEmbeeding: the threshold search; on RetrainPepEmbedding: the retraining table) ----
int mi_gather_fm_soft_fwd(const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw, const float *w1,
                          int64_t ldw1, const float *bias, const float *S, int64_t srs, int64_t scs, float *emb_out,
                          float *yfm_out, int64_t *rows_out, int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err,
                          void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0 || ldw < D || ldw1 < 1 || !soft_strides_ok(srs, scs, D)) return MI_ERR_INVALID_ARG;
  if (B > 0 && (!idx || !W || !w1 || !S || !emb_out || !yfm_out)) return MI_ERR_INVALID_ARG;
  const Xform xf = {S, srs, scs, nullptr};
  return launch_gather_fm_fwd<false, XF_SOFT>("gather_fm_soft_fwd", idx, offsets, W, ldw, w1, ldw1, bias, emb_out, yfm_out,
                                              rows_out, nullptr, B, F, D, N, err, stream, nullptr, nullptr, xf);
}

int mi_gather_fm_elemmask_fwd(const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw, const float *w1,
                              int64_t ldw1, const float *bias, const uint8_t *M, float *emb_out, float *yfm_out,
                              int64_t *rows_out, int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0 || ldw < D || ldw1 < 1) return MI_ERR_INVALID_ARG;
  if (B > 0 && (!idx || !W || !w1 || !M || !emb_out || !yfm_out)) return MI_ERR_INVALID_ARG;
  const Xform xf = {nullptr, 0, 0, M};
  return launch_gather_fm_fwd<false, XF_MASK>("gather_fm_elemmask_fwd", idx, offsets, W, ldw, w1, ldw1, bias, emb_out, yfm_out,
                                              rows_out, nullptr, B, F, D, N, err, stream, nullptr, nullptr, xf);
}

int64_t mi_gather_fm_soft_bwd_workspace_elems(int64_t B, int32_t D, int64_t srs) {
  if (B <= 0 || D <= 0 || srs != 0) return 0;
  return (int64_t)grid_for_waves(B) * D + 1;      // the workgroups' column sums, then the ticket
}

int mi_gather_fm_soft_bwd_rows(const int64_t *rows, const float *S, int64_t srs, int64_t scs, const float *emb,
                               const float *g_y, const float *g_emb, float *gvals, float *svals, float *g1vals, float *gbias,
                               float *workspace, int32_t armed, int64_t B, int32_t F, int32_t D, int64_t N, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0 || !soft_strides_ok(srs, scs, D)) return MI_ERR_INVALID_ARG;
  if (D > kJoinMaxD) return MI_ERR_UNSUPPORTED;
  if (B == 0 || F == 0) {      // no lookup: the summed forms still owe their zeros
    if (srs == 0 && svals && hipMemsetAsync(svals, 0, sizeof(float) * (scs ? D : 1), (hipStream_t)stream) != hipSuccess)
      return MI_ERR_LAUNCH;
    if (B == 0) return MI_OK;
  }
  if (!rows || !S || !emb || !g_y || !gvals || !svals || !g1vals || (srs == 0 && !workspace)) return MI_ERR_INVALID_ARG;
  const Xform xf = {S, srs, scs, nullptr};
  SoftGrad sg = {svals, nullptr, nullptr};
  if (srs == 0) {
    sg.part = workspace;
    sg.ticket = reinterpret_cast<unsigned *>(workspace + (int64_t)grid_for_waves(B) * D);
    if (!armed && hipMemsetAsync(sg.ticket, 0, sizeof(unsigned), (hipStream_t)stream) != hipSuccess) return MI_ERR_LAUNCH;
  }
  return gather_fm_xform_bwd_rows<XF_SOFT>("gather_fm_soft_bwd_rows", rows, emb, g_y, g_emb, gvals, g1vals, gbias, B, F, D, N,
                                           xf, sg, stream);
}

int mi_gather_fm_elemmask_bwd_rows(const int64_t *rows, const uint8_t *M, const float *emb, const float *g_y,
                                   const float *g_emb, float *gvals, float *g1vals, float *gbias, int64_t B, int32_t F,
                                   int32_t D, int64_t N, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0) return MI_ERR_INVALID_ARG;
  if (D > kJoinMaxD) return MI_ERR_UNSUPPORTED;
  if (B == 0) return MI_OK;
  if (!rows || !M || !emb || !g_y || !gvals || !g1vals) return MI_ERR_INVALID_ARG;
  const Xform xf = {nullptr, 0, 0, M};
  return gather_fm_xform_bwd_rows<XF_MASK>("gather_fm_elemmask_bwd_rows", rows, emb, g_y, g_emb, gvals, g1vals, gbias, B, F, D,
                                           N, xf, SoftGrad{}, stream);
}

int mi_prefetch_rows(const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw, const float *w1, int64_t ldw1,
                     int64_t B, int32_t F, int64_t N, void *stream) {
  if (B < 0 || F <= 0 || N < 0 || ldw <= 0) return MI_ERR_INVALID_ARG;
  if (B == 0) return MI_OK;
  if (!idx || !W) return MI_ERR_INVALID_ARG;
  PrefetchJob j;
  if (!prefetch_job(idx, offsets, W, ldw, w1, ldw1, B, F, N, j)) return MI_OK;
  int64_t grid = (j.n + kBlock - 1) / kBlock;
  if (grid > kMaxGrid) grid = kMaxGrid;
  MI_LAUNCH("prefetch_rows", k_prefetch_rows, (int)grid, kBlock, stream, j, (float *)nullptr);
  return launch_status();
}

int mi_gather_rows_fwd(const int64_t *idx, const float *W, float *out, int64_t n, int32_t D,
                       int64_t N, int32_t *err, void *stream) {
  if (n < 0 || D <= 0 || N < 0) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!idx || !W || !out) return MI_ERR_INVALID_ARG;
  if (vec_ok(D) && aligned16(W) && aligned16(out)) {
    const int lpr = D / 4;
    const int64_t tiles = (n + (int64_t)(kWave / lpr) * 4 - 1) / ((int64_t)(kWave / lpr) * 4);
    const int grid = grid_for_waves(tiles);
#define CALL(LPR) \
  MI_LAUNCH("gather_rows", (k_gather_rows<LPR>), grid, kBlock, stream, idx, W, out, n, N, err)
    MI_DISPATCH_LPR(lpr, CALL)
#undef CALL
  } else {
    MI_LAUNCH("gather_rows", k_gather_rows_anyD, grid_for_waves(((int64_t)n * D + kWave - 1) / kWave),
              kBlock, stream, idx, W, out, n, D, N, err);
  }
  return launch_status();
}

int mi_scatter_add_rows(const int64_t *idx, const float *g, float *gW, int64_t n, int32_t D,
                        int64_t N, void *stream) {
  if (n < 0 || D <= 0 || N < 0) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!idx || !g || !gW) return MI_ERR_INVALID_ARG;
  if (vec_ok(D) && aligned16(g)) {
    const int lpr = D / 4;
    const int64_t tiles = (n + (kWave / lpr) - 1) / (kWave / lpr);
    const int grid = grid_for_waves(tiles);
#define CALL(LPR) \
  MI_LAUNCH("scatter_add_rows", (k_scatter_add_rows<LPR>), grid, kBlock, stream, idx, g, gW, n, N)
    MI_DISPATCH_LPR(lpr, CALL)
#undef CALL
  } else {
    MI_LAUNCH("scatter_add_rows", k_scatter_add_rows_anyD,
              grid_for_waves(((int64_t)n * D + kWave - 1) / kWave), kBlock, stream, idx, g, gW, n, D, N);
  }
  return launch_status();
}

// ---- the same two kernels over the packed rows a sharded lookup received (route.hip) ----
int mi_slot_fm_fwd(const int64_t *slot, const float *buf, int64_t nrows, const float *bias,
                   float *emb_out, float *yfm_out, int64_t B, int32_t F, int32_t D, int32_t *err,
                   void *stream) {
  if (B < 0 || F < 0 || D <= 0 || nrows < 0) return MI_ERR_INVALID_ARG;
  if (B == 0) return MI_OK;
  if (!slot || !buf || !emb_out || !yfm_out) return MI_ERR_INVALID_ARG;
  if (!fwd_float4_ok(D, buf, D + 4, emb_out)) return MI_ERR_UNSUPPORTED;
  return launch_gather_fm_fwd("slot_fm_fwd", slot, nullptr, buf, D + 4, buf + D, D + 4, bias, emb_out, yfm_out, nullptr,
                              nullptr, B, F, D, nrows, err, stream);
}

int mi_slot_fm_bwd(const int64_t *slot, const float *emb, const float *g_y, const float *g_emb,
                   float *gbuf, float *gbias, int64_t nslot, int64_t B, int32_t F, int32_t D, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || nslot < 0) return MI_ERR_INVALID_ARG;
  if (nslot > 0 && !gbuf) return MI_ERR_INVALID_ARG;
  if (!vec_ok(D) || !aligned16(gbuf) || (emb && !aligned16(emb)) || (g_emb && !aligned16(g_emb)))
    return MI_ERR_UNSUPPORTED;
  // padding slots must read as zero gradients at the owner
  if (nslot > 0 &&
      hipMemsetAsync(gbuf, 0, (size_t)nslot * (D + 4) * sizeof(float), (hipStream_t)stream) != hipSuccess)
    return MI_ERR_LAUNCH;
  if (B == 0) return MI_OK;
  if (!slot || !emb || !g_y) return MI_ERR_INVALID_ARG;
  const int grid = grid_for_waves(B) + (gbias ? 1 : 0);      // + the workgroup that only sums the bias gradient
  const int lpr = D / 4, nit = nit_for(F, lpr);
#define CALL(LPR, NIT)                                                                         \
  MI_LAUNCH("slot_fm_bwd", (k_gather_fm_bwd_rows<LPR, NIT, true>), grid, kBlock, stream, emb,  \
            g_y, g_emb, gbuf, (float *)nullptr, B, F, slot, nslot, gbias)
  MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
  return launch_status();
}

int64_t mi_slot_fm_bwd_segments_workspace_elems(int64_t B, int32_t F, int32_t D) {
  if (B < 0 || F < 0 || D <= 0) return 0;
  return B * F * ((int64_t)D + 1) + 3;           // per-lookup rows [n, D], first-order values [n], (+3: 16-byte slack)
}

int mi_slot_fm_bwd_segments(const int32_t *segments, const float *emb, const float *g_y, const float *g_emb,
                            float *workspace, float *gbuf, float *gbias, int64_t nslot, int64_t B, int32_t F,
                            int32_t D, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || nslot < 0) return MI_ERR_INVALID_ARG;
  if (!gbuf || (nslot > 0 && !segments)) return MI_ERR_INVALID_ARG;
  const int64_t n = B * F;
  if (n >= (1ll << 31)) return MI_ERR_UNSUPPORTED;
  if (n > 0 && (!emb || !g_y || !workspace || !segments)) return MI_ERR_INVALID_ARG;
  if (!vec_ok(D) || !aligned16(gbuf) || !aligned16(workspace) || (emb && !aligned16(emb)) || (g_emb && !aligned16(g_emb)))
    return MI_ERR_UNSUPPORTED;
  float *gvals = workspace, *g1vals = workspace + n * D;
  if (n > 0) {
    const int rc = mi_gather_fm_bwd_rows(emb, g_y, g_emb, gvals, g1vals, gbias, B, F, D, stream);
    if (rc != MI_OK) return rc;
  } else if (gbias && hipMemsetAsync(gbias, 0, sizeof(float), (hipStream_t)stream) != hipSuccess) {
    return MI_ERR_LAUNCH;
  }
  const int lpr = D / 4;
  const int64_t rs = kWave / lpr;
  const int grid = grid_for_waves((nslot + 1 + rs - 1) / rs);
#define CALL(LPR) \
  MI_LAUNCH("slot_fm_bwd_segments", (k_segment_sum<LPR>), grid, kBlock, stream, segments, gvals, g1vals, gbuf, nslot, n)
  MI_DISPATCH_LPR(lpr, CALL)
#undef CALL
  return launch_status();
}

}  // extern "C"
