// gather_fm_walk.hpp — what the fused lookup + FM kernels share (gather_fm.hip: one table; gather_fm_dual.hip: two
// tables combined): the single-table forward walk over a sample's fields in its float4 and its scalar form, the float4
// helpers of both files' forward and row-form backward, the bias-gradient workgroup and the (LPR, NIT) dispatch.
//
// Both walks serve ONE table.  With the two-table lookup as a row source of the float4 walk every resource figure
// of the single-table kernels held, but y_fm of the two-table kernel moved in the last bit (its own body has sum e^2
// as packed multiplies and adds behind a loop unswitched on the combine op; in the walk it becomes the single-table
// kernels' fused multiply-add chain), so gather_fm_dual.hip keeps its forward bodies on the helpers below
// (DESIGN.md §6k).
//
// Everything here is local to the translation unit, like the kernels of the two files: Xform is an argument type of
// gather_fm.hip's kernels.
#pragma once
#include "common.hpp"
#include "dual_xform.hpp"

namespace {
using namespace mi;

// ------------------------------------------------------------ small helpers ----
// dE_bf = g_emb_bf + g_b (S_b - e_bf): the lookup's gradient row through the FM term (src/models/deepfm.py:91-92)
__device__ __forceinline__ float4 fm_grad_row(float4 ge, float gy, float4 S, float4 e) {
  return make_float4(ge.x + gy * (S.x - e.x), ge.y + gy * (S.y - e.y), ge.z + gy * (S.z - e.z), ge.w + gy * (S.w - e.w));
}

// keep_prefix: v with the columns at or past kw zeroed; the lane's float4 holds columns q*4 .. q*4+3.  ONE vector
// select, not four scalar ones: behind scalar selects the compiler turns dot4(v, v) into packed multiplies and adds
// instead of the unmasked kernels' fused multiply-add chain, and y_fm under keep = D then differs from the unmasked
// kernel's in the last bit (tests/test_optembed_deepfm_gpu.py holds the two to equal bits).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 keep_prefix(float4 v, int q, int kw) {
  const i32x4 col = {0, 1, 2, 3};
  const i32x4 c = (col + q * 4) < kw;
  f32x4 x = {v.x, v.y, v.z, v.w};
  x = c ? x : (f32x4)(0.f);
  return make_float4(x.x, x.y, x.z, x.w);
}
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// The element transforms of the PEP tables (mi_gather_fm_soft_* / mi_gather_fm_elemmask_*), XF of dual_xform.hpp:
//   XF_SOFT: emb[b, f, d] = soft_(W[row, d], S[row * srs + d * scs])  (PepEmbeeding; (srs, scs) as in mi_xform_gather_*:
//            (0,0) global, (0,1) dimension, (1,0) feature, (D,1) feature_dim)
//   XF_MASK: emb[b, f, d] = M[row, d] ? W[row, d] : +0                 (RetrainPepEmbedding.mask, one byte per element)
// The first-order term is not transformed.  soft_ / sigmoidf_ are the functions k_xform_gather_fwd (embed.hip) applies, so
// emb has that lookup's bits.
struct Xform {
  const float *S;
  int64_t srs, scs;
  const uint8_t *M;
};
// the lane's four threshold logits of `row` (columns q*4 .. q*4+3): one float4 where the threshold has columns, one scalar
// where it has not
__device__ __forceinline__ float4 thr4(const Xform &x, int64_t row, int q) {
  if (x.scs) return ld4(x.S + row * x.srs + q * 4);
  const float s = x.S[row * x.srs];
  return make_float4(s, s, s, s);
}
__device__ __forceinline__ float4 soft4(float4 w, float4 s) {
  return make_float4(soft_(w.x, s.x), soft_(w.y, s.y), soft_(w.z, s.z), soft_(w.w, s.w));
}
// the lane's four mask bytes as one word: those of the elements at o .. o+3, o = row D + q 4 (D % 4 == 0 and M 4-byte
// aligned: the launchers check)
__device__ __forceinline__ uint32_t mask4(const uint8_t *__restrict__ M, int64_t o) {
  return *reinterpret_cast<const uint32_t *>(M + o);
}

__device__ __forceinline__ float4 keep_bytes(float4 v, uint32_t m) {
  return make_float4((m & 0xffu) ? v.x : 0.f, (m & 0xff00u) ? v.y : 0.f, (m & 0xff0000u) ? v.z : 0.f,
                     (m & 0xff000000u) ? v.w : 0.f);
}

// ---------------------------------------------------------------- forward ----
// SHFL (F <= 64): the sample's F ids arrive by ONE coalesced load (lane l < F takes idx[b, l] + offsets[l]) and reach
// the row slots by shuffles — one dependent vector-memory instruction in front of the row gathers instead of NIT id
// loads plus NIT offset loads (measured -0.45 us of 5.8 at the headline shape, tools/probe_gather3.hip) — and
// rows_out is one coalesced store.  emb is written with non-temporal stores: nobody in this kernel reads it back, and
// what is not left dirty in L2 is not written back at the kernel's end (-0.4 us).
// ldw / ldw1: floats between consecutive rows of W / w1.  (D, 1) for the reference's two tensors; (32, 32) when both
// are views of ONE packed table fp32[N, 32] = {16 embedding floats, w1, padding} — a lookup then touches one 128-B
// line instead of two unrelated 64-B sectors (DeepFM.pack_tables()); (D + 4, D + 4) for the packed rows a sharded
// lookup received (route.hip).
// (SHFL is ignored by the generic NIT = 0 form.)
// (blk of nblk: the workgroups of the launch that gather — a launch may carry others, k_gather_fm_fwd_ride)
// MASK: the kept-width form.  The keep[row] byte is loaded in the SAME step as the row gather it belongs to (both need
// only the row id: one round trip, not two; the LPR lanes of a row slot read the same byte, one request), fwidth[f]
// arrives like offsets[f] — in SHFL form once per wave, next to offsets[lane], and by shuffle from there.  Every row is
// gathered whole whatever its width: the gather does not wait for the byte.  Without MASK none of this is compiled.
// XF (XF_SOFT / XF_MASK, never together with MASK): the row's threshold logits or mask bytes are loaded in the same step
// as the row as well — they, too, need only the row id — and applied before the row is stored and summed.
// (NIT > 0 and NIT = 0 stay two bodies: merged, the compiler contracts sum e^2 differently: y_fm moves in the last bit)
template <int LPR, int NIT, bool SHFL, bool MASK = false, int XF = XF_NONE>
__device__ __forceinline__ void gather_fm_fwd_blocks(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets,
    const float *__restrict__ W, const float *__restrict__ w1, const float *__restrict__ bias,
    float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int64_t N, int64_t ldw, int64_t ldw1, int *err, float *__restrict__ sum_out, int blk, int nblk,
    const uint8_t *__restrict__ keep = nullptr, const int32_t *__restrict__ fwidth = nullptr, Xform xf = {}) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blk * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
  const float bv = bias ? bias[0] : 0.f;
  int bad = 0;
  int64_t myoff = 0;
  if constexpr (SHFL) myoff = (offsets && lane < F) ? offsets[lane] : 0;
  int myfw = D;
  if constexpr (SHFL && MASK) myfw = (fwidth && lane < F) ? fwidth[lane] : D;

  for (int64_t b = wave0; b < B; b += nwaves) {
    float4 S = make_float4(0.f, 0.f, 0.f, 0.f);
    float ss = 0.f, lin = 0.f;
    const int64_t base = b * F;
    if constexpr (NIT > 0) {
      int64_t row[NIT];
      bool act[NIT], ok[NIT];
      float4 v[NIT];
      float l[NIT];
      int kw[NIT];      // (MASK only) the field's width, then the lookup's kept width
      float4 th[NIT];   // (XF_SOFT only) the row's threshold logits
      uint32_t mb[NIT]; // (XF_MASK only) the row's mask bytes
      if constexpr (SHFL) {
        const int64_t mine = lane < F ? idx[base + lane] + myoff : 0;
        if (rows_out && lane < F) rows_out[base + lane] = mine;
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
          const int f = r + k * RS;
          act[k] = f < F;
          row[k] = __shfl(mine, f & 63);
          if constexpr (MASK) kw[k] = __shfl(myfw, f & 63);
        }
      } else {
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
          const int f = r + k * RS;
          act[k] = f < F;
          row[k] = act[k] ? idx[base + f] + (offsets ? offsets[f] : 0) : 0;
          if constexpr (MASK) kw[k] = (act[k] && fwidth) ? fwidth[f] : D;
        }
      }
#pragma unroll
      for (int k = 0; k < NIT; ++k) {
        ok[k] = act[k] && (uint64_t)row[k] < (uint64_t)N;
        bad |= (act[k] && !ok[k]);
        v[k] = ok[k] ? ld4(W + row[k] * ldw + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        l[k] = (ok[k] && q == 0) ? w1[row[k] * ldw1] : 0.f;
        if constexpr (MASK) kw[k] = imin(kw[k], (ok[k] && keep) ? (int)keep[row[k]] : D);
        if constexpr (XF == XF_SOFT) th[k] = ok[k] ? thr4(xf, row[k], q) : make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (XF == XF_MASK) mb[k] = ok[k] ? mask4(xf.M, row[k] * D + q * 4) : 0u;
      }
#pragma unroll
      for (int k = 0; k < NIT; ++k) {
        const int f = r + k * RS;
        if constexpr (MASK) v[k] = keep_prefix(v[k], q, kw[k]);
        if constexpr (XF == XF_SOFT) v[k] = soft4(v[k], th[k]);
        if constexpr (XF == XF_MASK) v[k] = keep_bytes(v[k], mb[k]);
        if (act[k]) {
          st4_nt(emb + (base + f) * D + q * 4, v[k]);
          if (!SHFL && rows_out && q == 0) rows_out[base + f] = row[k];
        }
        S.x += v[k].x; S.y += v[k].y; S.z += v[k].z; S.w += v[k].w;
        ss += dot4(v[k], v[k]);
        lin += l[k];
      }
    } else {
      for (int f = r; f < F; f += RS) {
        const int64_t row = idx[base + f] + (offsets ? offsets[f] : 0);
        const bool ok = (uint64_t)row < (uint64_t)N;
        bad |= !ok;
        float4 v = ok ? ld4(W + row * ldw + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (MASK) {
          const int kb = (ok && keep) ? (int)keep[row] : D;
          v = keep_prefix(v, q, imin(kb, fwidth ? fwidth[f] : D));
        }
        if constexpr (XF == XF_SOFT) { if (ok) v = soft4(v, thr4(xf, row, q)); }
        if constexpr (XF == XF_MASK) v = keep_bytes(v, ok ? mask4(xf.M, row * D + q * 4) : 0u);
        if (ok && q == 0) lin += w1[row * ldw1];
        st4(emb + (base + f) * D + q * 4, v);
        if (rows_out && q == 0) rows_out[base + f] = row;
        S.x += v.x; S.y += v.y; S.z += v.z; S.w += v.w;
        ss += dot4(v, v);
      }
    }
    S = slot_sum<LPR>(S);
    // sum_f e[b, f, :] — what the FM backward needs besides the rows themselves (dE_bf = g_b (S_b - e_bf)): kept when the
    // backward runs in the epilogue of the MLP's first input-gradient product (tail.hip), which sees a tile of 6-7 fields
    // of a sample and cannot re-derive the sum over all F
    if (sum_out && r == 0) st4(sum_out + b * D + q * 4, S);
    float t = (r == 0 ? dot4(S, S) : 0.f) - ss;
    t = wave_sum(0.5f * t + lin);
    if (lane == 0) yfm[b] = t + bv;
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// Any D (scalar accesses): wave per sample, lanes stride over d.
template <bool MASK, int XF = XF_NONE>
__device__ __forceinline__ void gather_fm_fwd_anyD_blocks(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets,
    const float *__restrict__ W, const float *__restrict__ w1, const float *__restrict__ bias,
    float *__restrict__ emb, float *__restrict__ yfm, int64_t *__restrict__ rows_out,
    int64_t B, int F, int D, int64_t N, int *err, float *__restrict__ sum_out,
    const uint8_t *__restrict__ keep = nullptr, const int32_t *__restrict__ fwidth = nullptr, Xform xf = {}) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const float bv = bias ? bias[0] : 0.f;
  int bad = 0;
  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    float t = 0.f;
    for (int d0 = 0; d0 < D || d0 == 0; d0 += kWave) {
      const int d = d0 + lane;
      float S = 0.f, ss = 0.f;
      for (int f = 0; f < F; ++f) {
        const int64_t row = idx[base + f] + offsets[f];
        const bool ok = (uint64_t)row < (uint64_t)N;
        bad |= !ok;
        if (d0 == 0 && lane == 0) {
          if (ok) t += w1[row];
          if (rows_out) rows_out[base + f] = row;
        }
        if (d < D) {
          float v = ok ? W[row * D + d] : 0.f;
          if constexpr (MASK) {
            const int kb = (ok && keep) ? (int)keep[row] : D;
            v = d < imin(kb, fwidth ? fwidth[f] : D) ? v : 0.f;
          }
          if constexpr (XF == XF_SOFT) { if (ok) v = soft_(v, xf.S[row * xf.srs + d * xf.scs]); }
          if constexpr (XF == XF_MASK) v = (ok && xf.M[row * D + d]) ? v : 0.f;
          emb[(base + f) * D + d] = v;
          S += v;
          ss += v * v;
        }
      }
      if (sum_out && d < D) sum_out[b * D + d] = S;
      t += 0.5f * (S * S - ss);
    }
    t = wave_sum(t);
    if (lane == 0) yfm[b] = t + bv;
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// bias gradient = sum_b g_y[b] (the bias is added to every sample's y_fm): ONE EXTRA workgroup of a backward launch —
// workgroup 0, the first one dispatched; the launcher adds it when gbias is given — adds it up in a fixed order
// (deterministic, no atomics, no zero-fill, no separate launch) and does nothing else.  Round 2 had workgroup 0 sum it
// with one scalar load per thread and trip IN FRONT of its share of the rows: a 3.4 us kernel then ended 1.2 us late on
// that one workgroup (and at B = 65 536 the 256 dependent trips doubled the kernel: 55 -> 105 us,
// tools/probe_gather3.hip).  Now: float4 loads, four independent partial sums per thread, the other workgroups' ids
// shifted down by one.  Returns true in that workgroup; blk / nblk = this workgroup's index among, and the number of,
// the workgroups that share the rows.
__device__ __forceinline__ bool bias_grad_block(const float *__restrict__ g_y, int64_t B, float *__restrict__ gbias,
                                                int &blk, int &nblk) {
  blk = blockIdx.x;
  nblk = gridDim.x;
  if (!gbias) return false;
  nblk = gridDim.x - 1;
  blk = (int)blockIdx.x - 1;
  if (blockIdx.x != 0) return false;
  __shared__ float part[kWavesPerBlock];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const int64_t B4 = aligned16(g_y) ? (B & ~(int64_t)3) : 0;
  int64_t b = (int64_t)threadIdx.x * 4;
  for (; b + 3 * kBlock * 4 < B4; b += 4 * kBlock * 4) {         // four float4 loads in flight per thread
    const float4 a0 = ld4(g_y + b), a1 = ld4(g_y + b + kBlock * 4), a2 = ld4(g_y + b + 2 * kBlock * 4),
                 a3 = ld4(g_y + b + 3 * kBlock * 4);
    s0 += (a0.x + a0.y) + (a0.z + a0.w);
    s1 += (a1.x + a1.y) + (a1.z + a1.w);
    s2 += (a2.x + a2.y) + (a2.z + a2.w);
    s3 += (a3.x + a3.y) + (a3.z + a3.w);
  }
  for (; b < B4; b += kBlock * 4) {
    const float4 a0 = ld4(g_y + b);
    s0 += (a0.x + a0.y) + (a0.z + a0.w);
  }
  for (int64_t t = B4 + threadIdx.x; t < B; t += kBlock) s1 += g_y[t];
  float s = wave_sum((s0 + s1) + (s2 + s3));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int j = 0; j < kWavesPerBlock; ++j) t += part[j];
    gbias[0] = t;
  }
  return true;
}
// ------------------------------------------------------------- dispatch ------
inline int nit_for(int F, int LPR) {
  const int RS = kWave / LPR;
  const int n = (F + RS - 1) / RS;
  return n <= 4 ? n : 0;
}

}  // namespace

// Expands `CALL(LPR, NIT)` for the run-time (lpr, nit) pair.
#define MI_DISPATCH_LPR_NIT(lpr, nit, CALL)                               \
  switch (lpr) {                                                          \
    case 1: MI_DISPATCH_NIT(1, nit, CALL); break;                         \
    case 2: MI_DISPATCH_NIT(2, nit, CALL); break;                         \
    case 4: MI_DISPATCH_NIT(4, nit, CALL); break;                         \
    case 8: MI_DISPATCH_NIT(8, nit, CALL); break;                         \
    case 16: MI_DISPATCH_NIT(16, nit, CALL); break;                       \
    case 32: MI_DISPATCH_NIT(32, nit, CALL); break;                       \
    case 64: MI_DISPATCH_NIT(64, nit, CALL); break;                       \
    default: return MI_ERR_UNSUPPORTED;                                   \
  }
#define MI_DISPATCH_NIT(LPR, nit, CALL) \
  switch (nit) {                        \
    case 1: CALL(LPR, 1); break;        \
    case 2: CALL(LPR, 2); break;        \
    case 3: CALL(LPR, 3); break;        \
    case 4: CALL(LPR, 4); break;        \
    default: CALL(LPR, 0); break;       \
  }
