// gather_fm_quant.hip — DeepFM on the quantised tables: the lookup
//   row = idx[b, f] + offsets[f],   emb[b, f, :] = dequant(Wq[row, :])                  (PTQEmb_Int / PTQEmb_Fp16), or
//                                   emb[b, f, :] = stochastic_round(W[row, :] / scale) * scale      (QAT_EmbInt)
// fused with the FM second-order term and the first-order bag (src/models/deepfm.py:88-98 over
// src/models/embeddings/ptq_emb.py:7-96 / qat_emb.py:16-45,117-119), and the QAT lookup's row-form backward with the
// scale gradient of qat_emb.py:49-84.
//
// Forward mapping: gather_fm.hip's — one wave per sample, LPR = D / 4 lanes per row (lane q holds columns 4q .. 4q+3),
// RS = 64 / LPR rows per wave-instruction, the F ids by one coalesced load and shuffles when F <= 64, up to four row steps
// with all their loads in flight, emb stored non-temporally.  What differs is the row source: a lane's four codes are ONE
// 32-bit word (int8), ONE 64-bit word (int16, fp16) or ONE 16-bit word (packed int4) of an 8- to 32-byte row at D = 16, the source is a template
// parameter.  The dequantisation is k_gather_rows_q's (embed.hip), the rounding is sr_round.hpp's, so emb has the bits
// of mi_gather_rows_quant / mi_qat_gather_fwd over idx + offsets.
// The walks are bodies of this file on the helpers of gather_fm_walk.hpp: the shared forward walk is not touched, so no
// kernel of gather_fm.hip / gather_fm_dual.hip is compiled from other text than before.
//
// Backward (QAT): no float atomics.  One row-form launch over the saved emb writes the straight-through value rows;
// the scale gradient is summed per thread, per workgroup and then over the grid in a fixed order by the last workgroup
// to arrive (grid_join, common.hpp).
#include <hip/hip_fp16.h>

#include "common.hpp"
#include "gather_fm_walk.hpp"
#include "sr_round.hpp"

namespace {
using namespace mi;

// the row sources: the first three are the qtype codes of mi_gather_rows_quant, Q_INT4 is MI_QTYPE_INT4_PACKED (two codes
// per byte, PTQEmb_Int(n_bits=4, packed=True): the layout of mi_gather_rows_int4)
enum { Q_FP16 = 1, Q_INT8 = 2, Q_INT16 = 3, Q_QAT = 4, Q_INT4 = MI_QTYPE_INT4_PACKED };

constexpr int kQatBwdMaxD = MI_GATHER_FM_QAT_BWD_MAX_D;

struct QSrc {
  const void *W;          // fp16 / int8 / int16 codes, or the fp32 table (Q_QAT)
  const float *scale;     // device scalar (absent for fp16)
  const void *zero;       // device scalar in the table's integer type (integer tables)
  // Q_QAT: the arguments of sr_round
  float qmin, qmax;
  const float *prob;
  const int64_t *seed;
  int64_t salt;
};

template <int QT>
__device__ __forceinline__ float src_scale(const QSrc &s) { return QT == Q_FP16 ? 1.f : s.scale[0]; }
template <int QT>
__device__ __forceinline__ int src_zero(const QSrc &s) {
  if constexpr (QT == Q_INT8 || QT == Q_INT4) return (int)reinterpret_cast<const int8_t *>(s.zero)[0];      // (int4: never packed)
  else if constexpr (QT == Q_INT16) return (int)reinterpret_cast<const int16_t *>(s.zero)[0];
  else return 0;
}

// what a lane holds of a row between the gather and the dequantisation: its four codes as loaded
template <int QT> struct Raw { using T = uint2; };                 // int16 / fp16: one 64-bit word
template <> struct Raw<Q_INT8> { using T = uint32_t; };            // int8: one 32-bit word
template <> struct Raw<Q_QAT> { using T = float4; };
template <> struct Raw<Q_INT4> { using T = uint32_t; };            // packed int4: one 16-bit word, held widened

// the lane's four codes of the elements o .. o+3 (o = row D + 4 q; D % 4 == 0 and the table's base aligned to four codes:
// the launchers check)
template <int QT>
__device__ __forceinline__ typename Raw<QT>::T load_raw(const void *W, int64_t o) {
  if constexpr (QT == Q_INT8) return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const int8_t *>(W) + o);
  else if constexpr (QT == Q_QAT) return ld4(reinterpret_cast<const float *>(W) + o);
  else if constexpr (QT == Q_INT4)      // o is a multiple of four: byte o / 2 is even
    return (uint32_t)*reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(W) + (o >> 1));
  else return *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(W) + o);
}

__device__ __forceinline__ float deq(int code, int zero, float sc) { return (float)(code - zero) * sc; }
// nibble k of a word as the two's-complement 4-bit code it is
__device__ __forceinline__ int nibble(uint32_t w, int k) { return (int)(w << (28 - 4 * k)) >> 28; }
__device__ __forceinline__ float half_bits(uint32_t h) { return __half2float(__ushort_as_half((unsigned short)h)); }

// the four values of the codes at elements e .. e+3 of emb (e numbers the draws of the rounding)
template <int QT>
__device__ __forceinline__ float4 decode(const typename Raw<QT>::T &r, const QSrc &s, float sc, int zero, int64_t e) {
  if constexpr (QT == Q_INT8) {
    return make_float4(deq((int)(int8_t)(r & 0xffu), zero, sc), deq((int)(int8_t)((r >> 8) & 0xffu), zero, sc),
                       deq((int)(int8_t)((r >> 16) & 0xffu), zero, sc), deq((int)(int8_t)(r >> 24), zero, sc));
  } else if constexpr (QT == Q_INT16) {
    return make_float4(deq((int)(int16_t)(r.x & 0xffffu), zero, sc), deq((int)(int16_t)(r.x >> 16), zero, sc),
                       deq((int)(int16_t)(r.y & 0xffffu), zero, sc), deq((int)(int16_t)(r.y >> 16), zero, sc));
  } else if constexpr (QT == Q_INT4) {
    return make_float4(deq(nibble(r, 0), zero, sc), deq(nibble(r, 1), zero, sc), deq(nibble(r, 2), zero, sc),
                       deq(nibble(r, 3), zero, sc));
  } else if constexpr (QT == Q_FP16) {
    return make_float4(half_bits(r.x & 0xffffu), half_bits(r.x >> 16), half_bits(r.y & 0xffffu), half_bits(r.y >> 16));
  } else {
    float qf;
    return make_float4(sr_round(s, r.x, sc, e, qf) * sc, sr_round(s, r.y, sc, e + 1, qf) * sc,
                       sr_round(s, r.z, sc, e + 2, qf) * sc, sr_round(s, r.w, sc, e + 3, qf) * sc);
  }
}

// one element, for the scalar forms
template <int QT>
__device__ __forceinline__ float decode_el(const QSrc &s, int64_t o, float sc, int zero, int64_t e) {
  if constexpr (QT == Q_INT8) return deq((int)reinterpret_cast<const int8_t *>(s.W)[o], zero, sc);
  else if constexpr (QT == Q_INT16) return deq((int)reinterpret_cast<const int16_t *>(s.W)[o], zero, sc);
  else if constexpr (QT == Q_FP16) return __half2float(reinterpret_cast<const __half *>(s.W)[o]);
  else if constexpr (QT == Q_INT4) return deq(nibble(reinterpret_cast<const uint8_t *>(s.W)[o >> 1], (int)(o & 1)), zero, sc);
  else {
    float qf;
    return sr_round(s, reinterpret_cast<const float *>(s.W)[o], sc, e, qf) * sc;
  }
}

// ---------------------------------------------------------------- forward ----
// NIT > 0 (F <= 64, the launcher checks): the ids by one coalesced load + shuffles, the raw words of the NIT steps in
// flight together, emb stored non-temporally, rows_out (nullable) one coalesced store.  NIT = 0: one step at a time,
// any F.  An out-of-range row is a zero row (selected AFTER the dequantisation: a zero code is not a zero value).
template <int LPR, int NIT, int QT>
__global__ __launch_bounds__(kBlock) void k_gather_fm_q_fwd(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets, QSrc s, const float *__restrict__ w1,
    int64_t ldw1, const float *__restrict__ bias, float *__restrict__ emb, float *__restrict__ yfm,
    int64_t *__restrict__ rows_out, int64_t B, int F, int64_t N, int *err) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  using RawT = typename Raw<QT>::T;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const float bv = bias ? bias[0] : 0.f;
  const float sc = src_scale<QT>(s);
  const int zero = src_zero<QT>(s);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  int bad = 0;
  int64_t myoff = 0;
  if constexpr (NIT > 0) myoff = (offsets && lane < F) ? offsets[lane] : 0;

  for (int64_t b = wave0; b < B; b += nwaves) {
    float4 S = z;
    float ss = 0.f, lin = 0.f;
    const int64_t base = b * F;
    if constexpr (NIT > 0) {
      bool act[NIT], ok[NIT];
      RawT raw[NIT];
      float l[NIT];
      const int64_t mine = lane < F ? idx[base + lane] + myoff : 0;
      if (rows_out && lane < F) rows_out[base + lane] = mine;
#pragma unroll
      for (int k = 0; k < NIT; ++k) {
        const int f = r + k * RS;
        act[k] = f < F;
        const int64_t row = __shfl(mine, f & 63);
        ok[k] = act[k] && (uint64_t)row < (uint64_t)N;
        bad |= (act[k] && !ok[k]);
        raw[k] = ok[k] ? load_raw<QT>(s.W, row * D + q * 4) : RawT{};
        l[k] = (ok[k] && q == 0) ? w1[row * ldw1] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < NIT; ++k) {
        const int f = r + k * RS;
        const int64_t e = (base + f) * D + q * 4;
        const float4 v = ok[k] ? decode<QT>(raw[k], s, sc, zero, e) : z;
        if (act[k]) st4_nt(emb + e, v);
        S.x += v.x; S.y += v.y; S.z += v.z; S.w += v.w;
        ss += dot4(v, v);
        lin += l[k];
      }
    } else {
      for (int f = r; f < F; f += RS) {
        const int64_t row = idx[base + f] + (offsets ? offsets[f] : 0);
        const bool ok = (uint64_t)row < (uint64_t)N;
        bad |= !ok;
        const int64_t e = (base + f) * D + q * 4;
        float4 v = z;
        if (ok) {
          v = decode<QT>(load_raw<QT>(s.W, row * D + q * 4), s, sc, zero, e);
          if (q == 0) lin += w1[row * ldw1];
        }
        st4(emb + e, v);
        if (rows_out && q == 0) rows_out[base + f] = row;
        S.x += v.x; S.y += v.y; S.z += v.z; S.w += v.w;
        ss += dot4(v, v);
      }
    }
    S = slot_sum<LPR>(S);
    float t = (r == 0 ? dot4(S, S) : 0.f) - ss;
    t = wave_sum(0.5f * t + lin);
    if (lane == 0) yfm[b] = t + bv;
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// any D (scalar accesses): wave per sample, lanes stride over d
template <int QT>
__global__ __launch_bounds__(kBlock) void k_gather_fm_q_fwd_anyD(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets, QSrc s, const float *__restrict__ w1,
    int64_t ldw1, const float *__restrict__ bias, float *__restrict__ emb, float *__restrict__ yfm,
    int64_t *__restrict__ rows_out, int64_t B, int F, int D, int64_t N, int *err) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const float bv = bias ? bias[0] : 0.f;
  const float sc = src_scale<QT>(s);
  const int zero = src_zero<QT>(s);
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
        if (d < D) {
          const int64_t e = (base + f) * D + d;
          const float v = ok ? decode_el<QT>(s, row * D + d, sc, zero, e) : 0.f;
          emb[e] = v;
          S += v;
          ss += v * v;
        }
      }
      t += 0.5f * (S * S - ss);
    }
    t = wave_sum(t);
    if (lane == 0) yfm[b] = t + bv;
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// ------------------------------------------------ backward, row form (QAT) ----
// For lookup i = b F + f, from the SAVED emb (dE = g_emb + g_y (S_b - e), S_b = sum_f e[b, f, :]):
//   gvals[i, :] = dE        straight through the rounding, clamped elements included (qat_emb.py:49-84)
//   g1vals[i]   = g_y[b];   the bias gradient: bias_grad_block, ONE extra workgroup of the launch
//   dscale     += dE m,     m = q_max where qf >= q_max, q_min where qf <= q_min, else res - qf, with qf = W[row] / scale
//                           gathered again and res = rintf(e / scale), the code the forward rounded to: e = res * scale
//                           and the quotient are rounded once each, so the quotient lies within 2^-22 |res| of the integer
//                           res: below 1/2 for |res| <= 2^20, i.e. n_bits <= kScaleGradMaxBits = 21 (the launcher refuses a
//                           scale gradient past it; QAT_EmbInt takes 8 or 16) — the draw is not needed again.  A flagged
//                           lookup (a zero row) adds nothing.
// W == NULL (a fixed scale): the table is not read and dscale is not written.
// The join: grid_join (common.hpp) — every thread's sum, then the workgroup's, then the grid's in workgroup order by the
// last workgroup to arrive; the bias workgroup takes part with a zero, so that the ticket counts the whole grid.
struct QatBwd {
  const int64_t *rows;
  const float *W, *scale;
  float qmin, qmax;
  int64_t N;
  float *dscale, *part;
  unsigned *ticket;
};

constexpr int kScaleGradMaxBits = 21;      // rintf(emb / scale) recovers the rounded code up to here (above)
constexpr int kBwdSteps = 4;     // row steps per chunk of the float4 backward: their loads are in flight together

__device__ __forceinline__ float scale_term(float dE, float w, float e, float s, float qmin, float qmax) {
  const float qf = w / s;
  const float res = rintf(e / s);
  const float m = qf >= qmax ? qmax : (qf <= qmin ? qmin : res - qf);
  return dE * m;
}

template <int LPR>
__global__ __launch_bounds__(kBlock) void k_gather_fm_qat_bwd_rows(
    const float *__restrict__ emb, const float *__restrict__ g_y, const float *__restrict__ g_emb,
    float *__restrict__ gvals, float *__restrict__ g1vals, int64_t B, int F, float *__restrict__ gbias, QatBwd a) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  int blk, nblk;
  float acc[1] = {0.f};
  if (!bias_grad_block(g_y, B, gbias, blk, nblk)) {
    const int lane = threadIdx.x & 63;
    const int q = lane % LPR, r = lane / LPR;
    const int64_t wave0 = (int64_t)blk * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float s = a.W ? a.scale[0] : 1.f;
    const bool once = F <= kBwdSteps * RS;      // one chunk covers the sample: e[] stays in registers between the two walks
    for (int64_t b = wave0; b < B; b += nwaves) {
      const int64_t base = b * F;
      const float gy = g_y[b];
      float4 S = z;
      float4 e[kBwdSteps], ge[kBwdSteps], w[kBwdSteps];
      bool ok[kBwdSteps];
      for (int f0 = r; f0 < F + r; f0 += kBwdSteps * RS) {
#pragma unroll
        for (int k = 0; k < kBwdSteps; ++k) {
          const int f = f0 + k * RS;
          e[k] = f < F ? ld4(emb + (base + f) * D + q * 4) : z;
        }
#pragma unroll
        for (int k = 0; k < kBwdSteps; ++k) acc4(S, e[k]);
      }
      S = slot_sum<LPR>(S);
      // a chunk of kBwdSteps row steps: every load of the chunk — emb, g_emb, the ids, then the W rows the ids name — is
      // issued before the first use
      for (int f0 = r; f0 < F + r; f0 += kBwdSteps * RS) {
#pragma unroll
        for (int k = 0; k < kBwdSteps; ++k) {
          const int f = f0 + k * RS;
          const bool act = f < F;
          const int64_t i = base + f, eo = i * D + q * 4;
          if (!once) e[k] = act ? ld4(emb + eo) : z;
          ge[k] = (act && g_emb) ? ld4(g_emb + eo) : z;
          const int64_t row = (act && a.W) ? a.rows[i] : -1;
          ok[k] = (uint64_t)row < (uint64_t)a.N;
          w[k] = ok[k] ? ld4(a.W + row * D + q * 4) : z;
        }
#pragma unroll
        for (int k = 0; k < kBwdSteps; ++k) {
          const int f = f0 + k * RS;
          if (f < F) {
            const int64_t i = base + f;
            const float4 dE = fm_grad_row(ge[k], gy, S, e[k]);
            st4(gvals + i * D + q * 4, dE);
            if (q == 0) g1vals[i] = gy;
            if (ok[k])
              acc[0] += (scale_term(dE.x, w[k].x, e[k].x, s, a.qmin, a.qmax) + scale_term(dE.y, w[k].y, e[k].y, s, a.qmin, a.qmax)) +
                        (scale_term(dE.z, w[k].z, e[k].z, s, a.qmin, a.qmax) + scale_term(dE.w, w[k].w, e[k].w, s, a.qmin, a.qmax));
          }
        }
      }
    }
  }
  if (a.W) grid_join(acc, a.part, a.ticket, [&](const float (&total)[1]) { a.dscale[0] = total[0]; });
}

// any D <= kQatBwdMaxD (scalar accesses): wave per sample, lanes stride over d
__global__ __launch_bounds__(kBlock) void k_gather_fm_qat_bwd_rows_anyD(
    const float *__restrict__ emb, const float *__restrict__ g_y, const float *__restrict__ g_emb,
    float *__restrict__ gvals, float *__restrict__ g1vals, int64_t B, int F, int D, float *__restrict__ gbias, QatBwd a) {
  int blk, nblk;
  float acc[1] = {0.f};
  if (!bias_grad_block(g_y, B, gbias, blk, nblk)) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blk * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
    const float s = a.W ? a.scale[0] : 1.f;
    for (int64_t b = wave0; b < B; b += nwaves) {
      const int64_t base = b * F;
      const float gy = g_y[b];
      for (int f = lane; f < F; f += kWave) g1vals[base + f] = gy;
      for (int d = lane; d < D; d += kWave) {
        float S = 0.f;
        for (int f = 0; f < F; ++f) S += emb[(base + f) * D + d];
        for (int f = 0; f < F; ++f) {
          const int64_t eo = (base + f) * D + d;
          const float e = emb[eo];
          const float dE = (g_emb ? g_emb[eo] : 0.f) + gy * (S - e);
          gvals[eo] = dE;
          if (a.W) {
            const int64_t row = a.rows[base + f];
            if ((uint64_t)row < (uint64_t)a.N) acc[0] += scale_term(dE, a.W[row * D + d], e, s, a.qmin, a.qmax);
          }
        }
      }
    }
  }
  if (a.W) grid_join(acc, a.part, a.ticket, [&](const float (&total)[1]) { a.dscale[0] = total[0]; });
}

// the workgroups of a backward launch: those that share the samples, then the one that only sums the bias gradient
inline int bwd_grid(int64_t B, bool with_bias) { return grid_for_waves(B) + (with_bias ? 1 : 0); }

// the lane's four codes are one aligned word: D = 4 * 2^k and the table's base on a four-code boundary
inline bool codes_word_ok(const void *W, int qtype) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(W);
  return qtype == Q_INT8 ? (p & 3) == 0 : qtype == Q_INT4 ? (p & 1) == 0 : qtype == Q_QAT ? (p & 15) == 0 : (p & 7) == 0;
}

template <int QT>
int launch_q_fwd(const char *name, const int64_t *idx, const int64_t *offsets, const QSrc &s, const float *w1,
                 int64_t ldw1, const float *bias, float *emb, float *yfm, int64_t *rows_out, int64_t B, int F, int D,
                 int64_t N, int *err, void *stream) {
  const int grid = grid_for_waves(B);
  if (vec_ok(D) && codes_word_ok(s.W, QT) && aligned16(emb)) {
    const int lpr = D / 4, nit = F <= kWave ? nit_for(F, lpr) : 0;      // (unrolled only in shuffle form)
#define CALL(LPR, NIT)                                                                                                 \
  MI_LAUNCH(name, (k_gather_fm_q_fwd<LPR, NIT, QT>), grid, kBlock, stream, idx, offsets, s, w1, ldw1, bias, emb, yfm, \
            rows_out, B, F, N, err)
    MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
  } else {
    MI_LAUNCH(name, k_gather_fm_q_fwd_anyD<QT>, grid, kBlock, stream, idx, offsets, s, w1, ldw1, bias, emb, yfm, rows_out,
              B, F, D, N, err);
  }
  return launch_status();
}

inline bool qat_range(int32_t n_bits, float &qmin, float &qmax) {
  if (n_bits < 2 || n_bits > 24) return false;
  qmin = -(float)(1 << (n_bits - 1));
  qmax = (float)((1 << (n_bits - 1)) - 1);
  return true;
}

}  // namespace

extern "C" {

int mi_gather_fm_quant_fwd(const int64_t *idx, const int64_t *offsets, const void *Wq, int32_t qtype, const float *scale,
                           const void *zero, const float *w1, int64_t ldw1, const float *bias, float *emb_out,
                           float *yfm_out, int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err, void *stream) {
  if (B < 0 || F < 0 || D <= 0 || N < 0 || ldw1 < 1 || qtype < Q_FP16 || qtype > Q_INT4 || qtype == Q_QAT) return MI_ERR_INVALID_ARG;
  if (qtype == Q_INT4 && (D & 1)) return MI_ERR_INVALID_ARG;      // two codes per byte: a row is D / 2 bytes
  if (B == 0) return MI_OK;
  if (!idx || !Wq || !w1 || !emb_out || !yfm_out || (qtype != Q_FP16 && (!scale || !zero))) return MI_ERR_INVALID_ARG;
  const QSrc s{Wq, scale, zero, 0.f, 0.f, nullptr, nullptr, 0};
  const char *name = "gather_fm_quant_fwd";
  if (qtype == Q_FP16)
    return launch_q_fwd<Q_FP16>(name, idx, offsets, s, w1, ldw1, bias, emb_out, yfm_out, nullptr, B, F, D, N, err, stream);
  if (qtype == Q_INT4)
    return launch_q_fwd<Q_INT4>(name, idx, offsets, s, w1, ldw1, bias, emb_out, yfm_out, nullptr, B, F, D, N, err, stream);
  if (qtype == Q_INT8)
    return launch_q_fwd<Q_INT8>(name, idx, offsets, s, w1, ldw1, bias, emb_out, yfm_out, nullptr, B, F, D, N, err, stream);
  return launch_q_fwd<Q_INT16>(name, idx, offsets, s, w1, ldw1, bias, emb_out, yfm_out, nullptr, B, F, D, N, err, stream);
}

int mi_gather_fm_qat_fwd(const int64_t *idx, const int64_t *offsets, const float *W, const float *scale, int32_t n_bits,
                         const float *prob, const int64_t *seed, int64_t salt, const float *w1, int64_t ldw1,
                         const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out, int64_t B, int32_t F,
                         int32_t D, int64_t N, int32_t *err, void *stream) {
  QSrc s{W, scale, nullptr, 0.f, 0.f, prob, seed, salt};
  if (B < 0 || F < 0 || D <= 0 || N < 0 || ldw1 < 1 || !qat_range(n_bits, s.qmin, s.qmax)) return MI_ERR_INVALID_ARG;
  if (B == 0) return MI_OK;      // (an empty draw has no address: nothing below is asked of an empty batch)
  if (!W || !scale || (!prob && !seed)) return MI_ERR_INVALID_ARG;
  if (!idx || !w1 || !emb_out || !yfm_out) return MI_ERR_INVALID_ARG;
  return launch_q_fwd<Q_QAT>("gather_fm_qat_fwd", idx, offsets, s, w1, ldw1, bias, emb_out, yfm_out, rows_out, B, F, D, N,
                             err, stream);
}

int64_t mi_gather_fm_qat_bwd_workspace_elems(int64_t B) {
  if (B <= 0) return 0;
  return (int64_t)bwd_grid(B, true) + 1;      // one partial sum per workgroup, then the ticket
}

int mi_gather_fm_qat_bwd_rows(const int64_t *rows, const float *W, const float *scale, int32_t n_bits, const float *emb,
                              const float *g_y, const float *g_emb, float *gvals, float *g1vals, float *gbias,
                              float *dscale, float *workspace, int32_t armed, int64_t B, int32_t F, int32_t D, int64_t N,
                              void *stream) {
  QatBwd a{rows, W, scale, 0.f, 0.f, N, dscale, nullptr, nullptr};
  if (B < 0 || F < 0 || D <= 0 || N < 0 || !qat_range(n_bits, a.qmin, a.qmax)) return MI_ERR_INVALID_ARG;
  if ((W != nullptr) != (dscale != nullptr)) return MI_ERR_INVALID_ARG;      // the table is read for the scale gradient only
  if (D > kQatBwdMaxD || (W && n_bits > kScaleGradMaxBits)) return MI_ERR_UNSUPPORTED;
  if (B == 0 || F == 0) {      // no lookup: the scale gradient still owes its zero
    if (dscale && hipMemsetAsync(dscale, 0, sizeof(float), (hipStream_t)stream) != hipSuccess) return MI_ERR_LAUNCH;
    if (B == 0) return MI_OK;
  }
  if (!emb || !g_y || !gvals || !g1vals || (W && (!rows || !scale || !workspace))) return MI_ERR_INVALID_ARG;
  if (W) {
    a.part = workspace;
    a.ticket = reinterpret_cast<unsigned *>(workspace + bwd_grid(B, true));
    if (!armed && hipMemsetAsync(a.ticket, 0, sizeof(unsigned), (hipStream_t)stream) != hipSuccess) return MI_ERR_LAUNCH;
  }
  const int grid = bwd_grid(B, gbias != nullptr);
  if (vec_ok(D) && all_aligned16(emb, g_emb, gvals, W)) {
#define CALL(LPR)                                                                                                   \
  MI_LAUNCH("gather_fm_qat_bwd_rows", (k_gather_fm_qat_bwd_rows<LPR>), grid, kBlock, stream, emb, g_y, g_emb, gvals, \
            g1vals, B, F, gbias, a)
    MI_DISPATCH_LPR(D / 4, CALL)
#undef CALL
  } else {
    MI_LAUNCH("gather_fm_qat_bwd_rows", k_gather_fm_qat_bwd_rows_anyD, grid, kBlock, stream, emb, g_y, g_emb, gvals, g1vals,
              B, F, D, gbias, a);
  }
  return launch_status();
}

}  // extern "C"
