// gather_fm_dual.hip — DeepFM on the two-table compositional embeddings (QR hashing, CERP, CERP retrain): the lookup
//   row = idx[b, f] + offsets[f],   emb[b, f, :] = T1'[row % mod1] (op) T2'[row / div2]
// fused with the FM second-order term and the first-order bag (src/models/deepfm.py:88-98 over
// src/models/embeddings/qr_embedding.py:84-109 / cerp_embedding.py:160-175 and :329-367), its row-form backward, the
// once-per-table-row "finish" of the dense gradients, and CERP's whole-table prune loss
// (cerp_embedding.py get_prune_loss) forward and backward.
//
// Forward mapping: gather_fm.hip's — one wave per sample, LPR = De / 4 lanes per row, RS = 64 / LPR rows per
// wave-instruction, the F ids by one coalesced load and shuffles when F <= 64 — with TWO row gathers per lookup.  Both
// rows, and their threshold logits or mask bytes, need only the row id: all of a step's loads (up to 4 NIT float4 per
// lane for the soft form) are issued before the first use.  HBM / L2 latency-bound copy work: no LDS.  The element
// transforms are dual_xform.hpp's, so emb has the bits of mi_dual_gather_fwd.
// What the two files share lives in gather_fm_walk.hpp: the float4 helpers, the bias-gradient workgroup, fm_grad_row
// and the (LPR, NIT) dispatch.  The forward walks below stay bodies of their own: run by a shared float4 walk, y_fm
// moved in the last bit (see the header).
//
// Backward: no float atomics anywhere in this file.  The row kernel writes one value row per lookup and table
// (c1, c2) and the table-row keys (r1, r2); the caller sums the rows per key in a fixed order (mi_coalesce_rows_sorted)
// or hands them out as COO values.  The transform's derivative is a function of the table element, not of the lookup:
// k_dual_finish applies it once per table element after the sum.
#include "common.hpp"
#include "dual_xform.hpp"
#include "gather_fm_walk.hpp"

namespace {
using namespace mi;

struct DualFm {
  const float *T1, *T2;      // [n1, De], [n2, De]
  const float *S1, *S2;      // XF_SOFT: threshold logits, shaped like the tables
  const uint8_t *M1, *M2;    // XF_MASK: one byte per element, shaped like the tables
  int64_t n1, n2, mod1, div2;
  int op;                    // OP_MULT or OP_ADD
};

// r1 = row % mod1, r2 = row / div2 for a row in [0, N); false for a row the tables cannot serve.  Rows and divisors below
// 2^32 (every table of the reference's configs) divide in 32 bits: the 64-bit division by a run-time value is a
// ~150-instruction routine on this ISA.
__device__ __forceinline__ bool split_row(int64_t row, int64_t N, const DualFm &t, int64_t &r1, int64_t &r2) {
  r1 = r2 = 0;
  if ((uint64_t)row >= (uint64_t)N) return false;
  const uint64_t u = (uint64_t)row;
  if (((u | (uint64_t)t.mod1 | (uint64_t)t.div2) >> 32) == 0) {
    r1 = (int64_t)((uint32_t)u % (uint32_t)t.mod1);
    r2 = (int64_t)((uint32_t)u / (uint32_t)t.div2);
  } else {
    r1 = row % t.mod1;
    r2 = row / t.div2;
  }
  if (r1 < t.n1 && r2 < t.n2) return true;
  r1 = r2 = 0;
  return false;
}

__device__ __forceinline__ float4 combine(int op, float4 a, float4 b) { return op == OP_MULT ? mul4(a, b) : add4(a, b); }

// ---------------------------------------------------------------- forward ----
// rows_bwd (nullable, [B, F]): the row again where the lookup was served and -1 where it was flagged — the ids a backward
// that checks table bounds only (mi_dual_gather_bwd_*) has to see, so that it skips exactly what the forward zeroed.
// NIT > 0 (F <= 64, the launcher checks): the ids by one coalesced load + shuffles, all loads of the NIT steps in flight,
// emb stored non-temporally.  NIT = 0: one step at a time, any F.
template <int LPR, int NIT, int XF>
__global__ __launch_bounds__(kBlock) void k_gather_fm_dual_fwd(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets, DualFm t, const float *__restrict__ w1,
    int64_t ldw1, const float *__restrict__ bias, float *__restrict__ emb, float *__restrict__ yfm,
    int64_t *__restrict__ rows_out, int64_t *__restrict__ rows_bwd, int64_t B, int F, int64_t N, int *err) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const float bv = bias ? bias[0] : 0.f;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  int bad = 0;
  int64_t myoff = 0;
  if constexpr (NIT > 0) myoff = (offsets && lane < F) ? offsets[lane] : 0;

  for (int64_t b = wave0; b < B; b += nwaves) {
    float4 S = z;
    float ss = 0.f, lin = 0.f;
    const int64_t base = b * F;
    if constexpr (NIT > 0) {
      int64_t r1[NIT], r2[NIT];
      bool act[NIT], ok[NIT];
      float4 a[NIT], c[NIT];
      float l[NIT];
      float4 ta[NIT], tc[NIT];      // (XF_SOFT only)
      uint32_t ma[NIT], mc[NIT];    // (XF_MASK only)
      const int64_t mine = lane < F ? idx[base + lane] + myoff : 0;
      if (rows_out && lane < F) rows_out[base + lane] = mine;
      if (rows_bwd && lane < F) {
        int64_t a1, a2;
        rows_bwd[base + lane] = split_row(mine, N, t, a1, a2) ? mine : -1;
      }
#pragma unroll
      for (int k = 0; k < NIT; ++k) {
        const int f = r + k * RS;
        act[k] = f < F;
        const int64_t row = __shfl(mine, f & 63);
        ok[k] = split_row(row, N, t, r1[k], r2[k]) && act[k];
        bad |= (act[k] && !ok[k]);
        const int64_t o1 = r1[k] * D + q * 4, o2 = r2[k] * D + q * 4;
        a[k] = ok[k] ? ld4(t.T1 + o1) : z;
        c[k] = ok[k] ? ld4(t.T2 + o2) : z;
        l[k] = (ok[k] && q == 0) ? w1[row * ldw1] : 0.f;
        if constexpr (XF == XF_SOFT) {
          ta[k] = ok[k] ? ld4(t.S1 + o1) : z;
          tc[k] = ok[k] ? ld4(t.S2 + o2) : z;
        }
        if constexpr (XF == XF_MASK) {
          ma[k] = ok[k] ? mask4(t.M1, o1) : 0u;
          mc[k] = ok[k] ? mask4(t.M2, o2) : 0u;
        }
      }
#pragma unroll
      for (int k = 0; k < NIT; ++k) {
        const int f = r + k * RS;
        if constexpr (XF == XF_SOFT) {
          if (ok[k]) {      // (a flagged lookup is +0 whatever soft_(0, 0) would give)
            a[k] = soft4(a[k], ta[k]);
            c[k] = soft4(c[k], tc[k]);
          }
        }
        if constexpr (XF == XF_MASK) {
          a[k] = keep_bytes(a[k], ma[k]);
          c[k] = keep_bytes(c[k], mc[k]);
        }
        const float4 v = ok[k] ? combine(t.op, a[k], c[k]) : z;
        if (act[k]) st4_nt(emb + (base + f) * D + q * 4, v);
        S.x += v.x; S.y += v.y; S.z += v.z; S.w += v.w;
        ss += dot4(v, v);
        lin += l[k];
      }
    } else {
      for (int f = r; f < F; f += RS) {
        const int64_t row = idx[base + f] + (offsets ? offsets[f] : 0);
        int64_t r1, r2;
        const bool ok = split_row(row, N, t, r1, r2);
        bad |= !ok;
        float4 v = z;
        if (ok) {
          v = combine(t.op, load_row4<XF>(t.T1, t.S1, t.M1, r1 * D + q * 4), load_row4<XF>(t.T2, t.S2, t.M2, r2 * D + q * 4));
          if (q == 0) lin += w1[row * ldw1];
        }
        st4(emb + (base + f) * D + q * 4, v);
        if (rows_out && q == 0) rows_out[base + f] = row;
        if (rows_bwd && q == 0) rows_bwd[base + f] = ok ? row : -1;
        S.x += v.x; S.y += v.y; S.z += v.z; S.w += v.w;
        ss += dot4(v, v);
      }
    }
    S = slot_sum<LPR>(S);
    float tt = (r == 0 ? dot4(S, S) : 0.f) - ss;
    tt = wave_sum(0.5f * tt + lin);
    if (lane == 0) yfm[b] = tt + bv;
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

__device__ __forceinline__ float load_el(int xf, const float *T, const float *S, const uint8_t *M, int64_t o) {
  const float w = T[o];
  if (xf == XF_SOFT) return soft_(w, S[o]);
  if (xf == XF_MASK) return M[o] ? w : 0.f;
  return w;
}

// any De (scalar accesses): wave per sample, lanes stride over d
__global__ __launch_bounds__(kBlock) void k_gather_fm_dual_fwd_anyD(
    const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets, DualFm t, int xf, const float *__restrict__ w1,
    int64_t ldw1, const float *__restrict__ bias, float *__restrict__ emb, float *__restrict__ yfm,
    int64_t *__restrict__ rows_out, int64_t *__restrict__ rows_bwd, int64_t B, int F, int D, int64_t N, int *err) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const float bv = bias ? bias[0] : 0.f;
  int bad = 0;
  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    float tt = 0.f;
    for (int d0 = 0; d0 < D; d0 += kWave) {
      const int d = d0 + lane;
      float S = 0.f, ss = 0.f;
      for (int f = 0; f < F; ++f) {
        const int64_t row = idx[base + f] + (offsets ? offsets[f] : 0);
        int64_t r1, r2;
        const bool ok = split_row(row, N, t, r1, r2);
        bad |= !ok;
        if (d0 == 0 && lane == 0) {
          if (ok) tt += w1[row * ldw1];
          if (rows_out) rows_out[base + f] = row;
          if (rows_bwd) rows_bwd[base + f] = ok ? row : -1;
        }
        if (d < D) {
          float v = 0.f;
          if (ok) {
            const float a = load_el(xf, t.T1, t.S1, t.M1, r1 * D + d), c = load_el(xf, t.T2, t.S2, t.M2, r2 * D + d);
            v = t.op == OP_MULT ? a * c : a + c;
          }
          emb[(base + f) * D + d] = v;
          S += v;
          ss += v * v;
        }
      }
      tt += 0.5f * (S * S - ss);
    }
    tt = wave_sum(tt);
    if (lane == 0) yfm[b] = tt + bv;
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// ----------------------------------------------------- backward, row form ----
// (the bias gradient: bias_grad_block, gather_fm_walk.hpp — ONE extra workgroup of the launch)

// What the row kernels write for lookup i = b F + f (dE = g_emb + g_y (S_b - e), S_b = sum_f e[b, f, :]):
//   keys1[i] = r1, keys2[i] = r2 (0 for a lookup the forward flagged; its value rows are zeros)
//   op add : c1 = dE [M1[r1, :]],  c2 = dE [M2[r2, :]]   (the masks only when mask_vals: the COO form of the retrain table;
//            without them c1 == c2 and c2 may be NULL: one value array serves both tables)
//   op mult: c1 = dE * T2[r2, :],  c2 = dE * T1[r1, :]   (the partner rows gathered again)
//   g1vals[i] = g_y[b]
// field_off given (the caller sums in the order of mi_sort_field_rows): a row inside [0, N) but outside its own field is
// treated like a flagged one (zero value rows) — that sort moves such an id behind its field and the sums taken in its
// order drop it, so every table drops it —, and EVERY flagged lookup of field f gets keys2 = the largest table-2 row of
// field f instead of 0: behind the field's served ids and in front of the next field's, so keys2 gathered through the
// sort's permutation is monotone as it stands (a key out of order would cut a table row's segment in two, and the row
// would be written twice).
struct DualRowsOut {
  float *c1, *c2;
  int64_t *keys1, *keys2;
  float *g1vals;
  int mask_vals;
  const int64_t *field_off;      // (nullable, [F]) the fields' first rows: a row outside its own field counts as flagged
};

// (r1, r2) of the lookup of `row` in field f and whether it is served; see field_off above
__device__ __forceinline__ bool lookup_keys(const DualRowsOut &o, const DualFm &t, int f, int F, int64_t N, int64_t row,
                                            int64_t &r1, int64_t &r2) {
  const bool ok = split_row(row, N, t, r1, r2);
  if (!o.field_off) return ok;
  const int64_t hi = f + 1 < F ? o.field_off[f + 1] : N;      // field f is [field_off[f], hi)
  if (ok && row >= o.field_off[f] && row < hi) return true;
  const int64_t k = hi > 0 ? (hi - 1) / t.div2 : 0;
  r1 = 0;
  r2 = k < t.n2 ? k : t.n2 - 1;
  return false;
}

template <int LPR>
__global__ __launch_bounds__(kBlock) void k_gather_fm_dual_bwd_rows(
    const int64_t *__restrict__ rows, const float *__restrict__ emb, const float *__restrict__ g_y,
    const float *__restrict__ g_emb, DualFm t, DualRowsOut o, int64_t B, int F, int64_t N, float *__restrict__ gbias) {
  constexpr int RS = kWave / LPR;
  constexpr int D = LPR * 4;
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPR, r = lane / LPR;
  const int64_t wave0 = (int64_t)blk * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    const float gy = g_y[b];
    float4 S = z;
    for (int f = r; f < F; f += RS) acc4(S, ld4(emb + (base + f) * D + q * 4));
    S = slot_sum<LPR>(S);
    for (int f = r; f < F; f += RS) {
      const int64_t i = base + f, eo = i * D + q * 4;
      int64_t r1, r2;
      const bool ok = lookup_keys(o, t, f, F, N, rows[i], r1, r2);
      const float4 e = ld4(emb + eo), ge = g_emb ? ld4(g_emb + eo) : z;
      const float4 dE = fm_grad_row(ge, gy, S, e);
      float4 c1 = z, c2 = z;
      if (ok) {
        const int64_t o1 = r1 * D + q * 4, o2 = r2 * D + q * 4;
        if (t.op == OP_MULT) {
          c1 = mul4(dE, ld4(t.T2 + o2));
          c2 = mul4(dE, ld4(t.T1 + o1));
        } else if (o.mask_vals) {
          c1 = keep_bytes(dE, mask4(t.M1, o1));
          c2 = keep_bytes(dE, mask4(t.M2, o2));
        } else {
          c1 = c2 = dE;
        }
      }
      st4(o.c1 + eo, c1);
      if (o.c2) st4(o.c2 + eo, c2);
      if (q == 0) {
        o.keys1[i] = r1;
        o.keys2[i] = r2;
        o.g1vals[i] = gy;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_gather_fm_dual_bwd_rows_anyD(
    const int64_t *__restrict__ rows, const float *__restrict__ emb, const float *__restrict__ g_y,
    const float *__restrict__ g_emb, DualFm t, DualRowsOut o, int64_t B, int F, int D, int64_t N, float *__restrict__ gbias) {
  int blk, nblk;
  if (bias_grad_block(g_y, B, gbias, blk, nblk)) return;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blk * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)nblk * kWavesPerBlock;
  for (int64_t b = wave0; b < B; b += nwaves) {
    const int64_t base = b * F;
    const float gy = g_y[b];
    for (int f = lane; f < F; f += kWave) {
      int64_t r1, r2;
      lookup_keys(o, t, f, F, N, rows[base + f], r1, r2);
      o.keys1[base + f] = r1;
      o.keys2[base + f] = r2;
      o.g1vals[base + f] = gy;
    }
    for (int d = lane; d < D; d += kWave) {
      float S = 0.f;
      for (int f = 0; f < F; ++f) S += emb[(base + f) * D + d];
      for (int f = 0; f < F; ++f) {
        const int64_t eo = (base + f) * D + d;
        int64_t r1, r2;
        const bool ok = lookup_keys(o, t, f, F, N, rows[base + f], r1, r2);
        const float dE = (g_emb ? g_emb[eo] : 0.f) + gy * (S - emb[eo]);
        float c1 = 0.f, c2 = 0.f;
        if (ok) {
          if (t.op == OP_MULT) {
            c1 = dE * t.T2[r2 * D + d];
            c2 = dE * t.T1[r1 * D + d];
          } else if (o.mask_vals) {
            c1 = t.M1[r1 * D + d] ? dE : 0.f;
            c2 = t.M2[r2 * D + d] ? dE : 0.f;
          } else {
            c1 = c2 = dE;
          }
        }
        o.c1[eo] = c1;
        if (o.c2) o.c2[eo] = c2;
      }
    }
  }
}

// ------------------------------------------ the finish of the dense sums ----
// A (in place) -> gT = kept A and, for the soft form, gS = -sign(T) sig(S) (1 - sig(S)) kept A, with
// kept = M != 0 (mask) or |T| - sig(S) > 0 (soft): from the table and its threshold, never from the looked-up values — a
// kept element that holds exactly 0 keeps its gradient, a pruned one gets exactly 0.  One launch covers both tables:
// elements [0, e1) are table 1's, [e1, e1 + e2) table 2's.
struct FinishArgs {
  float *A[2];
  const float *T[2], *S[2];
  const uint8_t *M[2];
  float *gS[2];
  int64_t e[2];
};

__device__ __forceinline__ void finish_el(int xf, float a, float w, float s, uint8_t m, float &gw, float &gs) {
  if (xf == XF_MASK) {
    gw = m ? a : 0.f;
    gs = 0.f;
  } else {
    const float sg = sigmoidf_(s);
    const float keep = (fabsf(w) - sg > 0.f) ? 1.f : 0.f;
    gw = a * keep;
    gs = -a * signf_(w) * keep * sg * (1.f - sg);
  }
}

template <int XF>
__global__ __launch_bounds__(kBlock) void k_dual_finish(FinishArgs a) {
  const int64_t total = a.e[0] + a.e[1];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int tb = i < a.e[0] ? 0 : 1;
    const int64_t j = tb ? i - a.e[0] : i;
    float gw, gs;
    finish_el(XF, a.A[tb][j], XF == XF_SOFT ? a.T[tb][j] : 0.f, XF == XF_SOFT ? a.S[tb][j] : 0.f,
              XF == XF_MASK ? a.M[tb][j] : (uint8_t)1, gw, gs);
    a.A[tb][j] = gw;
    if constexpr (XF == XF_SOFT) a.gS[tb][j] = gs;
  }
}

// ------------------------------------------- CERP's whole-table prune loss ----
//   L = -sum tanh(K (soft(P, Sp) + soft(Q, Sq)))^2 over the n = bucket * D elements of the four tables
// Forward: every thread adds its elements (a grid-stride walk, coalesced; four independent tables, one pass), grid_join
// sums the workgroups' partials in a fixed order in the last workgroup: the same bits on every run.
struct PruneTables {
  const float *P, *Sp, *Q, *Sq;
  int64_t n;
  float K;
};

__device__ __forceinline__ float prune_term(float p, float sp, float q, float sq, float K) {
  const float th = tanhf(K * (soft_(p, sp) + soft_(q, sq)));
  return th * th;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_cerp_prune_loss_fwd(PruneTables a, float *part, unsigned *ticket, float *out) {
  float v[1] = {0.f};
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nthr = (int64_t)gridDim.x * kBlock;
  if constexpr (VEC) {
    for (int64_t i = tid * 4; i < a.n; i += nthr * 4) {
      const float4 p = ld4(a.P + i), sp = ld4(a.Sp + i), q = ld4(a.Q + i), sq = ld4(a.Sq + i);
      v[0] += (prune_term(p.x, sp.x, q.x, sq.x, a.K) + prune_term(p.y, sp.y, q.y, sq.y, a.K)) +
              (prune_term(p.z, sp.z, q.z, sq.z, a.K) + prune_term(p.w, sp.w, q.w, sq.w, a.K));
    }
  } else {
    for (int64_t i = tid; i < a.n; i += nthr) v[0] += prune_term(a.P[i], a.Sp[i], a.Q[i], a.Sq[i], a.K);
  }
  grid_join(v, part, ticket, [&](const float (&total)[1]) { out[0] = -total[0]; });
}

// Backward: with x = p' + q', t = tanh(K x), g = -2 K t (1 - t^2) grad_out:
//   gP = kept_p g,  gSp = -sign(P) sig(Sp) (1 - sig(Sp)) kept_p g   (the same from Q, Sq) — every element written once.
__device__ __forceinline__ void prune_grad(float p, float sp, float q, float sq, float K, float go, float &gp, float &gsp,
                                           float &gq, float &gsq) {
  const float th = tanhf(K * (soft_(p, sp) + soft_(q, sq)));
  const float g = -2.f * K * th * (1.f - th * th) * go;
  finish_el(XF_SOFT, g, p, sp, 1, gp, gsp);
  finish_el(XF_SOFT, g, q, sq, 1, gq, gsq);
}

struct PruneGrads {
  float *gP, *gSp, *gQ, *gSq;
};

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_cerp_prune_loss_bwd(PruneTables a, const float *__restrict__ grad_out, PruneGrads g) {
  const float go = grad_out[0];
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nthr = (int64_t)gridDim.x * kBlock;
  if constexpr (VEC) {
    for (int64_t i = tid * 4; i < a.n; i += nthr * 4) {
      const float4 p = ld4(a.P + i), sp = ld4(a.Sp + i), q = ld4(a.Q + i), sq = ld4(a.Sq + i);
      float4 gp, gsp, gq, gsq;
      prune_grad(p.x, sp.x, q.x, sq.x, a.K, go, gp.x, gsp.x, gq.x, gsq.x);
      prune_grad(p.y, sp.y, q.y, sq.y, a.K, go, gp.y, gsp.y, gq.y, gsq.y);
      prune_grad(p.z, sp.z, q.z, sq.z, a.K, go, gp.z, gsp.z, gq.z, gsq.z);
      prune_grad(p.w, sp.w, q.w, sq.w, a.K, go, gp.w, gsp.w, gq.w, gsq.w);
      st4(g.gP + i, gp);
      st4(g.gSp + i, gsp);
      st4(g.gQ + i, gq);
      st4(g.gSq + i, gsq);
    }
  } else {
    for (int64_t i = tid; i < a.n; i += nthr)
      prune_grad(a.P[i], a.Sp[i], a.Q[i], a.Sq[i], a.K, go, g.gP[i], g.gSp[i], g.gQ[i], g.gSq[i]);
  }
}


// the (op, xform) pairs the models produce: (mult, none) and (add, none) QR, (add, soft) CERP, (add, mask) CERP retrain
inline bool served(int op, int xform) {
  return (op == OP_MULT && xform == XF_NONE) || (op == OP_ADD && xform >= XF_NONE && xform <= XF_MASK);
}

inline int fill(DualFm &t, const float *T1, const float *T2, const float *S1, const float *S2, const uint8_t *M1,
                const uint8_t *M2, int64_t n1, int64_t n2, int64_t mod1, int64_t div2, int op, int xform) {
  if (n1 <= 0 || n2 <= 0 || mod1 <= 0 || div2 <= 0) return MI_ERR_INVALID_ARG;
  if (op < OP_MULT || op > OP_CAT || xform < XF_NONE || xform > XF_MASK) return MI_ERR_INVALID_ARG;
  if (!served(op, xform)) return MI_ERR_UNSUPPORTED;
  if (!T1 || !T2 || (xform == XF_SOFT && (!S1 || !S2)) || (xform == XF_MASK && (!M1 || !M2))) return MI_ERR_INVALID_ARG;
  t = DualFm{T1, T2, S1, S2, M1, M2, n1, n2, mod1, div2, op};
  return MI_OK;
}

inline bool tables_float4_ok(const DualFm &t, int xform) {
  return all_aligned16(t.T1, t.T2) && (xform != XF_SOFT || all_aligned16(t.S1, t.S2)) &&
         (xform != XF_MASK || ((((uintptr_t)t.M1 | (uintptr_t)t.M2) & 3) == 0));
}


inline int grid_for_elems(int64_t n) {
  int64_t g = (n + kBlock - 1) / kBlock;
  return (int)(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));
}

// workgroups of the prune loss forward for n elements (four elements per thread and trip when vectorised)
inline int prune_grid(int64_t n) { return grid_for_elems((n + 3) / 4); }

}  // namespace

extern "C" {

int mi_gather_fm_dual_fwd(const int64_t *idx, const int64_t *offsets, const float *T1, const float *T2, const float *S1,
                          const float *S2, const uint8_t *M1, const uint8_t *M2, const float *w1, int64_t ldw1,
                          const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out, int64_t *rows_bwd, int64_t B,
                          int32_t F, int32_t De, int64_t N, int64_t n1, int64_t n2, int64_t mod1, int64_t div2, int32_t op,
                          int32_t xform, int32_t *err, void *stream) {
  if (B < 0 || F < 0 || De <= 0 || N < 0 || ldw1 < 1) return MI_ERR_INVALID_ARG;
  DualFm t;
  const int rc = fill(t, T1, T2, S1, S2, M1, M2, n1, n2, mod1, div2, op, xform);
  if (rc != MI_OK) return rc;
  if (De > MI_GATHER_FM_DUAL_MAX_D) return MI_ERR_UNSUPPORTED;
  if (B == 0) return MI_OK;
  if (!idx || !w1 || !emb_out || !yfm_out) return MI_ERR_INVALID_ARG;
  const int grid = grid_for_waves(B);
  if (vec_ok(De) && tables_float4_ok(t, xform) && aligned16(emb_out)) {
    const int lpr = De / 4, nit = F <= kWave ? nit_for(F, lpr) : 0;      // (unrolled only in shuffle form)
    decltype(&k_gather_fm_dual_fwd<1, 0, XF_NONE>) kernel = nullptr;
#define CALL(LPR, NIT)                                                     \
  kernel = xform == XF_NONE   ? k_gather_fm_dual_fwd<LPR, NIT, XF_NONE>   \
           : xform == XF_SOFT ? k_gather_fm_dual_fwd<LPR, NIT, XF_SOFT>   \
                              : k_gather_fm_dual_fwd<LPR, NIT, XF_MASK>
    MI_DISPATCH_LPR_NIT(lpr, nit, CALL)
#undef CALL
    MI_LAUNCH("gather_fm_dual_fwd", kernel, grid, kBlock, stream, idx, offsets, t, w1, ldw1, bias, emb_out, yfm_out,
              rows_out, rows_bwd, B, F, N, err);
  } else {
    MI_LAUNCH("gather_fm_dual_fwd", k_gather_fm_dual_fwd_anyD, grid, kBlock, stream, idx, offsets, t, xform, w1, ldw1, bias,
              emb_out, yfm_out, rows_out, rows_bwd, B, F, De, N, err);
  }
  return launch_status();
}

int mi_gather_fm_dual_bwd_rows(const int64_t *rows, const int64_t *field_off, const float *emb, const float *g_y, const float *g_emb, const float *T1,
                               const float *T2, const uint8_t *M1, const uint8_t *M2, float *c1, float *c2, int64_t *keys1,
                               int64_t *keys2, float *g1vals, float *gbias, int64_t B, int32_t F, int32_t De, int64_t N,
                               int64_t n1, int64_t n2, int64_t mod1, int64_t div2, int32_t op, void *stream) {
  if (B < 0 || F < 0 || De <= 0 || N < 0) return MI_ERR_INVALID_ARG;
  const int mask_vals = (M1 || M2) ? 1 : 0;
  DualFm t;
  const int rc = fill(t, T1, T2, nullptr, nullptr, M1, M2, n1, n2, mod1, div2, op, mask_vals ? XF_MASK : XF_NONE);
  if (rc != MI_OK) return rc;
  if (De > MI_GATHER_FM_DUAL_MAX_D) return MI_ERR_UNSUPPORTED;
  if (B == 0) return MI_OK;
  if (!rows || !emb || !g_y || !c1 || !keys1 || !keys2 || !g1vals) return MI_ERR_INVALID_ARG;
  if ((op == OP_MULT || mask_vals) && !c2) return MI_ERR_INVALID_ARG;      // the two tables' value rows differ
  const DualRowsOut o{c1, c2, keys1, keys2, g1vals, mask_vals, field_off};
  const int grid = grid_for_waves(B) + (gbias ? 1 : 0);      // + the workgroup that only sums the bias gradient
  if (vec_ok(De) && tables_float4_ok(t, mask_vals ? XF_MASK : XF_NONE) && all_aligned16(emb, g_emb, c1, c2)) {
#define CALL(LPR) \
  MI_LAUNCH("gather_fm_dual_bwd_rows", (k_gather_fm_dual_bwd_rows<LPR>), grid, kBlock, stream, rows, emb, g_y, g_emb, t, o, B, F, N, gbias)
    MI_DISPATCH_LPR(De / 4, CALL)
#undef CALL
  } else {
    MI_LAUNCH("gather_fm_dual_bwd_rows", k_gather_fm_dual_bwd_rows_anyD, grid, kBlock, stream, rows, emb, g_y, g_emb, t, o, B, F,
              De, N, gbias);
  }
  return launch_status();
}

int mi_gather_fm_dual_finish(float *A1, float *A2, const float *T1, const float *T2, const float *S1, const float *S2,
                             const uint8_t *M1, const uint8_t *M2, float *gS1, float *gS2, int64_t n1, int64_t n2,
                             int32_t De, int32_t xform, void *stream) {
  if (n1 < 0 || n2 < 0 || De <= 0 || xform < XF_NONE || xform > XF_MASK) return MI_ERR_INVALID_ARG;
  if (xform == XF_NONE) return MI_OK;      // the sums are the gradients
  if ((n1 > 0 && !A1) || (n2 > 0 && !A2)) return MI_ERR_INVALID_ARG;
  if (xform == XF_SOFT && ((n1 > 0 && (!T1 || !S1 || !gS1)) || (n2 > 0 && (!T2 || !S2 || !gS2)))) return MI_ERR_INVALID_ARG;
  if (xform == XF_MASK && ((n1 > 0 && !M1) || (n2 > 0 && !M2))) return MI_ERR_INVALID_ARG;
  const FinishArgs a{{A1, A2}, {T1, T2}, {S1, S2}, {M1, M2}, {gS1, gS2}, {A1 ? n1 * De : 0, A2 ? n2 * De : 0}};
  if (a.e[0] + a.e[1] == 0) return MI_OK;
  const int grid = grid_for_elems(a.e[0] + a.e[1]);
  if (xform == XF_SOFT) MI_LAUNCH("gather_fm_dual_finish", k_dual_finish<XF_SOFT>, grid, kBlock, stream, a);
  else MI_LAUNCH("gather_fm_dual_finish", k_dual_finish<XF_MASK>, grid, kBlock, stream, a);
  return launch_status();
}

int64_t mi_cerp_prune_loss_workspace_elems(int64_t n) {
  if (n <= 0) return 0;
  return (int64_t)prune_grid(n) + 1;      // the workgroups' partial sums, then the ticket word
}

int mi_cerp_prune_loss_fwd(const float *P, const float *Sp, const float *Q, const float *Sq, int64_t n, float k_tanh,
                           float *workspace, int32_t armed, float *out, void *stream) {
  if (n <= 0 || !P || !Sp || !Q || !Sq || !workspace || !out) return MI_ERR_INVALID_ARG;
  const int grid = prune_grid(n);
  unsigned *ticket = reinterpret_cast<unsigned *>(workspace + grid);
  if (!armed && hipMemsetAsync(ticket, 0, sizeof(unsigned), (hipStream_t)stream) != hipSuccess) return MI_ERR_LAUNCH;
  const PruneTables a{P, Sp, Q, Sq, n, k_tanh};
  if ((n & 3) == 0 && all_aligned16(P, Sp, Q, Sq))
    MI_LAUNCH("cerp_prune_loss_fwd", k_cerp_prune_loss_fwd<true>, grid, kBlock, stream, a, workspace, ticket, out);
  else
    MI_LAUNCH("cerp_prune_loss_fwd", k_cerp_prune_loss_fwd<false>, grid, kBlock, stream, a, workspace, ticket, out);
  return launch_status();
}

int mi_cerp_prune_loss_bwd(const float *P, const float *Sp, const float *Q, const float *Sq, int64_t n, float k_tanh,
                           const float *grad_out, float *gP, float *gSp, float *gQ, float *gSq, void *stream) {
  if (n <= 0 || !P || !Sp || !Q || !Sq || !grad_out || !gP || !gSp || !gQ || !gSq) return MI_ERR_INVALID_ARG;
  const PruneTables a{P, Sp, Q, Sq, n, k_tanh};
  const PruneGrads g{gP, gSp, gQ, gSq};
  const int grid = prune_grid(n);
  if ((n & 3) == 0 && all_aligned16(P, Sp, Q, Sq, gP, gSp, gQ, gSq))
    MI_LAUNCH("cerp_prune_loss_bwd", k_cerp_prune_loss_bwd<true>, grid, kBlock, stream, a, grad_out, g);
  else
    MI_LAUNCH("cerp_prune_loss_bwd", k_cerp_prune_loss_bwd<false>, grid, kBlock, stream, a, grad_out, g);
  return launch_status();
}

}  // extern "C"
