// lightgcn_step.hip — the LightGCN step either side of the propagation.
//
//  * BPR loss over rows picked from the propagated tables — src/losses.py:6-22 applied to
//    torch.index_select(all_user_emb, 0, users) etc. (src/trainer/lightgcn.py:395-399): gathers,
//    two row dots, -logsigmoid, mean in ONE launch; the backward scatters the three gradient rows
//    straight into the dense table gradients (what index_select's backward builds with index_add).
//  * validation scoring tail — src/trainer/lightgcn.py:122-138: scores[ind0, ind1] = -inf for the
//    items a user already has in train (a Python double loop in the reference; here a CSR row per
//    user on the device) and torch.topk(scores, k) indices, one workgroup per user row.
//
// Ordering of the top-k: score descending, ties by ascending item index (a strict total order, so
// the result does not depend on scheduling).
#include <type_traits>

#include "common.hpp"

namespace {
using namespace mi;

// The batch's (user, positive, negative) triples: three tables with their row counts, the index arrays (NULL = row b; the
// host allows that for BPR only, see rows<Nullable>) and the sticky error word (common convention of the lookups: an out-of-range id never
// touches memory, it is skipped and MI_IDX_OUT_OF_RANGE is OR-ed into *err).
struct Triples {
  const float *U;
  const int64_t *ui;
  const float *P;
  const int64_t *pi;
  const float *Nn;
  const int64_t *ni;
  int64_t B, nU, nP, nN;
  int D;
  int *err;
  // the table rows of triple b; false when one of them lies outside its table (Nullable: the loss is one whose index
  // arrays may be NULL; the other pays no test for it)
  template <bool Nullable>
  __device__ __forceinline__ bool rows(int64_t b, int64_t &ur, int64_t &pr, int64_t &nr) const {
    if constexpr (Nullable) ur = ui ? ui[b] : b, pr = pi ? pi[b] : b, nr = ni ? ni[b] : b;
    else ur = ui[b], pr = pi[b], nr = ni[b];
    return (uint64_t)ur < (uint64_t)nU && (uint64_t)pr < (uint64_t)nP && (uint64_t)nr < (uint64_t)nN;
  }
};

__device__ __forceinline__ float softplus(float x) {   // log(1 + e^x), stable
  return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
}

// The forward walk over the triples, in two lane mappings:
//   LPR > 0: rows of D = 4 LPR floats (LPR a power of two <= 64, 16-byte aligned tables): LPR lanes x float4 per sample,
//            64 / LPR samples per wave side by side.  A quarter of the workgroups of the other form at D = 64 — the launch
//            is a chain of round trips (ids, rows, partial, ticket, partials) and the ticket is ONE word every workgroup
//            adds to: same-address atomics serialise at ~26 ns apiece, 512 of them were most of the kernel's 10 us.
//   LPR = 0: any D, a wave per sample, lanes stride over d.
// The loss is a small type:
//   term(u, p, n)  the summand of one element (float) or of one lane's four (float4);
//   kNullable      whether its index arrays may be NULL;
//   kPerSample     true: the terms of a sample are summed over its lanes to d — an out-of-range triple reads nothing and
//                  counts as u = p = n = 0, d = 0 — and the sample's first lane accumulates epi(b, d);
//                  false: no per-sample step, every lane accumulates its own terms across samples and an out-of-range
//                  triple is skipped.
// Returns the lane's accumulator.
template <int LPR, class Loss>
__device__ __forceinline__ float walk_triples(const Triples &t, const Loss &loss) {
  constexpr int SPW = LPR ? kWave / LPR : 1;
  const int lane = threadIdx.x & 63, q = LPR ? lane % LPR : lane, k = LPR ? lane / LPR : 0;
  const int64_t step = (int64_t)gridDim.x * kWavesPerBlock * SPW;
  float acc = 0.f;
  bool bad = false;
  for (int64_t b0 = ((int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * SPW; b0 < t.B; b0 += step) {
    const int64_t b = b0 + k;
    const bool valid = b < t.B;
    int64_t ur, pr, nr;
    const bool ok = valid && t.rows<Loss::kNullable>(b, ur, pr, nr);
    bad |= valid && !ok;
    float d = Loss::kPerSample ? 0.f : acc;      // the sum the terms go to: this sample's own, or the lane's running one
    if (ok) {
      const float *u = t.U + ur * t.D, *p = t.P + pr * t.D, *n = t.Nn + nr * t.D;
      if constexpr (LPR != 0) d += loss.term(ld4(u + q * 4), ld4(p + q * 4), ld4(n + q * 4));
      else for (int j = lane; j < t.D; j += kWave) d += loss.term(u[j], p[j], n[j]);
    }
    if constexpr (Loss::kPerSample) {
      if constexpr (LPR != 0) {
#pragma unroll
        for (int m = 1; m < LPR; m <<= 1) d += __shfl_xor(d, m);
      } else {
        d = wave_sum(d);
      }
      if (q == 0 && valid) acc += loss.epi(b, d);
    } else {
      acc = d;
    }
  }
  if (__any(bad) && lane == 0 && t.err) atomicOr(t.err, MI_IDX_OUT_OF_RANGE);
  return acc;
}

// BPR: d = u . (p - n) = y_pos - y_neg per sample; sig[b] = sigmoid(-d) = -dL_b/dd; loss = mean_b -logsigmoid(d).
// part[blockIdx.x] = the workgroup's sum, joined by the last workgroup (grid_join).
// plus (nullable): another term of the step's objective (the trainer's reg_weight * get_reg_loss, a scalar an earlier
// launch wrote) joins in the last workgroup instead of through a scale launch and an add launch; loss[1] is then the bare
// BPR term beside the sum (what a trainer logs).
struct Bpr {
  static constexpr bool kNullable = true, kPerSample = true;
  float *sig;
  __device__ float term(float u, float p, float n) const { return u * (p - n); }
  __device__ float term(float4 u, float4 p, float4 n) const {
    return u.x * (p.x - n.x) + u.y * (p.y - n.y) + u.z * (p.z - n.z) + u.w * (p.w - n.w);
  }
  __device__ float epi(int64_t b, float d) const {
    sig[b] = 1.f / (1.f + expf(d));
    return softplus(-d);
  }
};

template <int LPR>
__device__ __forceinline__ void bpr_fwd(const Triples &t, float *sig, float *part, unsigned *ticket, float *loss,
                                        const float *plus, float plus_w) {
  float acc[1] = {walk_triples<LPR>(t, Bpr{sig})};
  grid_join(acc, part, ticket, [&](const float (&s)[1]) {
    loss[0] = s[0] / (float)t.B + (plus ? plus_w * plus[0] : 0.f);
    if (plus) loss[1] = s[0] / (float)t.B;
  });
}

__global__ __launch_bounds__(kBlock) void k_bpr_fwd(Triples t, float *__restrict__ sig, float *__restrict__ part,
                                                    unsigned *ticket, float *__restrict__ loss,
                                                    const float *__restrict__ plus, float plus_w) {
  bpr_fwd<0>(t, sig, part, ticket, loss, plus, plus_w);
}
template <int LPR>
__global__ __launch_bounds__(kBlock) void k_bpr_fwd_v(Triples t, float *__restrict__ sig, float *__restrict__ part,
                                                      unsigned *ticket, float *__restrict__ loss,
                                                      const float *__restrict__ plus, float plus_w) {
  bpr_fwd<LPR>(t, sig, part, ticket, loss, plus, plus_w);
}

// dU[ui[b]] += c (p - n), dP[pi[b]] += c u, dN[ni[b]] -= c u with c = -g * sig[b] / B
// (float atomics when an index array is given — rows repeat —, plain stores otherwise)
__global__ __launch_bounds__(kBlock) void k_bpr_bwd(Triples t, const float *__restrict__ sig, const float *__restrict__ g,
                                                    float *__restrict__ dU, float *__restrict__ dP, float *__restrict__ dN) {
  const int lane = threadIdx.x & 63, D = t.D;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const float scale = -g[0] / (float)t.B;
  for (int64_t b = wave0; b < t.B; b += nwaves) {
    int64_t ur, pr, nr;
    if (!t.rows<Bpr::kNullable>(b, ur, pr, nr)) continue;  // flagged by the forward; nothing is read or added out of bounds
    const float c = scale * sig[b];
    for (int j = lane; j < D; j += kWave) {
      const float u = t.U[ur * D + j], p = t.P[pr * D + j], q = t.Nn[nr * D + j];
      if (dU) { if (t.ui) atomicAdd(dU + ur * D + j, c * (p - q)); else dU[ur * D + j] = c * (p - q); }
      if (dP) { if (t.pi) atomicAdd(dP + pr * D + j, c * u); else dP[pr * D + j] = c * u; }
      if (dN) { if (t.ni) atomicAdd(dN + nr * D + j, -c * u); else dN[nr * D + j] = -c * u; }
    }
  }
}

// ---- L2 regulariser over the batch rows: LightGCN.get_reg_loss (src/models/lightgcn.py:90-100) ----------------
//   reg = ( ||U[ui]||_F^2 + ||P[pi]||_F^2 + ||Nn[ni]||_F^2 ) / (2 B)
// (x.norm(2).pow(2) of the three gathered [B, D] blocks): gathers, squares and the deterministic mean-style join in
// one launch; backward dU[ui[b]] += g * U[ui[b]] / B etc. (float atomics into caller-zeroed dense gradients).
struct RowSq {
  static constexpr bool kNullable = false, kPerSample = false;
  __device__ float term(float u, float p, float n) const { return u * u + p * p + n * n; }
  __device__ float term(float4 u, float4 p, float4 n) const { return dot4(u, u) + dot4(p, p) + dot4(n, n); }
};

template <int LPR>
__device__ __forceinline__ void rowsq_fwd(const Triples &t, float *part, unsigned *ticket, float *out) {
  float acc[1] = {walk_triples<LPR>(t, RowSq{})};
  grid_join(acc, part, ticket, [&](const float (&s)[1]) { out[0] = s[0] / (2.f * (float)t.B); });
}

__global__ __launch_bounds__(kBlock) void k_rowsq_fwd(Triples t, float *__restrict__ part, unsigned *ticket,
                                                      float *__restrict__ out) {
  rowsq_fwd<0>(t, part, ticket, out);
}
template <int LPR>
__global__ __launch_bounds__(kBlock) void k_rowsq_fwd_v(Triples t, float *__restrict__ part, unsigned *ticket,
                                                        float *__restrict__ out) {
  rowsq_fwd<LPR>(t, part, ticket, out);
}

__global__ __launch_bounds__(kBlock) void k_rowsq_bwd(Triples t, const float *__restrict__ g, float *__restrict__ dU,
                                                      float *__restrict__ dP, float *__restrict__ dN) {
  const int lane = threadIdx.x & 63, D = t.D;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const float c = g[0] / (float)t.B;        // d/dw of w^2 / (2B) = w / B
  for (int64_t b = wave0; b < t.B; b += nwaves) {
    int64_t ur, pr, nr;
    if (!t.rows<RowSq::kNullable>(b, ur, pr, nr)) continue;
    for (int j = lane; j < D; j += kWave) {
      if (dU) atomicAdd(dU + ur * D + j, c * t.U[ur * D + j]);
      if (dP) atomicAdd(dP + pr * D + j, c * t.P[pr * D + j]);
      if (dN) atomicAdd(dN + nr * D + j, c * t.Nn[nr * D + j]);
    }
  }
}

// ---- CERP's batch-row terms: get_prune_and_reg_loss_lightgcn (src/models/embeddings/cerp_embedding_utils.py:15-62) on the
// materialised tables, both from one read of each row:
//   out[0] = reg   = ( sum_b |U[ui[b]]|^2 + sum_b |I[pi[b]]|^2 + sum_k |I[ni[k]]|^2 ) / (2 B)
//   out[1] = prune = -( sum_{b: uvalid[b]} |tanh(K U[ui[b]])|^2 + sum_b |tanh(K I[pi[b]])|^2 + sum_k |tanh(K I[ni[k]])|^2 )
// B users and positives, Bn negatives; uvalid flags the first occurrence of each user (the reference's torch.unique).
// Row x of the B + B + Bn is one wave's; an id outside its table is skipped and flagged.  The workgroup partials (two
// per workgroup) are joined by the last workgroup to take a ticket, in index order (grid_join).
struct BatchRows {
  const float *U, *I;
  const int64_t *ui, *pi, *ni;
  const uint8_t *uvalid;
  int64_t B, Bn, nU, nI;
  int D;
  // row x of the batch: its table row (NULL = out of range) and whether it counts in the prune term
  __device__ __forceinline__ const float *row(int64_t x, bool &prune, bool &bad, int64_t &off) const {
    const bool user = x < B;
    const int64_t id = user ? ui[x] : (x < 2 * B ? pi[x - B] : ni[x - 2 * B]);
    prune = !user || uvalid[x] != 0;
    bad = (uint64_t)id >= (uint64_t)(user ? nU : nI);
    off = id * D;
    return bad ? nullptr : (user ? U : I) + off;
  }
};

__global__ __launch_bounds__(kBlock) void k_reg_prune_fwd(BatchRows a, float k_tanh, int *err, float *__restrict__ part,
                                                          unsigned *ticket, float *__restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float acc[2] = {0.f, 0.f};                   // squares, tanh squares
  bool any_bad = false;
  const int64_t R = 2 * a.B + a.Bn;
  for (int64_t x = (int64_t)blockIdx.x * kWavesPerBlock + wv; x < R; x += (int64_t)gridDim.x * kWavesPerBlock) {
    bool prune, bad;
    int64_t off;
    const float *w = a.row(x, prune, bad, off);
    if (bad) { any_bad = true; continue; }
    for (int j = lane; j < a.D; j += kWave) {
      const float v = w[j], t = tanhf(k_tanh * v);
      acc[0] += v * v;
      acc[1] += prune ? t * t : 0.f;
    }
  }
  if (any_bad && lane == 0 && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
  grid_join(acc, part, ticket, [&](const float (&s)[2]) {
    out[0] = s[0] / (2.f * (float)a.B);
    out[1] = -s[1];
  });
}

// dTable[row] += g[0] w / B + g[1] d(-tanh^2(K w))/dw,   d(-tanh^2(K w))/dw = -2 K tanh(K w) (1 - tanh^2(K w))
// (float atomics into caller-zeroed dense gradients, as k_rowsq_bwd: a batch's rows repeat)
__global__ __launch_bounds__(kBlock) void k_reg_prune_bwd(BatchRows a, float k_tanh, const float *__restrict__ g,
                                                          float *__restrict__ dU, float *__restrict__ dI) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float cr = g[0] / (float)a.B, cp = -2.f * k_tanh * g[1];
  const int64_t R = 2 * a.B + a.Bn;
  for (int64_t x = (int64_t)blockIdx.x * kWavesPerBlock + wv; x < R; x += (int64_t)gridDim.x * kWavesPerBlock) {
    bool prune, bad;
    int64_t off;
    const float *w = a.row(x, prune, bad, off);
    float *d = x < a.B ? dU : dI;
    if (bad || !d) continue;
    for (int j = lane; j < a.D; j += kWave) {
      const float v = w[j], t = tanhf(k_tanh * v);
      atomicAdd(d + off + j, cr * v + (prune ? cp * t * (1.f - t * t) : 0.f));
    }
  }
}

// ------------------------------------------------------------------ mask + top-k per row ----
constexpr int kCand = 2048;   // candidate slots in LDS
constexpr int kSample = 4096; // row prefix that sets the candidate bound

struct Cand {
  float v;
  int i;
};

// f(value, column) over one row, 256 threads; float4 loads (4 independent elements in flight per
// iteration, two iterations unrolled) when the row is 16-byte aligned
template <class Fn>
__device__ __forceinline__ void scan_row(const float *__restrict__ row, int64_t ncol, bool vec, Fn f) {
  const int tid = threadIdx.x;
  int64_t done = 0;
  if (vec) {
    const int64_t n4 = ncol >> 2;
#pragma unroll 2
    for (int64_t c = tid; c < n4; c += kBlock) {
      const float4 x = ld4(row + c * 4);
      const int j = (int)(c * 4);
      f(x.x, j);
      f(x.y, j + 1);
      f(x.z, j + 2);
      f(x.w, j + 3);
    }
    done = n4 << 2;
  }
  for (int64_t j = done + tid; j < ncol; j += kBlock) f(row[j], (int)j);
}
__device__ __forceinline__ bool before(float av, int ai, float bv, int bi) {
  return av > bv || (av == bv && ai < bi);
}

__global__ __launch_bounds__(kBlock) void k_mask_topk(
    float *__restrict__ scores, int64_t ld, int64_t ncol, const int64_t *__restrict__ users,
    const int64_t *__restrict__ crow, const int64_t *__restrict__ col, int k,
    int64_t *__restrict__ out_idx, float *__restrict__ out_val) {
  __shared__ Cand cand[kCand];
  __shared__ float lmax[kBlock];
  __shared__ int lidx[kBlock];
  __shared__ float thr_v;
  __shared__ int thr_i;
  __shared__ int count;
  const int tid = threadIdx.x;
  float *row = scores + (int64_t)blockIdx.x * ld;
  const float ninf = -__builtin_huge_valf();

  if (crow) {   // items the user already interacted with in train never rank
    const int64_t u = users ? users[blockIdx.x] : blockIdx.x;
    for (int64_t e = crow[u] + tid; e < crow[u + 1]; e += kBlock) {
      const int64_t c = col[e];
      if ((uint64_t)c < (uint64_t)ncol) row[c] = ninf;
    }
    __syncthreads();
  }

  // pass 1 over a PREFIX of the row (a full second read of a 150 KB row would come from HBM again: 2048
  // rows are in flight): every thread's best element of the sample; the k-th best of those 256 bounds the
  // k-th best of the whole row from below
  const bool vec = ((ld & 3) == 0) && aligned16(scores);
  float bv = ninf;
  int bi = 0x7fffffff;
  scan_row(row, ncol < kSample ? ncol : (int64_t)kSample, vec, [&](float v, int j) {
    if (before(v, j, bv, bi)) { bv = v; bi = j; }
  });
  lmax[tid] = bv;
  lidx[tid] = bi;
  if (tid == 0) {
    count = 0;
    thr_v = ninf;          // default bound admits everything (fewer than k threads own an element)
    thr_i = 0x7fffffff;
  }
  __syncthreads();
  if (bi != 0x7fffffff) {
    int rank = 0;
    for (int t = 0; t < kBlock; ++t) rank += before(lmax[t], lidx[t], bv, bi);
    if (rank == k - 1) { thr_v = bv; thr_i = bi; }
  }
  __syncthreads();
  const float tv = thr_v;
  const int ti = thr_i;
  // pass 2, the one full read: everything not after the bound is a candidate (~k * ncol / kSample of them)
  scan_row(row, ncol, vec, [&](float v, int j) {
    if (!before(tv, ti, v, j)) {
      const int s = atomicAdd(&count, 1);
      if (s < kCand) { cand[s].v = v; cand[s].i = j; }
    }
  });
  __syncthreads();
  const int n = count;
  if (n <= kCand) {
    // bitonic sort of the candidates in LDS under the strict total order (padded to a power of two with
    // entries that sort last); the first k are the answer
    int P = 64;
    while (P < n) P <<= 1;
    for (int a = n + tid; a < P; a += kBlock) { cand[a].v = ninf; cand[a].i = 0x7fffffff; }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = tid; t < (P >> 1); t += kBlock) {
          const int lo = 2 * t - (t & (stride - 1));
          const int hi = lo + stride;
          const Cand a = cand[lo], b = cand[hi];
          const bool desc = (lo & size) == 0;
          const bool swap = desc ? before(b.v, b.i, a.v, a.i) : before(a.v, a.i, b.v, b.i);
          if (swap) { cand[lo] = b; cand[hi] = a; }
        }
        __syncthreads();
      }
    }
    if (tid < k) {
      out_idx[(int64_t)blockIdx.x * k + tid] = cand[tid].i;
      if (out_val) out_val[(int64_t)blockIdx.x * k + tid] = cand[tid].v;
    }
    return;
  }
  // too many candidates (massive ties): k rounds of "best element after the previous pick"
  float pv = __builtin_huge_valf();
  int pi = -1;
  for (int r = 0; r < k; ++r) {
    float cv = ninf;
    int ci = 0x7fffffff;
    scan_row(row, ncol, vec, [&](float v, int j) {
      const bool after_prev = (pi < 0) || before(pv, pi, v, j);
      if (after_prev && before(v, j, cv, ci)) { cv = v; ci = j; }
    });
    __syncthreads();
    lmax[tid] = cv;
    lidx[tid] = ci;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
      if (tid < s && before(lmax[tid + s], lidx[tid + s], lmax[tid], lidx[tid])) {
        lmax[tid] = lmax[tid + s];
        lidx[tid] = lidx[tid + s];
      }
      __syncthreads();
    }
    pv = lmax[0];
    pi = lidx[0];
    if (tid == 0) {
      out_idx[(int64_t)blockIdx.x * k + r] = pi;
      if (out_val) out_val[(int64_t)blockIdx.x * k + r] = pv;
    }
    __syncthreads();
  }
}

}  // namespace

// the argument checks of the six triple entry points (index arrays may be NULL where `nullable`: row b, which the table
// must then have)
static bool triples(Triples &t, bool nullable, const float *U, const int64_t *ui, const float *P, const int64_t *pi,
                    const float *Nn, const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, int32_t *err) {
  if (B <= 0 || D <= 0 || !U || !P || !Nn) return false;
  if (nullable ? (!ui && nU < B) || (!pi && nP < B) || (!ni && nN < B) : !ui || !pi || !ni) return false;
  t = Triples{U, ui, P, pi, Nn, ni, B, nU, nP, nN, D, err};
  return true;
}

// The forward launch of both losses: workspace = per-workgroup partials, then the ticket word at
// workspace[mi_bpr_workspace_elems(B) - 1] in either form — zeroed here once per call (captured as a memset node in a
// graph) unless the caller keeps it armed.  launch(LPR constant, grid, ticket) starts the float4 kernel of LPR lanes per
// row, or for LPR = 0 the any-D one.
template <class Launch>
static int triples_fwd(const Triples &t, bool zero_ticket, float *workspace, void *stream, Launch launch) {
  const int grid = grid_for_waves(t.B);
  if (zero_ticket && hipMemsetAsync(workspace + grid, 0, sizeof(unsigned), (hipStream_t)stream) != hipSuccess)
    return MI_ERR_LAUNCH;
  unsigned *ticket = reinterpret_cast<unsigned *>(workspace + grid);
  if (vec_ok(t.D) && all_aligned16(t.U, t.P, t.Nn)) {
    const int lpr = t.D / 4, spw = kWave / lpr;
#define FWDV(L) launch(std::integral_constant<int, L>{}, grid_for_waves((t.B + spw - 1) / spw), ticket)
    MI_DISPATCH_LPR(lpr, FWDV)
#undef FWDV
  } else {
    launch(std::integral_constant<int, 0>{}, grid, ticket);
  }
  return launch_status();
}

extern "C" {

int64_t mi_bpr_workspace_elems(int64_t B) {
  if (B < 0) return 0;
  return grid_for_waves(B) + 1;   // per-block partial sums + the ticket word
}

static int bpr_fwd_impl(bool zero_ticket, const float *U, const int64_t *ui, const float *P, const int64_t *pi, const float *Nn,
               const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, int32_t *err,
               float *sig, float *workspace, float *loss, void *stream, const float *plus = nullptr, float plus_w = 0.f) {
  Triples t;
  if (!triples(t, true, U, ui, P, pi, Nn, ni, B, D, nU, nP, nN, err) || !sig || !workspace || !loss) return MI_ERR_INVALID_ARG;
  return triples_fwd(t, zero_ticket, workspace, stream, [&](auto lpr, int grid, unsigned *ticket) {
    if constexpr (decltype(lpr)::value != 0)
      MI_LAUNCH("bpr_fwd", (k_bpr_fwd_v<decltype(lpr)::value>), grid, kBlock, stream, t, sig, workspace, ticket, loss, plus, plus_w);
    else
      MI_LAUNCH("bpr_fwd", k_bpr_fwd, grid, kBlock, stream, t, sig, workspace, ticket, loss, plus, plus_w);
  });
}

int mi_bpr_fwd(const float *U, const int64_t *ui, const float *P, const int64_t *pi, const float *Nn,
               const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, int32_t *err,
               float *sig, float *workspace, float *loss, void *stream) {
  return bpr_fwd_impl(true, U, ui, P, pi, Nn, ni, B, D, nU, nP, nN, err, sig, workspace, loss, stream);
}

// the same without the memset node: the caller promises that the ticket word (workspace[mi_bpr_workspace_elems(B) - 1])
// is zero on entry — the kernel leaves it zero, so a workspace zeroed ONCE and kept serves every later call
int mi_bpr_fwd_armed(const float *U, const int64_t *ui, const float *P, const int64_t *pi, const float *Nn,
               const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, int32_t *err,
               float *sig, float *workspace, float *loss, void *stream) {
  return bpr_fwd_impl(false, U, ui, P, pi, Nn, ni, B, D, nU, nP, nN, err, sig, workspace, loss, stream);
}

int mi_bpr_fwd_plus(const float *U, const int64_t *ui, const float *P, const int64_t *pi, const float *Nn,
                    const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, int32_t *err,
                    float *sig, float *workspace, int32_t armed, const float *plus, float plus_weight, float *loss,
                    void *stream) {
  return bpr_fwd_impl(!armed, U, ui, P, pi, Nn, ni, B, D, nU, nP, nN, err, sig, workspace, loss, stream, plus, plus_weight);
}

int mi_bpr_bwd(const float *U, const int64_t *ui, const float *P, const int64_t *pi, const float *Nn,
               const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, const float *sig,
               const float *g, float *dU, float *dP, float *dN, void *stream) {
  Triples t;
  if (!triples(t, true, U, ui, P, pi, Nn, ni, B, D, nU, nP, nN, nullptr) || !sig || !g) return MI_ERR_INVALID_ARG;
  MI_LAUNCH("bpr_bwd", k_bpr_bwd, grid_for_waves(B), kBlock, stream, t, sig, g, dU, dP, dN);
  return launch_status();
}

static int rowsq_fwd_impl(bool zero_ticket, const float *U, const int64_t *ui, const float *P, const int64_t *pi, const float *Nn,
                 const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, int32_t *err,
                 float *workspace, float *out, void *stream) {
  Triples t;
  if (!triples(t, false, U, ui, P, pi, Nn, ni, B, D, nU, nP, nN, err) || !workspace || !out) return MI_ERR_INVALID_ARG;
  return triples_fwd(t, zero_ticket, workspace, stream, [&](auto lpr, int grid, unsigned *ticket) {
    if constexpr (decltype(lpr)::value != 0)
      MI_LAUNCH("rowsq_fwd", (k_rowsq_fwd_v<decltype(lpr)::value>), grid, kBlock, stream, t, workspace, ticket, out);
    else
      MI_LAUNCH("rowsq_fwd", k_rowsq_fwd, grid, kBlock, stream, t, workspace, ticket, out);
  });
}

int mi_rowsq_fwd(const float *U, const int64_t *ui, const float *P, const int64_t *pi, const float *Nn,
                 const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, int32_t *err,
                 float *workspace, float *out, void *stream) {
  return rowsq_fwd_impl(true, U, ui, P, pi, Nn, ni, B, D, nU, nP, nN, err, workspace, out, stream);
}

int mi_rowsq_fwd_armed(const float *U, const int64_t *ui, const float *P, const int64_t *pi, const float *Nn,
                 const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, int32_t *err,
                 float *workspace, float *out, void *stream) {      // see mi_bpr_fwd_armed
  return rowsq_fwd_impl(false, U, ui, P, pi, Nn, ni, B, D, nU, nP, nN, err, workspace, out, stream);
}

int mi_rowsq_bwd(const float *U, const int64_t *ui, const float *P, const int64_t *pi, const float *Nn,
                 const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, const float *g,
                 float *dU, float *dP, float *dN, void *stream) {
  Triples t;
  if (!triples(t, false, U, ui, P, pi, Nn, ni, B, D, nU, nP, nN, nullptr) || !g) return MI_ERR_INVALID_ARG;
  MI_LAUNCH("rowsq_bwd", k_rowsq_bwd, grid_for_waves(B), kBlock, stream, t, g, dU, dP, dN);
  return launch_status();
}

static bool batch_rows(BatchRows &a, const float *U, const float *I, const int64_t *ui, const int64_t *pi, const int64_t *ni,
                       const uint8_t *uvalid, int64_t B, int64_t Bn, int32_t D, int64_t nU, int64_t nI) {
  if (B <= 0 || Bn < 0 || D <= 0 || nU < 0 || nI < 0 || !U || !I || !ui || !pi || (Bn > 0 && !ni) || !uvalid) return false;
  a = BatchRows{U, I, ui, pi, ni, uvalid, B, Bn, nU, nI, D};
  return true;
}

int64_t mi_reg_prune_rows_workspace_elems(int64_t B, int64_t Bn) {
  if (B < 0 || Bn < 0) return 0;
  return 2 * (int64_t)grid_for_waves(2 * B + Bn) + 1;   // two partials per workgroup + the ticket word
}

int mi_reg_prune_rows_fwd(const float *U, const float *I, const int64_t *ui, const int64_t *pi, const int64_t *ni,
                          const uint8_t *uvalid, int64_t B, int64_t Bn, int32_t D, int64_t nU, int64_t nI, float k_tanh,
                          int32_t *err, float *workspace, int32_t armed, float *out, void *stream) {
  BatchRows a;
  if (!batch_rows(a, U, I, ui, pi, ni, uvalid, B, Bn, D, nU, nI) || !workspace || !out) return MI_ERR_INVALID_ARG;
  const int grid = grid_for_waves(2 * B + Bn);
  if (!armed && hipMemsetAsync(workspace + 2 * grid, 0, sizeof(unsigned), (hipStream_t)stream) != hipSuccess)
    return MI_ERR_LAUNCH;
  MI_LAUNCH("reg_prune_rows_fwd", k_reg_prune_fwd, grid, kBlock, stream, a, k_tanh, err, workspace,
            reinterpret_cast<unsigned *>(workspace + 2 * grid), out);
  return launch_status();
}

int mi_reg_prune_rows_bwd(const float *U, const float *I, const int64_t *ui, const int64_t *pi, const int64_t *ni,
                          const uint8_t *uvalid, int64_t B, int64_t Bn, int32_t D, int64_t nU, int64_t nI, float k_tanh,
                          const float *g, float *dU, float *dI, void *stream) {
  BatchRows a;
  if (!batch_rows(a, U, I, ui, pi, ni, uvalid, B, Bn, D, nU, nI) || !g) return MI_ERR_INVALID_ARG;
  MI_LAUNCH("reg_prune_rows_bwd", k_reg_prune_bwd, grid_for_waves(2 * B + Bn), kBlock, stream, a, k_tanh, g, dU, dI);
  return launch_status();
}

int mi_mask_topk_rows(float *scores, int64_t ld, int64_t nrows, int64_t ncol, const int64_t *users,
                      const int64_t *crow, const int64_t *col, int32_t k, int64_t *out_idx,
                      float *out_val, void *stream) {
  if (nrows < 0 || ncol < 0 || ld < ncol || k < 1) return MI_ERR_INVALID_ARG;
  if (k > ncol || ncol >= (1ll << 31)) return MI_ERR_INVALID_ARG;   // torch.topk raises for k > size
  if (k > kBlock) return MI_ERR_UNSUPPORTED;
  if (nrows == 0) return MI_OK;
  if (!scores || !out_idx || (crow && !col)) return MI_ERR_INVALID_ARG;
  if (nrows > 0x7fffffff) return MI_ERR_UNSUPPORTED;
  MI_LAUNCH("mask_topk", k_mask_topk, (int)nrows, kBlock, stream, scores, ld, ncol, users, crow, col, k,
            out_idx, out_val);
  return launch_status();
}

}  // extern "C"
