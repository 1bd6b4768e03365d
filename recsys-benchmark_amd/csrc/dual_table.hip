// dual_table.hip — the two-table compositional family (QR hashing, CERP, CERP retrain) in TABLE form:
//   out[i] = T1'[i % mod1] (op) T2'[i / div2]   for i = 0 .. N-1
// what get_weight() of those tables is (src/models/embeddings/qr_embedding.py:111-113, cerp_embedding.py:177-180 and
// :369-372: the module's forward over arange(N)), and what a collaborative-filtering model asks for on every step.  With
// ids 0 .. N-1 there is nothing to look up: no index tensor, no range check, and the backward is a fixed reduction —
//   row r of T1 (remainder table) receives rows r, r + mod1, r + 2 mod1, ...        of g
//   row r of T2 (quotient table)  receives rows r div2 .. (r + 1) div2 - 1           of g
// so every gradient element is summed by ONE thread in ascending i and written once with a plain store: no atomics, no
// zero fill, the same bits on every run.
//
// Layout: one thread per float4 (De % 4 == 0, 16-byte aligned operands; nothing crosses lanes).  Forward: thread e owns
// out[e / C, 4 (e % C) ..] with C = De / 4.  Backward: a work item is (table, row, chunk of that row's contributors); a
// row with at most kLongRow contributors is one chunk and its owner applies the transform's derivative (a function of the
// table element only) after the sum and stores gT / gS.  Longer rows (QR's remainder table: `divider` rows of N / divider
// contributors) are cut into chunks of kChunk contributors — a constant, so the order of additions depends on the
// shapes only —, each chunk's raw sum goes to the workspace, and a second launch joins a row's chunks in a fixed order
// (thread t adds chunks t, t + 256, ... in turn, then a fixed pairwise tree over the 256 threads) and applies the
// derivative.
#include "dual_xform.hpp"

namespace {
using namespace mi;

constexpr int kLongRow = 16;   // contributors a single thread walks before the row is cut
constexpr int kChunk = 8;      // contributors per chunk of a cut row

struct TableArgs {
  const float *T1, *T2, *S1, *S2;
  const uint8_t *M1, *M2;
  uint32_t N, C;               // rows of the output, float4s per table row
  uint32_t n1, n2, mod1, div2;
  int op;
};

// how each table's rows are cut: chunks per row (1 = the owner finishes the row itself)
struct Cut {
  uint32_t nch1, nch2;
};

inline uint32_t chunks_for(int64_t contributors) {
  return contributors > kLongRow ? (uint32_t)((contributors + kChunk - 1) / kChunk) : 1u;
}

inline Cut cut_of(int64_t N, int64_t mod1, int64_t div2) {
  return Cut{chunks_for((N + mod1 - 1) / mod1), chunks_for(div2 < N ? div2 : N)};
}

template <int XF>
__global__ __launch_bounds__(kBlock) void k_dual_table_fwd(TableArgs a, float *__restrict__ out) {
  const uint32_t total = a.N * a.C, De = a.C * 4;
  for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < total; e += gridDim.x * kBlock) {
    const uint32_t i = e / a.C, c = e - i * a.C;
    const uint32_t i1 = i % a.mod1, i2 = i / a.div2;
    const float4 x = load_row4<XF>(a.T1, a.S1, a.M1, (int64_t)i1 * De + c * 4);
    const float4 y = load_row4<XF>(a.T2, a.S2, a.M2, (int64_t)i2 * De + c * 4);
    if (a.op == OP_CAT) {
      st4(out + (int64_t)i * 2 * De + c * 4, x);
      st4(out + (int64_t)i * 2 * De + De + c * 4, y);
    } else {
      st4(out + (int64_t)i * De + c * 4, a.op == OP_MULT ? mul4(x, y) : add4(x, y));
    }
  }
}

// gT (and gS) of one float4 of a table from the finished sum `s` of its contributors:
//   none: gT = s;   mask: gT = M ? s : 0;
//   soft (y = sign(w) relu(|w| - sig(t))): gT = s [|w| > sig(t)],  gS = -s sign(w) [|w| > sig(t)] sig(t) (1 - sig(t))
template <int XF>
__device__ __forceinline__ void finish(float4 s, const float *T, const float *S, const uint8_t *M, float *gT, float *gS, int64_t o) {
  if constexpr (XF == XF_NONE) {
    st4(gT + o, s);
  } else if constexpr (XF == XF_MASK) {
    const uchar4 m = *reinterpret_cast<const uchar4 *>(M + o);
    st4(gT + o, make_float4(m.x ? s.x : 0.f, m.y ? s.y : 0.f, m.z ? s.z : 0.f, m.w ? s.w : 0.f));
  } else {
    const float4 w = ld4(T + o), l = ld4(S + o);
    const float sv[4] = {s.x, s.y, s.z, s.w}, wv[4] = {w.x, w.y, w.z, w.w}, lv[4] = {l.x, l.y, l.z, l.w};
    float gw[4], gs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float t = sigmoidf_(lv[k]);
      const float keep = (fabsf(wv[k]) - t > 0.f) ? 1.f : 0.f;
      gs[k] = -sv[k] * signf_(wv[k]) * keep * t * (1.f - t);
      gw[k] = sv[k] * keep;
    }
    st4(gT + o, make_float4(gw[0], gw[1], gw[2], gw[3]));
    st4(gS + o, make_float4(gs[0], gs[1], gs[2], gs[3]));
  }
}

struct TableGrads {
  float *gT1, *gT2, *gS1, *gS2;
  float *ws;                   // chunk sums of the cut rows: [n1 * nch1 * De] (when nch1 > 1) then [n2 * nch2 * De] (when nch2 > 1)
};

template <int XF>
__global__ __launch_bounds__(kBlock) void k_dual_table_bwd(TableArgs a, Cut cut, const float *__restrict__ g, TableGrads gr) {
  const uint32_t De = a.C * 4;
  const uint32_t items1 = a.n1 * cut.nch1, items = items1 + a.n2 * cut.nch2;
  const uint32_t total = items * a.C;
  const int64_t gstride = a.op == OP_CAT ? 2 * (int64_t)De : De;
  for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < total; e += gridDim.x * kBlock) {
    const uint32_t item = e / a.C, c = e - item * a.C;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (item < items1) {
      // ---- remainder table: contributors i = row + j mod1
      const uint32_t row = item / cut.nch1, ch = item - row * cut.nch1;
      const uint32_t cnt = (row < a.N && row < a.mod1) ? (a.N - 1 - row) / a.mod1 + 1 : 0;
      const uint32_t j0 = cut.nch1 > 1 ? ch * kChunk : 0;
      const uint32_t j1 = cut.nch1 > 1 ? min(cnt, j0 + kChunk) : cnt;
#pragma unroll 8
      for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t i = row + j * a.mod1;
        float4 v = ld4(g + (int64_t)i * gstride + c * 4);
        if (a.op == OP_MULT) v = mul4(v, load_row4<XF>(a.T2, a.S2, a.M2, (int64_t)(i / a.div2) * De + c * 4));
        s = add4(s, v);
      }
      if (cut.nch1 > 1) st4(gr.ws + (int64_t)item * De + c * 4, s);
      else finish<XF>(s, a.T1, a.S1, a.M1, gr.gT1, gr.gS1, (int64_t)row * De + c * 4);
    } else {
      // ---- quotient table: contributors i = row div2 + j
      const uint32_t it2 = item - items1;
      const uint32_t row = it2 / cut.nch2, ch = it2 - row * cut.nch2;
      const uint64_t first = (uint64_t)row * a.div2;
      const uint32_t cnt = first < a.N ? (uint32_t)min((uint64_t)a.div2, (uint64_t)a.N - first) : 0;
      const uint32_t j0 = cut.nch2 > 1 ? ch * kChunk : 0;
      const uint32_t j1 = cut.nch2 > 1 ? min(cnt, j0 + kChunk) : cnt;
      const int64_t half = a.op == OP_CAT ? De : 0;
#pragma unroll 8
      for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t i = (uint32_t)first + j;
        float4 v = ld4(g + (int64_t)i * gstride + half + c * 4);
        if (a.op == OP_MULT) v = mul4(v, load_row4<XF>(a.T1, a.S1, a.M1, (int64_t)(i % a.mod1) * De + c * 4));
        s = add4(s, v);
      }
      if (cut.nch2 > 1) {
        const int64_t base = cut.nch1 > 1 ? (int64_t)items1 * De : 0;
        st4(gr.ws + base + (int64_t)it2 * De + c * 4, s);
      } else {
        finish<XF>(s, a.T2, a.S2, a.M2, gr.gT2, gr.gS2, (int64_t)row * De + c * 4);
      }
    }
  }
}

// The cut rows: one workgroup per (table, row, float4 column) in turn.  Thread t adds the row's chunks t, t + 256, ... in
// that order, then the 256 partial sums are folded by a fixed pairwise tree in LDS.
template <int XF>
__global__ __launch_bounds__(kBlock) void k_dual_table_join(TableArgs a, Cut cut, TableGrads gr) {
  __shared__ float4 part[kBlock];
  const uint32_t De = a.C * 4;
  const uint32_t rows1 = cut.nch1 > 1 ? a.n1 : 0, rows2 = cut.nch2 > 1 ? a.n2 : 0;
  for (uint32_t w = blockIdx.x; w < (rows1 + rows2) * a.C; w += gridDim.x) {
    const uint32_t rw = w / a.C, c = w - rw * a.C;
    const bool first = rw < rows1;
    const uint32_t row = first ? rw : rw - rows1, nch = first ? cut.nch1 : cut.nch2;
    const float *src = gr.ws + (first ? 0 : (int64_t)rows1 * cut.nch1 * De) + (int64_t)row * nch * De + c * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t k = threadIdx.x; k < nch; k += kBlock) s = add4(s, ld4(src + (int64_t)k * De));
    __syncthreads();             // (the previous item's readers are done with `part`)
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
      if ((int)threadIdx.x < h) part[threadIdx.x] = add4(part[threadIdx.x], part[threadIdx.x + h]);
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (first) finish<XF>(part[0], a.T1, a.S1, a.M1, gr.gT1, gr.gS1, (int64_t)row * De + c * 4);
      else finish<XF>(part[0], a.T2, a.S2, a.M2, gr.gT2, gr.gS2, (int64_t)row * De + c * 4);
    }
  }
}

inline int grid_for(int64_t threads) {
  int64_t g = (threads + kBlock - 1) / kBlock;
  return (int)(g < 1 ? 1 : (g > kMaxGrid ? kMaxGrid : g));
}

// argument checks shared by the three entry points; MI_OK, MI_ERR_INVALID_ARG or MI_ERR_UNSUPPORTED
inline int fill(TableArgs &a, const float *T1, const float *T2, const float *S1, const float *S2, const uint8_t *M1,
                const uint8_t *M2, int64_t N, int32_t De, int64_t n1, int64_t n2, int64_t mod1, int64_t div2, int32_t op,
                int32_t xform) {
  if (N < 0 || De <= 0 || n1 <= 0 || n2 <= 0 || mod1 <= 0 || div2 <= 0) return MI_ERR_INVALID_ARG;
  if (op < OP_MULT || op > OP_CAT || xform < XF_NONE || xform > XF_MASK) return MI_ERR_INVALID_ARG;
  if (!T1 || !T2 || (xform == XF_SOFT && (!S1 || !S2)) || (xform == XF_MASK && (!M1 || !M2))) return MI_ERR_INVALID_ARG;
  // every row 0 .. N-1 must find its two table rows
  if (n1 < (N < mod1 ? N : mod1) || n2 < (N + div2 - 1) / div2) return MI_ERR_INVALID_ARG;
  if (De % 4 != 0 || De / 4 > kBlock) return MI_ERR_UNSUPPORTED;
  const bool al = aligned16(T1) && aligned16(T2) && (xform != XF_SOFT || (aligned16(S1) && aligned16(S2))) &&
                  (xform != XF_MASK || (((uintptr_t)M1 & 3) == 0 && ((uintptr_t)M2 & 3) == 0));
  if (!al) return MI_ERR_UNSUPPORTED;
  // 32-bit element counters: the output, and the backward's work items
  const Cut cut = cut_of(N, mod1, div2);
  const int64_t lim = (int64_t)1 << 31;
  if (N * De * 2 >= lim || n1 >= lim || n2 >= lim || mod1 >= lim || div2 >= lim ||
      (n1 * cut.nch1 + n2 * cut.nch2) * De >= lim)
    return MI_ERR_UNSUPPORTED;
  a.T1 = T1; a.T2 = T2; a.S1 = S1; a.S2 = S2; a.M1 = M1; a.M2 = M2;
  a.N = (uint32_t)N; a.C = (uint32_t)De / 4; a.n1 = (uint32_t)n1; a.n2 = (uint32_t)n2;
  a.mod1 = (uint32_t)mod1; a.div2 = (uint32_t)div2; a.op = op;
  return MI_OK;
}

#define MI_XF_DISPATCH(XFORM, NAME, KERNEL, GRID, STREAM, ...)                                              \
  do {                                                                                                     \
    if ((XFORM) == XF_NONE) MI_LAUNCH(NAME, (KERNEL<XF_NONE>), GRID, kBlock, STREAM, __VA_ARGS__);          \
    else if ((XFORM) == XF_SOFT) MI_LAUNCH(NAME, (KERNEL<XF_SOFT>), GRID, kBlock, STREAM, __VA_ARGS__);     \
    else MI_LAUNCH(NAME, (KERNEL<XF_MASK>), GRID, kBlock, STREAM, __VA_ARGS__);                             \
  } while (0)

}  // namespace

extern "C" {

int mi_dual_table_fwd(const float *T1, const float *T2, const float *S1, const float *S2, const uint8_t *M1,
                      const uint8_t *M2, float *out, int64_t N, int32_t De, int64_t n1, int64_t n2, int64_t mod1,
                      int64_t div2, int32_t op, int32_t xform, void *stream) {
  TableArgs a;
  const int rc = fill(a, T1, T2, S1, S2, M1, M2, N, De, n1, n2, mod1, div2, op, xform);
  if (rc != MI_OK) return rc;
  if (!out) return MI_ERR_INVALID_ARG;
  if (!aligned16(out)) return MI_ERR_UNSUPPORTED;
  if (N == 0) return MI_OK;
  MI_XF_DISPATCH(xform, "dual_table_fwd", k_dual_table_fwd, grid_for((int64_t)a.N * a.C), stream, a, out);
  return launch_status();
}

int64_t mi_dual_table_bwd_workspace_elems(int64_t N, int32_t De, int64_t n1, int64_t n2, int64_t mod1, int64_t div2) {
  if (N < 0 || De <= 0 || n1 <= 0 || n2 <= 0 || mod1 <= 0 || div2 <= 0) return 0;
  const Cut cut = cut_of(N, mod1, div2);
  return (cut.nch1 > 1 ? n1 * cut.nch1 * De : 0) + (cut.nch2 > 1 ? n2 * cut.nch2 * De : 0);
}

int mi_dual_table_bwd(const float *g_out, const float *T1, const float *T2, const float *S1, const float *S2,
                      const uint8_t *M1, const uint8_t *M2, float *gT1, float *gT2, float *gS1, float *gS2, int64_t N,
                      int32_t De, int64_t n1, int64_t n2, int64_t mod1, int64_t div2, int32_t op, int32_t xform,
                      float *workspace, void *stream) {
  TableArgs a;
  const int rc = fill(a, T1, T2, S1, S2, M1, M2, N, De, n1, n2, mod1, div2, op, xform);
  if (rc != MI_OK) return rc;
  if (!gT1 || !gT2 || (N > 0 && !g_out) || (xform == XF_SOFT && (!gS1 || !gS2))) return MI_ERR_INVALID_ARG;
  const Cut cut = cut_of(N, mod1, div2);
  const bool joined = cut.nch1 > 1 || cut.nch2 > 1;
  if (joined && !workspace) return MI_ERR_INVALID_ARG;
  if (!aligned16(g_out) || !aligned16(gT1) || !aligned16(gT2) || (joined && !aligned16(workspace)) ||
      (xform == XF_SOFT && (!aligned16(gS1) || !aligned16(gS2))))
    return MI_ERR_UNSUPPORTED;
  const TableGrads gr{gT1, gT2, gS1, gS2, workspace};
  const int64_t items = (int64_t)a.n1 * cut.nch1 + (int64_t)a.n2 * cut.nch2;
  MI_XF_DISPATCH(xform, "dual_table_bwd", k_dual_table_bwd, grid_for(items * a.C), stream, a, cut, g_out, gr);
  if (joined) {
    const int64_t work = ((cut.nch1 > 1 ? (int64_t)a.n1 : 0) + (cut.nch2 > 1 ? (int64_t)a.n2 : 0)) * a.C;
    MI_XF_DISPATCH(xform, "dual_table_join", k_dual_table_join, (int)(work > kMaxGrid ? kMaxGrid : work), stream, a, cut, gr);
  }
  return launch_status();
}

}  // extern "C"
