/*
 * mi355x_recsys.h — C-ABI of libmi355x_recsys.so
 *
 * Hand-written gfx950 (MI355X / CDNA4) HIP kernels for the embedding-lookup +
 * feature-interaction hot path of chenxing1999/recsys-benchmark.
 *
 * Boundary conventions:
 *   - every pointer is a DEVICE pointer unless the parameter says "host";
 *   - the caller owns every buffer; the library allocates no persistent memory;
 *   - every entry point enqueues on `stream` (a hipStream_t passed as void*)
 *     and returns without synchronising; no hidden syncs, graph-capture safe;
 *   - an entry point enqueues its kernel(s) and NOTHING ELSE, with five documented exceptions that also enqueue one
 *     hipMemsetAsync on the same stream (a memset node when captured): mi_slot_fm_bwd zero-fills gbuf (unused slots must
 *     read as zero gradients), mi_bpr_fwd / mi_rowsq_fwd / mi_lse_diag_fwd zero the 4-byte arrival ticket at the end
 *     of their workspace, mi_tt_plan_level zeroes its p digit counters;
 *   - return value: MI_OK (0) or a negative MI_ERR_* code; no exceptions cross
 *     the ABI; calls are re-entrant;
 *   - `err` (nullable) is a device int32 word: kernels OR a bit into it when an
 *     index is out of range (the lookup then yields zeros and touches no memory
 *     out of bounds).  The reference raises IndexError from nn.Embedding on CPU
 *     (src/models/embeddings/base.py:74-75); the Python host side turns a
 *     non-zero word into IndexError when asked to check.
 *   - indices are int64 exactly as the reference passes them
 *     (src/models/deepfm.py:88); rows are fp32 row-major.
 *
 * Each declaration cites the reference interface (file:line under
 * /root/reference) whose arithmetic it replaces.
 */
#ifndef MI355X_RECSYS_H
#define MI355X_RECSYS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_API __attribute__((visibility("default")))

/* 2: round 3 — mi_sort_field_rows / mi_bpr_* / mi_rowsq_* had gained arguments under version 1 (callers built against
 * that header must rebuild); mi_gather_fm_fwd_ld, mi_sparse_adam_sorted's row stride and the later additions are new. */
/* 3: round 4 — mi_tail_bn_fwd gained `shift` and `nrep`, mi_tail_bn_bwd `dbias` and `affine` (a caller built against version 2 passes shorter structs). */
#define MI_ABI_VERSION 3

#define MI_OK 0
#define MI_ERR_INVALID_ARG (-1)  /* null pointer, negative size, bad enum */
#define MI_ERR_UNSUPPORTED (-2)  /* shape outside what the kernels cover */
#define MI_ERR_LAUNCH (-3)       /* hipLaunch / hipGetLastError failed */
#define MI_ERR_STATE (-4)        /* profiling ring misuse */

/* bits OR-ed into *err by the kernels */
#define MI_IDX_OUT_OF_RANGE 1
#define MI_IDX_OUT_OF_FIELD 2    /* mi_sort_field_rows: id inside [0,N) but outside its own field's range */

/* ---- library info -------------------------------------------------------- */
MI_API int mi_abi_version(void);
MI_API const char *mi_strerror(int code);

/* ---- a1-a4: DeepFM gather + FM 2nd order + first-order term ---------------
 * Replaces, in ONE kernel (src/models/deepfm.py:88-98):
 *   x = x + offsets                      (:88)
 *   emb = nn.Embedding(x)                (:89 -> embeddings/base.py:74-75)
 *   0.5*sum_d[(sum_f e)^2 - sum_f e^2]   (:91-92,98)
 *   EmbeddingBag(N,1,"sum")(x) + bias    (:95)
 * idx      int64[B,F] raw per-field ids (no offsets added)
 * offsets  int64[F]; NULL = the ids are row numbers already, where the float4 kernels run (D = 4, 8, 16 .. 256, W and
 *          emb_out 16-byte aligned, ldw % 4 == 0); MI_ERR_INVALID_ARG with NULL on the scalar path
 * W        fp32[N,D], w1 fp32[N] (fc.weight viewed flat), bias fp32[1] (nullable)
 * emb_out  fp32[B,F,D]   rows_out int64[B,F] (= idx+offsets; nullable)
 * yfm_out  fp32[B]
 */
MI_API int mi_gather_fm_fwd(const int64_t *idx, const int64_t *offsets,
                            const float *W, const float *w1, const float *bias,
                            float *emb_out, float *yfm_out, int64_t *rows_out,
                            int64_t B, int32_t F, int32_t D, int64_t N,
                            int32_t *err, void *stream);

/* The same lookup over tables with a ROW STRIDE (src/models/deepfm.py:47-51 declares the two tables; this is their
 * storage, not their arithmetic): row n of W starts at W + n*ldw floats (ldw >= D, a multiple of 4), the first-order
 * weight of row n is w1[n*ldw1].  (ldw, ldw1) = (D, 1) is mi_gather_fm_fwd.  (32, 32) with w1 = W + 16 reads ONE packed
 * table fp32[N,32] = {16 embedding floats, first-order weight, padding}: a lookup then touches one 128-byte line
 * instead of two unrelated 64-byte sectors (DeepFM.pack_tables() on the Python side; both parameters become views of
 * the packed buffer and state_dict() still emits the reference's two tensors). */
MI_API int mi_gather_fm_fwd_ld(const int64_t *idx, const int64_t *offsets,
                               const float *W, int64_t ldw, const float *w1, int64_t ldw1, const float *bias,
                               float *emb_out, float *yfm_out, int64_t *rows_out,
                               int64_t B, int32_t F, int32_t D, int64_t N,
                               int32_t *err, void *stream);

/* The same forward, additionally storing sum_out[b, :] = sum_f emb[b, f, :] (fp32[B, D], nullable) — the one quantity of the
 * FM backward (src/models/deepfm.py:91-92 through autograd: dE_bf = g_b (S_b - e_bf)) that a kernel seeing only SOME fields
 * of a sample cannot re-derive; mi_tail_dgrad_gemm_fm (below) consumes it. */
MI_API int mi_gather_fm_fwd_sum(const int64_t *idx, const int64_t *offsets,
                                const float *W, int64_t ldw, const float *w1, int64_t ldw1, const float *bias,
                                float *emb_out, float *yfm_out, int64_t *rows_out, float *sum_out,
                                int64_t B, int32_t F, int32_t D, int64_t N,
                                int32_t *err, void *stream);

/* Touch the table rows the NEXT batch's lookup will read (idx int64[B,F] raw ids of that batch, other arguments as
 * mi_gather_fm_fwd_ld): pulls their 128-byte lines into the 256 MiB Infinity Cache.  Meant for a side stream under an
 * MFMA-bound kernel of the current step; writes nothing.  (No reference counterpart: src/trainer/deepfm.py:40-60 gets the
 * next batch from its DataLoader while the step runs; this is what the device does with that lead.) */
MI_API int mi_prefetch_rows(const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw, const float *w1,
                            int64_t ldw1, int64_t B, int32_t F, int64_t N, void *stream);
/* The same job as a host struct, for a launch that carries it in extra workgroups (mi_gemm_f32_multi_ride). */
typedef struct mi_prefetch_rows_job {
  const int64_t *idx;       /* device int64[B, F]: the NEXT batch's raw ids */
  const int64_t *offsets;   /* device int64[F], nullable */
  const float *W;           /* the embedding table (row pitch ldw floats) */
  const float *w1;          /* the first-order table (row pitch ldw1), nullable */
  int64_t ldw, ldw1, B, N;
  int32_t F;
} mi_prefetch_rows_job;

/* Backward of the above, row-sparse form (the MI355X-native default):
 *   gvals[b,f,:] = g_emb[b,f,:] + g_y[b] * (S_b - emb[b,f,:]),  S_b = sum_f emb
 *   g1vals[b,f]  = g_y[b]
 * i.e. one gradient row per lookup, written with plain coalesced stores; the
 * caller pairs them with rows_out from the forward as an (uncoalesced) COO
 * gradient of W / w1.  Autograd equivalent: embedding_dense_backward +
 * _embedding_bag_dense_backward of src/models/deepfm.py:89,95 before the
 * duplicate-row sum.  g_emb is nullable (no deep branch).
  * gbias (nullable, both backward forms and mi_slot_fm_bwd): receives sum_b g_y[b], the gradient of the
 * scalar bias (src/models/deepfm.py:51,95), added up in a fixed order by workgroup 0 of the same launch.
 */
MI_API int mi_gather_fm_bwd_rows(const float *emb, const float *g_y,
                                 const float *g_emb, float *gvals, float *g1vals,
                                 float *gbias, int64_t B, int32_t F, int32_t D, void *stream);

/* Backward, dense form (the reference's weight.grad semantics): scatter-adds
 * the same rows into caller-zeroed gW fp32[N,D] / gw1 fp32[N] with float
 * atomics (sum order differs from the CPU index_add: fp32 tolerance).
 * rows int64[B,F] = idx+offsets as produced by the forward.
 */
MI_API int mi_gather_fm_bwd_dense(const int64_t *rows, const float *emb,
                                  const float *g_y, const float *g_emb,
                                  float *gW, float *gw1, float *gbias, int64_t B, int32_t F,
                                  int32_t D, int64_t N, void *stream);

/* ---- the same three kernels with a KEPT WIDTH per looked-up row (DeepFM on OptEmbed) ----
 * src/models/embeddings/deepfm_opt_embed.py:186-200 (a search candidate: emb * mask_d over the whole table, then the
 * lookup) and :693-706 (RetrainOptEmbed: _weight * _mask every step) without the masked copy of the table:
 *   row       = idx[b,f] + offsets[f]
 *   kept(b,f) = min(keep ? keep[row] : D, fwidth ? fwidth[f] : D)
 *   emb[b,f,d] = d < kept(b,f) ? W[row,d] : +0;  y_fm over the masked emb; the first-order term is NOT masked
 * keep    uint8[N], nullable: the row's kept width, 0 = a dead row (the row mask times the per-feature width)
 * fwidth  int32[F], nullable: one width per field (a search candidate of mode_threshold_d = "field")
 * A value above D acts as D.  D <= MI_GATHER_FM_MASKED_MAX_D (a width is one byte), else MI_ERR_UNSUPPORTED.
 * Forward: the other arguments as mi_gather_fm_fwd_ld (out-of-range rows flagged in *err and read as zeros).
 * Backward, row form: gvals[i,d] = g_emb[i,d] + g_y[b] (S[b,d] - emb[i,d]) for d < kept(i) and exactly 0 past it;
 *   g1vals[i] = g_y[b]; rows int64[B,F] = the forward's rows_out (needed with keep).
 * Backward, dense form: the same values scatter-added into the caller-zeroed gW / gw1; an element at or past its row's
 *   kept width issues no atomic (gW stays the caller's zero there).
 */
#define MI_GATHER_FM_MASKED_MAX_D 255
MI_API int mi_gather_fm_masked_fwd(const int64_t *idx, const int64_t *offsets,
                                   const float *W, int64_t ldw, const float *w1, int64_t ldw1, const float *bias,
                                   const uint8_t *keep, const int32_t *fwidth,
                                   float *emb_out, float *yfm_out, int64_t *rows_out,
                                   int64_t B, int32_t F, int32_t D, int64_t N,
                                   int32_t *err, void *stream);
MI_API int mi_gather_fm_masked_bwd_rows(const int64_t *rows, const uint8_t *keep, const int32_t *fwidth,
                                        const float *emb, const float *g_y, const float *g_emb,
                                        float *gvals, float *g1vals, float *gbias,
                                        int64_t B, int32_t F, int32_t D, int64_t N, void *stream);
MI_API int mi_gather_fm_masked_bwd_dense(const int64_t *rows, const uint8_t *keep, const int32_t *fwidth,
                                         const float *emb, const float *g_y, const float *g_emb,
                                         float *gW, float *gw1, float *gbias,
                                         int64_t B, int32_t F, int32_t D, int64_t N, void *stream);

/* ---- the same launch with PEP's element transforms (DeepFM on PepEmbeeding / RetrainPepEmbedding) ----
 * src/models/embeddings/pep_embedding.py:82-92 (soft-threshold the whole table, then the lookup) and :211-221
 * (emb.weight * mask every step) without the transformed copy of the table:
 *   soft:     emb[b,f,d] = sign(w) relu(|w| - sigmoid(s)),  w = W[row,d],  s = S[row*srs + d*scs]
 *             (srs, scs) as in mi_xform_gather_*: (0,0) global [1], (0,1) dimension [D], (1,0) feature [N,1],
 *             (D,1) feature_dim [N,D]; anything else is MI_ERR_INVALID_ARG.  The same device functions as
 *             mi_xform_gather_fwd: emb has that lookup's bits.
 *   elemmask: emb[b,f,d] = M[row,d] ? W[row,d] : +0,  M uint8[N,D] (a bool mask read as bytes, not packed into bits)
 * y_fm over the transformed emb; the first-order term and the bias are NOT transformed.  The other arguments as
 * mi_gather_fm_fwd_ld (out-of-range rows flagged in *err and read as zeros).
 * Backward, row form only (dense gradients are scattered from the row values, mi_scatter_axpy_rows, or coalesced in a fixed
 * order, mi_coalesce_rows_sorted): one launch over the saved emb, W is not read again.  rows int64[B,F] = the forward's
 * rows_out; dE[i,d] = g_emb[i,d] + g_y[b] (S[b,d] - emb[i,d]);  g1vals[i] = g_y[b];  gbias nullable.
 *   soft:     gvals[i,d] = dE [emb != 0];  svals = -dE sign(emb) [emb != 0] sig(s) (1 - sig(s)), laid out by the threshold:
 *             feature_dim fp32[B*F, D]; feature fp32[B*F] (summed over d); dimension fp32[D] / global fp32[1]: the final
 *             gradient, summed over the grid in a fixed order by the last workgroup to arrive — no float atomics.  These two
 *             take `workspace` (mi_gather_fm_soft_bwd_workspace_elems floats, 0 for the row layouts), whose LAST word is a
 *             ticket: armed != 0 says it is zero already (every launch leaves it zero), armed = 0 zeroes it first.
 *   elemmask: gvals[i,d] = M[row,d] ? dE : 0 (the mask from M: a kept element may hold exactly 0).
 * D <= 256 in the backward, else MI_ERR_UNSUPPORTED.
 */
MI_API int mi_gather_fm_soft_fwd(const int64_t *idx, const int64_t *offsets,
                                 const float *W, int64_t ldw, const float *w1, int64_t ldw1, const float *bias,
                                 const float *S, int64_t srs, int64_t scs,
                                 float *emb_out, float *yfm_out, int64_t *rows_out,
                                 int64_t B, int32_t F, int32_t D, int64_t N,
                                 int32_t *err, void *stream);
MI_API int mi_gather_fm_elemmask_fwd(const int64_t *idx, const int64_t *offsets,
                                     const float *W, int64_t ldw, const float *w1, int64_t ldw1, const float *bias,
                                     const uint8_t *M,
                                     float *emb_out, float *yfm_out, int64_t *rows_out,
                                     int64_t B, int32_t F, int32_t D, int64_t N,
                                     int32_t *err, void *stream);
MI_API int64_t mi_gather_fm_soft_bwd_workspace_elems(int64_t B, int32_t D, int64_t srs);
MI_API int mi_gather_fm_soft_bwd_rows(const int64_t *rows, const float *S, int64_t srs, int64_t scs,
                                      const float *emb, const float *g_y, const float *g_emb,
                                      float *gvals, float *svals, float *g1vals, float *gbias, float *workspace,
                                      int32_t armed, int64_t B, int32_t F, int32_t D, int64_t N, void *stream);
MI_API int mi_gather_fm_elemmask_bwd_rows(const int64_t *rows, const uint8_t *M,
                                          const float *emb, const float *g_y, const float *g_emb,
                                          float *gvals, float *g1vals, float *gbias,
                                          int64_t B, int32_t F, int32_t D, int64_t N, void *stream);

/* ---- the same launch over the two-table compositional embeddings (DeepFM on QR hashing, CERP, CERP retrain) ----
 * src/models/embeddings/qr_embedding.py:84-109, cerp_embedding.py:160-175 and :329-367 under src/models/deepfm.py:88-98.
 * mi_gather_fm_dual_fwd: for idx int64[B,F], offsets int64[F] (nullable: the ids are row numbers),
 *     row        = idx[b,f] + offsets[f]
 *     emb[b,f,:] = T1'[row % mod1] (op) T2'[row / div2]       T1 fp32[n1,De], T2 fp32[n2,De]
 *     y_fm[b]    = 0.5 (|sum_f e|^2 - sum_f |e|^2) + sum_f w1[row * ldw1] + bias[0]      (bias nullable)
 *   op 0 mult / 1 add; T' = T (xform 0), sign(T) relu(|T| - sigmoid(S)) (xform 1, S1 / S2 fp32 shaped like the tables) or
 *   M ? T : +0 (xform 2, M1 / M2 uint8 shaped like the tables).  Served: (mult, none), (add, none), (add, soft),
 *   (add, mask); every other pair (op 2 cat among them) is MI_ERR_UNSUPPORTED and the caller keeps mi_dual_gather_fwd +
 *   mi_fm_fwd.  The element transforms are mi_dual_gather_fwd's device functions: emb has that lookup's bits, signed
 *   zeros included.  rows_out int64[B,F] (nullable) = row; rows_bwd int64[B,F] (nullable) = row where the lookup was served, -1
 *   where it was flagged: the ids for mi_dual_gather_bwd_fields / _bwd_rows, which check table bounds only.  A row outside [0, N) (N = rows of w1), or one the tables do not
 *   cover (row % mod1 >= n1, row / div2 >= n2), reads as zeros everywhere and ORs MI_IDX_OUT_OF_RANGE into *err.
 *   De <= MI_GATHER_FM_DUAL_MAX_D; De = 4 * 2^k <= 256 with 16-byte aligned operands runs float4 kernels, any other De
 *   the scalar ones.
 * mi_gather_fm_dual_bwd_rows: the row-form backward from the saved emb and rows (= rows_out), no float atomics.  With
 *   dE[i,:] = g_emb[i,:] + g_y[b] (S_b - emb[i,:]), i = b F + f, S_b = sum_f emb[b,f,:] (g_emb nullable):
 *     keys1[i] = row % mod1,  keys2[i] = row / div2   (int64; 0 for a row the forward flagged, whose value rows are zeros)
 *     add : c1[i,:] = dE [M1[keys1,:]],  c2[i,:] = dE [M2[keys2,:]]  — the masks only when M1 / M2 are given (values masked
 *           per lookup: the COO gradients of the retrain table); without them c1 == c2 and c2 may be NULL
 *     mult: c1[i,:] = dE * T2[keys2,:],  c2[i,:] = dE * T1[keys1,:]   (c2 required)
 *     g1vals[i] = g_y[b];  gbias[0] = sum_b g_y[b] in a fixed order (nullable)
 *   field_off int64[F] (nullable; the forward's offsets), for a caller that sums in the order of mi_sort_field_rows: a row
 *   outside [field_off[f], field_off[f+1]) (the last field ends at N) counts as flagged too — what that sort drops —, and a
 *   flagged lookup of field f gets keys2 = the largest table-2 row of field f (value rows still zero), so that keys2 taken
 *   through the sort's permutation is monotone.
 * mi_gather_fm_dual_finish: the transform's derivative, once per table element AFTER the sums (A1 fp32[n1,De], A2 fp32[n2,De],
 *   in place; either may be NULL and is then skipped):
 *     mask: A = M ? A : 0
 *     soft: kept = |T| - sigmoid(S) > 0;  gS = -sign(T) sig(S) (1 - sig(S)) kept A;  A = kept A
 *   kept comes from the table and its threshold, never from looked-up values: a kept element that holds exactly 0 keeps its
 *   gradient, a pruned or masked one gets exactly 0; sig (1 - sig) is formed from the fp32 sigmoid (exactly 0 at s = +-150).
 *   xform 0 launches nothing.
 */
#define MI_GATHER_FM_DUAL_MAX_D 1024
MI_API int mi_gather_fm_dual_fwd(const int64_t *idx, const int64_t *offsets,
                                 const float *T1, const float *T2, const float *S1, const float *S2,
                                 const uint8_t *M1, const uint8_t *M2,
                                 const float *w1, int64_t ldw1, const float *bias,
                                 float *emb_out, float *yfm_out, int64_t *rows_out, int64_t *rows_bwd,
                                 int64_t B, int32_t F, int32_t De, int64_t N,
                                 int64_t n1, int64_t n2, int64_t mod1, int64_t div2, int32_t op, int32_t xform,
                                 int32_t *err, void *stream);
MI_API int mi_gather_fm_dual_bwd_rows(const int64_t *rows, const int64_t *field_off, const float *emb, const float *g_y, const float *g_emb,
                                      const float *T1, const float *T2, const uint8_t *M1, const uint8_t *M2,
                                      float *c1, float *c2, int64_t *keys1, int64_t *keys2,
                                      float *g1vals, float *gbias,
                                      int64_t B, int32_t F, int32_t De, int64_t N,
                                      int64_t n1, int64_t n2, int64_t mod1, int64_t div2, int32_t op, void *stream);
MI_API int mi_gather_fm_dual_finish(float *A1, float *A2, const float *T1, const float *T2,
                                    const float *S1, const float *S2, const uint8_t *M1, const uint8_t *M2,
                                    float *gS1, float *gS2, int64_t n1, int64_t n2, int32_t De, int32_t xform,
                                    void *stream);

/* ---- CERP's whole-table prune loss (DeepFM's search step) ----
 * src/models/embeddings/cerp_embedding.py get_prune_loss: -tanh((soft(P,Sp) + soft(Q,Sq)) K).norm(2)**2 over four
 * fp32 tables of n = bucket * D elements each (contiguous, equal shapes).
 * mi_cerp_prune_loss_fwd: out[0] = -sum tanh(K (soft(P,Sp) + soft(Q,Sq)))^2, one launch, one read of each table, no
 *   [bucket, D] temporary; the workgroups' partial sums are added in a fixed order by the last workgroup to take a ticket
 *   (the same bits on every run).  workspace: mi_cerp_prune_loss_workspace_elems(n) floats whose LAST word is the ticket;
 *   armed != 0 says it is zero already (every launch leaves it zero), armed = 0 zeroes it first.
 * mi_cerp_prune_loss_bwd: with x = soft(P,Sp) + soft(Q,Sq), t = tanh(K x), g = -2 K t (1 - t^2) grad_out[0]:
 *     gP = kept_p g,  gSp = -sign(P) sig(Sp) (1 - sig(Sp)) kept_p g,  kept_p = |P| - sig(Sp) > 0   (gQ, gSq alike)
 *   every element of the four outputs written once with a plain store: no zero fill, no atomics.
 */
MI_API int64_t mi_cerp_prune_loss_workspace_elems(int64_t n);
MI_API int mi_cerp_prune_loss_fwd(const float *P, const float *Sp, const float *Q, const float *Sq, int64_t n,
                                  float k_tanh, float *workspace, int32_t armed, float *out, void *stream);
MI_API int mi_cerp_prune_loss_bwd(const float *P, const float *Sp, const float *Q, const float *Sq, int64_t n,
                                  float k_tanh, const float *grad_out, float *gP, float *gSp, float *gQ, float *gSq,
                                  void *stream);

/* ---- a2: plain row gather (IEmbedding.forward on a vanilla table) ----------
 * src/models/embeddings/base.py:74-75 (nn.Embedding on int64[n] ids, already
 * offset).  out fp32[n,D].
 */
MI_API int mi_gather_rows_fwd(const int64_t *idx, const float *W, float *out,
                              int64_t n, int32_t D, int64_t N, int32_t *err,
                              void *stream);

/* dense backward of the row gather: gW[idx[i],:] += g[i,:] (float atomics). */
MI_API int mi_scatter_add_rows(const int64_t *idx, const float *g, float *gW,
                               int64_t n, int32_t D, int64_t N, void *stream);

/* ---- a3/a4 over an already gathered emb (DeepFM on a compressed table) -------
 * y_fm[b] = 0.5*sum_d[(sum_f e)^2 - sum_f e^2] + sum_f w1[rows[b,f]] + bias
 * (src/models/deepfm.py:91-98).  Its backward is mi_gather_fm_bwd_rows (gradient
 * w.r.t. emb) plus mi_scatter_add_rows with D=1 (dense w1 gradient).
 */
MI_API int mi_fm_fwd(const float *emb, const int64_t *rows, const float *w1,
                     const float *bias, float *yfm, int64_t B, int32_t F, int32_t D,
                     int64_t N, int32_t *err, void *stream);

/* ---- a6-a8: two-table compositional lookups, index math fused ---------------
 *   i1 = idx % mod1  -> row of T1 fp32[n1,De]     i2 = idx / div2 -> row of T2 fp32[n2,De]
 *   out = T1'[i1] (op) T2'[i2],  op: 0 mult, 1 add, 2 cat
 *   xform 0: T' = T
 *         1: T' = sign(T)*relu(|T| - sigmoid(S))   (S1,S2 fp32 threshold logits)
 *         2: T' = T * M                            (M1,M2 bool masks, 1 byte each)
 * QR hashing   (src/models/embeddings/qr_embedding.py:95-109): T1=emb1 (divider rows),
 *              T2=emb2, mod1 = div2 = divider, xform 0.  For op=cat the output is
 *              [n/F, 2F, De] (torch.cat(dim=1) on a [B,F] input), F=1 for 1-D input.
 * CERP         (src/models/embeddings/cerp_embedding.py:142-175): T1=P, T2=Q,
 *              mod1 = bucket_size, div2 = q_entity_per_row, op add, xform 1.
 * CERP retrain (cerp_embedding.py:329-367): xform 2.
 * idx int64[n]; negative ids and rows beyond n1/n2 are flagged in *err and yield zeros.
 */
MI_API int mi_dual_gather_fwd(const int64_t *idx, const float *T1, const float *T2,
                              const float *S1, const float *S2, const uint8_t *M1,
                              const uint8_t *M2, float *out, int64_t n, int32_t F,
                              int32_t De, int64_t n1, int64_t n2, int64_t mod1,
                              int64_t div2, int32_t op, int32_t xform, int32_t *err,
                              void *stream);
/* ... with the model's `x + offsets` (src/models/dcn.py:204 / deepfm.py:86: per-field ids [B, F] + cumulative field
 * offsets [F]) done inside the lookup: idx holds the raw ids, id i gets offsets[i % F] added, and the sums — what the
 * reference hands to its embedding module, what the backward and the sparse optimizer's field sort read — are written to
 * rows_out int64[n].  offsets == NULL: mi_dual_gather_fwd (rows_out untouched).  De % 4 == 0 with 16-byte aligned
 * tables only (MI_ERR_UNSUPPORTED otherwise: add the offsets first). */
MI_API int mi_dual_gather_fwd_off(const int64_t *idx, const int64_t *offsets, int64_t *rows_out, const float *T1,
                                  const float *T2, const float *S1, const float *S2, const uint8_t *M1,
                                  const uint8_t *M2, float *out, int64_t n, int32_t F, int32_t De, int64_t n1,
                                  int64_t n2, int64_t mod1, int64_t div2, int32_t op, int32_t xform, int32_t *err,
                                  void *stream);

/* The same family in TABLE form: out[i] = T1'[i % mod1] (op) T2'[i / div2] for i = 0 .. N-1 — get_weight() of
 * QRHashingEmbedding / CerpEmbedding / RetrainCerpEmbedding (the module's forward over arange(N)), which a LightGCN or
 * NeuMF asks for on every step.  No index tensor and no error word: every row is in range by construction (tables that
 * cannot cover N rows — n1 < min(N, mod1) or n2 < ceil(N / div2) — are MI_ERR_INVALID_ARG).  Same arithmetic per element as
 * mi_dual_gather_fwd: bit-identical to it over arange(N).  out is [N, De] ([N, 2 De] for cat).
 * mi_dual_table_bwd: owner computes.  Row r of T1 sums rows r, r + mod1, ... of g_out, row r of T2 rows r div2 ..
 * (r + 1) div2 - 1 (times the other table's transformed row for mult, its own half for cat), in ascending i, by one
 * thread per float4; the transform's derivative is applied once per table element after the sum; every element of
 * gT1 / gT2 (and gS1 / gS2 for xform 1) is WRITTEN exactly once (rows without a contributor get zeros): no atomics, no
 * zero fill, the same bits on every run.  Rows with more than 16 contributors are cut into chunks of 8 contributors
 * (constants: the order of additions depends on the shapes only), the chunk sums go to `workspace`
 * (mi_dual_table_bwd_workspace_elems floats, may be 0 / NULL when no row is cut; no state between launches) and a second
 * launch joins them in a fixed order.  De % 4 == 0 with 16-byte aligned operands (masks 4-byte aligned), De <= 1024 and
 * fewer than 2^31 output elements; anything else is MI_ERR_UNSUPPORTED (the caller keeps the lookup over arange(N)). */
MI_API int mi_dual_table_fwd(const float *T1, const float *T2, const float *S1, const float *S2, const uint8_t *M1,
                             const uint8_t *M2, float *out, int64_t N, int32_t De, int64_t n1, int64_t n2,
                             int64_t mod1, int64_t div2, int32_t op, int32_t xform, void *stream);
MI_API int64_t mi_dual_table_bwd_workspace_elems(int64_t N, int32_t De, int64_t n1, int64_t n2, int64_t mod1,
                                                 int64_t div2);
MI_API int mi_dual_table_bwd(const float *g_out, const float *T1, const float *T2, const float *S1, const float *S2,
                             const uint8_t *M1, const uint8_t *M2, float *gT1, float *gT2, float *gS1, float *gS2,
                             int64_t N, int32_t De, int64_t n1, int64_t n2, int64_t mod1, int64_t div2, int32_t op,
                             int32_t xform, float *workspace, void *stream);

/* Dense gradients of the above into caller-zeroed gT1/gT2 (and gS1/gS2 for xform 1),
 * float atomics; tables of <= 4096 elements are pre-summed per workgroup in LDS. */
MI_API int mi_dual_gather_bwd(const int64_t *idx, const float *g_out, const float *T1,
                              const float *T2, const float *S1, const float *S2,
                              const uint8_t *M1, const uint8_t *M2, float *gT1, float *gT2,
                              float *gS1, float *gS2, int64_t n, int32_t F, int32_t De,
                              int64_t n1, int64_t n2, int64_t mod1, int64_t div2,
                              int32_t op, int32_t xform, void *stream);
/* Row form of table 2's gradient (round 4; plain tables only — QRHashingEmbedding, src/models/embeddings/qr_embedding.py:95-109
 * through autograd): g2vals fp32[n, De] receives lookup i's contribution to row rows2[i] = idx[i] / div2 of table 2 (rows2
 * int64[n]; an id out of range gets row 0 and a ZERO value row) — an uncoalesced COO gradient like
 * nn.Embedding(sparse=True)'s, written with plain coalesced stores: no float atomics into scattered rows, no [n2, De]
 * zero-fill.  gT1 (dense) is added to (caller-zeroed) as above, EXCEPT in the joined form below.
 * workspace (nullable): mi_dual_gather_bwd_rows_workspace_elems(De, n1) floats (0: this shape has no use for one) whose first
 * word is ZERO on entry (the kernel leaves it zero): table 1's per-workgroup sums are then joined by the last workgroup to
 * arrive, in a fixed order, instead of by same-address float atomics — and gT1 is WRITTEN, not added to.  Which of the
 * three forms a launch takes is the library's decision alone: ask mi_dual_gather_bwd_rows_form with the operands the launch
 * will get (it reads addresses and shapes and dereferences nothing).
 * ONLY MI_DUAL_ROWS_FORM_WORKSPACE lets the caller skip zeroing gT1; the other two forms add into it.
 * mi_dual_gather_bwd_rows_overwrites(De, n1) != 0: the shape reaches MI_DUAL_ROWS_FORM_WORKSPACE when a workspace is passed
 * and the operands are aligned — a shape rule only, not an answer for a launch. */
#define MI_DUAL_ROWS_FORM_ELEMENT 0   /* element-per-thread kernel; adds into gT1 */
#define MI_DUAL_ROWS_FORM_ATOMIC 1    /* float4 kernel, workgroup sums joined by float atomics; adds into gT1 */
#define MI_DUAL_ROWS_FORM_WORKSPACE 2 /* float4 kernel, workgroup sums joined through the workspace; writes gT1 */
MI_API int32_t mi_dual_gather_bwd_rows_form(const float *g_out, const float *T1, const float *T2, const float *g2vals,
                                            const float *workspace, int32_t De, int64_t n1);
MI_API int32_t mi_dual_gather_bwd_rows_overwrites(int32_t De, int64_t n1);
MI_API int64_t mi_dual_gather_bwd_rows_workspace_elems(int32_t De, int64_t n1);
MI_API int mi_dual_gather_bwd_rows(const int64_t *idx, const float *g_out, const float *T1, const float *T2, float *gT1,
                                   float *g2vals, int64_t *rows2, int64_t n, int32_t F, int32_t De, int64_t n1,
                                   int64_t n2, int64_t mod1, int64_t div2, int32_t op, float *workspace, void *stream);
/* The same, told which FIELDS of idx[B, F] have a handful of values (n = B * F; xform 0 only, else the hint is ignored):
 * small_fields int32[n_small] = their column indices, is_small uint8[F] the same as flags, field_row0 int64[F] = the first
 * row of table 2 a field's ids reach (all device arrays).  A small field's B lookups land on <= 16 rows of table 2 from
 * field_row0[f]; their gradient is summed per field in registers by extra workgroups and added once per (row, column) and
 * workgroup instead of B same-address atomics (an id outside that span is still added, atomically).  n_small = 0: plain. */
MI_API int mi_dual_gather_bwd_fields(const int64_t *idx, const float *g_out, const float *T1, const float *T2,
                                     const float *S1, const float *S2, const uint8_t *M1, const uint8_t *M2, float *gT1,
                                     float *gT2, float *gS1, float *gS2, int64_t n, int32_t F, int32_t De, int64_t n1,
                                     int64_t n2, int64_t mod1, int64_t div2, int32_t op, int32_t xform,
                                     const int32_t *small_fields, int32_t n_small, const int64_t *field_row0,
                                     const uint8_t *is_small, void *stream);


/* ---- §8f rank 4 (first flavour): single-table gather with a per-element transform -------------
 * PEP (src/models/embeddings/pep_embedding.py:82-92): out = sign(w) relu(|w| - sigmoid(s)), w = W[idx],
 *   s = S[row*srs + d*scs] — strides (0,0) global, (0,1) dimension, (1,0) feature, (D,1) feature_dim.
 * RetrainPep (:211-221): out = W[idx] * M (bool mask, 1 byte).  xform as in mi_dual_gather_fwd.
 * Backward: dense gW (and gS, s_numel elements) caller-zeroed, float atomics; small S pre-summed in LDS.
 */
MI_API int mi_xform_gather_fwd(const int64_t *idx, const float *W, const float *S,
                               const uint8_t *M, int64_t srs, int64_t scs, float *out,
                               int64_t n, int32_t D, int64_t N, int32_t xform, int32_t *err,
                               void *stream);
MI_API int mi_xform_gather_bwd(const int64_t *idx, const float *g_out, const float *W,
                               const float *S, const uint8_t *M, int64_t srs, int64_t scs,
                               float *gW, float *gS, int64_t s_numel, int64_t n, int32_t D,
                               int64_t N, int32_t xform, void *stream);

/* PepEmbeeding.get_num_params() (pep_embedding.py:127-130): *count (a device int64, overwritten) = the number of
 * elements of W fp32[N,D] with |w| - sigmoid(s) > 0, s = S[row*srs + d*scs] as above — where the soft-thresholded table
 * is non-zero.  One read of W and S, integer adds only, no [N,D] temporary. */
MI_API int mi_soft_count_kept(const float *W, const float *S, int64_t srs, int64_t scs, int64_t N, int32_t D,
                              int64_t *count, void *stream);

/* Quantised tables, inference only (src/models/embeddings/ptq_emb.py:24-25,85-91):
 * qtype 1: W is fp16[N,D], out = fp32(W[idx]); 2 / 3: W is int8 / int16 codes, out = (code - bias[0]) * scale[0]
 * with bias a device int8 / int16 word and scale a device fp32 word.
 */
MI_API int mi_gather_rows_quant(const int64_t *idx, const void *W, int32_t qtype,
                                const float *scale, const void *bias, float *out, int64_t n,
                                int32_t D, int64_t N, int32_t *err, void *stream);

/* ---- §8f rank 4 (third flavour): quantisation-aware-training lookup -----------------------------
 * QAT_EmbInt.forward = row gather + StotasticRounding (src/models/embeddings/qat_emb.py:16-45,117-119):
 *   q = clamp(W[idx]/scale, q_min, q_max); out = (floor(q) + [u > floor(q) + 1 - q]) * scale,
 *   q_min = -2^(n_bits-1), q_max = 2^(n_bits-1) - 1, scale a device scalar.
 * u = prob[element] when prob != NULL (the reference's torch.rand_like draw, for parity tests), else the
 * library's counter generator on (seed[0] + salt, element index) — the backward re-derives the same rounding.
 * idx == NULL: rows 0..n-1 of W (rounding an already reduced bag).  Backward (:49-84): dW[idx] += g
 * (float atomics into a caller-zeroed dense gradient; plain store when idx == NULL),
 * dscale[0] += sum g * m, m = q_max | q_min at the clamps, else (rounded - W/scale).  dW / dscale nullable. */
MI_API int mi_qat_gather_fwd(const int64_t *idx, const float *W, const float *scale, int32_t n_bits,
                             const float *prob, const int64_t *seed, int64_t salt, float *out,
                             int64_t n, int32_t D, int64_t N, int32_t *err, void *stream);
MI_API int mi_qat_gather_bwd(const int64_t *idx, const float *W, const float *scale, int32_t n_bits,
                             const float *prob, const int64_t *seed, int64_t salt, const float *g,
                             float *dW, float *dscale, int64_t n, int32_t D, int64_t N, void *stream);

/* ---- DeepFM on the quantised tables: lookup + dequantisation / rounding + FM + first order, ONE launch ----
 * row = idx[b,f] + offsets[f] (offsets nullable); emb fp32[B,F,D]; yfm[b] = the FM second-order term of emb[b] + the
 * first-order bag sum_f w1[row * ldw1] + bias[0] (bias nullable).  A row outside [0, N) reads as a zero row and ORs
 * MI_IDX_OUT_OF_RANGE into *err.  D = 4 * 2^k <= 256 with the table's base aligned to four codes and emb to 16 bytes runs
 * the kernels that load a lane's four codes as one word, anything else the scalar ones: the same bits.
 * mi_gather_fm_quant_fwd (inference; PTQEmb_Int / PTQEmb_Fp16): Wq, qtype, scale and zero as W, qtype, scale and bias of
 *   mi_gather_rows_quant, and emb has that entry point's bits over idx + offsets.
 * mi_gather_fm_qat_fwd (QAT_EmbInt, training and evaluation): W, scale, n_bits, prob, seed and salt as mi_qat_gather_fwd;
 *   the draw of emb element (b F + f) D + d is prob[that index] or the generator's at that index, so emb has the bits of
 *   mi_qat_gather_fwd over idx + offsets.  rows_out int64[B,F], nullable: idx + offsets.
 * mi_gather_fm_qat_bwd_rows: the row-form backward from the saved emb, no float atomics.  For lookup i = b F + f:
 *   gvals[i,:] = g_emb[i,:] + g_y[b] (S_b - emb[i,:]), S_b = sum_f emb[b,f,:] (straight through the rounding; g_emb nullable),
 *   g1vals[i] = g_y[b], gbias[0] = sum_b g_y[b] (nullable).
 *   W and dscale both given (else both NULL: the table is not read): dscale[0] = sum gvals * m over the lookups inside [0, N),
 *   m = q_max where W[row]/scale >= q_max, q_min where <= q_min, else rintf(emb / scale) - W[row]/scale (the code the forward
 *   rounded to, recovered from emb); rows = rows_out.  The sum is joined over the grid in a fixed order by the last workgroup
 *   to arrive and is complete when the launch ends.  It takes `workspace` (mi_gather_fm_qat_bwd_workspace_elems floats), whose
 *   LAST word is a ticket: armed != 0 says it is zero already (every launch leaves it zero), armed = 0 zeroes it first.
 *   D <= MI_GATHER_FM_QAT_BWD_MAX_D, and n_bits <= 21 when dscale is wanted (the code is recovered from emb exactly up to
 *   there), else MI_ERR_UNSUPPORTED.
 */
#define MI_GATHER_FM_QAT_BWD_MAX_D 256
MI_API int mi_gather_fm_quant_fwd(const int64_t *idx, const int64_t *offsets, const void *Wq, int32_t qtype,
                                  const float *scale, const void *zero, const float *w1, int64_t ldw1,
                                  const float *bias, float *emb_out, float *yfm_out,
                                  int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err, void *stream);
MI_API int mi_gather_fm_qat_fwd(const int64_t *idx, const int64_t *offsets, const float *W, const float *scale,
                                int32_t n_bits, const float *prob, const int64_t *seed, int64_t salt,
                                const float *w1, int64_t ldw1, const float *bias, float *emb_out, float *yfm_out,
                                int64_t *rows_out, int64_t B, int32_t F, int32_t D, int64_t N,
                                int32_t *err, void *stream);
MI_API int64_t mi_gather_fm_qat_bwd_workspace_elems(int64_t B);
MI_API int mi_gather_fm_qat_bwd_rows(const int64_t *rows, const float *W, const float *scale, int32_t n_bits,
                                     const float *emb, const float *g_y, const float *g_emb,
                                     float *gvals, float *g1vals, float *gbias, float *dscale, float *workspace,
                                     int32_t armed, int64_t B, int32_t F, int32_t D, int64_t N, void *stream);

/* ---- PTQEmb_Int(n_bits=4) with two codes per byte, and the device-side quantiser of the PTQ integer tables ----
 * The reference keeps one 4-bit code per int8 byte (src/models/embeddings/ptq_emb.py:61-83).  The packed table is
 * uint8 [N, D/2] (D even): element d of row r in byte r*D/2 + d/2, the low nibble for even d, the high nibble for odd d,
 * each nibble a two's-complement code in [-8, 7]; scale a device fp32 word, zero a device INT8 word (the zero point of
 * ptq_emb.py:73 can lie outside the nibble range and is never packed).
 * MI_QTYPE_INT4_PACKED as the qtype of mi_gather_fm_quant_fwd: Wq is such a table, D the LOGICAL width; emb has the bits of
 *   qtype 2 over the unpacked codes.  D = 4 * 2^k <= 256 with Wq 2-byte and emb 16-byte aligned runs the kernels that load a
 *   lane's four codes as one 16-bit word, anything else (D % 4 == 2, an odd base) the scalar ones: the same bits.
 * mi_gather_rows_int4 (ptq_emb.py:85-91): out[i,:] = (code(W[row_i,:]) - zero[0]) * scale[0], row_i = idx[i] (idx NULL: i, the
 *   table form of get_weight()) + offsets[i % F] (offsets int64[F], nullable); rows_out int64[n], nullable (needs idx): row_i.
 *   The bits of mi_gather_rows_quant (qtype 2) over the unpacked codes; a row outside [0, N) reads as zeros and ORs
 *   MI_IDX_OUT_OF_RANGE into *err.
 * mi_ptq_quantise (ptq_emb.py:78-83): W fp32 [N, D] with row stride ldw >= D (elements) -> codes_out, in one pass:
 *   rintf(W / scale[0] + (float)zero[0]) — IEEE division, round half to even —, clamped to [-2^(n_bits-1), 2^(n_bits-1) - 1]
 *   for n_bits < 8, narrowed to the storage type through int32.  n_bits 4 or 8: int8 [N, D] (zero an int8 word), packed != 0
 *   (n_bits 4, D even): uint8 [N, D/2] in the layout above; n_bits 16: int16 [N, D] (zero an int16 word).
 * mi_int4_repack (ptq_emb.py:83, a reference n_bits = 4 checkpoint): unpack == 0: src int8 codes [N, D] -> dst packed
 *   [N, D/2]; a code outside [-8, 7] ORs MI_CODE_OUT_OF_RANGE into *err (dst is then not a table; no host read in the call).
 *   unpack != 0: src packed -> dst int8 [N, D].  src and dst do not overlap.
 */
#define MI_QTYPE_INT4_PACKED 5
#define MI_CODE_OUT_OF_RANGE 4   /* a bit of *err beside MI_IDX_OUT_OF_RANGE / MI_IDX_OUT_OF_FIELD */
MI_API int mi_gather_rows_int4(const int64_t *idx, const int64_t *offsets, const void *W, const float *scale,
                               const void *zero, float *out, int64_t *rows_out, int64_t n, int32_t F, int32_t D,
                               int64_t N, int32_t *err, void *stream);
MI_API int mi_ptq_quantise(const float *W, int64_t ldw, const float *scale, const void *zero, int32_t n_bits,
                           int32_t packed, void *codes_out, int64_t N, int32_t D, void *stream);
MI_API int mi_int4_repack(const void *src, void *dst, int32_t unpack, int64_t N, int32_t D, int32_t *err, void *stream);

/* ---- §8f rank 4 (fourth flavour): OptEmbed supernet lookup ---------------------------------------
 * OptEmbed.forward / get_weight (src/models/embeddings/deepfm_opt_embed.py:150-243) with _MaskEmbeddingModule
 * and BinaryStep (optembed_utils.py:10-112):
 *   y[i,:] = W[idx[i],:] * [ ||W[idx[i]]||_norm - t[tix] > 0 ] * [dim <= dmax[i]]
 * tix = tix[i] if given, else i % F (one threshold per field of a [B, F] lookup); t NULL = no row mask,
 * dmax NULL = all dimensions.  Backward: dW (dense, caller-zeroed, float atomics) gets the masked g plus the
 * straight-through term (sum_d g_d m_d w_d) * a(u) * d||w||/dw with BinaryStep's surrogate a(u); dt[tix] -= the
 * same scalar (caller-zeroed).  dW / dt nullable.                                                        */
MI_API int mi_optembed_fwd(const int64_t *idx, const float *W, const float *t, const int64_t *tix,
                           int32_t F, const int64_t *dmax, int32_t norm, float *out, int64_t n,
                           int32_t D, int64_t N, int32_t *err, void *stream);
MI_API int mi_optembed_bwd(const int64_t *idx, const float *W, const float *t, const int64_t *tix,
                           int32_t F, const int64_t *dmax, int32_t norm, const float *g, float *dW,
                           float *dt, int64_t n, int32_t D, int64_t N, void *stream);

/* ---- OptEmbed supernet for the CF tables (table form, no index array) ------------------------------
 * OptEmbed.get_weight of src/models/embeddings/lightgcn_opt_embed.py:121-177, _MaskEmbeddingModule and BinaryStep
 * (optembed_utils.py:25-86), the dimension draws of _sampling_by_weight (optembed_utils.py:181-202) and of the field
 * mode (lightgcn_opt_embed.py:138-152):
 *   out[r,:] = W[r,:] * [ ||W[r]||_norm - t(r) > 0 ] * [j <= k_r]
 * t(r) = t[field of r] (t_per_field; fields are the row ranges field_off[F+1]) or t[r]; t NULL = no row mask.
 * k_r = k[field of r] (k_per_field) or k[r]; k NULL = every dimension.  draw != 0: k is WRITTEN, one width per row
 * ([N]) or per field ([F]): law 0 uniform on [0, law_hi), law 1 P(k <= j) = cdf[j] (float64 [D]); the generator is
 * keyed by (seed[0], salt, row or field); seed is int64[2] on the device (seed word, zero ticket) and the launch adds
 * 1 to seed[0].  W NULL (with draw) = draw only.  A given k outside [0, D) ORs MI_IDX_OUT_OF_RANGE into *err.
 * D <= 1024 (D % 4 == 0) or D <= 256.                                                                       */
MI_API int mi_optembed_cf_fwd(const float *W, const float *t, int32_t t_per_field, const int64_t *field_off,
                              int32_t F, int64_t *k, int32_t k_per_field, int32_t draw, int32_t law, int32_t law_hi,
                              const double *cdf, int64_t *seed, int64_t salt, int32_t norm, float *out, int64_t N,
                              int32_t D, int32_t *err, void *stream);
/* Backward of mi_optembed_cf_fwd (lightgcn_opt_embed.py:121-177 through BinaryStep.backward, optembed_utils.py:34-43):
 *   dW[r] = G*s_r + c_r*a(u_r)*d||W[r]||/dW[r],  G = g*[j <= k_r],  c_r = sum_j G_j W_j,  u_r = ||W[r]|| - t(r)
 *   dt = -c_r*a(u_r), per row straight into dt, per field summed in a fixed order through dt_rows (float [N]).
 * Every dW / dt element is written once with a plain store (no zero fill, no atomics, bit-reproducible).
 * dW, dt nullable; k as given to (or drawn by) the forward.                                                  */
MI_API int mi_optembed_cf_bwd(const float *W, const float *t, int32_t t_per_field, const int64_t *field_off,
                              int32_t F, const int64_t *k, int32_t k_per_field, int32_t norm, const float *g,
                              float *dW, float *dt, float *dt_rows, int64_t N, int32_t D, void *stream);

/* ---- a11: CSR-pruned table rows (numba kernels K1/K2) ------------------------
 * src/models/embeddings/pruned_embedding.py:136-204: out[i,:] = dense row ids[i] of the
 * CSR matrix (values fp32, crow/col int64).  out fp32[n,D] need not be pre-zeroed.
 */
MI_API int mi_csr_rows_fwd(const float *values, const int64_t *crow, const int64_t *col,
                           const int64_t *ids, float *out, int64_t n, int32_t D,
                           int64_t N, int32_t *err, void *stream);

/* ---- the CTR models served from a CSR-pruned table (inference only) --------------
 * scripts/deepfm/infer_deepfm.py (_load_pep: PrunedEmbedding.from_other_emb inside a DeepFM).  The triple is trusted as
 * mi_csr_rows_fwd trusts it; crow is int32 (crow_bytes = 4) or int64 (8), col one unsigned byte (col_bytes = 1) or
 * int64 (8).  A row is densified as mi_csr_rows_fwd densifies it — zero, then out[col[j]] = values[j] for j ascending in
 * crow[row] .. crow[row + 1]: a later duplicate wins, a column outside [0, D) is ignored — by the lanes of a row slot
 * together: the entries are loaded once and passed round in order.  values / col may be NULL for a table without entries.
 * mi_gather_fm_csr_fwd: DeepFM's lookup in ONE launch.  row = idx[b,f] + offsets[f] (offsets nullable); emb fp32[B,F,D]
 *   the densified rows; yfm[b] = the FM second-order term of emb[b] + sum_f w1[row * ldw1] + bias[0] (bias nullable);
 *   rows_out int64[B,F], nullable: the row ids.  A row outside [0, N) reads as a zero row, adds nothing to yfm and ORs
 *   MI_IDX_OUT_OF_RANGE into *err.  D = 4 * 2^k <= 256 with emb 16-byte aligned runs the float4 kernels, anything else
 *   the scalar ones: the same emb bits.
 * mi_csr_rows_typed_fwd: the densify alone, out fp32[n,D] over the n flat ids.  offsets non-NULL (int64[F], n % F == 0):
 *   row = ids[i] + offsets[i % F].  rows_out int64[n], nullable: the row ids.                                           */
MI_API int mi_gather_fm_csr_fwd(const int64_t *idx, const int64_t *offsets, const float *values, const void *crow,
                                int32_t crow_bytes, const void *col, int32_t col_bytes, const float *w1, int64_t ldw1,
                                const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out,
                                int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err, void *stream);
MI_API int mi_csr_rows_typed_fwd(const float *values, const void *crow, int32_t crow_bytes, const void *col,
                                 int32_t col_bytes, const int64_t *ids, const int64_t *offsets, int32_t F,
                                 int64_t *rows_out, float *out, int64_t n, int32_t D, int64_t N, int32_t *err,
                                 void *stream);

/* ---- a9: DHE universal hash features ------------------------------------------
 * src/models/embeddings/dh_embedding.py:213-236:
 *   out[i,k] = 2*(((slopes[k]*(ids[i]+prefix+1)+bias[k]) mod primes[k]) mod m)/(m-1) - 1
 * int64 floor-mod (bit-exact with torch %), then fp32 in the reference's op order.
 */
MI_API int mi_dhe_hash(const int64_t *ids, const int64_t *slopes, const int64_t *bias,
                       const int64_t *primes, float *out, int64_t n, int32_t K,
                       int64_t prefix, int64_t m, void *stream);

/* ---- a14: LightGCN propagation step, CSR SpMM with fused layer-sum ----------
 * src/models/lightgcn.py:82-88 (`step = matrix @ step; res = res + step; res / (L+1)`):
 *   y        = A[row,:] . X                      A in CSR: crow int32[n_rows+1], col int32, val fp32
 *   Y[row]   = y                                 (Y nullable: the last layer needs no `step`)
 *   acc_out[row] = (acc_in[row] + y) * scale     (acc_out nullable; acc_in nullable = 0; in place ok)
 * The reference hands over int64 crow/col (torch CSR); the host converts them to int32 once per
 * matrix.  X fp32[n_cols,D] may be split in two row segments (Xa rows [0,x_split), Xb the rest;
 * Xb null = one segment) so cat(user_table, item_table) (lightgcn.py:71-77) is never built;
 * likewise acc_in.  short_rows / long_rows (nullable pair) list the rows handled one-per-wave
 * and one-per-workgroup (hubs); null = every row one-per-wave.
 * The backward of `matrix @ step` is the same call on the transposed CSR.
 */
MI_API int mi_spmm_csr(const int32_t *crow, const int32_t *col, const float *val,
                       const float *Xa, const float *Xb, int32_t x_split, float *Y,
                       const float *acc_in_a, const float *acc_in_b, int32_t acc_split,
                       float *acc_out, float scale, int32_t n_rows, int32_t D,
                       const int32_t *short_rows, int32_t n_short,
                       const int32_t *long_rows, int32_t n_long, void *stream);
/* The same product with a row mask of X: bit (r & 31) of xmask[r >> 5] == 0 promises that row r of X = [Xa; Xb] is all
 * zeros, and the planned kernel does not fetch it (NULL: mi_spmm_csr).  mi_row_mask builds such a mask from X itself
 * ((n_rows + 31) / 32 words; D / 4 a power of two <= 64).  Serves the FIRST layer of a backward propagation
 * (src/models/lightgcn.py:82-88 through autograd): the incoming gradient is non-zero only on the batch's rows. */
MI_API int mi_row_mask(const float *Xa, const float *Xb, int32_t x_split, int32_t n_rows, int32_t D, uint32_t *mask,
                       void *stream);
MI_API int mi_spmm_csr_masked(const int32_t *crow, const int32_t *col, const float *val, const float *Xa,
                              const float *Xb, int32_t x_split, float *Y, const float *acc_in_a,
                              const float *acc_in_b, int32_t acc_split, float *acc_out, float scale, int32_t n_rows,
                              int32_t D, const int32_t *short_rows, int32_t n_short, const int32_t *long_rows,
                              int32_t n_long, const uint32_t *xmask, void *stream);
/* The same with a selection of OUTPUT rows for the LAST layer of a training step's propagation, which is read at the
 * batch's rows only: short_rows = the batch's non-hub rows (repeats allowed — Y / acc_out must then not alias the
 * inputs), long_rows = the graph's hub rows, of which only those whose byte in hub_need is set are computed (the byte is
 * cleared again by the kernel; NULL: all of them).  mi_batch_row_list builds both from a batch: out[3B] = users | U + pos |
 * U + neg with hubs (is_hub[row] != 0) and out-of-range ids replaced by `filler` (any non-hub row) and hub_need[row] = 1
 * for the hubs.  Rows that are not selected keep whatever Y / acc_out held. */
MI_API int mi_batch_row_list(const int64_t *users, const int64_t *pos, const int64_t *neg, int64_t B, int64_t U,
                             int64_t n_rows, const uint8_t *is_hub, int32_t filler, int32_t *out, uint8_t *hub_need,
                             void *stream);
MI_API int mi_spmm_csr_sel(const int32_t *crow, const int32_t *col, const float *val, const float *Xa,
                           const float *Xb, int32_t x_split, float *Y, const float *acc_in_a,
                           const float *acc_in_b, int32_t acc_split, float *acc_out, float scale, int32_t n_rows,
                           int32_t D, const int32_t *short_rows, int32_t n_short, const int32_t *long_rows,
                           int32_t n_long, const uint32_t *xmask, uint8_t *hub_need, void *stream);

/* The same product (and fused epilogue) in the TILED form (round 3; csrc/spmm.hip): a workgroup owns a tile of consecutive
 * output rows whose sums live in LDS for the whole launch, the tile's edges — one per 16-lane group, gathered row of X
 * times value added with LDS float atomics — are walked column block by column block so that the block of X being
 * gathered from stays in the XCD's L2.  Built once per sparsity pattern by the caller (CsrPlan.tiles on the Python side):
 *   tile_edge0, tile_row0  int32[ntiles + 1]  first edge / first output row of every tile; the tiles' row ranges cover
 *                          [0, n_rows) exactly once, at most max_tile_rows rows each (max_tile_rows * D * 4 <= 64 KiB);
 *   ecr   int32[nnz] = column | (row - tile_row0[tile]) << 23   (columns < 2^23), eval fp32[nnz] the values, both in
 *                          tile order with each tile's edges grouped by column block.
 * X / acc_in as two row segments, Y / acc_out / scale as in mi_spmm_csr.  The order of the LDS adds depends on timing:
 * results agree with mi_spmm_csr to float rounding, not bitwise. */
MI_API int mi_spmm_tiled(const int32_t *tile_edge0, const int32_t *tile_row0, int32_t ntiles, int32_t max_tile_rows,
                         const int32_t *ecr, const float *eval, const float *Xa, const float *Xb, int32_t x_split,
                         float *Y, const float *acc_in_a, const float *acc_in_b, int32_t acc_split, float *acc_out,
                         float scale, int32_t D, void *stream);

/* Round 4: task-balanced, slice-phased SpMM (src/models/lightgcn.py:79-87, the same product).  The columns of A (rows of
 * X) are cut into slices of <= ~2 MiB of X; the rows of A are packed once per sparsity pattern into tasks of about equal work
 * whose edges are stored slice by slice: every wave of the chip then gathers from the same slice of X at about the same time
 * and each XCD's 4 MiB L2 serves the re-uses (the row-per-wave kernel re-fetches X 8.4x).  NPW = 256 / D lane groups per wave.
 *   tptr  int32[n_tasks, NPW + 1]  narrow task: lane group k's edges = [tptr[k], tptr[k+1]); wide task: [tptr[0], tptr[1])
 *   trows int32[n_tasks, 4 NPW]    narrow: group k owns rows trows[j NPW + k], j = 0..3; wide: rows trows[j NPW]; -1 = none
 *   twide uint8[n_tasks]           1 = wide (all groups stride one edge range: rows of 48..256 nonzeros)
 *   ecol  int32[n_edges]           column | (which of its owner's rows) << 28, slice by slice inside a range; eval the values
 *   long_rows: hub rows, computed from the CSR (crow, col, val) by an 8-wave workgroup each; tasks + hubs cover every row once.
 * Other arguments as mi_spmm_csr_masked.  Fixed summation order (no atomics). */
MI_API int mi_spmm_sliced(const int32_t *crow, const int32_t *col, const float *val, const int32_t *tptr,
                          const int32_t *trows, const uint8_t *twide, const int32_t *ecol, const float *eval,
                          int32_t n_tasks, const float *Xa, const float *Xb, int32_t x_split, float *Y,
                          const float *acc_in_a, const float *acc_in_b, int32_t acc_split, float *acc_out,
                          float scale, int32_t D, const int32_t *long_rows, int32_t n_long, const uint32_t *xmask,
                          void *stream);

/* ---- a14b: HCCF layer (src/models/hccf.py:53-63), the product above with a leaky-residual epilogue ----
 * With S = [user_emb_step; item_emb_step] (n_rows = users + items) and the square block adjacency
 * A = [[0, M], [M^T, 0]] in CSR (M = sparse_dropout(matrix): one draw serves both blocks, so A is symmetric):
 *   pre          = A[row,:] . S                       S as two row segments (Sa rows [0,s_split), Sb the rest; Sb null = one)
 *   S_out[row]   = S[row] + LeakyReLU_slope(pre)      (S_out nullable: the last layer; it must not alias S)
 *   R_out[row]   = (R[row] + S_out[row]) * scale      R as two row segments likewise; R_out may alias R (in place)
 *   bits[row]    = ceil(D/32) words, bit d%32 of word d/32 set iff pre[d] > 0   (nullable: no backward, or slope == 1)
 * short_rows / long_rows as in mi_spmm_csr.  D = 4 * 2^k <= 256 with 16-byte aligned operands takes the float4 kernel, any
 * other D one wave per row.  One launch; no atomics, so the sum order is the CSR's and reruns give the same bits.
 *
 * mi_hccf_bwd is one step of the backward recurrence  G_{k-1} = c g + G_k + A (G_k . f_k),  f_k = 1 where the bit of
 * layer k is set, else slope (torch's convention: pre == 0 takes the slope):
 *   out[row] = xscale * (sum_j A[row,j] * (G[j,:] . f[j,:]) + G[row]) + cg * g[row]
 * G and g as two row segments each; the first step (k = L) passes G = g and xscale = c (G_L = c g is never stored), later
 * steps xscale = 1.  bits null: f = 1.  xmask (nullable) as in mi_spmm_csr_masked: rows of G promised to be all zeros.
 * out must alias neither G nor g. */
MI_API int mi_hccf_fwd(const int32_t *crow, const int32_t *col, const float *val, const float *Sa, const float *Sb,
                       int32_t s_split, float *S_out, const float *Ra, const float *Rb, int32_t r_split, float *R_out,
                       float scale, float slope, uint32_t *bits, int32_t n_rows, int32_t D, const int32_t *short_rows,
                       int32_t n_short, const int32_t *long_rows, int32_t n_long, void *stream);
MI_API int mi_hccf_bwd(const int32_t *crow, const int32_t *col, const float *val, const float *Ga, const float *Gb,
                       int32_t G_split, float xscale, const uint32_t *bits, float slope, const float *ga, const float *gb,
                       int32_t g_split, float cg, float *out, int32_t n_rows, int32_t D, const int32_t *short_rows,
                       int32_t n_short, const int32_t *long_rows, int32_t n_long, const uint32_t *xmask, void *stream);

/* ---- a10: TT-Rec lookup (TTRecTorch semantics) --------------------------------
 * src/models/embeddings/tensortrain_embeddings.py:100-150: mixed-radix split of idx over
 * p_shapes, one slice per core (core c: fp32[1, p_c, r_c*q_c*r_{c+1}] viewed (p_c,r_c,q_c,r_{c+1})),
 * chain contraction -> out fp32[n, D], D = prod(q_shapes).  `cores`, `gcores`, `p_shapes`,
 * `q_shapes`, `ranks` (ncores+1 entries, first and last 1) are HOST arrays; cores[c]/gcores[c] are
 * device pointers.  2 <= ncores <= 4.  Ids outside [0, N) are flagged and yield zeros.
 * mi_tt_bwd adds the dense gradients of every core into caller-zeroed gcores[c] (float atomics).
 */
MI_API int mi_tt_fwd(const int64_t *idx, const float *const *cores, int32_t ncores,
                     const int32_t *p_shapes, const int32_t *q_shapes, const int32_t *ranks,
                     float *out, int64_t n, int32_t D, int64_t N, int32_t *err, void *stream);
MI_API int mi_tt_bwd(const int64_t *idx, const float *g_out, const float *const *cores,
                     float *const *gcores, int32_t ncores, const int32_t *p_shapes,
                     const int32_t *q_shapes, const int32_t *ranks, int64_t n, int32_t D,
                     int64_t N, void *stream);

/* ---- a10, grouped form: the TT-Rec lookup as one GEMM per core slice ---------------------------
 * Same arithmetic as mi_tt_fwd/bwd (tensortrain_embeddings.py:100-150).  The lookups of level c are
 * ordered by their digit i_c, so that all lookups sharing the slice core_c[i_c] are consecutive rows:
 *   res_c[(l,h), :] = res_{c-1}[(l,h), :] . core_c[i_c(l)]   viewed [r_c, q_c*r_{c+1}]
 * runs on the MFMA units through mi_gemm_f32_row_groups (forward and input gradient) and
 * mi_gemm_f32_k_groups (slice gradients); the host side (recsys-benchmark_amd/_kernels.py) builds the
 * orderings with device-side sorts, no host sync.
 *   mi_tt_digits: digits[c*n + i] = c-th mixed-radix digit of idx[i] over p_shapes (int32); ids outside
 *     [0, N) give digits 0, valid[i] = 0 and MI_IDX_OUT_OF_RANGE in *err.
 *   mi_move_chunks: dst[dst_row[i]*dst_stride + e] (= or +=, float atomics) src[src_row[i]*src_stride + e]
 *     for e < width (multiple of 4), zeroed / skipped where mask[i] == 0; NULL row arrays = identity.
 *   mi_gemm_f32_row_groups: C[M,N] = A[M,K] . opB(B + mtile_b[m/64]*sB); 64-row tiles with mtile_b < 0
 *     are skipped (the rows of a group are padded to whole tiles).
 *   mi_gemm_f32_k_groups: for each segment s: C[kseg[s][2]*sC ...][M,N] += A[k0:k0+K, :M]^T . B[k0:k0+K, :N]
 *     with (k0, K) = kseg[s][0:2], float atomics, C zeroed by the caller.
 *   mi_tt_plan_level: counting sort of the lookups by digit[n] in [0, p), p <= 4096: pos[i] = first row of lookup i in the
 *     level's layout (groups in digit order, each padded to whole 64-row tiles, H rows per lookup; order inside a
 *     group unspecified), mtile_b[ntiles] = group of every row tile (-1 unused), kseg[nseg][3] = the groups' rows
 *     cut into segments of <= seg rows, pbeg[p] = first row of every group.  ntiles >= ceil(n*H/64) + p,
 *     nseg >= ceil(n*H/seg) + p; workspace: 2*p int32.
 *   mi_segment_sum: out[kseg[s][2]*ldo + j] += sum_{r<K} X[(k0+r)*ldx + j], j < width (core 0's gradient:
 *     the lookups sharing a first digit are consecutive rows).                                          */
MI_API int mi_tt_digits(const int64_t *idx, int64_t n, int64_t N, const int32_t *p_shapes,
                        int32_t ncores, int32_t *digits, uint8_t *valid, int32_t *err, void *stream);
MI_API int mi_move_chunks(const float *src, const int64_t *src_row, int64_t src_stride, float *dst,
                          const int64_t *dst_row, int64_t dst_stride, int32_t width, int64_t n,
                          const uint8_t *mask, int32_t accumulate, void *stream);
MI_API int mi_gemm_f32_row_groups(const float *A, const float *B, float *C, int32_t M, int32_t N,
                                  int32_t K, int32_t lda, int32_t ldb, int32_t ldc, int32_t transB,
                                  int64_t sB, const int32_t *mtile_b, void *stream);
/*   mi_tt_last_fwd / mi_tt_last_bwd: the LAST level (rank 1 on the right, q = q_last output columns) without a GEMM:
 *     out[l, h*q + j] = sum_k chunk_l[h, k] * core[digit[l]][k, j], chunk_l = src + src_row[l]*src_stride (H x K floats);
 *     bwd: dst + dst_row[l]*dst_stride <- dchunk_l[h, k] = sum_j g[l, h*q+j] * core[digit[l]][k, j]   (dst nullable);
 *          gcore[grp][k, j] += sum over each kseg segment (first, count, grp) of lookups order[first + r]   (gcore nullable,
 *          caller-zeroed, float atomics).  H*q <= 64 and a divisor of 64, H*K <= 512, K*q <= 512.                                   */
MI_API int mi_tt_last_fwd(const float *src, const int64_t *src_row, int64_t src_stride, const float *core,
                          const int32_t *digit, const uint8_t *valid, int32_t H, int32_t K, int32_t q,
                          float *out, int64_t n, void *stream);
MI_API int mi_tt_last_bwd(const float *src, const int64_t *src_row, int64_t src_stride, const float *core,
                          const int32_t *digit, const uint8_t *valid, int32_t H, int32_t K, int32_t q,
                          const float *g, float *dst, const int64_t *dst_row, int64_t dst_stride,
                          const int64_t *order, const int64_t *kseg, int32_t nseg, float *gcore,
                          int64_t n, void *stream);
MI_API int mi_tt_plan_level(const int32_t *digit, int64_t n, int32_t p, int32_t H, int32_t seg,
                            int32_t *workspace, int64_t *pbeg, int64_t *pos, int32_t *mtile_b,
                            int32_t ntiles, int64_t *kseg, int32_t nseg, void *stream);
MI_API int mi_segment_sum(const float *X, int64_t ldx, int32_t width, const int64_t *kseg,
                          int32_t nseg, float *out, int64_t ldo, void *stream);
MI_API int mi_gemm_f32_k_groups(const float *A, const float *B, float *C, int32_t M, int32_t N,
                                int32_t lda, int32_t ldb, int32_t ldc, int64_t sC, const int64_t *kseg,
                                int32_t nseg, void *stream);

/* ---- a10, LFU row cache: the `tt_emb` table (TTEmbeddingBag with use_cache) ---------------------------
 * Buffers of src/models/embeddings/tt_embedding_ops.py:585-649: hashtbl int64[S] (ids, -1 empty), cache_freq int64[S],
 * cache_state int32[S] (row of cache_weight fp32[C, D] holding the slot's id, or -1).  The FBTT kernels behind
 * update_cache_state / preprocess_indices_sync / cache_forward are not in the reference tree; the probe rule is this
 * build's own: open addressing, start slot id % S, linear probing, a probe stops at the id, at an empty slot or after
 * MI_TT_CACHE_PROBE_BOUND probes — the same bound for insert and find.  S >= N is direct addressing (slot == id).
 *   mi_tt_cache_probe_count: for every lookup, in ONE launch: find or insert idx[i] (64-bit compare-and-swap on an empty
 *     slot; a loser re-reads the slot it lost), cache_freq[slot] += 1 (the lanes of a wave holding the same id elect one
 *     adder that carries their number; integer atomics only), loc[i] = cache_state[slot], or -1 when the id found no slot
 *     within the bound, is not cached, names a row >= cache_size, or *warmup != 0 (warmup: device word, nullable).  Ids
 *     outside [0, N) count nothing, get loc -1 and set MI_IDX_OUT_OF_RANGE.
 *   mi_tt_cache_rehash: inserts every src_ids[i] >= 0 by the rule above and stores (src_freq[i], src_state[i]) at its slot;
 *     the caller pre-fills hashtbl / cache_state with -1 and cache_freq with 0.  The sources must not alias the
 *     destinations.  An id that finds no slot within the bound is dropped (untracked).
 *   mi_tt_cached_fwd / mi_tt_cached_bwd: mi_tt_fwd / mi_tt_bwd where a lookup with 0 <= loc[i] < cache_size copies its
 *     cached row forward and adds nothing to gcores backward; every other lookup runs mi_tt_fwd / mi_tt_bwd's statements
 *     in their order (same bits forward).  cache_weight's gradient is the caller's (rows of g added at loc).          */
#define MI_TT_CACHE_PROBE_BOUND 64
MI_API int mi_tt_cache_probe_count(const int64_t *idx, int64_t n, int64_t N, int64_t *hashtbl, int64_t *cache_freq,
                                   const int32_t *cache_state, int64_t hashtbl_size, int32_t cache_size,
                                   const int32_t *warmup, int32_t *loc, int32_t *err, void *stream);
MI_API int mi_tt_cache_rehash(const int64_t *src_ids, const int64_t *src_freq, const int32_t *src_state,
                              int64_t n_src, int64_t *hashtbl, int64_t *cache_freq, int32_t *cache_state,
                              int64_t hashtbl_size, void *stream);
MI_API int mi_tt_cached_fwd(const int64_t *idx, const int32_t *loc, const float *cache_weight, int32_t cache_size,
                            const float *const *cores, int32_t ncores, const int32_t *p_shapes,
                            const int32_t *q_shapes, const int32_t *ranks, float *out, int64_t n, int32_t D,
                            int64_t N, int32_t *err, void *stream);
MI_API int mi_tt_cached_bwd(const int64_t *idx, const int32_t *loc, int32_t cache_size, const float *g_out,
                            const float *const *cores, float *const *gcores, int32_t ncores,
                            const int32_t *p_shapes, const int32_t *q_shapes, const int32_t *ranks, int64_t n,
                            int32_t D, int64_t N, void *stream);

/* ---- a12/a13: fp32 MFMA GEMM with fused CrossNet epilogues ------------------
 * C[M,N] = epi( sum_{g<kgroups} opA(A + g*gA)[M,K] . opB(B + g*gB)[K,N] ), batched over `batch`
 * with element strides sA/sB/sC (and sR1/sR2/sC2).  transA=0: A[m*lda+k], 1: A[k*lda+m];
 * transB=0: B[k*ldb+n], 1: B[n*ldb+k] (nn.Linear weight layout).  v_mfma_f32_32x32x2_f32, exact fp32.
 * epi: 0 C=acc | 1 C=acc+bias[n] | 2 C=tanh(acc)
 *      3 lin=acc+bias[n]*rs(m); C=R1+R2*lin; C2(opt)=lin   rs(m)=sum_{e<nrs} rowscale[m*nrs+e] (1 if null)
 *        -> DCNHead `x_l + x_0*(W x_l + b)` (src/models/layer_dcn.py:137-139) and the DCN_MixHead
 *           output `x_l + x_0 * sum_e g_e (U_e h_e + b)` (:102-113) with K = E*rank
 *      4 C=R1+acc(+R2)(+sum_{e<nrs} rowscale[m*nrs+e]*bias[e*N+n] when rowscale and bias are given: the gate's share
 *        dgate.G of dx_l, layer_dcn.py:100-113 differentiated) | 5 C=acc*(1-R1^2) (tanh') | 6 h=tanh(acc); C=h; C2=h*rowscale[m*nrs+z] | 7 C+=acc
 * splitk > 1 (epi 0 or 7 only; for epi 0 the caller zeroes C): the K loop is cut into `splitk` slices
 * on separate workgroups that add into C with float atomics — for the weight-gradient products
 * whose M x N is a handful of tiles while K is the batch (dW = dlin^T x_l, K = 4096).
 */
MI_API int mi_gemm_f32(const float *A, const float *B, float *C, int32_t M, int32_t N,
                       int32_t K, int32_t lda, int32_t ldb, int32_t ldc, int32_t transA,
                       int32_t transB, int32_t batch, int64_t sA, int64_t sB, int64_t sC,
                       int32_t kgroups, int64_t gA, int64_t gB, int32_t epi,
                       const float *bias, const float *R1, int32_t ldr1, int64_t sR1,
                       const float *R2, int32_t ldr2, int64_t sR2, const float *rowscale,
                       int32_t nrs, float *C2, int32_t ldc2, int64_t sC2, int32_t splitk,
                       void *stream);

/* Several independent products of ONE operand layout in a single launch — the weight gradients of a CrossNet backward
 * (src/models/layer_dcn.py:27-115 through autograd: dU, dC, dV, dG of every layer are each a few 64x64 tiles with a
 * B-long reduction; one at a time none fills the chip).  Problem j: C_j[batch] (+)= opA(A_j) opB(B_j), batch strides
 * sA/sB/sC, `splitk` K-slices that meet in float atomics (then C_j must be zeroed by the caller, or accumulate != 0);
 * splitk = 0 leaves the cut to the library (C_j zeroed / accumulate as for any cut).
 * n <= 16; transA/transB as in mi_gemm_f32 and common to all problems.  `probs` is a HOST array read during the call.
 * The form transA = 1, transB = 0 (both operands reduction-major: dW = dz^T a, also the MLP tail's weight gradients)
 * runs — when every problem has K % 32 == 0, M % 4 == N % 4 == 0 and 16-byte aligned operands / strides — on a kernel
 * that moves both operands global -> LDS by DMA in their memory layout (MI_GEMM_TN_DMA=0 in the environment: the
 * general kernel).
 * mi_gemm_f32_multi_plan: the cut that call would make, by host arithmetic only (nothing launched, no GPU needed):
 * *kind = 1 (the LDS-DMA kernel) or 0 (the general one), splitk[j] = K-slices of problem j (n entries; 0 for an empty
 * problem), *workgroups = the launch's size.
 * mi_gemm_f32_multi_slots: likewise host arithmetic only — *slots = the depth of the LDS ring the LDS-DMA kernel would run
 * that launch with: 3 (loads two slices ahead, three workgroups per CU) when all its workgroups are resident at three per
 * CU, else 2 (five per CU); MI_GEMM_TN_SLOTS=2|3 in the environment forces one; 0 when the general kernel takes the launch. */
typedef struct mi_gemm_problem {
  const float *A, *B;
  float *C;
  int32_t M, N, K;
  int32_t lda, ldb, ldc;
  int32_t batch;
  int64_t sA, sB, sC;
  int32_t splitk;
  int32_t accumulate;
} mi_gemm_problem;
MI_API int mi_gemm_f32_multi(const mi_gemm_problem *probs, int32_t n, int32_t transA, int32_t transB, void *stream);
/* ... carrying a mi_prefetch_rows job in workgroups past the products' grid: the MLP tail's weight-gradient launch is
 * MFMA-bound (~45 us with the HBM idle), the lookup of the NEXT step is a chain of HBM round trips — touched here, its table
 * lines wait in the Infinity Cache (DeepFM.prefetch_next; src/trainer/deepfm.py:40-60 holds the next batch while the step
 * runs).  ride == NULL: mi_gemm_f32_multi.  A launch that cannot carry it (not the A^T B LDS-DMA form) runs the job as a
 * launch of its own first. */
MI_API int mi_gemm_f32_multi_ride(const mi_gemm_problem *probs, int32_t n, int32_t transA, int32_t transB,
                                  const mi_prefetch_rows_job *ride, void *stream);
MI_API int mi_gemm_f32_multi_plan(const mi_gemm_problem *probs, int32_t n, int32_t transA, int32_t transB, int32_t *kind,
                                  int64_t *workgroups, int32_t *splitk);
MI_API int mi_gemm_f32_multi_slots(const mi_gemm_problem *probs, int32_t n, int32_t transA, int32_t transB, int32_t *slots);

/* The same contraction on a second tiling, for the large products of a DCN_MixHead layer (layer_dcn.py:90-115 and their
 * gradients): C[M,N] = epi(A[M,K] . B), A row-major.  A workgroup owns a 64-row panel of A by one of nt equal column ranges
 * (<= 112 columns), nt chosen so that the grid is whole rounds of 256 workgroups (N = 352: 4 x 88) — where 64 x 64 tiles
 * leave half of the second round empty.  B: b_layout 0: B(k,n) = B[(k/gw)*gstride + n*ldb + k%gw] (nn.Linear layout;
 * grouped: the experts' V_e^T side by side along k), b_layout 1: B(k,n) = B[(n/gw)*gstride + k*ldb + n%gw]; gw = the
 * whole extent and gstride = 0 for an ungrouped B.  epi: 0, 2, 3, 4 of mi_gemm_f32 (R1, R2, C2 share C's row pitch ldc;
 * epi 3/4 take bias / rowscale / nrs as there).  Everything 16-B aligned and N, K, gw, the pitches multiples of 4, else
 * MI_ERR_UNSUPPORTED (the caller keeps mi_gemm_f32). */
MI_API int mi_gemm_f32_panel(const float *A, int32_t lda, const float *B, int32_t ldb, int32_t b_layout,
                             int32_t gw, int64_t gstride, float *C, int32_t ldc, int32_t M, int32_t N,
                             int32_t K, int32_t epi, const float *bias, const float *R1, const float *R2,
                             const float *rowscale, int32_t nrs, float *C2, void *stream);

/* The per-expert middle of a DCN_MixHead layer (layer_dcn.py:96-108) with the r x r product in the epilogue of the d-long
 * one; a workgroup owns 64 rows and one expert e.  V fp32[E,d,r], C fp32[E,r,r], U fp32[E,r,d], gate fp32[M,E], the H / dZ
 * matrices fp32[M,E*r].
 *   mi_mix_expert_fwd: H1_e = tanh(x V_e); H2_e = tanh(H1_e C_e); H2g_e = H2_e * gate[m,e]
 *   mi_mix_expert_bwd: dH = dT U_e^T (never stored); dgate[m,e] = sum_k dH*H2_e + dgs[m];
 *                      dZ2_e = dH * gate[m,e] * (1 - H2_e^2); dZ1_e = (dZ2_e C_e^T) * (1 - H1_e^2)
 * r in {16, 32, 64}, d % 4 == 0, 16-B aligned; else MI_ERR_UNSUPPORTED (the caller keeps the separate products). */
MI_API int mi_mix_expert_fwd(const float *x, const float *V, const float *C, const float *gate, float *H1,
                             float *H2, float *H2g, int32_t M, int32_t d, int32_t E, int32_t r, void *stream);
MI_API int mi_mix_expert_bwd(const float *dT, const float *U, const float *C, const float *gate,
                             const float *H1, const float *H2, const float *dgs, float *dgate, float *dZ2,
                             float *dZ1, int32_t M, int32_t d, int32_t E, int32_t r, void *stream);

/* Elementwise / reduction pieces of the CrossNet backward (layer_dcn.py:90-140 differentiated):
 *   mi_cross_bwd_pre: dlin = g*x0; dx0 (+)= g*lin          (n elements)
 *   mi_colsum:        out[n] += sum_m X[m,n]*rs(m)          (out caller-zeroed; bias gradients);
 *                     rs_sum[0] += sum_m rs(m) if given (a 1-output Linear's dW and db in one launch)
 *   mi_rowdot:        out[m]  = sum_n X[m,n]*v[n] (+ bias[0]) (+ addend[m])   (also the forward of a 1-output Linear)
 *   mi_outer:         out[m,n] = g[m]*w[n]                       (its backward w.r.t. the input)
 *   mi_mix_gate_bwd:  dgate[m,e] = sum_k dH2g*H2 + dgsum[m]; dZ2 = dH2g*gate[m,e]*(1-H2^2)   ([M,E*r] operands)
 */
MI_API int mi_cross_bwd_pre(const float *g, const float *x0, const float *lin, float *dlin,
                            float *dx0, int64_t n, int32_t accumulate, void *stream);
MI_API int mi_colsum(const float *X, int32_t ldx, const float *rowscale, int32_t nrs,
                     float *out, float *rs_sum, int32_t M, int32_t N, void *stream);
MI_API int mi_rowdot(const float *X, int32_t ldx, const float *v, const float *bias,
                     const float *addend, float *out, int32_t M, int32_t N, void *stream);
/* The trainer's loss on the logits (src/trainer/deepfm.py:32,51: BCEWithLogitsLoss, reduction "mean"):
 * loss[0] = mean(max(x,0) - x*y + log1p(exp(-|x|)));  dx = g[0]*(sigmoid(x) - y)/n.  One launch each way; dx_unit
 * (nullable, [n]): the forward also writes dx for g = 1, so a backward seeded with 1 has nothing to launch. */
MI_API int mi_bce_logits_fwd(const float *x, const float *y, float *loss, float *dx_unit, int64_t n,
                             void *stream);
MI_API int mi_bce_logits_bwd(const float *x, const float *y, const float *g, float *dx, int64_t n,
                             void *stream);
MI_API int mi_outer(const float *g, const float *w, float *out, int32_t M, int32_t N,
                    void *stream);
MI_API int mi_mix_gate_bwd(const float *dH2g, const float *H2, const float *gate,
                           const float *dgsum, float *dgate, float *dZ2, int32_t M, int32_t E,
                           int32_t r, void *stream);
/*   mi_rowdot_multi:  out[m,e] = sum_n X[m,n]*W[e,n], e < E <= 8 — the DCN_MixHead gate g_e = x_l . G_e
 *                     (layer_dcn.py:100-103) as one pass over the row (N % 4 == 0, 16-B aligned; else MI_ERR_UNSUPPORTED).
 *   mi_cross_bwd_head: mi_cross_bwd_pre + the bias gradient db[n] += sum_m dlin[m,n]*rs(m) (rs = sum_e gate[m,e], 1 when
 *                     gate is NULL; db caller-zeroed) + dgs[m] = sum_n dlin[m,n]*b[n] (nullable) in ONE pass over the rows
 *                     (N % 4 == 0, N <= 1024, 16-B aligned; else MI_ERR_UNSUPPORTED and the caller uses the three calls). */
MI_API int mi_rowdot_multi(const float *X, int32_t ldx, const float *W, float *out, int32_t M,
                           int32_t N, int32_t E, void *stream);
MI_API int mi_cross_bwd_head(const float *g, const float *x0, const float *lin, const float *gate,
                             int32_t E, const float *b, float *dlin, float *dx0, int32_t accumulate,
                             float *db, float *dgs, int32_t M, int32_t N, void *stream);

/* ---- a5 (memory-bound part): BatchNorm1d + ReLU + Dropout around the MLP's Linears ---------
 * src/models/deepfm.py:53-66 / src/models/dcn.py:56-66.  Z fp32[M,N] (row stride ldz) is a Linear's
 * output.  has_bn=0 skips the normalisation (use_batchnorm=False).  training: batch statistics
 * (biased variance for the normalisation, running stats updated with `momentum` and the unbiased
 * variance, like nn.BatchNorm1d) — `stats` fp32[2,N] must be zeroed by the caller; eval: running
 * stats.  Dropout keeps an element iff splitmix64(seed[0]+salt, index) >= p*2^32 and scales by
 * 1/(1-p); the keep mask (1 byte/element) and save_mean/save_rstd fp32[N] feed the backward.
 * bump_seed (training BN only): the statistics launch first does seed[0] += 1 — one new dropout
 * stream per pass without a separate launch; num_batches_tracked (nullable) gets += 1.
 * mean_offset (nullable, training BN): added to the batch mean in the running_mean update only.  A Linear's
 * bias cancels inside a training-mode BatchNorm (it shifts z and its batch mean alike), so the caller may run the
 * contraction WITHOUT the bias, pass the bias here, and get the same y, gradients and running statistics.
 * Backward: dY NULL means a rank-1 upstream gradient dY[m,n] = gvec[m]*wvec[n] — the backward of a following
 * 1-output Linear (the tail's last layer), computed on the fly instead of being written and read back twice.
 * dgamma_dbeta fp32[2,N] (zeroed by the caller) receives dgamma then dbeta;
 * dZ = gamma*rstd*(dyh - dbeta/M - zh*dgamma/M) in training.
 */
MI_API int mi_bn_relu_dropout_fwd(const float *Z, int32_t ldz, int32_t M, int32_t N,
                                  int32_t has_bn, int32_t training, const float *gamma,
                                  const float *beta, float *running_mean, float *running_var,
                                  float momentum, float eps, float p, int64_t *seed,
                                  int64_t salt, int32_t bump_seed, int64_t *num_batches_tracked,
                                  float *stats, const float *mean_offset, float *Y, uint8_t *keep,
                                  float *save_mean, float *save_rstd, void *stream);
MI_API int mi_bn_relu_dropout_bwd(const float *dY, const float *Z, int32_t ldz, int32_t M,
                                  int32_t N, int32_t has_bn, int32_t training,
                                  const uint8_t *keep, float p, const float *gamma,
                                  const float *beta, const float *save_mean,
                                  const float *save_rstd, float *dgamma_dbeta, float *dZ,
                                  const float *gvec, const float *wvec, void *stream);

/* ---- §8f rank 3: the contrastive loss of the LightGCN step ------------------------------------
 * Reference: info_nce (src/losses.py:25-47) as called by the trainer (src/trainer/lightgcn.py:215-229).
 * mi_rownorm_fwd: Y[r,:] = X[r,:] * inv[r], inv[r] = 1/max(|X[r,:]|_2, eps)  (F.normalize(dim=1), eps 1e-12).
 * mi_rownorm_bwd: dX = inv * (dY - Y <Y,dY>)  (dX = inv * dY for a row clamped at eps).
 * mi_lse_diag_fwd: S fp32 [n,n] (row stride ld) raw scores; lse[i] = logsumexp_j(S[i,j]*inv_t);
 *   loss[0] = mean_i (lse[i] - S[i,i]*inv_t).  workspace: mi_lse_diag_workspace_elems(n) floats.
 * mi_lse_diag_bwd: S[i,j] <- g[0]/n * inv_t * (exp(S[i,j]*inv_t - lse[i]) - [i==j])  (in place: the gradient
 *   with respect to the raw scores; the two GEMMs that follow are mi_gemm_f32 calls).
 *   symmetric != 0 (both views are one matrix): writes dS + dS^T instead, so that the gradient is one product (dS+dS^T) v.
 *   valid uint8[n] + count fp32[1] (both or neither): rows/columns with valid == 0 are treated as absent and the mean runs
 *   over count[0] rows — the fixed-shape form of the trainer's torch.unique (src/trainer/lightgcn.py:407-413): the batch's
 *   rows as they come with repeated ids masked out, so the step has no data-dependent shape and can be captured.
 */
MI_API int mi_rownorm_fwd(const float *X, int64_t n, int32_t D, float eps, float *Y, float *inv,
                          void *stream);
MI_API int mi_rownorm_bwd(const float *Y, const float *inv, const float *dY, int64_t n, int32_t D,
                          float eps, float *dX, void *stream);
MI_API int64_t mi_lse_diag_workspace_elems(int32_t n);
MI_API int mi_lse_diag_fwd(const float *S, int64_t ld, int32_t n, float inv_t, const uint8_t *valid,
                           const float *count, float *lse, float *workspace, float *loss,
                           void *stream);
MI_API int mi_lse_diag_bwd(float *S, int64_t ld, int32_t n, float inv_t, const uint8_t *valid,
                           const float *count, const float *lse, const float *g, int32_t symmetric,
                           void *stream);

/* ---- §8f rank 1: fused row-sparse optimizer steps on row-form gradients -------------------
 * Reference: get_optimizers' sparse branch (src/models/deepfm.py:163-184): torch.optim.SparseAdam
 * on the embedding (no weight decay) / SGD with weight_decay=0 on it.
 * mi_sparse_adam_sorted: rows_sorted int64[n] ascending, perm int64[n] (sorted position -> entry of
 *   vals fp32[n,D]); duplicates are summed (== grad.coalesce()), then for each touched row
 *   m += (1-b1)(g-m); v += (1-b2)(g*g-v); W -= step_size * m/(sqrt(v)+eps),
 *   step_size = lr*sqrt(1-b2^t)/(1-b1^t) computed by the host (torch/optim/sparse_adam.py).
 *   step_size_dev (nullable): read the step size from device memory instead — mi_adam_tick(step, step_size, lr, b1, b2)
 *   does step[0] += 1 and writes it there, so a captured training step needs no host-side counter.
 *   acc fp32[n,D] is scratch (contents irrelevant before and after): a row repeated more often than one wave pass
 *   covers leaves a partial sum per pass there, which a second kernel adds in a fixed order (no atomics: the step is
 *   deterministic).
 */
MI_API int mi_sparse_adam_sorted(const int64_t *rows_sorted, const int64_t *perm,
                                 const float *vals, float *W, float *exp_avg,
                                 float *exp_avg_sq, float *acc, int64_t n, int32_t D,
                                 int64_t N, float step_size, const float *step_size_dev,
                                 double beta1, double beta2, float eps, void *stream);
/* the same step on a table with a row stride (row r of W starts at W + r*ldw floats, ldw >= D; exp_avg / exp_avg_sq stay
 * contiguous [N,D]): the packed DeepFM tables of mi_gather_fm_fwd_ld */
MI_API int mi_sparse_adam_sorted_ld(const int64_t *rows_sorted, const int64_t *perm,
                                    const float *vals, float *W, int64_t ldw, float *exp_avg,
                                    float *exp_avg_sq, float *acc, int64_t n, int32_t D,
                                    int64_t N, float step_size, const float *step_size_dev,
                                    double beta1, double beta2, float eps, void *stream);
/* mi_coalesce_rows_sorted: the deterministic dense gradient of a table out of its row-form gradient (what the reference's
 *   CPU index_add accumulates in a fixed order, src/models/embeddings/base.py:74-75 through autograd): G[row,:] = sum of
 *   vals[perm[i],:] over the sorted positions with rows_sorted[i] == row, added in a fixed order (the segmented sums of
 *   mi_sparse_adam_sorted, stored instead of applied; no atomics).  G fp32[N,D] zero-filled by the caller; acc fp32[n,D]
 *   scratch. */
MI_API int mi_coalesce_rows_sorted(const int64_t *rows_sorted, const int64_t *perm, const float *vals, float *G,
                                   float *acc, int64_t n, int32_t D, int64_t N, void *stream);
/* mi_sort_field_rows: rows int64[B,F] with rows[b,f] in [offsets[f], offsets[f+1]) (offsets ascending, offsets[F] := N —
 *   the ids DeepFM forms at src/models/deepfm.py:88).  rows_sorted[B*F] ascending and perm[i] = flat position b*F+f of
 *   the i-th smallest, equal ids in ascending b (a stable sort); an id outside its field's range comes back as N behind
 *   its field's valid ids (and, when it lies inside [0, N) — a row the lookup accepted — MI_IDX_OUT_OF_FIELD is OR-ed
 *   into *err: the row-wise optimizer skips id N, so that gradient is dropped and the caller must be told).  Every column is cut into runs of 1024 ids sorted by one workgroup each, then merged by
 *   rank; workspace: mi_sort_field_rows_workspace_bytes(B, F) bytes (0 when B <= 1024).  B <= 65536, N < 2^32-2, else
 *   MI_ERR_UNSUPPORTED (the caller sorts generically).
 */
MI_API int64_t mi_sort_field_rows_workspace_bytes(int64_t B, int32_t F);
MI_API int mi_sort_field_rows(const int64_t *rows, const int64_t *offsets, int64_t N, int64_t B,
                              int32_t F, int64_t *rows_sorted, int64_t *perm, void *workspace,
                              int32_t *err, void *stream);
MI_API int mi_adam_tick(float *step, float *step_size, double lr, double beta1, double beta2,
                        void *stream);
/* the same for `count` tables that share lr and betas, in one launch per 8 (host arrays of device pointers) */
MI_API int mi_adam_tick_multi(float *const *steps, float *const *step_sizes, int32_t count, double lr,
                              double beta1, double beta2, void *stream);
/* mi_adam_dense_multi: torch.optim.Adam (L2 weight decay, no amsgrad) over `count` dense fp32 tensors in as few launches as
 *   possible — get_optimizers' dense groups (src/models/deepfm.py:178-193).  The five pointer arrays and numels live in
 *   HOST memory; steps[i] points at tensor i's device-side step count (a float, torch's capturable layout), read as
 *   t = step + 1 and advanced by one after the update:
 *   g += wd*p; m += (1-b1)(g-m); v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).
 *   The betas are doubles: 1 - beta is formed in double and then rounded (1.f - 0.999f is off by 1.3e-5).
 *   tickets (nullable): ceil(count/24) device words, zero between calls — the last workgroup of each launch advances the
 *   step counts itself; without them a second one-wave launch does.
 *   Entries with numels[i] == 0 are skipped (their pointers are not read and their step counts do not advance: the
 *   caller counts those steps itself); each launch takes the next 24 non-empty entries, so no entry is updated twice.
 */
MI_API int mi_adam_dense_multi(float *const *params, const float *const *grads, float *const *exp_avgs,
                               float *const *exp_avg_sqs, float *const *steps, const int64_t *numels,
                               int32_t count, float lr, double beta1, double beta2, float eps,
                               float weight_decay, uint32_t *tickets, void *stream);
MI_API int mi_scatter_axpy_rows(const int64_t *idx, const float *g, float alpha, float *W,
                                int64_t n, int32_t D, int64_t N, void *stream);

/* ---- Adagrad and exact row-wise Adagrad on row-form gradients; dense Adagrad ----------------------------------------
 * The sparse steps run on the sorted-segment walker of mi_sparse_adam_sorted_ld and take its leading arguments:
 *   rows_sorted int64[n] ascending, perm int64[n] (sorted position -> entry of vals fp32[n,D]), W with row stride ldw >= D,
 *   acc fp32[n,D] scratch (contents irrelevant before and after), N rows; ids outside [0, N) are skipped.
 * G below is a row's COALESCED gradient: all its duplicates summed first, in the walker's fixed order (inside a pass of
 * 64 / LPR sorted positions a segmented suffix sum by shuffles; the pieces of a run that spans passes are added by a
 * second kernel, lane group r taking pieces r, r + RS, .. in that order and the groups joined by an xor tree).  The rule
 * is applied to that total only, once per row — never to a piece — so these are the EXACT forms, (sum_i g_i)^2.
 * No atomics anywhere: a rerun from the same state gives the same bits.
 *
 * mi_sparse_adagrad_sorted_ld: state_sum fp32[N,D] contiguous.  For every row that occurs, every d:
 *     s = state_sum[row,d] + G_d*G_d;  state_sum[row,d] = s;  W[row,d] -= clr * (G_d / (sqrtf(s) + eps))
 *   i.e. torch.optim.Adagrad on a sparse gradient (coalesce, touched rows only), clr = lr / (1 + (t-1)*lr_decay) formed
 *   by the host.
 * mi_rowwise_adagrad_sorted_ld: row_sum fp32[N], one accumulator per table row.  For every row that occurs:
 *     s = row_sum[row] + (sum_d G_d*G_d) / D;  row_sum[row] = s;  W[row,d] -= clr * (G_d / (sqrtf(s) + eps))  for every d
 *   sum_d runs in a fixed order: a lane adds the squares of its own VW consecutive elements in index order (VW = 4 for
 *   the float4 widths, 1 for D = 1 and 2), then the LPR = D / VW lanes of the row are joined by an xor tree over lane
 *   masks 1, 2, .. LPR/2.  In the any-D kernel lane l adds d = l, l + 64, .. in that order and the 64 lanes are joined by
 *   an xor tree over masks 32, 16, .. 1.  One lane of the group stores row_sum.
 * Width dispatch (both): D = 1 and D = 2 scalar forms; D/4 a power of two up to 64 the float4 forms when vals, W, acc
 *   (and state_sum) are 16-byte aligned — ldw % 4 != 0 at such a width is MI_ERR_UNSUPPORTED; anything else the any-D
 *   kernel.  ldw < D, negative sizes or a null pointer with n > 0: MI_ERR_INVALID_ARG; n == 0 returns MI_OK and writes
 *   nothing.
 */
MI_API int mi_sparse_adagrad_sorted_ld(const int64_t *rows_sorted, const int64_t *perm, const float *vals, float *W,
                                       int64_t ldw, float *state_sum, float *acc, int64_t n, int32_t D, int64_t N,
                                       float clr, float eps, void *stream);
MI_API int mi_rowwise_adagrad_sorted_ld(const int64_t *rows_sorted, const int64_t *perm, const float *vals, float *W,
                                        int64_t ldw, float *row_sum, float *acc, int64_t n, int32_t D, int64_t N,
                                        float clr, float eps, void *stream);
/* mi_adagrad_dense_multi: torch.optim.Adagrad (L2 weight decay, lr_decay = 0) over `count` dense fp32 tensors, 24 per
 *   launch; the three pointer arrays and numels live in HOST memory:
 *     g += wd*p;  s += g*g;  p -= lr * (g / (sqrtf(s) + eps)).
 *   No step count enters the rule, so there is no counter and no ticket.  Entries with numels[i] == 0 are skipped. */
MI_API int mi_adagrad_dense_multi(float *const *params, const float *const *grads, float *const *state_sums,
                                  const int64_t *numels, int32_t count, float lr, float eps, float weight_decay,
                                  void *stream);

/* ---- §8f rank 3: the LightGCN step either side of the propagation -------------------------------
 * mi_bpr_fwd/bwd: src/losses.py:6-22 on rows picked from the propagated tables
 *   (torch.index_select x3, src/trainer/lightgcn.py:395-399): x_b = u_b.(p_b - n_b) with
 *   u_b = U[ui[b]], p_b = P[pi[b]], n_b = Nn[ni[b]] (NULL index arrays = row b);
 *   loss = mean_b -logsigmoid(x_b) (partials joined in index order: deterministic), sig[b] = sigmoid(-x_b).
 *   bwd: dU[ui[b]] += c_b (p_b - n_b), dP[pi[b]] += c_b u_b, dN[ni[b]] -= c_b u_b, c_b = -g sig[b] / B
 *   (float atomics into caller-zeroed dense gradients when the index array is given, stores otherwise;
 *   any of dU/dP/dN may be NULL).  workspace: mi_bpr_workspace_elems(B) floats.
 *   nU/nP/nN = rows of U/P/Nn: a triple with an index outside its table touches no memory, counts as
 *   u = p = n = 0 forward, adds nothing backward, and ORs MI_IDX_OUT_OF_RANGE into *err (the
 *   reference's index_select raises: src/trainer/lightgcn.py:395-397).  Same for mi_rowsq_*.
 * mi_mask_topk_rows: src/trainer/lightgcn.py:122-138: for row b (user users[b], or b if NULL)
 *   scores[b, col[crow[u] .. crow[u+1])] = -inf (in place; crow may be NULL = no mask), then the
 *   indices (and optionally values) of the k largest entries, score descending, ties by ascending
 *   index.  k <= 256.                                                                               */
/* mi_rowsq_fwd/bwd: LightGCN.get_reg_loss (src/models/lightgcn.py:90-100) on plain tables:
 *   out = (sum_b |U[ui[b]]|^2 + |P[pi[b]]|^2 + |Nn[ni[b]]|^2) / (2B), joined in index order;
 *   bwd: dU[ui[b]] += g U[ui[b]] / B (and likewise dP, dN; float atomics, caller-zeroed, nullable).
 *   workspace: mi_bpr_workspace_elems(B) floats.                                                      */
MI_API int mi_rowsq_fwd(const float *U, const int64_t *ui, const float *P, const int64_t *pi,
                        const float *Nn, const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP,
                        int64_t nN, int32_t *err, float *workspace, float *out, void *stream);
MI_API int mi_rowsq_fwd_armed(const float *U, const int64_t *ui, const float *P, const int64_t *pi,
                              const float *Nn, const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP,
                              int64_t nN, int32_t *err, float *workspace, float *out, void *stream);
MI_API int mi_rowsq_bwd(const float *U, const int64_t *ui, const float *P, const int64_t *pi,
                        const float *Nn, const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP,
                        int64_t nN, const float *g, float *dU, float *dP, float *dN, void *stream);
/* mi_reg_prune_rows_fwd/bwd: the batch-row terms of the CERP step on LightGCN / SingleLightGCN
 *   (get_prune_and_reg_loss_lightgcn, src/models/embeddings/cerp_embedding_utils.py:15-62) on materialised tables U [nU, D]
 *   and I [nI, D], from one read of each row: ui, pi int64[B], ni int64[Bn], uvalid uint8[B] (1 = first occurrence of the
 *   user in the batch: the reference's torch.unique);
 *     out[0] = (sum_b |U[ui[b]]|^2 + sum_b |I[pi[b]]|^2 + sum_k |I[ni[k]]|^2) / (2 B)
 *     out[1] = -(sum_{b: uvalid[b]} |tanh(k_tanh U[ui[b]])|^2 + sum_b |tanh(k_tanh I[pi[b]])|^2 + sum_k |tanh(k_tanh I[ni[k]])|^2)
 *   An id outside its table is skipped and ORs MI_IDX_OUT_OF_RANGE into *err.  The workgroup partials are joined in index
 *   order by the last workgroup to take a ticket; workspace: mi_reg_prune_rows_workspace_elems(B, Bn) floats, armed != 0:
 *   the caller promises its last word is zero on entry (the kernel leaves it zero), else it is zeroed by a memset node.
 *   bwd: g[0], g[1] the upstream gradients of out[0], out[1]; adds both terms' row gradients into the caller-zeroed dense
 *   dU / dI (float atomics; either may be NULL).                                                                     */
MI_API int64_t mi_reg_prune_rows_workspace_elems(int64_t B, int64_t Bn);
MI_API int mi_reg_prune_rows_fwd(const float *U, const float *I, const int64_t *ui, const int64_t *pi,
                                 const int64_t *ni, const uint8_t *uvalid, int64_t B, int64_t Bn, int32_t D,
                                 int64_t nU, int64_t nI, float k_tanh, int32_t *err, float *workspace, int32_t armed,
                                 float *out, void *stream);
MI_API int mi_reg_prune_rows_bwd(const float *U, const float *I, const int64_t *ui, const int64_t *pi,
                                 const int64_t *ni, const uint8_t *uvalid, int64_t B, int64_t Bn, int32_t D,
                                 int64_t nU, int64_t nI, float k_tanh, const float *g, float *dU, float *dI,
                                 void *stream);
MI_API int64_t mi_bpr_workspace_elems(int64_t B);
MI_API int mi_bpr_fwd(const float *U, const int64_t *ui, const float *P, const int64_t *pi,
                      const float *Nn, const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP,
                      int64_t nN, int32_t *err, float *sig, float *workspace, float *loss, void *stream);
/* _armed: the same launch without the memset node that zeroes the arrival ticket — the caller promises the last word
 * of `workspace` is zero on entry; the kernel leaves it zero, so a workspace zeroed once serves every later call. */
MI_API int mi_bpr_fwd_armed(const float *U, const int64_t *ui, const float *P, const int64_t *pi,
                            const float *Nn, const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP,
                            int64_t nN, int32_t *err, float *sig, float *workspace, float *loss, void *stream);
/* ... with another scalar term of the step's objective joined in: loss = BPR + plus_weight * plus[0] (plus nullable; the
 * reference trainer's `loss = bpr + reg_weight * reg`, src/trainer/lightgcn.py:401-404, without a scale and an add launch).
 * With plus, `loss` has TWO words: loss[0] the sum, loss[1] the bare BPR term (what a trainer logs); without, one.
 * armed != 0: mi_bpr_fwd_armed's promise about the ticket word. */
MI_API int mi_bpr_fwd_plus(const float *U, const int64_t *ui, const float *P, const int64_t *pi, const float *Nn,
                           const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP, int64_t nN, int32_t *err,
                           float *sig, float *workspace, int32_t armed, const float *plus, float plus_weight,
                           float *loss, void *stream);
MI_API int mi_bpr_bwd(const float *U, const int64_t *ui, const float *P, const int64_t *pi,
                      const float *Nn, const int64_t *ni, int64_t B, int32_t D, int64_t nU, int64_t nP,
                      int64_t nN, const float *sig, const float *g, float *dU, float *dP, float *dN,
                      void *stream);
MI_API int mi_mask_topk_rows(float *scores, int64_t ld, int64_t nrows, int64_t ncol,
                             const int64_t *users, const int64_t *crow, const int64_t *col, int32_t k,
                             int64_t *out_idx, float *out_val, void *stream);

/* ---- NeuMF (GMF + MLP): src/models/mlp.py:11-344, trained by src/trainer/nmf.py:446-499 --------------
 * Four tables of width D = emb_size / 2: GU / GI (gmf-user / gmf-item), MU / MI (mlp-user / mlp-item).
 * flags: bit 0 = MLP, bit 1 = GMF (ModelFlag, mlp.py:11-14); at least one bit.  D <= 256.
 *
 * mi_neumf_fwd: mlp.py:82-101, 255-274 and 318-344 up to the tower: for sample s (u = users[s], i = items[s])
 *   y_gmf[s] = sum_k GU[u,k] GI[i,k] w[k] + b[0]   (gmf_fc; GMF only, else y_gmf unused)
 *   X0[s]    = [MU[u] ; MI[i]]  ([S, 2D]; the MLP tower's input, MLP only, else X0 unused)
 *   An id outside its table ORs MI_IDX_OUT_OF_RANGE into *err and reads as a zero row.               */
MI_API int mi_neumf_fwd(const int64_t *users, const int64_t *items, int64_t S, const float *GU, const float *GI,
                        const float *MU, const float *MI, int32_t D, int64_t nU, int64_t nI, const float *w, const float *b,
                        int32_t flags, float *y_gmf, float *X0, int32_t *err, void *stream);
/* mi_neumf_bwd: the backward of mi_neumf_fwd given dy [S] (GMF) and the tower's input gradient dX0 [S, 2D] (MLP):
 *   dGU[u] += dy[s] w * GI[i], dGI[i] += dy[s] w * GU[u], dMU[u] += dX0[s, :D], dMI[i] += dX0[s, D:]
 *   mode 0: the four outputs are dense [n, D] gradients, caller-zeroed, duplicates joined by float atomics;
 *   mode 1: they are row-form values [S, D] (row s belongs to users[s] / items[s]), written, no atomics.
 *   dw[k] = sum_s dy[s] GU[u,k] GI[i,k], db[0] = sum_s dy[s]: written (not accumulated) in a fixed order through
 *   `workspace` (mi_neumf_bwd_parts(S, D) * (D + 1) floats) and one finishing launch.                  */
MI_API int mi_neumf_bwd_parts(int64_t S, int32_t D);
MI_API int mi_neumf_bwd(const int64_t *users, const int64_t *items, int64_t S, const float *GU, const float *GI, int32_t D,
                        int64_t nU, int64_t nI, const float *w, int32_t flags, const float *dy, const float *dX0, int32_t mode,
                        float *dGU, float *dGI, float *dMU, float *dMI, float *dw, float *db, float *workspace,
                        void *stream);
/* mi_neumf_score_all: src/trainer/nmf.py:501-582 (the model over every item of a user batch) as one kernel:
 *   scores[b * ld + i] = mlp_fc(h_L(b, i)) + gmf_fc(GU[users[b]] * GI[i]),  b < B, i < N
 *   with h_1 = relu(P[b] + Q[i]) (P = MU[users] W1_u^T [B, h_1], Q = MI W1_i^T + b1 [N, h_1]: the caller's GEMMs)
 *   and h_l = relu(W[l-2] h_{l-1} + bias[l-2]) on v_mfma_f32_16x16x4_f32.  `hidden` (host, nhidden entries),
 *   W and bias (host arrays of nhidden - 1 device pointers).  Unused halves (flags) may be NULL.
 *   Supported (mi_neumf_score_supported != 0): 1..4 hidden layers, each <= 128 wide, the hidden weights within
 *   64 KiB of LDS once padded to 16-wide tiles, D <= 128; otherwise MI_ERR_UNSUPPORTED.               */
MI_API int mi_neumf_score_supported(int32_t nhidden, const int32_t *hidden, int32_t D, int32_t flags);
MI_API int mi_neumf_score_all(const float *P, const float *Q, int64_t B, int64_t N, int32_t nhidden, const int32_t *hidden,
                              const float *const *W, const float *const *bias, const float *wf, const float *bf,
                              const int64_t *users, const float *GU, const float *GI, int32_t D, int64_t nU, const float *wg,
                              const float *bg, int32_t flags, float *scores, int64_t ld, int32_t *err, void *stream);

/* ---- §8e: device-side routing of the row-sharded DeepFM lookup -------------------------------
 * No reference counterpart (the reference keeps one table on one device,
 * src/models/embeddings/base.py:52-57); the arithmetic either side of the exchange is the
 * reference's (src/models/deepfm.py:88-98).  Tables are sharded owner = row % world,
 * local = row / world; every shard ends in one extra SINK row that padding slots point at.
 *
 * mi_route_buckets: rows = idx + offsets[i % F] (offsets may be NULL) for n = B*F lookups; STABLE
 *   bucketing by owner into send_rows[world, cap] (owner-local row ids; unused slots = the owner's
 *   sink row ceil((N - owner) / world)), slot[n] = owner*cap + position of every lookup.  Lookups
 *   that overflow a bucket or are outside [0, N) get slot = world*cap (the dump slot) and OR 1 into
 *   *overflow / MI_IDX_OUT_OF_RANGE into *err.  workspace: mi_route_workspace_elems(n, world) int32.
 * mi_gather_pack_rows: out[i, 0:D] = W[rows[i], :], out[i, D] = w1[rows[i]], out[i, D+1:D+4] = 0;
 *   out rows are D + 4 floats (one all-to-all carries both tables).  D = 4 * 2^k only.
 * mi_slot_fm_fwd: mi_gather_fm_fwd over the received packed rows buf[nrows, D+4] addressed by slot
 *   (row nrows-1 = the zeroed dump row): emb[B,F,D], yfm[B].
 * mi_slot_fm_bwd: zero gbuf[nslot, D+4], then the row gradients of mi_gather_fm_bwd_rows written to
 *   gbuf[slot[b,f]] (first-order gradient in column D); slots >= nslot are skipped.
 * mi_unpack_rows: vals[i, 0:D] = packed[i, 0:D], lin[i] = packed[i, D] for m rows of D + 4 floats: the gradient rows
 *   received by the owner as the two contiguous value arrays of its shards' row-form gradients.
 *
 * De-duplicated routing (one slot per DISTINCT row; a hot id costs its owner one slot however often a batch holds it):
 * mi_route_buckets_unique: input is the batch's n rows in STABLE sorted order — rows_sorted[j] ascending over the rows
 *   in [0, N), perm[j] the flat lookup position of the j-th (a permutation of 0..n-1; equal rows in ascending position).
 *   mi_sort_field_rows' output qualifies (its value N for an id outside its own field counts as out of range), and so
 *   does any generic stable sort.  With owner = row % world, local = row / world as above:
 *     - an owner's bucket holds its distinct rows in ascending local order: the p-th has send_rows[owner*cap + p] = local,
 *       and EVERY lookup of that row gets slot[perm[j]] = owner*cap + p; unused slots carry the owner's sink row;
 *     - distinct rows beyond cap: their lookups get the dump slot world*cap and 1 is OR-ed into *overflow;
 *     - rows outside [0, N) get the dump slot and MI_IDX_OUT_OF_RANGE — unless `rows` (nullable: the n rows BEFORE the
 *       sort) shows the id inside [0, N): then the sort dropped it and has raised MI_IDX_OUT_OF_FIELD itself.
 *   Positions are prefix counts over the sorted order, so the outputs do not depend on scheduling.
 *   segments (int32 [2*world*cap + n], the description the backward pulls through):
 *     segments[2*s], segments[2*s + 1] = [begin, end) of slot s's lookups in the sorted order ((0, 0) for an unused slot),
 *     segments[2*world*cap + j]        = perm[j]: within [begin, end) the flat lookup positions ascend.
 *   workspace: mi_route_unique_workspace_elems(n, world) int32.  n < 2^31, world <= 64.
 * mi_slot_fm_bwd_segments: mi_slot_fm_bwd for shared slots.  gbuf[s, :] (s < nslot) = the SUM, in ascending flat lookup
 *   position, of its lookups' gradient rows (g_emb[b,f] + g_y[b] * (S_b - e) in columns 0..D-1, g_y[b] in column D, zeros
 *   behind); slots without lookups and row nslot (the dump row: gbuf has nslot + 1 rows) are written as zeros.  Two
 *   launches, no float atomics, no memset: the per-lookup rows of mi_gather_fm_bwd_rows go to `workspace`
 *   (mi_slot_fm_bwd_segments_workspace_elems(B, F, D) floats, 16-byte aligned), then every slot pulls its own.
 *   `segments` as written by mi_route_buckets_unique with world*cap = nslot.  D = 4 * 2^k only.  */
MI_API int64_t mi_route_workspace_elems(int64_t n, int32_t world);
MI_API int mi_route_buckets(const int64_t *idx, const int64_t *offsets, int64_t n, int32_t F,
                            int32_t world, int64_t N, int64_t cap, int32_t *workspace,
                            int64_t *send_rows, int64_t *slot, int32_t *overflow, int32_t *err,
                            void *stream);
MI_API int mi_gather_pack_rows(const int64_t *rows, const float *W, const float *w1, float *out,
                               int64_t m, int32_t D, int64_t Nl, int32_t *err, void *stream);
MI_API int mi_unpack_rows(const float *packed, float *vals, float *lin, int64_t m, int32_t D, void *stream);
MI_API int mi_slot_fm_fwd(const int64_t *slot, const float *buf, int64_t nrows, const float *bias,
                          float *emb_out, float *yfm_out, int64_t B, int32_t F, int32_t D,
                          int32_t *err, void *stream);
MI_API int mi_slot_fm_bwd(const int64_t *slot, const float *emb, const float *g_y,
                          const float *g_emb, float *gbuf, float *gbias, int64_t nslot, int64_t B,
                          int32_t F, int32_t D, void *stream);
MI_API int64_t mi_route_unique_workspace_elems(int64_t n, int32_t world);
MI_API int mi_route_buckets_unique(const int64_t *rows_sorted, const int64_t *perm, const int64_t *rows, int64_t n,
                                   int32_t world, int64_t N, int64_t cap, int32_t *workspace, int64_t *send_rows,
                                   int64_t *slot, int32_t *segments, int32_t *overflow, int32_t *err, void *stream);
MI_API int64_t mi_slot_fm_bwd_segments_workspace_elems(int64_t B, int32_t F, int32_t D);
MI_API int mi_slot_fm_bwd_segments(const int32_t *segments, const float *emb, const float *g_y, const float *g_emb,
                                   float *workspace, float *gbuf, float *gbias, int64_t nslot, int64_t B, int32_t F,
                                   int32_t D, void *stream);

/* ---- §8 a5 / f.2: the MLP tail as fused MFMA kernels (recsys-benchmark_amd/csrc/tail.hip) ---------------------------
 * Replaces, for (Linear, BatchNorm1d(training), ReLU, Dropout) x k + Linear(., 1) — src/models/deepfm.py:53-66,100-102
 * and src/models/dcn.py:56-66 — the library GEMMs and the separate BatchNorm / ReLU / Dropout passes.
 * An ACTIVATION is described by its saved pre-activation Z[M, ld] and per-feature constants:
 *     a(m, c) = max((Z[m,c] - mu[c]) * sc[c] + be[c], 0) * keep(m, c) / (1 - p)
 *   keep(m, c) = bit (c & 7) of keep_bits[(m*ld + c) >> 3] (ld % 8 == 0; used when p > 0), one bit per element written
 *   once per step by mi_tail_dropout_masks: 16 bits of splitmix64(seed[0] + salt', (m*ld + c)/4) >= p * 65536
 *   (nlayers <= 8 layers in one launch; salts / ps / lds / bits are HOST arrays, layers with p <= 0 are skipped).
 *   mu == NULL: the matrix is used as it is (the tail's input).
 * A PRE-ACTIVATION GRADIENT is described by DY (gradient w.r.t. the BatchNorm output, ReLU / dropout already applied),
 *   Z and constants:  dz(m, c) = al[c] * DY[m,c] + bz[c] * (Z[m,c] - mu[c]) + de[c];  al == NULL: DY is used as it is.
 * All matrices fp32 row-major, 16-byte aligned, leading dimensions and N, K multiples of 4 (else MI_ERR_UNSUPPORTED).
 * No atomics anywhere: every reduction is joined in a fixed order (bit-reproducible steps).
 *
 * mi_tail_fwd_gemm:  Z[M,N] = a(X)[M,K] . W[N,K]^T (no bias: it cancels in a training-mode BatchNorm; see mean_offset);
 *   part (nullable, mi_tail_part_elems(M, N) floats): (mean, M2) of every 64-row tile of Z, per column.
 *   a_out (nullable, [M,K] with X's pitch; needs x_mu): the activation a(X) as the operand load computed it — kept for the
 *   weight-gradient product when that runs on mi_gemm_f32_multi.
 * mi_tail_bn_finalize_fwd: joins `part` (Chan's formula, tile order) into mu = batch mean, sc = gamma * rstd, be = beta,
 *   rstd; running_mean / running_var updated as F.batch_norm(training=True) does (unbiased variance; mean_offset =
 *   the Linear's bias, added to the mean only there); *num_batches_tracked += 1; *seed_bump += 1 (nullable each).
 * mi_tail_head_fwd:  out[m] = sum_n a(m, n) w[n] + b[0] + add[m]  (b, add nullable).
 * mi_tail_head_bwd:  g[M] = dL/dout -> DY[M,N] of the last hidden layer, part[nblk, N, 2] = (sum dy, sum dy (z - mu)),
 *   wpart[nblk, N + 4] = (sum_m g a(m, n) ..., sum_m g); nblk = mi_tail_head_blocks(M).
 * mi_tail_bn_finalize_bwd: joins part[nblk, N, 2] -> dgamma, dbeta (nullable) and al, bz, de; wpart (nullable) -> dw[N], db[1].
 * mi_tail_dgrad_gemm: da[M,K] = dz[M,N] . W[N,K]; with the layer below given (p_mu != NULL):
 *   OUT = da * keep_prev/(1-p) * [pre_prev > 0] (= DY of that layer), part[MT, K, 2] (nullable) its column sums;
 *   otherwise OUT = da (the gradient of the tail's input).  dz_out (nullable, [M,N] with DY's pitch; needs al): dz as the
 *   operand load computed it, for the same purpose.
 * mi_tail_wgrad_gemm: dW[N,K] = dz[M,N]^T . a_prev[M,K]; the batch is cut into mi_tail_wgrad_splits(M, N, K) slices,
 *   slab (splits * N * K floats) holds their partial products, added in slice order into dW.                      */
/* The joins WITHOUT launches of their own (round 3): the kernel that CONSUMES an activation (or a pre-activation gradient)
 * joins the statistics behind its constants in its prologue — every workgroup for itself, in a fixed order, into LDS;
 * workgroup 0 writes the results where mi_tail_bn_finalize_fwd / _bwd would have (the backward pass and the optimizer
 * read them there).  Same arithmetic for every workgroup, no atomics: deterministic.  Host structs, read at call time.
 * mi_tail_bn_fwd: what mi_tail_bn_finalize_fwd takes — part[MT, N, 2] of the producing product, gamma / beta /
 *   mean_offset (nullable), running statistics + counters (nullable), momentum, eps — and its outputs mu, sc, be, rstd [N].
 * mi_tail_bn_bwd: what mi_tail_bn_finalize_bwd takes — part[nblk, N, 2], gamma (nullable), rstd, outputs dgamma / dbeta
 *   (nullable), al, bz, de [N]; wpart[nwblk, N + 4] (nullable) -> dw[N], db[1] (joined by a second workgroup).
 * mi_tail_fwd_gemm_m / mi_tail_head_fwd_m (x_stats / stats != NULL: the mu / sc / be arguments are ignored) and
 * mi_tail_dgrad_gemm_m (sums != NULL: al / bz / de are ignored; mu and Zl are still read); NULL = the plain entry point.
 * Features behind the joined constants <= 1024. */
typedef struct mi_tail_bn_fwd {
  const float *part;
  const float *gamma, *beta, *mean_offset;
  float *running_mean, *running_var;
  int64_t *num_batches_tracked, *seed_bump;
  float *mu, *sc, *be, *rstd;
  float momentum, eps;
  const float *shift;     /* nrep > 0: the shift the sums were taken around, [N] (mi_tail_fwd_gemm_s's shift_out) */
  int32_t nrep;           /* 0: `part` = tile statistics [MT, N, 2]; > 0: `part` = shifted sums fp64[nrep, 2, N] (mi_tail_fwd_gemm_s) */
} mi_tail_bn_fwd;
typedef struct mi_tail_bn_bwd {
  const float *part;
  const float *gamma, *rstd;
  float *dgamma, *dbeta, *al, *bz, *de;
  const float *wpart;
  float *dw, *db;
  int32_t nblk, nwblk;
  float *dbias;           /* affine != 0, nullable: the Linear bias's gradient al * sum dy, [N] */
  float *db2;             /* nullable: a second destination of db[0] (DeepFM: the scalar `_bias` is added to every logit like
                             the head's bias, so it has the same gradient — written here instead of by a copy launch) */
  int32_t affine;         /* != 0: fixed statistics (eval-mode BatchNorm) or none: dz = al dy, bz = de = 0 (mi_tail_bn_finalize_bwd_a) */
} mi_tail_bn_bwd;
MI_API int mi_tail_fwd_gemm_m(const float *X, int32_t ldx, const float *x_mu, const float *x_sc, const float *x_be,
                              float x_p, const uint8_t *x_keep, const float *W, int32_t ldw, float *Z, int32_t ldz,
                              float *part, float *a_out, int32_t M, int32_t N, int32_t K,
                              const mi_tail_bn_fwd *x_stats, void *stream);
/* BatchNorm statistics WITHOUT finalize launches (round 4).  The producing product adds, per column c and 64-row tile,
 *   t1 = sum (z - s_c),  t2 = sum (z - s_c)^2,   s_c = shift_running_mean[c] - shift_mean_offset[c]  (each nullable: 0)
 * (formed from the tile's exact count / mean / M2) into part[r, 0, c] / part[r, 1, c] — `part` holds DOUBLES here:
 * fp64[sum_reps, 2, N] = 4 sum_reps N floats, 8-byte aligned, ZEROED by the caller, r = row tile % sum_reps — with f64
 * atomics (the two sums cancel by (mean - s)^2 / var when the variance is derived: fp32 sums lose that many digits)
 * and stores s into shift_out[N]; the consuming kernel (mi_tail_fwd_gemm_* / mi_tail_head_fwd_m with a mi_tail_bn_fwd whose
 * nrep = sum_reps, part and shift point at these buffers) derives mean = s + t1/M, M2 = t2 - t1^2/M and the constants in
 * its prologue from (4 nrep + 3) N floats and its first workgroup writes mu / sc / be / rstd and the running statistics
 * (F.batch_norm(training=True) semantics, src/models/deepfm.py:57-58).  sum_reps = 0 is mi_tail_fwd_gemm_m.
 * mi_tail_dgrad_gemm_s: the backward mirror — part_reps > 0: part is fp32[part_reps, K, 2] (zeroed by the caller), every row
 * tile ADDS its column sums (sum dy, sum dy (z - mu)) into row (tile % part_reps); a mi_tail_bn_bwd with nblk = part_reps
 * over the same buffer then joins them in the next product's prologue (or mi_tail_bn_finalize_bwd does).
 * Float-atomic order: results vary in the last bits between runs; deterministic callers use the tile-statistics forms. */
MI_API int mi_tail_fwd_gemm_s(const float *X, int32_t ldx, const float *x_mu, const float *x_sc, const float *x_be,
                              float x_p, const uint8_t *x_keep, const float *W, int32_t ldw, float *Z, int32_t ldz,
                              float *part, float *a_out, int32_t M, int32_t N, int32_t K,
                              const mi_tail_bn_fwd *x_stats, int32_t sum_reps, float *shift_out,
                              const float *shift_running_mean, const float *shift_mean_offset, void *stream);
/* An INFERENCE forward's last hidden layer with the head in its epilogue (eval-mode BatchNorm or none on that layer, no
 * dropout, nothing kept): z = a(X) W^T is not stored; every 64-row x <= 112-column tile adds
 * sum_n relu((z - mu[n]) sc[n] + be[n]) w[n] into out[m] with a float atomic (out ZEROED by an earlier launch — the lookup's
 * riders do it in DeepFM's forward; column tile 0 also adds b[0] and add[m]): src/models/deepfm.py:100-105 under
 * model.eval() as one launch less. */
typedef struct mi_tail_head_in_epilogue {
  const float *w;            /* [N] the head Linear(N, 1)'s weight */
  const float *b;            /* [1], nullable */
  const float *add;          /* [M], nullable (DeepFM: y_fm) */
  const float *mu, *sc, *be; /* [N] constants of THIS layer's activation (mi_tail_affine_consts) */
  float *out;                /* [M] logits, zero on entry */
} mi_tail_head_in_epilogue;
MI_API int mi_tail_fwd_gemm_head(const float *X, int32_t ldx, const float *x_mu, const float *x_sc, const float *x_be,
                                 float x_p, const uint8_t *x_keep, const float *W, int32_t ldw, int32_t M, int32_t N,
                                 int32_t K, const mi_tail_bn_fwd *x_stats, const mi_tail_head_in_epilogue *head,
                                 void *stream);
MI_API int mi_tail_dgrad_gemm_s(const float *DY, const float *Zl, int32_t ld, const float *mu, const float *al,
                                const float *bz, const float *de, const float *W, int32_t ldw, const float *pZ,
                                int32_t pld, const float *p_mu, const float *p_sc, const float *p_be, float p_p,
                                const uint8_t *p_keep, float *OUT, int32_t ldo, float *part, int32_t part_reps,
                                float *dz_out, int32_t M, int32_t N, int32_t K, const mi_tail_bn_bwd *sums,
                                void *stream);
MI_API int mi_tail_head_fwd_m(const float *Z, int32_t ldz, const float *mu, const float *sc, const float *be, float p,
                              const uint8_t *keep, const float *w, const float *b, const float *add, float *out,
                              int32_t M, int32_t N, const mi_tail_bn_fwd *stats, void *stream);
MI_API int mi_tail_dgrad_gemm_m(const float *DY, const float *Zl, int32_t ld, const float *mu, const float *al,
                                const float *bz, const float *de, const float *W, int32_t ldw, const float *pZ,
                                int32_t pld, const float *p_mu, const float *p_sc, const float *p_be, float p_p,
                                const uint8_t *p_keep, float *OUT, int32_t ldo, float *part, float *dz_out, int32_t M,
                                int32_t N, int32_t K, const mi_tail_bn_bwd *sums, void *stream);
/* DeepFM: the FIRST layer's input-gradient product with the whole of mi_gather_fm_bwd_rows in its epilogue
 * (src/models/deepfm.py:88-102 through autograd).  The tail's input is the embedding block emb[M, K = F*D]; instead of
 * storing da = dz . W and launching the gather backward on it, the epilogue writes the lookup table's row-form gradient
 *   gvals[m, f, :] = da[m, f*D : (f+1)*D] + g_y[m] * (emb_sum[m, :] - emb[m, f, :])       (fp32[M*F, D], == [M, K])
 *   g1vals[m, f]   = g_y[m]                                                               (fp32[M, F], nullable)
 * emb_sum = mi_gather_fm_fwd_sum's sum_out.  The scalar bias's gradient sum_m g_y[m] equals the head bias's (both are
 * added to every logit): callers take it from mi_tail_bn_finalize_bwd's db.  One launch and 2 * 4 * M * K bytes (da written,
 * da read back) less than the two-kernel form.  Other arguments as mi_tail_dgrad_gemm_m with no layer below. */
MI_API int mi_tail_dgrad_gemm_fm(const float *DY, const float *Zl, int32_t ld, const float *mu, const float *al,
                                 const float *bz, const float *de, const float *W, int32_t ldw, float *gvals,
                                 float *dz_out, int32_t M, int32_t N, int32_t K, const mi_tail_bn_bwd *sums,
                                 const float *emb, const float *emb_sum, const float *g_y, float *g1vals, int32_t D,
                                 void *stream);
/* ... for the table-sharded lookup (mi_slot_fm_fwd's operands: rows gathered out of a receive buffer of packed
 * {D embedding floats, first-order weight, 3 pad} rows at row slot[m, f]): gbuf fp32[nrows, D + 4] is that buffer's gradient,
 * row slot[m, f] receives the embedding part and g_y[m] at column D — mi_slot_fm_bwd in the epilogue.  Rows no sample
 * points at keep what the caller put there (zeros: they travel back to owners as padding). */
MI_API int mi_tail_dgrad_gemm_fm_slot(const float *DY, const float *Zl, int32_t ld, const float *mu, const float *al,
                                      const float *bz, const float *de, const float *W, int32_t ldw, float *gbuf,
                                      float *dz_out, int32_t M, int32_t N, int32_t K, const mi_tail_bn_bwd *sums,
                                      const float *emb, const float *emb_sum, const float *g_y, const int64_t *slot,
                                      int32_t D, void *stream);
MI_API int mi_tail_dropout_masks(const int64_t *seed, int32_t nlayers, const int64_t *salts, const float *ps,
                                 const int32_t *lds, uint8_t *const *bits, int32_t M, void *stream);
/* the same launch also zero-fills zero_buf[0 .. zero_floats) (a multiple of 4 floats, 16-byte aligned): the backward pass's
 * accumulation buffer (split-K weight gradients) without a fill launch of its own */
MI_API int mi_tail_dropout_masks_z(const int64_t *seed, int32_t nlayers, const int64_t *salts, const float *ps,
                                   const int32_t *lds, uint8_t *const *bits, int32_t M, float *zero_buf,
                                   int64_t zero_floats, void *stream);
MI_API int mi_tail_fwd_gemm(const float *X, int32_t ldx, const float *x_mu, const float *x_sc, const float *x_be,
                            float x_p, const uint8_t *x_keep, const float *W, int32_t ldw, float *Z, int32_t ldz,
                            float *part, float *a_out, int32_t M, int32_t N, int32_t K, void *stream);
MI_API int64_t mi_tail_part_elems(int32_t M, int32_t N);
MI_API int mi_tail_bn_finalize_fwd(const float *part, int32_t M, int32_t N, const float *gamma, const float *beta,
                                   const float *mean_offset, float *running_mean, float *running_var, float momentum,
                                   float eps, int64_t *num_batches_tracked, int64_t *seed_bump, float *mu, float *sc,
                                   float *be, float *rstd, void *stream);
/* mi_tail_bn_finalize_fwd with the work of mi_tail_dropout_masks_z riding along in extra workgroups of the same launch
 * (ride == NULL: the plain entry point).  The layer whose statistics are joined is the FIRST of the step, so every kernel
 * that reads keep bits comes later.  seed_bump must not point at ride->seed (MI_ERR_INVALID_ARG): a launch cannot both
 * draw from the seed and advance it; let a later finalize launch bump it.  Host struct, read at call time. */
/* The arguments of mi_tail_affine_consts (below) as a host struct: a second job a carrying launch can take. */
typedef struct mi_tail_affine_job {
  int32_t nlayers;                          /* <= 8 */
  const int32_t *widths;                    /* host [nlayers] */
  const float *const *gamma, *const *beta, *const *running_mean, *const *running_var, *const *bias;   /* host arrays of device pointers */
  const float *eps;                         /* host [nlayers] */
  float *const *mu, *const *sc, *const *be, *const *rstd;                                             /* host arrays of device pointers */
} mi_tail_affine_job;
typedef struct mi_tail_mask_ride {
  const int64_t *seed;          /* device */
  int32_t nlayers;              /* <= 8 */
  int32_t M;
  const int64_t *salts;         /* host [nlayers] */
  const float *ps;              /* host [nlayers] */
  const int32_t *lds;           /* host [nlayers] */
  uint8_t *const *bits;         /* host [nlayers] of device pointers (NULL where ps == 0) */
  float *zero_buf;              /* device, nullable */
  int64_t zero_floats;
  const mi_tail_affine_job *affine;   /* nullable: the constants of the tail's fixed-statistics layers computed by further extra
                                         workgroups (read by mi_gather_fm_fwd_ride only: an inference forward is the lookup, the
                                         products and the head — no launch for the constants) */
} mi_tail_mask_ride;
MI_API int mi_tail_bn_finalize_fwd_r(const float *part, int32_t M, int32_t N, const float *gamma, const float *beta,
                                     const float *mean_offset, float *running_mean, float *running_var, float momentum,
                                     float eps, int64_t *num_batches_tracked, int64_t *seed_bump, float *mu, float *sc,
                                     float *be, float *rstd, const mi_tail_mask_ride *ride, void *stream);
/* The gather + FM forward (mi_gather_fm_fwd_sum) carrying the same job in extra workgroups at the end of its grid: in
 * DeepFM's fused step (src/models/deepfm.py:79-105) it is the first kernel of the step — every reader of the keep bits
 * and every adder into zero_buf is launched later — so the tail needs no mask launch and no finalize launch to carry one.
 * ride == NULL: mi_gather_fm_fwd_sum.  offsets may be NULL (ids used as they are: the sharded step's slot lookup, W / w1 the
 * receive buffer and its column D, ldw = ldw1 = D + 4).  A gather form without the extra workgroups (D % 4, F > 64, unaligned) runs the job
 * as a launch of its own first.  The seed must be advanced by a LATER kernel. */
MI_API int mi_gather_fm_fwd_ride(const int64_t *idx, const int64_t *offsets, const float *W, int64_t ldw, const float *w1,
                                 int64_t ldw1, const float *bias, float *emb_out, float *yfm_out, int64_t *rows_out,
                                 float *sum_out, int64_t B, int32_t F, int32_t D, int64_t N, int32_t *err,
                                 const mi_tail_mask_ride *ride, void *stream);
MI_API int mi_tail_head_fwd(const float *Z, int32_t ldz, const float *mu, const float *sc, const float *be, float p,
                            const uint8_t *keep, const float *w, const float *b, const float *add, float *out,
                            int32_t M, int32_t N, void *stream);
MI_API int32_t mi_tail_head_blocks(int32_t M);
MI_API int mi_tail_head_bwd(const float *Z, int32_t ldz, const float *mu, const float *sc, const float *be, float p,
                            const uint8_t *keep, const float *g, const float *w, float *DY, float *part, float *wpart,
                            int32_t M, int32_t N, void *stream);
/* sum_reps > 0: part is fp32[sum_reps, N, 2] and wpart fp32[sum_reps, N + 4], both ZEROED by the caller; workgroup b ADDS
 * its sums into row b % sum_reps (float atomics) — a mi_tail_bn_bwd with nblk = nwblk = sum_reps then joins them in the next
 * product's prologue and the head level needs no finalize launch.  sum_reps = 0 is mi_tail_head_bwd. */
MI_API int mi_tail_head_bwd_s(const float *Z, int32_t ldz, const float *mu, const float *sc, const float *be, float p,
                              const uint8_t *keep, const float *g, const float *w, float *DY, float *part, float *wpart,
                              int32_t sum_reps, int32_t M, int32_t N, void *stream);
/* Head + criterion + head backward in ONE launch, for a step whose labels are known at forward time and whose criterion is
 * BCE-with-logits, reduction "mean" (the reference trainer's: src/trainer/deepfm.py:32,51 around the head of
 * src/models/deepfm.py:100-105).  Per row m: out[m] = the logit (mi_tail_head_fwd_m), its loss term, g[m] =
 * (sigmoid(out[m]) - y[m]) / M (mi_bce_logits_fwd's dx_unit), DY / part / wpart as mi_tail_head_bwd_s(g) writes them
 * (sum_reps > 0 rows, zeroed by the caller).  loss_ws: fp32[mi_tail_head_bce_ws_elems(sum_reps)], ZEROED by the caller;
 * loss_ws[0] is the loss afterwards (the rest are per-replica partial sums and arrival counts).  g and the sums are those
 * of the upstream gradient upstream[0] — a device scalar, the one the caller seeds the backward with (NULL: exactly 1; a
 * table-sharded step seeds 1 / world) — a backward that arrives with another gradient calls mi_tail_head_bwd_s (after
 * zeroing part / wpart again).  N <= 512.  stats as in mi_tail_head_fwd_m (NULL: mu / sc / be are read). */
MI_API int32_t mi_tail_head_bce_ws_elems(int32_t sum_reps);
MI_API int mi_tail_head_bce(const float *Z, int32_t ldz, const float *mu, const float *sc, const float *be, float p,
                            const uint8_t *keep, const float *w, const float *b, const float *add, const float *y,
                            float *out, float *g, float *DY, float *part, float *wpart, int32_t sum_reps, float *loss_ws,
                            int32_t M, int32_t N, const mi_tail_bn_fwd *stats, const float *upstream, void *stream);
MI_API int mi_tail_bn_finalize_bwd(const float *part, int32_t nblk, int32_t M, int32_t N, const float *gamma,
                                   const float *rstd, float *dgamma, float *dbeta, float *al, float *bz, float *de,
                                   const float *wpart, int32_t nwblk, float *dw, float *db, void *stream);
/* Layers that normalise with FIXED statistics or not at all — eval mode (model.eval(): BatchNorm1d on its running
 * statistics, src/models/deepfm.py:57-58) and use_batchnorm=False (DeepFM's default, src/models/deepfm.py:20,56) — run on
 * the same products: a = relu((z - mu) sc + be) with z = x W^T (the Linear bias stays out of the product) and
 *   BatchNorm in eval mode: rstd = 1/sqrt(running_var + eps), mu = running_mean - bias, sc = gamma rstd, be = beta
 *   no BatchNorm:           mu = 0, sc = 1, be = bias, rstd = 1
 * mi_tail_affine_consts writes these for up to 8 layers in ONE launch (host arrays of device pointers; running_mean[l] ==
 * NULL: layer l has no BatchNorm; gamma / beta / bias nullable per layer).
 * mi_tail_bn_finalize_bwd_a: affine != 0 -> al = gamma rstd, bz = de = 0 (dz = al dy), dgamma = rstd sum dy (z - mu),
 *   dbeta = sum dy, dbias (nullable) = al sum dy = the Linear bias's gradient; affine == 0 is mi_tail_bn_finalize_bwd.
 * mi_tail_head_fwd_m with a mi_tail_bn_fwd whose `part` is NULL joins nothing and only advances *seed_bump (nullable): how
 *   a step without any statistics to join moves its dropout seed on. */
MI_API int mi_tail_affine_consts(int32_t nlayers, const int32_t *widths, const float *const *gamma,
                                 const float *const *beta, const float *const *running_mean,
                                 const float *const *running_var, const float *const *bias, const float *eps,
                                 float *const *mu, float *const *sc, float *const *be, float *const *rstd, void *stream);
MI_API int mi_tail_bn_finalize_bwd_a(const float *part, int32_t nblk, int32_t M, int32_t N, const float *gamma,
                                     const float *rstd, float *dgamma, float *dbeta, float *al, float *bz, float *de,
                                     const float *wpart, int32_t nwblk, float *dw, float *db, int32_t affine,
                                     float *dbias, void *stream);
/* ... and with a second destination db2[0] (nullable) for the head bias's gradient (see mi_tail_bn_bwd.db2) */
MI_API int mi_tail_bn_finalize_bwd_b(const float *part, int32_t nblk, int32_t M, int32_t N, const float *gamma,
                                     const float *rstd, float *dgamma, float *dbeta, float *al, float *bz, float *de,
                                     const float *wpart, int32_t nwblk, float *dw, float *db, int32_t affine,
                                     float *dbias, float *db2, void *stream);
MI_API int mi_tail_dgrad_gemm(const float *DY, const float *Zl, int32_t ld, const float *mu, const float *al,
                              const float *bz, const float *de, const float *W, int32_t ldw, const float *pZ,
                              int32_t pld, const float *p_mu, const float *p_sc, const float *p_be, float p_p,
                              const uint8_t *p_keep, float *OUT, int32_t ldo, float *part, float *dz_out, int32_t M,
                              int32_t N, int32_t K, void *stream);
MI_API int32_t mi_tail_wgrad_splits(int32_t M, int32_t N, int32_t K);
MI_API int mi_tail_wgrad_gemm(const float *DY, const float *Zl, int32_t ld, const float *mu, const float *al,
                              const float *bz, const float *de, const float *pZ, int32_t pld, const float *p_mu,
                              const float *p_sc, const float *p_be, float p_p, const uint8_t *p_keep, float *slab,
                              float *dW, int32_t M, int32_t N, int32_t K, void *stream);
/* mi_tail_ring_plan: the schedule the products' main loop walks for a reduction of nst 32-wide slices, by host arithmetic
 * only (nothing launched, no GPU needed): the very control flow the kernels compile, with a recorder in place of the
 * loads, LDS writes and MFMAs.  role 0 = the producer waves, 1 = the consumer waves, 2 = the producer waves of the
 * products whose operands use general addressing (one loop over all phases; the same schedule).  partial: the range is no multiple
 * of 32 (its short slice is slice 0); dead_half: that slice ends inside its first half; pre: the consumers join
 * statistics in front of the first LDS write (one extra barrier).  events: cap records of 6 int32 each,
 *   (kind, slice, reg, slot, any, pos)   kind 0 ring barrier, 1 the extra barrier, 2 fetch (loads of `slice` into register
 *   stage `reg`), 3 finish (stage `reg` transformed and written to LDS slot `slot`), 4 fragment read (half `reg` of
 *   `slice` out of `slot`), 5 the MFMAs of fragment set `reg`;
 *   any = 1: the form that may meet a partial slice; pos: the slice's position in the range (x 32 = its first index).
 * *n = the number of events (also when it exceeds cap: nothing is written beyond cap). */
MI_API int mi_tail_ring_plan(int32_t nst, int32_t partial, int32_t dead_half, int32_t pre, int32_t role, int32_t *events,
                             int32_t cap, int32_t *n);

/* ---- a9: DHEmbedding's MLP (src/models/embeddings/dh_embedding.py:100-117,345-356) -----------------------------------
 * Per layer Linear -> Mish (use_bn 0) | Linear -> BatchNorm1d -> Mish (use_bn 2, the default) | Linear -> Mish ->
 * BatchNorm1d (use_bn 1, the LightGCN configs).  The contractions are mi_tail_fwd_gemm_s / mi_tail_dgrad_gemm_s on plain
 * operands (+ mi_gemm_f32_multi for dW); these three entry points are the column-wise element work between them, with
 * BatchNorm statistics / gradient column sums as per-64-row-tile partials in the layouts mi_tail_bn_finalize_fwd / _bwd join.
 *   mi_col_act_fwd: out[M,N] = ACT((in - mu[c]) sc[c] + be[c]), act 0 = identity, 1 = mish (x tanh(log1p(exp x)), as
 *     torch's CPU kernel); mu / sc / be nullable (0 / 1 / 0); in has row pitch ld; part (nullable,
 *     mi_tail_part_elems(M, N) floats) = (mean, M2) of `out` per tile and column.
 *   mi_col_act_bwd: dy = g ACT'(pre) (dy nullable: with act 0 it equals g), part[tile, N, 2] = (sum dy, sum dy (in - mu)).
 *   mi_bn_mish_bwd (use_bn 1: a = BatchNorm(m), m = mish(z + bias)): dz = (al g + bz (m - mu) + de) mish'(z + bias),
 *     part[tile, N, 2] = (sum dz, 0); al / bz / de as mi_tail_bn_finalize_bwd[_a] writes them. */
MI_API int mi_col_act_fwd(const float *in, int32_t ld, const float *mu, const float *sc, const float *be, int32_t act,
                          float *out, float *part, int32_t M, int32_t N, void *stream);
MI_API int mi_col_act_bwd(const float *g, const float *in, int32_t ld, const float *mu, const float *sc, const float *be,
                          int32_t act, float *dy, float *part, int32_t M, int32_t N, void *stream);
/* dz[M,N] = al dy + bz (z - mu) + de: the BatchNorm backward materialised (a layer whose input needs no gradient has no
 * input-gradient product that would compute it in its operand load) */
MI_API int mi_bn_dz(const float *dy, const float *z, int32_t ldz, const float *mu, const float *al, const float *bz,
                    const float *de, float *dz, int32_t M, int32_t N, void *stream);
MI_API int mi_bn_mish_bwd(const float *g, const float *m_act, const float *z, int32_t ldz, const float *bias,
                          const float *mu, const float *al, const float *bz, const float *de, float *dz, float *part,
                          int32_t M, int32_t N, void *stream);

/* ---- §8e: the sharded lookup's collectives on the CALLER's stream (recsys-benchmark_amd/csrc/comm.hip) ------------------
 * No reference counterpart.  The library owns its own RCCL communicator (resolved with dlopen at first use: every entry
 * point returns MI_ERR_UNSUPPORTED when no librccl can be loaded) so that the all-to-alls and the all-reduce are enqueued
 * on the stream the kernels run on — torch.distributed's process-group stream costs two event hand-offs per collective.
 * mi_comm_unique_id: HOST buffer of 128 bytes, filled on one rank and distributed by the caller.  mi_comm_init is
 * collective (every rank calls it with the same id; the current HIP device is the rank's GPU).  mi_comm_all_to_all:
 * recv[p*bytes .. ) <- rank p's send[me*bytes .. ) for every peer p (ncclGroupStart / Send / Recv / GroupEnd).
 * mi_comm_all_reduce_sum_f32: in place.  mi_comm_abort: for a communicator whose enqueued work does not complete
 * (ncclCommAbort: stops its kernels, frees it without waiting); mi_comm_destroy is the orderly end. */
MI_API int mi_comm_available(void);   /* MI_OK when librccl could be loaded in this process; agree on it before mi_comm_init */
MI_API int mi_comm_unique_id(char *id128);
MI_API int mi_comm_init(const char *id128, int32_t world, int32_t rank, void **comm_out);
MI_API int mi_comm_destroy(void *comm);
MI_API int mi_comm_abort(void *comm);
MI_API int mi_comm_all_to_all(void *comm, const void *send, void *recv, int64_t bytes_per_peer, void *stream);
MI_API int mi_comm_all_reduce_sum_f32(void *comm, float *buf, int64_t count, void *stream);

/* ---- global magnitude pruning (src/utils.py:8-34 `prune`; scripts/lightgcn/run_mag_prune.py:55-81 and
 * scripts/cf_train/run_mag_prune.py:55-97 `get_v` call it once per table and per search candidate) ------------------
 * One table W fp32[N, D] (row stride ldw), k elements to prune, floor m kept per row.  key(w) = bits(|w|) (+0.0 and -0.0
 * share key 0; inf is the largest ordinary key; NaN is outside the contract: its key sorts above inf and nothing else is
 * promised for it).  The m largest keys of a row are protected (equal keys: lower column first); the k smallest
 * unprotected keys of the table become +0.0 (equal keys at the cut: lower flat index i * D + j first); every other
 * element is copied bit for bit.  The reference's topk / argsort / two index writes are a k-th element selection here: a
 * row cut (m > 0 only; 8 bytes per row), three histogram passes of a most-significant-first radix select (integer
 * adds only: the result does not depend on the order of arrival), one apply pass — and, when the cut falls inside a run
 * of equal keys (to be expected at hundreds of millions of fp32 values), one more read of the table that counts the
 * equals per chunk, so that the apply pass can take the first ones in flat order: five table passes (six with a floor)
 * in the plain case, one more in that case.  Nothing is read back to the host.
 *   mi_mag_prune: out == NULL selects only (the workspace then feeds mi_mag_csr_*); out may alias W (the reference
 *     prunes in place).  workspace: mi_mag_prune_workspace_bytes(N) bytes, no state between calls (zeroed by a memset
 *     node).  N * D <= 2^32 - 1, m <= D and N * m + k <= N * D, else MI_ERR_INVALID_ARG (beyond that bound the reference
 *     prunes its own `inf` markers in sort order); D <= 1024, else MI_ERR_UNSUPPORTED.
 *   mi_mag_prune_result: copies {T, elements with key < T, elements with key == T, equals of T that are pruned}
 *     (unprotected elements only) from the workspace of a finished mi_mag_prune to result4 (device uint32[4]).
 * CSR of the pruned table (what PrunedEmbedding serves, scripts/lightgcn/infer_lightgcn.py:224-247) without the dense
 * pruned table being written; exact zeros of either sign are dropped, as Tensor.to_sparse_csr() drops them:
 *   mi_mag_csr_count: crow int64[N + 1] (crow[N] = number of stored elements; the caller sizes col / values from it);
 *   mi_mag_csr_fill:  col int64 (ascending inside a row) and values fp32, by ballot / popcount compaction.
 *   prune_ws: the workspace of a finished mi_mag_prune with the same W, N, D, m — or NULL (then m == 0): W is taken as
 *   it is, a dense-to-CSR conversion.  csr_ws: mi_mag_csr_workspace_bytes(N) bytes, shared by count and fill.        */
MI_API int64_t mi_mag_prune_workspace_bytes(int64_t N);
MI_API int mi_mag_prune(const float *W, int64_t ldw, float *out, int64_t ldo, int64_t N, int32_t D, int64_t k,
                        int32_t m, void *workspace, void *stream);
MI_API int mi_mag_prune_result(const void *workspace, uint32_t *result4, void *stream);
MI_API int64_t mi_mag_csr_workspace_bytes(int64_t N);
MI_API int mi_mag_csr_count(const float *W, int64_t ldw, int64_t N, int32_t D, const void *prune_ws, int32_t m,
                            void *csr_ws, int64_t *crow, void *stream);
MI_API int mi_mag_csr_fill(const float *W, int64_t ldw, int64_t N, int32_t D, const void *prune_ws, int32_t m,
                           const void *csr_ws, const int64_t *crow, int64_t *col, float *values, void *stream);

/* ---- device-resident CF data (src/dataset/cf_graph_dataset.py:50-168 `CFGraphDataset`; src/metrics.py:70-108
 * `get_ndcg_recall`) ------------------------------------------------------------------------------------------------
 * mi_cf_sample_triples: samples [first, first + n) of an epoch in one launch, one thread per sample.
 *   pair_user / pair_item int64[P]: the stored interactions, duplicates kept; pair_crow int64[U + 1]: user u's stored
 *     list is pair_item[pair_crow[u] .. pair_crow[u + 1]) (read in uniform mode only; pair_user in popularity mode only).
 *   pos_crow int64[U + 1] / pos_col int32[pos_nnz]: the membership CSR, every row DISTINCT and ASCENDING.
 *   mode MI_CF_SAMPLE_POPULARITY: sample i is pair order[i - first] (order int64[n]; NULL: pair i).
 *   mode MI_CF_SAMPLE_UNIFORM: sample i belongs to user i / per_user_num; its positive is a uniformly drawn entry of the
 *     user's STORED list (a duplicated interaction is twice as likely, as random.choice over the reference's list).
 *   The K negatives of a sample are uniform over the items outside the user's pos_col row and pairwise distinct — the
 *     law of the reference's rejection loop, drawn without a loop: rank among the remaining non-positives, bumped past
 *     the earlier picks, mapped to the item by one binary search (<= K * ceil(log2(deg + 1)) reads of pos_col).
 *   Draws (all arithmetic modulo 2^64; mix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) *
 *     0x94D049BB133111EB; z ^ z >> 31):  base = mix64(seed + G * (epoch + 1));  key(i) = mix64(base + S * (i + 1));
 *     bits(i, d) = mix64(key(i) + G * (d + 1)) with G = 0x9E3779B97F4A7C15, S = 0xD1B54A32D192ED03, i the index in the
 *     epoch, d = 0 for the positive and 1 + t for negative t;  value = (bits * range) >> 64, range = the stored list's
 *     length resp. num_items - deg - t.  That reduction is biased by at most range / 2^64 per value; accepted.
 *     Stateless: any sub-range of an epoch gives the bits the whole epoch gives there.
 *   Outputs: users int64[n], pos int64[n], neg int64[K, n] (K-major: each of the K negative vectors is contiguous).
 *   A sample whose pair index or user is out of range, whose user has no stored item, or whose user has
 *     deg + K > num_items writes -1 to users, pos and its K negatives, ORs MI_IDX_OUT_OF_RANGE into *err and reads
 *     nothing else.  K > MI_CF_MAX_NEG or num_items >= 2^31: MI_ERR_UNSUPPORTED.
 * mi_ndcg_recall_rows: row i of pred int64[n, ld] (its first k columns; k <= ld) against the truth row of users[i] in
 *   crow int64[U + 1] / col int64[nnz] (rows distinct and ascending): relevant_j = pred[i, j] in the row, dcg = sum over
 *   ascending j of relevant_j * weight[j], length = min(row length, k), ndcg[i] = dcg / ideal[length - 1],
 *   recall[i] = hits / length, all float64.  weight double[k] = 1 / log2(j + 2) and ideal double[k] = its running sum
 *   come from the caller, so that host and device use the same constants to the last bit.  An empty truth row gives
 *   NaN for both (the reference's 0 / 0); users[i] outside [0, U) gives NaN and ORs MI_IDX_OUT_OF_RANGE into *err.   */
#define MI_CF_SAMPLE_UNIFORM 0
#define MI_CF_SAMPLE_POPULARITY 1
#define MI_CF_MAX_NEG 32
MI_API int mi_cf_sample_triples(const int64_t *pair_user, const int64_t *pair_item, const int64_t *pair_crow, int64_t P,
                                const int64_t *pos_crow, const int32_t *pos_col, int64_t pos_nnz, int64_t U,
                                int64_t num_items, int32_t mode, int64_t per_user_num, int32_t K, const int64_t *order,
                                int64_t seed, int64_t epoch, int64_t first, int64_t n, int64_t *users, int64_t *pos,
                                int64_t *neg, int *err, void *stream);
MI_API int mi_ndcg_recall_rows(const int64_t *pred, int64_t ld, const int64_t *users, int64_t n, int32_t k,
                               const int64_t *crow, const int64_t *col, int64_t U, int64_t nnz, const double *weight,
                               const double *ideal, double *ndcg, double *recall, int *err, void *stream);

/* ---- CTR validation metric (src/trainer/deepfm.py:96-139 `validate_epoch`: sklearn's roc_auc_score and log_loss over
 * the whole validation set) ---------------------------------------------------------------------------------------------
 * mi_binary_auc: the area under the ROC curve of score fp32[n] against label uint8[n] as roc_auc_score computes it for
 *   binary labels — the Mann-Whitney statistic, equal scores sharing their average rank — as an integer:
 *     S = sum over the groups g of equal score of pos_g * (2 * neg_below_g + neg_g),   AUC = S / (2 P N).
 *   key(score) = a monotone map of the float32 bits with -0.0 folded onto +0.0 (sklearn ties them); +-inf are the largest
 *   and smallest ordinary keys; NaN is outside the order.  The negatives' keys are sorted by a stable radix sort (four
 *   8-bit digits, least significant first; a positive travels as the key 0xffffffff, so the sorted negatives are the
 *   first N words), then every positive adds its lower- and its upper-bound position among them.  Integer adds only up to
 *   the one division: the record does not depend on the order of arrival and is the same bit for bit on every run.
 *   Nothing is read back, nothing is allocated: 4 * 3 + 2 launches and one memset node on `stream`.
 *   result: a device record of 48 bytes, 8-byte aligned —
 *     uint64 S | int64 P (labels == 1) | int64 N (labels == 0) | int64 NaN scores | int64 labels outside {0, 1} | double auc.
 *     auc = S / (2 P N) computed on the device; NaN when a score is NaN (S then says nothing), or P == 0, or N == 0.
 *     A label outside {0, 1} is counted and belongs to neither class.
 *   workspace: mi_binary_auc_workspace_bytes(n) bytes (about 9 n; 0 for n == 0, NULL is then fine), 16-byte aligned; no
 *     state between calls and nothing in it needs zeroing (the record is zeroed by the memset node).
 *   n <= 2^31 - 1, else MI_ERR_UNSUPPORTED (S < 2^63 follows); n == 0: MI_OK, counts zero, auc NaN.
 * mi_ctr_metric_append: one launch per validation batch.  logits fp32[b] are copied to score_buf[at, at + b) (fp32[cap]),
 *   the labels (int64[b] or fp32[b] by label_kind) to label_buf[at, at + b) (uint8[cap]) as 1, 0, or 2 for any other value,
 *   and *loss_sum (a device double) grows by the batch's BCE-with-logits sum: each term
 *   max(x, 0) - x * y + log1p(exp(-|x|)) in float64 from the float32 logit, summed in float64 in a fixed order (per-thread
 *   strides, a fixed tree per workgroup, the workgroups' partials joined in index order by the last one to arrive):
 *   reruns give the same bits.  The sigmoid is NOT applied: the caller ranks torch.sigmoid of the whole buffer, whose
 *   float32 rounding decides the ties.
 *   workspace: mi_ctr_metric_append_workspace_bytes() bytes, 8-byte aligned, ZERO before its first use; every launch
 *     leaves it ready for the next (the arrival ticket is re-armed).  Launches that share one must run one after another.
 *   at + b > cap (or a negative size, or a label_kind that is neither): MI_ERR_INVALID_ARG.  b == 0: MI_OK, no launch.   */
#define MI_CTR_LABEL_INT64 0
#define MI_CTR_LABEL_FLOAT32 1
MI_API int64_t mi_binary_auc_workspace_bytes(int64_t n);
MI_API int mi_binary_auc(const float *score, const uint8_t *label, int64_t n, void *workspace, void *result, void *stream);
MI_API int64_t mi_ctr_metric_append_workspace_bytes(void);
MI_API int mi_ctr_metric_append(const float *logits, const void *labels, int32_t label_kind, int64_t b, int64_t at,
                                float *score_buf, uint8_t *label_buf, int64_t cap, double *loss_sum, void *workspace,
                                void *stream);

/* ---- device-resident CTR data (src/dataset/criteo/criteo_torchfm.py: `__get_feat_mapper`, `__yield_buffer`,
 * `__getitems__` and the DataLoader's collate) --------------------------------------------------------------------------
 * mi_ctr_vocab_field: the vocabulary rule over ONE column whose keys the caller has sorted.
 *   sorted_keys int64[n] ascending, perm int64[n]: sorted_keys[i] is the key of row perm[i] (a stable sort's output).
 *   A key seen at least `threshold` (>= 1) times is kept; kept keys get the ids 0 .. kept-1 in ASCENDING KEY ORDER, every
 *   other key gets the id `kept`:  out[perm[i] * stride] = id of sorted_keys[i]  (out uint32, `stride` in elements: a
 *   column of the [n, 1 + F] record array has stride 1 + F),  *num_kept = kept  (a device int64; the field's dimension is
 *   kept + 1).  The reference numbers the kept features in set-iteration order; this rule agrees with it up to a renaming
 *   of the kept ids per field, and exactly on the field's dimension and on which positions are out-of-vocabulary.
 *   Three launches on `stream` (mark run heads and kept runs; scan the tiles' counts; scatter), integer adds only, plain
 *   stores: reruns give the same bits.  Nothing is read back.  A perm entry outside [0, n) writes nothing and ORs
 *   MI_IDX_OUT_OF_RANGE into *err.
 *   workspace: mi_ctr_vocab_workspace_bytes(n) bytes (about n + n / 64), 16-byte aligned, no state between calls, nothing
 *   in it needs zeroing.  n == 0: *num_kept = 0.  n > 2^31 - 1 or stride > 2^31 - 1: MI_ERR_UNSUPPORTED.
 * mi_ctr_batch: samples [first, first + count) of epoch `epoch` in ONE launch, one lane per output element.
 *   records uint32[n_records, 1 + F]: column 0 the label, column 1 + f field f's id.  index int64[n] (NULL: n must equal
 *   n_records): the record rows the epoch runs over.  The sample at epoch position j is record row index[p(j)] (p(j)
 *   without an index);  x[s, f] = (int64) records[row, 1 + f],  y[s] = (float) records[row, 0]  for s = j - first;
 *   x int64[count, F], y float[count].  p is the identity when shuffle == 0, else this bijection of [0, n) (all
 *   arithmetic modulo 2^64; mix64 as under mi_cf_sample_triples):
 *     mix64      = the splitmix64 finaliser of cf_data.hip; kGold = 0x9E3779B97F4A7C15, kSalt = 0xD1B54A32D192ED03
 *     bits       = max(2, bit_length(n - 1));  k = (bits + 1) / 2;  mask = (1 << k) - 1
 *     base       = mix64(seed + kGold * (epoch + 1))                       (mod 2^64 throughout)
 *     K[r]       = mix64(base + kSalt * (r + 1)),  r = 0..5
 *     step(x):   L = x >> k; R = x & mask; six times: (L, R) = (R, L ^ (mix64(K[r] + R) & mask)); return (L << k) | R
 *     p(j):      x = j; do x = step(x) while x >= n
 *   step is a Feistel network, hence a bijection of [0, 2^(2k)), and 2^(2k) < 4 n for n >= 2; walking until the value is
 *   below n restricts it to a bijection of [0, n) (the cycle through j returns to j at the latest, so the walk ends).
 *   Stateless: a sub-range of an epoch holds the bits the whole epoch holds there, for any grid.  A cheap keyed shuffle
 *   for SGD; no cryptographic claim.
 *   A row outside [0, n_records) writes -1 to its x and NaN to its y and ORs MI_IDX_OUT_OF_RANGE into *err.
 *   first + count > n (or a negative size, or F < 1): MI_ERR_INVALID_ARG.  count == 0: MI_OK, no launch.                */
MI_API int64_t mi_ctr_vocab_workspace_bytes(int64_t n);
MI_API int mi_ctr_vocab_field(const int64_t *sorted_keys, const int64_t *perm, int64_t n, int64_t threshold, uint32_t *out,
                              int64_t stride, int64_t *num_kept, void *workspace, int *err, void *stream);
MI_API int mi_ctr_batch(const uint32_t *records, int64_t n_records, int32_t F, const int64_t *index, int64_t n,
                        int32_t shuffle, int64_t seed, int64_t epoch, int64_t first, int64_t count, int64_t *x, float *y,
                        int *err, void *stream);

/* ---- the Criteo text format on the device (src/dataset/criteo/criteo_torchfm.py: `__yield_buffer`,
 * `convert_numeric_feature`; the host reader is `read_criteo_text` of ctr_data.py) ---------------------------------------
 * A chunk of the file's bytes in; keys int64[n, F], labels uint8[n] and 0-based line numbers int64[n] of the n kept lines
 * out, F = n_int + n_cat, equal element for element to the host reader's on every file both accept.  The grammar, which
 * the device enforces strictly:
 *   lines     a line is a run of bytes ended by '\n'; a non-empty run after the file's last '\n' is a line too.  Lines are
 *             numbered from 0 over the whole file, skipped ones included.  A line whose number of '\t' bytes is not F is
 *             skipped and its content ignored.  A '\r' byte anywhere is refused.
 *   label     column 0: exactly the byte '0' or '1'.
 *   integer   columns 1 .. n_int: empty gives the key -2^63; otherwise an optional '-' and 1 to 18 decimal digits (leading
 *             zeros and "-0" included) giving v; the key is v - 2 for v <= 2, else the number of entries <= v of
 *             `thresholds`, int64[n_thresholds] ascending.  With thresholds[k - 1] = the smallest v whose
 *             int(math.log(v) ** 2) is at least k (ctr_data.numeric_thresholds builds it from the host reader's own
 *             function) that number IS int(math.log(v) ** 2): no logarithm is evaluated on the device.
 *   category  columns n_int + 1 .. F: empty gives the key -1; otherwise 1 to 15 hexadecimal digits of either case.
 *   refused   anything else in a kept line ("+5", a space, "1_0", "0x1f", 19 digits, 16 hex digits, a label "2", an
 *             empty label ...).  A refusal lowers *err_record (a device uint64, all ones when there is none) to
 *             (line number << 16) | column by a 64-bit atomic minimum: the LOWEST offending (line, column) stays, whatever
 *             the order of arrival.  Outputs of a refused field are zero; the caller discards the chunk.
 * mi_ctr_text_index: six launches on `stream` (count separators per 4096-byte tile; scan; scatter their positions in order;
 *   count the lines with exactly F tabs per 256-line tile; scan; number the kept lines).
 *   text uint8[nbytes], any alignment, nbytes <= 2^31 - 1 (else MI_ERR_UNSUPPORTED).  is_final != 0: the chunk ends the
 *   file, and a last line without '\n' counts; is_final == 0: the bytes after the chunk's last '\n' belong to the next
 *   chunk and are ignored (a '\r' among them too).  first_line_no: the file's line number of the chunk's first line.
 *   record int64[3] (device) = {lines in the chunk, kept lines, bytes consumed (the offset after the last line)}.
 *   A '\r' in any line of the chunk, kept or not, lowers *err_record to (its line << 16) | min(its column, 65535).
 *   workspace: mi_ctr_text_workspace_bytes(nbytes, n_int, n_cat) bytes (about 8 nbytes), 16-byte aligned, nothing in it
 *   needs zeroing; mi_ctr_text_parse reads what this call left in it.
 * mi_ctr_text_parse: ONE launch, one lane per (kept line, column), each converting its own field (at most 19 bytes) from
 *   the two separator positions around it; the same text, nbytes, n_int, n_cat, first_line_no and workspace as the
 *   mi_ctr_text_index call before it, n_kept = record[1].  Every element of keys_out[n_kept, F], labels_out[n_kept] and
 *   line_no_out[n_kept] is written, nothing beyond.  n_kept == 0: MI_OK, no launch.
 * Integer arithmetic and plain stores; no arrival order enters any value.  The only atomics are on the error path:
 * *err_record, the workspace's own minimum over the '\r' bytes, and MI_IDX_OUT_OF_RANGE ORed into *err (NULL is fine) by
 * a workspace subscript that fails its check, which a workspace left by mi_ctr_text_index never does.  Every byte
 * subscript is checked against nbytes before it is used.  n_int + n_cat > 65534 or first_line_no > 2^46:
 * MI_ERR_UNSUPPORTED.                                                                                                       */
MI_API int64_t mi_ctr_text_workspace_bytes(int64_t nbytes, int32_t n_int, int32_t n_cat);
MI_API int mi_ctr_text_index(const uint8_t *text, int64_t nbytes, int32_t is_final, int32_t n_int, int32_t n_cat,
                             int64_t first_line_no, void *workspace, int64_t *record, uint64_t *err_record, int *err,
                             void *stream);
MI_API int mi_ctr_text_parse(const uint8_t *text, int64_t nbytes, int32_t n_int, int32_t n_cat, const void *workspace,
                             int64_t n_kept, int64_t first_line_no, const int64_t *thresholds, int32_t n_thresholds,
                             int64_t *keys_out, uint8_t *labels_out, int64_t *line_no_out, uint64_t *err_record, int *err,
                             void *stream);

/* ---- delimited text by a column spec: Avazu and KDD 2012 track 2 on the device (src/dataset/avazu/avazu_fm.py,
 * avazu_on_ram.py `_create_binary`, avazu/utils.py, src/dataset/kdd/kdd_dataset.py; the host readers are `read_avazu_text`
 * and `read_kdd_text` of ctr_data.py) ---------------------------------------------------------------------------------------
 * A chunk of the file's bytes in; keys int64[n, F_out], labels uint8[n] and 0-based line numbers int64[n] of the n kept
 * lines out, equal element for element to the host reader's on every file both accept.  The index kernels are the ones of
 * the Criteo reader above (ONE body), given the separator byte and the header count.  The grammar, enforced strictly:
 *   lines     a line is a run of bytes ended by '\n'; a non-empty run after the file's last '\n' is a line too.  The first
 *             n_header (0 or 1) lines of THE CHUNK are a header: never kept and never counted (the caller passes 1 for a
 *             file's first chunk only).  The other lines are numbered from first_line_no, skipped ones included: numbering
 *             starts at the line after the header.  A line is kept when it has exactly n_cols - 1 bytes equal to sep_byte
 *             (',' or '\t'; any byte but 0, '\n' and '\r' is taken).  A skipped line's content is ignored.  A '\r' byte
 *             anywhere, the header included, is refused (one in the header is named as line first_line_no).
 *   columns   spec int32[n_cols] on the device: entry c = kind | (output column << 8) for file column c.  The key kinds
 *             (TOKEN8, DEC64, TIME) must name the output columns 0 .. F - 1 once each, F being their number; other kinds'
 *             output column is ignored.  One column should be a label kind and at most one a TIME.
 *   SKIP         anything without '\r'; nothing of the field is read.
 *   LABEL01      exactly the byte '0' or '1': the label.
 *   LABEL_COUNT  1 to 18 decimal digits, no sign (leading zeros are fine): label = (value >= 1).
 *   TOKEN8       0 to 8 bytes, each in 0x21 .. 0x7E.  The key is the bytes big-endian in a 64-bit word, zero-padded at the
 *                low end, as int64; an empty field gives key 0.  Injective on accepted strings because NUL is not accepted.
 *                Refused: longer than 8 bytes, or any other byte (a space, 0x7F, 0x80 .., NUL).
 *   DEC64        1 to 20 decimal digits, no sign, no leading zero except "0" itself, value <= 2^64 - 1: the key is the
 *                value's 64-bit pattern as int64.  Refused: an empty field, '+', a leading zero, 21 or more digits, a value
 *                above 2^64 - 1.
 *   TIME         with derive_time == 0 a plain TOKEN8.  With derive_time != 0 (and a TIME column in the spec, F_out = F + 3,
 *                else F_out = F): exactly 8 digits yymmddHH; the key is the TOKEN8 key of those bytes, and three derived
 *                keys go to output columns F, F + 1 and F + 2: hour, weekday with Monday as 0, and weekday >= 5.  The year
 *                is 2000 + yy for yy <= 68, else 1900 + yy (Python's %y).  The weekday comes from a days-from-civil
 *                computation in integers.  Month 1 to 12, a day valid for the month with leap years, and hour 0 to 23;
 *                otherwise, or when the field is not exactly 8 digits, the field is refused.
 *   refused   a field longer than 20 bytes in any column but a SKIP one, an unknown kind, and everything the kinds refuse.
 *             A refusal lowers *err_record to (line number << 16) | file column by a 64-bit atomic minimum, exactly as the
 *             Criteo reader does: the LOWEST offending (line, column) stays.  Outputs of a refused field are zero.
 * mi_ctr_table_index: the six launches of mi_ctr_text_index; record int64[3] = {lines counted (the header is not), kept
 *   lines, bytes consumed}.  workspace: mi_ctr_table_workspace_bytes(nbytes, n_cols) bytes (about 8 nbytes), 16-byte
 *   aligned, nothing in it needs zeroing.  n_cols in [1, 256] (above: MI_ERR_UNSUPPORTED; 0 from the size function).
 * mi_ctr_table_parse: ONE launch, one lane per (kept line, file column): the lane reads the two separator positions around
 *   its field, loads at most 20 bytes with predicated loads that do not depend on one another, and converts them; the same
 *   text, nbytes, sep_byte, n_cols, first_line_no and workspace as the index call before it (the header count is read from
 *   the workspace), n_kept = record[1].  Every element of keys_out[n_kept, F_out], labels_out[n_kept] and
 *   line_no_out[n_kept] is written (by a spec as described above), nothing beyond.  n_kept == 0: MI_OK, no launch.
 * Integer arithmetic and plain vector stores; no arrival order enters any value, so reruns give the same bits.  Atomics
 * appear only on the error path: *err_record and MI_IDX_OUT_OF_RANGE ORed into *err (NULL is fine) by a workspace
 * subscript or an output column that fails its check.  Every byte and workspace subscript is checked before use.        */
#define MI_CTR_COL_SKIP 0
#define MI_CTR_COL_LABEL01 1
#define MI_CTR_COL_LABEL_COUNT 2
#define MI_CTR_COL_TOKEN8 3
#define MI_CTR_COL_DEC64 4
#define MI_CTR_COL_TIME 5
MI_API int64_t mi_ctr_table_workspace_bytes(int64_t nbytes, int32_t n_cols);
MI_API int mi_ctr_table_index(const uint8_t *text, int64_t nbytes, int32_t is_final, int32_t sep_byte, int32_t n_cols,
                              int32_t n_header, int64_t first_line_no, void *workspace, int64_t *record,
                              uint64_t *err_record, int *err, void *stream);
MI_API int mi_ctr_table_parse(const uint8_t *text, int64_t nbytes, int32_t sep_byte, int32_t n_cols, const int32_t *spec,
                              int32_t derive_time, const void *workspace, int64_t n_kept, int64_t first_line_no,
                              int64_t *keys_out, uint8_t *labels_out, int64_t *line_no_out, uint64_t *err_record, int *err,
                              void *stream);

/* ---- profiling ring (bench.py's per-kernel HIP-event timing) ---------------
 * When enabled every launcher brackets its kernel with a hipEvent pair on the
 * launch stream.  Not for use under graph capture.
 */
MI_API int mi_prof_enable(int32_t capacity); /* >0: (re)arm with that many records; 0: disable */
MI_API int mi_prof_count(void);
/* An empty kernel of the given geometry through the same launcher / timing ring ("empty"): the duration the
 * per-dispatch clock reads for a launch that does nothing — the floor under every kernel time it reports. */
MI_API int mi_prof_empty_launch(int32_t grid, int32_t block, void *stream);
/* Synchronises on record i's stop event; name_out is a host buffer of >=64 bytes. */
MI_API int mi_prof_read(int32_t i, char *name_out, float *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_RECSYS_H */
