// probe_mfma.hip — issue rate of v_mfma_f32_16x16x4_f32 at one wave per SIMD, with and without the LDS fragment reads of
// tail_gemm.hpp's stage (tools/, not product code).  Cycles by s_memtime inside the kernel.
// Second part (the exact column cover of tail_gemm.hpp): v_mfma_f32_4x4x1_16b_f32 — (a) its issue interval on four
// independent accumulators and its dependent interval on one, (b) the consumers' half-slice streams 28 x 16x16x4 against
// 24 x 16x16x4 + 4 (or 8, 12) x 4x4x1 interleaved j-major, (c) its operand / result lane maps against a scalar fmaf loop.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include <algorithm>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)
typedef float floatx4 __attribute__((ext_vector_type(4)));
constexpr int NSUB = 7, BK = 32;
__device__ __forceinline__ int kc_off(int row, int chunk) { return row * BK + ((chunk ^ ((row >> 1) & 7)) << 2); }

// MODE 0: operands from registers; 1: 16 ds_read_b128 per stage (swizzled, as the product); 2: same, un-swizzled layout
template <int MODE, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_mfma(float *out, uint64_t *cyc, int stages) {
  __shared__ __attribute__((aligned(16))) float lds[2 * (64 + 112) * BK];
  for (int i = threadIdx.x; i < 2 * (64 + 112) * BK; i += WAVES * 64) lds[i] = (float)(i % 13) * 0.01f;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) & 3, r = lane & 15, g = lane >> 4;
  floatx4 acc[NSUB];
#pragma unroll
  for (int s = 0; s < NSUB; ++s) acc[s] = floatx4{0.f, 0.f, 0.f, 0.f};
  float4 b[2], a[2][NSUB];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    b[h] = make_float4(lane * 0.001f, 0.5f, 0.25f, 0.125f);
#pragma unroll
    for (int s = 0; s < NSUB; ++s) a[h][s] = make_float4(s * 0.01f + lane * 0.002f, 0.3f, 0.2f, 0.1f);
  }
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  for (int st = 0; st < stages; ++st) {
    const float *Rt = lds + (st & 1) * (64 + 112) * BK, *Ct = Rt + 64 * BK;
    if (MODE != 0) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int rr = wave * 16 + r;
        b[h] = *reinterpret_cast<const float4 *>(Rt + (MODE == 1 ? kc_off(rr, 4 * h + g) : rr * BK + (4 * h + g) * 4));
#pragma unroll
        for (int s = 0; s < NSUB; ++s) {
          const int cr = s * 16 + r;
          a[h][s] = *reinterpret_cast<const float4 *>(Ct + (MODE == 1 ? kc_off(cr, 4 * h + g) : cr * BK + (4 * h + g) * 4));
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int s = 0; s < NSUB; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][s].x, b[h].x, acc[s], 0, 0, 0);
#pragma unroll
      for (int s = 0; s < NSUB; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][s].y, b[h].y, acc[s], 0, 0, 0);
#pragma unroll
      for (int s = 0; s < NSUB; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][s].z, b[h].z, acc[s], 0, 0, 0);
#pragma unroll
      for (int s = 0; s < NSUB; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[h][s].w, b[h].w, acc[s], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (MODE == 3) __syncthreads();
  }
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NSUB; ++k) s += acc[k][0] + acc[k][1] + acc[k][2] + acc[k][3];
  out[blockIdx.x * WAVES * 64 + threadIdx.x] = s;
  if (lane == 0) cyc[blockIdx.x * WAVES + (threadIdx.x >> 6)] = t1 - t0;
}
template <int MODE, int WAVES>
void run(const char *name, int grid, int stages) {
  float *o; uint64_t *c;
  CK(hipMalloc(&o, grid * WAVES * 64 * 4)); CK(hipMalloc(&c, grid * WAVES * 8));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  k_mfma<MODE, WAVES><<<grid, WAVES * 64>>>(o, c, stages);
  CK(hipEventRecord(e0));
  k_mfma<MODE, WAVES><<<grid, WAVES * 64>>>(o, c, stages);
  CK(hipEventRecord(e1));
  CK(hipDeviceSynchronize());
  float ms; CK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<uint64_t> h(grid * WAVES);
  CK(hipMemcpy(h.data(), c, grid * WAVES * 8, hipMemcpyDeviceToHost));
  std::sort(h.begin(), h.end());
  const double per = (double)h[h.size() / 2] / (stages * 56.0);
  printf("%-44s grid %3d waves %d: median %6.1f s_memtime ticks per MFMA (56 per stage), kernel %.1f us -> %.1f TFLOP/s\n", name, grid, WAVES, per, ms * 1e3,
         (double)grid * WAVES * stages * 56 * 2048.0 / (ms * 1e-3) / 1e12);
  CK(hipFree(o)); CK(hipFree(c));
}
// The timed streams are volatile asm with VGPR accumulators (the product's kernels hold theirs in VGPRs too): the order is
// the order written, and hipcc adds nothing between the instructions (the builtins drew accumulator copies and re-formed
// operands into the loops).
__device__ __forceinline__ void mfma16(floatx4 &acc, float a, float b) {
  asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma4(floatx4 &acc, float a, float b) {
  asm volatile("v_mfma_f32_4x4x1_16b_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
// ---- (a) v_mfma_f32_4x4x1_16b_f32 back to back: NACC independent accumulators (1 = the dependent chain) ----------------
template <int NACC>
__global__ __launch_bounds__(256) void k_issue4(float *out, uint64_t *cyc, int iters) {
  const int lane = threadIdx.x & 63;
  floatx4 acc[NACC];
#pragma unroll
  for (int s = 0; s < NACC; ++s) acc[s] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float a = out[lane], b = out[64 + lane];
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 16; ++u)
#pragma unroll
      for (int s = 0; s < NACC; ++s) mfma4(acc[s], a, b);
  }
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NACC; ++k) s += acc[k][0] + acc[k][1] + acc[k][2] + acc[k][3];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (lane == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
}
// ---- (b) one half slice of the consumers: NF full sub-tiles on 16x16x4 + NG four-column groups on 4x4x1, j-major ------
// SPREAD: group q goes behind full sub-tile (q + 1) NF / NG - 1 instead of all groups behind the last one
template <int NF, int NG, bool SPREAD = false>
__global__ __launch_bounds__(256) void k_half(float *out, uint64_t *cyc, int halves) {
  const int lane = threadIdx.x & 63;
  floatx4 acc[NF], gacc[NG > 0 ? NG : 1];
#pragma unroll
  for (int s = 0; s < NF; ++s) acc[s] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < (NG > 0 ? NG : 1); ++s) gacc[s] = floatx4{0.f, 0.f, 0.f, 0.f};
  float a[NF + NG][4], b[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    b[j] = out[j * 64 + lane];
#pragma unroll
    for (int s = 0; s < NF + NG; ++s) a[s][j] = out[(4 + s * 4 + j) * 64 + lane];
  }
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < halves; ++it) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int s = 0; s < NF; ++s) {
        mfma16(acc[s], a[s][j], b[j]);
        if constexpr (SPREAD && NG > 0) {
          if ((s + 1) % (NF / NG) == 0 && (s + 1) / (NF / NG) <= NG) mfma4(gacc[(s + 1) / (NF / NG) - 1], a[NF + (s + 1) / (NF / NG) - 1][j], b[j]);
        }
      }
      if constexpr (!SPREAD) {
#pragma unroll
        for (int q = 0; q < NG; ++q) mfma4(gacc[q], a[NF + q][j], b[j]);
      }
    }
  }
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NF; ++k) s += acc[k][0] + acc[k][1] + acc[k][2] + acc[k][3];
#pragma unroll
  for (int k = 0; k < NG; ++k) s += gacc[k][0] + gacc[k][1] + gacc[k][2] + gacc[k][3];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (lane == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
}
// ---- (c) layout: out[r][c] = sum_k R[r][k] C[c][k], 16 rows x 4 columns x 16 reduction indices, through the 4x4x1 form
// with the fragments of tail_gemm.hpp: lane (r = lane & 15, g = lane >> 4) holds R[r][4g .. 4g+3] and C[lane & 3][4g .. 4g+3].
__global__ __launch_bounds__(64) void k_layout4(const float *R, const float *C, float *out, float *raw) {
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const float4 fb = *reinterpret_cast<const float4 *>(R + r * 16 + 4 * g);
  const float4 fa = *reinterpret_cast<const float4 *>(C + (lane & 3) * 16 + 4 * g);
  floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(fa.x, fb.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(fa.y, fb.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(fa.z, fb.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(fa.w, fb.w, acc, 0, 0, 0);
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    raw[lane * 4 + v] = acc[v];                     // the partial sum of k-class g: row r, column v
    float s = acc[v];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (g == 0) out[r * 4 + v] = s;
  }
}
template <class K>
double run_cycles(K kern, int grid, int n, double per_iter, float *ms_out) {
  float *o; uint64_t *c;
  CK(hipMalloc(&o, grid * 256 * 4)); CK(hipMalloc(&c, grid * 4 * 8));
  CK(hipMemset(o, 0, grid * 256 * 4));      // the kernels read their operands from the first 44 x 64 floats (grid >= 11)
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  kern<<<grid, 256>>>(o, c, n);
  CK(hipEventRecord(e0));
  kern<<<grid, 256>>>(o, c, n);
  CK(hipEventRecord(e1));
  CK(hipDeviceSynchronize());
  CK(hipEventElapsedTime(ms_out, e0, e1));
  std::vector<uint64_t> h(grid * 4);
  CK(hipMemcpy(h.data(), c, grid * 4 * 8, hipMemcpyDeviceToHost));
  std::sort(h.begin(), h.end());
  CK(hipFree(o)); CK(hipFree(c));
  return (double)h[h.size() / 2] / (n * per_iter);
}
// The streams are compared with each other in s_memtime ticks and in wall time, and turned into shader cycles with the
// 16x16x4 issue interval (32 cycles) as the scale.
void cover_probe() {
  float ms;
  printf("\n== (a) v_mfma_f32_4x4x1_16b_f32 back to back, one wave per SIMD, grid 256\n");
  float ms28;
  const double t28 = run_cycles(k_half<7, 0>, 256, 20000, 1.0, &ms28);
  const double cyc_per_tick = 28.0 * 32.0 / t28;
  const double i4 = run_cycles(k_issue4<4>, 256, 4000, 64.0, &ms);
  printf("4 independent accumulators: %.4f ticks per instruction = %.2f cycles (scale: 28 x 16x16x4 = %.3f ticks = 896 cycles), kernel %.1f us\n",
         i4, i4 * cyc_per_tick, t28, ms * 1e3);
  const double i1 = run_cycles(k_issue4<1>, 256, 4000, 16.0, &ms);
  printf("1 accumulator (dependent):  %.4f ticks per instruction = %.2f cycles, kernel %.1f us\n", i1, i1 * cyc_per_tick, ms * 1e3);
  printf("\n== (b) half-slice streams, registers only, j-major, one wave per SIMD, grid 256, 20000 halves\n");
  printf("%-34s %10s %10s %12s\n", "stream", "ticks/half", "cycles/half", "kernel us");
  printf("%-34s %10.3f %10.1f %12.1f\n", "28 x 16x16x4 (today)", t28, t28 * cyc_per_tick, ms28 * 1e3);
  const double t24_4 = run_cycles(k_half<6, 1>, 256, 20000, 1.0, &ms);
  printf("%-34s %10.3f %10.1f %12.1f\n", "24 x 16x16x4 + 4 x 4x4x1 (100 cols)", t24_4, t24_4 * cyc_per_tick, ms * 1e3);
  const double t24_8 = run_cycles(k_half<6, 2>, 256, 20000, 1.0, &ms);
  printf("%-34s %10.3f %10.1f %12.1f\n", "24 x 16x16x4 + 8 x 4x4x1 (104 cols)", t24_8, t24_8 * cyc_per_tick, ms * 1e3);
  const double t24_12 = run_cycles(k_half<6, 3>, 256, 20000, 1.0, &ms);
  printf("%-34s %10.3f %10.1f %12.1f\n", "24 x 16x16x4 + 12 x 4x4x1 (108 cols)", t24_12, t24_12 * cyc_per_tick, ms * 1e3);
  const double t24_8s = run_cycles(k_half<6, 2, true>, 256, 20000, 1.0, &ms);
  printf("%-34s %10.3f %10.1f %12.1f\n", "24 + 8, groups spread (MMMgMMMg)", t24_8s, t24_8s * cyc_per_tick, ms * 1e3);
  const double t24_12s = run_cycles(k_half<6, 3, true>, 256, 20000, 1.0, &ms);
  printf("%-34s %10.3f %10.1f %12.1f\n", "24 + 12, groups spread (MMgMMgMMg)", t24_12s, t24_12s * cyc_per_tick, ms * 1e3);
  const double t24 = run_cycles(k_half<6, 0>, 256, 20000, 1.0, &ms);
  printf("%-34s %10.3f %10.1f %12.1f\n", "24 x 16x16x4 alone", t24, t24 * cyc_per_tick, ms * 1e3);
  const double saved = (t28 - t24_4) * cyc_per_tick;
  printf("saved per half slice, 100 columns: %.1f cycles of the predicted 96 -> %s (no-go below 48)\n", saved, saved >= 48.0 ? "GO" : "NO-GO");
  printf("saved per half slice, 104 columns: %.1f cycles of the predicted 64 (groups spread: %.1f)\n", (t28 - t24_8) * cyc_per_tick,
         (t28 - t24_8s) * cyc_per_tick);

  printf("\n== (c) lane maps: 16 rows x 4 columns x 16 reduction indices against a scalar fmaf loop (small integers: exact)\n");
  std::vector<float> R(16 * 16), C(4 * 16), ref(16 * 4), got(16 * 4), raw(64 * 4);
  for (int i = 0; i < 16 * 16; ++i) R[i] = (float)((i * 7 + 3) % 11 - 5);
  for (int i = 0; i < 4 * 16; ++i) C[i] = (float)((i * 5 + 1) % 13 - 6);
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 4; ++c) {
      float s = 0.f;
      for (int k = 0; k < 16; ++k) s = fmaf(R[r * 16 + k], C[c * 16 + k], s);
      ref[r * 4 + c] = s;
    }
  float *dR, *dC, *dO, *dRaw;
  CK(hipMalloc(&dR, R.size() * 4)); CK(hipMalloc(&dC, C.size() * 4)); CK(hipMalloc(&dO, got.size() * 4)); CK(hipMalloc(&dRaw, raw.size() * 4));
  CK(hipMemcpy(dR, R.data(), R.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dC, C.data(), C.size() * 4, hipMemcpyHostToDevice));
  k_layout4<<<1, 64>>>(dR, dC, dO, dRaw);
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(got.data(), dO, got.size() * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(raw.data(), dRaw, raw.size() * 4, hipMemcpyDeviceToHost));
  int bad = 0, bad_raw = 0;
  for (int i = 0; i < 64; ++i) bad += got[i] != ref[i];
  for (int l = 0; l < 64; ++l)          // lane (r, g), register v = row r, column v, reduction indices 4g .. 4g+3 only
    for (int v = 0; v < 4; ++v) {
      const int r = l & 15, g = l >> 4;
      float s = 0.f;
      for (int k = 4 * g; k < 4 * g + 4; ++k) s = fmaf(R[r * 16 + k], C[v * 16 + k], s);
      bad_raw += raw[l * 4 + v] != s;
    }
  printf("summed over the k-classes: %d of 64 elements differ; per-lane partial sums (row lane&15, column = register, k-class lane>>4): %d of 256 differ -> %s\n",
         bad, bad_raw, bad == 0 && bad_raw == 0 ? "lane maps VERIFIED" : "lane maps WRONG");
  CK(hipFree(dR)); CK(hipFree(dC)); CK(hipFree(dO)); CK(hipFree(dRaw));
}
int main() {
  run<0, 4>("registers only", 256, 2000);
  run<0, 4>("registers only", 1, 2000);
  run<1, 4>("16 ds_read_b128/stage, swizzled", 256, 2000);
  run<2, 4>("16 ds_read_b128/stage, plain rows", 256, 2000);
  run<0, 8>("registers only, 2 waves/SIMD", 256, 2000);
  run<1, 8>("16 ds_read_b128/stage swizzled, 2 waves/SIMD", 256, 2000);
  cover_probe();
  return 0;
}
