// common.hpp — shared helpers for the gfx950 kernels of libmi355x_recsys.so.
// Wave = 64 lanes everywhere (CDNA4); nothing here is portable to 32-wide warps.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/mi355x_recsys.h"

namespace mi {

constexpr int kWave = 64;
constexpr int kBlock = 256;            // 4 waves per workgroup
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kMaxGrid = 256 * 8;      // 256 CUs x 8 resident 256-thread workgroups

// ---- profiling ring (mi_prof_*) --------------------------------------------
// prof_acquire returns false when the ring is disarmed or full; otherwise the
// event pair that hipExtLaunchKernelGGL stamps with the dispatch's own begin /
// end timestamps (what rocprofv3 --kernel-trace reports), not stream markers.
bool prof_acquire(const char *name, hipEvent_t *a, hipEvent_t *b);

inline int launch_status() {
  return hipGetLastError() == hipSuccess ? MI_OK : MI_ERR_LAUNCH;
}

inline int grid_for_waves(int64_t n_wave_items) {
  int64_t g = (n_wave_items + kWavesPerBlock - 1) / kWavesPerBlock;
  if (g < 1) g = 1;
  if (g > kMaxGrid) g = kMaxGrid;
  return (int)g;
}

__host__ __device__ inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the row widths of the float4 kernels: a row of D floats is LPR = D / 4 lanes x float4, LPR one of 1, 2, 4 .. 64
inline bool vec_ok(int D) { return D >= 4 && D <= 256 && (D & 3) == 0 && ((D >> 2) & ((D >> 2) - 1)) == 0; }
// every pointer of the list is 16-byte aligned (a null one, i.e. an operand that is not given, passes)
template <class... P>
inline bool all_aligned16(const P *...p) { return (aligned16(p) && ...); }

// ---- device helpers ----------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// sum over the lanes that differ only in bits >= log2(lo) (lo a power of two):
// i.e. over the "row slot" index r = lane / lo, keeping q = lane % lo apart.
template <int LO>
__device__ __forceinline__ float4 slot_sum(float4 v) {
#pragma unroll
  for (int m = LO; m < kWave; m <<= 1) {
    v.x += __shfl_xor(v.x, m);
    v.y += __shfl_xor(v.y, m);
    v.z += __shfl_xor(v.z, m);
    v.w += __shfl_xor(v.w, m);
  }
  return v;
}

__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
// a += b, component by component (an accumulator kept as four scalars: the compiler keeps contracting the dot4 next to it)
__device__ __forceinline__ void acc4(float4 &a, float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
// non-temporal 16-B store (global_store_dwordx4 ... nt): for streams nobody in the kernel reads back
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st4_nt(float *p, float4 v) {
  f32x4_t x = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(x, reinterpret_cast<f32x4_t *>(p));
}

// ---- integer scans over a wave / the 256-thread workgroup (mag_prune.hip, ctr_metric.hip) ---------------------------
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    uint32_t o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// exclusive scan of one value per thread over the 256-thread workgroup; *total = the sum.  `sm` holds 4 words.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *sm, uint32_t *total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  uint32_t inc = wave_incl_scan(v);
  __syncthreads();                       // sm may still be read from an earlier call
  if (lane == kWave - 1) sm[wave] = inc;
  __syncthreads();
  uint32_t base = 0, t = 0;
#pragma unroll
  for (int w = 0; w < kWavesPerBlock; ++w) {
    uint32_t s = sm[w];
    if (w < wave) base += s;
    t += s;
  }
  *total = t;
  return base + inc - v;
}

// "last workgroup sums the partials" without agent-scope fences (on gfx950 a __threadfence() is an L2 write-back +
// invalidate per workgroup: the loss kernels took 13 us with it).  ONE lane per workgroup publishes: the partials travel
// as device-scope (sc1, write-through) stores, an explicit `s_waitcnt vmcnt(0)` holds the lane until those stores have
// been acknowledged by the coherence point behind the per-XCD L2s, and only then is the ticket taken (a workgroup-scope
// fence emits NO wait between the store and the atomic — checked in the .s — so the two, at different addresses, could
// be observed out of order).  The workgroup whose ticket came back last reads the partials with sc1 loads after its
// atomic has returned, behind a workgroup barrier (MI355X_MICROARCH.md, hand-offs measured with sc1 loads, row 1).
// These launches run up to kMaxGrid / 256 = 8 workgroups per CU, while that measured row says "one per CU".
//
// block_sum: v[i] summed over the workgroup, valid in thread 0 (wave sums, then thread 0 adds the waves in order).
// All NV wave sums come before the one masked LDS write, so that their cross-lane chains interleave.
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float (&red)[NV][kWavesPerBlock]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) red[i][threadIdx.x >> 6] = v[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      v[i] = 0.f;
      for (int j = 0; j < kWavesPerBlock; ++j) v[i] += red[i][j];
    }
  }
}

// block_join: thread 0 holds the workgroup's NV totals in v.  They go to part[NV * blockIdx.x + i]; the last workgroup
// to arrive adds all of them in index order (a fixed summation tree: deterministic), its thread 0 runs
// finish(const float (&total)[NV]) and re-arms the ticket (zero on entry, zero again on exit) for the next launch.
template <int NV, class Finish>
__device__ __forceinline__ void block_join(float (&v)[NV], float (&red)[NV][kWavesPerBlock], float *part, unsigned *ticket,
                                           Finish finish) {
  __shared__ bool last;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
      __hip_atomic_store(part + NV * blockIdx.x + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.f;
  for (unsigned j = threadIdx.x; j < gridDim.x; j += kBlock) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += __hip_atomic_load(part + NV * j + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  block_sum(v, red);
  if (threadIdx.x == 0) {
    finish(v);
    *ticket = 0;
  }
}

// grid_join: every thread's NV accumulators in, finish(totals over the whole grid) out
template <int NV, class Finish>
__device__ __forceinline__ void grid_join(float (&v)[NV], float *part, unsigned *ticket, Finish finish) {
  __shared__ float red[NV][kWavesPerBlock];
  block_sum(v, red);
  block_join(v, red, part, ticket, finish);
}

}  // namespace mi

// Launch `kernel` on `stream`; when the profiling ring is armed the dispatch is
// timed by its own start/stop events.
#define MI_LAUNCH(name, kernel, grid, block, stream, ...)                               \
  do {                                                                                  \
    hipEvent_t _ea, _eb;                                                                \
    if (mi::prof_acquire(name, &_ea, &_eb))                                             \
      hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (hipStream_t)(stream),  \
                            _ea, _eb, 0, __VA_ARGS__);                                  \
    else                                                                                \
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (hipStream_t)(stream),     \
                         __VA_ARGS__);                                                  \
  } while (0)

// Expands `CALL(LPR)` with the compile-time LPR that equals the run-time `lpr` (= D / 4 of a vec_ok(D)); any other
// value returns MI_ERR_UNSUPPORTED from the calling function.
#define MI_DISPATCH_LPR(lpr, CALL)      \
  switch (lpr) {                        \
    case 1: CALL(1); break;             \
    case 2: CALL(2); break;             \
    case 4: CALL(4); break;             \
    case 8: CALL(8); break;             \
    case 16: CALL(16); break;           \
    case 32: CALL(32); break;           \
    case 64: CALL(64); break;           \
    default: return MI_ERR_UNSUPPORTED; \
  }
