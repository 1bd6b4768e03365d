// ptq_int4.hip — the serving form of PTQEmb_Int(n_bits=4): two 4-bit codes per byte, and the device-side writer of every
// PTQ integer table (src/models/embeddings/ptq_emb.py:61-91 of the reference, which keeps one 4-bit code per int8 byte).
//
// The packed layout (public: it is what state_dict() carries): weight is uint8 [N, D / 2], element d of row r lives in
// byte r D / 2 + d / 2, the low nibble for even d, the high nibble for odd d, each nibble a two's-complement code in
// [-8, 7].  The scale (fp32) and the zero point (int8: it can lie outside the nibble range) stay device scalars.
//
//   k_gather_rows_i4   the dequantising row gather: one thread per BYTE (two elements, one 8-byte store), the per-field
//                      offsets added inside the launch, idx == NULL the table form (row r is r): the bits of
//                      k_gather_rows_q (embed.hip) over the unpacked int8 codes — (float)(code - zero) * scale.
//   k_ptq_quantise*    fp32 [N, D] of any row stride -> int8 codes, int16 codes or packed nibbles in one pass:
//                      rintf(w / scale + (float)zero), clamped to the n-bit range below 8 bits — the reference's operations
//                      in its order (ptq_emb.py:78-83): an IEEE division (this file is built without fast-math, and no
//                      multiply feeds the add: nothing contracts), round half to even, then the narrowing of a float to the
//                      storage type through int32, as the host does it.
//   k_int4_repack      int8 codes [N, D] <-> packed nibbles; a code outside [-8, 7] ORs MI_CODE_OUT_OF_RANGE into *err.
// No LDS, no scratch, no atomics but the error word's.
#include "common.hpp"

namespace {
using namespace mi;

enum { OUT_INT8 = 0, OUT_INT16 = 1, OUT_NIBBLES = 2 };

inline int grid_for_elems(int64_t total) {
  int64_t g = (total + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  if (g > kMaxGrid * 4) g = kMaxGrid * 4;
  return (int)g;
}

__device__ __forceinline__ int nibble(uint32_t w, int k) { return (int)(w << (28 - 4 * k)) >> 28; }

// ------------------------------------------------------------------ row gather ----
// VEC: out is 8-byte aligned, a thread's two values leave as one store
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_gather_rows_i4(const int64_t *__restrict__ idx, const int64_t *__restrict__ offsets,
                                                           const uint8_t *__restrict__ W, const float *__restrict__ scale,
                                                           const int8_t *__restrict__ zero, float *__restrict__ out,
                                                           int64_t *__restrict__ rows_out, int64_t n, int F, int D, int64_t N,
                                                           int *err) {
  const int H = D >> 1;
  const int64_t total = n * H;
  const float sc = scale[0];
  const int zp = (int)zero[0];
  int bad = 0;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / H;
    const int j = (int)(t - i * H);
    int64_t row = idx ? idx[i] : i;
    if (offsets) row += offsets[i % F];
    if (rows_out && j == 0) rows_out[i] = row;
    float lo = 0.f, hi = 0.f;
    if ((uint64_t)row < (uint64_t)N) {
      const uint32_t b = W[row * H + j];
      lo = (float)(nibble(b, 0) - zp) * sc;
      hi = (float)(nibble(b, 1) - zp) * sc;
    } else {
      bad = 1;
    }
    float *o = out + i * D + 2 * j;
    if constexpr (VEC) {
      *reinterpret_cast<float2 *>(o) = make_float2(lo, hi);
    } else {
      o[0] = lo;
      o[1] = hi;
    }
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// ------------------------------------------------------------------- quantiser ----
struct QuantArgs {
  const float *W;
  int64_t ldw;           // row stride of W in elements
  const float *scale;
  const void *zero;      // int8 word (int8 codes, nibbles) or int16 word (int16 codes)
  float lo, hi;          // the clamp; lo > hi: none (n_bits = 8, 16: the reference does not clamp there)
  void *out;
  int64_t N;
  int D;
};

template <int MODE>
__device__ __forceinline__ float zero_of(const QuantArgs &a) {
  if constexpr (MODE == OUT_INT16) return (float)reinterpret_cast<const int16_t *>(a.zero)[0];
  else return (float)reinterpret_cast<const int8_t *>(a.zero)[0];
}

// the code of w as the integer the storage type is narrowed from
__device__ __forceinline__ int code_of(float w, float sc, float zf, float lo, float hi) {
  float q = rintf(w / sc + zf);
  if (lo <= hi) q = fminf(fmaxf(q, lo), hi);
  return (int)q;
}

// D % 4 == 0: one thread per four consecutive elements of a row, one store of 4 (int8), 8 (int16) or 2 (nibbles) bytes.
// LD4: the four floats by one 16-byte load (W's base and row stride allow it)
template <int MODE, bool LD4>
__global__ __launch_bounds__(kBlock) void k_ptq_quantise4(QuantArgs a) {
  const int Q = a.D >> 2;
  const int64_t total = a.N * Q;
  const float sc = a.scale[0];
  const float zf = zero_of<MODE>(a);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / Q;
    const int q = (int)(t - r * Q);
    const float *src = a.W + r * a.ldw + 4 * q;
    float4 w;
    if constexpr (LD4) w = ld4(src);
    else w = make_float4(src[0], src[1], src[2], src[3]);
    const int c0 = code_of(w.x, sc, zf, a.lo, a.hi), c1 = code_of(w.y, sc, zf, a.lo, a.hi),
              c2 = code_of(w.z, sc, zf, a.lo, a.hi), c3 = code_of(w.w, sc, zf, a.lo, a.hi);
    if constexpr (MODE == OUT_INT8) {
      reinterpret_cast<uint32_t *>(a.out)[t] = (uint32_t)(c0 & 0xff) | ((uint32_t)(c1 & 0xff) << 8) |
                                               ((uint32_t)(c2 & 0xff) << 16) | ((uint32_t)(c3 & 0xff) << 24);
    } else if constexpr (MODE == OUT_INT16) {
      reinterpret_cast<uint2 *>(a.out)[t] = make_uint2((uint32_t)(c0 & 0xffff) | ((uint32_t)(c1 & 0xffff) << 16),
                                                       (uint32_t)(c2 & 0xffff) | ((uint32_t)(c3 & 0xffff) << 16));
    } else {
      reinterpret_cast<uint16_t *>(a.out)[t] = (uint16_t)((c0 & 0xf) | ((c1 & 0xf) << 4) | ((c2 & 0xf) << 8) | ((c3 & 0xf) << 12));
    }
  }
}

// any D (even for the nibbles): one thread per output element — a code, or a byte of two nibbles
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_ptq_quantise1(QuantArgs a) {
  const int per = MODE == OUT_NIBBLES ? 2 : 1;
  const int C = a.D / per;
  const int64_t total = a.N * C;
  const float sc = a.scale[0];
  const float zf = zero_of<MODE>(a);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / C;
    const int c = (int)(t - r * C);
    const float *src = a.W + r * a.ldw + per * c;
    const int c0 = code_of(src[0], sc, zf, a.lo, a.hi);
    if constexpr (MODE == OUT_INT8) {
      reinterpret_cast<int8_t *>(a.out)[t] = (int8_t)c0;
    } else if constexpr (MODE == OUT_INT16) {
      reinterpret_cast<int16_t *>(a.out)[t] = (int16_t)c0;
    } else {
      const int c1 = code_of(src[1], sc, zf, a.lo, a.hi);
      reinterpret_cast<uint8_t *>(a.out)[t] = (uint8_t)((c0 & 0xf) | ((c1 & 0xf) << 4));
    }
  }
}

template <int MODE>
int launch_quantise(const QuantArgs &a, void *stream) {
  const uintptr_t po = reinterpret_cast<uintptr_t>(a.out);
  const uintptr_t need = MODE == OUT_INT8 ? 3 : MODE == OUT_INT16 ? 7 : 1;      // the store of four codes is aligned
  if ((a.D & 3) == 0 && (po & need) == 0) {
    const int grid = grid_for_elems(a.N * (a.D >> 2));
    if (aligned16(a.W) && (a.ldw & 3) == 0)
      MI_LAUNCH("ptq_quantise", (k_ptq_quantise4<MODE, true>), grid, kBlock, stream, a);
    else
      MI_LAUNCH("ptq_quantise", (k_ptq_quantise4<MODE, false>), grid, kBlock, stream, a);
  } else {
    MI_LAUNCH("ptq_quantise", k_ptq_quantise1<MODE>, grid_for_elems(a.N * (a.D / (MODE == OUT_NIBBLES ? 2 : 1))), kBlock,
              stream, a);
  }
  return launch_status();
}

// -------------------------------------------------------------------- repacker ----
// one thread per packed byte.  PACK: codes int8 [N, D] -> nibbles; else nibbles -> codes
template <bool PACK>
__global__ __launch_bounds__(kBlock) void k_int4_repack(const void *__restrict__ src, void *__restrict__ dst, int64_t bytes,
                                                        int *err) {
  int bad = 0;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < bytes; t += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (PACK) {
      const int c0 = reinterpret_cast<const int8_t *>(src)[2 * t], c1 = reinterpret_cast<const int8_t *>(src)[2 * t + 1];
      bad |= (c0 < -8) | (c0 > 7) | (c1 < -8) | (c1 > 7);
      reinterpret_cast<uint8_t *>(dst)[t] = (uint8_t)((c0 & 0xf) | ((c1 & 0xf) << 4));
    } else {
      const uint32_t b = reinterpret_cast<const uint8_t *>(src)[t];
      reinterpret_cast<int8_t *>(dst)[2 * t] = (int8_t)nibble(b, 0);
      reinterpret_cast<int8_t *>(dst)[2 * t + 1] = (int8_t)nibble(b, 1);
    }
  }
  if (bad && err) atomicOr(err, MI_CODE_OUT_OF_RANGE);
}

}  // namespace

extern "C" {

int mi_gather_rows_int4(const int64_t *idx, const int64_t *offsets, const void *W, const float *scale, const void *zero,
                        float *out, int64_t *rows_out, int64_t n, int32_t F, int32_t D, int64_t N, int32_t *err,
                        void *stream) {
  if (n < 0 || D <= 0 || (D & 1) || N < 0 || (offsets && F < 1)) return MI_ERR_INVALID_ARG;
  if (rows_out && !idx) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!W || !scale || !zero || !out) return MI_ERR_INVALID_ARG;
  const int grid = grid_for_elems(n * (D >> 1));
  const uint8_t *Wb = reinterpret_cast<const uint8_t *>(W);
  const int8_t *zp = reinterpret_cast<const int8_t *>(zero);
  if ((reinterpret_cast<uintptr_t>(out) & 7) == 0)
    MI_LAUNCH("gather_rows_int4", k_gather_rows_i4<true>, grid, kBlock, stream, idx, offsets, Wb, scale, zp, out, rows_out, n,
              F, D, N, err);
  else
    MI_LAUNCH("gather_rows_int4", k_gather_rows_i4<false>, grid, kBlock, stream, idx, offsets, Wb, scale, zp, out, rows_out, n,
              F, D, N, err);
  return launch_status();
}

int mi_ptq_quantise(const float *W, int64_t ldw, const float *scale, const void *zero, int32_t n_bits, int32_t packed,
                    void *codes_out, int64_t N, int32_t D, void *stream) {
  if (N < 0 || D <= 0 || ldw < D || (n_bits != 4 && n_bits != 8 && n_bits != 16)) return MI_ERR_INVALID_ARG;
  if (packed && (n_bits != 4 || (D & 1))) return MI_ERR_INVALID_ARG;
  if (N == 0) return MI_OK;
  if (!W || !scale || !zero || !codes_out) return MI_ERR_INVALID_ARG;
  QuantArgs a{W, ldw, scale, zero, 0.f, -1.f, codes_out, N, D};
  if (n_bits < 8) {
    a.lo = -(float)(1 << (n_bits - 1));
    a.hi = (float)((1 << (n_bits - 1)) - 1);
  }
  if (packed) return launch_quantise<OUT_NIBBLES>(a, stream);
  if (n_bits == 16) return launch_quantise<OUT_INT16>(a, stream);
  return launch_quantise<OUT_INT8>(a, stream);
}

int mi_int4_repack(const void *src, void *dst, int32_t unpack, int64_t N, int32_t D, int32_t *err, void *stream) {
  if (N < 0 || D <= 0 || (D & 1)) return MI_ERR_INVALID_ARG;
  if (N == 0) return MI_OK;
  if (!src || !dst) return MI_ERR_INVALID_ARG;
  const int64_t bytes = N * (D >> 1);
  if (unpack)
    MI_LAUNCH("int4_repack", k_int4_repack<false>, grid_for_elems(bytes), kBlock, stream, src, dst, bytes, err);
  else
    MI_LAUNCH("int4_repack", k_int4_repack<true>, grid_for_elems(bytes), kBlock, stream, src, dst, bytes, err);
  return launch_status();
}

}  // extern "C"
