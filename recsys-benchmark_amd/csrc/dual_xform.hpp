// dual_xform.hpp — what the two-table compositional kernels share (embed.hip: lookups by id; dual_table.hip: the whole
// table): the combine / transform enums and the element transforms.  One definition, so that the table form and the
// lookup over arange(N) give the same bits.
#pragma once
#include "common.hpp"

namespace mi {

enum { OP_MULT = 0, OP_ADD = 1, OP_CAT = 2 };
enum { XF_NONE = 0, XF_SOFT = 1, XF_MASK = 2 };

__device__ __forceinline__ float sigmoidf_(float s) { return 1.f / (1.f + expf(-s)); }
__device__ __forceinline__ float signf_(float w) { return (w > 0.f) ? 1.f : ((w < 0.f) ? -1.f : 0.f); }
__device__ __forceinline__ float soft_(float w, float s) {
  const float u = fabsf(w) - sigmoidf_(s);
  return signf_(w) * (u > 0.f ? u : 0.f);
}

template <int XF>
__device__ __forceinline__ float4 load_row4(const float *T, const float *S, const uint8_t *M, int64_t o) {
  float4 w = ld4(T + o);
  if constexpr (XF == XF_SOFT) {
    const float4 s = ld4(S + o);
    w.x = soft_(w.x, s.x); w.y = soft_(w.y, s.y); w.z = soft_(w.z, s.z); w.w = soft_(w.w, s.w);
  } else if constexpr (XF == XF_MASK) {
    const uchar4 m = *reinterpret_cast<const uchar4 *>(M + o);
    w.x = m.x ? w.x : 0.f; w.y = m.y ? w.y : 0.f; w.z = m.z ? w.z : 0.f; w.w = m.w ? w.w : 0.f;
  }
  return w;
}

}  // namespace mi
