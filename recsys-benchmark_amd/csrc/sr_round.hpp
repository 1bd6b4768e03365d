// sr_round.hpp — the stochastic rounding of the QAT lookups (qat.hip: the row gather; gather_fm_quant.hip: the lookup
// fused with the FM term): the counter generator and the rounding itself, so that both files round a given element with a
// given draw to the same bits.
#pragma once
#include "common.hpp"

namespace {

__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t idx) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  const uint32_t r = (uint32_t)((z ^ (z >> 31)) >> 40);   // 24 random bits: exactly representable, < 1
  return (float)r * (1.0f / 16777216.0f);
}

// The rounded code of w under scale s; qf = w / s before the clamp.  A: the launch's arguments — qmin, qmax, prob
// (nullable: the draw of element e is prob[e]), seed (a device word) and salt (the generator's stream otherwise).
template <class A>
__device__ __forceinline__ float sr_round(const A &a, float w, float s, int64_t e, float &qf) {
  qf = w / s;
  const float q = fminf(fmaxf(qf, a.qmin), a.qmax);
  const float fl = floorf(q);
  const float pf = fl + 1.f - q;
  const float u = a.prob ? a.prob[e] : uniform01((uint64_t)(a.seed[0] + a.salt), (uint64_t)e);
  return fl + (u > pf ? 1.f : 0.f);
}

}  // namespace
