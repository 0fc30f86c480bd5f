// The Gaussian noise of mgr_add_gaussian_noise (elementwise.hip) and mgr_augment_apply (augment.hip): one device function, so that
// the two calls add the same bits to the same element.
#pragma once
#include "common.h"

// Box-Muller on two 24-bit uniforms per PAIR of elements: pair i of the flat buffer covers elements 2i (cosine half) and 2i + 1
// (sine half).  Returns the radius (stddev folded in) and the two halves of the unit vector.
__device__ static inline void mgr_noise_pair(uint64_t seed, size_t i, float stddev, float* rad, float* c, float* s) {
  uint64_t r = mgr_mix64(seed * 0xD1342543DE82EF95ull + i);
  float u1 = ((float)((uint32_t)(r >> 40)) + 1.0f) * (1.0f / 16777216.0f);  // (0,1]
  float u2 = (float)((uint32_t)(r >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
  *rad = sqrtf(-2.0f * logf(u1)) * stddev;
  sincosf(6.283185307179586f * u2, s, c);
}
// x + rad * trig in ONE rounding - what the compiler made of k_add_noise's `X[e] + rad * c` all along, written down so that it
// does not depend on what surrounds the expression
__device__ static inline float mgr_noise_add(float x, float rad, float trig) { return __fmaf_rn(rad, trig, x); }
