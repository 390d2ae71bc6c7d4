// Where a sample lies on its ray: the ONE expression the marchers (raymarch.hip) and the records feed of the fused
// field kernel (field_fused.hip) share, so that a position rebuilt from (t, ray) has the bits of the marched one.
// Operation order is the contract at the top of oracle/march.py: the multiply and the add are two IEEE operations
// (the build is -ffp-contract=off), then the clamp to the volume.
#pragma once
#include "common.h"

namespace inr {

__device__ __forceinline__ float sample_pos(float o, float t, float d, float bound) {
  return clampf(o + t * d, -bound, bound);
}

// x01 = (p + bound) / (2 bound) for a power-of-two 2*bound: the product with the exact reciprocal `rb_inv` is the
// correctly rounded quotient (scaling by a power of two is exact short of under- and overflow, and p + bound lies in
// [0, 2 bound]), bit for bit what the positions writer's division gives.  The host takes the records feed only for
// such bounds (records_bound_ok).
__device__ __forceinline__ float sample_x01_pow2(float p, float bound, float rb_inv) { return (p + bound) * rb_inv; }

// 2*bound is a power of two in the normal range (bound = ..., 0.5, 1, 2, 4, 8, ...)
inline bool records_bound_ok(float bound) {
  int e = 0;
  return bound > 0.0f && bound < 1e30f && frexpf(2.0f * bound, &e) == 0.5f && e > -100;
}

}  // namespace inr
