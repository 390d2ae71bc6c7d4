// IoU of two axis-aligned 3-D boxes (x1, y1, z1, x2, y2, z2) in fp32, in the operation order of evaluate.box_iou_3d
// (the reference's model/utils.py:391-462), every operation rounded on its own.  One definition for every kernel that
// has to reproduce the SAME bits for a pair (assign.hip compares a recomputed quality to a stored maximum with ==).
#pragma once
#include <stdint.h>

#pragma clang fp contract(off)

namespace inr {

// torch.maximum / torch.minimum: a NaN operand gives NaN (fmaxf / fminf would drop it)
__device__ __forceinline__ float iou_max_nan(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ float iou_min_nan(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

__device__ __forceinline__ float aabb_volume(const float* b) { return ((b[3] - b[0]) * (b[4] - b[1])) * (b[5] - b[2]); }

// a: first box with its volume va, b: second box with its volume vb.  union = (va + vb) - inter, IEEE division.
__device__ __forceinline__ float aabb_iou(const float* a, float va, const float* b, float vb) {
  float ext[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float d = iou_min_nan(a[3 + c], b[3 + c]) - iou_max_nan(a[c], b[c]);
    ext[c] = d < 0.0f ? 0.0f : d;             // clamp(min=0): NaN stays NaN
  }
  const float inter = (ext[0] * ext[1]) * ext[2];
  return inter / ((va + vb) - inter);
}

// Order-preserving uint32 key of a float for integer max: NaN is the top key, negatives sort below +0 (-0 just below
// +0), key 0 is below every key a number or a NaN maps to.  key_float inverts it (the top key comes back as a NaN).
__device__ __forceinline__ uint32_t float_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return v != v ? 0xFFFFFFFFu : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

}  // namespace inr
