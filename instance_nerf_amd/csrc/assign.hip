// Training targets of the detector heads (include/inr.h, "Detector training targets"): the IoU matcher of the RPN and
// of the RoI heads without the [G, A] quality matrix, and the box coder, in two launches.
//
// Both kernels stage the G ground-truth boxes in LDS as rows of 8 floats - six coordinates, the volume, one spare word -
// (32 B x G, 32 KB at G = 1024; one 16-byte and two narrower broadcast reads per pair) and recompute a box's column of
// qualities from them with box_iou.h's aabb_iou: the same function on the same operands in both kernels, so the float ==
// of the restore rule sees identical bits.
//
//   k_box_match_gt_max   a workgroup of 256 lanes owns kBmRun = 1024 consecutive boxes, four per lane (lane t: boxes
//                        t, t + 256, ...).  Per GT the lane's largest order-preserving key (box_iou.h) goes into the GT
//                        row's spare word with an LDS integer max - issued only when it exceeds the word's current value,
//                        which most pairs (IoU 0 after the first) do not - and at the end every GT is at most one global
//                        integer atomicMax, again only when it would raise the value.  Integers only: the result does
//                        not depend on the order of arrival.
//   k_box_match_assign   one lane per box.  The spare word holds the GT's row maximum as a float.  The lane walks the G
//                        qualities once (arg-max, restore flag), applies the thresholds, and writes its outputs; the
//                        24-byte rows of matched_boxes and targets are six dword stores per lane.
// The run length of 1024 and the store pattern of the 24-byte rows are first choices; nothing else was tried.
#include "common.h"
#include "box_iou.h"

#pragma clang fp contract(off)

namespace inr {
namespace {

constexpr int kBmBlock = INR_BOX_MATCH_BLOCK;
constexpr int kBmRun = INR_BOX_MATCH_BOXES_PER_WG;
constexpr int kBmPerLane = kBmRun / kBmBlock;
constexpr int kBmMaxGt = INR_BOX_MATCH_MAX_GT;
constexpr int kBmRow = 8;                       // floats per staged GT
static_assert(kBmRun % kBmBlock == 0, "a run is a whole number of boxes per lane");
static_assert(kBmMaxGt * kBmRow * 4 <= 65536, "the staged GT boxes fit the LDS of a workgroup");

// GT rows into LDS: coordinates, volume, and the spare word: the row maximum as a float, or the key 0 when `keys` is null.
__device__ __forceinline__ void bm_stage(const float* __restrict__ gt, int G, const uint32_t* __restrict__ keys, float* sg) {
  for (int g = threadIdx.x; g < G; g += kBmBlock) {
    float r[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) r[c] = gt[g * 6 + c];
#pragma unroll
    for (int c = 0; c < 6; ++c) sg[g * kBmRow + c] = r[c];
    sg[g * kBmRow + 6] = aabb_volume(r);
    sg[g * kBmRow + 7] = keys != nullptr ? key_float(keys[g]) : __uint_as_float(0u);
  }
}

__global__ __launch_bounds__(kBmBlock) void k_box_match_gt_max(const float* __restrict__ gt, int G,
                                                               const float* __restrict__ boxes,
                                                               const uint8_t* __restrict__ valid, int A,
                                                               uint32_t* __restrict__ keys) {
  extern __shared__ float sg[];
  bm_stage(gt, G, nullptr, sg);
  const int a0 = blockIdx.x * kBmRun + threadIdx.x;       // < A + kBmRun <= 2^31 / 6 + 1024
  float b[kBmPerLane][6], vb[kBmPerLane];
  int state[kBmPerLane];                        // 0: past the end, 1: a box, 2: a masked box (quality -1)
#pragma unroll
  for (int i = 0; i < kBmPerLane; ++i) {
    const int a = a0 + i * kBmBlock;
    state[i] = a < A ? ((valid == nullptr || valid[a] != 0) ? 1 : 2) : 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) b[i][c] = a < A ? boxes[a * 6 + c] : 0.0f;
    vb[i] = aabb_volume(b[i]);
  }
  __syncthreads();
  uint32_t* skey = reinterpret_cast<uint32_t*>(sg);
  for (int g = 0; g < G; ++g) {
    const float* s = sg + g * kBmRow;
    uint32_t k = 0;
#pragma unroll
    for (int i = 0; i < kBmPerLane; ++i) {
      const uint32_t ki = float_key(state[i] == 1 ? aabb_iou(s, s[6], b[i], vb[i]) : -1.0f);
      if (state[i] != 0 && ki > k) k = ki;
    }
    uint32_t* word = skey + g * kBmRow + 7;
    if (k > __atomic_load_n(word, __ATOMIC_RELAXED)) atomicMax(word, k);
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += kBmBlock) {
    const uint32_t k = skey[g * kBmRow + 7];
    if (k > __atomic_load_n(keys + g, __ATOMIC_RELAXED)) atomicMax(keys + g, k);
  }
}

// The six regression targets of box p against reference box r (coder/AABB_coder.py:7-56), one fp32 operation at a time.
__device__ __forceinline__ void bm_encode(const float* r, const float* p, float* t) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float ex = p[3 + c] - p[c], ectr = p[c] + 0.5f * ex;
    const float gx = r[3 + c] - r[c], gctr = r[c] + 0.5f * gx;
    t[c] = (gctr - ectr) / ex;
    t[3 + c] = logf(gx / ex);
  }
}

__global__ __launch_bounds__(kBmBlock) void k_box_match_assign(const float* __restrict__ gt, const int* __restrict__ gt_labels,
                                                               int G, const float* __restrict__ boxes,
                                                               const uint8_t* __restrict__ valid, int A,
                                                               const uint32_t* __restrict__ keys, float high, float low,
                                                               int allow, int* __restrict__ matched, int* __restrict__ labels,
                                                               float* __restrict__ best_iou, float* __restrict__ matched_boxes,
                                                               float* __restrict__ targets) {
  extern __shared__ float sg[];
  bm_stage(gt, G, keys, sg);
  __syncthreads();
  const int a = blockIdx.x * kBmBlock + threadIdx.x;
  if (a >= A) return;
  float b[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) b[c] = boxes[a * 6 + c];
  const bool ok = valid == nullptr || valid[a] != 0;
  const float vb = aabb_volume(b);
  float best = 0.0f;
  int arg = 0;
  bool restore = false;
  for (int g = 0; g < G; ++g) {
    const float* s = sg + g * kBmRow;
    const float q = ok ? aabb_iou(s, s[6], b, vb) : -1.0f;
    restore |= q == s[7];                       // never true for a NaN on either side
    // torch.max over dim 0 on CPU tensors: the lowest index among equals, a NaN above every number, the first NaN wins
    if (g == 0 || (best == best && (q > best || q != q))) {
      best = q;
      arg = g;
    }
  }
  int m = arg;
  if (best < low) m = -1;
  else if (best >= low && best < high) m = -2;  // a NaN keeps its arg-max
  if (allow && restore) m = arg;
  matched[a] = m;
  if (labels != nullptr) {
    int l = m >= 0 ? (gt_labels != nullptr ? gt_labels[m] : 1) : (m == -1 ? 0 : -1);
    if (!ok) l = -1;
    labels[a] = l;
  }
  if (best_iou != nullptr) best_iou[a] = best;
  const float* r = sg + (m > 0 ? m : 0) * kBmRow;
  if (matched_boxes != nullptr) {
#pragma unroll
    for (int c = 0; c < 6; ++c) matched_boxes[a * 6 + c] = r[c];
  }
  if (targets != nullptr) {
    float t[6];
    bm_encode(r, b, t);
#pragma unroll
    for (int c = 0; c < 6; ++c) targets[a * 6 + c] = t[c];
  }
}

// Shared by both entry points: the message for sizes the kernels do not take, or null.
const char* bm_sizes(int32_t G, int64_t A) {
  if (G < 1 || G > kBmMaxGt) return "G must be in 1..1024 (INR_BOX_MATCH_MAX_GT)";
  if (A < 0) return "A must not be negative";
  if (A > ((int64_t)1 << 31) / 6) return "too many boxes: 6*A must be below 2^31";
  return nullptr;
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_box_match_gt_max(const float* gt, int32_t G, const float* boxes, const uint8_t* valid, int64_t A,
                         uint32_t* gt_max_keys, inr_stream_t s) {
  const char* why = bm_sizes(G, A);
  INR_REQUIRE(why == nullptr, why);
  if (A == 0) return INR_OK;
  INR_REQUIRE(gt && boxes && gt_max_keys, "null pointer (gt, boxes, gt_max_keys)");
  INR_REQUIRE(aligned4(gt) && aligned4(boxes) && aligned4(gt_max_keys), "misaligned gt, boxes or gt_max_keys (4 bytes)");
  hipStream_t st = as_stream(s);
  if (hipMemsetAsync(gt_max_keys, 0, (size_t)G * 4, st) != hipSuccess) return check_launch("inr_box_match_gt_max");
  k_box_match_gt_max<<<blocks_for(A, kBmRun), kBmBlock, (size_t)G * kBmRow * 4, st>>>(gt, G, boxes, valid, (int)A, gt_max_keys);
  return check_launch("inr_box_match_gt_max");
}

int inr_box_match_assign(const float* gt, const int32_t* gt_labels, int32_t G, const float* boxes, const uint8_t* valid,
                         int64_t A, const uint32_t* gt_max_keys, float high, float low, int32_t allow_low_quality,
                         int32_t* matched, int32_t* labels, float* best_iou, float* matched_boxes, float* targets,
                         inr_stream_t s) {
  const char* why = bm_sizes(G, A);
  INR_REQUIRE(why == nullptr, why);
  INR_REQUIRE(low <= high, "low must not exceed high (and neither may be NaN)");
  if (A == 0) return INR_OK;
  INR_REQUIRE(gt && boxes && gt_max_keys && matched, "null pointer (gt, boxes, gt_max_keys, matched)");
  INR_REQUIRE(aligned4(gt) && aligned4(gt_labels) && aligned4(boxes) && aligned4(gt_max_keys) && aligned4(matched) &&
                  aligned4(labels) && aligned4(best_iou) && aligned4(matched_boxes) && aligned4(targets),
              "misaligned pointer (every array but valid is 4-byte aligned)");
  k_box_match_assign<<<blocks_for(A, kBmBlock), kBmBlock, (size_t)G * kBmRow * 4, as_stream(s)>>>(
      gt, gt_labels, G, boxes, valid, (int)A, gt_max_keys, high, low, allow_low_quality != 0, matched, labels, best_iou,
      matched_boxes, targets);
  return check_launch("inr_box_match_assign");
}

}  // extern "C"
