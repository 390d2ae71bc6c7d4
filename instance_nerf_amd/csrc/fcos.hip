// Training targets and losses of the FCOS proposal head (include/inr.h, "FCOS training targets and losses").
//
//   k_fcos_targets        one launch for all scenes and levels, one lane per location.  A workgroup of 256 lanes owns 256
//                         consecutive locations of one (level, scene); it stages that scene's boxes as rows of 13 floats
//                         (six coordinates, the volume, the six faces of the level's sample region: 52 B x G, 52 KB at
//                         G = 1024; every lane reads the same row, so the reads are broadcasts) and walks them once.
//   k_fcos_loss_forward   a workgroup owns 1024 consecutive locations of the level-first order, four per lane; terms in
//                         fp32, five float64 sums per workgroup into the workspace (shuffles, then the four waves in order).
//   k_fcos_loss_finish    one workgroup adds the partial sums in a fixed order and writes sums and losses.
//   k_fcos_loss_backward  one lane per location; normalisers and upstream gradients are read from device memory.
// The pyramid travels in the kernel arguments (a table per kernel); nothing is copied to the device or read back.
// The run lengths (256 and 1024) are first choices; nothing else was tried.
#include "common.h"

#pragma clang fp contract(off)

namespace inr {
namespace {

constexpr int kFcBlock = INR_FCOS_BLOCK;
constexpr int kFcRun = INR_FCOS_LOCATIONS_PER_WG;
constexpr int kFcLossRun = INR_FCOS_LOSS_LOCATIONS_PER_WG;
constexpr int kFcLossPerLane = kFcLossRun / kFcBlock;
constexpr int kFcMaxGt = INR_FCOS_MAX_GT;
constexpr int kFcMaxLevels = INR_FCOS_MAX_LEVELS;
constexpr int kFcRow = 13;                      // floats per staged GT
constexpr float kFcInf = 100000000.0f;          // the reference's INF
static_assert(kFcRun == kFcBlock, "one lane per location");
static_assert(kFcLossRun % kFcBlock == 0, "a run is a whole number of locations per lane");
static_assert(kFcMaxGt * kFcRow * 4 <= 65536, "the staged GT boxes fit the LDS of a workgroup");

struct FcLevel {
  int L, H, stride, P;
  int first_block, blocks_per_scene, base;      // base: the level's first location in the level-first arrays
  float lo, hi, s;                              // sizes of interest; stride * radius
};
struct FcTable {
  int n;
  FcLevel lv[kFcMaxLevels];
};

// torch's min / max over a pair: a NaN on either side stays
__device__ __forceinline__ float fc_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ float fc_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

__device__ __forceinline__ float fc_centerness(const float* r) {
  const float a = fc_min(r[0], r[3]) / fc_max(r[0], r[3]);
  const float b = fc_min(r[1], r[4]) / fc_max(r[1], r[4]);
  const float c = fc_min(r[2], r[5]) / fc_max(r[2], r[5]);
  return sqrtf((a * b) * c);
}

__global__ __launch_bounds__(kFcBlock) void k_fcos_targets(FcTable T, const float* __restrict__ gt,
                                                           const int* __restrict__ gt_off, int max_gt,
                                                           const float* __restrict__ ori, int use_region, int norm,
                                                           float* __restrict__ labels, float* __restrict__ reg,
                                                           float* __restrict__ ctr, int* __restrict__ matched,
                                                           uint8_t* __restrict__ valid) {
  extern __shared__ __attribute__((aligned(16))) float sg[];
  FcLevel lv = T.lv[0];
#pragma unroll
  for (int l = 1; l < kFcMaxLevels; ++l)
    if (l < T.n && (int)blockIdx.x >= T.lv[l].first_block) lv = T.lv[l];
  const int rel = (int)blockIdx.x - lv.first_block;
  const int b = rel / lv.blocks_per_scene, run = rel - b * lv.blocks_per_scene;
  const int g0 = gt_off[b];
  const int G = min(max(gt_off[b + 1] - g0, 0), max_gt);
  for (int g = threadIdx.x; g < G; g += kFcBlock) {
    float r[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) r[c] = gt[(size_t)(g0 + g) * 6 + c];
    float* row = sg + g * kFcRow;
#pragma unroll
    for (int c = 0; c < 6; ++c) row[c] = r[c];
    row[6] = ((r[3] - r[0]) * (r[4] - r[1])) * (r[5] - r[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float lo = r[a], hi = r[a + 3];
      const float c = (lo + hi) / 2.0f;
      const float cm = c - lv.s, cp = c + lv.s;
      row[7 + a] = use_region ? (cm > lo ? cm : lo) : lo;
      row[10 + a] = use_region ? (cp > hi ? hi : cp) : hi;
    }
  }
  __syncthreads();
  const int p = run * kFcRun + (int)threadIdx.x;
  if (p >= lv.P) return;
  const int iz = p % lv.H, iy = (p / lv.H) % lv.L, ix = p / (lv.H * lv.L);
  const int half = lv.stride / 2;
  const float x[3] = {(float)(ix * lv.stride + half), (float)(iy * lv.stride + half), (float)(iz * lv.stride + half)};
  float best = kFcInf;
  int arg = 0;
  for (int g = 0; g < G; ++g) {
    const float* s = sg + g * kFcRow;
    bool inside = true, le_hi = true, ge_lo = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float rl = x[a] - s[a], rh = s[a + 3] - x[a];
      inside = inside && (x[a] - s[7 + a] > 0.0f) && (s[10 + a] - x[a] > 0.0f);
      le_hi = le_hi && rl <= lv.hi && rh <= lv.hi;             // max(reg) <= hi, false for a NaN
      ge_lo = ge_lo || rl >= lv.lo || rh >= lv.lo;             // max(reg) >= lo, given no NaN (le_hi)
    }
    const float area = (inside && le_hi && ge_lo) ? s[6] : kFcInf;
    // torch.min over dim 1 on CPU tensors: the lowest index among equals, a NaN below every number, the first NaN wins
    if (g == 0 || (best == best && (area < best || area != area))) {
      best = area;
      arg = g;
    }
  }
  float t[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float label = 0.0f;
  if (G > 0) {
    const float* s = sg + arg * kFcRow;
    const float fs = (float)lv.stride;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t[a] = x[a] - s[a];
      t[a + 3] = s[a + 3] - x[a];
    }
    if (norm) {
#pragma unroll
      for (int c = 0; c < 6; ++c) t[c] = t[c] / fs;
    }
    label = best != kFcInf ? 1.0f : 0.0f;
  }
  const int i = lv.base + b * lv.P + p;         // < T: 6 T < 2^31
  labels[i] = label;
#pragma unroll
  for (int c = 0; c < 6; ++c) reg[(size_t)i * 6 + c] = t[c];
  if (ctr != nullptr) ctr[i] = label != 0.0f ? fc_centerness(t) : 0.0f;
  if (matched != nullptr) matched[i] = arg;
  if (valid != nullptr) valid[i] = (x[0] < ori[b * 3] && x[1] < ori[b * 3 + 1] && x[2] < ori[b * 3 + 2]) ? 1 : 0;
}

// ---- losses ----------------------------------------------------------------------------------------------------------
struct FcPred {
  int n;
  int base[kFcMaxLevels], P[kFcMaxLevels];
  const float* cls[kFcMaxLevels];
  const float* reg[kFcMaxLevels];
  const float* ctr[kFcMaxLevels];
};
struct FcGrad {
  float* cls[kFcMaxLevels];
  float* reg[kFcMaxLevels];
  float* ctr[kFcMaxLevels];
};

struct FcWhere {
  int level, j, p, P;
  size_t reg0;                                  // index of channel 0 in the level's planar reg tensor; channels are P apart
};
__device__ __forceinline__ FcWhere fc_where(const FcPred& T, int i) {
  int level = 0;
#pragma unroll
  for (int l = 1; l < kFcMaxLevels; ++l)
    if (l < T.n && i >= T.base[l]) level = l;
  FcWhere w;
  w.level = level;
  int base = T.base[0], P = T.P[0];
#pragma unroll
  for (int l = 1; l < kFcMaxLevels; ++l)
    if (l == level) { base = T.base[l]; P = T.P[l]; }
  w.P = P;
  w.j = i - base;
  const int b = w.j / P;
  w.p = w.j - b * P;
  w.reg0 = (size_t)b * 6 * P + w.p;
  return w;
}
template <typename Ptr>
__device__ __forceinline__ Ptr fc_pick(Ptr const* arr, int level) {
  Ptr r = arr[0];
#pragma unroll
  for (int l = 1; l < kFcMaxLevels; ++l)
    if (l == level) r = arr[l];
  return r;
}

__device__ __forceinline__ float fc_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float fc_bce(float x, float t) { return (fmaxf(x, 0.0f) - x * t) + log1pf(expf(-fabsf(x))); }

struct FcIou {
  float sp[3], in[3], gx[3];                    // per axis: pred extent, intersection, enclosing extent
  float ac, vi, vu, iou;
};
__device__ __forceinline__ FcIou fc_iou(const float* p, const float* t) {
  FcIou r;
  const float tv = ((t[0] + t[3]) * (t[1] + t[4])) * (t[2] + t[5]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.sp[a] = p[a] + p[a + 3];
    r.in[a] = fc_min(p[a], t[a]) + fc_min(p[a + 3], t[a + 3]);
    r.gx[a] = fc_max(p[a], t[a]) + fc_max(p[a + 3], t[a + 3]);
  }
  const float pv = (r.sp[0] * r.sp[1]) * r.sp[2];
  r.ac = (r.gx[0] * r.gx[1]) * r.gx[2] + 1e-7f;
  r.vi = (r.in[0] * r.in[1]) * r.in[2];
  r.vu = (tv + pv) - r.vi;
  r.iou = (r.vi + 1.0f) / (r.vu + 1.0f);
  return r;
}
__device__ __forceinline__ float fc_iou_loss(const FcIou& r, int type) {
  if (type == INR_FCOS_LOSS_IOU) return -logf(r.iou);
  if (type == INR_FCOS_LOSS_LINEAR_IOU) return 1.0f - r.iou;
  return 1.0f - (r.iou - (r.ac - r.vu) / r.ac);
}

// The sum over the workgroup of v[0..4], in a fixed order, valid in thread 0.  red: 4 * 5 doubles of LDS.
__device__ __forceinline__ void fc_block_sum(double* v, double* red) {
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_down(v[k], d, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 5; ++k) red[wave * 5 + k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = ((red[k] + red[5 + k]) + red[10 + k]) + red[15 + k];
}

__global__ __launch_bounds__(kFcBlock) void k_fcos_loss_forward(FcPred T, int total, const float* __restrict__ labels,
                                                                const float* __restrict__ regt,
                                                                const uint8_t* __restrict__ valid, int type,
                                                                float* __restrict__ cls_terms, float* __restrict__ reg_terms,
                                                                float* __restrict__ ctr_terms, double* __restrict__ partial) {
  __shared__ double red[4 * 5];
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};    // focal, regterm, bce, n_pos, sum of centerness
#pragma unroll 1
  for (int k = 0; k < kFcLossPerLane; ++k) {
    const int i = (int)blockIdx.x * kFcLossRun + k * kFcBlock + (int)threadIdx.x;   // < total + 1024 < 2^31 / 6 + 1024
    if (i >= total) break;
    float focal = 0.0f, regterm = 0.0f, bce = 0.0f;
    if (valid == nullptr || valid[i] != 0) {
      const FcWhere w = fc_where(T, i);
      const float t = labels[i];
      const float x = fc_pick(T.cls, w.level)[w.j];
      const float pr = fc_sigmoid(x);
      const float ce = fc_bce(x, t);
      const float pt = pr * t + (1.0f - pr) * (1.0f - t);
      const float q = 1.0f - pt;
      focal = (0.25f * t + 0.75f * (1.0f - t)) * (ce * (q * q));
      acc[0] += (double)focal;
      if (t > 0.0f) {
        float tg[6], pd[6];
        const float* rp = fc_pick(T.reg, w.level) + w.reg0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          tg[c] = regt[(size_t)i * 6 + c];
          pd[c] = rp[(size_t)c * w.P];
        }
        const float cw = fc_centerness(tg);
        regterm = fc_iou_loss(fc_iou(pd, tg), type) * cw;
        bce = fc_bce(fc_pick(T.ctr, w.level)[w.j], cw);
        acc[1] += (double)regterm;
        acc[2] += (double)bce;
        acc[3] += 1.0;
        acc[4] += (double)cw;
      }
    }
    if (cls_terms != nullptr) cls_terms[i] = focal;
    if (reg_terms != nullptr) reg_terms[i] = regterm;
    if (ctr_terms != nullptr) ctr_terms[i] = bce;
  }
  fc_block_sum(acc, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 5; ++k) partial[(size_t)blockIdx.x * 5 + k] = acc[k];
}

__global__ __launch_bounds__(kFcBlock) void k_fcos_loss_finish(const double* __restrict__ partial, int nblocks,
                                                               double* __restrict__ sums, float* __restrict__ losses) {
  __shared__ double red[4 * 5];
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = threadIdx.x; j < nblocks; j += kFcBlock)
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[k] += partial[(size_t)j * 5 + k];
  fc_block_sum(acc, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) sums[k] = acc[k];
    const double n = acc[3] > 1.0 ? acc[3] : 1.0;
    losses[0] = (float)(acc[0] / n);
    losses[1] = acc[3] > 0.0 ? (float)(acc[1] / acc[4]) : 0.0f;
    losses[2] = acc[3] > 0.0 ? (float)(acc[2] / n) : 0.0f;
  }
}

__global__ __launch_bounds__(kFcBlock) void k_fcos_loss_backward(FcPred T, FcGrad D, int total,
                                                                 const float* __restrict__ labels,
                                                                 const float* __restrict__ regt,
                                                                 const uint8_t* __restrict__ valid, int type,
                                                                 const double* __restrict__ norms,
                                                                 const float* __restrict__ gout) {
  const int i = (int)blockIdx.x * kFcBlock + (int)threadIdx.x;
  if (i >= total) return;
  const FcWhere w = fc_where(T, i);
  float dcls = 0.0f, dctr = 0.0f, dreg[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (valid == nullptr || valid[i] != 0) {
    const double npos = norms[0] > 1.0 ? norms[0] : 1.0;
    const float t = labels[i];
    const float x = fc_pick(T.cls, w.level)[w.j];
    const float pr = fc_sigmoid(x);
    const float ce = fc_bce(x, t);
    const float pt = pr * t + (1.0f - pr) * (1.0f - t);
    const float q = 1.0f - pt;
    const float at = 0.25f * t + 0.75f * (1.0f - t);
    const float dfocal = at * ((pr - t) * (q * q) - ((2.0f * q) * ce) * (((2.0f * t - 1.0f) * pr) * (1.0f - pr)));
    dcls = (float)((double)gout[0] / npos) * dfocal;
    if (t > 0.0f) {
      float tg[6], pd[6];
      const float* rp = fc_pick(T.reg, w.level) + w.reg0;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        tg[c] = regt[(size_t)i * 6 + c];
        pd[c] = rp[(size_t)c * w.P];
      }
      const float cw = fc_centerness(tg);
      const FcIou r = fc_iou(pd, tg);
      const float scale = (float)((double)gout[1] / norms[1]) * cw;
      const float U = r.vu + 1.0f;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const int a = c % 3, a1 = (a + 1) % 3, a2 = (a + 2) % 3;
        const float mn = pd[c] < tg[c] ? 1.0f : (pd[c] == tg[c] ? 0.5f : 0.0f);
        const float mx = pd[c] > tg[c] ? 1.0f : (pd[c] == tg[c] ? 0.5f : 0.0f);
        const float dpv = r.sp[a1] * r.sp[a2];
        const float dvi = mn * (r.in[a1] * r.in[a2]);
        const float dac = mx * (r.gx[a1] * r.gx[a2]);
        const float dvu = dpv - dvi;
        const float diou = (dvi * U - (r.vi + 1.0f) * dvu) / (U * U);
        float dl;
        if (type == INR_FCOS_LOSS_IOU) dl = -diou / r.iou;
        else if (type == INR_FCOS_LOSS_LINEAR_IOU) dl = -diou;
        else dl = -(diou + (dvu * r.ac - r.vu * dac) / (r.ac * r.ac));
        dreg[c] = scale * dl;
      }
      dctr = (float)((double)gout[2] / npos) * (fc_sigmoid(fc_pick(T.ctr, w.level)[w.j]) - cw);
    }
  }
  fc_pick(D.cls, w.level)[w.j] = dcls;
  fc_pick(D.ctr, w.level)[w.j] = dctr;
  float* dp = fc_pick(D.reg, w.level) + w.reg0;
#pragma unroll
  for (int c = 0; c < 6; ++c) dp[(size_t)c * w.P] = dreg[c];
}

// ---- host side -------------------------------------------------------------------------------------------------------
bool fc_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// The pyramid's extents -> P per level and T = B * sum P, or a message.  No pointer but level_dims / level_strides is read.
const char* fc_pyramid(const int32_t* level_dims, const int32_t* level_strides, int32_t n_levels, int32_t B, int* P,
                       int64_t* total) {
  if (n_levels < 1 || n_levels > kFcMaxLevels) return "n_levels must be in 1..8 (INR_FCOS_MAX_LEVELS)";
  if (B < 0) return "B must not be negative";
  if (level_dims == nullptr) return "null pointer (level_dims)";
  int64_t sum = 0;
  for (int l = 0; l < n_levels; ++l) {
    int64_t p = 1;
    const int64_t stride = level_strides != nullptr ? level_strides[l] : 1;
    if (stride < 1) return "level_strides: every stride must be at least 1";
    for (int a = 0; a < 3; ++a) {
      const int64_t e = level_dims[l * 3 + a];
      if (e < 1) return "level_dims: every extent must be at least 1";
      if (e * stride >= (1 << 24)) return "level_dims: extent * stride must be below 2^24";
      p *= e;
      if (p >= ((int64_t)1 << 31)) return "level_dims: too many locations: 6*T must be below 2^31";
    }
    P[l] = (int)p;
    sum += p;
  }
  *total = sum * B;
  if (*total * 6 >= ((int64_t)1 << 31)) return "level_dims, B: too many locations: 6*T must be below 2^31";
  return nullptr;
}

const char* fc_loss_args(const float* const* cls_ptrs, const float* const* reg_ptrs, const float* const* ctr_ptrs,
                         const int32_t* level_dims, int32_t n_levels, int32_t B, int32_t type, FcPred* T, int64_t* total) {
  if (n_levels >= 1 && n_levels <= kFcMaxLevels && B >= 0 && (!cls_ptrs || !reg_ptrs || !ctr_ptrs))
    return "null pointer (cls_ptrs, reg_ptrs, ctr_ptrs)";
  const char* why = fc_pyramid(level_dims, nullptr, n_levels, B, T->P, total);
  if (why != nullptr) return why;
  if (type != INR_FCOS_LOSS_IOU && type != INR_FCOS_LOSS_LINEAR_IOU && type != INR_FCOS_LOSS_GIOU)
    return "iou_loss_type must be INR_FCOS_LOSS_IOU (0), _LINEAR_IOU (1) or _GIOU (2)";
  T->n = n_levels;
  int64_t base = 0;
  for (int l = 0; l < kFcMaxLevels; ++l) {
    const bool on = l < n_levels;
    T->base[l] = on ? (int)base : 0x7fffffff;
    if (!on) T->P[l] = 1;
    T->cls[l] = on ? cls_ptrs[l] : nullptr;
    T->reg[l] = on ? reg_ptrs[l] : nullptr;
    T->ctr[l] = on ? ctr_ptrs[l] : nullptr;
    if (on) base += (int64_t)B * T->P[l];
  }
  return nullptr;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_fcos_targets(const int32_t* level_dims, const int32_t* level_strides, const float* level_ranges, int32_t n_levels,
                     int32_t B, const float* gt, const int32_t* gt_offsets, int32_t max_gt, const float* ori_sizes,
                     float radius, int32_t norm_reg_targets, float* labels, float* reg_targets, float* centerness,
                     int32_t* matched, uint8_t* valid, inr_stream_t s) {
  int P[kFcMaxLevels];
  int64_t total = 0;
  INR_REQUIRE(!(n_levels >= 1 && n_levels <= kFcMaxLevels && B >= 0) || (level_dims && level_strides && level_ranges),
              "null pointer (level_dims, level_strides, level_ranges)");
  const char* why = fc_pyramid(level_dims, level_strides, n_levels, B, P, &total);
  INR_REQUIRE(why == nullptr, why);
  INR_REQUIRE(max_gt >= 0 && max_gt <= kFcMaxGt, "max_gt must be in 0..1024 (INR_FCOS_MAX_GT)");
  INR_REQUIRE(radius >= 0.0f, "radius must not be negative (or NaN)");
  if (total == 0) return INR_OK;
  INR_REQUIRE(gt_offsets && labels && reg_targets && (gt || max_gt == 0),
              "null pointer (gt, gt_offsets, labels, reg_targets)");
  INR_REQUIRE(valid == nullptr || ori_sizes != nullptr, "valid needs ori_sizes");
  INR_REQUIRE(fc_aligned(gt, 4) && fc_aligned(gt_offsets, 4) && fc_aligned(ori_sizes, 4) && fc_aligned(labels, 4) &&
                  fc_aligned(reg_targets, 4) && fc_aligned(centerness, 4) && fc_aligned(matched, 4),
              "misaligned pointer (gt, gt_offsets, ori_sizes, labels, reg_targets, centerness and matched are 4-byte aligned)");
  FcTable T;
  T.n = n_levels;
  int64_t block = 0, base = 0;
  for (int l = 0; l < kFcMaxLevels; ++l) {
    FcLevel& e = T.lv[l];
    if (l >= n_levels) {
      e = T.lv[0];
      e.first_block = 0x7fffffff;
      continue;
    }
    e.L = level_dims[l * 3 + 1];
    e.H = level_dims[l * 3 + 2];
    e.stride = level_strides[l];
    e.P = P[l];
    e.blocks_per_scene = (int)blocks_for(P[l], kFcRun);
    e.first_block = (int)block;
    e.base = (int)base;
    e.lo = level_ranges[l * 2];
    e.hi = level_ranges[l * 2 + 1];
    e.s = (float)((double)e.stride * (double)radius);
    block += (int64_t)e.blocks_per_scene * B;   // <= T: below 2^31 / 6
    base += (int64_t)P[l] * B;
  }
  k_fcos_targets<<<(unsigned)block, kFcBlock, (size_t)std::max(max_gt, 1) * kFcRow * 4, as_stream(s)>>>(
      T, gt, gt_offsets, max_gt, ori_sizes, radius > 0.0f, norm_reg_targets != 0, labels, reg_targets, centerness, matched,
      valid);
  return check_launch("inr_fcos_targets");
}

int64_t inr_fcos_loss_workspace_bytes(int64_t T) {
  if (T < 0 || T * 6 >= ((int64_t)1 << 31)) {
    set_error("%s: T must be in 0..2^31/6 (6*T below 2^31)", __func__);
    return INR_EINVAL;
  }
  return (int64_t)std::max<int64_t>(blocks_for(T, kFcLossRun), 1) * 5 * 8;
}

int inr_fcos_loss_forward(const float* const* cls_ptrs, const float* const* reg_ptrs, const float* const* ctr_ptrs,
                          const int32_t* level_dims, int32_t n_levels, int32_t B, const float* labels,
                          const float* reg_targets, const uint8_t* valid, int32_t iou_loss_type, double* sums, float* losses,
                          float* cls_terms, float* reg_terms, float* ctr_terms, void* workspace, int64_t workspace_bytes,
                          inr_stream_t s) {
  FcPred T;
  int64_t total = 0;
  const char* why = fc_loss_args(cls_ptrs, reg_ptrs, ctr_ptrs, level_dims, n_levels, B, iou_loss_type, &T, &total);
  INR_REQUIRE(why == nullptr, why);
  INR_REQUIRE(workspace_bytes >= 0, "workspace_bytes must not be negative");
  if (total == 0) return INR_OK;
  const int64_t nblocks = blocks_for(total, kFcLossRun);
  INR_REQUIRE(labels && reg_targets && sums && losses && workspace, "null pointer (labels, reg_targets, sums, losses, workspace)");
  for (int l = 0; l < n_levels; ++l) {
    INR_REQUIRE(T.cls[l] && T.reg[l] && T.ctr[l], "null pointer in cls_ptrs, reg_ptrs or ctr_ptrs");
    INR_REQUIRE(fc_aligned(T.cls[l], 4) && fc_aligned(T.reg[l], 4) && fc_aligned(T.ctr[l], 4),
                "misaligned pointer in cls_ptrs, reg_ptrs or ctr_ptrs (4 bytes)");
  }
  INR_REQUIRE(workspace_bytes >= nblocks * 5 * 8, "workspace_bytes is too small (inr_fcos_loss_workspace_bytes)");
  INR_REQUIRE(fc_aligned(sums, 8) && fc_aligned(workspace, 8), "misaligned sums or workspace (8 bytes)");
  INR_REQUIRE(fc_aligned(labels, 4) && fc_aligned(reg_targets, 4) && fc_aligned(losses, 4) && fc_aligned(cls_terms, 4) &&
                  fc_aligned(reg_terms, 4) && fc_aligned(ctr_terms, 4),
              "misaligned pointer (labels, reg_targets, losses and the term arrays are 4-byte aligned)");
  hipStream_t st = as_stream(s);
  double* partial = static_cast<double*>(workspace);
  k_fcos_loss_forward<<<(unsigned)nblocks, kFcBlock, 0, st>>>(T, (int)total, labels, reg_targets, valid, iou_loss_type,
                                                             cls_terms, reg_terms, ctr_terms, partial);
  const int rc = check_launch("inr_fcos_loss_forward");
  if (rc != INR_OK) return rc;
  k_fcos_loss_finish<<<1, kFcBlock, 0, st>>>(partial, (int)nblocks, sums, losses);
  return check_launch("inr_fcos_loss_forward (finish)");
}

int inr_fcos_loss_backward(const float* const* cls_ptrs, const float* const* reg_ptrs, const float* const* ctr_ptrs,
                           const int32_t* level_dims, int32_t n_levels, int32_t B, const float* labels,
                           const float* reg_targets, const uint8_t* valid, int32_t iou_loss_type, const double* norms,
                           const float* grad_losses, float* const* d_cls_ptrs, float* const* d_reg_ptrs,
                           float* const* d_ctr_ptrs, inr_stream_t s) {
  FcPred T;
  int64_t total = 0;
  INR_REQUIRE(!(n_levels >= 1 && n_levels <= kFcMaxLevels && B >= 0) || (d_cls_ptrs && d_reg_ptrs && d_ctr_ptrs),
              "null pointer (d_cls_ptrs, d_reg_ptrs, d_ctr_ptrs)");
  const char* why = fc_loss_args(cls_ptrs, reg_ptrs, ctr_ptrs, level_dims, n_levels, B, iou_loss_type, &T, &total);
  INR_REQUIRE(why == nullptr, why);
  if (total == 0) return INR_OK;
  INR_REQUIRE(labels && reg_targets && norms && grad_losses, "null pointer (labels, reg_targets, norms, grad_losses)");
  FcGrad D;
  for (int l = 0; l < kFcMaxLevels; ++l) {
    const bool on = l < n_levels;
    D.cls[l] = on ? d_cls_ptrs[l] : nullptr;
    D.reg[l] = on ? d_reg_ptrs[l] : nullptr;
    D.ctr[l] = on ? d_ctr_ptrs[l] : nullptr;
    if (!on) continue;
    INR_REQUIRE(T.cls[l] && T.reg[l] && T.ctr[l] && D.cls[l] && D.reg[l] && D.ctr[l],
                "null pointer in cls_ptrs, reg_ptrs, ctr_ptrs, d_cls_ptrs, d_reg_ptrs or d_ctr_ptrs");
    INR_REQUIRE(fc_aligned(T.cls[l], 4) && fc_aligned(T.reg[l], 4) && fc_aligned(T.ctr[l], 4) && fc_aligned(D.cls[l], 4) &&
                    fc_aligned(D.reg[l], 4) && fc_aligned(D.ctr[l], 4),
                "misaligned pointer in cls_ptrs, reg_ptrs, ctr_ptrs, d_cls_ptrs, d_reg_ptrs or d_ctr_ptrs (4 bytes)");
  }
  INR_REQUIRE(fc_aligned(norms, 8), "misaligned norms (8 bytes)");
  INR_REQUIRE(fc_aligned(labels, 4) && fc_aligned(reg_targets, 4) && fc_aligned(grad_losses, 4),
              "misaligned pointer (labels, reg_targets and grad_losses are 4-byte aligned)");
  k_fcos_loss_backward<<<blocks_for(total, kFcBlock), kFcBlock, 0, as_stream(s)>>>(T, D, (int)total, labels, reg_targets,
                                                                                  valid, iou_loss_type, norms, grad_losses);
  return check_launch("inr_fcos_loss_backward");
}

}  // extern "C"
