// Matching of 2-D segments to projected 3-D masks (include/inr.h, "2-D mask matching").  Everything is integer counting
// with integer atomics plus one fp64 division per (segment, candidate), so two calls give identical bits.
//
//   pack:    k_pack_bits     one thread per (ray, 32 candidates): compares 32 soft sums and stores one word.
//   count:   k_match_zero    zeroes seg_area, inter and status in one launch.
//            k_match_count   the hot one.  A workgroup owns a run of pixels of one view and one word (32 candidates) and
//                            keeps that word's (S + 1) x 32 slice of `inter` in LDS.  Per step a wave looks at 64
//                            consecutive pixels; lanes that hold the same (rank, word value) pair - neighbouring pixels
//                            nearly always do - are found by ballot and counted once: lane l < 32 adds the size of the
//                            group to column l if bit l of the word is set (one conflict-free LDS atomic instruction per
//                            distinct pair), lane 32 adds it to the rank's area.  Non-zero entries are flushed with
//                            global integer adds.  Row 0 collects the pixels outside every segment (seg <= 0).
//            k_match_colsum  mask_area[j] = sum over the rows of inter[.][j] (every valid pixel is in exactly one row).
//   assign:  k_match_pick    one thread per (view, rank): fp64 IoU, first argmax, threshold.
//            k_match_apply   one thread per pixel.
#include "common.h"

namespace inr {
namespace {

constexpr int kMtBlock = 256;
constexpr int kMaxS = 1023, kMaxK = 1024;

__global__ __launch_bounds__(kMtBlock) void k_pack_bits(const float* __restrict__ soft, const int64_t* __restrict__ inds,
                                                        int64_t N, int k, int nw, float thresh, int64_t P,
                                                        uint32_t* __restrict__ words) {
  const int64_t t = (int64_t)blockIdx.x * kMtBlock + threadIdx.x;
  if (t >= N * nw) return;
  const int64_t n = t / nw;
  const int w = (int)(t % nw);
  const int64_t p = inds != nullptr ? inds[n] : n;
  if (p < 0 || p >= P) return;
  const float* row = soft + n * k + 32 * w;
  const int cols = min(32, k - 32 * w);
  uint32_t bits = 0;
  for (int j = 0; j < cols; ++j) bits |= (row[j] > thresh ? 1u : 0u) << j;          // NaN > thresh is false
  words[(int64_t)w * P + p] = bits;
}

__global__ __launch_bounds__(kMtBlock) void k_match_zero(int* seg_area, int64_t n_area, int* inter, int64_t n_inter,
                                                         int* status) {
  const int64_t stride = (int64_t)gridDim.x * kMtBlock;
  const int64_t t = (int64_t)blockIdx.x * kMtBlock + threadIdx.x;
  for (int64_t i = t; i < n_area; i += stride) seg_area[i] = 0;
  for (int64_t i = t; i < n_inter; i += stride) inter[i] = 0;
  if (t == 0) status[0] = 0;
}

// grid: x = run of pixels, y strides over the (view, word) pairs.  Dynamic LDS: hist int [(S + 1) * 32], area int [S + 1].
__global__ __launch_bounds__(kMtBlock) void k_match_count(const int* __restrict__ seg, const uint32_t* __restrict__ words,
                                                          int64_t pairs, int nwq, int64_t P, int S, int k, int64_t run,
                                                          int* seg_area, int* inter, int* status) {
  extern __shared__ int lds[];
  int* hist = lds;
  int* area = lds + (S + 1) * 32;
  const int n_hist = (S + 1) * 32;
  const int lane = threadIdx.x & 63;
  const int64_t p0 = (int64_t)blockIdx.x * run, p1 = min(P, p0 + run);
  bool bad = false;

  for (int64_t pair = blockIdx.y; pair < pairs; pair += gridDim.y) {
    const int64_t b = pair / nwq;
    const int w = (int)(pair % nwq);
    const bool with_area = w == 0;
    const bool with_words = k > 0;
    for (int i = threadIdx.x; i < n_hist; i += kMtBlock) hist[i] = 0;
    for (int i = threadIdx.x; i <= S; i += kMtBlock) area[i] = 0;
    __syncthreads();

    const int* sg = seg + b * P;
    const uint32_t* wd = with_words ? words + (b * nwq + w) * P : nullptr;
    // every wave takes the same number of steps: the ballots below need all 64 lanes
    for (int64_t base = p0 + (threadIdx.x & ~63); base < p1; base += kMtBlock) {
      const int64_t p = base + lane;
      int row = 0;
      uint32_t m = 0;
      bool active = false;
      if (p < p1) {
        const int s = sg[p];
        if (s < -1 || s > S) {
          bad = true;
        } else {
          row = max(s, 0);
          m = with_words ? wd[p] : 0u;
          active = with_area || m != 0;
        }
      }
      unsigned long long todo = __ballot(active);
      while (todo) {
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const int row0 = __builtin_amdgcn_readlane(row, leader);
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_readlane((int)m, leader);
        const unsigned long long same = __ballot(active && row == row0 && m == m0);
        const int cnt = __popcll(same);
        if (lane < 32) {
          if ((m0 >> lane) & 1u) atomicAdd(&hist[row0 * 32 + lane], cnt);
        } else if (lane == 32 && with_area) {
          atomicAdd(&area[row0], cnt);
        }
        todo &= ~same;
      }
    }
    __syncthreads();

    for (int i = threadIdx.x; i < n_hist; i += kMtBlock) {
      const int v = hist[i];
      const int col = w * 32 + (i & 31);
      if (v != 0 && col < k) atomicAdd(&inter[(b * (S + 1) + (i >> 5)) * k + col], v);
    }
    if (with_area)
      for (int i = threadIdx.x; i <= S; i += kMtBlock)
        if (area[i] != 0) atomicAdd(&seg_area[b * (S + 1) + i], area[i]);
    __syncthreads();
  }
  if (bad) atomicOr(status, 1);
}

__global__ __launch_bounds__(kMtBlock) void k_match_colsum(const int* __restrict__ inter, int64_t B, int S, int k,
                                                           int* __restrict__ mask_area) {
  const int64_t t = (int64_t)blockIdx.x * kMtBlock + threadIdx.x;
  if (t >= B * k) return;
  const int64_t b = t / k;
  const int j = (int)(t % k);
  const int* col = inter + b * (S + 1) * k + j;
  int sum = 0;
#pragma unroll 8                // independent loads: eight in flight instead of one
  for (int r = 0; r <= S; ++r) sum += col[(int64_t)r * k];
  mask_area[t] = sum;
}

__global__ __launch_bounds__(kMtBlock) void k_match_pick(const int* __restrict__ seg_area, const int* __restrict__ mask_area,
                                                         const int* __restrict__ inter, const int* __restrict__ ids,
                                                         int64_t B, int S, int k, double iou_thresh,
                                                         int* __restrict__ assigned) {
  const int64_t t = (int64_t)blockIdx.x * kMtBlock + threadIdx.x;
  if (t >= B * (S + 1)) return;
  const int64_t b = t / (S + 1);
  const int r = (int)(t % (S + 1));
  int result = -1;
  const int a = seg_area[t];
  if (r == 0) {
    result = 0;
  } else if (a > 0 && k > 0) {
    const int* in = inter + t * k;
    const int* ma = mask_area + b * k;
    double best = -1.0;
    int best_j = 0;
    for (int j = 0; j < k; ++j) {
      const int i = in[j];
      const double iou = (double)i / (double)(a + (ma[j] - i));          // the union is >= a > 0
      if (iou > best) {
        best = iou;
        best_j = j;
      }
    }
    if (best > iou_thresh) result = ids[best_j];
  }
  assigned[t] = result;
}

__global__ __launch_bounds__(kMtBlock) void k_match_apply(const int* __restrict__ seg, const int* __restrict__ assigned,
                                                          int64_t total, int64_t P, int S, int* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kMtBlock + threadIdx.x;
  if (t >= total) return;
  const int s = seg[t];
  int v = -1;
  if (s == 0) v = 0;
  else if (s > 0 && s <= S) v = assigned[(t / P) * (S + 1) + s];
  out[t] = v;
}

// the limits the count and assign exports share; `who` names the export in the message
bool match_sizes(int64_t B, int64_t P, int32_t S, int32_t k, const char* who) {
  if (B < 1 || P < 1) {
    set_error("%s: bad size (B and P must be >= 1)", who);
    return false;
  }
  if (B > INT32_MAX || P > INT32_MAX || B * P > INT32_MAX) {
    set_error("%s: B * P must be below 2^31 (pixel counts are int32)", who);
    return false;
  }
  if (S < 0 || S > kMaxS) {
    set_error("%s: S must be 0..1023 (the (S + 1) x 32 counters of one word live in LDS)", who);
    return false;
  }
  if (k < 0 || k > kMaxK) {
    set_error("%s: k must be 0..1024", who);
    return false;
  }
  return true;
}

struct CountAttr {
  bool done[64] = {};
};
CountAttr g_count_attr;

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" int inr_pack_mask_bits(const float* soft, const int64_t* inds, int64_t N, int32_t k, float thresh, int64_t P,
                                  uint32_t* words, inr_stream_t s) {
  INR_REQUIRE(N >= 0 && P >= 1, "bad size (N must be >= 0, P >= 1)");
  INR_REQUIRE(k >= 1 && k <= kMaxK, "k must be 1..1024");
  INR_REQUIRE(P <= INT32_MAX && N <= INT32_MAX, "N and P must be below 2^31");
  INR_REQUIRE(words != nullptr && (soft != nullptr || N == 0), "null pointer");
  INR_REQUIRE((((uintptr_t)soft | (uintptr_t)words) & 3) == 0 && ((uintptr_t)inds & 7) == 0,
              "misaligned soft, words (4 bytes) or inds (8 bytes)");
  INR_REQUIRE(thresh == thresh, "thresh is NaN");
  const int nw = (k + 31) / 32;
  hipStream_t st = as_stream(s);
  if (hipMemsetAsync(words, 0, (size_t)nw * (size_t)P * 4, st) != hipSuccess) return check_launch("inr_pack_mask_bits");
  if (N > 0)
    hipLaunchKernelGGL(k_pack_bits, dim3(blocks_for(N * nw, kMtBlock)), dim3(kMtBlock), 0, st, soft, inds, N, k, nw, thresh, P,
                       words);
  return check_launch("inr_pack_mask_bits");
}

extern "C" int inr_match_count(const int32_t* seg, const uint32_t* words, int64_t B, int64_t P, int32_t S, int32_t k,
                               int32_t* seg_area, int32_t* mask_area, int32_t* inter, int32_t* status, inr_stream_t s) {
  if (!match_sizes(B, P, S, k, __func__)) return INR_EINVAL;
  INR_REQUIRE(seg != nullptr && seg_area != nullptr && status != nullptr, "null pointer");
  INR_REQUIRE(k == 0 || (words != nullptr && mask_area != nullptr && inter != nullptr), "null pointer (words, mask_area, inter)");
  INR_REQUIRE((((uintptr_t)seg | (uintptr_t)words | (uintptr_t)seg_area | (uintptr_t)mask_area | (uintptr_t)inter |
                (uintptr_t)status) & 3) == 0, "misaligned buffer (4 bytes)");
  const int nwq = std::max((k + 31) / 32, 1);
  const int64_t pairs = B * nwq;
  const size_t lds = (size_t)(S + 1) * 33 * sizeof(int);
  // runs of pixels per (view, word): enough workgroups to fill the machine, but a run no shorter than the LDS slice,
  // which every workgroup zeroes and flushes once per pair
  const int64_t min_run = std::max<int64_t>(4096, (int64_t)(S + 1) * 32);
  const int64_t want = ((int64_t)cu_count() * 8 + pairs - 1) / pairs;
  const int64_t runs = std::max<int64_t>(1, std::min(want, (P + min_run - 1) / min_run));
  const int64_t run = ((P + runs - 1) / runs + 63) / 64 * 64;
  const unsigned gx = (unsigned)((P + run - 1) / run), gy = (unsigned)std::min<int64_t>(pairs, 65535);
  if (lds > 64 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
      set_error("%s: no current device", __func__);
      return INR_ENODEV;
    }
    if (!g_count_attr.done[dev]) {
      if (hipFuncSetAttribute((const void*)k_match_count, hipFuncAttributeMaxDynamicSharedMemorySize, (kMaxS + 1) * 33 * 4) !=
          hipSuccess)
        return check_launch("inr_match_count (LDS size)");
      g_count_attr.done[dev] = true;
    }
  }
  hipStream_t st = as_stream(s);
  const int64_t n_area = B * (S + 1), n_inter = n_area * k;
  const unsigned zb = (unsigned)std::min<int64_t>(blocks_for(std::max(n_inter, n_area), kMtBlock), 4096);
  hipLaunchKernelGGL(k_match_zero, dim3(zb), dim3(kMtBlock), 0, st, seg_area, n_area, inter, n_inter, status);
  hipLaunchKernelGGL(k_match_count, dim3(gx, gy), dim3(kMtBlock), lds, st, seg, words, pairs, nwq, P, S, k, run, seg_area, inter,
                     status);
  if (k > 0)
    hipLaunchKernelGGL(k_match_colsum, dim3(blocks_for(B * k, kMtBlock)), dim3(kMtBlock), 0, st, inter, B, S, k, mask_area);
  return check_launch("inr_match_count");
}

extern "C" int inr_match_assign(const int32_t* seg, const int32_t* seg_area, const int32_t* mask_area, const int32_t* inter,
                                const int32_t* instance_ids, int64_t B, int64_t P, int32_t S, int32_t k,
                                const double* iou_thresh, int32_t* assigned, int32_t* out, inr_stream_t s) {
  if (!match_sizes(B, P, S, k, __func__)) return INR_EINVAL;
  INR_REQUIRE(seg != nullptr && seg_area != nullptr && assigned != nullptr && out != nullptr && iou_thresh != nullptr,
              "null pointer");
  INR_REQUIRE(k == 0 || (mask_area != nullptr && inter != nullptr && instance_ids != nullptr),
              "null pointer (mask_area, inter, instance_ids)");
  INR_REQUIRE((((uintptr_t)seg | (uintptr_t)seg_area | (uintptr_t)mask_area | (uintptr_t)inter | (uintptr_t)instance_ids |
                (uintptr_t)assigned | (uintptr_t)out) & 3) == 0 && ((uintptr_t)iou_thresh & 7) == 0,
              "misaligned buffer (4 bytes; iou_thresh 8 bytes)");
  const double thresh = *iou_thresh;
  INR_REQUIRE(thresh >= 0.0 && thresh <= 1.0, "iou_thresh must lie in [0, 1]");
  hipStream_t st = as_stream(s);
  hipLaunchKernelGGL(k_match_pick, dim3(blocks_for(B * (S + 1), kMtBlock)), dim3(kMtBlock), 0, st, seg_area, mask_area, inter,
                     instance_ids, B, S, k, thresh, assigned);
  hipLaunchKernelGGL(k_match_apply, dim3(blocks_for(B * P, kMtBlock)), dim3(kMtBlock), 0, st, seg, assigned, B * P, P, S, out);
  return check_launch("inr_match_assign");
}
