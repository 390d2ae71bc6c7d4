// Confusion matrix of rendered instance maps (include/inr.h, "Segmentation confusion matrix of rendered instance maps").
//
// Both kernels: 1-D grid over (image, pixel run), 256 threads.  A workgroup owns kCfRun consecutive pixels of one image
// and keeps that image's K x (K + 1) counters as int32 in LDS (16,640 B at K = 64; a counter holds at most kCfRun).
// Every pixel is one LDS integer add (cf_add); at the end the non-zero counters go out as one 64-bit global integer add
// each (cf_flush): integer arithmetic only, so the result does not depend on the order of arrival.
//
// k_confusion_ids:     lane per pixel, both id maps read as coalesced dwords, four pixels per lane in flight.
// k_confusion_logits:  the run is walked in steps of P pixels.  The step's P x K floats (channels >= K are never touched)
//                      are read coalesced - 16 B per lane when K, ld and the base allow it, 4 B otherwise - into LDS rows of
//                      K | 1 floats; the odd stride lets lane q scan row q without bank conflicts for the arg-max.
//                      LDS: 16,640 (counters) + 33,280 (stage) + 4 B = 49,924 B -> 3 workgroups per CU.
#include "common.h"

namespace inr {
namespace {

constexpr int kCfBlock = INR_CONFUSION_BLOCK;
constexpr int kCfRun = INR_CONFUSION_PIXELS_PER_WG;
constexpr int kCfMaxK = INR_CONFUSION_MAX_K;
constexpr int kCfHist = kCfMaxK * (kCfMaxK + 1);
constexpr int kCfStageRows = 128;                              // rows of the stage at K = 64
constexpr int kCfStage = kCfStageRows * (kCfMaxK | 1);         // floats
constexpr int kCfMaxStep = 1024;
constexpr int kCfPerLane = kCfRun / kCfBlock;
static_assert(kCfRun % kCfBlock == 0, "a run is a whole number of pixels per lane");

__device__ __forceinline__ void cf_zero(int* hist, int K, int* ign) {
  for (int i = threadIdx.x; i < K * (K + 1); i += kCfBlock) hist[i] = 0;
  if (threadIdx.x == 0) *ign = 0;
}

// One pixel.  A truth outside [0, K) is ignored (counted by the caller's `mine`); a prediction outside goes to column K.
__device__ __forceinline__ void cf_add(int* hist, int K, int t, int p, int& mine) {
  if ((unsigned)t >= (unsigned)K) {
    ++mine;
    return;
  }
  const int col = (unsigned)p < (unsigned)K ? p : K;
  atomicAdd(&hist[t * (K + 1) + col], 1);
}

// After the last cf_add of the workgroup: a barrier inside, then the non-zero counters are added to the image's matrix.
__device__ __forceinline__ void cf_flush(const int* hist, int K, int* ign, int mine, int64_t b, int64_t* counts,
                                         int64_t* ignored) {
  if (mine != 0) atomicAdd(ign, mine);
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts) + b * K * (K + 1);
  for (int i = threadIdx.x; i < K * (K + 1); i += kCfBlock) {
    const int v = hist[i];
    if (v != 0) atomicAdd(out + i, (unsigned long long)v);
  }
  if (threadIdx.x == 0 && *ign != 0) atomicAdd(reinterpret_cast<unsigned long long*>(ignored) + b, (unsigned long long)*ign);
}

__global__ __launch_bounds__(kCfBlock) void k_confusion_ids(const int* __restrict__ pred, const int* __restrict__ truth,
                                                             int64_t N, int K, unsigned runs, int64_t* counts,
                                                             int64_t* ignored) {
  __shared__ int hist[kCfHist];
  __shared__ int ign;
  const int64_t b = blockIdx.x / runs;
  const int64_t p0 = (int64_t)(blockIdx.x % runs) * kCfRun;
  const int n = (int)min((int64_t)kCfRun, N - p0);
  cf_zero(hist, K, &ign);
  const int* pr = pred + b * N + p0;
  const int* tr = truth + b * N + p0;
  int t[kCfPerLane], p[kCfPerLane];
#pragma unroll
  for (int i = 0; i < kCfPerLane; ++i) {
    const int q = threadIdx.x + i * kCfBlock;
    t[i] = q < n ? tr[q] : 0;
    p[i] = q < n ? pr[q] : 0;
  }
  __syncthreads();
  int mine = 0;
#pragma unroll
  for (int i = 0; i < kCfPerLane; ++i)
    if ((int)threadIdx.x + i * kCfBlock < n) cf_add(hist, K, t[i], p[i], mine);
  cf_flush(hist, K, &ign, mine, b, counts, ignored);
}

// Lowest index of the maximum of r[0..K), NaN above every number (include/inr.h, "Arg-max rule").
__device__ __forceinline__ int cf_argmax(const float* r, int K) {
  float best = r[0];
  int arg = 0;
  for (int c = 1; c < K; ++c) {
    const float v = r[c];
    if (best == best && (v > best || v != v)) {        // a NaN, once found, is never replaced
      best = v;
      arg = c;
    }
  }
  return arg;
}

// Copies the first W * kVec floats of `rows` consecutive rows (stride ld) into LDS rows of stride Kp, kVec floats per lane.
template <int kVec>
__device__ __forceinline__ void cf_stage(const float* __restrict__ src, int64_t ld, int rows, int W, int Kp, float* stage) {
  int row = threadIdx.x / W, c = threadIdx.x % W;
  const int dr = kCfBlock / W, dc = kCfBlock % W;
#pragma unroll 4
  for (int j = threadIdx.x; j < rows * W; j += kCfBlock) {
    const float* g = src + row * ld + kVec * c;
    float* d = stage + row * Kp + kVec * c;
    if (kVec == 4) {
      const float4 v = *reinterpret_cast<const float4*>(g);
      d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    } else {
      d[0] = g[0];
    }
    row += dr, c += dc;
    if (c >= W) c -= W, ++row;
  }
}

__global__ __launch_bounds__(kCfBlock) void k_confusion_logits(const float* __restrict__ logits, const int* __restrict__ truth,
                                                                int64_t N, int K, int64_t ld, int P, int vec, unsigned runs,
                                                                int64_t* counts, int64_t* ignored) {
  __shared__ int hist[kCfHist];
  __shared__ float stage[kCfStage];
  __shared__ int ign;
  const int64_t b = blockIdx.x / runs;
  const int64_t p0 = (int64_t)(blockIdx.x % runs) * kCfRun;
  const int n = (int)min((int64_t)kCfRun, N - p0);
  const int Kp = K | 1;
  cf_zero(hist, K, &ign);          // the first barrier of the loop below orders this before every cf_add
  int mine = 0;
  for (int s0 = 0; s0 < n; s0 += P) {
    const int np = min(P, n - s0);
    const int64_t first = b * N + p0 + s0;
    if (vec) cf_stage<4>(logits + first * ld, ld, np, K >> 2, Kp, stage);
    else cf_stage<1>(logits + first * ld, ld, np, K, Kp, stage);
    __syncthreads();
    for (int q = threadIdx.x; q < np; q += kCfBlock) {
      const int t = truth[first + q];
      cf_add(hist, K, t, cf_argmax(stage + q * Kp, K), mine);
    }
    __syncthreads();               // the next step overwrites the stage
  }
  cf_flush(hist, K, &ign, mine, b, counts, ignored);
}

// Shared by both entry points: the message for sizes the kernels do not take, or null; `runs` = workgroups per image.
const char* cf_sizes(int64_t B, int64_t N, int32_t K, int64_t ld, int64_t* runs) {
  if (B < 0) return "B must not be negative";
  if (N < 0) return "N must not be negative";
  if (K < 1 || K > kCfMaxK) return "K must be in 1..64 (INR_CONFUSION_MAX_K)";
  if (ld < K) return "ld must be at least K";
  *runs = N / kCfRun + (N % kCfRun != 0);
  if (B == 0 || N == 0) return nullptr;
  if (N > INT64_MAX / B || B * N > INT64_MAX / ld) return "B*N*ld must be below 2^63";
  if (*runs > (int64_t)INT32_MAX / B) return "too many workgroups: B * ceil(N / 1024) must be below 2^31";
  return nullptr;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" {

int inr_confusion_ids(const int32_t* pred, const int32_t* truth, int64_t B, int64_t N, int32_t K, int64_t* counts,
                      int64_t* ignored, inr_stream_t s) {
  int64_t runs = 0;
  const char* why = cf_sizes(B, N, K, K, &runs);
  INR_REQUIRE(why == nullptr, why);
  if (B == 0 || N == 0) return INR_OK;
  INR_REQUIRE(pred && truth && counts && ignored, "null pointer (pred, truth, counts, ignored)");
  INR_REQUIRE(((uintptr_t)counts & 7) == 0, "counts is misaligned: it must be 8-byte aligned");
  INR_REQUIRE(((uintptr_t)ignored & 7) == 0, "ignored is misaligned: it must be 8-byte aligned");
  k_confusion_ids<<<(unsigned)(B * runs), kCfBlock, 0, as_stream(s)>>>(pred, truth, N, K, (unsigned)runs, counts, ignored);
  return check_launch("confusion_ids");
}

int inr_confusion_logits(const float* logits, const int32_t* truth, int64_t B, int64_t N, int32_t K, int64_t ld,
                         int64_t* counts, int64_t* ignored, inr_stream_t s) {
  int64_t runs = 0;
  const char* why = cf_sizes(B, N, K, ld, &runs);
  INR_REQUIRE(why == nullptr, why);
  if (B == 0 || N == 0) return INR_OK;
  INR_REQUIRE(logits && truth && counts && ignored, "null pointer (logits, truth, counts, ignored)");
  INR_REQUIRE(((uintptr_t)counts & 7) == 0, "counts is misaligned: it must be 8-byte aligned");
  INR_REQUIRE(((uintptr_t)ignored & 7) == 0, "ignored is misaligned: it must be 8-byte aligned");
  const int Kp = K | 1;
  int P = std::min(kCfMaxStep, kCfStage / Kp / kCfBlock * kCfBlock);      // whole blocks of pixels per step ...
  if (P == 0) P = kCfStageRows;                                           // ... or half a block where the rows are long
  const int vec = K % 4 == 0 && ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  k_confusion_logits<<<(unsigned)(B * runs), kCfBlock, 0, as_stream(s)>>>(logits, truth, N, K, ld, P, vec, (unsigned)runs,
                                                                          counts, ignored);
  return check_launch("confusion_logits");
}

}  // extern "C"
