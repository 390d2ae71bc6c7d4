// The tail of the 3-D detector (include/inr.h, "Detector tail"): per-class 3-D NMS and the pasting of M^3 mask
// probabilities into the scene grid, straight to BIT PLANES (overlap.hip's layout: bit v % 64 of word v / 64 = the mask
// holds flattened voxel v), plus the conversion of bit planes to the projector's 32-masks-per-voxel words.
//
//   paste:  k_paste_masks            grid (run of kPasteRun words, mask).  A wave takes 64 consecutive voxels, one per lane:
//                                    the lane resamples the mask at its voxel (torch's grid_sample, 3-D, bilinear, zeros
//                                    padding, align_corners=True, in fp32 in torch's operation order, NO contraction: the
//                                    bits of the reference's whole-volume path), one ballot of acc >= thresh is one word.
//                                    Eight words are gathered before lanes 0..7 store them (64 contiguous bytes).  Texels
//                                    are read through the vector cache: a mask is 32 KB at M = 20.  A workgroup whose
//                                    voxels all lie outside the mask's support along W stores zeros without sampling; the
//                                    decision evaluates the SAME coordinate arithmetic at the run's first and last w, and
//                                    every step of that arithmetic is monotone in w, so it never drops a set bit.
//                                    Set bits are counted as they go: per lane, LDS integer add, one global integer add
//                                    per (mask, workgroup).
//           k_planes_to_voxel_words  a wave takes 8 words of up to 32 planes (four 8-byte loads per lane, 64 contiguous
//                                    bytes per plane), and writes 8 x 64 int32 voxel words (256 contiguous bytes each);
//                                    the 32 x 64 bit transposes go through v_readlane with constant lane numbers.
//   nms:    k_nms_pairs              grid (block of 64 columns, block of 64 rows), one wave: lane = row i, the 64 column
//                                    boxes sit in LDS; bit j of the row's word = j > i, same class, !(iou <= thresh).
//           k_nms_scan               ONE wave.  Removed-bitset of 64 words in LDS.  Per block of 64 rows: the diagonal word
//                                    of each row is walked serially (64 scalar steps), then the rows that survived OR their
//                                    remaining words into the bitset, lane = word.  Writes the survivors in order.
// Integers only on every reduction: two calls give identical bits.
#include "common.h"

#pragma clang fp contract(off)

namespace inr {
namespace {

constexpr int kDtBlock = 256;                 // four waves
constexpr int kDtWaves = kDtBlock / 64;
constexpr int kPasteGroup = 8;                // words a wave gathers before it stores
constexpr int kPasteRun = 256;                // words per workgroup (16384 voxels)
constexpr int kPasteMaxMasks = 1024, kPasteMaxM = 1024;
constexpr int kNmsMax = 4096;
constexpr int kVwGroup = 8;                   // words of every plane a wave converts at a time

// Voxel index -> sample position in texel units: the reference's (i - x1) / (x2 - x1) * 2 - 1 followed by grid_sample's
// ((g + 1) / 2) * (M - 1).  Every operation rounds to fp32 and is non-decreasing in i (scale > 0, mtop >= 0).
__device__ __forceinline__ float paste_coord(int i, float lo, float side, float mtop) {
  const float g = ((float)i - lo) / side * 2.0f - 1.0f;
  return ((g + 1.0f) / 2.0f) * mtop;
}

__device__ __forceinline__ bool texel_ok(float p, float m) { return p >= 0.0f && p < m; }      // NaN: false

struct PasteBox {
  float x1, y1, z1, sx, sy, sz;
  bool live;                                  // finite, every side > 0
};

__device__ __forceinline__ PasteBox load_box(const float* __restrict__ b) {
  PasteBox r;
  const float x2 = b[3], y2 = b[4], z2 = b[5];
  r.x1 = b[0], r.y1 = b[1], r.z1 = b[2];
  r.sx = x2 - r.x1, r.sy = y2 - r.y1, r.sz = z2 - r.z1;
  const float big = __builtin_huge_valf();
  const bool finite = fabsf(r.x1) < big && fabsf(r.y1) < big && fabsf(r.z1) < big && fabsf(x2) < big && fabsf(y2) < big &&
                      fabsf(z2) < big;
  r.live = finite && r.sx > 0.0f && r.sy > 0.0f && r.sz > 0.0f;
  return r;
}

// One voxel of one mask: the eight taps in torch's order, each `acc = acc + value * weight` as two roundings.
__device__ __forceinline__ float paste_sample(const float* __restrict__ m, int M, float fm, float mtop, const PasteBox& bx,
                                              int i, int j, int k) {
  const float pw = paste_coord(i, bx.x1, bx.sx, mtop), pl = paste_coord(j, bx.y1, bx.sy, mtop),
              ph = paste_coord(k, bx.z1, bx.sz, mtop);
  const float w0 = floorf(pw), l0 = floorf(pl), h0 = floorf(ph);
  const float w1 = w0 + 1.0f, l1 = l0 + 1.0f, h1 = h0 + 1.0f;
  const float fw[2] = {w1 - pw, pw - w0}, fl[2] = {l1 - pl, pl - l0}, fh[2] = {h1 - ph, ph - h0};
  const bool okw[2] = {texel_ok(w0, fm), texel_ok(w1, fm)}, okl[2] = {texel_ok(l0, fm), texel_ok(l1, fm)},
             okh[2] = {texel_ok(h0, fm), texel_ok(h1, fm)};
  // an index is formed only from a coordinate that passed its test: 0 <= value < M <= 1024
  const int iw[2] = {okw[0] ? (int)w0 : 0, okw[1] ? (int)w1 : 0}, il[2] = {okl[0] ? (int)l0 : 0, okl[1] ? (int)l1 : 0},
            ih[2] = {okh[0] ? (int)h0 : 0, okh[1] ? (int)h1 : 0};
  float val[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {               // eight independent loads in flight
    const int a = t >> 2, b = (t >> 1) & 1, c = t & 1;
    val[t] = (okw[a] && okl[b] && okh[c]) ? m[(iw[a] * M + il[b]) * M + ih[c]] : 0.0f;
  }
  float acc = 0.0f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int a = t >> 2, b = (t >> 1) & 1, c = t & 1;
    if (okw[a] && okl[b] && okh[c]) acc = acc + val[t] * ((fh[c] * fl[b]) * fw[a]);
  }
  return acc;
}

// grid: x = run of kPasteRun words, y = mask.  planes [N, nW], area [N] (zeroed by the caller), soft [N, V] or null.
__global__ __launch_bounds__(kDtBlock) void k_paste_masks(const float* __restrict__ probs, const float* __restrict__ boxes,
                                                          int M, int L, int H, int64_t V, int64_t nW, float thresh,
                                                          unsigned long long* __restrict__ planes, int* __restrict__ area,
                                                          float* __restrict__ soft) {
  __shared__ int block_area;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = blockIdx.y;
  const float* m = probs + row * ((int64_t)M * M * M);
  unsigned long long* out = planes + row * nW;
  float* sout = soft != nullptr ? soft + row * V : nullptr;
  const int64_t w0 = (int64_t)blockIdx.x * kPasteRun, w1 = min(nW, w0 + kPasteRun);
  const PasteBox bx = load_box(boxes + row * 6);
  const float fm = (float)M, mtop = (float)(M - 1);
  const int LH = L * H;                       // L * H <= V < 2^31
  // the run's voxels span w indices ia..ib: nothing to sample if the box is dead, or every tap of every voxel misses the
  // texel range along W (p < -1 at ib, or p >= M at ia; the coordinate is monotone in the index).  M = 1 never skips:
  // the one texel covers every position (p = g * 0).
  bool skip = !bx.live;
  if (!skip && M > 1) {
    const int ia = (int)((w0 * 64) / LH), ib = (int)((min(V, w1 * 64) - 1) / LH);
    skip = paste_coord(ib, bx.x1, bx.sx, mtop) < -1.0f || paste_coord(ia, bx.x1, bx.sx, mtop) >= fm;
  }
  if (skip) {                                 // uniform over the workgroup
    for (int64_t w = w0 + threadIdx.x; w < w1; w += kDtBlock) out[w] = 0ull;
    if (sout != nullptr)
      for (int64_t v = w0 * 64 + threadIdx.x; v < min(V, w1 * 64); v += kDtBlock) sout[v] = 0.0f;
    return;
  }
  if (threadIdx.x == 0) block_area = 0;
  __syncthreads();
  int cnt = 0;                                // lanes 0..7: set bits of the words this lane stored
  // every wave takes whole groups: the ballots need all 64 lanes
  for (int64_t g = w0 + wave * kPasteGroup; g < w1; g += kDtWaves * kPasteGroup) {
    unsigned long long mine = 0;
#pragma unroll 2
    for (int q = 0; q < kPasteGroup; ++q) {
      const int64_t v = (g + q) * 64 + lane;
      bool bit = false;
      if (v < V) {                            // past the volume (and past the run's last word): zero bits
        const int vi = (int)v, i = vi / LH, rem = vi - i * LH, j = rem / H, k = rem - j * H;
        const float acc = paste_sample(m, M, fm, mtop, bx, i, j, k);
        bit = acc >= thresh;
        if (sout != nullptr) sout[v] = acc;
      }
      const unsigned long long word = __ballot(bit);
      if (lane == q) mine = word;
    }
    if (lane < kPasteGroup && g + lane < w1) {
      out[g + lane] = mine;
      cnt += __popcll(mine);
    }
  }
  if (cnt != 0) atomicAdd(&block_area, cnt);
  __syncthreads();
  if (threadIdx.x == 0 && block_area != 0) atomicAdd(&area[row], block_area);
}

// grid: x = run of kDtWaves * kVwGroup words.  planes [k, nW]; out int32 [V]: bit i = plane base + i, i < count <= 32.
__global__ __launch_bounds__(kDtBlock) void k_planes_to_voxel_words(const unsigned long long* __restrict__ planes,
                                                                    int64_t V, int64_t nW, int base, int count,
                                                                    unsigned int* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = ((int64_t)blockIdx.x * kDtWaves + wave) * kVwGroup;      // this wave's first word
  if (g >= nW) return;
  // slot s = r * 64 + lane holds plane s / 8, word g + s % 8: a plane's eight words are 64 contiguous bytes
  unsigned int lo[4], hi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int s = r * 64 + lane, p = s / kVwGroup;
    const int64_t w = g + s % kVwGroup;
    const unsigned long long x = (p < count && w < nW) ? planes[(int64_t)(base + p) * nW + w] : 0ull;
    lo[r] = (unsigned int)x, hi[r] = (unsigned int)(x >> 32);
  }
#pragma unroll
  for (int q = 0; q < kVwGroup; ++q) {
    unsigned int word = 0;
#pragma unroll
    for (int p = 0; p < 32; ++p) {
      const int s = p * kVwGroup + q;
      const unsigned int a = __builtin_amdgcn_readlane(lo[s >> 6], s & 63), b = __builtin_amdgcn_readlane(hi[s >> 6], s & 63);
      word |= (((lane < 32 ? a : b) >> (lane & 31)) & 1u) << p;
    }
    const int64_t v = (g + q) * 64 + lane;
    if (v < V) out[v] = word;
  }
}

// torch.maximum / torch.minimum: a NaN operand gives NaN
__device__ __forceinline__ float max_nan(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ float min_nan(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

__device__ __forceinline__ float box_volume(const float* b) { return ((b[3] - b[0]) * (b[4] - b[1])) * (b[5] - b[2]); }

// grid: x = block of 64 columns, y = block of 64 rows; 64 threads.  pairs [n, nw].
__global__ __launch_bounds__(64) void k_nms_pairs(const float* __restrict__ boxes, const int* __restrict__ cls, int n, int nw,
                                                  float thresh, unsigned long long* __restrict__ pairs) {
  __shared__ float cbox[64][6];
  __shared__ int ccls[64];
  const int lane = threadIdx.x;
  const int i = blockIdx.y * 64 + lane, j0 = blockIdx.x * 64;
  if (blockIdx.x < blockIdx.y) {              // every column lies before every row: no bit
    if (i < n) pairs[(int64_t)i * nw + blockIdx.x] = 0ull;
    return;
  }
  const int nj = min(64, n - j0);
  if (lane < nj) {
#pragma unroll
    for (int c = 0; c < 6; ++c) cbox[lane][c] = boxes[(int64_t)(j0 + lane) * 6 + c];
    ccls[lane] = cls[j0 + lane];
  }
  __syncthreads();
  if (i >= n) return;
  float a[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) a[c] = boxes[(int64_t)i * 6 + c];
  const int ca = cls[i];
  const float va = box_volume(a);
  unsigned long long word = 0;
  for (int t = 0; t < nj; ++t) {
    const float* b = cbox[t];
    float ext[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = min_nan(a[3 + c], b[3 + c]) - max_nan(a[c], b[c]);
      ext[c] = d < 0.0f ? 0.0f : d;           // clamp(min=0): NaN stays NaN
    }
    const float overlap = (ext[0] * ext[1]) * ext[2];
    const float iou = overlap / ((va + box_volume(b)) - overlap);
    if (j0 + t > i && ccls[t] == ca && !(iou <= thresh)) word |= 1ull << t;
  }
  pairs[(int64_t)i * nw + blockIdx.x] = word;
}

// one wave.  keep [n]: the rows that survive, ascending; n_keep [1].
__global__ __launch_bounds__(64) void k_nms_scan(const unsigned long long* __restrict__ pairs, int n, int nw,
                                                 int* __restrict__ keep, int* __restrict__ n_keep) {
  __shared__ unsigned long long removed[64];
  const int lane = threadIdx.x;
  removed[lane] = 0ull;
  __syncthreads();
  int kept = 0;
  for (int b = 0; b < nw; ++b) {
    const int r0 = b * 64, rows = min(64, n - r0);
    const unsigned long long diag = lane < rows ? pairs[(int64_t)(r0 + lane) * nw + b] : 0ull;
    const unsigned int dlo = (unsigned int)diag, dhi = (unsigned int)(diag >> 32);
    unsigned long long cur = removed[b];      // the same value in every lane
    if (rows < 64) cur |= ~0ull << rows;      // rows past n: never kept
#pragma unroll
    for (int r = 0; r < 64; ++r) {
      const unsigned int lo = __builtin_amdgcn_readlane(dlo, r), hi = __builtin_amdgcn_readlane(dhi, r);      // returns int
      const unsigned long long d = (unsigned long long)lo | ((unsigned long long)hi << 32);
      if (!((cur >> r) & 1ull)) cur |= d;     // row r survives: it removes its later same-class overlaps
    }
    const unsigned long long alive = ~cur;
    if ((alive >> lane) & 1ull) keep[kept + __popcll(alive & ((1ull << lane) - 1ull))] = r0 + lane;
    kept += __popcll(alive);
    // the surviving rows of this block mark the later blocks: lane = word
    unsigned long long acc = 0ull;
    if (lane > b && lane < nw) {
      for (int r = 0; r < rows; r += 16) {    // sixteen independent loads in flight, the removed rows' words masked out
        unsigned long long x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = r + u < rows ? pairs[(int64_t)(r0 + r + u) * nw + lane] : 0ull;
#pragma unroll
        for (int u = 0; u < 16; ++u) acc |= ((alive >> (r + u)) & 1ull) ? x[u] : 0ull;
      }
    }
    __syncthreads();
    removed[lane] |= acc;
    __syncthreads();
  }
  if (lane == 0) *n_keep = kept;
}

bool grid_ok(int32_t W, int32_t L, int32_t H, const char* who) {
  if (W < 1 || L < 1 || H < 1 || (int64_t)W * L * H > INT32_MAX) {
    set_error("%s: W, L, H must be >= 1 with W * L * H <= 2^31-1 (voxel counts are int32)", who);
    return false;
  }
  return true;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" int inr_paste_masks(const float* probs, const float* boxes, int32_t N, int32_t M, int32_t W, int32_t L, int32_t H,
                               float thresh, uint64_t* planes, int32_t* area, float* soft, inr_stream_t s) {
  if (!grid_ok(W, L, H, __func__)) return INR_EINVAL;
  INR_REQUIRE(N >= 0 && N <= kPasteMaxMasks, "N must be 0..1024");
  INR_REQUIRE(M >= 1 && M <= kPasteMaxM, "M must be 1..1024");
  INR_REQUIRE(thresh >= 0.0f, "thresh must be >= 0 (and not NaN)");
  if (N == 0) return INR_OK;
  INR_REQUIRE(probs != nullptr && boxes != nullptr && planes != nullptr && area != nullptr, "null pointer");
  INR_REQUIRE(((uintptr_t)planes & 7) == 0 && (((uintptr_t)area | (uintptr_t)probs | (uintptr_t)boxes | (uintptr_t)soft) & 3) == 0,
              "misaligned planes (8 bytes) or area, probs, boxes, soft (4 bytes)");
  const int64_t V = (int64_t)W * L * H, nW = (V + 63) / 64;
  hipStream_t st = as_stream(s);
  if (hipMemsetAsync(area, 0, (size_t)N * 4, st) != hipSuccess) return check_launch("inr_paste_masks");
  hipLaunchKernelGGL(k_paste_masks, dim3(blocks_for(nW, kPasteRun), (unsigned)N), dim3(kDtBlock), 0, st, probs, boxes, M, L, H,
                     V, nW, thresh, reinterpret_cast<unsigned long long*>(planes), area, soft);
  return check_launch("inr_paste_masks");
}

extern "C" int inr_planes_to_voxel_words(const uint64_t* planes, int32_t k, int64_t V, int32_t base, int32_t* words,
                                         inr_stream_t s) {
  INR_REQUIRE(V >= 1 && V <= INT32_MAX, "V must be 1..2^31-1 (voxel counts are int32)");
  INR_REQUIRE(k >= 1 && k <= kPasteMaxMasks, "k must be 1..1024");
  INR_REQUIRE(base >= 0 && base < k, "base must be 0..k-1");
  INR_REQUIRE(planes != nullptr && words != nullptr, "null pointer");
  INR_REQUIRE(((uintptr_t)planes & 7) == 0 && ((uintptr_t)words & 3) == 0, "misaligned planes (8 bytes) or words (4 bytes)");
  const int64_t nW = (V + 63) / 64;
  hipLaunchKernelGGL(k_planes_to_voxel_words, dim3(blocks_for(nW, kDtWaves * kVwGroup)), dim3(kDtBlock), 0, as_stream(s),
                     reinterpret_cast<const unsigned long long*>(planes), V, nW, base, std::min(32, k - base),
                     reinterpret_cast<unsigned int*>(words));
  return check_launch("inr_planes_to_voxel_words");
}

extern "C" int inr_nms_3d_pairs(const float* boxes, const int32_t* classes, int32_t n, float iou_thresh, uint64_t* pairs,
                                inr_stream_t s) {
  INR_REQUIRE(n >= 0 && n <= kNmsMax, "n must be 0..4096");
  if (n == 0) return INR_OK;
  INR_REQUIRE(boxes != nullptr && classes != nullptr && pairs != nullptr, "null pointer");
  INR_REQUIRE(((uintptr_t)pairs & 7) == 0 && (((uintptr_t)boxes | (uintptr_t)classes) & 3) == 0,
              "misaligned pairs (8 bytes) or boxes, classes (4 bytes)");
  const int nw = (n + 63) / 64;
  hipLaunchKernelGGL(k_nms_pairs, dim3((unsigned)nw, (unsigned)nw), dim3(64), 0, as_stream(s), boxes, classes, n, nw, iou_thresh,
                     reinterpret_cast<unsigned long long*>(pairs));
  return check_launch("inr_nms_3d_pairs");
}

extern "C" int inr_nms_3d_scan(const uint64_t* pairs, int32_t n, int32_t* keep, int32_t* n_keep, inr_stream_t s) {
  INR_REQUIRE(n >= 0 && n <= kNmsMax, "n must be 0..4096");
  INR_REQUIRE(n_keep != nullptr, "null pointer (n_keep)");
  INR_REQUIRE(((uintptr_t)n_keep & 3) == 0, "misaligned n_keep (4 bytes)");
  hipStream_t st = as_stream(s);
  if (n == 0) {
    if (hipMemsetAsync(n_keep, 0, 4, st) != hipSuccess) return check_launch("inr_nms_3d_scan");
    return INR_OK;
  }
  INR_REQUIRE(pairs != nullptr && keep != nullptr, "null pointer");
  INR_REQUIRE(((uintptr_t)pairs & 7) == 0 && ((uintptr_t)keep & 3) == 0, "misaligned pairs (8 bytes) or keep (4 bytes)");
  hipLaunchKernelGGL(k_nms_scan, dim3(1), dim3(64), 0, st, reinterpret_cast<const unsigned long long*>(pairs), n,
                     (n + 63) / 64, keep, n_keep);
  return check_launch("inr_nms_3d_scan");
}
