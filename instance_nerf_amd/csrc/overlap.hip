// Pairwise overlap counts of 3-D masks (include/inr.h, "3-D mask overlap").  Every mask is a BIT PLANE: a row of 64-bit
// words over the flattened volume, bit v % 64 of word v / 64 = the mask holds voxel v.  Then
//   inter[a][b] = sum_w popcount(A[a][w] & B[b][w]),   area[a] = sum_w popcount(A[a][w]),
// whose cost does not depend on how many masks overlap at a voxel.  Integer counting with integer atomics only: two
// calls give identical bits.
//
//   pack:   k_pack_mask_planes    grid (run of words, mask).  A wave reads 64 consecutive voxels of one mask, one byte per
//                                 lane; one ballot is one word.  Eight words are gathered before lanes 0..7 store them
//                                 (64 contiguous bytes).
//           k_pack_label_planes   grid (run of words).  A wave reads 64 consecutive labels; plane c is the ballot of
//                                 label == c, kept by lane (c - first) % 64 and stored after every 64 channels.
//           Both count the set bits as they go: per lane, then LDS integer adds per workgroup, then one global integer
//           add per (plane, workgroup).
//   count:  k_overlap_count       grid (run of words, tile of 8 A rows x 8 B rows).  A lane strides over the run's words
//                                 with the tile's 64 accumulators in registers: 16 loads for 64 AND + popcount.  The 64
//                                 lanes x 64 sums of a wave are folded by a halving exchange (63 shuffles; lane l ends
//                                 with sum l), the four waves meet in LDS, and wave 0 issues one global integer add per
//                                 (pair, workgroup).
#include "common.h"

namespace inr {
namespace {

constexpr int kOvBlock = 256;                 // four waves
constexpr int kOvWaves = kOvBlock / 64;
constexpr int kOvMaxMasks = 1024, kOvMaxChannels = 256;
constexpr int kPackGroup = 8;                 // words a wave gathers before it stores
constexpr int kPackRun = 256;                 // words per workgroup of the pack kernels (16384 voxels)
constexpr int kTile = 8;                      // rows of A and of B per workgroup of the count kernel
constexpr int kMinRun = 1024;                 // fewest words per workgroup the count kernel is launched with by default

// grid: x = run of kPackRun words, y = mask.  planes [k, nW], area [k] (zeroed by the caller).
__global__ __launch_bounds__(kOvBlock) void k_pack_mask_planes(const uint8_t* __restrict__ masks, int64_t V, int64_t nW,
                                                               unsigned long long* __restrict__ planes,
                                                               int* __restrict__ area) {
  __shared__ int block_area;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = blockIdx.y;
  const uint8_t* m = masks + row * V;
  unsigned long long* out = planes + row * nW;
  const int64_t w0 = (int64_t)blockIdx.x * kPackRun, w1 = min(nW, w0 + kPackRun);
  if (threadIdx.x == 0) block_area = 0;
  __syncthreads();
  int cnt = 0;                                 // lanes 0..7: set bits of the words this lane stored
  // every wave takes whole groups: the ballots need all 64 lanes
  for (int64_t g = w0 + wave * kPackGroup; g < w1; g += kOvWaves * kPackGroup) {
    uint8_t b[kPackGroup];
#pragma unroll
    for (int j = 0; j < kPackGroup; ++j) {     // eight independent loads in flight
      const int64_t v = (g + j) * 64 + lane;
      b[j] = v < V ? m[v] : (uint8_t)0;        // past the volume (and past the run's last word): zero bits
    }
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < kPackGroup; ++j) {
      const unsigned long long word = __ballot(b[j] != 0);
      if (lane == j) mine = word;
    }
    if (lane < kPackGroup && g + lane < w1) {
      out[g + lane] = mine;
      cnt += __popcll(mine);
    }
  }
  if (cnt != 0) atomicAdd(&block_area, cnt);
  __syncthreads();
  if (threadIdx.x == 0 && block_area != 0) atomicAdd(&area[row], block_area);
}

// grid: x = run of kPackRun words.  planes [K - first, nW], area [K - first] (zeroed by the caller).
__global__ __launch_bounds__(kOvBlock) void k_pack_label_planes(const uint8_t* __restrict__ labels, int64_t V, int64_t nW,
                                                                int K, int first, unsigned long long* __restrict__ planes,
                                                                int* __restrict__ area) {
  __shared__ int block_area[kOvMaxChannels];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = K - first;
  const int64_t w0 = (int64_t)blockIdx.x * kPackRun, w1 = min(nW, w0 + kPackRun);
  for (int i = threadIdx.x; i < k; i += kOvBlock) block_area[i] = 0;
  __syncthreads();
  int cnt[kOvMaxChannels / 64] = {0, 0, 0, 0};        // lane l: set bits of planes l, 64 + l, 128 + l, 192 + l
  for (int64_t w = w0 + wave; w < w1; w += kOvWaves) {
    const int64_t v = w * 64 + lane;
    const bool live = v < V;                          // past the volume: in no plane (255 is a channel when K = 256)
    const int lab = live ? (int)labels[v] : 255;
#pragma unroll
    for (int grp = 0; grp < kOvMaxChannels / 64; ++grp) {
      const int c0 = grp * 64;
      if (c0 >= k) break;
      const int n = min(64, k - c0);
      unsigned long long mine = 0;
      for (int i = 0; i < n; ++i) {
        const unsigned long long word = __ballot(live && lab == first + c0 + i);
        if (lane == i) mine = word;
      }
      if (lane < n) {
        planes[(int64_t)(c0 + lane) * nW + w] = mine;
        cnt[grp] += __popcll(mine);
      }
    }
  }
#pragma unroll
  for (int grp = 0; grp < kOvMaxChannels / 64; ++grp) {
    const int c = grp * 64 + lane;
    if (c < k && cnt[grp] != 0) atomicAdd(&block_area[c], cnt[grp]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += kOvBlock)
    if (block_area[i] != 0) atomicAdd(&area[i], block_area[i]);
}

// grid: x = run of `run` words, y = tile (ta, tb) = (y / tilesB, y % tilesB).  inter [kA, kB] (zeroed by the caller).
__global__ __launch_bounds__(kOvBlock) void k_overlap_count(const unsigned long long* __restrict__ A, int kA,
                                                            const unsigned long long* __restrict__ B, int kB, int64_t nW,
                                                            int64_t run, int tilesB, int* __restrict__ inter) {
  __shared__ int part[kOvWaves][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ta = blockIdx.y / tilesB, tb = blockIdx.y % tilesB;
  const int nA = min(kTile, kA - ta * kTile), nB = min(kTile, kB - tb * kTile);      // rows of an edge tile that exist
  const unsigned long long* pa = A + (int64_t)ta * kTile * nW;
  const unsigned long long* pb = B + (int64_t)tb * kTile * nW;
  const int64_t w0 = (int64_t)blockIdx.x * run, w1 = min(nW, w0 + run);
  int acc[kTile * kTile];
#pragma unroll
  for (int i = 0; i < kTile * kTile; ++i) acc[i] = 0;
  for (int64_t w = w0 + threadIdx.x; w < w1; w += kOvBlock) {
    unsigned long long a[kTile], b[kTile];
#pragma unroll
    for (int i = 0; i < kTile; ++i) a[i] = i < nA ? pa[(int64_t)i * nW + w] : 0ull;  // rows past kA / kB are not read
#pragma unroll
    for (int j = 0; j < kTile; ++j) b[j] = j < nB ? pb[(int64_t)j * nW + w] : 0ull;
#pragma unroll
    for (int i = 0; i < kTile; ++i)
#pragma unroll
      for (int j = 0; j < kTile; ++j) acc[i * kTile + j] += __popcll(a[i] & b[j]);
  }
  // 64 lanes x 64 sums -> lane l holds the wave's sum l: at each step a lane keeps the half of its values that its lane
  // bit selects and receives the partner's values for that half
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
    const bool upper = (lane & h) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const int keep = upper ? acc[i + h] : acc[i];
      const int send = upper ? acc[i] : acc[i + h];
      acc[i] = keep + __shfl_xor(send, h, 64);
    }
  }
  part[wave][lane] = acc[0];
  __syncthreads();
  if (wave == 0) {
    int sum = 0;
#pragma unroll
    for (int wv = 0; wv < kOvWaves; ++wv) sum += part[wv][lane];
    const int i = lane / kTile, j = lane % kTile;
    if (i < nA && j < nB && sum != 0) atomicAdd(&inter[(int64_t)(ta * kTile + i) * kB + tb * kTile + j], sum);
  }
}

bool volume_ok(int64_t V, const char* who) {
  if (V < 1 || V > INT32_MAX) {
    set_error("%s: V must be 1..2^31-1 (voxel counts are int32)", who);
    return false;
  }
  return true;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" int inr_pack_mask_planes(const uint8_t* masks, int32_t k, int64_t V, uint64_t* planes, int32_t* area,
                                    inr_stream_t s) {
  if (!volume_ok(V, __func__)) return INR_EINVAL;
  INR_REQUIRE(k >= 0 && k <= kOvMaxMasks, "k must be 0..1024");
  if (k == 0) return INR_OK;
  INR_REQUIRE(masks != nullptr && planes != nullptr && area != nullptr, "null pointer");
  INR_REQUIRE(((uintptr_t)planes & 7) == 0 && ((uintptr_t)area & 3) == 0, "misaligned planes (8 bytes) or area (4 bytes)");
  const int64_t nW = (V + 63) / 64;
  hipStream_t st = as_stream(s);
  if (hipMemsetAsync(area, 0, (size_t)k * 4, st) != hipSuccess) return check_launch("inr_pack_mask_planes");
  hipLaunchKernelGGL(k_pack_mask_planes, dim3(blocks_for(nW, kPackRun), (unsigned)k), dim3(kOvBlock), 0, st, masks, V, nW,
                     reinterpret_cast<unsigned long long*>(planes), area);
  return check_launch("inr_pack_mask_planes");
}

extern "C" int inr_pack_label_planes(const uint8_t* labels, int64_t V, int32_t K, int32_t first_channel, uint64_t* planes,
                                     int32_t* area, inr_stream_t s) {
  if (!volume_ok(V, __func__)) return INR_EINVAL;
  INR_REQUIRE(K >= 1 && K <= kOvMaxChannels, "K must be 1..256");
  INR_REQUIRE(first_channel >= 0 && first_channel <= K, "first_channel must be 0..K");
  INR_REQUIRE(labels != nullptr, "null pointer (labels)");
  const int k = K - first_channel;
  if (k == 0) return INR_OK;
  INR_REQUIRE(planes != nullptr && area != nullptr, "null pointer");
  INR_REQUIRE(((uintptr_t)planes & 7) == 0 && ((uintptr_t)area & 3) == 0, "misaligned planes (8 bytes) or area (4 bytes)");
  const int64_t nW = (V + 63) / 64;
  hipStream_t st = as_stream(s);
  if (hipMemsetAsync(area, 0, (size_t)k * 4, st) != hipSuccess) return check_launch("inr_pack_label_planes");
  hipLaunchKernelGGL(k_pack_label_planes, dim3(blocks_for(nW, kPackRun)), dim3(kOvBlock), 0, st, labels, V, nW, K,
                     first_channel, reinterpret_cast<unsigned long long*>(planes), area);
  return check_launch("inr_pack_label_planes");
}

extern "C" int inr_mask_overlap(const uint64_t* planes_a, int32_t kA, const uint64_t* planes_b, int32_t kB, int64_t V,
                                int32_t run_words, int32_t* inter, inr_stream_t s) {
  if (!volume_ok(V, __func__)) return INR_EINVAL;
  INR_REQUIRE(kA >= 0 && kA <= kOvMaxMasks, "kA must be 0..1024");
  INR_REQUIRE(kB >= 0 && kB <= kOvMaxMasks, "kB must be 0..1024");
  INR_REQUIRE(run_words >= 0 && run_words % kOvBlock == 0, "run_words must be 0 (the library's choice) or a multiple of 256");
  if (kA == 0 || kB == 0) return INR_OK;
  INR_REQUIRE(planes_a != nullptr && planes_b != nullptr && inter != nullptr, "null pointer");
  INR_REQUIRE((((uintptr_t)planes_a | (uintptr_t)planes_b) & 7) == 0 && ((uintptr_t)inter & 3) == 0,
              "misaligned planes (8 bytes) or inter (4 bytes)");
  const int64_t nW = (V + 63) / 64;
  const int tilesA = (kA + kTile - 1) / kTile, tilesB = (kB + kTile - 1) / kTile;
  int64_t run = run_words;
  if (run == 0) {
    // enough workgroups to fill the machine, but a run no shorter than kMinRun words: every workgroup pays the fold of
    // its 64 sums and 64 global adds once
    const int64_t tiles = (int64_t)tilesA * tilesB;
    const int64_t want = ((int64_t)cu_count() * 8 + tiles - 1) / tiles;
    const int64_t runs = std::max<int64_t>(1, std::min(want, (nW + kMinRun - 1) / kMinRun));
    run = ((nW + runs - 1) / runs + kOvBlock - 1) / kOvBlock * kOvBlock;
  }
  hipStream_t st = as_stream(s);
  if (hipMemsetAsync(inter, 0, (size_t)kA * (size_t)kB * 4, st) != hipSuccess) return check_launch("inr_mask_overlap");
  hipLaunchKernelGGL(k_overlap_count, dim3((unsigned)((nW + run - 1) / run), (unsigned)(tilesA * tilesB)), dim3(kOvBlock), 0, st, reinterpret_cast<const unsigned long long*>(planes_a), kA,
                     reinterpret_cast<const unsigned long long*>(planes_b), kB, nW, run, tilesB, inter);
  return check_launch("inr_mask_overlap");
}
