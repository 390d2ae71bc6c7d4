// Connected components of a label volume and the per-channel keep rule (include/inr.h, "connected components").
// A component is named by its root, the smallest linear index among its voxels, so the result does not depend on the
// order in which the integer atomics below land: two calls give identical bits.
//
// Global atomics execute at the memory side as uncached 64-byte requests, so they are spent on tile faces only:
//   label:  k_cc_tile      one workgroup per 8 x 8 x 64 tile (H the long axis: one wave per row of 64).  A ballot over
//                          "same label as my -h neighbour" gives every lane the start of its run in the row, which is
//                          its first parent; the remaining unions (other rows of the tile) are a union-find on LDS
//                          atomics.  Writes the global index of every voxel's tile-local root and zeroes the size
//                          counter of every tile-local root (a final root is always one of them).
//           k_cc_merge     one thread per voxel of a tile's shell: unites across tile faces (find both roots, atomicMin
//                          the larger root's parent to the smaller, retry).  A pair whose -h neighbours form the same
//                          kind of pair inside the same two tiles is skipped: that pair already joins the two pieces.
//           k_cc_compress  every voxel to its final root; component sizes by integer adds, one per run of equal roots in
//                          a wave.
//   filter: k_cc_init, k_cc_select (per-channel component count, kept voxels, largest component as a 64-bit
//           (size, ~root) key: LDS first, one global atomic per touched channel and workgroup), k_cc_finish, k_cc_apply.
#include "common.h"

namespace inr {
namespace {

constexpr int kCcBlock = 256;
constexpr int kTW = 8, kTL = 8, kTH = 64;          // tile; kTH = one wave
constexpr int kTileVox = kTW * kTL * kTH;
constexpr int kCcChannels = 256;

// the 13 neighbours that precede a voxel in (w, l, h) order; the first three are the face neighbours
__constant__ int8_t kCcOff[13][3] = {{0, 0, -1}, {0, -1, 0},  {-1, 0, 0},  {0, -1, -1}, {0, -1, 1},  {-1, 0, -1}, {-1, 0, 1},
                                     {-1, -1, 0}, {-1, 1, 0}, {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

__device__ __forceinline__ int lds_find(const int* parent, int x) {
  int q;
  while ((q = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = q;
  return x;
}

// parents only ever decrease, so the root of a set is its smallest member
__device__ __forceinline__ void lds_unite(int* parent, int a, int b) {
  while (true) {
    a = lds_find(parent, a);
    b = lds_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;                                  // a was no root any more: its former parent still has to meet b
  }
}

__device__ __forceinline__ int glob_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int glob_find(const int* parent, int x) {
  int q;
  while ((q = glob_load(parent + x)) != x) x = q;
  return x;
}

__device__ __forceinline__ void glob_unite(int* parent, int a, int b) {
  while (true) {
    a = glob_find(parent, a);
    b = glob_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(kCcBlock) void k_cc_tile(const uint8_t* __restrict__ labels, int W, int L, int H, int n_off,
                                                      int tiles_l, int tiles_h, int* __restrict__ roots,
                                                      int* __restrict__ sizes) {
  __shared__ int parent[kTileVox];
  __shared__ uint8_t lab[kTileVox];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bh = blockIdx.x % tiles_h, bt = blockIdx.x / tiles_h;
  const int w0 = (bt / tiles_l) * kTW, l0 = (bt % tiles_l) * kTL, h0 = bh * kTH;

  for (int row = wave; row < kTW * kTL; row += kCcBlock / 64) {
    const int iw = w0 + row / kTL, il = l0 + row % kTL, ih = h0 + lane;
    int c = 255;
    if (iw < W && il < L && ih < H) c = labels[((int64_t)iw * L + il) * H + ih];
    const int prev = __shfl_up(c, 1, 64);
    const bool same = lane > 0 && c != 255 && prev == c;
    const unsigned long long starts = ~__ballot(same);                     // bit i: lane i starts a run
    const unsigned long long upto = starts & ((2ull << lane) - 1ull);      // lanes 0..lane (2 << 63 wraps to 0: all ones)
    const int start = 63 - __clzll((long long)upto);
    lab[row * kTH + lane] = (uint8_t)c;
    parent[row * kTH + lane] = c == 255 ? -1 : row * kTH + start;
  }
  __syncthreads();

  for (int row = wave; row < kTW * kTL; row += kCcBlock / 64) {
    const int v = row * kTH + lane;
    const int c = lab[v];
    if (c == 255) continue;
    const int tw = row / kTL, tl = row % kTL;
    const bool run_v = lane > 0 && lab[v - 1] == c;
    for (int o = 1; o < n_off; ++o) {                                      // offset 0 (the -h neighbour) is the run
      const int nw = tw + kCcOff[o][0], nl = tl + kCcOff[o][1], nh = lane + kCcOff[o][2];
      if ((unsigned)nw >= (unsigned)kTW || (unsigned)nl >= (unsigned)kTL || (unsigned)nh >= (unsigned)kTH) continue;
      const int u = (nw * kTL + nl) * kTH + nh;
      if (lab[u] != c) continue;
      if (run_v && nh > 0 && lab[u - 1] == c) continue;                    // (v - 1, u - 1) is the same kind of pair
      lds_unite(parent, v, u);
    }
  }
  __syncthreads();

  for (int row = wave; row < kTW * kTL; row += kCcBlock / 64) {
    const int iw = w0 + row / kTL, il = l0 + row % kTL, ih = h0 + lane;
    if (iw >= W || il >= L || ih >= H) continue;
    const int v = row * kTH + lane;
    const int64_t g = ((int64_t)iw * L + il) * H + ih;
    if (lab[v] == 255) {
      roots[g] = -1;
      continue;
    }
    const int r = lds_find(parent, v);
    const int rrow = r / kTH;
    roots[g] = (int)((((int64_t)(w0 + rrow / kTL)) * L + (l0 + rrow % kTL)) * H + (h0 + r % kTH));
    if (r == v) sizes[g] = 0;
  }
}

__global__ __launch_bounds__(kCcBlock) void k_cc_merge(const uint8_t* __restrict__ labels, int W, int L, int H, int n_off,
                                                       int64_t N, int* roots) {
  const int64_t v = (int64_t)blockIdx.x * kCcBlock + threadIdx.x;
  if (v >= N) return;
  const int ih = (int)(v % H);
  const int64_t t = v / H;
  const int il = (int)(t % L), iw = (int)(t / L);
  const int tw = iw % kTW, tl = il % kTL, th = ih % kTH;
  if (!(tw == 0 || tl == 0 || th == 0 || (n_off > 3 && (tl == kTL - 1 || th == kTH - 1)))) return;
  const int c = labels[v];
  if (c == 255) return;
  const bool run_v = th > 0 && labels[v - 1] == c;
  for (int o = 0; o < n_off; ++o) {
    const int dw = kCcOff[o][0], dl = kCcOff[o][1], dh = kCcOff[o][2];
    const int nw = iw + dw, nl = il + dl, nh = ih + dh;
    if ((unsigned)nw >= (unsigned)W || (unsigned)nl >= (unsigned)L || (unsigned)nh >= (unsigned)H) continue;
    if (nw / kTW == iw / kTW && nl / kTL == il / kTL && nh / kTH == ih / kTH) continue;      // same tile: done in LDS
    const int64_t u = v + ((int64_t)dw * L + dl) * H + dh;
    if (labels[u] != c) continue;
    if (run_v && nh % kTH > 0 && labels[u - 1] == c) continue;
    glob_unite(roots, (int)v, (int)u);
  }
}

__global__ __launch_bounds__(kCcBlock) void k_cc_compress(int64_t N, int* roots, int* sizes) {
  const int64_t v = (int64_t)blockIdx.x * kCcBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int r = -1;
  if (v < N) {
    r = glob_load(roots + v);
    if (r >= 0) {
      const int f = glob_find(roots, r);
      if (f != r) __hip_atomic_store(roots + v, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      r = f;
    }
  }
  const int prev = __shfl_up(r, 1, 64);
  const bool head = lane == 0 || prev != r;
  const unsigned long long heads = __ballot(head);
  if (head && r >= 0) {
    const unsigned long long later = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    const int end = later ? __ffsll((long long)later) - 1 : 64;
    atomicAdd(&sizes[r], end - lane);
  }
}

__global__ void k_cc_init(int K, int* n_components, int* kept_voxels, unsigned long long* best) {
  const int t = threadIdx.x;
  if (t < K) {
    n_components[t] = 0;
    kept_voxels[t] = 0;
  }
  if (t < kCcChannels) best[t] = 0ull;
}

__global__ __launch_bounds__(kCcBlock) void k_cc_select(const uint8_t* __restrict__ labels, const int* __restrict__ roots,
                                                        const int* __restrict__ sizes, int64_t N, int K, int first,
                                                        int min_voxels, int keep_largest, int* n_components,
                                                        int* kept_voxels, unsigned long long* best) {
  __shared__ int s_n[kCcChannels], s_kept[kCcChannels];
  __shared__ unsigned long long s_best[kCcChannels];
  const int t = threadIdx.x;
  s_n[t] = 0;
  s_kept[t] = 0;
  s_best[t] = 0ull;
  __syncthreads();
  const int64_t v = (int64_t)blockIdx.x * kCcBlock + t;
  if (v < N && roots[v] == (int)v) {
    const int c = labels[v];
    if (c >= first && c < K) {
      atomicAdd(&s_n[c], 1);
      const int s = sizes[v];
      if (s >= min_voxels) {
        if (keep_largest)       // largest size first, then the lowest root
          atomicMax(&s_best[c], ((unsigned long long)(unsigned)s << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)v));
        else
          atomicAdd(&s_kept[c], s);
      }
    }
  }
  __syncthreads();
  if (s_n[t]) atomicAdd(&n_components[t], s_n[t]);
  if (s_kept[t]) atomicAdd(&kept_voxels[t], s_kept[t]);
  if (s_best[t]) atomicMax(&best[t], s_best[t]);
}

__global__ void k_cc_finish(int K, int keep_largest, const unsigned long long* best, int* kept_voxels, int* kept_root) {
  const int t = threadIdx.x;
  if (t >= K) return;
  int root = -1;
  if (keep_largest) {
    const unsigned long long key = best[t];
    if (key) {
      root = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
      kept_voxels[t] = (int)(key >> 32);
    }
  }
  kept_root[t] = root;
}

__global__ __launch_bounds__(kCcBlock) void k_cc_apply(const uint8_t* labels, const int* __restrict__ roots,
                                                       const int* __restrict__ sizes, const float* confidence, int64_t N,
                                                       int K, int first, int min_voxels, int keep_largest,
                                                       const int* __restrict__ kept_root, uint8_t* labels_out,
                                                       float* confidence_out) {
  const int64_t v = (int64_t)blockIdx.x * kCcBlock + threadIdx.x;
  if (v >= N) return;
  const int c = labels[v];
  bool keep = true;
  if (c >= first && c < K) {
    const int r = roots[v];
    keep = keep_largest ? r == kept_root[c] : sizes[r] >= min_voxels;
  }
  labels_out[v] = keep ? (uint8_t)c : (uint8_t)255;
  if (confidence_out != nullptr) confidence_out[v] = keep ? confidence[v] : 0.0f;
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct CcLayout {
  int64_t N, off_best, bytes;
};

// workspace: sizes int32 [N] (defined at roots only) | best uint64 [256]
bool cc_layout(int32_t W, int32_t L, int32_t H, CcLayout& o, const char* who) {
  if (W < 1 || L < 1 || H < 1) {
    set_error("%s: bad size (W, L, H must be >= 1)", who);
    return false;
  }
  const int64_t WL = (int64_t)W * L;
  if (WL > INT32_MAX || WL * H > INT32_MAX) {
    set_error("%s: the volume is too large (W * L * H must be below 2^31: roots are int32 linear indices)", who);
    return false;
  }
  o.N = WL * H;
  o.off_best = (4 * o.N + 7) / 8 * 8;
  o.bytes = (o.off_best + 8 * kCcChannels + 255) / 256 * 256;
  return true;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" int64_t inr_components_workspace_bytes(int32_t W, int32_t L, int32_t H) {
  CcLayout lay;
  if (!cc_layout(W, L, H, lay, __func__)) return INR_EINVAL;
  return lay.bytes;
}

extern "C" int inr_components_label(const uint8_t* labels, int32_t W, int32_t L, int32_t H, int32_t connectivity,
                                    void* workspace, int64_t workspace_bytes, int32_t* roots, inr_stream_t s) {
  CcLayout lay;
  if (!cc_layout(W, L, H, lay, __func__)) return INR_EINVAL;
  INR_REQUIRE(labels != nullptr && workspace != nullptr && roots != nullptr, "null pointer");
  INR_REQUIRE(connectivity == 6 || connectivity == 26, "connectivity must be 6 or 26");
  INR_REQUIRE(((uintptr_t)roots & 3) == 0, "misaligned roots (4 bytes)");
  INR_REQUIRE(((uintptr_t)workspace & 7) == 0, "misaligned workspace (8 bytes)");
  INR_REQUIRE(workspace_bytes >= lay.bytes, "workspace too small (inr_components_workspace_bytes)");
  int* sizes = static_cast<int*>(workspace);
  const int n_off = connectivity == 6 ? 3 : 13;
  const int64_t tiles_w = (W + kTW - 1) / kTW, tiles_l = (L + kTL - 1) / kTL, tiles_h = (H + kTH - 1) / kTH;
  // a launch holds fewer than 2^32 threads; only a volume far thinner than a tile in two axes comes near
  INR_REQUIRE(tiles_w * tiles_l * tiles_h <= (1 << 23), "too many tiles (W/8 * L/8 * H/64, rounded up, must be <= 2^23)");
  hipStream_t st = as_stream(s);
  const unsigned nb = blocks_for(lay.N, kCcBlock);
  hipLaunchKernelGGL(k_cc_tile, dim3((unsigned)(tiles_w * tiles_l * tiles_h)), dim3(kCcBlock), 0, st, labels, W, L, H, n_off,
                     (int)tiles_l, (int)tiles_h, roots, sizes);
  hipLaunchKernelGGL(k_cc_merge, dim3(nb), dim3(kCcBlock), 0, st, labels, W, L, H, n_off, lay.N, roots);
  hipLaunchKernelGGL(k_cc_compress, dim3(nb), dim3(kCcBlock), 0, st, lay.N, roots, sizes);
  return check_launch("inr_components_label");
}

extern "C" int inr_components_filter(const uint8_t* labels, const int32_t* roots, const float* confidence, int32_t W,
                                     int32_t L, int32_t H, int32_t K, int32_t first_channel, int32_t min_voxels,
                                     int32_t keep_largest, void* workspace, int64_t workspace_bytes, uint8_t* labels_out,
                                     float* confidence_out, int32_t* n_components, int32_t* kept_voxels, int32_t* kept_root,
                                     inr_stream_t s) {
  CcLayout lay;
  if (!cc_layout(W, L, H, lay, __func__)) return INR_EINVAL;
  INR_REQUIRE(labels != nullptr && roots != nullptr && workspace != nullptr && labels_out != nullptr &&
                  n_components != nullptr && kept_voxels != nullptr && kept_root != nullptr,
              "null pointer");
  INR_REQUIRE(K >= 1 && K <= 255, "K must be 1..255 (255 is the empty label)");
  INR_REQUIRE(first_channel >= 0 && first_channel <= K, "first_channel must be 0..K");
  INR_REQUIRE(min_voxels >= 1, "min_voxels must be >= 1");
  INR_REQUIRE(keep_largest == 0 || keep_largest == 1, "keep_largest must be 0 or 1");
  INR_REQUIRE(confidence_out == nullptr || confidence != nullptr, "confidence_out needs confidence");
  INR_REQUIRE((((uintptr_t)roots | (uintptr_t)confidence | (uintptr_t)confidence_out | (uintptr_t)n_components |
                (uintptr_t)kept_voxels | (uintptr_t)kept_root) & 3) == 0,
              "misaligned roots, confidence or per-channel output (4 bytes)");
  INR_REQUIRE(((uintptr_t)workspace & 7) == 0, "misaligned workspace (8 bytes)");
  INR_REQUIRE(workspace_bytes >= lay.bytes, "workspace too small (inr_components_workspace_bytes)");
  char* ws = static_cast<char*>(workspace);
  const int* sizes = reinterpret_cast<const int*>(ws);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(ws + lay.off_best);
  hipStream_t st = as_stream(s);
  const unsigned nb = blocks_for(lay.N, kCcBlock);
  hipLaunchKernelGGL(k_cc_init, dim3(1), dim3(kCcChannels), 0, st, K, n_components, kept_voxels, best);
  hipLaunchKernelGGL(k_cc_select, dim3(nb), dim3(kCcBlock), 0, st, labels, roots, sizes, lay.N, K, first_channel, min_voxels,
                     keep_largest, n_components, kept_voxels, best);
  hipLaunchKernelGGL(k_cc_finish, dim3(1), dim3(kCcChannels), 0, st, K, keep_largest, best, kept_voxels, kept_root);
  hipLaunchKernelGGL(k_cc_apply, dim3(nb), dim3(kCcBlock), 0, st, labels, roots, sizes, confidence, lay.N, K, first_channel,
                     min_voxels, keep_largest, kept_root, labels_out, confidence_out);
  return check_launch("inr_components_filter");
}
