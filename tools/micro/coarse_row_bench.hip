// Microbenchmark: what an x-neighbour ROW PAIR of a coarse (dense) level costs a CU, three ways.  One 512-thread
// workgroup per CU (the field kernel's shape), rows the size of level 1 of the bench table (24^3 = 13 824 rows of 8
// bytes), 16 row pairs in flight per lane and round.  The lanes of a wave are grouped: `share` consecutive lanes pick
// their rows inside one 128-byte line (16 or 4 lanes per line - a coarse instruction of the pair kernel is near the
// first), the line itself pseudo-random inside a window of the level (16 KB: served by the L1; 64 KB: by the L2).
//   mode 0 (a):   two 8-byte buffer gathers per pair (rows r and r + 1), all 64 lanes
//   mode 1 (b):   one 16-byte buffer gather per pair at 8-byte alignment (row r), all 64 lanes
//   mode 2 (a32): mode 0 with only the lanes 0..15 and 32..47 active (the s = 0 lanes of the pair kernel)
//   mode 3 (c):   the pair from a 39 360-byte LDS image (level 0: 4920 rows) as the compiler emits it, one ds_read2_b64;
//                 addresses of a patch: the lanes of a wave sit on one or two neighbouring cells
//   mode 4 (c):   the same as two separate ds_read_b64
// Every figure is per ROW PAIR and per active lane.  Each mode is timed five times: min / median / max.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <algorithm>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
__device__ __forceinline__ uint32_t hash32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }

typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));
typedef unsigned int u32x4 __attribute__((__vector_size__(4 * sizeof(unsigned int))));
constexpr int kPairs = 16;             // row pairs in flight per lane
constexpr uint32_t kRows = 13824;      // level 1
constexpr uint32_t kLdsRows = 4920;    // level 0

template <int MODE>
__global__ void __launch_bounds__(512) k_rows(const float2* __restrict__ table, uint32_t share_shift, uint32_t window_lines,
                                             int rounds, float* out) {
  extern __shared__ __attribute__((aligned(16))) float2 img[];
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = tid >> 6;
  if (MODE >= 3) {
    for (uint32_t i = threadIdx.x; i < kLdsRows; i += 512) img[i] = table[i];
    __syncthreads();
  }
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)table, 0, (int)(kRows * 8u), 0x00020000);
  const uint32_t n_lines = kRows / 16;
  const uint32_t window0 = window_lines >= n_lines ? 0u : hash32(blockIdx.x) % (n_lines - window_lines);
  const uint32_t window = window_lines >= n_lines ? n_lines : window_lines;
  const bool active = MODE != 2 || !(lane & 16);
  float acc = 0.f;
  for (int r = 0; r < rounds; ++r) {
    // Addresses must cost next to nothing, or the VALU sets the floor (a first version hashed twice per pair and
    // measured 28-43 clk for every mode): two hashes per ROUND, three or four cheap operations per pair.
    const uint32_t salt = (uint32_t)r * 0x9E3779B9u;
    const uint32_t hg = hash32(((MODE >= 3 ? wave : tid >> share_shift)) ^ salt), hl = hash32(tid ^ ~salt);
    uint32_t off[kPairs];
#pragma unroll
    for (int k = 0; k < kPairs; ++k) {
      uint32_t row;
      if (MODE >= 3) {
        const uint32_t cell = (hg + (uint32_t)k * 977u) & 4095u;               // the patch's cell ...
        row = cell + ((hl >> k) & 1u) + (k & 2 ? 17u : 0u) + (k & 4 ? 289u : 0u);   // ... its neighbour, its yz corners
      } else {
        const uint32_t line = window0 + ((hg + (uint32_t)k * 0x9E37u) & (window - 1u));      // window: a power of two
        row = std::min(line * 16u + ((hl >> k) & 15u), kRows - 2u);            // 8-byte aligned: 1 in 16 straddles two lines
      }
      off[k] = row * 8u;
    }
    if (MODE == 1) {
      u32x4 v[kPairs];
#pragma unroll
      for (int k = 0; k < kPairs; ++k) v[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off[k], 0, 0);
#pragma unroll
      for (int k = 0; k < kPairs; ++k) acc += __uint_as_float(v[k][0] ^ v[k][1] ^ v[k][2] ^ v[k][3]);
    } else if (MODE >= 3) {
      float2 v[kPairs][2];
#pragma unroll
      for (int k = 0; k < kPairs; ++k) {
        const float2* p = reinterpret_cast<const float2*>(reinterpret_cast<const char*>(img) + off[k]);
        v[k][0] = p[0];
        if (MODE == 4) {
          uint32_t next = off[k] + 8u;
          asm volatile("" : "+v"(next));    // opaque: two ds_read_b64 instead of one ds_read2_b64
          v[k][1] = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(img) + next);
        } else {
          v[k][1] = p[1];
        }
      }
#pragma unroll
      for (int k = 0; k < kPairs; ++k) acc += v[k][0].x + v[k][0].y + v[k][1].x + v[k][1].y;
    } else if (active) {
      u32x2 v[kPairs][2];
#pragma unroll
      for (int k = 0; k < kPairs; ++k) {
        uint32_t next = off[k] + 8u;
        asm volatile("" : "+v"(next));      // opaque: or the compiler merges the two into the 16-byte load of mode 1
        v[k][0] = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)off[k], 0, 0);
        v[k][1] = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)next, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < kPairs; ++k) acc += __uint_as_float(v[k][0][0] ^ v[k][0][1] ^ v[k][1][0] ^ v[k][1][1]);
    }
  }
  if (acc == 12345.678f) out[tid] = acc;
}

template <int MODE>
static int run(const float2* table, float* out, uint32_t share_shift, uint32_t window_lines, const char* what) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int rounds = 400, blocks = 256;
  const size_t lds = MODE >= 3 ? kLdsRows * 8 : 0;
  float ms[5];
  k_rows<MODE><<<blocks, 512, lds>>>(table, share_shift, window_lines, 4, out);
  for (int i = 0; i < 5; ++i) {
    CK(hipEventRecord(e0));
    k_rows<MODE><<<blocks, 512, lds>>>(table, share_shift, window_lines, rounds, out);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms[i], e0, e1));
  }
  std::sort(ms, ms + 5);
  const double lanes = MODE == 2 ? 256.0 : 512.0;
  const double pairs = (double)blocks * lanes * rounds * kPairs;
  // clocks (2.4 GHz) a CU spends per wave instruction's worth of row pairs (64 lanes; 32 in mode 2)
  const double clk = ms[2] * 1e-3 * 2.4e9 / ((double)rounds * kPairs * 8);
  printf("mode %d  share %2u  window %4u lines  ms %7.3f %7.3f %7.3f  %6.2f row pairs/clk/CU  %6.1f clk per wave and pair   %s\n", MODE,
         1u << share_shift, window_lines, ms[0], ms[2], ms[4], pairs / ms[2] / 1e6 / 256 / 2.4, clk, what);
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
  return 0;
}

int main() {
  float2* table; float* out;
  CK(hipMalloc(&table, (size_t)kRows * 8)); CK(hipMemset(table, 0, (size_t)kRows * 8));
  CK(hipMalloc(&out, 256 * 512 * 4));
  CK(hipFuncSetAttribute((const void*)k_rows<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsRows * 8)));
  CK(hipFuncSetAttribute((const void*)k_rows<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsRows * 8)));
  for (uint32_t window : {128u, 512u}) {          // 16 KB (L1) | 64 KB (twice the L1: L2)
    for (uint32_t shift : {4u, 2u}) {             // 16 | 4 lanes share a line
      if (run<0>(table, out, shift, window, "(a) two 8-byte gathers")) return 1;
      if (run<1>(table, out, shift, window, "(b) one 16-byte gather")) return 1;
      if (run<2>(table, out, shift, window, "(a) with 32 lanes active")) return 1;
    }
  }
  if (run<3>(table, out, 0, 0, "(c) the pair in one ds_read2_b64, patch addresses")) return 1;
  if (run<4>(table, out, 0, 0, "(c) two ds_read_b64, patch addresses")) return 1;
  CK(hipDeviceSynchronize());
  return 0;
}
