// SSIM and the squared error of rendered views in one launch (include/inr.h, "Image quality of rendered views").
//
// k_ssim_tiles: grid (tile column, tile row, image), 256 threads.  A workgroup owns a 64 x 16 rectangle of map pixels and
// loops over the channels.  Per channel: the 74 x 26 input patch of both images goes, minus the tile's pivot, into LDS
// (lane per pixel straight from the channels-last layout; the squared error of the pixels the tile owns is taken on the
// way); the 11-tap horizontal pass writes five planes (x, y, x^2, y^2, xy) of 26 x 64 back to LDS, one row per wave; the
// vertical pass reads a 14-row column per plane into registers and gives each lane its 4 map pixels.  Map values and
// squared errors are added in binary64 per lane, per wave by shuffles, per workgroup through LDS in wave order, into the
// workgroup's own slot of the workspace.  k_ssim_finish adds the slots of one image: no atomics anywhere.
//
// LDS: 2 x 26 x 74 + 5 x 26 x 64 floats + 8 doubles = 48,736 B -> 3 workgroups per CU.  Every LDS access of a wave is to
// consecutive floats of one row: no bank conflicts.
#include "common.h"

namespace inr {

constexpr int kSsimTaps = INR_SSIM_TAPS;
constexpr int kSsimHalo = kSsimTaps - 1;
constexpr int kSsimTW = INR_SSIM_TILE_W, kSsimTH = INR_SSIM_TILE_H;
constexpr int kSsimPW = kSsimTW + kSsimHalo, kSsimPH = kSsimTH + kSsimHalo;
constexpr int kSsimThreads = 256;
constexpr int kSsimRows = kSsimTH / (kSsimThreads / kSsimTW);        // map rows per lane in the vertical pass: 4
static_assert(kSsimTW == 64 && kSsimThreads == 4 * kSsimTW && kSsimRows * 4 == kSsimTH, "one wave per map row group");

struct SsimWindow {
  float g[kSsimTaps];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;      // lane 0 holds the sum
}

__global__ __launch_bounds__(kSsimThreads) void k_ssim_tiles(const float* __restrict__ pred, const float* __restrict__ truth,
                                                              int H, int W, int C, SsimWindow win,
                                                              const float* __restrict__ data_range, float* __restrict__ out_map,
                                                              double* __restrict__ workspace) {
  __shared__ float raw[2][kSsimPH][kSsimPW];
  __shared__ float hp[5][kSsimPH][kSsimTW];
  __shared__ double red[2][kSsimThreads / 64];
  const int tid = threadIdx.x;
  const int Hm = H - kSsimHalo, Wm = W - kSsimHalo;
  const int c0 = blockIdx.x * kSsimTW, r0 = blockIdx.y * kSsimTH, b = blockIdx.z;
  const int tw = min(kSsimTW, Wm - c0), th = min(kSsimTH, Hm - r0);        // map pixels of this tile
  const int pw = tw + kSsimHalo, ph = th + kSsimHalo;                      // its input patch
  // input pixels whose squared error this tile adds, in patch coordinates: the map rectangle shifted by (5, 5), plus the
  // 5-pixel border where the tile touches the image edge
  const int own_c_lo = blockIdx.x == 0 ? 0 : kSsimHalo / 2, own_c_hi = blockIdx.x == gridDim.x - 1 ? pw : tw + kSsimHalo / 2;
  const int own_r_lo = blockIdx.y == 0 ? 0 : kSsimHalo / 2, own_r_hi = blockIdx.y == gridDim.y - 1 ? ph : th + kSsimHalo / 2;
  const float L = data_range[0];
  const float k1 = 0.01f * L, k2 = 0.03f * L;
  const float C1 = k1 * k1, C2 = k2 * k2;
  const size_t img = (size_t)b * H * W * C;
  const int col = tid & (kSsimTW - 1), row_lo = (tid / kSsimTW) * kSsimRows;
  double ssim_sum = 0.0, sse_sum = 0.0;

  for (int ch = 0; ch < C; ++ch) {
    float pivot = truth[img + ((size_t)(r0 + kSsimHalo / 2) * W + (c0 + kSsimHalo / 2)) * C + ch];
    if (!(fabsf(pivot) <= 3.402823466e38f)) pivot = 0.0f;                  // NaN or inf: no pivot, the tile's other windows stay finite

    for (int idx = tid; idx < kSsimPH * kSsimPW; idx += kSsimThreads) {
      const int r = idx / kSsimPW, c = idx - r * kSsimPW;
      float xs = 0.0f, ys = 0.0f;                                          // outside the image: feeds masked map pixels only
      if (r < ph && c < pw) {
        const size_t off = img + ((size_t)(r0 + r) * W + (c0 + c)) * C + ch;
        const float x = pred[off], y = truth[off];
        if (r >= own_r_lo && r < own_r_hi && c >= own_c_lo && c < own_c_hi) {
          const float d = x - y;
          sse_sum += (double)(d * d);
        }
        xs = x - pivot;
        ys = y - pivot;
      }
      raw[0][r][c] = xs;
      raw[1][r][c] = ys;
    }
    __syncthreads();

    for (int idx = tid; idx < kSsimPH * kSsimTW; idx += kSsimThreads) {    // a wave = one patch row
      const int r = idx / kSsimTW, c = idx & (kSsimTW - 1);
      float hx, hy, hxx, hyy, hxy;
      {
        const float x = raw[0][r][c], y = raw[1][r][c];
        const float g = win.g[0];
        hx = g * x, hy = g * y, hxx = g * (x * x), hyy = g * (y * y), hxy = g * (x * y);
      }
#pragma unroll
      for (int k = 1; k < kSsimTaps; ++k) {
        const float x = raw[0][r][c + k], y = raw[1][r][c + k];
        const float g = win.g[k];
        hx = hx + g * x;
        hy = hy + g * y;
        hxx = hxx + g * (x * x);
        hyy = hyy + g * (y * y);
        hxy = hxy + g * (x * y);
      }
      hp[0][r][c] = hx, hp[1][r][c] = hy, hp[2][r][c] = hxx, hp[3][r][c] = hyy, hp[4][r][c] = hxy;
    }
    __syncthreads();

    float m[5][kSsimRows];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      float column[kSsimRows + kSsimHalo];
#pragma unroll
      for (int k = 0; k < kSsimRows + kSsimHalo; ++k) column[k] = hp[q][row_lo + k][col];
#pragma unroll
      for (int i = 0; i < kSsimRows; ++i) {
        float acc = win.g[0] * column[i];
#pragma unroll
        for (int k = 1; k < kSsimTaps; ++k) acc = acc + win.g[k] * column[i + k];
        m[q][i] = acc;
      }
    }
#pragma unroll
    for (int i = 0; i < kSsimRows; ++i) {
      const float sx = m[0][i], sy = m[1][i];
      const float mx = sx + pivot, my = sy + pivot;
      const float vx = m[2][i] - sx * sx, vy = m[3][i] - sy * sy, cov = m[4][i] - sx * sy;
      const float a1 = 2.0f * (mx * my) + C1, a2 = 2.0f * cov + C2;
      const float b1 = (mx * mx + my * my) + C1, b2 = (vx + vy) + C2;
      const float v = (a1 * a2) / (b1 * b2);
      const int row = row_lo + i;
      if (row < th && col < tw) {
        ssim_sum += (double)v;
        if (out_map) out_map[(((size_t)b * Hm + (r0 + row)) * Wm + (c0 + col)) * C + ch] = v;
      }
    }
    // no barrier here: the next channel's writes of `raw` follow this channel's second barrier (its last reads of `raw`
    // precede it), and its writes of `hp` follow the next first barrier, which no thread passes before its reads above
  }

  ssim_sum = wave_sum_f64(ssim_sum);
  sse_sum = wave_sum_f64(sse_sum);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = ssim_sum;
    red[1][tid >> 6] = sse_sum;
  }
  __syncthreads();
  if (tid == 0) {
    double a = red[0][0], e = red[1][0];
#pragma unroll
    for (int w = 1; w < kSsimThreads / 64; ++w) a += red[0][w], e += red[1][w];
    const size_t slot = ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    workspace[2 * slot] = a;
    workspace[2 * slot + 1] = e;
  }
}

// One wave per image: lane l adds slots l, l + 64, ... in that order, then the lanes meet in a shuffle tree - a fixed order.
__global__ __launch_bounds__(64) void k_ssim_finish(const double* __restrict__ workspace, int slots, double map_count,
                                                     float* __restrict__ out_ssim, float* __restrict__ out_sse) {
  const double* w = workspace + (size_t)blockIdx.x * slots * 2;
  double a = 0.0, e = 0.0;
  for (int i = threadIdx.x; i < slots; i += 64) {
    a += w[2 * i];
    e += w[2 * i + 1];
  }
  a = wave_sum_f64(a);
  e = wave_sum_f64(e);
  if (threadIdx.x == 0) {
    out_ssim[blockIdx.x] = (float)(a / map_count);
    if (out_sse) out_sse[blockIdx.x] = (float)e;
  }
}

// Shared by the size query and the launch: 0 and a message in `why` when the shape is not one the kernel takes.
static int64_t ssim_slots(int64_t B, int64_t H, int64_t W, int32_t C, const char** why) {
  *why = nullptr;
  if (B < 1 || B > 65535) *why = "B must be in 1..65535";
  else if (C < 1 || C > 4) *why = "C must be in 1..4";
  else if (H < kSsimTaps) *why = "H must be at least 11";
  else if (W < kSsimTaps) *why = "W must be at least 11";
  else if (H >= (1ll << 31) || W >= (1ll << 31) || B * H >= (1ll << 31) || B * H * W >= (1ll << 31) ||
           B * H * W * C >= (1ll << 31))
    *why = "B*H*W*C must be below 2^31";
  else if ((H - kSsimHalo + kSsimTH - 1) / kSsimTH > 65535) *why = "H gives more than 65535 tile rows";
  if (*why) return 0;
  return ((H - kSsimHalo + kSsimTH - 1) / kSsimTH) * ((W - kSsimHalo + kSsimTW - 1) / kSsimTW);
}

}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_ssim_workspace_bytes(int64_t B, int64_t H, int64_t W, int32_t C) {
  const char* why;
  const int64_t slots = ssim_slots(B, H, W, C, &why);
  if (why) {
    set_error("inr_ssim_workspace_bytes: %s", why);
    return INR_EINVAL;
  }
  return B * slots * 2 * (int64_t)sizeof(double);
}

int inr_ssim_forward(const float* pred, const float* truth, int64_t B, int64_t H, int64_t W, int32_t C, const float* window11,
                     const float* data_range_dev, float* out_ssim, float* out_sse, float* out_map, void* workspace,
                     int64_t workspace_bytes, inr_stream_t s) {
  const char* why;
  const int64_t slots = ssim_slots(B, H, W, C, &why);
  if (why) {
    set_error("inr_ssim_forward: %s", why);
    return INR_EINVAL;
  }
  INR_REQUIRE(pred && truth && window11 && data_range_dev && out_ssim && workspace, "null pointer");
  INR_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace is misaligned: it must be 8-byte aligned");
  INR_REQUIRE(workspace_bytes >= B * slots * 2 * (int64_t)sizeof(double),
              "workspace too small: inr_ssim_workspace_bytes(B, H, W, C) bytes are needed");
  SsimWindow win;
  for (int k = 0; k < kSsimTaps; ++k) {
    INR_REQUIRE(fabsf(window11[k]) <= 3.402823466e38f, "window11 must hold finite values");
    win.g[k] = window11[k];
  }
  const int tiles_x = (int)((W - kSsimHalo + kSsimTW - 1) / kSsimTW), tiles_y = (int)((H - kSsimHalo + kSsimTH - 1) / kSsimTH);
  k_ssim_tiles<<<dim3(tiles_x, tiles_y, (unsigned)B), kSsimThreads, 0, as_stream(s)>>>(
      pred, truth, (int)H, (int)W, C, win, data_range_dev, out_map, reinterpret_cast<double*>(workspace));
  k_ssim_finish<<<(unsigned)B, 64, 0, as_stream(s)>>>(reinterpret_cast<const double*>(workspace), (int)slots,
                                                      (double)((H - kSsimHalo) * (W - kSsimHalo) * C), out_ssim, out_sse);
  return check_launch("ssim_forward");
}

}  // extern "C"
