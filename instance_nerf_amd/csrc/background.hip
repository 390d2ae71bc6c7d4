// Background sphere model (upstream's bg_radius > 0) for gfx950: sphere coordinates of a ray, and the fused background
// field - sphere coordinates -> 4-level 2-D hash grid (8 features) + SH-4 of the direction (16) -> 24 -> 64 (ReLU) -> 3
// -> sigmoid - in ONE launch each way.  Compiled with -ffp-contract=off like every file that includes grid_common.h:
// the cell of a sample is the decision the stand-alone 2-D encoder (encoders.hip) takes.
//
// The work is per RAY: one lane owns one ray.  Both weight matrices (1 728 floats) are wave-uniform and reach the
// vector ALU as scalar operands (s_load of a `const __restrict__` pointer; the indices are compile-time constants in the
// fully unrolled forward and wave-uniform in the backward's partly unrolled loops): no LDS, no per-lane weight traffic.  The MLP is 1 728 fp32 FMAs per lane in a fixed order.
#include "common.h"
#include "grid_common.h"

namespace inr {

constexpr int kBgLevels = 4;            // 2-D levels of the fused form
constexpr int kBgIn = 24;               // 16 SH + 8 grid features (SH first, as upstream concatenates)
constexpr int kBgHidden = 64;
constexpr int kBgWeights = kBgHidden * kBgIn + 3 * kBgHidden;       // 1 728: w0 [64,24] then w1 [3,64]
constexpr int kBgBwdLanes = 128;        // rays per workgroup pass of the backward
constexpr int kBgBwdStride = kBgBwdLanes + 1;      // LDS row stride (floats): rows of different features start on different banks
constexpr int kBgMaxGroups = 512;       // workgroups of the backward (each walks ray tiles with stride gridDim.x)

// Where the ray o + t d leaves the sphere |p| = radius (the larger root), y up, as (2 theta / pi - 1, phi / pi), in the
// operation order of raymarching.sph_from_ray; both coordinates then clamped to [-1, 1] (in fp32 2 theta / pi - 1 can land
// one ulp past 1 at the pole), NaN kept.  A ray that never meets the sphere - negative discriminant, or both roots behind
// the origin - gets NaN coordinates: by the grid's rule that is "no grid features".
__device__ __forceinline__ void sph_coords(float ox, float oy, float oz, float dx, float dy, float dz, float radius,
                                           float& u, float& v) {
  const float kPi = 3.14159265358979323846f;
  const float A = dx * dx + dy * dy + dz * dz;
  const float B = ox * dx + oy * dy + oz * dz;
  const float C = (ox * ox + oy * oy + oz * oz) - radius * radius;
  const float t = (-B + sqrtf(B * B - A * C)) / A;
  const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
  const float theta = atan2f(sqrtf(px * px + pz * pz), py);
  const float phi = atan2f(pz, px);
  u = 2.0f * theta / kPi - 1.0f;
  v = phi / kPi;
  u = u < -1.0f ? -1.0f : (u > 1.0f ? 1.0f : u);          // (comparisons, not fminf / fmaxf: NaN stays NaN)
  v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
  if (!(t >= 0.0f)) u = v = __int_as_float(0x7FC00000);
}

// h[24] of a ray: SH-4 of the direction as given, then the 8 grid features at the sphere coordinates (bound 1).
__device__ __forceinline__ void bg_inputs(float u, float v, float dx, float dy, float dz, const GridDesc& G,
                                          const float2* __restrict__ emb, float* h, float& x0, float& x1, bool& inside) {
  sh4(dx, dy, dz, h);
  x0 = (u + 1.0f) / 2.0f;
  x1 = (v + 1.0f) / 2.0f;
  inside = !oob01_2d(x0, x1);
#pragma unroll
  for (int l = 0; l < kBgLevels; ++l) {
    float2 f = make_float2(0.f, 0.f);
    if (inside) f = encode2_level(G, l, x0, x1, emb);
    h[16 + 2 * l] = f.x;
    h[16 + 2 * l + 1] = f.y;
  }
}

// z_j = sum_i w0[j][i] h[i] (i ascending, fmaf), h1_j = max(z_j, 0), o_c = sum_j w1[c][j] h1_j (j ascending, fmaf).
// kKeep: h1 goes to `keep[j * kBgBwdStride]` (the backward's LDS column of this lane).
template <bool kKeep>
__device__ __forceinline__ void bg_mlp(const float* h, const float* __restrict__ w0, const float* __restrict__ w1, float* o,
                                       float* keep) {
  o[0] = o[1] = o[2] = 0.0f;
  // the forward unrolls all 64 rows (52 VGPRs); the backward, which also keeps h, the gradients and its accumulators,
  // takes them four at a time: fully unrolled it sat at the 255-VGPR ceiling with spills in AGPRs and 124 KB of code
#pragma unroll(kKeep ? 4 : kBgHidden)
  for (int j = 0; j < kBgHidden; ++j) {
    float z = 0.0f;
#pragma unroll
    for (int i = 0; i < kBgIn; ++i) z = fmaf(w0[j * kBgIn + i], h[i], z);
    z = fmaxf(z, 0.0f);
    if (kKeep) keep[j * kBgBwdStride] = z;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = fmaf(w1[c * kBgHidden + j], z, o[c]);
  }
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ void __launch_bounds__(256) k_sph_from_ray(const float* __restrict__ ro, const float* __restrict__ rd, int64_t N,
                                                      float radius, float2* __restrict__ coords) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float u, v;
  sph_coords(ro[n * 3], ro[n * 3 + 1], ro[n * 3 + 2], rd[n * 3], rd[n * 3 + 1], rd[n * 3 + 2], radius, u, v);
  coords[n] = make_float2(u, v);
}

__global__ void __launch_bounds__(256) k_background_fwd(const float* __restrict__ ro, const float* __restrict__ rd, int64_t N,
                                                        float radius, const float2* __restrict__ emb, GridDesc G,
                                                        const float* __restrict__ w0, const float* __restrict__ w1,
                                                        float* __restrict__ bg, float2* __restrict__ coords_out,
                                                        const float* __restrict__ weights_sum, float* __restrict__ image) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float dx = rd[n * 3], dy = rd[n * 3 + 1], dz = rd[n * 3 + 2];
  float u, v;
  sph_coords(ro[n * 3], ro[n * 3 + 1], ro[n * 3 + 2], dx, dy, dz, radius, u, v);
  if (coords_out) coords_out[n] = make_float2(u, v);
  float h[kBgIn], x0, x1, o[3];
  bool inside;
  bg_inputs(u, v, dx, dy, dz, G, emb, h, x0, x1, inside);
  bg_mlp<false>(h, w0, w1, o, nullptr);
  const float r = sigmoidf(o[0]), g = sigmoidf(o[1]), b = sigmoidf(o[2]);
  bg[n * 3] = r; bg[n * 3 + 1] = g; bg[n * 3 + 2] = b;
  if (image) {                                     // image += (1 - weights_sum) * bg, a separate multiply and add
    const float k = 1.0f - weights_sum[n];
    image[n * 3] = image[n * 3] + k * r;
    image[n * 3 + 1] = image[n * 3 + 1] + k * g;
    image[n * 3 + 2] = image[n * 3 + 2] + k * b;
  }
}

// Backward.  128 lanes, one ray each per tile; a workgroup walks tiles b, b + gridDim.x, ...  Per tile:
//   1. every lane recomputes its ray's forward (h1 to its LDS column), forms gz_c = grad_bg_c s_c (1 - s_c),
//      dz_j = (h1_j > 0) sum_c w1[c][j] gz_c (c ascending) and denc_i = sum_j w0[j][16 + i] dz_j (j ascending), leaves
//      h, dz and gz in LDS and scatters denc into the table gradient (fp32 atomics, 16 rows per ray);
//   2. the 128 threads change roles: thread t owns 12 elements of grad_w0 (rows t % 32 and t % 32 + 32, columns
//      6 (t / 32) .. + 5) and one or two of grad_w1, and adds the tile's rays to them in ray order.
// After its last tile the workgroup stores its 1 728 partial sums to partial[blockIdx.x]; k_background_wsum adds the
// workgroups' partials in workgroup order.  Same inputs, same grid -> same bits for both weight gradients.
// Rays beyond N take part in step 2 with dz = gz = 0 (an added +0.0 changes no sum).
__global__ void __launch_bounds__(kBgBwdLanes) k_background_bwd(const float* __restrict__ gbg, const float* __restrict__ ro,
                                                                const float* __restrict__ rd, int64_t N, float radius,
                                                                const float2* __restrict__ emb, GridDesc G,
                                                                const float* __restrict__ w0, const float* __restrict__ w1,
                                                                float* __restrict__ gemb, float* __restrict__ partial) {
  __shared__ float s_h1[kBgHidden * kBgBwdStride];
  __shared__ float s_dz[kBgHidden * kBgBwdStride];
  __shared__ float s_h[kBgIn * kBgBwdStride];
  __shared__ float s_gz[3 * kBgBwdStride];
  const int t = threadIdx.x;
  const int jg = t & 31, ig = t >> 5;              // step 2: rows jg, jg + 32; columns 6 ig .. 6 ig + 5
  const int j1 = t & 63, c1 = t >> 6;              // step 2: grad_w1[c1][j1], and [2][j1] for the threads with c1 == 0
  float a0[2][6], a1[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    a1[r] = 0.0f;
#pragma unroll
    for (int i = 0; i < 6; ++i) a0[r][i] = 0.0f;
  }
  const int64_t tiles = (N + kBgBwdLanes - 1) / kBgBwdLanes;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t n = tile * kBgBwdLanes + t;
    const bool live = n < N;
    const int64_t ns = live ? n : N - 1;
    {
      const float dx = rd[ns * 3], dy = rd[ns * 3 + 1], dz = rd[ns * 3 + 2];
      float u, v;
      sph_coords(ro[ns * 3], ro[ns * 3 + 1], ro[ns * 3 + 2], dx, dy, dz, radius, u, v);
      float h[kBgIn], x0, x1, o[3], gz[3];
      bool inside;
      bg_inputs(u, v, dx, dy, dz, G, emb, h, x0, x1, inside);
      bg_mlp<true>(h, w0, w1, o, s_h1 + t);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float sg = sigmoidf(o[c]);
        gz[c] = live ? gbg[ns * 3 + c] * (sg * (1.0f - sg)) : 0.0f;
        s_gz[c * kBgBwdStride + t] = gz[c];
      }
#pragma unroll
      for (int i = 0; i < kBgIn; ++i) s_h[i * kBgBwdStride + t] = h[i];
      float denc[2 * kBgLevels];
#pragma unroll
      for (int i = 0; i < 2 * kBgLevels; ++i) denc[i] = 0.0f;
#pragma unroll 4
      for (int j = 0; j < kBgHidden; ++j) {
        float d = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) d = fmaf(w1[c * kBgHidden + j], gz[c], d);
        d = s_h1[j * kBgBwdStride + t] > 0.0f ? d : 0.0f;
        s_dz[j * kBgBwdStride + t] = d;
#pragma unroll
        for (int i = 0; i < 2 * kBgLevels; ++i) denc[i] = fmaf(w0[j * kBgIn + 16 + i], d, denc[i]);
      }
      if (live && inside) {
#pragma unroll
        for (int l = 0; l < kBgLevels; ++l) scatter2_level(G, l, x0, x1, denc[2 * l], denc[2 * l + 1], gemb);
      }
    }
    __syncthreads();
    for (int r = 0; r < kBgBwdLanes; ++r) {
      const float da = s_dz[jg * kBgBwdStride + r], db = s_dz[(jg + 32) * kBgBwdStride + r];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const float hv = s_h[(6 * ig + i) * kBgBwdStride + r];
        a0[0][i] = fmaf(da, hv, a0[0][i]);
        a0[1][i] = fmaf(db, hv, a0[1][i]);
      }
      const float h1 = s_h1[j1 * kBgBwdStride + r];
      a1[0] = fmaf(s_gz[c1 * kBgBwdStride + r], h1, a1[0]);
      a1[1] = fmaf(s_gz[2 * kBgBwdStride + r], h1, a1[1]);
    }
    __syncthreads();
  }
  float* __restrict__ p = partial + (size_t)blockIdx.x * kBgWeights;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    p[jg * kBgIn + 6 * ig + i] = a0[0][i];
    p[(jg + 32) * kBgIn + 6 * ig + i] = a0[1][i];
  }
  p[kBgHidden * kBgIn + c1 * kBgHidden + j1] = a1[0];
  if (c1 == 0) p[kBgHidden * kBgIn + 2 * kBgHidden + j1] = a1[1];
}

// grad_w0 / grad_w1 = the workgroups' partial sums added in workgroup order (written, not accumulated).
__global__ void __launch_bounds__(64) k_background_wsum(const float* __restrict__ partial, int groups, float* __restrict__ gw0,
                                                       float* __restrict__ gw1) {
  const int e = blockIdx.x * 64 + threadIdx.x;           // 27 workgroups x 64 = 1 728 elements
  float s = 0.0f;
  for (int g = 0; g < groups; ++g) s += partial[(size_t)g * kBgWeights + e];
  if (e < kBgHidden * kBgIn) gw0[e] = s;
  else gw1[e - kBgHidden * kBgIn] = s;
}

static int bg_groups(int64_t N) {
  return (int)std::min<int64_t>((N + kBgBwdLanes - 1) / kBgBwdLanes, kBgMaxGroups);
}

static int bg_desc(const inr_grid_desc* desc, GridDesc& G) {
  int rc = make_grid_desc(desc, G);
  if (rc) return rc;
  if (G.num_levels != kBgLevels) {
    set_error("background: the fused form takes a %d-level 2-D table, got %d levels", kBgLevels, G.num_levels);
    return INR_EINVAL;
  }
  return INR_OK;
}

}  // namespace inr

using namespace inr;

extern "C" {

int inr_sph_from_ray(const float* rays_o, const float* rays_d, int64_t N, float radius, float* coords, inr_stream_t s) {
  INR_REQUIRE(N >= 0, "negative N");
  INR_REQUIRE(radius > 0.0f, "radius must be positive");
  if (N == 0) return INR_OK;
  INR_REQUIRE(rays_o && rays_d && coords, "null pointer");
  INR_REQUIRE(((uintptr_t)coords & 7) == 0, "coords must be 8-byte aligned");
  k_sph_from_ray<<<blocks_for(N, 256), 256, 0, as_stream(s)>>>(rays_o, rays_d, N, radius, reinterpret_cast<float2*>(coords));
  return check_launch("sph_from_ray");
}

int inr_background_forward(const float* rays_o, const float* rays_d, int64_t N, float radius, const float* embeddings,
                           const inr_grid_desc* desc, const float* w0, const float* w1, float* bg, float* coords_out,
                           const float* weights_sum, float* image, inr_stream_t s) {
  INR_REQUIRE(N >= 0 && desc, "bad argument");
  INR_REQUIRE(radius > 0.0f, "radius must be positive");
  INR_REQUIRE((weights_sum == nullptr) == (image == nullptr), "weights_sum and image go together");
  if (N == 0) return INR_OK;
  INR_REQUIRE(rays_o && rays_d && embeddings && w0 && w1 && bg, "null pointer");
  GridDesc G;
  int rc = bg_desc(desc, G);
  if (rc) return rc;
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && ((uintptr_t)coords_out & 7) == 0, "embeddings/coords_out must be 8-byte aligned");
  k_background_fwd<<<blocks_for(N, 256), 256, 0, as_stream(s)>>>(rays_o, rays_d, N, radius, reinterpret_cast<const float2*>(embeddings),
                                                                G, w0, w1, bg, reinterpret_cast<float2*>(coords_out), weights_sum,
                                                                image);
  return check_launch("background_forward");
}

int64_t inr_background_workspace_bytes(int64_t N) {
  if (N < 0) {
    set_error("inr_background_workspace_bytes: negative N");
    return INR_EINVAL;
  }
  return (int64_t)std::max(bg_groups(N), 1) * kBgWeights * (int64_t)sizeof(float);
}

int inr_background_backward(const float* grad_bg, const float* rays_o, const float* rays_d, int64_t N, float radius,
                            const float* embeddings, const inr_grid_desc* desc, const float* w0, const float* w1,
                            float* grad_embeddings, float* grad_w0, float* grad_w1, float* workspace, inr_stream_t s) {
  INR_REQUIRE(N >= 0 && desc, "bad argument");
  INR_REQUIRE(radius > 0.0f, "radius must be positive");
  if (N == 0) return INR_OK;
  INR_REQUIRE(grad_bg && rays_o && rays_d && embeddings && w0 && w1 && grad_embeddings && grad_w0 && grad_w1 && workspace,
              "null pointer");
  GridDesc G;
  int rc = bg_desc(desc, G);
  if (rc) return rc;
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0, "embeddings must be 8-byte aligned");
  INR_REQUIRE((uint64_t)desc->offsets[desc->num_levels] * 2ull < (1ull << 32), "table too large for 32-bit element offsets");
  const int groups = bg_groups(N);
  k_background_bwd<<<groups, kBgBwdLanes, 0, as_stream(s)>>>(grad_bg, rays_o, rays_d, N, radius,
                                                             reinterpret_cast<const float2*>(embeddings), G, w0, w1,
                                                             grad_embeddings, workspace);
  k_background_wsum<<<kBgWeights / 64, 64, 0, as_stream(s)>>>(workspace, groups, grad_w0, grad_w1);
  return check_launch("background_backward");
}

}  // extern "C"
