// Triangle meshes of a lattice field: marching tetrahedra over the Kuhn split of every lattice cell (include/inr.h,
// "iso-surface meshes").  Field-agnostic: loads, compares, one subtraction pair, one division and one multiply-add pair
// per vertex coordinate (no contraction: the build uses -ffp-contract=off), so tests/mesh_reference.py restates it bit
// for bit.  Every index comes from a scan - no atomics - so two calls give identical bits.
//
// Passes (all one thread per point of the extended lattice, h fastest, 256 per workgroup):
//   count: k_mesh_classify  7-bit crossed-edge mask of the point, triangles of its cell, per-workgroup sums
//          k_mesh_scan      one workgroup: exclusive scans of the two per-workgroup sums, totals -> counts[0..1]
//          k_mesh_offsets   first vertex id of every point
//   emit:  k_mesh_vertices  one vertex per set mask bit
//          k_mesh_faces     re-derives the cell's cases, scans the triangle counts inside the workgroup, looks the three
//                           vertex ids of a triangle up as offset[owner] + popcount(mask[owner] & below(direction))
// Neighbouring threads re-read each field row up to 4 times (2 in l x 2 in w); the rows come from L2 / the vector cache,
// nothing is staged through LDS.
#include "common.h"

namespace inr {
namespace {

constexpr int kMeshBlock = 256;

struct MeshParams {
  const float* field;
  int64_t stride;
  const uint8_t* labels;
  int select;
  float iso, lo, hi;
  int W, L, H, P;     // P = 1 with the virtual outside layer
  int Ew, El, Eh;     // extended sizes: W + 2P, ...
  int64_t Np;
};

// corners of tetrahedron t (cube corner code = 4 dw + 2 dl + dh), from (0,0,0) to (1,1,1) along one axis order
__constant__ uint8_t kTet[6][4] = {{0, 4, 6, 7}, {0, 4, 5, 7}, {0, 2, 6, 7}, {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 1, 3, 7}};
// tetrahedron edge e = 01 02 03 12 13 23 -> its two tetrahedron vertices
__constant__ uint8_t kEdgeI[6] = {0, 0, 0, 1, 1, 2};
__constant__ uint8_t kEdgeJ[6] = {1, 2, 3, 2, 3, 3};
// case (bit i = tetrahedron vertex i inside) -> up to two triangles of three tetrahedron edges, wound for an
// even-permutation tetrahedron so that the normal leaves the inside; 7 = unused
__constant__ uint8_t kCase[16][6] = {
    {7, 7, 7, 7, 7, 7}, {0, 1, 2, 7, 7, 7}, {0, 4, 3, 7, 7, 7}, {1, 2, 4, 1, 4, 3}, {1, 3, 5, 7, 7, 7}, {0, 5, 2, 0, 3, 5},
    {0, 4, 5, 0, 5, 1}, {2, 4, 5, 7, 7, 7}, {2, 5, 4, 7, 7, 7}, {0, 1, 5, 0, 5, 4}, {0, 5, 3, 0, 2, 5}, {1, 5, 3, 7, 7, 7},
    {1, 3, 4, 1, 4, 2}, {0, 3, 4, 7, 7, 7}, {0, 2, 1, 7, 7, 7}, {7, 7, 7, 7, 7, 7}};

__device__ __forceinline__ int case_triangles(int m) {
  const int n = __popc(m);
  return n == 2 ? 2 : (n & 1);
}

// the clamped value of an extended-lattice point: iso - clamp for virtual, masked-out and NaN points
__device__ __forceinline__ float mesh_value(const MeshParams& p, int ew, int el, int eh) {
  const int iw = ew - p.P, il = el - p.P, ih = eh - p.P;
  if ((unsigned)iw >= (unsigned)p.W || (unsigned)il >= (unsigned)p.L || (unsigned)ih >= (unsigned)p.H) return p.lo;
  const int64_t i = ((int64_t)iw * p.L + il) * p.H + ih;
  if (p.select >= 0 && p.labels[i] != p.select) return p.lo;
  const float v = p.field[i * p.stride];
  if (!(v == v)) return p.lo;
  return fminf(fmaxf(v, p.lo), p.hi);
}

struct MeshCell {
  float g[8];
  int ew, el, eh;
  uint32_t in_lattice;   // bit c: corner c exists
  uint32_t inside;       // bit c: corner c exists and is inside
};

__device__ __forceinline__ void load_cell(const MeshParams& p, int64_t idx, MeshCell& c) {
  c.eh = (int)(idx % p.Eh);
  const int64_t r = idx / p.Eh;
  c.el = (int)(r % p.El);
  c.ew = (int)(r / p.El);
  c.in_lattice = 0;
  c.inside = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int w = c.ew + ((k >> 2) & 1), l = c.el + ((k >> 1) & 1), h = c.eh + (k & 1);
    const bool ok = w < p.Ew && l < p.El && h < p.Eh;
    c.g[k] = ok ? mesh_value(p, w, l, h) : p.lo;
    if (ok) c.in_lattice |= 1u << k;
    if (ok && c.g[k] >= p.iso) c.inside |= 1u << k;
  }
}

__device__ __forceinline__ int tet_case(uint32_t inside, int t) {
  return (int)(((inside >> kTet[t][0]) & 1u) | (((inside >> kTet[t][1]) & 1u) << 1) | (((inside >> kTet[t][2]) & 1u) << 2) |
               (((inside >> kTet[t][3]) & 1u) << 3));
}

__device__ __forceinline__ int cell_triangles(const MeshCell& c) {
  if (!((c.in_lattice >> 7) & 1u) || c.inside == 0u || c.inside == 0xffu) return 0;
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) n += case_triangles(tet_case(c.inside, t));
  return n;
}

// exclusive scan of one value per thread of a 256-thread workgroup; `total` on every thread
__device__ __forceinline__ int block_exclusive_scan(int v, int32_t* wsum, int& total) {
  const int incl = wave_inclusive_scan(v);
  if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
  __syncthreads();
  int off = incl - v;
  total = 0;
#pragma unroll
  for (int w = 0; w < kMeshBlock / 64; ++w) {
    if (w < (int)(threadIdx.x >> 6)) off += wsum[w];
    total += wsum[w];
  }
  __syncthreads();
  return off;
}

__global__ void __launch_bounds__(kMeshBlock) k_mesh_classify(MeshParams p, uint8_t* __restrict__ mask,
                                                              int32_t* __restrict__ bsum_v, int32_t* __restrict__ bsum_t) {
  __shared__ int32_t wsum[kMeshBlock / 64];
  const int64_t idx = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  int nv = 0, nt = 0;
  if (idx < p.Np) {
    MeshCell c;
    load_cell(p, idx, c);
    const uint32_t in0 = c.inside & 1u;
    uint32_t m = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k)
      if (((c.in_lattice >> k) & 1u) && ((c.inside >> k) & 1u) != in0) m |= 1u << (k - 1);
    if (p.Ew < 2 || p.El < 2 || p.Eh < 2) m = 0;      // no cells: an edge exists only inside a cell
    mask[idx] = (uint8_t)m;
    nv = __popc(m);
    nt = cell_triangles(c);
  }
  int tv, tt;
  block_exclusive_scan(nv, wsum, tv);
  block_exclusive_scan(nt, wsum, tt);
  if (threadIdx.x == 0) {
    bsum_v[blockIdx.x] = tv;
    bsum_t[blockIdx.x] = tt;
  }
}

// one workgroup: both per-workgroup sum arrays -> exclusive prefixes in place; counts = {V, F}
__global__ void __launch_bounds__(1024) k_mesh_scan(int32_t* __restrict__ bsum_v, int32_t* __restrict__ bsum_t, int n_blocks,
                                                    int32_t* __restrict__ counts) {
  __shared__ int32_t wsum[16];
  __shared__ int32_t carry_s;
  for (int which = 0; which < 2; ++which) {
    int32_t* a = which ? bsum_t : bsum_v;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < n_blocks; base += 1024) {
      const int i = base + threadIdx.x;
      const int v = i < n_blocks ? a[i] : 0;
      const int incl = wave_inclusive_scan(v);
      if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
      __syncthreads();
      int wave_off = 0;
      for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) wave_off += wsum[w];
      const int carry = carry_s;
      if (i < n_blocks) a[i] = carry + wave_off + incl - v;
      __syncthreads();
      if (threadIdx.x == 1023) carry_s = carry + wave_off + incl;
      __syncthreads();
    }
    if (threadIdx.x == 0) counts[which] = carry_s;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kMeshBlock) k_mesh_offsets(int64_t Np, const uint8_t* __restrict__ mask,
                                                             const int32_t* __restrict__ bpre_v, int32_t* __restrict__ voff) {
  __shared__ int32_t wsum[kMeshBlock / 64];
  const int64_t idx = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const int nv = idx < Np ? __popc((uint32_t)mask[idx]) : 0;
  int total;
  const int off = block_exclusive_scan(nv, wsum, total);
  if (idx < Np) voff[idx] = bpre_v[blockIdx.x] + off;
}

struct MeshAxes {
  const float* ax[3];
  float ext[3];
};

// position of extended index e (real index e - P) on one axis; the virtual layer continues the first / last step
__device__ __forceinline__ float axis_pos(const float* __restrict__ ax, int n, int i, float ext) {
  if (i >= 0 && i < n) return ax[i];
  if (i < 0) return ax[0] - (n >= 2 ? ax[1] - ax[0] : ext);
  return ax[n - 1] + (n >= 2 ? ax[n - 1] - ax[n - 2] : ext);
}

__global__ void __launch_bounds__(kMeshBlock) k_mesh_vertices(MeshParams p, MeshAxes A, const float* __restrict__ rgb,
                                                              const uint8_t* __restrict__ mask,
                                                              const int32_t* __restrict__ voff, int32_t V,
                                                              float* __restrict__ vertices, float* __restrict__ colors) {
  const int64_t idx = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (idx >= p.Np) return;
  const uint32_t m = mask[idx];
  if (m == 0) return;
  const int eh = (int)(idx % p.Eh);
  const int64_t r = idx / p.Eh;
  const int el = (int)(r % p.El), ew = (int)(r / p.El);
  const int pe[3] = {ew, el, eh};
  const int n[3] = {p.W, p.L, p.H};
  const float a = mesh_value(p, ew, el, eh);
  float xp[3];
  bool p_real = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    xp[k] = axis_pos(A.ax[k], n[k], pe[k] - p.P, A.ext[k]);
    p_real = p_real && (unsigned)(pe[k] - p.P) < (unsigned)n[k];
  }
  int64_t vid = voff[idx];
  for (int c = 1; c < 8; ++c) {
    if (!((m >> (c - 1)) & 1u)) continue;
    if (vid >= V) return;
    const int qe[3] = {ew + ((c >> 2) & 1), el + ((c >> 1) & 1), eh + (c & 1)};
    const float b = mesh_value(p, qe[0], qe[1], qe[2]);
    const float t = (p.iso - a) / (b - a);
    bool q_real = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float xq = qe[k] == pe[k] ? xp[k] : axis_pos(A.ax[k], n[k], qe[k] - p.P, A.ext[k]);
      vertices[vid * 3 + k] = xp[k] + t * (xq - xp[k]);
      q_real = q_real && (unsigned)(qe[k] - p.P) < (unsigned)n[k];
    }
    if (colors != nullptr) {
      const int64_t ip = (((int64_t)(pe[0] - p.P) * p.L + (pe[1] - p.P)) * p.H + (pe[2] - p.P)) * 4;
      const int64_t iq = (((int64_t)(qe[0] - p.P) * p.L + (qe[1] - p.P)) * p.H + (qe[2] - p.P)) * 4;
#pragma unroll
      for (int k = 0; k < 3; ++k) {      // a crossed edge has at least one real end (virtual points are all outside)
        const float cp = p_real ? rgb[ip + k] : rgb[iq + k];
        const float cq = q_real ? rgb[iq + k] : cp;
        colors[vid * 3 + k] = cp + t * (cq - cp);
      }
    }
    ++vid;
  }
}

__global__ void __launch_bounds__(kMeshBlock) k_mesh_faces(MeshParams p, const uint8_t* __restrict__ mask,
                                                           const int32_t* __restrict__ voff,
                                                           const int32_t* __restrict__ bpre_t, int32_t F,
                                                           int32_t* __restrict__ faces, uint8_t* __restrict__ face_labels) {
  __shared__ int32_t wsum[kMeshBlock / 64];
  const int64_t idx = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  MeshCell c;
  int nt = 0;
  if (idx < p.Np) {
    load_cell(p, idx, c);
    nt = cell_triangles(c);
  }
  int total;
  int64_t f = bpre_t[blockIdx.x] + block_exclusive_scan(nt, wsum, total);
  if (nt == 0) return;
  const int64_t sw = (int64_t)p.El * p.Eh, sl = p.Eh;
  for (int t = 0; t < 6; ++t) {
    const int m = tet_case(c.inside, t);
    const int n = case_triangles(m);
    if (n == 0) continue;
    const bool flip = t == 1 || t == 2 || t == 5;      // odd axis permutations are mirror images
    uint8_t label = 255;
    if (face_labels != nullptr) {
      int best = -1;
      for (int i = 0; i < 4; ++i)
        if (((m >> i) & 1) && (best < 0 || c.g[kTet[t][i]] > c.g[kTet[t][best]])) best = i;
      const int k = kTet[t][best];
      const int iw = c.ew + ((k >> 2) & 1) - p.P, il = c.el + ((k >> 1) & 1) - p.P, ih = c.eh + (k & 1) - p.P;
      label = p.labels[((int64_t)iw * p.L + il) * p.H + ih];       // an inside corner is a real point
    }
    for (int j = 0; j < n; ++j, ++f) {
      if (f >= F) return;
      int32_t id[3];
      for (int v = 0; v < 3; ++v) {
        const int e = kCase[m][j * 3 + v];
        const int ci = kTet[t][kEdgeI[e]], cj = kTet[t][kEdgeJ[e]];
        const int64_t owner = idx + ((ci >> 2) & 1) * sw + ((ci >> 1) & 1) * sl + (ci & 1);
        const uint32_t below = (1u << ((cj ^ ci) - 1)) - 1u;
        id[v] = voff[owner] + __popc((uint32_t)mask[owner] & below);
      }
      faces[f * 3 + 0] = id[0];
      faces[f * 3 + 1] = flip ? id[2] : id[1];
      faces[f * 3 + 2] = flip ? id[1] : id[2];
      if (face_labels != nullptr) face_labels[f] = label;
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct MeshLayout {
  int64_t Np, n_blocks, off_bsum_v, off_bsum_t, off_mask, bytes;
};

// sizes -> layout of the workspace: voff int32 [Np] | bsum_v int32 [n_blocks] | bsum_t int32 [n_blocks] | mask uint8 [Np]
bool mesh_layout(int32_t W, int32_t L, int32_t H, int32_t cap, MeshLayout& o, const char* who) {
  if (W < 1 || L < 1 || H < 1) {
    set_error("%s: bad size (W, L, H must be >= 1)", who);
    return false;
  }
  if (cap != 0 && cap != 1) {
    set_error("%s: cap must be 0 or 1", who);
    return false;
  }
  const int64_t Np = ((int64_t)W + 2 * cap) * ((int64_t)L + 2 * cap) * ((int64_t)H + 2 * cap);
  if (Np > (int64_t)INT32_MAX / 12) {      // 7 vertices per point and 12 triangles per cell are int32 indices
    set_error("%s: the lattice is too large (12 * points must fit an int32)", who);
    return false;
  }
  o.Np = Np;
  o.n_blocks = (Np + kMeshBlock - 1) / kMeshBlock;
  o.off_bsum_v = 4 * Np;
  o.off_bsum_t = o.off_bsum_v + 4 * o.n_blocks;
  o.off_mask = o.off_bsum_t + 4 * o.n_blocks;
  o.bytes = (o.off_mask + Np + 255) / 256 * 256;
  return true;
}

int mesh_params(const char* who, const float* field, int32_t field_stride, float iso, float clamp, const uint8_t* labels,
                int32_t select, int32_t W, int32_t L, int32_t H, int32_t cap, const void* workspace, int64_t workspace_bytes,
                MeshParams& p, MeshLayout& lay) {
  if (!mesh_layout(W, L, H, cap, lay, who)) return INR_EINVAL;
  if (field == nullptr || workspace == nullptr) {
    set_error("%s: null pointer", who);
    return INR_EINVAL;
  }
  if (field_stride < 1) {
    set_error("%s: field_stride must be >= 1", who);
    return INR_EINVAL;
  }
  if (!(clamp > 0.0f) || !(clamp < INFINITY) || !(iso == iso) || !(iso - clamp < iso) || !(iso - clamp > -INFINITY) ||
      !(iso + clamp < INFINITY)) {
    set_error("%s: clamp must be > 0 and finite, and iso - clamp < iso in fp32", who);
    return INR_EINVAL;
  }
  if (select < -1 || select >= 255 || (select >= 0 && labels == nullptr)) {
    set_error("%s: select must be -1 or a channel 0..254 of a given label volume", who);
    return INR_EINVAL;
  }
  if (((uintptr_t)field & 3) || ((uintptr_t)workspace & 3)) {
    set_error("%s: misaligned field or workspace (4 bytes)", who);
    return INR_EINVAL;
  }
  if (workspace_bytes < lay.bytes) {
    set_error("%s: workspace too small (inr_mesh_workspace_bytes)", who);
    return INR_EINVAL;
  }
  p.field = field;
  p.stride = field_stride;
  p.labels = labels;
  p.select = select;
  p.iso = iso;
  p.lo = iso - clamp;
  p.hi = iso + clamp;
  p.W = W; p.L = L; p.H = H; p.P = cap;
  p.Ew = W + 2 * cap; p.El = L + 2 * cap; p.Eh = H + 2 * cap;
  p.Np = lay.Np;
  return INR_OK;
}

}  // namespace
}  // namespace inr

using namespace inr;

extern "C" int64_t inr_mesh_workspace_bytes(int32_t W, int32_t L, int32_t H, int32_t cap) {
  MeshLayout lay;
  if (!mesh_layout(W, L, H, cap, lay, __func__)) return INR_EINVAL;
  return lay.bytes;
}

extern "C" int inr_mesh_count(const float* field, int32_t field_stride, float iso, float clamp, const uint8_t* labels,
                              int32_t select, int32_t W, int32_t L, int32_t H, int32_t cap, void* workspace,
                              int64_t workspace_bytes, int32_t* counts, inr_stream_t s) {
  MeshParams p;
  MeshLayout lay;
  const int rc = mesh_params(__func__, field, field_stride, iso, clamp, labels, select, W, L, H, cap, workspace,
                             workspace_bytes, p, lay);
  if (rc != INR_OK) return rc;
  INR_REQUIRE(counts != nullptr, "null pointer");
  INR_REQUIRE(((uintptr_t)counts & 3) == 0, "misaligned counts (4 bytes)");
  char* ws = static_cast<char*>(workspace);
  int32_t* voff = reinterpret_cast<int32_t*>(ws);
  int32_t* bsum_v = reinterpret_cast<int32_t*>(ws + lay.off_bsum_v);
  int32_t* bsum_t = reinterpret_cast<int32_t*>(ws + lay.off_bsum_t);
  uint8_t* mask = reinterpret_cast<uint8_t*>(ws + lay.off_mask);
  hipStream_t st = as_stream(s);
  const unsigned nb = (unsigned)lay.n_blocks;
  hipLaunchKernelGGL(k_mesh_classify, dim3(nb), dim3(kMeshBlock), 0, st, p, mask, bsum_v, bsum_t);
  hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(1024), 0, st, bsum_v, bsum_t, (int)lay.n_blocks, counts);
  hipLaunchKernelGGL(k_mesh_offsets, dim3(nb), dim3(kMeshBlock), 0, st, lay.Np, mask, bsum_v, voff);
  return check_launch("inr_mesh_count");
}

extern "C" int inr_mesh_emit(const float* field, int32_t field_stride, float iso, float clamp, const uint8_t* labels,
                             int32_t select, const float* rgb, const float* ax_w, const float* ax_l, const float* ax_h,
                             int32_t W, int32_t L, int32_t H, float ext_w, float ext_l, float ext_h, int32_t cap,
                             const void* workspace, int64_t workspace_bytes, int32_t V, int32_t F, float* vertices,
                             int32_t* faces, float* colors, uint8_t* face_labels, inr_stream_t s) {
  MeshParams p;
  MeshLayout lay;
  const int rc = mesh_params(__func__, field, field_stride, iso, clamp, labels, select, W, L, H, cap, workspace,
                             workspace_bytes, p, lay);
  if (rc != INR_OK) return rc;
  INR_REQUIRE(ax_w != nullptr && ax_l != nullptr && ax_h != nullptr, "null pointer");
  INR_REQUIRE(V >= 0 && F >= 0, "bad size (V, F)");
  INR_REQUIRE((int64_t)V <= 7 * lay.Np && (int64_t)F <= 12 * lay.Np, "V or F larger than the lattice can give");
  INR_REQUIRE((V == 0 || vertices != nullptr) && (F == 0 || faces != nullptr), "null pointer");
  INR_REQUIRE((colors == nullptr) == (rgb == nullptr), "colors and rgb go together");
  INR_REQUIRE(face_labels == nullptr || labels != nullptr, "face_labels needs labels");
  INR_REQUIRE((((uintptr_t)vertices | (uintptr_t)faces | (uintptr_t)colors | (uintptr_t)rgb | (uintptr_t)ax_w |
                (uintptr_t)ax_l | (uintptr_t)ax_h) & 3) == 0, "misaligned buffer (4 bytes)");
  INR_REQUIRE(ext_w == ext_w && ext_l == ext_l && ext_h == ext_h, "NaN extent");
  if (V == 0 && F == 0) return INR_OK;
  const char* ws = static_cast<const char*>(workspace);
  const int32_t* voff = reinterpret_cast<const int32_t*>(ws);
  const int32_t* bpre_t = reinterpret_cast<const int32_t*>(ws + lay.off_bsum_t);
  const uint8_t* mask = reinterpret_cast<const uint8_t*>(ws + lay.off_mask);
  MeshAxes A;
  A.ax[0] = ax_w; A.ax[1] = ax_l; A.ax[2] = ax_h;
  A.ext[0] = ext_w; A.ext[1] = ext_l; A.ext[2] = ext_h;
  hipStream_t st = as_stream(s);
  const unsigned nb = (unsigned)lay.n_blocks;
  if (V > 0) hipLaunchKernelGGL(k_mesh_vertices, dim3(nb), dim3(kMeshBlock), 0, st, p, A, rgb, mask, voff, V, vertices, colors);
  if (F > 0) hipLaunchKernelGGL(k_mesh_faces, dim3(nb), dim3(kMeshBlock), 0, st, p, mask, voff, bpre_t, F, faces, face_labels);
  return check_launch("inr_mesh_emit");
}
