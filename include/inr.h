/*
 * inr.h - C ABI of libinr_hip.so: the MI355X (gfx950) implementation of the
 * instance-field NeRF render/train hot path.
 *
 * This is the drop-in boundary.  Every entry point
 * replaces one function of the reference's torch-ngp extension modules.  Those
 * modules are an UN-VENDORED SUBMODULE of the reference
 * (/root/reference/.gitmodules:4-6, pinned in prose at
 * /root/reference/README.md:27,59 to zymk9/torch-ngp @ 6be6af19), so the
 * "replaces" notes below name the upstream extension symbol and the survey
 * row instead of a file:line
 * inside /root/reference.  The one FFI call site that IS in the reference tree,
 * roi_align_3d (/root/reference/nerf_rcnn/model/utils.py:608), is a "next" row
 * (section 8f, f2) and is declared at the end of this header.
 *
 * Conventions (chosen to fix the flaws of the reference's only in-tree
 * extension, /root/reference/nerf_rcnn/model/rotated_iou/cuda_op/):
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless
 *     marked "host"; buffers are owned and sized by the caller; nothing is
 *     allocated or freed inside the library;
 *   - every launch goes onto the stream passed in (cf. the default-stream bug at
 *     sort_vert_kernel.cu:137-138); no call synchronises the device;
 *   - return value 0 = success, negative = INR_E*; never exit()/abort()
 *     (cf. cuda_utils.h:26-35); inr_last_error() gives a message for the
 *     calling thread;
 *   - arrays are dense row-major, fp32 unless stated.
 */
#ifndef INR_H
#define INR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an existing prototype changes or an entry point is removed (round 2 changed four argument lists
 * without a bump: a stale library or an external caller built against the old header was only rejected by accident).
 * instance_nerf_amd/_lib.py refuses a library whose version differs from the one it was written against.
 * 10: inr_instance_lattice, inr_instance_volume_stats.
 * 11: the fp16 variants folded into their base entry points as a `numerics` argument (INR_NUMERICS_*).
 * 12: inr_mesh_workspace_bytes, inr_mesh_count, inr_mesh_emit.
 * 13: inr_components_workspace_bytes, inr_components_label, inr_components_filter.
 * (inr_ssim_workspace_bytes and inr_ssim_forward were ADDED under 13: no prototype changed, nothing was removed; a
 * library built before them is named by the binding's loader, symbol by symbol.  inr_confusion_ids and
 * inr_confusion_logits likewise, inr_box_match_gt_max and inr_box_match_assign, and the four inr_fcos_* exports.) */
#define INR_ABI_VERSION 13
#define INR_MAX_LEVELS 16

enum {
  INR_OK = 0,
  INR_EINVAL = -1,   /* bad argument (null pointer, size, unsupported shape) */
  INR_ELAUNCH = -2,  /* hipLaunch / runtime error, see inr_last_error()       */
  INR_ENODEV = -3    /* no usable gfx950 device                                */
};

typedef void* inr_stream_t; /* a hipStream_t; NULL = the null stream */

/* `numerics` of the fused field entry points: 0 is the default (fp32 table, MLP GEMMs in the three-pass bf16 split that
 * keeps results fp32-class); each entry point lists the other values it accepts, anything else is INR_EINVAL.  Both
 * bits together are upstream's `-O` numerics, opt-in, for fields that are only evaluated (inference; the frozen NeRF of
 * the instance stage): NeRFNetwork.half_table + mlp_fp16, Trainer(fp16=True).  INR_NUMERICS_MLP_F16 does not exist in
 * the -DINR_MLP_FP32 build.                                                                                          */
enum {
  INR_NUMERICS_TABLE_F16 = 1, /* the table is an fp16 copy (T x 2 binary16): 11 significant bits, outputs ~1e-3 off  */
  INR_NUMERICS_MLP_F16 = 2    /* ONE fp16 MFMA pass per MLP GEMM (weights and activations rounded to fp16, fp32
                                 accumulation; 2^-12 relative per operand), weights packed with this same bit          */
};

/* Host-side description of a multiresolution hash grid.  Filled by
 * the caller (instance_nerf_amd.gridencoder.level_table) so host and device
 * index from the same numbers. */
typedef struct inr_grid_desc {
  int32_t num_levels;                    /* L <= INR_MAX_LEVELS                     */
  int32_t level_dim;                     /* F, features per row; 2 supported        */
  uint32_t offsets[INR_MAX_LEVELS + 1];  /* first row of each level; [L] = T        */
  float scales[INR_MAX_LEVELS];          /* pos = x01 * scale + 0.5                 */
  uint32_t resolutions[INR_MAX_LEVELS];  /* ceil(scale) + 1; dense stride = res + 1 */
  uint32_t hashed[INR_MAX_LEVELS];       /* 1: spatial hash, 0: dense index         */
} inr_grid_desc;

int inr_abi_version(void);
const char* inr_last_error(void);
/* Fills props[0..3] = {CU count, wavefront size, LDS bytes per CU, gcn arch number}. */
int inr_device_info(int32_t device, int64_t* props);
/* No upstream counterpart.  For a caller that renders view after view with the march of view i+1 on one stream and
 * the field kernel of view i on another (NeRFRenderer.run_cuda(shade_stream=...)): on != 0 makes the eval field
 * launch (inr_nerf_forward_table) and the march launches (inr_march_rays_train_count, inr_march_rays_patch_write)
 * request extra LDS per workgroup, which is how a launch tells the dispatcher to keep one field workgroup and a
 * bounded number of march workgroups per CU.  Results do not change; process-wide; off by default.  on >= 1024: the
 * field workgroup's request in BYTES instead of the default 84 KB (not clamped: a request no CU can satisfy makes the
 * next field launch return INR_ELAUNCH); negative values and 2..1023 are INR_EINVAL.                               */
int inr_set_overlap_placement(int32_t on);
/* THREADING / MULTI-DEVICE NOTE for the three mode switches of this header - inr_set_overlap_placement,
 * inr_set_march_mode, inr_roi_align_3d_set_mode: each writes one plain process-global variable that every later launch
 * of the library reads, on every device and every stream.  They are meant to be set once, before the work starts, by
 * the one process that drives one GPU (the deployment this library is written for).  They are NOT thread-safe and NOT
 * per-device: a host that drives several devices from one process, or flips a mode from one thread while another thread
 * launches, gets whichever value the launch happens to read (every value selects a correct kernel - results do not
 * depend on them beyond fp32 summation order in RoIAlign - only the speed and the LDS footprint change).  Everything
 * else in the library is stateless apart from inr_last_error()'s thread-local message.                              */
/* No upstream counterpart.  Which marcher inr_march_rays_train_count / _write use: -1 (default) by batch size
 * (wave per ray up to 32768 rays, lane per ray above), 0 lane per ray, 1 wave per ray.  Both produce the same
 * bits; the parity tests run both.  Process-wide.  (The library reads no environment variables.)                  */
int inr_set_march_mode(int32_t mode);

/* ---- rays: generation (replaces nerf/utils.py::get_rays) and ray/AABB (a2) -------------
 * poses [B,4,4] camera-to-world row-major; pixel `inds[k]` (flat j*W+i; NULL = 0..n-1) -> rays_o/rays_d [B,n,3]:
 * dir = ((i+.5-cx)/fx, (j+.5-cy)/fy, 1) normalised and rotated by the pose, origin = translation.     */
int inr_get_rays(const float* poses, int64_t B, float fx, float fy, float cx, float cy, int32_t W,
                 const int64_t* inds /*[n] nullable*/, int64_t n, float* rays_o, float* rays_d, inr_stream_t s);

/* One training batch of a loader whose images are resident on the device, in ONE launch (round 6; replaces the body of
 * upstream's nerf/provider.py::NeRFDataset.collate [U] - torch.randint pixel draw, get_rays, image gather, mask gather -
 * for the loader of the reference's two training stages, /root/reference/README.md:58-66; mask format
 * /root/reference/Mask2Former_sample/match_seg.py:131-140).  Sample k of step `step` (0 <= step < 2^31) draws the pixel
 *   inds[k] = ((mix64(seed + 0x9E3779B97F4A7C15 * (step * 2^32 + k)) >> 32) * (H*W)) >> 32      (SplitMix64 finaliser)
 * of ONE H x W image (H*W < 2^31): a counter-based draw with replacement, reproducible from (seed, step) alone;
 * rays_o / rays_d [n,3] as inr_get_rays for those pixels of `pose` [4,4] (bit-identical); rgb [n,channels] =
 * image[inds] (image float [H*W, channels], channels 3 or 4; nullable -> not gathered); labels int64 [n] = mask[inds]
 * (mask int32 [H*W], nullable; ids >= num_instances have no logit and become -1, -1 stays the ignore label).           */
int inr_sample_training_batch(const float* pose /*[4,4]*/, float fx, float fy, float cx, float cy, int32_t H, int32_t W,
                              const float* image /*nullable*/, int32_t channels, const int32_t* mask /*nullable*/,
                              int32_t num_instances, int64_t seed, int64_t step, int64_t n, int64_t* inds /*[n]*/,
                              float* rays_o, float* rays_d, float* rgb /*[n,channels]*/, int64_t* labels /*[n]*/,
                              inr_stream_t s);

/* The same batch with the pixels drawn from ONE image's row of a coarse error map (upstream's --error_map /
 * opt.error_map [U]: NeRFDataset.error_map [n_images, 128*128] and get_rays(error_map=...), a torch.multinomial draw of
 * n cells without replacement, then a uniform pixel inside each cell), still ONE launch (one workgroup; no read-back, no
 * float atomics).  error_map float [cells*cells], 1 <= cells <= 128, n <= cells*cells.  The draw has multinomial's
 * distribution (exponential race, Efraimidis-Spirakis: the n smallest keys E_c / w_c win) and is a function of
 * (seed, step, cell) alone:
 *   ctr(s, c) = 2^63 + step * 2^32 + s * 2^16 + c     stream s = 0 key, 1 row jitter, 2 column jitter (bit 63 keeps them
 *                                                     apart from inr_sample_training_batch's counters step * 2^32 + k)
 *   m_s(c)    = mix64(seed + 0x9E3779B97F4A7C15 * ctr(s, c)) >> 40          (24 bits)
 *   E_c       = -ln((m_0(c) + 0.5) * 2^-24) by a fixed binary32 sequence (csrc/raymarch.hip neg_ln_u24: integer
 *               exponent / mantissa split, s = (f-1)/(f+1), degree-4 polynomial in s*s, separate multiplies and adds;
 *               within 1e-6 relative of the exact value for every m)
 *   key_c     = E_c / w_c, an IEEE binary32 division; w_c <= 0 or NaN: +inf (such a cell is taken only after every
 *               positive one, lowest index first); w_c = +inf: 0.  Keys are >= 0: their bits order as unsigned integers.
 *   winners   = the n smallest (key bits, c) pairs - equal bits resolve to the smaller cell index.
 * Outputs are in ASCENDING cell index: inds_coarse[k] = c (upstream's key), and the pixel by upstream's rule in binary32,
 * every product and sum rounded on its own:
 *   cx_ = c / cells, cy_ = c % cells, sx = (float)H / (float)cells, sy = (float)W / (float)cells,
 *   r1 = (float)m_1(c) * 2^-24, r2 = (float)m_2(c) * 2^-24,
 *   px = min((int)((float)cx_ * sx + r1 * sx), H - 1), py = min((int)((float)cy_ * sy + r2 * sy), W - 1),
 *   inds[k] = px * W + py;
 * rays, rgb and labels for inds exactly as inr_sample_training_batch (the same device code).  Restated bit for bit by
 * tests/error_map_reference.py.                                                                                       */
int inr_sample_training_batch_weighted(const float* pose /*[4,4]*/, float fx, float fy, float cx, float cy, int32_t H,
                                       int32_t W, const float* image /*nullable*/, int32_t channels,
                                       const int32_t* mask /*nullable*/, int32_t num_instances,
                                       const float* error_map /*[cells*cells]*/, int32_t cells, int64_t seed, int64_t step,
                                       int64_t n, int64_t* inds /*[n]*/, int64_t* inds_coarse /*[n]*/, float* rays_o,
                                       float* rays_d, float* rgb /*[n,channels]*/, int64_t* labels /*[n]*/,
                                       inr_stream_t s);
/* The error map's update after a training step (upstream's Trainer.train_step [U]: error = MSELoss(reduction='none')
 * (pred, gt).mean(-1), map[inds_coarse] = 0.1 * map[inds_coarse] + 0.9 * error), one launch: for ray k with cell
 * c = inds_coarse[k], d = pred[k] - target[k]:  e = ((d0*d0 + d1*d1) + d2*d2) / 3.0f;  map[c] = 0.1f * map[c] + 0.9f * e
 * (separate multiplies and adds).  pred, target float [N,3]; map float [cells*cells] (one image's row), 1 <= cells <= 128.
 * An index outside [0, cells*cells) is skipped.  inr_sample_training_batch_weighted hands out distinct cells, so its
 * indices never race; for a caller's own DUPLICATE indices which of the rays writes last is unspecified.              */
int inr_error_map_update(const float* pred /*[N,3]*/, const float* target /*[N,3]*/, const int64_t* inds_coarse /*[N]*/,
                         float* map /*[cells*cells]*/, int64_t N, int32_t cells, inr_stream_t s);

int inr_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb /*[6]*/,
                           int64_t N, float min_near, float* nears, float* fars, inr_stream_t s);
/* The same with per-ray labels (int64 [N]): a ray whose label equals `ignore_index` is reported as a miss (near = far =
 * FLT_MAX), so the training march gives it no samples.  No upstream counterpart: upstream marches and evaluates the
 * rays its mask loss then ignores (cross entropy with ignore_index -1 over matched masks,
 * /root/reference/Mask2Former_sample/match_seg.py:111-138 writes the -1s).  Used by Trainer(stage="instance").          */
int inr_near_far_from_aabb_skip(const float* rays_o, const float* rays_d, const float* aabb /*[6]*/, int64_t N,
                                float min_near, const int64_t* labels, int64_t ignore_index, float* nears, float* fars,
                                inr_stream_t s);

/* ---- occupancy helpers (replace raymarching.morton3D / morton3D_invert / packbits, a3) */
int inr_morton3D(const int32_t* coords /*[N,3]*/, int64_t N, int32_t* indices, inr_stream_t s);
int inr_morton3D_invert(const int32_t* indices, int64_t N, int32_t* coords /*[N,3]*/, inr_stream_t s);
/* bitfield[k] bit i = grid[8k+i] > thresh; n_bytes = cells / 8 */
int inr_packbits(const float* grid, int64_t n_bytes, float thresh, uint8_t* bitfield, inr_stream_t s);

/* ---- occupancy-grid update (replaces the tensor-op body of NeRFRenderer.update_extra_state, a3) -------------------
 * One cascade at a time; the grid is in Morton order.  inr_occ_cell_positions: query position of cell morton_idx[i]
 * (NULL = cell i) - centre (2c/(H-1) - 1) * (b - b/H) plus (2 noise - 1) * b/H, noise [n,3] in [0,1) or NULL.
 * inr_occ_update: grid = max(grid * decay, sigma * density_scale) where both >= 0 (cells at -1 stay out), for all
 * cells (morton_idx NULL, m == n_cells, sigma in Morton order) or the listed ones (tmp = scratch [n_cells]);
 * *mean_sum (double, caller zeroes it once per update) accumulates sum(max(grid, 0)).
 * inr_packbits_mean: packbits with thresh = min(*mean_sum / n_cells, density_thresh) formed on the device (no host
 * round trip between the update and the bitfield); mean_out (nullable) receives the mean; with n_counters > 0
 * stats_out = {mean, sum_k counters[k * counter_stride]} - the one 16-byte read-back of an update (mean density and
 * the sample totals of the last steps, which size the next steps' buffers).                                         */
/* mark_untrained_grid (a3): grid[cas][cell] = -1 for every cell (Morton order) that none of the B training cameras
 * sees - poses [B,4,4] camera-to-world row-major, pinhole (fx, fy, cx, cy): the cell centre x in camera frame
 * cam = R^T (x - t) is seen if z > 0, |x| < cx/fx z + 2 half, |y| < cy/fy z + 2 half (half = half a cell).        */
int inr_mark_untrained_grid(const float* poses, int32_t B, float fx, float fy, float cx, float cy, int32_t H,
                            int32_t cascade, float bound, float* grid /*[cascade, H^3]*/, inr_stream_t s);
int inr_occ_cell_positions(const int32_t* morton_idx, const float* noise, int64_t n, int32_t H, float cascade_bound,
                           float* xyz /*[n,3]*/, inr_stream_t s);
int inr_occ_update(float* grid /*[n_cells]*/, const float* sigma /*[m]*/, const int32_t* morton_idx /*[m] or NULL*/,
                   int64_t n_cells, int64_t m, float decay, float density_scale, float* tmp, double* mean_sum,
                   inr_stream_t s);
int inr_packbits_mean(const float* grid, int64_t n_cells /*all cascades*/, const double* mean_sum, float density_thresh,
                      uint8_t* bitfield, float* mean_out /*nullable*/, const int32_t* counters /*nullable*/,
                      int32_t n_counters, int32_t counter_stride /*in int32*/, double* stats_out /*[2]*/,
                      inr_stream_t s);
/* The steady-state cell choice of update_extra_state (after the first 16 updates; one cascade): n cells uniformly at
 * random + n picks, with replacement, among the cells with grid > 0 - upstream's randint coordinates and
 * nonzero(grid > 0)[randint] - in three launches.  u [4n] uniform in [0,1): slice draws [2n] then in-slice draws [2n]
 * (uniform half first).  morton_idx [2n] receives the cells (Morton indices), uniform half first; each half comes out
 * grouped by 4096 slices of the Morton range / of the occupied ranks (an i.i.d. sample drawn as multinomial slice
 * counts + uniform positions inside the slices), which is what lets the field kernel evaluate them at its coherent
 * rate.  No cell occupied: the occupied half is cell 0.  Exact restatement: oracle/occupancy.py::sample_cells.   */
int64_t inr_occ_sample_workspace_bytes(int64_t n_cells);
int inr_occ_sample_cells(const float* grid /*[n_cells] Morton order*/, int64_t n_cells, const float* u /*[4n]*/,
                         int64_t n, int32_t* morton_idx /*[2n]*/, void* workspace, inr_stream_t s);

/* ---- training march (replaces raymarching.march_rays_train, a4) ----------------------
 * Deterministic: sample slots are an exclusive scan of the per-ray counts in ray
 * order.  Call inr_march_rays_train_count first (fills counts/offsets and
 * counter[0] = total samples, counter[1] = N), size the outputs (M rows), then
 * inr_march_rays_train_write.  A ray whose offset + count > M is dropped (its
 * rays row is still written).  workspace: inr_march_workspace_bytes(N, sample_cap), 8-byte aligned.
 * sample_cap > 0: the count pass records, one bit per step candidate (the sequence t_{i+1} = t_i + dt(t_i) is
 * independent of the grid), which of each ray's first sample_cap candidates were emitted; the write pass
 * regenerates the sequence and emits at the set bits instead of walking the occupancy grid again (rays that
 * need more candidates are re-marched); pass the SAME workspace and sample_cap to the write call.  Results
 * are identical.
 * Preconditions (every march entry point: _count, _write, the patch writers, inr_march_rays): each ray's direction is a
 * nonzero vector, and far is finite wherever near < far - what inr_near_far_from_aabb produces (a miss is
 * near = far = FLT_MAX and is never marched).  They are not checked: a zero direction, or an unbounded far in empty
 * space, gives a walk that does not end, because t stops growing once the step falls below half an ulp of t.    */
/* 1 when inr_march_rays_train_write zero-fills the rows of xyzs / dirs / deltas that no ray owns by itself (the staged
 * wave-per-ray marcher does; the caller may then pass uninitialised buffers), 0 when the caller must zero them first. */
int inr_march_write_fills_unowned_rows(int64_t N, int32_t sample_cap, int32_t max_steps);
int64_t inr_march_workspace_bytes(int64_t N, int32_t sample_cap);
int inr_march_rays_train_count(const float* rays_o, const float* rays_d, const uint8_t* bitfield,
                               float bound, float dt_gamma, int32_t max_steps, int64_t N,
                               int32_t cascade, int32_t H, const float* nears, const float* fars,
                               const float* noises /*nullable*/, int32_t* rays /*[N,3]*/,
                               int32_t* counter /*[2]*/, void* workspace, int32_t sample_cap, inr_stream_t s);
int inr_march_rays_train_write(const float* rays_o, const float* rays_d, const uint8_t* bitfield,
                               float bound, float dt_gamma, int32_t max_steps, int64_t N,
                               int32_t cascade, int32_t H, int64_t M, const float* nears,
                               const float* fars, const float* noises /*nullable*/,
                               const int32_t* rays /*[N,3] from _count*/, float* xyzs /*[M,3]*/,
                               float* dirs /*[M,3]*/, float* deltas /*[M,2]*/, const void* workspace,
                               int32_t sample_cap, inr_stream_t s);

/* ---- fused full-frame inference path (replaces the alive-ray loop of NeRFRenderer.run_cuda, a5) ----
 * Same counting pass as training (inr_march_rays_train_count), then samples are written in the
 * PATCH-INTERLEAVED layout: rays in groups of 16 consecutive rays; inside a group
 *   slot(r, k) = rays[g0,1] + sum_i min(c_i, k) + #{ i < r : c_i > k }
 * (all k-th samples of a group adjacent).  A group whose slots do not fit in M is dropped whole.
 * inr_composite_rays_patch_forward composites that layout (per ray, in k order, stop at T < T_thresh;
 * same arithmetic as the sequential training compositing); weights [M] (nullable unless extra is given)
 * receives the per-sample weight, which the K-channel pass (one wave per ray) then uses.              */
int inr_march_rays_patch_write(const float* rays_o, const float* rays_d, const uint8_t* bitfield,
                               float bound, float dt_gamma, int32_t max_steps, int64_t N,
                               int32_t cascade, int32_t H, int64_t M, const float* nears,
                               const float* fars, const float* noises /*nullable*/,
                               const int32_t* rays /*[N,3] from inr_march_rays_train_count*/,
                               float* xyzs, float* dirs /*nullable if ray_ids*/, float* deltas,
                               const void* workspace, int32_t sample_cap, int32_t* ray_ids /*[M] nullable*/,
                               int32_t normalise /*1: xyzs = (p+bound)/(2 bound)*/, inr_stream_t s);
int inr_composite_rays_patch_forward(const float* sigmas, const float* rgbs, const float* deltas,
                                     const int32_t* rays, int64_t N, int64_t M, float T_thresh,
                                     const float* extra /*[M,K] nullable*/, int32_t K,
                                     float* weights_sum, float* depth, float* image,
                                     float* extra_out /*[N,K]*/, float* weights /*[M]*/,
                                     uint64_t* skippable /*device, nullable: += samples of steps at which a whole
                                     16-ray group is already below T_thresh - what inr_nerf_render would skip*/,
                                     inr_stream_t s);
/* Records form of the two above (the frame path's 8-byte sample records): a sample is handed on as t [M] (float) and
 * ray_ids [M] (int32), two separate arrays in the same patch-interleaved slots - same count pass, mask replay, re-march
 * of rays past the capture row and rule for a group that does not fit; no position is formed, clamped or normalised.
 * Position, dt and t - t_prev are functions of (ray, t): inr_nerf_forward_table_records rebuilds x01, and
 * inr_composite_rays_patch_forward_records rebuilds (dt, t - t_prev) per ray from nears [N], noises [N] (nullable) and
 * the step parameters of the march - dt = step(t), tn = t + dt, delta = tn - last_t, last_t = near + step(near) * noise
 * at first and the previous sample's tn afterwards: the marcher's operations in its order, so every output has the bits
 * of the positions form.  (Neither the bitfield nor the bound enters the step rule.)                                  */
int inr_march_rays_patch_write_records(const float* rays_o, const float* rays_d, const uint8_t* bitfield,
                                       float bound, float dt_gamma, int32_t max_steps, int64_t N,
                                       int32_t cascade, int32_t H, int64_t M, const float* nears,
                                       const float* fars, const float* noises /*nullable*/,
                                       const int32_t* rays /*[N,3] from inr_march_rays_train_count*/,
                                       float* t /*[M]*/, int32_t* ray_ids /*[M]*/, const void* workspace,
                                       int32_t sample_cap, inr_stream_t s);
int inr_composite_rays_patch_forward_records(const float* sigmas, const float* rgbs, const float* t /*[M]*/,
                                             const int32_t* rays, int64_t N, int64_t M, float T_thresh,
                                             const float* nears /*[N]*/, const float* noises /*[N] nullable*/,
                                             float dt_gamma, int32_t max_steps, int32_t cascade, int32_t H,
                                             const float* extra /*[M,K] nullable*/, int32_t K,
                                             float* weights_sum, float* depth, float* image,
                                             float* extra_out /*[N,K]*/, float* weights /*[M]*/,
                                             uint64_t* skippable /*device, nullable*/, inr_stream_t s);
/* No upstream counterpart in the submodule's extension; the counterpart of the reference pipeline's project_3d_masks step
 * (voxel masks of nerf_rcnn/run_rcnn.py:652-666 projected into the training images that
 * Mask2Former_sample/match_seg.py:99-102 reads).  For the samples of a patch-interleaved frame (inr_march_rays_patch_write)
 * and their compositing weights (inr_composite_rays_patch_forward, weights != NULL): out[ray][k_base + i] =
 * sum over the ray's samples of w * bit_i(mask_words[cell(x)]), i < k_count <= 32; mask_words uint32 [W,L,H], bit i = mask
 * k_base + i contains the voxel; cell = floor((x - lo) / (hi - lo) * (W,L,H)), samples outside the box contribute nothing;
 * bbox: HOST array lo[3], hi[3]; out float [N, k_total].                                                               */
int inr_project_masks_patch(const float* xyzs, const float* weights, const int32_t* rays, int64_t N, int64_t M,
                            const uint32_t* mask_words, int32_t W, int32_t L, int32_t H, const float* bbox /*host*/,
                            int32_t k_total, int32_t k_base, int32_t k_count, float* out, inr_stream_t s);

/* ---- inference march/composite (replace raymarching.march_rays / composite_rays, a5) */
int inr_march_rays(int64_t n_alive, int32_t n_step, const int32_t* rays_alive, const float* rays_t,
                   const float* rays_o, const float* rays_d, float bound, float dt_gamma,
                   int32_t max_steps, int32_t cascade, int32_t H, const uint8_t* bitfield,
                   const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas,
                   inr_stream_t s);
int inr_composite_rays(int64_t n_alive, int32_t n_step, int32_t* rays_alive, float* rays_t,
                       const float* sigmas, const float* rgbs, const float* deltas,
                       float* weights_sum, float* depth, float* image, float T_thresh,
                       const float* extra /*[n_alive*n_step,K] nullable*/, float* extra_acc /*[N,K]*/,
                       int32_t K, inr_stream_t s);
/* order-preserving compaction of rays_alive >= 0; n_out (device int32[2]) = {survivors, n_alive};
 * `out` needs room for n_alive + inr_march_workspace_bytes(n_alive, 0)/4 int32 (list first, scratch after) */
int inr_compact_alive(const int32_t* rays_alive, int64_t n_alive, int32_t* out, int32_t* n_out,
                      inr_stream_t s);

/* ---- compositing for training (replaces raymarching.composite_rays_train fwd/bwd, a12/a13) ----
 * M = rows of the sample arrays: a ray with offset + count > M was dropped by the march writer and
 * composites to zero (its gradient rows are left untouched - the caller zero-initialises them - unless the backward
 * is given total_dev, the device int32 with the marcher's sample total: the rays' rows then tile [0, total) and the
 * backward writes every row of grad_sigmas / grad_rgbs in [0, M) itself, zeros where no ray owns the row).
 * weights [M] (nullable unless extra is given): receives the per-sample compositing weight
 * w = alpha * T (0 behind the termination point); the K-channel forward/backward use it.
 * sample_ray [M] (nullable; needs weights): receives, for every sample a ray owns, the row rays[n][0] of that ray's
 * outputs - what inr_instance_head_backward looks dL/d(rendered logits) up by.                       */
int inr_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* deltas,
                                     const int32_t* rays, int64_t N, int64_t M, float T_thresh,
                                     const float* extra /*[M,K] nullable*/, int32_t K,
                                     float* weights_sum, float* depth, float* image,
                                     float* extra_out /*[N,K]*/, float* weights /*[M]*/,
                                     int32_t* sample_ray /*[M]*/, inr_stream_t s);
/* The K-channel half of the call above on its own: extra_out[rays[n][0]][ch] = sum over the ray's samples of
 * weights[i] * extra[i][ch] (weights from an earlier inr_composite_rays_train_forward; rows of dropped rays are zero). */
/* Optional cross-entropy epilogue (labels non-null): the wave that has just rendered a ray's K logits also forms that
 * ray's cross-entropy row against labels[row] (int64 [N]; ignore_index rows skipped; classes 0 .. n_classes-1, K may be
 * padded beyond) - grad_pix [N,K] = softmax - onehot for the kept rows (NOT yet divided by their number), and a second
 * small launch leaves loss_out[0..3] = {mean loss over the kept rows, 1 / kept, kept, labels out of range}; a label that
 * is neither ignore_index nor a class makes the loss NaN.  workspace: N * 16 bytes.  inr_instance_head_backward takes
 * grad_pix with loss_out + 1 as one of its scale pointers.                                                         */
int inr_composite_rays_extra_forward(const float* weights /*[M]*/, const float* extra /*[M,K]*/, const int32_t* rays,
                                     int64_t N, int64_t M, int32_t K, float* extra_out /*[N,K]*/,
                                     const int64_t* labels /*nullable*/, int32_t n_classes, int64_t ignore_index,
                                     float* grad_pix, void* workspace, float* loss_out, inr_stream_t s);
int inr_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_image,
                                      const float* grad_extra_out /*nullable*/, const float* sigmas,
                                      const float* rgbs, const float* extra, const float* deltas,
                                      const int32_t* rays, const float* weights_sum,
                                      const float* image, const float* weights /*[M] from forward*/,
                                      int64_t N, int64_t M, float T_thresh, int32_t K,
                                      float* grad_sigmas, float* grad_rgbs /*both nullable: frozen NeRF*/,
                                      float* grad_extra /*[M,K] nullable*/, const int32_t* total_dev /*nullable*/,
                                      inr_stream_t s);

/* ---- hash grid (replaces gridencoder grid_encode_forward / _backward, a7/a8) -------- */
int inr_grid_encode_forward(const float* x /*[M,3]*/, const float* embeddings /*[T,F]*/,
                            const inr_grid_desc* desc /*host*/, int64_t M, float bound,
                            float* out /*[M,L*F]*/, inr_stream_t s);
/* grad_embeddings is ACCUMULATED into (caller zeroes it) */
int inr_grid_encode_backward(const float* x, const float* grad_out /*[M,L*F]*/,
                             const inr_grid_desc* desc /*host*/, int64_t M, float bound,
                             float* grad_embeddings /*[T,F]*/, inr_stream_t s);

/* same, processing the samples in the order given (int32 permutation of 0..M-1, nullable): the sum is
 * order-independent up to fp32 rounding; a spatial (Morton) order makes the atomics address-adjacent */
int inr_grid_encode_backward_ordered(const float* x, const float* grad_out, const int32_t* order,
                                     const inr_grid_desc* desc /*host*/, int64_t M, float bound,
                                     float* grad_embeddings /*[T,F]*/, inr_stream_t s);
/* Gradient with respect to the input coordinates (upstream's dy_dx path of gridencoder, taken when the positions
 * require grad): grad_x [M,3] = sum over levels and corners of grad_out . row * d(weight)/dx * scale_l / (2 bound);
 * zero for out-of-range points.  A.e. derivative of the trilinear interpolation (cells are piecewise linear).     */
int inr_grid_encode_backward_input(const float* x, const float* grad_out /*[M,L*F]*/, const float* embeddings,
                                   const inr_grid_desc* desc /*host*/, int64_t M, float bound, float* grad_x,
                                   inr_stream_t s);
/* The same scatter restricted to levels [level_lo, level_hi): a caller that all-reduces the table gradient over
 * several GPUs launches it in two or three level ranges and starts the collective on each row range
 * [offsets[level_lo], offsets[level_hi]) as soon as its launch is queued (nerf/network.py::_table_backward).      */
int inr_grid_encode_backward_levels(const float* x, const float* grad_out, const int32_t* order,
                                    const inr_grid_desc* desc, int64_t M, float bound, float* grad_embeddings,
                                    int32_t level_lo, int32_t level_hi, inr_stream_t s);

/* Fixed-point form of the table-gradient scatter (round 6; OPT-IN - the product's default stays the fp32 atomics of
 * upstream's grid_encode_backward, see the end of this comment).  Why: on MI355X every atomic is executed by the memory-side unit, which takes int32 adds at 26.9 G
 * requests/s against 21.0 for fp32 (tools/micro/atomic_type_bench.hip) - the scatter is the largest kernel of a
 * training step - and integer sums do not depend on the order of arrival: the gradient becomes bit-reproducible.
 * fx_state: INR_GRID_FX_STATE_FLOATS device floats per table, zero-initialised by the caller once, then owned by these
 * three calls: [0,16) the scale of each level for the current step (a power of two; 0 = this level uses fp32 atomics),
 * [16,32) reference magnitudes, [32,48) the last step's largest |row gradient| per level, [48] steps so far in which at
 * least one level (any level) ran on integer sums,
 * [49] near misses so far, [80,96) the largest fraction of the integer range a row sum of each level has ended at so far
 * (never above 1: a row that wrapped reads as a smaller value, a wrap cannot be observed here), the
 * rest scratch.  GUARANTEE: every value the scatter adds to a row - the sum v of a run of equal rows inside one wave,
 * possibly a single contribution - must have an integer image: |v x scale| < 2^31 (2^63 for int64 sums).  One that has
 * none (out of range - the conversion would saturate -, v x scale beyond fp32, Inf, NaN) raises its level's flag and
 * turns that level's WHOLE gradient into NaN in the finishing pass - as loud as the NaN rows fp32 atomics leave; the
 * scale update then resets the level (scale 0, reference 0, flag cleared: fp32 atomics for one step).
 * NOT detected: values that each fit but whose sum over one ROW, arriving from different waves, ends outside the
 * range: that row wraps silently into a finite wrong gradient (sums that leave the range and come back are exact).
 * Per training step, on one stream:
 *   inr_grid_encode_backward_levels_fx   scatter of a level range; a level with a scale accumulates round(w g scale) as
 *                                        int32 bit patterns in grad_embeddings (zeroed by the caller), others fp32;
 *                                        fx_state NULL = inr_grid_encode_backward_levels
 *   inr_grid_grad_finish_fx              in place: int32 sums -> fp32 gradients (exact: the scale is a power of two) and
 *                                        the level's largest |gradient|; afterwards grad_embeddings is an ordinary fp32
 *                                        gradient (call it for every level range that was scattered, fp32 levels too)
 *   inr_grid_fx_update                   once per step after all ranges (sum_bits = 32): next step's scales = 2^floor(log2(2^30 /
 *                                        (headroom x reference))), reference = max(this step's max, 0.97 reference).
 * A level runs on fp32 atomics only while it has no reference: before its first step (the Python host primes the scales
 * with one extra scatter into a scratch buffer, so that no training step ever depends on the order of arrival) and
 * after an all-zero or non-finite gradient.  A near miss (a step that used more than 1/8 of the int32 range) is
 * counted; a row's FINAL sum that grows more than `headroom` times (128 in the product) against the reference - the
 * largest of the last ~50 steps - poisons its level when a single wave's run sum is that large and otherwise wraps
 * unseen (see above; the wrapped row's maximum is arbitrary, so the next scale is not necessarily coarser); measured
 * peak use of the range over 3000 training steps: 0.06.  Quantisation: a row gradient is a multiple of headroom x
 * reference x 2^-30 (1.2e-7 of the level's recent largest at 128, ~5e-7 of a typical step's).
 * Why opt-in: a row whose gradient is below half a quantum gets none, and Adam with eps = 1e-15 (upstream's optimiser)
 * moves a row by a full lr step whatever its gradient's SIZE - rows fed only by weak samples learn at full speed under
 * fp32 atomics and not at all here.  Measured: identical PSNR / mIoU after 1500 + 1500 steps on the bench scene, but
 * held-out mIoU 0.75-0.82 against 0.80-0.86 on the shorter schedule of tests/test_pipeline_e2e.py
 * (profiles/r06_NOTES.txt 5).  Host switch: INR_FX_GRAD=1 / Trainer(fixed_point_grad=True).                          */
#define INR_GRID_FX_STATE_FLOATS 4192
int inr_grid_encode_backward_levels_fx(const float* x, const float* grad_out, const int32_t* order,
                                       const inr_grid_desc* desc, int64_t M, float bound, float* grad_embeddings,
                                       int32_t level_lo, int32_t level_hi, float* fx_state /*nullable*/,
                                       inr_stream_t s);
int inr_grid_grad_finish_fx(float* grad_embeddings, const inr_grid_desc* desc /*host*/, int32_t level_lo,
                            int32_t level_hi, float* fx_state, inr_stream_t s);
int inr_grid_fx_update(float* fx_state, int32_t num_levels, float headroom, int32_t sum_bits /*32 | 64*/, inr_stream_t s);
/* The 64-bit form of the same (opt-in too): the sums live in a caller-owned int64 accumulator acc64 [T,2] (zero-initialised
 * once; the finishing pass zeroes it again), the scale is 2^32 larger (sum_bits = 64 in inr_grid_fx_update; headroom 1024 in
 * the product) - a quantum of ~2e-16 of the level's recent maximum, below anything Adam with eps 1e-15 can see: the
 * FAITHFUL order-independent form (bit-reproducible steps, no weakly supervised row frozen).  The unit takes 8-byte integer
 * adds at 23.6 G requests/s (fp32 21.0, int32 26.9): about the fp32 scatter's speed after the extra pass over the
 * accumulator.  grad_embeddings receives the fp32 gradient from inr_grid_grad_finish_fx64 (levels without a scale are
 * scattered into it with fp32 atomics directly, as above).                                                            */
int inr_grid_encode_backward_levels_fx64(const float* x, const float* grad_out, const int32_t* order,
                                         const inr_grid_desc* desc, int64_t M, float bound, float* grad_embeddings,
                                         int64_t* acc64 /*[T,2]*/, int32_t level_lo, int32_t level_hi, float* fx_state,
                                         inr_stream_t s);
int inr_grid_grad_finish_fx64(int64_t* acc64, float* grad_embeddings, const inr_grid_desc* desc /*host*/, int32_t level_lo,
                              int32_t level_hi, float* fx_state, inr_stream_t s);

/* ---- 2-D hash grid (upstream's encoder_bg: get_encoder("hashgrid", input_dim=2, ...)) ----------------------------
 * The 3-D arithmetic minus an axis, with the same descriptor (it carries no dimension; its `hashed` flags come from
 * level_table(input_dim=2): a level is hashed iff (res+1)^2 > rows).  x [M,2] in [-bound, bound]:
 * x01 = (x + bound) / (2 bound); out of range on either axis (NaN included) -> zero features, no gradient;
 * pos = x01 * scale + 0.5 (separate multiply and add); corner k = 0..3, bit d of k = the +1 neighbour on axis d, weight
 * wx * wy, features accumulated in corner order; dense row cx + cy (res+1), hashed row (cx ^ cy 2654435761u) & (rows-1).
 * Backward: fp32 atomics into an ACCUMULATED grad_embeddings (the caller zeroes it); no input gradient (sphere
 * coordinates never require grad) and no fixed-point form.  out / grad_out [M, 2 L], 8-byte aligned.               */
int inr_grid2d_encode_forward(const float* x /*[M,2]*/, const float* embeddings, const inr_grid_desc* desc /*host*/,
                              int64_t M, float bound, float* out, inr_stream_t s);
int inr_grid2d_encode_backward(const float* x /*[M,2]*/, const float* grad_out, const inr_grid_desc* desc /*host*/,
                               int64_t M, float bound, float* grad_embeddings, inr_stream_t s);

/* ---- Background sphere model (upstream's bg_radius > 0; csrc/background.hip) -------------------------------------
 * inr_sph_from_ray: coords [N,2] (8-byte aligned) = where the ray leaves the sphere |p| = radius (the larger root), y up,
 * as (2 theta / pi - 1, phi / pi), in the operation order of raymarching.sph_from_ray, then clamped to [-1, 1] (NaN stays
 * NaN).  A ray that never meets the sphere (negative discriminant, or the exit point behind the origin) gets NaN
 * coordinates - for the 2-D grid that means zero features.
 *
 * inr_background_forward: bg [N,3] = sigmoid(w1 relu(w0 [sh4(rays_d), grid2d(coords)])) in ONE launch, one ray per lane:
 * embeddings / desc = a 4-level 2-D table read with bound 1 (8 features), w0 [64,24] and w1 [3,64] row-major fp32 (SH
 * columns first), fp32 FMAs in a fixed order.  coords_out (nullable, [N,2], 8-byte aligned) receives the coordinates,
 * bit-equal to inr_sph_from_ray's.  weights_sum [N] + image [N,3] (nullable, together): image += (1 - weights_sum) * bg
 * in place, a separate multiply and add - the background blend of an inference frame.
 *
 * inr_background_backward: recomputes the forward from its inputs (nothing else is saved) and, from grad_bg [N,3]:
 * grad_embeddings += the table gradient (fp32 atomics, 16 rows per ray; the caller zeroes it), grad_w0 [64,24] and
 * grad_w1 [3,64] WRITTEN (not accumulated).  The weight gradients are per-workgroup partial sums in `workspace`
 * (inr_background_workspace_bytes(N) bytes; INR_EINVAL for a negative N) added in workgroup order by a second tiny launch
 * inside the same call: the same inputs give the same bits.  N = 0 is valid and launches nothing (nothing is written). */
int inr_sph_from_ray(const float* rays_o /*[N,3]*/, const float* rays_d /*[N,3]*/, int64_t N, float radius,
                     float* coords /*[N,2]*/, inr_stream_t s);
int inr_background_forward(const float* rays_o, const float* rays_d, int64_t N, float radius, const float* embeddings,
                           const inr_grid_desc* desc /*host*/, const float* w0, const float* w1, float* bg,
                           float* coords_out /*nullable*/, const float* weights_sum /*nullable*/,
                           float* image /*nullable*/, inr_stream_t s);
int64_t inr_background_workspace_bytes(int64_t N);
int inr_background_backward(const float* grad_bg, const float* rays_o, const float* rays_d, int64_t N, float radius,
                            const float* embeddings, const inr_grid_desc* desc /*host*/, const float* w0,
                            const float* w1, float* grad_embeddings, float* grad_w0, float* grad_w1, float* workspace,
                            inr_stream_t s);

/* ---- SH (replaces shencoder sh_encode_forward / _backward, a10) ------------------------ */
int inr_sh_encode_forward(const float* d /*[M,3]*/, int64_t M, int32_t degree, float* out, inr_stream_t s);
int inr_sh_encode_backward(const float* grad_out, const float* d, int64_t M, int32_t degree,
                           float* grad_d, inr_stream_t s);
/* degree-4 SH of N ray directions in the lane order of the fused field kernel: out[n][q][ks] = sh[4 ks + q] */
int inr_sh_table_q(const float* d /*[N,3]*/, int64_t N, float* out /*[N,16], 16-byte aligned*/, inr_stream_t s);

/* ---- fused field evaluation (replaces NeRFNetwork.forward/density + the fork's
 * instance head, a9/a13; the MFMA kernel the north star asks for) ---------------------------
 * Weights are nn.Linear [out,in] row-major fp32, no bias:
 *   sigma_w0[64,32] sigma_w1[16,64] color_w0[64,31] color_w1[64,64] color_w2[3,64]
 *   inst_w0[64,32] inst_w1[64,64] inst_w2[K,64] (K <= 64, K % 16 == 0: a caller with another K zero-pads the rows, as NeRFNetwork does)
 * inr_*_pack_weights reorder them (on the host) into MFMA fragment order; the packed buffer is then copied to the
 * device by the caller.  numerics:
 *   - 0: the weights of the default numerics;
 *   - INR_NUMERICS_MLP_F16: fp16 values in the head slots of the same size and fragment layout, for the entry points
 *     called with that bit.                                                                   */
int64_t inr_nerf_packed_floats(void);
int inr_nerf_pack_weights(const float* sigma_w0, const float* sigma_w1, const float* color_w0,
                          const float* color_w1, const float* color_w2, float* packed /*host*/, int32_t numerics);
int64_t inr_instance_packed_floats(int32_t K);
int inr_instance_pack_weights(const float* w0, const float* w1, const float* w2, int32_t K,
                              float* packed /*host*/, int32_t numerics);
/* sigma[M] (= exp(h0) * density_scale), rgb[M,3] (nullable -> density only),
 * geo_feat[M,15] (nullable).  n_samples_dev: optional device int32 holding the
 * live row count (<= M); rows past it are skipped.  numerics:
 *   - 0: fp32 table (8-byte aligned);
 *   - INR_NUMERICS_TABLE_F16 | INR_NUMERICS_MLP_F16 (upstream's `-O`; the FROZEN NeRF of the instance stage): fp16
 *     table (4-byte aligned), weights packed with INR_NUMERICS_MLP_F16; rgb required, geo_feat must be NULL.        */
int inr_nerf_forward(const float* x, const float* d, int64_t M, const int32_t* n_samples_dev,
                     float bound, const void* embeddings, const inr_grid_desc* desc /*host*/,
                     const float* packed /*device*/, float density_scale, float* sigma, float* rgb,
                     float* geo_feat, int32_t numerics, inr_stream_t s);
/* Fused-frame variant of inr_nerf_forward: x01 [M,3] already normalised by inr_march_rays_patch_write
 * (normalise = 1), directions given as a per-sample ray id + the per-ray table of inr_sh_table_q
 * ([N,4,4]: row q holds SH components q, 4+q, 8+q, 12+q).  Same results, ~100 VALU instructions per tile less.
 * numerics, any combination of the two bits (opt-in, inference):
 *   - INR_NUMERICS_TABLE_F16 (NeRFNetwork.half_table): embeddings is the fp16 copy of the table (4 bytes per row: 512
 *     instead of 1024 algorithmic bytes per sample); index arithmetic and blending are unchanged;
 *   - INR_NUMERICS_MLP_F16 (NeRFNetwork.mlp_fp16): weights packed with INR_NUMERICS_MLP_F16.                       */
int inr_nerf_forward_table(const float* x01, const int32_t* ray_ids, const float* sh_table_q, int64_t M,
                           float bound, const void* embeddings, const inr_grid_desc* desc /*host*/,
                           const float* packed /*device*/, float density_scale, float* sigma, float* rgb,
                           int32_t numerics, inr_stream_t s);
/* Records feed of inr_nerf_forward_table (same results bit for bit, same numerics values, same launch shape): t [M] and
 * ray_ids [M] from inr_march_rays_patch_write_records, and the per-ray rows of inr_ray_table_q - [N] rows of
 * INR_RAY_TABLE_FLOATS floats, 16-byte aligned: the 16 values of inr_sh_table_q, then (o, 0) and (d, 0).  Every
 * lane forms x01 = (clamp(o + t d, -bound, bound) + bound) * (1 / (2 bound)) with the marcher's own operations; the
 * product equals the positions writer's division only where 2*bound is a power of two, and any other bound is refused
 * (INR_EINVAL: take the positions feed).  8 instead of 16 bytes are read per sample.
 * Launches with numerics 0 on a 16-level table whose levels 8..15 are all hashed run behind the pair front end
 * (k_nerf_fwd_pair: a wave encodes two consecutive tiles in one gather pass, two lanes per sample; same bits).
 * INR_FIELD_PAIR=0 in the process environment, read at every launch, selects the one-tile kernel for them too - a
 * switch for A/B measurements and tests, no export and no ABI change.
 * Where levels 0..3 of that table are all dense, the pair front end fetches their x-neighbour rows - adjacent on a dense
 * level - in one 16-byte load per yz corner (same bits).  INR_FIELD_COARSE=0 in the environment, read at every launch,
 * selects the 8-byte gathers for those launches too.  The debug counters below - plain data, not part of the function
 * ABI, not thread-safe - count the pair launches: [1] with the 16-byte loads, [0] without.                            */
extern int64_t inr_debug_field_coarse_launches[2];
#define INR_RAY_TABLE_FLOATS 24
int inr_ray_table_q(const float* rays_o /*[N,3]*/, const float* rays_d /*[N,3]*/, int64_t N, float* out, inr_stream_t s);
int inr_nerf_forward_table_records(const float* t, const int32_t* ray_ids, const float* ray_table_q, int64_t M,
                             float bound, const void* embeddings, const inr_grid_desc* desc /*host*/,
                             const float* packed /*device*/, float density_scale, float* sigma, float* rgb,
                             int32_t numerics, inr_stream_t s);
/* Sliced variant of inr_nerf_forward_table (round 5; same results bit for bit; fp32 table, 16 levels, hashed fine
 * levels): the three finest levels (13..15) are evaluated first, one level at a time over all samples - a hashed level
 * is 4 MiB, exactly one XCD's L2, and where those levels are finer than the spacing of a frame's samples nothing but a
 * cache that holds the whole level can serve their gathers (tools/micro/level_xcd_bench.hip: 259 against 69 G lines/s)
 * - into `fine_ws` (device, caller-owned, >= inr_nerf_forward_table_sliced_workspace_bytes(M) bytes: 24 bytes per
 * sample); the fused kernel then gathers the other thirteen levels.  Two launches on `s`.  Pays where the finest levels
 * have no locality at all (a scene filling a bound >= 4 volume: 30.2 -> 27.5 ms per 141 M samples); slower elsewhere -
 * NeRFNetwork.frame_slices = "auto" measures both paths and keeps the faster.                                          */
int64_t inr_nerf_forward_table_sliced_workspace_bytes(int64_t M);
int inr_nerf_forward_table_sliced(const float* x01, const int32_t* ray_ids, const float* sh_table_q, int64_t M,
                                  float bound, const float* embeddings, const inr_grid_desc* desc /*host*/,
                                  const float* packed /*device*/, float density_scale, float* sigma, float* rgb,
                                  float* fine_ws, inr_stream_t s);
/* Training path of the NeRF field (a9 under autograd): device-packed weights (forward layout of
 * inr_nerf_pack_weights + the transposed sections of the backward), a forward that also stores the activations
 * (enc [M,32], h1 [M,64], so [M,16] = raw sigma-net output, cin [M,32] = colour-net input with a zero pad column,
 * c1, c2 [M,64]) and ONE backward launch from (dL/dsigma [M], dL/drgb [M,3]) to
 * grad_o [M,4] (rgb logits, 3 live), grad_zc2, grad_zc1 [M,64], grad_so [M,16], grad_zh1 [M,64], grad_enc [M,32].
 * sigma here is exp(so[:,0]) (no density_scale); pass the scale the caller applies afterwards as density_scale = 1.
 * Weight gradients: inr_linear_wgrad(c2, grad_o), (c1, grad_zc2), (cin, grad_zc1), (h1, grad_so), (enc, grad_zh1). */
int64_t inr_nerf_bwd_packed_floats(void);
int inr_nerf_pack_weights_device(const float* sigma_w0, const float* sigma_w1, const float* color_w0,
                                 const float* color_w1, const float* color_w2, float* packed_fwd,
                                 float* packed_bwd, inr_stream_t s);
int inr_nerf_forward_train(const float* x, const float* d, int64_t M, float bound, const float* embeddings,
                           const inr_grid_desc* desc /*host*/, const float* packed_fwd, float* sigma, float* rgb,
                           float* enc, float* h1, float* so, float* cin, float* c1, float* c2, inr_stream_t s);
int inr_nerf_backward(const float* grad_sigma, const float* grad_rgb, const float* rgb, const float* so,
                      const float* h1, const float* c1, const float* c2, int64_t M, float density_scale,
                      const float* packed_bwd, float* grad_o, float* grad_zc2, float* grad_zc1, float* grad_so,
                      float* grad_zh1, float* grad_enc, inr_stream_t s);
/* The NeRF field of a training step in two launches per direction (round 3; the NeRF-stage twin of
 * inr_instance_forward_enc / inr_instance_head_backward).  Forward: as inr_nerf_forward_train but only the encoder
 * output [M,32] is kept.  Backward: ONE launch from (dL/dsigma [M], dL/drgb [M,3]) to dL/denc [M,32] and the five
 * weight gradients - grad_ws0 [64,32], grad_ws1 [16,64], grad_wc0 [64,31] (the colour net's 31 inputs, pitch 31), grad_wc1 [64,64],
 * grad_wc2 [16,64] (rows 0..2 live), written, not accumulated: the forward is recomputed from enc and the view
 * directions d [M,3] with packed_fwd, the input-gradient chain is inr_nerf_backward's, and the weight gradients are
 * accumulated on the fp32 matrix cores with the tiles transposed through LDS.  Replaces inr_nerf_backward and five
 * inr_linear_wgrad calls and the 1088 B per sample of saved activations.  workspace:
 * inr_instance_head_workspace_bytes() bytes.                                                                      */
int inr_nerf_forward_enc(const float* x, const float* d, int64_t M, float bound, const float* embeddings,
                         const inr_grid_desc* desc /*host*/, const float* packed_fwd, float* sigma, float* rgb,
                         float* enc, inr_stream_t s);
int inr_nerf_head_backward(const float* enc, const float* d, const float* grad_sigma, const float* grad_rgb, int64_t M,
                           float density_scale, const float* packed_fwd, const float* packed_bwd, float* grad_enc,
                           void* workspace, float* grad_ws0, float* grad_ws1, float* grad_wc0, float* grad_wc1,
                           float* grad_wc2, float* zero_buf /*nullable*/, int64_t zero_floats, inr_stream_t s);
/* Training path of the instance field (a13): weights are packed ON THE DEVICE every step (forward layout as
 * inr_instance_pack_weights, plus the transposed sections the input-gradient kernel uses); the forward also
 * stores the encoder output [M,32] and both hidden activations [M,64]; inr_instance_backward turns
 * dL/dlogits [M,K] into dL/dz2, dL/dz1 [M,64] (ReLU-masked) and dL/denc [M,32] in one launch.  Weight gradients
 * are inr_linear_wgrad(h2, dlogits), (h1, dz2), (enc, dz1); the table gradient is inr_grid_encode_backward(denc). */
int64_t inr_instance_bwd_packed_floats(void);
int inr_instance_pack_weights_device(const float* w0 /*[64,32]*/, const float* w1 /*[64,64]*/,
                                     const float* w2 /*[K,64]*/, int32_t K, float* packed_fwd, float* packed_bwd,
                                     inr_stream_t s);
int inr_instance_forward_train(const float* x, int64_t M, float bound, const float* embeddings,
                               const inr_grid_desc* desc /*host*/, const float* packed_fwd, int32_t K,
                               float* logits, float* enc, float* h1, float* h2, inr_stream_t s);
int inr_instance_backward(const float* grad_logits, int32_t K, const float* h1, const float* h2, int64_t M,
                          const float* packed_bwd, float* grad_z2, float* grad_z1, float* grad_enc,
                          inr_stream_t s);
/* The instance head of the instance stage in two launches per direction (round 3).  Forward: as
 * inr_instance_forward_train, but only the encoder output [M,32] is kept (n_samples_dev, nullable: device int32 with
 * the number of live rows; rows beyond it are not evaluated).  Backward: ONE launch from dL/d(rendered logits)
 * grad_pix [N,K] to dL/denc [M,32] (zero for rows >= *n_samples_dev) and the three weight gradients
 * grad_w0 [64,32], grad_w1 [64,64], grad_w2 [K,64] (written, not accumulated): per sample g = weights[m] *
 * grad_pix[sample_ray[m]] (the K-channel compositing backward, weights detached), the hidden layers are recomputed
 * from enc with packed_fwd, the input-gradient chain uses packed_bwd, and dW += g^T h on the fp32 matrix cores with
 * the tiles transposed through LDS - replaces inr_composite_rays_train_backward (K channels), inr_instance_backward
 * and three inr_linear_wgrad calls, and ~3 KB of HBM traffic per sample.  scale_a, scale_b: device scalars that
 * multiply grad_pix (1 / kept rows and dL/dloss of the fused cross entropy; NULL = 1).  zero_buf (nullable): zero_floats
 * floats that the launch zero-fills on the side - the table-gradient buffer of the scatter that follows.  workspace:
 * inr_instance_head_workspace_bytes() bytes.  The table gradient stays inr_grid_encode_backward(grad_enc).      */
int inr_instance_forward_enc(const float* x, int64_t M, const int32_t* n_samples_dev, float bound,
                             const float* embeddings, const inr_grid_desc* desc /*host*/, const float* packed_fwd,
                             int32_t K, float* logits, float* enc, inr_stream_t s);
int64_t inr_instance_head_workspace_bytes(void);
int inr_instance_head_backward(const float* enc, const float* weights, const int32_t* sample_ray,
                               const float* grad_pix, int32_t K, int64_t N, int64_t M, const int32_t* n_samples_dev,
                               const float* scale_a /*device scalar, nullable*/, const float* scale_b /*same*/,
                               const float* packed_fwd, const float* packed_bwd, float* grad_enc, void* workspace,
                               float* grad_w0, float* grad_w1, float* grad_w2, float* zero_buf /*nullable*/,
                               int64_t zero_floats, inr_stream_t s);
/* rgb-sigma lattice extraction (the step after the path that feeds NeRF-RCNN: /root/reference/nerf_rcnn/datasets.py:766-792
 * reads the result): out[m] = (mean over n_dirs fixed view directions of rgb(x_m, dir), raw density logit of x_m) -
 * one gather + one sigma-net pass per point, the colour net once per direction.  sh_dirs [n_dirs,16] = degree-4 SH rows
 * of the directions (inr_sh_encode_forward), n_dirs <= 8; out float [M,4], 16-byte aligned.                            */
int inr_nerf_forward_dirs(const float* x, int64_t M, float bound, const float* embeddings, const inr_grid_desc* desc /*host*/,
                          const float* packed /*device*/, const float* sh_dirs, int32_t n_dirs, float* out, inr_stream_t s);
/* The same for a [W, L, H] lattice given by its coordinate axes (x = ax_w[iw], y = ax_l[il], z = ax_h[ih], clamped to
 * [-bound, bound]; the rgb-sigma extraction of SURVEY f1 / BASELINE configs[4]): no point tensor, and the kernel walks the
 * lattice in runs of 16 along W - the table's fastest row index - instead of the writer's h-fastest order (2.4x faster:
 * the kernel is gather-bound).  logit_min: lower clamp of the density logit (channel 3; the writer uses log(1e-30),
 * -INFINITY for none).  out float [W, L, H, 4], 16-byte aligned.                                                        */
int inr_nerf_forward_lattice(const float* ax_w, const float* ax_l, const float* ax_h, int32_t W, int32_t L, int32_t H,
                             float bound, const float* embeddings, const inr_grid_desc* desc /*host*/,
                             const float* packed /*device*/, const float* sh_dirs, int32_t n_dirs, float logit_min,
                             float* out, inr_stream_t s);
int inr_instance_forward(const float* x, int64_t M, const int32_t* n_samples_dev, float bound,
                         const float* embeddings, const inr_grid_desc* desc /*host*/,
                         const float* packed /*device*/, int32_t K, float* logits /*[M,K]*/,
                         inr_stream_t s);
/* 3-D instance masks of a trained instance field (the field's own segmentation, in the voxel layout NeRF-RCNN's masks use).
 * One launch over the [W, L, H] lattice of inr_nerf_forward_lattice (same axes, same walk, coordinates clamped to
 * [-bound, bound]): the NeRF's density logit (gather + the two sigma-net layers; nerf_packed = inr_nerf_pack_weights'
 * buffer) gives sigma = exp(logit) * density_scale, and a voxel is occupied when sigma >= sigma_thresh.  Runs of 16
 * voxels along W without an occupied voxel skip the instance field; elsewhere the instance MLP (inst_packed =
 * inr_instance_pack_weights' buffer for K_pad = 16 * ceil(K / 16) rows, K = 1..64 real channels) is reduced on chip:
 *   labels     uint8 [W, L, H]: arg-max over channels 0..K-1 (lowest channel on ties), 255 = unoccupied;
 *   confidence float [W, L, H]: max-softmax over the K channels, 0 where unoccupied (4-byte aligned);
 *   density_logit float [W, L, H] (nullable, 4-byte aligned): the raw density logit of every voxel.
 * Padded channels K..K_pad-1 never win.  Tables below 2 GiB each; sigma_thresh / density_scale not NaN.             */
int inr_instance_lattice(const float* ax_w, const float* ax_l, const float* ax_h, int32_t W, int32_t L, int32_t H,
                         float bound, const float* nerf_embeddings, const inr_grid_desc* nerf_desc /*host*/,
                         const float* nerf_packed /*device*/, float density_scale, float sigma_thresh,
                         const float* inst_embeddings, const inr_grid_desc* inst_desc /*host*/,
                         const float* inst_packed /*device*/, int32_t K, uint8_t* labels, float* confidence,
                         float* density_logit, inr_stream_t s);
/* Per-channel statistics of such a label volume (labels uint8 [W, L, H], values >= K ignored): counts int32 [K],
 * boxes int32 [K, 6] = inclusive voxel-index bounds (min iw, il, ih, max iw, il, ih; all -1 for an empty channel),
 * conf_sum float [K] = sum of the channel's confidences.  Bit-reproducible: per-workgroup partials in fixed slots of
 * `workspace` (device, >= INR_INSTANCE_STATS_WORKSPACE_BYTES, 4-byte aligned) and a fixed-order final pass, no float
 * atomics.  Two launches on `s`.                                                                                    */
#define INR_INSTANCE_STATS_WORKSPACE_BYTES (512 * 64 * 8 * 4)
int inr_instance_volume_stats(const uint8_t* labels, const float* confidence, int32_t W, int32_t L, int32_t H, int32_t K,
                              void* workspace, int64_t workspace_bytes, int32_t* counts, int32_t* boxes, float* conf_sum,
                              inr_stream_t s);

/* ---- iso-surface meshes of a lattice field (no counterpart in the reference tree: upstream's Trainer.save_mesh runs
 * marching cubes on the host).  MARCHING TETRAHEDRA over the Kuhn split of every lattice cell: translation-invariant, so
 * neighbouring cells agree on every face diagonal and the surface is closed and edge-manifold for any field.
 *
 * Field: `field` float [W, L, H] read with an element stride (`field_stride` = 4 reads channel 3 of an rgbsigma
 * [W, L, H, 4] volume in place when `field` points at that channel).  A lattice point is INSIDE when field >= iso (NaN:
 * outside) and, with select >= 0, labels == select (labels uint8 [W, L, H], nullable when select = -1; select -1..254).
 * For interpolation a value is clamped to [iso - clamp, iso + clamp]; NaN and masked-out points take iso - clamp.
 * clamp > 0 and finite, iso - clamp < iso in fp32.
 *
 * cap = 1 surrounds the lattice with one layer of virtual outside points (value iso - clamp), so a surface that reaches
 * the border is closed; the extended lattice is [W+2, L+2, H+2] and a virtual point's coordinate continues the first /
 * last step of its axis (ax[0] - (ax[1] - ax[0]), ax[n-1] + (ax[n-1] - ax[n-2]); for an axis of length 1: ax[0] -/+ the
 * `ext_*` argument of that axis).  cap = 0 visits the (W-1)(L-1)(H-1) real cells only.
 *
 * Tables.  Cube corner code c = 4 dw + 2 dl + dh.  A cell is split into six tetrahedra, one per order in which the axes
 * are added on the way from corner 0 to corner 7; tetrahedron t has the corners (tetrahedron vertices 0..3)
 *   t0 wlh: 0 4 6 7   t1 whl: 0 4 5 7   t2 lwh: 0 2 6 7   t3 lhw: 0 2 3 7   t4 hwl: 0 1 5 7   t5 hlw: 0 1 3 7
 * Every tetrahedron edge runs from a lattice point p to p + d, d = (dw, dl, dh) != 0; p OWNS the edge, and the 7
 * directions are ordered by their code 4 dw + 2 dl + dh = 1..7: (0,0,1) (0,1,0) (0,1,1) (1,0,0) (1,0,1) (1,1,0) (1,1,1).
 * Tetrahedron edges by their two tetrahedron vertices: e0 = 01, e1 = 02, e2 = 03, e3 = 12, e4 = 13, e5 = 23.  Case m =
 * sum of 2^i over the inside tetrahedron vertices i; triangles as edge triples:
 *    1: e0 e1 e2            2: e0 e4 e3            3: e1 e2 e4, e1 e4 e3   4: e1 e3 e5            5: e0 e5 e2, e0 e3 e5
 *    6: e0 e4 e5, e0 e5 e1  7: e2 e4 e5            8: e2 e5 e4            9: e0 e1 e5, e0 e5 e4  10: e0 e5 e3, e0 e2 e5
 *   11: e1 e5 e3           12: e1 e3 e4, e1 e4 e2 13: e0 e3 e4           14: e0 e2 e1            0, 15: none
 * The triples are wound for t0, t3, t4 (even axis permutations); t1, t2, t5 are mirror images and swap the second and
 * third vertex of every triangle.  Normals then point from inside to outside: a closed surface has positive volume.
 *
 * A crossed edge p -> q = p + d (exactly one end inside) gets ONE vertex, in fp32 and in this order of operations (the
 * library is built without contraction and with IEEE division): a, b = clamped values at p, q; t = (iso - a) / (b - a);
 * x = xp + t * (xq - xp) per axis; colour (rgb float [W, L, H, 4], channels 0..2, nullable together with `colors`)
 * cp + t * (cq - cp), a virtual end taking the real end's colour.
 *
 * Canonical order, decided by scans (no atomics: two calls give identical bits).  Points and cells are walked in
 * (w, l, h) order of the (extended) lattice, h fastest.  Vertices: by owner point, then by direction code.  Triangles: by
 * cell (named by its corner 0), then tetrahedron 0..5, then the table's order.  face_labels (uint8 [F], nullable, needs
 * `labels`): the label of the tetrahedron's inside vertex with the largest clamped value, the lowest tetrahedron vertex on
 * ties (it may be 255 where the label volume and the field disagree about occupancy).
 *
 * inr_mesh_workspace_bytes: size of the caller-owned workspace (4-byte aligned); INR_EINVAL for sizes < 1, cap not 0 / 1,
 * or a lattice whose 12 * (extended) points do not fit an int32.  inr_mesh_count: three launches on `s` (classify, scan,
 * vertex offsets); fills the workspace and writes counts int32 [2] = (V, F) on the device.  inr_mesh_emit: with the SAME
 * field arguments and the workspace inr_mesh_count filled (read-only here), V and F as read back by the caller (rows
 * beyond them are never written): vertices float [V, 3], faces int32 [F, 3], colors float [V, 3], face_labels; two
 * launches on `s`, none when V = F = 0.  All buffers 4-byte aligned.                                                  */
int64_t inr_mesh_workspace_bytes(int32_t W, int32_t L, int32_t H, int32_t cap);
int inr_mesh_count(const float* field, int32_t field_stride, float iso, float clamp, const uint8_t* labels /*nullable*/,
                   int32_t select, int32_t W, int32_t L, int32_t H, int32_t cap, void* workspace, int64_t workspace_bytes,
                   int32_t* counts, inr_stream_t s);
int inr_mesh_emit(const float* field, int32_t field_stride, float iso, float clamp, const uint8_t* labels /*nullable*/,
                  int32_t select, const float* rgb /*nullable*/, const float* ax_w, const float* ax_l, const float* ax_h,
                  int32_t W, int32_t L, int32_t H, float ext_w, float ext_l, float ext_h, int32_t cap,
                  const void* workspace, int64_t workspace_bytes, int32_t V, int32_t F, float* vertices, int32_t* faces,
                  float* colors /*nullable*/, uint8_t* face_labels /*nullable*/, inr_stream_t s);

/* ---- connected components of a label volume (no counterpart in the reference tree; drops floaters from the masks and
 * meshes above).  Input: `labels` uint8 [W, L, H], h fastest, 255 = empty, as inr_instance_lattice writes it.  The
 * linear index of voxel (iw, il, ih) is (iw * L + il) * H + ih; W * L * H must be below 2^31.
 *
 * Two voxels are CONNECTED when they are neighbours and carry the same label != 255; a component is a class of the
 * transitive closure.  Neighbours: connectivity = 6, the face neighbours (exactly one of |dw|, |dl|, |dh| is 1, the
 * others 0); connectivity = 26, every (dw, dl, dh) in {-1, 0, 1}^3 except (0, 0, 0).  Any other value: INR_EINVAL.  The
 * volume does not wrap around.  A component is named by its ROOT: the smallest linear index among its voxels.
 *   roots int32 [W, L, H]: the root of the voxel's component, -1 for an empty voxel (4-byte aligned).
 * The definition does not depend on a traversal order, and the output is bit-identical between calls although the
 * kernels use integer atomics (min on parents, add on sizes: both order-independent).
 *
 * Keep rule (inr_components_filter), for every channel c in first_channel..K-1 (K = 1..255, first_channel = 0..K): the
 * SIZE of a component is its number of voxels; a component of label c SURVIVES when size >= min_voxels (>= 1) and, with
 * keep_largest = 1, it is also the largest component of label c - among components of equal size the one with the
 * lowest root (so at most one survives per channel).  keep_largest is 0 or 1.
 *   labels_out uint8 [W, L, H]: the label where the voxel's component survives, 255 where it does not.  Labels below
 *     first_channel or >= K (255 included) are copied through unchanged.  May alias `labels`.
 *   confidence_out float [W, L, H] (nullable; needs `confidence`; may alias it): confidence where the output label
 *     equals the input label, 0 where the voxel was dropped.
 *   n_components int32 [K]: components of label c before the rule; kept_voxels int32 [K]: voxels of label c in
 *     surviving components; kept_root int32 [K]: with keep_largest = 1 the root of the survivor, -1 when none;
 *     always -1 with keep_largest = 0.  Channels below first_channel report 0, 0, -1.
 * Feed labels_out to inr_instance_volume_stats for counts, boxes and confidence sums of what was kept.
 *
 * inr_components_workspace_bytes: size of the caller-owned workspace (8-byte aligned); INR_EINVAL for sizes < 1 or
 * W * L * H >= 2^31.  inr_components_label additionally needs ceil(W / 8) * ceil(L / 8) * ceil(H / 64) <= 2^23 tiles (one
 * workgroup each; only a volume far thinner than a tile in two axes, such as 1 x 1 x 2^30, comes near) and returns
 * INR_EINVAL beyond.  inr_components_label: three launches on `s` - one workgroup per 8 x 8 x 64 tile labels it in LDS,
 * one pass unites across tile faces, one pass compresses every voxel to its root and counts component sizes into the
 * workspace.  inr_components_filter: with the SAME labels, the roots and the workspace inr_components_label filled
 * (sizes are read, the per-channel scratch behind them is written); four launches on `s`.                           */
int64_t inr_components_workspace_bytes(int32_t W, int32_t L, int32_t H);
int inr_components_label(const uint8_t* labels, int32_t W, int32_t L, int32_t H, int32_t connectivity, void* workspace,
                         int64_t workspace_bytes, int32_t* roots, inr_stream_t s);
int inr_components_filter(const uint8_t* labels, const int32_t* roots, const float* confidence /*nullable*/, int32_t W,
                          int32_t L, int32_t H, int32_t K, int32_t first_channel, int32_t min_voxels, int32_t keep_largest,
                          void* workspace, int64_t workspace_bytes, uint8_t* labels_out, float* confidence_out /*nullable*/,
                          int32_t* n_components, int32_t* kept_voxels, int32_t* kept_root, inr_stream_t s);

/* ---- 2-D mask matching (replaces the reference's CPU script Mask2Former_sample/match_seg.py:94-150, the step between
 * the 3-D mask projector and the instance stage).  Additive: no version bump.  B views of P = H * W pixels, k candidate
 * masks in CANDIDATE ORDER (the reference's sorted-file-name order of "<img>_<id>.png"; the caller orders them), nw =
 * ceil(k / 32) words per pixel: bit j % 32 of words[b][j / 32][p] = candidate j covers pixel p of view b.
 *
 * The rule, per view: seg holds -1 (unlabeled), 0 (background) or the RANK 1..S of a segment (dense per view; the
 * caller ranks the segment ids).  For rank r with area_r = |seg == r| > 0 and every candidate j,
 *   iou[j] = inter / (area_r + area_j - inter),  inter = |seg == r & m_j|,  area_j = |m_j|,
 * the counts combined in integers and divided in fp64 (IEEE division: the bits of numpy's np.sum(..) / np.sum(..)).
 * j* = the FIRST maximum.  The rank is assigned instance_ids[j*] if iou[j*] > iou_thresh (fp64 comparison), else -1;
 * with k = 0 or area_r = 0 it is assigned -1.  Pixels <= 0 pass through.
 *
 * inr_pack_mask_bits: words uint32 [nw, P] of ONE view from the projector's soft sums: clears `words`, then sets bit
 *   j % 32 of words[j / 32][inds[n]] where soft[n][j] > thresh (NaN: false).  soft float [N, k]; inds int64 [N]
 *   (nullable = identity) are DISTINCT pixel indices by the caller's contract; one outside [0, P) is skipped.
 *   1 <= k <= 1024, 0 <= N, 1 <= P, both below 2^31.  One fill and one launch.
 * inr_match_count: zeroes its outputs, then counts.  seg int32 [B, P]; words uint32 [B, nw, P] (bits at and above k are
 *   ignored);  seg_area int32 [B, S + 1]: pixels per rank, [b][0] = pixels with seg <= 0;  mask_area int32 [B, k];
 *   inter int32 [B, S + 1, k], row 0 = the candidate's pixels outside every segment.  A seg value outside [-1, S] is
 *   counted nowhere and sets status[0] (int32 [1]) to non-zero; otherwise status[0] = 0.  words, mask_area and inter may
 *   be null when k = 0.  Limits: 1 <= B, 1 <= P, B * P < 2^31, 0 <= S <= 1023, 0 <= k <= 1024; INR_EINVAL beyond.
 *   Three launches: zero, count (all views and words in one launch; the (S + 1) x 32 counters of a word live in LDS,
 *   lanes of a wave that hold the same (rank, word) pair are counted once), column sums.
 * inr_match_assign: with the SAME seg and the counts inr_match_count wrote: assigned int32 [B, S + 1] per the rule
 *   ([b][0] = 0, unused), then out int32 [B, P] = -1, 0 or assigned[b][seg[p]] (-1 for a value outside [-1, S]).
 *   iou_thresh: HOST pointer to one double in [0, 1], read before the call returns.  Two launches.
 * Integer atomics only: two calls give identical bits.                                                             */
int inr_pack_mask_bits(const float* soft, const int64_t* inds /*nullable*/, int64_t N, int32_t k, float thresh, int64_t P,
                       uint32_t* words, inr_stream_t s);
int inr_match_count(const int32_t* seg, const uint32_t* words, int64_t B, int64_t P, int32_t S, int32_t k,
                    int32_t* seg_area, int32_t* mask_area, int32_t* inter, int32_t* status, inr_stream_t s);
int inr_match_assign(const int32_t* seg, const int32_t* seg_area, const int32_t* mask_area, const int32_t* inter,
                     const int32_t* instance_ids, int64_t B, int64_t P, int32_t S, int32_t k,
                     const double* iou_thresh /*host*/, int32_t* assigned, int32_t* out, inr_stream_t s);

/* ---- 3-D mask overlap (the counts behind the reference's mask_iou_3d, model/utils.py:786-802, which repeats both mask
 * sets to [N, M, W, L, H]; instance_nerf_amd/evaluate.py turns them into IoU, AP and recall).  Additive: no version
 * bump.  A mask over V = W * L * H voxels is a BIT PLANE: nW = ceil(V / 64) words, bit v % 64 of word v / 64 = the mask
 * holds flattened voxel v; the bits of the last word at and above V are zero.  planes uint64 [k, nW].
 *
 * inr_pack_mask_planes: masks uint8 (or bool) [k, V], non-zero = inside -> planes [k, nW] and area int32 [k] = voxels
 *   per mask (zeroed by the call).  One fill and one launch; k = 0 launches nothing (pointers may be null).
 * inr_pack_label_planes: labels uint8 [V] as extract_instances returns them -> planes [K - first_channel, nW], plane i =
 *   (label == first_channel + i), and area int32 [K - first_channel].  A label >= K (the 255 of an empty voxel when
 *   K < 256) lands in no plane.  One fill and one launch; first_channel = K launches nothing.
 * inr_mask_overlap: inter int32 [kA, kB] = |A_a & B_b| (zeroed by the call) from two plane sets over the same V.
 *   run_words: words per workgroup, a multiple of 256, or 0 = the library's choice (at least 1024 while the volume has
 *   them).  One fill and one launch; kA = 0 or kB = 0 launches nothing.
 * Limits: 1 <= V < 2^31, 0 <= k, kA, kB <= 1024, 1 <= K <= 256, 0 <= first_channel <= K; INR_EINVAL beyond.
 * Integer atomics only: two calls give identical bits.                                                              */
int inr_pack_mask_planes(const uint8_t* masks, int32_t k, int64_t V, uint64_t* planes, int32_t* area, inr_stream_t s);
int inr_pack_label_planes(const uint8_t* labels, int64_t V, int32_t K, int32_t first_channel, uint64_t* planes,
                          int32_t* area, inr_stream_t s);
int inr_mask_overlap(const uint64_t* planes_a, int32_t kA, const uint64_t* planes_b, int32_t kB, int64_t V,
                     int32_t run_words, int32_t* inter, inr_stream_t s);

/* ---- Detector tail (what the reference runs between its detector heads and masks/<scene>.npz: per-class 3-D NMS,
 * model/utils.py:217-267, and paste_masks_in_image, model/utils.py:646-782).  Additive: no version bump.
 *
 * inr_paste_masks: probs [N, M, M, M] mask probabilities, boxes [N, 6] = (x1, y1, z1, x2, y2, z2) in grid units (they
 *   may leave the grid) -> planes uint64 [N, nW] in the bit-plane layout above over V = W * L * H voxels (flattened
 *   (w, l, h), H fastest; tail bits zero) and area int32 [N] = set bits per mask (zeroed by the call).  Bit = acc >= thresh
 *   with acc the reference's whole-volume resampling (_do_paste_mask(skip_empty=False): the path its GPU runs take), per
 *   voxel index (i, j, k), all in fp32, every operation rounded on its own (no fused multiply-add), IEEE division:
 *     g = (float(i) - x1) / (x2 - x1) * 2 - 1;  p = ((g + 1) / 2) * (M - 1)           (grid_sample, align_corners=True)
 *   likewise for j with (y1, y2) and k with (z1, z2); p0 = floor(p), p1 = p0 + 1; eight taps added to 0.0f in the order
 *   (w0,l0,h0) (w0,l0,h1) (w0,l1,h0) (w0,l1,h1) (w1,l0,h0) (w1,l0,h1) (w1,l1,h0) (w1,l1,h1), tap weight = (fh * fl) * fw
 *   with f = p1 - p on the 0 side and p - p0 on the 1 side, acc = acc + value * weight; a tap with an index outside
 *   [0, M) on any axis adds nothing (zeros padding).  tests/paste_reference.py is this paragraph in numpy.
 *   DEPARTURE: a box with a non-finite coordinate or a side <= 0 gives an empty mask (the reference divides by zero; its
 *   own pipeline drops sides < 1e-2 before this point).
 *   soft (nullable): fp32 [N, V], acc itself - for tests.  A workgroup (256 words) whose voxels all lie outside the mask's
 *   support along W - the box widened by one texel (x2 - x1) / (M - 1) on each side - stores zeros without sampling; the
 *   test evaluates p at the run's first and last w with the arithmetic above, which is monotone in the index, so it
 *   never drops a set bit.  One fill and one launch; N = 0 launches nothing (pointers may be null).
 *   Limits: 0 <= N <= 1024, 1 <= M <= 1024, W, L, H >= 1, V < 2^31, thresh >= 0; INR_EINVAL beyond.
 * inr_planes_to_voxel_words: planes [k, nW] -> words int32 [V] in the layout inr_project_masks_patch reads: bit i of
 *   words[v] = bit v of plane base + i, i < min(32, k - base); the other bits zero.  1 <= k <= 1024, 0 <= base < k.
 *   One launch.
 * inr_nms_3d_pairs: boxes [n, 6] ALREADY SORTED by decreasing score, classes int32 [n] -> pairs uint64 [n, ceil(n / 64)]:
 *   bit j % 64 of pairs[i][j / 64] = j > i, classes[i] == classes[j] and !(iou(i, j) <= iou_thresh) - the reference's
 *   survival test `iou <= iou_threshold` (model/utils.py:230) negated, so a NaN IoU suppresses.  IoU = the axis-aligned
 *   form of model/utils.py:391-462 in fp32 without contraction: volume = ((x2 - x1) * (y2 - y1)) * (z2 - z1), overlap =
 *   (ex * ey) * ez of the extents min(hi) - max(lo) clamped at 0 (a NaN operand stays NaN), iou = overlap /
 *   ((volume_i + volume_j) - overlap).  Every word of the matrix is written.  0 <= n <= 4096.  One launch.
 * inr_nms_3d_scan: the greedy walk over that matrix in ONE workgroup: row i survives unless a surviving row before it
 *   holds its bit.  keep int32 [n]: the surviving rows in ascending order (= decreasing score) in keep[0 .. n_keep[0]);
 *   n_keep int32 [1] on the device.  n = 0 writes n_keep = 0 (pairs and keep may be null).  One launch.
 *   Together the two equal the reference's per-class greedy loop followed by its sort by score, for distinct scores.   */
int inr_paste_masks(const float* probs, const float* boxes, int32_t N, int32_t M, int32_t W, int32_t L, int32_t H,
                    float thresh, uint64_t* planes, int32_t* area, float* soft /*nullable*/, inr_stream_t s);
int inr_planes_to_voxel_words(const uint64_t* planes, int32_t k, int64_t V, int32_t base, int32_t* words, inr_stream_t s);
int inr_nms_3d_pairs(const float* boxes, const int32_t* classes, int32_t n, float iou_thresh, uint64_t* pairs,
                     inr_stream_t s);
int inr_nms_3d_scan(const uint64_t* pairs, int32_t n, int32_t* keep, int32_t* n_keep, inr_stream_t s);

/* ---- 3-D RoIAlign ("next" row f2; replaces roi_align.roi_align.roi_align_3d, the one FFI call in the
 * reference tree: /root/reference/nerf_rcnn/model/utils.py:604-609).  torchvision roi_align semantics
 * (aligned=False, adaptive ceil(roi/out) sampling grid, average) on three axes: x<->W, y<->L, z<->H.
 * input [N,C,W,L,H], rois [K,6] = (x1,y1,z1,x2,y2,z2) in input-scale units, roi_inds int32 [K],
 * out [K,C,out_w,out_l,out_h].  backward ACCUMULATES into grad_input (caller zeroes it).          */
/* No reference counterpart.  Which kernels the two calls below use: 0 (default) the separable ones (per-axis weight
 * tables built once per RoI in LDS, z -> y -> x contraction, 4 channels per lane) whenever the tables fit the LDS
 * window, 1 one lane per output element (the torchvision kernel shape; also the fallback), 2 separable or INR_EINVAL,
 * 3 separable without the workspace form of the backward (below).
 * Same sample geometry in both; sums differ by fp32 rounding.  Process-wide.                                        */
int inr_roi_align_3d_set_mode(int32_t mode);
int inr_roi_align_3d_forward(const float* input, const float* rois, const int32_t* roi_inds, int32_t N,
                             int32_t C, int32_t W, int32_t L, int32_t H, int64_t K, int32_t out_w,
                             int32_t out_l, int32_t out_h, float spatial_scale, float* out, inr_stream_t s);
int inr_roi_align_3d_backward(const float* grad_out, const float* rois, const int32_t* roi_inds, int32_t N,
                              int32_t C, int32_t W, int32_t L, int32_t H, int64_t K, int32_t out_w,
                              int32_t out_l, int32_t out_h, float spatial_scale, float* grad_input,
                              inr_stream_t s);

/* No reference counterpart.  The backward with a caller-owned workspace: the separable backward is bound by the
 * memory-side atomic unit (requests of up to 64 bytes, ~21 G/s whatever they carry), and a region row of the gradient's
 * own layout fills a request with ~6 floats.  This form accumulates into a channels-fastest scratch volume
 * (workspace: N*C*W*L*H floats, zeroed by the call) - one full 64-byte request per voxel and 16 channels - and writes
 * grad_input with a transposing copy: grad_input is OVERWRITTEN (no zero fill by the caller, no accumulation).
 * _workspace_bytes returns 0 where the form does not apply (C not a multiple of 16, out_l*out_h > 256, tables beyond
 * the LDS window, modes 1 and 3 of inr_roi_align_3d_set_mode): the caller then uses inr_roi_align_3d_backward.
 * Mode 3 (added with it) = separable kernels, accumulation in place (the round-4 form) - for A/B tests.             */
int64_t inr_roi_align_3d_backward_workspace_bytes(int32_t N, int32_t C, int32_t W, int32_t L, int32_t H, int64_t K,
                                                  int32_t out_w, int32_t out_l, int32_t out_h);
/* Which backward a caller should take (cost model, round 6): 1 = the workspace form is available AND expected to be
 * faster - it trades fuller atomic requests (16 channels of a voxel instead of ~6 floats of a row) for three extra passes
 * over the N*C*V volume and a per-RoI set-up that its 16-channel groups amortise worse; linear time models of both forms
 * fitted to 28 measured shapes (profiles/r06_roialign_bwd_shapes.txt).  covered_voxels: voxels inside the RoIs' regions,
 * summed over the RoIs, if known; < 0 = unknown (the lower bound K * min(bins, V) is then used, which biases towards the
 * in-place form; mode 2 of inr_roi_align_3d_set_mode answers 1 wherever the form exists).  Pure host arithmetic.    */
int inr_roi_align_3d_backward_prefers_workspace(int32_t N, int32_t C, int32_t W, int32_t L, int32_t H, int64_t K,
                                                int32_t out_w, int32_t out_l, int32_t out_h, int64_t covered_voxels);
int inr_roi_align_3d_backward_ws(const float* grad_out, const float* rois, const int32_t* roi_inds, int32_t N,
                                 int32_t C, int32_t W, int32_t L, int32_t H, int64_t K, int32_t out_w,
                                 int32_t out_l, int32_t out_h, float spatial_scale, float* grad_input,
                                 void* workspace, int64_t workspace_bytes, inr_stream_t s);

/* No reference counterpart as a native call: the reference's MultiScaleRoIAlign3D
 * (/root/reference/nerf_rcnn/model/poolers.py:115-188) pools from a feature pyramid with one roi_align_3d call per level
 * between host-synchronising index operations.  The pyramid form does it in ONE launch: every RoI names its level,
 * roi_levels int32 [K] (device), and row k of out [K,C,out_w,out_l,out_h] is RoI k whatever its level.  The level table
 * arrives as plain HOST arrays - level_ptrs [n_levels] device pointers of the volumes [N,C,W,L,H] (the same N and C on
 * every level), level_dims int32 [n_levels*3] = (W, L, H) per level, level_scales [n_levels] - and travels in the kernel
 * arguments: nothing is copied to the device or read back.  1 <= n_levels <= INR_ROI_MAX_LEVELS.  order int32 [K]
 * (device, nullable): the RoI that the i-th workgroup slot handles, a permutation of 0..K-1 - pass the stable argsort of
 * roi_levels, so that the workgroups resident at one time read one level (an entry outside [0, K) is ignored; the
 * lane-per-output kernels do not use it).  A RoI whose level is outside [0, n_levels) gives a row of zeros in the
 * forward and adds nothing in the backward.  Same arithmetic as inr_roi_align_3d_forward / _backward on the RoI's level:
 * the forward's rows carry the same bits.  Kernels (inr_roi_align_3d_set_mode): the separable ones if EVERY level fits
 * them, else one lane per output element; mode 2: INR_EINVAL naming the level that does not fit.
 * backward: level_grads [n_levels] are the grad_input volumes, ACCUMULATED into (the caller zeroes them); a null entry
 * = that level needs no gradient, its RoIs are skipped.  Always the in-place form (no workspace variant).
 * K == 0: INR_OK, nothing launched.  Limits: N, K >= 0, C, out_* >= 1, K*C*out_w*out_l*out_h < 2^39; INR_EINVAL beyond. */
#define INR_ROI_MAX_LEVELS 8
int inr_roi_align_3d_pyramid_forward(const float* const* level_ptrs /*host*/, const int32_t* level_dims /*host*/,
                                     const float* level_scales /*host*/, int32_t n_levels, const float* rois,
                                     const int32_t* roi_inds, const int32_t* roi_levels, const int32_t* order /*nullable*/,
                                     int32_t N, int32_t C, int64_t K, int32_t out_w, int32_t out_l, int32_t out_h,
                                     float* out, inr_stream_t s);
int inr_roi_align_3d_pyramid_backward(float* const* level_grads /*host*/, const int32_t* level_dims /*host*/,
                                      const float* level_scales /*host*/, int32_t n_levels, const float* rois,
                                      const int32_t* roi_inds, const int32_t* roi_levels, const int32_t* order /*nullable*/,
                                      int32_t N, int32_t C, int64_t K, int32_t out_w, int32_t out_l, int32_t out_h,
                                      const float* grad_out, inr_stream_t s);

/* Whole-ray rendering with early termination (inference, patch-interleaved layout): field evaluation and alpha
 * compositing in one launch; a 16-ray group stops being evaluated once all its rays are below T_thresh (what the
 * alive-ray loop of NeRFRenderer.run_cuda achieves, a5, without host round trips).  Same results as
 * inr_nerf_forward + inr_composite_rays_patch_forward up to fp32 rounding.  weights [M] nullable (w per sample,
 * 0 when skipped); evaluated: device uint64 [33], ZEROED BY THE CALLER - [0] receives the number of samples evaluated,
 * [1..32] are the cursors of the launch's dynamic group schedule (scratch).  numerics:
 *   - 0: fp32 table;
 *   - INR_NUMERICS_TABLE_F16 | INR_NUMERICS_MLP_F16 (upstream's `-O`, NeRFNetwork.half_table + mlp_fp16): fp16
 *     table, weights packed with INR_NUMERICS_MLP_F16.                                                              */
int inr_nerf_render(const float* xyzs, const float* deltas, const int32_t* rays, const float* rays_d /*[N,3]*/,
                    int64_t N, int64_t M, float bound, const void* embeddings, const inr_grid_desc* desc /*host*/,
                    const float* packed /*device*/, float density_scale, float T_thresh, float* weights_sum,
                    float* depth, float* image, float* weights, uint64_t* evaluated, int32_t x_is_01 /* xyzs are the
                    normalised coordinates of the patch writer's table feed */, int32_t numerics, inr_stream_t s);

/* Instance logits rendered in place (inference, patch-interleaved layout): extra_out[ray][ch] =
 * sum_k weights[slot(ray,k)] * logits(xyzs[slot(ray,k)])[ch]; the [M,K] logits never exist in memory.
 * xyzs/weights [M] in the patch-interleaved layout (inr_march_rays_patch_write / the weights output of
 * inr_composite_rays_patch_forward), rays [N,3] from the count pass, extra_out [N,K].  x_is_01 != 0: xyzs holds
 * the normalised coordinates (x + bound) / (2 bound) the patch writer emits with normalise = 1.  numerics:
 *   - 0: fp32 table;
 *   - INR_NUMERICS_TABLE_F16 | INR_NUMERICS_MLP_F16 (upstream's `-O`, NeRFNetwork.half_table + mlp_fp16): fp16 copy
 *     of the instance table, weights packed with INR_NUMERICS_MLP_F16.                                            */
int inr_instance_render(const float* xyzs, const int32_t* rays, const float* weights, int64_t N, int64_t M,
                        float bound, const void* embeddings, const inr_grid_desc* desc /*host*/,
                        const float* packed /*device*/, int32_t K, float* extra_out, int32_t x_is_01,
                        uint64_t* cursors /*device [32], ZEROED BY THE CALLER: the launch's dynamic group schedule*/,
                        int32_t numerics, inr_stream_t s);

/* ---- weight gradient of the tiny bias-free MLP layers (replaces the BLAS call autograd makes for
 * nn.Linear in NeRFNetwork, a9/a13):  grad_w[o][i] += sum_m grad_y[m][o] * x[m][i],  n_in, n_out <= 64.
 * x [M, n_in], grad_y [M, n_out], grad_w [n_out, n_in] is ACCUMULATED into (caller zeroes it).
 * workspace: inr_linear_wgrad_workspace_bytes() bytes of scratch (per-workgroup partial sums; two passes, no
 * atomics - same-address float atomics from hundreds of workgroups were the slowest part of this op).  */
int64_t inr_linear_wgrad_workspace_bytes(void);
int inr_linear_wgrad(const float* x, const float* grad_y, int64_t M, int32_t n_in, int32_t n_out,
                     float* grad_w, void* workspace, inr_stream_t s);

/* ---- optimiser (replaces the Trainer's torch.optim.Adam sweep over the table, a15) ------ */
int inr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, int32_t step, float grad_scale,
                  inr_stream_t s);
/* The same update for up to 16 tensors in one launch; host arrays of device pointers / sizes / learning rates. */
int inr_adam_step_multi(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avgs,
                        float* const* exp_avg_sqs, const int64_t* numels, const float* lrs, float beta1, float beta2,
                        float eps, int32_t step, float grad_scale, inr_stream_t s);
/* The same with the parameter EMA of upstream's Trainer (torch_ema: shadow += w * (param - shadow) after every step)
 * applied while the new parameter is in registers: ema_shadows[t] (device, nullable per tensor), w = ema_weight. */
int inr_adam_ema_step_multi(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avgs,
                            float* const* exp_avg_sqs, const int64_t* numels, const float* lrs, float beta1, float beta2,
                            float eps, int32_t step, float grad_scale, float* const* ema_shadows, float ema_weight,
                            inr_stream_t s);
/* The same with the step-dependent scalars in DEVICE memory (hyper_dev = [eps_t, lr_t[0..15]], written by
 * inr_adam_set_hyper on the stream - the values travel as kernel arguments, no host buffer has to stay alive): a
 * captured hipGraph of a training step can then be replayed with a new learning rate and bias correction. */
int inr_adam_set_hyper(const float* lrs /*host*/, int32_t n_tensors, float beta1, float beta2, float eps,
                       int32_t step, float* hyper_dev /*[17]*/, inr_stream_t s);
int inr_adam_step_multi_dev(int32_t n_tensors, float* const* params, const float* const* grads,
                            float* const* exp_avgs, float* const* exp_avg_sqs, const int64_t* numels,
                            const float* hyper_dev, float beta1, float beta2, float grad_scale, inr_stream_t s);
/* No upstream counterpart.  n <= 8 device-to-device copies in one launch (the fixed input buffers of a captured training
 * step); dsts / srcs / nbytes are HOST arrays, addresses and byte counts multiples of 4.                                */
int inr_copy_multi(int32_t n, void* const* dsts, const void* const* srcs, const int64_t* nbytes, inr_stream_t s);
/* The same two calls with the parameter EMA inside the captured sweep (no upstream counterpart; torch_ema's update folded
 * into the optimiser's launch as inr_adam_ema_step_multi does for eager steps): hyper_dev holds 18 floats, the last one
 * the EMA weight 1 - decay_t of the step, written by inr_adam_set_hyper_ema; ema_shadows[t] nullable per tensor.      */
int inr_adam_set_hyper_ema(const float* lrs /*host*/, int32_t n_tensors, float beta1, float beta2, float eps, int32_t step,
                           float ema_weight, float* hyper_dev, inr_stream_t s);
int inr_adam_ema_step_multi_dev(int32_t n_tensors, float* const* params /*host array of device pointers*/,
                                const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                                const int64_t* numels /*host*/, const float* hyper_dev, float beta1, float beta2,
                                float grad_scale, float* const* ema_shadows /*host array*/, inr_stream_t s);
/* Mask-supervised loss of the instance stage (a13; replaces F.cross_entropy(logits, labels, ignore_index) + its
 * backward in the fork's instance trainer): loss[0] = mean over rows with 0 <= label < K and label != ignore_index of
 * logsumexp(row) - row[label]; grad_logits [N,K] = d loss / d logits (zero rows where ignored); acc = 128 floats of
 * scratch (per-workgroup partial sums: no atomics), 8-byte aligned.  K <= 64.  NaN loss when no row is kept (torch's
 * mean over an empty set) AND when a label is neither ignore_index nor in [0, K) (torch asserts on the device for such
 * a label; the row is never dropped silently).                                                                    */
int inr_cross_entropy(const float* logits /*[N,K]*/, const int64_t* labels /*[N]*/, int64_t N, int32_t K,
                      int64_t ignore_index, float* grad_logits, float* acc, float* loss, inr_stream_t s);
/* Tail of NeRFRenderer.run_cuda (a14): image_out = image + (1 - weights_sum) * bg;
 * depth_out = clamp(depth [+ t0 * weights_sum] - near, 0) / (far - near); outputs may alias the inputs.  t0 (nullable)
 * = start parameter of every ray: upstream's inference compositing accumulates depth over the ABSOLUTE ray parameter
 * (composite_rays: t = rays_t), its training compositing over t counted from the first step (composite_rays_train:
 * t = 0); the one-pass inference kernels here count like the latter, so inference passes t0 (= nears without jitter).
 * No autograd: callers that need gradients through the image use torch ops. */
int inr_finish_rays(const float* image /*[N,3]*/, const float* depth /*[N]*/, const float* weights_sum,
                    const float* nears, const float* fars, const float* t0 /*[N] nullable*/, float bg_r, float bg_g,
                    float bg_b, int64_t N, float* image_out, float* depth_out, inr_stream_t s);

/* The training tail of the NeRF stage in one launch (Trainer.train_step, stage "nerf", default criterion): the blend and
 * depth of inr_finish_rays (training: no t0), loss[0] = mean((image_out - target)^2) over the 3N channels - upstream's
 * ``criterion(pred, gt).mean()`` with MSELoss(reduction='none') -, and the gradients of that loss:
 * grad[0, 3N) = d loss / d image, grad[3N, 4N) = d loss / d weights_sum (the blend's -sum_c g_c * bg_c).
 * bg_rays (nullable, [N,3]) replaces the uniform colour per ray.  One workgroup, fixed summation order:
 * 0 < N <= INR_FINISH_MSE_MAX_RAYS; larger batches use inr_finish_rays / torch ops. */
#define INR_FINISH_MSE_MAX_RAYS 65536
int inr_finish_rays_mse(const float* image /*[N,3]*/, const float* depth /*[N]*/, const float* weights_sum,
                        const float* nears, const float* fars, float bg_r, float bg_g, float bg_b,
                        const float* bg_rays /*[N,3] nullable*/, const float* target /*[N,3]*/, int64_t N,
                        float* image_out, float* depth_out, float* grad /*[4N]*/, float* loss /*[1]*/, inr_stream_t s);

/* ---- Image quality of rendered views: SSIM and the squared error in one launch (csrc/ssim.hip) ----------------------
 * Upstream's nerf/utils.py evaluates held-out views with PSNRMeter and SSIMMeter [U]; this is the kernel behind
 * instance_nerf_amd.metrics.image_quality and nerf.utils.SSIMMeter.  The reference project has no counterpart.
 *
 * Inputs: pred, truth float32 [B, H, W, C], dense and channels-last (the layout the renderer writes); 1 <= C <= 4;
 * H, W >= 11 (smaller: INR_EINVAL); B*H*W*C < 2^31; B and the number of tile rows <= 65535.
 * Window: separable, 11 taps, sigma 1.5: g[i] = exp(-(i-5)^2 / (2 sigma^2)), normalised to sum 1 in binary64, THEN
 * rounded to binary32 - those eleven binary32 values are the contract (instance_nerf_amd.metrics.gaussian_window).  The
 * caller computes them and passes them in `window11` (HOST memory, finite values; they travel as kernel arguments).
 * Valid windows only: the map is [B, H-10, W-10, C]; map pixel (i, j) covers input rows i..i+10 and columns j..j+10
 * (believed to equal torchmetrics' reflect-pad-then-crop default; not verified).
 * Per window and channel, with E[.] the windowed sum:  mu_x = E[x], mu_y = E[y], var_x = E[x^2] - mu_x^2, var_y likewise,
 * cov = E[xy] - mu_x mu_y, and
 *   SSIM = ((2 mu_x mu_y + C1) (2 cov + C2)) / ((mu_x^2 + mu_y^2 + C1) (var_x + var_y + C2)),  C1 = (0.01 L)^2, C2 = (0.03 L)^2.
 * L = data_range_dev[0], ONE float on the device (so neither a constant nor a range inferred by device reductions is
 * read back by the caller).
 * Arithmetic of the kernel (tests/ssim_reference.py restates it in binary32): a workgroup owns a tile of
 * INR_SSIM_TILE_W x INR_SSIM_TILE_H map pixels; per channel its pivot p is the truth pixel at the tile's first window
 * centre (row 16 ty + 5, column 64 tx + 5; 0 when that pixel is not finite); moments are taken of x - p and y - p
 * (variances and the covariance do not move under the shift - up to the 2-D window's |sum - 1| = 2.8e-9 - and lose far less to
 * cancellation), mu = shifted mean + p.  Products first (binary32), then the horizontal pass, then the vertical pass,
 * each acc = g[0] v0, acc = acc + g[k] vk for k = 1..10 with separate multiplies and adds; the formula as written above
 * with 2 (mu_x mu_y), an IEEE division.  Identical images give exactly 1.0f.
 * out_ssim [B] = mean of the map over valid pixels and channels (map entries are added in binary64, divided, rounded
 * to binary32).  out_sse [B] (nullable) = sum over ALL H*W*C elements of (pred - truth)^2: difference and square in
 * binary32, added in binary64, every input pixel counted exactly once (a tile owns its map rectangle shifted by (5, 5);
 * tiles on an image edge also own the 5-pixel border on that side).  out_map (nullable) receives the map.
 * Non-finite inputs are not masked: a NaN or +-inf under a window makes that map entry NaN and the image's mean with
 * it; a NaN pixel makes that image's sse NaN; other images of the batch are untouched.
 * Determinism: no float atomics.  Each workgroup writes its two binary64 partial sums into its own slot of `workspace`
 * (inr_ssim_workspace_bytes(B, H, W, C) bytes, 8-byte aligned, caller-owned; INR_EINVAL as a negative return for bad
 * sizes); a second tiny launch inside the same call adds the slots in a fixed order.  Two calls return the same bits. */
#define INR_SSIM_TAPS 11
#define INR_SSIM_TILE_W 64
#define INR_SSIM_TILE_H 16
int64_t inr_ssim_workspace_bytes(int64_t B, int64_t H, int64_t W, int32_t C);
int inr_ssim_forward(const float* pred, const float* truth, int64_t B, int64_t H, int64_t W, int32_t C,
                     const float* window11 /*host, [11]*/, const float* data_range_dev /*[1]*/, float* out_ssim /*[B]*/,
                     float* out_sse /*[B] nullable*/, float* out_map /*[B,H-10,W-10,C] nullable*/, void* workspace,
                     int64_t workspace_bytes, inr_stream_t s);

/* ---- Segmentation confusion matrix of rendered instance maps (csrc/confusion.hip) -----------------------------------
 * The joint (truth id, predicted id) histogram of B images of N pixels each: the one object from which mIoU, pixel
 * accuracy, per-pair IoU and panoptic quality follow exactly (instance_nerf_amd.metrics.segmentation_confusion /
 * segmentation_scores, nerf.utils.SegmentationMeter).  The reference project has no counterpart.
 *
 * Matrix: counts int64 [B, K, K+1], 1 <= K <= INR_CONFUSION_MAX_K (the project's limit on instance channels).
 * counts[b, t, p] = number of pixels of image b with truth id t and predicted id p, both in [0, K).  Column K collects
 * the pixels whose truth is valid but whose prediction lies outside [0, K): row sums stay equal to the truth areas, and
 * such a pixel counts towards the truth and the union of t and towards no prediction (what nerf.utils.MIoUMeter does
 * with it).
 * Ignored pixels: ignored int64 [B].  A pixel whose truth lies outside [0, K) - the ignore label -1, any other negative
 * value, any value >= K - is counted there and nowhere else, whatever its prediction.
 * Accumulation: a call ADDS into counts and ignored; the caller zeroes them.  A meter accumulates a whole scene in place,
 * one call per update, and nothing is read back.
 * Arithmetic: integer atomics only (32-bit in LDS per workgroup, one 64-bit global add per non-zero counter at the end):
 * two calls give the same bits.  A workgroup of INR_CONFUSION_BLOCK threads owns a run of INR_CONFUSION_PIXELS_PER_WG
 * consecutive pixels of one image.
 * Two entry points share the histogram code:
 *   inr_confusion_ids     pred int32 [B, N], truth int32 [B, N].
 *   inr_confusion_logits  logits float32 [B, N, ld] with ld >= K the row stride in floats, truth int32 [B, N].  The
 *                         prediction is the arg-max over channels 0 .. K-1 only; channels K .. ld-1 are never read.
 * Arg-max rule: NaN compares greater than every number; among equal maxima - several NaN, or equal numbers, so -0.0 and
 * +0.0 tie - the lowest index wins.  This is torch.argmax on CPU tensors.
 * Bad arguments are INR_EINVAL with a message, before any launch: K outside [1, 64], ld < K, negative B or N,
 * B*N*ld >= 2^63 (element indices are 64-bit) or more than 2^31 - 1 workgroups (B * ceil(N / INR_CONFUSION_PIXELS_PER_WG)),
 * null pointers, counts or ignored not 8-byte aligned.  B == 0 or N == 0 is a valid no-op returning 0 (sizes, K and ld are
 * still checked; no pointer is looked at).                                                                            */
#define INR_CONFUSION_MAX_K 64
#define INR_CONFUSION_BLOCK 256
#define INR_CONFUSION_PIXELS_PER_WG 1024
int inr_confusion_ids(const int32_t* pred /*[B,N]*/, const int32_t* truth /*[B,N]*/, int64_t B, int64_t N, int32_t K,
                      int64_t* counts /*[B,K,K+1]*/, int64_t* ignored /*[B]*/, inr_stream_t s);
int inr_confusion_logits(const float* logits /*[B,N,ld]*/, const int32_t* truth /*[B,N]*/, int64_t B, int64_t N, int32_t K,
                         int64_t ld, int64_t* counts /*[B,K,K+1]*/, int64_t* ignored /*[B]*/, inr_stream_t s);

/* ---- Detector training targets (csrc/assign.hip, csrc/box_iou.h) ----------------------------------------------------
 * What every RPN step and every RoI-head step of the reference starts with: a ground-truth box for each anchor or
 * proposal (model/rpn.py:240-290, nerf_rcnn.py:464-498: batched_box_iou, Matcher, model/utils.py:100-214,375-462) and
 * the regression targets of the box coder (coder/AABB_coder.py:7-56), without the [G, A] quality matrix.  Additive: no
 * version bump.
 *
 * Inputs: gt fp32 [G, 6] and boxes fp32 [A, 6], rows (x1, y1, z1, x2, y2, z2); valid uint8 [A], nullable: the
 * reference's padding mask (non-zero = a real box).
 * Quality: q[g, a] = the reference's AABB IoU of GT box g and box a, all in fp32, every operation rounded on its own (no
 * fused multiply-add), IEEE division: volume = ((x2 - x1) * (y2 - y1)) * (z2 - z1); extents e = min(hi) - max(lo)
 * clamped at 0; inter = (e0 * e1) * e2; q = inter / ((volume_gt + volume_box) - inter).  min, max and the clamp keep a
 * NaN operand (torch's rule); 0 / 0 is a NaN.  A box with valid == 0 has q[:, a] = -1.0f.
 * Row maxima: gt_max[g] = the maximum of q[g, :], a NaN above every number, kept as an order-preserving uint32 key:
 * NaN -> 0xFFFFFFFF; sign bit set -> ~bits; otherwise bits | 0x80000000 (so -1 sorts below +0).
 *
 * inr_box_match_gt_max: gt_max_keys uint32 [G] = those keys.  The call zeroes the keys itself (key 0 is below every
 *   value), then one launch: a workgroup of INR_BOX_MATCH_BLOCK lanes owns INR_BOX_MATCH_BOXES_PER_WG consecutive boxes,
 *   keeps the maxima with integer max in LDS and issues at most one global integer max per (workgroup, GT).  Integer
 *   arithmetic only: two calls give the same bits.
 * inr_box_match_assign: one lane per box recomputes its G qualities with the same device function and applies the
 *   Matcher:
 *     best, arg = the maximum of q[:, a] and its index: the lowest index among equals, a NaN counts as the maximum and
 *       the first NaN wins (torch.max over dim 0 on CPU tensors);
 *     matched[a] = arg;  -1 if best < low;  -2 if low <= best < high (fp32 comparisons; a NaN best keeps arg);
 *     allow_low_quality != 0: if q[g, a] == gt_max[g] for ANY g (float ==, never true for a NaN), matched[a] = arg again.
 *       This keeps the reference's quirk: a GT whose row maximum is 0 restores every box with IoU 0 against it, and a
 *       row maximum of -1 (every box masked) restores the masked boxes.
 *   Outputs: matched int32 [A]; and, each nullable,
 *     labels int32 [A]: with gt_labels (int32 [G]) gt_labels[matched] for matched >= 0, without it 1; 0 for -1; -1 for
 *       -2; and -1 wherever valid == 0, applied last (rpn.py:283-285);
 *     best_iou fp32 [A] = best;
 *     matched_boxes fp32 [A, 6] = gt[max(matched, 0)];
 *     targets fp32 [A, 6] = encode_boxes_3d(matched_boxes, boxes): per axis w = x2 - x1, ctr = x1 + 0.5f * w for both
 *       boxes, (ctr_gt - ctr_box) / w_box in columns 0..2 and logf(w_gt / w_box) in columns 3..5, one fp32 operation at
 *       a time in that order.
 *   One launch; nothing is read back.
 * Limits, checked before any launch (INR_EINVAL with a message): 1 <= G <= INR_BOX_MATCH_MAX_GT (32 B of LDS per GT:
 * 32 KB), A >= 0, 6 * A < 2^31, low <= high (neither a NaN), gt, boxes, gt_max_keys and matched not null, every array
 * but valid 4-byte aligned.  A == 0 is a valid no-op returning 0 (G and the thresholds are still checked; no pointer is
 * looked at, the keys are left alone).                                                                             */
#define INR_BOX_MATCH_MAX_GT 1024
#define INR_BOX_MATCH_BLOCK 256
#define INR_BOX_MATCH_BOXES_PER_WG 1024
int inr_box_match_gt_max(const float* gt /*[G,6]*/, int32_t G, const float* boxes /*[A,6]*/,
                         const uint8_t* valid /*[A] nullable*/, int64_t A, uint32_t* gt_max_keys /*[G]*/, inr_stream_t s);
int inr_box_match_assign(const float* gt /*[G,6]*/, const int32_t* gt_labels /*[G] nullable*/, int32_t G,
                         const float* boxes /*[A,6]*/, const uint8_t* valid /*[A] nullable*/, int64_t A,
                         const uint32_t* gt_max_keys /*[G]*/, float high, float low, int32_t allow_low_quality,
                         int32_t* matched /*[A]*/, int32_t* labels /*[A] nullable*/, float* best_iou /*[A] nullable*/,
                         float* matched_boxes /*[A,6] nullable*/, float* targets /*[A,6] nullable*/, inr_stream_t s);

/* ---- FCOS training targets and losses (csrc/fcos.hip) ---------------------------------------------------------------
 * What every training step of the reference's FCOS proposal head starts and ends with (nerf_rcnn/model/fcos/loss.py:
 * prepare_targets, compute_centerness_targets, IOULoss, __call__): one ground-truth box per location of the pyramid, and
 * the three losses with their gradients, without a [P, G] tensor, a permuted copy of the predictions or a read-back.
 * Axis-aligned boxes only.  Additive: no version bump.
 *
 * Pyramid: HOST arrays as in inr_roi_align_3d_pyramid_forward, travelling in the kernel arguments: level_dims int32
 * [n_levels*3] = (W, L, H) per level, level_strides int32 [n_levels], level_ranges fp32 [n_levels*2] = (lo_l, hi_l), the
 * sizes of interest.  P_l = W*L*H, 1 <= n_levels <= INR_FCOS_MAX_LEVELS; B scenes.  Every per-location array is
 * LEVEL-FIRST, the layout of the reference's lists: level l starts at B * (P_0 + ... + P_{l-1}), scene b of it at
 * b * P_l more, location p = (ix * L + iy) * H + iz.
 * Ground truth: gt fp32 [sum G_b, 6], rows (x1, y1, z1, x2, y2, z2), and gt_offsets int32 [B+1] on the DEVICE; scene b
 * owns rows gt_offsets[b] .. gt_offsets[b+1]-1.  max_gt >= every G_b sizes the LDS (52 B per box); the kernel looks at
 * no more than max_gt boxes of a scene.  0 <= max_gt <= INR_FCOS_MAX_GT.
 *
 * Target rule (all fp32, one operation at a time, no fused multiply-add, IEEE division and square root):
 *  1. location p of level l has the coordinate i * stride + stride / 2 (integer division) per axis;
 *  2. reg[g] = (x - x1, y - y1, z - z1, x2 - x, y2 - y, z2 - z);
 *  3. inside[g]: radius > 0: s = (float)((double)stride * radius), c = (lo + hi) / 2 per axis, rlo = c - s > lo ? c - s : lo,
 *     rhi = c + s > hi ? hi : c + s, and the minimum of the six distances to (rlo, rhi) is > 0; radius == 0: min(reg[g]) > 0;
 *  4. cared[g]: max(reg[g]) >= lo_l and max(reg[g]) <= hi_l (a NaN distance fails both tests);
 *  5. area[g] = inside and cared ? ((x2-x1)*(y2-y1))*(z2-z1) : 1e8f; matched = the arg-min over g, the lowest index among
 *     equals, a NaN counts as the minimum and the first NaN wins (torch.min on CPU tensors); label = area[matched] != 1e8f
 *     ? 1 : 0; reg_target = reg[matched] - ALSO where the label is 0, as the reference has it -, divided by (float)stride
 *     when norm_reg_targets != 0;
 *  6. centerness = sqrtf((min(r0,r3)/max(r0,r3)) * (min(r1,r4)/max(r1,r4)) * (min(r2,r5)/max(r2,r5))) of reg_target where
 *     the label is 1 (min and max keep a NaN), 0 elsewhere;
 *  7. valid = x < w_ori and y < l_ori and z < h_ori with ori_sizes fp32 [B, 3] (valid needs ori_sizes).
 *  A scene without boxes gives label 0, reg_target 0, centerness 0, matched 0.
 * inr_fcos_targets: ONE launch for all scenes and levels.  One lane per location; a workgroup of INR_FCOS_BLOCK lanes owns
 *   INR_FCOS_LOCATIONS_PER_WG consecutive locations of one (level, scene) and stages that scene's boxes, volumes and
 *   sample regions in LDS once.  Outputs labels fp32 [T], reg_targets fp32 [T, 6] and, each nullable, centerness fp32 [T],
 *   matched int32 [T], valid uint8 [T], with T = B * sum P_l.
 *
 * Losses.  Predictions are the head's own tensors, read in place: per level cls [B,1,W,L,H], reg [B,6,W,L,H]
 * (channel-planar), ctr [B,1,W,L,H], as HOST arrays of n_levels device pointers.  Per location with valid != 0 (all,
 * when valid is null), t = label:
 *   focal  = torchvision's sigmoid_focal_loss(x, t, alpha 0.25, gamma 2): p = sigmoid(x), ce = max(x,0) - x t +
 *            log1p(exp(-|x|)), p_t = p t + (1-p)(1-t), focal = (alpha t + (1-alpha)(1-t)) * (ce * (1-p_t)^2);
 *   and where t > 0, with c = the centerness of reg_target (rule 6; recomputed, not read):
 *   regterm = IOULoss(pred, reg_target) * c (loss.py:85-132 in that operation order; iou_loss_type INR_FCOS_LOSS_IOU
 *            -log(iou), _LINEAR_IOU 1 - iou, _GIOU 1 - giou);
 *   bce    = max(y,0) - y c + log1p(exp(-|y|)) of the centerness logit y.
 *   The reference sums the IoU losses unweighted when the weights do not sum above 0; positives of rule 5 have all six
 *   distances above 0, so that branch is not followed.
 * inr_fcos_loss_forward: terms in fp32, five sums in FLOAT64 per workgroup into `workspace`
 *   (inr_fcos_loss_workspace_bytes(T) bytes, 8-byte aligned; a negative return for a bad T), a second small launch adds
 *   the partial sums in a fixed order: two calls give the same bits.  sums double [5] = (focal, regterm, bce, n_pos,
 *   sum of c) - the two normalisers last, adjacent -; losses fp32 [3] = (focal / max(n_pos, 1), regterm / sum c,
 *   bce / max(n_pos, 1)), the last two 0 when n_pos == 0.  cls_terms, reg_terms, ctr_terms fp32 [T], each nullable: the
 *   per-location terms, 0 where a term does not apply.
 * inr_fcos_loss_backward: recomputes each location's derivative and scales it: d_cls = grad_losses[0] / max(norms[0], 1)
 *   * d focal / dx; d_reg = grad_losses[1] / norms[1] * c * d IOULoss / d pred; d_ctr = grad_losses[2] / max(norms[0], 1)
 *   * (sigmoid(y) - c).  norms double [2] = (n_pos, sum c) - sums + 3, or their all-reduced average - and grad_losses
 *   fp32 [3] are read from DEVICE memory.  d_cls, d_reg (channel-planar), d_ctr: HOST arrays of device pointers in the
 *   predictions' layouts, every element written (0 where valid == 0; d_reg and d_ctr 0 where the label is 0).  Inside
 *   min / max, pred == target sends half the gradient to each side (torch's rule for minimum / maximum).
 * Limits, checked before any launch (INR_EINVAL with a message): n_levels in 1..INR_FCOS_MAX_LEVELS, B >= 0, every
 * extent and stride >= 1 with extent * stride < 2^24, 6 * T < 2^31, max_gt in 0..INR_FCOS_MAX_GT, radius >= 0, a known
 * iou_loss_type, required pointers not null, fp32 / int32 arrays 4-byte and double arrays 8-byte aligned, the workspace
 * large enough.  T == 0 (B == 0) is a valid no-op returning 0 after these checks; no device pointer is looked at. */
#define INR_FCOS_MAX_LEVELS 8
#define INR_FCOS_MAX_GT 1024
#define INR_FCOS_BLOCK 256
#define INR_FCOS_LOCATIONS_PER_WG 256
#define INR_FCOS_LOSS_LOCATIONS_PER_WG 1024
#define INR_FCOS_LOSS_IOU 0
#define INR_FCOS_LOSS_LINEAR_IOU 1
#define INR_FCOS_LOSS_GIOU 2
int inr_fcos_targets(const int32_t* level_dims /*host*/, const int32_t* level_strides /*host*/,
                     const float* level_ranges /*host*/, int32_t n_levels, int32_t B, const float* gt /*[sum G,6]*/,
                     const int32_t* gt_offsets /*[B+1]*/, int32_t max_gt, const float* ori_sizes /*[B,3] nullable*/,
                     float radius, int32_t norm_reg_targets, float* labels /*[T]*/, float* reg_targets /*[T,6]*/,
                     float* centerness /*[T] nullable*/, int32_t* matched /*[T] nullable*/, uint8_t* valid /*[T] nullable*/,
                     inr_stream_t s);
int64_t inr_fcos_loss_workspace_bytes(int64_t T);
int inr_fcos_loss_forward(const float* const* cls_ptrs /*host*/, const float* const* reg_ptrs /*host*/,
                          const float* const* ctr_ptrs /*host*/, const int32_t* level_dims /*host*/, int32_t n_levels,
                          int32_t B, const float* labels /*[T]*/, const float* reg_targets /*[T,6]*/,
                          const uint8_t* valid /*[T] nullable*/, int32_t iou_loss_type, double* sums /*[5]*/,
                          float* losses /*[3]*/, float* cls_terms /*[T] nullable*/, float* reg_terms /*[T] nullable*/,
                          float* ctr_terms /*[T] nullable*/, void* workspace, int64_t workspace_bytes, inr_stream_t s);
int inr_fcos_loss_backward(const float* const* cls_ptrs /*host*/, const float* const* reg_ptrs /*host*/,
                           const float* const* ctr_ptrs /*host*/, const int32_t* level_dims /*host*/, int32_t n_levels,
                           int32_t B, const float* labels /*[T]*/, const float* reg_targets /*[T,6]*/,
                           const uint8_t* valid /*[T] nullable*/, int32_t iou_loss_type, const double* norms /*[2]*/,
                           const float* grad_losses /*[3]*/, float* const* d_cls_ptrs /*host*/,
                           float* const* d_reg_ptrs /*host*/, float* const* d_ctr_ptrs /*host*/, inr_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* INR_H */
