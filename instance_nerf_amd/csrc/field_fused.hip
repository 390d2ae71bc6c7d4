// Fused field evaluation for gfx950 (SURVEY a7 + a9 + a10 + a13): hash-grid gather, SH-4 and
// the sigma / colour / instance MLPs in ONE kernel; the 32 encoded features and all hidden
// activations live in registers and never touch HBM.
//
// MLP on the matrix cores with fp32-class accuracy at bf16 rate: v_mfma_f32_16x16x32_bf16 with a
// 3-term split  x*w ~= xh*wh + xh*wl + xl*wh  (xh/xl, wh/wl = bf16 head and remainder; the dropped
// xl*wl term is 2^-16 relative; products are exact and accumulate in fp32).  60 MFMAs of ~16 cycles
// per 16-sample tile instead of 160 fp32 MFMAs (v_mfma_f32_16x16x4_f32) of 32 cycles.  The exact-fp32
// variant is kept behind -DINR_MLP_FP32=1 for A/B runs.
// Operand maps (both shapes): A[i=lane&15][k-slot lane>>4], B[k-slot lane>>4][j=lane&15],
// D[i=4*(lane>>4)+r][j=lane&15]; the bf16 shape carries 8 k values per slot, the f32 shape one.
//
// Transposed formulation - H^T = W * X^T - with a 16-sample tile per wave:
//   * B operand = activations: lane (q = lane>>4, j = lane&15) holds input k-slot q of sample j;
//   * A operand = weights:     lane holds W[out = 16*mt + j][k-slot q], pre-packed on the host
//     into fragment order and staged once per workgroup in LDS (40 KB, ds_read_b128);
//   * D = 16 outputs x 16 samples: lane (q, j), register r holds output 4q+r of sample j.
// A dot product does not care in which order k is visited, so the k-step (nt, r) of the next
// layer is DEFINED to cover inputs {16nt + 4q + r : q = 0..3}: that is exactly register r of
// output tile nt of the previous layer.  Layer outputs therefore feed the next layer's B
// operand in place - no LDS transpose, no cross-lane traffic between layers.
// The same trick places the encoder: lane q of a sample owns levels {2q, 2q+1, 8+2q, 9+2q}
// (features 16*(s>>2) + 4q + (s&3), s = 0..7), so four lanes share one sample's 128 gathers.
//
// Compiled with -ffp-contract=off (cell selection is the oracle's decision); blending and the
// MFMA chain are explicit fmaf / MFMA.
#include <atomic>
#include <mutex>
#include <type_traits>

#include "common.h"
#include "grid_common.h"
#include "sample_pos.h"

namespace inr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#ifndef INR_MLP_FP32
#define INR_MLP_FP32 0
#endif

// Ablation variants for profiling (no MLP, per-workgroup time stamps, static tile deal, one slow XCD) produce WRONG
// results.  Their code lives outside the sources build.py compiles - csrc/probe/field_probe.h, which only
// tools/build_probe.py adds (-DINR_PROBE_BUILD) - and hooks in through the INR_PROBE_* macros below, all empty here
// (round-5 verdict item 7a: a stray -D must not be able to turn the product into a silently wrong library).
#ifdef INR_PROBE_BUILD
#include "probe/field_probe.h"
#else
#if defined(INR_PROBE_MODE) || defined(INR_PROBE_STATIC) || defined(INR_PROBE_SLOW_XCD)
#error "INR_PROBE_* switches need -DINR_PROBE_BUILD (tools/build_probe.py): those variants produce wrong results"
#endif
#define INR_PROBE_PROLOGUE()
#define INR_PROBE_SCHEDULE(steal)
#define INR_PROBE_TILE()
#define INR_PROBE_AFTER_GATHER()
#define INR_PROBE_GEO_IS_OUTPUT 1
#define INR_PROBE_EPILOGUE()
#endif

// (ns-1, BASELINE north star "LDS staging of per-level feature tiles": besides the weights and the level records,
//  level 0 of the table - dense, 4 920 rows = 39 KB - was made LDS-resident for the eval kernel in round 3, its eight
//  look-ups per sample served by ds_read_b64.  Bit-identical, measured, rejected: 5.37-5.40 vs 5.20-5.25 ms per 37 M
//  samples with the select placed after all loads are out (-3.3 % L1 look-ups, +8 % VALU instructions: the look-ups it
//  removes were the cheapest - 16 samples of a tile share one or two lines of level 0), 6.73 ms with the select inside
//  the issue loop.  profiles/r03_NOTES.txt section 6, r03f / r03g PMC files.)

// packed-buffer section offsets, in floats
constexpr int kSig0 = 0;                       // 64 x 32  : 4 mt x 8 ks
constexpr int kSig1 = kSig0 + 64 * 32;         // 16 x 64  : 1 mt x 16 ks
constexpr int kCol0 = kSig1 + 16 * 64;         // 64 x 32  : 4 mt x 8 ks   (16 sh + 16 sigma-net rows)
constexpr int kCol1 = kCol0 + 64 * 32;         // 64 x 64  : 4 mt x 16 ks
constexpr int kCol2 = kCol1 + 64 * 64;         // 16 x 64  : 1 mt x 16 ks  (3 live rows)
constexpr int kNerfFloats = kCol2 + 16 * 64;   // 10240 floats = 40 KB
constexpr int kIns0 = 0;                       // 64 x 32
constexpr int kIns1 = kIns0 + 64 * 32;         // 64 x 64
constexpr int kIns2 = kIns1 + 64 * 64;         // K x 64   : K/16 mt x 16 ks

// position of fragment value (mt, ks, lane) inside a section with n_ks k-steps
__host__ __device__ inline int frag_pos(int mt, int ks, int lane, int n_ks) {
  return ((mt * (n_ks / 4) + ks / 4) * 64 + lane) * 4 + (ks & 3);
}

__device__ __forceinline__ f32x4 mfma4(const float4 a, const f32x4 b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[3], c, 0, 0, 0);
  return c;
}
// ReLU as ONE integer max on the bit pattern (negative floats, -0 and negative NaNs are negative integers);
// fmaxf() costs two v_max_f32 here because the compiler canonicalises MFMA outputs first.
__device__ __forceinline__ float relu1(float x) { return __int_as_float(max(__float_as_int(x), 0)); }
__device__ __forceinline__ f32x4 relu4(f32x4 v) {
  v[0] = relu1(v[0]); v[1] = relu1(v[1]); v[2] = relu1(v[2]); v[3] = relu1(v[3]);
  return v;
}

// ---- encoder, one lane's quarter of a sample -----------------------------------------------------
// Lane q owns levels {2q, 2q+1, 8+2q, 9+2q}; their constants are loaded ONCE per wave (they do
// not depend on the tile).  Indexing is branch-free: the dense index cx + cy*s + cz*s^2 and the
// hash cx ^ cy*p1 ^ cz*p2 share the two multiplies (pa, pb = strides or primes) and differ only
// in the combining operator, selected per lane with v_cndmask; (cy+1)*pa = cy*pa + pa (mod 2^32).
// Gathers are buffer loads: one 32-bit byte offset per corner against a wave-uniform descriptor
// of the whole table (49 MB < 4 GB), so a corner costs ONE address VGPR and is bounds-checked.
// Per-(q, slot) level constants live in LDS (16 records of 8 words, written once per workgroup) and are
// re-read per tile right before use - two ds_read_b128 per level - instead of occupying ~24 VGPRs
// for the whole kernel: the gather phase already holds 64 data + 12 fraction registers per lane and
// must stay <= 128 VGPRs for 4 waves/SIMD.
//   word 0 scale (f32)   1 byte offset of the level's first row   2 pa   3 pb   4 mask   5 hashed(0/1)
//   word 6 all ones if hashed, else 0   7 all ones if dense, else 0   (the lane masks of index_terms below)
// A level beyond num_levels needs no predicate: all its words are 0, so its gathers read row 0 of the
// table (valid memory, finite) and its two features meet all-zero weight columns (the packer zero-fills
// inputs >= 2 * num_levels).
struct LevelRec {
  uint4 a, b;
};
constexpr int kLevelRecBytes = 16 * sizeof(LevelRec);   // 512 B after the weights

__device__ __forceinline__ void stage_level_recs(const GridDesc& G, LevelRec* recs) {
  const int t = threadIdx.x;
  if (t < 16) {
    const int q = t >> 2, li = t & 3;
    const int l = (li >> 1) * 8 + 2 * q + (li & 1);
    const bool live = l < G.num_levels;
    const int lc = live ? l : 0;
    const uint32_t m = G.mask[lc], s = G.res1[lc];
    LevelRec r;
    r.a.x = live ? __float_as_uint(G.scales[lc]) : 0u;
    r.a.y = live ? G.offsets[lc] * 8u : 0u;
    r.a.z = !live ? 0u : (m ? 2654435761u : s);
    r.a.w = !live ? 0u : (m ? 805459861u : s * s);
    r.b.x = !live ? 0u : (m ? m : 0xFFFFFFFFu);
    r.b.y = (live && m) ? 1u : 0u;
    r.b.z = (live && m) ? 0xFFFFFFFFu : 0u;
    r.b.w = (live && !m) ? 0xFFFFFFFFu : 0u;
    recs[t] = r;
  }
}

// wave-uniform (kernel arguments only): slot li is served by hashed, present levels for every q
__device__ __forceinline__ bool slot_all_hashed(const GridDesc& G, int li) {
  bool ah = true;
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    const int lq = (li >> 1) * 8 + 2 * qq + (li & 1);
    ah = ah && (lq < G.num_levels) && (G.mask[lq < G.num_levels ? lq : 0] != 0);
  }
  return ah;
}

typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));

// Default cache policy on the gathers (raw_buffer_load aux 0).  Measured and rejected in round 2:
// nt on the fine levels 15.5 ms, sc1 9.25 ms, sc0 = default 6.07 ms per 37 M samples.
// kHalf: the table is a half-precision copy ([T,2] fp16, 4 bytes per row - upstream's `-O` / fp16 storage as an
// OPT-IN for inference, NeRFNetwork.half_table): a row is one dword, its byte offset half the fp32 one, and the two
// features are widened when they are blended (v_cvt_f32_f16 x 2 per corner).  512 instead of 1024 algorithmic bytes
// per sample; 32 instead of 16 rows per 128-byte line.
// (two steps, so that a batch of gathers can form all its offsets first: see keep_offsets)
template <bool kHalf = false>
__device__ __forceinline__ uint32_t table_offset(uint32_t byte_off) {     // byte_off: of the fp32 table's row
  return kHalf ? byte_off >> 1 : byte_off;
}
template <bool kHalf = false>
__device__ __forceinline__ u32x2 gather_at(__amdgpu_buffer_rsrc_t rsrc, uint32_t off) {
  if constexpr (kHalf) {
    u32x2 r;
    r[0] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)off, 0, 0);
    r[1] = 0u;
    return r;
  } else {
    return __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)off, 0, 0);
  }
}
template <bool kHalf = false>
__device__ __forceinline__ u32x2 gather_row(__amdgpu_buffer_rsrc_t rsrc, uint32_t byte_off) {
  return gather_at<kHalf>(rsrc, table_offset<kHalf>(byte_off));
}

// Lane-paired gather for the FINE slots (levels 8..15).  Measured on MI355X (tools/micro/gather_bench.hip): the vector
// memory path prices a gather instruction by the number of DISTINCT 128-byte lines its 64 lanes touch - any two lanes
// of the wave that hit the same line share one look-up (1.6 distinct lines per clock per CU out of the L1, 0.45 out of
// the L2, 0.10 out of the Infinity Cache) - while the same line touched by two different instructions is looked up
// twice.  The two x-neighbour corners of a cell sit in one line 15 times out of 16 (x is the fastest index in dense
// and hashed levels), and on the fine levels neighbouring samples share nothing, so there every corner is its own
// look-up.  Hence: lanes q and q^1 of a sample (one "pair") together own the four fine levels {8+4p .. 11+4p},
// p = q>>1; each fetches ITS x side (q&1) of all four - 16 loads per lane as before - so that the x-neighbour rows are
// requested by two lanes of ONE instruction and share a look-up.  Each lane blends its side's four corners per level;
// the two halves meet through v_permlane16_swap_b32 (lanes 16 apart exchange registers): 4 swaps + 4 adds per tile,
// after which lane q holds the complete features of its own two fine levels exactly where the MLP expects them.
// The coarse slots (levels 0..7) keep the one-lane-per-level scheme: there neighbouring samples already share lines.
//
// Instruction diet (the kernel is co-limited by VALU issue: 775 VALU instructions per tile before):
//  * cell = (uint)pos and fraction = v_fract_f32(pos) instead of floor / subtract / convert: pos >= 0.5, so truncation
//    IS the floor, and pos - floor(pos) is exact in binary32, so v_fract returns the same bits;
//  * weights and blending on the packed-fp32 pipe: the two features of a row arrive as a register pair and take the
//    same weight (v_pk_fma_f32 with a broadcast operand), x-neighbour weights are formed two at a time (v_pk_mul_f32);
//    every component is the same IEEE operation as before - (wx*wy)*wz, then fma in corner order - so nothing changes
//    numerically;
//  * the dense/hashed select of the coarse slots once per level instead of once per corner (index_terms), the colour
//    sigmoid once on the lanes q < 3 instead of three times on the lanes q = 0 (rgb_channel_of_lane), and no clause
//    breaker between back-to-back gathers (keep_offsets).  Hot loop of k_nerf_fwd<true,true> after these, read off the
//    ISA (profiles/r07_issue_path_isa.md): xor-only gather block 210 VALU + 1 s_nop (was 235 + 18), blend + sigma net
//    186 VALU / 18 MFMA, colour net 157 VALU / 42 MFMA, epilogue 20 VALU of which 2 transcendental (was 49 / 6),
//    input loads 18: 591 VALU per tile (was 642 by the same reading).
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct Gathered {
  u32x2 c[2][8];      // coarse slots: raw rows [level][corner]
  u32x2 f[4][4];      // fine slots: this lane's x side, [level of the pair][yz corner]
  float cfx[2], cfy[2], cfz[2];
  float fwx[4], ffy[4], ffz[4];   // fine: weight of this lane's x side, y / z fractions
};

// ONE wave-uniform branch around the whole gather sequence, none inside it.  Round 1 chose between the xor-only and
// the general index maths per level: every such diamond is a control-flow merge at which the compiler's wait-count
// pass must assume that the loads of the side NOT taken are still outstanding into the registers the other side
// writes, so it put `s_waitcnt vmcnt(2)` in front of every level's block - the 32 gathers of a tile went out in five
// batches, each waiting for the previous one, instead of all at once (found in the ISA in round 2).
// Staging of the 32 gathers of a tile (measured, profiles/r02_NOTES.txt section 9): all 32 in flight at once is NOT
// the fastest - on the table feed 5.71 ms against 5.50 ms when the fine levels' loads go out only after all but 8
// of the 16 coarse loads have landed and each later fine level waits until at most 4 loads are outstanding.  The
// kernel is throughput-bound (look-ups, VALU issue), not latency-bound, and fewer lines in flight per wave leave
// more of the 32 KB L1 to the other seven waves of the CU.  (-1 = no wait.)
constexpr int kSliceLevels = 3;           // XCD-sliced frame path (k_grid_fine_slices): levels 13..15 arrive precomputed
constexpr int kWaitAfterCoarse = 8;
constexpr int kWaitBetweenFine = 4;
// s_waitcnt vmcnt(N) only (gfx9 encoding: vmcnt[3:0] | expcnt 7 << 4 | lgkmcnt 15 << 8 | vmcnt[5:4] << 14)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  if constexpr (N >= 0) __builtin_amdgcn_s_waitcnt((N & 0xF) | (0x7 << 4) | (0xF << 8) | ((N >> 4) << 14));
}

// Row index of a corner where the lanes of one instruction mix dense and hashed levels (the coarse slots; the fine slots
// of a table with dense or dead fine levels).  The two modes differ in the combining operator only - c ^ (hy ^ hz)
// against c + (hy + hz) - and used to be selected per CORNER (xor, add, v_cndmask each, after all four yz combinations
// had been formed both ways).  Selected once per LEVEL instead: with the record's lane masks,
//   X = hashed ? hy ^ hz : 0,   A = hashed ? 0 : hy + hz,   row = ((c ^ X) + A) & mask
// is c ^ (hy ^ hz) in a hashed lane and c + (hy + hz) in a dense one - the same integer modulo 2^32, hence the same
// address - at one v_bitop3 and an add/and per yz combination and a v_xad_u32 per corner.  A dead level (all-zero
// record) gives row 0 as before.
struct IndexTerms {
  uint32_t x[4], a[4];      // yz combinations (y0z0, y1z0, y0z1, y1z1)
  __device__ __forceinline__ uint32_t row(uint32_t c, int yz, uint32_t mask) const { return ((c ^ x[yz]) + a[yz]) & mask; }
};
__device__ __forceinline__ IndexTerms index_terms(uint32_t hy0, uint32_t hy1, uint32_t hz0, uint32_t hz1,
                                                  uint32_t hashed_lanes, uint32_t dense_lanes) {
  IndexTerms t;
  t.x[0] = (hy0 ^ hz0) & hashed_lanes; t.x[1] = (hy1 ^ hz0) & hashed_lanes;
  t.x[2] = (hy0 ^ hz1) & hashed_lanes; t.x[3] = (hy1 ^ hz1) & hashed_lanes;
  t.a[0] = (hy0 + hz0) & dense_lanes; t.a[1] = (hy1 + hz0) & dense_lanes;
  t.a[2] = (hy0 + hz1) & dense_lanes; t.a[3] = (hy1 + hz1) & dense_lanes;
  return t;
}

// The offsets of a batch of gathers stay live until the batch is out.  A gather's address register dies at the load, so
// the register allocator likes to hand it out again as (half of) the load's own destination.  gfx950 code objects are
// built for XNACK "any", where a run of back-to-back memory instructions must be replayable: none of them may write a
// register that one of them reads, so the compiler's hazard pass broke every such run with an `s_nop 0` - 18 per tile
// between the gathers of the benchmark's kernel, 4 issue cycles each.  With the offsets read once more behind the batch
// (an empty asm: no instruction) destinations and addresses are disjoint and the gathers go out back to back;
// no scratch, and no more registers at the kernel's peak, which lies in the MLP.
__device__ __forceinline__ void keep_offsets(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  asm volatile("" : : "v"(a), "v"(b), "v"(c), "v"(d));
}

template <bool kFineHashed, bool kHalf = false, bool kPre = false>
__device__ __forceinline__ void issue_gathers_impl(const LevelRec* __restrict__ my_recs, __amdgpu_buffer_rsrc_t rsrc,
                                                   float x0, float x1, float x2, Gathered& g) {
  const int q = (threadIdx.x >> 4) & 3;
  const uint32_t side = (uint32_t)(q & 1);
  const LevelRec* pair_recs = my_recs - 4 * (q & 1);     // records of the even lane of this pair
#pragma unroll
  for (int li = 0; li < 2; ++li) {
    const uint4 ra = my_recs[li].a;
    const float s = __uint_as_float(ra.x);
    const uint32_t base = ra.y, pa = ra.z, pb = ra.w;
    const uint4 rb = my_recs[li].b;
    const uint32_t mask = rb.x;
    const float px = x0 * s + 0.5f, py = x1 * s + 0.5f, pz = x2 * s + 0.5f;   // mul, add: not fused
    g.cfx[li] = __builtin_amdgcn_fractf(px); g.cfy[li] = __builtin_amdgcn_fractf(py); g.cfz[li] = __builtin_amdgcn_fractf(pz);
    const uint32_t cx = (uint32_t)px, cy = (uint32_t)py, cz = (uint32_t)pz;
    const uint32_t hy0 = cy * pa, hy1 = hy0 + pa;
    const uint32_t hz0 = cz * pb, hz1 = hz0 + pb;
    const IndexTerms t = index_terms(hy0, hy1, hz0, hz1, rb.z, rb.w);   // per lane: the four q of a coarse slot mix dense and hashed
    uint32_t off[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) off[k] = table_offset<kHalf>(base + t.row(cx + (k & 1), k >> 1, mask) * 8u);
#pragma unroll
    for (int k = 0; k < 8; ++k) g.c[li][k] = gather_at<kHalf>(rsrc, off[k]);
    keep_offsets(off[0], off[1], off[2], off[3]);
    keep_offsets(off[4], off[5], off[6], off[7]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const LevelRec* rec = pair_recs + (i >> 1) * 4 + 2 + (i & 1);    // level 8 + 4p + i
    const uint4 ra = rec->a;
    const float s = __uint_as_float(ra.x);
    const uint32_t base = ra.y, pa = ra.z, pb = ra.w;
    const uint4 rb = rec->b;
    const uint32_t mask = rb.x;
    const float px = x0 * s + 0.5f, py = x1 * s + 0.5f, pz = x2 * s + 0.5f;
    const float fx = __builtin_amdgcn_fractf(px);
    g.fwx[i] = side ? fx : 1.0f - fx;
    g.ffy[i] = __builtin_amdgcn_fractf(py); g.ffz[i] = __builtin_amdgcn_fractf(pz);
    const uint32_t c = (uint32_t)px + side, cy = (uint32_t)py, cz = (uint32_t)pz;
    const uint32_t hy0 = cy * pa, hy1 = hy0 + pa;
    const uint32_t hz0 = cz * pb, hz1 = hz0 + pb;
    if (i == 0) wait_vmcnt<kWaitAfterCoarse>();
    else wait_vmcnt<kWaitBetweenFine>();
    uint32_t off[4];           // byte offsets of the fp32 rows (y0z0, y1z0, y0z1, y1z1)
    if constexpr (kPre) {
      // sliced feed: the finest kSliceLevels levels (of pair 1's 12..15) arrive precomputed; its lanes ask for row 0 of
      // the table instead (all of them the SAME line: one look-up per instruction, no divergence) and the caller
      // overwrites those features
      const uint32_t keep = ((q >> 1) && i >= 4 - kSliceLevels) ? 0u : 0xFFFFFFFFu;
      off[0] = (base + ((c ^ (hy0 ^ hz0)) & mask) * 8u) & keep;
      off[1] = (base + ((c ^ (hy1 ^ hz0)) & mask) * 8u) & keep;
      off[2] = (base + ((c ^ (hy0 ^ hz1)) & mask) * 8u) & keep;
      off[3] = (base + ((c ^ (hy1 ^ hz1)) & mask) * 8u) & keep;
    } else if constexpr (kFineHashed) {       // every fine level of both pairs is hashed: xor-only index maths
      off[0] = base + ((c ^ (hy0 ^ hz0)) & mask) * 8u;
      off[1] = base + ((c ^ (hy1 ^ hz0)) & mask) * 8u;
      off[2] = base + ((c ^ (hy0 ^ hz1)) & mask) * 8u;
      off[3] = base + ((c ^ (hy1 ^ hz1)) & mask) * 8u;
    } else {
      const IndexTerms t = index_terms(hy0, hy1, hz0, hz1, rb.z, rb.w);
#pragma unroll
      for (int k = 0; k < 4; ++k) off[k] = base + t.row(c, k, mask) * 8u;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) off[k] = table_offset<kHalf>(off[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) g.f[i][k] = gather_at<kHalf>(rsrc, off[k]);
    keep_offsets(off[0], off[1], off[2], off[3]);
  }
}

template <bool kHalf = false, bool kPre = false>
__device__ __forceinline__ void issue_gathers(const LevelRec* __restrict__ my_recs, const bool (&all_hashed)[4],
                                              __amdgpu_buffer_rsrc_t rsrc, float x0, float x1, float x2, Gathered& g) {
  if constexpr (kPre) issue_gathers_impl<true, kHalf, true>(my_recs, rsrc, x0, x1, x2, g);   // (the host checks: fine levels hashed)
  else if (all_hashed[2] && all_hashed[3]) issue_gathers_impl<true, kHalf>(my_recs, rsrc, x0, x1, x2, g);
  else issue_gathers_impl<false, kHalf>(my_recs, rsrc, x0, x1, x2, g);
}

template <bool kHalf = false>
__device__ __forceinline__ f32x2 row2(const u32x2 v) {
  const unsigned bx = v[0], by = v[1];     // (scalars first: see the note on __builtin_bit_cast below)
  if constexpr (kHalf) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 h = __builtin_bit_cast(h2, bx);
    return f32x2{(float)h[0], (float)h[1]};
  } else {
    return f32x2{__uint_as_float(bx), __uint_as_float(by)};
  }
}

// trilinear blend: weight = (wx*wy)*wz, accumulated with fma - coarse levels in corner order 0..7, fine levels as
// (this side's corners in yz order) and then x side 0 + x side 1.
// out[s], s = 0..7 <-> feature 16*(s>>2) + 4q + (s&3).
template <bool kHalf = false>
__device__ __forceinline__ void blend(const Gathered& g, f32x4& lo, f32x4& hi) {
#pragma unroll
  for (int li = 0; li < 2; ++li) {
    const f32x2 wx = {1.0f - g.cfx[li], g.cfx[li]};
    const float wy0 = 1.0f - g.cfy[li], wz0 = 1.0f - g.cfz[li];
    const f32x2 a = wx * wy0, b = wx * g.cfy[li];                     // (wx*wy) for y side 0 / 1, both x sides
    const f32x2 w[4] = {a * wz0, b * wz0, a * g.cfz[li], b * g.cfz[li]};   // corners (0,1) (2,3) (4,5) (6,7)
    f32x2 acc = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const f32x2 wk = (k & 1) ? w[k >> 1].yy : w[k >> 1].xx;
      acc = __builtin_elementwise_fma(wk, row2<kHalf>(g.c[li][k]), acc);
    }
    lo[2 * li] = acc.x;
    lo[2 * li + 1] = acc.y;
  }
  f32x2 part[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 wy = {1.0f - g.ffy[i], g.ffy[i]};
    const f32x2 xy = wy * g.fwx[i];                                    // (wx*wy): y side 0 / 1 (product commutes)
    const f32x2 w0 = xy * (1.0f - g.ffz[i]), w1 = xy * g.ffz[i];       // corners (y0z0, y1z0), (y0z1, y1z1)
    f32x2 acc = {0.f, 0.f};
    acc = __builtin_elementwise_fma(w0.xx, row2<kHalf>(g.f[i][0]), acc);
    acc = __builtin_elementwise_fma(w0.yy, row2<kHalf>(g.f[i][1]), acc);
    acc = __builtin_elementwise_fma(w1.xx, row2<kHalf>(g.f[i][2]), acc);
    acc = __builtin_elementwise_fma(w1.yy, row2<kHalf>(g.f[i][3]), acc);
    part[i] = acc;
  }
  // v_permlane16_swap_b32 vdst, src: the odd 16-lane rows of vdst trade places with the even rows of src.  With
  // vdst = the partial of an even-lane level and src = the partial of an odd-lane level, afterwards BOTH registers of
  // every lane belong to that lane's own level: one is its own half, the other the partner's.
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int lv = t >> 1, ft = t & 1;
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(part[lv][ft]), __float_as_uint(part[2 + lv][ft]), false, false);
    const unsigned r0 = r[0], r1 = r[1];
    hi[t] = __uint_as_float(r0) + __uint_as_float(r1);      // = x side 0 + x side 1 in both lanes
  }
}

// (Round 1 had tried an x-split with EIGHT lanes per sample - twice the index maths per sample - and lost 11 % in
// the VALU-bound regime.  The pairing above keeps four lanes per sample and 32 loads per lane; only the fine levels'
// cell location is duplicated.)

// One MLP layer: out[mt] (N_MT output tiles) = W * in, K = 16 * N_G inputs.  in[g] is the B
// operand of k-steps 4g..4g+3.  The N_MT accumulator chains are interleaved (independent
// MFMAs back to back: the 16x16x4 f32 MFMA issues every 32 cycles but has a 40-cycle
// dependent latency); a single-tile layer splits K over two accumulators instead.
template <int N_MT, int N_G>
__device__ __forceinline__ void layer(const float4* __restrict__ w, int lane, const f32x4* in, f32x4* out) {
  if constexpr (N_MT == 1) {
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < N_G; g += 2) {
      __builtin_amdgcn_sched_barrier(0);
      const float4 w0 = w[g * 64 + lane], w1 = w[(g + 1) * 64 + lane];
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, in[g][0], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, in[g + 1][0], a1, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.y, in[g][1], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.y, in[g + 1][1], a1, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.z, in[g][2], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.z, in[g + 1][2], a1, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.w, in[g][3], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.w, in[g + 1][3], a1, 0, 0, 0);
    }
    out[0] = a0 + a1;
  } else {
    f32x4 acc[N_MT];
#pragma unroll
    for (int mt = 0; mt < N_MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < N_G; ++g) {
      __builtin_amdgcn_sched_barrier(0);   // keep weight reads next to their MFMAs (register pressure)
      float4 wv[N_MT];
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) wv[mt] = w[(mt * N_G + g) * 64 + lane];
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[mt].x, in[g][0], acc[mt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[mt].y, in[g][1], acc[mt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[mt].z, in[g][2], acc[mt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[mt].w, in[g][3], acc[mt], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < N_MT; ++mt) out[mt] = acc[mt];
  }
}

// ---- split-bf16 MLP ----------------------------------------------------------------------------------
// Packed weights (host, inr_*_pack_weights): per section [mt][step][hi|lo][lane][8 bf16]; the 8 values
// of lane (q, i) in step s are W[16mt + i][kidx(s, q, e)], e = 0..7, with
//   hidden / encoder inputs: kidx = 16*(2s + (e>>2)) + 4q + (e&3)   (= D register e&3 of output tile 2s + (e>>2))
// so the B operand of step s is registers {h[2s][0..3], h[2s+1][0..3]} of the previous layer, in place.
struct SplitB {
  uint4 hi, lo;   // 8 bf16 each
};

// bf16 head by truncation (v_perm_b32 packs the two high halves), remainder exactly in fp32, then truncated.
__device__ __forceinline__ void split2(float x0, float x1, uint32_t& hi, uint32_t& lo) {
  const uint32_t u0 = __float_as_uint(x0), u1 = __float_as_uint(x1);
  hi = __builtin_amdgcn_perm(u1, u0, 0x07060302u);
  const float l0 = x0 - __uint_as_float(u0 & 0xFFFF0000u);
  const float l1 = x1 - __uint_as_float(u1 & 0xFFFF0000u);
  lo = __builtin_amdgcn_perm(__float_as_uint(l1), __float_as_uint(l0), 0x07060302u);
}
__device__ __forceinline__ SplitB split8(const f32x4 a, const f32x4 b) {
  SplitB r;
  split2(a[0], a[1], r.hi.x, r.lo.x);
  split2(a[2], a[3], r.hi.y, r.lo.y);
  split2(b[0], b[1], r.hi.z, r.lo.z);
  split2(b[2], b[3], r.hi.w, r.lo.w);
  return r;
}
__device__ __forceinline__ f32x4 mfma_bf(const uint4 a, const uint4 b, const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// out[mt] = W * in over N_S steps of 32 inputs.  w: section base (uint4 = 8 bf16), fragment (mt, s, hl) at
// ((mt*N_S + s)*2 + hl)*64 + lane.  Independent accumulator chains are interleaved.
template <int N_MT, int N_S>
__device__ __forceinline__ void layer_bf(const uint4* __restrict__ w, int lane, const SplitB* in, f32x4* out) {
  if constexpr (N_MT == 1) {
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
#pragma unroll
    for (int st = 0; st < N_S; ++st) {
      __builtin_amdgcn_sched_barrier(0);
      const uint4 wh = w[(st * 2 + 0) * 64 + lane], wlo = w[(st * 2 + 1) * 64 + lane];
      a0 = mfma_bf(wh, in[st].hi, a0);
      a1 = mfma_bf(wlo, in[st].hi, a1);
      a2 = mfma_bf(wh, in[st].lo, a2);
    }
    out[0] = a0 + (a1 + a2);
  } else {
    f32x4 acc[N_MT];
#pragma unroll
    for (int mt = 0; mt < N_MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < N_S; ++st) {
      __builtin_amdgcn_sched_barrier(0);   // keep weight reads next to their MFMAs (register pressure)
      uint4 wh[N_MT], wlo[N_MT];
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) {
        wh[mt] = w[((mt * N_S + st) * 2 + 0) * 64 + lane];
        wlo[mt] = w[((mt * N_S + st) * 2 + 1) * 64 + lane];
      }
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) acc[mt] = mfma_bf(wh[mt], in[st].hi, acc[mt]);
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) acc[mt] = mfma_bf(wlo[mt], in[st].hi, acc[mt]);
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) acc[mt] = mfma_bf(wh[mt], in[st].lo, acc[mt]);
    }
#pragma unroll
    for (int mt = 0; mt < N_MT; ++mt) out[mt] = acc[mt];
  }
}

// Opt-in single-pass variant (kFast; upstream's `-O` numerics: fp16 MLP operands, fp32 accumulation): weights packed as
// fp16 in the head slots of the same fragment layout (pack_section_f16), activations rounded to fp16
// (v_cvt_pk_f16_f32, round to nearest even), ONE v_mfma_f32_16x16x32_f16 per (tile, step) instead of three bf16 passes,
// one conversion per activation pair instead of the head / remainder split.  2^-12 relative per operand: close to, but
// NOT, the fp32-class default.
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_f16x2(float a, float b) {
  const f32x2_t v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_t));
}
template <int N_MT, int N_S>
__device__ __forceinline__ void layer_h1(const uint4* __restrict__ w, int lane, const uint4* in, f32x4* out) {
  f32x4 acc[N_MT];
#pragma unroll
  for (int mt = 0; mt < N_MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < N_S; ++st) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mt = 0; mt < N_MT; ++mt)
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, w[((mt * N_S + st) * 2 + 0) * 64 + lane]),
                                                       __builtin_bit_cast(f16x8_t, in[st]), acc[mt], 0, 0, 0);
  }
#pragma unroll
  for (int mt = 0; mt < N_MT; ++mt) out[mt] = acc[mt];
}

// Layer entry points used by the kernels: `in` is N_G groups of 4 registers (N_G = K/16).
template <int N_MT, int N_G, bool kFast = false>
__device__ __forceinline__ void mlp_layer(const float4* __restrict__ wsec, int lane, const f32x4* in, f32x4* out) {
#if INR_MLP_FP32
  layer<N_MT, N_G>(wsec, lane, in, out);
#else
  if constexpr (kFast) {
    uint4 b[N_G / 2];
#pragma unroll
    for (int st = 0; st < N_G / 2; ++st)
      b[st] = uint4{pack_f16x2(in[2 * st][0], in[2 * st][1]), pack_f16x2(in[2 * st][2], in[2 * st][3]),
                    pack_f16x2(in[2 * st + 1][0], in[2 * st + 1][1]), pack_f16x2(in[2 * st + 1][2], in[2 * st + 1][3])};
    layer_h1<N_MT, N_G / 2>(reinterpret_cast<const uint4*>(wsec), lane, b, out);
  } else {
    SplitB b[N_G / 2];
#pragma unroll
    for (int st = 0; st < N_G / 2; ++st) b[st] = split8(in[2 * st], in[2 * st + 1]);
    layer_bf<N_MT, N_G / 2>(reinterpret_cast<const uint4*>(wsec), lane, b, out);
  }
#endif
}

// ---- two tiles through one layer (k_nerf_fwd_pair) -------------------------------------------------------------------
// layer_bf for tiles A and B at once: every (mt, step, hi|lo) weight fragment is read from LDS ONCE and feeds A's and
// B's MFMA back to back - two independent accumulator chains per output tile.  Per tile, the operands and their order
// are layer_bf's (per step hi.hi, lo.hi, hi.lo on that tile's own accumulator; a0 + (a1 + a2) for one output tile).
template <int N_MT, int N_S>
__device__ __forceinline__ void layer_bf2(const uint4* __restrict__ w, int lane, const SplitB* in_a, const SplitB* in_b,
                                          f32x4* out_a, f32x4* out_b) {
  if constexpr (N_MT == 1) {
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, b0 = a0, b1 = a0, b2 = a0;
#pragma unroll
    for (int st = 0; st < N_S; ++st) {
      __builtin_amdgcn_sched_barrier(0);
      const uint4 wh = w[(st * 2 + 0) * 64 + lane], wlo = w[(st * 2 + 1) * 64 + lane];
      a0 = mfma_bf(wh, in_a[st].hi, a0);
      b0 = mfma_bf(wh, in_b[st].hi, b0);
      a1 = mfma_bf(wlo, in_a[st].hi, a1);
      b1 = mfma_bf(wlo, in_b[st].hi, b1);
      a2 = mfma_bf(wh, in_a[st].lo, a2);
      b2 = mfma_bf(wh, in_b[st].lo, b2);
    }
    out_a[0] = a0 + (a1 + a2);
    out_b[0] = b0 + (b1 + b2);
  } else {
    f32x4 acc_a[N_MT], acc_b[N_MT];
#pragma unroll
    for (int mt = 0; mt < N_MT; ++mt) acc_a[mt] = acc_b[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < N_S; ++st) {
      __builtin_amdgcn_sched_barrier(0);   // keep weight reads next to their MFMAs (register pressure)
      uint4 wh[N_MT], wlo[N_MT];
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) {
        wh[mt] = w[((mt * N_S + st) * 2 + 0) * 64 + lane];
        wlo[mt] = w[((mt * N_S + st) * 2 + 1) * 64 + lane];
      }
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) {
        acc_a[mt] = mfma_bf(wh[mt], in_a[st].hi, acc_a[mt]);
        acc_b[mt] = mfma_bf(wh[mt], in_b[st].hi, acc_b[mt]);
      }
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) {
        acc_a[mt] = mfma_bf(wlo[mt], in_a[st].hi, acc_a[mt]);
        acc_b[mt] = mfma_bf(wlo[mt], in_b[st].hi, acc_b[mt]);
      }
#pragma unroll
      for (int mt = 0; mt < N_MT; ++mt) {
        acc_a[mt] = mfma_bf(wh[mt], in_a[st].lo, acc_a[mt]);
        acc_b[mt] = mfma_bf(wh[mt], in_b[st].lo, acc_b[mt]);
      }
    }
#pragma unroll
    for (int mt = 0; mt < N_MT; ++mt) {
      out_a[mt] = acc_a[mt];
      out_b[mt] = acc_b[mt];
    }
  }
}

// mlp_layer (default numerics) for two tiles.  (The exact-fp32 A/B library keeps one tile per layer call.)
// The split stays split8's two v_sub_f32 per pair of values.  A packed form - both remainders from one 2-vector
// subtraction, v_pk_add_f32 with neg: 64 VALU fewer per pair, the same bits - was measured beside this one and is NOT
// faster (profiles/r10_pair_mlp_bench.md): a packed f32 instruction next to MFMAs costs more than the two it replaces.
template <int N_MT, int N_G>
__device__ __forceinline__ void mlp_layer2(const float4* __restrict__ wsec, int lane, const f32x4* in_a, const f32x4* in_b,
                                           f32x4* out_a, f32x4* out_b) {
#if INR_MLP_FP32
  layer<N_MT, N_G>(wsec, lane, in_a, out_a);
  layer<N_MT, N_G>(wsec, lane, in_b, out_b);
#else
  SplitB a[N_G / 2], b[N_G / 2];
#pragma unroll
  for (int st = 0; st < N_G / 2; ++st) {
    a[st] = split8(in_a[2 * st], in_a[2 * st + 1]);
    b[st] = split8(in_b[2 * st], in_b[2 * st + 1]);
  }
  layer_bf2<N_MT, N_G / 2>(reinterpret_cast<const uint4*>(wsec), lane, a, b, out_a, out_b);
#endif
}

// Colour epilogue.  The last layer leaves the three pre-activations of sample j in registers 0..2 of its lane q = 0
// (rows 0..2 of D, both MFMA shapes).  Evaluating three sigmoids there costs three exp + three IEEE divisions - 49 VALU
// instructions, 6 of them transcendental - on a quarter of the lanes, and the exec mask saves no issue slot.  Two
// cross-row moves put channel c into lane q = c of the same sample instead:
//   v_permlane16_swap vdst = o[0], src = o[1]:  row 1 of vdst <- row 0 of src   (rows: 16-lane groups = q)
//   v_permlane32_swap vdst = that, src = o[2]:  rows 2, 3 of vdst <- rows 0, 1 of src
// and the SAME expression runs once for all three channels; lane q < 3 then owns channel q.  Same operations on the
// same values: the same bits.  (Lane q = 3 computes a value nobody reads.)
__device__ __forceinline__ float rgb_channel_of_lane(const f32x4 o) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(o[0]), __float_as_uint(o[1]), false, false);
  const unsigned a0 = a[0];
  const auto b = __builtin_amdgcn_permlane32_swap(a0, __float_as_uint(o[2]), false, false);
  const unsigned b0 = b[0];
  return __uint_as_float(b0);
}
__device__ __forceinline__ float sigmoid_rgb(float o) {
  return __frcp_rn(1.0f + __expf(-o));     // v_exp_f32 / v_rcp_f32: ~1e-7 relative
}

__device__ __forceinline__ float select4(int q, float a, float b, float c, float d) {
  return q == 0 ? a : (q == 1 ? b : (q == 2 ? c : d));
}

struct TileIn {
  float x0, x1, x2;   // x01
  float d0, d1, d2;
  bool oob;           // x01 left [0,1]: features are zero (upstream's flag_oob); x01 is then replaced by 0
};

// x01 = (x + bound) / (2 bound): a true IEEE division, as in the oracle.  (Replacing it by a multiplication
// with the exact reciprocal when 2*bound is a power of two - selected by a wave-uniform flag - measured 7 %
// SLOWER: the extra control flow in front of the gathers costs more than the ~30 instructions it saves.)
__device__ __forceinline__ float to_x01(float x, float bound, float rb, float) { return (x + bound) / rb; }

template <bool kDir>
__device__ __forceinline__ void load_tile_in(const float* __restrict__ x, const float* __restrict__ d, int64_t m,
                                             float bound, float rb, float rb_inv, TileIn& t) {
  t.x0 = to_x01(x[m * 3 + 0], bound, rb, rb_inv);
  t.x1 = to_x01(x[m * 3 + 1], bound, rb, rb_inv);
  t.x2 = to_x01(x[m * 3 + 2], bound, rb, rb_inv);
  t.oob = oob01(t.x0, t.x1, t.x2);
  if (t.oob) t.x0 = t.x1 = t.x2 = 0.0f;
  if constexpr (kDir) {
    t.d0 = d[m * 3]; t.d1 = d[m * 3 + 1]; t.d2 = d[m * 3 + 2];
  }
}

// Latency hiding is by wave-level parallelism, not by a per-wave software pipeline: a tile's 32 gathers
// per lane are all issued back to back (addresses first, then one wait) and while one wave of a SIMD
// runs its 60 MFMAs the other has its table reads in flight.  A per-wave double-buffered variant
// (next tile's gathers issued before this tile's MLP, 168 VGPRs) was built and measured twice: it is
// not faster (6.95 vs 6.81 ms at 8 waves/CU) because it enlarges the per-CU working set exactly like a
// higher occupancy does - see grid_for() - so it was removed.
// Workgroup b runs on XCD b % 8 (observed dispatch order, confirmed with HW_REG_XCC_ID; used for speed only - any
// placement gives the same results).  The sample stream is ray-major and rays are image-ordered, so a contiguous run of
// tiles is a compact region of space: the waves of an XCD sweep such runs together, which keeps the XCD's private 4 MB L2
// on one part of the hash table's working set instead of all of it.
// XCD-aware persistent schedule.  Every XCD gets the same number of tiles, but NOT one contiguous eighth of the stream
// (rounds 1 and most of 2 did that): equal sample counts are not equal work - a tile costs what its region of the
// scene costs in cache misses, and the frame is ray-ordered top to bottom - so the XCD with the expensive eighth set
// the kernel's time while the others idled (field kernel 5.53 -> 5.18 ms for 37 M samples once the eighths were
// interleaved, profiles/r02_NOTES.txt section 28).  The stream is cut into chunks of 2^kXcdChunkLog2 tiles dealt round
// robin to the XCDs (a chunk is still a compact run of patches: the XCD's private L2 keeps its locality); what is left
// after the last complete round of eight chunks is split into eighths as before, so the counts stay equal.  Launches
// with fewer than four rounds (training batches: random rays, no regional structure) keep the contiguous split.
constexpr int kXcdChunkLog2 = 10;
#ifndef INR_STEAL_SHIFT
#define INR_STEAL_SHIFT 1
#endif
constexpr int kStealRoundsShift = INR_STEAL_SHIFT;     // hybrid schedule: the last rounds >> shift rounds are drawn (TileWalk)
// kUnit: log2 of the tiles one schedule item stands for.  0: an item is a tile.  1 (the pair front end, k_nerf_fwd_pair):
// an item is a pair of consecutive tiles and the chunks, blocks and draws below halve in items, so that they stay the
// same runs of tiles - no pair straddles an XCD chunk or a cursor draw.
template <int kUnit = 0>
struct TileSchedT {
  static constexpr int kChunkLog2 = kXcdChunkLog2 - kUnit;
  int64_t lo, hi;      // hi: one past the last tile this wave may take
  int64_t first;       // first tile (contiguous split) or first XCD-local index (interleaved split)
  int64_t stride;      // distance between consecutive tiles / local indices of this wave
  int64_t main_local = 0, tail_base = 0;   // interleaved split: local indices below main_local map into the chunked part
  int64_t n_main = 0, tail = 0;            // tiles in complete rounds of eight chunks / behind them (interleaved split)
  int64_t static_local = 0;                // hybrid: local indices from here on are handed out by cursors (TileWalk)
  uint32_t xcd = 0;
  bool interleaved = false, hybrid = false;
  // local index u of XCD y -> tile; one past XCD y's last local index
  __device__ __forceinline__ int64_t tile_of(int y, int64_t u) const {
    if (u < main_local) return ((((u >> kChunkLog2) << 3) + y) << kChunkLog2) + (u & ((1 << kChunkLog2) - 1));
    return n_main + tail * y / 8 + (u - main_local);
  }
  __device__ __forceinline__ int64_t local_end(int y) const { return main_local + tail * (y + 1) / 8 - tail * y / 8; }
  __device__ __forceinline__ int64_t tile(int64_t i) const {
    if (interleaved) {
      const int64_t u = first + i * stride;
      if (u < main_local)
        return ((((u >> kChunkLog2) << 3) + xcd) << kChunkLog2) + (u & ((1 << kChunkLog2) - 1));
      return tail_base + (u - main_local);
    }
    return first + i * stride;
  }
};
using TileSched = TileSchedT<>;
template <int kUnit = 0>
__device__ __forceinline__ TileSchedT<kUnit> make_sched(int64_t n_tiles, int waves_per_block, bool steal = false) {
  constexpr int kChunkLog2 = TileSchedT<kUnit>::kChunkLog2;
  const int nb = gridDim.x, b = blockIdx.x;
  const int w = threadIdx.x >> 6;
  TileSchedT<kUnit> s;
  if (nb % 8 == 0) {
    const int xcd = b & 7, local = b >> 3, per = nb >> 3;
    const int64_t rounds = n_tiles >> (kChunkLog2 + 3);
    if (rounds >= 4) {
      const int64_t n_main = rounds << (kChunkLog2 + 3), tail = n_tiles - n_main;
      s.interleaved = true;
      s.xcd = (uint32_t)xcd;
      s.main_local = rounds << kChunkLog2;
      s.n_main = n_main;
      s.tail = tail;
      s.hybrid = steal;
      s.static_local = steal ? (rounds - max((int64_t)1, rounds >> kStealRoundsShift)) << kChunkLog2 : s.main_local;
      s.tail_base = n_main + tail * xcd / 8;
      s.lo = 0;
      s.hi = n_main + tail * (xcd + 1) / 8;
      s.first = (int64_t)local * waves_per_block + w;
      s.stride = (int64_t)per * waves_per_block;
      return s;
    }
    s.lo = n_tiles * xcd / 8;
    s.hi = n_tiles * (xcd + 1) / 8;
    s.first = s.lo + (int64_t)local * waves_per_block + w;
    s.stride = (int64_t)per * waves_per_block;
  } else {
    s.lo = 0;
    s.hi = n_tiles;
    s.first = (int64_t)b * waves_per_block + w;
    s.stride = (int64_t)nb * waves_per_block;
  }
  return s;
}

constexpr int kFieldThreads = 512;     // waves of a workgroup share one 40 KB weight image in LDS
constexpr int kGroupChunkLog2 = 6;     // dynamic group schedules: 2^k consecutive 16-ray groups per cursor and round
constexpr int kGroupDraw = 1;          // groups an owner takes per draw (must divide the chunk)
constexpr int kGroupPools = 4;                            // cursors per XCD, wave-owned groups (see GroupDraw)
// DYNAMIC schedule over 16-ray groups (kernels in which a wave or a workgroup owns a group for all its steps).  A group
// costs what its rays' sample counts and termination points make it cost (the ceiling rows of a frame: a dozen steps;
// the middle rows: seventy; an opaque group: two), so a fixed deal of ~20 groups per wave leaves the launch waiting for
// its unluckiest wave (round 2 measured 7.2 - 9.4 ms for the same work under four static deals).  Instead the owner of
// a group draws the next one from a cursor (zeroed by the caller): chunks of 2^kGroupChunkLog2 consecutive groups are
// dealt round robin to the XCDs - neighbouring patches still share an L2, every XCD sees every region of the frame -
// and inside an XCD groups go to whoever is free.  Same-address atomics are applied one after the other (~60 ns each):
// with one cursor per XCD an opaque frame of the wave-owned kernel - two steps per group, 2048 waves drawing - spent a
// quarter of its time queueing for it (1.22 vs 0.98 ms), so that kernel uses kGroupPools cursors per XCD, one per
// quarter of its workgroups (one chunk at a time each: the same window of the frame); the workgroup-owned kernel draws
// an eighth as often and is faster with ONE window per XCD (instance render 11.4 ms; four pools 12.0; the static deal
// 11.6).  Measured and not kept: 4 groups per draw (9.8 instead of 6.9 ms: the waves of an XCD then span four times the
// window and the L2 hit rate collapses), chunks of 16 / 256 / 1024 groups (6.9-7.0 / 7.1-7.5 / 7.2-8.0 ms), super-tiled
// pixel order (within noise).  Workgroup b runs on XCD b % 8 (observed; speed only - any placement gives the same results).
struct GroupDraw {
  unsigned long long* cursor;
  int owner, n_owner;
  __device__ __forceinline__ void init(unsigned long long* cursors, int pools) {
    const int n_xcd = (gridDim.x % 8 == 0) ? 8 : 1;
    const int n_pool = (gridDim.x % (8 * pools) == 0) ? pools : 1;
    const int xcd = (n_xcd == 8) ? (int)(blockIdx.x & 7) : 0;
    const int pool = (n_pool > 1) ? (int)((blockIdx.x >> 3) % pools) : 0;
    owner = pool * n_xcd + xcd;
    n_owner = n_pool * n_xcd;
    cursor = cursors + owner;
  }
  __device__ __forceinline__ int64_t group_of(uint32_t u) const {
    const int64_t chunk = (int64_t)(u >> kGroupChunkLog2) * n_owner + owner;
    return (chunk << kGroupChunkLog2) + (u & ((1u << kGroupChunkLog2) - 1u));
  }
  // called by ONE lane: the first of the kGroupDraw consecutive groups it now owns
  __device__ __forceinline__ int64_t draw() const { return group_of((uint32_t)atomicAdd(cursor, (unsigned long long)kGroupDraw)); }
};
// HYBRID schedule of the big field launches (frames): equal shares per XCD are equal WORK only while the eight XCDs
// run at the same speed, and on some boxes they do not - the same build, the same frame: 4.6 ms on one call, 5.1 ms on
// another, the trained scene 11.6 against 15.0 ms, while the kernels that draw their work (k_nerf_render,
// k_instance_render) and the ones that are not bound by the memory path (-O numerics) read the same on both
// (profiles/r03_NOTES.txt 21): with a static deal the launch waits for its slowest XCD.  So the second half of the
// rounds (and the ragged tail) is not dealt but DRAWN: every XCD's part of it sits behind kStealPools cursors
// (blocks of 64 local tiles dealt round robin to the pools, kStealDraw tiles per draw, the next draw in flight while
// the current tiles are evaluated), a wave draws from the cursor of its own XCD and pool, and when that runs dry it
// looks at all cursors at once (one 256-byte load) and moves to the first live one - its XCD's other pools first, then
// the next XCD's.  A fast XCD finishes its own part early and takes over what a slow one has left; with equal XCDs
// the drawn part is the same tiles in the same windows as before.  Cursors are zeroed by the launcher; nullptr (all
// other launches) is the static schedule.  Any order gives the same results: a tile's outputs depend on nothing else.
// Measured (view 0, 37 M samples, tools/field_probe.py on the profiling builds of tools/build_probe.py): static deal
// 5.12 ms, a quarter / half / all of the rounds drawn 4.88 / 4.85 / 4.91 ms; with one XCD made ~64 % slower
// (s_sleep per tile) 8.51 / 6.35 / 5.17 / 5.23 ms - half it is (kStealRoundsShift = 1).
constexpr int kStealPools = 4, kStealOwners = 8 * kStealPools, kStealDraw = 4, kStealBlockLog2 = 6;
template <int kUnit = 0>
struct TileWalkT {
  static constexpr int kBlockLog2 = kStealBlockLog2 - kUnit, kDraw = kStealDraw >> kUnit;     // in items (TileSchedT)
  TileSchedT<kUnit> s;
  unsigned long long* cur;
  int lane, own, owner, sub;
  int64_t it, k_base;
  unsigned long long raw_next;           // the draw in flight (lane 0), not looked at until it is needed
  bool dyn;
  __device__ __forceinline__ void init(const TileSchedT<kUnit>& sched, unsigned long long* cursors) {
    s = sched; cur = cursors; lane = threadIdx.x & 63; it = 0; dyn = false; sub = kDraw; k_base = 0; raw_next = 0;
    own = owner = (int)(((blockIdx.x >> 3) % kStealPools) * 8 + (blockIdx.x & 7));
    if (!cursors) s.hybrid = false;
    if (!s.hybrid) s.static_local = s.main_local;
  }
  // owner o = pool * 8 + xcd: number of cursor positions that map to local indices below the XCD's end (a multiple of
  // the block), and the local index of position k
  __device__ __forceinline__ int64_t pool_len(int o) const {
    const int64_t nb = (s.local_end(o & 7) - s.static_local + (1 << kBlockLog2) - 1) >> kBlockLog2;
    const int p = o >> 3;
    return nb > p ? ((nb - p + kStealPools - 1) / kStealPools) << kBlockLog2 : 0;
  }
  __device__ __forceinline__ int64_t local_of(int o, int64_t k) const {
    return s.static_local + ((((k >> kBlockLog2) * kStealPools) + (o >> 3)) << kBlockLog2) +
           (k & ((1 << kBlockLog2) - 1));
  }
  __device__ __forceinline__ unsigned long long issue(int o) const {
    unsigned long long v = 0;
    if (lane == 0) v = atomicAdd(cur + o, (unsigned long long)kDraw);
    return v;
  }
  __device__ __forceinline__ static int64_t uniform(unsigned long long v) {
    return (int64_t)(((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)v));
  }
  // first live owner in this wave's order (own XCD's pools, then the following XCDs'), -1: every cursor has run dry
  __device__ __forceinline__ int scan() const {
    bool live = false;
    if (lane < kStealOwners) live = (int64_t)__hip_atomic_load(cur + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < pool_len(lane);
    const uint32_t mask = (uint32_t)__ballot(live);
    for (int i = 0; i < kStealOwners; ++i) {
      const int o = (((own >> 3) + i) % kStealPools) * 8 + (((own & 7) + i / kStealPools) & 7);
      if ((mask >> o) & 1u) return o;
    }
    return -1;
  }
  // the wave's next tile, -1 when there is none
  __device__ __forceinline__ int64_t next() {
    if (!dyn) {
      if (!s.hybrid) {
        const int64_t t = s.tile(it++);
        return t < s.hi ? t : -1;
      }
      const int64_t u = s.first + (it++) * s.stride;
      if (u < s.static_local) return s.tile_of((int)s.xcd, u);
      dyn = true;
      raw_next = issue(owner);
    }
    for (;;) {
      if (sub < kDraw) {
        const int64_t u = local_of(owner, k_base + sub);
        ++sub;
        if (u < s.local_end(owner & 7)) return s.tile_of(owner & 7, u);
        continue;                                          // behind the ragged end of the XCD's part
      }
      int64_t k = uniform(raw_next);
      while (k >= pool_len(owner)) {
        const int o = scan();
        if (o < 0) return -1;
        owner = o;
        k = uniform(issue(owner));
      }
      k_base = k;
      sub = 0;
      raw_next = issue(owner);
    }
  }
};
using TileWalk = TileWalkT<>;
constexpr int kFieldMinWaves = 2;      // __launch_bounds__ second argument: <= 128 VGPRs

// kTable: fused-frame fast path - x is already normalised to [0,1] by the march writer and the direction
// encoding comes from a per-ray SH table (shq[ray][q] = this lane's four components) via a per-sample ray id:
// ~100 VALU instructions per tile less than dividing and evaluating 16 polynomials in every lane.
__device__ __forceinline__ f32x4 load4(const float* p) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  return f32x4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void store4(float* p, f32x4 v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ f32x4 mask4(f32x4 g, f32x4 h) {
  return f32x4{h[0] > 0.f ? g[0] : 0.f, h[1] > 0.f ? g[1] : 0.f, h[2] > 0.f ? g[2] : 0.f, h[3] > 0.f ? g[3] : 0.f};
}

// kSave (training) 1: activations the backward needs, row-major - enc [M,32], h1 [M,64], so [M,16] (raw sigma-net
// output: density logit + 15 geo features), cin [M,32] (colour-net input in weight-column order: 16 SH, 15 geo, 0),
// c1, c2 [M,64]; 2: enc only (k_nerf_head_bwd recomputes the rest).
struct NerfSave {
  float *enc, *h1, *so, *cin, *c1, *c2;
};

// kPre (table feed only; round 5, sliced frame path): the three FINEST levels (13..15, fine slots of lanes q = 2, 3) were
// evaluated by k_grid_fine_slices; `d` (unused by the table feed) then points to their features, float2 [3][m_pad],
// m_pad = M rounded up to 32; lanes q = 2, 3 read theirs from there and gather level 12 themselves.
// kRec (table feed only, not with kPre; records feed of the frame path): `x` is the [M] array of t of the records
// writer and `shq` the per-ray rows of k_ray_table_q - kRayRowVec float4 per ray: the four SH rows, then the ray's
// origin and direction.  A lane rebuilds its sample's x01 with the marcher's own operations (sample_pos.h; the host
// admits power-of-two 2*bound only): 8 instead of 16 bytes read per sample, and the rows of a ray are shared by its
// ~50 samples and the eight waves of a CU (L1 hits).  Everything behind the coordinates is the table feed's.
constexpr int kRayRowVec = INR_RAY_TABLE_FLOATS / 4;
template <bool kColor, bool kTable = false, int kSave = 0, bool kHalf = false, bool kFast = false, bool kPre = false,
          bool kRec = false>
__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_nerf_fwd(const float* __restrict__ x, const float* __restrict__ d,
                                                               int64_t M, const int32_t* __restrict__ n_dev, float bound,
                                                               const float2* __restrict__ emb, uint32_t emb_bytes, GridDesc G,
                                                               const float4* __restrict__ packed, float density_scale,
                                                               float* __restrict__ sigma, float* __restrict__ rgb,
                                                               float* __restrict__ geo, const int32_t* __restrict__ ray_ids,
                                                               const float4* __restrict__ shq, NerfSave sv,
                                                               unsigned long long* __restrict__ steal) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  INR_PROBE_PROLOGUE();
  // the field kernel's waves outrank whatever shares the CU with them (FramePipeline: the next view's marchers run
  // at priority 0 and take the issue slots this kernel leaves free); alone on the chip it changes nothing
  __builtin_amdgcn_s_setprio(3);
  constexpr int kStage = (kColor ? kNerfFloats : kCol0) / 4;
  for (int i = threadIdx.x; i < kStage; i += kFieldThreads) wl[i] = packed[i];
  LevelRec* recs = reinterpret_cast<LevelRec*>(wl + kStage);
  stage_level_recs(G, recs);
  __syncthreads();

  constexpr int kWaves = kFieldThreads / 64;
  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
  int64_t n = M;
  if (n_dev) n = min((int64_t)*n_dev, M);
  const int64_t n_tiles = (n + 15) >> 4;
  const float rb = 2.0f * bound;
  const float rb_inv = 0.0f;
  INR_PROBE_SCHEDULE(steal);
  TileWalk walk;
  walk.init(make_sched(n_tiles, kWaves, steal != nullptr), steal);

  const bool all_hashed[4] = {slot_all_hashed(G, 0), slot_all_hashed(G, 1), slot_all_hashed(G, 2), slot_all_hashed(G, 3)};
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)emb, 0, (int)emb_bytes, 0x00020000);

  // (Requesting the NEXT tile's coordinates and ray id one tile ahead - so that neither the gather addresses nor the
  //  dependent direction-table load wait for a fresh trip through the memory system - was measured twice, in round 1
  //  on the plain feed and in round 2 on this table feed: 0 % and -2 %; removed.)
  for (int64_t tile = walk.next(); tile >= 0; tile = walk.next()) {
    INR_PROBE_TILE();
    const int64_t m = tile * 16 + j;
    const bool valid = m < n;
    TileIn me;
    f32x4 sh_in = {0.f, 0.f, 0.f, 0.f};
    if constexpr (kRec) {
      static_assert(!kRec || (kTable && !kPre), "the records feed is a variant of the fused table feed");
      const int64_t mm = valid ? m : n - 1;
      const float t = x[mm];
      const float4* row = shq + (int64_t)ray_ids[mm] * kRayRowVec;
      const float4 t4 = row[q], o4 = row[4], d4 = row[5];
      sh_in = f32x4{t4.x, t4.y, t4.z, t4.w};
      const float rb_rcp = 1.0f / rb;        // exact: rb is a power of two
      me.x0 = sample_x01_pow2(sample_pos(o4.x, t, d4.x, bound), bound, rb_rcp);
      me.x1 = sample_x01_pow2(sample_pos(o4.y, t, d4.y, bound), bound, rb_rcp);
      me.x2 = sample_x01_pow2(sample_pos(o4.z, t, d4.z, bound), bound, rb_rcp);
    } else if constexpr (kTable) {
      const int64_t mm = valid ? m : n - 1;
      me.x0 = x[mm * 3 + 0]; me.x1 = x[mm * 3 + 1]; me.x2 = x[mm * 3 + 2];
      const float4 t4 = shq[(int64_t)ray_ids[mm] * 4 + q];
      sh_in = f32x4{t4.x, t4.y, t4.z, t4.w};
    } else {
      load_tile_in<kColor>(x, d, valid ? m : n - 1, bound, rb, rb_inv, me);
    }

    f32x4 enc[2];
    {
      Gathered g;
      uint32_t rec_off = (uint32_t)q * 4u * (uint32_t)sizeof(LevelRec);
      asm volatile("" : "+v"(rec_off));    // opaque per tile: keeps the records in LDS, not hoisted into VGPRs
      typedef float v2f __attribute__((ext_vector_type(2)));
      v2f fine_a = {0.f, 0.f}, fine_b = {0.f, 0.f};
      if constexpr (kPre) {                // lane q = 2: levels 12 (own gathers), 13 (slice 0); q = 3: 14, 15 (slices 1, 2)
        static_assert(!kPre || kTable, "the sliced feed is a variant of the table feed");
        static_assert(kSliceLevels == 3, "lane map below");
        const v2f* pre = reinterpret_cast<const v2f*>(d);
        const int64_t m_pad = (M + 31) & ~(int64_t)31, mm = valid ? m : n - 1;
        const int sl = (q & 1) ? 1 : 0;    // (lanes q = 0, 1 load the same rows: their values are not used)
        fine_a = __builtin_nontemporal_load(pre + (int64_t)sl * m_pad + mm);
        fine_b = __builtin_nontemporal_load(pre + (int64_t)(sl + 1) * m_pad + mm);
      }
      issue_gathers<kHalf, kPre>(reinterpret_cast<const LevelRec*>(reinterpret_cast<const char*>(recs) + rec_off), all_hashed,
                                 rsrc, me.x0, me.x1, me.x2, g);
      __builtin_amdgcn_sched_barrier(0);   // all 32 gathers in flight before the first blend waits
      blend<kHalf>(g, enc[0], enc[1]);
      if constexpr (kPre) {
        if (q == 2) enc[1] = f32x4{enc[1][0], enc[1][1], fine_a.x, fine_a.y};          // level 12 gathered here, 13 precomputed
        else if (q == 3) enc[1] = f32x4{fine_a.x, fine_a.y, fine_b.x, fine_b.y};       // 14, 15
      }
    }
    if constexpr (!kTable) {               // the table feed comes from the marcher, which clamps to the volume
      if (me.oob) enc[0] = enc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    INR_PROBE_AFTER_GATHER();

    f32x4 h1[4];
    mlp_layer<4, 2, kFast>(wl + kSig0 / 4, lane, enc, h1);
#pragma unroll
    for (int t = 0; t < 4; ++t) h1[t] = relu4(h1[t]);
    f32x4 h2[1];
    mlp_layer<1, 4, kFast>(wl + kSig1 / 4, lane, h1, h2);      // row 0 = raw density, rows 1..15 = geo features

    if (valid) {
      if (q == 0) sigma[m] = __expf(h2[0][0]) * density_scale;
      if (INR_PROBE_GEO_IS_OUTPUT && geo) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * q + r;
          if (row >= 1) geo[m * 15 + row - 1] = h2[0][r];
        }
      }
    }

    if constexpr (kColor) {
      f32x4 cin[2];
      if constexpr (kTable) {
        cin[0] = sh_in;
      } else {
        float sh[16];
        sh4(me.d0, me.d1, me.d2, sh);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) cin[0][ks] = select4(q, sh[4 * ks], sh[4 * ks + 1], sh[4 * ks + 2], sh[4 * ks + 3]);
      }
      cin[1] = h2[0];                                 // k-slot (q, r) = sigma-net row 4q+r (row 0 has zero weight)
      f32x4 c1[4], c2[4], o[1];
      mlp_layer<4, 2, kFast>(wl + kCol0 / 4, lane, cin, c1);
#pragma unroll
      for (int t = 0; t < 4; ++t) c1[t] = relu4(c1[t]);
      mlp_layer<4, 4, kFast>(wl + kCol1 / 4, lane, c1, c2);
#pragma unroll
      for (int t = 0; t < 4; ++t) c2[t] = relu4(c2[t]);
      mlp_layer<1, 4, kFast>(wl + kCol2 / 4, lane, c2, o);
      if constexpr (kSave == 2) {          // k_nerf_head_bwd recomputes everything else from the encoder output
        if (valid) {
#pragma unroll
          for (int t = 0; t < 2; ++t) store4(sv.enc + m * 32 + 16 * t + 4 * q, enc[t]);
        }
      }
      if constexpr (kSave == 1) {
        if (valid) {
#pragma unroll
          for (int t = 0; t < 2; ++t) store4(sv.enc + m * 32 + 16 * t + 4 * q, enc[t]);
          store4(sv.so + m * 16 + 4 * q, h2[0]);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            store4(sv.h1 + m * 64 + 16 * t + 4 * q, h1[t]);
            store4(sv.c1 + m * 64 + 16 * t + 4 * q, c1[t]);
            store4(sv.c2 + m * 64 + 16 * t + 4 * q, c2[t]);
          }
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) sv.cin[m * 32 + 4 * ks + q] = cin[0][ks];      // SH component 4ks+q
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 4 * q + r;                                                   // sigma-net output row
            sv.cin[m * 32 + (row >= 1 ? 15 + row : 31)] = row >= 1 ? h2[0][r] : 0.f;       // geo row-1 | pad column
          }
        }
      }
      const float ch = sigmoid_rgb(rgb_channel_of_lane(o[0]));   // lane q < 3: channel q of sample j
      if (valid && q < 3) rgb[m * 3 + q] = ch;
    }
  }
  INR_PROBE_EPILOGUE();
}

// ---- pair front end of the frame kernel: two tiles per gather pass, two lanes per sample ----------------------------
// Consecutive tiles of the patch-interleaved sample stream are consecutive steps of the same 16 rays, one dt apart, and
// touch many of the same 128-byte lines of the table - but k_nerf_fwd asks for them in separate instructions, and a line
// touched by two instructions is looked up twice (see the note on the lane-paired gather above).  Here a wave encodes
// the 32 samples of tiles (2p, 2p+1) in ONE instruction stream and then runs the MLP of k_nerf_fwd on both tiles in ONE
// pass over the weights (pair_mlp / mlp_layer2: every weight fragment is read from LDS once per pair and feeds tile A's
// and tile B's MFMA back to back; per tile the operations and their order are k_nerf_fwd's).  Per pair in the hot loop:
// 52 LDS reads instead of 92, 60 s_waitcnt instead of 95, the same 120 MFMAs; frame loop +1.5 %
// (profiles/r10_pair_mlp_bench.md, r10_pair_mlp_isa.md).
// tools/pair_line_model.py counts the distinct lines per instruction both ways on the bench geometry: 0.73-0.78.
// Measured (profiles/r09_pair_gather_bench.md): L1 accesses fall by 5 % only, but the L1's read requests to the L2 by
// 21 % and the waves' wait cycles by a third - the second tile finds its lines while they are still there.
// Encoder lane map: lane = 32 h + 16 s + j - tile h of the pair, sample j, s in {0, 1}.
//   coarse: lane s owns levels {0,1,4,5} (s = 0) or {2,3,6,7} (s = 1), eight corners each, blended in corner order;
//   fine:   lane s fetches x side s of ALL eight levels 8..15, four yz corners each, blends its side in yz order, and
//           the sides meet by v_permlane16_swap + add: lane s = 0 ends with levels {8,9,12,13}, s = 1 with {10,11,14,15}.
// 64 gathers per lane and pair - 32 per tile as before - but every fine instruction now covers 32 samples x both x sides
// of one level and every coarse instruction 32 samples x two levels; a lane locates 12 cells per pair instead of 2 x 6.
// Every operation of a (sample, level) and its order are k_nerf_fwd's: the results are the same bits.
// Hand-over: rows 0/1 (lanes 0..31) hold what lanes q = 0, 1 of tile A need; one v_permlane32_swap per register on the
// eight features of levels {4,5,12,13} / {6,7,14,15} (vdst = the register of levels {0,1,8,9} / {2,3,10,11}) moves tile
// A's to rows 2/3 and brings tile B's rows to the front: afterwards vdst is tile A's and src tile B's encoding in the
// MLP's layout (lane q owns levels {2q, 2q+1, 8+2q, 9+2q}).
// The fine levels are hashed for every launch that gets here (the host checks), so their constants are the primes and
// three wave-uniform words per level straight from the kernel arguments - no LDS record reads for them.
// Staging: 32 coarse + 16 fine gathers go out, the coarse levels are blended under those fine loads, then the other 16
// fine gathers, then the fine blend - at most 48 rows (96 registers) are held at once.  All 64 rows held until one
// blend at the end needs 242 VGPRs: two such waves fill a SIMD's 512 registers, the next view's marchers find no room
// on any CU and the frame loop LOSES 1 % although the kernel itself is 14 % faster; this form needs 196 and leaves the
// marchers the wave per SIMD they had.  Waits (INR_PAIR_WAIT_*, as in issue_gathers_impl) swept again for this form:
// 16 / 8 here; 8 / 4, 32 / 16, 16 / 4 and none are 0.4-1.2 % slower (profiles/r09_pair_gather_bench.md).
// Where levels 0..3 are all dense (the bench table: 0..4) the coarse slots 0 and 1 take issue_coarse_pair_dense: 24
// coarse gather instructions instead of 32, 56 per pair instead of 64; the waits above were not swept again for it.
#ifndef INR_PAIR_WAIT_COARSE
#define INR_PAIR_WAIT_COARSE 16
#endif
#ifndef INR_PAIR_WAIT_FINE
#define INR_PAIR_WAIT_FINE 8
#endif
constexpr int kPairWaitAfterCoarse = INR_PAIR_WAIT_COARSE;      // loads still in flight when the first fine level goes out
constexpr int kPairWaitBetweenFine = INR_PAIR_WAIT_FINE;        // ... and when each later fine level goes out
struct GatheredPair {
  u32x2 c[4][8];      // coarse: raw rows [slot][corner]; slot c is level 4 (c >> 1) + 2 s + (c & 1)
  u32x2 f[8][4];      // fine: this lane's x side of level 8 + i, [i][yz corner]
  float cfx[4], cfy[4], cfz[4];
  float fwx[8], ffy[8], ffz[8];
};

// my_recs: the records of levels 2 s, 2 s + 1 (q = s); those of levels 4 + 2 s, 5 + 2 s (q = 2 + s) lie 8 records on
__device__ __forceinline__ void issue_coarse_pair(const LevelRec* __restrict__ my_recs, __amdgpu_buffer_rsrc_t rsrc, float x0,
                                                  float x1, float x2, GatheredPair& g) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const LevelRec* rec = my_recs + (c >> 1) * 8 + (c & 1);
    const uint4 ra = rec->a;
    const float s = __uint_as_float(ra.x);
    const uint32_t base = ra.y, pa = ra.z, pb = ra.w;
    const uint4 rb = rec->b;
    const uint32_t mask = rb.x;
    const float px = x0 * s + 0.5f, py = x1 * s + 0.5f, pz = x2 * s + 0.5f;   // mul, add: not fused
    g.cfx[c] = __builtin_amdgcn_fractf(px); g.cfy[c] = __builtin_amdgcn_fractf(py); g.cfz[c] = __builtin_amdgcn_fractf(pz);
    const uint32_t cx = (uint32_t)px, cy = (uint32_t)py, cz = (uint32_t)pz;
    const uint32_t hy0 = cy * pa, hy1 = hy0 + pa;
    const uint32_t hz0 = cz * pb, hz1 = hz0 + pb;
    const IndexTerms t = index_terms(hy0, hy1, hz0, hz1, rb.z, rb.w);
    uint32_t off[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) off[k] = base + t.row(cx + (k & 1), k >> 1, mask) * 8u;
#pragma unroll
    for (int k = 0; k < 8; ++k) g.c[c][k] = gather_at(rsrc, off[k]);
    keep_offsets(off[0], off[1], off[2], off[3]);
    keep_offsets(off[4], off[5], off[6], off[7]);
  }
}

// Dense x-pairs for the coarse slots 0 and 1 (levels {0 | 2} and {1 | 3}); the host takes it when all four are dense.
// On a dense level row(cx + 1) = row(cx) + 1 and nothing wraps (mask all ones), so the two x-neighbour rows of a yz
// corner come in ONE 16-byte load at 8-byte alignment: four offsets and four instructions per level instead of eight,
// row = cx + hy + hz without the dense/hashed lane masks of index_terms.  The halves are corners k and k + 1 of
// blend_coarse_pair.  Slots 2 and 3 (levels 4..7) mix dense and hashed lanes and stay as they are.  Same rows, same
// weights, same corner order: the same bits.  Measured (tools/micro/coarse_row_bench.hip, profiles/r12_coarse_rows_*.md):
// the vector memory path prices a 16-byte lane-load like an 8-byte one (18.9 against 35.5 clk per wave and row pair);
// 60 VALU fewer per pair; field launch 4.05 -> 3.94 ms inside the view loop, frame loop +2.5 %.
// Built beside it, measured and left out: level 0 read from a copy in the launch's idle LDS by the s = 0 lanes of slot 0.
// A gather instruction with half its lanes active costs what it costs with all of them (33.0 against 35.5 clk), so the
// s = 1 lanes' level 2 keeps slot 0's instructions in the texture path at full price: frame loop -0.4 % alone, and +1.8 %
// together with the x-pairs, which alone give +2.5 %.
typedef unsigned int u32x4 __attribute__((__vector_size__(4 * sizeof(unsigned int))));
__device__ __forceinline__ void issue_coarse_pair_dense(const LevelRec* __restrict__ my_recs, __amdgpu_buffer_rsrc_t rsrc,
                                                        float x0, float x1, float x2, GatheredPair& g) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const LevelRec* rec = my_recs + (c >> 1) * 8 + (c & 1);
    const uint4 ra = rec->a;
    const float s = __uint_as_float(ra.x);
    const uint32_t base = ra.y, pa = ra.z, pb = ra.w;
    const float px = x0 * s + 0.5f, py = x1 * s + 0.5f, pz = x2 * s + 0.5f;   // mul, add: not fused
    g.cfx[c] = __builtin_amdgcn_fractf(px); g.cfy[c] = __builtin_amdgcn_fractf(py); g.cfz[c] = __builtin_amdgcn_fractf(pz);
    const uint32_t cx = (uint32_t)px, cy = (uint32_t)py, cz = (uint32_t)pz;
    const uint32_t hy0 = cy * pa, hy1 = hy0 + pa;
    const uint32_t hz0 = cz * pb, hz1 = hz0 + pb;
    if (c < 2) {
      uint32_t off[4];           // byte offsets of the row pairs (y0z0, y1z0, y0z1, y1z1)
      off[0] = base + (cx + (hy0 + hz0)) * 8u;
      off[1] = base + (cx + (hy1 + hz0)) * 8u;
      off[2] = base + (cx + (hy0 + hz1)) * 8u;
      off[3] = base + (cx + (hy1 + hz1)) * 8u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off[k], 0, 0);
        g.c[c][2 * k] = u32x2{v[0], v[1]};
        g.c[c][2 * k + 1] = u32x2{v[2], v[3]};
      }
      keep_offsets(off[0], off[1], off[2], off[3]);
    } else {
      const uint4 rb = rec->b;
      const uint32_t mask = rb.x;
      const IndexTerms t = index_terms(hy0, hy1, hz0, hz1, rb.z, rb.w);
      uint32_t off[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) off[k] = base + t.row(cx + (k & 1), k >> 1, mask) * 8u;
#pragma unroll
      for (int k = 0; k < 8; ++k) g.c[c][k] = gather_at(rsrc, off[k]);
      keep_offsets(off[0], off[1], off[2], off[3]);
      keep_offsets(off[4], off[5], off[6], off[7]);
    }
  }
}

// fine levels 8 + kFirst .. 8 + kFirst + 3
template <int kFirst>
__device__ __forceinline__ void issue_fine_pair(const GridDesc& G, __amdgpu_buffer_rsrc_t rsrc, uint32_t side, float x0, float x1,
                                                float x2, GatheredPair& g) {
#pragma unroll
  for (int i = kFirst; i < kFirst + 4; ++i) {
    const float s = G.scales[8 + i];
    const uint32_t base = G.offsets[8 + i] * 8u, mask = G.mask[8 + i];
    const uint32_t pa = 2654435761u, pb = 805459861u;
    const float px = x0 * s + 0.5f, py = x1 * s + 0.5f, pz = x2 * s + 0.5f;
    const float fx = __builtin_amdgcn_fractf(px);
    g.fwx[i] = side ? fx : 1.0f - fx;
    g.ffy[i] = __builtin_amdgcn_fractf(py); g.ffz[i] = __builtin_amdgcn_fractf(pz);
    const uint32_t c = (uint32_t)px + side, cy = (uint32_t)py, cz = (uint32_t)pz;
    const uint32_t hy0 = cy * pa, hy1 = hy0 + pa;
    const uint32_t hz0 = cz * pb, hz1 = hz0 + pb;
    if (i == 0) wait_vmcnt<kPairWaitAfterCoarse>();
    else wait_vmcnt<kPairWaitBetweenFine>();
    uint32_t off[4];           // byte offsets of the rows (y0z0, y1z0, y0z1, y1z1)
    off[0] = base + ((c ^ (hy0 ^ hz0)) & mask) * 8u;
    off[1] = base + ((c ^ (hy1 ^ hz0)) & mask) * 8u;
    off[2] = base + ((c ^ (hy0 ^ hz1)) & mask) * 8u;
    off[3] = base + ((c ^ (hy1 ^ hz1)) & mask) * 8u;
#pragma unroll
    for (int k = 0; k < 4; ++k) g.f[i][k] = gather_at(rsrc, off[k]);
    keep_offsets(off[0], off[1], off[2], off[3]);
  }
}

// p[0], p[1]: this lane's features of levels {2s, 2s+1}, {8+2s, 9+2s} - enc[0], enc[1] of MLP lane q = s;
// r[0], r[1]: of levels {4+2s, 5+2s}, {12+2s, 13+2s} - those of MLP lane q = 2 + s.  Operations: blend()'s.
__device__ __forceinline__ void blend_coarse_pair(const GatheredPair& g, f32x4 (&p)[2], f32x4 (&r)[2]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x2 wx = {1.0f - g.cfx[c], g.cfx[c]};
    const float wy0 = 1.0f - g.cfy[c], wz0 = 1.0f - g.cfz[c];
    const f32x2 a = wx * wy0, b = wx * g.cfy[c];
    const f32x2 w[4] = {a * wz0, b * wz0, a * g.cfz[c], b * g.cfz[c]};
    f32x2 acc = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const f32x2 wk = (k & 1) ? w[k >> 1].yy : w[k >> 1].xx;
      acc = __builtin_elementwise_fma(wk, row2(g.c[c][k]), acc);
    }
    f32x4& out = (c >> 1) ? r[0] : p[0];
    out[2 * (c & 1)] = acc.x;
    out[2 * (c & 1) + 1] = acc.y;
  }
}
__device__ __forceinline__ void blend_fine_pair(const GatheredPair& g, f32x4 (&p)[2], f32x4 (&r)[2]) {
  f32x2 part[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f32x2 wy = {1.0f - g.ffy[i], g.ffy[i]};
    const f32x2 xy = wy * g.fwx[i];
    const f32x2 w0 = xy * (1.0f - g.ffz[i]), w1 = xy * g.ffz[i];
    f32x2 acc = {0.f, 0.f};
    acc = __builtin_elementwise_fma(w0.xx, row2(g.f[i][0]), acc);
    acc = __builtin_elementwise_fma(w0.yy, row2(g.f[i][1]), acc);
    acc = __builtin_elementwise_fma(w1.xx, row2(g.f[i][2]), acc);
    acc = __builtin_elementwise_fma(w1.yy, row2(g.f[i][3]), acc);
    part[i] = acc;
  }
  // as in blend(): vdst = the partial of a level the s = 0 lanes end up with, src = of one the s = 1 lanes end up with
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i0 = (k >> 1) * 4 + (k & 1);      // levels 8, 9, 12, 13 (s = 0) | + 2 (s = 1)
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
      const auto v = __builtin_amdgcn_permlane16_swap(__float_as_uint(part[i0][ft]), __float_as_uint(part[i0 + 2][ft]), false, false);
      const unsigned v0 = v[0], v1 = v[1];
      f32x4& out = (k >> 1) ? r[1] : p[1];
      out[2 * (k & 1) + ft] = __uint_as_float(v0) + __uint_as_float(v1);      // = x side 0 + x side 1 in both lanes
    }
  }
}

// MLP, epilogue and stores of both tiles of a pair in one pass over the weights (mlp_layer2): per tile it is
// k_nerf_fwd<true, true>'s, operation by operation (no geo output, nothing saved) - the two tiles share the weight
// fragments read from LDS and nothing else; no value of one tile enters an operation of the other.  An odd last tile's
// invalid half B runs on the clamped samples (row n - 1) like the invalid rows of a ragged tile: its stores are masked.
__device__ __forceinline__ void pair_mlp(const float4* __restrict__ wl, int lane, bool valid_a, bool valid_b, int64_t ma,
                                         int64_t mb, const f32x4 (&enc_a)[2], const f32x4 (&enc_b)[2], f32x4 sh_a, f32x4 sh_b,
                                         float density_scale, float* __restrict__ sigma, float* __restrict__ rgb) {
  const int q = lane >> 4;
  f32x4 h1a[4], h1b[4];
  mlp_layer2<4, 2>(wl + kSig0 / 4, lane, enc_a, enc_b, h1a, h1b);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    h1a[t] = relu4(h1a[t]);
    h1b[t] = relu4(h1b[t]);
  }
  f32x4 h2a[1], h2b[1];
  mlp_layer2<1, 4>(wl + kSig1 / 4, lane, h1a, h1b, h2a, h2b);
  if (valid_a && q == 0) sigma[ma] = __expf(h2a[0][0]) * density_scale;
  if (valid_b && q == 0) sigma[mb] = __expf(h2b[0][0]) * density_scale;
  const f32x4 cin_a[2] = {sh_a, h2a[0]}, cin_b[2] = {sh_b, h2b[0]};
  f32x4 c1a[4], c1b[4], c2a[4], c2b[4], oa[1], ob[1];
  mlp_layer2<4, 2>(wl + kCol0 / 4, lane, cin_a, cin_b, c1a, c1b);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    c1a[t] = relu4(c1a[t]);
    c1b[t] = relu4(c1b[t]);
  }
  mlp_layer2<4, 4>(wl + kCol1 / 4, lane, c1a, c1b, c2a, c2b);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    c2a[t] = relu4(c2a[t]);
    c2b[t] = relu4(c2b[t]);
  }
  mlp_layer2<1, 4>(wl + kCol2 / 4, lane, c2a, c2b, oa, ob);
  const float ch_a = sigmoid_rgb(rgb_channel_of_lane(oa[0]));
  const float ch_b = sigmoid_rgb(rgb_channel_of_lane(ob[0]));
  if (valid_a && q < 3) rgb[ma * 3 + q] = ch_a;
  if (valid_b && q < 3) rgb[mb * 3 + q] = ch_b;
}

// The records feed of k_nerf_fwd<true, true, 0, false, false, false, true> behind the pair front end; same arguments
// where it has them.  The host takes it only for a 16-level fp32 table whose levels 8..15 are all hashed.
// kDenseX: levels 0..3 are all dense (the host's dense_x_pairs_qualify decides) - issue_coarse_pair_dense.
template <bool kDenseX = false>
__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_nerf_fwd_pair(
    const float* __restrict__ x, int64_t M, float bound, const float2* __restrict__ emb, uint32_t emb_bytes, GridDesc G,
    const float4* __restrict__ packed, float density_scale, float* __restrict__ sigma, float* __restrict__ rgb,
    const int32_t* __restrict__ ray_ids, const float4* __restrict__ shq, unsigned long long* __restrict__ steal) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  __builtin_amdgcn_s_setprio(3);
  constexpr int kStage = kNerfFloats / 4;
  for (int i = threadIdx.x; i < kStage; i += kFieldThreads) wl[i] = packed[i];
  LevelRec* recs = reinterpret_cast<LevelRec*>(wl + kStage);
  stage_level_recs(G, recs);
  __syncthreads();

  constexpr int kWaves = kFieldThreads / 64;
  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15, h = lane >> 5;
  const uint32_t side = (uint32_t)(q & 1);
  const int64_t n = M;
  const int64_t n_tiles = (n + 15) >> 4, n_pairs = (n_tiles + 1) >> 1;     // an odd last tile: a pair with an invalid half
  const float rb_rcp = 1.0f / (2.0f * bound);                               // exact: 2 * bound is a power of two
  TileWalkT<1> walk;
  walk.init(make_sched<1>(n_pairs, kWaves, steal != nullptr), steal);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)emb, 0, (int)emb_bytes, 0x00020000);

  for (int64_t pair = walk.next(); pair >= 0; pair = walk.next()) {
    // encoder layout: t, ray id, origin and direction of sample j of tile h, once per pair
    const int64_t mg = pair * 32 + h * 16 + j;
    const int64_t mm = mg < n ? mg : n - 1;
    const float t = x[mm];
    const int32_t rid = ray_ids[mm];
    const float4* row = shq + (int64_t)rid * kRayRowVec;
    const float4 o4 = row[4], d4 = row[5];
    // MLP layout: lanes (q, j) of tile A / B need sample j's SH row q - the ray ids of the lower / upper half-wave
    const auto rr = __builtin_amdgcn_permlane32_swap((unsigned)rid, (unsigned)rid, false, false);
    const unsigned rid_a = rr[0], rid_b = rr[1];
    const float4 sa = shq[(int64_t)(int32_t)rid_a * kRayRowVec + q], sb = shq[(int64_t)(int32_t)rid_b * kRayRowVec + q];
    const float x0 = sample_x01_pow2(sample_pos(o4.x, t, d4.x, bound), bound, rb_rcp);
    const float x1 = sample_x01_pow2(sample_pos(o4.y, t, d4.y, bound), bound, rb_rcp);
    const float x2 = sample_x01_pow2(sample_pos(o4.z, t, d4.z, bound), bound, rb_rcp);

    f32x4 enc_a[2], enc_b[2];
    {
      GatheredPair g;
      uint32_t rec_off = side * 4u * (uint32_t)sizeof(LevelRec);
      asm volatile("" : "+v"(rec_off));    // opaque per pair: keeps the records in LDS, not hoisted into VGPRs
      // 32 coarse + 16 fine gathers out, the coarse blend under the fine loads, then the other 16: at most 48 rows
      // (96 registers) are held at once, which leaves the marchers of the next view their registers on the CU
      const LevelRec* my_recs = reinterpret_cast<const LevelRec*>(reinterpret_cast<const char*>(recs) + rec_off);
      if constexpr (kDenseX) issue_coarse_pair_dense(my_recs, rsrc, x0, x1, x2, g);
      else issue_coarse_pair(my_recs, rsrc, x0, x1, x2, g);
      issue_fine_pair<0>(G, rsrc, side, x0, x1, x2, g);
      __builtin_amdgcn_sched_barrier(0);
      blend_coarse_pair(g, enc_a, enc_b);
      __builtin_amdgcn_sched_barrier(0);
      issue_fine_pair<4>(G, rsrc, side, x0, x1, x2, g);
      __builtin_amdgcn_sched_barrier(0);
      blend_fine_pair(g, enc_a, enc_b);
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const auto v = __builtin_amdgcn_permlane32_swap(__float_as_uint(enc_a[e][c]), __float_as_uint(enc_b[e][c]), false, false);
        const unsigned v0 = v[0], v1 = v[1];
        enc_a[e][c] = __uint_as_float(v0);
        enc_b[e][c] = __uint_as_float(v1);
      }
    }

    const int64_t ma = pair * 32 + j, mb = ma + 16;
    pair_mlp(wl, lane, ma < n, mb < n, ma, mb, enc_a, enc_b, f32x4{sa.x, sa.y, sa.z, sa.w}, f32x4{sb.x, sb.y, sb.z, sb.w},
             density_scale, sigma, rgb);
  }
}

// ---- sliced frame path: the finest levels level by level (round 5) ---------------------------------------------------
// A hashed level is 2^19 rows x 8 B = 4 MiB - exactly one XCD's L2.  Where the finest levels are finer than the spacing
// of the frame's samples (a scene that fills a bound >= 4 volume: finest level 8192), no two samples share a cell on
// them: each (sample, level) costs four 128-byte lines whatever the order, and the only cache that can serve them is
// one that holds the WHOLE level.  The fused kernel touches all 16 levels in every tile, so exactly those levels miss
// the L2 altogether - PMC at bound 4: 12.35 fabric requests per sample = 3 levels x 4 lines, 58 G requests/s against
// the 69 G random lines/s the XCD fabric ports deliver (profiles/r05_NOTES.txt 1-2).  This pre-pass evaluates the THREE
// finest levels (13..15) one level at a time over all samples - the level is the slow index of the launch, so at any
// moment every XCD's L2 holds the one level the chip is working on (tools/micro/level_xcd_bench.hip: 259 against 69 G
// lines/s; the kernel reaches 200) - and leaves 24 bytes per sample for k_nerf_fwd<.., kPre>, which gathers the other
// thirteen levels and reads these back, streamed.  2.8 ms per level and 141 M samples against 3.7 ms inside the fused
// kernel; level 12 costs 0.7 ms inside and stays there (history of the cut, from all eight fine levels on their own XCDs
// down to this: notes 3).  Lanes 2i, 2i+1 of a wave are the two x sides of sample i (one look-up for the x-neighbour
// rows).  Arithmetic = the fused kernel's fine slots, operation by operation: results are bit-identical.
constexpr int kSliceThreads = 256;
constexpr int kSliceTilesPerIter = 4;     // 32-sample tiles a wave has in flight (4 loads per lane each)
struct SliceX {
  float x0, x1, x2;
};
__device__ __forceinline__ SliceX slice_load_x(const float* __restrict__ x01, int64_t m, int64_t M) {
  const int64_t mm = m < M ? m : M - 1;
  const float* p = x01 + mm * 3;
  return SliceX{__builtin_nontemporal_load(p), __builtin_nontemporal_load(p + 1), __builtin_nontemporal_load(p + 2)};
}
// grid (workgroups per level, kSliceLevels): the level is the SLOW index of the launch, so the chip sweeps the chunk's
// samples level by level and at any time (nearly) all workgroups of every XCD gather from the same 4 MiB
__global__ void __launch_bounds__(kSliceThreads) k_grid_fine_slices(const float* __restrict__ x01, int64_t M,
                                                                    const float2* __restrict__ emb, uint32_t emb_bytes,
                                                                    GridDesc G, float* __restrict__ pre) {
  const int slice = blockIdx.y;
  const int l = 16 - kSliceLevels + slice;
  const float sc = G.scales[l];
  const uint32_t m_ = G.mask[l], res1 = G.res1[l];
  const bool h = m_ != 0;
  const uint32_t base = G.offsets[l] * 8u, pa = h ? 2654435761u : res1, pb = h ? 805459861u : res1 * res1;
  const uint32_t mask = h ? m_ : 0xFFFFFFFFu;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)emb, 0, (int)emb_bytes, 0x00020000);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t side = (uint32_t)(lane & 1);
  constexpr int kWaves = kSliceThreads / 64;
  constexpr int kT = kSliceTilesPerIter;
  const int64_t m_pad = (M + 31) & ~(int64_t)31;
  const int64_t n_iter = (M + 32 * kT - 1) / (32 * kT);
  float* __restrict__ out = pre + (int64_t)slice * m_pad * 2;
  for (int64_t it = (int64_t)blockIdx.x * kWaves + w; it < n_iter; it += (int64_t)gridDim.x * kWaves) {
    u32x2 rows[kT][4];
    float wx[kT], fy[kT], fz[kT];
#pragma unroll
    for (int t = 0; t < kT; ++t) {
      const SliceX X = slice_load_x(x01, (it * kT + t) * 32 + (lane >> 1), M);
      const float px = X.x0 * sc + 0.5f, py = X.x1 * sc + 0.5f, pz = X.x2 * sc + 0.5f;       // mul, add: not fused
      const float fx = __builtin_amdgcn_fractf(px);
      wx[t] = side ? fx : 1.0f - fx;
      fy[t] = __builtin_amdgcn_fractf(py); fz[t] = __builtin_amdgcn_fractf(pz);
      const uint32_t c = (uint32_t)px + side, cy = (uint32_t)py, cz = (uint32_t)pz;
      const uint32_t hy0 = cy * pa, hy1 = hy0 + pa;
      const uint32_t hz0 = cz * pb, hz1 = hz0 + pb;
      const uint32_t yz[4] = {h ? (hy0 ^ hz0) : (hy0 + hz0), h ? (hy1 ^ hz0) : (hy1 + hz0),
                              h ? (hy0 ^ hz1) : (hy0 + hz1), h ? (hy1 ^ hz1) : (hy1 + hz1)};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t idx = (h ? (c ^ yz[k]) : (c + yz[k])) & mask;
        rows[t][k] = gather_row<false>(rsrc, base + idx * 8u);
      }
    }
#pragma unroll
    for (int t = 0; t < kT; ++t) {
      const f32x2 wy = {1.0f - fy[t], fy[t]};
      const f32x2 xy = wy * wx[t];
      const f32x2 w0 = xy * (1.0f - fz[t]), w1 = xy * fz[t];
      f32x2 acc = {0.f, 0.f};
      acc = __builtin_elementwise_fma(w0.xx, row2<false>(rows[t][0]), acc);
      acc = __builtin_elementwise_fma(w0.yy, row2<false>(rows[t][1]), acc);
      acc = __builtin_elementwise_fma(w1.xx, row2<false>(rows[t][2]), acc);
      acc = __builtin_elementwise_fma(w1.yy, row2<false>(rows[t][3]), acc);
      const float ox = __shfl_xor(acc.x, 1), oy = __shfl_xor(acc.y, 1);
      const float v = side ? acc.y + oy : acc.x + ox;          // both lanes hold side 0 + side 1; lane `side` stores feature `side`
      const int64_t m = (it * kT + t) * 32 + (lane >> 1);
      if (m < M) __builtin_nontemporal_store(v, out + m * 2 + side);
    }
  }
}

// ---- rgb-sigma lattice extraction (BASELINE configs[4]) ---------------------------------------
// out[m] = (mean over D fixed view directions of rgb(x_m, dir), raw density logit h0(x_m)): ONE gather and ONE
// sigma-net pass per point, then the colour net once per direction with the direction's SH row as a wave-uniform
// operand (staged in LDS).  Replaces density() + D x color() through the unfused encoder / BLAS path.
// kLattice (round 4): the points are a [W, L, H] lattice given by its three coordinate axes (x = ax_w[iw], y = ax_l[il],
// z = ax_h[ih]: exactly the caller's floats, no meshgrid tensor) and a 16-sample tile is a RUN ALONG W at fixed (il, ih).
// The writer's own order has h fastest; x is the fastest index of the table's rows (dense and hashed levels alike), so
// 16 consecutive h are 16 different 128-byte lines per level and corner where 16 consecutive w share one or two: the
// kernel is purely gather-bound (1 or 4 colour-net passes: 2.546 / 2.545 ms) and went 2.55 -> 1.07 ms for 160^3 points
// on the order alone (tools/extract_order_probe.py, profiles/r04_NOTES.txt 6).  out stays [W, L, H, 4].
struct LatticeDesc {
  const float* ax_w;
  const float* ax_l;
  const float* ax_h;
  int W, L, H, Wp;          // Wp = W rounded up to 16: a tile never straddles two (il, ih)
};
constexpr int kMaxExtractDirs = 8;
template <bool kLattice>
__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_nerf_fwd_dirs(
    const float* __restrict__ x, int64_t M, float bound, const float2* __restrict__ emb, uint32_t emb_bytes, GridDesc G,
    const float4* __restrict__ packed, const float* __restrict__ sh_dirs /*[D,16]*/, int D, float4* __restrict__ out,
    LatticeDesc lat, float logit_min) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  constexpr int kStage = kNerfFloats / 4;
  for (int i = threadIdx.x; i < kStage; i += kFieldThreads) wl[i] = packed[i];
  LevelRec* recs = reinterpret_cast<LevelRec*>(wl + kStage);
  stage_level_recs(G, recs);
  float* shl = reinterpret_cast<float*>(recs + 16);                   // [D][q][ks]: lane q's four components per direction
  for (int i = threadIdx.x; i < D * 16; i += kFieldThreads) {
    const int d = i >> 4, qq = (i >> 2) & 3, ks = i & 3;
    shl[i] = sh_dirs[d * 16 + 4 * ks + qq];
  }
  __syncthreads();
  constexpr int kWaves = kFieldThreads / 64;
  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
  const int64_t n_tiles = (M + 15) >> 4;
  const float rb = 2.0f * bound;
  const TileSched sched = make_sched(n_tiles, kWaves);
  const bool all_hashed[4] = {slot_all_hashed(G, 0), slot_all_hashed(G, 1), slot_all_hashed(G, 2), slot_all_hashed(G, 3)};
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)emb, 0, (int)emb_bytes, 0x00020000);
  const float inv_d = 1.0f / (float)D;
  for (int64_t it = 0, tile = sched.tile(0); tile < sched.hi; tile = sched.tile(++it)) {
    int64_t m = tile * 16 + j;
    bool valid = m < M;
    TileIn me;
    if constexpr (kLattice) {
      // traversal index -> (il, ih, iw) with iw fastest; the caller clamps to [-bound, bound] like extract_rgbsigma did
      const int64_t row = m / lat.Wp;
      const int iw = (int)(m - row * lat.Wp);
      const int il = (int)(row / lat.H), ih = (int)(row - (int64_t)il * lat.H);
      valid = valid && iw < lat.W;
      const int cw = min(iw, lat.W - 1), cl = min(il, lat.L - 1);
      me.x0 = to_x01(fminf(fmaxf(lat.ax_w[cw], -bound), bound), bound, rb, 0.0f);
      me.x1 = to_x01(fminf(fmaxf(lat.ax_l[cl], -bound), bound), bound, rb, 0.0f);
      me.x2 = to_x01(fminf(fmaxf(lat.ax_h[ih], -bound), bound), bound, rb, 0.0f);
      me.oob = oob01(me.x0, me.x1, me.x2);
      if (me.oob) me.x0 = me.x1 = me.x2 = 0.0f;
      m = ((int64_t)cw * lat.L + cl) * lat.H + ih;      // where the point lives in [W, L, H]
    } else {
      load_tile_in<false>(x, nullptr, valid ? m : M - 1, bound, rb, 0.0f, me);
    }
    f32x4 enc[2];
    {
      Gathered g;
      uint32_t rec_off = (uint32_t)q * 4u * (uint32_t)sizeof(LevelRec);
      asm volatile("" : "+v"(rec_off));
      issue_gathers(reinterpret_cast<const LevelRec*>(reinterpret_cast<const char*>(recs) + rec_off), all_hashed, rsrc,
                    me.x0, me.x1, me.x2, g);
      __builtin_amdgcn_sched_barrier(0);
      blend(g, enc[0], enc[1]);
    }
    if (me.oob) enc[0] = enc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 h1[4], h2[1];
    mlp_layer<4, 2>(wl + kSig0 / 4, lane, enc, h1);
#pragma unroll
    for (int t = 0; t < 4; ++t) h1[t] = relu4(h1[t]);
    mlp_layer<1, 4>(wl + kSig1 / 4, lane, h1, h2);
    float ch = 0.f;                                                     // lane q < 3: channel q, summed over the directions
    for (int d = 0; d < D; ++d) {                                       // wave-uniform trip count
      f32x4 cin[2], c1[4], c2[4], o[1];
      const float4 s4 = *reinterpret_cast<const float4*>(shl + d * 16 + q * 4);
      cin[0] = f32x4{s4.x, s4.y, s4.z, s4.w};
      cin[1] = h2[0];
      mlp_layer<4, 2>(wl + kCol0 / 4, lane, cin, c1);
#pragma unroll
      for (int t = 0; t < 4; ++t) c1[t] = relu4(c1[t]);
      mlp_layer<4, 4>(wl + kCol1 / 4, lane, c1, c2);
#pragma unroll
      for (int t = 0; t < 4; ++t) c2[t] = relu4(c2[t]);
      mlp_layer<1, 4>(wl + kCol2 / 4, lane, c2, o);
      ch += sigmoid_rgb(rgb_channel_of_lane(o[0]));
    }
    if (valid) {
      float* o4 = reinterpret_cast<float*>(out + m);
      if (q < 3) o4[q] = ch * inv_d;
      if (q == 0) o4[3] = fmaxf(h2[0][0], logit_min);
    }
  }
}

// kSave (training) 1: the encoder output and the two hidden activations are also written, row-major, for the
// weight gradients and the ReLU masks of k_instance_bwd; 2: the encoder output only (k_instance_head_bwd recomputes
// the hidden layers: 512 B per sample less to write here and to read there).
template <int K_MT, int kSave = 0>
__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_instance_fwd(const float* __restrict__ x, int64_t M,
                                                                   const int32_t* __restrict__ n_dev, float bound,
                                                                   const float2* __restrict__ emb, uint32_t emb_bytes,
                                                                   GridDesc G, const float4* __restrict__ packed,
                                                                   float* __restrict__ logits, float* __restrict__ enc_out,
                                                                   float* __restrict__ h1_out, float* __restrict__ h2_out) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  constexpr int K = K_MT * 16;
  constexpr int kStage = (kIns2 + K * 64) / 4;
  for (int i = threadIdx.x; i < kStage; i += kFieldThreads) wl[i] = packed[i];
  LevelRec* recs = reinterpret_cast<LevelRec*>(wl + kStage);
  stage_level_recs(G, recs);
  __syncthreads();

  constexpr int kWaves = kFieldThreads / 64;
  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
  int64_t n = M;
  if (n_dev) n = min((int64_t)*n_dev, M);
  const int64_t n_tiles = (n + 15) >> 4;
  const float rb = 2.0f * bound;
  const float rb_inv = 0.0f;
  const TileSched sched = make_sched(n_tiles, kWaves);

  const bool all_hashed[4] = {slot_all_hashed(G, 0), slot_all_hashed(G, 1), slot_all_hashed(G, 2), slot_all_hashed(G, 3)};
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)emb, 0, (int)emb_bytes, 0x00020000);

  for (int64_t it = 0, tile = sched.tile(0); tile < sched.hi; tile = sched.tile(++it)) {
    const int64_t m = tile * 16 + j;
    const bool valid = m < n;
    TileIn me;
    load_tile_in<false>(x, nullptr, valid ? m : n - 1, bound, rb, rb_inv, me);
    f32x4 enc[2];
    {
      Gathered g;
      uint32_t rec_off = (uint32_t)q * 4u * (uint32_t)sizeof(LevelRec);
      asm volatile("" : "+v"(rec_off));    // opaque per tile: keeps the records in LDS, not hoisted into VGPRs
      issue_gathers(reinterpret_cast<const LevelRec*>(reinterpret_cast<const char*>(recs) + rec_off), all_hashed, rsrc,
                    me.x0, me.x1, me.x2, g);
      __builtin_amdgcn_sched_barrier(0);   // all 32 gathers in flight before the first blend waits
      blend(g, enc[0], enc[1]);
    }
    if (me.oob) enc[0] = enc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 h1[4], h2[4], o[K_MT];
    mlp_layer<4, 2>(wl + kIns0 / 4, lane, enc, h1);
#pragma unroll
    for (int t = 0; t < 4; ++t) h1[t] = relu4(h1[t]);
    mlp_layer<4, 4>(wl + kIns1 / 4, lane, h1, h2);
#pragma unroll
    for (int t = 0; t < 4; ++t) h2[t] = relu4(h2[t]);
    mlp_layer<K_MT, 4>(wl + kIns2 / 4, lane, h2, o);
    if (valid) {
#pragma unroll
      for (int mt = 0; mt < K_MT; ++mt) {
        float4 v = make_float4(o[mt][0], o[mt][1], o[mt][2], o[mt][3]);
        *reinterpret_cast<float4*>(logits + m * K + 16 * mt + 4 * q) = v;
      }
      if constexpr (kSave != 0) {
        // lane q holds encoder features 4q..4q+3 and 16+4q..16+4q+3, and rows 16t+4q..+3 of every hidden tile
#pragma unroll
        for (int t = 0; t < 2; ++t)
          *reinterpret_cast<float4*>(enc_out + m * 32 + 16 * t + 4 * q) = make_float4(enc[t][0], enc[t][1], enc[t][2], enc[t][3]);
      }
      if constexpr (kSave == 1) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          *reinterpret_cast<float4*>(h1_out + m * 64 + 16 * t + 4 * q) = make_float4(h1[t][0], h1[t][1], h1[t][2], h1[t][3]);
          *reinterpret_cast<float4*>(h2_out + m * 64 + 16 * t + 4 * q) = make_float4(h2[t][0], h2[t][1], h2[t][2], h2[t][3]);
        }
      }
    }
  }
}

// ---- instance-mask lattice extraction (3-D instance segmentation of a trained scene) -------------------------------
// One launch over the [W, L, H] lattice, walked like k_nerf_fwd_dirs<true> (runs of 16 along W, coordinates clamped to
// [-bound, bound]): NeRF gather + the two sigma-net layers -> sigma = exp(logit) * density_scale, the sigma the renderer
// composites; a voxel is occupied when sigma >= sigma_thresh.  A tile none of whose 16 voxels is occupied (wave-uniform
// ballot) skips the instance gather and MLP - most of a room is empty space, and this skip is where the launch saves its
// bytes.  Every other tile runs k_instance_fwd's math and reduces the logits IN REGISTERS: arg-max over the K real
// channels (the zero-padded MFMA channels K..K_pad-1 are excluded - exact zeros would beat all-negative real logits),
// lowest channel on ties (torch.argmax), max-softmax confidence.  A voxel's channels 16mt + 4q + r are spread over its
// four q lanes, so both reductions run across lanes j, j+16, j+32, j+48.  No logits go to memory: per voxel 1 label
// byte, 4 confidence bytes (and the 4-byte density logit when asked for).
constexpr uint8_t kLabelEmpty = 255;
constexpr int kNoChannel = 0x7fffffff;
template <int K_MT>
__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_instance_lattice(
    LatticeDesc lat, float bound, const float2* __restrict__ emb_n, uint32_t emb_n_bytes, GridDesc Gn,
    const float4* __restrict__ packed_n, float density_scale, float sigma_thresh, const float2* __restrict__ emb_i,
    uint32_t emb_i_bytes, GridDesc Gi, const float4* __restrict__ packed_i, int K, uint8_t* __restrict__ labels,
    float* __restrict__ confidence, float* __restrict__ logit_out) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  constexpr int kStageN = kCol0 / 4;                         // the sigma net only: no colour net here
  constexpr int kStageI = (kIns2 + K_MT * 16 * 64) / 4;
  const float4* wn = wl;
  const float4* wi = wl + kStageN;
  for (int i = threadIdx.x; i < kStageN; i += kFieldThreads) wl[i] = packed_n[i];
  for (int i = threadIdx.x; i < kStageI; i += kFieldThreads) wl[kStageN + i] = packed_i[i];
  LevelRec* recs_n = reinterpret_cast<LevelRec*>(wl + kStageN + kStageI);
  LevelRec* recs_i = recs_n + 16;
  stage_level_recs(Gn, recs_n);
  stage_level_recs(Gi, recs_i);
  __syncthreads();

  constexpr int kWaves = kFieldThreads / 64;
  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
  const int64_t n_tiles = ((int64_t)lat.Wp * lat.L * lat.H) >> 4;
  const float rb = 2.0f * bound;
  const TileSched sched = make_sched(n_tiles, kWaves);
  const bool hashed_n[4] = {slot_all_hashed(Gn, 0), slot_all_hashed(Gn, 1), slot_all_hashed(Gn, 2), slot_all_hashed(Gn, 3)};
  const bool hashed_i[4] = {slot_all_hashed(Gi, 0), slot_all_hashed(Gi, 1), slot_all_hashed(Gi, 2), slot_all_hashed(Gi, 3)};
  const __amdgpu_buffer_rsrc_t rsrc_n = __builtin_amdgcn_make_buffer_rsrc((void*)emb_n, 0, (int)emb_n_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_i = __builtin_amdgcn_make_buffer_rsrc((void*)emb_i, 0, (int)emb_i_bytes, 0x00020000);
  for (int64_t it = 0, tile = sched.tile(0); tile < sched.hi; tile = sched.tile(++it)) {
    const int64_t m = tile * 16 + j;
    const int64_t row = m / lat.Wp;
    const int iw = (int)(m - row * lat.Wp);
    const int il = (int)(row / lat.H), ih = (int)(row - (int64_t)il * lat.H);
    const bool valid = iw < lat.W;
    const int cw = min(iw, lat.W - 1);
    TileIn me;
    me.x0 = to_x01(fminf(fmaxf(lat.ax_w[cw], -bound), bound), bound, rb, 0.0f);
    me.x1 = to_x01(fminf(fmaxf(lat.ax_l[il], -bound), bound), bound, rb, 0.0f);
    me.x2 = to_x01(fminf(fmaxf(lat.ax_h[ih], -bound), bound), bound, rb, 0.0f);
    me.oob = oob01(me.x0, me.x1, me.x2);
    if (me.oob) me.x0 = me.x1 = me.x2 = 0.0f;
    const int64_t o = ((int64_t)cw * lat.L + il) * lat.H + ih;      // where the voxel lives in [W, L, H]
    const uint32_t rec_off0 = (uint32_t)q * 4u * (uint32_t)sizeof(LevelRec);

    float logit;
    {
      f32x4 enc[2];
      {
        Gathered g;
        uint32_t rec_off = rec_off0;
        asm volatile("" : "+v"(rec_off));
        issue_gathers(reinterpret_cast<const LevelRec*>(reinterpret_cast<const char*>(recs_n) + rec_off), hashed_n, rsrc_n,
                      me.x0, me.x1, me.x2, g);
        __builtin_amdgcn_sched_barrier(0);
        blend(g, enc[0], enc[1]);
      }
      if (me.oob) enc[0] = enc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 h1[4], h2[1];
      mlp_layer<4, 2>(wn + kSig0 / 4, lane, enc, h1);
#pragma unroll
      for (int t = 0; t < 4; ++t) h1[t] = relu4(h1[t]);
      mlp_layer<1, 4>(wn + kSig1 / 4, lane, h1, h2);
      logit = __shfl(h2[0][0], j);                  // row 0 of sample j lives in lane (q = 0, j)
    }
    const bool occ = valid && __expf(logit) * density_scale >= sigma_thresh;     // k_nerf_fwd's sigma, times the scale
    if (logit_out && valid && q == 0) logit_out[o] = logit;
    if (__ballot(occ) == 0) {                       // wave-uniform: no occupied voxel in this run of 16
      if (valid && q == 0) {
        labels[o] = kLabelEmpty;
        confidence[o] = 0.0f;
      }
      continue;
    }

    f32x4 out[K_MT];
    {
      f32x4 enc[2];
      {
        Gathered g;
        uint32_t rec_off = rec_off0;
        asm volatile("" : "+v"(rec_off));
        issue_gathers(reinterpret_cast<const LevelRec*>(reinterpret_cast<const char*>(recs_i) + rec_off), hashed_i, rsrc_i,
                      me.x0, me.x1, me.x2, g);
        __builtin_amdgcn_sched_barrier(0);
        blend(g, enc[0], enc[1]);
      }
      if (me.oob) enc[0] = enc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 h1[4], h2[4];
      mlp_layer<4, 2>(wi + kIns0 / 4, lane, enc, h1);
#pragma unroll
      for (int t = 0; t < 4; ++t) h1[t] = relu4(h1[t]);
      mlp_layer<4, 4>(wi + kIns1 / 4, lane, h1, h2);
#pragma unroll
      for (int t = 0; t < 4; ++t) h2[t] = relu4(h2[t]);
      mlp_layer<K_MT, 4>(wi + kIns2 / 4, lane, h2, out);
    }
    // arg-max: this lane's channels in ascending order (strict > keeps the lowest on ties), then across the q lanes
    float best = 0.0f;
    int bi = kNoChannel;
#pragma unroll
    for (int mt = 0; mt < K_MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * mt + 4 * q + r;
        if (c < K && (bi == kNoChannel || out[mt][r] > best)) {
          best = out[mt][r];
          bi = c;
        }
      }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float ob = __shfl_xor(best, off);
      const int oi = __shfl_xor(bi, off);
      if (oi != kNoChannel && (bi == kNoChannel || ob > best || (ob == best && oi < bi))) {
        best = ob;
        bi = oi;
      }
    }
    // max-softmax = 1 / sum_c exp(l_c - max); the butterfly gives every q lane the same sum (a + b == b + a)
    float s = 0.0f;
#pragma unroll
    for (int mt = 0; mt < K_MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * mt + 4 * q + r < K) s += __expf(out[mt][r] - best);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (valid && q == 0) {
      labels[o] = occ ? (uint8_t)bi : kLabelEmpty;
      confidence[o] = occ ? 1.0f / s : 0.0f;
    }
  }
}

// Per-channel statistics of a label volume (labels 0..K-1, kLabelEmpty elsewhere): voxel count, inclusive index AABB
// and the sum of the confidences - bit-reproducible without float atomics.  Pass 1: workgroup b owns a contiguous range
// of voxels; each wave walks its 64-voxel chunks in order and, for every label present in a chunk, reduces the chunk's
// confidences of that label with a fixed butterfly and adds the result to its OWN per-wave LDS slot (one writer, program
// order).  Counts and bounds go through LDS integer atomics (order-independent).  The workgroup then writes, per
// channel, (count, min iw, il, ih, max iw, il, ih, sum over its waves in wave order) to its fixed slot of the workspace.
// Pass 2 (k_instance_stats_final) adds the workgroups' slots in a fixed order.
constexpr int kStatsThreads = 256;
constexpr int kStatsWaves = kStatsThreads / 64;
constexpr int kStatsMaxBlocks = 512;
constexpr int kStatsSlot = 8;                        // int32 words per (workgroup, channel)
constexpr int64_t kStatsWorkspaceBytes = (int64_t)kStatsMaxBlocks * 64 * kStatsSlot * 4;
static_assert(kStatsWorkspaceBytes == INR_INSTANCE_STATS_WORKSPACE_BYTES, "include/inr.h");

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}

__global__ void __launch_bounds__(kStatsThreads) k_instance_stats_partial(const uint8_t* __restrict__ labels,
                                                                          const float* __restrict__ confidence,
                                                                          uint32_t N, uint32_t L, uint32_t H, int K,
                                                                          uint32_t per_block, int* __restrict__ part) {
  __shared__ int s_cnt[64], s_lo[3][64], s_hi[3][64];
  __shared__ float s_sum[kStatsWaves][64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t < 64) {
    s_cnt[t] = 0;
    for (int a = 0; a < 3; ++a) { s_lo[a][t] = 0x7fffffff; s_hi[a][t] = -1; }
  }
  s_sum[w][lane] = 0.0f;
  __syncthreads();
  const uint32_t lo = blockIdx.x * per_block;
  const uint32_t hi = min(N, lo + per_block);
  const uint32_t LH = L * H;
  for (uint32_t base = lo + (uint32_t)w * 64u; base < hi; base += kStatsThreads) {
    const uint32_t v = base + (uint32_t)lane;
    const bool in = v < hi;
    const int lab = in ? (int)labels[v] : (int)kLabelEmpty;
    const float cf = in ? confidence[v] : 0.0f;
    const bool live = lab < K;
    const uint32_t iw = v / LH, rem = v - iw * LH, il = rem / H, ih = rem - il * H;
    unsigned long long pending = __ballot(live);
    while (pending) {
      const int c = __builtin_amdgcn_readfirstlane(__shfl(lab, (int)__builtin_ctzll(pending)));
      const bool mine = live && lab == c;
      const unsigned long long mask = __ballot(mine);
      pending &= ~mask;
      float x = mine ? cf : 0.0f;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
      const int bw0 = wave_min(mine ? (int)iw : 0x7fffffff), bl0 = wave_min(mine ? (int)il : 0x7fffffff);
      const int bh0 = wave_min(mine ? (int)ih : 0x7fffffff);
      const int bw1 = wave_max(mine ? (int)iw : -1), bl1 = wave_max(mine ? (int)il : -1), bh1 = wave_max(mine ? (int)ih : -1);
      if (lane == 0) {
        s_sum[w][c] += x;
        atomicAdd(&s_cnt[c], (int)__popcll(mask));
        atomicMin(&s_lo[0][c], bw0); atomicMin(&s_lo[1][c], bl0); atomicMin(&s_lo[2][c], bh0);
        atomicMax(&s_hi[0][c], bw1); atomicMax(&s_hi[1][c], bl1); atomicMax(&s_hi[2][c], bh1);
      }
    }
  }
  __syncthreads();
  if (t < K) {
    float sum = 0.0f;
    for (int ww = 0; ww < kStatsWaves; ++ww) sum += s_sum[ww][t];
    int* slot = part + ((int64_t)blockIdx.x * 64 + t) * kStatsSlot;
    slot[0] = s_cnt[t];
    slot[1] = s_lo[0][t]; slot[2] = s_lo[1][t]; slot[3] = s_lo[2][t];
    slot[4] = s_hi[0][t]; slot[5] = s_hi[1][t]; slot[6] = s_hi[2][t];
    slot[7] = __float_as_int(sum);
  }
}

// 8 groups of 64 threads: thread (g, c) folds workgroups g, g + 8, g + 16, ... of channel c in that order, then thread
// (0, c) folds the eight groups in group order - a fixed order (bit-reproducible) with 1/8 of the serial chain of one
// thread per channel (0.13 ms at 512 workgroups)
constexpr int kStatsFinalGroups = 8;
__global__ void __launch_bounds__(64 * kStatsFinalGroups) k_instance_stats_final(const int* __restrict__ part, int n_blocks,
                                                                                 int K, int32_t* __restrict__ counts,
                                                                                 int32_t* __restrict__ boxes,
                                                                                 float* __restrict__ conf_sum) {
  __shared__ int s_b[kStatsFinalGroups][7][64];
  __shared__ float s_s[kStatsFinalGroups][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  int cnt = 0, b[6] = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1, -1, -1};
  float sum = 0.0f;
  if (c < K) {
    for (int blk = g; blk < n_blocks; blk += kStatsFinalGroups) {
      const int* slot = part + ((int64_t)blk * 64 + c) * kStatsSlot;
      cnt += slot[0];
      for (int a = 0; a < 3; ++a) {
        b[a] = min(b[a], slot[1 + a]);
        b[3 + a] = max(b[3 + a], slot[4 + a]);
      }
      sum += __int_as_float(slot[7]);
    }
  }
  s_b[g][0][c] = cnt;
  for (int a = 0; a < 6; ++a) s_b[g][1 + a][c] = b[a];
  s_s[g][c] = sum;
  __syncthreads();
  if (g != 0 || c >= K) return;
  for (int gg = 1; gg < kStatsFinalGroups; ++gg) {
    cnt += s_b[gg][0][c];
    for (int a = 0; a < 3; ++a) {
      b[a] = min(b[a], s_b[gg][1 + a][c]);
      b[3 + a] = max(b[3 + a], s_b[gg][4 + a][c]);
    }
    sum += s_s[gg][c];
  }
  counts[c] = cnt;
  for (int a = 0; a < 6; ++a) boxes[c * 6 + a] = cnt ? b[a] : -1;
  conf_sum[c] = sum;
}

// ---- instance MLP input gradients (training) ----------------------------------------------------------------
// The chain dL/dlogits -> dL/dz2 -> dL/dz1 -> dL/denc is the same transposed formulation with W^T as the A
// operand: G^T = W^T . dY^T, so every layer's D registers are again the next layer's B operand.  Sections of
// `packed`: W2^T (64 x 64, inputs beyond K zero), W1^T (64 x 64), W0^T (32 x 64).  ReLU masks come from the saved
// activations (h > 0), loaded in the D-register layout with one float4 per tile.
constexpr int kBwd2 = 0;
constexpr int kBwd1 = kBwd2 + 64 * 64;
constexpr int kBwd0 = kBwd1 + 64 * 64;
constexpr int kBwdFloats = kBwd0 + 32 * 64;

__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_instance_bwd(const float* __restrict__ dlogits, int K,
                                                                   const float* __restrict__ h1, const float* __restrict__ h2,
                                                                   int64_t M, const float4* __restrict__ packed,
                                                                   float* __restrict__ dz2, float* __restrict__ dz1,
                                                                   float* __restrict__ denc) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  for (int i = threadIdx.x; i < kBwdFloats / 4; i += kFieldThreads) wl[i] = packed[i];
  __syncthreads();
  constexpr int kWaves = kFieldThreads / 64;
  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
  const int64_t n_tiles = (M + 15) >> 4;
  const TileSched sched = make_sched(n_tiles, kWaves);
  for (int64_t it = 0, tile = sched.tile(0); tile < sched.hi; tile = sched.tile(++it)) {
    const int64_t m = tile * 16 + j;
    const bool valid = m < M;
    const int64_t mm = valid ? m : M - 1;
    f32x4 g[4], hh[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int c = 16 * t + 4 * q;
      g[t] = (valid && c < K) ? load4(dlogits + mm * K + c) : f32x4{0.f, 0.f, 0.f, 0.f};
      hh[t] = load4(h2 + mm * 64 + c);
    }
    f32x4 a[4], b[4], c0[2];
    mlp_layer<4, 4>(wl + kBwd2 / 4, lane, g, a);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t] = mask4(a[t], hh[t]);
      hh[t] = load4(h1 + mm * 64 + 16 * t + 4 * q);
    }
    if (valid) {
#pragma unroll
      for (int t = 0; t < 4; ++t) store4(dz2 + m * 64 + 16 * t + 4 * q, a[t]);
    }
    mlp_layer<4, 4>(wl + kBwd1 / 4, lane, a, b);
#pragma unroll
    for (int t = 0; t < 4; ++t) b[t] = mask4(b[t], hh[t]);
    if (valid) {
#pragma unroll
      for (int t = 0; t < 4; ++t) store4(dz1 + m * 64 + 16 * t + 4 * q, b[t]);
    }
    mlp_layer<2, 4>(wl + kBwd0 / 4, lane, b, c0);
    if (valid) {
#pragma unroll
      for (int t = 0; t < 2; ++t) store4(denc + m * 32 + 16 * t + 4 * q, c0[t]);
    }
  }
}

// ---- instance head: the WHOLE backward in one launch (round 3) -----------------------------------------------
// Replaces, for the instance stage, k_composite_train_extra_bwd (dL/dlogits rows [M,K] written and read back),
// k_instance_bwd (which read the saved h1 / h2 and wrote dz2 / dz1 for the weight gradients) and the three
// k_linear_wgrad launches (which read all of them again): per sample it reads the saved encoder output (128 B), the
// compositing weight and the ray's row of dL/d(rendered logits), and writes dL/denc (128 B) - ~0.3 KB instead of
// ~3.5 KB of HBM traffic per sample.  Per 16-sample tile a wave
//   1. forms g = w * dL/dpix[ray] (the K-channel compositing backward, weights detached),
//   2. recomputes h1 = relu(W0 enc), h2 = relu(W1 h1) with the forward's own weights and code (same bits: the ReLU
//      masks are the forward's),
//   3. runs the input-gradient chain a = (W2^T g) . [h2 > 0], b = (W1^T a) . [h1 > 0], denc = W0^T b,
//   4. and the weight gradients dW2 += g^T h2, dW1 += a^T h1, dW0 += b^T enc on the fp32 matrix cores
//      (v_mfma_f32_16x16x4_f32, exact products, k = 4 samples per instruction).  The contraction runs over SAMPLES,
//      which sit in lane & 15 of the D-layout registers: the (G, X) tiles of the workgroup's eight waves are staged in
//      LDS row-major (row pitch 68 floats: the 16-byte writes of the 16 lanes of a q group fall into different
//      banks) and read back as A[i = channel][k = sample], B[k = sample][j = channel].  The 40 accumulator tiles
//      (16 + 16 + 8 of 16x16) are OWNED by the waves - wave w: tiles 2w, 2w+1 of dW2 and dW1, tile w of dW0, 20
//      VGPRs - and every wave consumes all eight staged tiles for its own accumulators.
// The workgroup's accumulators go to partial[block] (fragment order); k_head_wgrad_reduce sums over the workgroups.
// Rows >= n (the device-side sample count; the buffer is sized from mean_count) are not read: their dL/denc is zero.
constexpr int kHbPitch = 68;
constexpr int kHbWaves = kFieldThreads / 64;
constexpr int kHbTileFloats = 16 * kHbPitch;
constexpr int kHbStageFloats = 2 * kHbWaves * kHbTileFloats;            // G and X of one round: 69.6 KB
constexpr int kHbFwdFloats = kIns2;                                      // forward sections kIns0, kIns1
constexpr int kHbAccTiles = 40;

// The table-gradient buffer of the scatter that FOLLOWS a head-backward launch is zero-filled by that launch (every
// workgroup a slice, before its first tile): one launch and one exposed 49 MB fill less per training step.
__device__ __forceinline__ void hb_zero_fill(float* __restrict__ buf, int64_t n) {
  if (!buf) return;
  float4* b4 = reinterpret_cast<float4*>(buf);
  const int64_t n4 = n >> 2;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) b4[i] = z;
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) buf[(n4 << 2) + threadIdx.x] = 0.f;
}

#if INR_MLP_FP32
// exact-fp32 build: the (G, X) tiles staged row-major as fp32, contraction with v_mfma_f32_16x16x4_f32
typedef float HbStage;
__device__ __forceinline__ HbStage* hb_my_tile(float* plane, int wave) { return plane + wave * kHbTileFloats; }
template <int N_T>
__device__ __forceinline__ void hb_stage(HbStage* __restrict__ tile_base, int q, int j, const f32x4* v) {
#pragma unroll
  for (int t = 0; t < N_T; ++t) store4(tile_base + j * kHbPitch + 16 * t + 4 * q, v[t]);
}
__device__ __forceinline__ void hb_stage_value(HbStage* __restrict__ tile_base, int j, int channel, float v) {
  tile_base[j * kHbPitch + channel] = v;
}

// acc0 += G[:, ot]^T X[:, it0], acc1 += G[:, ot]^T X[:, it1] over the 8 x 16 staged samples
__device__ __forceinline__ void hb_accum(const float* __restrict__ gS, const float* __restrict__ xS, int q, int j, int ot,
                                         int it0, int it1, bool two, f32x4& acc0, f32x4& acc1) {
#pragma unroll 2
  for (int T = 0; T < kHbWaves; ++T) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = T * kHbTileFloats + (4 * u + q) * kHbPitch;
      const float a = gS[row + 16 * ot + j];
      const float b0 = xS[row + 16 * it0 + j];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc0, 0, 0, 0);
      if (two) {
        const float b1 = xS[row + 16 * it1 + j];
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc1, 0, 0, 0);
      }
    }
  }
}
#else
// Default build (late round 3): the weight gradients take the bf16 matrix cores too.  The fp32 contraction
// (v_mfma_f32_16x16x4_f32: 4 samples per 32-cycle instruction) was 62 % of these kernels' MFMA time; split into bf16
// head + remainder like the MLP layers (hi*hi + lo*hi + hi*lo, fp32 accumulation: 2^-16 relative per product, random
// over ~2e5 samples) the same 32 samples cost three 16-cycle v_mfma_f32_16x16x32_bf16.  The operands of that
// instruction hold 8 CONSECUTIVE k (= samples) per lane, so the tiles are staged TRANSPOSED - [channel][sample], a head
// plane and a remainder plane of 64 x 136 bf16 each (pitch 136 halfwords = 68 dwords: rows land 4 banks apart, the
// 16-byte reads of a 16-lane row spread over all banks) - exactly the 34 816 bytes per operand of the fp32 staging.
typedef uint16_t HbStage;
constexpr int kHbPitchH = 136;                           // halfwords per channel row: 128 samples + 8
constexpr int kHbPlaneH = 64 * kHbPitchH;                // halfwords per plane (head | remainder)
static_assert(2 * kHbPlaneH * 2 == kHbWaves * kHbTileFloats * 4, "bf16 staging must fit the fp32 staging's footprint");
__device__ __forceinline__ HbStage* hb_my_tile(float* plane, int wave) {
  return reinterpret_cast<HbStage*>(plane) + wave * 16;  // this wave's 16 sample columns
}
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2h_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t hb_pack_bf16x2(float a, float b) {       // v_cvt_pk_bf16_f32: round to nearest even
  const f32x2h_t v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
// head / remainder of two values -> (hi0 | hi1 << 16), (lo0 | lo1 << 16)
__device__ __forceinline__ void hb_split2(float v0, float v1, uint32_t& hi, uint32_t& lo) {
  hi = hb_pack_bf16x2(v0, v1);
  lo = hb_pack_bf16x2(v0 - __uint_as_float(hi << 16), v1 - __uint_as_float(hi & 0xFFFF0000u));
}
__device__ __forceinline__ void hb_put(HbStage* __restrict__ tile_base, int j, int channel, uint32_t hi16, uint32_t lo16) {
  tile_base[channel * kHbPitchH + j] = (uint16_t)hi16;
  tile_base[kHbPlaneH + channel * kHbPitchH + j] = (uint16_t)lo16;
}
template <int N_T>
__device__ __forceinline__ void hb_stage(HbStage* __restrict__ tile_base, int q, int j, const f32x4* v) {
#pragma unroll
  for (int t = 0; t < N_T; ++t) {
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      uint32_t hi, lo;
      hb_split2(v[t][r], v[t][r + 1], hi, lo);
      hb_put(tile_base, j, 16 * t + 4 * q + r, hi & 0xFFFFu, lo & 0xFFFFu);
      hb_put(tile_base, j, 16 * t + 4 * q + r + 1, hi >> 16, lo >> 16);
    }
  }
}
__device__ __forceinline__ void hb_stage_value(HbStage* __restrict__ tile_base, int j, int channel, float v) {
  uint32_t hi, lo;
  hb_split2(v, 0.0f, hi, lo);
  hb_put(tile_base, j, channel, hi & 0xFFFFu, lo & 0xFFFFu);
}

// acc0 += G[:, ot]^T X[:, it0], acc1 += G[:, ot]^T X[:, it1] over the 128 staged samples (4 k-blocks of 32)
__device__ __forceinline__ void hb_accum(const float* __restrict__ gS, const float* __restrict__ xS, int q, int j, int ot,
                                         int it0, int it1, bool two, f32x4& acc0, f32x4& acc1) {
  const uint16_t* G = reinterpret_cast<const uint16_t*>(gS) + (16 * ot + j) * kHbPitchH + 8 * q;
  const uint16_t* X0 = reinterpret_cast<const uint16_t*>(xS) + (16 * it0 + j) * kHbPitchH + 8 * q;
  const uint16_t* X1 = reinterpret_cast<const uint16_t*>(xS) + (16 * it1 + j) * kHbPitchH + 8 * q;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    const uint4 a_hi = *reinterpret_cast<const uint4*>(G + 32 * kb), a_lo = *reinterpret_cast<const uint4*>(G + kHbPlaneH + 32 * kb);
    const uint4 b_hi = *reinterpret_cast<const uint4*>(X0 + 32 * kb), b_lo = *reinterpret_cast<const uint4*>(X0 + kHbPlaneH + 32 * kb);
    acc0 = mfma_bf(a_hi, b_hi, acc0);
    acc0 = mfma_bf(a_lo, b_hi, acc0);
    acc0 = mfma_bf(a_hi, b_lo, acc0);
    if (two) {
      const uint4 c_hi = *reinterpret_cast<const uint4*>(X1 + 32 * kb), c_lo = *reinterpret_cast<const uint4*>(X1 + kHbPlaneH + 32 * kb);
      acc1 = mfma_bf(a_hi, c_hi, acc1);
      acc1 = mfma_bf(a_lo, c_hi, acc1);
      acc1 = mfma_bf(a_hi, c_lo, acc1);
    }
  }
}
#endif

__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_instance_head_bwd(
    const float* __restrict__ enc, const float* __restrict__ wbuf, const int32_t* __restrict__ ray_of,
    const float* __restrict__ g_pix, int Kp, int64_t M, const int32_t* __restrict__ n_dev,
    const float* __restrict__ scale_a, const float* __restrict__ scale_b,
    const float4* __restrict__ packed_fwd, const float4* __restrict__ packed_bwd, float* __restrict__ denc,
    float4* __restrict__ partial, float* __restrict__ zero_buf, int64_t zero_n) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  hb_zero_fill(zero_buf, zero_n);
  float4* wf = wl;
  float4* wb = wl + kHbFwdFloats / 4;
  float* gS = reinterpret_cast<float*>(wb + kBwdFloats / 4);
  float* xS = gS + kHbWaves * kHbTileFloats;
  for (int i = threadIdx.x; i < kHbFwdFloats / 4; i += kFieldThreads) wf[i] = packed_fwd[i];
  for (int i = threadIdx.x; i < kBwdFloats / 4; i += kFieldThreads) wb[i] = packed_bwd[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15, wave = threadIdx.x >> 6;
  int64_t n = M;
  if (n_dev) n = min((int64_t)*n_dev, M);
  // g_pix may be an unnormalised gradient (softmax - onehot of the fused cross entropy): the two device scalars -
  // 1 / kept rows and dL/dloss - scale every sample's weight instead of a pass over [N,K]
  const float g_scale = (scale_a ? *scale_a : 1.0f) * (scale_b ? *scale_b : 1.0f);
  const int64_t n_tiles = (M + 15) >> 4;
  const int64_t per_round = (int64_t)gridDim.x * kHbWaves;
  const int64_t n_rounds = (n_tiles + per_round - 1) / per_round;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[5] = {zero4, zero4, zero4, zero4, zero4};
  HbStage* my_g = hb_my_tile(gS, wave);
  HbStage* my_x = hb_my_tile(xS, wave);
  const int ot = wave >> 1, it0 = 2 * (wave & 1), it1 = it0 + 1;
  // Inputs of the NEXT round are requested while this round's weight-gradient phases run (the kernel is a chain of
  // dependent round trips otherwise: 7 rounds x (HBM load -> dependent row load -> MFMA chain -> 6 barriers)):
  // stage 1 (encoder row, weight, ray row) right after this round's inputs are consumed, stage 2 (the ray's
  // dL/dpix row, which needs the ray row) before the last phase.
  f32x4 e[2] = {zero4, zero4}, graw[4] = {zero4, zero4, zero4, zero4};
  float w = 0.0f;
  auto tile_row = [&](int64_t round) { return (round * per_round + (int64_t)blockIdx.x * kHbWaves + wave) * 16 + j; };
  {
    const int64_t m = tile_row(0);
    if (m < n) {
      e[0] = load4(enc + m * 32 + 4 * q);
      e[1] = load4(enc + m * 32 + 16 + 4 * q);
      w = wbuf[m] * g_scale;
      const float* gp = g_pix + (int64_t)ray_of[m] * Kp;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (16 * t + 4 * q < Kp) graw[t] = load4(gp + 16 * t + 4 * q);
    }
  }
  for (int64_t round = 0; round < n_rounds; ++round) {
    const int64_t m = tile_row(round);
    f32x4 g[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) g[t] = graw[t] * w;
    f32x4 h1[4], h2[4], a[4], b[4], c0[2];
    mlp_layer<4, 2>(wf + kIns0 / 4, lane, e, h1);
#pragma unroll
    for (int t = 0; t < 4; ++t) h1[t] = relu4(h1[t]);
    mlp_layer<4, 4>(wf + kIns1 / 4, lane, h1, h2);
#pragma unroll
    for (int t = 0; t < 4; ++t) h2[t] = relu4(h2[t]);
    hb_stage<4>(my_g, q, j, g);
    hb_stage<4>(my_x, q, j, h2);
    const f32x4 e_cur[2] = {e[0], e[1]};
    // stage 1 of the next round
    const int64_t mn = tile_row(round + 1);
    const bool next_valid = round + 1 < n_rounds && mn < n;
    int32_t rid_n = 0;
    e[0] = e[1] = zero4;
    w = 0.0f;
    if (next_valid) {
      e[0] = load4(enc + mn * 32 + 4 * q);
      e[1] = load4(enc + mn * 32 + 16 + 4 * q);
      w = wbuf[mn] * g_scale;
      rid_n = ray_of[mn];
    }
    mlp_layer<4, 4>(wb + kBwd2 / 4, lane, g, a);
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = mask4(a[t], h2[t]);
    __syncthreads();
    hb_accum(gS, xS, q, j, ot, it0, it1, true, acc[0], acc[1]);                 // dW2 tiles 2w, 2w+1
    mlp_layer<4, 4>(wb + kBwd1 / 4, lane, a, b);
#pragma unroll
    for (int t = 0; t < 4; ++t) b[t] = mask4(b[t], h1[t]);
    __syncthreads();
    hb_stage<4>(my_g, q, j, a);
    hb_stage<4>(my_x, q, j, h1);
    mlp_layer<2, 4>(wb + kBwd0 / 4, lane, b, c0);
    if (m < M) {
      store4(denc + m * 32 + 4 * q, c0[0]);
      store4(denc + m * 32 + 16 + 4 * q, c0[1]);
    }
    __syncthreads();
    hb_accum(gS, xS, q, j, ot, it0, it1, true, acc[2], acc[3]);                 // dW1 tiles 2w, 2w+1
    __syncthreads();
    // stage 2 of the next round: the ray row has arrived long ago
#pragma unroll
    for (int t = 0; t < 4; ++t) graw[t] = zero4;
    if (next_valid) {
      const float* gp = g_pix + (int64_t)rid_n * Kp;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (16 * t + 4 * q < Kp) graw[t] = load4(gp + 16 * t + 4 * q);
    }
    hb_stage<4>(my_g, q, j, b);
    hb_stage<2>(my_x, q, j, e_cur);
    __syncthreads();
    hb_accum(gS, xS, q, j, ot, wave & 1, 0, false, acc[4], acc[4]);             // dW0 tile (ot, it = w & 1)
    __syncthreads();
  }
  float4* out = partial + (size_t)blockIdx.x * kHbAccTiles * 64;
  const int ids[5] = {2 * wave, 2 * wave + 1, 16 + 2 * wave, 16 + 2 * wave + 1, 32 + wave};
#pragma unroll
  for (int k = 0; k < 5; ++k) out[ids[k] * 64 + lane] = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
}

// gw2 [Kp,64], gw1 [64,64], gw0 [64,32] = sum over the workgroups' partials (written, not accumulated).
// Element idx of a partial: tile = idx >> 8, lane = (idx >> 2) & 63, r = idx & 3 -> D[4 (lane >> 4) + r][lane & 15].
__global__ void __launch_bounds__(1024) k_head_wgrad_reduce(const float* __restrict__ partial, int n_groups, int Kp,
                                                            float* __restrict__ gw0, float* __restrict__ gw1,
                                                            float* __restrict__ gw2) {
  __shared__ float red[16][64];
  const int e = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int idx = blockIdx.x * 64 + e;
  constexpr int per = kHbAccTiles * 256;
  float s = 0.f;
  int g = slice;
  for (; g + 7 * 16 < n_groups; g += 8 * 16) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(g + 16 * u) * per + idx];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; g < n_groups; g += 16) s += partial[(size_t)g * per + idx];
  red[slice][e] = s;
  __syncthreads();
  if (slice == 0) {
#pragma unroll
    for (int k = 1; k < 16; ++k) s += red[k][e];
    const int tile = idx >> 8, lane = (idx >> 2) & 63, r = idx & 3;
    const int ol = 4 * (lane >> 4) + r, il = lane & 15;
    if (tile < 16) {
      const int o = 16 * (tile >> 2) + ol, i = 16 * (tile & 3) + il;
      if (o < Kp) gw2[o * 64 + i] = s;
    } else if (tile < 32) {
      const int t = tile - 16;
      gw1[(16 * (t >> 2) + ol) * 64 + 16 * (t & 3) + il] = s;
    } else {
      const int t = tile - 32;
      gw0[(16 * (t >> 1) + ol) * 32 + 16 * (t & 1) + il] = s;
    }
  }
}

// ---- NeRF field input gradients (training) -------------------------------------------------------------------
// (g_sigma, g_rgb) -> colour net -> geo features + density logit -> sigma net -> dL/denc, one launch, same
// transposed formulation as k_instance_bwd.  Sections of `packed` (W^T as the A operand, zero-padded):
//   C2T 64 x 32 (3 live inputs)   C1T 64 x 64   C0T 16 x 64 (row i = sigma-net output row i: row 0 zero, row i >= 1
//   is colour-net input column 15 + i)   S1T 64 x 32 (16 live inputs)   S0T 32 x 64.
constexpr int kNbC2 = 0;
constexpr int kNbC1 = kNbC2 + 64 * 32;
constexpr int kNbC0 = kNbC1 + 64 * 64;
constexpr int kNbS1 = kNbC0 + 16 * 64;
constexpr int kNbS0 = kNbS1 + 64 * 32;
constexpr int kNerfBwdFloats = kNbS0 + 32 * 64;      // 11264 floats = 44 KB

struct NerfBwdIO {
  const float *g_sigma, *g_rgb, *rgb, *so, *h1, *c1, *c2;     // inputs
  float *d_o, *dz_c2, *dz_c1, *d_so, *dz_h1, *d_enc;           // outputs: [M,4] [M,64] [M,64] [M,16] [M,64] [M,32]
};

__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_nerf_bwd(NerfBwdIO io, int64_t M, float density_scale,
                                                               const float4* __restrict__ packed) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  for (int i = threadIdx.x; i < kNerfBwdFloats / 4; i += kFieldThreads) wl[i] = packed[i];
  __syncthreads();
  constexpr int kWaves = kFieldThreads / 64;
  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
  const int64_t n_tiles = (M + 15) >> 4;
  const TileSched sched = make_sched(n_tiles, kWaves);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int64_t it = 0, tile = sched.tile(0); tile < sched.hi; tile = sched.tile(++it)) {
    const int64_t m = tile * 16 + j;
    const bool valid = m < M;
    const int64_t mm = valid ? m : M - 1;
    // d(rgb logits): rows 0..2 of a 16-row tile live in lane q == 0
    f32x4 g[2] = {zero4, zero4};
    if (valid && q == 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float c = io.rgb[mm * 3 + r];
        g[0][r] = io.g_rgb[mm * 3 + r] * c * (1.0f - c);
      }
    }
    if (valid && q == 0) store4(io.d_o + m * 4, g[0]);
    f32x4 hh[4], a[4], b[4], ds[2], e0[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) hh[t] = load4(io.c2 + mm * 64 + 16 * t + 4 * q);
    mlp_layer<4, 2>(wl + kNbC2 / 4, lane, g, a);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t] = mask4(a[t], hh[t]);
      hh[t] = load4(io.c1 + mm * 64 + 16 * t + 4 * q);
    }
    if (valid) {
#pragma unroll
      for (int t = 0; t < 4; ++t) store4(io.dz_c2 + m * 64 + 16 * t + 4 * q, a[t]);
    }
    mlp_layer<4, 4>(wl + kNbC1 / 4, lane, a, b);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      b[t] = mask4(b[t], hh[t]);
      hh[t] = load4(io.h1 + mm * 64 + 16 * t + 4 * q);
    }
    if (valid) {
#pragma unroll
      for (int t = 0; t < 4; ++t) store4(io.dz_c1 + m * 64 + 16 * t + 4 * q, b[t]);
    }
    mlp_layer<1, 4>(wl + kNbC0 / 4, lane, b, ds);      // rows 1..15: d(geo); row 0: 0
    ds[1] = zero4;
    if (q == 0) {
      // density: sigma = density_scale * exp(so0), trunc_exp backward = g * exp(clamp(so0, -15, 15))
      const float so0 = io.so[mm * 16];
      ds[0][0] = valid ? io.g_sigma[mm] * density_scale * __expf(fminf(fmaxf(so0, -15.0f), 15.0f)) : 0.f;
    }
    if (valid) store4(io.d_so + m * 16 + 4 * q, ds[0]);
    mlp_layer<4, 2>(wl + kNbS1 / 4, lane, ds, a);
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = mask4(a[t], hh[t]);
    if (valid) {
#pragma unroll
      for (int t = 0; t < 4; ++t) store4(io.dz_h1 + m * 64 + 16 * t + 4 * q, a[t]);
    }
    mlp_layer<2, 4>(wl + kNbS0 / 4, lane, a, e0);
    if (valid) {
#pragma unroll
      for (int t = 0; t < 2; ++t) store4(io.d_enc + m * 32 + 16 * t + 4 * q, e0[t]);
    }
  }
}

// ---- NeRF field: the WHOLE backward in one launch (round 3; the NeRF-stage twin of k_instance_head_bwd) ---------
// Per 16-sample tile a wave recomputes the forward from the saved encoder output and the view direction (sigma net,
// SH, colour net - the forward's own weights and code, so the ReLU masks and the sigmoid are the forward's), runs the
// input-gradient chain of k_nerf_bwd, and accumulates the five weight gradients on the fp32 matrix cores through the
// same LDS staging as k_instance_head_bwd: dWc2 += d_o^T c2 (4 tiles), dWc1 += dz_c2^T c1 (16), dWc0 += dz_c1^T cin (8),
// dWs1 += d_so^T h1 (4), dWs0 += dz_h1^T enc (8) = 40 accumulator tiles, five per wave (wave w: tiles 2w, 2w+1 of dWc1,
// tile w of dWc0 and dWs0, and tile w of dWc2 (w < 4) or tile w - 4 of dWs1 (w >= 4)).  Replaces the activation
// stores of the training forward (1088 -> 128 B per sample), k_nerf_bwd and five k_linear_wgrad launches.
constexpr int kNhFwdFloats = kNerfFloats;

// colour-net input in weight-column order (16 SH, 15 geo, 1 zero) from the register layout of the forward:
// cin0[ks] = SH component 4 ks + q, so[r] = sigma-net row 4 q + r (row 0 is the density logit: column 31 gets 0)
__device__ __forceinline__ void nh_stage_cin(HbStage* __restrict__ tile_base, int q, int j, const f32x4 cin0, const f32x4 so) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) hb_stage_value(tile_base, j, 4 * ks + q, cin0[ks]);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int srow = 4 * q + r;
    hb_stage_value(tile_base, j, srow >= 1 ? 15 + srow : 31, srow >= 1 ? so[r] : 0.0f);
  }
}

__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_nerf_head_bwd(
    const float* __restrict__ enc, const float* __restrict__ dirs, const float* __restrict__ g_sigma,
    const float* __restrict__ g_rgb, int64_t M, float density_scale, const float4* __restrict__ packed_fwd,
    const float4* __restrict__ packed_bwd, float* __restrict__ d_enc, float4* __restrict__ partial,
    float* __restrict__ zero_buf, int64_t zero_n) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  hb_zero_fill(zero_buf, zero_n);
  float4* wf = wl;
  float4* wb = wl + kNhFwdFloats / 4;
  float* gS = reinterpret_cast<float*>(wb + kNerfBwdFloats / 4);
  float* xS = gS + kHbWaves * kHbTileFloats;
  for (int i = threadIdx.x; i < kNhFwdFloats / 4; i += kFieldThreads) wf[i] = packed_fwd[i];
  for (int i = threadIdx.x; i < kNerfBwdFloats / 4; i += kFieldThreads) wb[i] = packed_bwd[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15, wave = threadIdx.x >> 6;
  const int64_t n_tiles = (M + 15) >> 4;
  const int64_t per_round = (int64_t)gridDim.x * kHbWaves;
  const int64_t n_rounds = (n_tiles + per_round - 1) / per_round;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[5] = {zero4, zero4, zero4, zero4, zero4};
  HbStage* my_g = hb_my_tile(gS, wave);
  HbStage* my_x = hb_my_tile(xS, wave);
  const int ot = wave >> 1, it0 = 2 * (wave & 1), it1 = it0 + 1;
  for (int64_t round = 0; round < n_rounds; ++round) {
    const int64_t tile = round * per_round + (int64_t)blockIdx.x * kHbWaves + wave;
    const int64_t m = tile * 16 + j;
    const bool valid = m < M;
    f32x4 e[2] = {zero4, zero4};
    float d0 = 0.f, d1 = 0.f, d2 = 1.f, gs = 0.f, gr0 = 0.f, gr1 = 0.f, gr2 = 0.f;
    if (valid) {
      e[0] = load4(enc + m * 32 + 4 * q);
      e[1] = load4(enc + m * 32 + 16 + 4 * q);
      d0 = dirs[m * 3]; d1 = dirs[m * 3 + 1]; d2 = dirs[m * 3 + 2];
      if (q == 0) {
        gs = g_sigma[m];
        gr0 = g_rgb[m * 3]; gr1 = g_rgb[m * 3 + 1]; gr2 = g_rgb[m * 3 + 2];
      }
    }
    // ---- forward, recomputed (same code as k_nerf_fwd) ----
    f32x4 h1[4], so[1], cin[2], c1[4], c2[4], o[1];
    mlp_layer<4, 2>(wf + kSig0 / 4, lane, e, h1);
#pragma unroll
    for (int t = 0; t < 4; ++t) h1[t] = relu4(h1[t]);
    mlp_layer<1, 4>(wf + kSig1 / 4, lane, h1, so);
    {
      float sh[16];
      sh4(d0, d1, d2, sh);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) cin[0][ks] = select4(q, sh[4 * ks], sh[4 * ks + 1], sh[4 * ks + 2], sh[4 * ks + 3]);
    }
    cin[1] = so[0];
    mlp_layer<4, 2>(wf + kCol0 / 4, lane, cin, c1);
#pragma unroll
    for (int t = 0; t < 4; ++t) c1[t] = relu4(c1[t]);
    mlp_layer<4, 4>(wf + kCol1 / 4, lane, c1, c2);
#pragma unroll
    for (int t = 0; t < 4; ++t) c2[t] = relu4(c2[t]);
    mlp_layer<1, 4>(wf + kCol2 / 4, lane, c2, o);
    // ---- d(rgb logits): rows 0..2 of a 16-row tile live in lanes q == 0 ----
    f32x4 g[2] = {zero4, zero4};
    if (valid && q == 0) {
      const float c0v = __frcp_rn(1.0f + __expf(-o[0][0])), c1v = __frcp_rn(1.0f + __expf(-o[0][1])),
                  c2v = __frcp_rn(1.0f + __expf(-o[0][2]));
      g[0][0] = gr0 * c0v * (1.0f - c0v);
      g[0][1] = gr1 * c1v * (1.0f - c1v);
      g[0][2] = gr2 * c2v * (1.0f - c2v);
    }
    // phase 1: dWc2 (16 x 64, 3 live rows) += d_o^T c2          [waves 0..3: tile it = wave]
    hb_stage<1>(my_g, q, j, g);
    hb_stage<4>(my_x, q, j, c2);
    f32x4 a[4], b[4], ds[2], e0[2];
    mlp_layer<4, 2>(wb + kNbC2 / 4, lane, g, a);
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = mask4(a[t], c2[t]);
    __syncthreads();
    if (wave < 4) hb_accum(gS, xS, q, j, 0, wave, 0, false, acc[4], acc[4]);
    mlp_layer<4, 4>(wb + kNbC1 / 4, lane, a, b);
#pragma unroll
    for (int t = 0; t < 4; ++t) b[t] = mask4(b[t], c1[t]);
    __syncthreads();
    // phase 2: dWc1 += dz_c2^T c1
    hb_stage<4>(my_g, q, j, a);
    hb_stage<4>(my_x, q, j, c1);
    mlp_layer<1, 4>(wb + kNbC0 / 4, lane, b, ds);      // rows 1..15: d(geo); row 0: 0
    ds[1] = zero4;
    if (q == 0) ds[0][0] = valid ? gs * density_scale * __expf(fminf(fmaxf(so[0][0], -15.0f), 15.0f)) : 0.f;
    __syncthreads();
    hb_accum(gS, xS, q, j, ot, it0, it1, true, acc[0], acc[1]);
    mlp_layer<4, 2>(wb + kNbS1 / 4, lane, ds, a);
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = mask4(a[t], h1[t]);
    __syncthreads();
    // phase 3: dWc0 (64 x 32) += dz_c1^T cin
    hb_stage<4>(my_g, q, j, b);
    nh_stage_cin(my_x, q, j, cin[0], so[0]);
    mlp_layer<2, 4>(wb + kNbS0 / 4, lane, a, e0);
    if (valid) {
      store4(d_enc + m * 32 + 4 * q, e0[0]);
      store4(d_enc + m * 32 + 16 + 4 * q, e0[1]);
    }
    __syncthreads();
    hb_accum(gS, xS, q, j, ot, wave & 1, 0, false, acc[2], acc[2]);
    __syncthreads();
    // phase 4: dWs1 (16 x 64) += d_so^T h1                     [waves 4..7: tile it = wave - 4]
    hb_stage<1>(my_g, q, j, ds);
    hb_stage<4>(my_x, q, j, h1);
    __syncthreads();
    if (wave >= 4) hb_accum(gS, xS, q, j, 0, wave - 4, 0, false, acc[4], acc[4]);
    __syncthreads();
    // phase 5: dWs0 (64 x 32) += dz_h1^T enc
    hb_stage<4>(my_g, q, j, a);
    hb_stage<2>(my_x, q, j, e);
    __syncthreads();
    hb_accum(gS, xS, q, j, ot, wave & 1, 0, false, acc[3], acc[3]);
    __syncthreads();
  }
  float4* out = partial + (size_t)blockIdx.x * kHbAccTiles * 64;
  // tile ids: 0..15 dWc1 (ot, it), 16..23 dWc0, 24..31 dWs0, 32..35 dWc2 (it), 36..39 dWs1 (it)
  const int ids[5] = {2 * wave, 2 * wave + 1, 16 + wave, 24 + wave, 32 + wave};
#pragma unroll
  for (int k = 0; k < 5; ++k) out[ids[k] * 64 + lane] = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
}

// sums the workgroups' partials into gwc2 [16,64] (3 live rows), gwc1 [64,64], gwc0 [64,31],
// gws1 [16,64], gws0 [64,32] - written, not accumulated.
__global__ void __launch_bounds__(1024) k_nerf_head_wgrad_reduce(const float* __restrict__ partial, int n_groups,
                                                                 float* __restrict__ gwc2, float* __restrict__ gwc1,
                                                                 float* __restrict__ gwc0, float* __restrict__ gws1,
                                                                 float* __restrict__ gws0) {
  __shared__ float red[16][64];
  const int e = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int idx = blockIdx.x * 64 + e;
  constexpr int per = kHbAccTiles * 256;
  float s = 0.f;
  int g = slice;
  for (; g + 7 * 16 < n_groups; g += 8 * 16) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(g + 16 * u) * per + idx];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; g < n_groups; g += 16) s += partial[(size_t)g * per + idx];
  red[slice][e] = s;
  __syncthreads();
  if (slice == 0) {
#pragma unroll
    for (int k = 1; k < 16; ++k) s += red[k][e];
    const int tile = idx >> 8, lane = (idx >> 2) & 63, r = idx & 3;
    const int ol = 4 * (lane >> 4) + r, il = lane & 15;
    if (tile < 16) gwc1[(16 * (tile >> 2) + ol) * 64 + 16 * (tile & 3) + il] = s;
    else if (tile < 24) {                   // [64,31] as nn.Linear stores it (the padding column 31 is dropped)
      const int col = 16 * ((tile - 16) & 1) + il;
      if (col < 31) gwc0[(16 * ((tile - 16) >> 1) + ol) * 31 + col] = s;
    }
    else if (tile < 32) gws0[(16 * ((tile - 24) >> 1) + ol) * 32 + 16 * ((tile - 24) & 1) + il] = s;
    else if (tile < 36) gwc2[ol * 64 + 16 * (tile - 32) + il] = s;
    else gws1[ol * 64 + 16 * (tile - 36) + il] = s;
  }
}

// Device-side weight packing for training (the weights change every step; the host packers above would cost a
// device->host->device round trip per step).  One thread per packed bf16 pair position; same layout and
// rounding as pack_section_bf16.  transpose: the section holds W^T of the row-major [n_rows_w, n_cols_w] weight.
struct PackJob {
  const float* W;
  int w_rows, w_cols;      // row-major weight as stored by nn.Linear: [out, in]
  int n_out, n_in;         // logical section size (rows = MFMA output rows, cols = inputs)
  int n_mt, n_s;
  int transpose;
  int dst_off;             // float offset of the section in the packed buffer
  int kmode;               // 0: k-slot = feature 16*(ks>>2)+4q+(ks&3); 1: colour-net input (kidx_color_in)
  int row_min, row_shift;  // transpose only: rows below row_min are zero, row i reads source column i + row_shift
  int bwd;                 // which output buffer
};
struct PackJobs {
  PackJob j[10];
};

__device__ __forceinline__ uint16_t bf16_rne_dev(float x) {
  uint32_t u = __float_as_uint(x);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

__global__ void __launch_bounds__(256) k_pack_weights(PackJobs jobs, float* __restrict__ packed_fwd,
                                                      float* __restrict__ packed_bwd) {
  const PackJob J = jobs.j[blockIdx.y];
  const int total = J.n_mt * J.n_s * 64 * 8;
  float* base = (J.bwd ? packed_bwd : packed_fwd) + J.dst_off;
  uint16_t* dst = reinterpret_cast<uint16_t*>(base);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int e = i & 7, lane = (i >> 3) & 63, rest = i >> 9;
    const int st = rest % J.n_s, mt = rest / J.n_s;
    const int row = 16 * mt + (lane & 15);
    const int qq = lane >> 4;
    int col = 16 * (2 * st + (e >> 2)) + 4 * qq + (e & 3);
    if (J.kmode == 1) {                                  // colour-net input: 4 SH slots, then sigma-net rows (row 0 unused)
      const int r = 4 * qq + (e & 3);
      col = (e >> 2) == 0 ? 4 * (e & 3) + qq : (r >= 1 ? 15 + r : -1);
    }
    float v = 0.f;
    if (row < J.n_out && col >= 0 && col < J.n_in) {
      if (!J.transpose) v = J.W[(size_t)row * J.w_cols + col];
      else if (row >= J.row_min) v = J.W[(size_t)col * J.w_cols + row + J.row_shift];
    }
#if INR_MLP_FP32
    // exact-fp32 build (round 5: the training entry points too): the fragment order of pack_section_f32 - k-step
    // ks = 4 (2 st + (e >> 2)) + (e & 3) of the bf16 layout's element (st, e), value (mt, ks, lane) at frag_pos()
    (void)dst;
    base[frag_pos(mt, 4 * (2 * st + (e >> 2)) + (e & 3), lane, 8 * J.n_s)] = v;
#else
    const uint16_t hi = bf16_rne_dev(v);
    const uint16_t lo = bf16_rne_dev(v - __uint_as_float((uint32_t)hi << 16));
    dst[((((size_t)(mt * J.n_s + st) * 2 + 0) * 64 + lane) * 8) + e] = hi;
    dst[((((size_t)(mt * J.n_s + st) * 2 + 1) * 64 + lane) * 8) + e] = lo;
#endif
  }
}


// ---- instance logits rendered in place (inference) ---------------------------------------------------------
// out[ray][ch] = sum_k w(ray,k) * logits(x(ray,k))[ch] without ever writing the [M, K] logits.  A WORKGROUP owns a
// 16-ray group of the patch-interleaved layout; its eight waves take the group's steps round robin (wave w: steps w,
// w + 8, ...), so that at any time the CU works on eight consecutive depths of one 4x4 patch - the access pattern the
// plain field kernel owes its L1 hit rate to (round 1 / early round 2 gave each wave a group of its own: eight
// unrelated patches per CU, 7.8 ms for 37 M samples).  MFMA column j is FIXED to ray j (the slot of its k-th sample is
// base + sum_i min(c_i, k) + #{i < j: c_i > k}), w * logits accumulates in the MFMA output registers (16 per lane), and
// the eight partial sums meet in LDS when the group is done: one barrier per group, two LDS buffers by group parity
// (waves 0..3 add up and store group g while waves 4..7 already run group g + 1).  Steps where every live ray of the
// group has w == 0 (behind the termination point) skip the gather and the MLP.  x_is_01: the march writer already
// normalised the coordinates (table feed).
// kO: upstream's -O numerics (opt-in) - the table is the fp16 copy and the MLP GEMMs take one fp16 MFMA pass.
template <int K_MT, bool kO = false>
__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_instance_render(
    const float* __restrict__ x, const int32_t* __restrict__ rays, const float* __restrict__ wbuf, int64_t N, int64_t M,
    float bound, const float2* __restrict__ emb, uint32_t emb_bytes, GridDesc G, const float4* __restrict__ packed,
    float* __restrict__ extra_out, int x_is_01, unsigned long long* __restrict__ cursors) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  __shared__ int64_t drawn[2];
  constexpr int K = K_MT * 16;
  constexpr int kStage = (kIns2 + K * 64) / 4;
  constexpr int kWaves = kFieldThreads / 64;
  for (int i = threadIdx.x; i < kStage; i += kFieldThreads) wl[i] = packed[i];
  LevelRec* recs = reinterpret_cast<LevelRec*>(wl + kStage);
  float4* red = wl + kStage + kLevelRecBytes / 16;        // [2][kWaves][K_MT][64] float4
  stage_level_recs(G, recs);
  __syncthreads();

  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15, wave = threadIdx.x >> 6;
  const float rb = 2.0f * bound;
  const float x_add = x_is_01 ? 0.0f : bound, x_div = x_is_01 ? 1.0f : rb;
  // a WORKGROUP per group, drawn dynamically (GroupDraw): thread 0 requests the next group while this one is evaluated
  // and hands it over through LDS behind the barrier every group ends with.  (kGroupDraw == 1 here.)
  const int64_t n_groups = (N + 15) >> 4;
  GroupDraw gd;
  gd.init(cursors, 1);
  const bool all_hashed[4] = {slot_all_hashed(G, 0), slot_all_hashed(G, 1), slot_all_hashed(G, 2), slot_all_hashed(G, 3)};
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)emb, 0, (int)emb_bytes, 0x00020000);

  if (threadIdx.x == 0) drawn[0] = gd.draw();
  __syncthreads();
  int parity = 0;
  for (int64_t grp = drawn[0]; grp < n_groups; grp = drawn[parity ^= 1]) {
    if (threadIdx.x == 0) drawn[parity ^ 1] = gd.draw();
    const int64_t ray = grp * 16 + j;
    const int cnt = ray < N ? rays[ray * 3 + 2] : 0;
    const int64_t S0 = rays[grp * 16 * 3 + 1];             // slot base of the group (offset of its first ray)
    int gtot = cnt, kmax = cnt;                            // group total (to honour a dropped group), longest ray
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      gtot += __shfl_xor(gtot, d, 64);
      kmax = max(kmax, __shfl_xor(kmax, d, 64));
    }
    if (S0 + gtot > M) kmax = 0;
    f32x4 acc[K_MT];
#pragma unroll
    for (int mt = 0; mt < K_MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the sample of (ray j, step k): requested one step of this wave ahead of its use
    auto request = [&](int k, float& w, float& x0, float& x1, float& x2) {
      int below = min(cnt, k);                             // samples of ray i before step k, summed over the group
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) below += __shfl_xor(below, d, 64);
      const unsigned field = (unsigned)(__ballot(k < cnt) & 0xFFFFull);
      const bool active = k < cnt;
      const int64_t slot = active ? S0 + below + __popc(field & ((1u << j) - 1u)) : 0;
      w = active ? wbuf[slot] : 0.0f;
      x0 = x[slot * 3 + 0]; x1 = x[slot * 3 + 1]; x2 = x[slot * 3 + 2];
    };
    float w = 0.f, x0 = 0.f, x1 = 0.f, x2 = 0.f;
    if (wave < kmax) request(wave, w, x0, x1, x2);
    for (int k = wave; k < kmax; k += kWaves) {
      float wn = 0.f, xn0 = 0.f, xn1 = 0.f, xn2 = 0.f;
      if (k + kWaves < kmax) request(k + kWaves, wn, xn0, xn1, xn2);
      if (__ballot(w != 0.0f) != 0ull) {                   // else: the whole group is past its termination points
        const float p0 = (x0 + x_add) / x_div, p1 = (x1 + x_add) / x_div, p2 = (x2 + x_add) / x_div;
        f32x4 enc[2];
        {
          Gathered g;
          uint32_t rec_off = (uint32_t)q * 4u * (uint32_t)sizeof(LevelRec);
          asm volatile("" : "+v"(rec_off));
          issue_gathers<kO>(reinterpret_cast<const LevelRec*>(reinterpret_cast<const char*>(recs) + rec_off), all_hashed,
                            rsrc, p0, p1, p2, g);
          __builtin_amdgcn_sched_barrier(0);
          blend<kO>(g, enc[0], enc[1]);
        }
        f32x4 h1[4], h2[4], o[K_MT];
        mlp_layer<4, 2, kO>(wl + kIns0 / 4, lane, enc, h1);
#pragma unroll
        for (int t = 0; t < 4; ++t) h1[t] = relu4(h1[t]);
        mlp_layer<4, 4, kO>(wl + kIns1 / 4, lane, h1, h2);
#pragma unroll
        for (int t = 0; t < 4; ++t) h2[t] = relu4(h2[t]);
        mlp_layer<K_MT, 4, kO>(wl + kIns2 / 4, lane, h2, o);
#pragma unroll
        for (int mt = 0; mt < K_MT; ++mt) {
          acc[mt][0] = fmaf(w, o[mt][0], acc[mt][0]); acc[mt][1] = fmaf(w, o[mt][1], acc[mt][1]);
          acc[mt][2] = fmaf(w, o[mt][2], acc[mt][2]); acc[mt][3] = fmaf(w, o[mt][3], acc[mt][3]);
        }
      }
      w = wn; x0 = xn0; x1 = xn1; x2 = xn2;
    }
    float4* mine = red + ((size_t)(parity * kWaves + wave) * K_MT) * 64;
#pragma unroll
    for (int mt = 0; mt < K_MT; ++mt) mine[mt * 64 + lane] = make_float4(acc[mt][0], acc[mt][1], acc[mt][2], acc[mt][3]);
    __syncthreads();                                       // measured free: 14.5 ms per frame with and without it
    if (threadIdx.x < K_MT * 64 && ray < N) {              // thread t: tile row block t >> 6, lane position t & 63
      const float4* part = red + (size_t)parity * kWaves * K_MT * 64 + threadIdx.x;
      float4 sum = part[0];
#pragma unroll
      for (int wv = 1; wv < kWaves; ++wv) {
        const float4 v = part[(size_t)wv * K_MT * 64];
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
      }
      const int32_t rid = rays[ray * 3];
      *reinterpret_cast<float4*>(extra_out + (int64_t)rid * K + 16 * (threadIdx.x >> 6) + 4 * q) = sum;
    }
  }
}


// ---- whole-ray rendering with early termination (inference) --------------------------------------------------
// Field evaluation AND alpha compositing in one kernel: one wave owns a 16-ray group of the patch-interleaved
// layout for all its steps, MFMA column j is fixed to ray j, the compositing state (T, colour, opacity, depth)
// lives in the registers of lane (q = 0, j), sigma / rgb never reach HBM, and - the point - a step whose rays
// have all dropped below T_thresh is not evaluated at all: the group stops as soon as its last ray is opaque.
// This is what upstream's alive-ray loop buys on trained (opaque) scenes, without its per-iteration host sync.
// On a transparent scene it evaluates exactly the samples of the two-kernel path.  weights (nullable) receives
// w per sample (0 for skipped samples) for k_instance_render; evaluated[0] += samples of the steps that were evaluated
// (all rays of the group that have a sample at such a step, terminated or not).
// (Round 3 tried the k_instance_render pattern here - a WORKGROUP owns the group, its eight waves take eight consecutive
//  steps, wave 0 composites a round at a time from LDS, one round evaluated speculatively: 1.18x instead of 1.25-1.37x
//  the two-kernel path's time per evaluated sample, but termination at 8-16-step granularity: opaque scene 2.91 vs 0.94
//  ms (10.2 M instead of 0.6 M samples evaluated), half-trained scene 15.3 vs 17.1 ms with the two-kernel path at 13.6.
//  There is no skippable fraction at which it is the best of the three paths - profiles/r03_NOTES.txt 8 - so the
//  wave-owned kernel stays.)
template <bool kO = false>      // kO: upstream's -O numerics (opt-in) - fp16 table copy, one fp16 MFMA pass per MLP GEMM
__global__ void __launch_bounds__(kFieldThreads, kFieldMinWaves) k_nerf_render(
    const float* __restrict__ x, const float* __restrict__ deltas, const int32_t* __restrict__ rays,
    const float* __restrict__ rays_d, int64_t N, int64_t M, float bound, const float2* __restrict__ emb,
    uint32_t emb_bytes, GridDesc G, const float4* __restrict__ packed, float density_scale, float T_thresh,
    float* __restrict__ weights_sum, float* __restrict__ depth, float* __restrict__ image, float* __restrict__ wbuf,
    unsigned long long* __restrict__ evaluated, int x_is_01) {
  extern __shared__ __attribute__((aligned(16))) float4 wl[];
  constexpr int kStage = kNerfFloats / 4;
  for (int i = threadIdx.x; i < kStage; i += kFieldThreads) wl[i] = packed[i];
  LevelRec* recs = reinterpret_cast<LevelRec*>(wl + kStage);
  stage_level_recs(G, recs);
  __syncthreads();

  const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
  const float rb = 2.0f * bound;
  const float x_add = x_is_01 ? 0.0f : bound, x_div = x_is_01 ? 1.0f : rb;   // table feed: already normalised
  const bool all_hashed[4] = {slot_all_hashed(G, 0), slot_all_hashed(G, 1), slot_all_hashed(G, 2), slot_all_hashed(G, 3)};
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)emb, 0, (int)emb_bytes, 0x00020000);
  unsigned long long n_eval = 0;
  // dynamic group schedule (GroupDraw): the wave draws its next group(s) while it evaluates the current one
  const int64_t n_groups = (N + 15) >> 4;
  GroupDraw gd;
  gd.init(evaluated + 1, kGroupPools);
  auto draw = [&]() -> int64_t {
    int64_t g = 0;
    if (lane == 0) g = gd.draw();
    return ((int64_t)__builtin_amdgcn_readfirstlane((int)(g >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
  };

  int64_t base = draw(), base_next = draw();      // the next draw is always in flight while a batch is evaluated
  for (int sub = 0;;) {
    if (sub == kGroupDraw) {
      base = base_next;
      base_next = draw();
      sub = 0;
    }
    const int64_t grp = base + sub++;
    if (grp >= n_groups) {
      if (base >= n_groups) break;                 // the XCD's share is used up
      sub = kGroupDraw;                            // the frame ends inside this batch
      continue;
    }
    const int64_t ray = grp * 16 + j;
    const bool has_ray = ray < N;
    const int cnt = has_ray ? rays[ray * 3 + 2] : 0;
    int64_t S = rays[grp * 16 * 3 + 1];
    int gtot = cnt;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) gtot += __shfl_xor(gtot, d, 64);
    const bool fits = S + gtot <= M;
    const int64_t rc = has_ray ? ray : N - 1;
    float sh[16];
    sh4(rays_d[rc * 3], rays_d[rc * 3 + 1], rays_d[rc * 3 + 2], sh);   // the direction is constant along a ray
    f32x4 cin0;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) cin0[ks] = select4(q, sh[4 * ks], sh[4 * ks + 1], sh[4 * ks + 2], sh[4 * ks + 3]);
    float T = 1.0f, cr = 0.f, cg = 0.f, cb = 0.f, ws = 0.f, tt = 0.f, dsum = 0.f;   // meaningful in lanes q == 0
    bool done = false;
    // the slot of a step depends on the counts only: the coordinates of step k + 1 are requested while step k is
    // evaluated (they stream from HBM; a step used to start with that round trip)
    float xn0 = 0.f, xn1 = 0.f, xn2 = 0.f;
    if (fits && gtot > 0) {
      const unsigned f0 = (unsigned)(__ballot(0 < cnt) & 0xFFFFull);
      const int64_t m0 = ((f0 >> j) & 1u) ? S + __popc(f0 & ((1u << j) - 1u)) : 0;
      xn0 = x[m0 * 3 + 0]; xn1 = x[m0 * 3 + 1]; xn2 = x[m0 * 3 + 2];
    }
    for (int k = 0; fits; ++k) {
      const unsigned long long bal = __ballot(k < cnt);
      const unsigned field = (unsigned)(bal & 0xFFFFull);
      if (field == 0) break;
      const unsigned donef = (unsigned)(__ballot(done) & 0xFFFFull);
      const unsigned livef = field & ~donef;
      const bool active = (field >> j) & 1u, live = (livef >> j) & 1u;
      const int64_t slot = S + __popc(field & ((1u << j) - 1u));
      S += __popc(field);
      const float xr0 = xn0, xr1 = xn1, xr2 = xn2;
      {
        // only while a ray of the group is alive (alive at k + 1 implies alive at k): an opaque group must not stream
        // the coordinates of the samples it skips
        const unsigned fn = livef != 0 ? (unsigned)(__ballot(k + 1 < cnt) & 0xFFFFull) : 0u;
        if (fn != 0) {
          const int64_t mn = ((fn >> j) & 1u) ? S + __popc(fn & ((1u << j) - 1u)) : 0;
          xn0 = x[mn * 3 + 0]; xn1 = x[mn * 3 + 1]; xn2 = x[mn * 3 + 2];
        }
      }
      if (livef == 0) {                                   // every remaining ray of the group is opaque
        if (!wbuf) break;                                 // nothing left to do for this group
        if (active && q == 0) wbuf[slot] = 0.0f;          // the instance render reads a weight for every sample
        continue;
      }
      // group-level accounting, the same quantity the two-kernel path's compositing counts as NOT skippable: every
      // sample of a step that is evaluated at all (a terminated ray inside a live group still rides through the
      // MFMA tile).  Counting live rays only made infer_mode="auto" compare two different fractions (round-2 advisor).
      if (lane == 0) n_eval += __popc(field);
      const float2 dl = (q == 0 && live) ? reinterpret_cast<const float2*>(deltas)[slot] : make_float2(0.f, 0.f);
      const float x0 = (xr0 + x_add) / x_div, x1 = (xr1 + x_add) / x_div, x2 = (xr2 + x_add) / x_div;
      f32x4 enc[2];
      {
        Gathered g;
        uint32_t rec_off = (uint32_t)q * 4u * (uint32_t)sizeof(LevelRec);
        asm volatile("" : "+v"(rec_off));
        issue_gathers<kO>(reinterpret_cast<const LevelRec*>(reinterpret_cast<const char*>(recs) + rec_off), all_hashed, rsrc,
                          x0, x1, x2, g);
        __builtin_amdgcn_sched_barrier(0);
        blend<kO>(g, enc[0], enc[1]);
      }
      f32x4 h1[4], h2[1];
      mlp_layer<4, 2, kO>(wl + kSig0 / 4, lane, enc, h1);
#pragma unroll
      for (int t = 0; t < 4; ++t) h1[t] = relu4(h1[t]);
      mlp_layer<1, 4, kO>(wl + kSig1 / 4, lane, h1, h2);
      f32x4 cin[2], c1[4], c2[4], o[1];
      cin[0] = cin0;
      cin[1] = h2[0];
      mlp_layer<4, 2, kO>(wl + kCol0 / 4, lane, cin, c1);
#pragma unroll
      for (int t = 0; t < 4; ++t) c1[t] = relu4(c1[t]);
      mlp_layer<4, 4, kO>(wl + kCol1 / 4, lane, c1, c2);
#pragma unroll
      for (int t = 0; t < 4; ++t) c2[t] = relu4(c2[t]);
      mlp_layer<1, 4, kO>(wl + kCol2 / 4, lane, c2, o);
      if (q == 0 && active) {
        float w = 0.0f;
        if (live) {
          const float sg = __expf(h2[0][0]) * density_scale;
          const float alpha = 1.0f - expf(-sg * dl.x);
          w = alpha * T;
          cr += w * __frcp_rn(1.0f + __expf(-o[0][0]));
          cg += w * __frcp_rn(1.0f + __expf(-o[0][1]));
          cb += w * __frcp_rn(1.0f + __expf(-o[0][2]));
          tt += dl.y;
          dsum += w * tt;
          ws += w;
          T *= 1.0f - alpha;
          if (T < T_thresh) done = true;
        }
        if (wbuf) wbuf[slot] = w;
      }
    }
    if (q == 0 && has_ray) {
      const int32_t rid = rays[ray * 3];
      weights_sum[rid] = ws; depth[rid] = dsum;
      image[rid * 3] = cr; image[rid * 3 + 1] = cg; image[rid * 3 + 2] = cb;
    }
  }
  if (lane == 0 && n_eval) atomicAdd(evaluated, n_eval);
}

// ---- host-side packing into fragment order ------------------------------------------------------
// W is [n_out, n_in] row-major.  kidx(ks, q) -> input column (or -1 for a zero slot).
static inline uint16_t bf16_rne(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// bf16 split layout: [mt][step][hi|lo][lane][8]; kidx(step*8 + e style) is expressed through the same
// k-step functions as the fp32 layout: slot e of step s is fp32 k-step 4*(2s + (e>>2)) + (e&3).
template <class KIdx>
static void pack_section_bf16(float* dst_f, const float* W, int n_out, int n_in, int n_mt, int n_ks, KIdx kidx) {
  uint16_t* dst = reinterpret_cast<uint16_t*>(dst_f);
  const int n_s = n_ks / 8;
  for (int mt = 0; mt < n_mt; ++mt)
    for (int st = 0; st < n_s; ++st)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int row = 16 * mt + (lane & 15);
          const int col = kidx(4 * (2 * st + (e >> 2)) + (e & 3), lane >> 4);
          float v = 0.f;
          if (row < n_out && col >= 0 && col < n_in) v = W[(size_t)row * n_in + col];
          const uint16_t hi = bf16_rne(v);
          const uint16_t lo = bf16_rne(v - bf16_to_f32(hi));
          dst[((((size_t)(mt * n_s + st) * 2 + 0) * 64 + lane) * 8) + e] = hi;
          dst[((((size_t)(mt * n_s + st) * 2 + 1) * 64 + lane) * 8) + e] = lo;
        }
}

// fp16 variant of the same layout for the opt-in single-pass MLP: the head slot holds the weight rounded to fp16, the
// remainder slot is unused (zero).
template <class KIdx>
static void pack_section_f16(float* dst_f, const float* W, int n_out, int n_in, int n_mt, int n_ks, KIdx kidx) {
  uint16_t* dst = reinterpret_cast<uint16_t*>(dst_f);
  const int n_s = n_ks / 8;
  for (int mt = 0; mt < n_mt; ++mt)
    for (int st = 0; st < n_s; ++st)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int row = 16 * mt + (lane & 15);
          const int col = kidx(4 * (2 * st + (e >> 2)) + (e & 3), lane >> 4);
          float v = 0.f;
          if (row < n_out && col >= 0 && col < n_in) v = W[(size_t)row * n_in + col];
          const _Float16 h = (_Float16)v;                 // round to nearest even
          uint16_t bits;
          memcpy(&bits, &h, 2);
          dst[((((size_t)(mt * n_s + st) * 2 + 0) * 64 + lane) * 8) + e] = bits;
          dst[((((size_t)(mt * n_s + st) * 2 + 1) * 64 + lane) * 8) + e] = 0;
        }
}

template <class KIdx>
static void pack_section_f32(float* dst, const float* W, int n_out, int n_in, int n_mt, int n_ks, KIdx kidx) {
  for (int mt = 0; mt < n_mt; ++mt)
    for (int ks = 0; ks < n_ks; ++ks)
      for (int lane = 0; lane < 64; ++lane) {
        const int row = 16 * mt + (lane & 15);
        const int col = kidx(ks, lane >> 4);
        float v = 0.f;
        if (row < n_out && col >= 0 && col < n_in) v = W[(size_t)row * n_in + col];
        dst[frag_pos(mt, ks, lane, n_ks)] = v;
      }
}
template <class KIdx>
static void pack_section(float* dst, const float* W, int n_out, int n_in, int n_mt, int n_ks, KIdx kidx) {
#if INR_MLP_FP32
  pack_section_f32(dst, W, n_out, n_in, n_mt, n_ks, kidx);
#else
  pack_section_bf16(dst, W, n_out, n_in, n_mt, n_ks, kidx);
#endif
}
static int kidx_enc(int ks, int q) { return 16 * (ks >> 2) + 4 * q + (ks & 3); }      // encoder features
static int kidx_hidden(int ks, int q) { return 16 * (ks >> 2) + 4 * q + (ks & 3); }   // previous D registers
static int kidx_color_in(int ks, int q) {
  if (ks < 4) return 4 * ks + q;                 // sh component
  const int row = 4 * q + (ks - 4);              // sigma-net output row feeding this slot
  return row >= 1 ? 16 + row - 1 : -1;           // row 0 is the raw density: not an input
}

// Persistent grid.  MEASURED (tools/field_probe.py, 37 M samples, MI355X): the kernel is fastest with
// 8-12 waves per CU - 4: 10.3 ms, 6: 8.3, 8: 6.8, 12: 6.8, 16: 7.1-7.2 - because every resident wave adds a
// tile's worth of table lines to the L1/L2 working set; beyond ~2 waves/SIMD the extra latency hiding is
// worth less than the cache it costs (a per-wave double-buffered pipeline at 8 waves/CU measures 6.95 ms
// for the same reason).  So: ONE 512-thread workgroup per CU, all co-resident, no tail round.
constexpr int kFieldBlocksPerCU = 1;

template <class Kern>
static int grid_for(Kern kern, size_t lds_bytes, int64_t n_tiles) {
  // occupancy of (kernel, LDS size) is a constant of the build: ask the runtime once per pair
  struct Entry { const void* kern; size_t lds; int fit; };
  static Entry cache[64];
  static int n_cached = 0;
  const int cus = cu_count();
  int fit = 0;
  for (int i = 0; i < n_cached; ++i)
    if (cache[i].kern == (const void*)kern && cache[i].lds == lds_bytes) fit = cache[i].fit;
  if (fit < 1) {
    fit = kFieldBlocksPerCU;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kern, kFieldThreads, lds_bytes) != hipSuccess || fit < 1) fit = 1;
    if (n_cached < 64) cache[n_cached++] = Entry{(const void*)kern, lds_bytes, fit};
  }
  // (two workgroups per CU for small launches - training batches, ~6 tiles per wave - measured in round 3: no change,
  //  92.2 vs 90.9 us per 209 k samples; those launches are bound by the L2 fills of a cold table, not by latency)
  const int per_cu = std::min(fit, kFieldBlocksPerCU);
  const int64_t want = (n_tiles + kFieldThreads / 64 - 1) / (kFieldThreads / 64);
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)cus * per_cu));
}

// Cursors of the hybrid schedule (TileWalk): a ring of kStealRing sets per device, the next one zeroed on the launch's
// stream right before the launch.  Launches on different streams (FramePipeline) never share a set: every set carries
// the event of the launch that last used it, and a launch that is handed a set whose previous user has not finished
// (more than kStealRing field kernels pending at once) makes its stream wait for that event first (round-3 advisor: the
// set used to be re-zeroed under the running kernel - tiles skipped or duplicated without an error).
constexpr int kStealRing = 16;
struct StealSet {
  unsigned long long* cursors = nullptr;
  int dev = -1, slot = -1;
};
struct StealRing {
  std::atomic<unsigned long long*> base{nullptr};
  hipEvent_t ev[kStealRing] = {};
  bool used[kStealRing] = {};
};
static StealRing g_steal[64];
static std::mutex g_steal_mu;
static bool stream_is_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}
// Never called while `s` is capturing (round-4 advisor): a graph would bake ONE ring slot and its memset into every
// replay, with no event protection - an eager launch on another stream that draws the same slot could re-zero the cursors
// under the running replay (tiles skipped or duplicated, no error).  Captured launches take the static deal instead.
static StealSet steal_cursors(hipStream_t s) {
  static std::atomic<unsigned> turn{0};
  StealSet out;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return out;
  StealRing& R = g_steal[dev];
  if (!R.base.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lock(g_steal_mu);
    if (!R.base.load(std::memory_order_relaxed)) {
      void* p = nullptr;
      if (hipMalloc(&p, (size_t)kStealRing * kStealOwners * sizeof(unsigned long long)) != hipSuccess) {
        set_error("hybrid schedule: hipMalloc of the cursor ring failed");
        return out;
      }
      R.base.store((unsigned long long*)p, std::memory_order_release);
    }
  }
  const int slot = (int)(turn.fetch_add(1) % kStealRing);
  unsigned long long* p = R.base.load(std::memory_order_acquire) + (size_t)slot * kStealOwners;
  {
    std::lock_guard<std::mutex> lock(g_steal_mu);
    if (R.used[slot] && !stream_is_capturing(s) && hipEventQuery(R.ev[slot]) == hipErrorNotReady &&
        hipStreamWaitEvent(s, R.ev[slot], 0) != hipSuccess) {
      set_error("hybrid schedule: hipStreamWaitEvent failed");
      return out;
    }
  }
  if (hipMemsetAsync(p, 0, kStealOwners * sizeof(unsigned long long), s) != hipSuccess) {
    set_error("hybrid schedule: hipMemsetAsync failed");
    return out;
  }
  out.cursors = p;
  out.dev = dev;
  out.slot = slot;
  return out;
}
// after the launch that draws from the set: its completion event (not inside a stream capture: a captured event says
// nothing about a replay - captured steps are small launches and never take the hybrid schedule anyway)
static void steal_release(const StealSet& st, hipStream_t s) {
  if (!st.cursors || stream_is_capturing(s)) return;
  std::lock_guard<std::mutex> lock(g_steal_mu);
  StealRing& R = g_steal[st.dev];
  if (!R.ev[st.slot] && hipEventCreateWithFlags(&R.ev[st.slot], hipEventDisableTiming) != hipSuccess) return;
  R.used[st.slot] = hipEventRecord(R.ev[st.slot], s) == hipSuccess;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: once per (kernel call site, device), not once per
// process (round-3 advisor: a process that trained on a second GPU launched there without the attribute)
struct AttrOnce {
  std::atomic<bool> done[64] = {};
  template <typename K>
  bool ensure(K kern, size_t lds) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (done[dev].load(std::memory_order_acquire)) return true;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
    done[dev].store(true, std::memory_order_release);
    return true;
  }
};

// ---- host side of the field exports --------------------------------------------------------------------------------
// Hash table of a field launch: its descriptor and its size in bytes as stored (fp32 [T,2], or the fp16 copy), which the
// 32-bit gather offsets must be able to address.  `what` names the export in the error message.
struct FieldTable {
  GridDesc G;
  const float2* emb;
  uint32_t bytes;
};
static int field_table(const char* what, const inr_grid_desc* desc, const void* emb, bool half, FieldTable& t) {
  if (int rc = make_grid_desc(desc, t.G)) return rc;
  const uint64_t bytes = (uint64_t)desc->offsets[desc->num_levels] * (half ? 4ull : 8ull);
  if (bytes >= (1ull << 31)) {
    set_error("%s: table larger than 2 GiB is not addressable by the 32-bit gather offsets", what);
    return INR_EINVAL;
  }
  t.emb = reinterpret_cast<const float2*>(emb);
  t.bytes = (uint32_t)bytes;
  return INR_OK;
}
static const float4* f4(const float* p) { return reinterpret_cast<const float4*>(p); }

// Hybrid schedule (TileWalk) of one launch: frames and occupancy sweeps (four rounds of eight 1024-tile chunks and
// more) draw their tiles through a cursor set zeroed on the launch's stream; smaller launches, and every launch inside a
// stream capture (see steal_cursors), take the static deal (cursors() null).  finish() goes between the launch and its
// check_launch, so that a failed event record surfaces in that export's return code.
struct HybridSchedule {
  StealSet set;
  bool begin(hipStream_t s, int64_t n_tiles) {       // false: no cursor set (the error is set)
    if ((n_tiles >> (kXcdChunkLog2 + 3)) < 4 || stream_is_capturing(s)) return true;
    set = steal_cursors(s);
    return set.cursors != nullptr;
  }
  unsigned long long* cursors() const { return set.cursors; }
  void finish(hipStream_t s) { steal_release(set, s); }
};

// One field launch: the persistent grid of grid_for, kFieldThreads threads, `lds` bytes of dynamic LDS.
template <typename Kern, typename... Args>
static void launch_field(Kern kern, size_t lds, int64_t n_tiles, hipStream_t s, Args... args) {
  kern<<<grid_for(kern, lds, n_tiles), kFieldThreads, lds, s>>>(args...);
}

// Runtime choices as compile-time constants, so that each launch is written once: with_kmt calls f with
// std::integral_constant<int, K_MT> for the head's 16-row groups (1..3, 4 otherwise), with_flag with std::bool_constant.
// with_mlp_f16 is with_flag for INR_NUMERICS_MLP_F16, whose kernels the exact-fp32 build does not have (check_numerics
// refuses the bit there).
template <typename F>
static void with_kmt(int k_mt, F&& f) {
  switch (k_mt) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
template <typename F>
static void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}
template <typename F>
static void with_mlp_f16(bool on, F&& f) {
#if !INR_MLP_FP32
  if (on) return f(std::true_type{});
#endif
  f(std::false_type{});
}

// The `numerics` argument: a value whose bit is set in `accepted`.  Checked after an export's other arguments and its
// table, so that each of those keeps the message of its own check.
constexpr int kNumericsO = INR_NUMERICS_TABLE_F16 | INR_NUMERICS_MLP_F16;       // upstream's `-O`: both halves
constexpr unsigned kAcceptPlainOrO = 1u | 1u << kNumericsO;
constexpr unsigned kAcceptAny = 0xFu;
constexpr unsigned kAcceptPack = 1u | 1u << INR_NUMERICS_MLP_F16;
static int check_numerics(const char* what, int32_t numerics, unsigned accepted) {
  if (numerics < 0 || numerics > 3 || !((accepted >> numerics) & 1u)) {
    set_error("%s: numerics %d is not accepted here", what, numerics);
    return INR_EINVAL;
  }
#if INR_MLP_FP32
  if (numerics & INR_NUMERICS_MLP_F16) {
    set_error("%s: INR_NUMERICS_MLP_F16 is not available in the exact-fp32 build", what);
    return INR_EINVAL;
  }
#endif
  return INR_OK;
}

// host packer of one weight section: the build's fragment values, or fp16 ones (INR_NUMERICS_MLP_F16)
template <class KIdx>
static void pack_section_as(int32_t numerics, float* dst, const float* W, int n_out, int n_in, int n_mt, int n_ks,
                            KIdx kidx) {
  if (numerics & INR_NUMERICS_MLP_F16) pack_section_f16(dst, W, n_out, n_in, n_mt, n_ks, kidx);
  else pack_section(dst, W, n_out, n_in, n_mt, n_ks, kidx);
}

// The fused table launch behind inr_nerf_forward_table (kRec false: x = x01 [M,3], table = the SH rows) and
// inr_nerf_forward_table_records (kRec true: x = t [M], table = the ray rows): one LDS request, priority, tile schedule and
// cursor set for both - only where a tile's coordinates come from differs.
// k_nerf_fwd_pair serves the frame path's default variant only: records feed, 16-level fp32 table with every fine level
// (8..15) hashed, bf16x3 MLP.  INR_FIELD_PAIR=0 in the environment - read at every launch, so that one process can run
// both - selects k_nerf_fwd for those launches too (same bits; for A/B measurements and the tests).
static bool pair_front_end_qualifies(const inr_grid_desc* desc, int32_t numerics) {
#if INR_MLP_FP32
  return false;
#endif
  if (numerics != 0 || desc->num_levels != 16) return false;
  for (int l = 8; l < 16; ++l)
    if (!desc->hashed[l]) return false;
  const char* off = getenv("INR_FIELD_PAIR");
  return !(off && off[0] == '0' && off[1] == 0);
}

// k_nerf_fwd_pair<true> (dense x-pairs: one 16-byte load per x-neighbour row pair of levels 0..3) where those four levels
// are all dense; any other table takes k_nerf_fwd_pair<false>, the kernel of before.  INR_FIELD_COARSE=0 in the
// environment - read at every launch, like INR_FIELD_PAIR - selects the latter for every table (A/B runs and tests).
// inr_debug_field_coarse_launches[v] (include/inr.h) counts the pair launches that took <v>: how a test sees the gate.
extern "C" int64_t inr_debug_field_coarse_launches[2];
static bool dense_x_pairs_qualify(const inr_grid_desc* desc) {
  for (int l = 0; l < 4; ++l)
    if (desc->hashed[l]) return false;
  const char* off = getenv("INR_FIELD_COARSE");
  return !(off && off[0] == '0' && off[1] == 0);
}

template <bool kRec>
static int forward_table_launch(const char* what, const float* x, const int32_t* ray_ids, const float* table, int64_t M,
                                float bound, const void* embeddings, const inr_grid_desc* desc, const float* packed,
                                float density_scale, float* sigma, float* rgb, int32_t numerics, inr_stream_t s) {
  FieldTable t;
  if (int rc = field_table(what, desc, embeddings, numerics & INR_NUMERICS_TABLE_F16, t)) return rc;
  if (int rc = check_numerics(what, numerics, kAcceptAny)) return rc;
  const size_t lds = std::max(kNerfFloats * sizeof(float) + kLevelRecBytes, (size_t)g_field_lds_min);
  const int64_t n_tiles = (M + 15) / 16;
  const hipStream_t st = as_stream(s);
  HybridSchedule hybrid;         // frames (four rounds of eight 1024-tile chunks and more)
  if (!hybrid.begin(st, n_tiles)) return INR_ELAUNCH;
  if (kRec && pair_front_end_qualifies(desc, numerics)) {
    const bool dense = dense_x_pairs_qualify(desc);
    with_flag(dense, [&](auto dx) {
      launch_field(k_nerf_fwd_pair<decltype(dx)::value>, lds, (n_tiles + 1) / 2, st, x, M, bound, t.emb, t.bytes, t.G,
                   f4(packed), density_scale, sigma, rgb, ray_ids, f4(table), hybrid.cursors());
    });
    ++inr_debug_field_coarse_launches[dense ? 1 : 0];
    hybrid.finish(st);
    return check_launch(what + 4);
  }
  with_flag(numerics & INR_NUMERICS_TABLE_F16, [&](auto half) {
    with_mlp_f16(numerics & INR_NUMERICS_MLP_F16, [&](auto fast) {
      launch_field(k_nerf_fwd<true, true, 0, decltype(half)::value, decltype(fast)::value, false, kRec>, lds, n_tiles, st,
                   x, nullptr, M, nullptr, bound, t.emb, t.bytes, t.G, f4(packed), density_scale, sigma, rgb, nullptr,
                   ray_ids, f4(table), NerfSave{}, hybrid.cursors());
    });
  });
  hybrid.finish(st);
  return check_launch(what + 4);       // without "inr_"
}

// per-ray rows of the records feed: out[n] = kRayRowVec float4 - the SH rows of k_sh_table_q (out[n][q][ks] =
// sh[4*ks + q], the same sh4 on the same direction: the same bits), then (o, 0) and (d, 0)
__global__ void __launch_bounds__(256) k_ray_table_q(const float* __restrict__ o, const float* __restrict__ d, int64_t N,
                                                     float4* __restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float dx = d[n * 3], dy = d[n * 3 + 1], dz = d[n * 3 + 2];
  float v[16];
  sh4(dx, dy, dz, v);
  float4* row = out + n * kRayRowVec;
#pragma unroll
  for (int q = 0; q < 4; ++q) row[q] = make_float4(v[q], v[4 + q], v[8 + q], v[12 + q]);
  row[4] = make_float4(o[n * 3], o[n * 3 + 1], o[n * 3 + 2], 0.0f);
  row[5] = make_float4(dx, dy, dz, 0.0f);
}

}  // namespace inr

using namespace inr;

extern "C" {

int64_t inr_debug_field_coarse_launches[2] = {0, 0};

int64_t inr_nerf_packed_floats(void) { return kNerfFloats; }

int inr_nerf_pack_weights(const float* sigma_w0, const float* sigma_w1, const float* color_w0, const float* color_w1,
                          const float* color_w2, float* packed, int32_t numerics) {
  INR_REQUIRE(sigma_w0 && sigma_w1 && color_w0 && color_w1 && color_w2 && packed, "null pointer");
  if (int rc = check_numerics(__func__, numerics, kAcceptPack)) return rc;
  pack_section_as(numerics, packed + kSig0, sigma_w0, 64, 32, 4, 8, kidx_enc);
  pack_section_as(numerics, packed + kSig1, sigma_w1, 16, 64, 1, 16, kidx_hidden);
  pack_section_as(numerics, packed + kCol0, color_w0, 64, 31, 4, 8, kidx_color_in);
  pack_section_as(numerics, packed + kCol1, color_w1, 64, 64, 4, 16, kidx_hidden);
  pack_section_as(numerics, packed + kCol2, color_w2, 3, 64, 1, 16, kidx_hidden);
  return INR_OK;
}

int64_t inr_instance_packed_floats(int32_t K) {
  INR_REQUIRE(K > 0 && K <= 64 && K % 16 == 0, "K must be 16, 32, 48 or 64");
  return kIns2 + K * 64;
}

int inr_instance_pack_weights(const float* w0, const float* w1, const float* w2, int32_t K, float* packed,
                              int32_t numerics) {
  INR_REQUIRE(w0 && w1 && w2 && packed, "null pointer");
  INR_REQUIRE(K > 0 && K <= 64 && K % 16 == 0, "K must be 16, 32, 48 or 64");
  if (int rc = check_numerics(__func__, numerics, kAcceptPack)) return rc;
  pack_section_as(numerics, packed + kIns0, w0, 64, 32, 4, 8, kidx_enc);
  pack_section_as(numerics, packed + kIns1, w1, 64, 64, 4, 16, kidx_hidden);
  pack_section_as(numerics, packed + kIns2, w2, K, 64, K / 16, 16, kidx_hidden);
  return INR_OK;
}

int inr_nerf_forward(const float* x, const float* d, int64_t M, const int32_t* n_samples_dev, float bound,
                     const void* embeddings, const inr_grid_desc* desc, const float* packed, float density_scale,
                     float* sigma, float* rgb, float* geo_feat, int32_t numerics, inr_stream_t s) {
  const bool o = numerics == kNumericsO;
  INR_REQUIRE(M >= 0 && desc, "bad argument");
  if (M == 0) return INR_OK;
  INR_REQUIRE(x && embeddings && packed && sigma && (rgb || !o), "null pointer");
  INR_REQUIRE(!rgb || d, "rgb requested without view directions");
  INR_REQUIRE(!(o && geo_feat), "no geo_feat under the -O numerics");
  INR_REQUIRE(((uintptr_t)embeddings & (o ? 3 : 7)) == 0 && ((uintptr_t)packed & 15) == 0, "embeddings/packed misaligned");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, o, t)) return rc;
  if (int rc = check_numerics(__func__, numerics, kAcceptPlainOrO)) return rc;
  const int64_t n_tiles = (M + 15) / 16;
  const hipStream_t st = as_stream(s);
  // frames and occupancy sweeps take the hybrid schedule; the -O launch (the frozen NeRF of the instance stage) does not
  HybridSchedule hybrid;
  if (!o && !hybrid.begin(st, n_tiles)) return INR_ELAUNCH;
  const size_t lds = (rgb ? kNerfFloats : kCol0) * sizeof(float) + kLevelRecBytes;
  const auto launch = [&](auto kern) {
    launch_field(kern, lds, n_tiles, st, x, d, M, n_samples_dev, bound, t.emb, t.bytes, t.G, f4(packed), density_scale,
                 sigma, rgb, geo_feat, nullptr, nullptr, NerfSave{}, hybrid.cursors());
  };
  with_mlp_f16(o, [&](auto fast) {
    if constexpr (decltype(fast)::value) launch(k_nerf_fwd<true, false, 0, true, true>);
    else if (rgb) launch(k_nerf_fwd<true>);
    else launch(k_nerf_fwd<false>);
  });
  hybrid.finish(st);
  return check_launch("nerf_forward");
}

int inr_nerf_forward_table(const float* x01, const int32_t* ray_ids, const float* sh_table_q, int64_t M, float bound,
                           const void* embeddings, const inr_grid_desc* desc, const float* packed, float density_scale,
                           float* sigma, float* rgb, int32_t numerics, inr_stream_t s) {
  INR_REQUIRE(M >= 0 && desc, "bad argument");
  if (M == 0) return INR_OK;
  INR_REQUIRE(x01 && ray_ids && sh_table_q && embeddings && packed && sigma && rgb, "null pointer");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && ((uintptr_t)packed & 15) == 0 && ((uintptr_t)sh_table_q & 15) == 0,
              "embeddings/packed/sh_table_q misaligned");
  return forward_table_launch<false>(__func__, x01, ray_ids, sh_table_q, M, bound, embeddings, desc, packed,
                                     density_scale, sigma, rgb, numerics, s);
}

int inr_ray_table_q(const float* rays_o, const float* rays_d, int64_t N, float* out, inr_stream_t s) {
  INR_REQUIRE(N >= 0, "bad sizes");
  if (N == 0) return INR_OK;
  INR_REQUIRE(rays_o && rays_d && out, "null pointer");
  INR_REQUIRE(((uintptr_t)out & 15) == 0, "out misaligned");
  k_ray_table_q<<<blocks_for(N, 256), 256, 0, as_stream(s)>>>(rays_o, rays_d, N, reinterpret_cast<float4*>(out));
  return check_launch("ray_table_q");
}

int inr_nerf_forward_table_records(const float* t, const int32_t* ray_ids, const float* ray_table_q, int64_t M, float bound,
                             const void* embeddings, const inr_grid_desc* desc, const float* packed, float density_scale,
                             float* sigma, float* rgb, int32_t numerics, inr_stream_t s) {
  INR_REQUIRE(records_bound_ok(bound), "the records feed needs a power-of-two 2*bound (take the positions feed)");
  INR_REQUIRE(M >= 0 && desc, "bad argument");
  if (M == 0) return INR_OK;
  INR_REQUIRE(t && ray_ids && ray_table_q && embeddings && packed && sigma && rgb, "null pointer");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && ((uintptr_t)packed & 15) == 0 && ((uintptr_t)ray_table_q & 15) == 0,
              "embeddings/packed/ray_table_q misaligned");
  return forward_table_launch<true>(__func__, t, ray_ids, ray_table_q, M, bound, embeddings, desc, packed, density_scale,
                                    sigma, rgb, numerics, s);
}

// ---- sliced frame path: level-major pre-pass over the three finest levels + fused kernel on the other thirteen ------
int64_t inr_nerf_forward_table_sliced_workspace_bytes(int64_t M) {
  return M < 0 ? -1 : kSliceLevels * ((M + 31) & ~(int64_t)31) * (int64_t)sizeof(float2);
}

int inr_nerf_forward_table_sliced(const float* x01, const int32_t* ray_ids, const float* sh_table_q, int64_t M, float bound,
                                  const float* embeddings, const inr_grid_desc* desc, const float* packed,
                                  float density_scale, float* sigma, float* rgb, float* fine_ws, inr_stream_t s) {
  INR_REQUIRE(M >= 0 && desc, "bad argument");
  if (M == 0) return INR_OK;
  INR_REQUIRE(x01 && ray_ids && sh_table_q && embeddings && packed && sigma && rgb && fine_ws, "null pointer");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && ((uintptr_t)packed & 15) == 0 && ((uintptr_t)sh_table_q & 15) == 0 &&
              ((uintptr_t)fine_ws & 7) == 0, "embeddings/packed/sh_table_q/fine_ws misaligned");
  INR_REQUIRE(desc->num_levels == 16, "the sliced frame path needs the 16-level table");
  for (int l = 8; l < 16; ++l) INR_REQUIRE(desc->hashed[l], "the sliced frame path needs hashed fine levels (8..15)");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, false, t)) return rc;
  const size_t lds = std::max(kNerfFloats * sizeof(float) + kLevelRecBytes, (size_t)g_field_lds_min);
  hipStream_t st = as_stream(s);
  static int fit = 0;                      // resident pre-pass workgroups per CU (a constant of the build)
  if (fit < 1 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, k_grid_fine_slices, kSliceThreads, 0) != hipSuccess || fit < 1))
    fit = 4;
  // pre-pass: a full house of persistent workgroups per level; dispatch order (x fast, level slow) is the temporal order.
  // (Measured and not kept, profiles/r05_NOTES.txt 3: the frame in chunks with the pre-pass of chunk k+1 on a side stream
  //  beside the fused kernel of chunk k - the fused kernel's traffic then walks through the L2 the pre-pass lives on:
  //  27.3-27.9 ms against 27.5 ms one after the other, 4.2-4.4 against 4.07 ms with growing steps.)
  const int64_t per_wg = 32 * kSliceTilesPerIter * (kSliceThreads / 64);
  const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((M + per_wg - 1) / per_wg, (int64_t)cu_count() * fit));
  k_grid_fine_slices<<<dim3(gx, kSliceLevels), kSliceThreads, 0, st>>>(x01, M, t.emb, t.bytes, t.G, fine_ws);
  HybridSchedule hybrid;
  if (!hybrid.begin(st, (M + 15) / 16)) return INR_ELAUNCH;
  launch_field(k_nerf_fwd<true, true, 0, false, false, true>, lds, (M + 15) / 16, st, x01, fine_ws, M, nullptr, bound,
               t.emb, t.bytes, t.G, f4(packed), density_scale, sigma, rgb, nullptr, ray_ids, f4(sh_table_q), NerfSave{},
               hybrid.cursors());
  hybrid.finish(st);
  return check_launch("nerf_forward_table_sliced");
}

int inr_nerf_forward_dirs(const float* x, int64_t M, float bound, const float* embeddings, const inr_grid_desc* desc,
                          const float* packed, const float* sh_dirs, int32_t n_dirs, float* out, inr_stream_t s) {
  INR_REQUIRE(M >= 0 && desc, "bad argument");
  if (M == 0) return INR_OK;
  INR_REQUIRE(x && embeddings && packed && sh_dirs && out, "null pointer");
  INR_REQUIRE(n_dirs >= 1 && n_dirs <= kMaxExtractDirs, "1..8 view directions");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && ((uintptr_t)packed & 15) == 0 && ((uintptr_t)out & 15) == 0,
              "embeddings/packed/out misaligned");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, false, t)) return rc;
  const size_t lds = kNerfFloats * sizeof(float) + kLevelRecBytes + kMaxExtractDirs * 16 * sizeof(float);
  launch_field(k_nerf_fwd_dirs<false>, lds, (M + 15) / 16, as_stream(s), x, M, bound, t.emb, t.bytes, t.G, f4(packed),
               sh_dirs, n_dirs, reinterpret_cast<float4*>(out), LatticeDesc{}, -INFINITY);
  return check_launch("nerf_forward_dirs");
}

int inr_nerf_forward_lattice(const float* ax_w, const float* ax_l, const float* ax_h, int32_t W, int32_t L, int32_t H,
                             float bound, const float* embeddings, const inr_grid_desc* desc, const float* packed,
                             const float* sh_dirs, int32_t n_dirs, float logit_min, float* out, inr_stream_t s) {
  INR_REQUIRE(W >= 0 && L >= 0 && H >= 0 && desc, "bad argument");
  if ((int64_t)W * L * H == 0) return INR_OK;
  INR_REQUIRE(ax_w && ax_l && ax_h && embeddings && packed && sh_dirs && out, "null pointer");
  INR_REQUIRE(n_dirs >= 1 && n_dirs <= kMaxExtractDirs, "1..8 view directions");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && ((uintptr_t)packed & 15) == 0 && ((uintptr_t)out & 15) == 0,
              "embeddings/packed/out misaligned");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, false, t)) return rc;
  LatticeDesc lat{ax_w, ax_l, ax_h, W, L, H, (W + 15) / 16 * 16};
  const int64_t M = (int64_t)lat.Wp * L * H;           // traversal length: runs of 16 along w, padded per (il, ih)
  const size_t lds = kNerfFloats * sizeof(float) + kLevelRecBytes + kMaxExtractDirs * 16 * sizeof(float);
  launch_field(k_nerf_fwd_dirs<true>, lds, (M + 15) / 16, as_stream(s), nullptr, M, bound, t.emb, t.bytes, t.G,
               f4(packed), sh_dirs, n_dirs, reinterpret_cast<float4*>(out), lat, logit_min);
  return check_launch("nerf_forward_lattice");
}

int inr_instance_forward(const float* x, int64_t M, const int32_t* n_samples_dev, float bound, const float* embeddings,
                         const inr_grid_desc* desc, const float* packed, int32_t K, float* logits, inr_stream_t s) {
  INR_REQUIRE(M >= 0 && desc, "bad argument");
  if (M == 0) return INR_OK;
  INR_REQUIRE(x && embeddings && packed && logits, "null pointer");
  INR_REQUIRE(K > 0 && K <= 64 && K % 16 == 0, "K must be 16, 32, 48 or 64");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && ((uintptr_t)packed & 15) == 0 && ((uintptr_t)logits & 15) == 0,
              "embeddings/packed/logits misaligned");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, false, t)) return rc;
  const size_t lds = (size_t)(kIns2 + K * 64) * sizeof(float) + kLevelRecBytes;
  with_kmt(K / 16, [&](auto kmt) {
    launch_field(k_instance_fwd<decltype(kmt)::value>, lds, (M + 15) / 16, as_stream(s), x, M, n_samples_dev, bound,
                 t.emb, t.bytes, t.G, f4(packed), logits, nullptr, nullptr, nullptr);
  });
  return check_launch("instance_forward");
}

int64_t inr_instance_bwd_packed_floats(void) { return kBwdFloats; }

int inr_instance_pack_weights_device(const float* w0, const float* w1, const float* w2, int32_t K, float* packed_fwd,
                                     float* packed_bwd, inr_stream_t s) {
  INR_REQUIRE(w0 && w1 && w2 && packed_fwd && packed_bwd, "null pointer");
  INR_REQUIRE(K > 0 && K <= 64 && K % 16 == 0, "K must be 16, 32, 48 or 64");
  INR_REQUIRE(((uintptr_t)packed_fwd & 15) == 0 && ((uintptr_t)packed_bwd & 15) == 0, "packed buffers misaligned");
  PackJobs jobs;
  //           W   rows cols  n_out n_in  mt      steps T  offset
  jobs.j[0] = {w0, 64, 32, 64, 32, 4, 1, 0, kIns0, 0, 0, 0, 0};
  jobs.j[1] = {w1, 64, 64, 64, 64, 4, 2, 0, kIns1, 0, 0, 0, 0};
  jobs.j[2] = {w2, K, 64, K, 64, K / 16, 2, 0, kIns2, 0, 0, 0, 0};
  jobs.j[3] = {w2, K, 64, 64, K, 4, 2, 1, kBwd2, 0, 0, 0, 1};
  jobs.j[4] = {w1, 64, 64, 64, 64, 4, 2, 1, kBwd1, 0, 0, 0, 1};
  jobs.j[5] = {w0, 64, 32, 32, 64, 2, 2, 1, kBwd0, 0, 0, 0, 1};
  k_pack_weights<<<dim3(8, 6), 256, 0, as_stream(s)>>>(jobs, packed_fwd, packed_bwd);
  return check_launch("instance_pack_weights_device");
}

int inr_instance_forward_train(const float* x, int64_t M, float bound, const float* embeddings, const inr_grid_desc* desc,
                               const float* packed, int32_t K, float* logits, float* enc, float* h1, float* h2,
                               inr_stream_t s) {
  INR_REQUIRE(M >= 0 && desc, "bad argument");
  if (M == 0) return INR_OK;
  INR_REQUIRE(x && embeddings && packed && logits && enc && h1 && h2, "null pointer");
  INR_REQUIRE(K > 0 && K <= 64 && K % 16 == 0, "K must be 16, 32, 48 or 64");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 &&
                  (((uintptr_t)packed | (uintptr_t)logits | (uintptr_t)enc | (uintptr_t)h1 | (uintptr_t)h2) & 15) == 0,
              "embeddings/packed/outputs misaligned");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, false, t)) return rc;
  const size_t lds = (size_t)(kIns2 + K * 64) * sizeof(float) + kLevelRecBytes;
  with_kmt(K / 16, [&](auto kmt) {
    launch_field(k_instance_fwd<decltype(kmt)::value, 1>, lds, (M + 15) / 16, as_stream(s), x, M, nullptr, bound, t.emb,
                 t.bytes, t.G, f4(packed), logits, enc, h1, h2);
  });
  return check_launch("instance_forward_train");
}

int inr_instance_forward_enc(const float* x, int64_t M, const int32_t* n_samples_dev, float bound, const float* embeddings,
                             const inr_grid_desc* desc, const float* packed, int32_t K, float* logits, float* enc,
                             inr_stream_t s) {
  INR_REQUIRE(M >= 0 && desc, "bad argument");
  if (M == 0) return INR_OK;
  INR_REQUIRE(x && embeddings && packed && logits && enc, "null pointer");
  INR_REQUIRE(K > 0 && K <= 64 && K % 16 == 0, "K must be 16, 32, 48 or 64");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && (((uintptr_t)packed | (uintptr_t)logits | (uintptr_t)enc) & 15) == 0,
              "embeddings/packed/outputs misaligned");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, false, t)) return rc;
  const size_t lds = (size_t)(kIns2 + K * 64) * sizeof(float) + kLevelRecBytes;
  with_kmt(K / 16, [&](auto kmt) {
    launch_field(k_instance_fwd<decltype(kmt)::value, 2>, lds, (M + 15) / 16, as_stream(s), x, M, n_samples_dev, bound,
                 t.emb, t.bytes, t.G, f4(packed), logits, enc, nullptr, nullptr);
  });
  return check_launch("instance_forward_enc");
}

int inr_instance_lattice(const float* ax_w, const float* ax_l, const float* ax_h, int32_t W, int32_t L, int32_t H,
                         float bound, const float* nerf_embeddings, const inr_grid_desc* nerf_desc, const float* nerf_packed,
                         float density_scale, float sigma_thresh, const float* inst_embeddings,
                         const inr_grid_desc* inst_desc, const float* inst_packed, int32_t K, uint8_t* labels,
                         float* confidence, float* density_logit, inr_stream_t s) {
  INR_REQUIRE(W >= 0 && L >= 0 && H >= 0, "W, L, H must be >= 0");
  INR_REQUIRE(K >= 1 && K <= 64, "K must be 1..64 (packed with K_pad = 16 * ceil(K / 16) output rows)");
  INR_REQUIRE(nerf_desc && inst_desc, "null grid descriptor");
  INR_REQUIRE(ax_w && ax_l && ax_h && nerf_embeddings && nerf_packed && inst_embeddings && inst_packed && labels &&
                  confidence, "null pointer");
  INR_REQUIRE(!std::isnan(bound) && bound > 0.0f, "bound must be > 0");
  INR_REQUIRE(!std::isnan(sigma_thresh) && !std::isnan(density_scale), "sigma_thresh / density_scale must not be NaN");
  INR_REQUIRE((((uintptr_t)nerf_embeddings | (uintptr_t)inst_embeddings) & 7) == 0 &&
                  (((uintptr_t)nerf_packed | (uintptr_t)inst_packed) & 15) == 0 &&
                  (((uintptr_t)confidence | (uintptr_t)density_logit) & 3) == 0,
              "embeddings/packed/confidence/density_logit misaligned");
  INR_REQUIRE((int64_t)W * L * H < (1ll << 31), "lattice of 2^31 voxels or more");
  GridDesc Gn, Gi;
  int rc = make_grid_desc(nerf_desc, Gn);
  if (rc) return rc;
  rc = make_grid_desc(inst_desc, Gi);
  if (rc) return rc;
  const uint64_t bn = (uint64_t)nerf_desc->offsets[nerf_desc->num_levels] * 8ull;
  const uint64_t bi = (uint64_t)inst_desc->offsets[inst_desc->num_levels] * 8ull;
  INR_REQUIRE(bn < (1ull << 31) && bi < (1ull << 31), "table larger than 2 GiB is not addressable by the 32-bit gather offsets");
  if ((int64_t)W * L * H == 0) return INR_OK;
  LatticeDesc lat{ax_w, ax_l, ax_h, W, L, H, (W + 15) / 16 * 16};
  const int K_MT = (K + 15) / 16;
  const size_t lds = (size_t)(kCol0 + kIns2 + K_MT * 16 * 64) * sizeof(float) + 2 * kLevelRecBytes;
  const int64_t n_tiles = (int64_t)lat.Wp * L * H / 16;
  const float2* en = reinterpret_cast<const float2*>(nerf_embeddings);
  const float2* ei = reinterpret_cast<const float2*>(inst_embeddings);
  with_kmt(K_MT, [&](auto kmt) {
    launch_field(k_instance_lattice<decltype(kmt)::value>, lds, n_tiles, as_stream(s), lat, bound, en, (uint32_t)bn, Gn,
                 f4(nerf_packed), density_scale, sigma_thresh, ei, (uint32_t)bi, Gi, f4(inst_packed), K, labels,
                 confidence, density_logit);
  });
  return check_launch("instance_lattice");
}

int inr_instance_volume_stats(const uint8_t* labels, const float* confidence, int32_t W, int32_t L, int32_t H, int32_t K,
                              void* workspace, int64_t workspace_bytes, int32_t* counts, int32_t* boxes, float* conf_sum,
                              inr_stream_t s) {
  INR_REQUIRE(W >= 0 && L >= 0 && H >= 0, "W, L, H must be >= 0");
  INR_REQUIRE(K >= 1 && K <= 64, "K must be 1..64");
  INR_REQUIRE(workspace_bytes >= kStatsWorkspaceBytes, "workspace smaller than INR_INSTANCE_STATS_WORKSPACE_BYTES");
  INR_REQUIRE(labels && confidence && workspace && counts && boxes && conf_sum, "null pointer");
  INR_REQUIRE((((uintptr_t)confidence | (uintptr_t)workspace | (uintptr_t)counts | (uintptr_t)boxes | (uintptr_t)conf_sum) & 3) == 0,
              "confidence/workspace/outputs misaligned");
  const int64_t N = (int64_t)W * L * H;
  INR_REQUIRE(N < (1ll << 31), "volume of 2^31 voxels or more");
  // at least 16 chunks of 64 voxels per workgroup, at most kStatsMaxBlocks workgroups
  const int64_t per_min = 16 * 64;
  const int n_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(kStatsMaxBlocks, (N + per_min - 1) / per_min));
  const int64_t per_block = (N + n_blocks - 1) / n_blocks;
  hipStream_t st = as_stream(s);
  int* part = reinterpret_cast<int*>(workspace);
  k_instance_stats_partial<<<n_blocks, kStatsThreads, 0, st>>>(labels, confidence, (uint32_t)N, (uint32_t)L, (uint32_t)H, K,
                                                               (uint32_t)per_block, part);
  k_instance_stats_final<<<1, 64 * kStatsFinalGroups, 0, st>>>(part, n_blocks, K, counts, boxes, conf_sum);
  return check_launch("instance_volume_stats");
}

static size_t head_bwd_lds() { return (size_t)(kHbFwdFloats + kBwdFloats + kHbStageFloats) * sizeof(float); }

int64_t inr_instance_head_workspace_bytes(void) {
  return (int64_t)cu_count() * kFieldBlocksPerCU * kHbAccTiles * 64 * (int64_t)sizeof(float4);
}

int inr_instance_head_backward(const float* enc, const float* weights, const int32_t* sample_ray, const float* grad_pix,
                               int32_t K, int64_t N, int64_t M, const int32_t* n_samples_dev, const float* scale_a,
                               const float* scale_b, const float* packed_fwd, const float* packed_bwd, float* grad_enc,
                               void* workspace, float* grad_w0, float* grad_w1, float* grad_w2, float* zero_buf,
                               int64_t zero_floats, inr_stream_t s) {
  INR_REQUIRE(zero_floats >= 0 && (!zero_buf || ((uintptr_t)zero_buf & 15) == 0), "zero_buf must be 16-byte aligned");
  INR_REQUIRE(M >= 0 && N >= 0, "negative size");
  INR_REQUIRE(K > 0 && K <= 64 && K % 16 == 0, "K must be 16, 32, 48 or 64");
  INR_REQUIRE(grad_w0 && grad_w1 && grad_w2 && workspace && packed_fwd && packed_bwd, "null pointer");
  INR_REQUIRE(M == 0 || (enc && weights && sample_ray && grad_pix && grad_enc), "null sample arrays");
  INR_REQUIRE((((uintptr_t)enc | (uintptr_t)grad_pix | (uintptr_t)packed_fwd | (uintptr_t)packed_bwd | (uintptr_t)grad_enc |
                (uintptr_t)workspace) & 15) == 0, "arrays must be 16-byte aligned");
  hipStream_t st = as_stream(s);
  const size_t lds = head_bwd_lds();
  static AttrOnce attr;     // > 64 KB of dynamic LDS must be allowed explicitly, on every device
  if (!attr.ensure(k_instance_head_bwd, lds)) {
    set_error("instance_head_backward: %zu bytes of LDS refused", lds);
    return INR_ELAUNCH;
  }
  const int64_t n_tiles = (M + 15) / 16;
  const int grid = M == 0 ? 1 : grid_for(k_instance_head_bwd, lds, n_tiles);
  k_instance_head_bwd<<<grid, kFieldThreads, lds, st>>>(enc, weights, sample_ray, grad_pix, K, M, n_samples_dev,
                                                        scale_a, scale_b, reinterpret_cast<const float4*>(packed_fwd),
                                                        reinterpret_cast<const float4*>(packed_bwd), grad_enc,
                                                        reinterpret_cast<float4*>(workspace), zero_buf, zero_floats);
  k_head_wgrad_reduce<<<kHbAccTiles * 256 / 64, 1024, 0, st>>>(reinterpret_cast<const float*>(workspace), grid, K, grad_w0,
                                                               grad_w1, grad_w2);
  return check_launch("instance_head_backward");
}

int inr_instance_backward(const float* grad_logits, int32_t K, const float* h1, const float* h2, int64_t M,
                          const float* packed_bwd, float* grad_z2, float* grad_z1, float* grad_enc, inr_stream_t s) {
  INR_REQUIRE(M >= 0, "negative M");
  if (M == 0) return INR_OK;
  INR_REQUIRE(grad_logits && h1 && h2 && packed_bwd && grad_z2 && grad_z1 && grad_enc, "null pointer");
  INR_REQUIRE(K > 0 && K <= 64 && K % 16 == 0, "K must be 16, 32, 48 or 64");
  INR_REQUIRE((((uintptr_t)grad_logits | (uintptr_t)h1 | (uintptr_t)h2 | (uintptr_t)packed_bwd | (uintptr_t)grad_z2 |
                (uintptr_t)grad_z1 | (uintptr_t)grad_enc) & 15) == 0, "arrays must be 16-byte aligned");
  const size_t lds = (size_t)kBwdFloats * sizeof(float);
  const int64_t n_tiles = (M + 15) / 16;
  k_instance_bwd<<<grid_for(k_instance_bwd, lds, n_tiles), kFieldThreads, lds, as_stream(s)>>>(
      grad_logits, K, h1, h2, M, reinterpret_cast<const float4*>(packed_bwd), grad_z2, grad_z1, grad_enc);
  return check_launch("instance_backward");
}

int64_t inr_nerf_bwd_packed_floats(void) { return kNerfBwdFloats; }

int inr_nerf_pack_weights_device(const float* sigma_w0, const float* sigma_w1, const float* color_w0,
                                 const float* color_w1, const float* color_w2, float* packed_fwd, float* packed_bwd,
                                 inr_stream_t s) {
  INR_REQUIRE(sigma_w0 && sigma_w1 && color_w0 && color_w1 && color_w2 && packed_fwd && packed_bwd, "null pointer");
  INR_REQUIRE(((uintptr_t)packed_fwd & 15) == 0 && ((uintptr_t)packed_bwd & 15) == 0, "packed buffers misaligned");
  PackJobs jobs;
  //           W         rows cols n_out n_in mt steps T  offset kmode row_min shift bwd
  jobs.j[0] = {sigma_w0, 64, 32, 64, 32, 4, 1, 0, kSig0, 0, 0, 0, 0};
  jobs.j[1] = {sigma_w1, 16, 64, 16, 64, 1, 2, 0, kSig1, 0, 0, 0, 0};
  jobs.j[2] = {color_w0, 64, 31, 64, 31, 4, 1, 0, kCol0, 1, 0, 0, 0};
  jobs.j[3] = {color_w1, 64, 64, 64, 64, 4, 2, 0, kCol1, 0, 0, 0, 0};
  jobs.j[4] = {color_w2, 3, 64, 3, 64, 1, 2, 0, kCol2, 0, 0, 0, 0};
  jobs.j[5] = {color_w2, 3, 64, 64, 3, 4, 1, 1, kNbC2, 0, 0, 0, 1};
  jobs.j[6] = {color_w1, 64, 64, 64, 64, 4, 2, 1, kNbC1, 0, 0, 0, 1};
  jobs.j[7] = {color_w0, 64, 31, 16, 64, 1, 2, 1, kNbC0, 0, 1, 15, 1};      // row i >= 1 <- input column 15 + i
  jobs.j[8] = {sigma_w1, 16, 64, 64, 16, 4, 1, 1, kNbS1, 0, 0, 0, 1};
  jobs.j[9] = {sigma_w0, 64, 32, 32, 64, 2, 2, 1, kNbS0, 0, 0, 0, 1};
  k_pack_weights<<<dim3(8, 10), 256, 0, as_stream(s)>>>(jobs, packed_fwd, packed_bwd);
  return check_launch("nerf_pack_weights_device");
}

int inr_nerf_forward_train(const float* x, const float* d, int64_t M, float bound, const float* embeddings,
                           const inr_grid_desc* desc, const float* packed, float* sigma, float* rgb, float* enc,
                           float* h1, float* so, float* cin, float* c1, float* c2, inr_stream_t s) {
  INR_REQUIRE(M >= 0 && desc, "bad argument");
  if (M == 0) return INR_OK;
  INR_REQUIRE(x && d && embeddings && packed && sigma && rgb && enc && h1 && so && cin && c1 && c2, "null pointer");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 &&
                  (((uintptr_t)packed | (uintptr_t)enc | (uintptr_t)h1 | (uintptr_t)so | (uintptr_t)cin | (uintptr_t)c1 |
                    (uintptr_t)c2) & 15) == 0, "embeddings/packed/activation arrays misaligned");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, false, t)) return rc;
  const size_t lds = kNerfFloats * sizeof(float) + kLevelRecBytes;
  launch_field(k_nerf_fwd<true, false, 1>, lds, (M + 15) / 16, as_stream(s), x, d, M, nullptr, bound, t.emb, t.bytes,
               t.G, f4(packed), 1.0f, sigma, rgb, nullptr, nullptr, nullptr, NerfSave{enc, h1, so, cin, c1, c2}, nullptr);
  return check_launch("nerf_forward_train");
}

int inr_nerf_forward_enc(const float* x, const float* d, int64_t M, float bound, const float* embeddings,
                         const inr_grid_desc* desc, const float* packed, float* sigma, float* rgb, float* enc, inr_stream_t s) {
  INR_REQUIRE(M >= 0 && desc, "bad argument");
  if (M == 0) return INR_OK;
  INR_REQUIRE(x && d && embeddings && packed && sigma && rgb && enc, "null pointer");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && (((uintptr_t)packed | (uintptr_t)enc) & 15) == 0,
              "embeddings/packed/enc misaligned");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, false, t)) return rc;
  const size_t lds = kNerfFloats * sizeof(float) + kLevelRecBytes;
  NerfSave sv{};
  sv.enc = enc;
  launch_field(k_nerf_fwd<true, false, 2>, lds, (M + 15) / 16, as_stream(s), x, d, M, nullptr, bound, t.emb, t.bytes,
               t.G, f4(packed), 1.0f, sigma, rgb, nullptr, nullptr, nullptr, sv, nullptr);
  return check_launch("nerf_forward_enc");
}

int inr_nerf_head_backward(const float* enc, const float* d, const float* grad_sigma, const float* grad_rgb, int64_t M,
                           float density_scale, const float* packed_fwd, const float* packed_bwd, float* grad_enc,
                           void* workspace, float* grad_ws0, float* grad_ws1, float* grad_wc0, float* grad_wc1,
                           float* grad_wc2, float* zero_buf, int64_t zero_floats, inr_stream_t s) {
  INR_REQUIRE(M >= 0, "negative M");
  INR_REQUIRE(zero_floats >= 0 && (!zero_buf || ((uintptr_t)zero_buf & 15) == 0), "zero_buf must be 16-byte aligned");
  INR_REQUIRE(packed_fwd && packed_bwd && workspace && grad_ws0 && grad_ws1 && grad_wc0 && grad_wc1 && grad_wc2, "null pointer");
  INR_REQUIRE(M == 0 || (enc && d && grad_sigma && grad_rgb && grad_enc), "null sample arrays");
  INR_REQUIRE((((uintptr_t)enc | (uintptr_t)packed_fwd | (uintptr_t)packed_bwd | (uintptr_t)grad_enc | (uintptr_t)workspace) & 15) == 0,
              "arrays must be 16-byte aligned");
  hipStream_t st = as_stream(s);
  const size_t lds = (size_t)(kNhFwdFloats + kNerfBwdFloats + kHbStageFloats) * sizeof(float);
  static AttrOnce attr;
  if (!attr.ensure(k_nerf_head_bwd, lds)) {
    set_error("nerf_head_backward: %zu bytes of LDS refused", lds);
    return INR_ELAUNCH;
  }
  const int grid = M == 0 ? 1 : grid_for(k_nerf_head_bwd, lds, (M + 15) / 16);
  k_nerf_head_bwd<<<grid, kFieldThreads, lds, st>>>(enc, d, grad_sigma, grad_rgb, M, density_scale,
                                                    reinterpret_cast<const float4*>(packed_fwd),
                                                    reinterpret_cast<const float4*>(packed_bwd), grad_enc,
                                                    reinterpret_cast<float4*>(workspace), zero_buf, zero_floats);
  k_nerf_head_wgrad_reduce<<<kHbAccTiles * 256 / 64, 1024, 0, st>>>(reinterpret_cast<const float*>(workspace), grid, grad_wc2,
                                                                    grad_wc1, grad_wc0, grad_ws1, grad_ws0);
  return check_launch("nerf_head_backward");
}

int inr_nerf_backward(const float* grad_sigma, const float* grad_rgb, const float* rgb, const float* so, const float* h1,
                      const float* c1, const float* c2, int64_t M, float density_scale, const float* packed_bwd,
                      float* grad_o, float* grad_zc2, float* grad_zc1, float* grad_so, float* grad_zh1, float* grad_enc,
                      inr_stream_t s) {
  INR_REQUIRE(M >= 0, "negative M");
  if (M == 0) return INR_OK;
  INR_REQUIRE(grad_sigma && grad_rgb && rgb && so && h1 && c1 && c2 && packed_bwd && grad_o && grad_zc2 && grad_zc1 &&
                  grad_so && grad_zh1 && grad_enc, "null pointer");
  INR_REQUIRE((((uintptr_t)so | (uintptr_t)h1 | (uintptr_t)c1 | (uintptr_t)c2 | (uintptr_t)packed_bwd | (uintptr_t)grad_o |
                (uintptr_t)grad_zc2 | (uintptr_t)grad_zc1 | (uintptr_t)grad_so | (uintptr_t)grad_zh1 |
                (uintptr_t)grad_enc) & 15) == 0, "arrays must be 16-byte aligned");
  const size_t lds = (size_t)kNerfBwdFloats * sizeof(float);
  NerfBwdIO io{grad_sigma, grad_rgb, rgb, so, h1, c1, c2, grad_o, grad_zc2, grad_zc1, grad_so, grad_zh1, grad_enc};
  k_nerf_bwd<<<grid_for(k_nerf_bwd, lds, (M + 15) / 16), kFieldThreads, lds, as_stream(s)>>>(
      io, M, density_scale, reinterpret_cast<const float4*>(packed_bwd));
  return check_launch("nerf_backward");
}

int inr_instance_render(const float* xyzs, const int32_t* rays, const float* weights, int64_t N, int64_t M, float bound,
                        const void* embeddings, const inr_grid_desc* desc, const float* packed, int32_t K,
                        float* extra_out, int32_t x_is_01, uint64_t* cursors, int32_t numerics, inr_stream_t s) {
  const bool o = numerics == kNumericsO;
  INR_REQUIRE(N >= 0 && M >= 0 && desc, "bad argument");
  if (N == 0) return INR_OK;
  INR_REQUIRE(rays && embeddings && packed && extra_out && cursors && ((uintptr_t)cursors & 7) == 0, "null pointer");
  INR_REQUIRE(M == 0 || (xyzs && weights), "null sample arrays");
  INR_REQUIRE(K > 0 && K <= 64 && K % 16 == 0, "K must be 16, 32, 48 or 64");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && ((uintptr_t)packed & 15) == 0 && ((uintptr_t)extra_out & 15) == 0,
              "embeddings/packed/extra_out misaligned");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, o, t)) return rc;
  if (int rc = check_numerics(__func__, numerics, kAcceptPlainOrO)) return rc;
  // weights + level records + two buffers of eight partial [16 rays x K] sums
  const size_t lds = (size_t)(kIns2 + K * 64) * sizeof(float) + kLevelRecBytes + 2 * (kFieldThreads / 64) * (size_t)K * 64;
  const int64_t n_groups = (N + 15) / 16;
  const int64_t as_tiles = n_groups * (kFieldThreads / 64);        // one workgroup per group
  INR_REQUIRE(n_groups < ((int64_t)1 << 31) - 65536, "too many rays for the 32-bit group cursor");
  with_kmt(K / 16, [&](auto kmt) {
    with_mlp_f16(o, [&](auto fast) {
      launch_field(k_instance_render<decltype(kmt)::value, decltype(fast)::value>, lds, as_tiles, as_stream(s), xyzs, rays,
                   weights, N, M, bound, t.emb, t.bytes, t.G, f4(packed), extra_out, x_is_01,
                   reinterpret_cast<unsigned long long*>(cursors));
    });
  });
  return check_launch("instance_render");
}

int inr_nerf_render(const float* xyzs, const float* deltas, const int32_t* rays, const float* rays_d, int64_t N,
                    int64_t M, float bound, const void* embeddings, const inr_grid_desc* desc, const float* packed,
                    float density_scale, float T_thresh, float* weights_sum, float* depth, float* image, float* weights,
                    uint64_t* evaluated, int32_t x_is_01, int32_t numerics, inr_stream_t s) {
  const bool o = numerics == kNumericsO;
  INR_REQUIRE(N >= 0 && M >= 0 && desc, "bad argument");
  if (N == 0) return INR_OK;
  INR_REQUIRE(rays && rays_d && embeddings && packed && weights_sum && depth && image && evaluated, "null pointer");
  INR_REQUIRE(M == 0 || (xyzs && deltas), "null sample arrays");
  INR_REQUIRE(((uintptr_t)embeddings & 7) == 0 && ((uintptr_t)packed & 15) == 0 && ((uintptr_t)deltas & 7) == 0 &&
                  ((uintptr_t)evaluated & 7) == 0, "embeddings/packed/deltas/evaluated misaligned");
  FieldTable t;
  if (int rc = field_table(__func__, desc, embeddings, o, t)) return rc;
  if (int rc = check_numerics(__func__, numerics, kAcceptPlainOrO)) return rc;
  const size_t lds = kNerfFloats * sizeof(float) + kLevelRecBytes;
  const int64_t n_groups = (N + 15) / 16;
  INR_REQUIRE(n_groups < ((int64_t)1 << 31) - 65536, "too many rays for the 32-bit group cursor");
  with_mlp_f16(o, [&](auto fast) {
    launch_field(k_nerf_render<decltype(fast)::value>, lds, n_groups, as_stream(s), xyzs, deltas, rays, rays_d, N, M, bound,
                 t.emb, t.bytes, t.G, f4(packed), density_scale, T_thresh, weights_sum, depth, image, weights,
                 reinterpret_cast<unsigned long long*>(evaluated), x_is_01);
  });
  return check_launch("nerf_render");
}

}  // extern "C"
