"""Plain float64 restatement of the fused field's FORWARD kernels (csrc/field_fused.hip: k_nerf_fwd in all its
instantiations, k_nerf_fwd_pair, k_grid_fine_slices + the sliced feed, k_nerf_fwd_dirs plain and lattice, k_instance_fwd),
the generators of their test cases and the tolerances of tests/test_field_forward_kernels.py.  numpy only; the
arithmetic models Exact64 / SplitBf16 / SeqFp32 are those of field_backward_reference (imported, not copied), the records
feed's positions those of sample_records_ref; nothing shared with instance_nerf_amd or oracle/.

One restatement: position -> x01 -> 16-level trilinear gather -> sigma net (64 <- 32, 16 <- 64) -> sigma =
exp(so0) * density_scale, geo = so[1:] -> SH-4 of the direction or the ray's SH-table row -> colour net on [16 SH, 15 geo]
(64 <- 31, 64 <- 64, 3 <- 64) -> sigmoid; the instance net (64 <- 32, 64 <- 64, K <- 64) and the dirs variant (raw density
logit floored at logit_min, mean colour over n_dirs SH rows) run on the same encoder.

Specification (fp32, operation by operation; the library is built with -ffp-contract=off so that these decisions are the
oracle's): plain feed x01 = (x + bound) / (2 bound); lattice feed clamp(axis value, -bound, bound) first; records feed
p = clamp(o + t*d) as two operations and x01 = (p + bound) * (1 / (2 bound)) (sample_records_ref); then p = x01 * scale
+ 0.5 as a multiply and an add, floor, p - floor.  x01 outside [0, 1] on any axis (NaN included): all 32 features zero.
Row of a corner: dense cx + cy*s + cz*s^2, hashed (cx ^ cy*2654435761 ^ cz*805459861) & (rows - 1), in uint32 with
wrap-around (``row_index``; tests/test_field_forward_cpu.py cross-checks it against oracle.hashgrid).  From the fractions
on - corner weights (wx*wy)*wz, blend, MLP, SH, exp, sigmoid - the reference is float64.
A table with fewer than 16 levels leaves features 2L .. 31 to "dead" slots: the kernel lets them read row 0 and relies on
all-zero weight columns there.  The packers know no level count, so those zero columns are the CALLER's (every case
here zeroes them, the reference's dead features are 0), and test_dead_levels_read_row_0_against_zero_columns pins that
every packer carries the zeros into the right fragment slots: row 0 = +-1e4 changes no output bit.  (The enc array that
forward_train / _enc save holds row 0's blend in the dead columns; those columns are not specified and not compared.)

Models (|model - float64| is what MEASURED holds):
  bf16x3 / fp32     SplitBf16 / SeqFp32 layers; blend weights and fma chain rounded to fp32 step by step in the kernel's
                    order (levels 0..7 corners 0..7; levels 8..15 each x side's four corners, then side 0 + side 1).
  fp16 table (t16)  table values rounded to nearest-even fp16, everything else unchanged.
  fp16 MLP (m16)    HalfMlp: weights and layer inputs rounded to nearest-even fp16, products exact, one fp32 rounding per
                    layer.  "o" is both.
Every output comes with ``cond``, the same contraction over absolute values pushed through the 1-Lipschitz ReLUs:
features sum |w||v|; layers |x| @ |W|^T of the propagated bound; sigma: sigma * cond(so0) + sigma; rgb: c(1-c) cond(o) + c;
SH of a direction: the polynomial over |x|, |y|, |z| with every coefficient positive; an SH-table row is an input
(cond |row|, its fp16 rounding under m16 is real).  ReLU is continuous: no sample is left out of any comparison.  An
element with cond == 0 must be exactly 0.

Tolerance tier.  TOL[build][output@numerics] = margin x MEASURED; MEASURED is the largest |model - float64| / cond over
all tolerance-tier cases, measured on the CPU, two digits rounded up beside the value seen; the CPU suite asserts that
the models stay within TOL / margin.  Margin 8 for the default and fp32 numerics (MFMA-internal accumulation order,
v_exp_f32 / v_rcp_f32), margin 2 for t16 / m16 / o (the model's error is operand rounding that the device reproduces;
only activations on the other side of an fp16 tie differ).
Inputs: the level tables of field_issue_cases.TABLES (TABLE_SPECS; the CPU suite asserts they are equal), table values
U(-1,1), weights U(+-0.35) (32 inputs) / U(+-0.25) (64 inputs), the density row centred and scaled by SO0_SCALE (so0
passes +-15 on both sides at the 983-sample size), density_scale 1 and 0.3, bound 1 and 2 (plain feed also 1.5, where the
records feed returns its error code).  Positions: samples of rays (o + t d clamped: faces), the first rows volume faces,
centre and cell boundaries of the coarsest and finest level (rays with t = 0); the plain feeds get one row outside and
one NaN row.  All three feeds of a case see the same x01 (2 bound a power of two), so one float64 encoder run per
(table, size) serves every entry point.

Exact tier.  Bit equality with the float64 result rounded to fp32, both builds, every numerics mode: level tables with
per_level_scale 2 (scales base * 2^l - 1, 2^10 rows per hashed level: levels 0..2 dense, the rest hashed; "x16" xor-only
fine instantiation and pair front end, "x12" generic with dead fine slots), x01 on multiples of 1/8 (1/4 for the fp16 MLP),
table values integers in -2 .. 2 (both features of a row equal on levels 0..7), the sparse {-1,0,1} weights of the
backward suite's exact tier (so0 == 0 ON THE DATA, colour logits exactly 0), power-of-two density_scale, integer
SH-table rows.  ``exactness_violations``: bits per factor, bits per sum, fp16 width and range for the fp16 modes.  Exact
outputs: enc, h1, so, cin[16:], c1, c2 of forward_train / _enc; geo; all K logits; the raw density logit of dirs / lattice
and its floor (weights "logit": a live density row); sigma == density_scale; rgb == 0.5.

Rounding tier (fp16 MLP only).  Exact-tier tables and positions on multiples of 1/32 (features with up to 16 significant bits:
every layer input NEEDS its fp16 rounding), weights "live" (variant a with a +-1 density row and +-1 colour rows).
After the rounding every product is exact and every sum exact in fp32 in any order, so the kernel's so0 and colour
logits must be the HalfMlp model's bit for bit and sigma, rgb differ from the model only by the device's v_exp_f32 /
v_rcp_f32: |got - model| <= ROUNDING_TOL * model, ROUNDING_TOL = 8 * 2^-24 (exp2 within 1 ulp against the model's 0.5,
one more rounding each for 1 + e and the reciprocal, which is within 1 ulp: under 4 ulp = 8 * 2^-24 relative).  A
conversion that truncates moves an input by one fp16 quantum, 2^-11 relative: a thousand times the bound (the CPU suite
asserts that the truncating model misses it on more than a fifth of the rows).

Sizes: 0; 1, 15, 16, 17, 31, 32, 33 (pair boundary), 16*61+7; once each for the plain rgb, table and records feed
16*32768+7, the smallest launch on the hybrid schedule (HYBRID_MIN_TILES).

Seen on an MI355X, worst |got - ref| / cond as a fraction of TOL, per output.  Default build, margin 8: 0.117 .. 0.124
for every output (worst: enc 2.67e-7 of 2.16e-6 on all_dense at 983 samples, h1 1.54e-5 of 1.28e-4, c1 1.03e-5 of 8.8e-5,
sigma 1.72e-6 of 1.44e-5 at bound 1.5, rgb 2.22e-7 of 1.84e-6 on bench, logits 3.92e-7 of 3.2e-6), i.e. the GPU sits on
the split model (1/8 = 0.125), the hybrid-schedule launches included.  Margin 2: sigma@t16 0.476, rgb@t16 0.497,
sigma@m16 0.488, rgb@m16 0.491, sigma@o 0.495, rgb@o 0.496: the device reproduces the operand roundings (1/2 = 0.5), so
margin 2 holds with room to spare.  fp32 library: 0.08 .. 0.14, cin 0.39 (the SH columns: sh4's own fp32 steps against one
rounding of the float64 polynomial), sigma@t16 0.48, rgb@t16 0.50.  Both exact tiers: every bit equal; the fp16-table
identity and the dead-level test: every bit equal; rounding tier: at most 1.5e-7 of 4.8e-7.
(The fp32 child runs every size below the hybrid one.)
Mutations of csrc/field_fused.hip, each built once beside the tree and run once on the 253 default-build tests (never
committed):
  layer_bf / layer_bf2 without the xl * wh product     first failure test_forward[dense_coarse-fwd_rgb]; 198 of 253 fail
      (every case of the bf16x3 MLP in both tiers - the exact tier's features have 12 significant bits and need the
      remainder plane - and the device-count tests; the fp16 MLP and the identity tests rightly pass).
  blend: corner weights y1z0 / y0z1 of the fine levels exchanged   first failure test_forward[dense_coarse-fwd_rgb];
      185 of 253 fail, both tiers, every table with a fine level (the 5-level table, and k_nerf_fwd_pair with its own
      blend, rightly pass).
  pack_f16x2 truncating (v_cvt_pkrtz) instead of rounding   first failure test_forward[levels5-table_m16], 1 of 253: a
      truncation stays inside 2 x the rounding model's worst case nearly everywhere.  That gap is what the rounding tier
      closes: with it, all 6 test_fp16_mlp_rounds_to_nearest_even cases fail on that library (run once more, that test
      alone) and pass on the tree's.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_backward_reference as B  # noqa: E402
import sample_records_ref as S  # noqa: E402
from field_backward_reference import Exact64, worst_ratio, sigbits, quantum, _rng, _u  # noqa: E402,F401
from train_kernels_reference import sh64  # noqa: E402

F32, F64 = np.float32, np.float64
BUILDS = B.BUILDS
KS = B.KS
SO0_SCALE = 20.0
SMALL_SIZES = (1, 15, 16, 17, 31, 32, 33, 16 * 61 + 7)
HYBRID_MIN_TILES = 4 << 13        # HybridSchedule::begin: (n_tiles >> (kXcdChunkLog2 + 3)) >= 4, kXcdChunkLog2 = 10
BIG = 16 * HYBRID_MIN_TILES + 7
BIG_STEP = 61                     # the CPU measurement of MEASURED takes every 61st sample of the hybrid-schedule size
NUMERICS = {"": 0, "t16": 1, "m16": 2, "o": 3}
MARGIN = {"": 8.0, "t16": 2.0, "m16": 2.0, "o": 2.0}

TABLE_SPECS = {
    "dense_coarse": dict(base_resolution=4, desired_resolution=2048, log2_hashmap_size=19),
    "hashed_all": dict(base_resolution=16, desired_resolution=2048, log2_hashmap_size=12),
    "bench": dict(base_resolution=16, desired_resolution=2048, log2_hashmap_size=19),
    "all_dense": dict(base_resolution=4, desired_resolution=64, log2_hashmap_size=19),
    "levels12": dict(num_levels=12, base_resolution=16, desired_resolution=1024, log2_hashmap_size=19),
    "levels5": dict(num_levels=5, base_resolution=16, desired_resolution=128, log2_hashmap_size=19),
}
EXACT_SPECS = {
    "x16": dict(num_levels=16, base_resolution=2, log2_hashmap_size=10, per_level_scale=2.0),
    "x12": dict(num_levels=12, base_resolution=2, log2_hashmap_size=10, per_level_scale=2.0),
}
ALIASES = {"levels5_b15": "levels5"}      # the plain feeds once more at bound 1.5 (2 bound no power of two)
PLAIN_ONLY_ENTRIES = ("fwd_rgb", "fwd_density", "dirs3", "instance16")
TOL_TABLES, EXACT_TABLES = tuple(TABLE_SPECS) + tuple(ALIASES), tuple(EXACT_SPECS)
# per table: (bound, density_scale); tolerance tier 1 / 2 and 1 / 0.3, exact tier powers of two
SETTINGS = {"dense_coarse": (1.0, 1.0), "hashed_all": (2.0, 0.3), "bench": (1.0, 0.3), "all_dense": (2.0, 1.0),
            "levels12": (2.0, 0.3), "levels5": (1.0, 1.0), "levels5_b15": (1.5, 0.3), "x16": (1.0, 0.5), "x12": (2.0, 2.0)}
ROUNDING_TOL = 8 * 2.0 ** -24
ROUNDING_ENTRIES = ("table_m16", "table_o", "fwd_o")
LOGIT_MIN = {"tol": -2.5, "exact": -0.75}


def level_table(num_levels=16, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048, per_level_scale=None):
    """The level table of gridencoder.level_table (3-D, two features), restated: resolution_l = ceil(base * pls^l),
    rows_l = min(2^log2_hashmap_size, (resolution_l + 1)^3) rounded up to 8, scale_l = float32(base * pls^l - 1), a level
    is hashed iff (ceil(scale_l) + 2)^3 > rows_l."""
    if per_level_scale is None:
        per_level_scale = np.exp2(np.log2(desired_resolution / base_resolution) / max(num_levels - 1, 1))
    pls = float(per_level_scale)
    offsets, scales, ress, hashed = [0], [], [], []
    for l in range(num_levels):
        res = int(np.ceil(base_resolution * pls ** l))
        rows = int(np.ceil(min(2 ** log2_hashmap_size, (res + 1) ** 3) / 8) * 8)
        offsets.append(offsets[-1] + rows)
        scale = np.float32(np.exp2(l * np.log2(pls)) * base_resolution - 1.0)
        gres = int(np.ceil(scale)) + 1
        scales.append(scale)
        ress.append(gres)
        hashed.append(1 if (gres + 1) ** 3 > rows else 0)
    return dict(num_levels=num_levels, level_dim=2, per_level_scale=pls, offsets=np.asarray(offsets, np.uint32),
                scales=np.asarray(scales, F32), resolutions=np.asarray(ress, np.uint32),
                hashed=np.asarray(hashed, np.uint32), total_rows=int(offsets[-1]))


@functools.lru_cache(maxsize=None)
def table_for(name):
    name = ALIASES.get(name, name)
    return level_table(**(TABLE_SPECS[name] if name in TABLE_SPECS else EXACT_SPECS[name]))


def tier_of(table):
    return "exact" if table in EXACT_SPECS else "tol"


# |model - float64| / cond, largest over the tolerance-tier cases (value seen -> constant, two digits, rounded up)
MEASURED = {
    "bf16x3": {
        "c1": 1.1e-05,              # 1.033e-05
        "c2": 2.7e-06,              # 2.680e-06
        "cin": 2.5e-06,             # 2.402e-06
        "enc": 2.7e-07,             # 2.672e-07
        "geo": 2.5e-06,             # 2.402e-06
        "h1": 1.6e-05,              # 1.547e-05
        "ienc": 2.7e-07,            # 2.672e-07
        "ih1": 1.8e-05,             # 1.773e-05
        "ih2": 3.4e-06,             # 3.328e-06
        "logit": 1.8e-06,           # 1.737e-06
        "logits": 4.0e-07,          # 3.926e-07
        "rgb": 2.3e-07,             # 2.218e-07
        "rgb@m16": 2.9e-07,         # 2.848e-07
        "rgb@o": 4.5e-06,           # 4.460e-06
        "rgb@t16": 6.0e-08,         # 5.964e-08
        "rgbm": 1.9e-07,            # 1.806e-07
        "sigma": 1.8e-06,           # 1.724e-06
        "sigma1": 1.3e-06,          # 1.262e-06
        "sigma@m16": 4.2e-05,       # 4.103e-05
        "sigma@o": 4.1e-05,         # 4.057e-05
        "sigma@t16": 1.4e-05,       # 1.332e-05
        "so": 2.5e-06,              # 2.402e-06
    },
    "fp32": {
        "c1": 1.4e-07,              # 1.357e-07
        "c2": 3.4e-08,              # 3.394e-08
        "cin": 6.0e-08,             # 5.904e-08
        "enc": 2.7e-07,             # 2.672e-07
        "geo": 2.2e-08,             # 2.141e-08
        "h1": 1.5e-07,              # 1.472e-07
        "ienc": 2.7e-07,            # 2.672e-07
        "ih1": 1.9e-07,             # 1.813e-07
        "ih2": 2.9e-08,             # 2.855e-08
        "logit": 1.6e-08,           # 1.501e-08
        "logits": 4.1e-09,          # 4.010e-09
        "rgb": 6.1e-09,             # 6.022e-09
        "rgb@t16": 6.4e-08,         # 6.396e-08
        "rgbm": 5.5e-09,            # 5.438e-09
        "sigma": 1.5e-08,           # 1.440e-08
        "sigma1": 1.2e-08,          # 1.194e-08
        "sigma@t16": 1.4e-05,       # 1.342e-05
        "so": 2.2e-08,              # 2.141e-08
    },
}
TOL = {b: {k: MARGIN[k.partition("@")[2]] * v for k, v in m.items()} for b, m in MEASURED.items()}


# ---------------------------------------------------------------------------- number formats and models
def rne_f16(x):
    """fp32 value -> nearest fp16 (ties to even), as float64."""
    with np.errstate(over="ignore"):
        return np.asarray(x, F64).astype(F32).astype(np.float16).astype(F64)


class HalfMlp(B._Fp32Steps):
    """INR_NUMERICS_MLP_F16: one v_mfma_f32_16x16x32_f16 pass per layer on fp16 operands, fp32 accumulation."""
    name = "m16"

    def __init__(self, log=None, truncate=False):
        self.log, self.truncate = log, truncate          # truncate: the WRONG conversion (toward zero), for the tests

    def layer(self, W, x):
        xh = rne_f16(x)
        if self.truncate:
            xh = np.where(np.abs(xh) > np.abs(x), np.nextafter(xh.astype(np.float16), np.float16(0)).astype(F64), xh)
        if self.log is not None:
            self.log.append(("layer", rne_f16(W), xh))
        return self.r(xh @ rne_f16(W).T)


def model_for(build, numerics):
    """The arithmetic model of a launch: numerics "", "t16", "m16", "o" -> (model, table rounded to fp16?)."""
    half_mlp = bool(NUMERICS[numerics] & 2)
    assert not (half_mlp and build == "fp32"), "the exact-fp32 build has no fp16 MLP"
    return (HalfMlp() if half_mlp else B.MODELS[build]()), bool(NUMERICS[numerics] & 1)


def sh_abs(d):
    """cond of SH-4 of a direction: the polynomial over |x|, |y|, |z| with every coefficient positive."""
    d = np.abs(np.asarray(d, F64))
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    out = [0.0 * x + 0.28209479177387814, 0.48860251190291987 * y, 0.48860251190291987 * z, 0.48860251190291987 * x,
           1.0925484305920792 * xy, 1.0925484305920792 * yz, 0.94617469575755997 * z2 + 0.31539156525251999,
           1.0925484305920792 * xz, 0.54627421529603959 * (x2 + y2), 0.59004358992664352 * y * (3.0 * x2 + y2),
           2.8906114426405538 * xy * z, 0.45704579946446572 * y * (1.0 + 5.0 * z2),
           0.3731763325901154 * z * (5.0 * z2 + 3.0), 0.45704579946446572 * x * (1.0 + 5.0 * z2),
           1.4453057213202769 * z * (x2 + y2), 0.59004358992664352 * x * (x2 + 3.0 * y2)]
    return np.stack(out, -1)


# ---------------------------------------------------------------------------- specification: x01, cells, rows
def x01_plain(x, bound):
    """-> (x01 fp32 with out-of-range rows replaced by 0, oob [M])."""
    x01 = S.x01_div(x, bound)
    with np.errstate(invalid="ignore"):
        oob = ~((x01 >= 0) & (x01 <= 1)).all(-1)
    return np.where(oob[:, None], F32(0), x01).astype(F32), oob


def x01_lattice(ax_w, ax_l, ax_h, bound):
    """Points of the [W, L, H] lattice in that order, each axis value clamped to [-bound, bound] first."""
    b = F32(bound)
    c = [np.minimum(np.maximum(np.asarray(a, F32), -b), b) for a in (ax_w, ax_l, ax_h)]
    g = np.stack(np.meshgrid(*c, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    return x01_plain(g, bound)


def x01_records(o, d, ray_ids, t, bound):
    return S.x01_mul(S.position(np.asarray(o, F32)[ray_ids], np.asarray(d, F32)[ray_ids], t, bound), bound)


def cells(x01, table):
    """-> (cell uint32 [M,L,3], fraction fp32 [M,L,3]): p = x01 * scale + 0.5 (mul, add), floor, p - floor."""
    s = np.asarray(table["scales"], F32)
    pos = (np.asarray(x01, F32)[:, None, :] * s[None, :, None]).astype(F32) + F32(0.5)
    fl = np.floor(pos)
    return fl.astype(np.int64).astype(np.uint32), (pos - fl).astype(F32)


def level_rows(cell_l, table, l):
    """Absolute table row of the eight corners of level l, int64 [M,8] (cell_l uint32 [M,3]); corner k: bit d of k
    selects the +1 neighbour on axis d.  uint32 arithmetic with wrap-around, as the kernel's."""
    off, rows = int(table["offsets"][l]), int(table["offsets"][l + 1]) - int(table["offsets"][l])
    idx = np.empty((len(cell_l), 8), np.int64)
    with np.errstate(over="ignore"):
        for k in range(8):
            cx = cell_l[:, 0] + np.uint32(k & 1)
            cy = cell_l[:, 1] + np.uint32((k >> 1) & 1)
            cz = cell_l[:, 2] + np.uint32((k >> 2) & 1)
            if table["hashed"][l]:
                assert rows & (rows - 1) == 0
                r = (cx ^ (cy * np.uint32(2654435761)) ^ (cz * np.uint32(805459861))) & np.uint32(rows - 1)
            else:
                s = np.uint32(int(table["resolutions"][l]) + 1)
                r = cx + cy * s + cz * (s * s)
            idx[:, k] = r.astype(np.int64) + off
    return idx


def row_index(cell, table):
    """level_rows of every level -> int64 [M,L,8]."""
    return np.stack([level_rows(cell[:, l], table, l) for l in range(cell.shape[1])], 1)


def encode(mod, table, emb, x01, oob, log=None):
    """-> (enc [M,32], cond [M,32]) float64: level l in features 2l, 2l+1; dead levels and out-of-range rows zero."""
    x01 = np.asarray(x01, F32)
    M, L = len(x01), int(table["num_levels"])
    enc, cond = np.zeros((M, 32)), np.zeros((M, 32))
    if M == 0:
        return enc, cond
    cell, fr = cells(x01, table)
    emb = np.asarray(emb, F64)
    for l in range(L):
        f1 = fr[:, l, :].astype(F64)
        f0 = mod.r(1.0 - f1)
        v = emb[level_rows(cell[:, l], table, l)]                                         # [M,8,2]
        w = []
        for k in range(8):
            wx, wy, wz = ((f1 if (k >> a) & 1 else f0)[:, a] for a in range(3))
            w.append(mod.r(mod.r(wx * wy) * wz))
        w = np.stack(w, 1)                                               # [M,8]
        if log is not None:
            log.append(("blend", v[~oob].reshape(-1, 1), w[~oob].reshape(-1, 1)))
        cond[:, 2 * l:2 * l + 2] = (np.abs(w)[:, :, None] * np.abs(v)).sum(1)
        if l < 8:                                                        # fma chain in corner order
            acc = np.zeros((M, 2))
            for k in range(8):
                acc = mod.r(w[:, k, None] * v[:, k] + acc)
        else:                                                            # each x side's yz corners, then side 0 + side 1
            side = []
            for sx in range(2):
                a = np.zeros((M, 2))
                for yz in range(4):
                    a = mod.r(w[:, sx + 2 * yz, None] * v[:, sx + 2 * yz] + a)
                side.append(a)
            acc = mod.r(side[0] + side[1])
        enc[:, 2 * l:2 * l + 2] = acc
    enc[oob], cond[oob] = 0.0, 0.0
    return enc, cond


# ---------------------------------------------------------------------------- the networks
def _relu(p):
    return np.where(p > 0, p, 0.0)


def _lin(mod, W, x, cx):
    return mod.layer(W, x), cx @ np.abs(np.asarray(W, F64)).T


def sigma_part(mod, W, enc, cenc, density_scale):
    """-> (out, cond): h1 [M,64], so [M,16], sigma [M], geo [M,15]."""
    ws0, ws1 = np.asarray(W[0], F64), np.asarray(W[1], F64)
    o, c = {"enc": enc}, {"enc": cenc}
    p, c["h1"] = _lin(mod, ws0, enc, cenc)
    o["h1"] = _relu(p)
    o["so"], c["so"] = _lin(mod, ws1, o["h1"], c["h1"])
    ds = float(F32(density_scale))
    o["sigma"] = mod.r(mod.exp(o["so"][:, 0]) * ds)
    true_sigma = np.exp(o["so"][:, 0]) * ds
    c["sigma"] = true_sigma * c["so"][:, 0] + true_sigma
    o["sigma1"] = mod.r(mod.exp(o["so"][:, 0]) * 1.0)           # the training entry points apply no density_scale
    c["sigma1"] = np.exp(o["so"][:, 0]) * c["so"][:, 0] + np.exp(o["so"][:, 0])
    o["geo"], c["geo"] = o["so"][:, 1:], c["so"][:, 1:]
    return o, c


def colour_part(mod, W, sh, csh, so, cso):
    """sh [M,16] float64 (a direction's SH values or an SH-table row) -> (out, cond): cin [M,32] (16 SH, 15 geo, one
    zero column), c1, c2 [M,64], o [M,3], rgb [M,3]."""
    wc0, wc1, wc2 = (np.asarray(w, F64) for w in W[2:5])
    o, c = {}, {}
    cin, ccin = np.concatenate([sh, so[:, 1:]], 1), np.concatenate([csh, cso[:, 1:]], 1)
    z = np.zeros((len(sh), 1))
    o["cin"], c["cin"] = np.concatenate([cin, z], 1), np.concatenate([ccin, z], 1)
    p, c["c1"] = _lin(mod, wc0, cin, ccin)
    o["c1"] = _relu(p)
    p, c["c2"] = _lin(mod, wc1, o["c1"], c["c1"])
    o["c2"] = _relu(p)
    o["o"], c["o"] = _lin(mod, wc2, o["c2"], c["c2"])
    o["rgb"] = mod.sigmoid(o["o"])
    s = 1.0 / (1.0 + np.exp(-o["o"]))
    c["rgb"] = s * (1.0 - s) * c["o"] + s
    return o, c


def dirs_part(mod, W, sh_dirs, so, cso, logit_min):
    """k_nerf_fwd_dirs -> (out, cond): rgbm [M,3] mean colour over the directions (summed in fp32 one by one, then
    * 1/D), logit [M] = max(so0, logit_min) (max is 1-Lipschitz: cond(so0))."""
    D = len(sh_dirs)
    acc, cacc = np.zeros((len(so), 3)), np.zeros((len(so), 3))
    for dd in range(D):
        row = np.repeat(np.asarray(sh_dirs, F64)[dd:dd + 1], len(so), 0)
        oo, cc = colour_part(mod, W, row, np.abs(row), so, cso)
        acc, cacc = mod.r(acc + oo["rgb"]), cacc + cc["rgb"]
    inv = float(F32(1.0) / F32(D))
    out = {"rgbm": mod.r(acc * inv), "logit": np.maximum(so[:, 0], float(F32(logit_min)))}
    return out, {"rgbm": cacc / D + np.abs(acc) / D, "logit": cso[:, 0]}


def instance_part(mod, W, enc, cenc):
    w0, w1, w2 = (np.asarray(w, F64) for w in W)
    o, c = {"ienc": enc}, {"ienc": cenc}
    p, c["ih1"] = _lin(mod, w0, enc, cenc)
    o["ih1"] = _relu(p)
    p, c["ih2"] = _lin(mod, w1, o["ih1"], c["ih1"])
    o["ih2"] = _relu(p)
    o["logits"], c["logits"] = _lin(mod, w2, o["ih2"], c["ih2"])
    return o, c


# ---------------------------------------------------------------------------- inputs
def embeddings(table):
    """The table's values: tolerance tier U(-1,1); exact tier integers in -2 .. 2, both features of a row equal on
    levels 0..7 (columns 2i, 2i+1 of enc equal for i < 8: so0 == 0 on the data, see nerf_exact_case)."""
    t = table_for(table)
    rows = int(t["total_rows"])
    if tier_of(table) == "tol":
        return _u(_rng("fwd_emb", table), (rows, 2), 1.0)
    emb = _rng("fwd_emb", table).integers(-2, 3, size=(rows, 2)).astype(F32)
    coarse = int(t["offsets"][min(8, t["num_levels"])])
    emb[:coarse, 1] = emb[:coarse, 0]
    return emb


def _zero_dead(w, table):
    w[:, 2 * int(table_for(table)["num_levels"]):] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def nerf_weights(table, variant=None):
    """Tolerance tier: U(+-0.35) / U(+-0.25), density row centred and scaled.  Exact tier: the backward suite's exact
    weights, variant a | b | c (so0 == 0 on the data, colour logits 0) or "logit": variant a with a live density row
    of +-1.  Columns of dead levels are zero."""
    if tier_of(table) == "tol":
        rng = _rng("fwd_nerf_w", table)
        W = [_u(rng, (64, 32), 0.35), _u(rng, (16, 64), 0.25), _u(rng, (64, 31), 0.35), _u(rng, (64, 64), 0.25),
             _u(rng, (3, 64), 0.25)]
        W[1][0] = (W[1][0] - W[1][0].mean()) * F32(SO0_SCALE)
    else:
        W = [w.copy() for w in B.nerf_exact_case(0, "a" if variant in (None, "logit") else variant)["W"]]
        if variant in ("logit", "live"):
            W[1][0] = B._sparse(_rng("fwd_logit", table), 1, 64)[0]
        if variant == "live":                            # live colour logits too (the rounding tier)
            W[4] = B._sparse(_rng("fwd_live", table), 3, 64)
    _zero_dead(W[0], table)
    return W


@functools.lru_cache(maxsize=None)
def instance_weights(table, K):
    if tier_of(table) == "tol":
        rng = _rng("fwd_inst_w", table, K)
        W = [_u(rng, (64, 32), 0.35), _u(rng, (64, 64), 0.25), _u(rng, (K, 64), 0.25)]
    else:
        W = [w.copy() for w in B.instance_exact_case(0, K)["W"]]
    _zero_dead(W[0], table)
    return W


def sh_dirs_rows(table, D):
    """[D,16] rows of the dirs kernels: SH of fixed directions (tolerance tier, float64 rounded to fp32: inputs) or
    small integers (exact tier; Wc0 is zero on those columns)."""
    rng = _rng("fwd_shdirs", table, D)
    if tier_of(table) == "exact":
        return rng.integers(-2, 3, size=(D, 16)).astype(F32)
    d = rng.standard_normal((D, 3))
    return sh64(d / np.linalg.norm(d, axis=1, keepdims=True), 4).astype(F32)


def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def _specials(table, bound, grid):
    """World positions of the first rows: faces, centre, cell boundaries of the coarsest and the finest level."""
    t = table_for(table)
    s0, s1 = float(t["scales"][0]), float(t["scales"][-1])
    if grid:                                             # exact tier: faces and centre; the rest lies on the grid anyway
        u = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1, 0, 0.25], [1.0 / grid, 1, 1 - 1.0 / grid]]
    else:
        u = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1, 0, 0.25], [2.5 / s0, 0.5 / s0, 7.5 / s0],
             [(np.floor(0.8 * s1) + 0.5) / s1, 3.5 / s1, 0.0], [0.03125, 0.96875, 0.5]]
    u = np.asarray(u, F32)
    return (u * F32(2.0 * bound) - F32(bound)).astype(F32)


@functools.lru_cache(maxsize=4)
def scene(table, M, bound, grid=0):
    """Rays and samples shared by the three feeds of a case: o, d [N,3], ray_ids [M] (sorted), t [M]; x [M,3] the
    clamped positions p = clamp(o + t d) (plain feed, without the outside / NaN rows), x01 [M,3] (table feed), dirs
    [M,3], shrow [N,16] the SH-table rows (inputs).  grid: 0, or 8 / 4 for exact-tier positions with x01 on multiples of
    1 / grid (t = 0: the position is the ray's origin)."""
    rng = _rng("fwd_scene", table, M, bound, grid)
    sp = _specials(table, bound, grid)[:M]
    ns = len(sp)
    N = ns + max(1, M // 5)
    b = F32(bound)
    o, d = _u(rng, (N, 3), 0.9 * bound), _unit(rng, N)
    o[:ns] = sp
    ray_ids = np.concatenate([np.arange(ns), np.sort(rng.integers(ns, N, size=M - ns))]).astype(np.int32)
    t = _u(rng, (M,), 0.5 * bound) + F32(0.5 * bound)
    t[:ns] = 0.0
    if grid:
        N = M + 1                                        # one ray per sample and one without a sample
        o = (rng.integers(0, grid + 1, size=(N, 3)).astype(F32) / F32(grid) * (2 * b) - b).astype(F32)
        o[:ns] = sp
        d, ray_ids, t = _unit(rng, N), np.arange(M, dtype=np.int32), np.zeros(M, F32)
    x = S.position(o[ray_ids], d[ray_ids], t, bound)
    x01 = S.x01_mul(x, bound)
    if float(2 * bound) == 2.0 ** round(np.log2(2 * bound)):
        assert (x01 == S.x01_div(x, bound)).all()
    if grid:
        assert (x01 * grid == np.round(x01 * grid)).all()
        shrow = rng.integers(-2, 3, size=(N, 16)).astype(F32)
    else:
        shrow = sh64(d, 4).astype(F32)
    return dict(o=o, d=d, ray_ids=ray_ids, t=t, x=x, x01=x01, dirs=d[ray_ids], shrow=shrow, N=N, bound=bound)


def plain_x(sc, bound):
    """The plain feeds' positions: the scene's, with one row outside the volume and one NaN row."""
    x = sc["x"].copy()
    if len(x) > 9:
        x[9] = [1.5 * bound, 0.0, 0.0]
    if len(x) > 11:
        x[11] = [np.nan, 0.1 * bound, -0.2 * bound]
    return x


def lattice_axes(table, bound):
    """W = 19 (no multiple of 16), L = 3, H = 5; ax_w holds a value outside the bound (clamped to the face)."""
    rng = _rng("fwd_lattice", table)
    b = F32(bound)
    if tier_of(table) == "exact":
        ax = [(rng.integers(0, 9, size=n).astype(F32) / F32(8) * (2 * b) - b).astype(F32) for n in (19, 3, 5)]
    else:
        ax = [_u(rng, (n,), bound) for n in (19, 3, 5)]
    ax[0][4], ax[2][1] = F32(1.25) * b, -F32(3.0) * b
    return ax


def q_rows(sh):
    """[N,16] SH rows -> the table feed's sh_table_q [N,4,4]: row q holds components (q, 4+q, 8+q, 12+q)."""
    return np.ascontiguousarray(np.asarray(sh, F32).reshape(-1, 4, 4).transpose(0, 2, 1))


# ---------------------------------------------------------------------------- one reference per (table, size)
class Reference:
    """Everything the entry points of one (table, size) are compared with, on one model; the encoder runs once per
    feed class ("plain": with the outside / NaN rows; "table": the table, sliced and records feeds)."""

    def __init__(self, table, M, mod=None, half_table=False, grid=None, log=None, variant=None, step=1):
        self.table, self.mod = table, mod or Exact64(log)
        self.t = table_for(table)
        self.bound, self.ds = SETTINGS[table]
        self.tier = tier_of(table)
        if grid is None:
            grid = 8 if self.tier == "exact" else 0
        self.sc = scene(table, M, self.bound, grid)
        if step != 1:                                    # every step-th sample (samples are independent of each other)
            self.sc = {k: (v[::step] if k in ("ray_ids", "t", "x", "x01", "dirs") else v) for k, v in self.sc.items()}
        self.M = len(self.sc["t"])
        emb = embeddings(table)
        self.emb = rne_f16(emb) if half_table else emb.astype(F64)
        self.W = nerf_weights(table, variant)
        self.log = log
        self._cache = {}

    def _enc(self, feed):
        if feed not in self._cache:
            if feed == "plain":
                x01, oob = x01_plain(plain_x(self.sc, self.bound), self.bound)
            elif feed == "table":
                x01, oob = self.sc["x01"], np.zeros(self.M, bool)
            else:
                x01, oob = x01_lattice(*lattice_axes(self.table, self.bound), self.bound)
            self._cache[feed] = encode(self.mod, self.t, self.emb, x01, oob, self.log)
        return self._cache[feed]

    def sigma(self, feed):
        key = ("sigma", feed)
        if key not in self._cache:
            self._cache[key] = sigma_part(self.mod, self.W, *self._enc(feed), self.ds)
        return self._cache[key]

    def nerf(self, feed, sh=None):
        """feed plain: SH of the samples' directions; table: the SH-table rows ``sh`` [N,16] (default: the scene's) of
        the samples' rays -> (out, cond) with every array of sigma_part and colour_part."""
        o, c = self.sigma(feed)
        if feed == "plain":
            d = self.sc["dirs"]
            shv, csh = self.mod.sh(d), sh_abs(d)
        else:
            shv = np.asarray(self.sc["shrow"] if sh is None else sh, F64)[self.sc["ray_ids"]]
            csh = np.abs(shv)
        o2, c2 = colour_part(self.mod, self.W, shv, csh, o["so"], c["so"])
        return {**o, **o2}, {**c, **c2}

    def dirs(self, feed, D):
        o, c = self.sigma(feed)
        return dirs_part(self.mod, self.W, sh_dirs_rows(self.table, D), o["so"], c["so"], LOGIT_MIN[self.tier]
                         if feed == "lattice" else -np.inf)

    def instance(self, K):
        return instance_part(self.mod, instance_weights(self.table, K), *self._enc("plain"))


@functools.lru_cache(maxsize=3)
def _small_reference(table, M, variant, grid):
    return Reference(table, M, variant=variant, grid=grid)


@functools.lru_cache(maxsize=1)
def _big_reference(table, M, variant, grid):
    return Reference(table, M, variant=variant, grid=grid)


def reference(table, M, variant=None, grid=None):
    """The float64 reference of a (table, size), computed once and shared by the entry points (the hybrid-schedule size
    has a cache slot of its own)."""
    return (_big_reference if M >= BIG else _small_reference)(table, M, variant, grid)


# ---------------------------------------------------------------------------- exact tier preconditions
def exactness_violations(log, fp16=False):
    """The exact tier's preconditions on the operand pairs a float64 run has logged -> list of complaints.  Layers: the
    backward suite's rules (<= 16 significant bits into every product, <= 8 on one side, sum |terms| < 2^24 quanta).
    Blend: weight x table value under the same rules, and the eight terms of a feature sum within 2^24 quanta.  fp16:
    every layer input that meets a non-zero weight, every weight and every table value is an fp16 number (<= 11
    significant bits, magnitude in [2^-14, 65504] or zero)."""
    bad = B.exactness_violations([e for e in log if e[0] == "layer"])
    for i, (kind, A, Bv) in enumerate(log):
        if kind == "blend":
            sa, sb = sigbits(A), sigbits(Bv)
            if max(sa, sb) > 16 or min(sa, sb) > 8:
                bad.append(f"blend {i}: {sa} x {sb} significant bits")
            if 8 * np.abs(A).max(initial=0) * np.abs(Bv).max(initial=0) / (quantum(A) * quantum(Bv)) >= 2.0 ** 24:
                bad.append(f"blend {i}: sum of terms too wide")
        if not fp16:
            continue
        ops = [A] if kind == "blend" else [A, Bv[:, (A != 0).any(0)]]
        for v in ops:
            nz = np.abs(v[v != 0])
            if sigbits(v) > 11 or (nz.size and (nz.max() > 65504 or nz.min() < 2.0 ** -14)):
                bad.append(f"{kind} {i}: not an fp16 operand ({sigbits(v)} bits)")
    return bad


# ---------------------------------------------------------------------------- the case lists
# entry point -> (feed, numerics, outputs compared in the tolerance tier, outputs compared bit for bit in the exact tier)
NERF_ENTRIES = {
    "fwd_rgb": ("plain", "", ("sigma", "rgb"), ("sigma", "rgb")),
    "fwd_density": ("plain", "", ("sigma", "geo"), ("sigma", "geo")),
    "fwd_o": ("plain", "o", ("sigma", "rgb"), ("sigma", "rgb")),
    "train": ("plain", "", ("sigma1", "rgb", "enc", "h1", "so", "cin", "c1", "c2"),
              ("sigma1", "rgb", "enc", "h1", "so", "cin", "c1", "c2")),
    "enc": ("plain", "", ("sigma1", "rgb", "enc"), ("sigma1", "rgb", "enc")),
    "table": ("table", "", ("sigma", "rgb"), ("sigma", "rgb")),
    "table_t16": ("table", "t16", ("sigma", "rgb"), ("sigma", "rgb")),
    "table_m16": ("table", "m16", ("sigma", "rgb"), ("sigma", "rgb")),
    "table_o": ("table", "o", ("sigma", "rgb"), ("sigma", "rgb")),
    "sliced": ("table", "", ("sigma", "rgb"), ("sigma", "rgb")),
    "records": ("table", "", ("sigma", "rgb"), ("sigma", "rgb")),
    "records_nopair": ("table", "", ("sigma", "rgb"), ("sigma", "rgb")),
    "dirs1": ("plain", "", ("rgbm", "logit"), ("rgbm", "logit")),
    "dirs3": ("plain", "", ("rgbm", "logit"), ("rgbm", "logit")),
    "dirs8": ("plain", "", ("rgbm", "logit"), ("rgbm", "logit")),
    "lattice": ("lattice", "", ("rgbm", "logit"), ("rgbm", "logit")),
}
INSTANCE_ENTRIES = {f"instance{mode}{K}": (mode, K) for K in KS for mode in ("", "_train", "_enc")}
ENTRIES = tuple(NERF_ENTRIES) + tuple(INSTANCE_ENTRIES)
BIG_ENTRIES = ("fwd_rgb", "table", "records")
BIG_TABLE = "bench"


def sliceable(table):
    t = table_for(table)
    return int(t["num_levels"]) == 16 and bool(np.asarray(t["hashed"])[8:].all())


def applies(table, entry, build="bf16x3"):
    if table in ALIASES and entry not in PLAIN_ONLY_ENTRIES:
        return False
    if entry == "sliced" and not sliceable(table):
        return False
    if build == "fp32" and entry in NERF_ENTRIES and NUMERICS[NERF_ENTRIES[entry][1]] & 2:
        return False
    return True


def sizes_for(table, entry):
    if entry == "lattice":
        return (19 * 3 * 5,)
    if table in ALIASES:
        return (17, 16 * 61 + 7)
    return SMALL_SIZES + ((BIG,) if table == BIG_TABLE and entry in BIG_ENTRIES else ())


def cases(build="bf16x3"):
    """[(table, entry)] of both tiers, table-major (the reference of a (table, size) is cached)."""
    return [(t, e) for t in TOL_TABLES + EXACT_TABLES for e in ENTRIES if applies(t, e, build)]


def variant_for(table, entry):
    """Exact tier: which weight variant an entry point runs (a, b, c rotate; the dirs kernels get a live density row)."""
    if tier_of(table) != "exact":
        return None
    if entry.startswith("dirs") or entry == "lattice":
        return "logit"
    return "abc"[list(NERF_ENTRIES).index(entry) % 3] if entry in NERF_ENTRIES else None


def grid_for(table, entry):
    if tier_of(table) != "exact":
        return 0
    return 4 if entry in NERF_ENTRIES and NUMERICS[NERF_ENTRIES[entry][1]] & 2 else 8


def expected(ref, entry, sh=None):
    """(out, cond) of an entry point on ``ref`` restricted to the outputs the entry point writes."""
    if entry in INSTANCE_ENTRIES:
        mode, K = INSTANCE_ENTRIES[entry]
        o, c = ref.instance(K)
        names = {"": ("logits",), "_train": ("logits", "ienc", "ih1", "ih2"), "_enc": ("logits", "ienc")}[mode]
    else:
        feed, _, names, _ = NERF_ENTRIES[entry]
        if entry.startswith("dirs") or entry == "lattice":
            o, c = ref.dirs(feed, 3 if entry == "lattice" else int(entry[4:]))
        else:
            o, c = ref.nerf(feed, sh)
    return {k: o[k] for k in names}, {k: c[k] for k in names}


def tol_key(entry, name):
    num = NERF_ENTRIES[entry][1] if entry in NERF_ENTRIES else ""
    return name + ("@" + num if num else "")


def measure(build, table, entry, M):
    """The model of ``build`` and the entry's numerics against float64 -> {tolerance key: worst ratio}."""
    num = NERF_ENTRIES[entry][1] if entry in NERF_ENTRIES else ""
    ro, rc = expected(_model_reference("float64", "", table, M), entry)
    mo, _ = expected(_model_reference(build, num, table, M), entry)
    return {tol_key(entry, k): worst_ratio(mo[k], ro[k], rc[k]) for k in ro}


@functools.lru_cache(maxsize=6)
def _model_reference(build, num, table, M):
    mod, half = (Exact64(), False) if build == "float64" else model_for(build, num)
    return Reference(table, M, mod=mod, half_table=half, step=BIG_STEP if M >= BIG else 1)


def measure_all(build, tables=TOL_TABLES):
    """{tolerance key: largest |model - float64| / cond over every tolerance-tier case} of ``build``, size-major per table
    (a reference and a model run per (table, size, numerics) serve every entry point)."""
    worst = {}
    for table in tables:
        sizes = sorted({M for e in ENTRIES if applies(table, e, build) for M in sizes_for(table, e)})
        for M in sizes:
            for e in ENTRIES:
                if applies(table, e, build) and M in sizes_for(table, e):
                    for k, v in measure(build, table, e, M).items():
                        worst[k] = max(worst.get(k, 0.0), v)
    return worst


def rounding_reference(table, entry, M, truncate=False, log=None):
    """(out, model): the HalfMlp model's sigma and rgb of a rounding-tier launch."""
    ref = Reference(table, M, mod=HalfMlp(log, truncate), half_table=True, variant="live", grid=32)
    o, _ = ref.nerf(NERF_ENTRIES[entry][0])
    return {"sigma": o["sigma"], "rgb": o["rgb"]}, ref
