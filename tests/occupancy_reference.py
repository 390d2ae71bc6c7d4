"""Restatements of the occupancy-grid kernels of csrc/raymarch.hip (k_packbits, k_packbits_mean, k_occ_positions,
k_occ_scatter, k_occ_update, k_mark_untrained) and the cases their tests run, NumPy and Python only: nothing here
imports the product or oracle/.

Every operation is written twice.  The ``*32`` functions repeat the kernel's fp32 operations IN THE KERNEL'S ORDER (the
file is built with -ffp-contract=off, every NumPy call below is one IEEE operation per element): the GPU must equal
them bit for bit (tests/test_occupancy_kernels.py).  The ``*64`` functions are the same formulas in float64, the truth;
tests/test_occupancy_cpu.py bounds how far the fp32 restatement stands from them and checks the conditions the cases
have to meet.  Random inputs come from the integer hash ``detections_cases.uniform``.

fmaxf.  C leaves fmaxf(+0, -0) open; IEEE 754-2019 maximumNumber (and the v_max_f32 the compiler emits) orders
-0 < +0 and returns the number when one operand is a NaN.  ``fmax32`` is that function; the sign of a zero is part of
the bit comparison.

The listed update and upstream's rule.  NeRFRenderer.update_extra_state fills ``tmp_grid`` with -1, writes the visited
cells, then updates ``valid_mask = (density_grid >= 0) & (tmp_grid >= 0)`` only (oracle/occupancy.py::update_density_grid
restates it with ``np.full_like(grid, -1.0)``): a cell the list does not visit keeps its value - it does NOT decay - and
so does a visited cell whose scaled sigma is negative or NaN.  The kernel fills its scratch grid with the byte 0xBF,
i.e. the float 0xBFBFBFBF = -1.4980391: any negative fill gives upstream's mask, ``UNVISITED`` below is that value and
``update_listed32`` goes through it the way the kernel does; tests/test_occupancy_cpu.py checks it against the -1 fill."""
import math
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detections_cases import uniform  # noqa: E402

F = np.float32
D = np.float64
U = 2.0 ** -24                                   # unit roundoff of fp32
ONE_BELOW = np.nextafter(F(1.0), F(0.0))
UNVISITED = np.frombuffer(struct.pack("<I", 0xBFBFBFBF), F)[0]


def bits_of(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def ulp32(x):
    x = abs(F(x))
    return float(np.nextafter(x, F(np.inf)) - x)


# ---------------------------------------------------------------------------- Morton codes, written out bit by bit
def compact10(m):
    """Every third bit of m (bits 0, 3, 6, ... 27) gathered into a 10-bit number."""
    m = np.asarray(m).astype(np.int64)
    out = np.zeros_like(m)
    for j in range(10):
        out |= ((m >> (3 * j)) & 1) << j
    return out


def morton3(x, y, z):
    x, y, z = (np.asarray(v).astype(np.int64) for v in (x, y, z))
    out = np.zeros_like(x)
    for j in range(10):
        out |= (((x >> j) & 1) << (3 * j)) | (((y >> j) & 1) << (3 * j + 1)) | (((z >> j) & 1) << (3 * j + 2))
    return out


def coords_of(codes):
    """int64 [n, 3]: x from bit 0, y from bit 1, z from bit 2 of the code."""
    codes = np.asarray(codes).astype(np.int64)
    return np.stack([compact10(codes), compact10(codes >> 1), compact10(codes >> 2)], -1)


# ---------------------------------------------------------------------------- packbits
PACK_BYTES = (1, 255, 256, 257, 4099)
PACK_KINDS = ("t0.5", "t0")
PACK_SENTINEL = 0xA5


def packbits32(grid, thresh, n_bytes):
    """byte k bit i = grid[8k + i] > thresh (strict; a NaN compares false), fp32 comparison."""
    g = np.asarray(grid, F)[:8 * n_bytes].reshape(n_bytes, 8)
    with np.errstate(invalid="ignore"):
        b = g > F(thresh)
    out = np.zeros(n_bytes, np.int64)
    for i in range(8):
        out += b[:, i].astype(np.int64) << i
    return out.astype(np.uint8)


def packbits64(grid, thresh, n_bytes):
    """The same in Python floats (every fp32 is a double: the comparison is the same one), cell by cell."""
    g = [float(v) for v in np.asarray(grid, F)[:8 * n_bytes]]
    t = float(F(thresh))
    out = np.zeros(n_bytes, np.uint8)
    for k in range(n_bytes):
        v = 0
        for i in range(8):
            x = g[8 * k + i]
            if not math.isnan(x) and x > t:
                v |= 1 << i
        out[k] = v
    return out


def packbits_case(n_bytes, kind):
    """-> grid fp32 [8 * n_bytes + 64] (the cells behind n_bytes belong to bytes that must stay untouched), thresh.
    "t0.5": values in [-1, 2), every fifth cell EQUAL to the threshold, the cells next to it one ulp above and below.
    "t0": threshold 0 with +0, -0 (both bit 0), NaN (bit 0), +inf (bit 1), -inf (bit 0) and values either side."""
    n = 8 * n_bytes + 64
    g = (uniform(101 + n_bytes, n) * 3.0 - 1.0).astype(F)
    i = np.arange(n)
    if kind == "t0.5":
        t = F(0.5)
        g[i % 5 == 0] = t
        g[i % 5 == 1] = np.nextafter(t, F(1))
        g[i % 5 == 2] = np.nextafter(t, F(0))
        return g, t
    t = F(0.0)
    for r, v in enumerate((0.0, -0.0, np.nan, np.inf, -np.inf, np.nextafter(F(0), F(1)), -np.nextafter(F(0), F(1)))):
        g[i % 9 == r] = F(v)
    return g, t


# ---------------------------------------------------------------------------- cell positions
POS_N = (1, 255, 256, 257, 1000)
POS_H = (2, 4, 128, 1024)
POS_BOUNDS = (0.5, 1.0, 2.0, 4.0)
POS_NOISE = ("none", "zero", "one_below", "random")
# |fp32 - float64| <= POS_ROUNDINGS * 2^-24 * bound, with u = 2^-24 and b the cascade bound (second-order terms are
# below 2^-20 of that and covered by POS_SLACK).  The expression (2c/(H-1) - 1) * ext + (2n - 1) * half has five
# roundings of its own: the division (result <= 2: 2u), the subtraction (result <= 1: u) - together 3u on a factor that
# ext <= b scales to 3u b - the product (<= b: u b), the product with half (<= b/2: u b/2) and the sum (<= b: u b):
# 5.5 u b.  Its inputs carry three more: half = b / H (u b/2 at most, reaching the result through ext AND through the
# jitter term, each with a factor <= 1: u b), ext = b - half (u b) and 2n - 1 (<= 1: u, scaled by half <= b/2: u b/2).
# 5.5 + 1 + 1 + 0.5 = 8 half-ulps of b, i.e. four fp32 ulps of the extent.
POS_ROUNDINGS = 8
POS_SLACK = 1.0 + 2.0 ** -18


def positions32(codes, noise, H, bound):
    """codes int [n]; noise fp32 [n, 3] in [0, 1) or None -> fp32 [n, 3] in the kernel's order."""
    b = F(bound)
    half = b / F(H)
    ext = b - half
    c = coords_of(codes).astype(F)
    v = (F(2.0) * c / F(H - 1) - F(1.0)) * ext
    if noise is not None:
        v = v + (np.asarray(noise, F) * F(2.0) - F(1.0)) * half
    return v.astype(F)


def positions64(codes, noise, H, bound):
    b = float(F(bound))
    c = coords_of(codes).astype(D)
    v = (2.0 * c / (H - 1) - 1.0) * (b - b / H)
    if noise is not None:
        v = v + (2.0 * np.asarray(noise, F).astype(D) - 1.0) * (b / H)
    return v


def position_codes(n, H, listed):
    """None (the kernel counts 0 .. n-1) or int32 [n]: both corners first, then hashed codes of [0, H^3)."""
    if not listed:
        return None
    H3 = H ** 3
    codes = np.minimum((uniform(7 * H + n, n) * H3).astype(np.int64), H3 - 1)
    codes[0] = morton3(H - 1, H - 1, H - 1)
    if n > 1:
        codes[1] = 0
    return codes.astype(np.int32)


def position_noise(kind, n, seed=0):
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros((n, 3), F)
    if kind == "one_below":
        return np.full((n, 3), ONE_BELOW, F)
    return np.minimum(uniform(900 + seed, 3 * n).astype(F), ONE_BELOW).reshape(n, 3)


def position_cases(n):
    """(H, bound, listed, noise kind) for one n: every H x list x noise; the four bounds rotate through them.  The
    identity list needs H^3 >= n to stay inside the grid, so it runs with H = 128 and 1024 (and H = 2, 4 when they fit)."""
    out = []
    for ih, H in enumerate(POS_H):
        for listed in (False, True):
            if not listed and H ** 3 < n:
                continue
            for ik, kind in enumerate(POS_NOISE):
                out.append((H, POS_BOUNDS[(ih + ik + POS_N.index(n)) % 4], listed, kind))
    return out


# ---------------------------------------------------------------------------- the update
UPDATE_SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)
DECAYS = (0.0, 0.95, 1.0)
SCALES = (0.0, 0.7, 1.0)
OFFSETS = ((0, 0), (1, 0), (0, 1))               # (grid, sigma or tmp) offset in floats: 1 = not 16-byte aligned
LISTED_M = ("0", "1", "half", "double")
WG_CELLS = 1024                                  # one workgroup of 256 lanes takes 4 cells per lane and trip


def workgroup_cap_factor():
    """The k in ``min(ceil(n / 1024), k * CUs)`` workgroups of inr_occ_update, read from the source."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "instance_nerf_amd", "csrc",
                            "raymarch.hip")).read()
    m = re.search(r"std::min<int64_t>\(\(n_cells \+ 1023\) / 1024, \(int64_t\)cu_count\(\) \* (\d+)\)", src)
    return int(m.group(1))


def size_above_cap(cus):
    """The smallest multiple of the per-trip capacity above the cap, plus 2.5 workgroups and a 3-cell tail: every lane
    of the vector path makes a second trip for some cells, the tail too."""
    return workgroup_cap_factor() * cus * WG_CELLS + 2 * WG_CELLS + 512 + 3


def fmax32(a, b):
    """IEEE 754-2019 maximumNumber on fp32 arrays: the number if one operand is a NaN, +0 above -0."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(a >= b, a, b)))
        zz = (a == 0) & (b == 0)
    r = np.where(zz, np.where(np.signbit(a) & np.signbit(b), F(-0.0), F(0.0)), r)
    return r.astype(F)


def update_cells32(g, t_in, decay, scale):
    """k_occ_update's cell: t = t_in * scale; if g >= 0 and t >= 0: g = fmaxf(g * decay, t); else g stays (its bits)."""
    g = np.asarray(g, F)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(t_in, F) * F(scale)
        valid = (g >= 0) & (t >= 0)
        new = fmax32(g * F(decay), t)
    return np.where(valid, new, g).astype(F)


def update_cells64(g, t_in, decay, scale):
    """The same rule with the two products in float64 (exact: a product of two fp32 fits a double)."""
    g = np.asarray(g, F).astype(D)
    with np.errstate(invalid="ignore"):
        t = np.asarray(t_in, F).astype(D) * float(F(scale))
        valid = (g >= 0) & (t >= 0)
        a, b = g * float(F(decay)), t
        new = np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.maximum(a, b)))
    return np.where(valid, new, g)


def mean_term_sum(grid):
    """sum(max(g, 0)) over fp32 cells as the exactly rounded double (a NaN cell adds 0, as fmaxf(NaN, 0) = 0)."""
    g = np.asarray(grid, F).astype(D)
    g = np.where(np.isnan(g), 0.0, np.maximum(g, 0.0))
    if np.isinf(g).any():
        return math.inf
    return math.fsum(g.tolist())


def mean_sum_tolerance(n_cells, total):
    """n_cells * 2^-52 relative: n - 1 additions of non-negative doubles in ANY order err by at most (n - 1) * 2^-53 of
    the sum to first order; the factor 2 covers the higher orders and the exactly rounded reference."""
    return n_cells * 2.0 ** -52 * abs(total)


def update_full32(grid, sigma, decay, scale):
    return update_cells32(grid, sigma, decay, scale)


def update_listed32(grid, sigma, idx, decay, scale):
    """-> (candidates fp32 [m]: the value cell idx[i] takes if entry i is the one the scatter keeps, visited bool [n]).
    The scatter rounds sigma * scale into the scratch grid, the update multiplies by 1 (exact)."""
    grid = np.asarray(grid, F)
    idx = np.asarray(idx).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(sigma, F)[:len(idx)] * F(scale)
    cand = update_cells32(grid[idx], t, decay, 1.0)
    visited = np.zeros(len(grid), bool)
    visited[idx] = True
    assert UNVISITED < 0 and (update_cells32(grid, np.full(len(grid), UNVISITED, F), decay, 1.0).view(np.uint32)
                              == grid.view(np.uint32)).all()
    return cand, visited


def listed_outcome_ok(got, grid, cand, idx, visited):
    """bool [n]: an unvisited cell kept its bits; a visited cell holds the candidate of ONE of its entries."""
    got_b, idx = bits_of(got), np.asarray(idx).astype(np.int64)
    ok = np.zeros(len(grid), bool)
    np.logical_or.at(ok, idx, got_b[idx] == bits_of(cand))
    return np.where(visited, ok, got_b == bits_of(grid))


def update_grid(n, seed, with_inf):
    """Values in [0, 3) with the specials -1, -0.0, 0, NaN (and +inf) on about a third of the cells."""
    g = (uniform(3000 + seed, n) * 3.0).astype(F)
    pick = uniform(4000 + seed, n)
    specials = [-1.0, -0.0, 0.0, np.nan] + ([np.inf] if with_inf else [])
    for k, v in enumerate(specials):
        g[(pick >= k * 0.07) & (pick < (k + 1) * 0.07)] = F(v)
    return g


def update_sigma(m, seed, with_inf):
    """Values in [-0.5, 4) (an eighth negative) with -0.0, NaN (and +inf) on a fifth of the entries."""
    s = (uniform(5000 + seed, m) * 4.5 - 0.5).astype(F)
    pick = uniform(6000 + seed, m)
    specials = [-0.0, np.nan] + ([np.inf] if with_inf else [])
    for k, v in enumerate(specials):
        s[(pick >= k * 0.07) & (pick < (k + 1) * 0.07)] = F(v)
    return s


def update_combos():
    """(decay, scale, with_inf, mean_start): all nine decay x scale; +inf in a third of them (a grid holding +inf has an
    infinite mean, which says nothing about the finite terms); mean_sum starts non-zero in one."""
    out = []
    for i, d in enumerate(DECAYS):
        for j, s in enumerate(SCALES):
            k = 3 * i + j
            out.append((d, s, k % 3 == 0, 1234.5 if k == 4 else 0.0))
    return out


BIG_COMBOS = ((0.95, 0.7, False, 0.0), (1.0, 1.0, True, 0.0))


def listed_indices(n_cells, m_kind, seed):
    """int32 [m]: hashed cells; "double" visits 2 n cells, so most cells twice or more (duplicates with different
    sigmas); "half" makes every fourth entry repeat its neighbour's cell."""
    m = {"0": 0, "1": 1, "half": n_cells // 2, "double": 2 * n_cells}[m_kind]
    idx = np.minimum((uniform(7000 + seed, m) * n_cells).astype(np.int64), n_cells - 1)
    if m_kind == "half":
        idx[3::4] = idx[2::4][:len(idx[3::4])]
    return idx.astype(np.int32)


# ---------------------------------------------------------------------------- packbits with the mean
MEAN_CELLS = (8, 2048, 8 * (256 + 37))
MEAN_BRANCHES = ("mean", "thresh", "negative")
COUNTER_SHAPES = ((1, 1), (3, 2), (16, 1), (16, 2), (0, 1))        # (n_counters, stride)
COUNTER_POISON = 0x40000001


def mean32(mean_sum, n_cells):
    """(float)(mean_sum * (1.0 / n_cells)), the kernel's two operations."""
    return F(D(mean_sum) * (D(1.0) / D(n_cells)))


def packbits_mean32(grid, n_cells, mean_sum, density_thresh):
    """-> bits u8 [n_cells / 8], mean fp32, thresh fp32 = fminf(mean, density_thresh)."""
    mean = mean32(mean_sum, n_cells)
    thresh = min(mean, F(density_thresh))
    return packbits32(grid, thresh, n_cells // 8), mean, thresh


def packbits_mean64(grid, n_cells, mean_sum, density_thresh):
    """Cell by cell against min(mean_sum / n_cells, density_thresh) in float64 (the mean NOT rounded to fp32)."""
    thresh = min(float(mean_sum) / n_cells, float(F(density_thresh)))
    g = np.asarray(grid, F)[:n_cells].astype(D).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        b = g > thresh
    return (b * (1 << np.arange(8))).sum(-1).astype(np.uint8), thresh


def packbits_mean_case(n_cells, branch):
    """-> grid fp32 [n_cells], mean_sum double, density_thresh fp32, equal bool [n_cells] (cells placed ON the
    threshold).  "mean": the mean (about 0.6) is below density_thresh = 10.  "thresh": density_thresh = 0.75 is below
    the mean and every seventh cell equals it.  "negative": density_thresh = -2, below every cell, also the -1 ones."""
    g = (uniform(8000 + n_cells, n_cells) * 2.0).astype(F)
    i = np.arange(n_cells)
    g[i % 5 == 3] = F(-1.0)
    equal = np.zeros(n_cells, bool)
    dt = {"mean": F(10.0), "thresh": F(0.75), "negative": F(-2.0)}[branch]
    if branch == "thresh":
        equal = i % 7 == 1
        g[equal] = dt
    return g, mean_term_sum(g), dt, equal


def counters_case(n_counters, stride, seed=0):
    """int32 [max(n * stride, 1)]: counters up to 2^30 (their sum leaves int32) at the stride, poison between."""
    c = np.full(max(n_counters * stride, 1), COUNTER_POISON, np.int32)
    vals = (uniform(9000 + seed, max(n_counters, 1)) * (1 << 30)).astype(np.int64)
    for k in range(n_counters):
        c[k * stride] = vals[k]
    return c, int(sum(int(vals[k]) for k in range(n_counters)))


# ---------------------------------------------------------------------------- mark_untrained_grid
MARK_H = (2, 4, 8, 32)
MARK_CASCADES = ((1, 1.0), (2, 1.5), (3, 4.0))   # (cascades, bound): min(2^cas, bound) bites in the last two
MARK_B = (0, 1, 3)
MARK_INTRINSICS = {1: (100.0, 100.0, 30.0, 30.0), 3: (120.0, 90.0, 40.0, 20.0), 0: (100.0, 100.0, 30.0, 30.0)}
MARK_MARGIN = 1e-5
MARK_MAX_DIFFERENT = 1e-3


def _pose(eye, look):
    """Row-major 4x4 camera-to-world, fp32: columns right, up, forward (the kernel's z is the third column)."""
    fwd = np.asarray(look, D) / np.linalg.norm(look)
    up0 = np.array([0.13, 0.21, 0.97])
    right = np.cross(up0, fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = right, up, fwd, eye
    return P.astype(F)


def mark_poses(B, bmax):
    """B = 1: a camera inside the volume (cells behind it are unseen).  B = 3: one outside looking in, one outside
    looking away, one inside; intrinsics with cx/fx != cy/fy (MARK_INTRINSICS)."""
    inside = _pose((0.11 * bmax, -0.07 * bmax, 0.05 * bmax), (0.83, 0.41, -0.37))
    if B == 0:
        return np.zeros((0, 4, 4), F)
    if B == 1:
        return inside[None]
    eye = np.array([1.9, 0.6, -0.45]) * bmax
    # (aimed beside the centre: at H = 2 the slack 2 * half is the whole bound and a centred camera sees all 8 cells)
    return np.stack([_pose(eye, np.array([0.0, -1.2, 0.9]) * bmax - eye), _pose(eye, eye),
                     _pose((-0.21 * bmax, 0.17 * bmax, 0.3 * bmax), (0.35, -0.25, 0.9))])


def mark_case(H, cascades, bound, B):
    bmax = min(2.0 ** (cascades - 1), bound)
    return mark_poses(B, bmax), MARK_INTRINSICS[B]


def mark_prefill(H, cascades):
    """Distinct positive values: a seen cell must keep exactly these bits."""
    n = cascades * H ** 3
    return (F(0.25) + np.arange(n, dtype=F) * F(2.0 ** -10)).astype(F)


def _mark(poses, intrinsic, H, cascades, bound, dt, slack=2.0):
    fx, fy, cx, cy = (F(v) for v in intrinsic)
    kx, ky = (cx / fx, cy / fy) if dt is F else (D(cx) / D(fx), D(cy) / D(fy))      # the host forms cx / fx in fp32
    c = coords_of(np.arange(H ** 3)).astype(dt)
    P = np.asarray(poses, F).reshape(-1, 16).astype(dt)
    unseen = np.ones((cascades, H ** 3), bool)
    margin = np.full((cascades, H ** 3), np.inf)
    for cas in range(cascades):
        bnd = min(dt(2.0 ** cas), dt(F(bound)))
        half = bnd / dt(H)
        ext = bnd - half
        w = (dt(2.0) * c / dt(H - 1) - dt(1.0)) * ext
        seen = np.zeros(H ** 3, bool)
        for p in P:
            dx, dy, dz = w[:, 0] - p[3], w[:, 1] - p[7], w[:, 2] - p[11]
            cx_ = dx * p[0] + dy * p[4] + dz * p[8]              # left to right, one rounding per operation
            cy_ = dx * p[1] + dy * p[5] + dz * p[9]
            cz_ = dx * p[2] + dy * p[6] + dz * p[10]
            rx, ry = kx * cz_ + half * dt(slack), ky * cz_ + half * dt(slack)
            seen |= (cz_ > 0) & (np.abs(cx_) < rx) & (np.abs(cy_) < ry)
            if dt is D:
                for lhs, rhs in ((np.abs(cx_), rx), (np.abs(cy_), ry), (cz_, np.zeros_like(cz_))):
                    big = np.maximum(np.abs(lhs), np.abs(rhs))
                    margin[cas] = np.minimum(margin[cas], np.abs(lhs - rhs) / np.where(big > 0, big, 1.0))
        unseen[cas] = ~seen
    return unseen, margin


def mark_unseen32(poses, intrinsic, H, cascades, bound, slack=2.0):
    """bool [C, H^3] in Morton order, True = no camera sees the cell (the kernel writes -1 there)."""
    return _mark(poses, intrinsic, H, cascades, bound, F, slack)[0]


def mark_unseen64(poses, intrinsic, H, cascades, bound):
    """-> unseen bool [C, H^3], margin [C, H^3]: the smallest |lhs - rhs| / max(|lhs|, |rhs|) over the cameras and the
    three inequalities of a cell, in float64."""
    return _mark(poses, intrinsic, H, cascades, bound, D)
