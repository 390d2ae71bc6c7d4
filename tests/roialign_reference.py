"""Float64 reference of 3-D RoIAlign (csrc/roialign.hip) in its separable form, the generators of the test cases of
tests/test_roialign_cpu.py / tests/test_roialign_kernels.py and their tolerance.  numpy only; nothing shared with
instance_nerf_amd or oracle/ (tests/test_roialign_cpu.py compares this file WITH oracle/roialign.py).

Semantics: torchvision's roi_align (aligned=False, adaptive grid ceil(size / out), average pooling) on three axes.
Per RoI and axis a, with n = the volume's extent and o = the output's:
    start = roi[a] * scale; size = max(roi[a + 3] * scale - start, 1); bin = size / o; grid = ceil(size / o)
    sample (p, i) = start + p * bin + (i + 0.5) * bin / grid            p < o, i < grid
all in float32, operation by operation, left to right (roi_geom in roialign.hip).  Everything behind the coordinate is
float64: a sample v with v < -1 or v > n is skipped (and still counted in count = grid_x * grid_y * grid_z); otherwise
c = max(v, 0), lo = int(c), and lo >= n - 1 puts the whole weight on cell n - 1, else 1 - fr on lo and fr = c - lo on
lo + 1.  The summed tap weights of output index p give row p of a table T_a[o, n] and
    out[k, c, p, q, r]  = sum_xyz Tx[p, x] Ty[q, y] Tz[r, z] vol[ind_k, c, x, y, z] / count
    grad[n, c, x, y, z] = sum_{k: ind_k = n} sum_pqr Tx[p, x] Ty[q, y] Tz[r, z] g[k, c, p, q, r] / count.

Two more passes over the same tables feed the tolerance:
    mass: the same sums over |vol| or |g| - what the rounding errors of an element are relative to;
    n:    a table with += 1 per NONZERO tap instead of its weight - the number of nonzero terms the lane-per-output
          formulation (8 taps per sample) adds into the element: Nx[p] Ny[q] Nz[r] for the forward (row sums), the
          same product of per-cell counts summed over RoIs and output elements for the backward.
Bound of the tolerance tier: |got - ref| <= (n + 8) * 2^-24 * mass.  Every one of the n terms is a product of three
weights, a value and 1 / count - a handful of roundings of 2^-24 relative each - and every addition of it into the
running sum rounds once more, relative to a partial sum that |.| bounds by mass; linearly in n that is a few times
n * 2^-24 * mass in the worst case with all errors aligned, and the real alignment is random (sqrt(n)).  The separable
kernels add fewer terms (table entries are pre-summed), so one bound serves both forms.  The + 8 covers the fixed
operations (1 - fr in float32, the division by count, the table pre-sums) of elements with few terms.  It is a count of
roundings, not a measurement; tests print err / bound.

EXACT tier: dyadic geometry (bin in {0.5, 1, 2, 4} - or 0.125 in the thin-box case -, starts multiples of 0.25, scale a
power of two, integer values in [-8, 8]).  Every weight is then a multiple of 1/4 (1/16) per axis, every count a power
of two, every product and partial sum a multiple of 2^-12 below 2^11 - exact in fp32 in any order, fma or not, so
kernels must give the reference's float32 bits.  tests/test_roialign_cpu.py asserts that precondition for every case.
"""
import functools

import numpy as np

F32 = np.float32
EPS = 2.0 ** -24


# ----------------------------------------------------------------------------------------------- the reference proper
def axis_samples(r0, r1, scale, o):
    """-> (coords float64 [o, grid] of float32 values, grid)."""
    start = F32(r0) * F32(scale)
    end = F32(r1) * F32(scale)
    size = np.maximum(end - start, F32(1.0))
    binsz = size / F32(o)
    grid = int(np.ceil(size / F32(o)))
    v = np.empty((o, grid), np.float64)
    for p in range(o):
        for i in range(grid):
            v[p, i] = float(start + F32(p) * binsz + (F32(i) + F32(0.5)) * binsz / F32(grid))
    return v, grid


def axis_table(r0, r1, scale, n, o):
    """-> T float64 [o, n] summed tap weights, cnt int64 [o, n] nonzero taps, inside int64 [o] samples inside, grid."""
    v, grid = axis_samples(r0, r1, scale, o)
    T = np.zeros((o, n), np.float64)
    cnt = np.zeros((o, n), np.int64)
    inside = np.zeros(o, np.int64)
    for p in range(o):
        for x in v[p]:
            if x < -1.0 or x > n:
                continue
            inside[p] += 1
            c = max(x, 0.0)
            lo = int(c)
            if lo >= n - 1:
                T[p, n - 1] += 1.0
                cnt[p, n - 1] += 1
                continue
            fr = c - lo
            T[p, lo] += 1.0 - fr
            cnt[p, lo] += 1                      # 1 - fr > 0 always
            if fr != 0.0:
                T[p, lo + 1] += fr
                cnt[p, lo + 1] += 1
    return T, cnt, inside, grid


@functools.lru_cache(maxsize=8192)
def _roi_tables(roi, shape, osz, scale):
    tabs = [axis_table(roi[a], roi[a + 3], scale, shape[a], osz[a]) for a in range(3)]
    count = max(tabs[0][3] * tabs[1][3] * tabs[2][3], 1)
    return [t[0] for t in tabs], [t[1] for t in tabs], [t[2] for t in tabs], count


def roi_tables(roi, shape, osz, scale):
    """roi [6], shape (W, L, H), osz (ow, ol, oh) -> ([Tx, Ty, Tz], [Nx, Ny, Nz], [inside_x, ..], count)."""
    return _roi_tables(tuple(float(F32(v)) for v in roi), tuple(int(v) for v in shape), tuple(int(v) for v in osz),
                       float(scale))


def forward(vols, scales, rois, inds, levels, osz):
    """vols: list of [N, C, W_l, L_l, H_l]; scales: one per level; levels int [K] (outside the list: a zero row).
    -> dict(out, mass float64 [K, C, ow, ol, oh], n int64 [K, 1, ow, ol, oh])."""
    K, C = len(rois), vols[0].shape[1]
    out = np.zeros((K, C) + tuple(osz), np.float64)
    mass = np.zeros_like(out)
    n = np.zeros((K, 1) + tuple(osz), np.int64)
    for k in range(K):
        lv = int(levels[k])
        if not 0 <= lv < len(vols):
            continue
        vol = np.asarray(vols[lv][int(inds[k])], np.float64)
        T, Nn, _, count = roi_tables(rois[k], vol.shape[1:], osz, scales[lv])
        out[k] = np.einsum("px,qy,rz,cxyz->cpqr", T[0], T[1], T[2], vol, optimize=True) / count
        mass[k] = np.einsum("px,qy,rz,cxyz->cpqr", T[0], T[1], T[2], np.abs(vol), optimize=True) / count
        n[k, 0] = np.einsum("p,q,r->pqr", Nn[0].sum(1), Nn[1].sum(1), Nn[2].sum(1))
    return {"out": out, "mass": mass, "n": n}


def backward(g, shapes, scales, rois, inds, levels):
    """g [K, C, ow, ol, oh]; shapes: one (N, C, W, L, H) per level -> list per level of
    dict(grad, mass float64 [N, C, W, L, H], n int64 [N, 1, W, L, H])."""
    g = np.asarray(g, np.float64)
    osz = g.shape[2:]
    res = [{"grad": np.zeros(s, np.float64), "mass": np.zeros(s, np.float64),
            "n": np.zeros((s[0], 1) + tuple(s[2:]), np.int64)} for s in shapes]
    for k in range(len(rois)):
        lv = int(levels[k])
        if not 0 <= lv < len(shapes):
            continue
        T, Nn, _, count = roi_tables(rois[k], shapes[lv][2:], osz, scales[lv])
        b = int(inds[k])
        res[lv]["grad"][b] += np.einsum("px,qy,rz,cpqr->cxyz", T[0], T[1], T[2], g[k], optimize=True) / count
        res[lv]["mass"][b] += np.einsum("px,qy,rz,cpqr->cxyz", T[0], T[1], T[2], np.abs(g[k]), optimize=True) / count
        res[lv]["n"][b, 0] += np.einsum("x,y,z->xyz", Nn[0].sum(0), Nn[1].sum(0), Nn[2].sum(0))
    return res


def bound(n, mass):
    """The tolerance tier's bound per element (module docstring)."""
    return (n + 8) * EPS * mass


# ------------------------------------------------------------------------------------------------------- the dispatch
def channels_per_block(C, K):
    """sep_channels_per_block of csrc/roialign.hip, restated: 16 channels per workgroup while that leaves 4096 workgroups,
    else 8, else 4."""
    cpb = 16
    while cpb > 4 and K * ((C + cpb - 1) // cpb) < 4096:
        cpb //= 2
    return cpb


def regime(c):
    """What decides the kernels' paths, per RoI of a case, restated from the row windows of sep_build_tables (a row spans
    the lo cell of its first inside sample to the lo + 1 cell of its last, zero weights included): per axis the region
    [lo, hi] of cells any row reaches -> dict of int arrays [K, 3]: `size` (hi - lo + 1, 0 = nothing inside), `row` (the
    longest row in cells), `reach` (the most output indices whose rows hold one cell), `empty_rows`."""
    K = len(c["rois"])
    res = {k: np.zeros((K, 3), np.int64) for k in ("size", "row", "reach", "empty_rows")}
    for k, roi in enumerate(c["rois"]):
        for a in range(3):
            n, o = c["shape"][a], c["osz"][a]
            v, _ = axis_samples(roi[a], roi[a + 3], c["scale"], o)
            cover = np.zeros((o, n), bool)
            for p in range(o):
                ins = v[p][(v[p] >= -1.0) & (v[p] <= n)]
                if len(ins):
                    lo = np.minimum(np.maximum(ins, 0.0).astype(np.int64), n - 1)
                    cover[p, lo.min():min(lo.max() + 1, n - 1) + 1] = True
            cells = np.flatnonzero(cover.any(0))
            res["size"][k, a] = 0 if len(cells) == 0 else cells.max() - cells.min() + 1
            res["row"][k, a] = cover.sum(1).max()
            res["reach"][k, a] = cover.sum(0).max()
            res["empty_rows"][k, a] = (~cover.any(1)).sum()
    return res


CPB_LISTS = {16: [(2048, 18), (2048, 21)], 8: [(1400, 22)], 4: [(7, 1), (7, 3), (7, 5), (7, 37)]}    # (K, C)


# ----------------------------------------------------------------------------------------------------------- the cases
def dyadic_rois(rng, K, shape, osz, scale, bins=(0.5, 1.0, 2.0, 4.0), axis_bins=None):
    """K boxes in image units: per axis bin from `bins` (axis_bins: a tuple of three bin sets, one per axis), start a
    multiple of 0.25 in [-3, max extent), end = start + out * bin, all divided by the (power of two) scale.  Two of every
    three boxes are redrawn until one of their output elements has a sample inside the volume."""
    top = max(shape)
    rois = np.zeros((K, 6), np.float64)
    for k in range(K):
        while True:
            for a in range(3):
                b = float(rng.choice(axis_bins[a] if axis_bins else bins))
                s = float(rng.integers(-12, 4 * top)) / 4.0
                rois[k, a], rois[k, a + 3] = s / scale, (s + osz[a] * b) / scale
            if k % 3 == 2 or box_has_taps(rois[k], shape, osz, scale):
                break
    return rois.astype(F32)


def box_has_taps(roi, shape, osz, scale):
    return all(roi_tables(roi, shape, osz, scale)[2][a].sum() > 0 for a in range(3))


def explicit_rois(rows, scale=1.0):
    """rows of (start_xyz, size_xyz) in level units -> [K, 6] in image units."""
    r = np.asarray([list(s) + [s[a] + e[a] for a in range(3)] for s, e in rows], np.float64) / scale
    return r.astype(F32)


def int_values(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(F32)


def make_case(name, seed, N, C, shape, osz, scale, rois, inds=None, tier="exact", sep_fwd=True, sep_bwd=True):
    """The single-volume case record.  sep_fwd / sep_bwd: whether the forced separable mode must accept the call (True)
    or refuse it with an error return (False)."""
    rng = np.random.default_rng(seed)
    K = len(rois)
    if inds is None:
        inds = rng.integers(0, N, K)
    draw = int_values if tier == "exact" else (lambda r, s: r.normal(size=s).astype(F32))
    return {"name": name, "N": N, "C": C, "shape": tuple(shape), "osz": tuple(osz), "scale": float(scale),
            "rois": np.ascontiguousarray(rois, F32), "inds": np.asarray(inds, np.int32), "tier": tier,
            "vol": draw(rng, (N, C) + tuple(shape)), "g": draw(rng, (K, C) + tuple(osz)),
            "sep_fwd": sep_fwd, "sep_bwd": sep_bwd}


def case_forward(c):
    return forward([c["vol"]], [c["scale"]], c["rois"], c["inds"], np.zeros(len(c["rois"]), int), c["osz"])


def case_backward(c):
    return backward(c["g"], [(c["N"], c["C"]) + c["shape"]], [c["scale"]], c["rois"], c["inds"],
                    np.zeros(len(c["rois"]), int))[0]


# -- boundary rules: one axis at a time, bin = 1, grid = 1
BOUNDARY_SHAPE = (5, 6, 7)
#            sample at (n = the axis' extent), expected: cell index (negative: from the end) or None = skipped
BOUNDARY_SAMPLES = (("-1.25", lambda n: -1.25, None), ("-1", lambda n: -1.0, 0), ("-0.5", lambda n: -0.5, 0),
                    ("0", lambda n: 0.0, 0), ("n-1", lambda n: n - 1.0, -1), ("n-0.5", lambda n: n - 0.5, -1),
                    ("n", lambda n: float(n), -1), ("n+0.25", lambda n: n + 0.25, None),
                    ("reversed@0", lambda n: 0.0, 0), ("thin@n-1", lambda n: n - 1.0, -1))


def boundary_case(axis):
    """Ten boxes; on `axis` the output has one bin of size 1 whose single sample lies at BOUNDARY_SAMPLES[k]; on the other
    two axes the box is [-0.5, n - 0.5) with n bins: samples on the cell centres, the identity.  So row k is the slab
    vol[.., cell, ..] of the expected cell, or zero.  Box 8 has end < start and box 9 is 0.25 thick: size clamped to 1."""
    shape = BOUNDARY_SHAPE
    osz = tuple(1 if a == axis else shape[a] for a in range(3))
    rois = np.zeros((len(BOUNDARY_SAMPLES), 6), np.float64)
    for k, (name, at, _) in enumerate(BOUNDARY_SAMPLES):
        for a in range(3):
            rois[k, a], rois[k, a + 3] = -0.5, shape[a] - 0.5
        s = at(shape[axis]) - 0.5
        rois[k, axis] = s
        rois[k, axis + 3] = s - 3.0 if name.startswith("reversed") else (s + 0.25 if name.startswith("thin") else s + 1.0)
    return make_case(f"boundary/axis{axis}", 100 + axis, 2, 3, shape, osz, 1.0, rois,
                     inds=[k % 2 for k in range(len(rois))])


def boundary_expected(c, axis):
    """The literal expectation, written from the volume: no table involved."""
    want = np.zeros((len(c["rois"]), c["C"]) + c["osz"], F32)
    for k, (_, _, cell) in enumerate(BOUNDARY_SAMPLES):
        if cell is not None:
            want[k] = np.take(c["vol"][c["inds"][k]], [cell % c["shape"][axis]], axis=1 + axis)
    return want


def ones_case():
    """A volume of ones: out = inside samples / count.  Boxes with grids 2 and 4 hanging over a face by 0..4 samples."""
    shape, osz = (5, 6, 7), (2, 1, 3)
    rows = []
    for k in range(12):
        b = (2.0, 4.0, 2.0) if k % 2 else (4.0, 2.0, 4.0)
        s = (-3.0 + 0.25 * k, -2.75 + 0.5 * k, 4.0 + 0.25 * k) if k < 6 else (2.0 + 0.25 * k, -6.0 + 0.75 * k, -4.25 + 0.5 * k)
        rows.append((s, tuple(osz[a] * b[a] for a in range(3))))
    c = make_case("ones", 7, 1, 2, shape, osz, 1.0, explicit_rois(rows), inds=[0] * 12)
    c["vol"] = np.ones_like(c["vol"])
    return c


def ones_expected(c):
    """Samples counted directly (float32 coordinates, the inside test alone) over count."""
    want = np.zeros((len(c["rois"]), c["C"]) + c["osz"], np.float64)
    for k, roi in enumerate(c["rois"]):
        ins, count = [], 1
        for a in range(3):
            v, grid = axis_samples(roi[a], roi[a + 3], c["scale"], c["osz"][a])
            ins.append(((v >= -1.0) & (v <= c["shape"][a])).sum(1))
            count *= grid
        want[k] = np.einsum("p,q,r->pqr", *ins)[None] / count
    return want


def ceil_case():
    """Tolerance tier: boxes whose scaled size is a whole multiple of the output within float32 rounding, so that
    ceil(size / out) differs between float32 and float64.  The reference takes the float32 decision."""
    shape, osz, scale = (9, 8, 7), (3, 2, 3), 0.7
    found = []
    for i in range(4000):
        x1 = F32(0.013 * i)
        for g in (1, 2):
            x2 = F32((float(x1) * 0.7 + g * 3 + 1e-7) / 0.7)
            s32 = np.maximum(x2 * F32(scale) - x1 * F32(scale), F32(1.0))
            g32 = int(np.ceil(s32 / F32(3)))
            g64 = int(np.ceil(max(float(x2) * scale - float(x1) * scale, 1.0) / 3.0))
            if g32 != g64 and float(x1) * 0.7 < 6:
                found.append((float(x1), float(x2)))
        if len(found) >= 6:
            break
    rois = np.asarray([[x1, 0.5 + 0.3 * j, x1, x2, 7.1 + 0.2 * j, x2] for j, (x1, x2) in enumerate(found)], F32)
    return make_case("tol/ceil", 9, 1, 3, shape, osz, scale, rois, tier="tol"), len(found)


# -- extents 1..5
EXTENT_SHAPES = ((1, 1, 1), (3, 1, 2), (5, 4, 1), (2, 5, 4), (1, 3, 5), (4, 2, 3))


def extent_case(i):
    shape = EXTENT_SHAPES[i]
    osz = ((2, 3, 2), (3, 1, 4), (1, 2, 5), (4, 3, 2), (2, 2, 2), (3, 3, 3))[i]
    scale = (1.0, 0.5, 0.25, 1.0, 0.5, 1.0)[i]
    rng = np.random.default_rng(200 + i)
    rois = dyadic_rois(rng, 9, shape, osz, scale)
    return make_case(f"extent/{shape}", 210 + i, 2, 5, shape, osz, scale, rois, sep_fwd=shape[2] >= 4)


# -- forward dispatch edges
def dispatch_cases():
    out = {}
    rng = np.random.default_rng(300)
    for osz, sep_f, sep_b in (((8, 8, 16), True, True), ((11, 10, 10), True, True), ((16, 16, 16), True, False),
                              ((17, 16, 16), False, False), ((1, 17, 16), False, True)):
        shape = (6, 5, 7)
        rois = np.concatenate([dyadic_rois(rng, 4, shape, osz, 0.5, bins=(0.5, 1.0)),
                               explicit_rois([((-0.5, 0.25, -1.0), tuple(0.5 * o for o in osz))], 0.5)])
        out[f"nout{osz}"] = make_case(f"dispatch/nout{osz}", 301, 2, 3, shape, osz, 0.5, rois, sep_fwd=sep_f, sep_bwd=sep_b)
    # the LDS window (sep_lds_bytes: 64 KB = 65 536 bytes).  H = 2000 at out_h = 8: the forward's tables are 16 002 floats
    # + 20 ints + the RoI record + the smallest slabs = 64 432 bytes - the separable forward still takes it, with 1 104
    # bytes to spare; the backward's per-cell ranges (2 * 2002 ints more) do not fit.  H = 2048: 8 * 2048 floats alone
    # are the whole window - both fall back.
    for H, sep_f in ((2000, True), (2048, False)):
        out[f"window/H{H}"] = make_case(f"dispatch/window/H{H}", 302, 1, 1, (1, 1, H), (1, 1, 8), 1.0,
                                        explicit_rois([((-0.5, -0.5, 3.0), (1, 1, 32)), ((0, 0, H - 9.75), (1, 1, 16)),
                                                       ((-0.5, -0.5, -2.0), (1, 1, 8)),
                                                       ((0.5, -0.5, H - 8.5), (1, 1, 16))]),      # samples on x == W, z == H
                                        sep_fwd=sep_f, sep_bwd=False)
    # three x slabs: 12^3, output (4, 16, 16): XB = (10240 - 16) / (4 * (12 * 16 + 256)) = 5
    rois = np.concatenate([explicit_rois([((-1.0, -1.0, -1.0), (16, 16, 16)), ((0.25, -2.0, 1.5), (16, 16, 8)),
                                          ((-3.0, 2.0, 0.0), (8, 8, 16)), ((5.0, 5.0, 5.0), (2, 8, 8))]),
                           dyadic_rois(rng, 3, (12, 12, 12), (4, 16, 16), 1.0)])
    out["slabs"] = make_case("dispatch/slabs", 303, 1, 5, (12, 12, 12), (4, 16, 16), 1.0, rois)
    # rows longer than the four register taps (grid 4: five cells), one axis at a time
    for a, nm in enumerate(("morex", "morey", "morez")):
        ab = tuple((4.0,) if b == a else (0.5, 1.0) for b in range(3))
        rois = dyadic_rois(rng, 6, (12, 12, 12), (3, 3, 3), 1.0, axis_bins=ab)
        out[nm] = make_case(f"dispatch/{nm}", 304 + a, 2, 3, (12, 12, 12), (3, 3, 3), 1.0, rois)
    rois = dyadic_rois(rng, 5, (12, 12, 12), (11, 10, 10), 1.0, axis_bins=((4.0,), (0.5, 1.0), (0.5, 1.0)))
    out["morex_multi"] = make_case("dispatch/morex_multi", 308, 1, 2, (12, 12, 12), (11, 10, 10), 1.0, rois)
    # regions one to three cells deep along z (the four-cell window leaves them), at both faces and inside; H == 4
    for H in (8, 4):
        rows = []
        for z, dz in ((-0.5, 1), (0.0, 1), (2.0, 1), (1.25, 2), (H - 1.0, 1), (H - 2.0, 1), (H - 2.75, 2), (H - 0.5, 1),
                      (-1.25, 1), (0.75, 1)):
            rows.append(((0.25, -0.5, z), (3, 6, dz)))
        out[f"tiny_z/H{H}"] = make_case(f"dispatch/tiny_z/H{H}", 310 + H, 1, 6, (5, 6, H), (3, 3, 2), 1.0, explicit_rois(rows))
    # half outside: leading / trailing output indices without taps on every axis
    rows = [((-4.0, -5.0, -6.0), (8, 8, 8)), ((5.0, 4.0, 3.0), (8, 8, 8)), ((-9.0, 2.0, 5.0), (16, 4, 8)),
            ((-3.0, 6.0, -7.0), (4, 16, 16)), ((-2.0, -2.0, 6.5), (4, 4, 4)), ((8.0, -3.0, -3.0), (4, 4, 4))]
    out["half_outside"] = make_case("dispatch/half_outside", 320, 1, 4, (7, 8, 9), (4, 4, 4), 1.0, explicit_rois(rows))
    return out


# -- channel runs
def channel_case(K, C):
    rng = np.random.default_rng(400 + K + C)
    shape, osz = (4, 4, 4), (1, 1, 2)
    base = dyadic_rois(rng, min(K, 24), shape, osz, 0.5)
    rois = base[rng.integers(0, len(base), K)]                  # duplicates: atomics accumulate
    rois[:len(base)] = base
    inds = rng.choice([0, 2], K)                                # the last volume is reached, volume 1 is named by no RoI
    inds[0], inds[-1] = 2, 0
    c = make_case(f"channels/K{K}/C{C}", 401, 3, C, shape, osz, 0.5, rois, inds=inds)
    if K > 100:                                                 # 2048 boxes into 64 cells: keep the sums below 2^11
        c["g"] = np.random.default_rng(402).integers(-2, 3, size=c["g"].shape).astype(F32)
    return c


# -- backward forms
def backward_cases(tier):
    rng = np.random.default_rng(500 if tier == "exact" else 501)
    out = {}

    def boxes(K, shape, osz, scale, extra=()):
        if tier == "exact":
            r = dyadic_rois(rng, K, shape, osz, scale)
        else:
            r = tol_rois(rng, K, shape, scale)
        return np.concatenate([r] + [explicit_rois([e], scale) for e in extra]) if extra else r

    # generic roles (sy * oh > 256) next to small regions
    out["generic_syoh"] = make_case(f"bwd/{tier}/generic_syoh", 510, 2, 5, (4, 30, 6), (2, 12, 12), 1.0,
                                    boxes(5, (4, 30, 6), (2, 12, 12), 1.0, extra=[((-1.0, -3.0, -1.0), (4, 48, 12)),
                                                                                  ((0.5, 2.0, 1.0), (2, 6, 6))]), tier=tier)
    # generic roles (ol * oh > 256): the forward falls back
    out["generic_olh"] = make_case(f"bwd/{tier}/generic_olh", 511, 1, 3, (5, 6, 7), (2, 17, 16), 0.5,
                                   boxes(5, (5, 6, 7), (2, 17, 16), 0.5), tier=tier, sep_fwd=False)
    out["nout1024"] = make_case(f"bwd/{tier}/nout1024", 512, 2, 6, (6, 5, 7), (8, 8, 16), 0.5,
                                boxes(6, (6, 5, 7), (8, 8, 16), 0.5), tier=tier)
    out["nout1100"] = make_case(f"bwd/{tier}/nout1100", 513, 2, 6, (6, 5, 7), (11, 10, 10), 0.5,
                                boxes(6, (6, 5, 7), (11, 10, 10), 0.5), tier=tier)
    # boxes one cell thick under 8 bins: a cell is reached by more than four output indices (moreB, moreC)
    thin = [((1.0 + 0.5 * k, 0.5 * k, 4.0 - 0.5 * k), ((8, 1, 1), (4, 1, 8), (8, 8, 1), (1, 1, 1))[k % 4]) for k in range(8)]
    out["thin"] = make_case(f"bwd/{tier}/thin", 514, 2, 5, (7, 6, 8), (8, 8, 8), 1.0, explicit_rois(thin), tier=tier)
    return out


def workspace_cases(tier):
    rng = np.random.default_rng(600 if tier == "exact" else 601)
    out = {}
    for C in (16, 48):
        shape, osz = (5, 3, 7), (3, 2, 4)
        r = dyadic_rois(rng, 7, shape, osz, 0.5) if tier == "exact" else tol_rois(rng, 7, shape, 0.5)
        out[f"C{C}"] = make_case(f"ws/{tier}/C{C}", 610 + C, 2, C, shape, osz, 0.5, r, tier=tier)
    shape, osz = (4, 30, 6), (2, 12, 12)                       # sy * oh = 360 > 256: several y roles per thread
    r = dyadic_rois(rng, 4, shape, osz, 1.0) if tier == "exact" else tol_rois(rng, 4, shape, 1.0)
    r = np.concatenate([r, explicit_rois([((-1.0, -3.0, -1.0), (4, 48, 12))])])
    out["oneB_off"] = make_case(f"ws/{tier}/oneB_off", 620, 2, 16, shape, osz, 1.0, r, tier=tier)
    return out


# -- tolerance tier
def tol_rois(rng, K, shape, scale):
    """Uniform starts in [-3, max extent), extents from thinner than a voxel to 3 x the volume (every third box), else
    0.3 .. 6 cells; the last box outside."""
    top = max(shape)
    lo = rng.uniform(-3, top, size=(K, 3))
    ext = np.stack([rng.uniform(0.05, 3.0 * top, 3) if k % 3 == 0 else rng.uniform(0.3, 6, 3) for k in range(K)])
    for k in range(0, K, 2):                                   # half of the boxes start inside the lower corner region
        lo[k] = rng.uniform(-2, np.asarray(shape) / 2.0)
    rois = np.concatenate([lo, lo + ext], 1) / scale
    rois[-1] = np.asarray([500, 500, 500, 520, 510, 530])
    return rois.astype(F32)


def tol_cases():
    rng = np.random.default_rng(700)
    out = {}
    for i, (N, C, shape, osz) in enumerate(((2, 5, (9, 8, 7), (3, 4, 5)), (1, 3, (7, 7, 7), (7, 7, 7)),
                                            (2, 2, (6, 11, 5), (11, 10, 10)), (1, 7, (3, 2, 9), (2, 2, 2)))):
        out[f"t{i}"] = make_case(f"tol/t{i}", 710 + i, N, C, shape, osz, 0.7, tol_rois(rng, 8, shape, 0.7), tier="tol")
    return out


# -- pyramid
def pyramid_case():
    """Three levels (scales 1, 0.5, 0.25; one with H = 2), boxes per image in image units, one box naming level 3."""
    rng = np.random.default_rng(800)
    shapes = [(2, 4, 9, 10, 8), (2, 4, 5, 6, 4), (2, 4, 3, 4, 2)]
    scales = [1.0, 0.5, 0.25]
    osz = (3, 2, 4)
    levels = np.asarray([0, 1, 2, 2, 1, 0, 3, 2, 1, 0, 2, 1], np.int64)
    inds = np.asarray([0] * 7 + [1] * 5, np.int32)
    rois = np.zeros((len(levels), 6), F32)
    for k, lv in enumerate(levels):
        l = min(int(lv), 2)
        rois[k] = dyadic_rois(rng, 1, shapes[l][2:], osz, scales[l])[0]
    vols = [int_values(rng, s) for s in shapes]
    g = int_values(rng, (len(levels), 4) + osz)
    return {"name": "pyramid", "shapes": shapes, "scales": scales, "osz": osz, "levels": levels, "inds": inds, "rois": rois,
            "vols": vols, "g": g, "counts": [7, 5]}


ONE_HOT_CELLS = {"far_x": (4, 2, 3), "far_y": (1, 5, 2), "far_z": (2, 3, 6), "corner": (4, 5, 6), "origin": (0, 0, 0)}
ONE_HOT_OUTPUTS = {"far_x": (2, 0, 1), "far_y": (1, 1, 2), "far_z": (0, 0, 3), "corner": (2, 1, 3), "origin": (0, 0, 0)}


def one_hot_base():
    """(5, 6, 7) volume, output (3, 2, 4): box 0 is the whole volume, the others drawn.  The one-hot tests replace the
    volume (a single 1 at ONE_HOT_CELLS, in both volumes and every channel) or grad_out (a single 1 per channel at
    ONE_HOT_OUTPUTS, in every box)."""
    rng = np.random.default_rng(900)
    shape, osz = (5, 6, 7), (3, 2, 4)
    rois = np.concatenate([explicit_rois([((-0.5, -1.0, -0.5), (6, 8, 8))], 0.5), dyadic_rois(rng, 6, shape, osz, 0.5)])
    return make_case("one_hot", 901, 2, 3, shape, osz, 0.5, rois, inds=[0, 1, 0, 1, 1, 0, 0])


def one_hot_case(where, side):
    c = dict(one_hot_base())
    if side == "vol":
        c["vol"] = np.zeros_like(c["vol"])
        c["vol"][(slice(None), slice(None)) + ONE_HOT_CELLS[where]] = 1.0
    else:
        c["g"] = np.zeros_like(c["g"])
        c["g"][(slice(None), slice(None)) + ONE_HOT_OUTPUTS[where]] = 1.0
    c["name"] = f"one_hot/{side}/{where}"
    return c


def exact_cases():
    """name -> case for every single-volume exact-tier case of the GPU tests."""
    out = {"one_hot": one_hot_base()}
    for a in range(3):
        out[f"boundary{a}"] = boundary_case(a)
    out["ones"] = ones_case()
    for i in range(len(EXTENT_SHAPES)):
        out[f"extent{i}"] = extent_case(i)
    out.update({f"dispatch/{k}": v for k, v in dispatch_cases().items()})
    for cpb, lst in CPB_LISTS.items():
        for K, C in lst:
            out[f"channels/{K}/{C}"] = channel_case(K, C)
    out.update({f"bwd/{k}": v for k, v in backward_cases("exact").items()})
    out.update({f"ws/{k}": v for k, v in workspace_cases("exact").items()})
    return out


def separable_fits(shape, osz, bwd):
    """The host's decision between the separable kernels and the lane pair (inr_roi_align_3d_forward / _backward with
    sep_lds_bytes of csrc/roialign.hip), restated for shapes far from the index limits: what mode 2 accepts."""
    (W, L, H), (ow, ol, oh) = shape, osz
    nout = ow * ol * oh
    if not bwd and (nout > 16 * 256 or ol * oh > 256 or H < 4):
        return False
    fixed = (ow * W + ol * L + oh * H + 2 * (ow + ol + oh) + (2 * (W + L + H) if bwd else 0)) * 4 + 64 + 16
    need = 4 * (L * oh + ol * oh) + (4 * nout if bwd else 4 * ow)          # one x plane of the widest region (+ grad_out)
    return fixed + need * 4 <= 64 * 1024
