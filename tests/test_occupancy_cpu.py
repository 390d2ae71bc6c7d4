"""tests/occupancy_reference.py is right and its cases meet the conditions tests/test_occupancy_kernels.py relies on:
the fp32 restatements against their float64 forms (within the derived bounds) and against oracle/occupancy.py wherever
the oracle defines the case, the ambiguity caps of the mark_untrained cases, the distance of every packbits_mean grid
from its threshold, and what the listed update owes upstream's -1 fill - all on the CPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_reference as R  # noqa: E402

F, D = np.float32, np.float64


# ---------------------------------------------------------------------------- Morton, packbits
def test_morton_against_the_oracle():
    from oracle import occupancy
    codes = np.concatenate([np.arange(4096), (R.uniform(1, 500) * 2 ** 30).astype(np.int64)])
    c = R.coords_of(codes)
    assert np.array_equal(c, occupancy.morton3D_invert(codes))
    assert np.array_equal(R.morton3(c[:, 0], c[:, 1], c[:, 2]), codes)
    assert np.array_equal(occupancy.morton3D(c).astype(np.int64), codes)
    assert R.morton3(1023, 1023, 1023) == 2 ** 30 - 1 and R.morton3(127, 127, 127) == 128 ** 3 - 1


@pytest.mark.parametrize("kind", R.PACK_KINDS)
@pytest.mark.parametrize("n_bytes", R.PACK_BYTES)
def test_packbits_restatements_agree(n_bytes, kind):
    from oracle import occupancy
    g, t = R.packbits_case(n_bytes, kind)
    b32 = R.packbits32(g, t, n_bytes)
    assert np.array_equal(b32, R.packbits64(g, t, n_bytes))
    assert np.array_equal(b32, occupancy.packbits(g[:8 * n_bytes], t))
    cells = g[:8 * n_bytes]
    bit = (b32[:, None] >> np.arange(8)) & 1
    assert not bit.reshape(-1)[cells == t].any(), "a cell equal to the threshold is not above it"
    assert (cells == t).any() and (cells > t).any() and (cells < t).any()
    if kind == "t0" and n_bytes > 1:
        flat = bit.reshape(-1)
        assert not flat[np.isnan(cells)].any() and flat[np.isposinf(cells)].all() and not flat[np.isneginf(cells)].any()
        assert np.signbit(cells[cells == 0]).any() and not np.signbit(cells[cells == 0]).all()


# ---------------------------------------------------------------------------- positions
@pytest.mark.parametrize("n", R.POS_N)
def test_positions_fp32_against_float64_and_the_oracle(n):
    from oracle import occupancy
    seen = set()
    for H, bound, listed, kind in R.position_cases(n):
        codes = R.position_codes(n, H, listed)
        noise = R.position_noise(kind, n, seed=n + H)
        cc = np.arange(n) if codes is None else codes
        p32, p64 = R.positions32(cc, noise, H, bound), R.positions64(cc, noise, H, bound)
        e = float(np.abs(p32.astype(D) - p64).max())
        allowed = R.POS_ROUNDINGS * R.U * bound * R.POS_SLACK
        assert e <= allowed, (H, bound, listed, kind, e, allowed)
        assert np.abs(p64).max() <= bound
        # the oracle takes the jitter 2u - 1 already formed, and the cascade level with the bound: b = min(2^cas, bound)
        jit = None if noise is None else noise * F(2.0) - F(1.0)
        o = occupancy.cell_centers(R.coords_of(cc), H, 3, bound, jit)
        assert np.array_equal(o.view(np.uint32), p32.view(np.uint32)), (H, bound, listed, kind)
        if listed:
            c = R.coords_of(codes)
            assert (c[0] == H - 1).all() and (n == 1 or (c[1] == 0).all()) and c.max() <= H - 1
        seen.add((H, listed))
        seen.add(bound)
        seen.add(kind)
    assert all((H, True) in seen for H in R.POS_H) and all(k in seen for k in R.POS_NOISE)
    assert sum(b in seen for b in R.POS_BOUNDS) == 4


# ---------------------------------------------------------------------------- the update
def test_fmax32_is_maximum_number():
    a = np.array([0.0, -0.0, -0.0, 0.0, np.nan, 1.0, np.nan, np.inf, -1.0], F)
    b = np.array([-0.0, 0.0, -0.0, 0.0, 2.0, np.nan, np.nan, 3.0, -2.0], F)
    want = np.array([0.0, 0.0, -0.0, 0.0, 2.0, 1.0, np.nan, np.inf, -1.0], F)
    assert np.array_equal(R.fmax32(a, b).view(np.uint32), want.view(np.uint32))


def _full_cases():
    for n in R.UPDATE_SIZES:
        for k, (decay, scale, with_inf, start) in enumerate(R.update_combos()):
            yield n, k, decay, scale, with_inf


def test_update_fp32_against_float64_and_the_oracle():
    from oracle import occupancy
    kinds = set()
    for n, k, decay, scale, with_inf in _full_cases():
        g, s = R.update_grid(n, 10 * n + k, with_inf), R.update_sigma(n, 10 * n + k, with_inf)
        new32, new64 = R.update_full32(g, s, decay, scale), R.update_cells64(g, s, decay, scale)
        same_class = (np.isnan(new32) == np.isnan(new64)) & (np.isinf(new32) == np.isinf(new64))
        assert same_class.all()
        fin = np.isfinite(new64)
        assert (np.abs(new32[fin].astype(D) - new64[fin]) <= R.U * np.abs(new64[fin])).all(), (n, decay, scale)
        with np.errstate(invalid="ignore"):
            stays = ~((g >= 0) & (s * F(scale) >= 0))
            gd = g * F(decay)
        assert np.array_equal(new32.view(np.uint32)[stays], g.view(np.uint32)[stays])
        for v in g[stays]:
            kinds.add("nan" if np.isnan(v) else "-1" if v == -1 else "other")
        # the oracle's update line on these cells (np.maximum keeps a NaN and leaves the sign of max(+0, -0) open: those
        # cells are left out); its whole function runs on 2^3 cells below
        o = np.array(g, copy=True)
        with np.errstate(invalid="ignore"):
            tmp = s * F(scale)
            both_zero = (gd == 0) & (tmp == 0)
            valid = (g >= 0) & (tmp >= 0)
            o[valid] = np.maximum(g[valid] * F(decay), tmp[valid])
        cmp = ~both_zero & ~np.isnan(o)
        assert np.array_equal(o.view(np.uint32)[cmp], new32.view(np.uint32)[cmp])
    assert kinds >= {"nan", "-1"}
    # the oracle's own function on one cascade of 2^3 cells: sigma_fn hands back the list in coordinate order
    g, s = R.update_grid(8, 77, False), np.abs(R.update_sigma(8, 77, False))
    s[np.isnan(s)] = F(0.3)
    order = occupancy.morton3D(np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3)).astype(int)
    og, obits, omean = occupancy.update_density_grid(g[None], lambda xyz: s[order], 2, 1, 1.0, decay=0.95,
                                                     density_scale=0.7, density_thresh=0.4)
    new32 = R.update_full32(g, s, 0.95, 0.7)
    keep = ~np.isnan(new32)
    assert np.array_equal(og[0].view(np.uint32)[keep], new32.view(np.uint32)[keep])


def test_mean_sum_terms():
    g = np.array([-1.0, np.nan, 0.5, -0.0, 2.0], F)
    assert R.mean_term_sum(g) == 2.5 and R.mean_term_sum(np.array([1.0, np.inf], F)) == np.inf
    assert R.mean_sum_tolerance(1024, 100.0) == 1024 * 2.0 ** -52 * 100.0


@pytest.mark.parametrize("m_kind", R.LISTED_M)
def test_listed_update_is_upstreams_rule(m_kind):
    """The 0xBF fill against upstream's -1 fill (oracle/occupancy.py::update_density_grid: tmp = -1, valid = grid >= 0 &
    tmp >= 0): with unique indices the two give the same grid bit for bit; an unvisited cell does not decay."""
    assert R.UNVISITED < 0 and R.UNVISITED.view(np.uint32) == 0xBFBFBFBF
    for n in R.UPDATE_SIZES:
        idx = R.listed_indices(n, m_kind, n)
        m = len(idx)
        g, s = R.update_grid(n, n, True), R.update_sigma(max(m, 1), n, True)
        cand, visited = R.update_listed32(g, s, idx, 0.95, 0.7)
        assert visited.sum() <= m and (m == 0 or visited.any())
        # upstream, last writer wins (NumPy's index_put order) - one of the allowed outcomes
        tmp = np.full(n, -1.0, F)
        with np.errstate(invalid="ignore", over="ignore"):
            tmp[idx] = s[:m] * F(0.7)
            up = R.update_cells32(g, tmp, 0.95, 1.0)
        assert R.listed_outcome_ok(up, g, cand, idx, visited).all()
        assert np.array_equal(up.view(np.uint32)[~visited], g.view(np.uint32)[~visited])
        wrong = np.array(up, copy=True)
        if (~visited & (g > 0) & np.isfinite(g)).any():                           # a decayed unvisited cell is caught
            j = int(np.flatnonzero(~visited & (g > 0) & np.isfinite(g))[0])
            wrong[j] = g[j] * F(0.95)
            assert not R.listed_outcome_ok(wrong, g, cand, idx, visited)[j]
    if m_kind == "double":
        idx = R.listed_indices(1024, m_kind, 1024)
        assert (np.bincount(idx, minlength=1024) >= 2).sum() > 300, "few duplicate cells"


def test_size_above_the_cap():
    k = R.workgroup_cap_factor()
    assert k >= 1
    for cus in (64, 256, 304):
        n = R.size_above_cap(cus)
        assert (n + 1023) // 1024 > k * cus and n % 4 == 3 and n * 4 < 8 << 20      # a few MB at the most


# ---------------------------------------------------------------------------- packbits with the mean
@pytest.mark.parametrize("branch", R.MEAN_BRANCHES)
@pytest.mark.parametrize("n_cells", R.MEAN_CELLS)
def test_packbits_mean_cases(n_cells, branch):
    g, mean_sum, dt, equal = R.packbits_mean_case(n_cells, branch)
    bits, mean, thresh = R.packbits_mean32(g, n_cells, mean_sum, dt)
    bits64, thresh64 = R.packbits_mean64(g, n_cells, mean_sum, dt)
    assert (thresh == mean) == (branch == "mean") and (thresh == dt) == (branch != "mean")
    assert abs(float(mean) - mean_sum / n_cells) <= R.ulp32(mean)
    # no cell within two fp32 ulps of the threshold but the deliberate ones: then bit equality is owed
    near = np.abs(g.astype(D) - float(thresh)) <= 2 * R.ulp32(thresh)
    assert np.array_equal(near, equal), (n_cells, branch, int(near.sum()))
    assert abs(thresh64 - float(thresh)) <= R.ulp32(thresh)
    assert np.array_equal(bits, bits64)
    flat = ((bits[:, None] >> np.arange(8)) & 1).reshape(-1).astype(bool)
    assert not flat[equal].any() and flat.any()
    assert flat[g == -1].all() == (branch == "negative") and (g == -1).any()
    assert n_cells % 8 == 0 and (R.MEAN_CELLS[2] // 8) % 256 == 37, "the third size is off a workgroup multiple"
    if branch == "thresh":
        assert equal.any()


def test_counters_case():
    for n, stride in R.COUNTER_SHAPES:
        c, total = R.counters_case(n, stride, seed=n)
        assert total == int(c.astype(np.int64)[::stride][:n].sum()) if n else total == 0
        if stride == 2 and n:
            assert (c[1::2] == R.COUNTER_POISON).all()
    assert R.counters_case(16, 1, 16)[1] > 2 ** 31, "the sum is meant to leave int32"


# ---------------------------------------------------------------------------- mark_untrained_grid
MARK = [(H, c, b, B) for H in R.MARK_H for c, b in R.MARK_CASCADES for B in R.MARK_B]


@pytest.mark.parametrize("H,cascades,bound,B", MARK, ids=[f"H{h}-C{c}-b{b}-B{B}" for h, c, b, B in MARK])
def test_mark_untrained_cases(H, cascades, bound, B):
    from oracle import occupancy
    poses, intr = R.mark_case(H, cascades, bound, B)
    u32 = R.mark_unseen32(poses, intr, H, cascades, bound)
    u64, margin = R.mark_unseen64(poses, intr, H, cascades, bound)
    if B == 0:
        assert u32.all() and u64.all()
        return
    assert u32.any() and not u32.all(), "a case needs a seen and an unseen cell"
    diff = u32 != u64
    assert diff.mean() <= R.MARK_MAX_DIFFERENT, diff.mean()
    assert (margin[diff] < R.MARK_MARGIN).all()
    # the oracle (a matrix product in numpy's order): the same verdict wherever the float64 margin is not tiny
    o = occupancy.mark_untrained_cells(poses, intr, H, cascades, bound)
    clear = margin >= R.MARK_MARGIN
    assert np.array_equal(o[clear], u32[clear])
    # the cases see the slack 2 * half, and a transposed rotation (the cameras are not axis-aligned)
    assert (R.mark_unseen32(poses, intr, H, cascades, bound, slack=1.0) != u32).any() or H == 2
    swapped = poses.copy()
    swapped[:, 0, 1], swapped[:, 1, 0] = poses[:, 1, 0], poses[:, 0, 1]
    assert (R.mark_unseen32(swapped, intr, H, cascades, bound) != u32).any() or (H == 2 and B == 1)
    fx, fy, cx, cy = intr
    assert (cx / fx != cy / fy) == (B == 3)


def test_mark_slack_is_seen_somewhere_at_every_H():
    for H in R.MARK_H:
        hit = False
        for c, b in R.MARK_CASCADES:
            for B in (1, 3):
                poses, intr = R.mark_case(H, c, b, B)
                hit |= bool((R.mark_unseen32(poses, intr, H, c, b, slack=1.0) != R.mark_unseen32(poses, intr, H, c, b)).any())
        assert hit, H


def test_mark_prefill_is_distinct_and_positive():
    g = R.mark_prefill(32, 3)
    assert (g > 0).all() and len(np.unique(g.view(np.uint32))) == len(g)
