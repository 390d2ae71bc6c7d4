"""The occupancy-grid kernels of csrc/raymarch.hip on the GPU against tests/occupancy_reference.py, through the raw C
ABI on plain device tensors (no network, no renderer): inr_packbits, inr_packbits_mean, inr_occ_cell_positions,
inr_occ_update (full sweep and listed) and inr_mark_untrained_grid.

Everything is compared bit for bit with the fp32 restatements (the file is built with -ffp-contract=off and these
kernels use + - * / and comparisons only); the one sum, mean_sum, against the exactly rounded float64 sum within the
derived n_cells * 2^-52.  Float buffers a kernel writes sit inside a larger allocation between NaN-pattern guard words
(Buf of kernel_harness.py); byte outputs are longer than the call's n_bytes and filled with a sentinel byte.

What each seeded fault is caught by is listed with the tests below ("catches: ...")."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_reference as R  # noqa: E402
import train_kernels_reference as tk  # noqa: E402
from kernel_harness import Buf, check, cu_count, stream  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f = np.float32


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


def _bytes_out(n):
    """A sentinel-filled byte buffer with 64 bytes more than the call may write."""
    return torch.full((n + 64,), R.PACK_SENTINEL, dtype=torch.uint8, device=DEV)


def _check_bytes(out, want, what):
    got = out.cpu().numpy()
    n = len(want)
    assert np.array_equal(got[:n], want), f"{what}: {int((got[:n] != want).sum())} of {n} bytes differ"
    assert (got[n:] == R.PACK_SENTINEL).all(), f"{what}: a byte behind n_bytes was written"


# ---------------------------------------------------------------------------- packbits
@pytest.mark.parametrize("kind", R.PACK_KINDS)
@pytest.mark.parametrize("n_bytes", R.PACK_BYTES)
def test_packbits(lib, n_bytes, kind):
    """catches: >= for > in k_packbits (the cells equal to the threshold, both kinds)."""
    g, t = R.packbits_case(n_bytes, kind)
    grid, out = Buf(g), _bytes_out(n_bytes)
    check(lib.inr_packbits(grid.ptr, n_bytes, float(t), out.data_ptr(), stream()), "packbits")
    _check_bytes(out, R.packbits32(g, t, n_bytes), f"packbits {n_bytes} {kind}")
    grid.check_guards("packbits")


def test_packbits_of_nothing(lib):
    out = _bytes_out(0)
    check(lib.inr_packbits(None, 0, 0.5, out.data_ptr(), stream()), "packbits n_bytes = 0")
    check(lib.inr_packbits(None, 0, 0.5, None, stream()), "packbits n_bytes = 0, null pointers")
    _check_bytes(out, np.zeros(0, np.uint8), "packbits n_bytes = 0")


# ---------------------------------------------------------------------------- cell positions
@pytest.mark.parametrize("n", R.POS_N)
def test_cell_positions(lib, n):
    worst = 0.0
    for H, bound, listed, kind in R.position_cases(n):
        what = f"positions n{n} H{H} b{bound} {'listed' if listed else 'identity'} {kind}"
        codes = R.position_codes(n, H, listed)
        noise = R.position_noise(kind, n, seed=n + H)
        cc = np.arange(n) if codes is None else codes
        cb = Buf(codes) if listed else None
        nb = Buf(noise) if noise is not None else None
        out = Buf(np.zeros((n, 3), f))
        out.fill_nan()
        check(lib.inr_occ_cell_positions(cb.ptr if cb else None, nb.ptr if nb else None, n, H, bound, out.ptr, stream()), what)
        got = out.get()
        tk.assert_same_bits(got, R.positions32(cc, noise, H, bound), what)
        out.check_guards(what)
        e = float(np.abs(got.astype(np.float64) - R.positions64(cc, noise, H, bound)).max()) / bound
        worst = max(worst, e)
        assert e <= R.POS_ROUNDINGS * R.U * R.POS_SLACK, f"{what}: {e:.3e} of the bound"
    print(f"positions n{n}: worst {worst / R.U:.2f} x 2^-24 of the bound, allowed {R.POS_ROUNDINGS}")


# ---------------------------------------------------------------------------- the update
def _mean_buf(start):
    return torch.full((1,), start, dtype=torch.float64, device=DEV)


def _check_mean(mean, start, new_grid, n, what):
    got = float(mean.cpu()[0])
    total = R.mean_term_sum(new_grid)
    if np.isinf(total):
        assert got == np.inf, f"{what}: mean_sum {got} for a grid that holds +inf"
        return
    want = start + total
    tol = R.mean_sum_tolerance(n, want)
    assert abs(got - want) <= tol, f"{what}: mean_sum {got!r} want {want!r} (off {abs(got - want):.3e}, allowed {tol:.3e})"


def _full_sweep(lib, n, seed, off, decay, scale, with_inf, start):
    what = f"full n{n} off{off} decay{decay} scale{scale} inf{with_inf}"
    g, s = R.update_grid(n, seed, with_inf), R.update_sigma(n, seed, with_inf)
    grid, sig, mean = Buf(g, offset=off[0]), Buf(s, offset=off[1]), _mean_buf(start)
    assert (grid.ptr % 16 == 0) == (off[0] == 0) and (sig.ptr % 16 == 0) == (off[1] == 0)
    check(lib.inr_occ_update(grid.ptr, sig.ptr, None, n, n, decay, scale, None, mean.data_ptr(), stream()), what)
    want = R.update_full32(g, s, decay, scale)
    tk.assert_same_bits(grid.get(), want, what)
    tk.assert_same_bits(sig.get(), s, what + " (sigma is read only)")
    grid.check_guards(what)
    sig.check_guards(what)
    _check_mean(mean, start, want, n, what)


@pytest.mark.parametrize("n", R.UPDATE_SIZES)
def test_update_full_sweep(lib, n):
    """catches: fmaxf dropped from the mean accumulation (the -1 and NaN cells of every finite combination), the tail
    loop starting at n4 instead of n4 * 4 (aligned, n >= 5: cells n4 .. 4 * n4 decay twice and count twice), the update
    reaching a -1 cell (those cells must keep their bits)."""
    for off in R.OFFSETS:
        for k, (decay, scale, with_inf, start) in enumerate(R.update_combos()):
            _full_sweep(lib, n, 10 * n + k, off, decay, scale, with_inf, start)


def test_update_full_sweep_above_the_workgroup_cap(lib):
    """More cells than cap * 1024: the grid-stride loops of the vector path and of the scalar path make a second trip."""
    n = R.size_above_cap(cu_count(lib))
    assert (n + 1023) // 1024 > R.workgroup_cap_factor() * cu_count(lib)
    for off in R.OFFSETS:
        for k, (decay, scale, with_inf, start) in enumerate(R.BIG_COMBOS):
            _full_sweep(lib, n, 20 + k, off, decay, scale, with_inf, start)


def _listed(lib, n, m_kind, seed, off, decay, scale, with_inf, start, same_values=False):
    what = f"listed n{n} m={m_kind} off{off} decay{decay} scale{scale} inf{with_inf} same{same_values}"
    idx = R.listed_indices(n, m_kind, seed)
    m = len(idx)
    g, s = R.update_grid(n, seed, with_inf), R.update_sigma(max(m, 1), seed, with_inf)
    if same_values:                                   # duplicates carry equal values: the result is exact
        s = R.update_sigma(n, seed + 1, with_inf)[idx] if m else s
    grid, tmp, mean = Buf(g, offset=off[0]), Buf(np.zeros(n, f), offset=off[1]), _mean_buf(start)
    tmp.fill_nan()
    sig, ib = Buf(s), Buf(idx if m else np.zeros(1, np.int32))
    check(lib.inr_occ_update(grid.ptr, sig.ptr if m else None, ib.ptr, n, m, decay, scale, tmp.ptr, mean.data_ptr(),
                             stream()), what)
    got = grid.get()
    cand, visited = R.update_listed32(g, s, idx, decay, scale)
    ok = R.listed_outcome_ok(got, g, cand, idx, visited)
    assert ok.all(), f"{what}: {int((~ok).sum())} cells hold no allowed value (first {int(np.flatnonzero(~ok)[0])})"
    if same_values or m <= 1:
        want = np.array(g, copy=True)
        want[idx.astype(np.int64)] = cand
        tk.assert_same_bits(got, want, what)
    for b in (grid, tmp, sig, ib):
        b.check_guards(what)
    _check_mean(mean, start, got, n, what)


@pytest.mark.parametrize("m_kind", R.LISTED_M)
@pytest.mark.parametrize("n", R.UPDATE_SIZES)
def test_update_listed(lib, n, m_kind):
    """Unvisited cells keep their bits (upstream's -1 fill: no decay), visited cells hold the candidate of one of their
    entries, and mean_sum is the sum over the grid the call left."""
    combos = R.update_combos()
    for io, off in enumerate(R.OFFSETS):
        for k in range(3):
            decay, scale, with_inf, start = combos[(3 * io + k * 4 + R.UPDATE_SIZES.index(n)) % 9]
            _listed(lib, n, m_kind, 10 * n + k, off, decay, scale, with_inf, start)
    _listed(lib, n, m_kind, 10 * n + 7, (0, 0), 0.95, 0.7, False, 1234.5, same_values=True)


def test_update_listed_above_the_workgroup_cap(lib):
    n = R.size_above_cap(cu_count(lib))
    _listed(lib, n, "half", 31, (0, 0), 0.95, 0.7, False, 0.0)
    _listed(lib, n, "half", 32, (0, 1), 1.0, 1.0, False, 0.0, same_values=True)


# ---------------------------------------------------------------------------- packbits with the mean
@pytest.mark.parametrize("branch", R.MEAN_BRANCHES)
@pytest.mark.parametrize("n_cells", R.MEAN_CELLS)
def test_packbits_mean(lib, n_cells, branch):
    """catches: >= for > in k_packbits_mean and fminf(mean, density_thresh) replaced by mean (branch "thresh": the
    cells equal to density_thresh, and every cell between it and the mean), counter_stride ignored (stride 2 with
    poison between the counters)."""
    g, mean_sum, dt, equal = R.packbits_mean_case(n_cells, branch)
    want_bits, want_mean, _ = R.packbits_mean32(g, n_cells, mean_sum, dt)
    grid, ms = Buf(g), _mean_buf(mean_sum)
    for n_counters, stride in R.COUNTER_SHAPES:
        for with_mean_out in (True, False):
            what = f"packbits_mean n{n_cells} {branch} counters{n_counters}x{stride} mean_out{with_mean_out}"
            c, total = R.counters_case(n_counters, stride, seed=n_counters)
            cb = Buf(c)
            out = _bytes_out(n_cells // 8)
            mo = Buf(np.zeros(4, f))
            mo.fill_nan()
            stats = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
            with_stats = n_counters > 0 or with_mean_out          # n_counters = 0: once with stats_out, once all null
            check(lib.inr_packbits_mean(grid.ptr, n_cells, ms.data_ptr(), float(dt), out.data_ptr(),
                                        mo.ptr if with_mean_out else None, cb.ptr if n_counters else None, n_counters,
                                        stride, stats.data_ptr() if with_stats else None, stream()), what)
            _check_bytes(out, want_bits, what)
            mo_got, st = mo.get(), stats.cpu().numpy()
            if with_mean_out:
                tk.assert_same_bits(mo_got[:1], np.array([want_mean], f), what + " mean_out")
                assert abs(float(mo_got[0]) - mean_sum / n_cells) <= R.ulp32(want_mean)
            assert np.isnan(mo_got[1 if with_mean_out else 0:]).all(), what + ": mean_out written beyond its float"
            if with_stats:
                assert st[0] == float(want_mean) and st[1] == float(total), (what, st.tolist(), float(want_mean), total)
            assert (st[2 if with_stats else 0:] == -7.0).all(), what + ": stats_out written beyond its two doubles"
            for b in (grid, cb, mo):
                b.check_guards(what)
    assert float(ms.cpu()[0]) == mean_sum


# ---------------------------------------------------------------------------- mark_untrained_grid
MARK = [(H, c, b) for H in R.MARK_H for c, b in R.MARK_CASCADES]


@pytest.mark.parametrize("H,cascades,bound", MARK, ids=[f"H{h}-C{c}-b{b}" for h, c, b in MARK])
def test_mark_untrained_grid(lib, H, cascades, bound):
    """A seen cell keeps its bits, an unseen one is exactly -1.  catches: half * 2 replaced by half (every H: asserted on
    the CPU), P[4] and P[1] swapped (no camera is axis-aligned)."""
    pre = R.mark_prefill(H, cascades)
    for B in R.MARK_B:
        what = f"mark H{H} C{cascades} bound{bound} B{B}"
        poses, (fx, fy, cx, cy) = R.mark_case(H, cascades, bound, B)
        grid = Buf(pre)
        pb = Buf(poses.reshape(-1)) if B else None
        check(lib.inr_mark_untrained_grid(pb.ptr if B else None, B, fx, fy, cx, cy, H, cascades, bound, grid.ptr, stream()),
              what)
        unseen = R.mark_unseen32(poses, (fx, fy, cx, cy), H, cascades, bound).reshape(-1)
        tk.assert_same_bits(grid.get(), np.where(unseen, f(-1.0), pre).astype(f), what)
        grid.check_guards(what)
        assert unseen.all() if B == 0 else (unseen.any() and not unseen.all())
