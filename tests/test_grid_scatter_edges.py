"""The hash-table gradient scatter (csrc/encoders.hip: k_grid_bwd with run_reduce_atomic4, k_grid_grad_finish,
k_grid_grad_finish64, k_grid_fx_update) row by row against tests/grid_scatter_reference.py.  Needs an MI355X.

Every other test of the scatter compares a whole gradient norm-wise; a norm cannot see one lost or misplaced contribution
on one row.  Here the inputs are chosen so that the exact answer exists (lattice positions, integer gradients: see the
reference module) and every row of every form - fp32 atomics, int32 sums, int64 sums - must equal it BIT FOR BIT, at the
places the kernel can go wrong: runs of equal rows that end at a wave or workgroup boundary, out-of-range samples inside
runs, sample counts that are no multiple of 16 or 64, `order` given, the launch split at 65535 * 64 samples, sums that pass
the integer range on their way, and run sums that do not fit the integer at all (they must poison their level, not
saturate).  General inputs get a derived per-row bound; the scale rule is compared with the oracle's at its edges."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_scatter_reference as R  # noqa: E402
from train_kernels_reference import assert_same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = ("fp32", "int32", "int64")
FLAGS = slice(64, 80)
# hand-set scales of the exact tests (level 0, level 1): powers of two >= 8, different per level so that a mixed-up level
# shows, small enough for every row sum of those tests (|sum| < 2^21) to fit
SCALES = {"int32": (256.0, 64.0), "int64": (2.0 ** 40, 2.0 ** 36)}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


class Table:
    def __init__(self, log2_t=None, tb=None):
        from instance_nerf_amd import _lib
        self.tb = R.table(log2_t) if tb is None else tb
        self.desc = _lib.make_grid_desc(self.tb)
        self.L, self.T, self.offs = int(self.tb["num_levels"]), int(self.tb["total_rows"]), self.tb["offsets"].astype(np.int64)


def _new_state(scales):
    from instance_nerf_amd import _lib
    st = np.zeros(_lib.GRID_FX_STATE_FLOATS, np.float32)
    st[:len(scales)] = scales
    return _t(st)


def scatter(lib, form, tab, x, g, bound, order=None, ranges=None, fx=None, acc=None, scales=None):
    """Scatter + finishing pass of every level range -> (gradient f32[T,2] numpy, state numpy or None).  fp32: fx_state
    NULL.  int32 / int64: the state `fx` (or a fresh one holding `scales`); the int64 accumulator must be all zero after
    its finishing pass."""
    from instance_nerf_amd import _lib
    M = x.shape[0]
    grad = torch.zeros(tab.T, 2, device=DEV)
    s, po = _lib.stream_ptr(), _lib.ptr(order, torch.int32, "order", allow_none=True)
    if form != "fp32" and fx is None:
        fx = _new_state(scales if scales is not None else SCALES[form])
    if form == "int64" and acc is None:
        acc = torch.zeros(tab.T, 2, dtype=torch.int64, device=DEV)
    for lo, hi in (ranges or ((0, tab.L),)):
        if form == "fp32":
            _lib.check(lib.inr_grid_encode_backward_levels_fx(_lib.ptr(x), _lib.ptr(g), po, tab.desc, M, float(bound),
                                                              _lib.ptr(grad), lo, hi, None, s))
        elif form == "int32":
            _lib.check(lib.inr_grid_encode_backward_levels_fx(_lib.ptr(x), _lib.ptr(g), po, tab.desc, M, float(bound),
                                                              _lib.ptr(grad), lo, hi, _lib.ptr(fx), s))
            _lib.check(lib.inr_grid_grad_finish_fx(_lib.ptr(grad), tab.desc, lo, hi, _lib.ptr(fx), s))
        else:
            _lib.check(lib.inr_grid_encode_backward_levels_fx64(_lib.ptr(x), _lib.ptr(g), po, tab.desc, M, float(bound),
                                                                _lib.ptr(grad), _lib.ptr(acc), lo, hi, _lib.ptr(fx), s))
            _lib.check(lib.inr_grid_grad_finish_fx64(_lib.ptr(acc), _lib.ptr(grad), tab.desc, lo, hi, _lib.ptr(fx), s))
    if form == "int64":
        assert not bool(acc.any()), "the int64 accumulator is not zero after its finishing pass"
    return grad.cpu().numpy(), (None if fx is None else fx.cpu().numpy())


def _permuted(rng, x, g):
    """-> (order i32[M], x', g') with x'[order[m]] = x[m]: slot m of the ordered launch processes the sample that slot m
    of the plain launch does, from permuted arrays."""
    M = x.shape[0]
    order = rng.permutation(M).astype(np.int32)
    xp, gp = np.empty_like(x), np.empty_like(g)
    xp[order], gp[order] = x, g
    return order, xp, gp


def _all_forms_exact(lib, tab, x, g, bound, want, what, ranges_set=(None,), rng=None):
    """Every form, with `order` NULL and (rng given) a random permutation: each row equals `want` in its bits, no flag is
    raised, and the integer results are the same bits whatever the order."""
    runs = [(None, _t(x), _t(g))]
    if rng is not None:
        order, xp, gp = _permuted(rng, x, g)
        runs.append((_t(order), _t(xp), _t(gp)))
    for ranges in ranges_set:
        for form in FORMS:
            gots = []
            for order, xd, gd in runs:
                got, st = scatter(lib, form, tab, xd, gd, bound, order=order, ranges=ranges)
                tag = f"{what} {form} ranges={ranges} order={'NULL' if order is None else 'permutation'}"
                assert np.isfinite(got).all(), tag
                assert_same_bits(got, want, tag)
                assert st is None or not st[FLAGS].any(), tag
                gots.append(got)
            if form != "fp32" and len(gots) == 2:
                assert_same_bits(gots[0], gots[1], f"{what} {form}: order NULL against a permutation")


MS = (1, 15, 16, 17, 63, 64, 65, 129)        # a wave carries 16 samples, a workgroup 64
RANGES = (((0, 2),), ((1, 2), (0, 1)))


# ------------------------------------------------------------------------------------------------ a. exact on integers
@pytest.mark.parametrize("bound", [1.0, 2.0])
@pytest.mark.parametrize("log2_t", [R.DENSE, R.HASHED])
def test_integer_gradients_give_every_row_bit_for_bit(lib, log2_t, bound):
    """Lattice positions and integer gradients in -64..64: every row of every form equals float32(exact sum), for M around
    the wave (16 samples) and workgroup (64) sizes, the five run patterns, both level-range schedules, `order` NULL and a
    random permutation (integer results: the same bits either way); the int64 accumulator is zero afterwards."""
    tab = Table(log2_t)
    rng = np.random.default_rng(1000 + 10 * log2_t + int(bound))
    for M in MS:
        for kind in R.PATTERNS:
            x = R.positions(R.pattern_j(kind, M, rng), bound)
            g = rng.integers(-64, 65, size=(M, 4)).astype(np.float32)
            s8, _, a8 = R.row_sums(x, g, bound, tab.tb)
            assert a8.max() < 2 ** 24                          # 8 S_r < 2^24: every fp32 partial sum is exact
            _all_forms_exact(lib, tab, x, g, bound, R.as_f32(s8), f"M={M} {kind}", ranges_set=RANGES, rng=rng)


# ---------------------------------------------------------------------------- b. out-of-range samples inside the runs
@pytest.mark.parametrize("bound", [1.0, 2.0])
@pytest.mark.parametrize("log2_t", [R.DENSE, R.HASHED])
def test_out_of_range_samples_inside_runs_add_nothing(lib, log2_t, bound):
    """The patterns of (a) with every third sample moved outside the volume (x = 1.5 bound on one axis, or a NaN
    coordinate, in turn) and its grad_out set to Inf: the rows equal the reference over the in-range samples, no poison
    flag is raised, nothing is non-finite."""
    tab = Table(log2_t)
    rng = np.random.default_rng(2000 + 10 * log2_t + int(bound))
    for M in MS:
        for kind in R.PATTERNS:
            x = R.positions(R.pattern_j(kind, M, rng), bound)
            g = rng.integers(-64, 65, size=(M, 4)).astype(np.float32)
            out = np.arange(M) % 3 == 1
            for k, m in enumerate(np.flatnonzero(out)):
                x[m, k % 3] = np.nan if k % 2 else 1.5 * bound
            g[out] = np.inf
            s8, _, a8 = R.row_sums(x, g, bound, tab.tb)
            keep = ~out
            assert (s8 == R.row_sums(x[keep], g[keep], bound, tab.tb)[0]).all() and a8.max() < 2 ** 24
            _all_forms_exact(lib, tab, x, g, bound, R.as_f32(s8), f"M={M} {kind}", rng=rng)


# ------------------------------------------------------------------------------------------------- c. the launch split
def test_the_launch_split_at_65535_blocks_is_exact(lib):
    """M = 65535 * 64 + 70 samples: the host cuts the sample array into two launches (grid.y is limited to 65535 blocks of
    64 samples), offsetting x and grad_out when `order` is NULL and `order` alone otherwise.  Dense table, positions drawn
    from a pool of 4096 lattice points, integer gradients in -64..64: every row exact in every form, both ways."""
    tab = Table(R.DENSE)
    rng = np.random.default_rng(3)
    M, P, bound = 65535 * 64 + 70, 4096, 1.0
    pool = R.positions(rng.integers(0, R.J + 1, size=(P, 3)), bound)
    point = rng.integers(0, P, size=M)
    g = rng.integers(-64, 65, size=(M, 4)).astype(np.float32)
    tot, tot_abs, cnt = R.pooled(point, g, P)
    s8, n, a8 = R.row_sums(pool, tot, bound, tab.tb, count=cnt, gabs=tot_abs)
    assert n[tab.offs[1]:].sum() == 8 * M                                # level 1: eight weights of 1/8 per sample
    assert a8.max() < 2 ** 24, a8.max()                                  # 8 max_r S_r < 2^24: fp32 partial sums are exact
    _all_forms_exact(lib, tab, pool[point], g, bound, R.as_f32(s8), "launch split", rng=rng)


# -------------------------------------------------------------------------------------------- d. modular cancellation
VERTEX = np.array([[5, 7, 9]])           # odd j on every axis: ON a vertex of level 0, its weight there exactly 1


def _vertex_case(M, at, bound=1.0):
    """M samples, all outside the volume except those at the indices `at`, which sit on the level-0 vertex."""
    x = np.full((M, 3), 1.5 * bound, np.float32)
    x[at] = R.positions(VERTEX, bound)[0]
    return x


def test_sums_that_pass_the_range_on_their_way_cancel(lib):
    """Only a row's FINAL sum must fit: three samples on one vertex in three different workgroups (sample indices 0, 64,
    128; out-of-range fillers between them) contribute +1536, +1536, -1536 at scale 2^20 (int64: 2^52) - 1.5 x 2^30
    quanta each, so the sum passes 2^31 (2^63) when the two positive ones meet first - and the row must be exactly 1536."""
    tab = Table(R.DENSE)
    at = [0, 64, 128]
    x = _vertex_case(129, at)
    g = np.random.default_rng(4).integers(-64, 65, size=(129, 4)).astype(np.float32)
    g[at] = [[1536, 1, 8, 16], [1536, 2, -8, 24], [-1536, 3, 16, 0]]
    s8, _, _ = R.row_sums(x, g, 1.0, tab.tb)
    want = R.as_f32(s8)
    row = int(R.corners(x[:1], 1.0, tab.tb)[0][0, 0, 0])
    assert want[row].tolist() == [1536.0, 6.0] and np.count_nonzero(want[:tab.offs[1]]) == 2
    for form, scales in (("fp32", None), ("int32", (2.0 ** 20, 2.0 ** 10)), ("int64", (2.0 ** 52, 2.0 ** 36))):
        got, st = scatter(lib, form, tab, _t(x), _t(g), 1.0, scales=scales)
        assert got[row, 0] == 1536.0, (form, got[row])
        assert_same_bits(got, want, form)
        assert st is None or not st[FLAGS].any(), form


# ---------------------------------------------------------------------------------------- e. range overflow is loud
FITS = (2047.0, -2047.0)
# -2048 is left out: its image -2^31 (-2^63) is representable, either outcome is allowed there
OVERFLOWS = (2048.0, 4096.0, 1e9, 3e38, -4096.0, -1e9, -3e38)
FX_EDGE = {"int32": ((2.0 ** 20, 2.0 ** 10), 128.0, 32), "int64": ((2.0 ** 52, 2.0 ** 36), 1024.0, 64)}


def _expect_level0_poisoned(lib, form, tab, x, g, tag):
    """The scatter raises level 0's flag (and only it), the finishing pass turns level 0 into NaN and leaves level 1
    exact, the scale update resets level 0: scale 0, reference 0, flag cleared."""
    from instance_nerf_amd import _lib
    scales, headroom, bits = FX_EDGE[form]
    g_in = g.copy()
    g_in[:, :2] = 0.0                                               # level 1's reference: level 0 does not matter to it
    want = R.as_f32(R.row_sums(x, g_in, 1.0, tab.tb)[0])
    fx = _new_state(scales)
    fx[16:18] = 1.0                                                 # a reference, to be reset
    got, st = scatter(lib, form, tab, _t(x), _t(g), 1.0, fx=fx)
    assert st[64] != 0 and st[65] == 0, (tag, st[64:66])
    o = tab.offs
    assert np.isnan(got[:o[1]]).all(), tag
    assert_same_bits(got[o[1]:], want[o[1]:], tag + " level 1")
    _lib.check(lib.inr_grid_fx_update(_lib.ptr(fx), 2, headroom, bits, _lib.stream_ptr()))
    st = fx.cpu().numpy()
    assert st[0] == 0 and st[16] == 0 and st[64] == 0 and st[1] > 0 and st[17] > 0, (tag, st[:2], st[16:18], st[64:66])


@pytest.mark.parametrize("form", ["int32", "int64"])
@pytest.mark.parametrize("value", FITS)
def test_a_contribution_at_the_edge_of_the_range_is_exact(lib, form, value):
    """One sample on a level-0 vertex (weight exactly 1), scale 2^20 (int64: 2^52): 2047 x scale is the largest integer
    gradient below 2^31 (2^63) - it fits and must come back exactly, without a flag."""
    tab = Table(R.DENSE)
    x = _vertex_case(1, [0])
    g = np.array([[value, 3, 8, -16]], np.float32)
    want = R.as_f32(R.row_sums(x, g, 1.0, tab.tb)[0])
    got, st = scatter(lib, form, tab, _t(x), _t(g), 1.0, scales=FX_EDGE[form][0])
    assert_same_bits(got, want, f"{form} g={value}")
    assert not st[FLAGS].any() and float(np.abs(got).max()) == 2047.0


@pytest.mark.parametrize("form", ["int32", "int64"])
@pytest.mark.parametrize("value", OVERFLOWS)
def test_a_contribution_outside_the_range_poisons_its_level(lib, form, value):
    """One sample on a level-0 vertex, scale 2^20 (int64: 2^52), |g| >= 2048: g x scale has no int32 (int64) image - for
    1e9 (int64) and 3e38 the product even leaves fp32 with g finite.  The conversion would saturate into a finite wrong
    gradient; instead the level must be poisoned exactly as by a non-finite contribution."""
    tab = Table(R.DENSE)
    x = _vertex_case(1, [0])
    g = np.array([[value, 3, 8, -16]], np.float32)
    _expect_level0_poisoned(lib, form, tab, x, g, f"{form} g={value}")


@pytest.mark.parametrize("form", ["int32", "int64"])
def test_a_merged_run_outside_the_range_poisons_its_level(lib, form):
    """16 samples of one wave on one vertex, 128 each: every contribution fits (2^27 of 2^31 quanta; int64 2^59 of 2^63),
    the run sum the wave adds (2048) does not."""
    tab = Table(R.DENSE)
    x = _vertex_case(16, list(range(16)))
    g = np.tile(np.array([[128, 3, 8, -16]], np.float32), (16, 1))
    _expect_level0_poisoned(lib, form, tab, x, g, f"{form} merged run")


@pytest.mark.parametrize("value", FITS + OVERFLOWS)
def test_fp32_atomics_have_no_range(lib, value):
    """The same single contribution through fp32 atomics: the row is float32(g), whatever its size."""
    tab = Table(R.DENSE)
    x = _vertex_case(1, [0])
    g = np.array([[value, 3, 8, -16]], np.float32)
    got, _ = scatter(lib, "fp32", tab, _t(x), _t(g), 1.0)
    row = int(R.corners(x, 1.0, tab.tb)[0][0, 0, 0])
    assert got[row].tolist() == [float(np.float32(value)), 3.0] and np.isfinite(got).all()
    assert np.count_nonzero(got[:tab.offs[1]]) == 2 and (got[tab.offs[1]:].sum(0) == [8.0, -16.0]).all()


# -------------------------------------------------------------------------------- f. row-wise bound on general inputs
@pytest.mark.parametrize("seed", [0, 3])
def test_general_inputs_stay_inside_a_derived_bound_on_every_row(lib, seed):
    """The data of test_fixed_point_table_gradient_fuzz_over_level_tables (M = 20000 random points, partly outside the
    volume, gradients over four decades) against an fp64 reference, ROW BY ROW.  With n_r the contributions of a row,
    S_r = sum |w g| over them, q = 1 / scale of the row's level and u = 2^-24:
        int32 sums     |got - ref| <= n_r q / 2 + 21 u S_r
        int64 sums     |got - ref| <= 21 u S_r + q n_r
        fp32 atomics   |got - ref| <= (n_r + 20) u S_r
    Derived, not measured: each run sum is rounded once to the quantum (half a quantum to nearest; runs <= contributions);
    four roundings go into w g, at most 15 fp32 additions into a wave's run, one final rounding to fp32 follows (21 with
    one to spare); every fp32 atomic rounds the partial row sum, which |.| <= S_r bounds.
    No constant had to be widened.  Largest error / bound on MI355X, seeds 0 and 3: fp32 atomics 0.15 and 0.13, int64
    0.26 and 0.49, int32 1.000 both (a row with a single contribution that lands half a quantum off: the bound is tight)."""
    from instance_nerf_amd import _lib
    from oracle import hashgrid
    rng = np.random.default_rng(900 + seed)
    L = int(rng.choice([2, 5, 8, 13, 16]))
    base = int(rng.choice([4, 16, 32]))
    log2_t = int(rng.choice([8, 12, 15, 19]))
    res = int(rng.choice([64, 512, 2048, 4096]))
    bound = float(rng.choice([1.0, 2.0, 4.0]))
    tab = Table(tb=hashgrid.level_table(num_levels=L, base_resolution=base, log2_hashmap_size=log2_t, desired_resolution=res))
    gen = torch.Generator().manual_seed(seed)
    M = 20000
    x = ((torch.rand(M, 3, generator=gen) * 2.2 - 1.1) * bound).contiguous()
    go = (torch.randn(M, 2 * L, generator=gen) * 10.0 ** (torch.rand(M, 1, generator=gen) * 4 - 6)).contiguous()
    ref, n, S = R.row_sums_fp64(x.numpy(), go.numpy(), bound, tab.tb)
    xd, god = x.to(DEV), go.to(DEV)
    u = 2.0 ** -24
    level = np.searchsorted(tab.offs, np.arange(tab.T), side="right") - 1
    nn = n.astype(np.float64)[:, None]

    def worst(got, bnd):
        err = np.abs(got.astype(np.float64) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
        return float(ratio.max()), int((err > bnd).sum())

    got, _ = scatter(lib, "fp32", tab, xd, god, bound)
    r, bad = worst(got, (nn + 20) * u * S)
    print(f"seed {seed} (L={L} base={base} log2_t={log2_t} res={res} bound={bound}) fp32: largest error / bound {r:.3f}")
    assert bad == 0, ("fp32", r, bad)
    for form, headroom, bits in (("int32", 128.0, 32), ("int64", 1024.0, 64)):
        fx = _new_state(())
        acc = torch.zeros(tab.T, 2, dtype=torch.int64, device=DEV) if form == "int64" else None
        scatter(lib, form, tab, xd, god, bound, fx=fx, acc=acc)                          # no scales yet: fp32 atomics
        _lib.check(lib.inr_grid_fx_update(_lib.ptr(fx), L, headroom, bits, _lib.stream_ptr()))
        scales = fx[:16].cpu().numpy().astype(np.float64)
        assert (scales[:L] > 0).all()
        got, st = scatter(lib, form, tab, xd, god, bound, fx=fx, acc=acc)
        assert not st[FLAGS].any()
        q = (1.0 / scales[:L])[level][:, None]
        bnd = nn * q / 2 + 21 * u * S if form == "int32" else 21 * u * S + q * nn
        r, bad = worst(got, bnd)
        print(f"seed {seed} {form}: largest error / bound {r:.3f}")
        assert bad == 0, (form, r, bad)


# ------------------------------------------------------------------------------------------ g. the scale rule's edges
def _update(lib, ref, mx, num_levels, headroom, bits, rng):
    """One k_grid_fx_update over a hand-written state of 16 levels -> (state before, state after) as numpy."""
    from instance_nerf_amd import _lib
    st = np.zeros(_lib.GRID_FX_STATE_FLOATS, np.float32)
    st[:16] = 1.0                                                     # (an old scale: not an input of the rule)
    st[16:32] = ref
    st[32:48] = 7.0
    st[64:80] = 1.0                                                   # raised flags: the update clears them
    st[80:96] = 0.25
    for l in range(16):
        slots = (mx[l] * rng.uniform(0, 1, 256)).astype(np.float32) if np.isfinite(mx[l]) else np.zeros(256, np.float32)
        slots[rng.integers(0, 256)] = mx[l]
        st[96 + 256 * l:96 + 256 * (l + 1)] = slots
    fx = _t(st)
    _lib.check(lib.inr_grid_fx_update(_lib.ptr(fx), num_levels, headroom, bits, _lib.stream_ptr()))
    return st, fx.cpu().numpy()


@pytest.mark.parametrize("bits", [32, 64])
def test_the_scale_rule_at_its_edges(lib, bits):
    """k_grid_fx_update against oracle/hashgrid.py::fx_next_scale, scales and references bit for bit, for int32 and int64
    sums: headroom 2, 128, 1024, 2^20; references and maxima at 1e-38, 1e-30, 1e30, 3e38 (the +-100 clamp of the exponent
    is in play); every exact power of two 2^k, k = -40..40, as the step maximum - floor(log2(.)) then sits ON a boundary,
    one ulp of the logarithm would halve the scale - without a reference and under a larger one; and num_levels 1, 2, 16:
    levels >= num_levels stay untouched."""
    from oracle import hashgrid
    rng = np.random.default_rng(60 + bits)
    edge = [1e-38, 1e-30, 1e30, 3e38]
    pairs = [(r, m) for r in [0.0] + edge for m in edge]
    pairs += [(0.0, 2.0 ** k) for k in range(-40, 41)] + [(2.0 ** (k + 1), 2.0 ** k) for k in range(-40, 41)]
    while len(pairs) % 16:
        pairs.append((0.0, 1.0))
    pairs = np.asarray(pairs, dtype=np.float32)
    for headroom in (2.0, 128.0, 1024.0, 2.0 ** 20):
        for i in range(0, len(pairs), 16):
            ref, mx = pairs[i:i + 16, 0], pairs[i:i + 16, 1]
            _, got = _update(lib, ref, mx, 16, headroom, bits, rng)
            s_ref, r_ref = hashgrid.fx_next_scale(ref, mx, headroom=headroom, sum_bits=bits)
            what = f"bits={bits} headroom={headroom} pairs {i}.."
            assert_same_bits(got[:16], s_ref, what + f" scales (ref {ref}, max {mx})")
            assert_same_bits(got[16:32], r_ref, what + " references")
            assert_same_bits(got[32:48], mx, what + " step maxima")
            assert not got[FLAGS].any(), what
    ref = (10.0 ** rng.uniform(-6, 2, 16)).astype(np.float32)
    mx = (ref * 10.0 ** rng.uniform(-2, 1, 16)).astype(np.float32)
    for nl in (1, 2, 16):
        before, got = _update(lib, ref, mx, nl, 128.0, bits, rng)
        s_ref, r_ref = hashgrid.fx_next_scale(ref, mx, headroom=128.0, sum_bits=bits)
        assert_same_bits(got[:nl], s_ref[:nl], f"num_levels={nl} scales")
        assert_same_bits(got[16:16 + nl], r_ref[:nl], f"num_levels={nl} references")
        assert not got[64:64 + nl].any()
        for lo in (0, 16, 32, 64, 80):                                # levels >= num_levels: nothing moved
            assert_same_bits(got[lo + nl:lo + 16], before[lo + nl:lo + 16], f"num_levels={nl} state[{lo}+l] of the levels beyond")
        assert_same_bits(got[96 + 256 * nl:], before[96 + 256 * nl:], f"num_levels={nl} block maxima of the levels beyond")


# ------------------------------------------------------------------------------------------------------- h. fx[48]
@pytest.mark.parametrize("form", ["int32", "int64"])
def test_fixed_point_steps_are_counted_from_any_level(lib, form):
    """state[48] counts the steps with at least one fixed-point level.  Level 0 gets an all-zero gradient, so it never has
    a scale; level 1 runs on integer sums from the second step on: the counter must advance (and the gradient is exact
    in every step)."""
    from instance_nerf_amd import _lib
    tab = Table(R.DENSE)
    rng = np.random.default_rng(8)
    M = 70
    x = R.positions(rng.integers(0, R.J + 1, size=(M, 3)), 1.0)
    g = rng.integers(-64, 65, size=(M, 4)).astype(np.float32)
    g[:, :2] = 0.0
    want = R.as_f32(R.row_sums(x, g, 1.0, tab.tb)[0])
    headroom, bits = FX_EDGE[form][1:]
    fx = _new_state(())
    acc = torch.zeros(tab.T, 2, dtype=torch.int64, device=DEV) if form == "int64" else None
    for step, counted in enumerate((0, 1, 2)):
        got, st = scatter(lib, form, tab, _t(x), _t(g), 1.0, fx=fx, acc=acc)
        assert_same_bits(got, want, f"{form} step {step}")
        assert st[0] == 0 and (st[1] > 0) == (step > 0), (step, st[:2])
        _lib.check(lib.inr_grid_fx_update(_lib.ptr(fx), 2, headroom, bits, _lib.stream_ptr()))
        st = fx.cpu().numpy()
        assert st[0] == 0 and st[1] >= 8 and st[48] == counted, (form, step, st[:2], st[48])
