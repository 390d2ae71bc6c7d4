"""tests/grid_scatter_reference.py on the CPU: the properties that make the exact tests of the table-gradient scatter
(tests/test_grid_scatter_edges.py) exact, and the reference against the oracle's own scatter-add.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_scatter_reference as R  # noqa: E402
from oracle import hashgrid  # noqa: E402


def _lattice():
    j = np.stack(np.meshgrid(*[np.arange(R.J + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return j


@pytest.mark.parametrize("log2_t,rows,hashed", [(R.DENSE, (5832, 39304), 0), (R.HASHED, (256, 256), 1)])
def test_the_table_is_the_one_the_design_needs(log2_t, rows, hashed):
    tb = R.table(log2_t)
    assert tb["num_levels"] == 2 and tb["scales"].tolist() == [16.0, 32.0] and tb["resolutions"].tolist() == [17, 33]
    assert tuple(np.diff(tb["offsets"].astype(np.int64))) == rows and tb["hashed"].tolist() == [hashed, hashed]


@pytest.mark.parametrize("bound", [1.0, 2.0])
@pytest.mark.parametrize("log2_t", [R.DENSE, R.HASHED])
def test_every_lattice_weight_is_a_multiple_of_an_eighth_and_they_sum_to_one(log2_t, bound):
    """All 33^3 lattice points, both faces included: weights are multiples of 1/8, each sample's eight weights of a level
    sum to exactly 1, every index is a row of its level, and a point with odd j on every axis sits ON a vertex of level 0
    (one weight exactly 1) - the point the overflow tests use."""
    tb = R.table(log2_t)
    j = _lattice()
    x = R.positions(j, bound)
    assert x.min() == -bound and x.max() == bound
    idx, w = R.corners(x, bound, tb)
    w8 = R.eighths(w)                                                    # asserts the multiples
    assert (w8.sum(-1) == 8).all()
    for l in range(2):
        assert idx[:, l].min() >= tb["offsets"][l] and idx[:, l].max() < tb["offsets"][l + 1]
    odd = (j % 2 == 1).all(-1)
    assert (w8[odd, 0, 0] == 8).all() and (w8[odd, 0, 1:] == 0).all() and (w8[:, 1] == 1).all()
    assert not (w8[~odd, 0] == 8).any()


def test_out_of_range_samples_contribute_nothing_whatever_their_gradient():
    tb = R.table(R.DENSE)
    x = R.positions([[3, 4, 5], [3, 4, 5], [7, 7, 7]], 2.0)
    x[1] = [3.0, 0.0, 0.0]
    g = np.array([[1, 2, 3, 4], [np.inf, np.nan, -np.inf, 5], [8, -8, 16, 0]])
    s, n, a = R.row_sums(x, g, 2.0, tb)
    s2, n2, a2 = R.row_sums(x[[0, 2]], g[[0, 2]], 2.0, tb)
    assert (s == s2).all() and (n == n2).all() and (a == a2).all()
    x[1] = [np.nan, 0.0, 0.0]
    assert (R.row_sums(x, g, 2.0, tb)[0] == s2).all()
    assert s[:5832].sum(0).tolist() == [8 * 9, 8 * -6] and s[5832:].sum(0).tolist() == [8 * 19, 8 * 4]     # weights sum to 1
    assert a[:5832].sum(0).tolist() == [8 * 9, 8 * 10]


@pytest.mark.parametrize("log2_t,bound", [(R.DENSE, 1.0), (R.HASHED, 2.0)])
def test_row_sums_against_the_oracle_scatter(log2_t, bound):
    """300 lattice samples (every 7th outside the volume) with integer gradients: the int64 sums equal the oracle's fp32
    scatter-add exactly (all its partial sums are exact here), n and S count what they say."""
    tb = R.table(log2_t)
    rng = np.random.default_rng(5)
    M = 300
    x = R.positions(rng.integers(0, R.J + 1, size=(M, 3)), bound)
    x[::7, 1] = 1.5 * bound
    g = rng.integers(-64, 65, size=(M, 4)).astype(np.float32)
    s8, n, a8 = R.row_sums(x, g, bound, tb)
    ref = hashgrid.encode_backward_table(x, g, bound, tb).numpy()
    assert (R.as_f32(s8) == ref).all()
    idx, w = R.corners(x, bound, tb)
    assert n.sum() == int((w != 0).sum()) and (a8 >= np.abs(s8)).all()
    inside = np.ones(M, bool)
    inside[::7] = False
    assert a8.sum() == 8 * int(np.abs(g[inside]).sum())
    r64, n64, s64 = R.row_sums_fp64(x, g, bound, tb)
    assert (r64 * 8 == s8).all() and (n64 == n).all() and (s64 * 8 == a8).all()


def test_pooled_samples_give_the_sums_of_the_long_array():
    """5000 samples drawn from a pool of 64 points: aggregating the gradients per point first (the gradient is linear in
    g) gives the same sums, counts and S as the sample array itself."""
    tb = R.table(R.HASHED)
    rng = np.random.default_rng(6)
    P, M = 64, 5000
    pj = rng.integers(0, R.J + 1, size=(P, 3))
    point = rng.integers(0, P, size=M)
    g = rng.integers(-64, 65, size=(M, 4))
    tot, tot_abs, cnt = R.pooled(point, g, P)
    got = R.row_sums(R.positions(pj, 1.0), tot, 1.0, tb, count=cnt, gabs=tot_abs)
    want = R.row_sums(R.positions(pj[point], 1.0), g, 1.0, tb)
    for a, b in zip(got, want):
        assert (a == b).all()


def test_patterns_have_the_runs_they_promise():
    rng = np.random.default_rng(0)
    for M in (1, 15, 16, 17, 63, 64, 65, 129):
        for kind in R.PATTERNS:
            j = R.pattern_j(kind, M, rng)
            assert j.shape == (M, 3) and j.min() >= 0 and j.max() <= R.J
    j = R.pattern_j("same", 129, rng)
    assert (j == j[0]).all()
    j = R.pattern_j("aabb", 129, rng)
    assert (j[0::2][:64] == j[1::2]).all()
    j = R.pattern_j("abab", 129, rng)
    assert (j[:-1] != j[1:]).any(-1).all() and (j[:-2] == j[2:]).all()
    j = R.pattern_j("runs", 129, rng)
    assert (j[14:19] == j[14]).all() and (j[62:67] == j[62]).all()


def test_fx_next_scale_for_int64_sums():
    """sum_bits = 64 puts 2^62 in the place of 2^30: the scale is exactly 2^32 larger wherever neither clamp is in play;
    existing callers (no sum_bits) are unchanged."""
    ref = np.array([0.0, 1e-3, 1.0, 5.0, 0.0], np.float32)
    mx = np.array([2e-4, 4e-3, 0.25, np.inf, 0.0], np.float32)
    s32, r32 = hashgrid.fx_next_scale(ref, mx, headroom=1024.0)
    s64, r64 = hashgrid.fx_next_scale(ref, mx, headroom=1024.0, sum_bits=64)
    assert (r32 == r64).all() and (s64 == s32 * np.float32(2.0 ** 32)).all() and s64[3] == 0 and s64[4] == 0
    assert s64[2] == 2.0 ** 52 and s32[2] == 2.0 ** 20                       # 1024 x 1.0 x scale = 2^62 / 2^30
    a, b = hashgrid.fx_next_scale(ref, mx), hashgrid.fx_next_scale(ref, mx, 128.0, 32)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    assert hashgrid.fx_next_scale([0.0], [1e-30], sum_bits=64)[0][0] == 2.0 ** 100          # the clamp
    assert hashgrid.fx_next_scale([0.0], [3e38], sum_bits=64)[0][0] == 2.0 ** -100
    with pytest.raises(ValueError):
        hashgrid.fx_next_scale(ref, mx, sum_bits=48)
