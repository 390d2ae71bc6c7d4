"""An exact reference of the hash-table gradient scatter (csrc/encoders.hip: k_grid_bwd / run_reduce_atomic4 and the two
finishing passes), NumPy on the CPU only.

The design that makes "exact" possible: a table of two levels whose scales are 16 and 32 (``table``), positions on the
lattice x = (j / 32 * 2 - 1) * bound with integer j in 0..32 per axis (``positions``) and integer ``grad_out``.  Then every
trilinear weight is a multiple of 1/8, a sample's eight weights sum to exactly 1 and every contribution w * g is a multiple
of 1/8: ``row_sums`` accumulates round(8 w) * g in int64, and the kernel's fp32 sums are exact while 8 |partial sum| < 2^24,
its fixed-point sums for every scale >= 8.  tests/test_grid_scatter_cpu.py asserts these properties on the oracle, so the
design cannot rot; tests/test_grid_scatter_edges.py compares the kernels with the sums row by row, bit for bit.

Indices and weights always come from ``oracle.hashgrid.corner_indices_weights`` (the kernels take the same fp32 decisions
operation by operation).  ``row_sums_fp64`` is the same scatter for general inputs: fp32 weights of the oracle, products
and sums in fp64, plus what a derived per-row error bound needs."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import hashgrid  # noqa: E402

J = 32                      # lattice steps per axis: j in 0..J, both faces of the volume included
DENSE, HASHED = 19, 8       # log2_hashmap_size: 5832 + 39304 dense rows, or 256 + 256 hashed rows


def table(log2_hashmap_size):
    """Two levels, resolutions 17 and 33: scales exactly 16 and 32."""
    return hashgrid.level_table(num_levels=2, base_resolution=17, desired_resolution=33, log2_hashmap_size=log2_hashmap_size)


def positions(j, bound):
    """j int[M,3] in 0..32 -> x f32[M,3] = (j / 32 * 2 - 1) * bound (exact in fp32 for bound 1 and 2)."""
    j = np.asarray(j)
    assert j.ndim == 2 and j.shape[1] == 3 and j.min() >= 0 and j.max() <= J
    return ((j.astype(np.float32) / np.float32(J) * np.float32(2) - np.float32(1)) * np.float32(bound)).astype(np.float32)


def corners(x, bound, tb):
    """-> (idx i64[M,L,8] absolute rows, w f32[M,L,8]); an out-of-range sample has weight 0 everywhere."""
    idx, w = hashgrid.corner_indices_weights(np.ascontiguousarray(x, dtype=np.float32), bound, tb)
    return idx.numpy(), w.numpy()


def eighths(w):
    """Weights that are multiples of 1/8 -> int64 8 w (asserts that they are)."""
    w8 = np.rint(w.astype(np.float64) * 8.0)
    assert (w8 == w.astype(np.float64) * 8.0).all(), "a weight is not a multiple of 1/8"
    return w8.astype(np.int64)


def _scatter(idx, vals, rows):
    """sum of vals[..., f] into rows idx, f64 (exact for integers below 2^53) -> [rows, F]."""
    flat = idx.reshape(-1)
    return np.stack([np.bincount(flat, weights=vals[..., f].reshape(-1).astype(np.float64), minlength=rows)
                     for f in range(vals.shape[-1])], axis=1)


def row_sums(x, g, bound, tb, count=None, gabs=None):
    """The exact table gradient of lattice positions x f32[M,3] and integer gradients g [M, L*2].

    -> (sum8 i64[T,2], n i64[T], s8 i64[T,2]): the row sums, the number of contributions per row (in-range samples with a
    non-zero weight on the row) and S = sum |w g|, sums and S in EIGHTHS.  An out-of-range sample contributes nothing,
    whatever its gradient holds (Inf and NaN included).
    ``count`` i64[M] and ``gabs`` [M, L*2]: x is a pool of distinct points, g the per-point SUM of the gradients of the
    samples drawn from it (the gradient is linear in g), count how many samples each point stands for and gabs the
    per-point sum of |g| - n and S then describe the long sample array, not the pool."""
    idx, w = corners(x, bound, tb)
    M, L, _ = idx.shape
    T = int(tb["total_rows"])
    w8 = eighths(w)                                                              # [M,L,8]
    inside = (w8 != 0).any(axis=(1, 2))
    g = np.where(inside[:, None], np.asarray(g, dtype=np.float64), 0.0)         # (never int(Inf))
    assert np.isfinite(g).all() and (g == np.rint(g)).all(), "gradients of in-range samples must be integers"
    g = g.reshape(M, L, 1, 2)
    ga = np.abs(g) if gabs is None else np.where(inside[:, None], np.asarray(gabs, dtype=np.float64), 0.0).reshape(M, L, 1, 2)
    c = np.ones(M, np.int64) if count is None else np.asarray(count, dtype=np.int64)
    sum8 = _scatter(idx, w8[..., None] * g, T)
    s8 = _scatter(idx, w8[..., None] * ga, T)
    n = np.bincount(idx.reshape(-1), weights=((w8 != 0) * c[:, None, None]).reshape(-1).astype(np.float64), minlength=T)
    assert np.abs(sum8).max(initial=0) < 2.0 ** 53 and s8.max(initial=0) < 2.0 ** 53
    return sum8.astype(np.int64), n.astype(np.int64), s8.astype(np.int64)


def pooled(point, g, P):
    """Samples drawn from a pool: point i64[M] in 0..P-1, g integer [M, C] -> (sum of g, sum of |g|, samples) per point."""
    g = np.asarray(g, dtype=np.float64)
    tot = np.stack([np.bincount(point, weights=g[:, c], minlength=P) for c in range(g.shape[1])], axis=1)
    tot_abs = np.stack([np.bincount(point, weights=np.abs(g[:, c]), minlength=P) for c in range(g.shape[1])], axis=1)
    return tot, tot_abs, np.bincount(point, minlength=P).astype(np.int64)


def as_f32(sum8):
    """float32(exact row sum): what every form of the scatter must return, bit for bit, while the sums are exact."""
    assert np.abs(sum8).max(initial=0) < 2 ** 24, "the exact sum has more than 24 bits: fp32 cannot hold it"
    return (sum8.astype(np.float64) / 8.0).astype(np.float32)


def row_sums_fp64(x, g, bound, tb):
    """General inputs: -> (ref f64[T,2], n i64[T], S f64[T,2]) from the oracle's fp32 weights, products and sums in fp64."""
    idx, w = corners(x, bound, tb)
    M, L, _ = idx.shape
    T = int(tb["total_rows"])
    inside = (w != 0).any(axis=(1, 2))
    g = np.where(inside[:, None], np.asarray(g, dtype=np.float64), 0.0).reshape(M, L, 1, 2)
    contrib = w.astype(np.float64)[..., None] * g
    n = np.bincount(idx.reshape(-1), weights=(w != 0).reshape(-1).astype(np.float64), minlength=T).astype(np.int64)
    return _scatter(idx, contrib, T), n, _scatter(idx, np.abs(contrib), T)


# ---------------------------------------------------------------------------- sample patterns of the in-wave run merge
PATTERNS = ("same", "aabb", "abab", "runs", "random")


def pattern_j(kind, M, rng):
    """Lattice indices j i64[M,3] of M consecutive samples.  A wave of the scatter carries 16 samples, a workgroup 64:
    "same" = one run through every boundary, "aabb" = runs of two, "abab" = no two neighbours equal (nothing merges),
    "runs" = one run over samples 14..18 (across a wave boundary) and one over 62..66 (across a workgroup boundary) among
    random points, "random" = random points."""
    j = rng.integers(0, J + 1, size=(M, 3))
    if kind == "same":
        j[:] = j[0]
    elif kind == "aabb":
        j = j[np.arange(M) // 2]
    elif kind == "abab":
        a, b = np.array([5, 9, 30]), np.array([6, 9, 30])           # neighbours on x: they share rows
        j = np.where((np.arange(M) % 2 == 0)[:, None], a, b)
    elif kind == "runs":
        j[14:19] = j[14] if M > 14 else 0
        j[62:67] = j[62] if M > 62 else 0
    elif kind != "random":
        raise ValueError(kind)
    return j
