"""numpy restatement of the error-map loader (include/inr.h ``inr_sample_training_batch_weighted``) and of the map's
update (``inr_error_map_update``); test infrastructure only.  Every float operation below is ONE IEEE binary32 operation
in the order the header writes, so the kernels' outputs are compared with these bit for bit.

The draw: cell c of a ``cells x cells`` map row gets the key ``E_c / w_c`` with ``E_c = -ln(u_c)``,
``u_c = (m + 0.5) * 2^-24`` for a 24-bit counter hash m; the n smallest (key bits, c) pairs win - an exponential race,
which has the distribution of ``torch.multinomial(w, n, replacement=False)``.

``neg_ln_u24`` is the pinned fp32 sequence for ``-ln(u)``.  Measured over all 2^24 values of m against float64
``-log((m + 0.5) / 2^24)`` (tests/test_error_map_cpu.py::test_neg_ln_sequence_is_accurate_for_every_u):
maximum relative error 1.916557400076758e-07 (at m = 14781968), kept below as MEASURED_MAX_REL_ERR and asserted as an
upper bound without margin - the run is deterministic; the cap the loader needs is 1e-4.
"""
import numpy as np

from oracle.rays import get_rays

F32 = np.float32
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
STREAM_KEY, STREAM_ROW, STREAM_COL = 0, 1, 2
MEASURED_MAX_REL_ERR = 1.916557400076758e-07


def mix64(z):
    """SplitMix64 finaliser on a uint64 array (wrap-around arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash24(seed, step, stream, cell):
    """m_s(c) = mix64(seed + GOLDEN * (2^63 + step * 2^32 + s * 2^16 + c)) >> 40; ``step`` and ``cell`` may be arrays
    (broadcast).  -> uint64 array of 24-bit values."""
    step = np.asarray(step, dtype=np.uint64)
    cell = np.asarray(cell, dtype=np.uint64)
    ctr = np.uint64(1 << 63) + (step << np.uint64(32)) + np.uint64(stream << 16) + cell
    with np.errstate(over="ignore"):
        return mix64(np.uint64(int(seed) & MASK64) + np.uint64(GOLDEN) * ctr) >> np.uint64(40)


def neg_ln_u24(m):
    """-ln((m + 0.5) * 2^-24) for 24-bit m, the kernel's fp32 sequence (csrc/raymarch.hip ``neg_ln_u24``)."""
    v = 2 * np.asarray(m).astype(np.int64) + 1                      # odd, 1 .. 2^25 - 1: u = v / 2^25
    e0 = np.frexp(v.astype(np.float64))[1].astype(np.int64) - 1     # floor(log2 v)
    vn = v << (24 - e0)                                             # [2^24, 2^25)
    up = vn >= 23726566                                             # mantissa >= sqrt(2)
    one = np.where(up, 1 << 25, 1 << 24)
    a = (vn - one).astype(F32)
    b = (vn + one).astype(F32)                                      # round to nearest even
    s = a / b
    z = s * s
    p = z * F32(0.11111111) + F32(0.14285715)
    p = p * z + F32(0.2)
    p = p * z + F32(0.33333334)
    p = p * z + F32(1.0)
    lnf = (s + s) * p
    kf = (25 - e0 - up.astype(np.int64)).astype(F32)
    return (kf * F32(0.69314718) - lnf).astype(F32)


def keys(weights, seed, step):
    """uint32 key bits of every cell of ONE map row (``step`` scalar) or of many steps (``step`` [S] -> [S, cells^2])."""
    w = np.asarray(weights, dtype=F32).reshape(-1)
    step = np.asarray(step)
    cell = np.arange(w.shape[0])
    m = hash24(seed, step[..., None] if step.ndim else step, STREAM_KEY, cell)
    E = neg_ln_u24(m)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        k = (E / w).astype(F32)
    k = np.where(w > 0, k, F32(np.inf)).astype(F32)                 # w <= 0 or NaN: +inf
    return k.view(np.uint32)


def select(key_bits, n):
    """The n smallest (key bits, cell) pairs of one row, in ascending cell index.  -> int64 [n]."""
    kb = np.asarray(key_bits, dtype=np.uint32)
    order = np.lexsort((np.arange(kb.shape[0]), kb))
    return np.sort(order[:n]).astype(np.int64)


def sample_cells(weights, seed, step, n):
    return select(keys(weights, seed, step), n)


def pixels_of(cells_idx, cells, H, W, seed, step):
    """Upstream's in-cell pixel rule in fp32: -> (px, py, flat index) int64 arrays."""
    c = np.asarray(cells_idx, dtype=np.int64)
    r1 = hash24(seed, step, STREAM_ROW, c).astype(F32) * F32(2.0 ** -24)
    r2 = hash24(seed, step, STREAM_COL, c).astype(F32) * F32(2.0 ** -24)
    cx_, cy_ = c // cells, c % cells
    sx, sy = F32(H) / F32(cells), F32(W) / F32(cells)
    px = np.minimum((cx_.astype(F32) * sx + r1 * sx).astype(np.int64), H - 1)
    py = np.minimum((cy_.astype(F32) * sy + r2 * sy).astype(np.int64), W - 1)
    return px, py, px * W + py


def sample_training_batch_weighted(pose, intrinsics, H, W, image, mask, num_instances, error_map, cells, seed, step, n):
    """Restatement of ``inr_sample_training_batch_weighted``.  image f32 [H,W,C] or None, mask int32 [H,W] or None,
    error_map f32 [cells*cells]."""
    coarse = sample_cells(error_map, seed, step, n)
    _, _, inds = pixels_of(coarse, cells, H, W, seed, step)
    r = get_rays(np.asarray(pose, dtype=F32)[None], intrinsics, H, W, inds=inds)
    out = {"inds_coarse": coarse, "inds": inds, "rays_o": r["rays_o"][0], "rays_d": r["rays_d"][0]}
    if image is not None:
        out["rgb"] = np.asarray(image, dtype=F32).reshape(H * W, -1)[inds]
    if mask is not None:
        lab = np.asarray(mask).reshape(-1)[inds].astype(np.int64)
        out["labels"] = np.where(lab >= num_instances, -1, lab)
    return out


def error_map_update(pred, target, inds_coarse, row):
    """Restatement of ``inr_error_map_update`` for DISTINCT indices: -> the updated copy of ``row`` (f32 [cells*cells])."""
    row = np.array(row, dtype=F32).reshape(-1)
    d = np.asarray(pred, dtype=F32).reshape(-1, 3) - np.asarray(target, dtype=F32).reshape(-1, 3)
    e = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) / F32(3.0)
    c = np.asarray(inds_coarse, dtype=np.int64).reshape(-1)
    ok = (c >= 0) & (c < row.shape[0])
    row[c[ok]] = F32(0.1) * row[c[ok]] + F32(0.9) * e[ok]
    return row
