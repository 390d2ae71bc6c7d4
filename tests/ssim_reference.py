"""Reference for the SSIM kernel (include/inr.h, "Image quality of rendered views"; csrc/ssim.hip).  numpy only.

``ssim_f64``  the definition in binary64: the eleven binary32 window values (the contract) widened to binary64, valid
              windows only, E[x^2] - mu^2 as written, C1 = (0.01 L)^2, C2 = (0.03 L)^2, per-image mean, squared-error sum.
``ssim_f32``  the binary32 restatement of the kernel's arithmetic, operation for operation: per 64 x 16 tile and channel
              the pivot (the truth pixel at the tile's first window centre, 0 when not finite) is subtracted, products are
              rounded to binary32, the horizontal then the vertical 11-tap pass run as acc = g0 v0; acc = acc + gk vk with
              separate multiplies and adds, the formula follows the header, map entries are added in binary64.
``tolerance`` per case, 8 x max |restatement - definition| (the convention of the background and field suites), never
              below 8 half-ulps of the binary32 result: nothing comes from the code under test.
"""
import numpy as np

TAPS, SIGMA = 11, 1.5
TILE_W, TILE_H = 64, 16            # include/inr.h INR_SSIM_TILE_W / INR_SSIM_TILE_H
HALO = TAPS - 1


def window64():
    i = np.arange(TAPS, dtype=np.float64)
    g = np.exp(-(i - TAPS // 2) ** 2 / (2.0 * SIGMA ** 2))
    return g / g.sum()


def window32():
    """The contract: normalised in binary64, then rounded to binary32."""
    return window64().astype(np.float32)


def _as_batch(a):
    a = np.asarray(a)
    if a.ndim == 3:
        a = a[None]
    assert a.ndim == 4, a.shape
    return a


def infer_range(pred, truth):
    """``data_range=None``: max(pred.max() - pred.min(), truth.max() - truth.min()) over the whole call, in binary32."""
    p, t = np.asarray(pred, np.float32), np.asarray(truth, np.float32)
    return np.float32(max(np.float32(p.max() - p.min()), np.float32(t.max() - t.min())))


def _range32(pred, truth, data_range):
    return infer_range(pred, truth) if data_range is None else np.float32(data_range)


def _valid_windowed(a, g):
    """Separable valid correlation of [B, H, W, C] with g along H and W, in a's dtype, taps in order 0..10."""
    B, H, W, C = a.shape
    Wm, Hm = W - HALO, H - HALO
    h = g[0] * a[:, :, 0:Wm]
    for k in range(1, TAPS):
        h = h + g[k] * a[:, :, k:k + Wm]
    v = g[0] * h[:, 0:Hm]
    for k in range(1, TAPS):
        v = v + g[k] * h[:, k:k + Hm]
    return v


def ssim_f64(pred, truth, data_range=1.0):
    """-> (map [B, H-10, W-10, C], mean [B], sse [B]), all binary64."""
    L = np.float64(_range32(pred, truth, data_range))
    x, y = _as_batch(pred).astype(np.float64), _as_batch(truth).astype(np.float64)
    g = window32().astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mx, my = _valid_windowed(x, g), _valid_windowed(y, g)
        vx = _valid_windowed(x * x, g) - mx * mx
        vy = _valid_windowed(y * y, g) - my * my
        cov = _valid_windowed(x * y, g) - mx * my
        C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        m = ((2 * mx * my + C1) * (2 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
        d = x - y
        return m, m.mean(axis=(1, 2, 3)), (d * d).sum(axis=(1, 2, 3))


def ssim_f32(pred, truth, data_range=1.0):
    """The kernel's arithmetic in binary32 -> (map float32, mean float32 [B], sse float32 [B])."""
    f32 = np.float32
    L = _range32(pred, truth, data_range)
    x, y = _as_batch(pred).astype(f32), _as_batch(truth).astype(f32)
    B, H, W, C = x.shape
    Hm, Wm = H - HALO, W - HALO
    g = window32()
    k1, k2 = f32(0.01) * L, f32(0.03) * L
    C1, C2 = f32(k1 * k1), f32(k2 * k2)
    two = f32(2.0)
    out = np.empty((B, Hm, Wm, C), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, Hm, TILE_H):
            for c0 in range(0, Wm, TILE_W):
                th, tw = min(TILE_H, Hm - r0), min(TILE_W, Wm - c0)
                pivot = y[:, r0 + HALO // 2, c0 + HALO // 2, :].copy()                  # [B, C]
                pivot[~np.isfinite(pivot)] = 0
                pivot = pivot[:, None, None, :]
                xs = x[:, r0:r0 + th + HALO, c0:c0 + tw + HALO] - pivot
                ys = y[:, r0:r0 + th + HALO, c0:c0 + tw + HALO] - pivot
                sx, sy = _valid_windowed(xs, g), _valid_windowed(ys, g)
                exx, eyy, exy = _valid_windowed(xs * xs, g), _valid_windowed(ys * ys, g), _valid_windowed(xs * ys, g)
                assert sx.dtype == f32 and exy.dtype == f32
                mx, my = sx + pivot, sy + pivot
                vx, vy, cov = exx - sx * sx, eyy - sy * sy, exy - sx * sy
                a1, a2 = two * (mx * my) + C1, two * cov + C2
                b1, b2 = (mx * mx + my * my) + C1, (vx + vy) + C2
                out[:, r0:r0 + th, c0:c0 + tw] = (a1 * a2) / (b1 * b2)
        mean = (out.astype(np.float64).sum(axis=(1, 2, 3)) / float(Hm * Wm * C)).astype(f32)
        d = x - y
        sse = (d * d).astype(np.float64).sum(axis=(1, 2, 3)).astype(f32)
    return out, mean, sse


def tolerance(pred, truth, data_range=1.0):
    """-> dict: ``ssim`` = 8 x max(max |map32 - map64|, 2^-24) - it also bounds the mean, whose error is a mean of map
    errors -, ``sse`` = 8 x max(|sse32 - sse64|, 2^-24 |sse64|), and the binary64 reference itself (``map``, ``mean``,
    ``sse_ref``).  The 2^-24 terms are the format's share: every result is ONE binary32 of magnitude up to 1 (up to |sse|),
    which carries half an ulp whether or not this case's rounding happened to land closer.  Without it an 11 x 11 image -
    one map entry, one draw of the restatement's error - can measure 1e-8 (or 0) and would then allow less than the
    format can hold; with it the allowance of such a case is 4.8e-7.  ``map_error`` / ``mean_error`` are the raw figures."""
    m64, mean64, sse64 = ssim_f64(pred, truth, data_range)
    m32, mean32, sse32 = ssim_f32(pred, truth, data_range)
    def largest(got, want, floor=0.0):          # over the entries the definition keeps finite (the others: NaN patterns, exact)
        keep = np.isfinite(want)
        if not keep.any():
            return 0.0
        return float(np.max(np.maximum(np.abs(got.astype(np.float64)[keep] - want[keep]), floor * np.abs(want[keep]))))

    err, err_mean, err_sse = largest(m32, m64), largest(mean32, mean64), largest(sse32, sse64, 2.0 ** -24)
    return {"ssim": 8 * max(err, 2.0 ** -24), "sse": 8 * err_sse, "map_error": err, "mean_error": err_mean,
            "map": m64, "mean": mean64, "sse_ref": sse64}


# ---- tolerance-tier inputs: data_range >= 0.25 x max |value| -------------------------------------------------------
KINDS = ("random", "smooth_noisy", "flat_noise")


def make_case(kind, B, H, W, C, seed=0, scale=1.0):
    """(pred, truth) float32 [B, H, W, C] in [0, scale]: uniform noise against uniform noise; a smooth image against a
    noisy copy of it; a flat 0.7 wall against 0.7 + 1e-3 noise (pure cancellation in E[x^2] - mu^2)."""
    rng = np.random.default_rng([seed, B, H, W, C, KINDS.index(kind)])
    if kind == "random":
        truth, pred = rng.random((B, H, W, C)), rng.random((B, H, W, C))
    elif kind == "smooth_noisy":
        ii, jj = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
        phase = rng.random((B, 1, 1, C)) * 6.0
        truth = 0.5 + 0.4 * np.sin(5.0 * ii[None, :, :, None] + 3.0 * jj[None, :, :, None] + phase)
        pred = np.clip(truth + 0.05 * rng.standard_normal((B, H, W, C)), 0.0, 1.0)
    elif kind == "flat_noise":
        truth = np.full((B, H, W, C), 0.7)
        pred = truth + 1e-3 * rng.standard_normal((B, H, W, C))
    else:
        raise ValueError(kind)
    return (pred * scale).astype(np.float32), (truth * scale).astype(np.float32)
