"""Seeded inputs shared by tests/golden/make_detections_golden.py and the detector-tail tests.  Everything comes from an
integer hash written out here (no library generator whose stream could change), so the fixture needs to hold only what the
reference RETURNED for these inputs."""
import numpy as np

f = np.float32


def uniform(seed, n):
    """n doubles in [0, 1) on a 2^-24 lattice: splitmix64 of the index."""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x632BE59BD9B4E019)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def mask_probs(seed, N, M, kinds=()):
    """fp32 [N, M, M, M] in [0, 1] on a 1/256 lattice (no denormals anywhere near): contrast-stretched noise, so that many
    samples fall close to 0.5; ``kinds[n]``: "half" = 0.5 everywhere, "binary" = exact 0s and 1s."""
    u = uniform(seed, N * M ** 3).reshape(N, M, M, M)
    m = np.round(np.clip((u - 0.5) * 3 + 0.5, 0, 1) * 256) / 256
    for n, kind in enumerate(kinds):
        if kind == "half":
            m[n] = 0.5
        elif kind == "binary":
            m[n] = u[n] > 0.5
    return m.astype(f)


def random_boxes(seed, N, shape):
    """Boxes that start inside the grid and may end past it."""
    u = uniform(seed, N * 6).reshape(N, 6)
    size = np.asarray(shape, np.float64)
    lo = u[:, :3] * size * 0.6 - 1.0
    return np.concatenate([lo, lo + 0.7 + u[:, 3:] * size * 0.9], 1).astype(f)


def corner_boxes(shape):
    """The named corners for a grid (W, L, H): spanning the grid; inside; touching the far faces; leaving the grid on the
    low side and on the high side (unclipped); integer coordinates; side 0.3; spanning again (for the all-0.5 mask)."""
    W, L, H = (float(v) for v in shape)
    return np.asarray([
        [0, 0, 0, W, L, H],
        [0.13 * W, 0.17 * L, 0.14 * H, 0.76 * W, 0.73 * L, 0.78 * H],
        [0.4 * W, 0.35 * L, 0.3 * H, W, L, H],
        [-0.28 * W, -0.21 * L, -0.24 * H, 0.47 * W, 0.47 * L, 0.44 * H],
        [0.45 * W, 0.46 * L, 0.46 * H, 1.39 * W, 1.36 * L, 1.5 * H],
        [2, 1, 1, W - 2, L - 2, H - 1],
        [0.45 * W, 0.45 * L, 0.42 * H, 0.45 * W + 0.3, 0.45 * L + 0.3, 0.42 * H + 0.3],
        [-0.5, -0.5, -0.5, W - 0.5, L - 0.5, H - 0.5]], f)


CORNER_KINDS = ("noise", "noise", "noise", "noise", "noise", "binary", "noise", "half")


def paste_cases():
    """name -> (mask_probs, boxes, shape).  "small" is the M = 4 case whose texels span many voxels."""
    out = {}
    for name, shape, M, extra, seed in (("small", (9, 7, 5), 4, 0, 1), ("mid", (24, 20, 17), 20, 4, 2),
                                        ("big", (40, 33, 21), 28, 0, 3)):
        boxes = np.concatenate([corner_boxes(shape), random_boxes(seed, extra, shape)])
        out[name] = (mask_probs(seed, len(boxes), M, CORNER_KINDS), boxes, shape)
    out["empty"] = (np.zeros((0, 4, 4, 4), f), np.zeros((0, 6), f), (9, 7, 5))
    return out


def nms_case():
    """(boxes [n, 6], scores [n], classes [n]): random boxes of three classes in a 17^3 region, then
    rows n-6..n-5  classes 1 and 2, the same box: they overlap across classes only, both stay;
    rows n-4..n-3  class 1, IoU exactly 0.2 = 1 / (3 + 3 - 1): stays at threshold 0.2 (the reference keeps iou <= t);
    rows n-2..n-1  class 2, IoU exactly 0.25 = 2 / (5 + 5 - 2).
    Scores are distinct."""
    n0 = 42
    u = uniform(7, n0 * 6).reshape(n0, 6)
    lo = u[:, :3] * 8
    boxes = np.concatenate([lo, lo + 3 + u[:, 3:] * 6], 1)
    classes = (uniform(8, n0) * 3).astype(np.int64) + 1
    special = np.asarray([[30, 30, 30, 33, 33, 33], [30, 30, 30, 33, 33, 33],
                          [40, 0, 0, 43, 1, 1], [42, 0, 0, 45, 1, 1],
                          [50, 0, 0, 55, 1, 1], [53, 0, 0, 58, 1, 1]], np.float64)
    boxes = np.concatenate([boxes, special]).astype(f)
    classes = np.concatenate([classes, [1, 2, 1, 1, 2, 2]])
    n = len(boxes)
    scores = ((np.argsort(np.argsort(uniform(9, n))) + 1) / (n + 1.0)).astype(f)       # a permutation: distinct
    return boxes, scores, classes


def head_case():
    """(boxes [n, C, 6], scores [n, C], image_shape) for the ``postprocess_detections`` rule: C = 3 (class 0 = background),
    boxes that leave the grid (clipped), rows whose clipped box has a side < 1e-2, scores below the threshold."""
    n, C, shape = 30, 3, (20, 18, 16)
    u = uniform(11, n * C * 6).reshape(n, C, 6)
    size = np.asarray(shape, np.float64)
    lo = u[..., :3] * size * 1.1 - 2.0
    boxes = np.concatenate([lo, lo + 0.5 + u[..., 3:] * size * 0.8], -1)
    boxes[3, 1] = [19.995, 2, 2, 25, 6, 6]                 # clipped to a side of 0.005: dropped
    boxes[4, 2] = [-5, -5, -5, -1, 4, 4]                   # clipped to a side of 0: dropped
    raw = uniform(12, n * C).reshape(n, C) ** 3
    raw[5] = [1.0, 1e-4, 2e-4]                             # both below score_thresh after normalising
    scores = raw / raw.sum(1, keepdims=True)
    flat = scores[:, 1:].reshape(-1)
    assert len(np.unique(flat.astype(f))) == len(flat)
    return boxes.astype(f), scores.astype(f), shape
