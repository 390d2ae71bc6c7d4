"""Seeded inputs of the FCOS tests (tests/test_fcos_cpu.py, tests/test_fcos.py, tests/golden/make_fcos_golden.py).
Everything is regenerated from seeds; the fixture tests/golden/fcos.npz holds only what the reference made of them."""
import numpy as np

f32 = np.float32
RUN = 256                                  # INR_FCOS_LOCATIONS_PER_WG
STRIDES = [4, 8, 16, 32]
MAIN_GRID = (96, 80, 48)
MAIN_SHAPES = [(24, 20, 12), (12, 10, 6), (6, 5, 3), (3, 3, 2)]          # 6 588 locations
SHIPPED_SHAPES = [(40, 40, 40), (20, 20, 20), (10, 10, 10), (5, 5, 5)]   # the 160^3 scenes: 73 125 locations
LOSS_TYPES = ("iou", "linear_iou", "giou")
# single-level pyramids by their number of locations: 1, 63, 64, 65, R - 1, R, R + 1, 2 R + 1, none of them a cube
SINGLE_SHAPES = {1: (1, 1, 1), 63: (7, 3, 3), 64: (8, 4, 2), 65: (13, 5, 1), RUN - 1: (17, 5, 3), RUN: (8, 8, 4),
                 RUN + 1: (1, 257, 1), 2 * RUN + 1: (27, 19, 1)}


def boxes(seed, n, grid, lo=3.0, hi=150.0, quant=4, duplicates=0):
    """n boxes with log-uniform sides lo..hi inside ``grid``, corners rounded to multiples of ``quant`` (0: not rounded);
    the first ``duplicates`` boxes are appended again."""
    rng = np.random.default_rng(seed)
    grid = np.asarray(grid, np.float64)
    side = np.minimum(np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 3))), grid)
    lo_c = rng.uniform(0, 1, (n, 3)) * (grid - side)
    hi_c = lo_c + side
    if quant:
        lo_c = np.round(lo_c / quant) * quant
        hi_c = np.maximum(np.round(hi_c / quant) * quant, lo_c + quant)
    b = np.concatenate((lo_c, hi_c), 1).astype(f32)
    return np.concatenate((b, b[:duplicates]), 0) if duplicates else b


def main_gts(seed=5):
    """B = 3 for the 6 588-location pyramid: nine quantised boxes two of which are duplicates, an empty scene, five boxes."""
    return [boxes(seed, 7, MAIN_GRID, duplicates=2), np.zeros((0, 6), f32), boxes(seed + 100, 5, MAIN_GRID)]


MAIN_ORI = [(96, 80, 48), (90, 61, 48), (50, 80, 33)]


def fixture_cases():
    """name -> dict(shapes, strides, gts, radius, norm, ori_sizes)."""
    full = np.asarray([[0, 0, 0, 28, 24, 20]], f32)
    return {
        "one_level": dict(shapes=[(5, 4, 3)], strides=[4], gts=[boxes(11, 4, (20, 16, 12), hi=20, quant=2), boxes(12, 3, (20, 16, 12), hi=20, quant=0)],
                          radius=1.5, norm=True, ori_sizes=None),
        "two_levels": dict(shapes=[(7, 6, 5), (4, 3, 3)], strides=[4, 8],
                           gts=[np.concatenate((boxes(13, 5, (28, 24, 20), hi=28), full)), np.zeros((0, 6), f32)],
                           radius=0.0, norm=False, ori_sizes=None),
        "main_r15": dict(shapes=MAIN_SHAPES, strides=STRIDES, gts=main_gts(), radius=1.5, norm=True, ori_sizes=MAIN_ORI),
        "main_r0": dict(shapes=MAIN_SHAPES, strides=STRIDES, gts=main_gts(), radius=0.0, norm=False, ori_sizes=MAIN_ORI),
    }


def single_level_case(P, G, seed=0):
    """A one-level pyramid of P locations, stride 4, B = 2: G boxes and G // 2 boxes (an empty scene at G = 1)."""
    shape = SINGLE_SHAPES[P]
    grid = tuple(4 * n for n in shape)
    side = max(max(grid) / 2, 4)
    mk = lambda s, n: boxes(s, n, grid, lo=min(3.0, side), hi=max(grid), quant=2) if n else np.zeros((0, 6), f32)
    return dict(shapes=[shape], strides=[4], gts=[mk(seed + P + G, G), mk(seed + P + G + 1, G // 2)],
                radius=1.5 if (P + G) % 2 else 0.0, norm=bool(G % 2), ori_sizes=[grid, tuple(max(g - 5, 1) for g in grid)])


def predictions(seed, shapes, B):
    """The head's outputs: cls and ctr logits, positive distances (the head ends in an exponential)."""
    rng = np.random.default_rng(seed)
    cls = [(2 * rng.standard_normal((B, 1) + tuple(s))).astype(f32) for s in shapes]
    reg = [np.exp(rng.standard_normal((B, 6) + tuple(s))).astype(f32) * f32(2) for s in shapes]
    ctr = [rng.standard_normal((B, 1) + tuple(s)).astype(f32) for s in shapes]
    return cls, reg, ctr


TIED = (0, 4)                              # the distances that plant_ties copies where it does not copy all six


def plant_ties(reg, res, shapes, B, every=3):
    """Copies the target into the prediction at every ``every``-th positive, in place: pred == target inside min / max.
    Alternately the distances TIED alone - there half the one-sided gradient is what comes out - and all six, where the
    IoU is 1 and the halves cancel.  -> the number of positives touched."""
    first, n = 0, 0
    for l, s in enumerate(shapes):
        P = s[0] * s[1] * s[2]
        for b in range(B):
            lab = res["labels"][first:first + P]
            for k, p in enumerate(np.flatnonzero(lab > 0)):
                if k % every == 0:
                    which = list(TIED) if (k // every) % 2 == 0 else list(range(6))
                    reg[l][b].reshape(6, P)[which, p] = res["reg"][first + p][which]
                    n += 1
            first += P
    return n
