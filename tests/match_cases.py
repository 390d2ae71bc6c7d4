"""Inputs and expected outputs shared by tests/test_match_masks_cpu.py and tests/test_match_masks.py: the golden fixture of
the reference's own ``match_seg()`` run, seeded random views, and the layouts that stress the count kernel's aggregation
both ways.  The expectation of a generated case is the oracle's restatement (oracle/consumers.match_seg, pinned to the
reference by tests/test_match_seg_oracle.py), computed once per process."""
import os

import numpy as np

from oracle import consumers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_seg.npz")

# (name, (H, W), k, segments per view, big ids): every H x W, k, S and B of the issue's list occurs; the last case has
# more than 496 segments, from where the count kernel's LDS slice exceeds 64 KB
FUZZ = [
    ("1x1", (1, 1), 1, [1], False),
    ("7x9_k31", (7, 9), 31, [5, 1, 5], False),
    ("48x64_k32", (48, 64), 32, [64], True),
    ("61x67_k33", (61, 67), 33, [300, 5, 64], True),
    ("200x200_k70", (200, 200), 70, [64, 1, 5], False),
    ("200x200_k33", (200, 200), 33, [300], True),
    ("61x67_k70", (61, 67), 70, [1], False),
    ("48x64_k1", (48, 64), 1, [5, 64, 1], False),
    ("7x9_k70", (7, 9), 70, [64], True),
    ("200x200_k31", (200, 200), 31, [5], False),
    ("61x67_k33_S1000", (61, 67), 33, [1000, 5], True),
]
LAYOUTS = ["full", "checker", "stripes", "empty"]


def name_order(ids):
    """The reference's candidate order: sorted file names ``<img>_<id>.png``."""
    return sorted(range(len(ids)), key=lambda i: f"{int(ids[i])}.png")


def expected(seg, proj, ids, iou_thresh=0.05):
    """seg int32 [n, H, W], proj bool [n, k, H, W], ids [k] -> int32 [n, H, W] by the oracle, candidates in name order."""
    order = name_order(ids)
    out = np.empty_like(seg)
    for v in range(seg.shape[0]):
        out[v] = consumers.match_seg(seg[v], [proj[v, j] for j in order], [int(ids[j]) for j in order], iou_thresh)
    return out


def random_view(rng, H, W, k, S, big_ids):
    """Blocky segments (about S of them, ids arbitrary), some unlabeled and background area, and k ragged rectangles."""
    cells = max(1, int(np.ceil(np.sqrt(S))))
    gh, gw = min(H, cells), min(W, int(np.ceil(S / min(H, cells))))
    grid = rng.integers(0, S, size=(gh, gw))
    ys, xs = (np.arange(H) * gh) // H, (np.arange(W) * gw) // W
    lab = grid[ys[:, None], xs[None, :]]
    ids = rng.choice(np.arange(1, 5000 if big_ids else S + 1), size=S, replace=False)
    seg = ids[lab].astype(np.int32)
    if H * W > 4:
        seg[rng.random((H, W)) < 0.05] = -1
        seg[rng.random((H, W)) < 0.05] = 0
    proj = np.zeros((k, H, W), bool)
    for j in range(k):
        y0, x0 = rng.integers(0, H), rng.integers(0, W)
        y1, x1 = rng.integers(y0, H) + 1, rng.integers(x0, W) + 1
        proj[j, y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) > 0.1
    return seg, proj


def fuzz_case(name):
    """-> (seg [n, H, W], proj [n, k, H, W], instance ids [k]) of a FUZZ row, seeded by its position."""
    i = [f[0] for f in FUZZ].index(name)
    _, (H, W), k, per_view, big = FUZZ[i]
    rng = np.random.default_rng(1000 + i)
    views = [random_view(rng, H, W, k, min(S, H * W), big) for S in per_view]
    ids = rng.permutation(np.arange(1, k + 1)) if i % 2 else np.arange(1, k + 1)
    return np.stack([v[0] for v in views]), np.stack([v[1] for v in views]), ids.astype(np.int64)


def layout_case(name, H=61, W=67, k=33):
    """The aggregation stress layouts, one view each."""
    rng = np.random.default_rng(LAYOUTS.index(name))
    yy, xx = np.mgrid[0:H, 0:W]
    proj = rng.random((k, H, W)) > 0.5
    if name == "full":                      # one segment, every bit set: one group per wave step
        seg, proj = np.full((H, W), 7, np.int32), np.ones((k, H, W), bool)
    elif name == "checker":                 # neighbours never share (rank, word)
        seg = np.where((yy + xx) % 2 == 0, 3, 900).astype(np.int32)
    elif name == "stripes":                 # one-pixel rows: runs break at every row end inside a wave step
        seg = (yy % 40 + 1).astype(np.int32)
    else:                                   # "empty": no segment > 0
        seg = np.where(rng.random((H, W)) < 0.5, -1, 0).astype(np.int32)
    return seg[None], proj[None], np.arange(1, k + 1, dtype=np.int64)


_cache = {}


def case(name):
    """-> (seg, proj, ids, expected) of a FUZZ or LAYOUTS name; the oracle runs once per process and name."""
    if name not in _cache:
        seg, proj, ids = layout_case(name) if name in LAYOUTS else fuzz_case(name)
        want = expected(seg, proj, ids)
        want.setflags(write=False)
        _cache[name] = (seg, proj, ids, want)
    return _cache[name]


def golden_cases():
    """-> (z, list of (image, panoptic map, segment dicts with category_id, proj bool [k, H, W] in file order, ids,
    out), class_names) from tests/golden/match_seg.npz."""
    z = np.load(GOLDEN)
    things, stuff = {}, {}
    rows = []
    for img in (str(i) for i in z["images"]):
        info = []
        for (sid, isthing, cat), nm in zip(z[f"info_{img}"], z[f"names_{img}"]):
            (things if isthing else stuff)[int(cat)] = str(nm)
            info.append({"id": int(sid), "isthing": bool(isthing), "category_id": int(cat)})
        files, ids = consumers.projections_of([str(f) for f in z["proj_files"]], img)
        seg = z[f"seg_{img}"]
        proj = np.stack([z["proj_" + f[:-4]] for f in files]) if files else np.zeros((0,) + seg.shape, bool)
        rows.append((img, seg, info, proj, ids, z[f"out_{img}"]))
    names = {"thing_classes": [things.get(i, f"thing-{i}") for i in range(max(things) + 1)],
             "stuff_classes": [stuff.get(i, f"stuff-{i}") for i in range(max(stuff) + 1)]}
    return z, rows, names
