"""Seeded inputs shared by tests/golden/make_box_targets_golden.py and the box-target tests (instance_nerf_amd/targets.py,
csrc/assign.hip).  Everything comes from the integer hash of tests/detections_cases.py, so the fixture holds only what the
reference RETURNED for these inputs.

A case is a dict: gt fp32 [G, 6], boxes fp32 [A, 6], valid bool [A] or None, gt_labels int64 [G] or None, high, low (the
thresholds as Python floats), allow (low-quality matches)."""
import numpy as np

from detections_cases import uniform

f = np.float32
NAN = float("nan")
RPN = dict(high=0.35, low=0.2)         # the shipped RPN thresholds
HEAD = dict(high=0.25, low=0.25)       # the shipped head thresholds: no "between"
RUN = 1024                             # boxes of one workgroup (include/inr.h INR_BOX_MATCH_BOXES_PER_WG)


def case(gt, boxes, valid=None, gt_labels=None, high=0.35, low=0.2, allow=True):
    return dict(gt=np.ascontiguousarray(gt, f).reshape(-1, 6), boxes=np.ascontiguousarray(boxes, f).reshape(-1, 6),
                valid=None if valid is None else np.ascontiguousarray(valid, bool),
                gt_labels=None if gt_labels is None else np.ascontiguousarray(gt_labels, np.int64),
                high=high, low=low, allow=allow)


def scene(seed, A, G, extent=40.0):
    """G ground-truth boxes and A boxes in a cube of ``extent``: sides 3..15; every third box is a jittered copy of a GT
    box (IoU anywhere between 0.2 and 1), the others are placed at random (mostly IoU 0 or small)."""
    u = uniform(seed, G * 6).reshape(G, 6)
    lo = u[:, :3] * extent
    gt = np.concatenate([lo, lo + 3.0 + u[:, 3:] * 12.0], 1)
    v = uniform(seed + 1000, A * 6).reshape(A, 6)
    lo = v[:, :3] * extent
    boxes = np.concatenate([lo, lo + 3.0 + v[:, 3:] * 12.0], 1)
    w = uniform(seed + 2000, A * 6).reshape(A, 6)
    near = np.arange(A) % 3 == 0
    boxes[near] = gt[np.arange(A)[near] % G] + (w[near] - 0.5) * 2.0
    return gt.astype(f), boxes.astype(f)


def masked_runs(seed, A, run=RUN):
    """A padding mask: about a tenth masked at random, plus masked runs across every workgroup edge and at the end."""
    valid = uniform(seed + 3000, A) >= 0.1
    for edge in range(run, A, run):
        valid[max(edge - 3, 0):edge + 2] = False
    if A > 4:
        valid[A - 2:] = False
    return valid


def shape_case(A, G, seed=None, masked=False, labelled=False, **kw):
    seed = A * 7 + G if seed is None else seed
    gt, boxes = scene(seed, A, G)
    return case(gt, boxes, valid=masked_runs(seed, A) if masked else None,
                gt_labels=(uniform(seed + 4000, G) * 5).astype(np.int64) + 1 if labelled else None, **kw)


def far(n, start=500.0):
    """n unit boxes far from everything and from each other."""
    x = start + 3.0 * np.arange(n, dtype=np.float64)
    return np.stack([x, x * 0, x * 0, x + 1, x * 0 + 1, x * 0 + 1], 1)


def cross_workgroup_case(run=RUN):
    """GT 0's row maximum (IoU 1/10, below both thresholds) is attained twice: at the last box of workgroup 0 and the first
    box of workgroup 2.  GT 1 has one partner of IoU 3/20 at box 5.  Every other box has IoU 0 with both.  With low-quality
    matches the three boxes are restored and nothing else is."""
    A = 2 * run + 1
    boxes = far(A)
    boxes[run - 1] = boxes[2 * run] = [0, 0, 0, 10, 1, 1]
    boxes[5] = [0, 10, 0, 20, 11, 1]
    gt = np.asarray([[0, 0, 0, 1, 1, 1], [0, 10, 0, 3, 11, 1]], np.float64)
    return case(gt, boxes, **RPN)


def threshold_boxes():
    """Pairs whose IoU is exactly 7/20, 1/5 and 1/4 (a unit-section bar of length k inside one of length n: k / n), each
    with a neighbour just below: (gt, boxes)."""
    gt, boxes = [], []
    for row, (k, n) in enumerate(((7, 20), (1, 5), (1, 4))):
        y = 10.0 * row
        gt.append([0, y, 0, k, y + 1, 1])
        boxes.append([0, y, 0, n, y + 1, 1])
        boxes.append([0, y, 0, n + 0.001, y + 1, 1])
    return np.asarray(gt), np.asarray(boxes)


def special_cases(run=RUN):
    """name -> case: the named corners of the rule."""
    out = {"cross_workgroup": cross_workgroup_case(run)}
    tg, tb = threshold_boxes()
    out["thresholds_rpn"] = case(tg, tb, **RPN)
    out["thresholds_rpn_strict"] = case(tg, tb, allow=False, **RPN)
    out["thresholds_head"] = case(tg, tb, allow=False, **HEAD)
    # duplicate GT boxes: rows 0 and 3 are the same box, and so are 1, 2 and 4 - the lowest index wins
    gt, boxes = scene(11, 200, 5)
    gt[3], gt[2], gt[4] = gt[0], gt[1], gt[1]
    out["duplicate_gt"] = case(gt, boxes, **RPN)
    # a GT outside every box: its row maximum is 0, and with low-quality matches every box with IoU 0 against it is
    # restored to its arg-max (the reference's quirk)
    gt, boxes = scene(12, 300, 4)
    gt[2] = [900, 900, 900, 905, 905, 905]
    out["gt_outside"] = case(gt, boxes, **RPN)
    out["gt_outside_strict"] = case(gt, boxes, allow=False, **RPN)
    out["masked_edges"] = shape_case(2 * run + 1, 7, seed=13, masked=True, **RPN)
    gt, boxes = scene(14, 130, 3)
    out["all_masked"] = case(gt, boxes, valid=np.zeros(130, bool), **RPN)
    # zero-volume pairs: a point GT and the same point as a box (0 / 0), a flat box inside a GT (0 / volume)
    gt, boxes = scene(15, 70, 3)
    gt[1] = [5, 5, 5, 5, 5, 5]
    boxes[7] = [5, 5, 5, 5, 5, 5]
    boxes[8] = [gt[0][0], gt[0][1], gt[0][2], gt[0][3], gt[0][4], gt[0][2]]
    out["zero_volume"] = case(gt, boxes, **RPN)
    gt, boxes = scene(16, 140, 4)
    gt[1][3] = NAN
    out["nan_gt"] = case(gt, boxes, **RPN)
    gt, boxes = scene(17, 140, 4)
    boxes[9][0] = NAN
    boxes[77][5] = NAN
    out["nan_box"] = case(gt, boxes, valid=masked_runs(17, 140), **RPN)
    gt, boxes = scene(18, 90, 6)
    out["head_labels"] = case(np.concatenate([gt]), np.concatenate([boxes, gt]), gt_labels=[3, 1, 4, 1, 5, 9], **HEAD)
    return out


NAN_CASES = ("zero_volume", "nan_gt", "nan_box")


def fixture_cases():
    """name -> (case, record targets?): what the reference is run on for tests/golden/box_targets.npz."""
    out = {"rpn_small": (shape_case(777, 5, **RPN), True),
           "rpn_masked": (shape_case(1100, 9, masked=True, **RPN), False),
           "rpn_mid": (shape_case(5000, 24, **RPN), False),
           "head": (special_cases()["head_labels"], True)}
    sp = special_cases()
    for name in ("cross_workgroup", "thresholds_rpn", "thresholds_rpn_strict", "thresholds_head", "duplicate_gt", "gt_outside",
                 "all_masked", "masked_edges") + NAN_CASES:
        out[name] = (sp[name], name.startswith("thresholds") or name == "duplicate_gt")
    return out


# ---- the full-size case: the shipped pyramid (run_rcnn.py:37-40,114-121) ---------------------------------------------
FULL_GRID = 160
FULL_G = 24


FULL_SIZES = (8, 16, 32, 64)           # one anchor size per pyramid level of 40^3, 20^3, 10^3, 5^3 cells
FULL_RATIOS = ((1, 1, 1), (1, 1, 2), (1, 2, 2), (1, 1, 3), (1, 3, 3))


def full_size_anchors():
    """fp32 [950 625, 6]: 13 anchors (the distinct axis permutations of FULL_RATIOS, in sorted order per ratio) at every
    cell of the four levels - levels in order, cells with z fastest, the 13 shapes innermost; an anchor is its cell's
    corner (cell index x stride) plus the rounded half extents."""
    import itertools
    shapes = np.asarray([p for r in FULL_RATIOS for p in sorted(set(itertools.permutations(r)))], np.float64)
    out = []
    for size, cells in zip(FULL_SIZES, (40, 20, 10, 5)):
        stride = FULL_GRID // cells
        half = np.round(shapes * size / 2.0)
        base = np.concatenate([-half, half], 1)
        s = np.arange(cells, dtype=np.float64) * stride
        shift = np.stack(np.meshgrid(s, s, s, indexing="ij"), -1).reshape(-1, 3)
        out.append((np.concatenate([shift, shift], 1)[:, None, :] + base[None, :, :]).reshape(-1, 6))
    return np.concatenate(out).astype(f)


def full_size_gt():
    """24 seeded GT boxes inside the 160 grid, sides 10..60."""
    u = uniform(99, FULL_G * 6).reshape(FULL_G, 6)
    side = 10.0 + u[:, 3:] * 50.0
    lo = u[:, :3] * (FULL_GRID - side)
    return np.concatenate([lo, lo + side], 1).astype(f)
