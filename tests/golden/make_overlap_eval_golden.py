"""Golden fixture for the 3-D mask metric (instance_nerf_amd/evaluate.py), produced by running the REFERENCE's own
``mask_iou_3d`` / ``box_iou_3d`` (nerf_rcnn/model/utils.py) and ``evaluate_map_recall`` (nerf_rcnn/eval.py) on small seeded
scenes.

    python tests/golden/make_overlap_eval_golden.py

Runs only where /root/reference exists; packages the image lacks are stubbed as in make_reference_golden.py.  Output:
tests/golden/overlap_eval.npz, data only: per scene the masks (``np.packbits`` of the flattened bool array), boxes, scores
and classes, and what the reference returns - the IoU matrices of every scene with predictions, and (ap, recalls) of the
three-scene call for both IoU types at 0.25 and 0.5, with and without ``top_k``.

The corners the scenes hold (W, L, H = 12, 10, 8):
  scene 0  two predictions on one ground truth (the second is a false positive); a prediction whose best IoU is exactly
           0.5 and one at exactly 0.25 (the reference compares with `<`); class 4 only in the predictions, class 3 only in
           the ground truth; an empty prediction and an empty ground truth of one class (0 / 0 = NaN, which torch's max
           prefers: the empty prediction takes the empty ground truth)
  scene 1  no predictions
  scene 2  an empty prediction with the best score (a false positive), then a good one
Scores are distinct over all scenes: the reference's argsort is not stable.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/nerf_rcnn"
OUT = os.path.dirname(os.path.abspath(__file__))
SHAPE = (12, 10, 8)
TOP_K = 3


def block(lo, hi):
    m = np.zeros(SHAPE, bool)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    return m


def bounds(m):
    """(x1, y1, z1, x2, y2, z2) = min voxel index, max voxel index + 1; zeros for an empty mask."""
    idx = np.argwhere(m)
    if idx.size == 0:
        return np.zeros(6, np.float32)
    return np.concatenate([idx.min(0), idx.max(0) + 1]).astype(np.float32)


def scenes():
    rng = np.random.default_rng(0)
    empty = np.zeros(SHAPE, bool)
    g0, g1, g2, g3 = block((0, 0, 0), (5, 5, 4)), block((6, 0, 0), (10, 4, 4)), block((6, 5, 4), (10, 9, 8)), block((0, 6, 5), (3, 9, 8))
    ragged = g0 & (rng.random(SHAPE) > 0.1)
    out = [dict(gt_masks=[g0, g1, g2, g3, empty], gt_labels=[1, 1, 2, 3, 1],
                masks=[ragged,                                  # 0.90 class 1: most of g0
                       block((0, 0, 0), (5, 5, 3)),            # 0.80 class 1: g0 again, IoU 0.75 - the second one loses
                       block((6, 0, 0), (10, 4, 2)),           # 0.70 class 1: half of g1, IoU exactly 0.5
                       block((6, 5, 4), (10, 9, 5)),           # 0.60 class 2: a quarter of g2, IoU exactly 0.25
                       block((2, 2, 2), (6, 6, 6)),            # 0.50 class 4: a class without ground truth
                       empty,                                  # 0.40 class 1: empty, against the empty ground truth NaN
                       g2 & (rng.random(SHAPE) > 0.5)],        # 0.30 class 2: about half of g2, already taken at 0.25
                scores=[0.90, 0.80, 0.70, 0.60, 0.50, 0.40, 0.30], labels=[1, 1, 1, 2, 4, 1, 2])]
    h0, h1 = block((1, 1, 1), (6, 6, 6)), block((7, 2, 2), (11, 8, 7))
    out.append(dict(gt_masks=[h0, h1], gt_labels=[1, 2], masks=[], scores=[], labels=[]))
    out.append(dict(gt_masks=[h0, h1], gt_labels=[1, 2],
                    masks=[empty, h0 & (rng.random(SHAPE) > 0.2), block((7, 2, 2), (11, 8, 4))],
                    scores=[0.95, 0.85, 0.75], labels=[1, 1, 2]))
    return out


def main():
    for m in ("roi_align", "roi_align.roi_align", "sort_vertices", "wandb", "cv2", "h5py"):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.path.insert(0, REF)
    import eval as ref_eval
    from model import utils as ref_utils

    fixture = {"shape": np.asarray(SHAPE, np.int64), "top_k": np.int64(TOP_K)}
    lists = {k: [] for k in ("masks", "boxes", "scores", "labels", "gt_masks", "gt_boxes", "gt_labels")}
    ran = 0
    for i, sc in enumerate(scenes()):
        masks = np.stack(sc["masks"]) if sc["masks"] else np.zeros((0,) + SHAPE, bool)
        gt_masks = np.stack(sc["gt_masks"])
        boxes = np.stack([bounds(m) for m in masks]) if len(masks) else np.zeros((0, 6), np.float32)
        gt_boxes = np.stack([bounds(m) for m in gt_masks])
        scores = np.asarray(sc["scores"], np.float32)
        labels, gt_labels = np.asarray(sc["labels"], np.int64), np.asarray(sc["gt_labels"], np.int64)
        assert len(set(sc["scores"])) == len(sc["scores"])
        fixture.update({f"s{i}_masks": np.packbits(masks.reshape(-1)), f"s{i}_gt_masks": np.packbits(gt_masks.reshape(-1)),
                        f"s{i}_n": np.asarray([len(masks), len(gt_masks)], np.int64), f"s{i}_boxes": boxes,
                        f"s{i}_gt_boxes": gt_boxes, f"s{i}_scores": scores, f"s{i}_labels": labels,
                        f"s{i}_gt_labels": gt_labels})
        t = dict(masks=torch.from_numpy(masks), boxes=torch.from_numpy(boxes), scores=torch.from_numpy(scores),
                 labels=torch.from_numpy(labels), gt_masks=torch.from_numpy(gt_masks), gt_boxes=torch.from_numpy(gt_boxes),
                 gt_labels=torch.from_numpy(gt_labels))
        for k in lists:
            lists[k].append(t[k])
        if len(masks):
            fixture[f"s{i}_mask_iou"] = ref_utils.mask_iou_3d(t["masks"], t["gt_masks"]).numpy()
            fixture[f"s{i}_box_iou"] = ref_utils.box_iou_3d(t["boxes"], t["gt_boxes"]).numpy()
            assert fixture[f"s{i}_mask_iou"].dtype == np.float32 and fixture[f"s{i}_box_iou"].dtype == np.float32
            ran += 2
    fixture["n_scenes"] = np.int64(len(lists["masks"]))
    assert np.isnan(fixture["s0_mask_iou"][5, 4]) and fixture["s0_mask_iou"][2, 1] == 0.5 and fixture["s0_mask_iou"][3, 2] == 0.25
    for kind in ("mask", "box"):
        pred, gt = (lists["masks"], lists["gt_masks"]) if kind == "mask" else (lists["boxes"], lists["gt_boxes"])
        for thresh, tag in ((0.25, "25"), (0.5, "50")):
            for top_k, ktag in ((None, "all"), (TOP_K, "topk")):
                ap, rec = ref_eval.evaluate_map_recall(pred, lists["scores"], lists["labels"], gt, lists["gt_labels"],
                                                       iou_thresh=thresh, top_k=top_k, iou_type=kind)
                fixture[f"{kind}_{tag}_{ktag}_ap"], fixture[f"{kind}_{tag}_{ktag}_recalls"] = ap.numpy(), rec.numpy()
                ran += 1
    assert ran == 4 + 8, ran                      # every case ran in the reference without an exception
    np.savez_compressed(os.path.join(OUT, "overlap_eval.npz"), **fixture)
    for k in sorted(fixture):
        if k.endswith(("_ap", "_recalls")):
            print(k, fixture[k])
    print("bytes", os.path.getsize(os.path.join(OUT, "overlap_eval.npz")))


if __name__ == "__main__":
    main()
