"""Shared by tests/test_evaluate_cpu.py and tests/test_evaluate.py: the golden fixture of the reference's own run
(tests/golden/overlap_eval.npz, written by tests/golden/make_overlap_eval_golden.py), a brute-force count in numpy, and the
checks both paths of instance_nerf_amd/evaluate.py have to pass."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap_eval.npz")
_cache = {}


def golden():
    """-> (raw npz dict, list of per-scene dicts of numpy arrays); loaded once."""
    if "g" not in _cache:
        z = dict(np.load(GOLDEN))
        shape = tuple(int(v) for v in z["shape"])
        V = int(np.prod(shape))
        scenes = []
        for i in range(int(z["n_scenes"])):
            n, m = (int(v) for v in z[f"s{i}_n"])
            def unpack(key, k):
                return np.unpackbits(z[key])[:k * V].astype(bool).reshape((k,) + shape)
            scenes.append({"masks": unpack(f"s{i}_masks", n), "gt_masks": unpack(f"s{i}_gt_masks", m),
                           **{k: z[f"s{i}_{k}"] for k in ("boxes", "gt_boxes", "scores", "labels", "gt_labels")}})
        _cache["g"] = (z, scenes)
    return _cache["g"]


def brute_counts(a, b):
    """bool [n, ...], [m, ...] -> (inter int64 [n, m], area_a [n], area_b [m]) one pair at a time."""
    V = int(np.prod(np.shape(a)[1:]))
    a, b = np.asarray(a).astype(bool).reshape(len(a), V), np.asarray(b).astype(bool).reshape(len(b), V)
    inter = np.zeros((len(a), len(b)), np.int64)
    for i in range(len(a)):
        for j in range(len(b)):
            inter[i, j] = np.count_nonzero(a[i] & b[j])
    return inter, a.sum(1).astype(np.int64), b.sum(1).astype(np.int64)


def brute_iou(inter, a1, a2):
    """The reference's arithmetic in numpy: both integers to fp32, fp32 division (0 / 0 = NaN)."""
    union = a1[:, None] + a2[None, :] - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter.astype(np.float32) / union.astype(np.float32)


def same_bits(x, y):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return x.shape == y.shape and np.array_equal(x.view(np.uint32)[~np.isnan(x)], y.view(np.uint32)[~np.isnan(y)]) \
        and np.array_equal(np.isnan(x), np.isnan(y))


def check_golden(device, fused):
    """The fixture through instance_nerf_amd.evaluate on `device`: IoU matrices bit-equal, ap / recalls equal with NaNs
    in the same places."""
    from instance_nerf_amd import evaluate as ev
    z, scenes = golden()
    dev = torch.device(device)
    t = [{k: torch.from_numpy(v).to(dev) for k, v in s.items()} for s in scenes]
    for i, s in enumerate(t):
        if len(s["masks"]) == 0:
            continue
        iou = ev.mask_iou_3d(s["masks"], s["gt_masks"], fused=fused)
        assert iou.dtype == torch.float32 and iou.device.type == dev.type
        assert same_bits(iou.cpu().numpy(), z[f"s{i}_mask_iou"]), (i, iou, z[f"s{i}_mask_iou"])
        assert same_bits(ev.box_iou_3d(s["boxes"], s["gt_boxes"]).cpu().numpy(), z[f"s{i}_box_iou"]), i
    top = int(z["top_k"])
    for kind, pk, gk in (("mask", "masks", "gt_masks"), ("box", "boxes", "gt_boxes")):
        for thresh, tag in ((0.25, "25"), (0.5, "50")):
            for top_k, ktag in ((None, "all"), (top, "topk")):
                ap, rec = ev.evaluate_map_recall([s[pk] for s in t], [s["scores"] for s in t], [s["labels"] for s in t],
                                                 [s[gk] for s in t], [s["gt_labels"] for s in t], iou_thresh=thresh,
                                                 top_k=top_k, iou_type=kind, fused=fused)
                name = f"{kind}_{tag}_{ktag}"
                assert ap.dtype == torch.float32 and rec.dtype == torch.float32
                assert np.array_equal(ap.numpy(), z[name + "_ap"], equal_nan=True), (name, ap, z[name + "_ap"])
                assert np.array_equal(rec.numpy(), z[name + "_recalls"], equal_nan=True), (name, rec, z[name + "_recalls"])


def random_masks(rng, k, V, density):
    return rng.random((k, V)) < density


def as_volume(flat, V):
    """[k, V] -> [k, V, 1, 1]: any factorisation of V is the same flattened volume."""
    return flat.reshape(flat.shape[0], V, 1, 1)
