"""Golden fixture for the detector tail (instance_nerf_amd/detections.py), produced by running the REFERENCE's own
``_do_paste_mask`` / ``paste_masks_in_image`` / ``batched_nms`` / ``clip_boxes_to_mesh`` / ``remove_small_boxes``
(nerf_rcnn/model/utils.py) on the seeded inputs of tests/detections_cases.py.

    python tests/golden/make_detections_golden.py

Runs only where /root/reference exists; packages the image lacks are stubbed as in make_overlap_eval_golden.py.  Output:
tests/golden/detections.npz, data only (the inputs are regenerated from their seeds by the tests):

  <case>_soft       fp32 [N, W, L, H], "small" only: ``_do_paste_mask(skip_empty=False)`` itself
  <case>_bits       ``np.packbits`` of that result ``>= 0.5``, every case
  <case>_cpu_xor    ``np.packbits`` of (``paste_masks_in_image`` on the CPU, i.e. skip_empty=True) XOR the bits above;
  <case>_cpu_flips  how many bits that is.  Where the two paths differ the project follows the whole-volume path.
  nms_keep_<t>      ``batched_nms`` at thresholds 0.2, 0.25 and 0.5
  head_boxes / head_scores / head_labels   the detection rule of nerf_rcnn.py:606-635 (defaults of run_rcnn.py:143-147)
                    driven here by calling the reference's clip_boxes_to_mesh, remove_small_boxes and batched_nms in
                    that order; head_top5_* the same with detections_per_img = 5

The generator asserts that every case ran and that tests/paste_reference.py equals the reference bit for bit.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/nerf_rcnn"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import detections_cases as dc  # noqa: E402
import paste_reference as pr  # noqa: E402


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def head_rule(ru, boxes, scores, shape, score_thresh, nms_thresh, per_img):
    b = ru.clip_boxes_to_mesh(boxes, shape)
    labels = torch.arange(scores.shape[1]).view(1, -1).expand_as(scores)
    b, s, l = b[:, 1:].reshape(-1, 6), scores[:, 1:].reshape(-1), labels[:, 1:].reshape(-1)
    inds = torch.where(s > score_thresh)[0]
    b, s, l = b[inds], s[inds], l[inds]
    keep = ru.remove_small_boxes(b, min_size=1e-2)
    b, s, l = b[keep], s[keep], l[keep]
    keep = ru.batched_nms(b, s, l, nms_thresh)[:per_img]
    return b[keep].numpy(), s[keep].numpy(), l[keep].numpy()


def main():
    for m in ("roi_align", "roi_align.roi_align", "sort_vertices", "wandb", "cv2", "h5py"):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.path.insert(0, REF)
    from model import utils as ru

    fixture, ran = {}, 0
    for name, (masks, boxes, shape) in dc.paste_cases().items():
        tm, tb = torch.from_numpy(masks), torch.from_numpy(boxes)
        mine = pr.paste_soft(masks, boxes, shape)
        if len(masks):
            soft = ru._do_paste_mask(tm[:, None], tb, *shape, skip_empty=False)[0].numpy()
            assert soft.dtype == np.float32 and same_bits(soft, mine), name     # the restatement IS the reference
        else:
            soft = mine
        bits = soft >= np.float32(0.5)
        cpu = ru.paste_masks_in_image(tm, tb, tuple(shape), 0.5).numpy().astype(bool).reshape(bits.shape)
        if name == "small":
            fixture[f"{name}_soft"] = soft
        fixture[f"{name}_bits"] = np.packbits(bits.reshape(-1))
        fixture[f"{name}_cpu_xor"] = np.packbits((cpu ^ bits).reshape(-1))
        fixture[f"{name}_cpu_flips"] = np.int64((cpu ^ bits).sum())
        print(name, shape, "set", int(bits.sum()), "cpu path differs in", int((cpu ^ bits).sum()),
              "within 1e-6 of 0.5:", int((np.abs(soft - 0.5) < 1e-6).sum()))
        ran += 1
    boxes, scores, classes = dc.nms_case()
    assert len(set(scores.tolist())) == len(scores)
    for t in (0.2, 0.25, 0.5):
        keep = ru.batched_nms(torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(classes), t).numpy()
        assert np.array_equal(keep, pr.batched_nms(boxes, scores, classes, t)), t
        fixture[f"nms_keep_{t}"] = keep.astype(np.int64)
        ran += 1
    n = len(boxes)
    k2 = set(fixture["nms_keep_0.2"].tolist())
    assert {n - 6, n - 5} <= k2 and {n - 4, n - 3} <= k2 and len({n - 2, n - 1} & k2) == 1       # the named corners
    assert {n - 2, n - 1} <= set(fixture["nms_keep_0.25"].tolist())
    hb, hs, shape = dc.head_case()
    for tag, per in (("head", 100), ("head_top5", 5)):
        b, s, l = head_rule(ru, torch.from_numpy(hb), torch.from_numpy(hs), shape, 0.01, 0.2, per)
        fixture[f"{tag}_boxes"], fixture[f"{tag}_scores"], fixture[f"{tag}_labels"] = b, s, l.astype(np.int64)
        ran += 1
    assert ran == 4 + 3 + 2, ran                  # every case ran in the reference without an exception
    path = os.path.join(OUT, "detections.npz")
    np.savez_compressed(path, **fixture)
    print("head rule kept", len(fixture["head_boxes"]), "nms kept", {k: len(v) for k, v in fixture.items() if k.startswith("nms")})
    print("bytes", os.path.getsize(path))
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
