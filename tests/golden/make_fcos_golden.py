"""Golden fixture for the FCOS training targets and losses (instance_nerf_amd/fcos.py, csrc/fcos.hip), produced by running
the REFERENCE's own ``FCOSLossComputation.prepare_targets``, ``compute_centerness_targets`` and ``__call__``
(nerf_rcnn/model/fcos/loss.py) on the CPU, on the seeded inputs of tests/fcos_cases.py.

    python tests/golden/make_fcos_golden.py

Runs only where /root/reference exists.  The modules that file imports and this image lacks are stubbed: its oriented-box
helpers (never called for axis-aligned boxes) and ``torchvision.ops.sigmoid_focal_loss``, which is supplied as a
restatement of its published formula - so the focal term is pinned to the FORMULA, not to a reference run; everything else
in the three losses is the reference's own arithmetic.  Output: tests/golden/fcos.npz, data only (inputs are regenerated
from their seeds by the tests):

  <case>_matched     int16 [T]   the chosen ground-truth index per location, level-first (0 in a scene without boxes)
  <case>_labels      int8 [T]    prepare_targets' labels
  <case>_reg_sha256  the sha256 of the bytes of prepare_targets' regression targets (float32 [T, 6], levels concatenated)
  <case>_ctr_sha256  the sha256 of compute_centerness_targets at the positives (float32, level-first order)
  <case>_losses      float32 [3 loss types, 2, 3]: (cls, reg, centerness) of __call__ for iou / linear_iou / giou, without
                     and with padding masks; main cases only

The generator asserts that every case ran, that tests/fcos_reference.py equals the reference bit for bit on every case,
that each multi-level case has a positive on EVERY level, that at least one location has two equal smallest volumes and
that at least one location lies exactly on a box face.
"""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/nerf_rcnn"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
import fcos_cases as fc  # noqa: E402
import fcos_reference as fr  # noqa: E402


def sigmoid_focal_loss(inputs, targets, alpha=0.25, gamma=2, reduction="none"):
    """torchvision.ops.sigmoid_focal_loss as published (torchvision/ops/focal_loss.py)."""
    p = torch.sigmoid(inputs)
    ce_loss = torch.nn.functional.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce_loss * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss.sum() if reduction == "sum" else (loss.mean() if reduction == "mean" else loss)


def reference_loss_module():
    def stub(name, **names):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in names.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m
    never = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("oriented boxes are not part of this fixture"))  # noqa: E731
    stub("torchvision")
    stub("torchvision.ops", sigmoid_focal_loss=sigmoid_focal_loss)
    stub("refmodel")
    stub("refmodel.fcos")
    stub("refmodel.rotated_iou")
    stub("refmodel.rotated_iou.oriented_iou_loss", cal_iou_3d=never, cal_giou_3d=never, cal_diou_3d=never, box2corners_th=never)
    stub("refmodel.fcos.utils", decode_fcos_obb=never, encode_fcos_obb=never, get_w2cs=never, obb2points_3d=never, project=never)
    spec = importlib.util.spec_from_file_location("refmodel.fcos.loss", os.path.join(REF, "model", "fcos", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["refmodel.fcos.loss"] = mod
    spec.loader.exec_module(mod)
    return mod


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def main():
    ref = reference_loss_module()
    from instance_nerf_amd import fcos
    fixture, ran = {}, 0
    any_tie = any_face = False
    for name, c in fc.fixture_cases().items():
        shapes, strides, B = c["shapes"], c["strides"], len(c["gts"])
        comp = ref.FCOSLossComputation(strides, c["radius"], "iou", c["norm"], 1, False, False)
        locs = fcos.compute_locations(shapes, strides)
        gts = [torch.from_numpy(g) for g in c["gts"]]
        labels, reg = comp.prepare_targets(locs, gts)
        labels, reg = torch.cat(labels).numpy(), torch.cat(reg).numpy()
        mine = fr.targets(shapes, strides, c["gts"], c["radius"], c["norm"], ori_sizes=c["ori_sizes"])
        assert labels.dtype == np.float32 and fr.same(mine["labels"], labels), name
        assert fr.same(mine["reg"], reg), name                                  # the restatement IS the reference
        pos = labels > 0
        ctr = comp.compute_centerness_targets(torch.from_numpy(reg[pos])).numpy()
        assert fr.same(mine["centerness"][pos], ctr), name
        for l in range(len(shapes)):
            assert len(shapes) == 1 or ((mine["level"] == l) & pos).any(), (name, "no positive on level", l)
        any_tie, any_face = any_tie or bool(mine["ties"].any()), any_face or bool(mine["on_face"].any())
        # the locations and masks of the reference's fcos.py:221-265 are three lines each; fcos.py restates them and
        # tests/fcos_reference.py does so independently
        assert all(np.array_equal(a.numpy(), b) for a, b in zip(locs, fr.locations(shapes, strides)))
        fixture[f"{name}_matched"] = mine["matched"].astype(np.int16)
        fixture[f"{name}_labels"] = labels.astype(np.int8)
        fixture[f"{name}_reg_sha256"] = sha(reg)
        fixture[f"{name}_ctr_sha256"] = sha(ctr)
        print(name, "T", len(labels), "positives", int(pos.sum()), "ties", int(mine["ties"].sum()), "on a face",
              int(mine["on_face"].sum()))
        if c["ori_sizes"] is not None:
            cls, breg, bctr = [[torch.from_numpy(a) for a in arrs] for arrs in fc.predictions(7, shapes, B)]
            masks = fcos.compute_padding_masks(locs, c["ori_sizes"])
            assert np.array_equal(torch.cat([m.reshape(-1) for m in masks]).numpy(), mine["valid"])
            out = np.zeros((3, 2, 3), np.float32)
            for i, lt in enumerate(fc.LOSS_TYPES):
                comp = ref.FCOSLossComputation(strides, c["radius"], lt, c["norm"], 1, False, False)
                for j, m in enumerate((None, masks)):
                    out[i, j] = [float(v) for v in comp(locs, cls, breg, bctr, gts, m)]
            assert np.isfinite(out).all() and (out > 0).all(), out
            fixture[f"{name}_losses"] = out
            print(name, "losses", out.reshape(-1).tolist())
        ran += 1
    assert ran == len(fc.fixture_cases()) == 4, ran
    assert any_tie, "no location with two equal smallest volumes"
    assert any_face, "no location exactly on a box face"
    path = os.path.join(OUT, "fcos.npz")
    np.savez_compressed(path, **fixture)
    print("bytes", os.path.getsize(path))
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
