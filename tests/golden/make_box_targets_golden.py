"""Golden fixture for the detector's training targets (instance_nerf_amd/targets.py, csrc/assign.hip), produced by
running the REFERENCE's own ``RegionProposalNetwork.assign_targets_to_anchors``, ``Matcher``, ``batched_box_iou`` and
``AABBCoder.encode_single`` on the seeded inputs of tests/box_targets_cases.py.

    python tests/golden/make_box_targets_golden.py

Runs only where /root/reference exists; packages the image lacks are stubbed as in make_detections_golden.py.  Output:
tests/golden/box_targets.npz, data only (the inputs are regenerated from their seeds by the tests):

  <case>_matched   int16 [A]  the Matcher's result (-1 below, -2 between the thresholds)
  <case>_labels    int8 [A]   RPN cases: assign_targets_to_anchors' labels (1 / 0 / -1); the head case: the labels of
                              nerf_rcnn.py:464-498 - that module needs torchvision, so the reference's batched_box_iou and
                              Matcher are driven here and only the indexing lines are restated
  <case>_boxes     fp32 [A, 6] the matched GT boxes
  <case>_targets   fp32 [A, 6] AABBCoder().encode_single(matched boxes, boxes), small cases only
  full_counts      int64 [3]  foreground / ignored / background anchors of the full-size case: the shipped pyramid of
                              950 625 anchors (built by the reference's AnchorGenerator3D; the anchors of
                              box_targets_cases.full_size_anchors are asserted to be the same boxes in the same order)
                              against 24 seeded GT boxes at the RPN's thresholds
  full_sha256      the sha256 of that case's int64 matched indices, as bytes

The generator asserts that every case ran, that tests/box_targets_reference.py equals the reference bit for bit (NaN for
NaN) on every small case, and that targets.py's composable path equals it at full size.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/nerf_rcnn"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
import box_targets_cases as bc  # noqa: E402
import box_targets_reference as br  # noqa: E402


def rpn_assign(rpn_cls, ru, case, anchors=None):
    """The reference's assign_targets_to_anchors, unbound, on a namespace that carries what it reads."""
    ns = types.SimpleNamespace(box_similarity=ru.batched_box_iou, iou_batch_size=16,
                               proposal_matcher=ru.Matcher(case["high"], case["low"], allow_low_quality_matches=case["allow"]))
    boxes = torch.from_numpy(case["boxes"]) if anchors is None else anchors
    masks = None if case["valid"] is None else [torch.from_numpy(case["valid"])]
    labels, matched_boxes = rpn_cls.assign_targets_to_anchors(ns, [boxes], [torch.from_numpy(case["gt"])], masks)
    return labels[0], matched_boxes[0]


def matched_of(ru, case, boxes=None):
    q = ru.batched_box_iou(torch.from_numpy(case["gt"]), torch.from_numpy(case["boxes"]) if boxes is None else boxes, 16)
    if case["valid"] is not None:
        q[:, ~torch.from_numpy(case["valid"])] = -1.0
    return ru.Matcher(case["high"], case["low"], allow_low_quality_matches=case["allow"])(q)


def main():
    for m in ("roi_align", "roi_align.roi_align", "sort_vertices", "wandb", "cv2", "h5py"):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.path.insert(0, REF)
    from model import utils as ru
    from model.rpn import RegionProposalNetwork
    from model.coder.AABB_coder import AABBCoder
    from model.anchor import AnchorGenerator3D
    from instance_nerf_amd import targets

    fixture, ran = {}, 0
    for name, (case, with_targets) in bc.fixture_cases().items():
        gt, boxes = torch.from_numpy(case["gt"]), torch.from_numpy(case["boxes"])
        matched = matched_of(ru, case)
        if case["gt_labels"] is None:
            labels, mboxes = rpn_assign(RegionProposalNetwork, ru, case)
            assert labels.dtype == torch.float32
        else:                                              # nerf_rcnn.py:483-494, restated
            clamped = matched.clamp(min=0)
            labels = torch.from_numpy(case["gt_labels"])[clamped].to(torch.int64)
            labels[matched == -1] = 0
            labels[matched == -2] = -1
            mboxes = gt[clamped]
        enc = AABBCoder().encode_single(mboxes, boxes)
        mine = br.assign(**case)
        assert np.array_equal(mine["matched"], matched.numpy()), name
        assert np.array_equal(mine["labels"], labels.numpy().astype(np.int64)), name
        assert br.same(mine["matched_boxes"], mboxes.numpy()), name
        assert br.same(mine["targets"], enc.numpy()), name                # the restatement IS the reference
        assert -32768 <= int(matched.min()) and int(matched.max()) < 32768
        fixture[f"{name}_matched"] = matched.numpy().astype(np.int16)
        fixture[f"{name}_labels"] = labels.numpy().astype(np.int8)
        fixture[f"{name}_boxes"] = mboxes.numpy()
        if with_targets:
            fixture[f"{name}_targets"] = enc.numpy()
        m = matched.numpy()
        print(name, "A", len(m), "G", len(gt), "matched", int((m >= 0).sum()), "between", int((m == -2).sum()),
              "below", int((m == -1).sum()), "NaN targets", int(np.isnan(enc.numpy()).sum()))
        ran += 1
    assert ran == len(bc.fixture_cases()) == 15, ran

    # ---- the full-size case
    gen = AnchorGenerator3D(((8,), (16,), (32,), (64,)),
                            (((1., 1., 1.), (1., 1., 2.), (1., 2., 2.), (1., 1., 3.), (1., 3., 3.)),) * 4)
    feats = [torch.zeros(1, 1, n, n, n) for n in (40, 20, 10, 5)]
    ref_anchors = gen(torch.zeros(1, 1, bc.FULL_GRID, bc.FULL_GRID, bc.FULL_GRID), feats)[0][0]
    anchors = bc.full_size_anchors()
    assert ref_anchors.shape == (950625, 6) and ref_anchors.dtype == torch.float32
    same_set = np.array_equal(np.unique(ref_anchors.numpy(), axis=0), np.unique(anchors, axis=0))
    assert same_set, "box_targets_cases.full_size_anchors are not the reference's anchors"
    in_order = np.array_equal(ref_anchors.numpy(), anchors)
    print("full-size anchors: the same boxes;", "the same order" if in_order else "another order of the 13 shapes per cell")
    case = bc.case(bc.full_size_gt(), anchors, **bc.RPN)
    labels, mboxes = rpn_assign(RegionProposalNetwork, ru, case)
    matched = matched_of(ru, case).numpy()
    lab = labels.numpy()
    counts = np.asarray([(lab == 1).sum(), (lab == -1).sum(), (lab == 0).sum()], np.int64)
    assert np.array_equal(counts, [(matched >= 0).sum(), (matched == -2).sum(), (matched == -1).sum()])
    mine = targets.match_boxes(torch.from_numpy(case["gt"]), torch.from_numpy(anchors), 0.35, 0.2, True, fused=False)
    assert np.array_equal(mine.numpy(), matched)
    l2, b2 = targets.assign_targets_to_anchors([torch.from_numpy(anchors)], [torch.from_numpy(case["gt"])], 0.35, 0.2)
    assert torch.equal(l2[0], labels) and torch.equal(b2[0], mboxes)
    fixture["full_counts"] = counts
    fixture["full_sha256"] = np.frombuffer(hashlib.sha256(matched.astype(np.int64).tobytes()).digest(), np.uint8)
    print("full size: foreground / ignored / background", counts.tolist())

    path = os.path.join(OUT, "box_targets.npz")
    np.savez_compressed(path, **fixture)
    print("bytes", os.path.getsize(path))
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
