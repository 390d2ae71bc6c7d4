"""Training targets of the detector heads: which ground-truth box every anchor (RPN) or proposal (RoI heads) is trained
against, the regression targets of the box coder and the balanced sampler - what every training step of the reference's
detector starts with (nerf_rcnn/model/rpn.py:240-290,524, nerf_rcnn.py:464-498; Matcher, BalancedPositiveNegativeSampler
and batched_box_iou of model/utils.py:37-214,375-462; coder/AABB_coder.py).

Two paths give the same result:

  fused       GPU float32 boxes, 1 <= G <= 1024 ground-truth boxes: two launches of csrc/assign.hip (include/inr.h,
              "Detector training targets").  The [G, A] quality matrix is never built; nothing is read back.
  composable  everything else (CPU tensors, other float types, G > 1024, ``fused=False``): the reference's chunked IoU
              matrix followed by ``Matcher``, restated in plain torch.

Axis-aligned boxes only, rows (x1, y1, z1, x2, y2, z2); 7-number oriented boxes raise ValueError as elsewhere in the
project.  The detector networks and their losses are not part of this package."""
import math

import torch

from . import _lib
from .evaluate import box_iou_3d

BOX_MATCH_MAX_GT = _lib.BOX_MATCH_MAX_GT
# profiles/box_match_probe.json (tools/box_match_probe.py): the fused assignment is faster than the composable path on the
# same GPU inputs in every measured shape (x3.2 for the head's 2 524 proposals, x7.3 ... x8.7 at the shipped 950 625
# anchors), so fused=None takes the kernels; a shape that loses there sends the default back to the composable path
MATCH_FUSED_BY_DEFAULT = True


class Matcher:
    """The reference's Matcher (model/utils.py:100-214) on any [G, A] quality matrix: the index of the best ground-truth
    element per column, -1 (BELOW_LOW_THRESHOLD) where the best quality is below ``low_threshold``, -2
    (BETWEEN_THRESHOLDS) in [low, high); with ``allow_low_quality_matches`` every column that attains a row's maximum gets
    its arg-max back.  The matrix is not modified."""
    BELOW_LOW_THRESHOLD = -1
    BETWEEN_THRESHOLDS = -2

    def __init__(self, high_threshold, low_threshold, allow_low_quality_matches=False):
        if not low_threshold <= high_threshold:
            raise ValueError("low_threshold should be <= high_threshold")
        self.high_threshold = high_threshold
        self.low_threshold = low_threshold
        self.allow_low_quality_matches = allow_low_quality_matches

    def __call__(self, match_quality_matrix):
        q = match_quality_matrix
        if q.numel() == 0:
            if q.shape[0] == 0:
                raise ValueError("No ground-truth boxes available for one of the images during training")
            raise ValueError("No proposal boxes available for one of the images during training")
        matched_vals, matches = q.max(dim=0)
        all_matches = matches.clone() if self.allow_low_quality_matches else None
        below = matched_vals < self.low_threshold
        between = (matched_vals >= self.low_threshold) & (matched_vals < self.high_threshold)
        matches = torch.where(below, torch.full_like(matches, self.BELOW_LOW_THRESHOLD), matches)
        matches = torch.where(between, torch.full_like(matches, self.BETWEEN_THRESHOLDS), matches)
        if self.allow_low_quality_matches:
            # the reference gathers the (gt, column) pairs with torch.where - a read-back of a data-dependent size - and
            # writes all_matches back at those columns; the same set of columns as a mask
            highest, _ = q.max(dim=1)
            restore = (q == highest[:, None]).any(dim=0)
            matches = torch.where(restore, all_matches, matches)
        return matches


def _boxes(t, name):
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] not in (6, 7):
        raise ValueError(f"{name} must be a tensor [N, 6] of boxes (x1, y1, z1, x2, y2, z2)")
    if t.shape[1] == 7:
        raise ValueError(f"{name}: oriented boxes (7 numbers) are not supported")
    if not t.is_floating_point():
        raise ValueError(f"{name} must be floating point, got {t.dtype}")
    return t.detach()


def batched_box_iou(boxes1, boxes2, batch_size=16):
    """The reference's chunked IoU matrix (model/utils.py:375-388): ``box_iou_3d`` on ``batch_size`` rows of ``boxes1``
    at a time, concatenated -> [len(boxes1), len(boxes2)]."""
    n = boxes1.shape[0]
    if n == 0:
        return box_iou_3d(boxes1, boxes2)
    return torch.cat([box_iou_3d(boxes1[i:i + batch_size], boxes2) for i in range(0, n, batch_size)], dim=0)


def encode_boxes(reference_boxes, proposals):
    """Regression targets [N, 6] of ``proposals`` against ``reference_boxes`` (coder/AABB_coder.py:7-56): the centre
    offsets in units of the proposal's sides, then the logs of the side ratios, in the reference's operation order."""
    r, p = _boxes(reference_boxes, "reference_boxes"), _boxes(proposals, "proposals")
    ex = p[:, 3:] - p[:, :3]
    ex_ctr = p[:, :3] + 0.5 * ex
    gt = r[:, 3:] - r[:, :3]
    gt_ctr = r[:, :3] + 0.5 * gt
    return torch.cat(((gt_ctr - ex_ctr) / ex, torch.log(gt / ex)), dim=1)


def decode_boxes(rel_codes, boxes, bbox_xform_clip=math.log(2000.0)):
    """Boxes [N, 6 k] from ``rel_codes`` [N, 6 k] relative to ``boxes`` [N, 6] (AABBCoder.decode_single): the inverse of
    ``encode_boxes`` with the size terms clamped at ``bbox_xform_clip`` before the exponential."""
    boxes = _boxes(boxes, "boxes").to(rel_codes.dtype)
    if rel_codes.dim() != 2 or rel_codes.shape[1] % 6 != 0 or rel_codes.shape[0] != boxes.shape[0]:
        raise ValueError(f"rel_codes must be [N, 6 k] with N = {boxes.shape[0]}, got {tuple(rel_codes.shape)}")
    size = boxes[:, 3:] - boxes[:, :3]
    ctr = boxes[:, :3] + 0.5 * size
    codes = rel_codes.reshape(rel_codes.shape[0], -1, 6)
    pred_ctr = codes[..., :3] * size[:, None] + ctr[:, None]
    pred_size = torch.exp(torch.clamp(codes[..., 3:], max=bbox_xform_clip)) * size[:, None]
    half = torch.tensor(0.5, dtype=pred_size.dtype, device=pred_size.device) * pred_size
    return torch.cat((pred_ctr - half, pred_ctr + half), dim=-1).flatten(1)


# ---- the assignment ------------------------------------------------------------------------------------------------------
def _kernel_takes(gt, boxes):
    return (gt.is_cuda and boxes.is_cuda and gt.dtype == torch.float32 and boxes.dtype == torch.float32
            and 1 <= gt.shape[0] <= BOX_MATCH_MAX_GT and boxes.shape[0] * 6 < 2 ** 31)


def _use_kernel(gt, boxes, fused):
    takes = _kernel_takes(gt, boxes)
    if fused and not takes:
        raise RuntimeError(f"the fused matcher takes float32 GPU boxes with 1..{BOX_MATCH_MAX_GT} ground-truth boxes (got "
                           f"{gt.dtype} {tuple(gt.shape)} on {gt.device}, {boxes.dtype} {tuple(boxes.shape)} on "
                           f"{boxes.device}); fused=None picks the composable path")
    return takes and (fused or (fused is None and MATCH_FUSED_BY_DEFAULT))


def _check_pair(gt, boxes, valid):
    if gt.shape[0] == 0:
        raise ValueError("No ground-truth boxes available for one of the images during training")
    if boxes.shape[0] == 0:
        raise ValueError("No proposal boxes available for one of the images during training")
    if gt.device != boxes.device:
        raise ValueError(f"gt_boxes are on {gt.device}, boxes on {boxes.device}")
    if valid is not None and (valid.dtype != torch.bool or valid.shape != boxes.shape[:1] or valid.device != boxes.device):
        raise ValueError(f"valid must be a bool tensor [{boxes.shape[0]}] on {boxes.device}")


def _match_fused(gt, boxes, valid, high, low, allow, gt_labels=None, labels=False, best=False, matched_boxes=False,
                 targets=False):
    """The two launches.  -> dict with "matched" (int32 [A]) and the requested optional outputs of include/inr.h."""
    lib = _lib.load()
    G, A = gt.shape[0], boxes.shape[0]
    dev = boxes.device
    gt, boxes = gt.contiguous(), boxes.contiguous()
    vbytes = valid.contiguous().view(torch.uint8) if valid is not None else None
    lab32 = gt_labels.to(torch.int32).contiguous() if gt_labels is not None else None
    keys = torch.empty((G,), dtype=torch.int32, device=dev)
    out = {"matched": torch.empty((A,), dtype=torch.int32, device=dev),
           "labels": torch.empty((A,), dtype=torch.int32, device=dev) if labels else None,
           "best_iou": torch.empty((A,), dtype=torch.float32, device=dev) if best else None,
           "matched_boxes": torch.empty((A, 6), dtype=torch.float32, device=dev) if matched_boxes else None,
           "targets": torch.empty((A, 6), dtype=torch.float32, device=dev) if targets else None}
    with torch.cuda.device(dev):
        s = _lib.stream_ptr()
        gp, bp, vp, kp = _lib.ptr(gt, torch.float32, "gt_boxes"), _lib.ptr(boxes, torch.float32, "boxes"), \
            _lib.ptr(vbytes, torch.uint8, "valid", allow_none=True), _lib.ptr(keys, torch.int32, "keys")
        _lib.check(lib.inr_box_match_gt_max(gp, G, bp, vp, A, kp, s), "box_match_gt_max")
        _lib.check(lib.inr_box_match_assign(gp, _lib.ptr(lab32, torch.int32, "gt_labels", allow_none=True), G, bp, vp, A, kp,
                                            float(high), float(low), int(bool(allow)),
                                            _lib.ptr(out["matched"], torch.int32, "matched"),
                                            _lib.ptr(out["labels"], torch.int32, "labels", allow_none=True),
                                            _lib.ptr(out["best_iou"], torch.float32, "best_iou", allow_none=True),
                                            _lib.ptr(out["matched_boxes"], torch.float32, "matched_boxes", allow_none=True),
                                            _lib.ptr(out["targets"], torch.float32, "targets", allow_none=True), s),
                   "box_match_assign")
    return out


def _match_composable(gt, boxes, valid, high, low, allow, iou_batch_size=16):
    q = batched_box_iou(gt, boxes, iou_batch_size)
    if valid is not None:
        q = torch.where(valid[None, :], q, torch.full_like(q, -1.0))      # the reference's matrix[:, ~mask] = -1.0
    return Matcher(high, low, allow)(q)


def match_boxes(gt_boxes, boxes, high_threshold, low_threshold, allow_low_quality_matches=False, valid=None, fused=None):
    """-> int64 [A]: ``Matcher(high, low, allow)`` on the IoU matrix of ``gt_boxes`` [G, 6] and ``boxes`` [A, 6] - the
    index of the matched ground-truth box, -1 below ``low_threshold``, -2 between the thresholds.  ``valid``: bool [A],
    the padding mask (False: the box's qualities are -1).  ``fused``: None picks the kernels where they apply (module
    docstring), True insists on them (RuntimeError otherwise), False is the composable path.  Both follow the same rule;
    where the arg-max itself is in question (ties, NaN) the kernels follow torch's CPU rule - lowest index among equals, a
    NaN above every number - while ``torch.max`` on a GPU may pick another index."""
    gt, boxes = _boxes(gt_boxes, "gt_boxes"), _boxes(boxes, "boxes")
    if not low_threshold <= high_threshold:
        raise ValueError("low_threshold should be <= high_threshold")
    _check_pair(gt, boxes, valid)
    if _use_kernel(gt, boxes, fused):
        return _match_fused(gt, boxes, valid, high_threshold, low_threshold, allow_low_quality_matches)["matched"].long()
    return _match_composable(gt, boxes, valid, high_threshold, low_threshold, allow_low_quality_matches)


def assign_targets_to_anchors(anchors, gt_boxes, fg_iou_thresh, bg_iou_thresh, padding_masks=None, iou_batch_size=16,
                              encode=False, fused=None):
    """The RPN's assignment (model/rpn.py:240-290), per scene: ``anchors`` and ``gt_boxes`` are lists of [A_i, 6] and
    [G_i, 6]; ``padding_masks``: list of bool [A_i] (False: a padded anchor).  -> (labels, matched_gt_boxes) - lists of
    float32 [A_i] (1 foreground, 0 background, -1 ignored: between the thresholds or padded) and [A_i, 6] - plus the list
    of regression targets ``encode_boxes(matched_gt_boxes, anchors)`` when ``encode`` (rpn.py:524).  Low-quality matches
    are allowed, as in the reference's RPN.  A scene without ground truth gives zeros."""
    labels, matched_gt, reg = [], [], []
    for i, (a, g) in enumerate(zip(anchors, gt_boxes)):
        a = _boxes(a, "anchors")
        valid = padding_masks[i] if padding_masks is not None else None
        if g.numel() == 0:
            m = torch.zeros(a.shape, dtype=torch.float32, device=a.device)
            l = torch.zeros((a.shape[0],), dtype=torch.float32, device=a.device)
            if valid is not None:
                l = torch.where(valid, l, torch.full_like(l, -1.0))
            t = encode_boxes(m, a) if encode else None
        else:
            g = _boxes(g, "gt_boxes")
            _check_pair(g, a, valid)
            if _use_kernel(g, a, fused):
                out = _match_fused(g, a, valid, fg_iou_thresh, bg_iou_thresh, True, labels=True, matched_boxes=True,
                                   targets=encode)
                l, m, t = out["labels"].float(), out["matched_boxes"], out["targets"]
            else:
                idx = _match_composable(g, a, valid, fg_iou_thresh, bg_iou_thresh, True, iou_batch_size)
                m = g[idx.clamp(min=0)]
                l = (idx >= 0).to(torch.float32)
                l = torch.where(idx == Matcher.BETWEEN_THRESHOLDS, torch.full_like(l, -1.0), l)
                if valid is not None:
                    l = torch.where(valid, l, torch.full_like(l, -1.0))
                t = encode_boxes(m, a) if encode else None
        labels.append(l)
        matched_gt.append(m)
        reg.append(t)
    return (labels, matched_gt, reg) if encode else (labels, matched_gt)


def assign_targets_to_proposals(proposals, gt_boxes, gt_labels, fg_iou_thresh, bg_iou_thresh, fused=None):
    """The RoI heads' assignment (nerf_rcnn.py:464-498), per scene -> (matched_idxs, labels), lists of int64 [A_i]: the
    matched ground-truth index clamped at 0, and ``gt_labels`` of it - 0 for background (below ``bg_iou_thresh``), -1 for
    proposals between the thresholds, which the sampler ignores.  Low-quality matches are allowed, as the reference's
    head constructs its matcher.  A scene without ground truth gives zeros."""
    matched, labels = [], []
    for p, g, gl in zip(proposals, gt_boxes, gt_labels):
        p = _boxes(p, "proposals")
        if g.numel() == 0:
            idx = torch.zeros((p.shape[0],), dtype=torch.int64, device=p.device)
            l = torch.zeros((p.shape[0],), dtype=torch.int64, device=p.device)
        else:
            g = _boxes(g, "gt_boxes")
            _check_pair(g, p, None)
            if gl.shape != g.shape[:1] or gl.dtype.is_floating_point:
                raise ValueError(f"gt_labels must be integers [{g.shape[0]}], got {gl.dtype} {tuple(gl.shape)}")
            if _use_kernel(g, p, fused):
                out = _match_fused(g, p, None, fg_iou_thresh, bg_iou_thresh, True, gt_labels=gl, labels=True)
                idx, l = out["matched"].clamp(min=0).long(), out["labels"].long()
            else:
                m = _match_composable(g, p, None, fg_iou_thresh, bg_iou_thresh, True)
                idx = m.clamp(min=0)
                l = gl[idx].to(torch.int64)
                l = torch.where(m == Matcher.BELOW_LOW_THRESHOLD, torch.zeros_like(l), l)
                l = torch.where(m == Matcher.BETWEEN_THRESHOLDS, torch.full_like(l, -1), l)
        matched.append(idx)
        labels.append(l)
    return matched, labels


# ---- the sampler ---------------------------------------------------------------------------------------------------------
def sample_balanced(labels, batch_size_per_image, positive_fraction, generator=None):
    """BalancedPositiveNegativeSampler (model/utils.py:37-97) for one scene, without a read-back -> (pos_mask, neg_mask),
    uint8 [A].  Positives are ``labels >= 1``, negatives ``labels == 0``; min(P, int(batch * fraction)) positives and
    min(N, batch - positives) negatives are drawn uniformly without replacement: every element gets an independent
    uniform key and the largest keys of each kind win (``topk`` with a fixed k); the negatives' quota stays on the device.
    The draw is the reference's in distribution, not its random stream (that one is ``randperm`` of data-dependent
    sizes).  ``generator``: a torch.Generator on the labels' device."""
    if labels.dim() != 1:
        raise ValueError(f"labels must be [A], got {tuple(labels.shape)}")
    if batch_size_per_image < 0 or not 0.0 <= positive_fraction <= 1.0:
        raise ValueError("batch_size_per_image must be >= 0 and positive_fraction in [0, 1]")
    n, dev = labels.shape[0], labels.device
    pos, neg = labels >= 1, labels == 0
    keys = torch.rand((2, n), generator=generator, device=dev)
    minus = torch.full((n,), -1.0, device=dev)

    def draw(member, key, k, quota):
        mask = torch.zeros((n,), dtype=torch.uint8, device=dev)
        if k == 0:
            return mask, torch.zeros((), dtype=torch.int64, device=dev)
        vals, idx = torch.topk(torch.where(member, key, minus), k, sorted=True)       # keys are >= 0, the others -1
        chosen = vals >= 0
        if quota is not None:
            chosen = chosen & (torch.arange(k, device=dev) < quota)
        mask.scatter_(0, idx, chosen.to(torch.uint8))
        return mask, chosen.sum()

    pos_mask, num_pos = draw(pos, keys[0], min(int(batch_size_per_image * positive_fraction), n), None)
    neg_mask, _ = draw(neg, keys[1], min(int(batch_size_per_image), n), batch_size_per_image - num_pos)
    return pos_mask, neg_mask
