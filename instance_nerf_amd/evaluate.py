"""Scoring of 3-D instance masks: pairwise mask IoU, VOC average precision and recall.

The metric is the one the reference reports for ``masks/<scene>.npz``: per-class VOC AP and recall at IoU 0.25 and 0.5
over a pairwise 3-D mask IoU matrix (/root/reference/nerf_rcnn/eval.py:399-512 ``evaluate_map_recall``,
model/utils.py:786-802 ``mask_iou_3d``, called from run_rcnn.py:672-721).  The reference repeats both mask sets to
[N, M, W, L, H]; here every mask becomes a bit plane (64 voxels per word) and the counts are AND + popcount sums
(csrc/overlap.hip), so 30 x 30 masks at 160^3 cost two packs and one pair-count launch.

* ``pack_mask_planes`` / ``pack_label_planes``: masks or a label volume -> ``(planes, area, shape)``.
* ``mask_overlap`` / ``label_mask_overlap``: the integer counts ``(inter [N, M], area1 [N], area2 [M])``.
* ``mask_iou_3d`` / ``label_mask_iou``: fp32 IoU from those counts, the reference's arithmetic.
* ``box_iou_3d``: the axis-aligned box form (model/utils.py:391-462).
* ``evaluate_map_recall``: AP and recall per class; ``evaluate_masks``: the result dict of run_rcnn.py:712-721 for one
  scene.

GPU inputs with ``fused=True`` run the HIP kernels; CPU inputs, or ``fused=False``, take a composable torch path that
computes the same integers as chunked matmuls of the flattened masks (never the [N, M, V] repeat).  Everything that is
compared is an integer or an fp32 quotient of two integers, so both paths give the same bits.
"""
import os

import numpy as np
import torch

from . import _lib
from .maskbits import as_tensor, pack_planes, unpack_planes, words
from .masks import instance_detections, load_3d_masks

OVERLAP_MAX_MASKS, OVERLAP_MAX_CHANNELS = 1024, 256        # include/inr.h: limits of the overlap exports
OVERLAP_MIN_RUN_WORDS = 1024        # csrc/overlap.hip kMinRun: fewest words per workgroup of the default pair-count launch
_CHUNK = 1 << 20                    # voxels per matmul of the composable path (counts of a chunk are exact in fp32)


def _is_packed(m):
    return isinstance(m, (tuple, list)) and len(m) == 3 and torch.is_tensor(m[0]) and m[0].dtype == torch.int64


def _flat_masks(masks, who):
    """bool / uint8 [k, W, L, H] (numpy or tensor) -> (uint8 view [k, V], (W, L, H))."""
    m = as_tensor(masks)
    if m.ndim != 4 or m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{who}: masks must be bool or uint8 [k, W, L, H], got {m.dtype} {tuple(m.shape)}")
    shape = tuple(int(v) for v in m.shape[1:])
    if min(shape) < 1:
        raise ValueError(f"{who}: empty volume {shape}")
    m = m.contiguous()
    return (m.view(torch.uint8) if m.dtype == torch.bool else m).reshape(m.shape[0], int(np.prod(shape))), shape


def _check_labels(labels, K, first_channel, who):
    lab = as_tensor(labels)
    if lab.ndim != 3 or lab.dtype != torch.uint8 or lab.numel() == 0:
        raise ValueError(f"{who}: labels must be a non-empty uint8 [W, L, H] volume, got {lab.dtype} {tuple(lab.shape)}")
    if not 1 <= int(K) <= OVERLAP_MAX_CHANNELS or not 0 <= int(first_channel) <= int(K):
        raise ValueError(f"{who}: need 1 <= K <= {OVERLAP_MAX_CHANNELS} and 0 <= first_channel <= K")
    return lab.contiguous(), tuple(int(v) for v in lab.shape)


# ---- bit planes (the layout: maskbits.py) ------------------------------------------------------------------------------
def pack_mask_planes(masks, device=None, fused=True):
    """bool / uint8 [k, W, L, H] masks (non-zero = inside) -> ``(planes int64 [k, ceil(V / 64)], area int32 [k], (W, L, H))``
    on ``device`` (default: where the masks live): bit v % 64 of word v / 64 of row i = mask i holds flattened voxel v,
    tail bits zero (int64 is the storage type, the kernels read uint64).  ``mask_iou_3d`` takes the result in place of
    the masks, so a caller scoring one mask set many times packs once.  On the GPU with ``fused`` one launch of
    ``inr_pack_mask_planes`` (at most 1024 masks); otherwise plain torch."""
    flat, shape = _flat_masks(masks, "pack_mask_planes")
    if device is not None:
        flat = flat.to(device)
    k, V = (int(v) for v in flat.shape)
    if not (flat.is_cuda and fused):
        return pack_planes(flat), (flat != 0).sum(1).to(torch.int32), shape
    if k > OVERLAP_MAX_MASKS:
        raise ValueError(f"the fused pack takes at most {OVERLAP_MAX_MASKS} masks (got {k}); use fused=False")
    planes = torch.empty(k, words(V), dtype=torch.int64, device=flat.device)
    area = torch.empty(k, dtype=torch.int32, device=flat.device)
    _lib.check(_lib.load().inr_pack_mask_planes(_lib.ptr_or_null(flat, torch.uint8, "masks"), k, V, _lib.ptr_or_null(planes),
                                                _lib.ptr_or_null(area), _lib.stream_ptr()), "pack_mask_planes")
    return planes, area, shape


def pack_label_planes(labels, K, first_channel=1, device=None, fused=True):
    """uint8 [W, L, H] label volume (``extract_instances``'s ``labels``) -> ``(planes, area, (W, L, H))`` of the
    K - first_channel masks ``labels == c``, c = first_channel .. K - 1, in the layout of ``pack_mask_planes``, without
    materialising them.  A label >= K (``LABEL_EMPTY`` included) is in no mask.  On the GPU with ``fused`` one launch of
    ``inr_pack_label_planes`` (K <= 256)."""
    lab, shape = _check_labels(labels, K, first_channel, "pack_label_planes")
    if device is not None:
        lab = lab.to(device)
    K, first = int(K), int(first_channel)
    k, V = K - first, lab.numel()
    if not (lab.is_cuda and fused):
        onehot = lab.reshape(1, V) == torch.arange(first, K, device=lab.device, dtype=torch.int64).view(k, 1)
        return pack_planes(onehot), onehot.sum(1).to(torch.int32), shape
    planes = torch.empty(k, words(V), dtype=torch.int64, device=lab.device)
    area = torch.empty(k, dtype=torch.int32, device=lab.device)
    _lib.check(_lib.load().inr_pack_label_planes(_lib.ptr(lab, torch.uint8, "labels"), V, K, first, _lib.ptr_or_null(planes),
                                                 _lib.ptr_or_null(area), _lib.stream_ptr()), "pack_label_planes")
    return planes, area, shape


def overlap_planes(packed1, packed2, run_words=0):
    """The pair-count launch on two packed mask sets over the same volume -> inter int32 [k1, k2] (``inr_mask_overlap``).
    ``run_words``: words per workgroup, a multiple of 256; 0 = the library's choice."""
    (p1, _, s1), (p2, _, s2) = packed1, packed2
    if tuple(s1) != tuple(s2):
        raise ValueError(f"the two mask sets cover different volumes: {tuple(s1)} and {tuple(s2)}")
    k1, k2, V = int(p1.shape[0]), int(p2.shape[0]), int(np.prod(s1))
    if max(k1, k2) > OVERLAP_MAX_MASKS:
        raise ValueError(f"the fused overlap takes at most {OVERLAP_MAX_MASKS} masks per side (got {k1}, {k2}); use fused=False")
    inter = torch.empty(k1, k2, dtype=torch.int32, device=p1.device)
    if k1 == 0 or k2 == 0:
        return inter
    _lib.check(_lib.load().inr_mask_overlap(_lib.ptr(p1, torch.int64, "planes1"), k1, _lib.ptr(p2, torch.int64, "planes2"), k2,
                                            V, int(run_words), _lib.ptr(inter), _lib.stream_ptr()), "mask_overlap")
    return inter


# ---- counts ------------------------------------------------------------------------------------------------------------
class _Operand:
    """One side of ``_overlap``: k masks over a volume ``shape``, held as exactly one of flat uint8 masks [k, V], the
    (planes, area) of a packed triple, or a flattened label volume uint8 [V] whose channels first..K-1 are the masks."""

    def __init__(self, shape, flat=None, packed=None, labels=None, first=0, K=0):
        self.shape, self.V = tuple(int(v) for v in shape), int(np.prod(shape))
        self.flat, self.packed, self.labels, self.first, self.K = flat, packed, labels, first, K
        held = labels if labels is not None else flat if flat is not None else packed[0]
        self.device, self.k = held.device, K - first if labels is not None else int(held.shape[0])

    @classmethod
    def of_masks(cls, m, who):
        """bool / uint8 [k, W, L, H] masks, or - the second constructor - the triple of ``pack_mask_planes``."""
        if _is_packed(m):
            return cls(m[2], packed=(m[0], m[1]))
        flat, shape = _flat_masks(m, who)
        return cls(shape, flat=flat)

    @classmethod
    def of_labels(cls, labels, K, first_channel, who):
        lab, shape = _check_labels(labels, K, first_channel, who)
        return cls(shape, labels=lab.reshape(-1), first=int(first_channel), K=int(K))

    def to(self, dev):
        def move(t):
            return None if t is None else t.to(dev)
        return _Operand(self.shape, move(self.flat), None if self.packed is None else tuple(move(t) for t in self.packed),
                        move(self.labels), self.first, self.K)

    def planes(self):
        """The fused route: ``(planes, area, shape)``, packed by the kernels unless the operand came packed."""
        if self.packed is not None:
            return self.packed[0].contiguous(), self.packed[1], self.shape
        if self.flat is not None:
            return pack_mask_planes(self.flat.view((self.k,) + self.shape))
        return pack_label_planes(self.labels.view(self.shape), self.K, self.first)

    def rows(self, lo, hi):
        """The composable route: the masks over voxels [lo, hi), lo a multiple of 64, as a 0 / 1 float matrix [k, hi - lo]
        (fp32 on the GPU, fp64 on the CPU)."""
        dtype = torch.float32 if self.device.type == "cuda" else torch.float64
        if self.labels is not None:
            ch = torch.arange(self.first, self.K, device=self.device, dtype=torch.int64).view(-1, 1)
            return (self.labels[lo:hi].view(1, -1) == ch).to(dtype)
        if self.flat is not None:
            return (self.flat[:, lo:hi] != 0).to(dtype)
        return unpack_planes(self.packed[0][:, lo // 64:words(hi)], hi - lo).to(dtype)


def _overlap(op1, op2, fused, who):
    """-> (inter int64 [k1, k2], area1 int64 [k1], area2 int64 [k2]) of two ``_Operand``s, on the GPU if either lives
    there.  Fused: two packs (unless packed already) and the pair-count launch.  Composable: chunked matmuls of 0 / 1
    matrices; a chunk holds at most 2^20 voxels, so every entry of a product is an integer below 2^24 and exact in fp32
    (GPU) or fp64 (CPU)."""
    if op1.shape != op2.shape:
        raise ValueError(f"{who}: the two mask sets cover different volumes: {op1.shape} and {op2.shape}")
    dev = op2.device if op2.device.type == "cuda" and op1.device.type != "cuda" else op1.device
    op1, op2 = op1.to(dev), op2.to(dev)
    if fused and dev.type == "cuda":
        pa, pb = op1.planes(), op2.planes()
        return overlap_planes(pa, pb).long(), pa[1].long(), pb[1].long()
    inter = torch.zeros(op1.k, op2.k, dtype=torch.int64, device=dev)
    a1 = torch.zeros(op1.k, dtype=torch.int64, device=dev)
    a2 = torch.zeros(op2.k, dtype=torch.int64, device=dev)
    for lo in range(0, op1.V, _CHUNK):
        x, y = op1.rows(lo, min(op1.V, lo + _CHUNK)), op2.rows(lo, min(op1.V, lo + _CHUNK))
        inter += (x @ y.t()).to(torch.int64)
        a1 += x.sum(1).to(torch.int64)
        a2 += y.sum(1).to(torch.int64)
    return inter, a1, a2


def iou_from_counts(inter, area1, area2):
    """inter [N, M], area1 [N], area2 [M] integers -> fp32 [N, M] = inter / (area1 + area2 - inter): the union is formed
    in integers, both operands are converted to fp32 and divided in fp32 (what torch's true division of two int64
    tensors does, and so what the reference computes); 0 / 0 is NaN."""
    inter = inter.long()
    union = area1.long().view(-1, 1) + area2.long().view(1, -1) - inter
    return inter.to(torch.float32) / union.to(torch.float32)


@torch.no_grad()
def mask_overlap(masks1, masks2, fused=True):
    """-> ``(inter int64 [N, M], area1 int64 [N], area2 int64 [M])``: voxels shared by every pair and voxels per mask.
    Inputs as ``mask_iou_3d``."""
    return _overlap(_Operand.of_masks(masks1, "mask_overlap"), _Operand.of_masks(masks2, "mask_overlap"), fused, "mask_overlap")


@torch.no_grad()
def mask_iou_3d(masks1, masks2, fused=True):
    """Pairwise IoU of two sets of 3-D masks -> fp32 [N, M] (the reference's ``mask_iou_3d``, model/utils.py:786-802,
    same bits).  Each input is bool / uint8 [k, W, L, H] (numpy or tensor, non-zero = inside) or the ``(planes, area,
    shape)`` of an earlier ``pack_mask_planes``.  The result lives on the GPU if either input does.  A pair of empty
    masks gives NaN."""
    return iou_from_counts(*mask_overlap(masks1, masks2, fused))


@torch.no_grad()
def label_mask_overlap(labels, K, masks2, first_channel=1, fused=True):
    """As ``mask_overlap`` with the first set given as a label volume: row i is the mask ``labels == first_channel + i``."""
    return _overlap(_Operand.of_labels(labels, K, first_channel, "label_mask_overlap"),
                    _Operand.of_masks(masks2, "label_mask_overlap"), fused, "label_mask_overlap")


@torch.no_grad()
def label_mask_iou(labels, K, masks2, first_channel=1, fused=True):
    """IoU of the K - first_channel masks of a label volume (uint8 [W, L, H], ``extract_instances``'s ``labels``) against
    ``masks2`` -> fp32 [K - first_channel, M], without materialising K boolean volumes."""
    return iou_from_counts(*label_mask_overlap(labels, K, masks2, first_channel, fused))


def box_iou_3d(boxes1, boxes2):
    """Pairwise IoU of axis-aligned boxes (x1, y1, z1, x2, y2, z2) -> [N, M], the reference's AABB form
    (model/utils.py:391-462): volumes and the clamped overlap extents multiplied axis by axis in the boxes' own float
    type, union = volume1 + volume2 - overlap.  Plain torch on the inputs' device."""
    b1, b2 = as_tensor(boxes1), as_tensor(boxes2)
    if b1.ndim != 2 or b2.ndim != 2 or b1.shape[1] != 6 or b2.shape[1] != 6:
        raise ValueError("box_iou_3d: boxes must be [N, 6] and [M, 6] (oriented boxes are not supported)")
    if not b1.is_floating_point():
        b1, b2 = b1.float(), b2.float()
    b2 = b2.to(device=b1.device, dtype=b1.dtype)

    def volume(b):
        return (b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2])
    lo = torch.maximum(b1[:, None, :3], b2[None, :, :3])
    hi = torch.minimum(b1[:, None, 3:], b2[None, :, 3:])
    ext = (hi - lo).clamp(min=0)
    overlap = ext[..., 0] * ext[..., 1] * ext[..., 2]
    union = volume(b1)[:, None] + volume(b2)[None, :] - overlap
    return overlap / union


# ---- average precision and recall ------------------------------------------------------------------------------------------
def _voc_ap(prec, rec):
    """Area under the precision envelope (VOC): sentinels (recall 0 and 1, precision 0), precision made non-increasing
    from the right, then the sum of (recall step) x (precision after the step)."""
    zero = torch.zeros(1, dtype=torch.float32)
    p = torch.cat((zero, torch.nan_to_num(prec), zero))
    r = torch.cat((zero, rec, torch.ones(1, dtype=torch.float32)))
    p = torch.flip(torch.cummax(torch.flip(p, [0]), 0).values, [0])
    step = torch.where(r[1:] != r[:-1])[0]
    return torch.sum((r[step + 1] - r[step]) * p[step + 1])


@torch.no_grad()
def evaluate_map_recall(pred_list, scores_list, labels_list, gt_list, gt_labels_list, iou_thresh=0.25, top_k=None,
                        iou_type="box", fused=True, iou_list=None):
    """Per-class VOC average precision and recall at one IoU threshold over a list of scenes - the rule of the
    reference's ``evaluate_map_recall`` (eval.py:399-512).  Per scene: ``pred_list[i]`` / ``gt_list[i]`` are boxes
    [n, 6] (``iou_type='box'``) or masks [n, W, L, H] (``'mask'``; anything ``mask_iou_3d`` takes), ``scores_list[i]``
    [n], ``labels_list[i]`` / ``gt_labels_list[i]`` integer classes.

    With ``top_k``, a scene keeps its ``top_k`` best-scored predictions.  Per scene and class the predictions are taken
    in descending score order; each takes the ground truth of its class with the largest IoU (torch's ``max``: the first
    of equal values, and a NaN - a pair of empty masks - wins), or none if that IoU is below ``iou_thresh`` (an IoU equal
    to the threshold matches); it is a true positive only if no earlier prediction took that ground truth.  Per class,
    over all scenes in descending score order: precision = TP / (TP + FP), recall = TP / (number of ground truths), AP =
    the area under the precision envelope.

    -> ``(ap, recalls)``, fp32 [max class + 1].  AP is NaN for a class without ground truth; recall is NaN for a class
    without ground truth or without predictions (its AP is then 0), as in the reference.  Tied scores have no defined
    order.  The IoU matrices come from ``mask_iou_3d`` / ``box_iou_3d`` - one [n_pred, n_gt] matrix per scene, or
    ``iou_list`` when the caller has them already - and the matching loop runs on the host."""
    if iou_type not in ("box", "mask"):
        raise ValueError("iou_type must be 'box' or 'mask'")
    n_gt, scores, flags = {}, {}, {}
    for s in range(len(scores_list)):
        sc = as_tensor(scores_list[s]).detach().cpu().reshape(-1)
        pl = as_tensor(labels_list[s]).detach().cpu().reshape(-1).to(torch.int64)
        gl = as_tensor(gt_labels_list[s]).detach().cpu().reshape(-1).to(torch.int64)
        if iou_list is not None:
            iou = as_tensor(iou_list[s])
        elif len(pl) == 0 or len(gl) == 0:
            iou = torch.zeros(len(pl), len(gl))
        elif iou_type == "mask":
            iou = mask_iou_3d(pred_list[s], gt_list[s], fused=fused)
        else:
            iou = box_iou_3d(pred_list[s], gt_list[s])
        iou = iou.detach().cpu()
        if tuple(iou.shape) != (len(pl), len(gl)) or len(sc) != len(pl):
            raise ValueError(f"scene {s}: {len(sc)} scores, {len(pl)} labels, {len(gl)} ground truths, IoU {tuple(iou.shape)}")
        kept = torch.arange(len(pl))
        if top_k is not None and len(pl) > top_k:
            kept = torch.argsort(sc, descending=True)[:top_k]
        for c in torch.unique(torch.cat((pl[kept], gl))).tolist():
            mine = kept[pl[kept] == c]
            mine = mine[torch.argsort(sc[mine], descending=True)]
            truth = torch.where(gl == c)[0]
            n_gt[c] = n_gt.get(c, 0) + len(truth)
            scores.setdefault(c, []).extend(sc[mine].tolist())
            hit = flags.setdefault(c, [])
            if len(mine) == 0:
                continue
            if len(truth) == 0:
                hit.extend([0] * len(mine))
                continue
            best, choice = iou[mine][:, truth].max(dim=1)
            choice[best < iou_thresh] = -1
            taken = set()
            for g in choice.tolist():
                hit.append(1 if g >= 0 and g not in taken else 0)
                if g >= 0:
                    taken.add(g)
    if not n_gt:
        raise ValueError("evaluate_map_recall: no predictions and no ground truth in any scene")
    n_classes = max(n_gt) + 1
    ap = torch.full((n_classes,), float("nan"), dtype=torch.float32)
    recalls = torch.full((n_classes,), float("nan"), dtype=torch.float32)
    for c, n in n_gt.items():
        if n == 0:
            continue                                    # no ground truth: both stay NaN
        sc = torch.tensor(scores[c], dtype=torch.float32)
        hit = torch.tensor(flags[c], dtype=torch.int64)[torch.argsort(sc, descending=True)]
        tp = torch.cumsum(hit == 1, 0).to(torch.float32)
        fp = torch.cumsum(hit == 0, 0).to(torch.float32)
        prec, rec = tp / (fp + tp), tp / n
        if len(rec):
            recalls[c] = rec[-1]
        ap[c] = _voc_ap(prec, rec)
    return ap, recalls


# ---- one scene: the result dict ------------------------------------------------------------------------------------------
def _is_extract_result(d):
    return isinstance(d, dict) and "counts" in d and "labels" in d and getattr(d["labels"], "ndim", 0) == 3


def _load_scene(d, who):
    if isinstance(d, (str, os.PathLike)):
        d = load_3d_masks(d)
    missing = {"masks", "labels", "boxes"} - set(d)
    if missing:
        raise ValueError(f"{who}: missing keys {sorted(missing)} (the layout of masks.load_3d_masks)")
    return d


def _nanmean(t):
    return float(torch.mean(t[~torch.isnan(t)]))


@torch.no_grad()
def evaluate_masks(pred, gt, top_k=None, labels=None, min_voxels=1, fused=True):
    """Scores the 3-D masks of one scene against ground truth -> the dict of the reference's evaluation
    (run_rcnn.py:712-721): ``mAP_50, mAP_25, AR_50, AR_25`` over the mask IoU and ``box_mAP_50, box_mAP_25, box_AR_50,
    box_AR_25`` over the box IoU - means over the classes whose value is not NaN - plus, for reporting, ``gt_best_iou``
    fp32 [n_gt] (the best mask IoU any prediction reaches on each ground truth; NaN counts as 0) and ``gt_best_pred``
    int64 [n_gt] (its index, -1 without predictions).

    ``gt``: a dict in the layout of ``masks.load_3d_masks`` (``masks`` [k, W, L, H], ``labels`` [k], ``boxes`` [k, 6]) or
    the path of such an ``.npz``.  ``pred``: the same (with ``scores`` [k]), or the result of
    ``extract.extract_instances``: its label volume is scored directly (``label_mask_iou``, channel i + 1 = prediction
    i), with the conventions of ``masks.instance_detections``, which ``masks.write_instance_masks_npz`` writes - classes
    ``labels`` (default all ones), boxes = inclusive voxel bounds with + 1 on the upper corner, and an instance below
    ``min_voxels`` voxels an empty mask with score 0 and a zero box - so the result equals scoring that file.  With ``fused`` and a GPU
    present, host arrays (files) are moved there and scored by the HIP kernels."""
    gt = _load_scene(gt, "evaluate_masks: gt")
    g_masks, g_cls, g_boxes = gt["masks"], as_tensor(gt["labels"]).cpu(), as_tensor(gt["boxes"]).cpu().float()
    if fused and torch.cuda.is_available():                # host arrays (files) are scored on the GPU when there is one
        g_masks = as_tensor(g_masks).cuda()
    if _is_extract_result(pred):
        keep, p_cls, p_scores, p_boxes = (torch.from_numpy(a) for a in instance_detections(
            pred, labels, min_voxels, who="evaluate_masks: the extraction"))
        inter, a1, a2 = label_mask_overlap(pred["labels"], len(keep) + 1, g_masks, 1, fused)
        drop = ~keep.to(inter.device)
        inter[drop], a1[drop] = 0, 0
        iou = iou_from_counts(inter, a1, a2)
    else:
        pred = _load_scene(pred, "evaluate_masks: pred")
        if "scores" not in pred:
            raise ValueError("evaluate_masks: pred: missing key 'scores'")
        p_cls, p_scores = as_tensor(pred["labels"]).cpu(), as_tensor(pred["scores"]).cpu().float()
        p_boxes = as_tensor(pred["boxes"]).cpu().float()
        n_p, n_g = len(p_cls), len(g_cls)
        iou = mask_iou_3d(pred["masks"], g_masks, fused=fused) if n_p and n_g else torch.zeros(n_p, n_g)
    iou = iou.cpu()
    box_iou = box_iou_3d(p_boxes, g_boxes)
    out = {}
    for prefix, mat, kind in (("", iou, "mask"), ("box_", box_iou, "box")):
        for name, thresh in (("50", 0.5), ("25", 0.25)):
            ap, rec = evaluate_map_recall([None], [p_scores], [p_cls], [None], [g_cls], iou_thresh=thresh, top_k=top_k,
                                          iou_type=kind, iou_list=[mat])
            out[f"{prefix}mAP_{name}"], out[f"{prefix}AR_{name}"] = _nanmean(ap), _nanmean(rec)
    if iou.shape[0] > 0:
        best = torch.nan_to_num(iou, nan=0.0).max(dim=0)
        out["gt_best_iou"], out["gt_best_pred"] = best.values, best.indices
    else:
        out["gt_best_iou"] = torch.zeros(iou.shape[1])
        out["gt_best_pred"] = torch.full((iou.shape[1],), -1, dtype=torch.int64)
    return out
