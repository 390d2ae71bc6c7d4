"""The tail of the 3-D detector: from head outputs to ``masks/<scene>.npz``.

The reference ends its detector with a per-class 3-D NMS (/root/reference/nerf_rcnn/model/utils.py:217-267, called from
model/nerf_rcnn.py:606-635) and ``paste_masks_in_image`` (model/utils.py:646-782, called from nerf_rcnn.py:768-772),
which resamples each M^3 mask probability into the scene grid and thresholds it at 0.5, and writes the top detections
with ``np.savez`` (run_rcnn.py:652-666).  On a GPU its paste samples the whole volume per mask through an
[N, W, L, H, 3] fp32 grid to produce one bit per voxel; here the bits are produced directly (csrc/detect.hip), in the
bit-plane layout of maskbits.py, which the mask metric and - through
``planes_to_voxel_words`` - the projector take as they are.

* ``nms_3d`` / ``batched_nms_3d``: indices of the surviving boxes in decreasing score order.
* ``postprocess_detections``: the selection rule of nerf_rcnn.py:606-635 for one scene.
* ``paste_masks``: M^3 probabilities + boxes -> bit planes, bool masks, or the fp32 values.
* ``planes_to_voxel_words``: bit planes -> the ``masks.pack_mask_words`` list the projector reads.
* ``write_detections_npz``: the file ``masks.load_3d_masks`` reads.

GPU tensors with ``fused=True`` run the HIP kernels; CPU tensors, or ``fused=False``, take a composable torch path - for
the paste the reference's method restated (chunked ``F.grid_sample``, then ``>=``), for NMS the greedy loop.  The fused
paste reproduces torch's CPU ``grid_sample`` bit for bit (fp32, torch's operation order, no fused multiply-add; the
contract is spelled out in include/inr.h and tests/paste_reference.py); a GPU ``grid_sample`` may round differently, so
on a GPU the composable path is a baseline, not a bit-exact twin.

Departures from the reference, both at inputs its own pipeline never produces: a box with a non-finite coordinate or a
side <= 0 pastes an empty mask (the reference divides by zero), and boxes of equal score keep their input order (a stable
sort; the reference's order for ties is unspecified).  Boxes are taken as fp32.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .evaluate import box_iou_3d
from .maskbits import as_tensor, interleave32, pack_planes, unpack_planes, words

NMS_MAX_BOXES = 4096            # include/inr.h: limit of inr_nms_3d_pairs / inr_nms_3d_scan
PASTE_MAX_MASKS, PASTE_MAX_M = 1024, 1024        # include/inr.h: limits of inr_paste_masks
_PASTE_CHUNK_BYTES = 1 << 28    # fp32 bytes of one grid_sample output of the composable paste


# ---- NMS -----------------------------------------------------------------------------------------------------------------
def _check_boxes(boxes, who):
    b = as_tensor(boxes)
    if b.ndim != 2 or b.shape[1] != 6:
        raise ValueError(f"{who}: boxes must be [n, 6] (x1, y1, z1, x2, y2, z2); oriented boxes are not supported")
    return b.float()


def _greedy_sorted(boxes, cls, thresh):
    """boxes [n, 6] sorted by decreasing score, cls [n] -> sorted positions of the survivors (the reference's loop)."""
    n = boxes.shape[0]
    removed = torch.zeros(n, dtype=torch.bool, device=boxes.device)
    keep = []
    for i in range(n):
        if bool(removed[i]):
            continue
        keep.append(i)
        if i + 1 < n:
            iou = box_iou_3d(boxes[i:i + 1], boxes[i + 1:])[0]
            removed[i + 1:] |= ~(iou <= thresh) & (cls[i + 1:] == cls[i])
    return torch.tensor(keep, dtype=torch.int64, device=boxes.device)


@torch.no_grad()
def batched_nms_3d(boxes, scores, idxs, iou_threshold, fused=True):
    """Per-class greedy NMS of axis-aligned 3-D boxes (the reference's ``batched_nms``, model/utils.py:235-267): boxes
    [n, 6], scores [n], idxs [n] integer classes -> int64 indices of the survivors in decreasing score order.  A box is
    dropped when a surviving box of its class with a higher score has ``!(iou <= iou_threshold)`` with it (so a NaN IoU
    suppresses, as the reference's ``iou <= iou_threshold`` survival test does).  Equal scores: the lower index first.

    On the GPU with ``fused`` and n <= 4096: one sort, ``inr_nms_3d_pairs`` and ``inr_nms_3d_scan``; nothing is read
    back but the number of survivors.  The kernels compare class ids as int32: an id outside that range raises
    ValueError (after the launches, with the same read-back).  Above 4096 boxes, on the CPU, or with ``fused=False``: the greedy torch loop."""
    b = _check_boxes(boxes, "batched_nms_3d")
    sc, cl = as_tensor(scores).to(b.device).reshape(-1), as_tensor(idxs).to(b.device).reshape(-1)
    n = int(b.shape[0])
    if sc.shape[0] != n or cl.shape[0] != n:
        raise ValueError(f"batched_nms_3d: {n} boxes, {sc.shape[0]} scores, {cl.shape[0]} classes")
    if cl.is_floating_point():
        raise ValueError("batched_nms_3d: idxs must be integers")
    order = torch.sort(sc, descending=True, stable=True).indices
    bs, cs = b[order].contiguous(), cl[order]
    if not (b.is_cuda and fused and n <= NMS_MAX_BOXES):
        return order[_greedy_sorted(bs, cs, float(iou_threshold))]
    lib = _lib.load()
    keep = torch.empty(n, dtype=torch.int32, device=b.device)
    n_keep = torch.empty(1, dtype=torch.int32, device=b.device)
    wide = torch.zeros(1, dtype=torch.int32, device=b.device)
    pairs = None
    if n > 0:
        if cs.dtype == torch.int64:     # the kernels compare int32 ids: checked, never wrapped
            wide = ((cs < -2 ** 31) | (cs > 2 ** 31 - 1)).any().to(torch.int32).view(1)
        cs = cs.to(torch.int32).contiguous()
        pairs = torch.empty(n, (n + 63) // 64, dtype=torch.int64, device=b.device)
        _lib.check(lib.inr_nms_3d_pairs(_lib.ptr(bs, torch.float32, "boxes"), _lib.ptr(cs, torch.int32, "classes"), n,
                                        float(iou_threshold), _lib.ptr(pairs), _lib.stream_ptr()), "nms_3d_pairs")
    _lib.check(lib.inr_nms_3d_scan(_lib.ptr_or_null(pairs), n, _lib.ptr_or_null(keep), _lib.ptr(n_keep), _lib.stream_ptr()),
               "nms_3d_scan")
    kept, bad = torch.cat([n_keep, wide]).tolist()                 # the one read-back
    if bad:
        raise ValueError("batched_nms_3d: the fused path takes class ids in the int32 range; use fused=False")
    return order[keep[:kept].long()]


def nms_3d(boxes, scores, iou_threshold, fused=True):
    """Greedy NMS over one class (the reference's ``nms``, model/utils.py:217-232) -> int64 indices, decreasing score."""
    b = _check_boxes(boxes, "nms_3d")
    return batched_nms_3d(b, scores, torch.zeros(b.shape[0], dtype=torch.int64, device=b.device), iou_threshold, fused)


@torch.no_grad()
def postprocess_detections(boxes, scores, image_shape, score_thresh=0.01, nms_thresh=0.2, detections_per_img=100, fused=True):
    """The detection rule of the reference for one scene (model/nerf_rcnn.py:606-635; defaults run_rcnn.py:143-147) from
    the decoded head outputs: boxes [n, C, 6] (one box per proposal and class), scores [n, C] (softmax over the C classes,
    class 0 = background).  Clip every box to the grid ``image_shape`` = (W, L, H); drop class 0; make every (proposal,
    class) pair a detection; keep ``score > score_thresh``; drop boxes with a side < 1e-2; per-class NMS at
    ``nms_thresh``; the first ``detections_per_img`` by score.  -> ``(boxes [k, 6], scores [k], labels int64 [k])``."""
    b, sc = as_tensor(boxes).float(), as_tensor(scores)
    if b.ndim != 3 or b.shape[2] != 6 or sc.ndim != 2 or tuple(sc.shape) != tuple(b.shape[:2]):
        raise ValueError(f"postprocess_detections: boxes must be [n, C, 6] and scores [n, C], got {tuple(b.shape)}, {tuple(sc.shape)}")
    sc = sc.to(b.device)
    size = torch.tensor([float(v) for v in image_shape] * 2, dtype=b.dtype, device=b.device)
    b = torch.minimum(b.clamp(min=0), size)
    labels = torch.arange(b.shape[1], device=b.device).view(1, -1).expand_as(sc)
    b, sc, labels = b[:, 1:].reshape(-1, 6), sc[:, 1:].reshape(-1), labels[:, 1:].reshape(-1)
    keep = torch.where(sc > score_thresh)[0]
    b, sc, labels = b[keep], sc[keep], labels[keep]
    sides = b[:, 3:] - b[:, :3]
    keep = torch.where((sides >= 1e-2).all(1))[0]
    b, sc, labels = b[keep], sc[keep], labels[keep]
    keep = batched_nms_3d(b, sc, labels, nms_thresh, fused=fused)[:int(detections_per_img)]
    return b[keep], sc[keep], labels[keep]


# ---- paste ---------------------------------------------------------------------------------------------------------------
def _check_paste(mask_probs, boxes, image_shape, threshold, who):
    m = as_tensor(mask_probs)
    if m.ndim != 4 or not (m.shape[1] == m.shape[2] == m.shape[3]) or m.shape[1] < 1:
        raise ValueError(f"{who}: mask_probs must be [N, M, M, M] (only cube mask predictions are supported), got {tuple(m.shape)}")
    b = as_tensor(boxes)
    if b.ndim != 2 or b.shape[1] != 6 or b.shape[0] != m.shape[0]:
        raise ValueError(f"{who}: boxes must be [{m.shape[0]}, 6], got {tuple(b.shape)}")
    shape = tuple(int(v) for v in image_shape)
    if len(shape) != 3 or min(shape) < 1 or int(np.prod(shape)) >= 2 ** 31:
        raise ValueError(f"{who}: image_shape must be (W, L, H), each >= 1, fewer than 2^31 voxels; got {image_shape}")
    if not float(threshold) >= 0.0:
        raise ValueError(f"{who}: threshold must be >= 0 (the reference's uint8 debug output is not supported)")
    dev = m.device if m.is_cuda else b.device
    return m.to(dev).float().contiguous(), b.to(dev).float().contiguous(), shape


def _live_boxes(b):
    return torch.isfinite(b).all(1) & ((b[:, 3:] - b[:, :3]) > 0).all(1)


def _paste_soft_composable(m, b, shape):
    """The reference's whole-volume method (``_do_paste_mask(skip_empty=False)``), a chunk of masks at a time."""
    W, L, H = shape
    N = m.shape[0]
    out = torch.zeros((N,) + shape, dtype=torch.float32, device=m.device)
    live = _live_boxes(b)
    per = max(1, _PASTE_CHUNK_BYTES // (4 * W * L * H))
    ax = [torch.arange(s, dtype=torch.float32, device=m.device) for s in shape]
    for lo in range(0, N, per):
        idx = torch.where(live[lo:lo + per])[0] + lo
        if idx.numel() == 0:
            continue
        bb = b[idx]
        g = [(ax[a][None, :] - bb[:, a:a + 1]) / (bb[:, a + 3:a + 4] - bb[:, a:a + 1]) * 2 - 1 for a in range(3)]
        n = idx.numel()
        gx = g[0][:, :, None, None].expand(n, W, L, H)
        gy = g[1][:, None, :, None].expand(n, W, L, H)
        gz = g[2][:, None, None, :].expand(n, W, L, H)
        grid = torch.stack([gz, gy, gx], dim=-1)
        out[idx] = F.grid_sample(m[idx, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
    return out


@torch.no_grad()
def paste_masks(mask_probs, boxes, image_shape, threshold=0.5, out="planes", fused=True):
    """Pastes N mask probabilities of resolution M^3 into the scene grid (the reference's ``paste_masks_in_image``,
    model/utils.py:705-782, whole-volume path): mask_probs [N, M, M, M], boxes [N, 6] = (x1, y1, z1, x2, y2, z2) in grid
    units (they may leave the grid), image_shape (W, L, H).  Voxel (i, j, k) of mask n is set when the trilinear sample
    of the mask at the voxel's position inside the box (``grid_sample``, zeros padding, align_corners=True) is
    ``>= threshold``.

    ``out``: ``"planes"`` -> ``(planes int64 [N, ceil(V / 64)], area int32 [N], (W, L, H))``, the packed form that
    ``evaluate.mask_iou_3d`` / ``evaluate_masks`` accept in place of masks; ``"masks"`` -> bool [N, W, L, H];
    ``"soft"`` -> the fp32 samples [N, W, L, H] (tests).  On the GPU with ``fused``: one launch of ``inr_paste_masks``
    (N <= 1024, M <= 1024), which writes one bit per voxel and never holds a sampling grid; otherwise chunked
    ``F.grid_sample``.  A box with a non-finite coordinate or a side <= 0 gives an empty mask."""
    if out not in ("planes", "masks", "soft"):
        raise ValueError("out must be 'planes', 'masks' or 'soft'")
    m, b, shape = _check_paste(mask_probs, boxes, image_shape, threshold, "paste_masks")
    N, M, V = int(m.shape[0]), int(m.shape[1]), int(np.prod(shape))
    if not (m.is_cuda and fused):
        soft = _paste_soft_composable(m, b, shape)
        if out == "soft":
            return soft
        bits = soft >= threshold
        if out == "masks":
            return bits
        flat = bits.reshape(N, V)
        return pack_planes(flat), flat.sum(1).to(torch.int32), shape
    if N > PASTE_MAX_MASKS or M > PASTE_MAX_M:
        raise ValueError(f"the fused paste takes at most {PASTE_MAX_MASKS} masks of resolution at most {PASTE_MAX_M} "
                         f"(got {N}, {M}); use fused=False")
    planes = torch.empty(N, words(V), dtype=torch.int64, device=m.device)
    area = torch.empty(N, dtype=torch.int32, device=m.device)
    soft = torch.empty((N,) + shape, dtype=torch.float32, device=m.device) if out == "soft" else None
    P = _lib.ptr_or_null
    _lib.check(_lib.load().inr_paste_masks(P(m, torch.float32, "mask_probs"), P(b, torch.float32, "boxes"), N, M, shape[0],
                                           shape[1], shape[2], float(threshold), P(planes), P(area), P(soft),
                                           _lib.stream_ptr()), "paste_masks")
    if out == "soft":
        return soft
    if out == "planes":
        return planes, area, shape
    return unpack_planes(planes, V).bool().view((N,) + shape)


# ---- bit planes -> the projector's words ---------------------------------------------------------------------------------
@torch.no_grad()
def planes_to_voxel_words(packed, order=None, fused=True):
    """``(planes, area, shape)`` of ``paste_masks`` / ``evaluate.pack_mask_planes`` -> the list ``masks.pack_mask_words``
    returns for the same masks: one int32 tensor [W, L, H] per 32 masks, bit i of word j = mask 32 j + i holds the voxel.
    ``(k, words)`` is the ``packed`` argument of ``masks.soft_project`` / ``project_3d_masks`` / ``project_and_match``.
    ``order``: a permutation of the masks applied first (``masks.candidate_order`` for ``project_and_match``).  On the
    GPU with ``fused`` one launch of ``inr_planes_to_voxel_words`` per 32 masks: no bool volume, no int64 staging."""
    planes, _, shape = packed
    shape = tuple(int(v) for v in shape)
    k, V = int(planes.shape[0]), int(np.prod(shape))
    if planes.dtype != torch.int64 or planes.ndim != 2 or planes.shape[1] != words(V):
        raise ValueError(f"planes must be int64 [k, {words(V)}] for the volume {shape}")
    if order is not None:
        planes = planes[torch.as_tensor(list(order), dtype=torch.int64, device=planes.device)]
    planes = planes.contiguous()
    if not (planes.is_cuda and fused):
        return [interleave32(unpack_planes(planes[base:base + 32], V).bool()).view(shape) for base in range(0, k, 32)]
    out = []
    lib = _lib.load()
    for base in range(0, k, 32):
        w = torch.empty(shape, dtype=torch.int32, device=planes.device)
        _lib.check(lib.inr_planes_to_voxel_words(_lib.ptr(planes, torch.int64, "planes"), k, V, base, _lib.ptr(w),
                                                 _lib.stream_ptr()), "planes_to_voxel_words")
        out.append(w)
    return out


# ---- the file ----------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def write_detections_npz(path, mask_probs, boxes, scores, labels, image_shape, top_k=30, threshold=0.5, fused=True):
    """Writes ``masks/<scene>.npz`` as the reference does (run_rcnn.py:652-666) from a scene's detections: mask_probs
    [n, M, M, M], boxes [n, 6], scores [n], labels [n].  The ``top_k`` best-scored detections are selected FIRST (the
    reference pastes all and selects after; the file is the same and only ``top_k`` masks are pasted), pasted to bit
    planes, the planes copied to the host and unpacked there.  Keys: ``masks`` bool [k, W, L, H], ``scores`` float32 [k]
    descending, ``labels`` int64 [k], ``boxes`` float32 [k, 6] - what ``masks.load_3d_masks`` reads.  A scene without
    detections (or ``top_k=0``) writes the same keys with k = 0, as the reference does.  -> path."""
    sc = as_tensor(scores).detach().reshape(-1)
    n = int(sc.shape[0])
    m, b = as_tensor(mask_probs), as_tensor(boxes)
    lab = as_tensor(labels).detach().reshape(-1)
    if m.shape[0] != n or b.shape[0] != n or lab.shape[0] != n:
        raise ValueError(f"write_detections_npz: {n} scores, {m.shape[0]} masks, {b.shape[0]} boxes, {lab.shape[0]} labels")
    inds = torch.sort(sc, descending=True, stable=True).indices[:max(int(top_k), 0)]
    m, b = m[inds.to(m.device)], b[inds.to(b.device)]
    planes, _, shape = paste_masks(m, b, image_shape, threshold, out="planes", fused=fused)
    k, V = int(planes.shape[0]), int(np.prod(shape))
    bits = unpack_planes(planes.cpu(), V).numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, masks=bits.astype(bool).reshape((k,) + shape), scores=sc[inds].cpu().numpy().astype(np.float32),
                        labels=lab[inds.to(lab.device)].cpu().numpy().astype(np.int64),
                        boxes=b.detach().cpu().numpy().astype(np.float32))
    return path
