"""Training the FCOS proposal head: the targets of every location of the feature pyramid and the three losses of the
reference's ``FCOSLossComputation`` (nerf_rcnn/model/fcos/loss.py; locations and padding masks: fcos.py:221-265).

Two paths give the same result:

  fused       float32 GPU tensors: one launch of csrc/fcos.hip for the targets of all scenes and levels, two for the losses,
              one for their gradients (include/inr.h, "FCOS training targets and losses").  The head's tensors are read in
              place - no permuted or concatenated copy - and nothing is read back between the head's convolutions and
              ``backward()``.
  composable  everything else (CPU tensors, other float types, more than 1024 boxes in a scene, ``fused=False``): the
              reference's tensor program restated in plain torch, without ``nonzero`` or ``.item()``.

``fused=None`` picks the kernels where they apply, ``True`` insists on them (RuntimeError otherwise), ``False`` is the
composable path.  Axis-aligned boxes only, rows (x1, y1, z1, x2, y2, z2); 7-number oriented boxes raise ValueError as
elsewhere in the project.  Out of scope: the smooth_l1 and diou regression losses, the extra L1 and 2-D projection
losses, the post-processor and the head's own layers."""
import ctypes

import torch

from . import _lib

INF = 100000000
FCOS_MAX_GT, FCOS_MAX_LEVELS = _lib.FCOS_MAX_GT, _lib.FCOS_MAX_LEVELS
SIZES_OF_INTEREST = ((-1, 16), (16, 32), (32, 64), (64, INF))
LOSS_TYPES = {"iou": _lib.FCOS_LOSS_IOU, "linear_iou": _lib.FCOS_LOSS_LINEAR_IOU, "giou": _lib.FCOS_LOSS_GIOU}
FOCAL_ALPHA, FOCAL_GAMMA = 0.25, 2
# tools/fcos_probe.py writes profiles/fcos_probe.json; a shape in which the kernels lose to the composable path on the same
# GPU sends fused=None back to the composable path (see that file for what was measured)
TARGETS_FUSED_BY_DEFAULT = True
LOSS_FUSED_BY_DEFAULT = True


# ---- locations ---------------------------------------------------------------------------------------------------------
def _shapes(feature_shapes, strides):
    shapes = [tuple(int(v) for v in s) for s in feature_shapes]
    strides = [int(s) for s in strides]
    if not shapes or len(shapes) != len(strides) or any(len(s) != 3 or min(s) < 1 for s in shapes) or min(strides) < 1:
        raise ValueError("feature_shapes must be a list of (W, L, H) >= 1 with one stride >= 1 per level")
    return shapes, strides


def compute_locations(feature_shapes, strides, device="cpu"):
    """-> list per level of float32 [W*L*H, 3]: i * stride + stride // 2 per axis, x slowest (fcos.py:221-250)."""
    shapes, strides = _shapes(feature_shapes, strides)
    out = []
    for (w, l, h), stride in zip(shapes, strides):
        axes = [torch.arange(0, n * stride, step=stride, dtype=torch.float32, device=device) for n in (w, l, h)]
        x, y, z = torch.meshgrid(*axes, indexing="ij")
        out.append(torch.stack((x.reshape(-1), y.reshape(-1), z.reshape(-1)), dim=1) + stride // 2)
    return out


def compute_padding_masks(locations, ori_sizes):
    """-> list per level of bool [B, P_l]: the location lies inside scene b's unpadded extent (fcos.py:252-265)."""
    masks = []
    for loc in locations:
        masks.append(torch.stack([(loc[:, 0] < w) & (loc[:, 1] < l) & (loc[:, 2] < h) for (w, l, h) in ori_sizes], dim=0))
    return masks


def _gt(t, name="gt_boxes"):
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] not in (6, 7):
        if torch.is_tensor(t) and t.numel() == 0:
            return t.detach().reshape(0, 6)
        raise ValueError(f"{name} must be a list of tensors [G, 6] of boxes (x1, y1, z1, x2, y2, z2)")
    if t.shape[1] == 7:
        raise ValueError(f"{name}: oriented boxes (7 numbers) are not supported")
    if not t.is_floating_point():
        raise ValueError(f"{name} must be floating point, got {t.dtype}")
    return t.detach()


class FCOSTargets:
    """What ``prepare_targets`` returns.  ``labels`` (float32 [B P_l]), ``reg_targets`` (float32 [B P_l, 6]),
    ``centerness`` (float32), ``matched`` (int32) and ``valid`` (bool, or None without ``ori_sizes``) are lists per level,
    scenes concatenated inside each level - the reference's level-first lists - and views of one buffer per quantity
    (``labels_flat`` ...).  ``matched`` is meaningful where the scene has boxes; ``reg_targets`` are those of the matched
    box also where the label is 0, as in the reference."""

    def __init__(self, shapes, strides, B, labels, reg, ctr, matched, valid, host=None):
        self.feature_shapes, self.strides, self.B, self._host = shapes, strides, B, host
        self.labels_flat, self.reg_targets_flat, self.centerness_flat, self.matched_flat, self.valid_flat = \
            labels, reg, ctr, matched, valid
        sizes = [B * w * l * h for (w, l, h) in shapes]
        self.labels = list(labels.split(sizes))
        self.reg_targets = list(reg.split(sizes))
        self.centerness = list(ctr.split(sizes))
        self.matched = list(matched.split(sizes))
        self.valid = list(valid.split(sizes)) if valid is not None else None

    def with_valid(self, valid):
        return FCOSTargets(self.feature_shapes, self.strides, self.B, self.labels_flat, self.reg_targets_flat,
                           self.centerness_flat, self.matched_flat, valid)


def _f32(v):
    return ctypes.c_float(v).value


def _host_i32(values):
    return (ctypes.c_int32 * len(values))(*values)


def compute_centerness_targets(reg_targets):
    """loss.py:438-445 on [N, 6] targets."""
    lr, tb, fb = reg_targets[:, [0, 3]], reg_targets[:, [1, 4]], reg_targets[:, [2, 5]]
    c = (lr.min(dim=-1)[0] / lr.max(dim=-1)[0]) * (tb.min(dim=-1)[0] / tb.max(dim=-1)[0]) * \
        (fb.min(dim=-1)[0] / fb.max(dim=-1)[0])
    return torch.sqrt(c)


def _targets_composable(shapes, strides, gts, radius, norm, ranges, device, dtype):
    locations = compute_locations(shapes, strides, device)
    if dtype != torch.float32:
        locations = [l.to(dtype) for l in locations]
    P = [len(l) for l in locations]
    loc = torch.cat(locations, dim=0)

    def per_location(values):
        return torch.cat([torch.full((p,), float(v), dtype=dtype, device=device) for p, v in zip(P, values)])
    lo, hi = per_location([r[0] for r in ranges]), per_location([r[1] for r in ranges])
    reach = per_location([s * radius for s in strides])
    stride = per_location(strides)
    every = torch.arange(len(loc), device=device)
    per_scene = []
    for g in gts:
        if g.shape[0] == 0:
            per_scene.append((torch.zeros(len(loc), dtype=dtype, device=device), torch.zeros((len(loc), 6), dtype=dtype, device=device),
                              torch.zeros(len(loc), dtype=torch.int32, device=device)))
            continue
        reg = torch.cat((loc[:, None, :] - g[None, :, :3], g[None, :, 3:] - loc[:, None, :]), dim=2)
        if radius > 0:
            c = (g[:, :3] + g[:, 3:]) / 2
            cm, cp = c[None] - reach[:, None, None], c[None] + reach[:, None, None]
            rlo = torch.where(cm > g[None, :, :3], cm, g[None, :, :3].expand_as(cm))
            rhi = torch.where(cp > g[None, :, 3:], g[None, :, 3:].expand_as(cp), cp)
            inside = torch.cat((loc[:, None, :] - rlo, rhi - loc[:, None, :]), dim=2).min(dim=2)[0] > 0
        else:
            inside = reg.min(dim=2)[0] > 0
        largest = reg.max(dim=2)[0]
        cared = (largest >= lo[:, None]) & (largest <= hi[:, None])
        volume = ((g[:, 3] - g[:, 0]) * (g[:, 4] - g[:, 1])) * (g[:, 5] - g[:, 2])
        area = torch.where(inside & cared, volume[None].expand(len(loc), -1), torch.full_like(largest, INF))
        smallest, idx = area.min(dim=1)
        t = reg[every, idx]
        if norm:
            t = t / stride[:, None]
        per_scene.append(((smallest != INF).to(dtype), t, idx.to(torch.int32)))
    labels, reg, matched = [], [], []
    first = 0
    for p in P:                                           # level first, scenes inside a level
        for l, t, m in per_scene:
            labels.append(l[first:first + p])
            reg.append(t[first:first + p])
            matched.append(m[first:first + p])
        first += p
    labels, reg, matched = torch.cat(labels), torch.cat(reg), torch.cat(matched)
    ctr = torch.where(labels > 0, compute_centerness_targets(reg), torch.zeros_like(labels))
    return labels, reg, ctr, matched


def _valid_composable(shapes, strides, ori_sizes, device):
    masks = compute_padding_masks(compute_locations(shapes, strides, device), ori_sizes)
    return torch.cat([m.reshape(-1) for m in masks])


def _targets_fused(shapes, strides, gts, radius, norm, ranges, ori_sizes, device):
    lib = _lib.load()
    B, n = len(gts), len(shapes)
    total = B * sum(w * l * h for (w, l, h) in shapes)
    counts = [int(g.shape[0]) for g in gts]
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + c)
    gt = torch.cat([g.reshape(-1, 6) for g in gts]).contiguous() if offsets[-1] else None
    # two small host arrays go up without a synchronising copy; the result object keeps them alive (FCOSTargets._host)
    host = [torch.tensor(offsets, dtype=torch.int32)]
    off = host[0].to(device, non_blocking=True)
    ori = None
    if ori_sizes is not None:
        host.append(torch.tensor([[float(v) for v in o] for o in ori_sizes], dtype=torch.float32).reshape(B, 3))
        ori = host[1].to(device, non_blocking=True)
    labels = torch.empty((total,), dtype=torch.float32, device=device)
    reg = torch.empty((total, 6), dtype=torch.float32, device=device)
    ctr = torch.empty((total,), dtype=torch.float32, device=device)
    matched = torch.empty((total,), dtype=torch.int32, device=device)
    valid = torch.empty((total,), dtype=torch.uint8, device=device) if ori is not None else None
    dims = _host_i32([v for s in shapes for v in s])
    strd = _host_i32(strides)
    rng = (ctypes.c_float * (2 * n))(*[float(v) for r in ranges for v in r])
    with torch.cuda.device(device):
        _lib.check(lib.inr_fcos_targets(ctypes.cast(dims, _lib.P), ctypes.cast(strd, _lib.P), ctypes.cast(rng, _lib.P), n, B,
                                        _lib.ptr(gt, torch.float32, "gt_boxes", allow_none=True),
                                        _lib.ptr(off, torch.int32, "gt_offsets"), max(counts),
                                        _lib.ptr(ori, torch.float32, "ori_sizes", allow_none=True), float(radius), int(bool(norm)),
                                        _lib.ptr(labels), _lib.ptr(reg), _lib.ptr(ctr), _lib.ptr(matched),
                                        _lib.ptr(valid, torch.uint8, "valid", allow_none=True), _lib.stream_ptr()),
                   "fcos_targets")
    return labels, reg, ctr, matched, (valid.view(torch.bool) if valid is not None else None), host


def prepare_targets(feature_shapes, strides, gt_boxes, center_sampling_radius=1.5, norm_reg_targets=True,
                    sizes_of_interest=None, ori_sizes=None, fused=None):
    """The targets of every location (loss.py:269-436, the rule of include/inr.h) -> ``FCOSTargets``.  ``feature_shapes``:
    (W, L, H) per level; ``gt_boxes``: list per scene of [G_b, 6] (a scene with G_b == 0 gives zeros);
    ``sizes_of_interest``: (lo, hi) per level, default [-1, 16], [16, 32], [32, 64], [64, 1e8]; ``ori_sizes``: (w, l, h)
    per scene, the unpadded extents behind ``valid``.  Where the arg-min itself is in question (equal volumes, NaN) the
    kernel follows torch's CPU rule - the lowest index - while ``torch.min`` on a GPU may pick another index."""
    shapes, strides = _shapes(feature_shapes, strides)
    if not isinstance(gt_boxes, (list, tuple)) or len(gt_boxes) == 0:
        raise ValueError("gt_boxes must be a non-empty list of tensors [G, 6], one per scene")
    gts = [_gt(g) for g in gt_boxes]
    ranges = [tuple(r) for r in (sizes_of_interest if sizes_of_interest is not None else SIZES_OF_INTEREST[:len(shapes)])]
    if len(ranges) != len(shapes):
        raise ValueError(f"{len(shapes)} levels need {len(shapes)} sizes_of_interest (the default has {len(SIZES_OF_INTEREST)})")
    if not center_sampling_radius >= 0:
        raise ValueError("center_sampling_radius must be >= 0")
    if ori_sizes is not None and len(ori_sizes) != len(gts):
        raise ValueError(f"ori_sizes must have one (w, l, h) per scene ({len(gts)})")
    device, dtype = gts[0].device, gts[0].dtype
    if any(g.device != device or g.dtype != dtype for g in gts):
        raise ValueError("gt_boxes must share one device and dtype")
    total = len(gts) * sum(w * l * h for (w, l, h) in shapes)
    takes = (device.type == "cuda" and dtype == torch.float32 and len(shapes) <= FCOS_MAX_LEVELS and 6 * total < 2 ** 31
             and max(g.shape[0] for g in gts) <= FCOS_MAX_GT
             and all(max(s) * st < 2 ** 24 for s, st in zip(shapes, strides))
             # the ABI carries the radius as a float32: the kernels apply only where that changes no level's reach
             and all(_f32(st * center_sampling_radius) == _f32(st * _f32(center_sampling_radius)) for st in strides))
    if fused and not takes:
        raise RuntimeError(f"the fused FCOS targets take float32 GPU boxes, at most {FCOS_MAX_GT} per scene, and at most "
                           f"{FCOS_MAX_LEVELS} levels (got {dtype} on {device}, {max(g.shape[0] for g in gts)} boxes, "
                           f"{len(shapes)} levels); fused=None picks the composable path")
    if takes and (fused or (fused is None and TARGETS_FUSED_BY_DEFAULT)):
        out = _targets_fused(shapes, strides, gts, center_sampling_radius, norm_reg_targets, ranges, ori_sizes, device)
    else:
        out = _targets_composable(shapes, strides, gts, center_sampling_radius, norm_reg_targets, ranges, device, dtype)
        out += (_valid_composable(shapes, strides, ori_sizes, device) if ori_sizes is not None else None,)
    return FCOSTargets(shapes, strides, len(gts), *out)


# ---- losses ------------------------------------------------------------------------------------------------------------
def sigmoid_focal_terms(x, t, alpha=FOCAL_ALPHA, gamma=FOCAL_GAMMA):
    """torchvision.ops.sigmoid_focal_loss(x, t, alpha, gamma, reduction="none"), its published formula."""
    p = torch.sigmoid(x)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * ((1 - p_t) ** gamma)
    return (alpha * t + (1 - alpha) * (1 - t)) * loss


def iou_loss_terms(pred, target, loss_type):
    """IOULoss.forward (loss.py:85-126) without the reduction: the loss of each row of [N, 6] distances."""
    pl, pt, pf, pr, pb, pk = pred.unbind(1)
    tl, tt, tf, tr, tb, tk = target.unbind(1)
    target_volume = (tl + tr) * (tt + tb) * (tf + tk)
    pred_volume = (pl + pr) * (pt + pb) * (pf + pk)
    w = torch.min(pl, tl) + torch.min(pr, tr)
    gw = torch.max(pl, tl) + torch.max(pr, tr)
    h = torch.min(pb, tb) + torch.min(pt, tt)
    gh = torch.max(pb, tb) + torch.max(pt, tt)
    d = torch.min(pf, tf) + torch.min(pk, tk)
    gd = torch.max(pf, tf) + torch.max(pk, tk)
    ac = gw * gh * gd + 1e-7
    inter = w * h * d
    union = target_volume + pred_volume - inter
    ious = (inter + 1.0) / (union + 1.0)
    if loss_type == "iou":
        return -torch.log(ious)
    if loss_type == "linear_iou":
        return 1 - ious
    return 1 - (ious - (ac - union) / ac)


def _flatten_predictions(box_cls, box_regression, centerness):
    cls = torch.cat([c.permute(0, 2, 3, 4, 1).reshape(-1) for c in box_cls])
    reg = torch.cat([r.permute(0, 2, 3, 4, 1).reshape(-1, 6) for r in box_regression])
    ctr = torch.cat([c.reshape(-1) for c in centerness])
    return cls, reg, ctr


def loss_terms(box_cls, box_regression, centerness, targets, iou_loss_type="iou"):
    """The composable path's per-location terms -> (focal, regression term, centerness BCE, positives, centerness target),
    each [T] in the level-first order; a term is 0 where it does not apply.  Rows that are not positive enter the IoU and
    BCE formulas as ones, so neither a NaN nor a gradient leaks out of them."""
    cls, reg, ctr = _flatten_predictions(box_cls, box_regression, centerness)
    labels, regt = targets.labels_flat.to(cls.dtype), targets.reg_targets_flat.to(cls.dtype)
    valid = targets.valid_flat if targets.valid_flat is not None else torch.ones_like(labels, dtype=torch.bool)
    pos = valid & (labels > 0)
    zero = torch.zeros_like(cls)
    focal = torch.where(valid, sigmoid_focal_terms(torch.where(valid, cls, zero), labels), zero)
    one6 = torch.ones_like(regt)
    safe_t = torch.where(pos[:, None], regt, one6)
    cw = torch.where(pos, compute_centerness_targets(safe_t), zero)
    regterm = torch.where(pos, iou_loss_terms(torch.where(pos[:, None], reg, one6), safe_t, iou_loss_type) * cw, zero)
    bce = torch.where(pos, torch.nn.functional.binary_cross_entropy_with_logits(torch.where(pos, ctr, zero), cw,
                                                                                reduction="none"), zero)
    return focal, regterm, bce, pos, cw


def _reduce_norms(norms, world_size, group):
    """(n_pos, sum of centerness targets) summed over the ranks as ONE device tensor, divided by world_size."""
    if world_size <= 1:
        return norms
    import torch.distributed as dist
    norms = norms.clone()
    dist.all_reduce(norms, op=dist.ReduceOp.SUM, group=group)
    return norms / float(world_size)


def _finish(focal, weighted, bce, has, norms, dtype):
    n = norms[0].clamp(min=1.0)
    one = torch.ones_like(norms[1])
    return ((focal / n).to(dtype), torch.where(has, weighted / torch.where(has, norms[1], one), torch.zeros_like(weighted)).to(dtype),
            torch.where(has, bce / n, torch.zeros_like(bce)).to(dtype))


def _loss_composable(box_cls, box_regression, centerness, targets, iou_loss_type, world_size, group):
    focal, regterm, bce, pos, cw = loss_terms(box_cls, box_regression, centerness, targets, iou_loss_type)
    n_pos = pos.sum().to(focal.dtype)
    norms = _reduce_norms(torch.stack((n_pos, cw.sum())).detach(), world_size, group)
    return _finish(focal.sum(), regterm.sum(), bce.sum(), n_pos > 0, norms, focal.dtype)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _FusedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, targets, loss_type, world_size, group, n, *preds):
        lib = _lib.load()
        box_cls, box_reg, ctr = preds[:n], preds[n:2 * n], preds[2 * n:]
        dev = box_cls[0].device
        labels, regt, valid = targets.labels_flat, targets.reg_targets_flat, targets.valid_flat
        vbytes = valid.view(torch.uint8) if valid is not None else None
        total = labels.shape[0]
        dims = _host_i32([v for s in targets.feature_shapes for v in s])
        nbytes = int(lib.inr_fcos_loss_workspace_bytes(total))
        if nbytes < 0:
            _lib.check(nbytes, "fcos_loss_workspace_bytes")
        buf = torch.empty((nbytes // 8 + 5,), dtype=torch.float64, device=dev)          # partial sums, then sums [5]
        sums = buf[nbytes // 8:]
        losses = torch.empty((3,), dtype=torch.float32, device=dev)
        ptrs = [_ptr_array(box_cls), _ptr_array(box_reg), _ptr_array(ctr)]
        with torch.cuda.device(dev):
            _lib.check(lib.inr_fcos_loss_forward(*[ctypes.cast(p, _lib.P) for p in ptrs], ctypes.cast(dims, _lib.P), n, targets.B,
                                                 _lib.ptr(labels, torch.float32, "labels"), _lib.ptr(regt, torch.float32, "reg_targets"),
                                                 _lib.ptr(vbytes, torch.uint8, "valid", allow_none=True), loss_type,
                                                 ctypes.c_void_p(sums.data_ptr()), _lib.ptr(losses), None, None, None,
                                                 _lib.ptr(buf), nbytes, _lib.stream_ptr()), "fcos_loss_forward")
        norms = sums[3:5]
        if world_size > 1:
            norms = _reduce_norms(norms, world_size, group).contiguous()
            losses = torch.stack(_finish(sums[0], sums[1], sums[2], sums[3] > 0, norms, torch.float32))
        ctx.save_for_backward(norms, *preds)
        ctx.meta = (targets, loss_type, n)
        return losses

    @staticmethod
    def backward(ctx, grad_losses):
        lib = _lib.load()
        targets, loss_type, n = ctx.meta
        norms, preds = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        box_cls, box_reg, ctr = preds[:n], preds[n:2 * n], preds[2 * n:]
        dev = box_cls[0].device
        grads = [torch.empty_like(p) for p in preds]
        valid = targets.valid_flat
        vbytes = valid.view(torch.uint8) if valid is not None else None
        dims = _host_i32([v for s in targets.feature_shapes for v in s])
        g = grad_losses.to(torch.float32).contiguous()
        ptrs = [_ptr_array(box_cls), _ptr_array(box_reg), _ptr_array(ctr), _ptr_array(grads[:n]), _ptr_array(grads[n:2 * n]),
                _ptr_array(grads[2 * n:])]
        with torch.cuda.device(dev):
            _lib.check(lib.inr_fcos_loss_backward(*[ctypes.cast(p, _lib.P) for p in ptrs[:3]], ctypes.cast(dims, _lib.P), n,
                                                  targets.B, _lib.ptr(targets.labels_flat), _lib.ptr(targets.reg_targets_flat),
                                                  _lib.ptr(vbytes, torch.uint8, "valid", allow_none=True), loss_type,
                                                  ctypes.c_void_p(norms.data_ptr()), _lib.ptr(g),
                                                  *[ctypes.cast(p, _lib.P) for p in ptrs[3:]], _lib.stream_ptr()),
                       "fcos_loss_backward")
        return (None, None, None, None, None, *grads)


def _check_predictions(box_cls, box_regression, centerness, targets):
    n = len(targets.feature_shapes)
    if not (len(box_cls) == len(box_regression) == len(centerness) == n):
        raise ValueError(f"the targets have {n} levels: box_cls, box_regression and centerness need {n} tensors each")
    for l, (c, r, k) in enumerate(zip(box_cls, box_regression, centerness)):
        w = (targets.B,) + tuple(targets.feature_shapes[l])
        if tuple(c.shape) != (w[0], 1) + w[1:] or tuple(r.shape) != (w[0], 6) + w[1:] or tuple(k.shape) != (w[0], 1) + w[1:]:
            if r.dim() == 5 and r.shape[1] == 8:
                raise ValueError("box_regression: oriented boxes (8 channels) are not supported")
            raise ValueError(f"level {l}: expected box_cls / centerness [{w[0]}, 1, {w[1]}, {w[2]}, {w[3]}] and box_regression "
                             f"[{w[0]}, 6, ...], got {tuple(c.shape)}, {tuple(r.shape)}, {tuple(k.shape)}")


def fcos_loss(box_cls, box_regression, centerness, targets, iou_loss_type="iou", world_size=1, group=None, fused=None):
    """-> (cls_loss, reg_loss, centerness_loss), 0-dim tensors, differentiable with respect to the three lists of
    predictions (loss.py:477-591).  ``box_cls`` / ``centerness``: per level [B, 1, W, L, H]; ``box_regression``: per level
    [B, 6, W, L, H]; ``targets``: what ``prepare_targets`` returned.  With ``world_size > 1`` the number of positives and
    the sum of the centerness targets are all-reduced over ``group`` as one device tensor and divided by ``world_size``."""
    if iou_loss_type not in LOSS_TYPES:
        if iou_loss_type in ("smooth_l1", "diou"):
            raise NotImplementedError(f"iou_loss_type {iou_loss_type!r} is not supported (iou, linear_iou, giou)")
        raise ValueError(f"iou_loss_type must be one of {sorted(LOSS_TYPES)}, got {iou_loss_type!r}")
    if not isinstance(targets, FCOSTargets):
        raise ValueError("targets must be the result of prepare_targets")
    _check_predictions(box_cls, box_regression, centerness, targets)
    preds = list(box_cls) + list(box_regression) + list(centerness)
    dev = targets.labels_flat.device
    takes = (dev.type == "cuda" and targets.labels_flat.dtype == torch.float32
             and all(p.device == dev and p.dtype == torch.float32 and p.is_contiguous() for p in preds))
    if fused and not takes:
        raise RuntimeError("the fused FCOS loss takes contiguous float32 GPU predictions and targets on one device; "
                           "fused=None picks the composable path")
    if takes and (fused or (fused is None and LOSS_FUSED_BY_DEFAULT)):
        losses = _FusedLoss.apply(targets, LOSS_TYPES[iou_loss_type], int(world_size), group, len(box_cls), *preds)
        return losses[0], losses[1], losses[2]
    return _loss_composable(box_cls, box_regression, centerness, targets, iou_loss_type, int(world_size), group)


class FCOSLossComputation:
    """The reference's class (loss.py:174-591) over ``prepare_targets`` and ``fcos_loss``, for drop-in use."""

    def __init__(self, fpn_strides, center_sampling_radius, iou_loss_type, norm_reg_targets, world_size=1, use_obb=False,
                 use_additional_l1_loss=False, proj2d_loss_weight=0.0, fused=None):
        if use_obb:
            raise NotImplementedError("use_obb=True: oriented boxes are not supported")
        if iou_loss_type in ("smooth_l1", "diou"):
            raise NotImplementedError(f"iou_loss_type {iou_loss_type!r} is not supported (iou, linear_iou, giou)")
        if iou_loss_type not in LOSS_TYPES:
            raise ValueError(f"iou_loss_type must be one of {sorted(LOSS_TYPES)}, got {iou_loss_type!r}")
        if proj2d_loss_weight > 0:
            raise NotImplementedError("proj2d_loss_weight > 0: the 2-D projection loss is not supported")
        self.fpn_strides, self.center_sampling_radius = list(fpn_strides), center_sampling_radius
        self.iou_loss_type, self.norm_reg_targets, self.world_size, self.fused = iou_loss_type, norm_reg_targets, world_size, fused

    def prepare_targets(self, feature_shapes, targets, ori_sizes=None):
        return prepare_targets(feature_shapes, self.fpn_strides[:len(feature_shapes)], targets, self.center_sampling_radius,
                               self.norm_reg_targets, ori_sizes=ori_sizes, fused=self.fused)

    def __call__(self, locations, box_cls, box_regression, centerness, targets, padding_masks=None):
        """``locations`` are implied by the predictions' shapes and the strides; the argument is kept for the reference's
        signature.  ``padding_masks``: list per level of bool [B, P_l], or None."""
        t = self.prepare_targets([tuple(c.shape[-3:]) for c in box_cls], targets)
        if padding_masks is not None:
            t = t.with_valid(torch.cat([m.reshape(-1) for m in padding_masks]).to(torch.bool).contiguous())
        return fcos_loss(box_cls, box_regression, centerness, t, self.iou_loss_type, self.world_size, fused=self.fused)
