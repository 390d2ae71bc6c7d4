"""The reference's multi-scale pooler (/root/reference/nerf_rcnn/model/poolers.py: ``LevelMapper``,
``MultiScaleRoIAlign3D``, ``_multiscale_roi_align_3d``) with the pyramid pooled in ONE launch.

The reference maps every box to a pyramid level and then, per level, runs ``torch.where`` (a read-back of the result
size), a gather of the RoIs, one extension call and an indexed scatter, plus one more ``torch.where`` per image.  The
fused path here hands all levels to ``inr_roi_align_3d_pyramid_forward``: every RoI names its level, row k of the result
is RoI k, and the per-image results are views (``split``) - nothing between entry and return synchronises with the host,
in the forward or in the backward, so the call can be captured in a graph.

Swap into the reference (its own class passes the ``isinstance`` checks of nerf_rcnn.py:151-160):

    import model.poolers as mp, instance_nerf_amd.roi_align as ra
    mp._multiscale_roi_align_3d = ra.multiscale_roi_align_3d
"""
import ctypes

import torch
from torch import nn

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .roi_align import roi_align_3d


class LevelMapper:
    """Eqn. 1 of the FPN paper on box volumes, float32 operation by operation as the reference's (poolers.py:24-61):
    level = floor(canonical_level + log2(cbrt(volume) / canonical_scale) + eps), clamped to [k_min, k_max], returned as
    an int64 index from k_min.  Takes the list of per-image box tensors."""

    def __init__(self, k_min, k_max, canonical_scale=160, canonical_level=4, eps=1e-6):
        self.k_min = k_min
        self.k_max = k_max
        self.s0 = canonical_scale
        self.lvl0 = canonical_level
        self.eps = eps

    def __call__(self, boxlists):
        b = torch.cat(list(boxlists), dim=0)
        side = torch.pow((b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2]), 1.0 / 3.0)
        lvl = torch.floor(self.lvl0 + torch.log2(side / self.s0) + torch.tensor(self.eps, dtype=side.dtype))
        return torch.clamp(lvl, min=self.k_min, max=self.k_max).to(torch.int64) - self.k_min


def level_order(levels):
    """The ``order`` argument of the pyramid call: the stable argsort of the levels (int32 [K]) - workgroup slot i
    handles RoI order[i], so the workgroups resident at one time read one level."""
    return torch.argsort(levels, stable=True).to(torch.int32)


def infer_scale(feature, original_size):
    """poolers.py:75-83: 2 ** round(log2(s1 / s2)) - of the FIRST axis only, as the reference returns it."""
    approx = float(feature.shape[-3]) / float(original_size[0])
    return 2 ** float(torch.tensor(approx).log2().round())


def setup_scales(features, image_shapes, canonical_scale, canonical_level):
    """poolers.py:86-112: one scale per level from the largest image extents; k_min / k_max from the first / last scale."""
    if not image_shapes:
        raise ValueError("images list should not be empty")
    original = tuple(max(int(shape[a]) for shape in image_shapes) for a in range(3))
    scales = [infer_scale(f, original) for f in features]
    k_min = -torch.log2(torch.tensor(scales[0], dtype=torch.float32)).item()
    k_max = -torch.log2(torch.tensor(scales[-1], dtype=torch.float32)).item()
    return scales, LevelMapper(int(k_min), int(k_max), canonical_scale=canonical_scale, canonical_level=canonical_level)


def _level_table(tensors, shapes, scales):
    """The host arrays of the C ABI's level table; a None tensor gives a null pointer (backward: no gradient)."""
    n = len(shapes)
    ptrs = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in tensors])
    dims = (ctypes.c_int32 * (3 * n))(*[int(v) for s in shapes for v in s[2:]])
    sc = (ctypes.c_float * n)(*[float(s) for s in scales])
    return ptrs, dims, sc


class _PyramidRoIAlign3D(torch.autograd.Function):
    """One pyramid call each way; the feature maps are the variadic inputs, one gradient per level comes back (zeros for
    a level without RoIs, None for one that does not require grad)."""

    @staticmethod
    def forward(ctx, rois, roi_inds, levels, order, output_size, scales, *features):
        lib = _lib.load()
        n = len(features)
        if not 1 <= n <= _lib.ROI_MAX_LEVELS:
            raise RuntimeError(f"multiscale_roi_align_3d: 1..{_lib.ROI_MAX_LEVELS} pyramid levels, got {n}")
        features = [f.contiguous() for f in features]
        N, C = features[0].shape[:2]
        for l, f in enumerate(features):
            ptr(f, torch.float32, f"x_filtered[{l}]", allow_none=f.numel() == 0)
            if f.dim() != 5 or f.shape[0] != N or f.shape[1] != C:
                raise RuntimeError("multiscale_roi_align_3d: every level must be [N,C,W,L,H] with the same N and C")
        K = rois.shape[0]
        ow, ol, oh = output_size
        out = torch.empty(K, C, ow, ol, oh, dtype=torch.float32, device=rois.device)
        shapes = [tuple(f.shape) for f in features]
        ptrs, dims, sc = _level_table(features, shapes, scales)
        check(lib.inr_roi_align_3d_pyramid_forward(
            ptrs, dims, sc, n, ptr(rois, torch.float32, "rois", allow_none=K == 0),
            ptr(roi_inds, torch.int32, "roi_inds", allow_none=K == 0),
            ptr(levels, torch.int32, "levels", allow_none=K == 0), ptr(order, torch.int32, "order", allow_none=True),
            N, C, K, ow, ol, oh, ptr(out, allow_none=K == 0), stream_ptr()), "roi_align_3d_pyramid_forward")
        ctx.save_for_backward(rois, roi_inds, levels, *([] if order is None else [order]))
        ctx.shapes, ctx.scales, ctx.output_size = shapes, list(scales), (ow, ol, oh)
        return out

    @staticmethod
    def backward(ctx, grad):
        lib = _lib.load()
        rois, roi_inds, levels, *rest = ctx.saved_tensors
        order = rest[0] if rest else None
        shapes = ctx.shapes
        N, C = shapes[0][:2]
        K = rois.shape[0]
        ow, ol, oh = ctx.output_size
        grad = grad.contiguous().float()
        grads = [torch.zeros(s, dtype=torch.float32, device=grad.device) if need else None
                 for s, need in zip(shapes, ctx.needs_input_grad[6:])]
        if K > 0 and N > 0 and any(g is not None for g in grads):
            ptrs, dims, sc = _level_table(grads, shapes, ctx.scales)
            check(lib.inr_roi_align_3d_pyramid_backward(
                ptrs, dims, sc, len(shapes), ptr(rois), ptr(roi_inds), ptr(levels), ptr(order, allow_none=True),
                N, C, K, ow, ol, oh, ptr(grad), stream_ptr()), "roi_align_3d_pyramid_backward")
        return (None,) * 6 + tuple(grads)


def pyramid_roi_align_3d(features, rois, roi_inds, levels, output_size, scales, order=None):
    """features: list of f32[N,C,W_l,L_l,H_l]; rois f32[K,6]; roi_inds, levels int32[K]; order int32[K] or None
    -> f32[K,C,ow,ol,oh], row k = RoI k pooled from features[levels[k]] at scales[levels[k]] (zeros for a level outside
    the list).  Differentiable w.r.t. every feature map."""
    return _PyramidRoIAlign3D.apply(rois, roi_inds, levels, order, tuple(int(v) for v in output_size),
                                    tuple(float(s) for s in scales), *features)


def multiscale_roi_align_3d(x_filtered, boxes, output_size, sampling_ratio, scales, mapper, fused=True, roi_align=None):
    """The reference's ``_multiscale_roi_align_3d`` (poolers.py:115-188; same positional signature).  x_filtered: the
    pyramid levels [N,C,W_l,L_l,H_l]; boxes: one [n_i,6] tensor per image, in image units.  One level: a single tensor
    from a plain ``roi_align_3d``; several: a list with one float32 tensor per image.  ``sampling_ratio`` is accepted
    and never forwarded, as in the reference (utils.py:597,608).

    fused (GPU tensors): one ``inr_roi_align_3d_pyramid_forward`` call, no host synchronisation.  fused=False, a given
    ``roi_align`` or CPU tensors: the reference's per-level loop restated around ``roi_align`` (default: the product's
    ``roi_align_3d``; signature (input, rois, roi_inds, out_w, out_l, out_h, spatial_scale))."""
    if scales is None or mapper is None:
        raise ValueError("scales and mapper should not be None")
    if isinstance(output_size, int):
        output_size = (output_size,) * 3
    ow, ol, oh = (int(v) for v in output_size)
    composable = (not fused) or roi_align is not None or not x_filtered[0].is_cuda
    if roi_align is None:
        roi_align = roi_align_3d
    counts = [int(b.shape[0]) for b in boxes]
    rois = torch.cat(list(boxes), dim=0)
    # the image index of every RoI, built on the device from lengths the host already knows
    roi_inds = torch.cat([torch.full((n,), i, dtype=torch.int32, device=rois.device) for i, n in enumerate(counts)])

    if len(x_filtered) == 1:
        return roi_align(x_filtered[0], rois, roi_inds, ow, ol, oh, scales[0])

    levels = mapper(boxes)
    if not composable:
        levels = levels.to(torch.int32)
        result = pyramid_roi_align_3d(list(x_filtered), rois.contiguous().float(), roi_inds, levels, (ow, ol, oh), scales,
                                      order=level_order(levels))
        return list(result.split(counts))

    C = x_filtered[0].shape[1]
    result = torch.zeros((rois.shape[0], C, ow, ol, oh), dtype=torch.float32, device=rois.device)
    for level, (feature, scale) in enumerate(zip(x_filtered, scales)):
        idx = torch.where(levels == level)[0]
        if idx.shape[0] == 0:
            continue
        result[idx] = roi_align(feature, rois[idx], roi_inds[idx], ow, ol, oh, scale).to(result.dtype)
    return [result[torch.where(roi_inds == b)] for b in range(len(boxes))]


class MultiScaleRoIAlign3D(nn.Module):
    """The reference's module (poolers.py:191-281), same constructor and ``forward(x, boxes, image_shapes)``: scales and
    the level mapper are inferred on the first call and then kept.  ``fused`` / ``roi_align`` (attributes) choose the
    path of ``multiscale_roi_align_3d``."""

    def __init__(self, output_size, sampling_ratio, *, canonical_scale=160, canonical_level=4):
        super().__init__()
        if isinstance(output_size, int):
            output_size = (output_size, output_size, output_size)
        self.sampling_ratio = sampling_ratio
        self.output_size = tuple(output_size)
        self.scales = None
        self.map_levels = None
        self.canonical_scale = canonical_scale
        self.canonical_level = canonical_level
        self.fused = True
        self.roi_align = None

    def forward(self, x, boxes, image_shapes):
        if self.scales is None or self.map_levels is None:
            self.scales, self.map_levels = setup_scales(x, image_shapes, self.canonical_scale, self.canonical_level)
        return multiscale_roi_align_3d(x, boxes, self.output_size, self.sampling_ratio, self.scales, self.map_levels,
                                       fused=self.fused, roi_align=self.roi_align)

    def __repr__(self):
        return f"{self.__class__.__name__}(output_size={self.output_size}, sampling_ratio={self.sampling_ratio})"
