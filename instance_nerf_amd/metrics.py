"""Scores of rendered views.

Image quality: SSIM, MSE and PSNR from one fused launch (csrc/ssim.hip, include/inr.h "Image quality of rendered views"),
and the composable torch path with the same window and formula - the CPU path and the on-GPU baseline.

Segmentation: the confusion matrix of rendered instance maps from one fused launch (csrc/confusion.hip, include/inr.h
"Segmentation confusion matrix of rendered instance maps") or one ``torch.bincount`` (``segmentation_confusion``), and the
scores that follow from its integers on the host - mIoU, pixel accuracy, panoptic quality (``segmentation_scores``).

Semantics (the header states them once): channels-last float images [B, H, W, C] or [H, W, C]; separable 11-tap Gaussian
window, sigma 1.5, normalised in binary64 and rounded to binary32 (``gaussian_window``); valid windows only, so the map is
[B, H-10, W-10, C] (believed to equal torchmetrics' reflect-pad-then-crop default; not verified); the per-image SSIM is the
mean of the map; non-finite inputs are not masked.  Nothing here reads back to the host.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

TAPS, SIGMA = _lib.SSIM_TAPS, 1.5
TILE = (_lib.SSIM_TILE_W, _lib.SSIM_TILE_H)      # map pixels per workgroup of the fused kernel (width, height)
# profiles/ssim_probe.json: the fused call is faster than the composable path at every measured size, so fused=None takes it
FUSED_BY_DEFAULT = True


def gaussian_window():
    """The eleven binary32 window values of the contract, as a numpy array."""
    i = np.arange(TAPS, dtype=np.float64)
    g = np.exp(-(i - TAPS // 2) ** 2 / (2.0 * SIGMA ** 2))
    return (g / g.sum()).astype(np.float32)


_WINDOW = gaussian_window()
_WINDOW_PTR = _WINDOW.ctypes.data_as(ctypes.c_void_p)
_RANGES = {}


def _check_images(pred, truth):
    if pred.shape != truth.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and truth {tuple(truth.shape)} must have the same shape")
    if pred.dim() not in (3, 4):
        raise ValueError(f"images must be [B, H, W, C] or [H, W, C], got {tuple(pred.shape)}")
    if pred.device != truth.device:
        raise ValueError(f"pred is on {pred.device}, truth on {truth.device}")
    H, W = pred.shape[-3], pred.shape[-2]
    if H < TAPS or W < TAPS:
        raise ValueError(f"SSIM needs H and W of at least {TAPS} (one full window), got H = {H}, W = {W}")
    if pred.shape[-1] < 1 or (pred.dim() == 4 and pred.shape[0] < 1):
        raise ValueError(f"empty images: {tuple(pred.shape)}")


def _range_tensor(pred, truth, data_range):
    """L as ONE float32 on the images' device: a cached constant, or the range inferred by device reductions."""
    if data_range is None:
        p, t = pred.detach().float(), truth.detach().float()
        return torch.maximum(p.max() - p.min(), t.max() - t.min()).reshape(1)
    if torch.is_tensor(data_range):
        return data_range.detach().to(device=pred.device, dtype=torch.float32).reshape(1)
    key = (pred.device, float(data_range))
    if key not in _RANGES:
        if len(_RANGES) > 64:
            _RANGES.clear()
        _RANGES[key] = torch.full((1,), float(data_range), dtype=torch.float32, device=pred.device)
    return _RANGES[key]


def _kernel_takes(pred, truth):
    return (pred.is_cuda and truth.is_cuda and pred.dtype == torch.float32 and truth.dtype == torch.float32
            and pred.is_contiguous() and truth.is_contiguous() and 1 <= pred.shape[-1] <= 4
            and pred.numel() < 2 ** 31 and pred.shape[0] <= 65535
            and -(-(pred.shape[1] - TAPS + 1) // TILE[1]) <= 65535)        # the library's limits: images and tile rows per launch


def _fused(pred, truth, L, return_map):
    B, H, W, C = pred.shape
    lib = _lib.load()
    need = lib.inr_ssim_workspace_bytes(B, H, W, C)
    if need < 0:
        _lib.check(int(need), "ssim_workspace_bytes")
    dev = pred.device
    workspace = torch.empty((need // 8,), dtype=torch.float64, device=dev)
    ssim = torch.empty((B,), dtype=torch.float32, device=dev)
    sse = torch.empty((B,), dtype=torch.float32, device=dev)
    ssim_map = torch.empty((B, H - TAPS + 1, W - TAPS + 1, C), dtype=torch.float32, device=dev) if return_map else None
    with torch.cuda.device(dev):
        _lib.check(lib.inr_ssim_forward(_lib.ptr(pred, torch.float32, "pred"), _lib.ptr(truth, torch.float32, "truth"), B, H, W, C,
                                        _WINDOW_PTR, _lib.ptr(L, torch.float32, "data_range"), _lib.ptr(ssim), _lib.ptr(sse),
                                        _lib.ptr_or_null(ssim_map), _lib.ptr(workspace), need, _lib.stream_ptr()),
                   "ssim_forward")
    return ssim, sse, ssim_map


def _composable(pred, truth, L):
    """Grouped F.conv2d with the same eleven weights and the same formula.  Moments are taken about one pivot per image and
    channel (the truth pixel at the first window centre, 0 when not finite), as the kernel does per tile."""
    work = torch.float64 if pred.dtype == torch.float64 else torch.float32
    x, y = pred.to(work).permute(0, 3, 1, 2), truth.to(work).permute(0, 3, 1, 2)        # [B, C, H, W] views
    C = x.shape[1]
    g = torch.from_numpy(_WINDOW).to(device=x.device, dtype=work)
    gw, gh = g.reshape(1, 1, 1, TAPS).repeat(C, 1, 1, 1), g.reshape(1, 1, TAPS, 1).repeat(C, 1, 1, 1)

    def windowed(a):
        return F.conv2d(F.conv2d(a, gw, groups=C), gh, groups=C)

    pivot = y[:, :, TAPS // 2:TAPS // 2 + 1, TAPS // 2:TAPS // 2 + 1]
    pivot = torch.where(torch.isfinite(pivot), pivot, torch.zeros_like(pivot))
    xs, ys = x - pivot, y - pivot
    sx, sy = windowed(xs), windowed(ys)
    vx, vy, cov = windowed(xs * xs) - sx * sx, windowed(ys * ys) - sy * sy, windowed(xs * ys) - sx * sy
    mx, my = sx + pivot, sy + pivot
    L = L.to(work)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    m = ((2 * (mx * my) + C1) * (2 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    ssim = m.double().mean(dim=(1, 2, 3)).float()
    d = x - y
    sse = (d * d).double().sum(dim=(1, 2, 3)).float()
    return ssim, sse, m.permute(0, 2, 3, 1).float()


def image_quality(pred, truth, data_range=1.0, return_map=False, fused=None):
    """-> dict(ssim [B], mse [B], psnr [B] (, map [B, H-10, W-10, C])), float32 on the images' device.

    ``data_range``: L of C1 = (0.01 L)^2, C2 = (0.03 L)^2; None infers max(pred.max() - pred.min(), truth.max() - truth.min())
    over the whole call, on the device.  ``fused``: None picks the kernel for contiguous float32 GPU images of 1..4
    channels and the composable path for everything else; True insists on the kernel (RuntimeError when it does not take
    the input); False is the composable path.  psnr = -10 log10(max(mse, 1e-12)), PSNRMeter's rule."""
    _check_images(pred, truth)
    squeeze = pred.dim() == 3
    pred, truth = pred.detach(), truth.detach()
    if squeeze:
        pred, truth = pred[None], truth[None]
    L = _range_tensor(pred, truth, data_range)
    takes = _kernel_takes(pred, truth)
    if fused and not takes:
        raise RuntimeError("the fused SSIM kernel takes contiguous float32 GPU images [B, H, W, C] with 1 <= C <= 4 "
                           f"(got {pred.dtype}, {tuple(pred.shape)}, {pred.device}); fused=None picks the composable path")
    if takes and (fused or (fused is None and FUSED_BY_DEFAULT)):
        ssim, sse, ssim_map = _fused(pred, truth, L, return_map)
    else:
        ssim, sse, ssim_map = _composable(pred, truth, L)
    mse = sse / float(pred.shape[1] * pred.shape[2] * pred.shape[3])
    out = {"ssim": ssim, "mse": mse, "psnr": -10.0 * torch.log10(torch.clamp(mse, min=1e-12))}
    if return_map:
        out["map"] = ssim_map
    return out


def ssim(pred, truth, **kw):
    """Per-image SSIM [B] (``image_quality``'s arguments)."""
    return image_quality(pred, truth, **kw)["ssim"]


# ---- segmentation: confusion matrix and the scores derived from it ---------------------------------------------------
CONFUSION_MAX_K = _lib.CONFUSION_MAX_K
# profiles/segmentation_probe.json (tools/segmentation_probe.py): both fused entries are faster than the composable path
# (argmax + bincount) on the same GPU inputs in every measured shape, so fused=None takes them; a fused form that loses
# there sends the default back to the composable path
CONFUSION_FUSED_BY_DEFAULT = True


def _as_int32(t, K):
    """Ids as int32 on their device.  64-bit ids are clamped into [-1, K] first: every value outside [0, K) means the
    same thing (include/inr.h), and a plain narrowing would wrap 2^32 to 0."""
    if t.dtype == torch.int32:
        return t
    if t.dtype.itemsize == 8:
        t = t.clamp(-1, K)
    return t.to(torch.int32)


def _confusion_inputs(pred, truth, K):
    if not isinstance(K, int) or K < 1:
        raise ValueError(f"num_classes must be a positive integer, got {K!r}")
    if truth.dtype.is_floating_point or truth.dtype == torch.bool or truth.dtype.is_complex:
        raise ValueError(f"truth must hold integer ids, got {truth.dtype}")
    if pred.device != truth.device:
        raise ValueError(f"pred is on {pred.device}, truth on {truth.device}")
    logits = pred.dtype.is_floating_point
    if logits:
        if pred.shape[:-1] != truth.shape or pred.dim() < 1:
            raise ValueError(f"logits {tuple(pred.shape)} must have the shape of truth {tuple(truth.shape)} plus one "
                             "trailing channel dimension")
        if pred.shape[-1] < K:
            raise ValueError(f"logits have {pred.shape[-1]} channels, fewer than num_classes = {K}")
    elif pred.dtype == torch.bool or pred.dtype.is_complex or pred.shape != truth.shape:
        raise ValueError(f"predicted ids must be integers of truth's shape {tuple(truth.shape)}, got {pred.dtype} "
                         f"{tuple(pred.shape)}")
    B = truth.shape[0] if truth.dim() >= 2 else 1
    truth = truth.reshape(B, -1)
    pred = pred.reshape(B, truth.shape[1], pred.shape[-1]) if logits else pred.reshape(B, -1)
    return pred, truth, logits, B


def _confusion_kernel_takes(pred, truth, logits, K):
    return (truth.is_cuda and K <= CONFUSION_MAX_K
            and (not logits or (pred.dtype == torch.float32 and pred.is_contiguous())))


def _confusion_fused(pred, truth, logits, K, counts, ignored):
    B, N = truth.shape
    lib = _lib.load()
    truth = _as_int32(truth, K).contiguous()
    with torch.cuda.device(truth.device):
        if logits:
            _lib.check(lib.inr_confusion_logits(_lib.ptr_or_null(pred, torch.float32, "logits"),
                                                _lib.ptr_or_null(truth, torch.int32, "truth"), B, N, K, pred.shape[-1],
                                                _lib.ptr_or_null(counts, torch.int64, "counts"),
                                                _lib.ptr_or_null(ignored, torch.int64, "ignored"), _lib.stream_ptr()),
                       "confusion_logits")
        else:
            pred = _as_int32(pred, K).contiguous()
            _lib.check(lib.inr_confusion_ids(_lib.ptr_or_null(pred, torch.int32, "pred"),
                                             _lib.ptr_or_null(truth, torch.int32, "truth"), B, N, K,
                                             _lib.ptr_or_null(counts, torch.int64, "counts"),
                                             _lib.ptr_or_null(ignored, torch.int64, "ignored"), _lib.stream_ptr()),
                       "confusion_ids")


def _confusion_composable(pred, truth, logits, K, counts, ignored):
    """One bincount: kept pixels go to bin (b, t, p or K), ignored ones to one extra bin per image - nothing is read back."""
    B, N = truth.shape
    if logits:
        pred = torch.argmax(pred[..., :K], dim=-1)
    p, t = pred.long(), truth.long()
    image = torch.arange(B, device=t.device).reshape(B, 1)
    keep = (t >= 0) & (t < K)
    col = torch.where((p >= 0) & (p < K), p, torch.full_like(p, K))
    cells = B * K * (K + 1)
    bins = torch.where(keep, (image * K + t) * (K + 1) + col, cells + image)
    hist = torch.bincount(bins.reshape(-1), minlength=cells + B)
    counts += hist[:cells].reshape(B, K, K + 1)
    ignored += hist[cells:]


def segmentation_confusion(pred, truth, num_classes, out=None, fused=None):
    """-> (counts int64 [B, K, K+1], ignored int64 [B]) on the inputs' device: the confusion matrix of include/inr.h
    ("Segmentation confusion matrix of rendered instance maps"), K = ``num_classes``.

    ``truth``: integer ids, [B, ...] (two or more dimensions: the leading extent is B) or one flat image [N]; a single
    [H, W] map must be passed as [1, H, W].  ``pred``: integer ids of truth's shape (any integer dtype; made int32 on the
    device when needed), or floating-point logits with one more trailing dimension of at least K channels, of which only
    the first K are candidates of the arg-max.  ``out=(counts, ignored)``: accumulate into these in place (and return
    them) instead of into fresh zeros.  Nothing is read back.

    ``fused``: None picks the kernel for GPU tensors with K <= 64 (logits: contiguous float32) and the composable path -
    ``torch.argmax`` then one ``torch.bincount`` - for CPU tensors, K > 64 and everything else; True insists on the kernel
    (RuntimeError when it does not take the input); False is the composable path.  Both give the same integers, except
    where the arg-max itself is in question: the kernel follows the contract's rule (NaN above every number, lowest index
    among equals - torch.argmax on CPU tensors), while torch.argmax on a GPU may pick another index among NaNs or ties."""
    K = num_classes
    pred, truth, logits, B = _confusion_inputs(pred.detach(), truth.detach(), K)
    if out is None:
        counts = torch.zeros((B, K, K + 1), dtype=torch.int64, device=truth.device)
        ignored = torch.zeros((B,), dtype=torch.int64, device=truth.device)
    else:
        counts, ignored = out
        for name, t, shape in (("counts", counts, (B, K, K + 1)), ("ignored", ignored, (B,))):
            if t.dtype != torch.int64 or tuple(t.shape) != shape or t.device != truth.device or not t.is_contiguous():
                raise ValueError(f"out: {name} must be a contiguous int64 {shape} tensor on {truth.device}, got {t.dtype} "
                                 f"{tuple(t.shape)} on {t.device}")
    takes = _confusion_kernel_takes(pred, truth, logits, K)
    if fused and not takes:
        raise RuntimeError(f"the fused confusion kernel takes GPU tensors with num_classes <= {CONFUSION_MAX_K} and, for "
                           f"logits, contiguous float32 (got {pred.dtype}, {tuple(pred.shape)}, {pred.device}, K = {K}); "
                           "fused=None picks the composable path")
    if takes and (fused or (fused is None and CONFUSION_FUSED_BY_DEFAULT)):
        _confusion_fused(pred, truth, logits, K, counts, ignored)
    else:
        _confusion_composable(pred, truth, logits, K, counts, ignored)
    return counts, ignored


def _ratio(num, den):
    return float(num) / float(den) if den else 0.0


def _panoptic(iou, match, gt_ids, pred_ids):
    """PQ / SQ / RQ and the counts over the given present truth and predicted ids; `match` [K] holds partners or -1."""
    pairs = [(g, int(match[g])) for g in gt_ids if match[g] >= 0]
    tp = len(pairs)
    fn, fp = len(gt_ids) - tp, len(pred_ids) - tp
    total = float(np.sum(np.array([iou[g, p] for g, p in pairs], dtype=np.float64))) if pairs else 0.0
    den = tp + 0.5 * fp + 0.5 * fn
    return {"pq": _ratio(total, den), "sq": _ratio(total, tp), "rq": _ratio(tp, den), "tp": tp, "fp": fp, "fn": fn}


def segmentation_scores(counts, stuff_ids=(0,), match="id"):
    """Scores of a confusion matrix ``counts`` ([B, K, K+1] - summed over B first - or [K, K+1]; include/inr.h), on the
    host, in float64, from the integers.  -> dict:

    ``iou`` float64 [K] (I_k / U_k, NaN where U_k = 0), ``miou_gt_ids`` (mean over T_k > 0), ``miou_all_ids`` (mean over
    U_k > 0; both 0.0 over an empty set; bit for bit nerf.utils.MIoUMeter.measure_both() on the same pixels), ``pixel_acc``
    = sum I_k / sum T_g; with T_g the row sums (column K included), P_p the column sums for p < K, I_k = counts[k, k],
    U_k = T_k + P_k - I_k.
    Panoptic quality over the truth segments g with T_g > 0 and predicted segments p with P_p > 0: IoU(g, p) =
    counts[g, p] / (T_g + P_p - counts[g, p]); a pair is a true positive when IoU > 0.5 strictly (so a segment has at
    most one partner).  ``match="id"``: only g == p may match (prediction and truth share a numbering, as after
    match_seg); ``match="any"``: any pair of ids outside ``stuff_ids`` may match - the score does not change when the
    predicted thing ids are relabelled - and an id in ``stuff_ids`` matches only itself.  ``pq`` = sum of the matched IoU
    / (TP + FP/2 + FN/2), ``sq`` = that sum / TP, ``rq`` = TP / (TP + FP/2 + FN/2), 0.0 for a zero denominator; ``tp``,
    ``fp``, ``fn`` integers; ``matches`` int64 [K], the partner of each truth id or -1; ``pq_things`` / ``sq_things`` /
    ``rq_things``: the same over the segments outside ``stuff_ids``.  The matrix of all views of a scene gives the
    scene-level figures."""
    if match not in ("id", "any"):
        raise ValueError(f"match must be 'id' or 'any', got {match!r}")
    c = torch.as_tensor(counts).detach().cpu()
    if c.dim() == 3:
        c = c.sum(0)
    if c.dim() != 2 or c.shape[1] != c.shape[0] + 1 or c.dtype.is_floating_point:
        raise ValueError(f"counts must be integers [B, K, K+1] or [K, K+1], got {c.dtype} {tuple(counts.shape)}")
    c = c.to(torch.int64)
    K = c.shape[0]
    T, P, I = c.sum(1), c[:, :K].sum(0), c.diagonal()
    U = T + P - I
    inter, union = I.double(), U.double()

    def mean_over(present):
        return float((inter[present] / union[present]).mean()) if present.any() else 0.0

    out = {"iou": torch.where(U > 0, inter / union.clamp(min=1), torch.full_like(inter, float("nan"))),
           "miou_gt_ids": mean_over(T > 0), "miou_all_ids": mean_over(U > 0),
           "pixel_acc": _ratio(int(I.sum()), int(T.sum()))}

    cn, Tn, Pn = c.numpy(), T.numpy(), P.numpy()
    stuff = {int(s) for s in stuff_ids}
    gt_ids = [g for g in range(K) if Tn[g] > 0]
    pred_ids = [p for p in range(K) if Pn[p] > 0]
    iou = np.zeros((K, K), dtype=np.float64)
    partner = np.full((K,), -1, dtype=np.int64)
    for g in gt_ids:
        for p in pred_ids:
            iou[g, p] = float(cn[g, p]) / float(Tn[g] + Pn[p] - cn[g, p])
            allowed = g == p or (match == "any" and g not in stuff and p not in stuff)
            if allowed and iou[g, p] > 0.5:
                partner[g] = p
    out.update(_panoptic(iou, partner, gt_ids, pred_ids))
    things = _panoptic(iou, partner, [g for g in gt_ids if g not in stuff], [p for p in pred_ids if p not in stuff])
    out.update({k + "_things": things[k] for k in ("pq", "sq", "rq")})
    out["matches"] = torch.from_numpy(partner)
    return out
