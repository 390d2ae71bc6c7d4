"""Image quality of rendered views: SSIM, MSE and PSNR from one fused launch (csrc/ssim.hip, include/inr.h "Image quality
of rendered views"), and the composable torch path with the same window and formula - the CPU path and the on-GPU baseline.

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
