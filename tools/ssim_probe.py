"""SSIM on one MI355X: ``instance_nerf_amd.metrics.image_quality`` through the fused kernel (csrc/ssim.hip) against its
composable path (grouped F.conv2d, ``fused=False``) on the same GPU and inputs - 800x800x3 for B = 1 and B = 8, 400x400x3.

Device events around whole calls on the launch stream after warm-up, medians of ``--repeats``, the two compared calls
alternating.  These are CALL times (allocations, ctypes, launches), not kernel times.  Beside them: the peak device
memory each path adds on top of its inputs, and the largest difference between the two paths' per-image SSIM.  The
images are a smooth pattern against a noisy copy of it (the kernels' time does not depend on the values).

The SSIM of the bench scene's trained held-out view is NOT recorded: the trained-scene helper of tools/bench_secondary.py
(``trained_scene_probe``) trains, times and scores inside one function and hands out neither the network nor the view.
python tools/ssim_probe.py [--repeats 20] [--out profiles/ssim_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import build, metrics                            # noqa: E402

DEV = torch.device("cuda", 0)
SHAPES = [(1, 800, 800, 3), (8, 800, 800, 3), (1, 400, 400, 3)]


def alternating(fns, warmup, repeats):
    """Median / min / max ms of each callable, the callables taking turns."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "repeats": repeats}
            for k, v in ms.items()}


def images(B, H, W, C):
    gen = torch.Generator(device=DEV).manual_seed(B * 1000 + H)
    ii = torch.arange(H, device=DEV).view(1, H, 1, 1) / H
    jj = torch.arange(W, device=DEV).view(1, 1, W, 1) / W
    phase = torch.rand((B, 1, 1, C), device=DEV, generator=gen) * 6.0
    truth = 0.5 + 0.4 * torch.sin(5.0 * ii + 3.0 * jj + phase)
    pred = (truth + 0.05 * torch.randn((B, H, W, C), device=DEV, generator=gen)).clamp(0.0, 1.0)
    return pred.contiguous(), truth.contiguous()


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "ssim_probe.json"))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "source_sha": build.source_sha("ssim"), "tile": list(metrics.TILE),
           "what": "image_quality(pred, truth) call times in ms, fused kernel against the composable F.conv2d path, alternating; "
                   "peak_bytes = device memory a call adds on top of its inputs", "shapes": {}}
    for B, H, W, C in SHAPES:
        pred, truth = images(B, H, W, C)
        fns = {"fused": lambda: metrics.image_quality(pred, truth, fused=True),
               "composable": lambda: metrics.image_quality(pred, truth, fused=False)}
        rec = alternating(fns, warmup=5, repeats=args.repeats)
        a, b = fns["fused"](), fns["composable"]()
        rec["composable_over_fused"] = rec["composable"]["median_ms"] / rec["fused"]["median_ms"]
        rec["peak_bytes"] = {k: peak_bytes(fn) for k, fn in fns.items()}
        rec["input_bytes"] = 2 * pred.numel() * 4
        rec["max_abs_ssim_difference"] = float((a["ssim"].double() - b["ssim"].double()).abs().max())
        rec["ssim"] = [round(float(v), 6) for v in a["ssim"][:2]]
        rec["psnr_db"] = [round(float(v), 3) for v in a["psnr"][:2]]
        out["shapes"]["x".join(map(str, (B, H, W, C)))] = rec
        print(B, H, W, C, json.dumps(rec), flush=True)
    out["fused_is_faster_at_800"] = bool(all(out["shapes"][k]["composable_over_fused"] > 1.0 for k in ("1x800x800x3", "8x800x800x3")))
    out["trained_held_out_view"] = ("not recorded: tools/bench_secondary.py::trained_scene_probe hands out neither the trained "
                                    "network nor the held-out view")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "fused_is_faster_at_800": out["fused_is_faster_at_800"]}))


if __name__ == "__main__":
    main()
