"""Times the multi-scale pooler at the detector's shapes: the fused pyramid call against the composable per-level loop
(the reference's structure around this repository's single-level kernels) on the same GPU and inputs.

Pyramid of a 160 grid: 40^3 / 20^3 / 10^3 / 5^3, C = 256, two images; 256 boxes -> 5^3 (box head) and 100 boxes -> 10^3
(mask head), box sides log-uniform from 12 to 220 grid units (the mapper's three reachable levels).  Device events
around the whole call, median of RUNS runs after warm-up, the two paths alternating.  Also: the kernels alone (events
around the launches, levels / order / gathered RoIs prepared beforehand) - the fused forward against the sum of the
per-level forwards, the fused backward (in place) against the per-level backwards in the form roi_align_3d picks
(workspace form allowed).

    python tools/pyramid_pool_probe.py        -> profiles/pyramid_pool_probe.json"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from instance_nerf_amd.roi_align import MultiScaleRoIAlign3D, poolers, pyramid_roi_align_3d      # noqa: E402
from instance_nerf_amd.roi_align.roi_align import roi_align_3d                                   # noqa: E402

RUNS = 20
GRID, C, IMAGES = 160, 256, 2
DIMS = [40, 20, 10, 5]


def median_ms(fns, runs=RUNS, warmup=3):
    """Median event time of each callable, the callables alternating inside every run."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [round(float(np.median(t)), 4) for t in times]


def make_boxes(n, rng):
    """n boxes per image, sides log-uniform in [12, 220], inside the grid where they fit.  Canonical scale 160 at level 4
    puts sides below 80 on the 40^3 level, [80, 160) on 20^3 and [160, 320) on 10^3; the 5^3 level would take boxes of
    twice the grid and stays empty, as it does for a detector's proposals (the fused call still carries its table entry,
    the loop skips it)."""
    out = []
    for _ in range(IMAGES):
        side = np.exp(rng.uniform(np.log(12.0), np.log(220.0), (n, 1))) * rng.uniform(0.8, 1.25, (n, 3))
        lo = rng.uniform(0, 1, (n, 3)) * np.maximum(GRID - side, 1.0)
        out.append(torch.from_numpy(np.concatenate([lo, lo + side], 1).astype(np.float32)).cuda())
    return out


def probe_head(name, n_boxes, bins, feats, rng):
    boxes = make_boxes(n_boxes // IMAGES, rng)
    shapes = [(GRID, GRID, GRID)] * IMAGES
    fused, loop = MultiScaleRoIAlign3D(bins, 2), MultiScaleRoIAlign3D(bins, 2)
    loop.fused = False
    leaves = [f.clone().requires_grad_(True) for f in feats]
    g = torch.randn(n_boxes, C, bins, bins, bins, device="cuda")

    def fwd_bwd(pool):
        def run():
            for x in leaves:
                x.grad = None
            torch.cat(pool(leaves, boxes, shapes)).backward(g)
        return run

    res = {"boxes": n_boxes, "bins": bins}
    res["fused_forward_ms"], res["loop_forward_ms"] = median_ms([lambda: fused(feats, boxes, shapes),
                                                                 lambda: loop(feats, boxes, shapes)])
    res["fused_forward_backward_ms"], res["loop_forward_backward_ms"] = median_ms([fwd_bwd(fused), fwd_bwd(loop)])
    diff = max((a - b).abs().max().item() for a, b in zip(fused(feats, boxes, shapes), loop(feats, boxes, shapes)))
    res["fused_vs_loop_max_abs_diff"] = diff

    # ---- the kernels alone: everything the launches need is prepared beforehand
    rois = torch.cat(boxes).contiguous()
    inds = torch.cat([torch.full((len(b),), i, dtype=torch.int32, device="cuda") for i, b in enumerate(boxes)])
    levels = fused.map_levels(boxes).to(torch.int32)
    order = poolers.level_order(levels)
    res["boxes_per_level"] = [int((levels == l).sum()) for l in range(len(feats))]
    per_level = [(l, rois[levels == l].contiguous(), inds[levels == l].contiguous()) for l in range(len(feats))
                 if int((levels == l).sum()) > 0]
    size, scales = (bins,) * 3, fused.scales

    def loop_kernels(xs):
        return [roi_align_3d(xs[l], r, i, *size, scales[l]) for l, r, i in per_level]

    res["fused_forward_kernel_ms"], res["fused_forward_kernel_unordered_ms"], res["per_level_forward_kernels_ms"] = median_ms([
        lambda: pyramid_roi_align_3d(feats, rois, inds, levels, size, scales, order=order),
        lambda: pyramid_roi_align_3d(feats, rois, inds, levels, size, scales, order=None),
        lambda: loop_kernels(feats)])
    out_f = pyramid_roi_align_3d(leaves, rois, inds, levels, size, scales, order=order)
    outs_l = loop_kernels(leaves)
    gs_l = [g[levels == l].contiguous() for l, _, _ in per_level]
    xs_l = [leaves[l] for l, _, _ in per_level]
    # (both include the zero fill of the gradients; the per-level form is the one roi_align_3d's cost model picks)
    res["fused_backward_ms"], res["per_level_backward_ms"] = median_ms([
        lambda: torch.autograd.grad([out_f], leaves, [g], retain_graph=True),
        lambda: torch.autograd.grad(outs_l, xs_l, gs_l, retain_graph=True)])
    print(name, json.dumps(res), flush=True)
    return res


def main():
    assert torch.cuda.is_available(), "the probe needs a GPU"
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    feats = [torch.randn(IMAGES, C, d, d, d, device="cuda", generator=gen) for d in DIMS]
    res = {"device": torch.cuda.get_device_name(0), "pyramid": DIMS, "channels": C, "images": IMAGES, "runs": RUNS,
           "timing": "device events around each call, median; the compared calls alternate within a run",
           "box_head": probe_head("box_head", 256, 5, feats, rng),
           "mask_head": probe_head("mask_head", 100, 10, feats, rng)}
    path = os.environ.get("INR_PROBE_OUT") or os.path.join(ROOT, "profiles", "pyramid_pool_probe.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
