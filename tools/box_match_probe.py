"""The detector's target assignment on one MI355X: ``instance_nerf_amd.targets`` through the two fused launches
(csrc/assign.hip) against its composable path (the reference's chunked IoU matrix + Matcher in torch, ``fused=False``) on
the same GPU and inputs.

Shapes: the shipped anchor pyramid (40^3 / 20^3 / 10^3 / 5^3 cells of a 160 grid, 13 anchors per cell: A = 950 625)
against G = 8, 24 and 64 ground-truth boxes at the RPN's thresholds 0.35 / 0.2; two such scenes (G = 24) with padding
masks (a 128 x 160 x 112 scene inside the padded grid); and the RoI head's shape, A = 2 500 + G proposals with gt_labels
at 0.25 / 0.25 (``assign_targets_to_proposals``).

Device events around whole calls on the launch stream after warm-up, medians of ``--repeats``, the compared calls
alternating.  These are CALL times (ctypes, allocations of the outputs, the int32 -> float32 / int64 conversions of the
public interface included), not kernel times.  ``gb_per_s`` of a fused call: the bytes it must move - the boxes read twice
(2 x 24 B) plus the outputs written per box (matched 4, labels 4, matched boxes 24, targets 24 with ``encode``) - over
that call time.  ``peak_bytes``: device memory a call adds on top of its inputs.  The compiler's resource summary of the
two kernels is recorded when hipcc is at hand.

What the figures decide: ``targets.MATCH_FUSED_BY_DEFAULT`` (the fused form must not lose to the composable path on the
same inputs in any measured shape).
python tools/box_match_probe.py [--repeats 20] [--out profiles/box_match_probe.json]"""
import argparse
import itertools
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import _lib, build, targets                      # noqa: E402

DEV = torch.device("cuda", 0)
GRID = 160
RATIOS = ((1, 1, 1), (1, 1, 2), (1, 2, 2), (1, 1, 3), (1, 3, 3))


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


def shipped_anchors():
    """float32 [950 625, 6] on the device: levels in order, cells with z fastest, the 13 shapes innermost."""
    shapes = torch.tensor([p for r in RATIOS for p in sorted(set(itertools.permutations(r)))], dtype=torch.float64)
    out = []
    for size, cells in zip((8, 16, 32, 64), (40, 20, 10, 5)):
        half = torch.round(shapes * size / 2.0)
        base = torch.cat([-half, half], 1)
        s = torch.arange(cells, dtype=torch.float64) * (GRID // cells)
        shift = torch.stack(torch.meshgrid(s, s, s, indexing="ij"), -1).reshape(-1, 3)
        out.append((torch.cat([shift, shift], 1)[:, None, :] + base[None, :, :]).reshape(-1, 6))
    return torch.cat(out).to(torch.float32).to(DEV)


def gt_boxes(G, seed, extent=(GRID, GRID, GRID)):
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand((G, 6), generator=gen, dtype=torch.float64)
    side = 10.0 + u[:, 3:] * 50.0
    lo = u[:, :3] * (torch.tensor(extent, dtype=torch.float64) - side).clamp(min=0)
    return torch.cat([lo, lo + side], 1).to(torch.float32).to(DEV)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = int(torch.cuda.max_memory_allocated() - base)
    del out
    return peak


def resource_summary():
    """VGPRs, LDS and scratch of the two kernels from the compiler's remarks (the flags of build.py), or the reason why not.
    The GT rows are dynamic LDS (32 B per GT), which the remarks do not count."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return {"unavailable": "no hipcc"}
    cmd = [hipcc, "-x", "hip", "-c", os.path.join(build.CSRC, "assign.hip"), "-o", os.devnull, "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage"] + build.FLAGS
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = "k_box_match_gt_max" if "gt_max" in m.group(1) else "k_box_match_assign" if "assign" in m.group(1) else m.group(1)
            out[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out or {"unavailable": r.stderr[-300:]}


def same_results(a, b):
    """Lists of tensors per scene, every output: labels and matched boxes equal; of the targets the centre terms (the size
    terms are logs from two builds of the maths library and are compared in ulps by the tests)."""
    ok = True
    for kind, (x, y) in enumerate(zip(a, b)):               # labels, matched boxes, targets
        for p, q in zip(x, y):
            ok = ok and (torch.equal(p[:, :3], q[:, :3]) if kind == 2 else torch.equal(p, q))
    return bool(ok)


def anchors_config(anchors, gts, masks, repeats):
    A = anchors[0].shape[0]

    def call(fused, encode):
        return lambda: targets.assign_targets_to_anchors(anchors, gts, 0.35, 0.2, padding_masks=masks, encode=encode, fused=fused)
    fns = {"fused": call(True, False), "composable": call(False, False), "fused_encode": call(True, True),
           "composable_encode": call(False, True)}
    rec = alternating(fns, warmup=3, repeats=repeats)
    rec["outputs_equal"] = same_results(fns["fused_encode"](), fns["composable_encode"]())
    for k, out_bytes in (("fused", 32), ("fused_encode", 56)):
        rec[k]["gb_per_s"] = len(anchors) * A * (48 + out_bytes) / (rec[k]["median_ms"] * 1e-3) / 1e9
    rec["composable_over_fused"] = {"plain": rec["composable"]["median_ms"] / rec["fused"]["median_ms"],
                                    "encode": rec["composable_encode"]["median_ms"] / rec["fused_encode"]["median_ms"]}
    rec["peak_bytes"] = {k: peak_bytes(fn) for k, fn in fns.items()}
    labels = fns["fused"]()[0][0]
    rec["foreground_ignored_background"] = [int((labels == 1).sum()), int((labels == -1).sum()), int((labels == 0).sum())]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "box_match_probe.json"))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "source_sha": build.source_sha("assign"),
           "boxes_per_workgroup": _lib.BOX_MATCH_BOXES_PER_WG, "block": _lib.BOX_MATCH_BLOCK,
           "what": "targets.assign_targets_to_anchors / assign_targets_to_proposals call times in ms: the two fused launches "
                   "against the composable path (chunked IoU matrix + Matcher) on the same GPU tensors, alternating; "
                   "gb_per_s = bytes the fused call must move / call time; peak_bytes = device memory a call adds",
           "not_measured": "kernel times apart from the call's host work; other run lengths than 1024 boxes per workgroup "
                           "and other store patterns of the 24-byte rows; G above 64 at the full anchor count; "
                           "several scenes in one launch; other GPUs",
           "resources": resource_summary(), "configs": {}}
    anchors = shipped_anchors()
    assert anchors.shape == (950625, 6)
    for G in (8, 24, 64):
        rec = anchors_config([anchors], [gt_boxes(G, G)], None, args.repeats)
        out["configs"][f"anchors_G{G}"] = rec
        print("anchors", G, json.dumps(rec), flush=True)
    # two scenes of 128 x 160 x 112 inside the padded 160 grid: an anchor is real when its centre lies inside the scene
    ctr = (anchors[:, :3] + anchors[:, 3:]) * 0.5
    mask = ((ctr < torch.tensor([128.0, 160.0, 112.0], device=DEV)).all(1)).contiguous()
    rec = anchors_config([anchors, anchors.clone()], [gt_boxes(24, 1, (128, 160, 112)), gt_boxes(24, 2, (128, 160, 112))],
                         [mask, mask.clone()], args.repeats)
    rec["masked_fraction"] = float((~mask).float().mean())
    out["configs"]["two_scenes_masked_G24"] = rec
    print("two scenes", json.dumps(rec), flush=True)
    # the head: 2 500 proposals (jittered GT boxes and random boxes) plus the GT boxes themselves
    G = 24
    gt = gt_boxes(G, 7)
    gen = torch.Generator().manual_seed(8)
    near = gt.cpu()[torch.arange(1250) % G] + (torch.rand((1250, 6), generator=gen) - 0.5) * 8.0
    props = torch.cat([near.to(DEV), gt_boxes(1250, 9), gt])
    gl = (torch.arange(G, device=DEV) % 5 + 1)
    fns = {"fused": lambda: targets.assign_targets_to_proposals([props], [gt], [gl], 0.25, 0.25, fused=True),
           "composable": lambda: targets.assign_targets_to_proposals([props], [gt], [gl], 0.25, 0.25, fused=False)}
    rec = alternating(fns, warmup=3, repeats=args.repeats)
    a, b = fns["fused"](), fns["composable"]()
    rec["outputs_equal"] = bool(torch.equal(a[0][0], b[0][0]) and torch.equal(a[1][0], b[1][0]))
    rec["composable_over_fused"] = {"plain": rec["composable"]["median_ms"] / rec["fused"]["median_ms"]}
    rec["peak_bytes"] = {k: peak_bytes(fn) for k, fn in fns.items()}
    rec["proposals"] = int(props.shape[0])
    out["configs"]["head_G24"] = rec
    print("head", json.dumps(rec), flush=True)
    cfg = out["configs"]
    out["all_outputs_equal"] = bool(all(r["outputs_equal"] for r in cfg.values()))
    out["fused_never_loses"] = bool(all(v > 1.0 for r in cfg.values() for v in r["composable_over_fused"].values()))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": args.out, "fused_never_loses": out["fused_never_loses"], "all_outputs_equal": out["all_outputs_equal"]}))


if __name__ == "__main__":
    main()
