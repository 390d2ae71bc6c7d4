"""The FCOS head's targets and losses on one MI355X: ``instance_nerf_amd.fcos`` through the fused launches (csrc/fcos.hip)
against its composable path (the reference's tensor program in torch, ``fused=False``) on the same GPU and inputs.

Shape: the shipped pyramid (40^3 / 20^3 / 10^3 / 5^3 locations of a 160 grid, strides 4 / 8 / 16 / 32: 73 125 locations
per scene), B = 1 and 4 scenes, G = 8, 24 and 64 ground-truth boxes per scene, padding masks of a 128 x 160 x 112 scene,
the ``giou`` loss the reference's scripts train with.

Timed per configuration, fused against composable, the compared calls alternating: ``prepare_targets``; ``fcos_loss``
forward; forward plus ``backward()``.  Device events around whole calls on the launch stream after warm-up, medians of
``--repeats``.  These are CALL times (ctypes, the allocation of every output, the upload of the box offsets, autograd's
bookkeeping included), not kernel times.  ``peak_bytes``: device memory a call adds on top of its inputs.  Outputs are
compared: targets bit for bit except ``matched`` where two boxes tie (torch.min on a GPU may pick another index; the
labels and distances are then still equal when the tied boxes are equal), losses and gradients by their largest relative
difference.  The compiler's resource summary of the four kernels is recorded when hipcc is at hand; the staged boxes of
k_fcos_targets are dynamic LDS (52 B per box), which the remarks do not count.

What the figures decide: ``fcos.TARGETS_FUSED_BY_DEFAULT`` and ``fcos.LOSS_FUSED_BY_DEFAULT`` (a fused form must not lose to
the composable path on the same inputs in any measured shape).
python tools/fcos_probe.py [--repeats 20] [--out profiles/fcos_probe.json]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import _lib, build, fcos                      # noqa: E402

DEV = torch.device("cuda", 0)
SHAPES, STRIDES, GRID = [(40, 40, 40), (20, 20, 20), (10, 10, 10), (5, 5, 5)], [4, 8, 16, 32], 160
ORI = (128, 160, 112)
KERNELS = ("k_fcos_targets", "k_fcos_loss_forward", "k_fcos_loss_finish", "k_fcos_loss_backward")


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


def gt_boxes(G, seed):
    """Sides log-uniform 6 .. 120 inside the unpadded scene: every level of the pyramid gets positives."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand((G, 6), generator=gen, dtype=torch.float64)
    ext = torch.tensor(ORI, dtype=torch.float64)
    side = torch.minimum(torch.exp(np.log(6.0) + u[:, 3:] * np.log(20.0)), ext)
    lo = u[:, :3] * (ext - side)
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
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return {"unavailable": "no hipcc"}
    cmd = [hipcc, "-x", "hip", "-c", os.path.join(build.CSRC, "fcos.hip"), "-o", os.devnull, "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage"] + build.FLAGS
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = next((k for k in KERNELS if k in m.group(1)), m.group(1))
            out[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out or {"unavailable": r.stderr[-300:]}


def rel_diff(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-30))


def predictions(B, seed):
    gen = torch.Generator().manual_seed(seed)
    cls = [(2 * torch.randn((B, 1) + s, generator=gen)).to(DEV) for s in SHAPES]
    reg = [(2 * torch.exp(torch.randn((B, 6) + s, generator=gen))).to(DEV) for s in SHAPES]
    ctr = [torch.randn((B, 1) + s, generator=gen).to(DEV) for s in SHAPES]
    return cls, reg, ctr


def config(B, G, repeats):
    gts = [gt_boxes(G, 100 * b + G) for b in range(B)]
    ori = [ORI] * B

    def targets_call(fused):
        return lambda: fcos.prepare_targets(SHAPES, STRIDES, gts, ori_sizes=ori, fused=fused)
    tf, tc = targets_call(True)(), targets_call(False)()
    preds = predictions(B, G)
    leaves = [[p.clone().requires_grad_(True) for p in group] for group in preds]

    def loss_call(fused, t, backward):
        def run():
            out = fcos.fcos_loss(*(leaves if backward else preds), t, "giou", fused=fused)
            if backward:
                for group in leaves:
                    for p in group:
                        p.grad = None
                (out[0] + out[1] + out[2]).backward()
            return out
        return run
    fns = {"targets_fused": targets_call(True), "targets_composable": targets_call(False),
           "loss_fused": loss_call(True, tf, False), "loss_composable": loss_call(False, tf, False),
           "loss_backward_fused": loss_call(True, tf, True), "loss_backward_composable": loss_call(False, tf, True)}
    rec = alternating(fns, warmup=3, repeats=repeats)
    rec["composable_over_fused"] = {k: rec[f"{k}_composable"]["median_ms"] / rec[f"{k}_fused"]["median_ms"]
                                    for k in ("targets", "loss", "loss_backward")}
    differs = tf.matched_flat != tc.matched_flat
    rec["targets_equal"] = {"labels": bool(torch.equal(tf.labels_flat, tc.labels_flat)),
                            "reg_targets": bool(torch.equal(tf.reg_targets_flat, tc.reg_targets_flat)),
                            "centerness": bool(torch.equal(tf.centerness_flat, tc.centerness_flat)),
                            "valid": bool(torch.equal(tf.valid_flat, tc.valid_flat)),
                            "matched_differs_at": int(differs.sum())}
    rec["positives"] = int((tf.labels_flat > 0).sum())
    fns["loss_backward_fused"]()
    g_f = [p.grad.clone() for group in leaves for p in group]
    l_f = [float(v) for v in fns["loss_fused"]()]
    fns["loss_backward_composable"]()
    g_c = [p.grad.clone() for group in leaves for p in group]
    l_c = [float(v) for v in fns["loss_composable"]()]
    rec["losses"] = {"fused": l_f, "composable": l_c}
    rec["largest_relative_gradient_difference"] = max(rel_diff(a, b) for a, b in zip(g_f, g_c))
    rec["outputs_equal"] = bool(all(v for k, v in rec["targets_equal"].items() if k != "matched_differs_at")
                                and all(abs(a - b) <= 1e-4 * abs(b) for a, b in zip(l_f, l_c))
                                and rec["largest_relative_gradient_difference"] < 1e-3)
    rec["peak_bytes"] = {k: peak_bytes(fn) for k, fn in fns.items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "fcos_probe.json"))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "source_sha": build.source_sha("fcos"),
           "locations_per_workgroup": {"targets": _lib.FCOS_LOCATIONS_PER_WG, "loss": _lib.FCOS_LOSS_LOCATIONS_PER_WG},
           "block": _lib.FCOS_BLOCK, "locations_per_scene": sum(w * l * h for w, l, h in SHAPES),
           "what": "fcos.prepare_targets / fcos_loss (giou) call times in ms: the fused launches against the composable path "
                   "on the same GPU tensors, alternating; peak_bytes = device memory a call adds",
           "not_measured": "kernel times apart from the call's host work; other run lengths than 256 / 1024 locations per "
                           "workgroup; wider stores of the 24-byte target rows; G above 64; world_size > 1; other GPUs",
           "resources": resource_summary(), "configs": {}}
    for B in (1, 4):
        for G in (8, 24, 64):
            rec = config(B, G, args.repeats)
            out["configs"][f"B{B}_G{G}"] = rec
            print(f"B{B} G{G}", json.dumps(rec), flush=True)
    cfg = out["configs"]
    out["all_outputs_equal"] = bool(all(r["outputs_equal"] for r in cfg.values()))
    out["fused_never_loses"] = {k: bool(all(r["composable_over_fused"][k] > 1.0 for r in cfg.values()))
                                for k in ("targets", "loss", "loss_backward")}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": args.out, "fused_never_loses": out["fused_never_loses"], "all_outputs_equal": out["all_outputs_equal"]}))


if __name__ == "__main__":
    main()
