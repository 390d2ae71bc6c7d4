"""The confusion matrix of rendered instance maps on one MI355X: ``instance_nerf_amd.metrics.segmentation_confusion``
through the two fused entries (csrc/confusion.hip: ids, logits) against its composable path on the same GPU and inputs
(``torch.argmax`` + one ``torch.bincount``, ``fused=False``), and ``nerf.utils.MIoUMeter.update`` as it stands, read-back
included.  800x800 views, K = 16 and 64, B = 1 and 8; truth and prediction in three shapes: one (t, p) pair everywhere (a
view of a wall: every lane of a wave on one LDS counter), a room-like map of twelve large regions with the prediction's
borders a few pixels off, and uniformly random ids (every pixel of a workgroup on another counter: the costliest flush).

Device events around whole calls on the launch stream after warm-up, medians of ``--repeats``, the four compared calls
alternating.  These are CALL times (tensor reshapes, ctypes, launches), not kernel times; ``tb_per_s`` is the bytes a
launch has to read (8 B per pixel for ids, 4 ld + 4 for logits) over that call time.  ``peak_bytes``: device memory a
call adds on top of its inputs and its (pre-allocated) outputs.  MIoUMeter.update runs on the host: wall clock, median of
3, on the room-like map only (its time does not depend on the values).  The compiler's resource summary of the two
kernels is recorded when hipcc is at hand.

What the figures decide: ``metrics.CONFUSION_FUSED_BY_DEFAULT`` (each fused form must not lose to the composable path on
the same inputs) and whether the kernels need the ballot aggregation of csrc/match.hip (only if the one-pair image is
slower than the random one).
python tools/segmentation_probe.py [--repeats 20] [--out profiles/segmentation_probe.json]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import _lib, build, metrics                      # noqa: E402
from instance_nerf_amd.nerf.utils import MIoUMeter                      # noqa: E402

DEV = torch.device("cuda", 0)
H = W = 800
PATTERNS = ("one_pair", "room", "random")


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


def id_maps(pattern, B, K):
    """(pred, truth) int32 [B, H, W] on the device."""
    gen = torch.Generator(device=DEV).manual_seed(B * 100 + K)
    if pattern == "one_pair":
        return (torch.full((B, H, W), K // 2, dtype=torch.int32, device=DEV),
                torch.full((B, H, W), K - 1, dtype=torch.int32, device=DEV))
    if pattern == "random":
        return (torch.randint(0, K, (B, H, W), device=DEV, generator=gen, dtype=torch.int32),
                torch.randint(-1, K, (B, H, W), device=DEV, generator=gen, dtype=torch.int32))
    ii = torch.arange(H, device=DEV).view(1, H, 1)
    jj = torch.arange(W, device=DEV).view(1, 1, W)
    shift = torch.arange(B, device=DEV).view(B, 1, 1) * 7

    def regions(di, dj):                                  # 4 x 3 rectangles, ids 0..11 (mod K)
        return ((((ii + shift + di) % H) * 4 // H) * 3 + ((jj + dj) % W) * 3 // W) % K

    return regions(5, -4).to(torch.int32).contiguous(), regions(0, 0).to(torch.int32).contiguous()


def logits_of(pred, K):
    """float32 [B, H, W, K] whose arg-max is ``pred``, without ties."""
    gen = torch.Generator(device=DEV).manual_seed(K)
    x = torch.rand((*pred.shape, K), device=DEV, generator=gen)
    x.scatter_(-1, pred.long().unsqueeze(-1), 2.0)
    return x


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def resource_summary():
    """VGPRs, LDS and scratch of the two kernels from the compiler's remarks (the flags of build.py), or the reason why not."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return {"unavailable": "no hipcc"}
    cmd = [hipcc, "-x", "hip", "-c", os.path.join(build.CSRC, "confusion.hip"), "-o", os.devnull, "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage"] + build.FLAGS
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = "k_confusion_logits" if "logits" in m.group(1) else "k_confusion_ids" if "ids" in m.group(1) else m.group(1)
            out[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out or {"unavailable": r.stderr[-300:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "segmentation_probe.json"))
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "source_sha": build.source_sha("confusion"),
           "pixels_per_workgroup": _lib.CONFUSION_PIXELS_PER_WG, "block": _lib.CONFUSION_BLOCK,
           "what": "segmentation_confusion(pred, truth, K, out=...) call times in ms at 800x800: fused ids / logits entries "
                   "against the composable path (argmax + bincount) on the same GPU tensors, alternating; tb_per_s = bytes "
                   "the launch must read / call time; peak_bytes = device memory a call adds; miou_meter_update = "
                   "MIoUMeter.update on the same ids, host wall clock, read-back included",
           "resources": resource_summary(), "configs": {}}
    for K in (16, 64):
        for B in (1, 8):
            for pattern in PATTERNS:
                pred, truth = id_maps(pattern, B, K)
                logits = logits_of(pred, K)
                outs = {k: (torch.zeros((B, K, K + 1), dtype=torch.int64, device=DEV), torch.zeros((B,), dtype=torch.int64, device=DEV))
                        for k in ("ids_fused", "ids_composable", "logits_fused", "logits_composable")}
                fns = {"ids_fused": lambda: metrics.segmentation_confusion(pred, truth, K, out=outs["ids_fused"], fused=True),
                       "ids_composable": lambda: metrics.segmentation_confusion(pred, truth, K, out=outs["ids_composable"], fused=False),
                       "logits_fused": lambda: metrics.segmentation_confusion(logits, truth, K, out=outs["logits_fused"], fused=True),
                       "logits_composable": lambda: metrics.segmentation_confusion(logits, truth, K, out=outs["logits_composable"], fused=False)}
                rec = alternating(fns, warmup=3, repeats=args.repeats)
                same = all(torch.equal(outs["ids_fused"][i], outs[k][i]) for k in outs for i in (0, 1))
                rec["all_four_matrices_equal"] = bool(same)
                n = B * H * W
                for k, per_pixel in (("ids_fused", 8), ("logits_fused", 4 * K + 4)):
                    rec[k]["tb_per_s"] = n * per_pixel / (rec[k]["median_ms"] * 1e-3) / 1e12
                rec["composable_over_fused"] = {e: rec[e + "_composable"]["median_ms"] / rec[e + "_fused"]["median_ms"]
                                                for e in ("ids", "logits")}
                rec["peak_bytes"] = {k: peak_bytes(fn) for k, fn in fns.items()}
                if pattern == "room":
                    meter, ts = MIoUMeter(K), []
                    for _ in range(3):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        meter.update(pred, truth)
                        ts.append((time.perf_counter() - t0) * 1e3)
                    rec["miou_meter_update"] = {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "repeats": 3}
                out["configs"][f"K{K}_B{B}_{pattern}"] = rec
                print(K, B, pattern, json.dumps(rec), flush=True)
                del logits, pred, truth, outs, fns
    cfg = out["configs"]
    out["fused_never_loses"] = bool(all(v > 1.0 for r in cfg.values() for v in r["composable_over_fused"].values()))
    out["one_pair_slower_than_random"] = {
        e: bool(any(cfg[f"K{K}_B{B}_one_pair"][e]["median_ms"] > cfg[f"K{K}_B{B}_random"][e]["median_ms"]
                    for K in (16, 64) for B in (1, 8))) for e in ("ids_fused", "logits_fused")}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "fused_never_loses": out["fused_never_loses"],
                      "one_pair_slower_than_random": out["one_pair_slower_than_random"]}))


if __name__ == "__main__":
    main()
