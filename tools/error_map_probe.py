"""Error-map ray sampling (NeRFDataset(error_map=True), csrc/raymarch.hip) on one MI355X, the synthetic room:

1. the whole call of the weighted loader launch (``inr_sample_training_batch_weighted``) against the uniform one
   (``inr_sample_training_batch``): 4 096 rays of an 800x800 image, the map filled with values in (0.01, 1); and the
   whole call of the map's update (``inr_error_map_update``).  Device events on the launch stream after warm-up, medians
   of ``--repeats``, the compared calls alternating.  CALL times (allocations, ctypes, launch), not kernel times.
2. ``Trainer.train_one_epoch`` steps/s over the room on disk (24 views, 400x400, 4 096 rays) with the map on and off: a
   host clock around epochs that end in a device synchronise, after a warm-up epoch, the two trainers taking turns.
3. held-out PSNR (8 views from other cameras) of the two runs after the same number of steps.
None of these is asserted anywhere; the switch stays off by default whatever they show.
python tools/error_map_probe.py [--repeats 20] [--epochs 40] [--out profiles/error_map_probe.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import raymarching                               # noqa: E402
from instance_nerf_amd.nerf import NeRFNetwork                          # noqa: E402
from instance_nerf_amd.nerf.provider import NeRFDataset                 # noqa: E402
from instance_nerf_amd.nerf.utils import Trainer                        # noqa: E402
from instance_nerf_amd.scene import RoomScene                           # noqa: E402

DEV = torch.device("cuda", 0)


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


def psnr(net, test):
    net.eval()
    vals = []
    with torch.no_grad():
        for i in range(len(test)):
            b = test[i]
            out = net.render(b["rays_o"], b["rays_d"], bg_color=1)
            mse = float(((out["image"].reshape(-1, 3) - b["images"].reshape(-1, 3)) ** 2).mean())
            vals.append(-10.0 * np.log10(max(mse, 1e-12)))
    return float(np.mean(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--out", default=os.path.join("profiles", "error_map_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("error_map_probe needs a GPU: nothing is measured without one")
    room = RoomScene()
    rec = {"device": torch.cuda.get_device_name(0), "rays": 4096, "cells": 128}
    with tempfile.TemporaryDirectory() as tmp:
        # 1. the loader launch and the update launch, 800x800
        big = room.write_dataset(os.path.join(tmp, "big"), n_views=2, H=800, W=800)
        kw = dict(type="train", device=DEV, scale=1.0, num_rays=4096, seed=3)
        on, off = NeRFDataset(big["path"], error_map=True, **kw), NeRFDataset(big["path"], **kw)
        on.error_map.uniform_(0.01, 1.0)
        b = on[0]
        pred, gt = torch.rand(1, 4096, 3, device=DEV), torch.rand(1, 4096, 3, device=DEV)
        rec["loader_call_800x800"] = alternating({"weighted": lambda: on[0], "uniform": lambda: off[0]}, 5, args.repeats)
        rec["update_call"] = alternating(
            {"update": lambda: raymarching.error_map_update(pred, gt, b["inds_coarse"], on.error_map[0], 128)}, 5, args.repeats)
        del on, off
        # 2. + 3. the training loop with the map on and off, and what it learns
        train = room.write_dataset(os.path.join(tmp, "train"), n_views=24, H=400, W=400)
        held = room.write_dataset(os.path.join(tmp, "held"), n_views=8, H=400, W=400, seed=77)
        test = NeRFDataset(held["path"], type="train", device=DEV, scale=1.0)
        test.training, test.num_rays = False, -1                        # whole images, row-major
        runs = {}
        for name, flag in (("error_map_on", True), ("error_map_off", False)):
            torch.manual_seed(0)
            net = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05, density_thresh=10)
            ds = NeRFDataset(train["path"], type="train", device=DEV, scale=1.0, num_rays=4096, seed=5, error_map=flag)
            tr = Trainer(name, None, net, device=DEV, workspace=None, mute=True, lr=1e-2, iters=24 * (args.epochs + 1))
            tr.train(ds.dataloader(), max_epochs=1)                     # warm-up epoch (and adopts the map)
            runs[name] = (tr, ds.dataloader(), [])
        torch.cuda.synchronize()
        for _ in range(args.epochs):
            for name, (tr, loader, secs) in runs.items():
                t0 = time.perf_counter()
                tr.epoch += 1
                tr.train_one_epoch(loader)
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
        rec["train_one_epoch"] = {}
        for name, (tr, loader, secs) in runs.items():
            rec["train_one_epoch"][name] = {"steps": 24 * (args.epochs + 1), "median_steps_per_s": float(24 / np.median(secs)),
                                            "min_steps_per_s": float(24 / np.max(secs)), "max_steps_per_s": float(24 / np.min(secs)),
                                            "final_loss": tr.stats["loss"][-1], "held_out_psnr_db": psnr(tr.model, test)}
        m = runs["error_map_on"][0].error_map
        rec["final_map"] = {"min": float(m.min()), "median": float(m.median()), "max": float(m.max()),
                            "cells_visited": float((m != 1).float().mean())}
    t = rec["loader_call_800x800"]
    rec["summary"] = {
        "weighted_over_uniform_call": t["weighted"]["median_ms"] / t["uniform"]["median_ms"],
        "weighted_call_ms": t["weighted"]["median_ms"], "uniform_call_ms": t["uniform"]["median_ms"],
        "update_call_ms": rec["update_call"]["update"]["median_ms"],
        "steps_per_s_on_over_off": rec["train_one_epoch"]["error_map_on"]["median_steps_per_s"]
        / rec["train_one_epoch"]["error_map_off"]["median_steps_per_s"],
        "psnr_on_minus_off_db": rec["train_one_epoch"]["error_map_on"]["held_out_psnr_db"]
        - rec["train_one_epoch"]["error_map_off"]["held_out_psnr_db"],
    }
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec["summary"]))


if __name__ == "__main__":
    main()
