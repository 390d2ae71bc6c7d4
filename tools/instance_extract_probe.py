"""3-D instance-mask extraction (extract.extract_instances) on a trained room at 160^3, K = 16 / 31 / 64: the fused path
(inr_instance_lattice + inr_instance_volume_stats) against the composable one (density() + instance() over chunks).

The room is written to disk and its NeRF trained by the product's Trainer (`--steps`); the K = 16 instance field is
then trained on the matched masks (`--inst-steps`).  K = 31 / 64 reuse the trained NeRF with an untrained instance head:
the work of either path does not depend on the instance weights' values, only on which tiles are occupied, and that is
the NeRF's.  Per K: device-event time per extraction after warm-up (median / min / max over repeats), voxels/s, the
fraction of 16-voxel runs that run the instance field, algorithmic bytes (1024 B of NeRF table per voxel + 1024 B of
instance table per voxel of a non-skipped run) and their share of the 8 TB/s roofline.  Kernel times: run it once more
under `rocprofv3 --kernel-trace --stats`.
python tools/instance_extract_probe.py [--steps 2000] [--inst-steps 1500] [--repeats 10] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import extract                              # noqa: E402
from instance_nerf_amd.nerf import NeRFNetwork                      # noqa: E402
from instance_nerf_amd.nerf.provider import NeRFDataset             # noqa: E402
from instance_nerf_amd.nerf.utils import Trainer                    # noqa: E402
from instance_nerf_amd.scene import RoomScene                       # noqa: E402

DEV = torch.device("cuda", 0)


def run(tr, ds, steps):
    it = iter(())
    for _ in range(steps):
        try:
            batch = next(it)
        except StopIteration:
            it = iter(ds)
            batch = next(it)
        tr.train_one_step(batch)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--inst-steps", type=int, default=1500)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--max-side", type=int, default=160)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    room = RoomScene()
    scene = room.write_dataset(tempfile.mkdtemp(prefix="inr_inst_probe_"), n_views=24, H=200, W=200, num_instances=16)
    net = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05, density_thresh=10, num_instances=16).to(DEV)
    ds = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096)
    run(Trainer("p_nerf", None, net, stage="nerf", device=DEV, lr=1e-2, iters=1500, workspace=None, mute=True), ds, a.steps)
    ds2 = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096, mask_dir=scene["mask_dir"],
                      num_instances=16)
    net.mean_density = net.mean_density
    ti = Trainer("p_inst", None, net, stage="instance", device=DEV, lr=1e-2, iters=1500, update_extra_interval=10 ** 9,
                 workspace=None, mute=True)
    ti.global_step = 1
    run(ti, ds2, a.inst_steps)
    nerf_sd = {k: v for k, v in net.state_dict().items() if not k.startswith("instance_")}
    out = {"workload": f"synthetic room, NeRF trained {a.steps} steps, K=16 instance field {a.inst_steps} steps; "
                       f"lattice {a.max_side} on the longest side over [-1, 1]^3, sigma_thresh = density_thresh = 10",
           "per_K": {}}
    for K in (16, 31, 64):
        if K == 16:
            m = net
        else:
            m = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05, density_thresh=10, num_instances=K).to(DEV)
            m.load_state_dict(nerf_sd, strict=False)
        m.eval()
        res = extract.grid_resolution([-1, -1, -1], [1, 1, 1], a.max_side)
        n = int(np.prod(res))
        r = extract.extract_instances(m, max_side=a.max_side)
        lab = r["labels"]
        W, L, H = (int(v) for v in res)
        Wp = (W + 15) // 16 * 16
        padded = torch.full((Wp, L, H), 255, dtype=torch.uint8, device=DEV)
        padded[:W] = lab
        live = (padded != 255).view(Wp // 16, 16, L, H)
        run_live = live.any(1)                                           # [Wp/16, L, H]: the runs that ran the instance field
        n_runs = int(run_live.numel())
        n_live = int(run_live.sum())
        vox_live = int((run_live.unsqueeze(1).expand(-1, 16, -1, -1).reshape(Wp, L, H)[:W]).sum())
        axes = extract.cached_axes(np.float32([-1, -1, -1]), np.float32([1, 1, 1]), res, DEV)
        fused = timed(lambda: extract.extract_instances(m, max_side=a.max_side), 2, a.repeats)
        lattice_only = timed(lambda: m.instance_lattice(axes, 10.0), 2, a.repeats)
        comp = timed(lambda: extract.extract_instances(m, max_side=a.max_side, fused=False), 1, max(3, a.repeats // 3))
        nbytes = 1024 * n + 1024 * vox_live
        c = extract.extract_instances(m, max_side=a.max_side, fused=False)
        agree = float((c["labels"] == lab).float().mean())
        row = {"res": [W, L, H], "voxels": n, "occupied_voxels": int((lab != 255).sum()),
               "occupied_run_fraction": n_live / n_runs, "voxels_in_live_runs": vox_live,
               "fused_extract": fused, "fused_lattice_launch_only": lattice_only, "composable_extract": comp,
               "speedup_median": comp["median_ms"] / fused["median_ms"],
               "fused_voxels_per_s": n / (fused["median_ms"] * 1e-3),
               "algorithmic_bytes": nbytes,
               "lattice_roofline_share": nbytes / (lattice_only["median_ms"] * 1e-3) / 8e12,
               "labels_equal_to_composable": agree}
        out["per_K"][K] = row
        print(f"K={K}: fused {fused['median_ms']:.3f} ms [{fused['min_ms']:.3f}, {fused['max_ms']:.3f}] "
              f"(lattice launch {lattice_only['median_ms']:.3f}), composable {comp['median_ms']:.2f} ms, "
              f"x{row['speedup_median']:.1f}; {row['fused_voxels_per_s'] / 1e9:.2f} Gvoxels/s; live runs "
              f"{row['occupied_run_fraction']:.3f}; {nbytes / 1e9:.2f} GB algorithmic, "
              f"{row['lattice_roofline_share']:.2f} of 8 TB/s; labels equal to composable {agree:.5f}", flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
