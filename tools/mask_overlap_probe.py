"""3-D mask overlap and the reference's mask metric on the GPU (instance_nerf_amd/evaluate.py, csrc/overlap.hip).
(tools/overlap_probe.py is the older two-stream probe; this one writes profiles/overlap_probe.json.)

1. Timing on the analytic room's lattice at 160^3 and 256^3: k x k masks, k = 30 and 64 - side A detector-style box
   masks (boxes cut to the occupied voxels, as tools/match_probe.py builds them), side B the room's 12 analytic instance
   masks followed by k - 12 more boxes - and a label-volume prediction with K = 16 and 64 channels against side B.
   Each export on its own (pack from masks, pack from labels, pair count: one fill + one launch each, bracketed by
   device events on the launch stream, allocations of the outputs included), the whole fused call, and the composable
   torch path (chunked fp32 matmuls of the flattened masks) on the same GPU and inputs, outputs compared for equality.
   The pair count is also timed over a sweep of words per workgroup.  Achieved TB/s are each launch's OWN bytes: k * V
   read by the mask pack, V by the label pack, (kA * ceil(kB / 8) + kB * ceil(kA / 8)) * V / 8 by the pair count (every
   plane is re-read once per tile of the other side).  Peak memory: torch's allocator high-water mark over one call.
2. With --train: the reference's metric for the trained room's extracted masks (lattice 160, sigma >= 1), raw and with
   components="largest", against the analytic boxes' voxels.
Warm-up, then medians with min / max.  Numbers are written down as measured.
python tools/mask_overlap_probe.py [--repeats 20] [--train] [--steps 2000] [--inst-steps 1500] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import evaluate as ev                        # noqa: E402
from instance_nerf_amd.scene import RoomScene                       # noqa: E402

DEV = torch.device("cuda", 0)
RUNS = (256, 512, 1024, 2048, 4096, 8192, 16384)


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - base)


def room_ids(room, res):
    """Instance id (0 = none) of every voxel centre of the res^3 lattice over [-1, 1]^3, on the device, slab by slab."""
    ax = (np.arange(res, dtype=np.float64) + 0.5) / res * 2.0 - 1.0
    out = np.zeros((res, res, res), np.uint8)
    for i in range(res):
        pts = np.stack(np.meshgrid(ax[i:i + 1], ax, ax, indexing="ij"), -1).reshape(-1, 3)
        out[i] = room.instance_of_points(pts).reshape(res, res)
    return torch.from_numpy(out).to(DEV)


def box_masks(k, res, occ, rng):
    out = torch.zeros(k, res, res, res, dtype=torch.bool, device=DEV)
    for i in range(k):
        lo = rng.integers(0, res - res // 4, size=3)
        hi = lo + rng.integers(res // 7, res // 4, size=3)
        out[i, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        if rng.random(3).sum() <= 1.5:                     # some masks keep their whole box, most only its occupied part
            out[i] &= occ
    return out


def tb_per_s(nbytes, t):
    return nbytes / (t["median_ms"] * 1e-3) / 1e12


def timing(room, res, repeats):
    rng = np.random.default_rng(res)
    ids = room_ids(room, res)
    occ = ids > 0
    V = res ** 3
    n_inst = len(room.lo)
    out = {}
    for k in (30, 64):
        a = box_masks(k, res, occ, rng)
        b = torch.cat([torch.stack([ids == c for c in range(1, n_inst + 1)]), box_masks(k - n_inst, res, occ, rng)])
        pa, pb = ev.pack_mask_planes(a), ev.pack_mask_planes(b)
        fused = ev.mask_overlap(a, b)
        twin = ev.mask_overlap(a, b, fused=False)
        equal = all(bool(torch.equal(x, y)) for x, y in zip(fused, twin))
        tiles = -(-k // 8)
        pair_bytes = 2 * k * tiles * V // 8
        row = {"equal": equal, "mask_bytes_per_side": k * V, "plane_bytes_per_side": k * ((V + 63) // 64) * 8,
               "pair_count_bytes_read": pair_bytes, "planes_reread_factor": tiles}
        row["pack_masks"] = timed(lambda: ev.pack_mask_planes(a), 3, repeats)
        row["pack_masks"]["TB_per_s_of_k_V_bytes"] = tb_per_s(k * V, row["pack_masks"])
        row["pair_count_default_run"] = timed(lambda: ev.overlap_planes(pa, pb), 3, repeats)
        row["pair_count_default_run"]["TB_per_s_of_reread_plane_bytes"] = tb_per_s(pair_bytes, row["pair_count_default_run"])
        row["pair_count_by_run_words"] = {}
        for run in RUNS:
            t = timed(lambda: ev.overlap_planes(pa, pb, run_words=run), 2, repeats)
            t["TB_per_s_of_reread_plane_bytes"] = tb_per_s(pair_bytes, t)
            row["pair_count_by_run_words"][str(run)] = t
        row["fused_call_pack_pack_count"] = timed(lambda: ev.mask_overlap(a, b), 3, repeats)
        row["fused_call_packed_once"] = timed(lambda: ev.mask_overlap(pa, pb), 3, repeats)
        row["composable_torch_same_gpu"] = timed(lambda: ev.mask_overlap(a, b, fused=False), 1, max(3, repeats // 4))
        row["ratio_median"] = row["composable_torch_same_gpu"]["median_ms"] / row["fused_call_pack_pack_count"]["median_ms"]
        row["peak_bytes_fused"] = peak_bytes(lambda: ev.mask_overlap(a, b))
        row["peak_bytes_composable"] = peak_bytes(lambda: ev.mask_overlap(a, b, fused=False))
        out[f"masks_{k}x{k}"] = row
        print(f"{res}^3 {k}x{k}: pack {row['pack_masks']['median_ms']:.3f} ms ({row['pack_masks']['TB_per_s_of_k_V_bytes']:.2f} TB/s), "
              f"count {row['pair_count_default_run']['median_ms']:.3f} ms, fused {row['fused_call_pack_pack_count']['median_ms']:.3f} ms, "
              f"composable {row['composable_torch_same_gpu']['median_ms']:.2f} ms (x{row['ratio_median']:.1f}), equal {equal}", flush=True)
        if k == 64:
            for K in (16, 64):
                lab = torch.where(occ, (ids.long() * 5 + 1) % K, torch.full_like(ids, 255, dtype=torch.int64)).to(torch.uint8)
                f = ev.label_mask_overlap(lab, K, pb)
                t = ev.label_mask_overlap(lab, K, pb, fused=False)
                lrow = {"equal": all(bool(torch.equal(x, y)) for x, y in zip(f, t)), "label_bytes": V,
                        "plane_bytes_written": (K - 1) * ((V + 63) // 64) * 8}
                lrow["pack_labels"] = timed(lambda: ev.pack_label_planes(lab, K, 1), 3, repeats)
                lrow["pack_labels"]["TB_per_s_of_V_bytes"] = tb_per_s(V, lrow["pack_labels"])
                lrow["pack_labels"]["TB_per_s_of_V_plus_planes_written"] = tb_per_s(V + lrow["plane_bytes_written"], lrow["pack_labels"])
                lrow["fused_call_labels_vs_packed"] = timed(lambda: ev.label_mask_overlap(lab, K, pb), 3, repeats)
                lrow["composable_torch_same_gpu"] = timed(lambda: ev.label_mask_overlap(lab, K, pb, fused=False), 1, max(3, repeats // 4))
                lrow["ratio_median"] = lrow["composable_torch_same_gpu"]["median_ms"] / lrow["fused_call_labels_vs_packed"]["median_ms"]
                out[f"labels_K{K}_vs_64"] = lrow
                print(f"{res}^3 labels K={K}: pack {lrow['pack_labels']['median_ms']:.3f} ms, fused {lrow['fused_call_labels_vs_packed']['median_ms']:.3f} ms, "
                      f"composable {lrow['composable_torch_same_gpu']['median_ms']:.2f} ms, equal {lrow['equal']}", flush=True)
        del a, b, pa, pb
    return out


def quality(room, steps, inst_steps):
    from instance_nerf_amd import extract
    from instance_nerf_amd.nerf import NeRFNetwork
    from instance_nerf_amd.nerf.provider import NeRFDataset
    from instance_nerf_amd.nerf.utils import Trainer
    K = 16

    def run(tr, ds, n):
        it = iter(())
        for _ in range(n):
            try:
                batch = next(it)
            except StopIteration:
                it = iter(ds)
                batch = next(it)
            tr.train_one_step(batch)
    tmp = tempfile.mkdtemp(prefix="inr_overlap_probe_")
    scene = room.write_dataset(tmp, n_views=24, H=200, W=200, num_instances=K)
    net = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05, density_thresh=10, num_instances=K).to(DEV)
    ds = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096)
    run(Trainer("p_nerf", None, net, stage="nerf", device=DEV, lr=1e-2, iters=1500, workspace=None, mute=True), ds, steps)
    ds2 = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096, mask_dir=scene["mask_dir"],
                      num_instances=K)
    ti = Trainer("p_inst", None, net, stage="instance", device=DEV, lr=1e-2, iters=1500, update_extra_interval=10 ** 9,
                 workspace=None, mute=True)
    ti.global_step = 1
    run(ti, ds2, inst_steps)
    net.eval()
    res = 160
    ids = room_ids(room, res)
    n_inst = len(room.lo)
    gt_masks = torch.stack([ids == c for c in range(1, n_inst + 1)])
    boxes = []
    for m in gt_masks:
        idx = torch.nonzero(m)
        boxes.append(torch.cat([idx.min(0).values, idx.max(0).values + 1]).float().cpu())
    gt = {"masks": gt_masks, "labels": np.ones(n_inst, np.int64), "boxes": torch.stack(boxes)}
    out = {"workload": f"synthetic room, NeRF trained {steps} steps, K=16 instance field {inst_steps} steps; extract_instances at "
                       f"{res}^3, sigma_thresh = 1; ground truth = the voxel centres inside each analytic box (solid boxes)"}
    for name, kw in (("raw", {}), ("components_largest", {"components": "largest"})):
        r = ti.evaluate_instance_masks(gt, max_side=res, sigma_thresh=1.0, **kw)
        out[name] = {k: (v if isinstance(v, float) else [round(float(x), 4) for x in v.tolist()]) for k, v in r.items()}
        print(name, {k: round(v, 4) for k, v in r.items() if isinstance(v, float)}, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--inst-steps", type=int, default=1500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    room = RoomScene()
    out = {"workload": "analytic room lattice over [-1, 1]^3; A = k box masks, B = 12 analytic instance masks + k - 12 box masks",
           "method": "device events on the launch stream after warm-up, median / min / max; one process",
           "timing": {}}
    for res in (160, 256):
        out["timing"][f"{res}^3"] = timing(room, res, a.repeats)
    if a.train:
        out["quality"] = quality(room, a.steps, a.inst_steps)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
