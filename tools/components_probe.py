"""Connected components on the GPU (extract.label_components / filter_components, csrc/components.hip) on the label volume
of a trained room at 160^3 and 256^3, K = 16, both connectivities.

Timing, device events on the launch stream after warm-up (median / min / max): inr_components_label (its three launches:
tile label, face merge, compress + sizes) and inr_components_filter (four launches) as two calls, the whole
filter_components call (allocations included), the same call through the composable torch path on the same GPU, and the
lattice kernel that produces the labels, for scale.  An export issues its launches back to back, so events on the stream
bracket an export, not a launch.  The split per launch (k_cc_tile, k_cc_merge, k_cc_compress, k_cc_init, k_cc_select,
k_cc_finish, k_cc_apply) comes from a kernel trace: `rocprofv3 --kernel-trace --output-format csv -d DIR -- python
tools/components_probe.py --launches-only --repeats R` issues nothing but R label + filter calls per configuration on
the same trained volume, and `tools/components_launches.py DIR R` reads the trace (-> profiles/components_kernels.txt).
Against each time, a LOWER BOUND of the bytes the call moves: every array it must read or write, once per
pass that needs it (labels 1 B, roots 4 B, confidence 4 B per voxel); re-reads of neighbours are not counted.

Quality, before and after components="largest" (lattice 160, sigma >= 1 as in the loop-closure test): per-id AABB IoU
against the analytic boxes, components per id, voxels per id, and the coverage of a held-out view's instance pixels by
the projected masks.  Numbers are written down as measured.
python tools/components_probe.py [--steps 2000] [--inst-steps 1500] [--repeats 10] [--out FILE] [--launches-only]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import _lib, extract, masks as pmasks       # noqa: E402
from instance_nerf_amd.nerf import NeRFNetwork                      # noqa: E402
from instance_nerf_amd.nerf.provider import NeRFDataset             # noqa: E402
from instance_nerf_amd.nerf.utils import Trainer, get_rays          # noqa: E402
from instance_nerf_amd.scene import RoomScene                       # noqa: E402

DEV = torch.device("cuda", 0)
K = 16


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


def box_ious(room, boxes, res):
    vox = 2.0 / np.asarray(res, np.float64)
    out = {}
    for b, (lo, hi) in enumerate(zip(room.lo, room.hi)):
        bx = boxes[b + 1]
        if bx[0] < 0:
            out[b + 1] = 0.0
            continue
        elo, ehi = -1.0 + bx[:3] * vox, -1.0 + (bx[3:] + 1) * vox
        inter = np.prod(np.clip(np.minimum(ehi, hi) - np.maximum(elo, lo), 0, None))
        out[b + 1] = float(inter / (np.prod(ehi - elo) + np.prod(hi - lo) - inter))
    return out


def coverage(room, net, result, tmp, name):
    path = pmasks.write_instance_masks_npz(os.path.join(tmp, name + ".npz"), result)
    m3 = pmasks.load_3d_masks(path)
    H = W = 200
    _, intr, _, _ = room.cameras(n=1, H=H, W=W, focal=W / 2.0)
    pose = room.look_at([0.3, -0.2, 0.1])[None]
    proj = pmasks.project_3d_masks(net, m3["masks"], [-1, -1, -1], [1, 1, 1], pose, intr, H, W)[0]
    rh = get_rays(torch.from_numpy(pose).to(DEV), intr, H, W)
    with torch.no_grad():
        ids = net.render(rh["rays_o"], rh["rays_d"], bg_color=1)["instance"][0].argmax(-1).cpu().numpy().reshape(H, W)
    sel = ids >= 1
    hit = proj[np.clip(ids - 1, 0, None), np.arange(H)[:, None], np.arange(W)[None, :]]
    return float(hit[sel].mean()), int(sel.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--inst-steps", type=int, default=1500)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches-only", action="store_true", help="after training, only --repeats label + filter calls per "
                    "configuration and nothing else: the run to put under a kernel trace")
    a = ap.parse_args()
    torch.manual_seed(0)
    room = RoomScene()
    tmp = tempfile.mkdtemp(prefix="inr_cc_probe_")
    scene = room.write_dataset(tmp, n_views=24, H=200, W=200, num_instances=K)
    net = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05, density_thresh=10, num_instances=K).to(DEV)
    ds = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096)
    run(Trainer("p_nerf", None, net, stage="nerf", device=DEV, lr=1e-2, iters=1500, workspace=None, mute=True), ds, a.steps)
    ds2 = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096, mask_dir=scene["mask_dir"],
                      num_instances=K)
    ti = Trainer("p_inst", None, net, stage="instance", device=DEV, lr=1e-2, iters=1500, update_extra_interval=10 ** 9,
                 workspace=None, mute=True)
    ti.global_step = 1
    run(ti, ds2, a.inst_steps)
    net.eval()
    lib = _lib.load()
    P = _lib.ptr
    out = {"workload": f"synthetic room, NeRF trained {a.steps} steps, K=16 instance field {a.inst_steps} steps; label volume "
                       "of extract_instances over [-1, 1]^3, sigma_thresh = density_thresh = 10", "timing": {}, "quality": {},
           "per_launch_split": "profiles/components_kernels.txt (kernel trace of a --launches-only run): an export issues "
                               "its launches back to back, so the stream events here bracket the export (label = tile + "
                               "merge + compress, filter = init + select + finish + apply)"}
    for side in (160, 256):
        base = extract.extract_instances(net, max_side=side)
        labels, conf = base["labels"], base["confidence"]
        W, L, H = (int(v) for v in labels.shape)
        n = W * L * H
        axes = extract.cached_axes(np.float32([-1, -1, -1]), np.float32([1, 1, 1]), base["res"], DEV)
        lattice = timed(lambda: net.instance_lattice(axes, 10.0), 2, a.repeats)
        nbytes = int(lib.inr_components_workspace_bytes(W, L, H))
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
        roots = torch.empty(W, L, H, dtype=torch.int32, device=DEV)
        lab_out, conf_out = torch.empty_like(labels), torch.empty_like(conf)
        per = torch.empty(3, K, dtype=torch.int32, device=DEV)
        row = {"res": [W, L, H], "voxels": n, "occupied_voxels": int((labels != 255).sum()), "instance_lattice_launch": lattice}
        for connectivity in (6, 26):
            def label():
                _lib.check(lib.inr_components_label(P(labels), W, L, H, connectivity, P(ws), nbytes, P(roots), _lib.stream_ptr()))

            def filt():
                _lib.check(lib.inr_components_filter(P(labels), P(roots), P(conf), W, L, H, K, 1, 1, 1, P(ws), nbytes, P(lab_out),
                                                     P(conf_out), P(per[0]), P(per[1]), P(per[2]), _lib.stream_ptr()))
            if a.launches_only:
                for _ in range(a.repeats):
                    label()
                    filt()
                torch.cuda.synchronize()
                print(f"{side}^3 conn {connectivity}: {a.repeats} label + filter calls", flush=True)
                continue
            t_label = timed(label, 2, a.repeats)
            t_filter = timed(filt, 2, a.repeats)
            whole = timed(lambda: extract.filter_components(labels, conf, K=K, connectivity=connectivity), 2, a.repeats)
            torch_path = timed(lambda: extract.filter_components(labels, conf, K=K, connectivity=connectivity, fused=False), 1, 3)
            ref = extract.filter_components(labels, conf, K=K, connectivity=connectivity, fused=False)
            same = bool(torch.equal(ref["labels"], lab_out) and torch.equal(ref["roots"], roots))
            # lower bounds: label reads labels (1 B) and writes roots (4 B) in the tile pass, reads and rewrites roots and
            # touches sizes in the compress pass (4 + 4 B; sizes at roots only, not counted); filter reads labels + roots
            # in select (5 B) and labels + roots + confidence in apply (9 B), writes labels + confidence (5 B)
            b_label, b_filter = n * (1 + 4 + 4 + 4), n * (5 + 9 + 5)
            row[f"connectivity_{connectivity}"] = {
                "label_call_3_launches": t_label, "filter_call_4_launches": t_filter, "filter_components_whole_call": whole,
                "composable_torch_same_gpu": torch_path, "speedup_median": torch_path["median_ms"] / whole["median_ms"],
                "label_min_bytes": b_label, "label_min_TB_per_s": b_label / (t_label["median_ms"] * 1e-3) / 1e12,
                "filter_min_bytes": b_filter, "filter_min_TB_per_s": b_filter / (t_filter["median_ms"] * 1e-3) / 1e12,
                "equal_to_composable": same, "n_components": per[0].tolist(), "kept_voxels": per[1].tolist()}
            print(f"{side}^3 conn {connectivity}: label {t_label['median_ms']:.3f} ms, filter {t_filter['median_ms']:.3f} ms, whole "
                  f"call {whole['median_ms']:.3f} ms, torch path {torch_path['median_ms']:.1f} ms "
                  f"(x{torch_path['median_ms'] / whole['median_ms']:.0f}), lattice {lattice['median_ms']:.3f} ms, equal {same}",
                  flush=True)
        out["timing"][str(side)] = row
    if a.launches_only:
        return
    # ---- quality: 160, sigma >= 1 (the loop-closure setting) and sigma >= 10 (the default)
    for thresh in (1.0, 10.0):
        q = {}
        for name, kw in (("before", {}), ("largest_6", dict(components="largest", connectivity=6)),
                         ("largest_26", dict(components="largest", connectivity=26))):
            r = extract.extract_instances(net, max_side=160, sigma_thresh=thresh, **kw)
            ious = box_ious(room, r["boxes"].cpu().numpy(), r["res"])
            cov, pixels = coverage(room, net, r, tmp, f"{name}_{thresh}")
            q[name] = {"box_iou": {k: round(v, 4) for k, v in ious.items()}, "box_iou_mean": float(np.mean(list(ious.values()))),
                       "voxels_per_id": r["counts"].tolist()[1:13], "held_out_coverage": cov, "held_out_pixels": pixels}
            if "n_components" in r:
                q[name]["components_per_id"] = r["n_components"].tolist()[1:13]
                q[name]["raw_voxels_per_id"] = r["raw_counts"].tolist()[1:13]
            print(f"sigma >= {thresh} {name}: mean box IoU {q[name]['box_iou_mean']:.4f}, coverage {cov:.4f}", flush=True)
        clean = room.instance_of_points(extract.lattice([-1, -1, -1], [1, 1, 1], [160] * 3, "cpu").numpy()).reshape(160, 160, 160)
        q["analytic_voxels_per_id"] = [int((clean == k).sum()) for k in range(1, 13)]
        out["quality"][f"sigma_{thresh:g}"] = q
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
