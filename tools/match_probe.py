"""2-D mask matching on the GPU (masks.match_masks / project_and_match, csrc/match.hip) on the bench scene: 800x800 views,
30 voxel masks at 160^3 (the set-up of tools/project_probe.py; the masks are boxes, as a detector's are, not noise).

1. The two device calls (inr_match_count + inr_match_assign through masks.match_ranked) at B = 1 and B = 32 views against
   the composable torch path on the same GPU and the same ranked inputs; outputs compared for equality.
2. masks.project_and_match per view against masks.project_3d_masks (no PNGs) followed by the composable match - the
   hand-over as it was before the matcher existed.
Device events on the launch stream after warm-up, median / min / max.  The count kernel's rate is quoted against the 8
bytes per pixel it reads (4 B of seg + 4 B of words at k <= 32).  Per-launch times come from a kernel trace of a
--launches-only run: `rocprofv3 --kernel-trace --stats -d DIR -- python tools/match_probe.py --launches-only`.
python tools/match_probe.py [--repeats 20] [--views 32] [--out profiles/match_probe.json] [--launches-only]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import _lib, masks as pm                        # noqa: E402
from instance_nerf_amd.nerf import NeRFNetwork                          # noqa: E402
from instance_nerf_amd.nerf.utils import get_rays                       # noqa: E402
from instance_nerf_amd.scene import RoomScene                           # noqa: E402

DEV = torch.device("cuda", 0)
K, RES, H, W = 30, 160, 800, 800


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


def box_masks(room, rng):
    occ = room.occupancy_grid(RES, 1.0) > 0
    out = np.zeros((K, RES, RES, RES), bool)
    for i in range(K):
        lo = rng.integers(0, RES - 40, size=3)
        hi = lo + rng.integers(24, 40, size=3)
        out[i, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        out[i] &= occ | (rng.random(3).sum() > 1.5)          # some masks keep their whole box, most only its occupied part
    return out


def segments(words, rng):
    """Coherent 2-D segments for packed views [n, 1, H, W]: a pixel inside a projection belongs to the segment of its
    lowest candidate, the rest to a coarse grid of stuff segments; borders unlabeled, one grid column background."""
    n = words.shape[0]
    w = words[:, 0].long() & 0xFFFFFFFF
    low = torch.log2((w & -w).clamp(min=1).double()).long() + 1
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    grid = (40 + (yy // 100) * 8 + xx // 100).expand(n, H, W)
    seg = torch.where(w != 0, low, grid)
    seg = torch.where((xx // 100 == 3).expand(n, H, W) & (w == 0), torch.zeros_like(seg), seg)
    seg[:, :4], seg[:, -4:] = -1, -1
    return seg.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches-only", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    room = RoomScene()
    net = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05).to(DEV).eval()
    net.density_bitfield.copy_(torch.from_numpy(room.density_bitfield(128, 1.0)).to(DEV))
    poses, intr, _, _ = room.cameras(n=a.views, H=H, W=W, focal=400.0)
    poses = torch.from_numpy(poses).to(DEV)
    m3 = box_masks(room, rng)
    order = pm.candidate_order(range(1, K + 1))
    ids = [i + 1 for i in order]
    packed = (K, pm.pack_mask_words(m3[order], DEV))
    lib = _lib.load()
    P = H * W
    # the projector's sums of one view set the threshold: half of the largest sum (an untrained field spreads its weights)
    r = get_rays(poses[:1], intr, H, W, patch=4)
    soft, _ = pm.soft_project(net, None, [-1, -1, -1], [1, 1, 1], r["rays_o"][0], r["rays_d"][0], packed=packed)
    thresh = 0.5 * float(soft.max())
    words = torch.empty(a.views, 1, H, W, dtype=torch.int32, device=DEV)
    for v in range(a.views):
        r = get_rays(poses[v:v + 1], intr, H, W, patch=4)
        soft, _ = pm.soft_project(net, None, [-1, -1, -1], [1, 1, 1], r["rays_o"][0], r["rays_d"][0], packed=packed)
        _lib.check(lib.inr_pack_mask_bits(_lib.ptr(soft), _lib.ptr(r["inds"][0].contiguous()), P, K, thresh, P,
                                          _lib.ptr(words[v]), _lib.stream_ptr()))
    seg = segments(words, rng)
    ranks, S = pm._rank_segments(seg.reshape(a.views, P).contiguous())
    ids_t = torch.tensor(ids, dtype=torch.int32, device=DEV)
    flatw = words.reshape(a.views, 1, P)
    covered = float((words != 0).float().mean())
    out = {"workload": f"synthetic room, untrained field, {a.views} views {H}x{W}, {K} box masks at {RES}^3, projection "
                       f"threshold {thresh:.4f} (half the largest sum of view 0), {covered:.3f} of the pixels inside a "
                       f"projection, S = {S} segments per view", "match": {}, "pipeline": {}}
    for B in (1, a.views):
        rk, wd = ranks[:B].contiguous(), flatw[:B].contiguous()
        if a.launches_only:
            for _ in range(a.repeats):
                pm.match_ranked(rk, wd, S, K, ids_t)
            torch.cuda.synchronize()
            print(f"B = {B}: {a.repeats} match_ranked calls", flush=True)
            continue
        fused = timed(lambda: pm.match_ranked(rk, wd, S, K, ids_t), 3, a.repeats)
        twin = timed(lambda: pm._match_composable(rk, None, wd, S, K, ids_t, 0.05), 1, max(3, a.repeats // 4))
        same = bool(torch.equal(pm.match_ranked(rk, wd, S, K, ids_t), pm._match_composable(rk, None, wd, S, K, ids_t, 0.05)))
        out["match"][f"B_{B}"] = {"fused_count_plus_assign": fused, "composable_torch_same_gpu": twin,
                                  "ratio_median": twin["median_ms"] / fused["median_ms"], "equal": same,
                                  "count_bytes_read": 8 * B * P,
                                  "count_plus_assign_GB_per_s_of_8B_per_pixel": 8 * B * P / (fused["median_ms"] * 1e-3) / 1e9}
        print(f"B = {B}: fused {fused['median_ms']:.3f} ms, composable {twin['median_ms']:.2f} ms "
              f"(x{twin['median_ms'] / fused['median_ms']:.1f}), equal {same}", flush=True)
    if a.launches_only:
        return
    nv = 4
    seg4, poses4 = seg[:nv], poses[:nv]

    def new_chain():
        return pm.project_and_match(net, m3, [-1, -1, -1], [1, 1, 1], poses4, intr, H, W, seg4, thresh=thresh)

    def old_chain():
        proj = pm.project_3d_masks(net, m3, [-1, -1, -1], [1, 1, 1], poses4, intr, H, W, thresh=thresh)
        return pm.match_masks(seg4, torch.from_numpy(proj).to(DEV), fused=False)
    t_new, t_old = timed(new_chain, 1, 5), timed(old_chain, 1, 3)
    same = bool(torch.equal(new_chain(), old_chain()))
    out["pipeline"] = {"views": nv, "project_and_match_ms_per_view": {k: (v / nv if k != "repeats" else v) for k, v in t_new.items()},
                       "project_3d_masks_plus_composable_ms_per_view": {k: (v / nv if k != "repeats" else v) for k, v in t_old.items()},
                       "ratio_median": t_old["median_ms"] / t_new["median_ms"], "equal": same}
    print(f"per view: project_and_match {t_new['median_ms'] / nv:.2f} ms, project_3d_masks + composable match "
          f"{t_old['median_ms'] / nv:.2f} ms, equal {same}", flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
