"""Background sphere model (NeRFNetwork(bg_radius > 0), csrc/background.hip) on one MI355X, bench scene:

1. the background forward + blend of a 640 000-ray (800x800) eval frame - the fused launch (``blend_background``)
   against the composable path (``background(sph_from_ray(..), d)``) + the tensor blend, on the same GPU and rays;
2. forward + backward at 4 096 rays (a training batch), fused node against the composable chain;
3. beside both: the whole frame and the whole training step (Trainer.train_step + backward + optimiser step) with and
   without the model.
Device events on the launch stream after warm-up, medians of ``--repeats``, the two compared calls alternating.  These
are CALL times (allocations, ctypes, launches), not kernel times.
python tools/background_probe.py [--repeats 20] [--out profiles/background_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import raymarching                               # noqa: E402
from instance_nerf_amd.nerf import NeRFNetwork                          # noqa: E402
from instance_nerf_amd.nerf.utils import Trainer, get_rays              # noqa: E402
from instance_nerf_amd.scene import RoomScene                           # noqa: E402

DEV = torch.device("cuda", 0)
H = W = 800
RADIUS = 32.0


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


def network(room, bg_radius):
    torch.manual_seed(0)
    net = NeRFNetwork(cuda_ray=True, min_near=0.05, bg_radius=bg_radius).to(DEV)
    net.density_bitfield.copy_(torch.as_tensor(room.density_bitfield(128, 1.0)).to(DEV))
    with torch.no_grad():
        net.encoder.embeddings.uniform_(-1, 1)
        if bg_radius > 0:
            net.encoder_bg.embeddings.uniform_(-1, 1)
            for layer in net.bg_net:
                torch.nn.init.kaiming_normal_(layer.weight)
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "background_probe.json"))
    args = ap.parse_args()
    room = RoomScene()
    poses, intr, _, _ = room.cameras(n=2, H=H, W=W, focal=400.0)
    r = get_rays(torch.as_tensor(poses[:1]).to(DEV), intr, H, W, patch=4)
    ro, rd = r["rays_o"][0].contiguous(), r["rays_d"][0].contiguous()
    N = ro.shape[0]
    net, plain = network(room, RADIUS), network(room, -1)
    rec = {"rays_frame": N, "rays_batch": 4096, "radius": RADIUS, "device": torch.cuda.get_device_name(0)}

    # 1. frame: background forward + blend
    net.eval()
    image0, ws = torch.rand(N, 3, device=DEV), torch.rand(N, device=DEV)
    image = image0.clone()

    def fused_blend():
        image.copy_(image0)
        net.fused_background = True
        net.blend_background(ro, rd, ws, image)

    def composable_blend():
        image.copy_(image0)
        net.fused_background = False
        with torch.no_grad():
            bg = net.background(raymarching.sph_from_ray(ro, rd, RADIUS), rd)
            image.add_((1 - ws).unsqueeze(-1) * bg)

    def copy_only():
        image.copy_(image0)

    t = alternating({"fused": fused_blend, "composable": composable_blend, "copy_only": copy_only}, 3, args.repeats)
    fused_blend()
    a = image.clone()
    composable_blend()
    rec["frame_blend"] = dict(t, max_abs_diff=float((a - image).abs().max()),
                              fused_minus_copy_ms=t["fused"]["median_ms"] - t["copy_only"]["median_ms"],
                              composable_minus_copy_ms=t["composable"]["median_ms"] - t["copy_only"]["median_ms"])

    # 2. training batch: forward + backward
    net.train()
    idx = torch.randperm(N, device=DEV)[:4096]
    bo, bd, G = ro[idx].contiguous(), rd[idx].contiguous(), torch.randn(4096, 3, device=DEV)
    params = [net.encoder_bg.embeddings, net.bg_net[0].weight, net.bg_net[1].weight]

    def fwd_bwd(fused):
        def run():
            net.fused_background = fused
            torch.autograd.grad((net.background_rays(bo, bd) * G).sum(), params)
        return run

    rec["batch_forward_backward"] = alternating({"fused": fwd_bwd(True), "composable": fwd_bwd(False)}, 3, args.repeats)
    net.fused_background = True

    # 3. whole frame and whole training step, with and without the model
    def frame(n):
        def run():
            with torch.no_grad():
                n.eval().render(ro[None], rd[None], bg_color=1, infer_mode="fused")
        return run

    rec["frame"] = alternating({"with_background": frame(net), "without": frame(plain)}, 3, args.repeats)
    data = {"rays_o": bo[None], "rays_d": bd[None], "images": torch.rand(1, 4096, 3, device=DEV)}
    trainers = {k: Trainer(k, None, n, device=DEV, workspace=None, ema_decay=None) for k, n in (("with_background", net), ("without", plain))}

    def step(tr):
        def run():
            tr.model.train()
            tr.optimizer.zero_grad(set_to_none=True)
            _, _, loss = tr.train_step(data)
            loss.backward()
            tr.optimizer.step()
        return run

    rec["train_step"] = alternating({k: step(tr) for k, tr in trainers.items()}, 5, args.repeats)
    f, c = rec["frame_blend"]["fused_minus_copy_ms"], rec["frame_blend"]["composable_minus_copy_ms"]
    rec["summary"] = {
        "frame_blend_fused_over_composable": f / c,
        "batch_fused_over_composable": rec["batch_forward_backward"]["fused"]["median_ms"] / rec["batch_forward_backward"]["composable"]["median_ms"],
        "frame_share_of_background": f / rec["frame"]["with_background"]["median_ms"],
        "frame_with_over_without": rec["frame"]["with_background"]["median_ms"] / rec["frame"]["without"]["median_ms"],
        "train_step_with_over_without": rec["train_step"]["with_background"]["median_ms"] / rec["train_step"]["without"]["median_ms"],
    }
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec["summary"]))


if __name__ == "__main__":
    main()
