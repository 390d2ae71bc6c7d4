"""The detector tail on the GPU (instance_nerf_amd/detections.py, csrc/detect.hip): timing of the fused kernels against the
composable torch paths on the same GPU and inputs.  Writes profiles/paste_probe.json.

1. Paste at 160^3, M = 20, N = 30 and N = 100, two box sets: the analytic room's boxes (cycled to N, in grid units) and
   boxes that cover the whole grid - the worst case for the kernel's support skip.  Fused (``inr_paste_masks``: one fill
   and one launch) against the composable path (chunked ``F.grid_sample`` then ``>=``).  The thresholded outputs are
   compared first; a GPU ``grid_sample`` may round differently from the fp32 contract of include/inr.h (which the GPU
   tests hold to the bit against the CPU reference), so equality here means: at most 8 bits differ, and the fused sample
   of every differing voxel lies within 64 ulp (4e-6) of the threshold (a tie between two fp32 roundings).  Per CALL: time, bytes written (the planes:
   N * ceil(V / 64) * 8) and the TB/s that is.  These are CALL times - device events around the whole Python call, which
   includes the output allocations, the ctypes call and the fill before the launch - not kernel times.  Peak memory of both paths: torch's allocator high-water mark over a call.
2. ``inr_planes_to_voxel_words`` on the N = 100 planes (four launches) against ``masks.pack_mask_words`` of the bools.
3. NMS at n = 1000, 2 classes: sort + ``inr_nms_3d_pairs`` + ``inr_nms_3d_scan`` against the greedy torch loop.
Warm-up, then medians with min / max, bracketed by device events.  Numbers are written down as measured.
python tools/paste_probe.py [--repeats 20] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import detections as det, masks as mk       # noqa: E402
from instance_nerf_amd.scene import RoomScene                       # noqa: E402

DEV = torch.device("cuda", 0)
RES, M = 160, 20
# Bits that may differ from the GPU's own grid_sample, and how far from the threshold the fused sample of such a voxel may
# lie, in units of 2^-24 = ulp(0.5).  Two correct fp32 evaluations differ by the rounding of the sample position (p < 32:
# half an ulp is 2^-20 = 16 units; a few operations per axis, a mask gradient of at most 1 per texel) plus about 11
# roundings of the weighted sum of values in [0, 1] (11 units): 64 units bounds both.  A wrong tap or weight is off by 1e-2.
MAX_TIES, TIE_ULPS = 8, 64


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


def box_sets(N):
    room = RoomScene()
    lo, hi = (np.asarray(room.lo) + 1) / 2 * RES, (np.asarray(room.hi) + 1) / 2 * RES
    rooms = np.concatenate([lo, hi], 1).astype(np.float32)
    rooms = rooms[np.arange(N) % len(rooms)] + (np.arange(N) // len(rooms))[:, None].astype(np.float32) * 0.37
    whole = np.tile(np.asarray([[0, 0, 0, RES, RES, RES]], np.float32), (N, 1))
    return {"room_boxes": rooms, "whole_grid": whole}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "paste_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU: no fallback"
    shape, V = (RES, RES, RES), RES ** 3
    rec = {"device": torch.cuda.get_device_name(0), "grid": list(shape), "M": M, "paste": [], "repeats": args.repeats}
    gen = torch.Generator(device="cpu").manual_seed(0)
    for N in (30, 100):
        probs = torch.clamp((torch.rand(N, M, M, M, generator=gen) - 0.5) * 3 + 0.5, 0, 1).to(DEV)
        for name, boxes in box_sets(N).items():
            b = torch.from_numpy(boxes).to(DEV)
            fused = det.paste_masks(probs, b, shape, out="planes")
            twin = det.paste_masks(probs, b, shape, out="planes", fused=False)
            x = fused[0] ^ twin[0]
            rows, cols = torch.where(x != 0)
            differ, off = 0, 0.0
            assert rows.numel() <= MAX_TIES, (name, N, int(rows.numel()))
            for n, w in zip(rows.tolist(), cols.tolist()):             # every differing voxel must be a tie at the threshold
                lanes = torch.where((x[n, w] >> torch.arange(64, device=DEV)) & 1 != 0)[0] + 64 * w
                soft = det.paste_masks(probs[n:n + 1], b[n:n + 1], shape, out="soft").reshape(-1)[lanes]
                differ += int(lanes.numel())
                off = max(off, float((soft - 0.5).abs().max()))
            assert differ <= MAX_TIES and off <= TIE_ULPS * 2.0 ** -24, (name, N, differ, off)
            set_bits = int(fused[1].sum())
            del fused, twin, x
            row = {"boxes": name, "N": N, "set_bits": set_bits, "bits_differing_from_gpu_grid_sample": differ,
                   "largest_distance_of_a_differing_sample_from_the_threshold": off,
                   "plane_bytes": N * ((V + 63) // 64) * 8}
            row["fused"] = timed(lambda: det.paste_masks(probs, b, shape, out="planes"), 3, args.repeats)
            row["fused"]["plane_write_TB_per_s"] = row["plane_bytes"] / (row["fused"]["median_ms"] * 1e-3) / 1e12
            row["composable"] = timed(lambda: det.paste_masks(probs, b, shape, out="planes", fused=False), 1, max(3, args.repeats // 5))
            row["fused"]["peak_bytes"] = peak_bytes(lambda: det.paste_masks(probs, b, shape, out="planes"))
            row["composable"]["peak_bytes"] = peak_bytes(lambda: det.paste_masks(probs, b, shape, out="planes", fused=False))
            row["speedup"] = row["composable"]["median_ms"] / row["fused"]["median_ms"]
            rec["paste"].append(row)
            print(json.dumps(row), flush=True)
            if N == 100 and name == "room_boxes":
                packed = det.paste_masks(probs, b, shape, out="planes")
                bools = det.paste_masks(probs, b, shape, out="masks")
                got, want = det.planes_to_voxel_words(packed), mk.pack_mask_words(bools, DEV)
                assert all(torch.equal(x, y) for x, y in zip(got, want))
                del got, want
                vw = {"N": N, "launches": (N + 31) // 32, "bytes_read": N * ((V + 63) // 64) * 8, "bytes_written": ((N + 31) // 32) * V * 4,
                      "fused": timed(lambda: det.planes_to_voxel_words(packed), 3, args.repeats),
                      "pack_mask_words": timed(lambda: mk.pack_mask_words(bools, DEV), 1, max(3, args.repeats // 5))}
                vw["fused"]["peak_bytes"] = peak_bytes(lambda: det.planes_to_voxel_words(packed))
                vw["pack_mask_words"]["peak_bytes"] = peak_bytes(lambda: mk.pack_mask_words(bools, DEV))
                rec["planes_to_voxel_words"] = vw
                print(json.dumps(vw), flush=True)
                del packed, bools
    n = 1000
    lo = torch.rand(n, 3, generator=gen) * 40
    boxes = torch.cat([lo, lo + 2 + torch.rand(n, 3, generator=gen) * 6], 1).to(DEV)
    scores, cls = torch.rand(n, generator=gen).to(DEV), torch.randint(1, 3, (n,), generator=gen).to(DEV)
    keep = det.batched_nms_3d(boxes, scores, cls, 0.2)
    assert torch.equal(keep, det.batched_nms_3d(boxes, scores, cls, 0.2, fused=False))
    rec["nms"] = {"n": n, "classes": 2, "kept": int(keep.numel()),
                  "fused": timed(lambda: det.batched_nms_3d(boxes, scores, cls, 0.2), 3, args.repeats),
                  "greedy_torch_loop": timed(lambda: det.batched_nms_3d(boxes, scores, cls, 0.2, fused=False), 1, 3)}
    print(json.dumps(rec["nms"]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
