"""Mesh extraction (extract.extract_mesh / inr_mesh_count + inr_mesh_emit) on a trained room at 160 and 256 voxels a side:
the scene mesh (face labels + colours) and one mesh per instance channel.

The room is written to disk and its NeRF and K = 16 instance field trained by the product's Trainer, as
tools/instance_extract_probe.py does.  Per resolution: V and F; device-event times (median / min / max after warm-up) of
the field launches that feed the mesh (instance_lattice with the logit; forward_lattice for the colours), of
inr_mesh_count, of inr_mesh_emit and of the whole extract_mesh call (which includes the host read-back of (V, F) and the
allocations); the mesh kernels' own bytes - 4 B of field per extended-lattice point read once per pass plus the workspace
and outputs written - and the bytes/s they achieve; and the same for the per-instance meshes (count + emit only: the
field is evaluated once).
python tools/mesh_extract_probe.py [--steps 2000] [--inst-steps 1500] [--repeats 10] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import _lib, extract                          # noqa: E402
from instance_nerf_amd.nerf import NeRFNetwork                      # noqa: E402
from instance_nerf_amd.nerf.provider import NeRFDataset             # noqa: E402
from instance_nerf_amd.nerf.utils import Trainer                    # noqa: E402
from instance_nerf_amd.scene import RoomScene                       # noqa: E402
from instance_extract_probe import run, timed                       # noqa: E402

DEV = torch.device("cuda", 0)


def mesh_calls(lat, select, want_rgb, want_fl):
    """-> (count(), emit(), V, F): the two library calls on preallocated buffers, as extract.mesh_from_lattice makes them."""
    lib = _lib.load()
    P = _lib.ptr
    field = lat["field"]
    W, L, H = (int(v) for v in field.shape)
    stride = int(field.stride(2))
    nbytes = int(lib.inr_mesh_workspace_bytes(W, L, H, 1))
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=DEV)
    counts = torch.empty(2, dtype=torch.int32, device=DEV)
    head = (_lib.c_void_p(field.data_ptr()), stride, float(lat["iso"]), float(extract.MESH_CLAMP),
            P(lat["labels"], torch.uint8, "labels", allow_none=True), int(select))

    def count():
        _lib.check(lib.inr_mesh_count(*head, W, L, H, 1, P(ws), nbytes, P(counts), _lib.stream_ptr()), "mesh_count")

    count()
    V, F = (int(v) for v in counts.tolist())
    vertices = torch.empty(max(V, 1), 3, dtype=torch.float32, device=DEV)
    faces = torch.empty(max(F, 1), 3, dtype=torch.int32, device=DEV)
    colors = torch.empty(max(V, 1), 3, dtype=torch.float32, device=DEV) if want_rgb else None
    flab = torch.empty(max(F, 1), dtype=torch.uint8, device=DEV) if want_fl else None
    ax, ext = lat["axes"], lat["ext"]

    def emit():
        _lib.check(lib.inr_mesh_emit(*head, P(lat["rgb"], allow_none=True) if want_rgb else None, P(ax[0]), P(ax[1]), P(ax[2]),
                                     W, L, H, ext[0], ext[1], ext[2], 1, P(ws), nbytes, V, F, P(vertices), P(faces),
                                     P(colors, allow_none=True), P(flab, allow_none=True), _lib.stream_ptr()), "mesh_emit")

    return count, emit, V, F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--inst-steps", type=int, default=1500)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    K = 16
    room = RoomScene()
    scene = room.write_dataset(tempfile.mkdtemp(prefix="inr_mesh_probe_"), n_views=24, H=200, W=200, num_instances=K)
    net = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05, density_thresh=10, num_instances=K).to(DEV)
    ds = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096)
    run(Trainer("p_nerf", None, net, stage="nerf", device=DEV, lr=1e-2, iters=1500, workspace=None, mute=True), ds, a.steps)
    ds2 = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096, mask_dir=scene["mask_dir"],
                      num_instances=K)
    net.mean_density = net.mean_density
    ti = Trainer("p_inst", None, net, stage="instance", device=DEV, lr=1e-2, iters=1500, update_extra_interval=10 ** 9,
                 workspace=None, mute=True)
    ti.global_step = 1
    run(ti, ds2, a.inst_steps)
    net.eval()
    out = {"workload": f"synthetic room, NeRF trained {a.steps} steps, K={K} instance field {a.inst_steps} steps; voxel-centre "
                       "lattice over [-1, 1]^3 with the virtual outside layer, threshold 10", "per_resolution": {}}
    for R in (160, 256):
        lat = extract.mesh_lattices(net, resolution=R, threshold=10.0, labels=True, colors=True)
        axes = lat["axes"]
        dirs, sh = extract.view_dirs(net, DEV)
        t_inst = timed(lambda: net.instance_lattice(axes, 10.0, want_logit=True), 2, a.repeats)
        t_rgb = timed(lambda: net.forward_lattice(axes, dirs, logit_min=extract.LOGIT_MIN, sh=sh), 2, a.repeats)
        count, emit, V, F = mesh_calls(lat, -1, True, True)
        t_count, t_emit = timed(count, 2, a.repeats), timed(emit, 2, a.repeats)
        t_call = timed(lambda: extract.extract_mesh(net, resolution=R, threshold=10.0), 2, a.repeats)
        t_meshes = timed(lambda: extract.mesh_of_lattices(lat), 2, a.repeats)
        n_ext = (R + 2) ** 3
        n_blocks = (n_ext + 255) // 256
        # classify: field 4 B + label 1 B read, mask 1 B written; offsets: mask read, 4 B written; vertices: mask + offset
        # read; faces: field + label read again; outputs: 12 B (+ 12 B colour) per vertex, 12 B (+ 1 B) per face, and the
        # faces kernel reads 3 offsets + 3 masks per face
        count_bytes = n_ext * (4 + 1 + 1) + n_ext * (1 + 4) + 16 * n_blocks
        emit_bytes = n_ext * (1 + 4) + n_ext * (4 + 1) + V * 24 + F * (13 + 15)
        row = {"res": [R, R, R], "extended_points": n_ext, "V": V, "F": F,
               "field_instance_lattice_with_logit": t_inst, "field_forward_lattice_rgb": t_rgb,
               "mesh_count": t_count, "mesh_emit": t_emit, "mesh_of_lattices_call": t_meshes, "extract_mesh_call": t_call,
               "count_bytes": count_bytes, "emit_bytes": emit_bytes,
               "count_bytes_per_s": count_bytes / (t_count["median_ms"] * 1e-3),
               "emit_bytes_per_s": emit_bytes / (t_emit["median_ms"] * 1e-3), "instances": {}}
        present = torch.bincount(lat["labels"].reshape(-1).long(), minlength=256).tolist()
        tot_c = tot_e = 0.0
        for k in range(1, K):
            if not present[k]:
                continue
            ck, ek, Vk, Fk = mesh_calls(lat, k, True, False)
            tc, te = timed(ck, 1, max(3, a.repeats // 2)), timed(ek, 1, max(3, a.repeats // 2))
            row["instances"][k] = {"V": Vk, "F": Fk, "count_ms": tc["median_ms"], "emit_ms": te["median_ms"]}
            tot_c += tc["median_ms"]
            tot_e += te["median_ms"]
        row["instances_count_ms_total"], row["instances_emit_ms_total"] = tot_c, tot_e
        out["per_resolution"][R] = row
        print(f"{R}^3: V {V} F {F}; field {t_inst['median_ms']:.3f} ms (+ rgb {t_rgb['median_ms']:.3f}), count "
              f"{t_count['median_ms']:.3f} ms ({row['count_bytes_per_s'] / 1e12:.2f} TB/s), emit {t_emit['median_ms']:.3f} ms "
              f"({row['emit_bytes_per_s'] / 1e12:.2f} TB/s), mesh_of_lattices {t_meshes['median_ms']:.3f} ms, extract_mesh "
              f"{t_call['median_ms']:.3f} ms; {len(row['instances'])} instance meshes: count {tot_c:.3f} + emit {tot_e:.3f} ms",
              flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
