"""3-D instance masks of the instance field (``extract.extract_instances`` / ``NeRFNetwork.instance_lattice`` /
``inr_instance_lattice`` + ``inr_instance_volume_stats``) on the MI355X: against the C oracle on O(1) parameters, against
the composable path, on a trained room against its analytic geometry, through the npz file and the projection back
into a view, and under the exact-fp32 library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# an odd lattice (W not a multiple of 16) whose box reaches past the bound on every axis: clamped coordinates
BOX_MIN = np.asarray([-1.15, -0.9, -1.05], np.float32)
BOX_MAX = np.asarray([1.1, 0.95, 1.2], np.float32)
RES = np.asarray([37, 24, 19])


def _net(p, K, **kw):
    from instance_nerf_amd.nerf import NeRFNetwork
    net = NeRFNetwork(cuda_ray=True, num_instances=K, min_near=0.05, **kw).to(DEV)
    net.load_state_dict({"encoder.embeddings": p["embeddings"], "sigma_net.0.weight": p["sigma_w0"],
                         "sigma_net.1.weight": p["sigma_w1"], "color_net.0.weight": p["color_w0"],
                         "color_net.1.weight": p["color_w1"], "color_net.2.weight": p["color_w2"],
                         "instance_encoder.embeddings": p["inst_embeddings"], "instance_net.0.weight": p["inst_w0"],
                         "instance_net.1.weight": p["inst_w1"], "instance_net.2.weight": p["inst_w2"]}, strict=False)
    return net.eval()


def _params(K, negative=False, seed=0):
    from oracle.field import init_params
    from oracle.hashgrid import level_table
    p = init_params(seed=seed, table=level_table(), table_std=1.0, K=K)
    if negative:                       # h2 >= 0 after the ReLU: every logit <= 0, the zero-padded channels would win
        p["inst_w2"] = -p["inst_w2"].abs()
    return p


def _oracle(p, K, thresh, density_scale=1.0):
    """-> (occupied, log sigma, labels, confidence, top-2 margin) of the lattice voxels, [W*L*H] in (w, l, h) order."""
    from instance_nerf_amd import extract
    from oracle import c_port
    from oracle.hashgrid import level_table
    pts = extract.lattice(BOX_MIN, BOX_MAX, RES, "cpu").clamp(-1.0, 1.0).numpy()
    d = np.tile(np.asarray([[0.0, 0.0, 1.0]], np.float32), (pts.shape[0], 1))
    sigma, _ = c_port.nerf_forward(pts, d, p, 1.0, level_table())
    logits = c_port.instance_logits(pts, p, 1.0, level_table()).astype(np.float64)
    assert logits.shape[1] == K
    sigma = sigma.astype(np.float64) * density_scale
    srt = np.sort(logits, 1)
    margin = srt[:, -1] - srt[:, -2] if K > 1 else np.full(len(srt), np.inf)
    e = np.exp(logits - srt[:, -1:])
    return sigma >= thresh, np.log(np.maximum(sigma, 1e-30)), logits.argmax(1), 1.0 / e.sum(1), margin


def _median_sigma(p):
    from instance_nerf_amd import extract
    from oracle import c_port
    from oracle.hashgrid import level_table
    pts = extract.lattice(BOX_MIN, BOX_MAX, RES, "cpu").clamp(-1.0, 1.0).numpy()
    sig = c_port.nerf_forward(pts, np.tile([[0.0, 0.0, 1.0]], (len(pts), 1)).astype(np.float32), p, 1.0, level_table())[0]
    return float(np.median(sig)), sig.astype(np.float64)


@pytest.mark.parametrize("K,negative", [(16, False), (31, False), (31, True), (64, False), (5, False)])
def test_lattice_matches_the_oracle(K, negative):
    from instance_nerf_amd import extract
    p = _params(K, negative)
    net = _net(p, K)
    thresh, sig = _median_sigma(p)                   # half of the lattice occupied, half not
    occ_r, logsig, lab_r, conf_r, margin = _oracle(p, K, thresh)
    axes = extract.lattice_axes(BOX_MIN, BOX_MAX, RES, DEV)
    labels, conf, logit = net.instance_lattice(axes, thresh, want_logit=True)
    labels, conf = labels.cpu().numpy().reshape(-1).astype(np.int64), conf.cpu().numpy().reshape(-1)
    occ = labels != 255
    off_band = np.abs(logsig - np.log(thresh)) > 1e-3
    assert 0.2 < occ_r.mean() < 0.8
    assert np.array_equal(occ[off_band], occ_r[off_band])
    assert np.abs(logit.cpu().numpy().reshape(-1) - logsig)[sig > 1e-20].max() < 1e-3
    sure = occ & occ_r & off_band & (margin > 1e-3)
    assert sure.sum() > 0.3 * occ_r.sum()
    assert np.array_equal(labels[sure], lab_r[sure])
    assert labels[occ].max() < K                     # a padded channel never wins (K = 31: all logits negative)
    both = occ & occ_r
    assert np.abs(conf[both] - conf_r[both]).max() < 1e-5
    assert (conf[~occ] == 0).all() and (conf[occ] > 0).all() and (conf[occ] <= 1).all()
    if negative:
        assert (lab_r[occ_r] < K).all() and (margin[occ_r] > 0).any()


def test_fused_equals_composable_and_repeats_bit_for_bit():
    from instance_nerf_amd import extract
    K = 16
    p = _params(K, seed=3)
    net = _net(p, K)
    pts = extract.lattice(BOX_MIN, BOX_MAX, RES, DEV).clamp(-1.0, 1.0)
    with torch.no_grad():
        sig = net.density(pts)["sigma"].double().cpu().numpy()
        logits = net.instance(pts).double().cpu().numpy()
    thresh = float(np.median(sig))
    a = extract.extract_instances(net, BOX_MIN, BOX_MAX, res=RES, sigma_thresh=thresh)
    b = extract.extract_instances(net, BOX_MIN, BOX_MAX, res=RES, sigma_thresh=thresh)
    c = extract.extract_instances(net, BOX_MIN, BOX_MAX, res=RES, sigma_thresh=thresh, fused=False)
    for key in ("labels", "confidence", "counts", "boxes", "scores"):
        assert torch.equal(a[key], b[key]), key                     # bit-reproducible, statistics included
    assert a["labels"].dtype == torch.uint8 and tuple(a["labels"].shape) == tuple(RES)
    srt = np.sort(logits, 1)
    band = (np.abs(np.log(np.maximum(sig, 1e-30)) - np.log(thresh)) <= 1e-3) | (srt[:, -1] - srt[:, -2] <= 1e-3)
    la, lc = a["labels"].cpu().numpy().reshape(-1), c["labels"].cpu().numpy().reshape(-1)
    assert np.array_equal(la[~band], lc[~band])
    occ = (la != 255) & (lc != 255)
    assert np.abs(a["confidence"].cpu().numpy().reshape(-1)[occ] - c["confidence"].cpu().numpy().reshape(-1)[occ]).max() < 1e-5
    n_band = int(band.sum())
    assert int((a["counts"] - c["counts"]).abs().sum()) <= 2 * n_band
    if n_band == 0:
        assert torch.equal(a["boxes"], c["boxes"])
    # the statistics launch against the host form on the same volume
    hc, hb, hs = extract.volume_stats(a["labels"].cpu(), a["confidence"].cpu(), K)
    dc, db, ds = extract.volume_stats(a["labels"], a["confidence"], K)
    assert torch.equal(hc, dc.cpu()) and torch.equal(hb, db.cpu())
    assert torch.allclose(hs, ds.cpu(), rtol=1e-5, atol=1e-5)
    assert int(dc.sum()) == int((la != 255).sum())


def test_volume_stats_at_scale_are_reproducible():
    """4.1 M voxels (the 160^3 lattice): the full 512-workgroup partial pass, two calls bit-identical, equal to the host."""
    from instance_nerf_amd import extract
    g = torch.Generator(device=DEV).manual_seed(0)
    K = 64
    lab = torch.randint(0, 80, (160, 160, 160), device=DEV, generator=g).to(torch.uint8)
    lab[lab >= K] = 255
    conf = torch.where(lab != 255, torch.rand(lab.shape, device=DEV, generator=g), torch.zeros((), device=DEV))
    r1, r2 = extract.volume_stats(lab, conf, K), extract.volume_stats(lab, conf, K)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)
    h = extract.volume_stats(lab.cpu(), conf.cpu(), K)
    assert torch.equal(h[0], r1[0].cpu()) and torch.equal(h[1], r1[1].cpu())
    assert torch.allclose(h[2], r1[2].cpu(), rtol=1e-5)


def test_no_instance_head_is_an_error():
    from instance_nerf_amd import extract
    from instance_nerf_amd.nerf import NeRFNetwork
    net = NeRFNetwork(cuda_ray=True, num_instances=0).to(DEV)
    with pytest.raises(ValueError, match="no instance head"):
        extract.extract_instances(net, max_side=16)


# ---------------------------------------------------------------------------------------------- trained room
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The synthetic room with 12 boxes, written to disk (24 views of 200x200 + matched masks, K = 16), its NeRF and
    then its instance field trained through ``Trainer`` from those files."""
    from instance_nerf_amd.nerf import NeRFNetwork
    from instance_nerf_amd.nerf.provider import NeRFDataset
    from instance_nerf_amd.nerf.utils import Trainer
    from instance_nerf_amd.scene import RoomScene
    K = 16
    root = tmp_path_factory.mktemp("room")
    room = RoomScene()
    scene = room.write_dataset(str(root / "scene"), n_views=24, H=200, W=200, num_instances=K, ignore_frac=0.1)
    torch.manual_seed(0)
    net = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05, density_thresh=10, num_instances=K).to(DEV)

    def run(tr, ds, steps):
        it = iter(())
        for _ in range(steps):
            try:
                batch = next(it)
            except StopIteration:
                it = iter(ds)
                batch = next(it)
            tr.train_one_step(batch)

    ds = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096)
    run(Trainer("room_nerf", None, net, stage="nerf", device=torch.device(DEV), lr=1e-2, iters=1500, workspace=None,
                mute=True), ds, 2000)
    ds2 = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096, mask_dir=scene["mask_dir"],
                      num_instances=K)
    net.mean_density = net.mean_density
    ti = Trainer("room", None, net, stage="instance", device=torch.device(DEV), lr=1e-2, iters=1500,
                 update_extra_interval=10 ** 9, workspace=str(root / "ws"), mute=True)
    ti.global_step = 1
    run(ti, ds2, 2000)
    net.eval()
    return {"room": room, "net": net, "trainer": ti, "scene": scene, "root": root, "K": K}


def _centres(res):
    c = [(np.arange(int(n)) + 0.5) / int(n) * 2.0 - 1.0 for n in res]
    gw, gl, gh = np.meshgrid(*c, indexing="ij")
    return np.stack([gw.reshape(-1), gl.reshape(-1), gh.reshape(-1)], 1)


def test_trained_room_labels_and_boxes(trained):
    """Occupied voxels clear of every box face carry the room's analytic instance id: measured 0.869-0.872 on two runs
    (96 voxels on a side, sigma >= density_thresh = 10); the bar leaves 0.03.  The per-id AABBs are reported, not
    asserted: every id's voxel set includes stray voxels far from its box - floaters in free space and the unobserved
    space behind the walls, where neither the NeRF nor the instance field was supervised - so an AABB over ALL voxels of
    an id spans most of the room (IoU with the true box measured 0.001-0.017 for all twelve boxes, whatever the lattice
    size, threshold or box); a 0.7 IoU bar would need a robust box (largest connected component, trimmed bounds),
    which the extraction does not define."""
    from instance_nerf_amd import extract
    room, net = trained["room"], trained["net"]
    out = extract.extract_instances(net, max_side=96)
    res = out["res"]
    vox = 2.0 / res.astype(np.float64)
    x = _centres(res)
    lab = out["labels"].cpu().numpy().reshape(-1).astype(np.int64)
    occ = lab != 255
    # centres at least one voxel away from every box face: inside the shrunk box or outside the grown one, for every box
    clear = np.ones(len(x), bool)
    for lo, hi in zip(room.lo, room.hi):
        inner = np.all((x >= lo + vox) & (x <= hi - vox), 1)
        outer = np.any((x < lo - vox) | (x > hi + vox), 1)
        clear &= inner | outer
    gt = room.instance_of_points(x)
    sel = occ & clear
    agree = float((lab[sel] == gt[sel]).mean())
    # box IoU: the extracted AABB of id b + 1 against box b, for every box with enough occupied voxels inside it
    boxes = out["boxes"].cpu().numpy()
    ious = {}
    for b, (lo, hi) in enumerate(zip(room.lo, room.hi)):
        inside = np.all((x >= lo) & (x <= hi), 1) & occ
        if inside.sum() < 200 or b + 1 >= trained["K"]:
            continue
        bx = boxes[b + 1]
        if bx[0] < 0:
            ious[b] = 0.0
            continue
        elo, ehi = -1.0 + bx[:3] * vox, -1.0 + (bx[3:] + 1) * vox
        inter = np.prod(np.clip(np.minimum(ehi, hi) - np.maximum(elo, lo), 0, None))
        union = np.prod(ehi - elo) + np.prod(hi - lo) - inter
        ious[b] = float(inter / union)
    print(f"trained room: {int(occ.sum())} occupied voxels of {len(lab)}, label agreement {agree:.4f} on {int(sel.sum())}, "
          f"box IoU {json.dumps({k: round(v, 3) for k, v in ious.items()})}")
    assert sel.sum() > 1000 and len(ious) >= 4
    assert agree >= 0.84, agree


def test_loop_closure_through_the_npz_and_a_held_out_view(trained):
    """Extracted masks -> npz -> load_3d_masks -> project_3d_masks on a held-out pose: where the rendered instance
    arg-max is an id >= 1, the projection of that id's mask covers the pixel.  The masks are extracted at 160 voxels a
    side with sigma >= 1: the render's weights peak in front of the surface, where density is still rising, and a
    coarser or stricter lattice leaves those samples in unoccupied voxels (measured: 96 / sigma >= 10: 0.72,
    96 / 1: 0.90, 160 / 10: 0.77, 160 / 1: 0.934).  The bar leaves 0.03."""
    from instance_nerf_amd import extract, masks as pmasks
    from instance_nerf_amd.nerf.utils import get_rays
    room, net = trained["room"], trained["net"]
    out = extract.extract_instances(net, max_side=160, sigma_thresh=1.0)
    path = pmasks.write_instance_masks_npz(str(trained["root"] / "masks" / "room.npz"), out)
    m3 = pmasks.load_3d_masks(path)
    assert m3["masks"].shape == (trained["K"] - 1,) + tuple(int(v) for v in out["res"])
    H = W = 200
    _, intr, _, _ = room.cameras(n=1, H=H, W=W, focal=W / 2.0)
    pose = room.look_at([0.3, -0.2, 0.1])[None]
    proj = pmasks.project_3d_masks(net, m3["masks"], [-1, -1, -1], [1, 1, 1], pose, intr, H, W)[0]     # [k, H, W]
    held = torch.from_numpy(pose).to(DEV)
    rh = get_rays(held, intr, H, W)
    with torch.no_grad():
        ids = net.render(rh["rays_o"], rh["rays_d"], bg_color=1)["instance"][0].argmax(-1).cpu().numpy().reshape(H, W)
    sel = ids >= 1
    hit = proj[np.clip(ids - 1, 0, None), np.arange(H)[:, None], np.arange(W)[None, :]]
    agree = float(hit[sel].mean())
    print(f"loop closure: {int(sel.sum())} pixels with an instance id, projected masks agree on {agree:.4f}")
    assert sel.sum() > 2000
    assert agree >= 0.9, agree


def test_trainer_save_instance_masks(trained):
    from instance_nerf_amd import masks as pmasks
    ti, net = trained["trainer"], trained["net"]
    net.train()
    path = ti.save_instance_masks(max_side=48, min_voxels=5)
    assert path == os.path.join(str(trained["root"] / "ws"), "masks", "room.npz") and os.path.exists(path)
    assert net.training                                   # the previous mode is restored
    m3 = pmasks.load_3d_masks(path)
    assert m3["masks"].shape[0] == trained["K"] - 1 and m3["masks"].shape[1:] == (48, 48, 48)
    assert m3["masks"].any(axis=(1, 2, 3)).sum() >= 4
    net.eval()


def test_exact_fp32_library():
    """The lattice kernel under the -DINR_MLP_FP32=1 library (child process: a process binds one library): labels equal
    the oracle's off a 1e-5 margin band, confidence within 1e-5."""
    from instance_nerf_amd import build
    assert os.path.exists(build.LIB_FP32), "libinr_hip_fp32.so is built by __graft_entry__.build()"
    code = f"""
import json, sys, numpy as np
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, "tests")!r})
from test_instance_extract import _net, _params, _oracle, _median_sigma, BOX_MIN, BOX_MAX, RES, DEV
from instance_nerf_amd import extract
out = {{}}
for K in (16, 31):
    p = _params(K)
    net = _net(p, K)
    thresh = _median_sigma(p)[0]
    occ_r, logsig, lab_r, conf_r, margin = _oracle(p, K, thresh)
    labels, conf = net.instance_lattice(extract.lattice_axes(BOX_MIN, BOX_MAX, RES, DEV), thresh)
    labels, conf = labels.cpu().numpy().reshape(-1).astype(np.int64), conf.cpu().numpy().reshape(-1)
    occ = labels != 255
    off = np.abs(logsig - np.log(thresh)) > 1e-5
    sure = occ & occ_r & off & (margin > 1e-5)
    out[K] = [int((occ[off] != occ_r[off]).sum()), int((labels[sure] != lab_r[sure]).sum()), int(sure.sum()),
              float(np.abs(conf[occ & occ_r] - conf_r[occ & occ_r]).max())]
print("RES", json.dumps(out))
"""
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, INR_LIB_PATH=build.LIB_FP32), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RES")][-1][4:])
    print("exact-fp32 library: [occupancy mismatches, label mismatches, voxels compared, max confidence error]", res)
    for K, (occ_bad, lab_bad, n, cerr) in res.items():
        assert occ_bad == 0 and lab_bad == 0 and n > 1000 and cerr < 1e-5, (K, res)
