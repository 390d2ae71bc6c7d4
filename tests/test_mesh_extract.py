"""Triangle meshes on the MI355X (``inr_mesh_count`` / ``inr_mesh_emit``, ``extract.extract_mesh``, ``Trainer.save_mesh`` /
``save_instance_meshes``): the kernels against the numpy restatement tests/mesh_reference.py - integers equal, floats
bit-equal - on random fields and an analytic sphere; ``extract_mesh`` on an O(1)-parameter network against the
restatement applied to the lattices the field launches return; and end to end on a trained room through the PLY files."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_reference as mr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

BOX_MIN = np.asarray([-1.15, -0.9, -1.05], np.float32)
BOX_MAX = np.asarray([1.1, 0.95, 1.2], np.float32)
RES = np.asarray([37, 24, 19])


def _axes(shape, lo=(-1.0, -0.7, -0.2), hi=(1.0, 0.9, 1.3)):
    from instance_nerf_amd import extract
    return [a.cpu().numpy() for a in extract.lattice_axes(np.asarray(lo, np.float32), np.asarray(hi, np.float32), shape, "cpu")]


def _gpu_mesh(field, iso, clamp, axes, labels=None, select=-1, rgb=None, cap=True, stride=1, face_labels=False,
              ext=(2.0, 1.6, 1.5)):
    """The kernels on numpy inputs.  stride 4: the field is channel 3 of one [W, L, H, 4] tensor whose channels 0..2 are
    the colours, read in place."""
    from instance_nerf_amd import extract
    W, L, H = field.shape
    vol = torch.zeros(W, L, H, 4, dtype=torch.float32, device=DEV)
    if rgb is not None:
        vol[..., :3] = torch.from_numpy(rgb[..., :3]).to(DEV)
    if stride == 4:
        vol[..., 3] = torch.from_numpy(field).to(DEV)
        f = vol[..., 3]
        assert f.stride(2) == 4
    else:
        f = torch.from_numpy(field).to(DEV)
    out = extract.mesh_from_lattice(f, iso, [torch.from_numpy(a).to(DEV) for a in axes], ext,
                                    labels=None if labels is None else torch.from_numpy(labels).to(DEV), select=select,
                                    rgb=vol if rgb is not None else None, face_labels=face_labels, cap=cap, clamp=clamp)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, ref, what=""):
    """V, F, faces and face_labels equal; vertices and colours bit-equal (the kernels perform the restatement's fp32
    operations in the restatement's order: no contraction, IEEE division - no tolerance is needed)."""
    assert got["vertices"].shape == ref["vertices"].shape, (what, got["vertices"].shape, ref["vertices"].shape)
    assert got["faces"].shape == ref["faces"].shape, (what, got["faces"].shape, ref["faces"].shape)
    assert np.array_equal(got["faces"], ref["faces"]), what
    assert np.array_equal(_bits(got["vertices"]), _bits(ref["vertices"])), what
    if ref["colors"] is not None:
        assert np.array_equal(_bits(got["colors"]), _bits(ref["colors"])), what
    else:
        assert got["colors"] is None
    if ref["face_labels"] is not None and got["face_labels"] is not None:
        assert np.array_equal(got["face_labels"], ref["face_labels"]), what


def _random_inputs(shape, seed):
    rng = np.random.default_rng(seed)
    field = rng.normal(size=shape).astype(np.float32)
    # smooth it a little along h so that the surface is not pure salt and pepper, and plant the special values
    field[..., 1:] = 0.5 * (field[..., 1:] + field[..., :-1])
    flat = field.reshape(-1)
    idx = rng.choice(flat.size, size=min(12, flat.size), replace=False)
    for k, i in enumerate(idx):
        flat[i] = (np.nan, -np.inf, np.inf, 0.25)[k % 4]          # 0.25 = the iso value itself: inside
    labels = rng.integers(0, 4, size=shape).astype(np.uint8)
    labels[field < 0.25] = 255
    labels[rng.random(shape) < 0.02] = 255                        # labels and field disagree here and there
    rgb = rng.random(shape + (4,)).astype(np.float32)
    return field, labels, rgb


@pytest.mark.parametrize("shape", [(33, 17, 45), (1, 9, 12), (7, 1, 1), (5, 6, 1), (2, 2, 2)])
@pytest.mark.parametrize("cap", [True, False])
@pytest.mark.parametrize("stride", [1, 4])
def test_kernels_equal_the_restatement_on_random_fields(shape, cap, stride):
    field, labels, rgb = _random_inputs(shape, seed=sum(shape) + stride)
    axes = _axes(shape)
    iso, clamp = 0.25, 0.75
    ext = (2.0, 1.6, 1.5)
    modes = [dict(), dict(labels=labels, face_labels=True, rgb=rgb), dict(labels=labels, select=2, rgb=rgb),
             dict(labels=labels, select=0, face_labels=True)]
    for mode in modes:
        kw = dict(mode)
        want_fl = kw.pop("face_labels", False)
        ref = mr.marching_tetrahedra(field, iso, clamp, axes, cap=cap, ext=ext, want_face_labels=want_fl, **kw)
        got = _gpu_mesh(field, iso, clamp, axes, cap=cap, stride=stride, ext=ext, face_labels=want_fl, **kw)
        again = _gpu_mesh(field, iso, clamp, axes, cap=cap, stride=stride, ext=ext, face_labels=want_fl, **kw)
        what = (shape, cap, stride, sorted(mode))
        _assert_same(got, ref, what)
        assert (got["face_labels"] is not None) == want_fl
        for key in ("vertices", "faces", "colors", "face_labels"):           # two calls: identical bits
            if got[key] is not None:
                assert got[key].tobytes() == again[key].tobytes(), (what, key)
        assert not np.isnan(got["vertices"]).any()
        if cap and len(got["faces"]):
            assert mr.is_closed(got["faces"]), what
        if min(shape) < 2 and not cap:
            assert len(got["faces"]) == 0 and len(got["vertices"]) == 0


def test_kernels_equal_the_restatement_on_a_sphere():
    n = 41
    ax = _axes((n, n, n), lo=(-1, -1, -1), hi=(1, 1, 1))
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    field = (np.float32(0.6) - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    ref = mr.marching_tetrahedra(field, 0.0, 0.5, ax, cap=False)
    got = _gpu_mesh(field, 0.0, 0.5, ax, cap=False)
    _assert_same(got, ref, "sphere")
    assert mr.is_closed(got["faces"]) and mr.euler(got["vertices"], got["faces"]) == 2
    vol = mr.signed_volume(got["vertices"], got["faces"])
    assert 0.98 < vol / (4.0 / 3.0 * np.pi * 0.6 ** 3) < 1.0


def test_scan_carries_across_three_chunks_of_workgroups():
    """(131100, 2, 2) without the cap: 524400 points, 2049 workgroups of 256, so k_mesh_scan walks three chunks of 1024
    and carries both prefixes twice.  A sparse field (isolated inside points every 997 steps along W and on both sides of
    the points 262144 and 524288, where workgroups 1024 and 2048 begin) owns vertices and cells in every chunk and in the
    workgroups next to each chunk boundary."""
    shape = (131100, 2, 2)
    n_points = int(np.prod(shape))
    assert (n_points + 255) // 256 == 2049 > 2048
    rng = np.random.default_rng(11)
    field = (-0.1 - np.abs(rng.normal(size=shape))).astype(np.float32)
    sites = sorted(set(range(3, shape[0] - 1, 997)) | {65534, 65535, 65536, 65537, 131070, 131071, 131072, 131073})
    for k, w in enumerate(sites):
        field[w, (k >> 1) & 1, k & 1] = np.float32(0.1 + abs(rng.normal()))
    axes = _axes(shape)
    ref = mr.marching_tetrahedra(field, 0.0, 0.75, axes, cap=False)
    flat = lambda p: (p[:, 0] * shape[1] + p[:, 1]) * shape[2] + p[:, 2]                   # noqa: E731
    owner_wg = flat(ref["owners"]) // 256
    inside = ref["g"] >= 0
    cnt = sum(inside[a:shape[0] - 1 + a, b:1 + b, c:1 + c].astype(int) for a in (0, 1) for b in (0, 1) for c in (0, 1))
    cell_wg = flat(np.argwhere((cnt > 0) & (cnt < 8))) // 256
    for wg in (owner_wg, cell_wg):
        assert set(np.unique(wg // 1024)) == {0, 1, 2} and {1023, 1024, 2047, 2048} <= set(wg.tolist())
    got = _gpu_mesh(field, 0.0, 0.75, axes, cap=False)
    _assert_same(got, ref, "three scan chunks")
    assert len(got["vertices"]) == len(ref["owners"]) > 500 and len(got["faces"]) == len(ref["faces"]) > 500


def test_empty_result():
    field = np.full((6, 7, 8), -3.0, np.float32)
    got = _gpu_mesh(field, 0.0, 1.0, _axes(field.shape))
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3)


# ---------------------------------------------------------------------------------- extract_mesh on O(1) parameters
def _net(p, K, **kw):
    from instance_nerf_amd.nerf import NeRFNetwork
    net = NeRFNetwork(cuda_ray=True, num_instances=K, min_near=0.05, **kw).to(DEV)
    net.load_state_dict({"encoder.embeddings": p["embeddings"], "sigma_net.0.weight": p["sigma_w0"],
                         "sigma_net.1.weight": p["sigma_w1"], "color_net.0.weight": p["color_w0"],
                         "color_net.1.weight": p["color_w1"], "color_net.2.weight": p["color_w2"],
                         "instance_encoder.embeddings": p["inst_embeddings"], "instance_net.0.weight": p["inst_w0"],
                         "instance_net.1.weight": p["inst_w1"], "instance_net.2.weight": p["inst_w2"]}, strict=False)
    return net.eval()


def _params(K, seed=0):
    from oracle.field import init_params
    from oracle.hashgrid import level_table
    return init_params(seed=seed, table=level_table(), table_std=1.0, K=K)


def _quiet_threshold(net):
    """A threshold in the widest gap between neighbouring density logits near the lattice's median, so that the two field
    paths classify every point alike: they run the same sigma network through different launches and differ by the fp32
    rounding of its 64-wide dot products, ~1e-6 at logits of order 1; the gap asked for leaves ten times that on
    either side."""
    from instance_nerf_amd import extract
    pts = extract.lattice(BOX_MIN, BOX_MAX, RES, DEV).clamp(-1.0, 1.0)
    with torch.no_grad():
        logit = np.sort(np.log(np.maximum(net.density(pts)["sigma"].double().cpu().numpy(), 1e-30)))
    mid = len(logit) // 2
    gaps = logit[mid - 1500:mid + 1500]
    k = int(np.argmax(np.diff(gaps)))
    assert gaps[k + 1] - gaps[k] > 2e-5
    return float(np.exp(0.5 * (gaps[k] + gaps[k + 1])))


def _reference_of_lattices(lat, **kw):
    axes = [a.cpu().numpy() for a in lat["axes"]]
    labels = None if lat["labels"] is None else lat["labels"].cpu().numpy()
    rgb = None if lat["rgb"] is None else lat["rgb"].cpu().numpy()
    return mr.marching_tetrahedra(lat["field"].cpu().numpy(), lat["iso"], kw.pop("clamp"), axes, labels=labels, rgb=rgb,
                                  ext=lat["ext"], **kw)


def test_extract_mesh_equals_the_restatement_on_the_returned_lattices():
    from instance_nerf_amd import extract
    K = 16
    net = _net(_params(K, seed=3), K)
    thresh = _quiet_threshold(net)
    # scene mesh with face labels and colours: instance_lattice gives the logit and the labels, forward_lattice the rgb
    lat = extract.mesh_lattices(net, BOX_MIN, BOX_MAX, res=RES, threshold=thresh, labels=True, colors=True)
    assert lat["labels"] is not None and lat["rgb"] is not None and abs(lat["iso"] - np.log(thresh)) < 1e-6
    got = extract.extract_mesh(net, BOX_MIN, BOX_MAX, res=RES, threshold=thresh)
    ref = _reference_of_lattices(lat, clamp=extract.MESH_CLAMP, cap=True, want_face_labels=True)
    got = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    assert len(ref["faces"]) > 1000 and got["face_labels"] is not None and got["colors"] is not None
    _assert_same(got, ref, "scene")
    assert mr.is_closed(got["faces"])
    # one instance, closed on its own
    k = int(np.bincount(lat["labels"].cpu().numpy().reshape(-1), minlength=256)[:K].argmax())
    one = extract.extract_mesh(net, BOX_MIN, BOX_MAX, res=RES, threshold=thresh, instance=k, colors=False)
    ref1 = _reference_of_lattices(dict(lat, rgb=None), clamp=extract.MESH_CLAMP, cap=True, select=k, want_face_labels=False)
    one = {k_: (v.cpu().numpy() if torch.is_tensor(v) else v) for k_, v in one.items()}
    assert one["face_labels"] is None and one["colors"] is None and len(ref1["faces"]) > 0
    _assert_same(one, ref1, "instance")
    assert mr.is_closed(one["faces"])
    # without labels the field is channel 3 of forward_lattice's tensor, read in place
    lat2 = extract.mesh_lattices(net, BOX_MIN, BOX_MAX, res=RES, threshold=thresh, labels=False, colors=True)
    assert lat2["labels"] is None and lat2["field"].stride(2) == 4
    plain = extract.extract_mesh(net, BOX_MIN, BOX_MAX, res=RES, threshold=thresh, face_labels=False, cap=False, clamp=0.5)
    ref2 = _reference_of_lattices(lat2, clamp=0.5, cap=False)
    plain = {k_: (v.cpu().numpy() if torch.is_tensor(v) else v) for k_, v in plain.items()}
    _assert_same(plain, ref2, "plain")


def test_fused_and_composable_paths_give_the_same_faces():
    from instance_nerf_amd import extract
    K = 16
    net = _net(_params(K, seed=3), K)
    thresh = _quiet_threshold(net)
    for kw in (dict(face_labels=False), dict(face_labels=False, colors=False, cap=False)):
        a = extract.extract_mesh(net, BOX_MIN, BOX_MAX, res=RES, threshold=thresh, **kw)
        b = extract.extract_mesh(net, BOX_MIN, BOX_MAX, res=RES, threshold=thresh, fused=False, **kw)
        assert a["faces"].shape[0] > 1000 and torch.equal(a["faces"], b["faces"])
        assert (a["vertices"] - b["vertices"]).abs().max() < 1e-3
        if a["colors"] is not None:
            assert (a["colors"] - b["colors"]).abs().max() < 1e-3


def test_composable_lattices_with_labels_and_colours():
    """``labels=True`` with ``fused=False``: labels, field and colours of one sweep, against ``extract_instances`` and the
    model's own ``density()`` / ``color()`` on the clamped lattice."""
    from instance_nerf_amd import extract
    K = 16
    net = _net(_params(K, seed=3), K)
    thresh = _quiet_threshold(net)
    lat = extract.mesh_lattices(net, BOX_MIN, BOX_MAX, res=RES, threshold=thresh, labels=True, colors=True, fused=False)
    ref = extract.extract_instances(net, BOX_MIN, BOX_MAX, res=RES, sigma_thresh=thresh, fused=False)
    assert lat["labels"].dtype == torch.uint8 and torch.equal(lat["labels"], ref["labels"])
    pts = extract.lattice(BOX_MIN, BOX_MAX, RES, DEV).clamp(-1.0, 1.0)
    with torch.no_grad():
        den = net.density(pts)
        dirs = torch.from_numpy(extract.VIEW_DIRS).to(DEV)
        rgb = sum(net.color(pts, dirs[v].expand(pts.shape[0], 3).contiguous(), geo_feat=den["geo_feat"]) for v in range(4)) / 4
    assert torch.equal(lat["field"], torch.log(den["sigma"].clamp_min(1e-30)).view(*RES.tolist()))
    assert (lat["rgb"][..., :3] - rgb.view(*RES.tolist(), 3)).abs().max() <= 1e-6
    k = int(torch.bincount(ref["labels"].reshape(-1).long(), minlength=256)[:K].argmax())
    one = extract.extract_mesh(net, BOX_MIN, BOX_MAX, res=RES, threshold=thresh, instance=k, fused=False)
    assert one["faces"].shape[0] >= 1 and mr.is_closed(one["faces"].cpu().numpy())


def test_threshold_above_every_sigma_gives_an_empty_mesh_and_a_valid_ply(tmp_path):
    from instance_nerf_amd import extract, mesh_io
    net = _net(_params(16, seed=3), 16)
    m = extract.extract_mesh(net, BOX_MIN, BOX_MAX, res=RES, threshold=1e30)
    assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3) and m["face_labels"].shape == (0,)
    back = mesh_io.read_ply(mesh_io.write_ply(str(tmp_path / "empty.ply"), m["vertices"], m["faces"], m["colors"], m["face_labels"]))
    assert back["vertices"].shape == (0, 3) and back["faces"].shape == (0, 3)


# ---------------------------------------------------------------------------------------------- trained room
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The synthetic room of tests/test_instance_extract.py (12 boxes, K = 16), trained briefly through ``Trainer``."""
    from instance_nerf_amd.nerf import NeRFNetwork
    from instance_nerf_amd.nerf.provider import NeRFDataset
    from instance_nerf_amd.nerf.utils import Trainer
    from instance_nerf_amd.scene import RoomScene
    K = 16
    root = tmp_path_factory.mktemp("room_mesh")
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
    return {"net": net, "trainer": ti, "root": root, "K": K}


def _label_agreement(vertices, faces, face_labels, labels, res):
    """Area-weighted share of the faces whose label equals the label of the occupied voxel nearest to the face's centroid."""
    v = vertices.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    areas = np.linalg.norm(np.cross(b - a, c - a), axis=1) / 2.0
    cen = (a + b + c) / 3.0
    occ = np.argwhere(labels != 255)
    centres = (occ + 0.5) / np.asarray(res, np.float64) * 2.0 - 1.0
    lab = labels[labels != 255]
    near = np.empty(len(cen), np.int64)
    for s in range(0, len(cen), 256):
        d = ((cen[s:s + 256, None, :] - centres[None, :, :]) ** 2).sum(-1)
        near[s:s + 256] = d.argmin(1)
    return float((areas * (lab[near] == face_labels)).sum() / areas.sum())


def test_trainer_writes_closed_scene_and_instance_meshes(trained):
    from instance_nerf_amd import extract, mesh_io
    ti, net, K = trained["trainer"], trained["net"], trained["K"]
    R = 40
    net.train()
    path = ti.save_mesh(resolution=R)
    assert path == os.path.join(str(trained["root"] / "ws"), "meshes", f"room_{ti.epoch}.ply") and os.path.exists(path)
    assert net.training
    net.eval()
    scene = mesh_io.read_ply(path)
    assert len(scene["faces"]) > 1000 and mr.is_closed(scene["faces"])
    assert scene["colors"] is not None and scene["face_labels"] is not None
    assert mr.signed_volume(scene["vertices"], scene["faces"]) > 0

    written = ti.save_instance_meshes(resolution=R)
    again = mesh_io.read_ply(written["scene"])
    for key in ("vertices", "faces", "colors", "face_labels"):
        assert np.array_equal(again[key], scene[key]), key
    counts = extract.extract_instances(net, max_side=R, sigma_thresh=10.0)["counts"].cpu().numpy()
    lat = extract.mesh_lattices(net, resolution=R, threshold=10, labels=True, colors=False)
    for k in range(1, K):
        if counts[k] == 0:
            assert k not in written["instances"]
            continue
        # a channel whose every voxel fails field >= iso at the threshold's rounding would have no surface; the
        # restatement decides whether a mesh is due
        ref = _reference_of_lattices(lat, clamp=extract.MESH_CLAMP, cap=True, select=k, want_face_labels=False)
        if len(ref["faces"]) == 0:
            assert k not in written["instances"]
            continue
        p = written["instances"][k]
        assert p.endswith(f"room_{ti.epoch}_instance_{k}.ply")
        m = mesh_io.read_ply(p)
        assert len(m["faces"]) > 0 and mr.is_closed(m["faces"]), k
        assert np.array_equal(m["faces"], ref["faces"]) and np.array_equal(_bits(m["vertices"]), _bits(ref["vertices"])), k
    assert len(written["instances"]) >= 4

    # face labels against the label volume: the kernels' share equals the restatement's (labels are integers)
    labels = lat["labels"].cpu().numpy()
    ref = _reference_of_lattices(lat, clamp=extract.MESH_CLAMP, cap=True, want_face_labels=True)
    assert np.array_equal(ref["faces"], scene["faces"]) and np.array_equal(ref["face_labels"], scene["face_labels"])
    share = _label_agreement(scene["vertices"], scene["faces"], scene["face_labels"], labels, lat["res"])
    share_ref = _label_agreement(ref["vertices"], ref["faces"], ref["face_labels"], labels, lat["res"])
    print(f"trained room at {R}^3: V {len(scene['vertices'])}, F {len(scene['faces'])}, {len(written['instances'])} instance "
          f"meshes, area-weighted face-label agreement with the nearest occupied voxel {share:.4f} (restatement {share_ref:.4f})")
    assert share == share_ref
