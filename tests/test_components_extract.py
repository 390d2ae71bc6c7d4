"""Connected components on the GPU (csrc/components.hip behind extract.label_components / filter_components): exact
equality with the scipy restatement of tests/components_reference.py on every volume of the CPU suite and on volumes
that cross many tile faces, bit-identical repeats, floater recovery, and the options of extract_instances, the masks
npz and the instance meshes on a briefly trained room."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_reference as ref  # noqa: E402
from test_components_cpu import SHAPES, check_volume, keep_volume  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("shape", SHAPES + [(13, 11, 67), (9, 17, 63), (8, 8, 64), (7, 23, 200)])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_random_volumes_match_the_reference(shape, K, connectivity):
    for i, occupancy in enumerate((0.1, 0.3, 0.5, 0.9)):
        vol = ref.random_volume(shape, K, occupancy, seed=100 * K + i)
        check_volume(vol, K, connectivity, device=DEV, keep="largest", skip_background=False)
    check_volume(ref.blob_volume(shape, K, seed=K), K, connectivity, device=DEV, keep="all", min_voxels=30)


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("side", [160, 256])
def test_large_random_volumes(side, connectivity):
    shape = (side, side, side)
    check_volume(ref.random_volume(shape, 16, 0.5, seed=side), 16, connectivity, device=DEV, keep="largest")
    if side == 160:
        check_volume(ref.blob_volume(shape, 16, seed=side, cell=7), 16, connectivity, device=DEV, keep="all", min_voxels=400)


def test_structured_volumes():
    n = lambda v: int((v != ref.EMPTY).sum())       # noqa: E731
    vol = ref.checkerboard((16, 12, 70))
    assert int(check_volume(vol, 2, 6, device=DEV, keep="all")[0]["n_components"][1]) == n(vol)
    assert int(check_volume(vol, 2, 26, device=DEV, keep="all")[0]["n_components"][1]) == 1
    for shape in ((9, 9, 70), (32, 32, 32), (128, 128, 128)):
        vol = ref.serpentine(shape)
        for connectivity in (6, 26):
            got, _ = check_volume(vol, 2, connectivity, device=DEV, keep="largest")
            assert int(got["n_components"][1]) == 1 and int(got["kept_voxels"][1]) == n(vol)
    for shape in ((20, 17, 70), (100, 90, 150)):
        vol = ref.diagonal_sheets(shape, K=4)
        check_volume(vol, 4, 26, device=DEV, keep="all", skip_background=False)
        got, _ = check_volume(vol, 4, 6, device=DEV, keep="largest", skip_background=False)
        assert int(got["n_components"].sum()) == n(vol)
    check_volume(np.full((7, 9, 66), ref.EMPTY, np.uint8), 4, 6, device=DEV, keep="largest", skip_background=False)
    for connectivity in (6, 26):
        got, _ = check_volume(np.full((17, 9, 130), 2, np.uint8), 4, connectivity, device=DEV, keep="largest")
        assert got["kept_voxels"].tolist() == [0, 0, 17 * 9 * 130, 0]


def test_keep_rule_cases():
    vol = keep_volume()
    for rule in (dict(keep="largest"), dict(keep="all", min_voxels=6), dict(keep="all", min_voxels=7),
                 dict(keep="largest", min_voxels=5), dict(keep="largest", min_voxels=6),
                 dict(keep="largest", skip_background=False), dict(keep="all", skip_background=False, min_voxels=3)):
        check_volume(vol, 4, 6, device=DEV, **rule)
        check_volume(vol, 4, 26, device=DEV, **rule)
    got, _ = check_volume(vol, 4, 6, device=DEV, keep="largest")
    assert int(got["kept_root"][1]) == 2


def test_fused_and_composable_agree_on_the_gpu():
    vol = ref.blob_volume((50, 41, 90), 8, seed=2)
    check_volume(vol, 8, 26, device=DEV, fused=False, keep="largest")


def test_two_calls_give_identical_bytes():
    from instance_nerf_amd import extract
    vol = torch.from_numpy(ref.blob_volume((160, 160, 160), 16, seed=5, cell=6)).to(DEV)
    conf = torch.rand(vol.shape, device=DEV)
    for connectivity in (6, 26):
        a = extract.filter_components(vol, conf, K=16, connectivity=connectivity)
        for _ in range(3):
            b = extract.filter_components(vol, conf, K=16, connectivity=connectivity)
            for key in a:
                assert torch.equal(a[key], b[key]), key
        sa = extract.volume_stats(a["labels"], a["confidence"], 16)
        sb = extract.volume_stats(b["labels"], b["confidence"], 16)
        assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(sa, sb))


def test_in_place_confidence():
    from instance_nerf_amd import _lib, extract
    vol = torch.from_numpy(ref.blob_volume((30, 30, 70), 6, seed=9)).to(DEV)
    conf = torch.rand(vol.shape, device=DEV)
    want = extract.filter_components(vol, conf, K=6)
    lib = _lib.load()
    W, L, H = vol.shape
    nbytes = int(lib.inr_components_workspace_bytes(W, L, H))
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    roots = torch.empty(W, L, H, dtype=torch.int32, device=DEV)
    per = torch.empty(3, 6, dtype=torch.int32, device=DEV)
    lab, c = vol.clone(), conf.clone()
    P = _lib.ptr
    _lib.check(lib.inr_components_label(P(lab), W, L, H, 6, P(ws), nbytes, P(roots), _lib.stream_ptr()))
    _lib.check(lib.inr_components_filter(P(lab), P(roots), P(c), W, L, H, 6, 1, 1, 1, P(ws), nbytes, P(lab), P(c), P(per[0]),
                                         P(per[1]), P(per[2]), _lib.stream_ptr()))
    assert torch.equal(lab, want["labels"]) and torch.equal(c, want["confidence"]) and torch.equal(per[2], want["kept_root"])


@pytest.mark.parametrize("connectivity", [6, 26])
def test_floater_recovery_through_the_kernels(connectivity):
    from instance_nerf_amd import extract
    clean = ref.room_volume(160)
    noisy = ref.add_floaters(clean, 13, n_blobs=300, seed=3)
    counts, boxes = ref.voxel_stats(clean, 13)
    _, raw_boxes = ref.voxel_stats(noisy, 13)
    assert (raw_boxes[1:] != boxes[1:]).any(1).all()
    got = extract.filter_components(torch.from_numpy(noisy).to(DEV), torch.ones(noisy.shape, device=DEV), K=13,
                                    connectivity=connectivity, keep="largest")
    c, b, _ = extract.volume_stats(got["labels"], got["confidence"], 13)
    assert np.array_equal(c.cpu().numpy()[1:], counts[1:]) and np.array_equal(b.cpu().numpy()[1:], boxes[1:])
    assert np.array_equal(got["labels"].cpu().numpy(), clean)


# ---------------------------------------------------------------------------------------------- trained room
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The synthetic room (12 boxes, K = 16), trained briefly through ``Trainer``."""
    from instance_nerf_amd.nerf import NeRFNetwork
    from instance_nerf_amd.nerf.provider import NeRFDataset
    from instance_nerf_amd.nerf.utils import Trainer
    from instance_nerf_amd.scene import RoomScene
    K = 16
    root = tmp_path_factory.mktemp("room_components")
    scene = RoomScene().write_dataset(str(root / "scene"), n_views=24, H=200, W=200, num_instances=K, ignore_frac=0.1)
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
    run(Trainer("room_nerf", None, net, stage="nerf", device=torch.device(DEV), lr=1e-2, iters=600, workspace=None,
                mute=True), ds, 600)
    ds2 = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=4096, mask_dir=scene["mask_dir"],
                      num_instances=K)
    ti = Trainer("room", None, net, stage="instance", device=torch.device(DEV), lr=1e-2, iters=600,
                 update_extra_interval=10 ** 9, workspace=str(root / "ws"), mute=True)
    ti.global_step = 1
    run(ti, ds2, 600)
    net.eval()
    return {"net": net, "trainer": ti, "root": root, "K": K}


@pytest.mark.parametrize("components,connectivity", [("largest", 6), ("largest", 26), ("all", 6)])
def test_extract_instances_fused_against_composable(trained, components, connectivity):
    from instance_nerf_amd import extract
    net, K = trained["net"], trained["K"]
    kw = dict(max_side=64, sigma_thresh=5.0, components=components, connectivity=connectivity, min_component_voxels=4)
    a = extract.extract_instances(net, **kw)
    raw = extract.extract_instances(net, max_side=64, sigma_thresh=5.0)
    # the composable rule on the SAME label volume (the two field paths differ at the threshold's rounding)
    want = ref.reference_filter(raw["labels"].cpu().numpy(), raw["confidence"].cpu().numpy(), K, connectivity, keep=components,
                                min_voxels=4, skip_background=True)
    assert np.array_equal(a["labels"].cpu().numpy(), want["labels"])
    assert np.array_equal(a["confidence"].cpu().numpy(), want["confidence"])
    assert np.array_equal(a["n_components"].cpu().numpy(), want["n_components"])
    assert torch.equal(a["raw_counts"], raw["counts"])
    counts, boxes = ref.voxel_stats(want["labels"], K)
    assert np.array_equal(a["counts"].cpu().numpy(), counts) and np.array_equal(a["boxes"].cpu().numpy(), boxes)
    assert torch.equal(a["counts"][0], raw["counts"][0])                      # the walls are left alone
    assert int((a["n_components"][1:] > 1).sum()) >= 1                         # there were floaters to drop
    # fused against fused=False, whole call.  The two FIELD paths may disagree on a voxel whose sigma sits at the
    # threshold's rounding (tests/test_instance_extract.py bounds that band); the component code is exact, so with equal
    # raw label volumes every label and integer statistic must be equal, and otherwise the composable call must equal
    # the restatement on ITS raw volume.  The number of differing raw voxels is reported either way.
    b = extract.extract_instances(net, fused=False, **kw)
    raw_b = extract.extract_instances(net, max_side=64, sigma_thresh=5.0, fused=False)
    differing = int((raw["labels"] != raw_b["labels"]).sum())
    print(f"{components}/{connectivity}: raw label volumes of the fused and composable field paths differ in {differing} voxels")
    assert differing <= 1e-3 * raw["labels"].numel(), differing
    if differing == 0:
        for key in ("labels", "counts", "boxes", "n_components", "raw_counts"):
            assert torch.equal(a[key], b[key]), key
    want_b = ref.reference_filter(raw_b["labels"].cpu().numpy(), raw_b["confidence"].cpu().numpy(), K, connectivity,
                                  keep=components, min_voxels=4, skip_background=True)
    assert np.array_equal(b["labels"].cpu().numpy(), want_b["labels"])
    assert np.array_equal(b["n_components"].cpu().numpy(), want_b["n_components"])
    counts_b, boxes_b = ref.voxel_stats(want_b["labels"], K)
    assert np.array_equal(b["counts"].cpu().numpy(), counts_b) and np.array_equal(b["boxes"].cpu().numpy(), boxes_b)
    assert torch.equal(b["raw_counts"], raw_b["counts"])
    cpu = extract.filter_components(raw["labels"].cpu(), raw["confidence"].cpu(), K=K, connectivity=connectivity, keep=components,
                                    min_voxels=4)
    gpu_torch = extract.filter_components(raw["labels"], raw["confidence"], K=K, connectivity=connectivity, keep=components,
                                          min_voxels=4, fused=False)
    for key in ("labels", "confidence", "n_components", "kept_voxels", "kept_root", "roots"):
        assert torch.equal(cpu[key], gpu_torch[key].cpu()), key
    assert torch.equal(cpu["labels"], a["labels"].cpu())


def test_components_none_is_bit_identical(trained, tmp_path):
    from instance_nerf_amd import extract
    net = trained["net"]
    a = extract.extract_instances(net, max_side=48, sigma_thresh=5.0)
    b = extract.extract_instances(net, max_side=48, sigma_thresh=5.0, components=None, connectivity=26, min_component_voxels=9)
    assert set(a) == set(b)
    for key in a:
        assert (np.array_equal(a[key], b[key]) if key == "res" else
                torch.equal(a[key].view(torch.int32) if a[key].dtype == torch.float32 else a[key],
                            b[key].view(torch.int32) if b[key].dtype == torch.float32 else b[key])), key
    m0 = extract.extract_mesh(net, resolution=40, threshold=10)
    m1 = extract.extract_mesh(net, resolution=40, threshold=10, min_component_voxels=0)
    for key in ("vertices", "faces", "colors", "face_labels"):
        assert torch.equal(m0[key].view(torch.int32) if m0[key].dtype == torch.float32 else m0[key],
                           m1[key].view(torch.int32) if m1[key].dtype == torch.float32 else m1[key]), key
    l0 = extract.mesh_lattices(net, resolution=40, threshold=10, labels=True, colors=False)
    l1 = extract.mesh_lattices(net, resolution=40, threshold=10, labels=True, colors=False, components=None)
    assert torch.equal(l0["labels"], l1["labels"]) and torch.equal(l0["field"].view(torch.int32), l1["field"].view(torch.int32))


def test_save_instance_masks_round_trip(trained):
    from instance_nerf_amd import extract, masks as pmasks
    ti, net, K = trained["trainer"], trained["net"], trained["K"]
    path = ti.save_instance_masks(name="kept", max_side=64, sigma_thresh=5.0, components="largest", connectivity=6)
    m3 = pmasks.load_3d_masks(path)
    assert m3["masks"].shape == (K - 1, 64, 64, 64)
    kept = extract.extract_instances(net, max_side=64, sigma_thresh=5.0, components="largest")
    present = 0
    for i, mask in enumerate(m3["masks"]):
        if not mask.any():
            continue
        present += 1
        roots = ref.reference_roots(np.where(mask, 1, ref.EMPTY).astype(np.uint8), 6)
        assert np.unique(roots[mask]).size == 1, i                  # each written mask is one component
    assert present >= 4
    assert int(m3["masks"].sum()) == int(kept["counts"][1:].sum())


def _face_components(faces):
    """Connected components of a triangle mesh (faces sharing a vertex), union-find on the host."""
    parent = np.arange(int(faces.max()) + 1)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in faces:
        ra, rb, rc = find(a), find(b), find(c)
        m = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = m
    return len({find(v) for v in np.unique(faces)})


def test_instance_meshes_of_the_largest_component(trained):
    from instance_nerf_amd import extract, mesh_io
    ti, net, K = trained["trainer"], trained["net"], trained["K"]
    R = 48
    ti.mesh_components, ti.mesh_connectivity = "largest", 6
    try:
        written = ti.save_instance_meshes(resolution=R)
    finally:
        ti.mesh_components = None
    assert len(written["instances"]) >= 4
    lat = extract.mesh_lattices(net, resolution=R, threshold=10, labels=True, colors=False, components="largest")
    # marching tetrahedra over the Kuhn split join lattice points along 14 directions (the 7 edge directions of
    # include/inr.h and their opposites), inside and outside alike: a mesh has one closed surface per solid piece plus one
    # per hollow it encloses (regions and the surfaces between them form a tree).  The kept label component is exactly one
    # 6-connected piece; the meshed solid is that piece minus voxels the threshold's rounding puts below iso, so the
    # surface count is derived from the meshed solid, not assumed.
    kuhn = np.zeros((3, 3, 3), bool)
    for d in ((0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)):
        kuhn[1 + d[0], 1 + d[1], 1 + d[2]] = kuhn[1 - d[0], 1 - d[1], 1 - d[2]] = True
    kuhn[1, 1, 1] = True
    from scipy import ndimage
    for k, p in written["instances"].items():
        m = mesh_io.read_ply(p)
        inside = ((lat["labels"] == k) & (lat["field"] >= lat["iso"])).cpu().numpy()
        pieces = ndimage.label(inside, structure=kuhn)[1]
        outside = np.pad(~inside, 1, constant_values=True)               # the virtual outside layer of cap=True
        hollows = ndimage.label(outside, structure=kuhn)[1] - 1
        pieces6 = np.unique(ref.reference_roots(np.where(inside, 1, ref.EMPTY).astype(np.uint8), 6)[inside]).size
        n = _face_components(m["faces"])
        print(f"instance {k}: {len(m['faces'])} faces, {n} surface component(s); solid pieces {pieces} (6-connected: {pieces6}), "
              f"enclosed hollows {hollows}")
        kept = (lat["labels"] == k).cpu().numpy()
        assert np.unique(ref.reference_roots(np.where(kept, 1, ref.EMPTY).astype(np.uint8), 6)[kept]).size == 1, k
        assert n == pieces + hollows, k


def test_scene_mesh_without_small_components(trained):
    from instance_nerf_amd import extract, mesh_io
    ti, net = trained["trainer"], trained["net"]
    raw = extract.extract_mesh(net, resolution=48, threshold=10, face_labels=False)
    kept = extract.extract_mesh(net, resolution=48, threshold=10, min_component_voxels=50)
    assert 0 < kept["faces"].shape[0] <= raw["faces"].shape[0] and kept["face_labels"] is None
    lat = extract.mesh_lattices(net, resolution=48, threshold=10, colors=False)
    solid = np.where((lat["field"] >= lat["iso"]).cpu().numpy(), 0, ref.EMPTY).astype(np.uint8)
    want = ref.reference_filter(solid, None, 1, 6, keep="all", min_voxels=50, skip_background=False)
    same = extract.mesh_from_lattice(lat["field"], lat["iso"], lat["axes"], lat["ext"],
                                     labels=torch.from_numpy(want["labels"]).to(DEV), select=0)
    assert torch.equal(same["faces"], kept["faces"]) and torch.equal(same["vertices"], kept["vertices"])
    ti.mesh_min_component_voxels = 50
    try:
        path = ti.save_mesh(save_path=str(trained["root"] / "kept.ply"), resolution=48)
    finally:
        ti.mesh_min_component_voxels = 0
    assert np.array_equal(mesh_io.read_ply(path)["faces"], kept["faces"].cpu().numpy())
