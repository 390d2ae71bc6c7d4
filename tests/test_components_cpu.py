"""Connected components of a label volume, CPU side: the composable (plain torch) path of extract.label_components /
filter_components against the scipy restatement in tests/components_reference.py - exact integers - plus the keep rule,
floater recovery on the analytic room, and the argument validation of the new exports (child process, no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe  # noqa: E402
import components_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SHAPES = [(1, 1, 97), (37, 5, 129), (64, 64, 64)]


def check_volume(vol, K, connectivity, device="cpu", fused=True, **rule):
    """label_components and filter_components on `vol` against the reference, every output, exactly."""
    from instance_nerf_amd import extract
    rng = np.random.default_rng(7)
    conf = rng.random(vol.shape).astype(np.float32)
    want = ref.reference_filter(vol, conf, K, connectivity, **rule)
    t = torch.from_numpy(vol).to(device)
    roots = extract.label_components(t, connectivity, fused=fused)
    assert roots.dtype == torch.int32 and tuple(roots.shape) == vol.shape
    assert np.array_equal(roots.cpu().numpy(), want["roots"])
    got = extract.filter_components(t, torch.from_numpy(conf).to(device), K=K, connectivity=connectivity, fused=fused, **rule)
    for key in ("labels", "roots", "n_components", "kept_voxels", "kept_root", "confidence"):
        assert np.array_equal(got[key].cpu().numpy(), want[key]), key
    assert got["labels"].dtype == torch.uint8 and got["n_components"].dtype == torch.int32
    return got, want


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("K", [1, 3, 16])
def test_random_volumes_match_the_reference(shape, K, connectivity):
    for i, occupancy in enumerate((0.1, 0.3, 0.5, 0.9)):
        vol = ref.random_volume(shape, K, occupancy, seed=100 * K + i)
        check_volume(vol, K, connectivity, keep="largest", skip_background=False)
    check_volume(ref.blob_volume(shape, K, seed=K), K, connectivity, keep="all", min_voxels=30, skip_background=True)


def test_checkerboard_is_all_singletons_at_6_and_one_component_at_26():
    vol = ref.checkerboard((16, 12, 70))
    n = int((vol != ref.EMPTY).sum())
    got, _ = check_volume(vol, 2, 6, keep="all")
    assert int(got["n_components"][1]) == n
    assert np.array_equal(got["roots"].numpy().reshape(-1)[vol.reshape(-1) != ref.EMPTY], np.nonzero(vol.reshape(-1) != ref.EMPTY)[0])
    got, _ = check_volume(vol, 2, 26, keep="all")
    assert int(got["n_components"][1]) == 1 and int(got["kept_voxels"][1]) == n


@pytest.mark.parametrize("shape", [(9, 9, 70), (32, 32, 32)])
def test_serpentine_is_one_component(shape):
    vol = ref.serpentine(shape)
    for connectivity in (6, 26):
        got, _ = check_volume(vol, 2, connectivity, keep="largest")
        assert int(got["n_components"][1]) == 1 and int(got["kept_root"][1]) == 0
        assert int(got["kept_voxels"][1]) == int((vol == 1).sum())


def test_empty_and_uniform_volumes():
    empty = np.full((7, 9, 66), ref.EMPTY, np.uint8)
    got, _ = check_volume(empty, 4, 6, keep="largest", skip_background=False)
    assert int(got["roots"].max()) == -1 and int(got["n_components"].sum()) == 0 and got["kept_root"].tolist() == [-1] * 4
    full = np.full((7, 9, 66), 2, np.uint8)
    for connectivity in (6, 26):
        got, _ = check_volume(full, 4, connectivity, keep="largest")
        assert int(got["roots"].max()) == 0 and got["n_components"].tolist() == [0, 0, 1, 0]
        assert got["kept_voxels"].tolist() == [0, 0, full.size, 0]


def test_diagonal_sheets():
    vol = ref.diagonal_sheets((20, 17, 70), K=4)
    got, _ = check_volume(vol, 4, 26, keep="all", skip_background=False)
    assert int(got["n_components"].sum()) == len(np.unique((np.indices(vol.shape).sum(0))[vol != ref.EMPTY]))
    got, _ = check_volume(vol, 4, 6, keep="all", skip_background=False)
    assert int(got["n_components"].sum()) == int((vol != ref.EMPTY).sum())


# ---- the keep rule ---------------------------------------------------------------------------------------------------
def keep_volume():
    """Label 1: two components of 6 voxels (roots 10*... low and high) and one of 3; label 0: two components; label 9 (>= K)."""
    vol = np.full((6, 8, 20), ref.EMPTY, np.uint8)
    vol[0, 0, 2:8] = 1           # 6 voxels, the lower root
    vol[3, 3, 0:6] = 1           # 6 voxels
    vol[5, 7, 10:13] = 1         # 3 voxels
    vol[1, 5, 0:4] = 0           # background, 4
    vol[4, 0, 0:2] = 0           # background, 2
    vol[2, 2, 5:9] = 9           # a label >= K
    vol[5, 0, 0:5] = 2           # 5 voxels
    return vol


def test_ties_go_to_the_lowest_root():
    vol = keep_volume()
    got, _ = check_volume(vol, 4, 6, keep="largest")
    assert int(got["kept_root"][1]) == 2 and int(got["kept_voxels"][1]) == 6 and int(got["n_components"][1]) == 3
    out = got["labels"].numpy()
    assert (out[0, 0, 2:8] == 1).all() and (out[3, 3, 0:6] == ref.EMPTY).all() and (out[5, 7, 10:13] == ref.EMPTY).all()
    conf = got["confidence"].numpy()
    assert (conf[3, 3, 0:6] == 0).all() and (conf[0, 0, 2:8] > 0).all()


def test_min_voxels_boundary():
    vol = keep_volume()
    got, _ = check_volume(vol, 4, 6, keep="all", min_voxels=6)
    assert got["kept_voxels"].tolist() == [0, 12, 0, 0] and got["kept_root"].tolist() == [-1] * 4
    got, _ = check_volume(vol, 4, 6, keep="all", min_voxels=7)
    assert got["kept_voxels"].tolist() == [0, 0, 0, 0]
    got, _ = check_volume(vol, 4, 6, keep="largest", min_voxels=5)
    assert got["kept_root"].tolist() == [-1, 2, int(np.ravel_multi_index((5, 0, 0), vol.shape)), -1]
    got, _ = check_volume(vol, 4, 6, keep="largest", min_voxels=6)
    assert got["kept_root"].tolist() == [-1, 2, -1, -1] and (got["labels"].numpy() != 2).all()


def test_skip_background_and_labels_above_K_pass_through():
    vol = keep_volume()
    got, _ = check_volume(vol, 4, 6, keep="largest", skip_background=True)
    out = got["labels"].numpy()
    assert np.array_equal(out == 0, vol == 0) and int(got["n_components"][0]) == 0       # channel 0 left alone
    assert np.array_equal(out == 9, vol == 9)
    got, _ = check_volume(vol, 4, 6, keep="largest", skip_background=False)
    out = got["labels"].numpy()
    assert (out[1, 5, 0:4] == 0).all() and (out[4, 0, 0:2] == ref.EMPTY).all() and int(got["n_components"][0]) == 2
    assert np.array_equal(out == 9, vol == 9)


def test_argument_errors():
    from instance_nerf_amd import extract
    vol = torch.zeros(4, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="connectivity"):
        extract.label_components(vol, 18)
    with pytest.raises(ValueError, match="uint8"):
        extract.label_components(vol.int())
    with pytest.raises(ValueError, match="K must"):
        extract.filter_components(vol, K=256)
    with pytest.raises(ValueError, match="keep"):
        extract.filter_components(vol, K=4, keep="biggest")
    with pytest.raises(ValueError, match="min_voxels"):
        extract.filter_components(vol, K=4, min_voxels=0)


def test_product_does_not_import_scipy():
    import re
    for dp, _, fs in os.walk(os.path.join(ROOT, "instance_nerf_amd")):
        for f in fs:
            if f.endswith(".py"):
                assert not re.search(r"^\s*(from|import)\s+scipy\b", open(os.path.join(dp, f)).read(), flags=re.M), f


# ---- floater recovery on the analytic room ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room():
    clean = ref.room_volume(160)
    return clean, ref.add_floaters(clean, 13, n_blobs=300, seed=3)


def test_the_analytic_room_has_one_component_per_id(room):
    clean, _ = room
    counts, _ = ref.voxel_stats(clean, 13)
    assert counts[1:].max() == 31464 and counts[1:].min() == 3234
    for connectivity in (6, 26):
        roots = ref.reference_roots(clean, connectivity)
        for k in range(1, 13):
            assert np.unique(roots[clean == k]).size == 1, (k, connectivity)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_floater_recovery(room, connectivity):
    from instance_nerf_amd import extract
    clean, noisy = room
    K = 13
    counts, boxes = ref.voxel_stats(clean, K)
    raw_counts, raw_boxes = ref.voxel_stats(noisy, K)
    assert (raw_boxes[1:] != boxes[1:]).any(1).all() and (raw_counts[1:] > counts[1:]).all()      # the input is guarded
    t = torch.from_numpy(noisy)
    conf = torch.ones(noisy.shape, dtype=torch.float32)
    got = extract.filter_components(t, conf, K=K, connectivity=connectivity, keep="largest")
    c, b, s = extract.volume_stats(got["labels"], got["confidence"], K)
    assert np.array_equal(c.numpy()[1:], counts[1:]) and np.array_equal(b.numpy()[1:], boxes[1:])
    assert np.array_equal(got["labels"].numpy(), clean)
    assert np.array_equal(got["kept_voxels"].numpy()[1:], counts[1:]) and (got["n_components"].numpy()[1:] > 1).all()
    assert np.array_equal(s.numpy()[1:], counts[1:].astype(np.float32))


# ---- ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def abi():
    return abi_probe.run_abi_child("components_abi_child.py", env=abi_probe.NO_GPU)


@pytest.mark.parametrize("case,needle", [
    ("inr_components_label:connectivity_0", "connectivity"), ("inr_components_label:connectivity_4", "connectivity"),
    ("inr_components_label:connectivity_8", "connectivity"), ("inr_components_label:connectivity_18", "connectivity"),
    ("inr_components_label:connectivity_27", "connectivity"), ("inr_components_label:too_many_tiles", "tiles"),
    ("inr_components_filter:K_256", "K"), ("inr_components_filter:K_0", "K"),
    ("inr_components_filter:first_channel_negative", "first_channel"),
    ("inr_components_filter:first_channel_above_K", "first_channel"),
    ("inr_components_filter:min_voxels_0", "min_voxels"), ("inr_components_filter:keep_largest_2", "keep_largest"),
    ("inr_components_filter:confidence_out_without_confidence", "confidence"),
    ("inr_components_filter:n_components_misaligned", "misaligned"), ("inr_components_filter:labels_out_null", "null"),
] + [(f"{name}:{case}", needle) for name in ("inr_components_label", "inr_components_filter") for case, needle in (
    ("workspace_too_small", "workspace"), ("workspace_misaligned", "misaligned"), ("roots_misaligned", "misaligned"),
    ("volume_2_31", "2^31"), ("volume_2_33", "2^31"), ("size_zero", "size"))])
def test_exports_reject_one_bad_argument(abi, case, needle):
    rc, msg = abi[case]
    assert rc == EINVAL and needle in msg, (case, rc, msg)


def test_workspace_size_query(abi):
    for case in ("negative", "zero", "volume_2_31", "volume_2_33", "int32_product_wraps"):
        rc, msg = abi[f"inr_components_workspace_bytes:{case}"]
        assert rc == EINVAL and msg, case
    assert abi["inr_components_workspace_bytes:ok"][0] >= 4 * 256 ** 3
    assert abi["inr_components_workspace_bytes:largest"][0] >= 4 * 2047 * 1024 * 1024


def test_abi_version_is_13():
    from instance_nerf_amd import _lib
    assert _lib.ABI_VERSION == 13 and _lib.load().inr_abi_version() == 13
