"""3-D mask metric (instance_nerf_amd/evaluate.py) on the CPU: the composable path against the reference's own run (the
golden fixture) and a brute-force count, the label-volume form, files of write_instance_masks_npz, the analytic room, and
the argument validation of the new exports."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe  # noqa: E402
import evaluate_cases as ec  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NEW = ("inr_pack_mask_planes", "inr_pack_label_planes", "inr_mask_overlap")


# ---- the reference's own run -------------------------------------------------------------------------------------------
def test_golden_fixture_composable():
    ec.check_golden("cpu", fused=False)


def test_golden_fixture_is_small_and_holds_its_corners():
    z, scenes = ec.golden()
    assert os.path.getsize(ec.GOLDEN) < 64 * 1024
    assert np.isnan(z["s0_mask_iou"]).sum() == 1                       # the pair of empty masks
    assert (z["s0_mask_iou"] == 0.5).any() and (z["s0_mask_iou"] == 0.25).any()
    assert len(scenes[1]["masks"]) == 0                                 # a scene without predictions
    assert not scenes[2]["masks"][0].any()                              # an empty prediction
    pred = set(np.concatenate([s["labels"] for s in scenes]).tolist())
    truth = set(np.concatenate([s["gt_labels"] for s in scenes]).tolist())
    assert pred - truth and truth - pred                                # classes on one side only


# ---- counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n,m,density", [((5, 7, 9), 3, 4, 0.5), ((1, 1, 1), 2, 1, 0.5), ((4, 4, 4), 5, 5, 0.05),
                                               ((3, 21, 1), 0, 3, 0.5), ((13, 11, 9), 9, 7, 0.3)])
def test_composable_counts_match_brute_force(shape, n, m, density):
    from instance_nerf_amd import evaluate as ev
    rng = np.random.default_rng(n * 16 + m)
    a, b = rng.random((n,) + shape) < density, rng.random((m,) + shape) < density
    inter, a1, a2 = ev.mask_overlap(a, torch.from_numpy(b.astype(np.uint8)), fused=False)
    ref = ec.brute_counts(a, b)
    assert inter.dtype == torch.int64 and tuple(inter.shape) == (n, m)
    for got, want in zip((inter, a1, a2), ref):
        assert np.array_equal(got.numpy(), want)
    assert ec.same_bits(ev.mask_iou_3d(a, b, fused=False).numpy(), ec.brute_iou(*ref))


def test_chunked_counts_cross_a_chunk_boundary(monkeypatch):
    from instance_nerf_amd import evaluate as ev
    monkeypatch.setattr(ev, "_CHUNK", 100)
    rng = np.random.default_rng(3)
    a, b = rng.random((4, 7, 9, 5)) < 0.5, rng.random((3, 7, 9, 5)) < 0.5
    for got, want in zip(ev.mask_overlap(a, b, fused=False), ec.brute_counts(a, b)):
        assert np.array_equal(got.numpy(), want)


def test_division_is_fp32_of_the_converted_integers():
    """16777217 / 3: the numerator is not an fp32 number, so converting first and dividing in fp32 differs from rounding
    the fp64 quotient."""
    from instance_nerf_amd import evaluate as ev
    iou = ev.iou_from_counts(torch.tensor([[16777217]]), torch.tensor([16777217]), torch.tensor([3]))
    assert iou.dtype == torch.float32
    assert float(iou) == float(np.float32(16777217) / np.float32(3))
    assert torch.isnan(ev.iou_from_counts(torch.tensor([[0]]), torch.tensor([0]), torch.tensor([0]))).all()


def test_packed_planes_round_trip_and_are_accepted():
    from instance_nerf_amd import evaluate as ev
    rng = np.random.default_rng(4)
    for V in (1, 63, 64, 65, 130):
        a = rng.random((3, V, 1, 1)) < 0.5
        planes, area, shape = ev.pack_mask_planes(a)
        assert planes.dtype == torch.int64 and tuple(planes.shape) == (3, (V + 63) // 64) and shape == (V, 1, 1)
        bits = np.unpackbits(planes.numpy().view(np.uint8), axis=1, bitorder="little")
        assert np.array_equal(bits[:, :V].astype(bool), a.reshape(3, V)) and not bits[:, V:].any()
        assert np.array_equal(area.numpy(), a.reshape(3, V).sum(1))
        b = rng.random((2, V, 1, 1)) < 0.5
        for got, want in zip(ev.mask_overlap((planes, area, shape), b, fused=False), ec.brute_counts(a, b)):
            assert np.array_equal(got.numpy(), want)


@pytest.mark.parametrize("K,first", [(1, 0), (1, 1), (16, 1), (16, 0), (64, 1)])
def test_label_volume_form_equals_the_mask_form(K, first):
    from instance_nerf_amd import evaluate as ev
    rng = np.random.default_rng(K + first)
    shape = (6, 5, 7)
    lab = rng.integers(0, K + 3, size=shape).astype(np.uint8)
    lab[rng.random(shape) < 0.3] = 255
    b = rng.random((4,) + shape) < 0.4
    planes = np.stack([lab == c for c in range(first, K)]) if K > first else np.zeros((0,) + shape, bool)
    got = ev.label_mask_overlap(lab, K, b, first_channel=first, fused=False)
    for g, w in zip(got, ev.mask_overlap(planes, b, fused=False)):
        assert torch.equal(g, w)
    iou = ev.label_mask_iou(torch.from_numpy(lab), K, b, first_channel=first, fused=False)
    assert tuple(iou.shape) == (K - first, 4) and ec.same_bits(iou.numpy(), ev.mask_iou_3d(planes, b, fused=False).numpy())
    p, area, _ = ev.pack_label_planes(lab, K, first)
    assert torch.equal(p, ev.pack_mask_planes(planes)[0]) and np.array_equal(area.numpy(), planes.reshape(K - first, lab.size).sum(1))


def test_bad_inputs_raise():
    from instance_nerf_amd import evaluate as ev
    a = np.zeros((2, 3, 3, 3), bool)
    with pytest.raises(ValueError, match="different volumes"):
        ev.mask_iou_3d(a, np.zeros((2, 3, 3, 4), bool), fused=False)
    with pytest.raises(ValueError, match="bool or uint8"):
        ev.mask_iou_3d(a.astype(np.float32), a, fused=False)
    with pytest.raises(ValueError, match="first_channel"):
        ev.label_mask_iou(np.zeros((3, 3, 3), np.uint8), 4, a, first_channel=5, fused=False)
    with pytest.raises(ValueError, match="iou_type"):
        ev.evaluate_map_recall([], [], [], [], [], iou_type="obb")
    with pytest.raises(ValueError, match=r"\[N, 6\]"):
        ev.box_iou_3d(np.zeros((2, 7), np.float32), np.zeros((2, 7), np.float32))


# ---- one scene ---------------------------------------------------------------------------------------------------------
def _room_result(res=32, drop=None):
    """An extract_instances-style result for the analytic room on a res^3 voxel-centre lattice, and the ground truth dict
    of its non-empty ids."""
    from instance_nerf_amd.scene import RoomScene
    room = RoomScene()
    ax = (np.arange(res, dtype=np.float64) + 0.5) / res * 2.0 - 1.0
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    ids = room.instance_of_points(pts).reshape(res, res, res)
    K = len(room.lo) + 1
    present = [c for c in range(1, K) if (ids == c).any()]
    gt_masks = np.stack([ids == c for c in present])
    gt_boxes = np.stack([np.concatenate([np.argwhere(m).min(0), np.argwhere(m).max(0) + 1]) for m in gt_masks]).astype(np.float32)
    gt = {"masks": gt_masks, "labels": np.ones(len(present), np.int64), "boxes": gt_boxes}
    lab = np.where(ids > 0, ids, 255).astype(np.uint8)
    if drop is not None:
        lab[lab == drop] = 255
    counts = np.bincount(lab.reshape(-1), minlength=256)[:K]
    boxes = np.full((K, 6), -1, np.int64)
    for c in range(K):
        idx = np.argwhere(lab == c)
        if len(idx):
            boxes[c] = np.concatenate([idx.min(0), idx.max(0)])
    scores = np.where(counts > 0, 1.0 - 0.01 * np.arange(K), 0.0).astype(np.float32)
    result = {"labels": torch.from_numpy(lab), "counts": torch.from_numpy(counts), "boxes": torch.from_numpy(boxes),
              "scores": torch.from_numpy(scores)}
    return result, gt, present


METRICS = ("mAP_50", "mAP_25", "AR_50", "AR_25", "box_mAP_50", "box_mAP_25", "box_AR_50", "box_AR_25")


def test_room_prediction_equal_to_truth_scores_one():
    from instance_nerf_amd import evaluate as ev
    result, gt, present = _room_result()
    out = ev.evaluate_masks(result, gt, fused=False)
    assert set(METRICS) | {"gt_best_iou", "gt_best_pred"} == set(out)
    n = len(present)
    for k in METRICS:
        # recall is n / n = 1.0 exactly; AP is the reference's fp32 sum of n recall steps k/n - (k-1)/n times precision 1,
        # each step rounded to fp32 (n = 12 gives 1 - 2^-24): 1.0 to within n half-ulps
        assert (out[k] == 1.0) if "AR" in k else (abs(out[k] - 1.0) <= n * 2.0 ** -24), (k, out[k])
    assert torch.equal(out["gt_best_iou"], torch.ones(len(present)))
    assert out["gt_best_pred"].tolist() == [c - 1 for c in present]


def test_room_one_emptied_mask_costs_one_nth_of_the_recall():
    from instance_nerf_amd import evaluate as ev
    _, gt, present = _room_result()
    n = len(present)
    assert n >= 3
    result, _, _ = _room_result(drop=present[1])
    out = ev.evaluate_masks(result, gt, fused=False)
    want = float(np.float32(n - 1) / np.float32(n))
    for k in ("AR_50", "AR_25", "box_AR_50", "box_AR_25"):
        assert out[k] == want, (k, out[k], want)
    # every kept prediction is right: precision 1 up to recall (n - 1) / n, summed in n - 1 fp32 steps of 1 / n
    assert out["mAP_50"] == out["mAP_25"] and abs(out["mAP_50"] - want) < n * 2.0 ** -24
    assert float(out["gt_best_iou"][1]) == 0.0 and (np.delete(out["gt_best_iou"].numpy(), 1) == 1.0).all()


def test_evaluate_masks_reads_files_of_write_instance_masks_npz(tmp_path):
    from instance_nerf_amd import evaluate as ev
    from instance_nerf_amd.masks import load_3d_masks, write_instance_masks_npz
    result, gt, present = _room_result(drop=3)
    rng = np.random.default_rng(0)
    for m in gt["masks"]:                                               # ragged truth: IoUs on both sides of the thresholds
        m &= rng.random(m.shape) > rng.choice([0.1, 0.4, 0.7])
    cls = np.arange(len(result["counts"]) - 1) % 2 + 1
    gt["labels"] = np.asarray([cls[c - 1] for c in present])
    path = write_instance_masks_npz(str(tmp_path / "masks" / "room.npz"), result, labels=cls, min_voxels=40)
    gt_path = str(tmp_path / "gt.npz")
    np.savez_compressed(gt_path, masks=gt["masks"], labels=gt["labels"], boxes=gt["boxes"], scores=np.ones(len(present), np.float32))
    from_file = ev.evaluate_masks(path, gt_path, fused=False)
    from_dict = ev.evaluate_masks(load_3d_masks(path), gt, fused=False)
    direct = ev.evaluate_masks(result, gt, labels=cls, min_voxels=40, fused=False)
    small = (result["counts"][1:] < 40) & (result["counts"][1:] > 0)
    assert small.any()                                                  # the min_voxels rule is exercised
    for k in METRICS:
        assert from_file[k] == from_dict[k] == direct[k], k
        assert 0.0 <= from_file[k] <= 1.0
    assert from_file["mAP_25"] >= from_file["mAP_50"] and 0.0 < from_file["AR_25"]
    assert torch.equal(from_file["gt_best_iou"], direct["gt_best_iou"])
    assert torch.equal(from_file["gt_best_pred"], direct["gt_best_pred"])
    top = ev.evaluate_masks(path, gt_path, top_k=2, fused=False)
    assert top["AR_25"] <= from_file["AR_25"]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_exports_are_registered_and_the_abi_version_is_unchanged():
    from instance_nerf_amd import _lib, build
    assert _lib.ABI_VERSION == 13
    for name in NEW:
        assert name in _lib.EXPORTS
    assert "overlap.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "inr.h")).read()
    assert "#define INR_ABI_VERSION 13" in header
    assert _lib.load().inr_abi_version() == 13


@pytest.fixture(scope="module")
def abi():
    return abi_probe.run_abi_child("overlap_abi_child.py", env=abi_probe.NO_GPU)


@pytest.mark.parametrize("case,needle", [(f"{name}:{case}", "V must") for name in NEW for case in
                                         ("V_zero", "V_negative", "V_2_31", "V_2_40")] + [
    (f"{name}:{case}", needle) for name in NEW[:2] for case, needle in
    (("planes_null", "null"), ("area_null", "null"), ("planes_misaligned", "misaligned"))] + [
    ("inr_pack_mask_planes:k_negative", "k must"), ("inr_pack_mask_planes:k_1025", "k must"),
    ("inr_pack_mask_planes:masks_null", "null"),
    ("inr_pack_label_planes:K_zero", "K must"), ("inr_pack_label_planes:K_257", "K must"),
    ("inr_pack_label_planes:first_channel_negative", "first_channel must"),
    ("inr_pack_label_planes:first_channel_above_K", "first_channel must"), ("inr_pack_label_planes:labels_null", "null"),
    ("inr_mask_overlap:kA_negative", "kA must"), ("inr_mask_overlap:kA_1025", "kA must"),
    ("inr_mask_overlap:kB_negative", "kB must"), ("inr_mask_overlap:kB_1025", "kB must"),
    ("inr_mask_overlap:run_words_100", "run_words"), ("inr_mask_overlap:run_words_negative", "run_words"),
    ("inr_mask_overlap:planes_a_null", "null"), ("inr_mask_overlap:planes_b_misaligned", "misaligned"),
    ("inr_mask_overlap:inter_null", "null")])
def test_exports_reject_one_bad_argument(abi, case, needle):
    rc, msg = abi[case]
    assert rc == EINVAL and needle in msg, (case, rc, msg)


@pytest.mark.parametrize("case", ["inr_pack_mask_planes:k_zero_null_ok", "inr_pack_label_planes:first_channel_K_null_ok",
                                  "inr_mask_overlap:kA_zero_null_ok", "inr_mask_overlap:kB_zero_null_ok"])
def test_an_empty_side_is_valid_and_launches_nothing(abi, case):
    assert abi[case][0] == 0, (case, abi[case])
