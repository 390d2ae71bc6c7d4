"""2-D mask matching, CPU side: ``convert_segments`` and the composable path of ``masks.match_masks`` against the golden
fixture of the reference's own ``match_seg()`` run and against the oracle's restatement - exact integers -, the order, tie
and threshold rules, ``match_seg_dir`` as the script's drop-in, and the argument validation of the three new exports
(child process, no GPU)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe  # noqa: E402
import match_cases as mc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def run(seg, proj, ids=None, **kw):
    from instance_nerf_amd.masks import match_masks
    out = match_masks(seg, proj, ids, fused=False, **kw)
    assert torch.is_tensor(out) and out.dtype == torch.int32
    return out.numpy()


# ---- the reference's own run -------------------------------------------------------------------------------------------
def test_golden_fixture_through_convert_and_match():
    from instance_nerf_amd.masks import convert_segments, select_projections
    z, rows, names = mc.golden_cases()
    files = [str(f) for f in z["proj_files"]]
    for img, pan, info, proj, ids, want in rows:
        assert select_projections(files, img)[1] == ids                    # the file rule, prefix quirk included
        seg = convert_segments(pan, info, names)
        assert seg.dtype == np.int32
        got = run(seg, proj, ids, ordered=True)
        assert got.dtype == want.dtype == np.int32 and got.shape == want.shape
        assert np.array_equal(got, want), img
        assert np.array_equal(run(torch.from_numpy(seg), torch.from_numpy(proj), ids), want), img      # tensors, name order
    assert select_projections(files, "0001")[0][0] == "00010_9.png" and select_projections(files, "0010") == ([], [])


def test_match_seg_dir_writes_the_references_files(tmp_path):
    from instance_nerf_amd.masks import load_matched_masks, match_seg_dir, save_png_gray
    z, rows, names = mc.golden_cases()
    for d in ("proj", "seg"):
        os.makedirs(tmp_path / d)
    for f in (str(f) for f in z["proj_files"]):
        save_png_gray(str(tmp_path / "proj" / f), z["proj_" + f[:-4]].astype(np.uint8) * 255)
    for img, pan, info, _, _, _ in rows:
        np.save(tmp_path / "seg" / f"{img}.npy", pan)
        json.dump(info, open(tmp_path / "seg" / f"{img}.json", "w"))
    json.dump(names, open(tmp_path / "coco_id_to_name.json", "w"))
    done = match_seg_dir(str(tmp_path / "proj"), str(tmp_path / "seg"), str(tmp_path / "out"),
                         str(tmp_path / "coco_id_to_name.json"), device="cpu")
    assert done == [r[0] for r in rows]
    assert sorted(os.listdir(tmp_path / "out")) == [f"{r[0]}.npy" for r in rows]
    for img, _, _, _, _, want in rows:
        got = np.load(tmp_path / "out" / f"{img}.npy")
        assert got.dtype == np.int32 and np.array_equal(got, want), img
    back = load_matched_masks(str(tmp_path / "out"))
    assert all(np.array_equal(back[r[0]], r[5]) for r in rows)


# ---- order, ties, threshold --------------------------------------------------------------------------------------------
def test_name_order_decides_ties():
    from instance_nerf_amd.masks import candidate_order
    assert candidate_order([3, 12, 1]) == [2, 1, 0]                       # "1.png" < "12.png" < "3.png"
    seg = np.zeros((6, 8), np.int32)
    seg[1:4, 2:6] = 9
    m = seg == 9
    assert (run(seg, np.stack([m, m]), [12, 3])[m] == 12).all()            # given order 12, 3 = name order
    assert (run(seg, np.stack([m, m]), [3, 12])[m] == 12).all()            # given order 3, 12: name order still wins
    assert (run(seg, np.stack([m, m]), [3, 12], ordered=True)[m] == 3).all()
    got = run(seg, np.stack([m, m]), [12, 3])
    assert np.array_equal(got, mc.expected(seg[None], np.stack([m, m])[None], [12, 3])[0])


@pytest.mark.parametrize("extra,want", [(0, -1), (1, 12)])
def test_threshold_is_a_strict_fp64_comparison(extra, want):
    """ids (1, 12) are scored in the order 1, 12; candidate 1 is empty.  A segment whose best candidate has
    20 * inter == union sits exactly at 0.05 and is NOT matched (numpy: 2 / 40 > 0.05 is False); with
    20 * inter == union + 1 it is."""
    H, W = 10, 40
    seg = np.zeros((H, W), np.int32)
    m1, m12 = np.zeros((H, W), bool), np.zeros((H, W), bool)
    # from the counts: segment area a, mask area b, union = a + b - inter
    inter = 2 + extra
    union = 20 * inter - extra                    # extra = 0: 20 * inter == union; extra = 1: 20 * inter == union + 1
    a = 25
    b = union - a + inter
    seg.reshape(-1)[:a] = 5
    m12.reshape(-1)[a - inter:a - inter + b] = True
    assert (np.sum((seg == 5) & m12), np.sum((seg == 5) | m12)) == (inter, union) and 20 * inter == union + extra
    got = run(seg, np.stack([m1, m12]), [1, 12])
    assert (got[seg == 5] == want).all() and (got[seg == 0] == 0).all()
    assert np.array_equal(got, mc.expected(seg[None], np.stack([m1, m12])[None], [1, 12])[0])


def test_edge_cases():
    rng = np.random.default_rng(3)
    seg = rng.integers(-1, 4, size=(2, 9, 11)).astype(np.int32)
    got = run(seg, np.zeros((2, 0, 9, 11), bool))                           # k = 0: every segment becomes -1
    assert np.array_equal(got, np.where(seg > 0, -1, seg))
    flat = np.where(rng.random((1, 9, 11)) < 0.5, -1, 0).astype(np.int32)   # no segment > 0
    assert np.array_equal(run(flat, rng.random((1, 5, 9, 11)) > 0.5), flat)
    big = np.zeros((9, 11), np.int32)                                       # ids that only ranking makes small
    big[:4] = 10 ** 6
    big[5:, :5] = 70000
    proj = np.stack([big == 10 ** 6, big == 70000, np.ones_like(big, bool)])
    got = run(big, proj, [4, 2, 9])
    assert got.shape == (9, 11) and (got[big == 10 ** 6] == 4).all() and (got[big == 70000] == 2).all()
    assert np.array_equal(got, mc.expected(big[None], proj[None], [4, 2, 9])[0])
    with pytest.raises(ValueError, match="iou_thresh"):
        run(big, proj, iou_thresh=1.5)
    with pytest.raises(ValueError, match="-1"):
        run(np.full((2, 2), -2, np.int32), np.zeros((1, 2, 2), bool))


@pytest.mark.parametrize("name", [f[0] for f in mc.FUZZ] + mc.LAYOUTS)
def test_composable_path_equals_the_oracle(name):
    seg, proj, ids, want = mc.case(name)
    assert np.array_equal(run(seg, proj, ids), want)


def test_packed_words_round_trip_and_match():
    from instance_nerf_amd.masks import candidate_order, pack_mask_bits
    seg, proj, ids, want = mc.case("61x67_k33")
    order = candidate_order(ids)
    words = pack_mask_bits(proj[:, order])
    assert words.dtype == torch.int32 and tuple(words.shape) == (3, 2, 61, 67)
    bits = (words.numpy().view(np.uint32)[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :, None, None]) & 1
    assert np.array_equal(bits.reshape(3, 64, 61, 67)[:, :33].astype(bool), proj[:, order])
    assert np.array_equal(run(seg, words, [int(ids[i]) for i in order]), want)
    with pytest.raises(ValueError, match="candidate order"):
        run(seg, pack_mask_bits(proj), np.arange(1, 34))                   # 1, 2, ..: "10.png" sorts before "2.png"


# ---- the projector's view loop -----------------------------------------------------------------------------------------
def test_view_loop_restores_the_model_mode_when_its_consumer_raises(monkeypatch, tmp_path):
    """``project_3d_masks`` consumes the view loop; a failure while it writes a view's PNGs must not leave the model in
    eval mode.  The projector itself is stubbed (it needs a GPU): every pixel of every view is inside the one mask."""
    from instance_nerf_amd import masks as pm
    H = W = 2
    modes = []

    def rays(*a, **k):
        return {"rays_o": [None], "rays_d": [None], "inds": [torch.arange(H * W)]}

    def project(model, *a, **k):
        modes.append(model.training)
        return torch.ones(H * W, 1), None

    def fail(*a, **k):
        raise OSError("disk full")
    monkeypatch.setattr(pm, "get_rays", rays)
    monkeypatch.setattr(pm, "soft_project", project)
    model = torch.nn.Linear(1, 1).train()
    out = pm.project_3d_masks(model, None, None, None, torch.zeros(2, 4, 4), None, H, W, packed=(1, None))
    assert out.all() and modes == [False, False] and model.training
    monkeypatch.setattr(pm, "save_png_gray", fail)
    with pytest.raises(OSError, match="disk full") as err:
        pm.project_3d_masks(model, None, None, None, torch.zeros(2, 4, 4), None, H, W, proj_dir=str(tmp_path), packed=(1, None))
    assert model.training and modes == [False] * 3, err


# ---- convert_segments --------------------------------------------------------------------------------------------------
def test_convert_segments():
    from instance_nerf_amd.masks import BACKGROUND_STUFF, convert_segments
    from oracle import consumers
    assert BACKGROUND_STUFF == {n for n, v in consumers.COCO_STUFF_TO_NYU40.items() if v == 40}
    pan = np.asarray([[0, 1, 2, 3], [4, 5, 6, 6]], np.int64)
    info = [{"id": 1, "isthing": True, "name": "chair"}, {"id": 2, "isthing": False, "name": "wall-brick"},
            {"id": 3, "isthing": False, "name": "no-such-stuff"}, {"id": 4, "isthing": True, "name": "curtain"},
            {"id": 5, "isthing": False, "category_id": 1}]
    names = {"thing_classes": ["person"], "stuff_classes": ["banner", "stairs"]}
    out = convert_segments(pan, info, names)
    # unlabeled -1; thing kept; background stuff 0; unknown stuff keeps its id; a THING named like background stuff is kept;
    # category_id looked up (stairs: background); id 6 is missing from the info: 0
    assert out.dtype == np.int32 and out.tolist() == [[-1, 1, 0, 3], [4, 0, 0, 0]]
    named = [dict(s, name=names["stuff_classes"][s["category_id"]]) if "name" not in s else s for s in info]
    assert np.array_equal(out, consumers.convert_seg(pan, named))
    with pytest.raises(ValueError, match="negative"):
        convert_segments(np.asarray([[0, -1]]), [])
    with pytest.raises(ValueError, match="class_names"):
        convert_segments(pan, [{"id": 1, "isthing": True, "category_id": 0}])


# ---- ABI ---------------------------------------------------------------------------------------------------------------
NEW = ("inr_pack_mask_bits", "inr_match_count", "inr_match_assign")


def test_exports_are_registered():
    from instance_nerf_amd import _lib, build
    assert all(n in _lib.EXPORTS for n in NEW) and "match.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 13                       # additive: no bump


@pytest.fixture(scope="module")
def abi():
    return abi_probe.run_abi_child("match_abi_child.py", env=abi_probe.NO_GPU)


@pytest.mark.parametrize("case,needle", [(f"{name}:{case}", needle) for name in NEW[1:] for case, needle in (
    ("S_1024", "S must"), ("S_negative", "S must"), ("k_1025", "k must"), ("k_negative", "k must"), ("BP_2_31", "B * P"),
    ("BP_2_40", "B * P"), ("BP_wraps_int64", "B * P"), ("B_zero", "size"), ("P_zero", "size"), ("seg_null", "null"),
    ("inter_null", "null"), ("seg_area_misaligned", "misaligned"))] + [
    ("inr_match_count:status_null", "null"), ("inr_match_assign:iou_thresh_negative", "iou_thresh"),
    ("inr_match_assign:iou_thresh_1.5", "iou_thresh"), ("inr_match_assign:iou_thresh_nan", "iou_thresh"),
    ("inr_match_assign:iou_thresh_null", "null"), ("inr_match_assign:out_null", "null"),
    ("inr_pack_mask_bits:k_0", "k must"), ("inr_pack_mask_bits:k_1025", "k must"), ("inr_pack_mask_bits:N_negative", "size"),
    ("inr_pack_mask_bits:P_zero", "size"), ("inr_pack_mask_bits:words_null", "null"), ("inr_pack_mask_bits:soft_null", "null"),
    ("inr_pack_mask_bits:inds_misaligned", "misaligned")])
def test_exports_reject_one_bad_argument(abi, case, needle):
    rc, msg = abi[case]
    assert rc == EINVAL and needle in msg, (case, rc, msg)
