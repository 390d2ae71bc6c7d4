"""The detector tail on the CPU (instance_nerf_amd/detections.py, composable paths) against the committed record of the
reference's own run (tests/golden/detections.npz) and the numpy restatement (tests/paste_reference.py): every comparison
is an equality."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detections_cases as dc  # noqa: E402
import paste_reference as pr  # noqa: E402

from instance_nerf_amd import detections as det  # noqa: E402
from instance_nerf_amd import evaluate as ev  # noqa: E402
from instance_nerf_amd import masks as mk  # noqa: E402

NEW = ("inr_paste_masks", "inr_planes_to_voxel_words", "inr_nms_3d_pairs", "inr_nms_3d_scan")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "detections.npz"))


@pytest.fixture(scope="module")
def cases():
    return dc.paste_cases()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def recorded_bits(golden, name, N, shape):
    V = int(np.prod(shape))
    return np.unpackbits(golden[f"{name}_bits"])[:N * V].astype(bool).reshape((N,) + tuple(shape))


# ---- paste ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "mid", "big", "empty"])
def test_composable_paste_equals_the_reference_and_the_restatement(golden, cases, name):
    masks, boxes, shape = cases[name]
    want = recorded_bits(golden, name, len(masks), shape)
    restated = pr.paste_soft(masks, boxes, shape)
    assert np.array_equal(restated >= np.float32(0.5), want)
    soft = det.paste_masks(torch.from_numpy(masks), torch.from_numpy(boxes), shape, out="soft").numpy()
    assert same_bits(soft, restated)
    if name == "small":
        assert same_bits(soft, golden["small_soft"])
    got = det.paste_masks(masks, boxes, shape, out="masks")
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want)
    planes, area, shp = det.paste_masks(masks, boxes, shape, out="planes")
    assert shp == tuple(shape) and planes.dtype == torch.int64 and area.dtype == torch.int32
    assert np.array_equal(planes.numpy().view(np.uint64), pr.pack_planes(want))
    assert np.array_equal(area.numpy(), want.reshape(len(masks), int(np.prod(shape))).sum(1))


def test_the_reference_cpu_path_agrees_with_its_whole_volume_path_on_the_fixture(golden):
    """Recorded, not assumed: where they differ the project follows the whole-volume path (the fixture's ``_bits``)."""
    for name in ("small", "mid", "big", "empty"):
        assert int(golden[f"{name}_cpu_flips"]) == int(np.unpackbits(golden[f"{name}_cpu_xor"]).sum()) == 0


def test_the_half_mask_sits_on_the_threshold(cases):
    """The all-0.5 mask: every interior sample is 0.5 * (a weight sum that rounds to 1 or just below), so many voxels sit
    within an ulp of the threshold - the case that a reordered addition would flip."""
    masks, boxes, shape = cases["mid"]
    soft = pr.paste_soft(masks[7:8], boxes[7:8], shape)[0]
    assert (soft == np.float32(0.5)).sum() > 100 and ((soft < 0.5) & (soft > 0.4999)).sum() > 0


def test_dead_boxes_paste_nothing():
    m = np.ones((4, 3, 3, 3), np.float32)
    boxes = np.asarray([[1, 1, 1, 1, 4, 4], [1, 1, 1, 0.5, 4, 4], [np.nan, 0, 0, 3, 3, 3], [0, 0, 0, np.inf, 3, 3]], np.float32)
    assert not det.paste_masks(m, boxes, (5, 5, 5), out="masks").any()
    assert not pr.paste_bits(m, boxes, (5, 5, 5)).any()


def test_support_bound_of_the_skip():
    """What the kernel's skip relies on: outside the box widened by one texel on each side (rounded outward) the
    restatement is exactly zero - 200 boxes, sub-voxel and over-size ones among them."""
    shape = (13, 11, 9)
    u = dc.uniform(21, 200 * 7).reshape(200, 7)
    cut = 0
    for n in range(200):
        M = (1, 2, 3, 4, 7, 20)[n % 6]
        size = np.asarray(shape) * (0.02 if n % 5 == 0 else (3.0 if n % 5 == 1 else 0.7))
        lo = u[n, :3] * np.asarray(shape) * 1.6 - 0.4 * np.asarray(shape)
        box = np.concatenate([lo, lo + 0.05 + u[n, 3:6] * size]).astype(np.float32)
        soft = pr.paste_soft(np.ones((1, M, M, M), np.float32), box[None], shape)[0]
        lo_v, hi_v = pr.support(box, M)
        idx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
        outside = np.zeros(shape, bool)
        for a in range(3):
            outside |= (idx[a] < lo_v[a]) | (idx[a] > hi_v[a])
        assert not soft[outside].any(), (n, box, M)
        cut += int(outside.any() and soft.any())
    assert cut > 50                                                         # boxes with voxels on both sides of the bound


# ---- planes --------------------------------------------------------------------------------------------------------------
def test_planes_feed_the_mask_metric_and_the_projector_words(cases):
    masks, boxes, shape = cases["mid"]
    packed = det.paste_masks(masks, boxes, shape, out="planes")
    bits = det.paste_masks(masks, boxes, shape, out="masks")
    assert torch.equal(ev.mask_iou_3d(packed, packed, fused=False).nan_to_num(-1), ev.mask_iou_3d(bits, bits, fused=False).nan_to_num(-1))
    words = det.planes_to_voxel_words(packed)
    want = mk.pack_mask_words(bits, "cpu")
    assert len(words) == len(want) == 1 and torch.equal(words[0], want[0])
    order = mk.candidate_order(range(1, len(masks) + 1))
    assert torch.equal(det.planes_to_voxel_words(packed, order=order)[0], mk.pack_mask_words(bits[torch.as_tensor(order)], "cpu")[0])
    many = torch.from_numpy(np.repeat(bits.numpy(), 3, 0)[:33])            # 33 masks: two words, bit 31 set somewhere
    w2 = det.planes_to_voxel_words(ev.pack_mask_planes(many, fused=False))
    want2 = mk.pack_mask_words(many, "cpu")
    assert len(w2) == 2 and all(torch.equal(a, b) for a, b in zip(w2, want2)) and bool((w2[0] < 0).any())


# ---- NMS -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0.2, 0.25, 0.5])
def test_nms_equals_the_reference(golden, t):
    boxes, scores, classes = dc.nms_case()
    want = golden[f"nms_keep_{t}"]
    assert np.array_equal(pr.batched_nms(boxes, scores, classes, t), want)
    got = det.batched_nms_3d(torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(classes), t)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    one = classes == 1
    assert np.array_equal(det.nms_3d(boxes[one], scores[one], t).numpy(), pr.batched_nms(boxes[one], scores[one], classes[one], t))


def test_nms_corners(golden):
    boxes, scores, classes = dc.nms_case()
    n = len(boxes)
    k2, k25 = set(golden["nms_keep_0.2"].tolist()), set(golden["nms_keep_0.25"].tolist())
    assert {n - 6, n - 5} <= k2                       # overlap across classes only
    assert {n - 4, n - 3} <= k2                       # IoU exactly at the threshold survives
    assert len({n - 2, n - 1} & k2) == 1 and {n - 2, n - 1} <= k25
    assert pr.box_iou(boxes[n - 4], boxes[n - 3:n - 2])[0] == np.float32(0.2)
    nan = boxes[:4].copy()
    nan[1, 0] = np.nan                                # a NaN IoU suppresses (the reference keeps `iou <= t` only)
    keep = det.batched_nms_3d(nan, np.asarray([4, 3, 2, 1], np.float32), np.zeros(4, np.int64), 0.99)
    assert 1 not in keep.tolist() and np.array_equal(keep.numpy(), pr.batched_nms(nan, [4, 3, 2, 1], np.zeros(4, np.int64), 0.99))
    assert det.batched_nms_3d(np.zeros((0, 6), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), 0.2).shape == (0,)
    tie = det.nms_3d(np.asarray([[0, 0, 0, 1, 1, 1], [5, 5, 5, 6, 6, 6]], np.float32), np.asarray([0.5, 0.5], np.float32), 0.2)
    assert tie.tolist() == [0, 1]                     # equal scores: the lower index first


@pytest.mark.parametrize("tag,per", [("head", 100), ("head_top5", 5)])
def test_postprocess_detections_equals_the_reference_rule(golden, tag, per):
    hb, hs, shape = dc.head_case()
    b, s, l = det.postprocess_detections(torch.from_numpy(hb), torch.from_numpy(hs), shape, detections_per_img=per)
    assert same_bits(b.numpy(), golden[f"{tag}_boxes"]) and same_bits(s.numpy(), golden[f"{tag}_scores"])
    assert l.dtype == torch.int64 and np.array_equal(l.numpy(), golden[f"{tag}_labels"])
    assert len(b) == min(per, len(golden["head_boxes"])) and 0 < len(golden["head_boxes"]) < hb.shape[0] * 2


# ---- the file ----------------------------------------------------------------------------------------------------------------
def test_write_detections_npz_round_trip(golden, cases, tmp_path):
    masks, boxes, shape = cases["mid"]
    N = len(masks)
    scores = ((np.argsort(np.argsort(dc.uniform(31, N))) + 1) / (N + 1.0)).astype(np.float32)
    labels = (np.arange(N) % 3 + 1).astype(np.int64)
    path = det.write_detections_npz(str(tmp_path / "masks" / "scene.npz"), masks, boxes, scores, labels, shape, top_k=5)
    got = mk.load_3d_masks(path)
    inds = np.argsort(scores)[::-1][:5]                               # the reference's selection (run_rcnn.py:658-664)
    bits = recorded_bits(golden, "mid", N, shape)
    assert np.array_equal(got["masks"], bits[inds]) and got["masks"].dtype == bool
    assert np.array_equal(got["scores"], scores[inds]) and np.array_equal(got["labels"], labels[inds])
    assert np.array_equal(got["boxes"], boxes[inds])
    all_of_them = mk.load_3d_masks(det.write_detections_npz(str(tmp_path / "all.npz"), masks, boxes, scores, labels, shape))
    assert len(all_of_them["masks"]) == N


@pytest.mark.parametrize("n,top_k", [(0, 30), (3, 0)])
def test_write_detections_npz_without_detections(tmp_path, n, top_k):
    """A scene whose detector kept nothing (or top_k = 0): the four keys with k = 0, as the reference's np.savez writes."""
    shape = (5, 4, 3)
    m = np.full((n, 4, 4, 4), 0.9, np.float32)
    b = np.tile(np.asarray([[0, 0, 0, 3, 3, 3]], np.float32), (n, 1))
    path = det.write_detections_npz(str(tmp_path / "none.npz"), m, b, np.linspace(0.9, 0.5, n).astype(np.float32),
                                    np.ones(n, np.int64), shape, top_k=top_k)
    got = mk.load_3d_masks(path)
    assert got["masks"].shape == (0,) + shape and got["masks"].dtype == bool
    assert got["scores"].shape == (0,) and got["labels"].shape == (0,) and got["boxes"].shape == (0, 6)
    assert got["scores"].dtype == np.float32 and got["labels"].dtype == np.int64 and got["boxes"].dtype == np.float32


# ---- arguments and the C ABI ------------------------------------------------------------------------------------------------
def test_argument_errors():
    m, b = np.zeros((2, 4, 4, 4), np.float32), np.asarray([[0, 0, 0, 2, 2, 2]] * 2, np.float32)
    with pytest.raises(ValueError, match="cube"):
        det.paste_masks(np.zeros((2, 4, 4, 3), np.float32), b, (5, 5, 5))
    with pytest.raises(ValueError, match="boxes must be"):
        det.paste_masks(m, b[:1], (5, 5, 5))
    with pytest.raises(ValueError, match="image_shape"):
        det.paste_masks(m, b, (5, 5))
    with pytest.raises(ValueError, match="threshold"):
        det.paste_masks(m, b, (5, 5, 5), threshold=-1.0)
    with pytest.raises(ValueError, match="out must"):
        det.paste_masks(m, b, (5, 5, 5), out="uint8")
    with pytest.raises(ValueError, match="oriented"):
        det.nms_3d(np.zeros((3, 7), np.float32), np.zeros(3, np.float32), 0.2)
    with pytest.raises(ValueError, match="scores"):
        det.batched_nms_3d(np.zeros((3, 6), np.float32), np.zeros(2, np.float32), np.zeros(3, np.int64), 0.2)
    with pytest.raises(ValueError, match="boxes must be"):
        det.postprocess_detections(np.zeros((3, 2, 6), np.float32), np.zeros((3, 3), np.float32), (5, 5, 5))
    with pytest.raises(ValueError, match="planes must be"):
        det.planes_to_voxel_words((torch.zeros(2, 3, dtype=torch.int64), None, (5, 5, 5)))
    with pytest.raises(ValueError, match="scores"):
        det.write_detections_npz("unused.npz", m, b, np.zeros(3, np.float32), np.zeros(2, np.int64), (5, 5, 5))


def test_more_boxes_than_the_kernels_take_use_the_greedy_loop():
    """n > 4096 is documented to take the composable path whatever ``fused`` says (on the CPU it is the only path)."""
    n = det.NMS_MAX_BOXES + 1
    lo = np.arange(n, dtype=np.float32)[:, None] * np.ones(3, np.float32)
    boxes = np.concatenate([lo, lo + 1], 1)                           # disjoint unit cubes: every box survives
    keep = det.batched_nms_3d(boxes, np.arange(n, 0, -1, dtype=np.float32), np.zeros(n, np.int64), 0.2, fused=True)
    assert keep.tolist() == list(range(n))


def test_exports_are_registered_and_the_abi_version_is_unchanged():
    from instance_nerf_amd import _lib, build
    for name in NEW:
        assert name in _lib.EXPORTS
    assert "detect.hip" in build.SOURCES and _lib.ABI_VERSION == 13
    src = open(os.path.join(build.CSRC, "detect.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "-ffp-contract=off" in build.FLAGS


def test_exports_reject_one_bad_argument():
    """Host pointers, no launch: every limit the header names comes back as INR_EINVAL with a message."""
    import ctypes
    from instance_nerf_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 12)
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        return rc, (lib.inr_last_error() or b"").decode()
    good = dict(N=2, M=4, W=5, L=5, H=5, thresh=0.5)

    def paste(planes=a, **over):
        v = dict(good, **over)
        return call("inr_paste_masks", p(a), p(a), v["N"], v["M"], v["W"], v["L"], v["H"], v["thresh"], p(planes), p(a), None, None)
    for over, needle in ((dict(N=-1), "N must"), (dict(N=1025), "N must"), (dict(M=0), "M must"), (dict(M=1025), "M must"),
                         (dict(W=0), "W, L, H"), (dict(W=2048, L=2048, H=512), "W, L, H"), (dict(thresh=-0.5), "thresh"),
                         (dict(thresh=float("nan")), "thresh"), (dict(planes=a + 4), "misaligned"), (dict(planes=None), "null")):
        rc, msg = paste(**over)
        assert rc == -1 and needle in msg, (over, rc, msg)
    assert call("inr_paste_masks", None, None, 0, 4, 5, 5, 5, 0.5, None, None, None, None)[0] == 0       # N = 0: nothing to do
    for args, needle in (((p(a), 0, 64, 0, p(a), None), "k must"), ((p(a), 2, 0, 0, p(a), None), "V must"),
                         ((p(a), 2, 64, 2, p(a), None), "base must"), ((p(a), 2, 64, 0, None, None), "null")):
        rc, msg = call("inr_planes_to_voxel_words", *args)
        assert rc == -1 and needle in msg, (args, rc, msg)
    assert call("inr_nms_3d_pairs", p(a), p(a), 4097, 0.2, p(a), None)[0] == -1
    assert call("inr_nms_3d_pairs", p(a), None, 4, 0.2, p(a), None)[0] == -1
    assert call("inr_nms_3d_pairs", None, None, 0, 0.2, None, None)[0] == 0
    assert call("inr_nms_3d_scan", p(a), 4097, p(a), p(a), None)[0] == -1
    assert call("inr_nms_3d_scan", p(a), 4, None, p(a), None)[0] == -1
    assert call("inr_nms_3d_scan", p(a), 4, p(a), None, None)[0] == -1
