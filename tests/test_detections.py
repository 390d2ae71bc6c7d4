"""The detector tail on the GPU (csrc/detect.hip through instance_nerf_amd/detections.py): the fused kernels against the
numpy restatement (tests/paste_reference.py) and the committed record of the reference's own run
(tests/golden/detections.npz).  Planes, areas, the fp32 samples and the NMS survivors must all be EQUAL."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detections_cases as dc  # noqa: E402
import paste_reference as pr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUN_VOXELS = 256 * 64            # csrc/detect.hip kPasteRun words of 64 voxels: the unit of the paste kernel's skip


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "detections.npz"))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_paste(masks, boxes, shape, threshold=0.5, want_bits=None):
    """Fused planes, areas and samples against the restatement; two calls identical.  -> (packed, restated bits)."""
    from instance_nerf_amd import detections as det
    tm, tb = torch.from_numpy(masks).to(DEV), torch.from_numpy(boxes).to(DEV)
    N, V = len(masks), int(np.prod(shape))
    restated = pr.paste_soft(masks, boxes, shape)
    bits = restated >= np.float32(threshold)
    if want_bits is not None:
        assert np.array_equal(bits, want_bits)
    planes, area, shp = det.paste_masks(tm, tb, shape, threshold, out="planes")
    again = det.paste_masks(tm, tb, shape, threshold, out="planes")
    assert planes.is_cuda and planes.dtype == torch.int64 and tuple(planes.shape) == (N, (V + 63) // 64) and shp == tuple(shape)
    assert torch.equal(planes, again[0]) and torch.equal(area, again[1])
    got = planes.cpu().numpy().view(np.uint64)
    want = pr.pack_planes(bits)
    assert np.array_equal(got, want), (shape, int((got != want).sum()))
    assert area.dtype == torch.int32 and np.array_equal(area.cpu().numpy(), bits.reshape(N, V).sum(1))
    soft = det.paste_masks(tm, tb, shape, threshold, out="soft")
    assert same_bits(soft.cpu().numpy(), restated), (shape, int((soft.cpu().numpy() != restated).sum()))
    assert np.array_equal(det.paste_masks(tm, tb, shape, threshold, out="masks").cpu().numpy(), bits)
    return (planes, area, shp), bits


@pytest.mark.parametrize("name", ["small", "mid", "big", "empty"])
def test_fused_paste_equals_the_reference_record(golden, name):
    """(9,7,5) M = 4; (24,20,17) M = 20, V = 8160: the tail word is half full; (40,33,21) M = 28; N = 0.  The corners of
    the fixture: boxes inside, on the far faces, leaving the grid, integer, side 0.3, the all-0.5 mask, exact 0s and 1s."""
    masks, boxes, shape = dc.paste_cases()[name]
    V = int(np.prod(shape))
    want = np.unpackbits(golden[f"{name}_bits"])[:len(masks) * V].astype(bool).reshape((len(masks),) + tuple(shape))
    check_paste(masks, boxes, shape, want_bits=want)


@pytest.mark.parametrize("shape,M", [((3, 3, 3), 4), ((8, 8, 8), 4), ((5, 3, 70), 5), ((6, 5, 4), 1), ((6, 5, 4), 2)])
def test_fused_paste_small_volumes_and_masks(shape, M):
    """V below a word and exactly a word; rows longer than a wave; M = 1 (one texel covers everything) and M = 2."""
    boxes = np.concatenate([dc.corner_boxes(shape), dc.random_boxes(5, 3, shape)])
    masks = dc.mask_probs(10 + M, len(boxes), M, dc.CORNER_KINDS)
    check_paste(masks, boxes, shape)
    check_paste(masks, boxes, shape, threshold=0.25)


def test_fused_paste_dead_boxes_are_empty():
    m = np.ones((4, 3, 3, 3), np.float32)
    boxes = np.asarray([[1, 1, 1, 1, 4, 4], [1, 1, 1, 0.5, 4, 4], [np.nan, 0, 0, 3, 3, 3], [0, 0, 0, np.inf, 3, 3]], np.float32)
    packed, bits = check_paste(m, boxes, (5, 5, 5))
    assert not bits.any() and int(packed[1].sum()) == 0


@pytest.mark.parametrize("shape", [(130, 16, 16), (70, 17, 15)])
def test_fused_paste_support_on_run_boundaries(shape):
    """A workgroup (256 words) skips its run when every voxel of it lies outside the mask's support along W.  Boxes of
    side 8 with M = 5 (a texel is 2 voxels) whose support ends exactly on, one voxel before and one voxel after the first
    w of a run, and the same for where it starts; one box starts on the edge itself, so the last w of the run before it
    still holds samples (a skip too eager by half a texel would lose them); in (70,17,15) the run boundary falls inside a
    w slice."""
    LH = shape[1] * shape[2]
    edge = RUN_VOXELS // LH                              # (130,16,16): w = 64 starts run 1 exactly
    rows = []
    for d in (-1, 0, 1):
        rows.append([edge + d - 10, -1, -1, edge + d - 2, shape[1] + 1, shape[2] + 1])      # support ends at w = edge + d
        rows.append([edge + d + 2, -1, -1, edge + d + 10, shape[1] + 1, shape[2] + 1])      # support starts at w = edge + d
    rows.append([edge, -1, -1, edge + 8, shape[1] + 1, shape[2] + 1])      # starts ON the edge: p(edge - 1) = -0.5, weight 0.5
    boxes = np.concatenate([np.asarray(rows, np.float32), dc.random_boxes(6, 4, shape)])
    masks = np.maximum(dc.mask_probs(17, len(boxes), 5), np.float32(1 / 256))               # no zero texel: the support shows
    packed, bits = check_paste(masks, boxes, shape, threshold=1 / 1024)
    assert bits[6, edge - 1].any() and not bits[6, :edge - 1].any()        # the last w of the run before the box holds bits
    assert not bits[0, edge - 1:].any() and bits[0, edge - 2].any()                         # ends one voxel before the edge
    assert not bits[2, edge:].any() and bits[2, edge - 1].any()                             # ends exactly on it
    assert bits[4, edge].any() and bits[1].any() and bits[3].any() and bits[5].any()        # ends one voxel past it


@pytest.mark.parametrize("N", [0, 1, 33, 70])
def test_fused_planes_to_voxel_words(N):
    """0, 1, 33 and 70 masks: across the 32-mask word of the projector's layout, more than one grid row of the paste."""
    from instance_nerf_amd import detections as det, evaluate as ev, masks as mk
    shape = (24, 20, 17)
    boxes = dc.random_boxes(40 + N, N, shape)
    masks = dc.mask_probs(50 + N, N, 4)
    packed, bits = check_paste(masks, boxes, shape)
    words = det.planes_to_voxel_words(packed)
    want = mk.pack_mask_words(torch.from_numpy(bits), DEV)
    assert len(words) == len(want) == (N + 31) // 32
    for a, b in zip(words, want):
        assert a.dtype == torch.int32 and tuple(a.shape) == shape and torch.equal(a, b)
    for a, b in zip(words, det.planes_to_voxel_words(packed, fused=False)):
        assert torch.equal(a, b)
    if N:
        order = mk.candidate_order(range(1, N + 1))
        got = det.planes_to_voxel_words(packed, order=order)
        assert all(torch.equal(a, b) for a, b in zip(got, mk.pack_mask_words(torch.from_numpy(bits[order]), DEV)))
        iou = ev.mask_iou_3d(packed, packed).cpu()
        assert torch.equal(iou.nan_to_num(-1), ev.mask_iou_3d(bits, bits, fused=False).nan_to_num(-1))


# ---- NMS -----------------------------------------------------------------------------------------------------------------
def nms_inputs(n, classes, seed):
    u = dc.uniform(seed, n * 6).reshape(n, 6)
    span = 4.0 * max(n, 1) ** (1 / 3)                      # a few boxes per place: a good share is suppressed
    lo = u[:, :3] * span
    boxes = np.concatenate([lo, lo + 2 + u[:, 3:] * 6], 1).astype(np.float32)
    scores = ((np.argsort(np.argsort(dc.uniform(seed + 1, n))) + 1) / (n + 1.0)).astype(np.float32)
    cls = (dc.uniform(seed + 2, n) * classes).astype(np.int64)
    return boxes, scores, cls


@pytest.mark.parametrize("classes", [1, 5])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300, 4096])
def test_fused_nms_equals_the_greedy_restatement(n, classes):
    from instance_nerf_amd import detections as det
    boxes, scores, cls = nms_inputs(n, classes, 100 + n)
    want = pr.batched_nms(boxes, scores, cls, 0.2)
    got = det.batched_nms_3d(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(cls).to(DEV), 0.2)
    assert got.is_cuda and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (n, len(want), len(got))
    if n >= 63:
        assert n // 20 < len(want) < n                    # boxes are suppressed, boxes survive
    if n == 300:
        twin = det.batched_nms_3d(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(cls).to(DEV), 0.2,
                                  fused=False)
        assert torch.equal(twin, got)


@pytest.mark.parametrize("t", [0.2, 0.25, 0.5])
def test_fused_nms_equals_the_reference_record(golden, t):
    """The fixture's corners: overlap across classes only, an IoU exactly at the threshold."""
    from instance_nerf_amd import detections as det
    boxes, scores, cls = dc.nms_case()
    got = det.batched_nms_3d(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(cls).to(DEV), t)
    assert np.array_equal(got.cpu().numpy(), golden[f"nms_keep_{t}"])
    nan = boxes[:4].copy()
    nan[1, 0] = np.nan                                    # a NaN IoU suppresses
    keep = det.batched_nms_3d(torch.from_numpy(nan).to(DEV), torch.tensor([4., 3, 2, 1], device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), 0.99)
    assert np.array_equal(keep.cpu().numpy(), pr.batched_nms(nan, [4, 3, 2, 1], np.zeros(4, np.int64), 0.99))
    with pytest.raises(ValueError, match="int32"):            # ids that differ only above bit 31 are refused, not merged
        det.batched_nms_3d(torch.from_numpy(nan).to(DEV), torch.tensor([4., 3, 2, 1], device=DEV),
                           torch.tensor([1, 1 + 2 ** 32, 1, 1], dtype=torch.int64, device=DEV), 0.2)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_heads_to_file_to_projection(golden, tmp_path, room, room_bitfield, params_k16):
    """postprocess_detections -> write_detections_npz -> load_3d_masks -> project_3d_masks(packed=...) equals
    project_3d_masks on the bool masks of the file."""
    from instance_nerf_amd import detections as det, masks as mk
    from test_gpu_parity import _network, _t
    hb, hs, shape = dc.head_case()
    b, s, l = det.postprocess_detections(torch.from_numpy(hb).to(DEV), torch.from_numpy(hs).to(DEV), shape)
    assert same_bits(b.cpu().numpy(), golden["head_boxes"]) and same_bits(s.cpu().numpy(), golden["head_scores"])
    assert np.array_equal(l.cpu().numpy(), golden["head_labels"])
    k = 34                                                # two words per voxel in the projector
    probs = torch.from_numpy(np.maximum(dc.mask_probs(70, len(b), 6), np.float32(0.75))).to(DEV)
    path = det.write_detections_npz(str(tmp_path / "masks" / "scene.npz"), probs, b, s, l, shape, top_k=k)
    m3 = mk.load_3d_masks(path)
    assert m3["masks"].shape == (k,) + tuple(shape) and np.array_equal(m3["scores"], golden["head_scores"][:k])
    assert np.array_equal(m3["boxes"], golden["head_boxes"][:k]) and np.array_equal(m3["labels"], golden["head_labels"][:k])
    assert np.array_equal(m3["masks"], pr.paste_bits(probs[:k].cpu().numpy(), golden["head_boxes"][:k], shape))
    packed = det.paste_masks(probs[:k], b[:k], shape, out="planes")
    net = _network(params_k16, K=0).eval()
    net.density_bitfield.copy_(_t(room_bitfield))
    poses, intr, H, W = room.cameras(n=1, H=32, W=32, focal=16.0)
    want = mk.project_3d_masks(net, m3["masks"], [-1, -1, -1], [1, 1, 1], poses, intr, H, W, thresh=0.02)
    got = mk.project_3d_masks(net, None, [-1, -1, -1], [1, 1, 1], poses, intr, H, W, thresh=0.02,
                              packed=(k, det.planes_to_voxel_words(packed)))
    assert want.any() and np.array_equal(got, want)
    # project_and_match takes its words in CANDIDATE order (ids 10..34 sort before 2)
    yy, xx = np.mgrid[0:H, 0:W]
    seg = (((yy // 8) * 4 + xx // 8 + 1) * 50).astype(np.int32)[None]
    order = mk.candidate_order(range(1, k + 1))
    assert order != list(range(k))
    ref = mk.project_and_match(net, m3["masks"], [-1, -1, -1], [1, 1, 1], poses, intr, H, W, seg, thresh=0.02, iou_thresh=0.0)
    fast = mk.project_and_match(net, None, [-1, -1, -1], [1, 1, 1], poses, intr, H, W, seg, thresh=0.02, iou_thresh=0.0,
                                packed=(k, det.planes_to_voxel_words(packed, order=order)))
    assert torch.equal(fast, ref) and bool((ref > 0).any())
