"""3-D mask metric on the GPU (csrc/overlap.hip through instance_nerf_amd/evaluate.py): the fused counts against the
composable path on the same device and a brute-force count, every integer; IoU bit-equal; two calls identical."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluate_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(0, 7), (1, 0), (7, 8), (8, 9), (9, 1), (33, 65), (65, 33)]          # tile edges both ways, more than one tile
_POP = np.asarray([bin(i).count("1") for i in range(256)], np.int64)


def brute_counts_packed(a, b):
    """As ec.brute_counts for large volumes: bytes of np.packbits, AND, a 256-entry popcount table, one pair at a time."""
    pa, pb = np.packbits(a, axis=1), np.packbits(b, axis=1)
    inter = np.zeros((len(a), len(b)), np.int64)
    for i in range(len(a)):
        for j in range(len(b)):
            inter[i, j] = _POP[pa[i] & pb[j]].sum()
    return inter, _POP[pa].sum(1), _POP[pb].sum(1)


def contents(kind, rng, k, V):
    if kind == "ones":
        return np.ones((k, V), bool)
    if kind == "zeros":
        return np.zeros((k, V), bool)
    return ec.random_masks(rng, k, V, 0.5 if kind == "half" else 0.01)


def check_case(a, b, brute):
    """a [kA, V], b [kB, V] bool."""
    from instance_nerf_amd import evaluate as ev
    V = a.shape[1]
    ta, tb = torch.from_numpy(ec.as_volume(a, V)).to(DEV), torch.from_numpy(ec.as_volume(b, V)).to(DEV)
    fused = ev.mask_overlap(ta, tb, fused=True)
    again = ev.mask_overlap(ta, tb, fused=True)
    twin = ev.mask_overlap(ta, tb, fused=False)
    want = brute(a, b)
    for name, f, g, t, w in zip(("inter", "area1", "area2"), fused, again, twin, want):
        assert f.is_cuda and f.dtype == torch.int64
        assert torch.equal(f, g), name
        assert torch.equal(f, t), name
        assert np.array_equal(f.cpu().numpy(), w), (name, a.shape, b.shape)
    iou = ev.mask_iou_3d(ta, tb, fused=True)
    assert iou.dtype == torch.float32 and tuple(iou.shape) == (len(a), len(b))
    assert ec.same_bits(iou.cpu().numpy(), ec.brute_iou(*want))
    assert ec.same_bits(iou.cpu().numpy(), ev.mask_iou_3d(ta, tb, fused=False).cpu().numpy())
    return iou


@pytest.mark.parametrize("kind", ["half", "sparse", "ones", "zeros"])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 5 * 7 * 9])
def test_fused_counts_small_volumes(V, kind):
    rng = np.random.default_rng(V)
    for kA, kB in PAIRS:
        check_case(contents(kind, rng, kA, V), contents(kind, rng, kB, V), ec.brute_counts)


@pytest.mark.parametrize("V", [1, 65, 5 * 7 * 9])
def test_identical_sets_have_a_unit_diagonal(V):
    rng = np.random.default_rng(V + 1)
    a = ec.random_masks(rng, 9, V, 0.5)
    a[:, 0] = True                                       # no empty mask: the diagonal is 1, not NaN
    iou = check_case(a, a.copy(), ec.brute_counts)
    assert torch.equal(torch.diagonal(iou), torch.ones(9, device=DEV))


@pytest.mark.parametrize("kind", ["half", "sparse", "ones"])
def test_fused_counts_across_workgroups(kind):
    """70^3 voxels = 5360 words: with the default launch six runs of 1024 words, the last one ragged (240 words), and 21
    pack workgroups per mask."""
    from instance_nerf_amd import evaluate as ev
    V = 70 ** 3
    nW = (V + 63) // 64
    runs = -(-nW // ev.OVERLAP_MIN_RUN_WORDS)
    assert runs >= 3 and nW % ev.OVERLAP_MIN_RUN_WORDS != 0
    rng = np.random.default_rng(7)
    for kA, kB in [(9, 7), (8, 17)]:
        check_case(contents(kind, rng, kA, V), contents(kind, rng, kB, V), brute_counts_packed)


def test_run_words_do_not_change_the_counts():
    from instance_nerf_amd import evaluate as ev
    rng = np.random.default_rng(8)
    V = 41 * 43 * 37
    a, b = ec.random_masks(rng, 9, V, 0.3), ec.random_masks(rng, 10, V, 0.3)
    pa = ev.pack_mask_planes(torch.from_numpy(ec.as_volume(a, V)).to(DEV))
    pb = ev.pack_mask_planes(torch.from_numpy(ec.as_volume(b, V)).to(DEV))
    want = brute_counts_packed(a, b)[0]
    for run in (0, 256, 512, 4096):
        assert np.array_equal(ev.overlap_planes(pa, pb, run_words=run).cpu().numpy(), want), run


def test_uint8_masks_nonzero_is_inside_and_packed_input():
    from instance_nerf_amd import evaluate as ev
    rng = np.random.default_rng(9)
    shape = (5, 7, 9)
    a = (rng.integers(0, 256, size=(7,) + shape) * (rng.random((7,) + shape) < 0.5)).astype(np.uint8)
    b = rng.random((9,) + shape) < 0.5
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    want = ec.brute_counts(a != 0, b)
    packed = ev.pack_mask_planes(ta)
    assert torch.equal(packed[0], ev.pack_mask_planes(ta, fused=False)[0])             # same words, zero tail bits
    assert torch.equal(packed[1], ev.pack_mask_planes(ta, fused=False)[1])
    for got in (ev.mask_overlap(ta, tb), ev.mask_overlap(packed, tb), ev.mask_overlap(packed, b), ev.mask_overlap(packed, tb, fused=False)):
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("shape", [(5, 7, 9), (37, 41, 43)])
@pytest.mark.parametrize("K,first", [(1, 0), (1, 1), (16, 0), (16, 1), (64, 0), (64, 1)])
def test_label_volume_pack(K, first, shape):
    """(37, 41, 43) = 65231 voxels = 1020 words: four pack workgroups, the last one ragged."""
    from instance_nerf_amd import evaluate as ev
    rng = np.random.default_rng(K * 2 + first)
    lab = rng.integers(0, K + 5, size=shape).astype(np.uint8)                 # values >= K included
    lab[rng.random(shape) < 0.3] = 255
    tl = torch.from_numpy(lab).to(DEV)
    planes, area, shp = ev.pack_label_planes(tl, K, first)
    again = ev.pack_label_planes(tl, K, first)
    masks = torch.stack([tl == c for c in range(first, K)]) if K > first else torch.zeros((0,) + shape, dtype=torch.bool, device=DEV)
    want_planes, want_area, _ = ev.pack_mask_planes(masks, fused=False)
    assert shp == shape and tuple(planes.shape) == (K - first, (lab.size + 63) // 64)
    assert torch.equal(planes, want_planes) and torch.equal(area, want_area)
    assert torch.equal(planes, again[0]) and torch.equal(area, again[1])
    if K > first:
        assert torch.equal(planes, ev.pack_mask_planes(masks)[0])
    b = torch.from_numpy(rng.random((5,) + shape) < 0.4).to(DEV)
    got = ev.label_mask_overlap(tl, K, b, first_channel=first)
    for g, t, w in zip(got, ev.label_mask_overlap(tl, K, b, first_channel=first, fused=False), ev.mask_overlap(masks, b)):
        assert torch.equal(g, t) and torch.equal(g, w)
    assert ec.same_bits(ev.label_mask_iou(tl, K, b, first_channel=first).cpu().numpy(),
                        ev.mask_iou_3d(masks, b, fused=False).cpu().numpy())


def test_golden_fixture_fused():
    ec.check_golden(DEV, fused=True)


def test_golden_fixture_composable_on_the_gpu():
    ec.check_golden(DEV, fused=False)


def test_trainer_evaluate_instance_masks(tmp_path, level_table):
    """A small untrained field (O(1) outputs) on a 32^3 lattice against the analytic room: the returned dict equals
    evaluate_masks on the file save_instance_masks writes for the same arguments."""
    from instance_nerf_amd import evaluate as ev
    from instance_nerf_amd.nerf import NeRFNetwork
    from instance_nerf_amd.nerf.utils import Trainer
    from instance_nerf_amd.scene import RoomScene
    from oracle.field import init_params
    K, res = 16, 32
    p = init_params(seed=0, table=level_table, table_std=1.0, K=K)
    net = NeRFNetwork(cuda_ray=True, num_instances=K, min_near=0.05).to(DEV)
    net.load_state_dict({"encoder.embeddings": p["embeddings"], "sigma_net.0.weight": p["sigma_w0"],
                         "sigma_net.1.weight": p["sigma_w1"], "color_net.0.weight": p["color_w0"],
                         "color_net.1.weight": p["color_w1"], "color_net.2.weight": p["color_w2"],
                         "instance_encoder.embeddings": p["inst_embeddings"], "instance_net.0.weight": p["inst_w0"],
                         "instance_net.1.weight": p["inst_w1"], "instance_net.2.weight": p["inst_w2"]}, strict=False)
    tr = Trainer("room", None, net, stage="instance", device=torch.device(DEV), workspace=str(tmp_path / "ws"), mute=True)
    room = RoomScene()
    ax = (np.arange(res, dtype=np.float64) + 0.5) / res * 2.0 - 1.0
    ids = room.instance_of_points(np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)).reshape(res, res, res)
    present = [c for c in range(1, len(room.lo) + 1) if (ids == c).any()]
    gt_masks = np.stack([ids == c for c in present])
    gt = {"masks": gt_masks, "labels": np.asarray([c % 2 + 1 for c in present]),
          "boxes": np.stack([np.concatenate([np.argwhere(m).min(0), np.argwhere(m).max(0) + 1]) for m in gt_masks]).astype(np.float32)}
    cls = np.arange(K - 1) % 2 + 1
    for kw in (dict(max_side=res, sigma_thresh=1.0), dict(max_side=res, sigma_thresh=1.0, components="largest", labels=cls, min_voxels=3)):
        net.train()
        got = tr.evaluate_instance_masks(gt, **kw)
        assert net.training
        path = tr.save_instance_masks(name="scored", **kw)
        want = ev.evaluate_masks(path, gt)
        if "components" not in kw:
            assert np.load(path)["masks"].any(axis=(1, 2, 3)).sum() >= 4      # the field yields several non-empty masks
        assert set(got) == set(want)
        for k in want:
            if isinstance(want[k], float):
                assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), (k, got[k], want[k])
            else:
                assert torch.equal(got[k], want[k]), k
        assert 0.0 <= got["AR_25"] <= 1.0
