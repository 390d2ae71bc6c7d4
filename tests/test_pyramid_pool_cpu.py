"""The multi-scale pooler (instance_nerf_amd/roi_align/poolers.py) without a GPU: the level mapper and the composable
path against the reference's OWN recorded pooler run (tests/golden/reference_calls.npz, recorded by
tests/golden/make_reference_calls_golden.py from /root/reference/nerf_rcnn/model/poolers.py), with the oracle's
roi_align_3d as the callable; the argument checks of the two pyramid exports of include/inr.h."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe  # noqa: E402
from instance_nerf_amd.roi_align import LevelMapper, MultiScaleRoIAlign3D, multiscale_roi_align_3d, poolers
from oracle import consumers, roialign

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_calls.npz"))


class Recorder:
    """oracle.roialign.roi_align_3d behind the extension's signature, keeping every call it receives."""

    def __init__(self):
        self.calls = []

    def __call__(self, input, rois, roi_inds, out_w, out_l, out_h, spatial_scale):
        self.calls.append(dict(input=input, rois=rois, roi_inds=roi_inds, sizes=(out_w, out_l, out_h), scale=spatial_scale))
        return torch.from_numpy(roialign.roi_align_3d(input.numpy(), rois.numpy(), roi_inds.numpy(), out_w, out_l, out_h,
                                                      spatial_scale))


def _side_boxes(sides):
    b = np.zeros((len(sides), 6), np.float32)
    b[:, 3:] = np.asarray(sides, np.float32)[:, None]
    return b


def test_level_mapper_reproduces_the_recorded_levels(ref):
    mapper = LevelMapper(2, 4)
    edges = _side_boxes(ref["lm_sides"])
    assert {39.99, 40.0, 40.01, 79.99, 80.0, 80.01} <= {round(float(s), 2) for s in ref["lm_sides"]}
    got = mapper([torch.from_numpy(edges)])
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), ref["lm_levels"])
    assert np.array_equal(got.numpy(), consumers.level_mapper(edges, 2, 4))
    boxes = [torch.from_numpy(ref["ms_boxes0"]), torch.from_numpy(ref["ms_boxes1"])]
    got = mapper(boxes).numpy()
    assert np.array_equal(got, ref["ms_levels"])
    assert np.array_equal(got, consumers.level_mapper(np.concatenate([ref["ms_boxes0"], ref["ms_boxes1"]]), 2, 4))


@pytest.fixture(scope="module")
def replay(ref):
    rec = Recorder()
    pool = MultiScaleRoIAlign3D(4, 2)
    pool.roi_align = rec
    feats = [torch.from_numpy(ref[f"ms_feat{l}"]) for l in range(3)]
    boxes = [torch.from_numpy(ref["ms_boxes0"]), torch.from_numpy(ref["ms_boxes1"])]
    shapes = [tuple(int(v) for v in s) for s in ref["ms_image_shapes"]]
    out = pool(feats, boxes, shapes)
    return pool, rec, out, feats, boxes, shapes


def test_module_infers_the_recorded_scales_and_levels(ref, replay):
    pool = replay[0]
    assert pool.scales == [0.25, 0.125, 0.0625] == list(ref["ms_scales"])
    assert (pool.map_levels.k_min, pool.map_levels.k_max) == (2, 4) == tuple(int(v) for v in ref["ms_kmin_kmax"])
    assert pool.output_size == (4, 4, 4) and pool.sampling_ratio == 2


def test_composable_path_issues_exactly_the_recorded_calls(ref, replay):
    _, rec, _, feats, _, _ = replay
    assert len(rec.calls) == int(ref["ms_n_calls"]) == 3
    for l, c in enumerate(rec.calls):
        want_rois, want_inds = ref[f"call{2 + l}_rois"], ref[f"call{2 + l}_roi_inds"]
        assert c["input"] is feats[l] and str(ref[f"call{2 + l}_input_key"]) == f"ms_feat{l}"
        assert c["rois"].dtype == torch.float32 and np.array_equal(c["rois"].numpy(), want_rois)
        assert c["roi_inds"].dtype == torch.int32 and np.array_equal(c["roi_inds"].numpy(), want_inds)
        assert c["scale"] == float(ref[f"call{2 + l}_scale"])
        assert c["sizes"] == tuple(int(v) for v in ref[f"call{2 + l}_meta"][6:9]) == (4, 4, 4)


def test_composable_result_is_the_oracle_row_of_each_roi_on_its_recorded_level(ref, replay):
    _, _, out, _, _, _ = replay
    assert isinstance(out, list) and [tuple(o.shape) for o in out] == [(6, 2, 4, 4, 4), (4, 2, 4, 4, 4)]
    assert all(o.dtype == torch.float32 for o in out)
    rows = torch.cat(out).numpy()
    boxes = np.concatenate([ref["ms_boxes0"], ref["ms_boxes1"]])
    img = np.asarray([0] * 6 + [1] * 4, np.int32)
    tags = np.concatenate([ref["ms_result_tags0"], ref["ms_result_tags1"]])
    for k in range(10):
        level = int(ref["ms_levels"][k])
        assert tags[k] == 3 + level                  # the reference's own scatter put that call's row here
        want = roialign.roi_align_3d(ref[f"ms_feat{level}"], boxes[k:k + 1], img[k:k + 1], 4, 4, 4, float(ref["ms_scales"][level]))
        assert np.array_equal(rows[k], want[0]), k


def test_one_level_returns_a_single_tensor(ref):
    rec = Recorder()
    pool = MultiScaleRoIAlign3D((2, 3, 2), -1)
    pool.roi_align = rec
    feat = torch.from_numpy(ref["ms_feat2"])
    boxes = [torch.from_numpy(ref["ms_boxes0"][:2]), torch.from_numpy(ref["ms_boxes1"][:1])]
    out = pool([feat], boxes, [(160, 128, 96)])
    assert torch.is_tensor(out) and out.shape == (3, 2, 2, 3, 2) and out.dtype == torch.float32
    assert len(rec.calls) == 1 and rec.calls[0]["scale"] == 0.0625 and rec.calls[0]["sizes"] == (2, 3, 2)
    assert rec.calls[0]["roi_inds"].tolist() == [0, 0, 1]


def test_an_image_without_boxes_gets_an_empty_tensor(ref):
    feats = [torch.from_numpy(ref[f"ms_feat{l}"]) for l in range(3)]
    boxes = [torch.zeros(0, 6), torch.from_numpy(ref["ms_boxes1"][:2])]
    out = multiscale_roi_align_3d(feats, boxes, (2, 2, 2), 2, [0.25, 0.125, 0.0625], LevelMapper(2, 4), roi_align=Recorder())
    assert [tuple(o.shape) for o in out] == [(0, 2, 2, 2, 2), (2, 2, 2, 2, 2)]
    with pytest.raises(ValueError):
        multiscale_roi_align_3d(feats, boxes, (2, 2, 2), 2, None, None)


def test_scales_are_set_up_on_the_first_call_and_kept(replay):
    pool, rec, _, feats, boxes, _ = replay
    scales, mapper = pool.scales, pool.map_levels
    n = len(rec.calls)
    pool(feats, [boxes[0][:1], boxes[1][:0]], [(320, 256, 192)])            # other image extents: nothing is re-inferred
    assert pool.scales is scales and pool.map_levels is mapper
    assert len(rec.calls) == n + 1 and rec.calls[-1]["scale"] == 0.25
    del rec.calls[n:]


def test_order_is_the_stable_argsort_of_the_levels():
    levels = torch.tensor([2, 0, 1, 0, 2, 1, 0, 0, 2], dtype=torch.int32)
    order = poolers.level_order(levels)
    assert order.dtype == torch.int32 and order.tolist() == [1, 3, 6, 7, 2, 5, 0, 4, 8]
    assert order.tolist() == np.argsort(levels.numpy(), kind="stable").tolist()


def test_fused_path_has_no_cpu_fallback(ref):
    """CPU tensors take the composable loop; the product's own roi_align_3d behind it then refuses them loudly."""
    feats = [torch.from_numpy(ref[f"ms_feat{l}"]) for l in range(3)]
    boxes = [torch.from_numpy(ref["ms_boxes0"])]
    with pytest.raises(RuntimeError, match="GPU tensor"):
        multiscale_roi_align_3d(feats, boxes, (2, 2, 2), 2, [0.25, 0.125, 0.0625], LevelMapper(2, 4))


@pytest.fixture(scope="module")
def abi():
    return abi_probe.run_abi_child("pyramid_abi_child.py", env=abi_probe.NO_GPU)


@pytest.mark.parametrize("name", ["inr_roi_align_3d_pyramid_forward", "inr_roi_align_3d_pyramid_backward"])
@pytest.mark.parametrize("case,needle", [
    ("n_levels_0", "n_levels"), ("n_levels_9", "n_levels"), ("n_levels_9_null_table", "n_levels"), ("zero_bins", "out_l"),
    ("K_negative", "K"), ("C_zero", "C"), ("rois_null", "null pointer"), ("roi_levels_null", "null pointer"),
    ("level_dims_null", "null pointer"), ("level_dims_zero", "level_dims"),
])
def test_pyramid_exports_reject_bad_arguments(abi, name, case, needle):
    rc, msg = abi[f"{name}:{case}"]
    assert rc == EINVAL and needle in msg, (name, case, rc, msg)


def test_pyramid_forward_rejects_a_null_level_and_takes_no_rois(abi):
    rc, msg = abi["inr_roi_align_3d_pyramid_forward:level_ptrs_null_entry"]
    assert rc == EINVAL and "level_ptrs[1]" in msg, (rc, msg)
    for name in ("inr_roi_align_3d_pyramid_forward", "inr_roi_align_3d_pyramid_backward"):
        assert abi[f"{name}:K_zero_null_ok"][0] == 0, name


def test_abi_version_is_unchanged_and_the_level_limit_matches_the_header():
    import re
    from instance_nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "inr.h")).read()
    assert _lib.ABI_VERSION == 13
    assert _lib.ROI_MAX_LEVELS == int(re.search(r"#define INR_ROI_MAX_LEVELS (\d+)", header).group(1)) == 8
