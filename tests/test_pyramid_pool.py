"""RoIs pooled from a feature pyramid in one launch (inr_roi_align_3d_pyramid_forward / _backward,
instance_nerf_amd/roi_align/poolers.py): every row against the single-level call of its level (same bits) and against
the oracle, the backward as the transpose of the forward and against the per-level calls, the module against its own
composable path, and the absence of any host synchronisation (graph capture)."""
import numpy as np
import pytest
import torch

from instance_nerf_amd.roi_align import LevelMapper, MultiScaleRoIAlign3D, poolers, pyramid_roi_align_3d
from oracle import roialign

pytestmark = pytest.mark.gpu

DIMS = [(24, 20, 16), (12, 10, 8), (6, 5, 4)]          # the last level sits at the separable kernels' H >= 4 edge
SCALES = [0.5, 0.25, 0.125]
N, CMAX = 2, 16
SIZES = [(5, 5, 5), (4, 3, 5), (10, 10, 10), (11, 11, 11)]      # 11 bins: the chunked forward (kMulti)
# image units of a (48, 40, 32) volume; (x1, y1, z1, x2, y2, z2), image, level
BOXES = [
    ([2, 3, 1, 20, 18, 14], 0, 0),
    ([10.5, 4.2, 6.3, 30.1, 25.7, 20.9], 1, 1),
    ([0, 0, 0, 48, 40, 32], 0, 2),
    ([-6, -4, -2, 54, 24, 20], 1, 0),                   # larger than the volume: 30 cells on x, sampling grid 3..8 there
    ([20, 20, 10, 20.4, 20.6, 10.3], 0, 1),             # thinner than a voxel
    ([200, 200, 200, 230, 240, 250], 1, 1),             # entirely outside (beyond the far corner)
    ([-100, -90, -80, -60, -50, -40], 0, 0),            # entirely outside (before the origin)
    ([40, 10, 5, 60, 30, 20], 1, 2),                    # straddles the far x face
    ([-6, 5, 5, 10, 20, 18], 0, 0),                     # straddles the near x face
    ([12, 8, 4, 40, 36, 30], 1, 2),
    ([5.5, 6.5, 7.5, 25.5, 16.5, 27.5], 1, 1),
    ([30, 2, 3, 47, 39, 31], 0, 0),
    ([1, 1, 1, 9, 9, 9], 0, 1),
    ([16, 12, 8, 32, 28, 24], 1, 2),
]
OUTSIDE = [5, 6]


def _set_mode(mode):
    from instance_nerf_amd import _lib
    _lib.check(_lib.load().inr_roi_align_3d_set_mode(mode), "roi_align_3d_set_mode")


@pytest.fixture(scope="module")
def case():
    """The pyramid (C = 16; the C = 5 tests take its first channels), the boxes, and the same boxes with level 1 left
    empty.  Host copies for the oracle."""
    rng = np.random.default_rng(11)
    feats = [rng.normal(size=(N, CMAX) + d).astype(np.float32) for d in DIMS]
    rois = np.asarray([b[0] for b in BOXES], np.float32)
    inds = np.asarray([b[1] for b in BOXES], np.int32)
    levels = np.asarray([b[2] for b in BOXES], np.int32)
    assert set(levels.tolist()) == {0, 1, 2}
    levels_b = np.where(levels == 1, 2, levels).astype(np.int32)
    return dict(feats=feats, rois=rois, inds=inds, levels={"all": levels, "empty1": levels_b})


_ORACLE = {}


def oracle_rows(case, which, osz):
    """oracle.roialign.roi_align_3d of every RoI on its level, C = 16: computed once per (levels, output size)."""
    key = (which, osz)
    if key not in _ORACLE:
        levels = case["levels"][which]
        out = np.zeros((len(levels), CMAX) + osz, np.float32)
        for l in range(3):
            sel = levels == l
            if sel.any():
                out[sel] = roialign.roi_align_3d(case["feats"][l], case["rois"][sel], case["inds"][sel], *osz, SCALES[l])
        _ORACLE[key] = out
    return _ORACLE[key]


def device_case(case, which, C, requires_grad=False):
    feats = [torch.from_numpy(np.ascontiguousarray(f[:, :C])).cuda().requires_grad_(requires_grad) for f in case["feats"]]
    rois = torch.from_numpy(case["rois"]).cuda()
    inds = torch.from_numpy(case["inds"]).cuda()
    levels = torch.from_numpy(case["levels"][which]).cuda()
    return feats, rois, inds, levels


@pytest.mark.parametrize("mode", [2, 1, 0])
@pytest.mark.parametrize("osz", SIZES)
@pytest.mark.parametrize("C", [5, 16])
def test_pyramid_forward_rows_are_the_single_level_rows(case, C, osz, mode):
    from instance_nerf_amd.roi_align.roi_align import roi_align_3d
    _set_mode(mode)
    try:
        for which in ("all", "empty1"):
            feats, rois, inds, levels = device_case(case, which, C)
            order = poolers.level_order(levels)
            out = pyramid_roi_align_3d(feats, rois, inds, levels, osz, SCALES, order=order)
            assert out.shape == (len(BOXES), C) + osz and out.dtype == torch.float32
            for l in range(3):
                sel = levels == l
                if not bool(sel.any()):
                    continue
                single = roi_align_3d(feats[l], rois[sel], inds[sel], *osz, SCALES[l])
                assert torch.equal(out[sel], single), (which, l)
            err = np.abs(out.cpu().numpy() - oracle_rows(case, which, osz)[:, :C]).max()
            print(f"C {C} osz {osz} mode {mode} {which}: max err vs oracle {err:.2e}")
            assert err < 2e-5, (which, err)
            again = pyramid_roi_align_3d(feats, rois, inds, levels, osz, SCALES, order=order)
            assert torch.equal(out, again)
            unordered = pyramid_roi_align_3d(feats, rois, inds, levels, osz, SCALES, order=None)
            assert torch.equal(out, unordered)
            assert out[OUTSIDE].abs().max().item() == 0.0
    finally:
        _set_mode(0)


@pytest.mark.parametrize("mode", [2, 1])
def test_a_level_outside_the_table_gives_zeros_and_no_gradient(case, mode):
    _set_mode(mode)
    try:
        feats, rois, inds, levels = device_case(case, "all", 5, requires_grad=True)
        bad = levels.clone()
        bad[0], bad[3], bad[9] = 3, -1, 1 << 20
        ok = torch.ones(len(BOXES), dtype=torch.bool, device="cuda")
        ok[[0, 3, 9]] = False
        want = pyramid_roi_align_3d([f.detach() for f in feats], rois, inds, levels, (5, 5, 5), SCALES)
        out = pyramid_roi_align_3d(feats, rois, inds, bad, (5, 5, 5), SCALES, order=poolers.level_order(bad))
        assert torch.equal(out[ok], want[ok]) and out[~ok].abs().max().item() == 0.0
        g = torch.randn(out.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        out.backward(g)
        lhs = (out.detach().double() * g.double()).sum().item()
        rhs = sum((f.detach().double() * f.grad.double()).sum().item() for f in feats)
        assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(lhs)), (lhs, rhs)
    finally:
        _set_mode(0)


@pytest.mark.parametrize("mode", [2, 1, 0])
@pytest.mark.parametrize("osz", SIZES)
@pytest.mark.parametrize("C", [5, 16])
def test_pyramid_backward_is_the_transpose_and_matches_the_per_level_calls(case, C, osz, mode):
    from instance_nerf_amd.roi_align.roi_align import roi_align_3d
    g = torch.randn((len(BOXES), C) + osz, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    try:
        for which in ("all", "empty1"):
            _set_mode(mode)
            feats, rois, inds, levels = device_case(case, which, C, requires_grad=True)
            out = pyramid_roi_align_3d(feats, rois, inds, levels, osz, SCALES, order=poolers.level_order(levels))
            out.backward(g)
            lhs = (out.detach().double() * g.double()).sum().item()
            rhs = sum((f.detach().double() * f.grad.double()).sum().item() for f in feats)
            print(f"C {C} osz {osz} mode {mode} {which}: <out, g> {lhs:.6f}  sum <feat, grad> {rhs:.6f}")
            assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(lhs)), (which, lhs, rhs)
            _set_mode(1)                                   # the per-level single calls, one lane per output element
            for l in range(3):
                sel = levels == l
                if not bool(sel.any()):
                    assert feats[l].grad.abs().max().item() == 0.0       # the empty level: exactly zero
                    continue
                x = feats[l].detach().clone().requires_grad_(True)
                roi_align_3d(x, rois[sel], inds[sel], *osz, SCALES[l]).backward(g[sel])
                diff = (feats[l].grad - x.grad).abs().max().item()
                assert diff <= 1e-3 * x.grad.abs().max().item(), (which, l, diff)
    finally:
        _set_mode(0)


@pytest.mark.parametrize("mode", [2, 1])
def test_a_level_that_needs_no_gradient_gets_none(case, mode):
    _set_mode(mode)
    try:
        g = torch.randn((len(BOXES), 16, 5, 5, 5), device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
        full, rois, inds, levels = device_case(case, "all", 16, requires_grad=True)
        pyramid_roi_align_3d(full, rois, inds, levels, (5, 5, 5), SCALES).backward(g)
        part, _, _, _ = device_case(case, "all", 16, requires_grad=True)
        part[1].requires_grad_(False)
        pyramid_roi_align_3d(part, rois, inds, levels, (5, 5, 5), SCALES).backward(g)
        assert part[1].grad is None
        for l in (0, 2):
            diff = (part[l].grad - full[l].grad).abs().max().item()
            assert diff <= 1e-3 * full[l].grad.abs().max().item(), (l, diff)        # atomics reorder the sums
    finally:
        _set_mode(0)


# ---- the module -------------------------------------------------------------------------------------------------------
IMAGE_SHAPES = [(48, 40, 32)] * 2
# canonical_level + log2(cbrt(volume) / canonical_scale) of every box: fractional part in [0.1, 0.9], so that the
# device's pow / log2 cannot land on another level than the CPU's (a condition on the inputs, not a tolerance)
TARGETS = [[0.5, 1.3, 1.7, 2.2, 2.5, 2.85, 3.4, 4.6], [1.15, 2.6, 3.8, 0.2, 2.12, 1.88]]
TARGETS_B = [[2.3, 3.3, 1.4, 1.6, 0.7, 2.75, 2.2, 3.15], [3.5, 1.25, 1.5, 2.45, 4.2, 2.8]]


def module_boxes(targets, seed):
    rng = np.random.default_rng(seed)
    out = []
    for ts in targets:
        rows = []
        for t in ts:
            side = 40.0 * 2.0 ** (t - 4.0)
            a, b = rng.uniform(0.7, 1.4, 2)
            ext = side * np.asarray([a, b, 1.0 / (a * b)])
            lo = rng.uniform(0, 1, 3) * np.maximum(np.asarray([48, 40, 32]) - ext, 1.0)
            rows.append(np.concatenate([lo, lo + ext]))
        boxes = np.asarray(rows, np.float32)
        vol = np.prod((boxes[:, 3:] - boxes[:, :3]).astype(np.float64), 1)
        frac = (4.0 + np.log2(np.cbrt(vol) / 40.0)) % 1.0
        assert ((frac >= 0.1) & (frac <= 0.9)).all()
        out.append(boxes)
    return out


def test_module_fused_equals_composable_bit_for_bit(case):
    feats = [torch.from_numpy(f).cuda() for f in case["feats"]]
    host_boxes = module_boxes(TARGETS, 21)
    boxes = [torch.from_numpy(b).cuda() for b in host_boxes]
    _set_mode(2)
    try:
        for osz in (5, (4, 3, 5)):
            fused = MultiScaleRoIAlign3D(osz, 2, canonical_scale=40)
            loop = MultiScaleRoIAlign3D(osz, 2, canonical_scale=40)
            loop.fused = False
            a, b = fused(feats, boxes, IMAGE_SHAPES), loop(feats, boxes, IMAGE_SHAPES)
            assert fused.scales == SCALES and (fused.map_levels.k_min, fused.map_levels.k_max) == (1, 3)
            assert isinstance(a, list) and [len(t) for t in a] == [8, 6] == [len(t) for t in b]
            for ta, tb in zip(a, b):
                assert ta.dtype == torch.float32 and torch.equal(ta, tb)
            cpu_levels = LevelMapper(1, 3, canonical_scale=40)([torch.from_numpy(h) for h in host_boxes])
            assert torch.equal(fused.map_levels(boxes).cpu(), cpu_levels)
            assert set(cpu_levels.tolist()) == {0, 1, 2}
    finally:
        _set_mode(0)


def test_module_gradients_reach_every_level(case):
    feats = [torch.from_numpy(f).cuda().requires_grad_(True) for f in case["feats"]]
    boxes = [torch.from_numpy(b).cuda() for b in module_boxes(TARGETS, 21)]
    pool = MultiScaleRoIAlign3D(5, 2, canonical_scale=40)
    out = torch.cat(pool(feats, boxes, IMAGE_SHAPES))
    g = torch.randn(out.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    out.backward(g)
    lhs = (out.detach().double() * g.double()).sum().item()
    rhs = sum((f.detach().double() * f.grad.double()).sum().item() for f in feats)
    assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(lhs)), (lhs, rhs)
    assert all(f.grad.abs().max().item() > 0 for f in feats)


def test_fused_forward_is_captured_in_a_graph(case):
    """Capture raises on any host synchronisation; the replay with new features AND new boxes (other levels) must give
    the bits of the eager call on those inputs."""
    rng = np.random.default_rng(5)
    static_feats = [torch.from_numpy(f).cuda() for f in case["feats"]]
    static_boxes = [torch.from_numpy(b).cuda() for b in module_boxes(TARGETS, 21)]
    pool = MultiScaleRoIAlign3D(5, 2, canonical_scale=40)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pool(static_feats, static_boxes, IMAGE_SHAPES)                       # warm-up: scales, library, allocator
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = pool(static_feats, static_boxes, IMAGE_SHAPES)
    new_feats = [torch.from_numpy(rng.normal(size=f.shape).astype(np.float32)).cuda() for f in case["feats"]]
    new_boxes = [torch.from_numpy(b).cuda() for b in module_boxes(TARGETS_B, 22)]
    for s, n in zip(static_feats + static_boxes, new_feats + new_boxes):
        s.copy_(n)
    graph.replay()
    torch.cuda.synchronize()
    eager = pool(new_feats, new_boxes, IMAGE_SHAPES)
    assert [len(t) for t in static_out] == [8, 6]
    for a, b in zip(static_out, eager):
        assert torch.equal(a, b)
    assert not torch.equal(pool.map_levels(new_boxes), pool.map_levels([torch.from_numpy(b).cuda() for b in module_boxes(TARGETS, 21)]))
