"""Error-map ray sampling on the GPU: ``inr_sample_training_batch_weighted`` (the fused weighted draw) and
``inr_error_map_update`` through the raw C ABI against tests/error_map_reference.py - every output bit for bit:
``inds_coarse``, ``inds``, ``rays_o``, ``rays_d``, rgb, labels, the updated map - and the training loop over a
device-resident ``NeRFDataset(error_map=True)``.

Every buffer a kernel writes is a view between guard words, which must come back untouched.  The shapes are the smallest
at which each part can go wrong: one cell; fewer cells than one wave; a cell count that is no power of two; the full
128 x 128 map (every thread of the workgroup owns cells) over images whose cells are wider than, as wide as and narrower
than a pixel; batch sizes of one ray, of no multiple of the wave, and of every cell.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import error_map_reference as er  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
GUARD = 64
INTR = (41.5, 40.25, 26.5, 18.5)
K_INST = 5


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded:
    """``count`` elements between two runs of guard words (int64: -7, float32: a NaN pattern)."""

    def __init__(self, count, dtype):
        self.fill = -7 if dtype == torch.int64 else float("nan")
        self.buf = torch.full((count + 2 * GUARD,), self.fill, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + count]

    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.view.data_ptr())

    def numpy(self):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]]).cpu().numpy()
        assert (np.isnan(g) if g.dtype == f32 else g == self.fill).all(), "a guard word was written"
        return self.view.cpu().numpy()


def weights_of(kind, cells, rng):
    t = cells * cells
    if kind == "ones":
        return np.ones(t, f32)
    if kind == "random":
        return rng.random(t).astype(f32) + f32(0.01)
    if kind == "span":                                      # 1e-12 .. 1e3
        return (10.0 ** rng.uniform(-12, 3, t)).astype(f32)
    if kind == "denormal":                                  # below 2^-126, mixed with ordinary weights
        w = rng.random(t).astype(f32)
        w[::3] = (rng.integers(1, 1 << 22, size=w[::3].shape[0]).astype(np.uint32)).view(f32)
        return w
    if kind in ("zeros_few", "zeros_many"):                 # positives: a quarter of the cells
        w = np.zeros(t, f32)
        pos = rng.permutation(t)[:max(t // 4, 1)]
        w[pos] = rng.random(pos.shape[0]).astype(f32) + f32(0.5)
        w[rng.permutation(t)[:3]] *= f32(-1.0)              # and a few negative ones, which count as zero
        return w
    if kind == "nan":
        w = rng.random(t).astype(f32) + f32(0.01)
        w[t // 2] = np.nan
        return w
    if kind == "inf5":
        w = rng.random(t).astype(f32) + f32(0.01)
        w[rng.permutation(t)[:5]] = np.inf
        return w
    if kind == "quadrant":                                  # all mass in the lower right quadrant of the map
        w = np.zeros((cells, cells), f32)
        w[cells // 2:, cells // 2:] = rng.random((cells - cells // 2, cells - cells // 2)).astype(f32) + f32(0.1)
        return w.reshape(-1)
    raise KeyError(kind)


def run_case(lib, cells, n, H, W, w, channels=3, with_mask=False, seed=5, step=0, rng=None):
    from instance_nerf_amd import _lib
    rng = rng or np.random.default_rng(cells * 1000 + n)
    pose = np.eye(4, dtype=f32)
    pose[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0].astype(f32)
    pose[:3, 3] = rng.normal(size=3).astype(f32)
    img = rng.random((H, W, channels)).astype(f32)
    mask = rng.integers(-1, 8, size=(H, W)).astype(np.int32) if with_mask else None
    ref = er.sample_training_batch_weighted(pose, INTR, H, W, img, mask, K_INST, w, cells, seed, step, n)
    P, I, Wt = _t(pose), _t(img), _t(w)
    Mk = _t(mask) if with_mask else None
    inds, coarse = Guarded(n, torch.int64), Guarded(n, torch.int64)
    ro, rd, rgb = Guarded(3 * n, torch.float32), Guarded(3 * n, torch.float32), Guarded(channels * n, torch.float32)
    lab = Guarded(n, torch.int64)
    _lib.check(lib.inr_sample_training_batch_weighted(
        _lib.ptr(P), *INTR, H, W, _lib.ptr(I), channels, _lib.ptr(Mk) if with_mask else None, K_INST, _lib.ptr(Wt), cells,
        seed, step, n, inds.ptr(), coarse.ptr(), ro.ptr(), rd.ptr(), rgb.ptr(), lab.ptr() if with_mask else None,
        _lib.stream_ptr()), "sample_training_batch_weighted")
    torch.cuda.synchronize()
    got = {"inds_coarse": coarse.numpy(), "inds": inds.numpy(), "rays_o": ro.numpy().reshape(n, 3),
           "rays_d": rd.numpy().reshape(n, 3), "rgb": rgb.numpy().reshape(n, channels), "labels": lab.numpy()}
    assert np.array_equal(got["inds_coarse"], ref["inds_coarse"]), "inds_coarse"
    assert np.array_equal(got["inds"], ref["inds"]), "inds"
    for k in ("rays_o", "rays_d", "rgb"):
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
    if with_mask:
        assert np.array_equal(got["labels"], ref["labels"])
        assert n < 64 or ((ref["labels"] == -1).any() and (ref["labels"] >= 0).any())      # both sides of the label rule
    else:
        assert (got["labels"] == -7).all()                  # no mask: labels are not written
    c = ref["inds_coarse"]
    assert (np.diff(c) > 0).all() and c.shape == (n,)       # ascending, distinct
    return ref


# name, cells, n, H, W, weights, channels, mask
CASES = [
    ("one_cell", 1, 1, 5, 7, "ones", 3, False),
    ("cells2_n1", 2, 1, 7, 9, "random", 3, True),
    ("cells2_n2", 2, 2, 7, 9, "span", 4, False),
    ("cells2_n3", 2, 3, 7, 9, "random", 3, False),
    ("cells2_every_cell", 2, 4, 7, 9, "zeros_few", 3, True),
    ("cells3_n5", 3, 5, 10, 11, "random", 4, True),
    ("full_800", 128, 4096, 800, 800, "random", 3, False),
    ("full_800_rgba_mask", 128, 4096, 800, 800, "span", 4, True),
    ("full_40x48_clamp", 128, 4096, 40, 48, "ones", 3, True),
    ("full_128", 128, 4096, 128, 128, "denormal", 3, False),
    ("full_every_cell", 128, 128 * 128, 128, 128, "nan", 3, False),
    ("full_n1", 128, 1, 37, 53, "random", 3, False),
    ("full_n67", 128, 67, 37, 53, "span", 3, True),
    ("cells20_n67", 20, 67, 37, 53, "denormal", 4, False),
    ("zeros_n_below_positives", 16, 40, 37, 53, "zeros_few", 3, False),
    ("zeros_n_above_positives", 16, 100, 37, 53, "zeros_many", 3, True),
    ("nan_weight", 16, 255, 37, 53, "nan", 3, False),
    ("inf5_n3", 16, 3, 37, 53, "inf5", 3, False),
    ("quadrant", 32, 200, 64, 96, "quadrant", 3, False),
]


@pytest.mark.parametrize("name,cells,n,H,W,kind,channels,with_mask", CASES, ids=[c[0] for c in CASES])
def test_weighted_draw_is_bit_exact(lib, name, cells, n, H, W, kind, channels, with_mask):
    rng = np.random.default_rng(len(name) * 131 + cells)
    w = weights_of(kind, cells, rng)
    ref = run_case(lib, cells, n, H, W, w, channels, with_mask, seed=2 ** 40 + 5 if cells == 128 else 17, step=3, rng=rng)
    c, pix = ref["inds_coarse"], ref["inds"]
    px, py = pix // W, pix % W
    # the pixel lies in its cell (to the rounding of the cell's edge) and in the image
    assert (px >= np.floor(c // cells * (H / cells)) - 1).all() and (px <= np.ceil((c // cells + 1) * (H / cells))).all()
    assert (py >= np.floor(c % cells * (W / cells)) - 1).all() and (py <= np.ceil((c % cells + 1) * (W / cells))).all()
    assert px.max() < H and py.max() < W and pix.min() >= 0
    positive = np.flatnonzero(w > 0)
    if kind == "zeros_few" and n <= positive.shape[0]:
        assert np.isin(c, positive).all()                   # no zero-weight cell is drawn
    if kind == "zeros_many":
        assert n > positive.shape[0] and np.isin(positive, c).all()
        rest = np.setdiff1d(np.arange(cells * cells), positive)
        assert np.array_equal(np.setdiff1d(c, positive), rest[:n - positive.shape[0]])     # filled in index order
    if kind == "nan" and n < cells * cells:
        assert cells * cells // 2 not in c
    if kind == "inf5":
        assert np.array_equal(c, np.flatnonzero(np.isinf(w))[:3])                           # ties: the lowest indices
    if kind == "quadrant":
        assert (px >= H // 2).all() and (py >= W // 2).all()
    if n == cells * cells:
        assert np.array_equal(c, np.arange(n))
    if name == "full_40x48_clamp":
        assert (px == H - 1).any() and (py == W - 1).any()


def test_steps_differ_and_repeat(lib):
    w = weights_of("random", 16, np.random.default_rng(1))
    a = run_case(lib, 16, 67, 37, 53, w, seed=9, step=4, rng=np.random.default_rng(2))
    b = run_case(lib, 16, 67, 37, 53, w, seed=9, step=5, rng=np.random.default_rng(2))
    again = run_case(lib, 16, 67, 37, 53, w, seed=9, step=4, rng=np.random.default_rng(2))
    other_seed = run_case(lib, 16, 67, 37, 53, w, seed=10, step=4, rng=np.random.default_rng(2))
    assert not np.array_equal(a["inds_coarse"], b["inds_coarse"]) and not np.array_equal(a["inds"], b["inds"])
    assert not np.array_equal(a["inds_coarse"], other_seed["inds_coarse"])
    for k in a:
        assert np.array_equal(a[k], again[k]), k


def test_rays_are_get_rays_for_the_drawn_pixels_and_bad_arguments_are_codes(lib):
    from instance_nerf_amd import _lib, raymarching
    from instance_nerf_amd.nerf.utils import get_rays
    rng = np.random.default_rng(3)
    pose, img = np.eye(4, dtype=f32), rng.random((37, 53, 3)).astype(f32)
    pose[:3, 3] = (0.1, 0.2, 0.3)
    w = weights_of("random", 16, rng)
    P, I, Wt = _t(pose), _t(img), _t(w)
    out = raymarching.sample_training_batch_weighted(P, INTR, 37, 53, I, None, 0, Wt, 16, 4, 2, 99)
    g = get_rays(P[None], INTR, 37, 53, inds=out["inds"])
    assert torch.equal(g["rays_d"][0], out["rays_d"]) and torch.equal(g["rays_o"][0], out["rays_o"])
    assert out["labels"] is None and torch.equal(out["rgb"], I.reshape(-1, 3)[out["inds"]])
    ref = er.sample_training_batch_weighted(pose, INTR, 37, 53, img, None, 0, w, 16, 4, 2, 99)
    assert np.array_equal(out["inds_coarse"].cpu().numpy(), ref["inds_coarse"])
    args = lambda cells, n: (_lib.ptr(P), *INTR, 37, 53, _lib.ptr(I), 3, None, 0, _lib.ptr(Wt), cells, 4, 2, n,   # noqa: E731
                             _lib.ptr(out["inds"]), _lib.ptr(out["inds_coarse"]), _lib.ptr(out["rays_o"]),
                             _lib.ptr(out["rays_d"]), _lib.ptr(out["rgb"]), None, None)
    for cells, n, needle in ((0, 1, "cells"), (129, 1, "cells"), (4, 17, "n exceeds")):
        assert lib.inr_sample_training_batch_weighted(*args(cells, n)) == -1
        assert needle in lib.inr_last_error().decode()
    assert lib.inr_sample_training_batch_weighted(*args(16, 0)) == 0


@pytest.mark.parametrize("N,cells", [(1, 1), (1, 128), (67, 16), (4096, 128)])
def test_update_is_bit_exact(lib, N, cells):
    from instance_nerf_amd import _lib
    rng = np.random.default_rng(N + cells)
    t = cells * cells
    pred, gt = rng.random((N, 3)).astype(f32), rng.random((N, 3)).astype(f32)
    row = (rng.random(t).astype(f32) + f32(0.5))
    c = np.sort(rng.permutation(t)[:N]).astype(np.int64)
    m = Guarded(t, torch.float32)
    m.view.copy_(_t(row))
    Pd, Gt, Cd = _t(pred), _t(gt), _t(c)                    # (held: a temporary's memory would be handed out again)
    _lib.check(lib.inr_error_map_update(_lib.ptr(Pd), _lib.ptr(Gt), _lib.ptr(Cd), m.ptr(), N, cells, _lib.stream_ptr()),
               "error_map_update")
    want = er.error_map_update(pred, gt, c, row)
    assert np.array_equal(m.numpy().view(np.uint32), want.view(np.uint32)) and (want != row).sum() == N


def test_update_skips_indices_outside_the_map(lib):
    from instance_nerf_amd import _lib, raymarching
    rng = np.random.default_rng(8)
    cells, t = 4, 16
    pred, gt = rng.random((6, 3)).astype(f32), rng.random((6, 3)).astype(f32)
    row = rng.random(t).astype(f32)
    for c in (np.array([-1, 16, 17, 2 ** 40, -2 ** 40, 1 << 31], np.int64), np.array([-1, 3, 16, 0, 99, 15], np.int64)):
        m = Guarded(t, torch.float32)
        m.view.copy_(_t(row))
        Pd, Gt, Cd = _t(pred), _t(gt), _t(c)
        _lib.check(lib.inr_error_map_update(_lib.ptr(Pd), _lib.ptr(Gt), _lib.ptr(Cd), m.ptr(), 6, cells, _lib.stream_ptr()),
                   "error_map_update")
        want = er.error_map_update(pred, gt, c, row)
        assert np.array_equal(m.numpy().view(np.uint32), want.view(np.uint32))
        assert (want != row).sum() == ((c >= 0) & (c < t)).sum()
    # the wrapper: shapes [1,N,3] / [1,N], a row of a 2-D map, in place
    full = _t(np.stack([row, row]))
    raymarching.error_map_update(_t(pred)[None], _t(gt)[None], _t(np.array([[5, 1, 0, 9, 2, 7]], np.int64)), full[1], cells)
    want = er.error_map_update(pred, gt, [5, 1, 0, 9, 2, 7], row)
    assert np.array_equal(full[1].cpu().numpy(), want) and np.array_equal(full[0].cpu().numpy(), row)
    assert lib.inr_error_map_update(None, None, None, None, 0, 4, None) == 0
    assert lib.inr_error_map_update(_lib.ptr(full), _lib.ptr(full), _lib.ptr(full), _lib.ptr(full), 1, 129, None) == -1


def test_training_loop_draws_from_the_map_and_updates_it(tmp_path, room):
    """A device-resident NeRFDataset(error_map=True) trained for a few eager steps: every fused batch equals the
    reference batch for the dataset's (seed, draw number) and the map as it stood, and after the step the row of the
    visited image equals the reference update applied to that step's own pred / gt; everything else stays as it was."""
    from instance_nerf_amd.nerf import NeRFNetwork
    from instance_nerf_amd.nerf.provider import NeRFDataset
    from instance_nerf_amd.nerf.utils import Trainer
    H, W, cells, n = 24, 32, 16, 128
    scene = room.write_dataset(str(tmp_path / "room"), n_views=3, H=H, W=W, num_instances=8, ignore_frac=0.25)
    ds = NeRFDataset(scene["path"], type="train", device=DEV, scale=1.0, num_rays=n, seed=11, error_map=True,
                     error_map_cells=cells)
    assert ds.error_map.is_cuda and ds.error_map.shape == (3, cells * cells)
    torch.manual_seed(0)
    net = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05, density_thresh=10)
    tr = Trainer("em", None, net, device=torch.device(DEV), workspace=None, mute=True, lr=1e-2)
    tr.train(ds.dataloader(), max_epochs=0)                 # adopts the map, as upstream's train()
    assert tr.error_map is ds.error_map
    seen = []
    step_fn = tr.train_step

    def recording(data):
        out = step_fn(data)
        seen.append((out[0].detach().clone(), out[1].detach().clone()))
        return out
    tr.train_step = recording
    for draw, idx in enumerate([1, 0, 1, 2, 1]):
        before = ds.error_map.cpu().numpy().copy()
        batch = ds[idx]
        assert batch["inds_coarse"].shape == (1, n) and batch["inds_coarse"].dtype == torch.int64
        ref = er.sample_training_batch_weighted(ds.poses[idx].cpu().numpy(), ds.intrinsics, H, W,
                                                ds.images[idx].cpu().numpy(), None, 0, before[idx], cells, 11, draw, n)
        assert np.array_equal(batch["inds_coarse"][0].cpu().numpy(), ref["inds_coarse"])
        assert np.array_equal(batch["rays_d"][0].cpu().numpy(), ref["rays_d"])
        assert np.array_equal(batch["rays_o"][0].cpu().numpy(), ref["rays_o"])
        assert np.array_equal(batch["images"][0].cpu().numpy(), ref["rgb"])
        loss = tr.train_one_step(batch)
        assert torch.isfinite(loss)
        pred, gt = seen[-1]
        want = before.copy()
        want[idx] = er.error_map_update(pred.cpu().numpy(), gt.cpu().numpy(), ref["inds_coarse"], before[idx])
        assert np.array_equal(ds.error_map.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert (want[idx] != before[idx]).sum() == n
    assert len(seen) == 5 and tr.use_graph is False
