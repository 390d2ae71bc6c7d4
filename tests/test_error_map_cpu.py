"""Error-map ray sampling (upstream's --error_map) without a GPU: the two properties of the numpy restatement the GPU
tests compare the kernels with (tests/error_map_reference.py) - the accuracy of its fp32 ``-ln(u)`` sequence and the
distribution of its draw - and the wiring of ``NeRFDataset(error_map=True)`` and ``Trainer`` on CPU tensors, where the
draw is ``get_rays(error_map=...)`` and the update upstream's tensor expression."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import error_map_reference as er  # noqa: E402


def test_neg_ln_sequence_is_accurate_for_every_u():
    """All 2^24 values of u = (m + 0.5) * 2^-24 against float64 -log(u).  The cap is 1e-4 relative (a weight distorted
    by 0.01 % is far below what an average of fp32 losses resolves); the measured maximum is asserted as an upper bound
    with no margin, because the run is deterministic."""
    m = np.arange(1 << 24, dtype=np.int64)
    got = er.neg_ln_u24(m)
    assert got.dtype == np.float32 and np.isfinite(got).all() and (got > 0).all()
    exact = -np.log((m + 0.5) / 2.0 ** 24)
    rel = float((np.abs(got.astype(np.float64) - exact) / exact).max())
    print("max relative error of neg_ln_u24:", repr(rel))
    assert rel < 1e-4
    assert rel <= er.MEASURED_MAX_REL_ERR


def _pair_counts(weights, seed=20261020, steps=20000):
    kb = er.keys(np.asarray(weights, np.float32), seed, np.arange(steps))
    assert kb.shape == (steps, 4)
    won = np.stack([er.select(row, 2) for row in kb])
    batched = np.sort(np.argsort(kb, axis=1, kind="stable")[:, :2], axis=1)
    assert np.array_equal(won, batched)
    return {(i, j): int(((won[:, 0] == i) & (won[:, 1] == j)).sum()) for i in range(4) for j in range(i + 1, 4)}


@pytest.mark.parametrize("weights", [(1, 2, 3, 4), (1, 1, 1, 1)])
def test_draw_has_the_distribution_of_sampling_without_replacement(weights):
    """cells = 2, n = 2, steps 0..19999 of one seed: the six pairs appear with the frequencies of sequential sampling
    without replacement, P{i,j} = w_i w_j / (1 - w_i) + w_i w_j / (1 - w_j) on normalised weights (1/6 each for uniform
    weights).  Pearson's statistic stays below 25.7, the 1e-4 quantile of chi^2 with 5 degrees of freedom; the seed is
    part of the test, so the outcome is deterministic."""
    steps = 20000
    counts = _pair_counts(weights, steps=steps)
    assert sum(counts.values()) == steps
    p = np.asarray(weights, np.float64) / np.sum(weights)
    chi2 = 0.0
    for (i, j), obs in counts.items():
        want = steps * (p[i] * p[j] / (1 - p[i]) + p[i] * p[j] / (1 - p[j]))
        if len(set(weights)) == 1:
            assert abs(want - steps / 6) < 1e-9
        chi2 += (obs - want) ** 2 / want
    print("weights", weights, "counts", counts, "chi2", chi2)
    assert chi2 < 25.7


def test_selection_rules_of_the_restatement():
    """Bad weights last and in index order, +inf weights first, equal keys to the smaller index, output ascending."""
    w = np.array([0.0, 3.0, -1.0, np.nan, 2.0, np.inf, 1e-30, np.inf], np.float32)
    kb = er.keys(w, 7, 3)
    assert (kb[[0, 2, 3]] == 0x7F800000).all() and (kb[[5, 7]] == 0).all() and (kb[[1, 4, 6]] < 0x7F800000).all()
    assert er.select(kb, 1).tolist() == [5] and er.select(kb, 2).tolist() == [5, 7]
    assert sorted(er.select(kb, 5).tolist()) == [1, 4, 5, 6, 7]
    assert er.select(kb, 6).tolist() == [0, 1, 4, 5, 6, 7] and er.select(kb, 7).tolist() == [0, 1, 2, 4, 5, 6, 7]
    assert er.select(kb, 8).tolist() == list(range(8))
    assert not np.array_equal(er.keys(w, 7, 4), kb) and np.array_equal(er.keys(w, 7, 3), kb)


def _write_scene(root, n=3, H=12, W=16):
    from PIL import Image
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    rng = np.random.default_rng(0)
    frames = []
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(os.path.join(root, "images", f"{i:04d}.png"))
        T = np.eye(4)
        T[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        T[:3, 3] = rng.normal(size=3)
        frames.append({"file_path": f"images/{i:04d}", "transform_matrix": T.tolist()})
    for split in ("train", "test"):
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911, "frames": frames}, f)
    return str(root)


class _ToyField(torch.nn.Module):
    """The least a Trainer needs of a model: parameters, ``get_params`` and a differentiable ``render`` -> image."""
    cuda_ray = False

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, 3)

    def get_params(self, lr):
        return [{"params": list(self.parameters()), "lr": lr}]

    def render(self, rays_o, rays_d, **kwargs):
        return {"image": torch.sigmoid(self.lin(rays_d))}


def _trainer(**kw):
    from instance_nerf_amd.nerf.utils import Trainer
    return Trainer("t", None, _ToyField(), device=torch.device("cpu"), workspace=None, mute=True, **kw)


def test_dataset_owns_a_map_and_batches_carry_inds_coarse(tmp_path):
    from argparse import Namespace
    from instance_nerf_amd.nerf.provider import NeRFDataset
    root = _write_scene(tmp_path)
    cells, H, W = 8, 12, 16
    ds = NeRFDataset(root, type="train", num_rays=20, error_map=True, error_map_cells=cells)
    assert ds.error_map.shape == (3, cells * cells) and ds.error_map.dtype == torch.float32
    assert ds.error_map.device == ds.device and bool((ds.error_map == 1).all())
    b = ds[1]
    coarse, n = b["inds_coarse"], 20
    assert coarse.shape == (1, n) and coarse.dtype == torch.int64 and len(set(coarse[0].tolist())) == n
    assert b["rays_o"].shape == (1, n, 3) and b["images"].shape == (1, n, 3) and b["index"] == [1]
    # every pixel lies inside its coarse cell, and the colours are those of the drawn pixels
    img = ds.images[1].reshape(-1, 3)
    match = (b["images"][0][:, None, :] == img[None]).all(-1)                   # [n, H*W]
    cx_, cy_ = coarse[0] // cells, coarse[0] % cells
    rows, cols = torch.arange(H * W) // W, torch.arange(H * W) % W
    inside = ((rows[None] >= torch.floor(cx_[:, None] * (H / cells))) & (rows[None] < (cx_[:, None] + 1) * (H / cells))
              & (cols[None] >= torch.floor(cy_[:, None] * (W / cells))) & (cols[None] < (cy_[:, None] + 1) * (W / cells)))
    assert bool((match & inside).any(-1).all())
    # off by default; evaluation datasets never get a map; upstream's opt form reads opt.error_map
    off = NeRFDataset(root, type="train", num_rays=20)
    assert off.error_map is None and "inds_coarse" not in off[0]
    assert NeRFDataset(root, type="test", error_map=True).error_map is None
    opt = Namespace(path=root, num_rays=20, error_map=True)
    assert NeRFDataset(opt, "cpu").error_map.shape == (3, 128 * 128)
    assert NeRFDataset(Namespace(path=root, num_rays=20), "cpu").error_map is None


def test_num_rays_above_the_cell_count_raises(tmp_path):
    from instance_nerf_amd.nerf.provider import NeRFDataset
    root = _write_scene(tmp_path)
    with pytest.raises(ValueError, match="num_rays"):
        NeRFDataset(root, type="train", num_rays=65, error_map=True, error_map_cells=8)
    with pytest.raises(ValueError, match="num_rays"):
        NeRFDataset(root, type="train", num_rays=128 * 128 + 1, error_map=True)
    assert NeRFDataset(root, type="train", num_rays=64, error_map=True, error_map_cells=8).error_map is not None
    with pytest.raises(ValueError, match="error_map_cells"):
        NeRFDataset(root, type="train", num_rays=4, error_map=True, error_map_cells=129)


def test_train_step_folds_the_loss_into_the_visited_cells(tmp_path):
    from instance_nerf_amd.nerf.provider import NeRFDataset
    root = _write_scene(tmp_path)
    ds = NeRFDataset(root, type="train", num_rays=20, error_map=True, error_map_cells=8)
    tr = _trainer()
    assert tr.error_map is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr.train(ds.dataloader(), max_epochs=0)                    # adopts the map, as upstream's train()
    assert tr.error_map is ds.error_map
    b = ds[1]
    pred, gt, _ = tr.train_step(b)
    coarse = b["inds_coarse"][0]
    want = 0.1 * torch.ones(20) + 0.9 * torch.nn.MSELoss(reduction="none")(pred.detach(), gt).mean(-1).reshape(-1)
    assert torch.equal(ds.error_map[1][coarse], want) and bool((want != 1).all())
    untouched = torch.ones(64, dtype=torch.bool)
    untouched[coarse] = False
    assert bool((ds.error_map[1][untouched] == 1).all()) and bool((ds.error_map[[0, 2]] == 1).all())
    # a whole optimisation step goes through the same update, with a criterion of the caller's as well
    tr2 = _trainer(criterion=torch.nn.L1Loss(reduction="none"))
    tr2.error_map = ds.error_map
    b2 = ds[2]
    lin = [p.detach().clone() for p in tr2.model.parameters()]
    with torch.no_grad():
        pred2 = tr2.model.render(b2["rays_o"], b2["rays_d"])["image"]
    tr2.train_one_step(b2)
    want2 = 0.1 + 0.9 * (pred2 - b2["images"]).abs().mean(-1).reshape(-1)
    assert torch.equal(ds.error_map[2][b2["inds_coarse"][0]], want2)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(lin, tr2.model.parameters()))     # and the step was taken
    assert bool((ds.error_map[0] == 1).all())


def test_without_the_switch_nothing_changes(tmp_path):
    from instance_nerf_amd.nerf.provider import NeRFDataset
    root = _write_scene(tmp_path)
    ds = NeRFDataset(root, type="train", num_rays=20)
    tr = _trainer()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr.train(ds.dataloader(), max_epochs=1)
    assert tr.error_map is None and ds.error_map is None
    assert set(ds[0]) == {"H", "W", "rays_o", "rays_d", "index", "images"}


def test_instance_stage_and_use_graph_warn(tmp_path):
    from instance_nerf_amd.nerf.provider import NeRFDataset
    from instance_nerf_amd.nerf.utils import Trainer
    root = _write_scene(tmp_path)
    ds = NeRFDataset(root, type="train", num_rays=20, error_map=True, error_map_cells=8)
    tr = _trainer(use_graph=True)
    with pytest.warns(RuntimeWarning, match="use_graph=True is not available with an error map"):
        tr.train(ds.dataloader(), max_epochs=1)
    assert tr.use_graph is False and tr.error_map is ds.error_map
    assert bool((ds.error_map != 1).any())                         # and it trained on the eager step
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr.train(ds.dataloader(), max_epochs=1)                    # said once

    class _Frozen(_ToyField):
        def freeze_nerf(self):
            pass

        def render(self, rays_o, rays_d, **kwargs):
            return {"instance": self.lin(rays_d)}
    ds2 = NeRFDataset(root, type="train", num_rays=20, error_map=True, error_map_cells=8)
    inst = Trainer("i", None, _Frozen(), stage="instance", device=torch.device("cpu"), workspace=None, mute=True)
    with pytest.warns(RuntimeWarning, match="only updated in stage 'nerf'"):
        inst.train(ds2.dataloader(), max_epochs=0)
    b = ds2[0]
    b["masks"] = torch.zeros(1, 20, dtype=torch.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        inst.train_one_step(b)                                     # warned once; the map is left alone
    assert bool((ds2.error_map == 1).all())
