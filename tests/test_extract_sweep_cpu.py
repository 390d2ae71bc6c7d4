"""The composable lattice sweep of extract.py (``sweep_lattice``, under ``extract_rgbsigma`` and
``extract_instances(fused=False)``) on an analytic stub model: no GPU, no library.  The lattice reaches outside the bound
(the clamp matters), has one axis of length 1 and 35 points in chunks of 8: five chunks, the last one short, the first two
without an occupied point."""
import numpy as np
import pytest
import torch

from instance_nerf_amd import extract

BOX_MIN, BOX_MAX, RES, CHUNK, THRESH = [-1.3, -1.0, -1.0], [1.0, 1.0, 0.7], (5, 1, 7), 8, 1.0


class Stub(torch.nn.Module):
    """sigma is exactly 0 on the slab z <= -0.5 and density_scale * sigma >= THRESH exactly where x >= -0.15 above it
    (columns 2..4 of the lattice's W axis); instance() has K = 3 real columns and two padding columns that would win
    every arg-max."""
    bound, density_scale, num_instances, density_thresh = 1.0, 2.0, 3, THRESH

    def __init__(self, fail=False):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.fail = fail
        self.calls = {"density": 0, "color": 0, "instance": 0}

    def density(self, x):
        self.calls["density"] += 1
        if self.fail:
            raise RuntimeError("density failed")
        sigma = torch.where(x[:, 2] <= -0.5, torch.zeros_like(x[:, 0]), torch.exp(4.0 * x[:, 0] + 0.3 * x[:, 2] + 0.5))
        return {"sigma": sigma, "geo_feat": torch.stack([x[:, 0] * x[:, 2], torch.sin(3.0 * x[:, 0]), x[:, 2] - x[:, 1]], 1)}

    def color(self, x, d, geo_feat=None):
        self.calls["color"] += 1
        return torch.sigmoid(geo_feat + d * (1.0 + x[:, :1]))

    def instance(self, x):
        self.calls["instance"] += 1
        zero = torch.zeros_like(x[:, 0])
        return torch.stack([zero, 10.0 * (x[:, 2] - 0.2) - 50.0 * (x[:, 0] - 0.31) ** 2, 10.0 * (x[:, 0] - 0.5),
                            zero + 50.0, zero + 50.0], 1)


@pytest.fixture(scope="module")
def expected():
    """The rules of the sweep, written out on all 35 clamped points at once."""
    m = Stub()
    pts = extract.lattice(BOX_MIN, BOX_MAX, RES, "cpu").clamp(-1.0, 1.0)
    den = m.density(pts)
    rgb = sum(m.color(pts, torch.from_numpy(extract.VIEW_DIRS[v]).expand(35, 3), geo_feat=den["geo_feat"]) for v in range(4)) / 4
    occ = den["sigma"] * m.density_scale >= THRESH
    arg = torch.argmax(m.instance(pts)[:, :3], 1).to(torch.uint8)
    return {"logit": torch.log(den["sigma"].clamp_min(1e-30)).view(RES), "rgb": rgb.view(*RES, 3),
            "labels": torch.where(occ, arg, torch.full_like(arg, extract.LABEL_EMPTY)).view(RES)}


def test_rgbsigma_through_the_sweep(expected):
    m = Stub().train()
    grid, res = extract.extract_rgbsigma(m, BOX_MIN, BOX_MAX, res=RES, chunk=CHUNK)
    assert tuple(grid.shape) == RES + (4,) and res.tolist() == list(RES)
    assert torch.equal(grid[..., 3], expected["logit"])
    assert float(grid[..., 3].min()) == float(np.float32(np.log(np.float32(1e-30))))           # the slab: sigma = 0
    assert (grid[..., :3] - expected["rgb"]).abs().max() <= 1e-6
    assert m.calls == {"density": 5, "color": 20, "instance": 0}
    assert m.training


def test_instances_through_the_sweep(expected):
    m = Stub().train()
    r = extract.extract_instances(m, BOX_MIN, BOX_MAX, res=RES, sigma_thresh=THRESH, fused=False, chunk=CHUNK)
    assert r["labels"].dtype == torch.uint8 and torch.equal(r["labels"], expected["labels"])
    assert r["counts"].tolist() == [8, 2, 5]
    assert bool(((r["confidence"] > 0) == (r["labels"] != extract.LABEL_EMPTY)).all())
    assert m.calls == {"density": 5, "color": 0, "instance": 3}           # two chunks have no occupied point
    assert m.training


@pytest.mark.parametrize("call", [
    lambda m: extract.extract_rgbsigma(m, BOX_MIN, BOX_MAX, res=RES, chunk=CHUNK),
    lambda m: extract.extract_instances(m, BOX_MIN, BOX_MAX, res=RES, sigma_thresh=THRESH, fused=False, chunk=CHUNK)],
    ids=["extract_rgbsigma", "extract_instances"])
def test_training_mode_is_restored_when_density_raises(call):
    m = Stub(fail=True).train()
    with pytest.raises(RuntimeError, match="density failed"):
        call(m)
    assert m.training and m.calls["density"] == 1


def test_one_sweep_for_rgb_and_labels_evaluates_density_once_per_chunk(expected):
    m = Stub()
    logit, rgb, labels, conf = extract.sweep_lattice(m, np.float32(BOX_MIN), np.float32(BOX_MAX), RES, CHUNK, want_rgb=True,
                                                     thresh=THRESH)
    assert m.calls == {"density": 5, "color": 20, "instance": 3}
    assert torch.equal(logit, expected["logit"]) and torch.equal(labels, expected["labels"])
    assert (rgb[..., :3] - expected["rgb"]).abs().max() <= 1e-6 and tuple(conf.shape) == RES
