"""Background sphere model, the part that needs no GPU: the numpy reference checks itself (its analytic gradients
against central differences in float64; its fp32 restatement against float64 - the measurement the GPU suites'
tolerances are 8 x of), and the host logic of the feature: the 2-D level table, construction of
``NeRFNetwork(bg_radius > 0)``, its state-dict keys, parameter groups, freezing, the trainer's ``use_graph`` rule and
the new exports.  The host-logic tests fail before the feature exists, except the level-table one: ``level_table``
already took ``input_dim=2``, and the test pins what the kernels now rely on."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_reference as br  # noqa: E402

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------- the reference checks itself
def _loss64(coords, d, emb, tb, w0, w1, G):
    return float((br.field(coords, d, emb, tb, w0, w1, f64)["bg"] * G).sum())


def test_reference_gradients_match_central_differences():
    """d sum(bg * G) / d (table, w0, w1) of ``backward`` (float64) against central differences, on the small table (its
    hashed levels collide, so a row's gradient is a sum over many rays)."""
    tb = br.table("small")
    emb, w0, w1 = (a.astype(f64) for a in br.weights("small"))
    o, d, _ = br.rays(65)
    coords = br.sph_from_ray(o, d, br.RADIUS, f64)
    G = br.grad_bg(65).astype(f64)
    got = br.backward(G, coords, d, emb, tb, w0, w1, f64)
    rng = np.random.default_rng(5)
    eps = 1e-6
    for name, arr, grad in (("table", emb, got["grad_emb"]), ("w0", w0, got["grad_w0"]), ("w1", w1, got["grad_w1"])):
        flat = arr.reshape(-1)
        for idx in rng.choice(flat.size, 24, replace=False):
            keep = flat[idx]
            flat[idx] = keep + eps
            up = _loss64(coords, d, emb, tb, w0, w1, G)
            flat[idx] = keep - eps
            down = _loss64(coords, d, emb, tb, w0, w1, G)
            flat[idx] = keep
            num, ana = (up - down) / (2 * eps), grad.reshape(-1)[idx]
            assert abs(num - ana) <= 1e-6 * max(1.0, abs(ana)), (name, idx, num, ana)
    assert np.abs(got["grad_emb"]).max() > 0 and np.abs(got["grad_w0"][:, br.N_SH:]).max() > 0


def test_reference_sphere_coordinates_land_on_the_sphere_and_flag_misses():
    o, d, miss = br.rays(257)
    c = br.sph_from_ray(o, d, br.RADIUS, f64)
    assert np.array_equal(np.isnan(c).any(-1), miss) and miss.sum() == br.N_MISS
    hit = ~miss
    theta, phi = (c[hit, 0] + 1) * np.pi / 2, c[hit, 1] * np.pi
    p = br.RADIUS * np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], -1)
    t = ((p - o[hit]) * d[hit]).sum(-1, keepdims=True)
    assert (t > 0).all() and np.allclose(o[hit] + t * d[hit], p, atol=1e-9)
    assert c[3, 0] == -1 and c[4, 0] == 1                       # +y / -y from the centre: the poles
    assert c[6, 1] > 0.99 and c[7, 1] < -0.99                   # either side of the seam
    c32 = br.sph_from_ray(o, d, br.RADIUS, f32)
    assert np.array_equal(np.isnan(c32), np.isnan(c)) and np.nanmax(np.abs(c32)) <= 1


@pytest.mark.parametrize("name", ["upstream", "small"])
def test_fp32_restatement_against_float64(name):
    """The measurement behind the GPU tolerances (TOL = 8 x these), printed: the fp32 restatement in the kernels'
    operation order against float64, on the largest ray set."""
    tb = br.table(name)
    emb, w0, w1 = br.weights(name)
    o, d, miss = br.rays(4096)
    c32, c64 = br.sph_from_ray(o, d, br.RADIUS, f32), br.sph_from_ray(o, d, br.RADIUS, f64)
    G = br.grad_bg(4096)
    b32 = br.backward(G, c32, d, emb, tb, w0, w1, f32)
    b64 = br.backward(G, c32, d, emb, tb, w0, w1, f64)
    err = {"coords": br.tol(c32, c64) / 8}
    for k in ("bg", "grad_emb", "grad_w0", "grad_w1"):
        err[k] = br.tol(b32[k], b64[k]) / 8
    enc32, enc64 = b32["h"][:, br.N_SH:], b64["h"][:, br.N_SH:]
    err["features"] = br.tol(enc32, enc64) / 8
    print(name, {k: f"{v:.3e}" for k, v in err.items()})
    # sanity only (the finest level's scale of 2047 turns the 6e-8 resolution of x01 into 1.2e-4 of a cell, and the table
    # is U(-1, 1): features move by ~2e-4, and everything behind them follows)
    assert 0 < err["coords"] < 1e-5 and 0 < err["bg"] < 1e-3 and 0 < err["features"] < 1e-2
    for k in ("grad_emb", "grad_w0", "grad_w1"):
        print(k, "relative", err[k] / np.abs(b64[k]).max())
        assert err[k] < 1e-2 * np.abs(b64[k]).max()
    assert (enc32[miss] == 0).all() and (enc64[miss] == 0).all()
    # a missed ray: bg = sigmoid(MLP([sh, 0])), stated, not skipped
    h = np.concatenate([br.sh4(d[miss], f64), np.zeros((br.N_MISS, 8))], -1)
    assert np.allclose(b64["bg"][miss], br.sigmoid(br.mlp(h, w0, w1, f64)[1], f64), rtol=0, atol=1e-13)
    assert np.array_equal(br.blend(np.zeros((4096, 3)), np.zeros(4096), b64["bg"], f64), b64["bg"])


# ---------------------------------------------------------------------------- host logic
def test_level_table_2d_rows_and_hashed_flags():
    up, small = br.table("upstream"), br.table("small")
    assert list(up["resolutions"]) == [16, 81, 407, 2048] and list(up["hashed"]) == [0, 0, 0, 1]
    rows = np.diff(up["offsets"].astype(np.int64))
    assert list(rows) == [296, 6728, 166464, 1 << 19] and up["total_rows"] == 697776          # 17^2 -> 296, 82^2 -> 6728, 408^2
    assert list(small["hashed"]) == [0, 1, 1, 1] and list(np.diff(small["offsets"].astype(np.int64))) == [32, 64, 64, 64]
    for tb in (up, small):
        for l in range(4):
            res1 = int(tb["resolutions"][l]) + 1
            n = int(tb["offsets"][l + 1]) - int(tb["offsets"][l])
            assert bool(tb["hashed"][l]) == (res1 * res1 > n)
            assert not tb["hashed"][l] or n & (n - 1) == 0


def test_grid_encoder_dimensions():
    from instance_nerf_amd.encoding import get_encoder
    from instance_nerf_amd.gridencoder import GridEncoder
    enc, dim = get_encoder("hashgrid", input_dim=2, num_levels=4, log2_hashmap_size=19, desired_resolution=2048)
    assert dim == 8 and enc.input_dim == 2 and tuple(enc.embeddings.shape) == (697776, 2)
    assert not getattr(enc.embeddings, "_is_hash_table", False)          # no part in the fixed-point scatter
    assert not hasattr(enc.embeddings, "_inr_split_row")
    assert getattr(GridEncoder(input_dim=3).embeddings, "_is_hash_table", False)
    with pytest.raises(RuntimeError):
        GridEncoder(input_dim=4)
    with pytest.raises(RuntimeError):
        GridEncoder(input_dim=1)


@pytest.fixture(scope="module")
def nets():
    from instance_nerf_amd.nerf.network import NeRFNetwork
    return NeRFNetwork(bg_radius=32), NeRFNetwork()


def test_network_with_a_background_model_constructs_with_upstreams_keys(nets):
    """Three extra PARAMETERS under upstream's names; the state dict carries them plus ``encoder_bg.offsets``, the
    buffer every GridEncoder (here and upstream) registers, as ``encoder.offsets`` is carried."""
    bg, plain = nets
    extra = {k: tuple(v.shape) for k, v in bg.state_dict().items() if k not in plain.state_dict()}
    assert extra == {"encoder_bg.embeddings": (697776, 2), "encoder_bg.offsets": (5,), "bg_net.0.weight": (64, 24),
                     "bg_net.1.weight": (3, 64)}
    names = {n for n, _ in bg.named_parameters()} - {n for n, _ in plain.named_parameters()}
    assert names == {"encoder_bg.embeddings", "bg_net.0.weight", "bg_net.1.weight"}
    assert list(plain.state_dict()) == [k for k in bg.state_dict() if k not in extra]
    assert bg.unfused_reason is None and bg._fusable_bg and bg.fused_background
    assert not hasattr(plain, "encoder_bg") and plain._bg_params() == []


def test_get_params_and_freeze_nerf_cover_the_background(nets):
    bg, plain = nets
    ids = {id(p) for g in bg.get_params(1e-2) for p in g["params"]}
    assert {id(p) for p in bg.parameters()} == ids and all(g["lr"] == 1e-2 for g in bg.get_params(1e-2))
    assert len(bg.get_params(1e-2)) == len(plain.get_params(1e-2)) + 2
    assert {id(p) for p in bg._bg_params()} <= {id(p) for p in bg._nerf_params()} and len(bg._bg_params()) == 3
    from instance_nerf_amd.nerf.network import NeRFNetwork
    net = NeRFNetwork(bg_radius=4, num_instances=3)
    net.freeze_nerf()
    assert not any(p.requires_grad for p in net._bg_params())
    assert all(p.requires_grad for p in net.instance_net.parameters())


def test_state_dict_without_the_background_loads_non_strictly(nets):
    bg, plain = nets
    missing, unexpected = bg.load_state_dict(plain.state_dict(), strict=False)
    assert sorted(missing) == ["bg_net.0.weight", "bg_net.1.weight", "encoder_bg.embeddings", "encoder_bg.offsets"]
    assert not unexpected
    assert plain.load_state_dict(bg.state_dict(), strict=False).missing_keys == []


def test_other_background_shapes_are_reported_as_unfused():
    from instance_nerf_amd.nerf.network import NeRFNetwork
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = NeRFNetwork(bg_radius=32, hidden_dim_bg=32)
    assert not net._fusable_bg and "background field" in net.unfused_reason and "hidden_dim_bg=32" in net.unfused_reason
    assert tuple(net.bg_net[0].weight.shape) == (32, 24)


def test_trainer_drops_use_graph_for_a_background_model(nets):
    from instance_nerf_amd.nerf.utils import Trainer
    bg, plain = nets
    """On the CPU the optimiser is torch's Adam, so the captured step is off for that reason already and nothing is said
    about the background; where it would be on, the trainer warns (tests/test_background_render.py)."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr = Trainer("bg", None, bg, device=torch.device("cpu"), workspace=None, use_graph=True)
        assert tr.use_graph is False
        assert Trainer("plain", None, plain, device=torch.device("cpu"), workspace=None, use_graph=True).use_graph is False


def test_sph_from_ray_on_the_cpu_clamps_and_flags_misses():
    from instance_nerf_amd import raymarching
    o, d, miss = br.rays(257)
    c = raymarching.sph_from_ray(torch.from_numpy(o), torch.from_numpy(d), br.RADIUS).numpy()
    want = br.sph_from_ray(o, d, br.RADIUS, f64)
    assert np.array_equal(np.isnan(c), np.isnan(want)) and np.nanmax(np.abs(c)) <= 1
    assert np.nanmax(np.abs(c - want)) < 1e-5


def test_new_exports_are_bound():
    from instance_nerf_amd import _lib, build
    for name in ("inr_grid2d_encode_forward", "inr_grid2d_encode_backward", "inr_sph_from_ray", "inr_background_forward",
                 "inr_background_workspace_bytes", "inr_background_backward"):
        assert name in _lib.EXPORTS
    assert "background.hip" in build.SOURCES and "background.hip" in build.KERNEL_FILES["background"]
    lib = _lib.load()
    assert lib.inr_background_workspace_bytes(4096) == 32 * 1728 * 4
    assert lib.inr_background_workspace_bytes(1 << 20) == 512 * 1728 * 4
    assert lib.inr_background_workspace_bytes(-1) == -1 and b"negative" in lib.inr_last_error()
