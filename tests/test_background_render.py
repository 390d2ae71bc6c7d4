"""The background sphere model through the product API, on the GPU: ``NeRFNetwork(bg_radius > 0)`` -
``background_rays`` (the fused pair as one autograd node) against the composable ``background(sph_from_ray(..), d)``,
and ``render()`` in every inference mode, staged, and in training, against a twin network built with ``bg_radius = -1``
that carries the same NeRF weights.  What must hold bit for bit: the blended image against ``twin image + (1 - ws) *
bg`` formed in torch, depth and weights_sum against the twin's, the weight gradients of the rendered loss against the
direct call's.  Tolerances are the kernel suite's: 8 x |fp32 restatement - float64| of tests/background_reference.py for
the same rays, printed beside each comparison (table gradients come from fp32 atomics: their order is not fixed)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_reference as br  # noqa: E402
from conftest import scene_rays  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, f64 = np.float32, np.float64
R = br.RADIUS


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _net(params, bg_radius, bitfield=None):
    """A NeRF with the parity parameters (table U(-1,1)); with a background model: its table U(-1,1), He weights."""
    from instance_nerf_amd.nerf import NeRFNetwork
    net = NeRFNetwork(cuda_ray=True, num_instances=0, min_near=0.05, bg_radius=bg_radius).to(DEV)
    sd = {"encoder.embeddings": params["embeddings"], "sigma_net.0.weight": params["sigma_w0"],
          "sigma_net.1.weight": params["sigma_w1"], "color_net.0.weight": params["color_w0"],
          "color_net.1.weight": params["color_w1"], "color_net.2.weight": params["color_w2"]}
    if bg_radius > 0:
        emb, w0, w1 = br.weights("upstream")
        sd.update({"encoder_bg.embeddings": emb, "bg_net.0.weight": w0, "bg_net.1.weight": w1})
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and not any(k.endswith(("embeddings", "weight")) for k in missing), (missing, unexpected)
    if bitfield is not None:
        net.density_bitfield.copy_(_t(bitfield))
    return net


def _frame_rays(room):
    from instance_nerf_amd.nerf.utils import get_rays
    poses, intr, H, W = room.cameras(n=1, H=64, W=64, focal=32.0)
    r = get_rays(_t(poses[:1]), intr, 64, 64, patch=4)
    return r["rays_o"], r["rays_d"]                     # [1, 4096, 3]


def _close(got, want, tol, what):
    got, want = got.detach(), want.detach()
    e = float((got.double() - want.double()).abs().max())
    print(f"{what}: diff {e:.3e} allowed {tol:.3e}")
    assert torch.isfinite(got).all() and e <= tol, f"{what}: diff {e:.3e} allowed {tol:.3e}"


def _bg_grads(net, o, d, G):
    params = [net.encoder_bg.embeddings, net.bg_net[0].weight, net.bg_net[1].weight]
    bg = net.background_rays(o, d)
    return bg, torch.autograd.grad((bg * G).sum(), params)


def test_fused_background_equals_the_composable_chain(params_k16):
    from instance_nerf_amd import raymarching
    net = _net(params_k16, R).train()
    o_np, d_np, miss = br.rays(4096)
    o, d, G = _t(o_np), _t(d_np), _t(br.grad_bg(4096))
    coords = raymarching.sph_from_ray(o, d, R)
    c_np = coords.cpu().numpy()
    assert np.array_equal(np.isnan(c_np).any(-1), miss)
    emb, w0, w1 = br.weights("upstream")
    tb = br.table("upstream")
    r32, r64 = br.backward(br.grad_bg(4096), c_np, d_np, emb, tb, w0, w1, f32), br.backward(br.grad_bg(4096), c_np, d_np, emb, tb, w0, w1, f64)
    tol = {k: br.tol(r32[k], r64[k]) for k in ("bg", "grad_emb", "grad_w0", "grad_w1")}
    bg_f, g_f = _bg_grads(net, o, d, G)
    assert type(bg_f.grad_fn).__name__ == "_BackgroundFnBackward"
    net.fused_background = False
    bg_c, g_c = _bg_grads(net, o, d, G)
    assert "_BackgroundFn" not in type(bg_c.grad_fn).__name__
    direct = net.background(coords, d)
    assert torch.equal(direct, bg_c)
    _close(bg_f, bg_c, tol["bg"], "background_rays against background(sph_from_ray)")
    _close(bg_f, _t(r64["bg"]), tol["bg"], "background_rays against float64")
    for k, a, b in zip(("grad_emb", "grad_w0", "grad_w1"), g_f, g_c):
        _close(a, b, tol[k], f"{k}: fused against composable")
        _close(a, _t(r64[k]), tol[k], f"{k}: fused against float64")
    # a partly frozen background: only the gradients autograd asks for come back, with the same bits
    net.fused_background = True
    net.encoder_bg.embeddings.requires_grad_(False)
    (g1,) = torch.autograd.grad((net.background_rays(o, d) * G).sum(), [net.bg_net[1].weight])
    assert torch.equal(g1, g_f[2])
    net.encoder_bg.embeddings.requires_grad_(True)
    net.fused_background = False
    with torch.no_grad():
        assert torch.equal(net.background_rays(o, d), bg_c)            # still the composable path
        net.fused_background = True
        assert torch.equal(net.background_rays(o, d), bg_f)


@pytest.mark.parametrize("mode", ["fused", "fused_terminate", "wavefront", "staged"])
def test_empty_occupancy_renders_the_background(params_k16, room, mode):
    """A fresh bit field is empty: no sample anywhere, weights_sum == 0 and the image IS the background."""
    net = _net(params_k16, R).eval()
    ro, rd = _frame_rays(room)
    kw = dict(infer_mode=mode)
    if mode == "staged":
        net.min_staged_batch = 0
        kw = dict(staged=True, max_ray_batch=1000, infer_mode="fused")          # 4 chunks of 1000 and a ragged one of 96
    with torch.no_grad():
        out = net.render(ro, rd, bg_color=0.5, **kw)
        bg = net.background_rays(ro[0], rd[0])
    assert out["image"].shape == (1, 4096, 3) and not out["weights_sum"].any()
    assert torch.equal(out["image"][0], bg)
    assert 0.01 < float(bg.std())


def test_occupied_scene_blends_over_the_twins_image(params_k16, room, room_bitfield):
    net, twin = _net(params_k16, R, room_bitfield).eval(), _net(params_k16, -1, room_bitfield).eval()
    ro, rd = _frame_rays(room)
    with torch.no_grad():
        out = net.render(ro, rd, bg_color=1, infer_mode="fused")
        ref = twin.render(ro, rd, bg_color=0, infer_mode="fused")
        bg = net.background_rays(ro[0], rd[0])
    ws = ref["weights_sum"][0]
    assert 0.05 < float(ws.mean()) < 0.999
    assert torch.equal(out["weights_sum"], ref["weights_sum"]) and torch.equal(out["depth"], ref["depth"])
    assert torch.equal(out["image"][0], ref["image"][0] + (1 - ws).unsqueeze(-1) * bg)
    # the caller's bg_color is replaced, whatever it is
    with torch.no_grad():
        assert torch.equal(net.render(ro, rd, bg_color=torch.rand(4096, 3, device=DEV), infer_mode="fused")["image"], out["image"])


def test_training_render_sends_the_blends_gradient_to_the_background(params_k16, room, room_bitfield):
    net = _net(params_k16, R, room_bitfield).train()
    o_np, d_np = scene_rays(room, n=1024)
    ro, rd = _t(o_np.astype(f32))[None], _t(d_np.astype(f32))[None]
    Gi = _t(np.random.default_rng(21).standard_normal((1, 1024, 3)).astype(f32))
    target = torch.rand(1, 1024, 3, device=DEV)
    out = net.render(ro, rd, bg_color=1, perturb=False, mse_target=target)
    assert "image_mse" not in out and out["image"].requires_grad
    params = [net.encoder_bg.embeddings, net.bg_net[0].weight, net.bg_net[1].weight]
    got = torch.autograd.grad((out["image"] * Gi).sum(), params)
    ws = out["weights_sum"].detach()[0]
    assert 0.02 < float(ws.mean()) < 0.999
    bg = net.background_rays(ro[0], rd[0])
    want = torch.autograd.grad(bg, params, grad_outputs=(1 - ws).unsqueeze(-1) * Gi[0])
    emb, w0, w1 = br.weights("upstream")
    from instance_nerf_amd import raymarching
    c_np = raymarching.sph_from_ray(ro[0], rd[0], R).cpu().numpy()
    g_np = ((1 - ws).unsqueeze(-1) * Gi[0]).cpu().numpy()
    tb = br.table("upstream")
    tol = br.tol(br.backward(g_np, c_np, d_np.astype(f32), emb, tb, w0, w1, f32)["grad_emb"],
                 br.backward(g_np, c_np, d_np.astype(f32), emb, tb, w0, w1, f64)["grad_emb"])
    _close(got[0], want[0], tol, "table gradient of the rendered loss against the direct call")
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert float(got[0].abs().max()) > 0 and float(got[1].abs().max()) > 0
    # a frozen NeRF (the instance stage) freezes the background with it
    net.freeze_nerf()
    out = net.render(ro, rd, bg_color=1, perturb=False)
    assert not out["image"].requires_grad and all(p.grad is None for p in params)
    assert torch.equal(out["weights_sum"][0], ws)


def test_trainer_leaves_the_captured_step_for_a_background_model(params_k16):
    """use_graph=True: honoured without a background model, dropped with a warning with one - and no warning where the
    captured step was off anyway (here: an optimiser of the caller's)."""
    import warnings
    from instance_nerf_amd.nerf.utils import Trainer
    kw = dict(device=torch.device(DEV), workspace=None, mute=True, use_graph=True)
    assert Trainer("plain", None, _net(params_k16, -1), **kw).use_graph is True
    with pytest.warns(RuntimeWarning, match="use_graph"):
        tr = Trainer("bg", None, _net(params_k16, R), **kw)
    assert tr.use_graph is False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr = Trainer("bg", None, _net(params_k16, R), optimizer=lambda m: torch.optim.Adam(m.get_params(1e-2)), **kw)
    assert tr.use_graph is False


def test_without_a_background_model_nothing_changes(params_k16, room, room_bitfield):
    """bg_radius = -1: one frame and one training step (render, fused loss tail, backward, optimiser step) of a network,
    and the same calls on a twin after a network WITH a background model has rendered and trained in the same process:
    the same bits.  With the default fp32-atomic scatter the table gradient depends on the order in which the atomics
    arrive, so there the loss, the image and every MLP weight's gradient and updated value are compared; with the
    order-independent int64 sums (network.FX_GRAD = 64, the form tests/test_gpu_parity.py shows to be bit-reproducible)
    every parameter after the step, the table included."""
    from instance_nerf_amd.nerf import network
    from instance_nerf_amd.nerf.utils import Trainer
    ro, rd = _frame_rays(room)
    o_np, d_np = scene_rays(room, n=1024)
    data = {"rays_o": _t(o_np.astype(f32))[None], "rays_d": _t(d_np.astype(f32))[None],
            "images": _t(np.random.default_rng(22).uniform(0, 1, (1, 1024, 3)).astype(f32))}

    def calls(bg_radius, fx):
        old_fx, network.FX_GRAD = network.FX_GRAD, fx
        try:
            net = _net(params_k16, bg_radius, room_bitfield)
            with torch.no_grad():
                frame = net.eval().render(ro, rd, bg_color=1, infer_mode="fused")
            tr = Trainer("twin", None, net, device=torch.device(DEV), workspace=None, mute=True, lr=1e-2,
                         update_extra_interval=10 ** 9)
            tr.global_step = 1                                   # (no occupancy update: the bit field stays the room's)
            net.train()
            torch.manual_seed(7)
            out = net.render(data["rays_o"], data["rays_d"], bg_color=1, perturb=True, mse_target=data["images"])
            assert ("image_mse" in out) == (bg_radius <= 0)      # the fused loss tail is still taken without a background
            torch.manual_seed(7)
            loss = tr.train_one_step(data)
            named = dict(net.named_parameters())
            assert all(p.grad is not None and bool(p.grad.abs().max() > 0) for p in named.values())
            table = lambda k: k.endswith("embeddings") and not fx          # noqa: E731
            got = {"frame." + k: frame[k] for k in ("image", "depth", "weights_sum")}
            got.update({"image": out["image"].detach(), "loss": loss})
            got.update({"grad." + k: p.grad.clone() for k, p in named.items() if not table(k)})
            got.update({"param." + k: p.detach().clone() for k, p in named.items() if not table(k)})
            return got
        finally:
            network.FX_GRAD = old_fx

    for fx in (0, 64):
        first = calls(-1, fx)
        calls(R, fx)                                             # the class is touched: a background model renders and trains
        second = calls(-1, fx)
        assert first.keys() == second.keys() and ("param.encoder.embeddings" in first) == bool(fx)
        assert not torch.equal(first["param.sigma_net.0.weight"], _t(np.asarray(params_k16["sigma_w0"])))     # the step moved it
        for k in first:
            assert torch.equal(first[k], second[k]), (fx, k)
