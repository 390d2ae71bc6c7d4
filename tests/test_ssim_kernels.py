"""The SSIM kernel on the GPU (csrc/ssim.hip), through the raw C ABI and through instance_nerf_amd.metrics / SSIMMeter,
against tests/ssim_reference.py.

Tolerance tier: map, per-image mean and squared-error sum against the float64 definition within the case's TOL = 8 x the
binary32 restatement's own error (ssim_reference.tolerance; measured on the CPU for the same inputs, printed beside each
comparison).  Exact tier: identical images give 1.0f in every map entry and in the mean; two calls, and calls with and
without the nullable outputs, return the same bits; NaN lands in exactly the map entries whose windows cover it; guard
words around every buffer the kernel writes (outputs and workspace start as a NaN pattern) are intact.

Sizes are the smallest at which each piece can go wrong, with (tw, th) = (64, 16) the tile: one window; one more row /
column; exactly one tile's patch (26 x 74) and one more / fewer in each direction; a partial second tile column
(2 tw + 11 = 139 wide); 83 x 71; 66 tile rows (more slots than the final pass has lanes).

Seen on the MI355X (largest map error against float64 / allowed, 83 x 71 x 3, B = 3): random 1.2e-6 / 9.7e-6 (40 x 37 x 4),
smooth against noisy 1.44e-4 / 1.15e-3, flat wall 1.8e-7 / 1.46e-6 - each an eighth of its allowance, i.e. the kernel
reproduces the restatement; fused against the composable path at most 3e-7; the rendered 32 x 32 views of the Trainer test
SSIM 0.415520 against 0.415520.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_reference as sr  # noqa: E402
from kernel_harness import DEV, Buf, check, nan_out, stream  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TW, TH = sr.TILE_W, sr.TILE_H
SIZES = [(11, 11), (12, 11), (11, 12), (TH + 10, TW + 10), (TH + 11, TW + 10), (TH + 9, TW + 10), (TH + 10, TW + 11),
         (TH + 10, TW + 9), (27, 2 * TW + 11), (83, 71)]
ONE = np.float32(1.0).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def window():
    from instance_nerf_amd import metrics
    return metrics.gaussian_window()


@functools.lru_cache(maxsize=None)
def case(kind, B, H, W, C, scale=1.0, L=1.0):
    x, y = sr.make_case(kind, B, H, W, C, scale=scale)
    return x, y, sr.tolerance(x, y, L)


def run(lib, x, y, L=1.0, want_map=True, want_sse=True):
    """One inr_ssim_forward through guarded, NaN-poisoned buffers -> (ssim [B], sse [B] or None, map or None)."""
    B, H, W, C = x.shape
    need = lib.inr_ssim_workspace_bytes(B, H, W, C)
    assert need == B * (-(-(H - 10) // TH)) * (-(-(W - 10) // TW)) * 16
    X, Y, R = Buf(x), Buf(y), Buf(np.array([L], f32))
    S, E, M, WS = nan_out(B), nan_out(B), nan_out(B, H - 10, W - 10, C), nan_out(need // 4)
    assert WS.ptr % 8 == 0
    check(lib.inr_ssim_forward(X.ptr, Y.ptr, B, H, W, C, window().ctypes.data, R.ptr, S.ptr, E.ptr if want_sse else None,
                               M.ptr if want_map else None, WS.ptr, need, stream()), "ssim_forward")
    for b, what in ((X, "pred"), (Y, "truth"), (R, "data_range"), (S, "ssim"), (E, "sse"), (M, "map"), (WS, "workspace")):
        b.check_guards(what)
    if not want_sse:
        assert bool((E.raw == E.whole[0]).all()), "out_sse was null and yet written"
    if not want_map:
        assert bool((M.raw == M.whole[0]).all()), "out_map was null and yet written"
    return S.get(), E.get() if want_sse else None, M.get() if want_map else None


def close(got, want64, tol, what):
    got, want64 = np.asarray(got, f64), np.asarray(want64, f64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), f"{what}: NaN pattern differs"
    e = np.abs(got - want64)[~np.isnan(want64)]
    e = float(e.max()) if e.size else 0.0
    print(f"{what}: err {e:.3e} allowed {tol:.3e}")
    assert e <= tol, f"{what}: err {e:.3e} allowed {tol:.3e}"


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


# ---------------------------------------------------------------------------- tolerance tier
@pytest.mark.parametrize("H,W", SIZES)
def test_against_the_float64_definition(lib, H, W):
    for C in (1, 2, 3, 4):
        for B in (1, 3):
            for kind in sr.KINDS:
                x, y, t = case(kind, B, H, W, C)
                ssim, sse, m = run(lib, x, y)
                what = f"{kind} B{B} {H}x{W}x{C}"
                close(m, t["map"], t["ssim"], what + " map")
                close(ssim, t["mean"], t["ssim"], what + " mean")
                close(sse, t["sse_ref"], t["sse"], what + " sse")


def test_more_slots_than_lanes_in_the_final_pass(lib):
    H, W = TH * 65 + 11, 11                                  # 66 tile rows, one window wide
    x, y, t = case("smooth_noisy", 2, H, W, 1)
    ssim, sse, m = run(lib, x, y)
    close(m, t["map"], t["ssim"], "66 slots map")
    close(ssim, t["mean"], t["ssim"], "66 slots mean")
    close(sse, t["sse_ref"], t["sse"], "66 slots sse")


def test_data_range_is_read_from_the_device(lib):
    x, y, t = case("smooth_noisy", 2, 27, 2 * TW + 11, 3)
    x255, y255, t255 = case("smooth_noisy", 2, 27, 2 * TW + 11, 3, 255.0, 255.0)
    a, b = run(lib, x, y, 1.0), run(lib, x255, y255, 255.0)
    close(b[2], t255["map"], t255["ssim"], "L = 255 map")
    close(b[0], t255["mean"], t255["ssim"], "L = 255 mean")
    # both are within their allowance of their definitions, and the definitions differ by the re-rounding of the scaled inputs
    gap = float(np.max(np.abs(t["map"] - t255["map"])))
    close(a[2], b[2], t["ssim"] + t255["ssim"] + gap, "L = 1 against L = 255 on scaled inputs")
    x3, y3, t3 = case("random", 1, 27, 19, 3, 1.0, 0.25)
    close(run(lib, x3, y3, 0.25)[2], t3["map"], t3["ssim"], "L = 0.25 map")


# ---------------------------------------------------------------------------- exact tier
@pytest.mark.parametrize("H,W,C", [(11, 11, 1), (TH + 11, TW + 11, 3), (83, 71, 4)])
def test_identical_images_give_exactly_one(lib, H, W, C):
    for kind in sr.KINDS:
        x, _ = sr.make_case(kind, 3, H, W, C)
        ssim, sse, m = run(lib, x, x.copy())
        assert np.all(m.view(np.uint32) == ONE) and np.all(ssim.view(np.uint32) == ONE) and np.all(sse == 0), kind


def test_two_calls_and_nullable_outputs_return_the_same_bits(lib):
    x, y, _ = case("random", 3, 83, 71, 3)
    a, b = run(lib, x, y), run(lib, x, y)
    for u, v, what in zip(a, b, ("ssim", "sse", "map")):
        same_bits(u, v, f"second call: {what}")
    no_map = run(lib, x, y, want_map=False)
    same_bits(no_map[0], a[0], "out_map null: ssim")
    same_bits(no_map[1], a[1], "out_map null: sse")
    no_sse = run(lib, x, y, want_sse=False)
    same_bits(no_sse[0], a[0], "out_sse null: ssim")
    same_bits(no_sse[2], a[2], "out_sse null: map")
    same_bits(run(lib, x, y, want_map=False, want_sse=False)[0], a[0], "both null: ssim")


# ---------------------------------------------------------------------------- who owns which pixel of the squared error
def test_every_pixel_is_counted_once_in_the_squared_error(lib):
    B, H, W, C = 2, 3 * TH + 3, 2 * TW + 25, 2                 # 3 x 3 tiles, the last row and column partial
    rng = np.random.default_rng(11)
    truth = rng.random((B, H, W, C)).astype(f32)
    ring = np.ones((H, W), bool)
    ring[5:-5, 5:-5] = False
    pred = truth.copy()
    pred[:, ring] += (0.25 + 0.5 * rng.random((B, int(ring.sum()), C))).astype(f32)       # every term >= 0.06
    t = sr.tolerance(pred, truth)
    ssim, sse, m = run(lib, pred, truth)
    close(sse, t["sse_ref"], t["sse"], "border ring sse")
    assert t["sse"] < 0.01                                     # one pixel dropped or doubled is >= 0.06: it cannot hide
    close(m, t["map"], t["ssim"], "border ring map")
    # equal except at the four pixels around every corner where the owned rectangles of neighbouring tiles meet
    pred = truth.copy()
    n = 0
    for r0 in range(0, H - 10, TH):
        for c0 in range(0, W - 10, TW):
            for dr in (4, 5):
                for dc in (4, 5):
                    n += 1
                    pred[:, r0 + dr, c0 + dc, :] += f32(0.25 + 0.01 * n)
    t = sr.tolerance(pred, truth)
    ssim, sse, m = run(lib, pred, truth)
    close(sse, t["sse_ref"], t["sse"], "tile corners sse")
    assert t["sse"] < 0.01
    close(ssim, t["mean"], t["ssim"], "tile corners mean")


# ---------------------------------------------------------------------------- non-finite inputs
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_pixel_poisons_exactly_its_windows(lib, bad):
    B, H, W, C = 3, 30, TW + 16, 3
    x, y, _ = case("smooth_noisy", B, H, W, C)
    for where, r, c, ch in (("pred", 12, TW + 6, 1), ("truth", 5, 5, 0), ("truth", 5 + TH, 5, 2)):    # the last two are pivots
        xb, yb = x.copy(), y.copy()
        (xb if where == "pred" else yb)[1, r, c, ch] = bad
        t = sr.tolerance(xb, yb)                   # of THESE inputs: a tile whose pivot pixel is not finite works without one
        ssim, sse, m = run(lib, xb, yb)
        want = np.zeros((B, H - 10, W - 10, C), bool)
        want[1, max(r - 10, 0):r + 1, max(c - 10, 0):c + 1, ch] = True
        assert 0 < want.sum() <= 121 and np.array_equal(np.isnan(m), want), (where, r, c, ch)
        assert np.array_equal(np.isnan(t["map"]), want)
        close(m, t["map"], t["ssim"], f"{where} ({r}, {c}, {ch}) = {bad}: the other entries")
        assert np.isnan(ssim[1]) and np.isfinite(ssim[[0, 2]]).all()
        assert (np.isnan(sse[1]) if np.isnan(bad) else np.isposinf(sse[1])) and np.isfinite(sse[[0, 2]]).all()
        close(sse[[0, 2]], t["sse_ref"][[0, 2]], t["sse"], "the other images' sse")


# ---------------------------------------------------------------------------- instance_nerf_amd.metrics on GPU tensors
def test_image_quality_fused_against_the_composable_path(lib):
    from instance_nerf_amd import metrics
    for kind in sr.KINDS:
        for B, H, W, C in ((3, 83, 71, 3), (1, 40, 37, 4), (2, 27, 2 * TW + 11, 1)):
            x, y, t = case(kind, B, H, W, C)
            X, Y = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
            fused = metrics.image_quality(X, Y, return_map=True, fused=True)
            comp = metrics.image_quality(X, Y, return_map=True, fused=False)
            what = f"{kind} B{B} {H}x{W}x{C}"
            close(fused["map"].cpu().numpy(), t["map"], t["ssim"], what + " fused map")
            close(comp["map"].cpu().numpy(), t["map"], t["ssim"], what + " composable map")
            close(fused["ssim"].cpu().numpy(), comp["ssim"].cpu().numpy(), t["ssim"], what + " fused against composable")
            close(fused["mse"].cpu().numpy().astype(f64) * (H * W * C), t["sse_ref"],
                  t["sse"] + 2.0 ** -24 * float(t["sse_ref"].max()), what + " mse")      # one more rounding: the division
            psnr = -10 * np.log10(np.maximum(t["sse_ref"] / (H * W * C), 1e-12))
            close(fused["psnr"].cpu().numpy(), psnr, 1e-4, what + " psnr")
            auto = metrics.image_quality(X, Y, return_map=True)
            pick = fused if metrics.FUSED_BY_DEFAULT else comp
            assert torch.equal(auto["map"], pick["map"]) and torch.equal(auto["ssim"], pick["ssim"])


def test_image_quality_inputs_the_kernel_does_not_take(lib):
    from instance_nerf_amd import metrics
    x, y, t = case("smooth_noisy", 2, 27, 19, 3)
    X, Y = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    a = metrics.ssim(X, Y, fused=True)
    same_bits(metrics.ssim(X[0], Y[0], fused=True).cpu().numpy(), a[:1].cpu().numpy(), "[H, W, C]")
    Xt = X.permute(0, 2, 1, 3)
    assert not Xt.is_contiguous()
    with pytest.raises(RuntimeError, match="fused"):
        metrics.ssim(Xt, Xt, fused=True)
    assert float(metrics.ssim(Xt, Xt)[0]) == 1.0                              # composable
    close(metrics.ssim(X.double(), Y.double()).cpu().numpy(), t["mean"], 1e-6, "float64 images")
    close(metrics.ssim(X.half(), Y.half()).cpu().numpy(), sr.ssim_f64(x.astype(np.float16), y.astype(np.float16))[1], 1e-4, "half")
    with pytest.raises(ValueError, match="at least 11"):
        metrics.ssim(X[:, :10], Y[:, :10])
    # more tile rows than one launch takes (65535): fused=None goes through the composable path, fused=True says why not
    tall = torch.rand((1, TH * 65535 + 11, 11, 1), device=DEV)
    assert lib.inr_ssim_workspace_bytes(*tall.shape) == -1
    assert abs(float(metrics.ssim(tall, tall.clone())[0]) - 1.0) < 1e-6
    with pytest.raises(RuntimeError, match="fused"):
        metrics.ssim(tall, tall, fused=True)


def test_data_range_none_equals_the_explicit_value_bit_for_bit(lib):
    from instance_nerf_amd import metrics
    x, y = sr.make_case("smooth_noisy", 2, 27, 2 * TW + 11, 3, scale=3.0)
    X, Y = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    L = float(sr.infer_range(x, y))
    a = metrics.image_quality(X, Y, data_range=None, return_map=True, fused=True)
    b = metrics.image_quality(X, Y, data_range=L, return_map=True, fused=True)
    same_bits(a["map"].cpu().numpy(), b["map"].cpu().numpy(), "map")
    same_bits(a["ssim"].cpu().numpy(), b["ssim"].cpu().numpy(), "ssim")
    t = sr.tolerance(x, y, None)
    close(a["map"].cpu().numpy(), t["map"], t["ssim"], "inferred range map")
    assert not torch.equal(a["ssim"], metrics.ssim(X, Y, fused=True))


# ---------------------------------------------------------------------------- SSIMMeter
def test_meter_update_does_not_read_back():
    from instance_nerf_amd import metrics
    from instance_nerf_amd.nerf.utils import SSIMMeter
    x, y, t = case("smooth_noisy", 3, 83, 71, 3)
    X, Y = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    meter = SSIMMeter(with_psnr=True)
    meter.update(X, Y)                                   # the first update allocates the sums and the cached range
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")              # any host read-back or device synchronisation raises
    try:
        meter.update(X, Y)
        meter.update(X[:1], Y[:1])
        metrics.image_quality(X, Y, data_range=None, return_map=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = float(np.concatenate([t["mean"], t["mean"], t["mean"][:1]]).mean())
    assert meter.N == 7 and abs(meter.measure() - want) <= t["ssim"]


def test_meter_through_evaluate_one_epoch(tmp_path, room):
    from instance_nerf_amd.nerf import NeRFNetwork
    from instance_nerf_amd.nerf.utils import PSNRMeter, SSIMMeter, Trainer, get_rays
    poses, intr, H, W = room.cameras(n=4, H=32, W=32, focal=16.0)

    def view(i):
        r = get_rays(torch.as_tensor(np.ascontiguousarray(poses[i:i + 1])).to(DEV), intr, H, W, N=-1)
        rgb, _, _ = room.trace(r["rays_o"][0].cpu().numpy(), r["rays_d"][0].cpu().numpy())
        return {"rays_o": r["rays_o"], "rays_d": r["rays_d"], "H": H, "W": W,
                "images": torch.as_tensor(np.ascontiguousarray(rgb)).to(DEV).view(1, H, W, 3)}

    class Recorder:
        def clear(self):
            self.seen = []

        def update(self, preds, truths):
            self.seen.append((preds.detach().clone(), truths.detach().clone()))

        def measure(self):
            return 0.0

        def report(self):
            return "recorded"

    torch.manual_seed(0)
    net = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05, num_instances=16).to(DEV)
    net.density_bitfield.copy_(torch.as_tensor(room.density_bitfield(128, 1.0)).to(DEV))
    psnr, ssim, rec = PSNRMeter(), SSIMMeter(with_psnr=True), Recorder()
    tr = Trainer("ssim", None, net, stage="nerf", device=torch.device(DEV), workspace=str(tmp_path), mute=True,
                 metrics=[psnr, ssim, rec], use_checkpoint="scratch")
    loader = [view(2), view(3)]
    tr.evaluate_one_epoch(loader)
    assert len(rec.seen) == 2 and ssim.N == 2
    ssim_value, psnr_value = ssim.measure_both()
    assert abs(psnr_value - psnr.measure()) < 1e-4
    want, tol = [], 0.0
    for p, g in rec.seen:
        assert p.shape == (1, H, W, 3) and g.shape == (1, H, W, 3)
        t = sr.tolerance(p.cpu().numpy(), g.cpu().numpy())
        want.append(t["mean"][0])
        tol = max(tol, t["ssim"])
    print(f"SSIM {ssim_value:.6f} reference {np.mean(want):.6f} allowed {tol:.3e}; {ssim.report()}")
    assert abs(ssim_value - float(np.mean(want))) <= tol
    assert ssim.report() == f"SSIM = {ssim_value:.6f}, PSNR = {psnr_value:.6f}"
