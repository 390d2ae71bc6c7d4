"""SSIM without a GPU: the window, known answers of the float64 definition (tests/ssim_reference.py), its cross-check
against scipy, the binary32 restatement's own error (which IS the tolerance of every comparison, here and in
tests/test_ssim_kernels.py), the composable torch path of instance_nerf_amd.metrics on CPU tensors, SSIMMeter, and the
argument validation of the two exports (tests/ssim_abi_child.py).

Tolerance: per case TOL = 8 x max |binary32 restatement - float64 definition| over the map (never below 8 half-ulps of
a binary32 near 1, ssim_reference.tolerance); printed per case.  The restatement's largest map error seen here (40 x 37,
C = 3, data_range 1 / 255 on inputs scaled by 255 / 0.25): random 1.1e-6 / 1.1e-6 / 1.2e-6, smooth against noisy 7.8e-5 /
1.2e-4 / 1.2e-4, flat 0.7 against 0.7 + 1e-3 noise 1.6e-7 / 1.7e-7 / 1.8e-6 - the pivot removes the cancellation that
made the flat case 2.3e-4 in a prototype without it; the smooth case varies by 0.8 across a tile, so no single pivot helps
it, and its error sits where the truth is locally flat and 2 cov + C2 is small.

One known answer is restated: all-ones against all-zeros gives C1 / (1 + C1) only for a window that sums to exactly 1.
The eleven binary32 values of the contract sum to 1 - 1.4e-9, so the exact answer is the closed form in S = (sum g)^2
below; it is asserted to float64 rounding, and its distance from C1 / (1 + C1) is bounded from |S - 1|.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe  # noqa: E402
import ssim_reference as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SIZES = [(11, 11), (12, 11), (11, 12), (27, 19), (40, 37)]


# ---------------------------------------------------------------------------- window
def test_window_is_the_contract():
    from instance_nerf_amd import metrics
    g = metrics.gaussian_window()
    assert g.dtype == np.float32 and g.shape == (11,)
    assert abs(float(g.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23
    assert np.array_equal(g, g[::-1])
    i = np.arange(11, dtype=np.float64)
    want = np.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2))
    want = (want / want.sum()).astype(np.float32)
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(g.view(np.uint32), sr.window32().view(np.uint32))
    assert metrics.TILE == (sr.TILE_W, sr.TILE_H)


# ---------------------------------------------------------------------------- known answers of the definition
def test_identical_images_give_exactly_one():
    for kind in sr.KINDS:
        x, _ = sr.make_case(kind, 2, 27, 19, 3)
        m32, mean32, sse32 = sr.ssim_f32(x, x)
        assert np.all(m32 == np.float32(1.0)) and np.all(mean32 == np.float32(1.0)) and np.all(sse32 == 0)
        m64, mean64, _ = sr.ssim_f64(x, x)
        assert np.max(np.abs(m64 - 1.0)) < 1e-9


def test_ones_against_zeros():
    L = 1.0
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    m, mean, sse = sr.ssim_f64(np.ones((1, 20, 23, 2), np.float32), np.zeros((1, 20, 23, 2), np.float32))
    S = float(sr.window32().astype(np.float64).sum()) ** 2                # the 2-D window's sum: mu_x = E[x^2] = S
    exact = (C1 * C2) / ((S * S + C1) * ((S - S * S) + C2))
    assert np.max(np.abs(m - exact)) <= 4e-16 * 32                         # float64 rounding of 22-term sums
    # |d SSIM / d S| at S = 1 is below C1 (2 + 1 / C2) < 0.12
    assert abs(exact - C1 / (1 + C1)) <= 0.12 * abs(S - 1) + 1e-15 and abs(S - 1) < 2.0 ** -28
    assert sse[0] == 20 * 23 * 2


def test_one_window_against_a_direct_121_term_sum():
    x, y = sr.make_case("random", 1, 11, 11, 1)
    g = sr.window32().astype(np.float64)
    w2 = np.outer(g, g)
    X, Y = x[0, :, :, 0].astype(np.float64), y[0, :, :, 0].astype(np.float64)
    mx, my = (w2 * X).sum(), (w2 * Y).sum()
    vx, vy, cov = (w2 * X * X).sum() - mx * mx, (w2 * Y * Y).sum() - my * my, (w2 * X * Y).sum() - mx * my
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    want = ((2 * mx * my + C1) * (2 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    m, mean, sse = sr.ssim_f64(x, y)
    assert m.shape == (1, 1, 1, 1)
    assert abs(m[0, 0, 0, 0] - want) < 1e-12 and abs(mean[0] - want) < 1e-12
    assert abs(sse[0] - ((X - Y) ** 2).sum()) < 1e-12


def test_symmetry_and_scaling():
    x, y = sr.make_case("smooth_noisy", 2, 27, 19, 3)
    a, b = sr.ssim_f64(x, y), sr.ssim_f64(y, x)
    assert np.max(np.abs(a[0] - b[0])) < 1e-12 and np.array_equal(a[2], b[2])
    x255, y255 = (x.astype(np.float64) * 255).astype(np.float32), (y.astype(np.float64) * 255).astype(np.float32)
    c = sr.ssim_f64(x255, y255, 255.0)
    # inputs are re-rounded to binary32 after the scaling: 2^-24 relative per pixel, amplified by at most 1 / C2-scale terms
    assert np.max(np.abs(a[0] - c[0])) < 1e-4
    exact = sr.ssim_f64(x.astype(np.float64) * 255, y.astype(np.float64) * 255, 255.0)      # no re-rounding: rounding only
    assert np.max(np.abs(sr.ssim_f64(x.astype(np.float64), y.astype(np.float64))[0] - exact[0])) < 1e-10


def test_against_scipy_correlate1d():
    from scipy import ndimage
    x, y = sr.make_case("random", 1, 40, 37, 3)
    g = sr.window32().astype(np.float64)

    def windowed(a):
        a = ndimage.correlate1d(ndimage.correlate1d(a, g, axis=1, mode="reflect"), g, axis=2, mode="reflect")
        return a[:, 5:-5, 5:-5]

    X, Y = x.astype(np.float64), y.astype(np.float64)
    mx, my = windowed(X), windowed(Y)
    vx, vy, cov = windowed(X * X) - mx * mx, windowed(Y * Y) - my * my, windowed(X * Y) - mx * my
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    want = ((2 * mx * my + C1) * (2 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    assert np.max(np.abs(sr.ssim_f64(x, y)[0] - want)) < 1e-11


# ---------------------------------------------------------------------------- the restatement's own error = the tolerance
@pytest.mark.parametrize("kind", sr.KINDS)
def test_restatement_error_is_small_and_not_zero(kind):
    for scale, L in ((1.0, 1.0), (255.0, 255.0), (1.0, 0.25)):
        x, y = sr.make_case(kind, 1, 40, 37, 3, scale=scale)
        assert L >= 0.25 * max(np.abs(x).max(), np.abs(y).max()) * (1 - 1e-6)       # the tolerance tier's condition
        t = sr.tolerance(x, y, L)
        print(f"{kind} scale {scale} L {L}: map error {t['map_error']:.3e} mean error {t['mean_error']:.3e} "
              f"TOL {t['ssim']:.3e} sse TOL {t['sse']:.3e}")
        assert 2.0 ** -24 < t["map_error"] < 1e-3 and t["ssim"] == 8 * t["map_error"]
        assert t["mean_error"] <= t["map_error"]
        assert t["sse"] > 0


def test_restatement_propagates_non_finite_values_like_the_definition():
    x, y = sr.make_case("random", 2, 30, 80, 2)
    x[1, 12, 70, 1] = np.nan
    y[0, 5, 5, 0] = np.inf                     # the first tile's pivot pixel
    m64, mean64, sse64 = sr.ssim_f64(x, y)
    m32, mean32, sse32 = sr.ssim_f32(x, y)
    assert np.array_equal(np.isnan(m64), np.isnan(m32))
    assert int(np.isnan(m32[1]).sum()) == 11 * 10 and not np.isnan(m32[1, :, :, 0]).any()     # column 70 of 80: 10 windows wide
    assert int(np.isnan(m32[0]).sum()) == 6 * 6 and not np.isnan(m32[0, :, :, 1]).any()
    assert np.isnan(mean32).all() and np.isnan(sse32[1]) and np.isinf(sse32[0])


# ---------------------------------------------------------------------------- the composable path on CPU tensors
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("B", [1, 3])
def test_composable_path_on_cpu(B, H, W, C):
    from instance_nerf_amd import metrics
    for kind in sr.KINDS:
        x, y = sr.make_case(kind, B, H, W, C)
        t = sr.tolerance(x, y, 1.0)
        q = metrics.image_quality(torch.from_numpy(x), torch.from_numpy(y), return_map=True)
        assert q["map"].shape == (B, H - 10, W - 10, C) and q["ssim"].shape == (B,) and q["ssim"].dtype == torch.float32
        e_map = float(np.max(np.abs(q["map"].numpy().astype(np.float64) - t["map"])))
        e_mean = float(np.max(np.abs(q["ssim"].numpy().astype(np.float64) - t["mean"])))
        e_sse = float(np.max(np.abs(q["mse"].numpy().astype(np.float64) * (H * W * C) - t["sse_ref"])))
        print(f"{kind} B{B} {H}x{W}x{C}: map {e_map:.3e} mean {e_mean:.3e} allowed {t['ssim']:.3e}; sse {e_sse:.3e} allowed {t['sse']:.3e}")
        assert t["map_error"] < 1e-3 and e_map <= t["ssim"] and e_mean <= t["ssim"]
        # mse is sse / (H W C) rounded once more to binary32: one more half ulp on top of the sum's allowance
        assert e_sse <= t["sse"] + 2.0 ** -24 * float(np.max(t["sse_ref"]))
        psnr = -10 * np.log10(np.maximum(t["sse_ref"] / (H * W * C), 1e-12))
        assert np.max(np.abs(q["psnr"].numpy() - psnr)) < 1e-4


def test_composable_path_shapes_dtypes_and_errors():
    from instance_nerf_amd import metrics
    x, y = sr.make_case("smooth_noisy", 1, 27, 19, 3)
    X, Y = torch.from_numpy(x), torch.from_numpy(y)
    a = metrics.ssim(X, Y)
    assert torch.equal(metrics.ssim(X[0], Y[0]), a) and a.shape == (1,)
    assert torch.equal(metrics.image_quality(X, Y, fused=False)["ssim"], a)
    d = metrics.ssim(X.double(), Y.double())
    assert abs(float(d[0]) - sr.ssim_f64(x, y)[1][0]) < 1e-6               # float64 images are worked in float64
    x6, y6 = sr.make_case("random", 1, 12, 13, 6)                           # C > 4: the composable path takes it
    assert abs(float(metrics.ssim(torch.from_numpy(x6), torch.from_numpy(y6))[0]) - sr.ssim_f64(x6, y6)[1][0]) < 1e-4
    xt = torch.from_numpy(x).permute(0, 2, 1, 3)                            # non-contiguous
    assert not xt.is_contiguous() and metrics.ssim(xt, xt)[0] == 1.0
    with pytest.raises(ValueError, match="at least 11"):
        metrics.ssim(torch.zeros(1, 10, 20, 3), torch.zeros(1, 10, 20, 3))
    with pytest.raises(ValueError, match="at least 11"):
        metrics.ssim(torch.zeros(20, 10, 3), torch.zeros(20, 10, 3))
    with pytest.raises(ValueError, match="same shape"):
        metrics.ssim(torch.zeros(1, 20, 20, 3), torch.zeros(1, 20, 21, 3))
    with pytest.raises(RuntimeError, match="fused"):
        metrics.ssim(X, Y, fused=True)                                      # CPU tensors: never a quiet other path


def test_data_range_none_is_the_inferred_value():
    from instance_nerf_amd import metrics
    x, y = sr.make_case("smooth_noisy", 2, 27, 19, 3, scale=3.0)
    X, Y = torch.from_numpy(x), torch.from_numpy(y)
    L = float(sr.infer_range(x, y))
    assert L == max(float(x.max() - x.min()), float(y.max() - y.min()))
    a, b = metrics.image_quality(X, Y, data_range=None, return_map=True), metrics.image_quality(X, Y, data_range=L, return_map=True)
    assert torch.equal(a["map"], b["map"]) and torch.equal(a["ssim"], b["ssim"])
    assert not torch.equal(a["ssim"], metrics.ssim(X, Y))


# ---------------------------------------------------------------------------- SSIMMeter
def test_ssim_meter_on_cpu_tensors():
    from instance_nerf_amd import metrics
    from instance_nerf_amd.nerf.utils import PSNRMeter, SSIMMeter
    updates = [sr.make_case(kind, B, 27, 19, 3, seed=7) for kind, B in (("random", 1), ("smooth_noisy", 3), ("flat_noise", 2))]
    meter, psnr = SSIMMeter(with_psnr=True), PSNRMeter()
    per_image = []
    for x, y in updates:
        X, Y = torch.from_numpy(x), torch.from_numpy(y)
        meter.update(X, Y)
        psnr.update(X, Y)
        per_image += metrics.ssim(X, Y).tolist()
    assert len(per_image) == 6 and abs(meter.measure() - float(np.mean(per_image))) < 1e-7
    # the same rule on the same mse; the two mse differ by binary32 rounding (2^-23 relative: 10 log10(e) 2^-23 = 5e-7 dB each)
    ssim_value, psnr_value = meter.measure_both()
    assert abs(psnr_value - psnr.measure()) < 5e-6
    assert meter.report() == f"SSIM = {ssim_value:.6f}, PSNR = {psnr_value:.6f}"
    plain = SSIMMeter()
    plain.update(torch.from_numpy(updates[0][0][0]), torch.from_numpy(updates[0][1][0]))          # [H, W, C]
    assert abs(plain.measure() - per_image[0]) < 1e-7 and plain.report() == f"SSIM = {plain.measure():.6f}"
    meter.clear()
    assert meter.N == 0 and meter.measure() == 0.0
    meter.update(torch.from_numpy(updates[1][0]), torch.from_numpy(updates[1][1]))
    assert abs(meter.measure() - float(np.mean(per_image[1:4]))) < 1e-7
    with pytest.raises(ValueError, match="'H' and 'W'"):
        plain.update(torch.zeros(1, 27 * 19, 3), torch.zeros(1, 27 * 19, 3))


def test_ssim_meter_data_range():
    from instance_nerf_amd.nerf.utils import SSIMMeter
    x, y = sr.make_case("smooth_noisy", 2, 27, 19, 3, scale=3.0)
    X, Y = torch.from_numpy(x), torch.from_numpy(y)
    a, b = SSIMMeter(data_range=None), SSIMMeter(data_range=float(sr.infer_range(x, y)))
    a.update(X, Y)
    b.update(X, Y)
    assert a.measure() == b.measure() and abs(a.measure() - float(sr.ssim_f64(x, y, None)[1].mean())) < 1e-5


# ---------------------------------------------------------------------------- the C ABI's targeted cases
@pytest.fixture(scope="module")
def abi():
    return abi_probe.run_abi_child("ssim_abi_child.py", env=abi_probe.NO_GPU)


@pytest.mark.parametrize("case,needle", [
    ("inr_ssim_forward:C_5", "C must"), ("inr_ssim_forward:C_0", "C must"), ("inr_ssim_forward:H_10", "H must"),
    ("inr_ssim_forward:W_10", "W must"), ("inr_ssim_forward:B_0", "B must"), ("inr_ssim_forward:too_large", "2^31"),
    ("inr_ssim_forward:workspace_one_byte_short", "workspace too small"),
    ("inr_ssim_forward:workspace_misaligned", "misaligned"), ("inr_ssim_forward:workspace_null", "null"),
    ("inr_ssim_forward:pred_null", "null"), ("inr_ssim_forward:window_null", "null"),
    ("inr_ssim_forward:data_range_null", "null"), ("inr_ssim_forward:out_ssim_null", "null"),
    ("inr_ssim_forward:window_nan", "window11"),
    ("inr_ssim_workspace_bytes:C_5", "C must"), ("inr_ssim_workspace_bytes:H_10", "H must"),
    ("inr_ssim_workspace_bytes:W_negative", "W must"), ("inr_ssim_workspace_bytes:too_large", "2^31"),
])
def test_abi_rejects_the_named_argument(abi, case, needle):
    rc, msg = abi[case]
    assert rc == EINVAL and needle in msg, (case, rc, msg)


def test_abi_workspace_size(abi):
    # slots = tile rows x tile columns per image, two binary64 each
    assert abi["size:1x11x11x1"] == 16 and abi["size:3x26x74x4"] == 3 * 16 and abi["size:1x27x75x3"] == 4 * 16
    assert abi["size:8x800x800x3"] == 8 * 50 * 13 * 16
