"""tests/composite_reference.py is right, and its tolerances are what was measured: the float64 restatements against
the project's fp32 sequential ones (oracle.c_port, oracle.composite) within MEASURED = TOL / 8, the closed-form
backward against torch float64 autograd at 1e-12, the slot map against raymarching.patch_slots, the exact tier's
expected values against the float64 loops, and the ambiguity cap of every tolerance-tier case - all on the CPU."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_reference as cr  # noqa: E402
import train_kernels_reference as tk  # noqa: E402

f = np.float32


@functools.lru_cache(maxsize=None)
def _regime(regime):
    c = cr.regime_case("tol", regime)
    fwd = cr.forward(c["sig"], c["rgb"], c["deltas"], c["rays"], cr.T_THRESH, c["extra"])
    keep = cr.compared_rays(c, margin=fwd["margin"])
    by_id = np.zeros(len(keep), bool)
    by_id[c["rays"][:, 0]] = keep
    rows = np.zeros(len(c["sig"]), bool)
    for n, (_, off, cnt) in enumerate(c["rays"]):
        rows[off:off + cnt] = keep[n]
    return c, fwd, by_id, rows


def _err(a, b, keep):
    a = a.detach().numpy() if hasattr(a, "detach") else a
    e = np.abs(np.asarray(a, np.float64) - b)[keep]
    return float(e.max()) if e.size else 0.0


@pytest.mark.parametrize("regime", cr.REGIMES)
def test_forward_against_the_fp32_restatements(regime):
    """c_port.composite_rays_train (scalar C, sequential) stays within MEASURED = TOL / 8 of the float64 loops on every
    output - the constants are the measurement.  oracle.composite.composite_rays_train (torch cumprod / sum, NOT
    sequential) is held to TOL: on regime s0.3 its 1024-term sums are 2.8e-6 (weights_sum) and 2.9e-5 (depth) off,
    3.5x and 2.4x the sequential C; the constants are taken from the sequential restatement alone."""
    from oracle import c_port, composite
    c, fwd, by_id, rows = _regime(regime)
    r = c_port.composite_rays_train(c["sig"], c["rgb"], c["deltas"], c["rays"], cr.T_THRESH, extra=c["extra"])
    o = composite.composite_rays_train(c["sig"], c["rgb"], c["deltas"], c["rays"], cr.T_THRESH, extra=c["extra"])
    for name, key in (("weights_sum",) * 2, ("depth",) * 2, ("image",) * 2, ("extra_out", "extra"), ("weights",) * 2):
        keep = rows if name == "weights" else by_id
        e_c, e_t = _err(r[key], fwd[name], keep), _err(o[key], fwd[name], keep)
        print(f"{regime} {name}: c_port {e_c:.3e} torch {e_t:.3e} measured {cr.MEASURED[name]:.1e}")
        assert e_c <= cr.MEASURED[name] and cr.TOL[name] == 8 * cr.MEASURED[name], (name, e_c)
        assert e_t <= cr.TOL[name], (name, e_t)


def _torch_forward64(c, n_used):
    """oracle.composite.composite_rays_train in float64 (padded cumprod), the used set given -> leaves, outputs."""
    rays = torch.as_tensor(c["rays"].astype(np.int64))
    off, cnt, rid = rays[:, 1], rays[:, 2], rays[:, 0]
    ar = torch.arange(max(int(cnt.max()), 1))[None, :]
    valid = ar < cnt[:, None]
    used = ar < torch.as_tensor(n_used)[:, None]
    idx = torch.where(valid, off[:, None] + ar, torch.zeros_like(ar))
    sig = torch.tensor(c["sig"].astype(np.float64), requires_grad=True)
    rgb = torch.tensor(c["rgb"].astype(np.float64), requires_grad=True)
    ext = torch.tensor(c["extra"].astype(np.float64), requires_grad=True)
    dl = torch.tensor(c["deltas"].astype(np.float64))
    zero = torch.zeros((), dtype=torch.float64)
    alpha = torch.where(valid, 1 - torch.exp(-sig[idx] * dl[idx, 0]), zero)
    Tincl = torch.cumprod(1 - alpha, dim=1)
    T = torch.cat([torch.ones((len(rays), 1), dtype=torch.float64), Tincl[:, :-1]], dim=1)
    w = torch.where(used, alpha * T, zero)
    N = len(rays)
    ws = torch.zeros(N, dtype=torch.float64).index_add(0, rid, w.sum(1))
    img = torch.zeros(N, 3, dtype=torch.float64).index_add(0, rid, (w[..., None] * rgb[idx]).sum(1))
    ex = torch.zeros(N, cr.KMAX, dtype=torch.float64).index_add(0, rid, (w.detach()[..., None] * ext[idx]).sum(1))
    return (sig, rgb, ext), (ws, img, ex)


@pytest.mark.parametrize("regime", cr.REGIMES)
def test_backward_is_the_gradient_and_the_fp32_closed_form_is_close(regime):
    """The float64 closed form against torch float64 autograd of sum(g_ws ws) + sum(g_img image) + sum(g_extra
    extra_out) through a float64 copy of the torch forward: 1e-12 (times the largest gradient, at least 1) - the
    closed form IS the gradient.  composite_backward_analytic (fp32, sequential, fed with c_port's fp32 forward) stays
    within MEASURED = TOL / 8.  Regime "zero": all weights are zero, grad_sigmas is not."""
    from oracle import c_port, composite
    c, fwd, by_id, rows = _regime(regime)
    gs, gc, ge = cr.backward(c["g_ws"], c["g_img"], c["sig"], c["rgb"], c["deltas"], c["rays"], fwd, c["g_extra"])
    leaves, (ws, img, ex) = _torch_forward64(c, fwd["n_used"])
    t64 = lambda a: torch.tensor(a.astype(np.float64))  # noqa: E731
    ((ws * t64(c["g_ws"])).sum() + (img * t64(c["g_img"])).sum() + (ex * t64(c["g_extra"])).sum()).backward()
    assert _err(ws, fwd["weights_sum"], slice(None)) < 1e-12 and _err(img, fwd["image"], slice(None)) < 1e-12
    for name, mine, leaf in (("grad_sigmas", gs, leaves[0]), ("grad_rgbs", gc, leaves[1]), ("grad_extra", ge, leaves[2])):
        e = _err(leaf.grad, mine, slice(None))
        assert e <= 1e-12 * max(1.0, np.abs(mine).max()), (name, e)
    if regime == "zero":
        assert not fwd["weights"].any() and np.abs(gs).max() > 1e-3
    r = c_port.composite_rays_train(c["sig"], c["rgb"], c["deltas"], c["rays"], cr.T_THRESH)
    a_s, a_c = composite.composite_backward_analytic(c["g_ws"], c["g_img"], c["sig"], c["rgb"], c["deltas"], c["rays"],
                                                     r["weights_sum"], r["image"], cr.T_THRESH)
    a_e = r["weights"][:, None] * c["g_extra"][np.maximum(fwd["sample_ray"], 0)]
    for name, got, want in (("grad_sigmas", a_s, gs), ("grad_rgbs", a_c, gc), ("grad_extra", a_e, ge)):
        e = _err(got, want, rows)
        print(f"{regime} {name}: analytic fp32 {e:.3e} measured {cr.MEASURED[name]:.1e} largest {np.abs(want).max():.2e}")
        assert e <= cr.MEASURED[name], (name, e)


@pytest.mark.parametrize("regime", cr.REGIMES)
def test_wavefront_restatement_and_ambiguity_cap(regime):
    """The fp32 run of the wavefront restatement (T = 1 - ws, sequential) stays within MEASURED = TOL / 8 of the float64
    run at n_step 1, 3, 8; the float64 run agrees with the training form (a product of transmittances) to 1e-9 where no
    ray stops early or late; the ambiguity cap holds for the training form and for every wavefront run."""
    c, fwd, by_id, _ = _regime(regime)
    for n_step in (1, 3, 8):
        w64 = cr.wavefront_reference(c, n_step, K=16)
        keep = cr.compared_rays(c, ratio=w64["ratio"])
        kid = np.zeros(len(keep), bool)
        kid[c["rays"][:, 0]] = keep
        w32 = cr.wavefront_reference(c, n_step, K=16, dtype=f)
        for name, key in (("wf_weights_sum", "weights_sum"), ("wf_depth", "depth"), ("wf_image", "image"),
                          ("wf_extra", "extra_acc"), ("wf_rays_t", "rays_t")):
            e = _err(w32[key], w64[key], kid)
            assert e <= cr.MEASURED[name] and cr.TOL[name] == 8 * cr.MEASURED[name], (name, n_step, e)
        if c["T_wavefront"] == cr.T_THRESH:
            both = kid & by_id
            assert _err(w64["weights_sum"], fwd["weights_sum"], both) < 1e-9
            assert _err(w64["image"], fwd["image"], both) < 1e-9
            assert _err(w64["extra_acc"], fwd["extra_out"][:, :16], both) < 1e-9


def _ray_sets():
    rng = np.random.default_rng(5)
    sets = {"standard": cr.ray_set("slots")[:, 2], "one ray": [7], "exactly one group": rng.integers(0, 9, 16),
            "an empty group in the middle": np.concatenate([rng.integers(1, 40, 16), np.zeros(16, int), rng.integers(0, 40, 5)]),
            "all empty": np.zeros(19, int), "ragged": rng.integers(0, 70, 37)}
    out = {}
    for k, cnt in sets.items():
        cnt = np.asarray(cnt, np.int64)
        out[k] = np.stack([rng.permutation(len(cnt)), np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt], -1).astype(np.int32)
    return out


def test_patch_slot_map_is_a_permutation_and_equals_patch_slots():
    """Ragged, empty and dropped groups: the looped slot formula gives a permutation of [0, total), every group fills
    exactly [base, base + group total) - so the groups that fit into M rows fill rows below M only - and the map equals
    raymarching.patch_slots.  skippable() on a case worked by hand."""
    from instance_nerf_amd import raymarching
    for name, rays in _ray_sets().items():
        slots = cr.patch_slot_map(rays)
        total = int(rays[:, 2].sum())
        assert sorted(slots.tolist()) == list(range(total)), name
        assert np.array_equal(slots, raymarching.patch_slots(torch.from_numpy(rays)).numpy()), name
        for g0 in range(0, len(rays), cr.GROUP):
            lo, n = int(rays[g0, 1]), int(rays[g0:g0 + cr.GROUP, 2].sum())
            mine = np.concatenate([slots[o:o + c] for _, o, c in rays[g0:g0 + cr.GROUP]] + [np.zeros(0, np.int64)])
            assert sorted(mine.tolist()) == list(range(lo, lo + n)), (name, g0)
        if total > 1:
            M = total - 1
            drop = cr.dropped_groups(rays, M)
            assert drop.any() and drop[-1] or rays[-1, 2] == 0
            a = cr.to_patch(np.arange(total), slots, M, fill=-1)
            for n, (_, o, c) in enumerate(rays):
                assert drop[n] or np.array_equal(a[slots[o:o + c]], np.arange(o, o + c)), (name, n)
    rays = np.asarray([[0, 0, 3], [1, 3, 5]], np.int32)
    assert cr.skippable(rays, np.asarray([1, 2]), 8) == 4 and cr.skippable(rays, np.asarray([1, 2]), 7) == 0
    assert cr.skippable(rays, np.asarray([3, 5]), 8) == 0


def _z(a):
    return np.asarray(a, f) + f(0.0)


@pytest.mark.parametrize("nan_behind", [False, True])
def test_one_hot_case_is_exact(nan_behind):
    """The exact tier's expected values, written down from p alone, are what the float64 loops give, a float32 round
    trip leaves them unchanged, and the same holds with NaN behind the opaque sample (never read); the fp32 AND the
    float64 wavefront runs give them too.  Every p class, a transparent ray and the +inf ray are present."""
    c = cr.one_hot_case("exact", nan_behind=nan_behind)
    rays, p = c["rays"], c["p"]
    cnt = rays[:, 2]
    for q in (0, 62, 63, 64, 65, 127, 128):
        assert (p == q).any(), q
    assert ((p == cnt - 1) & (cnt > 129)).any() and ((p < 0) & (cnt == 1024)).any() and np.isinf(c["sig"]).sum() == 1
    assert (c["sig"][np.isfinite(c["sig"])] >= 0).all() and np.isnan(c["sig"]).any() == nan_behind
    K = cr.KMAX
    want = cr.one_hot_expected(c, K)
    fwd = cr.forward(c["sig"], c["rgb"], c["deltas"], rays, cr.T_THRESH, c["extra"])
    assert (fwd["margin"] >= 1.0 - 1e-3).all() and np.array_equal(fwd["n_used"], want["n_used"])
    gs, gc, ge = cr.backward(c["g_ws"], c["g_img"], c["sig"], c["rgb"], c["deltas"], rays, fwd, c["g_extra"])
    got = dict(fwd, grad_sigmas=gs, grad_rgbs=gc, grad_extra=ge)
    for k in ("weights_sum", "depth", "image", "weights", "extra_out", "grad_sigmas", "grad_rgbs", "grad_extra"):
        assert np.array_equal(got[k].astype(f).astype(np.float64), got[k]), k         # exactly representable
        tk.assert_same_bits(_z(got[k]), _z(want[k]), k)
    assert np.array_equal(fwd["sample_ray"], want["sample_ray"]) and (want["sample_ray"] >= 0).all()
    wantw = cr.one_hot_expected(c, 16, absolute_depth=True)
    for dtype in (np.float64, f):
        for n_step in (1, 3, 8):
            w = cr.wavefront_reference(c, n_step, K=16, dtype=dtype)
            for k, kk in (("weights_sum",) * 2, ("depth",) * 2, ("image",) * 2, ("extra_acc", "extra_out")):
                tk.assert_same_bits(_z(w[k]), _z(wantw[kk]), f"wavefront {k} n_step {n_step}")
    M = cr.last_ray_dropped_M(rays)
    cut = cr.forward(c["sig"][:M], c["rgb"][:M], c["deltas"][:M], rays, cr.T_THRESH, c["extra"][:M])
    wcut = cr.one_hot_expected(c, K, M=M)
    assert cut["dropped"].sum() == 1 and cut["dropped"][-1]
    for k in ("weights_sum", "depth", "image", "weights", "extra_out"):
        tk.assert_same_bits(_z(cut[k]), _z(wcut[k]), k)
    assert np.array_equal(cut["sample_ray"], wcut["sample_ray"])


@pytest.mark.parametrize("K,n_classes", [(5, 3), (5, 5), (64, 40)])
def test_ce_rows_against_torch_fp64(K, n_classes):
    """ce_rows (float64) against F.cross_entropy in float64 over the first n_classes channels, row by row: 1e-12; the
    padded channels, the ignored rows and the row with a label outside the classes are zero, and that row is flagged.
    Its fp32 run on c_port's fp32 logits stays within MEASURED = TOL / 8 of the float64 one."""
    from oracle import c_port
    ignore = -1
    for regime in cr.REGIMES:
        c, _, by_id, _ = _regime(regime)
        ex = np.ascontiguousarray(c["extra"][:, :K])
        x = cr.forward(c["sig"], c["rgb"], c["deltas"], c["rays"], cr.T_THRESH, ex)["extra_out"]
        lab = c["labels"] % n_classes
        lab[::7] = ignore
        lab[3] = n_classes
        loss, dpix, kept, bad = cr.ce_rows(x, lab, n_classes, ignore)
        assert bad.sum() == 1 and bad[3] and not kept[::7].any() and not dpix[~kept].any() and not dpix[:, n_classes:].any()
        xt = torch.tensor(x[:, :n_classes], requires_grad=True)
        lt = torch.nn.functional.cross_entropy(xt[kept], torch.as_tensor(lab[kept]), reduction="none")
        lt.sum().backward()
        assert np.abs(lt.detach().numpy() - loss[kept]).max() < 1e-12
        assert np.abs(xt.grad.numpy() - dpix[:, :n_classes]).max() < 1e-12
        x32 = c_port.composite_rays_train(c["sig"], c["rgb"], c["deltas"], c["rays"], cr.T_THRESH, extra=ex)["extra"]
        l32, d32, k32, b32 = cr.ce_rows(x32, lab, n_classes, ignore, dtype=f)
        assert np.array_equal(k32, kept) and np.array_equal(b32, bad)
        assert _err(l32, loss, by_id) <= cr.MEASURED["ce_loss"] and _err(d32, dpix, by_id) <= cr.MEASURED["ce_dpix"]
