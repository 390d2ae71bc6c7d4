"""tests/field_backward_reference.py checked on the CPU: the float64 restatements against torch float64 autograd, the
SH column order against oracle.sh, the arithmetic models within TOL / 8 (so the constants cannot drift from the
measurement), unambiguity and acceptance rate of the tolerance tier, the exact tier's preconditions, and that every
size class and every K is present."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_backward_reference as R  # noqa: E402

F32, F64 = np.float32, np.float64
CUS = R.NOMINAL_CUS


@functools.lru_cache(maxsize=None)
def cases():
    """(id, size, case) of both case lists on a NOMINAL_CUS device."""
    out = [(cid, spec[3], make(CUS)) for (cid, make), spec in zip(R.nerf_cases(), R._nerf_specs())]
    return out + [(cid, spec[2], make(CUS)) for (cid, make), spec in zip(R.instance_cases(), R._instance_specs())]


@functools.lru_cache(maxsize=None)
def measured():
    """build -> list of (size, measure_case(...)) over the tolerance tier."""
    return {b: [(size, R.measure_case(b, size, c, CUS)) for _, size, c in cases() if c["tier"] == "tol"] for b in R.BUILDS}


class _TruncExp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        return g * torch.exp(ctx.saved_tensors[0].clamp(-15, 15))


def _close(got, want, what):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, what
    assert np.abs(got - want).max(initial=0.0) <= 1e-12 * max(np.abs(want).max(initial=0.0), 1e-300), what


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, F64), requires_grad=grad)


def test_nerf_reference_equals_autograd():
    from train_kernels_reference import sh64
    for M, ds in ((129, 0.5), (17, 1.0)):
        c = R.nerf_tol_case(M, 0, ds)
        enc, W = _t(c["enc"], True), [_t(w, True) for w in c["W"]]
        h1 = torch.relu(enc @ W[0].t())
        so = h1 @ W[1].t()
        cin = torch.cat([_t(sh64(c["dirs"], 4)), so[:, 1:]], 1)
        c2 = torch.relu(torch.relu(cin @ W[2].t()) @ W[3].t())
        rgb = torch.sigmoid(c2 @ W[4].t())
        sigma = ds * _TruncExp.apply(so[:, 0])
        ((sigma * _t(c["g_sigma"])).sum() + (rgb * _t(c["g_rgb"])).sum()).backward()
        out, _, f, _ = R.nerf_head(R.Exact64(), c)
        assert (np.abs(f["so"][:, 0]) > 15).any()
        _close(f["rgb"], rgb.detach().numpy(), "rgb")
        _close(f["so"], so.detach().numpy(), "so")
        _close(out["d_enc"], enc.grad.numpy(), "d_enc")
        for k, w in zip(("gws0", "gws1", "gwc0", "gwc1"), W):
            _close(out[k], w.grad.numpy(), k)
        _close(out["gwc2"][:3], W[4].grad.numpy(), "gwc2")
        assert not out["gwc2"][3:].any() and out["gwc0"].shape == (64, 31)


def test_instance_reference_equals_autograd():
    for M, K, scales, n in ((129, 48, (0.37, 3.0), 92), (17, 16, (None, None), None), (40, 64, (None, 2.5), 45)):
        c = R.instance_tol_case(M, K, 0, scales, n)
        rows = R.instance_rows(c)
        enc, W = _t(c["enc"], True), [_t(w, True) for w in c["W"]]
        logits = torch.relu(torch.relu(enc @ W[0].t()) @ W[1].t()) @ W[2].t()
        a, b = (1.0 if s is None else float(F32(s)) for s in scales)
        w = _t(c["wbuf"]) * (a * b)
        g = _t(c["g_pix"])[torch.from_numpy(c["sample_ray"]).long()] * w[:, None]
        (logits[:rows] * g[:rows]).sum().backward()
        out, _, _ = R.instance_head(R.Exact64(), c)
        _close(out["d_enc"], enc.grad.numpy(), "d_enc")
        assert rows == M or not out["d_enc"][rows:].any()
        for k, wt in zip(("gw0", "gw1", "gw2"), W):
            _close(out[k], wt.grad.numpy(), k)


def test_chain_reference_equals_the_head_reference():
    """The chain functions on the head's own float64 activations give the head's d_enc (one code path, two entries)."""
    c = R.nerf_tol_case(33)
    out, _, f, (ch, _) = R.nerf_head(R.Exact64(), c)
    got, _ = R.chain_reference(R.Exact64(), c, {k: f[k] for k in ("rgb", "so", "h1", "c1", "c2")})
    assert all((got[k] == ch[k]).all() for k in got) and (got["d_enc"] == out["d_enc"]).all()
    assert got["d_o"].shape == (33, 4) and not got["d_o"][:, 3].any()


def test_sh_column_order_is_the_oracles():
    from oracle.sh import sh_encode
    d = R.nerf_tol_case(64)["dirs"]
    f = R.nerf_forward(R.Exact64(), np.zeros((64, 32)), d, R.nerf_weights(R._rng("w")))
    want = sh_encode(torch.from_numpy(d), 4).numpy().astype(F64)
    assert np.abs(f["cin"][:, :16] - want).max() < 1e-6 and f["cin"].shape == (64, 31)


def test_models_stay_within_the_measured_constants():
    for b in R.BUILDS:
        worst, big = {}, {}
        for size, (w, _, _) in measured()[b]:
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0.0), v)
                if size in R.BIG_SIZES:
                    big[k] = max(big.get(k, 0.0), v)
        print(b, "overall", {k: f"{v:.3e}" for k, v in sorted(worst.items())})
        print(b, "multi-round sizes", {k: f"{v:.3e}" for k, v in sorted(big.items())})
        assert set(worst) == set(R.MEASURED[b]) and set(big) == set(R.MEASURED_BIG[b])
        for k, v in worst.items():
            assert v <= R.MEASURED[b][k] == R.TOL[b][k] / 8, (b, k, v)
            assert v > 0.2 * R.MEASURED[b][k], (b, k, v, "the constant is stale")
        for k, v in big.items():
            assert v <= R.MEASURED_BIG[b][k] <= R.MEASURED[b][k], (b, k, v)
            assert R.tolerance(b, k, "16R+1") == 8 * R.MEASURED_BIG[b][k] and R.tolerance(b, k, 17) == R.TOL[b][k]


def test_tolerance_tier_is_unambiguous():
    """Every hidden pre-activation is exactly 0 or at least MARGIN * (|x| @ |W|^T) away from 0; MARGIN is at least 8 x
    the models' pre-activation error; both models reproduce the float64 masks; acceptance above 50 %; an all-zero enc
    row in every case; so0 beyond +-15 on both sides."""
    for b in R.BUILDS:
        assert all(same for _, (_, _, same) in measured()[b])
        assert 8 * max(pre for _, (_, pre, _) in measured()[b]) <= R.MARGIN
    n_tol = 0
    for cid, size, c in cases():
        if c["tier"] != "tol":
            continue
        n_tol += 1
        assert c["rate"] > 0.5, (cid, c["rate"])
        M = len(c["enc"])
        if c["kind"] == "nerf":
            f, names = R.nerf_forward(R.Exact64(), c["enc"], c["dirs"], c["W"]), ("h1", "c1", "c2")
            if M >= 127:
                assert (f["so"][:, 0] > 15).any() and (f["so"][:, 0] < -15).any(), cid
        else:
            f, names = R.instance_forward(R.Exact64(), c["enc"], c["W"]), ("h1", "h2")
        for nme in names:
            p, nrm = f["p_" + nme], f["n_" + nme]
            assert ((p == 0) | (np.abs(p) >= R.MARGIN * nrm)).all(), (cid, nme)
        if M:
            zero = ~np.asarray(c["enc"]).any(1)
            assert zero.any() and not f["h1"][zero].any(), cid
    assert n_tol >= 2 * len(R.SIZES)


def test_exact_tier_preconditions():
    """<= 16 significant bits into every product, <= 8 on one side, sum |terms| < 2^24 quanta; so0 and the colour logits
    exactly 0; the float64 result is an fp32 number; the tier is not vacuous (gradients flow where the variant says,
    the 12-bit variants fill the remainder planes)."""
    seen = set()
    for cid, size, c in cases():
        if c["tier"] != "exact":
            continue
        log = []
        res = R.head_of(c)(R.Exact64(log), c, CUS)
        out, f = res[0], res[2]
        assert R.exactness_violations(log) == [], cid
        for k, v in out.items():
            v = v[:, 16:] if k == "gwc0" else v              # the SH columns are compared in the tolerance tier only
            assert (v.astype(F32).astype(F64) == v).all(), (cid, k)
        M = len(c["enc"])
        if c["kind"] == "nerf":
            assert not f["so"][:, 0].any() and not f["o"].any() and (f["rgb"] == 0.5).all(), cid
            assert not c["W"][2][:, :16].any()
            if M >= 15:
                live = {k for k, v in out.items() if v.any()}
                want = {"a": {"d_enc", "gws0", "gws1", "gwc2"}, "b": {"d_enc", "gws0", "gws1", "gwc2", "gwc1"},
                        "c": {"d_enc", "gws0", "gws1", "gwc2", "gwc1", "gwc0"}}[c["variant"]]
                assert live == want, (cid, live)
                if c["variant"] == "c":
                    assert res[3][0]["d_so"][:, 1:].any() and res[3][0]["dz_c1"].any()
            seen.add(("nerf", c["variant"], size))
        else:
            if M >= 15 and R.instance_rows(c):
                assert all(v.any() for v in out.values()), cid
            seen.add(("instance", c["K"], size))
        if size == 150:                                     # the 12-bit variants: some operand needs its remainder plane
            assert max(R.sigbits(A) for _, A, _ in log) > 8 or max(R.sigbits(B) for _, _, B in log) > 8, cid
            wide_w = any(k == "layer" and R.sigbits(A) > 8 for k, A, _ in log)
            wide_x = any(k == "layer" and R.sigbits(B) > 8 for k, _, B in log)
            wide_g = any(k == "wgrad" and R.sigbits(A) > 8 for k, A, _ in log)
            wide_s = any(k == "wgrad" and R.sigbits(B) > 8 for k, _, B in log)
            seen.add(("planes", wide_w, wide_x, wide_g, wide_s))
    planes = [s[1:] for s in seen if s[0] == "planes"]
    assert all(any(p[i] for p in planes) for i in range(4)), planes      # weights, activations, staged G, staged X


def test_every_size_class_and_every_k_is_present():
    for kind, specs, at in (("nerf", R._nerf_specs(), 3), ("instance", R._instance_specs(), 2)):
        for tier in ("exact", "tol"):
            assert {s[at] for s in specs if s[0] == tier} >= set(R.SIZES), (kind, tier)
    for tier in ("exact", "tol"):
        assert {s[3] for s in R._instance_specs() if s[0] == tier} == set(R.KS)
    inst = R._instance_specs()
    assert {s[5] for s in inst} >= {None, "M-37", 0, "M+5"} and {s[4] != (None, None) for s in inst} == {True, False}
    assert {s[4] for s in R._nerf_specs()} == {1.0, 0.5}
    assert R.resolve("16R-5", 256) == 32763 and R.resolve("16R+1", 256) == 32769 and R.resolve("32R+151", 256) == 65687
    N, ray = R._rays(R._rng("r"), 500)
    assert ray.min() >= 0 and ray.max() < N and (np.diff(ray) < 0).any() and len(set(range(N)) - set(ray.tolist())) > 0
