"""The background sphere model's kernels on the GPU, through the raw C ABI, against tests/background_reference.py:
inr_sph_from_ray, inr_grid2d_encode_forward / _backward, inr_background_forward / _backward.

What must be EXACT: which rays get NaN coordinates, which table rows a sample touches (the integer index arithmetic of
the fp32 restatement), zeros for out-of-range samples, a table row with a single contribution, coords_out against
inr_sph_from_ray, the in-place blend against the same expression in torch, the weight gradients of two calls.
Everything else is within TOL = 8 x |fp32 restatement - float64|, measured on the CPU for the same case and printed
beside each comparison (the project's rule, tests/test_composite_kernels.py).  The fused field is compared with the
float64 field FED THE KERNEL'S OWN COORDINATES: the coordinates have their own test, and the finest level (scale 2047)
would amplify the last bit of the device's atan2f.  No case is left out of a comparison; for rays that miss the sphere
the expected value is stated (NaN coordinates, zero features, bg = sigmoid(MLP([sh, 0])), no table gradient).

Every buffer a kernel writes is a view between NaN guard words; plain outputs start as the NaN pattern, accumulated
gradients as zeros.

Seen on the MI355X (largest error / allowed, N or M = 4096): sph_from_ray 1.91e-7 / 1.53e-6; upstream table: 2-D forward
2.15e-4 / 1.72e-3, scatter 4.07e-4 / 3.26e-3, fused bg 4.67e-5 / 3.74e-4, grad_emb 1.20e-2 / 9.59e-2, grad_w0 1.58e-2 /
1.26e-1, grad_w1 5.25e-4 / 4.20e-3, fused against the composable chain 9.5e-7 / 9.59e-2; small table: fused bg 1.41e-6 /
1.13e-5, grad_emb 5.71e-6 / 4.76e-5, grad_w0 1.28e-5 / 1.01e-4, grad_w1 2.42e-5 / 1.86e-4, against the composable chain
1.9e-6 / 4.76e-5.  Every figure against float64 is the fp32 restatement's own error (an eighth of the allowance): the kernels reproduce the restatement.  The upstream table's
errors are large in absolute terms because its finest level has scale 2047 - the 6e-8 resolution of x01 is 1.2e-4 of a
cell - and the test's table is U(-1, 1): that is fp32, not the kernel.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import background_reference as br  # noqa: E402
from kernel_harness import SENTINEL, Buf, check, nan_out, stream  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TABLES = ("upstream", "small")
QNAN = 0x7FC00000


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def desc(name):
    from instance_nerf_amd import _lib
    return _lib.make_grid_desc(br.table(name))


def close(got, want64, tol, what):
    """|got - want| <= tol everywhere; NaN exactly where the reference has NaN."""
    got, want64 = np.asarray(got, f64), np.asarray(want64, f64)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), f"{what}: NaN pattern differs"
    e = np.abs(got - want64)[~np.isnan(want64)]
    e = float(e.max()) if e.size else 0.0
    print(f"{what}: err {e:.3e} allowed {tol:.3e}")
    assert e <= tol, f"{what}: err {e:.3e} allowed {tol:.3e}"


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32).reshape(np.shape(got))
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


def device_coords(lib, o, d):
    N = o.shape[0]
    O, D, C = Buf(o), Buf(d), nan_out(N, 2)
    check(lib.inr_sph_from_ray(O.ptr, D.ptr, N, br.RADIUS, C.ptr, stream()), "sph_from_ray")
    C.check_guards("sph_from_ray coords")
    return C.get()


# ---------------------------------------------------------------------------- sphere coordinates
def test_sph_from_ray(lib):
    for N in br.RAY_COUNTS:
        o, d, miss = br.rays(N)
        if N == 0:
            check(lib.inr_sph_from_ray(None, None, 0, br.RADIUS, None, stream()))
            continue
        got = device_coords(lib, o, d)
        c32, c64 = br.sph_from_ray(o, d, br.RADIUS, f32), br.sph_from_ray(o, d, br.RADIUS, f64)
        assert np.array_equal(np.isnan(c64).any(-1), miss)
        assert (got.view(np.uint32)[miss] == QNAN).all(), "a missed ray's coordinates are the kernel's own NaN"
        close(got, c64, br.tol(c32, c64), f"sph_from_ray N {N}")
        assert (np.abs(got[~miss]) <= 1).all()
        if N >= 63:
            assert got[3, 0] == -1 and got[4, 0] == 1 and got[6, 1] > 0.99 and got[7, 1] < -0.99


# ---------------------------------------------------------------------------- 2-D encode
@functools.lru_cache(maxsize=None)
def samples():
    """x [4096,2]: uniform in [-1,1]^2; the first rows: out of range on either axis, NaN, the corners and edges, zero."""
    x = np.random.default_rng(11).uniform(-1, 1, (4096, 2)).astype(f32)
    head = [(1.5, 0.0), (0.0, -1.0000001), (np.nan, 0.3), (0.3, np.nan), (-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (0.0, 0.0),
            (-1.0, 0.25), (0.999999, -0.999999)]
    x[:len(head)] = np.asarray(head, f32)
    return x, 4                                    # 4 samples outside


@pytest.mark.parametrize("name", TABLES)
def test_grid2d_forward_and_the_rows_a_sample_touches(lib, name):
    tb, (emb, _, _), (x, n_out) = br.table(name), br.weights(name), samples()
    L, T = 4, int(tb["total_rows"])
    E = Buf(emb)
    for M in br.RAY_COUNTS:
        if M == 0:
            check(lib.inr_grid2d_encode_forward(None, E.ptr, desc(name), 0, 1.0, None, stream()))
            check(lib.inr_grid2d_encode_backward(None, None, desc(name), 0, 1.0, None, stream()))
            continue
        X, OUT = Buf(x[:M]), nan_out(M, 2 * L)
        check(lib.inr_grid2d_encode_forward(X.ptr, E.ptr, desc(name), M, 1.0, OUT.ptr, stream()), "grid2d forward")
        OUT.check_guards("grid2d forward")
        got = OUT.get()
        e32, e64 = br.encode2d(x[:M], emb, tb, f32), br.encode2d(x[:M], emb, tb, f64)
        close(got, e64, br.tol(e32, e64), f"grid2d forward {name} M {M}")
        outside = ~br.cells(x[:M], tb, f32)[0]
        assert outside.sum() == min(M, n_out) and (got.view(np.uint32)[outside] == 0).all()
    # rows: a one-hot gradient per level; the non-zero rows are the restatement's, as sets - over all samples at once
    # (M = 257), and sample by sample for the first 16 (the special rows among them)
    for rows_of in [slice(0, 257)] + [slice(i, i + 1) for i in range(16)]:
        xs = x[rows_of]
        M = xs.shape[0]
        inside, rows, wts = br.cells(xs, tb, f32)
        X = Buf(xs)
        for l in range(L):
            g = np.zeros((M, L, 2), f32)
            g[:, l, 0] = 1
            G, GE = Buf(g), Buf(np.zeros((T, 2), f32))
            check(lib.inr_grid2d_encode_backward(X.ptr, G.ptr, desc(name), M, 1.0, GE.ptr, stream()), "grid2d backward")
            GE.check_guards("grid2d backward")
            ge = GE.get()
            want = set(rows[:, l][(wts[:, l] != 0) & inside[:, None]].tolist())
            assert set(np.nonzero(ge[:, 0])[0].tolist()) == want, f"{name} level {l} samples {rows_of}"
            assert not ge[:, 1].any()


@pytest.mark.parametrize("name", TABLES)
def test_grid2d_scatter(lib, name):
    tb = br.table(name)
    x = np.roll(samples()[0], -6, axis=0)          # from the (1, -1) corner on; the out-of-range samples come last
    L, T = 4, int(tb["total_rows"])
    for M in (1, 65, 4096):
        g = np.random.default_rng(12 + M).standard_normal((M, 2 * L)).astype(f32)
        X, G, GE = Buf(x[:M]), Buf(g), Buf(np.zeros((T, 2), f32))
        check(lib.inr_grid2d_encode_backward(X.ptr, G.ptr, desc(name), M, 1.0, GE.ptr, stream()), "grid2d backward")
        GE.check_guards("grid2d scatter")
        ge = GE.get()
        g32, g64 = br.table_grad(x[:M], g, tb, f32), br.table_grad(x[:M], g, tb, f64)
        close(ge, g64, br.tol(g32, g64), f"grid2d scatter {name} M {M}")
        count = br.touched_rows(x[:M], g, tb)
        assert (count == 0).any() and ((count == 1).any() or name == "small")     # (224 rows: every one is shared)
        same_bits(ge[count == 1], g32[count == 1], f"rows with one contribution, {name} M {M}")
        assert (ge.view(np.uint32)[count == 0] == 0).all(), "a row nobody touches stays +0.0"
        # accumulated, not written: a second call into the same buffer doubles every single-contribution row exactly
        check(lib.inr_grid2d_encode_backward(X.ptr, G.ptr, desc(name), M, 1.0, GE.ptr, stream()), "grid2d backward")
        same_bits(GE.get()[count == 1], 2 * g32[count == 1], f"accumulation, {name} M {M}")


# ---------------------------------------------------------------------------- fused forward
@pytest.mark.parametrize("name", TABLES)
def test_background_forward(lib, name):
    tb, (emb, w0, w1) = br.table(name), br.weights(name)
    E, W0, W1 = Buf(emb), Buf(w0), Buf(w1)
    for N in br.RAY_COUNTS:
        if N == 0:
            check(lib.inr_background_forward(None, None, 0, br.RADIUS, E.ptr, desc(name), W0.ptr, W1.ptr, None, None, None,
                                             None, stream()))
            continue
        o, d, miss = br.rays(N)
        coords = device_coords(lib, o, d)
        O, D, BG, CO = Buf(o), Buf(d), nan_out(N, 3), nan_out(N, 2)
        check(lib.inr_background_forward(O.ptr, D.ptr, N, br.RADIUS, E.ptr, desc(name), W0.ptr, W1.ptr, BG.ptr, CO.ptr, None,
                                         None, stream()), "background_forward")
        for b in (BG, CO):
            b.check_guards("background_forward")
        same_bits(CO.get().view(f32), coords, f"coords_out against inr_sph_from_ray, N {N}")
        bg = BG.get()
        r32, r64 = br.field(coords, d, emb, tb, w0, w1, f32), br.field(coords, d, emb, tb, w0, w1, f64)
        close(bg, r64["bg"], br.tol(r32["bg"], r64["bg"]), f"background_forward {name} N {N}")
        assert (r64["h"][miss, br.N_SH:] == 0).all()             # a missed ray: sigmoid(MLP([sh, 0])), compared above
        # the in-place blend; without coords_out
        rng = np.random.default_rng(13 + N)
        ws, img = rng.uniform(0, 1, N).astype(f32), rng.uniform(0, 1, (N, 3)).astype(f32)
        WS, IMG, BG2 = Buf(ws), Buf(img), nan_out(N, 3)
        check(lib.inr_background_forward(O.ptr, D.ptr, N, br.RADIUS, E.ptr, desc(name), W0.ptr, W1.ptr, BG2.ptr, None, WS.ptr,
                                         IMG.ptr, stream()), "background_forward (blend)")
        for b in (WS, IMG, BG2):
            b.check_guards("background_forward (blend)")
        same_bits(BG2.get(), bg, f"bg with and without the blend, N {N}")
        want = torch.from_numpy(img).cuda() + (1 - torch.from_numpy(ws).cuda()).unsqueeze(-1) * BG2.t
        same_bits(IMG.get(), want.cpu().numpy(), f"blend, N {N}")
        same_bits(WS.get(), ws, "weights_sum is read only")


# ---------------------------------------------------------------------------- fused backward
@pytest.mark.parametrize("name", TABLES)
def test_background_backward(lib, name):
    tb, (emb, w0, w1) = br.table(name), br.weights(name)
    T = int(tb["total_rows"])
    E, W0, W1 = Buf(emb), Buf(w0), Buf(w1)
    assert lib.inr_background_workspace_bytes(-1) == -1
    for N in br.RAY_COUNTS:
        if N == 0:
            check(lib.inr_background_backward(None, None, None, 0, br.RADIUS, E.ptr, desc(name), W0.ptr, W1.ptr, None, None,
                                              None, None, stream()))
            continue
        o, d, miss = br.rays(N)
        g = br.grad_bg(N)
        coords = device_coords(lib, o, d)
        O, D, G = Buf(o), Buf(d), Buf(g)
        runs = []
        for _ in range(2):
            GE, GW0, GW1 = Buf(np.zeros((T, 2), f32)), nan_out(64, 24), nan_out(3, 64)
            WSP = nan_out(lib.inr_background_workspace_bytes(N) // 4)
            check(lib.inr_background_backward(G.ptr, O.ptr, D.ptr, N, br.RADIUS, E.ptr, desc(name), W0.ptr, W1.ptr, GE.ptr,
                                              GW0.ptr, GW1.ptr, WSP.ptr, stream()), "background_backward")
            for b in (GE, GW0, GW1, WSP):
                b.check_guards("background_backward")
            runs.append((GE.get(), GW0.get(), GW1.get()))
        same_bits(runs[1][1], runs[0][1], f"grad_w0 of two calls, N {N}")
        same_bits(runs[1][2], runs[0][2], f"grad_w1 of two calls, N {N}")
        r32, r64 = br.backward(g, coords, d, emb, tb, w0, w1, f32), br.backward(g, coords, d, emb, tb, w0, w1, f64)
        tols = {k: br.tol(r32[k], r64[k]) for k in ("grad_emb", "grad_w0", "grad_w1")}
        for k, got in zip(("grad_emb", "grad_w0", "grad_w1"), runs[0]):
            close(got, r64[k], tols[k], f"background_backward {k} {name} N {N}")
        # against the composable chain: inr_grid2d_encode_forward and inr_sh_encode_forward of the same coordinates and
        # directions, the two layers and the sigmoid as torch ops, autograd back to the encoder output, and that encoder
        # gradient through inr_grid2d_encode_backward
        X, ENC, SH = Buf(coords), nan_out(N, 8), nan_out(N, 16)
        check(lib.inr_grid2d_encode_forward(X.ptr, E.ptr, desc(name), N, 1.0, ENC.ptr, stream()), "grid2d forward")
        check(lib.inr_sh_encode_forward(D.ptr, N, 4, SH.ptr, stream()), "sh forward")
        enc = ENC.t.clone().requires_grad_(True)
        h1 = torch.relu(torch.cat([SH.t, enc], -1) @ W0.t.t())
        (denc,) = torch.autograd.grad(torch.sigmoid(h1 @ W1.t.t()), enc, grad_outputs=G.t)
        DE, GC = Buf(denc.cpu().numpy()), Buf(np.zeros((T, 2), f32))
        check(lib.inr_grid2d_encode_backward(X.ptr, DE.ptr, desc(name), N, 1.0, GC.ptr, stream()), "grid2d backward")
        for b in (ENC, SH, GC):
            b.check_guards("composable chain")
        close(runs[0][0], GC.get(), tols["grad_emb"], f"fused against the composable chain {name} N {N}")
        count = br.touched_rows(coords, r32["denc"], tb)
        assert (runs[0][0].view(np.uint32)[count == 0] == 0).all(), "a row no ray touches stays +0.0"


def test_argument_checks(lib):
    """Null pointers, negative sizes and a table of the wrong depth come back as INR_EINVAL with a message."""
    from instance_nerf_amd import _lib
    E = Buf(np.zeros((64, 2), f32))
    assert lib.inr_sph_from_ray(E.ptr, E.ptr, -1, 1.0, E.ptr, stream()) == -1 and lib.inr_last_error()
    assert lib.inr_sph_from_ray(None, E.ptr, 4, 1.0, E.ptr, stream()) == -1
    assert lib.inr_sph_from_ray(E.ptr, E.ptr, 4, 0.0, E.ptr, stream()) == -1 and b"radius" in lib.inr_last_error()
    from instance_nerf_amd.gridencoder import level_table
    d16 = _lib.make_grid_desc(level_table(num_levels=16, input_dim=2))
    rc = lib.inr_background_forward(E.ptr, E.ptr, 4, 1.0, E.ptr, d16, E.ptr, E.ptr, E.ptr, None, None, None, stream())
    assert rc == -1 and b"4-level" in lib.inr_last_error()
    rc = lib.inr_background_forward(E.ptr, E.ptr, 4, 1.0, E.ptr, desc("small"), E.ptr, E.ptr, E.ptr, None, E.ptr, None, stream())
    assert rc == -1 and b"together" in lib.inr_last_error()
    assert SENTINEL == 0x7FC0BEEF
