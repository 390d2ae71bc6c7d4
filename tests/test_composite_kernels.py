"""The compositing kernels of csrc/raymarch.hip on the GPU against tests/composite_reference.py, through the raw C ABI:
k_composite_train_fwd / _bwd, k_composite_train_extra_fwd (with its fused cross entropy) / _extra_bwd,
k_composite_patch_fwd / _extra and k_composite_rays.

Two tiers.  EXACT: inputs on which every weight is 0 or 1 and every sum is exact in any order (one_hot_case) - outputs
and gradients must equal the values written down from the position of the opaque sample, bit for bit (the sign of a
zero aside: the expected values say "zero").  TOLERANCE: four density regimes against float64, each output within
TOL[name] = 8 x the error of the project's fp32 sequential restatement (measured on the CPU, composite_reference.py),
rays whose termination is ambiguous in fp32 left out (at most one of 51, asserted on the CPU).

Every ray set holds 0, 1, 2, 15 .. 17, 63 .. 65, 127 .. 129, 191 .. 193, 511 and 1024 samples (both sides of every
64-sample chunk boundary, a third and a sixteenth chunk) three times over, shuffled, ids permuted: 51 rays, a ragged
last 16-ray group, groups mixing empty and long rays.  Every buffer a kernel writes is a view inside a larger allocation
with NaN-pattern guard words on both sides (Buf of kernel_harness.py) and starts out as that NaN pattern wherever
the kernel has to write it: a row it skips, or a guard it touches, fails the test.

Seen on an MI355X (each comparison prints its own figure): the forward's weights_sum 5.5e-6 of 6.2e-6 allowed, depth 6.3e-5
of 1.0e-4, image 3.0e-6 of 6.1e-6 (regime s0.3, 1024-sample rays: alpha = 1 - expf(-x) at x ~ 1e-3 carries the device
expf's last-bit error of a value near 1, and 1024 of them add up; the sequential wavefront kernel shows the same 5.6e-6);
grad_sigmas 4.9e-8 of 1.44e-7; everything else below a fifth of its bound.  What the tests are known to catch: the colour
carry between chunks of k_composite_train_bwd zeroed (tolerance tier, regimes s0.3 and s40: grad_sigmas), its
g_ws * (1 - ws) term dropped (both tiers), the zero store behind the termination point of k_composite_patch_fwd removed
(both tiers), 0 * NaN from a sample behind the termination point reaching a sum (exact tier, "nan").  The exact tier
alone cannot see a lost colour carry: before the opaque sample every weight is zero."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_reference as cr  # noqa: E402
import train_kernels_reference as tk  # noqa: E402
from kernel_harness import SENTINEL, Buf, check, finish, nan_out, stream  # noqa: E402

pytestmark = pytest.mark.gpu
f = np.float32
T = cr.T_THRESH


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------- cases and expected values
@functools.lru_cache(maxsize=None)
def _exact_case(variant):
    return cr.one_hot_case("exact", nan_behind=variant == "nan")


@functools.lru_cache(maxsize=None)
def _tol_case(regime):
    """case, float64 outputs and gradients (64 channels), compared rays by id [N] and by sample row [M]."""
    c = cr.regime_case("tol", regime)
    fwd = cr.forward(c["sig"], c["rgb"], c["deltas"], c["rays"], T, c["extra"])
    gs, gc, ge = cr.backward(c["g_ws"], c["g_img"], c["sig"], c["rgb"], c["deltas"], c["rays"], fwd, c["g_extra"])
    want = dict(fwd, grad_sigmas=gs, grad_rgbs=gc, grad_extra=ge)
    keep = cr.compared_rays(c, margin=fwd["margin"])
    ids = np.zeros(len(keep), bool)
    ids[c["rays"][:, 0]] = keep
    return c, want, ids, _rows_of(c["rays"], keep, len(c["sig"]))


def _rows_of(rays, ray_mask, M):
    """bool [M]: rows owned by the rays (rows of ``rays``) that ray_mask selects and that fit into M."""
    rows = np.zeros(M, bool)
    for n, (_, off, cnt) in enumerate(rays):
        if ray_mask[n] and off + cnt <= M:
            rows[off:off + cnt] = True
    return rows


class Exact:
    """Bit for bit against one_hot_expected; K channels; M rows (rays beyond are dropped)."""

    def __init__(self, variant, K=0, M=None, absolute_depth=False):
        self.c = _exact_case(variant)
        self.want = cr.one_hot_expected(self.c, K, M=M, absolute_depth=absolute_depth)
        self.K = K
        self.what = f"exact/{variant}/K{K}/M{M}"

    def cmp(self, name, got, tolname=None, want=None, ids=None, rows=None):
        want = self.want[name] if want is None else want
        got = np.asarray(got)
        want = np.asarray(want).reshape(got.shape)
        if ids is not None:
            got, want = got[ids], want[ids]
        if rows is not None:
            got, want = got[rows], want[rows]
        if got.dtype == f:
            got, want = got + f(0.0), want.astype(f) + f(0.0)
        tk.assert_same_bits(got, want.astype(got.dtype), f"{self.what} {name}")


class Close:
    """Within TOL of the float64 reference, over the compared rays."""

    def __init__(self, regime, K=0):
        self.c, want, self.ids, self.rows = _tol_case(regime)
        self.want = dict(want)
        for k in ("extra_out", "grad_extra"):
            self.want[k] = want[k][:, :K]
        self.K = K
        self.what = f"tol/{regime}/K{K}"

    def cmp(self, name, got, tolname=None, want=None, ids=None, rows=None):
        want = self.want[name] if want is None else want
        got = np.asarray(got)
        want = np.asarray(want).reshape(got.shape)
        keep = self.ids if got.shape[0] == len(self.ids) else self.rows
        if len(keep) < got.shape[0]:                 # padding rows behind the samples: compared too (they must be zero)
            keep = np.concatenate([keep, np.ones(got.shape[0] - len(keep), bool)])
        for extra_mask in (ids, rows):
            if extra_mask is not None:
                keep = keep & extra_mask
        if got.dtype != f:
            assert np.array_equal(got[keep], want[keep]), f"{self.what} {name}"
            return
        tol = cr.TOL[tolname or name]
        assert np.isfinite(got[keep]).all(), f"{self.what} {name}: not finite"
        e = np.abs(got.astype(np.float64) - want)[keep]
        e = float(e.max()) if e.size else 0.0
        print(f"{self.what} {name}: err {e:.3e} allowed {tol:.2e}")
        assert e <= tol, f"{self.what} {name}: err {e:.3e} allowed {tol:.2e}"


def _pad(a, M, K=None):
    """M rows of ``a`` (its first K columns); rows beyond its end hold NaN - no ray owns them, nothing reads them."""
    a = a if K is None else a[:, :K]
    if M > len(a):
        a = np.concatenate([a, np.full((M - len(a),) + a.shape[1:], np.nan, a.dtype)])
    return np.ascontiguousarray(a[:M])


def _fresh(shape, dtype=f, written=None):
    """An output buffer: the NaN pattern where the kernel must write (everywhere, or the rows of ``written``), zero -
    the caller's fill - elsewhere."""
    if written is None:
        return nan_out(*np.atleast_1d(shape), dtype=dtype)
    b = Buf(np.zeros(shape, dtype))
    b.t[torch.from_numpy(written).to(b.t.device)] = float("nan") if dtype == f else -7
    return b


def _finish(ins, out, what):
    """Guards of inputs and outputs alike -> the outputs' contents, None for an output that was not asked for."""
    got = finish(dict(ins, **out), what)
    return {k: got.get(k) for k in out}


def _ptr(b):
    return None if b is None else b.ptr


# ---------------------------------------------------------------------------- launches
def run_forward(lib, c, M, K, weights=True):
    N = len(c["rays"])
    ins = dict(sig=Buf(_pad(c["sig"], M)), rgb=Buf(_pad(c["rgb"], M)), dl=Buf(_pad(c["deltas"], M)), rays=Buf(c["rays"]),
               ex=Buf(_pad(c["extra"], M, K)) if K else None)
    assert ins["dl"].ptr % 8 == 0
    out = dict(weights_sum=_fresh(N), depth=_fresh(N), image=_fresh((N, 3)), extra_out=_fresh((N, K)) if K else None,
               weights=_fresh(M) if (weights or K) else None, sample_ray=_fresh(M, np.int32) if weights else None)
    check(lib.inr_composite_rays_train_forward(ins["sig"].ptr, ins["rgb"].ptr, ins["dl"].ptr, ins["rays"].ptr, N, M, T,
                                               _ptr(ins["ex"]), K, out["weights_sum"].ptr, out["depth"].ptr,
                                               out["image"].ptr, _ptr(out["extra_out"]), _ptr(out["weights"]),
                                               _ptr(out["sample_ray"]), stream()), "composite_rays_train_forward")
    return _finish(ins, out, "forward")


def run_backward(lib, c, M, K, fwd, total=None, field=True, with_g_ws=True):
    """``fwd``: weights_sum, image, weights as the kernels take them (fp32).  ``total``: the marcher's sample total
    (the launch then writes EVERY row itself); None: rows no live ray owns are the caller's zeros."""
    N, rays = len(c["rays"]), c["rays"]
    owned = _rows_of(rays, np.ones(N, bool), M)
    ins = dict(sig=Buf(_pad(c["sig"], M)), rgb=Buf(_pad(c["rgb"], M)), dl=Buf(_pad(c["deltas"], M)), rays=Buf(rays),
               g_ws=Buf(c["g_ws"]) if with_g_ws else None, g_img=Buf(c["g_img"]),
               g_ex=Buf(np.ascontiguousarray(c["g_extra"][:, :K])) if K else None,
               ws=Buf(np.asarray(fwd["weights_sum"], f)), img=Buf(np.asarray(fwd["image"], f)),
               w=Buf(np.asarray(fwd["weights"], f)[:M]) if K else None,
               total=Buf(np.asarray([total], np.int32)) if total is not None else None)
    every = None if total is not None else owned
    out = dict(grad_sigmas=_fresh(M, written=every) if field else None,
               grad_rgbs=_fresh((M, 3), written=every) if field else None,
               grad_extra=_fresh((M, K), written=owned) if K else None)
    check(lib.inr_composite_rays_train_backward(
        _ptr(ins["g_ws"]) if field else None, ins["g_img"].ptr if field else None, _ptr(ins["g_ex"]), ins["sig"].ptr,
        ins["rgb"].ptr, None, ins["dl"].ptr, ins["rays"].ptr, ins["ws"].ptr, ins["img"].ptr, _ptr(ins["w"]), N, M, T, K,
        _ptr(out["grad_sigmas"]), _ptr(out["grad_rgbs"]), _ptr(out["grad_extra"]), _ptr(ins["total"]), stream()),
        "composite_rays_train_backward")
    return _finish(ins, out, "backward")


def run_extra_ce(lib, c, K, weights, labels=None, n_classes=0, ignore_index=-1):
    """inr_composite_rays_extra_forward: the K channels from given weights, with the cross-entropy rows when labelled."""
    N, M = len(c["rays"]), len(c["sig"])
    ins = dict(w=Buf(np.asarray(weights, f)), ex=Buf(_pad(c["extra"], M, K)), rays=Buf(c["rays"]),
               labels=None if labels is None else Buf(np.ascontiguousarray(labels, np.int64).view(np.int32)))
    out = dict(extra_out=_fresh((N, K)))
    if labels is not None:
        out.update(dpix=_fresh((N, K)), part=_fresh((N, 4)), loss=_fresh(4))
        assert out["part"].ptr % 16 == 0 and ins["labels"].ptr % 8 == 0
    check(lib.inr_composite_rays_extra_forward(ins["w"].ptr, ins["ex"].ptr, ins["rays"].ptr, N, M, K, out["extra_out"].ptr,
                                               _ptr(ins["labels"]), n_classes, ignore_index, _ptr(out.get("dpix")),
                                               _ptr(out.get("part")), _ptr(out.get("loss")), stream()),
          "composite_rays_extra_forward")
    return _finish(ins, out, "extra forward")


@functools.lru_cache(maxsize=None)
def _slots(ray_bytes, N):
    return cr.patch_slot_map(np.frombuffer(ray_bytes, np.int32).reshape(N, 3))


def run_patch(lib, c, M, K, weights=True, hide=None):
    """The case in the patch-interleaved layout, built with composite_reference.patch_slot_map.  ``hide`` bool [N by
    row]: the samples of those rays (dropped groups) are NaN, deltas included.  -> outputs, weights in patch rows."""
    rays, N = c["rays"], len(c["rays"])
    slots = _slots(rays.tobytes(), len(rays))
    hidden = _rows_of(rays, hide, len(slots)) if hide is not None else np.zeros(len(slots), bool)

    def lay(a, K=None):
        a = np.array(a if K is None else a[:, :K], f)
        a[hidden] = np.nan
        return cr.to_patch(a, slots, M, fill=np.nan)
    ins = dict(sig=Buf(lay(c["sig"])), rgb=Buf(lay(c["rgb"])), dl=Buf(lay(c["deltas"])), rays=Buf(rays),
               ex=Buf(lay(c["extra"], K)) if K else None)
    assert ins["dl"].ptr % 8 == 0
    out = dict(weights_sum=_fresh(N), depth=_fresh(N), image=_fresh((N, 3)), extra_out=_fresh((N, K)) if K else None,
               weights=_fresh(M) if (weights or K) else None, skippable=Buf(np.zeros(2, np.int32)))
    check(lib.inr_composite_rays_patch_forward(ins["sig"].ptr, ins["rgb"].ptr, ins["dl"].ptr, ins["rays"].ptr, N, M, T,
                                               _ptr(ins["ex"]), K, out["weights_sum"].ptr, out["depth"].ptr,
                                               out["image"].ptr, _ptr(out["extra_out"]), _ptr(out["weights"]),
                                               out["skippable"].ptr, stream()), "composite_rays_patch_forward")
    got = _finish(ins, out, "patch forward")
    got["skippable"] = int(got["skippable"].view(np.int64)[0])
    return got, slots


def run_wavefront(lib, c, n_step, K, T_thresh):
    """composite_rays looped to completion by composite_reference.wavefront_run -> accumulators, number of calls."""
    N = len(c["rays"])
    st = dict(weights_sum=Buf(np.zeros(N, f)), depth=Buf(np.zeros(N, f)), image=Buf(np.zeros((N, 3), f)),
              extra_acc=Buf(np.zeros((N, K), f)) if K else None, rays_t=Buf(np.asarray(c["t0"], f)))

    def step(n_alive, n_step, alive, sig, rgb, dl, ex):
        A, S, R, D = Buf(alive), Buf(sig), Buf(rgb), Buf(dl)
        E = Buf(ex) if K else None
        check(lib.inr_composite_rays(n_alive, n_step, A.ptr, st["rays_t"].ptr, S.ptr, R.ptr, D.ptr, st["weights_sum"].ptr,
                                     st["depth"].ptr, st["image"].ptr, T_thresh, _ptr(E), _ptr(st["extra_acc"]), K,
                                     stream()), "composite_rays")
        after = A.get()
        A.check_guards("rays_alive")
        assert ((after == alive) | (after == -1)).all()
        return after
    calls = cr.wavefront_run(c, n_step, step, K)
    got = _finish({}, st, "wavefront")
    got["calls"] = calls
    return got


# ---------------------------------------------------------------------------- checks shared by both tiers
def _fwd_inputs(chk):
    """The forward's outputs as the backward and the K-channel kernels take them: the expected values in fp32."""
    return {k: np.asarray(chk.want[k], f) for k in ("weights_sum", "image", "weights")}


def check_forward(lib, chk, M, K, weights=True):
    c = chk.c
    got = run_forward(lib, c, M, K, weights)
    for name in ("weights_sum", "depth", "image"):
        chk.cmp(name, got[name])
    if K:
        chk.cmp("extra_out", got["extra_out"])
    if weights or K:
        owned = chk.want["sample_ray"][:M] >= 0               # rows of [0, M) some ray owns (a dropped one: to the end)
        chk.cmp("weights", got["weights"], want=chk.want["weights"][:M], rows=owned)
    if weights:
        assert np.array_equal(got["sample_ray"][owned], chk.want["sample_ray"][:M][owned]), chk.what + " sample_ray"
    return got


def check_backward(lib, chk, M, K, total=None, field=True, with_g_ws=True):
    c = chk.c
    got = run_backward(lib, c, M, K, _fwd_inputs(chk), total, field, with_g_ws)
    if field:
        gs = _pad(np.asarray(chk.want["grad_sigmas"]), M)
        if not with_g_ws:                                        # d0 * g_ws * (1 - ws) taken out again, in float64
            ws_row = np.zeros(len(gs))
            for n, (rid, off, cnt) in enumerate(c["rays"]):
                if off + cnt <= M:
                    used = int(chk.want["n_used"][n])
                    ws_row[off:off + used] = c["g_ws"][rid] * (1.0 - np.float64(chk.want["weights_sum"][rid]))
            gs = gs.astype(np.float64) - c["deltas"][:len(gs), 0].astype(np.float64) * ws_row[:len(gs)]
        gs = np.nan_to_num(gs, nan=0.0)                          # padding rows [total, M): zero
        chk.cmp("grad_sigmas", got["grad_sigmas"], want=gs)
        chk.cmp("grad_rgbs", got["grad_rgbs"], want=np.nan_to_num(_pad(np.asarray(chk.want["grad_rgbs"]), M), nan=0.0))
    if K:
        chk.cmp("grad_extra", got["grad_extra"], want=np.nan_to_num(_pad(np.asarray(chk.want["grad_extra"]), M), nan=0.0))
    return got


def check_patch(lib, chk, M, K, weights=True):
    c = chk.c
    rays, N = c["rays"], len(c["rays"])
    drop = cr.dropped_groups(rays, M)
    got, slots = run_patch(lib, c, M, K, weights, hide=drop)
    live_ids = np.ones(N, bool)
    live_ids[rays[drop, 0]] = False
    for name in ("weights_sum", "depth", "image") + (("extra_out",) if K else ()):
        chk.cmp(name, got[name], ids=live_ids)
        dead = np.asarray(got[name])[~live_ids]
        assert not dead.any() and not np.isnan(dead).any(), f"{chk.what} {name}: a dropped group's ray is not zero"
    if weights or K:
        rows = np.zeros(M, bool)
        rows[slots[_rows_of(rays, ~drop, len(slots))]] = True
        want = cr.to_patch(np.asarray(chk.want["weights"], np.float64), slots, M)
        if isinstance(chk, Close):
            keep = np.zeros(M, bool)
            keep[slots[chk.rows & _rows_of(rays, ~drop, len(slots))]] = True
            got_w, want_w = got["weights"], want
            e = float(np.abs(got_w.astype(np.float64) - want_w)[keep].max())
            assert np.isfinite(got_w[keep]).all() and e <= cr.TOL["weights"], f"{chk.what} patch weights err {e:.3e}"
        else:
            chk.cmp("weights", got["weights"], want=want, rows=rows)
        # rows of [0, M) inside a dropped group belong to nobody: left alone
        assert (got["weights"][~rows].view(np.int32) == SENTINEL).all(), chk.what + ": a row of a dropped group was written"
    return got, drop


# ---------------------------------------------------------------------------- exact tier
def _exact_M(variant, c):
    return cr.last_ray_dropped_M(c["rays"]) if variant == "dropped" else len(c["sig"])


@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("variant", ["plain", "nan", "dropped"])
def test_exact_train_forward(lib, variant, weights):
    """k_composite_train_fwd with and without the weight / sample_ray outputs: ws == 1, image == rgb[p], depth ==
    (p+1) 2^-6, weights one-hot at p, sample_ray == ray id on every owned row; transparent rays all zero.  "dropped":
    the last ray does not fit into M rows - zero outputs, its rows to the end of the buffer zero weight.  "nan": NaN in
    sigma and rgb behind the opaque sample - the same outputs, those samples are never used."""
    chk = Exact(variant, 0, M=_exact_M(variant, _exact_case(variant)))
    check_forward(lib, chk, _exact_M(variant, chk.c), 0, weights)


@pytest.mark.parametrize("total", ["none", "total", "padded"])
@pytest.mark.parametrize("variant", ["plain", "nan", "dropped"])
def test_exact_train_backward(lib, variant, total):
    """k_composite_train_bwd: grad_rgbs one-hot times g_img; grad_sigmas[i<p] = 2^-8 g.(c_i - c_p), zero at and behind p;
    transparent rays 2^-8 (g.c_i + g_ws) - through all 16 chunks of a 1024-sample ray.  Without total_dev the rows of
    live rays are written (they start as NaN here) and the rest stays the caller's zero; with it EVERY row of [0, M) is
    written: "total" M == total, "padded" M = total + 37 (the padding is shared out over the waves)."""
    c = _exact_case(variant)
    n_total = len(c["sig"])
    M = _exact_M(variant, c) + (37 if total == "padded" and variant != "dropped" else 0)
    chk = Exact(variant, 0, M=min(M, n_total))
    check_backward(lib, chk, M, 0, total=None if total == "none" else n_total)
    if total == "none":
        check_backward(lib, chk, M, 0, with_g_ws=False)


@pytest.mark.parametrize("K", [1, 16, 31, 64])
def test_exact_extra_forward_and_backward(lib, K):
    """k_composite_train_extra_fwd behind k_composite_train_fwd (one call) and k_composite_train_extra_bwd at K = 1, 16,
    31, 64: extra_out == extra[p], grad_extra one-hot times g_extra; plain, NaN behind the opaque sample (sigma, rgb and
    extra), last ray dropped."""
    for variant in ("plain", "nan", "dropped"):
        c = _exact_case(variant)
        M = _exact_M(variant, c)
        chk = Exact(variant, K, M=M)
        check_forward(lib, chk, M, K)
        check_backward(lib, chk, M, K, field=False)
        check_backward(lib, chk, M, K)
        got = run_extra_ce(lib, c, K, chk.want["weights"]) if variant != "dropped" else None
        if got is not None:
            chk.cmp("extra_out", got["extra_out"])


@pytest.mark.parametrize("K", [0, 1, 16, 31, 64])
def test_exact_patch(lib, K):
    """k_composite_patch_fwd and k_composite_patch_extra in the patch-interleaved layout built by the independent slot
    map: the same exact outputs, the weights at their patch rows, skippable == the reference count.  "dropped": M =
    total - 1, the last group with samples does not fit and composites to nothing, its rows stay untouched.  K = 0 runs
    with and without the weight buffer."""
    for variant in ("plain", "nan", "dropped"):
        c = _exact_case(variant)
        M = len(c["sig"]) - (1 if variant == "dropped" else 0)
        chk = Exact(variant, K)
        for weights in ((True, False) if K == 0 else (True,)):
            got, drop = check_patch(lib, chk, M, K, weights)
            assert drop.any() == (variant == "dropped")
            want = cr.skippable(c["rays"], chk.want["n_used"], M)
            assert got["skippable"] == want and (want > 0), (variant, got["skippable"], want)


@pytest.mark.parametrize("n_step", [1, 3, 8])
def test_exact_wavefront(lib, n_step):
    """k_composite_rays looped to completion, n_step rows per ray and call, 16 extra channels accumulated in place: the
    exact outputs (depth over the absolute t), rays_t as the fp32 restatement leaves it, as many calls as the
    restatement needs; rows behind a ray's last sample (delta 0) hold NaN and are not read."""
    for variant in ("plain", "nan"):
        chk = Exact(variant, 16, absolute_depth=True)
        got = run_wavefront(lib, chk.c, n_step, 16, T)
        ref = cr.wavefront_reference(chk.c, n_step, K=16, dtype=f)
        for name in ("weights_sum", "depth", "image"):
            chk.cmp(name, got[name])
        chk.cmp("extra_out", got["extra_acc"])
        chk.cmp("rays_t", got["rays_t"], want=ref["rays_t"])
        assert got["calls"] == ref["calls"]


# ---------------------------------------------------------------------------- tolerance tier
@pytest.mark.parametrize("regime", cr.REGIMES)
def test_train_forward_and_backward_against_fp64(lib, regime):
    """k_composite_train_fwd (+ the 64 channels behind it), k_composite_train_bwd with and without total_dev and
    k_composite_train_extra_bwd against float64, each output within TOL (grad_sigmas: 1.44e-7 at gradients of 1.7e-2).
    The backward takes the float64 forward's weights_sum, image and weights rounded to fp32.  Regime "zero": all
    weights zero, grad_sigmas not."""
    chk = Close(regime, 64)
    M = len(chk.c["sig"])
    check_forward(lib, chk, M, 64)
    check_forward(lib, Close(regime, 0), M, 0, weights=False)
    check_backward(lib, chk, M, 64)
    check_backward(lib, chk, M + 37, 64, total=M)


@pytest.mark.parametrize("K,n_classes", [(5, 3), (5, 5), (31, 17), (31, 31), (64, 40), (64, 64)])
def test_fused_cross_entropy_against_fp64(lib, K, n_classes):
    """The cross-entropy rows of k_composite_train_extra_fwd (dpix, part) and k_ce_finalize's loss_out against ce_rows on
    the float64 logits, every regime: K = 5, 31, 64 with n_classes below and equal to K, every seventh row ignored.
    dpix is zero in the padded channels and on ignored rows.  Then one label outside the classes: loss_out[0] is NaN,
    the bad count 1, that row of dpix zero, everything else as before."""
    ignore = -1
    for regime in cr.REGIMES:
        chk = Close(regime, K)
        c, N = chk.c, len(chk.c["rays"])
        labels = c["labels"] % n_classes
        labels[::7] = ignore
        labels[~chk.ids] = ignore                     # an ambiguous ray's logits are not compared: out of the mean too
        bad_row = int(np.flatnonzero(chk.ids & (labels != ignore))[0])
        weights = np.asarray(chk.want["weights"], f)
        for with_bad in (False, True):
            lab = labels.copy()
            if with_bad:
                lab[bad_row] = n_classes
            loss, dpix, kept, bad = cr.ce_rows(chk.want["extra_out"], lab, n_classes, ignore)
            got = run_extra_ce(lib, c, K, weights, lab, n_classes, ignore)
            chk.cmp("extra_out", got["extra_out"])
            chk.cmp("ce_dpix", got["dpix"], want=dpix)
            assert not got["dpix"][~kept].any() and not got["dpix"][:, n_classes:].any()
            chk.cmp("ce_loss", got["part"][:, 0], want=loss)
            assert np.array_equal(got["part"][:, 1], kept.astype(f)) and np.array_equal(got["part"][:, 2], bad.astype(f))
            assert not got["part"][:, 3].any()
            n_kept = int(kept.sum())
            assert got["loss"][2] == n_kept and got["loss"][3] == int(with_bad) and got["loss"][1] == f(1.0) / f(n_kept)
            if with_bad:
                assert np.isnan(got["loss"][0]) and bad[bad_row] and not got["dpix"][bad_row].any()
            else:
                e = abs(float(got["loss"][0]) - float(loss[kept].mean()))
                print(f"{chk.what} n_classes {n_classes} loss: err {e:.3e} allowed {cr.TOL['ce_loss']:.2e}")
                assert e <= cr.TOL["ce_loss"]


@pytest.mark.parametrize("regime", cr.REGIMES)
def test_patch_against_fp64(lib, regime):
    """k_composite_patch_fwd and k_composite_patch_extra (31 channels) through the independent slot map against float64;
    skippable equals the reference count where no ray of the case is ambiguous."""
    chk = Close(regime, 31)
    M = len(chk.c["sig"])
    got, _ = check_patch(lib, chk, M, 31)
    check_patch(lib, Close(regime, 0), M, 0, weights=False)
    want = cr.skippable(chk.c["rays"], chk.want["n_used"], M)
    print(f"{chk.what} skippable {got['skippable']} reference {want}")
    if chk.ids.all():
        assert got["skippable"] == want


@pytest.mark.parametrize("n_step", [1, 3, 8])
@pytest.mark.parametrize("regime", cr.REGIMES)
def test_wavefront_against_fp64(lib, regime, n_step):
    """k_composite_rays looped to completion against the float64 restatement of its T = 1 - ws form (16 channels in
    place, rays_t), the rays left out whose stop is ambiguous in that form.  Regime s40 stops at T_thresh = 0.05
    (composite_reference.py, "Ambiguity")."""
    chk = Close(regime, 16)
    c = chk.c
    ref = cr.wavefront_reference(c, n_step, K=16)
    keep = cr.compared_rays(c, ratio=ref["ratio"])
    ids = np.zeros(len(keep), bool)
    ids[c["rays"][:, 0]] = keep
    chk.ids = ids
    got = run_wavefront(lib, c, n_step, 16, c["T_wavefront"])
    for name, key in (("wf_weights_sum", "weights_sum"), ("wf_depth", "depth"), ("wf_image", "image"),
                      ("wf_extra", "extra_acc"), ("wf_rays_t", "rays_t")):
        chk.cmp(key, got[key], tolname=name, want=ref[key])
    if ids.all():
        assert got["calls"] == ref["calls"]
