"""The restatements in tests/train_kernels_reference.py are right: the fp32 ones (which the GPU must equal bit for bit,
tests/test_train_kernels.py) against the fp64 textbook formulas, under bounds that come from another fp32
implementation's own error or from the project's existing tolerances - and the bit comparison has teeth."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_kernels_reference as ref  # noqa: E402

f = np.float32
HYPER = dict(lr=1e-2, b1=0.9, b2=0.99, eps=1e-15)


@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 128])
def test_adam32_is_as_close_to_fp64_as_torchs_fp32_adam(grad_scale):
    """adam32 (the kernels' order, bias corrections folded into lr_t and eps_t) after 1, 3 and 12 steps against adam64:
    its largest |p - p64| may be at most 2x that of torch.optim.Adam in fp32 on the CPU, from the same fp64 trajectory.
    The 2x is room for the two extra roundings of the folded lr_t and eps_t; rounding of p itself dominates both.
    Seen here on 20 000 elements: 9.3e-09, 1.2e-07 and 3.0e-07 after 1, 3 and 12 steps for adam32 AND for torch, at
    both grad_scales: ratio 1.000 every time."""
    n = 20000
    p0 = ref.signed(1, n)
    p32, m32, v32 = p0.copy(), np.zeros(n, f), np.zeros(n, f)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    pt = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=HYPER["lr"], betas=(HYPER["b1"], HYPER["b2"]), eps=HYPER["eps"])
    for step in range(1, 13):
        g = ref.adam_grads(100 + step, n)
        p32, m32, v32 = ref.adam32(p32, g, m32, v32, step=step, grad_scale=grad_scale, **HYPER)
        p64, m64, v64 = ref.adam64(p64, g, m64, v64, step=step, grad_scale=grad_scale, **HYPER)
        pt.grad = torch.from_numpy(g * f(grad_scale))
        opt.step()
        if step in (1, 3, 12):
            mine = np.abs(p32 - p64).max()
            torchs = np.abs(pt.detach().numpy() - p64).max()
            print(f"grad_scale {grad_scale:g} step {step}: adam32 {mine:.3e}, torch fp32 {torchs:.3e}, ratio {mine / torchs:.3f}")
            assert torchs > 0 and mine <= 2.0 * torchs, (step, mine, torchs)
            # the moments have no folded scalar: a few ulps of their size
            assert np.abs(m32 - m64).max() <= 4 * 2.0 ** -24 * np.abs(m64).max()
            assert np.abs(v32 - v64).max() <= 4 * 2.0 ** -24 * np.abs(v64).max()


def test_adam32_ema_and_edge_scales():
    """The shadow rule s + w*(p_new - s): w = 0 leaves the bits, w = 1 gives p_new exactly for these magnitudes;
    grad_scale 0 leaves zero moments zero and p untouched; lr 0 leaves p untouched while the moments advance."""
    n = 1000
    p, g, s = ref.signed(2, n), ref.adam_grads(3, n), ref.signed(4, n)
    z = np.zeros(n, f)
    p1, m1, v1, s0 = ref.adam32(p, g, z, z, step=1, grad_scale=1.0, shadow=s, ema_w=0.0, **HYPER)
    assert ref.bit_mismatches(s0, s) == 0
    s1 = ref.adam32(p, g, z, z, step=1, grad_scale=1.0, shadow=s, ema_w=1.0, **HYPER)[3]
    assert np.abs(s1 - p1).max() <= 2.0 ** -23 * 2         # s + (p - s): one rounding of the difference, one of the sum
    sw = ref.adam32(p, g, z, z, step=1, grad_scale=1.0, shadow=s, ema_w=0.05, **HYPER)[3]
    assert np.abs(sw - (s + 0.05 * (p1.astype(np.float64) - s))).max() < 1e-6
    p2, m2, v2 = ref.adam32(p, g, z, z, step=1, grad_scale=0.0, **HYPER)
    assert ref.bit_mismatches(p2, p) == 0 and not m2.any() and not v2.any()
    hyper0 = dict(HYPER, lr=0.0)
    p3, m3, v3 = ref.adam32(p, g, z, z, step=1, grad_scale=1.0, **hyper0)
    assert ref.bit_mismatches(p3, p) == 0 and ref.bit_mismatches(m3, m1) == 0 and ref.bit_mismatches(v3, v1) == 0


def test_adam_grads_stay_clear_of_underflow():
    g = ref.adam_grads(5, 100000)
    a = np.abs(g.astype(np.float64))
    assert a.min() >= 0.999e-6 and a.max() <= 1e2 and (g < 0).any() and (g > 0).any()
    assert ((a / 128) ** 2 * 0.01).min() > 1e-30                 # fp32 normals end at 1.2e-38


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_sh_restatements_against_fp64(degree):
    """Forward oracle (fp32, the order of sh4) within 1e-6 of the fp64 polynomial and sh_bwd32 within 1e-5 of its
    autograd gradient - the project's bounds (tests/test_gpu_parity.py::test_sh_forward_backward) - on directions in
    the closed unit ball (zero, axes, -0.0, short vectors) with upstream gradients ~N(0,1).  Seen here: forward
    1.5e-07, backward 1.3e-06 at the worst (degree 4).  Degree 1 is constant: zero gradient."""
    M = 5000
    d = ref.sh_directions(11, M)
    assert (np.linalg.norm(d.astype(np.float64), axis=1) <= 1.0 + 1e-7).all() and not d[0].any()
    go = ref.normal(12 + degree, M * degree * degree).reshape(M, -1).astype(f)
    val64, grad64 = ref.sh64(d, degree, go)
    fwd = ref.sh_fwd32(d, degree)
    bwd = ref.sh_bwd32(go, d, degree)
    assert fwd.dtype == f and fwd.shape == (M, degree * degree) and bwd.shape == (M, 3)
    e_f, e_b = np.abs(fwd - val64).max(), np.abs(bwd - grad64).max()
    print(f"degree {degree}: forward {e_f:.2e}, backward {e_b:.2e}")
    assert e_f < 1e-6 and e_b < 1e-5
    if degree == 1:
        assert not bwd.any() and not grad64.any()
    else:
        assert np.abs(grad64).max() > 1.0


def test_wgrad_int_is_the_int64_product():
    x, gy, gw0 = ref.small_ints(21, (517, 33), 3), ref.small_ints(22, (517, 31), 3), ref.small_ints(23, (31, 33), 5)
    assert x.min() == -3 and x.max() == 3 and gw0.min() == -5 and gw0.max() == 5
    want = np.einsum("mo,mi->oi", gy, x) + gw0
    got = ref.wgrad_int(x, gy, gw0)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(ref.wgrad_int(x[:0], gy[:0], gw0), gw0)


def test_ce64_is_softmax_minus_onehot():
    logits = (ref.normal(31, 7 * 5) * 4).reshape(7, 5)
    labels = np.asarray([0, 4, 2, -1, 1, 2, 3])
    for ignore, kept_rows in ((-1, [0, 1, 2, 4, 5, 6]), (2, [0, 1, 4, 6])):
        lb = np.where(labels == -1, ignore, labels)
        loss, grad, kept = ref.ce64(logits, lb, ignore)
        assert kept == len(kept_rows)
        e = np.exp(logits - logits.max(1, keepdims=True))
        sm = e / e.sum(1, keepdims=True)
        want = np.zeros_like(sm)
        for r in kept_rows:
            want[r] = sm[r]
            want[r, lb[r]] -= 1.0
        assert np.abs(grad - want).max() < 1e-14
        assert abs(loss - np.mean([-np.log(sm[r, lb[r]]) for r in kept_rows])) < 1e-13
    loss, grad, kept = ref.ce64(logits, np.full(7, -100), -100)
    assert np.isnan(loss) and kept == 0 and not grad.any()


# ---------------------------------------------------------------------------- teeth
def test_the_bit_comparison_reports_a_wrong_adam():
    n = 1027
    p, g, m, v = ref.signed(41, n), ref.adam_grads(42, n), ref.signed(43, n) * f(0.1), np.abs(ref.signed(44, n))
    good = ref.adam32(p, g, m, v, step=3, grad_scale=1.0, **HYPER)
    again = ref.adam32(p, g, m, v, step=3, grad_scale=1.0, **HYPER)
    for a, b in zip(good, again):
        ref.assert_same_bits(a, b)
    skipped = ref.adam32(p, g, m, v, step=3, grad_scale=1.0, wrong="skip_last", **HYPER)
    assert [ref.bit_mismatches(a, b) for a, b in zip(good, skipped)] == [1, 1, 1]
    assoc = ref.adam32(p, g, m, v, step=3, grad_scale=1.0, wrong="assoc", **HYPER)
    assert ref.bit_mismatches(good[1], assoc[1]) == 0           # m does not contain the product
    assert ref.bit_mismatches(good[2], assoc[2]) > n // 20      # v differs in its last bit in many places
    assert np.abs(good[2] - assoc[2]).max() <= 2.0 ** -22 * np.abs(good[2]).max()       # ... and only there
    with pytest.raises(AssertionError, match="differ in their bits"):
        ref.assert_same_bits(skipped[0], good[0], "p")


def test_the_bit_comparison_reports_a_flipped_sh_term_and_signed_zero():
    M = 300
    d = ref.sh_directions(51, M)
    go = ref.normal(52, M * 16).reshape(M, 16).astype(f)
    good, bad = ref.sh_bwd32(go, d, 4), ref.sh_bwd32(go, d, 4, wrong=True)
    assert ref.bit_mismatches(good, ref.sh_bwd32(go, d, 4)) == 0
    assert ref.bit_mismatches(good, bad) > M // 2
    assert ref.bit_mismatches(good[:, [0, 2]], bad[:, [0, 2]]) == 0         # only the y component
    assert ref.bit_mismatches(ref.sh_bwd32(go[:, :9], d, 3), ref.sh_bwd32(go[:, :9], d, 3, wrong=True)) == 0
    assert ref.bit_mismatches(np.zeros(3, f), -np.zeros(3, f)) == 3
    nan = np.full(2, np.nan, f)
    assert ref.bit_mismatches(nan, nan.copy()) == 0
    assert ref.bit_mismatches(np.zeros(3, f), np.zeros(4, f)) > 0
    assert ref.bit_mismatches(np.zeros(3, f), np.zeros(3, np.int32)) > 0
