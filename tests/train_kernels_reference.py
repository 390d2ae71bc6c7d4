"""Restatements of the small kernels every training step runs through (csrc/encoders.hip: k_adam, k_adam_tail,
k_adam_multi, k_sh_bwd, k_linear_wgrad; csrc/raymarch.hip: k_ce_rows), NumPy and torch on the CPU only.

The library is built with -ffp-contract=off and nothing fast-math, and Adam, the parameter EMA and SH use only + - * /
and sqrt: the ``*32`` functions below repeat the kernels' operations in fp32 IN THE KERNELS' ORDER and are what the GPU
must equal bit for bit (tests/test_train_kernels.py).  The ``*64`` functions are the textbook formulas in fp64; they are
what tests/test_train_kernels_cpu.py measures the fp32 restatements against.  Every random input comes from the integer
hash ``detections_cases.uniform``, no library generator whose stream could change."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detections_cases import uniform  # noqa: E402

f = np.float32


# ---------------------------------------------------------------------------- comparison
def bit_mismatches(a, b):
    """Number of elements of two arrays of a 4-byte type whose BITS differ (-0.0 != 0.0, a NaN equals the same NaN);
    a different shape or dtype counts as everything differing.  The comparison of every bit-for-bit test."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or a.dtype.itemsize != 4:
        return max(a.size, b.size, 1)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def assert_same_bits(got, want, what=""):
    n = bit_mismatches(got, want)
    if n:
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        where = ""
        if got.shape == want.shape and got.dtype == want.dtype:
            i = int(np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())[0])
            where = f"; first at flat index {i}: {got.ravel()[i]!r} != {want.ravel()[i]!r}"
        raise AssertionError(f"{what}: {n} of {want.size} elements differ in their bits{where}")


# ---------------------------------------------------------------------------- inputs
def signed(seed, n):
    """fp32 in [-1, 1) on a 2^-23 lattice."""
    return (uniform(seed, n) * 2.0 - 1.0).astype(f)


def normal(seed, n):
    """~N(0, 1) doubles: Box-Muller over two streams of the hash."""
    u1, u2 = uniform(seed, n), uniform(seed + 7919, n)
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


def adam_grads(seed, n):
    """fp32 gradients of either sign with |g| log-uniform in [1e-6, 1e2]: g*g (and (g/128)^2) stays far above the fp32
    denormals, so no product of the update depends on how denormals are flushed."""
    mag = np.clip(np.power(10.0, -6.0 + 8.0 * uniform(seed + 104729, n)), 1e-6, 1e2).astype(f)
    return np.where(uniform(seed, n) < 0.5, -mag, mag)


def small_ints(seed, shape, k):
    """Integers in {-k..k} as int64."""
    n = int(np.prod(shape))
    return (np.floor(uniform(seed, n) * (2 * k + 1)).astype(np.int64) - k).reshape(shape)


def sh_directions(seed, M):
    """[M, 3] fp32 in the closed unit ball: the zero vector, the six axes, -0.0 components, short vectors, points ON the
    sphere and random interior points."""
    special = np.asarray([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                          [-0.0, -0.0, -0.0], [-0.0, 1, 0.0], [1e-3, -2e-3, 5e-4], [0.25, -0.5, 0.125],
                          [0.6, 0.0, -0.8], [1e-10, 0, -1e-10]], np.float64)     # cubes stay above the denormals
    v = normal(seed, 3 * M).reshape(M, 3)
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    r = uniform(seed + 31, M)
    r[::3] = 1.0                                   # every third one on the sphere
    d = (v * r[:, None]).astype(f)
    n = np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
    d = np.where(n > 1.0, d / (n * (1 + 1e-6)), d).astype(f)       # fp32 rounding must not leave the ball
    k = min(M, len(special))
    d[:k] = special[:k].astype(f)
    return d


# ---------------------------------------------------------------------------- Adam
def adam_scalars(lr, b1, b2, eps, step):
    """(b1, b2, 1 - b1, 1 - b2, lr_t, eps_t) as the kernels receive them.  The C ABI takes lr, the betas and eps as
    ``float``; the host code then folds the bias corrections in double: bc = 1 - pow(double(beta), step),
    lr_t = float(lr * sqrt(bc2) / bc1), eps_t = float(eps * sqrt(bc2))."""
    b1, b2, lr, eps = f(b1), f(b2), f(lr), f(eps)
    bc1 = 1.0 - math.pow(float(b1), step)
    bc2 = 1.0 - math.pow(float(b2), step)
    return b1, b2, f(1.0) - b1, f(1.0) - b2, f(float(lr) * math.sqrt(bc2) / bc1), f(float(eps) * math.sqrt(bc2))


def adam32(p, g, m, v, lr, b1, b2, eps, step, grad_scale, shadow=None, ema_w=0.0, wrong=None):
    """One step in fp32 in the order of INR_ADAM1 (three copies in csrc/encoders.hip) -> new (p, m, v) or, with a
    shadow, (p, m, v, shadow):
        gr = g * gscale;  m = b1*m + (1-b1)*gr;  v = b2*v + ((1-b2)*gr)*gr;  p = p - (lr_t*m) / (sqrt(v) + eps_t)
        s = s + ema_w * (p_new - s)
    ``wrong``: deliberately broken variants for the tests of the comparison ("skip_last": the last element is left as
    it was; "assoc": (1-b2)*(gr*gr))."""
    b1, b2, c1, c2, lr_t, eps_t = adam_scalars(lr, b1, b2, eps, step)
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    gr = g * f(grad_scale)
    m1 = b1 * m + c1 * gr
    v1 = b2 * v + ((c2 * (gr * gr)) if wrong == "assoc" else (c2 * gr) * gr)
    p1 = p - (lr_t * m1) / (np.sqrt(v1) + eps_t)
    if wrong == "skip_last" and p.size:
        p1[-1], m1[-1], v1[-1] = p[-1], m[-1], v[-1]
    assert p1.dtype == m1.dtype == v1.dtype == f
    if shadow is None:
        return p1, m1, v1
    return p1, m1, v1, ema32(shadow, p1, ema_w)


def ema32(shadow, p_new, ema_w):
    """The parameter EMA inside the optimiser launch, fp32: s + w * (p_new - s)."""
    s, p_new = np.asarray(shadow, f), np.asarray(p_new, f)
    s1 = s + f(ema_w) * (p_new - s)
    assert s1.dtype == f
    return s1


def adam64(p, g, m, v, lr, b1, b2, eps, step, grad_scale):
    """torch.optim.Adam's formula in fp64 (the hyper-parameters as the fp32 values every implementation receives):
    p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)."""
    b1, b2, lr, eps = (float(f(a)) for a in (b1, b2, lr, eps))
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gr = g * float(f(grad_scale))
    m1 = b1 * m + (1.0 - b1) * gr
    v1 = b2 * v + (1.0 - b2) * gr * gr
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return p - lr / bc1 * m1 / (np.sqrt(v1) / math.sqrt(bc2) + eps), m1, v1


# ---------------------------------------------------------------------------- SH
_C1 = f(0.48860251190291987)
_C2 = f(1.0925484305920792)
_C6 = f(0.94617469575755997)
_C8 = f(0.54627421529603959)
_A = f(0.59004358992664352)
_B = f(2.8906114426405538)
_C = f(0.45704579946446572)
_E = f(0.3731763325901154)
_F = f(1.4453057213202769)


def sh_bwd32(go, d, degree, wrong=False):
    """k_sh_bwd in fp32, term by term in its order: products left-associated as written, constant products
    (2.0f * 0.946...f) folded in fp32 first, every term ADDED to an accumulator that starts at +0.0.
    ``wrong``: the sign of component 14's y-term flipped (for the test of the comparison)."""
    go, d = np.asarray(go, f), np.asarray(d, f)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    g = [go[:, i] for i in range(degree * degree)]
    gx, gy, gz = (np.zeros(len(d), f) for _ in range(3))
    if degree > 1:
        gy = gy + (-_C1) * g[1]
        gz = gz + _C1 * g[2]
        gx = gx + (-_C1) * g[3]
    if degree > 2:
        gx = gx + _C2 * y * g[4]
        gy = gy + _C2 * x * g[4]
        gy = gy + (-_C2) * z * g[5]
        gz = gz + (-_C2) * y * g[5]
        gz = gz + (f(2.0) * _C6) * z * g[6]
        gx = gx + (-_C2) * z * g[7]
        gz = gz + (-_C2) * x * g[7]
        gx = gx + (f(2.0) * _C8) * x * g[8]
        gy = gy + (f(-2.0) * _C8) * y * g[8]
    if degree > 3:
        x2, y2, z2 = x * x, y * y, z * z
        gx = gx + _A * (f(-6.0) * x * y) * g[9]
        gy = gy + _A * (f(-3.0) * x2 + f(3.0) * y2) * g[9]
        gx = gx + _B * y * z * g[10]
        gy = gy + _B * x * z * g[10]
        gz = gz + _B * x * y * g[10]
        gy = gy + _C * (f(1.0) - f(5.0) * z2) * g[11]
        gz = gz + _C * (f(-10.0) * y * z) * g[11]
        gz = gz + _E * (f(15.0) * z2 - f(3.0)) * g[12]
        gx = gx + _C * (f(1.0) - f(5.0) * z2) * g[13]
        gz = gz + _C * (f(-10.0) * x * z) * g[13]
        gx = gx + (_F * f(2.0)) * x * z * g[14]
        gy = gy + ((_F if wrong else -_F) * f(2.0)) * y * z * g[14]
        gz = gz + _F * (x2 - y2) * g[14]
        gx = gx + _A * (f(-3.0) * x2 + f(3.0) * y2) * g[15]
        gy = gy + _A * (f(6.0) * x * y) * g[15]
    out = np.stack([gx, gy, gz], 1)
    assert out.dtype == f
    return out


def sh_fwd32(d, degree):
    """The forward's bit reference: oracle.sh.sh_encode is fp32 in the order of ``sh4`` (csrc/grid_common.h)."""
    from oracle.sh import sh_encode
    return sh_encode(torch.from_numpy(np.ascontiguousarray(d, f)), degree).numpy()


def sh64(d, degree, go=None):
    """The same polynomial in fp64 -> values [M, degree^2] (and, given upstream gradients ``go``, d sum(go*sh) / d d
    through autograd) as fp64 arrays."""
    t = torch.tensor(np.asarray(d, np.float64), requires_grad=go is not None)
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    out = [0.0 * x + 0.28209479177387814]              # constant, but on the graph: degree 1 has a (zero) gradient
    if degree > 1:
        out += [-0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x]
    if degree > 2:
        out += [1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999,
                -1.0925484305920792 * xz, 0.54627421529603959 * (x2 - y2)]
    if degree > 3:
        out += [0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
                0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0),
                0.45704579946446572 * x * (1.0 - 5.0 * z2), 1.4453057213202769 * z * (x2 - y2),
                0.59004358992664352 * x * (-x2 + 3.0 * y2)]
    val = torch.stack(out, -1)
    if go is None:
        return val.numpy()
    (val * torch.tensor(np.asarray(go, np.float64))).sum().backward()
    return val.detach().numpy(), t.grad.numpy()


# ---------------------------------------------------------------------------- weight gradient
def wgrad_int(x, gy, gw0):
    """gw0[o, i] + sum_m gy[m, o] * x[m, i] for INTEGER inputs, as int64.  The int64 product is taken through fp64 BLAS,
    which is exact here (asserted): every product and partial sum is an integer below 2^53."""
    x, gy, gw0 = (np.asarray(a) for a in (x, gy, gw0))
    assert all(a.dtype.kind == "i" for a in (x, gy, gw0))
    bound = (int(np.abs(x).max()) * int(np.abs(gy).max()) if x.size else 0) * max(len(x), 1) + int(np.abs(gw0).max())
    assert bound < 2 ** 53
    prod = gy.astype(np.float64).T @ x.astype(np.float64)
    return prod.astype(np.int64) + gw0.astype(np.int64)


# ---------------------------------------------------------------------------- cross entropy
def ce64(logits, labels, ignore_index, dtype=torch.float64):
    """F.cross_entropy (mean over the kept rows) on the CPU in ``dtype`` -> (loss, UN-NORMALISED gradient
    = d loss / d logits * kept = softmax - onehot on kept rows, 0 on ignored rows, as fp64 [N, K]; kept).  With no kept
    row: (nan, zeros, 0)."""
    lg = torch.tensor(np.asarray(logits), dtype=dtype, requires_grad=True)
    lb = torch.from_numpy(np.asarray(labels, np.int64))
    kept = int((lb != ignore_index).sum())
    if kept == 0 or lg.numel() == 0:
        return float("nan"), np.zeros(lg.shape, np.float64), kept
    loss = torch.nn.functional.cross_entropy(lg, lb, ignore_index=ignore_index)
    loss.backward()
    return float(loss.detach()), lg.grad.double().numpy() * kept, kept
