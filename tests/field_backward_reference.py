"""Plain float64 restatements of the fused field's training backward (csrc/field_fused.hip: k_nerf_head_bwd +
k_nerf_head_wgrad_reduce, k_instance_head_bwd + k_head_wgrad_reduce, and the chain kernels k_nerf_bwd / k_instance_bwd),
the generators of their test cases and the tolerances of tests/test_field_backward_kernels.py.  numpy only (plus ``sh64``
of train_kernels_reference); nothing shared with instance_nerf_amd or oracle/.

Restatements.  One piece of code, ``nerf_head`` / ``instance_head`` / ``nerf_chain`` / ``instance_chain``, runs on a
*model* of the arithmetic:
  Exact64    float64 matmuls - the reference.
  SplitBf16  the default build: an MLP layer takes the weight as rne_bf16(w) + rne_bf16(w - hi), the activation as a
             truncated head plus a truncated remainder, forms hi*hi + lo*hi + hi*lo and rounds the sum to fp32; a weight
             gradient splits both staged operands with round-to-nearest (hb_split2) and takes the same three products;
             elementwise steps are rounded to fp32 one by one, expf is exp2(fp32(x * log2e)), the sigmoid
             1 / (1 + expf(-o)) in fp32.
  SeqFp32    the -DINR_MLP_FP32=1 build: fp32 accumulation of a layer input by input (product and sum each rounded).
Both models sum a weight gradient as the launch does (grid = min(ceil(M / 128), CUs) workgroups, 128 samples each per
round): the accumulator is rounded to fp32 after every MFMA (32 samples per instruction and three instructions per
chunk in the default build, 4 samples in the fp32 build), round after round, then the reduce kernel's order over the
workgroups (16 slices of every 16th workgroup, then the slices).
NeRF field: sigma net (64 <- 32, 16 <- 64) -> SH degree 4 -> colour net on [16 SH, 15 geo] (64 <- 31, 64 <- 64, 3 <- 64)
-> sigmoid; backward with the trunc_exp rule d so0 = g_sigma * density_scale * exp(clamp(so0, -15, 15)); ReLU mask h > 0.
Instance field: rows m < min(n, M) with g = g_pix[ray] * (wbuf * a * b); rows n <= m < M give d_enc = 0.
Every output comes with ``cond``, the same final contraction over absolute values (|dz_h1| @ |Ws0| for d_enc,
sum_m |G_m||X_m| for a weight gradient, |value| for an elementwise output, 0 where a ReLU mask is off).

Tolerance tier.  enc ~ U(-1,1), weights U(+-0.35) (32 inputs) / U(+-0.25) (64 inputs), gradients ~ N(0,1); the density
row of the NeRF sigma net is centred and scaled by SO0_SCALE so that so0 passes +-15 on both sides for a few samples.  Candidate
samples whose float64 pre-activation of ANY hidden unit has |pre| < MARGIN * (|x| @ |W|^T) are rejected and the first M
accepted ones kept, so the float64 ReLU masks are the masks of every kernel and no sample is excluded from any
comparison.  One all-zero enc row stays in every case (pre-activations exactly 0: pins ``> 0`` against ``>= 0``).
MARGIN = 2^-11 = 4.9e-4 >= 8 x the largest split-model pre-activation error in that normalisation (measured 4.8e-5 over
all cases, three layers deep; fp32 model 4.1e-7); acceptance stays above 50 % (measured: 69 .. 76 % NeRF, 77 .. 89 %
instance; asserted on the CPU).

TOL[build][name] = 8 x MEASURED[build][name]; MEASURED is the largest |model - float64| / cond over every
tolerance-tier case, measured on the CPU with NOMINAL_CUS workgroups, rounded up to two digits.  The 8 covers the
accumulation order inside an MFMA, the order over workgroups and the device's v_exp_f32 / v_rcp_f32.  An element with
cond == 0 must be exactly 0.  tests/test_field_backward_cpu.py asserts that the models stay within TOL / 8.
A weight gradient's worst element sits in the SMALL cases (a handful of samples under one element, each with an upstream
gradient that may be all cancellation: 1.4e-2 of cond for gw1), which would leave the multi-round launches with a
tolerance a thousand times their own error; those three sizes are therefore held to TOL_BIG = 8 x MEASURED_BIG, the same
measurement over the multi-round cases alone (never above TOL).

Exact tier.  Integer or power-of-two data on which both builds are exact in any summation order: the kernel must equal
the float64 result rounded to fp32 bit for bit.  Instance: enc in {-2..2}, sparse weights in {-1,0,1} (two to three
non-zeros per row), g_pix in {-1,0,1}, wbuf in {0,0.5,1,2}, power-of-two scales.  NeRF: the same integer sigma net with
so0 == 0 exactly ON THE DATA (enc columns 2i, 2i+1 equal, hidden units 2i, 2i+1 equal up to swapping them, +s / -s in the
density row: the density gradient reaches d_enc and gws0), Wc0 zero on the SH columns, colour logits
exactly 0 (sigmoid 0.5, c(1-c) 0.25): variant "a" Wc2 = 0 (only gwc2 receives a colour gradient); variant "b" Wc1 rows
u, v duplicated and Wc2 = +1 on u, -1 on v (gwc2 and gwc1 receive it; dz_c1 cancels exactly because the rows are equal);
variant "c" makes c2[u] == c2[v] only ON THE DATA (geo features 1 and 2 duplicated, Wc0 rows p, p' and Wc1 rows u, v equal
up to swapping the duplicated inputs), so that the gradient passes the whole colour chain down to d_so and gws1 and
cancels in dz_h1.  gwc0[:, :16] multiplies by SH values: tolerance tier only.  Variants "enc12", "w12", "g12" (M <= 200)
put 12-significant-bit values on one side of each product, so that the remainder planes of weights, activations and
both staged operands carry data while the dropped lo*lo term is zero.  ``exactness_violations`` checks, from the
float64 run's own operands: every value entering a product has <= 16 significant bits, one factor of each product <= 8,
every sum |terms| < 2^24 quanta.

Sizes: C = CUs, R = 8 C tiles per round; 0, 1, 15, 16, 17, 127, 128 (one workgroup), 129 (the second workgroup has one
row), 16R-5 (one full round, ragged end), 16R+1 (round two holds one row), 32R+151 (three rounds; the third has one
workgroup plus one full and one ragged tile).

Seen on an MI355X (256 CUs), worst |got - ref| / cond as a fraction of TOL, per output: default build 0.03 .. 0.13
(worst: instance_chain.denc at 16R+1, 3.66e-5 of 2.88e-4; nerf_head.d_enc 5.84e-4 of 4.72e-3; gw1 1.22e-5 of 1.04e-4 at
the multi-round sizes), i.e. the GPU sits on the split model (1/8 = 0.125); fp32 library 0.03 .. 0.30 (worst:
nerf_head.gwc0 1.42e-5 of 4.72e-5, gwc1 1.26e-4 of 6.24e-4).  Both exact tiers: every bit equal.
Mutations of csrc/field_fused.hip, each built once beside the tree and run once (never committed):
  hb_accum without its a_hi * b_lo product   first failure test_head_backward[nerf-exact-a-enc12-M150-ds1.0]; 24 of 93
      fail: the six enc12 / w12 exact cases and every tolerance-tier head case with a live weight gradient; the g12
      cases (wide G, narrow X) rightly pass.
  k_head_wgrad_reduce one group short        first failure test_head_backward[instance-exact-int-M15-K48-nNone-sy]; 22
      of 93 fail: every instance head case with a live gradient.
  next_valid from mn < M instead of mn < n    first failure test_head_backward[instance-exact-int-M16R+1-K32-nM-37-sn];
      4 of 93 fail: exactly the multi-round instance cases with n_dev = M - 37, both tiers (the NaN rows are read).
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_kernels_reference import sh64  # noqa: E402

F32, F64 = np.float32, np.float64
NOMINAL_CUS = 256
MARGIN = 2.0 ** -11
SO0_SCALE = 20.0
KS = (16, 32, 48, 64)
SMALL_SIZES = (0, 1, 15, 16, 17, 127, 128, 129)
BIG_SIZES = ("16R-5", "16R+1", "32R+151")
SIZES = SMALL_SIZES + BIG_SIZES
BUILDS = ("bf16x3", "fp32")


def resolve(size, cus):
    """A size of SIZES as a sample count on a device with ``cus`` compute units."""
    if isinstance(size, int):
        return size
    R = 8 * cus
    return {"16R-5": 16 * R - 5, "16R+1": 16 * R + 1, "32R+151": 32 * R + 16 * 9 + 7}[size]


# |model - float64| / cond, largest over the tolerance-tier cases (value seen -> constant, two digits, rounded up)
MEASURED = {
    "bf16x3": {
        "instance_chain.denc": 3.6e-05,       # 3.505e-05
        "instance_chain.dz1": 2.8e-05,        # 2.703e-05
        "instance_chain.dz2": 2.4e-05,        # 2.300e-05
        "instance_head.d_enc": 3.9e-05,       # 3.827e-05
        "instance_head.gw0": 1.2e-04,         # 1.168e-04
        "instance_head.gw1": 1.4e-02,         # 1.348e-02
        "instance_head.gw2": 6.1e-04,         # 6.000e-04
        "nerf_chain.d_enc": 6.6e-05,          # 6.526e-05
        "nerf_chain.d_o": 1.7e-07,            # 1.673e-07
        "nerf_chain.d_so": 4.1e-05,           # 4.095e-05
        "nerf_chain.dz_c1": 3.4e-05,          # 3.370e-05
        "nerf_chain.dz_c2": 5.0e-05,          # 4.998e-05
        "nerf_chain.dz_h1": 7.3e-05,          # 7.224e-05
        "nerf_head.d_enc": 5.9e-04,           # 5.845e-04
        "nerf_head.gwc0": 1.6e-03,            # 1.592e-03
        "nerf_head.gwc1": 8.8e-03,            # 8.714e-03
        "nerf_head.gwc2": 3.5e-03,            # 3.492e-03
        "nerf_head.gws0": 3.7e-04,            # 3.695e-04
        "nerf_head.gws1": 9.4e-04,            # 9.345e-04
    },
    "fp32": {
        "instance_chain.denc": 3.6e-07,       # 3.582e-07
        "instance_chain.dz1": 3.4e-07,        # 3.316e-07
        "instance_chain.dz2": 3.2e-07,        # 3.170e-07
        "instance_head.d_enc": 4.2e-07,       # 4.129e-07
        "instance_head.gw0": 9.5e-07,         # 9.438e-07
        "instance_head.gw1": 1.8e-04,         # 1.776e-04
        "instance_head.gw2": 2.9e-06,         # 2.820e-06
        "nerf_chain.d_enc": 7.1e-07,          # 7.095e-07
        "nerf_chain.d_o": 1.7e-07,            # 1.673e-07
        "nerf_chain.d_so": 9.1e-07,           # 9.097e-07
        "nerf_chain.dz_c1": 2.9e-07,          # 2.852e-07
        "nerf_chain.dz_c2": 2.7e-07,          # 2.664e-07
        "nerf_chain.dz_h1": 1.2e-06,          # 1.114e-06
        "nerf_head.d_enc": 7.3e-06,           # 7.231e-06
        "nerf_head.gwc0": 5.9e-06,            # 5.848e-06
        "nerf_head.gwc1": 7.8e-05,            # 7.766e-05
        "nerf_head.gwc2": 7.0e-06,            # 6.915e-06
        "nerf_head.gws0": 5.3e-06,            # 5.271e-06
        "nerf_head.gws1": 2.7e-05,            # 2.642e-05
    },
}
# the same over the three multi-round sizes alone: the weight gradients' worst elements sit in the small cases (few
# samples under one element, whose upstream gradient may be all cancellation), so the large launches get their own,
# tighter constants; never above MEASURED
MEASURED_BIG = {
    "bf16x3": {
        "instance_chain.denc": 3.6e-05,       # 3.505e-05
        "instance_chain.dz1": 2.8e-05,        # 2.703e-05
        "instance_chain.dz2": 1.3e-05,        # 1.290e-05
        "instance_head.d_enc": 3.9e-05,       # 3.827e-05
        "instance_head.gw0": 9.9e-07,         # 9.828e-07
        "instance_head.gw1": 1.3e-05,         # 1.215e-05
        "instance_head.gw2": 1.2e-05,         # 1.147e-05
        "nerf_chain.d_enc": 6.6e-05,          # 6.526e-05
        "nerf_chain.d_o": 1.7e-07,            # 1.673e-07
        "nerf_chain.d_so": 4.1e-05,           # 4.095e-05
        "nerf_chain.dz_c1": 3.4e-05,          # 3.370e-05
        "nerf_chain.dz_c2": 5.0e-05,          # 4.998e-05
        "nerf_chain.dz_h1": 7.3e-05,          # 7.224e-05
        "nerf_head.d_enc": 5.9e-04,           # 5.845e-04
        "nerf_head.gwc0": 2.3e-06,            # 2.218e-06
        "nerf_head.gwc1": 4.7e-05,            # 4.644e-05
        "nerf_head.gwc2": 1.2e-05,            # 1.105e-05
        "nerf_head.gws0": 2.1e-05,            # 2.058e-05
        "nerf_head.gws1": 1.4e-05,            # 1.303e-05
    },
    "fp32": {
        "instance_chain.denc": 3.6e-07,       # 3.582e-07
        "instance_chain.dz1": 3.4e-07,        # 3.316e-07
        "instance_chain.dz2": 3.2e-07,        # 3.170e-07
        "instance_head.d_enc": 4.2e-07,       # 4.129e-07
        "instance_head.gw0": 1.2e-08,         # 1.188e-08
        "instance_head.gw1": 1.1e-07,         # 1.004e-07
        "instance_head.gw2": 7.7e-08,         # 7.627e-08
        "nerf_chain.d_enc": 7.1e-07,          # 7.095e-07
        "nerf_chain.d_o": 1.7e-07,            # 1.673e-07
        "nerf_chain.d_so": 9.1e-07,           # 9.097e-07
        "nerf_chain.dz_c1": 2.9e-07,          # 2.852e-07
        "nerf_chain.dz_c2": 2.7e-07,          # 2.664e-07
        "nerf_chain.dz_h1": 1.2e-06,          # 1.114e-06
        "nerf_head.d_enc": 7.3e-06,           # 7.231e-06
        "nerf_head.gwc0": 1.5e-08,            # 1.482e-08
        "nerf_head.gwc1": 1.2e-06,            # 1.175e-06
        "nerf_head.gwc2": 3.3e-07,            # 3.239e-07
        "nerf_head.gws0": 2.1e-07,            # 2.054e-07
        "nerf_head.gws1": 1.6e-07,            # 1.521e-07
    },
}
TOL = {b: {k: 8.0 * v for k, v in m.items()} for b, m in MEASURED.items()}
TOL_BIG = {b: {k: 8.0 * v for k, v in m.items()} for b, m in MEASURED_BIG.items()}


def tolerance(build, name, size):
    """TOL of an output; at the three multi-round sizes the tighter TOL_BIG where one is measured."""
    if size in BIG_SIZES and name in TOL_BIG[build]:
        return TOL_BIG[build][name]
    return TOL[build][name]


# ---------------------------------------------------------------------------- number formats
def _f32(x):
    return np.asarray(x, F64).astype(F32)


def _bits_to_f64(u):
    return u.astype(np.uint32).view(F32).astype(F64)


def rne_bf16(x):
    """fp32 value -> nearest bf16 (ties to even), as float64."""
    u = _f32(x).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return _bits_to_f64(u)


def trunc_bf16(x):
    return _bits_to_f64(_f32(x).view(np.uint32) & np.uint32(0xFFFF0000))


def split_rne(x):
    hi = rne_bf16(x)
    return hi, rne_bf16(np.asarray(x, F64) - hi)


def split_trunc(x):
    hi = trunc_bf16(x)
    return hi, trunc_bf16(np.asarray(x, F64) - hi)


def sigbits(a):
    """Largest number of significant bits (first to last set bit of the significand) of the values of ``a``."""
    a = np.abs(np.asarray(a, F64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return 0
    m, _ = np.frexp(a)
    i = (m * 2.0 ** 53).astype(np.uint64)
    low = i & (~i + np.uint64(1))                           # lowest set bit
    return int(np.max(54 - np.log2(low.astype(F64)).astype(np.int64) - 1))


def quantum(a):
    """The largest power of two that divides every value of ``a`` (1.0 for an all-zero array)."""
    a = np.abs(np.asarray(a, F64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(a)
    i = (m * 2.0 ** 53).astype(np.uint64)
    low = np.log2((i & (~i + np.uint64(1))).astype(F64)).astype(np.int64)
    return float(2.0 ** int(np.min(low + e - 53)))


# ---------------------------------------------------------------------------- models of the arithmetic
def _grouped(pairs, cus, chunk):
    """sum_m G[m, :]^T X[m, :] of every (G, X) of ``pairs`` added up, in the launch's order: a workgroup takes 128
    samples per round; one MFMA adds ``chunk`` consecutive samples (float64 inside, the accumulator rounded to fp32
    after every instruction, the pairs of a chunk one after the other), round after round; k_*_wgrad_reduce then sums
    the workgroups g = slice, slice + 16, ... in each of 16 slices and the slices one after the other, all in fp32."""
    G0, X0 = pairs[0]
    M, no, ni = G0.shape[0], G0.shape[1], X0.shape[1]
    if M == 0:
        return np.zeros((no, ni), F64)
    nb = -(-M // 128)
    grid = min(nb, cus)
    rounds = -(-nb // grid)
    rows = rounds * grid * 128
    padded = []
    for G, X in pairs:
        Gp, Xp = np.zeros((rows, no), F64), np.zeros((rows, ni), F64)
        Gp[:M], Xp[:M] = G, X
        padded.append((Gp.reshape(rounds, grid, 128, no), Xp.reshape(rounds, grid, 128, ni)))
    acc = np.zeros((grid, no, ni), F32)
    for r in range(rounds):
        for c in range(0, 128, chunk):
            for Gp, Xp in padded:
                acc = (acc + np.matmul(Gp[r, :, c:c + chunk].transpose(0, 2, 1), Xp[r, :, c:c + chunk])).astype(F32)
    slices = [np.cumsum(acc[k::16], axis=0, dtype=F32)[-1] for k in range(min(16, grid))]
    return np.cumsum(np.stack(slices), axis=0, dtype=F32)[-1].astype(F64)


class Exact64:
    """float64.  With ``log`` a list, the operands of every contraction are appended to it as (kind, A, B)."""
    name = "float64"

    def __init__(self, log=None):
        self.log = log

    def r(self, x):
        return np.asarray(x, F64)

    def layer(self, W, x):                     # x [M, in], W [out, in] -> [M, out]
        if self.log is not None:
            self.log.append(("layer", np.asarray(W, F64), np.asarray(x, F64)))
        return x @ W.T

    def wgrad(self, G, X, cus, log=True):      # -> [out, in] = G^T X
        if self.log is not None and log:
            self.log.append(("wgrad", np.asarray(G, F64), np.asarray(X, F64)))
        return G.T @ X

    def exp(self, x):
        return np.exp(x)

    def sigmoid(self, o):
        return 1.0 / (1.0 + np.exp(-o))

    def sh(self, d):
        return sh64(d, 4)


class _Fp32Steps:
    log = None

    def r(self, x):
        return np.asarray(x, F64).astype(F32).astype(F64)

    def exp(self, x):                          # __expf: v_exp_f32(x * log2e)
        t = self.r(np.asarray(x, F64) * float(F32(1.4426950408889634)))
        return self.r(np.exp2(t))

    def sigmoid(self, o):                      # __frcp_rn(1.0f + __expf(-o))
        return self.r(1.0 / self.r(1.0 + self.exp(-np.asarray(o, F64))))

    def sh(self, d):
        return self.r(sh64(d, 4))


class SplitBf16(_Fp32Steps):
    name = "bf16x3"

    def layer(self, W, x):
        wh, wl = split_rne(W)
        xh, xl = split_trunc(x)
        return self.r(xh @ wh.T + xh @ wl.T + xl @ wh.T)

    def wgrad(self, G, X, cus, log=True):
        gh, gl = split_rne(G)
        xh, xl = split_rne(X)
        return _grouped([(gh, xh), (gl, xh), (gh, xl)], cus, 32)


class SeqFp32(_Fp32Steps):
    name = "fp32"

    def layer(self, W, x):
        W, x = np.asarray(W, F32), np.asarray(x, F32)
        acc = np.zeros((x.shape[0], W.shape[0]), F32)
        for k in range(W.shape[1]):                # product and sum each rounded to fp32
            acc += x[:, k:k + 1] * W[None, :, k]
        return acc.astype(F64)

    def wgrad(self, G, X, cus, log=True):
        return _grouped([(self.r(G), self.r(X))], cus, 4)


MODELS = {"bf16x3": SplitBf16, "fp32": SeqFp32}


# ---------------------------------------------------------------------------- the operations
def _relu(p):
    return np.where(p > 0, p, 0.0)


def _lin(mod, W, x, mask=None):
    """(value, cond) of x @ W^T, zero (cond 0) where ``mask`` is off."""
    v = mod.layer(W, x)
    c = np.abs(x) @ np.abs(np.asarray(W, F64)).T
    if mask is not None:
        v, c = np.where(mask, v, 0.0), np.where(mask, c, 0.0)
    return v, c


def _wg(mod, G, X, cus, log=True):
    return mod.wgrad(G, X, cus, log), np.abs(np.asarray(G, F64)).T @ np.abs(np.asarray(X, F64))


def nerf_forward(mod, enc, dirs, W):
    """-> dict of the forward's arrays: pre-activations p_h1, p_c1, p_c2 and their layer inputs' |x| @ |W|^T
    (n_h1, n_c1, n_c2), h1, so [M,16], cin [M,31], c1, c2, o [M,3], rgb."""
    ws0, ws1, wc0, wc1, wc2 = (np.asarray(w, F64) for w in W)
    enc, dirs = np.asarray(enc, F64), np.asarray(dirs, F64)
    f = {}
    f["p_h1"], f["n_h1"] = _lin(mod, ws0, enc)
    f["h1"] = _relu(f["p_h1"])
    f["so"] = mod.layer(ws1, f["h1"])
    f["cin"] = np.concatenate([mod.sh(dirs), f["so"][:, 1:]], 1)
    f["p_c1"], f["n_c1"] = _lin(mod, wc0, f["cin"])
    f["c1"] = _relu(f["p_c1"])
    f["p_c2"], f["n_c2"] = _lin(mod, wc1, f["c1"])
    f["c2"] = _relu(f["p_c2"])
    f["o"] = mod.layer(wc2, f["c2"])
    f["rgb"] = mod.sigmoid(f["o"])
    return f


def nerf_chain(mod, W, g_sigma, g_rgb, rgb, so, h1, c1, c2, density_scale):
    """k_nerf_bwd from the saved activations -> (out, cond): d_o [M,4], dz_c2, dz_c1, d_so [M,16], dz_h1, d_enc."""
    ws0, ws1, wc0, wc1, wc2 = (np.asarray(w, F64) for w in W)
    g_sigma, g_rgb, rgb = np.asarray(g_sigma, F64), np.asarray(g_rgb, F64), np.asarray(rgb, F64)
    M = len(g_sigma)
    out, cond = {}, {}
    d_o3 = mod.r(mod.r(g_rgb * rgb) * mod.r(1.0 - rgb))
    out["d_o"] = np.concatenate([d_o3, np.zeros((M, 1))], 1)
    cond["d_o"] = np.abs(g_rgb * rgb * (1.0 - rgb))
    cond["d_o"] = np.concatenate([cond["d_o"], np.zeros((M, 1))], 1)
    out["dz_c2"], cond["dz_c2"] = _lin(mod, wc2.T, d_o3, np.asarray(c2) > 0)
    out["dz_c1"], cond["dz_c1"] = _lin(mod, wc1.T, out["dz_c2"], np.asarray(c1) > 0)
    d_geo, c_geo = _lin(mod, wc0[:, 16:].T, out["dz_c1"])
    so0 = np.clip(np.asarray(so, F64)[:, 0], -15.0, 15.0)
    d_so0 = mod.r(mod.r(g_sigma * float(F32(density_scale))) * mod.exp(so0))
    out["d_so"] = np.concatenate([d_so0[:, None], d_geo], 1)
    cond["d_so"] = np.concatenate([np.abs(g_sigma * float(F32(density_scale)) * np.exp(so0))[:, None], c_geo], 1)
    out["dz_h1"], cond["dz_h1"] = _lin(mod, ws1.T, out["d_so"], np.asarray(h1) > 0)
    out["d_enc"], cond["d_enc"] = _lin(mod, ws0.T, out["dz_h1"])
    return out, cond


def nerf_head(mod, case, cus=NOMINAL_CUS):
    """inr_nerf_head_backward -> (out, cond, forward, chain): d_enc [M,32], gws0 [64,32], gws1 [16,64], gwc0 [64,31],
    gwc1 [64,64], gwc2 [16,64]; ``chain`` are the (out, cond) of nerf_chain on this model's own activations."""
    enc = np.asarray(case["enc"], F64)
    f = nerf_forward(mod, enc, case["dirs"], case["W"])
    ch, cc = nerf_chain(mod, case["W"], case["g_sigma"], case["g_rgb"], f["rgb"], f["so"], f["h1"], f["c1"], f["c2"],
                        case["density_scale"])
    out, cond = {"d_enc": ch["d_enc"]}, {"d_enc": cc["d_enc"]}
    out["gwc2"], cond["gwc2"] = _wg(mod, np.concatenate([ch["d_o"], np.zeros((len(enc), 12))], 1), f["c2"], cus)
    out["gwc1"], cond["gwc1"] = _wg(mod, ch["dz_c2"], f["c1"], cus)
    out["gwc0"], cond["gwc0"] = _wg(mod, ch["dz_c1"], f["cin"], cus, log=False)
    if mod.log is not None:                    # the SH columns are no exact-tier product
        mod.log.append(("wgrad", ch["dz_c1"], f["cin"][:, 16:]))
    out["gws1"], cond["gws1"] = _wg(mod, ch["d_so"], f["h1"], cus)
    out["gws0"], cond["gws0"] = _wg(mod, ch["dz_h1"], enc, cus)
    return out, cond, f, (ch, cc)


def instance_forward(mod, enc, W):
    w0, w1, w2 = (np.asarray(w, F64) for w in W)
    f = {}
    f["p_h1"], f["n_h1"] = _lin(mod, w0, np.asarray(enc, F64))
    f["h1"] = _relu(f["p_h1"])
    f["p_h2"], f["n_h2"] = _lin(mod, w1, f["h1"])
    f["h2"] = _relu(f["p_h2"])
    return f


def instance_chain(mod, W, g, h1, h2):
    """k_instance_bwd from the saved activations and grad_logits [M,K] -> (out, cond): dz2, dz1, denc."""
    w0, w1, w2 = (np.asarray(w, F64) for w in W)
    out, cond = {}, {}
    out["dz2"], cond["dz2"] = _lin(mod, w2.T, np.asarray(g, F64), np.asarray(h2) > 0)
    out["dz1"], cond["dz1"] = _lin(mod, w1.T, out["dz2"], np.asarray(h1) > 0)
    out["denc"], cond["denc"] = _lin(mod, w0.T, out["dz1"])
    return out, cond


def instance_rows(case):
    """Number of rows the launch uses: min(n, M), M without a device-side count."""
    M = len(case["enc"])
    return M if case["n"] is None else max(0, min(int(case["n"]), M))


def instance_head(mod, case, cus=NOMINAL_CUS):
    """inr_instance_head_backward -> (out, cond, forward): d_enc [M,32], gw0 [64,32], gw1 [64,64], gw2 [K,64].  Rows at
    or behind min(n, M) are never looked at (they may hold NaN)."""
    M, n = len(case["enc"]), instance_rows(case)
    enc = np.asarray(case["enc"], F64)[:n]
    a = 1.0 if case["scale_a"] is None else float(F32(case["scale_a"]))
    b = 1.0 if case["scale_b"] is None else float(F32(case["scale_b"]))
    w = mod.r(np.asarray(case["wbuf"], F64)[:n] * mod.r(a * b))
    ray = np.asarray(case["sample_ray"])[:n]
    g = mod.r(np.asarray(case["g_pix"], F64)[ray] * w[:, None])
    f = instance_forward(mod, enc, case["W"])
    ch, cc = instance_chain(mod, case["W"], g, f["h1"], f["h2"])
    out, cond = {}, {}
    out["d_enc"], cond["d_enc"] = np.zeros((M, 32)), np.zeros((M, 32))
    out["d_enc"][:n], cond["d_enc"][:n] = ch["denc"], cc["denc"]
    # the launch's grid comes from M, not from n: rows behind n are zero rows of the same blocks
    pad = lambda v: np.concatenate([v, np.zeros((M - n, v.shape[1]))], 0)
    out["gw2"], cond["gw2"] = _wg(mod, pad(g), pad(f["h2"]), cus)
    out["gw1"], cond["gw1"] = _wg(mod, pad(ch["dz2"]), pad(f["h1"]), cus)
    out["gw0"], cond["gw0"] = _wg(mod, pad(ch["dz1"]), pad(enc), cus)
    f["g"] = g
    return out, cond, f


# ---------------------------------------------------------------------------- comparison
def worst_ratio(got, ref, cond):
    """Largest |got - ref| / cond; inf if an element with cond == 0 is not exactly 0 (or anything is not finite)."""
    got, ref, cond = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(cond, F64)
    assert got.shape == ref.shape == cond.shape, (got.shape, ref.shape, cond.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    live = cond > 0
    if (got[~live] != 0).any():
        return float("inf")
    return float(np.max(np.abs(got - ref)[live] / cond[live])) if live.any() else 0.0


def exactness_violations(log):
    """The exact tier's preconditions on the operand pairs a float64 run has logged -> list of complaints."""
    bad = []
    for i, (kind, A, B) in enumerate(log):
        if kind == "layer":                    # an input whose weight column is all zero enters no product
            used = (A != 0).any(0)
            A, B = A[:, used], B[:, used]
        sa, sb = sigbits(A), sigbits(B)
        if max(sa, sb) > 16 or min(sa, sb) > 8:
            bad.append(f"{kind} {i}: {sa} x {sb} significant bits")
        total = np.abs(A).T @ np.abs(B) if kind == "wgrad" else np.abs(B) @ np.abs(A).T
        q = quantum(A) * quantum(B)
        if total.size and total.max() / q >= 2.0 ** 24:
            bad.append(f"{kind} {i}: sum |terms| = {total.max() / q:.3g} quanta")
    return bad


# ---------------------------------------------------------------------------- cases
def _rng(*key):
    return np.random.default_rng([int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:4], "little")])


def _u(rng, shape, s):
    return ((rng.random(shape, dtype=F32) * F32(2.0) - F32(1.0)) * F32(s)).astype(F32)


def _ambiguous(f, names):
    bad = np.zeros(len(f["p_" + names[0]]), bool)
    for n in names:
        bad |= (np.abs(f["p_" + n]) < MARGIN * f["n_" + n]).any(1)
    return bad


def _accept(rng, M, draw, forward, names):
    """The first M accepted candidates of ``draw(count)`` (dict of arrays, row 0 of every batch an all-zero enc) ->
    (arrays, acceptance rate)."""
    kept, seen, taken = [], 0, 0
    while taken < M or not kept:
        c = draw(max(64, (M - taken) * 3 // 2 + 32))
        ok = ~_ambiguous(forward(c), names)
        seen += len(ok)
        taken += int(ok.sum())
        kept.append({k: v[ok] for k, v in c.items()})
    arrays = {k: np.concatenate([p[k] for p in kept])[:M] for k in kept[0]}
    while M and arrays["enc"].any(1).all():                # no all-zero enc row among the kept ones: put one in
        c = draw(64)
        if not _ambiguous(forward(c), names)[0]:
            for k in arrays:
                arrays[k][M // 2] = c[k][0]
    return arrays, taken / seen


def nerf_weights(rng):
    W = [_u(rng, (64, 32), 0.35), _u(rng, (16, 64), 0.25), _u(rng, (64, 31), 0.35), _u(rng, (64, 64), 0.25),
         _u(rng, (3, 64), 0.25)]
    W[1][0] = (W[1][0] - W[1][0].mean()) * F32(SO0_SCALE)      # centred: so0 leaves [-15, 15] on both sides
    return W


def nerf_tol_case(M, seed=0, density_scale=1.0):
    rng = _rng("nerf_tol", M, seed)
    W = nerf_weights(rng)

    def draw(count):
        enc = _u(rng, (count, 32), 1.0)
        enc[0] = 0.0
        d = rng.standard_normal((count, 3))
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
        return {"enc": enc, "dirs": d}

    a, rate = _accept(rng, M, draw, lambda c: nerf_forward(Exact64(), c["enc"], c["dirs"], W), ("h1", "c1", "c2"))
    return dict(kind="nerf", tier="tol", W=W, enc=a["enc"], dirs=a["dirs"], density_scale=density_scale,
                g_sigma=rng.standard_normal(M).astype(F32), g_rgb=rng.standard_normal((M, 3)).astype(F32), rate=rate)


def _rays(rng, M):
    """(N, sample_ray): unsorted, every fifth ray without a sample, every index in range."""
    N = max(1, M // 4) + 3
    live = np.asarray([r for r in range(N) if r % 5 != 4], np.int32)
    return N, live[rng.integers(0, len(live), size=M)].astype(np.int32)


def instance_tol_case(M, K, seed=0, scales=(None, None), n=None):
    rng = _rng("instance_tol", M, K, seed)
    W = [_u(rng, (64, 32), 0.35), _u(rng, (64, 64), 0.25), _u(rng, (K, 64), 0.25)]

    def draw(count):
        enc = _u(rng, (count, 32), 1.0)
        enc[0] = 0.0
        return {"enc": enc}

    a, rate = _accept(rng, M, draw, lambda c: instance_forward(Exact64(), c["enc"], W), ("h1", "h2"))
    N, ray = _rays(rng, M)
    return dict(kind="instance", tier="tol", K=K, W=W, enc=a["enc"], N=N, sample_ray=ray,
                g_pix=rng.standard_normal((N, K)).astype(F32), wbuf=rng.random(M, dtype=F32),
                scale_a=scales[0], scale_b=scales[1], n=n, rate=rate)


def _sparse(rng, rows, cols, values=(-1.0, 1.0)):
    """Two to three non-zeros per row, drawn from ``values``."""
    W = np.zeros((rows, cols), F32)
    for r in range(rows):
        k = int(rng.integers(2, 4))
        W[r, rng.choice(cols, size=k, replace=False)] = rng.choice(values, size=k)
    return W


def _twelve(rng, shape, scale=2.0 ** -10):
    """Values with 12 significant bits: odd integers in +-(2^11 .. 2^12) times ``scale``."""
    v = (rng.integers(2 ** 10, 2 ** 11, size=shape) * 2 + 1) * rng.choice((-1.0, 1.0), size=shape)
    return (v * scale).astype(F32)


def instance_exact_case(M, K, variant="int", seed=0, scales=(None, None), n=None):
    """variant int | enc12 (12-bit enc, +-1 weights) | w12 (12-bit W0, enc in {-1,0,1}) | g12 (12-bit g_pix)."""
    rng = _rng("instance_exact", M, K, variant, seed)
    W = [_sparse(rng, 64, 32), _sparse(rng, 64, 64), _sparse(rng, K, 64)]
    enc = rng.integers(-2, 3, size=(M, 32)).astype(F32)
    N, ray = _rays(rng, M)
    g_pix = rng.integers(-1, 2, size=(N, K)).astype(F32)
    wbuf = rng.choice(np.asarray((0.0, 0.5, 1.0, 2.0), F32), size=M)
    if variant == "enc12":
        enc = np.where(rng.random((M, 32)) < 0.5, _twelve(rng, (M, 32)), 0.0).astype(F32)
    elif variant == "w12":
        enc = rng.integers(-1, 2, size=(M, 32)).astype(F32)
        W[0] = (W[0] * np.abs(_twelve(rng, (64, 32)))).astype(F32)
    elif variant == "g12":
        g_pix = np.where(rng.random((N, K)) < 0.25, _twelve(rng, (N, K)), 0.0).astype(F32)
        wbuf = rng.choice(np.asarray((0.0, 1.0, 2.0), F32), size=M)
    if M:
        enc[M // 2] = 0.0
    return dict(kind="instance", tier="exact", K=K, W=W, enc=enc, N=N, sample_ray=ray, g_pix=g_pix, wbuf=wbuf,
                scale_a=scales[0], scale_b=scales[1], n=n)


def nerf_exact_case(M, variant="a", seed=0, density_scale=1.0, twelve=None):
    """variant a | b | c (see the module text); twelve: None | enc12 | w12 | g12."""
    rng = _rng("nerf_exact", M, variant, seed, twelve)
    ws0, ws1 = _sparse(rng, 64, 32), _sparse(rng, 16, 64)
    enc = rng.integers(-2, 3, size=(M, 32)).astype(F32)
    if twelve == "enc12":
        enc = np.where(rng.random((M, 32)) < 0.5, _twelve(rng, (M, 32)), 0.0).astype(F32)
    elif twelve == "w12":
        enc = rng.integers(-1, 2, size=(M, 32)).astype(F32)
        ws0 = (ws0 * np.abs(_twelve(rng, (64, 32)))).astype(F32)
    # so0 == 0 ON THE DATA with a live gradient: enc columns 2i, 2i+1 are equal (i < 8), the hidden units 2i, 2i+1 have
    # equal rows up to swapping those two columns, and the density row holds +s_i, -s_i on them
    enc[:, 1:16:2] = enc[:, 0:16:2]
    ws1[0] = 0.0
    for i in range(8):
        a, b = 2 * i, 2 * i + 1
        ws0[a, a], ws0[a, b] = abs(ws0[a, a]) if ws0[a, a] else 1.0, 0.0
        ws0[b] = ws0[a]
        ws0[b, a], ws0[b, b] = ws0[a, b], ws0[a, a]
        ws1[0, a], ws1[0, b] = (1.0, -1.0) if i % 2 else (-1.0, 1.0)
    wc0 = np.zeros((64, 31), F32)
    wc0[:, 16:] = _sparse(rng, 64, 15)
    wc1 = _sparse(rng, 64, 64)
    wc2 = np.zeros((3, 64), F32)
    u, v, p, pp = 5, 9, 3, 7
    wc1[u] = np.abs(wc1[u])                               # unit u is live on most samples
    if variant == "b":
        wc1[v] = wc1[u]
    elif variant == "c":
        ws1[1, 0], ws1[1, 1] = 1.0, 0.0
        ws1[2] = ws1[1]                                   # geo features 1 and 2 (columns 16, 17 of cin) are equal
        ws1[2, 0], ws1[2, 1] = 0.0, 1.0                   # ... on the data: h1[:, 0] == h1[:, 1]
        wc0[p, 16:18], wc0[pp, 16:18] = (1.0, 0.0), (0.0, 1.0)
        wc0[pp, 18:] = wc0[p, 18:]                         # c1[p] == c1[pp] on the data
        wc1[u, p], wc1[u, pp] = 1.0, 0.0
        wc1[v] = wc1[u]
        wc1[v, p], wc1[v, pp] = 0.0, 1.0                   # c2[u] == c2[v] on the data
    if variant in ("b", "c"):
        for ch, s in enumerate((1.0, -1.0, 1.0)):
            wc2[ch, u], wc2[ch, v] = s, -s
    d = rng.standard_normal((M, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    g_sigma = rng.integers(-2, 3, size=M).astype(F32)
    g_rgb = rng.integers(-2, 3, size=(M, 3)).astype(F32)
    if twelve == "g12":
        g_sigma = np.where(rng.random(M) < 0.5, _twelve(rng, M), 0.0).astype(F32)
        g_rgb = np.where(rng.random((M, 3)) < 0.25, _twelve(rng, (M, 3)), 0.0).astype(F32)
    if M:
        enc[M // 2] = 0.0
    return dict(kind="nerf", tier="exact", variant=variant, W=[ws0, ws1, wc0, wc1, wc2], enc=enc, dirs=d,
                density_scale=density_scale, g_sigma=g_sigma, g_rgb=g_rgb)


# ---------------------------------------------------------------------------- the case lists
# (id, constructor) - the constructor takes the device's CU count.  n: None | "M-37" | 0 | "M+5".
def _n(spec, M):
    return None if spec is None else (M - 37 if spec == "M-37" else (M + 5 if spec == "M+5" else int(spec)))


def _instance_specs():
    specs = []
    n_of = {127: "M-37", 128: 0, 129: "M-37", 17: "M+5", "16R+1": "M-37", "32R+151": "M-37"}
    sc_of = {15: (0.5, None), 16: (None, 4.0), 127: (0.25, 8.0), "16R-5": (0.5, 0.5), "32R+151": (2.0, 0.125)}
    for i, size in enumerate(SIZES):
        specs.append(("exact", "int", size, KS[i % 4], sc_of.get(size, (None, None)), n_of.get(size)))
    for v, K in (("enc12", 48), ("w12", 16), ("g12", 64), ("enc12", 32)):
        specs.append(("exact", v, 150, K, (0.5, 2.0) if v == "w12" else (None, None), None))
    tol_sc = {16: (0.37, None), 127: (None, 1.0 / 3.0), 129: (0.01, 12.5), "16R+1": (1.0 / 4096, 3.0)}
    for i, size in enumerate(SIZES):
        specs.append(("tol", "tol", size, KS[(i + 1) % 4], tol_sc.get(size, (None, None)), n_of.get(size)))
    for K in KS:                                          # every K at a two-workgroup size in the tolerance tier
        specs.append(("tol", "tol", 300 + K, K, (None, None), "M-37" if K == 32 else None))
    return specs


def instance_cases():
    out = []
    for tier, variant, size, K, scales, n in _instance_specs():
        def make(cus, tier=tier, variant=variant, size=size, K=K, scales=scales, n=n):
            M = resolve(size, cus)
            if tier == "exact":
                return instance_exact_case(M, K, variant, 0, scales, _n(n, M))
            return instance_tol_case(M, K, 0, scales, _n(n, M))
        out.append((f"{tier}-{variant}-M{size}-K{K}-n{n}-s{'y' if scales != (None, None) else 'n'}", make))
    return out


def _nerf_specs():
    specs = []
    for i, size in enumerate(SIZES):
        specs.append(("exact", "abc"[i % 3], None, size, 0.5 if i % 2 else 1.0))
    for v, tw in (("a", "enc12"), ("b", "w12"), ("c", "g12"), ("c", "enc12")):
        specs.append(("exact", v, tw, 150, 0.5 if tw == "w12" else 1.0))
    for i, size in enumerate(SIZES):
        specs.append(("tol", "tol", None, size, 1.0 if i % 2 else 0.5))
    return specs


def nerf_cases():
    out = []
    for tier, variant, tw, size, ds in _nerf_specs():
        def make(cus, tier=tier, variant=variant, tw=tw, size=size, ds=ds):
            M = resolve(size, cus)
            return nerf_exact_case(M, variant, 0, ds, tw) if tier == "exact" else nerf_tol_case(M, 0, ds)
        out.append((f"{tier}-{variant}{'-' + tw if tw else ''}-M{size}-ds{ds}", make))
    return out


CHAIN_SIZES = SMALL_SIZES[1:] + ("16R+1",)            # the chain kernels return before launching at M = 0


def chain_inputs(case, mod=None):
    """The chain kernels' inputs for a head case: saved activations from the float64 forward ROUNDED TO fp32 (and, for
    the instance field, grad_logits = g_pix[ray] * w rounded to fp32, rows behind n dropped)."""
    e = Exact64()
    if case["kind"] == "nerf":
        f = nerf_forward(e, case["enc"], case["dirs"], case["W"])
        return {k: f[k].astype(F32) for k in ("rgb", "so", "h1", "c1", "c2")}
    full = dict(case, n=None)
    _, _, f = instance_head(e, full)
    return {"g": f["g"].astype(F32), "h1": f["h1"].astype(F32), "h2": f["h2"].astype(F32)}


def chain_reference(mod, case, saved):
    if case["kind"] == "nerf":
        return nerf_chain(mod, case["W"], case["g_sigma"], case["g_rgb"], saved["rgb"], saved["so"], saved["h1"],
                          saved["c1"], saved["c2"], case["density_scale"])
    return instance_chain(mod, case["W"], saved["g"], saved["h1"], saved["h2"])


def head_of(case):
    return nerf_head if case["kind"] == "nerf" else instance_head


def chain_applies(size):
    return size in CHAIN_SIZES


def measure_case(build, size, case, cus=NOMINAL_CUS):
    """The model of ``build`` against float64 on one tolerance-tier case -> (|model - float64| / cond per output name,
    worst pre-activation error / (|x| @ |W|^T), masks all equal)."""
    worst, pre, same_masks = {}, 0.0, True
    kind = case["kind"]
    ro, rc, rf = head_of(case)(Exact64(), case, cus)[:3]
    mo, _, mf = head_of(case)(MODELS[build](), case, cus)[:3]
    for k in ro:
        worst[f"{kind}_head.{k}"] = worst_ratio(mo[k], ro[k], rc[k])
    for p in ("h1", "h2", "c1", "c2"):
        if "p_" + p in rf and rf["p_" + p].size:
            live = rf["n_" + p] > 0
            pre = max(pre, float(np.max((np.abs(mf["p_" + p] - rf["p_" + p])[live] / rf["n_" + p][live]), initial=0.0)))
            same_masks &= bool(((mf["p_" + p] > 0) == (rf["p_" + p] > 0)).all())
    if chain_applies(size):
        saved = chain_inputs(case)
        co, cc = chain_reference(Exact64(), case, saved)
        mo, _ = chain_reference(MODELS[build](), case, saved)
        for k in co:
            worst[f"{kind}_chain.{k}"] = worst_ratio(mo[k], co[k], cc[k])
    return worst, pre, same_masks
