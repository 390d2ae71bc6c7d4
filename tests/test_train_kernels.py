"""The small kernels every training step runs through, on the GPU, against tests/train_kernels_reference.py:
Adam / EMA (k_adam, k_adam_tail, k_adam_multi, k_adam_set_hyper), the fused copy (k_copy_multi), the weight gradient
(k_linear_wgrad<N_OT, N_IT>, k_wgrad_reduce), SH (k_sh_fwd, k_sh_bwd, k_sh_table_q) and the cross entropy (k_ce_rows,
k_ce_scale).  Adam, the EMA, SH and the copy must EQUAL the fp32 restatements bit for bit (the library is built with
-ffp-contract=off and these kernels use only + - * / and sqrt); the weight gradient is exact on small integers in any
summation order; only the cross entropy (expf, logf) has a tolerance, calibrated against torch's fp32 CPU result.

Every buffer a kernel writes is a view inside a larger allocation with GUARD sentinel words (a NaN pattern) on either
side, which must come back unchanged.  Sizes that depend on the number of CUs are computed from the device."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_kernels_reference as ref  # noqa: E402
from kernel_harness import DEV, Buf, check, cu_count, stream  # noqa: E402

pytestmark = pytest.mark.gpu
f = np.float32
HYPER = dict(lr=1e-2, b1=0.9, b2=0.99, eps=1e-15)
ADAM_GRID = 4096 * 256                 # k_adam / k_adam_multi: at most 256*16 workgroups of 256 lanes, one float4 each
BIG = 4 * ADAM_GRID + 4 * 300 + 3      # 4 195 507 floats: 300 float4s on the second grid-stride trip and a 3-float tail


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


def same(buf, want, what):
    ref.assert_same_bits(buf.get(), np.asarray(want).reshape(buf.shape), what)
    buf.check_guards(what)


# ---------------------------------------------------------------------------- Adam, one tensor
def _adam_single(lib, n, offset, grad_scale, seed):
    p = ref.signed(seed, n)
    m, v = np.zeros(n, f), np.zeros(n, f)
    P, M, V = Buf(p, offset), Buf(m, offset), Buf(v, offset)
    for step in (1, 2, 3, 1000):
        g = ref.adam_grads(seed * 16 + step % 16, n)
        G = Buf(g, offset)
        check(lib.inr_adam_step(P.ptr, G.ptr, M.ptr, V.ptr, n, HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], step,
                                grad_scale, stream()), "adam_step")
        p, m, v = ref.adam32(p, g, m, v, step=step, grad_scale=grad_scale, **HYPER)
        what = f"n {n} offset {offset} grad_scale {grad_scale} step {step}"
        same(P, p, "p " + what), same(M, m, "m " + what), same(V, v, "v " + what)
        same(G, g, "g " + what)
    return p


@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 128, 0.0])
def test_adam_step_equals_the_restatement(lib, grad_scale):
    """inr_adam_step: p, m, v bit-equal to adam32 after steps 1, 2, 3 and then step 1000 (bias corrections ~1).
    Aligned, n = 1, 3 run k_adam_tail only, 4 and 1024 k_adam only, 5 ... 2049 both (tail of n % 4).  With the base
    pointers ONE FLOAT into the allocation the whole tensor goes through the 1024-wide k_adam_tail launches: one for
    n <= 1024, two for 1025, three for 2049 (start 0, 1024, 2048)."""
    for offset in (0, 1):
        for k, n in enumerate((1, 3, 4, 5, 1023, 1024, 1025, 2049)):
            p = _adam_single(lib, n, offset, grad_scale, seed=100 + k)
            assert grad_scale != 0.0 or ref.bit_mismatches(p, ref.signed(100 + k, n)) == 0     # zero moments: p stays


def test_adam_step_second_grid_stride_trip(lib):
    """k_adam launches at most 256*16 workgroups of 256 lanes, a float4 per lane per trip: n/4 > 4096*256 = 1 048 576
    enters the second trip.  n = 4*(4096*256) + 4*300 + 3 = 4 195 507: 300 float4s on the second trip, then a 3-float
    k_adam_tail launch."""
    assert BIG // 4 > ADAM_GRID and BIG % 4 == 3
    _adam_single(lib, BIG, 0, 1.0 / 128, seed=90)


# ---------------------------------------------------------------------------- Adam, many tensors in one launch
def _lengths(big):
    return [0, 1, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 4099, 65537, BIG if big else 2051, 4099]


OFFSET_VIEWS = (8, 13)                  # n = 257 and 65 537: p, g, m, v (and the shadow) all one float into their allocation
GRAD_ONLY_MISALIGNED = 15               # n = 4099: only the gradient is one float in
LR_ZERO = 11                            # n = 1025
LRS = [0.0 if t == LR_ZERO else 1e-3 * (t + 1) for t in range(16)]
SHADOWED = tuple(range(0, 16, 2))       # shadows for every second tensor (the big one and an offset view among them)


@functools.lru_cache(maxsize=None)
def _multi_reference(big, steps=3, grad_scale=1.0 / 128):
    """Inputs and the adam32 trajectory of the 16-tensor set, computed once: (p0[t], grads[step][t], after[step][t])."""
    ns = _lengths(big)
    p0 = [ref.signed(200 + t, n) for t, n in enumerate(ns)]
    state = [(p, np.zeros(len(p), f), np.zeros(len(p), f)) for p in p0]
    grads, after = [], []
    for step in range(1, steps + 1):
        gs = [ref.adam_grads(300 + 16 * step + t, n) for t, n in enumerate(ns)]
        state = [ref.adam32(p, g, m, v, LRS[t], HYPER["b1"], HYPER["b2"], HYPER["eps"], step, grad_scale)
                 for t, (g, (p, m, v)) in enumerate(zip(gs, state))]
        grads.append(gs), after.append(state)
    return p0, grads, after


class MultiState:
    """Device buffers of the 16-tensor set (guarded; offsets as OFFSET_VIEWS / GRAD_ONLY_MISALIGNED say)."""

    def __init__(self, big, shadows=None):
        self.ns = _lengths(big)
        p0 = _multi_reference(big)[0]
        off = [1 if t in OFFSET_VIEWS else 0 for t in range(16)]
        self.P = [Buf(p, o) for p, o in zip(p0, off)]
        self.M = [Buf(np.zeros(n, f), o) for n, o in zip(self.ns, off)]
        self.V = [Buf(np.zeros(n, f), o) for n, o in zip(self.ns, off)]
        self.S = [Buf(shadows[t], off[t]) if shadows is not None and t in SHADOWED else None for t in range(16)]
        self.goff = [1 if t in OFFSET_VIEWS or t == GRAD_ONLY_MISALIGNED else 0 for t in range(16)]
        for t in OFFSET_VIEWS:
            assert self.P[t].ptr % 16 == 4 and self.M[t].ptr % 16 == 4 and self.V[t].ptr % 16 == 4
        assert self.P[GRAD_ONLY_MISALIGNED].ptr % 16 == 0

    def load_grads(self, gs):
        self.G = [Buf(g, o) for g, o in zip(gs, self.goff)]
        assert self.G[GRAD_ONLY_MISALIGNED].ptr % 16 == 4

    @staticmethod
    def _ptrs(bufs):
        return (ctypes.c_void_p * 16)(*[b.ptr if b is not None else None for b in bufs])

    def args(self):
        return (16, self._ptrs(self.P), self._ptrs(self.G), self._ptrs(self.M), self._ptrs(self.V),
                (ctypes.c_int64 * 16)(*self.ns))

    def shadow_ptrs(self):
        return self._ptrs(self.S)

    def compare(self, want, what):
        for t, (p, m, v) in enumerate(want):
            w = f"{what} tensor {t} (n = {self.ns[t]})"
            same(self.P[t], p, "p " + w), same(self.M[t], m, "m " + w), same(self.V[t], v, "v " + w)

    def bits(self):
        return [b.whole.clone() for b in self.P + self.M + self.V + [s for s in self.S if s is not None]]


def _floats(vals):
    return (ctypes.c_float * len(vals))(*vals)


def test_adam_step_multi_equals_the_restatement(lib):
    """inr_adam_step_multi, ONE launch of 16 tensors, three steps, grad_scale 1/128; p, m, v bit-equal to adam32 per
    tensor.  Lengths 0 (null pointers), 1, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 4099, 65 537, 4 195 507, 4099.
    The grid is min(n_max/4/256 + 1, 4096) = 4096 workgroups per tensor, so the 4 195 507-float tensor (n/4 = 1 048 876
    > 4096*256) makes the second trip of the float4 loop and ends in a 3-float scalar tail.  Tensors 8 and 13 are views
    one float into their allocations (``aligned == false``: the scalar loop does everything, as for offset views of a
    sharded table); tensor 15 has only its GRADIENT misaligned and must still be right as a whole.  The learning rates
    are all different; tensor 11 has lr 0: its parameter keeps its bits while its moments advance."""
    p0, grads, after = _multi_reference(True)
    st = MultiState(True)
    for step in (1, 2, 3):
        st.load_grads(grads[step - 1])
        check(lib.inr_adam_step_multi(*st.args(), _floats(LRS), HYPER["b1"], HYPER["b2"], HYPER["eps"], step, 1.0 / 128,
                                      stream()), "adam_step_multi")
        st.compare(after[step - 1], f"step {step}")
    assert ref.bit_mismatches(after[2][LR_ZERO][0], p0[LR_ZERO]) == 0 and np.abs(after[2][LR_ZERO][1]).min() > 0
    assert len(set(LRS)) == 16


@pytest.mark.parametrize("ema_w", [0.0, 0.05, 1.0])
def test_adam_ema_step_multi_equals_the_restatement(lib, ema_w):
    """inr_adam_ema_step_multi on the same 16 tensors with shadows for tensors 0, 2, ..., 14 (tensor 0 is empty, 8 is
    an offset view, 14 the 4 195 507-float one) and null for the rest: shadows bit-equal to s + w*(p_new - s), p, m, v
    bit-equal to adam32 - for the tensors WITHOUT a shadow these are the bits of the launch without EMA
    (test_adam_step_multi_equals_the_restatement pins the same reference).  Weight 0 leaves every shadow's bits."""
    p0, grads, after = _multi_reference(True)
    shadows = [ref.signed(400 + t, n) for t, n in enumerate(_lengths(True))]
    st = MultiState(True, shadows)
    assert st.S[1] is None and st.S[14] is not None and st.S[8].ptr % 16 == 4
    for step in (1, 2, 3):
        st.load_grads(grads[step - 1])
        check(lib.inr_adam_ema_step_multi(*st.args(), _floats(LRS), HYPER["b1"], HYPER["b2"], HYPER["eps"], step,
                                          1.0 / 128, st.shadow_ptrs(), ema_w, stream()), "adam_ema_step_multi")
        st.compare(after[step - 1], f"ema {ema_w} step {step}")
        for t in SHADOWED:
            want = ref.ema32(shadows[t], after[step - 1][t][0], ema_w)
            if ema_w == 0.0:
                assert ref.bit_mismatches(want, shadows[t]) == 0
            same(st.S[t], want, f"shadow ema {ema_w} step {step} tensor {t}")
            shadows[t] = want


@pytest.mark.parametrize("with_ema", [False, True])
def test_adam_device_hyper_equals_host_hyper(lib, with_ema):
    """inr_adam_set_hyper + inr_adam_step_multi_dev (the scalars read from device memory: what a captured step replays)
    against inr_adam_step_multi, and the _ema pair likewise: all buffers bit-equal after each of four steps whose
    learning rates (and EMA weight) CHANGE from step to step.  The host form is pinned to adam32 here as well.  The
    hyper buffer has 18 floats: [eps_t, lr_t[0..15], ema weight], bit-equal to the host's folding; the non-EMA setter
    must leave slot 17 alone."""
    p0, grads, _ = _multi_reference(False, 4, 1.0)
    shadows = [ref.signed(400 + t, n) for t, n in enumerate(_lengths(False))] if with_ema else None
    a, b = MultiState(False, shadows), MultiState(False, shadows)
    hyper = Buf(np.full(18, 123.0, f))
    state = [(p, np.zeros(len(p), f), np.zeros(len(p), f)) for p in p0]
    for step in (1, 2, 3, 4):
        lrs = [lr * (1.0 - 0.2 * step) + (1e-4 if t == step else 0.0) for t, lr in enumerate(LRS)]
        w = 0.05 * step
        gs = grads[step - 1]
        a.load_grads(gs), b.load_grads(gs)
        tail = (HYPER["b1"], HYPER["b2"], HYPER["eps"], step)
        if with_ema:
            check(lib.inr_adam_ema_step_multi(*a.args(), _floats(lrs), *tail, 1.0, a.shadow_ptrs(), w, stream()))
            check(lib.inr_adam_set_hyper_ema(_floats(lrs), 16, *tail, w, hyper.ptr, stream()), "set_hyper_ema")
            check(lib.inr_adam_ema_step_multi_dev(*b.args(), hyper.ptr, HYPER["b1"], HYPER["b2"], 1.0, b.shadow_ptrs(),
                                                  stream()), "adam_ema_step_multi_dev")
        else:
            check(lib.inr_adam_step_multi(*a.args(), _floats(lrs), *tail, 1.0, stream()))
            check(lib.inr_adam_set_hyper(_floats(lrs), 16, *tail, hyper.ptr, stream()), "set_hyper")
            check(lib.inr_adam_step_multi_dev(*b.args(), hyper.ptr, HYPER["b1"], HYPER["b2"], 1.0, stream()),
                  "adam_step_multi_dev")
        for x, y in zip(a.bits(), b.bits()):
            assert torch.equal(x, y), f"step {step}: device-hyper and host-hyper launches differ"
        state = [ref.adam32(p, g, m, v, lrs[t], HYPER["b1"], HYPER["b2"], HYPER["eps"], step, 1.0)
                 for t, (g, (p, m, v)) in enumerate(zip(gs, state))]
        a.compare(state, f"host hyper step {step}"), b.compare(state, f"device hyper step {step}")
        scal = [ref.adam_scalars(lr, HYPER["b1"], HYPER["b2"], HYPER["eps"], step) for lr in lrs]
        want = np.asarray([scal[0][5]] + [s[4] for s in scal] + [f(w) if with_ema else f(123.0)], f)
        same(hyper, want, f"hyper buffer step {step}")
    if with_ema:
        for t in SHADOWED:
            assert ref.bit_mismatches(a.S[t].get(), b.S[t].get()) == 0 and (t == 0 or (a.S[t].get() != shadows[t]).any())


# ---------------------------------------------------------------------------- FusedAdam
FUSED_SHAPES = [(5,), (64, 32), (7,), (1003,), (3, 3), (1,), (16, 16), (33,), (2, 5, 7), (4,), (129,), (64,), (31, 3),
                (8, 8), (257,), (1024,), (6,), (12, 11), (2,)]


def _fused_setup():
    from instance_nerf_amd.nerf.utils import FusedAdam
    p0 = [ref.signed(500 + k, int(np.prod(s))).reshape(s) for k, s in enumerate(FUSED_SHAPES)]
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(DEV)) for p in p0]
    groups = [{"params": ps[:10], "lr": 1e-2}, {"params": ps[10:], "lr": 3e-3}]
    return p0, ps, groups, FusedAdam(groups)


def test_fused_adam_two_launches_and_a_missing_gradient(lib):
    """FusedAdam over 19 parameters (launches of 16 and 3), two learning rates, step(grad_scale=1/128): bit-equal to
    adam32.  Parameter 4 has grad = None in step 2: its data and moments keep their bits in that step, and step 3
    updates it with the optimiser's step count 3."""
    p0, ps, groups, opt = _fused_setup()
    assert len(ps) == 19
    state = [(p, np.zeros_like(p), np.zeros_like(p)) for p in p0]
    for step in (1, 2, 3):
        gs = [ref.adam_grads(600 + 32 * step + k, p.size).reshape(p.shape) for k, p in enumerate(p0)]
        for k, p in enumerate(ps):
            p.grad = None if (step == 2 and k == 4) else torch.from_numpy(gs[k]).to(DEV)
        before = [t.clone() for t in (ps[4].data, opt.state[ps[4]]["exp_avg"], opt.state[ps[4]]["exp_avg_sq"])] if step == 2 else None
        opt.step(grad_scale=1.0 / 128)
        if step == 2:
            for x, y in zip(before, (ps[4].data, opt.state[ps[4]]["exp_avg"], opt.state[ps[4]]["exp_avg_sq"])):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        for k, (p, m, v) in enumerate(state):
            if not (step == 2 and k == 4):
                state[k] = ref.adam32(p, gs[k], m, v, 1e-2 if k < 10 else 3e-3, 0.9, 0.99, 1e-15, step, 1.0 / 128)
            got = (ps[k].data, opt.state[ps[k]]["exp_avg"], opt.state[ps[k]]["exp_avg_sq"])
            for name, x, y in zip("pmv", got, state[k]):
                ref.assert_same_bits(x.cpu().numpy(), y, f"{name} of parameter {k} step {step}")


def test_fused_adam_plain_steps_match_torch_adam():
    """Three plain steps of the same 19 parameters within allclose(atol=1e-6, rtol=1e-5) of torch.optim.Adam (the
    bound of tests/test_gpu_parity.py::test_adam_matches_torch)."""
    p0, ps, groups, opt = _fused_setup()
    qs = [torch.from_numpy(p.copy()).requires_grad_(True) for p in p0]
    topt = torch.optim.Adam([{"params": qs[:10], "lr": 1e-2}, {"params": qs[10:], "lr": 3e-3}], betas=(0.9, 0.99), eps=1e-15)
    for step in (1, 2, 3):
        for k, (p, q) in enumerate(zip(ps, qs)):
            g = ref.normal(700 + 32 * step + k, q.numel()).astype(f).reshape(q.shape)
            p.grad, q.grad = torch.from_numpy(g).to(DEV), torch.from_numpy(g.copy())
        opt.step(), topt.step()
    for p, q in zip(ps, qs):
        assert torch.allclose(p.detach().cpu(), q.detach(), atol=1e-6, rtol=1e-5)


# ---------------------------------------------------------------------------- fused copies
def _words(seed, n):
    return (np.floor(ref.uniform(seed, n) * 2.0 ** 32) - 2.0 ** 31).astype(np.int64).astype(np.int32)


def _as(words, dtype):
    return words.view(dtype)


def test_copy_multi(lib):
    """inr_copy_multi, 8 jobs of 0 (null pointers), 1, 2, 255, 256, 257, 1024*256 + 1 and 1000 words; float32, int32
    and uint8 (byte counts divisible by 4); the 257- and the 262 145-word jobs have source AND destination at 4-byte
    (not 16-byte) offsets.  The grid is min(ceil(w_max/256), 1024) = 1024 workgroups of 256 lanes: word 1024*256 of the
    long job is the second trip of the stride loop.  Bytes equal, guards intact."""
    sizes = [0, 1, 2, 255, 256, 257, 1024 * 256 + 1, 1000]
    dtypes = [np.float32, np.int32, np.uint8, np.float32, np.uint8, np.int32, np.float32, np.uint8]
    off = [0, 0, 0, 0, 0, 1, 1, 0]
    src = [Buf(_as(_words(800 + k, n), dt), o) for k, (n, dt, o) in enumerate(zip(sizes, dtypes, off))]
    dst = [Buf(np.zeros(s.shape, s.dtype), o) for s, o in zip(src, off)]
    assert dst[6].ptr % 16 == 4 and src[6].ptr % 16 == 4 and dst[5].ptr % 16 == 4
    vp = lambda bufs: (ctypes.c_void_p * 8)(*[b.ptr for b in bufs])
    check(lib.inr_copy_multi(8, vp(dst), vp(src), (ctypes.c_int64 * 8)(*[4 * n for n in sizes]), stream()), "copy_multi")
    for k, (d, s) in enumerate(zip(dst, src)):
        assert d.t.dtype == s.t.dtype and torch.equal(d.raw, s.raw), f"job {k}"
        assert np.array_equal(d.get().view(np.uint8), _as(_words(800 + k, sizes[k]), np.uint8)), f"job {k}"
        d.check_guards(f"dst {k}"), s.check_guards(f"src {k}")


def test_copy_tensors_fused_and_fallback():
    """copy_tensors: 11 pairs that qualify for the fused kernel (launches of 8 and 3; float32, int32, uint8; one at a
    4-byte offset; one empty) and three that take dst.copy_(src): a non-contiguous destination, a 6-byte pair and a CPU
    pair.  Every destination equals its source; guards of the fused destinations intact."""
    from instance_nerf_amd.nerf.utils import copy_tensors
    sizes = [1, 2, 3, 255, 256, 257, 1000, 0, 4097, 64, 1025]
    dtypes = [np.float32, np.int32, np.uint8] * 4
    src = [Buf(_as(_words(900 + k, n), dt), k == 5) for k, (n, dt) in enumerate(zip(sizes, dtypes))]
    dst = [Buf(np.zeros(s.shape, s.dtype), k == 5) for k, s in enumerate(src)]
    pairs = [(d.t, s.t) for d, s in zip(dst, src)]
    strided = torch.zeros(20, device=DEV)[::2]
    six = torch.zeros(6, dtype=torch.uint8, device=DEV)
    on_cpu = torch.zeros(5)
    extra = [(strided, torch.arange(10, device=DEV, dtype=torch.float32) + 1),
             (six, torch.arange(6, dtype=torch.uint8, device=DEV) + 1), (on_cpu, torch.arange(5.0) + 1)]
    assert not strided.is_contiguous()
    copy_tensors(pairs[:4] + extra[:1] + pairs[4:9] + extra[1:] + pairs[9:])
    torch.cuda.synchronize()
    for k, (d, s) in enumerate(zip(dst, src)):
        assert torch.equal(d.raw, s.raw), f"pair {k}"
        d.check_guards(f"dst {k}")
    for d, s in extra:
        assert torch.equal(d, s) and float(s.sum()) > 0


# ---------------------------------------------------------------------------- weight gradient
SQUARE = [(o, i) for o in (16, 32, 48, 64) for i in (16, 32, 48, 64)]        # the 16 template instances, vector loads
RAGGED = [(1, 1), (3, 64), (15, 17), (31, 33), (47, 49), (63, 63), (64, 31)]
AT_4_BYTE_OFFSET = [(15, 17), (63, 63)]                                       # legal: neither width is a multiple of 16
SMALL_M = (0, 1, 15, 16, 17, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def _int_inputs(m_max):
    """x, gy in {-3..3} as int64 [m_max, 64] (sliced per case) and their fp32 copies on the device."""
    x, gy = ref.small_ints(1001, (m_max, 64), 3), ref.small_ints(1002, (m_max, 64), 3)
    return x, gy, torch.from_numpy(x.astype(f)).to(DEV), torch.from_numpy(gy.astype(f)).to(DEV)


def _at_offset(t, words):
    """A contiguous copy of ``t`` that starts ``words`` floats into a fresh allocation."""
    flat = torch.empty(t.numel() + words, dtype=t.dtype, device=t.device)
    out = flat[words:].view(t.shape)
    out.copy_(t)
    return out


def _wgrad_exact(lib, ws, n_out, n_in, Ms, m_max, offset=0):
    x, gy, xd, gyd = _int_inputs(m_max)
    for M in Ms:
        assert 9 * M + 5 < 2 ** 24                       # every partial sum is an integer fp32 holds exactly
        gw0 = ref.small_ints(1100 + n_out * 64 + n_in, (n_out, n_in), 5)
        GW = Buf(gw0.astype(f))
        xs, gys = _at_offset(xd[:M, :n_in], offset), _at_offset(gyd[:M, :n_out], offset)
        assert M == 0 or offset == 0 or (xs.data_ptr() % 16 == 4 and gys.data_ptr() % 16 == 4)
        ws.fill_nan()                                    # the reduce may read only what pass 1 wrote in THIS call
        check(lib.inr_linear_wgrad(xs.data_ptr() or None, gys.data_ptr() or None, M, n_in, n_out, GW.ptr, ws.ptr, stream()),
              "linear_wgrad")
        want = ref.wgrad_int(x[:M, :n_in], gy[:M, :n_out], gw0)
        what = f"n_out {n_out} n_in {n_in} M {M} offset {offset}"
        same(GW, want.astype(f), what)
        assert M > 0 or ref.bit_mismatches(GW.get(), gw0.astype(f)) == 0
        ws.check_guards("workspace " + what)


@pytest.fixture(scope="module")
def wgrad_ws(lib):
    n = lib.inr_linear_wgrad_workspace_bytes()
    assert n % 4 == 0 and n >= cu_count(lib) * 2 * 64 * 64 * 4
    return Buf(np.zeros(n // 4, f))


@pytest.mark.parametrize("n_out,n_in", SQUARE + RAGGED)
def test_linear_wgrad_exact_on_integers_small_m(lib, wgrad_ws, n_out, n_in):
    """inr_linear_wgrad with x, grad_y in {-3..3} and grad_w starting from {-5..5}: every partial sum is an integer
    below 2^24, any summation order is exact, the result must EQUAL the int64 product plus the start.  All 16
    k_linear_wgrad<N_OT, N_IT> instances (widths from {16, 32, 48, 64}^2: float4 / float2 / scalar row loads) and ragged
    widths; M = 0 (grad_w untouched), 1, 15, 16, 17 (one unit of 16 samples, ragged or not), 127, 128, 129 (one
    workgroup of 8 waves; a ninth unit).  The workspace is NaN before every call.  (15, 17) and (63, 63) run again
    with x and grad_y at a 4-byte offset."""
    _wgrad_exact(lib, wgrad_ws, n_out, n_in, SMALL_M, 129)
    if (n_out, n_in) in AT_4_BYTE_OFFSET:
        _wgrad_exact(lib, wgrad_ws, n_out, n_in, SMALL_M, 129, offset=1)


@pytest.mark.parametrize("n_out,n_in", [(64, 64), (16, 48), (48, 32), (31, 33)])
def test_linear_wgrad_exact_on_integers_large_m(lib, wgrad_ws, n_out, n_in):
    """The same at the sizes where the loops take another path, with C = CUs (256 on this part):
    M = 14 465: 905 units -> ceil(905/8) = 114 workgroups > 7*16: slices 0 and 1 of k_wgrad_reduce run one round of the
      8-deep unrolled loop (groups g, g+16, ..., g+112), the other slices only the remainder loop;
    M = C*256 + 17: the grid is capped at 2C workgroups = 16C waves; 16C + 2 units: waves 0 and 1 make a second
      grid-stride trip, the last unit holds one sample;
    M = 3*C*256 - 5: 48C units, three per wave, the last one ragged; 9*M + 5 = 1 769 432 < 2^24."""
    C = cu_count(lib)
    Ms = (14465, C * 256 + 17, 3 * C * 256 - 5)
    assert (Ms[0] + 15) // 16 > 8 * 112 and (Ms[1] + 15) // 16 > 16 * C and (Ms[2] + 15) // 16 == 48 * C
    _wgrad_exact(lib, wgrad_ws, n_out, n_in, Ms, Ms[2])


@pytest.mark.parametrize("n_out,n_in", [(64, 64), (31, 40)])
def test_linear_wgrad_floats_within_the_summation_bound(lib, wgrad_ws, n_out, n_in):
    """N(0,1) inputs, M = CUs*256 + 17, grad_w from zero, against the fp64 product: per element
    |err| <= (M + 2) * 2^-24 * sum_m |gy[m,o]| |x[m,i]| - the bound of a sum of M rounded products in ANY order
    (each partial sum carries at most one rounding per addition, M - 1 additions in a chain at the worst, plus the
    product's and the final accumulation's).  The integer tests carry the sensitivity; this keeps real inputs honest."""
    M = cu_count(lib) * 256 + 17
    x = ref.normal(1200 + n_in, M * n_in).reshape(M, n_in).astype(f)
    gy = ref.normal(1300 + n_out, M * n_out).reshape(M, n_out).astype(f)
    GW = Buf(np.zeros((n_out, n_in), f))
    xd, gyd = torch.from_numpy(x).to(DEV), torch.from_numpy(gy).to(DEV)
    wgrad_ws.fill_nan()
    check(lib.inr_linear_wgrad(xd.data_ptr(), gyd.data_ptr(), M, n_in, n_out, GW.ptr, wgrad_ws.ptr, stream()), "linear_wgrad")
    want = gy.astype(np.float64).T @ x.astype(np.float64)
    bound = (M + 2) * 2.0 ** -24 * (np.abs(gy).astype(np.float64).T @ np.abs(x).astype(np.float64))
    err = np.abs(GW.get().astype(np.float64) - want)
    print(f"wgrad floats ({n_out}, {n_in}): largest err / bound = {(err / bound).max():.2e}")
    assert (err <= bound).all()
    GW.check_guards(), wgrad_ws.check_guards()


# ---------------------------------------------------------------------------- SH
SH_M = (0, 1, 255, 256, 257, 5000)


@functools.lru_cache(maxsize=None)
def _sh_case(degree):
    d = ref.sh_directions(1400, 5000)
    go = ref.normal(1410 + degree, 5000 * degree * degree).reshape(5000, -1).astype(f)
    return d, go, ref.sh_fwd32(d, degree), ref.sh_bwd32(go, d, degree)


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_sh_forward_and_backward_equal_the_restatements(lib, degree):
    """inr_sh_encode_forward bit-equal to oracle.sh.sh_encode(d, degree), inr_sh_encode_backward bit-equal to sh_bwd32,
    degrees 1..4 (degree 1 writes zeros), M = 0, 1, 255, 256, 257 (one 256-lane workgroup, exactly, one more) and 5000;
    directions in the closed unit ball with the zero vector, the axes, -0.0 and short vectors in the first rows."""
    d, go, fwd, bwd = _sh_case(degree)
    C = degree * degree
    for M in SH_M:
        if M == 0:
            check(lib.inr_sh_encode_forward(None, 0, degree, None, stream()))
            check(lib.inr_sh_encode_backward(None, None, 0, degree, None, stream()))
            continue
        D, GO = Buf(d[:M]), Buf(go[:M])
        OUT, GD = Buf(np.zeros((M, C), f)), Buf(np.full((M, 3), 7.0, f))
        check(lib.inr_sh_encode_forward(D.ptr, M, degree, OUT.ptr, stream()), "sh_encode_forward")
        check(lib.inr_sh_encode_backward(GO.ptr, D.ptr, M, degree, GD.ptr, stream()), "sh_encode_backward")
        same(OUT, fwd[:M], f"sh forward degree {degree} M {M}")
        same(GD, bwd[:M], f"sh backward degree {degree} M {M}")
        if degree == 1:
            assert ref.bit_mismatches(GD.get(), np.zeros((M, 3), f)) == 0


@pytest.mark.parametrize("N", [1, 257])
def test_sh_table_q_is_the_forward_in_lane_order(lib, N):
    """inr_sh_table_q: out[n, 4q + ks] bit-equal to the degree-4 forward's [n, 4ks + q]."""
    d, _, fwd, _ = _sh_case(4)
    D, OUT = Buf(d[:N]), Buf(np.zeros((N, 16), f))
    check(lib.inr_sh_table_q(D.ptr, N, OUT.ptr, stream()), "sh_table_q")
    want = fwd[:N].reshape(N, 4, 4).transpose(0, 2, 1).reshape(N, 16)          # [n, ks, q] -> [n, q, ks]
    assert want[0, 4 * 1 + 2] == fwd[0, 4 * 2 + 1]
    same(OUT, want, f"sh_table_q N {N}")


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_sh_encoder_module_scales_and_reshapes(degree):
    """SHEncoder(degree)(x, size=2.0) on a [2, 3, 7, 3] input: values and autograd gradient equal the flat call on x/2,
    the gradient divided by 2 (a power of two: exact)."""
    from instance_nerf_amd.shencoder import SHEncoder
    enc = SHEncoder(degree=degree)
    x0 = (ref.sh_directions(1500, 42) * f(2.0)).reshape(2, 3, 7, 3)
    go = ref.normal(1510 + degree, 42 * degree * degree).reshape(2, 3, 7, -1).astype(f)
    x = torch.from_numpy(x0).to(DEV).requires_grad_(True)
    out = enc(x, size=2.0)
    assert tuple(out.shape) == (2, 3, 7, degree * degree)
    out.backward(torch.from_numpy(go).to(DEV))
    flat = torch.from_numpy(x0.reshape(-1, 3) / f(2.0)).to(DEV).requires_grad_(True)
    out_flat = enc(flat)
    out_flat.backward(torch.from_numpy(go.reshape(42, -1)).to(DEV))
    ref.assert_same_bits(out.detach().cpu().numpy().reshape(42, -1), out_flat.detach().cpu().numpy(), "values")
    ref.assert_same_bits(x.grad.cpu().numpy().reshape(42, 3), (flat.grad / 2).cpu().numpy(), "gradient")
    ref.assert_same_bits(out_flat.detach().cpu().numpy(), ref.sh_fwd32(x0.reshape(-1, 3) / f(2.0), degree), "flat values")


# ---------------------------------------------------------------------------- cross entropy
def _ce_case(lib, logits, labels, ignore_index, what):
    """Raw call (guarded buffers, twice: identical bits) and the autograd wrapper against fp64; -> err / allowed."""
    from instance_nerf_amd import raymarching
    N, K = logits.shape
    loss64, grad64, kept = ref.ce64(logits, labels, ignore_index)
    LG, LB = torch.from_numpy(logits).to(DEV), torch.from_numpy(labels).to(DEV)
    runs = []
    for _ in range(2):
        GR, ACC, LOSS = Buf(np.full((N, K), 9.0, f)), Buf(np.zeros(128, f)), Buf(np.zeros(1, f))
        check(lib.inr_cross_entropy(LG.data_ptr(), LB.data_ptr(), N, K, ignore_index, GR.ptr, ACC.ptr, LOSS.ptr, stream()),
              "cross_entropy")
        runs.append((GR.get(), LOSS.get()))
        for b in (GR, ACC, LOSS):
            b.check_guards(what)
    assert ref.bit_mismatches(runs[0][0], runs[1][0]) == 0 and ref.bit_mismatches(runs[0][1], runs[1][1]) == 0, what
    a = LG.clone().requires_grad_(True)
    la = raymarching.cross_entropy(a, LB, ignore_index=ignore_index)
    assert ref.bit_mismatches(la.detach().cpu().numpy().reshape(1), runs[0][1]) == 0, what
    la.backward()
    assert ref.bit_mismatches(a.grad.cpu().numpy(), runs[0][0]) == 0, what
    grad, loss = runs[0][0], float(runs[0][1][0])
    if kept == 0:
        assert np.isnan(loss) and np.isnan(loss64) and ref.bit_mismatches(grad, np.zeros((N, K), f)) == 0, what
        return 0.0
    assert abs(loss - loss64) <= 1e-5 * max(1.0, abs(loss64)), (what, loss, loss64)
    _, grad32, _ = ref.ce64(logits, labels, ignore_index, dtype=torch.float32)
    delta = np.abs(grad32 - grad64).max()
    allowed = max(4.0 * delta, 2.0 ** -22)
    err = np.abs(grad.astype(np.float64) * kept - grad64).max()
    assert err <= allowed, (what, err, allowed, delta)
    ignored = labels == ignore_index
    assert not grad[ignored].any() and np.isfinite(grad).all(), what
    return err / allowed


def _ce_inputs(seed, N, K, scale, ignore_index):
    logits = (ref.normal(seed, N * K) * scale).astype(f).reshape(N, K)
    labels = np.minimum(np.floor(ref.uniform(seed + 1, N) * K), K - 1).astype(np.int64)
    labels[ref.uniform(seed + 2, N) < 0.2] = ignore_index
    return logits, labels


@pytest.mark.parametrize("ignore_index", [-1, -100, 255, 2])
@pytest.mark.parametrize("K", [1, 2, 63, 64])
def test_cross_entropy_against_fp64(lib, K, ignore_index):
    """raymarching.cross_entropy and the raw inr_cross_entropy against F.cross_entropy in fp64: K = 1, 2, 63, 64;
    N = 1, 3, 255, 256, 257 and, at K = 64, N = CUs*4*256/64 + 1 (k_ce_scale runs min(ceil(N*K/256), 4*CUs) workgroups
    of 256 lanes: N*K = CUs*4*256 + 64 elements make 64 lanes take a second trip; 4097 rows on this part, which also
    gives each of k_ce_rows' 256 waves more than one row); logits ~N(0,1) times 1e-3, 4 and 1e4 (the max-subtraction);
    one input with -inf in a non-label class of every row; about 20 % of the rows ignored; every row ignored (loss NaN,
    gradient all zeros).  ignore_index -1, -100, 255 (>= K) and 2, which is a valid class for K > 2: rows labelled 2 are
    dropped and nothing is poisoned (the loss stays finite).
    Loss within 1e-5 * max(1, |loss|).  Gradient: grad * kept (entries in [-1, 1]) within max(4*delta, 2^-22) of fp64,
    delta = the deviation of torch's fp32 CPU gradient, scaled the same way, on the same input; the 4x allows for
    expf / logf on the GPU being specified to ~1 ulp.  Two calls give identical bits (no atomics).
    Largest err / allowed seen on an MI355X (each case prints its own): 0.586, at K = 63; 0.417 at K = 64, 0.381 at
    K = 2, 0 at K = 1."""
    C = cu_count(lib)
    Ns = [1, 3, 255, 256, 257] + ([C * 4 * 256 // 64 + 1] if K == 64 else [])
    worst = 0.0
    for N in Ns:
        for s, scale in enumerate((1e-3, 4.0, 1e4)):
            logits, labels = _ce_inputs(2000 + 7 * N + s, N, K, scale, ignore_index)
            worst = max(worst, _ce_case(lib, logits, labels, ignore_index, f"K {K} N {N} scale {scale} ignore {ignore_index}"))
    if K >= 2:
        logits, labels = _ce_inputs(2100 + K, 257, K, 4.0, ignore_index)
        y = np.where(labels == ignore_index, 0, labels)
        logits[np.arange(257), (y + 1) % K] = -np.inf
        worst = max(worst, _ce_case(lib, logits, labels, ignore_index, f"K {K} -inf ignore {ignore_index}"))
    logits, labels = _ce_inputs(2200 + K, 5, K, 4.0, ignore_index)
    _ce_case(lib, logits, np.full(5, ignore_index, np.int64), ignore_index, f"K {K} all ignored")
    print(f"cross entropy K {K} ignore_index {ignore_index}: largest gradient err / allowed = {worst:.3f}")
