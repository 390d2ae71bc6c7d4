"""The confusion kernels on the GPU (csrc/confusion.hip), through the raw C ABI with guarded buffers and through
instance_nerf_amd.metrics / SegmentationMeter / Trainer.evaluate_segmentation, against tests/confusion_reference.py.

Everything is exact: every integer of counts and ignored equals the restatement's; two calls into zeroed buffers give the
same bits and a second call into the same buffers exactly twice the counts; guard words around every buffer are intact.

Sizes are the smallest at which a piece can go wrong, with RUN = the pixels of one workgroup (1024) and 64 a wave: one
pixel; a wave less one, a wave, a wave and one; RUN - 1, RUN, RUN + 1 (a second workgroup of one pixel); for the logits
entry also the step of the LDS stage (128 pixels at K = 64, 512 at K = 13, 1024 at K <= 3) plus one, and more than two
runs.  K = 1, 2, 33, 64 (ids) and 1, 3, 13, 64 (logits: K = 64 takes the 16-byte loads, also with ld = 68 and, from a base
that is only 4-byte aligned, the 4-byte loads).

Seen on the MI355X: all 22 cases equal, 5 s in all; the untrained 16-channel field of the Trainer test scores
miou_gt_ids 0.012677011272223818 through evaluate_segmentation and through evaluate with the default MIoUMeter.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import confusion_reference as cr  # noqa: E402
from test_confusion_cpu import argmax_rows, ids_case, padded, random_views  # noqa: E402
from kernel_harness import DEV, Buf, check, stream  # noqa: E402

pytestmark = pytest.mark.gpu
i32, f32 = np.int32, np.float32
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


def run_len():
    from instance_nerf_amd import _lib
    assert _lib.CONFUSION_PIXELS_PER_WG % _lib.CONFUSION_BLOCK == 0
    return _lib.CONFUSION_PIXELS_PER_WG


class Out:
    """Zeroed int64 counts [B, K, K+1] and ignored [B] inside guarded allocations (Buf holds 32-bit words)."""

    def __init__(self, B, K):
        self.shape = (B, K, K + 1)
        self.counts, self.ignored = Buf(np.zeros((B * K * (K + 1) * 2,), i32)), Buf(np.zeros((B * 2,), i32))
        assert self.counts.ptr % 8 == 0 and self.ignored.ptr % 8 == 0

    def get(self):
        self.counts.check_guards("counts")
        self.ignored.check_guards("ignored")
        return self.counts.get().view(np.int64).reshape(self.shape), self.ignored.get().view(np.int64)


def run_ids(lib, p, t, K, out=None):
    B, N = t.shape
    out = out or Out(B, K)
    P, T = Buf(p.astype(i32)), Buf(t.astype(i32))
    check(lib.inr_confusion_ids(P.ptr, T.ptr, B, N, K, out.counts.ptr, out.ignored.ptr, stream()), "confusion_ids")
    P.check_guards("pred")
    T.check_guards("truth")
    return out.get()


def run_logits(lib, x, t, K, out=None, offset=0):
    B, N, ld = x.shape
    out = out or Out(B, K)
    X, T = Buf(x.astype(f32), offset), Buf(t.astype(i32))
    check(lib.inr_confusion_logits(X.ptr, T.ptr, B, N, K, ld, out.counts.ptr, out.ignored.ptr, stream()), "confusion_logits")
    X.check_guards("logits")
    T.check_guards("truth")
    return out.get()


def equal(got, want, what):
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]), what + " counts"
    assert np.array_equal(got[1], want[1]), what + " ignored"


def id_sizes():
    R = run_len()
    return [1, 63, 64, 65, R - 1, R, R + 1]


# ---------------------------------------------------------------------------- ids entry
@pytest.mark.parametrize("K", [1, 2, 33, 64])
def test_ids_random_and_out_of_range_on_both_sides(lib, K):
    for N in id_sizes():
        p, t = ids_case(3, N, K, seed=7 * N + K)             # three images of different content; 20 % out of range each
        want = cr.confusion_np(p, t, K)
        if N <= 65:
            equal(cr.confusion(p, t, K), want, "the two restatements")
        assert int(want[0].sum() + want[1].sum()) == 3 * N
        equal(run_ids(lib, p, t, K), want, f"K{K} N{N}")


@pytest.mark.parametrize("K", [1, 2, 33, 64])
def test_ids_one_pair_everywhere_and_everything_ignored(lib, K):
    for N in id_sizes():
        t = np.full((2, N), K - 1, i32)
        p = np.full((2, N), K // 2, i32)
        got = run_ids(lib, p, t, K)                          # every lane of every wave on one counter
        want = np.zeros((2, K, K + 1), np.int64)
        want[:, K - 1, K // 2] = N
        equal(got, (want, np.zeros(2, np.int64)), f"one pair K{K} N{N}")
        p[1] = -1                                            # image 1: every prediction outside -> column K
        want[1] = 0
        want[1, K - 1, K] = N
        equal(run_ids(lib, p, t, K), (want, np.zeros(2, np.int64)), f"column K, K{K} N{N}")
        for bad in (-1, -7, K, 2 ** 31 - 1, -2 ** 31):
            t[:] = bad
            equal(run_ids(lib, p, t, K), (np.zeros((2, K, K + 1), np.int64), np.full(2, N, np.int64)), f"ignored {bad} K{K} N{N}")


def test_ids_all_pairs(lib):
    """Every (t, p) cell of the largest matrix, column K included, with a different count each."""
    K = 64
    t, p = np.meshgrid(np.arange(K), np.arange(K + 1), indexing="ij")
    reps = 1 + (t * 7 + p * 3) % 5
    t, p = np.repeat(t.reshape(-1), reps.reshape(-1)), np.repeat(p.reshape(-1), reps.reshape(-1))
    order = np.random.default_rng(0).permutation(t.size)
    got = run_ids(lib, p[order][None], t[order][None], K)
    assert np.array_equal(got[0][0], reps) and got[1][0] == 0


# ---------------------------------------------------------------------------- logits entry
@pytest.mark.parametrize("K", [1, 3, 13, 64])
def test_logits_tie_nan_inf_and_signed_zero_rows(lib, K):
    rows = argmax_rows(K)
    want_arg = cr.argmax_logits(rows, K)
    assert np.array_equal(cr.argmax_logits_np(rows, K), want_arg)
    assert np.array_equal(torch.argmax(torch.from_numpy(rows), -1).numpy(), want_arg)
    reps = 70                                                # the special rows land in every lane position
    rows = np.tile(rows, (reps, 1))
    want_arg = np.tile(want_arg, reps)
    t = np.random.default_rng(K).integers(-1, K, (1, rows.shape[0]))
    want = cr.confusion_np(want_arg[None], t, K)
    for ld in (K, K + 3):
        got = run_logits(lib, padded(rows, ld)[None], t, K)
        equal(got, want, f"K{K} ld{ld}")


@pytest.mark.parametrize("K,lds", [(1, (1, 4)), (3, (3, 6)), (13, (13, 16)), (64, (64, 67, 68))])
def test_logits_random_at_every_size(lib, K, lds):
    R = run_len()
    rng = np.random.default_rng(K)
    for N in [1, 63, 64, 65, 129, 513, R - 1, R, R + 1, 2 * R + 130]:
        for ld in lds:
            x = rng.normal(size=(3, N, ld)).astype(f32)
            x[:, :, K:] = INF                                # padded channels would win if they were read
            t = rng.integers(-2, K + 1, (3, N))              # -2, -1 and K are ignored
            want = cr.confusion_np(cr.argmax_logits_np(x, K), t, K)
            equal(run_logits(lib, x, t, K), want, f"K{K} ld{ld} N{N}")
            if N in (65, R + 1):                             # a base that is 4- but not 16-byte aligned: the 4-byte loads
                equal(run_logits(lib, x, t, K, offset=1), want, f"K{K} ld{ld} N{N} offset 1")


def test_logits_one_pair_everywhere(lib):
    K, N = 64, run_len() + 1
    x = np.zeros((2, N, K), f32)
    x[:, :, 5] = 1.0
    got = run_logits(lib, x, np.full((2, N), 9, i32), K)
    want = np.zeros((2, K, K + 1), np.int64)
    want[:, 9, 5] = N
    equal(got, (want, np.zeros(2, np.int64)), "one pair")


# ---------------------------------------------------------------------------- contract checks, both entries
def test_two_calls_same_bits_and_accumulation(lib):
    K, N = 33, run_len() + 65
    p, t = ids_case(3, N, K, seed=3)
    x = np.random.default_rng(1).normal(size=(3, N, K + 3)).astype(f32)
    for name, call in (("ids", lambda out=None: run_ids(lib, p, t, K, out)),
                       ("logits", lambda out=None: run_logits(lib, x, t, K, out))):
        a, b = call(), call()
        equal(a, b, name + ": two calls")
        out = Out(3, K)
        call(out)
        twice = call(out)
        equal(twice, (2 * a[0], 2 * a[1]), name + ": a second call adds")
        assert int(a[0].sum() + a[1].sum()) == 3 * N


# ---------------------------------------------------------------------------- module and meter
def test_module_fused_equals_composable(lib):
    from instance_nerf_amd import metrics
    K = 13
    p, t = ids_case(2, 2 * run_len() + 5, K, seed=11)
    want = cr.confusion_np(p, t, K)
    for dtype in (torch.int64, torch.int32):
        P, T = torch.from_numpy(p).to(DEV, dtype), torch.from_numpy(t).to(DEV, dtype)
        fused = metrics.segmentation_confusion(P, T, K, fused=True)
        plain = metrics.segmentation_confusion(P, T, K, fused=False)
        assert fused[0].is_cuda and torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1])
        equal((fused[0].cpu().numpy(), fused[1].cpu().numpy()), want, f"module {dtype}")
    big = torch.tensor([[2 ** 32, 2 ** 32 + 1, -2 ** 40, 1]], device=DEV)         # 64-bit ids must not wrap into [0, K)
    c, ig = metrics.segmentation_confusion(torch.ones_like(big), big, K, fused=True)
    assert int(ig[0]) == 3 and int(c[0, 1, 1]) == 1 and int(c.sum()) == 1
    small = metrics.segmentation_confusion(P.to(torch.uint8), T.clamp(-1, K).to(torch.int8), K, fused=True)
    equal((small[0].cpu().numpy(), small[1].cpu().numpy()),
          cr.confusion_np(p.astype(np.uint8), np.clip(t, -1, K), K), "uint8 / int8")
    # logits without ties or NaN (torch.argmax on the GPU is only then bound to the contract's rule), [B, H, W, ld]
    x = torch.from_numpy(np.random.default_rng(2).normal(size=(2, 31, 37, K + 3)).astype(f32)).to(DEV)
    tt = torch.randint(-1, K, (2, 31, 37), device=DEV)
    fused = metrics.segmentation_confusion(x, tt, K, fused=True)
    plain = metrics.segmentation_confusion(x, tt, K, fused=False)
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1]) and int(fused[0].sum() + fused[1].sum()) == 2 * 31 * 37
    out = (torch.zeros_like(fused[0]), torch.zeros_like(fused[1]))
    for _ in range(2):
        metrics.segmentation_confusion(x, tt, K, out=out)
    assert torch.equal(out[0], 2 * fused[0]) and torch.equal(out[1], 2 * fused[1])
    with pytest.raises(RuntimeError, match="fused"):
        metrics.segmentation_confusion(x.double(), tt, K, fused=True)
    e = metrics.segmentation_confusion(x[:, :0], tt[:, :0], K, fused=True)        # empty input: a no-op
    assert int(e[0].sum()) == 0 and e[0].shape == (2, K, K + 1)


def test_meter_accumulates_on_the_device_without_a_read_back():
    from instance_nerf_amd.nerf.utils import MIoUMeter, SegmentationMeter
    K = 16
    views = [(p.to(DEV), t.to(DEV)) for p, t in random_views(K, seed=4, n_views=3, H=40, W=37)]
    old, new = MIoUMeter(K), SegmentationMeter(K)
    new.update(*views[0])                                    # the first update allocates the matrix
    logits = torch.randn(1, 40, 37, K, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                  # any host read-back or device synchronisation raises
    try:
        for p, t in views[1:]:
            new.update(p, t)
        other = SegmentationMeter(K, device=DEV)
        other.update(views[0][0], views[0][1])
        other.update(logits, views[0][1])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert new.counts.is_cuda and new.ignored.is_cuda and new.counts.shape == (K, K + 1)
    for p, t in views:
        old.update(p, t)
    assert new.measure() == old.measure()
    got, want = new.measure_all(), old.measure_both()
    assert got["miou_gt_ids"] == want["miou_gt_ids"] and got["miou_all_ids"] == want["miou_all_ids"]
    assert not got["counts"].is_cuda and int(got["counts"].sum() + got["ignored"].sum()) == 3 * 40 * 37
    assert int(other.counts.sum() + other.ignored.sum()) == 2 * 40 * 37


# ---------------------------------------------------------------------------- trainer
def test_trainer_evaluate_segmentation(tmp_path, room):
    from instance_nerf_amd.nerf import NeRFNetwork
    from instance_nerf_amd.nerf.utils import Trainer, get_rays
    K = 16
    poses, intr, H, W = room.cameras(n=3, H=32, W=32, focal=16.0)
    gen = torch.Generator().manual_seed(0)

    def view(i, masks=True):
        r = get_rays(torch.as_tensor(np.ascontiguousarray(poses[i:i + 1])).to(DEV), intr, H, W, N=-1)
        d = {"rays_o": r["rays_o"], "rays_d": r["rays_d"], "H": H, "W": W}
        if masks:
            d["masks"] = torch.randint(-1, K, (1, H * W), generator=gen).to(DEV)
        return d

    torch.manual_seed(0)
    net = NeRFNetwork(cuda_ray=True, bound=1, min_near=0.05, num_instances=K).to(DEV)
    net.density_bitfield.copy_(torch.as_tensor(room.density_bitfield(128, 1.0)).to(DEV))
    tr = Trainer("seg", None, net, stage="instance", device=torch.device(DEV), workspace=str(tmp_path), mute=True,
                 use_checkpoint="scratch")
    loader = [view(0), view(1), view(2)]
    want = tr.evaluate(loader)                               # the default MIoUMeter
    net.train()
    got = tr.evaluate_segmentation(loader, name="held-out")
    assert net.training and len(tr.stats["results"]) == 1    # the mode is restored, the statistics are untouched
    print(f"miou_gt_ids {got['miou_gt_ids']!r} MIoUMeter {want!r}; pq {got['pq']:.6f} pixel_acc {got['pixel_acc']:.6f}")
    assert got["miou_gt_ids"] == want
    assert int(got["counts"].sum() + got["ignored"].sum()) == 3 * H * W
    assert int(got["ignored"].sum()) == sum(int((d["masks"] < 0).sum()) for d in loader)
    assert got["counts"].shape == (K, K + 1) and set(got) >= {"pq", "sq", "rq", "tp", "fp", "fn", "matches", "pixel_acc"}
    with pytest.raises(ValueError, match="masks"):
        tr.evaluate_segmentation([view(0, masks=False)])
    assert net.training
    nerf = Trainer("rgb", None, net, stage="nerf", device=torch.device(DEV), workspace=str(tmp_path), mute=True,
                   use_checkpoint="scratch")
    with pytest.raises(ValueError, match="instance"):
        nerf.evaluate_segmentation(loader)
