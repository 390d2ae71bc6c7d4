"""The mask projector of csrc/raymarch.hip (k_project_masks_patch) on the GPU against tests/project_masks_reference.py,
through inr_project_masks_patch on plain device tensors: no march, no field.

Every case must equal the fp32 sequential restatement bit for bit - the kernel's contract is "same sums in the same
order" - over the WHOLE of ``out``, which starts as a NaN pattern: the columns outside [k_base, k_base + k_count) and the
rows no ray names must still hold it.  On top of that the exact tier (weights on a 2^-12 lattice, at most 256 samples a
ray: every partial sum is exact in fp32) must equal the float64 result bit for bit, and the general tier must lie within
cnt * 2^-24 * sum|w| of the float64 result on every ray without a sample whose fp32 and float64 cells differ (those
samples sit within 2^-20 of a cell face; tests/test_project_masks_cpu.py).  The sample arrays hold exactly M rows between
NaN-pattern guard words: a read behind M poisons the result.

catches: V.L and V.H swapped (volumes 3x5x7 and 7x9x11), fx < res made <= (samples on hi of the first axis), 0xFFFF made
0xFF (every group with a live ray in lanes 8 .. 15), the dropped-group test removed (M modes drop1, drop2, keep1, zero:
rows of zeros expected), i < k_count removed (k_count < 32: the NaN pattern beside the written columns), rid replaced
by n (ids are a permutation of a subset of the rows)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_masks_reference as R  # noqa: E402
import train_kernels_reference as tk  # noqa: E402
from kernel_harness import Buf, check, stream  # noqa: E402

pytestmark = pytest.mark.gpu
f = np.float32
CASES = R.all_cases()


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("kw", CASES, ids=[R.case_id(kw) for kw in CASES])
def test_project_masks(lib, kw):
    c = R.make_case(**kw)
    N, M = c["N"], c["M"]
    k_total, k_base, k_count = c["k"]
    W, L, H = c["vol"]
    assert c["words"].shape == (W, L, H) and len(c["xyz"]) == M == len(c["w"]) and c["rays"].shape == (N, 3)
    assert c["rays"][:, 0].max() < c["n_rows"] and k_base + k_count <= k_total
    want = R.project32(c)
    xyz, w = (Buf(c["xyz"]), Buf(c["w"])) if M else (None, None)
    rays, words = Buf(c["rays"]), Buf(c["words"])
    out = Buf(np.zeros((c["n_rows"], k_total), f))
    out.fill_nan()
    bbox = np.ascontiguousarray(np.concatenate(c["box"]), f)                     # host memory: lo[3], hi[3]
    check(lib.inr_project_masks_patch(xyz.ptr if M else None, w.ptr if M else None, rays.ptr, N, M, words.ptr, W, L, H,
                                      bbox.ctypes.data, k_total, k_base, k_count, out.ptr, stream()), c["name"])
    got = out.get()
    tk.assert_same_bits(got, want, c["name"])
    for b in (xyz, w, rays, words, out):
        if b is not None:
            b.check_guards(c["name"])
    written = np.zeros(got.shape, bool)
    written[c["rays"][:, 0], k_base:k_base + k_count] = True
    assert np.isfinite(got[written]).all(), c["name"] + ": not finite"
    if not M:
        assert (got[written] == 0).all()
        return
    truth = R.project64(c)
    if c["tier"] == "exact":
        tk.assert_same_bits(got[written], truth[written].astype(f), c["name"] + " against float64")
        return
    clear = ~R.rays_with(c, R.ambiguous(c))
    err = np.where(written, np.abs(got.astype(np.float64) - truth), 0.0).max(-1)
    bound = R.sum_bound(c)
    worst = float((err[clear] / np.maximum(bound[clear], 1e-300)).max()) if clear.any() else 0.0
    print(f"{c['name']}: worst error {worst:.3f} of cnt * 2^-24 * sum|w| over {int(clear.sum())} of {len(clear)} rows")
    assert (err[clear] <= bound[clear]).all(), c["name"]
