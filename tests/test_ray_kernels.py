"""k_near_far and k_get_rays of csrc/raymarch.hip on the GPU, through the raw C ABI: bit-equal to oracle/rays.py
(tolerance zero), inside the derived bounds of the float64 references of tests/ray_reference.py (near_far64: 4 * 2^-24
relative, hit / miss wherever the float64 margin decides it; get_rays64: 12 * 2^-24 * S), outputs NaN-poisoned between
guard words, every call run twice with equal bits.

What each seeded fault is caught by is listed with the tests below ("catches: ...")."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_reference as rr  # noqa: E402
from kernel_harness import Buf, check, finish, nan_out, poisoned, stream  # noqa: E402
from oracle import rays as orays  # noqa: E402

pytestmark = pytest.mark.gpu
F32, I32 = np.float32, np.int32
CUBE = np.asarray([-1, -1, -1, 1, 1, 1], F32)
BOX = np.asarray([-1, -2, 0.5, 3, 1, 4], F32)                    # neither cubic nor centred


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, F32).view(I32)


def i64_buf(a):
    return Buf(np.ascontiguousarray(a, np.int64).view(I32))


def near_far(lib, o, d, aabb, min_near, labels=None, ignore=-1):
    """Both entry points on poisoned, guarded outputs, twice -> (nears, fars)."""
    n = len(o)
    inp = {"o": Buf(o.reshape(-1, 3)), "d": Buf(d.reshape(-1, 3)), "aabb": Buf(aabb), "labels": None if labels is None else i64_buf(labels)}
    res = []
    for _ in range(2):
        out = {"nears": nan_out(n), "fars": nan_out(n)}
        if labels is None:
            rc = lib.inr_near_far_from_aabb(inp["o"].ptr, inp["d"].ptr, inp["aabb"].ptr, n, min_near, out["nears"].ptr, out["fars"].ptr, stream())
        else:
            rc = lib.inr_near_far_from_aabb_skip(inp["o"].ptr, inp["d"].ptr, inp["aabb"].ptr, n, min_near, inp["labels"].ptr, ignore,
                                                 out["nears"].ptr, out["fars"].ptr, stream())
        check(rc, "near_far_from_aabb")
        got = finish(dict(out, **inp), f"near_far n={n}")
        assert (bits(got["o"]) == bits(o.reshape(-1, 3))).all() and (bits(got["d"]) == bits(d.reshape(-1, 3))).all()
        res.append((got["nears"], got["fars"]))
    assert (bits(res[0][0]) == bits(res[1][0])).all() and (bits(res[0][1]) == bits(res[1][1])).all(), "second run differs"
    return res[0]


def directed_rays():
    """(o, d, what) - the rays of test_near_far_directed."""
    s = F32(1 / np.sqrt(2))
    rows = [((0, 0, 0), (0, 0, 1), "origin inside"),
            ((0.2, -0.3, 0.9), (0.6, 0, -0.8), "origin inside, oblique"),
            ((0, 0, -1), (0, 0, 1), "origin on a face, pointing in"),
            ((0, 0, 1), (0, 0, 1), "origin on a face, pointing out"),
            ((1, 1, 1), (-s, -s, 0), "origin on a corner"),
            ((0, 0, -3), (0, 0, 1), "origin outside"),
            ((0, 0, 3), (0, 0, 1), "pointing away: far < min_near"),
            ((0, 5, 0), (1, 0, 0), "outside the slab of a zero component"),
            ((-3, 1, 0.3), (1, 0.0, 0.0), "+0 components, origin ON the slab face (0 * inf)"),
            ((-3, 1, 0.3), (1, -0.0, -0.0), "-0 components, origin ON the slab face"),
            ((-3, -1, 1), (1, 0.0, -0.0), "+-0 components, origin on two slab faces"),
            ((-3, 0.3, -0.2), (1, 0.0, -0.0), "+-0 components, origin inside the slabs"),
            ((-3, 1.5, 0), (1, 0.0, 0.0), "+0 component, origin outside the slab"),
            ((-3, 1.5, 0), (1, -0.0, 0.0), "-0 component, origin outside the slab"),
            ((-3, -5, 0), (s, s, 0), "edge-grazing: lo == far, a hit with near == far"),
            ((-5, -3, 0), (s, s, 0), "edge-grazing, slabs the other way round: near == hi"),
            ((0, -5, -3), (0, s, s), "edge-grazing in y, z: near == hi on the last axis"),
            ((0, -3, -5), (0, s, s), "edge-grazing in y, z: lo == far on the last axis"),
            ((-3, -5.5, 0), (s, s, 0), "just past the edge: a miss")]
    o, d, what = zip(*rows)
    return np.asarray(o, F32), np.asarray(d, F32), what


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_near_far_sizes(lib, n):
    """catches: a thread past N that writes (guards); a wrong block count (rays 256.. left poisoned)."""
    if n == 0:
        check(lib.inr_near_far_from_aabb(None, None, None, 0, 0.05, None, None, stream()), "N = 0, null pointers")
        check(lib.inr_near_far_from_aabb_skip(None, None, None, 0, 0.05, None, -1, None, None, stream()), "N = 0, null pointers")
        return
    for aabb in (CUBE, BOX):
        o, d, _, min_near = rr.near_far_random(n, 40 + n)
        got_n, got_f = near_far(lib, o, d, aabb, min_near)
        want_n, want_f = orays.near_far_from_aabb(o, d, aabb, min_near)
        assert (bits(got_n) == bits(want_n)).all() and (bits(got_f) == bits(want_f)).all()
        rr.check_near_far(got_n, got_f, rr.near_far64(o, d, aabb, min_near))


def test_near_far_float64_reference(lib):
    """20 000 random rays against near_far64: values inside 4 * 2^-24 |t64|, hit / miss equal wherever the float64 margin
    exceeds twice the bound; the share of rays left out of the classification check is at most 1 %.
    catches: a slab value formed with another operation order or a fused operation (the bound), a swapped lo / hi."""
    o, d, aabb, min_near = rr.near_far_random(20000, 3)
    ref = rr.near_far64(o, d, aabb, min_near)
    got_n, got_f = near_far(lib, o, d, aabb, min_near)
    share = rr.check_near_far(got_n, got_f, ref)
    print(f"near_far64: excluded share {share:.2e}")
    assert share <= rr.NEAR_FAR_MAX_EXCLUDED
    want_n, want_f = orays.near_far_from_aabb(o, d, aabb, min_near)
    assert (bits(got_n) == bits(want_n)).all() and (bits(got_f) == bits(want_f)).all()


@pytest.mark.parametrize("min_near", [0.05, 2.5, 7.0])
def test_near_far_directed(lib, min_near):
    """Origin inside, on a face, outside; pointing away; +-0 components with the origin on, inside and outside the slab;
    the edge-grazing rays, whose two slab values are 4 * rd bit for bit; min_near below and above near; a cubic and an
    offset non-cubic box.  catches: `near > hi` changed to `near >= hi` (the grazing rays with near == hi become
    misses); a NaN slab (0 * inf) that poisons near or far; min_near applied to a miss."""
    o, d, what = directed_rays()
    for aabb in (CUBE, BOX):
        got_n, got_f = near_far(lib, o, d, aabb, min_near)
        want_n, want_f = orays.near_far_from_aabb(o, d, aabb, min_near)
        for k, w in enumerate(what):
            assert bits(got_n)[k] == bits(want_n)[k] and bits(got_f)[k] == bits(want_f)[k], f"{w}: {got_n[k]}, {got_f[k]} want {want_n[k]}, {want_f[k]}"
        assert not np.isnan(got_n).any() and not np.isnan(got_f).any()
        rr.check_near_far(got_n, got_f, rr.near_far64(o, d, aabb, min_near))
    # closed forms on the cube, independent of the oracle
    got_n, got_f = near_far(lib, o, d, CUBE, min_near)
    rd = F32(1) / F32(1 / np.sqrt(2))
    four = F32(4) * rd
    for k, w in enumerate(what):
        if w.startswith("edge-grazing"):
            assert got_f[k] == four and got_n[k] == max(four, F32(min_near)), f"{w}: {got_n[k]}, {got_f[k]} want {four} twice"
        if w.startswith("just past") or w.startswith("outside the slab") or "outside the slab" in w:
            assert got_n[k] == rr.FLT_MAX and got_f[k] == rr.FLT_MAX, w
        # 0 * inf = NaN compares false both ways: with +0 (1 / d = +inf) the NaN is the slab's upper value and drops out,
        # the ray in the face plane is a hit; with -0 the slab's lower value is +inf and the ray is a miss (the contract
        # of oracle/rays.py, pinned here)
        if w.startswith("+0 components, origin ON") or "inside the slabs" in w:
            assert got_f[k] == 4.0 and got_n[k] == max(F32(2), F32(min_near)), w
        if w.startswith("-0 components, origin ON"):
            assert got_n[k] == rr.FLT_MAX and got_f[k] == rr.FLT_MAX, w
    k = what.index("pointing away: far < min_near")
    assert got_f[k] == -2.0 and got_n[k] == F32(min_near)


@pytest.mark.parametrize("ignore", [-1, 3])
def test_near_far_skips_the_ignored_label(lib, ignore):
    """The ignored label in the first and the last lane of a wave, in every lane of a wave and in the last ray: those
    rays equal a miss bit for bit, every other ray is untouched.  catches: the label read with another index or width
    (int64), the skip applied to the neighbour lane."""
    n = 257
    o, d, aabb, min_near = rr.near_far_random(n, 77)
    labels = np.random.default_rng(5).integers(0, 3, n).astype(np.int64)        # 0..2: never an ignored value
    labels[[0, 63, 256]] = ignore
    labels[64:128] = ignore
    labels[130] = ignore + (1 << 32)                                            # equal in the low word only: NOT ignored
    got_n, got_f = near_far(lib, o, d, aabb, min_near, labels, ignore)
    want_n, want_f = orays.near_far_from_aabb(o, d, aabb, min_near)
    skip = labels == ignore
    assert skip.sum() == 67 and (want_n[skip] != rr.FLT_MAX).any()
    want_n[skip], want_f[skip] = rr.FLT_MAX, rr.FLT_MAX
    assert (bits(got_n) == bits(want_n)).all() and (bits(got_f) == bits(want_f)).all()


# ---------------------------------------------------------------------------- ray generation
def get_rays(lib, poses, intr, W, inds, n):
    B = len(poses)
    inp = {"poses": Buf(poses), "inds": None if inds is None else i64_buf(inds)}
    res = []
    for _ in range(2):
        out = {"o": nan_out(B * n, 3), "d": nan_out(B * n, 3)}
        check(lib.inr_get_rays(inp["poses"].ptr, B, *[float(v) for v in intr], W, inp["inds"].ptr if inp["inds"] else None, n,
                               out["o"].ptr, out["d"].ptr, stream()), "get_rays")
        got = finish(dict(out, **inp), f"get_rays B={B} n={n}")
        res.append((got["o"].reshape(B, n, 3), got["d"].reshape(B, n, 3)))
    assert (bits(res[0][0]) == bits(res[1][0])).all() and (bits(res[0][1]) == bits(res[1][1])).all(), "second run differs"
    return res[0]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("listed", [False, True])
def test_get_rays(lib, B, listed):
    """Pixels 0, W - 1, W, H * W - 1 and a repeated index (listed) or the whole image (inds NULL); non-square intrinsics;
    pose 2 has a non-orthonormal 3x3.  catches: row and column swapped (pix % W against pix / W), the pixel centre
    without its +0.5, a fused multiply-add in the rotation (bits), inds read as int32 (pixels W.. go wrong)."""
    poses, intr, H, W, inds = rr.get_rays_inputs()
    poses = poses[3 - B:]                                       # B = 1: the non-orthonormal pose
    px = inds if listed else np.arange(H * W, dtype=np.int64)
    got_o, got_d = get_rays(lib, poses, intr, W, inds if listed else None, len(px))
    want = orays.get_rays(poses, intr, H, W, inds=px)
    assert (bits(got_o) == bits(want["rays_o"])).all() and (bits(got_d) == bits(want["rays_d"])).all()
    ref = rr.get_rays64(poses, intr, W, px)
    worst = rr.check_get_rays(got_o, got_d, ref)
    print(f"get_rays B={B}: worst {worst:.2f} U S of {rr.GET_RAYS_ROUNDINGS}")
    if B == 3:                                                  # pose 0 is the identity: |d| = 1 in exact arithmetic
        assert (np.abs(np.linalg.norm(got_d[0].astype(np.float64), axis=-1) - 1.0) <= ref["tol_norm"][0]).all()


def test_get_rays_of_nothing(lib):
    """B * n = 0 returns INR_OK with null outputs.  catches: a launch with an empty grid, a null check ahead of the
    size check."""
    check(lib.inr_get_rays(None, 0, 1.0, 1.0, 0.0, 0.0, 4, None, 5, None, None, stream()), "B = 0, null pointers")
    check(lib.inr_get_rays(None, 2, 1.0, 1.0, 0.0, 0.0, 4, None, 0, None, None, stream()), "n = 0, null pointers")


@pytest.mark.parametrize("n", [1, 300])
def test_training_batch_rays_are_get_rays(lib, n):
    """inr_sample_training_batch must give, for the pixels it drew, the ray bits of inr_get_rays.  catches: the loader's
    copy of the ray arithmetic drifting from k_get_rays (operation order, a fused operation)."""
    poses, intr, H, W, _ = rr.get_rays_inputs()
    pose = poses[1:2]
    pb = Buf(pose)
    out = {"inds": nan_out(2 * n, dtype=I32), "o": nan_out(n, 3), "d": nan_out(n, 3)}
    check(lib.inr_sample_training_batch(pb.ptr, *[float(v) for v in intr], H, W, None, 3, None, 0, 1234, 7, n, out["inds"].ptr,
                                        out["o"].ptr, out["d"].ptr, None, None, stream()), "sample_training_batch")
    got = finish(dict(out, pose=pb), "sample_training_batch")
    inds = got["inds"].view(np.int64)
    assert (inds == orays.sample_pixels(1234, 7, n, H, W)).all() and inds.min() >= 0 and inds.max() < H * W
    ro, rd = get_rays(lib, pose, intr, W, inds, n)
    assert (bits(got["o"]) == bits(ro[0])).all() and (bits(got["d"]) == bits(rd[0])).all()
    assert not poisoned(got["o"]).any() and not poisoned(got["d"]).any()
