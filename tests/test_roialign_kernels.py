"""The ten kernels of csrc/roialign.hip on the GPU against tests/roialign_reference.py (float64, separable tables), through
the raw C ABI: the lane-per-output pair, the separable forward / backward and the channels-last workspace backward with
its transposing copy; the pyramid kernels through MultiScaleRoIAlign3D.

Two tiers (roialign_reference.py).  EXACT: dyadic boxes and integer values, every partial sum exact in fp32 in any order:
the kernels must give the reference's float32 BITS, element by element, forward and backward, in every mode.  TOLERANCE:
arbitrary boxes at scale 0.7 and normal values, every element within (n + 8) * 2^-24 * mass, n = nonzero terms of the
lane-per-output sum, mass = the same sum over absolute values; an element without mass is exactly 0.0.  Each tolerance
comparison prints its worst err / bound.

Every launch writes into NaN-poisoned buffers with 64-float guards on both sides; afterwards the guards are intact, every
row is written and finite, and vol / grad_out, rois and roi_inds keep their bits.  Which implementation ran is observed
through inr_roi_align_3d_set_mode: mode 2 (separable or error) must succeed on a case built for the separable kernels
and must come back as an error return on one built to fall back (H < 4 in the forward, more than 4096 outputs,
out_l * out_h > 256, tables beyond the LDS window); modes 0 and 3 then run the separable kernels or the lane pair
accordingly, mode 1 always the lane pair.  The channels-per-workgroup rule (sep_channels_per_block in roialign.hip) is
restated as roialign_reference.channels_per_block and pinned to the (K, C) lists on the CPU.

Seen on an MI355X: all 65 tests pass on the unchanged kernels, the exact tier bit for bit.  Worst err / bound of the
tolerance tier per kernel family: lane forward 0.25, separable forward 0.23, lane backward 0.27, separable backward in
place 0.25, workspace backward + transposing copy 0.31 (every case lies between 0.04 and 0.31).

Mutations tried by hand on scratch builds of roialign.hip (one at a time; number of the 65 tests that failed):
  * the `c + 2 < cend` store of sep_fwd_body dropped: 38 - boundary rules, one-hot volume, the extents with H >= 4, the
    dispatch edges, every channel run, the forwards of the backward cases, the tolerance tier (an unwritten row: NaN);
  * `x >= (float)W` for `x > (float)W` in tri_setup (the lane pair, x axis only): 30 - boundary axis 0, the volume of
    ones, one-hot far_x / corner, every extent, channel runs, the pyramid in both modes, the window cases;
  * `v >= (float)na` for `v > (float)na` in sep_build_tables: 44, in every test function but the tolerance tier (no
    sample of a drawn box lies exactly on n);
  * `cx1 = min(cx1, x0 + sx - 1) - 1` in chunk_setup (the last x cell of a chunk dropped): 40, every forward of the
    separable kernel, chunked or not;
  * the `c + 2 < cend` atomicAdd of sep_bwd_body's fixed-role path dropped: 48; the `c + 1 < cend` one of its generic
    path: 7 - generic_syoh / generic_olh in both tiers, nout(1, 17, 16), the workspace cases' in-place run of oneB_off;
  * the `moreB` loop of sep_bwd_body skipped (taps behind the fourth output index of a cell): 10 - exact/thin,
    exact/nout1024, and the tolerance cases with boxes thinner than their output;
  * `role += 2 * SEP_THREADS` in k_roi_align3d_sep_bwd_cl's y pass (every second y role skipped): 2 - oneB_off in both tiers.
Every test failed under at least one of them.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roialign_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32 = torch.float32, torch.int32
GUARD = 64
MODES = (1, 2, 3, 0)              # lane per output, separable or error, separable without workspace, auto


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


def _set_mode(lib, mode):
    from instance_nerf_amd._lib import check
    check(lib.inr_roi_align_3d_set_mode(mode), "roi_align_3d_set_mode")


class Guarded:
    """n floats inside an allocation with GUARD NaN words on both sides; the inside starts as NaN or as `fill`."""

    def __init__(self, n, fill=None):
        self.n = n
        self.whole = torch.full((n + 2 * GUARD,), float("nan"), dtype=F32, device=DEV)
        self.view = self.whole[GUARD:GUARD + n]
        if fill is not None:
            self.view.copy_(torch.as_tensor(np.ascontiguousarray(fill, np.float32).ravel()))

    def guards_intact(self):
        return bool(torch.isnan(self.whole[:GUARD]).all()) and bool(torch.isnan(self.whole[GUARD + self.n:]).all())

    def untouched(self):
        return bool(torch.isnan(self.whole).all())

    def numpy(self, shape):
        assert self.guards_intact(), "a guard word was written"
        got = self.view.cpu().numpy().reshape(shape)
        assert np.isfinite(got).all(), "a row was not written, or is not finite"
        return got


class Inputs:
    """The device copies of a case's inputs and their bits, to be found unchanged after every launch."""

    def __init__(self, c, first):
        self.t = [torch.as_tensor(np.ascontiguousarray(c[first])).to(DEV), torch.as_tensor(c["rois"]).to(DEV),
                  torch.as_tensor(c["inds"]).to(DEV)]
        self.bits = [x.clone() for x in self.t]

    def unchanged(self):
        return all(torch.equal(a.view(I32), b.view(I32)) for a, b in zip(self.t, self.bits))


def _dims(c):
    return (c["N"], c["C"]) + c["shape"], len(c["rois"])


def _launch_forward(lib, c, mode):
    """-> out float32 [K, C, ow, ol, oh], or None when the library refused the call (an error return before any launch)."""
    from instance_nerf_amd._lib import check, ptr, stream_ptr
    (N, C, W, L, H), K = _dims(c)
    inp = Inputs(c, "vol")
    out = Guarded(K * C * int(np.prod(c["osz"])))
    _set_mode(lib, mode)
    try:
        rc = lib.inr_roi_align_3d_forward(ptr(inp.t[0], F32), ptr(inp.t[1], F32), ptr(inp.t[2], I32), N, C, W, L, H, K,
                                          *c["osz"], c["scale"], ptr(out.view), stream_ptr())
        torch.cuda.synchronize()
    finally:
        _set_mode(lib, 0)
    assert inp.unchanged()
    if rc != 0:
        with pytest.raises(RuntimeError, match="separable kernel"):
            check(rc, "roi_align_3d_forward")
        assert out.untouched()
        return None
    return out.numpy((K, C) + c["osz"])


def _launch_backward(lib, c, mode, prefill, workspace=False, short=0):
    """grad_input (prefilled: the in-place form accumulates; None: NaN, the workspace form overwrites) -> float32
    [N, C, W, L, H], or None when refused."""
    from instance_nerf_amd._lib import check, ptr, stream_ptr
    dims, K = _dims(c)
    N, C, W, L, H = dims
    inp = Inputs(c, "g")
    gin = Guarded(int(np.prod(dims)), fill=prefill)
    _set_mode(lib, mode)
    try:
        if workspace:
            need = int(lib.inr_roi_align_3d_backward_workspace_bytes(N, C, W, L, H, K, *c["osz"]))
            assert need == int(np.prod(dims)) * 4
            ws = torch.full((need // 4 + 2 * GUARD,), float("nan"), dtype=F32, device=DEV)
            rc = lib.inr_roi_align_3d_backward_ws(ptr(inp.t[0], F32), ptr(inp.t[1], F32), ptr(inp.t[2], I32), N, C, W, L, H,
                                                  K, *c["osz"], c["scale"], ptr(gin.view), ws[GUARD:].data_ptr(),
                                                  need - short, stream_ptr())
            torch.cuda.synchronize()
            assert bool(torch.isnan(ws[:GUARD]).all()) and bool(torch.isnan(ws[GUARD + need // 4:]).all())
        else:
            rc = lib.inr_roi_align_3d_backward(ptr(inp.t[0], F32), ptr(inp.t[1], F32), ptr(inp.t[2], I32), N, C, W, L, H, K,
                                               *c["osz"], c["scale"], ptr(gin.view), stream_ptr())
            torch.cuda.synchronize()
    finally:
        _set_mode(lib, 0)
    assert inp.unchanged()
    if rc != 0:
        with pytest.raises(RuntimeError, match="separable kernel|workspace too small"):
            check(rc, "roi_align_3d_backward")
        assert gin.guards_intact()
        if prefill is None:
            assert gin.untouched()
        else:
            assert np.array_equal(gin.view.cpu().numpy(), np.asarray(prefill, np.float32).ravel())
        return None
    return gin.numpy(dims)


# ------------------------------------------------------------------------------------------- references and comparison
@functools.lru_cache(maxsize=None)
def _exact():
    return rr.exact_cases()


@functools.lru_cache(maxsize=None)
def _tol():
    out = {f"tol/{k}": v for k, v in rr.tol_cases().items()}
    out["tol/ceil"] = rr.ceil_case()[0]
    out.update({f"bwd/{k}": v for k, v in rr.backward_cases("tol").items()})
    out.update({f"ws/{k}": v for k, v in rr.workspace_cases("tol").items()})
    return out


def _case(tier, name):
    return (_exact() if tier == "exact" else _tol())[name]


_REFS = {}


def _ref(c, side):
    key = (c["name"], side)
    if key not in _REFS:
        _REFS[key] = rr.case_forward(c) if side == "fwd" else rr.case_backward(c)
    return _REFS[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _compare(c, got, want, n, mass, family, prefill=None):
    """Exact tier: the bits of float32(prefill + reference).  Tolerance tier: every element within the bound."""
    if c["tier"] == "exact":
        exp = want if prefill is None else want + prefill
        exp = (exp + 0.0).astype(np.float32)                 # the reference's zeros are +0
        bad = np.flatnonzero(_bits(got).ravel() != _bits(exp).ravel())
        assert bad.size == 0, (c["name"], family, bad.size, bad[:8].tolist(), got.ravel()[bad[:8]].tolist(),
                               exp.ravel()[bad[:8]].tolist())
        return
    assert prefill is None
    err = np.abs(got.astype(np.float64) - want)
    lim = rr.bound(n, mass)
    assert np.all(got[np.broadcast_to(mass == 0, got.shape)] == 0.0), (c["name"], family, "an element without mass is not 0.0")
    ratio = float(np.max(err[lim > 0] / lim[lim > 0])) if np.any(lim > 0) else 0.0
    print(f"roialign {family:24s} {c['name']:28s} worst err / bound {ratio:.4f}")
    assert np.all(err <= lim), (c["name"], family, ratio, int((err > lim).sum()))


def _family(mode, sep, side):
    if side == "ws":
        return "sep backward workspace"
    return ("lane " if mode == 1 or not sep else "sep ") + ("forward" if side == "fwd" else "backward in place")


def _check_forward(lib, c, modes=MODES):
    ref = _ref(c, "fwd")
    for mode in modes:
        got = _launch_forward(lib, c, mode)
        if mode == 2:
            assert (got is not None) == c["sep_fwd"], (c["name"], "mode 2 of the forward", "accepted" if got is not None else "refused")
            if got is None:
                continue
        _compare(c, got, ref["out"], ref["n"], ref["mass"], _family(mode, c["sep_fwd"], "fwd"))


def _prefill(c):
    if c["tier"] != "exact":
        return np.zeros((c["N"], c["C"]) + c["shape"], np.float32)
    return np.random.default_rng(77).integers(-4, 5, size=(c["N"], c["C"]) + c["shape"]).astype(np.float32)


def _check_backward(lib, c, modes=MODES):
    ref = _ref(c, "bwd")
    pre = _prefill(c)
    for mode in modes:
        got = _launch_backward(lib, c, mode, pre)
        if mode == 2:
            assert (got is not None) == c["sep_bwd"], (c["name"], "mode 2 of the backward", "accepted" if got is not None else "refused")
            if got is None:
                continue
        _compare(c, got, ref["grad"], ref["n"], ref["mass"], _family(mode, c["sep_bwd"], "bwd"),
                 prefill=pre if c["tier"] == "exact" else None)
        unnamed = [b for b in range(c["N"]) if b not in set(c["inds"].tolist())]
        for b in unnamed:
            assert np.array_equal(_bits(got[b]), _bits(pre[b])), (c["name"], mode, "a volume no RoI names changed")


def _check_workspace(lib, c):
    ref = _ref(c, "bwd")
    for mode in (0, 2):
        got = _launch_backward(lib, c, mode, None, workspace=True)
        assert got is not None
        _compare(c, got, ref["grad"], ref["n"], ref["mass"], _family(mode, True, "ws"))
    assert _launch_backward(lib, c, 0, None, workspace=True, short=1) is None        # one byte short: refused
    for mode in (1, 3):                                                              # no workspace form in these modes
        _set_mode(lib, mode)
        try:
            dims, K = _dims(c)
            assert lib.inr_roi_align_3d_backward_workspace_bytes(*dims, K, *c["osz"]) == 0
        finally:
            _set_mode(lib, 0)


# ------------------------------------------------------------------------------------------------------ boundary rules
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_boundary_rules(lib, axis):
    """Samples exactly on -1.25, -1, -0.5, 0, n-1, n-0.5, n and n+0.25 of one axis (identity on the other two): the
    expected rows are slabs of the volume or zero, written down without the reference; then reference and backward."""
    c = _exact()[f"boundary{axis}"]
    want = rr.boundary_expected(c, axis)
    n = c["shape"][axis]
    for mode in MODES:
        got = _launch_forward(lib, c, mode)
        assert got is not None
        assert np.array_equal(_bits(got), _bits(want)), (axis, mode)
        for k, cell in ((1, 0), (2, 0), (3, 0), (8, 0), (4, n - 1), (5, n - 1), (6, n - 1), (9, n - 1)):
            assert np.array_equal(got[k], np.take(c["vol"][c["inds"][k]], [cell], axis=1 + axis)), (axis, mode, k)
        assert not got[0].any() and not got[7].any()
    _check_forward(lib, c)
    _check_backward(lib, c)


def test_volume_of_ones_counts_the_inside_samples(lib):
    """out == inside samples / count: a sample outside [-1, n] is skipped and still counted."""
    c = _exact()["ones"]
    want = rr.ones_expected(c).astype(np.float32)
    for mode in MODES:
        got = _launch_forward(lib, c, mode)
        assert got is not None and np.array_equal(_bits(got), _bits(want)), mode
    _check_backward(lib, c)


# --------------------------------------------------------------------------------------------------- one-hot placement
@pytest.mark.parametrize("where", list(rr.ONE_HOT_CELLS))
def test_one_hot_volume_lands_on_the_reference_support(lib, where):
    c = rr.one_hot_case(where, "vol")
    ref = _ref(c, "fwd")["out"]
    assert np.count_nonzero(ref[0]) > 0
    for mode in MODES:
        got = _launch_forward(lib, c, mode)
        assert got is not None and np.array_equal(got != 0, ref != 0), (where, mode)
        assert np.array_equal(_bits(got), _bits((ref + 0.0).astype(np.float32))), (where, mode)


@pytest.mark.parametrize("where", list(rr.ONE_HOT_OUTPUTS))
def test_one_hot_grad_out_lands_on_the_reference_support(lib, where):
    c = rr.one_hot_case(where, "g")
    ref = _ref(c, "bwd")["grad"]
    assert np.count_nonzero(ref) > 0
    zeros = np.zeros(ref.shape, np.float32)
    for mode in MODES:
        got = _launch_backward(lib, c, mode, zeros)
        assert got is not None and np.array_equal(got != 0, ref != 0), (where, mode)
        assert np.array_equal(_bits(got), _bits((ref + 0.0).astype(np.float32))), (where, mode)


# -------------------------------------------------------------------------------------------------------------- extents
@pytest.mark.parametrize("i", range(len(rr.EXTENT_SHAPES)))
def test_extents_one_to_five(lib, i):
    """Volumes 1..5 cells a side.  The separable forward refuses H < 4 (its four-cell z window); the separable backward
    has no such limit and runs them in place."""
    c = _exact()[f"extent{i}"]
    assert c["sep_fwd"] == (c["shape"][2] >= 4) and c["sep_bwd"]
    _check_forward(lib, c)
    _check_backward(lib, c)


# ------------------------------------------------------------------------------------------------ forward dispatch edges
DISPATCH = ["nout(8, 8, 16)", "nout(11, 10, 10)", "nout(16, 16, 16)", "nout(17, 16, 16)", "nout(1, 17, 16)", "window/H2000", "window/H2048", "slabs",
            "morex", "morey", "morez", "morex_multi", "tiny_z/H8", "tiny_z/H4", "half_outside"]


@pytest.mark.parametrize("name", DISPATCH)
def test_forward_dispatch_edges(lib, name):
    """1024 / 1100 outputs (one chunk / chunks of whole pw planes), 4096 with out_l * out_h == 256, 4352 and
    out_l * out_h == 272 (fall back), tables that just fit the LDS window (H = 2000 at out_h = 8: 64 432 of 65 536 bytes)
    and tables beyond it (H = 2048: fall back), three x slabs, rows longer than the four
    register taps on one axis at a time and inside a chunked launch, regions 1-3 cells deep along z at both faces and with
    H == 4, boxes half outside (output indices without taps).  The in-place backward of the same cases rides along."""
    c = _exact()[f"dispatch/{name}"]
    _check_forward(lib, c)
    _check_backward(lib, c)


# --------------------------------------------------------------------------------------------------------- channel runs
@pytest.mark.parametrize("K,C", [kc for cpb in (16, 8, 4) for kc in rr.CPB_LISTS[cpb]])
def test_channel_runs(lib, K, C):
    """16, 8 and 4 channels per workgroup with runs that end inside a group of four (tails 2, 5, 6, 1, 3) and ten
    groups over the eight XCD slots; duplicate RoIs (atomics accumulate), the last of three volumes reached, one volume
    named by no RoI (its gradient does not change)."""
    c = _exact()[f"channels/{K}/{C}"]
    _check_forward(lib, c)
    _check_backward(lib, c)


# ------------------------------------------------------------------------------------------------------- backward forms
BWD = ["generic_syoh", "generic_olh", "nout1024", "nout1100", "thin"]


@pytest.mark.parametrize("name", BWD)
@pytest.mark.parametrize("tier", ["exact", "tol"])
def test_backward_in_place(lib, tier, name):
    """grad_input prefilled with small integers (exact tier: prefill + reference, bit for bit); generic roles
    (sy * out_h > 256, out_l * out_h > 256) beside fixed ones in one launch; 1024 / 1100 outputs (grad_out prefetched in
    registers or read in place); boxes one cell thick under 8 bins (more than four output indices per cell)."""
    c = _case(tier, f"bwd/{name}")
    _check_backward(lib, c)
    _check_forward(lib, c)


@pytest.mark.parametrize("name", ["C16", "C48", "oneB_off"])
@pytest.mark.parametrize("tier", ["exact", "tol"])
def test_backward_workspace_form(lib, tier, name):
    """C = 16 / 48, N = 2, V = 105 (no multiple of the copy's 32-voxel tile; C = 16 half a tile), grad_input NaN on
    entry, a region with sy * out_h > 256 (several y roles per thread); a workspace one byte short is refused."""
    c = _case(tier, f"ws/{name}")
    _check_workspace(lib, c)
    _check_backward(lib, c, modes=(1, 3))


# ------------------------------------------------------------------------------------------------------- tolerance tier
@pytest.mark.parametrize("name", ["tol/t0", "tol/t1", "tol/t2", "tol/t3", "tol/ceil"])
def test_tolerance_tier(lib, name):
    """Non-dyadic boxes (thinner than a voxel to 3 x the volume, scale 0.7), normal values; tol/ceil: boxes whose
    ceil(size / out) differs between float32 and float64 (the kernels and the reference take the float32 one)."""
    c = _tol()[name]
    _check_forward(lib, c)
    _check_backward(lib, c)


# -------------------------------------------------------------------------------------------------------------- pyramid
@pytest.mark.parametrize("mode", [0, 1])
def test_pyramid_through_the_module(lib, mode):
    """MultiScaleRoIAlign3D's fused path: three levels (scales 1 / 0.5 / 0.25, one with H = 2: the launch takes the lane
    kernels in the forward), one RoI naming a level outside the table (a zero row, no gradient): forward and every
    level's gradient bit for bit."""
    from instance_nerf_amd.roi_align.poolers import MultiScaleRoIAlign3D
    p = rr.pyramid_case()
    fwd = rr.forward(p["vols"], p["scales"], p["rois"], p["inds"], p["levels"], p["osz"])
    bwd = rr.backward(p["g"], p["shapes"], p["scales"], p["rois"], p["inds"], p["levels"])
    pool = MultiScaleRoIAlign3D(p["osz"], 0)
    levels = torch.as_tensor(p["levels"]).to(DEV)
    pool.scales, pool.map_levels = list(p["scales"]), (lambda boxes: levels)
    feats = [torch.as_tensor(v).to(DEV).requires_grad_(True) for v in p["vols"]]
    rois = torch.as_tensor(p["rois"]).to(DEV)
    boxes = list(rois.split(p["counts"]))
    _set_mode(lib, mode)
    try:
        out = torch.cat(pool(feats, boxes, None))
        out.backward(torch.as_tensor(p["g"]).to(DEV))
        torch.cuda.synchronize()
    finally:
        _set_mode(lib, 0)
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits((fwd["out"] + 0.0).astype(np.float32)))
    assert not out[int(np.flatnonzero(p["levels"] == 3)[0])].any()
    for f, b, v in zip(feats, bwd, p["vols"]):
        assert np.array_equal(_bits(f.grad.cpu().numpy()), _bits((b["grad"] + 0.0).astype(np.float32)))
        assert np.array_equal(f.detach().cpu().numpy(), v)
