"""tests/roialign_reference.py on the CPU: against oracle/roialign.py (another formulation: one sample after the other),
as its own adjoint, the preconditions of the exact tier for every case the GPU tests use, the literal boundary-rule
values, and the restated channels-per-workgroup rule on the (K, C) lists of the channel-run cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roialign_reference as rr  # noqa: E402
from oracle import roialign  # noqa: E402

F32 = np.float32


def _fwd32(c):
    return rr.case_forward(c)["out"].astype(F32)


@pytest.mark.parametrize("seed", range(6))
def test_reference_agrees_with_the_oracle(seed):
    """Random volumes with extents 1..7, reversed and thin boxes, scales 1 / 0.5 / 0.7: the oracle returns the float32
    rounding of a float64 sum over samples; the separable float64 form lies within that rounding."""
    rng = np.random.default_rng(seed)
    shape = tuple(int(v) for v in rng.integers(1, 8, 3))
    osz = tuple(int(v) for v in rng.integers(1, 5, 3))
    scale = (1.0, 0.5, 0.7)[seed % 3]
    rois = rr.tol_rois(rng, 6, shape, scale)
    rois[1, 3:] = rois[1, :3] - 2.0                                   # reversed
    rois[2, 3:] = rois[2, :3] + F32(0.2)                              # thin
    c = rr.make_case("cpu", seed, 2, 3, shape, osz, scale, rois, tier="tol")
    ref = rr.case_forward(c)
    want = roialign.roi_align_3d(c["vol"], c["rois"], c["inds"], *osz, scale).astype(np.float64)
    assert np.all(np.abs(ref["out"] - want) <= rr.EPS * np.abs(ref["out"]) + 1e-12 * ref["mass"] + 1e-300)
    assert np.all(ref["out"][ref["mass"] == 0] == 0) and np.all((ref["n"] == 0) <= (ref["mass"][:, :1] == 0))


@pytest.mark.parametrize("name", ["extent0", "extent1", "extent2", "extent3", "boundary0", "boundary2", "dispatch/half_outside",
                                  "dispatch/tiny_z/H4", "bwd/thin"])
def test_exact_cases_are_bit_equal_to_the_oracle(name):
    c = rr.exact_cases()[name]
    want = roialign.roi_align_3d(c["vol"], c["rois"], c["inds"], *c["osz"], c["scale"])
    assert np.array_equal(_fwd32(c), want)


@pytest.mark.parametrize("name", ["t0", "t3"])
def test_adjoint_identity_in_float64(name):
    """<forward(vol), g> == <vol, backward(g)> to 1e-12 relative, both sides in float64."""
    c = rr.tol_cases()[name]
    f, b = rr.case_forward(c), rr.case_backward(c)
    lhs = float((f["out"] * c["g"].astype(np.float64)).sum())
    rhs = float((b["grad"] * c["vol"].astype(np.float64)).sum())
    scale = float((f["mass"] * np.abs(c["g"])).sum())
    assert scale > 0 and abs(lhs - rhs) <= 1e-12 * scale
    # the term counts are adjoint too: every nonzero tap of the forward is one of the backward
    assert int(f["n"].sum()) == int(b["n"].sum())


def _dyadic(a, what):
    a = np.asarray(a, np.float64)
    assert np.all(np.abs(a) < 2.0 ** 11), what
    assert np.array_equal(a * 4096.0, np.round(a * 4096.0)), what


def test_exact_tier_preconditions():
    """Every exact case: reference values, masses and count x value are multiples of 2^-12 below 2^11 (so every partial
    sum is exact in fp32 in any order), the reference equals its own float32 rounding, inputs are integers in
    [-8, 8], and at least two thirds of the boxes have an output element with samples inside the volume."""
    cases = rr.exact_cases()
    assert len(cases) > 30
    for name, c in cases.items():
        assert c["tier"] == "exact"
        for v in (c["vol"], c["g"]):
            assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 8
        f, b = rr.case_forward(c), rr.case_backward(c)
        counts = np.asarray([rr.roi_tables(r, c["shape"], c["osz"], c["scale"])[3] for r in c["rois"]], np.float64)
        assert np.all(np.log2(counts) == np.round(np.log2(counts))), name
        for what, a in (("out", f["out"]), ("mass", f["mass"]), ("grad", b["grad"]), ("gmass", b["mass"])):
            _dyadic(a, (name, what))
            assert np.array_equal(a.astype(F32).astype(np.float64), a), (name, what)
        _dyadic(f["mass"] * counts[:, None, None, None, None], (name, "count x mass"))
        _dyadic(f["out"] * counts[:, None, None, None, None], (name, "count x out"))
        live = (f["n"].reshape(len(c["rois"]), -1).sum(1) > 0).mean()
        assert live >= 2.0 / 3.0, (name, live)
        assert np.any(f["out"] != 0) and np.any(b["grad"] != 0), name


def test_cases_reach_the_paths_they_are_named_after():
    """The path conditions of sep_fwd_body / sep_bwd_body / k_roi_align3d_sep_bwd_cl, evaluated on the cases' geometry."""
    cs = rr.exact_cases()

    def live(r):                                   # RoIs with a sample inside on every axis
        return (r["size"] > 0).all(1)

    # three x slabs: XB = (10240 - 4 * ow) / (4 * (sy * oh + ol * oh)) planes of a 12-cell region
    c = cs["dispatch/slabs"]
    r = rr.regime(c)
    ow, ol, oh = c["osz"]
    xb = (10240 - 4 * ow) // (4 * (int(r["size"][0, 1]) * oh + ol * oh))
    assert r["size"][0, 0] == 12 and xb == 5
    # rows longer than the four register taps, on one axis only
    for a, nm in enumerate(("morex", "morey", "morez")):
        r = rr.regime(cs[f"dispatch/{nm}"])
        assert (r["row"][live(r)][:, a] >= 5).any()
        assert (np.delete(r["row"], a, axis=1) <= 4).all()
    r = rr.regime(cs["dispatch/morex_multi"])
    assert (r["row"][live(r)][:, 0] >= 5).any() and np.prod(cs["dispatch/morex_multi"]["osz"]) > 1024
    # regions thinner than the four-cell z window: depths 1, 2 and 3, at both faces
    for H in (8, 4):
        r = rr.regime(cs[f"dispatch/tiny_z/H{H}"])
        assert {1, 2, 3} <= set(r["size"][:, 2].tolist()) and r["size"][:, 2].max() < 4
    r = rr.regime(cs["dispatch/half_outside"])
    assert (r["empty_rows"][live(r)] > 0).any(0).all()
    # backward: generic roles beside fixed ones, more than four output indices per cell
    for nm, big in (("bwd/generic_syoh", lambda r, c: r["size"][:, 1] * c["osz"][2] > 256),
                    ("ws/oneB_off", lambda r, c: r["size"][:, 1] * c["osz"][2] > 256)):
        c = cs[nm]
        r = rr.regime(c)
        assert big(r, c)[live(r)].any() and (~big(r, c))[live(r)].any(), nm
    c = cs["bwd/generic_olh"]
    assert c["osz"][1] * c["osz"][2] > 256
    assert np.prod(cs["bwd/nout1024"]["osz"]) == 1024 and np.prod(cs["bwd/nout1100"]["osz"]) == 1100
    r = rr.regime(cs["bwd/thin"])
    assert (r["reach"][:, 1] > 4).any() and (r["reach"][:, 2] > 4).any() and (r["reach"][:, 0] > 4).any()
    for nm in ("ws/C16", "ws/C48"):
        assert np.prod(cs[nm]["shape"]) % 32 != 0
    # channel runs: duplicates, the last volume reached, one volume unnamed
    for K, C in rr.CPB_LISTS[16] + rr.CPB_LISTS[8] + rr.CPB_LISTS[4]:
        c = cs[f"channels/{K}/{C}"]
        assert set(c["inds"].tolist()) == {0, 2} and c["N"] == 3
        assert len(np.unique(c["rois"], axis=0)) < K or K <= 24
    assert len(np.unique(cs["channels/2048/18"]["rois"], axis=0)) <= 24
    # extents: every one of 1..5 occurs, the separable forward refuses H < 4
    assert {1, 2, 3, 4, 5} == {e for s in rr.EXTENT_SHAPES for e in s}
    for s in ((1, 1, 1), (3, 1, 2), (5, 4, 1), (2, 5, 4)):
        assert s in rr.EXTENT_SHAPES


def test_declared_dispatch_is_the_restated_host_rule():
    """sep_fwd / sep_bwd of every case (what the GPU tests demand of mode 2) against the restated LDS arithmetic; the
    fall-back cases are there for the reason they are named after."""
    cases = dict(rr.exact_cases())
    cases.update(rr.tol_cases())
    for t in ("exact", "tol"):
        cases.update({f"{t}/bwd/{k}": v for k, v in rr.backward_cases(t).items()})
        cases.update({f"{t}/ws/{k}": v for k, v in rr.workspace_cases(t).items()})
    for name, c in cases.items():
        assert c["sep_fwd"] == rr.separable_fits(c["shape"], c["osz"], False), name
        assert c["sep_bwd"] == rr.separable_fits(c["shape"], c["osz"], True), name
    cs = rr.exact_cases()
    assert not cs["dispatch/window/H2048"]["sep_fwd"] and 8 * 2048 * 4 >= 64 * 1024      # the z table alone
    assert cs["dispatch/window/H2000"]["sep_fwd"] and not cs["dispatch/window/H2000"]["sep_bwd"]
    for H in (2000, 2048):                                         # one sample exactly on the far face z == H
        assert any(float(H) in rr.axis_samples(r[2], r[5], 1.0, 8)[0] for r in cs[f"dispatch/window/H{H}"]["rois"])
    assert not cs["dispatch/nout(17, 16, 16)"]["sep_fwd"] and 17 * 16 * 16 > 4096
    assert not cs["dispatch/nout(1, 17, 16)"]["sep_fwd"] and cs["dispatch/nout(1, 17, 16)"]["sep_bwd"]
    assert cs["dispatch/nout(16, 16, 16)"]["sep_fwd"] and not cs["dispatch/nout(16, 16, 16)"]["sep_bwd"]


def test_pyramid_case_preconditions():
    p = rr.pyramid_case()
    f = rr.forward(p["vols"], p["scales"], p["rois"], p["inds"], p["levels"], p["osz"])
    b = rr.backward(p["g"], p["shapes"], p["scales"], p["rois"], p["inds"], p["levels"])
    _dyadic(f["out"], "out")
    _dyadic(f["mass"], "mass")
    for lv in b:
        _dyadic(lv["grad"], "grad")
        _dyadic(lv["mass"], "gmass")
        assert np.any(lv["grad"] != 0)
    assert (f["n"].reshape(len(p["rois"]), -1).sum(1) > 0).mean() >= 2.0 / 3.0
    out_of_table = int(np.flatnonzero(p["levels"] == 3)[0])
    assert not f["out"][out_of_table].any() and p["shapes"][2][4] == 2


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_boundary_rules_on_the_reference(axis):
    """Samples exactly on -1.25, -1, -0.5, 0, n-1, n-0.5, n, n+0.25: skipped outside [-1, n], all weight on cell 0 up to
    0 and on cell n-1 from n-1 on; a reversed and a thin box have size 1."""
    c = rr.boundary_case(axis)
    n = c["shape"][axis]
    for k, (name, at, cell) in enumerate(rr.BOUNDARY_SAMPLES):
        v, grid = rr.axis_samples(c["rois"][k, axis], c["rois"][k, axis + 3], 1.0, 1)
        assert grid == 1 and v.shape == (1, 1) and v[0, 0] == at(n), name
        T = rr.roi_tables(c["rois"][k], c["shape"], c["osz"], 1.0)[0]
        row = np.zeros(n)
        if cell is not None:
            row[cell] = 1.0
        assert np.array_equal(T[axis][0], row), name
        for a in range(3):
            if a != axis:
                assert np.array_equal(T[a], np.eye(c["shape"][a])), name
    want = rr.boundary_expected(c, axis)
    assert np.array_equal(_fwd32(c), want)
    assert not want[0].any() and not want[7].any()
    assert np.array_equal(want[1], np.take(c["vol"][c["inds"][1]], [0], axis=1 + axis))
    assert np.array_equal(want[6], np.take(c["vol"][c["inds"][6]], [n - 1], axis=1 + axis))


def test_ones_volume_counts_samples():
    c = rr.ones_case()
    want = rr.ones_expected(c)
    assert np.array_equal(rr.case_forward(c)["out"], want)
    vals = set(np.unique(want).tolist())
    assert 0.0 in vals and 1.0 in vals and len(vals) >= 5          # whole, empty and partly counted bins
    # -1.25 with a grid of 2: skipped, yet counted
    T, _, inside, count = rr.roi_tables([-1.75, 0, 0, 0.25, 1, 1], (5, 6, 7), (1, 1, 1), 1.0)
    assert count == 2 and inside[0][0] == 1 and T[0][0].sum() == 1.0


def test_float32_ceil_decision():
    c, found = rr.ceil_case()
    assert found >= 3
    for roi in c["rois"]:
        g32 = rr.axis_samples(roi[0], roi[3], c["scale"], 3)[1]
        g64 = int(np.ceil(max(float(roi[3]) * c["scale"] - float(roi[0]) * c["scale"], 1.0) / 3.0))
        assert g32 != g64
    want = roialign.roi_align_3d(c["vol"], c["rois"], c["inds"], *c["osz"], c["scale"]).astype(np.float64)
    ref = rr.case_forward(c)
    assert np.all(np.abs(ref["out"] - want) <= rr.EPS * np.abs(ref["out"]) + 1e-12 * ref["mass"])


def test_channels_per_workgroup_lists():
    for cpb, lst in rr.CPB_LISTS.items():
        for K, C in lst:
            assert rr.channels_per_block(C, K) == cpb, (K, C)
    tails = {(cpb, C % cpb) for cpb, lst in rr.CPB_LISTS.items() for K, C in lst}
    assert {(16, 2), (16, 5), (8, 6), (4, 1), (4, 3)} <= tails
    assert -(-37 // 4) == 10                                       # ngroups beyond the 8 XCDs, with a tail of 1


def test_bound_is_zero_only_without_mass():
    c = rr.tol_cases()["t0"]
    f = rr.case_forward(c)
    b = rr.bound(f["n"], f["mass"])
    assert np.all((b == 0) == (f["mass"] == 0))
