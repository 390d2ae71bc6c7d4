"""The conditions tests/render_reference.py states about its own cases, checked from the float64 reference alone (no GPU):
where the rays of the tolerance cases stop, the ambiguity cap, ``evaluated`` worked by hand, cond == 0 => value == 0,
the exact tier's preconditions, the CPU models inside TOL / margin, and the GroupDraw schedule restated."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_reference as C  # noqa: E402
import field_forward_reference as R  # noqa: E402
import render_reference as X  # noqa: E402

F32 = np.float32
ROWS = (("bf16x3", ""), ("bf16x3", "o"), ("fp32", ""))


@pytest.fixture(scope="module")
def refs():
    return {n: X.nerf_render_ref(X.tol_case(n)) for n in X.TOL_CASES}


def test_case_shapes_and_settings():
    cases = [X.tol_case(n) for n in X.TOL_CASES]
    assert {c["table"] for c in cases} == {"bench", "levels12"} and R.table_for("levels12")["num_levels"] < 16
    assert {c["ds"] for c in cases} == {1.0, 0.3} and {c["bound"] for c in cases} == {1.0, 2.0}
    assert sorted(c["T"] for c in cases) == [1e-4, 1e-4, 0.05]
    for c in cases:
        rays = c["rays"]
        assert len(rays) == 33 and sorted(rays[:, 2]) == sorted(X.COUNTS * X.COPIES)
        assert sorted(rays[:, 0]) == list(range(33)) and (rays[:, 0] != np.arange(33)).any()
        assert ((c["deltas"] >= 0.005) & (c["deltas"] <= 0.05)).all()
        assert (np.abs(c["x"]) <= c["bound"]).all() and (np.abs(c["x"]) == c["bound"]).any()      # clamped samples: faces
    e = X.exact_case()
    assert len(e["rays"]) == len(X.COUNTS) * len(X.TERMINATION) and len(e["rays"]) % 16
    assert set(np.unique(e["deltas"][:, 0])) == {0.0, 1024.0}
    for n in range(len(e["rays"])):
        dy = e["deltas"][e["rays"][n, 1]:e["rays"][n, 1] + e["rays"][n, 2], 1]
        assert len(set(dy)) == len(dy) and (dy == np.round(dy)).all() and (dy > 0).all() and (dy < 1024).all()


def test_slot_map_is_the_compositing_suites(refs):
    for case in [X.tol_case(n) for n in X.TOL_CASES] + [X.exact_case(), X.schedule_case(37)]:
        slots = C.patch_slot_map(case["rays"])
        assert np.array_equal(slots, case["slots"]) and sorted(slots) == list(range(len(slots)))


@pytest.mark.parametrize("name", list(X.TOL_CASES))
def test_where_the_rays_stop(refs, name):
    """From the float64 reference alone: a ray that stops after its first sample, one strictly inside, one that never
    stops, a full group with a skipped step; no ray inside the widest band, and the margins the docstring states."""
    case, ref = X.tol_case(name), refs[name]
    t = X.termination_classes(case, ref)
    print(name, t, "smallest margin", ref["margin"].min())
    assert t["first"] >= 1 and t["inside"] >= 1 and t["never"] >= 1 and t["skipped_in_full_group"] > 0
    widest = max(v for b in X.BAND.values() for v in b.values())
    assert X.ambiguous_rays(case, ref, widest) == {}
    assert ref["margin"].min() >= X.SMALLEST_MARGIN[name] > widest
    assert ref["evaluated"] < int(case["rays"][:, 2].sum())


def test_ambiguity_cap_and_alternative(refs):
    """A band that catches rays trips the cap on a 33-ray case; the alternative of a flipped boundary changes that ray's
    stop by one sample and no other ray."""
    case, ref = X.tol_case("bench"), refs["bench"]
    with pytest.raises(AssertionError):
        X.ambiguous_rays(case, ref, 1e3)
    n = int(np.flatnonzero((ref["n_used"] > 1) & (ref["n_used"] < case["rays"][:, 2]))[0])
    for flip, step in ((int(ref["n_used"][n]), +1), (int(ref["n_used"][n]) - 1, -1)):
        alt = X.alternative(case, ref, {n: flip})
        d = alt["n_used"] - ref["n_used"]
        assert d[n] == step
        assert (np.delete(d, n) == 0).all()
        rid = np.delete(case["rays"][:, 0], n)
        assert np.array_equal(alt["out"]["image"][rid], ref["image"][rid])
        off = int(case["rays"][n, 1])
        w = alt["out"]["weights"][case["slots"][off + alt["n_used"][n]:off + case["rays"][n, 2]]]
        assert (w == 0).all()


def test_evaluated_by_hand():
    """Two groups.  Group 0: ray 0 (3 samples, opaque at its first), ray 1 (1 sample, transparent), ray 3 (2 samples,
    transparent): step 0 evaluates 3 samples, step 1 two (the terminated ray 0 rides along), step 2 is skipped -> 5 of 6.
    Group 1: two rays of 2 samples, both opaque at their first: step 0 evaluates 2, step 1 is skipped -> 2 of 4."""
    cnt = np.zeros(18, np.int64)
    p = np.full(18, -1)
    cnt[[0, 1, 3, 16, 17]] = (3, 1, 2, 2, 2)
    p[[0, 16, 17]] = 0
    case = X.constant_case("hand", X._rng("hand"), cnt, p)
    ref = X.nerf_render_ref(case)
    assert ref["evaluated"] == 7 and list(ref["n_used"][[0, 1, 3, 16, 17]]) == [1, 1, 2, 1, 1]
    assert X.cut_M(case, "last") == 9
    cut = X.nerf_render_ref(case, 9)
    assert cut["evaluated"] == 5 and cut["dropped"][16:].all() and not cut["dropped"][:16].any()
    assert cut["written"].sum() == 6 and not cut["written"][6:].any()
    rid = case["rays"][:, 0]
    assert (cut["weights_sum"][rid[16:]] == 0).all() and np.array_equal(cut["weights_sum"][rid[:16]], ref["weights_sum"][rid[:16]])
    assert np.array_equal(cut["weights"][:6], ref["weights"][:6])


def test_cond_zero_means_value_zero(refs):
    for name, ref in list(refs.items()) + [("exact", X.nerf_render_ref(X.exact_case()))]:
        for k in X.OUTPUTS:
            assert (ref[k][ref["cond"][k] == 0] == 0).all(), (name, k)
            assert (ref["cond"][k] >= 0).all()
        case = X.exact_case() if name == "exact" else X.tol_case(name)
        out, cond = X.instance_render_ref(case, 16)
        assert (out[cond == 0] == 0).all() and (cond == 0).any()


def test_exact_tier_is_exact():
    """exactness_violations over the encoder and every layer at the exact case's positions; sigma == density_scale and
    rgb == 0.5 on the data; every termination class present; the fp32 compositing model reproduces the float64 outputs
    bit for bit; the logits are small multiples of a power of two, so every instance sum is exact in any order."""
    case = X.exact_case()
    log = []
    f = X.Field(case, log=log)
    o, _ = f.nerf()
    for K in X.KS:
        lg, _ = f.logits(K)
        q = R.quantum(lg) / 2                             # the logits' quantum (trilinear weights: 2^-9), halved by w = 0.5
        assert lg.any() and q >= 2.0 ** -12 and max(X.COUNTS) * 2 * np.abs(lg).max() / q < 2 ** 24
    assert R.exactness_violations(log) == []
    assert (o["sigma"] == case["ds"]).all() and (o["rgb"] == 0.5).all()
    ref = X.nerf_render_ref(case)
    assert set(np.unique(ref["weights"])) == {0.0, 1.0} and set(np.unique(ref["weights_sum"])) == {0.0, 1.0}
    assert set(np.unique(ref["image"])) == {0.0, 0.5} and (ref["depth"] == np.round(ref["depth"])).all() and ref["depth"].max() < 2 ** 24
    used = {(c, t): int(ref["n_used"][n]) for n, (c, t) in enumerate(case["term"])}
    assert used[(130, "transparent")] == 130 and used[(130, "last")] == 130 and used[(130, "first")] == 1
    assert [used[(130, k)] for k in (1, 7, 8, 9, 16)] == [2, 8, 9, 10, 17] and used[(9, 16)] == 9 and used[(0, 7)] == 0
    mod = X._composite(case, ref["sigma"].astype(F32), ref["rgb"].astype(F32), None, None, len(ref["weights"]), dtype=F32)
    for k in X.OUTPUTS:
        assert np.array_equal(mod["out"][k].astype(np.float64), ref[k]), k
    assert 0 < ref["evaluated"] < len(ref["weights"])
    w_patch, w = X.instance_inputs(case, 64)
    assert set(np.unique(w)) == set(X.W_VALUES) and 0.2 < (w == 0).mean() < 0.5
    row, step = X.sample_rows(case["rays"])
    g = case["zero_group"]
    assert case["rays"][g * 16:(g + 1) * 16, 2].max() > X.ZERO_FROM + X.WAVES and not w[(row // 16 == g) & (step >= X.ZERO_FROM)].any()
    assert w[(row // 16 == g) & (step < X.ZERO_FROM)].any()


def test_strict_threshold_case():
    """At T_thresh == 1 the reference stops every ray where it stops at 1e-4, and rays with a transparent prefix exist:
    a test T <= T_thresh would stop them after their first sample."""
    a, b = X.nerf_render_ref(X.exact_case()), X.nerf_render_ref(X.strict_case())
    assert np.array_equal(a["n_used"], b["n_used"]) and a["evaluated"] == b["evaluated"] and (a["n_used"] > 1).sum() > 40
    for k in X.OUTPUTS:
        assert np.array_equal(a[k], b[k])


def test_never_read_rows():
    """NaN strictly behind every opaque sample, nowhere else; among them rows of a terminated ray at a step its group
    still evaluates (they ride through the gather), and rows of steps that are skipped whole."""
    case, poisoned = X.exact_case(), X.never_read_case()
    ref = X.nerf_render_ref(case)
    bad = np.isnan(poisoned["deltas"]).any(1)
    assert np.array_equal(bad, np.isnan(poisoned["x"]).any(1)) and np.array_equal(bad, case["behind"]) and bad.sum() > 100
    row, step = X.sample_rows(case["rays"])
    assert (step[bad] >= ref["n_used"][row[bad]]).all() and not np.isnan(case["deltas"]).any()
    live_step = np.zeros(len(bad), bool)
    for g0 in range(0, len(case["rays"]), 16):
        sel = (row >= g0) & (row < g0 + 16)
        for k in np.unique(step[sel]):
            at = sel & (step == k)
            live_step[at] = (ref["n_used"][row[at]] > k).any()
    assert (bad & live_step).any() and (bad & ~live_step).any()


@pytest.mark.parametrize("build,num", ROWS, ids=[f"{b}{'-' + n if n else ''}" for b, n in ROWS])
def test_models_stay_within_tol_over_margin(build, num):
    """MEASURED and BAND_MEASURED are what the CPU models give against float64 (never against a kernel), and the models
    stop every ray where the reference does."""
    worst, band, margins = X.measure(build, num)
    print(build, repr(num), {k: f"{v:.3e}" for k, v in worst.items()}, f"band {band:.3e}", margins)
    assert set(worst) == {k for k in X.MEASURED[build] if k.partition("@")[2] == num}
    for k, v in worst.items():
        assert v <= X.TOL[build][k] / X.MARGIN[num], (k, v)
        assert v > 0.5 * X.MEASURED[build][k], (k, v)
    assert 0.5 * X.BAND_MEASURED[build][num] < band <= X.BAND_MEASURED[build][num]
    assert X.BAND[build][num] == 8 * X.BAND_MEASURED[build][num]


@pytest.mark.parametrize("kernel,sizes", [("nerf", X.SCHEDULE_N), ("instance", X.SCHEDULE_N_INSTANCE)])
def test_group_draw_hands_every_group_out_once(kernel, sizes):
    """GroupDraw::group_of restated: over all cursors and positions the groups handed out are a permutation of
    0 .. n_groups - 1 plus indices beyond it - with 1, 8 and 32 owners, one chunk, several, a second round of chunks and a
    ragged last chunk; and the sizes reach those regimes on 256 CUs."""
    regimes = []
    for N in sizes:
        n_groups = -(-N // 16)
        grid, n_owner = X.render_grid(N, 256, kernel)
        owners = {X.group_draw_owner(b, grid, 4 if kernel == "nerf" else 1) for b in range(grid)}
        assert {o for o, _ in owners} == set(range(n_owner)) and {n for _, n in owners} == {n_owner}
        chunks = -(-n_groups // 64)
        rounds = -(-chunks // n_owner)
        handed = [X.group_of(u, o, n_owner) for o in range(n_owner) for u in range(64 * (rounds + 1))]
        inside = sorted(g for g in handed if g < n_groups)
        assert inside == list(range(n_groups)) and len(set(handed)) == len(handed)
        regimes.append((grid, n_owner, chunks, rounds, n_groups % 64 != 0))
    print(kernel, regimes)
    if kernel == "nerf":
        assert [r[:2] for r in regimes] == [(1, 1), (8, 8), (40, 8), (32, 32), (256, 32)]
        assert [r[2] for r in regimes] == [1, 1, 5, 4, 34] and regimes[-1][3] == 2 and regimes[-1][4]
    else:
        assert [r[:2] for r in regimes] == [(3, 1), (8, 8), (256, 8)] and regimes[-1][3] == 2 and regimes[-1][4]
    # the mutation "n_owner where owner belongs" hands groups out twice and leaves others out
    broken = [(((u >> 6) * 8 + 8) << 6) + (u & 63) for o in range(8) for u in range(128)]
    assert len(set(broken)) < len(broken)


def test_dropped_group_expectations():
    case = X.exact_case()
    full = X.nerf_render_ref(case)
    rid = case["rays"][:, 0]
    for where, n_dropped in (("last", 1), ("middle", 3)):
        M = X.cut_M(case, where)
        ref = X.nerf_render_ref(case, M)
        g = np.flatnonzero(ref["dropped"])
        assert len(g) and g.min() % 16 == 0 and g.max() == len(rid) - 1 and len(set(g // 16)) == n_dropped
        assert not ref["written"][M:].any() and ref["written"].sum() == case["rays"][~ref["dropped"], 2].sum()
        keep = ~ref["dropped"]
        for k in ("weights_sum", "depth", "image"):
            assert not ref[k][rid[g]].any() and np.array_equal(ref[k][rid[keep]], full[k][rid[keep]])
        assert np.array_equal(ref["weights"][ref["written"]], full["weights"][ref["written"]])
        assert ref["evaluated"] < full["evaluated"]
