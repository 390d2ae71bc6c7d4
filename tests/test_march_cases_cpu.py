"""The directed march cases (tests/march_cases.py) and the plain references (tests/ray_reference.py) checked on the
CPU: every case keeps the safety rules, shows the property it was built for under oracle/march.py, and check_samples
accepts the oracle's output and rejects a damaged one.  tests/test_march_kernels.py and test_ray_kernels.py then run
the same cases through the kernels."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import march_cases as mc  # noqa: E402
import ray_reference as rr  # noqa: E402
from oracle import march as omarch  # noqa: E402
from oracle import rays as orays  # noqa: E402

F32 = np.float32
CASES = {c["name"]: c for c in mc.all_train_cases()}
SCAN_CPU = mc.SCAN_N_COOP + mc.SCAN_N_LANE


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return mc.oracle(CASES[name])


def by_prefix(prefix):
    return [c for n, c in CASES.items() if n.startswith(prefix)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_safe_and_its_oracle_output_passes(name):
    case = CASES[name]
    mc.check_safety(case)
    ref = ref_of(name)
    rr.check_samples(case, ref["rays"], ref["xyzs"], ref["dirs"], ref["deltas"], counter=(ref["total"], case["o"].shape[0]))
    if "counts" in case["promise"]:
        assert ref["rays"][:, 2].tolist() == case["promise"]["counts"], name


def test_candidates_restates_the_oracle_chain():
    """On a full grid every candidate below far is emitted: the oracle's t of each sample is the chain."""
    for g, C in ((0.0, 1), (1 / 64, 2)):
        case = mc._case("chain", [mc.AXIS_O], [mc.AXIS_D], mc.full(C, 8), 0.3, 1.7, C=C, bound=2.0 ** (C - 1), dt_gamma=g, max_steps=128)
        ref = mc.oracle(case)
        c = mc.candidates(F32(0.3), ref["total"] + 1, 128, C, 8, g)
        assert (c[:-1] < F32(1.7)).all() and c[-1] >= F32(1.7)
        want = np.clip(case["o"][0] + c[:-1, None] * case["d"][0], -case["bound"], case["bound"]).astype(F32)
        assert (ref["xyzs"] == want).all()
        assert (ref["deltas"][:, 0] == mc.dt_of(c[:-1], 128, C, 8, g)).all()


def test_far_on_candidate_counts_in_closed_form():
    (case,) = mc.far_on_candidate()
    assert case["promise"]["counts"] == [63, 64, 64, 65, 65, 128]


def test_full_windows_end_by_max_steps():
    for case in mc.full_windows():
        ref = ref_of(case["name"])
        assert (ref["rays"][:, 2] == case["max_steps"]).all()
        # the ray is cut short by max_steps, not by far: the next candidate is still below far
        c = mc.candidates(0.0, case["max_steps"] + 1, case["max_steps"], 1, 8, 0.0)
        assert c[-1] < case["fars"][0]


def test_long_skip_spans_windows():
    for case in mc.long_skip():
        mk = omarch._Marcher(case["o"], case["d"], case["bits"], case["bound"], case["C"], case["H"], case["dt_gamma"], case["max_steps"])
        t0 = mc.start_t(case)
        _, _, occ, tt = mk.probe(np.arange(3), t0)
        assert not occ.any()
        for r in range(3):
            c = mc.candidates(t0[r], 400, case["max_steps"], 1, 8, 0.0)
            assert (c < tt[r]).sum() - 1 > case["promise"]["min_skip"], (case["name"], r)
        assert (ref_of(case["name"])["rays"][:, 2] > 0).all()          # and the occupied cell at the end is found


def test_skip_lands_on_the_promised_candidate():
    (case,) = mc.skip_lands_on_lane()
    mk = omarch._Marcher(case["o"], case["d"], case["bits"], case["bound"], case["C"], case["H"], case["dt_gamma"], case["max_steps"])
    _, _, occ, tt = mk.probe(np.arange(4), mc.start_t(case))
    c = mc.candidates(0.0, 70, 1024, 1, 8, 0.0)
    for r, j in enumerate(case["promise"]["landing"]):
        assert not occ[r] and tt[r].view(np.int32) == c[j].view(np.int32)              # tt == c_j bit for bit
        assert mc.emitted_indices(case, r)[0] == j
        assert ref_of(case["name"])["xyzs"][ref_of(case["name"])["rays"][r, 1], 0] == 0.0


def test_pending_skip_rounding_lands_elsewhere_from_candidate_64():
    (case,) = mc.pending_skip_rounding()
    mk = omarch._Marcher(case["o"], case["d"], case["bits"], case["bound"], case["C"], case["H"], case["dt_gamma"], case["max_steps"])
    c = mc.candidates(0.0, 80, 1024, 1, 8, 0.0)
    n = case["o"].shape[0]
    _, _, occ0, tt0 = mk.probe(np.arange(n), np.zeros(n, F32))
    _, _, occ64, tt64 = mk.probe(np.arange(n), np.full(n, c[64], F32))
    assert not occ0.any() and not occ64.any()                           # candidate 64 is still in the empty cell
    for r in range(n):
        first, again = int(np.argmax(c >= tt0[r])), int(np.argmax(c >= tt64[r]))
        assert (first, again) == (case["promise"]["landing"][r], case["promise"]["landing_from_64"][r]) and first != again
        assert first > 64 and mc.emitted_indices(case, r)[0] == first
        assert case["o"][r, 0] + c[min(first, again)] * case["d"][r, 0] >= 0      # both lie in the occupied slab


def test_landing_guess_edge_is_one_short():
    (case,) = mc.landing_guess_edge()
    mk = omarch._Marcher(case["o"], case["d"], case["bits"], case["bound"], case["C"], case["H"], case["dt_gamma"], case["max_steps"])
    c = mc.candidates(0.0, 64, 1024, 1, 8, 0.0)
    n = case["o"].shape[0]
    _, dt, occ, tt = mk.probe(np.arange(n), np.zeros(n, F32))
    assert not occ.any()
    for r, land in enumerate(case["promise"]["landing"]):
        assert land < 64 and c[land - 1] < tt[r] <= c[land] and mc.emitted_indices(case, r)[0] == land
        estimate = int(F32(F32(tt[r] - c[0]) * F32(F32(1.0) / dt[r])))        # floor((tt - c) / dt): lanes to jump, minus one
        assert estimate + 1 == land - 1                                      # the estimate names candidate land - 1 ...
        p = np.clip(case["o"][r] + c[land - 1] * case["d"][r], -1, 1).astype(F32)
        assert p[0] == 0.0                                                   # ... which lies in the occupied slab


def test_sparse_hits_have_runs_and_gaps():
    for case in mc.sparse_hits():
        runs, gaps, first = 0, 0, 0
        for r in range(case["o"].shape[0]):
            j = mc.emitted_indices(case, r)
            assert j.size
            brk = np.diff(j)
            gaps = max(gaps, int(brk.max()) - 1, int(j[0]))
            run = np.diff(np.concatenate([[-1], np.nonzero(brk != 1)[0], [j.size - 1]]))
            runs = max(runs, int(run.max()))
        assert runs >= case["promise"]["run"] and gaps > case["promise"]["gap"], (case["name"], runs, gaps)


def test_cascade_edges_take_the_level_from_frexp():
    for case in mc.cascade_edges():
        ref, level = ref_of(case["name"]), case["promise"]["level"]
        if case["dt_gamma"] != 0.0:
            t = mc.candidates(case["nears"][0], 40, 64, case["C"], 8, case["dt_gamma"])
            x = mc.dt_of(t[t < case["fars"][0]], 64, case["C"], 8, case["dt_gamma"]) * F32(8) * F32(0.5)
            assert x.min() < 1 <= x.max(), case["name"]                 # dt * H * 0.5 crosses 1 along ray 0
            continue

        def first(r):
            return float(ref["xyzs"][ref["rays"][r, 1], 0]) if ref["rays"][r, 2] else None
        below1, below2 = float(F32(1 - 2.0 ** -24)), float(F32(2 - 2.0 ** -23))
        assert (first(0) == 1.0) == (level == 1), case["name"]          # |p| == 1.0 is level 1 ...
        assert (first(1) == below1) == (level == 0), case["name"]       # ... one ulp below is level 0
        assert (first(2) == 2.0) == (level == min(2, case["C"] - 1)), case["name"]
        assert (first(3) == below2) == (level == 1), case["name"]
    assert {c["promise"]["level"] for c in mc.cascade_edges()} == {0, 1, 2}


def test_signed_zeros_give_the_same_samples():
    (case,) = mc.signed_zero_dirs()
    ref = ref_of(case["name"])
    r = ref["rays"]
    assert ref["total"] > 0
    nan_paths = 0
    mk = omarch._Marcher(case["o"], case["d"], case["bits"], case["bound"], case["C"], case["H"], case["dt_gamma"], case["max_steps"])
    with np.errstate(invalid="ignore"):
        p = case["o"] + F32(0.5) * case["d"]
        nan_paths = int(np.isnan((np.round(p * 4) / 4 - p) * mk.rd).any(1).sum())
    assert nan_paths >= 8                                               # (face - p) == 0 times 1 / d == inf occurs
    for k in range(case["promise"]["pairs"]):
        a, b = r[2 * k], r[2 * k + 1]
        assert a[2] == b[2]
        sa, sb = slice(a[1], a[1] + a[2]), slice(b[1], b[1] + b[2])
        assert (ref["xyzs"][sa] == ref["xyzs"][sb]).all() and (ref["deltas"][sa] == ref["deltas"][sb]).all()
    assert np.signbit(case["d"]).any() and (case["d"] == 0).any()


def test_capture_edges_replay_and_re_march():
    a, b = mc.capture_edges()
    last = [int(mc.emitted_indices(a, r)[-1]) for r in range(a["o"].shape[0])]
    assert last == a["promise"]["last"]
    for cap, words in ((32, 1), (33, 2), (64, 2), (1024, 32)):
        assert mc.cap_words(cap) == words
    assert [bool(mc.replays(j, 32)) for j in last] == [True, True, False, False, False, False, False, False]
    assert [bool(mc.replays(j, 33)) for j in last] == [True] * 6 + [False] * 2
    lo, hi = b["promise"]["empty_stretch"]
    assert lo % 8 == 0 and hi - lo >= 8
    for r in range(b["o"].shape[0]):
        j = mc.emitted_indices(b, r)
        assert not ((j >= lo) & (j < hi)).any() and (j < lo).any() and (j >= hi).any()
        assert not mc.replays(j[-1], 32) and mc.replays(j[-1], 33)


def test_buffer_cuts_cut_where_promised():
    case = mc.buffer_cuts_scene()
    rays = ref_of(case["name"])["rays"]
    cuts = mc.buffer_cuts(rays)
    total, N = int(rays[:, 2].sum()), rays.shape[0]
    assert N % 16 != 0 and (rays[:, 2] == 0).any() and total > N + 1
    m = cuts["inside_ray"]
    assert ((rays[:, 1] < m) & (m < rays[:, 1] + rays[:, 2])).sum() == 1
    m = cuts["ray_boundary"]
    assert 0 < m < total and (rays[:, 1] + rays[:, 2] == m).any() and not ((rays[:, 1] < m) & (m < rays[:, 1] + rays[:, 2])).any()
    assert len(set(cuts.values())) == len(cuts)
    for m in cuts.values():
        own = mc.owned_rows(rays, m)
        ref = mc.oracle(case, M=m)
        assert (ref["deltas"][~own] == 0).all() and (ref["deltas"][own, 0] > 0).all()


@pytest.mark.parametrize("n", SCAN_CPU)
def test_scan_trips(n):
    case = mc.scan_trips(n)
    mc.check_safety(case)
    ref = mc.oracle(case)
    cnt = ref["rays"][:, 2]
    assert (ref["rays"][:, 1] == np.concatenate([[0], np.cumsum(cnt)[:-1]])).all()
    assert n < 100 or ((cnt > 0).any() and (cnt == 0).any())
    if n in mc.SCAN_N_LANE:
        assert ((n + 255) // 256 > 1024) == (n > 262144)               # more than 1024 blocks of 256: a second trip
    if n <= 4097:
        rr.check_samples(case, ref["rays"], ref["xyzs"], ref["dirs"], ref["deltas"])


@pytest.mark.parametrize("how", ["dropped_sample", "ulp_off", "offset_shifted"])
def test_check_samples_rejects_damage(how):
    for name in ("buffer_cuts", "sparse_hits_slabs_256", "cascade_C3_b4_l1_g0.25"):
        bad = rr.damage(ref_of(name), how)
        with pytest.raises(AssertionError):
            rr.check_samples(CASES[name], bad["rays"], bad["xyzs"], bad["dirs"], bad["deltas"])


def test_check_samples_accepts_records():
    case = CASES["noise_mix"]
    ref = ref_of("noise_mix")
    t = np.concatenate([mc.candidates(mc.start_t(case)[r], 80, 64, 1, 8, 0.0)[mc.emitted_indices(case, r)] for r in range(64)])
    ids = np.repeat(np.arange(64), ref["rays"][:, 2])
    rr.check_samples(case, ref["rays"], None, None, None, t=t, ids=ids)
    t[3] = np.nextafter(t[3], F32(9))
    with pytest.raises(AssertionError):
        rr.check_samples(case, ref["rays"], None, None, None, t=t, ids=ids)


# ---------------------------------------------------------------------------- the float64 references
def test_near_far64_agrees_with_the_oracle_and_excludes_few():
    o, d, aabb, min_near = rr.near_far_random(20000, 3)
    ref = rr.near_far64(o, d, aabb, min_near)
    share = 1.0 - ref["decided"].mean()
    assert share <= rr.NEAR_FAR_MAX_EXCLUDED, share
    assert 0.1 < ref["miss"].mean() < 0.9
    n, f = orays.near_far_from_aabb(o, d, aabb, min_near)
    assert rr.check_near_far(n, f, ref) == share
    print(f"near_far64: excluded share {share:.2e} of {len(o)} rays")


def test_near_far64_rejects_a_wrong_value():
    o, d, aabb, min_near = rr.near_far_random(2000, 4)
    ref = rr.near_far64(o, d, aabb, min_near)
    n, f = orays.near_far_from_aabb(o, d, aabb, min_near)
    k = int(np.nonzero(n != rr.FLT_MAX)[0][0])
    f2 = f.copy()
    f2[k] = f[k] * F32(1 + 8 * rr.U)
    with pytest.raises(AssertionError):
        rr.check_near_far(n, f2, ref)
    n2, f3 = n.copy(), f.copy()
    n2[k] = f3[k] = rr.FLT_MAX
    with pytest.raises(AssertionError):
        rr.check_near_far(n2, f3, ref)


def test_get_rays64_agrees_with_the_oracle():
    poses, intr, H, W, inds = rr.get_rays_inputs()
    ref = rr.get_rays64(poses, intr, W, inds)
    got = orays.get_rays(poses, intr, H, W, inds=inds)
    worst = rr.check_get_rays(got["rays_o"], got["rays_d"], ref)
    assert worst > 0
    bad = got["rays_d"].copy()
    bad[1, 2, 0] += F32(40 * rr.U)
    with pytest.raises(AssertionError):
        rr.check_get_rays(got["rays_o"], bad, ref)


def test_alive_patterns():
    for p in mc.COMPACT_PATTERNS:
        for n in (1, 2, 65):
            a = mc.alive_pattern(n, p)
            assert a.dtype == np.int32 and len(a) == n
    assert (mc.alive_pattern(5, "ends") >= 0).tolist() == [True, False, False, False, True]
