"""tests/project_masks_reference.py is right and its cases meet the conditions tests/test_project_masks_kernels.py relies
on: the layout against the closed-form slot map of tests/composite_reference.py, the fp32-order cell against the
float64 cell (they part only next to a cell face, on at most 0.5 % of a case's samples that were not put on a face on
purpose), the exact tier's exactness, the derived bound of the general tier, and the coverage the issue lists (every
mask bit, every face, all six outer sides, dropped groups that leave a group standing) - all on the CPU."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_reference as cr  # noqa: E402
import project_masks_reference as R  # noqa: E402

F, D = np.float32, np.float64
CASES = R.all_cases()
IDS = [R.case_id(kw) for kw in CASES]


@functools.lru_cache(maxsize=None)
def _case(i):
    return R.make_case(**CASES[i])


def test_case_names_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("N", R.N_SIZES)
def test_layout_against_the_composite_slot_map(N):
    c = R.make_case(N)
    rays, slots = c["rays"], c["slots"]
    want = cr.patch_slot_map(rays)                       # ray-major sample rays[n, 1] + k -> patch row
    got = np.concatenate([s for s in slots]) if c["total"] else np.zeros(0, np.int64)
    assert np.array_equal(got, want)
    assert sorted(got.tolist()) == list(range(c["total"])), "the rows are not a permutation"
    for g, (base, tot) in enumerate(R.group_spans(rays)):
        rows = np.concatenate([slots[n] for n in range(g * 16, min(g * 16 + 16, N))])
        assert tot == 0 or (rows.min() == base and rows.max() == base + tot - 1)
    for M in (0, c["total"] // 2, c["total"]):
        assert np.array_equal(R.dropped_rays(rays, M), cr.dropped_groups(rays, M))
    ids = rays[:, 0]
    assert len(set(ids.tolist())) == N and ids.max() < c["n_rows"] and (N < 3 or not np.array_equal(ids, np.arange(N)))
    if N >= 48:
        assert c["counts"][16:32] == [0] * 16 and max(c["counts"][32:48]) == 200 and sorted(c["counts"][32:48])[-2] <= 2
    assert c["total"] <= 4000 and max(c["counts"]) <= 256
    assert set(c["counts"]) <= {0, 1, 2, 17, 64, 200}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_case_conditions(i):
    c = _case(i)
    M, rays = c["M"], c["rays"]
    drop = R.dropped_rays(rays, M)
    if c["m_mode"].startswith(("drop", "keep")):
        spans = R.group_spans(rays)
        kept = [t > 0 and b + t <= M for b, t in spans]
        gone = [b + t > M for b, t in spans]
        assert any(kept) and any(gone), "a case that drops groups keeps at least one"
        assert sum(g and t > 0 for g, (b, t) in zip(gone, spans)) >= {"drop1": 1, "drop2": 2, "keep1": 3}[c["m_mode"]]
        if c["m_mode"] == "keep1":
            assert sum(kept) == 1
    if c["m_mode"] == "padded":
        assert M > c["total"] and not drop.any()
    if M == 0:
        return
    c32, i32 = R.cells32(c["xyz"], *c["box"], c["vol"])
    c64, i64, u = R.cells64(c["xyz"], *c["box"], c["vol"])
    amb = R.ambiguous(c)
    assert not (amb & ~R.near_face(u, c["vol"])).any(), "the cells part away from a face"
    assert (amb & ~c["deliberate"]).sum() <= R.MAX_AMBIGUOUS * M
    out32, out64 = R.project32(c), R.project64(c)
    kt, kb, kc = c["k"]
    written = np.zeros(out32.shape, bool)
    written[rays[:, 0], kb:kb + kc] = True
    assert (out32.view(np.uint32)[~written] == R.SENTINEL).all() and np.isnan(out64[~written]).all()
    assert np.isfinite(out32[written]).all() and np.isfinite(out64[written]).all()
    assert (out32[rays[drop, 0], kb:kb + kc] == 0).all()
    if c["tier"] == "exact":
        assert not amb.any() and not c["deliberate"].any()
        w = c["w"][:c["total"]].astype(D) * 4096                  # (rows behind the total are padding no ray owns)
        assert (w == np.round(w)).all() and (w >= 0).all() and (w < 4096).all() and max(c["counts"]) <= 256
        assert np.array_equal(out32[written].astype(D), out64[written]), "the exact tier is not exact"
    else:
        clear = ~R.rays_with(c, amb)
        err = np.abs(out32.astype(D) - out64)
        err = np.where(written, err, 0.0).max(-1)
        assert (err[clear] <= R.sum_bound(c)[clear]).all()
    if c["box"] is R.DEGENERATE_BOX:
        assert not i32.any() and not i64.any() and (out32[written] == 0).all()


def test_coverage_of_the_cases():
    bits = 0
    sides = np.zeros((3, 2), bool)
    faces = {"lo": False, "hi": False, "below_hi": False, "interior": False}
    nan_behind_zero = False
    seen_k, seen_vol, seen_m = set(), set(), set()
    for i in range(len(CASES)):
        c = _case(i)
        seen_k.add(c["k"]), seen_vol.add(c["vol"]), seen_m.add(c["m_mode"])
        if not c["M"] or c["box"] is R.DEGENERATE_BOX:
            continue
        lo, hi = c["box"]
        cells, inside = R.cells32(c["xyz"], lo, hi, c["vol"])
        live = np.zeros(c["M"], bool)                      # samples of kept rays with a weight
        drop = R.dropped_rays(c["rays"], c["M"])
        for n in range(c["N"]):
            if not drop[n]:
                live[c["slots"][n]] = True
        live &= c["w"] != 0
        word = R.words_at(c["words"], cells, inside, c["vol"])
        for wd in word[live & inside]:
            bits |= int(wd) & ((1 << c["k"][2]) - 1)
        x = c["xyz"]
        if c["tier"] == "general":
            for a in range(3):
                sides[a, 0] |= bool((live & (x[:, a] < lo[a])).any())
                sides[a, 1] |= bool((live & (x[:, a] > hi[a])).any())
                on_lo, on_hi = live & (x[:, a] == lo[a]), live & (x[:, a] == hi[a])
                faces["lo"] |= bool((on_lo & inside & (cells[:, a] == 0)).any())
                faces["hi"] |= bool((on_hi & ~inside).any())
                faces["below_hi"] |= bool((live & (x[:, a] == np.nextafter(hi[a], lo[a]))).any())
            faces["interior"] |= bool((live & c["deliberate"] & inside & (cells > 0).any(-1)).any())
        nan_behind_zero |= bool((np.isnan(x).any(-1) & (c["w"] == 0)).any())
        assert not (np.isnan(x).any(-1) & live).any()
    assert bits == 0xFFFFFFFF, hex(bits)
    assert sides.all() and all(faces.values()), (sides, faces)
    assert nan_behind_zero
    assert seen_k == set(R.K_COMBOS) and seen_vol == set(R.VOLUMES) and seen_m == set(R.M_MODES)
    # a sample on hi of the FIRST axis with a weight (fx < res, not <=) in the anisotropic volumes
    c = R.make_case(65)
    lo, hi = c["box"]
    assert ((c["xyz"][:, 0] == hi[0]) & (c["w"] != 0)).any()
    assert len({*c["vol"]}) == 3


def test_words_hold_the_special_patterns():
    for vol in R.VOLUMES[1:]:
        w = R._words(vol, 5, None).reshape(-1)
        assert w.dtype == np.int32 and w[0] == -1 and w[1] == 0 and w[2] == -(1 << 31) and (w < 0).sum() > 3
    assert R._words((1, 1, 1), 5, "ones")[0, 0, 0] == -1 and R._words((1, 1, 1), 5, "zeros")[0, 0, 0] == 0
    assert R._words((1, 1, 1), 5, None)[0, 0, 0] < 0
