"""tests/instance_lattice_reference.py checked on the CPU: the reference against the project's independent forms
(extract.volume_stats, extract.sweep_lattice's arg-max, the C oracle), the arithmetic models within TOL / margin for the
confidence, the exact tier's preconditions and its ties, the tie kinds, and every band, cap and gap condition that
tests/test_instance_lattice_kernels.py relies on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_forward_reference as R  # noqa: E402
import instance_lattice_reference as I  # noqa: E402

F32, F64 = np.float32, np.float64
CASES = I.cases()
TOL_CASES = [c for c in CASES if I.tier_of(c[0]) == "tol"]
EXACT_CASES = [c for c in CASES if I.tier_of(c[0]) == "exact"]


def test_case_list_covers_what_the_kernel_tests_promise():
    assert {c[1] for c in CASES} == set(I.MAIN_LATTICES + I.SMALL_LATTICES)
    assert {c[2] for c in CASES} == {1, 5, 16, 31, 48, 64}
    for tier in (TOL_CASES, EXACT_CASES):
        assert {c[2] for c in tier} == {1, 5, 16, 31, 48, 64} and {c[1] for c in tier} >= set(I.MAIN_LATTICES + I.SMALL_LATTICES)
    assert {c[0] for c in TOL_CASES} == set(I.TOL_TABLES) and {c[0] for c in EXACT_CASES} == set(I.EXACT_TABLES)
    assert {R.SETTINGS[t][0] for t in I.TOL_TABLES} == {1.0, 1.5, 2.0} and {R.SETTINGS[t][1] for t in I.TOL_TABLES} == {1.0, 0.3}
    # the instance field's level table differs from the NeRF's in both tiers, and its values are another draw
    for t in ("bench", "dense_coarse", "x16"):
        a, b = R.table_for(t), R.table_for(I.INST_TABLE[t])
        assert a["total_rows"] != b["total_rows"] or not np.array_equal(a["scales"], b["scales"])
    for t in I.TOL_TABLES + I.EXACT_TABLES:
        e, n = I.inst_embeddings(t), R.embeddings(I.INST_TABLE[t])
        assert e.shape == n.shape and not np.array_equal(e, n)
    for b in I.BUILDS:
        assert I.TOL[b]["conf"] == 8.0 * I.MEASURED[b]["conf"] and I.TOL[b]["logit"] == R.TOL[b]["logit"]
    # one axis value outside the bound on the main lattices
    for t, dims, _ in CASES:
        ax = I.axes(t, dims)
        assert [len(a) for a in ax] == list(dims)
        if dims[0] > 4:
            assert abs(ax[0][4]) > R.SETTINGS[t][0]


def test_the_interleaved_case_is_the_smallest_kind_on_that_split():
    table, dims, K = I.BIG_CASE
    n_tiles = (dims[0] + 15) // 16 * dims[1] * dims[2]
    assert I.interleaved_min_tiles() == I.HYBRID_MIN_TILES == 4 << 13
    assert n_tiles == 33024 >= 4 << 13 > I.SMALL_TILES and max((d[0] + 15) // 16 * d[1] * d[2] for d in I.MAIN_LATTICES) < 4 << 13
    ref = I.big_reference()
    th, mid, gap, n_occ = ref.tail_threshold()
    assert gap > ref.gap_need(mid), (gap, ref.gap_need(mid))
    occ = ref.occupied(th)
    assert n_occ == occ.sum() >= 16 and np.array_equal(occ, ref.so0 > mid)
    k = I.tile_kinds(dims, occ)
    assert k["empty"] >= 30000 and k["mixed"] >= 16 and k["tail_empty"] >= 1, k
    assert I.tile_kinds(dims, ref.occupied(0.0))["full"] == n_tiles
    assert (ref.margin <= ref.band()).mean() <= 0.05


# ---------------------------------------------------------------------------- against the project's independent forms
@pytest.mark.parametrize("name", I.STATS_CASES)
def test_stats_restatement_against_volume_stats_on_the_host(name):
    """counts and boxes equal; sums within the fp32 / float64 difference: a summation tree of depth d is within d * 2^-24
    * sum |x| of the exact sum (butterfly 6, chunks, waves 4, workgroups / 8, groups 8, and the host's one rounding)."""
    from instance_nerf_amd import extract
    lab, conf, K = I.stats_inputs(name)
    counts, boxes, sums = I.stats_reference(lab, conf, K)
    hc, hb, hs = extract.volume_stats(torch.from_numpy(lab), torch.from_numpy(conf), K)
    assert np.array_equal(hc.numpy(), counts) and np.array_equal(hb.numpy(), boxes)
    nb, per = I.stats_blocks(lab.size)
    depth = 6 + max(1, -(-per // 256)) + 4 + -(-nb // 8) + 8 + 1
    flat, cf = lab.reshape(-1), conf.reshape(-1).astype(F64)
    for c in range(K):
        exact = cf[flat == c].sum()
        bound = depth * 2.0 ** -24 * np.abs(cf[flat == c]).sum()
        assert abs(float(sums[c]) - exact) <= bound and abs(float(hs[c]) - float(sums[c])) <= 2 * bound, (name, c)


def test_stats_workgroup_ranges():
    assert I.stats_blocks(0) == (1, 0) and I.stats_blocks(1) == (1, 1) and I.stats_blocks(1024) == (1, 1024)
    assert I.stats_blocks(1025) == (2, 513)
    nb, per = I.stats_blocks(65 * 64 * 127)
    assert (nb, per) == (512, 1032) and per % 64 != 0


def test_stats_restatement_has_teeth():
    """A plain sequential fp32 sum differs from the launch's order in at least one channel's bits on every statistics
    input with more than a handful of live voxels."""
    for name in I.STATS_CASES:
        if name in ("n0", "n1", "empty"):
            continue
        lab, conf, K = I.stats_inputs(name)
        _, _, sums = I.stats_reference(lab, conf, K)
        flat, cf = lab.reshape(-1), conf.reshape(-1)
        seq = np.asarray([np.cumsum(cf[flat == c], dtype=F32)[-1] if (flat == c).any() else 0.0 for c in range(K)], F32)
        assert (seq.view(np.uint32) != sums.view(np.uint32)).any(), name


def test_stats_inputs_are_what_their_names_say():
    lab, conf, K = I.stats_inputs("ignored")
    assert ((lab >= K) & (lab < 255)).sum() > 250 and (conf[(lab >= K)] > 0).any()
    lab, conf, K = I.stats_inputs("corners")
    assert np.argwhere(lab == 3).tolist() == [[0, 0, 0], [d - 1 for d in lab.shape]]
    lab, conf, K = I.stats_inputs("spread")
    e = np.frexp(conf[lab < K])[1]
    assert K == 64 and e.min() <= -11 and e.max() >= 11
    assert (I.stats_inputs("empty")[0] == 255).all()
    for name in ("n0", "n1", "n63", "n64", "n65", "n1023", "n1024", "n1025"):
        lab = I.stats_inputs(name)[0]
        assert lab.size == int(name[1:]) and (lab.size == 1 or lab.shape[1] != lab.shape[2])


def test_argmax_against_the_composable_sweep_on_the_stub_model():
    from instance_nerf_amd import extract
    from test_extract_sweep_cpu import BOX_MAX, BOX_MIN, CHUNK, RES, THRESH, Stub
    m = Stub()
    _, _, labels, conf = extract.sweep_lattice(m, np.float32(BOX_MIN), np.float32(BOX_MAX), RES, CHUNK, thresh=THRESH)
    pts = extract.lattice(BOX_MIN, BOX_MAX, RES, "cpu").clamp(-1.0, 1.0)
    logits = m.instance(pts)[:, :3].double().numpy()
    lab, cf, _, _, _ = I.confidence(logits, np.abs(logits))
    occ = labels.reshape(-1).numpy() != 255
    assert occ.sum() == 15
    assert np.array_equal(labels.reshape(-1).numpy()[occ], lab[occ])
    assert np.abs(conf.reshape(-1).numpy()[occ] - cf[occ]).max() <= 1e-6
    # ties: the lowest channel
    assert I.confidence(np.asarray([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0]]), np.ones((2, 3)))[0].tolist() == [1, 0]


def test_float64_reference_against_the_c_oracle():
    """bench NeRF table, hashed_all instance table: the fp32 C oracle within 1e-5 * cond (sums of at most 64 fp32 terms per
    layer: 64 * 2^-24 = 4e-6 of the contraction over absolute values, per layer)."""
    from oracle import c_port
    table, dims, K = "bench", (19, 3, 5), 16
    ref = I.reference(table, dims, K)
    b = F32(ref.bound)
    pts = np.stack(np.meshgrid(*[np.clip(a, -b, b) for a in ref.ax], indexing="ij"), -1).reshape(-1, 3).astype(F32)
    p = {"embeddings": R.embeddings(table), "sigma_w0": ref.Wn[0], "sigma_w1": ref.Wn[1], "color_w0": ref.Wn[2],
         "color_w1": ref.Wn[3], "color_w2": ref.Wn[4], "inst_embeddings": I.inst_embeddings(table), "inst_w0": ref.Wi[0],
         "inst_w1": ref.Wi[1], "inst_w2": ref.Wi[2]}
    d = np.tile(np.asarray([[0.0, 0.0, 1.0]], F32), (len(pts), 1))
    sigma, _ = c_port.nerf_forward(pts, d, p, ref.bound, R.table_for(table))
    live = sigma > 1e-30
    assert live.mean() > 0.9
    assert (np.abs(np.log(sigma.astype(F64)) - ref.so0)[live] <= 1e-5 * ref.cso0[live] + 1e-6).all()
    logits = c_port.instance_logits(pts, p, ref.bound, R.table_for(I.INST_TABLE[table])).astype(F64)
    assert logits.shape == ref.logits.shape and (np.abs(logits - ref.logits) <= 1e-5 * ref.clogits).all()


# ---------------------------------------------------------------------------- models and conditions on the reference
@pytest.mark.parametrize("build", I.BUILDS)
def test_models_stay_within_the_measured_confidence_error(build):
    seen = I.measure_conf(build)
    print(f"{build}: |model confidence - float64| / cond_conf {seen:.3e} (MEASURED {I.MEASURED[build]['conf']:.3e})")
    assert 0.5 * I.MEASURED[build]["conf"] < seen <= I.MEASURED[build]["conf"]


def test_exact_cases_are_exact_and_have_ties():
    """Every operand pair of every exact case keeps the exact tier's preconditions (so every logit is exact), and the
    reference itself has ties on at least 1 % of the voxels of every exact main-lattice case with K > 1."""
    extra = [(t, (48, 5, 7), I.TIE_K, "default", ("tie",) + p) for t in I.EXACT_TABLES for p in I.TIE_PAIRS]
    extra += [(t, (33, 2, 3), K, "default", "neg") for t in I.EXACT_TABLES for K in (1, 5, 31)]
    extra += [(t, (19, 3, 5), 16, None, "plain") for t in I.EXACT_TABLES]
    for table, dims, K, variant, w2 in [c + ("default", "plain") for c in EXACT_CASES] + extra:
        log = []
        ref = I.LatticeRef(table, dims, K, variant=variant, w2=w2, log=log)
        assert R.exactness_violations(log) == [], (table, dims, K, w2)
        assert np.array_equal(ref.logits.astype(F32).astype(F64), ref.logits) and np.abs(ref.logits).max() < 2 ** 12
        assert np.array_equal(ref.so0.astype(F32).astype(F64), ref.so0)
        if K > 1 and dims in I.MAIN_LATTICES and w2 == "plain" and variant == "default":
            ties = float((ref.margin == 0).mean())
            assert ties >= 0.01, (table, dims, K, ties)
        if w2 == "neg":
            assert (ref.logits <= 0).all() and (ref.logits < 0).all(1).sum() >= 1, (table, K)
        if variant is None:
            assert (ref.so0 == 0).all()
            assert ref.occupied(F32(ref.ds)).all() and not ref.occupied(np.nextafter(F32(ref.ds), F32(np.inf))).any()


@pytest.mark.parametrize("table", I.EXACT_TABLES)
def test_every_tie_kind_wins_somewhere(table):
    for a, b in I.TIE_PAIRS:
        ref = I.reference(table, (48, 5, 7), I.TIE_K, w2=("tie", a, b))
        mx = ref.logits.max(1)
        assert ((ref.logits[:, a] == mx) & (ref.logits[:, b] == mx) & (ref.label == a)).sum() >= 1, (a, b)
    # the four ways two channels of a voxel meet in the kernel's registers: c = 16 mt + 4 q + r
    where = [((a >> 4, (a >> 2) & 3), (b >> 4, (b >> 2) & 3)) for a, b in I.TIE_PAIRS]
    assert where[0][0] == where[0][1]                                    # same lane, same tile
    assert where[1][0][0] == where[1][1][0] and where[1][0][1] != where[1][1][1]     # across q
    assert where[2][0][1] == where[2][1][1] and where[2][0][0] != where[2][1][0]     # across mt
    assert I.TIE_PAIRS[3] == (I.TIE_K - 2, I.TIE_K - 1) and I.TIE_K % 16 == 15


@pytest.mark.parametrize("case", TOL_CASES, ids=[I.case_id(c) for c in TOL_CASES])
def test_label_band_is_narrow(case):
    ref = I.reference(*case)
    for build in I.BUILDS:
        share = float((ref.margin <= ref.band(build)).mean())
        assert share <= 0.05, (case, build, share)


@pytest.mark.parametrize("case", CASES, ids=[I.case_id(c) for c in CASES])
def test_threshold_gaps(case):
    """Both quantile thresholds lie in a gap wider than the need; 0 occupies all, the top threshold none."""
    ref = I.reference(*case)
    for q in (0.5, 0.9):
        th, mid, gap = ref.threshold(q)
        assert gap > ref.gap_need(mid), (case, q, gap, ref.gap_need(mid))
        occ = ref.occupied(th)
        assert np.array_equal(occ, ref.so0 > mid)
    th = ref.thresholds()
    assert ref.occupied(th["zero"]).all() and not ref.occupied(th["above"]).any() and np.isfinite(th["above"])
    if ref.N >= 285:
        assert 0.3 < ref.occupied(th["q50"]).mean() < 0.7 and 0.03 < ref.occupied(th["q90"]).mean() < 0.35


def test_the_skip_sees_empty_mixed_and_full_tiles_and_an_empty_padded_tail():
    kinds = {c: I.tile_kinds(c[1], I.reference(*c).occupied(I.reference(*c).threshold(0.9)[0]))
             for c in TOL_CASES if c[1] in I.MAIN_LATTICES}
    assert len(kinds) == 12
    for c, k in kinds.items():
        assert k["empty"] >= 1 and k["mixed"] >= 1, (c, k)
        if c[1][0] % 16:
            assert k["tail_empty"] >= 1, (c, k)
    assert any(k["full"] >= 1 for k in kinds.values()), kinds
