"""tests/field_forward_reference.py checked on the CPU: the level-table and row-index restatements against
gridencoder.level_table and oracle.hashgrid (two independent restatements agree on every table used), the float64 forward
against the torch oracle, the arithmetic models within TOL / margin (so the constants cannot drift from the measurement),
the exact tier's preconditions and that it is not vacuous, and that every entry point has cases at every size."""
import functools
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_forward_reference as R  # noqa: E402

F32, F64 = np.float32, np.float64
MID = 16 * 61 + 7


def test_level_tables_are_the_projects():
    import field_issue_cases as C
    from instance_nerf_amd.gridencoder import level_table
    assert R.TABLE_SPECS == C.TABLES
    for name in R.TOL_TABLES + R.EXACT_TABLES:
        spec = R.TABLE_SPECS.get(R.ALIASES.get(name, name)) or R.EXACT_SPECS[name]
        mine, theirs = R.table_for(name), level_table(**spec)
        assert set(mine) == set(theirs)
        for k in mine:
            assert np.array_equal(np.asarray(mine[k]), np.asarray(theirs[k])), (name, k)
    for name in R.EXACT_TABLES:                         # integer scales base * 2^l - 1, dense and hashed levels
        t = R.table_for(name)
        assert (t["scales"] == 2.0 * 2.0 ** np.arange(t["num_levels"]) - 1).all()
        assert t["hashed"][:3].tolist() == [0, 0, 0] and t["hashed"][3:].all()
    assert R.sliceable("x16") and not R.sliceable("x12") and R.sliceable("bench") and not R.sliceable("all_dense")


def test_row_index_and_weights_agree_with_the_oracle():
    """cells / row_index / the float64 corner weights against oracle.hashgrid.corner_indices_weights on every table,
    out-of-range and NaN rows included."""
    from oracle.hashgrid import corner_indices_weights
    for name in R.TOL_TABLES + R.EXACT_TABLES:
        t, bound = R.table_for(name), R.SETTINGS[name][0]
        sc = R.scene(name, MID, bound, R.grid_for(name, "fwd_rgb"))
        x = R.plain_x(sc, bound)
        x01, oob = R.x01_plain(x, bound)
        assert oob.sum() == 2
        cell, fr = R.cells(x01, t)
        idx = R.row_index(cell, t)
        want_i, want_w = corner_indices_weights(torch.from_numpy(x), bound, t)
        assert np.array_equal(idx, want_i.numpy()), name
        for l in range(t["num_levels"]):               # dense rows stay inside their level without the oracle's modulo
            assert idx[:, l].min() >= t["offsets"][l] and idx[:, l].max() < t["offsets"][l + 1]
        f1 = fr.astype(F64)
        f0 = 1.0 - f1
        w = np.stack([(f1 if k & 1 else f0)[..., 0] * (f1 if k & 2 else f0)[..., 1] * (f1 if k & 4 else f0)[..., 2]
                      for k in range(8)], -1)
        w[oob] = 0.0
        assert np.abs(w - want_w.numpy()).max() < 3e-7, name
        if R.tier_of(name) == "tol":                    # the special rows: faces and exact cell boundaries are present
            assert (fr[:7] == 0.5).any() and (x01[:2] == [[0, 0, 0], [1, 1, 1]]).all()


def test_float64_forward_equals_the_torch_oracle():
    """encode and the two networks in float64 against oracle.hashgrid.encode + plain torch float64 layers."""
    from oracle.hashgrid import encode
    from train_kernels_reference import sh64
    for name in ("bench", "levels12", "x12"):
        ref = R.Reference(name, 200)
        x = R.plain_x(ref.sc, ref.bound)
        o, c = ref.nerf("plain")
        L2 = 2 * ref.t["num_levels"]
        want = encode(torch.from_numpy(x), torch.from_numpy(R.embeddings(name)), ref.bound, ref.t).numpy()
        assert np.abs(o["enc"][:, :L2] - want).max() < 2e-6 and not o["enc"][:, L2:].any()
        W = [torch.tensor(np.asarray(w, F64)) for w in ref.W]
        enc = torch.tensor(o["enc"])
        so = torch.relu(enc @ W[0].t()) @ W[1].t()
        cin = torch.cat([torch.tensor(sh64(ref.sc["dirs"], 4)), so[:, 1:]], 1)
        rgb = torch.sigmoid(torch.relu(torch.relu(cin @ W[2].t()) @ W[3].t()) @ W[4].t())
        assert np.abs(o["so"] - so.numpy()).max() <= 1e-12 * np.abs(so.numpy()).max()
        assert np.abs(o["rgb"] - rgb.numpy()).max() <= 1e-12
        assert np.abs(o["sigma"] - (torch.exp(so[:, 0]) * float(F32(ref.ds))).numpy()).max() <= 1e-12 * o["sigma"].max()
        assert all((c[k] >= 0).all() and c[k].shape == o[k].shape for k in o if k in c)
        assert (np.abs(o["so"]) <= c["so"] * (1 + 1e-12)).all()      # cond bounds the value it belongs to
        oob = R.x01_plain(x, ref.bound)[1]
        assert not o["enc"][oob].any() and not c["geo"][oob].any() and (o["sigma"][oob] == F32(ref.ds)).all()


@functools.lru_cache(maxsize=None)
def measured(build):
    return R.measure_all(build)


def test_models_stay_within_the_measured_constants():
    for b in R.BUILDS:
        worst = measured(b)
        print(b, {k: f"{v:.3e}" for k, v in sorted(worst.items())})
        assert set(worst) == set(R.MEASURED[b])
        for k, v in worst.items():
            margin = R.MARGIN[k.partition("@")[2]]
            assert v <= R.MEASURED[b][k] == R.TOL[b][k] / margin, (b, k, v)
            assert v > 0.2 * R.MEASURED[b][k], (b, k, v, "the constant is stale")
    assert R.MARGIN == {"": 8.0, "t16": 2.0, "m16": 2.0, "o": 2.0}
    assert not any("@m16" in k or "@o" in k for k in R.MEASURED["fp32"])


def test_fp16_models_round_to_nearest_even():
    assert R.rne_f16(np.asarray([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65520.0, 2.0 ** -25])).tolist() == \
        [1.0, 1.0 + 2.0 ** -9, np.inf, 0.0]
    m = R.HalfMlp()
    W, x = np.asarray([[1.0 + 2.0 ** -11, 3.0]], F32), np.asarray([[2.0, 1.0 + 3 * 2.0 ** -11]], F32)
    assert m.layer(W, x)[0, 0] == float(F32(2.0 + 3.0 * (1.0 + 2.0 ** -9)))
    assert R.model_for("bf16x3", "o")[1] and not R.model_for("bf16x3", "m16")[1] and R.model_for("fp32", "t16")[1]


def test_tolerance_tier_inputs():
    """so0 passes +-15 on both sides somewhere, bound and density_scale take both values, dead columns are zero."""
    both = [0, 0]
    for name in R.TABLE_SPECS:
        so0 = R.reference(name, MID).sigma("table")[0]["so"][:, 0]
        both[0] += (so0 > 15).any()
        both[1] += (so0 < -15).any()
        L2 = 2 * R.table_for(name)["num_levels"]
        assert not R.nerf_weights(name)[0][:, L2:].any() and not R.instance_weights(name, 48)[0][:, L2:].any()
        assert R.nerf_weights(name)[0][:, :L2].all()
    assert min(both) >= 1, both
    st = [R.SETTINGS[n] for n in R.TOL_TABLES]
    assert {b for b, _ in st} == {1.0, 2.0, 1.5} and {d for _, d in st} == {1.0, 0.3}
    assert R.SETTINGS["levels5_b15"][0] == 1.5 and R.sizes_for("levels5_b15", "fwd_rgb") == (17, MID)


def test_exact_tier_preconditions():
    """No violation on the float64 run's own operands (with the fp16 rules for the fp16 MLP); the float64 result is an
    fp32 number; sigma == density_scale and rgb == 0.5 exactly; the tier is not vacuous."""
    for name in R.EXACT_TABLES:
        bound, ds = R.SETTINGS[name]
        assert ds == 2.0 ** round(np.log2(ds)) and bound == 2.0 ** round(np.log2(bound))
        emb = R.embeddings(name)
        assert (emb == np.round(emb)).all() and np.abs(emb).max() == 2 and (emb.astype(np.float16) == emb).all()
        for entry in R.ENTRIES:
            if not R.applies(name, entry):
                continue
            fp16 = entry in R.NERF_ENTRIES and bool(R.NUMERICS[R.NERF_ENTRIES[entry][1]] & 2)
            for M in (33, MID):
                log = []
                ref = R.Reference(name, M, log=log, variant=R.variant_for(name, entry), grid=R.grid_for(name, entry))
                out, cond = R.expected(ref, entry)
                assert R.exactness_violations(log, fp16) == [], (name, entry)
                assert any(k == "blend" for k, _, _ in log) and any(k == "layer" for k, _, _ in log)
                for k, v in out.items():
                    v = v[:, 16:] if k == "cin" else v
                    if k != "rgbm":                      # 1.5 * fp32(1/3) rounds to 0.5 in fp32, in one step
                        assert (v.astype(F32).astype(F64) == v).all(), (name, entry, k)
                    if k in ("sigma", "sigma1"):
                        assert (v == (ds if k == "sigma" else 1.0)).all()
                    elif k in ("rgb", "rgbm"):
                        assert (v.astype(F32) == F32(0.5)).all()
                    elif M == MID:
                        assert len(np.unique(v)) > 8, (name, entry, k)       # a live output, not a constant
                if "logit" in out and M == MID and entry == "lattice":
                    assert (out["logit"] == R.LOGIT_MIN["exact"]).any() and (out["logit"] > R.LOGIT_MIN["exact"]).any()
    assert R.exactness_violations([("blend", np.asarray([[3.0]]), np.asarray([[1.0 + 2.0 ** -17]]))]) != []
    assert R.exactness_violations([("layer", np.ones((1, 1)), np.asarray([[1.0 + 2.0 ** -12]]))], fp16=True) != []
    assert R.exactness_violations([("layer", np.ones((1, 1)), np.asarray([[1.0 + 2.0 ** -12]]))]) == []


def test_every_entry_point_has_cases_at_every_size():
    for build in R.BUILDS:
        cases = R.cases(build)
        for tier, tables in (("tol", R.TOL_TABLES), ("exact", R.EXACT_TABLES)):
            for e in R.ENTRIES:
                if build == "fp32" and e in R.NERF_ENTRIES and R.NUMERICS[R.NERF_ENTRIES[e][1]] & 2:
                    assert not [c for c in cases if c[1] == e]
                    continue
                mine = [t for t, ee in cases if ee == e and t in tables]
                assert mine, (build, tier, e)
                if e != "lattice":
                    assert any(set(R.sizes_for(t, e)) >= set(R.SMALL_SIZES) for t in mine), (tier, e)
    assert {K for _, K in R.INSTANCE_ENTRIES.values()} == {16, 32, 48, 64}
    assert {m for m, _ in R.INSTANCE_ENTRIES.values()} == {"", "_train", "_enc"}
    assert {e for e in R.NERF_ENTRIES if e.startswith("dirs")} == {"dirs1", "dirs3", "dirs8"}
    assert {R.NERF_ENTRIES[e][1] for e in R.NERF_ENTRIES if e.startswith("table")} == {"", "t16", "m16", "o"}
    big = [(t, e) for t, e in R.cases() if R.BIG in R.sizes_for(t, e)]
    assert big == [("bench", "fwd_rgb"), ("bench", "table"), ("bench", "records")]
    ax = R.lattice_axes("bench", 1.0)
    assert len(ax[0]) % 16 and (np.abs(ax[0]) > 1.0).any() and np.isfinite(R.LOGIT_MIN["tol"])
    assert {R.variant_for("x16", e) for e in R.NERF_ENTRIES} == {"a", "b", "c", "logit"}


def test_the_hybrid_size_is_the_smallest_on_the_cursor_schedule():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "instance_nerf_amd", "csrc",
                            "field_fused.hip")).read()
    chunk = int(re.search(r"constexpr int kXcdChunkLog2 = (\d+);", src).group(1))
    m = re.search(r"if \(\(n_tiles >> \(kXcdChunkLog2 \+ (\d+)\)\) < (\d+) \|\| stream_is_capturing", src)
    n = int(m.group(2)) << (chunk + int(m.group(1)))
    assert n == R.HYBRID_MIN_TILES == 32768 and R.BIG == 16 * n + 7
    assert (R.BIG + 15) // 16 >= n > (max(R.SMALL_SIZES) + 15) // 16      # every other size takes the static deal


def test_rounding_tier_is_exact_after_the_rounding_and_sees_a_truncation():
    """The fp16 MLP's rounding tier: inputs that need their rounding, sums exact in any order after it, and the
    truncating conversion misses ROUNDING_TOL on more than a fifth of the rows."""
    for name in R.EXACT_TABLES:
        for entry in R.ROUNDING_ENTRIES:
            log = []
            good, ref = R.rounding_reference(name, entry, MID, log=log)
            assert R.B.exactness_violations(log) == [], (name, entry)
            enc = ref._enc(R.NERF_ENTRIES[entry][0])[0]
            assert (R.rne_f16(enc) != enc).mean() > 0.02 and R.sigbits(enc) > 11      # the rounding is real
            bad, _ = R.rounding_reference(name, entry, MID, truncate=True)
            for k in good:
                miss = np.abs(bad[k] - good[k]) > R.ROUNDING_TOL * np.abs(good[k])
                assert miss.mean() > 0.2, (name, entry, k, miss.mean())
            assert len(np.unique(good["rgb"])) > 50 and len(np.unique(good["sigma"])) > 50
    assert R.ROUNDING_TOL == 8 * 2.0 ** -24
