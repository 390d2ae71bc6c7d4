"""The fused field's forward kernels on the GPU against tests/field_forward_reference.py, every entry point through the
C ABI (tests/field_forward_child.py): inr_nerf_forward (rgb, density + geo, -O), inr_nerf_forward_table x four numerics,
_table_sliced, _table_records with the pair kernel and with INR_FIELD_PAIR=0 (rows from inr_ray_table_q),
inr_nerf_forward_train / _enc, inr_instance_forward / _train / _enc for K = 16 .. 64, inr_nerf_forward_dirs for 1, 3, 8
directions and inr_nerf_forward_lattice.  Exact tier: bit equality with the float64 result rounded to fp32.  Tolerance
tier: |got - ref| <= TOL * cond elementwise.  Sizes 1 .. 33 around the tile and pair boundaries, 16*61+7, and once each
for the plain rgb, table and records feed the smallest launch on the hybrid schedule; 0; the device-side sample count;
the fp16-table identity; dead levels; the fp32 library through a child."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_forward_child as L  # noqa: E402
import field_forward_reference as R  # noqa: E402
from kernel_harness import nan_out, poisoned, run_result_child, stream  # noqa: E402
from train_kernels_reference import assert_same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = R.cases("bf16x3")
MID = 16 * 61 + 7


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


def hybrid_min_tiles():
    """The smallest tile count for which HybridSchedule::begin takes the cursor set, read from the source."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "instance_nerf_amd", "csrc",
                            "field_fused.hip")).read()
    chunk = int(re.search(r"constexpr int kXcdChunkLog2 = (\d+);", src).group(1))
    m = re.search(r"bool begin\(hipStream_t s, int64_t n_tiles\) \{[^\n]*\n\s*if \(\(n_tiles >> \(kXcdChunkLog2 \+ (\d+)\)\) < (\d+) \|\|",
                  src)
    return int(m.group(2)) << (chunk + int(m.group(1)))


@pytest.mark.parametrize("table,entry", CASES, ids=[f"{t}-{e}" for t, e in CASES])
def test_forward(lib, table, entry):
    """Every size of one (level table, entry point) against the float64 reference of that (table, size)."""
    sizes = R.sizes_for(table, entry)
    if R.BIG in sizes:
        n = hybrid_min_tiles()
        assert n == R.HYBRID_MIN_TILES and (R.BIG + 15) // 16 >= n > (max(R.SMALL_SIZES) + 15) // 16
    fails = L.run_case(lib, table, entry, "bf16x3", {})
    assert not fails, fails


def test_the_hybrid_size_runs_once_per_feed():
    big = [(t, e) for t, e in CASES if R.BIG in R.sizes_for(t, e)]
    assert big == [(R.BIG_TABLE, e) for e in ("fwd_rgb", "table", "records")]


def test_empty_launches_write_nothing(lib):
    """M == 0 (and an empty lattice): return code 0 with every array null but one poisoned output, which stays poisoned."""
    D = L.dev("levels5")
    out = nan_out(64)
    p, e, d, s = out.ptr, D.emb[0].ptr, D.desc, stream()
    rcs = [lib.inr_nerf_forward(None, None, 0, None, 1.0, e, d, None, 1.0, p, None, None, 0, s),
           lib.inr_nerf_forward_table(None, None, None, 0, 1.0, e, d, None, 1.0, p, None, 0, s),
           lib.inr_nerf_forward_table_records(None, None, None, 0, 1.0, e, d, None, 1.0, p, None, 0, s),
           lib.inr_nerf_forward_table_sliced(None, None, None, 0, 1.0, e, d, None, 1.0, p, None, None, s),
           lib.inr_nerf_forward_dirs(None, 0, 1.0, e, d, None, None, 3, p, s),
           lib.inr_nerf_forward_lattice(None, None, None, 19, 0, 5, 1.0, e, d, None, None, 3, 0.0, p, s),
           lib.inr_nerf_forward_train(None, None, 0, 1.0, e, d, None, p, None, None, None, None, None, None, None, s),
           lib.inr_nerf_forward_enc(None, None, 0, 1.0, e, d, None, p, None, None, s),
           lib.inr_instance_forward(None, 0, None, 1.0, e, d, None, 48, p, s),
           lib.inr_instance_forward_train(None, 0, 1.0, e, d, None, 48, p, None, None, None, s),
           lib.inr_instance_forward_enc(None, 0, None, 1.0, e, d, None, 48, p, None, s),
           lib.inr_ray_table_q(None, None, 0, p, s)]
    L._sync()
    assert rcs == [0] * len(rcs), rcs
    assert poisoned(out.get()).all()
    out.check_guards("empty launch")


@pytest.mark.parametrize("entry", ["fwd_rgb", "fwd_density", "instance48", "instance_enc32"])
@pytest.mark.parametrize("n", [None, "M-37", 0, "M+5"])
def test_device_side_sample_count(lib, entry, n):
    """n_samples_dev null, M - 37, 0 and above M: rows below min(n, M) against the reference, the rest keep their
    poison."""
    table, M = "bench", MID
    nd = {None: None, "M-37": M - 37, 0: 0, "M+5": M + 5}[n]
    got, sh = L.launch(lib, table, entry, M, n_dev=nd)
    rows = M if nd is None else min(nd, M)
    fails = L.compare(table, entry, M, got, sh, "bf16x3", {}, rows=rows)
    assert not fails, fails


def test_records_feed_refuses_a_bound_that_is_no_power_of_two(lib):
    got, _ = L.launch(lib, "levels5", "records", 33, bound=1.5, expect_rc=-1)       # INR_EINVAL
    assert all(poisoned(v).all() for v in got.values())


@pytest.mark.parametrize("table", ["dense_coarse", "hashed_all", "bench", "all_dense", "levels12", "levels5", "x16"])
def test_fp16_table_equals_the_fp32_launch_on_the_rounded_table(lib, table):
    """NUMERICS_TABLE_F16 on the fp16 copy == the fp32-table launch on the table rounded to fp16, bit for bit, at every
    size: the table feed with the bf16x3 MLP (numerics 1 against 0) and with the fp16 MLP (3 against 2), and the plain
    -O launch against the table feed with the fp16 MLP on the rounded table (one ray per sample, SH rows from
    inr_ray_table_q, the same x01: the same operations on the same values)."""
    bound = R.SETTINGS[table][0]
    for M in R.SMALL_SIZES:
        for half, full in ((1, 0), (3, 2)):
            a, _ = L.launch(lib, table, "table", M, numerics=half)
            b, _ = L.launch(lib, table, "table", M, numerics=full, emb_key="rounded")
            for k in a:
                assert np.isfinite(a[k]).all()
                assert_same_bits(a[k], b[k], f"{table} M{M} numerics {half} against {full} on the rounded table: {k}")
        sc = dict(R.scene(table, M, bound, R.grid_for(table, "fwd_o")))
        _, sh = L.ray_table(lib, sc["x"], sc["dirs"])
        sc.update(ray_ids=np.arange(M, dtype=np.int32), shrow=sh, x01=R.S.x01_div(sc["x"], bound))
        a, _ = L.launch(lib, table, "fwd_o", M, x=sc["x"], sc=sc)
        b, _ = L.launch(lib, table, "table", M, numerics=2, emb_key="rounded", sc=sc,
                        W=R.nerf_weights(table, R.variant_for(table, "fwd_o")))
        for k in a:
            assert_same_bits(a[k], b[k], f"{table} M{M} plain -O against the fp16-MLP table feed on the rounded table: {k}")


@pytest.mark.parametrize("entry", R.ROUNDING_ENTRIES)
@pytest.mark.parametrize("table", R.EXACT_TABLES)
def test_fp16_mlp_rounds_to_nearest_even(lib, table, entry):
    """The rounding tier: layer inputs that need their fp16 rounding, everything exact after it; sigma and rgb within
    ROUNDING_TOL (v_exp_f32 / v_rcp_f32 alone) of the HalfMlp model, which rounds to nearest even."""
    for M in (33, MID):
        want, ref = R.rounding_reference(table, entry, M)
        got, _ = L.launch(lib, table, entry, M, sc=ref.sc, W=ref.W)
        for k in want:
            err = np.abs(got[k].astype(np.float64) - want[k]) / np.abs(want[k])
            print(f"{table}/{entry}/M{M}.{k}: worst |got - model| / model {err.max():.3e}  (ROUNDING_TOL {R.ROUNDING_TOL:.3e})")
            assert np.isfinite(got[k]).all() and err.max() <= R.ROUNDING_TOL, (table, entry, M, k, err.max())


DEAD_ENTRIES = ("fwd_rgb", "fwd_density", "fwd_o", "table", "table_t16", "table_m16", "table_o", "records", "train", "enc",
                "dirs3", "instance16", "instance_train48", "instance_enc64")


@pytest.mark.parametrize("table", ["levels12", "levels5", "x12"])
def test_dead_levels_read_row_0_against_zero_columns(lib, table):
    """12- and 5-level tables: the slots of levels that do not exist gather row 0 of the table; with the weight columns
    of those features zero (host packers plain and fp16, device packers), row 0 = 0, +1e4 or -1e4 changes no output
    bit, in every numerics mode.  Row 0 is also the corner (0,0,0) of level 0: samples in that cell are left out."""
    M = MID
    emb = R.embeddings(table)
    t = R.table_for(table)
    assert not R.nerf_weights(table)[0][:, 2 * t["num_levels"]:].any()
    devs = []
    for v in (0.0, 1e4, -1e4):
        e = emb.copy()
        e[0] = v
        devs.append(L.Dev(table, e))
    for entry in DEAD_ENTRIES:
        sc = R.scene(table, M, R.SETTINGS[table][0], R.grid_for(table, entry))
        cell, _ = R.cells(R.x01_plain(R.plain_x(sc, sc["bound"]), sc["bound"])[0], t)
        cell2, _ = R.cells(sc["x01"], t)
        keep = cell[:, 0].any(1) & cell2[:, 0].any(1)
        assert keep.sum() > 0.9 * M
        outs = []
        for D in devs:
            outs.append(L.launch(lib, table, entry, M, D=D)[0])
        for k in outs[0]:
            cols = slice(0, 2 * t["num_levels"]) if k in ("enc", "ienc") else slice(None)      # the saved dead features ARE row 0
            assert np.isfinite(outs[0][k][keep]).all()
            for o in outs[1:]:
                assert_same_bits(o[k][keep][..., cols], outs[0][k][keep][..., cols],
                                 f"{table}/{entry}.{k}: row 0 reaches the output")


def test_fp32_library_both_tiers():
    """The -DINR_MLP_FP32=1 library (a process binds one library: a child with INR_LIB_PATH) runs the same exact tier
    and its own tolerance tier (every entry point its build has, every size below the hybrid one)."""
    from instance_nerf_amd import build
    assert os.path.exists(build.LIB_FP32), "libinr_hip_fp32.so is built by __graft_entry__.build()"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "field_forward_child.py")
    res = run_result_child(child, dict(INR_LIB_PATH=build.LIB_FP32, FIELD_FORWARD_BUILD="fp32"), timeout=600)
    print("fp32 library, worst |got - ref| / cond:", res["ratios"])
    assert res["build"] == "fp32" and set(res["ratios"]) == set(R.TOL["fp32"])
    assert not res["failures"], res["failures"][:10]
