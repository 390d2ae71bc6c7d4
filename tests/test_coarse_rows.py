"""The dense x-pair form of the pair front end (k_nerf_fwd_pair<true>: the x-neighbour rows of the dense levels 0..3 in
one 16-byte load per yz corner) against the one-tile kernel (INR_FIELD_PAIR=0) through the C ABI, bit for bit on sigma
and rgb, with guarded, poisoned buffers.  INR_FIELD_COARSE=0 selects the 8-byte gathers at every launch; the library's
inr_debug_field_coarse_launches counts what each launch took, and gridencoder.dense_x_pairs restates the host gate
(tests/test_coarse_rows_cpu.py pins it without a GPU).

(A second form - level 0 read from a copy in the launch's LDS - was built, measured and left out
(profiles/r12_coarse_rows_bench.md); its staging and LDS-size cases went with it.  What they exercise in the kept kernel
stays: a table rewritten in place between launches, overlap placement on and off.)"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_forward_reference as R  # noqa: E402
from kernel_harness import Buf, check, finish, nan_out, stream  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
BOUND, DENSITY_SCALE = 1.0, 0.3
SIZES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 1000]
M_MAX = max(SIZES)
TABLES = {
    "bench": dict(base_resolution=16, desired_resolution=2048, log2_hashmap_size=19),      # levels 0..4 dense
    "level0_hashed": dict(base_resolution=16, desired_resolution=2048, log2_hashmap_size=12),   # 2^12 rows per level
    "level3_hashed": dict(base_resolution=16, desired_resolution=2048, log2_hashmap_size=16),   # levels 0..2 dense
}


class _Env:
    """Environment switches for the duration of a block (None = unset); the previous values afterwards."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, str(v))

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _cell(x01, scale):
    """(cell, position) of the kernel's own arithmetic: pos = fl(fl(x01 * scale) + 0.5), cell = trunc(pos)."""
    pos = (np.asarray(x01, F32) * F32(scale)).astype(F32) + F32(0.5)
    return pos.astype(np.int64), pos


def _x01_of(o):
    return ((np.clip(np.asarray(o, F32), -BOUND, BOUND) + F32(BOUND)) * F32(0.5 / BOUND)).astype(F32)


def _scene(table):
    """M_MAX samples, one ray each (t = 0 on the placed ones: the position is the origin, exactly):
       0..15 | 16..31  left | right of a level-0 cell boundary in x: the two tiles of pair 0 sit in different cells;
       32..47          x01 = 0 and x01 = 1 on each axis, and all three at once (the level's last cell and last rows);
       48..63          cells of level 1 whose first x-neighbour row is the LAST row of a 128-byte line of the table:
                       the 16-byte load straddles two lines;
       the rest        random origins, directions and t (clamped to the volume by the kernel)."""
    rng = np.random.default_rng(11)
    o = rng.uniform(-1.0, 1.0, (M_MAX, 3)).astype(F32)
    d = rng.normal(size=(M_MAX, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    t = rng.uniform(0.0, 0.7, M_MAX).astype(F32)
    s0, s1 = float(table["scales"][0]), float(table["scales"][1])
    r1 = int(table["resolutions"][1]) + 1
    edge = (7.5 / s0) * 2.0 - 1.0                       # x01 = 7.5 / scale: pos = 8.0, the boundary of cells 7 | 8
    o[0:16, 0], o[16:32, 0] = F32(edge - 1e-3), F32(edge + 1e-3)
    ext = [(-1, None, None), (1, None, None), (None, -1, None), (None, 1, None), (None, None, -1), (None, None, 1),
           (-1, -1, -1), (1, 1, 1), (1, -1, 1), (-1, 1, 1), (1, 1, -1), (-1, -1, 1), (1, -1, -1), (-1, 1, -1), (1, 1, 1), (-1, -1, -1)]
    for i, e in enumerate(ext):
        for a in range(3):
            if e[a] is not None:
                o[32 + i, a] = F32(e[a])
    # level 1: cells (cx, cy, cz) with (offsets[1] + cx + cy r1 + cz r1^2) % 16 == 15, position 0.3 into the cell
    found, off1 = [], int(table["offsets"][1])
    for cz in range(1, r1 - 1):
        for cy in range(1, r1 - 1):
            for cx in range(1, r1 - 2):
                if (off1 + cx + cy * r1 + cz * r1 * r1) % 16 == 15:
                    found.append((cx, cy, cz))
    found = [found[i] for i in rng.permutation(len(found))[:16]]
    for i, c in enumerate(found):
        o[48 + i] = [F32(((c[a] - 0.2) / s1) * 2.0 - 1.0) for a in range(3)]
    t[:64] = 0.0
    x01 = _x01_of(o)
    # the scene is what it claims to be, in the kernel's own arithmetic
    c0, _ = _cell(x01[:, 0], s0)
    assert (c0[0:16] == 7).all() and (c0[16:32] == 8).all()
    assert all((x01[32 + i, a] == (0.0 if e[a] < 0 else 1.0)) for i, e in enumerate(ext) for a in range(3) if e[a] is not None)
    c1 = np.stack([_cell(x01[48:64, a], s1)[0] for a in range(3)], 1)
    assert len(found) == 16 and ((off1 + c1[:, 0] + c1[:, 1] * r1 + c1[:, 2] * r1 * r1) % 16 == 15).all()
    return dict(o=o, d=d, t=t, ray_ids=np.arange(M_MAX, dtype=np.int32))


class _Case:
    """One table on the device with U(-1, 1) values, the weights, and the scene's ray rows."""

    def __init__(self, lib, name, emb_offset=0):
        from instance_nerf_amd import _lib
        self.lib, self.table = lib, R.level_table(**TABLES[name])
        self.desc = _lib.make_grid_desc(self.table)
        rng = np.random.default_rng(5)
        self.emb = Buf(rng.uniform(-1.0, 1.0, (self.table["total_rows"], 2)).astype(F32), offset=emb_offset)
        ws = [np.ascontiguousarray(w, F32) for w in R.nerf_weights("bench")]
        packed = np.full(lib.inr_nerf_packed_floats(), np.nan, F32)
        check(lib.inr_nerf_pack_weights(*[w.ctypes.data for w in ws], packed.ctypes.data, 0), "nerf pack")
        self.packed = Buf(packed)
        sc = _scene(self.table)
        ob, db, self.rows = Buf(sc["o"]), Buf(sc["d"]), nan_out(M_MAX, 24)
        check(lib.inr_ray_table_q(ob.ptr, db.ptr, M_MAX, self.rows.ptr, stream()), "ray_table_q")
        finish({"rows": self.rows}, "ray_table_q")
        self.t, self.ids = Buf(sc["t"]), Buf(sc["ray_ids"])
        self.counters = (ctypes.c_int64 * 2).in_dll(lib, "inr_debug_field_coarse_launches")

    def launch(self, M, pair=True, coarse=None):
        """-> (sigma [M], rgb [M,3], variant the launch took or None for the one-tile kernel); guards checked."""
        o = {"sigma": nan_out(M), "rgb": nan_out(M, 3)}
        before = list(self.counters)
        with _Env(INR_FIELD_PAIR=None if pair else 0, INR_FIELD_COARSE=coarse):
            check(self.lib.inr_nerf_forward_table_records(self.t.ptr, self.ids.ptr, self.rows.ptr, M, BOUND, self.emb.ptr,
                                                          self.desc, self.packed.ptr, DENSITY_SCALE, o["sigma"].ptr,
                                                          o["rgb"].ptr, 0, stream()), "nerf_forward_table_records")
        got = finish(o, "records")
        took = [v for v in range(2) if self.counters[v] != before[v]]
        assert len(took) == (1 if pair else 0) and sum(self.counters) - sum(before) == len(took)
        assert not np.isnan(got["sigma"]).any() and not np.isnan(got["rgb"]).any()
        return got["sigma"], got["rgb"], (took[0] if took else None)

    def check_against_tile_kernel(self, M, coarse, expect):
        ref = self.launch(M, pair=False)
        got = self.launch(M, coarse=coarse)
        assert got[2] == expect, (coarse, got[2], expect)
        assert np.array_equal(ref[0].view(np.int32), got[0].view(np.int32)), (M, coarse, "sigma")
        assert np.array_equal(ref[1].view(np.int32), got[1].view(np.int32)), (M, coarse, "rgb")
        assert float(np.abs(ref[0]).max()) > 0
        return got


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def bench(lib):
    return _Case(lib, "bench")


def _plan(case, switch=None):
    from instance_nerf_amd.gridencoder import dense_x_pairs
    return int(dense_x_pairs(case.table, switch))


@pytest.mark.parametrize("M", SIZES)
def test_both_forms_equal_the_tile_kernel(bench, M):
    """INR_FIELD_COARSE = 0, 1 and unset: the bench table's levels 0..3 are dense, so only the switch turns the form off."""
    for coarse, expect in ((0, 0), (1, 1), (None, 1)):
        assert _plan(bench, coarse) == expect
        bench.check_against_tile_kernel(M, coarse, expect)


def test_a_table_rewritten_in_place_is_followed(lib):
    """New values written into level 0 of the table in place: the next launch must read them."""
    case = _Case(lib, "bench")
    first = case.check_against_tile_kernel(M_MAX, None, 1)
    rows0 = int(case.table["offsets"][1])
    case.emb.t[:rows0] = case.emb.t[:rows0].flip(0) * 0.5 + 0.25
    second = case.check_against_tile_kernel(M_MAX, None, 1)
    changed = first[0].view(np.int32) != second[0].view(np.int32)
    assert changed.mean() > 0.9, changed.mean()            # level 0 enters every sample


def test_placement_on_and_off(bench, lib):
    """Overlap placement raises the launch's LDS request to 84 KB; the kernel is the same and so are the bits."""
    try:
        for on in (1, 0):
            check(lib.inr_set_overlap_placement(on), "set_overlap_placement")
            for coarse in (0, None):
                bench.check_against_tile_kernel(M_MAX, coarse, 0 if coarse == 0 else 1)
    finally:
        lib.inr_set_overlap_placement(0)


@pytest.mark.parametrize("name, emb_offset, expect", [("level0_hashed", 0, 0), ("level3_hashed", 0, 0), ("bench", 2, 1)])
def test_fallback_where_the_table_does_not_allow_it(lib, name, emb_offset, expect):
    """Level 0 hashed (2^12 rows per level) or level 3 hashed: the 8-byte gathers.  A bench table whose address is 8- but
    not 16-byte aligned keeps the 16-byte loads - they need the rows' own alignment only.  The launch says what it took."""
    case = _Case(lib, name, emb_offset)
    hashed = [int(h) for h in case.table["hashed"]]
    assert hashed[8:] == [1] * 8
    assert {"level0_hashed": hashed[0] == 1, "level3_hashed": hashed[:4] == [0, 0, 0, 1], "bench": hashed[:4] == [0] * 4}[name]
    assert case.emb.ptr % 16 == (8 if emb_offset else 0)
    assert _plan(case) == expect
    for M in (33, M_MAX):
        case.check_against_tile_kernel(M, None, expect)
        case.check_against_tile_kernel(M, 1, expect)
