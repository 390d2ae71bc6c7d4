"""Bit identity of the fused field kernels (csrc/field_fused.hip) against tests/golden/field_issue_path.npz, which
tests/golden/make_field_issue_golden.py recorded on the GPU from the build BEFORE the issue path of a tile was
shortened (sigmoid epilogue on the lanes q < 3, one dense/hashed select per coarse level).  Those changes are the same
operations on the same values, so the assertion is equality of bits, not closeness.

Cases (tests/field_issue_cases.py): sample counts 1, 15, 16, 17 and 16*61+7; level tables with every coarse level dense,
every coarse level hashed, dense and hashed lanes mixed in one coarse slot (the benchmark's table), every level dense
(generic fine instantiation) and fewer than 16 levels (dead records in the fine and in the coarse slots); k_nerf_fwd
with and without colour, plain / table / sliced feed, kHalf, kFast, kSave 1 and 2, k_instance_fwd for K = 16 and 64,
k_nerf_fwd_dirs, and k_nerf_render / k_instance_render over three 16-ray groups.  Inputs include positions on cell
boundaries and volume faces, one position outside the volume, and colour pre-activations that are negative and exactly 0.

Checked by hand that it notices a mistake: a build whose epilogue exchanges the red and green channels fails every
test_field_kernels_bit_identical case (first: dense_coarse/fwd_rgb/1/rgb, 2 of 3 words differ).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_issue_cases as cases  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_issue_path.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _compare(golden, key, rec):
    names = [k[len(key) + 1:] for k in golden if k.startswith(key + "/")]
    assert sorted(names) == sorted(rec), f"{key}: fixture holds {sorted(names)}, the launch gave {sorted(rec)}"
    for name, got in rec.items():
        want = golden[f"{key}/{name}"]
        if name.endswith(".sha256"):
            assert str(got) == str(want), f"{key}/{name}: bits differ"
            continue
        assert got.dtype == np.uint32 and got.shape == want.shape, f"{key}/{name}: shape {got.shape} vs {want.shape}"
        bad = np.flatnonzero(got.ravel() != want.ravel())
        assert bad.size == 0, (f"{key}/{name}: {bad.size} of {got.size} words differ, first at {int(bad[0])}: "
                               f"{int(got.ravel()[bad[0]]):#010x} vs {int(want.ravel()[bad[0]]):#010x}")


def test_level_tables_cover_every_class_of_coarse_slot():
    hashed = {n: [int(h) for h in cases.table_for(n)["hashed"]] for n in cases.TABLES}
    assert hashed["dense_coarse"] == [0] * 8 + [1] * 8
    assert hashed["hashed_all"] == [1] * 16
    assert hashed["all_dense"] == [0] * 16
    b = hashed["bench"]
    assert len(b) == 16 and all(b[8:])
    for slot in (0, 1):                                   # slot li of lane q is level 2q + li
        lanes = [b[2 * q + slot] for q in range(4)]
        assert 0 in lanes and 1 in lanes, "the benchmark's table mixes dense and hashed lanes in both coarse slots"
    assert len(hashed["levels12"]) == 12 and len(hashed["levels5"]) == 5


def test_fixture_is_complete(golden):
    keys = {k.rsplit("/", 1)[0] for k in golden if "/" in k}
    assert keys == {k for k, _ in cases.all_cases()}
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("table", list(cases.TABLES))
def test_field_kernels_bit_identical(golden, table):
    for kernel in cases.KERNELS:
        if not cases.applies(table, kernel):
            continue
        for M in cases.sizes_for(kernel):
            _compare(golden, f"{table}/{kernel}/{M}", cases.record(cases.run(table, kernel, M), kernel, M))


@pytest.mark.gpu
@pytest.mark.parametrize("table", cases.RENDER_TABLES)
def test_render_kernels_bit_identical(golden, table):
    for kernel in cases.RENDER_KERNELS:
        _compare(golden, f"{table}/{kernel}", cases.record(cases.run_render(table, kernel), kernel, 0))


def test_zero_and_negative_colour_preactivations_are_covered(golden):
    """The all-zero green row gives a pre-activation of exactly 0 (sigmoid 0.5); the red row is mostly negative."""
    rgb = golden[f"bench/table_zero_g/{cases.BIG}/rgb"].view(np.float32)
    assert np.all(rgb[:, 1] == np.float32(0.5))
    assert np.mean(rgb[:, 0] < 0.5) > 0.5 and np.any(rgb[:, 2] > 0.5) and np.any(rgb[:, 2] < 0.5)
