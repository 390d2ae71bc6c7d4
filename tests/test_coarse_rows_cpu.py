"""The host gate of the pair front end's dense x-pair form, without a GPU: gridencoder.dense_x_pairs restates
dense_x_pairs_qualify of csrc/field_fused.hip (tests/test_coarse_rows.py holds the library's own choice against it on
the GPU) - which descriptors take the 16-byte loads - and that the second row of a pair stays inside its level."""
from instance_nerf_amd.gridencoder import dense_x_pairs, level_table


def test_bench_descriptor_takes_the_dense_form():
    t = level_table()                                   # the bench table: base 16, 2^19 rows per hashed level
    assert [int(h) for h in t["hashed"]] == [0] * 5 + [1] * 11
    assert dense_x_pairs(t) and dense_x_pairs(t, "1") and dense_x_pairs(t, 3)
    assert not dense_x_pairs(t, "0") and not dense_x_pairs(t, 0)


def test_descriptors_that_keep_the_gathers():
    assert not dense_x_pairs(level_table(log2_hashmap_size=12))                   # 2^12 rows per level: level 0 hashed
    t3 = level_table(log2_hashmap_size=16)
    assert [int(h) for h in t3["hashed"][:4]] == [0, 0, 0, 1] and not dense_x_pairs(t3)
    t4 = level_table(log2_hashmap_size=17)
    assert [int(h) for h in t4["hashed"][:5]] == [0, 0, 0, 0, 1] and dense_x_pairs(t4)    # level 4 is not in slots 0, 1
    assert not dense_x_pairs(level_table(num_levels=3, desired_resolution=64))   # fewer than four levels


def test_a_dense_level_keeps_its_neighbour_row_inside():
    """row + 1 of the last cell: the dense index of corner (res, res, res) is the level's last used row, so the 16-byte
    load of (row, row + 1) at x01 = 1 ends inside the level for every dense level of the bench table."""
    t = level_table()
    for l in range(4):
        r1 = int(t["resolutions"][l]) + 1
        rows = int(t["offsets"][l + 1]) - int(t["offsets"][l])
        cell = int(float(t["scales"][l]) + 0.5)                      # trunc(1.0 * scale + 0.5)
        last = (cell + 1) + cell * r1 + cell * r1 * r1 + r1 + r1 * r1   # corner (cx + 1, cy + 1, cz + 1)
        assert last < r1 ** 3 <= rows, (l, last, rows)
