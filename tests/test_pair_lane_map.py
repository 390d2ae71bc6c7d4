"""The lane map of the pair front end (k_nerf_fwd_pair in csrc/field_fused.hip) as a pure index computation: every
(sample, level, corner) of a pair of tiles is fetched exactly once, the two x sides of a fine level meet in the right
order, and after the hand-over swaps every register holds the feature the MLP layout expects.  No GPU, no library.

Encoder layout: lane = 32 h + 16 s + j (tile h of the pair, sample j, s in {0, 1}).
MLP layout of a tile: lane = 16 q + j; lane q holds levels {2q, 2q+1} in enc[0] and {8+2q, 9+2q} in enc[1], register
2 * (level & 1) + feature."""
import itertools

LANES = range(64)


def hsj(lane):
    return lane >> 5, (lane >> 4) & 1, lane & 15


def coarse_level(s, c):
    """slot c of lane s: levels {0,1,4,5} (s = 0) or {2,3,6,7} (s = 1)"""
    return 4 * (c >> 1) + 2 * s + (c & 1)


def gathers(lane):
    """(tile, sample, level, corner) of the 64 gathers of a lane, in issue order; corner = x | y << 1 | z << 2"""
    h, s, j = hsj(lane)
    out = [(h, j, coarse_level(s, c), k) for c in range(4) for k in range(8)]
    out += [(h, j, 8 + i, s | (yz << 1)) for i in range(8) for yz in range(4)]
    return out


def permlane16_swap(vdst, src):
    """v_permlane16_swap: the odd 16-lane rows of vdst trade places with the even rows of src -> (vdst, src)"""
    vdst, src = list(vdst), list(src)
    for lane in LANES:
        if (lane >> 4) & 1:
            vdst[lane], src[lane - 16] = src[lane - 16], vdst[lane]
    return vdst, src


def permlane32_swap(vdst, src):
    """v_permlane32_swap: lanes 32..63 of vdst trade places with lanes 0..31 of src -> (vdst, src)"""
    vdst, src = list(vdst), list(src)
    for lane in range(32, 64):
        vdst[lane], src[lane - 32] = src[lane - 32], vdst[lane]
    return vdst, src


def encode():
    """-> p, r: [e][c][lane] symbolic registers after blend_coarse_pair / blend_fine_pair.  A coarse feature is
    ("f", tile, sample, level, feature); a fine one ("sum", side-0 partial, side-1 partial) in the order of the add."""
    p = [[[None] * 64 for _ in range(4)] for _ in range(2)]
    r = [[[None] * 64 for _ in range(4)] for _ in range(2)]
    for lane in LANES:
        h, s, j = hsj(lane)
        for c in range(4):
            for ft in range(2):
                (r if c >> 1 else p)[0][2 * (c & 1) + ft][lane] = ("f", h, j, coarse_level(s, c), ft)
    part = [[[("part", *hsj(lane)[::2], 8 + i, ft, hsj(lane)[1]) for lane in LANES] for ft in range(2)] for i in range(8)]
    for k in range(4):
        i0 = (k >> 1) * 4 + (k & 1)
        for ft in range(2):
            v0, v1 = permlane16_swap(part[i0][ft], part[i0 + 2][ft])
            (r if k >> 1 else p)[1][2 * (k & 1) + ft] = [("sum", a, b) for a, b in zip(v0, v1)]
    return p, r


def test_every_sample_level_corner_is_fetched_exactly_once():
    seen = {}
    for lane in LANES:
        g = gathers(lane)
        assert len(g) == 64
        for x in g:
            seen[x] = seen.get(x, 0) + 1
    want = set(itertools.product(range(2), range(16), range(16), range(8)))
    assert set(seen) == want and set(seen.values()) == {1}


def test_an_instruction_covers_32_samples_of_two_coarse_levels_or_both_x_sides_of_a_fine_one():
    for n in range(64):
        rows = [gathers(lane)[n] for lane in LANES]
        assert {(h, j) for h, j, _, _ in rows} == set(itertools.product(range(2), range(16)))
        levels, corners = {l for _, _, l, _ in rows}, {k for _, _, _, k in rows}
        if n < 32:                      # coarse: two levels, one corner
            assert len(levels) == 2 and len(corners) == 1 and max(levels) < 8
        else:                           # fine: one level, both x sides of one yz corner
            assert len(levels) == 1 and min(levels) >= 8 and len(corners) == 2
            a, b = sorted(corners)
            assert b == a + 1 and a % 2 == 0


def test_fine_sides_meet_as_side0_plus_side1_in_the_owner_lanes():
    p, r = encode()
    for lane in LANES:
        h, s, j = hsj(lane)
        for regs, base in ((p, 8), (r, 12)):
            for c in range(4):
                level, ft = base + 2 * s + (c >> 1), c & 1
                assert regs[1][c][lane] == ("sum", ("part", h, j, level, ft, 0), ("part", h, j, level, ft, 1))


def test_features_land_where_the_mlp_layout_expects_them():
    p, r = encode()
    enc_a = [[None] * 4 for _ in range(2)]
    enc_b = [[None] * 4 for _ in range(2)]
    for e in range(2):
        for c in range(4):
            enc_a[e][c], enc_b[e][c] = permlane32_swap(p[e][c], r[e][c])
    for tile, enc in ((0, enc_a), (1, enc_b)):
        for lane in LANES:
            q, j = lane >> 4, lane & 15
            for c in range(4):
                assert enc[0][c][lane] == ("f", tile, j, 2 * q + (c >> 1), c & 1)
                level, ft = 8 + 2 * q + (c >> 1), c & 1
                assert enc[1][c][lane] == ("sum", ("part", tile, j, level, ft, 0), ("part", tile, j, level, ft, 1))


def test_ray_ids_reach_the_mlp_lanes_of_both_tiles():
    rid = [("rid",) + hsj(lane)[::2] for lane in LANES]              # (tile, sample) of the encoder lane
    rid_a, rid_b = permlane32_swap(rid, rid)
    for lane in LANES:
        assert rid_a[lane] == ("rid", 0, lane & 15) and rid_b[lane] == ("rid", 1, lane & 15)
