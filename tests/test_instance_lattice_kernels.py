"""inr_instance_lattice and inr_instance_volume_stats on the GPU against tests/instance_lattice_reference.py, through the
C ABI with poisoned, guarded buffers (tests/instance_lattice_child.py).  Lattice: density logit, occupancy of every
voxel, labels (ties to the lowest channel) and max-softmax confidence on both tiers, K = 1 .. 64, lattices around the
16-voxel run, the >= at the threshold, logits that are all <= 0, the interleaved XCD split once, the exact-fp32 library
through a child.  Statistics: every output bit-equal to the restatement of the launch's summation order."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instance_lattice_child as C  # noqa: E402
import instance_lattice_reference as I  # noqa: E402
from kernel_harness import run_result_child  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = I.cases()


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", CASES, ids=[I.case_id(c) for c in CASES])
def test_lattice(lib, case):
    """The four thresholds of one (table, lattice, K): both quantiles (density_logit null at the second), 0 and above
    every sigma."""
    ratios = {}
    fails = C.run_case(lib, case, "bf16x3", ratios)
    print(I.case_id(case), "worst |got - ref| as a fraction of its tolerance:", ratios)
    assert not fails, fails


def test_the_skip_sees_empty_mixed_and_full_tiles_and_an_empty_padded_tail():
    """What test_lattice's 0.9-quantile launches of the tolerance tier run through, asserted on the reference."""
    kinds = {c: I.tile_kinds(c[1], I.reference(*c).occupied(I.reference(*c).threshold(0.9)[0]))
             for c in CASES if I.tier_of(c[0]) == "tol" and c[1] in I.MAIN_LATTICES}
    for c, k in kinds.items():
        assert k["empty"] >= 1 and k["mixed"] >= 1, (c, k)
        if c[1][0] % 16:
            assert k["tail_empty"] >= 1, (c, k)
    assert any(k["full"] >= 1 for k in kinds.values()), kinds


@pytest.mark.parametrize("table", I.EXACT_TABLES)
@pytest.mark.parametrize("pair", I.TIE_PAIRS, ids=[f"{a}-{b}" for a, b in I.TIE_PAIRS])
def test_ties_resolve_to_the_lowest_channel(lib, table, pair):
    """Rows a and b of W2 equal: wherever the pair is the maximum the label is a, bit-exact logits on both sides."""
    ref = I.reference(table, (48, 5, 7), I.TIE_K, w2=("tie",) + pair)
    a, b = pair
    mx = ref.logits.max(1)
    won = (ref.logits[:, a] == mx) & (ref.logits[:, b] == mx) & (ref.label == a)
    assert won.sum() >= 1
    lab, conf, logit = C.launch(lib, ref, 0.0)
    fails = I.compare(ref, 0.0, lab, conf, logit, "bf16x3")
    assert not fails, fails
    assert (lab[won] == a).all()


@pytest.mark.parametrize("table", I.EXACT_TABLES)
@pytest.mark.parametrize("K", [1, 5, 31])
def test_all_logits_nonpositive_no_padded_channel_wins(lib, table, K):
    ref = I.reference(table, (33, 2, 3), K, w2="neg")
    assert (ref.logits <= 0).all() and (ref.logits < 0).all(1).any()          # a padding channel's 0 would be the maximum
    for th in (0.0, ref.threshold(0.5)[0]):
        lab, conf, logit = C.launch(lib, ref, th)
        assert (lab[lab != I.LABEL_EMPTY] < K).all()
        fails = I.compare(ref, th, lab, conf, logit, "bf16x3")
        assert not fails, fails


@pytest.mark.parametrize("table", I.EXACT_TABLES)
def test_a_voxel_on_the_threshold_is_occupied(lib, table):
    """so0 == 0 on every voxel: sigma == density_scale; sigma_thresh = density_scale occupies all, the next float none."""
    ref = I.reference(table, (19, 3, 5), 16, variant=None)
    assert (ref.so0 == 0).all()
    ds = F32(ref.ds)
    lab, conf, logit = C.launch(lib, ref, ds)
    assert (logit.view(np.uint32) == 0).all() and (lab != I.LABEL_EMPTY).all()
    assert not I.compare(ref, ds, lab, conf, logit, "bf16x3")
    up = np.nextafter(ds, F32(np.inf))
    lab, conf, logit = C.launch(lib, ref, up)
    assert (lab == I.LABEL_EMPTY).all() and (conf.view(np.uint32) == 0).all()
    assert not I.compare(ref, up, lab, conf, logit, "bf16x3")


def test_an_empty_lattice_writes_nothing(lib):
    ref = I.reference("bench", (19, 3, 5), 16)
    C.launch(lib, ref, 0.0, dims=(19, 0, 5), expect_written=False)


def test_the_interleaved_split_writes_every_voxel_once(lib):
    """(19, 128, 129): 33024 tiles, a launch make_sched deals to the XCDs in interleaved chunks (four rounds of eight
    chunks and a tail of 256 tiles split into eighths), against the reference of all 313 k voxels."""
    table, dims, K = I.BIG_CASE
    n_tiles = (dims[0] + 15) // 16 * dims[1] * dims[2]
    assert I.interleaved_min_tiles() == I.HYBRID_MIN_TILES and n_tiles == 33024 and n_tiles >= 4 << 13 > I.SMALL_TILES
    ref = I.big_reference()
    th, mid, gap, _ = ref.tail_threshold()
    assert gap > ref.gap_need(mid)
    ratios, fails = {}, []
    for t in (F32(0.0), th):                 # every tile through the instance field; nearly every tile skipped
        lab, conf, logit = C.launch(lib, ref, t)
        fails += I.compare(ref, t, lab, conf, logit, "bf16x3", ratios)
    print("interleaved split, worst |got - ref| as a fraction of its tolerance:", ratios)
    assert not fails, fails


def test_fp32_library_both_tiers():
    """The -DINR_MLP_FP32=1 library through a child (a process binds one library): every lattice case of both tiers
    under TOL["fp32"], its own confidence tolerance included."""
    from instance_nerf_amd import build
    assert os.path.exists(build.LIB_FP32), "libinr_hip_fp32.so is built by __graft_entry__.build()"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "instance_lattice_child.py")
    res = run_result_child(child, dict(INR_LIB_PATH=build.LIB_FP32, FIELD_FORWARD_BUILD="fp32"), timeout=600)
    print("fp32 library, worst |got - ref| as a fraction of its tolerance:", res["ratios"])
    assert res["build"] == "fp32" and set(res["ratios"]) == {"logit", "conf", "conf_exact"}
    assert not res["failures"], res["failures"][:10]


# ---------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("name", I.STATS_CASES)
def test_volume_stats_equal_the_restatement_bit_for_bit(lib, name):
    lab, conf, K = I.stats_inputs(name)
    counts, boxes, sums = I.stats_reference(lab, conf, K)
    got = C.launch_stats(lib, lab, conf, K)
    again = C.launch_stats(lib, lab, conf, K)
    assert np.array_equal(got[0], counts) and np.array_equal(got[1], boxes), name
    assert np.array_equal(got[2].view(np.uint32), sums.view(np.uint32)), (name, got[2], sums)
    for x, y in zip(got, again):
        assert x.tobytes() == y.tobytes(), name
    if name == "empty":
        assert not counts.any() and (boxes == -1).all() and (got[2].view(np.uint32) == 0).all()
    if name == "corners":
        assert counts[3] == 2 and boxes[3].tolist() == [0, 0, 0] + [d - 1 for d in lab.shape]


def test_volume_stats_through_extract(lib):
    """extract.volume_stats on device tensors: int64 counts and boxes, fp32 sums, on the volume's device, the same bits."""
    import torch
    from instance_nerf_amd import extract
    lab, conf, K = I.stats_inputs("spread")
    counts, boxes, sums = I.stats_reference(lab, conf, K)
    c, b, s = extract.volume_stats(torch.from_numpy(lab).cuda(), torch.from_numpy(conf).cuda(), K)
    assert c.dtype == torch.int64 and b.dtype == torch.int64 and s.dtype == torch.float32
    assert c.is_cuda and b.is_cuda and s.is_cuda and tuple(b.shape) == (K, 6)
    assert np.array_equal(c.cpu().numpy(), counts) and np.array_equal(b.cpu().numpy(), boxes)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), sums.view(np.uint32))
