"""The detector's training targets without a GPU: the numpy restatement (tests/box_targets_reference.py) and the
composable path of instance_nerf_amd/targets.py against the reference's own run (tests/golden/box_targets.npz) bit for
bit, the Matcher on hand-written matrices, the coder's round trip, the sampler's counts and frequencies, and the argument
validation of the two exports (tests/box_targets_abi_child.py)."""
import hashlib
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe  # noqa: E402
import box_targets_cases as bc  # noqa: E402
import box_targets_reference as br  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NAN = float("nan")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "box_targets.npz"))


def T(x):
    return None if x is None else torch.from_numpy(x)


# ---------------------------------------------------------------------------- against the reference's own run
@pytest.mark.parametrize("name", sorted(bc.fixture_cases()))
def test_restatement_and_composable_path_equal_the_reference(golden, name):
    from instance_nerf_amd import targets
    case, with_targets = bc.fixture_cases()[name]
    want_m = golden[f"{name}_matched"].astype(np.int64)
    want_l = golden[f"{name}_labels"].astype(np.int64)
    mine = br.assign(**case)
    assert np.array_equal(mine["matched"], want_m) and np.array_equal(mine["labels"], want_l)
    assert br.same(mine["matched_boxes"], golden[f"{name}_boxes"])
    got = targets.match_boxes(T(case["gt"]), T(case["boxes"]), case["high"], case["low"], case["allow"], valid=T(case["valid"]))
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want_m)
    if case["gt_labels"] is None and case["allow"]:
        labels, boxes, reg = targets.assign_targets_to_anchors(
            [T(case["boxes"])], [T(case["gt"])], case["high"], case["low"],
            padding_masks=None if case["valid"] is None else [T(case["valid"])], encode=True)
        assert labels[0].dtype == torch.float32 and np.array_equal(labels[0].numpy(), want_l.astype(np.float32))
        assert br.same(boxes[0].numpy(), golden[f"{name}_boxes"])
        enc = reg[0].numpy()
    elif case["gt_labels"] is not None:
        idx, labels = targets.assign_targets_to_proposals([T(case["boxes"])], [T(case["gt"])], [T(case["gt_labels"])],
                                                          case["high"], case["low"])
        assert idx[0].dtype == labels[0].dtype == torch.int64
        assert np.array_equal(idx[0].numpy(), np.maximum(want_m, 0)) and np.array_equal(labels[0].numpy(), want_l)
        enc = targets.encode_boxes(T(case["gt"])[idx[0]], T(case["boxes"])).numpy()
    else:
        enc = targets.encode_boxes(T(golden[f"{name}_boxes"]), T(case["boxes"])).numpy()
    assert br.same(enc, mine["targets"])
    if with_targets:
        assert br.same(enc, golden[f"{name}_targets"])


def test_full_size_counts_and_hash(golden):
    """The shipped pyramid: 950 625 anchors against 24 GT boxes through the composable path."""
    from instance_nerf_amd import targets
    anchors = bc.full_size_anchors()
    assert anchors.shape == (950625, 6)
    m = targets.match_boxes(T(bc.full_size_gt()), T(anchors), 0.35, 0.2, True, fused=False).numpy()
    counts = [int((m >= 0).sum()), int((m == -2).sum()), int((m == -1).sum())]
    assert counts == golden["full_counts"].tolist() and sum(counts) == 950625 and counts[0] > 0 and counts[1] > 0
    assert hashlib.sha256(m.astype(np.int64).tobytes()).digest() == golden["full_sha256"].tobytes()


def test_special_cases_composable_equals_restatement():
    from instance_nerf_amd import targets
    for name, case in bc.special_cases().items():
        mine = br.assign(**case)
        got = targets.match_boxes(T(case["gt"]), T(case["boxes"]), case["high"], case["low"], case["allow"], valid=T(case["valid"]))
        assert np.array_equal(got.numpy(), mine["matched"]), name
    cw = br.assign(**bc.special_cases()["cross_workgroup"])["matched"]
    assert np.flatnonzero(cw >= 0).tolist() == [5, bc.RUN - 1, 2 * bc.RUN] and cw[5] == 1 and cw[bc.RUN - 1] == 0
    th = br.assign(**bc.special_cases()["thresholds_rpn_strict"])["matched"]
    assert th.tolist() == [0, -2, -2, -1, -2, -2]                # 7/20 >= 0.35f; 1/5 >= 0.2f; 1/4 lies between
    assert br.assign(**bc.special_cases()["thresholds_head"])["matched"].tolist() == [0, 0, -1, -1, 2, -1]


# ---------------------------------------------------------------------------- the Matcher on hand-written matrices
def match(rows, high, low, allow=False):
    from instance_nerf_amd import targets
    q = torch.tensor(rows, dtype=torch.float32)
    keep = q.clone()
    out = targets.Matcher(high, low, allow)(q)
    assert out.dtype == torch.int64 and torch.equal(torch.nan_to_num(q, 7.0), torch.nan_to_num(keep, 7.0))
    want, _ = br.matcher(q.numpy(), high, low, allow)
    assert np.array_equal(out.numpy(), want)
    return out.tolist()


def test_matcher_ties_go_to_the_lower_index():
    assert match([[0.5, 0.1, 0.9], [0.5, 0.9, 0.9], [0.2, 0.9, 0.1]], 0.35, 0.2) == [0, 1, 0]


def test_matcher_at_both_thresholds():
    seven_twentieths = float(np.float32(7) / np.float32(20))
    fifth = float(np.float32(1) / np.float32(5))
    below = float(np.nextafter(np.float32(fifth), np.float32(0)))
    under = float(np.nextafter(np.float32(seven_twentieths), np.float32(0)))
    assert match([[seven_twentieths, under, fifth, below, 0.0]], 0.35, 0.2) == [0, -2, -2, -1, -1]


def test_matcher_with_equal_thresholds_has_no_between():
    out = match([[0.25, 0.2499, 0.3, 0.0], [0.1, 0.1, 0.1, 0.1]], 0.25, 0.25)
    assert out == [0, -1, 0, -1]


def test_matcher_row_maximum_zero_restores_every_zero_column():
    # GT 1 overlaps nothing: its maximum 0 is attained by every column, and each gets its arg-max back
    assert match([[0.9, 0.1, 0.0], [0.0, 0.0, 0.0]], 0.35, 0.2, allow=False) == [0, -1, -1]
    assert match([[0.9, 0.1, 0.0], [0.0, 0.0, 0.0]], 0.35, 0.2, allow=True) == [0, 0, 0]
    # without that row only the low-quality best of GT 1 comes back
    assert match([[0.9, 0.1, 0.0], [0.3, 0.15, 0.0]], 0.35, 0.2, allow=True) == [0, -1, -1]
    assert match([[0.9, 0.1, 0.0], [0.1, 0.15, 0.0]], 0.35, 0.2, allow=True) == [0, 1, -1]


def test_matcher_with_every_column_masked():
    assert match([[-1.0, -1.0], [-1.0, -1.0]], 0.35, 0.2) == [-1, -1]
    assert match([[-1.0, -1.0], [-1.0, -1.0]], 0.35, 0.2, allow=True) == [0, 0]      # the row maxima are -1: restored


def test_matcher_nan_column_and_nan_row():
    # a NaN is the column's maximum (its first NaN wins) and passes both threshold tests; it never equals a row maximum
    assert match([[0.1, 0.9], [NAN, 0.1], [NAN, 0.2]], 0.35, 0.2) == [1, 0]
    assert match([[NAN, NAN, NAN], [0.1, 0.3, 0.9]], 0.35, 0.2, allow=True) == [0, 0, 0]
    assert match([[0.1, NAN, 0.3], [0.25, 0.1, 0.1]], 0.35, 0.2, allow=True) == [1, 0, -2]


def test_matcher_refuses_empty_matrices():
    from instance_nerf_amd import targets
    m = targets.Matcher(0.35, 0.2)
    with pytest.raises(ValueError, match="No ground-truth"):
        m(torch.zeros(0, 5))
    with pytest.raises(ValueError, match="No proposal"):
        m(torch.zeros(3, 0))
    with pytest.raises(ValueError, match="No ground-truth"):
        targets.match_boxes(torch.zeros(0, 6), torch.zeros(4, 6), 0.35, 0.2)
    with pytest.raises(ValueError, match="No proposal"):
        targets.match_boxes(torch.zeros(3, 6), torch.zeros(0, 6), 0.35, 0.2)
    with pytest.raises(ValueError, match="low_threshold"):
        targets.Matcher(0.2, 0.35)
    with pytest.raises(ValueError, match="oriented"):
        targets.match_boxes(torch.zeros(3, 7), torch.zeros(4, 7), 0.35, 0.2)
    with pytest.raises(RuntimeError, match="fused"):
        targets.match_boxes(torch.zeros(3, 6), torch.ones(4, 6), 0.35, 0.2, fused=True)


def test_empty_ground_truth_gives_zeros():
    from instance_nerf_amd import targets
    a = T(bc.scene(3, 10, 2)[1])
    valid = torch.arange(10) < 8
    labels, boxes = targets.assign_targets_to_anchors([a], [torch.zeros(0, 6)], 0.35, 0.2, padding_masks=[valid])
    assert labels[0].tolist() == [0.0] * 8 + [-1.0] * 2 and torch.equal(boxes[0], torch.zeros(10, 6))
    idx, lab = targets.assign_targets_to_proposals([a], [torch.zeros(0, 6)], [torch.zeros(0, dtype=torch.int64)], 0.25, 0.25)
    assert idx[0].dtype == lab[0].dtype == torch.int64 and not idx[0].any() and not lab[0].any()


def test_other_float_types_take_the_composable_path():
    from instance_nerf_amd import targets
    gt, boxes = bc.scene(5, 50, 3)
    m32 = targets.match_boxes(T(gt), T(boxes), 0.35, 0.2, True)
    m64 = targets.match_boxes(T(gt).double(), T(boxes).double(), 0.35, 0.2, True)
    assert m64.dtype == torch.int64 and (m32 == m64).float().mean() > 0.9


# ---------------------------------------------------------------------------- the coder
def test_encode_then_decode_round_trip():
    from instance_nerf_amd import targets
    gt, boxes = bc.scene(21, 300, 300)
    enc = targets.encode_boxes(T(gt), T(boxes))
    assert enc.shape == (300, 6) and enc.dtype == torch.float32
    back = targets.decode_boxes(enc, T(boxes))
    # ratios of sides are at most 15 / 3 and offsets at most a few sides: a handful of fp32 roundings of values below 64
    assert float((back - T(gt)).abs().max()) <= 64 * 16 * 2.0 ** -24
    wide = targets.decode_boxes(torch.cat([enc, enc], 1), T(boxes))
    assert wide.shape == (300, 12) and torch.equal(wide[:, :6], back) and torch.equal(wide[:, 6:], back)
    # the clip: a size code above log(2000) decodes as 2000 sides
    code = torch.tensor([[0.0, 0.0, 0.0, 50.0, 0.0, 0.0]])
    box = targets.decode_boxes(code, torch.tensor([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0]]))
    assert abs(float(box[0, 3] - box[0, 0]) - 2000.0) < 1e-2 and abs(float(box[0, 4] - box[0, 1]) - 1.0) < 1e-6
    assert targets.decode_boxes.__defaults__ == (math.log(2000.0),)


# ---------------------------------------------------------------------------- the sampler
def check_sample(labels, batch, fraction, seed=0):
    from instance_nerf_amd import targets
    gen = torch.Generator().manual_seed(seed)
    pos, neg = targets.sample_balanced(labels, batch, fraction, generator=gen)
    assert pos.dtype == neg.dtype == torch.uint8 and pos.shape == neg.shape == labels.shape
    assert not bool((pos.bool() & ~(labels >= 1)).any()) and not bool((neg.bool() & ~(labels == 0)).any())
    P, N = int((labels >= 1).sum()), int((labels == 0).sum())
    num_pos = min(P, int(batch * fraction))
    assert int(pos.sum()) == num_pos and int(neg.sum()) == min(N, batch - num_pos)
    again = targets.sample_balanced(labels, batch, fraction, generator=torch.Generator().manual_seed(seed))
    assert torch.equal(again[0], pos) and torch.equal(again[1], neg)
    return pos, neg


def test_sampler_counts_and_subsets():
    labels = torch.tensor(([1.0] * 40 + [0.0] * 500 + [-1.0] * 60) * 2)
    labels = labels[torch.randperm(len(labels), generator=torch.Generator().manual_seed(1))]
    check_sample(labels, 256, 0.5)                            # too few positives: 80 + 176
    check_sample(labels, 64, 0.5)                             # enough of both: 32 + 32
    check_sample(labels, 64, 0.0)                             # no positives wanted
    check_sample(labels, 64, 1.0)                             # no negatives wanted
    check_sample(labels.long() * 3, 100, 0.25)                # the head's int64 labels, classes > 1
    few_neg = torch.tensor([2.0] * 300 + [0.0] * 7 + [-1.0] * 5)
    check_sample(few_neg, 256, 0.5)                           # too few negatives: 128 + 7
    check_sample(torch.tensor([1.0, 0.0, -1.0]), 256, 0.5)    # fewer elements than the batch
    check_sample(torch.full((50,), -1.0), 16, 0.5)            # nothing to draw from
    check_sample(torch.zeros(0), 16, 0.5)
    a, _ = check_sample(labels, 64, 0.5, seed=3)
    b, _ = check_sample(labels, 64, 0.5, seed=4)
    assert not torch.equal(a, b)


def test_sampler_draws_uniformly():
    """20 positives, 5 drawn, and 30 negatives, 11 drawn (batch 16), 2000 draws from one seeded generator: an element's
    count is Binomial(2000, p) with p = 1/4 and 11/30; the bound is 6 sigma = 6 sqrt(2000 p (1 - p)) = 116.2 and 129.3."""
    from instance_nerf_amd import targets
    labels = torch.tensor([1.0] * 20 + [0.0] * 30 + [-1.0] * 10)
    gen = torch.Generator().manual_seed(2024)
    draws = 2000
    pos_hits, neg_hits = torch.zeros(60), torch.zeros(60)
    for _ in range(draws):
        p, n = targets.sample_balanced(labels, 16, 5 / 16, generator=gen)
        pos_hits += p
        neg_hits += n
    for hits, lo, hi, prob in ((pos_hits, 0, 20, 5 / 20), (neg_hits, 20, 50, 11 / 30)):
        bound = 6 * math.sqrt(draws * prob * (1 - prob))
        assert float((hits[lo:hi] - draws * prob).abs().max()) <= bound, (hits[lo:hi], bound)
        assert float(hits.sum()) == float(hits[lo:hi].sum()) == round(draws * prob * (hi - lo))


# ---------------------------------------------------------------------------- ABI
def test_abi_facts():
    from instance_nerf_amd import _lib, build, targets
    header = open(os.path.join(ROOT, "include", "inr.h")).read()
    assert "inr_box_match_gt_max" in _lib.EXPORTS and "inr_box_match_assign" in _lib.EXPORTS
    assert "assign.hip" in build.SOURCES and "box_iou.h" in build.HEADERS and build.KERNEL_FILES["assign"][0] == "assign.hip"
    assert _lib.ABI_VERSION == 13 and "#define INR_ABI_VERSION 13" in header
    for py, c in ((_lib.BOX_MATCH_MAX_GT, "INR_BOX_MATCH_MAX_GT"), (_lib.BOX_MATCH_BLOCK, "INR_BOX_MATCH_BLOCK"),
                  (_lib.BOX_MATCH_BOXES_PER_WG, "INR_BOX_MATCH_BOXES_PER_WG")):
        assert py == int(re.search(rf"#define {c} (\d+)", header).group(1))
    assert targets.BOX_MATCH_MAX_GT == 1024 and bc.RUN == _lib.BOX_MATCH_BOXES_PER_WG
    # the headers the committed field profiles hash are not the new kernels' business
    assert "box_iou.h" not in build.KERNEL_FILES["field"] and "assign.hip" not in build.KERNEL_FILES["field"]


def test_float_keys_preserve_the_order():
    vals = np.asarray([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 0.2, 1.0, 3.0e38, np.inf, NAN], np.float32)
    keys = br.float_key(vals).astype(np.int64)
    assert (np.diff(keys) > 0).all() and keys[0] > 0 and keys[-1] == 0xFFFFFFFF
    assert br.float_key(np.float32(-NAN)) == 0xFFFFFFFF


@pytest.fixture(scope="module")
def abi():
    return abi_probe.run_abi_child("box_targets_abi_child.py")


@pytest.mark.parametrize("name", ["inr_box_match_gt_max", "inr_box_match_assign"])
def test_bad_arguments_are_einval_with_a_message_that_names_them(abi, name):
    cases = {"gt_null": "null", "boxes_null": "null", "gt_max_keys_null": "null", "G_0": "G", "G_1025": "G",
             "G_negative": "G", "A_negative": "A", "A_overflow": "2^31", "A_huge": "2^31", "gt_misaligned": "misaligned",
             "A_0_G_0": "G"}
    if name.endswith("assign"):
        cases.update(matched_null="null", low_above_high="low", low_nan="low", A_0_low_above_high="low")
    for case, needle in cases.items():
        rc, msg = abi[f"{name}:{case}"]
        assert rc == EINVAL and needle in msg and name in msg, (name, case, rc, msg)


@pytest.mark.parametrize("name", ["inr_box_match_gt_max", "inr_box_match_assign"])
def test_no_boxes_is_a_no_op(abi, name):
    for case in ("A_0", "A_0_null_pointers"):
        assert abi[f"{name}:{case}"][0] == 0, (name, case, abi[f"{name}:{case}"])
