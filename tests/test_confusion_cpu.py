"""The segmentation confusion matrix and its scores without a GPU: the composable path of metrics.segmentation_confusion
against the numpy restatement (tests/confusion_reference.py) integer for integer, the arg-max rule of the contract
against torch.argmax on CPU tensors, SegmentationMeter against MIoUMeter with ==, panoptic quality on hand-written
matrices, the argument validation of the two exports (tests/confusion_abi_child.py) and reduce() on a two-rank gloo
group.  Everything here is exact: integers, or float64 quotients of the same integers."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe  # noqa: E402
import confusion_reference as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NAN, INF = float("nan"), float("inf")


def ids_case(B, N, K, seed):
    """Truth and prediction mostly in range, with every out-of-range value of the contract sprinkled in."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, K, (B, N)).astype(np.int64)
    p = np.where(rng.random((B, N)) < 0.6, t, rng.integers(0, K, (B, N)))
    for arr, bad in ((t, [-1, -7, K, 2 ** 31 - 1]), (p, [-1, -5, K, K + 9, 2 ** 31 - 1])):
        where = rng.random((B, N)) < 0.2
        arr[where] = rng.choice(bad, int(where.sum()))
    return p, t


def equal_ints(got, want, what):
    counts, ignored = got
    assert counts.dtype == torch.int64 and ignored.dtype == torch.int64, what
    assert np.array_equal(counts.cpu().numpy(), want[0]), what + " counts"
    assert np.array_equal(ignored.cpu().numpy(), want[1]), what + " ignored"


# ---------------------------------------------------------------------------- the composable path
@pytest.mark.parametrize("K", [1, 2, 13, 64, 100])
def test_composable_ids_against_the_restatement(K):
    from instance_nerf_amd import metrics
    for B in (1, 3):
        for N in (1, 63, 64, 65, 1000):
            p, t = ids_case(B, N, K, seed=N + K)
            want = cr.confusion(p, t, K)
            assert int(want[0].sum() + want[1].sum()) == B * N
            assert np.array_equal(want[0].sum(2), np.stack([(t == k).sum(1) for k in range(K)], 1))   # rows = truth areas
            for dtype in (torch.int64, torch.int32):
                got = metrics.segmentation_confusion(torch.from_numpy(p).to(dtype), torch.from_numpy(t).to(dtype), K)
                equal_ints(got, want, f"K{K} B{B} N{N} {dtype}")


def test_small_integer_dtypes_and_shapes():
    from instance_nerf_amd import metrics
    rng = np.random.default_rng(5)
    t = rng.integers(-1, 7, (2, 5, 9)).astype(np.int8)
    p = rng.integers(0, 9, (2, 5, 9)).astype(np.uint8)
    want = cr.confusion(p.reshape(2, -1), t.reshape(2, -1), 7)
    equal_ints(metrics.segmentation_confusion(torch.from_numpy(p), torch.from_numpy(t), 7), want, "int8 / uint8 [B, H, W]")
    flat = cr.confusion(p.reshape(1, -1), t.reshape(1, -1), 7)
    got = metrics.segmentation_confusion(torch.from_numpy(p).reshape(-1), torch.from_numpy(t).reshape(-1), 7)
    equal_ints(got, flat, "one flat image")
    assert got[0].shape == (1, 7, 8) and np.array_equal(flat[0][0], want[0].sum(0))
    with pytest.raises(ValueError, match="integer"):
        metrics.segmentation_confusion(torch.zeros(4, dtype=torch.int64), torch.zeros(4), 3)
    with pytest.raises(ValueError, match="channels"):
        metrics.segmentation_confusion(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="shape"):
        metrics.segmentation_confusion(torch.zeros(5, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 3)
    with pytest.raises(RuntimeError, match="fused"):
        metrics.segmentation_confusion(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 3, fused=True)


def test_out_accumulates_in_place():
    from instance_nerf_amd import metrics
    p, t = ids_case(3, 65, 13, seed=1)
    P, T = torch.from_numpy(p), torch.from_numpy(t)
    once = metrics.segmentation_confusion(P, T, 13)
    out = (torch.zeros(3, 13, 14, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
    back = metrics.segmentation_confusion(P, T, 13, out=out)
    assert back[0] is out[0] and back[1] is out[1]
    metrics.segmentation_confusion(P, T, 13, out=out)
    assert torch.equal(out[0], 2 * once[0]) and torch.equal(out[1], 2 * once[1])
    with pytest.raises(ValueError, match="counts"):
        metrics.segmentation_confusion(P, T, 13, out=(torch.zeros(3, 13, 13, dtype=torch.int64), out[1]))
    with pytest.raises(ValueError, match="ignored"):
        metrics.segmentation_confusion(P, T, 13, out=(out[0], torch.zeros(3, dtype=torch.int32)))


# ---------------------------------------------------------------------------- the arg-max rule
def argmax_rows(K):
    """Rows of K channels: ties at the first, last and all channels, signed zeros, one and several NaN, +-inf."""
    rng = np.random.default_rng(K)
    rows = []

    def base():
        return rng.normal(size=K).astype(np.float32)

    r = base(); r[0] = r[K - 1] = 9.0; rows.append(r)                       # tie of the first and the last channel
    r = base(); r[K - 1] = 9.0; r[K // 2] = 9.0; rows.append(r)             # tie ending at the last channel
    rows.append(np.full(K, 0.25, np.float32))                               # all channels tie
    r = np.full(K, -1.0, np.float32); r[K - 1] = 0.0; r[K // 2] = -0.0; rows.append(r)      # -0.0 before +0.0
    r = np.full(K, -1.0, np.float32); r[K - 1] = -0.0; r[K // 2] = 0.0; rows.append(r)      # +0.0 before -0.0
    r = base(); r[K // 2] = NAN; rows.append(r)                             # one NaN
    r = base(); r[K - 1] = NAN; r[K // 3] = NAN; r[0] = INF; rows.append(r)   # several NaN, an inf before them
    r = base(); r[K - 1] = INF; rows.append(r)
    r = base(); r[K // 2] = INF; r[K - 1] = INF; rows.append(r)             # two +inf tie
    rows.append(np.full(K, -INF, np.float32))                               # all -inf tie
    r = np.full(K, -INF, np.float32); r[K - 1] = -3.0e38; rows.append(r)
    rows.append(np.full(K, NAN, np.float32))
    rows.append(base())
    return np.stack(rows)


def padded(rows, ld):
    """The rows widened to ld channels; the padded channels hold what would win if they were read: +inf and NaN."""
    out = np.full((rows.shape[0], ld), INF, np.float32)
    out[:, :rows.shape[1]] = rows
    out[::2, rows.shape[1]:] = NAN
    return out


@pytest.mark.parametrize("K", [1, 3, 13, 64])
def test_argmax_rule_is_torch_argmax_on_cpu_tensors(K):
    from instance_nerf_amd import metrics
    rows = argmax_rows(K)
    want = torch.argmax(torch.from_numpy(rows), dim=-1).numpy()
    assert np.array_equal(cr.argmax_logits(rows, K), want)
    rng = np.random.default_rng(K + 100)
    t = rng.integers(-1, K, (1, rows.shape[0])).astype(np.int64)
    ref = cr.confusion(want[None], t, K)
    for ld in (K, K + 3):
        wide = padded(rows, ld)
        assert np.array_equal(cr.argmax_logits(wide, K), want), "the padded channels must be ignored"
        got = metrics.segmentation_confusion(torch.from_numpy(wide)[None], torch.from_numpy(t), K)
        equal_ints(got, ref, f"K{K} ld{ld}")


def test_composable_logits_in_other_float_dtypes():
    from instance_nerf_amd import metrics
    rng = np.random.default_rng(3)
    logits = torch.from_numpy(rng.normal(size=(2, 50, 7))).to(torch.float64)
    t = torch.from_numpy(rng.integers(-1, 5, (2, 50)))
    want = cr.confusion(cr.argmax_logits(logits.numpy(), 5), t.numpy(), 5)
    equal_ints(metrics.segmentation_confusion(logits, t, 5), want, "float64 logits, ld 7")


# ---------------------------------------------------------------------------- the meter against MIoUMeter
def random_views(K, seed, n_views=3, H=17, W=23):
    """Views with -1 pixels, an id (K - 1) that only the prediction contains and an id (K - 2) only the truth has."""
    rng = np.random.default_rng(seed)
    views = []
    for _ in range(n_views):
        t = rng.integers(0, K - 2, (1, H, W))
        p = np.where(rng.random((1, H, W)) < 0.7, t, rng.integers(0, K - 2, (1, H, W)))
        p[rng.random((1, H, W)) < 0.05] = K - 1
        t[rng.random((1, H, W)) < 0.03] = K - 2
        t[rng.random((1, H, W)) < 0.1] = -1
        views.append((torch.from_numpy(p), torch.from_numpy(t)))
    return views


@pytest.mark.parametrize("K", [4, 16])
def test_meter_equals_miou_meter_as_python_floats(K):
    from instance_nerf_amd.nerf.utils import MIoUMeter, SegmentationMeter
    old, new = MIoUMeter(K), SegmentationMeter(K)
    assert new.measure() == 0.0 and new.measure_all()["pq"] == 0.0          # nothing seen yet
    for p, t in random_views(K, seed=K):
        old.update(p, t)
        new.update(p, t)
    want, got = old.measure_both(), new.measure_all()
    assert want["miou_gt_ids"] != want["miou_all_ids"] and 0.0 < want["miou_gt_ids"] < 1.0
    assert got["miou_gt_ids"] == want["miou_gt_ids"] and got["miou_all_ids"] == want["miou_all_ids"]
    assert new.measure() == old.measure()
    assert got["counts"].shape == (K, K + 1) and int(got["counts"].sum() + got["ignored"].sum()) == 3 * 17 * 23
    for key in ("mIoU", "pixel acc", "PQ", "SQ", "RQ"):
        assert key in new.report()
    new.clear()
    assert new.counts is None and new.measure() == 0.0


def test_meter_takes_logits_and_a_prediction_outside_the_classes():
    from instance_nerf_amd.nerf.utils import MIoUMeter, SegmentationMeter
    K = 6
    rng = np.random.default_rng(9)
    logits = torch.from_numpy(rng.normal(size=(2, 40, K)).astype(np.float32))
    t = torch.from_numpy(rng.integers(-1, K, (2, 40)))
    a, b = SegmentationMeter(K), SegmentationMeter(K)
    a.update(logits, t)
    b.update(logits.argmax(-1), t)
    assert torch.equal(a.counts, b.counts) and torch.equal(a.ignored, b.ignored)
    # a predicted id outside [0, K): MIoUMeter counts the pixel towards the truth and its union and towards no prediction
    p = logits.argmax(-1)
    p[:, ::3] = K + 2
    old, new = MIoUMeter(K), SegmentationMeter(K)
    old.update(p, t)
    new.update(p, t)
    assert new.measure_all()["miou_gt_ids"] == old.measure_both()["miou_gt_ids"]
    assert new.measure_all()["miou_all_ids"] == old.measure_both()["miou_all_ids"]
    assert int(new.counts[:, K].sum()) == int(((t >= 0) & (p == K + 2)).sum())


def test_scores_against_the_restatement():
    from instance_nerf_amd import metrics
    for K, seed in ((5, 0), (16, 1)):
        counts = np.zeros((2, K, K + 1), np.int64)
        for p, t in random_views(K, seed):
            c, _ = cr.confusion(p.reshape(1, -1).numpy(), t.reshape(1, -1).numpy(), K)
            counts[seed % 2] += c[0]
        for match in ("id", "any"):
            got, want = metrics.segmentation_scores(torch.from_numpy(counts), match=match), cr.scores(counts, match=match)
            for key in ("tp", "fp", "fn"):
                assert got[key] == want[key] and isinstance(got[key], int), (key, match)
            assert np.array_equal(got["matches"].numpy(), want["matches"])
            assert np.array_equal(got["iou"].numpy(), want["iou"], equal_nan=True)       # one float64 division each
            for key in ("miou_gt_ids", "miou_all_ids", "pixel_acc", "pq", "sq", "rq", "pq_things", "sq_things", "rq_things"):
                assert abs(got[key] - want[key]) <= 4 * K * 2.0 ** -53, (key, match)     # sums of at most K terms below 1


# ---------------------------------------------------------------------------- panoptic quality, known answers
def matrix(K, entries):
    c = np.zeros((K, K + 1), np.int64)
    for (g, p), n in entries.items():
        c[g, p] = n
    return c


def pq_of(c, **kw):
    from instance_nerf_amd import metrics
    s = metrics.segmentation_scores(torch.from_numpy(c), **kw)
    present = int((c.sum(1) > 0).sum())
    assert s["tp"] + s["fn"] == present, "tp + fn is the number of truth segments present"
    assert s["tp"] == int((s["matches"] >= 0).sum())
    return s


def test_pq_of_a_perfect_prediction():
    for match in ("id", "any"):
        s = pq_of(matrix(4, {(0, 0): 50, (1, 1): 7, (3, 3): 1}), match=match)
        assert (s["pq"], s["sq"], s["rq"]) == (1.0, 1.0, 1.0) and (s["tp"], s["fp"], s["fn"]) == (3, 0, 0)
        assert (s["pq_things"], s["sq_things"], s["rq_things"]) == (1.0, 1.0, 1.0)
        assert s["matches"].tolist() == [0, 1, -1, 3] and s["pixel_acc"] == 1.0 and s["miou_gt_ids"] == 1.0


def test_iou_of_exactly_one_half_is_not_a_match():
    # truth 1: 3 pixels, prediction 1: 3 pixels, 2 in common -> IoU 2 / 4
    c = matrix(3, {(1, 1): 2, (1, 2): 1, (2, 1): 1})
    s = pq_of(c, stuff_ids=())
    assert s["iou"][1] == 0.5 and s["tp"] == 0 and s["pq"] == 0.0 and s["matches"].tolist() == [-1, -1, -1]
    assert (s["fp"], s["fn"]) == (2, 2)
    c[1, 1] = 3                                           # 3 in common, 4 + 4 in area: IoU 3 / 5
    s = pq_of(c, stuff_ids=())
    assert s["tp"] == 1 and s["sq"] == 3 / 5 and s["matches"].tolist() == [-1, 1, -1]
    assert s["pq"] == (3 / 5) / (1 + 0.5 + 0.5)


def test_a_consistent_relabelling_scores_one_under_any_and_zero_under_id():
    # stuff 0 stays; things 1, 2, 3 are predicted as 3, 1, 2
    c = matrix(4, {(0, 0): 40, (1, 3): 10, (2, 1): 20, (3, 2): 30})
    s = pq_of(c, match="any")
    assert (s["pq"], s["sq"], s["rq"]) == (1.0, 1.0, 1.0) and s["matches"].tolist() == [0, 3, 1, 2]
    assert s["pq_things"] == 1.0
    s = pq_of(c, match="id")
    assert s["pq_things"] == 0.0 and s["matches"].tolist() == [0, -1, -1, -1]
    assert (s["tp"], s["fp"], s["fn"]) == (1, 3, 3) and s["pq"] == 1.0 / (1 + 1.5 + 1.5)


def test_a_stuff_id_never_matches_a_thing_id_under_any():
    # stuff 0 is predicted as 2, thing 1 as 0: perfect overlaps, yet neither may match
    c = matrix(3, {(0, 2): 25, (1, 0): 25})
    s = pq_of(c, match="any", stuff_ids=(0,))
    assert s["tp"] == 0 and s["pq"] == 0.0 and (s["fp"], s["fn"]) == (2, 2)
    s = pq_of(c, match="any", stuff_ids=())               # without stuff ids both pairs match
    assert s["tp"] == 2 and s["pq"] == 1.0


def test_one_split_segment_is_one_tp_and_one_fp():
    # truth 1 (10 pixels) is predicted as 1 (7 pixels) and 2 (3 pixels)
    c = matrix(3, {(0, 0): 5, (1, 1): 7, (1, 2): 3})
    for match in ("id", "any"):
        s = pq_of(c, match=match)
        assert (s["tp"], s["fp"], s["fn"]) == (2, 1, 0)                       # stuff 0 and thing 1 match; 2 is the FP
        assert s["matches"].tolist() == [0, 1, -1]
        assert s["sq"] == (1.0 + 0.7) / 2 and s["rq"] == 2 / 2.5 and s["pq"] == (1.0 + 0.7) / 2.5
        assert s["pq_things"] == 0.7 / 1.5                                    # things: one TP, one FP


def test_an_empty_matrix_scores_zero_everywhere():
    s = pq_of(np.zeros((5, 6), np.int64))
    for key in ("miou_gt_ids", "miou_all_ids", "pixel_acc", "pq", "sq", "rq", "pq_things", "sq_things", "rq_things"):
        assert s[key] == 0.0, key
    assert (s["tp"], s["fp"], s["fn"]) == (0, 0, 0) and bool(torch.isnan(s["iou"]).all())
    from instance_nerf_amd import metrics
    with pytest.raises(ValueError, match="match"):
        metrics.segmentation_scores(torch.zeros(5, 6, dtype=torch.int64), match="best")
    with pytest.raises(ValueError, match="counts"):
        metrics.segmentation_scores(torch.zeros(5, 5, dtype=torch.int64))


def test_a_pixel_predicted_outside_the_classes_counts_against_its_truth_only():
    c = matrix(2, {(1, 1): 6, (1, 2): 2})                 # column K = 2
    s = pq_of(c, stuff_ids=())
    assert s["iou"][1] == 6 / 8 and s["pixel_acc"] == 6 / 8 and (s["tp"], s["fp"], s["fn"]) == (1, 0, 0)


# ---------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def abi():
    return abi_probe.run_abi_child("confusion_abi_child.py")


@pytest.mark.parametrize("name", ["inr_confusion_ids", "inr_confusion_logits"])
def test_bad_arguments_are_einval_with_a_message_that_names_them(abi, name):
    first = "pred" if name.endswith("ids") else "logits"
    cases = {f"{first}_null": "null", "truth_null": "null", "counts_null": "null", "ignored_null": "null",
             "K_0": "K", "K_65": "K", "K_negative": "K", "B_negative": "B", "N_negative": "N", "too_large": "2^63",
             "too_many_workgroups": "workgroups", "counts_misaligned": "counts", "ignored_misaligned": "ignored"}
    if first == "logits":
        cases.update(ld_below_K="ld", ld_too_large="2^63")
    for case, needle in cases.items():
        rc, msg = abi[f"{name}:{case}"]
        assert rc == EINVAL and needle in msg and name in msg, (name, case, rc, msg)
    for case in ("counts_misaligned", "ignored_misaligned"):
        assert "misaligned" in abi[f"{name}:{case}"][1]


@pytest.mark.parametrize("name", ["inr_confusion_ids", "inr_confusion_logits"])
def test_empty_input_is_a_no_op(abi, name):
    for case in ("B_0", "N_0", "B_0_null_pointers"):
        assert abi[f"{name}:{case}"][0] == 0, (name, case, abi[f"{name}:{case}"])


def test_binding_constants_are_the_header():
    import re
    from instance_nerf_amd import _lib, build, metrics
    header = open(os.path.join(ROOT, "include", "inr.h")).read()
    for py, c in ((_lib.CONFUSION_MAX_K, "INR_CONFUSION_MAX_K"), (_lib.CONFUSION_BLOCK, "INR_CONFUSION_BLOCK"),
                  (_lib.CONFUSION_PIXELS_PER_WG, "INR_CONFUSION_PIXELS_PER_WG")):
        assert py == int(re.search(rf"#define {c} (\d+)", header).group(1))
    assert metrics.CONFUSION_MAX_K == 64 and _lib.ABI_VERSION == 13
    assert "confusion.hip" in build.SOURCES and build.KERNEL_FILES["confusion"][0] == "confusion.hip"


# ---------------------------------------------------------------------------- reduce() on two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from instance_nerf_amd.nerf.utils import SegmentationMeter
    K = 8
    views = random_views(K, seed=21, n_views=4)
    whole, mine = SegmentationMeter(K), SegmentationMeter(K)
    for p, t in views:
        whole.update(p, t)
    for p, t in views[rank::world]:
        mine.update(p, t)
    part = mine.counts.clone()
    mine.reduce()
    ok = torch.equal(mine.counts, whole.counts) and torch.equal(mine.ignored, whole.ignored)
    ok = ok and not torch.equal(part, whole.counts) and mine.measure_all()["pq"] == whole.measure_all()["pq"]
    idle = SegmentationMeter(K)                    # a rank without views joins the reduction with zeros
    idle.reduce()
    ok = ok and int(idle.counts.sum()) == 0
    dist.barrier()
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_reduce_gives_the_matrix_of_the_whole_set():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(60)
    assert sorted(r[0] for r in res) == [0, 1] and all(r[1] for r in res)
