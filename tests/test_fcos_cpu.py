"""The FCOS targets and losses without a GPU: the numpy restatement (tests/fcos_reference.py) and the composable path of
instance_nerf_amd/fcos.py against the reference's own run (tests/golden/fcos.npz), the wrapper class, the corner cases, a
two-rank gloo run, autograd against float64, and the argument validation of the exports (tests/fcos_abi_child.py)."""
import hashlib
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe  # noqa: E402
import fcos_cases as fc  # noqa: E402
import fcos_reference as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
U = 2.0 ** -24                 # the unit roundoff of float32


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "fcos.npz"))


def T(x):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in x]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def prepare(case, **kw):
    from instance_nerf_amd import fcos
    return fcos.prepare_targets(case["shapes"], case["strides"], T(case["gts"]), case["radius"], case["norm"],
                                ori_sizes=case["ori_sizes"], **kw)


# ---------------------------------------------------------------------------- against the reference's own run
@pytest.mark.parametrize("name", sorted(fc.fixture_cases()))
def test_targets_of_restatement_and_composable_path_equal_the_reference(golden, name):
    case = fc.fixture_cases()[name]
    mine = fr.targets(case["shapes"], case["strides"], case["gts"], case["radius"], case["norm"], ori_sizes=case["ori_sizes"])
    t = prepare(case)
    sizes = [len(case["gts"]) * w * l * h for (w, l, h) in case["shapes"]]
    assert [len(x) for x in t.labels] == sizes and [tuple(x.shape) for x in t.reg_targets] == [(n, 6) for n in sizes]
    assert t.labels[0].data_ptr() == t.labels_flat.data_ptr() and t.labels_flat.dtype == torch.float32      # views of one buffer
    assert t.matched_flat.dtype == torch.int32 and t.centerness_flat.dtype == torch.float32
    for got in (mine, dict(labels=t.labels_flat.numpy(), reg=t.reg_targets_flat.numpy(), matched=t.matched_flat.numpy(),
                           centerness=t.centerness_flat.numpy(), valid=None if t.valid is None else t.valid_flat.numpy())):
        assert np.array_equal(got["labels"], golden[f"{name}_labels"].astype(np.float32))
        assert np.array_equal(got["matched"], golden[f"{name}_matched"].astype(np.int32))
        assert sha(got["reg"]) == golden[f"{name}_reg_sha256"].tobytes()
        pos = got["labels"] > 0
        assert sha(got["centerness"][pos]) == golden[f"{name}_ctr_sha256"].tobytes() and not got["centerness"][~pos].any()
        assert (got["valid"] is None) == (case["ori_sizes"] is None)
    if case["ori_sizes"] is not None:
        assert t.valid_flat.dtype == torch.bool and np.array_equal(t.valid_flat.numpy(), mine["valid"])
        assert 0 < int(mine["valid"].sum()) < len(mine["valid"])


def loss_allowance(n_terms, quotient_of_sums):
    """Relative allowance between two float32 evaluations of a loss whose per-location terms are the same bits.  Any order of
    adding n non-negative float32 terms is within (n - 1) u of the exact sum (u = 2^-24, first order), so two orders are
    within 2 (n - 1) u of each other; the reference adds the n compacted terms, this package the same terms with zeros in
    between.  The number of positives is exact; the sum of the centerness targets (the denominator of the regression loss)
    is such a sum again; each division rounds once more on either side."""
    return (2 * (n_terms - 1) * (2 if quotient_of_sums else 1) + 2) * U


@pytest.mark.parametrize("name", ["main_r15", "main_r0"])
def test_losses_of_the_composable_path_equal_the_reference(golden, name):
    from instance_nerf_amd import fcos
    case = fc.fixture_cases()[name]
    cls, reg, ctr = [T(a) for a in fc.predictions(7, case["shapes"], len(case["gts"]))]
    t = prepare(case)
    for i, lt in enumerate(fc.LOSS_TYPES):
        for j, tt in enumerate((t.with_valid(None), t)):
            valid = np.ones(len(t.labels_flat), bool) if j == 0 else t.valid_flat.numpy()
            n_pos = int((valid & (t.labels_flat.numpy() > 0)).sum())
            assert n_pos > 20
            got = [float(v) for v in fcos.fcos_loss(cls, reg, ctr, tt, lt)]
            want = golden[f"{name}_losses"][i, j]
            for k, (g, w, n, q) in enumerate(zip(got, want, (int(valid.sum()), n_pos, n_pos), (False, True, False))):
                assert abs(g - float(w)) <= loss_allowance(n, q) * abs(float(w)), (name, lt, j, k, g, w)
    assert not np.array_equal(golden[f"{name}_losses"][:, 0], golden[f"{name}_losses"][:, 1])       # the masks matter


def test_wrapper_class_gives_the_same_results():
    from instance_nerf_amd import fcos
    case = fc.fixture_cases()["main_r15"]
    cls, reg, ctr = [T(a) for a in fc.predictions(7, case["shapes"], 3)]
    locs = fcos.compute_locations(case["shapes"], case["strides"])
    masks = fcos.compute_padding_masks(locs, case["ori_sizes"])
    t = prepare(case)
    assert torch.equal(torch.cat([m.reshape(-1) for m in masks]), t.valid_flat)
    for lt in fc.LOSS_TYPES:
        comp = fcos.FCOSLossComputation(case["strides"], case["radius"], lt, case["norm"], 1)
        for m, tt in ((masks, t), (None, t.with_valid(None))):
            a = comp(locs, cls, reg, ctr, T(case["gts"]), m)
            b = fcos.fcos_loss(cls, reg, ctr, tt, lt)
            assert all(x.dim() == 0 and torch.equal(x, y) for x, y in zip(a, b))
    for kw, needle in ((dict(use_obb=True), "use_obb"), (dict(proj2d_loss_weight=0.5), "proj2d")):
        with pytest.raises(NotImplementedError, match=needle):
            fcos.FCOSLossComputation([4], 1.5, "iou", True, 1, **kw)
    for lt in ("smooth_l1", "diou"):
        with pytest.raises(NotImplementedError, match=lt):
            fcos.FCOSLossComputation([4], 1.5, lt, True)
        with pytest.raises(NotImplementedError, match=lt):
            fcos.fcos_loss(cls, reg, ctr, t, lt)


def test_empty_scene_single_scene_and_error_messages():
    from instance_nerf_amd import fcos
    shapes, strides = [(5, 4, 3), (3, 2, 2)], [4, 8]
    empty = fcos.prepare_targets(shapes, strides, [torch.zeros(0, 6)])
    assert not empty.labels_flat.any() and not empty.reg_targets_flat.any() and not empty.centerness_flat.any()
    assert not empty.matched_flat.any() and empty.valid is None and len(empty.labels_flat) == 72
    cls, reg, ctr = [T(a) for a in fc.predictions(1, shapes, 1)]
    for r in reg:
        r.requires_grad_(True)
    c, r_, k = fcos.fcos_loss(cls, reg, ctr, empty)                  # no positive: the focal sum over 1, and two zeros
    focal = fr.loss_terms(np, *[a.astype(np.float64) for a in fr.flatten(np, *fc.predictions(1, shapes, 1))],
                          np.zeros(72), np.zeros((72, 6)), None, "iou")[0]
    assert abs(float(c.detach()) - focal.sum()) <= 72 * U * focal.sum() and float(r_.detach()) == 0.0 and float(k.detach()) == 0.0
    (c + r_ + k).backward()
    assert all(not x.grad.any() for x in reg)
    one = fcos.prepare_targets(shapes, strides, [torch.tensor([[2.0, 1.0, 0.0, 18.0, 14.0, 11.0]])], 0.0, False)     # B == 1, no masks
    want = fr.targets(shapes, strides, [np.asarray([[2, 1, 0, 18, 14, 11]], np.float32)], 0.0, False)
    assert fr.same(one.reg_targets_flat.numpy(), want["reg"]) and np.array_equal(one.labels_flat.numpy(), want["labels"])
    assert one.labels_flat.sum() > 0 and all(float(v) > 0 for v in fcos.fcos_loss(cls, reg, ctr, one, "giou"))
    with pytest.raises(ValueError, match="oriented"):
        fcos.prepare_targets(shapes, strides, [torch.zeros(2, 7)])
    with pytest.raises(ValueError, match="non-empty list"):
        fcos.prepare_targets(shapes, strides, [])
    with pytest.raises(ValueError, match="stride"):
        fcos.prepare_targets(shapes, [4], [torch.zeros(1, 6)])
    with pytest.raises(ValueError, match="sizes_of_interest"):
        fcos.prepare_targets([(2, 2, 2)] * 5, [4] * 5, [torch.zeros(1, 6)])
    with pytest.raises(ValueError, match="ori_sizes"):
        fcos.prepare_targets(shapes, strides, [torch.zeros(1, 6)], ori_sizes=[(1, 1, 1), (2, 2, 2)])
    with pytest.raises(RuntimeError, match="fused"):
        fcos.prepare_targets(shapes, strides, [torch.zeros(1, 6)], fused=True)
    with pytest.raises(RuntimeError, match="fused"):
        fcos.fcos_loss(cls, reg, ctr, one, fused=True)
    with pytest.raises(ValueError, match="iou_loss_type"):
        fcos.fcos_loss(cls, reg, ctr, one, "l2")
    with pytest.raises(ValueError, match="levels"):
        fcos.fcos_loss(cls[:1], reg, ctr, one)
    with pytest.raises(ValueError, match="level 1"):
        fcos.fcos_loss(cls, [reg[0], reg[1][:, :5]], ctr, one)
    with pytest.raises(ValueError, match="prepare_targets"):
        fcos.fcos_loss(cls, reg, ctr, (one.labels, one.reg_targets))
    t64 = fcos.prepare_targets(shapes, strides, [torch.tensor([[2.0, 1.0, 0.0, 18.0, 14.0, 11.0]], dtype=torch.float64)], 0.0, False)
    assert t64.reg_targets_flat.dtype == torch.float64 and np.array_equal(t64.labels_flat.numpy(), want["labels"])


# ---------------------------------------------------------------------------- autograd
def test_autograd_of_the_composable_path_against_float64():
    """Gradients of 1.0 cls + 0.5 reg + 2.0 ctr.  The float64 side is torch autograd of the restatement (half the gradient
    to each side where pred == target: every third positive carries the target itself).  Allowance per kind of gradient:
    256 ulp of float32 at the largest magnitude of that kind - an element is fewer than 64 rounded operations, and the
    subtractions of the union (target + pred - intersection, with intersection <= min of both) amplify by at most 4."""
    from instance_nerf_amd import fcos
    case = fc.fixture_cases()["main_r15"]
    t = prepare(case)
    res = fr.targets(case["shapes"], case["strides"], case["gts"], case["radius"], case["norm"], ori_sizes=case["ori_sizes"])
    arrs = fc.predictions(9, case["shapes"], 3)
    assert fc.plant_ties(arrs[1], res, case["shapes"], 3) > 10
    for lt in fc.LOSS_TYPES:
        p32 = [[torch.from_numpy(a.copy()).requires_grad_(True) for a in group] for group in arrs]
        c, r, k = fcos.fcos_loss(*p32, t, lt)
        (1.0 * c + 0.5 * r + 2.0 * k).backward()
        p64 = [[torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in group] for group in arrs]
        terms = fr.loss_terms(torch, *fr.flatten(torch, *p64), torch.from_numpy(res["labels"]).double(),
                              torch.from_numpy(res["reg"]).double(), torch.from_numpy(res["valid"]), lt)
        c64, r64, k64 = fr.losses(torch, terms)
        (1.0 * c64 + 0.5 * r64 + 2.0 * k64).backward()
        for g32, g64, kind in zip(p32, p64, ("cls", "reg", "ctr")):
            for a, b in zip(g32, g64):
                top = float(b.grad.abs().max())
                assert top > 0 and float((a.grad.double() - b.grad).abs().max()) <= 256 * 2.0 ** -23 * top, (lt, kind)
        flat_reg = fr.flatten(torch, [g.grad for g in p32[0]], [g.grad for g in p32[1]], [g.grad for g in p32[2]])
        dead = torch.from_numpy(~(res["valid"] & (res["labels"] > 0)))
        assert not flat_reg[1][dead].any() and not flat_reg[2][dead].any() and not flat_reg[0][torch.from_numpy(~res["valid"])].any()


# ---------------------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_inputs(rank, second_is_empty):
    gts = fc.main_gts()
    mine = gts[0] if rank == 0 else (gts[1] if second_is_empty else gts[2])
    return [mine], fc.predictions(20 + rank, fc.MAIN_SHAPES, 1)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from instance_nerf_amd import fcos
    out = []
    for second_is_empty in (False, True):
        gts, arrs = _rank_inputs(rank, second_is_empty)
        t = fcos.prepare_targets(fc.MAIN_SHAPES, fc.STRIDES, T(gts))
        preds = [[torch.from_numpy(a).requires_grad_(True) for a in group] for group in arrs]
        losses = fcos.fcos_loss(*preds, t, "giou", world_size=world)
        sum(losses).backward()
        out.append([float(v) for v in losses] + [float(preds[1][0].grad.abs().sum())])
    dist.barrier()
    q.put((rank, out))
    dist.destroy_process_group()


def test_two_ranks_share_the_normalisers():
    """fcos_loss(world_size=2) over gloo: each rank's losses equal the single-process formula with the SUMMED normalisers
    halved - also when the second rank has no positive at all (its regression and centerness losses are then 0, and its
    focal sum is still divided by the shared count).  Allowance: float32 summation of the case's n = 6 588 terms
    (n u, see loss_allowance) plus 32 u for the rounding of a term's own evaluation against float64."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(60)
    for round_, second_is_empty in enumerate((False, True)):
        terms = []
        for rank in range(2):
            gts, arrs = _rank_inputs(rank, second_is_empty)
            r = fr.targets(fc.MAIN_SHAPES, fc.STRIDES, gts)
            flat = [a.astype(np.float64) for a in fr.flatten(np, *arrs)]
            terms.append(fr.loss_terms(np, *flat, r["labels"].astype(np.float64), r["reg"].astype(np.float64), None, "giou"))
        norms = (sum(float(t[3].sum()) for t in terms) / 2, sum(float(t[4].sum()) for t in terms) / 2)
        assert (terms[1][3].sum() == 0) == second_is_empty and terms[0][3].sum() > 0
        for rank in range(2):
            want = [float(v) for v in fr.losses(np, terms[rank], norms)]
            alone = [float(v) for v in fr.losses(np, terms[rank])]
            got = res[rank][round_]
            for g, w in zip(got[:3], want):
                assert abs(g - w) <= (6588 + 32) * U * abs(w), (round_, rank, got, want)
            assert abs(alone[0] - want[0]) > 0.01 * want[0]                  # the shared count is not the rank's own
            assert (got[3] > 0) == (terms[rank][3].sum() > 0)
        if second_is_empty:
            assert res[1][round_][1] == 0.0 and res[1][round_][2] == 0.0 and res[1][round_][0] > 0


# ---------------------------------------------------------------------------- ABI
def test_abi_facts():
    from instance_nerf_amd import _lib, build, fcos
    header = open(os.path.join(ROOT, "include", "inr.h")).read()
    for name in ("inr_fcos_targets", "inr_fcos_loss_workspace_bytes", "inr_fcos_loss_forward", "inr_fcos_loss_backward"):
        assert name in _lib.EXPORTS and name in abi_probe.prototypes()
        assert len(abi_probe.prototypes()[name]) == len(_lib._SIGS[name][1])
    assert "FCOS training targets and losses" in header
    assert "fcos.hip" in build.SOURCES and build.KERNEL_FILES["fcos"][0] == "fcos.hip"
    assert not set(build.KERNEL_FILES["fcos"]) & set(build.KERNEL_FILES["field"])
    assert _lib.ABI_VERSION == 13 and "#define INR_ABI_VERSION 13" in header
    for py, c in ((_lib.FCOS_MAX_LEVELS, "INR_FCOS_MAX_LEVELS"), (_lib.FCOS_MAX_GT, "INR_FCOS_MAX_GT"),
                  (_lib.FCOS_BLOCK, "INR_FCOS_BLOCK"), (_lib.FCOS_LOCATIONS_PER_WG, "INR_FCOS_LOCATIONS_PER_WG"),
                  (_lib.FCOS_LOSS_LOCATIONS_PER_WG, "INR_FCOS_LOSS_LOCATIONS_PER_WG"), (_lib.FCOS_LOSS_IOU, "INR_FCOS_LOSS_IOU"),
                  (_lib.FCOS_LOSS_LINEAR_IOU, "INR_FCOS_LOSS_LINEAR_IOU"), (_lib.FCOS_LOSS_GIOU, "INR_FCOS_LOSS_GIOU")):
        assert py == int(re.search(rf"#define {c} (\d+)", header).group(1))
    assert (_lib.FCOS_MAX_LEVELS, _lib.FCOS_MAX_GT) == (8, 1024) == (fcos.FCOS_MAX_LEVELS, fcos.FCOS_MAX_GT)
    assert fc.RUN == _lib.FCOS_LOCATIONS_PER_WG and sum(w * l * h for w, l, h in fc.MAIN_SHAPES) == 6588


@pytest.fixture(scope="module")
def abi():
    return abi_probe.run_abi_child("fcos_abi_child.py")


NULLS = {
    "inr_fcos_targets": ("level_dims", "level_strides", "level_ranges", "gt", "gt_offsets", "labels", "reg_targets"),
    "inr_fcos_loss_forward": ("cls_ptrs", "reg_ptrs", "ctr_ptrs", "level_dims", "labels", "reg_targets", "sums", "losses",
                              "workspace"),
    "inr_fcos_loss_backward": ("cls_ptrs", "reg_ptrs", "ctr_ptrs", "level_dims", "labels", "reg_targets", "norms",
                               "grad_losses", "d_cls_ptrs", "d_reg_ptrs", "d_ctr_ptrs"),
}


@pytest.mark.parametrize("name", sorted(NULLS))
def test_bad_arguments_are_einval_with_a_message_that_names_them(abi, name):
    cases = {f"{arg}_null": arg for arg in NULLS[name]}
    cases.update(n_levels_9="n_levels", n_levels_0="n_levels", B_negative="B", extent_negative="level_dims",
                 T_overflow="2^31", labels_misaligned="labels", B_0_n_levels_9="n_levels")
    if name == "inr_fcos_targets":
        cases.update(max_gt_1025="max_gt", max_gt_negative="max_gt", radius_negative="radius", stride_0="level_strides",
                     valid_without_ori_sizes="ori_sizes")
    else:
        cases.update(iou_loss_type_7="iou_loss_type", iou_loss_type_negative="iou_loss_type", level_pointer_null="reg_ptrs",
                     level_pointer_misaligned="ctr_ptrs")
    if name == "inr_fcos_loss_forward":
        cases.update(workspace_too_small="workspace", workspace_bytes_negative="workspace_bytes", sums_misaligned="sums")
    if name == "inr_fcos_loss_backward":
        cases.update(norms_misaligned="norms")
    for case, needle in cases.items():
        rc, msg = abi[f"{name}:{case}"]
        assert rc == EINVAL and needle in msg and name in msg, (name, case, rc, msg)
        if case.endswith("misaligned"):
            assert "misaligned" in msg, (name, case, msg)


def test_no_location_is_a_no_op_and_the_workspace_query(abi):
    for name in NULLS:
        for case in ("B_0", "B_0_null_pointers"):
            assert abi[f"{name}:{case}"][0] == 0, (name, case, abi[f"{name}:{case}"])
    assert abi["inr_fcos_targets:max_gt_0_gt_null_B_0"][0] == 0
    for case in ("T_negative", "T_overflow"):
        rc, msg = abi[f"inr_fcos_loss_workspace_bytes:{case}"]
        assert rc == EINVAL and "T" in msg and "inr_fcos_loss_workspace_bytes" in msg
    assert abi["inr_fcos_loss_workspace_bytes:T_0"][0] >= 40
    assert abi["inr_fcos_loss_workspace_bytes:T_19764"][0] == 20 * 5 * 8          # 20 workgroups of 1024 locations
