"""The box-matching kernels on the GPU (csrc/assign.hip), through the raw C ABI with guarded buffers and through
instance_nerf_amd.targets, against the numpy restatement tests/box_targets_reference.py (which equals the reference's own
run bit for bit: tests/test_box_targets_cpu.py).

Exact tier: the row-maximum keys, matched, labels, best_iou, matched_boxes and the three centre terms of targets equal the
restatement bit for bit (a NaN for a NaN: payloads are not part of the rule); null and non-null optional outputs and two
successive calls give the same bits; the guard words around every buffer are intact.

Size terms of targets (logf): held against float64 log of the bit-exact fp32 quotient, rounded to fp32.  The allowance is
twice the largest ulp distance that torch's own fp32 log ON THE SAME GPU AND QUOTIENTS shows against that value, and never
below 1 ulp - the kernel's logf and torch's are separate builds of one maths library, each specified to a few ulps.
Seen on the MI355X over every case of this file: the kernel's logf at most 2 ulp from the float64 value, torch's GPU log
at most 2 ulp (MEASURED_ULPS); all 10 tests pass in 3.5 s; torch.max on the GPU broke no tie differently.

Sizes, with R = the boxes of one workgroup (1024) and 64 a wave: A = 1, 63, 64, 65, R - 1, R, R + 1, 2 R + 1, each with
G = 1, 2, 63, 64, 65 and 1024 (the limit); odd A carry a padding mask, even G carry gt_labels, and the boxes of every
second case start 4 bytes off a 16-byte boundary."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_targets_cases as bc  # noqa: E402
import box_targets_reference as br  # noqa: E402
from kernel_harness import DEV, Buf, check, stream  # noqa: E402

pytestmark = pytest.mark.gpu
i32, f32 = np.int32, np.float32
OPTIONAL = ("labels", "best_iou", "matched_boxes", "targets")
# the largest ulp distances seen on the MI355X over every case of this file, against float64 log rounded to fp32:
# the kernel's logf, and torch.log on the same GPU and quotients
MEASURED_ULPS = {"kernel_logf": 2, "torch_gpu_log": 2}     # so the allowance was 4 ulp where it was largest


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


def run_len():
    from instance_nerf_amd import _lib
    assert _lib.BOX_MATCH_BOXES_PER_WG == bc.RUN and bc.RUN % _lib.BOX_MATCH_BLOCK == 0
    return bc.RUN


def run(lib, case, offset=0, outputs=OPTIONAL):
    """Both launches on guarded buffers -> dict of numpy arrays (keys uint32 [G], matched, and the requested outputs)."""
    gt, boxes = case["gt"], case["boxes"]
    G, A = len(gt), len(boxes)
    ins = {"gt": Buf(gt), "boxes": Buf(boxes, offset)}
    if case["valid"] is not None:
        padded = np.ones((A + 3) // 4 * 4, np.uint8)
        padded[:A] = case["valid"]
        ins["valid"] = Buf(padded)
    if case["gt_labels"] is not None:
        ins["gt_labels"] = Buf(case["gt_labels"].astype(i32))
    outs = {"keys": Buf(np.zeros(G, i32)), "matched": Buf(np.zeros(A, i32))}
    shapes = {"labels": ((A,), i32), "best_iou": ((A,), f32), "matched_boxes": ((A, 6), f32), "targets": ((A, 6), f32)}
    for name in outputs:
        outs[name] = Buf(np.zeros(*shapes[name]), offset if name in ("matched_boxes", "targets") else 0)
    for b in outs.values():
        b.fill_nan()

    def p(d, k):
        return d[k].ptr if k in d else None
    check(lib.inr_box_match_gt_max(ins["gt"].ptr, G, ins["boxes"].ptr, p(ins, "valid"), A, outs["keys"].ptr, stream()),
          "box_match_gt_max")
    check(lib.inr_box_match_assign(ins["gt"].ptr, p(ins, "gt_labels"), G, ins["boxes"].ptr, p(ins, "valid"), A,
                                   outs["keys"].ptr, case["high"], case["low"], int(case["allow"]), outs["matched"].ptr,
                                   p(outs, "labels"), p(outs, "best_iou"), p(outs, "matched_boxes"), p(outs, "targets"),
                                   stream()), "box_match_assign")
    for name, b in {**ins, **outs}.items():
        b.check_guards(name)
    got = {k: b.get() for k, b in outs.items()}
    got["keys"] = got["keys"].view(np.uint32)
    return got


def log_allowance(quot):
    """(allowance in ulps, torch's own distance) for the finite logs of these fp32 quotients on this GPU."""
    want = br.log_f64(quot)
    ok = np.isfinite(want)
    torch_gpu = torch.log(torch.from_numpy(np.ascontiguousarray(quot)).to(DEV)).cpu().numpy()
    d_torch = int(br.ulps(torch_gpu[ok], want[ok]).max()) if ok.any() else 0
    return max(1, 2 * d_torch), d_torch


SEEN = {"kernel_logf": 0, "torch_gpu_log": 0}


def compare(got, case, what):
    ref = br.assign(**case, log=br.log_f64)
    assert np.array_equal(got["keys"], br.float_key(ref["gt_max"])), what + " keys"
    assert np.array_equal(got["matched"], ref["matched"].astype(i32)), what + " matched"
    if "labels" in got:
        assert np.array_equal(got["labels"], ref["labels"].astype(i32)), what + " labels"
    if "best_iou" in got:
        assert br.same(got["best_iou"], ref["best_iou"]), what + " best_iou"
    if "matched_boxes" in got:
        assert br.same(got["matched_boxes"], ref["matched_boxes"]), what + " matched_boxes"
    if "targets" in got:
        assert br.same(got["targets"][:, :3], ref["targets"][:, :3]), what + " centre terms"
        quot = br.size_quotients(ref["matched_boxes"], case["boxes"])
        mine, want = got["targets"][:, 3:], ref["targets"][:, 3:]
        ok = np.isfinite(want)
        assert br.same(np.where(ok, f32(0), mine), np.where(ok, f32(0), want)), what + " non-finite size terms"
        allowance, d_torch = log_allowance(quot)
        d_mine = int(br.ulps(mine[ok], want[ok]).max()) if ok.any() else 0
        SEEN["kernel_logf"], SEEN["torch_gpu_log"] = max(SEEN["kernel_logf"], d_mine), max(SEEN["torch_gpu_log"], d_torch)
        print(f"{what}: size terms: kernel logf {d_mine} ulp, torch GPU log {d_torch} ulp, allowance {allowance}")
        assert d_mine <= allowance, (what, d_mine, d_torch, allowance)
    return ref


@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 1024])
def test_shapes_against_the_restatement(lib, G):
    R = run_len()
    for n, A in enumerate((1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 1)):
        case = bc.shape_case(A, G, masked=A % 2 == 1, labelled=G % 2 == 0, allow=(A + G) % 3 != 0, **bc.RPN)
        ref = compare(run(lib, case, offset=n % 2), case, f"A{A} G{G}")
        assert (ref["matched"] >= 0).any() and (A < 1023 or (ref["matched"] == -1).any())       # the case exercises the rule
    print("largest distances so far", SEEN)


def test_named_corners_against_the_restatement(lib):
    cases = bc.special_cases(run_len())
    for name, case in cases.items():
        ref = compare(run(lib, case), case, name)
        if name in bc.NAN_CASES:
            assert np.isnan(ref["best_iou"]).any(), name
    R = run_len()
    cw = run(lib, cases["cross_workgroup"])["matched"]
    assert np.flatnonzero(cw >= 0).tolist() == [5, R - 1, 2 * R]            # restored across workgroups, nothing else
    assert run(lib, cases["thresholds_rpn_strict"])["matched"].tolist() == [0, -2, -2, -1, -2, -2]
    assert run(lib, cases["thresholds_head"])["matched"].tolist() == [0, 0, -1, -1, 2, -1]
    assert (run(lib, cases["all_masked"])["labels"] == -1).all()
    print("largest distances so far", SEEN)


def test_optional_outputs_and_repeated_calls_give_the_same_bits(lib):
    R = run_len()
    for case in (bc.shape_case(2 * R + 1, 65, masked=True, labelled=True, **bc.RPN), bc.special_cases(R)["nan_box"]):
        full = run(lib, case, offset=1)
        again = run(lib, case, offset=1)
        for k in full:
            assert np.array_equal(full[k].view(np.uint32), again[k].view(np.uint32)), k      # NaN payloads included
        bare = run(lib, case, outputs=())
        assert set(bare) == {"keys", "matched"}
        assert np.array_equal(bare["matched"], full["matched"]) and np.array_equal(bare["keys"], full["keys"])
        for only in OPTIONAL:
            one = run(lib, case, outputs=(only,))
            assert np.array_equal(one[only].view(np.uint32), full[only].view(np.uint32)), only
            assert np.array_equal(one["matched"], full["matched"])


# ---------------------------------------------------------------------------- through targets.py
def D(x):
    return None if x is None else torch.from_numpy(x).to(DEV)


def tied_columns(case):
    """Columns whose maximum quality is attained by more than one GT: only there may another arg-max be right."""
    q = br.iou_matrix(case["gt"], case["boxes"], case["valid"])
    best, _ = br.max_nan(q, 0)
    return (q == best[None, :]).sum(0) > 1


def test_fused_equals_composable_on_gpu_tensors():
    """NaN-free cases.  The fused path must equal the restatement everywhere; the composable path on GPU tensors must equal
    it too, except that torch.max on a GPU may pick another index among EQUAL maxima: a difference is accepted only in a
    column whose maximum is tied, where the restatement (torch's CPU rule) is the arbiter."""
    from instance_nerf_amd import targets
    R = run_len()
    cases = {k: v for k, v in bc.special_cases(R).items() if k not in bc.NAN_CASES}
    cases["shape"] = bc.shape_case(R + 1, 24, masked=True, **bc.RPN)
    for name, case in cases.items():
        ref = br.assign(**case)
        args = (D(case["gt"]), D(case["boxes"]), case["high"], case["low"], case["allow"])
        fused = targets.match_boxes(*args, valid=D(case["valid"]), fused=True)
        plain = targets.match_boxes(*args, valid=D(case["valid"]), fused=False)
        auto = targets.match_boxes(*args, valid=D(case["valid"]))
        assert fused.dtype == plain.dtype == torch.int64 and fused.is_cuda
        assert np.array_equal(fused.cpu().numpy(), ref["matched"]), name
        differs = plain.cpu().numpy() != ref["matched"]
        if differs.any():
            print(f"{name}: torch.max on the GPU breaks {int(differs.sum())} ties differently")
        assert not (differs & ~tied_columns(case)).any(), name
        assert torch.equal(auto, fused if targets.MATCH_FUSED_BY_DEFAULT else plain), name
        if case["gt_labels"] is not None:
            a = targets.assign_targets_to_proposals([args[1]], [args[0]], [D(case["gt_labels"])], case["high"], case["low"], fused=True)
            assert a[0][0].dtype == a[1][0].dtype == torch.int64
            assert np.array_equal(a[0][0].cpu().numpy(), np.maximum(ref["matched"], 0))
            assert np.array_equal(a[1][0].cpu().numpy(), ref["labels"])
        elif case["allow"]:
            masks = None if case["valid"] is None else [D(case["valid"])]
            l, b, t = targets.assign_targets_to_anchors([args[1]], [args[0]], case["high"], case["low"], padding_masks=masks,
                                                        encode=True, fused=True)
            assert l[0].dtype == torch.float32 and np.array_equal(l[0].cpu().numpy(), ref["labels"].astype(f32)), name
            assert br.same(b[0].cpu().numpy(), ref["matched_boxes"]), name
            assert br.same(t[0].cpu().numpy()[:, :3], ref["targets"][:, :3]), name
    with pytest.raises(RuntimeError, match="fused"):
        targets.match_boxes(D(bc.scene(1, 5, 3)[0]).double(), D(bc.scene(1, 5, 3)[1]).double(), 0.35, 0.2, fused=True)
    big_gt = D(bc.scene(2, 40, 1025)[0])
    over = targets.match_boxes(big_gt, D(bc.scene(2, 40, 1025)[1]), 0.35, 0.2, True)          # G above the limit: composable
    assert over.shape == (40,) and over.dtype == torch.int64


def test_fused_assignment_and_sampler_read_nothing_back():
    from instance_nerf_amd import targets
    R = run_len()
    cases = [bc.shape_case(R + 65, 24, masked=True, **bc.RPN), bc.shape_case(777, 5, masked=True, **bc.RPN)]
    anchors, gts, masks = [D(c["boxes"]) for c in cases], [D(c["gt"]) for c in cases], [D(c["valid"]) for c in cases]
    gen = torch.Generator(device=DEV).manual_seed(5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        labels, boxes, reg = targets.assign_targets_to_anchors(anchors, gts, 0.35, 0.2, padding_masks=masks, encode=True, fused=True)
        picks = [targets.sample_balanced(l, 256, 0.5, generator=gen) for l in labels]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for c, l, b, t, (pos, neg) in zip(cases, labels, boxes, reg, picks):
        ref = br.assign(**c)
        assert np.array_equal(l.cpu().numpy(), ref["labels"].astype(f32)) and br.same(b.cpu().numpy(), ref["matched_boxes"])
        assert br.same(t.cpu().numpy()[:, :3], ref["targets"][:, :3])
        P, N = int((ref["labels"] >= 1).sum()), int((ref["labels"] == 0).sum())
        assert pos.dtype == neg.dtype == torch.uint8 and pos.is_cuda
        assert int(pos.sum()) == min(P, 128) and int(neg.sum()) == min(N, 256 - min(P, 128))
        assert not bool((pos.bool() & ~(l >= 1)).any()) and not bool((neg.bool() & ~(l == 0)).any())
