"""The FCOS kernels on the GPU (csrc/fcos.hip), through the raw C ABI with guarded buffers and through
instance_nerf_amd.fcos, against the restatement tests/fcos_reference.py (which equals the reference's own run bit for bit:
tests/golden/make_fcos_golden.py, tests/test_fcos_cpu.py).

Exact tier (targets): labels, matched, regression targets, centerness and valid equal the restatement bit for bit (a NaN for
a NaN); null and non-null optional outputs and two successive calls give the same bits; guard words stay intact.
Loss sums: each of the five sums equals the float64 sum of the kernel's own emitted terms to within 1 ulp of float32, and
the three losses are exactly the quotients of those sums rounded to float32.
Loss terms and gradients: against the float64 restatement.  Per kind of term and case the kernel's largest absolute error
may be at most twice the largest absolute error that torch's own float32 composable path shows ON THE SAME GPU AND INPUTS
(both against float64), and the allowance is never below 1 ulp of the case's largest term of that kind.

Sizes, with R = the locations of one workgroup (256) and 64 a wave: single-level pyramids of 1, 63, 64, 65, R - 1, R,
R + 1 and 2 R + 1 locations (none a cube), each with G = 1, 2, 63, 64, 65 and 1024 boxes in the first scene and G // 2 in
the second (so G = 1 brings an empty scene); radius 0 and 1.5 and norm_reg_targets on and off alternate with P + G and G;
every second case has its outputs 4 bytes off a 16-byte boundary; the 6 588-location pyramid has B = 3 with an empty
scene."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fcos_cases as fc  # noqa: E402
import fcos_reference as fr  # noqa: E402
from kernel_harness import DEV, Buf, check, stream  # noqa: E402

pytestmark = pytest.mark.gpu
i32, f32, f64 = np.int32, np.float32, np.float64
OPTIONAL = ("centerness", "matched", "valid")
KINDS = ("cls_terms", "reg_terms", "ctr_terms", "d_cls", "d_reg", "d_ctr")
GRADS = (1.0, 0.5, 2.0)                    # the upstream gradients of (cls, reg, ctr)
# The largest absolute errors against float64 seen on the MI355X, per case and kind: (kernel, torch float32 composable on
# the same GPU and inputs, 1 ulp of the largest term), as a device run of this file printed them; all 18 tests took 5.2 s.
# The kernel's error is at most 1.7 times torch's own in every row (main_r0 iou d_reg), and centerness stayed in the exact tier.
MEASURED = {
    "main_r15 iou masks=1 ties=0 cls_terms": (1.068e-06, 1.068e-06, 4.768e-07),
    "main_r15 iou masks=1 ties=0 reg_terms": (4.198e-07, 4.198e-07, 4.768e-07),
    "main_r15 iou masks=1 ties=0 ctr_terms": (1.067e-07, 1.269e-07, 1.192e-07),
    "main_r15 iou masks=1 ties=0 d_cls": (1.052e-08, 1.052e-08, 1.863e-09),
    "main_r15 iou masks=1 ties=0 d_reg": (1.849e-09, 2.313e-09, 1.863e-09),
    "main_r15 iou masks=1 ties=0 d_ctr": (3.589e-09, 3.589e-09, 1.863e-09),
    "main_r15 linear_iou masks=0 ties=0 cls_terms": (1.068e-06, 1.068e-06, 4.768e-07),
    "main_r15 linear_iou masks=0 ties=0 reg_terms": (6.219e-08, 6.219e-08, 5.960e-08),
    "main_r15 linear_iou masks=0 ties=0 ctr_terms": (1.255e-07, 1.269e-07, 1.192e-07),
    "main_r15 linear_iou masks=0 ties=0 d_cls": (9.336e-09, 1.027e-08, 9.313e-10),
    "main_r15 linear_iou masks=0 ties=0 d_reg": (2.080e-10, 1.889e-10, 1.164e-10),
    "main_r15 linear_iou masks=0 ties=0 d_ctr": (3.145e-09, 3.145e-09, 1.863e-09),
    "main_r15 giou masks=1 ties=1 cls_terms": (1.068e-06, 1.068e-06, 4.768e-07),
    "main_r15 giou masks=1 ties=1 reg_terms": (9.212e-08, 9.212e-08, 1.192e-07),
    "main_r15 giou masks=1 ties=1 ctr_terms": (1.067e-07, 1.269e-07, 1.192e-07),
    "main_r15 giou masks=1 ties=1 d_cls": (1.052e-08, 1.052e-08, 1.863e-09),
    "main_r15 giou masks=1 ties=1 d_reg": (1.012e-09, 1.205e-09, 4.657e-10),
    "main_r15 giou masks=1 ties=1 d_ctr": (3.589e-09, 3.589e-09, 1.863e-09),
    "main_r0 giou masks=1 ties=0 cls_terms": (1.068e-06, 1.068e-06, 4.768e-07),
    "main_r0 giou masks=1 ties=0 reg_terms": (1.409e-07, 1.409e-07, 1.192e-07),
    "main_r0 giou masks=1 ties=0 ctr_terms": (1.067e-07, 1.269e-07, 2.384e-07),
    "main_r0 giou masks=1 ties=0 d_cls": (9.028e-09, 8.759e-09, 1.863e-09),
    "main_r0 giou masks=1 ties=0 d_reg": (2.898e-10, 2.898e-10, 2.328e-10),
    "main_r0 giou masks=1 ties=0 d_ctr": (2.643e-09, 2.643e-09, 1.863e-09),
    "main_r0 iou masks=0 ties=1 cls_terms": (1.068e-06, 1.068e-06, 4.768e-07),
    "main_r0 iou masks=0 ties=1 reg_terms": (6.182e-07, 6.182e-07, 4.768e-07),
    "main_r0 iou masks=0 ties=1 ctr_terms": (1.255e-07, 1.269e-07, 2.384e-07),
    "main_r0 iou masks=0 ties=1 d_cls": (7.971e-09, 7.971e-09, 9.313e-10),
    "main_r0 iou masks=0 ties=1 d_reg": (2.397e-09, 1.466e-09, 9.313e-10),
    "main_r0 iou masks=0 ties=1 d_ctr": (2.075e-09, 2.075e-09, 1.863e-09),
    "single linear_iou masks=1 ties=1 cls_terms": (5.106e-07, 5.106e-07, 4.768e-07),
    "single linear_iou masks=1 ties=1 reg_terms": (2.577e-08, 2.577e-08, 5.960e-08),
    "single linear_iou masks=1 ties=1 ctr_terms": (6.299e-08, 6.299e-08, 1.192e-07),
    "single linear_iou masks=1 ties=1 d_cls": (8.244e-08, 8.397e-08, 1.490e-08),
    "single linear_iou masks=1 ties=1 d_reg": (9.895e-10, 6.496e-10, 4.657e-10),
    "single linear_iou masks=1 ties=1 d_ctr": (1.416e-08, 1.416e-08, 1.490e-08),
}
SEEN = {}


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    assert _lib.FCOS_LOCATIONS_PER_WG == fc.RUN
    return _lib.load()


def host_i32(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def hp(arr):
    return ctypes.cast(arr, ctypes.c_void_p)


def total_of(case):
    return len(case["gts"]) * sum(w * l * h for (w, l, h) in case["shapes"])


def bytes_buf(n):
    b = Buf(np.zeros((n + 3) // 4 * 4, np.uint8))
    b.fill_nan()
    return b


def run_targets(lib, case, offset=0, outputs=OPTIONAL):
    """inr_fcos_targets on guarded buffers -> dict of numpy arrays."""
    shapes, strides, gts = case["shapes"], case["strides"], case["gts"]
    B, n, T = len(gts), len(shapes), total_of(case)
    counts = [len(g) for g in gts]
    ranges = fr.SIZES_OF_INTEREST[:n]
    ins = {"offsets": Buf(np.concatenate(([0], np.cumsum(counts))).astype(i32)),
           "ori": Buf(np.asarray(case["ori_sizes"], f32).reshape(B, 3))}
    if sum(counts):
        ins["gt"] = Buf(np.concatenate(gts).astype(f32), offset)
    outs = {"labels": Buf(np.zeros(T, f32), offset), "reg": Buf(np.zeros((T, 6), f32), offset)}
    if "centerness" in outputs:
        outs["centerness"] = Buf(np.zeros(T, f32), offset)
    if "matched" in outputs:
        outs["matched"] = Buf(np.zeros(T, i32), offset)
    for b in outs.values():
        b.fill_nan()
    if "valid" in outputs:
        outs["valid"] = bytes_buf(T)
    dims, strd = host_i32([v for s in shapes for v in s]), host_i32(strides)
    rng = (ctypes.c_float * (2 * n))(*[float(v) for r in ranges for v in r])

    def p(d, k):
        return d[k].ptr if k in d else None
    check(lib.inr_fcos_targets(hp(dims), hp(strd), hp(rng), n, B, p(ins, "gt"), ins["offsets"].ptr, max(counts), ins["ori"].ptr,
                               float(case["radius"]), int(case["norm"]), outs["labels"].ptr, outs["reg"].ptr,
                               p(outs, "centerness"), p(outs, "matched"), p(outs, "valid"), stream()), "fcos_targets")
    torch.cuda.synchronize()
    for name, b in {**ins, **outs}.items():
        b.check_guards(name)
    got = {k: b.get() for k, b in outs.items()}
    if "valid" in got:
        untouched = np.tile(np.frombuffer(np.int32(0x7FC0BEEF).tobytes(), np.uint8), len(got["valid"]) // 4)
        assert np.array_equal(got["valid"][T:], untouched[T:]), "valid: a byte past the last location was written"
        got["valid"] = got["valid"][:T]
    return got


def compare_targets(got, case, what):
    ref = fr.targets(case["shapes"], case["strides"], case["gts"], case["radius"], case["norm"], ori_sizes=case["ori_sizes"])
    assert fr.same(got["labels"], ref["labels"]), what + " labels"
    assert fr.same(got["reg"], ref["reg"]), what + " reg_targets"
    if "centerness" in got:
        assert fr.same(got["centerness"], ref["centerness"]), what + " centerness"
    if "matched" in got:
        assert np.array_equal(got["matched"], ref["matched"]), what + " matched"
    if "valid" in got:
        assert np.array_equal(got["valid"] != 0, ref["valid"]) and set(np.unique(got["valid"])) <= {0, 1}, what + " valid"
    return ref


@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 1024])
def test_target_shapes_against_the_restatement(lib, G):
    R = fc.RUN
    positives = 0
    for n, P in enumerate((1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 1)):
        case = fc.single_level_case(P, G)
        assert case["shapes"][0][0] * case["shapes"][0][1] * case["shapes"][0][2] == P
        ref = compare_targets(run_targets(lib, case, offset=n % 2), case, f"P{P} G{G}")
        positives += int(ref["labels"].sum())
    assert positives > 0                                   # the cases exercise the rule


@pytest.mark.parametrize("name", ["main_r15", "main_r0"])
def test_the_fixture_pyramid_with_an_empty_scene(lib, name):
    case = fc.fixture_cases()[name]
    assert total_of(case) == 3 * 6588 and len(case["gts"][1]) == 0
    ref = compare_targets(run_targets(lib, case, offset=1), case, name)
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcos.npz"))
    assert np.array_equal(ref["matched"], golden[f"{name}_matched"].astype(i32)) and ref["ties"].any() and ref["on_face"].any()
    for l in range(4):
        assert ((ref["level"] == l) & (ref["labels"] > 0)).any()


def test_nan_boxes_follow_the_rule(lib):
    case = fc.single_level_case(fc.RUN + 1, 5)
    case["gts"][0][1, 3] = np.nan                          # a NaN face: never inside, never chosen unless first
    case["gts"][0][3, :] = [np.inf, 0, 0, np.inf, 8, 8]    # inf - inf: a NaN volume
    compare_targets(run_targets(lib, case), case, "nan boxes")


def test_optional_outputs_and_repeated_calls_give_the_same_bits(lib):
    for case in (fc.fixture_cases()["main_r15"], fc.single_level_case(2 * fc.RUN + 1, 65)):
        full = run_targets(lib, case, offset=1)
        again = run_targets(lib, case, offset=1)
        for k in full:
            assert np.array_equal(full[k].view(np.uint8), again[k].view(np.uint8)), k
        bare = run_targets(lib, case, outputs=())
        assert set(bare) == {"labels", "reg"}
        for only in OPTIONAL:
            one = run_targets(lib, case, outputs=(only,))
            for k in one:
                assert np.array_equal(one[k].view(np.uint8), full[k].view(np.uint8)), (only, k)


# ---------------------------------------------------------------------------- losses through the raw ABI
LOSS_IDS = {"iou": 0, "linear_iou": 1, "giou": 2}


def run_loss(lib, shapes, B, preds, labels, regt, valid, loss_type, norms=None, terms=True, offset=0):
    """inr_fcos_loss_forward (and _backward with ``norms`` = (n_pos, sum of centerness targets)) on guarded buffers."""
    n, T = len(shapes), len(labels)
    dims = host_i32([v for s in shapes for v in s])
    pb = [[Buf(a, offset) for a in group] for group in preds]
    ptrs = [(ctypes.c_void_p * n)(*[b.ptr for b in group]) for group in pb]
    ins = {"labels": Buf(labels.astype(f32), offset), "regt": Buf(regt.astype(f32))}
    if valid is not None:
        padded = np.zeros((T + 3) // 4 * 4, np.uint8)
        padded[:T] = valid
        ins["valid"] = Buf(padded)
    nbytes = int(lib.inr_fcos_loss_workspace_bytes(T))
    assert nbytes == (T + 1023) // 1024 * 40
    outs = {"sums": Buf(np.zeros(10, f32)), "losses": Buf(np.zeros(3, f32), offset), "workspace": Buf(np.zeros(nbytes // 4, f32))}
    if terms:
        for k in KINDS[:3]:
            outs[k] = Buf(np.zeros(T, f32), offset)
    for b in outs.values():
        b.fill_nan()

    def p(d, k):
        return d[k].ptr if k in d else None
    vp = p(ins, "valid")
    check(lib.inr_fcos_loss_forward(hp(ptrs[0]), hp(ptrs[1]), hp(ptrs[2]), hp(dims), n, B, ins["labels"].ptr, ins["regt"].ptr, vp,
                                    LOSS_IDS[loss_type], outs["sums"].ptr, outs["losses"].ptr, p(outs, "cls_terms"),
                                    p(outs, "reg_terms"), p(outs, "ctr_terms"), outs["workspace"].ptr, nbytes, stream()),
          "fcos_loss_forward")
    grads = None
    if norms is not None:
        ins["norms"] = Buf(np.asarray(norms, f64).view(f32))
        ins["gout"] = Buf(np.asarray(GRADS, f32), offset)
        grads = [[Buf(np.zeros_like(a), offset) for a in group] for group in preds]
        for group in grads:
            for b in group:
                b.fill_nan()
        gptrs = [(ctypes.c_void_p * n)(*[b.ptr for b in group]) for group in grads]
        check(lib.inr_fcos_loss_backward(hp(ptrs[0]), hp(ptrs[1]), hp(ptrs[2]), hp(dims), n, B, ins["labels"].ptr,
                                         ins["regt"].ptr, vp, LOSS_IDS[loss_type], ins["norms"].ptr, ins["gout"].ptr,
                                         hp(gptrs[0]), hp(gptrs[1]), hp(gptrs[2]), stream()), "fcos_loss_backward")
    torch.cuda.synchronize()
    every = {**ins, **outs}
    for gi, group in enumerate(pb + (grads or [])):
        every.update({f"level buffer {gi}.{l}": b for l, b in enumerate(group)})
    for name, b in every.items():
        b.check_guards(name)
    got = {k: b.get() for k, b in outs.items() if k != "workspace"}
    got["sums"] = got["sums"].view(f64)
    if grads is not None:
        flat = fr.flatten(np, *[[b.get() for b in group] for group in grads])
        got.update(d_cls=flat[0], d_reg=flat[1], d_ctr=flat[2])
    return got


def float64_side(preds, ref, valid, loss_type):
    """The restatement in float64 with torch autograd -> dict of the six kinds, and (n_pos, sum of centerness targets)."""
    p64 = [[torch.from_numpy(a.astype(f64)).requires_grad_(True) for a in group] for group in preds]
    terms = fr.loss_terms(torch, *fr.flatten(torch, *p64), torch.from_numpy(ref["labels"]).double(),
                          torch.from_numpy(ref["reg"]).double(), None if valid is None else torch.from_numpy(valid), loss_type)
    norms = (float(terms[3].sum()), float(terms[4].detach().sum()))
    n1 = max(norms[0], 1.0)
    (GRADS[0] * terms[0].sum() / n1 + GRADS[1] * terms[1].sum() / norms[1] + GRADS[2] * terms[2].sum() / n1).backward()
    flat = fr.flatten(np, *[[t.grad.numpy() for t in group] for group in p64])
    out = dict(cls_terms=terms[0].detach().numpy(), reg_terms=terms[1].detach().numpy(), ctr_terms=terms[2].detach().numpy(),
               d_cls=flat[0], d_reg=flat[1], d_ctr=flat[2])
    return out, norms


def torch_float32_side(case, preds, valid, loss_type, norms):
    """The composable path's terms and gradients in float32 on this GPU, with the same normalisers."""
    from instance_nerf_amd import fcos
    t = fcos.prepare_targets(case["shapes"], case["strides"], [torch.from_numpy(g) for g in case["gts"]], case["radius"],
                             case["norm"], fused=False)
    t = fcos.FCOSTargets(t.feature_shapes, t.strides, t.B, t.labels_flat.to(DEV), t.reg_targets_flat.to(DEV),
                         t.centerness_flat.to(DEV), t.matched_flat.to(DEV), None if valid is None else torch.from_numpy(valid).to(DEV))
    p32 = [[torch.from_numpy(a).to(DEV).requires_grad_(True) for a in group] for group in preds]
    terms = fcos.loss_terms(*p32, t, loss_type)
    n1 = max(norms[0], 1.0)
    (GRADS[0] * terms[0].sum() / n1 + GRADS[1] * terms[1].sum() / norms[1] + GRADS[2] * terms[2].sum() / n1).backward()
    flat = fr.flatten(np, *[[x.grad.cpu().numpy() for x in group] for group in p32])
    return dict(cls_terms=terms[0].detach().cpu().numpy(), reg_terms=terms[1].detach().cpu().numpy(),
                ctr_terms=terms[2].detach().cpu().numpy(), d_cls=flat[0], d_reg=flat[1], d_ctr=flat[2])


def check_against_float64(what, got, want, plain):
    """The measured allowance per kind: twice torch's own float32 error, at least 1 ulp of the largest term."""
    for kind in KINDS:
        e_kernel = float(np.abs(got[kind].astype(f64) - want[kind]).max())
        e_torch = float(np.abs(plain[kind].astype(f64) - want[kind]).max())
        one_ulp = fr.ulp(np.abs(want[kind]).max())
        SEEN[f"{what} {kind}"] = (e_kernel, e_torch, one_ulp)
        print(f"MEASURED {what} {kind}: kernel {e_kernel:.3e}, torch float32 {e_torch:.3e}, 1 ulp of the largest {one_ulp:.3e}")
        assert np.isfinite(got[kind]).all() and np.abs(want[kind]).max() > 0, (what, kind)
        assert e_kernel <= max(2 * e_torch, one_ulp), (what, kind, e_kernel, e_torch, one_ulp)


def loss_case(name, loss_type, masks, ties):
    case = fc.fixture_cases()[name] if name in fc.fixture_cases() else fc.single_level_case(2 * fc.RUN + 1, 5)
    B = len(case["gts"])
    ref = fr.targets(case["shapes"], case["strides"], case["gts"], case["radius"], case["norm"], ori_sizes=case["ori_sizes"])
    preds = fc.predictions(9, case["shapes"], B)
    if ties:
        assert fc.plant_ties(preds[1], ref, case["shapes"], B) > 0
    return case, ref, preds, (ref["valid"] if masks else None)


@pytest.mark.parametrize("name,loss_type,masks,ties", [
    ("main_r15", "iou", True, False), ("main_r15", "linear_iou", False, False), ("main_r15", "giou", True, True),
    ("main_r0", "giou", True, False), ("main_r0", "iou", False, True), ("single", "linear_iou", True, True)])
def test_loss_terms_sums_and_gradients(lib, name, loss_type, masks, ties):
    case, ref, preds, valid = loss_case(name, loss_type, masks, ties)
    B, T = len(case["gts"]), len(ref["labels"])
    want, norms = float64_side(preds, ref, valid, loss_type)
    assert norms[0] > 0
    got = run_loss(lib, case["shapes"], B, preds, ref["labels"], ref["reg"], valid, loss_type, norms=norms, offset=int(ties))
    what = f"{name} {loss_type} masks={int(masks)} ties={int(ties)}"
    # ---- the five sums against the kernel's own terms, the losses against the sums
    ok = np.ones(T, bool) if valid is None else valid
    pos = ok & (ref["labels"] > 0)
    own = [got["cls_terms"].astype(f64).sum(), got["reg_terms"].astype(f64).sum(), got["ctr_terms"].astype(f64).sum(),
           float(pos.sum()), ref["centerness"][pos].astype(f64).sum()]
    for k, (s, o) in enumerate(zip(got["sums"], own)):
        assert abs(s - o) <= fr.ulp(o), (what, k, s, o)
    assert got["sums"][3] == own[3] == norms[0]
    assert not got["cls_terms"][~ok].any() and not got["reg_terms"][~pos].any() and not got["ctr_terms"][~pos].any()
    s = got["sums"]
    assert np.array_equal(got["losses"], np.asarray([s[0] / max(s[3], 1), s[1] / s[4], s[2] / max(s[3], 1)]).astype(f32)), what
    # ---- zero gradients
    assert not got["d_cls"][~ok].any() and not got["d_reg"][~pos].any() and not got["d_ctr"][~pos].any()
    # ---- terms and gradients against float64, allowance measured on this GPU
    check_against_float64(what, got, want, torch_float32_side(case, preds, valid, loss_type, norms))
    if ties:                                                # half the gradient to each side: nothing else gives these values
        equal = fr.flatten(np, *preds)[1] == ref["reg"]
        tied = pos & equal[:, fc.TIED].all(1) & ~equal.all(1)
        assert tied.sum() > 0 and (np.abs(want["d_reg"][tied][:, fc.TIED]) > 0).all()
        assert (pos & equal.all(1)).sum() > 0 or name == "single"
    # ---- two calls, with and without the term outputs: the same bits
    again = run_loss(lib, case["shapes"], B, preds, ref["labels"], ref["reg"], valid, loss_type, terms=False)
    assert np.array_equal(again["sums"].view(np.uint8), got["sums"].view(np.uint8))
    assert np.array_equal(again["losses"].view(np.uint8), got["losses"].view(np.uint8))


def test_no_positive_gives_zero_regression_and_centerness_losses(lib):
    case = fc.single_level_case(fc.RUN + 1, 1)
    shapes, B = case["shapes"], 2
    T = total_of(case)
    preds = fc.predictions(3, shapes, B)
    got = run_loss(lib, shapes, B, preds, np.zeros(T, f32), np.zeros((T, 6), f32), None, "giou", norms=(0.0, 0.0))
    assert got["losses"][0] > 0 and got["losses"][1] == 0 and got["losses"][2] == 0 and got["sums"][3] == 0
    assert np.isfinite(got["d_cls"]).all() and got["d_cls"].any() and not got["d_reg"].any() and not got["d_ctr"].any()


# ---------------------------------------------------------------------------- through fcos.py
def test_end_to_end_fused_against_composable_and_the_fixture():
    """prepare_targets and fcos_loss(...).backward() on the 6 588-location case, B = 3: fused against composable on the same
    GPU within the measured allowances, nothing read back on the fused path, and the three losses against the reference's
    run (tests/golden/fcos.npz).  Allowance for the losses: the reference adds its n float32 terms in float32 - within
    (n - 1) u of the exact sum, twice that for the quotient of two sums - while the kernel adds in float64; 16 u more for
    terms that two maths libraries evaluate a few ulp apart."""
    from instance_nerf_amd import fcos
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcos.npz"))
    U = 2.0 ** -24
    for name in ("main_r15", "main_r0"):
        case = fc.fixture_cases()[name]
        ref = fr.targets(case["shapes"], case["strides"], case["gts"], case["radius"], case["norm"], ori_sizes=case["ori_sizes"])
        gts = [torch.from_numpy(g).to(DEV) for g in case["gts"]]
        arrs = fc.predictions(7, case["shapes"], 3)
        for i, lt in enumerate(fc.LOSS_TYPES):
            p_f = [[torch.from_numpy(a).to(DEV).requires_grad_(True) for a in group] for group in arrs]
            p_c = [[torch.from_numpy(a).to(DEV).requires_grad_(True) for a in group] for group in arrs]
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                t = fcos.prepare_targets(case["shapes"], case["strides"], gts, case["radius"], case["norm"],
                                         ori_sizes=case["ori_sizes"], fused=True)
                fused = fcos.fcos_loss(*p_f, t, lt, fused=True)
                (GRADS[0] * fused[0] + GRADS[1] * fused[1] + GRADS[2] * fused[2]).backward()
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert fr.same(t.labels_flat.cpu().numpy(), ref["labels"]) and fr.same(t.reg_targets_flat.cpu().numpy(), ref["reg"])
            assert fr.same(t.centerness_flat.cpu().numpy(), ref["centerness"]) and np.array_equal(t.matched_flat.cpu().numpy(), ref["matched"])
            assert t.valid_flat.dtype == torch.bool and np.array_equal(t.valid_flat.cpu().numpy(), ref["valid"])
            assert t.labels[1].data_ptr() == t.labels_flat.data_ptr() + 4 * 3 * 24 * 20 * 12
            auto = fcos.fcos_loss([p.detach() for p in p_f[0]], [p.detach() for p in p_f[1]], [p.detach() for p in p_f[2]], t, lt)
            assert all(torch.equal(a, b.detach()) for a, b in zip(auto, fused)) or not fcos.LOSS_FUSED_BY_DEFAULT
            plain = fcos.fcos_loss(*p_c, t, lt, fused=False)
            (GRADS[0] * plain[0] + GRADS[1] * plain[1] + GRADS[2] * plain[2]).backward()
            want, norms = float64_side(arrs, ref, ref["valid"], lt)
            n_valid = int(ref["valid"].sum())
            for k, n, q in ((0, n_valid, 1), (1, int(norms[0]), 2), (2, int(norms[0]), 1)):
                w = float(golden[f"{name}_losses"][i, 1, k])
                assert fused[k].dim() == 0 and abs(float(fused[k]) - w) <= ((n - 1) * q + 2 + 16) * U * w, (name, lt, k, float(fused[k]), w)
            for kind, g_f, g_c in zip(KINDS[3:], p_f, p_c):
                flat_f = np.concatenate([x.grad.cpu().numpy().reshape(-1) for x in g_f])
                flat_c = np.concatenate([x.grad.cpu().numpy().reshape(-1) for x in g_c])
                flat_w = np.concatenate([x.reshape(-1) for x in split_levels(want[kind], case["shapes"], 3)])
                e_f, e_c = float(np.abs(flat_f - flat_w).max()), float(np.abs(flat_c - flat_w).max())
                one_ulp = fr.ulp(np.abs(flat_w).max())
                print(f"MEASURED end to end {name} {lt} {kind}: fused {e_f:.3e}, composable {e_c:.3e}, 1 ulp {one_ulp:.3e}")
                assert e_f <= max(2 * e_c, one_ulp), (name, lt, kind, e_f, e_c, one_ulp)
    with pytest.raises(RuntimeError, match="fused"):
        fcos.prepare_targets(case["shapes"], case["strides"], [g.double() for g in gts], fused=True)
    over = fcos.prepare_targets([(4, 4, 4)], [4], [torch.from_numpy(fc.boxes(1, 1025, (16, 16, 16), hi=16, quant=0)).to(DEV)])
    assert over.labels_flat.shape == (64,) and over.labels_flat.is_cuda          # above the limit: the composable path


def split_levels(flat, shapes, B):
    """Level-first [T] or [T, 6] -> per level the head's layout [B, C, W*L*H] flattened per level as [B, C * P]."""
    out, first = [], 0
    for (w, l, h) in shapes:
        n = B * w * l * h
        part = flat[first:first + n]
        out.append(part.reshape(B, w * l * h, -1).transpose(0, 2, 1).reshape(B, -1))
        first += n
    return out
