"""Launches of inr_nerf_render and inr_instance_render through the C ABI for tests/test_render_kernels.py, on plain
device buffers with guard words (``Buf`` of kernel_harness; every output pre-filled with the NaN sentinel), and the
comparisons with tests/render_reference.py.  Run as a script: both tiers at the small sizes on the library that
INR_LIB_PATH names (a process binds one library); prints ``RESULT {"build": ..., "failures": [...], "ratios": {...}}``."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import composite_reference as C  # noqa: E402
import field_forward_child as L  # noqa: E402
import field_forward_reference as R  # noqa: E402
import render_reference as X  # noqa: E402
from kernel_harness import Buf, finish, nan_out, poisoned, stream  # noqa: E402
from train_kernels_reference import bit_mismatches  # noqa: E402

F32 = np.float32
N_CURSORS = 32                               # GroupDraw: at most 8 XCDs x 4 pools


def _total(case):
    return int(case["rays"][:, 2].sum())


def _positions(case, x_is_01):
    a = case["x01"] if x_is_01 else case["x"]
    if x_is_01 and case.get("poisoned"):
        a = np.where(np.isnan(case["x"]), np.nan, a).astype(F32)
    return Buf(C.to_patch(a, case["slots"], _total(case)))


def launch_nerf(lib, case, M=None, numerics=0, weights=True, x_is_01=0):
    """One inr_nerf_render launch on ``case`` with ``M`` rows (the buffers always hold every row) -> dict(weights_sum,
    depth, image, weights | None, evaluated)."""
    rays = case["rays"]
    N, total = len(rays), _total(case)
    M = total if M is None else int(M)
    D = L.dev(case["table"])
    W = R.nerf_weights(case["table"], case.get("variant"))
    packed = L.pack_nerf(lib, W, numerics)
    xb, db = _positions(case, x_is_01), Buf(C.to_patch(case["deltas"], case["slots"], total))
    rb, rdb = Buf(rays), Buf(case["rays_d"])
    o = {"weights_sum": nan_out(N), "depth": nan_out(N), "image": nan_out(N, 3)}
    if weights:
        o["weights"] = nan_out(total)
    ev = Buf(np.zeros(2 * (1 + N_CURSORS), np.int32))
    rc = lib.inr_nerf_render(xb.ptr, db.ptr, rb.ptr, rdb.ptr, N, M, case["bound"], D.emb[numerics & 1].ptr, D.desc,
                             packed.ptr, case["ds"], case["T"], o["weights_sum"].ptr, o["depth"].ptr, o["image"].ptr,
                             o["weights"].ptr if weights else None, ev.ptr, x_is_01, numerics, stream())
    assert rc == 0, rc
    got = finish(dict(o, evaluated=ev), "nerf_render")
    got["evaluated"] = int(got["evaluated"].view(np.uint64)[0])
    return got


def launch_instance(lib, case, K, w_patch, M=None, numerics=0, x_is_01=0):
    """One inr_instance_render launch -> out [N,K]."""
    rays = case["rays"]
    N, total = len(rays), _total(case)
    M = total if M is None else int(M)
    D = L.dev(case["table"])
    packed = L.pack_instance(lib, R.instance_weights(case["table"], K), K, numerics=numerics & 2)
    xb, wb, rb = _positions(case, x_is_01), Buf(np.asarray(w_patch, F32)), Buf(rays)
    out, cur = nan_out(N, K), Buf(np.zeros(2 * N_CURSORS, np.int32))
    rc = lib.inr_instance_render(xb.ptr, rb.ptr, wb.ptr, N, M, case["bound"], D.emb[numerics & 1].ptr, D.desc, packed.ptr,
                                 K, out.ptr, x_is_01, cur.ptr, numerics, stream())
    assert rc == 0, rc
    return finish({"out": out, "cursors": cur}, "instance_render")["out"]


def _bits(name, got, want):
    want = (np.asarray(want) + 0.0).astype(F32)
    got = np.ascontiguousarray(got, F32)
    n = bit_mismatches(got, want)
    if not n:
        return []
    i = int(np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())[0])
    return [f"{name}: {n} of {want.size} elements differ in their bits, first at flat index {i}: "
            f"{got.ravel()[i]!r} != {want.ravel()[i]!r}"]


def compare_exact(name, got, ref):
    """Bit equality of every output with the float64 reference rounded to fp32; rows of ``weights`` that no kernel
    writes (dropped groups, everything from the cut on) keep the NaN pattern; evaluated equal."""
    fails = []
    for k in ("weights_sum", "depth", "image"):
        fails += _bits(f"{name}.{k}", got[k], ref[k])
    if got.get("weights") is not None:
        wr = ref["written"]
        fails += _bits(f"{name}.weights", got["weights"][wr], ref["weights"][wr])
        if not poisoned(got["weights"][~wr]).all():
            fails.append(f"{name}.weights: a row of a dropped group or beyond M was written")
    if got["evaluated"] != ref["evaluated"]:
        fails.append(f"{name}.evaluated: {got['evaluated']} != {ref['evaluated']}")
    return fails


def compare_tol(name, case, got, ref, build, num, ratios):
    """|got - ref| <= TOL * cond elementwise; a ray inside the ambiguity band may match the alternative instead (all
    its outputs, one choice); evaluated exact without such a ray, else between the alternatives."""
    rays = case["rays"].astype(np.int64)
    flips = X.ambiguous_rays(case, ref, X.BAND[build][num])
    alts = [ref]
    if flips:
        a = X.alternative(case, ref, flips)
        alts.append(dict(a["out"], cond=a["cond"], evaluated=a["evaluated"]))
    row_of_slot = np.zeros(_total(case), np.int64)
    row_of_slot[case["slots"]] = X.sample_rows(rays)[0]
    fails = []
    bad = [np.zeros(len(rays), bool) for _ in alts]            # per alternative: rays with an output out of tolerance
    for k in X.OUTPUTS:
        if got.get(k) is None:
            continue
        key = X.tol_key(k, num)
        tol = X.TOL[build][key]
        g = np.asarray(got[k], np.float64)
        if not np.isfinite(g).all():
            fails.append(f"{name}.{k}: not finite")
            continue
        for i, alt in enumerate(alts):
            c = alt["cond"][k]
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(c > 0, np.abs(g - alt[k]) / c, np.where(g == 0, 0.0, np.inf))
            if k == "weights":
                per_ray = np.zeros(len(rays))
                np.maximum.at(per_ray, row_of_slot, ratio)
            else:
                per_ray = np.zeros(len(rays))
                per_ray[:] = (ratio if ratio.ndim == 1 else ratio.max(1))[rays[:, 0]]
            bad[i] |= per_ray > tol
            if i == 0:
                clear = np.asarray([n not in flips for n in range(len(rays))])
                r = float(per_ray[clear].max(initial=0.0))
                ratios[key] = max(ratios.get(key, 0.0), r)
                print(f"{name}.{k}: worst |got - ref| / cond {r:.3e}  (TOL[{key}] {tol:.3e}, {r / tol:.3f} of it)")
    for n in range(len(rays)):
        if bad[0][n] and (n not in flips or bad[1][n]):
            fails.append(f"{name}: ray row {n} (count {rays[n, 2]}) out of tolerance")
    ev = sorted(a["evaluated"] for a in alts)
    if not ev[0] <= got["evaluated"] <= ev[-1]:
        fails.append(f"{name}.evaluated: {got['evaluated']} not in {ev}")
    return fails


def compare_instance(name, case, got, want, cond, build, num, ratios, key="extra"):
    if case["tier"] == "exact":
        return _bits(name, got, want)
    k = X.tol_key(key, num)
    r, tol = X.worst_ratio(got, want, cond), X.TOL[build][k]
    ratios[k] = max(ratios.get(k, 0.0), r)
    print(f"{name}: worst |got - ref| / cond {r:.3e}  (TOL[{k}] {tol:.3e}, {r / tol:.3f} of it)")
    return [] if r <= tol else [f"{name}: {r:.3e} > {tol:.3e}"]


def same_outputs(name, a, b):
    """Two launches that must agree bit for bit in weights_sum, depth, image and evaluated."""
    fails = []
    for k in ("weights_sum", "depth", "image"):
        fails += _bits(f"{name}.{k}", a[k], b[k].astype(np.float64))
    if a["evaluated"] != b["evaluated"]:
        fails.append(f"{name}.evaluated: {a['evaluated']} != {b['evaluated']}")
    return fails


def run_nerf_case(lib, case, build, num, ratios, ref=None):
    """weights given and null (the other outputs and evaluated equal between the two launches), and the normalised feed
    against the plain one -> failures."""
    ref = ref or X.nerf_render_ref(case)
    numerics = X.NUMERICS[num]
    name = f"{case['name']}/nerf_render{'@' + num if num else ''}"
    a = launch_nerf(lib, case, numerics=numerics)
    b = launch_nerf(lib, case, numerics=numerics, weights=False)
    c = launch_nerf(lib, case, numerics=numerics, x_is_01=1)
    fails = compare_exact(name, a, ref) if case["tier"] == "exact" else compare_tol(name, case, a, ref, build, num, ratios)
    fails += same_outputs(name + " without weights", b, a)
    fails += same_outputs(name + " x_is_01", c, a) + _bits(name + " x_is_01.weights", c["weights"], a["weights"].astype(np.float64))
    return fails, a


def run_instance_case(lib, case, K, build, num, ratios):
    w_patch, w = X.instance_inputs(case, K)
    want, cond = X.instance_render_ref(case, K, w)
    name = f"{case['name']}/instance_render{K}{'@' + num if num else ''}"
    got = launch_instance(lib, case, K, w_patch, numerics=X.NUMERICS[num])
    got01 = launch_instance(lib, case, K, w_patch, numerics=X.NUMERICS[num], x_is_01=1)
    return compare_instance(name, case, got, want, cond, build, num, ratios) + _bits(name + " x_is_01", got01, got.astype(np.float64))


def main():
    from instance_nerf_amd import _lib
    lib = _lib.load()
    build = os.environ.get("RENDER_BUILD", "fp32")
    ratios, fails = {}, []
    for case in [X.exact_case()] + [X.tol_case(n) for n in X.TOL_CASES]:
        fails += run_nerf_case(lib, case, build, "", ratios)[0]
        for K in X.KS:
            fails += run_instance_case(lib, case, K, build, "", ratios)
    print("RESULT " + json.dumps({"build": build, "failures": fails, "ratios": ratios}))


if __name__ == "__main__":
    main()
