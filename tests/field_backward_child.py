"""Launches of the fused field's backward entry points through the C ABI for tests/test_field_backward_kernels.py, and,
run as a script, the whole exact tier and tolerance tier on the library that INR_LIB_PATH names (a process binds one
library): prints ``RESULT {"build": ..., "failures": [...], "ratios": {name: worst |got - ref| / cond}}``.

Every buffer a kernel writes is a guarded view pre-filled with the NaN sentinel (``Buf`` of kernel_harness); inputs
carry NaN guard words behind their last row; rows the instance launch must not read (m >= n, rays without a sample
below n) hold NaN.  Only NaN poisons: every index in sample_ray stays in range."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import field_backward_reference as R  # noqa: E402
from kernel_harness import Buf, check, cu_count, finish, nan_out, pack_instance_device, pack_nerf_device, stream  # noqa: E402
from train_kernels_reference import assert_same_bits  # noqa: E402

F32 = np.float32
NAN = np.float32(np.nan)


def zero_floats_for(i, M, cus):
    """The side zero-fill of launch number i: none, lengths with zero_floats % 4 = 0..3, one longer than a whole
    grid-stride trip (grid * 512 lanes * 4 floats)."""
    grid = max(1, min(-(-M // 128), cus))
    return (None, 4096, 1029, 2, 7, grid * 2048 + 4 * 77 + 1)[i % 6]


def _zero_buf(zero_floats):
    return None if zero_floats is None else nan_out(zero_floats)


def _finish(bufs, zbuf, what):
    """finish() of the harness, and the side buffer must hold zeros between intact guards."""
    got = finish(dict(bufs, zero_buf=zbuf), what)
    if zbuf is not None:
        assert_same_bits(got.pop("zero_buf"), np.zeros(zbuf.shape, F32), what + " zero_buf")
    return got


def run_nerf_head(lib, case, zero_floats=None, enc_dev=None):
    """inr_nerf_head_backward on ``case`` -> dict of numpy outputs (guards checked).  enc_dev: a device tensor to use
    instead of case["enc"]."""
    M = len(case["g_sigma"])
    pf, pb, keep = pack_nerf_device(lib, case["W"])
    enc = None if enc_dev is not None else Buf(np.asarray(case["enc"], F32))
    d, gs, gr = Buf(np.asarray(case["dirs"], F32)), Buf(np.asarray(case["g_sigma"], F32)), Buf(np.asarray(case["g_rgb"], F32))
    o = {"d_enc": nan_out(M, 32), "gws0": nan_out(64, 32), "gws1": nan_out(16, 64), "gwc0": nan_out(64, 31),
         "gwc1": nan_out(64, 64), "gwc2": nan_out(16, 64),
         "workspace": nan_out(lib.inr_instance_head_workspace_bytes() // 4)}
    z = _zero_buf(zero_floats)
    enc_ptr = enc.ptr if enc is not None else (enc_dev.data_ptr() if M else None)
    rc = lib.inr_nerf_head_backward(enc_ptr, d.ptr, gs.ptr, gr.ptr, M, float(case["density_scale"]), pf.ptr, pb.ptr,
                                    o["d_enc"].ptr, o["workspace"].ptr, o["gws0"].ptr, o["gws1"].ptr, o["gwc0"].ptr,
                                    o["gwc1"].ptr, o["gwc2"].ptr, None if z is None else z.ptr, zero_floats or 0, stream())
    check(rc, "nerf_head_backward")
    got = _finish(o, z, "nerf_head")
    del keep, got["workspace"]
    return got


def run_instance_head(lib, case, zero_floats=None, enc_dev=None):
    M, K, N = len(case["wbuf"]), case["K"], case["N"]
    n = R.instance_rows(case)
    pf, pb, keep = pack_instance_device(lib, case["W"], K)
    enc_h, wbuf, gp = np.array(case["enc"], F32), np.array(case["wbuf"], F32), np.array(case["g_pix"], F32)
    enc_h[n:], wbuf[n:] = NAN, NAN
    used = np.zeros(N, bool)
    used[np.asarray(case["sample_ray"])[:n]] = True
    gp[~used] = NAN
    enc = None if enc_dev is not None else Buf(enc_h)
    wb, ray, gpb = Buf(wbuf), Buf(np.asarray(case["sample_ray"], np.int32)), Buf(gp)
    n_dev = None if case["n"] is None else Buf(np.asarray([case["n"]], np.int32))
    sa = None if case["scale_a"] is None else Buf(np.asarray([case["scale_a"]], F32))
    sb = None if case["scale_b"] is None else Buf(np.asarray([case["scale_b"]], F32))
    o = {"d_enc": nan_out(M, 32), "gw0": nan_out(64, 32), "gw1": nan_out(64, 64), "gw2": nan_out(K, 64),
         "workspace": nan_out(lib.inr_instance_head_workspace_bytes() // 4)}
    z = _zero_buf(zero_floats)
    p = lambda b: None if b is None else b.ptr
    enc_ptr = enc.ptr if enc is not None else (enc_dev.data_ptr() if M else None)
    rc = lib.inr_instance_head_backward(enc_ptr, wb.ptr, ray.ptr, gpb.ptr, K, N, M, p(n_dev), p(sa), p(sb), pf.ptr, pb.ptr,
                                        o["d_enc"].ptr, o["workspace"].ptr, o["gw0"].ptr, o["gw1"].ptr, o["gw2"].ptr, p(z),
                                        zero_floats or 0, stream())
    check(rc, "instance_head_backward")
    got = _finish(o, z, "instance_head")
    del keep, got["workspace"]
    return got


def run_nerf_chain(lib, case, saved):
    M = len(case["g_sigma"])
    pf, pb, keep = pack_nerf_device(lib, case["W"])
    gs, gr = Buf(np.asarray(case["g_sigma"], F32)), Buf(np.asarray(case["g_rgb"], F32))
    s = {k: Buf(np.asarray(saved[k], F32)) for k in ("rgb", "so", "h1", "c1", "c2")}
    o = {"d_o": nan_out(M, 4), "dz_c2": nan_out(M, 64), "dz_c1": nan_out(M, 64), "d_so": nan_out(M, 16), "dz_h1": nan_out(M, 64),
         "d_enc": nan_out(M, 32)}
    check(lib.inr_nerf_backward(gs.ptr, gr.ptr, s["rgb"].ptr, s["so"].ptr, s["h1"].ptr, s["c1"].ptr, s["c2"].ptr, M,
                                float(case["density_scale"]), pb.ptr, o["d_o"].ptr, o["dz_c2"].ptr, o["dz_c1"].ptr,
                                o["d_so"].ptr, o["dz_h1"].ptr, o["d_enc"].ptr, stream()), "nerf_backward")
    got = finish(o, "nerf_chain")
    del keep, pf
    return got


def run_instance_chain(lib, case, saved):
    M, K = len(saved["g"]), case["K"]
    pf, pb, keep = pack_instance_device(lib, case["W"], K)
    g, h1, h2 = (Buf(np.asarray(saved[k], F32)) for k in ("g", "h1", "h2"))
    o = {"dz2": nan_out(M, 64), "dz1": nan_out(M, 64), "denc": nan_out(M, 32)}
    check(lib.inr_instance_backward(g.ptr, K, h1.ptr, h2.ptr, M, pb.ptr, o["dz2"].ptr, o["dz1"].ptr, o["denc"].ptr,
                                    stream()), "instance_backward")
    got = finish(o, "instance_chain")
    del keep, pf
    return got


def compare(prefix, case, size, got, ref, cond, build, ratios):
    """Exact tier: ``got`` equals ``ref`` rounded to fp32 bit for bit (gwc0 without its SH columns).  Tolerance tier:
    |got - ref| <= TOL * cond elementwise.  The worst |got - ref| / cond per output goes into ``ratios`` first."""
    fails = []
    for k in ref:
        name = f"{prefix}.{k}"
        if case["tier"] == "exact":
            g, r = got[k], ref[k].astype(F32)
            if k == "gwc0":
                g, r = g[:, 16:], r[:, 16:]
            try:
                assert_same_bits(g, r, name)
            except AssertionError as e:
                fails.append(str(e))
        else:
            w = R.worst_ratio(got[k], ref[k], cond[k])
            tol = R.tolerance(build, name, size)
            key = name + ("@big" if size in R.BIG_SIZES else "")
            ratios[key] = max(ratios.get(key, 0.0), w)
            print(f"{key}: worst |got - ref| / cond {w:.3e}  (TOL {tol:.3e})")
            if not w <= tol:
                fails.append(f"{key}: {w:.3e} > {tol:.3e}")
    return fails


def head_case(lib, cid, i, size, case, cus, build, ratios):
    M = len(case["enc"])
    z = zero_floats_for(i, M, cus)
    if case["kind"] == "nerf":
        got, (ref, cond) = run_nerf_head(lib, case, z), R.nerf_head(R.Exact64(), case, cus)[:2]
    else:
        got, (ref, cond) = run_instance_head(lib, case, z), R.instance_head(R.Exact64(), case, cus)[:2]
    return [f"{cid}: {f}" for f in compare(case["kind"] + "_head", case, size, got, ref, cond, build, ratios)]


def chain_case(lib, cid, size, case, build, ratios):
    saved = R.chain_inputs(case)
    got = (run_nerf_chain if case["kind"] == "nerf" else run_instance_chain)(lib, case, saved)
    ref, cond = R.chain_reference(R.Exact64(), case, saved)
    return [f"{cid}: {f}" for f in compare(case["kind"] + "_chain", case, size, got, ref, cond, build, ratios)]


def sized(cases, specs, size_at):
    return [(cid, spec[size_at], make) for (cid, make), spec in zip(cases, specs)]


def all_cases():
    return sized(R.nerf_cases(), R._nerf_specs(), 3) + sized(R.instance_cases(), R._instance_specs(), 2)


def main():
    from instance_nerf_amd import _lib
    lib = _lib.load()
    cus = cu_count(lib)
    build = os.environ.get("FIELD_BACKWARD_BUILD", "fp32")
    ratios, fails = {}, []
    for i, (cid, size, make) in enumerate(all_cases()):
        case = make(cus)
        fails += head_case(lib, cid, i, size, case, cus, build, ratios)
        if R.chain_applies(size):
            fails += chain_case(lib, cid, size, case, build, ratios)
    print("RESULT " + json.dumps({"build": build, "failures": fails, "ratios": ratios}))


if __name__ == "__main__":
    main()
