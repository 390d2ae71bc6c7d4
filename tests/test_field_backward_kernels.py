"""The fused field's training backward on the GPU against tests/field_backward_reference.py: inr_nerf_head_backward
(k_nerf_head_bwd + k_nerf_head_wgrad_reduce), inr_instance_head_backward (k_instance_head_bwd + k_head_wgrad_reduce)
and the chain kernels behind inr_nerf_backward / inr_instance_backward, called through the C ABI with device-packed
weights.  Exact tier: bit equality with the float64 result rounded to fp32.  Tolerance tier: |got - ref| <= TOL * cond
elementwise.  Sizes come from the device's CU count (one workgroup ... three rounds, see the reference); K = 16 .. 64,
density_scale 1 and 0.5, the two device scalars null and given, n_dev null / M - 37 / 0 / above M, rays without
samples, unsorted sample_ray, the side zero-fill null and with zero_floats % 4 = 0 .. 3 and longer than one grid trip.
Guards and NaN poisons: tests/field_backward_child.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_backward_child as L  # noqa: E402
import field_backward_reference as R  # noqa: E402
from kernel_harness import check, cu_count, pack_instance_device, pack_nerf_device, run_result_child, stream  # noqa: E402
from train_kernels_reference import assert_same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = L.all_cases()
IDS = [("nerf-" if i < len(R.nerf_cases()) else "instance-") + c[0] for i, c in enumerate(CASES)]


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cus(lib):
    n = cu_count(lib)
    assert n == lib.inr_instance_head_workspace_bytes() // (40 * 64 * 16)
    return n


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_head_backward(lib, cus, i):
    """One launch of inr_nerf_head_backward / inr_instance_head_backward per case of the reference's lists (M = 0 among
    them: return code 0, every weight gradient exactly zero, the side buffer zeroed)."""
    cid, size, make = CASES[i]
    fails = L.head_case(lib, cid, i, size, make(cus), cus, "bf16x3", {})
    assert not fails, fails


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if R.chain_applies(c[1])],
                         ids=[IDS[i] for i, c in enumerate(CASES) if R.chain_applies(c[1])])
def test_chain_backward(lib, cus, i):
    """inr_nerf_backward / inr_instance_backward: every intermediate output, both tiers, at the single-workgroup sizes
    and 16R + 1; saved activations from the float64 forward rounded to fp32."""
    cid, size, make = CASES[i]
    fails = L.chain_case(lib, cid, size, make(cus), "bf16x3", {})
    assert not fails, fails


def test_empty_batch_with_null_sample_arrays(lib):
    """M == 0 with every sample array null: return code 0, weight gradients exactly zero, zero_buf zeroed."""
    for make, run, names in ((lambda: R.nerf_exact_case(0), L.run_nerf_head, ("gws0", "gws1", "gwc0", "gwc1", "gwc2")),
                             (lambda: R.instance_exact_case(0, 48), L.run_instance_head, ("gw0", "gw1", "gw2"))):
        got = run(lib, make(), zero_floats=4099)
        for k in names:
            assert_same_bits(got[k], np.zeros(got[k].shape, F32), k)
        assert got["d_enc"].shape == (0, 32)


def _g(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(F32)).cuda()


@pytest.mark.parametrize("table", ["bench", "levels5"])
def test_nerf_head_masks_are_the_forwards(lib, table):
    """Unfiltered random x through a real table: d_enc of inr_nerf_head_backward, fed with the enc of
    inr_nerf_forward_train, equals bit for bit the d_enc of inr_nerf_backward on that launch's saved activations (the
    same operations on the same values)."""
    import field_issue_cases as C
    st, M = C.state(table), C.BIG
    x, d = C._dev(C.points(table, M, False)), C._dev(C.dirs_for(table, M))
    E = lambda w: torch.zeros(M, w, device="cuda")
    sigma, rgb, enc, h1, so, cin, c1, c2 = torch.zeros(M, device="cuda"), E(3), E(32), E(64), E(16), E(32), E(64), E(64)
    pf, pb, keep = pack_nerf_device(lib, st.nerf_w)
    p = lambda t: t.data_ptr()
    check(lib.inr_nerf_forward_train(p(x), p(d), M, 1.0, p(st.emb), st.desc, pf.ptr, p(sigma), p(rgb), p(enc), p(h1), p(so),
                                     p(cin), p(c1), p(c2), stream()), "forward_train")
    torch.cuda.synchronize()
    case = dict(kind="nerf", W=st.nerf_w, dirs=d.cpu().numpy(), g_sigma=_g(1, M).cpu().numpy(),
                g_rgb=_g(2, M, 3).cpu().numpy(), density_scale=1.0)
    head = L.run_nerf_head(lib, case, enc_dev=enc)
    saved = {k: v.cpu().numpy() for k, v in (("rgb", rgb), ("so", so), ("h1", h1), ("c1", c1), ("c2", c2))}
    chain = L.run_nerf_chain(lib, case, saved)
    assert np.isfinite(head["d_enc"]).all() and np.abs(head["d_enc"]).max() > 0
    assert_same_bits(head["d_enc"], chain["d_enc"], f"{table}: head d_enc against chain d_enc")


@pytest.mark.parametrize("table,K", [("bench", 48), ("levels5", 16)])
def test_instance_head_masks_are_the_forwards(lib, table, K):
    """The same for the instance pair, with wbuf = 1 and one ray per sample."""
    import field_issue_cases as C
    st, M = C.state(table), C.BIG
    rng = np.random.default_rng(7)
    W = [R._u(rng, (64, 32), 0.35), R._u(rng, (64, 64), 0.25), R._u(rng, (K, 64), 0.25)]
    x = C._dev(C.points(table, M, False))
    logits, enc, h1, h2 = (torch.zeros(M, w, device="cuda") for w in (K, 32, 64, 64))
    pf, pb, keep = pack_instance_device(lib, W, K)
    p = lambda t: t.data_ptr()
    check(lib.inr_instance_forward_train(p(x), M, 1.0, p(st.emb), st.desc, pf.ptr, K, p(logits), p(enc), p(h1), p(h2),
                                         stream()), "forward_train")
    torch.cuda.synchronize()
    g = _g(3, M, K).cpu().numpy()
    case = dict(kind="instance", K=K, W=W, N=M, wbuf=np.ones(M, F32), sample_ray=np.arange(M, dtype=np.int32), g_pix=g,
                scale_a=None, scale_b=None, n=None, enc=np.zeros((M, 32), F32))
    head = L.run_instance_head(lib, case, enc_dev=enc)
    chain = L.run_instance_chain(lib, case, {"g": g, "h1": h1.cpu().numpy(), "h2": h2.cpu().numpy()})
    assert np.isfinite(head["d_enc"]).all() and np.abs(head["d_enc"]).max() > 0
    assert_same_bits(head["d_enc"], chain["denc"], f"{table}: head d_enc against chain denc")


def test_fp32_library_both_tiers():
    """The -DINR_MLP_FP32=1 library (a process binds one library: a child with INR_LIB_PATH) runs the same exact tier
    and its own tolerance tier."""
    from instance_nerf_amd import build
    assert os.path.exists(build.LIB_FP32), "libinr_hip_fp32.so is built by __graft_entry__.build()"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "field_backward_child.py")
    res = run_result_child(child, dict(INR_LIB_PATH=build.LIB_FP32, FIELD_BACKWARD_BUILD="fp32"), timeout=600)
    print("fp32 library, worst |got - ref| / cond:", res["ratios"])
    assert res["build"] == "fp32" and {k.split("@")[0] for k in res["ratios"]} == set(R.TOL["fp32"])
    assert not res["failures"], res["failures"][:10]
