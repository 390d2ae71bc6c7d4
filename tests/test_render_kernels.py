"""inr_nerf_render and inr_instance_render (k_nerf_render, k_instance_render of csrc/field_fused.hip) on the GPU against
tests/render_reference.py, through the C ABI on plain device buffers with guard words (tests/render_child.py).  Exact
tier: bit equality with the float64 result rounded to fp32 - placement (patch slot of every (ray, step)), termination,
zero fill, ``evaluated``, dropped groups, rows that must never be read, and the GroupDraw schedule with 1, 8 and 32
owners against NaN-prefilled outputs.  Tolerance tier: |got - ref| <= TOL * cond elementwise, default and -O numerics,
and the chain inr_nerf_render -> inr_instance_render the renderer runs.  N == 0, M == 0; the fp32 library through a
child."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_forward_child as L  # noqa: E402
import render_child as H  # noqa: E402
import render_reference as X  # noqa: E402
from kernel_harness import cu_count, nan_out, poisoned, run_result_child, stream  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
BUILD = "bf16x3"
TOL_ROWS = [(n, num) for n in X.TOL_CASES for num in ("", "o")]


@pytest.fixture(scope="module")
def lib():
    from instance_nerf_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("num", ["", "o"])
def test_nerf_render_exact(lib, num):
    """COUNTS x TERMINATION: every output bit, with ``weights`` given and null and on both feeds.  Under -O too: so0 and
    the colour logits cancel exactly whatever the operand format, so sigma and rgb stay 0.5."""
    fails, _ = H.run_nerf_case(lib, X.exact_case(), BUILD, num, {})
    assert not fails, fails


def test_threshold_is_strict(lib):
    """T_thresh == 1: T == T_thresh at every boundary of a transparent prefix, and the ray goes on (T < T_thresh)."""
    fails, _ = H.run_nerf_case(lib, X.strict_case(), BUILD, "", {})
    assert not fails, fails


@pytest.mark.parametrize("name,num", TOL_ROWS, ids=[f"{n}{'-O' if num else ''}" for n, num in TOL_ROWS])
def test_nerf_render_tolerance(lib, name, num):
    fails, _ = H.run_nerf_case(lib, X.tol_case(name), BUILD, num, {})
    assert not fails, fails


@pytest.mark.parametrize("K", X.KS)
def test_instance_render_exact(lib, K):
    """w from {0, 1, 2, 0.5, -1}, a group whose steps from ZERO_FROM on are all zero: every product and sum exact."""
    fails = H.run_instance_case(lib, X.exact_case(), K, BUILD, "", {})
    assert not fails, fails


@pytest.mark.parametrize("name,num", TOL_ROWS, ids=[f"{n}{'-O' if num else ''}" for n, num in TOL_ROWS])
def test_instance_render_tolerance(lib, name, num):
    fails = []
    for K in X.KS:
        fails += H.run_instance_case(lib, X.tol_case(name), K, BUILD, num, {})
    assert not fails, fails


@pytest.mark.parametrize("name", list(X.TOL_CASES))
def test_chained_weights_into_instance_render(lib, name):
    """The ``weights`` inr_nerf_render wrote, fed to inr_instance_render as renderer.py does, against the float64
    end-to-end value under the summed tolerance TOL[weights] sum cond(w) |logits| + TOL[extra] sum |w| cond(logits)."""
    case, K = X.tol_case(name), 32
    ref = X.nerf_render_ref(case)
    a = H.launch_nerf(lib, case)
    got = H.launch_instance(lib, case, K, a["weights"])
    scale = X.TOL[BUILD]["weights"] / X.TOL[BUILD]["extra"]
    want, cond = X.instance_render_ref(case, K, ref["weights"][case["slots"]], cw=scale * ref["cond"]["weights"][case["slots"]])
    fails = H.compare_instance(f"{name}/chained{K}", case, got, want, cond, BUILD, "", {})
    assert not fails, fails


@pytest.mark.parametrize("N", X.SCHEDULE_N)
def test_nerf_render_schedule(lib, N):
    """Every group drawn exactly once whatever the number of owners: NaN-prefilled outputs, every bit equal."""
    case = X.schedule_case(N)
    grid, n_owner = X.render_grid(N, cu_count(lib), "nerf")
    print(f"N {N}: {-(-N // 16)} groups, {grid} workgroups, {n_owner} owners, {-(-N // 16 // 64)} chunks")
    fails = H.compare_exact(case["name"], H.launch_nerf(lib, case), X.nerf_render_ref(case))
    assert not fails, fails


@pytest.mark.parametrize("N", X.SCHEDULE_N_INSTANCE)
def test_instance_render_schedule(lib, N):
    case, K = X.schedule_case(N), 16
    grid, n_owner = X.render_grid(N, cu_count(lib), "instance")
    print(f"N {N}: {-(-N // 16)} groups, {grid} workgroups, {n_owner} owners, {-(-N // 16 // 64)} chunks")
    w_patch, w = X.instance_inputs(case, K)
    want, _ = X.instance_render_ref(case, K, w)
    fails = H._bits(case["name"], H.launch_instance(lib, case, K, w_patch), want)
    assert not fails, fails


@pytest.mark.parametrize("where", ["last", "middle"])
def test_dropped_groups(lib, where):
    """M cut inside the last / the middle group: the rays of the groups that no longer fit give zeros, their ``weights``
    rows and every row from the cut on keep the NaN pattern, ``evaluated`` counts nothing of them, every other group is
    unchanged - in both kernels."""
    case = X.exact_case()
    M = X.cut_M(case, where)
    ref = X.nerf_render_ref(case, M)
    assert ref["dropped"].any() and not ref["dropped"].all()
    fails = H.compare_exact(f"cut {where}", H.launch_nerf(lib, case, M=M), ref)
    fails += H.same_outputs(f"cut {where} without weights", H.launch_nerf(lib, case, M=M, weights=False),
                            dict(ref, **{k: ref[k].astype(F32) for k in ("weights_sum", "depth", "image")}))
    for K in (16, 64):
        w_patch, w = X.instance_inputs(case, K)
        want, _ = X.instance_render_ref(case, K, w, M=M)
        assert not want[case["rays"][ref["dropped"], 0]].any()
        fails += H._bits(f"cut {where} instance{K}", H.launch_instance(lib, case, K, w_patch, M=M), want)
    assert not fails, fails


def test_rows_behind_the_termination_point_are_never_read(lib):
    """NaN in deltas and positions strictly behind every opaque sample: no output bit changes (render_reference.py
    spells out the rows).  inr_nerf_render only: inr_instance_render reads the position of every sample of a step it
    evaluates, zero weight or not, and 0 * NaN is NaN - its positions come from the marcher and are always finite."""
    case, poisoned = X.exact_case(), X.never_read_case()
    ref = X.nerf_render_ref(case)
    fails = []
    for x_is_01 in (0, 1):
        got = H.launch_nerf(lib, poisoned, x_is_01=x_is_01)
        fails += H.compare_exact(f"never read, x_is_01 {x_is_01}", got, ref)
        fails += H.same_outputs("never read without weights", H.launch_nerf(lib, poisoned, weights=False, x_is_01=x_is_01), got)
    assert not fails, fails


def test_no_rays_writes_nothing(lib):
    """N == 0: INR_OK with every array null but one poisoned output, which stays poisoned."""
    D = L.dev(X.EXACT_TABLE)
    out = nan_out(64)
    p = out.ptr
    rcs = [lib.inr_nerf_render(None, None, None, None, 0, 0, 1.0, D.emb[0].ptr, D.desc, None, 1.0, 1e-4, p, p, p, p, None,
                               0, 0, stream()),
           lib.inr_instance_render(None, None, None, 0, 0, 1.0, D.emb[0].ptr, D.desc, None, 16, p, 0, None, 0, stream())]
    L._sync()
    assert rcs == [0, 0], rcs
    assert poisoned(out.get()).all()
    out.check_guards("N == 0")


def test_no_samples_gives_zeros(lib):
    """M == 0 with N == 37 (every count 0, null sample arrays): all outputs zero, evaluated 0."""
    rng = X._rng("render_M0")
    case = X.constant_case("M0", rng, np.zeros(37, np.int64), np.full(37, -1))
    got = H.launch_nerf(lib, case)
    for k in ("weights_sum", "depth", "image"):
        assert not got[k].view(np.uint32).any(), k
    assert got["evaluated"] == 0 and got["weights"].size == 0
    out = H.launch_instance(lib, case, 48, np.zeros(0, F32))
    assert not out.view(np.uint32).any()


def test_fp32_library_both_tiers():
    """The -DINR_MLP_FP32=1 library (a process binds one library: a child with INR_LIB_PATH) on the exact case and the
    tolerance cases, both kernels, every K."""
    from instance_nerf_amd import build
    assert os.path.exists(build.LIB_FP32), "libinr_hip_fp32.so is built by __graft_entry__.build()"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "render_child.py")
    res = run_result_child(child, dict(INR_LIB_PATH=build.LIB_FP32, RENDER_BUILD="fp32"), timeout=300)
    print("fp32 library, worst |got - ref| / cond:", res["ratios"])
    assert res["build"] == "fp32" and set(res["ratios"]) == set(X.TOL["fp32"])
    assert not res["failures"], res["failures"][:10]
