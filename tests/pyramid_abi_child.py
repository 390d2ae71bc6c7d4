"""Child process of tests/test_pyramid_pool_cpu.py: calls the two pyramid RoIAlign exports of include/inr.h with every
argument valid except the one named and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation
precedes every read of a host array and every launch, so this runs on a CPU-only box; a crash ends the process without
the final line."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as A  # noqa: E402

ADDR = A.ADDR
N_LEVELS = 3
PTRS = (ctypes.c_void_p * 9)(*[ADDR] * 9)
DIMS = (ctypes.c_int32 * 27)(*[8] * 27)
SCALES = (ctypes.c_float * 9)(*[0.5] * 9)
# the per-level pointer table and the pooled tensor are named after the direction
FORWARD, BACKWARD = "inr_roi_align_3d_pyramid_forward", "inr_roi_align_3d_pyramid_backward"
TABLE, POOLED = {FORWARD: "level_ptrs", BACKWARD: "level_grads"}, {FORWARD: "out", BACKWARD: "grad_out"}


def call(name, table=PTRS, pooled=ctypes.c_void_p(ADDR), **over):
    p = ctypes.c_void_p(ADDR)
    base = dict(level_dims=DIMS, level_scales=SCALES, n_levels=N_LEVELS, rois=p, roi_inds=p, roi_levels=p, order=None, N=2, C=4,
                K=5, out_w=3, out_l=3, out_h=3, s=None)
    base.update({TABLE[name]: table, POOLED[name]: pooled}, **over)
    return A.call(name, A.default_args(name), **base)


out = {}
for name in (FORWARD, BACKWARD):
    out[f"{name}:n_levels_0"] = call(name, n_levels=0)
    out[f"{name}:n_levels_9"] = call(name, n_levels=9)
    out[f"{name}:n_levels_9_null_table"] = call(name, n_levels=9, table=None, level_dims=None, level_scales=None)
    out[f"{name}:zero_bins"] = call(name, out_l=0)
    out[f"{name}:K_negative"] = call(name, K=-1)
    out[f"{name}:C_zero"] = call(name, C=0)
    out[f"{name}:K_zero_null_ok"] = call(name, K=0, rois=None, roi_inds=None, roi_levels=None, pooled=None)
    out[f"{name}:rois_null"] = call(name, rois=None)
    out[f"{name}:roi_levels_null"] = call(name, roi_levels=None)
    out[f"{name}:level_dims_null"] = call(name, level_dims=None)
    bad_dims = (ctypes.c_int32 * 9)(8, 8, 8, 8, 0, 8, 8, 8, 8)
    out[f"{name}:level_dims_zero"] = call(name, level_dims=bad_dims)
null_entry = (ctypes.c_void_p * 3)(ADDR, None, ADDR)
out[f"{FORWARD}:level_ptrs_null_entry"] = call(FORWARD, table=null_entry)
A.emit(out)
