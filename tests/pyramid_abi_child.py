"""Child process of tests/test_pyramid_pool_cpu.py: calls the two pyramid RoIAlign exports of include/inr.h with every
argument valid except the one named and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation
precedes every read of a host array and every launch, so this runs on a CPU-only box; a crash ends the process without
the final line."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import _lib  # noqa: E402

lib = _lib.load()
HOST = ctypes.create_string_buffer(1 << 16)
ADDR = (ctypes.addressof(HOST) + 255) // 256 * 256
N_LEVELS = 3
PTRS = (ctypes.c_void_p * 9)(*[ADDR] * 9)
DIMS = (ctypes.c_int32 * 27)(*[8] * 27)
SCALES = (ctypes.c_float * 9)(*[0.5] * 9)

# argument positions (include/inr.h; the same in both exports)
POS = dict(level_ptrs=0, level_dims=1, level_scales=2, n_levels=3, rois=4, roi_inds=5, roi_levels=6, order=7, N=8, C=9,
           K=10, out_w=11, out_l=12, out_h=13, io=14, stream=15)


def call(name, **over):
    p = ctypes.c_void_p(ADDR)
    args = [PTRS, DIMS, SCALES, N_LEVELS, p, p, p, None, 2, 4, 5, 3, 3, 3, p, None]
    for key, v in over.items():
        args[POS[key]] = v
    rc = int(getattr(lib, name)(*args))
    msg = lib.inr_last_error()
    return [rc, msg.decode() if msg else ""]


out = {}
for name in ("inr_roi_align_3d_pyramid_forward", "inr_roi_align_3d_pyramid_backward"):
    out[f"{name}:n_levels_0"] = call(name, n_levels=0)
    out[f"{name}:n_levels_9"] = call(name, n_levels=9)
    out[f"{name}:n_levels_9_null_table"] = call(name, n_levels=9, level_ptrs=None, level_dims=None, level_scales=None)
    out[f"{name}:zero_bins"] = call(name, out_l=0)
    out[f"{name}:K_negative"] = call(name, K=-1)
    out[f"{name}:C_zero"] = call(name, C=0)
    out[f"{name}:K_zero_null_ok"] = call(name, K=0, rois=None, roi_inds=None, roi_levels=None, io=None)
    out[f"{name}:rois_null"] = call(name, rois=None)
    out[f"{name}:roi_levels_null"] = call(name, roi_levels=None)
    out[f"{name}:level_dims_null"] = call(name, level_dims=None)
    bad_dims = (ctypes.c_int32 * 9)(8, 8, 8, 8, 0, 8, 8, 8, 8)
    out[f"{name}:level_dims_zero"] = call(name, level_dims=bad_dims)
null_entry = (ctypes.c_void_p * 3)(ADDR, None, ADDR)
out["inr_roi_align_3d_pyramid_forward:level_ptrs_null_entry"] = call("inr_roi_align_3d_pyramid_forward", level_ptrs=null_entry)
out["alive"] = [0, "reached the end"]
sys.stdout.write(json.dumps(out) + "\n")
