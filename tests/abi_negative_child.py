"""Child process of tests/test_abi_negative.py: calls EVERY export of include/inr.h with bad arguments and prints one
JSON object {"<name>:<variant>": [return code, message]}.  Runs on a CPU-only box: the library loads without a GPU, and
a call that validates its arguments never reaches a launch.  A crash (abort, segfault, exit()) ends this process without
the final line, which is what the parent asserts on."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as A  # noqa: E402
from instance_nerf_amd import _lib  # noqa: E402

ADDR = A.ADDR
out = {}
# ---- every export, two generic variants: null pointers with plausible sizes; valid (host) pointers with negative sizes
for name, (restype, argtypes) in _lib._SIGS.items():
    if name in ("inr_abi_version", "inr_last_error"):
        continue
    out[f"{name}:null"] = A.call(name, [None if A.is_pointer(t) else a for t, a in zip(argtypes, A.default_args(name))])
    out[f"{name}:negative"] = A.call(name, A.default_args(name, ints=-1))


# ---- targeted cases: everything valid except the one thing named
def call(name, **by_name):
    """All pointers -> the host buffer, sizes 16, floats 1; `by_name` replaces arguments by the header's names."""
    return A.call(name, A.default_args(name), **by_name)


desc17 = A.good_desc(levels=17)
desc_f4 = A.good_desc(level_dim=4)
ok_desc = A.good_desc()
for name in ("inr_grid_encode_forward", "inr_grid_encode_backward"):
    out[f"{name}:num_levels_17"] = call(name, desc=ctypes.byref(desc17))
    out[f"{name}:level_dim_4"] = call(name, desc=ctypes.byref(desc_f4))
out["inr_nerf_forward:num_levels_17"] = call("inr_nerf_forward", desc=ctypes.byref(desc17))
out["inr_instance_forward:num_levels_17"] = call("inr_instance_forward", desc=ctypes.byref(desc17))
# K > 64 / K not a multiple of 16 wherever an entry point takes the instance head's K
out["inr_instance_forward:K_65"] = call("inr_instance_forward", desc=ctypes.byref(ok_desc), K=65)
out["inr_instance_forward:K_80"] = call("inr_instance_forward", desc=ctypes.byref(ok_desc), K=80)
out["inr_instance_forward_enc:K_80"] = call("inr_instance_forward_enc", desc=ctypes.byref(ok_desc), K=80)
out["inr_instance_pack_weights:K_65"] = call("inr_instance_pack_weights", K=65)
out["inr_instance_pack_weights_device:K_80"] = call("inr_instance_pack_weights_device", K=80)
out["inr_instance_head_backward:K_80"] = call("inr_instance_head_backward", K=80)
out["inr_instance_render:K_80"] = call("inr_instance_render", desc=ctypes.byref(ok_desc), K=80)
# a numerics value the entry point does not take (TABLE_F16 alone: instance_render takes 0 or both bits)
out["inr_nerf_forward_table:numerics_4"] = call("inr_nerf_forward_table", desc=ctypes.byref(ok_desc), numerics=4)
out["inr_instance_render:numerics_1"] = call("inr_instance_render", desc=ctypes.byref(ok_desc), numerics=_lib.NUMERICS_TABLE_F16)
out["inr_cross_entropy:K_65"] = call("inr_cross_entropy", K=65)
out["inr_composite_rays_extra_forward:K_65"] = call("inr_composite_rays_extra_forward", K=65)
out["inr_instance_packed_floats:K_65"] = A.size_query("inr_instance_packed_floats", 65)
# misaligned buffers where the header asks for an alignment
out["inr_cross_entropy:acc_misaligned"] = call("inr_cross_entropy", acc=ctypes.c_void_p(ADDR + 4))
out["inr_sh_table_q:out_misaligned"] = call("inr_sh_table_q", out=ctypes.c_void_p(ADDR + 4))
out["inr_nerf_forward_dirs:out_misaligned"] = call("inr_nerf_forward_dirs", desc=ctypes.byref(ok_desc), n_dirs=4,
                                                   out=ctypes.c_void_p(ADDR + 4))
out["inr_copy_multi:n_9"] = call("inr_copy_multi", n=9)
out["inr_adam_step_multi:n_17"] = call("inr_adam_step_multi", n_tensors=17)
out["inr_finish_rays_mse:N_too_large"] = call("inr_finish_rays_mse", N=65537)
out["inr_sh_encode_forward:degree_5"] = call("inr_sh_encode_forward", degree=5)
out["inr_linear_wgrad:n_in_65"] = call("inr_linear_wgrad", n_in=65)
out["inr_sample_training_batch:channels_5"] = call("inr_sample_training_batch", channels=5)
out["inr_sample_training_batch:negative_step"] = call("inr_sample_training_batch", step=-1)
out["inr_sample_training_batch:image_too_large"] = call("inr_sample_training_batch", H=65536, W=65536)
out["inr_set_march_mode:mode_7"] = call("inr_set_march_mode", mode=7)
out["inr_roi_align_3d_set_mode:mode_9"] = call("inr_roi_align_3d_set_mode", mode=9)
out["inr_roi_align_3d_forward:zero_bins"] = call("inr_roi_align_3d_forward", out_w=0)
out["inr_roi_align_3d_backward_ws:workspace_too_small"] = call("inr_roi_align_3d_backward_ws", workspace_bytes=64)
out["inr_nerf_forward_table_sliced:12_levels"] = call("inr_nerf_forward_table_sliced", desc=ctypes.byref(A.good_desc(levels=12)))
# ---- a launch that cannot succeed (this box has no GPU; on a GPU box the parent skips this key): INR_ELAUNCH, not abort
out["inr_nerf_pack_weights_device:launch"] = call("inr_nerf_pack_weights_device")
A.emit(out)
