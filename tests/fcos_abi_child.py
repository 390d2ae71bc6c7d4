"""Child process of tests/test_fcos_cpu.py: calls the FCOS exports of include/inr.h with every argument valid except the one
named and prints one JSON object {"<name>:<case>": [return code, message]}.  Every case either fails validation or has no
location (B = 0), so nothing is ever launched: the "device" pointers are host memory.  A crash ends the process without
the final line."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as probe  # noqa: E402

ADDR = probe.ADDR
SHAPES = [(24, 20, 12), (12, 10, 6), (6, 5, 3), (3, 3, 2)]


def i32(values):
    return (ctypes.c_int32 * len(values))(*values)


def host(arr):
    return ctypes.cast(arr, ctypes.c_void_p)


def pointers(n, addr=ADDR):
    return (ctypes.c_void_p * n)(*[addr + 256 * i for i in range(n)])


def pyramid(n):
    shapes = (SHAPES * 3)[:n]
    return (i32([v for s in shapes for v in s]), i32([4 * 2 ** (l % 4) for l in range(n)]),
            (ctypes.c_float * (2 * n))(*[float(v) for l in range(n) for v in (-1, 1e8)]))


DIMS, STRIDES, RANGES = pyramid(4)
PTRS = pointers(4)
KEEP = [DIMS, STRIDES, RANGES, PTRS]
COMMON = dict(level_dims=host(DIMS), n_levels=4, B=2, s=None)
VALID = {
    "inr_fcos_targets": dict(COMMON, level_strides=host(STRIDES), level_ranges=host(RANGES), max_gt=8, radius=1.5,
                             norm_reg_targets=1),
    "inr_fcos_loss_forward": dict(COMMON, cls_ptrs=host(PTRS), reg_ptrs=host(PTRS), ctr_ptrs=host(PTRS), iou_loss_type=0,
                                  workspace_bytes=1 << 16),
    "inr_fcos_loss_backward": dict(COMMON, cls_ptrs=host(PTRS), reg_ptrs=host(PTRS), ctr_ptrs=host(PTRS), iou_loss_type=2,
                                   d_cls_ptrs=host(PTRS), d_reg_ptrs=host(PTRS), d_ctr_ptrs=host(PTRS)),
}
REQUIRED = {
    "inr_fcos_targets": ("level_dims", "level_strides", "level_ranges", "gt", "gt_offsets", "labels", "reg_targets"),
    "inr_fcos_loss_forward": ("cls_ptrs", "reg_ptrs", "ctr_ptrs", "level_dims", "labels", "reg_targets", "sums", "losses",
                              "workspace"),
    "inr_fcos_loss_backward": ("cls_ptrs", "reg_ptrs", "ctr_ptrs", "level_dims", "labels", "reg_targets", "norms",
                               "grad_losses", "d_cls_ptrs", "d_reg_ptrs", "d_ctr_ptrs"),
}


def call(name, **over):
    """Pointers into the host buffer, the four-level pyramid, B = 2; `over` replaces arguments by the header's names."""
    return probe.call(name, probe.default_args(name), **dict(VALID[name], **over))


out = {}
for name in VALID:
    for arg in REQUIRED[name]:
        out[f"{name}:{arg}_null"] = call(name, **{arg: None})
    d9, s9, r9 = pyramid(9)
    nine = dict(level_dims=host(d9), n_levels=9)
    if name == "inr_fcos_targets":
        nine.update(level_strides=host(s9), level_ranges=host(r9))
    out[f"{name}:n_levels_9"] = call(name, **nine)
    out[f"{name}:n_levels_0"] = call(name, n_levels=0)
    out[f"{name}:B_negative"] = call(name, B=-1)
    bad = i32([24, 20, 12, 12, -10, 6, 6, 5, 3, 3, 3, 2])
    out[f"{name}:extent_negative"] = call(name, level_dims=host(bad))
    big = i32([800, 800, 800] + [1, 1, 1] * 3)
    ones = i32([1, 1, 1, 1])
    over = dict(level_dims=host(big))
    if name == "inr_fcos_targets":
        over.update(level_strides=host(ones))
    out[f"{name}:T_overflow"] = call(name, **over)
    out[f"{name}:labels_misaligned"] = call(name, labels=ctypes.c_void_p(ADDR + 2))
    arrays = [n for _, n in probe.prototypes()[name] if n not in VALID[name]]
    out[f"{name}:B_0"] = call(name, B=0)
    out[f"{name}:B_0_null_pointers"] = call(name, B=0, **{a: None for a in arrays})
    out[f"{name}:B_0_n_levels_9"] = call(name, B=0, **nine)
out["inr_fcos_targets:max_gt_1025"] = call("inr_fcos_targets", max_gt=1025)
out["inr_fcos_targets:max_gt_negative"] = call("inr_fcos_targets", max_gt=-1)
out["inr_fcos_targets:radius_negative"] = call("inr_fcos_targets", radius=-0.5)
out["inr_fcos_targets:stride_0"] = call("inr_fcos_targets", level_strides=host(i32([4, 0, 16, 32])))
out["inr_fcos_targets:valid_without_ori_sizes"] = call("inr_fcos_targets", ori_sizes=None)
out["inr_fcos_targets:max_gt_0_gt_null_B_0"] = call("inr_fcos_targets", max_gt=0, gt=None, B=0)
for name in ("inr_fcos_loss_forward", "inr_fcos_loss_backward"):
    out[f"{name}:iou_loss_type_7"] = call(name, iou_loss_type=7)
    out[f"{name}:iou_loss_type_negative"] = call(name, iou_loss_type=-1)
    holes = pointers(4)
    holes[2] = None
    out[f"{name}:level_pointer_null"] = call(name, reg_ptrs=host(holes))
    out[f"{name}:level_pointer_misaligned"] = call(name, ctr_ptrs=host(pointers(4, ADDR + 1)))
out["inr_fcos_loss_forward:workspace_too_small"] = call("inr_fcos_loss_forward", workspace_bytes=64)
out["inr_fcos_loss_forward:workspace_bytes_negative"] = call("inr_fcos_loss_forward", workspace_bytes=-8)
out["inr_fcos_loss_forward:sums_misaligned"] = call("inr_fcos_loss_forward", sums=ctypes.c_void_p(ADDR + 4))
out["inr_fcos_loss_backward:norms_misaligned"] = call("inr_fcos_loss_backward", norms=ctypes.c_void_p(ADDR + 4))
out["inr_fcos_loss_workspace_bytes:T_negative"] = probe.size_query("inr_fcos_loss_workspace_bytes", -1)
out["inr_fcos_loss_workspace_bytes:T_overflow"] = probe.size_query("inr_fcos_loss_workspace_bytes", (1 << 31) // 6 + 1)
out["inr_fcos_loss_workspace_bytes:T_0"] = probe.size_query("inr_fcos_loss_workspace_bytes", 0)
out["inr_fcos_loss_workspace_bytes:T_19764"] = probe.size_query("inr_fcos_loss_workspace_bytes", 19764)
probe.emit(out)
