"""Child process of tests/test_ssim_cpu.py: calls the SSIM exports of include/inr.h with every argument valid except the one
named and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation precedes every launch, so this
runs on a CPU-only box; a crash ends the process without the final line."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as A  # noqa: E402
from instance_nerf_amd import _lib, metrics  # noqa: E402

lib = _lib.load()
ADDR = A.ADDR
WINDOW = metrics.gaussian_window()
NAN_WINDOW = WINDOW.copy()
NAN_WINDOW[3] = np.nan
SHAPE = dict(B=2, H=40, W=100, C=3)


def forward(**over):
    """All pointers into the host buffer, a valid shape and the workspace size the library asks for; `over` replaces
    arguments by name (shape arguments before the workspace size is taken, unless that is given too)."""
    shape = dict(SHAPE, **{k: v for k, v in over.items() if k in SHAPE})
    need = lib.inr_ssim_workspace_bytes(shape["B"], shape["H"], shape["W"], shape["C"])
    base = dict(shape, window11=WINDOW.ctypes.data_as(ctypes.c_void_p), workspace_bytes=max(int(need), 16), s=None)
    base.update({k: v(need) if callable(v) else v for k, v in over.items()})
    return A.call("inr_ssim_forward", A.default_args("inr_ssim_forward"), **base)


out = {}
out["inr_ssim_forward:C_5"] = forward(C=5)
out["inr_ssim_forward:C_0"] = forward(C=0)
out["inr_ssim_forward:H_10"] = forward(H=10)
out["inr_ssim_forward:W_10"] = forward(W=10)
out["inr_ssim_forward:B_0"] = forward(B=0)
out["inr_ssim_forward:too_large"] = forward(B=4, H=1 << 14, W=1 << 14, C=2)
out["inr_ssim_forward:workspace_one_byte_short"] = forward(workspace_bytes=lambda need: need - 1)
out["inr_ssim_forward:workspace_misaligned"] = forward(workspace=ctypes.c_void_p(ADDR + 4))
for label, name in (("pred", "pred"), ("workspace", "workspace"), ("window", "window11"), ("data_range", "data_range_dev"),
                    ("out_ssim", "out_ssim")):
    out[f"inr_ssim_forward:{label}_null"] = forward(**{name: None})
out["inr_ssim_forward:window_nan"] = forward(window11=NAN_WINDOW.ctypes.data_as(ctypes.c_void_p))
out["inr_ssim_workspace_bytes:C_5"] = A.size_query("inr_ssim_workspace_bytes", 1, 40, 40, 5)
out["inr_ssim_workspace_bytes:H_10"] = A.size_query("inr_ssim_workspace_bytes", 1, 10, 40, 3)
out["inr_ssim_workspace_bytes:W_negative"] = A.size_query("inr_ssim_workspace_bytes", 1, 40, -1, 3)
out["inr_ssim_workspace_bytes:too_large"] = A.size_query("inr_ssim_workspace_bytes", 4, 1 << 14, 1 << 14, 2)
for shape in ((1, 11, 11, 1), (3, 26, 74, 4), (1, 27, 75, 3), (8, 800, 800, 3)):
    out["size:" + "x".join(map(str, shape))] = int(lib.inr_ssim_workspace_bytes(*shape))
A.emit(out)
