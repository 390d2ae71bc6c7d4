"""Child process of tests/test_mesh_cpu.py: calls the three mesh exports of include/inr.h with every argument valid except
the one named limit and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation precedes every
launch, so this runs on a CPU-only box; a crash ends the process without the final line."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as A  # noqa: E402
from instance_nerf_amd import _lib  # noqa: E402

lib = _lib.load()
ADDR = A.ADDR
W = L = H = 4
WS = int(lib.inr_mesh_workspace_bytes(W, L, H, 1))
assert 0 < WS < (1 << 15)


def call(name, **over):
    base = dict(field_stride=1, select=-1, W=W, L=L, H=H, cap=1, workspace_bytes=WS)
    if name == "inr_mesh_emit":
        base.update(V=8, F=8)
    return A.call(name, A.default_args(name, ints=1), **dict(base, **over))


out = {}
for name in ("inr_mesh_count", "inr_mesh_emit"):
    out[f"{name}:clamp_zero"] = call(name, clamp=0.0)
    out[f"{name}:clamp_negative"] = call(name, clamp=-1.0)
    out[f"{name}:clamp_nan"] = call(name, clamp=float("nan"))
    out[f"{name}:clamp_inf"] = call(name, clamp=float("inf"))
    out[f"{name}:select_255"] = call(name, select=255)
    out[f"{name}:select_without_labels"] = call(name, select=3, labels=None)
    out[f"{name}:workspace_too_small"] = call(name, workspace_bytes=WS - 4)
    out[f"{name}:size_overflows_int32"] = call(name, W=1024, L=1024, H=1024, workspace_bytes=1 << 40)
    out[f"{name}:cap_2"] = call(name, cap=2)
    out[f"{name}:stride_0"] = call(name, field_stride=0)
out["inr_mesh_count:counts_misaligned"] = call("inr_mesh_count", counts=ctypes.c_void_p(ADDR + 2))
out["inr_mesh_emit:vertices_misaligned"] = call("inr_mesh_emit", vertices=ctypes.c_void_p(ADDR + 2))
out["inr_mesh_emit:faces_misaligned"] = call("inr_mesh_emit", faces=ctypes.c_void_p(ADDR + 1))
out["inr_mesh_emit:colors_without_rgb"] = call("inr_mesh_emit", rgb=None)
out["inr_mesh_emit:face_labels_without_labels"] = call("inr_mesh_emit", labels=None)
out["inr_mesh_emit:negative_V"] = call("inr_mesh_emit", V=-1)
out["inr_mesh_emit:V_too_large"] = call("inr_mesh_emit", V=7 * 6 * 6 * 6 + 1)
for case, args in (("negative", (-1, 4, 4, 1)), ("zero", (4, 0, 4, 0)), ("cap_2", (4, 4, 4, 2)),
                   ("size_overflows_int32", (1024, 1024, 1024, 0))):
    out[f"inr_mesh_workspace_bytes:{case}"] = A.size_query("inr_mesh_workspace_bytes", *args)
out["inr_mesh_workspace_bytes:ok"] = [int(lib.inr_mesh_workspace_bytes(256, 256, 256, 1)), ""]
A.emit(out)
