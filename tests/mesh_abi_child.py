"""Child process of tests/test_mesh_cpu.py: calls the three mesh exports of include/inr.h with every argument valid except
the one named limit and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation precedes every
launch, so this runs on a CPU-only box; a crash ends the process without the final line."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import _lib  # noqa: E402

lib = _lib.load()
HOST = ctypes.create_string_buffer(1 << 16)
ADDR = (ctypes.addressof(HOST) + 255) // 256 * 256
W = L = H = 4
WS = int(lib.inr_mesh_workspace_bytes(W, L, H, 1))
assert 0 < WS < (1 << 15)

# argument positions (include/inr.h)
COUNT = dict(stride=1, iso=2, clamp=3, labels=4, select=5, W=6, L=7, H=8, cap=9, ws=10, ws_bytes=11, counts=12)
EMIT = dict(stride=1, iso=2, clamp=3, labels=4, select=5, rgb=6, W=10, L=11, H=12, cap=16, ws=17, ws_bytes=18, V=19, F=20,
            vertices=21, faces=22, colors=23, face_labels=24)


def call(name, pos, **over):
    _, argtypes = _lib._SIGS[name]
    args = [ctypes.c_void_p(ADDR) if t is _lib.P else (1.0 if t is ctypes.c_float else 1) for t in argtypes]
    base = dict(stride=1, select=-1, W=W, L=L, H=H, cap=1, ws_bytes=WS)
    if "V" in pos:
        base.update(V=8, F=8)
    base.update(over)
    for k, v in base.items():
        args[pos[k]] = v
    rc = int(getattr(lib, name)(*args))
    msg = lib.inr_last_error()
    return [rc, msg.decode() if msg else ""]


out = {}
for name, pos in (("inr_mesh_count", COUNT), ("inr_mesh_emit", EMIT)):
    out[f"{name}:clamp_zero"] = call(name, pos, clamp=0.0)
    out[f"{name}:clamp_negative"] = call(name, pos, clamp=-1.0)
    out[f"{name}:clamp_nan"] = call(name, pos, clamp=float("nan"))
    out[f"{name}:clamp_inf"] = call(name, pos, clamp=float("inf"))
    out[f"{name}:select_255"] = call(name, pos, select=255)
    out[f"{name}:select_without_labels"] = call(name, pos, select=3, labels=None)
    out[f"{name}:workspace_too_small"] = call(name, pos, ws_bytes=WS - 4)
    out[f"{name}:size_overflows_int32"] = call(name, pos, W=1024, L=1024, H=1024, ws_bytes=1 << 40)
    out[f"{name}:cap_2"] = call(name, pos, cap=2)
    out[f"{name}:stride_0"] = call(name, pos, stride=0)
out["inr_mesh_count:counts_misaligned"] = call("inr_mesh_count", COUNT, counts=ctypes.c_void_p(ADDR + 2))
out["inr_mesh_emit:vertices_misaligned"] = call("inr_mesh_emit", EMIT, vertices=ctypes.c_void_p(ADDR + 2))
out["inr_mesh_emit:faces_misaligned"] = call("inr_mesh_emit", EMIT, faces=ctypes.c_void_p(ADDR + 1))
out["inr_mesh_emit:colors_without_rgb"] = call("inr_mesh_emit", EMIT, rgb=None)
out["inr_mesh_emit:face_labels_without_labels"] = call("inr_mesh_emit", EMIT, labels=None)
out["inr_mesh_emit:negative_V"] = call("inr_mesh_emit", EMIT, V=-1)
out["inr_mesh_emit:V_too_large"] = call("inr_mesh_emit", EMIT, V=7 * 6 * 6 * 6 + 1)
for case, args in (("negative", (-1, 4, 4, 1)), ("zero", (4, 0, 4, 0)), ("cap_2", (4, 4, 4, 2)),
                   ("size_overflows_int32", (1024, 1024, 1024, 0))):
    rc = int(lib.inr_mesh_workspace_bytes(*args))
    out[f"inr_mesh_workspace_bytes:{case}"] = [rc, (lib.inr_last_error() or b"").decode()]
out["inr_mesh_workspace_bytes:ok"] = [int(lib.inr_mesh_workspace_bytes(256, 256, 256, 1)), ""]
out["alive"] = [0, "reached the end"]
sys.stdout.write(json.dumps(out) + "\n")
