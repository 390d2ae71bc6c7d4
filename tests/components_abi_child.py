"""Child process of tests/test_components_cpu.py: calls the connected-components exports of include/inr.h with every
argument valid except the one named and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation
precedes every launch, so this runs on a CPU-only box; a crash ends the process without the final line."""
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
WS = int(lib.inr_components_workspace_bytes(W, L, H))
assert 0 < WS < (1 << 15)

# argument positions (include/inr.h)
LABEL = dict(W=1, L=2, H=3, connectivity=4, ws=5, ws_bytes=6, roots=7)
FILTER = dict(roots=1, confidence=2, W=3, L=4, H=5, K=6, first_channel=7, min_voxels=8, keep_largest=9, ws=10, ws_bytes=11,
              labels_out=12, confidence_out=13, n_components=14)


def call(name, pos, **over):
    _, argtypes = _lib._SIGS[name]
    args = [ctypes.c_void_p(ADDR) if t is _lib.P else 1 for t in argtypes]
    base = dict(W=W, L=L, H=H, ws_bytes=WS)
    base.update(dict(connectivity=6) if "connectivity" in pos else dict(K=16, first_channel=1, min_voxels=1, keep_largest=1))
    base.update(over)
    for k, v in base.items():
        args[pos[k]] = v
    rc = int(getattr(lib, name)(*args))
    msg = lib.inr_last_error()
    return [rc, msg.decode() if msg else ""]


out = {}
for name, pos in (("inr_components_label", LABEL), ("inr_components_filter", FILTER)):
    out[f"{name}:workspace_too_small"] = call(name, pos, ws_bytes=WS - 8)
    out[f"{name}:workspace_misaligned"] = call(name, pos, ws=ctypes.c_void_p(ADDR + 4))
    out[f"{name}:roots_misaligned"] = call(name, pos, roots=ctypes.c_void_p(ADDR + 2))
    out[f"{name}:volume_2_31"] = call(name, pos, W=2048, L=1024, H=1024, ws_bytes=1 << 40)
    out[f"{name}:volume_2_33"] = call(name, pos, W=2048, L=2048, H=2048, ws_bytes=1 << 40)
    out[f"{name}:size_zero"] = call(name, pos, L=0)
for c in (0, 4, 8, 18, 27):
    out[f"inr_components_label:connectivity_{c}"] = call("inr_components_label", LABEL, connectivity=c)
out["inr_components_label:too_many_tiles"] = call("inr_components_label", LABEL, W=1 << 30, L=1, H=1, ws_bytes=1 << 40)
out["inr_components_filter:K_256"] = call("inr_components_filter", FILTER, K=256)
out["inr_components_filter:K_0"] = call("inr_components_filter", FILTER, K=0, first_channel=0)
out["inr_components_filter:first_channel_negative"] = call("inr_components_filter", FILTER, first_channel=-1)
out["inr_components_filter:first_channel_above_K"] = call("inr_components_filter", FILTER, first_channel=17)
out["inr_components_filter:min_voxels_0"] = call("inr_components_filter", FILTER, min_voxels=0)
out["inr_components_filter:keep_largest_2"] = call("inr_components_filter", FILTER, keep_largest=2)
out["inr_components_filter:confidence_out_without_confidence"] = call("inr_components_filter", FILTER, confidence=None)
out["inr_components_filter:n_components_misaligned"] = call("inr_components_filter", FILTER, n_components=ctypes.c_void_p(ADDR + 2))
out["inr_components_filter:labels_out_null"] = call("inr_components_filter", FILTER, labels_out=None)
for case, args in (("negative", (-1, 4, 4)), ("zero", (4, 0, 4)), ("volume_2_31", (2048, 1024, 1024)),
                   ("volume_2_33", (2048, 2048, 2048)), ("int32_product_wraps", (65536, 65536, 2))):
    rc = int(lib.inr_components_workspace_bytes(*args))
    out[f"inr_components_workspace_bytes:{case}"] = [rc, (lib.inr_last_error() or b"").decode()]
out["inr_components_workspace_bytes:ok"] = [int(lib.inr_components_workspace_bytes(256, 256, 256)), ""]
out["inr_components_workspace_bytes:largest"] = [int(lib.inr_components_workspace_bytes(2047, 1024, 1024)), ""]
out["alive"] = [0, "reached the end"]
sys.stdout.write(json.dumps(out) + "\n")
