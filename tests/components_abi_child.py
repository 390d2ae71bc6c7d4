"""Child process of tests/test_components_cpu.py: calls the connected-components exports of include/inr.h with every
argument valid except the one named and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation
precedes every launch, so this runs on a CPU-only box; a crash ends the process without the final line."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as A  # noqa: E402
from instance_nerf_amd import _lib  # noqa: E402

lib = _lib.load()
ADDR = A.ADDR
W = L = H = 4
WS = int(lib.inr_components_workspace_bytes(W, L, H))
assert 0 < WS < (1 << 15)
LABEL, FILTER = "inr_components_label", "inr_components_filter"
SIZES = dict(W=W, L=L, H=H, workspace_bytes=WS)
BASE = {LABEL: dict(SIZES, connectivity=6), FILTER: dict(SIZES, K=16, first_channel=1, min_voxels=1, keep_largest=1)}


def call(name, **over):
    return A.call(name, A.default_args(name, ints=1), **dict(BASE[name], **over))


out = {}
for name in (LABEL, FILTER):
    out[f"{name}:workspace_too_small"] = call(name, workspace_bytes=WS - 8)
    out[f"{name}:workspace_misaligned"] = call(name, workspace=ctypes.c_void_p(ADDR + 4))
    out[f"{name}:roots_misaligned"] = call(name, roots=ctypes.c_void_p(ADDR + 2))
    out[f"{name}:volume_2_31"] = call(name, W=2048, L=1024, H=1024, workspace_bytes=1 << 40)
    out[f"{name}:volume_2_33"] = call(name, W=2048, L=2048, H=2048, workspace_bytes=1 << 40)
    out[f"{name}:size_zero"] = call(name, L=0)
for c in (0, 4, 8, 18, 27):
    out[f"{LABEL}:connectivity_{c}"] = call(LABEL, connectivity=c)
out[f"{LABEL}:too_many_tiles"] = call(LABEL, W=1 << 30, L=1, H=1, workspace_bytes=1 << 40)
out[f"{FILTER}:K_256"] = call(FILTER, K=256)
out[f"{FILTER}:K_0"] = call(FILTER, K=0, first_channel=0)
out[f"{FILTER}:first_channel_negative"] = call(FILTER, first_channel=-1)
out[f"{FILTER}:first_channel_above_K"] = call(FILTER, first_channel=17)
out[f"{FILTER}:min_voxels_0"] = call(FILTER, min_voxels=0)
out[f"{FILTER}:keep_largest_2"] = call(FILTER, keep_largest=2)
out[f"{FILTER}:confidence_out_without_confidence"] = call(FILTER, confidence=None)
out[f"{FILTER}:n_components_misaligned"] = call(FILTER, n_components=ctypes.c_void_p(ADDR + 2))
out[f"{FILTER}:labels_out_null"] = call(FILTER, labels_out=None)
for case, args in (("negative", (-1, 4, 4)), ("zero", (4, 0, 4)), ("volume_2_31", (2048, 1024, 1024)),
                   ("volume_2_33", (2048, 2048, 2048)), ("int32_product_wraps", (65536, 65536, 2))):
    out[f"inr_components_workspace_bytes:{case}"] = A.size_query("inr_components_workspace_bytes", *args)
out["inr_components_workspace_bytes:ok"] = [int(lib.inr_components_workspace_bytes(256, 256, 256)), ""]
out["inr_components_workspace_bytes:largest"] = [int(lib.inr_components_workspace_bytes(2047, 1024, 1024)), ""]
A.emit(out)
