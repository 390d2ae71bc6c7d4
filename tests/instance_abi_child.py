"""Child process of tests/test_instance_masks_cpu.py: calls the two instance-mask exports of include/inr.h with every
argument valid except the one named limit (K = 0 / 65, a misaligned output, a NaN threshold, a short workspace) and
prints one JSON object {"<name>:<case>": [return code, message]}.  Validation precedes every launch, so this runs on a
CPU-only box; a crash ends the process without the final line."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as A  # noqa: E402
from instance_nerf_amd import _lib  # noqa: E402

ADDR, D = A.ADDR, A.good_desc()
WS = _lib.INSTANCE_STATS_WORKSPACE_BYTES


def call(name, **by_name):
    return A.call(name, A.default_args(name, desc=D), **by_name)


out = {}
L, S = "inr_instance_lattice", "inr_instance_volume_stats"
out[f"{L}:K_0"] = call(L, K=0)
out[f"{L}:K_65"] = call(L, K=65)
out[f"{L}:confidence_misaligned"] = call(L, confidence=ctypes.c_void_p(ADDR + 2))
out[f"{L}:packed_misaligned"] = call(L, inst_packed=ctypes.c_void_p(ADDR + 4))
out[f"{L}:sigma_thresh_nan"] = call(L, sigma_thresh=float("nan"))
out[f"{L}:null_desc"] = call(L, inst_desc=None)
out[f"{S}:K_0"] = call(S, K=0, workspace_bytes=WS)
out[f"{S}:K_65"] = call(S, K=65, workspace_bytes=WS)
out[f"{S}:workspace_too_small"] = call(S, workspace_bytes=WS - 4)
out[f"{S}:confidence_misaligned"] = call(S, confidence=ctypes.c_void_p(ADDR + 2), workspace_bytes=WS)
A.emit(out)
