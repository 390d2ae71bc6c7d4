"""Child process of tests/test_instance_masks_cpu.py: calls the two instance-mask exports of include/inr.h with every
argument valid except the one named limit (K = 0 / 65, a misaligned output, a NaN threshold, a short workspace) and
prints one JSON object {"<name>:<case>": [return code, message]}.  Validation precedes every launch, so this runs on a
CPU-only box; a crash ends the process without the final line."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import _lib  # noqa: E402

lib = _lib.load()
HOST = ctypes.create_string_buffer(1 << 16)
ADDR = (ctypes.addressof(HOST) + 255) // 256 * 256


def desc():
    d = _lib.GridDesc()
    d.num_levels, d.level_dim = 16, 2
    for l in range(16):
        d.offsets[l] = 4096 * l
        d.scales[l] = float(16 * 2 ** l - 1)
        d.resolutions[l] = 16 * 2 ** l
        d.hashed[l] = 1
    d.offsets[16] = 4096 * 16
    return d


D = desc()


def args_for(name, **over):
    _, argtypes = _lib._SIGS[name]
    args = []
    for t in argtypes:
        if t is _lib.P:
            args.append(ctypes.c_void_p(ADDR))
        elif isinstance(t, type) and issubclass(t, ctypes._Pointer):
            args.append(ctypes.byref(D))
        elif t is ctypes.c_float:
            args.append(1.0)
        else:
            args.append(16)
    for k, v in over.items():
        args[int(k[1:])] = v
    return args


def call(name, **over):
    rc = int(getattr(lib, name)(*args_for(name, **over)))
    msg = lib.inr_last_error()
    return [rc, msg.decode() if msg else ""]


out = {}
L, S = "inr_instance_lattice", "inr_instance_volume_stats"
out[f"{L}:K_0"] = call(L, a15=0)
out[f"{L}:K_65"] = call(L, a15=65)
out[f"{L}:confidence_misaligned"] = call(L, a17=ctypes.c_void_p(ADDR + 2))
out[f"{L}:packed_misaligned"] = call(L, a14=ctypes.c_void_p(ADDR + 4))
out[f"{L}:sigma_thresh_nan"] = call(L, a11=float("nan"))
out[f"{L}:null_desc"] = call(L, a13=None)
out[f"{S}:K_0"] = call(S, a5=0, a7=_lib.INSTANCE_STATS_WORKSPACE_BYTES)
out[f"{S}:K_65"] = call(S, a5=65, a7=_lib.INSTANCE_STATS_WORKSPACE_BYTES)
out[f"{S}:workspace_too_small"] = call(S, a7=_lib.INSTANCE_STATS_WORKSPACE_BYTES - 4)
out[f"{S}:confidence_misaligned"] = call(S, a1=ctypes.c_void_p(ADDR + 2), a7=_lib.INSTANCE_STATS_WORKSPACE_BYTES)
out["alive"] = [0, "reached the end"]
sys.stdout.write(json.dumps(out) + "\n")
