"""Child process of tests/test_confusion_cpu.py: calls the two confusion exports of include/inr.h with every argument
valid except the one named and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation precedes
every launch, so this runs on a CPU-only box; a crash ends the process without the final line."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instance_nerf_amd import _lib  # noqa: E402

lib = _lib.load()
HOST = ctypes.create_string_buffer(1 << 16)
ADDR = (ctypes.addressof(HOST) + 255) // 256 * 256

# argument positions (include/inr.h)
POS = {"inr_confusion_ids": dict(pred=0, truth=1, B=2, N=3, K=4, counts=5, ignored=6, stream=7),
       "inr_confusion_logits": dict(logits=0, truth=1, B=2, N=3, K=4, ld=5, counts=6, ignored=7, stream=8)}


def call(name, **over):
    """All pointers into the host buffer, B = 2, N = 100, K = 13 (ld = 16); `over` replaces arguments by name."""
    pos = POS[name]
    args = [ctypes.c_void_p(ADDR)] * len(pos)
    for k, v in dict(B=2, N=100, K=13, ld=16, stream=None).items():
        if k in pos:
            args[pos[k]] = v
    for k, v in over.items():
        args[pos[k]] = v
    rc = int(getattr(lib, name)(*args))
    msg = lib.inr_last_error()
    return [rc, msg.decode() if msg else ""]


out = {}
for name, pos in POS.items():
    for arg in pos:
        if arg in ("B", "N", "K", "ld", "stream"):
            continue
        out[f"{name}:{arg}_null"] = call(name, **{arg: None})
    out[f"{name}:K_0"] = call(name, K=0)
    out[f"{name}:K_65"] = call(name, K=65, **({"ld": 80} if "ld" in pos else {}))
    out[f"{name}:K_negative"] = call(name, K=-3)
    out[f"{name}:B_negative"] = call(name, B=-1)
    out[f"{name}:N_negative"] = call(name, N=-1)
    out[f"{name}:too_large"] = call(name, B=1 << 40, N=1 << 40)
    out[f"{name}:too_many_workgroups"] = call(name, B=1 << 20, N=1 << 22)
    out[f"{name}:counts_misaligned"] = call(name, counts=ctypes.c_void_p(ADDR + 4))
    out[f"{name}:ignored_misaligned"] = call(name, ignored=ctypes.c_void_p(ADDR + 4))
    out[f"{name}:B_0"] = call(name, B=0)
    out[f"{name}:N_0"] = call(name, N=0)
    out[f"{name}:B_0_null_pointers"] = call(name, B=0, **{a: None for a in pos if a not in ("B", "N", "K", "ld", "stream")})
out["inr_confusion_logits:ld_below_K"] = call("inr_confusion_logits", ld=12)
out["inr_confusion_logits:ld_too_large"] = call("inr_confusion_logits", B=1 << 20, N=1 << 20, ld=1 << 30)
out["alive"] = [0, "reached the end"]
sys.stdout.write(json.dumps(out) + "\n")
