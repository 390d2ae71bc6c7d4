"""Child process of tests/test_confusion_cpu.py: calls the two confusion exports of include/inr.h with every argument
valid except the one named and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation precedes
every launch, so this runs on a CPU-only box; a crash ends the process without the final line."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as A  # noqa: E402

ADDR = A.ADDR
SCALARS = dict(B=2, N=100, K=13, ld=16, s=None)


def call(name, **over):
    """All pointers into the host buffer, B = 2, N = 100, K = 13 (ld = 16); `over` replaces arguments by name."""
    params = [n for _, n in A.prototypes()[name]]
    return A.call(name, A.default_args(name), **dict({k: v for k, v in SCALARS.items() if k in params}, **over))


out = {}
for name in ("inr_confusion_ids", "inr_confusion_logits"):
    params = [n for _, n in A.prototypes()[name]]
    arrays = [n for n in params if n not in SCALARS]
    for arg in arrays:
        out[f"{name}:{arg}_null"] = call(name, **{arg: None})
    out[f"{name}:K_0"] = call(name, K=0)
    out[f"{name}:K_65"] = call(name, K=65, **({"ld": 80} if "ld" in params else {}))
    out[f"{name}:K_negative"] = call(name, K=-3)
    out[f"{name}:B_negative"] = call(name, B=-1)
    out[f"{name}:N_negative"] = call(name, N=-1)
    out[f"{name}:too_large"] = call(name, B=1 << 40, N=1 << 40)
    out[f"{name}:too_many_workgroups"] = call(name, B=1 << 20, N=1 << 22)
    out[f"{name}:counts_misaligned"] = call(name, counts=ctypes.c_void_p(ADDR + 4))
    out[f"{name}:ignored_misaligned"] = call(name, ignored=ctypes.c_void_p(ADDR + 4))
    out[f"{name}:B_0"] = call(name, B=0)
    out[f"{name}:N_0"] = call(name, N=0)
    out[f"{name}:B_0_null_pointers"] = call(name, B=0, **{a: None for a in arrays})
out["inr_confusion_logits:ld_below_K"] = call("inr_confusion_logits", ld=12)
out["inr_confusion_logits:ld_too_large"] = call("inr_confusion_logits", B=1 << 20, N=1 << 20, ld=1 << 30)
A.emit(out)
