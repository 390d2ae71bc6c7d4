"""Child process of tests/test_box_targets_cpu.py: calls the two box-matching exports of include/inr.h with every argument
valid except the one named and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation precedes
every launch, so this runs on a CPU-only box; a crash ends the process without the final line."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as probe  # noqa: E402

ADDR = probe.ADDR
SCALARS = dict(G=5, A=100, high=0.35, low=0.2, allow_low_quality=1, s=None)
REQUIRED = {"inr_box_match_gt_max": ("gt", "boxes", "gt_max_keys"),
            "inr_box_match_assign": ("gt", "boxes", "gt_max_keys", "matched")}


def call(name, **over):
    """All pointers into the host buffer, G = 5, A = 100, thresholds 0.35 / 0.2; `over` replaces arguments by name."""
    params = [n for _, n in probe.prototypes()[name]]
    return probe.call(name, probe.default_args(name), **dict({k: v for k, v in SCALARS.items() if k in params}, **over))


out = {}
for name in REQUIRED:
    arrays = [n for _, n in probe.prototypes()[name] if n not in SCALARS]
    for arg in REQUIRED[name]:
        out[f"{name}:{arg}_null"] = call(name, **{arg: None})
    out[f"{name}:G_0"] = call(name, G=0)
    out[f"{name}:G_1025"] = call(name, G=1025)
    out[f"{name}:G_negative"] = call(name, G=-4)
    out[f"{name}:A_negative"] = call(name, A=-1)
    out[f"{name}:A_overflow"] = call(name, A=(1 << 31) // 6 + 1)
    out[f"{name}:A_huge"] = call(name, A=1 << 40)
    out[f"{name}:gt_misaligned"] = call(name, gt=ctypes.c_void_p(ADDR + 2))
    out[f"{name}:A_0"] = call(name, A=0)
    out[f"{name}:A_0_null_pointers"] = call(name, A=0, **{a: None for a in arrays})
    out[f"{name}:A_0_G_0"] = call(name, A=0, G=0)
out["inr_box_match_assign:low_above_high"] = call("inr_box_match_assign", high=0.2, low=0.35)
out["inr_box_match_assign:low_nan"] = call("inr_box_match_assign", low=float("nan"))
out["inr_box_match_assign:A_0_low_above_high"] = call("inr_box_match_assign", A=0, high=0.2, low=0.35)
probe.emit(out)
