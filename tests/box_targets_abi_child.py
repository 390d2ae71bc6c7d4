"""Child process of tests/test_box_targets_cpu.py: calls the two box-matching exports of include/inr.h with every argument
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
POS = {"inr_box_match_gt_max": dict(gt=0, G=1, boxes=2, valid=3, A=4, gt_max_keys=5, stream=6),
       "inr_box_match_assign": dict(gt=0, gt_labels=1, G=2, boxes=3, valid=4, A=5, gt_max_keys=6, high=7, low=8,
                                    allow_low_quality=9, matched=10, labels=11, best_iou=12, matched_boxes=13, targets=14,
                                    stream=15)}
SCALARS = ("G", "A", "high", "low", "allow_low_quality", "stream")
REQUIRED = {"inr_box_match_gt_max": ("gt", "boxes", "gt_max_keys"),
            "inr_box_match_assign": ("gt", "boxes", "gt_max_keys", "matched")}


def call(name, **over):
    """All pointers into the host buffer, G = 5, A = 100, thresholds 0.35 / 0.2; `over` replaces arguments by name."""
    pos = POS[name]
    args = [ctypes.c_void_p(ADDR)] * len(pos)
    for k, v in dict(G=5, A=100, high=0.35, low=0.2, allow_low_quality=1, stream=None).items():
        if k in pos:
            args[pos[k]] = v
    for k, v in over.items():
        args[pos[k]] = v
    rc = int(getattr(lib, name)(*args))
    msg = lib.inr_last_error()
    return [rc, msg.decode() if msg else ""]


out = {}
for name, pos in POS.items():
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
    out[f"{name}:A_0_null_pointers"] = call(name, A=0, **{a: None for a in pos if a not in SCALARS})
    out[f"{name}:A_0_G_0"] = call(name, A=0, G=0)
out["inr_box_match_assign:low_above_high"] = call("inr_box_match_assign", high=0.2, low=0.35)
out["inr_box_match_assign:low_nan"] = call("inr_box_match_assign", low=float("nan"))
out["inr_box_match_assign:A_0_low_above_high"] = call("inr_box_match_assign", A=0, high=0.2, low=0.35)
out["alive"] = [0, "reached the end"]
sys.stdout.write(json.dumps(out) + "\n")
