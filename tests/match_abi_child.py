"""Child process of tests/test_match_masks_cpu.py: calls the 2-D mask matching exports of include/inr.h with every argument
valid except the one named and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation precedes
every launch, so this runs on a CPU-only box; a crash ends the process without the final line."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as A  # noqa: E402

ADDR = A.ADDR
PACK, COUNT, ASSIGN = "inr_pack_mask_bits", "inr_match_count", "inr_match_assign"


def _double(v):
    return ctypes.cast(ctypes.pointer(ctypes.c_double(v)), ctypes.c_void_p)


def call(name, **over):
    base = dict(iou_thresh=_double(0.05)) if name == ASSIGN else {}
    if over.get("iou_thresh") is not None:
        over["iou_thresh"] = _double(over["iou_thresh"])
    return A.call(name, A.default_args(name, ints=4, floats=0.5), **dict(base, **over))


out = {}
for name in (COUNT, ASSIGN):
    out[f"{name}:S_1024"] = call(name, S=1024)
    out[f"{name}:S_negative"] = call(name, S=-1)
    out[f"{name}:k_1025"] = call(name, k=1025)
    out[f"{name}:k_negative"] = call(name, k=-1)
    out[f"{name}:BP_2_31"] = call(name, B=1 << 15, P=1 << 16)
    out[f"{name}:BP_2_40"] = call(name, B=1 << 20, P=1 << 20)
    out[f"{name}:BP_wraps_int64"] = call(name, B=1 << 40, P=1 << 40)
    out[f"{name}:B_zero"] = call(name, B=0)
    out[f"{name}:P_zero"] = call(name, P=0)
    out[f"{name}:seg_null"] = call(name, seg=None)
    out[f"{name}:inter_null"] = call(name, inter=None)
    out[f"{name}:seg_area_misaligned"] = call(name, seg_area=ctypes.c_void_p(ADDR + 2))
out[f"{COUNT}:status_null"] = call(COUNT, status=None)
out[f"{ASSIGN}:iou_thresh_negative"] = call(ASSIGN, iou_thresh=-0.1)
out[f"{ASSIGN}:iou_thresh_1.5"] = call(ASSIGN, iou_thresh=1.5)
out[f"{ASSIGN}:iou_thresh_nan"] = call(ASSIGN, iou_thresh=float("nan"))
out[f"{ASSIGN}:iou_thresh_null"] = call(ASSIGN, iou_thresh=None)
out[f"{ASSIGN}:out_null"] = call(ASSIGN, out=None)
out[f"{PACK}:k_0"] = call(PACK, k=0)
out[f"{PACK}:k_1025"] = call(PACK, k=1025)
out[f"{PACK}:N_negative"] = call(PACK, N=-1)
out[f"{PACK}:P_zero"] = call(PACK, P=0)
out[f"{PACK}:words_null"] = call(PACK, words=None)
out[f"{PACK}:soft_null"] = call(PACK, soft=None)
out[f"{PACK}:inds_misaligned"] = call(PACK, inds=ctypes.c_void_p(ADDR + 4))
A.emit(out)
