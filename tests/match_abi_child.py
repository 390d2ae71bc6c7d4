"""Child process of tests/test_match_masks_cpu.py: calls the 2-D mask matching exports of include/inr.h with every argument
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
PACK = dict(soft=0, inds=1, N=2, k=3, P=5, words=6)
COUNT = dict(seg=0, words=1, B=2, P=3, S=4, k=5, seg_area=6, mask_area=7, inter=8, status=9)
ASSIGN = dict(seg=0, seg_area=1, mask_area=2, inter=3, instance_ids=4, B=5, P=6, S=7, k=8, iou_thresh=9, assigned=10, out=11)
THRESH = ctypes.c_double(0.05)


def call(name, pos, **over):
    _, argtypes = _lib._SIGS[name]
    args = [ctypes.c_void_p(ADDR) if t is _lib.P else (0.5 if t is ctypes.c_float else 4) for t in argtypes]
    if "iou_thresh" in pos:
        args[pos["iou_thresh"]] = ctypes.cast(ctypes.pointer(THRESH), ctypes.c_void_p)
    for key, v in over.items():
        if key == "iou_thresh" and v is not None:
            v = ctypes.cast(ctypes.pointer(ctypes.c_double(v)), ctypes.c_void_p)
        args[pos[key]] = v
    rc = int(getattr(lib, name)(*args))
    msg = lib.inr_last_error()
    return [rc, msg.decode() if msg else ""]


out = {}
for name, pos in (("inr_match_count", COUNT), ("inr_match_assign", ASSIGN)):
    out[f"{name}:S_1024"] = call(name, pos, S=1024)
    out[f"{name}:S_negative"] = call(name, pos, S=-1)
    out[f"{name}:k_1025"] = call(name, pos, k=1025)
    out[f"{name}:k_negative"] = call(name, pos, k=-1)
    out[f"{name}:BP_2_31"] = call(name, pos, B=1 << 15, P=1 << 16)
    out[f"{name}:BP_2_40"] = call(name, pos, B=1 << 20, P=1 << 20)
    out[f"{name}:BP_wraps_int64"] = call(name, pos, B=1 << 40, P=1 << 40)
    out[f"{name}:B_zero"] = call(name, pos, B=0)
    out[f"{name}:P_zero"] = call(name, pos, P=0)
    out[f"{name}:seg_null"] = call(name, pos, seg=None)
    out[f"{name}:inter_null"] = call(name, pos, inter=None)
    out[f"{name}:seg_area_misaligned"] = call(name, pos, seg_area=ctypes.c_void_p(ADDR + 2))
out["inr_match_count:status_null"] = call("inr_match_count", COUNT, status=None)
out["inr_match_assign:iou_thresh_negative"] = call("inr_match_assign", ASSIGN, iou_thresh=-0.1)
out["inr_match_assign:iou_thresh_1.5"] = call("inr_match_assign", ASSIGN, iou_thresh=1.5)
out["inr_match_assign:iou_thresh_nan"] = call("inr_match_assign", ASSIGN, iou_thresh=float("nan"))
out["inr_match_assign:iou_thresh_null"] = call("inr_match_assign", ASSIGN, iou_thresh=None)
out["inr_match_assign:out_null"] = call("inr_match_assign", ASSIGN, out=None)
out["inr_pack_mask_bits:k_0"] = call("inr_pack_mask_bits", PACK, k=0)
out["inr_pack_mask_bits:k_1025"] = call("inr_pack_mask_bits", PACK, k=1025)
out["inr_pack_mask_bits:N_negative"] = call("inr_pack_mask_bits", PACK, N=-1)
out["inr_pack_mask_bits:P_zero"] = call("inr_pack_mask_bits", PACK, P=0)
out["inr_pack_mask_bits:words_null"] = call("inr_pack_mask_bits", PACK, words=None)
out["inr_pack_mask_bits:soft_null"] = call("inr_pack_mask_bits", PACK, soft=None)
out["inr_pack_mask_bits:inds_misaligned"] = call("inr_pack_mask_bits", PACK, inds=ctypes.c_void_p(ADDR + 4))
out["alive"] = [0, "reached the end"]
sys.stdout.write(json.dumps(out) + "\n")
