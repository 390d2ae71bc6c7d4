"""Child process of tests/test_evaluate_cpu.py: calls the 3-D mask overlap exports of include/inr.h with every argument
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
MASKS = dict(masks=0, k=1, V=2, planes=3, area=4)
LABELS = dict(labels=0, V=1, K=2, first_channel=3, planes=4, area=5)
OVERLAP = dict(planes_a=0, kA=1, planes_b=2, kB=3, V=4, run_words=5, inter=6)


def call(name, pos, **over):
    _, argtypes = _lib._SIGS[name]
    args = [ctypes.c_void_p(ADDR) if t is _lib.P else 4 for t in argtypes]
    if "run_words" in pos:
        args[pos["run_words"]] = 0
    if "first_channel" in pos:
        args[pos["first_channel"]] = 1
    for key, v in over.items():
        args[pos[key]] = v
    rc = int(getattr(lib, name)(*args))
    msg = lib.inr_last_error()
    return [rc, msg.decode() if msg else ""]


out = {}
for name, pos in (("inr_pack_mask_planes", MASKS), ("inr_pack_label_planes", LABELS), ("inr_mask_overlap", OVERLAP)):
    out[f"{name}:V_zero"] = call(name, pos, V=0)
    out[f"{name}:V_negative"] = call(name, pos, V=-1)
    out[f"{name}:V_2_31"] = call(name, pos, V=1 << 31)
    out[f"{name}:V_2_40"] = call(name, pos, V=1 << 40)
    if name != "inr_mask_overlap":
        out[f"{name}:planes_null"] = call(name, pos, planes=None)
        out[f"{name}:area_null"] = call(name, pos, area=None)
        out[f"{name}:planes_misaligned"] = call(name, pos, planes=ctypes.c_void_p(ADDR + 4))
out["inr_pack_mask_planes:k_negative"] = call("inr_pack_mask_planes", MASKS, k=-1)
out["inr_pack_mask_planes:k_1025"] = call("inr_pack_mask_planes", MASKS, k=1025)
out["inr_pack_mask_planes:masks_null"] = call("inr_pack_mask_planes", MASKS, masks=None)
out["inr_pack_mask_planes:k_zero_null_ok"] = call("inr_pack_mask_planes", MASKS, k=0, masks=None, planes=None, area=None)
out["inr_pack_label_planes:K_zero"] = call("inr_pack_label_planes", LABELS, K=0)
out["inr_pack_label_planes:K_257"] = call("inr_pack_label_planes", LABELS, K=257)
out["inr_pack_label_planes:first_channel_negative"] = call("inr_pack_label_planes", LABELS, first_channel=-1)
out["inr_pack_label_planes:first_channel_above_K"] = call("inr_pack_label_planes", LABELS, first_channel=5)
out["inr_pack_label_planes:labels_null"] = call("inr_pack_label_planes", LABELS, labels=None)
out["inr_pack_label_planes:first_channel_K_null_ok"] = call("inr_pack_label_planes", LABELS, first_channel=4, planes=None,
                                                            area=None)
for side in ("kA", "kB"):
    out[f"inr_mask_overlap:{side}_negative"] = call("inr_mask_overlap", OVERLAP, **{side: -1})
    out[f"inr_mask_overlap:{side}_1025"] = call("inr_mask_overlap", OVERLAP, **{side: 1025})
    out[f"inr_mask_overlap:{side}_zero_null_ok"] = call("inr_mask_overlap", OVERLAP, **{side: 0}, planes_a=None, planes_b=None,
                                                         inter=None)
out["inr_mask_overlap:run_words_100"] = call("inr_mask_overlap", OVERLAP, run_words=100)
out["inr_mask_overlap:run_words_negative"] = call("inr_mask_overlap", OVERLAP, run_words=-256)
out["inr_mask_overlap:planes_a_null"] = call("inr_mask_overlap", OVERLAP, planes_a=None)
out["inr_mask_overlap:planes_b_misaligned"] = call("inr_mask_overlap", OVERLAP, planes_b=ctypes.c_void_p(ADDR + 4))
out["inr_mask_overlap:inter_null"] = call("inr_mask_overlap", OVERLAP, inter=None)
out["alive"] = [0, "reached the end"]
sys.stdout.write(json.dumps(out) + "\n")
