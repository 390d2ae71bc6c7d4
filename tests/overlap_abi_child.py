"""Child process of tests/test_evaluate_cpu.py: calls the 3-D mask overlap exports of include/inr.h with every argument
valid except the one named and prints one JSON object {"<name>:<case>": [return code, message]}.  Validation precedes
every launch, so this runs on a CPU-only box; a crash ends the process without the final line."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_probe as A  # noqa: E402

ADDR = A.ADDR
MASKS, LABELS, OVERLAP = "inr_pack_mask_planes", "inr_pack_label_planes", "inr_mask_overlap"
BASE = {MASKS: {}, LABELS: dict(first_channel=1), OVERLAP: dict(run_words=0)}


def call(name, **over):
    return A.call(name, A.default_args(name, ints=4), **dict(BASE[name], **over))


out = {}
for name in (MASKS, LABELS, OVERLAP):
    out[f"{name}:V_zero"] = call(name, V=0)
    out[f"{name}:V_negative"] = call(name, V=-1)
    out[f"{name}:V_2_31"] = call(name, V=1 << 31)
    out[f"{name}:V_2_40"] = call(name, V=1 << 40)
    if name != OVERLAP:
        out[f"{name}:planes_null"] = call(name, planes=None)
        out[f"{name}:area_null"] = call(name, area=None)
        out[f"{name}:planes_misaligned"] = call(name, planes=ctypes.c_void_p(ADDR + 4))
out[f"{MASKS}:k_negative"] = call(MASKS, k=-1)
out[f"{MASKS}:k_1025"] = call(MASKS, k=1025)
out[f"{MASKS}:masks_null"] = call(MASKS, masks=None)
out[f"{MASKS}:k_zero_null_ok"] = call(MASKS, k=0, masks=None, planes=None, area=None)
out[f"{LABELS}:K_zero"] = call(LABELS, K=0)
out[f"{LABELS}:K_257"] = call(LABELS, K=257)
out[f"{LABELS}:first_channel_negative"] = call(LABELS, first_channel=-1)
out[f"{LABELS}:first_channel_above_K"] = call(LABELS, first_channel=5)
out[f"{LABELS}:labels_null"] = call(LABELS, labels=None)
out[f"{LABELS}:first_channel_K_null_ok"] = call(LABELS, first_channel=4, planes=None, area=None)
for side in ("kA", "kB"):
    out[f"{OVERLAP}:{side}_negative"] = call(OVERLAP, **{side: -1})
    out[f"{OVERLAP}:{side}_1025"] = call(OVERLAP, **{side: 1025})
    out[f"{OVERLAP}:{side}_zero_null_ok"] = call(OVERLAP, **{side: 0}, planes_a=None, planes_b=None, inter=None)
out[f"{OVERLAP}:run_words_100"] = call(OVERLAP, run_words=100)
out[f"{OVERLAP}:run_words_negative"] = call(OVERLAP, run_words=-256)
out[f"{OVERLAP}:planes_a_null"] = call(OVERLAP, planes_a=None)
out[f"{OVERLAP}:planes_b_misaligned"] = call(OVERLAP, planes_b=ctypes.c_void_p(ADDR + 4))
out[f"{OVERLAP}:inter_null"] = call(OVERLAP, inter=None)
A.emit(out)
