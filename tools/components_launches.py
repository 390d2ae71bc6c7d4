"""Per-launch times of the connected-components kernels, from the rocprofv3 --kernel-trace csv of
`tools/components_probe.py --launches-only --repeats R`: that run issues R label + filter calls for each of 160^3 / 256^3
x connectivity 6 / 26, in this order, so the i-th dispatch of a kernel belongs to configuration i // R.  The first two
calls of a configuration are warm-up and left out.  Mean / min / max in us.
usage: python tools/components_launches.py <trace dir> <R>"""
import csv, glob, sys
import numpy as np
files = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)
R = int(sys.argv[2])
rows = [r for f in files for r in csv.DictReader(open(f)) if "k_cc_" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
configs = ["160^3 conn 6", "160^3 conn 26", "256^3 conn 6", "256^3 conn 26"]
print(f"# kernel, configuration, dispatches, mean / min / max duration in us ({R - 2} of {R} calls per configuration)")
for name in ("k_cc_tile", "k_cc_merge", "k_cc_compress", "k_cc_init", "k_cc_select", "k_cc_finish", "k_cc_apply"):
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
    if len(us) != len(configs) * R:
        sys.exit(f"{name}: {len(us)} dispatches in the trace, expected {len(configs) * R}")
    for i, c in enumerate(configs):
        d = np.asarray(us[i * R + 2:(i + 1) * R])
        print(f"{name:<16}{c:<16}{len(d):>4}{d.mean():>10.1f}{d.min():>10.1f}{d.max():>10.1f}")
