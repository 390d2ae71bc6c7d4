"""Records tests/golden/field_issue_path.npz: the raw output bits of the fused field kernels on the seeded cases of
tests/field_issue_cases.py, as the library that is built in this tree computes them ON THE GPU.

The fixture pins a build, not the oracle: run it on the commit whose bits are to be kept (before a change of
csrc/field_fused.hip that must not move a bit), commit the file, and tests/test_field_issue_path.py holds every later
build to it.  From the repository root:  python tests/golden/make_field_issue_golden.py [OUT.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import field_issue_cases as cases                       # noqa: E402
from instance_nerf_amd.build import source_sha          # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                             "field_issue_path.npz")
    rec = {"field_sources_sha256": np.asarray(source_sha("field"))}
    n = 0
    for key, thunk in cases.all_cases():
        for name, a in thunk().items():
            rec[f"{key}/{name}"] = a
        n += 1
    np.savez_compressed(out, **rec)
    print(f"{out}: {n} launches, {len(rec)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
