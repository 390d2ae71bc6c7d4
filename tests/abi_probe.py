"""What the bad-argument children (tests/abi_negative_child.py, tests/*_abi_child.py) and their parents share.  A child
calls exports of include/inr.h with every argument valid except the one its case names and prints one JSON object
{"<name>:<case>": [return code, message]}; validation precedes every launch, so it runs on a CPU-only box, and a crash
ends it without the final line.  Arguments are addressed by the parameter names of the header, never by position: a
parameter inserted into an export moves no probe to a neighbour, and one renamed or removed kills the child."""
import ctypes
import functools
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "inr.h")
sys.path.insert(0, ROOT)


@functools.lru_cache(maxsize=None)
def prototypes(header=HEADER):
    """export -> [(type string, parameter name), ...], parsed from the header."""
    src = open(header).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for m in re.finditer(r"\b(?:int|int64_t|const char\*)\s+(inr_[a-zA-Z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = " ".join(m.group(2).split())
        params = []
        for a in ([] if args in ("", "void") else args.split(",")):
            decl, name = re.fullmatch(r"\s*(.*?)\s*\b([A-Za-z_][A-Za-z0-9_]*)\s*", a).groups()
            params.append((decl, name))
        out[m.group(1)] = params
    return out


# ---------------------------------------------------------------------------- the children
HOST = ctypes.create_string_buffer(1 << 16)              # 64 KB of zeroed, readable, writable host memory
ADDR = (ctypes.addressof(HOST) + 255) // 256 * 256


def _binding():
    from instance_nerf_amd import _lib
    return _lib


def last_error():
    msg = _binding().load().inr_last_error()
    return msg.decode() if msg else ""


def good_desc(levels=16, level_dim=2):
    _lib = _binding()
    d = _lib.GridDesc()
    d.num_levels, d.level_dim = levels, level_dim
    off = 0
    for l in range(min(levels, _lib.MAX_LEVELS)):
        d.offsets[l] = off
        d.scales[l] = float(16 * 2 ** l - 1)
        d.resolutions[l] = 16 * 2 ** l
        d.hashed[l] = 1
        off += 4096
    d.offsets[min(levels, _lib.MAX_LEVELS)] = off
    return d


def is_pointer(t):
    return t is _binding().P or t is ctypes.c_char_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def pointer(t, addr):
    return ctypes.c_void_p(addr) if t is _binding().P else ctypes.cast(addr, t)


def default_args(name, ints=16, floats=1.0, desc=None):
    """One argument per `_SIGS` type: pointers into the host buffer (grid descriptors -> ``desc`` where one is given),
    every integer ``ints``, every float ``floats``."""
    args = []
    for t in _binding()._SIGS[name][1]:
        if is_pointer(t):
            typed = t is not _binding().P and t is not ctypes.c_char_p
            args.append(ctypes.byref(desc) if typed and desc is not None else pointer(t, ADDR))
        else:
            args.append(floats if t is ctypes.c_float else ints)
    return args


def call(name, defaults, /, **by_name):
    """The export on ``defaults`` with the parameters ``by_name`` names (as include/inr.h does) replaced
    -> [return code, message]."""
    names = [n for _, n in prototypes()[name]]
    args = list(defaults)
    assert len(args) == len(names), (name, len(args), names)
    for key, v in by_name.items():
        if key not in names:
            raise KeyError(f"{name} has no parameter {key!r} in include/inr.h (it has {', '.join(names)})")
        args[names.index(key)] = v
    rc = int(getattr(_binding().load(), name)(*args))
    return [rc, last_error()]


def size_query(name, *args):
    rc = int(getattr(_binding().load(), name)(*args))
    return [rc, last_error()]


def emit(out):
    out["alive"] = [0, "reached the end"]
    sys.stdout.write(json.dumps(out) + "\n")


# ---------------------------------------------------------------------------- the parents
NO_GPU = dict(HIP_VISIBLE_DEVICES=os.environ.get("HIP_VISIBLE_DEVICES", ""))


def run_abi_child(script, env=None):
    """Builds the library if it is missing and runs tests/<script> -> the dict of its last line."""
    from instance_nerf_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script)], capture_output=True, text=True, timeout=600,
                       env=None if env is None else dict(os.environ, **env))
    assert r.returncode == 0, f"the child died (rc {r.returncode}): an export crashed on bad arguments\n{r.stderr[-2000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, r.stdout[-1000:]
    out = json.loads(lines[-1])
    assert out["alive"] == [0, "reached the end"]
    return out
