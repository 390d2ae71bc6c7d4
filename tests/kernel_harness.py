"""What the kernel tests and their child scripts share: guarded device buffers, the NaN-filled output buffer, "synchronise,
check every guard, fetch", the device weight packers and the runner of a child that prints a ``RESULT`` line.

Every buffer a kernel writes is a view inside a larger allocation with guard words (``Buf``: GUARD words of a NaN
pattern) or guard bytes (``ByteBuf``: GUARD_BYTES bytes of POISON_BYTE) on either side, which must come back unchanged;
tests/test_kernel_harness.py pins that they notice a write one element outside the data."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

DEV = "cuda:0"
GUARD = 64
SENTINEL = 0x7FC0BEEF                  # a quiet NaN as fp32: a kernel that READS a guard word poisons its result too
GUARD_BYTES, POISON_BYTE = 67, 0xA5    # an odd guard: the pointer is not even 2-byte aligned; no label (< 64 or 255)
F32 = np.float32
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}


def check(rc, what=""):
    from instance_nerf_amd import _lib
    _lib.check(rc, what)


def stream():
    from instance_nerf_amd import _lib
    return _lib.stream_ptr()


def cu_count(lib):
    """The CU count the library's launch arithmetic uses (hipDeviceAttributeMultiprocessorCount)."""
    props = (ctypes.c_int64 * 8)()
    check(lib.inr_device_info(0, props), "device_info")
    assert props[0] == torch.cuda.get_device_properties(0).multi_processor_count > 0
    return int(props[0])


class Buf:
    """``data`` (float32 / int32, or uint8 with a byte count divisible by 4) inside a larger int32 allocation:
    GUARD sentinel words, ``offset`` more words (1 = a base pointer that is 4- but not 16-byte aligned), the data,
    GUARD sentinel words."""

    def __init__(self, data, offset=0):
        data = np.ascontiguousarray(data)
        self.shape, self.dtype = data.shape, data.dtype
        words = data.reshape(-1).view(np.int32)
        self.start, self.words = GUARD + offset, len(words)
        self.whole = torch.full((self.start + self.words + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        assert self.whole.data_ptr() % 256 == 0
        self.raw = self.whole[self.start:self.start + self.words]
        self.raw.copy_(torch.from_numpy(words))
        self.t = self.raw.view(_TORCH[self.dtype]).view(self.shape)

    @property
    def ptr(self):
        return self.raw.data_ptr() if self.words else None

    def get(self):
        return self.raw.cpu().numpy().view(self.dtype).reshape(self.shape)

    def fill_nan(self):
        self.raw.fill_(SENTINEL)

    def check_guards(self, what=""):
        head, tail = self.whole[:self.start], self.whole[self.start + self.words:]
        assert bool((head == SENTINEL).all()) and bool((tail == SENTINEL).all()), f"{what}: a guard word was written"


class ByteBuf:
    """n bytes between two runs of GUARD_BYTES guard bytes, everything POISON_BYTE."""

    def __init__(self, n):
        self.n = int(n)
        self.whole = torch.full((2 * GUARD_BYTES + self.n,), POISON_BYTE, dtype=torch.uint8, device=DEV)
        self.raw = self.whole[GUARD_BYTES:GUARD_BYTES + self.n]

    @property
    def ptr(self):
        return self.whole.data_ptr() + GUARD_BYTES

    def get(self):
        return self.raw.cpu().numpy()

    def check_guards(self, what=""):
        head, tail = self.whole[:GUARD_BYTES], self.whole[GUARD_BYTES + self.n:]
        assert bool((head == POISON_BYTE).all()) and bool((tail == POISON_BYTE).all()), f"{what}: a guard byte was written"


def nan_out(*shape, dtype=F32):
    """An output buffer of ``shape`` that holds the NaN sentinel in every word."""
    b = Buf(np.zeros(shape, dtype))
    b.fill_nan()
    return b


def poisoned(a):
    """Elementwise: the value is still the NaN sentinel the buffer was filled with."""
    return np.ascontiguousarray(a, F32).view(np.int32) == SENTINEL


def finish(bufs, what):
    """Synchronise, check the guards of every buffer of the dict ``bufs`` (None entries are skipped) -> their contents."""
    torch.cuda.synchronize()
    bufs = {k: b for k, b in bufs.items() if b is not None}
    for k, b in bufs.items():
        b.check_guards(f"{what} {k}")
    return {k: b.get() for k, b in bufs.items()}


def pack_nerf_device(lib, W):
    """inr_nerf_pack_weights_device -> (packed_fwd, packed_bwd, weight buffers: keep them until the launch has run)."""
    wb = [Buf(np.asarray(w, F32)) for w in W]
    pf, pb = nan_out(lib.inr_nerf_packed_floats()), nan_out(lib.inr_nerf_bwd_packed_floats())
    check(lib.inr_nerf_pack_weights_device(*[b.ptr for b in wb], pf.ptr, pb.ptr, stream()), "nerf pack")
    return pf, pb, wb


def pack_instance_device(lib, W, K):
    wb = [Buf(np.asarray(w, F32)) for w in W]
    pf, pb = nan_out(lib.inr_instance_packed_floats(K)), nan_out(lib.inr_instance_bwd_packed_floats())
    check(lib.inr_instance_pack_weights_device(*[b.ptr for b in wb], K, pf.ptr, pb.ptr, stream()), "instance pack")
    return pf, pb, wb


def run_result_child(script, env, timeout):
    """Runs ``script`` in a process of its own (a process binds one library: ``env`` names it) -> the JSON behind its
    last ``RESULT `` line."""
    r = subprocess.run([sys.executable, script], env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
