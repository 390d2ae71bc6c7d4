"""Launches of inr_instance_lattice and inr_instance_volume_stats through the C ABI for
tests/test_instance_lattice_kernels.py, in the style of tests/field_forward_child.py, and, run as a script, both tiers of
the lattice cases on the library that INR_LIB_PATH names (a process binds one library): prints ``RESULT {"build": ...,
"failures": [...], "ratios": {output: worst |got - ref| as a fraction of its tolerance}}``.

``labels`` is one byte per voxel, so it lives in a byte buffer of its own (``ByteBuf``) with GUARD_BYTES guard bytes on
both sides, data and guards pre-filled with POISON_BYTE (no label: labels are < 64 or 255); confidence and density_logit
are ``Buf`` views pre-filled with the NaN sentinel.  After a launch no poison may be left inside and every guard must be
intact."""
import functools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import field_forward_child as L  # noqa: E402
import instance_lattice_reference as I  # noqa: E402
from test_train_kernels import Buf, check, stream  # noqa: E402

F32 = np.float32
GUARD_BYTES, POISON_BYTE = 67, 0xA5          # an odd guard: the label pointer is not even 2-byte aligned


class ByteBuf:
    """n bytes between two runs of GUARD_BYTES guard bytes, everything POISON_BYTE."""

    def __init__(self, n):
        import torch
        self.n = int(n)
        self.whole = torch.full((2 * GUARD_BYTES + self.n,), POISON_BYTE, dtype=torch.uint8, device="cuda:0")
        self.raw = self.whole[GUARD_BYTES:GUARD_BYTES + self.n]

    @property
    def ptr(self):
        return self.whole.data_ptr() + GUARD_BYTES

    def get(self):
        return self.raw.cpu().numpy()

    def check_guards(self, what=""):
        head, tail = self.whole[:GUARD_BYTES], self.whole[GUARD_BYTES + self.n:]
        assert bool((head == POISON_BYTE).all()) and bool((tail == POISON_BYTE).all()), f"{what}: a guard byte was written"


@functools.lru_cache(maxsize=2)
def inst_dev(table):
    return L.Dev(I.INST_TABLE[table], I.inst_embeddings(table))


def pack_instance(lib, W, K):
    """inr_instance_pack_weights for K_pad = 16 * ceil(K / 16) rows, rows K .. K_pad - 1 zero."""
    kp = (K + 15) // 16 * 16
    w2 = np.zeros((kp, 64), F32)
    w2[:K] = W[2]
    return L.pack_instance(lib, [W[0], W[1], w2], kp)


def launch(lib, ref, sigma_thresh, want_logit=True, dims=None, expect_written=True):
    """One inr_instance_lattice launch of ``ref``'s inputs -> (labels uint8 [N], confidence fp32 [N], density_logit fp32
    [N] or None).  dims: launch these (W, L, H) instead (ref's axis buffers, outputs of ref's size); expect_written False: every output must
    keep its poison (an empty lattice)."""
    Dn, Di = L.dev(ref.table), inst_dev(ref.table)
    W, Ln, H = dims or ref.dims
    N = W * Ln * H if expect_written else int(np.prod(ref.dims))
    axb = [Buf(a) for a in ref.ax]
    pn, pi = L.pack_nerf(lib, ref.Wn, 0), pack_instance(lib, ref.Wi, ref.K)
    lab, conf = ByteBuf(N), L._out(N)
    logit = L._out(N) if want_logit else None
    rc = lib.inr_instance_lattice(axb[0].ptr, axb[1].ptr, axb[2].ptr, W, Ln, H, ref.bound, Dn.emb[0].ptr, Dn.desc, pn.ptr,
                                  float(F32(ref.ds)), float(F32(sigma_thresh)), Di.emb[0].ptr, Di.desc, pi.ptr, ref.K, lab.ptr,
                                  conf.ptr, logit.ptr if want_logit else None, stream())
    check(rc, "instance_lattice")
    L._sync()
    lab.check_guards("labels")
    conf.check_guards("confidence")
    if want_logit:
        logit.check_guards("density_logit")
    out = lab.get(), conf.get(), logit.get() if want_logit else None
    for name, a in zip(("labels", "confidence", "density_logit"), out):
        if a is None:
            continue
        left = (a == POISON_BYTE) if name == "labels" else L.poisoned(a)
        if expect_written:
            assert not left.any(), f"{name}: {int(left.sum())} of {N} voxels were not written"
        else:
            assert left.all(), f"{name}: an empty lattice wrote something"
    return out


def run_case(lib, case, build, ratios, null_logit_on="q90"):
    """Every threshold of one lattice case -> list of failures; density_logit is null on one of them."""
    ref = I.reference(*case)
    fails = []
    for name, th in ref.thresholds().items():
        lab, conf, logit = launch(lib, ref, th, want_logit=name != null_logit_on)
        fails += [f"{I.case_id(case)}/{name}: {f}" for f in I.compare(ref, th, lab, conf, logit, build, ratios)]
    return fails


def launch_stats(lib, lab, conf, K):
    """inr_instance_volume_stats on a label volume -> (counts int32 [K], boxes int32 [K, 6], conf_sum fp32 [K]); the
    outputs are 64 channels long, and entries K .. 63 must keep their poison."""
    W, Ln, H = lab.shape
    N = lab.size
    lb = ByteBuf(max(N, 1))
    if N:
        import torch
        lb.raw.copy_(torch.from_numpy(np.ascontiguousarray(lab).reshape(-1)))
    cb = Buf(np.ascontiguousarray(conf, F32).reshape(-1) if N else np.zeros(1, F32))
    ws = L._out(lib_workspace_words())
    counts, boxes, sums = (Buf(np.zeros(s, t)) for s, t in (((64,), np.int32), ((64, 6), np.int32), ((64,), F32)))
    for b in (counts, boxes, sums):
        b.fill_nan()
    check(lib.inr_instance_volume_stats(lb.ptr, cb.ptr, W, Ln, H, K, ws.ptr, lib_workspace_words() * 4, counts.ptr, boxes.ptr,
                                        sums.ptr, stream()), "instance_volume_stats")
    L._sync()
    lb.check_guards("labels")
    for name, b in (("confidence", cb), ("workspace", ws), ("counts", counts), ("boxes", boxes), ("conf_sum", sums)):
        b.check_guards(name)
    c, bx, s = counts.get(), boxes.get(), sums.get()
    assert (c[K:] == L.SENTINEL).all() and (bx[K:] == L.SENTINEL).all() and L.poisoned(s[K:]).all(), "an entry beyond K was written"
    assert not (c[:K] == L.SENTINEL).any() and not (bx[:K] == L.SENTINEL).any() and not L.poisoned(s[:K]).any()
    return c[:K], bx[:K], s[:K]


def lib_workspace_words():
    from instance_nerf_amd import _lib
    return _lib.INSTANCE_STATS_WORKSPACE_BYTES // 4


def main():
    from instance_nerf_amd import _lib
    lib = _lib.load()
    build = os.environ.get("FIELD_FORWARD_BUILD", "fp32")
    ratios, fails = {}, []
    for case in I.cases():
        fails += run_case(lib, case, build, ratios)
    print("RESULT " + json.dumps({"build": build, "failures": fails, "ratios": ratios}))


if __name__ == "__main__":
    main()
