"""Launches of inr_instance_lattice and inr_instance_volume_stats through the C ABI for
tests/test_instance_lattice_kernels.py, in the style of tests/field_forward_child.py, and, run as a script, both tiers of
the lattice cases on the library that INR_LIB_PATH names (a process binds one library): prints ``RESULT {"build": ...,
"failures": [...], "ratios": {output: worst |got - ref| as a fraction of its tolerance}}``.

``labels`` is one byte per voxel, so it lives in a byte buffer of its own (``ByteBuf`` of kernel_harness) with guard bytes
on both sides, data and guards pre-filled with POISON_BYTE (no label: labels are < 64 or 255); confidence and density_logit
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
from kernel_harness import POISON_BYTE, SENTINEL, Buf, ByteBuf, check, finish, nan_out, poisoned, stream  # noqa: E402

F32 = np.float32


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
    lab, conf = ByteBuf(N), nan_out(N)
    logit = nan_out(N) if want_logit else None
    rc = lib.inr_instance_lattice(axb[0].ptr, axb[1].ptr, axb[2].ptr, W, Ln, H, ref.bound, Dn.emb[0].ptr, Dn.desc, pn.ptr,
                                  float(F32(ref.ds)), float(F32(sigma_thresh)), Di.emb[0].ptr, Di.desc, pi.ptr, ref.K, lab.ptr,
                                  conf.ptr, logit.ptr if want_logit else None, stream())
    check(rc, "instance_lattice")
    got = finish(dict(labels=lab, confidence=conf, density_logit=logit), "instance_lattice")
    for name, a in got.items():
        left = (a == POISON_BYTE) if name == "labels" else poisoned(a)
        if expect_written:
            assert not left.any(), f"{name}: {int(left.sum())} of {N} voxels were not written"
        else:
            assert left.all(), f"{name}: an empty lattice wrote something"
    return got["labels"], got["confidence"], got.get("density_logit")


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
    ws = nan_out(lib_workspace_words())
    counts, boxes, sums = nan_out(64, dtype=np.int32), nan_out(64, 6, dtype=np.int32), nan_out(64)
    check(lib.inr_instance_volume_stats(lb.ptr, cb.ptr, W, Ln, H, K, ws.ptr, lib_workspace_words() * 4, counts.ptr, boxes.ptr,
                                        sums.ptr, stream()), "instance_volume_stats")
    got = finish(dict(labels=lb, confidence=cb, workspace=ws, counts=counts, boxes=boxes, conf_sum=sums),
                 "instance_volume_stats")
    c, bx, s = got["counts"], got["boxes"], got["conf_sum"]
    assert (c[K:] == SENTINEL).all() and (bx[K:] == SENTINEL).all() and poisoned(s[K:]).all(), "an entry beyond K was written"
    assert not (c[:K] == SENTINEL).any() and not (bx[:K] == SENTINEL).any() and not poisoned(s[:K]).any()
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
