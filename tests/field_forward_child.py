"""Launches of the fused field's forward entry points through the C ABI for tests/test_field_forward_kernels.py (every
template instantiation is reached whatever the Python layer would choose), and, run as a script, both tiers on the
library that INR_LIB_PATH names (a process binds one library): prints ``RESULT {"build": ..., "failures": [...],
"ratios": {output: worst |got - ref| / cond}}``.

Every buffer a kernel writes is a guarded view pre-filled with the NaN sentinel (``Buf`` of kernel_harness); inputs
carry NaN guard words on both sides.  Guards, and rows at or beyond the valid count, must keep their poison.  Host
packers (inr_*_pack_weights, plain and fp16) serve the inference entry points, the device packers
(inr_*_pack_weights_device) the training ones."""
import functools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import field_forward_reference as R  # noqa: E402
from kernel_harness import Buf, check, finish, nan_out, pack_instance_device, pack_nerf_device, poisoned, stream  # noqa: E402
from train_kernels_reference import assert_same_bits, bit_mismatches  # noqa: E402

F32 = np.float32


def _sync():
    import torch
    torch.cuda.synchronize()


class Dev:
    """A level table on the device: fp32 values, the fp16 copy, and the fp16 copy widened to fp32 again."""

    def __init__(self, table, emb=None):
        from instance_nerf_amd import _lib
        self.name, self.t = table, R.table_for(table)
        self.desc = _lib.make_grid_desc(self.t)
        emb = R.embeddings(table) if emb is None else np.asarray(emb, F32)
        half = emb.astype(np.float16)
        self.emb = {0: Buf(emb), 1: Buf(np.ascontiguousarray(half).view(np.int32).reshape(-1)), "rounded": Buf(half.astype(F32))}


@functools.lru_cache(maxsize=2)
def dev(table):
    return Dev(table)


def pack_nerf(lib, W, numerics=0, device=False):
    if device:
        pf, _, keep = pack_nerf_device(lib, W)
        _sync()
        return pf
    ws = [np.ascontiguousarray(w, F32) for w in W]
    buf = np.full(lib.inr_nerf_packed_floats(), np.nan, F32)
    check(lib.inr_nerf_pack_weights(*[w.ctypes.data for w in ws], buf.ctypes.data, numerics & 2), "nerf pack")
    return Buf(buf)


def pack_instance(lib, W, K, device=False, numerics=0):
    if device:
        pf, _, keep = pack_instance_device(lib, W, K)
        _sync()
        return pf
    ws = [np.ascontiguousarray(w, F32) for w in W]
    buf = np.full(lib.inr_instance_packed_floats(K), np.nan, F32)
    check(lib.inr_instance_pack_weights(*[w.ctypes.data for w in ws], K, buf.ctypes.data, numerics), "instance pack")
    return Buf(buf)


def ray_table(lib, o, d):
    """inr_ray_table_q -> (device rows [N,24], the SH rows [N,16] it holds); the origin and direction columns must echo
    the inputs bit for bit."""
    N = len(o)
    ob, db, rt = Buf(np.asarray(o, F32)), Buf(np.asarray(d, F32)), nan_out(N, 24)
    check(lib.inr_ray_table_q(ob.ptr, db.ptr, N, rt.ptr, stream()), "ray_table_q")
    rows = finish({"ray_table": rt}, "ray_table_q")["ray_table"]
    assert_same_bits(rows[:, 16:19], np.asarray(o, F32), "ray table origins")
    assert_same_bits(rows[:, 20:23], np.asarray(d, F32), "ray table directions")
    sh = rows[:, :16].reshape(N, 4, 4).transpose(0, 2, 1).reshape(N, 16)
    return rt, np.ascontiguousarray(sh)


def launch(lib, table, entry, M, D=None, W=None, n_dev=None, emb_key=None, numerics=None, bound=None, x=None, sc=None,
           expect_rc=0):
    """One launch of ``entry`` on the scene of (table, M) -> (outputs as numpy, SH rows the launch used or None).
    D: a Dev to use instead of dev(table); W: weights instead of the table's; n_dev: device-side sample count;
    emb_key / numerics: override which table copy / numerics the launch gets; x: plain-feed positions instead of the
    scene's; sc: a scene instead of the table's."""
    D = D or dev(table)
    variant, grid = R.variant_for(table, entry), R.grid_for(table, entry)
    bound0, ds = R.SETTINGS[table]
    bound = bound0 if bound is None else bound
    sc = sc or R.scene(table, M, bound0, grid)
    nb = None if n_dev is None else Buf(np.asarray([n_dev], np.int32))
    nbp = None if nb is None else nb.ptr
    s, sh_used = stream(), None

    if entry in R.INSTANCE_ENTRIES:
        mode, K = R.INSTANCE_ENTRIES[entry]
        packed = pack_instance(lib, W or R.instance_weights(table, K), K, device=mode != "")
        xb = Buf(R.plain_x(sc, bound) if x is None else x)
        o = {"logits": nan_out(M, K)}
        if mode == "":
            rc = lib.inr_instance_forward(xb.ptr, M, nbp, bound, D.emb[0].ptr, D.desc, packed.ptr, K, o["logits"].ptr, s)
        elif mode == "_train":
            o.update(ienc=nan_out(M, 32), ih1=nan_out(M, 64), ih2=nan_out(M, 64))
            rc = lib.inr_instance_forward_train(xb.ptr, M, bound, D.emb[0].ptr, D.desc, packed.ptr, K, o["logits"].ptr,
                                                o["ienc"].ptr, o["ih1"].ptr, o["ih2"].ptr, s)
        else:
            o["ienc"] = nan_out(M, 32)
            rc = lib.inr_instance_forward_enc(xb.ptr, M, nbp, bound, D.emb[0].ptr, D.desc, packed.ptr, K, o["logits"].ptr,
                                              o["ienc"].ptr, s)
        assert rc == expect_rc, (entry, rc)
        return finish(o, entry), None

    feed, num_name = R.NERF_ENTRIES[entry][:2]
    numerics = R.NUMERICS[num_name] if numerics is None else numerics
    ek = (numerics & 1) if emb_key is None else emb_key
    W = W or R.nerf_weights(table, variant)
    packed = pack_nerf(lib, W, numerics, device=entry in ("train", "enc"))
    emb = D.emb[ek].ptr
    if entry in ("fwd_rgb", "fwd_density", "fwd_o", "train", "enc"):
        xb, db = Buf(R.plain_x(sc, bound) if x is None else x), Buf(sc["dirs"])
        o = {"sigma": nan_out(M)}
        if entry != "fwd_density":
            o["rgb"] = nan_out(M, 3)
        if entry == "fwd_density":
            o["geo"] = nan_out(M, 15)
        if entry.startswith("fwd"):
            rc = lib.inr_nerf_forward(xb.ptr, None if entry == "fwd_density" else db.ptr, M, nbp, bound, emb, D.desc,
                                      packed.ptr, ds, o["sigma"].ptr, o["rgb"].ptr if "rgb" in o else None,
                                      o["geo"].ptr if "geo" in o else None, numerics, s)
        elif entry == "train":
            o.update(enc=nan_out(M, 32), h1=nan_out(M, 64), so=nan_out(M, 16), cin=nan_out(M, 32), c1=nan_out(M, 64),
                     c2=nan_out(M, 64))
            rc = lib.inr_nerf_forward_train(xb.ptr, db.ptr, M, bound, emb, D.desc, packed.ptr, o["sigma"].ptr, o["rgb"].ptr,
                                            o["enc"].ptr, o["h1"].ptr, o["so"].ptr, o["cin"].ptr, o["c1"].ptr, o["c2"].ptr, s)
        else:
            o["enc"] = nan_out(M, 32)
            rc = lib.inr_nerf_forward_enc(xb.ptr, db.ptr, M, bound, emb, D.desc, packed.ptr, o["sigma"].ptr, o["rgb"].ptr,
                                          o["enc"].ptr, s)
        if entry in ("train", "enc"):
            o["sigma1"] = o.pop("sigma")
    elif entry.startswith("table") or entry == "sliced":
        xb, rb, qb = Buf(sc["x01"]), Buf(sc["ray_ids"]), Buf(R.q_rows(sc["shrow"]))
        o = {"sigma": nan_out(M), "rgb": nan_out(M, 3)}
        if entry == "sliced":
            ws = nan_out(max(1, lib.inr_nerf_forward_table_sliced_workspace_bytes(M) // 4))
            rc = lib.inr_nerf_forward_table_sliced(xb.ptr, rb.ptr, qb.ptr, M, bound, emb, D.desc, packed.ptr, ds,
                                                   o["sigma"].ptr, o["rgb"].ptr, ws.ptr, s)
            _sync()
            ws.check_guards("sliced workspace")
        else:
            rc = lib.inr_nerf_forward_table(xb.ptr, rb.ptr, qb.ptr, M, bound, emb, D.desc, packed.ptr, ds, o["sigma"].ptr,
                                            o["rgb"].ptr, numerics, s)
    elif entry.startswith("records"):
        rt, sh_used = ray_table(lib, sc["o"], sc["d"])
        tb, rb = Buf(sc["t"]), Buf(sc["ray_ids"])
        o = {"sigma": nan_out(M), "rgb": nan_out(M, 3)}
        old = os.environ.get("INR_FIELD_PAIR")
        if entry == "records_nopair":
            os.environ["INR_FIELD_PAIR"] = "0"
        else:
            os.environ.pop("INR_FIELD_PAIR", None)
        try:
            rc = lib.inr_nerf_forward_table_records(tb.ptr, rb.ptr, rt.ptr, M, bound, emb, D.desc, packed.ptr, ds,
                                                    o["sigma"].ptr, o["rgb"].ptr, numerics, s)
        finally:
            os.environ.pop("INR_FIELD_PAIR", None)
            if old is not None:
                os.environ["INR_FIELD_PAIR"] = old
    elif entry.startswith("dirs"):
        nd = int(entry[4:])
        xb, shb = Buf(R.plain_x(sc, bound) if x is None else x), Buf(R.sh_dirs_rows(table, nd))
        o4 = nan_out(M, 4)
        rc = lib.inr_nerf_forward_dirs(xb.ptr, M, bound, emb, D.desc, packed.ptr, shb.ptr, nd, o4.ptr, s)
        o = {"o4": o4}
    elif entry == "lattice":
        ax = R.lattice_axes(table, bound)
        axb, shb = [Buf(a) for a in ax], Buf(R.sh_dirs_rows(table, 3))
        Wn, Ln, Hn = (len(a) for a in ax)
        o4 = nan_out(Wn, Ln, Hn, 4)
        rc = lib.inr_nerf_forward_lattice(axb[0].ptr, axb[1].ptr, axb[2].ptr, Wn, Ln, Hn, bound, emb, D.desc, packed.ptr,
                                          shb.ptr, 3, R.LOGIT_MIN[R.tier_of(table)], o4.ptr, s)
        o = {"o4": o4}
    else:
        raise KeyError(entry)
    assert rc == expect_rc, (entry, rc)
    got = finish(o, entry)
    if "o4" in got:
        o4 = got.pop("o4").reshape(-1, 4)
        got["rgbm"], got["logit"] = o4[:, :3], o4[:, 3]
    return got, sh_used


def compare(table, entry, M, got, sh, build, ratios, rows=None):
    """Exact tier: every output equals the float64 result rounded to fp32 bit for bit (cin without its SH columns).
    Tolerance tier: |got - ref| <= TOL * cond elementwise; the worst ratio per output goes into ``ratios`` first.
    rows: compare the first ``rows`` rows only (device-side sample count); the rest must still be poisoned."""
    ref = R.reference(table, M, R.variant_for(table, entry), R.grid_for(table, entry))
    want, cond = R.expected(ref, entry, sh)
    fails = []
    for k in want:
        g, w, c = got[k], want[k], cond[k]
        if rows is not None:
            if not poisoned(g[rows:]).all():
                fails.append(f"{k}: a row at or beyond the valid count {rows} was written")
            g, w, c = g[:rows], w[:rows], c[:rows]
        if k in ("enc", "ienc"):                   # a dead level's saved features hold row 0: not specified
            live = 2 * int(R.table_for(table)["num_levels"])
            g, w, c = g[:, :live], w[:, :live], c[:, :live]
        name = f"{table}/{entry}/M{M}.{k}"
        if R.tier_of(table) == "exact":
            if k == "cin":
                g, w = g[:, 16:], w[:, 16:]
            n = bit_mismatches(np.ascontiguousarray(g, F32), (w + 0.0).astype(F32))
            if n:
                i = int(np.flatnonzero(np.ascontiguousarray(g, F32).view(np.uint32).ravel() !=
                                       (w + 0.0).astype(F32).view(np.uint32).ravel())[0])
                fails.append(f"{name}: {n} of {w.size} elements differ in their bits, first at flat index {i}: "
                             f"{g.ravel()[i]!r} != {w.ravel()[i]!r}")
        else:
            r = R.worst_ratio(g, w, c)
            key = R.tol_key(entry, k)
            tol = R.TOL[build].get(key, 0.0)
            ratios[key] = max(ratios.get(key, 0.0), r)
            print(f"{name}: worst |got - ref| / cond {r:.3e}  (TOL[{key}] {tol:.3e})")
            if not r <= tol:
                fails.append(f"{name}: {r:.3e} > {tol:.3e}")
    return fails


def run_case(lib, table, entry, build, ratios, sizes=None):
    """Every size of one (table, entry point) -> list of failures."""
    fails = []
    for M in sizes or R.sizes_for(table, entry):
        got, sh = launch(lib, table, entry, M)
        fails += compare(table, entry, M, got, sh, build, ratios)
    return fails


def main():
    from instance_nerf_amd import _lib
    lib = _lib.load()
    build = os.environ.get("FIELD_FORWARD_BUILD", "fp32")
    ratios, fails = {}, []
    for table, entry in R.cases(build):
        fails += run_case(lib, table, entry, build, ratios, [M for M in R.sizes_for(table, entry) if M < R.BIG])
    print("RESULT " + json.dumps({"build": build, "failures": fails, "ratios": ratios}))


if __name__ == "__main__":
    main()
