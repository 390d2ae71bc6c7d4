"""Seeded inputs and raw launches of the fused field kernels (csrc/field_fused.hip) for the bit-identity fixture
tests/golden/field_issue_path.npz: tests/golden/make_field_issue_golden.py records what a build computes,
tests/test_field_issue_path.py asserts that the current build computes the same BITS.

Everything is derived from seeds with numpy's PCG64 (stable across numpy versions for `random` / `integers`), nothing
from the GPU; the kernels are called through the C ABI directly, so that every template instantiation is reached
whatever the Python layer would choose.

Level tables - one per class of coarse slot (levels 0..7; lane q of a sample owns levels 2q, 2q+1):
  dense_coarse  every coarse level dense, every fine level hashed       (xor-only fine instantiation)
  hashed_all    every level hashed (2^12 rows)                          (xor-only fine instantiation)
  bench         base 16, finest 2048, 2^19 rows: levels 0..4 dense, 5.. hashed - dense and hashed lanes in BOTH coarse slots
  all_dense     every level dense                                       (generic fine instantiation)
  levels12      12 levels: dead records in the fine slots               (generic fine instantiation)
  levels5       5 levels: dead records in the coarse slots too
"""
import ctypes
import functools
import hashlib

import numpy as np
import torch

from instance_nerf_amd import _lib
from instance_nerf_amd.gridencoder import level_table

SIZES = (1, 15, 16, 17, 16 * 61 + 7)      # one lane, ragged tiles on both sides of 16, 62 tiles with a ragged last one
BIG = SIZES[-1]
RAW_AT_BIG = ("table", "table_zero_g")    # at M = BIG only these kernels' outputs are kept as raw bits (file size)

TABLES = {
    "dense_coarse": dict(base_resolution=4, desired_resolution=2048, log2_hashmap_size=19),
    "hashed_all": dict(base_resolution=16, desired_resolution=2048, log2_hashmap_size=12),
    "bench": dict(base_resolution=16, desired_resolution=2048, log2_hashmap_size=19),
    "all_dense": dict(base_resolution=4, desired_resolution=64, log2_hashmap_size=19),
    "levels12": dict(num_levels=12, base_resolution=16, desired_resolution=1024, log2_hashmap_size=19),
    "levels5": dict(num_levels=5, base_resolution=16, desired_resolution=128, log2_hashmap_size=19),
}
SLICED_TABLES = ("dense_coarse", "hashed_all", "bench")       # 16 levels, levels 8..15 hashed

# kernel -> what it instantiates
KERNELS = (
    "fwd_rgb",          # k_nerf_fwd<true>                          plain feed, colour
    "fwd_density",      # k_nerf_fwd<false>                         plain feed, no colour, geo features
    "fwd_o",            # k_nerf_fwd<true,false,0,true,true>        plain feed, kHalf + kFast
    "table",            # k_nerf_fwd<true,true>                     table feed (the benchmark's kernel)
    "table_half",       # k_nerf_fwd<true,true,0,true,false>
    "table_fast",       # k_nerf_fwd<true,true,0,false,true>
    "table_o",          # k_nerf_fwd<true,true,0,true,true>
    "table_sliced",     # k_grid_fine_slices + k_nerf_fwd<true,true,0,false,false,true>   (SLICED_TABLES only)
    "train_save1",      # k_nerf_fwd<true,false,1>
    "train_save2",      # k_nerf_fwd<true,false,2>
    "instance16",       # k_instance_fwd<1>
    "instance64",       # k_instance_fwd<4>
    "dirs",             # k_nerf_fwd_dirs<false>
    "table_zero_g",     # "table" with an all-zero green row in the last colour layer: pre-activation exactly 0
)
RENDER_TABLES = ("bench", "hashed_all")
RENDER_KERNELS = ("nerf_render", "nerf_render_o", "instance_render16", "instance_render48")


def table_for(name):
    return level_table(**TABLES[name])


def applies(table, kernel):
    return kernel != "table_sliced" or table in SLICED_TABLES


def sizes_for(kernel):
    return (17, BIG) if kernel == "table_zero_g" else SIZES


def _rng(*key):
    return np.random.default_rng([int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:4], "little")])


def _uniform(rng, shape, lo, hi):
    return (rng.random(shape, dtype=np.float32) * np.float32(hi - lo) + np.float32(lo)).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _weights(rng, rows, cols, scale):
    return _uniform(rng, (rows, cols), -scale, scale)


class State:
    """One level table on the device: embeddings (fp32 and the fp16 copy), descriptor, packed weights."""

    def __init__(self, name):
        lib = _lib.load()
        self.name = name
        self.table = table_for(name)
        self.desc = _lib.make_grid_desc(self.table)
        rows = int(self.table["total_rows"])
        emb = _uniform(_rng("emb", name), (rows, 2), -1.0, 1.0)
        self.emb = _dev(emb)
        self.emb_half = _dev(emb.astype(np.float16))
        r = _rng("weights", name)
        self.nerf_w = [_weights(r, 64, 32, 0.35), _weights(r, 16, 64, 0.25), _weights(r, 64, 31, 0.35),
                       _weights(r, 64, 64, 0.25), _weights(r, 3, 64, 0.25)]
        self.packed = {n: self._pack_nerf(lib, self.nerf_w, n) for n in (0, _lib.NUMERICS_MLP_F16)}
        zero_g = [w.copy() for w in self.nerf_w]
        zero_g[4][1, :] = 0.0
        zero_g[4][0, :] = -np.abs(zero_g[4][0, :])        # red: mostly negative pre-activations
        self.packed_zero_g = self._pack_nerf(lib, zero_g, 0)
        self.inst_packed = {}
        for K in (16, 48, 64):
            w = [_weights(r, 64, 32, 0.35), _weights(r, 64, 64, 0.25), _weights(r, K, 64, 0.25)]
            for n in (0, _lib.NUMERICS_MLP_F16):
                buf = np.zeros(lib.inr_instance_packed_floats(K), np.float32)
                _lib.check(lib.inr_instance_pack_weights(*[a.ctypes.data for a in w], K, buf.ctypes.data, n), "pack")
                self.inst_packed[K, n] = _dev(buf)

    @staticmethod
    def _pack_nerf(lib, ws, numerics):
        buf = np.zeros(lib.inr_nerf_packed_floats(), np.float32)
        _lib.check(lib.inr_nerf_pack_weights(*[a.ctypes.data for a in ws], buf.ctypes.data, numerics), "pack")
        return _dev(buf)


@functools.lru_cache(maxsize=1)
def state(name):
    return State(name)


def points(table, M, unit):
    """[M,3] positions: unit False -> [-1,1] (bound 1, plain feed), True -> [0,1] (table feed).  The first rows are
    faces and centres of the volume and cell boundaries of level 0 and of the finest level; one row of the plain feed
    lies outside the volume."""
    rng = _rng("x", table, M, unit)
    x = _uniform(rng, (M, 3), 0.0, 1.0)
    t = table_for(table)
    s0, s1 = float(t["scales"][0]), float(t["scales"][-1])
    special = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1, 0, 0.25],
               [np.float32(2.5) / np.float32(s0), np.float32(0.5) / np.float32(s0), np.float32(7.5) / np.float32(s0)],
               [np.float32(np.floor(0.8 * s1) + 0.5) / np.float32(s1), np.float32(3.5) / np.float32(s1), 0.0],
               [0.03125, 0.96875, 0.5]]
    n = min(M, len(special))
    x[:n] = np.asarray(special[:n], np.float32)
    if not unit:
        x = (x * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
        if M > 9:
            x[9] = [1.5, 0.0, 0.0]
    return x


def dirs_for(table, M):
    d = _uniform(_rng("d", table, M), (M, 3), -1.0, 1.0) + np.float32(1e-3)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _sp():
    return _lib.stream_ptr()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _empty(*shape):
    return torch.zeros(*shape, dtype=torch.float32, device="cuda")


def run(table, kernel, M):
    """-> dict output name -> numpy array (float32 viewed as uint32 by the caller)."""
    lib = _lib.load()
    st = state(table)
    O = _lib.NUMERICS_TABLE_F16 | _lib.NUMERICS_MLP_F16
    out = {}
    if kernel in ("fwd_rgb", "fwd_density", "fwd_o"):
        x, d = _dev(points(table, M, False)), _dev(dirs_for(table, M))
        numerics = O if kernel == "fwd_o" else 0
        rgb = None if kernel == "fwd_density" else _empty(M, 3)
        geo = _empty(M, 15) if kernel == "fwd_density" else None
        sigma = _empty(M)
        emb = st.emb_half if numerics else st.emb
        _lib.check(lib.inr_nerf_forward(_p(x), None if rgb is None else _p(d), M, None, 1.0, _p(emb), st.desc,
                                        _p(st.packed[numerics & _lib.NUMERICS_MLP_F16]), 1.0, _p(sigma), _p(rgb), _p(geo),
                                        numerics, _sp()), kernel)
        out = {"sigma": sigma, "rgb": rgb, "geo": geo}
    elif kernel.startswith("table"):
        x01 = _dev(points(table, M, True))
        n_rays = max(1, M // 5)
        rng = _rng("rays", table, M)
        ray_ids = _dev(np.sort(rng.integers(0, n_rays, size=M)).astype(np.int32))
        shq = _dev(_uniform(rng, (n_rays, 16), -1.0, 1.0))
        sigma, rgb = _empty(M), _empty(M, 3)
        if kernel == "table_sliced":
            ws = _empty(lib.inr_nerf_forward_table_sliced_workspace_bytes(M) // 4)
            _lib.check(lib.inr_nerf_forward_table_sliced(_p(x01), _p(ray_ids), _p(shq), M, 1.0, _p(st.emb), st.desc,
                                                         _p(st.packed[0]), 1.0, _p(sigma), _p(rgb), _p(ws), _sp()), kernel)
        else:
            numerics = {"table": 0, "table_zero_g": 0, "table_half": _lib.NUMERICS_TABLE_F16,
                        "table_fast": _lib.NUMERICS_MLP_F16, "table_o": O}[kernel]
            packed = st.packed_zero_g if kernel == "table_zero_g" else st.packed[numerics & _lib.NUMERICS_MLP_F16]
            emb = st.emb_half if numerics & _lib.NUMERICS_TABLE_F16 else st.emb
            _lib.check(lib.inr_nerf_forward_table(_p(x01), _p(ray_ids), _p(shq), M, 1.0, _p(emb), st.desc, _p(packed), 1.0,
                                                  _p(sigma), _p(rgb), numerics, _sp()), kernel)
        out = {"sigma": sigma, "rgb": rgb}
    elif kernel in ("train_save1", "train_save2"):
        x, d = _dev(points(table, M, False)), _dev(dirs_for(table, M))
        sigma, rgb, enc = _empty(M), _empty(M, 3), _empty(M, 32)
        if kernel == "train_save1":
            acts = {"h1": _empty(M, 64), "so": _empty(M, 16), "cin": _empty(M, 32), "c1": _empty(M, 64), "c2": _empty(M, 64)}
            _lib.check(lib.inr_nerf_forward_train(_p(x), _p(d), M, 1.0, _p(st.emb), st.desc, _p(st.packed[0]), _p(sigma),
                                                  _p(rgb), _p(enc), _p(acts["h1"]), _p(acts["so"]), _p(acts["cin"]),
                                                  _p(acts["c1"]), _p(acts["c2"]), _sp()), kernel)
            saved = torch.cat([enc] + [acts[k] for k in ("h1", "so", "cin", "c1", "c2")], dim=1)
        else:
            _lib.check(lib.inr_nerf_forward_enc(_p(x), _p(d), M, 1.0, _p(st.emb), st.desc, _p(st.packed[0]), _p(sigma),
                                                _p(rgb), _p(enc), _sp()), kernel)
            saved = enc
        out = {"sigma": sigma, "rgb": rgb, "saved": saved}
    elif kernel in ("instance16", "instance64"):
        K = int(kernel[len("instance"):])
        x = _dev(points(table, M, False))
        logits = _empty(M, K)
        _lib.check(lib.inr_instance_forward(_p(x), M, None, 1.0, _p(st.emb), st.desc, _p(st.inst_packed[K, 0]), K,
                                            _p(logits), _sp()), kernel)
        out = {"logits": logits}
    elif kernel == "dirs":
        x = _dev(points(table, M, False))
        sh = _dev(_uniform(_rng("shdirs", table), (3, 16), -1.0, 1.0))
        o4 = _empty(M, 4)
        _lib.check(lib.inr_nerf_forward_dirs(_p(x), M, 1.0, _p(st.emb), st.desc, _p(st.packed[0]), _p(sh), 3, _p(o4),
                                             _sp()), kernel)
        out = {"rgb_logit": o4}
    else:
        raise KeyError(kernel)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def run_render(table, kernel):
    """One launch of a rendering kernel over 37 rays (two full 16-ray groups and a ragged one) in the patch-interleaved
    layout: the samples of a group step by step, the rays that still have a sample at that step in ray order."""
    lib = _lib.load()
    st = state(table)
    O = _lib.NUMERICS_TABLE_F16 | _lib.NUMERICS_MLP_F16
    rng = _rng("render", table)
    N = 37
    cnt = rng.integers(0, 20, size=N).astype(np.int32)
    cnt[3] = 0
    rays = np.zeros((N, 3), np.int32)
    rays[:, 0] = rng.permutation(N)
    rays[:, 2] = cnt
    base = 0
    for g in range(0, N, 16):
        rays[g:g + 16, 1] = base
        base += int(cnt[g:g + 16].sum())
    M = base
    unit = kernel != "nerf_render_o"                                   # one launch takes the un-normalised feed
    x = _uniform(rng, (M, 3), 0.0, 1.0) if unit else _uniform(rng, (M, 3), -1.0, 1.0)
    deltas = np.stack([_uniform(rng, (M,), 0.005, 0.05), _uniform(rng, (M,), 0.005, 0.05)], -1)
    rays_d = dirs_for(table, N)
    # every device tensor of a launch keeps a name until the launch has been waited for: a temporary would go back to
    # the caching allocator while the arguments are still being put together, and the next upload could land in it
    xd, rd, deltas_d, rays_d_d = _dev(x), _dev(rays), _dev(deltas), _dev(rays_d)
    if kernel.startswith("nerf_render"):
        numerics = O if kernel == "nerf_render_o" else 0
        ws, depth, image, w = _empty(N), _empty(N), _empty(N, 3), _empty(M)
        evaluated = torch.zeros(33, dtype=torch.int64, device="cuda")
        emb = st.emb_half if numerics else st.emb
        _lib.check(lib.inr_nerf_render(_p(xd), _p(deltas_d), _p(rd), _p(rays_d_d), N, M, 1.0, _p(emb), st.desc,
                                       _p(st.packed[numerics & _lib.NUMERICS_MLP_F16]), 1.0, 1e-4, _p(ws), _p(depth),
                                       _p(image), _p(w), _p(evaluated), 1 if unit else 0, numerics, _sp()), kernel)
        out = {"weights_sum": ws, "depth": depth, "image": image, "weights": w, "evaluated": evaluated[:1].float()}
    else:
        K = int(kernel[len("instance_render"):])
        w = _uniform(rng, (M,), 0.0, 1.0)
        w[rng.random(M) < 0.3] = 0.0
        w_d = _dev(w)
        res = _empty(N, K)
        cursors = torch.zeros(32, dtype=torch.int64, device="cuda")
        _lib.check(lib.inr_instance_render(_p(xd), _p(rd), _p(w_d), N, M, 1.0, _p(st.emb), st.desc,
                                           _p(st.inst_packed[K, 0]), K, _p(res), 1, _p(cursors), 0, _sp()), kernel)
        out = {"logits": res}
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(outputs, kernel, M):
    """What the fixture keeps of one launch: the raw bits of every output (float32 as uint32).  To keep the file small,
    the saved training activations always, and at M = BIG every output of a kernel outside RAW_AT_BIG, are kept as the
    SHA-256 of those bits instead."""
    rec = {}
    for k, a in outputs.items():
        a = np.ascontiguousarray(a, np.float32)
        if k == "saved" or (M == BIG and kernel not in RAW_AT_BIG):
            rec[k + ".sha256"] = np.asarray(digest(a))
        else:
            rec[k] = a.view(np.uint32)
    return rec


def all_cases():
    """(key, thunk) of every launch of the fixture; key = table/kernel/M or table/kernel."""
    for t in TABLES:
        for k in KERNELS:
            if not applies(t, k):
                continue
            for M in sizes_for(k):
                yield f"{t}/{k}/{M}", (lambda t=t, k=k, M=M: record(run(t, k, M), k, M))
    for t in RENDER_TABLES:
        for k in RENDER_KERNELS:
            yield f"{t}/{k}", (lambda t=t, k=k: record(run_render(t, k), k, 0))
