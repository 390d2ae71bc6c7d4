"""The frame path's (t, ray id) sample records against the positions feed, on the GPU: writer, field, compositing and
the whole path.  Every comparison is exact (``torch.equal`` on int32 views / numpy uint32 views): the records feed
rebuilds position, dt and t - t_prev with the marcher's operations, so nothing may differ by a bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_records_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32 = torch.float32, torch.int32
H_GRID, MAX_STEPS = 128, 1024


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(I32), b.contiguous().view(I32))


_SCENES = {}


def _scene(bound):
    """-> (RoomScene(scale=bound), its bitfield on the device, cascade), built once per bound."""
    if bound not in _SCENES:
        from instance_nerf_amd.scene import RoomScene
        sc = RoomScene(scale=float(bound))
        _SCENES[bound] = (sc, _t(sc.density_bitfield(H_GRID, float(bound))), 1 + int(np.ceil(np.log2(max(bound, 1.0)))))
    return _SCENES[bound]


def _rays(bound, N, seed=0):
    """N rays of a 64x64 view from inside the room, patch order; ray 3 misses the box; with N >= 32 the rays 16..31 all
    miss it (a group with all counts zero)."""
    from instance_nerf_amd.nerf.utils import get_rays
    sc, _, _ = _scene(bound)
    poses, intr, H, W = sc.cameras(n=3, H=64, W=64, focal=32.0)
    r = get_rays(_t(poses[seed % 3:seed % 3 + 1]), intr, 64, 64, patch=4)
    ro, rd = r["rays_o"].view(-1, 3)[:N].clone(), r["rays_d"].view(-1, 3)[:N].clone()
    away_o = torch.tensor([0.0, 0.0, -3.0 * bound], device=DEV)
    away_d = torch.tensor([1.0, 0.0, 0.0], device=DEV)
    miss = [3] + (list(range(16, 32)) if N >= 32 else [])
    ro[miss], rd[miss] = away_o, away_d
    return ro.contiguous(), rd.contiguous()


class _Marched:
    """Both writers on the same rays (one count pass): positions feed (x01, ids, deltas) and records feed (t, ids)."""

    def __init__(self, bound, N, dt_gamma, noise, cap=None, M_short=0, seed=0):
        from instance_nerf_amd import _lib, raymarching as rm
        from instance_nerf_amd._lib import check, ptr, stream_ptr
        lib = _lib.load()
        _, bits, C = _scene(bound)
        self.bound, self.C, self.dt_gamma, self.N = float(bound), C, float(dt_gamma), N
        self.ro, self.rd = _rays(bound, N, seed)
        aabb = torch.tensor([-bound] * 3 + [bound] * 3, dtype=F32, device=DEV)
        self.nears, self.fars = rm.near_far_from_aabb(self.ro, self.rd, aabb, 0.05)
        self.noises = torch.rand(N, dtype=F32, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) if noise else None
        cap = rm.SAMPLE_CAP if cap is None else cap
        counter = torch.zeros(2, dtype=I32, device=DEV)
        self.rays = torch.empty(N, 3, dtype=I32, device=DEV)
        ws = torch.empty(lib.inr_march_workspace_bytes(N, cap) // 8 + 1, dtype=torch.int64, device=DEV)
        args = (ptr(self.ro), ptr(self.rd), ptr(bits, torch.uint8), float(bound), float(dt_gamma), MAX_STEPS, N, C, H_GRID)
        tail = (ptr(self.nears), ptr(self.fars), ptr(self.noises, allow_none=True), ptr(self.rays))
        check(lib.inr_march_rays_train_count(*args, *tail, ptr(counter), ptr(ws), cap, stream_ptr()), "count")
        self.total = int(counter[0].item())
        self.M = M = self.total - M_short
        # (filled with a pattern: rows of a dropped group must stay untouched in both)
        self.xyzs = torch.full((M, 3), -7.0, dtype=F32, device=DEV)
        self.deltas = torch.full((M, 2), -7.0, dtype=F32, device=DEV)
        self.ids = torch.full((M,), -7, dtype=I32, device=DEV)
        self.t = torch.full((M,), -7.0, dtype=F32, device=DEV)
        self.ids_rec = torch.full((M,), -7, dtype=I32, device=DEV)
        check(lib.inr_march_rays_patch_write(*args, M, *tail, ptr(self.xyzs, allow_none=M == 0), None,
                                             ptr(self.deltas, allow_none=M == 0), ptr(ws), cap,
                                             ptr(self.ids, allow_none=M == 0), 1, stream_ptr()), "write")
        check(lib.inr_march_rays_patch_write_records(*args, M, *tail, ptr(self.t, allow_none=M == 0),
                                                     ptr(self.ids_rec, allow_none=M == 0), ptr(ws), cap, stream_ptr()),
              "write_records")
        torch.cuda.synchronize()
        self.records = rm.MarchRecords(self.nears, self.noises, dt_gamma, MAX_STEPS, C, H_GRID)


# (bound, N, dt_gamma, noise, cap, M_short)
WRITER_CASES = [
    (1, 16, 0.0, False, None, 0), (1, 17, 0.0, True, None, 0), (1, 40, 0.0, False, None, 0),
    (1, 4096, 0.0, True, None, 0),
    (1, 40, 0.0, True, 32, 0),               # capture row of 32 candidates: most rays run past it and are marched again
    (2, 40, 0.0, False, None, 0), (2, 40, 1.0 / 128, True, None, 0), (2, 4096, 1.0 / 128, False, None, 0),
    (2, 40, 1.0 / 128, True, 32, 0),
    (1, 40, 0.0, True, None, 5),             # M five short: the last group is dropped whole in both
]
_CACHE = {}


def _marched(case):
    if case not in _CACHE:
        _CACHE[case] = _Marched(*case)
    return _CACHE[case]


def _written_rows(m):
    """bool [M]: rows some kept group owns (a group that does not fit in M is dropped whole)."""
    from instance_nerf_amd.raymarching import GROUP
    r = m.rays.cpu().numpy().astype(np.int64)
    own = np.zeros(m.M, bool)
    for g0 in range(0, m.N, GROUP):
        tot = int(r[g0:g0 + GROUP, 2].sum())
        if tot and r[g0, 1] + tot <= m.M:
            own[r[g0, 1]:r[g0, 1] + tot] = True
    return own


@pytest.mark.parametrize("case", WRITER_CASES, ids=lambda c: "b%d-N%d-g%.4f-n%d-cap%s-short%d" % c)
def test_writer_records_rebuild_the_positions_feed(case):
    m = _marched(case)
    cnt = m.rays[:, 2].cpu().numpy()
    assert m.total > 0 and cnt[3] == 0 and (m.N < 32 or not cnt[16:32].any())
    assert len(set(cnt[:16].tolist())) > 2                         # counts differ inside a group
    own = _written_rows(m)
    assert own.any() and (case[5] == 0) == bool(own.all())
    assert torch.equal(m.ids, m.ids_rec)
    ids = m.ids.cpu().numpy()
    t = m.t.cpu().numpy()
    assert (ids[~own] == -7).all() and (t[~own] == -7.0).all() and (m.xyzs.cpu().numpy()[~own] == -7.0).all()
    # positions from t: un-fused float32 numpy operations
    o, d = m.ro.cpu().numpy(), m.rd.cpu().numpy()
    rid = ids[own]
    x01 = ref.x01_div(ref.position(o[rid], d[rid], t[own], m.bound), m.bound)
    assert np.array_equal(ref.bits(x01), ref.bits(m.xyzs.cpu().numpy()[own]))
    assert np.array_equal(ref.bits(ref.x01_mul(ref.position(o[rid], d[rid], t[own], m.bound), m.bound)), ref.bits(x01))
    # (dt, t - t_prev) from t, ray by ray in sample order
    if case[5] == 0:
        from instance_nerf_amd.raymarching import patch_slots
        slots = patch_slots(m.rays).numpy()
        tr = t[slots]
        dt = ref.step_dt(tr, m.dt_gamma, MAX_STEPS, m.C, H_GRID)
        tn = (tr + dt).astype(np.float32)
        t0 = ref.start_t(m.nears.cpu().numpy(), None if m.noises is None else m.noises.cpu().numpy(), m.dt_gamma,
                         MAX_STEPS, m.C, H_GRID)
        last = np.concatenate([[np.float32(0)], tn[:-1]]).astype(np.float32)
        first = np.cumsum(cnt) - cnt                               # ray-major offset of every ray's first sample
        last[first[cnt > 0]] = t0[cnt > 0]
        want = np.stack([dt, (tn - last).astype(np.float32)], -1)
        assert np.array_equal(ref.bits(want), ref.bits(m.deltas.cpu().numpy()[slots]))
    if case[4] == 32:
        # some rays did run past the capture row (they are marched again): they own a sample behind their 32nd candidate
        t0 = ref.start_t(m.nears.cpu().numpy(), None if m.noises is None else m.noises.cpu().numpy(), m.dt_gamma,
                         MAX_STEPS, m.C, H_GRID)
        c32 = t0.copy()
        for _ in range(32):
            c32 = (c32 + ref.step_dt(c32, m.dt_gamma, MAX_STEPS, m.C, H_GRID)).astype(np.float32)
        assert (t[own] >= c32[rid]).any()


@pytest.mark.parametrize("K", [0, 16])
@pytest.mark.parametrize("case", WRITER_CASES, ids=lambda c: "b%d-N%d-g%.4f-n%d-cap%s-short%d" % c)
def test_compositing_records_equal_positions(case, K):
    from instance_nerf_amd import raymarching as rm
    m = _marched(case)
    g = torch.Generator(DEV).manual_seed(11)
    sig = torch.rand(m.M, dtype=F32, device=DEV, generator=g) * 50.0       # some rays cross T_thresh mid-ray
    rgb = torch.rand(m.M, 3, dtype=F32, device=DEV, generator=g)
    extra = torch.randn(m.M, K, dtype=F32, device=DEV, generator=g) if K else None
    outs = []
    for deltas, rec in ((m.deltas, None), (m.t, m.records)):
        skip = torch.zeros(1, dtype=torch.int64, device=DEV)
        out = rm.composite_rays_patch(sig, rgb, deltas, m.rays, 1e-4, extra=extra, return_weights=True, skippable=skip,
                                      records=rec)
        outs.append(tuple(out) + (skip,))
    torch.cuda.synchronize()
    assert len(outs[0]) == len(outs[1]) == (6 if K else 5)
    own = torch.from_numpy(_written_rows(m)).to(DEV)
    for i, (a, b) in enumerate(zip(*outs)):
        if i == len(outs[0]) - 2:
            a, b = a[:m.M][own], b[:m.M][own]                      # the weights buffer: rows of a dropped group are not written
        assert _same(a, b) if a.dtype == F32 else torch.equal(a, b), i
    ws = outs[0][0]
    if m.M > 1000:
        assert int((ws > 0.9999).sum()) > 0 and int(outs[0][-1][0]) >= 0


@pytest.fixture(scope="module")
def frame_samples():
    """Both feeds of one 256x256 view at bound 1 (~3 M samples): (x01, t, ids, ro, rd)."""
    from instance_nerf_amd import raymarching as rm
    from instance_nerf_amd.nerf.utils import get_rays
    sc, bits, C = _scene(1)
    poses, intr, H, W = sc.cameras(n=1, H=256, W=256, focal=128.0)
    r = get_rays(_t(poses[:1]), intr, 256, 256, patch=4)
    ro, rd = r["rays_o"].view(-1, 3).contiguous(), r["rays_d"].view(-1, 3).contiguous()
    aabb = torch.tensor([-1.0] * 3 + [1.0] * 3, dtype=F32, device=DEV)
    nears, fars = rm.near_far_from_aabb(ro, rd, aabb, 0.05)
    x01, ids, _, rays = rm.march_rays_patch(ro, rd, 1.0, bits, C, H_GRID, nears, fars, 0.0, MAX_STEPS, table=True)
    t, ids2, none, rays2 = rm.march_rays_patch(ro, rd, 1.0, bits, C, H_GRID, nears, fars, 0.0, MAX_STEPS, table="records")
    assert none is None and torch.equal(ids, ids2) and torch.equal(rays, rays2) and t.shape[0] >= (1 << 19) + 3
    return x01, t, ids, ro, rd


@pytest.fixture(scope="module")
def field_net(params_k16):
    from instance_nerf_amd.nerf import NeRFNetwork
    net = NeRFNetwork(cuda_ray=True, num_instances=0, min_near=0.05).to(DEV).eval()       # table U(-1,1): every level matters
    net.load_state_dict({"encoder.embeddings": params_k16["embeddings"], "sigma_net.0.weight": params_k16["sigma_w0"],
                         "sigma_net.1.weight": params_k16["sigma_w1"], "color_net.0.weight": params_k16["color_w0"],
                         "color_net.1.weight": params_k16["color_w1"], "color_net.2.weight": params_k16["color_w2"]},
                        strict=False)
    return net


@pytest.mark.parametrize("half_table,mlp_fp16", [(False, False), (True, False), (False, True), (True, True)])
def test_field_records_equal_positions(frame_samples, field_net, half_table, mlp_fp16):
    x01, t, ids, ro, rd = frame_samples
    net = field_net
    net.half_table, net.mlp_fp16, net.frame_slices = half_table, mlp_fp16, False
    try:
        with torch.no_grad():
            shq, rows = net.sh_table(rd), net.ray_table(ro, rd)
            assert _same(rows[:, :16], shq)
            for M in (0, 1, 15, 16, 17, 16 * 1024 + 5, (1 << 19) + 3):      # the last: XCD-interleaved, cursor-drawn schedule
                want = net.forward_table(x01[:M].contiguous(), ids[:M].contiguous(), rd, shq=shq)
                got = net.forward_table(t[:M].contiguous(), ids[:M].contiguous(), rd, shq=rows, rays_o=ro)
                torch.cuda.synchronize()
                assert got[0].shape == (M,) and got[1].shape == (M, 3)
                assert _same(got[0], want[0]) and _same(got[1], want[1]), M
            got = net.forward_table(t[:1000].contiguous(), ids[:1000].contiguous(), rd, rays_o=ro)   # builds its own rows
            want = net.forward_table(x01[:1000].contiguous(), ids[:1000].contiguous(), rd)
            assert _same(got[0], want[0]) and _same(got[1], want[1])
    finally:
        net.half_table, net.mlp_fp16 = False, False


def test_field_records_refuse_other_bounds(frame_samples, params_k16):
    from instance_nerf_amd import _lib
    x01, t, ids, ro, rd = frame_samples
    lib = _lib.load()
    from instance_nerf_amd._lib import ptr
    sig, rgb = torch.empty(16, device=DEV), torch.empty(16, 3, device=DEV)
    rc = lib.inr_nerf_forward_table_records(ptr(t), ptr(ids, I32), ptr(torch.zeros(4, 24, device=DEV)), 16, 1.5, None, None,
                                      None, 1.0, ptr(sig), ptr(rgb), 0, None)
    assert rc != 0


def _net_for(bound, K, params_k16):
    from instance_nerf_amd.nerf import NeRFNetwork
    p = params_k16
    net = NeRFNetwork(cuda_ray=True, num_instances=K, min_near=0.05, bound=bound).to(DEV).eval()
    sd = {"sigma_net.0.weight": p["sigma_w0"], "sigma_net.1.weight": p["sigma_w1"],
          "color_net.0.weight": p["color_w0"], "color_net.1.weight": p["color_w1"], "color_net.2.weight": p["color_w2"]}
    if K:
        sd.update({"instance_encoder.embeddings": p["inst_embeddings"], "instance_net.0.weight": p["inst_w0"],
                   "instance_net.1.weight": p["inst_w1"], "instance_net.2.weight": p["inst_w2"]})
    if bound == 1:
        sd["encoder.embeddings"] = p["embeddings"]
    net.load_state_dict(sd, strict=False)
    if bound != 1:              # the table of another bound has other level sizes: U(-1,1) here as well
        with torch.no_grad():
            net.encoder.embeddings.uniform_(-1.0, 1.0, generator=torch.Generator(DEV).manual_seed(4))
    net.density_scale = 0.3                                         # table U(-1,1): keep the rays semi-transparent
    sc, bits, _ = _scene(bound)
    net.density_bitfield.copy_(bits)
    return net, sc


@pytest.mark.parametrize("bound,K,feed", [(1, 0, "records"), (2, 0, "records"), (1.5, 0, "positions"), (1, 16, "positions")])
def test_whole_path_records_equal_forced_positions(params_k16, bound, K, feed):
    """Three 64x64 views through FramePipeline: the records feed against the forced positions feed, every output
    tensor identical; a bound whose double is no power of two and a network with instances stay on positions."""
    from instance_nerf_amd.nerf.renderer import FramePipeline
    from instance_nerf_amd.nerf.utils import get_rays
    net, sc = _net_for(bound, K, params_k16)
    assert net.frame_records is True
    poses, intr, H, W = sc.cameras(n=3, H=64, W=64, focal=32.0)
    rays = [get_rays(_t(poses[v:v + 1]), intr, 64, 64, patch=4) for v in range(3)]
    dt_gamma = 0.0 if bound == 1 else 1.0 / 128

    def run():
        pipe = FramePipeline(net)
        with torch.no_grad():
            outs = [pipe.render(r["rays_o"], r["rays_d"], bg_color=1, infer_mode="fused", dt_gamma=dt_gamma) for r in rays]
        pipe.close()
        torch.cuda.synchronize()
        return outs
    got = run()
    net.frame_records = False
    want = run()
    for a, b in zip(got, want):
        assert a["frame_feed"] == feed and b["frame_feed"] == "positions" and a["frame_path"] == b["frame_path"] == "fused"
        tensors = [k for k, v in b.items() if torch.is_tensor(v)]
        assert {"image", "depth", "weights_sum", "num_samples"} <= set(tensors) and (("instance" in tensors) == bool(K))
        assert sorted(k for k, v in a.items() if torch.is_tensor(v)) == sorted(tensors)
        for k in tensors:
            assert a[k].dtype == b[k].dtype and (_same(a[k], b[k]) if a[k].dtype == F32 else torch.equal(a[k], b[k])), k
        assert int(a["num_samples"][0]) > 50_000
