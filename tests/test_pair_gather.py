"""The pair front end of the frame's field kernel (k_nerf_fwd_pair: two tiles per gather pass, two lanes per sample)
against k_nerf_fwd on the same inputs, on the GPU.  INR_FIELD_PAIR=0 in the environment selects k_nerf_fwd for the
launches the pair kernel would take; the library reads it at every launch.  Every comparison is on the bits.

(There is no case with a device-side sample count below M: inr_nerf_forward_table_records has no such argument - a
records launch always evaluates M samples - so no such launch exists to compare.)

That the records feed - the pair kernel by default - equals the positions feed bit for bit, up to cursor-drawn launch
sizes, is tests/test_sample_records.py::test_field_records_equal_positions."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32 = torch.float32, torch.int32
H_GRID, MAX_STEPS = 128, 1024
GUARD = 64
# 32 samples per pair; the XCD-interleaved, cursor-drawn schedule starts at 4 rounds of 8 chunks of 1024 tiles.  The last
# size: 4 complete rounds, one more chunk and a single tile behind it - an odd tile count, the last sample row ragged.
M_CHUNKS = (4 * 8192 + 1024 + 1) * 16 - 5
SIZES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, M_CHUNKS]


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


class _Switch:
    """INR_FIELD_PAIR for the duration of a block; the previous value afterwards."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("INR_FIELD_PAIR")
        if self.on:
            os.environ.pop("INR_FIELD_PAIR", None)
        else:
            os.environ["INR_FIELD_PAIR"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("INR_FIELD_PAIR", None)
        else:
            os.environ["INR_FIELD_PAIR"] = self.old


@pytest.fixture(scope="module")
def net(params_k16, room_bitfield):
    from instance_nerf_amd.nerf import NeRFNetwork
    p = params_k16
    n = NeRFNetwork(cuda_ray=True, num_instances=0, min_near=0.05).to(DEV).eval()       # table U(-1,1): every level matters
    n.load_state_dict({"encoder.embeddings": p["embeddings"], "sigma_net.0.weight": p["sigma_w0"],
                       "sigma_net.1.weight": p["sigma_w1"], "color_net.0.weight": p["color_w0"],
                       "color_net.1.weight": p["color_w1"], "color_net.2.weight": p["color_w2"]}, strict=False)
    n.density_bitfield.copy_(_t(room_bitfield))
    n.density_scale = 0.3
    assert n.encoder.desc.num_levels == 16 and all(n.encoder.desc.hashed[l] for l in range(8, 16))   # the launch qualifies
    return n


@pytest.fixture(scope="module")
def marched(net, room, room_bitfield):
    """One 160x160 view of the room marched in patch order with the records writer: consecutive 16-sample tiles are
    consecutive steps of the same 4x4 patch of rays.  -> (t [M], ray ids [M], ray rows [N, 24])"""
    from instance_nerf_amd import raymarching as rm
    from instance_nerf_amd.nerf.utils import get_rays
    poses, intr, H, W = room.cameras(n=1, H=160, W=160, focal=80.0)
    r = get_rays(_t(poses[:1]), intr, 160, 160, patch=4)
    ro, rd = r["rays_o"].view(-1, 3).contiguous(), r["rays_d"].view(-1, 3).contiguous()
    aabb = torch.tensor([-1.0] * 3 + [1.0] * 3, dtype=F32, device=DEV)
    nears, fars = rm.near_far_from_aabb(ro, rd, aabb, 0.05)
    t, ids, none, rays = rm.march_rays_patch(ro, rd, 1.0, _t(room_bitfield), 1, H_GRID, nears, fars, 0.0, MAX_STEPS,
                                             table="records")
    assert none is None and t.shape[0] >= M_CHUNKS
    # pairs really are consecutive steps: inside the first rays' run, slot m + 16 is the same ray one step on
    same = ids[:4096 - 16] == ids[16:4096]
    assert float(same.float().mean()) > 0.8
    with torch.no_grad():
        rows = net.ray_table(ro, rd)
    return t.contiguous(), ids.contiguous(), rows


@pytest.fixture(scope="module")
def unrelated(marched):
    """Samples that share nothing: a random ray and a random t each (positions are clamped to the volume)."""
    _, _, rows = marched
    g = torch.Generator(DEV).manual_seed(3)
    M = 4 * 8192 * 16 + 16 * 7 + 3          # cursor-drawn, odd tile count
    ids = torch.randint(0, rows.shape[0], (M,), device=DEV, generator=g, dtype=torch.int64).to(I32)
    t = torch.rand(M, dtype=F32, device=DEV, generator=g) * 3.0 + 0.05
    return t, ids, rows


def _launch(net, t, ids, rows, M, pair):
    """inr_nerf_forward_table_records on the first M samples into guarded, NaN-poisoned buffers -> (sigma, rgb) whole."""
    from instance_nerf_amd import _lib
    from instance_nerf_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    sig = torch.full((M + 2 * GUARD,), float("nan"), dtype=F32, device=DEV)
    rgb = torch.full((3 * M + 2 * GUARD,), float("nan"), dtype=F32, device=DEV)
    with _Switch(pair):
        check(lib.inr_nerf_forward_table_records(ptr(t), ptr(ids, I32), ptr(rows), M, float(net.bound),
                                                 net._table_ptr(net.encoder, 0), net.encoder.desc,
                                                 ptr(net._packed_weights("nerf", 0)), 0.3, ptr(sig[GUARD:GUARD + M]),
                                                 ptr(rgb[GUARD:GUARD + 3 * M]), 0, stream_ptr()), "nerf_forward_table_records")
        torch.cuda.synchronize()
    return sig, rgb


def _check(net, t, ids, rows, M):
    old = _launch(net, t, ids, rows, M, pair=False)
    new = _launch(net, t, ids, rows, M, pair=True)
    for a, b, n in zip(old, new, (M, 3 * M)):
        assert torch.equal(a.view(I32), b.view(I32))                                        # outputs and guards, bit for bit
        assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + n:]).all())  # guards intact
        assert not bool(torch.isnan(b[GUARD:GUARD + n]).any())                              # every row written
    assert float(new[0][GUARD:GUARD + M].abs().max()) > 0


@pytest.mark.parametrize("M", SIZES)
def test_pair_kernel_equals_tile_kernel_on_marched_samples(net, marched, M):
    t, ids, rows = marched
    _check(net, t, ids, rows, M)


@pytest.mark.parametrize("M", [49, None])
def test_pair_kernel_equals_tile_kernel_on_unrelated_samples(net, unrelated, M):
    t, ids, rows = unrelated
    _check(net, t, ids, rows, t.shape[0] if M is None else M)


def test_frames_are_the_same_with_the_pair_kernel_on_and_off(net, room, tmp_path):
    """Three 64x64 views through Trainer.render_sequence (FramePipeline, records feed): every output array_equal."""
    from instance_nerf_amd.nerf.utils import Trainer, get_rays
    poses, intr, H, W = room.cameras(n=3, H=64, W=64, focal=32.0)
    views = []
    for v in range(3):
        r = get_rays(_t(poses[v:v + 1]), intr, H, W)
        views.append({"rays_o": r["rays_o"], "rays_d": r["rays_d"], "H": H, "W": W, "images": torch.rand(1, H, W, 3, device=DEV)})
    tr = Trainer("pair", None, net, stage="nerf", device=torch.device(DEV), workspace=str(tmp_path), use_checkpoint="scratch",
                 mute=True)
    net.eval()

    def run(pair):
        with _Switch(pair):
            outs = [{k: v.clone() for k, v in o.items() if torch.is_tensor(v)} for _, o in tr.render_sequence(views)]
            torch.cuda.synchronize()
        assert net.last_frame_path == "fused" and net.last_frame_feed == "records"
        return outs
    run(True)                                # (a network's first frames settle its frame path on the positions feed)
    old, new = run(False), run(True)
    assert len(old) == len(new) == 3
    for a, b in zip(old, new):
        assert sorted(a) == sorted(b) and {"image", "depth", "weights_sum"} <= set(a)
        for k in a:
            assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k
        assert float(a["weights_sum"].max()) > 0               # the frames are not empty
