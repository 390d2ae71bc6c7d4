"""2-D mask matching on the GPU (csrc/match.hip through masks.match_masks / project_and_match): the fused path equals the
composable torch path equals the oracle - exact integers - on the golden fixture of the reference's own run, on seeded
views of every size at which the kernels take another path, and on the layouts that stress the count kernel's
aggregation both ways; the bit packer; determinism; the status word; the projector-fed pipeline."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def fused(seg, proj, ids=None, **kw):
    from instance_nerf_amd.masks import match_masks
    out = match_masks(torch.as_tensor(seg).to(DEV), torch.as_tensor(proj).to(DEV), ids, fused=True, **kw)
    assert out.is_cuda and out.dtype == torch.int32
    return out


def test_golden_fixture_through_the_kernels():
    from instance_nerf_amd.masks import convert_segments
    _, rows, names = mc.golden_cases()
    for img, pan, info, proj, ids, want in rows:
        got = fused(convert_segments(pan, info, names), proj, ids, ordered=True)
        assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), img


@pytest.mark.parametrize("name", [f[0] for f in mc.FUZZ] + mc.LAYOUTS)
def test_fused_equals_composable_equals_oracle(name):
    from instance_nerf_amd.masks import match_masks
    seg, proj, ids, want = mc.case(name)
    got = fused(seg, proj, ids)
    assert np.array_equal(got.cpu().numpy(), want)
    twin = match_masks(torch.from_numpy(seg).to(DEV), torch.from_numpy(proj).to(DEV), ids, fused=False)
    assert twin.is_cuda and torch.equal(twin, got)
    assert np.array_equal(match_masks(seg, torch.from_numpy(proj).to(DEV), ids).cpu().numpy(), want)     # numpy maps: host ranks


def test_large_segment_ids_and_no_candidates():
    seg = np.zeros((1, 9, 11), np.int32)
    seg[0, :4], seg[0, 5:, :5], seg[0, 8, 8] = 10 ** 6, 70000, -1
    proj = np.stack([seg[0] == 10 ** 6, seg[0] == 70000, np.ones((9, 11), bool)])[None]
    got = fused(seg, proj, [4, 2, 9]).cpu().numpy()
    assert np.array_equal(got, mc.expected(seg, proj, [4, 2, 9])) and (got[seg == 10 ** 6] == 4).all()
    assert np.array_equal(fused(seg, np.zeros((1, 0, 9, 11), bool)).cpu().numpy(), np.where(seg > 0, -1, seg))


def test_pack_mask_bits_equals_the_dense_compare():
    from instance_nerf_amd import _lib
    from instance_nerf_amd.nerf.utils import get_rays
    lib = _lib.load()
    H, W, k, thresh = 8, 12, 33, 0.25
    P = H * W
    rng = np.random.default_rng(0)
    pose = torch.eye(4, device=DEV)[None]
    inds = get_rays(pose, (10.0, 10.0, W / 2, H / 2), H, W, patch=4)["inds"][0].contiguous()
    assert inds.dtype == torch.int64 and sorted(inds.tolist()) == list(range(P)) and inds.tolist() != list(range(P))
    soft = torch.from_numpy(rng.random((P, k)).astype(np.float32)).to(DEV)
    soft[3, 5], soft[4, 32], soft[5, 0], soft[6, 31] = float("nan"), thresh, thresh, float(np.nextafter(np.float32(thresh), np.float32(1)))

    def pack(soft, inds, n):
        words = torch.full((2, P), -1, dtype=torch.int32, device=DEV)           # the call clears it
        _lib.check(lib.inr_pack_mask_bits(_lib.ptr(soft), _lib.ptr(inds, allow_none=True), n, k, thresh, P, _lib.ptr(words),
                                          _lib.stream_ptr()))
        bits = (words.cpu().numpy().view(np.uint32)[:, None, :] >> np.arange(32, dtype=np.uint32)[None, :, None]) & 1
        return bits.reshape(64, P).astype(bool)

    for ind in (inds, None):
        flat = torch.zeros(P, k, device=DEV)
        flat[ind if ind is not None else torch.arange(P, device=DEV)] = soft
        want = (flat > thresh).t().cpu().numpy()
        got = pack(soft, ind, P)
        assert np.array_equal(got[:k], want) and not got[k:].any()
        assert not want[5, int(inds[3]) if ind is not None else 3] and want[31, int(inds[6]) if ind is not None else 6]
    # a subset of the pixels (and one index outside the image): the others stay 0
    some = inds[: P // 2].clone()
    some[0] = P + 7
    got = pack(soft[: P // 2].contiguous(), some, P // 2)
    want = np.zeros((k, P), bool)
    want[:, some[1:].cpu().numpy()] = (soft[1: P // 2] > thresh).t().cpu().numpy()
    assert np.array_equal(got[:k], want)


def test_two_calls_give_identical_bits():
    seg, proj, ids, _ = mc.case("200x200_k70")
    a, b = fused(seg, proj, ids), fused(seg, proj, ids)
    assert torch.equal(a, b)


def test_a_rank_outside_the_range_raises_and_the_next_call_works():
    from instance_nerf_amd.masks import match_ranked, pack_mask_bits
    seg, proj, ids, want = mc.case("7x9_k31")
    order = mc.name_order(ids)
    words = pack_mask_bits(torch.from_numpy(proj[:, order]).to(DEV)).reshape(3, 1, 63).contiguous()
    ids_t = torch.tensor([int(ids[i]) for i in order], dtype=torch.int32, device=DEV)
    ranks = torch.from_numpy(seg.reshape(3, 63)).to(DEV)
    S = int(ranks.max())
    bad = ranks.clone()
    bad[1, 17] = S + 1
    with pytest.raises(ValueError, match="outside"):
        match_ranked(bad, words, S, 31, ids_t)
    assert np.array_equal(match_ranked(ranks, words, S, 31, ids_t).cpu().numpy().reshape(want.shape), want)


def test_project_and_match_equals_projector_plus_oracle(tmp_path, room, room_bitfield, params_k16):
    from instance_nerf_amd.masks import load_matched_masks, project_3d_masks, project_and_match
    from test_gpu_parity import _network, _t
    net = _network(params_k16, K=0).eval()
    net.density_bitfield.copy_(_t(room_bitfield))
    res = 20
    occ = room.occupancy_grid(res, 1.0)
    masks = np.zeros((12, res, res, res), np.float32)
    masks[0, :10], masks[1, :, :10], masks[2, :, :, 10:] = occ[:10], occ[:, :10], occ[:, :, 10:]
    masks[9, 5:15], masks[10, :, 5:15], masks[11, :, :, :10] = occ[5:15], occ[:, 5:15], occ[:, :, :10]     # ids 10..12 sort before 2
    poses, intr, H, W = room.cameras(n=2, H=32, W=32, focal=16.0)
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:H, 0:W]
    seg = np.stack([((yy // 8) * 4 + xx // 8 + 1) * 50, (xx // 4 + 1) + 0 * yy]).astype(np.int32)     # blocks; columns
    seg[rng.random(seg.shape) < 0.1] = -1
    seg[rng.random(seg.shape) < 0.1] = 0
    got = project_and_match(net, masks, [-1, -1, -1], [1, 1, 1], poses, intr, H, W, seg, out_dir=str(tmp_path),
                            img_names=["a", "b"], thresh=0.02)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (2, H, W)
    proj = project_3d_masks(net, masks, [-1, -1, -1], [1, 1, 1], poses, intr, H, W, thresh=0.02)
    assert proj.any(axis=(2, 3)).sum() >= 6
    want = mc.expected(seg, proj, np.arange(1, 13))
    assert np.array_equal(got.cpu().numpy(), want) and (want > 0).any()
    back = load_matched_masks(str(tmp_path))
    assert sorted(back) == ["a", "b"] and np.array_equal(back["a"], want[0]) and np.array_equal(back["b"], want[1])
