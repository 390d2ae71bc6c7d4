"""The reconstruction rule of the frame path's (t, ray id) sample records, pinned without a GPU.

(a) for a power-of-two 2*bound the field kernel's product with the exact reciprocal is the positions writer's division,
    bit for bit;
(b) position, dt and t - t_prev of every sample the oracle marcher emits are rebuilt from the ray's candidate sequence
    t0, t0 + dt(t0), ... with the operations of tests/sample_records_ref.py, bit for bit.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_records_ref as ref  # noqa: E402

F32 = np.float32


@pytest.mark.parametrize("bound", [1, 2, 4, 8])
def test_reciprocal_product_is_the_division_for_power_of_two_bounds(bound):
    rng = np.random.default_rng(bound)
    b = F32(bound)
    p = rng.uniform(-bound, bound, 300_000).astype(F32)
    ends = np.asarray([-b, b, np.nextafter(-b, F32(0)), np.nextafter(b, F32(0)), np.nextafter(-b, -F32(np.inf)),
                       np.nextafter(b, F32(np.inf)), F32(0.0), -F32(0.0), np.nextafter(F32(0), F32(1)),
                       -np.nextafter(F32(0), F32(1)), np.finfo(F32).tiny, -np.finfo(F32).tiny], F32)
    # (the two values just outside never reach the kernel - positions are clamped - but the identity holds there too)
    p = np.concatenate([p, ends, -p[:1000], np.minimum(np.maximum(p[:1000] * F32(1e-6), -b), b)])
    assert p.dtype == F32
    assert np.array_equal(ref.bits(ref.x01_div(p, bound)), ref.bits(ref.x01_mul(p, bound)))


def _near_far(o, d, bound, min_near=F32(0.05)):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = ((-F32(bound) - o) / d).astype(F32)
        t2 = ((F32(bound) - o) / d).astype(F32)
    near = np.max(np.minimum(t1, t2), -1)
    far = np.min(np.maximum(t1, t2), -1)
    miss = far < np.maximum(near, min_near)
    near = np.maximum(near, min_near)
    big = F32(np.finfo(F32).max)
    return np.where(miss, big, near).astype(F32), np.where(miss, big, far).astype(F32)


def _scene(cascade, seed):
    """64 rays from a point outside-ish the box into a 32^3 grid per cascade with some empty and some full cells."""
    from oracle.occupancy import packbits
    rng = np.random.default_rng(seed)
    H, bound = 32, float(2 ** (cascade - 1))
    grid = np.zeros((cascade, H ** 3), F32)
    for c in range(cascade):
        occ = rng.random((H // 4,) * 3) < 0.35                       # blocks of 4^3 cells: runs of hits and of misses
        cells = np.repeat(np.repeat(np.repeat(occ, 4, 0), 4, 1), 4, 2)
        grid[c] = cells.reshape(-1).astype(F32)                       # (Morton order of a random field is a random field)
    bitfield = packbits(grid.reshape(-1), 0.5)
    N = 64
    o = (rng.uniform(-0.3, 0.3, (N, 3)) * bound + np.asarray([0.0, 0.0, -1.4 * bound])).astype(F32)
    target = rng.uniform(-0.8, 0.8, (N, 3)).astype(F32) * F32(bound)
    d = target - o
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)
    d[0] = np.asarray([1.0, 0.0, 0.0], F32)                           # parallel to a face and beside the box: a miss
    nears, fars = _near_far(o, d, bound)
    return dict(o=o, d=d, bitfield=bitfield, bound=bound, H=H, nears=nears, fars=fars, N=N)


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("cascade", [1, 2])
@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 128])
def test_oracle_samples_are_rebuilt_from_the_candidate_sequence(dt_gamma, cascade, noise):
    from oracle.march import march_rays_train
    S = _scene(cascade, 7 + cascade)
    max_steps = 256
    noises = np.random.default_rng(3).random(S["N"]).astype(F32) if noise else None
    out = march_rays_train(S["o"], S["d"], S["bitfield"], S["bound"], cascade, S["H"], S["nears"], S["fars"],
                           noises=noises, dt_gamma=dt_gamma, max_steps=max_steps)
    rays, xyzs, deltas = out["rays"], out["xyzs"], out["deltas"]
    assert out["total"] > 20 * S["N"] // 4 and (rays[:, 2] == 0).any() and len(set(rays[:, 2].tolist())) > 8
    t0 = ref.start_t(S["nears"], noises, dt_gamma, max_steps, cascade, S["H"])
    step = lambda t: ref.step_dt(t, dt_gamma, max_steps, cascade, S["H"])      # noqa: E731
    for n in range(S["N"]):
        off, cnt = int(rays[n, 1]), int(rays[n, 2])
        if cnt == 0:
            continue
        # the candidate sequence does not depend on the grid: repeated float32 additions from t0
        cand = [t0[n]]
        while cand[-1] < S["fars"][n] and len(cand) < 100_000:
            cand.append(F32(cand[-1] + step(cand[-1])))
        cand = np.asarray(cand, F32)
        pos = ref.position(S["o"][n], S["d"][n], cand, S["bound"])            # [n_cand, 3]
        want = ref.bits(xyzs[off:off + cnt])
        got = ref.bits(pos)
        taken, j = [], 0
        for k in range(cnt):          # every sample is matched by a LATER candidate than the one before it
            while j < len(cand) and not np.array_equal(got[j], want[k]):
                j += 1
            assert j < len(cand), (n, k)
            taken.append(j)
            j += 1
        t = cand[taken]
        # two candidates can share a clamped position; dt and t - t_prev then tell whether the right ones were taken
        assert np.array_equal(ref.bits(ref.deltas_of_ray(t, t0[n], dt_gamma, max_steps, cascade, S["H"])),
                              ref.bits(deltas[off:off + cnt])), n
        assert np.array_equal(ref.bits(ref.x01_mul(pos[taken], S["bound"])), ref.bits(ref.x01_div(xyzs[off:off + cnt], S["bound"])))
