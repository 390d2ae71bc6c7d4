"""Plain references for the front of the pipeline (k_near_far, k_get_rays and the marchers of csrc/raymarch.hip):
the slab test and the ray generation in float64 with tolerances derived from the kernels' operation lists, and
``check_samples`` - properties of a marcher's output that hold whatever the occupancy walk did, so they would still
fail if the kernel and oracle/march.py shared a mistake.  Which candidates are emitted is the business of
oracle/march.py alone; nothing here walks a grid."""
import numpy as np

from oracle.occupancy import morton3D

import march_cases as mc

F32 = np.float32
U = 2.0 ** -24                       # unit roundoff of binary32
FLT_MAX = np.finfo(np.float32).max
NEAR_FAR_ROUNDINGS = 4               # (1 + U)^3 - 1 < 4 U: subtract, reciprocal, multiply
NEAR_FAR_MAX_EXCLUDED = 0.01
GET_RAYS_ROUNDINGS = 12              # see get_rays64


# ---------------------------------------------------------------------------- slab test
def near_far64(o, d, aabb, min_near):
    """The slab test of k_near_far in float64 on the fp32 inputs, with the kernel's comparison structure (so the NaN of
    0 * inf - a zero direction component with the origin on that slab's face - drops out the same way; (face - o) == 0
    holds in float64 exactly when it holds in binary32).

    -> dict(near, far: float64 [N] (the hit values, min_near applied); miss: bool; margin: |max lo - min hi|;
            tol: the bound below for near and for far, [N,2]; decided: bool - the classification check applies).

    Bound: the kernel rounds three times per slab value - (face - o), 1 / d, their product - so a finite, normal value
    lies within ((1 + U)^3 - 1) |t64| < 4 U |t64| of the float64 one.  near = max of three such values (and of
    min_near, exact), far = min: the extremum of perturbed values moves by at most the perturbation of the value that
    wins, whose magnitude is that of the float64 extremum up to a factor 1 + O(U) - inside the slack between
    3 U + 3 U^2 + U^3 and 4 U.  Values below the normal range (2^-126) carry an absolute error instead: 2^-126 * 4 U is
    added.  Hit or miss must agree wherever margin > 2 * 4 U * max(|max lo|, |min hi|): each side moves by at most
    one bound."""
    o, d, aabb = np.asarray(o, F32).astype(np.float64), np.asarray(d, F32).astype(np.float64), np.asarray(aabb, F32).astype(np.float64)
    n = o.shape[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rd = 1.0 / d
        near, far, miss = np.full(n, -np.inf), np.full(n, np.inf), np.zeros(n, bool)
        for a in range(3):
            t0, t1 = (aabb[a] - o[:, a]) * rd[:, a], (aabb[a + 3] - o[:, a]) * rd[:, a]
            lo, hi = np.where(t0 > t1, t1, t0), np.where(t0 > t1, t0, t1)
            if a > 0:
                miss |= (near > hi) | (lo > far)
            near, far = np.where(lo > near, lo, near), np.where(hi < far, hi, far)
        margin = np.abs(near - far)
        scale = np.maximum(np.abs(near), np.abs(far))
        decided = margin > 2 * NEAR_FAR_ROUNDINGS * U * scale          # False for a NaN or inf - inf margin
        tol_near = NEAR_FAR_ROUNDINGS * U * (np.abs(near) + 2.0 ** -126)
        near = np.where(near < np.float64(F32(min_near)), np.float64(F32(min_near)), near)
        tol = np.stack([tol_near, NEAR_FAR_ROUNDINGS * U * (np.abs(far) + 2.0 ** -126)], -1)
    return dict(near=near, far=far, miss=miss, margin=margin, tol=tol, decided=decided)


def check_near_far(got_near, got_far, ref):
    """got (fp32 arrays of the kernel or of oracle/rays.py) against ``near_far64``: classification where decided, values
    of the hits inside the bound.  -> share of rays excluded from the classification check."""
    got_near, got_far = np.asarray(got_near, F32), np.asarray(got_far, F32)
    got_miss = (got_near == FLT_MAX) & (got_far == FLT_MAX)
    dec = ref["decided"]
    assert (got_miss[dec] == ref["miss"][dec]).all(), f"hit / miss differs on rays {np.nonzero(dec & (got_miss != ref['miss']))[0][:8]}"
    hit = ~got_miss & ~ref["miss"]
    for k, (g, name) in enumerate(((got_near, "near"), (got_far, "far"))):
        fin = hit & np.isfinite(ref[name]) & np.isfinite(g)
        err = np.abs(g[fin].astype(np.float64) - ref[name][fin])
        bad = err > ref["tol"][fin, k]
        assert not bad.any(), f"{name}: off by {(err / np.maximum(ref['tol'][fin, k], 1e-300)).max() * NEAR_FAR_ROUNDINGS:.2f} U (allowed {NEAR_FAR_ROUNDINGS})"
        inf = hit & ~np.isfinite(ref[name])
        assert (g[inf].astype(np.float64) == ref[name][inf]).all(), f"{name}: an infinite value differs"
    return 1.0 - float(dec.mean()) if dec.size else 0.0


def near_far_random(n, seed):
    """Random rays whose hit / miss is decided with a wide margin for all but a vanishing share (origins in [-2, 2]^3,
    directions uniform on the sphere: the margin is a continuous variable of order 1, the bound of order 1e-7):
    (o, d, aabb, min_near)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-2, 2, (n, 3)).astype(F32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return o, d, np.asarray([-1, -1, -1, 1, 1, 1], F32), 0.05


# ---------------------------------------------------------------------------- ray generation
def get_rays64(poses, intr, W, inds):
    """k_get_rays in float64 on the fp32 inputs -> dict(rays_o, rays_d float64 [B,n,3], tol [B,n,3], tol_norm [B,n]).

    Tolerance, from the kernel's operation list (U = 2^-24, first order; the second-order terms are below the slack
    taken at the end).  i = (pix % W) + 0.5 and j are exact.
      xs = (i - cx) / fx                 2 roundings: relative error 2 U           (ys alike)
      xs * xs, ys * ys                   2 * 2 U + U = 5 U each; 1 * 1 is exact
      (xs^2 + ys^2) + 1                  positive terms, two adds: 5 U + 2 U = 7 U
      nrm = sqrt(.)                      halves it, one rounding: 4.5 U
      dx = xs / nrm                      2 U + 4.5 U + U = 7.5 U    (dy alike; dz = 1 / nrm: 5.5 U)
      dx * P0, dy * P1, dz * P2          8.5 U each
      (a + b) + c                        each add rounds once, relative to a partial sum that is at most
                                         S = |dx P0| + |dy P1| + |dz P2|: 2 U S
    so |rays_d - rays_d64| <= 10.5 U S per component; GET_RAYS_ROUNDINGS = 12 covers the second order.  S is formed
    from the float64 magnitudes, so the bound holds for any pose, orthonormal or not.  rays_o is a copy: exact.
    tol_norm: | |d| - |d64| | <= the Euclidean norm of the three component bounds."""
    poses = np.asarray(poses, F32).astype(np.float64).reshape(-1, 4, 4)
    fx, fy, cx, cy = [np.float64(F32(v)) for v in intr]
    inds = np.asarray(inds, np.int64)
    i, j = (inds % W) + 0.5, (inds // W) + 0.5
    xs, ys = (i - cx) / fx, (j - cy) / fy
    nrm = np.sqrt(xs * xs + ys * ys + 1.0)
    dcam = np.stack([xs / nrm, ys / nrm, 1.0 / nrm], -1)                       # [n,3]
    R = poses[:, :3, :3]
    rays_d = np.einsum("nc,brc->bnr", dcam, R)
    S = np.einsum("nc,brc->bnr", np.abs(dcam), np.abs(R))
    tol = GET_RAYS_ROUNDINGS * U * S
    rays_o = np.broadcast_to(poses[:, None, :3, 3], rays_d.shape).copy()
    return dict(rays_o=rays_o, rays_d=rays_d, tol=tol, tol_norm=np.linalg.norm(tol, axis=-1))


def get_rays_inputs():
    """(poses [3,4,4]: identity, a rotation, a NON-orthonormal 3x3 - the bound is stated in magnitudes; non-square
    intrinsics; H, W; inds with pixel 0, W - 1, W, H * W - 1 and a repeated index)."""
    rng = np.random.default_rng(8)
    poses = np.tile(np.eye(4, dtype=F32), (3, 1, 1))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    poses[1, :3, :3] = q
    poses[2, :3, :3] = rng.normal(size=(3, 3)) * 1.7
    poses[:, :3, 3] = rng.normal(size=(3, 3))
    H, W = 37, 53
    inds = np.asarray([0, W - 1, W, H * W - 1, 7, 7, 1000], np.int64)
    return poses, (61.5, 48.25, 26.0, 19.5), H, W, inds


def check_get_rays(got_o, got_d, ref):
    got_o, got_d = np.asarray(got_o, F32).reshape(ref["rays_o"].shape), np.asarray(got_d, F32).reshape(ref["rays_d"].shape)
    assert (got_o.astype(np.float64) == ref["rays_o"]).all(), "rays_o is not the pose's translation"
    err = np.abs(got_d.astype(np.float64) - ref["rays_d"])
    assert (err <= ref["tol"]).all(), f"rays_d off by {(err / np.maximum(ref['tol'], 1e-300)).max() * GET_RAYS_ROUNDINGS:.2f} U S (allowed {GET_RAYS_ROUNDINGS})"
    nerr = np.abs(np.linalg.norm(got_d.astype(np.float64), axis=-1) - np.linalg.norm(ref["rays_d"], axis=-1))
    assert (nerr <= ref["tol_norm"]).all(), "|rays_d| outside its bound"
    return float((err / np.maximum(ref["tol"], 1e-300)).max() * GET_RAYS_ROUNDINGS)


# ---------------------------------------------------------------------------- marcher outputs
def _cell_is_set(case, p, dt):
    """The contract's cell of a sample (oracle/march.py, top) from its position and step alone -> bool [n]."""
    C, H, bound = case["C"], case["H"], F32(case["bound"])
    _, e0 = np.frexp(np.abs(p).max(axis=-1))
    _, e1 = np.frexp(dt * F32(H) * F32(0.5))
    level = np.maximum(np.clip(e0, 0, C - 1), np.clip(e1, 0, C - 1)).astype(np.int64)
    mb = np.minimum(np.ldexp(F32(1.0), level).astype(F32), bound)
    rmb = (F32(1.0) / mb).astype(F32)
    f = ((p * rmb[:, None] + F32(1.0)) * F32(0.5)) * F32(H)
    n = np.clip(f.astype(np.int32), 0, H - 1)
    bit = level * H ** 3 + morton3D(n).astype(np.int64)
    return ((case["bits"][bit >> 3] >> (bit & 7).astype(np.uint8)) & 1).astype(bool)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def check_samples(case, rays, xyzs, dirs, deltas, t=None, ids=None, counter=None):
    """Properties of one training march, samples in RAY-MAJOR order (row offset_r + k = k-th sample of ray r; M = total):

      1. rays[:,0] == arange, rays[:,1] == exclusive cumsum of rays[:,2], rays[:,2] <= max_steps,
         counter == (total, N) when given.
      2. every ray's samples sit at strictly increasing numbers j of its candidate chain c_j (march_cases.candidates):
         xyz == clamp(o + c_j * d) and deltas[:,0] == dt(c_j) bit for bit, deltas[:,1] == (c_j + dt_j) - (c_prev +
         dt_prev), the subtrahend being t0 for the ray's first sample; the first such j behind the previous one is taken.
         With ``t`` (the records form: xyzs, dirs, deltas may be None) t == c_j instead, and ids == the ray.
      3. the cell of every emitted position (from p and dt alone) is set in the bitfield.
      4. every emitted c_j < far.
      5. dirs rows are the ray's direction, bit for bit.

    Raises AssertionError naming the first ray and sample that fail."""
    rays = np.asarray(rays)
    N = case["o"].shape[0]
    cnt, off = rays[:, 2].astype(np.int64), rays[:, 1].astype(np.int64)
    assert rays.shape == (N, 3) and (rays[:, 0] == np.arange(N)).all(), "rays[:,0] is not arange"
    want_off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    assert (off == want_off).all(), f"offset of ray {np.nonzero(off != want_off)[0][0]} is not the exclusive cumsum"
    assert (cnt >= 0).all() and (cnt <= case["max_steps"]).all(), "a count outside 0 .. max_steps"
    total = int(cnt.sum())
    if counter is not None:
        assert tuple(int(v) for v in counter) == (total, N), f"counter {tuple(counter)} != {(total, N)}"
    rows = total
    for name, a, w in (("xyzs", xyzs, 3), ("dirs", dirs, 3), ("deltas", deltas, 2), ("t", t, 0), ("ids", ids, 0)):
        assert a is None or (a.shape[0] == rows and (a.ndim == 1 if w == 0 else a.shape[1:] == (w,))), f"{name}: shape {a.shape}"
    if total == 0:
        return
    t0, fars = mc.start_t(case), case["fars"]
    live = np.nonzero(cnt > 0)[0]
    marches = t0[live] < fars[live]
    assert marches.all(), f"ray {live[~marches][0]} has samples without t0 < far"
    # the chains of the rays that have samples: CH [n_live, J]
    o, d, bound = case["o"][live], case["d"][live], F32(case["bound"])
    step = lambda x: mc.dt_of(x, case["max_steps"], case["C"], case["H"], case["dt_gamma"])
    chain, cur = [], t0[live].copy()
    while (cur < fars[live]).any():
        assert len(chain) <= mc.MAX_CANDIDATES + 1, "a chain beyond the safety rule"
        chain.append(cur)
        cur = (cur + step(cur)).astype(F32)
    CH = np.stack(chain, 1)
    DT = step(CH)
    TN = (CH + DT).astype(F32)
    J = CH.shape[1]
    jj = np.arange(J)[None, :]
    prev_j, last = np.full(len(live), -1), t0[live].copy()
    lcnt, loff = cnt[live], off[live]
    for k in range(int(lcnt.max())):
        act = np.nonzero(lcnt > k)[0]
        row = loff[act] + k
        ok = (jj > prev_j[act, None]) & (CH[act] < fars[live][act, None])
        if t is not None:
            ok &= _bits(CH[act]) == _bits(t[row])[:, None]
        else:
            P = np.minimum(np.maximum(o[act, None, :] + CH[act][:, :, None] * d[act, None, :], -bound), bound).astype(F32)
            ok &= (_bits(P) == _bits(xyzs[row])[:, None, :]).all(-1)
            ok &= _bits(DT[act]) == _bits(deltas[row, 0])[:, None]
            ok &= _bits((TN[act] - last[act, None]).astype(F32)) == _bits(deltas[row, 1])[:, None]
        found = ok.any(1)
        assert found.all(), (f"{case['name']}: sample {k} of ray {live[act[~found][0]]} is no candidate behind the previous "
                             f"sample with the contract's position, dt and t - t_prev (or lies at or beyond far)")
        j = ok.argmax(1)
        prev_j[act], last[act] = j, TN[act, j]
        pos = np.minimum(np.maximum(o[act] + CH[act, j][:, None] * d[act], -bound), bound).astype(F32)
        occ = _cell_is_set(case, pos, DT[act, j])
        assert occ.all(), f"{case['name']}: sample {k} of ray {live[act[~occ][0]]} lies in a cell whose bit is clear"
    ray_of_row = np.repeat(np.arange(N), cnt)
    if dirs is not None:
        same = (_bits(dirs) == _bits(case["d"][ray_of_row])).all(-1)
        assert same.all(), f"{case['name']}: dirs row {np.nonzero(~same)[0][0]} is not its ray's direction"
    if ids is not None:
        assert (np.asarray(ids) == ray_of_row).all(), f"{case['name']}: a record names another ray"


def ray_major(rays, M):
    """Row numbers of the ray-major writers for the rays that fit in M: int64 [kept total] (a dropped ray has none)."""
    out = [np.arange(off, off + cnt) for _, off, cnt in np.asarray(rays) if cnt > 0 and off + cnt <= M]
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def damage(ref, how):
    """A hand-damaged copy of an oracle output dict (rays, xyzs, dirs, deltas) that check_samples must reject."""
    rays, xyzs, dirs, deltas = (ref[k].copy() for k in ("rays", "xyzs", "dirs", "deltas"))
    r = int(np.nonzero(rays[:, 2] >= 3)[0][0])
    row = int(rays[r, 1]) + 1                                   # the ray's second sample
    if how == "dropped_sample":                                 # the ray's samples close up, counts stay: its last row
        xyzs[row:rays[r, 1] + rays[r, 2] - 1] = ref["xyzs"][row + 1:rays[r, 1] + rays[r, 2]]      # repeats the one before
        deltas[row:rays[r, 1] + rays[r, 2] - 1] = ref["deltas"][row + 1:rays[r, 1] + rays[r, 2]]
    elif how == "ulp_off":
        a = int(np.abs(dirs[row]).argmax())                     # the axis along which the ray moves
        xyzs[row, a] = np.nextafter(xyzs[row, a], F32(np.inf))
    elif how == "offset_shifted":
        rays[r:, 1] += 1
    else:
        raise ValueError(how)
    return dict(rays=rays, xyzs=xyzs, dirs=dirs, deltas=deltas)
