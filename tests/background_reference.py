"""numpy reference of the background sphere model (csrc/background.hip, the 2-D kernels of csrc/encoders.hip): sphere
coordinates of a ray, the 2-D hash-grid encode and its table gradient, SH-4, the 24 -> 64 -> 3 MLP, the sigmoid, the
blend and the full backward.  Every function takes ``dt``: np.float64 is the statement of WHAT is computed (plain
arithmetic, numpy's own sums), np.float32 is the restatement of HOW the kernels compute it - the same operations in the
same order, one rounding per operation, fmaf where the kernels use fmaf (emulated through float64: the product of two
fp32 numbers is exact there, so only the final rounding to fp32 is doubled, which differs from a true fma in about one
case in 2^29).  The integer index arithmetic of the fp32 restatement (cell, corner rows, hash) is what the kernels must
reproduce EXACTLY; its values set the tolerances: TOL = 8 x |fp32 restatement - float64| (``tol``), the project's rule
(tests/composite_reference.py).  No torch on the path.
"""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
HIDDEN, N_SH, N_IN = 64, 16, 24
BWD_LANES, BWD_MAX_GROUPS = 128, 512          # csrc/background.hip kBgBwdLanes, kBgMaxGroups
RADIUS = 32.0
RAY_COUNTS = (0, 1, 63, 64, 65, 257, 4096)
N_MISS = 3


def fma(a, b, c, dt):
    if dt is f64:
        return a * b + c
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def tol(restated32, reference64):
    """8 x the largest error of the fp32 restatement against float64 (NaN pairs, which must agree, aside)."""
    a, b = np.asarray(restated32, f64), np.asarray(reference64, f64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    e = np.abs(a - b)[~np.isnan(b)]
    return 8.0 * float(e.max()) if e.size else 0.0


# ---------------------------------------------------------------------------- level tables
@functools.lru_cache(maxsize=None)
def table(name):
    """"upstream": encoder_bg's 4-level table (base 16 -> 2048, 2^19 rows: three dense levels, one hashed);
    "small": base 4 -> 64, 2^6 rows: one dense level and three heavily colliding hashed ones."""
    from instance_nerf_amd.gridencoder import level_table
    kw = {"upstream": dict(base_resolution=16, log2_hashmap_size=19, desired_resolution=2048),
          "small": dict(base_resolution=4, log2_hashmap_size=6, desired_resolution=64)}[name]
    return level_table(num_levels=4, level_dim=2, input_dim=2, **kw)


# ---------------------------------------------------------------------------- sphere coordinates
def sph_from_ray(o, d, radius, dt):
    """o, d [N,3] -> coords [N,2]: the exit point of the ray from the sphere as (2 theta / pi - 1, phi / pi), y up,
    clamped to [-1,1]; NaN for a ray that never meets the sphere (negative discriminant, or the exit behind the origin)."""
    o, d = np.asarray(o, dt), np.asarray(d, dt)
    pi, r = dt(np.pi), dt(radius)
    ox, oy, oz, dx, dy, dz = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        A = dx * dx + dy * dy + dz * dz
        B = ox * dx + oy * dy + oz * dz
        C = (ox * ox + oy * oy + oz * oz) - r * r
        t = (-B + np.sqrt(B * B - A * C)) / A
        px, py, pz = ox + t * dx, oy + t * dy, oz + t * dz
        theta = np.arctan2(np.sqrt(px * px + pz * pz), py)
        phi = np.arctan2(pz, px)
        u = dt(2) * theta / pi - dt(1)
        v = phi / pi
        u = np.where(u < -1, dt(-1), np.where(u > 1, dt(1), u))
        v = np.where(v < -1, dt(-1), np.where(v > 1, dt(1), v))
        miss = ~(t >= 0)
    out = np.stack([u, v], -1).astype(dt)
    out[miss] = np.nan
    return out


# ---------------------------------------------------------------------------- 2-D grid
def cells(x, tb, dt):
    """x [M,2] in [-1,1] (bound 1) -> inside bool [M], rows int64 [M,L,4] (absolute table rows), weights dt [M,L,4].
    Corner k: bit 0 = +1 on axis 0, bit 1 = +1 on axis 1; weight wx * wy.  Rows / weights of outside samples: 0."""
    x = np.asarray(x, dt)
    M, L = x.shape[0], int(tb["num_levels"])
    with np.errstate(invalid="ignore"):
        x01 = (x + dt(1)) / dt(2)
        inside = (x01[:, 0] >= 0) & (x01[:, 0] <= 1) & (x01[:, 1] >= 0) & (x01[:, 1] <= 1)
    x01 = np.where(inside[:, None], x01, dt(0))
    rows = np.zeros((M, L, 4), np.int64)
    wts = np.zeros((M, L, 4), dt)
    for l in range(L):
        s = dt(tb["scales"][l])
        pos = x01 * s + dt(0.5)
        fl = np.floor(pos)
        fr = pos - fl
        g = fl.astype(np.int64)
        n_rows = int(tb["offsets"][l + 1]) - int(tb["offsets"][l])
        for k in range(4):
            cx, cy = g[:, 0] + (k & 1), g[:, 1] + ((k >> 1) & 1)
            wx = fr[:, 0] if k & 1 else dt(1) - fr[:, 0]
            wy = fr[:, 1] if k & 2 else dt(1) - fr[:, 1]
            if tb["hashed"][l]:
                assert n_rows & (n_rows - 1) == 0
                r = (cx ^ ((cy * 2654435761) & 0xFFFFFFFF)) & (n_rows - 1)
            else:
                r = cx + cy * (int(tb["resolutions"][l]) + 1)
                assert (r[inside] < n_rows).all()
            rows[:, l, k] = np.where(inside, int(tb["offsets"][l]) + r, 0)
            wts[:, l, k] = np.where(inside, wx * wy, dt(0))
    return inside, rows, wts


def encode2d(x, emb, tb, dt):
    """-> features [M, 2L]: sum over the corners in corner order (fmaf), zeros outside."""
    inside, rows, wts = cells(x, tb, dt)
    emb = np.asarray(emb, dt)
    M, L = rows.shape[:2]
    out = np.zeros((M, L, 2), dt)
    for k in range(4):
        out = fma(wts[:, :, k, None], emb[rows[:, :, k]], out, dt)
    out[~inside] = 0
    return out.reshape(M, 2 * L)


def table_grad(x, gout, tb, dt):
    """-> grad_embeddings [T,2] = sum over samples and corners of w * gout (samples in order; an atomic scatter adds in
    ANY order, so for rows with several contributions only the float64 form is a reference)."""
    inside, rows, wts = cells(x, tb, dt)
    M, L = rows.shape[:2]
    g = np.asarray(gout, dt).reshape(M, L, 2)
    out = np.zeros((int(tb["total_rows"]), 2), dt)
    contrib = (wts[:, :, :, None] * g[:, :, None, :]).astype(dt)              # [M,L,4,2]
    keep = np.broadcast_to(inside[:, None, None], rows.shape)
    np.add.at(out, rows[keep], contrib[keep])
    return out


def touched_rows(x, gout, tb):
    """Rows that receive a NON-ZERO contribution in the fp32 restatement, and how many each row receives."""
    inside, rows, wts = cells(x, tb, f32)
    M, L = rows.shape[:2]
    g = np.asarray(gout, f32).reshape(M, L, 2)
    contrib = wts[:, :, :, None] * g[:, :, None, :]
    hit = (contrib != 0).any(-1) & inside[:, None, None]
    count = np.zeros(int(tb["total_rows"]), np.int64)
    np.add.at(count, rows[hit], 1)
    return count


# ---------------------------------------------------------------------------- SH-4, MLP, sigmoid, blend
def sh4(d, dt):
    d = np.asarray(d, dt)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c = dt
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    v = [np.full_like(x, c(0.28209479177387814)),
         c(-0.48860251190291987) * y, c(0.48860251190291987) * z, c(-0.48860251190291987) * x,
         c(1.0925484305920792) * xy, c(-1.0925484305920792) * yz,
         c(0.94617469575755997) * z2 - c(0.31539156525251999), c(-1.0925484305920792) * xz,
         c(0.54627421529603959) * (x2 - y2),
         c(0.59004358992664352) * y * (c(-3.0) * x2 + y2), c(2.8906114426405538) * xy * z,
         c(0.45704579946446572) * y * (c(1.0) - c(5.0) * z2), c(0.3731763325901154) * z * (c(5.0) * z2 - c(3.0)),
         c(0.45704579946446572) * x * (c(1.0) - c(5.0) * z2), c(1.4453057213202769) * z * (x2 - y2),
         c(0.59004358992664352) * x * (-x2 + c(3.0) * y2)]
    return np.stack(v, -1).astype(dt)


def sigmoid(x, dt):
    return (dt(1) / (dt(1) + np.exp(-np.asarray(x, dt)))).astype(dt)


def mlp(h, w0, w1, dt):
    """h [N,24] -> (h1 [N,64] after ReLU, o [N,3]): z_j = sum_i w0[j,i] h[i] (i ascending), o_c = sum_j w1[c,j] h1_j."""
    h, w0, w1 = np.asarray(h, dt), np.asarray(w0, dt), np.asarray(w1, dt)
    if dt is f64:
        h1 = np.maximum(h @ w0.T, 0)
        return h1, h1 @ w1.T
    z = np.zeros((h.shape[0], HIDDEN), dt)
    for i in range(N_IN):
        z = fma(w0[None, :, i], h[:, i, None], z, dt)
    h1 = np.maximum(z, dt(0))
    o = np.zeros((h.shape[0], 3), dt)
    for j in range(HIDDEN):
        o = fma(w1[None, :, j], h1[:, j, None], o, dt)
    return h1, o


def field(coords, d, emb, tb, w0, w1, dt):
    """Background colour of rays with the given sphere coordinates: -> dict(h, h1, o, bg)."""
    h = np.concatenate([sh4(d, dt), encode2d(coords, emb, tb, dt)], -1)
    h1, o = mlp(h, w0, w1, dt)
    return dict(h=h, h1=h1, o=o, bg=sigmoid(o, dt))


def blend(image, weights_sum, bg, dt):
    image, ws, bg = np.asarray(image, dt), np.asarray(weights_sum, dt), np.asarray(bg, dt)
    return (image + ((dt(1) - ws)[:, None] * bg).astype(dt)).astype(dt)


def backward(grad_bg, coords, d, emb, tb, w0, w1, dt):
    """-> dict(grad_emb [T,2], grad_w0 [64,24], grad_w1 [3,64], denc [N,8]).  fp32: the kernel's order - gz = g (s (1 - s)),
    dz_j = sum_c w1[c,j] gz_c (c ascending, fmaf) masked by h1_j > 0, denc_i = sum_j w0[j,16+i] dz_j (fmaf); weight
    gradients: tiles of 128 rays dealt round-robin to min(tiles, 512) workgroups, rays added in order (fmaf) per
    workgroup, the workgroups' sums added in workgroup order."""
    fw = field(coords, d, emb, tb, w0, w1, dt)
    w0, w1, g = np.asarray(w0, dt), np.asarray(w1, dt), np.asarray(grad_bg, dt)
    N = g.shape[0]
    s = fw["bg"]
    gz = (g * (s * (dt(1) - s))).astype(dt)
    if dt is f64:
        dz = (gz @ w1) * (fw["h1"] > 0)
        denc = dz @ w0[:, N_SH:]
        gw0, gw1 = dz.T @ fw["h"], gz.T @ fw["h1"]
    else:
        dz = np.zeros((N, HIDDEN), dt)
        for c in range(3):
            dz = fma(w1[None, c, :], gz[:, c, None], dz, dt)
        dz = np.where(fw["h1"] > 0, dz, dt(0))
        denc = np.zeros((N, N_IN - N_SH), dt)
        for j in range(HIDDEN):
            denc = fma(w0[None, j, N_SH:], dz[:, j, None], denc, dt)
        tiles = (N + BWD_LANES - 1) // BWD_LANES
        groups = min(tiles, BWD_MAX_GROUPS)
        gw0, gw1 = np.zeros((HIDDEN, N_IN), dt), np.zeros((3, HIDDEN), dt)
        for b in range(groups):
            p0, p1 = np.zeros((HIDDEN, N_IN), dt), np.zeros((3, HIDDEN), dt)
            for tile in range(b, tiles, groups):
                for r in range(tile * BWD_LANES, min((tile + 1) * BWD_LANES, N)):
                    p0 = fma(dz[r, :, None], fw["h"][r, None, :], p0, dt)
                    p1 = fma(gz[r, :, None], fw["h1"][r, None, :], p1, dt)
            gw0, gw1 = (gw0 + p0).astype(dt), (gw1 + p1).astype(dt)
    return dict(grad_emb=table_grad(coords, denc, tb, dt), grad_w0=gw0, grad_w1=gw1, denc=denc, **fw)


# ---------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def weights(name, seed=0):
    """Table U(-1, 1), He-scaled weights (the product's U(-1e-4, 1e-4) table init would make every output 0.5)."""
    tb = table(name)
    rng = np.random.default_rng(1000 + seed)
    emb = rng.uniform(-1, 1, (int(tb["total_rows"]), 2)).astype(f32)
    w0 = (rng.standard_normal((HIDDEN, N_IN)) * np.sqrt(2.0 / N_IN)).astype(f32)
    w1 = (rng.standard_normal((3, HIDDEN)) * np.sqrt(2.0 / HIDDEN)).astype(f32)
    return emb, w0, w1


SPECIAL = 9          # rows of the special rays below


@functools.lru_cache(maxsize=None)
def rays(N, radius=RADIUS, seed=0):
    """-> o, d float32 [N,3], miss bool [N].  Origins with |o| <= radius / 2 (a well-conditioned root), unit directions.
    From N = 63 on the first rows are: three rays that miss the sphere (origin outside pointing away; two negative
    discriminants), rays along +y and -y from the centre and one along +y from off the centre (the poles), and a pair on
    either side of the phi = +-pi seam."""
    rng = np.random.default_rng(2000 + seed)
    d = rng.standard_normal((N, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = rng.standard_normal((N, 3))
    o *= (radius / 2) * rng.uniform(0, 1, (N, 1)) ** (1 / 3) / np.linalg.norm(o, axis=-1, keepdims=True)
    miss = np.zeros(N, bool)
    if N >= 63:
        R = radius
        special = [((2 * R, 0, 0), (1, 0, 0)), ((2 * R, 0, 0), (0, 1, 0)), ((0, 3 * R, 1), (0, 0, 1)),
                   ((0, 0, 0), (0, 1, 0)), ((0, 0, 0), (0, -1, 0)), ((0.5, 1, -0.25), (0, 1, 0)),
                   ((0, 0, 0), (-1, 0.2, 1e-4)), ((0, 0, 0), (-1, 0.2, -1e-4)), ((1, 2, 3), (-1, 0, 0))]
        assert len(special) == SPECIAL
        for i, (so, sd) in enumerate(special):
            o[i] = so
            d[i] = np.asarray(sd, f64) / np.linalg.norm(sd)
        miss[:N_MISS] = True
    return o.astype(f32), d.astype(f32), miss


@functools.lru_cache(maxsize=None)
def grad_bg(N, seed=0):
    return np.random.default_rng(3000 + seed).standard_normal((N, 3)).astype(f32)
