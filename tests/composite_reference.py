"""Plain float64 restatements of the compositing kernels of csrc/raymarch.hip (k_composite_train_fwd / _bwd,
k_composite_train_extra_fwd with its cross entropy / _extra_bwd, k_composite_patch_fwd / _extra, k_composite_rays),
the generators of their test cases and the tolerances of tests/test_composite_kernels.py.  numpy and Python loops only:
one sample after the other, nothing shared with instance_nerf_amd or oracle/.

Semantics (upstream's): per ray, from T = 1, t = 0, for the samples in order
    alpha = 1 - exp(-sigma * delta.x);  w = alpha * T;  ws += w;  t += delta.y;  depth += w * t;  image += w * rgb;
    extra_out += w * extra;  T *= 1 - alpha;  stop if T < T_thresh
so a sample is used iff the transmittance before it is at least T_thresh, and the first one always.  A ray with
off + cnt > M was dropped by the writer: all its outputs are zero.  Samples behind the termination point are NEVER READ
(they may hold NaN).  T_thresh is compared as the fp32 value the kernels receive.

Tolerances.  TOL[name] = 8 x MEASURED[name]; MEASURED[name] is the largest error of the project's fp32 SEQUENTIAL
restatement against this file's float64 on every regime_case (oracle.c_port.composite_rays_train for the forward,
oracle.composite.composite_backward_analytic fed with c_port's forward for the backward, ``wavefront_run(dtype=fp32)``
and ``ce_rows(dtype=fp32)`` of this file for the two forms the oracle has no sequential fp32 of), measured on the CPU,
rounded up to two digits.  The 8 covers what a kernel may do differently: tree-order scans (~1 ulp per level, 6 levels
per chunk, up to 16 chunks) and the device expf.  tests/test_composite_cpu.py asserts that the restatements stay within
TOL / 8, so the constants cannot drift from the measurement.

Ambiguity.  A ray whose float64 ``margin`` (smallest |T_i - T_thresh| / T_thresh over the step boundaries at which the
termination test is taken) is below MARGIN may stop one sample earlier or later in fp32 and is left out of the
tolerance comparisons.  The wavefront form tests T = 1 - ws, whose ABSOLUTE error grows with the number of additions:
there a ray is ambiguous when some test value lies within steps * 2^-23 of T_thresh, steps = additions so far.  With
alpha <= 0.13 per step (regime 40) and T_thresh = 1e-4 a ray that stops after ~270 steps passes ~10 boundaries inside
that band whatever the seed, so the wavefront cases of regime 40 use T_thresh = WAVEFRONT_T40 (band / step ~ 1 %); the
other regimes and the exact tier keep 1e-4.  At most 2 % of a case's rays may be excluded and every count class keeps
a compared ray (asserted on the CPU from this file alone).
"""
import hashlib
import math

import numpy as np

F32, F64 = np.float32, np.float64
GROUP = 16
T_THRESH = 1e-4
WAVEFRONT_T40 = 0.05
MARGIN = 1e-4
MAX_EXCLUDED = 0.02
COUNTS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 511, 1024)
COPIES = 3                                   # 51 rays (not a multiple of 16), 8214 samples
P_CLASSES = ("transparent", "last", 128, 127, 65, 64, 63, 62, 0)
REGIMES = ("s0.3", "s40", "s2000", "zero")
_SCALE = {"s0.3": 0.3, "s40": 40.0, "s2000": 2000.0, "zero": 0.0}
KMAX = 64

# Largest |fp32 sequential restatement - float64| over the four regimes, compared rays only, as measured on the CPU
# (value seen -> constant, rounded up to two digits); the absolute size of the output is given for scale.
MEASURED = {
    "weights_sum": 7.8e-7,     # 7.79e-7  (regime s0.3, 1024-sample rays; outputs up to 1)
    "depth": 1.3e-5,           # 1.20e-5  (s0.3: t reaches 25, depth 3)
    "image": 7.6e-7,           # 7.58e-7
    "weights": 5.8e-8,         # 5.71e-8  (s2000: weights up to 1)
    "extra_out": 1.3e-6,       # 1.29e-6  (64 channels, |extra_out| up to 3.2)
    "grad_sigmas": 1.8e-8,     # 1.70e-8  (|grad_sigmas| up to 1.7e-2)
    "grad_rgbs": 2.7e-7,       # 2.65e-7  (up to 2.8)
    "grad_extra": 2.8e-7,      # 2.72e-7  (fp32 w * g against float64; up to 2.9)
    "wf_weights_sum": 1.5e-6,  # 1.41e-6  (T = 1 - ws form, fp32 wavefront_run; n_step 1, 3, 8)
    "wf_depth": 3.0e-5,        # 2.93e-5  (absolute t: up to 26)
    "wf_image": 8.6e-7,        # 8.59e-7
    "wf_extra": 3.2e-6,        # 3.17e-6
    "wf_rays_t": 2.2e-5,       # 2.15e-5  (1024 sequential additions of delta.y)
    "ce_loss": 1.1e-6,         # 1.03e-6  (fp32 ce_rows on c_port's fp32 logits against float64 on float64 logits)
    "ce_dpix": 2.8e-7,         # 2.74e-7
}
TOL = {k: 8.0 * v for k, v in MEASURED.items()}
# Rays excluded as ambiguous, of 51, regime_case("tol", r): s0.3 0, s40 0, s2000 1 (margin 7.6e-6), zero 0; the same
# counts for the wavefront form (s2000: the same ray).  Smallest margin kept: 5.3e-4 (s40).


def _rng(*key):
    """PCG64 keyed by the case name: the same numbers wherever the case is built."""
    return np.random.Generator(np.random.PCG64(int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:8], "little")))


def _th(T_thresh):
    return float(F32(T_thresh))


# ---------------------------------------------------------------------------- training compositing
def forward(sig, rgb, deltas, rays, T_thresh, extra=None):
    """-> dict(weights_sum [N], depth [N], image [N,3], weights [M], extra_out [N,K] | None, sample_ray int32 [M]
    (-1 where no ray owns the row; a dropped ray owns [off, M)), margin [N] (inf when no test is taken), n_used [N],
    dropped bool [N]), float64.  Outputs are indexed by ray id rays[:,0], margin / n_used / dropped by row of rays."""
    sig, rgb, deltas = np.asarray(sig, F64), np.asarray(rgb, F64), np.asarray(deltas, F64)
    rays = np.asarray(rays).astype(np.int64)
    N, M, th = len(rays), sig.shape[0], _th(T_thresh)
    K = 0 if extra is None else extra.shape[1]
    ex = None if extra is None else np.asarray(extra, F64)
    ws, depth, image, weights = np.zeros(N), np.zeros(N), np.zeros((N, 3)), np.zeros(M)
    extra_out = np.zeros((N, K)) if K else None
    sample_ray = np.full(M, -1, np.int32)
    margin, n_used, dropped = np.full(N, np.inf), np.zeros(N, np.int64), np.zeros(N, bool)
    for n in range(N):
        rid, off, cnt = (int(v) for v in rays[n])
        if off + cnt > M:
            dropped[n] = True
            sample_ray[off:M] = rid
            continue
        sample_ray[off:off + cnt] = rid
        T, t = 1.0, 0.0
        for j in range(cnt):
            i = off + j
            if j > 0:
                margin[n] = min(margin[n], abs(T - th) / th)
                if T < th:
                    break
            alpha = 1.0 - math.exp(-sig[i] * deltas[i, 0])
            w = alpha * T
            ws[rid] += w
            t += deltas[i, 1]
            depth[rid] += w * t
            image[rid] += w * rgb[i]
            if K:
                extra_out[rid] += w * ex[i]
            weights[i] = w
            T *= 1.0 - alpha
            n_used[n] += 1
    return dict(weights_sum=ws, depth=depth, image=image, weights=weights, extra_out=extra_out, sample_ray=sample_ray,
                margin=margin, n_used=n_used, dropped=dropped)


def backward(g_ws, g_img, sig, rgb, deltas, rays, fwd, g_extra=None):
    """The closed form of oracle/composite.py::composite_backward_analytic in float64 over the used set of ``fwd``:
        d/d rgb_i = g_img * w_i;   d/d sigma_i = delta.x_i * (g_img . (T_{i+1} rgb_i - (C - C_upto_i)) + g_ws (1 - ws))
        d/d extra_i = w_i * g_extra_out         (the K channels see the weights detached)
    -> grad_sigmas [M], grad_rgbs [M,3], grad_extra [M,K] | None; rows no ray owns or uses are zero."""
    sig, rgb, deltas = np.asarray(sig, F64), np.asarray(rgb, F64), np.asarray(deltas, F64)
    rays = np.asarray(rays).astype(np.int64)
    M = sig.shape[0]
    g_img = np.asarray(g_img, F64)
    g_s, g_c = np.zeros(M), np.zeros((M, 3))
    g_e = None if g_extra is None else np.zeros((M, np.asarray(g_extra).shape[1]))
    for n in range(len(rays)):
        rid, off, _ = (int(v) for v in rays[n])
        gw = 0.0 if g_ws is None else float(g_ws[rid])
        T, acc = 1.0, np.zeros(3)
        for j in range(int(fwd["n_used"][n])):
            i = off + j
            alpha = 1.0 - math.exp(-sig[i] * deltas[i, 0])
            w = alpha * T
            acc = acc + w * rgb[i]
            T *= 1.0 - alpha
            g_c[i] = g_img[rid] * w
            g_s[i] = deltas[i, 0] * (float(np.dot(g_img[rid], T * rgb[i] - (fwd["image"][rid] - acc)))
                                     + gw * (1.0 - fwd["weights_sum"][rid]))
            if g_e is not None:
                g_e[i] = fwd["weights"][i] * np.asarray(g_extra[rid], F64)
    return g_s, g_c, g_e


# ---------------------------------------------------------------------------- patch-interleaved layout
def patch_slot_map(rays, group=GROUP):
    """slot(r, k) = base_g + sum_i min(c_i, k) + #{i < r : c_i > k} for every ray (in groups of ``group`` consecutive
    rows of ``rays``) and step, written out with loops.  rays[:,1] must be the exclusive scan of rays[:,2] (as the
    marcher's count pass leaves it).  -> int64 [total]: the patch row of ray-major sample rays[n,1] + k."""
    rays = np.asarray(rays).astype(np.int64)
    N = len(rays)
    cnt, off = [int(c) for c in rays[:, 2]], [int(o) for o in rays[:, 1]]
    assert off == [sum(cnt[:n]) for n in range(N)], "offsets are not the exclusive scan of the counts"
    slots = np.zeros(sum(cnt), np.int64)
    for g0 in range(0, N, group):
        c = cnt[g0:g0 + group]
        for r in range(len(c)):
            for k in range(c[r]):
                below = 0
                for ci in c:
                    below += min(ci, k)
                rank = 0
                for i in range(r):
                    if c[i] > k:
                        rank += 1
                slots[off[g0 + r] + k] = off[g0] + below + rank
    return slots


def dropped_groups(rays, M, group=GROUP):
    """bool [N]: the ray's group does not fit into M rows (base + group total > M) - the writer dropped it whole."""
    rays = np.asarray(rays).astype(np.int64)
    out = np.zeros(len(rays), bool)
    for g0 in range(0, len(rays), group):
        out[g0:g0 + group] = int(rays[g0, 1]) + int(rays[g0:g0 + group, 2].sum()) > M
    return out


def to_patch(a, slots, M=None, fill=0):
    """Ray-major rows -> patch layout with M rows (default: all); rows beyond M are cut, rows nobody fills hold ``fill``."""
    a = np.asarray(a)
    M = len(slots) if M is None else int(M)
    out = np.full((M,) + a.shape[1:], fill, a.dtype)
    keep = slots < M
    out[slots[keep]] = a[:len(slots)][keep]
    return out


def skippable(rays, n_used, M, group=GROUP):
    """Samples at steps k at which every ray of the group that still has a sample (c_i > k) has terminated before k
    (n_used_i <= k); dropped groups count nothing."""
    rays = np.asarray(rays).astype(np.int64)
    drop = dropped_groups(rays, M, group)
    total = 0
    for g0 in range(0, len(rays), group):
        if drop[g0]:
            continue
        c = [int(v) for v in rays[g0:g0 + group, 2]]
        u = [int(v) for v in n_used[g0:g0 + group]]
        for k in range(max(c) if c else 0):
            act = [i for i in range(len(c)) if c[i] > k]
            if act and all(u[i] <= k for i in act):
                total += len(act)
    return total


# ---------------------------------------------------------------------------- wavefront step
def wavefront_step(n_alive, n_step, rays_alive, rays_t, sig, rgb, deltas, ws, depth, image, T_thresh, extra=None,
                   extra_acc=None, dtype=F64, track=None):
    """One call of composite_rays, in place, every operation in ``dtype``: for slot n with ray r = rays_alive[n] >= 0 and
    its rows n*n_step ..: stop (dead) at a row with delta.x == 0; alpha = 1 - exp(-sigma delta.x); T = 1 - ws[r];
    w = alpha T; ws += w; t += delta.y; depth += w t; image += w rgb; extra_acc += w extra; dead if T (1 - alpha) <
    T_thresh.  Dead: rays_alive[n] = -1; else rays_t[r] = t.  ``track`` = dict(steps int [N], ratio float [N]): the
    smallest |T (1 - alpha) - T_thresh| / (steps 2^-23) of each ray, steps = additions into ws so far."""
    d = dtype
    th, one = d(F32(T_thresh)), d(1.0)
    for n in range(n_alive):
        r = int(rays_alive[n])
        if r < 0:
            continue
        t = d(rays_t[r])
        dead = False
        for step in range(n_step):
            i = n * n_step + step
            d0 = d(deltas[i, 0])
            if d0 == 0:
                dead = True
                break
            alpha = one - d(np.exp(-d(sig[i]) * d0))
            T = one - ws[r]
            w = alpha * T
            ws[r] = ws[r] + w
            t = t + d(deltas[i, 1])
            depth[r] = depth[r] + w * t
            image[r] = image[r] + w * np.asarray(rgb[i], d)
            if extra is not None:
                extra_acc[r] = extra_acc[r] + w * np.asarray(extra[i], d)
            Tn = T * (one - alpha)
            if track is not None:
                track["steps"][r] += 1
                track["ratio"][r] = min(track["ratio"][r], abs(float(Tn) - float(th)) / (track["steps"][r] * 2.0 ** -23))
            if Tn < th:
                dead = True
                break
        if dead:
            rays_alive[n] = -1
        else:
            rays_t[r] = t


def wavefront_run(case, n_step, step, K=0):
    """The renderer's loop around composite_rays, restated: every call hands each live ray its next ``n_step`` samples
    (rows behind a ray's last sample have delta == 0 and NaN in sigma / rgb / extra: a ray that has run out stops at
    delta.x == 0 without reading them); the live list is compacted, order kept, after every SECOND call, so dead (-1)
    slots are seen too (their rows are NaN throughout).  ``step(n_alive, n_step, rays_alive int32, sig, rgb, deltas,
    extra | None) -> rays_alive after the call`` owns the accumulators.  Rays are named by their id rays[:,0]."""
    rays = np.asarray(case["rays"]).astype(np.int64)
    M = case["sig"].shape[0]
    span = {int(r): (int(o), int(c)) for r, o, c in rays if o + c <= M}
    alive = np.asarray([int(r) for r in rays[:, 0] if int(r) in span], np.int32)
    cursor = {r: 0 for r in span}
    calls = 0
    while len(alive):
        n_alive = len(alive)
        rows = n_alive * n_step
        sig, rgb = np.full(rows, np.nan, F32), np.full((rows, 3), np.nan, F32)
        dl = np.full((rows, 2), np.nan, F32)
        ex = np.full((rows, K), np.nan, F32) if K else None
        for n, r in enumerate(alive):
            if r < 0:
                continue
            off, cnt = span[int(r)]
            lo = cursor[int(r)]
            m = max(0, min(n_step, cnt - lo))
            a, b = n * n_step, n * n_step + m
            sig[a:b], rgb[a:b], dl[a:b] = case["sig"][off + lo:off + lo + m], case["rgb"][off + lo:off + lo + m], \
                case["deltas"][off + lo:off + lo + m]
            dl[b:(n + 1) * n_step] = 0.0
            if K:
                ex[a:b] = case["extra"][off + lo:off + lo + m, :K]
            cursor[int(r)] = lo + n_step
        alive = np.asarray(step(n_alive, n_step, alive.copy(), sig, rgb, dl, ex), np.int32)
        calls += 1
        assert calls <= 2 * (max(COUNTS) + 2), "the wavefront loop does not end"
        if calls % 2 == 0 or not (alive >= 0).any():
            alive = alive[alive >= 0]
    return calls


def wavefront_reference(case, n_step, K=0, dtype=F64, T_thresh=None):
    """wavefront_run over wavefront_step in ``dtype`` from rays_t = case["t0"] -> dict(weights_sum, depth, image,
    extra_acc | None, rays_t, ratio [N by ray id], calls)."""
    N = len(case["rays"])
    T_thresh = case["T_wavefront"] if T_thresh is None else T_thresh
    st = dict(weights_sum=np.zeros(N, dtype), depth=np.zeros(N, dtype), image=np.zeros((N, 3), dtype),
              extra_acc=np.zeros((N, K), dtype) if K else None, rays_t=np.asarray(case["t0"], dtype).copy())
    track = dict(steps=np.zeros(N, np.int64), ratio=np.full(N, np.inf))

    def step(n_alive, n_step, alive, sig, rgb, dl, ex):
        wavefront_step(n_alive, n_step, alive, st["rays_t"], sig, rgb, dl, st["weights_sum"], st["depth"], st["image"],
                       T_thresh, ex, st["extra_acc"], dtype, track)
        return alive
    st["calls"] = wavefront_run(case, n_step, step, K)
    st["ratio"] = track["ratio"]
    return st


# ---------------------------------------------------------------------------- cross entropy rows
def ce_rows(logits, labels, n_classes, ignore_index, dtype=F64):
    """Per row: loss = logsumexp(x[:n_classes]) - x[y]; dpix = softmax - onehot over the classes, 0 in the padded
    channels >= n_classes; kept = y is a class and not ignore_index; bad = y is neither.  Rows not kept: loss 0, dpix 0.
    -> loss [N], dpix [N,K], kept bool [N], bad bool [N] in ``dtype``, one row after the other."""
    d = dtype
    x = np.asarray(logits, d)
    N, K = x.shape
    loss, dpix = np.zeros(N, d), np.zeros((N, K), d)
    kept, bad = np.zeros(N, bool), np.zeros(N, bool)
    for n in range(N):
        y = int(labels[n])
        in_range = 0 <= y < n_classes
        kept[n] = in_range and y != ignore_index
        bad[n] = (not in_range) and y != ignore_index
        if not kept[n]:
            continue
        m = x[n, 0]
        for k in range(1, n_classes):
            m = max(m, x[n, k])
        s = d(0.0)
        e = np.zeros(n_classes, d)
        for k in range(n_classes):
            e[k] = np.exp(x[n, k] - m)
            s = s + e[k]
        loss[n] = (m + np.log(s)) - x[n, y]
        for k in range(n_classes):
            dpix[n, k] = e[k] / s - (d(1.0) if k == y else d(0.0))
    return loss, dpix, kept, bad


# ---------------------------------------------------------------------------- cases
def ray_set(name):
    """COPIES x COUNTS shuffled, offsets = exclusive scan, ids a random permutation -> int32 [51, 3]."""
    rng = _rng("rays", name)
    cnt = rng.permutation(np.repeat(np.asarray(COUNTS, np.int64), COPIES))
    while cnt[-1] < 15:                                   # the last ray has samples: the dropped-ray cases cut its last one
                                                          # off, and the rows it leaves inside the buffer belong to nobody
        cnt = np.roll(cnt, 1)
    N = len(cnt)
    assert N % GROUP != 0
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return np.stack([rng.permutation(N), off, cnt], -1).astype(np.int32)


def _ints(rng, shape, k):
    return rng.integers(-k, k + 1, size=shape).astype(F32)


def one_hot_case(name, nan_behind=False):
    """The exact tier: delta = (2^-8, 2^-6); rgb, extra, g_* small integers; per ray sigma = 0 up to p, one opaque sample
    (sigma 2^15: sigma delta.x = 128, expf gives 0 and alpha == 1; one ray +inf), then finite non-negative garbage.
    p runs through P_CLASSES over the rays long enough for it, longest rays first; p = -1: transparent throughout.
    ``nan_behind``: the same case with NaN in sigma, rgb and extra strictly behind the opaque sample.
    -> dict(rays, sig, rgb, deltas, extra [M,64], g_ws, g_img, g_extra [N,64], p [N by row], t0 [N], T_wavefront)."""
    rng = _rng("one_hot", name)
    rays = ray_set(name)
    N, M = len(rays), int(rays[:, 2].sum())
    order = sorted(range(N), key=lambda n: (-int(rays[n, 2]), n))
    p = np.full(N, -1, np.int64)
    for j, n in enumerate(order):
        c = int(rays[n, 2])
        if c == 0:
            continue
        want = P_CLASSES[j % len(P_CLASSES)]
        if want == "transparent":
            continue
        p[n] = c - 1 if (want == "last" or want >= c) else want
    sig = np.zeros(M, F32)
    rgb, extra = _ints(rng, (M, 3), 4), _ints(rng, (M, KMAX), 3)
    garbage = rng.integers(0, 9, size=M).astype(F32) * F32(37.5)
    first_opaque = True
    for n in range(N):
        off, c = int(rays[n, 1]), int(rays[n, 2])
        if p[n] < 0:
            continue
        sig[off + p[n]] = np.inf if first_opaque else 2.0 ** 15
        first_opaque = False
        sig[off + p[n] + 1:off + c] = garbage[off + p[n] + 1:off + c]
        if nan_behind:
            sig[off + p[n] + 1:off + c] = np.nan
            rgb[off + p[n] + 1:off + c] = np.nan
            extra[off + p[n] + 1:off + c] = np.nan
    deltas = np.empty((M, 2), F32)
    deltas[:, 0], deltas[:, 1] = 2.0 ** -8, 2.0 ** -6
    return dict(name=name, rays=rays, sig=sig, rgb=rgb, deltas=deltas, extra=extra, g_ws=_ints(rng, N, 4),
                g_img=_ints(rng, (N, 3), 4), g_extra=_ints(rng, (N, KMAX), 3), p=p,
                t0=(rng.integers(0, 4, size=N) * 2.0 ** -6).astype(F32), T_wavefront=T_THRESH)


def one_hot_expected(case, K=0, M=None, absolute_depth=False):
    """What the exact tier must give, written down from p alone (fp32; every value is a small integer times a power of
    two).  ``M`` < total: rays that do not fit are dropped.  ``absolute_depth``: the wavefront form starts t at t0."""
    rays, p = case["rays"].astype(np.int64), case["p"]
    N, total = len(rays), case["sig"].shape[0]
    M = total if M is None else M
    out = dict(weights_sum=np.zeros(N, F32), depth=np.zeros(N, F32), image=np.zeros((N, 3), F32),
               weights=np.zeros(M, F32), extra_out=np.zeros((N, K), F32), sample_ray=np.full(M, -1, np.int32),
               grad_sigmas=np.zeros(M, F32), grad_rgbs=np.zeros((M, 3), F32), grad_extra=np.zeros((M, K), F32),
               n_used=np.zeros(N, np.int64))
    dx = F32(2.0 ** -8)
    for n in range(N):
        rid, off, c = (int(v) for v in rays[n])
        if off + c > M:
            out["sample_ray"][off:M] = rid
            continue
        out["sample_ray"][off:off + c] = rid
        g, gw = case["g_img"][rid], case["g_ws"][rid]
        if p[n] < 0:
            out["n_used"][n] = c
            out["grad_sigmas"][off:off + c] = dx * (case["rgb"][off:off + c] @ g + gw)
            continue
        i = off + int(p[n])
        out["n_used"][n] = p[n] + 1
        out["weights_sum"][rid] = 1.0
        out["image"][rid] = case["rgb"][i]
        out["depth"][rid] = F32((p[n] + 1) * 2.0 ** -6) + (case["t0"][rid] if absolute_depth else F32(0))
        out["weights"][i] = 1.0
        out["extra_out"][rid] = case["extra"][i, :K]
        out["grad_rgbs"][i] = g
        out["grad_sigmas"][off:i] = dx * ((case["rgb"][off:i] - case["rgb"][i]) @ g)
        out["grad_extra"][i] = case["g_extra"][rid, :K]
    return out


def regime_case(name, regime):
    """The tolerance tier: sigma = u^3 * s (s = 0.3, 40, 2000) or 0 everywhere; delta.x in [2e-3, 5e-3), delta.y in
    [0, 0.05); rgb in [0, 1); extra, g_* ~ N(0, 1); labels for 64 channels (each test reduces them modulo its class
    count).  Same keys as one_hot_case, without p."""
    rng = _rng("regime", name, regime)
    rays = ray_set(name + regime)
    N, M = len(rays), int(rays[:, 2].sum())
    sig = (rng.random(M) ** 3 * _SCALE[regime]).astype(F32)
    deltas = np.stack([2e-3 + 3e-3 * rng.random(M), 0.05 * rng.random(M)], -1).astype(F32)
    return dict(name=name, regime=regime, rays=rays, sig=sig, rgb=rng.random((M, 3)).astype(F32), deltas=deltas,
                extra=rng.normal(size=(M, KMAX)).astype(F32), g_ws=rng.normal(size=N).astype(F32),
                g_img=rng.normal(size=(N, 3)).astype(F32), g_extra=rng.normal(size=(N, KMAX)).astype(F32),
                t0=(0.05 + rng.random(N)).astype(F32), labels=rng.integers(0, KMAX, size=N).astype(np.int64),
                T_wavefront=WAVEFRONT_T40 if regime == "s40" else T_THRESH)


def last_ray_dropped_M(rays):
    """The largest M at which the last ray no longer fits."""
    return int(rays[-1, 1]) + int(rays[-1, 2]) - 1


def compared_rays(case, margin=None, ratio=None):
    """bool [N by row of rays]: the rays the tolerance comparisons keep.  ``margin`` (forward()) or ``ratio``
    (wavefront_reference(), by ray id).  Asserts the ambiguity cap: at most 2 % excluded, every count class kept."""
    rays = case["rays"]
    keep = margin >= MARGIN if margin is not None else ratio[rays[:, 0]] >= 1.0
    assert (~keep).sum() <= MAX_EXCLUDED * len(rays), f"{(~keep).sum()} of {len(rays)} rays ambiguous"
    for c in COUNTS:
        assert keep[rays[:, 2] == c].any(), f"no compared ray with {c} samples"
    return keep
