"""float64 reference of the two fused RENDER kernels of csrc/field_fused.hip (k_nerf_render behind inr_nerf_render,
k_instance_render behind inr_instance_render), the generators of their test cases and the tolerances of
tests/test_render_kernels.py.  numpy only.  It composes two existing references and adds nothing of its own to either:
field_forward_reference (per-sample float64 sigma, rgb and K logits with ``cond``, the arithmetic models, the exact
tier's tables and weights) and composite_reference (sequential float64 compositing with ``margin`` and ``n_used``,
patch_slot_map, dropped_groups, skippable, to_patch); positions are sample_records_ref's.  Nothing is shared with
instance_nerf_amd or oracle/.

nerf_render_ref(case).  sigma and rgb of every sample from field_forward_reference.Reference's encoder and networks at
the case's positions, each ray with SH-4 of its own direction; composite_reference.forward over the ray-major samples;
``weights`` placed at their patch rows by patch_slot_map.  A 16-ray group with base + total > M is dropped whole: its
rays give zeros, its ``weights`` rows (and every row from the cut on) are not written.
    evaluated = sum of the counts of the groups that fit  -  composite_reference.skippable(rays, n_used, M)
i.e. every sample of a step at which ANY ray of the group is still live, terminated rays of that step included.
``cond`` per output is the field's cond pushed through the compositing sums, absolute values accumulated along the ray.
The derivatives are those of the closed form of composite_reference.backward (d w_j / d sigma_j = dx_j T_{j+1},
d w_j / d sigma_i = -dx_i w_j for i < j), carried forward step by step together with one unit for each value that is
rounded on the way:
    cond(alpha_j) = dx_j (1 - alpha_j) cond(sigma_j) + 1
    cond(w_j)     = cond(alpha_j) T_j + alpha_j cond(T_j) + w_j
    cond(T_{j+1}) = cond(T_j) (1 - alpha_j) + T_j cond(alpha_j) + T_{j+1},   cond(T_0) = 0
    cond(weights_sum) = sum_j cond(w_j);  cond(depth) = sum_j t_j cond(w_j);
    cond(image) = sum_j (cond(w_j) rgb_j + w_j cond(rgb_j))
The unit in cond(alpha) is not decoration: alpha = 1 - e is rounded at the scale of 1, so behind a nearly opaque sample
(e = 1e-4) T = T (1 - alpha) carries a RELATIVE error of 2^-25 / e whatever the field's accuracy - without it the fp32
model itself sits 2e-3 cond away from float64 on ``weights``, in every build alike.
An element with cond == 0 must be exactly 0 (rays without samples, samples behind the termination point).

instance_render_ref(case, K).  out[rid, ch] = sum_k w[slot] * logits64(x[slot])[ch] with w an INPUT array;
cond = sum_k |w| cond(logits).

Cases (all from keyed _rng).
  Tolerance tier, TOL_CASES: 3 copies of COUNTS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 33, 130) in shuffled order, 33 rays = two
  full groups and a ragged group of one (7 / 8 / 9 and 15 / 16 / 17 straddle the eight-wave round robin of
  k_instance_render), ray ids a permutation, positions clamped ray samples o + t d, deltas in [0.005, 0.05]; level tables
  "bench" (dense and hashed lanes mixed) and "levels12" (dead slots); density_scale 1 / 0.3, bound 1 / 2, T_thresh 1e-4
  and once 0.05.  The field's own so0 spread of +-15 decides where rays stop; the seeds are chosen so that the float64
  reference alone gives, in every case, a ray that stops after its first sample, one that stops strictly inside, one that
  never stops, and a full group with a skipped step (tests/test_render_cpu.py asserts it).
  Exact tier, table "x16", density_scale 0.5: the forward suite's exact weights (sigma == density_scale, rgb == 0.5 on
  the data), deltas.x in {0, 1024} (alpha == 1 - expf(-0) == 0 or 1 - expf(-512) == 1), deltas.y distinct integers
  below 2^10 within a ray.  Each weight is 0 or 1, weights_sum 0 or 1, depth an integer prefix sum that names the slots
  used, image 0 or 0.5, evaluated exact: every output is compared bit for bit with the float64 result rounded to fp32.
  Rays: COUNTS x TERMINATION = ("transparent", "last", "first", 1, 7, 8, 9, 16), the opaque sample at min(k, count - 1).
  No identity needed an exception on the device: __expf(0) == 1, __frcp_rn(2) == 0.5, expf(-512) == 0 all hold.
  inr_instance_render there: the exact tier's integer logits, w from {0, 1, 2, 0.5, -1} with ~30 % zeros and one group
  whose steps from ZERO_FROM on are all zero: every product and sum exact in any order, bit equality for K = 16 .. 64.
  Schedule cases (exact tier, constant field: no encoder run): counts 0 .. 3, N = SCHEDULE_N (k_nerf_render: 1, 8, 40, 32
  and 256 workgroups on 256 CUs -> 1 / 8 / 32 owners, one chunk, several chunks, a second round, a ragged last chunk) and
  SCHEDULE_N_INSTANCE for k_instance_render (a workgroup per group: 8 owners, then a second round); every output buffer
  pre-filled with a NaN pattern, so "written exactly once with the right value" is "no NaN left and all bits equal".
  Dropped groups: M cut inside the last and inside the middle group of the exact case.
  Strict threshold: the exact case once more at T_thresh == 1 (T == T_thresh exactly at every boundary of a transparent
  prefix: the test is T < T_thresh, and the outputs are those at 1e-4).
  Never read: the exact case with NaN in ``deltas`` and ``xyzs`` strictly behind each ray's opaque sample (rows p+1 ..
  count-1 of every ray with an opaque sample).  deltas is loaded for live rays only; the positions of a terminated ray
  inside a live group still ride through the gather (NaN -> outside the volume -> zero features) and its weight must be
  exactly 0; no output bit may change.  (inr_nerf_render only.  inr_instance_render multiplies the logits of every
  sample of an evaluated step by its weight, and 0 * NaN is NaN: its positions are the marcher's and always finite.)

Tolerances.  TOL[build][output@numerics] = margin x MEASURED; MEASURED is the largest |model - float64| / cond over
TOL_CASES, measured on the CPU against the float64 reference (never against the kernel): the model is
field_forward_reference.model_for(build, numerics) feeding an fp32 sequential compositing in the kernel's operation order
(alpha = 1 - expf(-sigma dx); w = alpha T; image += w rgb; t += dy; depth += w t; ws += w; T *= 1 - alpha; image's
sigmoid with one reciprocal is the model's), for the instance kernel fp32 fma chains of the steps k = wave (mod 8) added
wave after wave.  Margin 8 for the default and fp32 numerics (MFMA-internal order, v_exp_f32 / v_rcp_f32, the device
expf), 2 for -O (operand rounding the device reproduces): the margins of the two suites being composed.
tests/test_render_cpu.py asserts that the models stay within TOL / margin.

Ambiguous rays.  A ray whose float64 ``margin`` is below BAND may stop one sample earlier or later in fp32.  BAND = 8 x
the model's largest |T_model - T_64| / max(T_64, T_thresh) over the boundaries at which the reference takes the test
(relative to T where the ray goes on, to T_thresh - the margin's own unit - at the boundary that stops it, where T_64 may
be 1e-300).  Such a ray is NOT skipped: its outputs must match, within TOL, the float64 result of ``n_used`` or of the
alternative with the test at its closest boundary flipped, its weights zero from the chosen stop on; ``evaluated`` is
exact in a case without an ambiguous ray, else between the alternatives' counts.  At most 2 % of a case's rays may be
ambiguous and every count class keeps an unambiguous ray: with 33 rays that is none, and the seeds are chosen so
(asserted on the CPU from the reference alone).
Ambiguous rays per case at the widest band (-O, 8 x 3.1e-2 = 0.25): bench 0, levels12 0, bench_T05 0 of 33; the smallest
margins are 0.69, 0.68 and 0.45 (SMALLEST_MARGIN).

Seen on an MI355X, worst |got - ref| / cond as a fraction of TOL (SEEN_ON_MI355X).  Default build, margin 8:
weights_sum 0.124, depth 0.122, image 0.115, weights 0.128, extra 0.124 (every K), the chained launch 0.086: the GPU sits
on the split model (1/8 = 0.125).  -O, margin 2: weights_sum 0.494, depth 0.498, image 0.468, weights 0.494, extra 0.485:
the device reproduces the operand roundings (1/2).  fp32 library: weights_sum 0.035, depth 0.035, image 0.040, weights
0.052, extra 0.142.  Exact tier, schedule, dropped-group, strict-threshold and never-read cases: every bit equal on both
libraries; no ray was ambiguous.
Mutations of csrc/field_fused.hip, each built once beside the tree and run once on the 35 default-build tests (never
committed); the two that can index past M were not run:
  T < T_thresh made <=                    1 fails: test_threshold_is_strict (T == T_thresh needs the case at T_thresh 1)
  n_eval += popc(livef)                   17 fail: every nerf test with a terminated ray in a live group (evaluated)
  zero fill of skipped weights removed    19 fail: exact, tolerance (NaN rows), chained, schedule, dropped, never-read
  tt += dl.y behind dsum += w * tt        17 fail: depth in both tiers
  k += kWaves - 1 (request to match)      15 fail: every instance test with a ray of 8 or more samples
  n_owner for owner in group_of           34 fail: groups never drawn keep their NaN pattern, from 3 groups on
  LDS parity fixed to 0                   0 fail: the reduction reads its eight partial sums right behind the barrier,
      the next group's first store into the same buffer waits for two dependent global loads (count, slot base) and a
      shuffle tree; the window did not open in 516 groups on 256 workgroups.  A timing fault no assertion here can force.
  rank mask (1u << j)                     not run: a step with one live ray writes slot S + 1, past M in the last group;
      the exact tier's ``depth`` (a prefix sum of distinct integers) and ``weights`` name the slot of every sample.
  if (S0 + gtot > M) kmax = 0 removed     not run: reads past M; test_dropped_groups asserts zeros for dropped rays.
"""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_reference as C  # noqa: E402
import field_forward_reference as R  # noqa: E402
import sample_records_ref as S  # noqa: E402
from field_forward_reference import Exact64, _rng, _u, worst_ratio  # noqa: E402,F401

F32, F64 = np.float32, np.float64
GROUP = 16
WAVES = 8                                   # k_instance_render: steps round robin over the workgroup's waves
CHUNK_LOG2 = 6                              # GroupDraw: 2^6 consecutive groups per cursor and round
COUNTS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 33, 130)
COPIES = 3
TERMINATION = ("transparent", "last", "first", 1, 7, 8, 9, 16)
KS = R.KS
ZERO_FROM = 3
W_VALUES = (0.0, 1.0, 2.0, 0.5, -1.0)
SCHEDULE_N = (37, 16 * 64, 16 * 320 - 5, 16 * 256, 16 * (2048 + 64 + 3) + 9)
SCHEDULE_N_INSTANCE = (37, 16 * 8, 16 * (512 + 3) + 9)
EXACT_TABLE = "x16"
MAX_AMBIGUOUS = 0.02
NUMERICS = {"": 0, "o": 3}
MARGIN = {"": 8.0, "o": 2.0}
OUTPUTS = ("weights_sum", "depth", "image", "weights")

# name -> level table, bound, density_scale, T_thresh, seed (chosen for the conditions of the module text)
TOL_CASES = {
    "bench": dict(table="bench", bound=1.0, ds=1.0, T=1e-4, seed=5),
    "levels12": dict(table="levels12", bound=2.0, ds=0.3, T=1e-4, seed=2),
    "bench_T05": dict(table="bench", bound=2.0, ds=0.3, T=0.05, seed=14),
}

# |model - float64| / cond, largest over TOL_CASES (value seen -> constant, two digits, rounded up)
MEASURED = {
    "bf16x3": {
        "weights_sum": 4.0e-07,     # 3.978e-07
        "depth": 1.9e-07,           # 1.861e-07
        "image": 5.9e-08,           # 5.837e-08
        "weights": 6.3e-07,         # 6.250e-07
        "extra": 1.9e-07,           # 1.883e-07
        "weights_sum@o": 1.1e-05,   # 1.086e-05
        "depth@o": 8.3e-06,         # 8.273e-06
        "image@o": 1.4e-06,         # 1.310e-06
        "weights@o": 2.1e-05,       # 2.076e-05
        "extra@o": 2.7e-06,         # 2.621e-06
    },
    "fp32": {
        "weights_sum": 6.7e-08,     # 6.627e-08
        "depth": 6.7e-08,           # 6.626e-08
        "image": 5.9e-08,           # 5.836e-08
        "weights": 8.4e-08,         # 8.341e-08
        "extra": 1.2e-09,           # 1.180e-09
    },
}
# largest |T_model - T_64| / max(T_64, T_thresh) at a test boundary (value seen -> constant); BAND is 8 x this
BAND_MEASURED = {
    "bf16x3": {"": 1.1e-03, "o": 3.1e-02},      # 1.008e-03, 3.013e-02
    "fp32": {"": 1.9e-04},                      # 1.842e-04
}
# smallest float64 margin of a ray, per case (value seen, rounded down): all above the widest band, 8 x 3.1e-2 = 0.25
SMALLEST_MARGIN = {"bench": 0.69, "levels12": 0.68, "bench_T05": 0.45}
SEEN_ON_MI355X = {
    "bf16x3": {"weights_sum": 0.124, "depth": 0.122, "image": 0.115, "weights": 0.128, "extra": 0.124,
               "weights_sum@o": 0.494, "depth@o": 0.498, "image@o": 0.468, "weights@o": 0.494, "extra@o": 0.485},
    "fp32": {"weights_sum": 0.035, "depth": 0.035, "image": 0.040, "weights": 0.052, "extra": 0.142},
}


def _tol(measured):
    return {b: {k: MARGIN[k.partition("@")[2]] * v for k, v in m.items()} for b, m in measured.items()}


TOL = _tol(MEASURED)
BAND = {b: {k: 8.0 * v for k, v in m.items()} for b, m in BAND_MEASURED.items()}


def tol_key(name, num):
    return name + ("@" + num if num else "")


# ---------------------------------------------------------------------------- rays and layouts
def ray_table(rng, cnt):
    """counts -> int32 [N,3] (ray id: a permutation; offset: exclusive scan; count)."""
    cnt = np.asarray(cnt, np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return np.stack([rng.permutation(len(cnt)), off, cnt], -1).astype(np.int32)


def sample_rows(rays):
    """-> (row of ``rays`` [total], step within the ray [total]) of every ray-major sample."""
    cnt = np.asarray(rays)[:, 2].astype(np.int64)
    row = np.repeat(np.arange(len(cnt)), cnt)
    step = np.arange(int(cnt.sum())) - np.repeat(np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
    return row, step


def slot_map(rays):
    """composite_reference.patch_slot_map, array form (the CPU suite asserts they agree): the patch row of every
    ray-major sample."""
    rays = np.asarray(rays).astype(np.int64)
    N = len(rays)
    G = -(-N // GROUP)
    cnt = np.zeros(G * GROUP, np.int64)
    cnt[:N] = rays[:, 2]
    cnt = cnt.reshape(G, GROUP)
    base = np.zeros(G, np.int64)
    base[:] = rays[::GROUP, 1]
    row, step = sample_rows(rays)
    g, r = row // GROUP, row % GROUP
    below = np.minimum(cnt[g], step[:, None]).sum(1)
    earlier = (cnt[g] > step[:, None]) & (np.arange(GROUP)[None, :] < r[:, None])
    return base[g] + below + earlier.sum(1)


def group_draw_owner(block, grid, pools):
    """GroupDraw::init -> (owner, n_owner) of workgroup ``block`` in a grid of ``grid``."""
    n_xcd = 8 if grid % 8 == 0 else 1
    n_pool = pools if grid % (8 * pools) == 0 else 1
    xcd = block & 7 if n_xcd == 8 else 0
    pool = (block >> 3) % pools if n_pool > 1 else 0
    return pool * n_xcd + xcd, n_pool * n_xcd


def group_of(u, owner, n_owner):
    """GroupDraw::group_of: the group behind position ``u`` of an owner's cursor."""
    chunk = (u >> CHUNK_LOG2) * n_owner + owner
    return (chunk << CHUNK_LOG2) + (u & ((1 << CHUNK_LOG2) - 1))


def render_grid(N, cus, kernel):
    """Workgroups of a launch (grid_for: a wave per group for k_nerf_render, a workgroup per group for
    k_instance_render, one workgroup per CU at most) -> (grid, n_owner)."""
    n_groups = -(-N // GROUP)
    grid = max(1, min(-(-n_groups // WAVES) if kernel == "nerf" else n_groups, cus))
    return grid, group_draw_owner(0, grid, 4 if kernel == "nerf" else 1)[1]


# ---------------------------------------------------------------------------- the field at a case's samples
class Field(R.Reference):
    """field_forward_reference.Reference at positions of the caller's: the table feed's encoder (x01 given) with the
    plain feed's SH of the sample's direction."""

    def __init__(self, case, mod=None, half_table=False, log=None):
        self.table, self.mod = case["table"], mod or Exact64(log)
        self.t = R.table_for(self.table)
        self.bound, self.ds = case["bound"], case["ds"]
        self.tier = R.tier_of(self.table)
        self.sc = dict(x01=case["x01"], dirs=case["dirs"])
        self.M = len(case["x01"])
        emb = R.embeddings(self.table)
        self.emb = R.rne_f16(emb) if half_table else emb.astype(F64)
        self.W = R.nerf_weights(self.table, case.get("variant"))
        self.log = log
        self._cache = {}

    def nerf(self):
        o, c = self.sigma("table")
        d = self.sc["dirs"]
        o2, c2 = R.colour_part(self.mod, self.W, self.mod.sh(d), R.sh_abs(d), o["so"], c["so"])
        return {**o, **o2}, {**c, **c2}

    def logits(self, K):
        o, c = R.instance_part(self.mod, R.instance_weights(self.table, K), *self._enc("table"))
        return o["logits"], c["logits"]


# ---------------------------------------------------------------------------- one ray, sample by sample
def ray_pass(sig, rgb, dl, th, csig=None, crgb=None, flip=None, dtype=F64):
    """The kernel's compositing of one ray in its operation order, every operation in ``dtype``.  flip: the boundary
    (index of the sample the test precedes) whose outcome is inverted.  -> dict(weights_sum, depth, image [3], w [cnt],
    n_used, Tb: T at every boundary tested, and with csig / crgb the cond of each output)."""
    d = dtype
    one, th = d(1.0), d(F32(th))
    T, t, ws, dep, img = one, d(0.0), d(0.0), d(0.0), np.zeros(3, d)
    cnt = len(sig)
    w_out, cw_out = np.zeros(cnt, d), np.zeros(cnt)
    cT = cws = cdep = 0.0
    cimg = np.zeros(3)
    Tb, n_used = [], 0
    for j in range(cnt):
        if j > 0:
            Tb.append(float(T))
            if (T < th) != (flip == j):
                break
        sg, dx = d(sig[j]), d(dl[j, 0])
        with np.errstate(under="ignore"):
            alpha = one - (d(math.exp(-sg * dx)) if d is F64 else np.exp(-sg * dx))
        w = alpha * T
        if csig is not None:
            ca = float(dx) * float(one - alpha) * csig[j] + 1.0
            cw = ca * float(T) + float(alpha) * cT + float(w)
            cT = cT * float(one - alpha) + float(T) * ca + float(T * (one - alpha))
        img = img + w * np.asarray(rgb[j], d)
        t = t + d(dl[j, 1])
        dep = dep + w * t
        ws = ws + w
        T = T * (one - alpha)
        w_out[j] = w
        n_used += 1
        if csig is not None:
            cws += cw
            cdep += float(t) * cw
            cimg = cimg + cw * np.asarray(rgb[j], F64) + float(w) * np.asarray(crgb[j], F64)
            cw_out[j] = cw
    return dict(weights_sum=ws, depth=dep, image=img, w=w_out, n_used=n_used, Tb=Tb,
                cond=dict(weights_sum=cws, depth=cdep, image=cimg, w=cw_out))


def _composite(case, sig, rgb, csig, crgb, M, dtype=F64, flips=None):
    """ray_pass over every ray of a group that fits -> outputs by ray id, weights in the patch layout (written: which
    rows a kernel writes), n_used / boundary values by row of ``rays``."""
    rays = case["rays"].astype(np.int64)
    N, total = len(rays), int(rays[:, 2].sum())
    slots = case["slots"]
    drop = C.dropped_groups(rays, M)
    out = dict(weights_sum=np.zeros(N), depth=np.zeros(N), image=np.zeros((N, 3)), weights=np.zeros(total))
    cond = {k: np.zeros_like(v) for k, v in out.items()}
    n_used, Tb = np.zeros(N, np.int64), [[] for _ in range(N)]
    written = np.zeros(total, bool)
    for n in range(N):
        rid, off, cnt = (int(v) for v in rays[n])
        if drop[n] or cnt == 0:
            continue
        sl = slice(off, off + cnt)
        r = ray_pass(sig[sl], rgb[sl], case["deltas"][sl], case["T"], None if csig is None else csig[sl],
                     None if crgb is None else crgb[sl], None if flips is None else flips.get(n), dtype)
        for k in ("weights_sum", "depth", "image"):
            out[k][rid], cond[k][rid] = r[k], r["cond"][k]
        out["weights"][slots[sl]], cond["weights"][slots[sl]] = r["w"], r["cond"]["w"]
        written[slots[sl]] = True
        n_used[n], Tb[n] = r["n_used"], r["Tb"]
    fit = int(rays[~drop, 2].sum())
    return dict(out=out, cond=cond, n_used=n_used, Tb=Tb, dropped=drop, written=written,
                evaluated=fit - C.skippable(rays, n_used, M))


def field_values(case, mod=None, half_table=False, log=None):
    """-> (sigma [total], rgb [total,3], cond sigma, cond rgb) of the ray-major samples."""
    if case.get("constant_field"):                       # exact tier: sigma == density_scale and rgb == 0.5 on the data
        total = int(case["rays"][:, 2].sum())
        return np.full(total, case["ds"]), np.full((total, 3), 0.5), np.ones(total), np.ones((total, 3))
    o, c = Field(case, mod, half_table, log).nerf()
    return o["sigma"], o["rgb"], c["sigma"], c["rgb"]


def nerf_render_ref(case, M=None):
    """The float64 reference of one inr_nerf_render launch with ``M`` rows (default: all) -> dict(weights_sum [N], depth
    [N], image [N,3] by ray id; weights [total] in the patch layout and written bool [total]; n_used, margin, dropped by
    row of rays; evaluated; cond: dict per output; sigma, rgb and their cond).
    evaluated = samples of the groups that fit - composite_reference.skippable(rays, n_used, M)."""
    rays = case["rays"]
    total = int(rays[:, 2].sum())
    M = total if M is None else int(M)
    sig, rgb, csig, crgb = field_values(case)
    fwd = C.forward(sig, rgb, case["deltas"], rays, case["T"])
    own = _composite(case, sig, rgb, csig, crgb, M)
    drop = own["dropped"]
    rid = rays[:, 0].astype(np.int64)
    out = {}
    for k in ("weights_sum", "depth", "image"):          # composite_reference.forward, dropped GROUPS zeroed
        out[k] = fwd[k].copy()
        out[k][rid[drop]] = 0.0
        assert np.array_equal(out[k], own["out"][k]), k
    out["weights"] = C.to_patch(fwd["weights"], case["slots"], total) * own["written"]
    assert np.array_equal(out["weights"], own["out"]["weights"])
    n_used = np.where(drop, 0, fwd["n_used"])
    assert np.array_equal(n_used, own["n_used"])
    fit = int(rays[~drop, 2].astype(np.int64).sum())
    evaluated = fit - C.skippable(rays, n_used, M)
    assert evaluated == own["evaluated"]
    return dict(out, written=own["written"], n_used=n_used, margin=np.where(drop, np.inf, fwd["margin"]), dropped=drop,
                evaluated=evaluated, cond=own["cond"], Tb=own["Tb"], sigma=sig, rgb=rgb, csigma=csig, crgb=crgb)


def nerf_render_model(case, build, num):
    """The CPU model of a build's launch: the field on model_for(build, num), fp32 sequential compositing."""
    mod, half = R.model_for(build, num)
    sig, rgb, _, _ = field_values(case, mod, half)
    total = int(case["rays"][:, 2].sum())
    return _composite(case, sig.astype(F32), rgb.astype(F32), None, None, total, dtype=F32)


def instance_inputs(case, K):
    """(w in the patch layout [total], ray-major w) of an inr_instance_render launch on ``case``."""
    rays = case["rays"]
    total = int(rays[:, 2].sum())
    rng = _rng("render_w", case["name"], K)
    if case["tier"] == "exact":
        w = rng.choice(np.asarray(W_VALUES, F32), size=total, p=(0.3, 0.2, 0.15, 0.2, 0.15)).astype(F32)
        row, step = sample_rows(rays)
        w[(row // GROUP == case.get("zero_group", 0)) & (step >= ZERO_FROM)] = 0.0
    else:
        w = rng.random(total, dtype=F32)
        w[rng.random(total) < 0.3] = 0.0
    return C.to_patch(w, case["slots"], total), w


def _wave_sum(w, lg, step, dtype):
    """One ray's sum over its samples as the kernel adds them: wave v takes the steps k = v (mod 8) in an fma chain,
    the eight partial sums are added wave after wave."""
    parts = np.zeros((WAVES, lg.shape[1]), dtype)
    for j in range(len(w)):
        v = int(step[j]) % WAVES
        parts[v] = (np.asarray(w[j], F64) * np.asarray(lg[j], F64) + parts[v].astype(F64)).astype(dtype)
    acc = parts[0]
    for v in range(1, WAVES):
        acc = (acc + parts[v]).astype(dtype)
    return acc


def instance_render_ref(case, K, w=None, M=None, mod=None, half_table=False, cw=None):
    """out[rid, ch] = sum_k w * logits64(x)[ch] over the ray's samples (w ray-major, default instance_inputs), dropped
    groups zero; cond = sum |w| cond(logits) (+ cond(w) |logits| when the weights carry an error cw of their own).
    With a model ``mod``: the kernel's fp32 order.  -> (out [N,K], cond [N,K])."""
    rays = case["rays"].astype(np.int64)
    N, total = len(rays), int(rays[:, 2].sum())
    M = total if M is None else int(M)
    w = instance_inputs(case, K)[1] if w is None else w
    if case.get("logit_pool") is not None:
        lg, cl = case["logit_pool"](K)
    else:
        lg, cl = Field(case, mod, half_table).logits(K)
    drop = C.dropped_groups(rays, M)
    out, cond = np.zeros((N, K)), np.zeros((N, K))
    for n in range(N):
        rid, off, cnt = (int(v) for v in rays[n])
        if drop[n] or cnt == 0:
            continue
        sl = slice(off, off + cnt)
        wj = np.asarray(w[sl], F64)
        if mod is None:
            out[rid] = (wj[:, None] * lg[sl]).sum(0)
        else:
            out[rid] = _wave_sum(np.asarray(w[sl], F32), lg[sl], np.arange(cnt), F32)
        cond[rid] = (np.abs(wj)[:, None] * cl[sl]).sum(0)
        if cw is not None:
            cond[rid] += (np.asarray(cw[sl], F64)[:, None] * np.abs(lg[sl])).sum(0)
    return out, cond


# ---------------------------------------------------------------------------- cases
def _finish_case(case, rng, x01, d_rows):
    rays = case["rays"]
    row, _ = sample_rows(rays)
    b = F32(case["bound"])
    case["x01"] = np.asarray(x01, F32)
    case["x"] = (case["x01"] * (2 * b) - b).astype(F32) if "x" not in case else case["x"]
    assert (S.x01_div(case["x"], case["bound"]) == case["x01"]).all() and (S.x01_mul(case["x"], case["bound"]) == case["x01"]).all()
    case["rays_d"] = np.asarray(d_rows, F32)
    case["dirs"] = case["rays_d"][row]
    case["slots"] = slot_map(rays)
    return case


def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


@functools.lru_cache(maxsize=None)
def tol_case(name, seed=None):
    """dict(name, tier, table, bound, ds, T, rays [33,3], x [total,3] / x01 / deltas [total,2] ray-major, rays_d [N,3] by
    row of rays, dirs per sample, slots)."""
    spec = TOL_CASES[name]
    rng = _rng("render_tol", name, spec["seed"] if seed is None else seed)
    rays = ray_table(rng, rng.permutation(np.repeat(np.asarray(COUNTS, np.int64), COPIES)))
    N, total = len(rays), int(rays[:, 2].sum())
    assert N % GROUP == 1
    b = spec["bound"]
    o, d = _u(rng, (N, 3), 0.9 * b), _unit(rng, N)
    row, _ = sample_rows(rays)
    t = np.empty(total, F32)
    for n in range(N):                                   # increasing along the ray, as a marcher leaves them
        off, cnt = int(rays[n, 1]), int(rays[n, 2])
        t[off:off + cnt] = np.sort(_u(rng, (cnt,), 0.5 * b) + F32(0.5 * b))
    x = S.position(o[row], d[row], t, b)
    deltas = (_u(rng, (total, 2), 0.0225) + F32(0.0275)).astype(F32)
    case = dict(name=name, tier="tol", table=spec["table"], bound=b, ds=spec["ds"], T=spec["T"], rays=rays, x=x,
                deltas=deltas)
    return _finish_case(case, rng, S.x01_mul(x, b), d)


def _exact_fill(case, rng, p):
    """deltas of the exact tier from the opaque sample p of every ray (-1: none); behind p finite garbage."""
    rays = case["rays"]
    total = int(rays[:, 2].sum())
    row, step = sample_rows(rays)
    dx = np.zeros(total, F32)
    behind = step > p[row]
    dx[(step == p[row])] = 1024.0
    has = p[row] >= 0
    dx[behind & has] = rng.choice(np.asarray((0.0, 1024.0), F32), size=int((behind & has).sum()))
    dy = np.empty(total, F32)
    for n in range(len(rays)):
        off, cnt = int(rays[n, 1]), int(rays[n, 2])
        dy[off:off + cnt] = rng.permutation(1023)[:cnt] + 1
    case["deltas"] = np.stack([dx, dy], -1)
    case["p"], case["behind"] = p, behind & has
    return case


@functools.lru_cache(maxsize=None)
def exact_case(name="exact"):
    """COUNTS x TERMINATION shuffled (88 rays: five full groups and a ragged one), positions on multiples of 1/8."""
    rng = _rng("render_exact", name)
    pairs = [(c, t) for c in COUNTS for t in TERMINATION]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    rays = ray_table(rng, [c for c, _ in pairs])
    p = np.asarray([-1 if (c == 0 or t == "transparent") else c - 1 if t == "last" else 0 if t == "first"
                    else min(int(t), c - 1) for c, t in pairs], np.int64)
    bound, ds = R.SETTINGS[EXACT_TABLE]
    N, total = len(rays), int(rays[:, 2].sum())
    # a group whose longest ray is long enough for ZERO_FROM to leave whole steps of zero weights
    zero_group = int(np.argmax([rays[g:g + GROUP, 2].max() for g in range(0, N, GROUP)]))
    case = dict(name=name, tier="exact", table=EXACT_TABLE, bound=bound, ds=ds, T=1e-4, rays=rays, term=pairs,
                zero_group=zero_group, variant="b")
    _exact_fill(case, rng, p)
    x01 = rng.integers(0, 9, size=(total, 3)).astype(F32) / F32(8)
    return _finish_case(case, rng, x01, _unit(rng, N))


def strict_case():
    """exact_case at T_thresh == 1: T is exactly 1 at every boundary before the opaque sample, and T < T_thresh is
    false there - the same outputs as at 1e-4, where T <= T_thresh would stop every ray after its first sample."""
    return dict(exact_case(), name="exact_T1", T=1.0)


def never_read_case():
    """exact_case with NaN in deltas and positions strictly behind every opaque sample (same expected outputs)."""
    case = dict(exact_case())
    case["deltas"], case["x"] = case["deltas"].copy(), case["x"].copy()
    case["deltas"][case["behind"]] = np.nan
    case["x"][case["behind"]] = np.nan
    case["poisoned"] = True
    return case


def constant_case(name, rng, cnt, p):
    """Exact tier with the field constant (sigma == density_scale, rgb == 0.5 wherever the sample lies): counts and the
    opaque sample of every ray (-1: none) given; positions from a pool of 64 grid points, so the K logits need one small
    encoder run."""
    rays = ray_table(rng, cnt)
    N, total = len(rays), int(rays[:, 2].sum())
    bound, ds = R.SETTINGS[EXACT_TABLE]
    case = dict(name=name, tier="exact", table=EXACT_TABLE, bound=bound, ds=ds, T=1e-4, rays=rays,
                constant_field=True, zero_group=0)
    _exact_fill(case, rng, np.asarray(p, np.int64))
    pool = rng.integers(0, 9, size=(64, 3)).astype(F32) / F32(8)
    pick = rng.integers(0, 64, size=total)
    _finish_case(case, rng, pool[pick], _unit(rng, N))

    @functools.lru_cache(maxsize=None)
    def logit_pool(K):
        lg, cl = Field(dict(case, x01=pool, dirs=np.zeros((64, 3), F32))).logits(K)
        return lg[pick], cl[pick]
    case["logit_pool"] = logit_pool
    return case


@functools.lru_cache(maxsize=2)
def schedule_case(N):
    """counts 0 .. 3; a quarter of the rays transparent, the others opaque at their first, second or third sample."""
    rng = _rng("render_schedule", N)
    cnt = rng.integers(0, 4, size=N)
    cls = rng.integers(0, 4, size=N)
    return constant_case(f"schedule{N}", rng, cnt, np.where((cls == 0) | (cnt == 0), -1, np.minimum(cls - 1, cnt - 1)))


def cut_M(case, where):
    """M that ends inside the last ("last") or the middle ("middle") group: one row short of that group's end."""
    rays = case["rays"].astype(np.int64)
    n_groups = -(-len(rays) // GROUP)
    g = n_groups - 1 if where == "last" else n_groups // 2
    assert rays[g * GROUP:(g + 1) * GROUP, 2].sum() > 0
    return int(rays[g * GROUP, 1] + rays[g * GROUP:(g + 1) * GROUP, 2].sum()) - 1


# ---------------------------------------------------------------------------- conditions, ambiguity, measurement
def termination_classes(case, ref):
    """The CPU-asserted conditions of a tolerance case, from the float64 reference alone."""
    rays = case["rays"].astype(np.int64)
    cnt, used = rays[:, 2], ref["n_used"]
    skipped = 0
    for g0 in range(0, len(rays) - GROUP + 1, GROUP):
        skipped = max(skipped, C.skippable(rays[g0:g0 + GROUP], used[g0:g0 + GROUP], int(cnt.sum())))
    return dict(first=int(((used == 1) & (cnt > 1)).sum()), inside=int(((used > 1) & (used < cnt)).sum()),
                never=int(((used == cnt) & (cnt > 1)).sum()), skipped_in_full_group=skipped)


def ambiguous_rays(case, ref, band):
    """{row of rays: boundary to flip} of the rays whose margin is below ``band``; asserts the cap (at most 2 % of the
    rays, every count class keeps an unambiguous ray)."""
    th = float(F32(case["T"]))
    flips = {}
    for n in np.flatnonzero(ref["margin"] < band):
        m = np.abs(np.asarray(ref["Tb"][n]) - th) / th
        flips[int(n)] = int(np.argmin(m)) + 1
    assert len(flips) <= MAX_AMBIGUOUS * len(case["rays"]), f"{len(flips)} of {len(case['rays'])} rays ambiguous"
    for c in set(int(v) for v in case["rays"][:, 2]):
        assert any(int(case["rays"][n, 2]) == c and n not in flips for n in range(len(case["rays"]))), c
    return flips


def alternative(case, ref, flips):
    """The float64 reference with the tests of ``flips`` inverted (same keys as nerf_render_ref's out / cond / evaluated)."""
    total = int(case["rays"][:, 2].sum())
    return _composite(case, ref["sigma"], ref["rgb"], ref["csigma"], ref["crgb"], total, flips=flips)


def measure(build, num, names=tuple(TOL_CASES)):
    """-> ({output@num: worst |model - float64| / cond}, worst |T_model - T_64| / max(T_64, T_thresh), {case: smallest
    margin}) over the tolerance cases."""
    worst, band, margins = {}, 0.0, {}
    for name in names:
        case = tol_case(name)
        ref, mod = nerf_render_ref(case), nerf_render_model(case, build, num)
        th = float(F32(case["T"]))
        margins[name] = float(ref["margin"].min())
        assert np.array_equal(ref["n_used"], mod["n_used"]), f"{name}: the {build}/{num} model stops elsewhere"
        for k in OUTPUTS:
            key = tol_key(k, num)
            worst[key] = max(worst.get(key, 0.0), worst_ratio(mod["out"][k], ref[k], ref["cond"][k]))
        for a, b in zip(ref["Tb"], mod["Tb"]):
            for t64, tm in zip(a, b):
                band = max(band, abs(tm - t64) / max(t64, th))
        m = R.model_for(build, num)
        for K in KS:
            w = instance_inputs(case, K)[1]
            want, cond = instance_render_ref(case, K, w)
            got, _ = instance_render_ref(case, K, w, mod=m[0], half_table=m[1])
            key = tol_key("extra", num)
            worst[key] = max(worst.get(key, 0.0), worst_ratio(got, want, cond))
    return worst, band, margins
