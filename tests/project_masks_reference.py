"""Restatement of the mask projector of csrc/raymarch.hip (k_project_masks_patch behind inr_project_masks_patch) and
the cases its tests run, NumPy and Python only: nothing here imports the product or oracle/.

The layout.  A frame's samples are patch-interleaved (k_composite_patch_fwd; the step rule of tests/sample_records_ref.py
decides only WHERE a sample lies, not its row): rays are taken in groups of 16 consecutive rows of ``rays``; at step k the
rays of a group that still have a sample (cnt > k) take consecutive rows in lane order; a group's rows follow the rows of
the groups before it.  rays[n] = (ray id, off, cnt); ``off`` of a group's first ray is the group's first row and is the
only offset the kernel reads (the others hold the exclusive scan of the counts, as the marcher's count pass leaves them).
A group whose rows do not fit, off + total > M, was dropped whole by the writer: its rays get zeros.  ``build_layout``
assigns the rows by walking the steps; tests/test_project_masks_cpu.py compares it with the closed-form slot map of
tests/composite_reference.py.

The operation.  out[rid][k_base + i] = sum over the ray's samples, in sample order, of w * bit_i(word(cell(x))) for
i < k_count; cell(x) = floor(((x - lo) / (hi - lo)) * res) per axis, inside if 0 <= cell < res on all three, the word at
((cx * L) + cy) * H + cz of a (W, L, H) volume; a sample with w == 0 is never read.  ``project32`` does this in fp32 in
that order - the GPU must equal it bit for bit - ``project64`` in float64 with float64 cells: the truth."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from detections_cases import uniform  # noqa: E402

F = np.float32
D = np.float64
GROUP = 16
U = 2.0 ** -24
SENTINEL = 0x7FC0BEEF                                   # the NaN pattern ``out`` starts with
FACE_REL = 2.0 ** -20
MAX_AMBIGUOUS = 0.005

N_SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)
COUNT_POOL = (0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 17, 17, 64)      # the draw; 200 comes in through the lone long ray
K_COMBOS = ((1, 0, 1), (31, 0, 31), (32, 0, 32), (33, 32, 1), (40, 32, 8), (64, 32, 32))   # (k_total, k_base, k_count)
VOLUMES = ((1, 1, 1), (3, 5, 7), (7, 9, 11))
BOX = (np.array([-1.0, -0.8, -0.6], F), np.array([0.9, 1.0, 0.7], F))   # strictly inside the sampled [-1.2, 1.2]^3
M_MODES = ("exact", "padded", "drop1", "drop2", "keep1", "zero")
TIERS = ("exact", "general")


# ---------------------------------------------------------------------------- layout
def build_layout(counts, ids):
    """-> rays int32 [N, 3], slots: list of int arrays (slots[n][k] = row of sample k of the ray in row n), total."""
    counts = [int(c) for c in counts]
    N = len(counts)
    rays = np.zeros((N, 3), np.int32)
    slots = [np.zeros(c, np.int64) for c in counts]
    pos = scan = 0
    for g0 in range(0, N, GROUP):
        c = counts[g0:g0 + GROUP]
        for k in range(max(c)):
            for r, cr in enumerate(c):
                if cr > k:
                    slots[g0 + r][k] = pos
                    pos += 1
    for n in range(N):
        rays[n] = (ids[n], scan, counts[n])
        scan += counts[n]
    return rays, slots, pos


def group_spans(rays):
    """[(first row, total)] per group, from the leader's offset and the group's counts."""
    return [(int(rays[g0, 1]), int(rays[g0:g0 + GROUP, 2].sum())) for g0 in range(0, len(rays), GROUP)]


def dropped_rays(rays, M):
    out = np.zeros(len(rays), bool)
    for g, (base, tot) in enumerate(group_spans(rays)):
        out[g * GROUP:(g + 1) * GROUP] = base + tot > M
    return out


# ---------------------------------------------------------------------------- cells
def cells32(xyz, lo, hi, res):
    """fp32, the kernel's order -> int64 [M, 3] cell per axis and inside bool [M]; NaN, +-inf: outside."""
    xyz, lo, hi = np.asarray(xyz, F), np.asarray(lo, F), np.asarray(hi, F)
    r = np.asarray(res, F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fl = np.floor(((xyz - lo) / (hi - lo)) * r)
        inside = ((fl >= 0) & (fl < r)).all(-1)
    return np.where(inside[:, None], fl, 0).astype(np.int64), inside


def cells64(xyz, lo, hi, res):
    """float64 on the same fp32 inputs -> cells, inside, u [M, 3] (the position in cell units)."""
    xyz, lo, hi = np.asarray(xyz, F).astype(D), np.asarray(lo, F).astype(D), np.asarray(hi, F).astype(D)
    r = np.asarray(res, D)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = ((xyz - lo) / (hi - lo)) * r
        fl = np.floor(u)
        inside = ((fl >= 0) & (fl < r)).all(-1)
    return np.where(inside[:, None], fl, 0).astype(np.int64), inside, u


def near_face(u, res):
    """bool [M]: some axis lies within FACE_REL (relative to the position in cell units, at least one cell) of a cell
    face - the only samples whose fp32 and float64 cells may differ: the fp32 cell position carries four roundings
    (x - lo, hi - lo, the quotient, the product), 2^-22 relative."""
    with np.errstate(invalid="ignore"):
        d = np.abs(u - np.round(u))
        return (d <= FACE_REL * np.maximum(np.abs(u), 1.0)).any(-1)


def words_at(words, cells, inside, vol):
    W, L, H = vol
    idx = (cells[:, 0] * L + cells[:, 1]) * H + cells[:, 2]
    return np.where(inside, np.asarray(words).astype(np.int64).reshape(-1)[np.where(inside, idx, 0)] & 0xFFFFFFFF, 0)


# ---------------------------------------------------------------------------- the projection
def _project(case, dt, cells, inside, out):
    rays, M = case["rays"], case["M"]
    k_total, k_base, k_count = case["k"]
    w_all = case["w"]
    word = words_at(case["words"], cells, inside, case["vol"]) if M else np.zeros(0, np.int64)
    drop = dropped_rays(rays, M)
    shifts = np.arange(32)
    for n, (rid, _, cnt) in enumerate(rays):
        acc = np.zeros(32, dt)
        if not drop[n]:
            for k in range(cnt):
                s = case["slots"][n][k]
                w = w_all[s]
                if w != 0 and inside[s]:
                    acc = acc + np.where((word[s] >> shifts) & 1, dt(w), dt(0.0))
        out[rid, k_base:k_base + k_count] = acc[:k_count]
    return out


def project32(case):
    """-> fp32 [n_rows, k_total] starting from the SENTINEL pattern: what ``out`` must hold, bit for bit."""
    out = np.full((case["n_rows"], case["k"][0]), SENTINEL, np.uint32).view(F)
    c, inside = cells32(case["xyz"], *case["box"], case["vol"]) if case["M"] else (None, None)
    return _project(case, F, c, inside, out)


def project64(case):
    """-> float64 [n_rows, k_total] (NaN where nothing is written), float64 cells."""
    out = np.full((case["n_rows"], case["k"][0]), np.nan, D)
    c, inside = cells64(case["xyz"], *case["box"], case["vol"])[:2] if case["M"] else (None, None)
    return _project(case, D, c, inside, out)


def sum_bound(case):
    """[n_rows]: cnt * 2^-24 * sum |w| per ray id - a sequential fp32 sum of cnt terms errs by at most (cnt - 1) u sum|w|."""
    out = np.zeros(case["n_rows"])
    for n, (rid, _, cnt) in enumerate(case["rays"]):
        if cnt and not dropped_rays(case["rays"], case["M"])[n]:
            out[rid] = cnt * U * float(np.abs(case["w"][case["slots"][n]].astype(D)).sum())
    return out


def ambiguous(case):
    """bool [M]: the fp32 and the float64 cell of the sample differ (as inside / which cell), for samples with weight."""
    if not case["M"]:
        return np.zeros(0, bool)
    c32, i32 = cells32(case["xyz"], *case["box"], case["vol"])
    c64, i64, _ = cells64(case["xyz"], *case["box"], case["vol"])
    return ((i32 != i64) | (c32 != c64).any(-1)) & (case["w"] != 0)


def rays_with(case, sample_mask):
    """bool [n_rows] by ray id: the ray owns a (kept) sample that ``sample_mask`` selects."""
    out = np.zeros(case["n_rows"], bool)
    for n, (rid, _, cnt) in enumerate(case["rays"]):
        s = case["slots"][n]
        s = s[s < case["M"]]
        out[rid] = bool(sample_mask[s].any())
    return out


# ---------------------------------------------------------------------------- cases
def _counts(N, seed):
    pick = (uniform(seed, N) * len(COUNT_POOL)).astype(int)
    c = [COUNT_POOL[p] for p in pick]
    if N >= 3 * GROUP:
        c[GROUP:2 * GROUP] = [0] * GROUP                           # a group of nothing
        c[2 * GROUP:3 * GROUP] = [1, 2] * (GROUP // 2)             # one ray much longer than the rest
        c[2 * GROUP + 11] = 200
    elif N >= 2:
        c[N // 2] = 200
    if N == 1:
        c[0] = 17
    return c


def _positions(total, seed, vol, box, tier):
    """-> xyz fp32 [total, 3], deliberate bool [total] (samples put ON a face).  "exact": cell centres +- a quarter cell
    and points half a cell outside, no face anywhere near.  "general": uniform in [-1.2, 1.2]^3 (outside the box on all
    six sides) and an eighth of the samples on a face of one axis: lo, hi, nextafter(hi, lo), an interior face."""
    lo, hi = (np.asarray(b, F) for b in box)
    res = np.asarray(vol, D)
    u = uniform(seed, 3 * total).reshape(total, 3)
    v = uniform(seed + 1, 3 * total).reshape(total, 3)
    deliberate = np.zeros(total, bool)
    if tier == "exact":
        cell = np.floor(u * (res + 2.0)) - 1.0                    # -1 .. res: one cell outside on either side
        pos = cell + 0.25 + 0.5 * v
        xyz = (lo.astype(D) + (hi.astype(D) - lo.astype(D)) * pos / res).astype(F)
        return xyz, deliberate
    xyz = (u * 2.4 - 1.2).astype(F)
    inner = (lo.astype(D) + (hi.astype(D) - lo.astype(D)) * (0.05 + 0.9 * u)).astype(F)    # a point inside the box
    kind = (v[:, 0] * 32).astype(int)                              # 0 .. 3: a face sample, its axis from v[:, 1]
    axis = (v[:, 1] * 3).astype(int)
    for i in np.flatnonzero(kind < 4):
        a = axis[i]
        xyz[i] = inner[i]
        if kind[i] == 0:
            xyz[i, a] = lo[a]
        elif kind[i] == 1:
            xyz[i, a] = hi[a]
        elif kind[i] == 2:
            xyz[i, a] = np.nextafter(hi[a], lo[a])
        else:
            j = 1 + int(v[i, 2] * max(vol[a] - 1, 1)) if vol[a] > 1 else 0
            xyz[i, a] = F(D(lo[a]) + (D(hi[a]) - D(lo[a])) * j / vol[a])
        deliberate[i] = True
    return xyz, deliberate


def _words(vol, seed, special):
    n = vol[0] * vol[1] * vol[2]
    hi16 = (uniform(seed, n) * 65536).astype(np.uint32)
    lo16 = (uniform(seed + 1, n) * 65536).astype(np.uint32)
    w = (hi16 << np.uint32(16)) | lo16
    if n == 1:
        w[0] = {"ones": 0xFFFFFFFF, "zeros": 0, None: 0x80000001 | w[0]}[special]
    else:
        w[0], w[1], w[2] = 0xFFFFFFFF, 0x00000000, 0x80000000
        w[n - 1] |= 0x80000000
    return w.view(np.int32).reshape(vol)


def make_case(N, tier="general", m_mode="exact", vol=(3, 5, 7), k=(32, 0, 32), nan_tail=False, box=BOX, special=None,
              seed=0):
    """One call of inr_project_masks_patch.  Arrays are cut to M rows; n_rows = N + 3 rows of ``out`` (ids are a
    permutation of a subset: rows no ray names stay untouched)."""
    seed = 1000 * N + 17 * seed + 1
    counts = _counts(N, seed)
    perm = np.argsort(uniform(seed + 1, N + 3), kind="stable")[:N]
    rays, slots, total = build_layout(counts, perm)
    xyz, deliberate = _positions(total, seed + 2, vol, box, tier)
    if tier == "exact":
        w = (np.floor(uniform(seed + 4, total) * 4096) / 4096).astype(F)          # multiples of 2^-12 below 1
    else:
        w = (uniform(seed + 4, total) * 1.5 - 0.25).astype(F)                     # a sixth negative: sum |w| matters
    if nan_tail:                                                                  # the last third of every ray: behind
        for n in range(N):                                                        # its termination point
            tail = slots[n][counts[n] - counts[n] // 3:]
            w[tail] = 0
            xyz[tail] = np.nan
    spans = group_spans(rays)
    full = [g for g, (b, t) in enumerate(spans) if t > 0]
    M = {"exact": total, "padded": total + 37, "zero": 0,
         "drop1": sum(spans[full[-1]]) - 1 if full else 0,
         "drop2": sum(spans[full[-2]]) - 1 if len(full) > 1 else 0,
         "keep1": sum(spans[full[1]]) - 1 if len(full) > 1 else 0}[m_mode]
    pad = max(M - total, 0)
    xyz = np.concatenate([xyz, np.full((pad, 3), np.nan, F)])[:M]
    w = np.concatenate([w, np.full(pad, np.nan, F)])[:M]
    deliberate = np.concatenate([deliberate, np.zeros(pad, bool)])[:M]
    return dict(N=N, M=M, total=total, rays=rays, slots=slots, counts=counts, xyz=np.ascontiguousarray(xyz), w=w,
                deliberate=deliberate, words=_words(vol, seed + 6, special), vol=vol, box=box, k=k, n_rows=N + 3, tier=tier,
                m_mode=m_mode, name=f"N{N}-{tier}-M{m_mode}-vol{'x'.join(map(str, vol))}-k{k}-nan{int(nan_tail)}")


DEGENERATE_BOX = (np.array([-1.0, 0.25, -0.6], F), np.array([0.9, 0.25, 0.7], F))


def all_cases():
    """name -> arguments of make_case: every list of the issue, each case a few thousand samples at the most."""
    out = []
    for N in N_SIZES:
        for tier in TIERS:
            out.append(dict(N=N, tier=tier))
    for m_mode in M_MODES[1:]:
        for tier in TIERS:
            out.append(dict(N=65, tier=tier, m_mode=m_mode))
    for tier in TIERS:
        out.append(dict(N=65, tier=tier, nan_tail=True))
        out.append(dict(N=257, tier=tier, nan_tail=True, m_mode="drop1"))
    for vol in VOLUMES:
        for k in K_COMBOS:
            if vol == (3, 5, 7) and k == (32, 0, 32):
                continue
            out.append(dict(N=65, vol=vol, k=k, seed=VOLUMES.index(vol)))
    out.append(dict(N=65, vol=(1, 1, 1), special="ones"))
    out.append(dict(N=65, vol=(1, 1, 1), special="zeros", tier="exact"))
    out.append(dict(N=65, box=DEGENERATE_BOX))
    out.append(dict(N=65, box=DEGENERATE_BOX, tier="exact", k=(40, 32, 8)))
    return out


def case_id(kw):
    return "-".join(f"{k}{'x'.join(map(str, v)) if isinstance(v, tuple) and k != 'box' else ('deg' if k == 'box' else v)}"
                    for k, v in kw.items())
