"""Directed inputs for the ray, march and compaction kernels of csrc/raymarch.hip (pure numpy, no GPU): every builder
returns a ``case`` - the arguments of one march call - plus, under ``promise``, the property it was built for, which
tests/test_march_cases_cpu.py checks with oracle/march.py before tests/test_march_kernels.py uses the case.

A case is a dict: o, d f32 [N,3]; bits u8 [C * H^3 / 8]; bound, C, H, dt_gamma, max_steps; nears, fars f32 [N];
noises f32 [N] or None; name; promise (a dict, see each builder).

Safety rules of every case (``check_safety``; preconditions of the ABI, include/inr.h): every direction is a nonzero
vector, every far is finite wherever near < far, and (far - t0) / dt_min <= 16384 - the marchers' loops advance t
by at least dt_min per candidate only while dt >= ulp(t) / 2, so an unbounded far in empty space never ends."""
import numpy as np

from oracle import march as omarch
from oracle import rays as orays
from oracle.occupancy import morton3D

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
MAX_CANDIDATES = 16384
SCAN_N_COOP = (1, 255, 256, 257, 1023, 1024, 1025, 4097)       # k_scan_counts: 1024 entries per trip
SCAN_N_LANE = (262144 - 1, 262144 + 300)                        # k_scan_block_sums: 1024 blocks of 256 rays per trip
COMPACT_N = (0, 1, 63, 64, 65, 255, 256, 257, 262144 + 300)
COMPACT_PATTERNS = ("all_alive", "all_dead", "alternating", "ends")


# ---------------------------------------------------------------------------- the candidate chain
def dt_of(t, max_steps, C, H, dt_gamma):
    dt_min, dt_max = omarch.dt_limits(max_steps, C, H)
    return np.minimum(np.maximum(np.asarray(t, F32) * F32(dt_gamma), dt_min), dt_max).astype(F32)


def candidates(t0, n, max_steps, C, H, dt_gamma):
    """c_0 = t0, c_{j+1} = c_j + clamp(c_j * dt_gamma, dt_min, dt_max), every operation one binary32 operation: the
    step candidates of a ray, which do not depend on the grid.  -> f32 [n]."""
    c = np.empty(n, F32)
    t = F32(t0)
    for j in range(n):
        c[j] = t
        t = F32(t + dt_of(t, max_steps, C, H, dt_gamma))
    return c


def start_t(case):
    """near + dt(near) * noise, the marchers' first candidate -> f32 [N]."""
    nears = np.asarray(case["nears"], F32)
    noises = np.zeros_like(nears) if case["noises"] is None else np.asarray(case["noises"], F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (nears + dt_of(nears, case["max_steps"], case["C"], case["H"], case["dt_gamma"]) * noises).astype(F32)


# ---------------------------------------------------------------------------- bitfields
def full(C, H):
    return np.full(C * H ** 3 // 8, 0xFF, np.uint8)


def empty(C, H):
    return np.zeros(C * H ** 3 // 8, np.uint8)


def set_cells(bits, H, cells, level=0):
    """Sets the bits of the cells [k,3] = (nx, ny, nz) of one cascade level, in place."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    idx = level * H ** 3 + morton3D(cells).astype(np.int64)
    np.bitwise_or.at(bits, idx >> 3, (1 << (idx & 7)).astype(np.uint8))
    return bits


def x_slab(C, H, xs, level=0):
    """Every cell whose x index is in ``xs``."""
    g = np.stack(np.meshgrid(np.asarray(xs), np.arange(H), np.arange(H), indexing="ij"), -1).reshape(-1, 3)
    return set_cells(empty(C, H), H, g, level)


def level_only(C, H, level):
    bits = empty(C, H)
    n = H ** 3 // 8
    bits[level * n:(level + 1) * n] = 0xFF
    return bits


def half_full(C, H, seed):
    return np.random.default_rng(seed).integers(0, 256, C * H ** 3 // 8).astype(np.uint8)


def _case(name, o, d, bits, nears, fars, *, bound=1.0, C=1, H=8, dt_gamma=0.0, max_steps=1024, noises=None, **promise):
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    n = o.shape[0]
    return dict(name=name, o=o, d=d, bits=np.ascontiguousarray(bits, np.uint8), bound=float(bound), C=int(C), H=int(H),
                dt_gamma=float(dt_gamma), max_steps=int(max_steps), nears=np.broadcast_to(np.asarray(nears, F32), (n,)).copy(),
                fars=np.broadcast_to(np.asarray(fars, F32), (n,)).copy(),
                noises=None if noises is None else np.broadcast_to(np.asarray(noises, F32), (n,)).copy(), promise=promise)


def check_safety(case):
    """The three rules of the module docstring; raises AssertionError."""
    d, near, far = case["d"], case["nears"], case["fars"]
    assert (np.abs(d).max(axis=1) > 0).all() and np.isfinite(d).all(), f"{case['name']}: a zero or non-finite direction"
    marches = near < far
    assert np.isfinite(far[marches]).all(), f"{case['name']}: an unbounded far on a ray that marches"
    dt_min, _ = omarch.dt_limits(case["max_steps"], case["C"], case["H"])
    t0 = start_t(case)
    steps = (far[marches].astype(np.float64) - t0[marches]) / float(dt_min)
    assert (steps <= MAX_CANDIDATES).all(), f"{case['name']}: {steps.max():.0f} candidates on one ray"
    assert case["bits"].size * 8 == case["C"] * case["H"] ** 3 and case["H"] >= 8
    if case["noises"] is not None:
        assert ((case["noises"] >= 0) & (case["noises"] < 1)).all()


def random_rays(n, seed, bound=1.0, min_near=0.05):
    """Origins inside twice the volume, unit directions towards a point of the volume: (o, d, nears, fars) with the
    slab test of oracle/rays.py (a miss: near = far = FLT_MAX, never marched)."""
    rng = np.random.default_rng(seed)
    o = (rng.uniform(-2, 2, (n, 3)) * bound).astype(F32)
    target = (rng.uniform(-1, 1, (n, 3)) * bound).astype(F32)
    d = target - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    aabb = np.asarray([-bound] * 3 + [bound] * 3, F32)
    nears, fars = orays.near_far_from_aabb(o, d, aabb, min_near)
    return o, d, nears, fars


def oracle(case, M=None):
    return omarch.march_rays_train(case["o"], case["d"], case["bits"], case["bound"], case["C"], case["H"], case["nears"],
                                   case["fars"], case["noises"], case["dt_gamma"], case["max_steps"], M)


def emitted_indices(case, ray, t_first_samples=None):
    """Candidate numbers of the samples the oracle emits for ``ray`` (by walking the ray's chain next to the oracle's
    deltas: the k-th sample is candidate j iff dt and t + dt - t_prev agree) -> int array.  For the promises only."""
    one = dict(case, o=case["o"][ray:ray + 1], d=case["d"][ray:ray + 1], nears=case["nears"][ray:ray + 1],
               fars=case["fars"][ray:ray + 1], noises=None if case["noises"] is None else case["noises"][ray:ray + 1])
    ref = oracle(one)
    t0 = start_t(one)[0]
    far = one["fars"][0]
    out, last, t, j = [], t0, t0, 0
    for k in range(ref["total"]):
        while True:
            assert t < far, "the oracle emitted past its chain"
            dt = dt_of(t, case["max_steps"], case["C"], case["H"], case["dt_gamma"])
            tn = F32(t + dt)
            p = np.minimum(np.maximum(one["o"][0] + t * one["d"][0], -F32(case["bound"])), F32(case["bound"])).astype(F32)
            hit = dt == ref["deltas"][k, 0] and F32(tn - last) == ref["deltas"][k, 1] and (p == ref["xyzs"][k]).all()
            t, j = tn, j + 1
            if hit:
                out.append(j - 1)
                last = tn
                break
    return np.asarray(out, np.int64)


# ---------------------------------------------------------------------------- the cases
AXIS_O, AXIS_D = (-0.9, 0.05, 0.05), (1.0, 0.0, 0.0)


def far_on_candidate():
    """Full grid, one axis ray per far in {c_63, next(c_63), c_64, next(c_64), c_65, c_128}: the count is
    #{j : c_j < far} = 63, 64, 64, 65, 65, 128 - `c < far` at a candidate EQUAL to far, at the window edge."""
    c = candidates(0.0, 129, 1024, 1, 8, 0.0)
    up = lambda x: np.nextafter(F32(x), F32(np.inf))
    fars = np.asarray([c[63], up(c[63]), c[64], up(c[64]), c[65], c[128]], F32)
    counts = [int((c < f).sum()) for f in fars]
    n = len(fars)
    return [_case("far_on_candidate", [AXIS_O] * n, [AXIS_D] * n, full(1, 8), 0.0, fars, counts=counts)]


def full_windows():
    """Full grid, far = 4.0 (beyond the volume: positions clamp at the face and stay occupied), the ray ends by
    max_steps: count == max_steps for 63, 64, 65, 127, 128, 129 - runs of 64 hits and the truncation inside a window."""
    o = [AXIS_O, (-0.5, -0.5, -0.5), (0.3, 0.9, -0.2)]
    d = [AXIS_D, tuple(F32(1 / np.sqrt(3)) for _ in range(3)), (0.0, -1.0, 0.0)]
    return [_case(f"full_windows_{m}", o, d, full(1, 8), 0.0, 4.0, max_steps=m, counts=[m] * 3) for m in (63, 64, 65, 127, 128, 129)]


def long_skip():
    """One occupied cell at the far end of an H = 8 row: every empty cell in front of it is one skip of ~74 candidates at
    max_steps = 1024 (more than a window) and ~296 at 4096 (more than two) - the pending skip that leaves the window."""
    bits = set_cells(empty(1, 8), 8, [[7, 4, 4]])
    o = [(-1.0, 0.1, 0.1), (-1.0, 0.01, 0.2), (-0.99, 0.13, 0.07)]
    d = np.asarray([(1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 0.002, 0.001)], np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return [_case(f"long_skip_{m}", o, d, bits, 0.0, 1.98, max_steps=m, min_skip=k) for m, k in ((1024, 64), (4096, 128))]


def skip_lands_on_lane():
    """Constant step, near = 0, o.x = -c_j, d = +x: the ray starts in the empty cell [-0.25, 0) whose exit distance is
    (0 - (-c_j)) * 1 = c_j exactly, so the first skip ends on tt == c_j bit for bit; everything at x >= 0 is occupied.
    j = 62, 63 land inside the first window, 64, 65 behind it.  The first sample is candidate j, at x == 0."""
    c = candidates(0.0, 70, 1024, 1, 8, 0.0)
    js = [62, 63, 64, 65]
    assert c[65] <= 0.25
    o = [(-c[j], 0.1, 0.1) for j in js]
    return [_case("skip_lands_on_lane", o, [AXIS_D] * 4, x_slab(1, 8, [4, 5, 6, 7]), 0.0, 1.0, landing=js)]


def pending_skip_rounding():
    """Rays (o.x, d.x picked by search) whose first skip, from candidate 0, ends behind the first window on candidate
    L, while the exit distance taken again from candidate 64 of the same empty cell rounds to the neighbour of L: the
    skip target must be carried over the window edge, not formed again.  o.x = -fl(c_j * d.x), cells x >= 0 occupied;
    both L and its neighbour lie at x >= 0, so the ray's first sample shows which one was taken."""
    rows = [(0.8238935470581055, -0.18952670693397522, 69, 68), (0.8238935470581055, -0.19231386482715607, 70, 69),
            (0.6660082936286926, -0.15320712327957153, 69, 68), (0.5676186084747314, -0.12865357100963593, 67, 68),
            (0.5676186084747314, -0.1324939727783203, 69, 70), (0.5571069121360779, -0.12438639998435974, 66, 67)]
    o = [(ox, 0.1, 0.1) for _, ox, _, _ in rows]
    d = [(dx, 0.0, 0.0) for dx, _, _, _ in rows]
    return [_case("pending_skip_rounding", o, d, x_slab(1, 8, [4, 5, 6, 7]), 0.0, 1.0, landing=[r[2] for r in rows],
                  landing_from_64=[r[3] for r in rows])]


def landing_guess_edge():
    """Constant step, a miss in lane 0 whose skip ends INSIDE the window, a few ulps above candidate j (rows picked by
    search, o.x = -fl(c_j * d.x)): c_j < tt, so the skip lands on j + 1, while floor((tt - c_0) * (1 / dt)) + 1 == j -
    the constant-step estimate of the landing lane is one short and only its probes (c_i < tt) tell.  Candidate j lies
    at x == 0, in the occupied slab: a marcher that lands there emits one sample too many."""
    dx = 0.7798079252243042
    rows = [(-0.03165625408291817, 12), (-0.04220833256840706, 16), (-0.1187109500169754, 45), (-0.1503671556711197, 57)]
    o = [(ox, 0.1, 0.1) for ox, _ in rows]
    return [_case("landing_guess_edge", o, [(dx, 0.0, 0.0)] * len(rows), x_slab(1, 8, [4, 5, 6, 7]), 0.0, 1.0,
                  landing=[j + 1 for _, j in rows])]


def sparse_hits():
    """Isolated occupied cells (x index 2, 5 and 7 of a row, and the same as slabs) at 74 and at 18.5 candidates per
    cell: a skip lands on an occupied cell (a hit in the first lane of the next window), the cell's run of hits fills
    a window to its last lane and goes on in the next one, and windows in empty space have no hit at all."""
    o = [(-1.0, 0.1, 0.1), (-0.93, 0.1, 0.1), (-1.0, 0.12, 0.03), (1.0, 0.1, 0.1)]
    d = np.asarray([(1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 0.004, 0.003), (-1.0, 0.0, 0.0)], np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    cells = set_cells(empty(1, 8), 8, [[2, 4, 4], [5, 4, 4], [7, 4, 4]])
    return [_case("sparse_hits_cells_1024", o, d, cells, 0.0, 1.9, max_steps=1024, run=64, gap=64),
            _case("sparse_hits_slabs_1024", o, d, x_slab(1, 8, [2, 5, 7]), 0.0, 1.9, max_steps=1024, run=64, gap=64),
            _case("sparse_hits_slabs_256", o, d, x_slab(1, 8, [2, 5, 7]), 0.0, 1.9, max_steps=256, run=10, gap=10)]


def cascade_edges():
    """C = 2, 3 and bound = 2, 4 with ONE level occupied.  Ray 0: o.x = 0.5, near = 0.5, d = +x - its first candidate is
    at max|p| == 1.0 exactly, where frexp gives exponent 1: level 1.  Ray 1: o.x = 0.5 - 2^-24, one ulp below 1: level 0.
    Rays 2, 3 the same at 2.0 (o.x = 1.5).  dt_gamma = 1/4 and H = 8: dt * H * 0.5 crosses 1 at t = 1, where the step
    size lifts the level.  The rest are random rays."""
    out = []
    for C, bound in ((2, 2.0), (3, 4.0), (3, 2.0)):
        ro, rd, rn, rf = random_rays(28, 100 + C, bound)
        o = np.concatenate([np.asarray([(0.5, 0, 0), (0.5 - 2.0 ** -24, 0, 0), (1.5, 0, 0), (1.5 - 2.0 ** -23, 0, 0)], F32), ro])
        d = np.concatenate([np.asarray([AXIS_D] * 4, F32), rd])
        nears = np.concatenate([np.full(4, 0.5, F32), rn])
        fars = np.concatenate([bound + 1.0 - o[:4, 0], rf]).astype(F32)      # beyond the face: positions clamp
        for level in range(C):
            for g in (0.0, 0.25):
                out.append(_case(f"cascade_C{C}_b{bound:g}_l{level}_g{g:g}", o, d, level_only(C, 8, level), nears, fars,
                                 bound=bound, C=C, dt_gamma=g, max_steps=64, level=level))
    return out


def signed_zero_dirs():
    """Axis-parallel rays with +0 and with -0 in the other two components, origins on cell faces (multiples of 2 / H)
    and at +-bound: the exit distance of a miss multiplies (face - p) == 0 by 1 / d == +-inf on those axes - NaN, which
    the minimum must drop.  Rays 2k (+0) and 2k + 1 (-0) must give the same samples."""
    o, d = [], []
    for axis in range(3):
        for y, z in ((0.25, 0.5), (-1.0, 1.0), (0.0, -0.75), (1.0, 0.1)):
            for sgn in (1.0, -1.0):
                for zero in (0.0, -0.0):
                    oo, dd = [y, z], [zero, zero]
                    oo.insert(axis, -sgn)
                    dd.insert(axis, sgn)
                    o.append(oo)
                    d.append(dd)
    return [_case("signed_zero_dirs", o, d, half_full(1, 8, 7), 0.0, 2.0, max_steps=64, pairs=len(o) // 2)]


def no_samples():
    """Rays that emit nothing: near > far, near == far, the slab test's miss (both FLT_MAX), NaN near, NaN far, and
    an ordinary ray in an empty grid.  Count 0 each, total 0."""
    nears = np.asarray([1.5, 1.0, FLT_MAX, np.nan, 0.0, 0.05], F32)
    fars = np.asarray([0.5, 1.0, FLT_MAX, 2.0, np.nan, 1.9], F32)
    o = [AXIS_O] * 6
    return [_case("no_samples_full", o[:5], [AXIS_D] * 5, full(1, 8), nears[:5], fars[:5], max_steps=64, counts=[0] * 5),
            _case("no_samples_empty", o, [AXIS_D] * 6, empty(1, 8), nears, fars, max_steps=64, counts=[0] * 6)]


def noise_edges():
    """noises = 0, nextafter(1, 0), a mix, and NULL (the same as 0) on one random scene."""
    o, d, nears, fars = random_rays(64, 11)
    one = np.nextafter(F32(1), F32(0))
    mix = np.where(np.arange(64) % 2 == 0, F32(0), one).astype(F32)
    bits = half_full(1, 8, 12)
    return [_case(f"noise_{k}", o, d, bits, nears, fars, max_steps=64, noises=v)
            for k, v in (("null", None), ("zero", F32(0)), ("almost_one", one), ("mix", mix))]


def scan_trips(n):
    """n random rays, max_steps = 16, H = 8, a random half-full grid: offsets == exclusive cumsum across the scan trips."""
    o, d, nears, fars = random_rays(n, 1000 + n % 997)
    return _case(f"scan_trips_{n}", o, d, half_full(1, 8, 13), nears, fars, max_steps=16, noises=None)


def capture_edges():
    """Lane-per-ray captures (sample_cap 32 -> one 32-candidate word, 33 and 64 -> two).  A: full grid, far set so
    that the ray's LAST emitted candidate is number 30, 31, 32, 33, 62, 63, 64, 65: number 32w - 1 still replays from w
    words, number 32w is re-marched.  B: slabs x < 2 and x >= 5 occupied, all 16 rays on the same chain (max_steps = 64,
    ~4.6 candidates per cell): candidates 16..23 lie in the gap for every ray of the wave, 37 candidates in all."""
    c = candidates(0.0, 70, 1024, 1, 8, 0.0)
    last = [30, 31, 32, 33, 62, 63, 64, 65]
    a = _case("capture_A", [AXIS_O] * 8, [AXIS_D] * 8, full(1, 8), 0.0, [np.nextafter(c[j], F32(np.inf)) for j in last],
              last=last)
    yz = np.random.default_rng(5).uniform(-0.9, 0.9, (16, 2))
    o = np.concatenate([np.full((16, 1), -1.0), yz], 1)
    b = _case("capture_B", o, [AXIS_D] * 16, x_slab(1, 8, [0, 1, 5, 6, 7]), 0.0, 2.0, max_steps=64, empty_stretch=(16, 24))
    return [a, b]


def cap_words(sample_cap):
    return (sample_cap + 31) // 32 if sample_cap > 0 else 0


def replays(last_emitted, sample_cap):
    """A captured ray is replayed iff every emitted candidate lies in the cap_words * 32 recorded ones."""
    return last_emitted < cap_words(sample_cap) * 32


def buffer_cuts_scene():
    """37 rays (not a multiple of the 16-ray group), max_steps = 32, rays with count 0 among them."""
    o, d, nears, fars = random_rays(37, 21)
    return _case("buffer_cuts", o, d, half_full(1, 8, 22), nears, fars, max_steps=32)


def buffer_cuts(rays):
    """The M of the table for an [N,3] rays array (ray, offset, count) -> {label: M}."""
    N = rays.shape[0]
    total = int(rays[-1, 1] + rays[-1, 2])
    long_rays, some = np.nonzero(rays[:, 2] >= 2)[0], np.nonzero(rays[:, 2] > 0)[0]
    r, b = int(long_rays[len(long_rays) // 2]), int(some[len(some) // 3])
    return {"zero": 0, "one": 1, "total-1": total - 1, "total": total, "total+1": total + 1, "total+N-1": total + N - 1,
            "total+N+1": total + N + 1, "inside_ray": int(rays[r, 1] + 1), "ray_boundary": int(rays[b, 1] + rays[b, 2])}


def owned_rows(rays, M):
    """bool [M]: the row belongs to a ray the ray-major writers keep (offset + count <= M)."""
    own = np.zeros(M, bool)
    for _, off, cnt in rays:
        if cnt > 0 and off + cnt <= M:
            own[off:off + cnt] = True
    return own


def all_train_cases():
    """Every case a training marcher runs (the scan trips and the buffer cuts have tests of their own)."""
    out = []
    for b in (far_on_candidate, full_windows, long_skip, skip_lands_on_lane, pending_skip_rounding, landing_guess_edge,
              sparse_hits, cascade_edges, signed_zero_dirs,
              no_samples, noise_edges, capture_edges):
        out += b()
    return out + [buffer_cuts_scene()]


# ---------------------------------------------------------------------------- compaction
def alive_pattern(n, pattern):
    a = np.arange(n, dtype=np.int32) * 3 + 1            # distinct, not the positions: order and values both show
    if pattern == "all_dead":
        a[:] = -1
    elif pattern == "alternating":
        a[1::2] = -1
    elif pattern == "ends":
        a[1:-1] = -1
    return a
