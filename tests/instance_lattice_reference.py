"""Plain float64 restatement of the 3-D instance-mask launches (csrc/field_fused.hip: k_instance_lattice in its four
K_MT instantiations - inr_instance_lattice - and k_instance_stats_partial / k_instance_stats_final -
inr_instance_volume_stats), the generators of their test cases and the tolerances of
tests/test_instance_lattice_kernels.py.  numpy only; the encoder, the two networks, the arithmetic models, TOL, the level
tables and the weights are field_forward_reference's (imported, not copied).

Specification, per voxel (iw, il, ih) of a [W, L, H] lattice, h fastest: position (ax_w[iw], ax_l[il], ax_h[ih]), every
axis value clamped to [-bound, bound] first, x01 = (x + bound) / (2 bound) (``x01_lattice``).  The NeRF's table and sigma
net give the density logit so0 (written as it is to density_logit when that is asked for); the voxel is OCCUPIED when
exp(so0) * density_scale >= sigma_thresh (>=: a voxel exactly on the threshold is occupied).  The INSTANCE field has a
table of its own - own values, own level table - and the net 64 <- 32, 64 <- 64, K <- 64; of its K real logits (K = 1 ..
64; the packed weights hold 16 * ceil(K / 16) rows, the padding rows zero and never candidates) an occupied voxel gets
label = arg-max, the LOWEST channel on ties, and confidence = 1 / sum_c exp(l_c - max); an unoccupied voxel gets label
255 and confidence exactly 0.  Every voxel is written exactly once, nothing else is.

The kernel walks runs ("tiles") of 16 voxels along W, W padded to a multiple of 16 (the padded lanes compute voxel W - 1
again and write nothing); a tile without an occupied voxel skips the instance field.  A voxel's channel c = 16 mt + 4 q + r
lives in register (mt, r) of its lane q, so the arg-max runs over a lane's channels in ascending order, then across the
four q lanes; ``TIE_PAIRS`` names one pair of channels per way two equal maxima can meet (same lane, across q, across
mt, the last real channel of a padded tile).  ``tiles`` restates which voxels share a tile.

Tolerances.  The density logit uses field_forward_reference's TOL["logit"] * cond(so0); logits enter only through
labels and confidence.  Label: equal to the reference wherever the reference's top-2 margin is above the band
2 * TOL["logits"] * max_c cond_c; inside the band the label must be a channel within the band of the reference maximum.
Confidence: cond_conf = conf * sum_c p_c (cond_c + cond_best), p = softmax; |got - ref| <= TOL["conf"] * cond_conf +
the device term.  TOL["conf"] = 8 x MEASURED["conf"], MEASURED the largest |model - float64| / cond_conf of the build's
model (SplitBf16 / SeqFp32 logits, then the kernel's fp32 steps l_c - max, __expf, sum, 1 / s) over the tolerance
cases, measured on the CPU (tests/test_instance_lattice_cpu.py asserts the models stay within TOL / 8).  The device
term is what no CPU model measures, derived as ROUNDING_TOL is: per channel v_exp_f32 of (l_c - max) * log2(e) - the
argument's rounding moves the result by |l_c - max| * log2(e) * 2^-24 relative, the instruction is within 1 ulp - the
sum and v_rcp_f32: conf * sum_c p_c * 8 * 2^-24 * (1 + |l_c - max| * log2(e)).  The maximum is continuous, so no voxel
is left out of the confidence comparison.  Exact tier: the logits are exact, so the confidence is within the device
term alone, exactly 1.0 for K = 1.

Thresholds.  Per case sigma_thresh = float32(density_scale * exp(mid)), mid the middle of the widest gap between
neighbouring reference logits around a quantile (``threshold``); the gap must exceed 2 * (TOL["logit"] * max cond(so0) +
8 * 2^-24 * (1 + |mid|)) (the logit's tolerance and the device's exp, product and the threshold's own rounding), so the
occupancy of EVERY voxel is compared.  Tolerance tier: quantiles 0.5 and 0.9; exact tier: mid between two distinct exact
values next to the 0.5 and 0.9 quantiles of the distinct values; both: sigma_thresh = 0 (all occupied) and twice the
largest sigma (none).  On the exact tier's so0 == 0 weights sigma == density_scale: sigma_thresh = density_scale is all
occupied, nextafter(density_scale, inf) none.

The 313 k-voxel lattice of the interleaved split has no such gap near a quantile (``tail_threshold``): it runs with
sigma_thresh = 0 (every tile through the instance field) and with the lowest usable gap among its 256 largest logits (a
few dozen mixed tiles, every other tile skipped).

Inputs.  NeRF side: field_forward_reference's tables, values, weights ("logit" density row in the exact tier) and
SETTINGS (bound 1, 1.5, 2; density_scale 1, 0.3, powers of two).  Instance side: ``INST_TABLE`` names the instance
field's level table (bench / hashed_all, dense_coarse / bench, x16 / x12 differ from the NeRF's: a kernel that mixes the
two tables' level records or buffer resources reads other rows), its values are another draw (``inst_embeddings``),
its weights field_forward_reference.instance_weights, padded with zero rows by the launcher.  Axes: U(+-bound), one value
of ax_w (W > 4) and of ax_h (H > 1) outside the bound; exact tier: x01 on multiples of 1/8.

Statistics (``stats_reference``), bit for bit in fp32: n_blocks = clamp(ceil(N / 1024), 1, 512), per_block = ceil(N /
n_blocks); workgroup b owns voxels [b per_block, min(N, (b + 1) per_block)); its wave w takes the 64-voxel chunks at
b per_block + 64 w + 256 i; per chunk and label present, the confidences of that label (0 elsewhere) go through the xor
butterfly 32, 16, ..., 1 and lane 0's value is added to the wave's sum in chunk order; waves 0..3 are added in order
to 0; the final pass folds workgroups g, g + 8, ... per group g and then groups 0..7 in order.  counts and boxes are
integers, boxes -1 for an empty channel; labels >= K are ignored.

Seen on the CPU (asserted by tests/test_instance_lattice_cpu.py): threshold gaps 2.4 .. 84 times the need on the
tolerance tier's main lattices; at the 0.9 quantile every one of them has empty and mixed tiles, every W = 19 / 33 one an
empty padded tail tile, bench at (33, 2, 3) a tile whose valid voxels are all occupied; reference ties on 4 .. 14 % of
the voxels of the exact cases with K > 1; at most 3.1 % of a tolerance case's voxels inside the label band.

Seen on an MI355X, worst |got - ref| as a fraction of its tolerance, per output.  Default build: density_logit 0.153
(levels5_b15 at (48, 5, 7); 0.098 on the interleaved split); confidence, tolerance tier 0.118 (levels5_b15, K = 64;
0.067 on the interleaved split), i.e. the GPU sits on the split model (1 / 8 = 0.125); confidence, exact tier 0.167 of
the device term alone (x16 at (16, 1, 1), K = 16), exactly 1.0 for K = 1; occupancy and labels equal on every voxel
compared, every exact-tier bit of density_logit equal.  fp32 library: density_logit 0.114, confidence 0.049 (tolerance
tier), 0.167 (exact tier).  Statistics: every bit equal, conf_sum included, twice.
Mutations of csrc/field_fused.hip, each built once beside the tree and run on the 62 tests of
tests/test_instance_lattice_kernels.py (never committed):
  (a) cross-lane tie rule oi < bi -> oi > bi      first failure test_lattice[x16-19x3x5-K16]; 18 of 62 fail (the five
      exact main-lattice cases with K > 1 - the small lattices hold no tie across lanes -, all eight tie-pair tests - the
      duplicated pair is not the only tie of its lattice -, three of the all-negative cases with K = 5 and 31, both
      threshold-pair cases; the tolerance tier, where two logits are never equal, rightly passes).
  (b) c < K dropped from the arg-max              first failure test_lattice[hashed_all-19x3x5-K5]; 11 of 62 fail (K = 1
      and 5 wherever every real logit is negative, and all six all-negative cases, K = 31 included: label K).
  (c) >= turned to > in occ                       first failure test_a_voxel_on_the_threshold_is_occupied[x16]; 2 of 62
      fail (nothing else puts a voxel exactly on the threshold: the gap conditions keep every other voxel off it).
  (d) final fold in plain workgroup order         first failure test_volume_stats_equal_the_restatement_bit_for_bit[cap1];
      3 of 62 fail (cap1, cap5, cap64: with at most eight workgroups the two orders are the same order).
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_forward_reference as R  # noqa: E402
from field_forward_reference import (Exact64, encode, sigma_part, instance_part, tier_of, table_for, embeddings,  # noqa: E402
                                     nerf_weights, instance_weights, x01_lattice, SETTINGS, MARGIN, _rng, _u)
from field_forward_reference import B  # noqa: E402

F32, F64 = np.float32, np.float64
BUILDS = R.BUILDS
LABEL_EMPTY = 255
LOG2E = 1.4426950408889634
DEVICE_ULP = 8 * 2.0 ** -24

# |model confidence - float64| / cond_conf, largest over the tolerance-tier cases (value seen -> constant, two digits,
# rounded up), recorded as field_forward_reference.MEASURED records the others
MEASURED = {
    "bf16x3": {"conf": 1.7e-07},            # 1.629e-07
    "fp32": {"conf": 4.6e-09},              # 4.541e-09
}
TOL = {b: dict(R.TOL[b], conf=MARGIN[""] * MEASURED[b]["conf"]) for b in BUILDS}

TOL_TABLES = ("bench", "hashed_all", "levels5_b15", "dense_coarse")
EXACT_TABLES = ("x16", "x12")
# NeRF table -> the instance field's level table
INST_TABLE = {"bench": "hashed_all", "hashed_all": "hashed_all", "levels5_b15": "levels5", "dense_coarse": "bench",
              "x16": "x12", "x12": "x12"}
MAIN_LATTICES = ((19, 3, 5), (33, 2, 3), (48, 5, 7))
SMALL_LATTICES = ((1, 1, 1), (15, 1, 2), (16, 1, 1), (17, 2, 1))
KS = (16, 31, 64, 5, 48, 1)
BIG_CASE = ("bench", (19, 128, 129), 16)          # 32 * 128 * 129 / 16 = 33024 tiles: the interleaved XCD split
SMALL_TILES = 1368                                # the lattice of tests/test_instance_extract.py
HYBRID_MIN_TILES = R.HYBRID_MIN_TILES             # make_sched: (n_tiles >> (kXcdChunkLog2 + 3)) >= 4
# channel pairs whose equal maxima meet (a) in one lane's registers of one tile, (b) across the q lanes, (c) across the mt
# tiles of one lane, (d) on the last real channel of a padded tile (K = 31)
TIE_K = 31
TIE_PAIRS = ((0, 1), (2, 6), (3, 19), (TIE_K - 2, TIE_K - 1))


def interleaved_min_tiles():
    """The smallest tile count that make_sched deals to the XCDs in interleaved chunks, read from the source."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "instance_nerf_amd", "csrc",
                            "field_fused.hip")).read()
    chunk = int(re.search(r"constexpr int kXcdChunkLog2 = (\d+);", src).group(1))
    m = re.search(r"const int64_t rounds = n_tiles >> \(kChunkLog2 \+ (\d+)\);\s*if \(rounds >= (\d+)\) \{", src)
    return int(m.group(2)) << (chunk + int(m.group(1)))


def cases():
    """[(NeRF table, (W, L, H), K)]: every table on the three main lattices with K rotating through KS, the small
    lattices on one table of each tier."""
    out, i = [], 0
    for t in TOL_TABLES + EXACT_TABLES:
        for dims in MAIN_LATTICES:
            out.append((t, dims, KS[i % len(KS)]))
            i += 1
    for t in ("bench", "x16"):
        for dims in SMALL_LATTICES:
            out.append((t, dims, KS[i % len(KS)]))
            i += 1
    return out


def case_id(case):
    t, d, K = case[:3]
    return f"{t}-{d[0]}x{d[1]}x{d[2]}-K{K}"


# ---------------------------------------------------------------------------- inputs
def axes(table, dims):
    """ax_w [W], ax_l [L], ax_h [H]: U(+-bound) (exact tier: x01 on multiples of 1/8); one value of ax_w and one of ax_h
    lie outside the bound and are clamped to the face."""
    bound = SETTINGS[table][0]
    rng = _rng("inst_lattice_axes", table, tuple(dims))
    b = F32(bound)
    if tier_of(table) == "exact":
        ax = [(rng.integers(0, 9, size=n).astype(F32) / F32(8) * (2 * b) - b).astype(F32) for n in dims]
    else:
        ax = [_u(rng, (n,), bound) for n in dims]
    if dims[0] > 4:
        ax[0][4] = F32(1.25) * b
    if dims[2] > 1:
        ax[2][1] = -F32(3.0) * b
    return ax


@functools.lru_cache(maxsize=None)
def inst_embeddings(table):
    """The instance table's values for the NeRF table ``table``: another draw than ``embeddings`` of either table."""
    t = table_for(INST_TABLE[table])
    rows = int(t["total_rows"])
    rng = _rng("inst_lattice_emb", table)
    if tier_of(table) == "tol":
        return _u(rng, (rows, 2), 1.0)
    return rng.integers(-2, 3, size=(rows, 2)).astype(F32)


def inst_weights(table, K, w2="plain"):
    """field_forward_reference.instance_weights of the instance table; w2 "neg": W2 = -|W2| and -1 on eight more columns per row (h2 >= 0: every
    logit <= 0, and where all of them are < 0 a zero padding channel would win); ("tie", a, b): rows a and b of W2 are the same row, +1 on every column either of
    them used (h2 >= 0: the pair is the maximum on many voxels, and the sums stay small integers)."""
    W = [w.copy() for w in instance_weights(INST_TABLE[table], K)]
    if w2 == "neg":
        W[2] = -np.abs(W[2])
        for r in range(K):                               # eight more columns per row: some voxels have no logit of 0
            W[2][r, (5 * r + 3 * np.arange(8)) % 64] = -1.0
    elif w2 != "plain":
        _, a, b = w2
        row = ((W[2][a] != 0) | (W[2][b] != 0)).astype(F32)
        W[2][a], W[2][b] = row, row
    return W


# ---------------------------------------------------------------------------- the per-voxel reference
def confidence(logits, cond):
    """-> (label, conf, cond_conf, device term, top-2 margin) of float64 logits [M, K]."""
    l = np.asarray(logits, F64)
    M, K = l.shape
    label = np.argmax(l, 1)                                  # the first maximum: the lowest channel on ties
    mx = l[np.arange(M), label]
    d = l - mx[:, None]
    e = np.exp(d)
    s = e.sum(1)
    conf = 1.0 / s
    p = e / s[:, None]
    cbest = np.asarray(cond, F64)[np.arange(M), label]
    cond_conf = conf * (p * (cond + cbest[:, None])).sum(1)
    dev = conf * (p * DEVICE_ULP * (1.0 + np.abs(d) * LOG2E)).sum(1)
    srt = np.sort(l, 1)
    margin = srt[:, -1] - srt[:, -2] if K > 1 else np.full(M, np.inf)
    return label, conf, cond_conf, dev, margin


def model_confidence(mod, logits):
    """The kernel's fp32 steps on a model's logits: d = l_c - max, __expf(d), the sum in channel order, 1 / s."""
    l = np.asarray(logits, F64)
    mx = l.max(1)
    e = mod.exp(mod.r(l - mx[:, None]))
    s = np.zeros(len(l))
    for c in range(l.shape[1]):
        s = mod.r(s + e[:, c])
    return mod.r(1.0 / s)


class LatticeRef:
    """Everything one (NeRF table, lattice, K) is compared with, on one arithmetic model (default float64)."""

    def __init__(self, table, dims, K, mod=None, variant="default", w2="plain", log=None):
        self.table, self.dims, self.K = table, tuple(int(v) for v in dims), int(K)
        self.mod = mod or Exact64(log)
        self.tier = tier_of(table)
        self.bound, self.ds = SETTINGS[table]
        self.N = int(np.prod(self.dims))
        self.ax = axes(table, self.dims)
        if variant == "default":
            variant = "logit" if self.tier == "exact" else None
        self.Wn = nerf_weights(table, variant)
        self.Wi = inst_weights(table, self.K, w2)
        x01, oob = x01_lattice(*self.ax, self.bound)
        assert not oob.any()
        enc, cenc = encode(self.mod, table_for(table), embeddings(table).astype(F64), x01, oob, log)
        o, c = sigma_part(self.mod, self.Wn, enc, cenc, self.ds)
        self.so0, self.cso0 = o["so"][:, 0], c["so"][:, 0]
        ienc, cienc = encode(self.mod, table_for(INST_TABLE[table]), inst_embeddings(table).astype(F64), x01, oob, log)
        o, c = instance_part(self.mod, self.Wi, ienc, cienc)
        self.logits, self.clogits = o["logits"], c["logits"]
        self.label, self.conf, self.cond_conf, self.dev, self.margin = confidence(self.logits, self.clogits)

    def occupied(self, sigma_thresh):
        """exp(so0) * density_scale >= the fp32 threshold the launch gets, in float64."""
        return np.exp(self.so0) * float(F32(self.ds)) >= float(F32(sigma_thresh))

    def band(self, build="bf16x3"):
        return 2.0 * TOL[build]["logits"] * self.clogits.max(1)

    def gap_need(self, mid, build="bf16x3"):
        cond_part = TOL[build]["logit"] * float(self.cso0.max()) if self.tier == "tol" else 0.0
        return 2.0 * (cond_part + DEVICE_ULP * (1.0 + abs(mid)))

    def threshold(self, q):
        """-> (sigma_thresh fp32, mid, gap): the widest gap between neighbouring logits around quantile q (tolerance
        tier: among the N / 20 neighbours on either side; exact tier: between the two distinct values next to the
        quantile of the distinct values)."""
        v = np.sort(np.unique(self.so0) if self.tier == "exact" else self.so0)
        if len(v) < 2:
            mid, gap = float(v[0]) - 1.0, 2.0
        else:
            k = int(q * (len(v) - 1))
            w = 0 if self.tier == "exact" else max(1, len(v) // 20)
            lo, hi = max(0, k - w), min(len(v) - 1, k + w + 1)
            g = np.diff(v[lo:hi + 1])
            i = int(np.argmax(g))
            mid, gap = 0.5 * float(v[lo + i] + v[lo + i + 1]), float(g[i])
        return F32(float(F32(self.ds)) * np.exp(mid)), mid, gap

    def tail_threshold(self, count=256):
        """-> (sigma_thresh, mid, gap, occupied voxels): among the ``count`` largest logits, the lowest gap that exceeds
        its need.  A lattice of 3e5 voxels has no such gap near a quantile (neighbouring logits lie 1e-4 apart, the need
        is 1e-2), only in its tails."""
        v = np.sort(self.so0)[-count:]
        for i in range(len(v) - 1):
            mid, gap = 0.5 * float(v[i] + v[i + 1]), float(v[i + 1] - v[i])
            if gap > 1.5 * self.gap_need(mid):
                return F32(float(F32(self.ds)) * np.exp(mid)), mid, gap, len(v) - 1 - i
        raise AssertionError("no usable gap")

    def thresholds(self):
        """{name: sigma_thresh}: the two quantiles, 0 (all occupied) and twice the largest sigma (none)."""
        top = F32(2.0 * float(F32(self.ds)) * np.exp(float(self.so0.max())))
        return {"q50": self.threshold(0.5)[0], "q90": self.threshold(0.9)[0], "zero": F32(0.0), "above": top}

    def expected(self, sigma_thresh):
        """-> (occ, labels uint8 [N], conf float64 [N]) as the launch writes them."""
        occ = self.occupied(sigma_thresh)
        return occ, np.where(occ, self.label, LABEL_EMPTY).astype(np.uint8), np.where(occ, self.conf, 0.0)


@functools.lru_cache(maxsize=4)
def reference(table, dims, K, variant="default", w2="plain"):
    return LatticeRef(table, dims, K, variant=variant, w2=w2)


@functools.lru_cache(maxsize=1)
def big_reference():
    return LatticeRef(*BIG_CASE)


def tiles(dims, occ):
    """The kernel's runs of 16 along W -> (n_valid [rows, Wp / 16], n_occupied [rows, Wp / 16]), rows = (il, ih)."""
    W, L, H = dims
    Wp = (W + 15) // 16 * 16
    o = np.zeros((Wp, L * H), np.int64)
    o[:W] = np.asarray(occ).reshape(W, L * H)
    v = np.zeros((Wp, L * H), np.int64)
    v[:W] = 1
    return v.reshape(Wp // 16, 16, L * H).sum(1).T, o.reshape(Wp // 16, 16, L * H).sum(1).T


def tile_kinds(dims, occ):
    """-> dict(empty, mixed, full: tile counts; tail_empty: rows whose padded tail tile has no occupied voxel, or None
    when W is a multiple of 16)."""
    nv, no = tiles(dims, occ)
    out = dict(empty=int((no == 0).sum()), full=int((no == nv).sum()), mixed=int(((no > 0) & (no < nv)).sum()))
    out["tail_empty"] = int((no[:, -1] == 0).sum()) if dims[0] % 16 else None
    return out


def compare(ref, sigma_thresh, labels, conf, logit, build, ratios=None):
    """One launch against ``ref`` -> list of failures.  labels uint8 [N], conf fp32 [N], logit fp32 [N] or None."""
    fails, tier, N = [], ref.tier, ref.N
    ratios = {} if ratios is None else ratios
    labels, conf = np.asarray(labels).reshape(-1), np.asarray(conf, F32).reshape(-1)
    occ_r, lab_r, conf_r = ref.expected(sigma_thresh)
    if logit is not None:
        lg = np.asarray(logit, F32).reshape(-1)
        if tier == "exact":
            want = (ref.so0 + 0.0).astype(F32)
            n = int((lg.view(np.uint32) != want.view(np.uint32)).sum())
            if n:
                fails.append(f"density_logit: {n} of {N} differ in their bits")
        else:
            r = B.worst_ratio(lg, ref.so0, ref.cso0)
            ratios["logit"] = max(ratios.get("logit", 0.0), r / TOL[build]["logit"])
            if not r <= TOL[build]["logit"]:
                fails.append(f"density_logit: {r:.3e} > {TOL[build]['logit']:.3e}")
    occ = labels != LABEL_EMPTY
    if not np.array_equal(occ, occ_r):
        fails.append(f"occupancy differs on {int((occ != occ_r).sum())} of {N} voxels, first {int(np.flatnonzero(occ != occ_r)[0])}")
        return fails
    if (labels[occ] >= ref.K).any():
        fails.append(f"a label >= K = {ref.K}: {int(labels[occ].max())}")
    if (conf[~occ].view(np.uint32) != 0).any():
        fails.append("confidence of an unoccupied voxel is not +0")
    if tier == "exact":
        bad = labels != lab_r
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            fails.append(f"labels differ on {int(bad.sum())} voxels, first {i}: {int(labels[i])} != {int(lab_r[i])}")
        tol = ref.dev
        if ref.K == 1 and not (conf[occ] == 1.0).all():
            fails.append("K = 1: confidence is not exactly 1")
    else:
        band = ref.band(build)
        sure = occ & (ref.margin > band)
        bad = sure & (labels != lab_r)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            fails.append(f"labels differ on {int(bad.sum())} voxels off the band, first {i}: {int(labels[i])} != {int(lab_r[i])}")
        inb = np.flatnonzero(occ & ~sure & (labels < ref.K))
        got_l = ref.logits[inb, labels[inb].astype(np.int64)]
        far = ref.logits[inb].max(1) - got_l > band[inb]
        if far.any():
            fails.append(f"{int(far.sum())} labels inside the band name a channel beyond the band of the maximum")
        tol = TOL[build]["conf"] * ref.cond_conf + ref.dev
    err = np.abs(conf.astype(F64) - conf_r)[occ]
    if occ.any():
        if not np.isfinite(conf[occ]).all():
            fails.append("confidence not finite")
        else:
            r = float((err / tol[occ]).max())
            key = "conf" if tier == "tol" else "conf_exact"
            ratios[key] = max(ratios.get(key, 0.0), r)
            if not r <= 1.0:
                i = int(np.flatnonzero(occ)[int(np.argmax(err / tol[occ]))])
                fails.append(f"confidence: |got - ref| = {r:.3f} x its tolerance at voxel {i} ({conf[i]!r} against {conf_r[i]!r})")
    return fails


def measure_conf(build, case_list=None):
    """Largest |model confidence - float64| / cond_conf of ``build``'s model over the tolerance-tier cases."""
    worst = 0.0
    for table, dims, K in case_list or [c for c in cases() if tier_of(c[0]) == "tol"]:
        ref = reference(table, dims, K)
        m = LatticeRef(table, dims, K, mod=R.model_for(build, "")[0])
        worst = max(worst, B.worst_ratio(model_confidence(m.mod, m.logits), ref.conf, ref.cond_conf))
    return worst


# ---------------------------------------------------------------------------- statistics, bit for bit
STATS_THREADS, STATS_MAX_BLOCKS, STATS_GROUPS = 256, 512, 8


def stats_blocks(N):
    n_blocks = max(1, min(STATS_MAX_BLOCKS, -(-N // 1024)))
    return n_blocks, -(-N // n_blocks)


def stats_reference(labels, conf, K):
    """labels uint8 [W, L, H], conf fp32 [W, L, H] -> (counts int64 [K], boxes int64 [K, 6], conf_sum fp32 [K]) with
    conf_sum in the launch's order (module text)."""
    W, L, H = labels.shape
    N = W * L * H
    lab, cf = np.asarray(labels).reshape(-1).astype(np.int64), np.asarray(conf, F32).reshape(-1)
    counts, boxes = np.zeros(K, np.int64), np.full((K, 6), -1, np.int64)
    iw, il, ih = np.unravel_index(np.arange(N), (W, L, H)) if N else (np.zeros(0, np.int64),) * 3
    for c in range(K):
        m = lab == c
        counts[c] = int(m.sum())
        if counts[c]:
            boxes[c] = [iw[m].min(), il[m].min(), ih[m].min(), iw[m].max(), il[m].max(), ih[m].max()]
    nb, per = stats_blocks(N)
    ni = max(1, -(-per // STATS_THREADS))
    b, w, i, lane = np.meshgrid(np.arange(nb), np.arange(4), np.arange(ni), np.arange(64), indexing="ij")
    v = b * per + w * 64 + i * STATS_THREADS + lane
    hi = np.minimum(N, (b + 1) * per)
    valid = v < hi
    v = np.where(valid, v, 0)
    lv = np.where(valid, lab[v] if N else 0, LABEL_EMPTY)
    cv = np.where(valid, cf[v] if N else F32(0), F32(0)).astype(F32)
    idx = np.arange(64)
    sums = np.zeros(K, F32)
    for c in range(K):
        x = np.where(lv == c, cv, F32(0)).astype(F32)
        for off in (32, 16, 8, 4, 2, 1):
            x = (x + x[..., idx ^ off]).astype(F32)
        chunk = x[..., 0]                                    # [nb, 4, ni]: lane 0 of every chunk
        wave = np.zeros((nb, 4), F32)
        for k in range(ni):
            wave = (wave + chunk[:, :, k]).astype(F32)
        blk = np.zeros(nb, F32)
        for ww in range(4):
            blk = (blk + wave[:, ww]).astype(F32)
        grp = np.zeros(STATS_GROUPS, F32)
        for g in range(STATS_GROUPS):
            for bb in range(g, nb, STATS_GROUPS):
                grp[g] = F32(grp[g] + blk[bb])
        tot = grp[0]
        for g in range(1, STATS_GROUPS):
            tot = F32(tot + grp[g])
        sums[c] = tot
    return counts, boxes, sums


def stats_inputs(name):
    """-> (labels uint8 [W, L, H], conf fp32 [W, L, H], K) of the statistics cases."""
    rng = _rng("inst_stats", name)
    sizes = {"n0": (0, 3, 5), "n1": (1, 1, 1), "n63": (1, 7, 9), "n64": (4, 2, 8), "n65": (1, 5, 13), "n1023": (3, 11, 31),
             "n1024": (8, 4, 32), "n1025": (1, 25, 41)}
    if name in sizes:
        dims, K = sizes[name], 5
    elif name.startswith("cap"):                         # 512 workgroups, per_block 1032: no multiple of 64
        dims, K = (65, 64, 127), {"cap1": 1, "cap5": 5, "cap64": 64}[name]
    else:
        dims, K = (9, 17, 23), {"empty": 5, "ignored": 5, "corners": 5, "spread": 64}[name]
    N = int(np.prod(dims))
    lab = rng.integers(0, K + max(1, K // 4), size=dims).astype(np.uint8)
    lab[lab >= K] = LABEL_EMPTY
    conf = rng.random(dims, dtype=F32)
    if name == "empty":
        lab[:] = LABEL_EMPTY
    elif name == "ignored":                              # labels K .. 254 carry confidences and must not be counted
        sel = rng.random(dims) < 0.3
        lab[sel] = rng.integers(K, 255, size=int(sel.sum())).astype(np.uint8)
        lab.reshape(-1)[:250] = np.arange(K, K + 250).astype(np.uint8)
    elif name == "corners":                              # channel 3 at the two opposite corners only
        lab[lab == 3] = 0
        lab[0, 0, 0] = lab[-1, -1, -1] = 3
    elif name in ("spread", "cap5"):                     # exponents 2^-12 .. 2^12: the summation order shows in the bits
        conf = (conf * np.exp2(rng.integers(-12, 13, size=dims)).astype(F32)).astype(F32)
    if name != "ignored":
        conf[lab == LABEL_EMPTY] = F32(0)
    return lab, conf, K


STATS_CASES = ("n0", "n1", "n63", "n64", "n65", "n1023", "n1024", "n1025", "cap1", "cap5", "cap64", "empty", "ignored",
               "corners", "spread")
