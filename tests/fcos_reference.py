"""Restatement of the FCOS target rule and loss terms of include/inr.h ("FCOS training targets and losses").

``targets``: numpy float32, one operation at a time - the rule the kernel, the composable path of
instance_nerf_amd/fcos.py and the reference's own prepare_targets (tests/golden/make_fcos_golden.py asserts it bit for bit)
all follow.  ``loss_terms`` / ``losses``: float64, evaluated on the float32 inputs, written once for numpy and torch (the
torch form is what float64 autograd differentiates; torch.minimum / maximum send half the gradient to each side of a tie)."""
import numpy as np

f32 = np.float32
INF = f32(100000000)
SIZES_OF_INTEREST = ((-1, 16), (16, 32), (32, 64), (64, 100000000))
ALPHA = 0.25


def same(a, b):
    """Bit for bit, a NaN for a NaN (payloads are not part of the rule)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def locations(shapes, strides):
    out = []
    for (w, l, h), s in zip(shapes, strides):
        x, y, z = np.meshgrid(*[np.arange(n, dtype=np.int64) * s + s // 2 for n in (w, l, h)], indexing="ij")
        out.append(np.stack((x.reshape(-1), y.reshape(-1), z.reshape(-1)), 1).astype(f32))
    return out


def centerness(t):
    with np.errstate(all="ignore"):
        a = np.minimum(t[:, 0], t[:, 3]) / np.maximum(t[:, 0], t[:, 3])
        b = np.minimum(t[:, 1], t[:, 4]) / np.maximum(t[:, 1], t[:, 4])
        c = np.minimum(t[:, 2], t[:, 5]) / np.maximum(t[:, 2], t[:, 5])
        return np.sqrt((a * b) * c)


def scene_targets(loc, stride, lo, hi, g, radius, norm):
    """One level of one scene: loc [P, 3], g [G, 6] -> labels, reg targets, matched, ties (locations whose smallest volume
    is attained by more than one box), on_face (locations with a zero distance to a box)."""
    P = len(loc)
    if len(g) == 0:
        return np.zeros(P, f32), np.zeros((P, 6), f32), np.zeros(P, np.int32), np.zeros(P, bool), np.zeros(P, bool)
    with np.errstate(all="ignore"):
        reg = np.concatenate((loc[:, None, :] - g[None, :, :3], g[None, :, 3:] - loc[:, None, :]), 2)      # [P, G, 6]
        if radius > 0:
            s = f32(stride * radius)
            c = (g[:, :3] + g[:, 3:]) / f32(2)
            cm, cp = c - s, c + s
            rlo = np.where(cm > g[:, :3], cm, g[:, :3])
            rhi = np.where(cp > g[:, 3:], g[:, 3:], cp)
            dist = np.concatenate((loc[:, None, :] - rlo[None], rhi[None] - loc[:, None, :]), 2)
            inside = dist.min(2) > 0                                   # np.min keeps a NaN, as torch.min does
        else:
            inside = reg.min(2) > 0
        largest = reg.max(2)
        cared = (largest >= f32(lo)) & (largest <= f32(hi))
        volume = ((g[:, 3] - g[:, 0]) * (g[:, 4] - g[:, 1])) * (g[:, 5] - g[:, 2])
        area = np.where(inside & cared, volume[None, :], INF).astype(f32)
        matched = np.argmin(area, 1)                                   # the first NaN, else the first minimum
        best = area[np.arange(P), matched]
        labels = (best != INF).astype(f32)
        t = reg[np.arange(P), matched]
        if norm:
            t = t / f32(stride)
        ties = ((area == best[:, None]).sum(1) > 1) & (best != INF)
        on_face = (reg == 0).any((1, 2))
    return labels, t.astype(f32), matched.astype(np.int32), ties, on_face


def targets(shapes, strides, gts, radius=1.5, norm=True, ranges=None, ori_sizes=None):
    """-> dict of level-first arrays: labels f32 [T], reg f32 [T, 6], centerness f32 [T], matched i32 [T], valid bool [T]
    (None without ori_sizes), plus ties / on_face / level (bookkeeping of the fixture generator)."""
    ranges = ranges if ranges is not None else SIZES_OF_INTEREST[:len(shapes)]
    out = {k: [] for k in ("labels", "reg", "matched", "ties", "on_face", "valid", "level")}
    for l, loc in enumerate(locations(shapes, strides)):
        for b, g in enumerate(gts):
            lab, t, m, ties, face = scene_targets(loc, strides[l], ranges[l][0], ranges[l][1], np.asarray(g, f32).reshape(-1, 6),
                                                  radius, norm)
            for k, v in (("labels", lab), ("reg", t), ("matched", m), ("ties", ties), ("on_face", face)):
                out[k].append(v)
            out["level"].append(np.full(len(loc), l, np.int32))
            if ori_sizes is not None:
                o = [f32(v) for v in ori_sizes[b]]
                out["valid"].append((loc[:, 0] < o[0]) & (loc[:, 1] < o[1]) & (loc[:, 2] < o[2]))
    res = {k: np.concatenate(v) for k, v in out.items() if v}
    res["valid"] = res.get("valid")
    with np.errstate(all="ignore"):
        res["centerness"] = np.where(res["labels"] > 0, centerness(res["reg"]), f32(0)).astype(f32)
    return res


# ---- losses, float64 ---------------------------------------------------------------------------------------------------
def flatten(xp, box_cls, box_reg, ctr):
    """The head's per-level tensors [B,1,W,L,H], [B,6,W,L,H], [B,1,W,L,H] -> level-first cls [T], reg [T, 6], ctr [T]."""
    if xp is np:
        cat, perm = np.concatenate, lambda r: np.transpose(r, (0, 2, 3, 4, 1))
    else:
        cat, perm = xp.cat, lambda r: r.permute(0, 2, 3, 4, 1)
    return (cat([c.reshape(-1) for c in box_cls]), cat([perm(r).reshape(-1, 6) for r in box_reg]),
            cat([c.reshape(-1) for c in ctr]))


def _bce(xp, x, t):
    return xp.maximum(x, 0 * x) - x * t + xp.log1p(xp.exp(-xp.abs(x)))


def loss_terms(xp, cls, reg, ctr, labels, regt, valid, loss_type):
    """Per-location terms in the arrays' own precision (pass float64): focal, regterm, bce, pos, cw.  ``xp``: numpy or
    torch.  Rows that are not positive enter the IoU and BCE formulas as ones and come out as 0."""
    one, zero = 0 * cls + 1, 0 * cls
    valid = (labels == labels) if valid is None else valid
    pos = valid & (labels > 0)
    x = xp.where(valid, cls, zero)
    p = 1 / (1 + xp.exp(-x))
    ce = _bce(xp, x, labels)
    p_t = p * labels + (1 - p) * (1 - labels)
    focal = xp.where(valid, (ALPHA * labels + (1 - ALPHA) * (1 - labels)) * (ce * (1 - p_t) ** 2), zero)
    t = xp.where(pos[:, None], regt, 0 * regt + 1)
    q = xp.where(pos[:, None], reg, 0 * reg + 1)
    cw = xp.sqrt((xp.minimum(t[:, 0], t[:, 3]) / xp.maximum(t[:, 0], t[:, 3])) *
                 (xp.minimum(t[:, 1], t[:, 4]) / xp.maximum(t[:, 1], t[:, 4])) *
                 (xp.minimum(t[:, 2], t[:, 5]) / xp.maximum(t[:, 2], t[:, 5])))
    cw = xp.where(pos, cw, zero)
    tv = (t[:, 0] + t[:, 3]) * (t[:, 1] + t[:, 4]) * (t[:, 2] + t[:, 5])
    pv = (q[:, 0] + q[:, 3]) * (q[:, 1] + q[:, 4]) * (q[:, 2] + q[:, 5])
    inter, enclose = one, one
    for a in range(3):
        inter = inter * (xp.minimum(q[:, a], t[:, a]) + xp.minimum(q[:, a + 3], t[:, a + 3]))
        enclose = enclose * (xp.maximum(q[:, a], t[:, a]) + xp.maximum(q[:, a + 3], t[:, a + 3]))
    ac = enclose + 1e-7
    union = tv + pv - inter
    iou = (inter + 1) / (union + 1)
    if loss_type == "iou":
        l = -xp.log(iou)
    elif loss_type == "linear_iou":
        l = 1 - iou
    else:
        assert loss_type == "giou"
        l = 1 - (iou - (ac - union) / ac)
    regterm = xp.where(pos, l * cw, zero)
    bce = xp.where(pos, _bce(xp, xp.where(pos, ctr, zero), cw), zero)
    return focal, regterm, bce, pos, cw


def losses(xp, terms, norms=None):
    """(cls, reg, ctr) from the terms; ``norms`` = (n_pos, sum cw) replaces the case's own normalisers (world_size > 1)."""
    focal, regterm, bce, pos, cw = terms
    n_local = pos.sum()
    n, sc = (n_local + 0.0, cw.sum()) if norms is None else norms
    n1 = n if float(n) > 1 else 1.0
    if int(n_local) == 0:
        return focal.sum() / n1, 0 * focal.sum(), 0 * focal.sum()
    return focal.sum() / n1, regterm.sum() / sc, bce.sum() / n1


def ulp(x):
    """The spacing of float32 at |x| (at least that of the smallest normal number)."""
    return float(np.spacing(np.maximum(np.abs(np.asarray(x, f32)), np.finfo(f32).tiny)).max())
