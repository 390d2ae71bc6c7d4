"""Executable statement of the detector tail's arithmetic (include/inr.h, "Detector tail") in numpy fp32: the mask paste
and the greedy per-class NMS.  Every operation is a numpy fp32 operation of its own (numpy never fuses a multiply and an
add), so the results are the bits the HIP kernels must produce.  tests/golden/make_detections_golden.py asserts that
``paste_soft`` equals the reference's own ``_do_paste_mask(skip_empty=False)`` bit for bit."""
import numpy as np

f = np.float32


def box_is_live(b):
    """The departure from the reference: a box with a non-finite coordinate or a side <= 0 pastes nothing."""
    b = np.asarray(b, f)
    return bool(np.all(np.isfinite(b)) and b[3] - b[0] > 0 and b[4] - b[1] > 0 and b[5] - b[2] > 0)


def coord(size, lo, hi, M):
    """Voxel indices 0..size-1 -> sample positions in texel units."""
    with np.errstate(all="ignore"):
        g = (np.arange(size, dtype=f) - f(lo)) / (f(hi) - f(lo)) * f(2) - f(1)
        return ((g + f(1)) / f(2)) * f(M - 1)


def paste_soft(masks, boxes, shape):
    """masks fp32 [N, M, M, M], boxes fp32 [N, 6], shape (W, L, H) -> fp32 [N, W, L, H]: per mask, eight whole-volume
    taps in torch's order, weight = (h-factor * l-factor) * w-factor, acc = acc + value * weight, zeros padding."""
    masks, boxes = np.asarray(masks, f), np.asarray(boxes, f).reshape(-1, 6)
    W, L, H = (int(v) for v in shape)
    N = masks.shape[0]
    M = masks.shape[1] if N else 1
    out = np.zeros((N, W, L, H), f)
    for n in range(N):
        b = boxes[n]
        if not box_is_live(b):
            continue
        pw, pl, ph = np.meshgrid(coord(W, b[0], b[3], M), coord(L, b[1], b[4], M), coord(H, b[2], b[5], M), indexing="ij")
        with np.errstate(all="ignore"):
            w0, l0, h0 = np.floor(pw), np.floor(pl), np.floor(ph)
            w1, l1, h1 = w0 + f(1), l0 + f(1), h0 + f(1)
            fw, fl, fh = (w1 - pw, pw - w0), (l1 - pl, pl - l0), (h1 - ph, ph - h0)
        iw, il, ih = (w0, w1), (l0, l1), (h0, h1)
        acc = np.zeros((W, L, H), f)
        for t in range(8):
            a, bb, c = t >> 2, (t >> 1) & 1, t & 1
            ok = ((iw[a] >= 0) & (iw[a] < M) & (il[bb] >= 0) & (il[bb] < M) & (ih[c] >= 0) & (ih[c] < M))
            zi, yi, xi = (np.where(ok, v, 0).astype(np.int64) for v in (iw[a], il[bb], ih[c]))
            with np.errstate(all="ignore"):
                weight = ((fh[c] * fl[bb]).astype(f) * fw[a]).astype(f)
                term = (masks[n][zi, yi, xi] * weight).astype(f)
                acc = np.where(ok, (acc + term).astype(f), acc)
        out[n] = acc
    return out


def paste_bits(masks, boxes, shape, threshold=0.5):
    return paste_soft(masks, boxes, shape) >= f(threshold)


def pack_planes(bits):
    """bool [N, W, L, H] -> uint64 [N, ceil(V / 64)]: bit v % 64 of word v / 64, tail bits zero."""
    N = bits.shape[0]
    V = int(np.prod(bits.shape[1:]))
    nW = (V + 63) // 64
    flat = np.zeros((N, nW * 64), np.uint8)
    flat[:, :V] = bits.reshape(N, V)
    return np.packbits(flat.reshape(N, nW, 64), axis=2, bitorder="little").view(np.uint64).reshape(N, nW)


def support(box, M):
    """The voxel range along each axis outside which a pasted mask is exactly zero: the box widened by one texel on each
    side, rounded outward (fp64 from the fp32 box).  -> (lo [3], hi [3]): voxels i < lo or i > hi hold 0.  M = 1: the one
    texel covers everything."""
    b = np.asarray(box, f).astype(np.float64)
    if M == 1:
        return np.full(3, -np.inf), np.full(3, np.inf)
    t = (b[3:] - b[:3]) / (M - 1)
    return np.floor(b[:3] - t), np.ceil(b[3:] + t)


def box_iou(a, b):
    """fp32 IoU of one box against boxes [m, 6]: the reference's axis-aligned arithmetic (model/utils.py:391-462)."""
    a, b = np.asarray(a, f), np.asarray(b, f).reshape(-1, 6)
    with np.errstate(all="ignore"):
        va = ((a[3] - a[0]) * (a[4] - a[1])).astype(f) * (a[5] - a[2])
        vb = ((b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1])).astype(f) * (b[:, 5] - b[:, 2])
        ext = np.minimum(a[3:], b[:, 3:]) - np.maximum(a[:3], b[:, :3])
        ext = np.where(ext < 0, f(0), ext).astype(f)
        overlap = ((ext[:, 0] * ext[:, 1]).astype(f) * ext[:, 2]).astype(f)
        return (overlap / ((va + vb).astype(f) - overlap).astype(f)).astype(f)


def batched_nms(boxes, scores, idxs, iou_threshold):
    """Greedy per-class NMS -> int64 indices in decreasing score order (a stable sort: ties go to the lower index)."""
    boxes, scores, idxs = np.asarray(boxes, f).reshape(-1, 6), np.asarray(scores, f), np.asarray(idxs)
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    b, c = boxes[order], idxs[order]
    removed = np.zeros(len(order), bool)
    keep = []
    for i in range(len(order)):
        if removed[i]:
            continue
        keep.append(order[i])
        if i + 1 < len(order):
            iou = box_iou(b[i], b[i + 1:])
            removed[i + 1:] |= ~(iou <= f(iou_threshold)) & (c[i + 1:] == c[i])
    return np.asarray(keep, np.int64)
