"""The rule of include/inr.h, "Detector training targets", restated in numpy: the fp32 IoU in the reference's operation
order, the Matcher with torch's CPU arg-max and NaN rules, the labels and the box coder.  Everything is float32 arithmetic
one operation at a time (numpy never contracts), so on NaN-free inputs it gives the reference's bits; a NaN is a NaN
(payloads and signs of NaNs differ between processors and are not part of the rule).

The coder's size terms are logs.  ``size_quotients`` returns their exact fp32 arguments; ``encode(..., log=)`` takes the
log to apply: ``log_torch`` (torch's fp32 log on the CPU: what the reference's own run used, so the fixture compares bit
for bit) or ``log_f64`` (float64 log rounded to fp32: the yardstick for a GPU's logf)."""
import numpy as np

f = np.float32


def iou_matrix(gt, boxes, valid=None):
    """fp32 [G, A]; masked columns are -1."""
    gt, boxes = np.asarray(gt, f), np.asarray(boxes, f)
    with np.errstate(all="ignore"):
        def volume(b):
            return ((b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1])) * (b[:, 5] - b[:, 2])
        lo = np.maximum(gt[:, None, :3], boxes[None, :, :3])          # np.maximum / np.minimum keep a NaN operand
        hi = np.minimum(gt[:, None, 3:], boxes[None, :, 3:])
        ext = hi - lo
        ext = np.where(ext < 0, f(0), ext)                            # clamp(min=0): NaN stays NaN
        inter = (ext[..., 0] * ext[..., 1]) * ext[..., 2]
        q = inter / ((volume(gt)[:, None] + volume(boxes)[None, :]) - inter)
    assert q.dtype == f
    if valid is not None:
        q[:, ~np.asarray(valid, bool)] = f(-1)
    return q


def max_nan(q, axis):
    """(values, lowest index of the maximum) along ``axis`` with a NaN above every number, the first NaN winning."""
    nan = np.isnan(q)
    arg = np.where(nan.any(axis), nan.argmax(axis), np.where(nan, -np.inf, q).argmax(axis))
    return np.take_along_axis(q, np.expand_dims(arg, axis), axis).squeeze(axis), arg


def matcher(q, high, low, allow):
    """-> (matched int64 [A], best fp32 [A]).  Thresholds are compared as fp32."""
    best, arg = max_nan(q, 0)
    with np.errstate(invalid="ignore"):
        m = arg.astype(np.int64)
        m[best < f(low)] = -1
        m[(best >= f(low)) & (best < f(high))] = -2
        if allow:
            row_max, _ = max_nan(q, 1)
            restore = (q == row_max[:, None]).any(0)                  # never true for a NaN
            m[restore] = arg[restore]
    return m, best


def size_quotients(matched_boxes, boxes):
    """fp32 [A, 3]: w_gt / w_box per axis, the arguments of the coder's logs."""
    r, p = np.asarray(matched_boxes, f), np.asarray(boxes, f)
    with np.errstate(all="ignore"):
        return (r[:, 3:] - r[:, :3]) / (p[:, 3:] - p[:, :3])


def log_torch(x):
    import torch
    return torch.log(torch.from_numpy(np.ascontiguousarray(x, f))).numpy()


def log_f64(x):
    with np.errstate(all="ignore"):
        return np.log(np.asarray(x, np.float64)).astype(f)


def encode(matched_boxes, boxes, log=log_torch):
    """fp32 [A, 6]: encode_boxes_3d(matched_boxes, boxes)."""
    r, p = np.asarray(matched_boxes, f), np.asarray(boxes, f)
    with np.errstate(all="ignore"):
        ex = p[:, 3:] - p[:, :3]
        ectr = p[:, :3] + f(0.5) * ex
        gx = r[:, 3:] - r[:, :3]
        gctr = r[:, :3] + f(0.5) * gx
        out = np.concatenate([(gctr - ectr) / ex, log(gx / ex)], 1)
    assert out.dtype == f
    return out


def assign(gt, boxes, valid=None, gt_labels=None, high=0.35, low=0.2, allow=True, log=log_torch):
    """Everything inr_box_match_assign writes -> dict(matched int64, labels int64, best_iou, matched_boxes, targets,
    gt_max fp32 [G])."""
    gt, boxes = np.asarray(gt, f), np.asarray(boxes, f)
    q = iou_matrix(gt, boxes, valid)
    m, best = matcher(q, high, low, allow)
    if gt_labels is not None:
        labels = np.asarray(gt_labels, np.int64)[np.maximum(m, 0)]
    else:
        labels = np.ones(len(m), np.int64)
    labels[m == -1] = 0
    labels[m == -2] = -1
    if valid is not None:
        labels[~np.asarray(valid, bool)] = -1
    mb = gt[np.maximum(m, 0)]
    return dict(matched=m, labels=labels, best_iou=best, matched_boxes=mb, targets=encode(mb, boxes, log),
                gt_max=max_nan(q, 1)[0])


def float_key(v):
    """The order-preserving uint32 key of include/inr.h for fp32 values."""
    v = np.asarray(v, f)
    u = v.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(v), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def same(a, b):
    """Same shape, dtype and bits, a NaN matching any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    bits = a.view(np.uint32) == b.view(np.uint32)
    return bool(np.array_equal(nan, np.isnan(b)) and bits[~nan].all())


def ulps(a, b):
    """Distance in fp32 units in the last place between finite arrays of one sign pattern (|a| and |b| as ordered ints)."""
    a, b = np.asarray(a, f), np.asarray(b, f)

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))
