"""A numpy restatement of the confusion-matrix contract (include/inr.h, "Segmentation confusion matrix of rendered
instance maps") and of metrics.segmentation_scores, written without looking at either implementation's structure: a plain
loop over pixels for the matrix, the arg-max rule spelled out comparison by comparison, the scores in float64."""
import math

import numpy as np


def argmax_rule(row):
    """Lowest index of the maximum; NaN is above every number, the first NaN wins; equal numbers (-0.0 and +0.0) tie."""
    best, arg = row[0], 0
    for c in range(1, len(row)):
        v = row[c]
        if math.isnan(best):
            break
        if math.isnan(v) or v > best:
            best, arg = v, c
    return arg


def argmax_logits(logits, K):
    """[..., ld] -> [...] int64: the rule over the first K channels only."""
    flat = np.asarray(logits, dtype=np.float64).reshape(-1, logits.shape[-1])
    return np.array([argmax_rule(r[:K]) for r in flat], dtype=np.int64).reshape(logits.shape[:-1])


def argmax_logits_np(logits, K):
    """The same rule in whole-array numpy, for inputs too large for the loop: the first NaN of a row that has one, else
    the first index that equals the row's maximum.  (The tests hold it to ``argmax_logits`` on the special rows.)"""
    x = np.asarray(logits)[..., :K]
    nan = np.isnan(x)
    has_nan = nan.any(-1)
    top = np.max(np.where(nan, -np.inf, x), axis=-1, keepdims=True)
    return np.where(has_nan, nan.argmax(-1), (x == top).argmax(-1)).astype(np.int64)


def confusion_np(pred, truth, K):
    """``confusion`` with np.add.at, for inputs too large for the loop."""
    pred, truth = np.asarray(pred).astype(np.int64), np.asarray(truth).astype(np.int64)
    B = truth.shape[0]
    counts, ignored = np.zeros((B, K, K + 1), np.int64), np.zeros((B,), np.int64)
    image = np.broadcast_to(np.arange(B)[:, None], truth.shape)
    keep = (truth >= 0) & (truth < K)
    col = np.where((pred >= 0) & (pred < K), pred, K)
    np.add.at(counts, (image[keep], truth[keep], col[keep]), 1)
    np.add.at(ignored, image[~keep], 1)
    return counts, ignored


def confusion(pred, truth, K):
    """pred, truth integer [B, N] -> (counts int64 [B, K, K+1], ignored int64 [B])."""
    pred, truth = np.asarray(pred).astype(np.int64), np.asarray(truth).astype(np.int64)
    B, N = truth.shape
    counts, ignored = np.zeros((B, K, K + 1), np.int64), np.zeros((B,), np.int64)
    for b in range(B):
        for n in range(N):
            t, p = int(truth[b, n]), int(pred[b, n])
            if t < 0 or t >= K:
                ignored[b] += 1
            elif p < 0 or p >= K:
                counts[b, t, K] += 1
            else:
                counts[b, t, p] += 1
    return counts, ignored


def scores(counts, stuff_ids=(0,), match="id"):
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim == 3:
        c = c.sum(0)
    K = c.shape[0]
    T = [int(c[g, :].sum()) for g in range(K)]
    P = [int(c[:, p].sum()) for p in range(K)]
    I = [int(c[k, k]) for k in range(K)]
    U = [T[k] + P[k] - I[k] for k in range(K)]
    iou = [I[k] / U[k] if U[k] > 0 else float("nan") for k in range(K)]
    gt = [iou[k] for k in range(K) if T[k] > 0]
    al = [iou[k] for k in range(K) if U[k] > 0]
    out = {"iou": np.array(iou), "miou_gt_ids": sum(gt) / len(gt) if gt else 0.0,
           "miou_all_ids": sum(al) / len(al) if al else 0.0, "pixel_acc": sum(I) / sum(T) if sum(T) else 0.0}
    stuff = set(stuff_ids)
    matches = [-1] * K
    pair_iou = {}
    for g in range(K):
        for p in range(K):
            if T[g] == 0 or P[p] == 0:
                continue
            if match == "id" and g != p:
                continue
            if match == "any" and g != p and (g in stuff or p in stuff):
                continue
            v = int(c[g, p]) / (T[g] + P[p] - int(c[g, p]))
            if v > 0.5:
                assert matches[g] == -1
                matches[g], pair_iou[g] = p, v

    def pq(things_only):
        gs = [g for g in range(K) if T[g] > 0 and not (things_only and g in stuff)]
        ps = [p for p in range(K) if P[p] > 0 and not (things_only and p in stuff)]
        tp = [g for g in gs if matches[g] >= 0]
        fn, fp = len(gs) - len(tp), len(ps) - len(tp)
        s, den = sum(pair_iou[g] for g in tp), len(tp) + fp / 2 + fn / 2
        return (s / den if den else 0.0, s / len(tp) if tp else 0.0, len(tp) / den if den else 0.0, len(tp), fp, fn)

    out["pq"], out["sq"], out["rq"], out["tp"], out["fp"], out["fn"] = pq(False)
    out["pq_things"], out["sq_things"], out["rq_things"] = pq(True)[:3]
    out["matches"] = np.array(matches, dtype=np.int64)
    return out
