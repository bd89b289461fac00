"""TEST INFRASTRUCTURE -- the numpy specification of evaluation.score_order, ranking_curve and ranking_metrics (the kernels of
csrc/mtadgat_curves.hip).  Vectorised: a stable argsort on the order key, cumsum, np.unique; the average-precision sum is an exact
math.fsum, AUROC is a quotient of Python ints, and the F1 arg-max is numpy float64 with the expression of
evaluation._scores_from_counts.  tests/test_host_curves.py holds it against scikit-learn, oracle.eval_oracle.point_adjust and a
direct per-threshold PA%K loop."""
import math

import numpy as np


def order_key(x, descending=True):
    """uint32 keys whose ascending order is the rank order: -0.0 = +0.0, the sign bit flipped for non-negative values and all bits
    for negative ones, inverted for descending order, every NaN 0xffffffff."""
    x = np.asarray(x, dtype=np.float32)
    x = np.where(x == 0, np.float32(0), x).astype(np.float32)
    u = np.ascontiguousarray(x).view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    if descending:
        k = ~k
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def score_order(x, descending=True):
    return np.argsort(order_key(x, descending), kind="stable").astype(np.int64)


def labels_bool(labels):
    labels = np.asarray(labels)
    return labels if labels.dtype == np.bool_ else labels > 0.1


def segments(lab):
    """[start, end) of the runs of set labels."""
    d = np.diff(np.concatenate(([0], lab.astype(np.int8), [0])))
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1)


def adjusted_scores(scores, labels, adjust=None):
    """The float32 array that is ranked: see evaluation.ranking_curve."""
    s = np.asarray(scores, dtype=np.float32)
    lab = labels_bool(labels)
    out = s.copy()
    if adjust is None:
        return out
    point = isinstance(adjust, str) and adjust == "point"
    if not point:
        tag, K = adjust
        assert tag == "k" and 0 <= K <= 100
    for a, b in zip(*segments(lab)):
        seg = s[a:b]
        numbers = np.sort(seg[~np.isnan(seg)])[::-1]
        if point:
            if numbers.size:
                out[a:b] = numbers[0]
                if a == 0:
                    out[0] = s[0]
        else:
            m = K * int(b - a) // 100 + 1
            if numbers.size >= m:
                kth = numbers[m - 1]
                out[a:b] = np.where(np.isnan(seg), kth, np.maximum(seg, kth))
    return out


def ranking_curve(scores, labels, adjust=None):
    lab = labels_bool(labels)
    adj = adjusted_scores(scores, lab, adjust)
    key = order_key(adj, True)
    order = np.argsort(key, kind="stable")
    key, pos = key[order], lab[order].astype(np.int64)
    numeric = key != np.uint32(0xFFFFFFFF)
    last = np.flatnonzero(numeric & np.concatenate((key[1:] != key[:-1], [True])))
    tp = np.cumsum(pos)[last]
    fp = (last + 1) - tp
    thresholds = adj[order][last].astype(np.float32)
    thresholds = np.where(thresholds == 0, np.float32(0), thresholds).astype(np.float32)
    n_pos, n_neg = int(pos.sum()), int(pos.size - pos.sum())
    num_pos = int(tp[-1]) if last.size else 0
    num_neg = int(fp[-1]) if last.size else 0
    return {"thresholds": thresholds, "tp": tp.astype(np.int64), "fp": fp.astype(np.int64), "n_pos": n_pos, "n_neg": n_neg,
            "nan_pos": n_pos - num_pos, "nan_neg": n_neg - num_neg}


def f1_of_counts(tp, fp, fn):
    tp, fp, fn = (np.asarray(v, dtype=np.float64) for v in (tp, fp, fn))
    prec = tp / (tp + fp + 0.00001)
    rec = tp / (tp + fn + 0.00001)
    return 2 * prec * rec / (prec + rec + 0.00001), prec, rec


def ranking_metrics(scores, labels, adjust=None):
    c = ranking_curve(scores, labels, adjust)
    tp, fp, n_pos, n_neg = c["tp"], c["fp"], c["n_pos"], c["n_neg"]
    tpg = np.diff(np.concatenate(([0], tp)))
    fpg = np.diff(np.concatenate(([0], fp)))
    auc2 = sum(int(a) * (2 * (n_neg - int(F)) + int(b)) for a, b, F in zip(tpg, fpg, fp)) + c["nan_pos"] * c["nan_neg"]
    auroc = auc2 / (2 * n_pos * n_neg) if n_pos and n_neg else float("nan")
    terms = tpg.astype(np.float64) * (tp.astype(np.float64) / (tp + fp).astype(np.float64))
    ap = math.fsum(terms.tolist()) / n_pos if n_pos else float("nan")
    best = best_index = None
    if tp.size:
        f1, prec, rec = f1_of_counts(tp, fp, n_pos - tp)
        best_index = int(np.argmax(f1))                     # the first of equal values: the highest threshold
        g = best_index
        best = {"f1": float(f1[g]), "precision": float(prec[g]), "recall": float(rec[g]), "TP": float(tp[g]), "TN": float(n_neg - fp[g]),
                "FP": float(fp[g]), "FN": float(n_pos - tp[g]), "threshold": float(c["thresholds"][g])}
    return {"auroc": auroc, "average_precision": ap, "best": best, "best_index": best_index, "n_thresholds": int(tp.size), "n_pos": n_pos,
            "n_neg": n_neg, "adjust": adjust}
