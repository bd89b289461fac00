"""Reference arithmetic of the event table (evaluation.flag_runs / run_statistics / first_hits / anomaly_events) in numpy,
straight from the definitions.  Imports neither the package nor torch."""
import numpy as np


def flags(scores, threshold, compare_f32=False):
    """scores > threshold as numpy compares a float32 array with a Python float (float64), or in float32; NaN is not flagged."""
    s = np.asarray(scores, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (s > np.float32(threshold)) if compare_f32 else (s.astype(np.float64) > float(threshold))


def runs(flag, merge_gap=0, min_length=1):
    """(start, end) int64 of the maximal runs of `flag`, end exclusive: runs at most merge_gap apart merged, then those shorter than
    min_length dropped."""
    d = np.diff(np.concatenate(([0], np.asarray(flag).astype(bool).astype(np.int8), [0])))
    start, end = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    if start.size:
        keep = start[1:] - end[:-1] > merge_gap
        start, end = start[np.concatenate(([True], keep))], end[np.concatenate((keep, [True]))]
    long_enough = end - start >= min_length
    return start[long_enough].astype(np.int64), end[long_enough].astype(np.int64)


def stats(scores, start, end, per_dim=None, thresholds=None, top_k=5):
    """Per run: peak (first argmax with NaN masked to -inf), peak_score, mean_score (float64 sum / length, not rounded); with
    per_dim (n, d): feature_means (float64), top_features / top_values by the float32 means (stable descending argsort, NaN last);
    with thresholds (d,): feature_hits, rows with per_dim >= threshold in float64."""
    s = np.asarray(scores, dtype=np.float32)
    count = len(start)
    out = {"peak": np.empty(count, np.int64), "peak_score": np.empty(count, np.float32), "mean_score": np.empty(count, np.float64)}
    if per_dim is not None:
        a = np.asarray(per_dim, dtype=np.float32)
        k = min(top_k, a.shape[1], 64)
        out["feature_means"] = np.empty((count, a.shape[1]), np.float64)
        out["top_features"] = np.empty((count, k), np.int32)
        out["top_values"] = np.empty((count, k), np.float32)
        if thresholds is not None:
            out["feature_hits"] = np.empty((count, a.shape[1]), np.int32)
    for i, (lo, hi) in enumerate(zip(start, end)):
        x = s[lo:hi]
        masked = np.where(np.isnan(x), -np.inf, x)
        p = int(np.argmax(masked))
        out["peak"][i], out["peak_score"][i] = lo + p, masked[p]
        out["mean_score"][i] = x.astype(np.float64).sum() / (hi - lo)
        if per_dim is not None:
            rows = a[lo:hi].astype(np.float64)
            out["feature_means"][i] = rows.sum(axis=0) / (hi - lo)
            means32 = out["feature_means"][i].astype(np.float32)
            order = np.argsort(-means32, kind="stable")[:k]
            out["top_features"][i], out["top_values"][i] = order, means32[order]
            if thresholds is not None:
                out["feature_hits"][i] = (rows >= np.asarray(thresholds, dtype=np.float64)).sum(axis=0)
    return out


def first_hit(flag, start, end):
    """The first set index of `flag` inside every [start, end), or -1."""
    f = np.asarray(flag).astype(bool)
    out = np.full(len(start), -1, np.int64)
    for i, (lo, hi) in enumerate(zip(start, end)):
        hit = np.flatnonzero(f[lo:hi])
        if hit.size:
            out[i] = lo + hit[0]
    return out


def events(scores, threshold, per_dim=None, thresholds=None, labels=None, merge_gap=0, min_length=1, top_k=5, compare_f32=False):
    """What evaluation.anomaly_events returns, as numpy arrays."""
    flag = flags(scores, threshold, compare_f32)
    start, end = runs(flag, merge_gap, min_length)
    out = {"count": len(start), "start": start, "end": end}
    out.update(stats(scores, start, end, per_dim, thresholds if per_dim is not None else None, top_k))
    if labels is not None:
        lab = np.asarray(labels).astype(bool)
        out["event_is_true"] = first_hit(lab, start, end) >= 0
        seg_start, seg_end = runs(lab)
        hit = first_hit(flag, seg_start, seg_end)
        out["segments"] = {"start": seg_start, "end": seg_end, "first_hit": hit, "latency": np.where(hit >= 0, hit - seg_start, -1)}
    return out
