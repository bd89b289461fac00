"""The specification of the part-aware score passes (evaluation.score_parts, adjust_part_scores, moving_average(parts=),
find_epsilon_parts, part_predictions), in numpy float64 straight from the definitions.  Imports neither the package nor pandas.

A series of N rows is the concatenation of P parts with `lengths` rows each; score i (0 <= i < n = N - W) targets row i + W and
belongs to the part of that row.  The reference's adjust_anomaly_scores (utils.py:210-255) could not be run here; where this file
departs from it on purpose it says so."""
import numpy as np

import score_refs
from oracle import eval_oracle


def offsets(lengths):
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64))))


def spans(lengths, W):
    """(start, end): part p owns the scores [max(o_p - W, 0), max(o_{p+1} - W, 0)) -- half-open, where the reference's slices
    [c_start : c_end + 1] share one sample."""
    o = offsets(lengths)
    cut = np.maximum(o - W, 0)
    return cut[:-1], cut[1:]


def part_labels(lengths, W):
    """The part of every score by brute force: the part of its target row."""
    row_part = np.repeat(np.arange(len(lengths)), np.asarray(lengths, dtype=np.int64))
    return row_part[W:]


def seams(lengths, W):
    """o_p - W for 1 <= p < P, those inside [0, n) only."""
    o = offsets(lengths)
    n = int(o[-1]) - W
    return [int(t) for t in o[1:-1] - W if 0 <= t < n]


def transition_mask(lengths, W, transition):
    """True where a score lies in [t - before, t + after] of some seam t, by brute force over the seams."""
    n = int(offsets(lengths)[-1]) - W
    before, after = transition
    mask = np.zeros(n, dtype=bool)
    for t in seams(lengths, W):
        mask[max(t - before, 0):min(t + after, n - 1) + 1] = True
    return mask


def adjust(x, lengths, W, transition, normalize=True):
    """Transitional scores become +0.0; then per part (and column) y = (x - lo) / (hi - lo) with lo / hi over the part's non-NaN
    values after blanking.  NaN stays NaN, infinities are ordinary values; a part with hi == lo, without a non-NaN value or empty
    maps its non-NaN values to +0.0 (the reference has 0 / 0 = NaN for a constant part).  float64, not rounded."""
    x = np.asarray(x)
    y = x.astype(np.float64).reshape(x.shape[0], -1).copy()
    y[transition_mask(lengths, W, transition)] = 0.0
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for s, e in zip(*spans(lengths, W)):
                for c in range(y.shape[1]):
                    v = y[s:e, c]
                    ok = ~np.isnan(v)
                    if not ok.any():
                        continue
                    lo, hi = v[ok].min(), v[ok].max()
                    v[ok] = (v[ok] - lo) / (hi - lo) if hi > lo else 0.0
    return y.reshape(x.shape)


def ewm_parts(x, lengths, W, span):
    """score_refs.ewm of every part's slice on its own (the reference smooths across the seams).  float64."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    for s, e in zip(*spans(lengths, W)):
        if e > s:
            out[s:e] = score_refs.ewm(x[s:e], span)
    return out


def thresholds(x, lengths, W, reg_level=1):
    """eval_oracle.find_epsilon of every part's slice; +inf for an empty part."""
    x = np.asarray(x)
    return np.array([eval_oracle.find_epsilon(x[s:e], reg_level) if e > s else np.inf for s, e in zip(*spans(lengths, W))], dtype=np.float64)


def flags(x, lengths, W, thr):
    """score_i > thr[part(i)], compared in float64: NaN and equality are not flagged."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (x > np.asarray(thr, dtype=np.float64)[part_labels(lengths, W)]).astype(np.uint8)


# ---- layouts the tests share ---------------------------------------------------------------------------------------------------
def lengths_from_seams(n, W, at):
    """The lengths of the parts of an (n + W)-row series whose seams, in score space, are the sorted positions `at` inside (0, n)."""
    cuts = sorted({int(t) + W for t in at if 0 < t < n})
    return np.diff([0] + cuts + [n + W]).tolist()


def layouts(n, W):
    """{name: lengths} for n scores and window W: one part; every part of length 1 (n <= 4097); seams at every multiple of 1024
    and at +-1 of it; many short parts around one long part; parts with empty spans (parts that end inside the first window,
    zero-length parts in the middle and at the end)."""
    N = n + W
    out = {"one": [N]}
    if n <= 4097:
        out["ones"] = [1] * N
    out["k1024"] = lengths_from_seams(n, W, [1024 * k + j for k in range(1, n // 1024 + 2) for j in (-1, 0, 1)])
    short = [t for t in (1, 3, 4, 9, 10, 17, 30, 31, 33, 64) if t < n] + [n - t for t in (65, 40, 39, 12, 5, 2, 1) if n - t > 64]
    out["short_long"] = lengths_from_seams(n, W, short)
    head = [1, 0, W // 2] if W >= 4 else [0]
    rest = N - sum(head)
    body = [rest // 3, 0, 0, rest - rest // 3 - rest // 5, 0, rest // 5, 0]
    out["empty"] = head + body
    for name, ls in out.items():
        assert sum(ls) == N and min(ls) >= 0, (name, n, W)
    return out
