"""The specification of scoring a gappy series (evaluation.scored_rows, anomaly_scores(age=), the skip_nan arguments,
MTAD_GAT.anomaly_scores(age=), predict_anomalies(mask=); the mtadgat_eval_mark_rows, _scores_masked, _row_means_valid,
_column_quantiles_valid, _ewm_valid and _moments_valid entry points), in numpy float64 straight from the definitions.  Imports
neither the package nor pandas.

A score exists exactly where a training window would have been drawn: score i belongs to window start i and target row i + W, and
exists iff fit_mask_refs' three window rules hold for start i.  NaN means "no score"; +-inf is a value.

  scored_rows           uint8 (n_rows - W,): the three rules, start by start (brute force; fit_mask_refs.windows is held equal).
  scores_masked         eval_refs.scores' expression -- the subtractions in float32 as in the kernel -- where the target sample is
                        observed (age <= max_age) and keep != 0, NaN elsewhere; per row the mean over those entries, NaN without
                        one; their number.
  row_means_valid       the mean over the non-NaN entries of every row.
  nan_quantile          score_refs.quantile's definition over the m non-NaN entries of each column; NaN for m = 0.
  ewm_valid             N_t = (obs ? x_t : 0) + b N_{t-1}, D_t = (obs ? 1 : 0) + b D_{t-1}, y_t = N_t / D_t at an observed row, NaN at
                        an unobserved one; the sequential float64 recursion.
  moments_valid         (sum, sum of squares, count) of the non-NaN entries (exact sums: math.fsum).
  find_epsilon_valid    find_epsilon with mean, sd and counts over the non-NaN entries; a NaN row is neither pruned nor hot but
                        counts as dilated inside a hot row's halo; the fallback is the maximum over the non-NaN entries; NaN
                        without one.  Returns the threshold and the z scores (for the seeds' margin check).
  anomaly_scores_masked the composition MTAD_GAT.anomaly_scores(age=) performs."""
import math

import numpy as np

import fit_mask_refs
import score_refs

ZS = np.arange(2.5, 12, 0.5)
HALO = 49


def min_count(min_observed, W, F):
    return int(math.ceil(float(min_observed) * W * F))


def scored_rows(n_rows, W, F, age, max_age=0, min_observed=0.5, dims=None, lengths=None):
    obs = np.asarray(age) <= max_age
    cols = list(range(F)) if dims is None else [int(c) for c in dims]
    offs = fit_mask_refs.part_offsets(lengths, n_rows)
    need = min_count(min_observed, W, F)
    keep = np.zeros(max(n_rows - W, 0), dtype=np.uint8)
    for i in range(keep.size):
        one_part = any(lo <= i and i + W < hi for lo, hi in zip(offs[:-1], offs[1:]))
        target = any(obs[i + W, c] for c in cols)
        enough = int(obs[i:i + W].sum()) >= need
        keep[i] = one_part and target and enough
    return keep


def scores_masked(preds32, recons32, actual32, age_rows, max_age=0, keep=None, dims=None, gamma=1.0):
    """(per_dim (n, d) float64, global (n,) float64, count (n,) int32).  actual32 / age_rows: the rows of the scores, indexed by the
    column dims[k] (None: k)."""
    p, r = np.asarray(preds32, np.float32), np.asarray(recons32, np.float32)
    n, d = p.shape
    cols = np.arange(d) if dims is None else np.asarray(dims, dtype=np.int64)
    with np.errstate(all="ignore"):
        t = np.asarray(actual32, np.float32)[:, cols]
        a = np.abs((p - t).astype(np.float64)) + np.float64(np.float32(gamma)) * np.abs((r - t).astype(np.float64))
    valid = np.asarray(age_rows)[:, cols] <= max_age
    if keep is not None:
        valid = valid & (np.asarray(keep).reshape(-1, 1) != 0)
    cnt = valid.sum(axis=1)
    with np.errstate(all="ignore"):                    # (a NaN that IS observed is a value: it reaches the mean)
        glob = np.where(cnt > 0, np.where(valid, a, 0.0).sum(axis=1) / np.maximum(cnt, 1), np.nan)
    return np.where(valid, a, np.nan), glob, cnt.astype(np.int32)


def row_means_valid(per_dim):
    a = np.asarray(per_dim, dtype=np.float64)
    valid = ~np.isnan(a)
    cnt = valid.sum(axis=1)
    with np.errstate(all="ignore"):
        s = np.where(valid, a, 0.0).sum(axis=1)
        return np.where(cnt > 0, s / np.maximum(cnt, 1), np.nan)


def nan_quantile(a, qs):
    """(len(qs), d) float64, not rounded; (d,) int64 counts."""
    a = np.asarray(a)
    if a.ndim == 1:
        a = a[:, None]
    out = np.full((len(qs), a.shape[1]), np.nan)
    counts = np.zeros(a.shape[1], dtype=np.int64)
    for c in range(a.shape[1]):
        v = a[:, c]
        v = v[~np.isnan(v)]
        counts[c] = v.size
        if v.size:
            out[:, c] = score_refs.quantile(v, qs)[:, 0]
    return out, counts


def ewm_valid(x, span):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    b = 1.0 - 2.0 / (float(span) + 1.0)
    out = np.full(x.size, np.nan)
    num = den = 0.0
    for t, v in enumerate(x.tolist()):
        obs = not math.isnan(v)
        num = (v if obs else 0.0) + b * num
        den = (1.0 if obs else 0.0) + b * den
        if obs:
            out[t] = num / den
    return out


def moments_valid(e32):
    """(d, 3) float64: sum, sum of squares, count per column of the non-NaN entries."""
    e = np.asarray(e32, dtype=np.float32).astype(np.float64)
    if e.ndim == 1:
        e = e[:, None]
    out = np.zeros((e.shape[1], 3))
    for c in range(e.shape[1]):
        v = e[~np.isnan(e[:, c]), c]
        out[c] = math.fsum(v.tolist()), math.fsum((v * v).tolist()), v.size
    return out


def find_epsilon_valid(e32, reg_level=1, with_scores=False):
    e = np.asarray(e32, dtype=np.float32).astype(np.float64).reshape(-1)
    valid = ~np.isnan(e)
    m = int(valid.sum())
    if m == 0:
        return (float("nan"), []) if with_scores else float("nan")
    v = e[valid]
    mean, sd = v.mean(), v.std()
    best, max_score, scores = None, -10000000, []
    n = e.size
    idx = np.arange(n)
    with np.errstate(all="ignore"):
        for z in ZS:
            eps = mean + sd * z
            above = e >= eps                                   # (false for NaN)
            if not above.any():
                continue
            c = np.concatenate(([0], np.cumsum(above)))
            dil = int(np.sum(c[np.minimum(idx + HALO, n - 1) + 1] - c[np.maximum(idx - HALO, 0)] > 0))
            pruned = e[e < eps]                                # (false for NaN)
            if pruned.size == 0:
                continue
            score = ((mean - pruned.mean()) / mean + (sd - pruned.std()) / sd) / (1 if reg_level == 0 else dil if reg_level == 1 else dil ** 2)
            scores.append((float(score), dil < m * 0.5))
            if score >= max_score and dil < m * 0.5:
                max_score, best = score, eps
    thr = float(v.max()) if best is None else float(best)
    return (thr, scores) if with_scores else thr


def best_two_margin(scores):
    """The relative distance of the two best DISTINCT qualifying z scores (inf with fewer than two).  Two z with the same pruned set
    and dilation have the same score exactly -- the last of them wins, here and on the device, whose comparison takes "equal" with a
    1e-9 margin --, so scores within 1e-12 relative are one value; what must not happen is two different sets scoring within the
    device's margin of each other."""
    s = sorted((v for v, ok in scores if ok and math.isfinite(v)), reverse=True)
    for v in s[1:]:
        if s[0] - v > 1e-12 * abs(s[0]):
            return (s[0] - v) / abs(s[0])
    return math.inf


def scale_valid(per_dim):
    q, _ = nan_quantile(np.asarray(per_dim, dtype=np.float32), [0.25, 0.5, 0.75])
    with np.errstate(all="ignore"):
        return (np.asarray(per_dim, dtype=np.float64) - q[1]) / (1.0 + (q[2] - q[0]))


def anomaly_scores_masked(preds32, recons32, values32, W, age, max_age=0, min_observed=0.5, dims=None, lengths=None, gamma=1.0,
                          scale=False, span=None):
    """(global (n,), per_dim (n, d), keep (n,) uint8) in float64, each stage from the previous stage's float64 values."""
    values32 = np.asarray(values32, dtype=np.float32)
    n_rows, F = values32.shape
    keep = scored_rows(n_rows, W, F, age, max_age, min_observed, dims, lengths)
    per_dim, glob, _ = scores_masked(preds32, recons32, values32[W:], np.asarray(age)[W:], max_age, keep, dims, gamma)
    if scale:
        per_dim = scale_valid(per_dim.astype(np.float32))
        glob = row_means_valid(per_dim)
    if span is not None:
        glob = ewm_valid(glob, span)
    return glob, per_dim, keep
