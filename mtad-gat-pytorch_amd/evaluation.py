"""Anomaly-score post-processing on the GPU, under the reference's own function names.

Mirrors `eval_methods.py` (find_epsilon :189-236, adjust_predicts :6-55, calc_point2point :58-72,
epsilon_eval :164-186, bf_search :117-158) and the score arithmetic of `Predictor.get_score`
(prediction.py:72-91) on device-resident arrays: the O(N) passes -- moments, the 19-z epsilon table with its
+-49-sample dilation, point-adjusted confusion counts for one threshold or a whole sweep -- are HIP kernels
(csrc/mtadgat_eval.hip behind the `mtadgat_eval_*` C entry points); the scalar bookkeeping on top (which z /
threshold wins, precision / recall / F1 from the counts) is done here in float64 exactly as the reference writes
it -- find_epsilon's host half once (_epsilon_thresholds, _chosen_epsilons) for an array, its columns and its parts.
Results equal the reference's dictionaries (tests/test_gpu_eval.py: the shipped MSL run's summary.txt).

The Predictor's options on top of the raw score (prediction.py:65-165) stay on the device too
(csrc/mtadgat_evalcol.hip, tests/test_gpu_score_pipeline.py):
  column_quantiles / scale_scores   --scale_scores: (a - median) / (1 + IQR) per output dimension; np.percentile's linear
                                    quantiles of all columns from one exact radix select (no sort, any n < 2^31)
  moving_average                    --use_mov_av: pandas' ewm(span).mean() as a float64 blocked scan; with parts= the same scan
                                    restarted at every part (one kernel template, two entry points)
  find_epsilon_columns /            the per-feature thresholds and predictions (prediction.py:140-154): both find_epsilon
  feature_predictions               passes over all columns in one launch each
  predict_anomalies                 what Predictor.predict_anomalies computes from a train and a test series, in one call

From the thresholded scores to alarms (csrc/mtadgat_events.hip, tests/test_gpu_events.py), beyond what the reference offers:
  flag_runs                         ordered [start, end) runs of scores > threshold or of labels, near-by runs merged and short
                                    ones dropped: three stream compactions as blocked scans, nothing sorted, no atomics
  run_statistics                    per run: peak, mean, per-feature means and hit counts, top-k features (segmented reductions)
  first_hits                        the first flagged sample per run: detection latency per labelled segment, true / false events
  anomaly_events                    the three together: the event table of a score array, in score-index space
  explain_events                    model.score_attribution at the events' peaks, with per-feature and per-lag marginals

Peaks-over-threshold thresholds, static and adaptive (csrc/mtadgat_spot.hip and mtadgat_spot.h, tests/test_gpu_spot.py):
  spot_calibrate / spot_run         SPOT (Siffer et al., KDD 2017) for every column of a score matrix at once: one wave per column
                                    fits the generalized Pareto tail of the column's excesses in float64; the state stays on the
                                    device and also serves streaming.StreamScorer as a per-stream adaptive threshold
  pot_eval                          the reference's third threshold method beside epsilon_eval and bf_search (`--dynamic_pot` with
                                    dynamic=True)
Threshold-free quality of a score array (csrc/mtadgat_curves.hip, tests/test_gpu_curves.py; tests/curve_refs.py is the specification):
  score_order                       the indices of a score array in rank order: a deterministic, stable key / payload radix sort
  ranking_curve                     every distinct threshold with its cumulative TP / FP, for the raw scores, the reference's point
                                    adjust or PA%K (Kim et al., AAAI 2022), adjusted and ranked without the scores leaving the device
  ranking_metrics                   exact AUROC, average precision and the best-F1 point of that curve, from one small copy
Series that are concatenations of independent parts -- the channels of MSL / SMAP, the machines of SMD (csrc/mtadgat_parts.hip, the
segmented scan of csrc/mtadgat_evalcol.hip and the epsilon tile of csrc/mtadgat_scan.h that find_epsilon shares;
tests/test_gpu_parts.py; tests/part_refs.py is the specification; the reference's adjust_anomaly_scores, utils.py:210-255):
  score_parts                       where the parts lie among the scores: spans, seams and the transition blanked around a seam
  adjust_part_scores                the scores around every seam set to 0, then min-max normalisation per part (and per column)
  moving_average(parts=)            the exponentially weighted mean restarted at every part: a segmented float64 scan
  find_epsilon_parts /              find_epsilon of every part's slice in two launches and two small copies whatever the number
  part_predictions                  of parts, and scores > the threshold of their own part
  part_quantiles /                  np.percentile of every (part, column) from one segmented exact radix select: short parts wholly
  scale_scores(parts=)              inside one workgroup, long ones through the column select's passes restricted to their rows; then
                                    (a - median) / (1 + IQR) with every row's own part's quantiles (tests/test_gpu_part_scale.py;
                                    tests/part_scale_refs.py is the specification)
  predict_anomalies(parts=)         the above inside the one-call pipeline, with one global or one threshold per part, and with
                                    scale_scores="per_part" the per-dimension scores scaled part by part
The reference's Trainer.evaluate (training.py:188-228) on the device (csrc/mtadgat_losses.hip, tests/test_gpu_losses.py; tests/loss_refs.py
is the specification):
  window_sse                        per window the squared forecast and reconstruction error against the series the windows were cut
                                    from, and the same squares per output dimension: float32 differences, float64 sums, fixed order
  group_sums / group_losses         sums over consecutive loader batches of windows, and the reference's epoch losses from them
                                    (MTAD_GAT.series_losses runs the forward and these without the reconstructions leaving the library)
Series with filled sensor gaps (csrc/mtadgat_evalmask.hip and the NaN-skipping instantiation of the column select in
csrc/mtadgat_evalcol.hip; tests/test_gpu_score_mask.py; tests/score_mask_refs.py is the specification).  A score exists exactly where
fitting.training_windows would have drawn a training window; NaN means "no score", +-inf is a value:
  scored_rows                       which scores exist, from the ages the preparation reports: mtadgat_fit_windows and a marking
                                    kernel, the count never leaving the device
  anomaly_scores(age=, keep=)       the score arithmetic over observed target samples only, with the number of them per row
  column_quantiles / scale_scores / np.nanpercentile from the exact select with per-column ranks, the exponentially weighted mean
  moving_average / find_epsilon*    over scored rows as a two-component scan, fixed-order moments with counts: all with
  (skip_nan=True)                   skip_nan=True; not together with parts=
  predict_anomalies(mask=)          the above inside the one-call pipeline.  Not covered: masks in streams, per-part masked scoring,
                                    SPOT and ranking curves on unscored rows
The fit follows the paper, not the reference's vendored spot.py (its optimiser-based root search cannot be reproduced bit for
bit): tests/spot_refs.py is the specification, csrc/mtadgat_spot.h spells it out.
"""
import ctypes
import math

import numpy as np
import torch

import _native

_c_double_p = ctypes.POINTER(ctypes.c_double)


_lib = _native.load_library           # (tests/pointer_proxy.py replaces it: every call below fetches the library through it)
_stream, _scratch, _fail = _native._stream, _native._scratch, _native._fail


def _dev1d(t, dtype, name):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{name} must be a tensor on the GPU (the evaluation kernels are HIP only)")
    t = t.detach().reshape(-1)
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"mtadgat {what} failed (status {rc})")


def _dev2d(t, name):
    """A float32 (n, d) GPU tensor whose rows are contiguous (a column slice keeps its row stride: no copy)."""
    return _native._rows2d(t, name, gpu_only=True)


def scored_rows(n_rows, window_size, n_features, age, max_age=0, min_observed=0.5, target_dims=None, lengths=None):
    """Which scores of a gappy series exist: a uint8 (n_rows - W,) device tensor, 1 exactly where fitting.training_windows would have
    drawn a training window.  Score i belongs to window start i and target row i + W; it exists iff
      1. rows i .. i + W lie in one part (lengths: the parts' row counts; None: one part),
      2. the target row i + W has an observed sample among the columns target_dims (None: all),
      3. rows i .. i + W - 1 hold at least ceil(min_observed W F) observed samples over all columns.
    age: int32 (n_rows, F) on the device as SeriesScaler.transform(..., return_age=True) returns it; a sample is observed iff
    age <= max_age.  Arguments are checked as training_windows checks them.  Two device calls (mtadgat_fit_windows,
    mtadgat_eval_mark_rows); the number of valid starts stays on the device: nothing is read back."""
    import fitting
    import preparation
    lib = _lib()
    n_rows, W, F = int(n_rows), int(window_size), int(n_features)
    min_count = fitting._min_count(min_observed, W, F)
    if not isinstance(age, torch.Tensor) or age.device.type != "cuda":
        raise RuntimeError("age must be an int32 tensor on the GPU (the window sampler is HIP only)")
    device = age.device
    if n_rows < W + 1:
        raise ValueError("the series is shorter than a window and its target row")
    dims = None
    if target_dims is not None:
        cols = [target_dims] if isinstance(target_dims, int) else [int(d) for d in target_dims]
        dims = torch.tensor(_target_dims(cols, len(cols), F), dtype=torch.int32, device=device)
    offsets = None
    if lengths is not None:
        offsets = torch.tensor(preparation._part_offsets(lengths, n_rows), dtype=torch.int64, device=device)
    starts, count = _native.fit_windows(n_rows, W, F, device, age=age, max_age=max_age, dims=dims, offsets=offsets, min_count=min_count)
    n = n_rows - W
    keep = _native._empty((n,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        rc = lib.mtadgat_eval_mark_rows(starts.data_ptr(), count.data_ptr(), n, keep.data_ptr(), _stream(device))
    if rc != 0:
        _fail(lib, rc, "eval_mark_rows")
    return keep


def anomaly_scores(preds, recons, values, window_size, target_dims=None, gamma=1.0, age=None, max_age=0, keep=None):
    """a_i[d] = |y_hat_i[d] - x_{i+W}[d]| + gamma |recon_i[d] - x_{i+W}[d]| and its mean over d
    (prediction.py:72-91, before the optional per-dimension scaling).  Returns (global (n,), per_dim (n, d)).
    With age -- the whole series' (N, F) int32 ages of SeriesScaler.transform(..., return_age=True) -- a filled sample is not scored:
    per_dim[i][d] is NaN where the target sample is unobserved (age > max_age) or keep[i] == 0 (keep: uint8 (n,) on the device as
    scored_rows returns it, None: all rows kept), global is the mean over the row's remaining entries (NaN when there is none), and
    the result is (global, per_dim, count) with count (n,) int32 their number.  With everything observed and kept global and per_dim
    are the plain call's bit for bit."""
    lib = _lib()
    if age is None and keep is not None:
        raise ValueError("keep needs age")
    n, d = preds.shape
    if values.ndim != 2 or values.shape[0] < window_size + n:
        raise ValueError(f"values must hold at least window_size + n = {window_size + n} rows (the series the {n} windows were cut "
                         f"from), got shape {tuple(values.shape)}")
    if recons.shape[0] != n or recons.shape[-1] != d:
        raise ValueError(f"recons {tuple(recons.shape)} does not match preds {tuple(preds.shape)}")
    actual = values[window_size:window_size + n].float().contiguous()
    dims = None
    if target_dims is not None:
        dims = torch.tensor([target_dims] if isinstance(target_dims, int) else list(target_dims), dtype=torch.int32, device=preds.device)
        if dims.numel() != d:
            raise RuntimeError("target_dims do not match the model's out_dim")
        tl = [target_dims] if isinstance(target_dims, int) else list(target_dims)
        if min(tl) < 0 or max(tl) >= actual.shape[1]:
            raise ValueError(f"target_dims {tl} outside the series' {actual.shape[1]} columns")
    elif actual.shape[1] != d:
        raise RuntimeError("out_dim differs from the number of features: pass target_dims")
    p, r = preds.float().contiguous(), recons.float().contiguous()
    per_dim = _native._empty((n, d), dtype=torch.float32, device=preds.device)
    glob = _native._empty((n,), dtype=torch.float32, device=preds.device)
    if age is not None:
        N, F = values.shape
        _native._age_rows(age, N, F, preds.device)
        rows = age[window_size:window_size + n]
        if keep is not None and (not isinstance(keep, torch.Tensor) or keep.dtype != torch.uint8 or keep.device != preds.device
                                 or keep.ndim != 1 or keep.numel() != n or not keep.is_contiguous()):
            raise ValueError(f"keep must be a contiguous uint8 ({n},) tensor on {preds.device}")
        count = _native._empty((n,), dtype=torch.int32, device=preds.device)
        with torch.cuda.device(preds.device):
            rc = lib.mtadgat_eval_scores_masked(p.data_ptr(), r.data_ptr(), actual.data_ptr(), n, d, actual.shape[1],
                                                dims.data_ptr() if dims is not None else None, float(gamma), rows.data_ptr(),
                                                age.stride(0) if N > 1 else F, int(max_age), _ptr(keep), per_dim.data_ptr(),
                                                glob.data_ptr(), count.data_ptr(), _stream(preds))
        if rc != 0:
            _fail(lib, rc, "eval_scores_masked")
        return glob, per_dim, count
    with torch.cuda.device(preds.device):
        _check(lib.mtadgat_eval_scores(p.data_ptr(), r.data_ptr(), actual.data_ptr(), n, d, actual.shape[1],
                                       dims.data_ptr() if dims is not None else None, float(gamma), per_dim.data_ptr(),
                                       glob.data_ptr(), _stream(preds)), "eval_scores")
    return glob, per_dim


def row_means_valid(per_dim):
    """The mean over the non-NaN entries of every row of an (n, d) float32 GPU tensor, added in column order in float32 and divided
    by their number: (n,) float32, NaN for a row without one.  What anomaly_scores(age=) returns as its global score, for
    per-dimension scores that were scaled after the mask was applied."""
    lib = _lib()
    a = _dev2d(per_dim, "per_dim")
    n, d = a.shape
    glob = _native._empty((n,), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = lib.mtadgat_eval_row_means_valid(a.data_ptr(), n, d, a.stride(0), glob.data_ptr(), None, _stream(a))
    if rc != 0:
        _fail(lib, rc, "eval_row_means_valid")
    return glob


def _choose_epsilon(n, mean, sd, eps, tab, reg_level):
    """The host half of find_epsilon (eval_methods.py:205-236): the z whose threshold scores best, from the table the
    device pass returns for one array -- tab[4 k : 4 k + 4] = pruned sum, pruned sum of squares, pruned count, dilated count
    for threshold eps[k].  None when no z qualifies."""
    best, max_score = None, -10000000
    mean64, sd64 = np.float64(mean), np.float64(sd)
    for k in range(len(eps)):
        ps, ps2, pc, dil = tab[4 * k], tab[4 * k + 1], tab[4 * k + 2], tab[4 * k + 3]
        if dil > 0:
            if pc > 0:
                pm = ps / pc
                psd = math.sqrt(max(ps2 / pc - pm * pm, 0.0))
            else:
                pm = psd = float("nan")         # np.mean / np.std of an empty pruned set
            # numpy float64 arithmetic as in the reference: constant scores (sd == 0) or a zero mean give nan / inf here,
            # not ZeroDivisionError; a nan score fails the comparison below and the z is skipped (eval_methods.py:220-231)
            with np.errstate(divide="ignore", invalid="ignore"):
                mean_perc_decrease = (mean64 - np.float64(pm)) / mean64
                sd_perc_decrease = (sd64 - np.float64(psd)) / sd64
                denom = 1 if reg_level == 0 else (dil if reg_level == 1 else dil ** 2)
                score = float((mean_perc_decrease + sd_perc_decrease) / denom)
            # `>=`: among equal scores the reference keeps the last z.  Two z with the same pruned set have the same
            # score exactly in the reference; here their float64 sums come from atomics in varying order, so
            # "equal" is taken with a 1e-9 relative margin.
            at_least = score >= max_score or (math.isfinite(max_score) and score >= max_score - 1e-9 * abs(max_score))
            if at_least and dil < n * 0.5:
                max_score, best = max(score, max_score), float(eps[k])
    return best


_EPSILON_ZS = np.arange(2.5, 12, 0.5)
_EPSILON_HALO = 49


def _epsilon_thresholds(sums, squares, counts):
    """The host half of find_epsilon between its two device passes, for P problems at once: from (sum, sum of squares, count) per
    problem the mean and sd (float64, (P,)) and the (P, nz) thresholds mean + sd * z.  A problem without samples: NaN throughout."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    means, sds = np.full(counts.size, np.nan), np.full(counts.size, np.nan)
    for p in np.flatnonzero(counts > 0):
        means[p] = sums[p] / counts[p]
        sds[p] = math.sqrt(max(squares[p] / counts[p] - means[p] * means[p], 0.0))
    return means, sds, np.ascontiguousarray(means[:, None] + sds[:, None] * _EPSILON_ZS)


def _chosen_epsilons(counts, means, sds, eps, tab, reg_level):
    """_choose_epsilon of every problem that has samples, from the (P, 4 nz) table rows: a list of thresholds, None where no z
    qualifies or there is no sample (the callers differ in what they fall back to)."""
    return [_choose_epsilon(int(counts[p]), float(means[p]), float(sds[p]), eps[p], tab[p], reg_level) if counts[p] > 0 else None
            for p in range(len(eps))]


def find_epsilon(errors, reg_level=1, skip_nan=False):
    """Threshold of Hundman et al. as the reference computes it (eval_methods.py:189-236).
    skip_nan: a NaN is a row without a score (find_epsilon_columns(skip_nan=True) of the one column)."""
    if skip_nan:
        return find_epsilon_columns(_dev1d(errors, torch.float32, "errors"), reg_level, skip_nan=True)[0]
    lib = _lib()
    e = _dev1d(errors, torch.float32, "errors")
    n = e.numel()
    scratch = _native._empty(64 + 4 * 64, dtype=torch.float64, device=e.device)
    mom = (ctypes.c_double * 2)()
    with torch.cuda.device(e.device):
        _check(lib.mtadgat_eval_moments(e.data_ptr(), n, scratch.data_ptr(), mom, _stream(e)), "eval_moments")
    means, sds, eps = _epsilon_thresholds(mom[0:1], mom[1:2], [n])
    tab = np.empty((1, 4 * eps.shape[1]), dtype=np.float64)
    with torch.cuda.device(e.device):
        _check(lib.mtadgat_eval_epsilon_table(e.data_ptr(), n, eps.ctypes.data_as(_c_double_p), eps.shape[1], _EPSILON_HALO,
                                              scratch.data_ptr(), tab.ctypes.data_as(_c_double_p), _stream(e)), "eval_epsilon_table")
    best = _chosen_epsilons([n], means, sds, eps, tab, reg_level)[0]
    return float(e.max().item()) if best is None else best


def moments_valid(errors):
    """Per column of an (n,) or (n, d) float32 GPU tensor the float64 sum, sum of squares and count of its non-NaN entries: a (d, 3)
    float64 numpy array.  Added in a fixed order (mtadgat_eval_moments_valid): two calls give the same bits."""
    lib = _lib()
    e = _dev2d(errors, "errors")
    n, d = e.shape
    scratch = _scratch(lib.mtadgat_eval_moments_valid_scratch(n, d), e.device)
    mom = np.empty((d, 3), dtype=np.float64)
    with torch.cuda.device(e.device):
        rc = lib.mtadgat_eval_moments_valid(e.data_ptr(), n, d, e.stride(0), scratch.data_ptr(), scratch.numel() * 8,
                                            mom.ctypes.data_as(_c_double_p), _stream(e))
    if rc != 0:
        _fail(lib, rc, "eval_moments_valid")
    return mom


def find_epsilon_columns(errors, reg_level=1, skip_nan=False):
    """find_epsilon of every column of an (n, d) array (the per-feature thresholds of prediction.py:140-147): the moments
    and the z table of all columns in one launch each.  Returns a list of d floats; a column where no z qualifies gets its
    maximum, as in find_epsilon.
    skip_nan: a NaN is a row without a score.  Mean, sd and the counts are those of the column's non-NaN entries (moments_valid);
    in the z table a NaN row is neither pruned nor hot -- both comparisons are false -- but counts as dilated inside a hot row's
    halo; the fallback is the maximum over the non-NaN entries; a column without one gets a NaN threshold, which flags nothing."""
    lib = _lib()
    e = _dev2d(errors, "errors")
    n, d = e.shape
    ld = e.stride(0)
    nz = len(_EPSILON_ZS)
    scratch = _native._empty(max(2 * d, 5 * d * nz), dtype=torch.float64, device=e.device)
    if skip_nan:
        mom = moments_valid(e)
        counts = [int(c) for c in mom[:, 2]]
    else:
        mom = np.empty((d, 2), dtype=np.float64)
        with torch.cuda.device(e.device):
            _check(lib.mtadgat_eval_moments_columns(e.data_ptr(), n, d, ld, scratch.data_ptr(), mom.ctypes.data_as(_c_double_p), _stream(e)),
                   "eval_moments_columns")
        counts = [n] * d
    means, sds, eps = _epsilon_thresholds(mom[:, 0], mom[:, 1], counts)
    tab = np.empty((d, 4 * nz), dtype=np.float64)
    with torch.cuda.device(e.device):
        _check(lib.mtadgat_eval_epsilon_table_columns(e.data_ptr(), n, d, ld, eps.ctypes.data_as(_c_double_p), nz, _EPSILON_HALO,
                                                      scratch.data_ptr(), tab.ctypes.data_as(_c_double_p), _stream(e)),
               "eval_epsilon_table_columns")
    out = _chosen_epsilons(counts, means, sds, eps, tab, reg_level)
    if None in out:
        # (the valid maximum: the q = 1 order statistic of the non-NaN entries, NaN for a column without one)
        col_max = (column_quantiles(e, [1.0], skip_nan=True)[0] if skip_nan else e.max(dim=0).values).cpu()
        out = [float(col_max[c]) if best is None else best for c, best in enumerate(out)]
    return out


def column_quantiles(a, qs, skip_nan=False, return_counts=False):
    """np.percentile(a, 100 * qs, axis=0) for an (n, d) float32 GPU tensor, (len(qs), d) float32 on the device: the "linear"
    definition, interpolated in float64 between the two exact order statistics and rounded once.  A column that holds a NaN
    gives NaN, as in numpy.  A column slice of a wider tensor is read in place.  Bitwise reproducible.
    skip_nan: np.nanpercentile -- the same definition over the m non-NaN entries of each column, NaN for m = 0; with return_counts
    the result is (quantiles, m (d,) int64 on the device)."""
    lib = _lib()
    a = _dev2d(a, "a")
    n, d = a.shape
    q = np.ascontiguousarray(np.asarray(qs, dtype=np.float64).reshape(-1))
    if q.size < 1 or not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError(f"quantile probabilities must lie in [0, 1], got {qs!r}")
    if return_counts and not skip_nan:
        raise ValueError("return_counts needs skip_nan")
    if skip_nan:
        scratch = _scratch(lib.mtadgat_eval_column_quantiles_valid_scratch(n, d, q.size), a.device)
        out = _native._empty((q.size, d), dtype=torch.float32, device=a.device)
        counts = _native._empty((d,), dtype=torch.int64, device=a.device)
        with torch.cuda.device(a.device):
            rc = lib.mtadgat_eval_column_quantiles_valid(a.data_ptr(), n, d, a.stride(0), q.ctypes.data_as(_c_double_p), q.size,
                                                         scratch.data_ptr(), scratch.numel() * 8, out.data_ptr(), counts.data_ptr(), _stream(a))
        if rc != 0:
            _fail(lib, rc, "eval_column_quantiles_valid")
        return (out, counts) if return_counts else out
    scratch = _scratch(lib.mtadgat_eval_column_quantiles_scratch(n, d, q.size), a.device)
    out = _native._empty((q.size, d), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = lib.mtadgat_eval_column_quantiles(a.data_ptr(), n, d, a.stride(0), q.ctypes.data_as(_c_double_p), q.size,
                                               scratch.data_ptr(), scratch.numel() * 8, out.data_ptr(), _stream(a))
    if rc != 0:
        _fail(lib, rc, "eval_column_quantiles")
    return out


def part_quantiles(a, qs, parts):
    """np.percentile(a[start[p]:end[p]], 100 * qs, axis=0) for every part p of an (n,) or (n, d) float32 GPU tensor (parts: a
    ScoreParts with parts.n == n), (len(qs), P, d) float32 on the device.  Per (part, column) as column_quantiles: exact order
    statistics, interpolated in float64 and rounded once; a NaN makes its own (part, column) NaN and no other; an empty part gives
    NaN, a part of one row that row.  At most 8 probabilities.  A column slice of a wider tensor is read in place.  The number of
    launches does not depend on P; asynchronous, bitwise reproducible."""
    lib = _lib()
    a = _dev2d(a, "a")
    n, d = a.shape
    start, end, _ = _parts_on(parts, a, n)
    q = np.ascontiguousarray(np.asarray(qs, dtype=np.float64).reshape(-1))
    if q.size < 1 or q.size > 8 or not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError(f"1 to 8 quantile probabilities in [0, 1] are needed, got {qs!r}")
    P = parts.n_parts
    scratch = _scratch(lib.mtadgat_eval_part_quantiles_scratch(n, d, P, q.size), a.device)
    out = _native._empty((q.size, P, d), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = lib.mtadgat_eval_part_quantiles(a.data_ptr(), n, d, a.stride(0), start.data_ptr(), end.data_ptr(), P, q.ctypes.data_as(_c_double_p),
                                             q.size, scratch.data_ptr(), scratch.numel() * 8, out.data_ptr(), _stream(a))
    if rc != 0:
        _fail(lib, rc, "eval_part_quantiles")
    return out


def scale_scores(per_dim, parts=None, skip_nan=False):
    """(a - median) / (1 + IQR) per column (prediction.py:84-88), quantiles from column_quantiles.
    With parts (a ScoreParts with parts.n == len(per_dim)) every part's rows are scaled by the part's own median and IQR
    (part_quantiles), in float32 with every operation rounded on its own: one noisy part no longer sets the scale of the others.
    skip_nan: median and IQR are those of the column's non-NaN entries (column_quantiles(skip_nan=True)); NaN stays NaN.  Not
    together with parts (ValueError): per-part masked scoring is not covered.
    Returns a new float32 tensor of the input's shape."""
    if skip_nan and parts is not None:
        raise ValueError("skip_nan together with parts= is not supported: per-part masked scoring is not covered")
    if parts is None:
        q = column_quantiles(per_dim, [0.25, 0.5, 0.75], skip_nan=skip_nan)
        return (per_dim - q[1]) / (1.0 + (q[2] - q[0]))
    lib = _lib()
    one_d = isinstance(per_dim, torch.Tensor) and per_dim.ndim == 1
    a = _dev2d(per_dim, "per_dim")
    n, d = a.shape
    start, end, _ = _parts_on(parts, a, n)
    q = part_quantiles(a, [0.25, 0.5, 0.75], parts)
    out = _native._empty((n, d), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = lib.mtadgat_eval_part_scale(a.data_ptr(), n, d, a.stride(0), start.data_ptr(), end.data_ptr(), parts.n_parts, q.data_ptr(),
                                         out.data_ptr(), d, _stream(a))
    if rc != 0:
        _fail(lib, rc, "eval_part_scale")
    return out.reshape(-1) if one_d else out


def moving_average(scores, span, parts=None, skip_nan=False):
    """pandas.DataFrame(scores).ewm(span=span).mean() (prediction.py:99-103) of a 1-D GPU tensor: (n,) float32.
    Accumulated in float64 on the device, stored as float32; bitwise reproducible.
    With parts (a ScoreParts with parts.n == len(scores)) the average restarts at the first score of every part, so that no part is
    smoothed into the next: ewm(span).mean() of every part's slice on its own.  The reference smooths across the seams.
    skip_nan: a NaN is a row without a score: it adds nothing to the weighted sum or to the weights, which both decay across it
    (pandas' ewm(span, adjust=True, ignore_na=False).mean() at the scored rows), and stays NaN, where pandas repeats the previous
    mean.  Not together with parts (ValueError)."""
    if not span >= 1:
        raise ValueError(f"span must be >= 1, got {span!r}")
    if skip_nan and parts is not None:
        raise ValueError("skip_nan together with parts= is not supported: per-part masked scoring is not covered")
    lib = _lib()
    x = _dev1d(scores, torch.float32, "scores")
    n = x.numel()
    if n < 1:
        raise ValueError("scores is empty")
    alpha = 2.0 / (float(span) + 1.0)
    out = _native._empty((n,), dtype=torch.float32, device=x.device)
    if parts is None:
        what, spans = ("eval_ewm_valid" if skip_nan else "eval_ewm"), ()
    else:
        start, end, _ = _parts_on(parts, x, n)
        what, spans = "eval_ewm_parts", (start.data_ptr(), end.data_ptr(), parts.n_parts)
    scratch = _scratch(getattr(lib, f"mtadgat_{what}_scratch")(n), x.device)
    with torch.cuda.device(x.device):
        rc = getattr(lib, f"mtadgat_{what}")(x.data_ptr(), n, *spans, alpha, scratch.data_ptr(), scratch.numel() * 8, out.data_ptr(), _stream(x))
    if rc != 0:
        _fail(lib, rc, what)
    return out


def feature_predictions(train_per_dim, test_per_dim, reg_level=1, skip_nan=False):
    """Per-feature thresholds and predictions (prediction.py:140-154): eps_i = find_epsilon(train_per_dim[:, i]) and
    preds[:, i] = test_per_dim[:, i] >= eps_i.  The comparison is `>=`: the reference tree was not at hand to pin the
    operator, so this package fixes it -- a score equal to its threshold counts as anomalous.
    skip_nan: the thresholds from find_epsilon_columns(skip_nan=True); a NaN score or a NaN threshold flags nothing.
    Returns (thresholds (d,) float64 on the host, preds (n_test, d) uint8 on the device)."""
    test = _dev2d(test_per_dim, "test_per_dim")
    thr = find_epsilon_columns(train_per_dim, reg_level, skip_nan=skip_nan)
    if test.shape[1] != len(thr):
        raise ValueError(f"train has {len(thr)} columns, test has {test.shape[1]}")
    # compared in float64 like a float32 array against Python floats in numpy
    thr_d = torch.tensor(thr, dtype=torch.float64, device=test.device)
    return np.asarray(thr, dtype=np.float64), (test.double() >= thr_d).to(torch.uint8)


def point_adjust_counts(score, label, thresholds, compare_f32=False, max_segments=65536):
    """adjust_predicts + calc_point2point for every threshold in one launch.
    Returns an (n_thr, 6) float64 array: TP, TN, FP, FN, latency sum, detected segments."""
    lib = _lib()
    s = _dev1d(score, torch.float32, "score")
    lab = _labels_u8(label, "label")
    if lab.numel() != s.numel():
        raise ValueError("score and label must have the same length")
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    nt = thr.size
    scratch = _native._empty(7 * nt + max_segments + 2, dtype=torch.float64, device=s.device)
    out = np.zeros((nt, 6), dtype=np.float64)
    with torch.cuda.device(s.device):
        _check(lib.mtadgat_eval_point_adjust(s.data_ptr(), lab.data_ptr(), s.numel(), thr.ctypes.data_as(_c_double_p), nt,
                                             1 if compare_f32 else 0, max_segments, scratch.data_ptr(),
                                             out.ctypes.data_as(_c_double_p), _stream(s)), "eval_point_adjust")
    return out


def _scores_from_counts(tp, tn, fp, fn):
    """F1 / precision / recall with the reference's 1e-5 guards (eval_methods.py:6-21)."""
    prec = tp / (tp + fp + 0.00001)
    rec = tp / (tp + fn + 0.00001)
    return 2 * prec * rec / (prec + rec + 0.00001), prec, rec


def _result(counts, threshold, **extra):
    f1, prec, rec = _scores_from_counts(counts[0], counts[1], counts[2], counts[3])
    out = {"f1": f1, "precision": prec, "recall": rec, "TP": counts[0], "TN": counts[1], "FP": counts[2], "FN": counts[3],
           "threshold": threshold, "latency": counts[4] / (counts[5] + 1e-4)}
    out.update(extra)
    return out


def epsilon_eval(train_scores, test_scores, test_labels, reg_level=1, skip_nan=False):
    """Threshold from the training scores (find_epsilon), point-adjusted metrics on the test scores (eval_methods.py:164-186).
    skip_nan: find_epsilon(skip_nan=True); a test row without a score (NaN) is never above the threshold."""
    eps = find_epsilon(train_scores, reg_level, skip_nan=skip_nan)
    if test_labels is None:
        return {"threshold": eps, "reg_level": reg_level}
    return _result(point_adjust_counts(test_scores, test_labels, [eps])[0], eps, reg_level=reg_level)


def bf_search(score, label, start, end=None, step_num=1, display_freq=1, verbose=False):
    """Best-F1 threshold sweep (eval_methods.py:117-158): all thresholds evaluated by one kernel launch."""
    if step_num is None or end is None:
        end, step_num = start, 1
    # the reference walks the thresholds by repeated addition in a Python float: the same sums, so the same thresholds
    increment = (end - start) / float(step_num)
    grid, at = [], start
    for _ in range(step_num):
        at += increment
        grid.append(at)
    table = point_adjust_counts(score, label, grid, compare_f32=True)      # float32 array > Python float: a float32 comparison
    best_row, best_thr, best_f1 = None, 0.0, -1.0
    for thr, row in zip(grid, table):
        f1 = _scores_from_counts(row[0], row[1], row[2], row[3])[0]
        if f1 > best_f1:                               # strict: the first of equal F1 values wins, as in the reference
            best_row, best_thr, best_f1 = row, thr, f1
    if best_row is None:
        return {"f1": -1.0, "precision": -1.0, "recall": -1.0, "TP": -1.0, "TN": -1.0, "FP": -1.0, "FN": -1.0, "threshold": 0.0, "latency": 0}
    return _result(best_row, best_thr)


_sweep = bf_search       # predict_anomalies has a keyword of that name


# ---- series made of parts ----------------------------------------------------------------------------------------------------------
class ScoreParts:
    """Where the parts of a concatenated series lie among its scores (made by score_parts).  Score i (0 <= i < n = N - W) targets
    row i + W and belongs to the part of that row, so part p owns the scores [start[p], end[p]) with
    start[p] = max(o_p - W, 0), end[p] = max(o_{p+1} - W, 0), o the row offsets of the parts: disjoint, ascending, covering
    [0, n), some possibly empty.  `seams` are the positions o_p - W (1 <= p < P) that fall inside [0, n): the first score of a
    new part, around which `transition` = (before, after) scores are blanked by adjust_part_scores.
      lengths, window_size, transition, n, n_parts      as given / derived
      start_host, end_host, seams_host                  int64 numpy arrays
      start, end, seams                                 the same as int64 tensors on `device` (seams is None without a seam)"""

    def __init__(self, lengths, window_size, transition, device):
        self.lengths, self.window_size, self.transition = lengths, window_size, transition
        offsets = np.concatenate(([0], np.cumsum(lengths, dtype=np.int64)))
        self.n = int(offsets[-1]) - window_size
        self.n_parts = len(lengths)
        cut = np.maximum(offsets - window_size, 0)
        self.start_host, self.end_host = np.ascontiguousarray(cut[:-1]), np.ascontiguousarray(cut[1:])
        t = offsets[1:-1] - window_size
        self.seams_host = np.ascontiguousarray(t[(t >= 0) & (t < self.n)])
        self.device = torch.device("cpu" if device is None else device)
        self._on = {}
        self.start, self.end, self.seams = self.tensors(self.device)

    def tensors(self, device):
        """(start, end, seams) on `device`, copied there once."""
        key = str(torch.device(device))
        if key not in self._on:
            put = lambda a: torch.from_numpy(a).to(device) if a.size else None
            self._on[key] = (put(self.start_host), put(self.end_host), put(self.seams_host))
        return self._on[key]

    def use_tensors(self, start, end, seams=None):
        """Hand the kernels the caller's own copies of the span arrays on their device instead of the ones tensors() would make:
        contiguous int64 tensors holding start_host, end_host and seams_host (seams None without a seam).  Only the shapes, types
        and devices are checked; the values are the caller's promise.  Returns self."""
        want = (self.n_parts, self.n_parts, self.seams_host.size)
        for t, size, name in zip((start, end, seams), want, ("start", "end", "seams")):
            if t is None and name == "seams" and size == 0:
                continue
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.ndim != 1 or t.numel() != size or not t.is_contiguous()
                    or t.device != start.device):
                raise ValueError(f"{name} must be a contiguous int64 tensor of {size} entries on the device of start")
        self._on[str(start.device)] = (start, end, seams if self.seams_host.size else None)
        return self

    def part_of(self, i):
        """The part that owns score i (an int or an array of ints in [0, n)): an int or an int64 array."""
        idx = np.asarray(i, dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n):
            raise IndexError(f"score index outside [0, {self.n})")
        p = np.searchsorted(self.end_host, idx, side="right")
        return int(p) if np.ndim(i) == 0 else p


def score_parts(lengths, window_size, transition=(19, 19), device=None):
    """Describe a series of N rows that is the concatenation of len(lengths) independent parts (the channels of MSL / SMAP, the
    machines of SMD) with `lengths` rows each, for a model of window `window_size`: a ScoreParts for the N - window_size scores.
    transition = (before, after): the scores t - before .. t + after around every seam t are blanked by adjust_part_scores; the
    default is the reference's buffer of 19 (utils.py:210-255), and after = window_size - 1 blanks every window that straddles two
    parts.  device: where the span arrays are kept (they are copied to the scores' device on first use otherwise).
    Raises ValueError on negative lengths, a negative transition or sum(lengths) <= window_size."""
    ls = np.asarray(lengths)
    if ls.ndim != 1 or ls.size < 1 or not np.issubdtype(ls.dtype, np.integer):
        raise ValueError(f"lengths must be a non-empty 1-D sequence of integers, got {lengths!r}")
    ls = ls.astype(np.int64)
    if ls.min() < 0:
        raise ValueError("lengths must be >= 0")
    if isinstance(window_size, bool) or int(window_size) != window_size or window_size < 1:
        raise ValueError(f"window_size must be a positive integer, got {window_size!r}")
    if len(transition) != 2 or any(isinstance(t, bool) or int(t) != t or t < 0 for t in transition):
        raise ValueError(f"transition must be two integers >= 0, got {transition!r}")
    if int(ls.sum()) <= window_size:
        raise ValueError(f"the parts hold {int(ls.sum())} rows, which leaves no score for window_size {window_size}")
    return ScoreParts(ls, int(window_size), (int(transition[0]), int(transition[1])), device)


def _parts_on(parts, x, n):
    """parts' arrays on the device of x, after checking that parts describe n scores."""
    if not isinstance(parts, ScoreParts):
        raise TypeError("parts must be a ScoreParts (score_parts)")
    if n != parts.n:
        raise ValueError(f"parts describe {parts.n} scores, got {n}")
    return parts.tensors(x.device)


def adjust_part_scores(scores, parts, normalize=True):
    """The seam handling of the reference's adjust_anomaly_scores (utils.py:210-255) for (n,) or (n, d) scores on the GPU: the
    scores in parts.transition around every seam become +0.0 (a window that straddles two parts cannot be predicted), then, with
    normalize, every part's stretch (per column) is min-max normalised on its own: (x - lo) / (hi - lo) in float64, rounded once,
    lo / hi over the part's non-NaN values after blanking.  NaN stays NaN; +-inf are ordinary values.  Returns a new float32 tensor
    of the input's shape; asynchronous, bitwise reproducible.
    Departures from the reference (whose source could not be run here to pin it; tests/part_refs.py is the specification): a constant,
    all-NaN or empty part maps to +0.0 where the reference divides 0 by 0; the parts are half-open, where the reference's slices
    [c_start : c_end + 1] share one sample that is normalised twice."""
    lib = _lib()
    one_d = isinstance(scores, torch.Tensor) and scores.ndim == 1
    x = _dev2d(scores, "scores")
    n, d = x.shape
    start, end, seams = _parts_on(parts, x, n)
    out = _native._empty((n, d), dtype=torch.float32, device=x.device)
    scratch = _scratch(lib.mtadgat_eval_part_adjust_scratch(n, d, parts.n_parts), x.device) if normalize else None
    with torch.cuda.device(x.device):
        rc = lib.mtadgat_eval_part_adjust(x.data_ptr(), n, d, x.stride(0), start.data_ptr(), end.data_ptr(), parts.n_parts, _ptr(seams),
                                          0 if seams is None else seams.numel(), parts.transition[0], parts.transition[1],
                                          1 if normalize else 0, _ptr(scratch), 0 if scratch is None else scratch.numel() * 8,
                                          out.data_ptr(), d, None, _stream(x))
    if rc != 0:
        _fail(lib, rc, "eval_part_adjust")
    return out.reshape(-1) if one_d else out


def find_epsilon_parts(scores, parts, reg_level=1):
    """find_epsilon of every part's slice of a 1-D score array: a float64 array (P,).  Moments, the 19 z values and the +-49 dilation
    never look outside the part; a part where no z qualifies gets its maximum, an empty part +inf.  Two device passes over all
    parts and two small copies to the host, whatever P is."""
    lib = _lib()
    x = _dev1d(scores, torch.float32, "scores")
    n = x.numel()
    start, end, _ = _parts_on(parts, x, n)
    P, nz = parts.n_parts, len(_EPSILON_ZS)
    scratch = _scratch(lib.mtadgat_eval_part_epsilon_scratch(n, P, nz), x.device)
    mom = np.empty((P, 3), dtype=np.float64)
    with torch.cuda.device(x.device):
        rc = lib.mtadgat_eval_part_epsilon_moments(x.data_ptr(), n, start.data_ptr(), end.data_ptr(), P, nz, scratch.data_ptr(),
                                                   scratch.numel() * 8, mom.ctypes.data_as(_c_double_p), _stream(x))
    if rc != 0:
        _fail(lib, rc, "eval_part_epsilon_moments")
    count = parts.end_host - parts.start_host
    means, sds, eps = _epsilon_thresholds(mom[:, 0], mom[:, 1], count)
    tab = np.empty((P, 4 * nz), dtype=np.float64)
    with torch.cuda.device(x.device):
        rc = lib.mtadgat_eval_part_epsilon_table(x.data_ptr(), n, start.data_ptr(), end.data_ptr(), P, eps.ctypes.data_as(_c_double_p), nz,
                                                 _EPSILON_HALO, scratch.data_ptr(), scratch.numel() * 8, tab.ctypes.data_as(_c_double_p),
                                                 _stream(x))
    if rc != 0:
        _fail(lib, rc, "eval_part_epsilon_table")
    out = np.full(P, np.inf)
    for p, best in enumerate(_chosen_epsilons(count, means, sds, eps, tab, reg_level)):
        if count[p] > 0:
            out[p] = mom[p, 2] if best is None else best
    return out


def part_predictions(scores, parts, thresholds):
    """flags[i] = scores[i] > thresholds[part of i], compared in float64 (NaN and equality are not flagged: flag_runs' convention):
    (n,) uint8 on the device.  thresholds: (P,) numbers, as find_epsilon_parts returns them."""
    lib = _lib()
    x = _dev1d(scores, torch.float32, "scores")
    n = x.numel()
    start, end, _ = _parts_on(parts, x, n)
    thr = torch.as_tensor(np.asarray(thresholds, dtype=np.float64).reshape(-1)).to(x.device)
    if thr.numel() != parts.n_parts:
        raise ValueError(f"{thr.numel()} thresholds for {parts.n_parts} parts")
    flags = _native._empty(n, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.mtadgat_eval_part_flags(x.data_ptr(), n, start.data_ptr(), end.data_ptr(), parts.n_parts, thr.data_ptr(), flags.data_ptr(),
                                         _stream(x))
    if rc != 0:
        _fail(lib, rc, "eval_part_flags")
    return flags


# ---- peaks over threshold ----------------------------------------------------------------------------------------------------------
class SpotState:
    """The device-resident SPOT state of `n_columns` score series (made by spot_calibrate): per column the initial threshold t, the
    alarm threshold z, the counts n and Nt, the fitted tail (gamma, sigma) and a ring of its most recent `max_peaks` excesses.
    The ring is this package's own bound -- Nt counts every excess, the fit sees only the stored ones; until the ring wraps this
    is SPOT's Algorithm 1.  spot_run and a StreamScorer advance the state in place."""

    def __init__(self, buf, n_columns, max_peaks, q, level, dynamic):
        self.buf, self.n_columns, self.max_peaks = buf, int(n_columns), int(max_peaks)
        self.q, self.level, self.dynamic = float(q), float(level), bool(dynamic)

    @property
    def device(self):
        return self.buf.device

    def data_ptr(self):
        return self.buf.data_ptr()

    def read(self):
        """The per-column values as float64 numpy arrays: a dict of t, z, n, Nt, gamma, sigma.  Synchronises."""
        lib = _lib()
        out = np.empty((self.n_columns, 6), dtype=np.float64)
        with torch.cuda.device(self.device):
            rc = lib.mtadgat_spot_read(self.data_ptr(), self.n_columns, self.max_peaks, out.ctypes.data_as(_c_double_p), _stream(self.buf))
        if rc != 0:
            _fail(lib, rc, "spot_read")
        return {name: out[:, k].copy() for k, name in enumerate(("t", "z", "n", "Nt", "gamma", "sigma"))}

    def thresholds(self):
        """The current alarm threshold z of every column: (n_columns,) float64 on the state's device."""
        return torch.from_numpy(self.read()["z"]).to(self.device)

    def clone(self):
        """An independent copy of the state as it stands."""
        return SpotState(self.buf.clone(), self.n_columns, self.max_peaks, self.q, self.level, self.dynamic)

    def expand(self, n_columns):
        """A new state of `n_columns` columns that each start as this state's ONE column: one training series serving many streams."""
        if self.n_columns != 1:
            raise ValueError(f"expand needs a state of one column, this one has {self.n_columns}")
        if int(n_columns) != n_columns or n_columns < 1:
            raise ValueError(f"n_columns must be a positive integer, got {n_columns!r}")
        lib = _lib()
        nbytes = lib.mtadgat_spot_state_bytes(int(n_columns), self.max_peaks)
        if nbytes == 0:
            raise ValueError(f"{n_columns} columns are refused")
        buf = _native._empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)
        buf.zero_()
        with torch.cuda.device(self.device):
            rc = lib.mtadgat_spot_copy(buf.data_ptr(), int(n_columns), self.data_ptr(), 1, self.max_peaks, None, int(n_columns), 1,
                                       _stream(self.buf))
        if rc != 0:
            _fail(lib, rc, "spot_copy")
        return SpotState(buf, n_columns, self.max_peaks, self.q, self.level, self.dynamic)


def spot_calibrate(init_scores, q=1e-3, level=0.98, max_peaks=1024, dynamic=True):
    """Calibrate SPOT on `init_scores`, an (n_init,) or (n_init, S) GPU tensor (read as float32 like every score array here), one
    independent problem per column: the initial threshold t = sorted[int(level * n_init)], the excesses over it in row order (the last
    `max_peaks` of them are kept), and the first generalized Pareto fit, whose q-quantile is the alarm threshold z.  dynamic=False
    makes a state that spot_run and StreamScorer never change (the reference's static POT).  Returns a SpotState.
    The fit is the package's own definition from the paper (tests/spot_refs.py is its specification), not the reference's spot.py.
    Raises ValueError for q or level outside (0, 1), max_peaks outside [8, 4096] or n_init < 16, and RuntimeError naming the
    column when a column has fewer than 8 excesses, holds a NaN or has a non-positive mean excess."""
    lib = _lib()
    if not (0.0 < q < 1.0) or not (0.0 < level < 1.0):
        raise ValueError(f"q and level must lie in (0, 1), got {q!r}, {level!r}")
    if int(max_peaks) != max_peaks or not 8 <= max_peaks <= 4096:
        raise ValueError(f"max_peaks must be an integer in [8, 4096], got {max_peaks!r}")
    e = _dev2d(init_scores, "init_scores")
    n, S = e.shape
    if n < 16:
        raise ValueError(f"calibration needs at least 16 scores, got {n}")
    nbytes = lib.mtadgat_spot_state_bytes(S, int(max_peaks))
    sbytes = lib.mtadgat_spot_calibrate_scratch(n, S)
    if nbytes == 0 or sbytes == 0:
        raise ValueError(f"{S} columns are refused (at most 65536 per call)")
    buf = _native._empty((nbytes + 7) // 8, dtype=torch.float64, device=e.device)
    buf.zero_()
    scratch = _scratch(sbytes, e.device)
    with torch.cuda.device(e.device):
        rc = lib.mtadgat_spot_calibrate(e.data_ptr(), n, S, e.stride(0), float(q), float(level), int(max_peaks), 1 if dynamic else 0,
                                        buf.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, _stream(e))
    if rc != 0:
        _fail(lib, rc, "spot_calibrate")
    return SpotState(buf, S, max_peaks, q, level, dynamic)


def spot_run(state, scores):
    """The SPOT step over the rows of `scores`, (n,) or (n, S) on the GPU with S = state.n_columns, in order.  Returns (thresholds,
    flags): (n, S) float64 -- what each score was compared against, the column's z BEFORE the step -- and (n, S) uint8
    (score > threshold; NaN is not flagged and changes nothing); 1-D for 1-D scores.  The state is advanced in place, so a second call
    continues where the first stopped; a state calibrated with dynamic=False never changes."""
    lib = _lib()
    if not isinstance(state, SpotState):
        raise TypeError("state must be a SpotState (spot_calibrate)")
    one_d = isinstance(scores, torch.Tensor) and scores.ndim == 1
    x = _dev2d(scores, "scores")
    n, S = x.shape
    if S != state.n_columns or x.device != state.device:
        raise ValueError(f"scores have {S} columns on '{x.device}', the state {state.n_columns} on '{state.device}'")
    thr = _native._empty((n, S), dtype=torch.float64, device=x.device)
    flags = _native._empty((n, S), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.mtadgat_spot_run(state.data_ptr(), S, state.max_peaks, x.data_ptr(), n, x.stride(0), thr.data_ptr(), flags.data_ptr(), _stream(x))
    if rc != 0:
        _fail(lib, rc, "spot_run")
    return (thr.reshape(-1), flags.reshape(-1)) if one_d else (thr, flags)


def pot_eval(init_scores, scores, labels, q=1e-3, level=0.98, dynamic=False, max_peaks=1024):
    """The reference's pot_eval on the device, in epsilon_eval's shape: SPOT calibrated on the 1-D `init_scores` (the training
    scores), applied to `scores`, point-adjusted metrics against `labels` (None: the threshold only).
    Static: the one threshold z of the calibration, through point_adjust_counts.  dynamic (`--dynamic_pot`): the adaptive run's
    flags through the same point-adjust pass, `threshold` being the mean of the per-row thresholds.
    The fit is the package's own definition (see spot_calibrate), so thresholds differ from spot.py's in the last digits."""
    init = _dev1d(init_scores, torch.float32, "init_scores")
    s = _dev1d(scores, torch.float32, "scores")
    state = spot_calibrate(init, q=q, level=level, max_peaks=max_peaks, dynamic=dynamic)
    extra = {"q": q, "level": level, "dynamic": bool(dynamic)}
    if not dynamic:
        z = float(state.read()["z"][0])
        if labels is None:
            return dict(threshold=z, **extra)
        return _result(point_adjust_counts(s, labels, [z])[0], z, **extra)
    thr, flags = spot_run(state, s)
    z = float(thr.mean().item())
    if labels is None:
        return dict(threshold=z, **extra)
    return _result(point_adjust_counts(flags.float(), labels, [0.5])[0], z, **extra)


def predict_anomalies(model, train, test, labels=None, target_dims=None, gamma=1.0, scale_scores=False, use_mov_av=False, reg_level=1,
                      bf_search=None, events=None, pot=None, curves=None, parts=None, prepare=None, mask=None):
    """What Predictor.predict_anomalies (prediction.py:106-165) derives from a train and a test series, with every score array
    staying on the device.  train, test: device-resident (N, F) series; labels: the test labels for rows window_size.. (one
    per score) or None; bf_search: (start, end, step_num) for the best-F1 sweep, run when labels are given too.
    Returns a dict:
      train_scores, test_scores   (N - W,) global scores from model.anomaly_scores with the options given
      test_per_dim                (N_test - W, out_dim) per-dimension scores (scaled if asked, never smoothed)
      feature_thresholds,         feature_predictions(train per-dimension scores, test_per_dim, reg_level)
      feature_preds
      epsilon_result              epsilon_eval(train_scores, test_scores, labels, reg_level), or None without labels
      bf_result                   bf_search(test_scores, labels, *bf_search), or None without labels or bf_search
      events                      only with events=dict(merge_gap=, min_length=, top_k=) (any subset): anomaly_events of test_scores
                                  against find_epsilon(train_scores, reg_level), with test_per_dim, the feature thresholds and the labels
      pot_result                  only with pot=dict(q=, level=, dynamic=) (any subset): pot_eval(train_scores, test_scores, labels, ...),
                                  SPOT calibrated on the training scores; without labels its threshold only
      curve_result                only with curves=dict(adjust=) (or an empty dict): ranking_metrics(test_scores, labels, adjust), or None
                                  without labels
      part_result                 only with parts=dict(..., thresholds="per_part"), see below
    parts=dict(train_lengths=, test_lengths=, transition=, normalize=, thresholds=) (any subset) scores series that are
    concatenations of independent parts (the channels of MSL / SMAP, the machines of SMD) part by part, the reference's
    adjust_anomaly_scores (utils.py:210-255): train_lengths / test_lengths are the parts' row counts (left out: one part),
    transition and normalize as in score_parts and adjust_part_scores.  Train and test scores then come from
    model.anomaly_scores(..., parts=): smoothed per part when use_mov_av, blanked around the seams, min-max normalised per part;
    the per-dimension scores are as without parts, unless scale_scores="per_part": then every series' per-dimension scores are
    scaled by the median and IQR of its own parts (scale_scores(parts=)) instead of the whole series' (scale_scores=True keeps
    meaning that); "per_part" without parts raises ValueError.  thresholds="global" (the default) leaves everything else as it is, now on
    the adjusted scores; "per_part" adds part_result, a dict of
      thresholds   find_epsilon_parts of the train scores -- of the test scores when train and test differ in their number of parts
      preds        part_predictions(test_scores, ...): (n,) uint8 on the device
      f1, precision, recall, TP, TN, FP, FN, latency      with labels: the point-adjusted counts of those flags
    Three departures from the reference, whose own function could not be run here to pin it (tests/part_refs.py is the specification):
    a constant part maps to 0 where the reference has 0 / 0; the parts are half-open where the reference's slices share a sample
    that is normalised twice; the moving average restarts per part where the reference smooths across the seams.  Events
    (events=) may still merge across a seam; with both sides blanked that takes merge_gap >= before + after.
    Without parts every returned value is what it was before parts existed.
    prepare=dict(fill=, clip=, gaps=) (any subset; defaults "zero", False, "zero": the reference's normalize_data) takes train and
    test as RAW series: a preparation.SeriesScaler is fitted on train (fit_scaler(train, gaps)) and both series go through its
    transform(fill=, clip=) before anything else, a "hold" fill stopping at the seams of parts' train_lengths / test_lengths when
    those are given; the result gains "scaler".  Without prepare nothing changes.
    mask=dict(max_age=, min_observed=) (any subset; defaults 0 and 0.5) keeps filled samples out of scores and thresholds.  It
    needs prepare=: both transforms then run with return_age=True, train and test scores come from
    model.anomaly_scores(..., age=, max_age=, min_observed=) -- a score exists exactly where a training window would have been drawn,
    NaN elsewhere --, and every threshold is computed with skip_nan.  The result gains train_scored and test_scored, uint8 on the
    device: 1 where the score exists.  mask without prepare, or together with parts, pot or curves, raises ValueError: per-part
    masked scoring is not covered, and SPOT's and the ranking sort's treatment of unscored rows is not defined.  With events=: a NaN
    is never flagged, so an unscored row ends a run unless merge_gap bridges it; and by run_statistics' rule a run that contains an
    unscored row has a NaN mean_score."""
    mask_opts = None
    if mask is not None:
        unknown = set(mask) - {"max_age", "min_observed"}
        if unknown:
            raise ValueError(f"mask takes max_age and min_observed, got {sorted(unknown)}")
        if prepare is None:
            raise ValueError("mask needs prepare=: the ages of the filled samples come from the preparation's transform")
        for name, other in (("parts", parts), ("pot", pot), ("curves", curves)):
            if other is not None:
                raise ValueError(f"mask together with {name}= is not supported: " + (
                    "per-part masked scoring is not covered" if name == "parts" else
                    "SPOT's treatment of unscored rows is not defined" if name == "pot" else
                    "the ranking curves' treatment of unscored rows is not defined"))
        mask_opts = dict(max_age=0, min_observed=0.5)
        mask_opts.update(mask)
    scaler = None
    if prepare is not None and mask_opts is not None:
        import preparation
        unknown = set(prepare) - {"fill", "clip", "gaps"}
        if unknown:
            raise ValueError(f"prepare takes fill, clip and gaps, got {sorted(unknown)}")
        prep_opts = dict(fill="zero", clip=False, gaps="zero")
        prep_opts.update(prepare)
        scaler = preparation.fit_scaler(train, gaps=prep_opts["gaps"])
        train, train_age = scaler.transform(train, fill=prep_opts["fill"], clip=prep_opts["clip"], return_age=True)
        test, test_age = scaler.transform(test, fill=prep_opts["fill"], clip=prep_opts["clip"], return_age=True)
    elif prepare is not None:
        import preparation
        unknown = set(prepare) - {"fill", "clip", "gaps"}
        if unknown:
            raise ValueError(f"prepare takes fill, clip and gaps, got {sorted(unknown)}")
        prep_opts = dict(fill="zero", clip=False, gaps="zero")
        prep_opts.update(prepare)
        scaler = preparation.fit_scaler(train, gaps=prep_opts["gaps"])
        seams = parts or {}
        train = scaler.transform(train, fill=prep_opts["fill"], clip=prep_opts["clip"], lengths=seams.get("train_lengths"))
        test = scaler.transform(test, fill=prep_opts["fill"], clip=prep_opts["clip"], lengths=seams.get("test_lengths"))
    part_opts = None
    if isinstance(scale_scores, str) and scale_scores != "per_part":
        raise ValueError(f"scale_scores must be False, True or 'per_part', got {scale_scores!r}")
    if isinstance(scale_scores, str) and parts is None:
        raise ValueError("scale_scores='per_part' needs parts=")
    if parts is not None:
        unknown = set(parts) - {"train_lengths", "test_lengths", "transition", "normalize", "thresholds"}
        if unknown:
            raise ValueError(f"parts takes train_lengths, test_lengths, transition, normalize and thresholds, got {sorted(unknown)}")
        part_opts = dict(transition=(19, 19), normalize=True, thresholds="global", train_lengths=None, test_lengths=None)
        part_opts.update(parts)
        if part_opts["thresholds"] not in ("global", "per_part"):
            raise ValueError(f"parts' thresholds must be 'global' or 'per_part', got {part_opts['thresholds']!r}")
    score_kw = dict(target_dims=target_dims, gamma=gamma, scale_scores=scale_scores, use_mov_av=use_mov_av)
    skip = mask_opts is not None
    if skip:
        train_scores, train_per_dim = model.anomaly_scores(train, age=train_age, **mask_opts, **score_kw)
        test_scores, test_per_dim = model.anomaly_scores(test, age=test_age, **mask_opts, **score_kw)
    elif part_opts is None:
        train_scores, train_per_dim = model.anomaly_scores(train, **score_kw)
        test_scores, test_per_dim = model.anomaly_scores(test, **score_kw)
    else:
        def described(values, lengths):
            return score_parts([values.shape[0]] if lengths is None else lengths, model.window_size, part_opts["transition"], values.device)
        train_parts, test_parts = described(train, part_opts["train_lengths"]), described(test, part_opts["test_lengths"])
        for name, values, sp in (("train", train, train_parts), ("test", test, test_parts)):
            if sp.n != values.shape[0] - model.window_size:
                raise ValueError(f"{name}_lengths add up to {sp.n + model.window_size} rows, the {name} series has {values.shape[0]}")
        train_scores, train_per_dim = model.anomaly_scores(train, parts=train_parts, normalize_parts=part_opts["normalize"], **score_kw)
        test_scores, test_per_dim = model.anomaly_scores(test, parts=test_parts, normalize_parts=part_opts["normalize"], **score_kw)
    eps_result = bf_result = None
    if labels is not None:
        eps_result = epsilon_eval(train_scores, test_scores, labels, reg_level, **({"skip_nan": True} if skip else {}))
        if bf_search is not None:
            start, end, step_num = bf_search
            bf_result = _sweep(test_scores, labels, start, end, step_num)
    thr, preds = feature_predictions(train_per_dim, test_per_dim, reg_level, **({"skip_nan": True} if skip else {}))
    out = {"epsilon_result": eps_result, "bf_result": bf_result, "feature_thresholds": thr, "train_scores": train_scores,
           "test_scores": test_scores, "test_per_dim": test_per_dim, "feature_preds": preds}
    if scaler is not None:
        out["scaler"] = scaler
    if skip:
        # (a score is NaN exactly where it does not exist: finite model outputs give finite scores at the rows that are kept)
        out["train_scored"] = scored_rows(train.shape[0], model.window_size, train.shape[1], train_age, target_dims=target_dims, **mask_opts)
        out["test_scored"] = scored_rows(test.shape[0], model.window_size, test.shape[1], test_age, target_dims=target_dims, **mask_opts)
    if part_opts is not None and part_opts["thresholds"] == "per_part":
        same = train_parts.n_parts == test_parts.n_parts
        part_thr = find_epsilon_parts(train_scores, train_parts, reg_level) if same else find_epsilon_parts(test_scores, test_parts, reg_level)
        part_preds = part_predictions(test_scores, test_parts, part_thr)
        out["part_result"] = {"thresholds": part_thr, "preds": part_preds}
        if labels is not None:
            metrics = _result(point_adjust_counts(part_preds.float(), labels, [0.5])[0], None)
            del metrics["threshold"]
            out["part_result"].update(metrics)
    if pot is not None:
        unknown = set(pot) - {"q", "level", "dynamic"}
        if unknown:
            raise ValueError(f"pot takes q, level and dynamic, got {sorted(unknown)}")
        out["pot_result"] = pot_eval(train_scores, test_scores, labels, **pot)
    if curves is not None:
        unknown = set(curves) - {"adjust"}
        if unknown:
            raise ValueError(f"curves takes adjust, got {sorted(unknown)}")
        out["curve_result"] = ranking_metrics(test_scores, labels, **curves) if labels is not None else None
    if events is not None:
        unknown = set(events) - {"merge_gap", "min_length", "top_k"}
        if unknown:
            raise ValueError(f"events takes merge_gap, min_length and top_k, got {sorted(unknown)}")
        eps = eps_result["threshold"] if eps_result is not None else find_epsilon(train_scores, reg_level, **({"skip_nan": True} if skip else {}))
        out["events"] = anomaly_events(test_scores, eps, per_dim=test_per_dim, feature_thresholds=thr, labels=labels, **events)
    return out


# ---- events ----------------------------------------------------------------------------------------------------------------------
RUNS_CHUNK = 1024        # chunk length of the run-extraction scans (mtadgat_eval_runs_chunk(); tests pick sizes around it)

_c_int64_p = ctypes.POINTER(ctypes.c_int64)


def _labels_u8(label, name="labels"):
    """Labels as point_adjust_counts reads them: bool as it is, numbers as label > 0.1 -- which for uint8 is label != 0, what the
    kernels test: a uint8 tensor is handed on unchanged."""
    if not isinstance(label, torch.Tensor) or label.device.type != "cuda":
        raise RuntimeError(f"{name} must be a tensor on the GPU (the evaluation kernels are HIP only)")
    return _dev1d(label if label.dtype in (torch.bool, torch.uint8) else (label > 0.1), torch.uint8, name)


def _flag_source(scores, labels):
    if (scores is None) == (labels is None):
        raise ValueError("give scores or labels, not both")
    if scores is not None:
        return _dev1d(scores, torch.float32, "scores"), None
    return None, _labels_u8(labels)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def flag_runs(scores=None, labels=None, threshold=0.0, merge_gap=0, min_length=1, compare_f32=False, max_runs=65536):
    """The maximal runs of flagged samples as (count, start, end): `count` a Python int, start / end (count,) int64 on the device,
    ascending, end exclusive.  flag_i = scores_i > threshold (compared in float64 like a float32 array against a Python float, or
    in float32 with compare_f32; NaN and equality are not flagged), or labels_i set.  Runs separated by at most merge_gap samples
    are merged (chains; the gap belongs to the event), then events shorter than min_length are dropped.  max_runs sizes the
    first attempt only: when there are more, the call is repeated once with the count the library reported."""
    lib = _lib()
    s, lab = _flag_source(scores, labels)
    src = s if s is not None else lab
    n = src.numel()
    if n < 1:
        raise ValueError("the flag source is empty")
    if merge_gap < 0 or min_length < 1 or max_runs < 1:
        raise ValueError(f"needs merge_gap >= 0, min_length >= 1, max_runs >= 1, got {merge_gap}, {min_length}, {max_runs}")
    scratch = _scratch(lib.mtadgat_eval_runs_scratch(n), src.device)
    count = ctypes.c_int64(0)
    cap = int(max_runs)
    for attempt in range(2):
        start = _native._empty(cap, dtype=torch.int64, device=src.device)
        end = _native._empty(cap, dtype=torch.int64, device=src.device)
        with torch.cuda.device(src.device):
            rc = lib.mtadgat_eval_runs(_ptr(s), _ptr(lab), n, float(threshold), 1 if compare_f32 else 0, int(merge_gap), int(min_length), cap,
                                       scratch.data_ptr(), scratch.numel() * 8, start.data_ptr(), end.data_ptr(), ctypes.byref(count),
                                       _stream(src))
        if rc == -5 and attempt == 0 and count.value > cap:
            cap = count.value
            continue
        if rc != 0:
            _fail(lib, rc, "eval_runs")
        break
    return count.value, start[:count.value], end[:count.value]


def _runs(start, end, device):
    st, en = _dev1d(start, torch.int64, "start"), _dev1d(end, torch.int64, "end")
    if st.numel() != en.numel() or st.device != device or en.device != device:
        raise ValueError("start and end must have the same length and live on the device of the scores")
    return st, en


def run_statistics(scores, start, end, per_dim=None, feature_thresholds=None, top_k=5):
    """Per-run reductions over the runs [start_k, end_k) of flag_runs: a dict of device tensors
      peak (int64), peak_score   the first index attaining the run's maximum score (NaN read as -inf), and that score
      mean_score                 float64 sum / length, stored as float32
      feature_means (E, d), top_features (E, k) int32, top_values (E, k)      with per_dim (n, d): the column means of the run and
                                 its k = min(top_k, d, 64) largest (descending, ties to the lower column, NaN last)
      feature_hits (E, d) int32  with feature_thresholds (d,): the run's rows with per_dim >= threshold, compared in float64
    Bitwise reproducible; nothing is copied to the host."""
    lib = _lib()
    s = _dev1d(scores, torch.float32, "scores")
    n, dev = s.numel(), s.device
    st, en = _runs(start, end, dev)
    count = st.numel()
    pd, thr, d, ld, k = None, None, 0, 0, 0
    if per_dim is not None:
        pd = _dev2d(per_dim, "per_dim")
        if pd.device != dev or pd.shape[0] != n:
            raise ValueError(f"per_dim must hold one row per score on the same device, got {tuple(pd.shape)} for {n} scores")
        d, ld = pd.shape[1], pd.stride(0)
        if top_k < 1:
            raise ValueError(f"top_k must be >= 1, got {top_k}")
        k = min(int(top_k), d, 64)
        if feature_thresholds is not None:
            thr = torch.as_tensor(feature_thresholds, dtype=torch.float64).reshape(-1).to(dev).contiguous()
            if thr.numel() != d:
                raise ValueError(f"{thr.numel()} feature thresholds for {d} columns")
    elif feature_thresholds is not None:
        raise ValueError("feature_thresholds need per_dim")
    peak = _native._empty(count, dtype=torch.int64, device=dev)
    peak_score = _native._empty(count, dtype=torch.float32, device=dev)
    mean_score = _native._empty(count, dtype=torch.float32, device=dev)
    out = {"peak": peak, "peak_score": peak_score, "mean_score": mean_score}
    if pd is not None:
        feature_means = _native._empty((count, d), dtype=torch.float32, device=dev)
        top_features = _native._empty((count, k), dtype=torch.int32, device=dev)
        top_values = _native._empty((count, k), dtype=torch.float32, device=dev)
        out.update(feature_means=feature_means, top_features=top_features, top_values=top_values)
    if thr is not None:
        feature_hits = _native._empty((count, d), dtype=torch.int32, device=dev)
        out["feature_hits"] = feature_hits
    if count == 0:
        return out
    scratch = _scratch(lib.mtadgat_eval_run_stats_scratch(n, count, d), dev)
    with torch.cuda.device(dev):
        rc = lib.mtadgat_eval_run_stats(s.data_ptr(), n, st.data_ptr(), en.data_ptr(), count, _ptr(pd), d, ld, _ptr(thr), k, scratch.data_ptr(),
                                        scratch.numel() * 8, out["peak"].data_ptr(), out["peak_score"].data_ptr(), out["mean_score"].data_ptr(),
                                        _ptr(out.get("feature_means")), _ptr(out.get("top_features")), _ptr(out.get("top_values")),
                                        _ptr(out.get("feature_hits")), _stream(s))
    if rc != 0:
        _fail(lib, rc, "eval_run_stats")
    return out


def first_hits(start, end, scores=None, labels=None, threshold=0.0, compare_f32=False):
    """The first flagged index inside every run [start_k, end_k), or -1: (E,) int64 on the device.  The flag source is read as in
    flag_runs.  Scores against labelled segments: where each segment was detected; labels against events: which events are true."""
    lib = _lib()
    s, lab = _flag_source(scores, labels)
    src = s if s is not None else lab
    st, en = _runs(start, end, src.device)
    first = _native._empty(st.numel(), dtype=torch.int64, device=src.device)
    if st.numel() == 0:
        return first
    if src.numel() < 1:
        raise ValueError("the flag source is empty")
    with torch.cuda.device(src.device):
        rc = lib.mtadgat_eval_first_hit(_ptr(s), _ptr(lab), src.numel(), float(threshold), 1 if compare_f32 else 0, st.data_ptr(), en.data_ptr(),
                                        st.numel(), first.data_ptr(), _stream(src))
    if rc != 0:
        _fail(lib, rc, "eval_first_hit")
    return first


def anomaly_events(scores, threshold, per_dim=None, feature_thresholds=None, labels=None, merge_gap=0, min_length=1, top_k=5,
                   compare_f32=False, max_events=65536):
    """The alarms behind a thresholded score array: the contiguous stretches with scores > threshold, merged across gaps of at
    most merge_gap samples and kept from min_length samples on, each with its peak, its means and the features that carry it.
    Everything is computed on the device (csrc/mtadgat_events.hip); only the number of events comes to the host.

    Indices are in score-index space: event [start, end) covers scores[start:end], and score i belongs to row i + W of the series
    the windows were cut from (W = window_size).  `peak` is therefore what `model.score_attribution(values, indices)` takes.

    Returns a dict:
      count                                  Python int; threshold: the float compared against
      start, end, peak                       (E,) int64; peak_score, mean_score (E,) float32    (flag_runs, run_statistics)
      feature_means, top_features, top_values   with per_dim (n, d): (E, d), (E, k) int32, (E, k), k = min(top_k, d, 64)
      feature_hits                           with feature_thresholds (d,) too: (E, d) int32 rows with per_dim >= threshold
      event_is_true                          with labels (n,): (E,) bool, the event overlaps a labelled sample
      segments                               with labels: dict of start, end (the labelled runs), first_hit (the first sample of the
                                             segment with scores > threshold, -1 if none) and latency = first_hit - start (-1 if
                                             undetected), all (S,) int64 -- the per-segment view of point_adjust_counts
    No events gives empty tensors of these shapes.  max_events sizes the first attempt; more events cost one repeat."""
    s = _dev1d(scores, torch.float32, "scores")
    count, start, end = flag_runs(scores=s, threshold=threshold, merge_gap=merge_gap, min_length=min_length, compare_f32=compare_f32,
                                  max_runs=max_events)
    out = {"count": count, "threshold": float(threshold), "start": start, "end": end}
    out.update(run_statistics(s, start, end, per_dim=per_dim, feature_thresholds=feature_thresholds if per_dim is not None else None,
                              top_k=top_k))
    if labels is not None:
        lab = _labels_u8(labels)
        if lab.numel() != s.numel():
            raise ValueError("scores and labels must have the same length")
        out["event_is_true"] = first_hits(start, end, labels=lab) >= 0
        _, seg_start, seg_end = flag_runs(labels=lab, max_runs=max_events)
        hit = first_hits(seg_start, seg_end, scores=s, threshold=threshold, compare_f32=compare_f32)
        out["segments"] = {"start": seg_start, "end": seg_end, "first_hit": hit, "latency": torch.where(hit >= 0, hit - seg_start, hit)}
    return out


def explain_events(model, values, events, which=None, max_events=64, **attribution_kwargs):
    """Attribution of the events' peak scores to the input: model.score_attribution(values, events["peak"][which], ...) and its two
    marginals.  `which` selects events (None: all; an index, slice, list or tensor); every selected peak costs two training
    forwards, so more than max_events of them is an error rather than a long wait.
    Returns a dict: peaks (E',) int64, attributions (E', W+1, F), per_feature (E', F) = |attributions| summed over the W+1 rows,
    per_lag (E', W+1) = summed over the features."""
    peaks = events["peak"]
    if which is not None:
        peaks = peaks[which]
    peaks = peaks.reshape(-1)
    if peaks.numel() > max_events:
        raise ValueError(f"{peaks.numel()} events selected, max_events is {max_events}: pick some with `which` or raise max_events")
    attr = model.score_attribution(values, peaks, **attribution_kwargs)
    mag = attr.abs()
    return {"peaks": peaks, "attributions": attr, "per_feature": mag.sum(1), "per_lag": mag.sum(2)}


# ---- ranking curves ----------------------------------------------------------------------------------------------------------------
def score_order(scores, descending=True):
    """The indices of a 1-D float32 GPU tensor in rank order, (n,) int64 on the device: largest first (or smallest first), ties in
    ascending index, -0.0 and +0.0 one value, +-inf ordinary values, NaNs last in both directions in index order.  A stable
    radix sort without atomics: bitwise reproducible, any 1 <= n < 2**31."""
    lib = _lib()
    s = _dev1d(scores, torch.float32, "scores")
    n = s.numel()
    if n < 1:
        raise ValueError("scores is empty")
    nbytes = lib.mtadgat_eval_score_order_scratch(n)
    if nbytes == 0:
        raise ValueError(f"{n} scores are refused (fewer than 2**31)")
    scratch = _scratch(nbytes, s.device)
    order = _native._empty(n, dtype=torch.int64, device=s.device)
    with torch.cuda.device(s.device):
        rc = lib.mtadgat_eval_score_order(s.data_ptr(), n, 1 if descending else 0, scratch.data_ptr(), scratch.numel() * 8, order.data_ptr(),
                                          _stream(s))
    if rc != 0:
        _fail(lib, rc, "eval_score_order")
    return order


def _adjust_code(adjust):
    """(mode, K) of the library for adjust = None | "point" | ("k", K)."""
    if adjust is None:
        return 0, 0
    if isinstance(adjust, str):
        if adjust == "point":
            return 1, 0
    elif isinstance(adjust, (tuple, list)) and len(adjust) == 2 and adjust[0] == "k":
        k = adjust[1]
        if isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 0 <= k <= 100:
            return 2, int(k)
        raise ValueError(f"K of ('k', K) must be an integer in [0, 100], got {k!r}")
    raise ValueError(f"adjust must be None, 'point' or ('k', K), got {adjust!r}")


_CURVE_SUMMARY = 12      # int64 the library copies back: G, n_pos, n_neg, nan_pos, nan_neg, 2 x AUROC numerator, AP sum, best ...


def _curve(scores, labels, adjust):
    lib = _lib()
    s = _dev1d(scores, torch.float32, "scores")
    lab = _labels_u8(labels)
    mode, k = _adjust_code(adjust)
    n = s.numel()
    if n < 1:
        raise ValueError("scores is empty")
    if lab.numel() != n or lab.device != s.device:
        raise ValueError("scores and labels must have the same length and live on the same device")
    nbytes = lib.mtadgat_eval_curve_scratch(n, mode)
    if nbytes == 0:
        raise ValueError(f"{n} scores are refused (fewer than 2**31)")
    scratch = _scratch(nbytes, s.device)
    thr = _native._empty(n, dtype=torch.float32, device=s.device)
    tp = _native._empty(n, dtype=torch.int64, device=s.device)
    fp = _native._empty(n, dtype=torch.int64, device=s.device)
    summary = (ctypes.c_int64 * _CURVE_SUMMARY)()
    with torch.cuda.device(s.device):
        rc = lib.mtadgat_eval_curve(s.data_ptr(), lab.data_ptr(), n, mode, k, scratch.data_ptr(), scratch.numel() * 8, thr.data_ptr(),
                                    tp.data_ptr(), fp.data_ptr(), summary, _stream(s))
    if rc != 0:
        _fail(lib, rc, "eval_curve")
    g = summary[0]
    thr, tp, fp = thr[:g], tp[:g], fp[:g]
    if 2 * g <= n:          # few distinct values: do not keep the n-entry buffers alive behind the views
        thr, tp, fp = thr.clone(), tp.clone(), fp.clone()
    return s, lab, thr, tp, fp, list(summary)


def ranking_curve(scores, labels, adjust=None):
    """Every operating point of a score array against labels (read as point_adjust_counts reads them): a dict of
      thresholds        (G,) float32 on the device: the distinct non-NaN values of the adjusted scores, descending
      tp, fp            (G,) int64: the positives / negatives with adjusted score >= thresholds[g]
      n_pos, n_neg, nan_pos, nan_neg     Python ints; a NaN score is never flagged: a false or true negative at every threshold
    adjust=None ranks the scores as they are (-0.0 read as +0.0); "point" gives every sample of a labelled segment the segment's
    largest non-NaN score (sample 0 of a segment that starts at index 0 keeps its own: adjust_predicts' back-fill never reaches
    index 0), so that point g equals point_adjust_counts at the float32 just below thresholds[g]; ("k", K) is PA%K: a sample of a
    segment of length L takes max(own, the m-th largest non-NaN score of the segment), m = K * L // 100 + 1, and keeps its own when
    the segment has fewer than m non-NaN scores.  The scores are adjusted, sorted and scanned on the device; the counts are the only
    values read back.  Bitwise reproducible."""
    _, _, thr, tp, fp, summary = _curve(scores, labels, adjust)
    return {"thresholds": thr, "tp": tp, "fp": fp, "n_pos": summary[1], "n_neg": summary[2], "nan_pos": summary[3], "nan_neg": summary[4]}


def ranking_metrics(scores, labels, adjust=None):
    """Threshold-free quality of a score array under ranking_curve's `adjust`: a dict of Python numbers
      auroc               area under the ROC curve, ties joined by straight lines, the NaN samples one last tie group; an exact
                          integer numerator from the device over 2 n_pos n_neg; NaN when a class is empty
      average_precision   sum over the tie groups of (positives of the group) x precision at the group / n_pos (scikit-learn's)
      best                the curve point of largest F1 (the reference's 1e-5 guards; the highest threshold among equals), chosen on
                          the device, in epsilon_eval's shape: f1, precision, recall, TP, TN, FP, FN, threshold -- flagged means
                          adjusted score >= threshold -- and with adjust="point" the latency of point_adjust_counts just below that
                          threshold (None at threshold -inf, below which no float32 lies); None when every score is NaN
      best_index          its position in ranking_curve's arrays (None with best)
      n_thresholds, n_pos, n_neg, adjust"""
    s, lab, _, _, _, summary = _curve(scores, labels, adjust)
    g, n_pos, n_neg, nan_pos, nan_neg, auc2, ap_bits, best, best_tp, best_fp, thr_bits = summary[:11]
    auroc = auc2 / (2 * n_pos * n_neg) if n_pos and n_neg else float("nan")
    ap_sum = float(np.array([ap_bits], dtype=np.int64).view(np.float64)[0])
    out = {"auroc": auroc, "average_precision": ap_sum / n_pos if n_pos else float("nan"), "best": None, "best_index": None, "n_thresholds": g,
           "n_pos": n_pos, "n_neg": n_neg, "adjust": adjust}
    if best >= 0:
        v = float(np.array([thr_bits], dtype=np.uint32).view(np.float32)[0])
        counts = [float(best_tp), float(n_neg - best_fp), float(best_fp), float(n_pos - best_tp)]
        f1, prec, rec = _scores_from_counts(*counts)
        res = {"f1": f1, "precision": prec, "recall": rec, "TP": counts[0], "TN": counts[1], "FP": counts[2], "FN": counts[3], "threshold": v}
        if adjust == "point":
            below = float(np.nextafter(np.float32(v), np.float32(-np.inf)))
            row = None
            if v > -math.inf:           # no float32 lies below -inf: `> below` cannot flag what `>= v` flags
                row = point_adjust_counts(s, lab, [below], compare_f32=True, max_segments=max(65536, (s.numel() + 1) // 2))[0]
            if row is not None and (row[0] != counts[0] or row[2] != counts[2]):
                raise RuntimeError(f"the curve's best point (TP {counts[0]}, FP {counts[2]}) differs from point_adjust_counts' "
                                   f"(TP {row[0]}, FP {row[2]}) at threshold {below!r}")
            res["latency"] = row[4] / (row[5] + 1e-4) if row is not None else None
        out["best"], out["best_index"] = res, best
    return out


# ---- forecast / reconstruction losses of a series (csrc/mtadgat_losses.hip; tests/loss_refs.py is the specification) ---------------
def _target_dims(target_dims, out_dim, n_features):
    """The series columns the out_dim outputs are compared with, checked as MTAD_GAT.score_attribution checks them."""
    dims = list(range(n_features)) if target_dims is None else ([target_dims] if isinstance(target_dims, int) else [int(d) for d in target_dims])
    if len(dims) != out_dim:
        raise RuntimeError(f"target_dims select {len(dims)} columns but the model has out_dim={out_dim}")
    if any(d < 0 or d >= n_features for d in dims):
        raise IndexError(f"target_dims must lie in [0, {n_features})")
    return dims


def window_sse(preds, recons, series, starts=None, start=0, stride=1, dims=None):
    """Squared errors of model outputs the caller already has against the series their windows were cut from.  preds (n, out) and
    recons (n, W, out) are the outputs for the windows w = series[s_w : s_w + W], s_w = starts[w] or start + w * stride; output
    dimension d is compared with series column dims[d] (None: d).  Returns (window_sse (n, 2), dim_sse (2, out)), float64 on the
    device: window_sse[w, 0] = sum_d (preds[w, d] - series[s_w + W, dims[d]])^2, window_sse[w, 1] = sum_{t, d} (recons[w, t, d] -
    series[s_w + t, dims[d]])^2, dim_sse the same squares summed over the windows (and time steps) instead of over d.  Every
    difference is one float32 subtraction, squared and summed in float64 in a fixed order without atomics: a window's pair
    depends on that window alone, identical calls give identical bits."""
    lib = _lib()
    if preds.ndim != 2 or recons.ndim != 3 or recons.shape[0] != preds.shape[0] or recons.shape[2] != preds.shape[1]:
        raise ValueError(f"preds {tuple(preds.shape)} / recons {tuple(recons.shape)} are not (n, out) / (n, W, out)")
    n, W, out = recons.shape
    if n < 1:
        raise ValueError("window_sse needs at least one window")
    ser = _dev2d(series, "series")
    if preds.device != ser.device or recons.device != ser.device:
        raise RuntimeError("preds, recons and series must be on the same GPU")
    n_rows, F = ser.shape
    dims_t = None
    if dims is not None:
        dims_t = torch.tensor(_target_dims(dims, out, F), dtype=torch.int32, device=ser.device)
    elif out > F:
        raise RuntimeError("out_dim exceeds the number of series columns: pass dims")
    st = None
    if starts is not None:
        st = _dev1d(starts, torch.int64, "starts")
        if st.numel() != n:
            raise ValueError(f"starts holds {st.numel()} windows, the outputs {n}")
        if int(st.min()) < 0 or int(st.max()) + W > n_rows - 1:
            raise RuntimeError("a window or its target row does not lie inside the series")
    p, r = preds.detach().float().contiguous(), recons.detach().float().contiguous()
    wsse = _native._empty((n, 2), dtype=torch.float64, device=ser.device)
    dsse = _native._empty((2, out), dtype=torch.float64, device=ser.device)
    need = lib.mtadgat_eval_window_sse_scratch(n, out)
    if need == 0:
        raise ValueError(f"window_sse: sizes outside the kernel's limits (n = {n}, out_dim = {out})")
    scratch = _scratch(need, ser.device)
    with torch.cuda.device(ser.device):
        rc = lib.mtadgat_eval_window_sse(p.data_ptr(), r.data_ptr(), n, W, out, ser.data_ptr(), n_rows, F, ser.stride(0),
                                         st.data_ptr() if st is not None else None, int(start), int(stride),
                                         dims_t.data_ptr() if dims_t is not None else None, 0, wsse.data_ptr(), dsse.data_ptr(),
                                         scratch.data_ptr(), need, _stream(ser))
    if rc:
        _fail(lib, rc, "eval_window_sse")
    return wsse, dsse


def _ordered_sums(x):
    """The fixed-order sum over the rows of x (m, cols) float64 that k_group_sums computes: lane t of 256 adds rows t, t + 256, ..
    in order, then the lanes meet in a halving tree (mtadgat_scan.h: block_sum)."""
    lanes = np.zeros((256, x.shape[1]), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(0, x.shape[0], 256):
            blk = x[j:j + 256]
            lanes[:blk.shape[0]] += blk
        s = 128
        while s:
            lanes[:s] += lanes[s:2 * s]
            s //= 2
    return lanes[0].copy()


def group_sums(x, group):
    """Sums of consecutive groups of `group` rows of x (n, cols) float64 -- the last group may be short -- in a fixed order:
    (ceil(n / group), cols) float64 on x's device (GPU: mtadgat_eval_group_sums; CPU: the same order in numpy)."""
    if x.ndim != 2 or x.shape[0] < 1 or x.dtype != torch.float64:
        raise ValueError(f"x must be a float64 (n, cols) tensor with n >= 1, got {tuple(x.shape)} {x.dtype}")
    group = int(group)
    if group < 1:
        raise ValueError(f"group must be >= 1, got {group}")
    n, cols = x.shape
    G = (n + group - 1) // group
    if x.device.type != "cuda":
        xn = x.detach().contiguous().numpy()
        return torch.from_numpy(np.stack([_ordered_sums(xn[i:i + group]) for i in range(0, n, group)]))
    lib = _lib()
    xc = x.detach().contiguous()
    out = _native._empty((G, cols), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.mtadgat_eval_group_sums(xc.data_ptr(), n, cols, group, out.data_ptr(), _stream(xc))
    if rc:
        _fail(lib, rc, "eval_group_sums")
    return out


def group_losses(sums, n, W, out, batch_size=None):
    """(forecast_loss, recon_loss, total_loss) from the (G, 2) host sums of group_sums(window_sse, batch_size or n) over n windows:
    per group its two MSEs, then sqrt(mean over the groups) -- Trainer.evaluate's epoch value, in which a short last batch
    weighs as much as a full one; one group gives the global RMSEs."""
    sums = np.asarray(sums, dtype=np.float64)
    b = n if batch_size is None else int(batch_size)
    counts = np.array([min(b, n - i) for i in range(0, n, b)], dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = float(np.sqrt((sums[:, 0] / (counts * out)).mean()))
        r = float(np.sqrt((sums[:, 1] / (counts * W * out)).mean()))
    return f, r, f + r
