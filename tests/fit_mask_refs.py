"""The specification of training on gappy, concatenated series (fitting.training_windows, SeriesTrainer.step / fit with `age`,
MTAD_GAT.series_losses with `age`; the mtadgat_fit_windows, mtadgat_fit_masked_sse, mtadgat_fit_masked_loss_grad and
mtadgat_series_losses_masked entry points), in plain numpy on tests/loss_refs.py and tests/fit_refs.py.  Imports nothing of the package.

age (N, F) integers as the preparation reports them: 0 for a real sample, k for the k-th consecutive filled row.  A sample is
OBSERVED iff age <= max_age.  The series is `lengths` parts laid end to end.  Window s reads rows s .. s + W - 1 and is asked for
row s + W; output dimension d is compared with column dims[d].

  windows       the starts s in [0, N - W), ascending, with (1) rows s .. s + W in one part, (2) an observed sample in row s + W among
                the columns dims, (3) at least min_count observed samples in rows s .. s + W - 1 over all F columns.
  window_sums   per window (S_f, S_r, N_f, N_r): loss_refs.squares with every unobserved term replaced by +0.0 -- a select, so a NaN
                under the mask does not reach the sum --, summed as loss_refs.window_sse sums them, and the number of observed terms.
  loss_grad     from the batch's four sums (loss_refs.ordered_sum over window_sums), per head in float64:
                rmse = sqrt(S / N) for N > 0 else 0;  c = NaN if S is not finite, 0 if N == 0 or rmse == 0, else 1 / (N rmse);
                an observed entry gets store(float64(df) c) with df the ONE float32 subtraction, an unobserved one +0.0.
                It is the gradient of sqrt(sum m r^2 / sum m) + sqrt(sum m r^2 / sum m), heads with rmse == 0 taken as 0.
  group_losses  per group of batch_size windows mse = S_g / N_g; groups with N_g == 0 are left out; sqrt(mean) per head, NaN when no
                group is left."""
import numpy as np

import loss_refs


def part_offsets(lengths, n_rows):
    offs = np.concatenate([[0], np.cumsum(np.asarray([n_rows] if lengths is None else lengths, dtype=np.int64))])
    assert offs[-1] == n_rows
    return offs


def observed(age, max_age, shape=None):
    """The boolean (N, F) mask of observed samples; age None: all of `shape`."""
    return np.ones(shape, dtype=bool) if age is None else np.asarray(age) <= max_age


def rule_masks(n_rows, W, F, lengths=None, age=None, max_age=0, dims=None, min_count=0):
    """(same_part, target_seen, enough) boolean arrays over the starts 0 .. n_rows - W - 1: the three rules one by one."""
    obs = observed(age, max_age, (n_rows, F))
    cols = np.arange(F) if dims is None else np.asarray(dims, dtype=np.int64).reshape(-1)
    offs = part_offsets(lengths, n_rows)
    n = max(n_rows - W, 0)
    s = np.arange(n, dtype=np.int64)
    part = np.searchsorted(offs, s, side="right") - 1                    # the part whose rows hold s (empty parts are skipped)
    same_part = s + W < offs[part + 1]
    target_seen = obs[s + W][:, cols].any(axis=1) if n else np.zeros(0, dtype=bool)
    prefix = np.concatenate([[0], np.cumsum(obs.sum(axis=1).astype(np.int64))])
    enough = prefix[s + W] - prefix[s] >= min_count
    return same_part, target_seen, enough


def windows(n_rows, W, F, lengths=None, age=None, max_age=0, dims=None, min_count=0):
    """The valid starts, ascending, int64."""
    a, b, c = rule_masks(n_rows, W, F, lengths, age, max_age, dims, min_count)
    return np.nonzero(a & b & c)[0].astype(np.int64)


def _masks(age, max_age, starts, W, cols):
    obs = np.asarray(age) <= max_age
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    return obs[starts + W][:, cols], obs[starts[:, None] + np.arange(W)[None, :]][:, :, cols]


def window_sums(preds, recons, series, starts, age, max_age=0, dims=None):
    """(n, 4) float64: S_f, S_r, N_f, N_r per window."""
    qf, qr = loss_refs.squares(preds, recons, series, starts, dims)
    cols = loss_refs._dims(dims, qf.shape[1])
    mf, mr = _masks(age, max_age, starts, recons.shape[1], cols)
    qf, qr = np.where(mf, qf, 0.0), np.where(mr, qr, 0.0)
    n = qf.shape[0]
    return np.stack([qf.sum(axis=1), qr.reshape(n, -1).sum(axis=1), mf.sum(axis=1).astype(np.float64),
                     mr.reshape(n, -1).sum(axis=1).astype(np.float64)], axis=1)


def dim_sums(preds, recons, series, starts, age, max_age=0, dims=None):
    """(4, out) float64: the same four summed over the windows (and time steps) instead of over d."""
    qf, qr = loss_refs.squares(preds, recons, series, starts, dims)
    cols = loss_refs._dims(dims, qf.shape[1])
    mf, mr = _masks(age, max_age, starts, recons.shape[1], cols)
    return np.stack([np.where(mf, qf, 0.0).sum(axis=0), np.where(mr, qr, 0.0).sum(axis=(0, 1)), mf.sum(axis=0).astype(np.float64),
                     mr.sum(axis=(0, 1)).astype(np.float64)], axis=0)


def batch_sums(preds, recons, series, starts, age, max_age=0, dims=None):
    """(S_f, S_r, N_f, N_r) of the batch in the order of mtadgat_eval_group_sums(cols = 4, group = b) over window_sums."""
    return loss_refs.ordered_sum(window_sums(preds, recons, series, starts, age, max_age, dims))


def cotangent_scale(S, N):
    """(c, rmse) of one head."""
    with np.errstate(all="ignore"):
        S, N = np.float64(S), np.float64(N)
        rmse = np.sqrt(S / N) if N > 0 else np.float64(0.0)
        if not np.isfinite(S):
            return np.float64(np.nan), rmse
        if N == 0 or rmse == 0.0:
            return np.float64(0.0), rmse
        return np.float64(1.0) / (N * rmse), rmse


def loss_grad(preds, recons, series, starts, age, max_age=0, dims=None, sums=None, store=np.float32):
    """(d_preds (b, out), d_recons (b, W, out), (rmse_f, rmse_r) float64).  sums: the batch's four sums when the caller has them
    (the device's), else batch_sums.  store: float32 is the kernel's specification, float64 what is held against autograd."""
    preds, recons, series = (np.ascontiguousarray(a, dtype=np.float32) for a in (preds, recons, series))
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    b, W, out = recons.shape
    cols = loss_refs._dims(dims, out)
    S = batch_sums(preds, recons, series, starts, age, max_age, dims) if sums is None else np.asarray(sums, dtype=np.float64)
    cf, rf = cotangent_scale(S[0], S[2])
    cr, rr = cotangent_scale(S[1], S[3])
    mf, mr = _masks(age, max_age, starts, W, cols)
    df = preds - series[starts + W][:, cols]
    dr = recons - series[starts[:, None] + np.arange(W)[None, :]][:, :, cols]
    assert df.dtype == np.float32 and dr.dtype == np.float32
    with np.errstate(all="ignore"):
        gp = np.where(mf, (df.astype(np.float64) * cf).astype(store), store(0.0))
        gr = np.where(mr, (dr.astype(np.float64) * cr).astype(store), store(0.0))
    return gp, gr, np.array([rf, rr])


def group_losses(wsums, batch_size=None):
    """(forecast_loss, recon_loss, total_loss) floats from window_sums (n, 4)."""
    wsums = np.asarray(wsums, dtype=np.float64)
    sums = loss_refs.group_sums(wsums, wsums.shape[0] if batch_size is None else int(batch_size))
    out = []
    with np.errstate(all="ignore"):
        for j in (0, 1):
            seen = sums[:, 2 + j] > 0
            out.append(float(np.sqrt((sums[seen, j] / sums[seen, 2 + j]).mean())) if seen.any() else float("nan"))
    return out[0], out[1], out[0] + out[1]


# ---- the reference gap pattern of tests/test_gpu_fit_mask.py ------------------------------------------------------------------------
def age_of(missing, lengths=None):
    """age from a boolean (N, F) array of missing samples: 0 where present, k for the k-th consecutive missing row of a column,
    counted anew in every part."""
    missing = np.asarray(missing, dtype=bool)
    n, F = missing.shape
    offs = part_offsets(lengths, n)
    age = np.zeros((n, F), dtype=np.int32)
    for lo, hi in zip(offs[:-1], offs[1:]):
        run = np.zeros(F, dtype=np.int32)
        for r in range(lo, hi):
            run = np.where(missing[r], run + 1, 0)
            age[r] = run
    return age


def reference_gaps(n_rows=80, F=6, lengths=(31, 5, 44), p=0.15, seed=11, outages=((50, 3), (60, 7))):
    """(missing (N, F) bool, age (N, F) int32): independent gaps with probability p, whole-row outages (row, rows), age per part."""
    rng = np.random.default_rng(seed)
    missing = rng.random((n_rows, F)) < p
    for row, rows in outages:
        missing[row:row + rows] = True
    return missing, age_of(missing, lengths)
