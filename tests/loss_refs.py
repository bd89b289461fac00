"""The specification of the forecast / reconstruction losses of a series (evaluation.window_sse, MTAD_GAT.series_losses and the
mtadgat_eval_window_sse / mtadgat_eval_group_sums entry points), in plain numpy.  Imports neither the package's kernels nor pandas.

Window w of a series (N, F) starts at row s_w, reads rows s_w .. s_w + W - 1 and is asked to forecast row s_w + W; output
dimension d is compared with series column dims[d].  Arithmetic, everywhere: the difference is ONE float32 subtraction, it is
converted to float64 and squared there (exact: the square of a 24-bit significand fits 53 bits), and the squares are summed in
float64.  The addends are non-negative, so two summation orders differ by at most terms * 2^-53 relative (`bound`).

trainer_evaluate restates the reference's Trainer.evaluate (training.py:188-228): per loader batch sqrt(mse(y, preds)) and
sqrt(mse(x[:, :, dims], recons)), then sqrt(mean(l^2)) over the batches -- so a short last batch weighs as much as a full one.
Deliberate departure: the reference forms the MSEs in float32 with torch's reduction order; here they are float64 sums of the
float32 differences, which is what the package computes and what a summation-order bound can be stated for."""
import numpy as np

EPS64 = 2.0 ** -53


def bound(terms):
    """Relative distance allowed between two float64 sums of the same `terms` non-negative addends."""
    return terms * EPS64


def _dims(dims, out):
    return np.arange(out) if dims is None else np.asarray(dims, dtype=np.int64).reshape(-1)


def squares(preds, recons, series, starts, dims=None):
    """(forecast squares (n, out), reconstruction squares (n, W, out)) float64, from float32 differences."""
    preds, recons, series = (np.ascontiguousarray(a, dtype=np.float32) for a in (preds, recons, series))
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    n, W, out = recons.shape
    cols = _dims(dims, out)
    rows = starts[:, None] + np.arange(W)[None, :]
    df = preds - series[starts + W][:, cols]
    dr = recons - series[rows][:, :, cols]
    assert df.dtype == np.float32 and dr.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        return df.astype(np.float64) ** 2, dr.astype(np.float64) ** 2


def window_sse(preds, recons, series, starts, dims=None):
    """(n, 2) float64: [w, 0] the forecast's squared error summed over d, [w, 1] the reconstruction's over (t, d)."""
    qf, qr = squares(preds, recons, series, starts, dims)
    return np.stack([qf.sum(axis=1), qr.reshape(qr.shape[0], -1).sum(axis=1)], axis=1)


def dim_sse(preds, recons, series, starts, dims=None):
    """(2, out) float64: the same squares summed over the windows (and time steps) instead of over d."""
    qf, qr = squares(preds, recons, series, starts, dims)
    return np.stack([qf.sum(axis=0), qr.sum(axis=(0, 1))], axis=0)


def ordered_sum(x):
    """The sum over the rows of x (m, cols) in THE fixed order of the group sums, part of the specification so that the losses
    formed from them can be compared exactly: 256 lanes, lane t adds rows t, t + 256, .. in that order starting from +0.0; then
    the lanes are added in a halving tree, lane t += lane t + s for s = 128, 64, .., 1."""
    x = np.asarray(x, dtype=np.float64)
    lanes = np.zeros((256, x.shape[1]), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(min(256, x.shape[0])):
            for row in x[t::256]:
                lanes[t] = lanes[t] + row
        s = 128
        while s:
            for t in range(s):
                lanes[t] = lanes[t] + lanes[t + s]
            s //= 2
    return lanes[0].copy()


def group_sums(x, group):
    """ordered_sum of consecutive groups of `group` rows of x (n, cols); the last group may be short."""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([ordered_sum(x[i:i + group]) for i in range(0, x.shape[0], group)], axis=0)


def group_losses(wsse, W, out, batch_size=None):
    """(forecast_loss, recon_loss, total_loss) floats from window_sse (n, 2).  batch_size None: the global RMSEs
    sqrt(sum SSE_f / (n out)), sqrt(sum SSE_r / (n W out)); otherwise the reference's epoch value, sqrt(mean over the loader's
    batches of that batch's MSE) -- the mean of the batches' squared RMSEs, each batch with weight 1."""
    wsse = np.asarray(wsse, dtype=np.float64)
    n = wsse.shape[0]
    b = n if batch_size is None else int(batch_size)
    sums = group_sums(wsse, b)
    counts = np.array([min(b, n - i) for i in range(0, n, b)], dtype=np.float64)
    mse_f = sums[:, 0] / (counts * out)
    mse_r = sums[:, 1] / (counts * W * out)
    f = float(np.sqrt(mse_f.mean()))
    r = float(np.sqrt(mse_r.mean()))
    return f, r, f + r


def trainer_evaluate(model, series, W, target_dims=None, batch_size=256):
    """Trainer.evaluate over SlidingWindowDataset(series, W) with shuffle=False: `model` maps a float32 (b, W, F) torch tensor to
    (preds, recons).  Returns (forecast_loss, recon_loss, total_loss, window_sse (n, 2)): the per-window sums are a by-product
    of the per-batch MSEs, kept for the tests."""
    import torch
    series = np.ascontiguousarray(series, dtype=np.float32)
    N, F = series.shape
    n = N - W
    dims = None if target_dims is None else ([target_dims] if isinstance(target_dims, int) else list(target_dims))
    f2, r2, rows = [], [], []
    with torch.no_grad():
        for lo in range(0, n, batch_size):
            hi = min(n, lo + batch_size)
            starts = np.arange(lo, hi)
            x = np.stack([series[s:s + W] for s in starts])
            preds, recons = model(torch.from_numpy(x))
            preds, recons = preds.numpy(), recons.numpy()
            if preds.ndim == 3:
                preds = preds.squeeze(1)
            out = preds.shape[1]
            w = window_sse(preds, recons, series, starts, dims)
            rows.append(w)
            f2.append(w[:, 0].sum() / ((hi - lo) * out))              # = mse(y, preds): l^2 of the batch
            r2.append(w[:, 1].sum() / ((hi - lo) * W * out))
    f = float(np.sqrt(np.mean(f2)))
    r = float(np.sqrt(np.mean(r2)))
    return f, r, f + r, np.concatenate(rows)
