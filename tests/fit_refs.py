"""The specification of the series trainer's kernels (fitting.SeriesTrainer; the mtadgat_fit_* entry points of include/mtadgat.h), in
plain numpy.  Imports nothing of the package; the squared-error sums are those of tests/loss_refs.py.

One step on a batch of b windows of a series, window w starting at row s_w, output dimension d compared with series column dims[d]:
  gather      x[w, t, :] = series[s_w + t]                                                       t < W
  loss_grad   S_f, S_r = loss_refs.ordered_sum(loss_refs.window_sse(..))   N_f = b out, N_r = b W out
              rmse = sqrt(S / N), c = 1 / (N rmse) in float64;  c = 0 where rmse == 0, c = NaN where S is not finite
              d_preds = float32(float64(preds - y) c_f), d_recons = float32(float64(recons - x) c_r), each difference ONE float32
              subtraction.  This is the gradient of loss = rmse_f + rmse_r (the reference's sqrt(mse) + sqrt(mse)).
              DEPARTURE from torch: at rmse == 0 autograd's sqrt gives 0 / 0 = NaN, here the cotangent is 0.
  grad_norm_sq  the float64 sum of float64(g)^2 in a fixed order: blocks of NORM_CHUNK consecutive entries, each summed by
              loss_refs.ordered_sum, the blocks' sums by ordered_sum again.  The squares are exact, so the order alone decides the
              bits; two orders differ by at most loss_refs.bound(n) relative.
  prepare     the step record: t <- t + 1, clip = min(1, max_norm / (norm + 1e-6)) (torch's clip_grad_norm_) or 1,
              step_size = lr / (1 - beta1^t), bc2s = sqrt(1 - beta2^t), b^t by int_power (squaring: the multiplications in a fixed
              order, so both sides of a comparison hold the same bits and 1 - b^t does not amplify a last-bit difference);
              applied = 0 and t unchanged when skip_nonfinite is set and the norm or a loss is not finite.
  adam_step   Adam / AdamW in float64 on float32-stored state, every product rounded (no fused multiply-add), every result rounded
              to float32 ONCE.  torch.optim.Adam on float32 tensors rounds after every operation instead: its parameters differ from
              these in the last bits (tests/test_host_fit.py holds the float64 algebra against torch's to 1e-12)."""
import numpy as np

import loss_refs

NORM_CHUNK = 4096
STATE_FIELDS = ("t", "calls", "clip", "step_size", "bc2s", "applied", "norm_sq", "norm")
EPS32 = 2.0 ** -24


def gather(series, starts, W):
    series = np.asarray(series, dtype=np.float32)
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    return series[starts[:, None] + np.arange(W)[None, :]]


def batch_sums(preds, recons, series, starts, dims=None):
    """(S_f, S_r) float64: the batch's sums in the order of mtadgat_eval_group_sums(group = b) over window_sse."""
    return loss_refs.ordered_sum(loss_refs.window_sse(preds, recons, series, starts, dims))


def cotangent_scale(S, N):
    """(c, rmse) of one head."""
    with np.errstate(all="ignore"):
        rmse = np.sqrt(np.float64(S) / np.float64(N))
        if not np.isfinite(S):
            return np.float64(np.nan), rmse
        return (np.float64(0.0) if rmse == 0.0 else np.float64(1.0) / (np.float64(N) * rmse)), rmse


def loss_grad(preds, recons, series, starts, dims=None, sums=None, store=np.float32):
    """(d_preds (b, out) float32, d_recons (b, W, out) float32, (rmse_f, rmse_r) float64).  sums: the two batch sums when the caller
    has them (the device's, so that only the division and the square root can differ), else batch_sums.  store: the type the
    cotangents are rounded to -- float32 is the specification of the kernel, float64 (no rounding) what the host test holds against
    autograd in float64 on inputs whose float32 differences are exact."""
    preds, recons, series = (np.ascontiguousarray(a, dtype=np.float32) for a in (preds, recons, series))
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    b, W, out = recons.shape
    cols = np.arange(out) if dims is None else np.asarray(dims, dtype=np.int64).reshape(-1)
    S = batch_sums(preds, recons, series, starts, dims) if sums is None else np.asarray(sums, dtype=np.float64)
    cf, rf = cotangent_scale(S[0], b * out)
    cr, rr = cotangent_scale(S[1], b * W * out)
    df = preds - series[starts + W][:, cols]
    dr = recons - series[starts[:, None] + np.arange(W)[None, :]][:, :, cols]
    assert df.dtype == np.float32 and dr.dtype == np.float32
    with np.errstate(all="ignore"):
        return (df.astype(np.float64) * cf).astype(store), (dr.astype(np.float64) * cr).astype(store), np.array([rf, rr])


def grad_norm_sq(g):
    sq = np.asarray(g, dtype=np.float32).reshape(-1).astype(np.float64) ** 2
    parts = [loss_refs.ordered_sum(sq[i:i + NORM_CHUNK, None]) for i in range(0, sq.size, NORM_CHUNK)]
    return float(loss_refs.ordered_sum(np.stack(parts))[0])


def int_power(b, t):
    r, b, t = np.float64(1.0), np.float64(b), int(t)
    while t > 0:
        if t & 1:
            r = r * b
        b = b * b
        t >>= 1
    return r


def prepare(state, norm_sq, rmse, lr, betas, max_grad_norm=None, skip_nonfinite=False):
    """The record after the call, a dict over STATE_FIELDS, from the record before it (a dict; {} is the zeroed record)."""
    old = {k: np.float64(state.get(k, 0.0)) for k in STATE_FIELDS}
    with np.errstate(all="ignore"):
        norm = np.sqrt(np.float64(norm_sq))
        finite = bool(np.isfinite(norm) and np.isfinite(rmse[0]) and np.isfinite(rmse[1]))
        applied = 0.0 if (skip_nonfinite and not finite) else 1.0
        new = dict(old, calls=old["calls"] + 1, applied=np.float64(applied), norm_sq=np.float64(norm_sq), norm=norm)
        if applied:
            t = int(old["t"]) + 1
            clip = np.float64(1.0)
            if max_grad_norm is not None:
                clip = np.float64(max_grad_norm) / (norm + np.float64(1e-6))
                clip = np.float64(1.0) if clip > 1.0 else clip
            new.update(t=np.float64(t), clip=clip, step_size=np.float64(lr) / (np.float64(1.0) - int_power(betas[0], t)),
                       bc2s=np.sqrt(np.float64(1.0) - int_power(betas[1], t)))
    return new


def adam_step(p, g, m, v, rec, lr, betas, eps, weight_decay=0.0, decoupled=False, store=np.float32):
    """(p, m, v) after the step from the record `rec` of prepare.  store: the type the three results are rounded to -- float32 is the
    specification of the kernel, float64 (no rounding) the algebra that the host test holds against torch in float64."""
    if not rec["applied"]:
        return np.array(p, copy=True), np.array(m, copy=True), np.array(v, copy=True)
    b1, b2 = np.float64(betas[0]), np.float64(betas[1])
    lr, eps, wd = np.float64(lr), np.float64(eps), np.float64(weight_decay)
    with np.errstate(all="ignore"):
        pd = np.asarray(p).astype(np.float64)
        gd = np.asarray(g).astype(np.float64) * rec["clip"]
        if wd != 0.0:
            if decoupled:
                pd = pd * (np.float64(1.0) - lr * wd)
            else:
                gd = gd + wd * pd
        md = b1 * np.asarray(m).astype(np.float64) + (np.float64(1.0) - b1) * gd
        vd = b2 * np.asarray(v).astype(np.float64) + (np.float64(1.0) - b2) * (gd * gd)
        pd = pd - rec["step_size"] * (md / (np.sqrt(vd) / rec["bc2s"] + eps))
        return pd.astype(store), md.astype(store), vd.astype(store)


def ulps32(a, b):
    """|a - b| in units of the float32 spacing at b, elementwise (0 where both are NaN or equal, inf where one is NaN)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(all="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)
    d = np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, d)
    return np.where(np.isnan(d), np.inf, d)
