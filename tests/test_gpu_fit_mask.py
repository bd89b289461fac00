"""Training on gappy, concatenated series on the GPU (fitting.training_windows, SeriesTrainer.step / fit with `age`,
MTAD_GAT.series_losses(age=); csrc/mtadgat_fitwin.hip and the masked instances of csrc/mtadgat_losses.hip / mtadgat_fit.hip) against
tests/fit_mask_refs.py.

The reference gap pattern (fit_mask_refs.reference_gaps): shape w8 of train_route_cases (W = 8, F = 6), 80 rows in parts of
31, 5 and 44 -- the middle one shorter than W + 1 --, independent gaps with probability 0.15 and two whole-row outages; of the 72
starts 13 fall to the seam rule, and the target-row and the min_observed rule each remove and keep windows at the settings used
(tests/test_host_fit_mask.py pins the counts; the tests here assert it of their inputs again).

Tolerances.  The sampler is integer arithmetic: exact.  The counts N: exact.  A sum S of `terms` non-negative float64 addends against
another order of the same addends: loss_refs.bound(terms) relative.  A float64 scalar formed by one or two correctly rounded
operations from identical inputs: 4 * 2^-53 relative (REL64); an rmse = sqrt(S / N) from sums that differ by bound(terms): half of
that bound plus REL64.  A cotangent is ONE float32 rounding of a float64 product whose factors agree to a few 2^-53: 1 float32 ulp of
the specification evaluated on the device's sums; an unobserved entry is exactly +0.0.  Parameter gradients of the step against the
existing route's: train_route_cases.GATE_C per tensor, as tests/test_gpu_fit.py holds the unmasked step.

Launch counts: mtadgat_fit_windows issues the same seven launches for 1 and for 37 parts -- checked by reading the entry point: the
launch sequence has no branch on `parts` (a start's part is a binary search inside the predicate), the only conditional launches are
the two that a series of exactly W rows, which has no start at all, would give an empty grid."""
import math

import numpy as np
import pytest
import torch

import arena
import fit_mask_refs as fm
import fit_refs
import loss_refs
import train_route_cases as tc
from guard_rows import four_calls
from test_gpu_fit import (BATCH, HYPER, K_STEPS, LOSS_CASES, N_ROWS, REL64, SEED, SHAPE, STEP_MODELS, _batches, _close64, _dev, _flat_state,
                          _kwargs, _new_model, _record, _series, _starts, _strided_series, _trainer, _ulp1)
from test_gpu_guard_bands_eval import refuse_scratch

pytestmark = pytest.mark.gpu

W8, F6 = tc.SHAPES[SHAPE]["window_size"], tc.SHAPES[SHAPE]["n_features"]
LENGTHS = [31, 5, 44]
GRID = [([4, 0, 2], 0), ([3], 0), ([4, 0, 2], 2)]
MIN_OBSERVED = (0.0, 0.5, 0.8, 1.0)


def _min_count(m, W, F):
    return math.ceil(m * W * F)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32 if t.element_size() == 4 else np.uint64)


def _rel(got, want, rel, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = (np.abs(got - want) <= rel * np.abs(want)) | (np.isnan(got) & np.isnan(want))
    assert np.all(ok), (what, got[~ok][:4], want[~ok][:4])


# ---- 1. the sampler ------------------------------------------------------------------------------------------------------------------
def _sample(dev, n_rows, W, F, lengths, age, max_age, dims, min_observed):
    import fitting
    age_dev = None if age is None else _dev(dev, age)
    return fitting.training_windows(n_rows, W, F, lengths=lengths, age=age_dev, max_age=max_age, min_observed=min_observed,
                                    target_dims=dims, device=dev)


@pytest.mark.parametrize("dims,max_age", GRID, ids=["dims3", "dim1", "dims3-age2"])
def test_sampler_on_the_reference_grid(dims, max_age, gpu_device):
    _, age = fm.reference_gaps(N_ROWS, F6, LENGTHS)
    same, target, _ = fm.rule_masks(N_ROWS, W8, F6, LENGTHS, age, max_age, dims, 0)
    assert same.any() and (~same).any() and (same & target).any() and (same & ~target).any()       # rules 1 and 2 remove and keep
    for m in MIN_OBSERVED:
        mc = _min_count(m, W8, F6)
        enough = fm.rule_masks(N_ROWS, W8, F6, LENGTHS, age, max_age, dims, mc)[2]
        want = fm.windows(N_ROWS, W8, F6, LENGTHS, age, max_age, dims, mc)
        got = _sample(gpu_device, N_ROWS, W8, F6, LENGTHS, age, max_age, dims, m)
        assert got.dtype == torch.int64 and got.device.type == "cuda" and np.array_equal(got.cpu().numpy(), want), (m, got, want)
        if m == 0.8:
            assert (same & target & enough).any() and (same & target & ~enough).any()               # rule 3 removes and keeps
        for lengths, a in ((None, age), (LENGTHS, None), (None, None)):
            got = _sample(gpu_device, N_ROWS, W8, F6, lengths, a, max_age, dims, m)
            assert np.array_equal(got.cpu().numpy(), fm.windows(N_ROWS, W8, F6, lengths, a, max_age, dims, mc)), (m, lengths is None, a is None)
    assert np.array_equal(_sample(gpu_device, N_ROWS, W8, F6, None, None, 0, None, 1.0).cpu().numpy(), np.arange(N_ROWS - W8))


def test_sampler_without_a_valid_window_and_identical_calls(gpu_device):
    import _native
    _, age = fm.reference_gaps(N_ROWS, F6, LENGTHS)
    age_dev = _dev(gpu_device, age)
    dims = torch.tensor([4, 0, 2], dtype=torch.int32, device=gpu_device)
    offs = torch.tensor(fm.part_offsets(LENGTHS, N_ROWS), dtype=torch.int64, device=gpu_device)
    assert fm.windows(N_ROWS, W8, F6, LENGTHS, age, 0, [4, 0, 2], W8 * F6).size == 0
    starts, count = _native.fit_windows(N_ROWS, W8, F6, gpu_device, age=age_dev, dims=dims, offsets=offs, min_count=W8 * F6)
    assert count.item() == 0 and starts.shape == (N_ROWS - W8,)
    runs = []
    for _ in range(2):
        starts, count = _native.fit_windows(N_ROWS, W8, F6, gpu_device, age=age_dev, dims=dims, offsets=offs, min_count=24)
        runs.append((starts[:int(count.item())].cpu().numpy(), int(count.item())))
    assert runs[0][1] == runs[1][1] == 44 and np.array_equal(runs[0][0], runs[1][0])
    # a series of exactly one window: no start, count 0
    starts, count = _native.fit_windows(W8, W8, F6, gpu_device, age=age_dev[:W8].contiguous())
    assert count.item() == 0 and starts.numel() == 0


@pytest.mark.parametrize("parts", [1, 37])
@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("n_rows", [W8 + 1, 1023, 1024, 1025, 5000])
def test_sampler_at_scan_boundaries(n_rows, F, parts, gpu_device):
    """Around one and several chunks of 1 024 rows of the scans, one part and 37 (most of them empty at 9 rows)."""
    rng = np.random.default_rng(1000 * n_rows + 10 * F + parts)
    lengths = [n_rows] if parts == 1 else rng.multinomial(n_rows, np.full(parts, 1.0 / parts)).tolist()
    missing = rng.random((n_rows, F)) < 0.3
    if n_rows > 600:
        missing[500:520] = True                                      # an outage longer than a window
    age = fm.age_of(missing, lengths)
    dims = None if F == 1 else [4, 0]
    for max_age, m in ((0, 0.6), (1, 0.9)):
        want = fm.windows(n_rows, W8, F, lengths, age, max_age, dims, _min_count(m, W8, F))
        got = _sample(gpu_device, n_rows, W8, F, lengths if parts > 1 else None, age, max_age, dims, m)
        assert np.array_equal(got.cpu().numpy(), want), (max_age, m, got.numel(), want.size)
        if n_rows > 600:
            assert 0 < want.size < n_rows - W8


# ---- 2. the masked sums and cotangents ---------------------------------------------------------------------------------------------------
def _gappy(rng, n_rows, F, p=0.25):
    """(series, age) with gaps of probability p; hide() puts a NaN under the mask."""
    return rng.standard_normal((n_rows, F)).astype(np.float32), fm.age_of(rng.random((n_rows, F)) < p)


def _hide(series, age, max_age=0):
    """NaN at every unobserved sample: what the mask hides must not reach a sum or a cotangent."""
    series = series.copy()
    series[age > max_age] = np.nan
    return series


def _check_masked(dev, series, age, preds, recons, starts, dims, pad=3, max_age=0):
    import _native
    import evaluation
    b, W, out = recons.shape
    series = _hide(series, age, max_age)
    s = _strided_series(dev, series, pad)
    a = torch.zeros((age.shape[0], age.shape[1] + pad + 1), dtype=torch.int32, device=dev)[:, :age.shape[1]]
    a.copy_(_dev(dev, age))
    assert a.stride(0) == age.shape[1] + pad + 1
    p, r, st = _dev(dev, preds), _dev(dev, recons), _dev(dev, starts)
    dims_dev = None if dims is None else torch.tensor(dims, dtype=torch.int32, device=dev)
    window, dim = _native.fit_masked_sse(p, r, s, st, a, max_age=max_age, dims=dims_dev)
    want_w, want_d = fm.window_sums(preds, recons, series, starts, age, max_age, dims), fm.dim_sums(preds, recons, series, starts, age, max_age, dims)
    got_w, got_d = window.cpu().numpy(), dim.cpu().numpy()
    assert np.array_equal(got_w[:, 2:], want_w[:, 2:]) and np.array_equal(got_d[2:], want_d[2:])                 # N: exact
    assert np.isfinite(got_w).all() and np.isfinite(got_d).all()
    _rel(got_w[:, 0], want_w[:, 0], loss_refs.bound(out), "S_f")
    _rel(got_w[:, 1], want_w[:, 1], loss_refs.bound(W * out), "S_r")
    _rel(got_d[0], want_d[0], loss_refs.bound(b + 4), "dim S_f")
    _rel(got_d[1], want_d[1], loss_refs.bound(b * W + 4), "dim S_r")
    sums = evaluation.group_sums(window, b).reshape(4)
    spec_sums = fm.batch_sums(preds, recons, series, starts, age, max_age, dims)
    assert np.array_equal(sums.cpu().numpy()[2:], spec_sums[2:])
    _rel(sums.cpu().numpy()[:2], spec_sums[:2], loss_refs.bound(W * out + b), "batch sums")
    dp, dr, rmse = _native.fit_masked_loss_grad(p, r, s, st, a, sums, max_age=max_age, dims=dims_dev)
    want_p, want_r, want_rmse = fm.loss_grad(preds, recons, series, starts, age, max_age, dims, sums=sums.cpu().numpy())
    _ulp1(dp.cpu().numpy(), want_p, "d_preds")
    _ulp1(dr.cpu().numpy(), want_r, "d_recons")
    _close64(rmse.cpu().numpy(), want_rmse, "rmse")
    cols = loss_refs._dims(dims, out)
    mf, mr = fm._masks(age, max_age, starts, W, cols)
    assert not _bits(dp)[~mf].any() and not _bits(dr)[~mr].any()                                              # unobserved: +0.0 exactly
    assert np.isfinite(dp.cpu().numpy()).all() and np.isfinite(dr.cpu().numpy()).all()
    # identical calls, identical bits
    window2, dim2 = _native.fit_masked_sse(p, r, s, st, a, max_age=max_age, dims=dims_dev)
    dp2, dr2, rmse2 = _native.fit_masked_loss_grad(p, r, s, st, a, sums, max_age=max_age, dims=dims_dev)
    assert torch.equal(window, window2) and torch.equal(dim, dim2) and torch.equal(dp, dp2) and torch.equal(dr, dr2) and torch.equal(rmse, rmse2)
    return mf, mr


@pytest.mark.parametrize("batch", [1, 7, 33])
@pytest.mark.parametrize("case", list(LOSS_CASES))
def test_masked_sums_and_cotangents_against_the_reference(case, batch, gpu_device):
    out, dims = LOSS_CASES[case]
    W, F, n_rows = 10, 7, 60
    rng = np.random.default_rng(7 * batch + out)
    series, age = _gappy(rng, n_rows, F)
    preds = rng.standard_normal((batch, out)).astype(np.float32)
    recons = rng.standard_normal((batch, W, out)).astype(np.float32)
    starts = _starts(rng, n_rows, W, batch)
    mf, mr = _check_masked(gpu_device, series, age, preds, recons, starts, dims)
    if batch > 1:
        assert mr.any() and (~mr).any()                               # the mask hides and shows
        _check_masked(gpu_device, series, age, preds, recons, starts, dims, pad=0, max_age=1)


def test_masked_sums_of_a_wide_output(gpu_device):
    """out_dim = 300 > 256 reaches the 8-column instance of the reduction (handle-free: no model of that width is built)."""
    rng = np.random.default_rng(300)
    out, W, batch, n_rows = 300, 3, 5, 20
    series, age = _gappy(rng, n_rows, out)
    preds = rng.standard_normal((batch, out)).astype(np.float32)
    recons = rng.standard_normal((batch, W, out)).astype(np.float32)
    mf, mr = _check_masked(gpu_device, series, age, preds, recons, np.array([0, 16, 3, 3, 9]), None)
    assert mr.any() and (~mr).any() and mf.any() and (~mf).any()


@pytest.mark.parametrize("case", ["out5 dims", "wide"])
def test_all_observed_equals_the_unmasked_calls_bit_for_bit(case, gpu_device):
    import _native
    import evaluation
    rng = np.random.default_rng(17)
    (out, dims), W, F, n_rows, batch = (LOSS_CASES[case], 10, 7, 60, 33) if case != "wide" else ((300, None), 3, 300, 20, 5)
    series = rng.standard_normal((n_rows, F)).astype(np.float32)
    preds, recons = rng.standard_normal((batch, out)).astype(np.float32), rng.standard_normal((batch, W, out)).astype(np.float32)
    starts = _starts(rng, n_rows, W, batch)
    s, p, r, st = _strided_series(gpu_device, series, 3), _dev(gpu_device, preds), _dev(gpu_device, recons), _dev(gpu_device, starts)
    dims_dev = None if dims is None else torch.tensor(dims, dtype=torch.int32, device=gpu_device)
    for max_age, fill in ((0, 0), (3, 2)):
        age = torch.full((n_rows, F), fill, dtype=torch.int32, device=gpu_device)
        window, dim = _native.fit_masked_sse(p, r, s, st, age, max_age=max_age, dims=dims_dev)
        wsse, dsse = evaluation.window_sse(p, r, s, starts=st, dims=dims)
        assert np.array_equal(_bits(window[:, :2]), _bits(wsse)) and np.array_equal(_bits(dim[:2]), _bits(dsse))
        assert (window[:, 2] == out).all() and (window[:, 3] == W * out).all() and (dim[2] == batch).all() and (dim[3] == batch * W).all()
        sums4 = evaluation.group_sums(window, batch).reshape(4)
        sums2 = evaluation.group_sums(wsse, batch).reshape(2)
        assert np.array_equal(_bits(sums4[:2]), _bits(sums2)) and sums4[2] == batch * out and sums4[3] == batch * W * out
        got = _native.fit_masked_loss_grad(p, r, s, st, age, sums4, max_age=max_age, dims=dims_dev)
        want = _native.fit_loss_grad(p, r, s, st, sums2, dims=dims_dev)
        for g, w in zip(got, want):
            assert np.array_equal(_bits(g), _bits(w))


def test_a_nan_under_the_mask_reaches_neither_sums_nor_cotangents(gpu_device):
    """A single NaN at a row that is only ever a target (starts = [r - W]), marked unobserved."""
    import _native
    import evaluation
    rng = np.random.default_rng(23)
    W, F, n_rows, out, r_nan = 10, 7, 60, 5, 41
    series = rng.standard_normal((n_rows, F)).astype(np.float32)
    series[r_nan, 2] = np.nan
    age = np.zeros((n_rows, F), dtype=np.int32)
    age[r_nan, 2] = 1
    dims = [4, 0, 2, 2, 6]
    preds, recons = rng.standard_normal((1, out)).astype(np.float32), rng.standard_normal((1, W, out)).astype(np.float32)
    starts = np.array([r_nan - W])
    s, a, p, r, st = (_dev(gpu_device, x) for x in (series, age, preds, recons, starts))
    dims_dev = torch.tensor(dims, dtype=torch.int32, device=gpu_device)
    window, dim = _native.fit_masked_sse(p, r, s, st, a, dims=dims_dev)
    assert torch.isfinite(window).all() and torch.isfinite(dim).all() and window[0, 2] == 3 and window[0, 3] == W * out
    dp, dr, rmse = _native.fit_masked_loss_grad(p, r, s, st, a, evaluation.group_sums(window, 1).reshape(4), dims=dims_dev)
    assert torch.isfinite(dp).all() and torch.isfinite(dr).all() and torch.isfinite(rmse).all()
    assert dp[0, 2] == 0 and dp[0, 3] == 0 and dp[0, [0, 1, 4]].abs().min() > 0
    # the unmasked sum of the same window is NaN: the select is what keeps it out
    assert torch.isnan(evaluation.window_sse(p, r, s, starts=st, dims=dims)[0][0, 0])


# ---- 3. the step against the existing route ------------------------------------------------------------------------------------------------
def _reference_age(dev):
    _, age = fm.reference_gaps(N_ROWS, F6, LENGTHS)
    return age, _dev(dev, age)


def _masked_loss(preds, recons, x, y, mx, my, cols):
    """The masked loss in torch, float32: sqrt(sum m r^2 / sum m) per head."""
    if cols is not None:
        x, y, mx, my = x[:, :, cols], y[:, cols], mx[:, :, cols], my[:, cols]
    if preds.ndim == 3:
        preds = preds.squeeze(1)
    mx, my = mx.to(preds.dtype), my.to(preds.dtype)
    return torch.sqrt((my * (preds - y) ** 2).sum() / my.sum()), torch.sqrt((mx * (recons - x) ** 2).sum() / mx.sum())


@pytest.mark.parametrize("p_drop", [0.0, tc.P_DROP])
@pytest.mark.parametrize("name", ["dims3", "all"])
def test_masked_step_against_the_existing_route(name, p_drop, gpu_device):
    import _hipgrad
    from mtad_gat import MTAD_GAT
    dev = gpu_device
    kw = _kwargs(name, p_drop)
    W, out = kw["window_size"], kw["out_dim"]
    cols = STEP_MODELS[name]["target_dims"]
    A = _new_model(name, p_drop, dev)
    tr = _trainer(A, name)
    B = MTAD_GAT(**kw).to(dev).train()
    series = _series(dev)
    ser = series.cpu().numpy()
    age, age_dev = _reference_age(dev)
    seen = age_dev <= 0
    rows_of = torch.arange(W, device=dev)[None, :]
    for k, starts in enumerate(_batches(dev)):
        B.load_state_dict(A.state_dict())
        p0, m0, v0 = _flat_state(tr)
        rec0 = _record(tr.state)
        tr.step(series, starts, age=age_dev)
        x, mx = series[starts[:, None] + rows_of], seen[starts[:, None] + rows_of]
        y, my = series[starts + W], seen[starts + W]
        assert 0 < int(mx.sum()) < mx.numel() and 0 < int(my.sum())
        B.dropout_stream = (tr.step_seed(k), 0)
        B.zero_grad(set_to_none=True)
        preds, recons = B(x)
        assert B.grad_path == "hip"
        lf, lr_ = _masked_loss(preds, recons, x, y, mx, my, cols)
        (lf + lr_).backward()
        # 1. the same outputs, bit for bit
        assert torch.equal(preds, tr.last_preds) and torch.equal(recons, tr.last_recons), k
        # 2. the gradients, per parameter tensor
        for (pname, pb), (o, n) in zip(zip(A._engine.flat_keys(), _hipgrad.param_order(B)), tr._spans):
            ga, gb = tr.grads[o:o + n].view(pb.shape), pb.grad
            s = gb.abs().max().item()
            assert (ga - gb).abs().max().item() <= tc.GATE_C * s + 1e-30, (k, pname)
        assert tr.grads.abs().max().item() > 0.0
        # 3. the parameters after the step: Adam's specification on the state before it and the step's gradients
        g = tr.grads.cpu().numpy()
        logged = tr.losses(last=1)[0]
        rec = fit_refs.prepare(rec0, fit_refs.grad_norm_sq(g), logged[:2], HYPER["lr"], (0.9, 0.999), HYPER["max_grad_norm"])
        want = fit_refs.adam_step(p0, g, m0, v0, rec, HYPER["lr"], (0.9, 0.999), 1e-8, HYPER["weight_decay"])
        for got, ref, what in zip(_flat_state(tr), want, ("params", "exp_avg", "exp_avg_sq")):
            _ulp1(got, ref, (k, what))
        assert _record(tr.state)["t"] == k + 1 and logged[3] == 1.0
        # 4. the logged losses: B's outputs through the specification (the sums in another order: half their bound under the root)
        starts_h = starts.cpu().numpy()
        ws = fm.window_sums(preds.detach().cpu().numpy(), recons.detach().cpu().numpy(), ser, starts_h, age, 0, cols)
        f, r, _ = fm.group_losses(ws)
        _rel(logged[:2], [f, r], loss_refs.bound(W * out + BATCH) / 2 + REL64, "logged losses")
        assert abs(lf.item() - f) <= 1e-5 * f and abs(lr_.item() - r) <= 1e-5 * r


@pytest.mark.parametrize("p_drop", [0.0, tc.P_DROP])
def test_an_all_zero_age_steps_like_no_age(p_drop, gpu_device):
    dev = gpu_device
    series = _series(dev)
    zero = torch.zeros((N_ROWS, F6), dtype=torch.int32, device=dev)
    trainers = []
    for age in (zero, None):
        tr = _trainer(_new_model("dims3", p_drop, dev), "dims3")
        for starts in _batches(dev, K_STEPS):
            if age is None:
                tr.step(series, starts)
            else:
                tr.step(series, starts, age=age)
        trainers.append(tr)
    for a, b in zip(_flat_state(trainers[0]), _flat_state(trainers[1])):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(trainers[0].losses(), trainers[1].losses())


def test_a_batch_whose_forecast_targets_are_all_unobserved(gpu_device):
    """rmse_f == 0, d_preds all zero, and the step is applied on the reconstruction's gradient alone."""
    dev = gpu_device
    tr = _trainer(_new_model("dims3", 0.0, dev), "dims3", skip_nonfinite=True)
    series = _series(dev).clone()
    starts = torch.tensor([52, 52, 52], dtype=torch.int64, device=dev)                 # rows 52 .. 59, target 60: the second outage begins
    age, age_dev = _reference_age(dev)
    assert (age[60] > 0).all() and (age[53:60] == 0).any()
    series[60] = float("nan")                                                          # what the outage holds does not matter
    before = tr.params.clone()
    tr.step(series, starts, age=age_dev)
    logged = tr.losses(last=1)[0]
    assert logged[0] == 0.0 and logged[1] > 0.0 and math.isfinite(logged[2]) and logged[2] > 0 and logged[3] == 1.0
    d_preds = tr._bufs[3]["d_preds"]
    assert not _bits(d_preds).any() and torch.isfinite(tr.params).all() and not torch.equal(tr.params, before)


# ---- 4. fit ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dims3", "all"])
def test_fit_on_the_sampled_windows(name, gpu_device):
    import fitting
    dev = gpu_device
    cols = STEP_MODELS[name]["target_dims"]
    series, val = _series(dev), _series(dev, seed=11)
    age, age_dev = _reference_age(dev)
    tr = _trainer(_new_model(name, tc.P_DROP, dev), name)
    out = tr.fit(series, val_series=val, epochs=1, batch_size=16, shuffle=False, lengths=LENGTHS, age=age_dev, val_lengths=LENGTHS, val_age=age_dev)
    windows = fitting.training_windows(N_ROWS, W8, F6, LENGTHS, age_dev, 0, 0.5, cols, dev)
    want = fm.windows(N_ROWS, W8, F6, LENGTHS, age, 0, cols, 24)
    assert np.array_equal(windows.cpu().numpy(), want) and 0 < want.size < N_ROWS - W8
    steps = math.ceil(want.size / 16)
    assert _record(tr.state)["calls"] == steps == tr.losses().shape[0]
    rows = tr.losses(last=steps)
    f, r = (float(np.sqrt(np.mean(rows[:, j] ** 2))) for j in (0, 1))
    assert out["train_forecast"] == [f] and out["train_recon"] == [r] and out["train_total"] == [f + r]
    direct = tr.model.series_losses(val, target_dims=cols, batch_size=16, starts=windows, age=age_dev)
    assert (out["val_forecast"], out["val_recon"], out["val_total"]) == ([direct.forecast_loss], [direct.recon_loss], [direct.total_loss])
    assert direct.n_windows == want.size and math.isfinite(direct.total_loss)
    # the same steps by hand
    tb = _trainer(_new_model(name, tc.P_DROP, dev), name)
    for lo in range(0, want.size, 16):
        tb.step(series, windows[lo:lo + 16], age=age_dev)
    assert torch.equal(tb.params, tr.params) and np.array_equal(tb.losses(), tr.losses())
    # lengths alone: the seam rule, unmasked steps
    tl = _trainer(_new_model(name, tc.P_DROP, dev), name)
    tl.fit(series, epochs=1, batch_size=16, shuffle=False, lengths=LENGTHS)
    th = _trainer(_new_model(name, tc.P_DROP, dev), name)
    seam = _dev(dev, fm.windows(N_ROWS, W8, F6, LENGTHS))
    assert seam.numel() == N_ROWS - W8 - 13
    for lo in range(0, seam.numel(), 16):
        th.step(series, seam[lo:lo + 16])
    assert torch.equal(tl.params, th.params)
    # shuffled: a permutation of the windows drawn on the device from the trainer's seed, reproducible
    o1 = _trainer(_new_model(name, tc.P_DROP, dev), name).fit(series, epochs=2, batch_size=16, lengths=LENGTHS, age=age_dev)
    t2 = _trainer(_new_model(name, tc.P_DROP, dev), name)
    o2 = t2.fit(series, epochs=2, batch_size=16, lengths=LENGTHS, age=age_dev)
    assert o1 == o2 and len(o1["train_total"]) == 2 and _record(t2.state)["calls"] == 2 * steps
    # no valid window
    with pytest.raises(ValueError, match="no window"):
        tr.fit(series, lengths=LENGTHS, age=age_dev, min_observed=1.0)


def test_fit_without_the_new_arguments_is_the_loop_it_was(gpu_device):
    dev = gpu_device
    series = _series(dev)
    n = N_ROWS - W8
    tr = _trainer(_new_model("dims3", tc.P_DROP, dev), "dims3")
    tr.fit(series, epochs=2, batch_size=32)
    tb = _trainer(_new_model("dims3", tc.P_DROP, dev), "dims3")
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    for _ in range(2):
        order = torch.randperm(n, device=dev, generator=gen)
        for lo in range(0, n, 32):
            tb.step(series, order[lo:lo + 32])
    assert torch.equal(tb.params, tr.params) and np.array_equal(tb.losses(), tr.losses())


# ---- 5. series_losses(age=) --------------------------------------------------------------------------------------------------------------------
def _eval_model(dev, name="dims3"):
    model = _new_model(name, 0.0, dev).eval()
    return model, STEP_MODELS[name]["target_dims"]


def _check_losses(res, preds, recons, ser, starts, age, cols, W, out, batch_size, what):
    n = len(starts)
    ws = fm.window_sums(preds, recons, ser, starts, age, 0, cols)
    got_w, got_c = res.window_sse.cpu().numpy(), res.window_count.cpu().numpy()
    assert got_w.shape == (n, 2) and np.array_equal(got_c, ws[:, 2:]), what
    _rel(got_w[:, 0], ws[:, 0], loss_refs.bound(out), (what, "S_f"))
    _rel(got_w[:, 1], ws[:, 1], loss_refs.bound(W * out), (what, "S_r"))
    f, r, t = fm.group_losses(ws, batch_size)
    group = n if batch_size is None else batch_size
    _rel([res.forecast_loss, res.recon_loss], [f, r], loss_refs.bound(W * out + group) / 2 + 2 * REL64, (what, "losses"))
    assert res.total_loss == res.forecast_loss + res.recon_loss and res.n_windows == n
    ds = fm.dim_sums(preds, recons, ser, starts, age, 0, cols)
    with np.errstate(all="ignore"):
        want_d = np.where(ds[2:] > 0, ds[:2] / ds[2:], np.nan)
    _rel(res.dim_mse.cpu().numpy(), want_d, loss_refs.bound(n * W + 4) + REL64, (what, "dim_mse"))
    return ws


@pytest.mark.parametrize("batch_size", [None, 16, 4])
def test_series_losses_with_age_against_the_reference(batch_size, gpu_device):
    dev = gpu_device
    model, cols = _eval_model(dev)
    series = _series(dev)                                                 # (finite everywhere: a filled value is still an input)
    age, age_dev = _reference_age(dev)
    n = N_ROWS - W8
    res = model.series_losses(series, target_dims=cols, batch_size=batch_size, age=age_dev)
    preds, recons, _ = model._engine.forward_series(series.contiguous(), count=n)
    ws = _check_losses(res, preds.cpu().numpy(), recons.cpu().numpy(), series.cpu().numpy(), np.arange(n), age, cols, W8, 3, batch_size,
                       f"batch_size={batch_size}")
    assert (ws[:, 2] == 0).any() and (ws[:, 2] == 3).any() and (ws[:, 3] < W8 * 3).any()
    if batch_size == 4:                                                   # windows 52 .. 55 ask for rows 60 .. 63 of the outage: no forecast term
        sums = loss_refs.group_sums(ws, 4)
        assert (sums[:, 2] == 0).sum() >= 1 and (sums[:, 2] > 0).any() and math.isfinite(res.forecast_loss)
    again = model.series_losses(series, target_dims=cols, batch_size=batch_size, age=age_dev)
    assert torch.equal(res.window_sse, again.window_sse) and (res.forecast_loss, res.recon_loss) == (again.forecast_loss, again.recon_loss)
    # no observed forecast term at all: NaN, the reconstruction's loss stays
    st = torch.tensor([52, 53, 54], dtype=torch.int64, device=dev)
    none = model.series_losses(series, target_dims=cols, starts=st, age=age_dev)
    assert math.isnan(none.forecast_loss) and math.isfinite(none.recon_loss) and torch.isnan(none.dim_mse[0]).all()


@pytest.mark.parametrize("name", ["dims3", "all"])
def test_series_losses_all_observed_equals_the_unmasked_call(name, gpu_device):
    dev = gpu_device
    model, cols = _eval_model(dev, name)
    out = _kwargs(name, 0.0)["out_dim"]
    series = _series(dev)
    zero = torch.zeros((N_ROWS, F6), dtype=torch.int32, device=dev)
    for batch_size in (None, 16):
        plain = model.series_losses(series, target_dims=cols, batch_size=batch_size)
        masked = model.series_losses(series, target_dims=cols, batch_size=batch_size, age=zero)
        assert (plain.forecast_loss, plain.recon_loss, plain.total_loss) == (masked.forecast_loss, masked.recon_loss, masked.total_loss)
        assert np.array_equal(_bits(plain.window_sse), _bits(masked.window_sse)) and np.array_equal(_bits(plain.dim_mse), _bits(masked.dim_mse))
        assert plain.window_count is None and (masked.window_count[:, 0] == out).all() and (masked.window_count[:, 1] == W8 * out).all()


@pytest.mark.parametrize("n", [63, 65])
def test_series_losses_with_age_around_a_chunk(n, gpu_device):
    """One window below and above a chunk of 64 windows, forced as tests/test_gpu_losses.py forces it."""
    dev = gpu_device
    model, cols = _eval_model(dev)
    series = _series(dev)
    age, age_dev = _reference_age(dev)
    whole = model.series_losses(series, target_dims=cols, count=n, age=age_dev)
    eng = model._engine
    before = eng.chunk_windows()
    eng.set_chunk_windows(64)
    try:
        assert eng.series_losses_chunk() == 64
        res = model.series_losses(series, target_dims=cols, count=n, batch_size=16, age=age_dev)
        cuts = [eng.forward_series(series.contiguous(), start0=c0, count=min(64, n - c0)) for c0 in range(0, n, 64)]
        preds, recons = (torch.cat([c[j] for c in cuts]) for j in (0, 1))       # every chunk's windows called on their own
        ws_bytes = eng.lib.mtadgat_series_losses_masked_workspace_bytes
        assert ws_bytes(eng.handle, 4 * 64) == ws_bytes(eng.handle, 64) > 0
    finally:
        eng.set_chunk_windows(before)
    _check_losses(res, preds.cpu().numpy(), recons.cpu().numpy(), series.cpu().numpy(), np.arange(n), age, cols, W8, 3, 16, f"chunks n={n}")
    assert torch.equal(res.window_count, whole.window_count)             # (the counts do not depend on the forward's route)


# ---- 6. guard bands -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,ld", [(6, 6), (5, 8)])
def test_guard_bands_of_the_sampler(F, ld, gpu_device, monkeypatch):
    import _native
    n_rows, parts = 1500, 7
    rng = np.random.default_rng(F)
    lengths = rng.multinomial(n_rows, np.full(parts, 1.0 / parts)).tolist()
    age = fm.age_of(rng.random((n_rows, F)) < 0.3, lengths)
    inputs = {"age": _dev(gpu_device, age), "dims": torch.tensor([F - 1, 0], dtype=torch.int32, device=gpu_device),
              "offsets": _dev(gpu_device, fm.part_offsets(lengths, n_rows))}

    def call(ins):
        starts, count = _native.fit_windows(n_rows, W8, F, gpu_device, age=ins["age"], dims=ins["dims"], offsets=ins["offsets"], min_count=20)
        k = int(count.item())
        head = starts[:k].clone()
        assert np.array_equal(head.cpu().numpy(), fm.windows(n_rows, W8, F, lengths, age, 0, [F - 1, 0], 20))
        return {"count": count, "head": head, "starts": starts}          # (the tail beyond count is not written: it keeps the pattern)

    def tail_untouched(got, ordinary, what):
        k = fm.windows(n_rows, W8, F, lengths, age, 0, [F - 1, 0], 20).size
        tail = got[k:].view(torch.int32)
        assert tail.numel() > 0 and (tail == tail[0]).all(), what
    four_calls(monkeypatch, gpu_device, [], inputs, call, f"fit_windows F={F} ld={ld}", finite=False, layout={"age": ld} if ld != F else None,
               compare={"starts": tail_untouched})


@pytest.mark.parametrize("F,ld,out", [(7, 7, 5), (7, 10, 5), (300, 303, 300)])
def test_guard_bands_of_the_masked_calls(F, ld, out, gpu_device, monkeypatch):
    import _native
    import evaluation
    rng = np.random.default_rng(F + out)
    W, batch = (10, 33) if out == 5 else (3, 5)
    n_rows = 3 * W + 30
    series, age = _gappy(rng, n_rows, F)
    series = _hide(series, age)
    dims = rng.permutation(F)[:out].astype(np.int32)
    inputs = {"preds": _dev(gpu_device, rng.standard_normal((batch, out)).astype(np.float32)),
              "recons": _dev(gpu_device, rng.standard_normal((batch, W, out)).astype(np.float32)), "series": _dev(gpu_device, series),
              "age": _dev(gpu_device, age), "starts": _dev(gpu_device, _starts(rng, n_rows, W, batch)), "dims": _dev(gpu_device, dims)}

    def call(ins):
        window, dim = _native.fit_masked_sse(ins["preds"], ins["recons"], ins["series"], ins["starts"], ins["age"], dims=ins["dims"])
        sums = evaluation.group_sums(window, batch)
        dp, dr, rmse = _native.fit_masked_loss_grad(ins["preds"], ins["recons"], ins["series"], ins["starts"], ins["age"], sums.reshape(4),
                                                    dims=ins["dims"])
        return {"window": window, "dim": dim, "sums": sums, "d_preds": dp, "d_recons": dr, "rmse": rmse}
    ref, _ = four_calls(monkeypatch, gpu_device, [], inputs, call, f"masked calls F={F} ld={ld} out={out}", finite=True,
                        layout={"series": ld, "age": ld} if ld != F else None)
    assert ref["d_recons"].abs().max() > 0 and (ref["window"][:, 3] < W * out).any()


def _refusals(lib, t, device):
    n, Wn, d = 3000, 5, 3
    b = n - Wn - 1
    p = lambda a: a.data_ptr()                                                                                        # noqa: E731
    i64, f64, f32, i32 = torch.int64, torch.float64, torch.float32, torch.int32
    stream = torch.cuda.current_stream(device).cuda_stream
    return {
        "fit_windows": (8, lib.mtadgat_fit_windows_scratch(n),
                        lambda s, nb: lib.mtadgat_fit_windows(p(t("age", (n, d), i32, 0)), d, 0, n, d, Wn, None, d, None, 1, 4, p(t("starts", (n - Wn,), i64)),
                                                              p(t("count", (1,), i64)), s, nb, stream)),
        "fit_masked_sse": (16, lib.mtadgat_fit_masked_sse_scratch(b, d),
                           lambda s, nb: lib.mtadgat_fit_masked_sse(p(t("preds", (b, d), f32, 0.5)), p(t("recons", (b, Wn, d), f32, 0.5)), b, Wn, d,
                                                                    p(t("series", (n, d), f32, 0.25)), n, d, d, None, 0, 1, None,
                                                                    p(t("age", (n, d), i32, 0)), d, 0, 0, p(t("window", (b, 4), f64)),
                                                                    p(t("dim", (4, d), f64)), s, nb, stream)),
    }


@pytest.mark.parametrize("entry", ["fit_windows", "fit_masked_sse"])
def test_short_or_misaligned_scratch_is_refused_before_anything_launches(entry, gpu_device):
    import _native
    refuse_scratch(_native.load_library(), _refusals, entry, gpu_device)


# ---- 7. refused arguments ----------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(gpu_device):
    import fitting
    dev = gpu_device
    model = _new_model("dims3", 0.0, dev)
    tr = _trainer(model, "dims3")
    series = _series(dev)
    starts = torch.zeros(3, dtype=torch.int64, device=dev)
    good = torch.zeros((N_ROWS, F6), dtype=torch.int32, device=dev)
    bad_ages = {"dtype": good.to(torch.int64), "bool": good == 0, "device": good.cpu(), "rows": good[:-1], "columns": good[:, :5],
                "transposed": torch.zeros((F6, N_ROWS), dtype=torch.int32, device=dev).t(), "1-D": good.reshape(-1)}
    for what, age in bad_ages.items():
        with pytest.raises(RuntimeError):
            tr.step(series, starts, age=age)
        with pytest.raises(RuntimeError):
            fitting.training_windows(N_ROWS, W8, F6, age=age, device=dev)
        with pytest.raises(RuntimeError):
            model.series_losses(series, target_dims=[4, 0, 2], age=age)
    assert _record(tr.state)["calls"] == 0                               # nothing ran
    for lengths in ([31, 5, 43], [80, 1], [], [40.5, 39.5], [-1, 81]):
        with pytest.raises(ValueError):
            fitting.training_windows(N_ROWS, W8, F6, lengths=lengths, device=dev)
        with pytest.raises(ValueError):
            tr.fit(series, lengths=lengths)
    for m in (-0.01, 1.01):
        with pytest.raises(ValueError, match="min_observed"):
            fitting.training_windows(N_ROWS, W8, F6, min_observed=m, device=dev)
        with pytest.raises(ValueError, match="min_observed"):
            tr.fit(series, age=good, min_observed=m)
    with pytest.raises(ValueError):
        fitting.training_windows(W8, W8, F6, device=dev)                  # no target row
    with pytest.raises(IndexError):
        fitting.training_windows(N_ROWS, W8, F6, target_dims=[6], device=dev)
    with pytest.raises(RuntimeError, match="GPU"):
        model.cpu().series_losses(series.cpu(), target_dims=[4, 0, 2], age=good.cpu())
