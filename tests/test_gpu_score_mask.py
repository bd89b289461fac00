"""Scoring a gappy series on the device (csrc/mtadgat_evalmask.hip and the NaN-skipping instantiation of the column select in
csrc/mtadgat_evalcol.hip, through evaluation.py and MTAD_GAT.anomaly_scores(age=)) against tests/score_mask_refs.py, which
tests/test_host_score_mask.py holds against pandas, numpy and the unmasked references.

Gates
  scored rows, NaN patterns, counts: exact.
  masked scores:  |per_dim - ref| <= 2^-22 |ref| (two float32 roundings, contracted or not, the subtractions done in float32 in the
                  reference as in the kernel); |global - ref| <= (d + 4) 2^-23 |ref| (a sequential float32 sum of d non-negative terms
                  and the division).
  quantiles:      1 float32 ulp of the reference (tests/test_gpu_score_pipeline.py); q = 0 and q = 1 are the valid minimum and maximum
                  bit for bit.
  moving average: 2^-23 |ref| + 1e-30 at the observed rows (tests/test_gpu_score_pipeline.py).
  moments:        eval_refs.check_sums; thresholds: 1e-9 relative (tests/test_gpu_score_pipeline.py); the cases' margin is held in
                  tests/test_host_score_mask.py.
  scaled scores:  (a - med) / (1 + q75 - q25) in float32 from quantiles that are each within one ulp: with den = 1 + q75 - q25 >= 1,
                  |got - ref| <= 2^-22 (|a| + |med|) / den + 2^-21 |ref| (1 + |q25| + |q75|) -- the numerator's two roundings and the
                  median's ulp; the denominator's two roundings and two ulps, relative to den >= 1; the division.
  row means of scaled (signed) scores: (d + 4) 2^-23 sum |term| / count.
Every call is made twice where the issue of reproducibility arises: equal bits."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import eval_refs as er
import score_mask_refs as spec
import score_refs
from test_host_score_mask import EPSILON_CASES, bursty, planted

pytestmark = pytest.mark.gpu

QS = [0.0, 0.25, 0.5, 0.75, 1.0]
GAPS = (0.0, 0.15, 0.6)
_dp = ctypes.POINTER(ctypes.c_double)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _age(n_rows, F, p, rng, lengths=None):
    import fit_mask_refs
    return fit_mask_refs.age_of(rng.random((n_rows, F)) < p, lengths)


# ---- which scores exist -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,W,F", [(8, 7, 1), (3, 1, 5), (300, 12, 5), (1100, 7, 38), (2100, 12, 5)])
def test_scored_rows(n_rows, W, F, gpu_device):
    import evaluation as ev
    import fitting
    rng = np.random.default_rng(n_rows + F)
    third = n_rows // 3
    short = min(W, n_rows - third)                                     # a part shorter than W + 1: no score targets it
    for p in GAPS:
        for lengths in (None, [third, short, n_rows - third - short]):
            age = _age(n_rows, F, p, rng, lengths)
            age_t = _dev(age, gpu_device)
            for dims in (None, [F - 1, 0] if F > 1 else [0]):
                for mo in (0.0, 0.5, 1.0):
                    keep = ev.scored_rows(n_rows, W, F, age_t, max_age=0, min_observed=mo, target_dims=dims, lengths=lengths)
                    assert keep.dtype == torch.uint8 and tuple(keep.shape) == (n_rows - W,) and keep.device.type == "cuda"
                    want = spec.scored_rows(n_rows, W, F, age, 0, mo, dims, lengths)
                    assert np.array_equal(keep.cpu().numpy(), want), (p, lengths, dims, mo)
                    starts = fitting.training_windows(n_rows, W, F, lengths=lengths, age=age_t, max_age=0, min_observed=mo, target_dims=dims)
                    assert torch.equal(keep.nonzero().flatten(), starts), (p, lengths, dims, mo)
    age = _age(n_rows, F, 0.6, rng)
    got = ev.scored_rows(n_rows, W, F, _dev(age, gpu_device), max_age=2, min_observed=0.5)
    assert np.array_equal(got.cpu().numpy(), spec.scored_rows(n_rows, W, F, age, 2, 0.5))


def test_scored_rows_checks_its_arguments(gpu_device):
    import evaluation as ev
    age = torch.zeros((20, 3), dtype=torch.int32, device=gpu_device)
    with pytest.raises(ValueError):
        ev.scored_rows(20, 20, 3, age)
    with pytest.raises(ValueError):
        ev.scored_rows(20, 5, 3, age, lengths=[10, 9])
    with pytest.raises(RuntimeError):
        ev.scored_rows(20, 5, 3, age.cpu())
    with pytest.raises(RuntimeError):
        ev.scored_rows(20, 5, 3, age.long())
    with pytest.raises(IndexError):
        ev.scored_rows(20, 5, 3, age, target_dims=[3])


# ---- masked scores ------------------------------------------------------------------------------------------------------------------
def _assert_masked(got, ref, d, what):
    glob, per_dim, count = (t.cpu().numpy() for t in got)
    ref_pd, ref_glob, ref_count = ref
    assert np.array_equal(count, ref_count), (what, "count")
    assert np.array_equal(np.isnan(per_dim), np.isnan(ref_pd)), (what, "per_dim NaN pattern")
    assert np.array_equal(np.isnan(glob), np.isnan(ref_glob)), (what, "global NaN pattern")
    ok = ~np.isnan(ref_pd)
    err = np.abs(per_dim.astype(np.float64)[ok] - ref_pd[ok])
    assert np.all(err <= 2.0 ** -22 * np.abs(ref_pd[ok])), (what, "per_dim")
    ok = ~np.isnan(ref_glob)
    err = np.abs(glob.astype(np.float64)[ok] - ref_glob[ok])
    assert np.all(err <= (d + 4) * 2.0 ** -23 * np.abs(ref_glob[ok])), (what, "global")
    # the canonical quiet NaN
    nan_bits = np.concatenate([per_dim.view(np.uint32)[np.isnan(per_dim)], glob.view(np.uint32)[np.isnan(glob)]])
    assert np.all(nan_bits == 0x7fc00000), what


@pytest.mark.parametrize("gamma", [1.0, 0.37])
@pytest.mark.parametrize("d", [1, 3, 38, 65])
@pytest.mark.parametrize("n", [1, 255, 257, 1025])
def test_masked_scores(n, d, gamma, gpu_device):
    import evaluation as ev
    W, F = 7, d + 5
    rng = np.random.default_rng(1000 * n + d)
    preds, recons = rng.random((n, d)).astype(np.float32), rng.random((n, d)).astype(np.float32)
    values = rng.random((W + n, F)).astype(np.float32)
    dims = [int(c) for c in rng.permutation(F)[:d]]
    for p in GAPS:
        age = (rng.random((W + n, F)) < p).astype(np.int32) * rng.integers(1, 4, (W + n, F)).astype(np.int32)
        age[W + n // 3] = 2                                            # one fully unobserved row
        planted_values = values.copy()
        under = age > 0
        planted_values[under] = np.where(rng.random(int(under.sum())) < 0.5, np.nan, np.inf).astype(np.float32)
        keep = np.ones(n, np.uint8)
        if n > 1:
            keep[n // 2] = 0                                           # one row that is not kept
        wide_age = torch.full((W + n, F + 3), 9, dtype=torch.int32, device=gpu_device)
        wide_age[:, :F] = _dev(age, gpu_device)
        age_t = wide_age[:, :F]
        assert age_t.stride(0) > F
        args = (_dev(preds, gpu_device), _dev(recons, gpu_device), _dev(planted_values, gpu_device), W)
        for k in (keep, None, np.zeros(n, np.uint8)):
            got = ev.anomaly_scores(*args, target_dims=dims, gamma=gamma, age=age_t, max_age=0, keep=None if k is None else _dev(k, gpu_device))
            ref = spec.scores_masked(preds, recons, planted_values[W:], age[W:], 0, k, dims, gamma)
            _assert_masked(got, ref, d, (n, d, gamma, p, None if k is None else int(k.sum())))
            assert got[2].dtype == torch.int32
        assert int(got[2].sum()) == 0 and bool(torch.isnan(got[0]).all())
    # everything observed and kept: the plain call's bits
    zero = torch.zeros((W + n, F), dtype=torch.int32, device=gpu_device)
    args = (_dev(preds, gpu_device), _dev(recons, gpu_device), _dev(values, gpu_device), W)
    glob, per_dim, count = ev.anomaly_scores(*args, target_dims=dims, gamma=gamma, age=zero, keep=torch.ones(n, dtype=torch.uint8, device=gpu_device))
    plain_glob, plain_pd = ev.anomaly_scores(*args, target_dims=dims, gamma=gamma)
    assert torch.equal(_bits(glob), _bits(plain_glob)) and torch.equal(_bits(per_dim), _bits(plain_pd))
    assert bool((count == d).all())


def test_masked_scores_check_their_arguments(gpu_device):
    import evaluation as ev
    p, r, v = (torch.rand(s, device=gpu_device) for s in ((10, 3), (10, 3), (17, 3)))
    age = torch.zeros((17, 3), dtype=torch.int32, device=gpu_device)
    with pytest.raises(ValueError):
        ev.anomaly_scores(p, r, v, 7, keep=torch.ones(10, dtype=torch.uint8, device=gpu_device))
    with pytest.raises(ValueError):
        ev.anomaly_scores(p, r, v, 7, age=age, keep=torch.ones(9, dtype=torch.uint8, device=gpu_device))
    with pytest.raises(RuntimeError):
        ev.anomaly_scores(p, r, v, 7, age=age[:16])
    assert len(ev.anomaly_scores(p, r, v, 7, age=age)) == 3 and len(ev.anomaly_scores(p, r, v, 7)) == 2


# ---- quantiles ----------------------------------------------------------------------------------------------------------------------
def _assert_valid_quantiles(got, a, what):
    ref, _ = spec.nan_quantile(a, QS)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", got, ref)
    same_inf = np.isinf(ref) & (got == ref)
    fin = ~nan & ~same_inf
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= score_refs.ulp32(ref[fin])), (what, float(err.max()))


@pytest.mark.parametrize("layout", ["contiguous", "sliced"])
@pytest.mark.parametrize("d", [1, 3, 9, 65])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 4099])
def test_valid_quantiles(n, d, layout, gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(1000 * n + d)
    for p in GAPS:
        for rot in range(5 if d < 5 else 1):
            a = score_refs.columns(n, d, rng, rot)
            clean = a.copy()
            a[rng.random((n, d)) < p] = np.nan
            if p > 0:
                a[:, 0] = np.nan                                          # one column without a valid entry
                if d > 1:
                    a[:, 1] = np.nan                                      # and one with exactly one
                    a[n // 2, 1] = clean[n // 2, 1]
                bits = a.view(np.uint32)
                where = np.argwhere(np.isnan(a))
                for k, (i, j) in enumerate(where[::3]):
                    bits[i, j] = 0xffc00000 if k % 2 else 0x7fc12345     # the sign bit set; a payload that is not the canonical one
            if layout == "contiguous":
                t = _dev(a, gpu_device)
            else:
                wide = torch.full((n, d + 5), -7.0, device=gpu_device)
                wide[:, 2:2 + d] = _dev(a, gpu_device)
                t = wide[:, 2:2 + d]
                assert t.stride(0) == d + 5
            got, counts = ev.column_quantiles(t, QS, skip_nan=True, return_counts=True)
            what = (n, d, layout, p, rot)
            _assert_valid_quantiles(got, a, what)
            assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), (~np.isnan(a)).sum(axis=0)), what
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                          # (all-NaN columns)
                lo, hi = np.nanmin(a, axis=0), np.nanmax(a, axis=0)
            cols = ~np.isinf(a).any(axis=0) & ~np.isnan(a).all(axis=0)
            assert torch.equal(got[0].cpu()[cols], torch.from_numpy(lo)[cols]), (what, "minimum")
            assert torch.equal(got[-1].cpu()[cols], torch.from_numpy(hi)[cols]), (what, "maximum")
            again = ev.column_quantiles(t, QS, skip_nan=True)
            assert torch.equal(_bits(got), _bits(again)), what
            if p == 0:
                assert torch.equal(_bits(got), _bits(ev.column_quantiles(t, QS))), (what, "the plain call")
    with pytest.raises(ValueError):
        ev.column_quantiles(t, QS, return_counts=True)


def test_scale_scores_skips_nan(gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(7)
    a = (rng.random((1001, 7)) * 3.0).astype(np.float32)
    a[rng.random(a.shape) < 0.3] = np.nan
    a[:, 6] = np.nan
    got = ev.scale_scores(_dev(a, gpu_device), skip_nan=True).cpu().numpy()
    _assert_scaled(got, a, "scale_scores")
    with pytest.raises(ValueError):
        ev.scale_scores(_dev(a, gpu_device), parts=ev.score_parts([1001 + 5], 5), skip_nan=True)


def _assert_scaled(got, a, what):
    q, _ = spec.nan_quantile(a, [0.25, 0.5, 0.75])
    ref = spec.scale_valid(a)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isnan(got), np.isnan(a)), what
    den = 1.0 + (q[2] - q[0])
    with np.errstate(invalid="ignore"):
        bound = 2.0 ** -22 * (np.abs(a.astype(np.float64)) + np.abs(q[1])) / den + 2.0 ** -21 * np.abs(ref) * (1.0 + np.abs(q[0]) + np.abs(q[2]))
    ok = ~np.isnan(ref)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err[ok] <= bound[ok]), (what, float((err[ok] / bound[ok]).max()))


# ---- moving average -------------------------------------------------------------------------------------------------------------------
def _missing(kind, n, rng):
    m = np.zeros(n, dtype=bool)
    if kind == "iid 0.15":
        m = rng.random(n) < 0.15
    elif kind == "iid 0.6":
        m = rng.random(n) < 0.6
    elif kind == "first 300":
        m[:300] = True
    elif kind == "gap 2500":                     # more than two chunks and, for span 2, past the underflow of b^gap
        m[n // 8:n // 8 + 2500] = True
    elif kind == "all":
        m[:] = True
    return m


def _assert_ewm_valid(got, x, span, what):
    ref = spec.ewm_valid(x, span)
    obs = ~np.isnan(x)
    g = got.cpu().numpy()
    assert np.array_equal(np.isnan(g), ~obs), (what, "NaN pattern")
    assert np.all(g.view(np.uint32)[~obs] == 0x7fc00000), (what, "canonical NaN")
    err = np.abs(g.astype(np.float64)[obs] - ref[obs])
    bound = 2.0 ** -23 * np.abs(ref[obs]) + 1e-30
    assert np.all(err <= bound), (what, float((err / bound).max()))


def _ewm_in_place(x, span, device):
    import _native
    import evaluation as ev
    lib = ev._lib()
    n = x.numel()
    scratch = _native._scratch(lib.mtadgat_eval_ewm_valid_scratch(n), device)
    with torch.cuda.device(device):
        rc = lib.mtadgat_eval_ewm_valid(x.data_ptr(), n, 2.0 / (span + 1.0), scratch.data_ptr(), scratch.numel() * 8, x.data_ptr(), ev._stream(x))
    assert rc == 0
    return x


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 1025, 4097, 70001])
def test_moving_average_over_observed_rows(n, gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(n)
    for kind in ("none", "iid 0.15", "iid 0.6", "first 300", "gap 2500", "all"):
        x = (rng.random(n) * 3.0).astype(np.float32)
        x[_missing(kind, n, rng)] = np.nan
        t = _dev(x, gpu_device)
        for span in (1, 2, 7, 1280):
            got = ev.moving_average(t, span, skip_nan=True)
            _assert_ewm_valid(got, x, span, (n, kind, span))
            assert torch.equal(_bits(got), _bits(ev.moving_average(t, span, skip_nan=True))), (n, kind, span, "two calls")
            assert torch.equal(_bits(got), _bits(_ewm_in_place(t.clone(), span, gpu_device))), (n, kind, span, "in place")
            if kind == "none":
                plain = ev.moving_average(t, span).cpu().numpy().astype(np.float64)
                err = np.abs(got.cpu().numpy().astype(np.float64) - plain)
                assert np.all(err <= 2.0 ** -23 * np.abs(plain) + 1e-30), (n, span, "the plain call")
    with pytest.raises(ValueError):
        ev.moving_average(t, 7, parts=ev.score_parts([n + 3], 3), skip_nan=True)


# ---- moments and thresholds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 65])
@pytest.mark.parametrize("n", [1, 257, 1023, 1025, 4099])
def test_valid_moments(n, d, gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(100 * n + d)
    for p in GAPS:
        e = er.moment_columns(n, d, seed=n + d)
        e[rng.random((n, d)) < p] = np.nan
        if p > 0:
            e[:, d - 1] = np.nan
        wide = torch.full((n, d + 3), float("nan"), device=gpu_device)
        wide[:, 1:1 + d] = _dev(e, gpu_device)
        for t in (_dev(e, gpu_device), wide[:, 1:1 + d]):
            got = ev.moments_valid(t)
            ref = spec.moments_valid(e)
            assert got.shape == (d, 3) and np.array_equal(got[:, 2], ref[:, 2]), (n, d, p)
            for c in range(d):
                v = e[~np.isnan(e[:, c]), c]
                m = int(ref[c, 2])
                er.check_sums([got[c, 0]], [ref[c, 0]], m, er.abs_sum(v))
                er.check_sums([got[c, 1]], [ref[c, 1]], m, ref[c, 1])
            assert np.array_equal(got, ev.moments_valid(t)), (n, d, p, "two calls")


@pytest.mark.parametrize("n,d,seed", EPSILON_CASES)
def test_find_epsilon_skips_nan(n, d, seed, gpu_device):
    import evaluation as ev
    clean, e = bursty(n, d, seed), planted(n, d, seed)
    t = _dev(e, gpu_device)
    for reg in (0, 1, 2):
        got = ev.find_epsilon_columns(t, reg_level=reg, skip_nan=True)
        for c in range(d):
            ref = spec.find_epsilon_valid(e[:, c], reg)
            one = ev.find_epsilon(_dev(e[:, c].copy(), gpu_device), reg, skip_nan=True)
            if np.isnan(ref):
                assert d >= 2 and c == d - 1 and np.isnan(got[c]) and np.isnan(one)
                continue
            assert abs(got[c] - ref) <= 1e-9 * abs(ref), (c, reg, got[c], ref)
            assert abs(one - ref) <= 1e-9 * abs(ref), (c, reg, one, ref)
        # nothing missing: the plain call
        tc = _dev(clean, gpu_device)
        plain, valid = ev.find_epsilon_columns(tc, reg_level=reg), ev.find_epsilon_columns(tc, reg_level=reg, skip_nan=True)
        for c in range(d):
            assert abs(valid[c] - plain[c]) <= 1e-9 * abs(plain[c]), (c, reg, valid[c], plain[c])
    thr, preds = ev.feature_predictions(t, t, reg_level=1, skip_nan=True)
    want = (e.astype(np.float64) >= np.asarray(ev.find_epsilon_columns(t, 1, skip_nan=True))[None, :])      # (false for NaN on either side)
    assert np.array_equal(preds.cpu().numpy(), want.astype(np.uint8)) and (d < 2 or int(preds[:, d - 1].sum()) == 0)
    assert not preds.cpu().numpy()[np.isnan(e)].any()


def test_find_epsilon_falls_back_to_the_valid_maximum(gpu_device):
    import evaluation as ev
    e = np.full(400, 0.25, np.float32)                                   # constant: no z qualifies
    e[::7] = np.nan
    e[3] = 0.5
    e2 = np.stack([e, np.full(400, np.nan, np.float32)], axis=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = ev.find_epsilon_columns(_dev(e2, gpu_device), skip_nan=True)
        ref = spec.find_epsilon_valid(e)
    assert got[0] == ref or abs(got[0] - ref) <= 1e-9 * abs(ref)
    assert np.isnan(got[1])


# ---- model and pipeline -----------------------------------------------------------------------------------------------------------------
F_, W_ = 5, 12


@pytest.fixture(scope="module")
def gappy(gpu_device):
    import preparation
    from mtad_gat import MTAD_GAT
    torch.manual_seed(19)
    model = MTAD_GAT(n_features=F_, window_size=W_, out_dim=F_, kernel_size=3, gru_hid_dim=24, forecast_hid_dim=24,
                     recon_hid_dim=24).to(gpu_device).eval()
    rng = np.random.default_rng(20)

    def raw(n, spike):
        x = (np.sin(np.arange(n)[:, None] * (0.05 + 0.01 * np.arange(F_))) * 2.0 + rng.random((n, F_))).astype(np.float32)
        x[spike:spike + 9] += 4.0
        x[rng.random((n, F_)) < 0.15] = np.nan
        x[200:240, 1:3] = np.nan                                       # a 40-row drop-out of two sensors
        x[300:306] = np.nan                                            # and six rows without any sample: no target to score
        return _dev(x, gpu_device)
    train, test = raw(700, 500), raw(700, 420)
    scaler = preparation.fit_scaler(train, gaps="ignore")
    values, age = scaler.transform(train, fill="hold", return_age=True)
    with torch.no_grad():
        preds, recons = model.score_series(values)
    return dict(model=model, train=train, test=test, values=values, age=age, preds=preds, recons=recons)


def test_model_scores_stage_by_stage(gappy, gpu_device):
    model, values, age = gappy["model"], gappy["values"], gappy["age"]
    v, a = values.cpu().numpy(), age.cpu().numpy()
    p, r = gappy["preds"].cpu().numpy(), gappy["recons"].cpu().numpy()
    n = 700 - W_
    assert int((a > 0).sum()) > 400 and int((a[200:240, 1:3] > 0).all())
    with torch.no_grad():
        raw_glob, raw_pd = model.anomaly_scores(values, age=age, gamma=0.8)
        sc_glob, sc_pd = model.anomaly_scores(values, age=age, gamma=0.8, scale_scores=True)
        sm_glob, sm_pd = model.anomaly_scores(values, age=age, gamma=0.8, scale_scores=True, use_mov_av=True, smoothing_span=7)
    keep = spec.scored_rows(700, W_, F_, a)
    assert 0 < int(keep.sum()) < n
    ref = spec.scores_masked(p, r, v[W_:], a[W_:], 0, keep, None, 0.8)
    _assert_masked((raw_glob, raw_pd, torch.from_numpy(ref[2])), ref, F_, "model raw")
    assert np.array_equal(np.isnan(raw_glob.cpu().numpy()), keep == 0)
    # scaled from the device's own unscaled scores
    raw_np = raw_pd.cpu().numpy()
    _assert_scaled(sc_pd.cpu().numpy(), raw_np, "model scaled")
    sc_np = sc_pd.cpu().numpy()
    want = spec.row_means_valid(sc_np)
    cnt = (~np.isnan(sc_np)).sum(axis=1)
    got = sc_glob.cpu().numpy()
    assert np.array_equal(np.isnan(got), cnt == 0) and np.array_equal(np.isnan(got), keep == 0)
    ok = cnt > 0
    bound = (F_ + 4) * 2.0 ** -23 * np.nansum(np.abs(sc_np.astype(np.float64)), axis=1) / np.maximum(cnt, 1)
    assert np.all(np.abs(got.astype(np.float64) - want)[ok] <= bound[ok])
    # smoothed from the device's own scaled global scores; the per-dimension scores are never smoothed
    _assert_ewm_valid(sm_glob, got, 7, "model smoothed")
    assert torch.equal(_bits(sm_pd), _bits(sc_pd))
    # the composed specification agrees in its NaN pattern
    full, full_pd, full_keep = spec.anomaly_scores_masked(p, r, v, W_, a, gamma=0.8, scale=True, span=7)
    assert np.array_equal(np.isnan(full), np.isnan(sm_glob.cpu().numpy())) and np.array_equal(full_keep, keep)
    assert np.array_equal(np.isnan(full_pd), np.isnan(sc_np))


def test_model_scores_with_nothing_missing_and_with_parts(gappy, gpu_device):
    model, values, age = gappy["model"], gappy["values"], gappy["age"]
    zero = torch.zeros_like(age)
    with torch.no_grad():
        glob, per_dim = model.anomaly_scores(values, age=zero, min_observed=0)
        plain_glob, plain_pd = model.anomaly_scores(values)
    assert torch.equal(_bits(per_dim), _bits(plain_pd))                    # gamma = 1: a contracted 1 x + y rounds like x + y
    err = (glob.double() - plain_glob.double()).abs()
    assert bool((err <= (F_ + 4) * 2.0 ** -23 * plain_glob.double().abs()).all())
    # a concatenated series: the windows over a seam are unscored
    lengths = [300, 400]
    with torch.no_grad():
        seam, _ = model.anomaly_scores(values, age=zero, min_observed=0, lengths=lengths)
    nan = torch.isnan(seam).cpu().numpy()
    want = np.zeros(700 - W_, dtype=bool)
    want[300 - W_:300] = True
    assert np.array_equal(nan, want)
    import evaluation as ev
    with pytest.raises(ValueError):
        model.anomaly_scores(values, age=age, parts=ev.score_parts([700], W_))
    with pytest.raises(ValueError):
        model.anomaly_scores(values, age=age, scale_scores="per_part", parts=ev.score_parts([700], W_))
    with pytest.raises(ValueError):
        model.anomaly_scores(values, lengths=lengths)
    with pytest.raises(RuntimeError):
        model.anomaly_scores(values, age=age.cpu())


def test_predict_anomalies_with_a_mask(gappy, gpu_device):
    import evaluation as ev
    model, train, test = gappy["model"], gappy["train"], gappy["test"]
    labels = torch.zeros(700 - W_, dtype=torch.bool, device=gpu_device)
    labels[420 - W_:429 - W_] = True
    opts = dict(scale_scores=True, use_mov_av=True)
    with torch.no_grad():
        out = ev.predict_anomalies(model, train, test, labels=labels, prepare=dict(fill="hold", gaps="ignore"), mask={},
                                   events=dict(merge_gap=0), **opts)
        bare = ev.predict_anomalies(model, train, test, prepare=dict(fill="hold", gaps="ignore"), mask=dict(max_age=0, min_observed=0.5), **opts)
    assert set(out) == {"epsilon_result", "bf_result", "feature_thresholds", "train_scores", "test_scores", "test_per_dim", "feature_preds",
                        "scaler", "train_scored", "test_scored", "events"}
    assert torch.equal(_bits(out["test_scores"]), _bits(bare["test_scores"])) and bare["epsilon_result"] is None
    for name in ("train", "test"):
        scored, scores = out[f"{name}_scored"], out[f"{name}_scores"]
        assert scored.dtype == torch.uint8 and torch.equal(scored.bool(), ~torch.isnan(scores))
        assert 0 < int(scored.sum()) < scored.numel()
    # the thresholds: the specification on the device's own training scores
    values, age = out["scaler"].transform(train, fill="hold", return_age=True)
    with torch.no_grad():
        tr_glob, tr_pd = model.anomaly_scores(values, age=age, **opts)
    assert torch.equal(_bits(tr_glob), _bits(out["train_scores"]))
    ref = spec.find_epsilon_valid(tr_glob.cpu().numpy(), 1)
    thr = out["epsilon_result"]["threshold"]
    assert abs(thr - ref) <= 1e-9 * abs(ref), (thr, ref)
    tr_np = tr_pd.cpu().numpy()
    for c in range(F_):
        ref = spec.find_epsilon_valid(tr_np[:, c], 1)
        assert abs(out["feature_thresholds"][c] - ref) <= 1e-9 * abs(ref), (c, out["feature_thresholds"][c], ref)
    te_pd = out["test_per_dim"].cpu().numpy()
    want = te_pd.astype(np.float64) >= out["feature_thresholds"][None, :]
    assert np.array_equal(out["feature_preds"].cpu().numpy(), want.astype(np.uint8))
    assert not out["feature_preds"].cpu().numpy()[np.isnan(te_pd)].any()
    # events: an unscored row is never flagged, so with merge_gap = 0 no event holds one
    events, scored = out["events"], out["test_scored"].cpu().numpy()
    for s, e in zip(events["start"].tolist(), events["end"].tolist()):
        assert scored[s:e].all() and bool((out["test_scores"][s:e] > events["threshold"]).all())
    # what is refused, and why
    prep = dict(fill="hold")
    for kw, word in ((dict(mask={}), "prepare"), (dict(mask={}, prepare=prep, parts=dict(train_lengths=[700])), "parts"),
                     (dict(mask={}, prepare=prep, pot={}), "pot"), (dict(mask={}, prepare=prep, curves={}), "curves"),
                     (dict(mask=dict(age=1), prepare=prep), "max_age")):
        with pytest.raises(ValueError, match=word):
            ev.predict_anomalies(model, train, test, **kw)
