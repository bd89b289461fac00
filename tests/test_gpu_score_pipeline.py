"""The Predictor's score post-processing on the device (csrc/mtadgat_evalcol.hip and the column passes of mtadgat_eval.hip
through evaluation.py and MTAD_GAT.anomaly_scores): per-column quantiles, the exponentially weighted moving average,
per-feature thresholds, and predict_anomalies, against the float64 references of tests/score_refs.py and the CPU oracle.

Gates
  quantiles: |ours - ref| <= 1 float32 ulp of the reference (ours is rounded once from float64: half an ulp; the other
             half allows for the reference's own float64 rounding next to a tie); the order statistics themselves are exact.
  ewm:       |ours - ref64| <= 2^-23 |ref64| + 1e-30 (one float32 rounding plus float64 reassociation of about 1e-14).
"""
import numpy as np
import pytest
import torch

import score_refs
from oracle import eval_oracle as eo

pytestmark = pytest.mark.gpu

QS = [0.0, 0.25, 0.5, 0.75, 1.0]


def _assert_quantiles(got, a, qs, what):
    ref = score_refs.quantile(a, qs)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)                      # inf - inf / a NaN in the column: NaN in numpy too
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", got, ref)
    same_inf = np.isinf(ref) & (got == ref)
    fin = ~nan & ~same_inf
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= score_refs.ulp32(ref[fin])), (what, float(err.max()))


@pytest.mark.parametrize("layout", ["contiguous", "sliced"])
@pytest.mark.parametrize("d", [1, 3, 38, 65])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 4099])
def test_column_quantiles(n, d, layout, gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(1000 * n + d)
    for rot in range(5 if d < 5 else 1):                 # every column kind also where d < 5
        a = score_refs.columns(n, d, rng, rot)
        if layout == "contiguous":
            t = torch.from_numpy(a).to(gpu_device)
        else:
            wide = torch.full((n, d + 5), -7.0, device=gpu_device)      # the neighbours would change every quantile if they were read
            wide[:, 2:2 + d] = torch.from_numpy(a).to(gpu_device)
            t = wide[:, 2:2 + d]
            assert t.stride(0) == d + 5
        got = ev.column_quantiles(t, QS)
        _assert_quantiles(got, a, QS, (n, d, layout, rot))
        s = np.sort(a, axis=0)
        keep = ~np.isinf(s).any(axis=0)                  # a column holding inf: s[hi] - s[lo] is inf - inf at the top rank
        assert torch.equal(got[0].cpu()[keep], torch.from_numpy(s[0])[keep]), "minimum"
        assert torch.equal(got[-1].cpu()[keep], torch.from_numpy(s[-1])[keep]), "maximum"


@pytest.mark.parametrize("n", [3, 257, 4099])
def test_order_statistics_are_exact(n, gpu_device):
    """Probabilities whose position q (n - 1) is an integer in float64 return that order statistic bit for bit."""
    import evaluation as ev
    rng = np.random.default_rng(n)
    a = score_refs.columns(n, 9, rng)
    ks = [k for k in range(n) if np.floor(np.float64(k / (n - 1)) * np.float64(n - 1)) == k
          and np.float64(k / (n - 1)) * np.float64(n - 1) == k]
    if n > 300:
        ks = ks[::37] + ks[-3:]
    assert len(ks) >= 3
    got = ev.column_quantiles(torch.from_numpy(a).to(gpu_device), [k / (n - 1) for k in ks]).cpu()
    s = torch.from_numpy(np.sort(a, axis=0))
    for c in range(a.shape[1]):
        if np.isinf(a[:, c]).any():
            continue                                     # inf - inf in the interpolation, covered by test_column_quantiles
        assert torch.equal(got[:, c], s[ks, c]), (n, c)


def test_a_nan_poisons_its_column_only(gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(5)
    for n, d in ((1, 3), (257, 3), (4099, 38)):
        a = (rng.random((n, d)) * 3.0).astype(np.float32)
        a[n // 3, 1] = np.nan
        got = ev.column_quantiles(torch.from_numpy(a).to(gpu_device), QS)
        assert torch.isnan(got[:, 1]).all()
        _assert_quantiles(got, a, QS, (n, d))
        a[n // 3, 1] = -np.nan                           # sign bit set: sorts below -inf as a key
        got = ev.column_quantiles(torch.from_numpy(a).to(gpu_device), QS)
        _assert_quantiles(got, a, QS, (n, d, "negative NaN"))


def test_column_quantiles_are_bitwise_reproducible(gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(6)
    t = torch.from_numpy(score_refs.columns(4099, 38, rng)).to(gpu_device)
    first = ev.column_quantiles(t, QS)
    again = ev.column_quantiles(t, QS)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))


def test_scale_scores_follows_get_score(gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(7)
    a = (rng.random((1001, 7)) * 3.0).astype(np.float32)
    got = ev.scale_scores(torch.from_numpy(a).to(gpu_device)).cpu().numpy()
    q25, med, q75 = np.percentile(a.astype(np.float64), [25, 50, 75], axis=0)
    ref = (a - med) / (1 + (q75 - q25))
    assert np.abs(got - ref).max() <= 1e-6


def _ewm_inputs(n, rng):
    spike = np.zeros(n, np.float32)
    spike[n // 2] = 50.0
    return {"uniform": (rng.random(n) * 3.0).astype(np.float32), "constant": np.full(n, 1.25, np.float32), "spike": spike}


def _assert_ewm(got, x, span, what):
    ref = score_refs.ewm(x, span)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    bound = 2.0 ** -23 * np.abs(ref) + 1e-30
    assert np.all(err <= bound), (what, float((err / bound).max()))


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 1025, 4097, 70001])
def test_moving_average(n, gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(n)
    for kind, x in _ewm_inputs(n, rng).items():
        t = torch.from_numpy(x).to(gpu_device)
        for span in (1, 2, 7, 1280):
            got = ev.moving_average(t, span)
            _assert_ewm(got, x, span, (n, kind, span))
            again = ev.moving_average(t, span)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (n, kind, span)


def test_moving_average_rejects_bad_arguments(gpu_device):
    import evaluation as ev
    t = torch.rand(10, device=gpu_device)
    for span in (0, 0.5, -3):
        with pytest.raises(ValueError):
            ev.moving_average(t, span)
    with pytest.raises(RuntimeError):
        ev.moving_average(t.cpu(), 3)
    with pytest.raises(RuntimeError):
        ev.column_quantiles(torch.rand(10, 2), [0.5])
    with pytest.raises(ValueError):
        ev.column_quantiles(torch.rand(10, 2, device=gpu_device), [1.5])


def _bursty(n, d, seed):
    rng = np.random.default_rng(seed)
    e = (rng.random((n, d)) * 0.1).astype(np.float32)
    for c in range(d):
        for _ in range(3):
            at = int(rng.integers(0, n - 12))
            e[at:at + int(rng.integers(1, 12)), c] += np.float32(1.0 + 2.0 * rng.random())
    return e


@pytest.mark.parametrize("n,d", [(300, 1), (1000, 5), (5000, 38)])
def test_find_epsilon_columns(n, d, gpu_device):
    import evaluation as ev
    e = _bursty(n, d, 100 + d)
    wide = torch.zeros((n, d + 3), device=gpu_device)
    wide[:, 1:1 + d] = torch.from_numpy(e).to(gpu_device)
    for reg in (0, 1, 2):
        got = ev.find_epsilon_columns(torch.from_numpy(e).to(gpu_device), reg_level=reg)
        sliced = ev.find_epsilon_columns(wide[:, 1:1 + d], reg_level=reg)
        assert len(got) == d
        for c in range(d):
            ref = eo.find_epsilon(e[:, c], reg)
            one = ev.find_epsilon(torch.from_numpy(e[:, c].copy()).to(gpu_device), reg)
            assert abs(got[c] - ref) <= 1e-9 * abs(ref), (c, reg, got[c], ref)
            assert abs(got[c] - one) <= 1e-9 * abs(one), (c, reg, got[c], one)
            assert abs(sliced[c] - ref) <= 1e-9 * abs(ref), (c, reg, sliced[c], ref)


def test_find_epsilon_columns_degenerate_scores(gpu_device):
    """Constant columns, all zeros, and a column where no z qualifies (the column maximum is returned), as
    test_gpu_eval.py::test_find_epsilon_degenerate_scores asks of the 1-D function."""
    import warnings
    import evaluation as ev
    n = 4000
    e = np.zeros(n, np.float32)
    e[100], e[2000] = 3.0, -3.0
    cols = np.stack([np.full(n, 0.25, np.float32), np.zeros(n, np.float32), e, _bursty(n, 1, 3)[:, 0]], axis=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for reg in (0, 1, 2):
            got = ev.find_epsilon_columns(torch.from_numpy(cols).to(gpu_device), reg_level=reg)
            for c in range(cols.shape[1]):
                ref = eo.find_epsilon(cols[:, c], reg_level=reg)
                assert abs(got[c] - ref) <= 1e-6 * max(1.0, abs(ref)), (c, reg, got[c], ref)


def test_feature_predictions(gpu_device):
    import evaluation as ev
    train, test = _bursty(1000, 5, 21), _bursty(700, 5, 22)
    tr, te = torch.from_numpy(train).to(gpu_device), torch.from_numpy(test).to(gpu_device)
    thr, preds = ev.feature_predictions(tr, te, reg_level=1)
    assert thr.shape == (5,) and thr.dtype == np.float64
    assert list(thr) == ev.find_epsilon_columns(tr, reg_level=1) or np.allclose(thr, ev.find_epsilon_columns(tr, 1), rtol=1e-9, atol=0)
    assert preds.dtype == torch.uint8 and preds.shape == (700, 5) and preds.device.type == "cuda"
    assert np.array_equal(preds.cpu().numpy(), (test.astype(np.float64) >= thr[None, :]).astype(np.uint8))
    assert 0 < int(preds.sum()) < preds.numel()
    # `>=`: a score equal to its threshold is anomalous.  A constant training column has no qualifying z, so its threshold
    # is the column maximum, exactly 0.25.
    tr2, te2 = tr.clone(), te.clone()
    tr2[:, 3] = 0.25
    te2[:4, 3] = torch.tensor([0.25, 0.24999999, 0.25000003, 0.0], device=gpu_device)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        thr2, p2 = ev.feature_predictions(tr2, te2, reg_level=1)
    assert thr2[3] == 0.25 and p2[:4, 3].tolist() == [1, 0, 1, 0]


# ---- model level ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(gpu_device):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(9)
    model = MTAD_GAT(n_features=7, window_size=12, out_dim=7, kernel_size=3, gru_hid_dim=24, forecast_hid_dim=24,
                     recon_hid_dim=24).to(gpu_device).eval()
    g = torch.Generator().manual_seed(10)
    train = torch.rand(12 + 400, 7, generator=g)
    test = torch.rand(12 + 500, 7, generator=g)
    labels = torch.zeros(500, dtype=torch.bool)
    labels[60:85] = True
    labels[300:340] = True
    test[12 + 60:12 + 85] += 1.5                # what the model cannot forecast: high scores inside the labelled segments
    test[12 + 300:12 + 340, :3] -= 1.0
    return model, train.to(gpu_device), test.to(gpu_device), labels.to(gpu_device)


@pytest.mark.parametrize("scale", [False, True])
def test_anomaly_scores_moving_average(setup, scale, gpu_device):
    model, _, test, _ = setup
    with torch.no_grad():
        plain, per_dim = model.anomaly_scores(test, gamma=0.8, scale_scores=scale)
        for span in (5, 40):
            smooth, per_dim_s = model.anomaly_scores(test, gamma=0.8, scale_scores=scale, use_mov_av=True, smoothing_span=span)
            _assert_ewm(smooth, plain.cpu().numpy(), span, (scale, span))
            assert torch.equal(per_dim_s.view(torch.int32), per_dim.view(torch.int32))
        default, _ = model.anomaly_scores(test, gamma=0.8, scale_scores=scale, use_mov_av=True)
        assert int(256 * 12 * 0.05) == 153
        explicit, _ = model.anomaly_scores(test, gamma=0.8, scale_scores=scale, use_mov_av=True, smoothing_span=153)
        assert torch.equal(default.view(torch.int32), explicit.view(torch.int32))
        _assert_ewm(default, plain.cpu().numpy(), 153, (scale, "default span"))
        other, _ = model.anomaly_scores(test, gamma=0.8, scale_scores=scale, use_mov_av=True, smoothing_span=152)
        assert not torch.equal(default, other)
        # keyword defaults: today's results
        again, per_dim_again = model.anomaly_scores(test, None, 0.8, scale)
        assert torch.equal(again, plain) and torch.equal(per_dim_again, per_dim)
        with pytest.raises(ValueError):
            model.anomaly_scores(test, use_mov_av=True, smoothing_span=0)


def test_scaled_scores_follow_numpy_percentile(setup, gpu_device):
    model, _, test, _ = setup
    with torch.no_grad():
        _, raw = model.anomaly_scores(test, gamma=0.8)
        scores, per_dim = model.anomaly_scores(test, gamma=0.8, scale_scores=True)
    a = raw.cpu().numpy()
    q25, med, q75 = np.percentile(a, [25, 50, 75], axis=0)
    ref = (a - med) / (1 + (q75 - q25))
    assert np.abs(per_dim.cpu().numpy() - ref).max() <= 1e-6
    assert np.abs(scores.cpu().numpy() - ref.mean(1)).max() <= 1e-6


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k] or abs(a[k] - b[k]) <= 1e-9 * abs(b[k]), (k, a[k], b[k])


@pytest.mark.parametrize("options", [dict(), dict(scale_scores=True, use_mov_av=True, reg_level=0)])
def test_predict_anomalies(setup, options, gpu_device):
    import evaluation as ev
    model, train, test, labels = setup
    sweep = (0.01, 2.0, 50)
    with torch.no_grad():
        out = ev.predict_anomalies(model, train, test, labels=labels, gamma=0.8, bf_search=sweep, **options)
        score_kw = {k: v for k, v in options.items() if k != "reg_level"}
        tr_s, tr_pd = model.anomaly_scores(train, gamma=0.8, **score_kw)
        te_s, te_pd = model.anomaly_scores(test, gamma=0.8, **score_kw)
    reg = options.get("reg_level", 1)
    assert torch.equal(out["train_scores"], tr_s) and torch.equal(out["test_scores"], te_s) and torch.equal(out["test_per_dim"], te_pd)
    assert out["test_scores"].device.type == "cuda" and out["feature_preds"].device.type == "cuda"
    _same(out["epsilon_result"], ev.epsilon_eval(tr_s, te_s, labels, reg))
    _same(out["bf_result"], ev.bf_search(te_s, labels, *sweep))
    thr, preds = ev.feature_predictions(tr_pd, te_pd, reg)
    assert np.allclose(out["feature_thresholds"], thr, rtol=1e-9, atol=0)
    assert torch.equal(out["feature_preds"], preds)
    assert out["epsilon_result"]["TP"] + out["epsilon_result"]["FN"] == 65
    # without labels nothing is evaluated; without a sweep only the sweep is left out
    with torch.no_grad():
        bare = ev.predict_anomalies(model, train, test, gamma=0.8)
        half = ev.predict_anomalies(model, train, test, labels=labels, gamma=0.8)
    assert bare["epsilon_result"] is None and bare["bf_result"] is None and bare["feature_preds"].shape == (500, 7)
    assert half["epsilon_result"] is not None and half["bf_result"] is None
