"""Ranking curves on the device (csrc/mtadgat_curves.hip through evaluation.score_order, ranking_curve, ranking_metrics and
predict_anomalies(curves=...)) against the numpy specification of tests/curve_refs.py.

Gates
  orders, thresholds, tp, fp, the four counts, AUROC, the best point and its index: exact.
  average_precision: |ours - ref| <= 1e-12 ref.  The terms are non-negative and carry two roundings each, the device adds them in a
      fixed order whose longest chain has at most 4096 additions: (4096 + 2) 2^-53 = 4.6e-13 relative, one more rounding for the
      division by n_pos; the reference is an exactly rounded math.fsum.
"""
import json
import os

import numpy as np
import pytest
import torch

import curve_refs
import evaluation as ev

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE, LEVEL2 = ev._lib().mtadgat_eval_sort_tile(), ev._lib().mtadgat_eval_sort_scan_tiles()     # sizes are chosen around both
SIZES = sorted({1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 70001, TILE * LEVEL2 + 1})
ADJUSTS = [None, "point", ("k", 0), ("k", 30), ("k", 100)]
SPECIALS = (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, 0.5, np.nextafter(np.float32(0.5), np.float32(1)),
            np.nextafter(np.float32(0.5), np.float32(0)), np.nan, np.inf, -0.0, np.finfo(np.float32).max, -np.finfo(np.float32).max)


def _special(n, rng):
    x = rng.random(n).astype(np.float32) - np.float32(0.5)
    for j, v in enumerate(SPECIALS):
        x[(j * 37 + 5) % n] = v
    return x


def _order_inputs(n, rng):
    noise = rng.random(n).astype(np.float32)
    ramp = np.sort(noise)
    return {"noise": noise, "equal": np.full(n, 0.25, np.float32), "three": rng.integers(0, 3, n).astype(np.float32),
            "seventeen": (rng.integers(0, 17, n) - 8).astype(np.float32), "sorted": ramp, "reversed": ramp[::-1].copy(),
            "special": _special(n, rng)}


def test_sizes_straddle_the_sort_paths():
    assert TILE >= 256 and LEVEL2 >= 1 and TILE * LEVEL2 + 1 in SIZES and max(SIZES) > TILE * LEVEL2


@pytest.mark.parametrize("n", SIZES)
def test_score_order(n, gpu_device):
    rng = np.random.default_rng(n)
    for kind, x in _order_inputs(n, rng).items():
        t = torch.from_numpy(x).to(gpu_device)
        for descending in (True, False):
            got = ev.score_order(t, descending=descending)
            assert got.dtype == torch.int64 and got.device.type == "cuda" and got.shape == (n,)
            assert np.array_equal(got.cpu().numpy(), curve_refs.score_order(x, descending)), (n, kind, descending)
    assert torch.equal(ev.score_order(t), ev.score_order(t, descending=True))


def _scores(n, rng):
    """Ties, signed zeros, a few NaN and infinities."""
    s = (rng.integers(0, 41, n) / np.float32(40) - np.float32(0.25)).astype(np.float32)
    fine = rng.random(n) < 0.3
    s[fine] = rng.random(int(fine.sum())).astype(np.float32)
    for j, v in enumerate((np.nan, -0.0, 0.0, np.inf, -np.inf, np.nan)):
        s[(j * 53 + 11) % n] = v
    return s


def _label_layouts(n, rng, s):
    """kind -> labels; `mixed` changes s in place where it needs an all-NaN segment."""
    mixed = np.convolve(rng.random(n + 8), np.ones(9) / 9.0, mode="valid")[:n] > 0.56
    mixed[::97] = ~mixed[::97]                              # segments (and gaps) of length 1
    for c in range(TILE, n, TILE):                          # a segment across every tile boundary
        mixed[c - 3:c + 3] = True
    mixed[0] = mixed[n - 1] = True                          # segments at index 0 and at the last index
    if n > 40:
        mixed[19], mixed[20:24], mixed[24] = False, True, False
        s[20:24] = np.nan                                   # an all-NaN segment
        mixed[29], mixed[30:36], mixed[36] = False, True, False
        s[31], s[33] = np.nan, np.nan                       # a segment with fewer numbers than samples
    if n > 2:
        mixed[n // 2] = False
    return {"mixed": mixed, "none": np.zeros(n, bool), "all": np.ones(n, bool)}


def _assert_curve(got, ref, what):
    assert got["thresholds"].dtype == torch.float32 and got["tp"].dtype == torch.int64 and got["fp"].dtype == torch.int64, what
    assert got["thresholds"].device.type == "cuda" and got["tp"].device.type == "cuda"
    thr = got["thresholds"].cpu().numpy()
    assert thr.shape == ref["thresholds"].shape, (what, thr.shape, ref["thresholds"].shape)
    assert np.array_equal(thr.view(np.uint32), ref["thresholds"].view(np.uint32)), what
    assert np.array_equal(got["tp"].cpu().numpy(), ref["tp"]) and np.array_equal(got["fp"].cpu().numpy(), ref["fp"]), what
    for k in ("n_pos", "n_neg", "nan_pos", "nan_neg"):
        assert isinstance(got[k], int) and got[k] == ref[k], (what, k)


def _assert_metrics(got, ref, what):
    if np.isnan(ref["auroc"]):
        assert np.isnan(got["auroc"]), what
    else:
        assert got["auroc"] == ref["auroc"], what
    if np.isnan(ref["average_precision"]):
        assert np.isnan(got["average_precision"]), what
    else:
        assert abs(got["average_precision"] - ref["average_precision"]) <= 1e-12 * ref["average_precision"], what
    assert got["best_index"] == ref["best_index"], (what, got["best_index"], ref["best_index"])
    best = None if got["best"] is None else {k: v for k, v in got["best"].items() if k != "latency"}
    assert best == ref["best"], (what, best, ref["best"])
    for k in ("n_thresholds", "n_pos", "n_neg", "adjust"):
        assert got[k] == ref[k], (what, k)


@pytest.mark.parametrize("n", SIZES)
def test_ranking_curve_and_metrics(n, gpu_device):
    rng = np.random.default_rng(100 + n)
    s = _scores(n, rng)
    layouts = _label_layouts(n, rng, s)
    t = torch.from_numpy(s).to(gpu_device)
    for kind, lab in layouts.items():
        tl = torch.from_numpy(lab).to(gpu_device)
        for adjust in ADJUSTS:
            what = (n, kind, adjust)
            _assert_curve(ev.ranking_curve(t, tl, adjust), curve_refs.ranking_curve(s, lab, adjust), what)
            _assert_metrics(ev.ranking_metrics(t, tl, adjust), curve_refs.ranking_metrics(s, lab, adjust), what)
    # labels as numbers are read as label > 0.1
    as_float = torch.from_numpy(np.where(layouts["mixed"], 0.7, 0.05).astype(np.float32)).to(gpu_device)
    _assert_curve(ev.ranking_curve(t, as_float), curve_refs.ranking_curve(s, layouts["mixed"]), (n, "float labels"))


def test_pak_with_more_segments_than_one_scan_block(gpu_device):
    """B + 3 labelled segments (length 3, gaps of 1; the first at index 0, the last at n - 1), B = the entries one scan block takes:
    the span starts of PA%K come from the scan's multi-block route.  One segment has two NaN of three, one is all NaN."""
    B = 256 * LEVEL2
    n = 4 * (B + 2) + 1
    lab = np.arange(n) % 4 != 3
    s = (np.random.default_rng(7).integers(0, 41, n) / np.float32(40) - np.float32(0.25)).astype(np.float32)
    s[0] = -0.25
    s[[9, 10, 12, 13, 14, 30]] = np.nan
    t, tl = torch.from_numpy(s).to(gpu_device), torch.from_numpy(lab).to(gpu_device)
    for adjust in (None, "point", ("k", 0), ("k", 50), ("k", 100)):
        _assert_curve(ev.ranking_curve(t, tl, adjust), curve_refs.ranking_curve(s, lab, adjust), ("segments", adjust))
        _assert_metrics(ev.ranking_metrics(t, tl, adjust), curve_refs.ranking_metrics(s, lab, adjust), ("segments", adjust))


def test_all_scores_nan(gpu_device):
    s = np.full(300, np.nan, np.float32)
    lab = np.arange(300) % 3 == 0
    for adjust in ADJUSTS:
        got = ev.ranking_metrics(torch.from_numpy(s).to(gpu_device), torch.from_numpy(lab).to(gpu_device), adjust)
        _assert_metrics(got, curve_refs.ranking_metrics(s, lab, adjust), adjust)
        assert got["best"] is None and got["n_thresholds"] == 0 and got["auroc"] == 0.5


@pytest.mark.parametrize("n", [257, 4097])
def test_point_curve_against_point_adjust_counts(n, gpu_device):
    rng = np.random.default_rng(n)
    s = (rng.integers(0, 60, n) / np.float32(60)).astype(np.float32)
    s[5], s[6] = -0.0, 0.0
    lab = np.convolve(rng.random(n + 8), np.ones(9) / 9.0, mode="valid")[:n] > 0.56
    lab[:4] = True
    t, tl = torch.from_numpy(s).to(gpu_device), torch.from_numpy(lab).to(gpu_device)
    c = ev.ranking_curve(t, tl, "point")
    thr = c["thresholds"].cpu().numpy()
    below = np.nextafter(thr, np.float32(-np.inf)).astype(np.float64)
    table = ev.point_adjust_counts(t, tl, below, compare_f32=True)
    assert np.array_equal(table[:, 0], c["tp"].cpu().numpy()) and np.array_equal(table[:, 2], c["fp"].cpu().numpy())
    m = ev.ranking_metrics(t, tl, "point")
    g = m["best_index"]
    assert m["best"]["latency"] == table[g, 4] / (table[g, 5] + 1e-4)


def _msl():
    z = np.load(os.path.join(HERE, "golden", "msl_eval.npz"))
    return z["test_scores"], z["test_labels"], json.loads(bytes(z["summary"]).decode())


def test_shipped_msl_run(gpu_device):
    s, lab, summary = _msl()
    assert s.size == 73629
    t, tl = torch.from_numpy(s).to(gpu_device), torch.from_numpy(lab).to(gpu_device)
    for adjust in (None, "point"):
        got = ev.ranking_metrics(t, tl, adjust)
        _assert_metrics(got, curve_refs.ranking_metrics(s, lab, adjust), ("msl", adjust))
    assert got["best"]["f1"] >= summary["bf_result"]["f1"]              # the sweep's grid is a subset of the thresholds visited
    assert 0.0 <= got["best"]["latency"]


def _all_outputs(t, tl, adjust):
    c = ev.ranking_curve(t, tl, adjust)
    m = ev.ranking_metrics(t, tl, adjust)
    return [ev.score_order(t), ev.score_order(t, descending=False), c["thresholds"].view(torch.int32), c["tp"], c["fp"]], \
        (c["n_pos"], c["n_neg"], c["nan_pos"], c["nan_neg"], repr(m))


def test_reproducible(gpu_device):
    n = TILE * LEVEL2 + 1
    rng = np.random.default_rng(3)
    s = _scores(n, rng)
    lab = _label_layouts(n, rng, s)["mixed"]
    t, tl = torch.from_numpy(s).to(gpu_device), torch.from_numpy(lab).to(gpu_device)
    for adjust in (None, "point", ("k", 30)):
        first = _all_outputs(t, tl, adjust)
        second = _all_outputs(t, tl, adjust)
        side = torch.cuda.Stream(gpu_device)
        side.wait_stream(torch.cuda.current_stream(gpu_device))
        with torch.cuda.stream(side):
            third = _all_outputs(t, tl, adjust)
        side.synchronize()
        for other in (second, third):
            assert other[1] == first[1]
            assert all(torch.equal(a, b) for a, b in zip(first[0], other[0]))


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
    test[12 + 60:12 + 85] += 1.5
    test[12 + 300:12 + 340, :3] -= 1.0
    return model, train.to(gpu_device), test.to(gpu_device), labels.to(gpu_device)


def test_predict_anomalies_curves(setup):
    model, train, test, labels = setup
    with torch.no_grad():
        plain = ev.predict_anomalies(model, train, test, labels=labels, gamma=0.8)
        for curves in (dict(), dict(adjust="point"), dict(adjust=("k", 20))):
            out = ev.predict_anomalies(model, train, test, labels=labels, gamma=0.8, curves=curves)
            assert set(out) == set(plain) | {"curve_result"}
            assert torch.equal(out["test_scores"], plain["test_scores"])
            assert out["curve_result"] == ev.ranking_metrics(out["test_scores"], labels, **curves)
            assert out["curve_result"]["adjust"] == curves.get("adjust") and out["curve_result"]["n_pos"] == 65
        assert "curve_result" not in plain
        assert ev.predict_anomalies(model, train, test, gamma=0.8, curves=dict())["curve_result"] is None
        with pytest.raises(ValueError, match="curves takes"):
            ev.predict_anomalies(model, train, test, labels=labels, curves=dict(adjusted="point"))


def test_argument_checks(gpu_device):
    t = torch.rand(50, device=gpu_device)
    lab = t > 0.5
    empty = torch.empty(0, device=gpu_device)
    with pytest.raises(ValueError):
        ev.score_order(empty)
    with pytest.raises(ValueError):
        ev.ranking_curve(empty, empty > 0)
    with pytest.raises(ValueError):
        ev.ranking_curve(t, lab[:49])
    with pytest.raises(ValueError):
        ev.ranking_metrics(t, lab[:49], "point")
    for bad in ("points", ("k", 101), ("k", -1), ("k", 2.5), ("j", 3), 7):
        with pytest.raises(ValueError):
            ev.ranking_curve(t, lab, bad)
        with pytest.raises(ValueError):
            ev.ranking_metrics(t, lab, bad)
    with pytest.raises(RuntimeError, match="on the GPU"):
        ev.ranking_curve(t.cpu(), lab)
    with pytest.raises(RuntimeError, match="on the GPU"):
        ev.ranking_curve(t, lab.cpu())
    with pytest.raises(RuntimeError, match="on the GPU"):
        ev.score_order(t.cpu())
    # a 2-D score tensor is read flat, like every 1-D entry point here
    assert torch.equal(ev.score_order(t.reshape(5, 10)), ev.score_order(t))
