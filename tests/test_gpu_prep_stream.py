"""Live rows through the preparation step: preparation.StreamPreparer (k_prep_stream_push of csrc/mtadgat_prep.hip) against
SeriesScaler.transform over each stream's rows as one part, StreamScorer(prepare=) against a plain StreamScorer fed the rows the
series path prepared, and predict_anomalies(prepare=) against predict_anomalies on hand-prepared series.  Everything is compared
bit for bit: the stream state carries the same float32 values the scan carries."""
import numpy as np
import pytest
import torch

import prep_refs

pytestmark = pytest.mark.gpu

S, N, D, W = 5, 150, 38, 12
PATTERNS = {"1": [1], "7": [7], "64": [64], "irregular": [3, 1, 20, 64, 2, 9]}


def _raw(n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, D)) * rng.uniform(0.1, 5.0, D) + rng.uniform(-10.0, 10.0, D)).astype(np.float32)
    x[rng.random((n, D)) < 0.04] = np.nan
    x[rng.random((n, D)) < 0.005] = np.inf
    return x


@pytest.fixture(scope="module")
def setup(gpu_device):
    """(scaler, raw rows (S, N, D) on the host, the same on the device)"""
    import preparation
    scaler = preparation.fit_scaler(torch.from_numpy(_raw(300, 1)).to(gpu_device))
    rows = np.stack([_raw(N, 10 + s) for s in range(S)])
    rows[0, :9, :] = np.nan                     # a leading run: nothing heard yet
    rows[1, 20:101, 3] = np.nan                 # a run longer than any push
    rows[2, 30:33, :] = -np.inf                 # whole rows missing
    rows[3, 70, :] = np.nan
    rows[4, N - 1, :] = np.nan                  # the last row
    return scaler, rows, torch.from_numpy(rows).to(gpu_device)


def _series(scaler, dev, fill, clip=False):
    """per stream, the series path over its rows as one part: (prepared (S, N, D), age (S, N, D)) on the host"""
    out = [scaler.transform(dev[s], fill=fill, clip=clip, lengths=[N], return_age=True) for s in range(S)]
    return np.stack([y.cpu().numpy() for y, _ in out]), np.stack([a.cpu().numpy() for _, a in out])


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert got.tobytes() == want.tobytes() or (np.array_equal(np.isnan(got), np.isnan(want)) and
                                              np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])), what


def _cuts(pattern):
    at, i = 0, 0
    while at < N:
        T = min(PATTERNS[pattern][i % len(PATTERNS[pattern])], N - at)
        yield at, T
        at, i = at + T, i + 1


@pytest.mark.parametrize("fill,clip", [("hold", False), ("hold", True), ("zero", False), (None, False)])
def test_every_cut_gives_the_series_path(setup, fill, clip, gpu_device):
    import preparation
    scaler, rows, dev = setup
    want, want_age = _series(scaler, dev, fill, clip)
    rec = scaler.read()
    for s in range(S):                          # and both are the specification's row-at-a-time replay
        y, a = prep_refs.stream_replay(rows[s], rec, fill, clip)
        _same(want[s], y, (fill, s, "replay"))
        assert np.array_equal(want_age[s], a), (fill, s)
    if fill == "hold":
        assert not np.isnan(want).any()
    for pattern in PATTERNS:
        prep = preparation.StreamPreparer(scaler, S, fill=fill, clip=clip)
        got, age = [], []
        for at, T in _cuts(pattern):
            chunk = dev[:, at] if T == 1 and pattern == "1" else dev[:, at:at + T]          # (n, D) and (n, T, D) pushes
            y, a = prep.push(chunk, return_age=True)
            assert y.shape == chunk.shape and a.shape == chunk.shape and a.dtype == torch.int32
            got.append(y.reshape(S, T, D).cpu().numpy())
            age.append(a.reshape(S, T, D).cpu().numpy())
        _same(np.concatenate(got, axis=1), want, (fill, pattern))
        assert np.array_equal(np.concatenate(age, axis=1), want_age), (fill, pattern, "age")


def test_subsets_permutations_and_reset(setup, gpu_device):
    import preparation
    scaler, rows, dev = setup
    want, want_age = _series(scaler, dev, "hold")
    # subsets at their own cadence: streams (4, 0) seven rows at a time, 2 in blocks of 64, 1 in fives; 3 stays idle
    prep = preparation.StreamPreparer(scaler, S, fill="hold")
    groups = {(4, 0): 7, (2,): 64, (1,): 5}
    at = {g: 0 for g in groups}
    got = {s: [] for s in range(S)}
    ages = {s: [] for s in range(S)}
    while any(at[g] < N for g in groups):
        for g, T in groups.items():
            if at[g] >= N:
                continue
            T = min(T, N - at[g])
            idx = torch.tensor(g, dtype=torch.int64, device=gpu_device)
            y, a = prep.push(dev[list(g), at[g]:at[g] + T], streams=idx, return_age=True)
            for j, s in enumerate(g):
                got[s].append(y[j].cpu().numpy())
                ages[s].append(a[j].cpu().numpy())
            at[g] += T
    for s in (0, 1, 2, 4):
        _same(np.concatenate(got[s]), want[s], ("subset", s))
        assert np.array_equal(np.concatenate(ages[s]), want_age[s]), ("subset", s)
    # stream 3 has heard nothing: its first push is a fresh stream's
    y = prep.push(dev[3:4, :20], streams=torch.tensor([3], device=gpu_device))
    _same(y[0].cpu().numpy(), want[3, :20], "idle stream")
    # permuted stream indices
    prep = preparation.StreamPreparer(scaler, S, fill="hold")
    perm = [3, 0, 4, 1, 2]
    idx = torch.tensor(perm, dtype=torch.int64, device=gpu_device)
    out = [prep.push(dev[perm, at_:at_ + T], streams=idx).cpu().numpy() for at_, T in _cuts("7")]
    _same(np.concatenate(out, axis=1), want[perm], "permuted")
    # reset restores "nothing heard yet" for the streams named, and for those only
    prep = preparation.StreamPreparer(scaler, S, fill="hold")
    prep.push(dev[:, :40])
    prep.reset(torch.tensor([2, 0], dtype=torch.int64, device=gpu_device))
    y, a = prep.push(dev[:, 40:], return_age=True)
    for s in range(S):
        if s in (0, 2):
            fresh, fresh_age = scaler.transform(dev[s, 40:], fill="hold", return_age=True)
            _same(y[s].cpu().numpy(), fresh.cpu().numpy(), ("reset", s))
            assert torch.equal(a[s], fresh_age), ("reset", s)
        else:
            _same(y[s].cpu().numpy(), want[s, 40:], ("not reset", s))
    prep.reset()
    _same(prep.push(dev[:, :40]).cpu().numpy(), want[:, :40], "reset of all streams")
    # a stream index outside the preparer touches no state and gets NaN
    before = prep._state.clone()
    y, a = prep.push(dev[:2, 40:43], streams=torch.tensor([9, -1], dtype=torch.int64, device=gpu_device), return_age=True)
    assert bool(torch.isnan(y).all()) and bool((a == -1).all()) and torch.equal(prep._state.view(torch.int64), before.view(torch.int64))
    with pytest.raises(ValueError):
        prep.push(dev[:3, :4])                  # three rows for five streams, no selection
    with pytest.raises(ValueError):
        prep.push(dev[:, :4, :7])


# ---- StreamScorer(prepare=) and predict_anomalies(prepare=) ----------------------------------------------------------------------
_MODEL = {}
FIELDS = ("scores", "flags", "per_dim", "closed_start", "closed_end", "closed_peak", "closed_peak_score", "closed_mean")


def _model(device):
    from mtad_gat import MTAD_GAT
    if "m" not in _MODEL:
        torch.manual_seed(11)
        _MODEL["m"] = MTAD_GAT(n_features=D, window_size=W, out_dim=D, kernel_size=3, gru_hid_dim=8, forecast_hid_dim=8,
                               recon_hid_dim=8).to(device).eval()
    return _MODEL["m"]


def _push_all(scorer, dev, pattern="7"):
    outs = [scorer.push(dev[:, at:at + T]) for at, T in _cuts(pattern)]
    return {k: np.concatenate([o[k].cpu().numpy() for o in outs], axis=1) for k in FIELDS}


@pytest.mark.parametrize("span", [None, 5])
def test_stream_scorer_prepares_its_rows(setup, span, gpu_device):
    import preparation
    from streaming import StreamScorer
    scaler, rows, dev = setup
    model = _model(gpu_device)
    kw = dict(threshold=0.6, smoothing_span=span, merge_gap=1, min_length=2)
    want_rows, _ = _series(scaler, dev, "hold")
    plain = _push_all(StreamScorer(model, S, **kw), torch.from_numpy(want_rows).to(gpu_device))
    scorer = StreamScorer(model, S, prepare=(scaler, "hold"), **kw)
    got = _push_all(scorer, dev)
    for k in FIELDS:
        assert got[k].tobytes() == plain[k].tobytes(), (span, k)
    assert np.isnan(got["scores"][:, :W]).all() and np.isfinite(got["scores"][:, W:]).all()       # finite after every gap, smoothed or not
    assert np.isfinite(got["per_dim"][:, W:]).all()
    # the raw rows themselves: a missing row has no score, and poisons a moving average for good
    raw = _push_all(StreamScorer(model, S, **kw), dev)
    assert np.isnan(raw["scores"][3, 70])
    if span is not None:
        assert np.isnan(raw["scores"][3, 70:]).all()
    # a StreamPreparer given as it is, other cuts, and reset() resetting it too
    prep = preparation.StreamPreparer(scaler, S, fill="hold")
    scorer = StreamScorer(model, S, prepare=prep, **kw)
    first = _push_all(scorer, dev, "irregular")
    scorer.reset()
    second = _push_all(scorer, dev, "64")
    for k in FIELDS:
        assert first[k].tobytes() == plain[k].tobytes() and second[k].tobytes() == plain[k].tobytes(), (span, k, "reset")
    with pytest.raises(ValueError):
        StreamScorer(model, S + 1, prepare=prep, **kw)


def test_update_prepares_its_rows(setup, gpu_device):
    from streaming import StreamScorer
    scaler, rows, dev = setup
    model = _model(gpu_device)
    g = torch.Generator().manual_seed(3)
    preds, last = torch.rand(S, 20, D, generator=g).to(gpu_device), torch.rand(S, 20, D, generator=g).to(gpu_device)
    want_rows, _ = _series(scaler, dev, "zero")
    plain = StreamScorer(model, S, 0.5).update(preds, last, torch.from_numpy(want_rows[:, :20]).to(gpu_device))
    got = StreamScorer(model, S, 0.5, prepare=(scaler, "zero")).update(preds, last, dev[:, :20])
    for k in FIELDS:
        assert got[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("prepare", [dict(fill="hold", gaps="ignore"), dict(), dict(fill="zero", clip=True)])
def test_predict_anomalies_prepares_raw_series(prepare, gpu_device):
    import evaluation as ev
    import preparation
    model = _model(gpu_device)
    train, test = torch.from_numpy(_raw(300, 21)).to(gpu_device), torch.from_numpy(_raw(260, 22)).to(gpu_device)
    test[100:104] = float("nan")                # the second test part starts in a gap
    parts = dict(train_lengths=[140, 160], test_lengths=[100, 160], transition=(3, W - 1))
    labels = torch.zeros(260 - W, dtype=torch.bool, device=gpu_device)
    labels[150:170] = True
    opts = dict(fill="zero", clip=False, gaps="zero")
    opts.update(prepare)
    with torch.no_grad():
        got = ev.predict_anomalies(model, train, test, labels=labels, parts=parts, prepare=prepare)
        scaler = preparation.fit_scaler(train, gaps=opts["gaps"])
        tr = scaler.transform(train, fill=opts["fill"], clip=opts["clip"], lengths=parts["train_lengths"])
        te = scaler.transform(test, fill=opts["fill"], clip=opts["clip"], lengths=parts["test_lengths"])
        want = ev.predict_anomalies(model, tr, te, labels=labels, parts=parts)
        assert "scaler" not in want and torch.equal(got["scaler"].record.view(torch.int32), scaler.record.view(torch.int32))
        for k in ("train_scores", "test_scores", "test_per_dim"):
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
            assert bool(torch.isfinite(got[k]).all()), k
        assert repr(got["epsilon_result"]) == repr(want["epsilon_result"])
        # without parts: one part per series
        got = ev.predict_anomalies(model, train, test, prepare=prepare)
        want = ev.predict_anomalies(model, scaler.transform(train, fill=opts["fill"], clip=opts["clip"]),
                                    scaler.transform(test, fill=opts["fill"], clip=opts["clip"]))
        assert torch.equal(got["test_scores"].view(torch.int32), want["test_scores"].view(torch.int32))
    with pytest.raises(ValueError):
        ev.predict_anomalies(model, train, test, prepare=dict(fill="hold", span=3))
