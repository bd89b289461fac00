"""StreamScorer with adaptive peaks-over-threshold thresholds (k_stream_score<true>, csrc/mtadgat_stream.hip) against
evaluation.spot_run over the same per-stream scores: the step is the same device function, so everything is compared bit for bit
(torch.equal / numpy array_equal) -- thresholds, flags and the events, however the rows are cut into pushes.  spot_run itself is
gated against the numpy specification in tests/test_gpu_spot.py.

The model is tiny (F = 3, W = 5) and update() is driven with made-up model outputs: every column of a stream's row carries the same
forecast error v, so the stream's score is |v| exactly and the scores can be prescribed (the trick of tests/test_gpu_stream.py).
"""
import numpy as np
import pytest
import torch

import event_refs
import spot_cases

pytestmark = pytest.mark.gpu

W, F = 5, 3
S = 6
ROWS = W + 500                   # the level shift of the matrix starts at row 400
MAX_BLOCK = 16
GAP, MIN_LENGTH = 1, 2
FIELDS = ("scores", "flags", "thresholds", "closed_start", "closed_end", "closed_peak", "closed_peak_score", "closed_mean")
CLOSED = FIELDS[3:]

_MODEL = {}


def _model(device):
    from mtad_gat import MTAD_GAT
    if "m" not in _MODEL:
        torch.manual_seed(5)
        _MODEL["m"] = MTAD_GAT(n_features=F, window_size=W, out_dim=F, kernel_size=3, gru_hid_dim=8, forecast_hid_dim=8,
                               recon_hid_dim=8).to(device).eval()
    return _MODEL["m"]


def _inputs(device):
    """The prescribed scores v (S, ROWS) float32 -- six columns of the seventy-column matrix, NaN rows, level shift and bursts
    included -- and the update() arguments that produce them: rows 0, recons_last 0, preds[k - 1] = v[k]."""
    _, x = spot_cases.data("seventy columns")
    v = np.ascontiguousarray(x[:ROWS, :S].T)
    preds = np.zeros((S, ROWS, F), np.float32)
    preds[:, :-1] = v[:, 1:, None]
    dev = tuple(torch.from_numpy(a).to(device) for a in (np.zeros((S, ROWS, F), np.float32), preds, np.zeros((S, ROWS, F), np.float32)))
    return v, dev


def _state(device, dynamic=True, columns=S):
    import evaluation
    init, _ = spot_cases.data("seventy columns")
    return evaluation.spot_calibrate(torch.from_numpy(init[:, :columns]).to(device), q=spot_cases.Q, level=0.98, max_peaks=8, dynamic=dynamic)


def _scorer(device, threshold, n_streams=S, **kw):
    from streaming import StreamScorer
    return StreamScorer(_model(device), n_streams, threshold, gamma=0.5, max_block=MAX_BLOCK, merge_gap=GAP, min_length=MIN_LENGTH, **kw)


def _run(scorer, dev, pattern, lo=0, streams=None, fields=FIELDS):
    x, p, r = dev
    sel = slice(None) if streams is None else streams
    parts, at = [], lo
    for T in pattern:
        parts.append(scorer.update(p[sel, at:at + T], r[sel, at:at + T], x[sel, at:at + T], streams=streams))
        at += T
    return {key: torch.cat([part[key] for part in parts], dim=1) for key in fields}


def _pattern(T, rows=ROWS):
    return [T] * (rows // T) + ([rows % T] if rows % T else [])


def _same(a, b, what):
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (what, key)
        assert np.array_equal(a[key].cpu().numpy(), b[key].cpu().numpy(), equal_nan=True), (what, key)


def _assert_events(out, flushed, what):
    """The closed events in push order, then flush(), against numpy over each stream's own flags."""
    flags = out["flags"][:, W:].cpu().numpy().astype(bool)
    start = out["closed_start"].cpu().numpy()
    end = out["closed_end"].cpu().numpy()
    for s in range(flags.shape[0]):
        at = np.flatnonzero(start[s] >= 0)
        got_start, got_end = start[s, at], end[s, at]
        assert np.array_equal(at - W, got_end + GAP), (what, s)
        if flushed["closed_start"][s] >= 0:
            got_start, got_end = np.append(got_start, int(flushed["closed_start"][s])), np.append(got_end, int(flushed["closed_end"][s]))
        ref_start, ref_end = event_refs.runs(flags[s], GAP, MIN_LENGTH)
        assert np.array_equal(got_start, ref_start) and np.array_equal(got_end, ref_end), (what, s)


@pytest.mark.parametrize("dynamic", [True, False], ids=["dynamic", "static"])
def test_streams_match_spot_run_however_the_rows_are_cut(dynamic, gpu_device):
    import evaluation
    v, dev = _inputs(gpu_device)
    state = _state(gpu_device, dynamic)
    one = _scorer(gpu_device, state)
    out = _run(one, dev, _pattern(1))
    assert torch.equal(state.buf, _state(gpu_device, dynamic).buf), "the scorer works on a clone"
    scores = out["scores"][:, W:]
    assert np.array_equal(scores.cpu().numpy(), np.abs(v[:, W:]), equal_nan=True), "the prescribed scores"
    assert torch.isnan(out["thresholds"][:, :W]).all() and not out["flags"][:, :W].any()

    thr, flags = evaluation.spot_run(state.clone(), scores.T)
    assert torch.equal(out["thresholds"][:, W:], thr.T.contiguous()), "thresholds"
    assert torch.equal(out["flags"][:, W:], flags.T.contiguous()), "flags"
    assert flags.any() and not flags.all() and (thr[1:] != thr[:-1]).any() == dynamic
    assert torch.equal(one.spot_state().buf, _advanced(evaluation, state, scores).buf), "the live state"
    _assert_events(out, {k: t.cpu().numpy() for k, t in one.flush().items()}, ("one", dynamic))

    for T in (7, MAX_BLOCK):
        other = _scorer(gpu_device, state)
        _same(_run(other, dev, _pattern(T)), out, (T, dynamic))
        assert torch.equal(other.spot_state().buf, one.spot_state().buf), (T, "state")


def _advanced(evaluation, state, scores):
    st = state.clone()
    evaluation.spot_run(st, scores.T)
    return st


def test_mixed_subsets_reset_and_one_column_for_all(gpu_device):
    """Streams pushed through `streams=` at their own cadence, one reset mid-way, all started from ONE calibrated column: each
    stream reproduces the run of that column over its own scores."""
    import evaluation
    v, dev = _inputs(gpu_device)
    single = _state(gpu_device, True, columns=1)
    scorer = _scorer(gpu_device, single)
    assert scorer.spot_state().n_columns == S
    cadence = {0: 1, 1: 7, 2: 16, 3: 3, 5: 5}                  # rows per push; stream 4 stays idle
    RESET, RESET_AT = 3, 150
    at = {s: 0 for s in cadence}
    parts = {s: [] for s in cadence}
    step = 0
    while any(at[s] < ROWS for s in cadence):
        step += 1
        by_T = {}
        for s, T in cadence.items():
            if at[s] < ROWS and step % (1 + s % 3) == 0:
                if s == RESET and at[s] == RESET_AT:
                    scorer.reset(torch.tensor([s], device=gpu_device))
                by_T.setdefault(min(T, ROWS - at[s], RESET_AT - at[s] if s == RESET and at[s] < RESET_AT else ROWS), []).append(s)
        for T, group in by_T.items():
            group = group[::-1]
            idx = torch.tensor(group, device=gpu_device)
            x, p, r = (torch.stack([a[s, at[s]:at[s] + T] for s in group]) for a in dev)
            out = scorer.update(p, r, x, streams=idx)
            for j, s in enumerate(group):
                parts[s].append({key: out[key][j:j + 1] for key in FIELDS})
                at[s] += T
    live = scorer.spot_state().read()
    first = single.read()
    assert live["n"][4] == first["n"][0] and live["z"][4] == first["z"][0], "the idle stream keeps the calibrated column"
    for s in cadence:
        got = {key: torch.cat([part[key] for part in parts[s]], dim=1) for key in FIELDS}
        spans = [(0, ROWS)] if s != RESET else [(0, RESET_AT), (RESET_AT, ROWS)]
        for lo, hi in spans:                                    # after the reset the stream warms up and starts from the calibration
            sc = got["scores"][:, lo + W:hi]
            assert torch.isnan(got["scores"][:, lo:lo + W]).all() and torch.isnan(got["thresholds"][:, lo:lo + W]).all(), (s, lo)
            thr, flags = evaluation.spot_run(single.clone(), sc.T)
            assert torch.equal(got["thresholds"][:, lo + W:hi], thr.T.contiguous()), (s, lo, "thresholds")
            assert torch.equal(got["flags"][:, lo + W:hi], flags.T.contiguous()), (s, lo, "flags")
        solo = _scorer(gpu_device, single, n_streams=1)
        one = tuple(a[s:s + 1] for a in dev)
        if s != RESET:
            ref = _run(solo, one, _pattern(1))
        else:
            head = _run(solo, one, [1] * RESET_AT)
            solo.flush(reset=True)
            tail = _run(solo, one, [1] * (ROWS - RESET_AT), lo=RESET_AT)
            ref = {key: torch.cat((head[key], tail[key]), dim=1) for key in FIELDS}
        _same(got, ref, ("stream", s))


def test_smoothing_applies_before_the_threshold(gpu_device):
    import evaluation
    _, dev = _inputs(gpu_device)
    dev = tuple(torch.nan_to_num(a, nan=0.25) for a in dev)     # a NaN would stay in the moving average for good
    state = _state(gpu_device, True)
    scorer = _scorer(gpu_device, state, smoothing_span=3)
    out = _run(scorer, dev, _pattern(7))
    plain = _run(_scorer(gpu_device, state), dev, _pattern(7))
    smoothed = out["scores"][:, W:]
    assert not torch.equal(smoothed, plain["scores"][:, W:])
    want = torch.stack([evaluation.moving_average(plain["scores"][s, W:], 3) for s in range(S)])
    assert torch.allclose(smoothed, want, rtol=2.0 ** -22, atol=0.0), "the moving average of the scores"
    thr, flags = evaluation.spot_run(state.clone(), smoothed.T)
    assert torch.equal(out["thresholds"][:, W:], thr.T.contiguous()) and torch.equal(out["flags"][:, W:], flags.T.contiguous())
    assert flags.any()
    _assert_events(out, {k: t.cpu().numpy() for k, t in scorer.flush().items()}, "smoothed")
    _same(_run(_scorer(gpu_device, state, smoothing_span=3), dev, _pattern(1)), out, "smoothed, one row at a time")


def test_a_fixed_threshold_scorer_beside_it_is_unchanged(gpu_device):
    """The fixed-threshold instance of the kernel next to the adaptive one: the same scores, flags = float64(score) > threshold and
    the events of those flags, no "thresholds" output -- with a float and with per-stream thresholds."""
    v, dev = _inputs(gpu_device)
    state = _state(gpu_device, True)
    adaptive = _run(_scorer(gpu_device, state), dev, _pattern(7))
    per_stream = torch.from_numpy(state.read()["z"])
    for threshold in (0.6, per_stream):
        scorer = _scorer(gpu_device, threshold)
        assert scorer.spot_state() is None
        x, p, r = dev
        assert "thresholds" not in scorer.update(p[:, :1], r[:, :1], x[:, :1])
        scorer.reset()
        out = _run(scorer, dev, _pattern(7), fields=tuple(k for k in FIELDS if k != "thresholds"))
        _same({"scores": out["scores"]}, {"scores": adaptive["scores"]}, "scores")            # (NaN for warm-up and NaN rows)
        thr = torch.as_tensor(threshold, dtype=torch.float64).reshape(-1, 1).to(gpu_device)
        assert torch.equal(out["flags"][:, W:].bool(), out["scores"][:, W:].double() > thr)
        _assert_events(out, {k: t.cpu().numpy() for k, t in scorer.flush().items()}, "fixed")
    # a static SPOT state and the fixed per-stream thresholds it holds flag the same rows
    static = _run(_scorer(gpu_device, _state(gpu_device, False)), dev, _pattern(7))
    fixed = _run(_scorer(gpu_device, per_stream), dev, _pattern(7), fields=("flags", "closed_start", "closed_end"))
    for key in fixed:
        assert torch.equal(static[key], fixed[key]), key


def test_argument_checks(gpu_device):
    state = _state(gpu_device, True, columns=2)
    with pytest.raises(ValueError, match="one column or one per stream"):
        _scorer(gpu_device, state)
    scorer = _scorer(gpu_device, _state(gpu_device, True))
    x = torch.zeros(2, 1, F, device=gpu_device)
    out = scorer.update(x, x, x, streams=torch.tensor([1, 9], device=gpu_device))          # a stream index outside touches nothing
    assert torch.isnan(out["thresholds"]).all() and int(out["flags"].sum()) == 0
