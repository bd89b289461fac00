"""Row-by-row scoring of live streams on the device (csrc/mtadgat_stream.hip through streaming.StreamScorer) against references
computed over each stream's whole array: float64 straight from the definition for the scores, tests/score_refs.py for the moving
average, tests/event_refs.py for flags, events and their statistics; and against the batch route MTAD_GAT.anomaly_scores.

Gates
  per-dimension scores, unsmoothed score: |ours - ref64| <= 1 float32 ulp of the reference (ours is rounded once from float64: half
      an ulp; the float64 sums differ in their order only, which matters next to a rounding tie -- hence one ulp, not a half).
  smoothed score: |ours - ref64| <= 2^-23 |ref64| + 1e-30, the gate of test_gpu_score_pipeline.py::_assert_ewm.
  flags, event bounds, peaks, peak scores, the sample an event is reported at: exact.  closed_mean: 1 float32 ulp.
  push patterns, subsets, permutations: bit-identical.
  against the batch route: max |stream - batch| <= FP32_TOL max(1, |batch|) (the two sides take different batch-size routes
      through the recurrence kernels, so this is a tolerance, and events are gated against the STREAMED scores).
"""
import numpy as np
import pytest
import torch

import event_refs
import score_refs
from helpers import FP32_TOL

pytestmark = pytest.mark.gpu

W, F = 12, 7
ROWS = W + 300                   # 300 scored rows per stream
THR = 0.5
GAMMA = 0.25
MAX_BLOCK = 64
S_SIZES = [1, 3, 65, 257]        # streams on either side of the wave (1 per wave) and workgroup (4 waves) boundaries
D_SIZES = [1, 7, 64, 65, 130]    # columns on either side of a 64-lane row
KINDS = ("noise", "below", "above", "alternating", "special")
GAPS = (0, 1, 2, 7, 300)
MIN_LENGTHS = (1, 2, 5, 301)
FIELDS = ("scores", "flags", "per_dim", "closed_start", "closed_end", "closed_peak", "closed_peak_score", "closed_mean")
CLOSED = FIELDS[3:]


def _pattern(kind):
    """The rows per push of one pass over ROWS rows."""
    if kind == "irregular":
        cycle, out = (1, 3, 7, 2, 64, 5, 1, 1, 30, 4, 13, 2), []
        while sum(out) < ROWS:
            out.append(min(cycle[len(out) % len(cycle)], ROWS - sum(out)))
        return out
    T = int(kind)
    return [T] * (ROWS // T) + ([ROWS % T] if ROWS % T else [])


# ---- models: only their shapes matter to update() ----------------------------------------------------------------------------------
_MODELS = {}


def _model(out_dim, device, seed=9):
    from mtad_gat import MTAD_GAT
    key = (out_dim, seed)
    if key not in _MODELS:
        torch.manual_seed(seed)
        _MODELS[key] = MTAD_GAT(n_features=F, window_size=W, out_dim=out_dim, kernel_size=3, gru_hid_dim=24, forecast_hid_dim=24,
                                recon_hid_dim=24).to(device).eval()
    return _MODELS[key]


def _dims(d):
    return [(3 * c + 1) % F for c in range(d)]            # every column, in another order, repeated when d > F


# ---- inputs and their reference --------------------------------------------------------------------------------------------------
def _inputs(S, d, rot, seed):
    """rows (S, ROWS, F), preds and recons_last (S, ROWS, d) float32; stream s is of kind KINDS[(s + rot) % 5]."""
    rng = np.random.default_rng(seed)
    dims = _dims(d)
    x = rng.random((S, ROWS, F)).astype(np.float32)
    p = np.empty((S, ROWS, d), np.float32)
    r = np.empty((S, ROWS, d), np.float32)
    k = np.arange(ROWS)
    for s in range(S):
        kind = KINDS[(s + rot) % len(KINDS)]
        if kind == "special":                             # every column carries the same value v: the mean is v exactly
            x[s] = 0.0
            v = rng.random(ROWS).astype(np.float32)
            specials = (np.nan, np.inf, -np.inf, THR, np.nan, np.inf, np.float32(np.nextafter(np.float32(THR), np.float32(1))))
            for j, val in enumerate(specials):
                v[W - 1 + (j * 37 + 5) % 300] = val
            p[s], r[s] = v[:, None], 0.0
            continue
        xd = x[s][:, dims]
        nxt = np.concatenate((xd[1:], np.zeros((1, d), np.float32)))        # what a perfect forecast of the next row would be
        if kind == "noise":
            z = np.convolve(rng.random(ROWS + 4), np.ones(5) / 5.0, mode="valid")[:ROWS] * 0.9
            p[s], r[s] = nxt + z[:, None].astype(np.float32), rng.random((ROWS, d))
        else:
            lift = {"below": 0.0 * k, "above": 2.0 + 0.0 * k, "alternating": 2.0 * (k % 2)}[kind]
            p[s], r[s] = nxt + lift[:, None].astype(np.float32), xd
    return x, p, r


def _reference(x, p, r, d, gamma, scale=None):
    """(per_dim (S, 300, d), score (S, 300)) in float64: row W + i is scored with the forecast made at row W + i - 1."""
    actual = x[:, W:, _dims(d)].astype(np.float64)
    with np.errstate(invalid="ignore"):
        a = np.abs(p[:, W - 1:-1].astype(np.float64) - actual) + gamma * np.abs(r[:, W:].astype(np.float64) - actual)
        if scale is not None:
            a = (a - scale[0].astype(np.float64)) / (1.0 + scale[1].astype(np.float64))
        return a, a.sum(axis=2) / d


def _assert_ulp(got, ref, what):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    same_inf = np.isinf(ref) & (got == ref)
    fin = ~nan & ~same_inf
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= score_refs.ulp32(ref[fin])), (what, float(err.max()))


def _assert_ewm(got, x, span, what):
    """test_gpu_score_pipeline.py::_assert_ewm for one stream."""
    ref = score_refs.ewm(x, span)
    err = np.abs(got.astype(np.float64) - ref)
    bound = 2.0 ** -23 * np.abs(ref) + 1e-30
    assert np.all(err <= bound), (what, float((err / bound).max()))


# ---- running a scorer ------------------------------------------------------------------------------------------------------------
def _scorer(device, S, d, max_block=MAX_BLOCK, threshold=THR, **kw):
    from streaming import StreamScorer
    return StreamScorer(_model(d, device), S, threshold, target_dims=_dims(d), gamma=GAMMA, max_block=max_block, **kw)


def _run(scorer, dev_inputs, pattern, streams=None, lo=0):
    """update() over the pattern from row `lo` on; the outputs concatenated along the rows, as numpy arrays."""
    x, p, r = dev_inputs
    parts, at = [], lo
    for T in pattern:
        parts.append(scorer.update(p[:, at:at + T], r[:, at:at + T], x[:, at:at + T], streams=streams))
        at += T
    return {key: torch.cat([part[key] for part in parts], dim=1).cpu().numpy() for key in FIELDS}


def _same_bits(a, b, what):
    for key in FIELDS:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (what, key)
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


def _assert_events(out, flushed, gap, min_length, what, threshold=THR):
    """The closed events in push order, then flush(), against event_refs over every stream's whole score array."""
    scores, start = out["scores"][:, W:], out["closed_start"]
    flags = event_refs.flags(scores, threshold)
    assert np.array_equal(out["flags"][:, W:].astype(bool), flags), what
    assert np.all(start[:, :W] == -1), what
    for s in range(scores.shape[0]):
        at = np.flatnonzero(start[s] >= 0)
        got = {key: out[key][s, at] for key in CLOSED}
        # an event whose last flagged sample is e - 1 is reported at sample e + merge_gap
        assert np.array_equal(at - W, got["closed_end"] + gap), (what, s)
        if flushed["closed_start"][s] >= 0:
            got = {key: np.append(got[key], flushed[key][s]) for key in CLOSED}
        ref_start, ref_end = event_refs.runs(flags[s], gap, min_length)
        assert np.array_equal(got["closed_start"], ref_start) and np.array_equal(got["closed_end"], ref_end), (what, s)
        ref = event_refs.stats(scores[s], ref_start, ref_end)
        assert np.array_equal(got["closed_peak"], ref["peak"]), (what, s)
        assert np.array_equal(got["closed_peak_score"], ref["peak_score"]), (what, s)
        _assert_ulp(got["closed_mean"], ref["mean_score"], (what, s, "mean"))
    none = start < 0
    for key in ("closed_end", "closed_peak"):
        assert np.all(out[key][none] == -1), (what, key)
    assert np.all(np.isnan(out["closed_peak_score"][none])) and np.all(np.isnan(out["closed_mean"][none])), what


def _flush(scorer):
    return {key: val.cpu().numpy() for key, val in scorer.flush().items()}


# ---- the state machine alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", D_SIZES)
@pytest.mark.parametrize("S", S_SIZES)
def test_state_machine(S, d, gpu_device):
    rot = D_SIZES.index(d)
    x, p, r = _inputs(S, d, rot, 1000 * S + d)
    dev = tuple(torch.from_numpy(v).to(gpu_device) for v in (x, p, r))
    kinds = [KINDS[(s + rot) % len(KINDS)] for s in range(S)]
    ref_dim, ref_score = _reference(x, p, r, d, GAMMA)

    # one row at a time: the scores and everything derived from them
    one = _run(_scorer(gpu_device, S, d, merge_gap=2, min_length=2), dev, _pattern("1"))
    assert np.all(np.isnan(one["scores"][:, :W])) and np.all(np.isnan(one["per_dim"][:, :W])) and not one["flags"][:, :W].any()
    _assert_ulp(one["per_dim"][:, W:], ref_dim, (S, d, "per_dim"))
    _assert_ulp(one["scores"][:, W:], ref_score, (S, d, "score"))
    flags = one["flags"][:, W:].astype(bool)
    for s, kind in enumerate(kinds):
        if kind == "below":
            assert not flags[s].any()
        if kind == "above":
            assert flags[s].all()
        if kind == "special":                             # NaN and the threshold itself are not flagged, the next float32 is
            v = p[s, W - 1:-1, 0]
            assert np.array_equal(one["scores"][s, W:], np.abs(v), equal_nan=True)
            assert np.array_equal(flags[s], np.nan_to_num(np.abs(v), nan=0.0) > THR) and flags[s][np.isinf(v)].all()

    # every way of cutting the rows into pushes gives the same bits; so does a ring that wraps every few rows
    irregular = _pattern("irregular")
    for name, pattern, block in (("7", _pattern("7"), MAX_BLOCK), ("64", _pattern("64"), MAX_BLOCK), ("irregular", irregular, MAX_BLOCK),
                                 ("wrap", _pattern("5"), 5)):
        scorer = _scorer(gpu_device, S, d, max_block=block, merge_gap=2, min_length=2)
        assert scorer.ring_rows == W + block - 1
        out = _run(scorer, dev, pattern)
        _same_bits(out, one, (S, d, name))
        if name == "irregular":
            _assert_events(out, _flush(scorer), 2, 2, (S, d, name))
    if S >= len(KINDS):
        edges = np.cumsum(irregular)[:-1] - W             # score index of the first row of every later push
        edges = edges[edges > 0]
        assert (flags[:, edges - 1] & flags[:, edges]).any(), "a run across a push boundary"
        assert (flags[:, edges - 1] & ~flags[:, edges]).any(), "a run that ends on the last row of a push"
        assert (~flags[:, edges - 1] & flags[:, edges]).any(), "a run that starts on the first row of a push"

    # the event rules
    for gap in GAPS:
        for min_length in MIN_LENGTHS:
            scorer = _scorer(gpu_device, S, d, merge_gap=gap, min_length=min_length)
            out = _run(scorer, dev, _pattern("64"))
            assert out["scores"].tobytes() == one["scores"].tobytes()
            _assert_events(out, _flush(scorer), gap, min_length, (S, d, gap, min_length))

    # fixed scaling, then the moving average of the scaled score
    rng = np.random.default_rng(d)
    scale = (rng.random(d).astype(np.float32) * 0.2, rng.random(d).astype(np.float32))
    ref_dim_s, ref_score_s = _reference(x, p, r, d, GAMMA, scale)
    scale_t = tuple(torch.from_numpy(v) for v in scale)
    plain = _run(_scorer(gpu_device, S, d, scale=scale_t), dev, _pattern("64"))
    _assert_ulp(plain["per_dim"][:, W:], ref_dim_s, (S, d, "scaled per_dim"))
    _assert_ulp(plain["scores"][:, W:], ref_score_s, (S, d, "scaled score"))
    for span in (1, 2, 7, 153):
        scorer = _scorer(gpu_device, S, d, scale=scale_t, smoothing_span=span, merge_gap=1)
        out = _run(scorer, dev, irregular)
        assert out["per_dim"].tobytes() == plain["per_dim"].tobytes(), "the per-dimension scores are never smoothed"
        for s in range(S):
            if np.isfinite(plain["scores"][s, W:]).all():
                _assert_ewm(out["scores"][s, W:], plain["scores"][s, W:], span, (S, d, span, s))
        _assert_events(out, _flush(scorer), 1, 1, (S, d, "span", span))
        if span == 7:
            _same_bits(_run(_scorer(gpu_device, S, d, scale=scale_t, smoothing_span=span, merge_gap=1), dev, _pattern("1")), out, (S, d, "span 7"))


def test_subsets_of_streams(gpu_device):
    """Streams pushed through `streams=` at their own cadence, one left idle, one reset mid-way, each with its own threshold:
    every stream reproduces its own solo run bit for bit."""
    S, d = 6, 7
    x, p, r = _inputs(S, d, 0, 77)
    dev = tuple(torch.from_numpy(v).to(gpu_device) for v in (x, p, r))
    thr = torch.tensor([0.5, 0.45, 0.55, 0.5, 0.6, 0.4], dtype=torch.float64)
    scorer = _scorer(gpu_device, S, d, threshold=thr, merge_gap=1, min_length=2, smoothing_span=3)
    cadence = {0: 1, 1: 5, 2: 64, 4: 7, 5: 3}                  # rows per push; stream 3 stays idle
    RESET, RESET_AT = 5, 140
    at = {s: 0 for s in cadence}
    parts = {s: [] for s in cadence}
    flushed_at_reset = None
    step = 0
    while any(at[s] < ROWS for s in cadence):
        step += 1
        by_T = {}
        for s, T in cadence.items():
            if at[s] < ROWS and step % (1 + s % 3) == 0:       # not every stream at every step
                if s == RESET and at[s] == RESET_AT:
                    flushed_at_reset = {k: v.cpu().numpy() for k, v in scorer.flush(torch.tensor([s], device=gpu_device), reset=True).items()}
                by_T.setdefault(min(T, ROWS - at[s], RESET_AT - at[s] if s == RESET and at[s] < RESET_AT else ROWS), []).append(s)
        for T, group in by_T.items():
            group = group[::-1]                                # any order of distinct streams
            idx = torch.tensor(group, device=gpu_device)
            rows = [torch.stack([v[s, at[s]:at[s] + T] for s in group]) for v in dev]
            out = scorer.update(rows[1], rows[2], rows[0], streams=idx)
            for j, s in enumerate(group):
                parts[s].append({key: out[key][j:j + 1] for key in FIELDS})
                at[s] += T
    final = _flush(scorer)
    assert final["closed_start"][3] == -1, "the idle stream has no event"
    assert flushed_at_reset is not None
    for s in cadence:
        got = {key: torch.cat([part[key] for part in parts[s]], dim=1).cpu().numpy() for key in FIELDS}
        solo = _scorer(gpu_device, 1, d, threshold=float(thr[s]), merge_gap=1, min_length=2, smoothing_span=3)
        one = tuple(v[s:s + 1] for v in dev)
        if s != RESET:
            ref = _run(solo, one, _pattern("1"))
            ref_flush = _flush(solo)
        else:
            first = _run(solo, one, [1] * RESET_AT)
            before = _flush(solo)
            for key in CLOSED:
                assert flushed_at_reset[key].tobytes() == before[key].tobytes(), ("flush before the reset", key)
            solo.reset()
            rest = _run(solo, one, [1] * (ROWS - RESET_AT), lo=RESET_AT)
            assert np.all(np.isnan(rest["scores"][:, :W])) and np.isfinite(rest["scores"][:, W:]).all(), "a reset stream warms up again"
            ref = {key: np.concatenate((first[key], rest[key]), axis=1) for key in FIELDS}
            ref_flush = _flush(solo)
        _same_bits(got, ref, ("stream", s))
        for key in CLOSED:
            assert final[key][s:s + 1].tobytes() == ref_flush[key].tobytes(), ("flush", s, key)


def test_argument_checks_on_the_device(gpu_device):
    scorer = _scorer(gpu_device, 3, 7, max_block=5)
    rows = torch.rand(3, 5, F, device=gpu_device)
    with pytest.raises(ValueError):
        scorer.push(torch.rand(3, 5, F + 1, device=gpu_device))
    with pytest.raises(ValueError):
        scorer.push(torch.rand(3, 6, F, device=gpu_device))
    with pytest.raises(ValueError):
        scorer.push(rows[:2])                                   # two rows for three streams, and no `streams`
    with pytest.raises(ValueError):
        scorer.push(rows, streams=torch.tensor([0, 1], device=gpu_device))
    with pytest.raises(ValueError):
        scorer.push(rows, streams=torch.tensor([0, 1, 2], dtype=torch.int32, device=gpu_device))
    with pytest.raises(RuntimeError):
        scorer.push(rows.cpu())
    with pytest.raises(ValueError):
        scorer.update(torch.rand(3, 5, 6, device=gpu_device), torch.rand(3, 5, 7, device=gpu_device), rows)
    with pytest.raises(ValueError):
        _scorer(gpu_device, 3, 7, smoothing_span=0.5)
    # a stream index outside the scorer touches nothing and reports nothing
    out = scorer.update(torch.rand(2, 1, 7, device=gpu_device), torch.rand(2, 1, 7, device=gpu_device), rows[:2, :1],
                        streams=torch.tensor([1, 9], device=gpu_device))
    assert torch.isnan(out["scores"]).all() and int(out["flags"].sum()) == 0 and bool((out["closed_start"] == -1).all())
    model = _model(7, gpu_device)
    model.train()
    try:
        with pytest.raises(NotImplementedError):
            scorer.push(rows)
    finally:
        model.eval()


# ---- with the model ----------------------------------------------------------------------------------------------------------------
N_ROWS = 212
MODEL_PATTERN = (1, 3, 7, 2, 30, 5, 1, 1, 13, 4, 2, 20)


def _series(device):
    g = torch.Generator().manual_seed(10)
    out = []
    for s in range(3):
        v = torch.rand(N_ROWS, F, generator=g)
        v[40 + 20 * s:55 + 20 * s] += 1.5                       # what the model cannot forecast: a stretch of high scores
        v[120 + 10 * s:150, :3] -= 1.0
        v[170:172 + s] += 2.0
        out.append(v)
    return torch.stack(out).to(device)


def _push_all(scorer, series, order=(0, 1, 2)):
    rows = series[list(order)]
    parts, at, k = [], 0, 0
    while at < N_ROWS:
        T = min(MODEL_PATTERN[k % len(MODEL_PATTERN)], N_ROWS - at)
        parts.append(scorer.push(rows[:, at:at + T] if T > 1 or k % 2 else rows[:, at]))      # (n, F) is one row per stream
        at, k = at + T, k + 1
    return {key: torch.cat([part[key] for part in parts], dim=1).cpu().numpy() for key in FIELDS}


@pytest.mark.parametrize("case", ["plain", "target_dims", "scaled_smoothed"])
def test_streamed_scores_match_the_batch_route(case, gpu_device):
    from streaming import StreamScorer
    series = _series(gpu_device)
    dims = [5, 0, 3] if case == "target_dims" else None
    model = _model(3 if dims else F, gpu_device, seed=11 if dims else 9)
    gamma, span, scale = 0.8, None, None
    n = N_ROWS - W
    with torch.no_grad():
        batch = [model.anomaly_scores(series[s], target_dims=dims, gamma=gamma) for s in range(3)]
    batch_scores = np.stack([b[0].cpu().numpy() for b in batch])
    if case == "scaled_smoothed":
        import evaluation
        span = 5
        q = evaluation.column_quantiles(batch[0][1], [0.25, 0.5, 0.75])                 # "training" scores: the first series'
        scale = (q[1], q[2] - q[0])
        c64, s64 = scale[0].cpu().numpy().astype(np.float64), scale[1].cpu().numpy().astype(np.float64)
        scaled = [((b[1].cpu().numpy().astype(np.float64) - c64) / (1.0 + s64)).mean(axis=1) for b in batch]
        batch_scores = np.stack([score_refs.ewm(v, span) for v in scaled])

    # the threshold sits in the widest gap of the batch scores between their 60th and 95th percentiles
    flat = np.sort(batch_scores.reshape(-1).astype(np.float64))
    lo, hi = int(0.60 * (flat.size - 1)), int(0.95 * (flat.size - 1))
    at = lo + int(np.argmax(np.diff(flat[lo:hi + 1])))
    threshold = float(0.5 * (flat[at] + flat[at + 1]))

    kw = dict(target_dims=dims, gamma=gamma, smoothing_span=span, scale=scale, merge_gap=2, min_length=2, max_block=30)
    scorer = StreamScorer(model, 3, threshold, **kw)
    out = _push_all(scorer, series)
    assert out["scores"].shape == (3, N_ROWS) and out["per_dim"].shape == (3, N_ROWS, model.out_dim)
    warm = np.isnan(out["scores"])
    assert warm[:, :W].all() and not warm[:, W:].any(), "exactly W rows of warm-up per stream"
    streamed = out["scores"][:, W:]
    err = np.abs(streamed.astype(np.float64) - batch_scores)
    assert np.all(err <= FP32_TOL * np.maximum(1.0, np.abs(batch_scores))), (case, float(err.max()))
    if case != "scaled_smoothed":
        per_dim = np.stack([b[1].cpu().numpy() for b in batch])
        assert np.abs(out["per_dim"][:, W:] - per_dim).max() <= FP32_TOL * max(1.0, float(np.abs(per_dim).max()))

    # events: exactly those of the streamed scores
    flushed = _flush(scorer)
    _assert_events(out, flushed, 2, 2, case, threshold)
    flags = out["flags"][:, W:].astype(bool)
    assert (out["closed_start"] >= 0).any() or (flushed["closed_start"] >= 0).any(), "at least one event"
    assert flags.any() and (~flags).any(), "flagged and unflagged stretches"

    # a second scorer on the same model, the streams permuted: the same bits
    order = (2, 0, 1)
    other = _push_all(StreamScorer(model, 3, threshold, **kw), series, order)
    for key in FIELDS:
        assert other[key].tobytes() == out[key][list(order)].tobytes(), (case, key)

