"""Non-finite samples poison exactly their own windows on every GPU route (the contract of include/mtadgat.h; cases and the pure
`affected` functions in tests/nonfinite_cases.py; models, inputs and float64 references from tests/test_host_nonfinite.py, which holds
the torch-op algebra to the same contract on the CPU).

Per run: the engine's plan and routes must equal the hand-written table before the call -- a call that leaves its route fails --,
then ONE call carries all bad samples of the run (NaN, +inf and -inf at the window's corners and just inside the convolution's
padding; windows 0, n - 1, 15 | 16, 31 | 32, 63 | 64, 255 | 256 and both sides of every piece edge), and
  * isnan of every output, reduced per window with `all` and with `any`, equals `affected`;
  * the clean windows are within helpers.FP32_TOL (1e-5) of the float64 model in the fp32 arithmetics, gru_route_cases.BF16_TOL
    (2e-2) in the bf16 mode;
  * the clean windows are within gru_route_cases.FP32_REL_TOL * max(1, |ref64|max) (bf16: BF16_TOL) of the same call on the clean
    input -- the bad samples replaced by 0.5 --: the bound the suite holds between any two routes, so a range guard may fall back for
    the launch and nothing more.
The measured maxima are printed.  Gradients, attention maps and attributions of non-finite input are unspecified and not asked."""
import numpy as np
import pytest
import torch

import gru_route_cases as rc
import helpers
import loss_refs
import nonfinite_cases as nf
from test_host_nonfinite import (TRAIN_CASE, case_options, front_description, geometry, new_model, poisoned, reference64, torch_forward,
                                 window_nan)

pytestmark = pytest.mark.gpu


def _tols(mode, ref64_clean):
    """(against float64, against the clean call) for outputs whose float64 reference on the clean windows is ref64_clean."""
    if mode == 1:
        return rc.BF16_TOL, rc.BF16_TOL
    return helpers.FP32_TOL, rc.FP32_REL_TOL * max(1.0, ref64_clean.abs().max().item())


def check_outputs(what, mode, mask, named):
    """named: [(name, ours on the bad input, ours on the clean input, float64 reference of the clean windows' input)] with windows
    along dim 0; mask (n,) bool: the affected windows.  Returns the printed line."""
    assert 2 * int(mask.sum()) <= mask.numel() and mask.any(), what
    clean = ~mask
    parts = []
    for name, bad_out, clean_out, ref in named:
        every, some = window_nan(bad_out)
        wrong = (every != mask).nonzero().flatten().tolist()
        assert not wrong, (what, name, "isnan.all per window differs from `affected` at windows", wrong[:8],
                           "affected there:", mask[wrong[:8]].tolist())
        wrong = (some != mask).nonzero().flatten().tolist()
        assert not wrong, (what, name, "isnan.any per window differs from `affected` at windows", wrong[:8])
        assert torch.isfinite(clean_out).all(), (what, name, "the clean call is not finite")
        ours, ref = bad_out.detach().cpu().double()[clean].flatten(1), ref.double()[clean].flatten(1)
        tol64, tol_clean = _tols(mode, ref)
        d64 = (ours - ref).abs().amax(1)
        dcl = (ours - clean_out.detach().cpu().double()[clean].flatten(1)).abs().amax(1)
        parts.append(f"{name}: |ours - ref64| {d64.max().item():.2e} (<= {tol64:.0e}), |ours - clean call| {dcl.max().item():.2e} (<= {tol_clean:.1e})")
        rows = clean.nonzero().flatten()
        over = rows[d64 > tol64].tolist()
        assert not over, (what, name, f"clean windows {over[:8]} are {d64.max().item():.3e} from the float64 model, beyond {tol64:.1e}")
        over = rows[dcl > tol_clean].tolist()
        assert not over, (what, name, f"clean windows {over[:8]} are {dcl.max().item():.3e} from the clean call, beyond {tol_clean:.2e}")
    line = f"{what}: {int(mask.sum())} of {mask.numel()} windows affected; " + "; ".join(parts)
    print(line)
    return line


# ---- windows: the front-end and recurrence routes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("run", nf.RUNS, ids=nf.RUN_IDS)
def test_windows_with_a_bad_sample_answer_nan_on_every_route(run, gpu_device):
    import _native
    c, rot = run
    what = f"{c['id']} run {rot}"
    key, mode, n = c["model"], c["mode"], c["n"]
    bf16_in = c["source"] == "windows_bf16"
    bad, clean, mask, smp = poisoned(key, c["pieces"], rot, bf16=bf16_in)
    ref = reference64(key, n, bf16=bf16_in)
    model = new_model(key).to(gpu_device)
    model.precision = rc.MODES[mode]
    eng = model._sync_engine(gpu_device, bf16=mode == 1)
    options = case_options(c)
    try:
        eng.set_precision(mode)
        for k, v in options.items():
            eng.set_option(k, v)
        # before the call: a call that leaves its route fails
        pieces = [p for _, p, _ in eng.forward_plan(n)["pieces"]]
        assert pieces == c["pieces"], (what, pieces)
        if c["family"] == "front":
            route = front_description(eng.front_route(_native.FRONT_KINDS.index("forward"), _native.FRONT_SOURCES.index(c["source"]), n))
            assert route == c["route"], (what, route)
        else:
            _, routes = helpers.call_routes(eng, n, helpers.device_compute_units(gpu_device))
            assert routes == c["routes"], (what, routes)
            fronts = {front_description(eng.front_route(_native.FRONT_KINDS.index("forward"), _native.FRONT_SOURCES.index("windows"), p))
                      for p in pieces}
            what += " (front end: " + ", ".join(sorted(fronts)) + ")"
        to_dev = (lambda t: t.to(gpu_device).bfloat16().contiguous()) if bf16_in else (lambda t: t.to(gpu_device))
        preds, recons = eng.forward(to_dev(bad))
        preds_c, recons_c = eng.forward(to_dev(clean))
        torch.cuda.synchronize()
    finally:
        for k in options:
            eng.set_option(k, 0)
        eng.set_precision(2)
        model._finish_weight_check()
    check_outputs(what + " " + ",".join(sorted({v for *_, v in smp})), mode, mask,
                  [("preds", preds, preds_c, ref[0]), ("recons", recons, recons_c, ref[1])])


# ---- a series: forward_series, score_series, explicit starts, series_losses ----------------------------------------------------------
_SERIES, _STREAM = {}, {}


def _series_setup(gpu_device):
    """The shared-rows model on the GPU with the case's options set for the module's lifetime of the engine, its clean series and the
    float64 reference of all its unit-stride windows.  Built once."""
    import test_gpu_front_route as fr
    if not _SERIES:
        W, F, pad = geometry(nf.SERIES_MODEL)
        n = nf.SERIES_WINDOWS
        n_rows = n + W - 1
        series = torch.rand(n_rows, F, generator=torch.Generator().manual_seed(nf.X_SEED + 1))
        windows = series.unfold(0, W, 1).permute(0, 2, 1).contiguous()
        model = new_model(nf.SERIES_MODEL)
        ref = torch_forward(helpers.model64(model), windows)
        _SERIES.update(model=model.to(gpu_device), series=series, ref=ref, options=dict(fr.CASES[nf.SERIES_MODEL][1]), n=n, n_rows=n_rows)
    return _SERIES


@pytest.mark.parametrize("rot", range(3))
@pytest.mark.parametrize("group", range(3))
def test_series_rows_poison_exactly_the_windows_that_hold_them(group, rot, gpu_device):
    import _native
    S = _series_setup(gpu_device)
    W, F, pad = geometry(nf.SERIES_MODEL)
    n, n_rows, model = S["n"], S["n_rows"], S["model"]
    smp = nf.series_samples(n_rows, W, F, pad, group, rot)
    what = f"series rows {[(r, f, v) for r, f, v in smp]}"
    bad, clean = S["series"].clone(), S["series"].clone()
    for r, f, v in smp:
        bad[r, f] = nf.VALUES[v]
        clean[r, f] = nf.CLEAN_VALUE
    rows = [(r, f) for r, f, _ in smp]
    mask = torch.tensor(nf.affected(n, W, rows, "series"))
    for r, _ in rows:                                            # the windows just outside each span are clean in this call
        assert all(not mask[w] for w in (r - W, r + 1) if 0 <= w < n)
    starts = torch.arange(0, n, nf.SERIES_STRIDE)
    mask_s = torch.tensor(nf.affected(len(starts), W, rows, ("series", starts.tolist())))
    bad_d, clean_d, starts_d = bad.to(gpu_device), clean.to(gpu_device), starts.to(gpu_device)
    dims = list(range(model.out_dim))                            # the series columns the outputs are compared with
    model.precision = "fp32"
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    kind, unit, strided = _native.FRONT_KINDS.index("forward"), _native.FRONT_SOURCES.index("series_unit"), _native.FRONT_SOURCES.index("series")
    try:
        for k, v in S["options"].items():
            eng.set_option(k, v)
        assert front_description(eng.front_route(kind, unit, n)) == nf.SERIES_ROUTE
        assert front_description(eng.front_route(kind, unit, n - 1)) == nf.SERIES_LOSSES_ROUTE
        assert front_description(eng.front_route(kind, strided, len(starts))) == nf.SERIES_STRIDED_ROUTE
        assert [p for _, p, _ in eng.forward_plan(n)["pieces"]] == [n] and eng.series_losses_chunk() >= n - 1
        with torch.no_grad():
            p, r = model.forward_series(bad_d)
            p_c, r_c = model.forward_series(clean_d)
            sp, sl = model.score_series(bad_d)
            sp_c, sl_c = model.score_series(clean_d)
            tp, tr = model.forward_series(bad_d, starts=starts_d)
            tp_c, tr_c = model.forward_series(clean_d, starts=starts_d)
            lp, lr = model.forward_series(bad_d, count=n - 1)    # the windows of series_losses, for tests/loss_refs.py
            losses = model.series_losses(bad_d, target_dims=dims)
        torch.cuda.synchronize()
    finally:
        for k in S["options"]:
            eng.set_option(k, 0)
        model.precision = "auto"
    ref_p, ref_r = S["ref"]
    assert p.shape[0] == n and sp.shape[0] == n - 1 and tp.shape[0] == len(starts) and losses.n_windows == n - 1
    check_outputs(what + ": forward_series", 2, mask, [("preds", p, p_c, ref_p), ("recons", r, r_c, ref_r)])
    # score_series: preds of windows 0 .. n-2, the last reconstruction step of windows 1 .. n-1
    check_outputs(what + ": score_series preds", 2, mask[:n - 1], [("preds", sp, sp_c, ref_p[:n - 1])])
    check_outputs(what + ": score_series recons_last", 2, mask[1:], [("recons_last", sl, sl_c, ref_r[1:, -1])])
    check_outputs(what + f": starts with stride {nf.SERIES_STRIDE}", 2, mask_s,
                  [("preds", tp, tp_c, ref_p[starts]), ("recons", tr, tr_c, ref_r[starts])])
    # series_losses: window_sse is NaN exactly on the affected windows, in both columns.  The window r - W just outside a span is
    # clean, but its forecast is compared with the bad row r itself: where the sample sits in a compared column its forecast column
    # is not finite (NaN, or inf for an infinite target), its reconstruction column is.
    wsse = losses.window_sse.cpu().numpy()
    m = mask[:n - 1].numpy()
    target_bad = np.array([any(r == w + W and f in dims for r, f in rows) for w in range(n - 1)])
    assert not (target_bad & m).any()
    assert np.array_equal(np.isnan(wsse[:, 1]), m), what
    assert np.array_equal(np.isnan(wsse).all(axis=1), m), what
    assert np.array_equal(np.isnan(wsse).any(axis=1)[~target_bad], m[~target_bad]), what
    assert not np.isfinite(wsse[target_bad, 0]).any() and np.isfinite(wsse[target_bad, 1]).all(), what
    with np.errstate(invalid="ignore", over="ignore"):
        ref_w = loss_refs.window_sse(lp.cpu().numpy(), lr.cpu().numpy(), bad.numpy(), np.arange(n - 1), dims)
    od = lp.shape[1]
    for col, terms, keep in ((0, od, ~(m | target_bad)), (1, W * od, ~m)):
        err = np.abs(wsse[keep, col] - ref_w[keep, col])
        assert np.isfinite(ref_w[keep, col]).all() and np.all(err <= loss_refs.bound(terms) * ref_w[keep, col]), (what, col, err.max())
    print(f"{what}: series_losses: {int(m.sum())} of {n - 1} windows NaN, {int((target_bad & ~m).sum())} more in the forecast column")


# ---- streams ---------------------------------------------------------------------------------------------------------------------------
STREAM_GAMMA = 0.25


def _stream_reference(model64, rows):
    """Scores (S, n_rows) in float64 straight from the definition, NaN for the first W rows: row k against the forecast of the window
    k - W .. k - 1 and the last reconstruction step of the window k - W + 1 .. k, all output columns."""
    S, n_rows, F = rows.shape
    W = model64.window_size
    out = torch.full((S, n_rows), float("nan"), dtype=torch.float64)
    for s in range(S):
        windows = rows[s].unfold(0, W, 1).permute(0, 2, 1).contiguous()      # window j: rows j .. j + W - 1
        p, r = torch_forward(model64, windows)
        x = rows[s].double()
        a = (p[:-1] - x[W:]).abs() + STREAM_GAMMA * (r[1:, -1] - x[W:]).abs()
        out[s, W:] = a.mean(1)
    return out


@pytest.mark.parametrize("rot", range(3))
@pytest.mark.parametrize("T", nf.STREAM_PUSHES)
def test_stream_rows_lose_their_score_for_one_window_and_no_other_stream_moves(T, rot, gpu_device):
    from streaming import StreamScorer
    W, F, _ = geometry("stream")
    S, n_rows = nf.STREAMS, nf.STREAM_ROWS
    smp = nf.stream_samples(W, F, rot)
    what = f"stream T={T} samples {smp}"
    rows = torch.rand(S, n_rows, F, generator=torch.Generator().manual_seed(nf.X_SEED + 2))
    model = new_model("stream")
    if "ref" not in _STREAM:
        _STREAM["ref"] = _stream_reference(helpers.model64(model), rows)
    ref = _STREAM["ref"]
    model = model.to(gpu_device)
    model.precision = "fp32"
    bad = rows.clone()
    for s, r, f, v in smp:
        bad[s, r, f] = nf.VALUES[v]
    expect_nan = torch.zeros(S, n_rows, dtype=torch.bool)
    expect_nan[:, :W] = True                                     # a stream's first W rows have no score
    for s in range(S):
        expect_nan[s] |= torch.tensor(nf.affected_rows(n_rows, W, [r for q, r, _, _ in smp if q == s]))
    for s, r, _, _ in smp:
        assert not expect_nan[s, r + W + 1] and expect_nan[s, r:r + W + 1].all()

    def run(data):
        # threshold 0: every finite score is flagged, so "never flagged" is asked of the NaN rows alone; no moving average (it stays
        # NaN by design)
        scorer = StreamScorer(model, S, 0.0, gamma=STREAM_GAMMA, max_block=nf.STREAM_MAX_BLOCK)
        dev = data.to(gpu_device)
        outs = [scorer.push(dev[:, at:at + T]) for at in range(0, n_rows, T)]
        torch.cuda.synchronize()
        return torch.cat([o["scores"] for o in outs], 1).cpu(), torch.cat([o["flags"] for o in outs], 1).cpu()

    try:
        scores, flags = run(bad)
        scores_c, flags_c = run(rows)
    finally:
        model.precision = "auto"
    assert torch.equal(torch.isnan(scores), expect_nan), (what, (torch.isnan(scores) != expect_nan).nonzero()[:8].tolist())
    assert torch.equal(torch.isnan(scores_c), expect_nan & (torch.arange(n_rows) < W)[None, :])
    assert not flags[expect_nan].any(), (what, "a row without a score is flagged")
    ok = ~expect_nan
    assert torch.isfinite(scores[ok]).all() and torch.equal(flags[ok] != 0, scores[ok] > 0), what
    # every row with a score, in the clean streams and around the affected rows alike: against float64 -- the forecast and the
    # reconstruction are each within FP32_TOL, the score is their float64 mean rounded once to float32 -- and against the clean run
    got, want = scores[ok].double(), ref[ok]
    tol64 = (1.0 + STREAM_GAMMA) * helpers.FP32_TOL + 2.0 ** -23 * want.abs()
    tol_clean = (1.0 + STREAM_GAMMA) * rc.FP32_REL_TOL * max(1.0, want.abs().max().item())
    d64, dcl = (got - want).abs(), (got - scores_c[ok].double()).abs()
    print(f"{what}: {int(expect_nan[:, W:].sum())} rows without a score; |ours - ref64| {d64.max().item():.2e}, "
          f"|ours - clean run| {dcl.max().item():.2e} (<= {tol_clean:.1e})")
    assert (d64 <= tol64).all(), (what, d64.max().item())
    assert (dcl <= tol_clean).all(), (what, dcl.max().item())
    others = [s for s in range(S) if s not in {q for q, *_ in smp}]
    assert len(others) == S - 2 and not expect_nan[others][:, W:].any()


# ---- the training forward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "fp32_strict"])
@pytest.mark.parametrize("rot", range(3))
def test_training_forward_answers_nan_for_the_affected_windows(rot, mode, gpu_device):
    from test_host_train_route_cases import assert_case_routes
    c = TRAIN_CASE
    n = c["n"]
    bad, clean, mask, smp = poisoned("train", [n], rot)
    what = f"training forward {mode} n={n} run {rot}"
    ref = reference64("train", n)
    model = new_model("train").to(gpu_device)
    model.precision = mode
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    try:
        assert_case_routes(eng, c, mode, what=what)              # before the call
        with torch.no_grad():
            preds, recons, _ = eng.forward_train(bad.to(gpu_device), 0.0, 0)         # dropout = 0
            preds_c, recons_c, _ = eng.forward_train(clean.to(gpu_device), 0.0, 0)
        torch.cuda.synchronize()
    finally:
        model.precision = "auto"
    check_outputs(what, {"fp32": 2, "fp32_strict": 0}[mode], mask, [("preds", preds, preds_c, ref[0]), ("recons", recons, recons_c, ref[1])])
    # the loss a caller forms is NaN and seen
    y = torch.rand(n, 1, bad.shape[2])
    f_loss, r_loss = helpers.training_loss(preds.cpu(), recons.cpu(), bad[:, :, :recons.shape[2]], y[:, :, :preds.shape[1]], None)
    assert torch.isnan(f_loss) and torch.isnan(r_loss), what
