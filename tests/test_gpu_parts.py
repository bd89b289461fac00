"""Scoring a concatenated series part by part on the device (csrc/mtadgat_parts.hip through evaluation.score_parts,
adjust_part_scores, moving_average(parts=), find_epsilon_parts, part_predictions, MTAD_GAT.anomaly_scores(parts=) and
predict_anomalies(parts=)) against the numpy specification tests/part_refs.py.

Gates
  adjust:     blanked positions and the NaN pattern exact; values within 1 float32 ulp of the float64 reference (ours is rounded once
              from float64: half an ulp; the other half allows for the reference's own rounding next to a tie -- the project's
              convention for quantiles); (n, d) input equal to the column-by-column 1-D result bit for bit.
  ewm:        |ours - ref64| <= 2^-23 |ref64| + 1e-30, the gate of test_moving_average; with one part the bits of moving_average.
  thresholds: 1e-9 relative to eval_oracle.find_epsilon on the slice, the gate of find_epsilon_columns; flags exact.
The sizes sit around 1024: CHUNK_L, SPAN_RB and the scan's chunk are all 1024."""
import warnings

import numpy as np
import pytest
import torch

import part_refs
import score_refs
from oracle import eval_oracle as eo

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 70001]
WINDOWS = (1, 100)


def _transitions(W):
    return [(0, 0), (19, 19), (3, W - 1), (600, 700)]       # the last is wider than the parts around 1024: overlapping, clipped at both ends


def _bits(t):
    return t.contiguous().view(torch.int32)


def _adjust_inputs(n, lengths, W, rng, kinds):
    start, end = part_refs.spans(lengths, W)
    P = len(lengths)
    out = {}
    if "noise" in kinds:
        out["noise"] = (rng.random(n) * 3.0).astype(np.float32)
    if "constant" in kinds:
        x = (rng.random(n) * 3.0).astype(np.float32)
        for p in range(P):
            if p % 2 == 1 or P == 1:
                x[start[p]:end[p]] = 0.625
        out["constant"] = x
    if "special" in kinds:
        x = ((rng.random(n) - 0.5) * 4.0).astype(np.float32)
        for k, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, -0.0, 0.0)):
            x[(k * 37 + 5) % n] = v
        longest = int(np.argmax(end - start))
        if P > 2:
            x[start[longest - 1]:end[longest - 1]] = np.nan                  # an all-NaN part
        x[start[longest] + (end[longest] - start[longest]) // 2] = np.nan   # and a NaN inside an ordinary one
        out["special"] = x
    return out


def _assert_adjusted(got, x, lengths, W, transition, what):
    ref = part_refs.adjust(x, lengths, W, transition)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    same_inf = np.isinf(ref) & (got == ref)
    fin = ~nan & ~same_inf
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= score_refs.ulp32(ref[fin])), (what, float(err.max()))
    assert not np.signbit(got[fin]).any(), (what, "a negative zero or value")


def _assert_blanked(got, x, lengths, W, transition, what):
    """normalize=False: +0.0 in the transitions, the input's bits everywhere else."""
    mask = part_refs.transition_mask(lengths, W, transition)
    want = x.copy()
    want[mask] = 0.0
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), what


@pytest.mark.parametrize("n", SIZES)
def test_adjust_part_scores(n, gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(n)
    for W in WINDOWS:
        for name, lengths in part_refs.layouts(n, W).items():
            many = len(lengths) > 1000
            transitions = _transitions(W)[:2] if many else _transitions(W)
            for kind, x in _adjust_inputs(n, lengths, W, rng, ("noise", "special") if many else ("noise", "constant", "special")).items():
                t = torch.from_numpy(x).to(gpu_device)
                for transition in transitions:
                    what = (n, W, name, kind, transition)
                    sp = ev.score_parts(lengths, W, transition, device=gpu_device)
                    got = ev.adjust_part_scores(t, sp)
                    assert got.shape == (n,) and got.dtype == torch.float32
                    _assert_adjusted(got, x, lengths, W, transition, what)
                    _assert_blanked(ev.adjust_part_scores(t, sp, normalize=False), x, lengths, W, transition, what)
                    assert torch.equal(_bits(got), _bits(ev.adjust_part_scores(t, sp))), (what, "not reproducible")


@pytest.mark.parametrize("layout", ["contiguous", "sliced"])
@pytest.mark.parametrize("d", [1, 3, 65])
def test_adjust_columns_equal_the_one_dimensional_result(d, layout, gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(d)
    for n, W, name in ((257, 1, "short_long"), (4097, 100, "k1024"), (4097, 1, "empty")):
        lengths = part_refs.layouts(n, W)[name]
        cols = [_adjust_inputs(n, lengths, W, rng, ("noise", "constant", "special"))[("noise", "constant", "special")[c % 3]] for c in range(d)]
        a = np.stack(cols, axis=1)
        if layout == "contiguous":
            t = torch.from_numpy(a).to(gpu_device)
        else:
            wide = torch.full((n, d + 5), -7.0, device=gpu_device)          # the neighbours would change every minimum if they were read
            wide[:, 2:2 + d] = torch.from_numpy(a).to(gpu_device)
            t = wide[:, 2:2 + d]
            assert t.stride(0) == d + 5
        for transition in ((19, 19), (3, W - 1)):
            sp = ev.score_parts(lengths, W, transition, device=gpu_device)
            for normalize in (True, False):
                got = ev.adjust_part_scores(t, sp, normalize=normalize)
                assert got.shape == (n, d)
                for c in range(d):
                    one = ev.adjust_part_scores(torch.from_numpy(cols[c]).to(gpu_device), sp, normalize=normalize)
                    assert torch.equal(_bits(got[:, c]), _bits(one)), (n, W, name, c, transition, normalize)
            _assert_adjusted(ev.adjust_part_scores(t, sp), a, lengths, W, transition, (n, W, name, d, layout))
    if layout == "sliced":
        assert torch.equal(wide[:, :2], torch.full((n, 2), -7.0, device=gpu_device)) and torch.equal(wide[:, 2 + d:], torch.full((n, 3), -7.0, device=gpu_device))


def test_adjust_entry_point_reports_lo_and_hi_and_works_in_place(gpu_device):
    """What evaluation.adjust_part_scores does not use of mtadgat_eval_part_adjust: the (count, d, 2) float64 lo / hi output, and an
    output that is the input itself."""
    import evaluation as ev
    lib = ev._lib()
    rng = np.random.default_rng(3)
    n, W, d, transition = 4097, 100, 3, (19, 19)
    lengths = part_refs.layouts(n, W)["empty"]
    P = len(lengths)
    kinds = _adjust_inputs(n, lengths, W, rng, ("noise", "constant", "special"))
    a = np.stack([kinds["noise"], kinds["constant"], kinds["special"]], axis=1)
    sp = ev.score_parts(lengths, W, transition, device=gpu_device)
    x = torch.from_numpy(a).to(gpu_device)
    want = ev.adjust_part_scores(x, sp)
    lohi = torch.full((P, d, 2), 7.0, dtype=torch.float64, device=gpu_device)
    scratch = ev._scratch(lib.mtadgat_eval_part_adjust_scratch(n, d, P), gpu_device)
    rc = lib.mtadgat_eval_part_adjust(x.data_ptr(), n, d, d, sp.start.data_ptr(), sp.end.data_ptr(), P, sp.seams.data_ptr(), sp.seams.numel(),
                                      transition[0], transition[1], 1, scratch.data_ptr(), scratch.numel() * 8, x.data_ptr(), d,
                                      lohi.data_ptr(), ev._stream(x))
    assert rc == 0, lib.mtadgat_last_error()
    assert torch.equal(_bits(x), _bits(want)), "in place"
    blanked = a.astype(np.float64)
    blanked[part_refs.transition_mask(lengths, W, transition)] = 0.0
    ref = np.empty((P, d, 2))
    for p, (s, e) in enumerate(zip(*part_refs.spans(lengths, W))):
        for c in range(d):
            v = blanked[s:e, c]
            v = v[~np.isnan(v)]
            ref[p, c] = (v.min(), v.max()) if v.size else (np.inf, -np.inf)
    got = lohi.cpu().numpy()
    assert np.array_equal(got, ref) and not np.signbit(got[got == 0.0]).any()
    assert (ref[:, :, 0] > ref[:, :, 1]).any() and (ref[:, :, 0] < ref[:, :, 1]).any()       # empty or all-NaN parts among ordinary ones


def test_adjust_checks_the_number_of_scores(gpu_device):
    import evaluation as ev
    sp = ev.score_parts([20, 30], 10)
    x = torch.rand(41, device=gpu_device)
    for call in (lambda: ev.adjust_part_scores(x, sp), lambda: ev.moving_average(x, 5, parts=sp), lambda: ev.find_epsilon_parts(x, sp),
                 lambda: ev.part_predictions(x, sp, [0.5, 0.5]), lambda: ev.adjust_part_scores(torch.rand(41, 2, device=gpu_device), sp)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        ev.part_predictions(x[:40], sp, [0.5])
    with pytest.raises(TypeError):
        ev.adjust_part_scores(x[:40], ([0], [40]))


# ---- segmented moving average ----------------------------------------------------------------------------------------------------
SPANS = (1, 2, 7, 1280)


def _ewm_inputs(n, lengths, W, rng):
    start, end = part_refs.spans(lengths, W)
    spike = np.zeros(n, np.float32)
    spike[n // 2] = 50.0
    scaled = (rng.random(n) + 0.5)
    live = [p for p in range(len(lengths)) if end[p] > start[p]]
    for k, p in enumerate(live):                                 # consecutive parts a factor 1e12 apart: a prefix difference would cancel
        scaled[start[p]:end[p]] *= 1e6 if k % 2 == 0 else 1e-6
    return {"uniform": (rng.random(n) * 3.0).astype(np.float32), "scaled": scaled.astype(np.float32), "spike": spike}


def _assert_ewm_parts(got, x, lengths, W, span, what):
    ref = part_refs.ewm_parts(x, lengths, W, span)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    bound = 2.0 ** -23 * np.abs(ref) + 1e-30
    assert np.all(err <= bound), (what, float((err / bound).max()), int(np.argmax(err / bound)))


@pytest.mark.parametrize("n", SIZES)
def test_moving_average_parts(n, gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(n)
    for W in WINDOWS:
        for name, lengths in part_refs.layouts(n, W).items():
            sp = ev.score_parts(lengths, W, device=gpu_device)
            kinds = _ewm_inputs(n, lengths, W, rng)
            if (W != 1 and name != "k1024") or len(lengths) > 1000:
                kinds = {"scaled": kinds["scaled"]}          # the float64 reference is a Python loop: keep the suite quick
            for kind, x in kinds.items():
                t = torch.from_numpy(x).to(gpu_device)
                for span in SPANS:
                    got = ev.moving_average(t, span, parts=sp)
                    _assert_ewm_parts(got, x, lengths, W, span, (n, W, name, kind, span))
                    assert torch.equal(_bits(got), _bits(ev.moving_average(t, span, parts=sp))), (n, W, name, kind, span)
                    if name == "one":
                        assert torch.equal(_bits(got), _bits(ev.moving_average(t, span))), (n, W, kind, span, "one part is moving_average")


def test_moving_average_with_a_seam_on_every_element_of_a_chunk(gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(11)
    n, W = 4097, 1
    for at in (range(1024, 2049), range(1, 1100), list(range(1000, 1030)) + list(range(3000, 4097, 2))):
        lengths = part_refs.lengths_from_seams(n, W, at)
        sp = ev.score_parts(lengths, W, device=gpu_device)
        for kind, x in _ewm_inputs(n, lengths, W, rng).items():
            for span in SPANS:
                got = ev.moving_average(torch.from_numpy(x).to(gpu_device), span, parts=sp)
                _assert_ewm_parts(got, x, lengths, W, span, (at[0], kind, span))


def test_a_small_part_after_a_large_one_keeps_its_precision(gpu_device):
    """The case a prefix-difference scan loses: values of 1e6 followed by values of 1e-6, the seam in the middle of a chunk and a
    part that spans many chunks on either side."""
    import evaluation as ev
    rng = np.random.default_rng(12)
    n, W = 9000, 1
    lengths = part_refs.lengths_from_seams(n, W, [4500])
    x = (rng.random(n) + 0.5)
    x[:4500] *= 1e6
    x[4500:] *= 1e-6
    x = x.astype(np.float32)
    sp = ev.score_parts(lengths, W, device=gpu_device)
    for span in SPANS:
        got = ev.moving_average(torch.from_numpy(x).to(gpu_device), span, parts=sp)
        _assert_ewm_parts(got, x, lengths, W, span, span)
        assert float(got[4500:].max()) < 2e-6


# ---- thresholds per part -------------------------------------------------------------------------------------------------------------
PART_SCORES = (13, 40, 64, 0, 300, 1023, 1024, 1025, 2500)       # scores per part: both sides of SPAN_RB, and an empty part


def _bursty_parts(W, seed):
    """test_gpu_score_pipeline's _bursty, per part: noise, one burst of 1..11 samples inside every part of 300 scores or more, every
    part on a scale of its own.  Returns (scores, lengths)."""
    rng = np.random.default_rng(seed)
    lengths = list(PART_SCORES)
    lengths[0] += W
    n = sum(PART_SCORES)
    x = rng.random(n) * 0.1
    start, end = part_refs.spans(lengths, W)
    for p, (s, e) in enumerate(zip(start, end)):
        if e - s >= 300:
            at = s + int(rng.integers(60, e - s - 72))
            x[at:at + int(rng.integers(1, 12))] += 1.0 + 2.0 * rng.random()
        x[s:e] *= 10.0 ** (p % 5 - 2)
    return x.astype(np.float32), lengths


@pytest.mark.parametrize("W", WINDOWS)
def test_find_epsilon_parts(W, gpu_device):
    import evaluation as ev
    x, lengths = _bursty_parts(W, 31)
    start, end = part_refs.spans(lengths, W)
    assert (end - start).tolist() == list(PART_SCORES)
    sp = ev.score_parts(lengths, W, device=gpu_device)
    t = torch.from_numpy(x).to(gpu_device)
    for reg in (0, 1, 2):
        ref = part_refs.thresholds(x, lengths, W, reg)
        got = ev.find_epsilon_parts(t, sp, reg_level=reg)
        assert got.shape == (len(lengths),) and got.dtype == np.float64
        for p, (s, e) in enumerate(zip(start, end)):
            if e == s:
                assert got[p] == np.inf and ref[p] == np.inf
                continue
            # both branches of find_epsilon: a short slice never qualifies (its dilation covers it) and gets its maximum, a long one a z
            assert (ref[p] == float(x[s:e].max())) == (e - s <= 64), (p, reg)
            assert abs(got[p] - ref[p]) <= 1e-9 * abs(ref[p]), (W, reg, p, got[p], ref[p])
            one = ev.find_epsilon(t[s:e].clone(), reg)
            assert abs(got[p] - one) <= 1e-9 * abs(one), (W, reg, p, got[p], one)
        again = ev.find_epsilon_parts(t, sp, reg_level=reg)
        assert np.array_equal(got, again)


def test_find_epsilon_parts_with_one_part_is_find_epsilon(gpu_device):
    import evaluation as ev
    x, _ = _bursty_parts(1, 32)
    t = torch.from_numpy(x).to(gpu_device)
    sp = ev.score_parts([x.size + 10], 10, device=gpu_device)
    for reg in (0, 1, 2):
        got, one = ev.find_epsilon_parts(t, sp, reg_level=reg), ev.find_epsilon(t, reg)
        assert got.shape == (1,) and abs(got[0] - one) <= 1e-9 * abs(one), (reg, got, one)


def test_find_epsilon_parts_degenerate_parts(gpu_device):
    """Constant parts, all zeros and a part where no z qualifies, as test_find_epsilon_columns_degenerate_scores asks of the columns."""
    import evaluation as ev
    e = np.zeros(1500, np.float32)
    e[100], e[900] = 3.0, -3.0
    pieces = [np.full(700, 0.25, np.float32), np.zeros(1100, np.float32), e, _bursty_parts(1, 3)[0][-2500:]]
    x = np.concatenate(pieces)
    lengths = [len(p) for p in pieces]
    lengths[0] += 7
    sp = ev.score_parts(lengths, 7, device=gpu_device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for reg in (0, 1, 2):
            got = ev.find_epsilon_parts(torch.from_numpy(x).to(gpu_device), sp, reg_level=reg)
            ref = part_refs.thresholds(x, lengths, 7, reg)
            for p in range(len(pieces)):
                assert abs(got[p] - ref[p]) <= 1e-6 * max(1.0, abs(ref[p])), (p, reg, got[p], ref[p])


@pytest.mark.parametrize("n", [1, 65, 1025, 4097])
def test_part_predictions(n, gpu_device):
    import evaluation as ev
    rng = np.random.default_rng(n)
    for W in WINDOWS:
        for name, lengths in part_refs.layouts(n, W).items():
            P = len(lengths)
            thr = rng.choice(np.array([0.25, 0.5, 1.0, 2.0, np.inf]), size=P)
            x = (rng.random(n) * 3.0).astype(np.float32)
            labels = part_refs.part_labels(lengths, W)
            x[0] = thr[labels[0]] if np.isfinite(thr[labels[0]]) else 0.5       # equal to its threshold: not flagged
            x[n // 2] = np.nan
            x[n - 1] = np.float32(np.nextafter(np.float32(min(thr[labels[n - 1]], 4.0)), np.float32(np.inf)))
            got = ev.part_predictions(torch.from_numpy(x).to(gpu_device), ev.score_parts(lengths, W, device=gpu_device), thr)
            assert got.dtype == torch.uint8 and got.shape == (n,)
            assert np.array_equal(got.cpu().numpy(), part_refs.flags(x, lengths, W, thr)), (n, W, name)
            if n > 2:
                assert got[0].item() == 0 and got[n // 2].item() == 0
                assert got[n - 1].item() == (1 if np.isfinite(thr[labels[n - 1]]) else 0)


# ---- the model and the one-call pipeline -----------------------------------------------------------------------------------------
E2E_W = 10
E2E_LENGTHS = dict(train=[150, 120, 140], test=[170, 160, 130])


def _series(lengths, g):
    """Three parts with very different amplitudes; the second one begins with a start-up transient, which a window that straddles
    the seam cannot forecast."""
    parts = [torch.rand(lengths[0], 5, generator=g), 30.0 * torch.rand(lengths[1], 5, generator=g), 0.05 * torch.rand(lengths[2], 5, generator=g)]
    parts[1][:2] += 500.0
    return torch.cat(parts)


@pytest.fixture(scope="module")
def setup(gpu_device):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(9)
    model = MTAD_GAT(n_features=5, window_size=E2E_W, out_dim=5, kernel_size=3, gru_hid_dim=24, forecast_hid_dim=24,
                     recon_hid_dim=24).to(gpu_device).eval()
    g = torch.Generator().manual_seed(10)
    train, test = _series(E2E_LENGTHS["train"], g), _series(E2E_LENGTHS["test"], g)
    labels = torch.zeros(test.shape[0] - E2E_W, dtype=torch.bool)
    labels[60:85] = True
    labels[400:420] = True
    test[E2E_W + 60:E2E_W + 85] += 1.5
    test[E2E_W + 400:E2E_W + 420] += 0.5
    return model, train.to(gpu_device), test.to(gpu_device), labels.to(gpu_device)


@pytest.mark.parametrize("transition", [(19, 19), (3, E2E_W - 1)])
def test_anomaly_scores_with_parts(setup, transition, gpu_device):
    import evaluation as ev
    model, _, test, _ = setup
    lengths = E2E_LENGTHS["test"]
    sp = ev.score_parts(lengths, E2E_W, transition, device=gpu_device)
    with torch.no_grad():
        raw, per_dim = model.anomaly_scores(test, gamma=0.8)
        x = raw.cpu().numpy()
        mask = part_refs.transition_mask(lengths, E2E_W, transition)
        assert mask[int(np.argmax(x))], "the strongest raw score is a seam artefact"
        got, pd = model.anomaly_scores(test, gamma=0.8, parts=sp)
        _assert_adjusted(got, x, lengths, E2E_W, transition, ("model", transition))
        assert got[int(np.argmax(x))].item() == 0.0 and np.all(got.cpu().numpy()[mask] == 0.0)
        assert torch.equal(_bits(pd), _bits(per_dim)), "the per-dimension scores are as without parts"
        blank, _ = model.anomaly_scores(test, gamma=0.8, parts=sp, normalize_parts=False)
        _assert_blanked(blank, x, lengths, E2E_W, transition, ("model", transition))
        # smoothed per part, then adjusted
        smooth = ev.moving_average(raw, 5, parts=sp)
        _assert_ewm_parts(smooth, x, lengths, E2E_W, 5, ("model", "ewm"))
        both, _ = model.anomaly_scores(test, gamma=0.8, use_mov_av=True, smoothing_span=5, parts=sp)
        _assert_adjusted(both, smooth.cpu().numpy(), lengths, E2E_W, transition, ("model", "ewm + adjust"))
        across, _ = model.anomaly_scores(test, gamma=0.8, use_mov_av=True, smoothing_span=5)
        assert not torch.equal(across, smooth), "without parts the smoothing runs across the seams"
    with pytest.raises(ValueError):
        model.anomaly_scores(test, parts=ev.score_parts([100, 100], E2E_W))


@pytest.mark.parametrize("use_mov_av", [False, True])
@pytest.mark.parametrize("mode", ["global", "per_part"])
def test_predict_anomalies_with_parts(setup, mode, use_mov_av, gpu_device):
    import evaluation as ev
    model, train, test, labels = setup
    transition = (3, E2E_W - 1)
    opts = dict(train_lengths=E2E_LENGTHS["train"], test_lengths=E2E_LENGTHS["test"], transition=transition, thresholds=mode)
    tr_parts = ev.score_parts(E2E_LENGTHS["train"], E2E_W, transition, device=gpu_device)
    te_parts = ev.score_parts(E2E_LENGTHS["test"], E2E_W, transition, device=gpu_device)
    with torch.no_grad():
        out = ev.predict_anomalies(model, train, test, labels=labels, gamma=0.8, use_mov_av=use_mov_av, parts=opts)
        tr_s, tr_pd = model.anomaly_scores(train, gamma=0.8, use_mov_av=use_mov_av, parts=tr_parts)
        te_s, te_pd = model.anomaly_scores(test, gamma=0.8, use_mov_av=use_mov_av, parts=te_parts)
        te_raw, _ = model.anomaly_scores(test, gamma=0.8)
        if use_mov_av:
            te_raw = ev.moving_average(te_raw, int(256 * E2E_W * 0.05), parts=te_parts)
    assert torch.equal(_bits(out["train_scores"]), _bits(tr_s)) and torch.equal(_bits(out["test_scores"]), _bits(te_s))
    assert torch.equal(_bits(out["test_per_dim"]), _bits(te_pd))
    _assert_adjusted(out["test_scores"], te_raw.cpu().numpy(), E2E_LENGTHS["test"], E2E_W, transition, ("pipeline", mode, use_mov_av))
    # the rest of the function as it was, now on the adjusted scores
    want = ev.epsilon_eval(tr_s, te_s, labels, 1)
    assert out["epsilon_result"].keys() == want.keys()
    for k in want:
        assert out["epsilon_result"][k] == want[k] or abs(out["epsilon_result"][k] - want[k]) <= 1e-9 * abs(want[k]), k
    thr, preds = ev.feature_predictions(tr_pd, te_pd, 1)
    assert np.allclose(out["feature_thresholds"], thr, rtol=1e-9, atol=0) and torch.equal(out["feature_preds"], preds)
    if mode == "global":
        assert "part_result" not in out
        return
    res = out["part_result"]
    ref_thr = part_refs.thresholds(tr_s.cpu().numpy(), E2E_LENGTHS["train"], E2E_W, 1)
    assert res["thresholds"].shape == (3,) and np.all(np.abs(res["thresholds"] - ref_thr) <= 1e-9 * np.abs(ref_thr)), (res["thresholds"], ref_thr)
    flags = part_refs.flags(te_s.cpu().numpy(), E2E_LENGTHS["test"], E2E_W, res["thresholds"])
    assert res["preds"].dtype == torch.uint8 and np.array_equal(res["preds"].cpu().numpy(), flags)
    pred, latency = eo.point_adjust(flags.astype(np.float32), labels.cpu().numpy(), 0.5)
    f1, prec, rec, tp, tn, fp, fn = eo.confusion(pred, labels.cpu().numpy())
    assert (res["TP"], res["TN"], res["FP"], res["FN"]) == (tp, tn, fp, fn)
    assert abs(res["f1"] - f1) <= 1e-12 and abs(res["latency"] - latency) <= 1e-9
    # a different number of parts in the training series: the thresholds come from the test scores
    with torch.no_grad():
        other = ev.predict_anomalies(model, train, test, gamma=0.8, use_mov_av=use_mov_av,
                                     parts=dict(test_lengths=E2E_LENGTHS["test"], transition=transition, thresholds="per_part"))
    ref_thr = part_refs.thresholds(other["test_scores"].cpu().numpy(), E2E_LENGTHS["test"], E2E_W, 1)
    assert np.all(np.abs(other["part_result"]["thresholds"] - ref_thr) <= 1e-9 * np.abs(ref_thr))
    assert "TP" not in other["part_result"]


def test_predict_anomalies_without_parts_is_unchanged(setup, gpu_device):
    import evaluation as ev
    model, train, test, labels = setup
    with torch.no_grad():
        a = ev.predict_anomalies(model, train, test, labels=labels, gamma=0.8, use_mov_av=True)
        b = ev.predict_anomalies(model, train, test, labels=labels, gamma=0.8, use_mov_av=True)
        tr_s, _ = model.anomaly_scores(train, gamma=0.8, use_mov_av=True)
    assert a.keys() == b.keys() and "part_result" not in a
    for k, v in a.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, b[k]), k
    assert torch.equal(_bits(a["train_scores"]), _bits(tr_s))
    with pytest.raises(ValueError):
        ev.predict_anomalies(model, train, test, parts=dict(test_lengths=[100, 100]))
