"""Peaks-over-threshold thresholds on the device (csrc/mtadgat_spot.hip through evaluation.spot_calibrate / spot_run / pot_eval)
against the numpy specification tests/spot_refs.py, on the seeded matrices of tests/spot_cases.py: 1, 3, 5 and 70 columns (a wave,
a workgroup boundary, many workgroups), calibrations of 200 and 2000 rows, 600 to 3000 score rows, rings of 8 (they wrap at once)
and 256 excesses (they do not), static and dynamic, with NaN rows, a level shift and a burst of alarms in every matrix.

Gates
  device against the float64 reference (the only approximate comparison: libm and the device's log differ in the last bit and
      bisection amplifies that): tests/spot_cases.py first asserts, on the CPU, that the reference's float64 and long-double runs
      agree to 1e-10 relative on every threshold and that no score lies within 1e-6 relative of the threshold it met or of t; under
      those conditions every device threshold lies within 1e-9 relative of the float64 reference -- the precondition with a factor
      ten -- and flags, events and the counts n and Nt are exactly equal.  The initial threshold t is an order statistic: exact.
  device against device (a run cut in two, a clone, one column serving many): torch.equal.
"""
import numpy as np
import pytest
import torch

import event_refs
import spot_cases

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def _calibrated(case, dynamic, device):
    import evaluation
    S, n_init, rows, max_peaks, level, _ = spot_cases.CASES[case]
    init, x = spot_cases.data(case)
    state = evaluation.spot_calibrate(torch.from_numpy(init).to(device), q=spot_cases.Q, level=level, max_peaks=max_peaks, dynamic=dynamic)
    return state, torch.from_numpy(x).to(device)


def _assert_close(got, ref, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert np.all(err <= RTOL * np.abs(ref)), (what, float(np.max(err / np.abs(ref))))


@pytest.mark.parametrize("dynamic", [True, False], ids=["dynamic", "static"])
@pytest.mark.parametrize("case", list(spot_cases.CASES))
def test_calibrate_and_run_match_the_reference(case, dynamic, gpu_device):
    import evaluation
    S, n_init, rows, max_peaks, level, _ = spot_cases.CASES[case]
    ref = spot_cases.reference(case, dynamic)
    state, x = _calibrated(case, dynamic, gpu_device)
    assert state.n_columns == S and state.max_peaks == max_peaks and state.dynamic == dynamic
    first = state.read()
    assert np.array_equal(first["t"], ref["t"]), (case, "t")
    assert np.all(first["n"] == n_init) and np.array_equal(first["Nt"], (spot_cases.data(case)[0] > ref["t"]).sum(axis=0))
    _assert_close(first["z"], ref["z0"], (case, "calibrated z"))
    assert torch.equal(state.thresholds().cpu(), torch.from_numpy(first["z"]))

    pristine = state.clone()
    thr, flags = evaluation.spot_run(state, x)
    assert thr.shape == (rows, S) and thr.dtype == torch.float64 and flags.shape == (rows, S) and flags.dtype == torch.uint8
    _assert_close(thr.cpu().numpy(), ref["thresholds"], (case, dynamic, "thresholds"))
    got_flags = flags.cpu().numpy().astype(bool)
    assert np.array_equal(got_flags, ref["flags"]), (case, dynamic, "flags")
    assert ref["flags"].any() and not ref["flags"][np.isnan(spot_cases.data(case)[1])].any()
    last = state.read()
    assert np.array_equal(last["n"], ref["n"]) and np.array_equal(last["Nt"], ref["Nt"]), (case, dynamic, "counts")
    if dynamic:
        assert np.all(ref["Nt"] > first["Nt"]) and (np.all(ref["Nt"] > max_peaks) or max_peaks == 256)
        assert np.unique(ref["thresholds"][:, 0]).size > 5, "the threshold moves"
    else:
        assert all(np.array_equal(first[k], last[k]) for k in first), "a static state never changes"
        assert torch.equal(thr, thr[:1].expand(rows, S))
    # events of the flags: the existing run extraction on the device against numpy over the reference's flags
    for c in {0, S // 2, S - 1}:
        count, start, end = evaluation.flag_runs(labels=flags[:, c].contiguous().bool(), merge_gap=2, min_length=2)
        ref_start, ref_end = event_refs.runs(ref["flags"][:, c], 2, 2)
        assert count == len(ref_start) and np.array_equal(start.cpu().numpy(), ref_start) and np.array_equal(end.cpu().numpy(), ref_end)

    # the same rows in two calls, cut inside a block of 64 rows: the same bits, and the same state after them
    twice = pristine.clone()
    cut = 257
    thr_a, flags_a = evaluation.spot_run(twice, x[:cut])
    thr_b, flags_b = evaluation.spot_run(twice, x[cut:])
    assert torch.equal(torch.cat((thr_a, thr_b)), thr) and torch.equal(torch.cat((flags_a, flags_b)), flags), (case, dynamic, "split")
    assert torch.equal(twice.buf, state.buf), (case, dynamic, "state after the split run")
    # a column slice of a wider tensor is read in place; 1-D scores give 1-D results
    wide = torch.cat((x, x), dim=1)
    again = pristine.clone()
    thr_w, flags_w = evaluation.spot_run(again, wide[:, S:])
    assert torch.equal(thr_w, thr) and torch.equal(flags_w, flags)
    if S == 1:
        thr_1, flags_1 = evaluation.spot_run(pristine.clone(), x[:, 0])
        assert thr_1.shape == (rows,) and torch.equal(thr_1, thr[:, 0]) and torch.equal(flags_1, flags[:, 0])


def test_one_column_serves_many_streams(gpu_device):
    import evaluation
    state, x = _calibrated("one column", True, gpu_device)
    many = state.expand(9)
    assert many.n_columns == 9 and torch.equal(many.thresholds(), state.thresholds().expand(9))
    scores = x[:300].expand(300, 9).contiguous().clone()
    scores[:, 4] = x[300:600, 0]                                # one column sees other scores: its neighbours must not notice
    thr, flags = evaluation.spot_run(many, scores)
    solo_thr, solo_flags = evaluation.spot_run(state.clone(), x[:300])
    other_thr, other_flags = evaluation.spot_run(state.clone(), x[300:600])
    for c in range(9):
        want = (other_thr, other_flags) if c == 4 else (solo_thr, solo_flags)
        assert torch.equal(thr[:, c:c + 1], want[0]) and torch.equal(flags[:, c:c + 1], want[1]), c
    with pytest.raises(ValueError):
        many.expand(3)
    with pytest.raises(ValueError):
        evaluation.spot_run(many, x[:10])


def test_calibration_names_the_column_it_refuses(gpu_device):
    import evaluation
    init = torch.from_numpy(spot_cases.data("five columns")[0]).to(gpu_device).clone()
    bad = init.clone()
    bad[7, 3] = float("nan")
    with pytest.raises(RuntimeError, match="column 3 holds a NaN"):
        evaluation.spot_calibrate(bad, level=0.9, max_peaks=64)
    bad = init.clone()
    bad[:, 1] = 0.25                                            # no excess over its own order statistic
    with pytest.raises(RuntimeError, match="column 1 has fewer than 8 excesses"):
        evaluation.spot_calibrate(bad, level=0.9, max_peaks=64)
    with pytest.raises(RuntimeError, match="column 0 has fewer than 8 excesses"):
        evaluation.spot_calibrate(init, level=0.98, max_peaks=64)           # 200 rows: three excesses
    with pytest.raises(ValueError):
        evaluation.spot_calibrate(init[:15], level=0.5)
    # a state used with other sizes than it was calibrated for is refused on the host
    state = evaluation.spot_calibrate(init, level=0.9, max_peaks=64)
    state.n_columns = 4
    with pytest.raises(RuntimeError, match="not calibrated for these sizes"):
        state.read()


def test_pot_eval(gpu_device):
    import evaluation
    init, x = spot_cases.data("one column")
    z0 = spot_cases.reference("one column", False)["z0"][0]
    x = np.nan_to_num(x[:, 0], nan=0.0)                         # the metrics take a score per label
    labels = torch.zeros(x.size, dtype=torch.bool)
    labels[45:75] = True                                        # the burst lies inside
    labels[900:910] = True
    dev_init, dev_x, dev_labels = (torch.from_numpy(v).to(gpu_device) if isinstance(v, np.ndarray) else v.to(gpu_device)
                                   for v in (init[:, 0], x, labels))
    static = evaluation.pot_eval(dev_init, dev_x, dev_labels, q=spot_cases.Q, level=0.98, max_peaks=256)
    assert abs(static["threshold"] - z0) <= RTOL * z0 and static["dynamic"] is False
    want = evaluation._result(evaluation.point_adjust_counts(dev_x, dev_labels, [static["threshold"]])[0], static["threshold"])
    assert {k: static[k] for k in want} == want
    assert static["TP"] >= 30 and set(evaluation.epsilon_eval(dev_init, dev_x, dev_labels)) - {"reg_level"} <= set(static)

    dynamic = evaluation.pot_eval(dev_init, dev_x, dev_labels, q=spot_cases.Q, level=0.98, dynamic=True, max_peaks=256)
    state = evaluation.spot_calibrate(dev_init, q=spot_cases.Q, level=0.98, max_peaks=256)
    thr, flags = evaluation.spot_run(state, dev_x)
    assert dynamic["threshold"] == float(thr.mean().item()) and dynamic["dynamic"] is True
    want = evaluation._result(evaluation.point_adjust_counts(flags.float(), dev_labels, [0.5])[0], dynamic["threshold"])
    assert {k: dynamic[k] for k in want} == want
    flagged = flags.cpu().numpy().astype(bool)
    fp = int((flagged & ~labels.numpy()).sum())
    assert dynamic["FP"] == fp and dynamic["TP"] >= 30
    assert evaluation.pot_eval(dev_init, dev_x, None, level=0.98) == {"threshold": static["threshold"], "q": 1e-3, "level": 0.98, "dynamic": False}


def test_predict_anomalies_with_pot(gpu_device):
    import evaluation
    from mtad_gat import MTAD_GAT
    torch.manual_seed(21)
    model = MTAD_GAT(n_features=3, window_size=5, out_dim=3, kernel_size=3, gru_hid_dim=8, forecast_hid_dim=8, recon_hid_dim=8).to(gpu_device).eval()
    g = torch.Generator().manual_seed(22)
    train = torch.rand(405, 3, generator=g).to(gpu_device)
    test = torch.rand(305, 3, generator=g)
    test[100:110] += 3.0
    test = test.to(gpu_device)
    labels = torch.zeros(300, dtype=torch.bool, device=gpu_device)
    labels[95:112] = True
    plain = evaluation.predict_anomalies(model, train, test, labels=labels, bf_search=(0.01, 2.0, 20))
    assert "pot_result" not in plain
    for pot in (dict(q=1e-2, level=0.9), dict(q=1e-2, level=0.9, dynamic=True)):
        out = evaluation.predict_anomalies(model, train, test, labels=labels, bf_search=(0.01, 2.0, 20), pot=pot)
        assert set(out) == set(plain) | {"pot_result"}
        for key, val in plain.items():                          # (find_epsilon's float64 sums are atomic: equal to rounding)
            if isinstance(val, torch.Tensor):
                assert torch.equal(out[key], val), key
            elif isinstance(val, np.ndarray):
                assert np.allclose(out[key], val, rtol=1e-9, atol=0.0), key
            else:
                assert out[key] == pytest.approx(val, rel=1e-9), key
        want = evaluation.pot_eval(plain["train_scores"], plain["test_scores"], labels, max_peaks=1024, **pot)
        assert out["pot_result"] == want and want["TP"] > 0
    assert evaluation.predict_anomalies(model, train, test, pot=dict(level=0.9))["pot_result"].keys() == {"threshold", "q", "level", "dynamic"}
    with pytest.raises(ValueError):
        evaluation.predict_anomalies(model, train, test, pot=dict(risk=1e-3))
