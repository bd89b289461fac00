"""From thresholded scores to events on the device (csrc/mtadgat_events.hip through evaluation.flag_runs, run_statistics,
first_hits, anomaly_events, explain_events and predict_anomalies(events=...)) against the numpy reference of tests/event_refs.py.

Gates
  runs, peaks, hit counts, first hits, latencies, rankings: exact.
  mean_score, feature_means: |ours - ref| <= 1 float32 ulp of the reference.  Both are float64 sums divided by the length; ours is
      then rounded once to float32 (half an ulp), and the float64 sums differ only in their order (about 1e-16 relative for the
      non-negative data used here), which matters next to a rounding tie -- hence one ulp, not a half.
"""
import ctypes

import numpy as np
import pytest
import torch

import evaluation as ev
import event_refs
import score_refs

pytestmark = pytest.mark.gpu

CHUNK = ev.RUNS_CHUNK
SIZES = sorted({1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 70001, CHUNK - 1, CHUNK, CHUNK + 1})
THR = 0.5


def _run_inputs(n, rng):
    """kind -> float32 scores, to be flagged against THR."""
    idx = np.arange(n)
    noise = np.convolve(rng.random(n + 4), np.ones(5) / 5.0, mode="valid")[:n].astype(np.float32)
    straddle = np.zeros(n, np.float32)
    for c in range(CHUNK, n, CHUNK):                     # a run across every chunk boundary, and one at either end of the array
        straddle[c - 3:c + 3] = 1.0
    straddle[0] = straddle[n - 1] = 1.0
    special = rng.random(n).astype(np.float32)
    for j, v in enumerate((np.nan, np.inf, -np.inf, THR, np.nan, np.inf, np.float32(np.nextafter(np.float32(THR), np.float32(1))))):
        special[(j * 37 + 5) % n] = v
    return {"noise": noise, "below": np.zeros(n, np.float32), "above": np.ones(n, np.float32), "alternating": (idx % 2).astype(np.float32),
            "straddle": straddle, "special": special}


def _assert_runs(got, ref, what):
    count, start, end = got
    assert start.dtype == torch.int64 and end.dtype == torch.int64 and start.device.type == "cuda"
    assert count == len(ref[0]) == start.numel() == end.numel(), (what, count, len(ref[0]))
    assert np.array_equal(start.cpu().numpy(), ref[0]) and np.array_equal(end.cpu().numpy(), ref[1]), what


@pytest.mark.parametrize("n", SIZES)
def test_run_extraction(n, gpu_device):
    rng = np.random.default_rng(n)
    for kind, x in _run_inputs(n, rng).items():
        t = torch.from_numpy(x).to(gpu_device)
        flag = event_refs.flags(x, THR)
        if kind == "below":
            assert not flag.any()
        if kind == "above":
            assert flag.all()
        for gap in (0, 1, 2, 7, n):
            for min_length in (1, 2, 5, n + 1):
                ref = event_refs.runs(flag, gap, min_length)
                _assert_runs(ev.flag_runs(scores=t, threshold=THR, merge_gap=gap, min_length=min_length), ref, (n, kind, gap, min_length))
        # the same flags as labels
        _assert_runs(ev.flag_runs(labels=torch.from_numpy(flag).to(gpu_device), merge_gap=2, min_length=2), event_refs.runs(flag, 2, 2),
                     (n, kind, "labels"))
    assert ev.flag_runs(scores=torch.zeros(n, device=gpu_device), threshold=THR)[0] == 0
    one = ev.flag_runs(scores=torch.ones(n, device=gpu_device), threshold=THR, merge_gap=n)
    assert one[0] == 1 and one[1].tolist() == [0] and one[2].tolist() == [n]


@pytest.mark.parametrize("n", [1, 65, CHUNK + 1])
def test_comparison_precision(n, gpu_device):
    """float32(0.1) > 0.1 in float64 (a float32 array against a Python float), not in float32; equality and NaN are not flagged."""
    t = torch.full((n,), 0.1, dtype=torch.float32, device=gpu_device)
    count, start, end = ev.flag_runs(scores=t, threshold=0.1)
    assert count == 1 and start.tolist() == [0] and end.tolist() == [n]
    assert ev.flag_runs(scores=t, threshold=0.1, compare_f32=True)[0] == 0
    assert ev.flag_runs(scores=torch.full((n,), 0.5, device=gpu_device), threshold=0.5)[0] == 0
    assert ev.flag_runs(scores=torch.full((n,), float("nan"), device=gpu_device), threshold=-1.0)[0] == 0
    assert ev.flag_runs(scores=torch.full((n,), float("inf"), device=gpu_device), threshold=1e30)[0] == 1


def _c_runs(lib, t, gap, min_length, cap, fill=0xFF, thr=THR):
    n = t.numel()
    nbytes = lib.mtadgat_eval_runs_scratch(n)
    scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=t.device)
    start = torch.full((cap,), -99, dtype=torch.int64, device=t.device)
    end = torch.full((cap,), -99, dtype=torch.int64, device=t.device)
    count = ctypes.c_int64(-1)
    rc = lib.mtadgat_eval_runs(t.data_ptr(), None, n, thr, 0, gap, min_length, cap, scratch.data_ptr(), nbytes, start.data_ptr(), end.data_ptr(),
                               ctypes.byref(count), ev._stream(t))
    return rc, count.value, start, end


def test_more_runs_than_capacity(gpu_device):
    lib = ev._lib()
    n = 4097
    x = (np.arange(n) % 2 == 0).astype(np.float32)
    t = torch.from_numpy(x).to(gpu_device)
    ref = event_refs.runs(event_refs.flags(x, THR))
    assert len(ref[0]) == 2049
    rc, count, start, end = _c_runs(lib, t, 0, 1, 100)
    assert rc == -5 and count == 2049 and "max_runs" in lib.mtadgat_last_error().decode()
    assert np.array_equal(start.cpu().numpy(), ref[0][:100]) and np.array_equal(end.cpu().numpy(), ref[1][:100])
    rc, count, start, end = _c_runs(lib, t, 0, 1, 2049)
    assert rc == 0 and count == 2049 and np.array_equal(start.cpu().numpy(), ref[0])
    _assert_runs(ev.flag_runs(scores=t, threshold=THR, max_runs=100), ref, "retry")
    out = ev.anomaly_events(t, THR, max_events=7)
    assert out["count"] == 2049 and np.array_equal(out["peak"].cpu().numpy(), ref[0])


# ---- statistics ------------------------------------------------------------------------------------------------------------------
def _stats_input(kind, d, seed):
    """scores (n,), per_dim (n, d), thresholds (d,), runs: `short` thousands of runs of 1-4 samples, `long` a run over several row blocks."""
    rng = np.random.default_rng(seed)
    n = 20000 if kind == "short" else 6000
    per_dim = rng.random((n, d)).astype(np.float32)
    per_dim[:, d // 2] = np.round(per_dim[:, d // 2] * 4) / 4          # a column of ties with its threshold below
    if d >= 3:
        per_dim[::7, 1] = np.nan                                         # this column's mean is NaN in all but the shortest runs
        per_dim[:, 2] = per_dim[:, 0]                                    # equal means: the lower column ranks first
    scores = rng.random(n).astype(np.float32)
    scores[rng.integers(0, n, 40)] = np.nan
    scores[rng.integers(0, n, 40)] = 0.75                                # repeated maxima: the first index wins
    flag = np.zeros(n, bool)
    if kind == "short":
        at = 0
        while at < n:
            length = int(rng.integers(1, 5))
            flag[at:at + length] = True
            at += length + int(rng.integers(1, 4))
    else:
        flag[100:5300] = True
        flag[0:3] = flag[5400:5401] = flag[n - 2:n] = True
    thr = rng.random(d) * 0.4 + 0.3
    thr[d // 2] = 0.5
    return scores, per_dim, thr, event_refs.runs(flag)


def _assert_ulp(got, ref, what):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    err = np.abs(got[~nan] - ref[~nan])
    assert np.all(err <= score_refs.ulp32(ref[~nan])), (what, float(err.max()))


def _top_ks(d):
    return sorted({1, min(d, 16), min(d, 64)})


@pytest.mark.parametrize("kind", ["short", "long"])
@pytest.mark.parametrize("d", [1, 3, 64, 65, 130])
def test_run_statistics(d, kind, gpu_device):
    scores, per_dim, thr, (start, end) = _stats_input(kind, d, 10 * d + len(kind))
    assert (len(start) > 3000) if kind == "short" else (end - start).max() > 5 * 1024
    n = scores.size
    wide = torch.full((n, d + 5), 9.0, device=gpu_device)                # the neighbours would change every mean if they were read
    wide[:, 2:2 + d] = torch.from_numpy(per_dim).to(gpu_device)
    pd = wide[:, 2:2 + d]
    assert pd.stride(0) == d + 5
    s = torch.from_numpy(scores).to(gpu_device)
    st, en = torch.from_numpy(start).to(gpu_device), torch.from_numpy(end).to(gpu_device)
    ref = event_refs.stats(scores, start, end, per_dim, thr, min(d, 64))          # a smaller top_k is a prefix of the ranking
    for top_k in _top_ks(d):
        got = ev.run_statistics(s, st, en, per_dim=pd, feature_thresholds=thr, top_k=top_k)
        assert got["peak"].dtype == torch.int64 and got["top_features"].dtype == torch.int32 and got["feature_hits"].dtype == torch.int32
        assert np.array_equal(got["peak"].cpu().numpy(), ref["peak"]), (d, kind)
        assert np.array_equal(got["peak_score"].cpu().numpy(), ref["peak_score"]), (d, kind)
        assert np.array_equal(got["feature_hits"].cpu().numpy(), ref["feature_hits"]), (d, kind)
        _assert_ulp(got["mean_score"], ref["mean_score"], (d, kind, "mean_score"))
        _assert_ulp(got["feature_means"], ref["feature_means"], (d, kind, "feature_means"))
        means = got["feature_means"].cpu().numpy()
        k = min(top_k, d)
        order = np.stack([np.argsort(-row, kind="stable")[:k] for row in means]) if len(means) else np.empty((0, k), np.int64)
        assert got["top_features"].shape == (len(start), k)
        assert np.array_equal(got["top_features"].cpu().numpy(), order), (d, kind, top_k)
        assert np.array_equal(got["top_values"].cpu().numpy(), np.take_along_axis(means, order, axis=1), equal_nan=True), (d, kind, top_k)
        if d >= 3 and top_k == min(d, 64) and d <= 64:
            nan_rows = np.isnan(means[:, 1])
            assert nan_rows.any() and np.all(got["top_features"].cpu().numpy()[nan_rows, -1] == 1), "a NaN mean ranks last"
            first0 = [list(r).index(0) for r in order]
            assert all(list(r).index(2) == p + 1 for r, p in zip(order, first0)), "equal means: the lower column first"
    # without per_dim / without thresholds only the keys that apply come back, with the same bits
    bare = ev.run_statistics(s, st, en)
    assert set(bare) == {"peak", "peak_score", "mean_score"} and torch.equal(bare["peak"], got["peak"])
    assert torch.equal(bare["mean_score"].view(torch.int32), got["mean_score"].view(torch.int32))
    half = ev.run_statistics(s, st, en, per_dim=pd, top_k=1)
    assert "feature_hits" not in half and torch.equal(half["feature_means"].view(torch.int32), got["feature_means"].view(torch.int32))


def test_top_k_is_clipped_and_checked(gpu_device):
    s = torch.rand(50, device=gpu_device)
    pd = torch.rand(50, 3, device=gpu_device)
    out = ev.anomaly_events(s, 0.5, per_dim=pd, top_k=5)
    assert out["top_features"].shape == (out["count"], 3) and out["count"] > 0
    with pytest.raises(ValueError):
        ev.anomaly_events(s, 0.5, per_dim=pd, top_k=0)
    with pytest.raises(ValueError):
        ev.anomaly_events(s, 0.5, per_dim=pd[:40])
    with pytest.raises(ValueError):
        ev.anomaly_events(s, 0.5, merge_gap=-1)
    with pytest.raises(ValueError):
        ev.anomaly_events(s, 0.5, min_length=0)


def test_no_events_gives_empty_tensors(gpu_device):
    s = torch.rand(300, device=gpu_device)
    out = ev.anomaly_events(s, 2.0, per_dim=torch.rand(300, 7, device=gpu_device), feature_thresholds=[0.5] * 7, labels=s > 0.9, top_k=4)
    assert out["count"] == 0
    shapes = {"start": (0,), "end": (0,), "peak": (0,), "peak_score": (0,), "mean_score": (0,), "feature_means": (0, 7), "top_features": (0, 4),
              "top_values": (0, 4), "feature_hits": (0, 7), "event_is_true": (0,)}
    for key, shape in shapes.items():
        assert tuple(out[key].shape) == shape and out[key].device.type == "cuda", key
    assert out["event_is_true"].dtype == torch.bool
    seg = out["segments"]
    assert seg["start"].numel() > 0 and torch.all(seg["first_hit"] == -1) and torch.all(seg["latency"] == -1)


# ---- contract --------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b, what=""):
    assert a.keys() == b.keys(), what
    for k in a:
        if isinstance(a[k], dict):
            _same_bits(a[k], b[k], k)
        elif isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) if a[k].numel() else True, (what, k)
        else:
            assert a[k] == b[k], (what, k)


def test_results_are_bitwise_reproducible(gpu_device):
    scores, per_dim, thr, _ = _stats_input("long", 38, 77)
    scores = np.nan_to_num(scores, nan=0.9)
    s, pd = torch.from_numpy(scores).to(gpu_device), torch.from_numpy(per_dim).to(gpu_device)
    labels = torch.from_numpy(scores > 0.8).to(gpu_device)
    kw = dict(per_dim=pd, feature_thresholds=thr, labels=labels, merge_gap=3, min_length=2, top_k=5)
    first = ev.anomaly_events(s, 0.6, **kw)
    again = ev.anomaly_events(s, 0.6, **kw)
    assert first["count"] > 100
    _same_bits(first, again)
    # the C entry points with scratch pre-filled with 0xFF bytes, and with zeros: nothing is read before it is written
    lib = ev._lib()
    n, d, count = s.numel(), 38, first["count"]
    thr_d = torch.tensor(thr, dtype=torch.float64, device=gpu_device)
    for fill in (0xFF, 0x00):
        rc, cnt, start, end = _c_runs(lib, s, 3, 2, count, fill, thr=0.6)
        assert rc == 0 and cnt == count and torch.equal(start, first["start"]) and torch.equal(end, first["end"])
        nbytes = lib.mtadgat_eval_run_stats_scratch(n, count, d)
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=gpu_device)
        out = {"peak": torch.empty(count, dtype=torch.int64, device=gpu_device), "peak_score": torch.empty(count, device=gpu_device),
               "mean_score": torch.empty(count, device=gpu_device), "feature_means": torch.empty(count, d, device=gpu_device),
               "top_features": torch.empty(count, 5, dtype=torch.int32, device=gpu_device), "top_values": torch.empty(count, 5, device=gpu_device),
               "feature_hits": torch.empty(count, d, dtype=torch.int32, device=gpu_device)}
        rc = lib.mtadgat_eval_run_stats(s.data_ptr(), n, start.data_ptr(), end.data_ptr(), count, pd.data_ptr(), d, d, thr_d.data_ptr(), 5,
                                        scratch.data_ptr(), nbytes, out["peak"].data_ptr(), out["peak_score"].data_ptr(),
                                        out["mean_score"].data_ptr(), out["feature_means"].data_ptr(), out["top_features"].data_ptr(),
                                        out["top_values"].data_ptr(), out["feature_hits"].data_ptr(), ev._stream(s))
        assert rc == 0, lib.mtadgat_last_error().decode()
        _same_bits(out, {k: first[k] for k in out}, f"fill {fill:#x}")


# ---- labels ----------------------------------------------------------------------------------------------------------------------
def _labels(n, rng, first=False):
    lab = np.convolve(rng.random(n + 8), np.ones(9) / 9.0, mode="valid")[:n] > 0.56
    lab[0] = first
    return lab


@pytest.mark.parametrize("n", [1, 2, 300, 5000, 70001])
def test_labelled_segments(n, gpu_device):
    rng = np.random.default_rng(n + 3)
    scores = rng.random(n).astype(np.float32)
    s = torch.from_numpy(scores).to(gpu_device)
    for thr, f32, first in ((0.9, False, False), (0.97, True, False), (0.5, False, False), (2.0, False, False), (0.97, False, True)):
        lab = _labels(n, rng, first)
        labels = torch.from_numpy(lab).to(gpu_device)
        ref = event_refs.events(scores, thr, labels=lab, merge_gap=1, compare_f32=f32)
        got = ev.anomaly_events(s, thr, labels=labels, merge_gap=1, compare_f32=f32)
        assert got["event_is_true"].dtype == torch.bool and np.array_equal(got["event_is_true"].cpu().numpy(), ref["event_is_true"])
        for key in ("start", "end", "first_hit", "latency"):
            assert got["segments"][key].dtype == torch.int64
            assert np.array_equal(got["segments"][key].cpu().numpy(), ref["segments"][key]), (n, thr, key)
        if first:
            continue                         # point adjust treats a segment that starts at index 0 specially (its back-fill stops at 1)
        seg = ev.anomaly_events(s, thr, labels=labels.float(), compare_f32=f32)["segments"]       # merge_gap=0, min_length=1; float labels
        counts = ev.point_adjust_counts(s, labels, [thr], compare_f32=f32)[0]
        detected = seg["first_hit"] >= 0
        assert int(detected.sum()) == counts[5], (n, thr)
        assert int(seg["latency"][detected].sum()) == counts[4], (n, thr)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(gpu_device):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(21)
    model = MTAD_GAT(n_features=3, window_size=8, out_dim=3, kernel_size=3, gru_hid_dim=16, forecast_hid_dim=16,
                     recon_hid_dim=16).to(gpu_device).eval()
    g = torch.Generator().manual_seed(22)
    train = torch.rand(200, 3, generator=g)
    test = torch.rand(200, 3, generator=g)
    labels = torch.zeros(192, dtype=torch.bool)
    for lo, hi in ((40, 52), (120, 126), (170, 173)):
        labels[lo:hi] = True
        test[8 + lo:8 + hi] += 2.0              # what the model cannot forecast: high scores inside the labelled segments
    return model, train.to(gpu_device), test.to(gpu_device), labels.to(gpu_device)


def test_predict_anomalies_events(tiny, gpu_device):
    model, train, test, labels = tiny
    opts = dict(merge_gap=2, min_length=2, top_k=2)
    with torch.no_grad():
        out = ev.predict_anomalies(model, train, test, labels=labels, events=opts)
        plain = ev.predict_anomalies(model, train, test, labels=labels)
        again = ev.predict_anomalies(model, train, test, labels=labels)
    events = out["events"]
    assert events["count"] >= 1 and events["threshold"] == out["epsilon_result"]["threshold"]
    by_hand = ev.anomaly_events(out["test_scores"], events["threshold"], per_dim=out["test_per_dim"], feature_thresholds=out["feature_thresholds"],
                                labels=labels, **opts)
    _same_bits(events, by_hand)
    ref = event_refs.events(out["test_scores"].cpu().numpy(), events["threshold"], out["test_per_dim"].cpu().numpy(), out["feature_thresholds"],
                            labels.cpu().numpy(), **opts)
    assert np.array_equal(events["start"].cpu().numpy(), ref["start"]) and np.array_equal(events["peak"].cpu().numpy(), ref["peak"])
    assert np.array_equal(events["feature_hits"].cpu().numpy(), ref["feature_hits"])
    assert bool(events["event_is_true"].any())
    # the default: the keys and tensors of before
    assert set(plain) == set(again) == set(out) - {"events"}
    assert set(plain) == {"epsilon_result", "bf_result", "feature_thresholds", "train_scores", "test_scores", "test_per_dim", "feature_preds"}
    for key in plain:
        if isinstance(plain[key], torch.Tensor):
            assert torch.equal(plain[key].view(torch.uint8), again[key].view(torch.uint8)), key
            assert torch.equal(plain[key].view(torch.uint8), out[key].view(torch.uint8)), key
    # without labels the threshold is find_epsilon's and the label columns are absent
    with torch.no_grad():
        bare = ev.predict_anomalies(model, train, test, events={})["events"]
    assert "segments" not in bare and "event_is_true" not in bare and bare["count"] >= 1
    with pytest.raises(ValueError):
        ev.predict_anomalies(model, train, test, events={"gap": 1})


def test_explain_events(tiny, gpu_device):
    model, train, test, labels = tiny
    with torch.no_grad():
        scores, per_dim = model.anomaly_scores(test)
    events = ev.anomaly_events(scores, float(scores.median()), per_dim=per_dim, merge_gap=1)
    assert 3 <= events["count"] <= 64
    got = ev.explain_events(model, test, events)
    ref = model.score_attribution(test, events["peak"])
    assert got["attributions"].shape == (events["count"], 9, 3) and torch.equal(got["attributions"], ref)
    assert torch.equal(got["peaks"], events["peak"])
    assert torch.equal(got["per_feature"], ref.abs().sum(1)) and torch.equal(got["per_lag"], ref.abs().sum(2))
    some = ev.explain_events(model, test, events, which=[2, 0], method="integrated", steps=4)
    assert torch.equal(some["attributions"], model.score_attribution(test, events["peak"][[2, 0]], method="integrated", steps=4))
    with pytest.raises(ValueError, match="max_events"):
        ev.explain_events(model, test, events, max_events=2)
