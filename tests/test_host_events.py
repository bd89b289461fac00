"""The event entry points (csrc/mtadgat_events.hip: runs, run statistics, first hits) without a GPU: symbols, argument
validation before anything touches the device, scratch sizes, the Python wrappers' refusal of CPU tensors; and the numpy
reference the GPU tests compare against (tests/event_refs.py), held against a hand-worked case and the CPU oracle."""
import ctypes

import numpy as np
import pytest
import torch

import event_refs
from oracle import eval_oracle as eo

PTR = 0x10000            # a non-null, 16-byte aligned "device pointer": validation fails before it would be used
TOO_LONG = 1 << 31


@pytest.fixture(scope="module")
def lib():
    import evaluation
    return evaluation._lib()


def _err(lib):
    return lib.mtadgat_last_error().decode()


def test_symbols_are_exported(lib):
    import evaluation
    for name in ("mtadgat_eval_runs", "mtadgat_eval_runs_scratch", "mtadgat_eval_runs_chunk", "mtadgat_eval_run_stats",
                 "mtadgat_eval_run_stats_scratch", "mtadgat_eval_first_hit"):
        assert hasattr(lib, name), name
    for name in ("flag_runs", "run_statistics", "first_hits", "anomaly_events", "explain_events"):
        assert callable(getattr(evaluation, name)), name
    assert lib.mtadgat_eval_runs_chunk() == evaluation.RUNS_CHUNK >= 64


def _runs(lib, score=PTR, label=None, n=1000, gap=0, min_length=1, max_runs=16, scratch=PTR, scratch_bytes=None, start=PTR, end=PTR,
          count=True):
    if scratch_bytes is None:
        scratch_bytes = lib.mtadgat_eval_runs_scratch(1000)
    c = ctypes.c_int64(-7)
    return lib.mtadgat_eval_runs(score, label, n, 0.5, 0, gap, min_length, max_runs, scratch, scratch_bytes, start, end,
                                 ctypes.byref(c) if count else None, None)


RUNS_BAD = {
    "null source": dict(score=None), "both sources": dict(label=PTR), "null scratch": dict(scratch=None), "null start": dict(start=None),
    "null end": dict(end=None), "null count": dict(count=False), "n < 1": dict(n=0), "n >= 2^31": dict(n=TOO_LONG),
    "merge_gap < 0": dict(gap=-1), "min_length < 1": dict(min_length=0), "max_runs < 1": dict(max_runs=0),
    "scratch one byte short": dict(scratch_bytes=-1), "misaligned scratch": dict(scratch=PTR + 4),
}


@pytest.mark.parametrize("case", list(RUNS_BAD))
def test_runs_rejects_invalid_arguments(lib, case):
    kw = dict(RUNS_BAD[case])
    if kw.get("scratch_bytes") == -1:
        kw["scratch_bytes"] = lib.mtadgat_eval_runs_scratch(1000) - 1
    assert _runs(lib, **kw) in (-1, -5)
    assert "runs:" in _err(lib)
    if "source" not in case:                          # the same with labels as the flag source
        assert _runs(lib, **dict(kw, score=None, label=PTR)) in (-1, -5)
        assert "runs:" in _err(lib)


def _stats(lib, score=PTR, n=1000, start=PTR, end=PTR, count=5, per_dim=PTR, d=4, ld=4, thr=PTR, top_k=2, scratch=PTR, scratch_bytes=None,
           peak=PTR, peak_score=PTR, mean=PTR, fmeans=PTR, tidx=PTR, tval=PTR, hits=PTR):
    if scratch_bytes is None:
        scratch_bytes = lib.mtadgat_eval_run_stats_scratch(1000, 5, 130)
    return lib.mtadgat_eval_run_stats(score, n, start, end, count, per_dim, d, ld, thr, top_k, scratch, scratch_bytes, peak, peak_score, mean,
                                      fmeans, tidx, tval, hits, None)


STATS_BAD = {
    "null score": dict(score=None), "null start": dict(start=None), "null end": dict(end=None), "null scratch": dict(scratch=None),
    "null peak": dict(peak=None), "null peak_score": dict(peak_score=None), "null mean_score": dict(mean=None),
    "null feature_means": dict(fmeans=None), "null top_idx": dict(tidx=None), "null top_val": dict(tval=None),
    "null feature_hits": dict(hits=None), "thresholds without per_dim": dict(per_dim=None),
    "n < 1": dict(n=0), "n >= 2^31": dict(n=TOO_LONG), "count < 0": dict(count=-1), "d < 1": dict(d=0), "d > 2048": dict(d=2049, ld=2049),
    "ld < d": dict(ld=3), "top_k < 1": dict(top_k=0), "top_k > d": dict(top_k=5), "top_k > 64": dict(d=130, ld=130, top_k=65),
    "scratch one byte short": dict(scratch_bytes=-1), "misaligned scratch": dict(scratch=PTR + 4),
}


@pytest.mark.parametrize("case", list(STATS_BAD))
def test_run_stats_rejects_invalid_arguments(lib, case):
    kw = dict(STATS_BAD[case])
    if kw.get("scratch_bytes") == -1:
        kw["scratch_bytes"] = lib.mtadgat_eval_run_stats_scratch(1000, 5, 4) - 1
    assert _stats(lib, **kw) in (-1, -5)
    assert "run_stats:" in _err(lib)


FIRST_BAD = {"null source": dict(score=None), "both sources": dict(label=PTR), "null start": dict(start=None), "null end": dict(end=None),
             "null first": dict(first=None), "n < 1": dict(n=0), "n >= 2^31": dict(n=TOO_LONG), "count < 0": dict(count=-1)}


@pytest.mark.parametrize("case", list(FIRST_BAD))
def test_first_hit_rejects_invalid_arguments(lib, case):
    kw = dict(score=PTR, label=None, n=1000, start=PTR, end=PTR, count=5, first=PTR)
    kw.update(FIRST_BAD[case])
    assert lib.mtadgat_eval_first_hit(kw["score"], kw["label"], kw["n"], 0.5, 0, kw["start"], kw["end"], kw["count"], kw["first"], None) == -1
    assert "first_hit:" in _err(lib)


def test_scratch_queries(lib):
    rs, ss = lib.mtadgat_eval_runs_scratch, lib.mtadgat_eval_run_stats_scratch
    for n in (0, -1, TOO_LONG):
        assert rs(n) == 0 and ss(n, 5, 4) == 0
    assert ss(1000, -1, 4) == 0 and ss(1000, 5, -1) == 0 and ss(1000, 5, 2049) == 0
    assert rs(1) > 0 and ss(1, 0, 0) > 0
    ns = [1, 2, 1023, 1024, 1025, 70001, 1 << 22, TOO_LONG - 1]
    for a, b in zip(ns, ns[1:]):
        assert rs(a) <= rs(b) and ss(a, 5, 4) <= ss(b, 5, 4)
    assert rs(1 << 22) > rs(1024)
    assert ss(1 << 22, 5, 38) > ss(1 << 22, 5, 1) > ss(1 << 22, 5, 0)
    assert ss(1000, 5000, 4) > ss(1000, 5, 4)
    assert all(v % 8 == 0 for v in (rs(70001), ss(70001, 33, 3)))


def test_python_wrappers_refuse_cpu_tensors():
    import evaluation as ev
    s, idx = torch.rand(20), torch.zeros(1, dtype=torch.int64)
    calls = [lambda: ev.flag_runs(scores=s, threshold=0.5), lambda: ev.flag_runs(labels=s > 0.5),
             lambda: ev.run_statistics(s, idx, idx + 1), lambda: ev.first_hits(idx, idx + 1, scores=s, threshold=0.5),
             lambda: ev.first_hits(idx, idx + 1, labels=s > 0.5), lambda: ev.anomaly_events(s, 0.5),
             lambda: ev.anomaly_events(s, 0.5, labels=s > 0.5)]
    for call in calls:
        with pytest.raises(RuntimeError, match="on the GPU"):
            call()


HAND = [0, 2, 2, 0, 0, 3, 0, 0, 0, 5, 0, 1]
HAND_CASES = [(0, 1, [(1, 3), (5, 6), (9, 10)], [1, 5, 9]), (1, 1, [(1, 3), (5, 6), (9, 10)], [1, 5, 9]), (2, 1, [(1, 6), (9, 10)], [5, 9]),
              (3, 1, [(1, 10)], [9]), (0, 2, [(1, 3)], None), (2, 4, [(1, 6)], None)]


@pytest.mark.parametrize("gap,min_length,expected,peaks", HAND_CASES)
def test_reference_on_the_hand_worked_case(gap, min_length, expected, peaks):
    score = np.asarray(HAND, np.float32)
    start, end = event_refs.runs(event_refs.flags(score, 1.0), gap, min_length)
    assert list(zip(start.tolist(), end.tolist())) == expected
    st = event_refs.stats(score, start, end)
    if peaks is not None:
        assert st["peak"].tolist() == peaks
    assert st["peak_score"].tolist() == [float(score[p]) for p in st["peak"]]
    assert st["mean_score"].tolist() == [float(np.float64(sum(HAND[a:b])) / (b - a)) for a, b in expected]


def test_reference_statistics_by_hand():
    score = np.asarray([1, np.nan, 4, 4, -np.inf], np.float32)
    per_dim = np.asarray([[1, 5, 0], [3, 5, np.nan], [2, 5, 1], [0, -0.0, 0.0], [9, 9, 9]], np.float32)
    start, end = np.asarray([0, 3]), np.asarray([3, 5])
    st = event_refs.stats(score, start, end, per_dim, thresholds=[2.0, 5.0, 0.5], top_k=2)
    assert st["peak"].tolist() == [2, 3] and st["peak_score"].tolist() == [4.0, 4.0]
    assert np.isnan(st["mean_score"][0]) and st["mean_score"][1] == -np.inf
    assert st["feature_means"][0, :2].tolist() == [2.0, 5.0] and np.isnan(st["feature_means"][0, 2])
    assert st["top_features"].tolist() == [[1, 0], [0, 1]]           # NaN last; 4.5, 4.5, 4.5: ties to the lower column
    assert st["top_values"].tolist() == [[5.0, 2.0], [4.5, 4.5]]
    assert st["feature_hits"].tolist() == [[2, 3, 1], [1, 1, 1]]
    assert event_refs.first_hit(score > 3, start, end).tolist() == [2, 3]
    assert event_refs.first_hit(score > 3, [0, 4], [2, 5]).tolist() == [-1, -1]
    assert event_refs.flags(np.float32(0.1), 0.1).tolist() is True and event_refs.flags(np.float32(0.1), 0.1, True).tolist() is False


def _labels(n, rng):
    lab = np.convolve(rng.random(n + 8), np.ones(9) / 9.0, mode="valid")[:n] > 0.56
    lab[0] = False                       # the reference's back-fill never reaches index 0 (oracle.eval_oracle.point_adjust)
    return lab


@pytest.mark.parametrize("n", [1, 2, 3, 17, 100, 1000, 5000])
def test_reference_segment_table_reproduces_point_adjust(n):
    rng = np.random.default_rng(n)
    for trial in range(20 if n <= 100 else 4):
        score = rng.random(n).astype(np.float32)
        lab = _labels(n, rng)
        thr = float(rng.choice([0.5, 0.9, 0.97, 2.0]))
        for f32 in (False, True):
            ref = event_refs.events(score, thr, labels=lab, compare_f32=f32)
            seg = ref["segments"]
            assert list(zip(seg["start"].tolist(), (seg["end"] - 1).tolist())) == [(int(a), int(b)) for a, b in eo.segments(lab)]
            predict, latency = eo.point_adjust(score, lab, thr, compare_f32=f32)
            mine = event_refs.flags(score, thr, f32).copy()
            detected = seg["first_hit"] >= 0
            for a, b in zip(seg["start"][detected], seg["end"][detected]):
                mine[a:b] = True
            assert np.array_equal(mine, predict), (n, trial)
            assert np.array_equal(seg["latency"][detected], (seg["first_hit"] - seg["start"])[detected]) and np.all(seg["latency"][~detected] == -1)
            assert seg["latency"][detected].sum() / (detected.sum() + 1e-4) == latency, (n, trial)
            # an event is true exactly when one of its samples is labelled
            assert ref["event_is_true"].tolist() == [bool(lab[a:b].any()) for a, b in zip(ref["start"], ref["end"])]
