"""The ranking curves without a GPU: the numpy specification tests/curve_refs.py (what tests/test_gpu_curves.py compares the kernels of
csrc/mtadgat_curves.hip against) held against scikit-learn, the CPU oracle's point adjust and a direct per-threshold PA%K loop; the
host-callable order key; argument validation before anything touches the device.

Gates
  AUROC and average precision against scikit-learn: 1e-12 absolute -- both sides are float64 evaluations of the same rational numbers.
  Adjusted curves: every (tp, fp) exact at every distinct threshold."""
import ctypes

import numpy as np
import pytest
import torch

import curve_refs
from oracle import eval_oracle as eo

PTR = 0x10000            # a non-null, aligned "device pointer": validation fails before it would be used
TOO_LONG = 1 << 31
N_CASES = 200


@pytest.fixture(scope="module")
def lib():
    import evaluation
    return evaluation._lib()


def _case(seed):
    """(scores, labels) of n <= 400 with ties, -0.0 and, in every third case, a segment at index 0; None when a class is empty."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 401))
    levels = int(rng.choice([3, 17, 1000]))
    s = (rng.integers(0, levels, n) / np.float32(levels) - np.float32(0.3)).astype(np.float32)
    s[rng.integers(0, n, 3)] = np.float32(-0.0)
    s[rng.integers(0, n, 2)] = np.float32(0.0)
    lab = np.convolve(rng.random(n + 6), np.ones(7) / 7.0, mode="valid")[:n] > 0.55
    s[lab] += np.float32(0.25) * (rng.random(int(lab.sum())) < 0.5)
    if seed % 3 == 0:
        lab[:int(rng.integers(1, 6))] = True
    if seed % 5 == 0:
        lab[n - 1] = True
    if lab.all():
        lab[n // 2] = False
    if not lab.any():
        lab[n // 2] = True
    if lab.all() or not lab.any():
        return None
    return s, lab


def _cases():
    made = [_case(seed) for seed in range(N_CASES)]
    kept = [c for c in made if c is not None]
    assert len(made) - len(kept) <= 0.05 * len(made)
    assert sum(1 for s, lab in kept if lab[0]) >= len(kept) // 4
    return kept


CASES = _cases()


def test_reference_against_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    for s, lab in CASES:
        assert np.unique(s).size < s.size or s.size < 4          # tied data
        ref = curve_refs.ranking_metrics(s, lab)
        assert abs(ref["auroc"] - metrics.roc_auc_score(lab, s)) <= 1e-12
        assert abs(ref["average_precision"] - metrics.average_precision_score(lab, s)) <= 1e-12


def test_reference_curve_by_hand():
    s = np.asarray([0.5, np.nan, -0.0, 0.5, 0.0, 2.0, np.nan, -np.inf], np.float32)
    lab = np.asarray([1, 1, 0, 0, 1, 0, 0, 1], bool)
    c = curve_refs.ranking_curve(s, lab)
    assert c["thresholds"].tolist() == [2.0, 0.5, 0.0, -np.inf] and not np.signbit(c["thresholds"][2])
    assert c["tp"].tolist() == [0, 1, 2, 3] and c["fp"].tolist() == [1, 2, 3, 3]
    assert (c["n_pos"], c["n_neg"], c["nan_pos"], c["nan_neg"]) == (4, 4, 1, 1)
    m = curve_refs.ranking_metrics(s, lab)
    # groups (tp_g, fp_g): (0, 1), (1, 1), (1, 1), (1, 0), NaN (1, 1): 2 x numerator = 0 + 1 x 5 + 1 x 3 + 1 x 2 + 1 x 1
    assert m["auroc"] == 11 / 32
    assert m["average_precision"] == (1 / 3 + 2 / 5 + 3 / 6) / 4
    assert curve_refs.score_order(s).tolist() == [5, 0, 3, 2, 4, 7, 1, 6]
    assert curve_refs.score_order(s, descending=False).tolist() == [7, 2, 4, 0, 3, 5, 1, 6]
    # point: segment [0, 2) starts at index 0 -- sample 0 keeps its own score, the NaN takes the maximum; [4, 5); [7, 8)
    assert np.array_equal(curve_refs.adjusted_scores(s, lab, "point"), np.asarray([0.5, 0.5, -0.0, 0.5, 0.0, 2.0, np.nan, -np.inf], np.float32),
                          equal_nan=True)
    all_nan = np.asarray([np.nan, np.nan], np.float32)
    m = curve_refs.ranking_metrics(all_nan, np.asarray([1, 0], bool))
    assert m["best"] is None and m["n_thresholds"] == 0 and m["auroc"] == 0.5


def test_reference_point_adjust_against_the_oracle():
    for s, lab in CASES:
        c = curve_refs.ranking_curve(s, lab, "point")
        assert c["thresholds"].size >= 1 and np.all(np.diff(c["thresholds"]) < 0)
        for v, tp, fp in zip(c["thresholds"], c["tp"], c["fp"]):
            below = np.nextafter(np.float32(v), np.float32(-np.inf))
            predict, _ = eo.point_adjust(s, lab, below, compare_f32=True)
            assert int(np.sum(predict & lab)) == tp and int(np.sum(predict & ~lab)) == fp


def _pak_flags(s, lab, v, K):
    """PA%K at "flagged = score >= v", straight from the definition: a segment with more than K % of its samples flagged is flagged whole."""
    flag = s >= v
    out = flag.copy()
    for a, b in zip(*curve_refs.segments(lab)):
        if 100 * int(flag[a:b].sum()) > K * int(b - a):
            out[a:b] = True
    return out


@pytest.mark.parametrize("K", [0, 20, 50, 100])
def test_reference_pa_k_against_the_definition(K):
    for s, lab in CASES:
        s = s.copy()
        s[3 % s.size] = np.nan                                   # a NaN is never flagged by itself
        c = curve_refs.ranking_curve(s, lab, ("k", K))
        values = np.unique(np.concatenate((s[~np.isnan(s)], c["thresholds"])))
        at = {float(v): (int(tp), int(fp)) for v, tp, fp in zip(c["thresholds"], c["tp"], c["fp"])}
        last = (0, 0)
        for v in values[::-1]:
            flag = _pak_flags(s, lab, v, K)
            got = (int(np.sum(flag & lab)), int(np.sum(flag & ~lab)))
            last = at.get(float(v), last)                        # between two thresholds of the curve nothing changes
            assert got == last, (K, v)


def test_order_key(lib):
    import evaluation  # noqa: F401  (binds the argument types)
    key = lib.mtadgat_eval_order_key
    tiny, big = np.float32(1e-45), np.finfo(np.float32).max
    values = [-np.inf, -big, np.nextafter(-big, np.float32(0)), -1.5, -1.0, np.nextafter(np.float32(-1), np.float32(0)),
              -np.finfo(np.float32).tiny, -2 * tiny, -tiny, 0.0, tiny, 2 * tiny, np.finfo(np.float32).tiny, 0.5, 1.0,
              np.nextafter(np.float32(1), np.float32(2)), big, np.inf]
    values = [float(np.float32(v)) for v in values]
    assert values == sorted(values) and len(set(values)) == len(values)
    up = [key(v, 0) for v in values]
    down = [key(v, 1) for v in values]
    assert all(a < b for a, b in zip(up, up[1:])) and all(a > b for a, b in zip(down, down[1:]))
    assert up == curve_refs.order_key(values, False).tolist() and down == curve_refs.order_key(values, True).tolist()
    for d in (0, 1):
        assert key(-0.0, d) == key(0.0, d)
        for bits in (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF):
            nan = float(np.array([bits], np.uint32).view(np.float32)[0])
            assert np.isnan(nan) and key(nan, d) == 0xFFFFFFFF
        assert max(key(v, d) for v in values) < 0xFFFFFFFF
    rng = np.random.default_rng(0)
    x = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    for d in (0, 1):
        assert [key(float(v), d) for v in x] == curve_refs.order_key(x, bool(d)).tolist()


def test_symbols_and_sizes(lib):
    import evaluation
    for name in ("mtadgat_eval_order_key", "mtadgat_eval_sort_tile", "mtadgat_eval_sort_scan_tiles", "mtadgat_eval_score_order",
                 "mtadgat_eval_score_order_scratch", "mtadgat_eval_curve", "mtadgat_eval_curve_scratch"):
        assert hasattr(lib, name), name
    for name in ("score_order", "ranking_curve", "ranking_metrics"):
        assert callable(getattr(evaluation, name)), name
    assert lib.mtadgat_eval_sort_tile() >= 256 and lib.mtadgat_eval_sort_tile() % 256 == 0
    assert lib.mtadgat_eval_sort_scan_tiles() >= 1
    so, cu = lib.mtadgat_eval_score_order_scratch, lib.mtadgat_eval_curve_scratch
    for n in (0, -1, TOO_LONG):
        assert so(n) == 0 and cu(n, 0) == 0
    assert cu(1000, -1) == 0 and cu(1000, 3) == 0
    tile = lib.mtadgat_eval_sort_tile()
    ns = [1, 2, tile - 1, tile, tile + 1, 70001, 1 << 22, TOO_LONG - 1]
    for a, b in zip(ns, ns[1:]):
        assert 0 < so(a) <= so(b) and 0 < cu(a, 0) <= cu(b, 0) and cu(a, 2) <= cu(b, 2)
    for n in ns:
        assert so(n) >= 24 * n and so(n) <= cu(n, 0) < cu(n, 1) == cu(n, 2)
        assert so(n) % 8 == 0 and cu(n, 1) % 8 == 0


def _order(lib, score=PTR, n=1000, scratch=PTR, scratch_bytes=None, order=PTR):
    if scratch_bytes is None:
        scratch_bytes = lib.mtadgat_eval_score_order_scratch(1000)
    return lib.mtadgat_eval_score_order(score, n, 1, scratch, scratch_bytes, order, None)


ORDER_BAD = {"null score": dict(score=None), "null scratch": dict(scratch=None), "null order": dict(order=None), "n < 1": dict(n=0),
             "n >= 2^31": dict(n=TOO_LONG), "scratch one byte short": dict(scratch_bytes=-1), "misaligned scratch": dict(scratch=PTR + 4)}


@pytest.mark.parametrize("case", list(ORDER_BAD))
def test_score_order_rejects_invalid_arguments(lib, case):
    kw = dict(ORDER_BAD[case])
    if kw.get("scratch_bytes") == -1:
        kw["scratch_bytes"] = lib.mtadgat_eval_score_order_scratch(1000) - 1
    assert _order(lib, **kw) in (-1, -5)
    assert "score_order:" in lib.mtadgat_last_error().decode()


def _curve(lib, score=PTR, label=PTR, n=1000, adjust=2, k=30, scratch=PTR, scratch_bytes=None, thr=PTR, tp=PTR, fp=PTR, summary=True):
    if scratch_bytes is None:
        scratch_bytes = lib.mtadgat_eval_curve_scratch(1000, 2)
    out = (ctypes.c_int64 * 12)()
    return lib.mtadgat_eval_curve(score, label, n, adjust, k, scratch, scratch_bytes, thr, tp, fp, out if summary else None, None)


CURVE_BAD = {"null score": dict(score=None), "null label": dict(label=None), "null scratch": dict(scratch=None), "null thresholds": dict(thr=None),
             "null tp": dict(tp=None), "null fp": dict(fp=None), "null summary": dict(summary=False), "n < 1": dict(n=0),
             "n >= 2^31": dict(n=TOO_LONG), "adjust < 0": dict(adjust=-1), "adjust > 2": dict(adjust=3), "K < 0": dict(k=-1), "K > 100": dict(k=101),
             "scratch one byte short": dict(scratch_bytes=-1), "misaligned scratch": dict(scratch=PTR + 4)}


@pytest.mark.parametrize("case", list(CURVE_BAD))
def test_curve_rejects_invalid_arguments(lib, case):
    kw = dict(CURVE_BAD[case])
    if kw.get("scratch_bytes") == -1:
        kw["scratch_bytes"] = lib.mtadgat_eval_curve_scratch(1000, 2) - 1
    assert _curve(lib, **kw) in (-1, -5)
    assert "curve:" in lib.mtadgat_last_error().decode()


def test_python_wrappers_check_their_arguments():
    import evaluation as ev
    s = torch.rand(20)
    for call in (lambda: ev.score_order(s), lambda: ev.ranking_curve(s, s > 0.5), lambda: ev.ranking_metrics(s, s > 0.5, "point")):
        with pytest.raises(RuntimeError, match="on the GPU"):
            call()
    for bad in ("points", ("k",), ("k", 101), ("k", -1), ("k", 2.5), ("k", True), ("j", 3), 7):
        with pytest.raises(ValueError):
            ev._adjust_code(bad)
    assert ev._adjust_code(None) == (0, 0) and ev._adjust_code("point") == (1, 0) and ev._adjust_code(("k", 0)) == (2, 0)
    assert ev._adjust_code(("k", np.int64(100))) == (2, 100) and ev._adjust_code(["k", 30]) == (2, 30)
