"""The host side of the part-aware score passes: evaluation.score_parts' spans and seams against a brute-force labelling of every
score by the part of its target row (tests/part_refs.py), the argument validation, and what needs no GPU of the public calls."""
import numpy as np
import pytest
import torch

import part_refs


def _random_lengths(rng, P, W):
    kind = rng.integers(0, 4)
    if kind == 0:
        ls = rng.integers(0, 3 * W + 2, size=P)                  # zeros and parts shorter than the window
    elif kind == 1:
        ls = rng.integers(0, 2, size=P) * rng.integers(1, 50, size=P)
    elif kind == 2:
        ls = np.ones(P, dtype=np.int64)
    else:
        ls = rng.integers(1, 400, size=P)
    ls = ls.astype(np.int64)
    if ls.sum() <= W:
        ls[rng.integers(0, P)] += W + 1 - ls.sum() + rng.integers(0, 5)
    return ls.tolist()


def _check_spans(lengths, W):
    import evaluation as ev
    sp = ev.score_parts(lengths, W)
    n = sum(lengths) - W
    labels = part_refs.part_labels(lengths, W)
    assert sp.n == n == labels.size and sp.n_parts == len(lengths)
    start, end = sp.start_host, sp.end_host
    assert start.dtype == np.int64 and end.dtype == np.int64
    assert start[0] == 0 and end[-1] == n and np.all(start <= end) and np.all(end[:-1] == start[1:])      # disjoint, ascending, covering
    mine = np.full(n, -1, dtype=np.int64)
    for p in range(len(lengths)):
        assert np.all(mine[start[p]:end[p]] == -1)
        mine[start[p]:end[p]] = p
    assert np.array_equal(mine, labels)
    assert np.array_equal(sp.part_of(np.arange(n)), labels)
    assert sp.part_of(0) == labels[0] and sp.part_of(n - 1) == labels[-1] and isinstance(sp.part_of(0), int)
    # a seam is the first score of a new part, counted once per seam of the series that falls among the scores
    assert sp.seams_host.tolist() == part_refs.seams(lengths, W)
    assert torch.equal(sp.start, torch.from_numpy(start)) and torch.equal(sp.end, torch.from_numpy(end))
    assert (sp.seams is None) == (len(part_refs.seams(lengths, W)) == 0)
    return sp


def test_spans_equal_a_brute_force_labelling():
    rng = np.random.default_rng(0)
    for trial in range(200):
        W = int(rng.choice([1, 2, 10, 100]))
        P = int(rng.choice([1, 2, 3, 7, 40]))
        _check_spans(_random_lengths(rng, P, W), W)
    _check_spans([50], 10)                                       # P = 1
    _check_spans([1] * 64, 1)                                    # all ones
    _check_spans([1] * 64, 10)
    _check_spans([0, 0, 5, 0, 3, 0], 4)
    _check_spans([3, 3, 3, 30], 10)                              # three parts end inside the first window: empty spans, no seam
    for n in (1, 65, 1025):
        for W in (1, 100):
            for lengths in part_refs.layouts(n, W).values():
                _check_spans(lengths, W)


def test_part_of_rejects_indices_outside_the_scores():
    import evaluation as ev
    sp = ev.score_parts([20, 30], 10)
    assert sp.n == 40 and sp.part_of([9, 10]).tolist() == [0, 1]
    for bad in (-1, 40, [0, 40]):
        with pytest.raises(IndexError):
            sp.part_of(bad)


def test_transition_defaults_to_the_reference_buffer():
    import evaluation as ev
    assert ev.score_parts([20, 30], 10).transition == (19, 19)
    assert ev.score_parts([20, 30], 10, transition=(3, 9)).transition == (3, 9)


@pytest.mark.parametrize("bad", [dict(lengths=[5, -1, 30], window_size=10), dict(lengths=[5, 5], window_size=10),
                                 dict(lengths=[5, 4], window_size=10), dict(lengths=[], window_size=10),
                                 dict(lengths=[20.5, 30], window_size=10), dict(lengths=[20, 30], window_size=0),
                                 dict(lengths=[20, 30], window_size=10, transition=(-1, 3)),
                                 dict(lengths=[20, 30], window_size=10, transition=(3, -1)),
                                 dict(lengths=[20, 30], window_size=10, transition=(3,))])
def test_score_parts_validates_its_arguments(bad):
    import evaluation as ev
    with pytest.raises(ValueError):
        ev.score_parts(**bad)


def test_predict_anomalies_rejects_unknown_part_keys_before_touching_the_model():
    import evaluation as ev
    with pytest.raises(ValueError, match="bogus"):
        ev.predict_anomalies(None, None, None, parts={"bogus": 1})
    with pytest.raises(ValueError, match="thresholds"):
        ev.predict_anomalies(None, None, None, parts={"thresholds": "each"})


def test_cpu_tensors_are_refused():
    import evaluation as ev
    sp = ev.score_parts([20, 30], 10)
    x = torch.rand(40)
    for call in (lambda: ev.adjust_part_scores(x, sp), lambda: ev.adjust_part_scores(torch.rand(40, 3), sp),
                 lambda: ev.moving_average(x, 5, parts=sp), lambda: ev.find_epsilon_parts(x, sp),
                 lambda: ev.part_predictions(x, sp, [0.5, 0.5])):
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_scratch_queries_return_zero_for_invalid_sizes():
    import evaluation as ev
    lib = ev._lib()
    assert lib.mtadgat_eval_part_adjust_scratch(1000, 3, 7) > 0
    assert lib.mtadgat_eval_ewm_parts_scratch(1000) > 0
    assert lib.mtadgat_eval_part_epsilon_scratch(1000, 7, 19) > 0
    for n, d, count in ((0, 1, 1), (2 ** 31, 1, 1), (10, 0, 1), (10, 2049, 1), (10, 1, 0)):
        assert lib.mtadgat_eval_part_adjust_scratch(n, d, count) == 0
    assert lib.mtadgat_eval_ewm_parts_scratch(0) == 0 and lib.mtadgat_eval_ewm_parts_scratch(2 ** 31) == 0
    for n, count, nz in ((0, 1, 19), (10, 0, 19), (10, 1, 0), (10, 1, 65)):
        assert lib.mtadgat_eval_part_epsilon_scratch(n, count, nz) == 0


def test_entry_points_validate_before_they_launch():
    """Status -1 with a message for arguments the host can judge; the pointers are never followed, so this needs no GPU."""
    import evaluation as ev
    lib = ev._lib()
    p = 4096                                                     # stands for a device pointer
    assert lib.mtadgat_eval_part_adjust(p, 10, 1, 1, p, p, 1, None, 0, -1, 0, 0, None, 0, p, 1, None, None) == -1
    assert b"before" in lib.mtadgat_last_error()
    assert lib.mtadgat_eval_part_adjust(p, 10, 3, 2, p, p, 1, None, 0, 0, 0, 0, None, 0, p, 3, None, None) == -1
    assert lib.mtadgat_eval_part_adjust(p, 10, 1, 1, p, p, 1, None, 2, 0, 0, 0, None, 0, p, 1, None, None) == -1      # seams without an array
    assert lib.mtadgat_eval_part_adjust(p, 10, 1, 1, p, p, 1, None, 0, 0, 0, 1, p, 8, p, 1, None, None) == -5        # scratch too small
    assert lib.mtadgat_eval_ewm_parts(p, 10, p, p, 1, 1.5, p, 1 << 20, p, None) == -1
    assert lib.mtadgat_eval_ewm_parts(p, 10, p, p, 0, 0.5, p, 1 << 20, p, None) == -1
    assert lib.mtadgat_eval_ewm_parts(p, 10, p, p, 1, 0.5, p, 8, p, None) == -5
    out = (ev.ctypes.c_double * 512)()
    assert lib.mtadgat_eval_part_epsilon_moments(p, 0, p, p, 1, 19, p, 1 << 20, out, None) == -1
    assert lib.mtadgat_eval_part_epsilon_table(p, 10, p, p, 1, out, 19, 129, p, 1 << 20, out, None) == -1
    assert b"halo" in lib.mtadgat_last_error()
    assert lib.mtadgat_eval_part_epsilon_table(p, 10, p, p, 1, out, 19, 49, p, 8, out, None) == -5
    assert lib.mtadgat_eval_part_flags(p, 10, p, p, 1, None, p, None) == -1


def test_use_tensors_hands_on_the_callers_own_span_arrays():
    """ScoreParts.use_tensors registers the caller's tensors for their device -- tensors() then returns those very tensors -- and
    refuses wrong types, lengths and layouts."""
    import evaluation as ev
    sp = ev.score_parts([9, 1, 0, 65, 3], 7)
    start, end, seams = (torch.from_numpy(a.copy()) for a in (sp.start_host, sp.end_host, sp.seams_host))
    assert sp.use_tensors(start, end, seams) is sp
    got = sp.tensors("cpu")
    assert got[0] is start and got[1] is end and got[2] is seams
    for bad in ((start.int(), end, seams), (start[:-1], end, seams), (start, end, seams[:-1]), (start, end, None),
                (start, torch.stack([end, end], 1)[:, 0], seams), (start.tolist(), end, seams)):
        with pytest.raises((ValueError, AttributeError)):
            sp.use_tensors(*bad)
    one = ev.score_parts([30], 7)                                       # no seam: None or an empty tensor, handed on as None
    s1, e1 = torch.from_numpy(one.start_host.copy()), torch.from_numpy(one.end_host.copy())
    assert one.use_tensors(s1, e1).tensors("cpu") == (s1, e1, None)
    assert one.use_tensors(s1, e1, torch.zeros(0, dtype=torch.int64)).tensors("cpu")[2] is None
