"""The threshold-evaluation entry points of csrc/mtadgat_eval.hip without a GPU: the float64 specification the GPU tests
compare against (tests/eval_refs.py) held against the oracle, the rules of evaluation._choose_epsilon on hand-written tables, the
gates of eval_refs shown to catch one mutation at a time on the inputs of tests/test_gpu_eval_tables.py, and the argument
refusals of the four 1-D entry points (decided before anything touches a device)."""
import ctypes
import warnings

import numpy as np
import pytest

import eval_refs as er
from oracle import eval_oracle as eo

_dp = ctypes.POINTER(ctypes.c_double)
PTR = 0x10000            # a non-null "device pointer": validation fails before it would be used


@pytest.fixture(scope="module")
def choose():
    import evaluation
    return evaluation._choose_epsilon


# ---- (a) the specification against the oracle ------------------------------------------------------------------------------------
def _bursts(n, k, rng):
    e = (rng.random(n) * 0.1).astype(np.float32)
    for _ in range(k):
        at = int(rng.integers(0, n))
        e[at:at + int(rng.integers(1, 12))] += np.float32(1.0 + 2.0 * rng.random())
    return e


@pytest.mark.parametrize("n", [1, 2, 49, 50, 99, 100, 255, 256, 257, 305, 1000, 4099])
def test_reference_find_epsilon_equals_the_oracle(n, choose):
    rng = np.random.default_rng([21, n])
    differences = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # the oracle's mean of an empty pruned set, 0 / 0 at n = 1
        for bursts in (0, 1, 2, 3):
            for _ in range(3):
                e = _bursts(n, bursts, rng)
                for reg in (0, 1, 2):
                    got, ref = er.find_epsilon(e, reg, choose), eo.find_epsilon(e, reg)
                    differences += not abs(got - ref) <= 1e-12 * abs(ref)
    assert differences == 0


def _adjust_cases():
    return [(n, kind) for n in er.ADJUST_SIZES for kind in er.ADJUST_LABELS]


@pytest.mark.parametrize("compare_f32", [False, True])
def test_reference_point_adjust_equals_the_oracle(compare_f32):
    for n, kind in _adjust_cases():
        s, lab, thr = er.adjust_case(n, kind)
        tab = er.point_adjust_table(s, lab, thr, compare_f32)
        assert np.all(tab[:, :4].sum(axis=1) == n), (n, kind)
        for k in range(0, thr.size, 5):
            with np.errstate(invalid="ignore"):
                pred, lat = eo.point_adjust(s, lab, thr[k], compare_f32)
            f = eo.confusion(pred, lab)
            assert tuple(tab[k, :4]) == (f[3], f[4], f[5], f[6]), (n, kind, k)
            assert abs(tab[k, 4] / (tab[k, 5] + 1e-4) - lat) <= 1e-12 * max(1.0, lat), (n, kind, k)


def test_point_adjust_inputs_separate_the_two_comparison_modes():
    """The thresholds just below a score: `score > thr` in float64, not once thr is rounded to float32."""
    for n in (255, 4099):
        s, lab, thr = er.adjust_case(n, "random")
        t64, t32 = er.point_adjust_table(s, lab, thr, False), er.point_adjust_table(s, lab, thr, True)
        assert np.array_equal(t64[:24], t32[:24])                         # exact float32 thresholds: the modes agree
        assert (t64[24:48] != t32[24:48]).any(axis=1).sum() >= 12, n      # just below a score: they do not
        with pytest.raises(AssertionError):
            er.check_counts(t32, t64)
        # NaN scores are never above, a NaN threshold flags nothing, -inf flags every non-NaN score
        nan_row, minus_inf = t64[50], t64[49]
        assert nan_row[0] == 0 and nan_row[2] == 0 and nan_row[5] == 0
        assert minus_inf[2] == np.sum((lab == 0) & ~np.isnan(s))


def test_reference_scores_definition():
    p, r, a = er.score_case(257, 3)
    dims = er.score_dims(3)
    per_dim, glob = er.scores(p, r, a, dims, 0.3)
    g = float(np.float32(0.3))
    for i in (0, 100, 256):
        for k in range(3):
            t = float(a[i, dims[k]])
            assert per_dim[i, k] == abs(float(p[i, k]) - t) + g * abs(float(r[i, k]) - t)
        assert abs(glob[i] - per_dim[i].mean()) <= 1e-15 * glob[i]
    assert (er.scores(p, r, a, None, 0.0)[0] == 0).any()                # the exact equalities p = t are there
    assert (er.scores(p, r, a, dims, 0.0)[0] == 0).any()


# ---- (b) the rules of _choose_epsilon ----------------------------------------------------------------------------------------------
N, MEAN, SD = 1000, 1.0, 0.5


def _row(pruned_mean, pruned_sd, count, dil):
    """A table row whose pruned set has the given mean, standard deviation and size."""
    return [pruned_mean * count, (pruned_sd ** 2 + pruned_mean ** 2) * count, count, dil]


def _pick(choose, rows, reg_level=0, eps=None):
    eps = np.arange(1.0, 1.0 + len(rows)) if eps is None else eps
    return choose(N, MEAN, SD, eps, [x for r in rows for x in r], reg_level)


def test_choose_epsilon_keeps_the_last_of_two_z_with_the_same_pruned_set(choose):
    same = _row(0.8, 0.3, 990, 20)
    assert _pick(choose, [same, same]) == 2.0
    assert _pick(choose, [same, same, _row(0.9, 0.4, 995, 10)]) == 2.0       # a worse row after them does not win
    # sums that differ in their last bits (the device's atomics) still count as equal
    wobble = [same[0] * (1 + 2e-16), same[1] * (1 - 2e-16), same[2], same[3]]
    assert _pick(choose, [wobble, same]) == 2.0 and _pick(choose, [same, wobble]) == 2.0


def test_choose_epsilon_skips_a_row_dilated_over_half_the_array(choose):
    best, fair = _row(0.5, 0.1, 400, N // 2), _row(0.8, 0.3, 990, 20)
    assert _pick(choose, [fair, best]) == 1.0
    assert _pick(choose, [best, fair]) == 2.0
    assert _pick(choose, [fair, _row(0.5, 0.1, 400, N // 2 - 1)]) == 2.0     # one under n / 2 qualifies


def test_choose_epsilon_skips_a_row_without_exceedances(choose):
    best, fair = _row(0.5, 0.1, 400, 0), _row(0.8, 0.3, 990, 20)
    assert _pick(choose, [fair, best]) == 1.0
    assert _pick(choose, [best, fair]) == 2.0


def test_choose_epsilon_skips_an_empty_pruned_set(choose):
    empty, fair = [0.0, 0.0, 0.0, 20], _row(0.8, 0.3, 990, 20)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # NaN, not a warning and not ZeroDivisionError
        assert _pick(choose, [fair, empty]) == 1.0
        assert _pick(choose, [empty, fair]) == 2.0
        assert _pick(choose, [empty]) is None


def test_choose_epsilon_returns_none_when_no_row_qualifies(choose):
    rows = [_row(0.5, 0.1, 400, 0), _row(0.5, 0.1, 400, N // 2), [0.0, 0.0, 0.0, 20], [0.0] * 4]
    for reg in (0, 1, 2):
        assert _pick(choose, rows, reg) is None


def test_choose_epsilon_regularisation_divides_by_the_dilated_count(choose):
    few, many = _row(0.8, 0.3, 990, 10), _row(0.6, 0.2, 900, 200)           # `many` prunes more, `few` dilates less
    assert _pick(choose, [few, many], 0) == 2.0
    assert _pick(choose, [few, many], 1) == 1.0 and _pick(choose, [few, many], 2) == 1.0


# ---- (c) the gates are sharp ---------------------------------------------------------------------------------------------------------
def _small_eps_cases():
    return [(n, h) for h in er.EPS_HALOS for n in er.eps_sizes(h) if n <= 257 + h]


def test_gates_catch_a_halo_one_off():
    """On every small input of the GPU test where a halo one off changes the table at all (n >= halo + 2), and at a trip edge."""
    seen = 0
    for n, halo in _small_eps_cases() + [(er.EPS_TRIP + 1, 49)]:
        if n < halo + 2:
            continue
        e, eps = er.epsilon_case(n, halo)
        sel = slice(er.EPS_ROW_BELOW, er.EPS_ROW_OWN + 8) if n > 1000 else slice(None)       # the large case: some rows are enough
        want = er.epsilon_table(e, eps[sel], halo)
        for wrong in (halo - 1, halo + 1):
            if wrong < 0:
                continue
            with pytest.raises(AssertionError, match="count row"):
                er.check_counts(er.epsilon_table(e, eps[sel], wrong)[:, 2:], want[:, 2:])
            seen += 1
    assert seen >= 50                    # the loop did not run empty


def test_gates_catch_a_strict_hot_flag():
    for n, halo in _small_eps_cases():
        e, eps = er.epsilon_case(n, halo)
        want = er.epsilon_table(e, eps, halo)

        def strict(e32, ez):
            with np.errstate(invalid="ignore"):
                return np.asarray(e32, np.float32).astype(np.float64) > ez
        got = er.epsilon_table(e, eps, halo, hot=strict)
        assert want[er.EPS_ROW_OWN, 3] > 0 and want[er.EPS_ROW_OWN + 1, 3] == got[er.EPS_ROW_OWN, 3]
        with pytest.raises(AssertionError, match="count row"):
            er.check_counts(got[:, 2:], want[:, 2:])


def test_gates_catch_one_pruned_count_and_the_sample_at_a_tile_edge():
    T = er.EPS_TILE
    for halo in er.EPS_HALOS:
        n = T + halo
        if n <= T:
            n = T + 1
        e, eps = er.epsilon_case(n, halo)
        want = er.epsilon_table(e, eps, halo)
        got = want.copy()
        got[7, 2] += 1
        with pytest.raises(AssertionError, match="count row 7"):
            er.check_counts(got[:, 2:], want[:, 2:])

        def without_edge(e32, ez):
            hot = er.hot_flags(e32, ez).copy()
            hot[T] = False
            return hot
        assert er.spike_indices(n, halo)[:2] == [0, T]        # the row of the second spike's own value: 0 and T alone are hot
        with pytest.raises(AssertionError, match="count row"):
            er.check_counts(er.epsilon_table(e, eps, halo, hot=without_edge)[:, 2:], want[:, 2:])


def test_the_part_table_references_keep_the_row_conventions():
    """What tests/test_gpu_eval_tables.py asserts of the per-part rows holds for the reference alone, on every part's slice."""
    for halo in er.PART_TABLE_HALOS:
        x, start, end, eps = er.part_table_case(halo)
        assert (end - start).tolist() == list(er.PART_TABLE_SCORES) and x.size == end[-1]
        for s, e, row in zip(start, end, eps):
            n = int(e - s)
            tab = er.epsilon_table(x[s:e], row, halo)
            assert tab[er.EPS_ROW_NAN].tolist() == [0.0, 0.0, 0.0, 0.0]
            if n == 0:
                assert not tab.any() and er.moments(x[s:e]) == (0.0, 0.0)
                continue
            assert tab[er.EPS_ROW_BELOW].tolist() == [0.0, 0.0, 0.0, float(n)] and tab[er.EPS_ROW_ABOVE, 2:].tolist() == [float(n), 0.0]
            assert er.spike_indices(n, halo)[:2] == ([0, n - 1] if n > 1 and n <= er.EPS_TILE else [0, er.EPS_TILE][:n])


def test_gates_catch_a_sum_outside_its_bound():
    e, eps = er.epsilon_case(257, 49)
    want, absum = er.epsilon_table(e, eps, 49, with_abs=True)
    assert er.check_sums(want[:, 0], want[:, 0], want[:, 2], absum) == 0.0
    bound = want[:, 2] * er.U64 * absum
    k = er.EPS_ROW_ABOVE
    assert bound[k] > 0 and bound[er.EPS_ROW_BELOW] == 0 and bound[er.EPS_ROW_NAN] == 0
    for sign in (-2.0, 2.0):
        got = want[:, 0].copy()
        got[k] += sign * bound[k]
        with pytest.raises(AssertionError, match=f"sum row {k}"):
            er.check_sums(got, want[:, 0], want[:, 2], absum)
        got = want[:, 1].copy()
        got[k] += sign * want[k, 2] * er.U64 * want[k, 1]
        with pytest.raises(AssertionError, match=f"sum row {k}"):
            er.check_sums(got, want[:, 1], want[:, 2], want[:, 1])
    got = want[:, 0].copy()
    got[k] += 0.5 * bound[k]
    assert 0.45 <= er.check_sums(got, want[:, 0], want[:, 2], absum) <= 0.55      # inside the bound passes and is reported
    got = want[:, 0].copy()
    got[er.EPS_ROW_NAN] = 5e-324                                                   # the zero row is exact
    with pytest.raises(AssertionError, match=f"sum row {er.EPS_ROW_NAN}"):
        er.check_sums(got, want[:, 0], want[:, 2], absum)
    m = er.moment_columns(257, 1)[:, 0]
    s, s2 = er.moments(m)
    with pytest.raises(AssertionError):
        er.check_sums([s + 2 * 257 * er.U64 * er.abs_sum(m)], [s], 257, er.abs_sum(m))
    with pytest.raises(AssertionError):
        er.check_sums([float("nan")], [s2], 257, s2)


def test_gates_catch_one_sample_moved_from_tp_to_fn():
    s, lab, thr = er.adjust_case(257, "random")
    want = er.point_adjust_table(s, lab, thr)
    got = want.copy()
    got[3, 0] -= 1
    got[3, 3] += 1
    with pytest.raises(AssertionError, match="count row 3"):
        er.check_counts(got, want)
    er.check_counts(want.copy(), want)


def test_gates_catch_a_score_outside_its_bound():
    p, r, a = er.score_case(257, 3)
    per_dim, glob = er.scores(p, r, a, None, 0.3)
    i = tuple(int(x[0]) for x in np.nonzero(per_dim > 0))
    for sign in (-2.0, 2.0):
        got = per_dim.copy()
        got[i] += sign * 4 * er.U32 * per_dim[i]
        with pytest.raises(AssertionError, match="score"):
            er.check_scores(got, per_dim)
        got = glob.copy()
        got[5] += sign * (3 + 4) * er.U32 * glob[5]
        with pytest.raises(AssertionError, match="score"):
            er.check_scores(got, glob, d=3)
    got = per_dim.copy()
    zero = tuple(int(x[0]) for x in np.nonzero(per_dim == 0))
    got[zero] = 1e-30                                                    # p = t and r = t: the score is 0 exactly
    with pytest.raises(AssertionError, match="score"):
        er.check_scores(got, per_dim)
    assert er.check_scores(per_dim.astype(np.float32), per_dim) <= 0.25            # rounding the reference once: one of the four


# ---- (d) argument refusals of the 1-D entry points ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import evaluation
    return evaluation._lib()


MOMENTS_BAD = {"n = 0": dict(n=0), "n < 0": dict(n=-5), "null e": dict(e=None), "null scratch": dict(scratch=None), "null out": dict(out=False)}


@pytest.mark.parametrize("case", list(MOMENTS_BAD))
def test_moments_rejects_invalid_arguments(lib, case):
    kw = dict(e=PTR, n=300, scratch=PTR, out=True)
    kw.update(MOMENTS_BAD[case])
    out = (ctypes.c_double * 2)() if kw["out"] else None
    assert lib.mtadgat_eval_moments(kw["e"], kw["n"], kw["scratch"], out, None) == -1


EPSILON_BAD = {"nz = 0": dict(nz=0), "nz < 0": dict(nz=-1), "nz = 65": dict(nz=65), "n = 0": dict(n=0), "halo < 0": dict(halo=-1),
               "halo very negative": dict(halo=-2 ** 31), "null e": dict(e=None), "null eps": dict(eps=False), "null scratch": dict(scratch=None),
               "null out": dict(out=False)}


@pytest.mark.parametrize("case", list(EPSILON_BAD))
def test_epsilon_table_rejects_invalid_arguments(lib, case):
    kw = dict(e=PTR, n=300, eps=True, nz=19, halo=49, scratch=PTR, out=True)
    kw.update(EPSILON_BAD[case])
    eps = (ctypes.c_double * 65)() if kw["eps"] else None
    out = (ctypes.c_double * (4 * 65))() if kw["out"] else None
    assert lib.mtadgat_eval_epsilon_table(kw["e"], kw["n"], eps, kw["nz"], kw["halo"], kw["scratch"], out, None) == -1


ADJUST_BAD = {"n_thr = 0": dict(n_thr=0), "n_thr < 0": dict(n_thr=-3), "max_seg = 0": dict(max_seg=0), "max_seg < 0": dict(max_seg=-1),
              "n = 0": dict(n=0), "null score": dict(score=None), "null label": dict(label=None), "null thr": dict(thr=False),
              "null scratch": dict(scratch=None), "null out": dict(out=False)}


@pytest.mark.parametrize("case", list(ADJUST_BAD))
def test_point_adjust_rejects_invalid_arguments(lib, case):
    kw = dict(score=PTR, label=PTR, n=300, thr=True, n_thr=7, max_seg=64, scratch=PTR, out=True)
    kw.update(ADJUST_BAD[case])
    thr = (ctypes.c_double * 7)() if kw["thr"] else None
    out = (ctypes.c_double * (6 * 7))() if kw["out"] else None
    for mode in (0, 1):
        assert lib.mtadgat_eval_point_adjust(kw["score"], kw["label"], kw["n"], thr, kw["n_thr"], mode, kw["max_seg"], kw["scratch"], out,
                                             None) == -1


SCORES_BAD = {"d = 0": dict(d=0), "d < 0": dict(d=-2), "null preds": dict(preds=None), "null recons": dict(recons=None),
              "null actual": dict(actual=None)}


@pytest.mark.parametrize("case", list(SCORES_BAD))
def test_scores_rejects_invalid_arguments(lib, case):
    kw = dict(preds=PTR, recons=PTR, actual=PTR, n=300, d=3)
    kw.update(SCORES_BAD[case])
    assert lib.mtadgat_eval_scores(kw["preds"], kw["recons"], kw["actual"], kw["n"], kw["d"], 3, None, 1.0, PTR, PTR, None) == -1
