"""tests/score_mask_refs.py -- the specification the masked scoring kernels are held to (tests/test_gpu_score_mask.py) -- against
pandas and numpy, against the unmasked references where nothing is missing, and against the window rule of tests/fit_mask_refs.py.
Also the margin of the threshold cases the GPU test uses: their two best z scores differ by more than 1e-6 relative, so the 1e-9
gate there cannot fail on a tie."""
import numpy as np
import pytest

import fit_mask_refs
import score_mask_refs as spec
import score_refs
from oracle import eval_oracle as eo

SIZES = (1, 2, 3, 64, 65, 257, 1025, 4099)
GAPS = (0.0, 0.15, 0.6, 1.0)
SPANS = (1, 2, 7, 1280)


def _gappy(n, p, seed):
    rng = np.random.default_rng(seed)
    x = (rng.random(n) * 3.0).astype(np.float32)
    x[rng.random(n) < p] = np.nan
    return x


@pytest.mark.parametrize("n", SIZES)
def test_ewm_valid_equals_pandas_at_observed_rows(n):
    pd = pytest.importorskip("pandas")
    for p in GAPS:
        x = _gappy(n, p, 7 * n + int(100 * p))
        for span in SPANS:
            got = spec.ewm_valid(x, span)
            want = pd.Series(x.astype(np.float64)).ewm(span=span, adjust=True, ignore_na=False).mean().to_numpy()
            obs = ~np.isnan(x)
            assert np.array_equal(np.isnan(got), ~obs)                  # the departure: pandas repeats the previous mean there
            assert np.all(np.abs(got[obs] - want[obs]) <= 1e-13 * np.abs(want[obs])), (n, p, span)


@pytest.mark.parametrize("n", SIZES)
def test_nan_quantile_equals_nanpercentile(n):
    qs = [0.0, 0.25, 0.5, 0.75, 1.0]
    for p in GAPS:
        rng = np.random.default_rng(11 * n + int(100 * p))
        a = score_refs.columns(n, 7, rng)[:, [0, 1, 2, 3, 5, 6]]       # (the inf column gives inf - inf warnings in numpy: left out)
        a[rng.random(a.shape) < p] = np.nan
        got, counts = spec.nan_quantile(a, qs)
        assert np.array_equal(counts, (~np.isnan(a)).sum(axis=0))
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = np.nanpercentile(a.astype(np.float64), [100 * q for q in qs], axis=0, method="linear")
        assert np.array_equal(np.isnan(got), np.isnan(want)), (n, p)
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok]) + 1e-300), (n, p)


@pytest.mark.parametrize("n", SIZES)
def test_without_nan_the_spec_is_the_unmasked_reference(n):
    rng = np.random.default_rng(n)
    a = score_refs.columns(n, 5, rng)
    qs = [0.0, 0.25, 0.5, 0.75, 1.0]
    got, counts = spec.nan_quantile(a, qs)
    want = score_refs.quantile(a, qs)
    assert np.array_equal(counts, np.full(5, n)) and np.array_equal(got, want, equal_nan=True)
    x = (rng.random(n) * 3.0).astype(np.float32)
    for span in SPANS:
        got, want = spec.ewm_valid(x, span), score_refs.ewm(x, span)
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (n, span)
    mom = spec.moments_valid(a[:, :3])
    assert np.array_equal(mom[:, 2], np.full(3, n))
    assert np.allclose(mom[:, 0], a[:, :3].astype(np.float64).sum(axis=0), rtol=1e-12)


def bursty(n, d, seed):
    """The scores of tests/test_gpu_score_pipeline.py::_bursty, restated: that module is marked gpu as a whole."""
    rng = np.random.default_rng(seed)
    e = (rng.random((n, d)) * 0.1).astype(np.float32)
    for c in range(d):
        for _ in range(3):
            at = int(rng.integers(0, n - 12))
            e[at:at + int(rng.integers(1, 12)), c] += np.float32(1.0 + 2.0 * rng.random())
    return e


def planted(n, d, seed):
    """Bursty columns with NaN planted inside a burst, next to one and away from them; the last column all NaN (d >= 2)."""
    e = bursty(n, d, seed)
    rng = np.random.default_rng(seed + 1)
    for c in range(d):
        hot = np.flatnonzero(e[:, c] > 0.5)
        e[hot[len(hot) // 2], c] = np.nan                               # inside
        e[min(hot[-1] + 1, n - 1), c] = np.nan                         # next to
        e[max(hot[0] - 1, 0), c] = np.nan
        cold = np.flatnonzero(e[:, c] < 0.5)
        e[rng.choice(cold, size=max(n // 20, 1), replace=False), c] = np.nan     # away
    if d >= 2:
        e[:, d - 1] = np.nan
    return e


EPSILON_CASES = ((300, 1, 101), (1000, 5, 105), (5000, 9, 109))


@pytest.mark.parametrize("n,d,seed", EPSILON_CASES)
def test_find_epsilon_valid_without_nan_is_the_oracle_and_the_cases_have_a_margin(n, d, seed):
    e = bursty(n, d, seed)
    for reg in (0, 1, 2):
        for c in range(d):
            assert spec.find_epsilon_valid(e[:, c], reg) == pytest.approx(eo.find_epsilon(e[:, c], reg), rel=1e-12)
    g = planted(n, d, seed)
    for reg in (0, 1, 2):
        for c in range(d):
            thr, scores = spec.find_epsilon_valid(g[:, c], reg, with_scores=True)
            if d >= 2 and c == d - 1:
                assert np.isnan(thr)
                continue
            assert np.isfinite(thr)
            assert spec.best_two_margin(scores) > 1e-6, (n, c, reg, scores)
            plain, plain_scores = spec.find_epsilon_valid(e[:, c], reg, with_scores=True)
            assert spec.best_two_margin(plain_scores) > 1e-6, (n, c, reg, plain_scores)


@pytest.mark.parametrize("n_rows,W,F", [(8, 7, 1), (3, 1, 5), (300, 12, 5), (1100, 7, 38)])
def test_scored_rows_is_the_window_rule(n_rows, W, F):
    rng = np.random.default_rng(n_rows + F)
    third = n_rows // 3
    for p in (0.0, 0.15, 0.6):
        for lengths in (None, [third, min(W, n_rows - third), n_rows - third - min(W, n_rows - third)]):
            age = fit_mask_refs.age_of(rng.random((n_rows, F)) < p, lengths)
            for dims in (None, [F - 1] if F > 1 else [0]):
                for mo in (0.0, 0.5, 1.0):
                    for max_age in (0, 2):
                        keep = spec.scored_rows(n_rows, W, F, age, max_age, mo, dims, lengths)
                        starts = fit_mask_refs.windows(n_rows, W, F, lengths, age, max_age, dims, spec.min_count(mo, W, F))
                        assert keep.dtype == np.uint8 and keep.shape == (n_rows - W,)
                        assert np.array_equal(np.flatnonzero(keep), starts), (p, lengths, dims, mo, max_age)


def test_scores_masked_select_and_counts():
    rng = np.random.default_rng(3)
    n, d, F = 40, 3, 6
    p, r = rng.random((n, d)).astype(np.float32), rng.random((n, d)).astype(np.float32)
    actual = rng.random((n, F)).astype(np.float32)
    age = (rng.random((n, F)) < 0.4).astype(np.int32) * 3
    dims = [4, 0, 5]
    actual[age > 0] = np.nan                                            # a NaN under the mask does not reach the mean
    keep = np.ones(n, np.uint8)
    keep[7] = 0
    per_dim, glob, count = spec.scores_masked(p, r, actual, age, 0, keep, dims, 0.37)
    valid = (age[:, dims] <= 0) & (keep[:, None] != 0)
    assert np.array_equal(np.isnan(per_dim), ~valid) and np.array_equal(count, valid.sum(axis=1))
    assert np.array_equal(np.isnan(glob), count == 0) and count[7] == 0
    row = int(np.flatnonzero(count == d)[0])
    t = actual[row, dims]
    want = np.abs((p[row] - t).astype(np.float64)) + np.float64(np.float32(0.37)) * np.abs((r[row] - t).astype(np.float64))
    assert np.array_equal(per_dim[row], want) and glob[row] == pytest.approx(want.mean(), rel=1e-15)
    # with a permissive max_age the NaN under the former mask is a value again
    assert np.isnan(spec.scores_masked(p, r, actual, age, 3, None, dims, 0.37)[1]).sum() == (age[:, dims] > 0).any(axis=1).sum()
