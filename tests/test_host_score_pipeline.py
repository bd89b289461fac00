"""The score post-processing entry points (column quantiles, moving average, column find_epsilon passes) without a GPU:
symbols, argument validation before anything touches the device, scratch sizes; and the float64 references the GPU
tests compare against (tests/score_refs.py), held against numpy and pandas."""
import ctypes

import numpy as np
import pytest

import score_refs

_dp = ctypes.POINTER(ctypes.c_double)
PTR = 0x10000            # a non-null, 16-byte aligned "device pointer": validation fails before it would be used


@pytest.fixture(scope="module")
def lib():
    import evaluation
    return evaluation._lib()


def _err(lib):
    return lib.mtadgat_last_error().decode()


def test_symbols_are_exported(lib):
    for name in ("mtadgat_eval_column_quantiles", "mtadgat_eval_column_quantiles_scratch", "mtadgat_eval_ewm", "mtadgat_eval_ewm_scratch",
                 "mtadgat_eval_moments_columns", "mtadgat_eval_epsilon_table_columns"):
        assert hasattr(lib, name), name


def _quantiles(lib, a=PTR, n=100, d=4, ld=4, q=(0.25, 0.5), nq=None, scratch=PTR, scratch_bytes=None, out=PTR):
    qa = (ctypes.c_double * max(len(q), 1))(*q)
    nq = len(q) if nq is None else nq
    if scratch_bytes is None:
        scratch_bytes = lib.mtadgat_eval_column_quantiles_scratch(max(n, 1), max(d, 1), max(nq, 1))
    return lib.mtadgat_eval_column_quantiles(a, n, d, ld, qa, nq, scratch, scratch_bytes, out, None)


QUANTILE_BAD = {
    "null a": dict(a=None), "null scratch": dict(scratch=None), "null out": dict(out=None),
    "n < 1": dict(n=0), "d < 1": dict(d=0, ld=4), "ld < d": dict(ld=3), "nq < 1": dict(nq=0),
    "q < 0": dict(q=(0.5, -0.01)), "q > 1": dict(q=(1.0000001,)), "q nan": dict(q=(float("nan"),)),
    "scratch one byte short": dict(scratch_bytes=-1),
}


@pytest.mark.parametrize("case", list(QUANTILE_BAD))
def test_column_quantiles_rejects_invalid_arguments(lib, case):
    kw = dict(QUANTILE_BAD[case])
    if kw.get("scratch_bytes") == -1:
        kw["scratch_bytes"] = lib.mtadgat_eval_column_quantiles_scratch(100, 4, 2) - 1
    assert _quantiles(lib, **kw) != 0
    assert _err(lib)


def test_column_quantiles_rejects_null_q(lib):
    need = lib.mtadgat_eval_column_quantiles_scratch(100, 4, 2)
    assert lib.mtadgat_eval_column_quantiles(PTR, 100, 4, 4, None, 2, PTR, need, PTR, None) != 0
    assert "null" in _err(lib)


EWM_BAD = {
    "null x": dict(x=None), "null scratch": dict(scratch=None), "null out": dict(out=None), "n < 1": dict(n=0),
    "alpha = 0": dict(alpha=0.0), "alpha < 0": dict(alpha=-0.5), "alpha > 1": dict(alpha=1.0000001), "alpha nan": dict(alpha=float("nan")),
    "scratch one byte short": dict(scratch_bytes=-1),
}


@pytest.mark.parametrize("case", list(EWM_BAD))
def test_ewm_rejects_invalid_arguments(lib, case):
    kw = dict(x=PTR, n=5000, alpha=0.25, scratch=PTR, scratch_bytes=lib.mtadgat_eval_ewm_scratch(5000), out=PTR)
    kw.update(EWM_BAD[case])
    if kw["scratch_bytes"] == -1:
        kw["scratch_bytes"] = lib.mtadgat_eval_ewm_scratch(5000) - 1
    assert lib.mtadgat_eval_ewm(kw["x"], kw["n"], kw["alpha"], kw["scratch"], kw["scratch_bytes"], kw["out"], None) != 0
    assert _err(lib)


COLUMNS_BAD = {"null e": dict(e=None), "null scratch": dict(scratch=None), "null out": dict(out=False), "n < 1": dict(n=0),
               "d < 1": dict(d=0), "ld < d": dict(ld=2)}


@pytest.mark.parametrize("case", list(COLUMNS_BAD))
def test_column_epsilon_passes_reject_invalid_arguments(lib, case):
    kw = dict(e=PTR, n=300, d=3, ld=3, scratch=PTR, out=True)
    kw.update(COLUMNS_BAD[case])
    nz = 19
    mom = (ctypes.c_double * 6)() if kw["out"] else None
    assert lib.mtadgat_eval_moments_columns(kw["e"], kw["n"], kw["d"], kw["ld"], kw["scratch"], mom, None) != 0
    assert _err(lib)
    eps = (ctypes.c_double * (3 * nz))()
    tab = (ctypes.c_double * (4 * 3 * nz))() if kw["out"] else None
    assert lib.mtadgat_eval_epsilon_table_columns(kw["e"], kw["n"], kw["d"], kw["ld"], eps, nz, 49, kw["scratch"], tab, None) != 0
    assert _err(lib)
    assert lib.mtadgat_eval_epsilon_table_columns(PTR, 300, 3, 3, None, nz, 49, PTR, tab or eps, None) != 0      # null eps


def test_scratch_queries_grow_monotonically(lib):
    cq, ew = lib.mtadgat_eval_column_quantiles_scratch, lib.mtadgat_eval_ewm_scratch
    assert cq(1, 1, 1) > 0 and ew(1) > 0
    ns = [1, 2, 1000, 1024, 1025, 65536, 1 << 24, (1 << 31) - 1]
    ds = [1, 2, 7, 8, 9, 38, 512, 2048]
    nqs = [1, 2, 3, 4, 5, 64]
    for a, b in zip(ns, ns[1:]):
        assert cq(a, 38, 3) <= cq(b, 38, 3) and ew(a) <= ew(b)
    assert ew(1 << 24) > ew(1024)
    for a, b in zip(ds, ds[1:]):
        assert cq(65536, a, 3) < cq(65536, b, 3)
    for a, b in zip(nqs, nqs[1:]):
        assert cq(65536, 38, a) < cq(65536, 38, b)


def test_ewm_scratch_queries_are_the_documented_bytes(lib):
    """With c = ceil(n / 1024) chunks: S and carry, a double per chunk each; the per-part scan adds an int per chunk, its region
    rounded up to 8 bytes; the scan over observed rows carries two doubles where the plain one carries one."""
    plain, parts, valid = lib.mtadgat_eval_ewm_scratch, lib.mtadgat_eval_ewm_parts_scratch, lib.mtadgat_eval_ewm_valid_scratch
    for n in (1, 1024, 1025, 65536, 65537, (1 << 31) - 1):
        c = (n + 1023) // 1024
        assert plain(n) == 16 * c, n
        assert parts(n) == 16 * c + (4 * c + 7) // 8 * 8, n
        assert valid(n) == 32 * c, n
    for n in (0, -1):
        assert plain(n) == 0 and parts(n) == 0 and valid(n) == 0, n
    assert parts(1 << 31) == 0 and valid(1 << 31) == 0
    assert plain(1 << 31) == 16 * (1 << 21)           # the plain query alone leaves n > 2^31 - 1 to the call, which rejects it


def test_reference_moving_average_equals_pandas():
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(11)
    for n in (1, 2, 257, 4097, 70001):
        for x in (rng.random(n) * 3.0, np.full(n, 1.25)):
            for span in (1, 2, 7, 1280):
                ref = pd.DataFrame(x).ewm(span=span).mean().to_numpy()[:, 0]
                got = score_refs.ewm(x, span)
                assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref)), (n, span, np.abs(got - ref).max())


def test_reference_quantile_equals_numpy_percentile():
    rng = np.random.default_rng(12)
    qs = [0.0, 0.25, 0.5, 0.75, 1.0, 0.3333, 0.9]
    for n in (1, 2, 3, 255, 256, 257, 4099):
        a = score_refs.columns(n, 4, rng)              # every kind but the column with an inf
        ref = np.percentile(a.astype(np.float64), [100.0 * q for q in qs], axis=0)
        got = score_refs.quantile(a, qs)
        assert np.all(np.abs(got - ref) <= 0.5 * score_refs.ulp32(ref)), (n, np.abs(got - ref).max())
    a = rng.random((50, 3)).astype(np.float32)
    a[7, 1] = np.nan
    got = score_refs.quantile(a, qs)
    assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, [0, 2]]).all()
    assert np.isnan(np.percentile(a.astype(np.float64), 50, axis=0)[1])
