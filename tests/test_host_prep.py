"""The preparation step without a GPU: the C entry points' argument checks and scratch queries, the specification
(tests/prep_refs.py) against sklearn's MinMaxScaler bit for bit, hand-written hold / age cases, and the torch-op route CPU tensors
take in preparation.py against the specification bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import prep_refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -5
P = 4096                     # a non-null, 16-byte aligned stand-in for a device pointer: every call below is refused before it is used
NAMES = ("mtadgat_prep_rows_per_block", "mtadgat_prep_fit_scratch", "mtadgat_prep_fit", "mtadgat_prep_transform_scratch",
         "mtadgat_prep_transform", "mtadgat_prep_inverse", "mtadgat_prep_stream_state_bytes", "mtadgat_prep_stream_init",
         "mtadgat_prep_stream_push", "mtadgat_prep_stream_reset")


@pytest.fixture(scope="module")
def lib():
    import preparation
    return preparation._lib()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), what


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "mtadgat.h")).read()
    declared = set(re.findall(r"\b(mtadgat_prep_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(NAMES)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.mtadgat_abi_version() == 1
    rb = lib.mtadgat_prep_rows_per_block()
    assert rb >= 64 and rb % 64 == 0


def test_fit_refuses_bad_arguments(lib):
    ok = dict(x=P, n=100, d=5, ld=5, gaps=0, scratch=P, nbytes=1 << 30, rec=P)

    def call(**over):
        a = dict(ok, **over)
        return lib.mtadgat_prep_fit(a["x"], a["n"], a["d"], a["ld"], a["gaps"], a["scratch"], a["nbytes"], a["rec"], None)

    for bad in (dict(x=None), dict(scratch=None), dict(rec=None), dict(n=0), dict(n=1 << 31), dict(d=0), dict(d=2049), dict(ld=4),
                dict(ld=1 << 31), dict(gaps=2), dict(gaps=-1)):
        assert call(**bad) == INVALID, bad
        assert b"prep_fit" in lib.mtadgat_last_error()
    assert call(nbytes=lib.mtadgat_prep_fit_scratch(100, 5) - 1) == WORKSPACE
    assert call(scratch=P + 4) == WORKSPACE


def test_transform_refuses_bad_arguments(lib):
    ok = dict(x=P, n=100, d=5, ld=5, rec=P, fill=2, clip=0, start=None, end=None, count=0, scratch=P, nbytes=1 << 30, out=2 * P, ld_out=5,
              age=None)

    def call(**over):
        a = dict(ok, **over)
        return lib.mtadgat_prep_transform(a["x"], a["n"], a["d"], a["ld"], a["rec"], a["fill"], a["clip"], a["start"], a["end"], a["count"],
                                          a["scratch"], a["nbytes"], a["out"], a["ld_out"], a["age"], None)

    for bad in (dict(x=None), dict(rec=None), dict(out=None), dict(scratch=None), dict(n=0), dict(n=1 << 31), dict(d=0), dict(d=2049),
                dict(ld=4), dict(ld_out=4), dict(fill=3), dict(fill=-1), dict(count=-1), dict(count=2), dict(count=2, start=P),
                dict(count=2, end=P), dict(out=P, ld=7, ld_out=5), dict(fill=1, age=P, scratch=None)):
        assert call(**bad) == INVALID, bad
        assert b"prep_transform" in lib.mtadgat_last_error()
    need = lib.mtadgat_prep_transform_scratch(100, 5, 2, 0)
    assert call(nbytes=need - 1) == WORKSPACE
    assert call(scratch=P + 4) == WORKSPACE
    assert call(fill=0, age=P, nbytes=need - 1) == WORKSPACE                 # the age alone takes the scan, and its scratch


def test_inverse_and_stream_calls_refuse_bad_arguments(lib):
    def inverse(y=P, n=10, d=3, ld=3, rec=P, ds=5, dims=None, out=2 * P, ld_out=3):
        return lib.mtadgat_prep_inverse(y, n, d, ld, rec, ds, dims, out, ld_out, None)

    for bad in (dict(y=None), dict(rec=None), dict(out=None), dict(n=0), dict(d=0), dict(d=2049), dict(ld=2), dict(ld_out=2), dict(ds=0),
                dict(ds=2049), dict(d=6, ld=6, ld_out=6), dict(out=P, ld=4)):
        assert inverse(**bad) == INVALID, bad

    assert lib.mtadgat_prep_stream_state_bytes(0, 5) == 0 and lib.mtadgat_prep_stream_state_bytes(4, 0) == 0
    assert lib.mtadgat_prep_stream_state_bytes(4, 2049) == 0
    small, large = lib.mtadgat_prep_stream_state_bytes(4, 5), lib.mtadgat_prep_stream_state_bytes(5, 5)
    assert 3 * 4 * 4 * 5 <= small < large and small % 16 == 0
    for args in ((None, 4, 5), (P, 0, 5), (P, 4, 0), (P, 4, 2049), (P + 8, 4, 5)):
        assert lib.mtadgat_prep_stream_init(*args, None) == INVALID, args

    def push(state=P, S=4, d=5, rows=P, streams=None, n=4, T=2, rec=P, fill=2, clip=0, out=2 * P, age=None):
        return lib.mtadgat_prep_stream_push(state, S, d, rows, streams, n, T, rec, fill, clip, out, age, None)

    for bad in (dict(state=None), dict(rows=None), dict(rec=None), dict(out=None), dict(S=0), dict(d=0), dict(d=2049), dict(n=0), dict(n=5),
                dict(T=0), dict(fill=3), dict(state=P + 8), dict(S=1 << 20, n=1 << 20, T=1 << 20)):
        assert push(**bad) == INVALID, bad
    for args in ((None, 4, 5, None, 4), (P, 0, 5, None, 1), (P, 4, 0, None, 4), (P, 4, 5, None, 0), (P, 4, 5, None, 5), (P + 8, 4, 5, None, 4)):
        assert lib.mtadgat_prep_stream_reset(*args, None) == INVALID, args


def test_scratch_queries_are_consistent(lib):
    rb = lib.mtadgat_prep_rows_per_block()
    for n, d in ((0, 5), (1 << 31, 5), (10, 0), (10, 2049)):
        assert lib.mtadgat_prep_fit_scratch(n, d) == 0
        assert lib.mtadgat_prep_transform_scratch(n, d, 2, 0) == 0
    assert lib.mtadgat_prep_transform_scratch(10, 5, 3, 0) == 0
    for fill in (0, 1):
        assert lib.mtadgat_prep_transform_scratch(5000, 38, fill, 0) == 0       # one pass, no scratch
        assert lib.mtadgat_prep_transform_scratch(5000, 38, fill, 1) == lib.mtadgat_prep_transform_scratch(5000, 38, 2, 0)
    last_fit = last_scan = 0
    for n in (1, rb, rb + 1, 2 * rb + 70, 1 << 20):
        blocks = (n + rb - 1) // rb
        fit, scan = lib.mtadgat_prep_fit_scratch(n, 38), lib.mtadgat_prep_transform_scratch(n, 38, 2, 1)
        assert fit >= blocks * 38 * 20 and scan >= blocks * 38 * 12              # (sum, lo, hi, count) and (flags, value, age) per cell
        assert fit <= blocks * 38 * 20 + 64 and scan <= blocks * 38 * 12 + 64
        assert fit >= last_fit and scan >= last_scan
        last_fit, last_scan = fit, scan
    assert lib.mtadgat_prep_fit_scratch((1 << 31) - 1, 2048) > 1 << 32              # size_t, not int


# ---- the specification against sklearn ------------------------------------------------------------------------------------------
def _raw(n, d, seed, gap_share=0.08):
    """raw telemetry with NaN gaps: columns of different offsets and spreads, a constant column and one whose range is below 10 eps32"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.1, 50.0, d) + rng.uniform(-100.0, 100.0, d)).astype(np.float32)
    x[:, 1] = np.float32(3.25)
    x[:, 2] = np.float32(1.0) + np.float32(2.0 ** -23) * rng.integers(0, 2, n).astype(np.float32)      # range 2^-23 < 10 eps32
    x[rng.random((n, d)) < gap_share] = np.nan
    return x


def test_zero_policy_is_the_reference_bit_for_bit():
    from sklearn.preprocessing import MinMaxScaler
    train, test = _raw(700, 9, 1), _raw(500, 9, 2)
    assert np.isnan(train).any() and np.isnan(test).any()
    sk = MinMaxScaler().fit(np.nan_to_num(train))
    want = sk.transform(np.nan_to_num(test))
    assert want.dtype == np.float32 and sk.scale_.dtype == np.float32
    rec = prep_refs.fit(train, gaps="zero")
    assert rec["scale"][1] == 1.0 or np.isnan(train[:, 1]).any()           # (a gap counted as 0.0 widens the constant column's range)
    _same_bits(rec["scale"], sk.scale_, "scale_")
    _same_bits(rec["offset"], sk.min_, "min_")
    _same_bits(rec["lo"], sk.data_min_, "data_min_")
    _same_bits(rec["hi"], sk.data_max_, "data_max_")
    _same_bits(prep_refs.transform(test, rec, "zero"), want, "transform")
    # and without a gap in the training series: the constant and the tiny-range column take scale 1
    clean = _raw(300, 9, 3, gap_share=0.0)
    sk = MinMaxScaler().fit(clean)
    rec = prep_refs.fit(clean, gaps="zero")
    assert rec["scale"][1] == 1.0 and rec["scale"][2] == 1.0 and rec["hi"][2] > rec["lo"][2]
    _same_bits(rec["scale"], sk.scale_, "scale_ (clean)")
    _same_bits(rec["offset"], sk.min_, "min_ (clean)")
    _same_bits(prep_refs.transform(test, rec, "zero"), sk.transform(np.nan_to_num(test)), "transform (clean)")


def test_ignore_policy_is_sklearn_on_data_with_nans():
    from sklearn.preprocessing import MinMaxScaler
    train = _raw(700, 9, 4)
    sk = MinMaxScaler().fit(train)
    rec = prep_refs.fit(train, gaps="ignore")
    _same_bits(rec["lo"], sk.data_min_, "data_min_")
    _same_bits(rec["hi"], sk.data_max_, "data_max_")
    _same_bits(rec["scale"], sk.scale_, "scale_")
    _same_bits(rec["offset"], sk.min_, "min_")
    assert rec["scale"][1] == 1.0 and rec["scale"][2] == 1.0
    assert np.array_equal(rec["n_valid"], (~np.isnan(train)).sum(axis=0))
    _same_bits(prep_refs.transform(train, rec, None), sk.transform(train), "transform keeps the NaNs")


# ---- hand-written hold / age cases ------------------------------------------------------------------------------------------------
NAN, INF = np.nan, np.inf
HAND = np.array([[NAN, 1.0], [2.0, NAN], [NAN, -INF], [NAN, 4.0], [6.0, NAN], [INF, NAN], [NAN, NAN], [10.0, 8.0]], np.float32)
UNIT = dict(lo=np.zeros(2, np.float32), hi=np.ones(2, np.float32), scale=np.ones(2, np.float32), offset=np.zeros(2, np.float32),
            mean=np.array([-1.0, -2.0], np.float32), n_valid=np.array([3, 3], np.int32))


def test_hold_and_age_by_hand():
    got = prep_refs.transform(HAND, UNIT, "hold")
    assert got.tolist() == [[-1.0, 1.0], [2.0, 1.0], [2.0, 1.0], [2.0, 4.0], [6.0, 4.0], [6.0, 4.0], [6.0, 4.0], [10.0, 8.0]]
    assert prep_refs.age(HAND).tolist() == [[1, 0], [0, 1], [1, 2], [2, 0], [0, 1], [1, 2], [2, 3], [0, 0]]
    # parts of 3, 0, 2 and 3 rows: nothing crosses a seam, a part that starts in a gap takes the mean and counts from its first row
    lengths = [3, 0, 2, 3]
    got = prep_refs.transform(HAND, UNIT, "hold", lengths=lengths)
    assert got.tolist() == [[-1.0, 1.0], [2.0, 1.0], [2.0, 1.0], [-1.0, 4.0], [6.0, 4.0], [-1.0, -2.0], [-1.0, -2.0], [10.0, 8.0]]
    assert prep_refs.age(HAND, lengths).tolist() == [[1, 0], [0, 1], [1, 2], [1, 0], [0, 1], [1, 1], [2, 2], [0, 0]]
    zero = prep_refs.transform(HAND, UNIT, "zero")
    assert zero.tolist() == np.where(np.isfinite(HAND), HAND, 0.0).tolist()
    none = prep_refs.transform(HAND, UNIT, None)
    assert np.array_equal(np.isnan(none), ~np.isfinite(HAND))
    rec = dict(UNIT, scale=np.array([0.25, 2.0], np.float32), offset=np.array([-0.5, 0.5], np.float32))
    assert prep_refs.transform(HAND, rec, "hold", clip=True).tolist() == [[0.0, 1.0], [0.0, 1.0], [0.0, 1.0], [0.0, 1.0], [1.0, 1.0], [1.0, 1.0],
                                                                          [1.0, 1.0], [1.0, 1.0]]
    for fill in ("hold", "zero", None):
        y, a = prep_refs.stream_replay(HAND, rec, fill)
        _same_bits(y, prep_refs.transform(HAND, rec, fill), fill)
        assert np.array_equal(a, prep_refs.age(HAND))


def test_fit_by_hand():
    rec = prep_refs.fit(HAND, gaps="ignore")
    assert rec["lo"].tolist() == [2.0, 1.0] and rec["hi"].tolist() == [10.0, 8.0] and rec["n_valid"].tolist() == [3, 3]
    assert rec["mean"].tolist() == [6.0, np.float32(13.0 / 3.0)]
    assert rec["scale"].tolist() == [0.125, np.float32(1.0) / np.float32(7.0)]
    rec = prep_refs.fit(HAND, gaps="zero")
    assert rec["lo"].tolist() == [0.0, 0.0] and rec["n_valid"].tolist() == [8, 8] and rec["mean"].tolist() == [2.25, 1.625]
    empty = prep_refs.fit(np.full((4, 1), NAN, np.float32))
    assert [empty[k][0] for k in prep_refs.FIELDS] == [0.0, 0.0, 1.0, 0.0, 0.0, 0]
    back = prep_refs.inverse(prep_refs.transform(HAND, rec, "zero"), rec)
    assert np.allclose(back, np.where(np.isfinite(HAND), HAND, 0.0), rtol=1e-6)


# ---- the CPU route -------------------------------------------------------------------------------------------------------------------
def _planted(n, d, seed):
    x = _raw(n, d, seed)
    x[0, :] = np.nan
    x[n // 3:n // 3 + 40, 0] = np.inf
    x[:, 3] = np.nan                                   # a column that is all gap
    x[-1, 4] = -np.inf
    return x


@pytest.mark.parametrize("gaps", ["ignore", "zero"])
def test_cpu_route_is_the_specification(gaps):
    import preparation
    train, test = _planted(600, 7, 5), _planted(450, 7, 6)
    lengths = [100, 0, 217, 133]
    scaler = preparation.fit_scaler(torch.from_numpy(train), gaps=gaps)
    rec, got = prep_refs.fit(train, gaps), scaler.read()
    for k in prep_refs.FIELDS[:5]:
        _same_bits(got[k], rec[k], k)
    assert np.array_equal(got["n_valid"], rec["n_valid"]) and got["n_valid"].dtype == np.int32
    for fill in ("zero", "hold", None):
        for clip in (False, True):
            for ls in (None, lengths):
                y, a = scaler.transform(torch.from_numpy(test), fill=fill, clip=clip, lengths=ls, return_age=True)
                _same_bits(y.numpy(), prep_refs.transform(test, rec, fill, clip, ls), (fill, clip, ls))
                assert a.dtype == torch.int32 and np.array_equal(a.numpy(), prep_refs.age(test, ls))
    y = scaler.transform(torch.from_numpy(test), fill="hold")
    _same_bits(scaler.inverse(y).numpy(), prep_refs.inverse(y.numpy(), rec), "inverse")
    dims = [4, 0, 6]
    _same_bits(scaler.inverse(y[:, dims], dims=dims).numpy(), prep_refs.inverse(y.numpy()[:, dims], rec, dims), "inverse with dims")
    work = torch.from_numpy(test.copy())
    assert scaler.transform(work, fill="hold", out=work) is work
    _same_bits(work.numpy(), y.numpy(), "in place")


def test_scaler_state_round_trip_and_errors():
    import preparation
    train = _planted(200, 7, 7)
    scaler = preparation.fit_scaler(torch.from_numpy(train))
    again = preparation.SeriesScaler.from_state(scaler.state_dict())
    assert again.gaps == "ignore" and torch.equal(again.record.view(torch.int32), scaler.record.view(torch.int32))
    assert scaler.to("cpu") is scaler and scaler.n_columns == 7
    one = preparation.fit_scaler(torch.from_numpy(train[:, 0]))
    assert one.n_columns == 1 and one.transform(torch.from_numpy(train[:, 0])).shape == (200,)
    with pytest.raises(ValueError):
        preparation.fit_scaler(torch.from_numpy(train), gaps="mean")
    with pytest.raises(ValueError):
        scaler.transform(torch.from_numpy(train), fill="linear")
    with pytest.raises(ValueError):
        scaler.transform(torch.from_numpy(train), lengths=[100, 99])
    with pytest.raises(ValueError):
        scaler.transform(torch.from_numpy(train[:, :3]))
    with pytest.raises(ValueError):
        scaler.inverse(torch.zeros(4, 2), dims=[0, 7])
    with pytest.raises(RuntimeError):
        preparation.StreamPreparer(scaler, 4)                # GPU only


def test_a_single_row_is_handed_on_in_place_with_a_legal_row_stride():
    """_rows2d: a (1, d) input whose elements are contiguous is not copied -- it is re-viewed with row stride d, whatever stride torch
    gave its one row (a row of a wider tensor, a row stride of 0 or 1) --, so its first element keeps its address; a single row whose
    elements are strided is copied.  The values are the row's in every case."""
    import preparation
    wide = torch.arange(40, dtype=torch.float32).reshape(4, 10)
    cases = [wide[2:3, 3:8], wide[1:2], torch.arange(5.0).as_strided((1, 5), (0, 1)), torch.arange(5.0).as_strided((1, 5), (1, 1)),
             wide[3:4, 9:10], wide[0:1, ::3][:, :1], wide[0, 2:6]]
    for t in cases:
        got = preparation._rows2d(t, "t")
        want = t.reshape(-1, 1) if t.ndim == 1 else t
        assert got.shape == want.shape and torch.equal(got, want)
        if t.ndim == 2:
            assert got.data_ptr() == t.data_ptr() and got.stride() == (t.shape[1], 1), (t.shape, t.stride(), got.stride())
    strided = wide[0:1, ::3]                                            # (1, 4), elements 3 apart: copied
    got = preparation._rows2d(strided, "t")
    assert torch.equal(got, strided) and got.data_ptr() != strided.data_ptr() and got.stride() == (4, 1)
    multi = wide[:, 2:5]                                                # more than one row: as before, no copy
    assert preparation._rows2d(multi, "t").data_ptr() == multi.data_ptr()
