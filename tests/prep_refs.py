"""The specification of the preparation step (preparation.py, csrc/mtadgat_prep.hip) in numpy: the per-column min-max scaler, the gap
fills, the age, the inverse and a row-at-a-time replay of a live stream.  No library call and no GPU.

A gap is a sample that is not finite.  All scaler arithmetic is float32 with every operation rounded on its own -- numpy's float32
array operations -- which is what sklearn's MinMaxScaler computes on float32 input (tests/test_host_prep.py checks the bits)."""
import math

import numpy as np

EPS32 = np.finfo(np.float32).eps
FIELDS = ("lo", "hi", "scale", "offset", "mean", "n_valid")


def valid(x):
    return np.isfinite(x)


def derive(lo, hi):
    """(scale, offset) from float32 lo / hi: range = hi - lo; scale = 1 / (range < 10 eps32 ? 1 : range); offset = 0 - lo scale"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    rng = hi - lo
    rng = np.where(rng < np.float32(10) * EPS32, np.float32(1), rng).astype(np.float32)
    scale = (np.float32(1) / rng).astype(np.float32)
    offset = (np.float32(0) - lo * scale).astype(np.float32)
    return scale, offset


def fit(x, gaps="ignore"):
    """The record of every column of the (n, d) float32 array x as a dict of (d,) arrays.  gaps="ignore": gaps are left out;
    "zero": a gap is the sample 0.0.  mean: the exactly rounded sum (math.fsum) of the samples, divided once in float64 and
    rounded once to float32.  A column without a sample: lo = hi = mean = 0."""
    x = np.asarray(x, np.float32)
    ok = valid(x)
    if gaps == "zero":
        x = np.where(ok, x, np.float32(0))
        ok = np.ones_like(ok)
    elif gaps != "ignore":
        raise ValueError(gaps)
    d = x.shape[1]
    lo, hi, mean = np.zeros(d, np.float32), np.zeros(d, np.float32), np.zeros(d, np.float32)
    n_valid = ok.sum(axis=0).astype(np.int32)
    for c in range(d):
        v = x[ok[:, c], c]
        if v.size:
            lo[c], hi[c] = v.min(), v.max()
            mean[c] = np.float32(math.fsum(v.astype(np.float64).tolist()) / v.size)
    scale, offset = derive(lo, hi)
    return dict(lo=lo, hi=hi, scale=scale, offset=offset, mean=mean, n_valid=n_valid)


def _spans(n, lengths):
    offs = np.concatenate(([0], np.cumsum([n] if lengths is None else lengths))).astype(np.int64)
    assert offs[-1] == n
    return list(zip(offs[:-1], offs[1:]))


def last_valid(x, lengths=None):
    """(last, start): per sample the row of the last valid sample of its column at or before it within its part (-1: none), and
    per row the first row of its part"""
    x = np.asarray(x, np.float32)
    n, d = x.shape
    last = np.full((n, d), -1, np.int64)
    start = np.zeros(n, np.int64)
    for s, e in _spans(n, lengths):
        if e > s:
            rows = np.arange(s, e, dtype=np.int64)[:, None]
            last[s:e] = np.maximum.accumulate(np.where(valid(x[s:e]), rows, -1), axis=0)
            start[s:e] = s
    return last, start


def age(x, lengths=None):
    """int32 (n, d): 0 at a valid sample, k at the k-th consecutive gap row since the last valid one, i - part_start + 1 where the
    part has no valid sample yet"""
    last, start = last_valid(x, lengths)
    rows = np.arange(x.shape[0], dtype=np.int64)[:, None]
    return np.where(last >= 0, rows - last, rows - start[:, None] + 1).astype(np.int32)


def transform(x, rec, fill, clip=False, lengths=None):
    """fl(fl(v scale) + offset), v = x or the fill of a gap: "zero" 0.0, "hold" the last valid raw value of the column in the part
    (the column's mean when there is none yet), None NaN"""
    x = np.asarray(x, np.float32)
    ok = valid(x)
    if fill == "hold":
        last, _ = last_valid(x, lengths)
        held = np.take_along_axis(x, np.maximum(last, 0), axis=0)
        v = np.where(ok, x, np.where(last >= 0, held, rec["mean"][None, :]))
    elif fill == "zero":
        v = np.where(ok, x, np.float32(0))
    elif fill is None:
        v = np.where(ok, x, np.float32(np.nan))
    else:
        raise ValueError(fill)
    v = v.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (v * rec["scale"][None, :]).astype(np.float32)
        y = (y + rec["offset"][None, :]).astype(np.float32)
    if clip:
        y = np.where(y < 0, np.float32(0), np.where(y > 1, np.float32(1), y)).astype(np.float32)
    return y


def inverse(y, rec, dims=None):
    """fl(fl(y - offset) / scale) with the record of column dims[j] for column j"""
    y = np.asarray(y, np.float32)
    cols = np.arange(y.shape[1]) if dims is None else np.asarray(dims)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return ((y - rec["offset"][cols][None, :]).astype(np.float32) / rec["scale"][cols][None, :]).astype(np.float32)


def stream_replay(rows, rec, fill, clip=False):
    """One stream's (n, d) raw rows prepared one row at a time from the state a live stream keeps per column -- the last valid raw
    value, whether there was one, the age: (prepared (n, d) float32, age (n, d) int32)"""
    rows = np.asarray(rows, np.float32)
    n, d = rows.shape
    has = np.zeros(d, bool)
    val = np.zeros(d, np.float32)
    run = np.zeros(d, np.int32)
    out = np.empty((n, d), np.float32)
    ages = np.empty((n, d), np.int32)
    for i in range(n):
        ok = valid(rows[i])
        has |= ok
        val = np.where(ok, rows[i], val)
        run = np.where(ok, 0, run + 1).astype(np.int32)
        if fill == "hold":
            v = np.where(ok, rows[i], np.where(has, val, rec["mean"]))
        elif fill == "zero":
            v = np.where(ok, rows[i], np.float32(0))
        else:
            v = np.where(ok, rows[i], np.float32(np.nan))
        with np.errstate(invalid="ignore", over="ignore"):
            y = ((v.astype(np.float32) * rec["scale"]).astype(np.float32) + rec["offset"]).astype(np.float32)
        if clip:
            y = np.where(y < 0, np.float32(0), np.where(y > 1, np.float32(1), y)).astype(np.float32)
        out[i], ages[i] = y, run
    return out, ages


def ulp32(v):
    """the spacing of float32 at |v| (float64 in, float64 out; the smallest normal's for tiny values)"""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), np.float64(np.finfo(np.float32).tiny))
    return 2.0 ** (np.floor(np.log2(a)) - 23)
