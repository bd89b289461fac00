"""The per-part quantile and scaling entry points without a GPU: symbols, the threshold between the two routes, argument validation
before anything touches the device, the scratch bound; and the reference the GPU tests compare against (tests/part_scale_refs.py),
held against numpy."""
import ctypes

import numpy as np
import pytest

import part_refs
import part_scale_refs
import score_refs

PTR = 0x10000            # a non-null, 16-byte aligned "device pointer": validation fails before it would be used


@pytest.fixture(scope="module")
def lib():
    import evaluation
    return evaluation._lib()


def _err(lib):
    return lib.mtadgat_last_error().decode()


def test_symbols_are_exported(lib):
    for name in ("mtadgat_eval_part_quantiles", "mtadgat_eval_part_quantiles_scratch", "mtadgat_eval_partq_long", "mtadgat_eval_part_scale"):
        assert hasattr(lib, name), name
    L = lib.mtadgat_eval_partq_long()
    assert L > 0 and L % 1024 == 0


def _quantiles(lib, a=PTR, n=100, d=4, ld=4, start=PTR, end=PTR, count=3, q=(0.25, 0.5), nq=None, scratch=PTR, scratch_bytes=None, out=PTR):
    qa = (ctypes.c_double * max(len(q), 1))(*q)
    nq = len(q) if nq is None else nq
    if scratch_bytes is None:
        scratch_bytes = max(lib.mtadgat_eval_part_quantiles_scratch(n, d, count, nq), 1 << 20)
    return lib.mtadgat_eval_part_quantiles(a, n, d, ld, start, end, count, qa, nq, scratch, scratch_bytes, out, None)


QUANTILE_BAD = {
    "null a": (dict(a=None), -1), "null start": (dict(start=None), -1), "null end": (dict(end=None), -1),
    "null scratch": (dict(scratch=None), -1), "null out": (dict(out=None), -1),
    "n < 1": (dict(n=0), -1), "n > 2^31 - 1": (dict(n=2 ** 31), -1), "d < 1": (dict(d=0), -1), "d > 2048": (dict(d=2049, ld=2049), -1),
    "count < 1": (dict(count=0), -1), "count > 2^31 - 1": (dict(count=2 ** 31), -1), "ld < d": (dict(ld=3), -1),
    "nq < 1": (dict(nq=0), -1), "nq > 8": (dict(q=(0.5,) * 9), -1),
    "q < 0": (dict(q=(0.5, -0.01)), -1), "q > 1": (dict(q=(1.0000001,)), -1), "q nan": (dict(q=(float("nan"),)), -1),
    "scratch one byte short": (dict(scratch_bytes=-1), -5), "misaligned scratch": (dict(scratch=PTR + 8), -5),
}


@pytest.mark.parametrize("case", list(QUANTILE_BAD))
def test_part_quantiles_rejects_invalid_arguments(lib, case):
    kw, status = QUANTILE_BAD[case]
    kw = dict(kw)
    if kw.get("scratch_bytes") == -1:
        kw["scratch_bytes"] = lib.mtadgat_eval_part_quantiles_scratch(100, 4, 3, 2) - 1
    assert _quantiles(lib, **kw) == status
    assert _err(lib)


def test_part_quantiles_rejects_null_q(lib):
    assert lib.mtadgat_eval_part_quantiles(PTR, 100, 4, 4, PTR, PTR, 3, None, 2, PTR, 1 << 20, PTR, None) == -1
    assert "null" in _err(lib)


SCALE_BAD = {"null a": dict(a=None), "null start": dict(start=None), "null end": dict(end=None), "null q": dict(q=None),
             "null out": dict(out=None), "n < 1": dict(n=0), "n > 2^31 - 1": dict(n=2 ** 31), "d < 1": dict(d=0), "d > 2048": dict(d=2049, ld=2049, ld_out=2049),
             "count < 1": dict(count=0), "ld < d": dict(ld=3), "ld_out < d": dict(ld_out=3)}


@pytest.mark.parametrize("case", list(SCALE_BAD))
def test_part_scale_rejects_invalid_arguments(lib, case):
    kw = dict(a=PTR, n=100, d=4, ld=4, start=PTR, end=PTR, count=3, q=PTR, out=PTR, ld_out=4)
    kw.update(SCALE_BAD[case])
    assert lib.mtadgat_eval_part_scale(kw["a"], kw["n"], kw["d"], kw["ld"], kw["start"], kw["end"], kw["count"], kw["q"], kw["out"],
                                       kw["ld_out"], None) == -1
    assert _err(lib)


def test_scratch_query(lib):
    sq = lib.mtadgat_eval_part_quantiles_scratch
    assert sq(1, 1, 1, 1) > 0
    for bad in ((0, 4, 3, 2), (2 ** 31, 4, 3, 2), (100, 0, 3, 2), (100, 2049, 3, 2), (100, 4, 0, 2), (100, 4, 2 ** 31, 2), (100, 4, 3, 0),
                (100, 4, 3, 9)):
        assert sq(*bad) == 0, bad
    L = lib.mtadgat_eval_partq_long()
    assert sq(L, 38, 10, 3) < sq(L + 1, 38, 10, 3) <= sq(1 << 24, 38, 10, 3)        # bins only where a part can be long
    assert sq(1 << 20, 38, 10, 3) < sq(1 << 20, 38, 1000, 3) and sq(1 << 20, 38, 10, 2) < sq(1 << 20, 38, 10, 3)
    assert sq(1 << 20, 7, 10, 3) < sq(1 << 20, 8, 10, 3)


def test_scratch_is_bounded_by_a_fraction_of_the_input(lib):
    """Bins and select state exist per slot of L rows, (n / L + 1) d 2 nq (1024 + 8) bytes: at nq = 3 and L = 16 384 that is
    0.38 n d bytes, below the eighth of the input's 4 n d bytes this asks for whenever L >= 12 384 nq / 3.  Per (part, column,
    probability) there are two float32 order statistics, and per (part, column) one 4-byte NaN flag: c = 8 + 4 = 12 covers both."""
    sq = lib.mtadgat_eval_part_quantiles_scratch
    c = 12
    for n, d, count, nq in (((1 << 24), 55, 1024, 3), ((1 << 24), 1, 1024, 3), ((1 << 20), 38, 1024, 3), ((1 << 24), 55, 1, 3),
                            (73629, 1, 27, 3), (5000, 38, 1 << 20, 3)):
        need = sq(n, d, count, nq)
        assert 0 < need < n * d * 4 // 8 + c * count * d * nq + 64, (n, d, count, nq, need)
    # what the whole-column layout would take with a part dimension: 1 KiB per (part, column, rank)
    assert 20 * sq(1 << 20, 55, 1 << 14, 3) < (1 << 14) * 55 * 6 * 1024


def test_reference_quantiles_equal_numpy_percentile_per_slice():
    rng = np.random.default_rng(21)
    qs = [0.0, 0.25, 0.5, 0.75, 1.0, 0.3333, 0.9]
    W = 5
    lengths = part_scale_refs.lengths_of([0, 1, 2, 3, 255, 256, 257, 0, 4099, 0], W)
    n = sum(lengths) - W
    a = score_refs.columns(n, 4, rng)              # every kind but the column with an inf
    got = part_scale_refs.quantiles(a, lengths, W, qs)
    start, end = part_refs.spans(lengths, W)
    assert got.shape == (len(qs), len(lengths), 4)
    for p, (s, e) in enumerate(zip(start, end)):
        if e == s:
            assert np.isnan(got[:, p]).all(), p
            continue
        ref = np.percentile(a[s:e].astype(np.float64), [100.0 * q for q in qs], axis=0, method="linear")
        assert np.all(np.abs(got[:, p] - ref) <= score_refs.ulp32(ref)), (p, np.abs(got[:, p] - ref).max())
    b = a.copy()
    b[start[5] + 7, 1] = np.nan                    # one (part, column)
    got = part_scale_refs.quantiles(b, lengths, W, qs)
    nan = np.isnan(got)
    assert nan[:, 5, 1].all() and nan.sum() == len(qs) * (1 + 4 * 4)      # that one and the four empty parts
    one = part_scale_refs.quantiles(a[:, 0], lengths, W, qs)
    assert np.array_equal(one[:, :, 0], part_scale_refs.quantiles(a, lengths, W, qs)[:, :, 0], equal_nan=True)


def test_reference_scale_is_float32_arithmetic_per_part():
    rng = np.random.default_rng(22)
    W = 3
    lengths = part_scale_refs.lengths_of([40, 0, 1, 300], W)
    n = sum(lengths) - W
    a = (rng.random((n, 3)) * 3.0).astype(np.float32)
    a[40:] *= 100.0                                                        # a noisy part must not set the scale of the quiet one
    q3 = part_scale_refs.quantiles(a, lengths, W, [0.25, 0.5, 0.75]).astype(np.float32)
    got = part_scale_refs.scale(a, q3, lengths, W)
    assert got.dtype == np.float32 and got.shape == a.shape
    for p, (s, e) in enumerate(zip(*part_refs.spans(lengths, W))):
        for i in range(s, e):
            for c in range(3):
                want = np.float32(np.float32(a[i, c] - q3[1, p, c]) / np.float32(np.float32(1) + np.float32(q3[2, p, c] - q3[0, p, c])))
                assert got[i, c] == want
    q25, med, q75 = np.percentile(a[:40].astype(np.float64), [25, 50, 75], axis=0)
    assert np.abs(got[:40] - (a[:40] - med) / (1 + (q75 - q25))).max() <= 1e-6
    assert np.array_equal(part_scale_refs.scale(a[:, 0], q3[:, :, :1], lengths, W), got[:, 0])


def test_layouts_cover_the_threshold_between_the_routes():
    L = 16384
    lay = part_scale_refs.layouts(L)
    every = sorted({v for ls in lay.values() for v in ls})
    for v in (0, 1, 2, 3, 255, 256, 257, L - 1, L, L + 1):
        assert v in every, v
    assert len(lay["many"]) == 1024 and max(lay["many"]) <= 5
    assert max(sum(ls) for ls in lay.values()) <= 3 * L + 70
    assert (lay["unaligned_long"][0]) % L != 0
    for ls in lay.values():
        lengths = part_scale_refs.lengths_of(ls, 7)
        start, end = part_refs.spans(lengths, 7)
        assert (end - start).tolist() == [0] + list(ls)
