"""The preparation kernels (csrc/mtadgat_prep.hip through preparation.fit_scaler / SeriesScaler) against tests/prep_refs.py.

Sizes: with RB = mtadgat_prep_rows_per_block(), n in {1, 63, RB, 2 RB + 70} x d in {1, 38, 65}, plus (200, 2048); contiguous arrays
and a column slice of a wider array whose neighbours are poison.  Gaps sit where the blocked scan can go wrong (_planted): row 0, the
last row, a run across a block boundary, a block that is all gap between two valid ones, a part that is all gap, a column that is all
gap, +-inf; the parts start on a block boundary, inside a 64-row group, and one is empty.

Gates
  fit        lo, hi, n_valid exact; scale, offset the bits of the float32 replay (prep_refs.derive) of the device's lo / hi; mean
             within 1 float32 ulp of math.fsum's sum / n_valid; a second run gives the same bits.
  transform  the bits of prep_refs.transform with the device's own record (fill=None: NaN pattern and the bits elsewhere); age exact;
             in place == out of place; a second run gives the same bits.
  inverse    the bits of prep_refs.inverse, and the round trip bound of test_round_trip."""
import math

import numpy as np
import pytest
import torch

import prep_refs

pytestmark = pytest.mark.gpu

U = 2.0 ** -24               # float32 unit roundoff


@pytest.fixture(scope="module")
def RB():
    import preparation
    return preparation.rows_per_block()


def _sizes(RB):
    return [(n, d) for n in (1, 63, RB, 2 * RB + 70) for d in (1, 38, 65)] + [(200, 2048)]


def _lengths(n, RB):
    """parts whose starts lie inside a 64-row group (37), on a block boundary (RB) and mid-block, one of them empty"""
    cuts = [c for c in (37, RB, RB, RB + 100, 2 * RB + 5) if c < n]
    offs = [0] + cuts + [n]
    return [b - a for a, b in zip(offs[:-1], offs[1:])]


def _planted(n, d, RB, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.1, 50.0, d) + rng.uniform(-100.0, 100.0, d)).astype(np.float32)
    x[rng.random((n, d)) < 0.05] = np.nan
    x[rng.random((n, d)) < 0.01] = np.inf
    x[rng.random((n, d)) < 0.01] = -np.inf
    if n > 1:
        x[0, :] = np.nan                                               # row 0
        x[-1, d - 1] = np.nan                                          # the last row
    if n > RB + 2:
        x[RB - 3:RB + 3, 0] = np.nan                                   # a run across a block boundary
        x[RB:min(RB + 100, n), 0] = np.nan                             # a part that is all gap (column 0)
        x[RB - 70:RB, d // 2] = np.inf                                 # a run that ends with its block
    if n > 2 * RB:
        x[RB:2 * RB, min(1, d - 1)] = np.nan                           # a block that is all gap between two valid ones
    if d >= 3:
        x[:, 2] = np.nan                                               # a column that is all gap
    if d >= 5:
        x[:, 4] = np.float32(-3.5)                                     # a constant column
    return x


_DATA = {}


def _case(n, d, RB):
    key = (n, d)
    if key not in _DATA:
        _DATA[key] = (_planted(n, d, RB, 100 * n + d), _planted(n, d, RB, 100 * n + d + 1))
    return _DATA[key]


def _on_device(a, layout, device):
    n, d = a.shape
    if layout == "contiguous":
        return torch.from_numpy(a).to(device)
    wide = torch.full((n, d + 5), -7.0e6, device=device)              # the neighbours would change every lo if they were read
    wide[:, 2:2 + d] = torch.from_numpy(a).to(device)
    t = wide[:, 2:2 + d]
    assert n == 1 or t.stride(0) == d + 5
    return t


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), what


def _record_bits(scaler):
    return scaler.record.cpu().view(torch.int32)


@pytest.mark.parametrize("layout", ["contiguous", "sliced"])
@pytest.mark.parametrize("gaps", ["ignore", "zero"])
def test_fit(gaps, layout, RB, gpu_device):
    import preparation
    for n, d in _sizes(RB):
        train, _ = _case(n, d, RB)
        scaler = preparation.fit_scaler(_on_device(train, layout, gpu_device), gaps=gaps)
        got, ref = scaler.read(), prep_refs.fit(train, gaps)
        what = (n, d, gaps, layout)
        assert np.array_equal(got["lo"], ref["lo"]) and np.array_equal(got["hi"], ref["hi"]), what
        assert got["n_valid"].dtype == np.int32 and np.array_equal(got["n_valid"], ref["n_valid"]), what
        scale, offset = prep_refs.derive(got["lo"], got["hi"])
        _same_bits(got["scale"], scale, what + ("scale",))
        _same_bits(got["offset"], offset, what + ("offset",))
        ok = np.isfinite(train) if gaps == "ignore" else np.ones_like(train, bool)
        vals = np.where(np.isfinite(train), train, np.float32(0)).astype(np.float64)
        for c in range(d):
            k = int(ok[:, c].sum())
            want = math.fsum(vals[ok[:, c], c].tolist()) / k if k else 0.0
            assert abs(float(got["mean"][c]) - want) <= prep_refs.ulp32(want), what + (c, float(got["mean"][c]), want)
        again = preparation.fit_scaler(_on_device(train, layout, gpu_device), gaps=gaps)
        assert torch.equal(_record_bits(again), _record_bits(scaler)), what + ("two runs differ",)


@pytest.mark.parametrize("layout", ["contiguous", "sliced"])
@pytest.mark.parametrize("fill", ["zero", "hold", None])
def test_transform(fill, layout, RB, gpu_device):
    import preparation
    for n, d in _sizes(RB):
        train, test = _case(n, d, RB)
        scaler = preparation.fit_scaler(torch.from_numpy(train).to(gpu_device), gaps="ignore")
        rec = scaler.read()
        for lengths in (None, _lengths(n, RB)):
            for clip in (False, True):
                what = (n, d, fill, layout, lengths, clip)
                want = prep_refs.transform(test, rec, fill, clip, lengths)
                x = _on_device(test, layout, gpu_device)
                got, age = scaler.transform(x, fill=fill, clip=clip, lengths=lengths, return_age=True)
                _same_bits(got, want, what)
                assert age.dtype == torch.int32 and np.array_equal(age.cpu().numpy(), prep_refs.age(test, lengths)), what + ("age",)
                plain = scaler.transform(x, fill=fill, clip=clip, lengths=lengths)            # without the age: fill zero / None take one pass
                _same_bits(plain, want, what + ("no age",))
                again = scaler.transform(x, fill=fill, clip=clip, lengths=lengths)
                assert torch.equal(again.view(torch.int32), plain.view(torch.int32)), what + ("two runs differ",)
                work = _on_device(test, layout, gpu_device)
                assert scaler.transform(work, fill=fill, clip=clip, lengths=lengths, out=work) is work
                _same_bits(work.contiguous(), want, what + ("in place",))
                if layout == "sliced":
                    base = work._base
                    assert bool((base[:, :2] == -7.0e6).all()) and bool((base[:, 2 + d:] == -7.0e6).all()), what + ("neighbours written",)
                wide = torch.zeros(n, d + 3, device=gpu_device)                                 # ld_out differs from ld
                scaler.transform(x, fill=fill, clip=clip, lengths=lengths, out=wide[:, :d])
                _same_bits(wide[:, :d].contiguous(), want, what + ("ld_out",))
                assert bool((wide[:, d:] == 0).all()), what


def test_gaps_zero_record_transforms_like_the_reference(RB, gpu_device):
    """fit(gaps="zero") + transform(fill="zero"): the reference's normalize_data, whose bits tests/test_host_prep.py pins to sklearn's"""
    import preparation
    n, d = 2 * RB + 70, 38
    train, test = _case(n, d, RB)
    scaler = preparation.fit_scaler(torch.from_numpy(train).to(gpu_device), gaps="zero")
    ref = prep_refs.fit(train, "zero")
    got = scaler.read()
    for k in ("lo", "hi", "scale", "offset"):
        _same_bits(got[k], ref[k], k)
    _same_bits(scaler.transform(torch.from_numpy(test).to(gpu_device), fill="zero"), prep_refs.transform(test, ref, "zero"), "transform")


@pytest.mark.parametrize("layout", ["contiguous", "sliced"])
def test_round_trip(layout, RB, gpu_device):
    """inverse(transform(x)) against x on the valid samples of non-constant columns.

    With u = 2^-24 and every operation rounded on its own, a = x s (1 + d1), y = (a + o)(1 + d2), b = (y - o)(1 + d3),
    x' = (b / s)(1 + d4), |d_i| <= u.  The same float32 o is added and subtracted, so y - o = a + (a + o) d2 and, to first order,
        x' - x = x (d1 + d3 + d4) + ((a + o) / s) d2,       |(a + o) / s| <= |x - lo| + u (|x| + |lo|)
    (o = fl(-lo s)).  Hence |x' - x| <= u (3 |x| + |x - lo|) (1 + 2^-10), the last factor covering the second-order terms.  u |x| is at
    most one float32 ulp of x, so the first part is the "few ulps of x" one expects -- but the second part is an ulp of the column's
    RANGE, not of x: a sample near zero in a column that spans +-100 comes back with the absolute error of its scaled value.  The
    2-ulp-of-x bound therefore cannot hold on such columns: the float32 numpy replay of the specification alone (no kernel involved)
    misses it on this test's data -- 9 % of the samples come back more than 2 ulp32 of x away, the worst 1.2e5 ulp32 of x (a sample near
    zero), 0.975 of the derived bound; the test prints both figures -- so the gate is the derived bound, and the kernels' results are the
    replay's bit for bit."""
    import preparation
    worst_ulps = worst_bound = 0.0
    for n, d in _sizes(RB):
        train, test = _case(n, d, RB)
        scaler = preparation.fit_scaler(torch.from_numpy(train).to(gpu_device), gaps="ignore")
        rec = scaler.read()
        x = _on_device(test, layout, gpu_device)
        y = scaler.transform(x, fill=None)
        back = scaler.inverse(y)
        replay = prep_refs.inverse(prep_refs.transform(test, rec, None), rec)
        _same_bits(back, replay, (n, d, layout, "inverse"))
        dims = list(range(d - 1, -1, -2))
        _same_bits(scaler.inverse(y[:, dims], dims=dims), np.ascontiguousarray(replay[:, dims]), (n, d, layout, "inverse with dims"))
        live = np.isfinite(test) & (rec["hi"] > rec["lo"])[None, :]
        if not live.any():
            continue
        x64 = test.astype(np.float64)
        err = np.abs(replay.astype(np.float64) - x64)[live]
        bound = (U * (3.0 * np.abs(x64) + np.abs(x64 - rec["lo"].astype(np.float64)[None, :])) * (1.0 + 2.0 ** -10))[live]
        worst_ulps = max(worst_ulps, float((err / prep_refs.ulp32(x64[live])).max()))
        worst_bound = max(worst_bound, float((err / bound).max()))
        got_err = np.abs(back.cpu().numpy().astype(np.float64) - x64)[live]
        assert np.all(got_err <= bound), (n, d, layout, float((got_err / bound).max()))
    print(f"round trip of the float32 replay: at most {worst_ulps:.2f} ulp32 of x, {worst_bound:.3f} of the derived bound")


def test_value_errors(RB, gpu_device):
    import preparation
    train, _ = _case(63, 38, RB)
    scaler = preparation.fit_scaler(torch.from_numpy(train).to(gpu_device))
    x = torch.from_numpy(train).to(gpu_device)
    with pytest.raises(RuntimeError):
        scaler.transform(torch.from_numpy(train))                     # the scaler lives on the GPU
    with pytest.raises(ValueError):
        scaler.transform(x, lengths=[60, 2])
    with pytest.raises(ValueError):
        scaler.transform(x, out=torch.empty(63, 37, device=gpu_device))
    moved = scaler.to("cpu")
    assert moved.device.type == "cpu" and torch.equal(moved.record.view(torch.int32), scaler.record.cpu().view(torch.int32))
    _same_bits(moved.transform(torch.from_numpy(train), fill="hold"), scaler.transform(x, fill="hold").cpu().numpy(), "CPU route == kernels")
