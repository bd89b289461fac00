"""The peaks-over-threshold entry points (csrc/mtadgat_spot.hip, csrc/mtadgat_spot.h) without a GPU: the symbols, every argument
refusal that happens before anything is launched, and mtadgat_spot_fit_host -- the fit's own statements compiled for the host, with
the sums taken in a wave's order -- against the numpy specification tests/spot_refs.py on seeded peak sets.

Gate of the fit (the only approximate comparison: libm's and numpy's log / pow may differ in the last bit, and bisection amplifies
that).  Per peak set, on the CPU: the float64 and the long-double runs of the reference must agree to 1e-10 relative on the
threshold (a condition on the seeded input: a set that fails it gets another seed, the bound stays); then the host hook's threshold
must lie within 1e-9 relative of the float64 reference -- that precondition with a factor ten -- and it must have chosen a
candidate of the same kind (gamma zero or of the same sign, gamma and sigma within 1e-7 relative).
"""
import ctypes

import numpy as np
import pytest
import torch

import spot_refs

PTR = 0x10000            # a non-null, 16-byte aligned "device pointer": validation fails before it would be used
_dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def lib():
    import evaluation
    import streaming
    streaming._lib()
    return evaluation._lib()


def _err(lib):
    return lib.mtadgat_last_error().decode()


def test_symbols_are_exported(lib):
    import evaluation
    import streaming
    for name in ("mtadgat_spot_state_bytes", "mtadgat_spot_calibrate_scratch", "mtadgat_spot_calibrate", "mtadgat_spot_run", "mtadgat_spot_read",
                 "mtadgat_spot_copy", "mtadgat_spot_fit_host", "mtadgat_stream_push_spot", "mtadgat_stream_update_spot",
                 "mtadgat_stream_reset_spot"):
        assert hasattr(lib, name), name
    for name in ("spot_calibrate", "spot_run", "pot_eval", "SpotState"):
        assert hasattr(evaluation, name), name
    assert callable(streaming.StreamScorer.spot_state)
    assert lib.mtadgat_abi_version() == 1


def test_size_queries(lib):
    sb, cs = lib.mtadgat_spot_state_bytes, lib.mtadgat_spot_calibrate_scratch
    assert sb(0, 64) == 0 and sb(3, 7) == 0 and sb(3, 4097) == 0 and sb(1 << 31, 64) == 0
    assert sb(3, 8) >= 3 * (6 * 8 + 8 * 8) and sb(3, 8) % 16 == 0
    assert sb(4, 8) - sb(3, 8) == sb(3, 8) - sb(2, 8) and sb(3, 9) - sb(3, 8) == 3 * 8
    assert cs(15, 3) == 0 and cs(16, 0) == 0 and cs(16, 65537) == 0 and cs(16, 3) > 0


CALIBRATE_BAD = {"q = 0": dict(q=0.0), "q = 1": dict(q=1.0), "q NaN": dict(q=float("nan")), "q < 0": dict(q=-0.1),
                 "level = 0": dict(level=0.0), "level = 1": dict(level=1.0), "level NaN": dict(level=float("nan")),
                 "max_peaks 7": dict(P=7), "max_peaks 4097": dict(P=4097), "n_init 15": dict(n=15), "no columns": dict(S=0),
                 "too many columns": dict(S=65537), "null state": dict(state=None), "misaligned state": dict(state=PTR + 8),
                 "null scores": dict(init=None), "ld < columns": dict(ld=2)}


@pytest.mark.parametrize("case", list(CALIBRATE_BAD))
def test_calibrate_rejects_invalid_arguments(lib, case):
    kw = dict(init=PTR, n=200, S=3, ld=3, q=1e-3, level=0.9, P=64, state=PTR)
    kw.update(CALIBRATE_BAD[case])
    rc = lib.mtadgat_spot_calibrate(kw["init"], kw["n"], kw["S"], kw["ld"], kw["q"], kw["level"], kw["P"], 1, kw["state"], PTR, 1 << 30, None)
    assert rc == -1 and "spot_calibrate:" in _err(lib), (case, rc, _err(lib))


def test_calibrate_checks_its_scratch(lib):
    args = (PTR, 200, 3, 3, 1e-3, 0.9, 64, 1, PTR)
    need = lib.mtadgat_spot_calibrate_scratch(200, 3)
    assert lib.mtadgat_spot_calibrate(*args, None, need, None) == -5 and "scratch" in _err(lib)
    assert lib.mtadgat_spot_calibrate(*args, PTR + 4, need, None) == -5 and "scratch" in _err(lib)
    assert lib.mtadgat_spot_calibrate(*args, PTR, need - 1, None) == -5 and "too small" in _err(lib)


RUN_BAD = {"null state": dict(state=None), "misaligned state": dict(state=PTR + 8), "no columns": dict(S=0), "max_peaks 7": dict(P=7),
           "max_peaks 4097": dict(P=4097), "null scores": dict(scores=None), "no rows": dict(n=0), "ld < columns": dict(ld=2)}


@pytest.mark.parametrize("case", list(RUN_BAD))
def test_run_read_copy_reject_invalid_arguments(lib, case):
    kw = dict(state=PTR, S=3, P=64, scores=PTR, n=10, ld=3)
    kw.update(RUN_BAD[case])
    rc = lib.mtadgat_spot_run(kw["state"], kw["S"], kw["P"], kw["scores"], kw["n"], kw["ld"], None, None, None)
    assert rc == -1 and "spot_run:" in _err(lib), (case, rc, _err(lib))
    if case in ("null state", "misaligned state", "no columns", "max_peaks 7", "max_peaks 4097"):
        out = (ctypes.c_double * 18)()
        assert lib.mtadgat_spot_read(kw["state"], kw["S"], kw["P"], out, None) == -1 and "spot_read:" in _err(lib), case
        assert lib.mtadgat_spot_copy(kw["state"], kw["S"], PTR, 1, kw["P"], None, 1, 0, None) == -1 and "spot_copy:" in _err(lib), case
        assert lib.mtadgat_spot_copy(PTR, 3, kw["state"], kw["S"], kw["P"], None, 1, 0, None) == -1 and "spot_copy:" in _err(lib), case


def test_read_and_copy_reject_the_rest(lib):
    assert lib.mtadgat_spot_read(PTR, 3, 64, None, None) == -1 and "out is NULL" in _err(lib)
    assert lib.mtadgat_spot_copy(PTR, 3, PTR, 2, 64, None, 3, 0, None) == -1 and "one column" in _err(lib)
    assert lib.mtadgat_spot_copy(PTR, 3, PTR, 3, 64, None, 0, 0, None) == -1 and "n must" in _err(lib)
    assert lib.mtadgat_spot_copy(PTR, 3, PTR, 3, 64, None, 4, 0, None) == -1 and "n must" in _err(lib)
    assert lib.mtadgat_spot_copy(PTR, 3, PTR, 1, 64, PTR, 3, 1, None) == -1 and "new state" in _err(lib)
    assert lib.mtadgat_spot_copy(PTR, 3, PTR, 1, 64, None, 2, 1, None) == -1 and "new state" in _err(lib)


@pytest.fixture(scope="module")
def handle(lib):
    import _native
    cfg = _native.Config(n_features=3, window_size=5, out_dim=3, kernel_size=3, use_gatv2=1, feat_embed=6, time_embed=10, gru_n_layers=1,
                         gru_hid_dim=8, forecast_n_linear=2, forecast_hid_dim=8, recon_n_layers=1, recon_hid_dim=8, alpha=0.2)
    h = ctypes.c_void_p()
    assert lib.mtadgat_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    yield h
    lib.mtadgat_destroy(h)


STREAM_BAD = {"null handle": dict(h=None), "null state": dict(state=None), "n > n_streams": dict(n=4), "T > max_block": dict(T=6),
              "null SPOT state": dict(spot=None), "misaligned SPOT state": dict(spot=PTR + 8), "max_peaks 7": dict(P=7),
              "max_peaks 4097": dict(P=4097), "null rows": dict(rows=None)}


@pytest.mark.parametrize("case", list(STREAM_BAD))
def test_stream_entry_points_reject_invalid_arguments(lib, handle, case):
    import streaming
    kw = dict(h=handle, state=PTR, S=3, B=5, n=3, T=5, rows=PTR, spot=PTR, P=64)
    kw.update(STREAM_BAD[case])
    out = streaming._Outputs()
    ws = lib.mtadgat_stream_workspace_bytes(handle, 15)
    rc = lib.mtadgat_stream_push_spot(kw["h"], kw["state"], kw["S"], kw["B"], kw["rows"], None, kw["n"], kw["T"], kw["spot"], kw["P"], None,
                                      ctypes.byref(out), PTR, ws, None)
    assert rc == -1 and "stream_push_spot:" in _err(lib), (case, rc, _err(lib))
    rc = lib.mtadgat_stream_update_spot(kw["h"], kw["state"], kw["S"], kw["B"], PTR, PTR, kw["rows"], None, kw["n"], kw["T"], 0, kw["spot"],
                                        kw["P"], None, ctypes.byref(out), None)
    assert rc == -1 and "stream_update_spot:" in _err(lib), (case, rc, _err(lib))
    if case not in ("T > max_block", "null rows"):
        rc = lib.mtadgat_stream_reset_spot(kw["h"], kw["state"], kw["S"], kw["B"], kw["spot"], PTR, 1, kw["P"], None, kw["n"], None)
        assert rc == -1 and "stream_reset_spot:" in _err(lib), (case, rc, _err(lib))


def test_stream_reset_checks_the_calibrated_state(lib, handle):
    assert lib.mtadgat_stream_reset_spot(handle, PTR, 3, 5, PTR, None, 1, 64, None, 3, None) == -1 and "SPOT state" in _err(lib)
    assert lib.mtadgat_stream_reset_spot(handle, PTR, 3, 5, PTR, PTR, 2, 64, None, 3, None) == -1 and "one column" in _err(lib)
    ws = lib.mtadgat_stream_workspace_bytes(handle, 15)
    assert lib.mtadgat_stream_push_spot(handle, PTR, 3, 5, PTR, None, 3, 5, PTR, 64, None, None, PTR, ws - 1, None) == -5
    assert lib.mtadgat_stream_push_spot(handle, PTR, 3, 5, PTR, None, 3, 5, PTR, 64, None, None, PTR, ws, None) == -4     # no weights loaded


PY_BAD = {"q = 0": dict(q=0.0), "q = 1": dict(q=1.0), "level = 0": dict(level=0.0), "level = 1": dict(level=1.0), "max_peaks 7": dict(max_peaks=7),
          "max_peaks 4097": dict(max_peaks=4097), "fractional max_peaks": dict(max_peaks=64.5)}


@pytest.mark.parametrize("case", list(PY_BAD))
def test_python_validates_before_it_needs_a_device(case):
    import evaluation
    with pytest.raises(ValueError):
        evaluation.spot_calibrate(torch.rand(200), **PY_BAD[case])


def test_cpu_scores_are_refused_naming_the_gpu():
    import evaluation
    with pytest.raises(RuntimeError, match="GPU"):
        evaluation.spot_calibrate(torch.rand(200))
    with pytest.raises(TypeError):
        evaluation.spot_run(None, torch.rand(200))


# ---- the fit on the host -----------------------------------------------------------------------------------------------------------
def _host_fit(lib, Y, n, Nt, t, q):
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    out = (ctypes.c_double * 3)()
    rc = lib.mtadgat_spot_fit_host(Y.ctypes.data_as(_dp), Y.size, n, Nt, t, q, out)
    assert rc == 0, _err(lib)
    return out[0], out[1], out[2]


def test_fit_host_rejects_invalid_arguments(lib):
    Y = np.array([0.5, 1.0, 0.25])
    out = (ctypes.c_double * 3)()
    p = Y.ctypes.data_as(_dp)
    for args in ((None, 3, 10, 3, 0.5, 1e-3, out), (p, 3, 10, 3, 0.5, 1e-3, None), (p, 0, 10, 3, 0.5, 1e-3, out), (p, 3, 0, 3, 0.5, 1e-3, out),
                 (p, 3, 10, 0, 0.5, 1e-3, out), (p, 3, 10, 3, 0.5, 0.0, out), (p, 3, 10, 3, 0.5, 1.0, out), (p, 3, 10, 3, 0.5, float("nan"), out)):
        assert lib.mtadgat_spot_fit_host(*args) == -1 and "spot_fit_host:" in _err(lib), args[1:6]
    for bad in (0.0, -1.0, float("nan")):
        Z = np.array([0.5, bad, 0.25])
        assert lib.mtadgat_spot_fit_host(Z.ctypes.data_as(_dp), 3, 10, 3, 0.5, 1e-3, out) == -1 and "positive" in _err(lib)


KINDS = {
    "gamma": lambda rng, m: rng.gamma(2.0, 1.0, m),
    "exponential": lambda rng, m: rng.exponential(0.3, m),
    "pareto": lambda rng, m: rng.pareto(2.0, m) + 1e-3,
    "near-constant": lambda rng, m: 1.0 + 1e-6 * rng.random(m),
    "lognormal": lambda rng, m: rng.lognormal(0.0, 0.3, m),
}
SIZES = (8, 63, 64, 65, 1024)


def _check(lib, Y, n, Nt, t, q, what):
    ref = [float(v) for v in spot_refs.fit(Y, n, Nt, t, q, np.float64)]
    wide = [float(v) for v in spot_refs.fit(Y, n, Nt, t, q, np.longdouble)]
    assert abs(ref[2] - wide[2]) <= 1e-10 * abs(wide[2]), (what, "the input is ill-conditioned: pick another seed", ref, wide)
    got = _host_fit(lib, Y, n, Nt, t, q)
    assert abs(got[2] - ref[2]) <= 1e-9 * abs(ref[2]), (what, got, ref)
    assert (got[0] == 0.0) == (ref[0] == 0.0) and got[0] * ref[0] >= 0.0, (what, got, ref)
    assert abs(got[0] - ref[0]) <= 1e-7 * abs(ref[0]) and abs(got[1] - ref[1]) <= 1e-7 * abs(ref[1]), (what, got, ref)
    return ref


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_fit_host_matches_the_reference(lib, kind, m):
    rng = np.random.default_rng(1000 * list(KINDS).index(kind) + m)
    Y = KINDS[kind](rng, m)
    _check(lib, Y, 50 * m, m, 0.5, 1e-3, (kind, m))
    # the ring has wrapped: more excesses seen than stored, another risk and threshold
    _check(lib, Y, 400 * m, 3 * m + 1, -1.25, 1e-4, (kind, m, "wrapped"))


def test_fit_host_covers_every_kind_of_candidate(lib):
    """Over the seeded sets both outcomes occur -- a root of the left interval wins (gamma < 0), the exponential tail wins -- and
    sets with roots and without any."""
    seen = set()
    for kind in KINDS:
        for m in SIZES:
            Y = KINDS[kind](np.random.default_rng(1000 * list(KINDS).index(kind) + m), m)
            left, right = spot_refs.interval_roots(Y)
            g = float(spot_refs.fit(Y, 50 * m, m, 0.5, 1e-3)[0])
            seen.add(("roots" if left or right else "no roots", "gamma < 0" if g < 0 else ("gamma = 0" if g == 0 else "gamma > 0")))
    assert ("roots", "gamma < 0") in seen and ("no roots", "gamma = 0") in seen, seen


def test_fit_host_without_roots(lib):
    """No sign change of w on either grid: the exponential candidate stands."""
    rng = np.random.default_rng(5)
    for m in (8, 65):
        Y = rng.uniform(1.0, 2.0, m)
        assert spot_refs.interval_roots(Y) == ([], []) and Y.mean() > Y.min()
        ref = _check(lib, Y, 5000, m, 0.5, 1e-3, ("no roots", m))
        assert ref[0] == 0.0 and ref[1] == float(spot_refs.wave_sum(Y) / m)


def test_fit_host_with_a_huge_peak(lib):
    """1 / Ymax < 2e-8: the left interval starts at -1/Ymax + 1/(32 Ymax)."""
    rng = np.random.default_rng(6)
    for m in (8, 64, 65):
        Y = rng.exponential(1e9, m)
        Y[m // 2] = 9.6e8 * 16
        assert 1.0 / Y.max() < 2e-8
        _check(lib, Y, 5000, m, 0.5, 1e-3, ("huge", m))


def test_fit_host_with_equal_peaks(lib):
    """Ymean == Ymin: the right interval is skipped; the exponential tail with sigma = Y."""
    for m in (8, 64, 100):
        Y = np.full(m, 0.75)
        ref = _check(lib, Y, 5000, m, 0.5, 1e-3, ("equal", m))
        assert ref[0] == 0.0 and ref[1] == 0.75
        assert ref[2] == 0.5 - 0.75 * float(np.log(np.float64(1e-3) * 5000 / m))
