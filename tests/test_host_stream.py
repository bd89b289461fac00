"""The streaming entry points (csrc/mtadgat_stream.hip, streaming.StreamScorer) without a GPU: the ring index arithmetic the
stage kernel shares with mtadgat_stream_window_start, checked exhaustively against a numpy simulation of the mirrored writes --
mtadgat_forward_series trusts the starts it is given, so an off-by-one there is a memory fault --, the symbols, and every
argument check that happens before anything touches the device."""
import ctypes

import numpy as np
import pytest
import torch

PTR = 0x10000            # a non-null, 16-byte aligned "device pointer": validation fails before it would be used


@pytest.fixture(scope="module")
def lib():
    import streaming
    return streaming._lib()


def _err(lib):
    return lib.mtadgat_last_error().decode()


# ---- index arithmetic --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_block", [1, 5, 12, 13])
@pytest.mark.parametrize("W", [1, 2, 12])
def test_window_starts_exhaustively(lib, W, max_block):
    """Every row count 0 .. 4R and every t < max_block, with the rows after t of the same (full) push already written, as the
    stage kernel leaves them before the forward reads: the start is in bounds, the W slots hold rows k-W+1 .. k, and none of
    them was overwritten by a later row of the push."""
    import streaming
    R = W + max_block - 1
    ring = np.full(2 * R, -1, np.int64)                   # the row number each slot holds
    for count in range(4 * R + 1):
        snapshot = ring.copy()
        for t in range(max_block):                        # the push of max_block rows that starts at `count`
            k = count + t
            snapshot[k % R] = snapshot[k % R + R] = k
        for t in range(max_block):
            k = count + t
            start = lib.mtadgat_stream_window_start(count, t, W, R)
            assert start == streaming.window_start(count, t, W, R)
            assert 0 <= start <= 2 * R - W, (count, t, start)
            held = snapshot[start:start + W]
            if k >= W - 1:
                assert np.array_equal(held, np.arange(k - W + 1, k + 1)), (count, t, start, held)
            # whatever the window holds was written no later than its own row
            assert np.all(held <= k), (count, t, start, held)
            # a shorter push (T = t + 1) reads the same rows: later rows only ever touch other slots
            short = ring.copy()
            for u in range(t + 1):
                short[(count + u) % R] = short[(count + u) % R + R] = count + u
            assert np.array_equal(short[start:start + W], held) or k < W - 1, (count, t)
        ring[count % R] = ring[count % R + R] = count     # rows arrive one at a time between the checks


def test_window_start_rejects_nonsense(lib):
    assert lib.mtadgat_stream_window_start(-1, 0, 12, 16) == -1
    assert lib.mtadgat_stream_window_start(0, -1, 12, 16) == -1
    assert lib.mtadgat_stream_window_start(0, 0, 0, 16) == -1
    assert lib.mtadgat_stream_window_start(0, 0, 12, 11) == -1
    assert lib.mtadgat_stream_window_start(2 ** 40 + 3, 4, 12, 16) == (2 ** 40 + 7) % 16 + 16 - 12 + 1


# ---- exports -----------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported(lib):
    import streaming
    for name in ("mtadgat_stream_state_bytes", "mtadgat_stream_init", "mtadgat_stream_workspace_bytes", "mtadgat_stream_push",
                 "mtadgat_stream_update", "mtadgat_stream_flush", "mtadgat_stream_window_start"):
        assert hasattr(lib, name), name
    for name in ("push", "update", "flush", "reset"):
        assert callable(getattr(streaming.StreamScorer, name)), name
    assert lib.mtadgat_abi_version() == 1


# ---- the C entry points' validation --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(lib):
    import _native
    cfg = _native.Config(n_features=7, window_size=12, out_dim=7, kernel_size=3, use_gatv2=1, feat_embed=24, time_embed=14, gru_n_layers=1,
                         gru_hid_dim=24, forecast_n_linear=2, forecast_hid_dim=24, recon_n_layers=1, recon_hid_dim=24, alpha=0.2)
    h = ctypes.c_void_p()
    assert lib.mtadgat_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    yield h
    lib.mtadgat_destroy(h)


def test_size_queries(lib, handle):
    sb, wb = lib.mtadgat_stream_state_bytes, lib.mtadgat_stream_workspace_bytes
    assert sb(None, 3, 5) == 0 and sb(handle, 0, 5) == 0 and sb(handle, 3, 0) == 0 and sb(handle, 3, 65537) == 0 and sb(handle, 1 << 31, 5) == 0
    assert wb(None, 5) == 0 and wb(handle, 0) == 0 and wb(handle, 1 << 31) == 0
    # the histories dominate: S streams x 2 (W + max_block - 1) rows x F floats
    assert sb(handle, 3, 5) >= 3 * 2 * 16 * 7 * 4 and sb(handle, 3, 5) % 16 == 0
    assert sb(handle, 4, 5) > sb(handle, 3, 5) and sb(handle, 3, 6) > sb(handle, 3, 5)
    # the forward's workspace, two (windows, out_dim) outputs and an int64 start per window
    assert wb(handle, 15) >= lib.mtadgat_workspace_bytes(handle, 15) + 15 * (2 * 7 * 4 + 8) and wb(handle, 15) % 16 == 0


INIT_BAD = {"null handle": dict(h=None), "null state": dict(state=None), "misaligned state": dict(state=PTR + 8), "no streams": dict(S=0),
            "max_block < 1": dict(B=0), "max_block too large": dict(B=65537), "alpha > 1": dict(alpha=1.5), "alpha < 0": dict(alpha=-0.1),
            "alpha NaN": dict(alpha=float("nan")), "gamma NaN": dict(gamma=float("nan")), "merge_gap < 0": dict(gap=-1),
            "min_length < 1": dict(min_length=0), "center without spread": dict(center=True), "dimension outside": dict(dims=[0, 1, 2, 3, 4, 5, 7]),
            "negative dimension": dict(dims=[-1, 1, 2, 3, 4, 5, 6])}


@pytest.mark.parametrize("case", list(INIT_BAD))
def test_init_rejects_invalid_arguments(lib, handle, case):
    kw = dict(h=handle, state=PTR, S=3, B=5, gamma=1.0, alpha=0.0, gap=0, min_length=1, dims=None, center=False)
    kw.update(INIT_BAD[case])
    dims = (ctypes.c_int32 * 7)(*kw["dims"]) if kw["dims"] else None
    center = (ctypes.c_float * 7)() if kw["center"] else None
    rc = lib.mtadgat_stream_init(kw["h"], kw["state"], kw["S"], kw["B"], kw["gamma"], kw["alpha"], kw["gap"], kw["min_length"], dims, center, None,
                                 None)
    assert rc == -1 and "stream_init:" in _err(lib), (case, rc, _err(lib))


CALL_BAD = {"null handle": dict(h=None), "null state": dict(state=None), "no streams": dict(S=0), "n < 1": dict(n=0), "n > n_streams": dict(n=4),
            "T < 1": dict(T=0), "T > max_block": dict(T=6), "null rows": dict(rows=None)}


@pytest.mark.parametrize("case", list(CALL_BAD))
def test_push_update_flush_reject_invalid_arguments(lib, handle, case):
    import streaming
    kw = dict(h=handle, state=PTR, S=3, B=5, n=3, T=5, rows=PTR)
    kw.update(CALL_BAD[case])
    out = streaming._Outputs()
    ws = lib.mtadgat_stream_workspace_bytes(handle, 15)
    rc = lib.mtadgat_stream_push(kw["h"], kw["state"], kw["S"], kw["B"], kw["rows"], None, kw["n"], kw["T"], 0.5, None, ctypes.byref(out), PTR, ws,
                                 None)
    assert rc == -1 and "stream_push:" in _err(lib), (case, rc, _err(lib))
    rc = lib.mtadgat_stream_update(kw["h"], kw["state"], kw["S"], kw["B"], PTR, PTR, kw["rows"], None, kw["n"], kw["T"], 0, 0.5, None,
                                   ctypes.byref(out), None)
    assert rc == -1 and "stream_update:" in _err(lib), (case, rc, _err(lib))
    if case not in ("T < 1", "T > max_block", "null rows"):
        rc = lib.mtadgat_stream_flush(kw["h"], kw["state"], kw["S"], kw["B"], None, kw["n"], 0, ctypes.byref(out), None)
        assert rc == -1 and "stream_flush:" in _err(lib), (case, rc, _err(lib))


def test_push_checks_its_workspace_and_weights(lib, handle):
    import streaming
    out = streaming._Outputs()
    ws = lib.mtadgat_stream_workspace_bytes(handle, 15)
    args = (handle, PTR, 3, 5, PTR, None, 3, 5, 0.5, None, ctypes.byref(out))
    assert lib.mtadgat_stream_push(*args, None, ws, None) == -5 and "workspace" in _err(lib)
    assert lib.mtadgat_stream_push(*args, PTR + 4, ws, None) == -5 and "aligned" in _err(lib)
    assert lib.mtadgat_stream_push(*args, PTR, ws - 1, None) == -5 and "too small" in _err(lib)
    assert lib.mtadgat_stream_push(*args, PTR, ws, None) == -4                 # no weights loaded: nothing was launched
    assert lib.mtadgat_stream_flush(handle, PTR, 3, 5, None, 3, 0, None, None) == -1 and "neither" in _err(lib)
    assert lib.mtadgat_stream_update(handle, PTR, 3, 5, None, PTR, PTR, None, 3, 5, 0, 0.5, None, ctypes.byref(out), None) == -1


# ---- the Python class ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_model():
    from mtad_gat import MTAD_GAT
    torch.manual_seed(3)
    return MTAD_GAT(n_features=7, window_size=12, out_dim=3, kernel_size=3, gru_hid_dim=24, forecast_hid_dim=24, recon_hid_dim=24).eval()


def test_a_cpu_model_is_refused_naming_the_gpu(cpu_model):
    from streaming import StreamScorer
    with pytest.raises(RuntimeError, match="GPU"):
        StreamScorer(cpu_model, 4, 0.5, target_dims=[0, 2, 5])


SCORER_BAD = {
    "no streams": dict(n_streams=0), "fractional streams": dict(n_streams=2.5), "max_block < 1": dict(max_block=0),
    "max_block too large": dict(max_block=65537), "span < 1": dict(smoothing_span=0.5), "span 0": dict(smoothing_span=0),
    "merge_gap < 0": dict(merge_gap=-1), "min_length < 1": dict(min_length=0), "gamma NaN": dict(gamma=float("nan")),
    "target_dims missing": dict(target_dims=None), "too few target_dims": dict(target_dims=[0, 1]), "target_dims outside": dict(target_dims=[0, 1, 7]),
    "scale of the wrong length": dict(scale=(torch.zeros(2), torch.zeros(3))), "thresholds of the wrong length": dict(threshold=torch.zeros(5)),
}


@pytest.mark.parametrize("case", list(SCORER_BAD))
def test_scorer_validates_before_it_needs_a_device(cpu_model, case):
    from streaming import StreamScorer
    kw = dict(n_streams=4, threshold=0.5, target_dims=[0, 2, 5])
    kw.update(SCORER_BAD[case])
    with pytest.raises(ValueError):
        StreamScorer(cpu_model, **kw)
