"""Attention maps (MTAD_GAT.attention_maps / attention_series, the mtadgat_attention* C ABI) without a GPU: the exported
symbols, the workspace query, argument errors, and the CPU route against the oracle."""
import ctypes

import pytest
import torch

from helpers import ALL_CASES, Case, gate
from oracle import mtad_gat_oracle as oracle

MSL = dict(n_features=55, window_size=100, out_dim=55, kernel_size=7, gru_hid_dim=150, forecast_hid_dim=150, recon_hid_dim=150)


def _lib():
    import _native
    return _native.load_library()


def _handle(lib, **kw):
    import _native
    from mtad_gat import MTAD_GAT
    model = MTAD_GAT(**kw)
    h = ctypes.c_void_p()
    assert lib.mtadgat_create(ctypes.byref(_native.Config(**model._native_cfg)), ctypes.byref(h)) == 0, lib.mtadgat_last_error()
    return h


def test_symbols_exported():
    lib = _lib()
    for name in ("mtadgat_attention", "mtadgat_attention_mean", "mtadgat_attention_series", "mtadgat_attention_series_mean",
                 "mtadgat_attention_workspace_bytes"):
        assert hasattr(lib, name), name


def test_workspace_query():
    lib = _lib()
    h = _handle(lib, **MSL)
    try:
        q = lambda b, r: lib.mtadgat_attention_workspace_bytes(h, b, r)     # noqa: E731
        assert q(256, 0) > 0 and q(256, 1) > 0
        assert q(512, 0) > q(256, 0)
        # the mean mode is bounded by one chunk: 65 536 windows need no more than the chunk size does
        assert q(65536, 1) == q(1 << 20, 1)
        assert q(65536, 1) < 65536 * (55 * 55 + 100 * 100) * 4 // 4
        # a chunk's maps go through the workspace in the mean mode
        assert q(8, 1) >= 8 * 100 * 100 * 4
        assert q(0, 0) == 0 and q(0, 1) == 0
        assert lib.mtadgat_attention_workspace_bytes(None, 256, 1) == 0
    finally:
        lib.mtadgat_destroy(h)


def test_argument_errors():
    lib = _lib()
    buf = ctypes.c_void_p(16)          # never dereferenced: every call below fails its checks first
    assert lib.mtadgat_attention(None, buf, 4, buf, buf, buf, 1 << 20, None) == -1
    assert lib.mtadgat_attention_mean(None, buf, 4, buf, buf, buf, 1 << 20, None) == -1
    assert lib.mtadgat_attention_series(None, buf, 200, None, 0, 1, 4, buf, buf, buf, 1 << 20, None) == -1
    assert lib.mtadgat_attention_series_mean(None, buf, 200, None, 0, 1, 4, buf, buf, buf, 1 << 20, None) == -1
    h = _handle(lib, **MSL)
    try:
        assert lib.mtadgat_attention(h, buf, 0, buf, buf, buf, 1 << 20, None) == -1
        assert lib.mtadgat_attention_mean(h, buf, 0, buf, buf, buf, 1 << 20, None) == -1
        # windows outside the series
        assert lib.mtadgat_attention_series_mean(h, buf, 150, None, 0, 1, 52, buf, buf, buf, 1 << 30, None) == -1
        # no weights loaded yet
        assert lib.mtadgat_attention(h, buf, 4, buf, buf, buf, 1 << 30, None) == -4
    finally:
        lib.mtadgat_destroy(h)


def _oracle_maps(model, x, dtype=torch.float32):
    """oracle.graph_attention(...)[1] of both layers, fed oracle.conv_layer's output, in `dtype`."""
    sd = {k: v.to(dtype) for k, v in model.state_dict().items()}
    xc = oracle.conv_layer(x.to(dtype), sd["conv.conv.weight"], sd["conv.conv.bias"])
    v2 = model.feature_gat.use_gatv2
    _, af = oracle.graph_attention(xc.permute(0, 2, 1), sd["feature_gat.lin.weight"], sd["feature_gat.lin.bias"], sd["feature_gat.a"],
                                   sd.get("feature_gat.bias"), model.alpha, v2)
    _, at = oracle.graph_attention(xc, sd["temporal_gat.lin.weight"], sd["temporal_gat.lin.bias"], sd["temporal_gat.a"],
                                   sd.get("temporal_gat.bias"), model.alpha, v2)
    return af, at


@pytest.mark.parametrize("name", [c for c in ALL_CASES if c in ("msl", "smap", "smd_1_1") or c.startswith("syn_v1")])
def test_cpu_maps_match_oracle(name):
    case = Case(name)
    model = case.build_model()
    x = case.x[:6]
    af, at = model.attention_maps(x)
    rf, rt = _oracle_maps(model, x)
    rf64, rt64 = _oracle_maps(model, x, torch.float64)
    F, W = model.n_features, model.window_size
    assert af.dtype == torch.float32 and at.dtype == torch.float32
    assert af.shape == (x.shape[0], F, F) and at.shape == (x.shape[0], W, W)
    # (smd_1_1's temporal scores are ill-conditioned: the float32 oracle itself is 2e-2 off its float64 evaluation there, and
    # gate() then bounds the distance to float64 by that rounding noise)
    gate(af, rf, rf64, tol=1e-6, what="feature maps")
    gate(at, rt, rt64, tol=1e-6, what="temporal maps")
    assert (af.double().sum(-1) - 1).abs().max().item() <= 1e-5
    assert (at.double().sum(-1) - 1).abs().max().item() <= 1e-5
    mf, mt = model.attention_maps(x, reduce="mean")
    assert mf.shape == (F, F) and mt.shape == (W, W)
    assert torch.equal(mf, af.double().mean(0).float()) and torch.equal(mt, at.double().mean(0).float())


def test_cpu_maps_are_eval_maps_and_keep_the_mode():
    case = Case("syn_v1_small")
    model = case.build_model().train()
    x = case.x[:4]
    a1 = model.attention_maps(x)
    assert model.training and torch.is_grad_enabled()
    model.eval()
    a0 = model.attention_maps(x)
    assert torch.equal(a1[0], a0[0]) and torch.equal(a1[1], a0[1])
    assert not a1[0].requires_grad
    # reduced-precision inputs: maps come back in float32
    for dt in (torch.bfloat16, torch.float16):
        af, at = model.attention_maps(x.to(dt))
        assert af.dtype == torch.float32 and at.dtype == torch.float32


def test_cpu_series_matches_materialised_windows():
    case = Case("msl")
    model = case.build_model()
    W = model.window_size
    g = torch.Generator().manual_seed(3)
    series = torch.rand(W + 20, model.n_features, generator=g)
    for kw, starts in ((dict(stride=1), list(range(21))), (dict(stride=3), list(range(0, 21, 3))),
                       (dict(starts=torch.tensor([5, 0, 17, 2])), [5, 0, 17, 2])):
        x = torch.stack([series[s:s + W] for s in starts])
        af, at = model.attention_series(series, reduce=None, **kw)
        rf, rt = model.attention_maps(x)
        assert torch.equal(af, rf) and torch.equal(at, rt)
        mf, mt = model.attention_series(series, **kw)
        assert (mf - rf.double().mean(0).float()).abs().max().item() == 0.0


def test_bad_arguments_raise():
    case = Case("smap")
    model = case.build_model()
    with pytest.raises(RuntimeError):
        model.attention_maps(case.x[:, :, :3])
    with pytest.raises(ValueError):
        model.attention_maps(case.x[:2], reduce="sum")
    with pytest.raises(RuntimeError):
        model.attention_maps(case.x[:0], reduce="mean")
    with pytest.raises(RuntimeError):
        model.attention_series(torch.rand(10, model.n_features))
