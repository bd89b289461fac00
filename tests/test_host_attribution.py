"""Score attribution (MTAD_GAT.score_attribution, mtadgat_score_attribution / mtadgat_backward_data) without a GPU: the exported
symbols, the workspace query, argument errors, and the CPU route -- Integrated Gradients' completeness and the gradient against
central finite differences on a tiny float64 model."""
import ctypes

import pytest
import torch

MSL = dict(n_features=55, window_size=100, out_dim=1, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3, forecast_hid_dim=150,
           recon_hid_dim=150)
TINY = dict(n_features=4, window_size=6, out_dim=2, kernel_size=3, feat_gat_embed_dim=3, time_gat_embed_dim=3, gru_hid_dim=5,
            forecast_n_layers=1, forecast_hid_dim=6, recon_hid_dim=5, dropout=0.3, alpha=0.2)
TINY_DIMS = [1, 3]


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


def _tiny(dtype=torch.float64, seed=3):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(seed)
    model = MTAD_GAT(**TINY).to(dtype)
    with torch.no_grad():
        model.feature_gat.bias.normal_()
        model.temporal_gat.bias.normal_()
    g = torch.Generator().manual_seed(seed)
    values = torch.rand(20, TINY["n_features"], generator=g, dtype=torch.float64).to(dtype)
    return model, values


def _score(model, S, dims, dim_w, gamma):
    """a_i(S) of one slice S (W+1, F), straight from the definition (eval mode, torch ops)."""
    import _torchpath
    W = model.window_size
    with torch.no_grad(), _torchpath._eval_mode(model):
        preds, _ = _torchpath.forward(model, S[None, :W])
        _, recons = _torchpath.forward(model, S[None, 1:])
        y = S[W, dims]
        return float((dim_w * ((preds[0] - y).abs() + gamma * (recons[0, -1] - y).abs())).sum())


def test_symbols_exported():
    lib = _lib()
    for name in ("mtadgat_backward_data", "mtadgat_score_attribution", "mtadgat_score_attribution_workspace_bytes"):
        assert hasattr(lib, name), name


def test_workspace_query_is_bounded():
    lib = _lib()
    h = _handle(lib, **MSL)
    try:
        q = lambda c, s: lib.mtadgat_score_attribution_workspace_bytes(h, c, s)     # noqa: E731
        assert q(0, 0) == 0 and q(-1, 0) == 0 and q(4, -1) == 0
        assert 0 < q(1, 0) < q(16, 0) <= q(16, 8)
        # the windows are walked in chunks: the workspace stops growing (~4 GiB of chunk scratch)
        big = q(4096, 32)
        assert big == q(100000, 32) and big <= 4.5 * 2 ** 30
    finally:
        lib.mtadgat_destroy(h)


def test_c_argument_errors():
    lib = _lib()
    h = _handle(lib, **MSL)
    try:
        args = lambda handle: (handle, None, 200, None, 1, None, 1, None, ctypes.c_float(1.0), 0, None, 0, None, None, 0, None)  # noqa: E731
        assert lib.mtadgat_score_attribution(*args(None)) == -1
        assert lib.mtadgat_score_attribution(*args(h)) == -4          # no weights loaded
        assert b"load_weights" in lib.mtadgat_last_error()
        assert lib.mtadgat_backward_data(h, None, 4, 0, ctypes.c_float(0.0), ctypes.c_uint64(0), None, None, None, 0, None, None, 0, None) == -4
    finally:
        lib.mtadgat_destroy(h)


def test_python_argument_errors():
    model, values = _tiny(torch.float32)
    W, F = TINY["window_size"], TINY["n_features"]
    n = values.shape[0] - W
    with pytest.raises(IndexError):
        model.score_attribution(values, [n], TINY_DIMS)
    with pytest.raises(IndexError):
        model.score_attribution(values, [-1], TINY_DIMS)
    with pytest.raises(ValueError):
        model.score_attribution(values, [0], TINY_DIMS, method="saliency")
    with pytest.raises(ValueError):
        model.score_attribution(values, [0], TINY_DIMS, method="integrated", steps=0)
    with pytest.raises(RuntimeError):
        model.score_attribution(values, [0], [0, 1, 2])                           # out_dim is 2
    with pytest.raises(IndexError):
        model.score_attribution(values, [0], [0, F])
    with pytest.raises(RuntimeError):
        model.score_attribution(values, [0], TINY_DIMS, method="integrated", baseline=torch.zeros(W, F))
    with pytest.raises(RuntimeError):
        model.score_attribution(values[:, :3], [0], TINY_DIMS)
    empty = model.score_attribution(values, [], TINY_DIMS)
    assert empty.shape == (0, W + 1, F) and empty.dtype == torch.float32


def test_cpu_route_leaves_state_alone():
    model, values = _tiny(torch.float32)
    model.train()
    for p in model.parameters():
        p.grad = None
    x = values[:TINY["window_size"]][None]
    torch.manual_seed(0)
    model.eval()
    before = model(x)
    model.train()
    a1 = model.score_attribution(values, [0, 5], TINY_DIMS, gamma=0.7)
    a2 = model.score_attribution(values, [0, 5], TINY_DIMS, gamma=0.7)
    assert model.training and all(m.training for m in model.modules())
    assert all(p.grad is None for p in model.parameters())
    assert torch.equal(a1, a2)                                                    # eval-mode function: no dropout
    model.eval()
    after = model(x)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_gradient_matches_central_differences():
    """method="gradient" on a tiny float64 model against central differences of a_i(S) taken from the definition: the score
    is piecewise smooth (abs, ReLU), so h = 1e-6 stays inside one piece for random data; the difference quotient's error is
    O(h^2) there, far below the 1e-6 gate."""
    model, values = _tiny()
    W, F = TINY["window_size"], TINY["n_features"]
    gamma = 0.6
    dim_w = torch.full((2,), 0.5, dtype=torch.float64)
    for i in (0, 7, values.shape[0] - W - 1):
        attr = model.score_attribution(values, [i], TINY_DIMS, gamma=gamma)[0]
        assert attr.dtype == torch.float64 and attr.shape == (W + 1, F)
        S = values[i:i + W + 1].clone()
        fd = torch.zeros_like(S)
        h = 1e-6
        for r in range(W + 1):
            for f in range(F):
                Sp, Sm = S.clone(), S.clone()
                Sp[r, f] += h
                Sm[r, f] -= h
                fd[r, f] = (_score(model, Sp, TINY_DIMS, dim_w, gamma) - _score(model, Sm, TINY_DIMS, dim_w, gamma)) / (2 * h)
        err = (attr - fd).abs().max().item()
        assert err <= 1e-6 * max(1.0, fd.abs().max().item()), (i, err)
        assert attr[W].abs().sum() > 0                                           # the direct dependence through the target row


def test_integrated_gradients_completeness():
    """sum(attr) = (1/m) sum_k g(alpha_k), g(alpha) = <grad a_i(b + alpha (S - b)), S - b>: the midpoint rule for
    integral_0^1 g = a_i(S) - a_i(b).  On each of the m cells |integral_cell g - g(alpha_k)/m| <= osc_cell(g)/m, so the error is
    at most TV(g)/m; TV(g) is estimated from the m samples (sum |g(alpha_k+1) - g(alpha_k)|) and taken twice as a margin for the
    variation between samples."""
    model, values = _tiny()
    W = TINY["window_size"]
    gamma, m, i = 1.3, 256, 4
    dim_w = torch.full((2,), 0.5, dtype=torch.float64)
    for baseline in (None, values[:W + 1].mean(0) * 0.5):
        attr = model.score_attribution(values, [i], TINY_DIMS, gamma=gamma, method="integrated", steps=m, baseline=baseline)[0]
        S = values[i:i + W + 1]
        b = torch.zeros_like(S) if baseline is None else baseline.expand_as(S)
        delta = _score(model, S, TINY_DIMS, dim_w, gamma) - _score(model, b.clone(), TINY_DIMS, dim_w, gamma)
        g = []
        for k in range(m):
            v = values.clone()
            v[i:i + W + 1] = b + ((k + 0.5) / m) * (S - b)
            g.append(float((model.score_attribution(v, [i], TINY_DIMS, gamma=gamma)[0] * (S - b)).sum()))
        g = torch.tensor(g, dtype=torch.float64)
        assert abs(attr.sum().item() - g.mean().item()) <= 1e-12 * max(1.0, g.abs().max().item())
        tv = (g[1:] - g[:-1]).abs().sum().item()
        bound = 2 * tv / m + 1e-12
        err = abs(attr.sum().item() - delta)
        print(f"baseline={'zeros' if baseline is None else 'row'}: |sum attr - delta a| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_scale_scores_weights_cpu():
    """scale_scores divides w_d by 1 + IQR_d of the whole series' per-dimension scores (constant): with a single output
    dimension the attribution is the unscaled one over (1 + IQR)."""
    import _torchpath
    from mtad_gat import MTAD_GAT, _column_quantiles
    torch.manual_seed(5)
    kw = dict(TINY, out_dim=1)
    model = MTAD_GAT(**kw).double()
    g = torch.Generator().manual_seed(5)
    values = torch.rand(30, kw["n_features"], generator=g, dtype=torch.float64)
    plain = model.score_attribution(values, [2, 9], [2], gamma=0.5)
    scaled = model.score_attribution(values, [2, 9], [2], gamma=0.5, scale_scores=True)
    per_dim = _torchpath.per_dim_scores(model, values, [2], 0.5)
    q = _column_quantiles(per_dim[:, 0], torch.tensor([0.25, 0.75], dtype=torch.float64))
    assert torch.allclose(scaled, plain / (1.0 + (q[1] - q[0])), rtol=1e-12, atol=1e-15)
