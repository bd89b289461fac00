"""The float64 per-window reference of tests/test_gpu_large_batch_gradients.py, checked on the CPU: the sampled input gradient of
the window-separable loss is the full batch's, the dropout masks are keyed by the global window, the kink detector finds a kink,
and the attribution chunk arithmetic the sampler relies on is what a brute-force walk over the (index, step) units gives."""
import torch

import helpers


def _model(**over):
    from mtad_gat import MTAD_GAT
    kw = dict(n_features=7, window_size=12, out_dim=3, kernel_size=3, gru_hid_dim=20, forecast_n_layers=2, forecast_hid_dim=16,
              recon_hid_dim=18, dropout=0.3, alpha=0.2)
    kw.update(over)
    torch.manual_seed(3)
    m = MTAD_GAT(**kw)
    with torch.no_grad():
        m.feature_gat.bias.normal_()
        m.temporal_gat.bias.normal_()
    return helpers.model64(m)


def test_sampled_input_gradient_equals_the_full_batch_rows():
    m = _model()
    b = 50
    g = torch.Generator().manual_seed(5)
    x = torch.rand(b, 12, 7, generator=g, dtype=torch.float64)
    cp, cr = helpers.separable_cotangents(b, 12, 3, seed=6)
    keep = {"feat": torch.bernoulli(torch.full((b, 7, 7), 0.7, dtype=torch.float64), generator=g),
            "temp": torch.bernoulli(torch.full((b, 12, 12), 0.7, dtype=torch.float64), generator=g),
            "fc": [torch.bernoulli(torch.full((b, 16), 0.7, dtype=torch.float64), generator=g) for _ in range(2)]}
    for masks in (None, keep):
        full = helpers.separable_input_grad(m, x, cp, cr, masks)
        rows = helpers.sample_windows(b, edges=[16, 33], n=12, seed=1)
        sub = None if masks is None else {"feat": masks["feat"][rows], "temp": masks["temp"][rows], "fc": [f[rows] for f in masks["fc"]]}
        part = helpers.separable_input_grad(m, x[rows], cp[rows], cr[rows], sub)
        assert full.dtype == torch.float64 and full.abs().max().item() > 0
        assert (part - full[rows]).abs().max().item() <= 1e-12 * full.abs().max().item()


def test_stacked_masks_reach_the_recurrences():
    """`gru` / `rec` keep-masks change the input gradient of a model with stacked recurrences (they are not ignored)."""
    m = _model(gru_n_layers=2, recon_n_layers=2)
    b = 6
    g = torch.Generator().manual_seed(7)
    x = torch.rand(b, 12, 7, generator=g, dtype=torch.float64)
    cp, cr = helpers.separable_cotangents(b, 12, 3, seed=8)
    ones = {"feat": torch.ones(b, 7, 7, dtype=torch.float64), "temp": torch.ones(b, 12, 12, dtype=torch.float64),
            "fc": [torch.ones(b, 16, dtype=torch.float64)] * 2, "gru": [torch.ones(b, 12, 20, dtype=torch.float64)],
            "rec": [torch.ones(b, 12, 18, dtype=torch.float64)]}
    dropped = dict(ones, gru=[torch.bernoulli(torch.full((b, 12, 20), 0.7, dtype=torch.float64), generator=g)])
    d1 = helpers.separable_input_grad(m, x, cp, cr, ones)
    d2 = helpers.separable_input_grad(m, x, cp, cr, dropped)
    assert (d1 - d2).abs().max().item() > 1e-6


def test_dropout_mask_is_keyed_by_the_global_window():
    full = helpers.dropout_keep_mask(seed=123456789012, stream=2, p=0.3, n_windows=40, n_per_window=50, window0=0)
    for w in (0, 1, 17, 39):
        row = helpers.dropout_keep_mask(seed=123456789012, stream=2, p=0.3, n_windows=1, n_per_window=50, window0=w)
        assert (row[0] == full[w]).all()
    shifted = helpers.dropout_keep_mask(seed=123456789012, stream=2, p=0.3, n_windows=30, n_per_window=50, window0=10)
    assert (shifted == full[10:40]).all()
    big = helpers.dropout_keep_mask(seed=5, stream=16, p=0.3, n_windows=3, n_per_window=8, window0=(1 << 32) + 12345)
    assert (big[1] == helpers.dropout_keep_mask(5, 16, 0.3, 1, 8, window0=(1 << 32) + 12346)[0]).all()


def test_kink_detector_flags_a_zero_conv_preactivation():
    import torch.nn.functional as F
    m = _model()
    g = torch.Generator().manual_seed(9)
    x = torch.rand(3, 12, 7, generator=g, dtype=torch.float64)
    assert not helpers.kink_windows(m, x).any()
    conv = m.conv.conv
    pre = F.conv1d(F.pad(x.permute(0, 2, 1), (1, 1)), conv.weight, conv.bias)       # kernel 3: pad 1, (b, F, W)
    c, t = 2, 5
    x[1, t, c] += -pre[1, c, t] / conv.weight[c, c, 1]                               # centre tap: channel c at step t cancels
    pre2 = F.conv1d(F.pad(x.permute(0, 2, 1), (1, 1)), conv.weight, conv.bias)
    assert abs(pre2[1, c, t].item()) < 1e-12
    assert helpers.kink_windows(m, x).tolist() == [False, True, False]


def test_kink_detector_sees_gat_v1_leaky_relu_arguments():
    m = _model(use_gatv2=False)
    g = torch.Generator().manual_seed(10)
    x = torch.rand(2, 12, 7, generator=g, dtype=torch.float64)
    assert not helpers.kink_windows(m, x).any()
    assert helpers.kink_windows(m, x, rel=0.5).all()                  # (a coarse threshold flags every window)


def test_attribution_chunk_arithmetic_matches_brute_force():
    for count, steps, units in ((160, 32, 1000), (200, 32, 2000), (3000, 0, 1150), (7, 5, 3), (5, 0, 2), (1, 32, 7), (4, 3, 12)):
        chunks = helpers.attribution_chunks(count, steps, units)
        m = max(steps, 1)
        unit_chunk = {}
        for ci, (u0, nu) in enumerate(chunks):
            assert 0 < nu <= units
            for u in range(u0, u0 + nu):
                assert u not in unit_chunk
                unit_chunk[u] = ci
        assert sorted(unit_chunk) == list(range(count * m))
        brute = [p for p in range(count) if len({unit_chunk[p * m + k] for k in range(m)}) > 1]
        assert helpers.straddling_indices(count, steps, units) == brute, (count, steps, units)
    assert helpers.straddling_indices(160, 32, 1000)[:2] == [31, 62]


def test_window_sampler():
    for b, edges in ((656, [656]), (8193, [656, 2561, 4096, 8192]), (20000, [656, 2561, 4096, 8192, 16384]), (3, [])):
        s = helpers.sample_windows(b, edges, n=32, seed=4)
        assert len(s) == min(b, 32) and len(set(s)) == len(s) and s == sorted(s)
        assert all(0 <= w < b for w in s)
        assert {0, b - 1} <= set(s)
        for e in edges:
            assert e - 1 in s and (e >= b or e in s)
