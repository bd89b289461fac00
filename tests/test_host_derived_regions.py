"""Host-side checks of the split-pack regions the library reports (mtadgat_derived_regions), against the C ABI library; no GPU
needed.  The device re-pack tests mask exactly these regions, so the list must be complete: tests/test_host_split_table.py proves that
every step that derives a split pack writes inside exactly one of them (and that each has one writer); this file counts them."""
import ctypes

import pytest

from test_gpu_device_pack import CONFIGS

SHAPES = dict(CONFIGS)
SHAPES["wide_features"] = dict(n_features=600, window_size=12, out_dim=1, kernel_size=3, gru_hid_dim=16, forecast_n_layers=1,
                               forecast_hid_dim=8, recon_hid_dim=16)
SHAPES["deep_stack"] = dict(n_features=38, window_size=100, out_dim=38, kernel_size=7, gru_n_layers=3, gru_hid_dim=150,
                            forecast_n_layers=4, forecast_hid_dim=150, recon_n_layers=3, recon_hid_dim=150)
SHAPES["deep_stack_v1"] = dict(n_features=25, window_size=50, out_dim=5, kernel_size=5, use_gatv2=False, gru_n_layers=3,
                               gru_hid_dim=64, forecast_n_layers=3, forecast_hid_dim=40, recon_n_layers=2, recon_hid_dim=48)


def _create(kw):
    import _native
    from mtad_gat import MTAD_GAT
    lib = _native.load_library()
    model = MTAD_GAT(**kw)
    h = ctypes.c_void_p()
    assert lib.mtadgat_create(ctypes.byref(_native.Config(**model._native_cfg)), ctypes.byref(h)) == 0, lib.mtadgat_last_error()
    return lib, model, h


def _expected_regions(model, kw):
    """Non-empty split-pack regions of the layout: convolution w3, w2h, scale; per attention layer w3, w2h, scale when the fused
    kernel takes it (<= 128 nodes and node dimensions: these shapes fit its LDS), else the (unused) scale and the row GEMM's uw3;
    per recurrence layer wx3, wh3, scale, the chunk-major wxq (all but the decoder's first layer) and wx2 (the first GRU layer),
    plus the first GRU layer's hoisted input projection; recon fc; the backward's transposed packs (one per Linear and per
    recurrence layer), whT3 per recurrence layer, and for GATv2 the score backward's wu3 and lrT per attention layer."""
    F, W = kw["n_features"], kw["window_size"]
    Lg, Ld = kw.get("gru_n_layers", 1), kw.get("recon_n_layers", 1)
    v2 = kw.get("use_gatv2", True)
    n_fc = len(model.forecasting_model.layers)
    gat = sum(3 if K <= 128 and D <= 128 else 2 for K, D in ((F, W), (W, F)))
    forward = 3 + gat + (6 + 4 * (Lg - 1)) + (3 + 4 * (Ld - 1)) + 1
    backward = 2 * (Lg + Ld) + n_fc + 1 + (4 if v2 else 0)
    return forward + backward


@pytest.mark.parametrize("name", list(SHAPES))
def test_derived_regions_are_complete_and_disjoint(name):
    lib, model, h = _create(SHAPES[name])
    try:
        total = lib.mtadgat_packed_floats(h)
        n = lib.mtadgat_derived_regions(h, None, 0)              # count query
        buf = (ctypes.c_int64 * (2 * n + 2))(*([-7] * (2 * n + 2)))
        assert lib.mtadgat_derived_regions(h, buf, n) == n
        assert list(buf[2 * n:]) == [-7, -7]                     # nothing written beyond max_pairs
        regions = [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]
        nonempty = sorted(r for r in regions if r[1] > 0)
        assert all(r[1] >= 0 for r in regions)
        assert len(nonempty) == _expected_regions(model, SHAPES[name]), (name, len(nonempty))
        for (o0, n0), (o1, _) in zip(nonempty, nonempty[1:]):
            assert o0 + n0 <= o1, (name, (o0, n0), o1)           # listed once, no overlap
        assert nonempty[0][0] >= 0 and nonempty[-1][0] + nonempty[-1][1] <= total
        # a short buffer receives the first pairs, the return value stays the full count
        short = (ctypes.c_int64 * 8)(*([-7] * 8))
        assert lib.mtadgat_derived_regions(h, short, 3) == n
        assert [(short[2 * i], short[2 * i + 1]) for i in range(3)] == regions[:3] and list(short[6:]) == [-7, -7]
    finally:
        lib.mtadgat_destroy(h)


def test_deep_stacks_report_more_than_32_regions():
    lib, _, h = _create(SHAPES["deep_stack"])
    try:
        assert lib.mtadgat_derived_regions(h, None, 0) > 32
    finally:
        lib.mtadgat_destroy(h)
