"""Host-side checks of models with more than 512 features (up to 2048), against the C ABI library; no GPU needed."""
import ctypes

import pytest

WIDE = dict(window_size=12, out_dim=1, kernel_size=3, gru_hid_dim=16, forecast_n_layers=1, forecast_hid_dim=8, recon_hid_dim=16)


def _lib():
    import _native
    return _native.load_library()


def _create(lib, **kw):
    import _native
    from mtad_gat import MTAD_GAT
    model = MTAD_GAT(**kw)
    h = ctypes.c_void_p()
    rc = lib.mtadgat_create(ctypes.byref(_native.Config(**model._native_cfg)), ctypes.byref(h))
    return rc, h


@pytest.mark.parametrize("F", [513, 777, 1024, 2048])
@pytest.mark.parametrize("v2", [True, False])
def test_create_accepts_up_to_2048_features(F, v2):
    lib = _lib()
    rc, h = _create(lib, n_features=F, use_gatv2=v2, **WIDE)
    assert rc == 0, lib.mtadgat_last_error()
    # the workspace holds the (K, K) score matrix of the feature layer per window
    assert lib.mtadgat_workspace_bytes(h, 4) >= 4 * F * F * 4
    assert lib.mtadgat_destroy(h) == 0


def test_create_refuses_2049_features_naming_the_limit():
    lib = _lib()
    rc, _ = _create(lib, n_features=2049, **WIDE)
    assert rc == -2 and b"2048" in lib.mtadgat_last_error()


@pytest.mark.parametrize("bad, word", [(dict(window_size=600), b"512"), (dict(gru_hid_dim=300), b"hidden")])
def test_other_limits_stay(bad, word):
    lib = _lib()
    kw = dict(WIDE, n_features=1024)
    kw.update(bad)
    rc, _ = _create(lib, **kw)
    assert rc == -2 and word in lib.mtadgat_last_error()


def test_default_chunk_of_the_widest_model_fits_the_budget():
    """F = 2048, W = 512: ~70 MB of scratch per window; the default chunk stays near the 6 GB the un-fused path is given (the
    chunk is sized on the large-batch plan, without the small-batch buffers a chunk of this size also gets)."""
    lib = _lib()
    rc, h = _create(lib, n_features=2048, window_size=512, out_dim=2048, kernel_size=7, gru_hid_dim=150, forecast_n_layers=1,
                    forecast_hid_dim=150, recon_hid_dim=150)
    assert rc == 0, lib.mtadgat_last_error()
    chunk = lib.mtadgat_chunk_windows(h)
    assert 8 <= chunk < 128 and chunk % 8 == 0
    assert lib.mtadgat_workspace_bytes(h, chunk) <= 7 * 1024 ** 3
    assert lib.mtadgat_destroy(h) == 0


@pytest.mark.parametrize("v2", [True, False])
@pytest.mark.parametrize("F", [1024, 2048])
def test_wide_feature_models_have_a_hip_backward(F, v2):
    lib = _lib()
    rc, h = _create(lib, n_features=F, use_gatv2=v2, **WIDE)
    assert rc == 0
    assert lib.mtadgat_backward_supported(h) == 1, lib.mtadgat_last_error()
    assert lib.mtadgat_tape_bytes(h, 4) >= 4 * F * F * 4          # the feature layer's attention matrix per window
    assert lib.mtadgat_destroy(h) == 0


@pytest.mark.parametrize("F", [1024, 2048])
def test_device_repack_gather_table_of_wide_feature_models(F):
    """Host-side self check of the device re-pack's index table (as for the narrow models in test_host_module.py)."""
    import _native
    import torch
    from mtad_gat import MTAD_GAT
    torch.manual_seed(3)
    model = MTAD_GAT(n_features=F, **dict(WIDE, out_dim=3))
    lib = _lib()
    h = ctypes.c_void_p()
    assert lib.mtadgat_create(ctypes.byref(_native.Config(**model._native_cfg)), ctypes.byref(h)) == 0
    sd = {k: v.detach().float().contiguous() for k, v in model.state_dict().items()}
    cfg = model._native_cfg
    p = _native.Params()
    ptr = lambda key: ctypes.c_void_p(sd[key].data_ptr())      # noqa: E731
    p.conv_weight, p.conv_bias = ptr("conv.conv.weight"), ptr("conv.conv.bias")
    p.feat_lin_weight, p.feat_lin_bias = ptr("feature_gat.lin.weight"), ptr("feature_gat.lin.bias")
    p.feat_a, p.feat_bias = ptr("feature_gat.a"), ptr("feature_gat.bias")
    p.temp_lin_weight, p.temp_lin_bias = ptr("temporal_gat.lin.weight"), ptr("temporal_gat.lin.bias")
    p.temp_a, p.temp_bias = ptr("temporal_gat.a"), ptr("temporal_gat.bias")
    for l in range(cfg["gru_n_layers"]):
        p.gru_w_ih[l], p.gru_w_hh[l] = ptr(f"gru.gru.weight_ih_l{l}").value, ptr(f"gru.gru.weight_hh_l{l}").value
        p.gru_b_ih[l], p.gru_b_hh[l] = ptr(f"gru.gru.bias_ih_l{l}").value, ptr(f"gru.gru.bias_hh_l{l}").value
    for i in range(cfg["forecast_n_linear"]):
        p.fc_weight[i] = ptr(f"forecasting_model.layers.{i}.weight").value
        p.fc_bias[i] = ptr(f"forecasting_model.layers.{i}.bias").value
    for l in range(cfg["recon_n_layers"]):
        pre = "recon_model.decoder.rnn."
        p.rec_w_ih[l], p.rec_w_hh[l] = ptr(f"{pre}weight_ih_l{l}").value, ptr(f"{pre}weight_hh_l{l}").value
        p.rec_b_ih[l], p.rec_b_hh[l] = ptr(f"{pre}bias_ih_l{l}").value, ptr(f"{pre}bias_hh_l{l}").value
    p.rec_fc_weight, p.rec_fc_bias = ptr("recon_model.fc.weight"), ptr("recon_model.fc.bias")
    covered = ctypes.c_int64(0)
    bad = lib.mtadgat_selfcheck_gather_table(h, ctypes.byref(p), ctypes.byref(covered))
    assert bad == 0, (F, bad, lib.mtadgat_last_error())
    n_copied = sum(v.numel() for k, v in sd.items() if not k.startswith(("feature_gat", "temporal_gat")))
    assert covered.value >= n_copied
    assert lib.mtadgat_destroy(h) == 0
