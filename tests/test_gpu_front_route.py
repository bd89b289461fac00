"""The launch helpers launch what front_route names: for each front-end route the options can force at a small shape, one forward with
profiling on, and the bracketed scope counts (mtadgat_profile_read) must be those the route reported by mtadgat_front_route for the
same handle and window count implies -- convolution scopes: 0 with the convolution inside k_gath, 1 for k_conv_win or launch_conv, 4
for the shared rows of a series (three launches and the row placement); projection scopes: one per un-fused layer; attention scopes:
one per layer.  (What the routes compute is checked by test_gpu_gath.py, test_gpu_parity.py, test_gpu_shapes.py and
test_gpu_stream.py; which route a call gets, without a GPU, by test_host_front_route.py.)

Shapes: the smallest the host route accepts -- k_gath's convolution needs the temporal layer's eight-wave workgroup (97 or more time
steps), the un-fused layers more than 128 nodes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FUSED = dict(n_features=9, window_size=100, out_dim=2, kernel_size=5, gru_hid_dim=16, forecast_n_layers=1, forecast_hid_dim=8, recon_hid_dim=16)
UNFUSED = dict(n_features=5, window_size=140, out_dim=5, kernel_size=3, gru_hid_dim=16, forecast_n_layers=1, forecast_hid_dim=8, recon_hid_dim=16)

CASES = {
    # name: (model, options, windows, series, the route's convolution, un-fused layers)
    "conv_in_gath": (FUSED, dict(conv_kernel=2, gat_kernel=3), 24, False, "in_gath", 0),
    "conv_win": (FUSED, dict(conv_kernel=2, gat_kernel=3, conv_fused=1), 24, False, "k_conv_win", 0),
    "conv_lds": (FUSED, dict(conv_kernel=1), 24, False, "launch_conv", 0),
    "shared_rows": (FUSED, dict(conv_kernel=2, conv_shared=1), 1024, True, "shared_rows", 0),
    "unfused": (UNFUSED, dict(), 8, False, "launch_conv", 2),
}


def _implied(r):
    conv = {0: 0, 1: 1, 2: 4, 3: 1}[r["conv"]]
    layers = (r["temp_kernel"], r["feat_kernel"])
    return conv, sum(k in (3, 4) for k in layers), sum(k != 0 for k in layers)


@pytest.mark.parametrize("name", list(CASES))
def test_scopes_are_those_the_route_implies(name, gpu_device):
    import _native
    from mtad_gat import MTAD_GAT
    kw, options, n, series, conv, unfused = CASES[name]
    torch.manual_seed(11)
    model = MTAD_GAT(**kw).eval().to(gpu_device)
    eng = model._sync_engine(gpu_device)
    W, F = kw["window_size"], kw["n_features"]
    try:
        for key, v in options.items():
            eng.set_option(key, v)
        r = eng.front_route(_native.FRONT_KINDS.index("forward"), _native.FRONT_SOURCES.index("series_unit" if series else "windows"), n)
        # the case is the one its name says (the host route decides; test_host_front_route.py pins it)
        assert _native.FRONT_CONVS[r["conv"]] == conv and _implied(r)[1] == unfused, r
        if name == "conv_in_gath":
            assert r["temp_kernel"] == _native.FRONT_LAYERS.index("k_gath+k_gat"), r
        eng.profile_enable(True)
        eng.profile_read()
        with torch.no_grad():
            if series:
                p, rec = model.forward_series(torch.rand(n + W - 1, F, device=gpu_device))
            else:
                p, rec = model(torch.rand(n, W, F, device=gpu_device))
        torch.cuda.synchronize()
        prof = eng.profile_read()
        got = tuple(prof[k][1] for k in ("conv", "proj", "attend"))
        print(f"{name}: route {r} -> scopes (conv, proj, attend) = {got}")
        assert got == _implied(r), (got, r)
        assert p.shape[0] == n and torch.isfinite(p).all() and torch.isfinite(rec).all()
    finally:
        eng.profile_enable(False)
        for key in options:
            eng.set_option(key, 0)
