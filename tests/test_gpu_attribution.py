"""Score attribution on the GPU (MTAD_GAT.score_attribution -> mtadgat_score_attribution: gather / seed / combine kernels of
csrc/mtadgat_attrib.hip around the training forward and the data-only backward) against the CPU route (torch ops +
torch.autograd.grad with respect to the slices), same weights; the data-only backward (mtadgat_backward_data) against
mtadgat_backward + mtadgat_backward_input bit for bit; determinism, chunking, and that the call leaves the model alone.

Gate: 1e-5 + 1e-4 * max|ref| per attribution tensor."""
import copy

import pytest
import torch

from helpers import Case

pytestmark = pytest.mark.gpu

SMALL = dict(gru_hid_dim=32, forecast_n_layers=1, forecast_hid_dim=24, recon_hid_dim=28, dropout=0.3, alpha=0.2)
MODELS = {
    # name: (ctor kwargs or a golden case, target_dims, gamma, scale_scores)
    "msl_checkpoint": ("msl", [0], 1.0, False),
    "smd_out_f": (dict(n_features=38, window_size=100, out_dim=38, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3,
                       forecast_hid_dim=150, recon_hid_dim=150, dropout=0.3, alpha=0.2), None, 1.0, False),
    "gat_v1": (dict(n_features=9, window_size=20, out_dim=3, kernel_size=5, use_gatv2=False, feat_gat_embed_dim=5, time_gat_embed_dim=6,
                    **SMALL), [1, 4, 8], 1.0, False),
    "stacked": (dict(n_features=7, window_size=16, out_dim=2, kernel_size=3, gru_n_layers=2, recon_n_layers=2, **SMALL), [0, 6], 1.0,
                False),
    "gamma_scaled": (dict(n_features=12, window_size=30, out_dim=12, kernel_size=5, **SMALL), None, 0.4, True),
    "f513": (dict(n_features=513, window_size=12, out_dim=3, kernel_size=3, **SMALL), [0, 100, 512], 1.0, False),
    # W F = 22 400 > 16 384: the input gradient of the wide-window convolution (k_conv over the flipped kernel), wide attention
    "wide_window": (dict(n_features=140, window_size=160, out_dim=2, kernel_size=5, feat_gat_embed_dim=21, time_gat_embed_dim=9, **SMALL),
                    [3, 77], 1.0, False),
}


def _model(spec, seed=0):
    from mtad_gat import MTAD_GAT
    if isinstance(spec, str):
        return Case(spec).build_model().eval()
    torch.manual_seed(seed)
    m = MTAD_GAT(**spec).eval()
    with torch.no_grad():
        m.feature_gat.bias.normal_()
        m.temporal_gat.bias.normal_()
    return m


def _series(model, n_extra, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(model.window_size + 1 + n_extra, model.n_features, generator=g)


def _gate(out, ref, what):
    assert out.shape == ref.shape and out.dtype == torch.float32, what
    d, scale = (out.cpu() - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: |gpu - cpu| = {d:.3e}, scale {scale:.3e}")
    assert torch.isfinite(out).all() and d <= 1e-5 + 1e-4 * scale, what
    assert scale > 0, what


@pytest.mark.parametrize("name", list(MODELS))
def test_gpu_matches_cpu_route(name, gpu_device):
    spec, dims, gamma, scaled = MODELS[name]
    cpu = _model(spec)
    values = _series(cpu, 9, 1)
    idx = [0, 4, 9]
    gpu = copy.deepcopy(cpu).to(gpu_device)
    vg = values.to(gpu_device)
    kw = dict(target_dims=dims, gamma=gamma, scale_scores=scaled)
    for method, extra in (("gradient", {}), ("integrated", dict(steps=8)), ("integrated", dict(steps=8, baseline=values.mean(0)))):
        ref = cpu.score_attribution(values, idx, method=method, **extra, **kw)
        if "baseline" in extra:
            extra = dict(extra, baseline=extra["baseline"].to(gpu_device))
        out = gpu.score_attribution(vg, idx, method=method, **extra, **kw)
        assert out.device == vg.device
        _gate(out, ref, f"{name} {method} {sorted(extra)}")


def test_slice_baseline_and_empty(gpu_device):
    spec = MODELS["gat_v1"][0]
    cpu = _model(spec)
    values = _series(cpu, 5, 2)
    base = torch.rand(cpu.window_size + 1, cpu.n_features, generator=torch.Generator().manual_seed(3))
    ref = cpu.score_attribution(values, [1, 5], [1, 4, 8], method="integrated", steps=5, baseline=base)
    gpu = copy.deepcopy(cpu).to(gpu_device)
    out = gpu.score_attribution(values.to(gpu_device), [1, 5], [1, 4, 8], method="integrated", steps=5, baseline=base.to(gpu_device))
    _gate(out, ref, "slice baseline")
    empty = gpu.score_attribution(values.to(gpu_device), [], [1, 4, 8])
    assert empty.shape == (0, cpu.window_size + 1, cpu.n_features) and empty.device.type == "cuda"
    with pytest.raises(IndexError):
        gpu.score_attribution(values.to(gpu_device), [values.shape[0] - cpu.window_size], [1, 4, 8])


def test_deterministic_chunk_independent_and_stateless(gpu_device):
    """Identical calls give identical bits; a chunk of 2 windows (one unit) gives the result of the default chunk within the gate;
    self.training, the precision setting, every .grad and the next forward are untouched."""
    spec, dims, _, _ = MODELS["stacked"]
    model = _model(spec).to(gpu_device).train()
    model.precision = "fp32"
    values = _series(model, 40, 4).to(gpu_device)
    idx = list(range(0, 40, 3))
    x = values[:model.window_size][None].repeat(3, 1, 1)
    model.eval()
    with torch.no_grad():
        before = model(x)
    model.train()
    for p in model.parameters():
        p.grad = None
    a1 = model.score_attribution(values, idx, dims, method="integrated", steps=6)
    a2 = model.score_attribution(values, idx, dims, method="integrated", steps=6)
    assert torch.equal(a1, a2)
    g1 = model.score_attribution(values, idx, dims)
    assert torch.equal(g1, model.score_attribution(values, idx, dims))
    eng = model._engine
    default_chunk = eng.chunk_windows()
    try:
        for chunk in (2, 7):
            eng.set_chunk_windows(chunk)
            c = model.score_attribution(values, idx, dims, method="integrated", steps=6)
            assert (c - a1).abs().max().item() <= 1e-5 + 1e-4 * a1.abs().max().item(), chunk
    finally:
        eng.set_chunk_windows(default_chunk)
    assert model.training and model.precision == "fp32"
    assert all(p.grad is None for p in model.parameters())
    model.eval()
    with torch.no_grad():
        after = model(x)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


@pytest.mark.parametrize("name,batch", [("odd_small", 5), ("odd_large_band", 4200), ("v1_small", 9), ("msl_shape", 7),
                                        ("wide_window", 3)])
def test_data_only_backward_is_bit_identical(name, batch, gpu_device):
    """mtadgat_backward_data's d x equals mtadgat_backward + mtadgat_backward_input on the same chunk bit for bit, at a small batch
    and at 4 200 windows (the throughput recurrences past 4 096 windows, split-operand row GEMMs past 65 536 rows); it takes no
    gradient buffer, and the flat gradient buffer of an earlier backward is not written by it."""
    specs = {
        "odd_small": dict(n_features=12, window_size=30, out_dim=12, kernel_size=5, **SMALL),
        "odd_large_band": dict(n_features=12, window_size=30, out_dim=12, kernel_size=5, **SMALL),
        "v1_small": MODELS["gat_v1"][0],
        "msl_shape": dict(n_features=55, window_size=100, out_dim=1, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3,
                          forecast_hid_dim=150, recon_hid_dim=150, dropout=0.3, alpha=0.2),
        "wide_window": MODELS["wide_window"][0],
    }
    kw = specs[name]
    model = _model(kw).to(gpu_device)
    eng = model._sync_engine(gpu_device)
    g = torch.Generator().manual_seed(8)
    W, F, od = kw["window_size"], kw["n_features"], kw["out_dim"]
    x = torch.rand(batch, W, F, generator=g).to(gpu_device)
    dp = torch.randn(batch, od, generator=g).to(gpu_device)
    dr = torch.randn(batch, W, od, generator=g).to(gpu_device)
    for p_drop, seed in ((0.0, 0), (0.3, 1234)):
        _, _, tape = eng.forward_train(x, p_drop, seed)
        offs, total = eng.grad_layout()
        grads = torch.zeros(total, device=gpu_device)
        eng.backward(x, p_drop, seed, dp, dr, tape, grads)
        dx_full = eng.backward_input(x)
        snapshot = grads.clone()
        dx_data = eng.backward_data(x, p_drop, seed, dp, dr, tape)
        torch.cuda.synchronize()
        assert torch.isfinite(dx_data).all() and dx_data.abs().sum() > 0
        assert torch.equal(dx_data, dx_full), (name, p_drop, (dx_data - dx_full).abs().max().item())
        assert torch.equal(grads, snapshot)


def test_device_repack_keeps_matching_the_host_packer(gpu_device):
    """A model whose windows exceed 64 KB carries the flipped-kernel pack of the input gradient: the device re-pack rebuilds it
    like every other plain-copy region, bit for bit."""
    from mtad_gat import MTAD_GAT
    torch.manual_seed(0)
    model = MTAD_GAT(**MODELS["wide_window"][0]).to(gpu_device).eval()
    eng = model._sync_engine(gpu_device)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.01 * torch.randn_like(p))
    sd = model.state_dict()
    assert eng.update_weights_device(sd, gpu_device)
    img_dev = eng.read_packed(gpu_device)
    eng.load_weights(sd, gpu_device, allow_device_pack=False)
    img_host = eng.read_packed(gpu_device)
    mism = img_dev.view(torch.int32) != img_host.view(torch.int32)
    for off, n in eng.derived_regions():
        mism[off:off + n] = False
    assert mism.float().mean().item() < 0.02
    if mism.any():
        assert (img_dev[mism] - img_host[mism]).abs().max().item() <= 1e-6 * max(img_host[mism].abs().max().item(), 1.0)
