"""The HIP training step of models with more than 512 features: training forward through the score-matrix path (softmax rows
kept on the tape, counter-based dropout applied in the aggregation GEMM), backward through mtadgat_bwdw.hip beyond 512 keys
(k_bw_softmax / k_bw_v1 with 32 keys per lane, k_bw_pair in segments of 512 keys).  Against autograd through the torch-op
algebra (_torchpath.py) on the same device and weights, gate 1e-5 + 1e-4 * scale as tests/test_gpu_backward.py; and the device
re-pack of such models against the host packer."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CONFIGS = {
    # temporal layer D = F = 513 (E = 1026), feature layer K = 513: k_bw_pair with two key segments (512 + 1)
    "f513_v2": (dict(n_features=513, window_size=12, out_dim=3, kernel_size=3, gru_hid_dim=24, forecast_n_layers=1,
                     forecast_hid_dim=16, recon_hid_dim=20, dropout=0.2, alpha=0.2), 3),
    # three key segments, the last one partial
    "f1100_v2": (dict(n_features=1100, window_size=6, out_dim=2, kernel_size=3, gru_hid_dim=16, forecast_n_layers=1,
                      forecast_hid_dim=8, recon_hid_dim=16, dropout=0.2, alpha=0.1), 2),
    "f777_v1": (dict(n_features=777, window_size=10, out_dim=4, kernel_size=5, use_gatv2=False, feat_gat_embed_dim=13,
                     time_gat_embed_dim=40, gru_hid_dim=20, forecast_n_layers=2, forecast_hid_dim=16, recon_hid_dim=20,
                     dropout=0.3, alpha=0.2), 3),
}


def _model(kw, device, seed=0):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(seed)
    m = MTAD_GAT(**kw)
    with torch.no_grad():
        m.feature_gat.bias.normal_()
        m.temporal_gat.bias.normal_()
    return m.to(device)


def _loss(preds, recons, x, y):
    return torch.sqrt(F.mse_loss(y, preds)) + torch.sqrt(F.mse_loss(x[:, :, : recons.shape[2]], recons))


def _reference_grads(model, x, y, masks=None):
    import _torchpath
    for p in model.parameters():
        p.grad = None
    with torch.backends.cudnn.flags(enabled=False):
        pr, rc = _torchpath.forward(model, x, masks)
        _loss(pr, rc, x, y).backward()
    ref = {n: p.grad.clone() for n, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    return pr.detach(), rc.detach(), ref


def _check_grads(model, ref, tol_abs=1e-5, tol_rel=1e-4):
    bad = []
    for name, p in model.named_parameters():
        g, r = p.grad, ref[name]
        if g is None:
            bad.append(f"{name}: no gradient")
            continue
        d, scale = (g - r).abs().max().item(), r.abs().max().item()
        if not (d <= tol_abs + tol_rel * scale) or not torch.isfinite(g).all():
            bad.append(f"{name} |diff|={d:.3e} scale={scale:.3e}")
    assert not bad, "\n".join(bad)


def _data(kw, b, seed, device):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(b, kw["window_size"], kw["n_features"], generator=g).to(device)
    y = torch.rand(b, kw["out_dim"], generator=g).to(device)
    return x, y


@pytest.mark.parametrize("name", list(CONFIGS))
def test_wide_feature_gradients_eval_mode(name, gpu_device):
    kw, b = CONFIGS[name]
    model = _model(kw, gpu_device).eval()
    x, y = _data(kw, b, 11, gpu_device)
    pr_ref, rc_ref, ref = _reference_grads(model, x, y)
    pr, rc = model(x)
    assert model.grad_path == "hip", model.grad_path
    assert (pr - pr_ref).abs().max().item() <= 1e-5 and (rc - rc_ref).abs().max().item() <= 1e-5
    _loss(pr, rc, x, y).backward()
    _check_grads(model, ref)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_wide_feature_gradients_with_dropout(name, gpu_device):
    kw, b = CONFIGS[name]
    model = _model(kw, gpu_device).train()
    x, y = _data(kw, b, 12, gpu_device)
    torch.manual_seed(77)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())       # what _hipgrad.forward will draw
    torch.manual_seed(77)
    pr, rc = model(x)
    assert model.grad_path == "hip"
    masks = model._engine.dropout_masks(b, kw["dropout"], seed, gpu_device)
    _loss(pr, rc, x, y).backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters()}
    pr_ref, rc_ref, ref = _reference_grads(model, x, y, masks)
    assert (pr - pr_ref).abs().max().item() <= 1e-5 and (rc - rc_ref).abs().max().item() <= 1e-5
    for n, p in model.named_parameters():
        p.grad = got[n]
    _check_grads(model, ref)


def test_wide_feature_input_gradient_and_chunked_step(gpu_device, monkeypatch):
    """d loss / d x against autograd, and a step walked in chunks of 2 windows equal to the one-chunk step (dropout on)."""
    import _hipgrad
    import _torchpath
    kw, _ = CONFIGS["f513_v2"]
    b = 5
    model = _model(kw, gpu_device).eval()
    x0, y = _data(kw, b, 13, gpu_device)
    xr = x0.clone().requires_grad_(True)
    with torch.backends.cudnn.flags(enabled=False):
        pr, rc = _torchpath.forward(model, xr)
        _loss(pr, rc, xr, y).backward()
    dx_ref = xr.grad.clone()
    for p in model.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    pr, rc = model(x)
    assert model.grad_path == "hip"
    _loss(pr, rc, x, y).backward()
    d, scale = (x.grad - dx_ref).abs().max().item(), dx_ref.abs().max().item()
    assert d <= 1e-6 + 1e-4 * scale, (d, scale)

    model.train()

    def step():
        for p in model.parameters():
            p.grad = None
        torch.manual_seed(5)
        pr, rc = model(x0)
        _loss(pr, rc, x0, y).backward()
        return pr.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}

    p1, g1 = step()
    monkeypatch.setattr(_hipgrad, "TRAIN_CHUNK", 2)            # 5 windows -> 2 + 2 + 1
    p2, g2 = step()
    assert torch.equal(p1, p2)
    for n in g1:
        dd = (g1[n] - g2[n]).abs().max().item()
        assert dd <= 1e-6 + 1e-5 * g1[n].abs().max().item(), (n, dd)


@pytest.mark.parametrize("F_", [1024, 2048])
def test_wide_feature_device_repack_equals_the_host_packer(F_, gpu_device):
    """After an optimizer step the image re-packed on the device (two-run gather table above 2^24 parameters, integer column
    codes) equals the host packer's (pattern of tests/test_gpu_device_pack.py)."""
    from mtad_gat import MTAD_GAT
    kw = dict(n_features=F_, window_size=12, out_dim=3, kernel_size=3, gru_hid_dim=16, forecast_n_layers=1, forecast_hid_dim=8,
              recon_hid_dim=16, dropout=0.0)
    torch.manual_seed(0)
    model = MTAD_GAT(**kw).to(gpu_device).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    x, y = _data(kw, 2, 14, gpu_device)
    pr, rc = model(x)
    assert model.grad_path == "hip"
    _loss(pr, rc, x, y).backward()
    opt.step()
    with torch.no_grad():
        for a in (model.feature_gat.a, model.temporal_gat.a):  # move embedding columns across the sign boundary
            a.mul_(torch.where(torch.rand(a.shape, device=a.device) < 0.3, -1.0, 1.0))
    eng = model._sync_engine(gpu_device)
    sd = model.state_dict()
    assert eng.update_weights_device(sd, gpu_device), "the library declined the device-side re-pack"
    img_dev = eng.read_packed(gpu_device)
    eng.load_weights(sd, gpu_device, allow_device_pack=False)
    img_host = eng.read_packed(gpu_device)
    mism = img_dev.view(torch.int32) != img_host.view(torch.int32)
    for off, n in eng.derived_regions():
        mism[off:off + n] = False
    assert mism.float().mean().item() < 0.02, int(mism.sum())
    if mism.any():
        a, b = img_dev[mism], img_host[mism]
        assert (a - b).abs().max().item() <= 1e-6 * max(b.abs().max().item(), 1.0)
