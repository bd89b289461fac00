"""x.requires_grad on models whose windows exceed 64 KB (W F > 16 384 floats): the HIP training step returns d loss / d x through the
convolution of the pre-activation gradients with the flipped, transposed kernel (k_conv over the conv_wT pack) -- against
autograd through the torch-op algebra, as tests/test_gpu_backward.py::test_input_gradient_matches_autograd does for small
windows.  W F = 16 384 is the control that still takes k_conv_dx."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SMALL = dict(gru_hid_dim=24, forecast_n_layers=1, forecast_hid_dim=16, recon_hid_dim=20, dropout=0.2, alpha=0.2)
CONFIGS = {
    "control_f128_w128": (dict(n_features=128, window_size=128, out_dim=3, kernel_size=5, feat_gat_embed_dim=16, time_gat_embed_dim=16,
                               **SMALL), 3),
    "f129_w128": (dict(n_features=129, window_size=128, out_dim=3, kernel_size=5, feat_gat_embed_dim=16, time_gat_embed_dim=16, **SMALL), 3),
    "f140_w160": (dict(n_features=140, window_size=160, out_dim=2, kernel_size=3, use_gatv2=False, feat_gat_embed_dim=12,
                       time_gat_embed_dim=10, **SMALL), 2),
    "config4_f512_w256": (dict(n_features=512, window_size=256, out_dim=512, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3,
                               forecast_hid_dim=150, recon_hid_dim=150, dropout=0.3, alpha=0.2), 2),
    "f2048_w40": (dict(n_features=2048, window_size=40, out_dim=4, kernel_size=3, feat_gat_embed_dim=8, time_gat_embed_dim=16, **SMALL), 1),
}


def _loss(preds, recons, x, y):
    return torch.sqrt(F.mse_loss(y, preds)) + torch.sqrt(F.mse_loss(x[:, :, : recons.shape[2]], recons))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_wide_window_input_gradient_matches_autograd(name, gpu_device):
    import _torchpath
    from mtad_gat import MTAD_GAT
    kw, b = CONFIGS[name]
    torch.manual_seed(0)
    model = MTAD_GAT(**kw).to(gpu_device).eval()
    g = torch.Generator().manual_seed(13)
    x0 = torch.rand(b, kw["window_size"], kw["n_features"], generator=g).to(gpu_device)
    y = torch.rand(b, kw["out_dim"], generator=g).to(gpu_device)
    xr = x0.clone().requires_grad_(True)
    with torch.backends.cudnn.flags(enabled=False):
        pr, rc = _torchpath.forward(model, xr)
        dx_ref = torch.autograd.grad(_loss(pr, rc, xr, y), xr)[0]
    x = x0.clone().requires_grad_(True)
    pr, rc = model(x)
    assert model.grad_path == "hip", model.grad_path
    _loss(pr, rc, x, y).backward()
    assert x.grad is not None and x.grad.shape == x.shape and torch.isfinite(x.grad).all()
    d, scale = (x.grad - dx_ref).abs().max().item(), dx_ref.abs().max().item()
    print(f"{name}: |dx - ref| = {d:.3e}, scale {scale:.3e}")
    assert scale > 0 and d <= 1e-6 + 1e-4 * scale
