"""Models with more than 512 features (up to 2048) on the GPU: both attention layers go through the score-matrix path
(k_attend + softmax + the sigmoid epilogue of k_bgemm).  Forward against the oracle at 1e-5, the other arithmetics, the
series entry points, chunking; the training step's gradients are checked in test_gpu_wide_features_training.py."""
import pytest
import torch

from helpers import gate
from oracle import mtad_gat_oracle as oracle

pytestmark = pytest.mark.gpu

SHAPES = [
    (dict(n_features=513, window_size=12, out_dim=3, kernel_size=3, gru_hid_dim=24, forecast_hid_dim=16, recon_hid_dim=20), (1, 35)),
    (dict(n_features=777, window_size=30, out_dim=5, kernel_size=5, use_gatv2=False, feat_gat_embed_dim=13, time_gat_embed_dim=40,
          gru_n_layers=2, gru_hid_dim=33, forecast_n_layers=2, forecast_hid_dim=24, recon_n_layers=2, recon_hid_dim=35), (1, 35)),
    (dict(n_features=1024, window_size=100, out_dim=1, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3, forecast_hid_dim=150,
          recon_hid_dim=150), (1, 2)),
    (dict(n_features=2048, window_size=8, out_dim=2048, kernel_size=3, gru_hid_dim=32, forecast_hid_dim=32, recon_hid_dim=32), (1, 3)),
]


def _model(kw, seed=17):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(seed)
    model = MTAD_GAT(**kw).eval()
    with torch.no_grad():
        model.feature_gat.bias.normal_()
        model.temporal_gat.bias.normal_()
    return model


@pytest.mark.parametrize("kw, batches", SHAPES, ids=["F513W12", "F777W30v1", "F1024W100", "F2048W8"])
def test_wide_feature_forward_against_oracle(kw, batches, gpu_device):
    model = _model(kw)
    sd = model.state_dict()
    m = model.to(gpu_device)
    for b in batches:
        x = torch.rand(b, kw["window_size"], kw["n_features"])
        with torch.no_grad():
            p_ref, r_ref = oracle.forward(x, sd, alpha=kw.get("alpha", 0.2))
            p, r = m(x.to(gpu_device))
        gate(p, p_ref, what=f"preds b={b}")
        gate(r, r_ref, what=f"recons b={b}")


def test_wide_feature_arithmetics(gpu_device):
    kw = SHAPES[0][0]
    model = _model(kw, seed=5)
    x = torch.rand(35, kw["window_size"], kw["n_features"])
    with torch.no_grad():
        p_ref, r_ref = oracle.forward(x, model.state_dict(), alpha=0.2)
        m = model.to(gpu_device)
        xd = x.to(gpu_device)
        for prec in ("fp32", "fp32_strict"):
            m.precision = prec
            p, r = m(xd)
            gate(p, p_ref, what=f"preds {prec}")
            gate(r, r_ref, what=f"recons {prec}")
        m.precision = "auto"
        p, r = m(xd.bfloat16())
    assert p.dtype == torch.bfloat16
    gate(p.float(), p_ref, tol=2e-2, what="preds bf16")
    gate(r.float(), r_ref, tol=2e-2, what="recons bf16")


def test_wide_feature_large_batch_and_chunks(gpu_device):
    """9 000 windows (large-batch recurrence kernels, split-operand projections) and a call cut into chunks of 1 000 (a call
    larger than the engine's chunk) both match the oracle on a subset of windows."""
    kw = SHAPES[0][0]
    model = _model(kw, seed=7)
    x = torch.rand(9000, kw["window_size"], kw["n_features"])
    idx = list(range(0, 20)) + list(range(8980, 9000))
    with torch.no_grad():
        p_ref, r_ref = oracle.forward(x[idx], model.state_dict(), alpha=0.2)
        m = model.to(gpu_device)
        xd = x.to(gpu_device)
        p, r = m(xd)
        gate(p[idx], p_ref, what="preds, 9000 windows")
        gate(r[idx], r_ref, what="recons, 9000 windows")
        m._engine.set_chunk_windows(1000)
        p, r = m(xd)
    gate(p[idx], p_ref, what="preds, chunked")
    gate(r[idx], r_ref, what="recons, chunked")


def test_wide_feature_series_paths(gpu_device):
    kw = SHAPES[0][0]
    model = _model(kw, seed=9).to(gpu_device)
    w = kw["window_size"]
    series = torch.rand(60, kw["n_features"])
    sd = series.to(gpu_device)
    n = series.shape[0] - w
    with torch.no_grad():
        x = torch.stack([series[i:i + w] for i in range(n + 1)]).to(gpu_device)
        p_ref, r_ref = model(x)
        p, r = model.forward_series(sd)
        assert torch.equal(p, p_ref) and torch.equal(r, r_ref)
        starts = [5, 5, 40, 0, 33]
        p, r = model.forward_series(sd, starts=torch.tensor(starts, dtype=torch.int64, device=gpu_device))
        assert torch.equal(p, p_ref[starts]) and torch.equal(r, r_ref[starts])
        preds, last = model.score_series(sd)
        assert torch.equal(preds, p_ref[:n]) and torch.equal(last, r_ref[1:, -1, :])
        scores, per_dim = model.anomaly_scores(sd, target_dims=[0, 1, 2], gamma=0.8)
        actual = series[w:, :3].to(gpu_device)
        ref = (preds - actual).abs() + 0.8 * (last - actual).abs()
        assert (per_dim - ref).abs().max().item() <= 1e-6
        assert (scores - ref.mean(1)).abs().max().item() <= 1e-6


def test_widest_model_runs_in_default_chunks(gpu_device):
    """F = 2048, W = 512 (16 MB score matrix per window): 256 windows in chunks of the default size, finite outputs, the
    first window equal (1e-5) to a call of that window alone, and a training step with finite gradients."""
    kw = dict(n_features=2048, window_size=512, out_dim=2048, kernel_size=7, gru_hid_dim=150, forecast_hid_dim=150, recon_hid_dim=150)
    model = _model(kw, seed=11).to(gpu_device)
    x = torch.rand(256, 512, 2048, device=gpu_device)
    with torch.no_grad():
        p, r = model(x)
        p1, r1 = model(x[:1])
    assert model._engine.chunk_windows() < 256
    assert torch.isfinite(p).all() and torch.isfinite(r).all()
    gate(p[:1], p1.cpu(), what="preds, first window")
    gate(r[:1], r1.cpu(), what="recons, first window")
    # and a HIP training step of the same 256 windows
    pr, rc = model(x)
    assert model.grad_path == "hip", model.grad_path
    (pr.square().mean() + rc.square().mean()).backward()
    for n, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), n
