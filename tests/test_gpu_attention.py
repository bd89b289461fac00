"""Attention maps on the GPU (MTAD_GAT.attention_maps / attention_series, mtadgat_attention*): per-window maps against the oracle on
every attention route (fused k_gat, k_gat_wide, k_attend), chunking, the series gather, the mean reduction (k_att_mean_part /
k_att_mean_final), independence from the precision mode, and that the call leaves the handle's forward unchanged."""
import pytest
import torch

from helpers import ALL_CASES, Case, gate
from oracle import mtad_gat_oracle as oracle

pytestmark = pytest.mark.gpu


def _oracle_maps(model, x, dtype):
    sd = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()}
    xc = oracle.conv_layer(x.cpu().to(dtype), sd["conv.conv.weight"], sd["conv.conv.bias"])
    v2 = model.feature_gat.use_gatv2
    _, af = oracle.graph_attention(xc.permute(0, 2, 1), sd["feature_gat.lin.weight"], sd["feature_gat.lin.bias"], sd["feature_gat.a"],
                                   sd.get("feature_gat.bias"), model.alpha, v2)
    _, at = oracle.graph_attention(xc, sd["temporal_gat.lin.weight"], sd["temporal_gat.lin.bias"], sd["temporal_gat.a"],
                                   sd.get("temporal_gat.bias"), model.alpha, v2)
    return af, at


def _check_against_oracle(model, x, af, at, what):
    rf, rt = _oracle_maps(model, x, torch.float32)
    rf64, rt64 = _oracle_maps(model, x, torch.float64)
    gate(af, rf, rf64, tol=1e-5, what=f"{what} feature maps")
    gate(at, rt, rt64, tol=1e-5, what=f"{what} temporal maps")
    assert (af.double().sum(-1) - 1).abs().max().item() <= 1e-5
    assert (at.double().sum(-1) - 1).abs().max().item() <= 1e-5


def _model(kw, seed=11):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(seed)
    model = MTAD_GAT(**kw).eval()
    with torch.no_grad():
        model.feature_gat.bias.normal_()
        model.temporal_gat.bias.normal_()
    return model


@pytest.mark.parametrize("name", ALL_CASES)
def test_fused_route_against_oracle(name, gpu_device):
    case = Case(name)
    model = case.build_model()
    x = case.x
    m = model.to(gpu_device)
    af, at = m.attention_maps(x.to(gpu_device))
    assert af.device.type == "cuda" and af.dtype == torch.float32
    assert af.shape == (x.shape[0], model.n_features, model.n_features) and at.shape == (x.shape[0], model.window_size, model.window_size)
    _check_against_oracle(model, x, af, at, name)


WIDE = [
    # k_gat_wide (129 .. 512 nodes / node dimensions) for both layers
    dict(n_features=140, window_size=300, out_dim=2, kernel_size=5, gru_hid_dim=24, forecast_hid_dim=16, recon_hid_dim=20),
    dict(n_features=140, window_size=300, out_dim=2, kernel_size=5, use_gatv2=False, gru_hid_dim=24, forecast_hid_dim=16, recon_hid_dim=20),
    # k_attend (more than 512 features): the score matrix is the map
    dict(n_features=513, window_size=12, out_dim=3, kernel_size=3, gru_hid_dim=24, forecast_hid_dim=16, recon_hid_dim=20),
    dict(n_features=513, window_size=20, out_dim=3, kernel_size=3, use_gatv2=False, gru_hid_dim=24, forecast_hid_dim=16, recon_hid_dim=20),
]


@pytest.mark.parametrize("kw", WIDE, ids=["wide_v2", "wide_v1", "attend_v2", "attend_v1"])
def test_unfused_routes_against_oracle(kw, gpu_device):
    model = _model(kw)
    x = torch.rand(3, kw["window_size"], kw["n_features"])
    m = model.to(gpu_device)
    af, at = m.attention_maps(x.to(gpu_device))
    _check_against_oracle(model, x, af, at, str(kw["n_features"]))
    mf, mt = m.attention_maps(x.to(gpu_device), reduce="mean")
    assert (mf.double() - af.double().mean(0)).abs().max().item() <= 1e-6
    assert (mt.double() - at.double().mean(0)).abs().max().item() <= 1e-6


def test_chunks_and_large_call(gpu_device):
    case = Case("msl")
    model = case.build_model().to(gpu_device)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(4100, model.window_size, model.n_features, generator=g).to(gpu_device)
    af, at = model.attention_maps(x)
    sel = torch.tensor([0, 1, 2047, 2048, 4095, 4096, 4099])
    _check_against_oracle(model, x[sel].cpu(), af[sel], at[sel], "4100 windows")
    # ragged chunks: 23 windows in chunks of 7 equal the one-chunk call, per window and for the mean
    xs = x[:23]
    ref = model.attention_maps(xs)
    ref_mean = model.attention_maps(xs, reduce="mean")
    eng = model._sync_engine(gpu_device)
    chunk = eng.chunk_windows()
    try:
        eng.set_chunk_windows(7)
        got = eng.attention(xs)
        got_mean = eng.attention(xs, reduce=True)
    finally:
        eng.set_chunk_windows(chunk)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    for a, b in zip(got_mean, ref_mean):
        assert (a.double() - b.double()).abs().max().item() <= 1e-6


def test_series_equals_materialised_windows(gpu_device):
    case = Case("smap")
    model = case.build_model().to(gpu_device)
    W = model.window_size
    g = torch.Generator().manual_seed(9)
    series = torch.rand(W + 300, model.n_features, generator=g).to(gpu_device)
    starts = torch.tensor([17, 0, 300, 5, 5, 123], dtype=torch.int64, device=gpu_device)
    for kw, s_list in ((dict(stride=1), list(range(301))), (dict(stride=3, start=2, count=90), list(range(2, 272, 3))),
                       (dict(starts=starts), starts.tolist())):
        x = torch.stack([series[s:s + W] for s in s_list])
        af, at = model.attention_series(series, reduce=None, **kw)
        rf, rt = model.attention_maps(x)
        assert torch.equal(af, rf) and torch.equal(at, rt), kw
        mf, mt = model.attention_series(series, **kw)
        rmf, rmt = model.attention_maps(x, reduce="mean")
        assert torch.equal(mf, rmf) and torch.equal(mt, rmt), kw


def test_mean_accuracy_and_determinism_65536_windows(gpu_device):
    """65 536 MSL windows of a series: the mean within 1e-6 of the float64 mean of the per-window maps, identical bits from two
    calls, and no allocation of the 3.4 GB of per-window maps."""
    case = Case("msl")
    model = case.build_model().to(gpu_device)
    W, F = model.window_size, model.n_features
    n = 65536
    g = torch.Generator().manual_seed(5)
    series = torch.rand(n + W - 1, F, generator=g).to(gpu_device)
    model.attention_series(series, count=256)                 # warm-up (engine, packed weights)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(gpu_device)
    torch.cuda.reset_peak_memory_stats(gpu_device)
    mf, mt = model.attention_series(series)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(gpu_device) - base
    assert peak < n * (F * F + W * W) * 4 // 3, f"{peak / 2**20:.0f} MiB"
    mf2, mt2 = model.attention_series(series)
    assert torch.equal(mf, mf2) and torch.equal(mt, mt2)
    sf = torch.zeros(F, F, dtype=torch.float64, device=gpu_device)
    st = torch.zeros(W, W, dtype=torch.float64, device=gpu_device)
    step = 8192
    for s0 in range(0, n, step):
        af, at = model.attention_series(series, start=s0, count=step, reduce=None)
        sf += af.double().sum(0)
        st += at.double().sum(0)
    assert (mf.double() - sf / n).abs().max().item() <= 1e-6
    assert (mt.double() - st / n).abs().max().item() <= 1e-6
    assert abs(mt.double().sum(-1) - 1).max().item() <= 1e-5


def test_precision_modes_and_no_state_left(gpu_device):
    case = Case("msl")
    model = case.build_model().to(gpu_device)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(300, model.window_size, model.n_features, generator=g).to(gpu_device)
    p0, r0 = model(x)
    ref = model.attention_maps(x)
    p1, r1 = model(x)
    assert torch.equal(p0, p1) and torch.equal(r0, r1)
    eng = model._sync_engine(gpu_device, bf16=True)           # mode 1 with its bf16 weight streams
    for mode in (0, 1, 2):
        eng.set_precision(mode)
        for reduce in (False, True):
            got = eng.attention(x, reduce=reduce)
            want = ref if not reduce else tuple(a.double().mean(0) for a in ref)
            for a, b in zip(got, want):
                assert (a.double() - b.double()).abs().max().item() <= 1e-6, (mode, reduce)
    # a handle in mode 1 whose bf16 streams were never packed is served as well
    from mtad_gat import MTAD_GAT
    fresh = MTAD_GAT(**case.kwargs).eval()
    fresh.load_state_dict(model.state_dict())
    fresh = fresh.to(gpu_device)
    e2 = fresh._sync_engine(gpu_device)
    e2.set_precision(1)
    got = e2.attention(x)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    # train() mode: eval-mode maps, the flag untouched, nothing recorded for autograd
    model.train()
    got = model.attention_maps(x)
    assert model.training and not got[0].requires_grad
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    model.eval()
    p2, r2 = model(x)
    assert torch.equal(p0, p2) and torch.equal(r0, r2)
    # either output alone; reduced-precision inputs give float32 maps
    af, at = eng.attention(x, feat=False)
    assert af is None and torch.equal(at, ref[1])
    af, at = model.attention_maps(x.bfloat16())
    assert af.dtype == torch.float32 and at.dtype == torch.float32
