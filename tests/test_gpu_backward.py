"""The HIP training step (mtadgat_forward_train / mtadgat_backward behind torch.autograd.Function, _hipgrad.py)
against autograd through the package's torch-op algebra (_torchpath.py, itself pinned to the oracle / the
reference by the CPU tests) on the same device, same weights, same dropout masks.

Gate: every parameter gradient within 1e-5 absolute + 1e-4 of the gradient's own scale (fp32 sums over up to
b*W rows in a different order than autograd's), outputs of the training forward within 1e-5.
"""
import pytest
import torch
import torch.nn.functional as F

from helpers import Case

pytestmark = pytest.mark.gpu

CONFIGS = {
    # name: (ctor kwargs, batch)
    "small_v2": (dict(n_features=9, window_size=16, out_dim=3, kernel_size=5, feat_gat_embed_dim=5, time_gat_embed_dim=3,
                      gru_hid_dim=33, forecast_n_layers=1, forecast_hid_dim=40, recon_hid_dim=35, dropout=0.2, alpha=0.1), 37),
    "odd_shapes": (dict(n_features=12, window_size=30, out_dim=12, kernel_size=5, gru_hid_dim=40, forecast_n_layers=2,
                        forecast_hid_dim=36, recon_hid_dim=44, dropout=0.3, alpha=0.2), 70),
    "msl_shape": (dict(n_features=55, window_size=100, out_dim=1, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3,
                       forecast_hid_dim=150, recon_hid_dim=150, dropout=0.3, alpha=0.2), 40),
    "smd_shape": (dict(n_features=38, window_size=100, out_dim=38, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3,
                       forecast_hid_dim=150, recon_hid_dim=150, dropout=0.3, alpha=0.2), 33),
    # GAT (v1) scoring (reference modules.py:80-83 / :180-183): LeakyReLU(a1 . Wx_i + a2 . Wx_j), custom embedding dims
    "v1_small": (dict(n_features=7, window_size=12, out_dim=7, kernel_size=3, use_gatv2=False, feat_gat_embed_dim=5, time_gat_embed_dim=6,
                      gru_hid_dim=20, forecast_n_layers=2, forecast_hid_dim=24, recon_hid_dim=18, dropout=0.2, alpha=0.2), 37),
    "v1_msl_shape": (dict(n_features=25, window_size=100, out_dim=1, kernel_size=7, use_gatv2=False, gru_hid_dim=150, forecast_n_layers=3,
                          forecast_hid_dim=150, recon_hid_dim=150, dropout=0.3, alpha=0.2), 20),
    # stacked recurrences: two GRU layers, two decoder layers (nn.GRU's inter-layer dropout in training)
    "stacked": (dict(n_features=6, window_size=14, out_dim=2, kernel_size=3, gru_n_layers=2, gru_hid_dim=40, forecast_n_layers=1,
                     forecast_hid_dim=20, recon_n_layers=2, recon_hid_dim=36, dropout=0.25, alpha=0.2), 21),
    "stacked3_v1": (dict(n_features=5, window_size=10, out_dim=5, kernel_size=3, use_gatv2=False, gru_n_layers=3, gru_hid_dim=33,
                         forecast_n_layers=2, forecast_hid_dim=16, recon_n_layers=1, recon_hid_dim=20, dropout=0.1, alpha=0.2), 9),
    "wide_nodes": (dict(n_features=70, window_size=120, out_dim=5, kernel_size=3, gru_hid_dim=64, forecast_n_layers=1,
                        forecast_hid_dim=32, recon_hid_dim=96, dropout=0.1, alpha=0.2), 9),
    # attention layers beyond the fused per-window kernels (more than 128 nodes or node dimensions): projections through memory +
    # k_gat_wide in the training forward, the generic backward of csrc/mtadgat_bwdw.hip (round 5)
    "wide_w130": (dict(n_features=20, window_size=130, out_dim=4, kernel_size=3, gru_hid_dim=48, forecast_n_layers=1,
                       forecast_hid_dim=32, recon_hid_dim=40, dropout=0.2, alpha=0.2), 6),
    "wide_w256": (dict(n_features=12, window_size=256, out_dim=2, kernel_size=5, feat_gat_embed_dim=40, time_gat_embed_dim=20, gru_hid_dim=40,
                       forecast_n_layers=2, forecast_hid_dim=24, recon_hid_dim=36, dropout=0.3, alpha=0.2), 3),
    # BASELINE config 4's shape (F = 512, W = 256, out = 512): both attention layers at the top of what the wide kernels take
    "config4_shape": (dict(n_features=512, window_size=256, out_dim=512, kernel_size=7, gru_hid_dim=150, forecast_n_layers=3,
                           forecast_hid_dim=150, recon_hid_dim=150, dropout=0.3, alpha=0.2), 2),
    "wide_f150": (dict(n_features=150, window_size=40, out_dim=3, kernel_size=3, feat_gat_embed_dim=33, gru_hid_dim=40, forecast_n_layers=1,
                       forecast_hid_dim=32, recon_hid_dim=40, dropout=0.1, alpha=0.1), 5),
    # GATv2 layers of 257 .. 384 nodes: the 32-key-group build of the one-pass score backward with three key quads per group
    # (k_bw_pair<3, 32>; config 4's 512 nodes take <4, 32>, everything up to 256 the 16-group builds)
    "wide_w300": (dict(n_features=9, window_size=300, out_dim=2, kernel_size=3, feat_gat_embed_dim=24, time_gat_embed_dim=12, gru_hid_dim=32,
                       forecast_n_layers=1, forecast_hid_dim=16, recon_hid_dim=24, dropout=0.2, alpha=0.2), 3),
    # GAT (v1) on wide layers (round 6: k_bw_v1, csrc/mtadgat_bwdw.hip): temporal layer of 160 nodes; feature layer of 140 nodes with
    # 300-dimensional node vectors
    "v1_wide_w160": (dict(n_features=14, window_size=160, out_dim=3, kernel_size=3, use_gatv2=False, gru_hid_dim=40, forecast_n_layers=1,
                          forecast_hid_dim=24, recon_hid_dim=36, dropout=0.2, alpha=0.2), 5),
    "v1_wide_f140": (dict(n_features=140, window_size=300, out_dim=2, kernel_size=5, use_gatv2=False, feat_gat_embed_dim=21, time_gat_embed_dim=9,
                          gru_hid_dim=33, forecast_n_layers=2, forecast_hid_dim=20, recon_hid_dim=40, dropout=0.3, alpha=0.1), 3),
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


def _grad_report(model, ref_grads, tol_abs=1e-5, tol_rel=1e-4):
    rows, bad = [], []
    for name, p in model.named_parameters():
        g, r = p.grad, ref_grads[name]
        if g is None:
            bad.append(f"{name}: no gradient")
            continue
        d = (g - r).abs().max().item()
        scale = r.abs().max().item()
        rows.append(f"{name:45s} |diff|={d:.3e} scale={scale:.3e}")
        if not (d <= tol_abs + tol_rel * scale) or not torch.isfinite(g).all():
            bad.append(rows[-1])
    return rows, bad


def _reference_grads(model, x, y, masks=None):
    """Autograd through the torch-op algebra on the same device / weights (and dropout masks)."""
    import _torchpath
    for p in model.parameters():
        p.grad = None
    with torch.backends.cudnn.flags(enabled=False):       # MIOpen's fused RNN refuses to back-propagate in eval mode
        pr, rc = _torchpath.forward(model, x, masks)
        _loss(pr, rc, x, y).backward()
    ref = {n: p.grad.clone() for n, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    return pr.detach(), rc.detach(), ref


@pytest.mark.parametrize("name", list(CONFIGS))
def test_gradients_match_autograd_eval_mode(name, gpu_device):
    """eval() + grad enabled: the deterministic function (dropout off) through the HIP forward_train / backward."""
    kw, b = CONFIGS[name]
    model = _model(kw, gpu_device).eval()
    g = torch.Generator().manual_seed(11)
    x = torch.rand(b, kw["window_size"], kw["n_features"], generator=g).to(gpu_device)
    y = torch.rand(b, kw["out_dim"], generator=g).to(gpu_device)
    pr_ref, rc_ref, ref = _reference_grads(model, x, y)
    pr, rc = model(x)
    assert model.grad_path == "hip", model.grad_path
    assert pr.requires_grad and rc.requires_grad
    assert (pr - pr_ref).abs().max().item() <= 1e-5 and (rc - rc_ref).abs().max().item() <= 1e-5
    with torch.no_grad():
        pe, re_ = model(x)                                  # the inference kernels agree with the training forward
    assert (pr - pe).abs().max().item() <= 1e-5 and (rc - re_).abs().max().item() <= 1e-5
    _loss(pr, rc, x, y).backward()
    rows, bad = _grad_report(model, ref)
    print("\n".join(rows))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["small_v2", "odd_shapes", "stacked"])
def test_gradients_match_autograd_above_the_small_batch_kernels(name, gpu_device):
    """Up to 4096 windows the fp32 recurrences run in 16-window groups (k_gru16 / k_gru16_bwd), above that on the
    hidden-tile-split kernels (k_gru_split / k_gru_bwd): the same check on a 4100-window batch, and the two kernel
    families against each other on the shared windows."""
    kw, _ = CONFIGS[name]
    b = 4100
    model = _model(kw, gpu_device).eval()
    g = torch.Generator().manual_seed(12)
    x = torch.rand(b, kw["window_size"], kw["n_features"], generator=g).to(gpu_device)
    y = torch.rand(b, kw["out_dim"], generator=g).to(gpu_device)
    pr_ref, rc_ref, ref = _reference_grads(model, x, y)
    pr, rc = model(x)
    assert model.grad_path == "hip", model.grad_path
    route = model._engine.train_route(b)                     # k_gru_split (on either operand build) + k_gru_bwd in every layer
    assert all(fwd in (3, 4) and bwd == 2 for fwd, bwd, _ in route["gru"] + route["rec"]), route
    assert (pr - pr_ref).abs().max().item() <= 1e-5 and (rc - rc_ref).abs().max().item() <= 1e-5
    with torch.no_grad():
        pe, re_ = model(x)
        ps, rs = model(x[:512])                              # small batch: the 16-window-group kernels
    assert (pr - pe).abs().max().item() <= 1e-5 and (rc - re_).abs().max().item() <= 1e-5
    assert (ps - pe[:512]).abs().max().item() <= 1e-5 and (rs - re_[:512]).abs().max().item() <= 1e-5
    _loss(pr, rc, x, y).backward()
    rows, bad = _grad_report(model, ref)
    assert not bad, "\n".join(bad)


_WINDOW_EDGE = {}


def _window_edge_step(n, device):
    """One eval-mode HIP step on the first n of 1793 fixed windows of `small_v2` and its autograd reference, computed once per n."""
    if n not in _WINDOW_EDGE:
        kw, _ = CONFIGS["small_v2"]
        model = _model(kw, device).eval()
        g = torch.Generator().manual_seed(16)
        x = torch.rand(1793, kw["window_size"], kw["n_features"], generator=g)[:n].to(device)
        y = torch.rand(1793, kw["out_dim"], generator=g)[:n].to(device)
        pr_ref, rc_ref, ref = _reference_grads(model, x, y)
        pr, rc = model(x)
        assert model.grad_path == "hip", model.grad_path
        _loss(pr, rc, x, y).backward()
        rows, bad = _grad_report(model, ref)
        route = model._engine.train_route(n)
        _WINDOW_EDGE[n] = (pr.detach(), rc.detach(), pr_ref, rc_ref, rows, bad, route)
    return _WINDOW_EDGE[n]


@pytest.mark.parametrize("n", [1792, 1793])
def test_gradients_match_autograd_on_both_sides_of_the_window_kernel_edge(n, gpu_device):
    """Up to 1792 windows the single-layer stacks run one window per workgroup at a time (k_gru1 / k_gru1_bwd), from 1793 on in
    16-window groups (k_gru16 / k_gru16_bwd): the file's gate against autograd on either side, on the smallest shape whose
    stacks take these kernels, and the two calls against each other on the windows they share."""
    pr, rc, pr_ref, rc_ref, rows, bad, route = _window_edge_step(n, gpu_device)
    kernels = (1, 0, 0) if n <= 1792 else (2, 1, 0)             # (forward, backward, x3): k_gru1 + k_gru1_bwd | k_gru16 + k_gru16_bwd
    assert route["gru"] == [kernels] and route["rec"] == [kernels], route
    dp, dr = (pr - pr_ref).abs().max().item(), (rc - rc_ref).abs().max().item()
    print(f"n={n}: |preds - ref| = {dp:.3e}, |recons - ref| = {dr:.3e}")
    print("\n".join(rows))
    assert dp <= 1e-5 and dr <= 1e-5
    assert not bad, "\n".join(bad)
    po, ro = _window_edge_step(1792 + 1793 - n, gpu_device)[:2]
    dp, dr = (pr[:1792] - po[:1792]).abs().max().item(), (rc[:1792] - ro[:1792]).abs().max().item()
    print(f"n={n}: the other call on the first 1792 windows: |preds| {dp:.3e}, |recons| {dr:.3e}")
    assert dp <= 1e-5 and dr <= 1e-5


def test_gradients_above_the_fp16_range_guard(gpu_device):
    """The training forward's recurrences run on split operands (k_gru_split on two fp16 pieces, with two fp16 pieces for the
    convolution's channels) from 2561 windows where the stack is not on the small-batch kernels -- a single-layer stack like this
    one leaves them above 4096 windows, hence 4100 -- unless the convolution recorded outputs of 2^15 and more: then the
    device-side guard hands the launch to the fp32 kernel (both are enqueued, one returns at once).  Un-normalised inputs must
    give the same gradients as autograd through the torch-op algebra, the route must be the guarded one and the guard must
    actually have tripped."""
    kw, _ = CONFIGS["odd_shapes"]
    b = 4100
    model = _model(kw, gpu_device).eval()
    g = torch.Generator().manual_seed(14)
    x = (torch.rand(b, kw["window_size"], kw["n_features"], generator=g) * 4e5).to(gpu_device)
    y = torch.rand(b, kw["out_dim"], generator=g).to(gpu_device)
    pr_ref, rc_ref, ref = _reference_grads(model, x, y)
    pr, rc = model(x)
    assert model.grad_path == "hip", model.grad_path
    route = model._engine.train_route(b)                     # k_gru_split on split operands + k_gru_bwd on three bf16 pieces ...
    assert route["gru"] == [(4, 2, 1)] and route["rec"] == [(4, 2, 1)], route
    first = model._engine.gru_route(0, 0, b, training=True, compute_units=torch.cuda.get_device_properties(gpu_device).multi_processor_count)
    assert (first["first"], first["fallback"]) == (4, 3), first      # ... with k_gru_split on fp32 operands behind the range guard
    # pre-activations of ~1e5: fp32 itself resolves ~1e-2 there, two summation orders differ by ~1e-4 in the outputs
    assert (pr - pr_ref).abs().max().item() <= 5e-4 and (rc - rc_ref).abs().max().item() <= 5e-4
    _loss(pr, rc, x, y).backward()
    rows, bad = _grad_report(model, ref, tol_abs=1e-5, tol_rel=5e-3)
    print("\n".join(rows))
    assert not bad, "\n".join(bad)
    with torch.no_grad():
        assert model.conv(x[:64]).max().item() >= 32768.0            # the inputs do exceed the fp16 pieces' range


@pytest.mark.parametrize("name", ["small_v2", "odd_shapes", "msl_shape", "v1_small", "v1_msl_shape", "stacked", "stacked3_v1", "wide_w130", "wide_w256", "wide_w300",
                                  "wide_f150", "v1_wide_w160", "v1_wide_f140"])
def test_gradients_match_autograd_with_dropout(name, gpu_device):
    """train(): dropout inside the kernels; the same keep-masks (exported by the library) injected into the
    torch-op algebra must give the same outputs and gradients."""
    kw, b = CONFIGS[name]
    model = _model(kw, gpu_device).train()
    g = torch.Generator().manual_seed(12)
    x = torch.rand(b, kw["window_size"], kw["n_features"], generator=g).to(gpu_device)
    y = torch.rand(b, kw["out_dim"], generator=g).to(gpu_device)
    torch.manual_seed(77)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())       # what _hipgrad.forward will draw
    torch.manual_seed(77)
    pr, rc = model(x)
    assert model.grad_path == "hip"
    masks = model._engine.dropout_masks(b, kw["dropout"], seed, gpu_device)
    keep = torch.cat([m.reshape(-1) for m in [masks["feat"], masks["temp"]] + masks["fc"]]).mean().item()
    assert abs(keep - (1.0 - kw["dropout"])) < 0.02, keep
    _loss(pr, rc, x, y).backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters()}
    pr_ref, rc_ref, ref = _reference_grads(model, x, y, masks)
    assert (pr - pr_ref).abs().max().item() <= 1e-5 and (rc - rc_ref).abs().max().item() <= 1e-5
    for n, p in model.named_parameters():
        p.grad = got[n]
    rows, bad = _grad_report(model, ref)
    print("\n".join(rows))
    assert not bad, "\n".join(bad)
    # another call draws another seed -> other masks
    pr2, _ = model(x)
    assert not torch.equal(pr2, pr)


def test_chunked_training_step_equals_single_chunk(gpu_device, monkeypatch):
    """Batches above the chunk size are processed chunk by chunk with the chunk's forward recomputed in
    backward; the counter-based dropout makes that the same function as the one-chunk step."""
    import _hipgrad
    kw, b = CONFIGS["odd_shapes"]
    model = _model(kw, gpu_device).train()
    g = torch.Generator().manual_seed(13)
    x = torch.rand(b, kw["window_size"], kw["n_features"], generator=g).to(gpu_device)
    y = torch.rand(b, kw["out_dim"], generator=g).to(gpu_device)

    def step():
        for p in model.parameters():
            p.grad = None
        torch.manual_seed(5)
        pr, rc = model(x)
        _loss(pr, rc, x, y).backward()
        return pr.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}

    p1, g1 = step()
    monkeypatch.setattr(_hipgrad, "TRAIN_CHUNK", 32)         # 70 windows -> 32 + 32 + 6
    p2, g2 = step()
    assert torch.equal(p1, p2)
    for n in g1:
        d = (g1[n] - g2[n]).abs().max().item()
        assert d <= 1e-6 + 1e-5 * g1[n].abs().max().item(), (n, d)


def test_backward_stage_diagnostics(gpu_device):
    """Not a gate by itself: prints where the HIP training step and autograd part ways, stage by stage
    (tape contents after the forward, workspace contents after the backward), for a linear loss whose
    upstream gradients do not couple the windows."""
    import _torchpath as tp
    kw, b = CONFIGS["odd_shapes"]
    b = 5
    model = _model(kw, gpu_device).eval()
    eng = model._sync_engine(gpu_device)
    W, Fn, H = kw["window_size"], kw["n_features"], kw["gru_hid_dim"]
    g = torch.Generator().manual_seed(21)
    x = torch.rand(b, W, Fn, generator=g).to(gpu_device)
    cp = torch.randn(b, kw["out_dim"], generator=g).to(gpu_device)
    cr = torch.randn(b, W, kw["out_dim"], generator=g).to(gpu_device)
    # torch side with retained intermediates
    with torch.backends.cudnn.flags(enabled=False):
        xc = tp.conv_stage(model, x); xc.retain_grad()
        hf = tp.feature_gat_stage(model, xc); hf.retain_grad()
        ht = tp.temporal_gat_stage(model, xc); ht.retain_grad()
        hcat = torch.cat([xc, hf, ht], dim=2); hcat.retain_grad()
        hend = tp.gru_stage(model, hcat); hend.retain_grad()
        pr = tp.forecast_stage(model, hend)
        rc = tp.recon_stage(model, hend)
        ((pr * cp).sum() + (rc * cr).sum()).backward()
    ref = {n: p.grad.clone() for n, p in model.named_parameters()}
    # HIP side
    prh, rch, tape = eng.forward_train(x, 0.0, 0)
    offs, total = eng.grad_layout()
    grads = torch.zeros(total, device=gpu_device)
    eng.backward(x, 0.0, 0, cp.contiguous(), cr.contiguous(), tape, grads)
    torch.cuda.synchronize()
    to, wo = eng.train_layout(b)
    ws = eng._bws
    c = eng.cfg
    Dp = (3 * Fn + 7) // 8 * 8
    Hp = (H + 31) // 32 * 32
    Fp = (Fn + 7) // 8 * 8
    Wp = (W + 7) // 8 * 8
    rep = []

    def cmp(label, ours, theirs):
        rep.append(f"{label:34s} |diff|={(ours - theirs).abs().max().item():.3e} scale={theirs.abs().max().item():.3e}")

    cmp("fwd preds", prh, pr.detach())
    cmp("fwd recons", rch, rc.detach())
    hc = tape[to["hcat"]: to["hcat"] + b * W * Dp].view(b, W, Dp)
    cmp("tape h_cat", hc[:, :, :3 * Fn], hcat.detach())
    cmp("tape h_end", tape[to["hend"]: to["hend"] + b * Hp].view(b, Hp)[:, :H], hend.detach())
    cmp("tape xcT", tape[to["xct"]: to["xct"] + b * Fn * Wp].view(b, Fn, Wp)[:, :, :W], xc.detach().permute(0, 2, 1))
    cmp("ws d h_end", ws[wo["dhend"]: wo["dhend"] + b * Hp].view(b, Hp)[:, :H], hend.grad)
    dhc = ws[wo["dhcat"]: wo["dhcat"] + b * W * Dp].view(b, W, Dp)
    # d h_cat as the GRU backward leaves it = gradient through the GRU only (the attention layers' share is added later)
    cmp("ws d h_cat[:, 2F:3F] (temporal out)", dhc[:, :, 2 * Fn:3 * Fn], ht.grad)
    cmp("ws d h_cat[:, F:2F] (feature out)", dhc[:, :, Fn:2 * Fn], hf.grad)
    dpre = ws[wo["dpre"]: wo["dpre"] + b * W * Fp].view(b, W, Fp)[:, :, :Fn]
    cmp("ws d conv pre-activation", dpre, xc.grad * (xc.detach() > 0))
    names = [n for n, _ in model.named_parameters()]
    import _hipgrad
    for p_, o in zip(_hipgrad.param_order(model), offs):
        nm = [n for n, q in model.named_parameters() if q is p_][0]
        cmp("grad " + nm, grads[o:o + p_.numel()].view(p_.shape), ref[nm])
    print("\n".join(rep))
    assert len(names) == len(offs)


@pytest.mark.parametrize("name", ["odd_shapes", "smd_shape"])
def test_bf16_request_trains_on_the_fp32_step(name, gpu_device):
    """BASELINE config 3 names a "bf16 train loop": precision = "bf16" (or bf16 tensors) in train() is served by the fp32 HIP
    training step -- the bf16-operand recurrence kernels of rounds 2-5 were slower and less accurate than it at every batch size
    and were removed in round 6.  Same outputs bit for bit, same gradients up to the backward's summation order; bf16 tensors are
    answered in bf16; a few Adam steps learn; the C ABI refuses a bf16-mode training call."""
    import _native
    kw, b = CONFIGS[name]
    model = _model(kw, gpu_device).train()
    g = torch.Generator().manual_seed(14)
    x = torch.rand(b, kw["window_size"], kw["n_features"], generator=g).to(gpu_device)
    y = torch.rand(b, kw["out_dim"], generator=g).to(gpu_device)

    def step(precision):
        model.precision = precision
        for p in model.parameters():
            p.grad = None
        torch.manual_seed(9)                                  # same dropout seed -> same masks
        pr, rc = model(x)
        assert model.grad_path == "hip"
        _loss(pr, rc, x, y).backward()
        return pr.detach(), rc.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}

    p32, r32, g32 = step("fp32")
    pd, rd, gd = step("bf16")
    assert torch.equal(pd, p32) and torch.equal(rd, r32)      # (the backward sums through float atomics: not bit-reproducible)
    assert all((gd[n] - g32[n]).abs().max().item() <= 1e-6 + 1e-5 * g32[n].abs().max().item() for n in g32)
    model.precision = "auto"
    torch.manual_seed(9)
    pb, rb = model(x.to(torch.bfloat16))
    assert pb.dtype == torch.bfloat16 and rb.dtype == torch.bfloat16
    eng = model._engine
    eng.set_precision(1)
    with pytest.raises(RuntimeError, match="computes in fp32"):
        eng.forward_train(x, 0.0, 0, 0)
    eng.set_precision(2)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    model.precision = "bf16"
    for _ in range(6):
        opt.zero_grad()
        pr, rc = model(x)
        loss = _loss(pr, rc, x, y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0]


def test_sharded_dropout_stream_equals_the_single_process_step(gpu_device):
    """`model.dropout_stream = (seed, first_global_window)` (what sharding.dp_training_step sets per rank): two
    shards of a batch draw exactly the masks of the one-process step over the whole batch -- outputs bit-equal,
    gradients of a shard-additive loss equal up to the summation order."""
    kw, b = CONFIGS["odd_shapes"]
    model = _model(kw, gpu_device).train()
    g = torch.Generator().manual_seed(15)
    x = torch.rand(b, kw["window_size"], kw["n_features"], generator=g).to(gpu_device)
    cp = torch.randn(b, kw["out_dim"], generator=g).to(gpu_device)
    cr = torch.randn(b, kw["window_size"], kw["out_dim"], generator=g).to(gpu_device)

    def run(lo, hi):
        object.__setattr__(model, "dropout_stream", (4242, lo))
        pr, rc = model(x[lo:hi].contiguous())
        ((pr * cp[lo:hi]).sum() + (rc * cr[lo:hi]).sum()).backward()
        object.__setattr__(model, "dropout_stream", None)
        return pr.detach(), rc.detach()

    for p in model.parameters():
        p.grad = None
    p_all, r_all = run(0, b)
    g_all = {n: p.grad.clone() for n, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    pa, ra = run(0, 41)
    pb, rb = run(41, b)                                   # gradients accumulate in .grad across the two shards
    assert torch.equal(torch.cat([pa, pb]), p_all) and torch.equal(torch.cat([ra, rb]), r_all)
    for n, p in model.named_parameters():
        d = (p.grad - g_all[n]).abs().max().item()
        assert d <= 1e-6 + 1e-5 * g_all[n].abs().max().item(), (n, d)


def test_gradients_are_views_of_one_flat_buffer(gpu_device):
    """The HIP backward fills one flat buffer in the field order of mtadgat_params; autograd adopts its per-parameter views as
    `.grad` without copying, so sharding.dp_training_step exchanges the whole gradient with one in-place all-reduce (no
    torch.cat, no per-parameter copies)."""
    import sharding
    kw, b = CONFIGS["odd_shapes"]
    model = _model(kw, gpu_device).train()
    g = torch.Generator().manual_seed(21)
    x = torch.rand(b, kw["window_size"], kw["n_features"], generator=g).to(gpu_device)
    y = torch.rand(b, kw["out_dim"], generator=g).to(gpu_device)
    for p in model.parameters():
        p.grad = None
    pr, rc = model(x)
    assert model.grad_path == "hip"
    _loss(pr, rc, x, y).backward()
    flat = sharding._flat_gradient_buffer(model)
    assert flat is not None and flat.numel() == sum(p.numel() for p in model.parameters())
    total = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    assert total.abs().sum().item() > 0 and abs(flat.sum().item() - total.sum().item()) <= 1e-3 * total.abs().sum().item()
    flat.mul_(2.0)                                              # the bucket IS the gradients
    assert torch.allclose(torch.cat([p.grad.reshape(-1) for p in model.parameters()]).abs().sum(), 2.0 * total.abs().sum(), rtol=1e-5)
    # a second backward into existing gradients accumulates into autograd's own tensors: then the views no longer alias
    pr, rc = model(x)
    _loss(pr, rc, x, y).backward()
    assert sharding._flat_gradient_buffer(model) is None


@pytest.mark.parametrize("name", ["small_v2", "odd_shapes", "msl_shape", "v1_small", "stacked"])
def test_input_gradient_matches_autograd(name, gpu_device, monkeypatch):
    """x.requires_grad: the HIP step also returns d loss / d x (mtadgat_backward_input: the convolution's data gradient of the
    pre-activation gradients the backward leaves in its workspace) -- against autograd through the torch-op algebra, same
    weights; also when the batch is walked in several chunks."""
    import _hipgrad
    kw, b = CONFIGS[name]
    model = _model(kw, gpu_device).eval()
    g = torch.Generator().manual_seed(13)
    x0 = torch.rand(b, kw["window_size"], kw["n_features"], generator=g).to(gpu_device)
    y = torch.rand(b, kw["out_dim"], generator=g).to(gpu_device)
    import _torchpath
    xr = x0.clone().requires_grad_(True)
    with torch.backends.cudnn.flags(enabled=False):
        pr, rc = _torchpath.forward(model, xr)
        _loss(pr, rc, xr, y).backward()
    dx_ref = xr.grad.clone()
    ref = {n: p.grad.clone() for n, p in model.named_parameters()}
    for chunk in (None, 16):
        if chunk:
            monkeypatch.setattr(_hipgrad, "TRAIN_CHUNK", chunk)
        for p in model.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        pr, rc = model(x)
        assert model.grad_path == "hip", model.grad_path
        _loss(pr, rc, x, y).backward()
        assert x.grad is not None and x.grad.shape == x.shape and torch.isfinite(x.grad).all()
        d, scale = (x.grad - dx_ref).abs().max().item(), dx_ref.abs().max().item()
        print(f"{name} chunk={chunk}: |dx - ref| = {d:.3e}, scale {scale:.3e}")
        assert d <= 1e-6 + 1e-4 * scale
        rows, bad = _grad_report(model, ref)
        assert not bad, "\n".join(bad)
