"""Parity of the HIP path (through the C ABI, via the drop-in module) with the reference:
golden vectors generated from the reference itself (tests/golden/make_golden.py)."""
import pytest
import torch

from helpers import ALL_CASES, SHIPPED_CASES, Case, call_routes, device_compute_units, gate
from oracle import mtad_gat_oracle as oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=ALL_CASES)
def case_model(request, gpu_device):
    case = Case(request.param)
    model = case.build_model().to(gpu_device)
    return case, model


def test_forward_matches_reference(case_model, gpu_device):
    case, model = case_model
    with torch.no_grad():
        preds, recons = model(case.x.to(gpu_device))
    assert preds.shape == case.preds.shape and recons.shape == case.recons.shape
    assert preds.dtype == torch.float32 and preds.device.type == "cuda"
    dp = gate(preds, case.preds, case.preds64, what=f"{case.name} predictions")
    dr = gate(recons, case.recons, case.recons64, what=f"{case.name} recons")
    print(f"{case.name}: |preds-ref|={dp:.2e} |recons-ref|={dr:.2e}")


def test_stages_match_reference(case_model, gpu_device):
    case, model = case_model
    x = case.x.to(gpu_device)
    with torch.no_grad():
        xc = model.conv(x)
        gate(xc, case.stages["xc"], what=f"{case.name} conv")
        xc_ref = case.stages["xc"].to(gpu_device)
        hf = model.feature_gat(xc_ref)
        gate(hf, case.stages["h_feat"], what=f"{case.name} feature_gat")
        ht = model.temporal_gat(xc_ref)
        gate(ht, case.stages["h_temp"], what=f"{case.name} temporal_gat")
        hcat = torch.cat([case.stages["xc"], case.stages["h_feat"], case.stages["h_temp"]], dim=2).to(gpu_device)
        _, h_end = model.gru(hcat)
        gate(h_end, case.stages["h_end"], case.h_end64, what=f"{case.name} gru h_end")
        h_ref = case.stages["h_end"].to(gpu_device)
        p = model.forecasting_model(h_ref)
        gate(p, case.preds, case.preds64, what=f"{case.name} forecasting head")
        r = model.recon_model(h_ref)
        gate(r, case.recons, case.recons64, what=f"{case.name} reconstruction head")


@pytest.mark.parametrize("name", ["msl_wide", "smap_wide", "smd_1_1_wide", "msl_c1"])
def test_wide_fixtures_match_reference(name, gpu_device):
    """300 / 320 windows of each shipped checkpoint (a full 256-window Predictor batch + a ragged tail),
    every window compared with the reference's output; `msl_c1` has the C1 input statistics (sine +
    Bernoulli(0.05) columns, values outside [0,1]) and is also fed through the GPU-side window gather."""
    from helpers import WideCase
    case = WideCase(name)
    model = case.build_model().to(gpu_device)
    x = case.x.to(gpu_device)
    with torch.no_grad():
        outs = []
        for lo in range(0, x.shape[0], 256):                      # the reference Predictor's batching
            outs.append(model(x[lo:lo + 256].contiguous()))
        preds = torch.cat([o[0] for o in outs])
        recons = torch.cat([o[1] for o in outs])
        p1, r1 = model(x)
    assert torch.equal(p1, preds) and torch.equal(r1, recons)
    dp = gate(preds, case.preds, case.preds64, what=f"{name} predictions")
    dr = gate(recons, case.recons, case.recons64, what=f"{name} recons")
    print(f"{name}: |preds-ref|={dp:.2e} |recons-ref|={dr:.2e}")
    if case.series is not None:
        with torch.no_grad():
            ps, rs = model.forward_series(case.series.to(gpu_device), count=x.shape[0])
        assert torch.equal(ps, preds) and torch.equal(rs, recons)


def test_input_not_modified(case_model, gpu_device):
    case, model = case_model
    x = case.x.to(gpu_device)
    x0 = x.clone()
    with torch.no_grad():
        model(x)
    assert torch.equal(x, x0)


@pytest.mark.parametrize("name", SHIPPED_CASES)
def test_ragged_batches_and_chunking(name, gpu_device):
    """Batch-split invariance (what data-parallel sharding relies on), batches that do not fill
    a 32-window tile, and the internal chunk loop."""
    case = Case(name)
    model = case.build_model().to(gpu_device)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(77, case.kwargs["window_size"], case.kwargs["n_features"], generator=g).to(gpu_device)
    with torch.no_grad():
        p_all, r_all = model(x)
        # windows are independent: any split gives bit-identical rows
        for lo, hi in [(0, 1), (1, 34), (34, 77)]:
            p, r = model(x[lo:hi].contiguous())
            assert torch.equal(p, p_all[lo:hi]) and torch.equal(r, r_all[lo:hi]), (lo, hi)
        perm = torch.randperm(77, generator=g).to(gpu_device)
        p, r = model(x[perm].contiguous())
        assert torch.equal(p, p_all[perm]) and torch.equal(r, r_all[perm])
        model._engine.set_chunk_windows(20)   # 77 = 20+20+20+17
        p, r = model(x)
        assert torch.equal(p, p_all) and torch.equal(r, r_all)
        # the first 6 windows of the fixture still match the reference when embedded in a batch
        xx = torch.cat([case.x.to(gpu_device), x], dim=0)
        p, r = model(xx)
        gate(p[:6], case.preds, case.preds64, what="embedded preds")
        gate(r[:6], case.recons, case.recons64, what="embedded recons")
    assert model(x[:0])[0].shape == (0, case.kwargs["out_dim"])


@pytest.mark.parametrize("precision", ["fp32", "fp32_strict"])
@pytest.mark.parametrize("name", ["msl", "syn_v2_embed", "syn_v1_small"])
def test_large_batch_kernels_match_small_batch_kernels(name, precision, gpu_device):
    """Batches above 16 k windows run the register-resident GRU (k_gru: by default its split-bf16 build -- three bf16
    pieces per operand on the bf16 matrix pipe --, with precision "fp32_strict" the fp32-MFMA build), smaller ones the
    small-batch kernels; the fixture windows embedded in a 20 000-window batch must still match the reference, and
    the large batch must agree with the same windows run as a small batch."""
    case = Case(name)
    model = case.build_model().to(gpu_device)
    model.precision = precision
    g = torch.Generator().manual_seed(11)
    W, F = case.kwargs["window_size"], case.kwargs["n_features"]
    x = torch.rand(20000, W, F, generator=g)
    x[:case.x.shape[0]] = case.x
    x = x.to(gpu_device)
    with torch.no_grad():
        p_big, r_big = model(x)
        p_small, r_small = model(x[19000:19300].contiguous())
    n = case.x.shape[0]
    gate(p_big[:n], case.preds, case.preds64, what="preds in a 20000-window batch")
    gate(r_big[:n], case.recons, case.recons64, what="recons in a 20000-window batch")
    assert (p_big[19000:19300] - p_small).abs().max().item() <= 2e-6
    assert (r_big[19000:19300] - r_small).abs().max().item() <= 2e-6


@pytest.mark.parametrize("scale", [1e-4, 1.0, 3e4])
def test_split_operand_kernels_track_the_fp32_mfma_kernels_at_any_input_scale(scale, gpu_device):
    """The default arithmetic of large batches splits operands into 16-bit pieces: three bf16 pieces (fp32's exponent range)
    where magnitudes are unbounded -- the window values and the convolution's outputs --, two fp16 pieces only where the
    range is bounded by construction (recurrent state, attention outputs; weights scaled per layer).  Inputs far outside
    [0, 1] (un-normalised series) must therefore still reproduce the fp32-MFMA kernels, and weights of unusual magnitude
    too."""
    case = Case("msl")
    model = case.build_model().to(gpu_device)
    g = torch.Generator().manual_seed(17)
    W, F = case.kwargs["window_size"], case.kwargs["n_features"]
    x = (torch.rand(20000, W, F, generator=g) * scale).to(gpu_device)
    with torch.no_grad():
        outs = {}
        for wmul in (1.0, 0.23):                       # also: smaller recurrent weights (another power-of-two weight scale)
            for p in (model.gru.gru.weight_hh_l0, model.recon_model.decoder.rnn.weight_hh_l0):
                p.mul_(wmul)
            for precision in ("fp32", "fp32_strict"):
                model.precision = precision
                outs[(wmul, precision)] = model(x)
            pa, ra = outs[(wmul, "fp32")]
            pb, rb = outs[(wmul, "fp32_strict")]
            assert torch.isfinite(pa).all() and torch.isfinite(ra).all()
            # un-normalised inputs drive the pre-activations to ~1e4, where fp32 itself resolves 1e-3: any two summation
            # orders differ by ~1e-3 in the few units whose large terms cancel
            tol = (2e-6 if scale <= 1.0 else 5e-3) * max(1.0, rb.abs().max().item())
            assert (pa - pb).abs().max().item() <= tol and (ra - rb).abs().max().item() <= tol, (scale, wmul)


# What test_full_machine_batch_matches runs, hand-written (256 compute units): the 65 573 windows go as a piece of 65 536 and one of 37.
FULL_MACHINE_ROUTES = {
    ("msl", "fp32"): "cm+tile:x3_hi:2 | cm:fc",
    ("msl", "fp32_strict"): "tile:fp32:2 | tile:fp32:2:fc",
    ("syn_v2_embed", "fp32"): "cm+tile:x3_lo:2 | cm:fc",
    ("syn_v2_embed", "fp32_strict"): "tile:fp32:2 | tile:fp32:2:fc",
}


@pytest.mark.parametrize("precision", ["fp32", "fp32_strict"])
@pytest.mark.parametrize("name", ["msl", "syn_v2_embed"])
def test_full_machine_batch_matches(name, precision, gpu_device):
    """A ragged batch of 65 536 + 37 windows runs as two pieces: 65 536 windows on the large-batch kernels -- "fp32_strict": the
    tile-major kernel with two 32-window groups per wave (one wave per SIMD); the default arithmetic: the chunk-major kernel, the
    two-group tile-major kernel on split operands behind its range guard -- and the last 37 on the window-per-workgroup kernel.  The
    fixture windows are embedded twice, at the end of the call (the 37-window piece) and at the end of the 65 536-window piece (its
    last wave); both copies must match the reference, and the large piece must agree with a small-batch run.  (A ragged last wave
    under two groups per wave: tests/test_gpu_gru_routes.py.)"""
    case = Case(name)
    model = case.build_model().to(gpu_device)
    model.precision = precision
    g = torch.Generator().manual_seed(13)
    W, F = case.kwargs["window_size"], case.kwargs["n_features"]
    n_big = 65536 + 37
    x = torch.rand(n_big, W, F, generator=g)
    n = case.x.shape[0]
    assert n <= 37
    x[-n:] = case.x                                   # the last piece
    x[65536 - n:65536] = case.x                       # the last windows of the 65 536-window piece
    x = x.to(gpu_device)
    with torch.no_grad():
        p_big, r_big = model(x)
        pieces, routes = call_routes(model._sync_engine(gpu_device), n_big, device_compute_units(gpu_device))
        p_small, r_small = model(x[40000:40100].contiguous())
    assert pieces == [65536, 37] and routes == [FULL_MACHINE_ROUTES[name, precision], "gru1 | gru1"], (pieces, routes)
    gate(p_big[-n:], case.preds, case.preds64, what="preds at the end of a 65573-window batch")
    gate(r_big[-n:], case.recons, case.recons64, what="recons at the end of a 65573-window batch")
    gate(p_big[65536 - n:65536], case.preds, case.preds64, what="preds at the end of the 65536-window piece")
    gate(r_big[65536 - n:65536], case.recons, case.recons64, what="recons at the end of the 65536-window piece")
    assert (p_big[40000:40100] - p_small).abs().max().item() <= 2e-6
    assert (r_big[40000:40100] - r_small).abs().max().item() <= 2e-6


@pytest.mark.parametrize("precision", ["fp32", "fp32_strict"])
def test_headline_batch_random_windows_against_the_oracle(precision, gpu_device):
    """The headline workload itself (bench.py: 65 536 MSL windows, x ~ U[0,1) seed 1234, the shipped MSL checkpoint, eval): 64
    windows drawn at random from the whole batch -- both rounds of the large-batch recurrence, every chunk -- against the oracle
    (the reference's algorithm on the CPU, mtad_gat.py:64-79), not only the fixture windows at the tail."""
    from bench import load_msl_state_dict
    from mtad_gat import MTAD_GAT
    sd, kw = load_msl_state_dict()
    model = MTAD_GAT(**kw)
    model.load_state_dict(sd)
    model = model.eval()
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(65536, kw["window_size"], kw["n_features"], generator=g)
    pick = torch.randperm(65536, generator=torch.Generator().manual_seed(7))[:64].sort().values
    with torch.no_grad():
        p_ref, r_ref = oracle.forward_chunked(x[pick], sd, alpha=kw.get("alpha", 0.2), chunk=16)
        m = model.to(gpu_device)
        m.precision = precision
        p, r = m(x.to(gpu_device))
    pk = pick.to(gpu_device)
    gate(p[pk], p_ref, what=f"preds, 64 random windows of the 65 536-window bench batch, {precision}")
    gate(r[pk], r_ref, what=f"recons, 64 random windows of the 65 536-window bench batch, {precision}")


def test_bf16_io_smap_batch_4096(gpu_device):
    """BASELINE config 2 (SMAP, F=25, W=100, bf16 inference, batch 4096): bf16 tensors in and out.
    precision "auto" (default) answers bf16 tensors with the bf16-operand kernels; precision "fp32" keeps fp32
    arithmetic and only rounds the I/O: then the result is exactly the fp32 path applied to the bf16-rounded input,
    rounded once on the way out.  Against the un-rounded fp32 input the input rounding alone moves the outputs by up
    to 2.1e-2 over these 4096 windows (SURVEY section 8d measured 5e-3 on 16 windows and set the bf16 gate at 2e-2)."""
    case = Case("smap")
    model = case.build_model().to(gpu_device)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4096, case.kwargs["window_size"], case.kwargs["n_features"], generator=g)
    n = case.x.shape[0]
    x[:n] = case.x
    x = x.to(gpu_device)
    xb = x.to(torch.bfloat16)
    with torch.no_grad():
        p32, r32 = model(x)
        p16, r16 = model(xb)                      # bf16 operands
        model.precision = "fp32"
        pf, rf = model(xb)                        # bf16 I/O, fp32 arithmetic
        pr, rr = model(xb.float())
    assert p16.dtype == torch.bfloat16 and r16.dtype == torch.bfloat16 and pf.dtype == torch.bfloat16
    assert torch.equal(pf, pr.to(torch.bfloat16)) and torch.equal(rf, rr.to(torch.bfloat16))
    for p_, r_ in ((p16, r16), (pf, rf)):
        assert (p_.float() - p32).abs().max().item() <= 5e-2 and (r_.float() - r32).abs().max().item() <= 5e-2
        assert (p_[:n].float().cpu() - case.preds).abs().max().item() <= 2e-2
        assert (r_[:n].float().cpu() - case.recons).abs().max().item() <= 2e-2


def test_weight_update_is_seen(gpu_device):
    """Parameters changed in place (optimizer.step, load_state_dict) must reach the kernels."""
    a = Case("smap")
    model = a.build_model().to(gpu_device)
    x = a.x.to(gpu_device)
    with torch.no_grad():
        p0, _ = model(x)
        model.forecasting_model.layers[3].bias.add_(1.0)
        p1, _ = model(x)
        assert torch.allclose(p1, p0 + 1.0, atol=1e-6)
        model.load_state_dict(a.state_dict())
        p2, _ = model(x)
        assert torch.equal(p2, p0)
        # edits through .data do not bump autograd's version counter: the content fingerprint sees them
        bias = model.forecasting_model.layers[3].bias
        orig = bias.detach().clone()
        v = bias._version
        bias.data.add_(2.0)
        assert bias._version == v
        p3, _ = model(x)
        assert torch.allclose(p3, p0 + 2.0, atol=1e-6)
        # ... unless the caller opts out of the per-call check; then refresh_weights() is the contract
        model.check_weight_contents = False
        model(x)
        bias.data.copy_(orig)
        assert torch.equal(model(x)[0], p3)
        model.refresh_weights()
        assert torch.equal(model(x)[0], p0)


def test_data_edit_behind_an_unchecked_call_is_seen(gpu_device):
    """check_weight_contents = "eval_only": a train-mode call runs unchecked (the contents on record are dropped), a `p.data`
    edit follows (no version counter moves, the packed-weight key is unchanged), then the first checked call has nothing to
    compare with -- it must re-pack instead of serving the old weights.  Same when the flag is toggled off and on."""
    a = Case("smap")
    model = a.build_model().to(gpu_device)
    model.check_weight_contents = "eval_only"
    x = a.x.to(gpu_device)
    bias = model.forecasting_model.layers[3].bias
    orig = bias.detach().clone()
    with torch.no_grad():
        p0, _ = model(x)
    model.train()
    model(x)                                           # unchecked (training): hip training forward, weights as packed
    model.eval()
    v = bias._version
    bias.data.add_(0.75)
    assert bias._version == v
    with torch.no_grad():
        p1, _ = model(x)
        assert torch.allclose(p1, p0 + 0.75, atol=1e-6)
        model.check_weight_contents = False
        model(x)
        bias.data.copy_(orig)
        model.check_weight_contents = True
        assert torch.equal(model(x)[0], p0)


def test_errors_are_loud(gpu_device):
    case = Case("syn_v2_embed")
    model = case.build_model()
    with pytest.raises(RuntimeError, match="parameters are on"):
        model(case.x.to(gpu_device))         # model left on the CPU, input on the GPU: no silent host round trip
    model = model.to(gpu_device)
    with pytest.raises(RuntimeError, match="expected input of shape"):
        model(case.x[:, :-1].to(gpu_device))
    with pytest.raises(RuntimeError, match="GPU-side data path"):
        model.forward_series(torch.rand(300, case.kwargs["n_features"]))


@pytest.mark.parametrize("name", ["msl_wide", "smap_wide", "smd_1_1_wide", "msl_c1"])
def test_bf16_operand_mode_within_2e_2(name, gpu_device):
    """precision = "bf16": bf16 MFMA operands with fp32 accumulation, fp32 recurrent state, gates and softmax.
    Gate: abs err <= 2e-2 against the fp32 reference on the shipped checkpoints -- the
    all-bf16 reference model itself is off by 3e-2 .. 1.1e-1 -- while the default fp32 build stays <= 1e-5."""
    from helpers import WideCase
    case = WideCase(name)
    model = case.build_model().to(gpu_device)
    x = case.x.to(gpu_device)
    with torch.no_grad():
        p32, r32 = model(x)
        model.precision = "bf16"
        pb, rb = model(x)
        pa, ra = model(x.to(torch.bfloat16))              # "auto" semantics: bf16 tensors in -> bf16 operands, bf16 out
        model.precision = "auto"
        pa2, ra2 = model(x.to(torch.bfloat16))
        big = torch.cat([x] * 60)[:17000].contiguous()    # > 16 k windows: the register-resident GRU kernels
        model.precision = "bf16"
        pbig, rbig = model(big)
        model.precision = "fp32"
        p32b, _ = model(x)
    assert torch.equal(p32b, p32)
    dp = (pb.cpu() - case.preds).abs().max().item()
    dr = (rb.cpu() - case.recons).abs().max().item()
    print(f"{name}: bf16 operands |preds-ref|={dp:.2e} |recons-ref|={dr:.2e}")
    assert dp <= 2e-2 and dr <= 2e-2
    assert not torch.equal(pb, p32)                                     # it really is a different arithmetic
    assert pa.dtype == torch.bfloat16 and torch.equal(pa, pa2)
    n = x.shape[0]
    assert (pbig[:n].cpu() - case.preds).abs().max().item() <= 2e-2 and (rbig[:n].cpu() - case.recons).abs().max().item() <= 2e-2
    assert (pa.float().cpu() - case.preds).abs().max().item() <= 3e-2 and (ra.float().cpu() - case.recons).abs().max().item() <= 3e-2


def test_short_last_chunk_is_planned_for_its_own_size(gpu_device):
    """A batch of one chunk + a few windows: the short last chunk runs exactly what a call with only those windows runs
    (small-batch recurrence kernels and their buffers), not the full chunk's layout -- a 65 537-window call used to spend
    6 ms on its 1-window tail."""
    a = Case("smap")
    model = a.build_model().to(gpu_device)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2000 + 5, a.kwargs["window_size"], a.kwargs["n_features"], generator=g).to(gpu_device)
    with torch.no_grad():
        eng = model._sync_engine(gpu_device)
        keep = eng.chunk_windows()
        try:
            p1, r1 = model(x[:2000])
            p2, r2 = model(x[2000:])
            eng.set_chunk_windows(2000)
            p, r = model(x)
        finally:
            eng.set_chunk_windows(keep)
    assert torch.equal(p, torch.cat([p1, p2])) and torch.equal(r, torch.cat([r1, r2]))


# What test_mid_size_batches_match runs, hand-written (256 compute units, one piece each): the automatic choice, the calls forced with
# "gru_kernel" = 1 / 2 at n_mid windows (3000 / 8192), and the 10 273-window call forced with "gru_kernel" = 1 on one lane.  Up to 8192
# windows nothing forces the tile-major kernel onto a layer of two or more hidden tiles: "gru_kernel" = 1 only refuses the split-operand
# kernels there, and at 3000 windows values 1 and 2 leave the 16-window-group kernel in place.  (syn_v1_small: v1 attention records no
# convolution range and its decoder has one hidden tile: no split-operand kernel applies, the option changes nothing.)
MID_ROUTES = {
    "msl": dict(auto="splitx3+tile:x3_hi | splitx3:fc", k1=("gru16 | gru16", "split:fp32:xp | split:fp32:fc"),
                k2=("gru16 | gru16", "cm+tile:x3_hi | cm:fc"), tile="tile:x3_hi | tile:x3_hi:fc"),
    "smd_1_1": dict(auto="splitx3+tile:x3_hi | splitx3", k1=("gru16 | gru16", "split:fp32:xp | split:fp32"),
                    k2=("gru16 | gru16", "cm+tile:x3_hi | cm"), tile="tile:x3_hi | tile:x3_hi"),
    "syn_v2_embed": dict(auto="splitx3+tile:x3_lo | splitx3:fc", k1=("gru16 | gru16", "split:fp32:xp | split:fp32:fc"),
                         k2=("gru16 | gru16", "cm+tile:x3_lo | cm:fc"), tile="tile:x3_lo | tile:x3_lo:fc"),
    "syn_v1_small": dict(auto="split:fp32:xp | tile:fp32 | tile:fp32 | tile:fp32", k1=("split:fp32:xp | tile:fp32 | tile:fp32 | tile:fp32",) * 2,
                         k2=("split:fp32:xp | tile:fp32 | tile:fp32 | tile:fp32",) * 2, tile="tile:x3_lo | tile:x3_lo | tile:x3_lo | tile:x3_lo"),
}
N_TILE = 10273                                        # more than 1.25 32-window groups per compute unit, the last group of one window


@pytest.mark.parametrize("n_mid", [3000, 8192])
@pytest.mark.parametrize("name", ["msl", "smd_1_1", "syn_v2_embed", "syn_v1_small"])
def test_mid_size_batches_match(name, n_mid, gpu_device):
    """2 561 - 8 192 windows: the hidden-tile-split recurrence on split operands (two fp16 pieces per value, one workgroup
    of NCG waves per 32 windows) -- fixture windows embedded in such a batch match the reference, the batch agrees with the
    same windows run as a small batch (16-window-group / window-per-workgroup kernels) and, forced through the engine's
    measurement hook, with the kernels MID_ROUTES names: "gru_kernel" = 1 (3000 windows: the 16-window-group kernel, 8192: the
    hidden-tile split on fp32 operands), 2 (3000: the same, 8192: the chunk-major kernel) and 3 (the automatic choice); and with the
    tile-major kernel on split operands, which takes these windows as the head of a 10 273-window call on one lane."""
    case = Case(name)
    model = case.build_model().to(gpu_device)
    g = torch.Generator().manual_seed(19)
    W, F = case.kwargs["window_size"], case.kwargs["n_features"]
    x = torch.rand(n_mid, W, F, generator=g)
    n = case.x.shape[0]
    x[100:100 + n] = case.x
    x = x.to(gpu_device)
    cus = device_compute_units(gpu_device)
    with torch.no_grad():
        p_mid, r_mid = model(x)
        p_small, r_small = model(x[1000:1300].contiguous())
        eng = model._sync_engine(gpu_device)
        outs, routes = {}, {0: call_routes(eng, n_mid, cus)}
        try:
            for k in (1, 2, 3):
                eng.set_option("gru_kernel", k)
                routes[k] = call_routes(eng, n_mid, cus)
                outs[k] = model(x)
            eng.set_option("gru_kernel", 1)
            eng.set_option("lanes", 1)
            routes["tile"] = call_routes(eng, N_TILE, cus)
            x_tile = torch.cat([x] * (N_TILE // n_mid + 1))[:N_TILE].contiguous()
            outs["tile"] = model(x_tile)
        finally:
            eng.set_option("gru_kernel", 0)
            eng.set_option("lanes", 0)
    want, i = MID_ROUTES[name], (3000, 8192).index(n_mid)
    assert routes[0] == ([n_mid], [want["auto"]]) and routes[3] == routes[0], routes
    assert routes[1] == ([n_mid], [want["k1"][i]]) and routes[2] == ([n_mid], [want["k2"][i]]), routes
    assert routes["tile"] == ([N_TILE], [want["tile"]]), routes
    gate(p_mid[100:100 + n], case.preds, case.preds64, what=f"preds in a {n_mid}-window batch")
    gate(r_mid[100:100 + n], case.recons, case.recons64, what=f"recons in a {n_mid}-window batch")
    assert (p_mid[1000:1300] - p_small).abs().max().item() <= 2e-6
    assert (r_mid[1000:1300] - r_small).abs().max().item() <= 2e-6
    assert torch.equal(outs[3][0], p_mid) and torch.equal(outs[3][1], r_mid)       # the automatic choice in this band
    for k in (1, 2):
        assert (outs[k][0] - p_mid).abs().max().item() <= 2e-6 and (outs[k][1] - r_mid).abs().max().item() <= 2e-6, k
    gate(outs["tile"][0][100:100 + n], case.preds, case.preds64, what="preds, tile-major kernel on split operands")
    gate(outs["tile"][1][100:100 + n], case.recons, case.recons64, what="recons, tile-major kernel on split operands")
    assert (outs["tile"][0][:n_mid] - p_mid).abs().max().item() <= 2e-6 and (outs["tile"][1][:n_mid] - r_mid).abs().max().item() <= 2e-6
