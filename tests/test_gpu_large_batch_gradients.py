"""Per-window input gradients and score attributions of LARGE calls against float64.

The data path of the training step picks its kernels by the size of each call: from 65 536 (window, step) rows the backward's
data-gradient and projection GEMMs run on split-bf16 operands, from 2 561 windows the training recurrences on split operands, from
4 096 k_gath keeps the softmax rows and applies dropout in the training forward, above 4 096 the backward recurrence leaves the
16-window-group kernel, above TRAIN_CHUNK = 8 192 the Python step walks chunks, and score attribution runs thousands of windows per
chunk.  Under the window-separable loss  L = sum_w <cp_w, preds_w> + <cr_w, recons_w>  the gradient d L / d x_w depends on window w
alone, so a float64 evaluation of a sample of windows (tests/helpers.py) is an exact reference for a call of any size.

Gate per window (helpers.window_gate): max |ours_w - ref64_w| <= 1e-6 + 1e-4 max |ref64_w|, or within the fp32 torch-op route's
own distance from float64 for that window + 1e-6 + 1e-5 max |ref64_w|.  Windows with a ReLU / LeakyReLU argument within 1e-6 of
its kink are left out (helpers.kink_windows) and counted.  Run with -s to see the worst ratio err / bound of every band."""
import copy

import pytest
import torch

import helpers
from helpers import Case

pytestmark = pytest.mark.gpu

MODES = ("fp32", "fp32_strict")                  # precision mode 2 (split operands on the large-batch kernels) and mode 0
P_DROP = 0.3
TRAIN_CHUNK = 8192                               # _hipgrad.TRAIN_CHUNK

ODD_SHAPES = dict(n_features=12, window_size=30, out_dim=12, kernel_size=5, gru_hid_dim=40, forecast_n_layers=2, forecast_hid_dim=36,
                  recon_hid_dim=44, dropout=P_DROP, alpha=0.2)
MODELS = {
    "msl": "msl",                                # the shipped checkpoint: F 55, W 100, H 150
    "odd_shapes": ODD_SHAPES,                    # H 40: split-operand training recurrence and k_gru16 both apply
    "v1_msl_shape": dict(n_features=25, window_size=100, out_dim=1, kernel_size=7, use_gatv2=False, gru_hid_dim=150, forecast_n_layers=3,
                         forecast_hid_dim=150, recon_hid_dim=150, dropout=P_DROP, alpha=0.2),
    # stacked recurrences: the 16-window-group kernels never apply
    "stacked": dict(n_features=6, window_size=14, out_dim=2, kernel_size=3, gru_n_layers=2, gru_hid_dim=40, forecast_n_layers=1,
                    forecast_hid_dim=20, recon_n_layers=2, recon_hid_dim=36, dropout=P_DROP, alpha=0.2),
    # W F = 22 400 > 16 384, 160 / 140 nodes: the unfused attention route
    "wide_window": dict(n_features=140, window_size=160, out_dim=2, kernel_size=5, feat_gat_embed_dim=21, time_gat_embed_dim=9,
                        gru_hid_dim=32, forecast_n_layers=1, forecast_hid_dim=24, recon_hid_dim=28, dropout=P_DROP, alpha=0.2),
}
# call sizes: both sides of 65 536 rows (n W), of the split-operand recurrence (2 561), of k_gath / k_gru_bwd (4 096), one chunk
SIZES = {
    "msl": [655, 656, 2560, 2561, 4096, 4097, 8193],
    "v1_msl_shape": [655, 656, 2560, 2561, 4096, 4097, 8193],
    "odd_shapes": [2184, 2185, 2560, 2561, 4096, 4097, 8193, 20000],
    "stacked": [2560, 2561, 4096, 4097, 4681, 4682, 8193],
    "wide_window": [420],
}

_worst = {}                                      # band -> (worst ratio, rejected windows, sampled windows)
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _worst:
        print("\nworst per-window err / (1e-6 + 1e-4 max|ref64|) by band:")
        for band, (r, rej, n) in sorted(_worst.items()):
            print(f"  {band:55s} {r:8.4f}   kinks rejected {rej}/{n}")


def _record(band, ratio, rejected, n):
    r0 = _worst.get(band, (0.0, 0, 0))
    _worst[band] = (max(r0[0], ratio), r0[1] + rejected, r0[2] + n)
    print(f"{band}: worst ratio {ratio:.4f} (kinks rejected {rejected}/{n})")


def _cpu_model(spec, seed=0):
    from mtad_gat import MTAD_GAT
    if isinstance(spec, str):
        return Case(spec).build_model().eval()
    torch.manual_seed(seed)
    m = MTAD_GAT(**spec)
    with torch.no_grad():
        m.feature_gat.bias.normal_()
        m.temporal_gat.bias.normal_()
    return m.eval()


def _models(name, device):
    """(GPU model, float64 CPU copy, float32 CPU copy) -- built once per module."""
    if name not in _cache:
        cpu = _cpu_model(MODELS[name])
        _cache[name] = (copy.deepcopy(cpu).to(device), helpers.model64(cpu), copy.deepcopy(cpu).eval())
    gm = _cache[name][0]
    gm.eval()
    return _cache[name]


def _edges(window):
    return [-(-65536 // window), 2560, 2561, 4096, 4097, TRAIN_CHUNK, 2 * TRAIN_CHUNK]


def _take(masks, rows, dtype):
    if masks is None:
        return None
    return {k: ([t[rows].to(dtype) for t in v] if isinstance(v, list) else v[rows].to(dtype)) for k, v in masks.items()}


def _dx_reference(m64, m32, xs, cps, crs, masks, chunk=8):
    """(keep (k,) bool, float64 d x of the kept windows, fp32-route evaluator of rows of the kept windows)."""
    bad = helpers.kink_windows(m64, xs, masks)
    keep = (~bad).nonzero().flatten().tolist()
    assert len(keep) >= 0.9 * xs.shape[0], f"{int(bad.sum())} of {xs.shape[0]} sampled windows sit at a kink: change the seed"
    parts = []
    for lo in range(0, len(keep), chunk):
        r = keep[lo:lo + chunk]
        parts.append(helpers.separable_input_grad(m64, xs[r].double(), cps[r], crs[r], _take(masks, r, torch.float64)))
    ref = torch.cat(parts)

    def ref32_of(rows):
        r = [keep[i] for i in rows]
        return helpers.separable_input_grad(m32, xs[r].float(), cps[r], crs[r], _take(masks, r, torch.float32))
    return keep, ref, ref32_of, int(bad.sum())


# ---- A. Engine.backward_data by band ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,b", [(n, b) for n, sizes in SIZES.items() for b in sizes])
def test_backward_data_per_window(name, b, gpu_device):
    gm, m64, m32 = _models(name, gpu_device)
    W, F, od = gm.window_size, gm.n_features, gm.out_dim
    g = torch.Generator(device=gpu_device).manual_seed(1000 + b)
    x = torch.rand(b, W, F, generator=g, device=gpu_device)
    cp, cr = helpers.separable_cotangents(b, W, od, seed=2000 + b, device=gpu_device)
    rows = helpers.sample_windows(b, _edges(W), n=32, seed=b, groups=(16, 32, 128))
    xs, cps, crs = x[rows].cpu(), cp[rows].cpu(), cr[rows].cpu()
    for p, w0 in ((0.0, 0), (P_DROP, 12345)):
        seed = 0 if p == 0.0 else 0x5EED0000 + b
        eng = gm._sync_engine(gpu_device)
        masks = helpers.masks_at(eng, [w0 + r for r in rows], p, seed, gpu_device)
        keep, ref, ref32_of, rejected = _dx_reference(m64, m32, xs, cps, crs, masks)
        for mode in MODES:
            gm.precision = mode
            eng = gm._sync_engine(gpu_device)
            _, _, tape = eng.forward_train(x, p, seed, w0)
            dx = eng.backward_data(x, p, seed, cp, cr, tape, w0)
            ours = dx[rows].cpu()[keep]
            del tape, dx
            band = f"A {name} n={b} {mode} p={p}"
            _record(band, helpers.window_gate(ours, ref, ref32_of, band), rejected, len(rows))
    gm.precision = "auto"


# ---- B. model(x) with x.requires_grad across TRAIN_CHUNK chunks ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["msl", "odd_shapes"])
@pytest.mark.parametrize("b", [TRAIN_CHUNK + 1, TRAIN_CHUNK + 4096])
def test_model_input_gradient_across_train_chunks(name, b, gpu_device):
    """Two chunks of the Python step: the backward re-runs each chunk's forward with window0 = lo; at 12 288 windows the second
    chunk (4 096 windows from window0 = 8 192) takes k_gath with dropout."""
    gm, m64, m32 = _models(name, gpu_device)
    W, F, od = gm.window_size, gm.n_features, gm.out_dim
    g = torch.Generator(device=gpu_device).manual_seed(3000 + b)
    x0 = torch.rand(b, W, F, generator=g, device=gpu_device)
    cp, cr = helpers.separable_cotangents(b, W, od, seed=4000 + b, device=gpu_device)
    rows = helpers.sample_windows(b, _edges(W), n=32, seed=b + 1, groups=(16, 32, 128))
    xs, cps, crs = x0[rows].cpu(), cp[rows].cpu(), cr[rows].cpu()
    try:
        for train in (False, True):
            gm.train(train)
            torch.manual_seed(77)
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if train else 0     # what _hipgrad.forward will draw
            masks = helpers.masks_at(gm._sync_engine(gpu_device), rows, gm.dropout_p, seed, gpu_device) if train else None
            keep, ref, ref32_of, rejected = _dx_reference(m64, m32, xs, cps, crs, masks)
            for mode in MODES:
                gm.precision = mode
                x = x0.clone().requires_grad_(True)
                torch.manual_seed(77)
                pr, rc = gm(x)
                assert gm.grad_path == "hip", gm.grad_path
                ((pr * cp).sum() + (rc * cr).sum()).backward()
                ours = x.grad[rows].cpu()[keep]
                del pr, rc, x
                for q in gm.parameters():
                    q.grad = None
                band = f"B {name} n={b} {mode} {'train' if train else 'eval'}"
                _record(band, helpers.window_gate(ours, ref, ref32_of, band), rejected, len(rows))
    finally:
        gm.eval()
        gm.precision = "auto"


# ---- C. parameter gradients across the TRAIN_CHUNK boundary --------------------------------------------------------------------
def test_parameter_gradients_across_the_train_chunk(gpu_device):
    """odd_shapes, 12 288 windows with dropout: every parameter's gradient against float64 over ALL windows (CPU chunks of 1 024
    windows with the library's masks of those windows), gated per parameter as test_gpu_backward._grad_report.

    Windows with an argument near a kink -- the GATv2 pair arguments included -- get zero cotangents: in a sum over 12 288 windows
    with random-sign cotangents a few such windows put the fp32 torch-op route itself up to 1e-3 of the scale away from float64
    in feature_gat.lin (the sign of |u_ij| flips with the rounding); without them the HIP step is within a tenth of the gate."""
    gm, m64, _ = _models("odd_shapes", gpu_device)
    b, W, F, od = TRAIN_CHUNK + 4096, gm.window_size, gm.n_features, gm.out_dim
    g = torch.Generator(device=gpu_device).manual_seed(5000)
    x = torch.rand(b, W, F, generator=g, device=gpu_device)
    cp, cr = helpers.separable_cotangents(b, W, od, seed=5001, device=gpu_device)
    torch.manual_seed(78)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    eng = gm._sync_engine(gpu_device)
    names = [n for n, _ in m64.named_parameters()]
    params64 = [q for _, q in m64.named_parameters()]
    ref = [torch.zeros_like(q) for q in params64]
    import _torchpath
    chunks = []
    for lo in range(0, b, 1024):
        hi = min(b, lo + 1024)
        ms = eng.dropout_masks(hi - lo, P_DROP, seed, gpu_device, window0=lo)
        ms = {k: ([t.cpu().double() for t in v] if isinstance(v, list) else v.cpu().double()) for k, v in ms.items()}
        chunks.append((lo, hi, ms))
        bad = helpers.kink_windows(m64, x[lo:hi].cpu().double(), ms, gatv2_pairs=True)
        cp[lo:hi][bad.to(gpu_device)] = 0.0
        cr[lo:hi][bad.to(gpu_device)] = 0.0
    zeroed = int((cp.abs().sum(1) == 0).sum())
    assert zeroed < 0.1 * b, f"{zeroed} of {b} windows sit at a kink: change the seed"
    for lo, hi, ms in chunks:
        pr, rc = _torchpath.forward(m64, x[lo:hi].cpu().double(), ms)
        gs = torch.autograd.grad((pr * cp[lo:hi].cpu().double()).sum() + (rc * cr[lo:hi].cpu().double()).sum(), params64)
        for r, q in zip(ref, gs):
            r += q
    ref = dict(zip(names, ref))
    try:
        gm.train()
        for mode in MODES:
            gm.precision = mode
            for q in gm.parameters():
                q.grad = None
            torch.manual_seed(78)
            pr, rc = gm(x)
            assert gm.grad_path == "hip"
            ((pr * cp).sum() + (rc * cr).sum()).backward()
            worst, bad = 0.0, []
            for n, q in gm.named_parameters():
                r = ref[n]
                d = (q.grad.cpu().double() - r).abs().max().item()
                bound = 1e-5 + 1e-4 * r.abs().max().item()
                worst = max(worst, d / bound)
                if not d <= bound or not torch.isfinite(q.grad).all():
                    bad.append(f"{n}: |diff| {d:.3e} > {bound:.3e}")
            _record(f"C odd_shapes n={b} {mode} parameter gradients", worst, zeroed, b)
            assert not bad, "\n".join(bad)
    finally:
        for q in gm.parameters():
            q.grad = None
        gm.eval()
        gm.precision = "auto"


# ---- D. score attribution at production sizes --------------------------------------------------------------------------------
def _attr_units(eng, count, steps):
    """(index, step) units per chunk of mtadgat_score_attribution, read from the workspace size (it grows with the units of a chunk
    and stops growing at the chunk's capacity); None when all count * max(steps, 1) units fit one chunk."""
    total = count * max(steps, 1)
    ws = [eng.score_attribution_workspace_bytes(u, 0) for u in (total - 1, total)]
    if ws[1] > ws[0]:
        return None
    lo, hi = 1, total                            # smallest u with ws(u) == ws(total)
    while lo < hi:
        mid = (lo + hi) // 2
        if eng.score_attribution_workspace_bytes(mid, 0) == ws[1]:
            hi = mid
        else:
            lo = mid + 1
    return lo


ATTR = {
    # name: (model, count, index stride, method kwargs, baseline, scale_scores, gamma, target_dims, chunk windows)
    # chunk None: the default (at the MSL shape the 4 GiB scratch bound: 895 units of 2 windows), "one": all units in one chunk
    "msl_ig32": ("msl", 160, 7, dict(method="integrated", steps=32), None, False, 1.0, [0], None),
    "msl_gradient": ("msl", 3000, 1, dict(method="gradient"), None, False, 1.0, [0], None),
    "odd_ig32_zeros": ("odd_shapes", 200, 5, dict(method="integrated", steps=32), None, False, 1.0, None, "one"),
    "odd_ig32_row": ("odd_shapes", 200, 5, dict(method="integrated", steps=32), "row", False, 1.0, None, 4000),
    "odd_ig32_slice": ("odd_shapes", 200, 5, dict(method="integrated", steps=32), "slice", False, 1.0, None, 4000),
    "odd_ig32_scaled": ("odd_shapes", 200, 5, dict(method="integrated", steps=32), None, True, 0.4, None, 4000),
}


@pytest.mark.parametrize("case", list(ATTR))
def test_score_attribution_per_index(case, gpu_device):
    import _torchpath
    from mtad_gat import _column_quantiles
    name, count, stride, meth, base_kind, scaled, gamma, dims, chunk = ATTR[case]
    gm, m64, m32 = _models(name, gpu_device)
    W, F = gm.window_size, gm.n_features
    steps = meth.get("steps", 0)
    m = max(steps, 1)
    gen = torch.Generator().manual_seed(6000 + count)
    values = torch.rand(W + 1 + stride * count + 3, F, generator=gen)
    idx = [3 + stride * i for i in range(count)]
    baseline = None
    if base_kind == "row":
        baseline = values.mean(0)
    elif base_kind == "slice":
        baseline = torch.rand(W + 1, F, generator=gen)
    eng = gm._sync_engine(gpu_device)
    old_chunk = eng.chunk_windows()
    try:
        if isinstance(chunk, int):
            eng.set_chunk_windows(chunk)
        units = _attr_units(eng, count, steps)
        if chunk == "one":
            assert units is None, "the call was meant to run in one chunk"     # 200 indices x 32 steps: 12 800 windows at once
            units = count * m
        elif chunk is None:
            assert units is not None and units < count * m, "the call was meant to run in several chunks"
        else:
            assert units == chunk // 2, units
        straddle = helpers.straddling_indices(count, steps, units)
        assert straddle or steps == 0 or units >= count * m
        bounds = [u0 // m for u0, _ in helpers.attribution_chunks(count, steps, units)[1:]]      # first index of a later chunk
        pos = sorted({0, 1, count - 2, count - 1, *straddle[:3], *straddle[-2:], *[q + d for q in bounds[:2] for d in (-1, 0)]})
        pos += [q for q in torch.randperm(count, generator=gen)[:16].tolist() if q not in pos][: max(0, 10 - len(pos))]
        pos = sorted(pos)
        ours = {}
        for mode in MODES:
            gm.precision = mode
            out = gm.score_attribution(values.to(gpu_device), idx, target_dims=dims, gamma=gamma, scale_scores=scaled,
                                       baseline=None if baseline is None else baseline.to(gpu_device), **meth)
            ours[mode] = out[pos].cpu()
    finally:
        eng.set_chunk_windows(old_chunk)
        gm.precision = "auto"
    # float64 reference of the sampled indices only (indices are independent); w_d as MTAD_GAT.score_attribution builds it
    dl = list(range(F)) if dims is None else dims
    v64 = values.double()
    b64 = None if baseline is None else baseline.double()
    dim_w = torch.full((len(dl),), 1.0 / len(dl), dtype=torch.float64)
    if scaled:
        per_dim = _torchpath.per_dim_scores(m64, v64, dl, gamma)
        qs = torch.tensor([0.25, 0.75], dtype=torch.float64)
        q = torch.stack([_column_quantiles(per_dim[:, d], qs) for d in range(per_dim.shape[1])], dim=1)
        dim_w = dim_w / (1.0 + (q[1] - q[0]))
    # sign(0) is where the score is not differentiable: no sampled unit may have a residual near it at any step
    with torch.no_grad():
        for p_ in pos:
            S = v64[idx[p_]: idx[p_] + W + 1]
            bb = torch.zeros_like(S) if b64 is None else b64.expand_as(S)
            Z = torch.stack([bb + ((k + 0.5) / m) * (S - bb) for k in range(m)]) if steps else S[None]
            pa, _ = _torchpath.forward(m64, Z[:, :W])
            _, rb = _torchpath.forward(m64, Z[:, 1:])
            y = Z[:, W][:, dl]
            res = torch.minimum((pa - y).abs().min(), (rb[:, -1] - y).abs().min()).item()
            assert res >= 1e-4, f"{case}: index {idx[p_]} has a residual of {res:.2e}: pick another series seed"
    ref = _torchpath.score_attribution(m64, v64, [idx[p_] for p_ in pos], dl, dim_w, gamma, steps, b64)

    def ref32_of(rows):
        return _torchpath.score_attribution(m32, values, [idx[pos[r]] for r in rows], dl, dim_w.float(), gamma, steps, baseline)
    for mode in MODES:
        band = f"D {case} {mode} ({count} indices, {units} units / chunk, {len([p_ for p_ in pos if p_ in straddle])} straddling)"
        _record(band, helpers.window_gate(ours[mode], ref, ref32_of, band), 0, len(pos))


# ---- E. k_gat without k_gath in front (gat_kernel = 1) from 4 096 windows --------------------------------------------------------
def test_gat_kernel_1_large_batches_match_float64(gpu_device):
    """gat_kernel = 1 keeps k_gath out of the GATv2 layers.  From 4 096 windows in mode 2 k_gat then used to take the fp16-piece
    pack, which is in k_gath's compact column order: wrong attention outputs whenever a layer's number of non-negative columns
    mod 8 is neither 0 nor 7 (the compact and the 8-padded order differ).  Inference and the training forward, per window."""
    from oracle import mtad_gat_oracle as oracle
    cpu = _cpu_model(ODD_SHAPES, seed=3)
    for layer in (cpu.feature_gat, cpu.temporal_gat):
        a = layer.a.detach().double().flatten()
        npos = int(((1.0 - cpu.alpha) * 0.5 * a >= 0.0).sum())              # k_gat_colorder's sign convention
        assert npos % 8 not in (0, 7), npos
    gm = copy.deepcopy(cpu).to(gpu_device)
    gm.precision = "fp32"
    eng = gm._sync_engine(gpu_device)
    assert eng.chunk_windows() >= 6000
    eng.set_option("gat_kernel", 1)
    sd = cpu.state_dict()
    for b in (4096, 6000):
        g = torch.Generator(device=gpu_device).manual_seed(7000 + b)
        x = torch.rand(b, gm.window_size, gm.n_features, generator=g, device=gpu_device)
        rows = helpers.sample_windows(b, [4096], n=32, seed=b)
        xs = x[rows].cpu()
        p32, r32 = oracle.forward(xs, sd, alpha=cpu.alpha)
        p64, r64 = oracle.forward(xs.double(), sd, alpha=cpu.alpha)
        with torch.no_grad():
            pi, ri = gm(x)
        eng = gm._sync_engine(gpu_device)
        pt, rt, _ = eng.forward_train(x, 0.0, 0)
        for what, ours, ref32, ref64 in (("inference preds", pi, p32, p64), ("inference recons", ri, r32, r64),
                                         ("forward_train preds", pt, p32, p64), ("forward_train recons", rt, r32, r64)):
            o = ours[rows].cpu()
            for j in range(len(rows)):
                helpers.gate(o[j], ref32[j], ref64[j], what=f"gat_kernel=1 n={b} {what} window {rows[j]}")
            _record(f"E gat_kernel=1 n={b} {what}", (o.double() - ref64).abs().max().item() / helpers.FP32_TOL, 0, len(rows))
    eng.set_option("gat_kernel", 0)
