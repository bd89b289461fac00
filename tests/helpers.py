"""Shared test helpers: golden fixtures (tests/golden/*.npz, generated from the reference by
tests/golden/make_golden.py) and tolerance gates."""
import hashlib
import json
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_CASES = ["msl", "smap", "smd_1_1", "syn_v1_small", "syn_v2_embed", "syn_v2_wide", "syn_v1_default", "syn_c4"]
SHIPPED_CASES = ["msl", "smap", "smd_1_1"]
FP32_TOL = 1e-5   # BASELINE.json north_star: outputs within 1e-5 of the reference fp32 forward


def sd_digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


class Case:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.name = name
        self.meta = json.loads(bytes(z["meta"]).decode())
        self.kwargs = self.meta["kwargs"]
        self.x = torch.from_numpy(z["x"])
        self.preds = torch.from_numpy(z["preds"])
        self.recons = torch.from_numpy(z["recons"])
        self.preds64 = torch.from_numpy(z["preds64"])
        self.recons64 = torch.from_numpy(z["recons64"])
        self.h_end64 = torch.from_numpy(z["h_end64"])
        self.stages = {k[len("stage_"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("stage_")}
        self._sd = {k[len("sd/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")} or None

    def build_model(self):
        """Our MTAD_GAT with this case's parameters (CPU).  Cases that do not store the state_dict
        re-create it from the recorded seeds; the digest check proves it equals the reference's."""
        from mtad_gat import MTAD_GAT
        if self._sd is not None:
            model = MTAD_GAT(**self.kwargs)
            model.load_state_dict(self._sd)   # strict
        else:
            torch.manual_seed(self.meta["init_seed"])
            model = MTAD_GAT(**self.kwargs)
            g = torch.Generator().manual_seed(self.meta["init_seed"] + 1)
            with torch.no_grad():
                model.feature_gat.bias.copy_(torch.randn(model.feature_gat.bias.shape, generator=g))
                model.temporal_gat.bias.copy_(torch.randn(model.temporal_gat.bias.shape, generator=g))
        assert sd_digest(model.state_dict()) == self.meta["sd_sha256"], "parameters differ from the reference's"
        return model.eval()

    def state_dict(self):
        return self._sd if self._sd is not None else self.build_model().state_dict()


def gate(ours, ref32, ref64=None, tol=FP32_TOL, what=""):
    """|ours - ref32| <= tol, or -- so a kernel *more* accurate than the reference's own float32
    rounding is not failed -- |ours - ref64| <= |ref32 - ref64| + tol."""
    ours = ours.detach().cpu().double()
    d32 = (ours - ref32.double()).abs().max().item()
    if d32 <= tol:
        return d32
    if ref64 is not None:
        d64 = (ours - ref64.double()).abs().max().item()
        noise = (ref32.double() - ref64.double()).abs().max().item()
        assert d64 <= noise + tol, f"{what}: |ours-ref32|={d32:.3e}, |ours-ref64|={d64:.3e} > ref noise {noise:.3e} + {tol}"
        return d32
    raise AssertionError(f"{what}: max abs diff {d32:.3e} > {tol}")


WIDE_CASES = ["msl_wide", "smap_wide", "smd_1_1_wide", "msl_c1"]


class WideCase:
    """>= 256-window fixture of a shipped checkpoint (tests/golden/make_golden.py --wide): reference
    outputs only; the input is regenerated from the recorded seed (or the stored C1 series) and
    checked against the recorded sha-256, the weights come from the small fixture of the same checkpoint."""

    def __init__(self, name):
        import hashlib
        z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.name = name
        self.meta = json.loads(bytes(z["meta"]).decode())
        self.kwargs = self.meta["kwargs"]
        self.base = Case({"msl_wide": "msl", "smap_wide": "smap", "smd_1_1_wide": "smd_1_1", "msl_c1": "msl"}[name])
        self.preds = torch.from_numpy(z["preds"])
        self.recons = torch.from_numpy(z["recons"])
        self.preds64 = torch.from_numpy(z["preds64_f32"])
        self.recons64 = torch.from_numpy(z["recons64_f32"])
        self.h_end = torch.from_numpy(z["stage_h_end"])
        if "series" in z.files:
            self.series = torch.from_numpy(z["series"])
            w = self.kwargs["window_size"]
            self.x = torch.stack([self.series[i:i + w] for i in range(self.meta["batch"])])
        else:
            self.series = None
            g = torch.Generator().manual_seed(4321)
            self.x = torch.rand(self.meta["batch"], self.kwargs["window_size"], self.kwargs["n_features"], generator=g)
        assert hashlib.sha256(self.x.numpy().tobytes()).hexdigest() == self.meta["x_sha256"], "regenerated input differs"

    def build_model(self):
        return self.base.build_model()

    def state_dict(self):
        return self.base.state_dict()


# ---- the library's counter-based dropout, restated (csrc/mtadgat_device.h: mix32 / drop_window_key / drop_keep;
# stream numbers csrc/mtadgat_kernels.h: DROP_FEAT = 1, DROP_TEMP = 2, DROP_FC0 = 16).  The reference draws its masks from
# torch's generator (modules.py:90, :189, :310); to hold the reference's gradients WITH dropout as a fixture, the fixture
# generator injects these masks into the unmodified reference and the GPU test runs the kernels with the same seed.
def _mix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16); x *= np.uint32(0x7FEB352D); x ^= x >> np.uint32(15); x *= np.uint32(0x846CA68B); x ^= x >> np.uint32(16)
    return x


def dropout_keep_mask(seed, stream, p, n_windows, n_per_window, window0=0):
    """float32 (n_windows, n_per_window) of 0/1: element e of window w is kept iff the library's hash says so."""
    if p <= 0.0:
        return np.ones((n_windows, n_per_window), np.float32)
    t = p * 4294967296.0
    thresh = np.uint32(4294967295 if t >= 4294967295.0 else max(int(t), 1))
    w = np.arange(window0, window0 + n_windows, dtype=np.uint64)
    lo, hi = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32), (w >> np.uint64(32)).astype(np.uint32)
    seed_lo, seed_hi = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        h = _mix32(lo ^ seed_lo)
        h = _mix32(h + hi * np.uint32(0x9E3779B9) + seed_hi + np.uint32((stream * 0x85EBCA6B) & 0xFFFFFFFF))
        e = np.arange(n_per_window, dtype=np.uint32) * np.uint32(0x9E3779B1) + np.uint32(0x7F4A7C15)
        keep = _mix32(h[:, None] ^ e[None, :]) >= thresh
    return keep.astype(np.float32)


def dropout_masks_like_the_library(kwargs, batch, seed, window0=0):
    """{"feat": (b,F,F), "temp": (b,W,W), "fc": [(b,hid)] * hidden layers} -- the layout of Engine.dropout_masks."""
    p, F_, W_ = kwargs["dropout"], kwargs["n_features"], kwargs["window_size"]
    hid, nh = kwargs["forecast_hid_dim"], kwargs["forecast_n_layers"]
    return {"feat": torch.from_numpy(dropout_keep_mask(seed, 1, p, batch, F_ * F_, window0)).reshape(batch, F_, F_),
            "temp": torch.from_numpy(dropout_keep_mask(seed, 2, p, batch, W_ * W_, window0)).reshape(batch, W_, W_),
            "fc": [torch.from_numpy(dropout_keep_mask(seed, 16 + i, p, batch, hid, window0)) for i in range(nh)]}


GRAD_CASES = ["grads_msl_eval", "grads_msl_masks", "grads_smd_eval", "grads_smd_masks", "grads_msl_b2000_masks", "grads_msl_b4100_eval"]


class GradCase:
    """Reference-held gradients of the training loss (tests/golden/make_golden.py --grads): every parameter's gradient from
    the unmodified reference model on CPU (float32), the per-parameter rounding noise of that computation (max |g32 - g64|
    against the same model in float64), the outputs at a few windows.  Inputs are regenerated from the recorded seeds and
    checked against their sha-256; weights come from the shipped checkpoint's small fixture."""

    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.name = name
        self.meta = json.loads(bytes(z["meta"]).decode())
        self.kwargs = self.meta["kwargs"]
        self.base = Case(self.meta["weights_from"])
        self.grads = {k[len("g/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("g/")}
        self.noise = {k[len("n/"):]: float(z[k]) for k in z.files if k.startswith("n/")}
        self.preds_head = torch.from_numpy(z["preds_head"])
        self.recons_head = torch.from_numpy(z["recons_head"])
        self.loss = [float(v) for v in z["loss"]]
        self.x, self.y = grad_case_inputs(self.kwargs, self.meta["batch"], self.meta["xy_seed"])
        assert hashlib.sha256(self.x.numpy().tobytes() + self.y.numpy().tobytes()).hexdigest() == self.meta["xy_sha256"], \
            "torch.rand no longer reproduces the fixture's inputs"


def grad_case_inputs(kwargs, batch, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(batch, kwargs["window_size"], kwargs["n_features"], generator=g)
    y = torch.rand(batch, 1, kwargs["n_features"], generator=g)
    return x, y


def training_loss(preds, recons, x, y, target_dims):
    """reference training.py:113-124, verbatim in meaning: returns (forecast_loss, recon_loss)."""
    if target_dims is not None:
        x = x[:, :, target_dims]
        y = y[:, :, target_dims].squeeze(-1)
    if preds.ndim == 3:
        preds = preds.squeeze(1)
    if y.ndim == 3:
        y = y.squeeze(1)
    mse = torch.nn.MSELoss()
    return torch.sqrt(mse(y, preds)), torch.sqrt(mse(x, recons))


# ---- float64 per-window references of large GPU calls (tests/test_gpu_large_batch_gradients.py) ---------------------------------
# The check of a call of b windows evaluates only a sample of them: under the window-separable loss
#     L = sum_w <cp_w, preds_w> + <cr_w, recons_w>
# (seeded random cotangents cp, cr) d L / d x_w depends on window w alone, so the reference of a sampled window is exact.
WINDOW_ABS, WINDOW_REL, WINDOW_NOISE_REL = 1e-6, 1e-4, 1e-5     # the global gates of the existing gradient tests, per window
KINK_REL = 1e-6


def model64(model):
    """A float64 copy of `model` on the CPU in eval mode (dropout only through explicit masks)."""
    import copy
    return copy.deepcopy(model).cpu().double().eval()


def separable_cotangents(b, window, out_dim, seed, device="cpu"):
    """(cp (b, out_dim), cr (b, window, out_dim)) float32 normal cotangents of the window-separable loss."""
    g = torch.Generator(device=device).manual_seed(seed)
    cp = torch.randn(b, out_dim, generator=g, device=device)
    cr = torch.randn(b, window, out_dim, generator=g, device=device)
    return cp, cr


def separable_input_grad(model, x, cp, cr, masks=None):
    """d/dx of sum_w <cp_w, preds_w> + <cr_w, recons_w> through the torch-op algebra (_torchpath.forward) in model's dtype."""
    import _torchpath
    dt = next(model.parameters()).dtype
    x = x.detach().to(dt).requires_grad_(True)
    with torch.enable_grad():
        pr, rc = _torchpath.forward(model, x, masks)
        return torch.autograd.grad((pr * cp.to(dt)).sum() + (rc * cr.to(dt)).sum(), x)[0]


def masks_at(eng, windows, p, seed, device, dtype=torch.float64):
    """The library's keep-masks (Engine.dropout_masks) of the given GLOBAL windows, stacked, on the CPU in `dtype`; None for p = 0."""
    if p <= 0.0:
        return None
    parts = [eng.dropout_masks(1, p, seed, device, window0=int(w)) for w in windows]

    def cat(ms):
        return torch.cat([m.cpu() for m in ms]).to(dtype)
    out = {"feat": cat([q["feat"] for q in parts]), "temp": cat([q["temp"] for q in parts]),
           "fc": [cat([q["fc"][i] for q in parts]) for i in range(len(parts[0]["fc"]))]}
    for key in ("gru", "rec"):
        if key in parts[0]:
            out[key] = [cat([q[key][i] for q in parts]) for i in range(len(parts[0][key]))]
    return out


def host_masks_at(kwargs, windows, p, seed, dtype=torch.float64):
    """masks_at without a GPU: the same keep-masks of the given GLOBAL windows from the restated hash (dropout_keep_mask), the
    masks between stacked recurrence layers included (streams DROP_GRU0 = 64 + l / DROP_REC0 = 96 + l, element t * H + j of a
    window: k_seq_dropout); None for p = 0.  tests/test_gpu_train_routes.py holds it equal to the library's."""
    if p <= 0.0:
        return None
    W = kwargs["window_size"]
    parts = [dropout_masks_like_the_library(kwargs, 1, seed, window0=int(w)) for w in windows]
    out = {"feat": torch.cat([q["feat"] for q in parts]).to(dtype), "temp": torch.cat([q["temp"] for q in parts]).to(dtype),
           "fc": [torch.cat([q["fc"][i] for q in parts]).to(dtype) for i in range(len(parts[0]["fc"]))]}
    lg, ld = kwargs.get("gru_n_layers", 1) - 1, kwargs.get("recon_n_layers", 1) - 1
    if lg > 0 or ld > 0:
        for key, layers, stream0, H in (("gru", lg, 64, kwargs["gru_hid_dim"]), ("rec", ld, 96, kwargs["recon_hid_dim"])):
            out[key] = [torch.cat([torch.from_numpy(dropout_keep_mask(seed, stream0 + l, p, 1, W * H, int(w))).reshape(1, W, H)
                                   for w in windows]).to(dtype) for l in range(layers)]
    return out


def _near_zero(t, rel):
    """bool per window (dim 0): some entry of t within rel * (the window's max |entry|) of zero."""
    t = t.flatten(1).abs()
    return (t < rel * t.amax(1, keepdim=True)).any(1) if t.shape[1] else torch.zeros(t.shape[0], dtype=torch.bool)


def kink_windows(m64, x, masks=None, rel=KINK_REL, gatv2_pairs=False):
    """bool (k,): windows whose float64 evaluation puts a convolution ReLU, a forecasting ReLU or a GAT (v1) LeakyReLU argument
    within `rel` of zero, relative to that layer's largest |argument| in the window.  Either side's rounding can put such a point
    on the other side of the kink: a property of the input, not of the kernels.  gatv2_pairs: also the GATv2 LeakyReLU arguments
    u_ij = W_l v_i + b + W_r v_j (K * K * E per layer and window) -- one sign flip there moves a sum of parameter gradients over
    thousands of windows by more than the summation's rounding does."""
    import torch.nn.functional as F
    import _torchpath as tp
    masks = masks or {}
    with torch.no_grad():
        x = x.to(torch.float64)
        conv = m64.conv.conv
        pad = (conv.kernel_size[0] - 1) // 2
        pre = F.conv1d(F.pad(x.permute(0, 2, 1), (pad, pad)), conv.weight, conv.bias)
        bad = _near_zero(pre, rel)
        xc = F.relu(pre).permute(0, 2, 1)
        for layer, v in ((m64.feature_gat, xc.permute(0, 2, 1)), (m64.temporal_gat, xc)):
            if not layer.use_gatv2:
                e_dim = layer.lin.weight.shape[0]
                pv = layer.lin(v)
                a = layer.a.squeeze(1)
                bad |= _near_zero((pv @ a[:e_dim]).unsqueeze(2) + (pv @ a[e_dim:]).unsqueeze(1), rel)
            elif gatv2_pairs:
                d = v.shape[2]
                left = F.linear(v, layer.lin.weight[:, :d], layer.lin.bias)
                right = F.linear(v, layer.lin.weight[:, d:])
                bad |= _near_zero(left.unsqueeze(2) + right.unsqueeze(1), rel)
        hf = tp.feature_gat_stage(m64, xc, False, masks.get("feat"))
        ht = tp.temporal_gat_stage(m64, xc, False, masks.get("temp"))
        y = tp.gru_stage(m64, torch.cat([xc, hf, ht], dim=2), masks.get("gru"))
        layers = m64.forecasting_model.layers
        for i, lin in enumerate(layers[:-1]):
            pre = lin(y)
            bad |= _near_zero(pre, rel)
            y = F.relu(pre)
            if masks.get("fc") is not None:
                y = y * masks["fc"][i] * (1.0 / (1.0 - m64.forecasting_model.dropout.p))
    return bad


def edge_windows(b, edges=(), groups=(16, 32), row_edges=(), window=1):
    """The windows of a b-window call that sample_windows always takes, sorted: 0, 1, the last two, both sides of every window edge
    e (windows e - 1, e), of the last `groups`-window group edges, and of every ROW edge r of a (window, step)-row buffer with
    `window` steps per window -- the windows of rows r - 1 and r and, where the edge falls inside one window, the window before it
    too, so that a row dropped, duplicated or taken from the neighbouring slab always involves two adjacent sampled windows."""
    must = [0, 1, b - 2, b - 1]
    for e in list(edges) + [(b - 1) // gsz * gsz for gsz in groups]:
        must += [e - 1, e]
    for r in row_edges:
        lo, hi = (r - 1) // window, r // window
        must += [lo, hi] + ([lo - 1] if lo == hi else [])
    return sorted({w for w in must if 0 <= w < b})


def sample_windows(b, edges=(), n=32, seed=0, groups=(16, 32), row_edges=(), window=1, reject=None):
    """<= n window indices of a b-window call: edge_windows(...), then seeded random windows.  reject(windows) -> one bool per
    window: a random window it rejects is replaced by the next seeded one (the edge windows are never replaced)."""
    must = edge_windows(b, edges, groups, row_edges, window)[:n]
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(b, generator=g)
    if reject is None:
        rest = [w for w in perm[: n + len(must)].tolist() if w not in must][: n - len(must)]
        return sorted(must + rest)
    rest, at = [], 0
    while len(rest) < n - len(must) and at < b:
        cand = [w for w in perm[at:at + n].tolist() if w not in must]
        at += n
        if cand:
            rest += [w for w, bad in zip(cand, reject(cand)) if not bad]
    return sorted(must + rest[: n - len(must)])


def window_gate(ours, ref64, ref32_of, what=""):
    """Per window w of (k, ...) tensors, s_w = max |ref64_w|: pass when max |ours_w - ref64_w| <= 1e-6 + 1e-4 s_w; otherwise only
    when it is within the fp32 torch-op route's own distance from float64 for that window + 1e-6 + 1e-5 s_w (helpers.gate's rule).
    ref32_of(rows) evaluates the fp32 route for the window rows it is given.  Returns the worst err / (1e-6 + 1e-4 s_w)."""
    ours = ours.detach().cpu().double().flatten(1)
    ref = ref64.detach().cpu().double().flatten(1)
    assert ours.shape == ref.shape, (what, ours.shape, ref.shape)
    assert torch.isfinite(ours).all(), f"{what}: non-finite values"
    err, s = (ours - ref).abs().amax(1), ref.abs().amax(1)
    bound = WINDOW_ABS + WINDOW_REL * s
    over = (err > bound).nonzero().flatten().tolist()
    if over:
        ref32 = ref32_of(over).detach().cpu().double().flatten(1)
        noise = (ref32 - ref[over]).abs().amax(1)
        for j, r in enumerate(over):
            lim = noise[j].item() + WINDOW_ABS + WINDOW_NOISE_REL * s[r].item()
            assert err[r].item() <= lim, (f"{what}: row {r}: |ours - ref64| = {err[r].item():.3e} > fp32 route's {noise[j].item():.3e} "
                                          f"+ 1e-6 + 1e-5 * {s[r].item():.3e}")
    return (err / bound).max().item() if err.numel() else 0.0


def attribution_chunks(count, steps, units):
    """(u0, nu) of the chunks mtadgat_score_attribution walks: count * max(steps, 1) (index, step) units, index-major, `units` per
    chunk."""
    total = count * max(steps, 1)
    return [(u0, min(units, total - u0)) for u0 in range(0, total, units)]


def straddling_indices(count, steps, units):
    """Positions p whose step range [p m, (p + 1) m) (m = max(steps, 1)) crosses a chunk boundary of attribution_chunks."""
    m = max(steps, 1)
    return [p for p in range(count) if (p * m) // units != ((p + 1) * m - 1) // units]


# ---- which recurrence kernels a GPU call runs (tests that claim a kernel assert it) ----------------------------------------------------
def device_compute_units(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def call_routes(eng, n, compute_units):
    """(piece sizes, ["GRU 0 | ... | decoder 0 | ..." per piece]) of an inference call of n windows under the engine's current
    precision, chunk size and options: Engine.forward_plan and Engine.gru_route, each route spelled as tests/test_host_gru_route.py's
    `_describe` spells it, "+" joining a first kernel to its range-guard fallback."""
    from test_host_gru_route import _describe
    pieces = [p for _, p, _ in eng.forward_plan(n)["pieces"]]
    layers = [(0, l) for l in range(eng.cfg.gru_n_layers)] + [(1, l) for l in range(eng.cfg.recon_n_layers)]
    return pieces, [" | ".join("+".join(_describe(eng.gru_route(s, l, p, compute_units=compute_units))) for s, l in layers) for p in pieces]
