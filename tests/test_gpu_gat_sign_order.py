"""The GATv2 attention kernels where the sign-sorted column order degenerates (cases and specification: tests/gat_sign_cases.py;
their preconditions on the CPU, and the oracle references: tests/test_host_gat_sign_cases.py).  Every (shape, route) walks all sign
patterns of a = |a_init| * pattern -- one sign only, one column of a sign, the boundary on a tile edge, the c / d column in a
32-column part of its own, exact +0.0 / -0.0, more than 256 embedding columns -- on ONE handle: each pattern is written in place
into the GPU-resident parameters, packed by the device packer (k_gat_colorder, mtadgat_update_weights_device), observed, packed
again by the host packer (gat_column_order) and observed again.

Routes, taken from Engine.front_route and asserted: fused k_gat (gat_kernel = 1; precision fp32_strict and fp32), k_gath on the
compact order (gat_kernel = 3, conv_kernel = 2; on msl_like, the one shape that has it, with the convolution inside the temporal
workgroup and, conv_fused off, as k_conv_win), row GEMM + k_gat_wide, row GEMM + k_attend, the attention-maps call and the training
forward.  Observables, all through helpers.gate (1e-5, or the reference's own float32 rounding + 1e-5 against float64) against the
oracle: the stage entry point eng.gat on the oracle's xc, MTAD_GAT.attention_maps (rows sum to 1 within 1e-5), model(x) with the
GRU's final state, and eng.forward_train(x, 0, 0).  eng.gat and the maps are bit-identical across the two packers.  Gradients of
the HIP step (eval mode) against float64 autograd through _torchpath.forward on the CPU, gate of test_gpu_backward._grad_report.
The whole file runs once more in a child process with poisoned scratch.

Measured on an MI355X, largest |ours - ref64| over all patterns and both packers (the reference's own |fp32 - fp64| in brackets):
    route               layer outputs (eng.gat)   attention maps         model outputs (h_end, preds, recons)
    k_gat_strict        1.19e-07 (1.25e-07)       -                      4.49e-07 (3.23e-07)
    k_gat               1.19e-07 (1.25e-07)       -                      4.49e-07 (3.23e-07)
    k_gath              -                         -                      3.69e-07 (3.23e-07)
    k_gath_conv_win     -                         -                      3.69e-07 (3.23e-07)
    k_gat_wide          1.61e-07 (1.09e-07)       -                      1.58e-07 (1.28e-07)
    k_attend            1.29e-07 (8.98e-08)       -                      1.28e-06 (6.24e-07)
    maps (every shape)  -                         7.37e-07 (3.00e-07)    -
    train               -                         -                      9.41e-08 (5.60e-08)   (forward_train's preds, recons)
    alpha 0 / 1 / 1.5   6.94e-08 (6.25e-08)       4.98e-08 (7.13e-08)    1.16e-07 (6.91e-08)
    sequence            6.82e-08 (6.55e-08)       8.81e-08 (7.74e-08)    1.01e-07 (6.33e-08)
Largest gradient error over its bound 1e-5 + 1e-4 * scale: 0.002 on e2 and on small (every parameter, d a_k of the zero columns
included).  Nothing disagreed with the oracle, and eng.gat / the maps were bit-identical across the two packers for every pattern,
also under poisoned scratch.  The file discriminates: with the non-negative tile count of k_gat's inference loop off by one, the
sign of k_gath's mixed-tile steps off by one step, and k_gat_colorder's chunk carry of the non-negative group dropped (three
experiments, not kept), every k_gat / maps / train case, every k_gath case and every attend / long_embedding case failed, at
errors of 1.7e-5 (k_gath, msl_like predictions) to 1.6e-1 (long_embedding maps); wide, which none of the three touches, passed.
"""
import os
import subprocess
import sys

import pytest
import torch

import _native
import gat_sign_cases as gc
import test_host_gat_sign_cases as host           # the models, inputs and oracle references of the cases
from helpers import gate, model64

pytestmark = pytest.mark.gpu

FUSED, GATH, WIDE, ATTEND = (_native.FRONT_LAYERS.index(k)
                             for k in ("k_gat", "k_gath+k_gat", "rowgemm+k_gat_wide", "rowgemm+k_attend"))
KIND = {k: _native.FRONT_KINDS.index(k) for k in ("forward", "forward_unfused", "train", "attention")}
WINDOWS_SOURCE = _native.FRONT_SOURCES.index("windows")
LAYER_CODE = {"e2": FUSED, "small": FUSED, "msl_like": FUSED, "wide": WIDE, "attend": ATTEND, "long_embedding": WIDE}

# name: (precision, options, observables, front kind whose layer codes are asserted, layer code or None = the shape's own)
ROUTES = {
    "k_gat_strict": ("fp32_strict", dict(gat_kernel=1), ("gat", "model"), "forward", FUSED),
    "k_gat": ("fp32", dict(gat_kernel=1), ("gat", "model"), "forward", FUSED),
    # k_gath: the convolution runs inside the temporal workgroup where that exists (msl_like: 97 time steps or more), as k_conv_win
    # elsewhere; k_gath_conv_win turns the fused convolution off, which changes the route on msl_like only
    "k_gath": ("fp32", dict(gat_kernel=3, conv_kernel=2), ("model",), "forward", GATH),
    "k_gath_conv_win": ("fp32", dict(gat_kernel=3, conv_kernel=2, conv_fused=1), ("model",), "forward", GATH),
    "k_gat_wide": ("fp32", dict(), ("gat", "model"), "forward", WIDE),
    "k_attend": ("fp32", dict(), ("gat", "model"), "forward", ATTEND),
    "maps": ("fp32", dict(), ("maps",), "attention", None),
    "train": ("fp32", dict(), ("train",), "train", None),
}
TABLE = ([(s, r) for s in ("e2", "small", "msl_like") for r in ("k_gat_strict", "k_gat", "k_gath", "maps")]
         + [("msl_like", "k_gath_conv_win"), ("e2", "train"), ("small", "train"), ("wide", "k_gat_wide"), ("wide", "maps"), ("wide", "train"),
            ("attend", "k_attend"), ("attend", "maps"), ("long_embedding", "k_gat_wide"), ("long_embedding", "maps")])

FIGURES = {}        # route -> kind -> [largest |ours - ref64|, largest |ref32 - ref64|]


def _gate(route, kind, ours, ref32, ref64, what):
    ours = ours.detach().cpu()
    assert ours.shape == ref32.shape and torch.isfinite(ours).all(), what
    fig = FIGURES.setdefault(route, {}).setdefault(kind, [0.0, 0.0])
    fig[0] = max(fig[0], (ours.double() - ref64).abs().max().item())
    fig[1] = max(fig[1], (ref32.double() - ref64).abs().max().item())
    gate(ours, ref32, ref64, what=what)


def _report(route):
    for kind, (d, noise) in sorted(FIGURES.get(route, {}).items()):
        print(f"  {route:18s} {kind:8s} |ours - ref64| <= {d:.2e}   (|ref32 - ref64| <= {noise:.2e})")


def _assert_route(eng, shape, route, n):
    """The dispatch gives this (shape, route) the kernels its name says: a change of the route cannot silently empty the test."""
    precision, options, observe, kind, code = ROUTES[route]
    code = LAYER_CODE[shape] if code is None else code
    r = eng.front_route(KIND[kind], WINDOWS_SOURCE, n)
    assert (r["temp_kernel"], r["feat_kernel"]) == (code, code), (shape, route, r)
    if "gat" in observe:        # the stage entry point: the un-fused call kind
        ru = eng.front_route(KIND["forward_unfused"], WINDOWS_SOURCE, n)
        assert (ru["temp_kernel"], ru["feat_kernel"]) == (code, code), (shape, route, ru)
    if code == GATH:
        conv = _native.FRONT_CONVS[r["conv"]]
        if options.get("conv_fused") == 1:
            assert conv == "k_conv_win", r
        else:                   # (the convolution inside k_gath needs the temporal layer's eight-wave workgroup: msl_like has it)
            assert conv == ("in_gath" if shape == "msl_like" else "k_conv_win"), r
        assert r["temp_fp16"] == 1 and r["feat_fp16"] == 1, r


def _observe(model, eng, observe, x, xc):
    out = {}
    with torch.no_grad():
        if "gat" in observe:
            out["hf"], out["ht"] = eng.gat(0, xc), eng.gat(1, xc)
        if "maps" in observe:
            out["af"], out["at"] = model.attention_maps(x)
        if "model" in observe:
            out["preds"], out["recons"] = model(x)
            out["hend"] = eng.forward(x, want_hend=True)[2]     # the recurrence's final state: the observable next to the layers
        if "train" in observe:
            out["preds"], out["recons"], _ = eng.forward_train(x, 0.0, 0)
    return out


def _check(route, out, ref, what):
    r32, r64, l64 = ref[32], ref[64], ref["l64"]
    for k in ("hf", "ht"):
        if k in out:
            _gate(route, "layers", out[k], r32[k], l64[k], f"{what} {k}")
    for k in ("af", "at"):
        if k in out:
            _gate(route, "maps", out[k], r32[k], r64[k], f"{what} {k}")
            assert (out[k].double().sum(-1) - 1).abs().max().item() <= 1e-5, f"{what} {k}: rows do not sum to 1"
    for k in ("hend", "preds", "recons"):
        if k in out:
            _gate(route, "outputs", out[k], r32[k], r64[k], f"{what} {k}")


def _packer_difference(eng, model, dev):
    """Where the device-packed image differs from the host-packed one (float offsets outside the derived regions), for the message
    of a failed bit-identity check."""
    sd = model.state_dict()
    assert eng.update_weights_device(sd, dev)
    img_dev = eng.read_packed(dev)
    eng.load_weights(sd, dev, allow_device_pack=False)
    img_host = eng.read_packed(dev)
    mism = img_dev.view(torch.int32) != img_host.view(torch.int32)
    for off, n in eng.derived_regions():
        mism[off:off + n] = False
    idx = mism.nonzero().flatten()
    return f"{idx.numel()} words differ, first at {idx[:8].tolist()}: device {img_dev[idx[:8]].tolist()} host {img_host[idx[:8]].tolist()}"


def _repack_on_device(model, dev):
    """The engine after an in-place parameter change: the next call re-packs on the device (update_weights_device)."""
    eng = model._sync_engine(dev)
    assert eng.update_weights_device(model.state_dict(), dev), "the library declined the device-side re-pack"
    return eng


def _set_options(eng, options, reset=False):
    for key, v in options.items():
        eng.set_option(key, 0 if reset else v)


def _run_route(shape, route, dev):
    precision, options, observe, kind, code = ROUTES[route]
    model, x, mags = host.new_model(shape)
    model = model.to(dev)
    model.precision = precision
    xd = x.to(dev)
    eng = model._sync_engine(dev)                           # first load: the host packer
    try:
        _set_options(eng, options)
        _assert_route(eng, shape, route, x.shape[0])
        for pattern in gc.patterns_of(shape):
            ref = host.reference(shape, pattern)
            xc = ref[32]["xc"].contiguous().to(dev)
            host.apply_pattern(model, mags, pattern)          # in place, on the GPU
            eng = _repack_on_device(model, dev)
            dev_out = _observe(model, eng, observe, xd, xc)
            _check(route, dev_out, ref, f"{shape}/{route}/{pattern} (device packer)")
            eng.load_weights(model.state_dict(), dev, allow_device_pack=False)
            host_out = _observe(model, eng, observe, xd, xc)
            _check(route, host_out, ref, f"{shape}/{route}/{pattern} (host packer)")
            for k in ("hf", "ht", "af", "at"):              # the attention regions of the image are bit-identical on both paths
                if k in dev_out and not torch.equal(dev_out[k], host_out[k]):
                    raise AssertionError(f"{shape}/{route}/{pattern} {k}: the two packers disagree by "
                                         f"{(dev_out[k] - host_out[k]).abs().max().item():.3e}; {_packer_difference(eng, model, dev)}")
    finally:
        _set_options(eng, options, reset=True)
    print(f"{shape}/{route}: {len(gc.patterns_of(shape))} patterns, both packers")
    _report(route)


@pytest.mark.parametrize("shape,route", TABLE, ids=[f"{s}-{r}" for s, r in TABLE])
def test_sign_patterns(shape, route, gpu_device):
    _run_route(shape, route, gpu_device)


# ---- alpha = 0 / 1 / 1.5: no LeakyReLU slope, every a' a signed zero, the sign sense reversed ----------------------------------
K_GATH = dict(gat_kernel=3, conv_kernel=2)


def _run_alpha(alpha, dev):
    shape, pattern = gc.ALPHA_CASE
    model, x, mags = host.new_model(shape, alpha)
    model = model.to(dev)
    model.precision = "fp32"
    ref = host.reference(shape, pattern, alpha)             # (the library takes all three values: test_host_gat_sign_cases.py)
    xd, xc = x.to(dev), ref[32]["xc"].contiguous().to(dev)
    host.apply_pattern(model, mags, pattern)
    eng = _repack_on_device(model, dev)
    what = f"alpha={alpha}"
    try:
        _set_options(eng, dict(gat_kernel=1))
        _check(f"alpha {alpha}", _observe(model, eng, ("gat", "maps", "model", "train"), xd, xc), ref, what + " (k_gat)")
        _set_options(eng, K_GATH)
        _assert_route(eng, shape, "k_gath", x.shape[0])
        _check(f"alpha {alpha}", _observe(model, eng, ("model",), xd, xc), ref, what + " (k_gath)")
        eng.load_weights(model.state_dict(), dev, allow_device_pack=False)
        _check(f"alpha {alpha}", _observe(model, eng, ("model",), xd, xc), ref, what + " (k_gath, host packer)")
        _set_options(eng, dict(gat_kernel=1))
        _check(f"alpha {alpha}", _observe(model, eng, ("gat", "maps", "model"), xd, xc), ref, what + " (k_gat, host packer)")
    finally:
        _set_options(eng, K_GATH, reset=True)
    _report(f"alpha {alpha}")


@pytest.mark.parametrize("alpha", gc.ALPHAS)
def test_alpha_edges(alpha, gpu_device):
    _run_alpha(alpha, gpu_device)


# ---- one handle through a sequence of orders: a stale `ord`, or stale pads of the previous order, shows up here -----------------
def _run_sequence(dev):
    shape = "small"
    model, x, mags = host.new_model(shape)
    model = model.to(dev)
    model.precision = "fp32"
    xd = x.to(dev)
    eng = model._sync_engine(dev)
    try:
        for pattern in gc.SEQUENCE:
            ref = host.reference(shape, pattern)
            xc = ref[32]["xc"].contiguous().to(dev)
            host.apply_pattern(model, mags, pattern)
            eng = _repack_on_device(model, dev)
            _set_options(eng, K_GATH, reset=True)
            _set_options(eng, dict(gat_kernel=1))
            _check("sequence", _observe(model, eng, ("gat", "maps", "model", "train"), xd, xc), ref, f"sequence/{pattern} (k_gat)")
            _set_options(eng, K_GATH)
            _assert_route(eng, shape, "k_gath", x.shape[0])
            _check("sequence", _observe(model, eng, ("model",), xd, xc), ref, f"sequence/{pattern} (k_gath)")
    finally:
        _set_options(eng, K_GATH, reset=True)
    _report("sequence")


def test_sequence_of_orders_on_one_handle(gpu_device):
    _run_sequence(gpu_device)


# ---- gradients ------------------------------------------------------------------------------------------------------------------
def _run_gradients(shape, dev):
    """The HIP step in eval mode against autograd through _torchpath.forward on a float64 copy on the CPU (test_gpu_fuzz.py: stock
    GPU ops are no safe checker).  d a_k of a column with a_k == 0 is as well defined as any other: d e / d a_k does not depend on
    a."""
    import _torchpath
    from test_gpu_backward import _grad_report, _loss
    x, y = host.grad_inputs(shape)
    xd, yd = x.to(dev), y.to(dev)
    model, _, mags = host.new_model(shape)
    model = model.to(dev).eval()
    worst = 0.0
    for pattern in gc.GRAD_PATTERNS:
        host.apply_pattern(model, mags, pattern)
        m64 = model64(model)
        pr64, rc64 = _torchpath.forward(m64, x.double(), None)
        _loss(pr64, rc64, x.double(), y.double()).backward()
        ref = {n: p.grad.to(dev) for n, p in m64.named_parameters()}
        for p in model.parameters():
            p.grad = None
        pr, rc = model(xd)
        assert model.grad_path == "hip", model.grad_path
        assert (pr.detach().cpu() - pr64.detach()).abs().max().item() <= 1e-5 and (rc.detach().cpu() - rc64.detach()).abs().max().item() <= 1e-5
        _loss(pr, rc, xd, yd).backward()
        rows, bad = _grad_report(model, ref)
        assert not bad, f"{shape}/{pattern}:\n" + "\n".join(bad)
        for n, p in model.named_parameters():
            d, s = (p.grad - ref[n]).abs().max().item(), ref[n].abs().max().item()
            worst = max(worst, d / (1e-5 + 1e-4 * s))
        has_zero = bool((model.feature_gat.a == 0).any() or (model.temporal_gat.a == 0).any())
        assert has_zero == (pattern in ("zeros", "all_zero"))
    FIGURES.setdefault("gradients", {})[shape] = [worst, 0.0]
    print(f"{shape}: largest gradient error / (1e-5 + 1e-4 * scale) = {worst:.3f}")


@pytest.mark.parametrize("shape", gc.GRAD_SHAPES)
def test_gradients_at_degenerate_orders(shape, gpu_device):
    _run_gradients(shape, gpu_device)


# ---- the same under poisoned scratch --------------------------------------------------------------------------------------------
def run_all(dev):
    for shape, route in TABLE:
        _run_route(shape, route, dev)
    for alpha in gc.ALPHAS:
        _run_alpha(alpha, dev)
    _run_sequence(dev)
    for shape in gc.GRAD_SHAPES:
        _run_gradients(shape, dev)


def test_poisoned_scratch(tmp_path, gpu_device):
    """Every check of this file in a fresh process whose scratch buffers and outputs start out as 7777.0 instead of a new allocation's
    zeros (MTADGAT_POISON_SCRATCH, _native.py): a part without pair tiles that reads a c / d column nobody wrote cannot hide.  The
    child is handed the references this process has computed."""
    refs = os.path.join(str(tmp_path), "refs.pt")
    torch.save(host._REFS, refs)
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys, torch\n"
        f"sys.path[:0] = [{here!r}, {os.path.join(os.path.dirname(here), 'mtad-gat-pytorch_amd')!r}, {os.path.dirname(here)!r}]\n"
        "import test_host_gat_sign_cases as host\n"
        "import test_gpu_gat_sign_order as t\n"
        f"host._REFS.update(torch.load({refs!r}, weights_only=False))\n"
        "t.run_all(torch.device('cuda:0'))\n"
        "print('poisoned run ok')\n")
    env = dict(os.environ, MTADGAT_POISON_SCRATCH="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "poisoned run ok" in out.stdout, out.stdout[-3000:] + out.stderr[-4000:]
