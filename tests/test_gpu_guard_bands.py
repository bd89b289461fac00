"""The inference calls of the model path stay inside the buffers they are handed, and read nothing outside their inputs: every row
below runs four times (tests/guard_rows.py) -- on allocator buffers, then with every buffer the Python layer hands the library carved
from a guard-banded arena (tests/arena.py: exact sizes, 256 KiB of pattern on both sides) under the NaN pattern, under the huge finite
pattern, and under the NaN pattern with every data buffer 4, 8 or 12 bytes past a 16-byte boundary (bfloat16 inputs: 2; workspaces
stay aligned, the ABI asks for that).  No guard may change and every result must equal the ordinary call's bit for bit.

Rows: every case of gru_route_cases.CASES (variant plain) under its mode, "gru_kernel", "lanes" and chunk, the route asserted before
each call as tests/test_gpu_gru_routes.py does; the five front-end cases of tests/test_gpu_front_route.py; the un-fused shapes of
gat_sign_cases; the stage entries at the shapes of tests/test_gpu_gemm_cores.py; bfloat16 windows; series calls with and without
explicit starts; the attention maps; series_losses, score_attribution and the dropout masks.  The last tests show that the harness can
fail: a guard that begins one element early catches the kernel's own last store, an input whose guard begins one element early
poisons exactly the last window, and the size and alignment refusals of the entry points launch nothing.

The training step's rows are in tests/test_gpu_guard_bands_train.py."""
import contextlib
import copy
import ctypes

import pytest
import torch

import _native
import arena
import gru_route_cases as rc
import test_gpu_front_route as fr
import test_host_gat_sign_cases as gat_host
import train_route_cases as tc
from guard_rows import four_calls, place, same_bits
from helpers import call_routes, device_compute_units
from test_gpu_gat_sign_order import LAYER_CODE
from test_host_gru_route_cases import base_model as gru_base_model, case_input

pytestmark = pytest.mark.gpu

KIND = {k: i for i, k in enumerate(_native.FRONT_KINDS)}
SOURCE = {k: i for i, k in enumerate(_native.FRONT_SOURCES)}
ERR_WORKSPACE = -5
_models = {}


@contextlib.contextmanager
def _options(eng, **options):
    try:
        for k, v in options.items():
            eng.set_option(k, v)
        yield
    finally:
        for k in options:
            eng.set_option(k, 0)


def _cached(key, make, device):
    if key not in _models:
        _models[key] = make().eval().to(device)
    return _models[key]


def _seeded(kw, seed=11):
    from mtad_gat import MTAD_GAT

    def make():
        torch.manual_seed(seed)
        m = MTAD_GAT(**kw)
        with torch.no_grad():
            m.feature_gat.bias.normal_()
            m.temporal_gat.bias.normal_()
        return m
    return make


def _gru_model(shape, device):
    return _cached(("gru", shape), lambda: copy.deepcopy(gru_base_model(shape)), device)


def _front_model(kw, device):
    return _cached(("front", tuple(sorted(kw.items()))), _seeded(kw), device)


def _conv_of(eng, kind, source, n):
    return _native.FRONT_CONVS[eng.front_route(KIND[kind], SOURCE[source], n)["conv"]]


def _rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


# ---- every recurrence route -------------------------------------------------------------------------------------------------------
def test_the_recurrence_rows_reach_every_ledger_entry():
    """Variant plain of every case runs below under the case's own mode, kernel option, lanes and chunk: the rows reach what the
    table reaches (tests/test_host_gru_route_cases.py holds the table to its ledger with the same function)."""
    got = rc.ledger_of(rc.CASES)
    assert {k: sorted(v) for k, v in got.items()} == {k: sorted(v) for k, v in rc.LEDGER.items()}


@pytest.mark.parametrize("c", rc.CASES, ids=[rc.case_id(c) for c in rc.CASES])
def test_recurrence_routes(c, gpu_device, monkeypatch):
    what = rc.case_id(c)
    model = _gru_model(c["shape"], gpu_device)
    model.precision = rc.MODES[c["mode"]]
    eng = model._sync_engine(gpu_device, bf16=c["mode"] == 1)
    keep_chunk = eng.chunk_windows()
    cu = device_compute_units(gpu_device)

    def before():
        pieces, routes = call_routes(eng, c["n"], cu)
        assert pieces == c["pieces"] and routes == c["routes"], (what, pieces, routes)
    try:
        eng.set_precision(c["mode"])
        eng.set_option("gru_kernel", c["gru_kernel"])
        eng.set_option("lanes", c["lanes"])
        if c["chunk"]:
            eng.set_chunk_windows(c["chunk"])
        four_calls(monkeypatch, gpu_device, [eng], {"x": case_input(c, "plain").to(gpu_device)},
                   lambda ins: dict(zip(("preds", "recons", "hend"), eng.forward(ins["x"], want_hend=True))), what, before=before)
    finally:
        eng.set_option("gru_kernel", 0)
        eng.set_option("lanes", 0)
        eng.set_chunk_windows(keep_chunk)
        eng.set_precision(2)
        model.precision = "auto"
        model._finish_weight_check()


# ---- the front end's routes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fr.CASES))
def test_front_routes(name, gpu_device, monkeypatch):
    """tests/test_gpu_front_route.py's five cases: the window forward; for shared_rows the series forward, the series ending with the
    last window's last row."""
    kw, options, n, series, conv, unfused = fr.CASES[name]
    model = _front_model(kw, gpu_device)
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    W, F = kw["window_size"], kw["n_features"]

    def before():
        r = eng.front_route(KIND["forward"], SOURCE["series_unit" if series else "windows"], n)
        assert _native.FRONT_CONVS[r["conv"]] == conv and fr._implied(r)[1] == unfused, (name, r)
    x = _rand(n + W - 1, F, seed=12) if series else _rand(n, W, F, seed=12)

    def call(ins):
        with torch.no_grad():
            p, r = model.forward_series(ins["x"]) if series else model(ins["x"])
        assert p.shape[0] == n
        return {"preds": p, "recons": r}
    with _options(eng, **options):
        four_calls(monkeypatch, gpu_device, [eng], {"x": x.to(gpu_device)}, call, name, before=before)


@pytest.mark.parametrize("shape", ["wide", "attend", "long_embedding"])
def test_unfused_attention_shapes(shape, gpu_device, monkeypatch):
    """gat_sign_cases' shapes whose layers go through memory: row GEMM + k_gat_wide, row GEMM + k_attend."""
    model, x, _ = gat_host.base_model(shape)
    model = _cached(("gat", shape), lambda: copy.deepcopy(model), gpu_device)
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()

    def before():
        r = eng.front_route(KIND["forward"], SOURCE["windows"], x.shape[0])
        assert (r["temp_kernel"], r["feat_kernel"]) == (LAYER_CODE[shape],) * 2, (shape, r)

    def call(ins):
        with torch.no_grad():
            return dict(zip(("preds", "recons"), model(ins["x"])))
    four_calls(monkeypatch, gpu_device, [eng], {"x": x.to(gpu_device)}, call, shape, before=before)


# ---- the stage entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [136, 134])
@pytest.mark.parametrize("option,build", [(1, "fp32"), (2, "x3")])
def test_stage_convolution(F, option, build, gpu_device, monkeypatch):
    """tests/test_gpu_gemm_cores.py's two convolution shapes (3 windows of 21 steps; F = 134 takes the scalar loader)."""
    kw = dict(n_features=F, window_size=21, out_dim=2, kernel_size=7, gru_hid_dim=8, forecast_hid_dim=8, recon_hid_dim=8)
    model = _front_model(kw, gpu_device)
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    x = torch.randn(3, 21, F, generator=torch.Generator().manual_seed(42)).to(gpu_device)

    def before():
        r = eng.front_route(KIND["conv"], SOURCE["windows"], 3)
        assert _native.FRONT_CONVS[r["conv"]] == "launch_conv" and _native.FRONT_BUILDS[r["conv_build"]] == build, r
    with _options(eng, conv_kernel=option):
        four_calls(monkeypatch, gpu_device, [eng], {"x": x}, lambda ins: {"y": eng.conv(ins["x"])}, f"conv F={F} {build}", before=before)


@pytest.mark.parametrize("hid", [41, 3], ids=["K41", "K3"])
@pytest.mark.parametrize("option,split", [(1, 0), (2, 1)])
def test_stage_heads(hid, option, split, gpu_device, monkeypatch):
    """tests/test_gpu_gemm_cores.py's heads shape: 401 windows of 41 steps, out_dim 130, K = 41 and K = 3 (the 4-byte loader)."""
    n, W = 401, 41
    kw = dict(n_features=6, window_size=W, out_dim=130, kernel_size=3, gru_hid_dim=35, forecast_hid_dim=33, recon_hid_dim=hid)
    model = _front_model(kw, gpu_device)
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    hend = (_rand(n, 35, seed=46) * 2 - 1).to(gpu_device)

    def before():
        assert eng.lib.mtadgat_rowgemm_split(eng.handle, 1, n * W, 0) == split
    with _options(eng, rowgemm_kernel=option):
        four_calls(monkeypatch, gpu_device, [eng], {"h_end": hend}, lambda ins: dict(zip(("preds", "recons"), eng.heads(ins["h_end"]))),
                   f"heads K={hid} split={split}", before=before)


def test_stage_attention_and_recurrence(gpu_device, monkeypatch):
    """Engine.gat (both layers) and Engine.gru once on the fused shape."""
    kw = fr.FUSED
    model = _front_model(kw, gpu_device)
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    n, W, F = 24, kw["window_size"], kw["n_features"]

    def before():
        r = eng.front_route(KIND["forward_unfused"], SOURCE["windows"], n)
        assert (r["temp_kernel"], r["feat_kernel"]) == (_native.FRONT_LAYERS.index("k_gat"),) * 2, r
    xc = _rand(n, W, F, seed=13).to(gpu_device)
    four_calls(monkeypatch, gpu_device, [eng], {"xc": xc}, lambda ins: {"feat": eng.gat(0, ins["xc"]), "temp": eng.gat(1, ins["xc"])},
               "gat stages", before=before)
    hcat = _rand(n, W, 3 * F, seed=14).to(gpu_device)

    def before_gru():
        assert call_routes(eng, n, device_compute_units(gpu_device)) == ([n], ["gru1 | gru1"])
    four_calls(monkeypatch, gpu_device, [eng], {"h_cat": hcat}, lambda ins: {"h_end": eng.gru(ins["h_cat"])}, "gru stage", before=before_gru)


# ---- bfloat16 windows -------------------------------------------------------------------------------------------------------------------
BF16_ROWS = {
    # name: (model, windows, options, the convolution that reads the bfloat16 elements)
    "fused_in_gath": ("front", 24, dict(conv_kernel=2, gat_kernel=3), "in_gath"),
    "fused_conv_win": ("front", 24, dict(conv_kernel=2, gat_kernel=3, conv_fused=1), "k_conv_win"),
    "L_in_gath": ("L", 4097, dict(), "in_gath"),
    "L_conv_win": ("L", 4097, dict(conv_fused=1), "k_conv_win"),
}


@pytest.mark.parametrize("name", list(BF16_ROWS))
def test_bfloat16_windows(name, gpu_device, monkeypatch):
    """mtadgat_forward_xbf16: k_gath / k_conv_win read the bfloat16 elements themselves; the skewed call starts them 2 bytes past a
    16-byte boundary."""
    which, n, options, conv = BF16_ROWS[name]
    model = _front_model(fr.FUSED, gpu_device) if which == "front" else _gru_model("L", gpu_device)
    model.precision = "fp32"
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    W, F = model.window_size, model.n_features
    xb = _rand(n, W, F, seed=15).to(gpu_device).to(torch.bfloat16)

    def before():
        assert _conv_of(eng, "forward", "windows_bf16", n) == conv
    try:
        with _options(eng, **options):
            four_calls(monkeypatch, gpu_device, [eng], {"x": xb}, lambda ins: dict(zip(("preds", "recons"), eng.forward(ins["x"]))), name,
                       before=before)
    finally:
        model.precision = "auto"


# ---- series calls -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["recons_last", "recons"])
def test_series_stride_one(full, gpu_device, monkeypatch):
    """4 097 stride-1 windows of shape L: the series ends with the last window's last row."""
    model = _gru_model("L", gpu_device)
    model.precision = "fp32"
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    n, W, F = 4097, model.window_size, model.n_features
    series = _rand(n + W - 1, F, seed=16).to(gpu_device)

    def before():
        assert _conv_of(eng, "forward", "series_unit", n) == "in_gath"
    try:
        four_calls(monkeypatch, gpu_device, [eng], {"series": series},
                   lambda ins: dict(zip(("preds", "recons", "last"), eng.forward_series(ins["series"], want_recons=full, want_last=True))),
                   f"series stride 1, full={full}", before=before)
    finally:
        model.precision = "auto"


@pytest.mark.parametrize("n", [45, 4097])
def test_series_explicit_starts(n, gpu_device, monkeypatch):
    """Explicit starts, guard-banded themselves, unsorted, with repeats, the first and the last possible window among them."""
    model = _gru_model("L", gpu_device)
    model.precision = "fp32"
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    W, F, rows = model.window_size, model.n_features, 700
    series = _rand(rows, F, seed=17).to(gpu_device)
    starts = torch.randint(0, rows - W + 1, (n,), generator=torch.Generator().manual_seed(18))
    starts[0], starts[n // 2], starts[-1], starts[1] = rows - W, 0, rows - W, starts[2]

    def before():
        assert _conv_of(eng, "forward", "series", n) == ("in_gath" if n > 4096 else "launch_conv")
    try:
        four_calls(monkeypatch, gpu_device, [eng], {"series": series, "starts": starts.to(gpu_device)},
                   lambda ins: dict(zip(("preds", "recons", "last"), eng.forward_series(ins["series"], starts=ins["starts"], want_last=True))),
                   f"series starts n={n}", before=before)
    finally:
        model.precision = "auto"


# ---- attention maps -------------------------------------------------------------------------------------------------------------------------
def _attention_models(device):
    return {"fused": (_front_model(fr.FUSED, device), 24, "k_gat"), "unfused": (_front_model(fr.UNFUSED, device), 8, "rowgemm+k_gat_wide"),
            "attend": (_cached(("gat", "attend"), lambda: copy.deepcopy(gat_host.base_model("attend")[0]), device), 3,
                       "rowgemm+k_attend")}


@pytest.mark.parametrize("reduce", [False, True], ids=["maps", "mean"])
@pytest.mark.parametrize("shape", ["fused", "unfused", "attend"])
def test_attention_maps(shape, reduce, gpu_device, monkeypatch):
    model, n, layer = _attention_models(gpu_device)[shape]
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    x = _rand(n, model.window_size, model.n_features, seed=19).to(gpu_device)

    def before():
        r = eng.front_route(KIND["attention"], SOURCE["windows"], n)
        assert (r["temp_kernel"], r["feat_kernel"]) == (_native.FRONT_LAYERS.index(layer),) * 2, (shape, r)
    four_calls(monkeypatch, gpu_device, [eng], {"x": x}, lambda ins: dict(zip(("att_feat", "att_temp"), eng.attention(ins["x"], reduce=reduce))),
               f"attention {shape} reduce={reduce}", before=before)


def test_attention_series(gpu_device, monkeypatch):
    model, n, _ = _attention_models(gpu_device)["fused"]
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    series = _rand(n + model.window_size - 1, model.n_features, seed=20).to(gpu_device)

    def before():
        r = eng.front_route(KIND["attention"], SOURCE["series_unit"], n)
        assert (_native.FRONT_CONVS[r["conv"]], r["temp_kernel"], r["feat_kernel"]) == ("launch_conv",) + (_native.FRONT_LAYERS.index("k_gat"),) * 2, r
    four_calls(monkeypatch, gpu_device, [eng], {"series": series},
               lambda ins: dict(zip(("att_feat", "att_temp"), eng.attention_series(ins["series"], reduce=True))), "attention_series",
               before=before)


# ---- losses, attribution, masks ------------------------------------------------------------------------------------------------------------
def test_series_losses(gpu_device, monkeypatch):
    """tests/test_gpu_losses.py's smallest model case (syn_v1_small, 150 windows), and the same with three picked columns."""
    from helpers import Case
    case = Case("syn_v1_small")
    model = _cached(("case", "syn_v1_small"), case.build_model, gpu_device)
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    W, F, out = case.kwargs["window_size"], case.kwargs["n_features"], case.kwargs["out_dim"]
    series = _rand(150 + W, F, seed=5).to(gpu_device)
    dims = torch.arange(out, dtype=torch.int32).flip(0).contiguous().to(gpu_device)

    def before():                                                    # one chunk of 150 stride-1 windows of the series
        assert eng.series_losses_chunk() >= 150
        assert call_routes(eng, 150, device_compute_units(gpu_device)) == ([150], ["split:fp32:xp | tile:fp32 | tile:fp32 | tile:fp32"])
        assert tc.describe_front(eng.front_route(KIND["forward"], SOURCE["series_unit"], 150)) == tc.F_GAT
    for name, d in (("all columns", None), ("dims", dims)):
        four_calls(monkeypatch, gpu_device, [eng], {"series": series, "dims": d},
                   lambda ins: dict(zip(("window_sse", "dim_sse"), eng.series_losses(ins["series"], dims=ins["dims"]))), f"series_losses {name}",
                   before=before)


@pytest.mark.parametrize("steps", [0, 8], ids=["gradient", "integrated"])
def test_score_attribution(steps, gpu_device, monkeypatch):
    """tests/test_gpu_attribution.py's smallest model (gat_v1: 9 features, 20 steps), indices 0, 4 and the last one possible."""
    from test_gpu_attribution import MODELS
    kw, dims, gamma, _ = MODELS["gat_v1"]
    model = _cached(("attr", "gat_v1"), _seeded(kw, seed=0), gpu_device)
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    W, F = kw["window_size"], kw["n_features"]
    series = _rand(W + 1 + 9, F, seed=1)
    inputs = {"series": series, "idx": torch.tensor([0, 4, 9], dtype=torch.int64), "dims": torch.tensor(dims, dtype=torch.int32),
              "dim_w": torch.tensor([1.0, 0.5, 2.0]), "baseline": series.mean(0) if steps else None}
    inputs = {k: (v.to(gpu_device) if v is not None else None) for k, v in inputs.items()}

    def before():                                                    # training forward + data backward of 2 windows per (index, step) unit
        for n in (2, 2 * 3 * max(steps, 1)):                         # (however the units are cut into chunks, the kernels are these)
            assert tc.describe_train(eng.train_route(n), "fused:v1") == "gru1>gru1_bwd | gru1>gru1_bwd | fc:row", n
            assert tc.describe_front(eng.front_route(KIND["train"], SOURCE["windows"], n)) == tc.F_GAT, n
    four_calls(monkeypatch, gpu_device, [eng], inputs,
               lambda ins: {"out": eng.score_attribution(ins["series"], ins["idx"], ins["dims"], ins["dim_w"], gamma, steps, ins["baseline"])},
               f"score_attribution steps={steps}", before=before)


def test_dropout_masks(gpu_device, monkeypatch):
    """Engine.dropout_masks at p = 0.2 on a model with stacked recurrence layers: the masks between the layers too."""
    from test_host_train_route_cases import base_model
    model = _cached(("train", "stacked"), lambda: copy.deepcopy(base_model("stacked")), gpu_device)
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()

    def call(ins):
        m = eng.dropout_masks(37, tc.P_DROP, 1234567, gpu_device, window0=5)
        assert set(m) == {"feat", "temp", "fc", "gru", "rec"}
        return {"feat": m["feat"], "temp": m["temp"], "fc0": m["fc"][0], "gru0": m["gru"][0], "rec0": m["rec"][0]}
    ref, _ = four_calls(monkeypatch, gpu_device, [eng], {}, call, "dropout_masks")      # (the mask kernels have no dispatch to assert)
    assert 0.7 < ref["temp"].mean().item() < 0.9


# ---- the harness can fail ---------------------------------------------------------------------------------------------------------------------
def _fused_call(device):
    model = _front_model(fr.FUSED, device)
    eng = model._sync_engine(device)
    model._finish_weight_check()
    x = _rand(24, model.window_size, model.n_features, seed=21).to(device)
    return model, eng, x


@pytest.mark.parametrize("out", ["preds", "recons"])
def test_a_guard_that_begins_one_element_early_catches_the_last_store(out, gpu_device, monkeypatch):
    """The library is not told the size of its outputs: the arena hands it one whose last element is already guard.  The kernel's own
    last store lands there -- inside the arena -- and must be reported as exactly that buffer, behind it, 4 bytes."""
    model, eng, x = _fused_call(gpu_device)
    ref = eng.forward(x)
    torch.cuda.synchronize()
    meter = arena.Meter(gpu_device)
    with meter.patched(monkeypatch, eng):
        eng.forward(x)
    ar = arena.Arena(gpu_device, arena.PATTERN_A, arena.capacity_for(meter.sizes + [x.numel() * 4]))
    ins = place(ar, {"x": x}, False)
    with ar.patched(monkeypatch, eng, rules={f"forward.{out}": dict(early=1)}):
        got = eng.forward(ins["x"])
    t = got[0] if out == "preds" else got[1]
    assert ar.check() == [dict(name=f"forward.{out}", side="behind", offset=t.numel() * 4 - 4, words=1)]
    assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1])


def test_an_input_whose_guard_begins_one_element_early_poisons_the_last_window(gpu_device, monkeypatch):
    """The last element of x is guard (the NaN pattern): the last window answers NaN, every other window is unchanged."""
    model, eng, x = _fused_call(gpu_device)
    ref = eng.forward(x)
    torch.cuda.synchronize()
    meter = arena.Meter(gpu_device)
    with meter.patched(monkeypatch, eng):
        eng.forward(x)
    ar = arena.Arena(gpu_device, arena.PATTERN_A, arena.capacity_for(meter.sizes + [x.numel() * 4]))
    xa = ar.take(x.shape, fill=x, early=1, name="x")
    with ar.patched(monkeypatch, eng):
        got = eng.forward(xa)
    assert ar.check() == []
    for o, r in zip(got, ref):
        assert bool(torch.isnan(o[-1]).all()), "the last window did not read the guard"
        assert same_bits(o[:-1], r[:-1])


REFUSALS = ("forward", "forward_series", "attention", "series_losses", "score_attribution", "forward_train", "backward", "backward_data")


@pytest.mark.parametrize("entry", REFUSALS)
def test_short_or_misaligned_scratch_is_refused_before_anything_launches(entry, gpu_device):
    """A workspace or tape 4 bytes short, or 4 bytes past a 16-byte boundary, is refused with MTADGAT_ERR_WORKSPACE by the checks at
    the top of each entry point (check_common and the aligned16 lines of csrc/mtadgat_capi.cpp), and the whole arena -- outputs and
    scratch included -- still holds its pattern."""
    from test_host_train_route_cases import base_model
    model = _cached(("train", "base"), lambda: copy.deepcopy(base_model("base")), gpu_device)
    eng = model._sync_engine(gpu_device)
    model._finish_weight_check()
    lib, h = eng.lib, eng.handle
    kw = tc.SHAPES["base"]
    b, W, F, od = 5, kw["window_size"], kw["n_features"], kw["out_dim"]
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(gpu_device).cuda_stream)
    need = {"forward": lib.mtadgat_workspace_bytes(h, b), "forward_series": lib.mtadgat_workspace_bytes(h, b),
            "attention": lib.mtadgat_attention_workspace_bytes(h, b, 0), "series_losses": lib.mtadgat_series_losses_workspace_bytes(h, b),
            "score_attribution": lib.mtadgat_score_attribution_workspace_bytes(h, b, 0), "forward_train": lib.mtadgat_tape_bytes(h, b),
            "backward": lib.mtadgat_backward_workspace_bytes(h, b), "backward_data": lib.mtadgat_backward_workspace_bytes(h, b)}[entry]
    tape_need = lib.mtadgat_tape_bytes(h, b)
    assert need > 16 and need % 4 == 0
    for scratch_short, scratch_skew, tape_short, tape_skew in ((4, 0, 0, 0), (0, 4, 0, 0), (0, 0, 4, 0), (0, 0, 0, 4)):
        if (tape_short or tape_skew) and entry not in ("backward", "backward_data"):
            continue
        ar = arena.Arena(gpu_device, arena.PATTERN_A, arena.capacity_for([need + 16, tape_need + 16] + [1 << 17] * 14))
        t = lambda name, *shape, **k: ar.take(shape, name=name, **k)                                                   # noqa: E731
        x = t("x", b, W, F, fill=0.5)
        series = t("series", b + W, F, fill=0.5)
        preds, recons, last = t("preds", b, od), t("recons", b, W, od), t("last", b, od)
        ws = ar.take(((need - scratch_short + 3) // 4,), skew=scratch_skew, name="scratch")
        tape = ar.take(((tape_need - tape_short + 3) // 4,), skew=tape_skew, name="tape")
        wsb, tpb = need - scratch_short, tape_need - tape_short
        p = lambda a: vp(a.data_ptr())                                                                                 # noqa: E731
        with torch.cuda.device(gpu_device):
            if entry == "forward":
                rc_ = lib.mtadgat_forward(h, p(x), b, p(preds), p(recons), None, p(ws), wsb, stream)
            elif entry == "forward_series":
                rc_ = lib.mtadgat_forward_series(h, p(series), b + W, None, 0, 1, b, p(preds), p(recons), p(last), p(ws), wsb, stream)
            elif entry == "attention":
                rc_ = lib.mtadgat_attention(h, p(x), b, p(t("att_f", b, F, F)), p(t("att_t", b, W, W)), p(ws), wsb, stream)
            elif entry == "series_losses":
                rc_ = lib.mtadgat_series_losses(h, p(series), b + W, None, 0, 1, b, None, p(ar.take((b, 2), torch.float64, name="wsse")),
                                                p(ar.take((2, od), torch.float64, name="dsse")), p(ws), wsb, stream)
            elif entry == "score_attribution":
                idx = ar.take((b,), torch.int64, fill=torch.arange(b, device=gpu_device), name="idx")
                dims = ar.take((od,), torch.int32, fill=torch.arange(od, dtype=torch.int32, device=gpu_device), name="dims")
                rc_ = lib.mtadgat_score_attribution(h, p(series), b + W, p(idx), b, p(dims), od, p(t("dim_w", od, fill=1.0)), 1.0, 0, None, 0,
                                                    p(t("out", b, W + 1, F)), p(ws), wsb, stream)
            elif entry == "forward_train":
                rc_ = lib.mtadgat_forward_train(h, p(x), b, 0, 0.0, 0, p(preds), p(recons), p(ws), wsb, stream)
            else:
                d_preds, d_recons = t("d_preds", b, od, fill=1.0), t("d_recons", b, W, od, fill=1.0)
                n_grads = eng.grad_layout()[1]
                out = t("grads", n_grads, fill=0.0) if entry == "backward" else t("dx", b, W, F)
                fn = lib.mtadgat_backward if entry == "backward" else lib.mtadgat_backward_data
                rc_ = fn(h, p(x), b, 0, 0.0, 0, p(d_preds), p(d_recons), p(tape), tpb, p(out), p(ws), wsb, stream)
        what = (entry, scratch_short, scratch_skew, tape_short, tape_skew)
        assert rc_ == ERR_WORKSPACE, (what, rc_, lib.mtadgat_last_error())
        assert ar.check(interiors=True) == [], what
        if entry == "backward":
            assert not bool(ar.buffer("grads").tensor.any()), what
