"""Preconditions of tests/test_gpu_gru_routes.py, checked on the CPU: every case of tests/gru_route_cases.py gets the pieces and the
recurrence routes its hand-written strings say (mtadgat_forward_plan / mtadgat_gru_route on 256 compute units), the table reaches every
(layer kind, route) pair of its ledger, the float32 oracle stays inside its cap against the float64 oracle on the picked windows of
every run, and the GPU test's comparison raises on two altered truths.  No GPU needed."""
import copy
import ctypes

import pytest
import torch

import gru_route_cases as rc
from test_host_gru_route import _create, _describe

# ---- the models, inputs and oracle references of the runs (CPU), built once; the GPU file imports them -----------------------------
_MODELS, _INPUTS, _REFS = {}, {}, {}
RECURRENCES = ("gru.gru.", "recon_model.decoder.rnn.")


def base_model(shape):
    """The model of a shape on the CPU in eval mode, seeded, both attention biases drawn from a normal distribution.  Cached: callers
    deep-copy it."""
    from mtad_gat import MTAD_GAT
    if shape not in _MODELS:
        torch.manual_seed(rc.MODEL_SEED)
        model = MTAD_GAT(**rc.SHAPES[shape]).eval()
        with torch.no_grad():
            model.feature_gat.bias.normal_()
            model.temporal_gat.bias.normal_()
        _MODELS[shape] = model
    return _MODELS[shape]


def new_model(shape, variant):
    """A fresh copy of the shape's model with the variant's weights (gru_route_cases: saturate, carry)."""
    model = copy.deepcopy(base_model(shape))
    with torch.no_grad():
        for name, p in model.named_parameters():
            if not name.startswith(RECURRENCES):
                continue
            if variant == "saturate" and ".weight_" in name:
                p.mul_(rc.SATURATE_FACTOR)
            if variant == "carry" and ".bias_ih_" in name:
                H = p.shape[0] // 3
                p[H:2 * H] += rc.CARRY_SHIFT                     # gate order r | z | n
    return model


def case_input(c, variant):
    """x (n, W, F) ~ U[0, 1) under the fixed seed; spike: window n // 2 times 2^17.  Cached per (n, W, F): do not modify."""
    kw = rc.SHAPES[c["shape"]]
    key = (c["n"], kw["window_size"], kw["n_features"], variant == "spike")
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(rc.X_SEED)
        x = torch.rand(c["n"], kw["window_size"], kw["n_features"], generator=g)
        if variant == "spike":
            x[rc.spike_window(c)] *= rc.SPIKE_SCALE
        _INPUTS[key] = x
    return _INPUTS[key]


def oracle_outputs(sd, x, dtype):
    """{"h_end", "preds", "recons"} of oracle.forward on the windows x, computed in dtype."""
    from oracle import mtad_gat_oracle as oracle
    with torch.no_grad():
        p, r, st = oracle.forward(x.to(dtype), {k: v.detach().cpu() for k, v in sd.items()}, alpha=0.2, return_stages=True)
    return {"h_end": st["h_end"], "preds": p, "recons": r}


def reference(c, variant):
    """The oracle of a run on its picked windows: {"picks", "x" (the picked windows), "sd", 32: ..., 64: ...}, each of 32 / 64 a dict
    of h_end / preds / recons in float32 / float64, and "conv_max": the largest convolution output of the whole call and of its
    ordinary windows (float64).  Computed once and left unchanged."""
    from oracle import mtad_gat_oracle as oracle
    key = (rc.case_id(c), variant)
    if key not in _REFS:
        model = new_model(c["shape"], variant)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        x = case_input(c, variant)
        picks = rc.picks(c)
        xp = x[picks]
        with torch.no_grad():
            xc = oracle.conv_layer(x.double(), sd["conv.conv.weight"].double(), sd["conv.conv.bias"].double()).flatten(1).amax(1)
        ordinary = torch.ones(c["n"], dtype=torch.bool)
        if variant == "spike":
            ordinary[rc.spike_window(c)] = False
        _REFS[key] = {"picks": picks, "x": xp, "sd": sd, 32: oracle_outputs(sd, xp, torch.float32), 64: oracle_outputs(sd, xp, torch.float64),
                      "conv_max": (xc.max().item(), xc[ordinary].max().item())}
    return _REFS[key]


def ordinary_rows(c, variant, picks):
    """bool per picked window: not the spiked one."""
    return torch.tensor([not (variant == "spike" and w == rc.spike_window(c)) for w in picks])


def route_gate(ours, ref32, ref64, mode, rows=None, what=""):
    """The GPU test's comparison.  Per output (h_end, preds, recons) and per picked window w:
        max |ours - ref64|(w) <= max |ref32 - ref64|(w) + tol,
    tol = 2e-6 * max(1, |ref64|max) in the fp32 modes (0, 2), 2e-2 in the bf16 mode (1).  rows: bool per window, the ones held (all by
    default); every window must be finite.  Returns {output: largest |ours - ref64| over the held windows}."""
    worst = {}
    for name in ("h_end", "preds", "recons"):
        o = ours[name].detach().cpu().double().flatten(1)
        r64, r32 = ref64[name].double().flatten(1), ref32[name].double().flatten(1)
        assert o.shape == r64.shape, (what, name, tuple(o.shape), tuple(r64.shape))
        assert torch.isfinite(o).all(), f"{what}: {name}: non-finite values"
        keep = torch.ones(o.shape[0], dtype=torch.bool) if rows is None else rows
        tol = rc.BF16_TOL if mode == 1 else rc.FP32_REL_TOL * max(1.0, r64[keep].abs().max().item())
        err, noise = (o - r64).abs().amax(1), (r32 - r64).abs().amax(1)
        bad = (keep & (err > noise + tol)).nonzero().flatten().tolist()
        assert not bad, (f"{what}: {name}: picked rows {bad[:8]}: |ours - ref64| = {err[bad].max().item():.3e} > "
                         f"|ref32 - ref64| {noise[bad].max().item():.3e} + {tol:.3e}")
        worst[name] = err[keep].max().item()
    return worst


# ---- library queries ---------------------------------------------------------------------------------------------------------------
def _answers(lib, h, c):
    """(piece sizes, [route string per layer] per piece) the library gives a case on rc.CU compute units."""
    import _native
    assert lib.mtadgat_set_precision(h, c["mode"]) == 0
    assert lib.mtadgat_set_option(h, b"gru_kernel", c["gru_kernel"]) == 0 and lib.mtadgat_set_option(h, b"lanes", c["lanes"]) == 0
    if c["chunk"]:
        assert lib.mtadgat_set_chunk_windows(h, c["chunk"]) == 0
    cap = 5 + 3 * 64
    buf = (ctypes.c_int64 * cap)()
    got = lib.mtadgat_forward_plan(h, c["n"], buf, cap)
    assert got >= 8 and got == 5 + 3 * buf[0], (rc.case_id(c), got, lib.mtadgat_last_error())
    pieces = [int(buf[i + 1]) for i in range(5, got, 3)]
    assert [int(buf[i]) for i in range(5, got, 3)] == [sum(pieces[:k]) for k in range(len(pieces))]
    lg, ld = rc.layers_of(c)
    routes = []
    for n in pieces:
        per_layer = []
        for stack, layer in [(0, l) for l in range(lg)] + [(1, l) for l in range(ld)]:
            out = (ctypes.c_int * 8)(*([-7] * 8))
            assert lib.mtadgat_gru_route(h, stack, layer, n, 0, rc.CU, out) == 0, lib.mtadgat_last_error()
            per_layer.append("+".join(_describe(dict(zip(_native.GRU_ROUTE_FIELDS, out)))))
        routes.append(per_layer)
    return pieces, routes


# ---- the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(rc.SHAPES))
def test_plans_and_routes_equal_the_hand_written_table(shape):
    cases = [c for c in rc.CASES if c["shape"] == shape]
    assert cases, shape
    for c in cases:
        lib, _, h = _create(rc.SHAPES[shape])                    # a fresh handle per case: the library's default chunk
        try:
            pieces, routes = _answers(lib, h, c)
        finally:
            lib.mtadgat_destroy(h)
        assert pieces == c["pieces"] and sum(pieces) == c["n"], (rc.case_id(c), pieces)
        assert routes == rc.piece_routes(c), (rc.case_id(c), routes)


def test_the_table_is_well_formed():
    assert len(set(rc.RUN_IDS)) == len(rc.RUN_IDS) and len(set(map(rc.case_id, rc.CASES))) == len(rc.CASES)
    for c in rc.CASES:
        assert c["mode"] in rc.MODES and set(c["variants"]) <= {"plain", "spike", "saturate", "carry"} and "plain" in c["variants"]
        assert len(c["pieces"]) == len(c["routes"])
        # the range guard only exists in the split-operand arithmetic: both of its sides are run wherever it can act
        assert ("spike" in c["variants"]) == rc.needs_spike(c), rc.case_id(c)
        if "spike" in c["variants"]:                              # the spiked window lies in a piece whose layer 0 reads the range
            at = 0
            for n, r in zip(c["pieces"], rc.piece_routes(c)):
                if at <= rc.spike_window(c) < at + n:
                    assert "+" in r[0] or r[0].startswith("tile:x3"), rc.case_id(c)
                at += n
        if "saturate" in c["variants"]:
            assert rc.SHAPES[c["shape"]]["window_size"] <= 8, rc.case_id(c)
        p = rc.picks(c)
        assert p == sorted(set(p)) and 0 <= p[0] and p[-1] == c["n"] - 1, rc.case_id(c)
        at = 0
        for n in c["pieces"]:                                     # both sides of every piece boundary, the ragged last group
            lg = (n - 1) // 32 * 32
            assert {at, at + n - 1, at + lg, at + max(lg - 1, 0)} <= set(p), rc.case_id(c)
            at += n


def test_the_sizes_are_ragged_as_the_table_means_them():
    groups = lambda n: (n + 31) // 32
    assert 45 == 32 + 13 and 129 == 128 + 1 and 4127 == 4096 + 31
    for n in (2561, 10273, 16417, 65505):
        assert n % 32 == 1                                       # the last 32-window group holds one window
    assert groups(65540) == 2049 and 2049 % 2 == 1               # two groups per wave: the last wave's second group is past the batch
    assert groups(65505) == 8 * rc.CU and groups(65504) < 8 * rc.CU                # the first size with two groups per wave
    assert groups(10273) > 5 * rc.CU // 4                        # more than 1.25 groups per compute unit: the tile-major kernel takes split operands


def test_ledger_every_route_is_still_reached():
    got = rc.ledger_of(rc.CASES)
    missing = {(k, r) for k, want in rc.LEDGER.items() for r in want if r not in got[k]}
    assert not missing, f"no case reaches {sorted(missing)}"
    # both sides of the range guard for every guarded / split-operand layer-0 route of the ledger
    spiked = rc.ledger_of([c for c in rc.CASES if "spike" in c["variants"]])["gru0"]
    assert {r for r in rc.LEDGER["gru0"] if "+" in r or r.startswith("tile:x3")} <= spiked
    # the clamped gate functions on each kernel
    for variant in ("saturate", "carry"):
        seen = set()
        for c in rc.CASES:
            if variant in c["variants"]:
                seen |= {s.split(":")[0] for routes in rc.piece_routes(c) for r in routes for s in r.split("+")}
        assert seen >= {"gru1", "gru16", "split", "splitx3", "cm", "tile"}, (variant, seen)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "spike", "saturate", "carry"])
def test_float32_oracle_stays_inside_its_cap(variant):
    """On the picked windows of every run the float32 oracle is within 1e-5 (saturate: 5e-6) of the float64 oracle -- the spiked window
    excepted --, so the noise term of the GPU gate never opens it beyond the project's own fp32 gate; and the recorded convolution
    range is on the side of 2^15 the variant means."""
    runs = [c for c in rc.CASES if variant in c["variants"]]
    assert runs
    worst = 0.0
    for c in runs:
        ref = reference(c, variant)
        rows = ordinary_rows(c, variant, ref["picks"])
        assert rows.sum() >= len(ref["picks"]) - 1
        for name in ("h_end", "preds", "recons"):
            d = (ref[32][name].double() - ref[64][name]).flatten(1).abs().amax(1)[rows].max().item()
            worst = max(worst, d)
            assert d <= (rc.SATURATE_CAP if variant == "saturate" else rc.REF_CAP), (rc.case_id(c, variant), name, d)
        whole, ordinary = ref["conv_max"]
        assert ordinary < rc.RANGE_EDGE and (whole >= rc.RANGE_EDGE) == (variant == "spike"), (rc.case_id(c, variant), whole, ordinary)
    print(f"{variant}: float32 oracle against float64, worst picked window {worst:.2e}")


def test_saturate_and_carry_reach_the_gates_ends():
    """The variants do to the first GRU layer's gate arguments what they are meant to: saturate widens them well beyond the plain
    model's (the factor acts on the matrices, not on the biases), carry holds the update gate's above 3 (z > 0.95) at every step.
    (The clamps of gate_sigmoid / gate_tanh themselves, +-60 / +-30, are reached only by the spiked window, which must stay finite.)"""
    import torch.nn.functional as F
    from oracle import mtad_gat_oracle as oracle
    c = next(c for c in rc.CASES if "saturate" in c["variants"] and c["n"] > 1000)
    widest = {}
    for variant in ("plain", "saturate", "carry"):
        ref = reference(c, variant)
        sd = {k: v.double() for k, v in ref["sd"].items()}
        with torch.no_grad():
            _, _, st = oracle.forward(ref["x"].double(), sd, return_stages=True)
            gx = F.linear(st["h_cat"], sd["gru.gru.weight_ih_l0"], sd["gru.gru.bias_ih_l0"])
        H = gx.shape[2] // 3
        widest[variant] = gx.abs().max().item()
        if variant == "carry":
            assert gx[:, :, H:2 * H].min().item() > 3.0           # (the state's part of the argument is small: |h| stays small)
    assert widest["saturate"] > 0.5 * rc.SATURATE_FACTOR * widest["plain"], widest


# ---- the gate can fail ----------------------------------------------------------------------------------------------------------------
def _gate_case(variant):
    """plain: the first case of shape A beyond 1000 windows; carry: the first such case of shape L, where the carried state has 100
    steps to build up (gru_route_cases: after 8 steps it is too small for the recurrent product to matter)."""
    shape = "L" if variant == "carry" else "A"
    c = next(c for c in rc.CASES if c["shape"] == shape and variant in c["variants"] and c["n"] > 1000)
    ref = reference(c, variant)
    route_gate(ref[64], ref[32], ref[64], c["mode"], what="the truth itself")        # passes
    route_gate(ref[32], ref[32], ref[64], c["mode"], what="the float32 oracle")      # passes: that is what the noise term is for
    return c, ref


@pytest.mark.parametrize("variant", ["plain", "carry"])
def test_the_gate_raises_on_a_dropped_low_piece(variant):
    """A float64 replay in which weight_hh_l0 (of the GRU stack and of the decoder) is rounded to one fp16 value each -- a dropped low
    piece of the split operands -- must not pass as the kernels' result; rounding the GRU stack's matrix alone is seen in h_end.
    Measured: plain (W = 8) moves h_end by 2.6e-5, preds by 4.4e-6, recons by 5.3e-6; carry on shape L (W = 100) moves h_end by
    4.5e-6 in every window, against 2.9e-7 of float32 noise + 2e-6.  (carry on the W = 8 shapes: 5.6e-8, under the float32 oracle's
    own 1.1e-7 -- those runs hold the gates' ends, not the low piece.)"""
    c, ref = _gate_case(variant)
    sd = {k: (v.half().to(v.dtype) if k.endswith("weight_hh_l0") else v) for k, v in ref["sd"].items()}
    assert sum(k.endswith("weight_hh_l0") for k in sd) == 2
    one_piece = oracle_outputs(sd, ref["x"], torch.float64)
    for name in one_piece:
        print(f"{variant}: fp16 weight_hh_l0 moves {name} by {(one_piece[name] - ref[64][name]).abs().max().item():.2e}")
    with pytest.raises(AssertionError, match="ours - ref64"):
        route_gate(one_piece, ref[32], ref[64], c["mode"], what="fp16 weight_hh_l0")
    sd = {k: (v.half().to(v.dtype) if k == "gru.gru.weight_hh_l0" else v) for k, v in ref["sd"].items()}
    with pytest.raises(AssertionError, match="h_end"):
        route_gate(oracle_outputs(sd, ref["x"], torch.float64), ref[32], ref[64], c["mode"], what="fp16 gru weight_hh_l0")


@pytest.mark.parametrize("variant", ["plain", "carry"])
def test_the_gate_raises_on_exchanged_windows(variant):
    """The truth with two neighbouring picked windows exchanged: a kernel that writes a group's rows in the wrong order."""
    c, ref = _gate_case(variant)
    for i in (0, len(ref["picks"]) // 2, len(ref["picks"]) - 2):
        perm = list(range(len(ref["picks"])))
        perm[i], perm[i + 1] = perm[i + 1], perm[i]
        swapped = {k: v[perm] for k, v in ref[64].items()}
        with pytest.raises(AssertionError, match="ours - ref64"):
            route_gate(swapped, ref[32], ref[64], c["mode"], what="windows exchanged")
