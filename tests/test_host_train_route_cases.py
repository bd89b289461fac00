"""Preconditions of tests/test_gpu_train_routes.py, checked on the CPU: every case of tests/train_route_cases.py gets the train route,
the training forward's front route and the weight-gradient slab plans its hand-written entries say (mtadgat_train_route /
mtadgat_front_route / mtadgat_wgrad_plan), the slab plans equal a transcription of the arithmetic run_wgrad and wgrad_slabs had before
the hook existed, the table reaches every entry of its ledgers, no picked edge window sits at a kink, the float32 torch-op route stays
inside its cap against float64 on the picked windows of every run (the number the GPU gate's constant is derived from is printed), and
the GPU test's gate raises on three altered truths.  No GPU needed.

The references rest on sparse cotangents: under  L = sum_w <cp_w, preds_w> + <cr_w, recons_w>  with cp, cr non-zero only at K picked
windows every adjoint of every other window is zero in every layer, so each parameter gradient of the n-window call equals the sum over
the picked windows -- which _torchpath.forward evaluates in float64 in milliseconds whatever n is."""
import copy
import ctypes

import pytest
import torch

import helpers
import train_route_cases as tc
from test_host_gru_route import _create

PRECISION = {"fp32": 2, "fp32_strict": 0}
FWD_REL_TOL = 2e-6                                               # gru_route_cases.FP32_REL_TOL: the forward route gate's constant

# ---- models, inputs, picked windows and references of the runs (CPU), built once; the GPU file imports them -------------------------
_MODELS, _INPUTS, _REFS = {}, {}, {}


def base_model(shape):
    """The model of a shape on the CPU in eval mode, seeded, both attention biases drawn from a normal distribution.  Cached: callers
    deep-copy it."""
    from mtad_gat import MTAD_GAT
    if shape not in _MODELS:
        torch.manual_seed(tc.MODEL_SEEDS.get(shape, tc.MODEL_SEED))
        model = MTAD_GAT(**tc.SHAPES[shape]).eval()
        with torch.no_grad():
            model.feature_gat.bias.normal_()
            model.temporal_gat.bias.normal_()
        _MODELS[shape] = (model, helpers.model64(model))
    return _MODELS[shape][0]


def model64(shape):
    base_model(shape)
    return _MODELS[shape][1]


def case_input(c):
    """x (n, W, F) ~ U[0, 1) under the case's seed, times the case's scale (un-normalised cases).  Cached: do not modify."""
    kw = tc.SHAPES[c["shape"]]
    scale = c.get("scale", 1.0)
    key = (c["n"], kw["window_size"], kw["n_features"], c["x_seed"], scale)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * c["x_seed"] + c["n"] % 1000)
        _INPUTS[key] = torch.rand(c["n"], kw["window_size"], kw["n_features"], generator=g) * scale
    return _INPUTS[key]


def dropout_seed():
    """The seed _hipgrad draws for a call made right after torch.manual_seed(tc.DROP_TORCH_SEED) (draw_dropout_stream)."""
    g = torch.Generator().manual_seed(tc.DROP_TORCH_SEED)
    return int(torch.randint(0, 2 ** 62, (1,), generator=g).item())


def picked_windows(c, p):
    """(picked windows, the edge windows among them, random windows replaced for sitting at a kink) of a run: windows 0, 1, n - 2,
    n - 1, both sides of the last 16-, 32- and 128-window group edges, of the chunk edges and of the slab edges of the n W-row sites
    (tc.pick_edges), then seeded random windows up to tc.K -- one at a kink (helpers.kink_windows with the GATv2 pair arguments, under
    the run's dropout masks) is replaced by the next seeded one."""
    kw = tc.SHAPES[c["shape"]]
    x = case_input(c)
    seed = dropout_seed() if p > 0 else 0
    edges, rows = tc.pick_edges(c)
    must = helpers.edge_windows(c["n"], edges, (16, 32, 128), rows, kw["window_size"])
    replaced = []

    def reject(ws):
        bad = helpers.kink_windows(model64(c["shape"]), x[ws], helpers.host_masks_at(kw, ws, p, seed), gatv2_pairs=True).tolist()
        replaced.extend(w for w, b in zip(ws, bad) if b)
        return bad
    picks = helpers.sample_windows(c["n"], edges, tc.K, seed=7000 + c["n"], groups=(16, 32, 128), row_edges=rows, window=kw["window_size"],
                                   reject=reject)
    return picks, must, replaced


def _as(masks, dtype):
    if masks is None:
        return None
    return {k: ([t.to(dtype) for t in v] if isinstance(v, list) else v.to(dtype)) for k, v in masks.items()}


def evaluate(model, xs, cp, cr, masks):
    """{"grads": {parameter name: gradient}, "preds", "recons"} of  sum_w <cp_w, preds_w> + <cr_w, recons_w>  over the windows xs through
    the torch-op algebra in the model's dtype, under the given keep-masks."""
    import _torchpath
    dt = next(model.parameters()).dtype
    names = [n for n, _ in model.named_parameters()]
    params = [q for _, q in model.named_parameters()]
    with torch.enable_grad():
        pr, rc = _torchpath.forward(model, xs.to(dt), _as(masks, dt))
        gs = torch.autograd.grad((pr * cp.to(dt)).sum() + (rc * cr.to(dt)).sum(), params)
    return {"grads": dict(zip(names, [g.detach() for g in gs])), "preds": pr.detach(), "recons": rc.detach()}


def reference(c, p):
    """The truth of a run: {"picks", "must", "replaced", "x" (the picked windows), "cp", "cr" (their cotangents), "seed", "masks"
    (host_masks_at of the picked GLOBAL windows, float64; None for p = 0), 64: evaluate() in float64, 32: in float32}.  Computed once
    and left unchanged."""
    key = (tc.case_id(c), p)
    if key not in _REFS:
        kw = tc.SHAPES[c["shape"]]
        picks, must, replaced = picked_windows(c, p)
        xs = case_input(c)[picks]
        cp, cr = helpers.separable_cotangents(len(picks), kw["window_size"], kw["out_dim"], seed=9000 + c["n"])
        seed = dropout_seed() if p > 0 else 0
        masks = helpers.host_masks_at(kw, picks, p, seed)
        m32 = copy.deepcopy(base_model(c["shape"])).eval()
        _REFS[key] = {"picks": picks, "must": must, "replaced": replaced, "x": xs, "cp": cp, "cr": cr, "seed": seed, "masks": masks,
                      64: evaluate(model64(c["shape"]), xs, cp, cr, masks), 32: evaluate(m32, xs, cp, cr, masks)}
    return _REFS[key]


# ---- the gates of the GPU test -------------------------------------------------------------------------------------------------------
def gate_constants(c, ref):
    """{parameter name: c_p} of a run's gate: tc.GATE_C, a route's own constant where tc.ROUTE_C names one; an un-normalised case:
    4 x the float32 route's own max |ref32_p - ref64_p| / s_p on this run, between tc.GATE_C and tc.GATE_C_MAX."""
    out = {}
    for name, g64 in ref[64]["grads"].items():
        out[name] = tc.ROUTE_C.get((tc.ATTENTION[c["shape"]], name), (tc.GATE_C,))[0]
        s = g64.abs().max().item()
        if c.get("scale") and s > 0:
            noise = (ref[32]["grads"][name].double() - g64).abs().max().item()
            out[name] = min(max(4 * noise / s, tc.GATE_C), tc.GATE_C_MAX)
    return out


def grad_gate(ours, ref32, ref64, c=tc.GATE_C, what=""):
    """Per parameter tensor p, s_p = max |ref64_p|:  max |ours_p - ref64_p| <= max |ref32_p - ref64_p| + c s_p + 1e-30, every entry
    finite.  ours / ref32 / ref64: {parameter name: gradient}; c: one constant or gate_constants' dict.  Returns
    {name: max |ours - ref64| / s_p} (0 where s_p is 0)."""
    assert set(ours) == set(ref64), (what, sorted(set(ours) ^ set(ref64)))
    worst, bad = {}, []
    for name, r64 in ref64.items():
        o, r64, r32 = ours[name].detach().cpu().double(), r64.double(), ref32[name].double()
        assert o.shape == r64.shape, (what, name, tuple(o.shape), tuple(r64.shape))
        assert torch.isfinite(o).all(), f"{what}: {name}: non-finite values"
        s = r64.abs().max().item()
        cp = c[name] if isinstance(c, dict) else c
        err, noise = (o - r64).abs().max().item(), (r32 - r64).abs().max().item()
        worst[name] = err / s if s > 0 else 0.0
        if not err <= noise + cp * s + 1e-30:
            bad.append(f"{name}: |ours - ref64| = {err:.3e} > |ref32 - ref64| {noise:.3e} + {cp:.1e} * {s:.3e}")
    assert not bad, what + ": " + "; ".join(bad)
    return worst


def forward_gate(ours, ref32, ref64, what=""):
    """tests/test_host_gru_route_cases.route_gate's rule on the training forward's outputs, per picked window w:
    max |ours - ref64|(w) <= max |ref32 - ref64|(w) + 2e-6 max(1, |ref64|max)."""
    worst = {}
    for name in ("preds", "recons"):
        o = ours[name].detach().cpu().double().flatten(1)
        r64, r32 = ref64[name].double().flatten(1), ref32[name].double().flatten(1)
        assert o.shape == r64.shape and torch.isfinite(o).all(), (what, name)
        tol = FWD_REL_TOL * max(1.0, r64.abs().max().item())
        err, noise = (o - r64).abs().amax(1), (r32 - r64).abs().amax(1)
        over = (err > noise + tol).nonzero().flatten().tolist()
        assert not over, f"{what}: {name}: picked rows {over[:8]}: |ours - ref64| = {err[over].max().item():.3e} > noise + {tol:.3e}"
        worst[name] = err.max().item()
    return worst


# ---- library queries -----------------------------------------------------------------------------------------------------------------
def host_engine(kw):
    """(lib, cfg, handle, a host-only Engine over a handle created as test_host_gru_route._create does): the hooks' Python wrappers
    without a device.  The engine owns the handle (its finaliser destroys it)."""
    import _native
    lib, cfg, h = _create(kw)
    e = _native.Engine.__new__(_native.Engine)
    e.lib, e.handle, e.cfg = lib, h, _native.Config(**cfg)
    return lib, cfg, h, e


def chunk_answers(eng, c, ch, mode):
    """(train route, front route, {site: (R, slabs, rows per slab, x3)}, row GEMM split) the engine gives one chunk under its current
    precision and options, spelled as the table spells them."""
    kw = tc.SHAPES[c["shape"]]
    n = ch["n"]
    plan = {s: (d["R"], d["nslab"], d["rows_per_slab"], d["x3"]) for s, d in eng.wgrad_plan(n).items()}
    split = eng.lib.mtadgat_rowgemm_split(eng.handle, 1, n * kw["window_size"], 1)
    return tc.describe_train(eng.train_route(n), tc.ATTENTION[c["shape"]]), tc.describe_front(eng.front_route(2, 0, n)), plan, split


def expected_plan(c, ch, mode, wk=0):
    """{site: (R, slabs, rows per slab, x3)} of a chunk from the table's hand-written entries, under Engine.wgrad_sites' names."""
    kw = tc.SHAPES[c["shape"]]
    x3 = int(tc.arithmetic(mode, wk) == "x3")
    out = {"conv": ch["rows"] + (x3,), "rec_fc": ch["rows"] + (x3,)}
    if kw["use_gatv2"]:
        out.update(feat_lin=ch["feat"] + (x3,), temp_lin=ch["rows"] + (x3,))
    for stack, layers in (("gru", kw["gru_n_layers"]), ("rec", kw["recon_n_layers"])):
        for l in range(layers):
            out[f"{stack}{l}_ih"] = out[f"{stack}{l}_hh"] = ch["rows"] + (x3,)
    for i in range(kw["forecast_n_layers"] + 1):
        out[f"fc{i}"] = ch["fc"] + (x3,)
    return out


def assert_case_routes(eng, c, mode, wk=0, what=""):
    """The hooks' answers for every chunk of a case equal the table (the engine already in `mode` with "wgrad_kernel" = wk)."""
    for ch in c["chunks"]:
        route, front, plan, split = chunk_answers(eng, c, ch, mode)
        assert route == ch["route"][mode], (what, ch["n"], route)
        assert front == ch["front"][mode], (what, ch["n"], front)
        assert plan == expected_plan(c, ch, mode, wk), (what, ch["n"], plan)
        assert split == (ch["rowsplit"] if mode == "fp32" else 0), (what, ch["n"], split)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _ru(v, m):
    return (v + m - 1) // m * m


def _parent_wgrad(cfg, n, prec, wk):
    """What run_wgrad computed inline next to wgrad_slabs (mtadgat_capi.cpp / mtadgat_pack.cpp) before mtadgat_wgrad_plan, per call of
    backward_impl / walk_stack_backward in the hook's site order: [R, M, N, Mp, Np, nslab, rows_per_slab, bmode, bshift, x3]."""
    F, W, taps = cfg["n_features"], cfg["window_size"], cfg["kernel_size"]
    Hg, Hr, od = cfg["gru_hid_dim"], cfg["recon_hid_dim"], cfg["out_dim"]
    RW = n * W
    sites = [(RW, F, taps * F, 1, 0)]
    if cfg["use_gatv2"]:
        sites += [(n * F, 2 * _ru(cfg["feat_embed"], 32), W, 0, 0), (RW, 2 * _ru(cfg["time_embed"], 32), F, 0, 0)]
    for l in range(cfg["gru_n_layers"]):
        sites += [(RW, 3 * _ru(Hg, 32), 3 * F if l == 0 else Hg, 0, 0), (RW, 3 * _ru(Hg, 32), Hg, 0, 1)]
    for l in range(cfg["recon_n_layers"]):
        sites += [(RW, 3 * _ru(Hr, 32), Hg if l == 0 else Hr, 0, 0), (RW, 3 * _ru(Hr, 32), Hr, 0, 1)]
    sites.append((RW, od, Hr, 0, 0))
    dims = [Hg] + [cfg["forecast_hid_dim"]] * (cfg["forecast_n_linear"] - 1) + [od]
    sites += [(n, dims[i + 1], dims[i], 0, 0) for i in range(cfg["forecast_n_linear"])]
    out = []
    for R, M, N, bmode, bshift in sites:
        Mp, Np = _ru(M, 32), _ru(N + 1, 32)
        tiles = ((Mp + 127) // 128) * ((Np + 127) // 128)        # wgrad_slabs
        s = min(1024 // tiles, (R + 383) // 384, 512)
        if s >= 8:
            s = s // 8 * 8
        s = max(s, 1)
        rps = _ru((R + s - 1) // s, 16)                          # run_wgrad
        x3 = int((prec == 2 and wk != 1) or wk == 2)
        out.append([R, M, N, Mp, Np, s, rps, bmode, bshift, x3])
    return out


@pytest.mark.parametrize("shape", list(tc.SHAPES))
def test_routes_and_slab_plans_equal_the_hand_written_table(shape):
    import _native
    cases = [c for c in tc.CASES + tc.UNNORMALISED_CASES if c["shape"] == shape]
    assert cases, shape
    lib, cfg, h, eng = host_engine(tc.SHAPES[shape])
    try:
        for c in cases:
            for mode in tc.MODES:
                assert lib.mtadgat_set_precision(h, PRECISION[mode]) == 0
                for wk in [0] + [k for m, k in c["wgrad_kernels"] if m == mode]:
                    assert lib.mtadgat_set_option(h, b"wgrad_kernel", wk) == 0
                    assert_case_routes(eng, c, mode, wk, what=(tc.case_id(c), mode, wk))
                    for ch in c["chunks"]:                       # ... and the whole answer equals the parent's arithmetic
                        got = eng.wgrad_plan(ch["n"])
                        assert list(got) == eng.wgrad_sites()
                        flat = [[d[k] for k in _native.WGRAD_PLAN_FIELDS] for d in got.values()]
                        assert flat == _parent_wgrad(cfg, ch["n"], PRECISION[mode], wk), (tc.case_id(c), mode, wk, ch["n"])
    finally:
        lib.mtadgat_set_option(h, b"wgrad_kernel", 0)


@pytest.mark.parametrize("shape", ["base", "stacked", "fc_out", "wide", "wide_v1"])
def test_slab_plan_equals_the_parent_arithmetic_at_every_edge(shape):
    """Beyond the table: both sides of every slab-count step up to a chunk, in both modes and under every "wgrad_kernel" value."""
    import _native
    lib, cfg, h, eng = host_engine(tc.SHAPES[shape])
    W = cfg["window_size"]
    sizes = sorted({n for r in range(384, 8192 * 10 + 1, 384) for n in (r // W, r // W + 1, r, r + 1) if 1 <= n <= tc.TRAIN_CHUNK} | {1, 2, 63, 64})
    if W > 100:
        sizes = sizes[:400]
    try:
        for mode, prec in PRECISION.items():
            assert lib.mtadgat_set_precision(h, prec) == 0
            for wk in (0, 1, 2):
                assert lib.mtadgat_set_option(h, b"wgrad_kernel", wk) == 0
                for n in sizes if wk == 0 else sizes[::37]:
                    flat = [[d[k] for k in _native.WGRAD_PLAN_FIELDS] for d in eng.wgrad_plan(n).values()]
                    assert flat == _parent_wgrad(cfg, n, prec, wk), (shape, mode, wk, n)
    finally:
        lib.mtadgat_set_option(h, b"wgrad_kernel", 0)


def test_wgrad_plan_rejects_bad_arguments_and_needs_no_weights():
    lib, cfg, h, eng = host_engine(tc.SHAPES["stacked"])
    cap = 10 * len(eng.wgrad_sites())
    buf = (ctypes.c_int64 * (cap + 1))(*([-7] * (cap + 1)))
    assert lib.mtadgat_wgrad_plan(h, 256, buf, cap) == cap and buf[cap] == -7           # no weights loaded, no GPU touched
    assert lib.mtadgat_wgrad_plan(None, 256, buf, cap) == -1 and lib.mtadgat_wgrad_plan(h, 256, None, cap) == -1
    assert lib.mtadgat_wgrad_plan(h, 0, buf, cap) == -1
    untouched = (ctypes.c_int64 * cap)(*([-7] * cap))
    assert lib.mtadgat_wgrad_plan(h, 256, untouched, cap - 1) == -1 and list(untouched) == [-7] * cap


def test_the_table_is_well_formed():
    assert len(set(tc.RUN_IDS)) == len(tc.RUN_IDS) and len(set(map(tc.case_id, tc.CASES))) == len(tc.CASES)
    assert 16 % tc.BASE["window_size"] != 0 and tc.BASE["window_size"] % 16 != 0      # slab edges fall inside windows
    for c in tc.CASES:
        kw = tc.SHAPES[c["shape"]]
        for ch in c["chunks"]:
            assert ch["rows"][0] == ch["n"] * kw["window_size"] and ch["fc"][0] == ch["n"], tc.case_id(c)
            assert (ch["feat"] is None) == (not kw["use_gatv2"]) and (ch["feat"] is None or ch["feat"][0] == ch["n"] * kw["n_features"])
            for _, plan in tc.site_plans(c, ch):
                tc.slab_class(plan)                              # (asserts the plan's own consistency)
    # the sizes mean what the table's comments say
    by = {tc.case_id(c): c for c in tc.CASES}
    assert tc.slab_class(by["base-n1792"]["chunks"][0]["rows"]) == "x8_full" and tc.slab_class(by["base-n1793"]["chunks"][0]["rows"]) == "x8_empty"
    R, nslab, rps = by["w8-n8192"]["chunks"][0]["rows"]
    assert (R, nslab, rps) == (65536, 168, 400) and nslab % 8 == 0 and [s for s in range(nslab) if s * rps >= R] == [164, 165, 166, 167]
    assert by["base-n6553"]["chunks"][0]["rowsplit"] == 0 and by["base-n6554"]["chunks"][0]["rowsplit"] == 1
    assert [ch["n"] for ch in by["base-n12288"]["chunks"]] == [8192, 4096] and [ch["n"] for ch in by["base-n8193"]["chunks"]] == [8192, 1]


def test_ledgers_every_entry_is_still_reached():
    slabs, recs, fcs, atts = tc.ledger_of(tc.RUNS)
    missing = [e for e in tc.SLAB_LEDGER if e not in slabs]
    assert not missing, f"no run reaches {missing}"
    assert not (slabs & set(tc.UNREACHABLE_SLABS)), slabs & set(tc.UNREACHABLE_SLABS)
    assert set(tc.RECURRENCE_LEDGER) == recs, (sorted(recs), "the table and the recurrence ledger differ")
    assert set(tc.FC_LEDGER) == fcs and set(tc.ATTENTION_LEDGER) == atts, (fcs, atts)
    # every arithmetic at every site kind also through the "wgrad_kernel" option (the staging builds crossed with the arithmetic)
    crossed, _, _, _ = tc.ledger_of([r for r in tc.RUNS if r[2]])
    assert {(k, a) for k, a, _ in crossed} == {(k, a) for k in tc.SITE_KINDS for a in ("x3", "fp32")}


def test_the_unreachable_slab_entries_are_unreachable():
    """A forecasting Linear walks n <= TRAIN_CHUNK rows: the parent arithmetic never leaves it an empty trailing slab, whatever n."""
    for n in range(1, tc.TRAIN_CHUNK + 1):
        s = min(1024, (n + 383) // 384, 512)
        s = max(s // 8 * 8 if s >= 8 else s, 1)
        rps = _ru((n + s - 1) // s, 16)
        assert (s - 1) * rps < n, (n, s, rps)


# ---- the picked windows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, tc.P_DROP])
def test_picked_windows_cover_the_edges_and_avoid_the_kinks(p):
    """No edge window sits at a kink (the case's x_seed is chosen so), a random window at a kink was replaced by the next seeded one,
    and no run is left with fewer than 90 % of its K windows."""
    replaced = 0
    for c in tc.CASES + tc.UNNORMALISED_CASES:
        kw = tc.SHAPES[c["shape"]]
        ref = reference(c, p)
        picks, must = ref["picks"], ref["must"]
        what = (tc.case_id(c), p)
        assert picks == sorted(set(picks)) and set(must) <= set(picks) and len(picks) >= 0.9 * min(tc.K, c["n"]), what
        n, W = c["n"], kw["window_size"]
        want = {0, 1, n - 2, n - 1} | {e + d for g in (16, 32, 128) for e in [(n - 1) // g * g] for d in (-1, 0)}
        at = 0
        for ch in c["chunks"]:
            want |= {at - 1, at} if at else set()
            for r in tc.slab_edges(ch["rows"]):                  # both sides of the slab edge, as windows: rows r - 1 and r
                want |= {(at * W + r - 1) // W, (at * W + r) // W}
            at += ch["n"]
        assert {w for w in want if 0 <= w < n} <= set(must), what
        bad = helpers.kink_windows(model64(c["shape"]), ref["x"], ref["masks"], gatv2_pairs=True)
        assert not bad.any(), (what, "picked windows at a kink", [w for w, b in zip(picks, bad.tolist()) if b])
        assert not (set(ref["replaced"]) & set(picks)), what
        replaced += len(ref["replaced"])
    print(f"p = {p}: {replaced} random windows at a kink replaced over {len(tc.CASES)} cases")


def test_the_restated_dropout_seed_is_what_a_seeded_call_draws():
    torch.manual_seed(tc.DROP_TORCH_SEED)
    assert int(torch.randint(0, 2 ** 62, (1,)).item()) == dropout_seed()


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def test_float32_route_stays_inside_its_cap():
    """Per run and parameter tensor: max |ref32 - ref64| / max |ref64| of the float32 torch-op route on the CPU.  The largest is the
    number tc.GATE_C is derived from (4 x, between 2e-6 and 1e-5): printed, held under tc.REF32_REL_CAP, and tc.GATE_C is held to
    the recorded measurement."""
    worst, where = 0.0, None
    for c in tc.CASES:
        for p in (0.0, tc.P_DROP):
            ref = reference(c, p)
            for name, g64 in ref[64]["grads"].items():
                s = g64.abs().max().item()
                assert s >= 1e-6, (tc.case_id(c), p, name, s, "a parameter whose gradient vanishes: nothing to hold a kernel against")
                r = (ref[32]["grads"][name].double() - g64).abs().max().item() / s
                if r > worst:
                    worst, where = r, (tc.case_id(c), p, name)
                assert r <= tc.REF32_REL_CAP, (tc.case_id(c), p, name, r)
    print(f"float32 torch-op route against float64, largest max|ref32 - ref64| / max|ref64| per parameter tensor: {worst:.2e} at {where}")
    for c in tc.UNNORMALISED_CASES:                              # not capped: the gate's noise term carries what these inputs cost float32
        for p in (0.0, tc.P_DROP):
            ref = reference(c, p)
            r = max((ref[32]["grads"][n].double() - g).abs().max().item() / g.abs().max().item() for n, g in ref[64]["grads"].items())
            print(f"{tc.case_id(c)} p={p}: largest max|ref32 - ref64| / max|ref64| {r:.2e}")
    assert worst <= 1.25 * tc.REF32_REL_MEASURED, (worst, "beyond the recorded measurement: re-derive tc.GATE_C")
    assert tc.GATE_C == min(max(4 * tc.REF32_REL_MEASURED, tc.GATE_C_FLOOR), tc.GATE_C_CEIL)
    for (att, name), (cr, measured, reason) in tc.ROUTE_C.items():
        assert att in tc.ATTENTION_LEDGER and tc.GATE_C <= cr <= tc.GATE_C_MAX and measured <= cr and reason
        own = max((reference(c, p)[32]["grads"][name].double() - reference(c, p)[64]["grads"][name]).abs().max().item() /
                  reference(c, p)[64]["grads"][name].abs().max().item() for c in tc.CASES if tc.ATTENTION[c["shape"]] == att for p in (0.0, tc.P_DROP))
        assert cr <= 4 * 1.25 * own, (att, name, cr, own, "beyond 4 x the float32 route's own ratio on this tensor")


# ---- the gate can fail ----------------------------------------------------------------------------------------------------------------
GATE_CASES = [("base-n1793", 0.0), ("stacked-n2561", tc.P_DROP)]   # a plain case; a stacked case with dropout


def _gate_case(cid, p):
    c = next(c for c in tc.CASES if tc.case_id(c) == cid)
    ref = reference(c, p)
    grad_gate(ref[64]["grads"], ref[32]["grads"], ref[64]["grads"], what="the truth itself")          # passes
    grad_gate(ref[32]["grads"], ref[32]["grads"], ref[64]["grads"], what="the float32 route")          # passes: the noise term
    return c, ref


@pytest.mark.parametrize("cid,p", GATE_CASES)
def test_the_gate_raises_on_a_dropped_row(cid, p):
    """The truth with the cotangent of ONE (window, step) row zeroed -- a row a slab dropped -- at the first, a middle and the last
    picked window."""
    c, ref = _gate_case(cid, p)
    W = tc.SHAPES[c["shape"]]["window_size"]
    for i, t in ((0, 0), (len(ref["picks"]) // 2, W // 2), (len(ref["picks"]) - 1, W - 1)):
        cr = ref["cr"].clone()
        cr[i, t] = 0.0
        got = evaluate(model64(c["shape"]), ref["x"], ref["cp"], cr, ref["masks"])["grads"]
        with pytest.raises(AssertionError, match="ours - ref64"):
            grad_gate(got, ref[32]["grads"], ref[64]["grads"], what=f"row ({ref['picks'][i]}, {t}) dropped")


@pytest.mark.parametrize("cid,p", GATE_CASES)
def test_the_gate_raises_on_exchanged_windows(cid, p):
    """The truth with the inputs of two adjacent picked windows exchanged (cotangents and masks stay): rows taken from the neighbour."""
    c, ref = _gate_case(cid, p)
    for i in (0, len(ref["picks"]) // 2, len(ref["picks"]) - 2):
        perm = list(range(len(ref["picks"])))
        perm[i], perm[i + 1] = perm[i + 1], perm[i]
        got = evaluate(model64(c["shape"]), ref["x"][perm], ref["cp"], ref["cr"], ref["masks"])["grads"]
        with pytest.raises(AssertionError, match="ours - ref64"):
            grad_gate(got, ref[32]["grads"], ref[64]["grads"], what="windows exchanged")


def _two_bf16_pieces(t):
    hi = t.to(torch.bfloat16).to(t.dtype)
    return hi + (t - hi).to(torch.bfloat16).to(t.dtype)


# whether the gate refuses a weight_hh_l0 held on two bf16 pieces instead of three, per gate case (DESIGN.md section 7 records the
# measured movement)
DROPPED_PIECE_REFUSED = {"base-n1793": False, "stacked-n2561": False}


@pytest.mark.parametrize("cid,p", GATE_CASES)
def test_the_gate_on_a_dropped_third_piece(cid, p):
    """A float64 replay in which weight_hh_l0 of the GRU stack and of the decoder is the sum of two bf16 pieces -- the split operands
    with their third piece dropped (relative error up to 2^-17 per weight).  The movement of every gradient is printed; whether the
    gate refuses it is held to what DESIGN.md section 7 records."""
    c, ref = _gate_case(cid, p)
    m = copy.deepcopy(model64(c["shape"]))
    with torch.no_grad():
        for name, q in m.named_parameters():
            if name.endswith("weight_hh_l0"):
                q.copy_(_two_bf16_pieces(q))
    got = evaluate(m, ref["x"], ref["cp"], ref["cr"], ref["masks"])["grads"]
    moved = {n: (got[n] - g).abs().max().item() / g.abs().max().item() for n, g in ref[64]["grads"].items()}
    top = sorted(moved.items(), key=lambda kv: -kv[1])[:3]
    print(f"{cid} p={p}: two-piece weight_hh_l0 moves " + ", ".join(f"{n} by {v:.2e}" for n, v in top) + f" of its scale; gate c = {tc.GATE_C:.1e}")
    try:
        grad_gate(got, ref[32]["grads"], ref[64]["grads"], what="two-piece weight_hh_l0")
        refused = False
    except AssertionError as e:
        assert "ours - ref64" in str(e)
        refused = True
    assert refused == DROPPED_PIECE_REFUSED[cid], (cid, refused, top)
