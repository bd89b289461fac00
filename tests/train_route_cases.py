"""Cases and specification for the parameter gradients of a training step, route by route (tests/test_host_train_route_cases.py on
the CPU, tests/test_gpu_train_routes.py on the GPU): tiny models at call sizes that reach every recurrence pair (training forward,
backward) mtadgat_train_route can name, both attention backwards, the decoder's Linear inside and outside its recurrence, k_gath in the
training forward, and every slab layout of the weight-gradient GEMM (k_wgrad_lds) that mtadgat_wgrad_plan can report -- one slab,
fewer than 8, whole groups of 8 (the XCD-aware block map) with full and with EMPTY trailing slabs, per site kind and arithmetic.

Both staging builds of the kernel run in every case: the sites whose row strides are multiples of 4 floats take float4 loads, the
decoder's Linear and the last forecasting Linear (A rows of out_dim = 3 floats) dword loads, the convolution its im2col loader; the
"wgrad_kernel" option crosses them with the other arithmetic at a few small sizes.  Which one a site takes depends on the alignment of
the call's buffers and is not part of mtadgat_wgrad_plan.

The default window length is 10: it does not divide the 16-row staging step, so slab edges fall inside windows and the rows that W_hh's
gradient reads one step earlier (bshift) cross them.

Every case carries its HAND-WRITTEN expectations per chunk of the Python step (_hipgrad.TRAIN_CHUNK = 8192 windows): the train route
and the training forward's front route in both fp32 precision modes, the slab plan (rows, slabs, rows per slab) of the sites that walk
all (window, step) rows -- convolution, temporal projection, W_ih / W_hh of every layer, the decoder's Linear --, of the feature
projection (n F rows) and of the forecasting Linears (n rows), and whether the backward's row GEMMs over n W rows take split operands.
The CPU test holds the library's hooks against these and the slab plans against a transcription of the arithmetic of the commit before
mtadgat_wgrad_plan existed; the GPU test asserts them again before each call.

This file is the specification in plain Python: it imports nothing, uses no GPU and makes no library call.  The models, inputs, picked
windows, float32 / float64 references and the gate are built by tests/test_host_train_route_cases.py, for both test files."""

TRAIN_CHUNK = 8192                                               # _hipgrad.TRAIN_CHUNK
MODEL_SEED = 41
# GAT (v1) under seed 41: the scores of the temporal layer have one sign everywhere, the softmax rows do not see lin.bias and its
# gradient vanishes (1e-18 in float64) -- nothing to hold a kernel against; these seeds give every parameter a gradient
MODEL_SEEDS = {"v1": 46, "wide_v1": 44}
DROP_TORCH_SEED = 77                                             # torch.manual_seed before the call: what _hipgrad draws its dropout seed from
K = 32                                                           # picked windows per run; the rest of the call gets zero cotangents
MODES = ("fp32", "fp32_strict")                                  # MTAD_GAT.precision: mtadgat_set_precision 2 / 0
P_DROP = 0.2

# ---- the gate ----------------------------------------------------------------------------------------------------------------------
# Per parameter tensor p, s_p = max |ref64_p|:   max |ours_p - ref64_p| <= max |ref32_p - ref64_p| + GATE_C s_p + 1e-30.
# GATE_C is measured against the REFERENCE, not against the kernels: tests/test_host_train_route_cases.py prints the largest
# max |ref32_p - ref64_p| / s_p of the float32 torch-op route on the CPU over every run of the table -- REF32_REL_MEASURED below --
# and GATE_C = 4 x that (the factor covers another summation order of the K W terms), not below 2e-6 (the forward route gate's
# constant, gru_route_cases.FP32_REL_TOL) and not above 1e-5 (helpers.WINDOW_NOISE_REL).
REF32_REL_MEASURED = 7.0e-6    # wide_v1-n40, p = 0, temporal_gat.lin.bias (a sum that cancels to 5e-4); the attention layers' a and
#                                lin.bias hold the top twenty entries (2e-6 .. 7e-6), every recurrence and Linear weight is below 1e-6
REF32_REL_CAP = 1e-5                                             # the float32 route is held to helpers.WINDOW_NOISE_REL per tensor
GATE_C_FLOOR, GATE_C_CEIL = 2e-6, 1e-5
GATE_C = 1e-5                                                    # 4 x 7.0e-6 = 2.8e-5, cut to the ceiling
# Routes that need their own constant on the MI355X: {(attention route, parameter): (c, measured |ours - ref64| / s_p, reason)}.
# Never above 1e-4; derived like GATE_C, from the reference's own ratio on that tensor, not from the HIP output.
ROUTE_C = {
    ("wide:v1", "temporal_gat.lin.bias"): (
        2.8e-5, 1.5e-5,
        "GAT (v1): d lin.bias = (a1 + a2) sum d s over all pairs of all windows, a sum that cancels (the softmax rows are nearly blind "
        "to a shift of the scores) to 6e-4 here; the float32 route itself is 7.0e-6 off on this tensor at 40 windows of 130 nodes "
        "(REF32_REL_MEASURED), 4 x that without the ceiling is 2.8e-5; k_bw_v1 + k_sum_rows measured 1.5e-5 with dropout, 9.0e-6 without"),
}
GATE_C_MAX = 1e-4                                                # the whole-tensor gate of tests/test_gpu_backward.py: no constant goes above it
# The un-normalised runs (UNNORMALISED_CASES below): inputs x 4e5.  Gate pre-activations of 1e5 carry 1e-2 of float32 rounding, the
# first GRU layer's gate gradients e^-|a| move by per cent with it: the float32 route itself is 1.5e-4 of the scale off on
# gru.weight_ih_l0.  Their gate is scaled by the reference, per tensor: c_p = 4 x (max |ref32_p - ref64_p| / s_p) of that run, not below
# GATE_C, not above GATE_C_MAX.
UNNORMALISED_SCALE = 4e5

# ---- shapes: MTAD_GAT kwargs -------------------------------------------------------------------------------------------------------
BASE = dict(n_features=6, window_size=10, out_dim=3, kernel_size=3, gru_n_layers=1, gru_hid_dim=24, recon_n_layers=1, recon_hid_dim=20,
            forecast_n_layers=1, forecast_hid_dim=16, use_gatv2=True, dropout=P_DROP, alpha=0.2)
SHAPES = {
    "base": dict(BASE),
    "v1": dict(BASE, use_gatv2=False),
    # two layers per stack: the 16-window-group kernels never apply, nn.GRU's inter-layer dropout runs.  Two hidden tiles (40 / 36):
    # with one tile (the base shape) no training forward ever takes split operands, with two it does from 2 561 windows
    "stacked": dict(BASE, gru_n_layers=2, recon_n_layers=2, gru_hid_dim=40, recon_hid_dim=36),
    # rec_fc_rides_train: (NCG 1024 + NCG out_dim 32) 4 <= 65 536 bytes.  One tile breaks it only above 480 outputs, four tiles
    # (hidden 97) from 97 outputs: the smallest product.  Two decoder layers keep the decoder off the small-batch kernels at any size
    "fc_out": dict(BASE, out_dim=97, recon_n_layers=2, recon_hid_dim=97),
    "fc_in": dict(BASE, out_dim=96, recon_n_layers=2, recon_hid_dim=97),
    # more than 128 nodes in the temporal layer (and node vectors of more than 128 entries in the feature layer): both un-fused
    "wide": dict(BASE, window_size=130),
    "wide_v1": dict(BASE, window_size=130, use_gatv2=False),
    "gath": dict(BASE, window_size=100),                          # W >= 97: k_gath keeps the softmax rows from 4 096 windows
    "blocks": dict(BASE, gru_hid_dim=48),                         # 3 Hp = 192 > 128: two output block rows, the second half padding
    "w8": dict(BASE, window_size=8),                              # 8 192 windows = 65 536 rows: 168 slabs of 400, 164 .. 167 empty
}
# (wide, v1) of both attention layers, hand-written per shape
ATTENTION = {"base": "fused:v2", "v1": "fused:v1", "stacked": "fused:v2", "fc_out": "fused:v2", "fc_in": "fused:v2", "wide": "wide:v2",
             "wide_v1": "wide:v1", "gath": "fused:v2", "blocks": "fused:v2", "w8": "fused:v2"}

# ---- route spellings ---------------------------------------------------------------------------------------------------------------
# one recurrence layer: "<training forward's first kernel>><backward kernel>[:x3]"
FWD = {1: "gru1", 2: "gru16", 3: "split", 4: "splitx3"}           # GruKernel codes a training forward can get
BWD = {0: "gru1_bwd", 1: "gru16_bwd", 2: "gru_bwd"}              # GruBwdKernel
G1, G16 = "gru1>gru1_bwd", "gru16>gru16_bwd"
SP, SP3, SX3 = "split>gru_bwd", "split>gru_bwd:x3", "splitx3>gru_bwd:x3"
# front route of the training forward (kind 2, float32 windows): "convolution | temporal layer | feature layer"
F_GAT = "launch_conv:fp32:range | k_gat:fp32 | k_gat:fp32"
F_GATH = "launch_conv:fp32:range | k_gath+k_gat:x3:fp16:pack | k_gath+k_gat:x3:fp16:pack"
F_WIDE = "launch_conv:fp32:range | rowgemm+k_gat_wide:fp32 | rowgemm+k_gat_wide:fp32"


def describe_train(r, attention):
    """A train_route dict (Engine.train_route) as "GRU layers | decoder layers | fc:in / fc:row"; its (wide, v1) pairs must spell
    `attention` (the shape's entry of ATTENTION)."""
    def layer(t):
        return FWD[t[0]] + ">" + BWD[t[1]] + (":x3" if t[2] else "")
    att = {(0, 0): "fused:v2", (0, 1): "fused:v1", (1, 0): "wide:v2", (1, 1): "wide:v1"}
    assert r["feat"] == r["temp"], r
    assert att[tuple(r["feat"])] == attention, (r, attention)
    return " | ".join([", ".join(map(layer, r["gru"])), ", ".join(map(layer, r["rec"])), "fc:in" if r["rec_fc_rides"] else "fc:row"])


def describe_front(f):
    """A front_route dict (Engine.front_route) of the training forward as the F_* strings spell it."""
    convs = ("in_gath", "k_conv_win", "shared_rows", "launch_conv")
    layers = ("none", "k_gat", "k_gath+k_gat", "rowgemm+k_gat_wide", "rowgemm+k_attend")
    builds = ("fp32", "bf16", "x3")
    out = [convs[f["conv"]] + ":" + builds[f["conv_build"]] + (":pack" if f["conv_split_pack"] else "") + (":range" if f["range"] else "")]
    for k in ("temp", "feat"):
        out.append(layers[f[k + "_kernel"]] + ":" + builds[f[k + "_build"]] + (":fp16" if f[k + "_fp16"] else "") +
                   (":splitgemm" if f[k + "_split_gemm"] else "") + (":pack" if f[k + "_split_pack"] else ""))
    return " | ".join(out)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _chunk(n, route32, route0, front32, rows, feat, fc, rowsplit=0, front0=F_GAT):
    """One chunk of n windows.  route32 / route0: "GRU | decoder | fc" in mode fp32 / fp32_strict; front32 / front0 likewise; rows,
    feat, fc: (R, slabs, rows per slab) of the n W-row sites, the feature projection (None: GAT v1 has none) and the forecasting
    Linears; rowsplit: the backward's row GEMMs over n W rows take split operands in mode fp32 (never in fp32_strict)."""
    return dict(n=n, route={"fp32": route32, "fp32_strict": route0}, front={"fp32": front32, "fp32_strict": front0}, rows=rows, feat=feat,
                fc=fc, rowsplit=rowsplit)


def _case(shape, n, chunks, x_seed, wgrad_kernels=()):
    """x_seed: the input's seed, the first from 1 on that leaves no edge window of the case at a kink, with and without dropout
    (tests/test_host_train_route_cases.py asserts that none is).  wgrad_kernels: extra runs (mode, "wgrad_kernel" value): 1 the fp32 MFMA in mode fp32, 2 split operands in mode fp32_strict."""
    chunks = [chunks] if isinstance(chunks, dict) else list(chunks)
    assert sum(c["n"] for c in chunks) == n and all(c["n"] == TRAIN_CHUNK for c in chunks[:-1])
    return dict(shape=shape, n=n, chunks=chunks, x_seed=x_seed, wgrad_kernels=tuple(wgrad_kernels))


SMALL1 = "%s | %s | fc:row" % (G1, G1)
SMALL16 = "%s | %s | fc:row" % (G16, G16)
BIG32, BIG0 = "%s | %s | fc:in" % (SP3, SP3), "%s | %s | fc:in" % (SP, SP)
ST32 = "%s, %s | %s, %s | fc:in" % (SP3, SP3, SP3, SP3)
ST0 = "%s, %s | %s, %s | fc:in" % (SP, SP, SP, SP)
STX = "%s, %s | %s, %s | fc:in" % (SX3, SX3, SX3, SX3)
CROSS = (("fp32", 1), ("fp32_strict", 2))
# the chunks that several cases share
_C8192 = _chunk(8192, BIG32, BIG0, F_GATH, (81920, 208, 400), (49152, 128, 384), (8192, 16, 512), rowsplit=1)
_C1 = _chunk(1, SMALL1, SMALL1, F_GAT, (10, 1, 16), (6, 1, 16), (1, 1, 16))
_C4096 = _chunk(4096, SMALL16, SMALL16, F_GATH, (40960, 104, 400), (24576, 64, 384), (4096, 8, 512))

CASES = [
    # ---- base: one layer per stack, fused GATv2
    # R = 370 < 384: one slab of 384 rows everywhere; the forecasting sites have 37 < 64 rows
    _case("base", 37, _chunk(37, SMALL1, SMALL1, F_GAT, (370, 1, 384), (222, 1, 224), (37, 1, 48)), 1, CROSS),
    # 4 slabs of 384 rows (the last holds 348), 3 of 304 in the feature projection
    _case("base", 150, _chunk(150, SMALL1, SMALL1, F_GAT, (1500, 4, 384), (900, 3, 304), (150, 1, 160)), 1, CROSS),
    # 40 FULL slabs of 448 rows = 17 920: the XCD map on; the last size of k_gru1 / k_gru1_bwd
    _case("base", 1792, _chunk(1792, SMALL1, SMALL1, F_GAT, (17920, 40, 448), (10752, 24, 448), (1792, 5, 368)), 1),
    # 17 930 rows: 449 per slab rounded up to 464, 39 x 464 = 18 096 > R: slab 39 is EMPTY (feature projection: 24 x 464, slab 23 holds 86)
    _case("base", 1793, _chunk(1793, SMALL16, SMALL16, F_GAT, (17930, 40, 464), (10758, 24, 464), (1793, 5, 368)), 1, CROSS),
    # 2 560 | 2 561: where a training forward of two hidden tiles turns to split operands (shape "stacked"); with one tile nothing
    # changes but the slabs: 64 full slabs of 400 | 64 of 416 with slabs 62, 63 empty (62 x 416 = 25 792 > 25 610)
    _case("base", 2560, _chunk(2560, SMALL16, SMALL16, F_GAT, (25600, 64, 400), (15360, 40, 384), (2560, 7, 368)), 1),
    _case("base", 2561, _chunk(2561, SMALL16, SMALL16, F_GAT, (25610, 64, 416), (15366, 40, 400), (2561, 7, 368)), 1),
    # 4 096: the last size of k_gru16_bwd, the first of k_gath in the training forward (mode fp32); 4 097: k_gru_split + k_gru_bwd,
    # the decoder's Linear inside the recurrence
    _case("base", 4096, _C4096, 2),
    _case("base", 4097, _chunk(4097, BIG32, BIG0, F_GATH, (40970, 104, 400), (24582, 64, 400), (4097, 8, 528)), 1),
    # n W = 65 530 | 65 540: the backward's row GEMMs turn to split operands from 65 536 rows (mode fp32)
    _case("base", 6553, _chunk(6553, BIG32, BIG0, F_GATH, (65530, 168, 400), (39318, 96, 416), (6553, 16, 416)), 1),
    _case("base", 6554, _chunk(6554, BIG32, BIG0, F_GATH, (65540, 168, 400), (39324, 96, 416), (6554, 16, 416), rowsplit=1), 1),
    # TRAIN_CHUNK: one chunk | two chunks whose gradients accumulate, the second of ONE window | a second chunk at window0 = 8 192
    _case("base", 8192, _C8192, 1),
    _case("base", 8193, [_C8192, _C1], 1),
    _case("base", 12288, [_C8192, _C4096], 1),
    # ---- v1: GAT (v1) scores; no projection site (its parameter gradients are column sums)
    _case("v1", 37, _chunk(37, SMALL1, SMALL1, F_GAT, (370, 1, 384), None, (37, 1, 48)), 1),
    _case("v1", 1793, _chunk(1793, SMALL16, SMALL16, F_GAT, (17930, 40, 464), None, (1793, 5, 368)), 1),
    _case("v1", 4097, _chunk(4097, BIG32, BIG0, F_GATH, (40970, 104, 400), None, (4097, 8, 528)), 1),
    _case("v1", 8193, [dict(_C8192, feat=None), dict(_C1, feat=None)], 1),
    # ---- stacked: two layers of two hidden tiles per stack
    _case("stacked", 37, _chunk(37, ST32, ST0, F_GAT, (370, 1, 384), (222, 1, 224), (37, 1, 48)), 1, CROSS),
    _case("stacked", 2560, _chunk(2560, ST32, ST0, F_GAT, (25600, 64, 400), (15360, 40, 384), (2560, 7, 368)), 1),
    _case("stacked", 2561, _chunk(2561, STX, ST0, F_GAT, (25610, 64, 416), (15366, 40, 400), (2561, 7, 368)), 1),
    _case("stacked", 4097, _chunk(4097, STX, ST0, F_GATH, (40970, 104, 400), (24582, 64, 400), (4097, 8, 528)), 1),
    _case("stacked", 8193, [dict(_C8192, route={"fp32": STX, "fp32_strict": ST0}), dict(_C1, route={"fp32": ST32, "fp32_strict": ST0})], 1),
    # ---- the decoder's per-step Linear outside | inside the recurrence
    _case("fc_out", 150, _chunk(150, "%s | %s, %s | fc:row" % (G1, SP3, SP3), "%s | %s, %s | fc:row" % (G1, SP, SP), F_GAT,
                                (1500, 4, 384), (900, 3, 304), (150, 1, 160)), 1),
    _case("fc_in", 150, _chunk(150, "%s | %s, %s | fc:in" % (G1, SP3, SP3), "%s | %s, %s | fc:in" % (G1, SP, SP), F_GAT,
                               (1500, 4, 384), (900, 3, 304), (150, 1, 160)), 1),
    # ---- un-fused attention layers, small calls only (650 rows: 2 slabs of 336; 5 200 rows: 8 slabs of 656, the last holds 608)
    _case("wide", 5, _chunk(5, SMALL1, SMALL1, F_WIDE, (650, 2, 336), (30, 1, 32), (5, 1, 16), front0=F_WIDE), 2),
    _case("wide", 40, _chunk(40, SMALL1, SMALL1, F_WIDE, (5200, 8, 656), (240, 1, 240), (40, 1, 48), front0=F_WIDE), 9),
    _case("wide_v1", 5, _chunk(5, SMALL1, SMALL1, F_WIDE, (650, 2, 336), None, (5, 1, 16), front0=F_WIDE), 1),
    _case("wide_v1", 40, _chunk(40, SMALL1, SMALL1, F_WIDE, (5200, 8, 656), None, (40, 1, 48), front0=F_WIDE), 1),
    # ---- k_gath with the softmax rows kept and dropout applied: W = 100 at 4 096 windows; 409 600 rows in the 512 slabs the plan allows
    _case("gath", 4096, _chunk(4096, SMALL16, SMALL16, F_GATH, (409600, 512, 800), (24576, 64, 384), (4096, 8, 512), rowsplit=1), 3),
    # ---- two output block rows in W_hh / W_ih of the GRU layer (Mp = 192), the last 64 x 128 of the second all padding
    _case("blocks", 150, _chunk(150, SMALL1, SMALL1, F_GAT, (1500, 4, 384), (900, 3, 304), (150, 1, 160)), 1, CROSS),
    _case("blocks", 4097, _chunk(4097, "%s | %s | fc:in" % (SX3, SP3), BIG0, F_GATH, (40970, 104, 400), (24582, 64, 400), (4097, 8, 528)), 1),
    # ---- 65 536 rows in 168 slabs of 400: 164 x 400 = 65 600 > R, slabs 164 .. 167 are empty, 168 % 8 == 0: the XCD map is on
    _case("w8", 8192, _chunk(8192, BIG32, BIG0, F_GATH, (65536, 168, 400), (49152, 128, 384), (8192, 16, 512), rowsplit=1), 1),
]

# ---- un-normalised inputs (x 4e5: convolution outputs beyond 2^15, the range of the two-fp16-piece operands) at 2 600 windows, held by
# the same gate -- its noise term, the float32 route's own distance from float64 on these inputs, scales it.  The base shape (one
# hidden tile) has no guarded recurrence at any size: its run holds the hoisted input products and the convolution's recorded range;
# "stacked" at 2 600 windows is on split operands (splitx3) with k_gru_split on fp32 operands as the device-side guard's fallback.
UNNORMALISED_CASES = [
    dict(_case("base", 2600, _chunk(2600, SMALL16, SMALL16, F_GAT, (26000, 64, 416), (15600, 40, 400), (2600, 7, 384)), 6), scale=UNNORMALISED_SCALE),
    dict(_case("stacked", 2600, _chunk(2600, STX, ST0, F_GAT, (26000, 64, 416), (15600, 40, 400), (2600, 7, 384)), 6), scale=UNNORMALISED_SCALE),
]


def case_id(c):
    return f"{c['shape']}-n{c['n']}" + ("-unnormalised" if c.get("scale") else "")


# one GPU test id per (case, mode, "wgrad_kernel"); every run does p = 0 and p = P_DROP
RUNS = [(c, m, 0) for c in CASES for m in MODES] + [(c, m, wk) for c in CASES for m, wk in c["wgrad_kernels"]]
RUN_IDS = [case_id(c) + "-" + m + ("-wk%d" % wk if wk else "") for c, m, wk in RUNS]


def arithmetic(mode, wgrad_kernel=0):
    """"x3" / "fp32": what the weight-gradient GEMMs multiply on (run_wgrad: mode fp32 unless "wgrad_kernel" is 1, or "wgrad_kernel" 2)."""
    return "x3" if (mode == "fp32" and wgrad_kernel != 1) or wgrad_kernel == 2 else "fp32"


# ---- slabs -------------------------------------------------------------------------------------------------------------------------
SLAB_CLASSES = ("one", "few", "x8_full", "x8_empty")


def slab_class(plan):
    """(R, slabs, rows per slab) -> one slab | fewer than 8 | a multiple of 8 (XCD map on) with every slab holding rows | with empty
    trailing slabs."""
    R, nslab, rps = plan
    assert nslab >= 1 and rps % 16 == 0 and nslab * rps >= R, plan
    if nslab == 1:
        return "one"
    if nslab < 8:
        assert (nslab - 1) * rps < R, plan
        return "few"
    assert nslab % 8 == 0, plan
    return "x8_empty" if (nslab - 1) * rps >= R else "x8_full"


def slab_edges(plan):
    """Row edges of a plan that a run picks windows around: two interior slab starts and the start of the last slab that holds rows."""
    R, nslab, rps = plan
    live = (R + rps - 1) // rps                                  # slabs that hold rows
    return sorted({s * rps for s in (1, live // 2, live - 1) if 0 < s < live})


def site_plans(c, chunk):
    """[(site kind, (R, slabs, rows per slab))] of one chunk of a case, from its hand-written entries."""
    rows = chunk["rows"]
    out = [("conv", rows), ("ih", rows), ("hh", rows), ("rec_fc", rows), ("fc", chunk["fc"])]
    if SHAPES[c["shape"]]["use_gatv2"]:
        out += [("gat_lin", chunk["feat"]), ("gat_lin", rows)]     # the feature projection (n F rows), the temporal one (n W rows)
    return out


SITE_KINDS = ("conv", "gat_lin", "ih", "hh", "rec_fc", "fc")
# (site kind, arithmetic, slab class) no supported configuration reaches, with the reason
UNREACHABLE_SLABS = {
    ("fc", a, "x8_empty"): "R = n <= TRAIN_CHUNK = 8192 rows give at most 16 slabs of more than 384 rows each; rounding them up to 16 "
                           "rows adds at most 15 x 15 rows in front of the last slab (tests/test_host_train_route_cases.py walks every n)"
    for a in ("x3", "fp32")}
SLAB_LEDGER = [(k, a, s) for k in SITE_KINDS for a in ("x3", "fp32") for s in SLAB_CLASSES if (k, a, s) not in UNREACHABLE_SLABS]
assert len(SLAB_LEDGER) == 46

# (training forward, backward, x3) of a recurrence layer under the default "gru_kernel" option
RECURRENCE_LEDGER = ["gru1>gru1_bwd", "gru16>gru16_bwd", "split>gru_bwd", "split>gru_bwd:x3", "splitx3>gru_bwd:x3"]
UNREACHABLE_RECURRENCES = {
    "splitx3>gru_bwd": "k_gru_split takes split operands only in mode fp32, where k_gru_bwd multiplies on three bf16 pieces",
    "gru1>gru1_bwd:x3": "x3 is a build of k_gru_bwd alone", "gru16>gru16_bwd:x3": "x3 is a build of k_gru_bwd alone",
    "cm / tile": "the chunk-major and tile-major kernels keep no gates: a training forward never takes them",
}
FC_LEDGER = ["fc:in", "fc:row"]
ATTENTION_LEDGER = ["fused:v2", "fused:v1", "wide:v2", "wide:v1"]


def ledger_of(runs):
    """(slab triples, recurrence pairs, fc, attention) the given (case, mode, wgrad_kernel) runs reach, from the hand-written entries."""
    slabs, recs, fcs, atts = set(), set(), set(), set()
    for c, mode, wk in runs:
        a = arithmetic(mode, wk)
        atts.add(ATTENTION[c["shape"]])
        for ch in c["chunks"]:
            for kind, plan in site_plans(c, ch):
                slabs.add((kind, a, slab_class(plan)))
            gru, rec, fc = [s.strip() for s in ch["route"][mode].split("|")]
            recs.update(s.strip() for s in (gru + ", " + rec).split(","))
            fcs.add(fc)
    return slabs, recs, fcs, atts


# ---- picked windows ----------------------------------------------------------------------------------------------------------------
def pick_edges(c):
    """(window edges, row edges) of a case: the chunk edge(s) of the Python step; per chunk the slab edges of the n W-row sites -- the
    convolution's and W_hh's (bshift) slabs are the same rows -- as GLOBAL rows."""
    W = SHAPES[c["shape"]]["window_size"]
    edges, rows, at = [], [], 0
    for ch in c["chunks"]:
        if at:
            edges.append(at)
        rows += [at * W + r for r in slab_edges(ch["rows"])]
        at += ch["n"]
    return edges, rows
