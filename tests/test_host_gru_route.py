"""Which recurrence kernels a GRU / decoder layer gets (gru_route, queried through mtadgat_gru_route on 256 compute units): pinned on
both sides of every band edge, for inference and training, in the three precision modes and under every "gru_kernel" value.  No GPU
needed.  Outputs pass their tolerances on every route, so a shifted threshold would otherwise be a silent slowdown.

The reference is not taken from gru_route: `_parent_layer` / `_parent_use_g16` below transcribe the predicates of the commit before
gru_route existed (run_gru_layer's cm_fit / use_sp / use_cm / sp_train / x3, use_g16, split_kernels_fit, launch_gru's choice and the
callers' buffer decisions) line by line.  Every expected entry is HAND-DERIVED in this way: no kernel trace of that commit is on record
for these cases (the table a trace would give has the same form: the launches `_describe` names, per call)."""
import ctypes

import pytest

from helpers import Case
from test_host_derived_regions import SHAPES as REGION_SHAPES

CU = 256
SIZES = [1024, 1025, 1792, 1793, 2560, 2561, 4096, 4097, 8192, 8193, 10240, 10272, 16384, 16385, 16416]
PRECISIONS = {"fp32": 2, "fp32_strict": 0, "bf16": 1}            # mtadgat_set_precision modes


def _shapes():
    s = dict(REGION_SHAPES)
    s["msl"] = Case("msl").kwargs
    s["smd_1_1"] = Case("smd_1_1").kwargs
    return s


SHAPES = _shapes()


def _create(kw):
    import _native
    from mtad_gat import MTAD_GAT
    lib = _native.load_library()
    model = MTAD_GAT(**kw)
    h = ctypes.c_void_p()
    assert lib.mtadgat_create(ctypes.byref(_native.Config(**model._native_cfg)), ctypes.byref(h)) == 0, lib.mtadgat_last_error()
    return lib, model._native_cfg, h


def _route(lib, h, stack, layer, n, training):
    import _native
    buf = (ctypes.c_int * 8)(*([-7] * 8))
    assert lib.mtadgat_gru_route(h, stack, layer, n, int(training), CU, buf) == 0, lib.mtadgat_last_error()
    return dict(zip(_native.GRU_ROUTE_FIELDS, buf))


def _describe(r):
    """The launches of a route as the trace names them: kernel, operand build, hoisted input (xp), two groups per wave (2), Linear inside (fc)."""
    builds = ("fp32", "bf16", "x3_hi", "x3_lo")
    fc = ":fc" if r["fc_rides"] else ""

    def one(k):
        if k == 1:
            return "gru1"
        if k == 2:
            return "gru16"
        if k == 3:
            return "split:" + builds[r["build"]] + (":xp" if r["hoist"] else "") + fc
        if k == 4:
            return "splitx3" + fc
        if k == 5:
            return "cm" + fc
        assert k == 6, k
        return "tile:" + builds[r["build"]] + (":2" if r["two"] else "") + fc
    return [one(r["first"])] + ([one(r["fallback"])] if r["fallback"] else [])


# ---- hand-derived reference: the plans and predicates of the commit before gru_route, transcribed -----------------------------------
def _ru(v, m):
    return (v + m - 1) // m * m


class _Plan:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _parent_plans(cfg):
    """validate_and_plan's recurrence plans (mtadgat_pack.cpp): what the predicates read."""
    F, W = cfg["n_features"], cfg["window_size"]
    Hg, Hr = cfg["gru_hid_dim"], cfg["recon_hid_dim"]
    gru, rec = [], []
    for l in range(cfg["gru_n_layers"]):
        Qx = ((3 * F if l == 0 else Hg) + 7) // 8
        Qxp16 = _ru((Qx + 1) // 2, 6)
        gru.append(_Plan(xmode=0, H=Hg, NCG=_ru(Hg, 32) // 32, Qx=Qx, Qxp16=Qxp16, qb3=min(Qxp16, _ru((F + 15) // 16, 2)) if l == 0 else 0,
                         wx2=l == 0, wxq=True, has_xproj=l == 0, has16=l == 0 and _ru(Hg, 16) <= 160))
    for l in range(cfg["recon_n_layers"]):
        if l == 0:
            nm = max((t * Hg + Hg - 1) // W - (t * Hg) // W + 1 for t in range(W))
            Qx = (nm + 7) // 8
            Qxp16 = 1 if Qx == 1 else _ru((Qx + 1) // 2, 6)
            rec.append(_Plan(xmode=1, H=Hr, NCG=_ru(Hr, 32) // 32, Qx=Qx, Qxp16=Qxp16, qb3=0, wx2=False, wxq=False, has_xproj=False,
                             has16=_ru(Hr, 16) <= 160 and Qx == 1))
        else:
            Qx = (Hr + 7) // 8
            rec.append(_Plan(xmode=0, H=Hr, NCG=_ru(Hr, 32) // 32, Qx=Qx, Qxp16=_ru((Qx + 1) // 2, 6), qb3=0, wx2=False, wxq=True,
                             has_xproj=False, has16=False))
    # both attention layers fused: up to 128 nodes and node dimensions (these shapes fit the fused kernel's LDS, as in
    # test_host_derived_regions._expected_regions)
    fused = F <= 128 and W <= 128
    return _Plan(W=W, out_dim=cfg["out_dim"], gru=gru, rec=rec, fused=fused)


def _cm_supported(ncg, xmode, fc, out_dim):
    return 2 <= ncg <= 5 and xmode in (0, 1) and not (fc and (xmode != 1 or out_dim > 4))


def _parent_split_kernels_fit(m, g):
    if m.W > 512 or not (g.Qxp16 == 1 or g.Qxp16 % 2 == 0):
        return False
    if g.xmode == 1:
        return g.Qxp16 == 1 and _cm_supported(g.NCG, 1, False, 0)
    return _cm_supported(g.NCG, 0, False, 0) and g.wxq and g.Qx >= 3 and ((m.fused and g.wx2 and g.qb3 > 0) or g.qb3 == 0)


def _parent_use_g16(m, stack, n, training, prec, gk):
    if len(stack) != 1 or not stack[0].has16:
        return False
    if prec == 1:
        return not training and n <= 1024
    if prec == 2 and not training and stack[0].NCG >= 2 and _parent_split_kernels_fit(m, stack[0]) and (gk == 3 or (gk == 0 and n >= 2561)):
        return False
    return n <= 4096


def _parent_layer(m, g, n, prec, gk, g16, xp, vmax, gates, fc_out):
    """run_gru_layer (mtadgat_capi.cpp) and launch_gru (mtadgat_gru.hip) of that commit; hend == nullptr || ldhe >= Hp holds in forward()."""
    if g16:
        return ["gru1" if n <= 1792 else "gru16"]
    fc = fc_out is not None
    fcs = ":fc" if fc else ""
    lds = (g.NCG * 1024 + (g.NCG * fc_out * 32 if fc else 0)) * 4
    par2 = g.Qxp16 == 1 or g.Qxp16 % 2 == 0
    range_ok = (vmax and g.wx2 and g.qb3 > 0) or g.qb3 == 0
    cm_fit = (prec == 2 and not gates and _cm_supported(g.NCG, g.xmode, fc, fc_out if fc else 0) and par2 and
              ((g.Qxp16 == 1) if g.xmode == 1 else (g.wxq and g.Qx >= 3 and range_ok)) and m.W <= 512)
    use_sp = cm_fit and g.NCG >= 2 and (gk == 3 or (gk == 0 and 2561 <= n <= 8192))
    use_cm = cm_fit and not use_sp and gk != 1 and gk != 3 and (gk == 2 or n >= 4097)
    sp_train = (gates and prec == 2 and g.NCG >= 2 and gk != 1 and n >= 2561 and (g.Qxp16 == 1 or g.Qxp16 % 6 == 0) and
                ((g.Qxp16 == 1) if g.xmode == 1 else range_ok) and lds <= 64 * 1024)
    groups = (n + 31) // 32
    x3 = prec == 2 and not gates and (groups > 5 * CU // 4 or use_cm or use_sp) and par2
    if sp_train:
        xp = False
    xmode = 3 if (not x3 and xp and g.has_xproj and g.xmode == 0) else g.xmode
    plain = "split:" + ("bf16" if prec == 1 else "fp32") + (":xp" if xmode == 3 else "") + fcs
    if gates:
        if sp_train:
            return ["splitx3" + fcs] + ([plain] if (xmode == 0 and g.qb3 > 0) else [])
        return [plain]
    out = []
    a_vmax = x3 and vmax and g.wx2 and g.qb3 > 0
    if use_sp:
        if lds <= 64 * 1024:
            out.append("splitx3" + fcs)
            if not a_vmax:
                return out
    elif use_cm:
        out.append("cm" + fcs)
        if not a_vmax:
            return out
    if xmode == 3 or (not x3 and g.NCG >= 2 and groups <= 2 * CU and lds <= 64 * 1024):
        return out + [plain]
    build = ("x3_hi" if g.NCG >= 5 else "x3_lo") if x3 else ("bf16" if prec == 1 else "fp32")
    return out + ["tile:" + build + (":2" if groups >= 8 * CU else "") + fcs]


def _parent_call(m, n, training, prec, gk):
    """{(stack, layer): launches} of forward() (predictions and reconstructions wanted, one piece of n windows with its own workspace
    plan) / of the training forward, as run_gru_stack, run_heads and mtadgat_forward_train called run_gru_layer."""
    out = {}
    has_xp = m.gru[0].has_xproj and n <= 16384                       # plan_workspace
    rec16 = len(m.rec) == 1 and m.rec[0].has16 and n <= 4096
    g16_g = _parent_use_g16(m, m.gru, n, training, prec, gk)
    g16_r = _parent_use_g16(m, m.rec, n, training, prec, gk)
    for l, g in enumerate(m.gru):
        if training:
            out[0, l] = _parent_layer(m, g, n, prec, gk, l == 0 and g16_g, l == 0, l == 0, True, None)
        else:
            g16 = g16_g and has_xp
            xp = l == 0 and has_xp and (g16 or n <= 64 * CU)
            out[0, l] = _parent_layer(m, g, n, prec, gk, g16, xp, l == 0 and m.fused, False, None)
    Ld = len(m.rec)
    if training:
        if Ld == 1 and g16_r:
            out[1, 0] = _parent_layer(m, m.rec[0], n, prec, gk, True, True, False, True, None)
        else:
            fc_rides = (m.rec[-1].NCG * 1024 + m.rec[-1].NCG * m.out_dim * 32) * 4 <= 64 * 1024
            for l, g in enumerate(m.rec):
                out[1, l] = _parent_layer(m, g, n, prec, gk, False, False, False, True, m.out_dim if (l == Ld - 1 and fc_rides) else None)
    elif g16_r and rec16:
        out[1, 0] = _parent_layer(m, m.rec[0], n, prec, gk, True, True, False, False, None)
    else:
        for l, g in enumerate(m.rec):
            out[1, l] = _parent_layer(m, g, n, prec, gk, False, False, False, False, m.out_dim if (l == Ld - 1 and m.out_dim <= 4) else None)
    return out, g16_g, g16_r


def _cases():
    for prec in PRECISIONS:
        for training in (False, True):
            for gk in (0, 1, 2, 3):
                yield prec, training, gk


@pytest.mark.parametrize("name", list(SHAPES))
def test_routes_equal_the_hand_derived_predicates(name):
    lib, cfg, h = _create(SHAPES[name])
    m = _parent_plans(cfg)
    try:
        for prec, training, gk in _cases():
            assert lib.mtadgat_set_precision(h, PRECISIONS[prec]) == 0
            assert lib.mtadgat_set_option(h, b"gru_kernel", gk) == 0
            for n in SIZES:
                want, small_g, small_r = _parent_call(m, n, training, PRECISIONS[prec], gk)
                for (stack, layer), launches in want.items():
                    r = _route(lib, h, stack, layer, n, training)
                    what = (name, prec, "train" if training else "infer", gk, n, stack, layer)
                    assert _describe(r) == launches, (what, r)                                   # hand-derived
                    # consistency: the stack-level answer is "layer 0's route is a small-batch kernel"; the split-operand and
                    # chunk-major kernels never run without their packs
                    assert r["small_stack"] == (small_r if stack else small_g), what
                    if layer == 0 and (stack == 1 or n <= 16384):        # (GRU layer 0 above 16 384 windows has no buffer for the hoisted products)
                        assert r["small_stack"] == (r["first"] in (1, 2)), (what, r)
                    elif layer > 0:
                        assert r["first"] not in (1, 2), (what, r)
                    if r["first"] in (4, 5) or r["build"] in (2, 3):
                        assert r["split_packs"], (what, r)
                    if r["first"] in (1, 2):
                        assert r["hoist"] and not r["fallback"] and not r["fc_rides"], (what, r)
    finally:
        lib.mtadgat_set_option(h, b"gru_kernel", 0)
        lib.mtadgat_destroy(h)


def test_hook_rejects_bad_arguments_and_needs_no_weights():
    lib, cfg, h = _create(SHAPES["msl"])
    try:
        buf = (ctypes.c_int * 8)()
        assert lib.mtadgat_gru_route(h, 0, 0, 256, 0, CU, buf) == 0           # no weights loaded, no GPU touched
        for bad in ((2, 0, 256, CU), (0, cfg["gru_n_layers"], 256, CU), (1, -1, 256, CU), (0, 0, 0, CU), (0, 0, 256, 0)):
            assert lib.mtadgat_gru_route(h, bad[0], bad[1], bad[2], 0, bad[3], buf) != 0, bad
        assert lib.mtadgat_gru_route(h, 0, 0, 256, 0, CU, None) != 0
    finally:
        lib.mtadgat_destroy(h)
