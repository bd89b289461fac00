"""Which kernels run the front end of a call -- window convolution, temporal and feature attention layer (front_route, queried
through mtadgat_front_route): pinned on both sides of every band edge, for the five call kinds, the four sources, the three precision
modes, every value of "conv_kernel", "gat_kernel", "conv_fused", "conv_shared" and "rowgemm_kernel" (the full product) and each pointer
fact (all true, each one false, all false).  No GPU needed.  Outputs pass their tolerances on every route, so a drifted predicate would otherwise be a silent slowdown or a
silently wrong pack.

The reference is not taken from front_route: the `_p_*` functions below transcribe the predicates of the commit before front_route
existed line by line -- split_front, conv_win_selected, run_conv, conv_shared_applies, run_proj, run_attend, run_gat_fused,
fused_conv_args, run_gat_layer and their callers forward_impl, mtadgat_conv, attention_impl and mtadgat_forward_train
(mtadgat_capi.cpp), conv_win_applies (mtadgat_convw.hip), gath_conv_applies (mtadgat_gath.hip), launch_conv's choice of kernel
(mtadgat_kernels.hip) and the plans they read (validate_and_plan).  Every expected entry is HAND-DERIVED in this way.

The shapes are those of test_host_gru_route.py; among them are GAT (v1) and GATv2 models, un-fused layers with K, D <= 512
(many_nodes, long_embedding), a layer above 512 and rows too long for the LDS-staged convolution (wide_features); "msl_v1" adds a GAT
(v1) model large enough for k_gath."""
import ctypes
import itertools

import pytest

from test_host_gru_route import PRECISIONS, SHAPES as GRU_SHAPES, _create

SHAPES = dict(GRU_SHAPES)
SHAPES["msl_v1"] = dict(SHAPES["msl"], use_gatv2=False)

KINDS = ("forward", "forward_unfused", "train", "attention", "conv")
SOURCES = ("windows", "windows_bf16", "series_unit", "series")
OPTIONS = {"conv_kernel": (0, 1, 2), "gat_kernel": (0, 1, 3), "conv_fused": (0, 1), "conv_shared": (0, 1), "rowgemm_kernel": (0, 1, 2)}


def _ru(v, m):
    return (v + m - 1) // m * m


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _sizes(F, W):
    """both sides of 1024 (shared rows), 4096, and of the counts where n * W (convolution rows, temporal projection rows) and n * F
    (feature projection rows) reach 65536"""
    s = {256, 1023, 1024, 4095, 4096}
    for k in (W, F):
        e = -(-65536 // k)
        s.update((max(1, e - 1), e))
    return sorted(s)


# ---- hand-derived reference: the plans and predicates of the commit before front_route, transcribed ---------------------------------
def _p_plan_gat(K, D, E, v2):
    """plan_gat of validate_and_plan (mtadgat_pack.cpp): what the predicates read (no measurement hook set in the environment)."""
    g = _Obj(K=K, D=D, E=E, fused=False, f_nw=0, fh_lr=0, fh_lds_bytes=0)
    ptcap = _ru(E, 8) + 8 if v2 else 0
    g.Q = (D + 7) // 8
    if K <= 128 and D <= 128:
        ibw = 16
        nwa = (K + ibw - 1) // ibw
        ntask = 2 * ((K + 31) // 32)
        nw = nwa
        if ntask > nwa:
            nw = min(8, max(nwa, min(ntask, _ru(nwa, 4))))
        rows = nwa * ibw
        qf = (D + 8) // 8
        vld = 8 * qf + 4
        lr = _ru(max((rows + K) * 34, rows * 68), 4)
        if (_ru(K, 16) * vld + lr) * 4 <= 80 * 1024:
            g.fused, g.f_nw, g.Q = True, nw, qf
            f_RJ = 8 if (K <= 56 and ((K + 7) // 8) % 2 == 1) else 16
    g.Q16 = (D + 1 + 15) // 16 if g.fused else 0
    if g.fused:
        shortrows = 16 - 64 // f_RJ
        best, bf, bs = 1 << 30, 0, 0
        for nf in range(g.f_nw + 1):
            for ns in range(g.f_nw - nf + 1):
                r = 16 * nf + shortrows * ns
                if r >= K and (r < best or (r == best and nf + ns < bf + bs)):
                    best, bf, bs = r, nf, ns
        fh_vld = (D + 1 + 3) & ~3
        if (fh_vld >> 2) % 2 == 0:
            fh_vld += 4
        fh_vld = min(fh_vld, 16 * g.Q16 + 4)
        orows = (bf + bs) * 16
        g.fh_lr = _ru(max((orows + K) * 34, orows * 36), 4)
        pieces = 2 * ((K + 1) * fh_vld + 16) * 2
        g.fh_lds_bytes = g.fh_lr * 4 + pieces
        buf = _ru((K + K) * 34, 4)
        total = 2 * buf * 4 + pieces

        def resident(b):
            return min(160 * 1024 // b, 16 // g.f_nw)
        if (g.f_nw == 8 and bf + bs <= 7 and g.Q16 <= 4 and ptcap >= 32 and orows * 36 <= 2 * buf and total <= 160 * 1024 and
                resident(total) == resident(g.fh_lds_bytes)):
            g.fh_lr, g.fh_lds_bytes = 2 * buf, total
    g.uQ16 = 0 if g.fused else (g.Q + 1) // 2
    g.uw3 = not g.fused                 # uw3_off: a region behind the convolution's, never offset 0; empty for fused layers
    return g


def _p_plans(cfg):
    F, W, taps = cfg["n_features"], cfg["window_size"], cfg["kernel_size"]
    v2 = bool(cfg["use_gatv2"])
    return _Obj(F=F, W=W, Fp=_ru(F, 8), Wp=_ru(W, 8), Dp=_ru(3 * F, 8), Fp16=_ru(F, 16), taps=taps, pad=(taps - 1) // 2, NT=(F + 31) // 32,
                v2=v2, feat=_p_plan_gat(F, W, cfg["feat_embed"], v2), temp=_p_plan_gat(W, F, cfg["time_embed"], v2))


def _staged(taps, Fq):
    return (32 + taps - 1) * (Fq + 4) * 4 <= 20 * 1024


def _p_split_front(m, o, n):
    return o.prec == 1 and n >= 4096 and o.conv_kernel == 0 and o.gat_kernel == 0


def _p_conv_win_selected(m, o, n):
    return (o.prec == 2 or _p_split_front(m, o, n)) and o.conv_kernel != 1 and (n >= 4096 or o.conv_kernel == 2)


def _conv_win_pitch(F, Fq):
    p = (F + 3) & ~3
    if (p >> 2) % 2 == 0:
        p += 4
    while 2 * p < Fq:
        p += 8
    return p if p < Fq + 4 else Fq + 4


def _conv_win_lds(W, F, Fq, taps):
    return 2 * (W + taps + 1) * _conv_win_pitch(F, Fq) * 2 + 32


def _p_conv_win_applies(m, a):
    if a.bf16 or not a.HCAT or a.XC or a.XCT or a.Y or not a.wscale:
        return False
    if m.taps != 2 * m.pad + 1 or m.NT > 2 or a.W > 128 or a.W < 1:
        return False
    if a.W * m.F > 12 * 128 * 4 or (a.Fq & 15) != 0 or a.Fq < m.F:
        return False
    if (m.Dp & 3) != 0:
        return False
    return _conv_win_lds(a.W, m.F, a.Fq, m.taps) <= 64 * 1024


def _p_run_conv(m, o, src, n, xc, xct, hcat, y, vmax, geo_W=0):
    """-> (launcher, operands, reads the split pack, range recorded)"""
    Wk = geo_W or m.W
    x_bf16 = src == "windows_bf16"
    a = _Obj(W=Wk, Fq=m.Fp, bf16=0, XC=xc, XCT=xct, HCAT=hcat, Y=y, wscale=False, Wp3=False)
    if (o.prec == 1 and not xc and not xct and _staged(m.taps, m.Fp16) and
            not (_p_conv_win_selected(m, o, n) and not geo_W and hcat and not y)):
        a.bf16, a.Fq = 1, m.Fp16
    if _p_conv_win_selected(m, o, n) and not geo_W and hcat and not xc and not xct and not y:
        b = _Obj(**a.__dict__)
        b.Fq, b.wscale = m.Fp16, True
        if _p_conv_win_applies(m, b):
            return ("k_conv_win", "fp16", True, vmax)
    if (o.prec == 2 and not a.bf16 and not x_bf16 and o.conv_kernel != 1 and (n * Wk >= 65536 or o.conv_kernel == 2) and
            not _staged(m.taps, m.Fp)):
        a.Wp3, a.Fq = True, m.Fp16
    # launch_conv: LDS-staged where it fits (the 16-bit inputs need it), else straight from memory on fp32 or three bf16 pieces
    return ("launch_conv", "bf16" if a.bf16 else "x3" if a.Wp3 else "fp32", a.Wp3, vmax)


def _p_conv_shared_applies(m, o, src, n):
    if src != "series_unit" or n < 1024 or o.prec == 1:
        return False
    if _p_conv_win_selected(m, o, n) and o.conv_shared != 1:
        b = _Obj(W=m.W, Fq=m.Fp16, bf16=0, XC=False, XCT=False, HCAT=True, Y=False, wscale=True)
        if _p_conv_win_applies(m, b):
            return False
    if m.taps != 2 * m.pad + 1 or m.pad < 1 or m.W < 4 * m.pad:
        return False
    return _staged(m.taps, m.Fp)


def _p_run_proj(m, o, g, nrows):
    return o.prec == 2 and g.uw3 and g.uQ16 > 0 and o.rowgemm_kernel != 1 and (nrows >= 65536 or o.rowgemm_kernel == 2)


def _p_run_gat_fused(m, o, g, aligned_v, ldv_fits, n, att, vmax, cv):
    """-> (kernel, projection operands, k_gat holds the fp16 pack, split packs read) or "internal error" """
    bf16, Wp2, a_vmax = 0, False, False
    if o.prec == 1 and not att and not (_p_split_front(m, o, n) and vmax):
        bf16 = 1
    elif (o.prec == 2 or (_p_split_front(m, o, n) and not att)) and (n >= 4096 or (o.gat_kernel == 3 and not att)):
        bf16, Wp2, a_vmax = 2, True, vmax
    gath = False
    if (bf16 == 2 and vmax and (not att or n >= 4096) and o.gat_kernel in (0, 3) and g.fh_lds_bytes <= 160 * 1024 and aligned_v and
            ldv_fits):
        gath = True
    elif cv:
        return "internal error"
    elif m.v2:
        Wp2, a_vmax = False, False
    return ("k_gath+k_gat" if gath else "k_gat", ("fp32", "bf16", "x3")[bf16], Wp2, False, bf16 == 2)


def _p_gath_conv_applies(m, g, cv):
    if g.K != m.W or g.D != m.F or g.f_nw != 8:
        return False
    if m.taps != 2 * m.pad + 1 or m.NT > 2 or m.NT < 1 or m.W > 128 or m.W < 1 or m.W * m.F > 6144:
        return False
    if (m.Fp16 & 15) != 0 or m.Fp16 < m.F or (m.Dp & 3) != 0 or 32 * m.NT < m.F:
        return False
    return _conv_win_lds(m.W, m.F, m.Fp16, m.taps) + 24 * 4 <= g.fh_lr * 4


def _p_fused_conv_args(m, o, n, aligned_hcat):
    g = m.temp
    if (o.conv_fused == 1 or not (o.prec == 2 or _p_split_front(m, o, n)) or not _p_conv_win_selected(m, o, n) or not g.fused or
            not m.feat.fused):
        return False
    if not (n >= 4096 or o.gat_kernel == 3) or o.gat_kernel not in (0, 3) or g.fh_lds_bytes > 160 * 1024:
        return False
    if g.K != m.W or g.D != m.F or not aligned_hcat or (m.Dp & 3) != 0 or ((g.D + 3) & ~3) > m.Dp:
        return False
    return _p_gath_conv_applies(m, g, True)


def _p_layer(m, o, g, aligned_v, ldv_fits, nrows, n, att, vmax, cv=False):
    """run_gat_layer and the hand-written copies of it in attention_impl / mtadgat_forward_train"""
    if g.fused:
        return _p_run_gat_fused(m, o, g, aligned_v, ldv_fits, n, att, vmax, cv)
    x3 = _p_run_proj(m, o, g, nrows)
    return ("rowgemm+k_gat_wide" if (g.K <= 512 and g.D <= 512) else "rowgemm+k_attend", "x3" if x3 else "fp32", False, x3, x3)


_NO_LAYER = ("none", "fp32", False, False, False)


def _p_call(m, o, kind, src, n, facts):
    """-> (convolution, temporal layer, feature layer) as the callers of that commit launched them"""
    aligned_v, ldv_fits, aligned_hcat = facts
    F, W = m.F, m.W
    if kind == "conv":                                       # mtadgat_conv
        return _p_run_conv(m, o, src, n, False, False, False, True, False), _NO_LAYER, _NO_LAYER
    if kind == "forward" and m.temp.fused and m.feat.fused:  # forward_impl, fused front
        cv = False
        if _p_conv_shared_applies(m, o, src, n):
            three = [_p_run_conv(m, o, "series_unit", k, True, False, False, False, True, geo) for k, geo in ((1, n + W - 1), (n, 2 * m.pad), (n, 2 * m.pad))]
            assert three == [("launch_conv", "fp32", False, True)] * 3
            conv = ("shared_rows", "fp32", False, True)
        elif _p_fused_conv_args(m, o, n, aligned_hcat):
            cv = True
            conv = ("in_gath", "fp16", True, True)           # (cv.Wp is the two-fp16-piece pack; vmax zeroed by the caller)
        else:
            conv = _p_run_conv(m, o, src, n, False, False, True, False, True)
        temp = _p_run_gat_fused(m, o, m.temp, aligned_v, ldv_fits, n, False, True, cv)
        feat = _p_run_gat_fused(m, o, m.feat, aligned_v, ldv_fits, n, False, True, False)
        return conv, temp, feat
    if kind in ("forward", "forward_unfused"):               # forward_impl, un-fused front (and mtadgat_gat: the same layer calls)
        conv = _p_run_conv(m, o, src, n, True, True, True, False, False)
        return conv, _p_layer(m, o, m.temp, aligned_v, ldv_fits, n * W, n, False, False), _p_layer(m, o, m.feat, aligned_v, ldv_fits, n * F, n, False, False)
    if kind == "attention":                                  # attention_impl (both maps wanted): precision 0 for the call
        o = _Obj(**dict(o.__dict__, prec=0))
        conv = _p_run_conv(m, o, src, n, False, not m.feat.fused, True, False, False)
        return conv, _p_layer(m, o, m.temp, aligned_v, ldv_fits, n * W, n, True, False), _p_layer(m, o, m.feat, aligned_v, ldv_fits, n * F, n, True, False)
    assert kind == "train"                                   # mtadgat_forward_train
    conv = _p_run_conv(m, o, src, n, False, True, True, False, True)
    return conv, _p_layer(m, o, m.temp, aligned_v, ldv_fits, n * W, n, True, True), _p_layer(m, o, m.feat, aligned_v, ldv_fits, n * F, n, True, True)


def _p_rowgemm_split(prec, rk, has_pack, rows, site):
    """the four spellings of that commit: run_proj / lin_split_operands (forward), run_rowgemm_T / run_bwd_projection (backward)"""
    if site == "run_proj" or site == "lin_split_operands":
        return prec == 2 and has_pack and rk != 1 and (rows >= 65536 or rk == 2)
    return has_pack and ((prec == 2 and rk != 1 and rows >= 65536) or rk == 2)


# ---- the library's answer ------------------------------------------------------------------------------------------------------------
_BUF = (ctypes.c_int * 14)()


def _route(lib, h, kind, src, n, facts):
    import _native
    bits = facts[0] + 2 * facts[1] + 4 * facts[2]
    assert lib.mtadgat_front_route(h, KINDS.index(kind), SOURCES.index(src), n, bits, _BUF) == 0, lib.mtadgat_last_error()
    return dict(zip(_native.FRONT_ROUTE_FIELDS, _BUF))


def _describe(r):
    import _native
    conv = _native.FRONT_CONVS[r["conv"]]
    build = "fp16" if conv in ("in_gath", "k_conv_win") else _native.FRONT_BUILDS[r["conv_build"]]

    def layer(p):
        return (_native.FRONT_LAYERS[r[p + "_kernel"]], _native.FRONT_BUILDS[r[p + "_build"]], bool(r[p + "_fp16"]), bool(r[p + "_split_gemm"]),
                bool(r[p + "_split_pack"]))
    return (conv, build, bool(r["conv_split_pack"]), bool(r["range"])), layer("temp"), layer("feat")


@pytest.mark.parametrize("name", list(SHAPES))
def test_routes_equal_the_hand_derived_predicates(name):
    lib, cfg, h = _create(SHAPES[name])
    m = _p_plans(cfg)
    v2 = bool(cfg["use_gatv2"])
    sizes = _sizes(m.F, m.W)
    facts_all = [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)]
    seen = set()
    try:
        for prec in PRECISIONS.values():
            assert lib.mtadgat_set_precision(h, prec) == 0
            for values in itertools.product(*OPTIONS.values()):
                for key, v in zip(OPTIONS, values):
                    assert lib.mtadgat_set_option(h, key.encode(), v) == 0
                o = _Obj(prec=prec, **dict(zip(OPTIONS, values)))
                for kind, src, n, facts in itertools.product(KINDS, SOURCES, sizes, facts_all):
                    r = _route(lib, h, kind, src, n, facts)
                    got = _describe(r)
                    want = _p_call(m, o, kind, src, n, facts)
                    what = (name, prec, values, kind, src, n, facts)
                    seen.add(got[0][0])
                    # consistency, without the reference
                    if r["conv"] == 0:
                        assert r["temp_kernel"] == 2 and kind == "forward", (what, r)        # convolution: none => inside k_gath
                    for p in ("temp", "feat"):
                        assert not (v2 and r[p + "_kernel"] != 2 and r[p + "_fp16"]), (what, r)  # GATv2 without k_gath: never the fp16 pack
                        if r[p + "_build"] == 2 or r[p + "_fp16"] or r[p + "_split_gemm"]:
                            assert r[p + "_split_pack"], (what, r)                           # a named split pack is marked needed
                    if r["conv"] in (0, 1) or r["conv_build"] == 2:
                        assert r["conv_split_pack"], (what, r)
                    if want[1] == "internal error":
                        # the commit before handed k_gath's convolution to a run_gat_fused that refused k_gath when the node rows
                        # failed a pointer fact h_cat passed (its callers pass h_cat as both, so it never happened): the route has
                        # one copy of k_gath's conditions and keeps the convolution launch
                        assert facts[2] and not (facts[0] and facts[1]) and r["conv"] != 0, (what, r)
                        continue
                    assert got == want, (what, r)                                            # hand-derived
        if name in ("msl", "msl_v1"):
            assert seen == {"in_gath", "k_conv_win", "shared_rows", "launch_conv"}, seen
    finally:
        lib.mtadgat_set_precision(h, 0)
        for key in OPTIONS:
            lib.mtadgat_set_option(h, key.encode(), 0)
        lib.mtadgat_destroy(h)


def test_rowgemm_split_forward_and_backward_sites():
    """rowgemm_split against the four spellings it replaced, the forward / backward difference included: "rowgemm_kernel" = 2 forces
    the split pack in the backward whatever the precision mode, in the forward only in mode 2."""
    lib, cfg, h = _create(SHAPES["msl"])
    try:
        for prec, rk in itertools.product((0, 1, 2), (0, 1, 2)):
            assert lib.mtadgat_set_precision(h, prec) == 0 and lib.mtadgat_set_option(h, b"rowgemm_kernel", rk) == 0
            for has_pack, rows in itertools.product((False, True), (1, 65535, 65536, 1 << 20)):
                fwd, bwd = lib.mtadgat_rowgemm_split(h, has_pack, rows, 0), lib.mtadgat_rowgemm_split(h, has_pack, rows, 1)
                for site in ("run_proj", "lin_split_operands"):
                    assert fwd == _p_rowgemm_split(prec, rk, has_pack, rows, site), (prec, rk, has_pack, rows, site)
                for site in ("run_rowgemm_T", "run_bwd_projection"):
                    assert bwd == _p_rowgemm_split(prec, rk, has_pack, rows, site), (prec, rk, has_pack, rows, site)
                if prec != 2 and rk == 2 and has_pack:
                    assert bwd == 1 and fwd == 0                                     # the difference, kept as it was
    finally:
        lib.mtadgat_set_precision(h, 0)
        lib.mtadgat_set_option(h, b"rowgemm_kernel", 0)
        lib.mtadgat_destroy(h)


def test_hook_rejects_bad_arguments_and_needs_no_weights():
    lib, cfg, h = _create(SHAPES["msl"])
    try:
        buf = (ctypes.c_int * 14)()
        assert lib.mtadgat_front_route(h, 0, 0, 256, 7, buf) == 0             # no weights loaded, no GPU touched
        for bad in ((-1, 0, 256, 7), (5, 0, 256, 7), (0, 4, 256, 7), (0, -1, 256, 7), (0, 0, 0, 7), (0, 0, 256, 8), (0, 0, 256, -1)):
            assert lib.mtadgat_front_route(h, *bad, buf) != 0, bad
        assert lib.mtadgat_front_route(h, 0, 0, 256, 7, None) != 0
    finally:
        lib.mtadgat_destroy(h)
