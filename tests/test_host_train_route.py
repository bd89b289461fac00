"""Which kernels a training step runs (mtadgat_train_route): per recurrence layer the training forward's first kernel and the
backward's kernel -- gru_bwd_route derives the second from the first, whose tape it reads --, whether the decoder's per-step Linear
rides in the recurrence, and per attention layer which backward runs.  Pinned on both sides of the k_gru1 / k_gru16 edge (1792 | 1793)
and the k_gru16 / k_gru_split edge (4096 | 4097), in the two fp32 precision modes and under "gru_kernel" 0, 1 and 3.  No GPU needed.

The reference is not taken from gru_bwd_route: `_parent_step` transcribes what the commit before it did -- backward_impl's layer_bwd
(gru_stack_small, then `n <= G1_MAX_WINDOWS` inline, then `precision == 2 && whT3_off` for the three-piece build; whT3 is planned for
every layer), its `gb.wide` / `use_gatv2` branches, and mtadgat_forward_train's small-decoder branch and rec_fc_rides_train."""
import ctypes

import pytest

from test_gpu_backward import CONFIGS as BACKWARD_CONFIGS
from test_host_forward_plan import _golden
from test_host_gru_route import _create, _parent_plans

SIZES = [1, 1792, 1793, 4096, 4097, 8193]
PRECISIONS = {"fp32": 2, "fp32_strict": 0}
GRU_KERNEL_OPTIONS = (0, 1, 3)
INVALID, UNSUPPORTED = -1, -2                     # MTADGAT_ERR_INVALID, MTADGAT_ERR_UNSUPPORTED
WINDOW, GROUP16, SPLIT = 0, 1, 2                     # GruBwdKernel
PARTNER = {1: WINDOW, 2: GROUP16, 3: SPLIT, 4: SPLIT}   # forward kernel (GruKernel) -> the backward that reads its tape


def _shapes():
    """The golden shapes with a HIP backward, and a wide GAT (v1) model, which they lack."""
    rec = _golden()
    s = {name: r["kwargs"] for name, r in rec["shapes"].items() if r["backward_supported"] == 1}
    s["v1_wide_w160"] = {k: v for k, v in BACKWARD_CONFIGS["v1_wide_w160"][0].items() if k != "dropout"}
    return s


SHAPES = _shapes()


def _train_route(lib, h, cfg, n):
    cap = 3 * (cfg["gru_n_layers"] + cfg["recon_n_layers"]) + 5
    buf = (ctypes.c_int * (cap + 1))(*([-7] * (cap + 1)))
    assert lib.mtadgat_train_route(h, n, buf, cap) == cap, lib.mtadgat_last_error()
    assert buf[cap] == -7
    v = list(buf[:cap])
    layers = [tuple(v[3 * i:3 * i + 3]) for i in range(cap // 3 - 1)]
    return dict(gru=layers[:cfg["gru_n_layers"]], rec=layers[cfg["gru_n_layers"]:], rec_fc_rides=v[-5], feat=tuple(v[-4:-2]), temp=tuple(v[-2:]))


def _parent_step(m, cfg, n, prec):
    """(backward kernel, x3) per layer of the two stacks, rec_fc_rides, (wide, v1) of an attention layer, as the parent decided them."""
    def stack_small(stack):                              # gru_stack_small(m, stack, n, training = true), precision 0 or 2
        return len(stack) == 1 and stack[0].has16 and n <= 4096

    def layers(stack):
        if stack_small(stack):
            return [(WINDOW if n <= 1792 else GROUP16, 0)]
        return [(SPLIT, int(prec == 2)) for _ in stack]

    top = m.rec[-1]
    lds_rule = (top.NCG * 1024 + top.NCG * m.out_dim * 32) * 4 <= 64 * 1024      # rec_fc_rides_train
    gat = (int(not m.fused), int(not cfg["use_gatv2"]))
    return layers(m.gru), layers(m.rec), int(not stack_small(m.rec) and lds_rule), gat


def test_the_shapes_cover_what_the_routes_branch_on():
    kinds = set()
    for kw in SHAPES.values():
        wide = kw["n_features"] > 128 or kw["window_size"] > 128
        kinds.add(("wide" if wide else "fused", "v2" if kw.get("use_gatv2", True) else "v1"))
        if kw.get("gru_n_layers", 1) == 2 and kw.get("recon_n_layers", 1) == 2:
            kinds.add("stacked")
    assert kinds >= {("fused", "v2"), ("fused", "v1"), ("wide", "v2"), ("wide", "v1"), "stacked"}, kinds


@pytest.mark.parametrize("name", list(SHAPES))
def test_train_route_equals_the_parent_predicates(name):
    lib, cfg, h = _create(SHAPES[name])
    m = _parent_plans(cfg)
    try:
        for prec in PRECISIONS.values():
            assert lib.mtadgat_set_precision(h, prec) == 0
            for gk in GRU_KERNEL_OPTIONS:
                assert lib.mtadgat_set_option(h, b"gru_kernel", gk) == 0
                for n in SIZES:
                    what = (name, prec, gk, n)
                    r = _train_route(lib, h, cfg, n)
                    gru, rec, rides, gat = _parent_step(m, cfg, n, prec)
                    assert [l[1:] for l in r["gru"]] == gru, (what, r)
                    assert [l[1:] for l in r["rec"]] == rec, (what, r)
                    assert r["rec_fc_rides"] == rides, (what, r)
                    assert r["feat"] == gat and r["temp"] == gat, (what, r)
                    # the forward kernel is the one mtadgat_gru_route reports for the training forward, and the backward is its partner
                    for stack, layers in ((0, r["gru"]), (1, r["rec"])):
                        for layer, (fwd, bwd, x3) in enumerate(layers):
                            buf = (ctypes.c_int * 8)()
                            assert lib.mtadgat_gru_route(h, stack, layer, n, 1, 256, buf) == 0
                            assert fwd == buf[0] and PARTNER[fwd] == bwd, (what, stack, layer, r)
                            assert x3 in (0, 1) and not (x3 and bwd != SPLIT), (what, stack, layer, r)
    finally:
        lib.mtadgat_set_option(h, b"gru_kernel", 0)
        lib.mtadgat_destroy(h)


def test_hook_rejects_bad_arguments_and_needs_no_weights():
    lib, cfg, h = _create(SHAPES["stacked"])
    cap = 3 * (cfg["gru_n_layers"] + cfg["recon_n_layers"]) + 5
    try:
        buf = (ctypes.c_int * cap)()
        assert lib.mtadgat_train_route(h, 256, buf, cap) == cap               # no weights loaded, no GPU touched
        assert lib.mtadgat_train_route(None, 256, buf, cap) == INVALID
        assert lib.mtadgat_train_route(h, 256, None, cap) == INVALID
        assert lib.mtadgat_train_route(h, 0, buf, cap) == INVALID and lib.mtadgat_train_route(h, -3, buf, cap) == INVALID
        untouched = (ctypes.c_int * cap)(*([-7] * cap))
        assert lib.mtadgat_train_route(h, 256, untouched, cap - 1) == INVALID and lib.mtadgat_train_route(h, 256, untouched, 0) == INVALID
        assert list(untouched) == [-7] * cap
    finally:
        lib.mtadgat_destroy(h)


def test_hook_answers_exactly_where_a_backward_exists():
    """MTADGAT_ERR_UNSUPPORTED goes with mtadgat_backward_supported() == 0, an answer with 1.  (Every configuration the planner accepts
    today has a HIP backward -- the fused layers' backward tiles stay below the LDS limit up to 128 nodes --, so the refusal itself
    cannot be provoked from here.)"""
    for name, kw in SHAPES.items():
        lib, cfg, h = _create(kw)
        cap = 3 * (cfg["gru_n_layers"] + cfg["recon_n_layers"]) + 5
        try:
            got = lib.mtadgat_train_route(h, 256, (ctypes.c_int * cap)(), cap)
            assert got == (cap if lib.mtadgat_backward_supported(h) == 1 else UNSUPPORTED), name
        finally:
            lib.mtadgat_destroy(h)
