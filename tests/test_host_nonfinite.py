"""The reference side of the non-finite contract, on the CPU (tests/nonfinite_cases.py; tests/test_gpu_nonfinite.py holds the HIP
path to it): the unmodified torch-op algebra (_torchpath.forward), in float64 (helpers.model64) and in float32, answers NaN in every
output element of exactly the windows `affected` names and leaves the other windows BIT-equal to the clean input's -- for every model
the case table uses, NaN / +inf / -inf at the four sample positions.  Also here: the table's own promises (neighbours clean, at
least half of every call clean, hand-written pieces and routes equal to the library's host answers) and `affected` against a brute
force.  No GPU needed.

The models, inputs and float64 references of the cases are built by the helpers at the top, for both test files."""
import copy
import ctypes

import pytest
import torch

import gru_route_cases as rc
import helpers
import nonfinite_cases as nf
import train_route_cases as tc

# ---- the models, inputs and float64 references of the cases (CPU), built once ------------------------------------------------------
_MODELS, _INPUTS, _REFS = {}, {}, {}
TRAIN_CASE = tc.CASES[0]                                         # the base shape at its smallest batch
assert TRAIN_CASE["shape"] == "base" and TRAIN_CASE["n"] == min(c["n"] for c in tc.CASES if c["shape"] == "base")


def model_kwargs(key):
    """MTAD_GAT kwargs of a model key: a case of tests/test_gpu_front_route.py, "wide" (tests/test_gpu_wide_features.py's smallest
    model above 512 features), a shape of tests/gru_route_cases.py, "stream" (tests/test_gpu_stream.py) or "train" / "train_v1"
    (tests/train_route_cases.py's base shape and its GAT (v1) twin)."""
    import test_gpu_front_route as fr
    import test_gpu_stream as ts
    import test_gpu_wide_features as wf
    if key in fr.CASES:
        return fr.CASES[key][0]
    if key == "wide":
        return wf.SHAPES[0][0]
    if key == "stream":
        return dict(n_features=ts.F, window_size=ts.W, out_dim=ts.F, kernel_size=3, gru_hid_dim=24, forecast_hid_dim=24, recon_hid_dim=24)
    if key in ("train", "train_v1"):
        return tc.SHAPES["base" if key == "train" else "v1"]
    return rc.SHAPES[key]


def case_options(c):
    import test_gpu_front_route as fr
    return dict(fr.CASES[c["model"]][1]) if c["options"] is None else dict(c["options"])


def base_model(key):
    """The CPU model of a key in eval mode, built as the test file it comes from builds it.  Cached: callers deep-copy it."""
    from mtad_gat import MTAD_GAT
    import test_gpu_front_route as fr
    if key not in _MODELS:
        if key in rc.SHAPES:
            from test_host_gru_route_cases import base_model as gru_model
            model = gru_model(key)
        elif key in ("train", "train_v1"):
            from test_host_train_route_cases import base_model as train_model
            model = train_model("base" if key == "train" else "v1")
        elif key == "wide":
            import test_gpu_wide_features as wf
            model = wf._model(model_kwargs(key))
        else:
            torch.manual_seed(9 if key == "stream" else 11)      # the seeds of tests/test_gpu_stream.py / test_gpu_front_route.py
            model = MTAD_GAT(**model_kwargs(key)).eval()
        _MODELS[key] = model
    return _MODELS[key]


def new_model(key):
    return copy.deepcopy(base_model(key))


def geometry(key):
    kw = model_kwargs(key)
    return kw["window_size"], kw["n_features"], (kw["kernel_size"] - 1) // 2


def clean_input(key, n, bf16=False):
    """x (n, W, F) ~ U[0, 1) under the fixed seed (bf16: rounded to bfloat16 values, still float32).  Cached: do not modify."""
    W, F, _ = geometry(key)
    k = (n, W, F, bf16)
    if k not in _INPUTS:
        x = torch.rand(n, W, F, generator=torch.Generator().manual_seed(nf.X_SEED))
        _INPUTS[k] = x.bfloat16().float() if bf16 else x
    return _INPUTS[k]


def poisoned(key, pieces, rot, bf16=False):
    """(x with the run's bad samples, x with nf.CLEAN_VALUE in their places, affected (n,) bool, the samples) of a windows case."""
    W, F, pad = geometry(key)
    n = sum(pieces)
    smp = nf.samples(pieces, W, F, pad, rot)
    bad, clean = clean_input(key, n, bf16).clone(), clean_input(key, n, bf16).clone()
    for w, t, f, v in smp:
        bad[w, t, f] = nf.VALUES[v]
        clean[w, t, f] = nf.CLEAN_VALUE
    mask = torch.tensor(nf.affected(n, W, [(w, t, f) for w, t, f, _ in smp], "windows"))
    return bad, clean, mask, smp


def torch_forward(model, x):
    """_torchpath.forward of the windows x in the model's dtype, a chunk of windows at a time -- the pair tensor of an attention layer
    is chunk * K * K * E values, held to 2^21 E --: (preds, recons)."""
    import _torchpath
    dt = next(model.parameters()).dtype
    K = max(x.shape[1], x.shape[2])
    chunk = max(1, min(4096, (1 << 21) // (K * K)))
    with torch.no_grad():
        outs = [_torchpath.forward(model, x[i:i + chunk].to(dt)) for i in range(0, x.shape[0], chunk)]
    return torch.cat([p for p, _ in outs]), torch.cat([r for _, r in outs])


def reference64(key, n, bf16=False):
    """(preds, recons) of the float64 model on the clean input of (key, n).  Computed once and left unchanged: the clean windows of
    every run of a case are the clean input's."""
    k = (key, n, bf16)
    if k not in _REFS:
        _REFS[k] = torch_forward(helpers.model64(base_model(key)), clean_input(key, n, bf16))
    return _REFS[k]


def window_nan(t):
    """(all, any) of isnan per window (dim 0) of an output tensor."""
    m = torch.isnan(t).flatten(1)
    return m.all(1).cpu(), m.any(1).cpu()


# ---- the reference does what the contract says ---------------------------------------------------------------------------------------
HOST_MODELS = ["conv_lds", "unfused", "wide", "A", "B", "stream", "train", "train_v1"]      # every model of the table, by shape


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("key", HOST_MODELS)
def test_the_torch_op_algebra_poisons_exactly_the_affected_windows(key, dtype):
    n = 4 if key == "wide" else 40                               # 40: the 16- and 32-window group edges lie inside (wide: two clean, two bad)
    model = new_model(key).to(dtype)
    for rot in range(3):
        bad, clean, mask, smp = poisoned(key, [n], rot)
        assert mask.sum() == len(smp) and 2 * mask.sum() <= n
        outs_bad, outs_clean = torch_forward(model, bad), torch_forward(model, clean)
        for name, a, b in zip(("preds", "recons"), outs_bad, outs_clean):
            every, some = window_nan(a)
            assert torch.equal(every, mask), (key, rot, name, "not every element of an affected window is NaN", smp)
            assert torch.equal(some, mask), (key, rot, name, "NaN outside the affected windows", smp)
            assert torch.equal(a[~mask], b[~mask]), (key, rot, name, "a clean window is not bit-equal to the clean input's")
            assert torch.isfinite(b).all()


# ---- the specification ---------------------------------------------------------------------------------------------------------------
def test_the_table_is_well_formed():
    assert len(set(nf.CASE_IDS)) == len(nf.CASES)
    for c in nf.CASES:
        n, pieces = c["n"], c["pieces"]
        assert sum(pieces) == n and c["mode"] in rc.MODES and c["source"] in ("windows", "windows_bf16")
        bad = nf.bad_windows(pieces)
        assert {0, n - 1} <= set(bad) and set(bad) >= {w for w in nf.GROUP_EDGES if w < n} and {15, 16, 31, 32} <= set(nf.GROUP_EDGES)
        at = 0
        for p in pieces[:-1]:
            at += p
            assert {at - 1, at} <= set(bad) and at - 2 not in bad and at + 1 not in bad
        assert 2 * len(bad) <= n, c["id"]                        # at least half of every call is clean
        runs, prev = [], None                                    # maximal runs of consecutive bad windows
        for w in bad:
            if prev is not None and w == prev + 1:
                runs[-1].append(w)
            else:
                runs.append([w])
            prev = w
        for run in runs:                                         # a pair at the most, with a clean window next to it: a leak's first stop
            assert len(run) <= 2 and any(0 <= w < n and w not in bad for w in (run[0] - 1, run[-1] + 1)), (c["id"], run)
        W, F, pad = geometry(c["model"])
        seen = set()
        for rot in range(3):
            smp = nf.samples(pieces, W, F, pad, rot)
            assert [s[0] for s in smp] == bad and all(0 <= t < W and 0 <= f < F for _, t, f, _ in smp)
            seen |= {(s[0], s[3]) for s in smp}
        assert seen == {(w, v) for w in bad for v in nf.VALUES}  # every bad window carries every value in one of the runs
    assert len({p for p in nf.positions(100, 9, 2)}) == 4 and len({p for p in nf.positions(8, 6, 1)}) == 4


def test_affected_against_a_brute_force():
    W = 5
    assert nf.affected(4, W, [(2, 0, 0), (0, 4, 1)], "windows") == [True, False, True, False]
    assert nf.affected(4, W, [(3, 1, 1)], "windows_bf16") == [False, False, False, True]
    for rows in ([0], [4], [5], [7, 11], [11]):
        for starts in (list(range(8)), [0, 3, 6, 9], [7, 7, 0, 2]):
            want = [any(r in range(s, s + W) for r in rows) for s in starts]
            assert nf.affected(len(starts), W, [(r, 0) for r in rows], ("series", starts)) == want
            if starts == list(range(8)):
                assert nf.affected(8, W, [(r, 0) for r in rows], "series") == want
    # a stream: the row itself and the next W rows, the row after that scores again
    got = nf.affected_rows(20, W, [3, 12])
    assert [k for k, b in enumerate(got) if b] == list(range(3, 9)) + list(range(12, 18))


def test_series_groups_leave_the_windows_just_outside_each_span_clean():
    W, F, pad = geometry(nf.SERIES_MODEL)
    n = nf.SERIES_WINDOWS
    n_rows = n + W - 1
    groups = nf.series_row_groups(n_rows, W, pad)
    assert sorted(r for g in groups for r in g) == sorted({0, pad, W - 1, n_rows // 2, n_rows - 1 - pad, n_rows - 1})
    for gi, rows in enumerate(groups):
        mask = nf.affected(n, W, [(r, 0) for r in rows], "series")
        assert 2 * sum(mask) <= n
        for r in rows:
            assert all(mask[w] for w in range(max(0, r - W + 1), min(n - 1, r) + 1))
            for w in (r - W, r + 1):
                assert not (0 <= w < n) or not mask[w], (gi, r, w)
        for rot in range(3):
            smp = nf.series_samples(n_rows, W, F, pad, gi, rot)
            assert [s[0] for s in smp] == rows and all(0 <= f < F for _, f, _ in smp)
    # stride 3: both kinds of windows remain
    starts = list(range(0, n_rows - W + 1, nf.SERIES_STRIDE))
    for rows in groups:
        m = nf.affected(len(starts), W, [(r, 0) for r in rows], ("series", starts))
        assert any(m) and 2 * sum(m) <= len(m)


def test_stream_samples_lie_where_the_table_says():
    W, F, _ = geometry("stream")
    R = W + nf.STREAM_MAX_BLOCK - 1
    assert nf.STREAM_ROWS % 7 == 0 and nf.STREAM_ROWS > 2 * R
    for rot in range(3):
        smp = nf.stream_samples(W, F, rot)
        assert [s[0] for s in smp] == [1, 3] and smp[0][3] != smp[1][3]
        for _, r, f, _ in smp:
            assert W <= r and r + W + 1 < nf.STREAM_ROWS and 0 <= f < F      # the row after the affected ones exists
        # the window that ends at the second sample's row + 1 starts before the ring's edge and ends behind it
        assert smp[1][1] % R == R - 1 and smp[0][1] != smp[1][1]


# ---- the hand-written pieces and routes are the library's ------------------------------------------------------------------------------
def front_description(r):
    import _native
    return " | ".join([_native.FRONT_CONVS[r["conv"]], _native.FRONT_LAYERS[r["temp_kernel"]], _native.FRONT_LAYERS[r["feat_kernel"]]])


def _host_front(kw, options, mode, source, n):
    import _native
    from test_host_gru_route import _create
    lib, _, h = _create(kw)
    try:
        assert lib.mtadgat_set_precision(h, mode) == 0
        for k, v in options.items():
            assert lib.mtadgat_set_option(h, k.encode(), v) == 0
        buf = (ctypes.c_int * 14)()
        assert lib.mtadgat_front_route(h, _native.FRONT_KINDS.index("forward"), _native.FRONT_SOURCES.index(source), n, 7, buf) == 0
        cap = 5 + 3 * 64
        plan = (ctypes.c_int64 * cap)()
        got = lib.mtadgat_forward_plan(h, n, plan, cap)
        assert got >= 8
        return front_description(dict(zip(_native.FRONT_ROUTE_FIELDS, (int(v) for v in buf)))), [int(plan[i + 1]) for i in range(5, got, 3)]
    finally:
        lib.mtadgat_destroy(h)


@pytest.mark.parametrize("c", nf.CASES, ids=nf.CASE_IDS)
def test_pieces_and_routes_equal_the_hand_written_table(c):
    if c["family"] == "front":
        route, pieces = _host_front(model_kwargs(c["model"]), case_options(c), c["mode"], c["source"], c["n"])
        assert route == c["route"] and pieces == c["pieces"], (c["id"], route, pieces)
        return
    from test_host_gru_route import _create
    from test_host_gru_route_cases import _answers
    lib, _, h = _create(rc.SHAPES[c["shape"]])
    try:
        pieces, routes = _answers(lib, h, c)
    finally:
        lib.mtadgat_destroy(h)
    assert pieces == c["pieces"] and routes == rc.piece_routes(c), (c["id"], pieces, routes)


def test_series_routes_equal_the_hand_written_table():
    import test_gpu_front_route as fr
    kw, options = fr.CASES[nf.SERIES_MODEL][0], fr.CASES[nf.SERIES_MODEL][1]
    n = nf.SERIES_WINDOWS
    assert _host_front(kw, options, 2, "series_unit", n) == (nf.SERIES_ROUTE, [n])
    # one window fewer (series_losses: the last window has no target row) and the strided starts leave the shared rows
    assert _host_front(kw, options, 2, "series_unit", n - 1) == (nf.SERIES_LOSSES_ROUTE, [n - 1])
    assert _host_front(kw, options, 2, "series", (n + nf.SERIES_STRIDE - 1) // nf.SERIES_STRIDE) == (nf.SERIES_STRIDED_ROUTE, [(n + 2) // 3])
