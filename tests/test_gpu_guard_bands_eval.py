"""The evaluation calls (csrc/mtadgat_eval.hip, _evalcol.hip, _events.hip, _parts.hip, _curves.hip, _spot.hip, _losses.hip behind
evaluation.py) stay inside the buffers they are handed and read nothing outside their inputs: every row runs four times
(tests/guard_rows.py) -- on allocator buffers, then with every buffer carved from a guard-banded arena (tests/arena.py: exact sizes,
256 KiB of pattern on both sides) under the NaN pattern, under the huge finite pattern, and under the NaN pattern with every data
buffer 4, 8 or 12 bytes past a 16-byte boundary (int64 / float64: 8; scratch and the SPOT state keep the alignment their
declarations in include/mtadgat.h ask for).  No guard may change, no input may change, and every result must equal the ordinary
call's bit for bit.  Every arena call runs under tests/pointer_proxy.py: a device pointer outside the arena -- a buffer the Python
layer built or copied itself -- fails the row, so inputs are given in the form the layer hands on unchanged (float32 contiguous rows,
uint8 labels, int64 starts, the parts' spans placed in the arena), and where the layer always builds a tensor (target_dims, dims,
per-part thresholds) the entry point is driven through ctypes.

Sizes: 1, 65, 257 and one below / above the constant the library reports for the call (sort tile and second scan level, run chunk,
long-part threshold of the segmented select; the epsilon tile of eval_refs for the threshold tables); fewer only where the call
sets its own sizes (parts: two span layouts; window_sse: 37 windows; SPOT: the cases of spot_cases); column calls at d in {1, 3, 64, 65}, contiguous and with ld = d + 3 over exactly
(n - 1) ld + d elements -- the last row is short, the guard begins behind its d-th element, the gap columns hold the pattern.  The
data holds ties, signed zeros, NaN and infinities.

Compared by tolerance instead of bits: mtadgat_eval_moments, _epsilon_table and their _columns forms (k_eval_moments and
k_eval_epsilon combine float64 sums with atomicAdd, two identical calls may differ in the last bits) -- counts exact, sums inside
eval_refs.check_sums against the float64 reference, as tests/test_gpu_eval_tables.py holds them -- and find_epsilon_columns, which
picks from those tables: 1e-9 relative to the oracle, the gate of tests/test_gpu_score_pipeline.py.  The calls that take no byte count
get scratch of exactly the header's minimum.  The last tests show that the harness can fail and that every entry point with a
scratch_bytes argument refuses short or misaligned scratch before anything is launched.

The preparation calls are in tests/test_gpu_guard_bands_prep.py."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import _native
import arena
import eval_refs as er
import evaluation as ev
import event_refs
import part_scale_refs as psr
import score_refs
import spot_cases
from guard_rows import place, same_bits, watched_calls
from test_gpu_curves import _label_layouts, _scores, _special
from test_gpu_eval_tables import _check_moments, _check_table
from test_gpu_score_pipeline import _bursty, eo

pytestmark = pytest.mark.gpu

_dp = ctypes.POINTER(ctypes.c_double)
TILE, LEVEL2 = ev._lib().mtadgat_eval_sort_tile(), ev._lib().mtadgat_eval_sort_scan_tiles()
CHUNK = ev._lib().mtadgat_eval_runs_chunk()
LONG = ev._lib().mtadgat_eval_partq_long()
COLUMNS = [(d, ld) for d in (1, 3, 64, 65) for ld in (d, d + 3)]
COLUMN_IDS = [f"d{d}-ld{ld}" for d, ld in COLUMNS]
ERR_WORKSPACE = -5
W = 7


def _around(c):
    return sorted({1, 65, 257, c - 1, c + 1})


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _host(a):
    """A host table of the library as an output of a row."""
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _numbers(*values):
    return torch.tensor([float("nan") if v is None else float(v) for v in values], dtype=torch.float64)


def _layout(name, x, ld):
    return {name: ld} if ld != x.shape[1] else None


def _columns(n, d, seed):
    """(n, d) float32: the column kinds of score_refs (ties, signed zeros, infinities) and, from 8 rows on, a NaN in column 0."""
    a = score_refs.columns(n, d, np.random.default_rng(seed), rot=d % 5)
    if n >= 8:
        a[n // 3, 0] = np.nan
    return a


# ---- scores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 65])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_anomaly_scores(n, d, gpu_device, monkeypatch):
    rng = np.random.default_rng(1000 * n + d)
    F = d + 3
    inputs = {"preds": _dev(_special(n * d, rng).reshape(n, d), gpu_device), "recons": _dev(_special(n * d, rng).reshape(n, d), gpu_device),
              "values": _dev(rng.random((W + n, d)).astype(np.float32), gpu_device)}
    watched_calls(monkeypatch, gpu_device, inputs,
                  lambda ins: dict(zip(("global", "per_dim"), ev.anomaly_scores(ins["preds"], ins["recons"], ins["values"], W, gamma=0.3))),
                  f"anomaly_scores n={n} d={d}")
    # with target_dims the layer builds the index tensor itself: mtadgat_eval_scores directly, the indices in the arena
    inputs["values"] = _dev(rng.random((W + n, F)).astype(np.float32), gpu_device)
    inputs["dims"] = torch.arange(F - 1, F - 1 - d, -1, dtype=torch.int32).to(gpu_device)

    def call(ins):
        per_dim = _native._empty((n, d), dtype=torch.float32, device=gpu_device)
        glob = _native._empty((n,), dtype=torch.float32, device=gpu_device)
        actual = ins["values"][W:]
        with torch.cuda.device(gpu_device):
            rc = ev._lib().mtadgat_eval_scores(ins["preds"].data_ptr(), ins["recons"].data_ptr(), actual.data_ptr(), n, d, F, ins["dims"].data_ptr(),
                                               0.3, per_dim.data_ptr(), glob.data_ptr(), ev._stream(per_dim))
        assert rc == 0
        return {"global": glob, "per_dim": per_dim}
    watched_calls(monkeypatch, gpu_device, inputs, call, f"eval_scores with dims n={n} d={d}")


# ---- thresholds: the calls that take no byte count, on scratch of exactly the header's minimum ------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 257, 65535, 65537])
def test_moments_on_two_doubles(n, gpu_device, monkeypatch):
    e = er.moment_columns(n, 1)[:, 0]
    ref = er.moments(e) + (er.abs_sum(e),)

    def call(ins):
        scratch = _native._empty(2, dtype=torch.float64, device=gpu_device)
        out = (ctypes.c_double * 2)()
        with torch.cuda.device(gpu_device):
            assert ev._lib().mtadgat_eval_moments(ins["e"].data_ptr(), n, scratch.data_ptr(), out, ev._stream(scratch)) == 0
        return {"moments": _host(list(out))}
    held = lambda got, _, what: _check_moments(got.tolist(), ref, n)                                                    # noqa: E731
    watched_calls(monkeypatch, gpu_device, {"e": _dev(e, gpu_device)}, call, f"moments n={n}", compare={"moments": held},
                  on_ordinary=lambda r: held(r["moments"], None, "ordinary"))


@pytest.mark.parametrize("n", [1, 65, 257, er.EPS_TILE - 1, er.EPS_TILE + 1])
def test_epsilon_table_on_its_minimum(n, gpu_device, monkeypatch):
    halo, nz = 49, er.EPS_NZ
    e, eps = er.epsilon_case(n, halo, 0, n >= 257)
    tab, absum = er.epsilon_table(e, eps, halo, with_abs=True)

    def call(ins):
        scratch = _native._empty(64 + 4 * nz, dtype=torch.float64, device=gpu_device)
        out = (ctypes.c_double * (4 * nz))()
        with torch.cuda.device(gpu_device):
            rc = ev._lib().mtadgat_eval_epsilon_table(ins["e"].data_ptr(), n, eps.ctypes.data_as(_dp), nz, halo, scratch.data_ptr(), out,
                                                      ev._stream(scratch))
        assert rc == 0
        return {"table": _host(list(out))}
    held = lambda got, _, what: _check_table(got.numpy(), tab, absum, n, finite=n < 257)                                # noqa: E731
    watched_calls(monkeypatch, gpu_device, {"e": _dev(e, gpu_device)}, call, f"epsilon_table n={n}", compare={"table": held},
                  on_ordinary=lambda r: held(r["table"], None, "ordinary"))


@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("n", [1, 65, 257, er.EPS_TILE - 1, er.EPS_TILE + 1])
def test_column_tables_on_their_minimum(n, d, ld, gpu_device, monkeypatch):
    """mtadgat_eval_moments_columns on 2 d doubles, mtadgat_eval_epsilon_table_columns on 5 d nz doubles."""
    halo, nz = 49, er.EPS_NZ
    m = er.moment_columns(n, d)
    mref = [er.moments(m[:, c]) + (er.abs_sum(m[:, c]),) for c in range(d)]
    cases = [er.epsilon_case(n, halo, 1 + c) for c in range(d)]
    e, eps = np.stack([c[0] for c in cases], axis=1), np.ascontiguousarray(np.stack([c[1] for c in cases]))
    tabs = [er.epsilon_table(e[:, c], eps[c], halo, with_abs=True) for c in range(d)]

    def call(ins):
        lib = ev._lib()
        s_mom = _native._empty(2 * d, dtype=torch.float64, device=gpu_device)
        s_tab = _native._empty(5 * d * nz, dtype=torch.float64, device=gpu_device)
        mom, tab = (ctypes.c_double * (2 * d))(), (ctypes.c_double * (4 * nz * d))()
        with torch.cuda.device(gpu_device):
            assert lib.mtadgat_eval_moments_columns(ins["m"].data_ptr(), n, d, ins["m"].stride(0), s_mom.data_ptr(), mom, ev._stream(s_mom)) == 0
            assert lib.mtadgat_eval_epsilon_table_columns(ins["e"].data_ptr(), n, d, ins["e"].stride(0), eps.ctypes.data_as(_dp), nz, halo,
                                                          s_tab.data_ptr(), tab, ev._stream(s_tab)) == 0
        return {"moments": _host(list(mom)), "table": _host(list(tab))}

    def held_moments(got, _, what):
        for c in range(d):
            _check_moments(got[2 * c:2 * c + 2].tolist(), mref[c], n)

    def held_table(got, _, what):
        for c in range(d):
            _check_table(got[4 * nz * c:4 * nz * (c + 1)].numpy(), tabs[c][0], tabs[c][1], n)
    inputs = {"m": _dev(m, gpu_device), "e": _dev(e, gpu_device)}
    watched_calls(monkeypatch, gpu_device, inputs, call, f"column tables n={n} d={d} ld={ld}",
                  layout={"m": ld, "e": ld} if ld != d else None, compare={"moments": held_moments, "table": held_table},
                  on_ordinary=lambda r: (held_moments(r["moments"], None, ""), held_table(r["table"], None, "")))


def _point_adjust(ins, n, thr, max_seg, device):
    nt = thr.size
    scratch = _native._empty(7 * nt + max_seg + 1, dtype=torch.float64, device=device)      # 7 nt doubles, then 2 max_seg + 2 ints
    out = np.full((nt, 6), -1.0)
    with torch.cuda.device(device):
        rc = ev._lib().mtadgat_eval_point_adjust(ins["score"].data_ptr(), ins["label"].data_ptr(), n, thr.ctypes.data_as(_dp), nt, 0, max_seg,
                                                 scratch.data_ptr(), out.ctypes.data_as(_dp), ev._stream(scratch))
    return rc, out


@pytest.mark.parametrize("kind", ["alternating", "random", "ending_at_end"])
@pytest.mark.parametrize("n", [1, 65, 257, 4099])
def test_point_adjust_on_its_minimum(n, kind, gpu_device, monkeypatch):
    """max_seg is exactly the number of labelled segments."""
    s, lab, thr = er.adjust_case(n, kind)
    nseg = max(len(event_refs.runs(lab)[0]), 1)
    want = er.point_adjust_table(s, lab, thr)

    def call(ins):
        rc, out = _point_adjust(ins, n, thr, nseg, gpu_device)
        assert rc == 0
        return {"counts": _host(out)}
    watched_calls(monkeypatch, gpu_device, {"score": _dev(s, gpu_device), "label": _dev(lab, gpu_device)}, call, f"point_adjust n={n} {kind}",
                  on_ordinary=lambda r: er.check_counts(r["counts"].numpy(), want))


def test_point_adjust_with_one_segment_too_many_is_refused_inside_its_scratch(gpu_device, monkeypatch):
    n = 257
    s, lab, thr = er.adjust_case(n, "alternating")
    nseg = len(event_refs.runs(lab)[0])
    assert nseg >= 2

    def call(ins):
        rc, _ = _point_adjust(ins, n, thr, nseg - 1, gpu_device)
        return {"status": torch.tensor([rc])}
    ref, _ = watched_calls(monkeypatch, gpu_device, {"score": _dev(s, gpu_device), "label": _dev(lab, gpu_device)}, call, "point_adjust over max_seg")
    assert ref["status"].tolist() == [ERR_WORKSPACE]


# ---- thresholds through the layer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("n", [1, 65, 257, 4099])
def test_column_quantiles(n, d, ld, gpu_device, monkeypatch):
    a = _dev(_columns(n, d, 7 * n + d), gpu_device)
    for qs in ([0.5], [0.0, 0.25, 0.5, 0.75, 1.0]):
        watched_calls(monkeypatch, gpu_device, {"a": a}, lambda ins: {"q": ev.column_quantiles(ins["a"], qs)},
                      f"column_quantiles n={n} d={d} ld={ld} nq={len(qs)}", layout=_layout("a", a, ld))


@pytest.mark.parametrize("n", _around(CHUNK))
def test_moving_average(n, gpu_device, monkeypatch):
    x = _dev(_special(n, np.random.default_rng(n)), gpu_device)
    watched_calls(monkeypatch, gpu_device, {"x": x}, lambda ins: {"y": ev.moving_average(ins["x"], 7)}, f"moving_average n={n}")


@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("n", [1, 65, 257, er.EPS_TILE - 1, er.EPS_TILE + 1])
def test_find_epsilon_columns(n, d, ld, gpu_device, monkeypatch):
    """Bursty columns; a single row (no z qualifies: the column's maximum) is uniform noise."""
    e = _bursty(n, d, 100 + d) if n > 12 else np.random.default_rng(d).random((n, d)).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                              # (the oracle divides by a zero deviation at n = 1)
        ref = np.array([eo.find_epsilon(e[:, c], 1) for c in range(d)])

    def held(got, _, what):
        assert bool((torch.abs(got - torch.from_numpy(ref)) <= 1e-9 * torch.from_numpy(np.abs(ref))).all()), (what, got.tolist(), ref.tolist())
    x = _dev(e, gpu_device)
    def call(ins):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return {"eps": torch.tensor(ev.find_epsilon_columns(ins["e"]), dtype=torch.float64)}
    watched_calls(monkeypatch, gpu_device, {"e": x}, call,
                  f"find_epsilon_columns n={n} d={d} ld={ld}", layout=_layout("e", x, ld), compare={"eps": held},
                  on_ordinary=lambda r: held(r["eps"], None, "ordinary"))


# ---- events --------------------------------------------------------------------------------------------------------------------------------
def _event_scores(n, seed):
    """Scores in [0, 1) with runs above 0.5 of several lengths, one across every chunk boundary and at both ends, NaN and +-inf."""
    rng = np.random.default_rng(seed)
    x = np.convolve(rng.random(n + 4), np.ones(5) / 5.0, mode="valid")[:n].astype(np.float32)
    for c in range(CHUNK, n, CHUNK):
        x[c - 3:c + 3] = 1.0
    x[0] = x[n - 1] = 1.0
    if n >= 65:
        for j, v in enumerate((np.nan, np.inf, -np.inf, 0.5, np.nan)):
            x[(j * 37 + 5) % n] = v
    return x


@pytest.mark.parametrize("source", ["scores", "labels"])
@pytest.mark.parametrize("n", _around(CHUNK))
def test_flag_runs(n, source, gpu_device, monkeypatch):
    """max_runs exactly the count; with one too few the entry point answers -5, writes the first max_runs runs and no more."""
    x = _event_scores(n, n)
    flag = event_refs.flags(x, 0.5)
    src = {"x": _dev(x, gpu_device)} if source == "scores" else {"x": _dev(flag.astype(np.uint8), gpu_device)}
    for gap, min_length in ((0, 1), (2, 3)):
        want = event_refs.runs(flag, gap, min_length)
        count = len(want[0])

        def call(ins):
            kw = dict(scores=ins["x"], threshold=0.5) if source == "scores" else dict(labels=ins["x"])
            got, start, end = ev.flag_runs(merge_gap=gap, min_length=min_length, max_runs=max(count, 1), **kw)
            return {"count": torch.tensor([got]), "start": start, "end": end}
        ref, _ = watched_calls(monkeypatch, gpu_device, src, call, f"flag_runs {source} n={n} gap={gap} min={min_length}")
        assert ref["count"].tolist() == [count] and np.array_equal(ref["start"].cpu().numpy(), want[0])
        if count < 2:
            continue

        def short(ins):
            lib = ev._lib()
            scratch = ev._scratch(lib.mtadgat_eval_runs_scratch(n), gpu_device)
            start = _native._empty(count - 1, dtype=torch.int64, device=gpu_device)
            end = _native._empty(count - 1, dtype=torch.int64, device=gpu_device)
            found = ctypes.c_int64(-1)
            s, lab = (ins["x"].data_ptr(), None) if source == "scores" else (None, ins["x"].data_ptr())
            with torch.cuda.device(gpu_device):
                rc = lib.mtadgat_eval_runs(s, lab, n, 0.5, 0, gap, min_length, count - 1, scratch.data_ptr(), scratch.numel() * 8, start.data_ptr(),
                                           end.data_ptr(), ctypes.byref(found), ev._stream(start))
            return {"status": torch.tensor([rc, found.value]), "start": start, "end": end}
        ref, _ = watched_calls(monkeypatch, gpu_device, src, short, f"flag_runs {source} n={n} gap={gap}: one run too many")
        assert ref["status"].tolist() == [ERR_WORKSPACE, count] and np.array_equal(ref["end"].cpu().numpy(), want[1][:-1])


@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("n", _around(CHUNK))
def test_run_statistics(n, d, ld, gpu_device, monkeypatch):
    x = _event_scores(n, n + d)
    start, end = event_refs.runs(event_refs.flags(x, 0.5), 0, 1)
    assert len(start) >= (2 if n > 1 else 1) and start[0] == 0 and end[-1] == n       # runs at both ends of the scores
    per_dim = _columns(n, d, n + 3 * d)
    thr = np.linspace(0.25, 1.75, d)
    inputs = {"x": _dev(x, gpu_device), "start": _dev(start, gpu_device), "end": _dev(end, gpu_device), "per_dim": _dev(per_dim, gpu_device),
              "thr": _dev(thr, gpu_device)}
    layout = _layout("per_dim", inputs["per_dim"], ld)
    for top_k in sorted({1, min(d, 64)}):
        watched_calls(monkeypatch, gpu_device, inputs,
                      lambda ins: ev.run_statistics(ins["x"], ins["start"], ins["end"], per_dim=ins["per_dim"], feature_thresholds=ins["thr"], top_k=top_k),
                      f"run_statistics n={n} d={d} ld={ld} top_k={top_k}", layout=layout)
    watched_calls(monkeypatch, gpu_device, inputs, lambda ins: ev.run_statistics(ins["x"], ins["start"], ins["end"], per_dim=ins["per_dim"], top_k=1),
                  f"run_statistics n={n} d={d} ld={ld} without thresholds", layout=layout)
    if (d, ld) == COLUMNS[0]:
        plain = {k: inputs[k] for k in ("x", "start", "end")}
        watched_calls(monkeypatch, gpu_device, plain, lambda ins: ev.run_statistics(ins["x"], ins["start"], ins["end"]), f"run_statistics n={n} scores only")


@pytest.mark.parametrize("n", _around(CHUNK))
def test_first_hits(n, gpu_device, monkeypatch):
    x = _event_scores(n, 3 * n)
    lab = (np.convolve(np.random.default_rng(n).random(n + 8), np.ones(9) / 9.0, mode="valid")[:n] > 0.5).astype(np.uint8)
    lab[0] = lab[n - 1] = 1
    seg = event_refs.runs(lab)
    ev_runs = event_refs.runs(event_refs.flags(x, 0.5))
    inputs = {"x": _dev(x, gpu_device), "lab": _dev(lab, gpu_device), "seg_start": _dev(seg[0], gpu_device), "seg_end": _dev(seg[1], gpu_device),
              "ev_start": _dev(ev_runs[0], gpu_device), "ev_end": _dev(ev_runs[1], gpu_device)}
    watched_calls(monkeypatch, gpu_device, inputs,
                  lambda ins: {"detected": ev.first_hits(ins["seg_start"], ins["seg_end"], scores=ins["x"], threshold=0.5),
                               "true": ev.first_hits(ins["ev_start"], ins["ev_end"], labels=ins["lab"])}, f"first_hits n={n}")


# ---- parts ---------------------------------------------------------------------------------------------------------------------------------
PART_SPANS = {"short": [1, 0, 65, 3], "long": [1, 0, LONG + 1, 257, 0, 2]}     # a part of one row, an empty one, one longer than LONG


def _part_inputs(spans, device):
    """The spans' start / end / seams as inputs of a row, and a function that makes the ScoreParts of a call from the placed ones."""
    lengths = psr.lengths_of(spans, W)
    host = ev.score_parts(lengths, W, transition=(2, 3))
    inputs = {"start": _dev(host.start_host, device), "end": _dev(host.end_host, device), "seams": _dev(host.seams_host, device)}

    def parts(ins):                                                  # the placed spans instead of the copies tensors() would make
        return ev.score_parts(lengths, W, transition=(2, 3)).use_tensors(ins["start"], ins["end"], ins["seams"])
    return host, inputs, parts


@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("spans", list(PART_SPANS))
def test_part_quantiles_and_scale(spans, d, ld, gpu_device, monkeypatch):
    host, inputs, parts = _part_inputs(PART_SPANS[spans], gpu_device)
    inputs["a"] = _dev(_columns(host.n, d, host.n + d), gpu_device)
    layout = _layout("a", inputs["a"], ld)
    for qs in ([0.5], [0.0, 0.25, 0.5, 0.75, 1.0]):
        watched_calls(monkeypatch, gpu_device, inputs, lambda ins: {"q": ev.part_quantiles(ins["a"], qs, parts(ins))},
                      f"part_quantiles {spans} d={d} ld={ld} nq={len(qs)}", layout=layout)
    watched_calls(monkeypatch, gpu_device, inputs, lambda ins: {"scaled": ev.scale_scores(ins["a"], parts=parts(ins))},
                  f"scale_scores(parts=) {spans} d={d} ld={ld}", layout=layout)
    for normalize in (True, False):
        watched_calls(monkeypatch, gpu_device, inputs, lambda ins: {"adjusted": ev.adjust_part_scores(ins["a"], parts(ins), normalize=normalize)},
                      f"adjust_part_scores {spans} d={d} ld={ld} normalize={normalize}", layout=layout)


@pytest.mark.parametrize("spans", [[1, 0, 65, 3], [1, 0, CHUNK - 1, 0, CHUNK + 1, 300]], ids=["short", "chunks"])
def test_part_scans_and_thresholds(spans, gpu_device, monkeypatch):
    """moving_average(parts=), find_epsilon_parts (no atomics: bits) and mtadgat_eval_part_flags, whose thresholds the layer always
    copies to the device itself: driven directly."""
    host, inputs, parts = _part_inputs(spans, gpu_device)
    n, P = host.n, host.n_parts
    rng = np.random.default_rng(n)
    inputs["x"] = _dev(_special(n, rng), gpu_device)
    watched_calls(monkeypatch, gpu_device, inputs, lambda ins: {"y": ev.moving_average(ins["x"], 7, parts=parts(ins))}, f"moving_average(parts=) n={n}")
    burst = (rng.random(n) * 0.1).astype(np.float32)
    for s, e in zip(host.start_host, host.end_host):
        if e - s >= 300:
            burst[s + 100:s + 107] += 2.0
    inputs["x"] = _dev(burst, gpu_device)
    watched_calls(monkeypatch, gpu_device, inputs, lambda ins: {"eps": torch.from_numpy(ev.find_epsilon_parts(ins["x"], parts(ins)))},
                  f"find_epsilon_parts n={n}", seam=False)
    inputs["x"] = _dev(_special(n, rng), gpu_device)
    inputs["thr"] = _dev(rng.choice(np.array([-0.25, 0.0, 0.25, np.inf]), size=P), gpu_device)

    def flags(ins):
        out = _native._empty(n, dtype=torch.uint8, device=gpu_device)
        with torch.cuda.device(gpu_device):
            rc = ev._lib().mtadgat_eval_part_flags(ins["x"].data_ptr(), n, ins["start"].data_ptr(), ins["end"].data_ptr(), P, ins["thr"].data_ptr(),
                                                   out.data_ptr(), ev._stream(out))
        assert rc == 0
        return {"flags": out}
    ref, _ = watched_calls(monkeypatch, gpu_device, inputs, flags, f"part_flags n={n}")
    assert torch.equal(ref["flags"], ev.part_predictions(inputs["x"], host, inputs["thr"].cpu().numpy()))


# ---- curves --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(set(_around(TILE)) | {TILE * LEVEL2 + 1}))
def test_score_order(n, gpu_device, monkeypatch):
    x = _dev(_special(n, np.random.default_rng(n)), gpu_device)
    for descending in (True, False):
        watched_calls(monkeypatch, gpu_device, {"x": x}, lambda ins: {"order": ev.score_order(ins["x"], descending=descending)},
                      f"score_order n={n} descending={descending}")


@pytest.mark.parametrize("adjust", [None, "point", ("k", 30)], ids=["raw", "point", "k30"])
@pytest.mark.parametrize("n", _around(TILE))
def test_ranking_curve_and_metrics(n, adjust, gpu_device, monkeypatch):
    rng = np.random.default_rng(n)
    s = _scores(n, rng)
    lab = _label_layouts(n, rng, s)["mixed"].astype(np.uint8)

    def call(ins):
        c = ev.ranking_curve(ins["s"], ins["lab"], adjust=adjust)
        m = ev.ranking_metrics(ins["s"], ins["lab"], adjust=adjust)
        best = m["best"] or {}
        return {"thresholds": c["thresholds"], "tp": c["tp"], "fp": c["fp"],
                "numbers": _numbers(c["n_pos"], c["n_neg"], c["nan_pos"], c["nan_neg"], m["auroc"], m["average_precision"], m["best_index"],
                                    best.get("f1"), best.get("threshold"), best.get("latency"))}
    watched_calls(monkeypatch, gpu_device, {"s": _dev(s, gpu_device), "lab": _dev(lab, gpu_device)}, call, f"ranking curve n={n} adjust={adjust}")


# ---- losses --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,ld", [(1, 1), (3, 6), (65, 65), (65, 68)])
def test_window_sse(F, ld, gpu_device, monkeypatch):
    n, Wn, out = 37, 5, min(F, 3)
    rows = 3 * (n - 1) + Wn + 1
    rng = np.random.default_rng(F)
    series = rng.standard_normal((rows, F)).astype(np.float32)
    series[rows // 2, 0] = np.nan
    starts = rng.integers(0, rows - Wn, n)
    starts[0], starts[n // 2] = rows - Wn - 1, 0                     # the last possible window among them, unsorted
    inputs = {"preds": _dev(rng.standard_normal((n, out)).astype(np.float32), gpu_device),
              "recons": _dev(rng.standard_normal((n, Wn, out)).astype(np.float32), gpu_device), "series": _dev(series, gpu_device),
              "starts": _dev(starts.astype(np.int64), gpu_device), "dims": torch.arange(F - 1, F - 1 - out, -1, dtype=torch.int32).to(gpu_device)}
    layout = _layout("series", inputs["series"], ld)
    for what, kw in (("stride 1", dict(stride=1)), ("stride 3", dict(stride=3)), ("starts", None)):
        watched_calls(monkeypatch, gpu_device, inputs,
                      lambda ins: dict(zip(("window_sse", "dim_sse"),
                                           ev.window_sse(ins["preds"], ins["recons"], ins["series"], **(kw or dict(starts=ins["starts"]))))),
                      f"window_sse F={F} ld={ld} {what}", layout=layout)

    def with_dims(ins):                                              # the layer builds the column indices itself: driven directly
        lib = ev._lib()
        need = lib.mtadgat_eval_window_sse_scratch(n, out)
        scratch = ev._scratch(need, gpu_device)
        wsse = _native._empty((n, 2), dtype=torch.float64, device=gpu_device)
        dsse = _native._empty((2, out), dtype=torch.float64, device=gpu_device)
        with torch.cuda.device(gpu_device):
            rc = lib.mtadgat_eval_window_sse(ins["preds"].data_ptr(), ins["recons"].data_ptr(), n, Wn, out, ins["series"].data_ptr(), rows, F,
                                             ins["series"].stride(0), ins["starts"].data_ptr(), 0, 0, ins["dims"].data_ptr(), 0, wsse.data_ptr(),
                                             dsse.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, ev._stream(wsse))
        assert rc == 0, lib.mtadgat_last_error()
        return {"window_sse": wsse, "dim_sse": dsse}
    watched_calls(monkeypatch, gpu_device, inputs, with_dims, f"window_sse F={F} ld={ld} dims", layout=layout)


@pytest.mark.parametrize("n", [1, 65, 257, 1025])
def test_group_sums(n, gpu_device, monkeypatch):
    x = _dev(np.random.default_rng(n).standard_normal((n, 2)), gpu_device)
    for group in (1, 7, n + 1):
        watched_calls(monkeypatch, gpu_device, {"x": x}, lambda ins: {"sums": ev.group_sums(ins["x"], group)}, f"group_sums n={n} group={group}",
                      finite=True)


# ---- peaks over threshold ---------------------------------------------------------------------------------------------------------------------
def spot_state(template, device):
    """A copy of a calibrated state's bytes in a buffer from the seam (16-byte aligned in every run: arena.SCRATCH_BUFFERS)."""
    buf = _native._empty(template.shape, dtype=torch.float64, device=device)
    buf.copy_(template)
    return buf


@pytest.mark.parametrize("max_peaks", [8, 64])
@pytest.mark.parametrize("case,ld", [("one column", 1), ("one column", 4), ("three columns", 3), ("three columns", 6), ("seventy columns", 70)])
def test_spot_calibrate(case, ld, max_peaks, gpu_device, monkeypatch):
    """The state is exactly mtadgat_spot_state_bytes: the guard begins where the library says the state ends."""
    S, _, _, _, level, _ = spot_cases.CASES[case]
    init = _dev(spot_cases.data(case)[0], gpu_device)
    nbytes = ev._lib().mtadgat_spot_state_bytes(S, max_peaks)
    assert nbytes > 0 and nbytes % 8 == 0
    for dynamic in (True, False):
        def call(ins):
            state = ev.spot_calibrate(ins["init"], q=spot_cases.Q, level=level, max_peaks=max_peaks, dynamic=dynamic)
            assert state.buf.numel() * 8 == nbytes
            return {"state": state.buf}
        watched_calls(monkeypatch, gpu_device, {"init": init}, call, f"spot_calibrate {case} ld={ld} max_peaks={max_peaks} dynamic={dynamic}",
                      layout=_layout("init", init, ld), seam=False)            # (state and scratch: both keep their alignment)


@pytest.mark.parametrize("dynamic", [True, False], ids=["dynamic", "static"])
@pytest.mark.parametrize("case,ld", [("three columns", 3), ("three columns", 6), ("seventy columns", 70)])
def test_spot_run_and_copy(case, ld, dynamic, gpu_device, monkeypatch):
    """max_peaks 8: the ring wraps during the run.  The state is an input and an output: the call works on a copy placed by the seam, and
    the copy's bits after the run are compared."""
    S, _, _, max_peaks, level, _ = spot_cases.CASES[case]
    assert max_peaks == 8
    init, scores = (_dev(a, gpu_device) for a in spot_cases.data(case))
    calibrated = ev.spot_calibrate(init, q=spot_cases.Q, level=level, max_peaks=max_peaks, dynamic=dynamic)

    def call(ins):
        state = ev.SpotState(spot_state(ins["state"], gpu_device), S, max_peaks, spot_cases.Q, level, dynamic)
        thr, flags = ev.spot_run(state, ins["scores"])
        return {"thresholds": thr, "flags": flags, "state": state.buf}
    ref, _ = watched_calls(monkeypatch, gpu_device, {"state": calibrated.buf, "scores": scores}, call, f"spot_run {case} ld={ld} dynamic={dynamic}",
                           layout=_layout("scores", scores, ld))
    assert same_bits(ref["state"], calibrated.buf) == (not dynamic)
    if dynamic:
        one = ev.spot_calibrate(init[:, :1].contiguous(), q=spot_cases.Q, level=level, max_peaks=max_peaks)

        def expand(ins):
            return {"state": ev.SpotState(spot_state(ins["state"], gpu_device), 1, max_peaks, spot_cases.Q, level, True).expand(S).buf}
        watched_calls(monkeypatch, gpu_device, {"state": one.buf}, expand, f"spot expand to {S} columns", seam=False)


# ---- what the layer hands on unchanged ---------------------------------------------------------------------------------------------------------
def test_a_single_row_is_read_where_it_lies(gpu_device):
    """_dev2d re-views a (1, d) input with contiguous elements instead of copying it (a row of a wider tensor, a row stride of 0):
    same address, row stride d, and the quantiles of one row are that row."""
    wide = torch.arange(40, dtype=torch.float32, device=gpu_device).reshape(4, 10)
    for t in (wide[2:3, 3:8], wide[1:2], wide[3:4, 9:10], torch.arange(5.0, device=gpu_device).as_strided((1, 5), (0, 1))):
        got = ev._dev2d(t, "t")
        assert got.data_ptr() == t.data_ptr() and got.stride() == (t.shape[1], 1) and torch.equal(got, t)
        assert torch.equal(ev.column_quantiles(t, [0.0, 0.5, 1.0]), t.expand(3, -1))
    strided = wide[0:1, ::3]
    got = ev._dev2d(strided, "t")
    assert got.data_ptr() != strided.data_ptr() and torch.equal(got, strided)


@pytest.mark.parametrize("n", [1, 65, CHUNK + 1])
def test_uint8_labels_other_than_one_are_labels(n, gpu_device):
    """uint8 labels reach the kernels as they are, and the kernels test != 0: labels of 2, 128 and 255 give what 1 gives, as
    `label > 0.1` did."""
    rng = np.random.default_rng(n)
    s = _scores(n, rng)
    lab = _label_layouts(n, rng, s)["mixed"].astype(np.uint8)
    odd = lab * rng.choice(np.array([1, 2, 128, 255], np.uint8), size=n)
    assert n == 1 or (odd > 1).any()
    sd, one, other = _dev(s, gpu_device), _dev(lab, gpu_device), _dev(odd, gpu_device)
    for a, b in zip(ev.flag_runs(labels=one), ev.flag_runs(labels=other)):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))
    _, start, end = ev.flag_runs(labels=one)
    assert torch.equal(ev.first_hits(start, end, labels=one), ev.first_hits(start, end, labels=other))
    thr = [0.1, 0.5]
    assert np.array_equal(ev.point_adjust_counts(sd, one, thr), ev.point_adjust_counts(sd, other, thr))
    assert np.array_equal(ev.point_adjust_counts(sd, one.bool(), thr), ev.point_adjust_counts(sd, other, thr))
    for adjust in (None, "point", ("k", 30)):
        a, b = ev.ranking_curve(sd, one, adjust=adjust), ev.ranking_curve(sd, other, adjust=adjust)
        assert all(same_bits(a[k], b[k]) for k in ("thresholds", "tp", "fp")) and a["n_pos"] == b["n_pos"] and a["nan_pos"] == b["nan_pos"]


# ---- the harness can fail ----------------------------------------------------------------------------------------------------------------------
def _arena_for(monkeypatch, device, inputs, call):
    meter = arena.Meter(device)
    with meter.patched(monkeypatch):
        call(inputs)
    return arena.Arena(device, arena.PATTERN_A, arena.capacity_for(meter.sizes + [t.numel() * t.element_size() for t in inputs.values()]))


def test_an_output_guard_that_begins_one_element_early_catches_the_last_store(gpu_device, monkeypatch):
    """score_order's `order` with its last int64 already guard: reported as exactly that buffer, behind it, one or two words (the
    high word of a small index is zero, the pattern's is not)."""
    n = TILE + 1
    x = _dev(_special(n, np.random.default_rng(5)), gpu_device)
    call = lambda ins: ev.score_order(ins["x"])                                                                       # noqa: E731
    ref = call({"x": x})
    ar = _arena_for(monkeypatch, gpu_device, {"x": x}, call)
    ins = place(ar, {"x": x}, False)
    with ar.patched(monkeypatch, rules={"score_order.order": dict(early=1)}):
        got = call(ins)
    report = ar.check()
    assert len(report) == 1 and report[0]["words"] in (1, 2), report
    assert {k: report[0][k] for k in ("name", "side", "offset")} == dict(name="score_order.order", side="behind", offset=8 * (n - 1)), report
    assert same_bits(got, ref)


def test_an_input_guard_that_begins_one_element_early_poisons_the_last_output(gpu_device, monkeypatch):
    """The last score of moving_average is guard and holds the NaN pattern: the last average alone turns NaN."""
    n = CHUNK + 1
    x = _dev(np.random.default_rng(6).random(n).astype(np.float32), gpu_device)
    call = lambda ins: ev.moving_average(ins["x"], 7)                                                                 # noqa: E731
    ref = call({"x": x})
    ar = _arena_for(monkeypatch, gpu_device, {"x": x}, call)
    xa = ar.take(x.shape, fill=x, early=1, name="x")
    with ar.patched(monkeypatch):
        got = call({"x": xa})
    assert ar.check() == []
    assert bool(torch.isnan(got[-1])) and same_bits(got[:-1], ref[:-1]) and bool(torch.isfinite(ref).all())


def _refusal_calls(lib, t, device):
    """{entry: (alignment, need, call(scratch pointer, bytes))} for every entry point with a scratch_bytes argument; t(name, shape,
    dtype, fill) takes a buffer from the arena of the attempt."""
    n, d, P, nq, Wn = 3000, 3, 2, 3, 5
    p = lambda a: a.data_ptr()                                                                                        # noqa: E731
    i64, f64, f32 = torch.int64, torch.float64, torch.float32
    q = (ctypes.c_double * nq)(0.25, 0.5, 0.75)
    eps = (ctypes.c_double * (P * 19))(*([1.0] * (P * 19)))
    host = (ctypes.c_double * (P * 4 * 19))()
    count, summary = ctypes.c_int64(0), (ctypes.c_int64 * 12)()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    x = lambda: t("x", (n,), f32, 0.5)                                                                                # noqa: E731
    a = lambda: t("a", (n, d), f32, 0.5)                                                                              # noqa: E731
    lab = lambda: t("lab", (n,), torch.uint8, 1)                                                                      # noqa: E731
    span = lambda: (t("start", (P,), i64, torch.tensor([0, 100], device=device)), t("end", (P,), i64, torch.tensor([100, n], device=device)))  # noqa: E731

    def spans(fn, *before):
        s, e = span()
        return lambda *after: fn(*before, p(s), p(e), P, *after)
    return {
        "column_quantiles": (16, lib.mtadgat_eval_column_quantiles_scratch(n, d, nq),
                             lambda s, b: lib.mtadgat_eval_column_quantiles(p(a()), n, d, d, q, nq, s, b, p(t("out", (nq, d), f32)), stream)),
        "ewm": (8, lib.mtadgat_eval_ewm_scratch(n), lambda s, b: lib.mtadgat_eval_ewm(p(x()), n, 0.25, s, b, p(t("out", (n,), f32)), stream)),
        "runs": (8, lib.mtadgat_eval_runs_scratch(n),
                 lambda s, b: lib.mtadgat_eval_runs(p(x()), None, n, 0.25, 0, 0, 1, 4, s, b, p(t("start", (4,), i64)), p(t("end", (4,), i64)),
                                                    ctypes.byref(count), stream)),
        "run_stats": (8, lib.mtadgat_eval_run_stats_scratch(n, P, d),
                      lambda s, b: spans(lib.mtadgat_eval_run_stats, p(x()), n)(p(a()), d, d, None, 1, s, b, p(t("peak", (P,), i64)),
                                                                                p(t("peak_score", (P,), f32)), p(t("mean", (P,), f32)),
                                                                                p(t("means", (P, d), f32)), p(t("top", (P, 1), torch.int32)),
                                                                                p(t("top_values", (P, 1), f32)), None, stream)),
        "part_quantiles": (16, lib.mtadgat_eval_part_quantiles_scratch(n, d, P, nq),
                           lambda s, b: spans(lib.mtadgat_eval_part_quantiles, p(a()), n, d, d)(q, nq, s, b, p(t("out", (nq, P, d), f32)), stream)),
        "part_adjust": (8, lib.mtadgat_eval_part_adjust_scratch(n, d, P),
                        lambda s, b: spans(lib.mtadgat_eval_part_adjust, p(a()), n, d, d)(None, 0, 2, 2, 1, s, b, p(t("out", (n, d), f32)), d, None,
                                                                                          stream)),
        "ewm_parts": (8, lib.mtadgat_eval_ewm_parts_scratch(n),
                      lambda s, b: spans(lib.mtadgat_eval_ewm_parts, p(x()), n)(0.25, s, b, p(t("out", (n,), f32)), stream)),
        "part_epsilon_moments": (8, lib.mtadgat_eval_part_epsilon_scratch(n, P, 19),
                                 lambda s, b: spans(lib.mtadgat_eval_part_epsilon_moments, p(x()), n)(19, s, b, host, stream)),
        "part_epsilon_table": (8, lib.mtadgat_eval_part_epsilon_scratch(n, P, 19),
                               lambda s, b: spans(lib.mtadgat_eval_part_epsilon_table, p(x()), n)(eps, 19, 49, s, b, host, stream)),
        "window_sse": (16, lib.mtadgat_eval_window_sse_scratch(n - Wn - 1, d),
                       lambda s, b: lib.mtadgat_eval_window_sse(p(t("preds", (n - Wn - 1, d), f32, 0.5)), p(t("recons", (n - Wn - 1, Wn, d), f32, 0.5)),
                                                                n - Wn - 1, Wn, d, p(a()), n, d, d, None, 0, 1, None, 0,
                                                                p(t("wsse", (n - Wn - 1, 2), f64)), p(t("dsse", (2, d), f64)), s, b, stream)),
        "score_order": (8, lib.mtadgat_eval_score_order_scratch(n),
                        lambda s, b: lib.mtadgat_eval_score_order(p(x()), n, 1, s, b, p(t("order", (n,), i64)), stream)),
        "curve": (8, lib.mtadgat_eval_curve_scratch(n, 1),
                  lambda s, b: lib.mtadgat_eval_curve(p(x()), p(lab()), n, 1, 0, s, b, p(t("thr", (n,), f32)), p(t("tp", (n,), i64)),
                                                      p(t("fp", (n,), i64)), summary, stream)),
        "spot_calibrate": (16, lib.mtadgat_spot_calibrate_scratch(n, d),
                           lambda s, b: lib.mtadgat_spot_calibrate(p(a()), n, d, d, 1e-3, 0.9, 8, 1,
                                                                   p(t("state", ((lib.mtadgat_spot_state_bytes(d, 8) + 7) // 8,), f64)), s, b, stream)),
    }


REFUSALS = ("column_quantiles", "ewm", "runs", "run_stats", "part_quantiles", "part_adjust", "ewm_parts", "part_epsilon_moments",
            "part_epsilon_table", "window_sse", "score_order", "curve", "spot_calibrate")


@pytest.mark.parametrize("entry", REFUSALS)
def test_short_or_misaligned_scratch_is_refused_before_anything_launches(entry, gpu_device):
    """Scratch 8 bytes short of what the _scratch function reports, or past the alignment the declaration states -- 8 bytes past a
    16-byte boundary where it asks for 16, 4 bytes past an 8-byte boundary where it asks for 8 --, is refused with -5, and the whole
    arena -- outputs and scratch included -- still holds its pattern: nothing was launched.  The same call on scratch of exactly the
    reported size is not refused, stays inside its buffers and leaves its outputs or scratch changed: the comparison sees a launch."""
    refuse_scratch(ev._lib(), _refusal_calls, entry, gpu_device)


def refuse_scratch(lib, calls, entry, device):
    need = calls(lib, None, device)[entry][1]
    assert need >= 16 and need % 4 == 0, (entry, need)
    for short, skew in ((8, 0), (0, None), (0, 0)):
        ar = arena.Arena(device, arena.PATTERN_A, arena.capacity_for([need + 16] + [1 << 16] * 16))

        def t(name, shape, dtype, fill=None):
            return ar.take(shape, dtype, fill=fill, name=name)
        align, _, call = calls(lib, t, device)[entry]
        skew = (8 if align == 16 else 4) if skew is None else skew
        scratch = ar.take((need - short,), torch.uint8, skew=skew, name="scratch")
        assert scratch.data_ptr() % align == skew
        with torch.cuda.device(device):
            rc = call(scratch.data_ptr(), need - short)
        if (short, skew) == (0, 0):                                       # the control: the call as it should be made
            assert rc != ERR_WORKSPACE, (entry, rc, lib.mtadgat_last_error())
            assert ar.check() == [] and any(r["side"] == "interior" for r in ar.check(interiors=True)), (entry, rc)
            continue
        assert rc == ERR_WORKSPACE, (entry, short, skew, rc, lib.mtadgat_last_error())
        assert ar.check(interiors=True) == [], (entry, short, skew)
