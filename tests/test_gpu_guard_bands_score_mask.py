"""The calls that score a gappy series (csrc/mtadgat_evalmask.hip, the NaN-skipping select of csrc/mtadgat_evalcol.hip behind
evaluation.scored_rows, anomaly_scores(age=), row_means_valid and the skip_nan arguments) stay inside the buffers they are handed and
read nothing outside their inputs, exactly as tests/test_gpu_guard_bands_eval.py holds the other evaluation calls: every row runs
four times (tests/guard_rows.py) -- on allocator buffers, then with every buffer carved from a guard-banded arena (tests/arena.py)
under the NaN pattern, under the huge finite pattern, and under the NaN pattern with every data buffer 4, 8 or 12 bytes past a 16-byte
boundary -- under tests/pointer_proxy.py; every result equals the ordinary call's bit for bit.

Sizes: 1, 65, 257 and one below / above the constant of the call -- the 1024-element chunks of the window sampler's and the moving
average's scans, the 256 x 256 rows the first stage of the moments covers in one trip; column calls at d in {1, 3, 64, 65} with ld = d
and ld = d + 3 over exactly (n - 1) ld + d elements.  The data holds NaN of either sign, infinities, ties and signed zeros.
find_epsilon_columns(skip_nan=True) picks from mtadgat_eval_epsilon_table_columns, whose float64 sums are combined with atomics: held
to 1e-9 relative of the specification instead of bits, as its plain form is.  Where the layer always builds a tensor (target_dims) the
entry point is driven through ctypes.  Short or misaligned scratch is refused before anything is launched."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import _native
import evaluation as ev
import score_mask_refs as spec
from guard_rows import watched_calls
from test_gpu_curves import _special
from test_gpu_guard_bands_eval import COLUMN_IDS, COLUMNS, _around, _columns, _dev, _layout, refuse_scratch
from test_host_score_mask import planted

pytestmark = pytest.mark.gpu

CHUNK = 1024                 # CHUNK_L / EWM_L of the scans
TRIP = 256 * 256             # rows of k_momv_blocks per trip of its grid
W = 7


def _gappy_columns(n, d, seed):
    """_columns with NaN of both signs planted, an all-NaN column (d >= 2) and, from 8 rows on, a column with one valid entry (d >= 3)."""
    a = _columns(n, d, seed)
    rng = np.random.default_rng(seed + 1)
    a[rng.random((n, d)) < 0.2] = np.nan
    bits = a.view(np.uint32)
    bits[np.isnan(a) & (rng.random((n, d)) < 0.5)] = 0xffc12345
    if d >= 2:
        a[:, 1] = np.nan
    if d >= 3 and n >= 8:
        a[:, 2] = np.nan
        a[n // 2, 2] = 0.625
    return a


@pytest.mark.parametrize("F,ld", [(1, 1), (3, 6), (65, 68)])
@pytest.mark.parametrize("n", _around(CHUNK))
def test_scored_rows(n, F, ld, gpu_device, monkeypatch):
    rng = np.random.default_rng(n + F)
    age = _dev(((rng.random((W + n, F)) < 0.4) * rng.integers(1, 5, (W + n, F))).astype(np.int32), gpu_device)
    ref, _ = watched_calls(monkeypatch, gpu_device, {"age": age},
                           lambda ins: {"keep": ev.scored_rows(W + n, W, F, ins["age"], max_age=1, min_observed=0.5)},
                           f"scored_rows n={n} F={F} ld={ld}", layout=_layout("age", age, ld))
    assert np.array_equal(ref["keep"].cpu().numpy(), spec.scored_rows(W + n, W, F, age.cpu().numpy(), 1, 0.5))


@pytest.mark.parametrize("d", [1, 3, 64, 65])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_masked_scores(n, d, gpu_device, monkeypatch):
    rng = np.random.default_rng(1000 * n + d)
    F = d + 3
    age = ((rng.random((W + n, F)) < 0.3) * 2).astype(np.int32)
    keep = (rng.random(n) < 0.8).astype(np.uint8)
    inputs = {"preds": _dev(_special(n * d, rng).reshape(n, d), gpu_device), "recons": _dev(_special(n * d, rng).reshape(n, d), gpu_device),
              "values": _dev(_special((W + n) * d, rng).reshape(W + n, d), gpu_device), "age": _dev(age[:, :d], gpu_device),
              "keep": _dev(keep, gpu_device)}
    names = ("global", "per_dim", "count")
    watched_calls(monkeypatch, gpu_device, inputs,
                  lambda ins: dict(zip(names, ev.anomaly_scores(ins["preds"], ins["recons"], ins["values"], W, gamma=0.3, age=ins["age"],
                                                                keep=ins["keep"]))), f"anomaly_scores(age=) n={n} d={d}")
    watched_calls(monkeypatch, gpu_device, inputs, lambda ins: {"global": ev.row_means_valid(ev.anomaly_scores(
        ins["preds"], ins["recons"], ins["values"], W, gamma=0.3, age=ins["age"], keep=ins["keep"])[1])}, f"row_means_valid n={n} d={d}")
    # with target_dims the layer builds the index tensor itself: mtadgat_eval_scores_masked directly, the indices in the arena, the
    # series and its ages wider than the outputs and at different row strides
    inputs["values"] = _dev(_special((W + n) * F, rng).reshape(W + n, F), gpu_device)
    inputs["age"] = _dev(age, gpu_device)
    inputs["dims"] = torch.arange(F - 1, F - 1 - d, -1, dtype=torch.int32).to(gpu_device)
    ld_age = F + 2

    def call(ins):
        per_dim = _native._empty((n, d), dtype=torch.float32, device=gpu_device)
        glob = _native._empty((n,), dtype=torch.float32, device=gpu_device)
        count = _native._empty((n,), dtype=torch.int32, device=gpu_device)
        actual, rows = ins["values"][W:], ins["age"][W:]
        with torch.cuda.device(gpu_device):
            rc = ev._lib().mtadgat_eval_scores_masked(ins["preds"].data_ptr(), ins["recons"].data_ptr(), actual.data_ptr(), n, d, F,
                                                      ins["dims"].data_ptr(), 0.3, rows.data_ptr(), ins["age"].stride(0), 0, ins["keep"].data_ptr(),
                                                      per_dim.data_ptr(), glob.data_ptr(), count.data_ptr(), ev._stream(per_dim))
        assert rc == 0
        return {"global": glob, "per_dim": per_dim, "count": count}
    watched_calls(monkeypatch, gpu_device, inputs, call, f"eval_scores_masked with dims n={n} d={d}", layout={"age": ld_age})


@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("n", [1, 65, 257, 4099])
def test_valid_quantiles(n, d, ld, gpu_device, monkeypatch):
    a = _dev(_gappy_columns(n, d, 7 * n + d), gpu_device)
    for qs in ([0.5], [0.0, 0.25, 0.5, 0.75, 1.0]):
        watched_calls(monkeypatch, gpu_device, {"a": a},
                      lambda ins: dict(zip(("q", "counts"), ev.column_quantiles(ins["a"], qs, skip_nan=True, return_counts=True))),
                      f"column_quantiles(skip_nan) n={n} d={d} ld={ld} nq={len(qs)}", layout=_layout("a", a, ld))


@pytest.mark.parametrize("n", _around(CHUNK))
def test_moving_average_over_observed_rows(n, gpu_device, monkeypatch):
    rng = np.random.default_rng(n)
    x = _special(n, rng)
    x[rng.random(n) < 0.3] = np.nan
    t = _dev(x, gpu_device)
    watched_calls(monkeypatch, gpu_device, {"x": t}, lambda ins: {"y": ev.moving_average(ins["x"], 7, skip_nan=True)},
                  f"moving_average(skip_nan) n={n}")


@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("n", [1, 65, 257, TRIP - 1, TRIP + 1])
def test_valid_moments(n, d, ld, gpu_device, monkeypatch):
    a = _gappy_columns(n, d, 3 * n + d)
    a[np.isinf(a)] = 2.5                                                # (inf - inf in a sum is a NaN whose sign the order may decide)
    t = _dev(a, gpu_device)
    ref, _ = watched_calls(monkeypatch, gpu_device, {"e": t}, lambda ins: {"moments": torch.from_numpy(ev.moments_valid(ins["e"]))},
                           f"moments_valid n={n} d={d} ld={ld}", layout=_layout("e", t, ld), seam=False)    # (its only buffer is scratch)
    assert np.array_equal(ref["moments"][:, 2].numpy(), (~np.isnan(a)).sum(axis=0))


@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("n", [1, 65, 257, CHUNK - 1, CHUNK + 1])
def test_find_epsilon_columns_skips_nan(n, d, ld, gpu_device, monkeypatch):
    if n > 12:
        e = planted(n, d, 100 + d)
    else:
        e = np.random.default_rng(d).random((n, d)).astype(np.float32)
        e[:, d - 1] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = np.array([spec.find_epsilon_valid(e[:, c], 1) for c in range(d)])

    def held(got, _, what):
        got = got.numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
        ok = ~np.isnan(ref)
        assert np.all(np.abs(got[ok] - ref[ok]) <= 1e-9 * np.abs(ref[ok])), (what, got.tolist(), ref.tolist())
    x = _dev(e, gpu_device)

    def call(ins):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return {"eps": torch.tensor(ev.find_epsilon_columns(ins["e"], skip_nan=True), dtype=torch.float64)}
    watched_calls(monkeypatch, gpu_device, {"e": x}, call, f"find_epsilon_columns(skip_nan) n={n} d={d} ld={ld}", layout=_layout("e", x, ld),
                  compare={"eps": held}, on_ordinary=lambda r: held(r["eps"], None, "ordinary"))


def _refusal_calls(lib, t, device):
    n, d, nq = 3000, 3, 3
    p = lambda a: a.data_ptr()                                                                                        # noqa: E731
    f32 = torch.float32
    q = (ctypes.c_double * nq)(0.25, 0.5, 0.75)
    host = (ctypes.c_double * (3 * d))()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    return {
        "column_quantiles_valid": (16, lib.mtadgat_eval_column_quantiles_valid_scratch(n, d, nq),
                                   lambda s, b: lib.mtadgat_eval_column_quantiles_valid(p(t("a", (n, d), f32, 0.5)), n, d, d, q, nq, s, b,
                                                                                        p(t("out", (nq, d), f32)), p(t("counts", (d,), torch.int64)),
                                                                                        stream)),
        "ewm_valid": (8, lib.mtadgat_eval_ewm_valid_scratch(n),
                      lambda s, b: lib.mtadgat_eval_ewm_valid(p(t("x", (n,), f32, 0.5)), n, 0.25, s, b, p(t("out", (n,), f32)), stream)),
        "moments_valid": (8, lib.mtadgat_eval_moments_valid_scratch(n, d),
                          lambda s, b: lib.mtadgat_eval_moments_valid(p(t("e", (n, d), f32, 0.5)), n, d, d, s, b, host, stream)),
    }


@pytest.mark.parametrize("entry", ["column_quantiles_valid", "ewm_valid", "moments_valid"])
def test_short_or_misaligned_scratch_is_refused_before_anything_launches(entry, gpu_device):
    refuse_scratch(ev._lib(), _refusal_calls, entry, gpu_device)
