"""The loss entry points without a GPU: symbols, argument validation before anything touches the device, the scratch query; the
reference the GPU tests compare against (tests/loss_refs.py) held against a naive loop; and MTAD_GAT.series_losses on CPU tensors
against the restated Trainer.evaluate."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import helpers
import loss_refs

PTR = 0x10000            # a non-null, 16-byte aligned "device pointer": validation fails before it would be used


@pytest.fixture(scope="module")
def lib():
    import evaluation
    return evaluation._lib()


def _err(lib):
    return lib.mtadgat_last_error().decode()


def test_symbols_are_exported(lib):
    import _native
    for name in ("mtadgat_eval_window_sse", "mtadgat_eval_window_sse_scratch", "mtadgat_eval_group_sums", "mtadgat_series_losses",
                 "mtadgat_series_losses_chunk", "mtadgat_series_losses_workspace_bytes"):
        assert hasattr(lib, name), name
    assert lib.mtadgat_abi_version() == 1
    from mtad_gat import MTAD_GAT
    assert hasattr(MTAD_GAT, "series_losses") and hasattr(_native.Engine, "series_losses")


def _sse(lib, preds=PTR, recons=PTR, batch=10, W=5, out=3, series=PTR, n_rows=100, F=4, ld=4, starts=None, start0=0, stride=1, dims=None,
         accumulate=0, wsse=PTR, dsse=PTR, scratch=PTR, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = max(lib.mtadgat_eval_window_sse_scratch(batch, out), 1 << 20)
    return lib.mtadgat_eval_window_sse(preds, recons, batch, W, out, series, n_rows, F, ld, starts, start0, stride, dims, accumulate, wsse,
                                       dsse, scratch, scratch_bytes, None)


SSE_BAD = {
    "null preds": (dict(preds=None), -1), "null recons": (dict(recons=None), -1), "null series": (dict(series=None), -1),
    "null window_sse": (dict(wsse=None), -1), "null scratch": (dict(scratch=None), -1),
    "batch < 1": (dict(batch=0), -1), "batch > 2^31 - 1": (dict(batch=2 ** 31, n_rows=2 ** 33), -1),
    "out_dim < 1": (dict(out=0), -1), "out_dim > 2048": (dict(out=2049, F=2049, ld=2049), -1),
    "W < 1": (dict(W=0), -1), "W > 512": (dict(W=513, n_rows=10000), -1),
    "F < 1": (dict(F=0, dims=PTR), -1), "ld_series < F": (dict(ld=3), -1),
    "out_dim > F without dims": (dict(out=5), -1),
    "series shorter than W + 1": (dict(n_rows=5, batch=1), -1),
    "start0 < 0": (dict(start0=-1), -1), "stride < 0": (dict(stride=-1, start0=50), -1),
    "target row of the last window missing": (dict(batch=95, n_rows=99), -1),                    # 94 + 5 = 99 > n_rows - 1
    "strided progression too long": (dict(batch=33, stride=3, n_rows=101), -1),                  # 96 + 5 = 101 > 100
    "accumulate not 0 / 1": (dict(accumulate=2), -1),
    "scratch one byte short": (dict(scratch_bytes=-1), -5), "misaligned scratch": (dict(scratch=PTR + 8), -5),
}


@pytest.mark.parametrize("case", list(SSE_BAD))
def test_window_sse_rejects_invalid_arguments(lib, case):
    kw, status = SSE_BAD[case]
    kw = dict(kw)
    if kw.get("scratch_bytes") == -1:
        kw["scratch_bytes"] = lib.mtadgat_eval_window_sse_scratch(10, 3) - 1
    assert _sse(lib, **kw) == status
    assert _err(lib)


def test_window_sse_progression_bounds_are_exact(lib):
    """The last legal progression passes validation (it would go on to launch: checked with a one-byte-short scratch, which is
    refused only after every argument check) and one more window does not."""
    short = lib.mtadgat_eval_window_sse_scratch(95, 3) - 1
    assert _sse(lib, batch=95, n_rows=100, scratch_bytes=short) == -5                # 94 + 5 = 99 = n_rows - 1
    assert _sse(lib, batch=96, n_rows=100, scratch_bytes=short) == -1
    assert _sse(lib, batch=32, stride=3, n_rows=99, scratch_bytes=lib.mtadgat_eval_window_sse_scratch(32, 3) - 1) == -5   # 93 + 5 = 98
    assert _sse(lib, batch=7, stride=0, start0=94, n_rows=100, scratch_bytes=lib.mtadgat_eval_window_sse_scratch(7, 3) - 1) == -5
    assert _sse(lib, batch=7, stride=0, start0=95, n_rows=100) == -1
    assert _sse(lib, out=4, dims=PTR, F=2, ld=2, scratch_bytes=lib.mtadgat_eval_window_sse_scratch(10, 4) - 1) == -5     # dims lifts out <= F


GROUP_BAD = {"null x": dict(x=None), "null out": dict(out=None), "n < 1": dict(n=0), "n > 2^31 - 1": dict(n=2 ** 31),
             "cols < 1": dict(cols=0), "cols > 64": dict(cols=65), "group < 1": dict(group=0)}


@pytest.mark.parametrize("case", list(GROUP_BAD))
def test_group_sums_rejects_invalid_arguments(lib, case):
    kw = dict(x=PTR, n=100, cols=2, group=7, out=PTR)
    kw.update(GROUP_BAD[case])
    assert lib.mtadgat_eval_group_sums(kw["x"], kw["n"], kw["cols"], kw["group"], kw["out"], None) == -1
    assert _err(lib)


def test_scratch_query(lib):
    sq = lib.mtadgat_eval_window_sse_scratch
    assert sq(1, 1) > 0
    for bad in ((0, 3), (-1, 3), (2 ** 31, 3), (10, 0), (10, -1), (10, 2049)):
        assert sq(*bad) == 0, bad
    sizes = [sq(b, 55) for b in (1, 4, 100, 8192, 65536, 2 ** 31 - 1)]
    assert sizes == sorted(sizes)                                        # a call's scratch serves every shorter call
    assert sq(2 ** 31 - 1, 55) == sq(65536, 55) <= 2048 * 2 * 55 * 8 + 2 * 55 * 8 + 64       # bounded: slabs, not windows
    assert sq(2 ** 31 - 1, 2048) <= 16 * (1 << 20)


def test_losses_entry_points_refuse_a_null_handle(lib):
    assert lib.mtadgat_series_losses_chunk(None) == 0
    assert lib.mtadgat_series_losses_workspace_bytes(None, 100) == 0
    assert lib.mtadgat_series_losses(None, PTR, 100, None, 0, 1, 10, None, PTR, PTR, PTR, 1 << 20, None) == -1
    assert _err(lib)


# ---- the reference itself -------------------------------------------------------------------------------------------------------
def _random_case(rng, n, W, out, F, dims=None, n_rows=None):
    n_rows = n_rows or n + W + 3
    series = rng.standard_normal((n_rows, F)).astype(np.float32)
    preds = rng.standard_normal((n, out)).astype(np.float32)
    recons = rng.standard_normal((n, W, out)).astype(np.float32)
    starts = rng.integers(0, n_rows - W, size=n)
    return preds, recons, series, starts, dims


def test_reference_window_sse_equals_a_naive_triple_loop():
    rng = np.random.default_rng(31)
    for n, W, out, F, dims in ((6, 5, 3, 7, [6, 0, 3]), (4, 3, 4, 4, None), (3, 1, 1, 1, None)):
        preds, recons, series, starts, dims = _random_case(rng, n, W, out, F, dims)
        got = loss_refs.window_sse(preds, recons, series, starts, dims)
        gotd = loss_refs.dim_sse(preds, recons, series, starts, dims)
        cols = list(range(out)) if dims is None else dims
        want, wantd = np.zeros((n, 2)), np.zeros((2, out))
        for w in range(n):
            for d in range(out):
                q = float(np.float32(preds[w, d] - series[starts[w] + W, cols[d]])) ** 2
                want[w, 0] += q
                wantd[0, d] += q
                for t in range(W):
                    q = float(np.float32(recons[w, t, d] - series[starts[w] + t, cols[d]])) ** 2
                    want[w, 1] += q
                    wantd[1, d] += q
        assert got.dtype == np.float64 and got.shape == (n, 2)
        assert np.all(np.abs(got[:, 0] - want[:, 0]) <= loss_refs.bound(out) * want[:, 0])
        assert np.all(np.abs(got[:, 1] - want[:, 1]) <= loss_refs.bound(W * out) * want[:, 1])
        assert np.all(np.abs(gotd[0] - wantd[0]) <= loss_refs.bound(n) * wantd[0])
        assert np.all(np.abs(gotd[1] - wantd[1]) <= loss_refs.bound(n * W) * wantd[1])


def test_reference_differences_are_float32():
    """(1 + 2^-23) - 2^-30 rounds back to 1 + 2^-23 in float32; a float64 difference of the same inputs would keep the 2^-30."""
    a, b = np.float32(1.0) + np.float32(2.0 ** -23), np.float32(2.0 ** -30)
    series = np.array([[b], [b]], dtype=np.float32)
    got = loss_refs.window_sse(np.array([[a]]), np.array([[[a]]]), series, [0])
    assert got[0, 0] == got[0, 1] == float(a) ** 2 != (float(a) - float(b)) ** 2
    big = np.float32(1e20)
    got = loss_refs.window_sse(np.array([[big]]), np.array([[[big]]]), np.array([[-big], [-big]]), [0])
    assert np.isfinite(got).all() and got[0, 0] == float(np.float32(big + big)) ** 2          # overflows float32, not float64


def test_reference_group_losses():
    rng = np.random.default_rng(32)
    W, out, n = 5, 3, 23
    wsse = rng.random((n, 2)) * 10.0
    glob = (np.sqrt(wsse[:, 0].sum() / (n * out)), np.sqrt(wsse[:, 1].sum() / (n * W * out)))
    for b in (None, n, n + 1, 1000):
        f, r, t = loss_refs.group_losses(wsse, W, out, b)
        assert abs(f - glob[0]) <= 1e-14 * glob[0] and abs(r - glob[1]) <= 1e-14 * glob[1] and t == f + r, b
    wsse[20:] *= 50.0                                                    # a ragged last batch of 3 noisy windows weighs as much as a full one
    glob = np.sqrt(wsse[:, 0].sum() / (n * out))
    f, r, t = loss_refs.group_losses(wsse, W, out, 10)
    by_hand = np.sqrt(np.mean([wsse[0:10, 0].sum() / (10 * out), wsse[10:20, 0].sum() / (10 * out), wsse[20:23, 0].sum() / (3 * out)]))
    assert abs(f - by_hand) <= 1e-14 * by_hand
    assert abs(f - glob) > 0.1 * glob
    assert np.array_equal(loss_refs.group_sums(wsse, 1), wsse)
    by7 = np.stack([wsse[i:i + 7].sum(0) for i in range(0, n, 7)])
    assert np.all(np.abs(loss_refs.group_sums(wsse, 7) - by7) <= loss_refs.bound(7) * by7)


def test_package_group_sums_follow_the_reference_order():
    import evaluation
    rng = np.random.default_rng(33)
    x = rng.random((1000, 2)) * np.exp(rng.standard_normal((1000, 2)) * 5)
    for g in (1, 7, 256, 300, 1000, 1001):
        assert np.array_equal(evaluation.group_sums(torch.from_numpy(x), g).numpy(), loss_refs.group_sums(x, g)), g


# ---- the CPU path of MTAD_GAT.series_losses against the restated Trainer.evaluate ---------------------------------------------
CPU_CASES = {"syn_v1_small": dict(dims=None, n=45, batch=16), "syn_v2_embed": dict(dims=[4, 0, 7], n=37, batch=10)}


def _series(case, n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n + case.kwargs["window_size"], case.kwargs["n_features"], generator=g)


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_cpu_series_losses_agree_with_the_restated_trainer_evaluate(name):
    import _torchpath
    cfg = CPU_CASES[name]
    case = helpers.Case(name)
    model = case.build_model()
    W, out = case.kwargs["window_size"], case.kwargs["out_dim"]
    series = _series(case, cfg["n"])
    got = model.series_losses(series, target_dims=cfg["dims"], batch_size=cfg["batch"])
    with _torchpath._eval_mode(model):
        f, r, t, wref = loss_refs.trainer_evaluate(lambda x: _torchpath.forward(model, x), series.numpy(), W, cfg["dims"], cfg["batch"])
    w = got.window_sse.numpy()
    assert got.n_windows == cfg["n"] == w.shape[0] and w.dtype == np.float64
    assert np.all(np.abs(w[:, 0] - wref[:, 0]) <= loss_refs.bound(out) * wref[:, 0])
    assert np.all(np.abs(w[:, 1] - wref[:, 1]) <= loss_refs.bound(W * out) * wref[:, 1])
    assert (got.forecast_loss, got.recon_loss, got.total_loss) == loss_refs.group_losses(w, W, out, cfg["batch"])
    assert tuple(got) == (got.forecast_loss, got.recon_loss, got.total_loss)
    # the epoch value of the reference: within the rounding of a few float64 operations of the restatement's
    for a, b in ((got.forecast_loss, f), (got.recon_loss, r), (got.total_loss, t)):
        assert abs(a - b) <= 1e-13 * b
    # the per-dimension errors: the same squares, summed the other way
    n = cfg["n"]
    d = got.dim_mse.numpy()
    assert d.shape == (2, out)
    assert abs(d[0].sum() * n - w[:, 0].sum()) <= loss_refs.bound(2 * n * out) * w[:, 0].sum()
    assert abs(d[1].sum() * n * W - w[:, 1].sum()) <= loss_refs.bound(2 * n * W * out) * w[:, 1].sum()


def test_cpu_series_losses_modes_and_arguments():
    case = helpers.Case("syn_v2_embed")
    model = case.build_model()
    W = case.kwargs["window_size"]
    series = _series(case, 20)
    dims = [4, 0, 7]
    ref = model.series_losses(series, target_dims=dims)
    model.train()
    try:
        got = model.series_losses(series, target_dims=dims)
        assert model.training and all(m.training for m in model.modules())
    finally:
        model.eval()
    assert torch.equal(got.window_sse, ref.window_sse) and got.total_loss == ref.total_loss          # eval-mode numbers: no dropout
    sub = model.series_losses(series, target_dims=dims, start=2, stride=3, count=5)
    assert torch.equal(sub.window_sse, model.series_losses(series, target_dims=dims, starts=[2, 5, 8, 11, 14]).window_sse)
    assert sub.n_windows == 5
    with pytest.raises(RuntimeError):
        model.series_losses(series)                                       # out_dim 3 != 9 features: target_dims wanted
    with pytest.raises(IndexError):
        model.series_losses(series, target_dims=[0, 1, 9])
    with pytest.raises(RuntimeError):
        model.series_losses(series, target_dims=dims, starts=[series.shape[0] - W])       # no target row
    with pytest.raises(RuntimeError):
        model.series_losses(series[:W], target_dims=dims)
    with pytest.raises(ValueError):
        model.series_losses(series, target_dims=dims, batch_size=0)


@pytest.mark.skipif(not os.path.isdir(os.environ.get("MTADGAT_REFERENCE", "")), reason="MTADGAT_REFERENCE (the reference tree) is not set")
def test_against_the_reference_trainer_evaluate():
    """The real Trainer.evaluate over the real SlidingWindowDataset: its float32 MSEs against series_losses' float64 ones."""
    ref_root = os.environ["MTADGAT_REFERENCE"]
    sys.path.insert(0, ref_root)
    try:
        from training import Trainer
        from utils import SlidingWindowDataset
    finally:
        sys.path.remove(ref_root)
    case = helpers.Case("syn_v1_small")
    model = case.build_model()
    W, F = case.kwargs["window_size"], case.kwargs["n_features"]
    series = _series(case, 45)
    loader = torch.utils.data.DataLoader(SlidingWindowDataset(series, W), batch_size=16, shuffle=False)
    trainer = Trainer(model, torch.optim.Adam(model.parameters()), W, F, target_dims=None, use_cuda=False, print_every=10 ** 9)
    f, r, t = trainer.evaluate(loader)
    got = model.series_losses(series, batch_size=16)
    for a, b in ((got.forecast_loss, f), (got.recon_loss, r), (got.total_loss, t)):
        assert abs(a - b) <= 1e-5 * abs(b)
