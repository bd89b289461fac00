"""The series trainer without a GPU: the specification of its kernels (tests/fit_refs.py) held against torch in float64 -- Adam / AdamW
with clip_grad_norm_, the gradient of sqrt(mse) + sqrt(mse) --, the mtadgat_fit_* entry points' argument validation before anything
touches the device, and the module's name."""
import os
import sys

import numpy as np
import pytest
import torch

import fit_refs
import loss_refs

PTR = 0x10000            # a non-null, 16-byte aligned "device pointer": validation fails before it would be used


@pytest.fixture(scope="module")
def lib():
    import _native
    return _native.load_library()


def _err(lib):
    return lib.mtadgat_last_error().decode()


def test_symbols_and_bindings(lib):
    import _native
    for name in ("mtadgat_fit_gather", "mtadgat_fit_loss_grad", "mtadgat_fit_prepare", "mtadgat_fit_prepare_scratch", "mtadgat_fit_adam"):
        assert hasattr(lib, name), name
    assert _native.FIT_STATE_FIELDS == fit_refs.STATE_FIELDS
    for name in ("fit_gather", "fit_loss_grad", "fit_prepare", "fit_adam"):
        assert callable(getattr(_native, name))


# ---- Adam: the float64 algebra of the specification against torch's --------------------------------------------------------------------
ADAM_CASES = {
    "plain": dict(), "weight_decay": dict(weight_decay=0.01), "decoupled": dict(weight_decay=0.01, decoupled=True),
    "clip_bites": dict(max_grad_norm=0.5, clip_bites=True), "clip_idle": dict(max_grad_norm=1e9, clip_bites=False),
    "all": dict(weight_decay=0.05, decoupled=True, max_grad_norm=0.5, clip_bites=True, lr=3e-3, betas=(0.8, 0.99), eps=1e-6),
}
GRAD_SCALES = (1e-6, 1e-3, 1.0, 10.0)


@pytest.mark.parametrize("scale", GRAD_SCALES)
@pytest.mark.parametrize("name", list(ADAM_CASES))
def test_adam_step_agrees_with_torch_in_float64(name, scale):
    cfg = dict(ADAM_CASES[name])
    lr, betas, eps = cfg.pop("lr", 1e-3), cfg.pop("betas", (0.9, 0.999)), cfg.pop("eps", 1e-8)
    wd, decoupled, max_norm = cfg.get("weight_decay", 0.0), cfg.get("decoupled", False), cfg.get("max_grad_norm")
    if max_norm is not None and cfg["clip_bites"]:
        max_norm = max_norm * scale                                     # below the gradients' norm (~ 8 scale) at every scale
    rng = np.random.default_rng(17)
    shapes = [(7, 5), (11,), (3, 2, 4)]
    p0 = [rng.standard_normal(s) for s in shapes]
    tp = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in p0]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(tp, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p = np.concatenate([a.reshape(-1) for a in p0])
    m, v, rec = np.zeros_like(p), np.zeros_like(p), {}
    worst, bit = 0.0, False
    for step in range(5):
        gs = [rng.standard_normal(s) * scale * (1.0 + step) for s in shapes]
        for q, g in zip(tp, gs):
            q.grad = torch.from_numpy(g.copy())
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(tp, max_norm)
        opt.step()
        g = np.concatenate([a.reshape(-1) for a in gs])
        norm_sq = float(np.sum(g ** 2))
        rec = fit_refs.prepare(rec, norm_sq, (1.0, 1.0), lr, betas, max_norm)
        bit = bit or rec["clip"] < 1.0
        p, m, v = fit_refs.adam_step(p, g, m, v, rec, lr, betas, eps, wd, decoupled, store=np.float64)
        want = np.concatenate([q.detach().numpy().reshape(-1) for q in tp])
        worst = max(worst, float(np.max(np.abs(p - want) / np.abs(want))))
    assert rec["t"] == 5 and rec["calls"] == 5
    if max_norm is not None:
        assert bit == cfg["clip_bites"]
    assert worst <= 1e-12, worst


def test_adam_step_storage_and_skipped_steps():
    rng = np.random.default_rng(3)
    p, g = rng.standard_normal(9).astype(np.float32), rng.standard_normal(9).astype(np.float32)
    m, v = np.zeros(9, np.float32), np.zeros(9, np.float32)
    rec = fit_refs.prepare({}, fit_refs.grad_norm_sq(g), (0.5, 0.5), 1e-3, (0.9, 0.999))
    p64, m64, v64 = fit_refs.adam_step(p, g, m, v, rec, 1e-3, (0.9, 0.999), 1e-8, store=np.float64)
    p32, m32, v32 = fit_refs.adam_step(p, g, m, v, rec, 1e-3, (0.9, 0.999), 1e-8)
    for a32, a64 in ((p32, p64), (m32, m64), (v32, v64)):
        assert a32.dtype == np.float32 and np.array_equal(a32, a64.astype(np.float32))           # ONE rounding of the float64 result
    # g = 0 with v = 0: m / (0 / bc2s + eps) = 0, nothing moves
    z = np.zeros(9, np.float32)
    pz, mz, vz = fit_refs.adam_step(p, z, z, z, rec, 1e-3, (0.9, 0.999), 1e-8)
    assert np.array_equal(pz, p) and not mz.any() and not vz.any()
    # a non-finite norm under skip_nonfinite: t stays, nothing is applied; without it the NaN goes through
    bad = fit_refs.prepare(rec, np.nan, (0.5, 0.5), 1e-3, (0.9, 0.999), skip_nonfinite=True)
    assert bad["applied"] == 0 and bad["t"] == rec["t"] and bad["calls"] == rec["calls"] + 1 and bad["step_size"] == rec["step_size"]
    same = fit_refs.adam_step(p, g, m, v, bad, 1e-3, (0.9, 0.999), 1e-8)
    assert np.array_equal(same[0], p) and np.array_equal(same[1], m) and np.array_equal(same[2], v)
    assert fit_refs.prepare(rec, 1.0, (np.inf, 0.5), 1e-3, (0.9, 0.999), skip_nonfinite=True)["applied"] == 0
    thru = fit_refs.prepare(rec, np.nan, (0.5, 0.5), 1e-3, (0.9, 0.999), 1.0)
    assert thru["applied"] == 1 and thru["t"] == rec["t"] + 1 and np.isnan(thru["clip"])


def test_int_power_and_the_step_sizes():
    for b in (0.9, 0.999, 0.5, 0.0):
        for t in (1, 2, 3, 7, 1000, 100000):
            want = float(torch.tensor(b, dtype=torch.float64) ** t)
            # a rounding made at exponent e is carried to the power t / e by the squarings after it: at most ~t roundings' worth
            assert abs(float(fit_refs.int_power(b, t)) - want) <= 2 * t * 2.0 ** -53 * want, (b, t)
        assert fit_refs.int_power(b, 1) == b and fit_refs.int_power(b, 0) == 1.0
    rec = fit_refs.prepare({"t": 999.0, "calls": 999.0}, 4.0, (0.1, 0.2), 1e-3, (0.9, 0.999), 1.0)
    assert rec["t"] == 1000 and rec["norm"] == 2.0 and rec["clip"] == 1.0 / (2.0 + 1e-6)
    assert rec["step_size"] == 1e-3 / (1.0 - fit_refs.int_power(0.9, 1000)) and rec["bc2s"] == np.sqrt(1.0 - fit_refs.int_power(0.999, 1000))


def test_grad_norm_sq_order():
    rng = np.random.default_rng(5)
    for n in (1, 3, 255, 256, 257, 4099, 9000):
        g = (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 3)).astype(np.float32)
        got, want = fit_refs.grad_norm_sq(g), float(np.sum(g.astype(np.float64) ** 2))
        assert abs(got - want) <= loss_refs.bound(n) * want, n
    # the order is the specification: a block's lanes, then the blocks
    g = rng.standard_normal(4099).astype(np.float32)
    sq = g.astype(np.float64) ** 2
    by_hand = loss_refs.ordered_sum(np.array([[loss_refs.ordered_sum(sq[:4096, None])[0]], [loss_refs.ordered_sum(sq[4096:, None])[0]]]))[0]
    assert fit_refs.grad_norm_sq(g) == by_hand


# ---- the loss cotangents against autograd ------------------------------------------------------------------------------------------
def _grid(rng, shape):
    """float32 values on the grid 2^-10 in [-4, 4): every difference of two of them is exact in float32."""
    return (rng.integers(-4096, 4096, size=shape) / 1024.0).astype(np.float32)


@pytest.mark.parametrize("dims", [None, [4, 0, 2]])
def test_loss_grad_agrees_with_autograd_in_float64(dims):
    rng = np.random.default_rng(11)
    b, W, F = 7, 5, 6
    out = F if dims is None else len(dims)
    series, preds, recons = _grid(rng, (40, F)), _grid(rng, (b, out)), _grid(rng, (b, W, out))
    starts = np.array([0, 34, 3, 3, 17, 20, 9])
    dp, dr, rmse = fit_refs.loss_grad(preds, recons, series, starts, dims, store=np.float64)
    dp32, dr32, _ = fit_refs.loss_grad(preds, recons, series, starts, dims)
    cols = list(range(F)) if dims is None else dims
    tp_ = torch.from_numpy(preds).double().requires_grad_(True)
    tr_ = torch.from_numpy(recons).double().requires_grad_(True)
    s64 = torch.from_numpy(series).double()
    x = s64[torch.from_numpy(starts)[:, None] + torch.arange(W)[None, :]][:, :, cols]
    y = s64[torch.from_numpy(starts) + W][:, cols]
    mse = torch.nn.MSELoss()
    lf, lr_ = torch.sqrt(mse(y, tp_)), torch.sqrt(mse(x, tr_))
    (lf + lr_).backward()
    assert abs(rmse[0] - lf.item()) <= 1e-12 * lf.item() and abs(rmse[1] - lr_.item()) <= 1e-12 * lr_.item()
    for mine, auto, stored in ((dp, tp_.grad.numpy(), dp32), (dr, tr_.grad.numpy(), dr32)):
        assert mine.dtype == np.float64 and np.max(np.abs(mine - auto)) <= 1e-12 * np.abs(auto).max()
        assert stored.dtype == np.float32 and np.array_equal(stored, mine.astype(np.float32))    # the kernel's value: ONE rounding of it


def test_loss_grad_of_zero_residuals_is_zero():
    rng = np.random.default_rng(12)
    series = rng.standard_normal((20, 3)).astype(np.float32)
    starts = np.array([0, 5, 14])
    recons = fit_refs.gather(series, starts, 5)
    preds = series[starts + 5]
    dp, dr, rmse = fit_refs.loss_grad(preds, recons, series, starts)
    assert not dp.any() and not dr.any() and not rmse.any() and np.isfinite(dp).all() and np.isfinite(dr).all()
    # one head at zero, the other not: only that head's cotangent vanishes
    dp, dr, rmse = fit_refs.loss_grad(preds + 1.0, recons, series, starts)
    assert dp.all() and not dr.any() and rmse[0] > 0.0 and rmse[1] == 0.0
    # a sum that is not finite hides nothing
    bad = recons.copy()
    bad[1, 2, 0] = np.inf
    dp, dr, rmse = fit_refs.loss_grad(preds + 1.0, bad, series, starts)
    assert np.isnan(dr).all() and np.isfinite(dp).all() and np.isinf(rmse[1])


def test_reference_gather():
    series = np.arange(40, dtype=np.float32).reshape(8, 5)
    x = fit_refs.gather(series, [0, 5, 5], 3)
    assert x.shape == (3, 3, 5) and np.array_equal(x[0], series[0:3]) and np.array_equal(x[1], series[5:8]) and np.array_equal(x[1], x[2])


# ---- argument validation of the entry points: status -1 and a message, before anything touches the device ---------------------------
def _gather(lib, series=PTR, n_rows=100, F=5, ld=5, starts=PTR, batch=7, W=10, x=PTR):
    return lib.mtadgat_fit_gather(series, n_rows, F, ld, starts, batch, W, x, None)


GATHER_BAD = {"null series": dict(series=None), "null starts": dict(starts=None), "null x": dict(x=None), "batch 0": dict(batch=0),
              "batch > 2^31 - 1": dict(batch=2 ** 31), "W < 1": dict(W=0), "W > 512": dict(W=513, n_rows=10000), "F < 1": dict(F=0),
              "ld_series < F": dict(ld=4), "series shorter than W": dict(n_rows=9)}


@pytest.mark.parametrize("case", list(GATHER_BAD))
def test_gather_rejects_invalid_arguments(lib, case):
    assert _gather(lib, **GATHER_BAD[case]) == -1
    assert "fit_gather" in _err(lib)


def _loss_grad(lib, preds=PTR, recons=PTR, batch=7, W=10, out=3, series=PTR, n_rows=100, F=5, ld=5, starts=PTR, dims=None, sums=PTR,
               d_preds=PTR, d_recons=PTR, rmse=PTR):
    return lib.mtadgat_fit_loss_grad(preds, recons, batch, W, out, series, n_rows, F, ld, starts, dims, sums, d_preds, d_recons, rmse, None)


LOSS_BAD = {"null preds": dict(preds=None), "null recons": dict(recons=None), "null series": dict(series=None), "null starts": dict(starts=None),
            "null sums": dict(sums=None), "null d_preds": dict(d_preds=None), "null d_recons": dict(d_recons=None), "null rmse": dict(rmse=None),
            "batch 0": dict(batch=0), "out_dim < 1": dict(out=0), "out_dim > 2048": dict(out=2049, dims=PTR), "W < 1": dict(W=0),
            "W > 512": dict(W=513, n_rows=10000), "ld_series < F": dict(ld=4), "out_dim > F without dims": dict(out=6),
            "series shorter than W + 1": dict(n_rows=10)}


@pytest.mark.parametrize("case", list(LOSS_BAD))
def test_loss_grad_rejects_invalid_arguments(lib, case):
    assert _loss_grad(lib, **LOSS_BAD[case]) == -1
    assert "fit_loss_grad" in _err(lib)


def _prepare(lib, grads=PTR, n=1000, rmse=PTR, lr=1e-3, b1=0.9, b2=0.999, max_norm=-1.0, skip=0, state=PTR, log=PTR, capacity=16, scratch=PTR,
             scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = max(lib.mtadgat_fit_prepare_scratch(n), 8)
    return lib.mtadgat_fit_prepare(grads, n, rmse, lr, b1, b2, max_norm, skip, state, log, capacity, scratch, scratch_bytes, None)


PREPARE_BAD = {"null grads": (dict(grads=None), -1), "null rmse": (dict(rmse=None), -1), "null state": (dict(state=None), -1),
               "null log": (dict(log=None), -1), "null scratch": (dict(scratch=None), -1), "n 0": (dict(n=0), -1),
               "n > 2^31 - 1": (dict(n=2 ** 31), -1), "negative lr": (dict(lr=-1e-3), -1), "NaN lr": (dict(lr=float("nan")), -1),
               "beta1 = 1": (dict(b1=1.0), -1), "beta1 < 0": (dict(b1=-0.1), -1), "beta2 = 1": (dict(b2=1.0), -1), "beta2 NaN": (dict(b2=float("nan")), -1),
               "NaN max_norm": (dict(max_norm=float("nan")), -1), "skip_nonfinite not 0 / 1": (dict(skip=2), -1), "capacity 0": (dict(capacity=0), -1),
               "scratch one byte short": (dict(n=10000, scratch_bytes=23), -5), "misaligned scratch": (dict(scratch=PTR + 4), -5)}


@pytest.mark.parametrize("case", list(PREPARE_BAD))
def test_prepare_rejects_invalid_arguments(lib, case):
    kw, status = PREPARE_BAD[case]
    assert _prepare(lib, **kw) == status
    assert "fit_prepare" in _err(lib)


def test_prepare_scratch_query(lib):
    sq = lib.mtadgat_fit_prepare_scratch
    assert sq(0) == 0 and sq(-1) == 0 and sq(2 ** 31) == 0
    assert sq(1) == sq(4096) == 8 and sq(4097) == 16 and sq(10000) == 24
    assert sq(2 ** 31 - 1) == 8 * ((2 ** 31 - 1 + fit_refs.NORM_CHUNK - 1) // fit_refs.NORM_CHUNK)


def _adam(lib, p=PTR, g=PTR, m=PTR, v=PTR, n=1000, state=PTR, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=0):
    return lib.mtadgat_fit_adam(p, g, m, v, n, state, lr, b1, b2, eps, wd, decoupled, None)


ADAM_BAD = {"null params": dict(p=None), "null grads": dict(g=None), "null exp_avg": dict(m=None), "null exp_avg_sq": dict(v=None),
            "null state": dict(state=None), "n 0": dict(n=0), "negative lr": dict(lr=-1.0), "beta1 = 1": dict(b1=1.0), "beta2 < 0": dict(b2=-0.5),
            "negative eps": dict(eps=-1e-8), "NaN eps": dict(eps=float("nan")), "negative weight decay": dict(wd=-0.1),
            "decoupled not 0 / 1": dict(decoupled=2)}


@pytest.mark.parametrize("case", list(ADAM_BAD))
def test_adam_rejects_invalid_arguments(lib, case):
    assert _adam(lib, **ADAM_BAD[case]) == -1
    assert "fit_adam" in _err(lib)


# ---- the module ------------------------------------------------------------------------------------------------------------------------
def test_import_fitting_does_not_shadow_the_reference_training_module():
    """The reference's train.py does `from training import Trainer` with this package flat on sys.path: no module of the package may
    answer to that name."""
    import fitting
    pkg = os.path.dirname(os.path.abspath(fitting.__file__))
    assert hasattr(fitting, "SeriesTrainer") and fitting.__name__ == "fitting"
    assert not any(os.path.splitext(f)[0] == "training" for f in os.listdir(pkg))
    mod = sys.modules.get("training")
    assert mod is None or os.path.dirname(os.path.abspath(getattr(mod, "__file__", ""))) != pkg


def test_step_seed_is_a_pure_function_and_a_cpu_model_is_refused():
    import fitting
    from mtad_gat import MTAD_GAT
    tr = object.__new__(fitting.SeriesTrainer)
    tr.seed = 1234
    seeds = [tr.step_seed(k) for k in range(64)]
    assert seeds == [tr.step_seed(k) for k in range(64)] and len(set(seeds)) == 64 and all(0 <= s < 2 ** 62 for s in seeds)
    tr.seed = 1235
    assert tr.step_seed(0) != seeds[0]
    model = MTAD_GAT(n_features=4, window_size=6, out_dim=4, kernel_size=3, gru_hid_dim=8, forecast_hid_dim=8, recon_hid_dim=8)
    with pytest.raises(RuntimeError, match="GPU"):
        fitting.SeriesTrainer(model)
