"""The series trainer on the GPU (fitting.SeriesTrainer; csrc/mtadgat_fit.hip): its four kernels alone against tests/fit_refs.py, and
the whole step held against the existing route -- model(x) in train mode, torch's sqrt(mse) + sqrt(mse), .backward() -- step by step:
before every step the comparison model is loaded from the trained one, so nothing drifts.

Tolerances: the gather is a copy (bitwise).  The cotangents, Adam's results and the step's parameters are ONE float32 rounding of a
float64 expression whose inputs agree to a few 2^-53, so they may differ from the specification by the rounding falling the other
way: 1 float32 ulp.  Float64 scalars formed by one or two correctly rounded operations from identical inputs: 4 * 2^-53 relative.
The squared gradient norm: loss_refs.bound(n), the distance between two summation orders of n non-negative addends.  Parameter
gradients of the step against the existing route's: train_route_cases.GATE_C per tensor -- both sides run the same forward and backward
kernels on the same bits, only the cotangents differ (by at most two float32 roundings per element) and the backward is linear in
them."""
import math

import numpy as np
import pytest
import torch

import fit_refs
import helpers
import loss_refs
import train_route_cases as tc

pytestmark = pytest.mark.gpu

REL64 = 4 * 2.0 ** -53
N_VALUES = (1, 3, 255, 256, 257, 4099)          # one lane, a few, around one round of the 256 lanes, two blocks of the norm


def _close64(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.all(np.abs(got - want) <= REL64 * np.abs(want)), (what, got, want)


def _ulp1(got, want, what=""):
    worst = float(np.max(fit_refs.ulps32(got, want))) if np.size(want) else 0.0
    assert worst <= 1.0, (what, worst)


def _dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _strided_series(dev, series, pad):
    """The series on the device with row stride F + pad."""
    n, F = series.shape
    base = torch.full((n, F + pad), 1e30, dtype=torch.float32, device=dev)
    base[:, :F] = _dev(dev, series)
    return base[:, :F]


def _starts(rng, n_rows, W, batch):
    """Window starts with 0, the last window that has a target row, and a duplicate among them (as far as the batch has room)."""
    s = rng.integers(0, n_rows - W, size=batch)
    for i, v in enumerate((n_rows - W - 1, 0, n_rows - W - 1)[:batch]):
        s[i] = v
    return s.astype(np.int64)


# ---- the gather --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("F", [1, 5, 8, 55])
def test_gather_equals_torch_indexing(F, pad, gpu_device):
    import _native
    rng = np.random.default_rng(100 * F + pad)
    for W in (3, 100):
        n_rows = W + 37
        series = rng.standard_normal((n_rows, F)).astype(np.float32)
        s = _strided_series(gpu_device, series, pad)
        assert s.stride(0) == F + pad
        for batch in (1, 7, 33):
            starts = _dev(gpu_device, _starts(rng, n_rows, W, batch))
            want = s[starts[:, None] + torch.arange(W, device=gpu_device)[None, :]]
            got = _native.fit_gather(s, starts, W)
            assert got.shape == (batch, W, F) and torch.equal(got, want), (W, batch)
            assert np.array_equal(got.cpu().numpy(), fit_refs.gather(series, starts.cpu().numpy(), W))
            # an output that is not 16-byte aligned: the scalar stores
            buf = torch.zeros(batch * W * F + 1, dtype=torch.float32, device=gpu_device)
            out = buf[1:].view(batch, W, F)
            _native.fit_gather(s, starts, W, out=out)
            assert torch.equal(out, want) and buf[0] == 0.0, (W, batch, "unaligned")


# ---- the loss cotangents -----------------------------------------------------------------------------------------------------------
LOSS_CASES = {"out1": (1, None), "out1 dims": (1, [3]), "out5": (5, None), "out5 dims": (5, [4, 0, 2, 2, 6])}


def _sums(p, r, s, starts, dims):
    import evaluation
    wsse, _ = evaluation.window_sse(p, r, s, starts=starts, dims=dims)
    return evaluation.group_sums(wsse, wsse.shape[0]).reshape(2)


@pytest.mark.parametrize("batch", [1, 7, 33])
@pytest.mark.parametrize("case", list(LOSS_CASES))
def test_loss_cotangents_against_the_reference(case, batch, gpu_device):
    import _native
    out, dims = LOSS_CASES[case]
    W, F, n_rows = 10, 7, 60
    rng = np.random.default_rng(7 * batch + out)
    series = rng.standard_normal((n_rows, F)).astype(np.float32)
    preds = rng.standard_normal((batch, out)).astype(np.float32)
    recons = rng.standard_normal((batch, W, out)).astype(np.float32)
    starts = _starts(rng, n_rows, W, batch)
    s, p, r, st = _strided_series(gpu_device, series, 3), _dev(gpu_device, preds), _dev(gpu_device, recons), _dev(gpu_device, starts)
    dims_dev = None if dims is None else torch.tensor(dims, dtype=torch.int32, device=gpu_device)
    sums = _sums(p, r, s, st, dims)
    dp, dr, rmse = _native.fit_loss_grad(p, r, s, st, sums, dims=dims_dev)
    want_p, want_r, want_rmse = fit_refs.loss_grad(preds, recons, series, starts, dims, sums=sums.cpu().numpy())
    _ulp1(dp.cpu().numpy(), want_p, "d_preds")
    _ulp1(dr.cpu().numpy(), want_r, "d_recons")
    _close64(rmse.cpu().numpy(), want_rmse, "rmse")
    # the sums themselves: the order of ordered_sum over per-window sums that lie within their own bound
    spec = fit_refs.batch_sums(preds, recons, series, starts, dims)
    assert np.all(np.abs(sums.cpu().numpy() - spec) <= loss_refs.bound(W * out + batch) * spec)
    # identical calls, identical bits
    dp2, dr2, rmse2 = _native.fit_loss_grad(p, r, s, st, sums, dims=dims_dev)
    assert torch.equal(dp, dp2) and torch.equal(dr, dr2) and torch.equal(rmse, rmse2)
    # all residuals zero: zero cotangents, not 0 / 0
    cols = list(range(out)) if dims is None else dims
    p0 = _dev(gpu_device, series[starts + W][:, cols])
    r0 = _dev(gpu_device, fit_refs.gather(series, starts, W)[:, :, cols])
    dp, dr, rmse = _native.fit_loss_grad(p0, r0, s, st, _sums(p0, r0, s, st, dims), dims=dims_dev)
    assert not dp.any() and not dr.any() and not rmse.any()


def test_loss_cotangents_of_a_sum_that_is_not_finite(gpu_device):
    import _native
    rng = np.random.default_rng(5)
    series = rng.standard_normal((30, 4)).astype(np.float32)
    preds, recons = rng.standard_normal((3, 4)).astype(np.float32), rng.standard_normal((3, 5, 4)).astype(np.float32)
    recons[1, 2, 3] = np.inf
    starts = np.array([0, 24, 7])
    s, p, r, st = (_dev(gpu_device, a) for a in (series, preds, recons, starts))
    dp, dr, rmse = _native.fit_loss_grad(p, r, s, st, _sums(p, r, s, st, None))
    assert torch.isnan(dr).all() and torch.isfinite(dp).all() and torch.isinf(rmse[1]) and torch.isfinite(rmse[0])


# ---- the gradient norm and the step record --------------------------------------------------------------------------------------------
def _state(dev, **fields):
    return torch.tensor([float(fields.get(k, 0.0)) for k in fit_refs.STATE_FIELDS], dtype=torch.float64, device=dev)


def _record(state):
    return dict(zip(fit_refs.STATE_FIELDS, state.cpu().numpy()))


@pytest.mark.parametrize("n", N_VALUES)
def test_norm_and_step_record(n, gpu_device):
    import _native
    rng = np.random.default_rng(n)
    g = (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 2)).astype(np.float32)
    gd = _dev(gpu_device, g)
    lr, betas = 2e-3, (0.9, 0.999)
    rmse = torch.tensor([0.25, 0.5], dtype=torch.float64, device=gpu_device)
    log = torch.full((4, 4), -1.0, dtype=torch.float64, device=gpu_device)
    spec_sq = fit_refs.grad_norm_sq(g)
    max_norm = 0.5 * math.sqrt(spec_sq)                                  # clipping bites
    state = _state(gpu_device)
    before = {}
    for t in (1, 2, 1000):
        if t == 1000:
            state = _state(gpu_device, t=999, calls=5)
            before = dict(t=999.0, calls=5.0)
        _native.fit_prepare(gd, rmse, state, log, lr, betas, max_norm)
        rec = _record(state)
        assert abs(rec["norm_sq"] - spec_sq) <= loss_refs.bound(n) * spec_sq, (t, rec["norm_sq"], spec_sq)
        want = fit_refs.prepare(before, rec["norm_sq"], (0.25, 0.5), lr, betas, max_norm)
        assert rec["t"] == t == want["t"] and rec["calls"] == want["calls"] and rec["applied"] == 1.0
        for k in ("clip", "step_size", "bc2s", "norm"):
            _close64(rec[k], want[k], (k, t))
        assert rec["clip"] < 1.0
        before = rec
    rows = log.cpu().numpy()
    for row in (0, 1):                                                   # calls 0, 1 and 5 -> rows 0, 1 and 5 mod 4 = 1
        assert rows[row, 0] == 0.25 and rows[row, 1] == 0.5 and rows[row, 3] == 1.0
        assert abs(rows[row, 2] - rec["norm"]) <= REL64 * rec["norm"]
    assert np.all(rows[2:] == -1.0)
    # without clipping: clip is exactly 1
    state = _state(gpu_device)
    _native.fit_prepare(gd, rmse, state, log, lr, betas, None)
    assert _record(state)["clip"] == 1.0


@pytest.mark.parametrize("n", [3, 4099])
def test_a_nan_gradient_is_skipped_or_reaches_the_parameters(n, gpu_device):
    import _native
    rng = np.random.default_rng(n)
    p, g, m = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    v = (rng.standard_normal(n) ** 2).astype(np.float32)
    g[n // 2] = np.nan
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    rmse = torch.tensor([0.25, 0.5], dtype=torch.float64, device=gpu_device)
    for skip in (True, False):
        pd, gd, md, vd = (_dev(gpu_device, a) for a in (p, g, m, v))
        state = _state(gpu_device, t=3, calls=3, clip=0.5, step_size=0.125, bc2s=0.75, applied=1)
        log = torch.zeros((8, 4), dtype=torch.float64, device=gpu_device)
        _native.fit_prepare(gd, rmse, state, log, lr, betas, 1.0, skip_nonfinite=skip)
        _native.fit_adam(pd, gd, md, vd, state, lr, betas, eps)
        rec, row = _record(state), log[3].cpu().numpy()
        assert rec["calls"] == 4 and np.isnan(row[2]) and row[0] == 0.25 and row[1] == 0.5
        if skip:
            assert rec["t"] == 3 and rec["applied"] == 0 and row[3] == 0
            assert (rec["clip"], rec["step_size"], rec["bc2s"]) == (0.5, 0.125, 0.75)
            for got, was in ((pd, p), (md, m), (vd, v)):
                assert np.array_equal(got.cpu().numpy().view(np.uint32), was.view(np.uint32))
        else:
            assert rec["t"] == 4 and rec["applied"] == 1 and row[3] == 1
            assert torch.isnan(pd).all()                                 # the clip factor is NaN: it reaches every parameter
    # a loss that is not finite is skipped as well
    state = _state(gpu_device)
    g[n // 2] = 0.0
    _native.fit_prepare(_dev(gpu_device, g), torch.tensor([np.inf, 0.5], dtype=torch.float64, device=gpu_device), state,
                        torch.zeros((8, 4), dtype=torch.float64, device=gpu_device), lr, betas, None, skip_nonfinite=True)
    assert _record(state)["applied"] == 0 and _record(state)["t"] == 0


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------
ADAM_CASES = {"plain": dict(), "weight_decay": dict(weight_decay=0.01), "decoupled": dict(weight_decay=0.01, decoupled=True),
              "clipped": dict(max_grad_norm=0.25), "all": dict(weight_decay=0.05, decoupled=True, max_grad_norm=0.25)}


def _adam_inputs(n, seed):
    """A third ordinary entries, a third with g = 0 (half of those with m = v = 0 too), a third with |g| around eps = 1e-8."""
    rng = np.random.default_rng(seed)
    p, g, m = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    v = (rng.standard_normal(n) ** 2).astype(np.float32)
    kind = np.arange(n) % 6
    g[(kind == 1) | (kind == 2)] = 0.0
    m[kind == 2] = 0.0
    v[kind == 2] = 0.0
    tiny = (kind == 3) | (kind == 4)
    g[tiny] = (rng.standard_normal(n)[tiny] * 1e-8).astype(np.float32)
    m[kind == 4] *= np.float32(1e-8)
    v[kind == 4] *= np.float32(1e-16)
    return p, g, m, v


@pytest.mark.parametrize("n", N_VALUES)
@pytest.mark.parametrize("case", list(ADAM_CASES))
def test_adam_against_the_reference(case, n, gpu_device):
    import _native
    cfg = ADAM_CASES[case]
    wd, decoupled, max_norm = cfg.get("weight_decay", 0.0), cfg.get("decoupled", False), cfg.get("max_grad_norm")
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    p, g, m, v = _adam_inputs(n, 31 * n + len(case))
    rmse = torch.tensor([0.25, 0.5], dtype=torch.float64, device=gpu_device)
    log = torch.zeros((8, 4), dtype=torch.float64, device=gpu_device)
    results = []
    for run in range(3):                                                 # two identical calls, then one on unaligned buffers
        bufs = []
        for a in (p, g, m, v):
            if run == 2:
                bufs.append(torch.cat([torch.zeros(1, device=gpu_device), _dev(gpu_device, a)])[1:])
            else:
                bufs.append(_dev(gpu_device, a))
        pd, gd, md, vd = bufs
        state = _state(gpu_device, t=4, calls=4)
        _native.fit_prepare(gd, rmse, state, log, lr, betas, max_norm)
        _native.fit_adam(pd, gd, md, vd, state, lr, betas, eps, wd, decoupled)
        results.append((pd.cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy(), _record(state)))
    rec = results[0][3]
    want_rec = fit_refs.prepare(dict(t=4.0, calls=4.0), rec["norm_sq"], (0.25, 0.5), lr, betas, max_norm)
    if max_norm is not None and n > 3:
        assert want_rec["clip"] < 1.0
    want = fit_refs.adam_step(p, g, m, v, want_rec, lr, betas, eps, wd, decoupled)
    for got, ref, what in zip(results[0][:3], want, ("p", "m", "v")):
        assert np.isfinite(got).all()
        _ulp1(got, ref, (case, n, what))
    for other in results[1:]:
        for a, b in zip(results[0][:3], other[:3]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the step against the existing route ------------------------------------------------------------------------------------------------
SHAPE = "w8"                                        # the GATv2 shape of train_route_cases.SHAPES with the fewest parameters and rows
STEP_MODELS = {
    "dims3": dict(kw={}, target_dims=[4, 0, 2]),                         # the shape as it stands: out_dim 3 of 6 features
    "all": dict(kw=dict(out_dim=6), target_dims=None),                   # the reference's default: every feature
    "dim1": dict(kw=dict(out_dim=1), target_dims=3),                     # out_dim = 1 != F through an int target_dims
}
N_ROWS, BATCH, K_STEPS, SEED = 80, 7, 4, 2024
HYPER = dict(lr=1e-2, weight_decay=1e-3, max_grad_norm=0.05)


def _kwargs(name, p_drop):
    return dict(tc.SHAPES[SHAPE], dropout=p_drop, **STEP_MODELS[name]["kw"])


def _new_model(name, p_drop, dev):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(tc.MODEL_SEED)
    model = MTAD_GAT(**_kwargs(name, p_drop))
    with torch.no_grad():
        model.feature_gat.bias.normal_()
        model.temporal_gat.bias.normal_()
    return model.to(dev).train()


def _series(dev, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N_ROWS, tc.SHAPES[SHAPE]["n_features"], generator=g).to(dev)


def _batches(dev, steps=K_STEPS):
    W = tc.SHAPES[SHAPE]["window_size"]
    rng = np.random.default_rng(77)
    return [_dev(dev, _starts(rng, N_ROWS, W, BATCH)) for _ in range(steps)]


def _trainer(model, name, **kw):
    import fitting
    return fitting.SeriesTrainer(model, target_dims=STEP_MODELS[name]["target_dims"], **{**HYPER, "seed": SEED, **kw})


def _flat_state(tr):
    return [t.cpu().numpy().copy() for t in (tr.params, tr.exp_avg, tr.exp_avg_sq)]


@pytest.mark.parametrize("p_drop", [0.0, tc.P_DROP])
@pytest.mark.parametrize("name", list(STEP_MODELS))
def test_step_against_the_existing_route(name, p_drop, gpu_device):
    import _hipgrad
    from mtad_gat import MTAD_GAT
    dev = gpu_device
    kw = _kwargs(name, p_drop)
    W, out = kw["window_size"], kw["out_dim"]
    dims = STEP_MODELS[name]["target_dims"]
    cols = None if dims is None else ([dims] if isinstance(dims, int) else dims)
    A = _new_model(name, p_drop, dev)
    tr = _trainer(A, name)
    assert all(p.data_ptr() == tr.params[o:o + n].data_ptr() for p, (o, n) in zip(_hipgrad.param_order(A), tr._spans))
    B = MTAD_GAT(**kw).to(dev).train()
    series = _series(dev)
    ser = series.cpu().numpy()
    for k, starts in enumerate(_batches(dev)):
        B.load_state_dict(A.state_dict())
        p0, m0, v0 = _flat_state(tr)
        rec0 = _record(tr.state)
        tr.step(series, starts)
        # the existing route on B
        x = series[starts[:, None] + torch.arange(W, device=dev)[None, :]]
        y = series[starts + W].unsqueeze(1)
        B.dropout_stream = (tr.step_seed(k), 0)
        B.zero_grad(set_to_none=True)
        preds, recons = B(x)
        assert B.grad_path == "hip"
        lf, lr_ = helpers.training_loss(preds, recons, x, y, cols)
        (lf + lr_).backward()
        # 1. the same outputs, bit for bit: the weights the step re-packed from the flat buffer are the parameters
        assert torch.equal(preds, tr.last_preds) and torch.equal(recons, tr.last_recons), k
        # 2. the gradients, per parameter tensor
        for (pname, pb), (o, n) in zip(zip(A._engine.flat_keys(), _hipgrad.param_order(B)), tr._spans):
            ga, gb = tr.grads[o:o + n].view(pb.shape), pb.grad
            s = gb.abs().max().item()
            assert (ga - gb).abs().max().item() <= tc.GATE_C * s + 1e-30, (k, pname)
        assert tr.grads.abs().max().item() > 0.0
        # 3. the parameters after the step: Adam's specification applied to the state before it and the step's gradients
        g = tr.grads.cpu().numpy()
        logged = tr.losses(last=1)[0]
        rec = fit_refs.prepare(rec0, fit_refs.grad_norm_sq(g), logged[:2], HYPER["lr"], (0.9, 0.999), HYPER["max_grad_norm"])
        want = fit_refs.adam_step(p0, g, m0, v0, rec, HYPER["lr"], (0.9, 0.999), 1e-8, HYPER["weight_decay"])
        for got, ref, what in zip(_flat_state(tr), want, ("params", "exp_avg", "exp_avg_sq")):
            _ulp1(got, ref, (k, what))
        assert _record(tr.state)["t"] == k + 1 and logged[3] == 1.0
        # (the norm: half the distance two orders of the sum of squares may have, and the square root's rounding)
        assert abs(logged[2] - rec["norm"]) <= (loss_refs.bound(g.size) + REL64) * rec["norm"]
        # 4. the logged losses: B's outputs through the loss reference
        starts_h = starts.cpu().numpy()
        wsse = loss_refs.window_sse(preds.detach().cpu().numpy(), recons.detach().cpu().numpy(), ser, starts_h, cols)
        f, r, _ = loss_refs.group_losses(wsse, W, out)
        _close64(logged[:2], [f, r], "logged losses")
        assert abs(lf.item() - f) <= 1e-5 * f and abs(lr_.item() - r) <= 1e-5 * r          # torch's float32 losses: the same quantities


def _run(name, p_drop, dev, steps, between=None, **kw):
    A = _new_model(name, p_drop, dev)
    tr = _trainer(A, name, **kw)
    series = _series(dev)
    for k, starts in enumerate(_batches(dev, steps)):
        if between is not None:
            between(k, A, tr, series)
        tr.step(series, starts)
    return A, tr


def test_two_trainers_from_one_seed_agree_bit_for_bit(gpu_device):
    _, t1 = _run("dims3", tc.P_DROP, gpu_device, K_STEPS)
    _, t2 = _run("dims3", tc.P_DROP, gpu_device, K_STEPS)
    for a, b in zip(_flat_state(t1), _flat_state(t2)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(t1.losses(), t2.losses()) and t1.losses().shape == (K_STEPS, 4)
    _, t3 = _run("dims3", tc.P_DROP, gpu_device, K_STEPS, seed=SEED + 1)       # another seed, other dropout masks
    assert not np.array_equal(_flat_state(t1)[0], _flat_state(t3)[0])


def test_a_resumed_run_continues_bit_for_bit(gpu_device):
    import copy
    from mtad_gat import MTAD_GAT
    dev = gpu_device
    _, straight = _run("dims3", tc.P_DROP, dev, K_STEPS)
    A, tr = _run("dims3", tc.P_DROP, dev, 2)
    model_sd = {k: v.cpu().clone() for k, v in A.state_dict().items()}
    opt_sd = copy.deepcopy(tr.state_dict())
    C = MTAD_GAT(**_kwargs("dims3", tc.P_DROP)).to(dev).train()
    C.load_state_dict(model_sd)
    trc = _trainer(C, "dims3", seed=1, lr=0.5)                            # overwritten by the checkpoint
    trc.load_state_dict(opt_sd)
    assert trc.lr == HYPER["lr"] and trc.seed == SEED
    series = _series(dev)
    for starts in _batches(dev)[2:]:
        trc.step(series, starts)
    for a, b in zip(_flat_state(straight), _flat_state(trc)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(straight.losses(), trc.losses())


def test_the_module_sees_the_step(gpu_device):
    from mtad_gat import MTAD_GAT
    dev = gpu_device
    A, tr = _run("all", 0.0, dev, 2)
    W = tc.SHAPES[SHAPE]["window_size"]
    x = _series(dev, seed=10)[:5 * W].reshape(5, W, -1).contiguous()
    A.eval()
    with torch.no_grad():
        got = A(x)
    fresh = MTAD_GAT(**_kwargs("all", 0.0))
    fresh.load_state_dict({k: v.cpu().clone() for k, v in A.state_dict().items()})
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = fresh(x)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # state_dict() and parameter identity survive the re-pointing
    named = dict(A.named_parameters())
    assert all(A.state_dict()[k].data_ptr() == named[k].data_ptr() for k in named)


def test_a_bf16_inference_call_between_steps_does_not_disturb_the_next(gpu_device):
    W = tc.SHAPES[SHAPE]["window_size"]

    def infer(k, model, tr, series):
        if k == 1:
            model.eval()
            with torch.no_grad():
                model(series[:3 * W].reshape(3, W, -1).contiguous().bfloat16())
            model.train()
    _, plain = _run("dims3", tc.P_DROP, gpu_device, 2)
    _, mixed = _run("dims3", tc.P_DROP, gpu_device, 2, between=infer)
    for a, b in zip(_flat_state(plain), _flat_state(mixed)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_in_place_edits_and_moves_are_adopted(gpu_device):
    """load_state_dict writes the parameters in place (their version counters move); .data re-pointing breaks the aliasing: the next
    step notices either by a host check and trains on the new values."""
    import _hipgrad
    dev = gpu_device
    A, tr = _run("dims3", 0.0, dev, 1)
    ref, tref = _run("dims3", 0.0, dev, 1)
    series, batches = _series(dev), _batches(dev)
    sd = {k: v.clone() for k, v in A.state_dict().items()}
    A.load_state_dict(sd)                                                # same values, moved counters
    with torch.no_grad():
        p = next(A.parameters())
        p.data = p.data.clone()                                          # same values, another allocation
    tr.step(series, batches[1])
    tref.step(series, batches[1])
    assert all(q.data_ptr() == tr.params[o:o + n].data_ptr() for q, (o, n) in zip(_hipgrad.param_order(A), tr._spans))
    assert torch.equal(tr.params, tref.params)


def test_refused_arguments(gpu_device):
    import _hipgrad
    import fitting
    from mtad_gat import MTAD_GAT
    dev = gpu_device
    A = _new_model("dims3", 0.0, dev)
    tr = _trainer(A, "dims3")
    limit = _hipgrad._chunk_windows(A._engine, dev)
    series = _series(dev)
    with pytest.raises(ValueError, match=str(limit)):
        tr.step(series, torch.zeros(limit + 1, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        tr.step(series, torch.zeros(0, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError):
        tr.step(series.cpu(), torch.zeros(3, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError):
        tr.step(series, torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        fitting.SeriesTrainer(MTAD_GAT(**_kwargs("dims3", 0.0)))          # a CPU model
    with pytest.raises(RuntimeError):
        fitting.SeriesTrainer(A)                                         # out_dim 3 of 6 features wants target_dims
    frozen = _new_model("dims3", 0.0, dev)
    frozen.conv.conv.bias.requires_grad_(False)
    with pytest.raises(RuntimeError):
        _trainer(frozen, "dims3")
    assert _record(tr.state)["calls"] == 0                               # nothing ran


# ---- fit -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dims3", "all"])
def test_fit_one_epoch(name, gpu_device):
    dev = gpu_device
    W = tc.SHAPES[SHAPE]["window_size"]
    A = _new_model(name, tc.P_DROP, dev)
    tr = _trainer(A, name)
    series, val = _series(dev), _series(dev, seed=11)[:50]
    out = tr.fit(series, val_series=val, epochs=1, batch_size=32, shuffle=False)
    steps = math.ceil((N_ROWS - W) / 32)
    assert _record(tr.state)["calls"] == steps == tr.losses().shape[0] and _record(tr.state)["t"] == steps
    rows = tr.losses(last=steps)
    f, r = (float(np.sqrt(np.mean(rows[:, j] ** 2))) for j in (0, 1))
    assert out["train_forecast"] == [f] and out["train_recon"] == [r] and out["train_total"] == [f + r]
    direct = A.series_losses(val, target_dims=STEP_MODELS[name]["target_dims"], batch_size=32)
    assert (out["val_forecast"], out["val_recon"], out["val_total"]) == ([direct.forecast_loss], [direct.recon_loss], [direct.total_loss])
    assert A.training
    # the epoch is the batches 0..31, 32..63, 64..71 in order: the same steps by hand
    B = _new_model(name, tc.P_DROP, dev)
    tb = _trainer(B, name)
    order = torch.arange(N_ROWS - W, device=dev)
    for lo in range(0, N_ROWS - W, 32):
        tb.step(series, order[lo:lo + 32])
    assert torch.equal(tb.params, tr.params)
    # a shuffled epoch: a permutation drawn on the device from the trainer's seed, reproducible
    o1 = _trainer(_new_model(name, tc.P_DROP, dev), name).fit(series, epochs=2, batch_size=32)
    o2 = _trainer(_new_model(name, tc.P_DROP, dev), name).fit(series, epochs=2, batch_size=32)
    assert o1 == o2 and len(o1["train_total"]) == 2 and o1["val_total"] == []
