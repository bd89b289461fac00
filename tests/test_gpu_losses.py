"""Forecast / reconstruction losses on the GPU: the mtadgat_eval_window_sse and mtadgat_eval_group_sums kernels alone against
tests/loss_refs.py, and MTAD_GAT.series_losses (mtadgat_series_losses) against the same reference applied to what forward_series
returns for the same windows.  Every float64 sum is held to loss_refs.bound(terms) = terms * 2^-53 relative: the addends are
non-negative, so that bounds the distance between any two summation orders."""
import numpy as np
import pytest
import torch

import helpers
import loss_refs

pytestmark = pytest.mark.gpu


def _within(got, ref, terms, what=""):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(ref).all(), what
    err = np.abs(got - ref)
    assert np.all(err <= loss_refs.bound(terms) * ref), (what, float((err / np.maximum(ref, 1e-300)).max()), loss_refs.bound(terms))


def _check_all(wsse, dsse, preds, recons, series, starts, dims, what=""):
    n, W, out = recons.shape
    ref_w = loss_refs.window_sse(preds, recons, series, starts, dims)
    ref_d = loss_refs.dim_sse(preds, recons, series, starts, dims)
    _within(wsse[:, 0], ref_w[:, 0], out, what + " forecast")
    _within(wsse[:, 1], ref_w[:, 1], W * out, what + " recon")
    _within(dsse[0], ref_d[0], n, what + " dim forecast")
    _within(dsse[1], ref_d[1], n * W, what + " dim recon")


def _tensors(W, out, F, batch, seed, extra_rows=4, scale=1.0):
    rng = np.random.default_rng(seed)
    series = (rng.standard_normal((batch + W + extra_rows, F)) * scale).astype(np.float32)
    preds = (rng.standard_normal((batch, out)) * scale).astype(np.float32)
    recons = (rng.standard_normal((batch, W, out)) * scale).astype(np.float32)
    return preds, recons, series


def _gpu(dev, *arrays):
    return [torch.from_numpy(a).to(dev) for a in arrays]


SHAPES = {"1x1x1x1": (1, 1, 1, 1, None), "5x3x7x130 dims": (5, 3, 7, 130, [6, 0, 3]), "7x7x7x257": (7, 7, 7, 257, None),
          "4x260x260x9": (4, 260, 260, 9, None), "3x2048x2048x2": (3, 2048, 2048, 2, None), "512x1x2x5": (512, 1, 2, 5, None)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_against_the_reference(shape, gpu_device):
    import evaluation
    W, out, F, batch, dims = SHAPES[shape]
    preds, recons, series = _tensors(W, out, F, batch, seed=41)
    p, r, s = _gpu(gpu_device, preds, recons, series)
    wsse, dsse = evaluation.window_sse(p, r, s, dims=dims)
    assert wsse.dtype == torch.float64 and tuple(wsse.shape) == (batch, 2) and tuple(dsse.shape) == (2, out)
    _check_all(wsse.cpu().numpy(), dsse.cpu().numpy(), preds, recons, series, np.arange(batch), dims, shape)


# ---- one shape, (W, out, F, batch) = (5, 3, 7, 130), for the properties ------------------------------------------------------------
W0, OUT0, F0, N0, DIMS0 = 5, 3, 7, 130, [6, 0, 3]


@pytest.fixture(scope="module")
def base(gpu_device):
    """The tensors of the property tests, 3 * N0 spare series rows for stride 3, and the clean result."""
    import evaluation
    preds, recons, series = _tensors(W0, OUT0, F0, N0, seed=42, extra_rows=2 * N0 + 4)
    p, r, s = _gpu(gpu_device, preds, recons, series)
    wsse, dsse = evaluation.window_sse(p, r, s, dims=DIMS0)
    return dict(preds=preds, recons=recons, series=series, p=p, r=r, s=s, wsse=wsse.cpu().numpy(), dsse=dsse.cpu().numpy())


def test_series_with_a_row_stride(base, gpu_device):
    import evaluation
    wide = torch.full((base["s"].shape[0], F0 + 3), float("nan"), device=gpu_device)
    wide[:, :F0] = base["s"]
    view = wide[:, :F0]
    assert view.stride(0) == F0 + 3
    wsse, dsse = evaluation.window_sse(base["p"], base["r"], view, dims=DIMS0)
    assert np.array_equal(wsse.cpu().numpy(), base["wsse"]) and np.array_equal(dsse.cpu().numpy(), base["dsse"])


def test_stride_zero_gives_identical_rows(base):
    import evaluation
    r_same = base["r"][:1].expand(N0, W0, OUT0).contiguous()
    p_same = base["p"][:1].expand(N0, OUT0).contiguous()
    wsse, dsse = evaluation.window_sse(p_same, r_same, base["s"], start=9, stride=0, dims=DIMS0)
    w = wsse.cpu().numpy()
    assert np.array_equal(w, np.broadcast_to(w[:1], w.shape))
    _check_all(w, dsse.cpu().numpy(), p_same.cpu().numpy(), r_same.cpu().numpy(), base["series"], np.full(N0, 9), DIMS0, "stride 0")


def test_stride_three(base):
    import evaluation
    wsse, dsse = evaluation.window_sse(base["p"], base["r"], base["s"], start=2, stride=3, dims=DIMS0)
    _check_all(wsse.cpu().numpy(), dsse.cpu().numpy(), base["preds"], base["recons"], base["series"], 2 + 3 * np.arange(N0), DIMS0, "stride 3")


def test_explicit_starts_unsorted_with_repeats(base, gpu_device):
    import evaluation
    rng = np.random.default_rng(43)
    starts = rng.integers(0, base["series"].shape[0] - W0, size=N0)
    starts[[7, 64, 129]] = starts[3]
    p, r = base["p"].clone(), base["r"].clone()
    for j in (7, 64, 129):                             # repeated windows: the same outputs against the same rows
        p[j], r[j] = p[3], r[3]
    wsse, dsse = evaluation.window_sse(p, r, base["s"], starts=torch.from_numpy(starts).to(gpu_device), dims=DIMS0)
    w = wsse.cpu().numpy()
    for j in (7, 64, 129):
        assert np.array_equal(w[j], w[3]), j
    assert not np.all(np.diff(starts) >= 0)
    _check_all(w, dsse.cpu().numpy(), p.cpu().numpy(), r.cpu().numpy(), base["series"], starts, DIMS0, "starts")


def test_squares_that_overflow_float32(gpu_device):
    import evaluation
    preds, recons, series = _tensors(W0, OUT0, F0, N0, seed=44, scale=1e20)
    p, r, s = _gpu(gpu_device, preds, recons, series)
    wsse, dsse = evaluation.window_sse(p, r, s, dims=DIMS0)
    w = wsse.cpu().numpy()
    assert np.isfinite(w).all() and w.max() > float(np.finfo(np.float32).max)
    _check_all(w, dsse.cpu().numpy(), preds, recons, series, np.arange(N0), DIMS0, "1e20")


def test_a_nan_row_touches_exactly_the_windows_that_read_it(base):
    import evaluation
    R = 40
    s = base["s"].clone()
    s[R] = float("nan")
    wsse, _ = evaluation.window_sse(base["p"], base["r"], s, dims=DIMS0)
    w = wsse.cpu().numpy()
    starts = np.arange(N0)
    as_target = starts + W0 == R
    as_input = (starts <= R) & (R < starts + W0)
    assert as_target.sum() == 1 and as_input.sum() == W0
    assert np.array_equal(np.isnan(w[:, 0]), as_target) and np.array_equal(np.isnan(w[:, 1]), as_input)
    assert np.array_equal(w[~as_target, 0], base["wsse"][~as_target, 0]) and np.array_equal(w[~as_input, 1], base["wsse"][~as_input, 1])


def _raw(lib, p, r, s, n, W, out, F, start0, dims_t, accumulate, wsse, dsse, scratch):
    with torch.cuda.device(p.device):
        rc = lib.mtadgat_eval_window_sse(p.data_ptr(), r.data_ptr(), n, W, out, s.data_ptr(), s.shape[0], F, s.stride(0), None, start0, 1,
                                         dims_t.data_ptr(), accumulate, wsse.data_ptr(), dsse.data_ptr(), scratch.data_ptr(),
                                         scratch.numel() * 8, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mtadgat_last_error().decode()


def test_accumulate_over_two_calls(base, gpu_device):
    import evaluation
    lib = evaluation._lib()
    h = 70                                              # unequal halves: the second call runs fewer slabs than the first
    dims_t = torch.tensor(DIMS0, dtype=torch.int32, device=gpu_device)
    scratch = torch.full(((lib.mtadgat_eval_window_sse_scratch(h, OUT0) + 7) // 8,), float("nan"), dtype=torch.float64, device=gpu_device)
    wsse = torch.full((N0, 2), -1.0, dtype=torch.float64, device=gpu_device)
    dsse = torch.full((2, OUT0), -1.0, dtype=torch.float64, device=gpu_device)
    p, r = base["p"], base["r"]
    _raw(lib, p[:h], r[:h], base["s"], h, W0, OUT0, F0, 0, dims_t, 0, wsse[:h], dsse, scratch)
    first = dsse.cpu().numpy().copy()
    _raw(lib, p[h:], r[h:], base["s"], N0 - h, W0, OUT0, F0, h, dims_t, 1, wsse[h:], dsse, scratch)
    assert np.array_equal(wsse.cpu().numpy(), base["wsse"])                  # a window's pair depends on the window alone
    ref_h = loss_refs.dim_sse(base["preds"][:h], base["recons"][:h], base["series"], np.arange(h), DIMS0)
    _within(first[0], ref_h[0], h, "first half forecast")
    _within(first[1], ref_h[1], h * W0, "first half recon")
    _check_all(wsse.cpu().numpy(), dsse.cpu().numpy(), base["preds"], base["recons"], base["series"], np.arange(N0), DIMS0, "accumulate")


def test_identical_calls_give_identical_bits(base):
    import evaluation
    wsse, dsse = evaluation.window_sse(base["p"], base["r"], base["s"], dims=DIMS0)
    assert np.array_equal(wsse.cpu().numpy(), base["wsse"]) and np.array_equal(dsse.cpu().numpy(), base["dsse"])


@pytest.mark.parametrize("group", ["1", "7", "n", "n + 1"])
def test_group_sums(group, base, gpu_device):
    import evaluation
    g = {"1": 1, "7": 7, "n": N0, "n + 1": N0 + 1}[group]
    x = torch.from_numpy(base["wsse"]).to(gpu_device)
    got = evaluation.group_sums(x, g).cpu().numpy()
    ref = loss_refs.group_sums(base["wsse"], g)
    assert got.shape == ((N0 + g - 1) // g, 2)
    assert np.array_equal(got, ref)                                        # the order is part of the specification
    naive = np.stack([base["wsse"][i:i + g].sum(axis=0) for i in range(0, N0, g)])
    _within(got, naive, min(g, N0), "group sums")
    if g == 1:
        assert np.array_equal(got, base["wsse"])


# ---- through the model ------------------------------------------------------------------------------------------------------------
MODEL_CASES = {"syn_v1_small": dict(dims=None, n=150), "syn_v2_embed": dict(dims=[4, 0, 7], n=150), "msl_c1": dict(dims=0, n=320)}


class _Loaded:
    def __init__(self, name, dev):
        cfg = MODEL_CASES[name]
        self.name, self.dims, self.n = name, cfg["dims"], cfg["n"]
        if name == "msl_c1":
            self.case = helpers.WideCase(name)
            self.series = self.case.series.clone()
        else:
            self.case = helpers.Case(name)
            g = torch.Generator().manual_seed(5)
            self.series = torch.rand(self.n + self.case.kwargs["window_size"], self.case.kwargs["n_features"], generator=g)
        self.W, self.out = self.case.kwargs["window_size"], self.case.kwargs["out_dim"]
        self.dim_list = None if self.dims is None else ([self.dims] if isinstance(self.dims, int) else list(self.dims))
        self.model = self.case.build_model().to(dev)
        self.dev_series = self.series.to(dev)
        assert self.series.shape[0] - self.W == self.n

    def reference(self, **windows):
        """loss_refs applied to what forward_series returns for the windows: (window_sse, dim_sse, starts)."""
        p, r = self.model.forward_series(self.dev_series, **windows)
        n = p.shape[0]
        if "starts" in windows:
            starts = windows["starts"].cpu().numpy()
        else:
            starts = windows.get("start", 0) + windows.get("stride", 1) * np.arange(n)
        args = (p.cpu().numpy(), r.cpu().numpy(), self.series.numpy(), starts, self.dim_list)
        return loss_refs.window_sse(*args), loss_refs.dim_sse(*args), starts


@pytest.fixture(scope="module")
def loaded(gpu_device):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Loaded(name, gpu_device)
        return cache[name]
    return get


def _check_result(res, ref_w, ref_d, W, out, what):
    n = ref_w.shape[0]
    assert res.n_windows == n and res.window_sse.dtype == torch.float64 and res.window_sse.is_cuda
    w = res.window_sse.cpu().numpy()
    _within(w[:, 0], ref_w[:, 0], out, what + " forecast")
    _within(w[:, 1], ref_w[:, 1], W * out, what + " recon")
    d = res.dim_mse.cpu().numpy()
    # dim_mse = dim_sse / n and / (n W): one more rounding each, so one more term
    _within(d[0] * n, ref_d[0], n + 2, what + " dim forecast")
    _within(d[1] * (n * W), ref_d[1], n * W + 2, what + " dim recon")


@pytest.mark.parametrize("precision", ["auto", "fp32_strict"])
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_window_sse_of_the_model_equals_the_reference_on_forward_series(name, precision, loaded):
    L = loaded(name)
    L.model.precision = precision
    try:
        ref_w, ref_d, _ = L.reference(count=L.n)
        res = L.model.series_losses(L.dev_series, target_dims=L.dims)
    finally:
        L.model.precision = "auto"
    _check_result(res, ref_w, ref_d, L.W, L.out, f"{name} {precision}")
    assert (res.forecast_loss, res.recon_loss, res.total_loss) == loss_refs.group_losses(res.window_sse.cpu().numpy(), L.W, L.out, None)


def test_global_rmse_against_the_fixture_reference(loaded):
    L = loaded("msl_c1")
    res = L.model.series_losses(L.dev_series, target_dims=0)
    series = L.series.double()
    y = series[L.W:L.W + L.n, :1]
    x = torch.stack([series[i:i + L.W, :1] for i in range(L.n)])
    ref_f = float(torch.sqrt(((L.case.preds.double().reshape(L.n, 1) - y) ** 2).mean()))
    ref_r = float(torch.sqrt(((L.case.recons.double() - x) ** 2).mean()))
    print(f"msl_c1 forecast RMSE {res.forecast_loss!r} (reference {ref_f!r}), recon RMSE {res.recon_loss!r} (reference {ref_r!r})")
    assert abs(res.forecast_loss - ref_f) <= helpers.FP32_TOL
    assert abs(res.recon_loss - ref_r) <= helpers.FP32_TOL
    assert res.total_loss == res.forecast_loss + res.recon_loss


@pytest.mark.parametrize("batch_size", [256, 100])
def test_loader_batches(batch_size, loaded):
    L = loaded("msl_c1")
    res = L.model.series_losses(L.dev_series, target_dims=0, batch_size=batch_size)
    w = res.window_sse.cpu().numpy()
    assert (res.forecast_loss, res.recon_loss, res.total_loss) == loss_refs.group_losses(w, L.W, L.out, batch_size)
    glob = loss_refs.group_losses(w, L.W, L.out, None)
    assert res.forecast_loss != glob[0]                                    # 320 windows: a ragged last batch either way
    assert torch.equal(res.window_sse, L.model.series_losses(L.dev_series, target_dims=0).window_sse)


def test_window_selection_matches_forward_series(loaded, gpu_device):
    L = loaded("syn_v2_embed")
    starts = torch.tensor([17, 3, 3, 120, 149, 0, 64, 17], dtype=torch.int64, device=gpu_device)
    for what, kw in (("starts", dict(starts=starts)), ("stride 3", dict(start=2, stride=3, count=40)), ("count", dict(start=11, count=23))):
        ref_w, ref_d, st = L.reference(**kw)
        res = L.model.series_losses(L.dev_series, target_dims=L.dims, **kw)
        _check_result(res, ref_w, ref_d, L.W, L.out, what)
    res = L.model.series_losses(L.dev_series, target_dims=L.dims, starts=starts)
    w = res.window_sse.cpu().numpy()
    assert np.array_equal(w[1], w[2]) and np.array_equal(w[0], w[7])


def test_several_chunks(loaded):
    L = loaded("syn_v1_small")
    L.model.series_losses(L.dev_series)                 # (the engine exists)
    eng = L.model._engine
    before = eng.chunk_windows()
    eng.set_chunk_windows(64)
    try:
        if eng.series_losses_chunk() != 64:
            pytest.skip(f"mtadgat_series_losses_chunk reports {eng.series_losses_chunk()}, not the 64 this test cuts 150 windows by")
        res = L.model.series_losses(L.dev_series)
        again = L.model.series_losses(L.dev_series)
        refs = [L.reference(start=c0, count=min(64, L.n - c0)) for c0 in (0, 64, 128)]
        assert eng.series_losses_workspace_bytes(4 * 64) == eng.series_losses_workspace_bytes(64)
    finally:
        eng.set_chunk_windows(before)
    assert [r[0].shape[0] for r in refs] == [64, 64, 22]
    w = res.window_sse.cpu().numpy()
    ref_w = np.concatenate([r[0] for r in refs])
    _within(w[:, 0], ref_w[:, 0], L.out, "chunks forecast")
    _within(w[:, 1], ref_w[:, 1], L.W * L.out, "chunks recon")
    # the per-dimension sums of the chunks' squares, each chunk's own reference sum within its bound: so is their total
    ref_d = sum(r[1] for r in refs)
    d = res.dim_mse.cpu().numpy()
    _within(d[0] * L.n, ref_d[0], L.n + 4, "chunks dim forecast")
    _within(d[1] * (L.n * L.W), ref_d[1], L.n * L.W + 4, "chunks dim recon")
    assert torch.equal(res.window_sse, again.window_sse) and torch.equal(res.dim_mse, again.dim_mse)
    assert (res.forecast_loss, res.recon_loss) == (again.forecast_loss, again.recon_loss)


def test_workspace_does_not_grow_beyond_a_chunk(loaded):
    L = loaded("msl_c1")
    L.model.series_losses(L.dev_series, target_dims=0)
    eng = L.model._engine
    chunk = eng.series_losses_chunk()
    assert 1 <= chunk <= eng.chunk_windows() and chunk * L.W * L.out <= 2 ** 26
    assert eng.series_losses_workspace_bytes(4 * chunk) == eng.series_losses_workspace_bytes(chunk) > 0


def test_the_call_leaves_no_state(loaded, gpu_device):
    L = loaded("syn_v2_embed")
    x = L.case.x.to(gpu_device)
    p0, r0 = L.model(x)
    L.model.series_losses(L.dev_series, target_dims=L.dims)
    p1, r1 = L.model(x)
    assert torch.equal(p0, p1) and torch.equal(r0, r1)


def test_train_mode_gives_the_eval_numbers(loaded):
    L = loaded("syn_v1_small")
    ref = L.model.series_losses(L.dev_series, batch_size=64)
    L.model.train()
    try:
        res = L.model.series_losses(L.dev_series, batch_size=64)
        assert L.model.training and all(m.training for m in L.model.modules())
    finally:
        L.model.eval()
    assert torch.equal(res.window_sse, ref.window_sse) and torch.equal(res.dim_mse, ref.dim_mse)
    assert (res.forecast_loss, res.recon_loss, res.total_loss) == (ref.forecast_loss, ref.recon_loss, ref.total_loss)
