"""Training on gappy, concatenated series without a GPU: the specification (tests/fit_mask_refs.py) held against a per-start loop,
against the unmasked specifications it must reduce to, and against torch's autograd in float64; the new entry points' argument
validation before anything touches the device; the host-side checks of fitting.training_windows."""
import math

import numpy as np
import pytest
import torch

import fit_mask_refs as fm
import fit_refs
import loss_refs

PTR = 0x10000            # a non-null, 16-byte aligned "device pointer": validation fails before it would be used
W8, F6, N80, LENGTHS = 8, 6, 80, [31, 5, 44]


@pytest.fixture(scope="module")
def lib():
    import _native
    return _native.load_library()


def _err(lib):
    return lib.mtadgat_last_error().decode()


def _grid(rng, shape):
    """float32 values on the grid 2^-10 in [-4, 4): every difference of two of them is exact in float32."""
    return (rng.integers(-4096, 4096, size=shape) / 1024.0).astype(np.float32)


# ---- the sampler's specification -------------------------------------------------------------------------------------------------------
def _brute(n_rows, W, F, lengths, age, max_age, dims, min_count):
    offs = fm.part_offsets(lengths, n_rows)
    cols = range(F) if dims is None else dims
    keep = []
    for s in range(n_rows - W):
        part = [p for p in range(len(offs) - 1) if offs[p] <= s < offs[p + 1]][0]
        if s + W >= offs[part + 1]:
            continue
        if age is not None and not any(age[s + W][c] <= max_age for c in cols):
            continue
        seen = W * F if age is None else sum(int(age[r][c] <= max_age) for r in range(s, s + W) for c in range(F))
        if seen >= min_count:
            keep.append(s)
    return np.array(keep, dtype=np.int64)


@pytest.mark.parametrize("dims,max_age", [([4, 0, 2], 0), ([3], 0), ([4, 0, 2], 2), (None, 1)])
def test_windows_against_a_loop_over_the_starts(dims, max_age):
    _, age = fm.reference_gaps(N80, F6, LENGTHS)
    for min_observed in (0.0, 0.5, 0.8, 1.0):
        mc = math.ceil(min_observed * W8 * F6)
        assert np.array_equal(fm.windows(N80, W8, F6, LENGTHS, age, max_age, dims, mc), _brute(N80, W8, F6, LENGTHS, age, max_age, dims, mc))
    assert np.array_equal(fm.windows(N80, W8, F6, None, age, max_age, dims, 24), _brute(N80, W8, F6, None, age, max_age, dims, 24))
    assert np.array_equal(fm.windows(N80, W8, F6, LENGTHS, None, max_age, dims, 48), _brute(N80, W8, F6, LENGTHS, None, max_age, dims, 48))
    # parts of no rows and a last part shorter than a window
    lengths = [0, 20, 0, 0, 53, 7]
    assert np.array_equal(fm.windows(N80, W8, F6, lengths, age, max_age, dims, 10), _brute(N80, W8, F6, lengths, age, max_age, dims, 10))


def test_the_reference_pattern_exercises_every_rule():
    """The counts the GPU tests rely on: of the 72 starts 13 fall to the seam rule; every rule removes and keeps windows."""
    _, age = fm.reference_gaps(N80, F6, LENGTHS)
    table = {((4, 0, 2), 0): (10, [49, 44, 15, 0]), ((3,), 0): (19, [40, 35, 13, 0]), ((4, 0, 2), 2): (6, [53, 49, 46, 28])}
    for (dims, max_age), (target_fall, kept) in table.items():
        same, target, _ = fm.rule_masks(N80, W8, F6, LENGTHS, age, max_age, list(dims), 0)
        assert same.size == 72 and int((~same).sum()) == 13 and int((same & ~target).sum()) == target_fall
        got = [fm.windows(N80, W8, F6, LENGTHS, age, max_age, list(dims), math.ceil(m * W8 * F6)).size for m in (0.0, 0.5, 0.8, 1.0)]
        assert got == kept
    assert np.array_equal(fm.windows(N80, W8, F6), np.arange(72))             # nothing given: every start
    assert fm.windows(W8, W8, F6).size == 0                                  # a series of one window has no target row


def test_age_of_counts_per_part():
    missing = np.zeros((7, 1), dtype=bool)
    missing[[1, 2, 3, 4, 6], 0] = True
    assert fm.age_of(missing)[:, 0].tolist() == [0, 1, 2, 3, 4, 0, 1]
    assert fm.age_of(missing, [3, 4])[:, 0].tolist() == [0, 1, 2, 1, 2, 0, 1]


# ---- the sums and cotangents -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [None, [4, 0, 2]])
def test_all_observed_is_the_unmasked_specification(dims):
    rng = np.random.default_rng(3)
    b, W, F = 7, 5, 6
    out = F if dims is None else len(dims)
    series, preds, recons = (rng.standard_normal(s).astype(np.float32) for s in ((40, F), (b, out), (b, W, out)))
    starts = np.array([0, 34, 3, 3, 17, 20, 9])
    age = np.zeros((40, F), dtype=np.int32)
    ws = fm.window_sums(preds, recons, series, starts, age, 0, dims)
    assert np.array_equal(ws[:, :2], loss_refs.window_sse(preds, recons, series, starts, dims))
    assert np.all(ws[:, 2] == out) and np.all(ws[:, 3] == W * out)
    assert np.array_equal(fm.dim_sums(preds, recons, series, starts, age, 0, dims)[:2], loss_refs.dim_sse(preds, recons, series, starts, dims))
    got, want = fm.loss_grad(preds, recons, series, starts, age, 0, dims), fit_refs.loss_grad(preds, recons, series, starts, dims)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    f, r, t = fm.group_losses(ws, 3)
    assert (f, r, t) == loss_refs.group_losses(ws[:, :2], W, out, 3)
    # max_age: ages up to it count as observed
    assert np.array_equal(fm.window_sums(preds, recons, series, starts, age + 2, 2, dims), ws)


@pytest.mark.parametrize("dims", [None, [4, 0, 2]])
def test_loss_grad_agrees_with_autograd_in_float64(dims):
    rng = np.random.default_rng(11)
    b, W, F = 7, 5, 6
    out = F if dims is None else len(dims)
    series, preds, recons = _grid(rng, (40, F)), _grid(rng, (b, out)), _grid(rng, (b, W, out))
    starts = np.array([0, 34, 3, 3, 17, 20, 9])
    age = (rng.random((40, F)) < 0.3).astype(np.int32) * rng.integers(1, 4, size=(40, F)).astype(np.int32)
    series_nan = series.copy()
    series_nan[age > 0] = np.nan                       # what the mask hides may be anything: it reaches neither sum nor cotangent
    dp, dr, rmse = fm.loss_grad(preds, recons, series_nan, starts, age, 0, dims, store=np.float64)
    dp32, dr32, _ = fm.loss_grad(preds, recons, series_nan, starts, age, 0, dims)
    cols = list(range(F)) if dims is None else dims
    st = torch.from_numpy(starts)
    tp_ = torch.from_numpy(preds).double().requires_grad_(True)
    tr_ = torch.from_numpy(recons).double().requires_grad_(True)
    s64, m = torch.from_numpy(series).double(), torch.from_numpy(age <= 0)
    rows = st[:, None] + torch.arange(W)[None, :]
    x, mx = s64[rows][:, :, cols], m[rows][:, :, cols].double()
    y, my = s64[st + W][:, cols], m[st + W][:, cols].double()
    assert 0 < mx.sum() < mx.numel() and 0 < my.sum() < my.numel()
    lf = torch.sqrt((my * (tp_ - y) ** 2).sum() / my.sum())
    lr_ = torch.sqrt((mx * (tr_ - x) ** 2).sum() / mx.sum())
    (lf + lr_).backward()
    assert abs(rmse[0] - lf.item()) <= 1e-12 * lf.item() and abs(rmse[1] - lr_.item()) <= 1e-12 * lr_.item()
    for mine, auto, stored in ((dp, tp_.grad.numpy(), dp32), (dr, tr_.grad.numpy(), dr32)):
        assert mine.dtype == np.float64 and np.isfinite(mine).all() and np.max(np.abs(mine - auto)) <= 1e-12 * np.abs(auto).max()
        assert stored.dtype == np.float32 and np.array_equal(stored, mine.astype(np.float32))
    assert not dp[my.numpy() == 0].any() and not dr[mx.numpy() == 0].any()
    f, r, _ = fm.group_losses(fm.window_sums(preds, recons, series_nan, starts, age, 0, dims))
    assert abs(f - lf.item()) <= 1e-12 * f and abs(r - lr_.item()) <= 1e-12 * r


def test_a_head_without_observed_terms_and_a_head_at_zero_give_zero_cotangents():
    rng = np.random.default_rng(12)
    series = rng.standard_normal((20, 3)).astype(np.float32)
    starts = np.array([0, 5, 14])
    W = 5
    preds, recons = series[starts + W] + 1.0, fit_refs.gather(series, starts, W).copy()
    age = np.zeros((20, 3), dtype=np.int32)
    # rmse == 0: the reconstruction head is exact
    dp, dr, rmse = fm.loss_grad(preds, recons, series, starts, age)
    assert dp.all() and not dr.any() and rmse[0] > 0 and rmse[1] == 0 and np.isfinite(dr).all()
    # N == 0: every forecast target is unobserved
    age[starts + W] = 1
    dp, dr, rmse = fm.loss_grad(preds, recons + 1.0, series, starts, age)
    assert not dp.any() and np.isfinite(dp).all() and rmse[0] == 0 and dr.any() and rmse[1] > 0
    assert not np.signbit(dp).any()                                          # +0.0
    sums = fm.batch_sums(preds, recons + 1.0, series, starts, age)
    rows = starts[:, None] + np.arange(W)[None, :]
    assert sums[0] == 0 and sums[2] == 0 and sums[3] == 3 * W * 3 - np.count_nonzero(age[rows])
    # a sum that is not finite: NaN on the observed entries, +0.0 on the others
    bad = recons + 1.0
    bad[1, 2, 0] = np.inf
    age[6, 1] = 3
    _, dr, rmse = fm.loss_grad(preds, bad, series, starts, age)
    seen = age[rows] <= 0
    assert np.isnan(dr[seen]).all() and not dr[~seen].any() and not seen[1, 1, 1] and np.isinf(rmse[1])
    # no group with an observed term: NaN
    assert math.isnan(fm.group_losses(np.array([[0.0, 2.0, 0.0, 4.0]]))[0]) and fm.group_losses(np.array([[0.0, 2.0, 0.0, 4.0]]))[1] == math.sqrt(0.5)
    # a group without observed terms is left out of the mean
    rows = np.array([[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0], [4.0, 4.0, 1.0, 1.0]])
    assert fm.group_losses(rows, 1)[0] == math.sqrt(2.5)


# ---- the entry points refuse bad arguments before anything touches the device ----------------------------------------------------------
def test_symbols_and_bindings(lib):
    import _native
    for name in ("mtadgat_fit_windows", "mtadgat_fit_windows_scratch", "mtadgat_fit_masked_sse", "mtadgat_fit_masked_sse_scratch",
                 "mtadgat_fit_masked_loss_grad", "mtadgat_series_losses_masked", "mtadgat_series_losses_masked_workspace_bytes"):
        assert hasattr(lib, name) and name in _native._HEADER.prototypes, name
    for name, (_, params, _) in _native._HEADER.prototypes.items():
        if name.startswith(("mtadgat_fit_windows", "mtadgat_fit_masked", "mtadgat_series_losses_masked")):
            text = _native._HEADER.prototypes[name][2]
            decls = [d.strip() for d in text[text.index("(") + 1:-1].split(",")]
            assert all(p.endswith("_dev") for (p, _), d in zip(params, decls) if "*" in d and p != "stream"), name


def _windows(lib, age=PTR, ld=6, max_age=0, n_rows=80, F=6, W=8, dims=None, out=3, offs=PTR, parts=3, min_count=24, starts=PTR, count=PTR,
             scratch=PTR, nbytes=None):
    nbytes = lib.mtadgat_fit_windows_scratch(max(n_rows, 1)) if nbytes is None else nbytes
    return lib.mtadgat_fit_windows(age, ld, max_age, n_rows, F, W, dims, out, offs, parts, min_count, starts, count, scratch, nbytes, None)


WINDOWS_BAD = {"null starts": dict(starts=None), "null count": dict(count=None), "null scratch": dict(scratch=None), "W < 1": dict(W=0),
               "W > 512": dict(W=513, n_rows=10000), "F < 1": dict(F=0), "F > 2048": dict(F=2049, ld=2049), "ld_age < F": dict(ld=5),
               "n_rows < W": dict(n_rows=7), "n_rows > 2^31 - 1": dict(n_rows=2 ** 31, nbytes=1 << 40), "out_dim < 1": dict(out=0),
               "out_dim > F without dims": dict(out=7), "parts < 1": dict(parts=0), "min_count < 0": dict(min_count=-1)}


@pytest.mark.parametrize("case", list(WINDOWS_BAD))
def test_fit_windows_rejects_invalid_arguments(lib, case):
    assert _windows(lib, **WINDOWS_BAD[case]) == -1
    assert "fit_windows" in _err(lib)


def test_fit_windows_scratch(lib):
    assert lib.mtadgat_fit_windows_scratch(0) == 0 and lib.mtadgat_fit_windows_scratch(2 ** 31) == 0
    need = lib.mtadgat_fit_windows_scratch(5000)
    assert need % 8 == 0 and 12 * 5000 <= need <= 12 * 5000 + 1024
    assert _windows(lib, n_rows=5000, nbytes=need - 8) == -5 and "scratch" in _err(lib)
    assert _windows(lib, n_rows=5000, scratch=PTR + 4) == -5 and "aligned" in _err(lib)


def _masked_sse(lib, preds=PTR, recons=PTR, batch=7, W=10, out=3, series=PTR, n_rows=100, F=5, ld=5, starts=PTR, start0=0, stride=1, dims=None,
                age=PTR, ld_age=5, max_age=0, accumulate=0, window=PTR, dim=PTR, scratch=PTR, nbytes=None):
    nbytes = lib.mtadgat_fit_masked_sse_scratch(7, 3) if nbytes is None else nbytes
    return lib.mtadgat_fit_masked_sse(preds, recons, batch, W, out, series, n_rows, F, ld, starts, start0, stride, dims, age, ld_age, max_age,
                                      accumulate, window, dim, scratch, nbytes, None)


SSE_BAD = {"null age": dict(age=None), "ld_age < F": dict(ld_age=4), "null preds": dict(preds=None), "null window": dict(window=None),
           "batch 0": dict(batch=0), "out_dim > 2048": dict(out=2049, dims=PTR), "W > 512": dict(W=513, n_rows=10000),
           "ld_series < F": dict(ld=4), "out_dim > F without dims": dict(out=6), "series shorter than W + 1": dict(n_rows=10),
           "accumulate 2": dict(accumulate=2), "progression beyond the series": dict(starts=None, start0=90)}


@pytest.mark.parametrize("case", list(SSE_BAD))
def test_masked_sse_rejects_invalid_arguments(lib, case):
    assert _masked_sse(lib, **SSE_BAD[case]) == -1
    assert "fit_masked_sse" in _err(lib)


def test_masked_sse_scratch(lib):
    assert lib.mtadgat_fit_masked_sse_scratch(0, 3) == 0 and lib.mtadgat_fit_masked_sse_scratch(7, 2049) == 0
    for batch, out in ((7, 3), (1000, 300)):
        assert lib.mtadgat_fit_masked_sse_scratch(batch, out) >= 2 * lib.mtadgat_eval_window_sse_scratch(batch, out) - 64
    assert _masked_sse(lib, nbytes=lib.mtadgat_fit_masked_sse_scratch(7, 3) - 8) == -5
    assert _masked_sse(lib, scratch=PTR + 8) == -5


def _masked_grad(lib, preds=PTR, recons=PTR, batch=7, W=10, out=3, series=PTR, n_rows=100, F=5, ld=5, starts=PTR, dims=None, age=PTR, ld_age=5,
                 max_age=0, sums=PTR, d_preds=PTR, d_recons=PTR, rmse=PTR):
    return lib.mtadgat_fit_masked_loss_grad(preds, recons, batch, W, out, series, n_rows, F, ld, starts, dims, age, ld_age, max_age, sums, d_preds,
                                            d_recons, rmse, None)


GRAD_BAD = {"null age": dict(age=None), "ld_age < F": dict(ld_age=4), "null sums": dict(sums=None), "null starts": dict(starts=None),
            "null rmse": dict(rmse=None), "batch 0": dict(batch=0), "out_dim < 1": dict(out=0), "W < 1": dict(W=0),
            "out_dim > F without dims": dict(out=6), "series shorter than W + 1": dict(n_rows=10)}


@pytest.mark.parametrize("case", list(GRAD_BAD))
def test_masked_loss_grad_rejects_invalid_arguments(lib, case):
    assert _masked_grad(lib, **GRAD_BAD[case]) == -1
    assert "fit_masked_loss_grad" in _err(lib)


def test_masked_series_losses_needs_a_handle_and_an_age(lib):
    assert lib.mtadgat_series_losses_masked_workspace_bytes(None, 5) == 0
    assert lib.mtadgat_series_losses_masked(None, PTR, 100, None, 0, 1, 5, None, PTR, 6, 0, PTR, None, PTR, 1 << 20, None) != 0
    assert lib.mtadgat_series_losses_masked(None, PTR, 100, None, 0, 1, 5, None, None, 6, 0, PTR, None, PTR, 1 << 20, None) != 0


# ---- the Python layer's host checks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_observed", [-0.1, 1.5, float("nan")])
def test_min_observed_outside_the_unit_interval_raises(min_observed):
    import fitting
    with pytest.raises(ValueError, match="min_observed"):
        fitting.training_windows(80, 8, 6, min_observed=min_observed, device="cpu")


def test_min_count_is_a_ceiling():
    import fitting
    assert [fitting._min_count(m, 8, 6) for m in (0.0, 0.5, 0.8, 1.0, 1 / 48, 1 / 48 + 1e-9)] == [0, 24, 39, 48, 1, 2]


def test_a_cpu_age_is_refused():
    import fitting
    from mtad_gat import MTAD_GAT
    with pytest.raises(RuntimeError, match="GPU"):
        fitting.training_windows(80, 8, 6, age=torch.zeros((80, 6), dtype=torch.int32))
    torch.manual_seed(0)
    model = MTAD_GAT(n_features=6, window_size=8, out_dim=6)
    values = torch.rand(40, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        model.series_losses(values, age=torch.zeros((40, 6), dtype=torch.int32))
    assert model.series_losses(values).window_count is None
