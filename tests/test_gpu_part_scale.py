"""Per-part quantiles and score scaling on the device (the k_partq_* kernels and the segmented instantiations of the column
select in csrc/mtadgat_evalcol.hip, k_part_scale in csrc/mtadgat_parts.hip, through evaluation.part_quantiles,
scale_scores(parts=), MTAD_GAT.anomaly_scores(scale_scores="per_part") and predict_anomalies) against tests/part_scale_refs.py.

Gates (those of tests/test_gpu_score_pipeline.py)
  quantiles: |ours - ref| <= 1 float32 ulp of the float64 reference, same NaN pattern, infinities equal; the order statistics
             themselves are exact, bit for bit np.sort's.
  scaling:   the bits of the float32 numpy replay on the device's own quantiles.
  ewm:       |ours - ref64| <= 2^-23 |ref64| + 1e-30.
L = mtadgat_eval_partq_long() separates the select inside one workgroup (len <= L) from the passes with bins in memory."""
import ctypes

import numpy as np
import pytest
import torch

import part_scale_refs
import score_refs

pytestmark = pytest.mark.gpu

QS = [0.0, 0.25, 0.5, 0.75, 1.0]
W = 7


@pytest.fixture(scope="module")
def L():
    import evaluation as ev
    return ev._lib().mtadgat_eval_partq_long()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same_bits(got, want, what):
    """float32 arrays equal bit for bit; where both are NaN (inf - inf, inf / inf in a part whose quartile is an infinity) the payload,
    which numpy's host and the device choose differently, is not compared"""
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), what


def _assert_quantiles(got, ref, what):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    same_inf = np.isinf(ref) & (got == ref)
    fin = ~nan & ~same_inf
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= score_refs.ulp32(ref[fin])), (what, float(err.max()))


def _on_device(a, layout, device):
    n, d = a.shape
    if layout == "contiguous":
        return torch.from_numpy(a).to(device)
    wide = torch.full((n, d + 5), -7.0, device=device)          # the neighbours would change every quantile if they were read
    wide[:, 2:2 + d] = torch.from_numpy(a).to(device)
    t = wide[:, 2:2 + d]
    assert t.stride(0) == d + 5
    return t


def _integer_positions(m):
    """ranks k of a part of m rows whose probability k / (m - 1) lands on k exactly in float64 (test_order_statistics_are_exact)"""
    ks = [k for k in range(m) if np.floor(np.float64(k / (m - 1)) * np.float64(m - 1)) == k and np.float64(k / (m - 1)) * np.float64(m - 1) == k]
    return sorted(set(ks[::max(len(ks) // 5, 1)][:5] + ks[-2:]))        # at most seven: a call takes eight probabilities


_DATA = {}


def _case(name, d, L):
    """(a, lengths, float64 reference for QS) of a layout, computed once"""
    key = (name, d)
    if key not in _DATA:
        spans = part_scale_refs.layouts(L)[name]
        lengths = part_scale_refs.lengths_of(spans, W)
        a = score_refs.columns(sum(spans), d, np.random.default_rng(1000 * len(name) + d), rot=d % 5)
        _DATA[key] = (a, lengths, part_scale_refs.quantiles(a, lengths, W, QS))
    return _DATA[key]


@pytest.mark.parametrize("layout", ["contiguous", "sliced"])
@pytest.mark.parametrize("d", [1, 3, 38, 65])
def test_part_quantiles(d, layout, L, gpu_device):
    import evaluation as ev
    for name in part_scale_refs.layouts(L):
        a, lengths, ref = _case(name, d, L)
        sp = ev.score_parts(lengths, W, device=gpu_device)
        got = ev.part_quantiles(_on_device(a, layout, gpu_device), QS, sp)
        _assert_quantiles(got, ref, (name, d, layout))
        again = ev.part_quantiles(_on_device(a, layout, gpu_device), QS, sp)
        assert torch.equal(_bits(got), _bits(again)), (name, d, layout, "two calls differ")
        for p, (s, e) in enumerate(zip(sp.start_host, sp.end_host)):       # minimum and maximum, bit for bit
            if e == s or (len(lengths) > 100 and p % 97):
                continue
            srt = np.sort(a[s:e], axis=0)
            keep = ~np.isinf(srt).any(axis=0)
            assert torch.equal(got[0, p].cpu()[keep], torch.from_numpy(srt[0])[keep]), (name, p, "minimum")
            assert torch.equal(got[-1, p].cpu()[keep], torch.from_numpy(srt[-1])[keep]), (name, p, "maximum")


def test_a_one_dimensional_array_is_one_column(L, gpu_device):
    import evaluation as ev
    a, lengths, ref = _case("short_long_short", 1, L)
    sp = ev.score_parts(lengths, W, device=gpu_device)
    got = ev.part_quantiles(torch.from_numpy(a[:, 0]).to(gpu_device), QS, sp)
    assert got.shape == (len(QS), len(lengths), 1)
    _assert_quantiles(got, ref, "1-D")


@pytest.mark.parametrize("name", ["edges", "at_L", "short_long_short", "unaligned_long"])
def test_order_statistics_are_exact(name, L, gpu_device):
    """Probabilities whose position q (len - 1) is an integer in float64 return that element of np.sort of the part bit for bit."""
    import evaluation as ev
    a, lengths, _ = _case(name, 3, L)
    sp = ev.score_parts(lengths, W, device=gpu_device)
    t = torch.from_numpy(a).to(gpu_device)
    for p, (s, e) in enumerate(zip(sp.start_host, sp.end_host)):
        m = int(e - s)
        if m < 2:
            continue
        ks = _integer_positions(m)
        assert len(ks) >= 2
        got = ev.part_quantiles(t, [k / (m - 1) for k in ks], sp)[:, p].cpu()
        srt = torch.from_numpy(np.sort(a[s:e], axis=0))
        for c in range(a.shape[1]):
            if np.isinf(a[s:e, c]).any():
                continue                                     # inf - inf in the interpolation, covered by test_part_quantiles
            assert torch.equal(got[:, c], srt[ks, c]), (name, p, c)


@pytest.mark.parametrize("which", ["short", "long"])
def test_one_part_over_everything_is_column_quantiles(which, L, gpu_device):
    import evaluation as ev
    a, lengths, _ = _case(which, 9, L)
    assert sum(lengths) - W == (257 if which == "short" else L + 1)
    t = torch.from_numpy(a).to(gpu_device)
    qs = QS + [0.3333, 0.9]
    whole = ev.column_quantiles(t, qs)
    got = ev.part_quantiles(t, qs, ev.score_parts(lengths, W, device=gpu_device))
    assert torch.isnan(got[:, 0]).all()                      # the window's own part owns no score
    assert torch.equal(_bits(got[:, 1]), _bits(whole))
    alone = ev.part_quantiles(t, qs, ev.score_parts([a.shape[0] + W], W, device=gpu_device))
    assert torch.equal(_bits(alone[:, 0]), _bits(whole))


def test_the_routes_agree(L, gpu_device):
    """The same rows as one part of L + 1 (bins in memory) and cut into L + 1 (bins in LDS): each side's order statistics are np.sort's."""
    import evaluation as ev
    a, lengths, _ = _case("long", 3, L)
    t = torch.from_numpy(a).to(gpu_device)
    for spans in ([L + 1], [L, 1]):
        sp = ev.score_parts(part_scale_refs.lengths_of(spans, W), W, device=gpu_device)
        at = 0
        for p, m in enumerate(spans, start=1):
            ks = [0, m - 1] + (_integer_positions(m) if m > 1 else [])
            qs = [k / (m - 1) if m > 1 else 0.5 for k in ks][:8]
            got = ev.part_quantiles(t, qs, sp)[:, p].cpu()
            srt = torch.from_numpy(np.sort(a[at:at + m], axis=0))
            for c in range(a.shape[1]):
                if not np.isinf(a[at:at + m, c]).any():
                    assert torch.equal(got[:, c], srt[ks[:8], c]), (spans, p, c)
            at += m


def test_a_nan_poisons_its_part_and_column_only(L, gpu_device):
    import evaluation as ev
    a, lengths, _ = _case("short_long_short", 3, L)
    sp = ev.score_parts(lengths, W, device=gpu_device)
    for part in (1, 2):                                      # a short part and the long one
        for value in (np.nan, -np.nan):                      # sign bit set: sorts below -inf as a key
            b = a.copy()
            b[sp.start_host[part] + (sp.end_host[part] - sp.start_host[part]) // 3, 1] = value
            got = ev.part_quantiles(torch.from_numpy(b).to(gpu_device), QS, sp)
            assert torch.isnan(got[:, part, 1]).all()
            _assert_quantiles(got, part_scale_refs.quantiles(b, lengths, W, QS), ("NaN", part))


@pytest.mark.parametrize("name", ["short_long_short", "empty", "many"])
def test_scale_scores_bits(name, L, gpu_device):
    import evaluation as ev
    a, lengths, _ = _case(name, 3, L)
    a = np.ascontiguousarray(a[:, [0, 1, 2]])
    sp = ev.score_parts(lengths, W, device=gpu_device)
    t = torch.from_numpy(a).to(gpu_device)
    q3 = ev.part_quantiles(t, [0.25, 0.5, 0.75], sp)
    got = ev.scale_scores(t, parts=sp)
    want = part_scale_refs.scale(a, q3.cpu().numpy(), lengths, W)
    assert got.dtype == torch.float32 and got.shape == t.shape
    _assert_same_bits(got, want, name)
    if name == "short_long_short":
        assert not np.isnan(want).any()
    one = ev.scale_scores(t[:, 0], parts=sp)
    assert one.shape == (a.shape[0],) and torch.equal(_bits(one), _bits(got[:, 0]))
    # in place, through the C entry
    lib = ev._lib()
    start, end, _ = sp.tensors(gpu_device)
    work = t.clone()
    torch.cuda.synchronize()
    rc = lib.mtadgat_eval_part_scale(work.data_ptr(), a.shape[0], 3, 3, start.data_ptr(), end.data_ptr(), sp.n_parts, q3.data_ptr(),
                                     work.data_ptr(), 3, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert torch.equal(_bits(work), _bits(got))


def test_scale_gives_nan_outside_every_span(gpu_device):
    import evaluation as ev
    lib = ev._lib()
    rng = np.random.default_rng(31)
    a = (rng.random((50, 2)) * 3.0).astype(np.float32)
    t = torch.from_numpy(a).to(gpu_device)
    start = torch.tensor([3, 20, 30], dtype=torch.int64, device=gpu_device)      # rows 0-2, 15-19 and 45-49 belong to no span
    end = torch.tensor([15, 20, 45], dtype=torch.int64, device=gpu_device)
    q3 = torch.from_numpy(rng.random((3, 3, 2)).astype(np.float32)).to(gpu_device)
    out = torch.empty_like(t)
    torch.cuda.synchronize()
    rc = lib.mtadgat_eval_part_scale(t.data_ptr(), 50, 2, 2, start.data_ptr(), end.data_ptr(), 3, q3.data_ptr(), out.data_ptr(), 2,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = out.cpu().numpy()
    q = q3.cpu().numpy()
    inside = np.zeros(50, bool)
    for p, (s, e) in enumerate(((3, 15), (20, 20), (30, 45))):
        inside[s:e] = True
        want = (a[s:e] - q[1, p]) / (np.float32(1) + (q[2, p] - q[0, p]))
        assert np.array_equal(got[s:e].view(np.int32), want.view(np.int32)), p
    assert np.isnan(got[~inside]).all() and not np.isnan(got[inside]).any()


# ---- the model and the one-call pipeline -----------------------------------------------------------------------------------------
E2E_W = 10
E2E_LENGTHS = dict(train=[150, 120, 0, 140, 90], test=[170, 160, 130, 0, 75])


def _series(lengths, g):
    """Parts of unequal length; the second one's values, and so its errors, are 30 times the others'."""
    parts = [torch.rand(m, 5, generator=g) * (30.0 if p == 1 else 1.0) for p, m in enumerate(lengths)]
    return torch.cat(parts)


@pytest.fixture(scope="module")
def setup(gpu_device):
    from mtad_gat import MTAD_GAT
    torch.manual_seed(9)
    model = MTAD_GAT(n_features=5, window_size=E2E_W, out_dim=5, kernel_size=3, gru_hid_dim=24, forecast_hid_dim=24,
                     recon_hid_dim=24).to(gpu_device).eval()
    g = torch.Generator().manual_seed(10)
    train, test = _series(E2E_LENGTHS["train"], g), _series(E2E_LENGTHS["test"], g)
    labels = torch.zeros(test.shape[0] - E2E_W, dtype=torch.bool)
    labels[60:85] = True
    test[E2E_W + 60:E2E_W + 85] += 1.5
    return model, train.to(gpu_device), test.to(gpu_device), labels.to(gpu_device)


@pytest.mark.parametrize("use_mov_av", [False, True])
def test_anomaly_scores_scaled_per_part(setup, use_mov_av, gpu_device):
    import evaluation as ev
    model, _, test, _ = setup
    lengths = E2E_LENGTHS["test"]
    sp = ev.score_parts(lengths, E2E_W, (3, E2E_W - 1), device=gpu_device)
    kw = dict(gamma=0.8, use_mov_av=use_mov_av, smoothing_span=5)
    with torch.no_grad():
        raw = model.anomaly_scores(test, gamma=0.8)[1]
        got, got_pd = model.anomaly_scores(test, scale_scores="per_part", parts=sp, **kw)
        # rebuilt from the package's own pieces, the scaling from the reference on the host
        x = raw.cpu().numpy()
        q3 = part_scale_refs.quantiles(x, lengths, E2E_W, [0.25, 0.5, 0.75])
        ref_pd = part_scale_refs.scale(x, q3.astype(np.float32), lengths, E2E_W)
        pd = got_pd.cpu().numpy().astype(np.float64)
        err = np.abs(pd - ref_pd.astype(np.float64))
        print("per-dimension: max error in float32 ulps", float((err / score_refs.ulp32(ref_pd)).max()))
        assert np.all(err <= score_refs.ulp32(ref_pd)), float((err / score_refs.ulp32(ref_pd)).max())
        scores = torch.from_numpy(ref_pd).to(gpu_device).mean(dim=1)
        if use_mov_av:
            scores = ev.moving_average(scores, 5, parts=sp)
        want = ev.adjust_part_scores(scores, sp).cpu().numpy().astype(np.float64)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        bound = 2.0 ** -23 * np.abs(want) + 1e-30
        print("global: max error / bound", float((err / bound).max()))
        assert np.all(err <= bound), float((err / bound).max())
        # and bit for bit the package's own scaling pass
        assert torch.equal(_bits(got_pd), _bits(ev.scale_scores(raw, parts=sp)))
        # scale_scores=True keeps its meaning with parts: the whole series' quantiles
        glob, glob_pd = model.anomaly_scores(test, scale_scores=True, parts=sp, **kw)
        q = ev.column_quantiles(raw, [0.25, 0.5, 0.75])
        assert torch.equal(_bits(glob_pd), _bits((raw - q[1]) / (1.0 + (q[2] - q[0]))))
        assert torch.equal(_bits(glob_pd), _bits(model.anomaly_scores(test, gamma=0.8, scale_scores=True)[1]))
        assert not torch.equal(glob_pd, got_pd) and not torch.equal(glob, got)


@pytest.mark.parametrize("mode", ["global", "per_part"])
def test_predict_anomalies_scaled_per_part(setup, mode, gpu_device):
    import evaluation as ev
    model, train, test, labels = setup
    transition = (3, E2E_W - 1)
    opts = dict(train_lengths=E2E_LENGTHS["train"], test_lengths=E2E_LENGTHS["test"], transition=transition, thresholds=mode)
    tr_parts = ev.score_parts(E2E_LENGTHS["train"], E2E_W, transition, device=gpu_device)
    te_parts = ev.score_parts(E2E_LENGTHS["test"], E2E_W, transition, device=gpu_device)
    with torch.no_grad():
        out = ev.predict_anomalies(model, train, test, labels=labels, gamma=0.8, scale_scores="per_part", parts=opts)
        tr_s, tr_pd = model.anomaly_scores(train, gamma=0.8, scale_scores="per_part", parts=tr_parts)
        te_s, te_pd = model.anomaly_scores(test, gamma=0.8, scale_scores="per_part", parts=te_parts)
    assert torch.equal(_bits(out["test_per_dim"]), _bits(te_pd))
    assert torch.equal(_bits(out["train_scores"]), _bits(tr_s)) and torch.equal(_bits(out["test_scores"]), _bits(te_s))
    thr, preds = ev.feature_predictions(tr_pd, te_pd, 1)
    assert np.allclose(out["feature_thresholds"], thr, rtol=1e-9, atol=0) and torch.equal(out["feature_preds"], preds)
    assert ("part_result" in out) == (mode == "per_part")
    if mode == "per_part":
        assert out["part_result"]["thresholds"].shape == (len(E2E_LENGTHS["test"]),)


def test_value_errors(setup, gpu_device):
    import evaluation as ev
    model, train, test, _ = setup
    sp = ev.score_parts(E2E_LENGTHS["test"], E2E_W, device=gpu_device)
    with pytest.raises(ValueError):
        model.anomaly_scores(test, scale_scores="per_part")
    with pytest.raises(ValueError):
        model.anomaly_scores(test, scale_scores="per-part", parts=sp)
    with pytest.raises(ValueError):
        model.anomaly_scores(test, scale_scores="yes")
    with pytest.raises(ValueError):
        ev.predict_anomalies(model, train, test, scale_scores="per_part")
    with pytest.raises(ValueError):
        ev.predict_anomalies(model, train, test, scale_scores="global", parts=dict(test_lengths=E2E_LENGTHS["test"]))
    with pytest.raises(ValueError, match="per-part"):
        model.score_attribution(test, [3], scale_scores="per_part")
    with pytest.raises(ValueError):
        ev.part_quantiles(test[:, 0], [0.5] * 9, ev.score_parts([test.shape[0] + 3], 3))
    with pytest.raises(ValueError):
        ev.part_quantiles(test[:, 0], [0.5], ev.score_parts([test.shape[0]], 3))      # parts describe another number of scores
