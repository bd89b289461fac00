"""The kernels of csrc/mtadgat_eval.hip (k_eval_moments, k_eval_epsilon, k_eval_segments + k_eval_adjust, k_eval_scores) and the
per-part tables of csrc/mtadgat_parts.hip (k_part_moments, k_part_epsilon) table by table against the float64 specification of
tests/eval_refs.py: every row of the z table, not only the threshold find_epsilon picks from it; at the sizes where a tile of
epsilon_tile (csrc/mtadgat_scan.h: 1024 rows, flags in 64-bit words), a trip of the grid-stride loops or the staged / direct
dilation paths change; contiguous and as a column slice of a wider tensor.  The bounds are derived in eval_refs.check_*; each test
prints the largest error / bound it met (pytest -s).  Scratch buffers have the sizes evaluation.py allocates."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eval_refs as er

pytestmark = pytest.mark.gpu
_dp = ctypes.POINTER(ctypes.c_double)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _scratch(doubles, device):
    import _native
    return _native._empty(doubles, dtype=torch.float64, device=device)


def _note(what, cases, ratio=None):
    print(f"[eval tables] {what}: {cases} cases" + ("" if ratio is None else f", largest error / bound {ratio:.3g}"))


# ---- (a) moments ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _moment_ref(n, d):
    """The columns and per column (sum, sum of squares, sum of |v|)."""
    e = er.moment_columns(n, d)
    return e, [er.moments(e[:, c]) + (er.abs_sum(e[:, c]),) for c in range(d)]


def _check_moments(got, ref, n):
    s, s2, sa = ref
    return max(er.check_sums([got[0]], [s], n, sa), er.check_sums([got[1]], [s2], n, s2))


@pytest.mark.parametrize("n", er.MOMENT_SIZES)
def test_moments(n, gpu_device):
    import evaluation as ev
    lib = ev._lib()
    e, ref = _moment_ref(n, 1)
    x = _dev(e[:, 0], gpu_device)
    scratch = _scratch(2, gpu_device)
    out = (ctypes.c_double * 2)()
    with torch.cuda.device(gpu_device):
        assert lib.mtadgat_eval_moments(x.data_ptr(), n, scratch.data_ptr(), out, ev._stream(x)) == 0
    _note(f"moments n={n}", 1, _check_moments(list(out), ref[0], n))


@pytest.mark.parametrize("d", er.MOMENT_COLUMNS)
@pytest.mark.parametrize("n", er.MOMENT_SIZES)
def test_moments_columns(n, d, gpu_device):
    import evaluation as ev
    lib = ev._lib()
    e, ref = _moment_ref(n, d)
    wide = torch.full((n, d + 3), 1e6, device=gpu_device)           # what a wrong column or row stride would pick up
    wide[:, 1:1 + d] = _dev(e, gpu_device)
    worst = 0.0
    for x in (_dev(e, gpu_device), wide[:, 1:1 + d]):
        ld = x.stride(0)
        scratch = _scratch(max(2 * d, 5 * d * 19), gpu_device)
        out = (ctypes.c_double * (2 * d))()
        with torch.cuda.device(gpu_device):
            assert lib.mtadgat_eval_moments_columns(x.data_ptr(), n, d, ld, scratch.data_ptr(), out, ev._stream(x)) == 0
        for c in range(d):
            try:
                worst = max(worst, _check_moments(out[2 * c:2 * c + 2], ref[c], n))
            except AssertionError as err:
                raise AssertionError(f"column {c} of {d}, ld {ld}: {err}") from None
    _note(f"moments_columns n={n} d={d}", 2 * d, worst)


# ---- (b) the epsilon table -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _eps_ref(n, halo, seed=0, nonfinite=False):
    e, eps = er.epsilon_case(n, halo, seed, nonfinite)
    tab, absum = er.epsilon_table(e, eps, halo, with_abs=True)
    return e, eps, tab, absum


def _check_table(got, tab, absum, n, finite=True):
    """Counts exact, both sums inside the bound of eval_refs.check_sums with n = the row's pruned count."""
    got = np.asarray(got, np.float64).reshape(-1, 4)
    er.check_counts(got[:, 2:], tab[:, 2:])
    assert got[er.EPS_ROW_NAN].tolist() == [0.0, 0.0, 0.0, 0.0]                     # a NaN threshold: the zero row
    assert got[er.EPS_ROW_BELOW].tolist() == [0.0, 0.0, 0.0, float(n)]             # below every sample: nothing pruned, all dilated
    if finite:
        assert got[er.EPS_ROW_ABOVE, 2:].tolist() == [float(n), 0.0]               # above every sample: all pruned, none hot
    return max(er.check_sums(got[:, 0], tab[:, 0], tab[:, 2], absum), er.check_sums(got[:, 1], tab[:, 1], tab[:, 2], tab[:, 1]))


def _epsilon_table(ev, x, n, eps, halo):
    lib = ev._lib()
    scratch = _scratch(64 + 4 * 64, x.device)
    out = (ctypes.c_double * (4 * eps.size))()
    with torch.cuda.device(x.device):
        rc = lib.mtadgat_eval_epsilon_table(x.data_ptr(), n, eps.ctypes.data_as(_dp), eps.size, halo, scratch.data_ptr(), out, ev._stream(x))
    assert rc == 0
    return out


@pytest.mark.parametrize("n,halo", [(n, h) for h in er.EPS_HALOS for n in er.eps_sizes(h)] + [er.EPS_THREE_TRIPS])
def test_epsilon_table(n, halo, gpu_device):
    import evaluation as ev
    e, eps, tab, absum = _eps_ref(n, halo)
    assert eps.size == er.EPS_NZ
    got = _epsilon_table(ev, _dev(e, gpu_device), n, eps, halo)
    _note(f"epsilon_table n={n} halo={halo}", 1, _check_table(got, tab, absum, n))


def test_epsilon_table_nan_and_inf_samples(gpu_device):
    """NaN and +inf samples under finite thresholds: both stay out of the pruned sums, +inf is hot, NaN is not."""
    import evaluation as ev
    n, halo = 4099, 49
    e, eps, tab, absum = _eps_ref(n, halo, 0, True)
    assert np.isnan(e).sum() == 6 and np.isinf(e).sum() == 6
    assert tab[er.EPS_ROW_ABOVE, 2] == n - 12 and 6 <= tab[er.EPS_ROW_ABOVE, 3] <= 6 * (2 * halo + 1)      # the +inf samples alone are hot
    assert np.isfinite(tab).all()
    got = _epsilon_table(ev, _dev(e, gpu_device), n, eps, halo)
    _note("epsilon_table with NaN and +inf samples", 1, _check_table(got, tab, absum, n, finite=False))


@pytest.mark.parametrize("n,halo", [(257, 49), (32769, 49), (65793, 49), (257, 129), (32769, 129), (1025, 49), (131073, 49), (1025, 129)])
def test_epsilon_table_columns(n, halo, gpu_device):
    """Three columns of a six-column tensor, each with its own data and thresholds; at n = 131073 the grid cap
    min(ceil(n / 1024), 128) holds and the first block makes a second trip (three trips: test_epsilon_table at EPS_THREE_TRIPS)."""
    import evaluation as ev
    lib = ev._lib()
    d, ld, nz = 3, 6, er.EPS_NZ
    refs = [_eps_ref(n, halo, 1 + c) for c in range(d)]
    wide = np.full((n, ld), 2.5, np.float32)                         # hot under most thresholds: a wrong column shows
    for c in range(d):
        wide[:, 2 + c] = refs[c][0]
    x = _dev(wide, gpu_device)[:, 2:2 + d]
    assert x.stride(0) == ld and x.data_ptr() % 16 == 8
    eps = np.ascontiguousarray(np.stack([r[1] for r in refs]))
    scratch = _scratch(max(2 * d, 5 * d * nz), gpu_device)
    out = (ctypes.c_double * (4 * nz * d))()
    with torch.cuda.device(gpu_device):
        rc = lib.mtadgat_eval_epsilon_table_columns(x.data_ptr(), n, d, ld, eps.ctypes.data_as(_dp), nz, halo, scratch.data_ptr(), out,
                                                    ev._stream(x))
    assert rc == 0
    worst = 0.0
    for c in range(d):
        try:
            worst = max(worst, _check_table(out[4 * nz * c:4 * nz * (c + 1)], refs[c][2], refs[c][3], n))
        except AssertionError as err:
            raise AssertionError(f"column {c}: {err}") from None
    _note(f"epsilon_table_columns n={n} halo={halo}", d, worst)


def _check_part_rows(mom, tab, x, start, end, eps, halo):
    """Every part's moments and table rows against the reference of its slice alone; the largest error / bound."""
    worst = 0.0
    for p, (s, e) in enumerate(zip(start, end)):
        part, n = x[s:e], int(e - s)
        try:
            if n == 0:
                assert mom[p].tolist() == [0.0, 0.0, -np.inf] and not tab[p].any()
                continue
            ref, absum = er.epsilon_table(part, eps[p], halo, with_abs=True)
            worst = max(worst, _check_table(tab[p], ref, absum, n), _check_moments(mom[p, :2], er.moments(part) + (er.abs_sum(part),), n))
            assert mom[p, 2] == float(part.max())
        except AssertionError as err:
            raise AssertionError(f"part {p} of {n} scores: {err}") from None
    return worst


@pytest.mark.parametrize("halo", er.PART_TABLE_HALOS)
def test_part_epsilon_table(halo, gpu_device):
    """mtadgat_eval_part_epsilon_moments / _table called directly: parts on both sides of a tile and an empty one, each under its own
    64 thresholds.  The dilation never looks outside a part, so the part's slice alone is the reference; counts exact, sums inside
    the bound of eval_refs.check_sums with n = the row's pruned count."""
    import evaluation as ev
    lib = ev._lib()
    x, start, end, eps = er.part_table_case(halo)
    P, nz, n = len(start), er.EPS_NZ, x.size
    xd, sd, ed = _dev(x, gpu_device), _dev(start, gpu_device), _dev(end, gpu_device)
    scratch = ev._scratch(lib.mtadgat_eval_part_epsilon_scratch(n, P, nz), gpu_device)
    mom, tab = np.empty((P, 3)), np.empty((P, 4 * nz))
    eps = np.ascontiguousarray(eps)
    with torch.cuda.device(gpu_device):
        rc = lib.mtadgat_eval_part_epsilon_moments(xd.data_ptr(), n, sd.data_ptr(), ed.data_ptr(), P, nz, scratch.data_ptr(),
                                                   scratch.numel() * 8, mom.ctypes.data_as(_dp), ev._stream(xd))
        assert rc == 0, lib.mtadgat_last_error()
        rc = lib.mtadgat_eval_part_epsilon_table(xd.data_ptr(), n, sd.data_ptr(), ed.data_ptr(), P, eps.ctypes.data_as(_dp), nz, halo,
                                                 scratch.data_ptr(), scratch.numel() * 8, tab.ctypes.data_as(_dp), ev._stream(xd))
        assert rc == 0, lib.mtadgat_last_error()
    _note(f"part_epsilon_table halo={halo}", P, _check_part_rows(mom, tab, x, start, end, eps, halo))


# ---- (c) point adjust ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", er.ADJUST_SIZES)
def test_point_adjust_table(n, gpu_device):
    import evaluation as ev
    cases = 0
    for kind in er.ADJUST_LABELS:
        s, lab, thr = er.adjust_case(n, kind)
        assert thr.size == 64
        sd, labd = _dev(s, gpu_device), _dev(lab, gpu_device).bool()
        for f32 in (False, True):
            got = ev.point_adjust_counts(sd, labd, thr, compare_f32=f32)
            try:
                er.check_counts(got, er.point_adjust_table(s, lab, thr, f32))
            except AssertionError as err:
                raise AssertionError(f"labels {kind}, compare_f32 {f32}: {err}") from None
            cases += 1
    _note(f"point_adjust n={n}", cases)


def test_point_adjust_segment_limit(gpu_device):
    """2049 segments: room for exactly that many passes, one fewer is status -5, and the next call with room is right again."""
    import evaluation as ev
    s, lab, thr = er.adjust_case(4099, "alternating")
    nseg = int(lab.sum())
    assert nseg == 2049
    want = er.point_adjust_table(s, lab, thr)
    sd, labd = _dev(s, gpu_device), _dev(lab, gpu_device).bool()
    er.check_counts(ev.point_adjust_counts(sd, labd, thr, max_segments=nseg), want)
    with pytest.raises(RuntimeError, match="status -5"):
        ev.point_adjust_counts(sd, labd, thr, max_segments=nseg - 1)
    er.check_counts(ev.point_adjust_counts(sd, labd, thr, max_segments=nseg), want)
    er.check_counts(ev.point_adjust_counts(sd, labd, thr), want)


# ---- (d) scores ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", er.SCORE_DIMS)
@pytest.mark.parametrize("n", er.SCORE_SIZES)
def test_scores(n, d, gpu_device):
    import _native
    import evaluation as ev
    lib = ev._lib()
    p, r, a = er.score_case(n, d)
    pd, rd = _dev(p, gpu_device), _dev(r, gpu_device)
    worst_dim = worst_glob = 0.0
    cases = 0
    for dims in (None, er.score_dims(d)):
        actual = _dev(a[:, :d] if dims is None else a, gpu_device)
        dims_dev = None if dims is None else torch.tensor(dims, dtype=torch.int32, device=gpu_device)
        for gamma in er.SCORE_GAMMAS:
            want_dim, want_glob = er.scores(p, r, a, dims, gamma)
            for outputs in ("both", "per_dim", "global"):
                per_dim = _native._empty((n, d), dtype=torch.float32, device=gpu_device) if outputs != "global" else None
                glob = _native._empty((n,), dtype=torch.float32, device=gpu_device) if outputs != "per_dim" else None
                with torch.cuda.device(gpu_device):
                    rc = lib.mtadgat_eval_scores(pd.data_ptr(), rd.data_ptr(), actual.data_ptr(), n, d, actual.shape[1],
                                                 None if dims_dev is None else dims_dev.data_ptr(), gamma,
                                                 None if per_dim is None else per_dim.data_ptr(), None if glob is None else glob.data_ptr(),
                                                 ev._stream(pd))
                assert rc == 0
                try:
                    if per_dim is not None:
                        worst_dim = max(worst_dim, er.check_scores(per_dim.cpu().numpy(), want_dim))
                    if glob is not None:
                        worst_glob = max(worst_glob, er.check_scores(glob.cpu().numpy(), want_glob, d=d))
                except AssertionError as err:
                    raise AssertionError(f"dims {'none' if dims is None else 'listed'}, gamma {gamma}, outputs {outputs}: {err}") from None
                cases += 1
    _note(f"scores per dimension n={n} d={d}", cases, worst_dim)
    _note(f"scores mean n={n} d={d}", cases, worst_glob)
