"""Reference arithmetic of the threshold-evaluation kernels of csrc/mtadgat_eval.hip (k_eval_moments, k_eval_epsilon,
k_eval_segments + k_eval_adjust, k_eval_scores) and of the per-part tables of csrc/mtadgat_parts.hip (k_part_moments,
k_part_epsilon) in numpy / float64, table by table, straight from the definitions; the gates the GPU tests hold the kernels to; and
the seeded inputs those tests and tests/test_host_eval.py share.  No torch, no GPU.
Both epsilon kernels run epsilon_tile (csrc/mtadgat_scan.h): tiles of 1024 rows, the hot flags staged as 64-bit ballot words.

The gates return the largest error / bound ratio they met, so a caller can report how much room a derived bound leaves."""
import math

import numpy as np

from oracle import eval_oracle as eo

U64 = 2.0 ** -52          # float64 machine epsilon
U32 = 2.0 ** -24          # float32 unit roundoff


# ---- the specification ---------------------------------------------------------------------------------------------------------------
def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).tolist())


def moments(e32):
    """(sum v, sum v^2) of the float32 values widened to float64, correctly rounded (v^2 is exact in float64)."""
    v = np.asarray(e32, dtype=np.float32).astype(np.float64).reshape(-1)
    return _fsum(v), _fsum(v * v)


def abs_sum(e32):
    """sum |v|: what the bound of check_sums scales with."""
    return _fsum(np.abs(np.asarray(e32, dtype=np.float32).astype(np.float64).reshape(-1)))


def hot_flags(e32, eps):
    """v >= eps on the widened values; a NaN sample or a NaN threshold is not hot."""
    v = np.asarray(e32, dtype=np.float32).astype(np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return v >= np.float64(eps)


def dilated_count(hot, halo):
    """|{ i : some |k| <= halo with 0 <= i + k < n has hot[i + k] }| through a prefix sum."""
    hot = np.asarray(hot, dtype=bool)
    n = hot.size
    if halo < 0:
        return 0
    c = np.concatenate(([0], np.cumsum(hot, dtype=np.int64)))
    idx = np.arange(n, dtype=np.int64)
    return int(np.sum(c[np.minimum(idx + halo, n - 1) + 1] - c[np.maximum(idx - halo, 0)] > 0))


def epsilon_table(e32, eps, halo, with_abs=False, hot=hot_flags):
    """(nz, 4) float64: per threshold fsum(v[v < eps]), fsum(v^2[v < eps]), |{v < eps}|, dilated_count(v >= eps, halo).
    Comparisons on the widened values, literally `<` and `>=`: a NaN sample is neither pruned nor hot, a NaN threshold gives a
    zero row.  with_abs: also the (nz,) array of fsum(|v|[v < eps]) for the bound of check_sums.  `hot` is replaceable so that
    tests/test_host_eval.py can state mutations of the definition."""
    v = np.asarray(e32, dtype=np.float32).astype(np.float64).reshape(-1)
    eps = np.asarray(eps, dtype=np.float64).reshape(-1)
    tab = np.zeros((eps.size, 4), np.float64)
    absum = np.zeros(eps.size, np.float64)
    for k, ez in enumerate(eps):
        with np.errstate(invalid="ignore"):
            pruned = v[v < ez]
        tab[k] = (_fsum(pruned), _fsum(pruned * pruned), pruned.size, dilated_count(hot(e32, ez), halo))
        absum[k] = _fsum(np.abs(pruned))
    return (tab, absum) if with_abs else tab


def point_adjust_table(score32, label, thresholds, compare_f32=False):
    """(n_thr, 6) float64: TP, TN, FP, FN, latency sum, detected segments, from oracle.eval_oracle.point_adjust / confusion.  The
    oracle returns the latency as sum / (detected + 1e-4); the sum and the count are carried separately here and held to it."""
    s = np.asarray(score32, dtype=np.float32).reshape(-1)
    lab = np.asarray(label).reshape(-1)
    segs = eo.segments(lab)
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    out = np.zeros((thr.size, 6), np.float64)
    for k, t in enumerate(thr):
        with np.errstate(invalid="ignore", over="ignore"):
            raw = (s > np.float32(t)) if compare_f32 else (s.astype(np.float64) > float(t))
            pred, latency = eo.point_adjust(s, lab, t, compare_f32)
        f = eo.confusion(pred, lab)
        lat, det = 0, 0
        for s0, s1 in segs:
            hit = np.flatnonzero(raw[s0:s1 + 1])
            if hit.size:
                det += 1
                lat += max(int(s0 + hit[0]) - max(int(s0), 1), 0)
        assert abs(lat / (det + 1e-4) - latency) <= 1e-12 * max(1.0, abs(latency)), (t, lat, det, latency)
        out[k] = (f[3], f[4], f[5], f[6], lat, det)
    return out


def scores(preds32, recons32, actual32, dims=None, gamma=1.0):
    """(per_dim (n, d), global (n,)) float64: |p - t| + g |r - t| with t = actual[:, dims[k]] (dims None: column k) and its mean
    over d, evaluated in float64 from the float32 inputs with g = float(np.float32(gamma))."""
    p = np.asarray(preds32, dtype=np.float32).astype(np.float64)
    r = np.asarray(recons32, dtype=np.float32).astype(np.float64)
    a = np.asarray(actual32, dtype=np.float32).astype(np.float64)
    t = a[:, :p.shape[1]] if dims is None else a[:, np.asarray(dims, dtype=np.int64)]
    g = float(np.float32(gamma))
    per_dim = np.abs(p - t) + g * np.abs(r - t)
    return per_dim, per_dim.sum(axis=1) / p.shape[1]


def find_epsilon(e32, reg_level, choose, zs=np.arange(2.5, 12, 0.5), halo=49):
    """find_epsilon rebuilt from the tables above and `choose` = evaluation._choose_epsilon, the way evaluation.find_epsilon does."""
    e32 = np.asarray(e32, dtype=np.float32).reshape(-1)
    n = e32.size
    s, s2 = moments(e32)
    mean = s / n
    sd = math.sqrt(max(s2 / n - mean * mean, 0.0))
    eps = mean + sd * zs
    best = choose(n, mean, sd, eps, epsilon_table(e32, eps, halo).reshape(-1), reg_level)
    return float(e32.max()) if best is None else best


# ---- the gates -----------------------------------------------------------------------------------------------------------------------
def check_sums(got, want, n, abs_sum):
    """|got - want| <= n 2^-52 sum |term| elementwise: any order of float64 additions of n terms stays inside it (the standard
    (n - 1) u / (1 - (n - 1) u) with u = 2^-53, plus the half ulp of the correctly rounded reference); n = 0 asks for 0 exactly.
    Raises AssertionError naming the first offending row; returns the largest error / bound."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    bound = np.broadcast_to(np.asarray(n, np.float64) * U64 * np.asarray(abs_sum, np.float64), want.shape).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    bad = ~(err <= bound)                       # a NaN fails
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"sum row {k}: got {got[k]!r}, want {want[k]!r}, error {err[k]:.3e} > bound {bound[k]:.3e}")
    pos = bound > 0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


def check_counts(got, want):
    """Exact equality of count tables (any shape); raises AssertionError naming the first offending row."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    g2, w2 = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    bad = ~np.all(g2 == w2, axis=1)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"count row {k}: got {g2[k].tolist()}, want {w2[k].tolist()}")


def check_scores(got, want, d=None):
    """d None, per-dimension scores: |got - want| <= 4 2^-24 want -- every path to a = fl(fl|p - t| + fl(g fl|r - t|)) carries at
    most three roundings (its terms are non-negative, so relative errors do not add across the sum), contracted to an fma or not,
    plus one of slack.  d given, the mean over d: <= (d + 4) 2^-24 want -- three from each term, d - 1 sequential float32 additions of
    non-negative terms, one division, one of slack.  Raises AssertionError naming the first offending element; returns the largest
    error / bound."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bound = (4 if d is None else d + 4) * U32 * np.abs(want)
    err = np.abs(got - want)
    bad = ~(err <= bound)
    if bad.any():
        k = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError(f"score {k}: got {got[k]!r}, want {want[k]!r}, error {err[k]:.3e} > bound {bound[k]:.3e}")
    pos = bound > 0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


# ---- the shared, seeded inputs -------------------------------------------------------------------------------------------------------
MOMENT_SIZES = (1, 255, 256, 257, 65535, 65536, 65537, 131073)       # k_eval_moments: 256 x 256 rows per trip of the grid
MOMENT_COLUMNS = (1, 3, 65)
EPS_HALOS = (0, 1, 49, 127, 128, 129, 300)                            # 128 = EPS_HALO_MAX: 129 and 300 read memory directly
EPS_TILE = 1024                                                       # rows of epsilon_tile (SPAN_RB), staged as words of 64 flags
EPS_TRIP = 128 * EPS_TILE                                             # rows of k_eval_epsilon per trip of the grid (at most 128 tiles)
EPS_OLD_TILE, EPS_OLD_TRIP = 256, 128 * 256                           # the byte-flag tile k_eval_epsilon had: its sizes stay in the lists
EPS_THREE_TRIPS = (2 * EPS_TRIP + EPS_TILE + 1, 49)                   # the one (n, halo) at which every block makes three trips
EPS_COLUMN_SIZES = (257, 1025, 32769, 65793, EPS_TRIP + 1)
PART_TABLE_SCORES = (13, 0, 300, 1023, 1024, 1025, 2500)              # scores per part of the per-part table test: around EPS_TILE
PART_TABLE_HALOS = (0, 49, 128)
EPS_NZ = 64
ADJUST_SIZES = (1, 2, 255, 256, 257, 4099)
ADJUST_LABELS = ("none", "all", "alternating", "one_at_0", "longer_at_0", "ending_at_end", "spanning_250_520", "random")
SCORE_SIZES = (1, 255, 256, 257, 1000)
SCORE_DIMS = (1, 3, 38, 65)
SCORE_GAMMAS = (0.0, 1.0, 0.3)
SCORE_ACTUAL_COLUMNS = 70


def eps_sizes(halo):
    """n one below, at and one above a tile and a trip, and a tile / a trip and a partial tile with its halo more; the same around
    the earlier tile of 256 rows, which is four words."""
    ns = (1, 2, halo, halo + 1, 2 * halo + 1)
    for tile, trip in ((EPS_OLD_TILE, EPS_OLD_TRIP), (EPS_TILE, EPS_TRIP)):
        ns += (tile - 1, tile, tile + 1, tile + halo, trip - 1, trip, trip + 1, trip + tile + 1 + halo)
    return sorted({n for n in ns if n >= 1})


def moment_columns(n, d, seed=0):
    """(n, d) float32 of both signs (the sums cancel, the bound of check_sums does not) on an offset."""
    rng = np.random.default_rng([11, n, d, seed])
    return (rng.standard_normal((n, d)) * 3.0 + 0.25).astype(np.float32)


def spike_indices(n, halo):
    """Where epsilon_case puts its isolated spikes, tallest first, twelve at the most: a dilation window then ends exactly on a tile
    edge (1024) or a trip edge (131072) of k_eval_epsilon, or one sample short of / past it.  A tile's flag t is sample
    r0 - halo + t, so the spikes at 1024 - halo and 1024 - halo - 1 are bit 0 of one 64-bit word and bit 63 of the word before it.
    Below n = 1024 the places around 256 (a multiple of the word as well) take over."""
    T, R, t = EPS_TILE, EPS_TRIP, EPS_OLD_TILE
    want = (0, T, n - 1, T - 1, R, R - 1, T + halo + 1, T - halo - 1, T + halo, T - halo, R + halo, R - halo,
            t, t - 1, t + halo + 1, t - halo - 1, t + halo, t - halo)
    out = []
    for i in want:
        if 0 <= i < n and i not in out:
            out.append(i)
    return out[:12]


def epsilon_case(n, halo, seed=0, nonfinite=False):
    """(e (n,) float32, eps (64,) float64): a noise floor in [0, 0.1), two random bursts in [1, 2), the spikes of spike_indices
    with distinct heights in (2, 3] (the tallest first, so the threshold `own value of spike k` has exactly the first k + 1 spikes
    hot), and 64 thresholds: the 19 of find_epsilon; per spike its own value widened (hot, not pruned) and the next double above
    (pruned, not hot), the tallest first, as many as fit; one below every sample, one above, a NaN; the rest random between the floor
    and the spikes.  nonfinite: NaN and +inf samples as well, away from the spikes."""
    rng = np.random.default_rng([12, n, halo, seed])
    e = (rng.random(n) * 0.1).astype(np.float32)
    for _ in range(2):
        at = int(rng.integers(0, n))
        e[at:at + int(rng.integers(1, 12))] = np.float32(1.0 + rng.random())
    spikes = spike_indices(n, halo)
    for k, i in enumerate(spikes):
        e[i] = np.float32(3.0 - 0.0625 * k - 0.03125 * rng.random())
    if nonfinite:
        free = np.setdiff1d(np.arange(n), spikes)
        at = rng.choice(free, size=12, replace=False)
        e[at[:6]], e[at[6:]] = np.nan, np.inf
    finite = e[np.isfinite(e)].astype(np.float64)
    mean, sd = finite.mean(), finite.std()
    eps = list(mean + sd * np.arange(2.5, 12, 0.5))
    eps += [float(finite.min()) - 1.0, float(finite.max()) + 1.0, float("nan")]
    for i in spikes:                              # at most 12 of them
        own = float(e[i])
        eps += [own, float(np.nextafter(own, np.inf))]
    eps += list(0.1 + rng.random(EPS_NZ - len(eps)) * 2.0)
    return e, np.asarray(eps, dtype=np.float64)


EPS_ROW_BELOW, EPS_ROW_ABOVE, EPS_ROW_NAN, EPS_ROW_OWN = 19, 20, 21, 22      # rows of epsilon_case's thresholds


def part_table_case(halo):
    """The per-part tables' case: parts of PART_TABLE_SCORES scores side by side, part p holding epsilon_case(count, halo, seed p)
    with its own 64 thresholds (an empty part: a NaN row).  Every part has spikes on its first and last score, so a dilation that
    looked across a seam would count the neighbour's.  Returns (x (n,) float32, start, end, eps (P, 64) float64)."""
    cases = [epsilon_case(c, halo, seed=p) if c else (np.zeros(0, np.float32), np.full(EPS_NZ, np.nan)) for p, c in enumerate(PART_TABLE_SCORES)]
    end = np.cumsum(PART_TABLE_SCORES, dtype=np.int64)
    return np.concatenate([c[0] for c in cases]), end - np.asarray(PART_TABLE_SCORES, np.int64), end, np.stack([c[1] for c in cases])


def adjust_labels(kind, n, rng):
    lab = np.zeros(n, np.uint8)
    if kind == "all":
        lab[:] = 1
    elif kind == "alternating":
        lab[1::2] = 1                             # 2049 segments at n = 4099: more than the 256 threads that walk them
    elif kind == "one_at_0":
        lab[0] = 1
    elif kind == "longer_at_0":
        lab[:min(n, 7)] = 1
    elif kind == "ending_at_end":
        lab[max(n - 5, 0):] = 1
    elif kind == "spanning_250_520":
        lab[250:521] = 1                          # across the 256-thread stride; empty below n = 251
    elif kind == "random":
        lab[:] = rng.random(n) < 0.2
    elif kind != "none":
        raise ValueError(kind)
    return lab


def adjust_case(n, kind, seed=0):
    """(score (n,) float32, label (n,) uint8, thresholds (64,) float64): uniform scores with NaNs inside and outside the labelled
    segments; thresholds: 24 exact score values, 24 times the double just below a score (`score > thr` holds in float64 and fails
    once the threshold is rounded to float32), +inf, -inf, NaN and 13 uniform ones."""
    rng = np.random.default_rng([13, n, ADJUST_LABELS.index(kind), seed])
    lab = adjust_labels(kind, n, rng)
    s = rng.random(n).astype(np.float32)
    if n > 2:
        for idx in (np.flatnonzero(lab), np.flatnonzero(lab == 0)):
            if idx.size:
                s[rng.choice(idx, size=min(idx.size, max(1, n // 40)), replace=False)] = np.nan
    pool = s[~np.isnan(s)] if (~np.isnan(s)).any() else s
    exact = rng.choice(pool, size=24).astype(np.float64)
    below = np.nextafter(rng.choice(pool, size=24).astype(np.float64), -np.inf)
    thr = np.concatenate((exact, below, [np.inf, -np.inf, np.nan], rng.random(13)))
    return s, lab, thr


def score_dims(d):
    """A column list into SCORE_ACTUAL_COLUMNS columns: reversed, with one repeat."""
    dims = list(range(SCORE_ACTUAL_COLUMNS - 1, SCORE_ACTUAL_COLUMNS - 1 - d, -1))
    if d > 1:
        dims[d // 2] = dims[0]
    return dims


def score_case(n, d, seed=0):
    """(preds (n, d), recons (n, d), actual (n, 70)) float32 of both signs with magnitudes in [1e-3, 1e3] (no subnormal
    intermediates), with exact equalities p = t and r = t for both column selections of the tests (dims None and score_dims(d))."""
    rng = np.random.default_rng([14, n, d, seed])

    def draw(shape):
        return (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)

    p, r, a = draw((n, d)), draw((n, d)), draw((n, SCORE_ACTUAL_COLUMNS))
    for dims in (list(range(d)), score_dims(d)):
        t = a[:, dims]
        eq_p, eq_r = rng.random((n, d)) < 0.04, rng.random((n, d)) < 0.04
        p[eq_p], r[eq_r] = t[eq_p], t[eq_r]
    return p, r, a
