"""The specification of the package's peaks-over-threshold thresholds (csrc/mtadgat_spot.h), in numpy.

This is SPOT (Siffer et al., KDD 2017: Algorithm 1 with Grimshaw's reduction of the generalized Pareto likelihood to the roots of
one scalar function) as THIS package defines it -- not a port of the reference's spot.py, whose optimiser-based root search cannot
be reproduced bit for bit.  Every function takes a dtype, so the same statements run in float64 (what the device and the host hook
compute) and in np.longdouble (how far float64 can be trusted on a given input).

  sums over the m stored peaks Y (oldest first): 64 accumulators, accumulator l adds the elements i = l (mod 64) in ascending
      order; then an xor butterfly (32, 16, .. 1) combines them -- the order of a 64-lane wave
  Ymean = sum(Y) / m,  u(x) = 1 + sum(log(1 + x Y)) / m,  v(x) = sum(1 / (1 + x Y)) / m,  w(x) = u(x) v(x) - 1
  candidates, in this order: (gamma, sigma) = (0, Ymean); the roots of w in (-1/Ymax + e, -1e-3 / Ymean), ascending, e = 1e-8 or
      1 / (32 Ymax) when 1/Ymax < 2e, skipped when empty; the roots of w in (2 (Ymean - Ymin) / (Ymean Ymin), 2 (Ymean - Ymin) / Ymin^2),
      ascending, when Ymean > Ymin
  roots: w at the 32 points lo + (hi - lo) k / 31; adjacent finite values whose (w < 0) differ are a bracket; 64 bisections, the end
      whose (w < 0) equals the midpoint's is replaced; the root is the last interval's midpoint; gamma = u(root) - 1, sigma = gamma / root,
      kept when sigma is finite and positive and gamma != 0
  choice: the largest finite L = -m log sigma - (1 + 1/gamma) sum(log(1 + (gamma / sigma) Y))  (gamma = 0: -m (1 + log Ymean)); ties
      go to the earlier candidate
  threshold, r = q n / Nt: z = t + (sigma / gamma) (r^-gamma - 1), or t - sigma log r for gamma = 0

The state of one series is (t, z, n, Nt, gamma, sigma) and the most recent max_peaks excesses -- the package's own bound: Nt counts
every excess, the fit sees the stored ones only.  `step` is the rule for one score.
"""
import numpy as np

EPS = 1e-8
GRID = 32
BISECTIONS = 64
MIN_PEAKS = 8


def wave_sum(values, dtype=np.float64):
    """The sum over the last axis of `values` in the order of a wave.  The butterfly is written as the tree lane 0 sees: every lane
    ends with the same bits, a + b being b + a."""
    values = np.asarray(values, dtype=dtype)
    acc = np.zeros(values.shape[:-1] + (64,), dtype=dtype)
    for at in range(0, values.shape[-1], 64):
        part = values[..., at:at + 64]
        acc[..., :part.shape[-1]] = acc[..., :part.shape[-1]] + part
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :off] + acc[..., off:]
    return acc[..., 0]


def _uw(Y, x, dtype):
    """u and w at x; x may be an array of points (evaluated independently, one row each)."""
    m = dtype(Y.size)
    one = dtype(1)
    x = np.asarray(x, dtype=dtype)
    a = one + x[..., None] * Y
    with np.errstate(all="ignore"):
        sums = wave_sum(np.stack((np.log(a), one / a)), dtype)
        u = one + sums[0] / m
        v = sums[1] / m
        return u, u * v - one


def _roots(Y, lo, hi, dtype):
    out = []
    xs = lo + (hi - lo) * np.arange(GRID).astype(dtype) / dtype(GRID - 1)
    ws = _uw(Y, xs, dtype)[1]
    for k in range(1, GRID):
        wp, wk = ws[k - 1], ws[k]
        if np.isfinite(wp) and np.isfinite(wk) and (wp < 0) != (wk < 0):
            l, h, lneg = xs[k - 1], xs[k], bool(wp < 0)
            for _ in range(BISECTIONS):
                mid = (l + h) / dtype(2)
                if bool(_uw(Y, mid, dtype)[1] < 0) == lneg:
                    l = mid
                else:
                    h = mid
            out.append((l + h) / dtype(2))
    return out


def interval_roots(peaks, dtype=np.float64):
    """(roots in the left interval, roots in the right interval) of w for the stored excesses, each ascending; a skipped interval
    has none."""
    Y = np.asarray(peaks, dtype=dtype)
    m, one = dtype(Y.size), dtype(1)
    ymin, ymax = Y.min(), Y.max()
    ymean = wave_sum(Y, dtype) / m
    left, right = [], []
    with np.errstate(all="ignore"):
        eps = dtype(EPS)
        if one / ymax < dtype(2) * eps:
            eps = one / (dtype(32) * ymax)
        lo, hi = -one / ymax + eps, dtype(-1e-3) / ymean
        if lo < hi:
            left = _roots(Y, lo, hi, dtype)
        if ymean > ymin:
            a = dtype(2) * (ymean - ymin)
            right = _roots(Y, a / (ymean * ymin), a / (ymin * ymin), dtype)
    return left, right


def fit(peaks, n, Nt, t, q, dtype=np.float64):
    """(gamma, sigma, z) for the stored excesses `peaks` (oldest first), n observations, Nt excesses, initial threshold t, risk q."""
    Y = np.asarray(peaks, dtype=dtype)
    m, one = dtype(Y.size), dtype(1)
    t, q = dtype(t), dtype(q)
    ymean = wave_sum(Y, dtype) / m
    left, right = interval_roots(Y, dtype)
    with np.errstate(all="ignore"):
        best_g, best_s = dtype(0), ymean
        best_L = -m * (one + np.log(ymean))
        if not np.isfinite(best_L):
            best_L = dtype(-np.inf)
        for x in left + right:
            g = _uw(Y, x, dtype)[0] - one
            s = g / x
            if not (np.isfinite(s) and s > 0) or g == 0 or g != g:
                continue
            L = -m * np.log(s) - (one + one / g) * wave_sum(np.log(one + (g / s) * Y), dtype)
            if np.isfinite(L) and L > best_L:
                best_g, best_s, best_L = g, s, L
        r = q * dtype(n) / dtype(Nt)
        if best_g != 0:
            z = t + (best_s / best_g) * (r ** (-best_g) - one)
        else:
            z = t - best_s * np.log(r)
    return best_g, best_s, z


class State:
    """One series' state.  `peaks` holds the last max_peaks excesses, oldest first."""

    def __init__(self, t, peaks, n, Nt, q, max_peaks, dtype):
        self.t, self.n, self.Nt, self.q, self.max_peaks, self.dtype = dtype(t), int(n), int(Nt), q, int(max_peaks), dtype
        self.peaks = list(peaks)[-self.max_peaks:]
        self.gamma, self.sigma, self.z = fit(self.peaks, self.n, self.Nt, self.t, q, dtype)

    def copy(self):
        other = State.__new__(State)
        other.__dict__.update(self.__dict__)
        other.peaks = list(self.peaks)
        return other

    def step(self, x, dynamic):
        """(threshold the score was compared with, flag); the state advances as the definition says."""
        z = self.z
        x = self.dtype(x)
        if x != x:
            return z, False
        if x > z:
            return z, True
        if dynamic:
            if x > self.t:
                self.peaks.append(x - self.t)
                del self.peaks[:-self.max_peaks]
                self.Nt += 1
                self.n += 1
                self.gamma, self.sigma, self.z = fit(self.peaks, self.n, self.Nt, self.t, self.q, self.dtype)
            else:
                self.n += 1
        return z, False


def calibrate(init, q, level, max_peaks, dtype=np.float64):
    """The state after the calibration scores `init` (1-D): t = sorted[int(level * n_init)], the excesses in order, the first fit."""
    init = np.asarray(init)
    if np.isnan(init).any():
        raise ValueError("the calibration scores hold a NaN")
    t = dtype(np.sort(init)[int(level * init.size)])
    x = init.astype(dtype)
    peaks = list(x[x > t] - t)
    if len(peaks) < MIN_PEAKS:
        raise ValueError("fewer than 8 excesses over the initial threshold")
    return State(t, [dtype(p) for p in peaks], init.size, len(peaks), q, max_peaks, dtype)


def run(state, scores, dynamic):
    """(thresholds (n,) of the state's dtype, flags (n,) bool) over the scores in order; `state` is advanced."""
    thr = np.empty(len(scores), dtype=state.dtype)
    flags = np.zeros(len(scores), dtype=bool)
    for i, x in enumerate(scores):
        thr[i], flags[i] = state.step(x, dynamic)
    return thr, flags
