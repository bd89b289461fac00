"""Reference arithmetic of the score post-processing (quantiles for --scale_scores, the moving average of --use_mov_av),
in numpy float64 straight from the definitions.  Imports neither the package nor pandas."""
import numpy as np


def quantile(a, qs):
    """np.percentile's "linear" definition per column of a (n, d) array, in float64:
    pos = q (n - 1), lo = floor(pos), hi = min(lo + 1, n - 1), v = s[lo] + (s[hi] - s[lo]) (pos - lo).
    A column that holds a NaN gives NaN for every q.  Returns (len(qs), d) float64, not rounded."""
    a = np.asarray(a)
    if a.ndim == 1:
        a = a[:, None]
    n, d = a.shape
    s = np.sort(a.astype(np.float64), axis=0)
    out = np.empty((len(qs), d), np.float64)
    with np.errstate(invalid="ignore"):
        for k, q in enumerate(qs):
            pos = np.float64(q) * np.float64(n - 1)
            lo = int(np.floor(pos))
            hi = min(lo + 1, n - 1)
            out[k] = s[lo] + (s[hi] - s[lo]) * (pos - lo)
    out[:, np.isnan(a).any(axis=0)] = np.nan
    return out


def ewm(x, span):
    """pandas' DataFrame(x).ewm(span=span).mean() (adjust=True): alpha = 2 / (span + 1),
    N_t = x_t + (1 - alpha) N_{t-1}, D_t = (1 - (1 - alpha)^(t + 1)) / alpha (1 for alpha = 1), y_t = N_t / D_t, in float64."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    alpha = 2.0 / (float(span) + 1.0)
    b = 1.0 - alpha
    num = np.empty_like(x)
    acc = 0.0
    for t, v in enumerate(x.tolist()):
        acc = v + b * acc
        num[t] = acc
    if alpha == 1.0:
        return num
    den = (1.0 - np.power(b, np.arange(1, x.size + 1, dtype=np.float64))) / alpha
    return num / den


def ulp32(ref):
    """Spacing of float32 at |ref| (elementwise), as float64."""
    return np.spacing(np.abs(np.asarray(ref, dtype=np.float64)).astype(np.float32)).astype(np.float64)


COLUMN_KINDS = ("uniform", "ties", "signed", "constant", "inf")


def column(kind, n, rng):
    """One float32 test column of length n."""
    if kind == "uniform":
        c = rng.random(n) * 3.0
    elif kind == "ties":
        c = rng.choice(np.array([0.25, 0.5, 1.75, 2.0]), size=n)
    elif kind == "signed":
        c = (rng.random(n) - 0.5) * 2e-3
        for i, v in enumerate((-0.0, 0.0, 1e-41, -3e-42)):            # both zeros and float32 denormals
            if i < n:
                c[(i * 7 + 1) % n] = v
    elif kind == "constant":
        c = np.full(n, 0.625)
    elif kind == "inf":
        c = rng.random(n) * 3.0
        c[n // 2] = np.inf
    else:
        raise ValueError(kind)
    return c.astype(np.float32)


def columns(n, d, rng, rot=0):
    """(n, d) float32 whose column j is of kind COLUMN_KINDS[(j + rot) % 5]."""
    return np.stack([column(COLUMN_KINDS[(j + rot) % len(COLUMN_KINDS)], n, rng) for j in range(d)], axis=1)
