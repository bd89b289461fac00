"""Seeded score matrices for the peaks-over-threshold tests and their reference (tests/spot_refs.py), computed once per case and
shared.  Every matrix carries the situations the step has to get right: NaN rows, a level shift (the last third of the scores times
1.5) and a burst of alarms.

`reference(case, dynamic)` also checks the two conditions under which a 1e-9 gate against the float64 reference is meaningful, on
the CPU, before anything is compared with the device:
  * the float64 and the long-double runs of the reference agree to 1e-10 relative on every threshold (and raise the same flags);
  * no score lies within 1e-6 relative of the threshold it was compared with, or of its column's initial threshold t.
Both are properties of the seeded input.  A seed that fails them is replaced by another one; the bounds stay.
"""
import numpy as np

import spot_refs

Q = 1e-3

#          S  n_init  rows  max_peaks  level  seed
CASES = {
    "one column":         (1, 2000, 3000, 256, 0.98, 11),      # the ring never wraps: SPOT's Algorithm 1
    "three columns":      (3, 2000, 1500, 8, 0.98, 12),        # the ring wraps at once (40 calibration excesses for 8 slots)
    "five columns":       (5, 200, 600, 256, 0.90, 13),        # a second workgroup; a short calibration
    "seventy columns":    (70, 2000, 600, 8, 0.99, 14),        # many workgroups
}

_DATA, _REFS = {}, {}


def data(case):
    """(init (n_init, S), scores (rows, S)) float32."""
    if case not in _DATA:
        S, n_init, rows, _, _, seed = CASES[case]
        rng = np.random.default_rng(seed)
        scale = 0.5 + rng.random(S)
        init = (rng.gamma(4.0, 0.05, (n_init, S)) * scale).astype(np.float32)
        x = rng.gamma(4.0, 0.05, (rows, S)) * scale
        x[rows - rows // 3:] *= 1.5                                         # the level shift
        for c in range(S):
            at = 50 + (37 * c) % (rows // 2)
            x[at:at + 10, c] = 20.0 * scale[c] * (1.0 + rng.random(10))    # a burst of alarms
            x[(at + 200) % rows, c] = np.nan                               # a NaN of the column's own
        x[[17, 18, rows // 2]] = np.nan                                     # whole NaN rows
        _DATA[case] = (init, x.astype(np.float32))
    return _DATA[case]


def _close(x, ref, rel):
    with np.errstate(invalid="ignore"):
        return np.abs(x - ref) <= rel * np.abs(ref)


def reference(case, dynamic):
    """A dict: t (S,), z0 (S,) the calibrated thresholds, thresholds (rows, S) float64, flags (rows, S) bool, n and Nt (S,) after the
    run -- from the float64 reference, with the input conditions asserted."""
    key = (case, bool(dynamic))
    if key in _REFS:
        return _REFS[key]
    S, n_init, rows, max_peaks, level, _ = CASES[case]
    init, x = data(case)
    out = {"t": np.empty(S), "z0": np.empty(S), "thresholds": np.empty((rows, S)), "flags": np.zeros((rows, S), bool),
           "n": np.empty(S, np.int64), "Nt": np.empty(S, np.int64)}
    for c in range(S):
        runs = {}
        for dtype in (np.float64, np.longdouble):
            st = spot_refs.calibrate(init[:, c], Q, level, max_peaks, dtype)
            z0 = st.z
            thr, flags = spot_refs.run(st, x[:, c], dynamic)
            runs[dtype] = (z0, thr, flags, st)
        (z0, thr, flags, st), (z0w, thrw, flagsw, _) = runs[np.float64], runs[np.longdouble]
        assert abs(z0 - z0w) <= 1e-10 * abs(z0w) and np.all(_close(thr.astype(np.longdouble), thrw, 1e-10)), (case, c, "pick another seed")
        assert np.array_equal(flags, flagsw), (case, c, "pick another seed")
        xc = x[:, c].astype(np.float64)
        seen = ~np.isnan(xc)
        assert not np.any(_close(xc[seen], thr[seen], 1e-6)) and not np.any(_close(xc[seen], float(st.t), 1e-6)), (case, c, "pick another seed")
        out["t"][c], out["z0"][c], out["thresholds"][:, c], out["flags"][:, c], out["n"][c], out["Nt"][c] = st.t, z0, thr, flags, st.n, st.Nt
    _REFS[key] = out
    return out
