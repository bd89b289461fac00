"""The specification of the per-part score scaling (evaluation.part_quantiles, scale_scores(parts=),
MTAD_GAT.anomaly_scores(scale_scores="per_part")), in numpy straight from the definitions.  Imports neither the package nor pandas.

The parts are those of part_refs: a series of N rows is the concatenation of P parts with `lengths` rows each, and part p owns the
scores part_refs.spans(lengths, W)[p].  Every (part, column) is a quantile problem of its own."""
import numpy as np

import part_refs
import score_refs


def quantiles(a, lengths, W, qs):
    """score_refs.quantile of every part's slice of an (n,) or (n, d) array: (len(qs), P, d) float64, not rounded.  A (part, column)
    that holds a NaN gives NaN for every q; an empty part gives NaN."""
    a = np.asarray(a)
    if a.ndim == 1:
        a = a[:, None]
    start, end = part_refs.spans(lengths, W)
    out = np.full((len(qs), len(start), a.shape[1]), np.nan, np.float64)
    for p, (s, e) in enumerate(zip(start, end)):
        if e > s:
            out[:, p, :] = score_refs.quantile(a[s:e], qs)
    return out


def scale(a, q3, lengths, W):
    """(a - median) / (1 + (q75 - q25)) with q3 (3, P, d) float32 = q25, median, q75 of the part that owns the row, in float32 with
    every operation rounded on its own -- numpy float32 arithmetic does exactly that.  A row outside every part gives NaN.
    Returns (n, d) float32."""
    a = np.asarray(a, dtype=np.float32)
    a2 = a.reshape(a.shape[0], -1)
    q3 = np.asarray(q3, dtype=np.float32)
    out = np.full(a2.shape, np.nan, np.float32)
    one = np.float32(1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for p, (s, e) in enumerate(zip(*part_refs.spans(lengths, W))):
            if e > s:
                out[s:e] = (a2[s:e] - q3[1, p]) / (one + (q3[2, p] - q3[0, p]))
    assert out.dtype == np.float32
    return out.reshape(a.shape)


# ---- layouts the tests share ---------------------------------------------------------------------------------------------------
def lengths_of(spans_lengths, W):
    """The lengths of the parts of a series whose parts own `spans_lengths` scores each, for window W: the window's rows go to a
    part of their own in front (which owns no score), so span p + 1 of the result has exactly spans_lengths[p] scores."""
    return [W] + [int(v) for v in spans_lengths]


def layouts(L):
    """{name: the scores per part} around the threshold L between the two routes of the select: the boundary lengths, one part over
    everything, short / long / short, two long parts back to back, empty parts first, last and in between, a long part that does
    not start on a multiple of L, and 1 024 parts of a few rows each."""
    return {
        "edges": [0, 1, 2, 3, 255, 256, 257],
        "short": [257],
        "at_L": [L - 1, L, 5],
        "long": [L + 1],
        "short_long_short": [70, L + 1, 33],
        "long_long": [L + 1, L + 2],
        "empty": [0, 300, 0, 0, L + 1, 17, 0],
        "unaligned_long": [L // 2 + 3, L + 64, 7],
        "many": [(p * 7) % 6 for p in range(1024)],
    }
