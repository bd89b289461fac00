"""Cases and specification of the forward's non-finite contract (include/mtadgat.h; tests/test_host_nonfinite.py on the CPU,
tests/test_gpu_nonfinite.py on the GPU).

The contract: a sample is non-finite if it is NaN, +inf or -inf.  A window that holds one answers NaN in `preds`, in every element
of `recons` and in `recons_last`; no other window of the call changes beyond what a change of kernel allows.  For a series the
affected windows are exactly those whose rows [start, start + W) contain the sample; for a stream the affected rows are those of
that stream only: the row itself and the next W rows, the row after that scores again.  That is what the unmodified torch-op
algebra (_torchpath.forward) does in float64 and float32: the convolution spreads the sample over all channels, each attention
layer's softmax makes the whole layer output NaN, the GRU carries it to h_end.

This file is the specification in plain Python: it imports nothing but tests/gru_route_cases.py (itself plain Python), uses no GPU
and makes no library call.  It holds the case table -- which model, options, precision mode, window count and source, with the
HAND-WRITTEN pieces and routes the call must take -- the bad windows, sample positions and values of every case, and the pure
functions `affected` (windows) and `affected_rows` (stream rows)."""
import gru_route_cases as rc

NAN, INF = float("nan"), float("inf")
VALUES = {"nan": NAN, "+inf": INF, "-inf": -INF}
VALUE_NAMES = tuple(VALUES)
CLEAN_VALUE = 0.5                                                # what replaces a bad sample in the clean call
X_SEED = 53
GROUP_EDGES = (15, 16, 31, 32, 63, 64, 255, 256)                 # both sides of the 16-, 32-, 64- and 256-window group edges


def positions(W, F, pad):
    """(t, f) of a bad sample inside a window: its corners, the first row no left tap of which leaves the window with a feature the
    convolution's 4-wide staging does not start on, and the last such row at the middle feature."""
    return [(0, 0), (W - 1, F - 1), (pad, 1), (W - 1 - pad, F // 2)]


def bad_windows(pieces):
    """The windows of a call that carry a bad sample, sorted: 0 and n - 1, 15 | 16 and 31 | 32 (the edges of the 16- and 32-window
    groups), 63 | 64 and 255 | 256 (the edges of the waves and workgroups of the kernel that reads the windows' flags), both sides of
    every piece edge.  Their neighbours (1, 14, 17, 30, 33, n - 2, two windows off a piece edge, ...) stay clean: those are the ones
    a leak would reach first."""
    n = sum(pieces)
    bad = set(GROUP_EDGES) | {0, n - 1}
    at = 0
    for p in pieces[:-1]:
        at += p
        bad |= {at - 1, at}
    return sorted(w for w in bad if 0 <= w < n)


def samples(pieces, W, F, pad, rot):
    """[(window, t, f, value name)] of a case's run `rot` (0, 1, 2): bad window number i gets position (i + rot) % 4 and value
    (i + rot) % 3, so the three runs of a case give every bad window every value, and 12 consecutive bad windows every pair."""
    pos = positions(W, F, pad)
    return [(w,) + pos[(i + rot) % 4] + (VALUE_NAMES[(i + rot) % 3],) for i, w in enumerate(bad_windows(pieces))]


def affected(n_windows, W, positions, source):
    """The boolean mask (a list of n_windows bools) of the windows that must answer NaN.
    source "windows" / "windows_bf16": positions are (window, t, f) of the bad samples of an (n, W, F) tensor.
    source "series": positions are (row, f) of a series whose window w starts at row w.
    source ("series", starts): the same with window w starting at row starts[w]."""
    mask = [False] * n_windows
    if source in ("windows", "windows_bf16"):
        for w, t, _ in positions:
            assert 0 <= w < n_windows and 0 <= t < W
            mask[w] = True
        return mask
    starts = list(range(n_windows)) if source == "series" else list(source[1])
    assert (source == "series" or source[0] == "series") and len(starts) == n_windows
    for r, _ in positions:
        for w, s in enumerate(starts):
            if s <= r < s + W:
                mask[w] = True
    return mask


def affected_rows(n_rows, W, bad_rows):
    """Stream rows without a score because of the bad rows: row r scores against the sample itself, rows r + 1 .. r + W - 1 end a
    window that holds it, row r + W is scored with the forecast of the window r .. r + W - 1.  Row r + W + 1 scores again."""
    return [any(r <= k <= r + W for r in bad_rows) for k in range(n_rows)]


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _front(name, n, route, source="windows", mode=2, pieces=None):
    """A front-end route: model, options and window count of tests/test_gpu_front_route.py's CASES[name]; route: the convolution of
    mtadgat_front_route and the two layers' kernels (temporal, feature)."""
    return dict(id="front-" + name, family="front", model=name, options=None, mode=mode, n=n, pieces=list(pieces or [n]), source=source,
                route=route)


def _gru(shape, mode, gk, lanes, n, routes, pieces=None):
    """A recurrence route: a shape of tests/gru_route_cases.py with the options of its table; routes as that table spells them."""
    routes = [routes] if isinstance(routes, str) else list(routes)
    return dict(id="gru-%s-%s-gk%d-n%d" % (shape, rc.MODES[mode], gk, n), family="gru", model=shape, options=dict(gru_kernel=gk, lanes=lanes),
                shape=shape, mode=mode, gru_kernel=gk, lanes=lanes, chunk=None, n=n, pieces=list(pieces or [n]), source="windows",
                routes=routes)


CASES = [
    # front-end routes (tests/test_gpu_front_route.py)
    _front("conv_in_gath", 24, "in_gath | k_gath+k_gat | k_gath+k_gat"),
    _front("conv_win", 24, "k_conv_win | k_gath+k_gat | k_gath+k_gat"),
    _front("conv_lds", 24, "launch_conv | k_gat | k_gat"),
    _front("unfused", 8, "launch_conv | rowgemm+k_gat_wide | rowgemm+k_gat_wide"),
    # the smallest model above 512 features of tests/test_gpu_wide_features.py: both layers' node rows are too long for the pair-grid
    # kernels, the scores go through the score-matrix kernel
    dict(id="front-wide", family="front", model="wide", options={}, mode=2, n=35, pieces=[35], source="windows",
         route="launch_conv | rowgemm+k_attend | rowgemm+k_attend"),
    # a bfloat16 tensor read by the convolution itself, fp32 arithmetic behind it
    dict(id="front-bf16-input", family="front", model="conv_lds", options={}, mode=2, n=24, pieces=[24], source="windows_bf16",
         route="launch_conv | k_gat | k_gat"),
    # recurrence routes: shape A at the smallest n that reaches each first kernel
    _gru("A", 2, 0, 0, 33, "gru1 | gru1"),
    _gru("A", 2, 0, 0, 1793, "gru16 | gru16"),
    _gru("A", 2, 3, 0, 45, "splitx3+tile:x3_lo | splitx3:fc"),
    # (the chunk-major kernel on shape A at the size tests/gru_route_cases.py reaches it with; at 45 windows "gru_kernel" = 2 leaves
    # shape A on the window-per-workgroup kernel and reaches the chunk-major one on the stacked shape B, below)
    _gru("A", 2, 2, 0, 4127, "cm+tile:x3_lo | cm:fc"),
    _gru("A", 2, 1, 1, 10273, "tile:x3_lo | tile:x3_lo:fc"),
    _gru("A", 0, 0, 0, 4097, "split:fp32:xp | split:fp32:fc"),
    _gru("A", 0, 0, 0, 16417, "tile:fp32 | tile:fp32:fc"),
    _gru("A", 1, 0, 0, 1025, "split:bf16:xp | split:bf16:fc"),
    _gru("A", 2, 0, 0, 9001, ["splitx3+tile:x3_lo | splitx3:fc", "gru1 | gru1"], pieces=[8192, 809]),
    # stacked layers
    _gru("B", 2, 0, 0, 45, "split:fp32:xp | split:fp32 | split:fp32 | split:fp32:fc"),
    _gru("B", 2, 2, 0, 45, "cm+tile:x3_lo | cm | cm | split:fp32:fc"),
]
CASE_IDS = [c["id"] for c in CASES]
RUNS = [(c, rot) for c in CASES for rot in range(3)]
RUN_IDS = ["%s-r%d" % (c["id"], rot) for c, rot in RUNS]

# ---- the series: the shared-rows case of tests/test_gpu_front_route.py as a 1 024-window series --------------------------------------
SERIES_MODEL, SERIES_WINDOWS, SERIES_ROUTE = "shared_rows", 1024, "shared_rows | k_gat | k_gat"
SERIES_STRIDE = 3
# one window fewer (series_losses: the last window of the series has no target row) and strided starts leave the shared rows
SERIES_LOSSES_ROUTE = SERIES_STRIDED_ROUTE = "k_conv_win | k_gat | k_gat"


def series_row_groups(n_rows, W, pad):
    """The bad rows of a series of n_rows rows -- 0, pad, W - 1, the middle, n_rows - 1 - pad, n_rows - 1 -- in three groups, one call
    each, chosen so that the spans of a group's rows are disjoint and the windows just outside each span (r - W and r + 1) are clean
    in that call."""
    return [[0, n_rows // 2, n_rows - 1], [pad, n_rows - 1 - pad], [W - 1]]


def series_samples(n_rows, W, F, pad, group, rot):
    """[(row, f, value name)] of run (group, rot): the features of `positions`, the values in turn."""
    feats = [f for _, f in positions(W, F, pad)]
    rows = series_row_groups(n_rows, W, pad)[group]
    return [(r, feats[(i + group + rot) % 4], VALUE_NAMES[(i + rot) % 3]) for i, r in enumerate(rows)]


# ---- the streams: the model of tests/test_gpu_stream.py, S = 5 ------------------------------------------------------------------------
STREAMS, STREAM_MAX_BLOCK, STREAM_ROWS = 5, 7, 63                # ring of W + 6 rows; 63 rows: 63 pushes of 1 row, 9 of 7
STREAM_PUSHES = (1, 7)


def stream_samples(W, F, rot):
    """[(stream, row, f, value name)]: stream 1 early, stream 3 at the last row of its ring's second lap (row 2 R - 1, R = W +
    STREAM_MAX_BLOCK - 1), so the windows that hold it wrap around the ring."""
    R = W + STREAM_MAX_BLOCK - 1
    return [(1, W + 5, 0, VALUE_NAMES[rot % 3]), (3, 2 * R - 1, F - 1, VALUE_NAMES[(rot + 1) % 3])]
