"""How a forward call is cut into pieces, which lane each piece runs on, whether a small call forks its stages, and where each lane's
part of the workspace begins (plan_forward, queried through mtadgat_forward_plan) -- and every workspace / tape / scratch size the
library reports.  No GPU needed.  Outputs pass their tolerances under any schedule, so a shifted threshold would otherwise be a silent
slowdown or a silent overlap of the two lanes' scratch.

The references are not taken from plan_forward.  The sizes are those the commit before it reported (tests/golden/plan_sizes.json,
written there by tests/golden/make_plan_sizes.py); `_parent_schedule` / `_parent_fork` transcribe that commit's forward_schedule and
the `second` / `fork` predicates of its forward_impl (mtadgat_capi.cpp) line by line."""
import ctypes
import json
import os
import sys

import pytest

from helpers import GOLDEN_DIR

if GOLDEN_DIR not in sys.path:
    sys.path.insert(0, GOLDEN_DIR)
import make_plan_sizes as rec  # noqa: E402

SHAPES = rec.shapes()
INVALID = -1                                                     # MTADGAT_ERR_INVALID
HEAD = 5                                                         # [n_pieces, fork, lane0_floats, lane1_floats, total_floats]


def _golden():
    with open(rec.PATH) as f:
        return json.load(f)


def _plan(lib, h, batch):
    """mtadgat_forward_plan as a dict; the pieces as (c0, n, lane)."""
    got = lib.mtadgat_forward_plan(h, batch, _BUF, _CAP)
    assert HEAD + 3 <= got < _CAP, (batch, got, lib.mtadgat_last_error())
    v = _BUF[:got]
    assert got == HEAD + 3 * v[0] and _BUF[got] == -7                            # the count of values written, nothing beyond them
    _BUF[:got] = [-7] * got
    return dict(fork=v[1], lane_floats=(v[2], v[3]), total_floats=v[4], pieces=[tuple(v[i:i + 3]) for i in range(HEAD, got, 3)])


_CAP = HEAD + 3 * 4200                                           # (config 4 in chunks of 24 windows: 4 167 pieces of 100 000 windows)
_BUF = (ctypes.c_int64 * _CAP)(*([-7] * _CAP))


# ---- reference: forward_schedule and forward_impl's predicates of the commit before plan_forward, transcribed ------------------------
def _ru(v, m):
    return (v + m - 1) // m * m


def _parent_fused(K, D):
    """validate_and_plan's plan_gat (mtadgat_pack.cpp): the fused kernel takes a layer of K nodes of dimension D."""
    if not (K <= 128 and D <= 128):
        return False
    rows = (K + 15) // 16 * 16
    vld = 8 * ((D + 8) // 8) + 4
    lr = _ru(max((rows + K) * 34, rows * 68), 4)
    return (_ru(K, 16) * vld + lr) * 4 <= 80 * 1024


def _parent_both_fused(kw):
    F, W = kw["n_features"], kw["window_size"]
    return _parent_fused(F, W) and _parent_fused(W, F)


def _parent_schedule(both_fused, precision, lanes, chunk, batch, pieces_env=None):
    out = []
    two = lanes == 0 and precision == 2 and both_fused
    alt = lanes == 0 and not both_fused and batch > chunk and pieces_env is None
    if alt:
        c0, ci = 0, 0
        half = max(32, chunk // 2 // 32 * 32)
        while c0 < batch:
            n = min(half if ci == 0 else chunk, batch - c0)
            out.append((c0, n, ci & 1))
            c0 += n
            ci += 1
        return out
    for c0 in range(0, batch, chunk):
        n = min(chunk, batch - c0)
        k, base = 1, n
        if two and 8192 < n <= 2 * 8192:
            k = 2
            base = n // 2 // 32 * 32
            if n - 8192 <= 1536:
                base = 8192
        elif two and n > 32768 and n % 32768 != 0:
            k = (n + 32767) // 32768
            base = 32768
        if pieces_env is not None:
            at, lane = 0, 0
            for tok in pieces_env.split(","):                    # (strtoll over "a,b,c")
                if at >= n:
                    break
                ln = min(n - at, int(tok))
                if ln <= 0:
                    break
                out.append((c0 + at, ln, lane))
                lane ^= 1
                at += ln
            if at < n:
                out.append((c0 + at, n - at, lane))
            continue
        at = 0
        for i in range(k):
            ln = base if i + 1 < k else n - at
            out.append((c0 + at, ln, i & 1))
            at += ln
    return out


def _parent_fork(both_fused, lanes, sched):
    second = any(lane == 1 for _, _, lane in sched)
    return not second and len(sched) == 1 and lanes == 0 and sched[0][1] <= 1024 and both_fused


def _combinations(lib, h, name):
    for mode in rec.MODES:
        assert lib.mtadgat_set_precision(h, mode) == 0
        for lanes in rec.LANES:
            assert lib.mtadgat_set_option(h, b"lanes", lanes) == 0
            for chunk in rec.chunks_of(name):
                assert lib.mtadgat_set_chunk_windows(h, chunk) == 0
                yield mode, lanes, chunk


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
def test_the_fixture_covers_the_recorded_cases():
    g = _golden()
    assert g["batches"] == list(rec.BATCHES) and set(g["shapes"]) == set(SHAPES)
    for name, r in g["shapes"].items():
        assert r["kwargs"] == SHAPES[name], name
        keys = {rec.key(m, l, c) for m in rec.MODES for l in rec.LANES for c in rec.chunks_of(name)}
        assert set(r["workspace"]) == keys and set(r["stream"]) == keys, name
        # every shape here has a HIP backward: none of the training / attribution sizes is skipped
        assert r["backward_supported"] == 1 and len(r["train_layout"]) == len(rec.BATCHES), name
        assert all(len(v) == rec.N_LAYOUT for v in r["train_layout"]), name


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_size_query_equals_the_recorded_one(name):
    want = _golden()["shapes"][name]
    got = json.loads(json.dumps(rec.collect_shape(name, SHAPES[name])))          # (lists and string keys, as the fixture holds them)
    assert set(got) == set(want)
    for what in want:
        if isinstance(want[what], dict) and what != "kwargs":
            for k in want[what]:
                assert got[what][k] == want[what][k], (name, what, k)
        else:
            assert got[what] == want[what], (name, what)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_plans_equal_the_transcribed_schedule(name):
    lib, h = rec.create(SHAPES[name])
    both_fused = _parent_both_fused(SHAPES[name])
    one_piece = {}                                               # floats of a call of n windows in one piece on one lane (plan_workspace's total)

    def single(n):
        if n not in one_piece:
            assert lib.mtadgat_set_option(h, b"lanes", 1) == 0 and lib.mtadgat_set_chunk_windows(h, max(n, 65536)) == 0
            p = _plan(lib, h, n)
            assert p["pieces"] == [(0, n, 0)] and p["lane_floats"] == (p["total_floats"], 0), (name, n, p)
            one_piece[n] = p["total_floats"]
        return one_piece[n]

    try:
        lane1_used = forks = 0
        for mode, lanes, chunk in _combinations(lib, h, name):
            for batch in rec.BATCHES:
                p = _plan(lib, h, batch)
                what = (name, mode, lanes, chunk, batch)
                sched = _parent_schedule(both_fused, mode, lanes, chunk, batch)
                assert p["pieces"] == sched, (what, p)                                       # transcribed
                assert p["fork"] == int(_parent_fork(both_fused, lanes, sched)), (what, p)   # transcribed
                # invariants: contiguous, non-empty pieces; the lanes' parts fit the reported total, which is what
                # mtadgat_workspace_bytes reports; lane 1 has scratch exactly when a piece runs there
                at = 0
                for c0, n, lane in p["pieces"]:
                    assert c0 == at and n > 0 and lane in (0, 1), (what, p)
                    at += n
                assert at == batch, (what, p)
                l0, l1 = p["lane_floats"]
                assert l0 + l1 <= p["total_floats"] and p["total_floats"] * 4 == lib.mtadgat_workspace_bytes(h, batch), (what, p)
                assert (l1 == 0) == all(lane == 0 for _, _, lane in p["pieces"]), (what, p)
                lane1_used += l1 > 0
                forks += p["fork"]
                # every piece's own plan fits its lane -- and each lane is exactly as large as its largest piece needs
                need = [0, 0]
                for _, n, lane in p["pieces"]:
                    need[lane] = max(need[lane], single(n))
                assert lib.mtadgat_set_option(h, b"lanes", lanes) == 0 and lib.mtadgat_set_chunk_windows(h, chunk) == 0
                assert (l0, l1) == tuple(need), (what, p, need)
        assert lane1_used > 0 or name not in ("msl", rec.CONFIG4), name
        assert forks > 0 or not both_fused, name
    finally:
        lib.mtadgat_set_option(h, b"lanes", 0)
        lib.mtadgat_destroy(h)


def test_schedule_edges_by_hand():
    """The bands of the transcription, spelled out once for the flagship shape (split-operand arithmetic, chunk of 65 536 windows) and
    for BASELINE config 4's alternating chunks -- so that a reader sees the walk, and the transcription itself is pinned."""
    f = lambda batch, chunk=65536, fused=True, lanes=0: [(n, lane) for _, n, lane in _parent_schedule(fused, 2, lanes, chunk, batch)]
    assert f(8192) == [(8192, 0)] and f(8193) == [(8192, 0), (1, 1)]                         # two pieces above the hidden-tile-split band
    assert f(8192 + 1536) == [(8192, 0), (1536, 1)] and f(8192 + 1537) == [(4864, 0), (4865, 1)]    # a short tail rides beside a full piece
    assert f(16384) == [(8192, 0), (8192, 1)] and f(16385) == [(16385, 0)]
    assert f(32768) == [(32768, 0)] and f(32769) == [(32768, 0), (1, 1)]                     # full k_gru_cm rounds, then the rest
    assert f(65536) == [(65536, 0)] and f(98304, chunk=98304) == [(98304, 0)]                # whole multiples stay one piece
    assert f(98304) == [(65536, 0), (32768, 0)]                                              # (chunk by chunk)
    assert f(100000) == [(65536, 0), (32768, 0), (1696, 1)]
    assert f(23000, chunk=10000) == [(4992, 0), (5008, 1)] * 2 + [(3000, 0)]                 # several chunks, a ragged last one
    assert f(9000, lanes=1) == [(9000, 0)]
    # un-fused layers: chunks alternate between the lanes, the first piece is half a chunk -- at least 32 windows, also where that is
    # more than the chunk
    assert f(2048, chunk=896, fused=False) == [(448, 0), (896, 1), (704, 0)]
    assert f(64, chunk=24, fused=False) == [(32, 0), (24, 1), (8, 0)]
    assert f(896, chunk=896, fused=False) == [(896, 0)] and f(64, chunk=24, fused=False, lanes=1) == [(24, 0), (24, 0), (16, 0)]


@pytest.mark.parametrize("name", ["msl", "many_nodes", rec.CONFIG4])
def test_fork_flag_on_both_sides_of_its_edge(name):
    """Small calls fork their independent stages onto the second lane: up to 1024 windows, both attention layers fused, lanes automatic."""
    lib, h = rec.create(SHAPES[name])
    both_fused = _parent_both_fused(SHAPES[name])
    assert both_fused == (name == "msl")
    try:
        assert lib.mtadgat_set_chunk_windows(h, 65536) == 0
        for mode in rec.MODES:
            assert lib.mtadgat_set_precision(h, mode) == 0
            for lanes in rec.LANES:
                assert lib.mtadgat_set_option(h, b"lanes", lanes) == 0
                assert _plan(lib, h, 1024)["fork"] == int(both_fused and lanes == 0), (name, mode, lanes)
                assert _plan(lib, h, 1025)["fork"] == 0, (name, mode, lanes)
    finally:
        lib.mtadgat_set_option(h, b"lanes", 0)
        lib.mtadgat_destroy(h)


def test_the_pieces_hook_cuts_every_chunk_as_told():
    """MTADGAT_PIECES = "a,b,c" (measurement hook): piece sizes of every chunk, alternating lanes, the rest as a last piece."""
    assert "MTADGAT_PIECES" not in os.environ
    for name, chunk in (("msl", 65536), ("msl", 6000), (rec.CONFIG4, 896)):
        lib, h = rec.create(SHAPES[name])
        both_fused = _parent_both_fused(SHAPES[name])
        try:
            assert lib.mtadgat_set_chunk_windows(h, chunk) == 0
            for mode in rec.MODES:
                assert lib.mtadgat_set_precision(h, mode) == 0
                os.environ["MTADGAT_PIECES"] = "5000,3000"
                try:
                    plans = {batch: _plan(lib, h, batch) for batch in (9000, 7000)}
                finally:
                    del os.environ["MTADGAT_PIECES"]
                for batch, p in plans.items():
                    sched = _parent_schedule(both_fused, mode, 0, chunk, batch, "5000,3000")
                    assert p["pieces"] == sched and p["fork"] == 0, (name, chunk, mode, batch, p)
                    assert (p["lane_floats"][1] > 0) == any(lane for _, _, lane in sched), (name, chunk, mode, batch, p)
                    assert sum(p["lane_floats"]) <= p["total_floats"], (name, chunk, mode, batch, p)
                assert _plan(lib, h, 9000)["pieces"] == _parent_schedule(both_fused, mode, 0, chunk, 9000)       # the hook is gone again
        finally:
            lib.mtadgat_destroy(h)
    assert _parent_schedule(True, 2, 0, 65536, 9000, "5000,3000") == [(0, 5000, 0), (5000, 3000, 1), (8000, 1000, 0)]
    assert _parent_schedule(True, 2, 0, 65536, 7000, "5000,3000") == [(0, 5000, 0), (5000, 2000, 1)]


def test_hook_rejects_bad_arguments_and_needs_no_weights():
    lib, h = rec.create(SHAPES["msl"])
    try:
        assert lib.mtadgat_set_precision(h, 2) == 0 and lib.mtadgat_set_chunk_windows(h, 65536) == 0
        buf = (ctypes.c_int64 * 16)(*([-7] * 16))
        assert lib.mtadgat_forward_plan(h, 9000, buf, 16) == HEAD + 6             # no weights loaded, no GPU touched
        assert list(buf[:2]) == [2, 0] and list(buf[HEAD:HEAD + 6]) == [0, 8192, 0, 8192, 808, 1] and list(buf[HEAD + 6:]) == [-7] * 5
        assert lib.mtadgat_forward_plan(None, 9000, buf, 16) == INVALID
        assert lib.mtadgat_forward_plan(h, 9000, None, 16) == INVALID
        assert lib.mtadgat_forward_plan(h, 0, buf, 16) == INVALID and lib.mtadgat_forward_plan(h, -5, buf, 16) == INVALID
        untouched = (ctypes.c_int64 * 16)(*([-7] * 16))
        assert lib.mtadgat_forward_plan(h, 9000, untouched, HEAD + 5) == INVALID and lib.mtadgat_forward_plan(h, 256, untouched, HEAD + 2) == INVALID
        assert list(untouched) == [-7] * 16                                      # an array that is too small is left alone
        assert lib.mtadgat_forward_plan(h, 256, untouched, HEAD + 3) == HEAD + 3 and list(untouched[:2]) == [1, 1]
    finally:
        lib.mtadgat_destroy(h)
