"""The table of steps that derives the split weight packs (mtadgat_split_steps), checked on the CPU against the regions the library
reports (mtadgat_derived_regions) and against the footprints of tests/split_refs.py; and split_refs' own conversions against their
contracts.  tests/test_gpu_split_packs.py replays the same table on the images the device kernels write.

The scale slots are the one place where steps share a destination by design: a group's ZERO_SCALE, ABSMAX and SCALE_FROM_MAX steps
all write its 4-float slot.  They are checked as a sequence (below); the disjointness and one-writer rules apply to every other
step."""
import ctypes

import numpy as np
import pytest

import gat_sign_cases as gc
import split_refs as sr
from test_host_derived_regions import SHAPES as REGION_SHAPES
from test_host_derived_regions import _create

SHAPES = dict(REGION_SHAPES)
SHAPES.update({"sign_" + k: v for k, v in gc.SHAPES.items()})

_TABLES = {}


def table(name):
    """(steps, regions, n_infer, packed floats) of a shape, read once."""
    if name not in _TABLES:
        import _native
        lib, _, h = _create(SHAPES[name])
        try:
            steps = _native.split_steps(lib, h)
            n = lib.mtadgat_derived_regions(h, None, 0)
            buf = (ctypes.c_int64 * (2 * n))()
            lib.mtadgat_derived_regions(h, buf, n)
            regions = [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n)]
            _TABLES[name] = (steps, regions, int(lib.mtadgat_split_n_infer(h)), int(lib.mtadgat_packed_floats(h)))
        finally:
            lib.mtadgat_destroy(h)
    return _TABLES[name]


def _inside(span, region):
    return region[0] <= span[0] and span[0] + span[1] <= region[0] + region[1]


def _overlap(a, b):
    return a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


def _groups(steps):
    out = {}
    for s in steps:
        out.setdefault(s["group"], []).append(s)
    return out


def test_split_steps_follows_the_count_query_convention():
    lib, _, h = _create(SHAPES["stacked"])
    try:
        n = lib.mtadgat_split_steps(h, None, 0)                     # count query
        assert n > 0
        buf = (ctypes.c_int64 * (10 * n + 10))(*([-7] * (10 * n + 10)))
        assert lib.mtadgat_split_steps(h, buf, n) == n
        assert list(buf[10 * n:]) == [-7] * 10                      # nothing written beyond max_steps
        full = list(buf[:10 * n])
        assert all(0 <= full[10 * i + 1] < len(sr.OPS) for i in range(n))
        groups = [full[10 * i] for i in range(n)]
        assert groups == sorted(groups) and groups[0] == 0 and set(groups) == set(range(groups[-1] + 1))   # group order, none empty
        # a short buffer receives the first records, the return value stays the full count
        short = (ctypes.c_int64 * 40)(*([-7] * 40))
        assert lib.mtadgat_split_steps(h, short, 3) == n
        assert list(short[:30]) == full[:30] and list(short[30:]) == [-7] * 10
        assert 0 < lib.mtadgat_split_n_infer(h) <= groups[-1] + 1
        assert lib.mtadgat_split_steps(None, None, 0) == 0 and lib.mtadgat_split_n_infer(None) == 0
        import _native
        assert _native.SPLIT_OPS == sr.OPS
        assert [s["op"] for s in _native.split_steps(lib, h)] == [sr.OPS[full[10 * i + 1]] for i in range(n)]
    finally:
        lib.mtadgat_destroy(h)


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_destination_fits_one_region_and_every_region_has_one_writer(name):
    steps, regions, _, total = table(name)
    writers = {r: [] for r in regions if r[1] > 0}
    for s in steps:
        span = sr.dst_span(s)
        assert span[1] > 0, s
        home = [r for r in writers if _inside(span, r)]
        assert len(home) == 1, (name, s, span)                      # inside exactly one reported region, and fits it
        assert all(r == home[0] or not _overlap(span, r) for r in writers), (name, s)
        if s["op"] in sr.SCALE_OPS:
            assert home[0] == (s["scale"], 4), (name, s)            # a slot is a region of its own
        else:
            writers[home[0]].append(s)
    for r, w in writers.items():
        if r[1] > 4:
            assert len(w) == 1, (name, r, w)                        # (which also makes the destinations of different steps disjoint)
        else:
            assert r[1] == 4 and not w, (name, r, w)                # the other regions are scale slots
    spans = sorted(sr.dst_span(s) for s in steps if s["op"] not in sr.SCALE_OPS)
    for a, b in zip(spans, spans[1:]):
        assert a[0] + a[1] <= b[0], (name, a, b)
    assert all(0 <= r[0] and r[0] + r[1] <= total for r in regions)


@pytest.mark.parametrize("name", list(SHAPES))
def test_scale_slots_are_zeroed_ranged_and_scaled_before_they_are_read(name):
    steps, _, _, _ = table(name)
    slot_group = {}
    for g, gs in _groups(steps).items():
        for i, s in enumerate(gs):
            if s["op"] in sr.SCALE_OPS:
                assert slot_group.setdefault(s["scale"], g) == g, (name, s)     # no two groups share a slot
            if s["op"] not in ("SPLIT2H", "SPLIT2H_GATH", "SPLIT_X"):
                continue
            before = [t for t in gs[:i] if t["op"] in sr.SCALE_OPS and t["scale"] == s["scale"]]
            ops = [t["op"] for t in before]
            assert ops and ops[0] == "ZERO_SCALE" and ops[-1] == "SCALE_FROM_MAX", (name, s, ops)
            assert ops.count("ZERO_SCALE") == 1 and ops.count("SCALE_FROM_MAX") == 1 and ops.count("ABSMAX") >= 1, (name, s, ops)
            # ... and the range covers what is scaled: S v stays below 2^14 only for values the maximum was taken over
            src = (s["src"], sr.footprint(s)[0])
            assert any(_inside(src, (t["src"], t["n"])) for t in before if t["op"] == "ABSMAX"), (name, s)
        # nothing touches a slot once it is scaled
        for sc in {s["scale"] for s in gs if s["op"] in sr.SCALE_OPS}:
            ops = [t["op"] for t in gs if t["op"] in sr.SCALE_OPS and t["scale"] == sc]
            assert ops == ["ZERO_SCALE"] + ["ABSMAX"] * (len(ops) - 2) + ["SCALE_FROM_MAX"], (name, sc, ops)


@pytest.mark.parametrize("name", list(SHAPES))
def test_sources_are_fp32_packs_and_no_chunk_is_dropped(name):
    steps, regions, _, total = table(name)
    for g, gs in _groups(steps).items():
        for i, s in enumerate(gs):
            op = s["op"]
            if op in sr.SPLIT_OPS or op == "ABSMAX":
                src = (s["src"], sr.footprint(s)[0])
                assert src[1] > 0 and 0 <= src[0] and src[0] + src[1] <= total, (name, s)
                assert not any(_overlap(src, r) for r in regions if r[1] > 0), (name, s)     # outside all derived regions
            if op in sr.SPLIT_OPS:
                assert s["Qs"] >= 1 and 2 * s["Qd"] >= s["Qs"], (name, s)
            if op == "SPLIT_X":
                assert 0 <= s["arg"] <= s["Qd"], (name, s)
            if op == "SPLIT2H":
                assert s["arg"] >= 1, (name, s)
            if op == "SPLIT2H_GATH":
                E, NT_L = s["arg"], s["n"]
                assert E >= 1 and _round8(E + 1) < 32 * NT_L, (name, s)       # the compact order's c / d column has a place
                ordspan = (s["ord"], 4)
                assert 0 < s["ord"] and s["ord"] + 4 <= total and not any(_overlap(ordspan, r) for r in regions if r[1] > 0), (name, s)
            if op == "REORDER_XQ":
                earlier = [t for t in gs[:i] if t["op"] not in sr.SCALE_OPS and t["dst"] == s["src"]]
                assert len(earlier) == 1 and earlier[0]["op"] == "SPLIT_X", (name, s)
                assert sr.footprint(earlier[0])[1] == sr.footprint(s)[0], (name, s, earlier[0])
                assert earlier[0]["arg"] == 0 and earlier[0]["Qd"] == s["Qd"] and earlier[0]["n"] == s["n"], (name, s, earlier[0])


def _round8(n):
    return (n + 7) // 8 * 8


@pytest.mark.parametrize("name", list(SHAPES))
def test_inference_and_backward_groups(name):
    steps, _, n_infer, _ = table(name)
    groups = _groups(steps)
    assert 0 < n_infer <= len(groups)
    if SHAPES[name].get("use_gatv2", True):
        assert n_infer < len(groups), name                          # the training backward has packs of its own
    # the backward's packs are all plain three-bf16-piece row GEMM / recurrence operands
    assert all(s["op"] == "SPLIT3" for g in groups if g >= n_infer for s in groups[g])


def test_the_shape_list_covers_every_kind_of_step():
    kinds = set()
    for name, kw in SHAPES.items():
        steps, _, _, _ = table(name)
        for gs in _groups(steps).values():
            ncg = [t["n"] for t in gs if t["op"] == "SPLIT2H" and t["arg"] == 3]
            for s in gs:
                op = s["op"]
                kinds.add(op)
                if op in sr.SPLIT_OPS:
                    if s["Qs"] % 2:
                        kinds.add("odd Qs")
                    if 2 * s["Qd"] > s["Qs"] + 1:
                        kinds.add("whole padding chunks")
                    if s["Qs"] % 2 and op != "SPLIT3":
                        kinds.add("odd Qs on fp16 pieces")
                if op == "SPLIT_X":
                    kinds.add("SPLIT_X 0 < qb < Qd" if 0 < s["arg"] < s["Qd"] else "SPLIT_X qb == 0" if s["arg"] == 0 else "SPLIT_X qb == Qd")
                    if ncg and s["n"] == kw["window_size"] * ncg[0] and kw["window_size"] > 1:
                        kinds.add("SPLIT_X outer = W NCG")
                if op == "SPLIT2H":
                    kinds.add("SPLIT2H G = %d" % s["arg"])
    want = set(sr.OPS) | {"odd Qs", "whole padding chunks", "SPLIT_X 0 < qb < Qd", "SPLIT_X qb == 0", "SPLIT_X outer = W NCG",
                          "SPLIT2H G = 3", "SPLIT2H G = 1"}
    assert want <= kinds, sorted(want - kinds)


# ---- split_refs on its own ------------------------------------------------------------------------------------------------------
def _values(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    v = (np.exp2(rng.uniform(lo, hi, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    v[rng.random(n) < 0.01] = 0.0
    return v


def test_three_bf16_pieces_sum_to_the_value_exactly():
    v = _values(1_000_000, -60, 60, 1)
    hi, mid, lo = (sr.bf16_to_f32(p).astype(np.float64) for p in sr.split3(v))
    assert np.array_equal(hi + mid + lo, v.astype(np.float64))
    # RNE, not truncation: a value just above a tie rounds up, a tie goes to the even neighbour
    probe = np.array([0x3F808000, 0x3F808001, 0x3F818000, 0x3F807FFF], dtype=np.uint32).view(np.float32)
    assert list(sr.bf16_rne(probe)) == [0x3F80, 0x3F81, 0x3F82, 0x3F80]


@pytest.mark.parametrize("span", [(-60, 60), (-12, -3)])
def test_two_fp16_pieces_meet_their_contract(span):
    v = _values(1_000_000, span[0], span[1], 2)
    bits = np.abs(v).max().view(np.uint32)
    slot = sr.scale_slot(bits)
    S, inv = slot[1:3].view(np.float32)
    assert slot[0] == bits and slot[3] == 0 and S * inv == 1.0
    sv = (v * S).astype(np.float64)
    assert 2.0 ** 13 <= np.abs(sv).max() < 2.0 ** 14
    hi, lo = (sr.f16_to_f32(p).astype(np.float64) for p in sr.split2h(v * S))
    err = np.abs(sv - hi - lo)
    assert np.all(err <= sr.f16_bound(sv)), float((err / sr.f16_bound(sv)).max())


def test_scale_rule_at_its_edges():
    def S(x):
        return sr.scale_slot(np.float32(x).view(np.uint32))[1:2].view(np.float32)[0]
    assert S(0.125) == 2.0 ** 16 and S(np.nextafter(np.float32(0.125), np.float32(0))) == 2.0 ** 17       # [2^13, 2^14) both ends
    assert S(0.0) == 2.0 ** 14 and S(np.inf) == 2.0 ** 14 and S(3.2e38) == 2.0 ** 14
    assert S(2.0 ** -120) == 2.0 ** 100 and S(2.0 ** 120) == 2.0 ** -100                                  # the clamp


def test_pairing_and_compact_order_of_the_reference():
    # element e of lane l of 16-bit chunk qd: float e & 3 of the lane in source chunk 2 qd + (e >> 2); chunks >= Qs read as zeros
    outer, Qs, Qd, G = 2, 3, 3, 2
    src = np.arange(outer * Qs * G * 256, dtype=np.float32) + 1
    p = sr.pair_chunks(src, outer, Qs, Qd, G)
    a = src.reshape(outer, Qs, G, 64, 4)
    for o, qd, g, lane, e in [(0, 0, 0, 0, 0), (1, 0, 1, 63, 5), (0, 1, 1, 17, 3), (1, 1, 0, 40, 7), (1, 2, 1, 9, 2)]:
        q = 2 * qd + (e >> 2)
        assert p[o, qd, g, lane, e] == (a[o, q, g, lane, e & 3] if q < Qs else 0.0)
    assert not p[:, 1, :, :, 4:].any() and not p[:, 2].any()
    # compact order against the specification of tests/gat_sign_cases.py
    for E, pattern in [(8, "one_pos"), (8, "first7_pos"), (32, "all_pos"), (32, "all_neg"), (2, "alternating"), (110, "alternating")]:
        (colk, P8, PT, npos), (colk2, P2, PT2) = gc.column_order(gc.factors(pattern, E), 0.2)
        ncols = (_round8(E) + 8 + 1 + 31) // 32 * 32
        cols = sr.compact_columns(ncols, E, P8, PT, npos)
        got = [colk[c] if 0 <= c < PT else (-2 if c == PT else -1) for c in cols]      # embedding column behind every compact column
        assert got[:PT2] == colk2 and got[PT2] == -2 and set(got[PT2 + 1:]) <= {-1}, (E, pattern)


@pytest.mark.parametrize("name", ["stacked", "odd_shapes", "gat_v1_embed", "sign_small", "wide_hidden"])
def test_replay_of_a_synthetic_image_meets_the_piece_contracts(name):
    """The replay on an image of random initialisation-sized values under the real table: every pack it writes decodes back to its
    source (split_refs.check_contract decodes along another path: per step, from the stored bits), and a second replay on its own
    output changes nothing."""
    steps, regions, _, total = table(name)
    rng = np.random.default_rng(3)
    img = rng.uniform(-0.2, 0.2, total).astype(np.float32)
    for off, n in regions:
        img[off:off + n] = 0
    for s in steps:
        if s["op"] == "SPLIT2H_GATH":
            E = s["arg"]
            (_, P8, PT, npos), _ = gc.column_order(gc.factors("first7_pos" if E > 7 else "alternating", E), 0.2)
            img.view(np.int32)[s["ord"]:s["ord"] + 4] = [P8, PT, npos, 0]
    out = sr.replay(img, steps)
    sr.check_contract(out, steps, name)
    assert np.array_equal(sr.replay(out, steps).view(np.int32), out.view(np.int32))
    for s in steps:
        if s["op"] == "SCALE_FROM_MAX":
            S = out[s["scale"] + 1]
            assert 2.0 ** 16 <= S <= 2.0 ** 17                      # max |v| just under 0.2 (or under 0.125 in a small pack)
