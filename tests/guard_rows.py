"""What tests/test_gpu_guard_bands.py and tests/test_gpu_guard_bands_train.py share: one row of the guard-band table is run as FOUR
calls -- the ordinary call on allocator buffers, then the same call with every buffer carved from an arena (tests/arena.py) under
pattern A, under pattern B, and under pattern A with every data buffer 4, 8 or 12 bytes past a 16-byte boundary.  After each arena
call no guard may have changed and every result must equal the ordinary call's bit for bit (which the route tests gate against
float64: the reference chain is theirs).  A NaN in an arena result is a read of something the call never wrote, or of a neighbour.

tests/test_gpu_guard_bands_eval.py and _prep.py run the evaluation and preparation calls through the same four calls, with what
those calls need on top: inputs that hold NaN and infinities (finite=False: a NaN the ordinary call does not have is still
reported), (n, d) inputs placed with a row stride and a short last row (layout=), a watcher around every arena call (watch=: the
pointer proxy of tests/pointer_proxy.py) and, for the float64 sums that are combined with atomics, a comparison of their own
(compare=)."""
import contextlib

import torch

import arena

RUNS = (("A", arena.PATTERN_A, False), ("B", arena.PATTERN_B, False), ("A skewed", arena.PATTERN_A, True))
INPUT_SKEWS = {4: arena.SKEWS, 8: (8,), 2: (2,), 1: (4,)}       # by element size: bf16 at 2 (the kernels test & 7), int64 / float64 at 8


def bits(t):
    """A tensor's bytes as integers, so that -0.0 differs from 0.0 and a NaN equals itself."""
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def place(ar, inputs, skewed, first=0, layout=None):
    """The inputs {name: tensor or None} as arena buffers holding their data; skewed: one skew class per buffer, in turn.
    layout {name: ld}: that (n, d) input gets the row stride ld and a short last row (Arena.take_rows)."""
    out = {}
    for k, (name, t) in enumerate(inputs.items()):
        if t is None:
            out[name] = None
            continue
        classes = INPUT_SKEWS[t.element_size()]
        skew = classes[(first + k) % len(classes)] if skewed else 0
        if layout and name in layout:
            out[name] = ar.take_rows(t, layout[name], skew=skew, name=name)
        else:
            out[name] = ar.take(t.shape, t.dtype, skew=skew, fill=t, name=name)
    return out


def input_bytes(inputs, layout=None):
    """The byte counts of the inputs as place() lays them out."""
    out = []
    for name, t in inputs.items():
        if t is not None:
            n = ((t.shape[0] - 1) * layout[name] + t.shape[1]) if layout and name in layout else t.numel()
            out.append(n * t.element_size())
    return out


def watched_calls(monkeypatch, device, inputs, call, what, **kw):
    """four_calls for the handle-free calls of evaluation.py and preparation.py: no engine, data that may hold NaN and infinities,
    and every arena call under the pointer proxy (tests/pointer_proxy.py) -- every device pointer handed to the library lies inside
    the arena, and there was at least one."""
    import evaluation
    import pointer_proxy
    import preparation
    kw.setdefault("finite", False)
    return four_calls(monkeypatch, device, [], inputs, call, what,
                      watch=lambda ar: pointer_proxy.watching(monkeypatch, (evaluation, preparation), *ar.span()), **kw)


def four_calls(monkeypatch, device, engines, inputs, call, what, before=None, rules=None, runs=RUNS, on_ordinary=None, finite=True,
               layout=None, watch=None, compare=None, seam=True):
    """call(inputs) -> {name: tensor} on the ordinary buffers, then once per run of `runs` inside an arena.  before(): the row's
    route assertions, made before every call.  on_ordinary(results): called with the ordinary call's results before the arena calls.
    finite=False: the row's data holds NaN / infinities on purpose, so the ordinary results may.  layout: see place().  watch(arena):
    a context manager entered around every arena call.  compare {output name: f(got, ordinary, what)}: that output is held by f
    instead of bit equality.  seam=False: the row places every buffer itself and takes none from the seam.
    Returns (ordinary results, {run: the names of the arena's buffers})."""
    def run_call(ins):
        if before is not None:
            before()
        out = call(ins)
        torch.cuda.synchronize(device)
        return {k: v for k, v in out.items() if v is not None}

    meter = arena.Meter(device)
    with meter.patched(monkeypatch, *engines):
        ref = run_call(inputs)
    for name, t in ref.items():
        assert not finite or not t.is_floating_point() or bool(torch.isfinite(t).all()), (what, name, "the ordinary call is not finite")
    if on_ordinary is not None:
        on_ordinary(ref)
    sizes = meter.sizes + input_bytes(inputs, layout)
    names = {}
    for run, pattern, skewed in runs:
        ar = arena.Arena(device, pattern, arena.capacity_for(sizes))
        ins = place(ar, inputs, skewed, layout=layout)
        with ar.patched(monkeypatch, *engines, skew=skewed, rules=rules), (watch(ar) if watch is not None else contextlib.nullcontext()):
            out = run_call(ins)
        bad = ar.check()
        assert bad == [], (what, run, bad, ar.names())
        # the run was what its name says: workspaces and tapes 16-byte aligned, every other buffer -- inputs, outputs, accumulators --
        # 16-byte aligned in the plain runs and NOT in the skewed one
        for b in ar.buffers:
            off = b.tensor.data_ptr() % 16
            assert (off != 0) == (skewed and not b.scratch), (what, run, b.name, off, "scratch" if b.scratch else "data")
        placed = sum(t is not None for t in ins.values())
        assert not seam or any(not b.scratch for b in ar.buffers[placed:]), (what, run, "the call took no data buffer from the seam")
        assert set(out) == set(ref), (what, run)
        for name, t in out.items():
            if compare and name in compare:
                compare[name](t, ref[name], (what, run, name))
            elif not same_bits(t, ref[name]):
                assert t.shape == ref[name].shape and t.dtype == ref[name].dtype, (what, run, name, t.shape, ref[name].shape, t.dtype)
                # a NaN the ordinary call does not have: a read outside the inputs
                nan = int((torch.isnan(t) & ~torch.isnan(ref[name])).sum()) if t.is_floating_point() else 0
                diff = (bits(t) != bits(ref[name])).flatten().nonzero().flatten()
                raise AssertionError(f"{what}: pattern {run}: {name} differs from the ordinary call in {diff.numel()} of {t.numel()} "
                                     f"elements, the first {diff[:6].tolist()}, {nan} NaN the ordinary call does not have; buffers "
                                     f"{ar.names()}")
        for name, t in ins.items():                                   # the call leaves its inputs alone
            assert t is None or same_bits(t, inputs[name]), (what, run, name, "an input changed")
        names[run] = ar.names()
        del ar, ins, out                                              # one arena at a time: each holds the call's whole workspace
    return ref, names
