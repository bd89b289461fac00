"""What tests/test_gpu_guard_bands.py and tests/test_gpu_guard_bands_train.py share: one row of the guard-band table is run as FOUR
calls -- the ordinary call on allocator buffers, then the same call with every buffer carved from an arena (tests/arena.py) under
pattern A, under pattern B, and under pattern A with every data buffer 4, 8 or 12 bytes past a 16-byte boundary.  After each arena
call no guard may have changed and every result must equal the ordinary call's bit for bit (which the route tests gate against
float64: the reference chain is theirs).  A NaN in an arena result is a read of something the call never wrote, or of a neighbour."""
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


def place(ar, inputs, skewed, first=0):
    """The inputs {name: tensor or None} as arena buffers holding their data; skewed: one skew class per buffer, in turn."""
    out = {}
    for k, (name, t) in enumerate(inputs.items()):
        if t is None:
            out[name] = None
            continue
        classes = INPUT_SKEWS[t.element_size()]
        out[name] = ar.take(t.shape, t.dtype, skew=classes[(first + k) % len(classes)] if skewed else 0, fill=t, name=name)
    return out


def four_calls(monkeypatch, device, engines, inputs, call, what, before=None, rules=None, runs=RUNS, on_ordinary=None):
    """call(inputs) -> {name: tensor} on the ordinary buffers, then once per run of `runs` inside an arena.  before(): the row's
    route assertions, made before every call.  on_ordinary(results): called with the ordinary call's results before the arena calls.
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
        assert not t.is_floating_point() or bool(torch.isfinite(t).all()), (what, name, "the ordinary call is not finite")
    if on_ordinary is not None:
        on_ordinary(ref)
    sizes = meter.sizes + [t.numel() * t.element_size() for t in inputs.values() if t is not None]
    names = {}
    for run, pattern, skewed in runs:
        ar = arena.Arena(device, pattern, arena.capacity_for(sizes))
        ins = place(ar, inputs, skewed)
        with ar.patched(monkeypatch, *engines, skew=skewed, rules=rules):
            out = run_call(ins)
        bad = ar.check()
        assert bad == [], (what, run, bad, ar.names())
        # the run was what its name says: workspaces and tapes 16-byte aligned, every other buffer -- inputs, outputs, accumulators --
        # 16-byte aligned in the plain runs and NOT in the skewed one
        for b in ar.buffers:
            off = b.tensor.data_ptr() % 16
            assert (off != 0) == (skewed and not b.scratch), (what, run, b.name, off, "scratch" if b.scratch else "data")
        placed = sum(t is not None for t in ins.values())
        assert any(not b.scratch for b in ar.buffers[placed:]), (what, run, "the call took no data buffer from the seam")
        assert set(out) == set(ref), (what, run)
        for name, t in out.items():
            if not same_bits(t, ref[name]):
                nan = int(torch.isnan(t).sum()) if t.is_floating_point() else 0
                diff = (bits(t) != bits(ref[name])).flatten().nonzero().flatten()
                raise AssertionError(f"{what}: pattern {run}: {name} differs from the ordinary call in {diff.numel()} of {t.numel()} "
                                     f"elements, the first {diff[:6].tolist()}, {nan} NaN; buffers {ar.names()}")
        for name, t in ins.items():                                   # the call leaves its inputs alone
            assert t is None or same_bits(t, inputs[name]), (what, run, name, "an input changed")
        names[run] = ar.names()
        del ar, ins, out                                              # one arena at a time: each holds the call's whole workspace
    return ref, names
