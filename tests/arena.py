"""Guard-banded device memory for the model-path calls (tests/test_host_arena.py holds the bookkeeping on the CPU,
tests/test_gpu_guard_bands*.py use it on the GPU).

The library is handed raw pointers and the byte counts it reports itself; no sanitizer runs on the GPU, and the caching allocator
hides an overrun: its blocks are 512-byte aligned, rounded up and surrounded by other live tensors.  An Arena owns ONE byte tensor
filled with a 32-bit pattern and carves typed tensors out of it:

  * a buffer holds exactly the requested bytes -- no rounding up --, its first byte `align`-aligned plus `skew` bytes;
  * in front of it and directly behind its last byte lies a guard of GUARD = 256 KiB of the pattern (a 256-row workgroup tile of
    1 KiB rows: more than one workgroup's store footprint at the shapes of the tests).  A stray write FURTHER off than 256 KiB from
    every buffer lands in unused arena space, which is patterned and compared as well, or outside the arena, where it is not seen;
  * scratch and outputs start out as the pattern (fill=None), inputs and accumulators get their data (fill=tensor or number);
  * check() compares every guard and all unused space with the pattern as int32 on the device and reports, per violated guard, the
    buffer's name, the side, the first changed byte's offset from the buffer's first byte and the number of changed words.

Two patterns: A = 0x7FC5A5A5, a quiet NaN -- a read of anything the call did not write, or of a neighbour, poisons the result even
through a multiplication by zero --, and B = 0xC9A5A5A5, about -1.4e6: finite and huge against inputs in [0, 1), for the paths a NaN
would be filtered from.

The seam: every buffer the Python layer hands the library comes from _native._empty / _native._empty_like (and _hipgrad's gradient
buffer from _empty + zero_).  Arena.patched(monkeypatch, engine) points both at the arena, drops the engine's cached workspaces so
that every call gets buffers of exactly the reported size, and puts everything back on exit."""
import contextlib
import linecache
import re
import sys

import torch

GUARD = 256 * 1024
PATTERN_A = 0x7FC5A5A5                      # a quiet NaN
PATTERN_B = 0xC9A5A5A5                      # about -1.4e6
SKEWS = (4, 8, 12)                          # the three classes of "4-byte but not 16-byte aligned"
# The buffers the ABI wants 16-byte aligned -- workspaces and the tape --, by the names the seam gives them ("<Engine method>.<variable>";
# Engine._buf's by its attribute).  Everything else is a data buffer and is skewed by patched(skew=True).  A scratch buffer that is
# renamed in _native.py falls out of this list, is skewed, and the library refuses the call: the list cannot go stale silently.
SCRATCH_BUFFERS = ("_workspace.ws", "_bws", "forward_train.tape", "_attention_ws", "score_attribution.ws", "series_losses.ws",
                   # evaluation.py / preparation.py: the _scratch helpers (8 or 16 bytes per declaration in include/mtadgat.h) and the
                   # SPOT state (16 bytes).  (The scratch of the calls that take no byte count is float64 and asks for 8 bytes only:
                   # a data buffer, skewed by 8.)
                   "_scratch", "spot_calibrate.buf", "expand.buf", "spot_state.buf")  # (spot_state: the tests' copy of a calibrated state)
ENGINE_CACHES = ("_ws", "_bws", "_train_tape", "_flat_grads")


def _round_up(v, m):
    return (v + m - 1) // m * m


def as_int32(pattern):
    return pattern - (1 << 32) if pattern >= (1 << 31) else pattern


def pattern_float(pattern):
    """The pattern as the float32 whose bits it is."""
    return torch.tensor([as_int32(pattern)], dtype=torch.int32).view(torch.float32)[0]


def nbytes_of(shape, dtype):
    n = 1
    for s in shape:
        n *= int(s)
    return n * torch.empty(0, dtype=dtype).element_size()


def rows_fill(x, ld, pattern):
    """The flat ((n - 1) * ld + d,) tensor that holds the rows of x (n, d) at stride ld, the pattern's bits in the gaps (4-byte
    elements)."""
    n, d = x.shape
    assert x.element_size() == 4
    flat = torch.full(((n - 1) * ld + d,), as_int32(pattern), dtype=torch.int32, device=x.device)
    flat.as_strided((n, d), (ld, 1)).copy_(x.contiguous().view(torch.int32))
    return flat.view(x.dtype)


def capacity_for(sizes):
    """Bytes an arena needs for buffers of the given byte counts, whatever their alignment and skew."""
    return sum(_round_up(s, 16) + 2 * GUARD + 64 for s in sizes) + GUARD


def _shape_of(shape):
    if len(shape) == 1 and not isinstance(shape[0], int):
        return tuple(int(s) for s in shape[0])
    return tuple(int(s) for s in shape)


class Buffer:
    def __init__(self, name, start, end, guard_from, patterned, tensor, scratch=False):
        self.name, self.start, self.end, self.guard_from, self.patterned, self.tensor = name, start, end, guard_from, patterned, tensor
        self.scratch = scratch


class Meter:
    """Records the byte counts of the buffers a call asks the seam for (the call itself runs on allocator memory): what an arena
    for the same call has to hold."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.sizes = []

    @contextlib.contextmanager
    def patched(self, monkeypatch, *engines):
        import _native
        real = _native._empty

        def empty(*shape, **kw):
            t = real(*shape, **kw)
            if t.device.type == self.device.type:
                self.sizes.append(t.numel() * t.element_size())
            return t
        with _seam(monkeypatch, empty, lambda x: empty(x.shape, dtype=x.dtype, device=x.device), engines):
            yield self


@contextlib.contextmanager
def _seam(monkeypatch, empty, empty_like, engines):
    import _native
    kept = [{k: getattr(e, k, None) for k in ENGINE_CACHES} for e in engines]
    real_buf, real_train = _native.Engine._buf, _native.Engine.forward_train

    def buf(self, name, nbytes, device, fresh=True):
        if fresh:                                                  # (not fresh: backward_input reads what backward left there)
            setattr(self, name, None)
        return real_buf(self, name, nbytes, device, fresh)

    def forward_train(self, x, p, seed, window0=0, tape=None):     # a chunked step re-uses the first chunk's tape: here every chunk
        return real_train(self, x, p, seed, window0, None)         # gets one of exactly mtadgat_tape_bytes
    with monkeypatch.context() as m:
        m.setattr(_native, "_empty", empty)
        m.setattr(_native, "_empty_like", empty_like)
        m.setattr(_native.Engine, "_buf", buf)
        m.setattr(_native.Engine, "forward_train", forward_train)
        for e in engines:
            for k in ENGINE_CACHES:
                setattr(e, k, None)
        try:
            yield
        finally:
            for e, caches in zip(engines, kept):
                for k, v in caches.items():
                    setattr(e, k, v)


class Arena:
    def __init__(self, device, pattern, capacity):
        self.device, self.pattern = torch.device(device), int(pattern)
        capacity = _round_up(int(capacity), 16)
        raw = torch.empty(capacity + 16, dtype=torch.uint8, device=self.device)
        lead = -raw.data_ptr() % 16
        self.mem = raw[lead:lead + capacity]                       # first byte 16-byte aligned, a whole number of words
        self.words = self.mem.view(torch.int32)
        self.words.fill_(as_int32(self.pattern))
        self.pattern_bytes = torch.tensor([as_int32(self.pattern)], dtype=torch.int32).view(torch.uint8).to(self.device)
        self.buffers = []
        self.cursor = 0
        self.skew_classes = None                                   # patched(skew=True): SKEWS, walked by the seam's data buffers
        self.rules = {}
        self._n_skewed = 0

    # ---- carving ---------------------------------------------------------------------------------------------------------------
    def take(self, shape, dtype=torch.float32, align=16, skew=0, fill=None, name=None, early=0, scratch=False):
        """A tensor of `shape` / `dtype` over exactly its own bytes of the arena: first byte `align`-aligned + `skew` bytes, GUARD
        bytes of pattern on both sides.  fill: None -- the pattern stays (scratch, outputs) --, a tensor of that shape or a number
        (inputs, accumulators).  early: the trailing guard begins that many ELEMENTS before the tensor's end (the self-tests of the
        harness: the tensor still has its full shape, its last elements are guard, hold the pattern and are compared by check())."""
        shape = _shape_of((shape,)) if not isinstance(shape, int) else (int(shape),)
        item = torch.empty(0, dtype=dtype).element_size()
        nbytes = nbytes_of(shape, dtype)
        assert align >= 1 and skew >= 0 and skew % item == 0, (align, skew, dtype)
        base = self.mem.data_ptr()
        start = _round_up(base + self.cursor + GUARD, align) - base + skew
        end = start + nbytes
        if end + GUARD > self.mem.numel():
            raise MemoryError(f"arena of {self.mem.numel()} bytes is full: {name or shape} needs [{start}, {end + GUARD})")
        t = self.mem[start:end].view(dtype).view(shape)
        assert t.data_ptr() == base + start
        live = t.numel() - early
        assert 0 <= live <= t.numel()
        if fill is not None:
            flat = t.view(-1)[:live]
            if isinstance(fill, torch.Tensor):
                assert tuple(fill.shape) == shape and fill.dtype == dtype, (name, tuple(fill.shape), shape, fill.dtype)
                flat.copy_(fill.reshape(-1)[:live])
            else:
                flat.fill_(fill)
        name = name or f"buffer{len(self.buffers)}"
        taken = {b.name for b in self.buffers}
        if name in taken:
            k = 1
            while f"{name}#{k}" in taken:
                k += 1
            name = f"{name}#{k}"
        self.buffers.append(Buffer(name, start, end, end - early * item, fill is None, t, scratch))
        self.cursor = end + GUARD
        return t

    def take_rows(self, x, ld, skew=0, name=None):
        """The (n, d) tensor x as rows of stride ld >= d over exactly (n - 1) * ld + d elements: the last row is short, the guard
        begins right behind its d-th element, and the ld - d gap elements behind every other row hold the pattern."""
        n, d = x.shape
        assert x.ndim == 2 and ld >= d and n >= 1
        flat = self.take(((n - 1) * ld + d,), x.dtype, skew=skew, fill=rows_fill(x, ld, self.pattern), name=name)
        return flat.as_strided((n, d), (ld, 1))

    def span(self):
        """[first byte, one past the last byte) of the arena's memory, guards and unused space included."""
        return self.mem.data_ptr(), self.mem.data_ptr() + self.mem.numel()

    def buffer(self, name):
        return next(b for b in self.buffers if b.name == name)

    def names(self):
        return [b.name for b in self.buffers]

    def misaligned(self):
        """{buffer name: its first byte's address modulo 16}."""
        return {b.name: b.tensor.data_ptr() % 16 for b in self.buffers}

    # ---- checking --------------------------------------------------------------------------------------------------------------
    def _segments(self):
        """(name, side, lo, hi, origin) over everything that is not a buffer's own bytes, in address order."""
        out, at = [], 0
        bufs = sorted(self.buffers, key=lambda b: b.start)
        for b in bufs:                                                 # (take() leaves at least 2 GUARD between two buffers)
            front, behind = b.start - GUARD, b.guard_from + GUARD
            assert at <= front and behind <= self.mem.numel()
            if front > at:
                out.append(("<unused>", "unused", at, front, 0))
            out.append((b.name, "front", front, b.start, b.start))
            out.append((b.name, "behind", b.guard_from, behind, b.start))
            at = behind
        if at < self.mem.numel():
            out.append(("<unused>", "unused", at, self.mem.numel(), 0))
        return out

    def _changed(self, lo, hi):
        """bool per word of [lo, hi) (a partial word at either end counts as one), the byte offset of each word's first byte."""
        parts, offs = [], []
        lo4, hi4 = min(_round_up(lo, 4), hi), max(hi // 4 * 4, lo)
        if lo4 > hi4:                                                  # inside one word
            lo4 = hi4 = hi
        for a, b in ((lo, lo4), (hi4, hi)):
            if b > a:
                want = self.pattern_bytes[a % 4:a % 4 + (b - a)]
                parts.append((self.mem[a:b] != want).any().reshape(1))
                offs.append(torch.tensor([a], device=self.device))
        if hi4 > lo4:
            parts.append(self.words[lo4 // 4:hi4 // 4] != as_int32(self.pattern))
            offs.append(None)
        return parts, offs, lo4

    def check(self, interiors=False):
        """[] when every guard and all unused space still hold the pattern; else one dict per violated guard: name, side ("front" /
        "behind" / "unused"), offset -- the first changed byte, counted from the buffer's first byte (negative in front of it; from
        the arena's first byte for unused space) -- and words, the number of changed 32-bit words.  interiors=True: the buffers
        that were handed out as pattern (fill=None) are compared too, side "interior" (a refused call launches nothing)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        segs = self._segments()
        if interiors:
            segs += [(b.name, "interior", b.start, b.guard_from, b.start) for b in self.buffers if b.patterned and b.guard_from > b.start]
        found = [self._changed(lo, hi) for _, _, lo, hi, _ in segs]
        counts = torch.stack([sum(p.sum() for p in parts) if parts else torch.zeros((), dtype=torch.int64, device=self.device)
                              for parts, _, _ in found]).tolist()
        report = []
        for (name, side, lo, hi, origin), (parts, offs, lo4), n in zip(segs, found, counts):
            if not n:
                continue
            first = None
            for p, o in zip(parts, offs):
                idx = p.nonzero().flatten()
                if idx.numel():
                    at = int(o[0]) if o is not None else lo4 + 4 * int(idx[0])
                    first = at if first is None else min(first, at)
            report.append(dict(name=name, side=side, offset=first - origin, words=int(n)))
        return report

    # ---- the seam --------------------------------------------------------------------------------------------------------------
    def _skew_for(self, name, dtype, scratch):
        if self.skew_classes is None or scratch:
            return 0
        item = torch.empty(0, dtype=dtype).element_size()
        classes = [s for s in self.skew_classes if s % item == 0]
        if not classes:
            return 0
        self._n_skewed += 1
        return classes[(self._n_skewed - 1) % len(classes)]

    def _empty(self, *shape, _depth=1, **kw):
        """_native._empty's stand-in: the caller's function and the name it assigns to name the buffer."""
        device = torch.device(kw.get("device", "cpu"))
        if device.type != self.device.type:
            return torch.empty(*shape, **kw)
        frame = sys._getframe(_depth)
        func = frame.f_code.co_name
        line = linecache.getline(frame.f_code.co_filename, frame.f_lineno)
        m = re.match(r"\s*(\w+)\s*=\s*(?:_native\.)?_empty", line)
        lhs = m.group(1) if m else None
        if func == "_buf":
            name = str(frame.f_locals.get("name", "_buf"))
        else:
            name = f"{func}.{lhs}" if lhs else func
        scratch = name in SCRATCH_BUFFERS
        dtype = kw.get("dtype", torch.float32)
        rule = self.rules.get(name, {})
        skew = rule.get("skew", self._skew_for(name, dtype, scratch))
        return self.take(_shape_of(shape), dtype, skew=skew, name=name, early=rule.get("early", 0), scratch=scratch)

    def _empty_like(self, x):
        return self._empty(x.shape, _depth=2, dtype=x.dtype, device=x.device)

    @contextlib.contextmanager
    def patched(self, monkeypatch, *engines, skew=False, rules=None):
        """Inside: _native._empty / _empty_like carve from this arena and the engines' cached workspaces, tape and gradient buffer
        are dropped -- and a chunked training step gets a fresh tape and backward workspace per chunk instead of re-using the first
        chunk's larger ones --, so every buffer of a call is exactly as large as the library reports.  skew=True: every buffer that is not
        workspace or tape starts 4, 8 or 12 bytes past a 16-byte boundary, one class per buffer, in turn.  rules: {buffer name:
        dict(skew=bytes, early=elements)} for single buffers.  On exit the seam and the caches are what they were."""
        self.skew_classes = SKEWS if skew else None
        self.rules = dict(rules or {})
        try:
            with _seam(monkeypatch, self._empty, self._empty_like, engines):
                yield self
        finally:
            self.skew_classes, self.rules = None, {}
