"""The guard-band arena (tests/arena.py) on the CPU: its bookkeeping -- offsets, alignment and skew, exact sizes --, that a planted
one-word write on either side of a buffer is reported with the right name, side and offset, that both patterns survive a float32
round trip as bits, and that the seam names, places and restores what the GPU tests rely on.  No GPU needed."""
import pytest
import torch

import arena
from arena import GUARD, PATTERN_A, PATTERN_B, Arena


def _off(a, t):
    return t.data_ptr() - a.mem.data_ptr()


@pytest.mark.parametrize("pattern", [PATTERN_A, PATTERN_B])
def test_offsets_alignment_skew_and_exact_sizes(pattern):
    a = Arena("cpu", pattern, arena.capacity_for([28, 3, 10, 40, 16]))
    assert a.mem.data_ptr() % 16 == 0 and a.mem.numel() % 16 == 0
    t0 = a.take((7,), torch.float32, name="seven")                       # 28 bytes: not a multiple of 16
    t1 = a.take((3,), torch.uint8, name="three")                         # 3 bytes: not a multiple of 4
    t2 = a.take((5,), torch.bfloat16, skew=2, name="five")               # 10 bytes at 2 past a 16-byte boundary
    t3 = a.take((2, 5), torch.float32, skew=12, name="ten", fill=1.5)
    t4 = a.take((2,), torch.int64, align=64, skew=8, name="two", fill=torch.tensor([3, -4]))
    for t, skew, align in ((t0, 0, 16), (t1, 0, 16), (t2, 2, 16), (t3, 12, 16), (t4, 8, 64)):
        assert t.data_ptr() % align == skew
    # exactly the requested bytes, 2 GUARD or more between neighbours, a whole guard at both ends of the arena
    for b, t in zip(a.buffers, (t0, t1, t2, t3, t4)):
        assert (b.start, b.end) == (_off(a, t), _off(a, t) + t.numel() * t.element_size()) and b.guard_from == b.end
    assert [b.end - b.start for b in a.buffers] == [28, 3, 10, 40, 16]
    assert a.buffers[0].start >= GUARD and a.buffers[-1].end + GUARD <= a.mem.numel()
    for lo, hi in zip(a.buffers, a.buffers[1:]):
        assert 2 * GUARD <= hi.start - lo.end < 2 * GUARD + 64
    assert a.names() == ["seven", "three", "five", "ten", "two"]
    # outputs and scratch start out as the pattern, inputs hold their data
    assert torch.equal(t0.view(torch.int32), torch.full((7,), arena.as_int32(pattern), dtype=torch.int32))
    assert torch.equal(t3, torch.full((2, 5), 1.5)) and t4.tolist() == [3, -4]
    assert a.check() == [] and a.check(interiors=True) == []
    t0.fill_(2.0), t1.fill_(9), t2.fill_(1.0)                            # writing every byte of every buffer violates nothing
    assert a.check() == []
    assert [r["name"] for r in a.check(interiors=True)] == ["seven", "three", "five"]


def test_duplicate_names_and_a_full_arena():
    a = Arena("cpu", PATTERN_A, arena.capacity_for([4, 4]))
    a.take(1, name="y"), a.take(1, name="y")
    assert a.names() == ["y", "y#1"]
    with pytest.raises(MemoryError):
        a.take(1, name="z")


@pytest.mark.parametrize("pattern", [PATTERN_A, PATTERN_B])
def test_a_planted_word_is_reported_with_name_side_and_offset(pattern):
    a = Arena("cpu", pattern, arena.capacity_for([28, 12, 3, 2 * GUARD]))
    first = a.take((7,), name="first")
    mid = a.take((3,), skew=4, name="mid")
    odd = a.take((3,), torch.uint8, name="odd")
    words, bytes_ = a.words, a.mem

    def plant(byte, value=0):
        assert byte % 4 == 0
        keep = int(words[byte // 4])
        words[byte // 4] = value
        got = a.check()
        words[byte // 4] = keep
        assert a.check() == []
        return got
    s, e = a.buffer("mid").start, a.buffer("mid").end
    assert plant(e) == [dict(name="mid", side="behind", offset=12, words=1)]                 # the word directly behind the last byte
    assert plant(s - 4) == [dict(name="mid", side="front", offset=-4, words=1)]              # the word directly in front
    assert plant(e + GUARD - 4) == [dict(name="mid", side="behind", offset=12 + GUARD - 4, words=1)]
    assert plant(s - GUARD) == [dict(name="mid", side="front", offset=-GUARD, words=1)]
    assert plant(a.buffer("first").end) == [dict(name="first", side="behind", offset=28, words=1)]
    # further off than a guard from every buffer: unused space, compared as well; the arena's first and last words
    tail = a.buffer("odd").end + GUARD
    assert tail % 4 == 3 and a.mem.numel() - tail > GUARD
    assert plant(tail + 1) == [dict(name="<unused>", side="unused", offset=tail + 1, words=1)]
    assert plant(a.mem.numel() - 4) == [dict(name="<unused>", side="unused", offset=a.mem.numel() - 4, words=1)]
    assert plant(0) == [dict(name="first", side="front", offset=-GUARD, words=1)]
    # a value that differs from the pattern in one bit only
    assert plant(e, arena.as_int32(pattern ^ 1)) == [dict(name="mid", side="behind", offset=12, words=1)]
    # the byte directly behind a buffer of 3 bytes shares its word: a partial word counts as one
    o = a.buffer("odd")
    keep = int(bytes_[o.end])
    bytes_[o.end] = keep ^ 0xFF
    assert a.check() == [dict(name="odd", side="behind", offset=3, words=1)]
    bytes_[o.end] = keep
    # several words on both sides of one buffer, one report per guard, the first offset and the count
    k1, k2, k3 = int(words[s // 4 - 2]), int(words[e // 4 + 5]), int(words[e // 4 + 9])
    words[s // 4 - 2], words[e // 4 + 5], words[e // 4 + 9] = 1, 2, 3
    assert a.check() == [dict(name="mid", side="front", offset=-8, words=1), dict(name="mid", side="behind", offset=12 + 20, words=2)]
    words[s // 4 - 2], words[e // 4 + 5], words[e // 4 + 9] = k1, k2, k3
    assert a.check() == [] and first.numel() == 7 and mid.numel() == 3 and odd.numel() == 3


def test_a_guard_that_begins_early_owns_the_last_elements():
    a = Arena("cpu", PATTERN_B, arena.capacity_for([40, 40]))
    data = torch.arange(10, dtype=torch.float32)
    x = a.take((2, 5), fill=data.view(2, 5), early=1, name="x")
    y = a.take((2, 5), early=2, name="y")
    assert x.shape == (2, 5) and torch.equal(x.view(-1)[:9], data[:9])
    assert int(x.view(torch.int32).view(-1)[9]) == arena.as_int32(PATTERN_B)                 # the last element is guard: the pattern
    assert a.check() == []
    y.view(-1)[7] = 0.0                                                                       # the buffer's own last element
    assert a.check() == []
    y.view(-1)[9] = 0.0
    assert a.check() == [dict(name="y", side="behind", offset=36, words=1)]
    y.view(-1)[8] = 0.0
    assert a.check() == [dict(name="y", side="behind", offset=32, words=2)]


@pytest.mark.parametrize("pattern,nan", [(PATTERN_A, True), (PATTERN_B, False)])
def test_patterns_survive_a_float32_round_trip_as_bits(pattern, nan):
    f = arena.pattern_float(pattern)
    assert bool(torch.isnan(f)) == nan
    if not nan:
        assert -1.5e6 < float(f) < -1.3e6
    a = Arena("cpu", pattern, arena.capacity_for([64]))
    t = a.take((16,), name="t")
    back = t.clone().contiguous().view(torch.int32)                      # read as float32, copied as float32
    assert torch.equal(back, torch.full((16,), arena.as_int32(pattern), dtype=torch.int32))
    u = torch.empty(16)
    u.copy_(t)
    t.copy_(u)                                                           # and written back as float32
    assert a.check(interiors=True) == []
    assert torch.equal((t * 0.0).isnan(), torch.full((16,), nan))        # what 7777.0 cannot do: A times zero is still NaN


class _Engine:
    """What the seam touches of _native.Engine."""
    _ws = _bws = _train_tape = _flat_grads = None

    def _buf(self, name, nbytes, device):
        import _native
        cur = _native._empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        setattr(self, name, cur)
        return cur

    def _workspace(self, device):
        import _native
        ws = _native._empty(9, dtype=torch.float32, device=device)
        return ws

    def forward(self, x):
        import _native
        preds = _native._empty((x.shape[0], 3), dtype=torch.float32, device=x.device)
        hend = _native._empty((x.shape[0], 5), dtype=torch.float32, device=x.device) if x.shape[0] else None
        ws = self._workspace(x.device)
        y = _native._empty_like(x)
        wsse = _native._empty((x.shape[0], 2), dtype=torch.float64, device=x.device)
        return preds, hend, ws, y, wsse, self._buf("_bws", 30, x.device)


def test_the_seam_names_places_and_restores(monkeypatch):
    import _native
    real, real_like = _native._empty, _native._empty_like
    eng = _Engine()
    eng._ws = kept = torch.zeros(4)
    x = torch.rand(7, 2)
    meter = arena.Meter("cpu")
    with meter.patched(monkeypatch, eng):
        assert eng._ws is None
        eng.forward(x)
    assert meter.sizes == [84, 140, 36, 56, 112, 32] and eng._ws is kept and _native._empty is real
    a = Arena("cpu", PATTERN_A, arena.capacity_for(meter.sizes))
    with a.patched(monkeypatch, eng):
        assert eng._ws is None
        out = eng.forward(x)
    assert _native._empty is real and _native._empty_like is real_like and eng._ws is kept and eng._bws is None
    assert a.names() == ["forward.preds", "forward.hend", "_workspace.ws", "forward.y", "forward.wsse", "_bws"]
    assert [b.end - b.start for b in a.buffers] == meter.sizes and all(t.data_ptr() % 16 == 0 for t in out)
    assert out[3].shape == x.shape and out[4].dtype == torch.float64 and bool(out[0].isnan().all())
    # skewed: every data buffer 4, 8 or 12 bytes past a 16-byte boundary in turn (float64: 8), workspace and tape stay aligned
    b = Arena("cpu", PATTERN_B, arena.capacity_for(meter.sizes))
    with b.patched(monkeypatch, eng, skew=True, rules={"forward.y": dict(early=1)}):
        out = eng.forward(x)
    assert [t.data_ptr() % 16 for t in out] == [4, 8, 0, 12, 8, 0]
    assert [bf.scratch for bf in b.buffers] == [False, False, True, False, False, True]
    assert list(b.misaligned().values()) == [4, 8, 0, 12, 8, 0]
    assert b.buffer("forward.y").guard_from == b.buffer("forward.y").end - 4 and b.check() == []
    out[3].fill_(0.0)
    assert b.check() == [dict(name="forward.y", side="behind", offset=52, words=1)]
    # a buffer on another device than the arena's is not the arena's business
    with a.patched(monkeypatch, eng):
        assert _native._empty(3, dtype=torch.float32, device="meta").device.type == "meta"


# ---- the short last row and the pointer proxy (tests/test_gpu_guard_bands_eval.py, _prep.py) ------------------------------------------
@pytest.mark.parametrize("pattern", [PATTERN_A, PATTERN_B])
@pytest.mark.parametrize("n,d,ld,skew", [(1, 3, 6, 0), (5, 3, 6, 4), (4, 1, 4, 12), (3, 65, 68, 8)])
def test_rows_with_a_stride_end_behind_the_last_rows_own_elements(pattern, n, d, ld, skew):
    x = torch.arange(n * d, dtype=torch.float32).reshape(n, d) + 1.0
    a = Arena("cpu", pattern, arena.capacity_for([((n - 1) * ld + d) * 4]))
    t = a.take_rows(x, ld, skew=skew, name="x")
    b = a.buffer("x")
    assert t.shape == (n, d) and t.stride() == (ld, 1) and t.data_ptr() % 16 == skew and t.data_ptr() == a.mem.data_ptr() + b.start
    assert b.end - b.start == ((n - 1) * ld + d) * 4 and b.guard_from == b.end      # the guard starts behind the last row's d-th element
    assert torch.equal(t, x) and a.check() == []
    flat = b.tensor.view(torch.int32)
    gaps = torch.ones(flat.numel(), dtype=torch.bool)
    gaps.as_strided((n, d), (ld, 1)).fill_(False)
    assert int(gaps.sum()) == (n - 1) * (ld - d)
    assert bool((flat[gaps] == arena.as_int32(pattern)).all())                       # the gap columns hold the pattern
    if pattern == PATTERN_A and n > 1:
        assert bool(torch.isnan(b.tensor[gaps]).all())
    a.words[b.end // 4] = 0                                                          # the element a full last row would have had
    assert a.check() == [dict(name="x", side="behind", offset=b.end - b.start, words=1)]


def test_the_pointer_proxy_holds_every_device_pointer_to_the_range():
    import ctypes

    import pointer_proxy

    class Fn:
        def __init__(self, argtypes):
            self.argtypes, self.got = argtypes, []

        def __call__(self, *args):
            self.got.append(args)
            return 0

    class Lib:
        pass
    vp, i64, dp = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)
    lib = Lib()
    lib.mtadgat_eval_thing = Fn([vp, i64, vp, dp, vp])            # in, n, out, a host pointer, the stream
    lib.mtadgat_eval_thing_scratch = Fn([i64])
    lib.mtadgat_last_error = Fn(None)
    lib.other = Fn([vp, vp])
    proxy = pointer_proxy.PointerProxy(lib, 1000, 2000)
    host = (ctypes.c_double * 2)()
    assert proxy.mtadgat_eval_thing(1000, 7, vp(1999), host, vp(5)) == 0      # both ends of the range; the stream is not a buffer
    assert proxy.mtadgat_eval_thing(None, 7, 0, host, None) == 0              # NULL is allowed
    assert proxy.mtadgat_eval_thing(vp(None), 7, 1500, host, None) == 0
    assert proxy.seen == 3 and proxy.calls == [("mtadgat_eval_thing", 2), ("mtadgat_eval_thing", 0), ("mtadgat_eval_thing", 1)]
    for bad in (999, 2000, vp(123456)):
        with pytest.raises(AssertionError, match="argument 2 .* outside the arena"):
            proxy.mtadgat_eval_thing(1000, 7, bad, host, None)
    with pytest.raises(AssertionError, match="argument 0"):
        proxy.mtadgat_eval_thing(2000, 7, 1000, host, None)
    assert len(lib.mtadgat_eval_thing.got) == 3                               # a refused call never reaches the library
    with pytest.raises(AssertionError):
        proxy.mtadgat_eval_thing(1000, 7, 1000, host)                         # an argument short
    assert proxy.mtadgat_eval_thing_scratch(5) == 0 and proxy.mtadgat_last_error() == 0 and proxy.other(1, 2) == 0
    proxy._bound = True                                                        # marks land on the library itself
    assert lib._bound is True


def test_watching_replaces_and_restores_the_loaders(monkeypatch):
    import types

    import pointer_proxy
    lib = types.SimpleNamespace(mtadgat_x=lambda *a: 0)
    lib.mtadgat_x.__dict__["argtypes"] = None
    mod = types.SimpleNamespace(_lib=lambda: lib)
    loader = mod._lib
    with pytest.raises(AssertionError, match="no device pointer"):
        with pointer_proxy.watching(monkeypatch, [mod], 0, 10) as proxies:
            assert mod._lib() is proxies[0] and mod._lib().mtadgat_x() == 0
    assert mod._lib is loader


def test_the_seam_names_the_evaluation_buffers(monkeypatch):
    """The scratch helpers and the SPOT state keep their alignment in the skewed run; every other buffer of evaluation.py and
    preparation.py is a data buffer.  (The names are what Arena._empty derives from the caller's line.)"""
    import _native
    import evaluation
    import preparation
    a = Arena("cpu", PATTERN_A, arena.capacity_for([64] * 6))
    with a.patched(monkeypatch, skew=True):
        s0 = evaluation._scratch(20, "cpu")
        s1 = preparation._scratch(0, "cpu")
        scratch = _native._empty(4, dtype=torch.float64, device="cpu")
        order = _native._empty(4, dtype=torch.int64, device="cpu")
        flags = _native._empty(5, dtype=torch.uint8, device="cpu")
    assert a.names() == ["_scratch", "_scratch#1", "test_the_seam_names_the_evaluation_buffers.scratch",
                         "test_the_seam_names_the_evaluation_buffers.order", "test_the_seam_names_the_evaluation_buffers.flags"]
    assert s0.numel() == 3 and s1.numel() == 1
    assert [b.scratch for b in a.buffers] == [True, True, False, False, False]
    assert s0.data_ptr() % 16 == 0 and s1.data_ptr() % 16 == 0
    assert scratch.data_ptr() % 16 == 8 and order.data_ptr() % 16 == 8 and flags.data_ptr() % 16 != 0
