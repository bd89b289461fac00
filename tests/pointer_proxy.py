"""A proxy around the ctypes functions of the library that holds every device pointer of a call to a byte range (tests/test_host_arena.py
holds its bookkeeping on the CPU, tests/test_gpu_guard_bands_eval.py and _prep.py use it on the GPU).

The Python layer sometimes builds or converts an input itself -- bool labels become uint8, ScoreParts.tensors() builds start / end, a
.contiguous() copies.  Such a buffer lives outside the guard-banded arena of a row, and the row would test nothing.  The proxy uses
the argtypes evaluation._lib() and preparation._lib() declare: for every c_void_p argument except the final one (the stream) the
value must be NULL or lie inside [lo, hi); anything else raises AssertionError naming the function and the argument's position.
Host pointers (POINTER(c_double), POINTER(c_int64)) are not c_void_p and are left alone.  Functions without argtypes, or whose
name does not start with `prefix`, pass through."""
import contextlib
import ctypes


def _address(v):
    if v is None:
        return 0
    if isinstance(v, ctypes.c_void_p):
        return v.value or 0
    return int(v)


class PointerProxy:
    def __init__(self, lib, lo, hi, prefix="mtadgat_"):
        self.__dict__.update(_lib=lib, _lo=int(lo), _hi=int(hi), _prefix=prefix, calls=[], seen=0)

    def _wrap(self, name, fn):
        argtypes = getattr(fn, "argtypes", None)
        if not name.startswith(self._prefix) or not argtypes or not callable(fn):
            return fn
        checked = [i for i, t in enumerate(argtypes[:-1]) if t is ctypes.c_void_p]

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            inside = 0
            for i in checked:
                at = _address(args[i])
                if at:
                    assert self._lo <= at < self._hi, (f"{name}: argument {i} is the device pointer {at:#x}, outside the arena "
                                                       f"[{self._lo:#x}, {self._hi:#x}): the layer built or copied this buffer itself")
                    inside += 1
            self.__dict__["seen"] += inside                       # (not through __setattr__, which writes to the library)
            if checked:
                self.calls.append((name, inside))
            return fn(*args)
        return call

    def __getattr__(self, name):
        return self._wrap(name, getattr(self._lib, name))

    def __setattr__(self, name, value):          # (_lib() marks the library as bound: that mark belongs to the library)
        setattr(self._lib, name, value)


@contextlib.contextmanager
def watching(monkeypatch, modules, lo, hi):
    """Inside: module._lib() of every module returns a PointerProxy over [lo, hi) around the module's library.  Yields the list of
    proxies; on exit every proxy must have seen at least one device pointer in all."""
    proxies = []
    with monkeypatch.context() as m:
        for mod in modules:
            proxy = PointerProxy(mod._lib(), lo, hi)
            proxies.append(proxy)
            m.setattr(mod, "_lib", lambda proxy=proxy: proxy)
        yield proxies
    assert sum(p.seen for p in proxies) > 0, "the call handed the library no device pointer"
