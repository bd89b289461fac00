"""The preparation calls (csrc/mtadgat_prep.hip behind preparation.fit_scaler, SeriesScaler.transform and .inverse) under the four
calls of tests/guard_rows.py, as tests/test_gpu_guard_bands_eval.py holds the evaluation calls: exact buffers in a guard-banded arena
under both patterns and skewed, every device pointer inside the arena (tests/pointer_proxy.py), results equal to the ordinary call's
bit for bit, inputs unchanged.

Sizes: 1, 65, 257 and one row below / above mtadgat_prep_rows_per_block(); d in {1, 3, 64, 65}, contiguous and with ld = d + 3 over
exactly (n - 1) ld + d elements.  The data is tests/test_gpu_prep.py's: gaps (NaN, +-inf) in row 0, in the last row, across a block
boundary, whole blocks, whole columns.  The scaler's record is an input like any other.  Parts and the column list of inverse are
tensors the layer always builds itself: those two are driven through ctypes with the spans and the indices in the arena.  The
in-place transform works on a copy the seam places, since a row's inputs must come back unchanged."""
import numpy as np
import pytest
import torch

import _native
import preparation as prep
from guard_rows import watched_calls
from test_gpu_guard_bands_eval import COLUMN_IDS, COLUMNS, _dev, _layout, refuse_scratch
from test_gpu_prep import _lengths, _planted

pytestmark = pytest.mark.gpu

RB = prep.rows_per_block()
SIZES = sorted({1, 65, 257, RB - 1, RB + 1})


def _record(n, d, device):
    """A scaler fitted on other data of the same shape (an ordinary call: its record is then placed as an input)."""
    return prep.fit_scaler(_dev(_planted(n, d, RB, 100 * n + d + 1), device), gaps="ignore").record


@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_fit_scaler(n, d, ld, gpu_device, monkeypatch):
    x = _dev(_planted(n, d, RB, 100 * n + d), gpu_device)
    for gaps in ("ignore", "zero"):
        watched_calls(monkeypatch, gpu_device, {"x": x}, lambda ins: {"record": prep.fit_scaler(ins["x"], gaps=gaps).record},
                      f"fit_scaler n={n} d={d} ld={ld} gaps={gaps}", layout=_layout("x", x, ld))


@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_transform(n, d, ld, gpu_device, monkeypatch):
    x = _dev(_planted(n, d, RB, 100 * n + d), gpu_device)
    offs = np.concatenate(([0], np.cumsum(_lengths(n, RB)))).astype(np.int64)
    P = len(offs) - 1
    inputs = {"x": x, "record": _record(n, d, gpu_device), "start": _dev(offs[:-1], gpu_device), "end": _dev(offs[1:], gpu_device)}
    layout = _layout("x", x, ld)
    plain = {k: inputs[k] for k in ("x", "record")}
    for fill in ("zero", "hold", None):
        for age in (False, True):
            def call(ins):
                out = prep.SeriesScaler(ins["record"]).transform(ins["x"], fill=fill, return_age=age)
                return dict(zip(("y", "age"), out)) if age else {"y": out}
            watched_calls(monkeypatch, gpu_device, plain, call, f"transform n={n} d={d} ld={ld} fill={fill} age={age}", layout=layout)

    def with_parts(ins):
        lib = prep._lib()
        scratch = prep._scratch(lib.mtadgat_prep_transform_scratch(n, d, 2, 1), gpu_device)
        y = _native._empty((n, d), dtype=torch.float32, device=gpu_device)
        age = _native._empty((n, d), dtype=torch.int32, device=gpu_device)
        with torch.cuda.device(gpu_device):
            rc = lib.mtadgat_prep_transform(ins["x"].data_ptr(), n, d, ins["x"].stride(0), ins["record"].data_ptr(), 2, 1, ins["start"].data_ptr(),
                                            ins["end"].data_ptr(), P, scratch.data_ptr(), scratch.numel() * 8, y.data_ptr(), d, age.data_ptr(),
                                            prep._stream(y))
        assert rc == 0, lib.mtadgat_last_error()
        return {"y": y, "age": age}
    ref, _ = watched_calls(monkeypatch, gpu_device, inputs, with_parts, f"transform n={n} d={d} ld={ld} parts", layout=layout)
    want = prep.SeriesScaler(inputs["record"]).transform(x, fill="hold", clip=True, lengths=np.diff(offs).tolist(), return_age=True)
    assert torch.equal(ref["y"].view(torch.int32), want[0].view(torch.int32)) and torch.equal(ref["age"], want[1])
    if ld == d:
        def in_place(ins):
            buf = _native._empty((n, d), dtype=torch.float32, device=gpu_device)
            buf.copy_(ins["x"])
            prep.SeriesScaler(ins["record"]).transform(buf, fill="hold", out=buf)
            return {"y": buf}
        watched_calls(monkeypatch, gpu_device, plain, in_place, f"transform n={n} d={d} in place")


@pytest.mark.parametrize("d,ld", COLUMNS, ids=COLUMN_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_inverse(n, d, ld, gpu_device, monkeypatch):
    y = _dev(_planted(n, d, RB, 100 * n + d + 2), gpu_device)
    k = min(d, 3)
    inputs = {"y": y, "record": _record(n, d, gpu_device), "dims": torch.arange(d - 1, d - 1 - k, -1, dtype=torch.int32).to(gpu_device)}
    layout = _layout("y", y, ld)
    watched_calls(monkeypatch, gpu_device, {k_: inputs[k_] for k_ in ("y", "record")},
                  lambda ins: {"x": prep.SeriesScaler(ins["record"]).inverse(ins["y"])}, f"inverse n={n} d={d} ld={ld}", layout=layout)

    def with_dims(ins):                                              # the first k columns of y as the scaler's columns dims
        lib = prep._lib()
        x = _native._empty((n, k), dtype=torch.float32, device=gpu_device)
        with torch.cuda.device(gpu_device):
            rc = lib.mtadgat_prep_inverse(ins["y"].data_ptr(), n, k, ins["y"].stride(0), ins["record"].data_ptr(), d, ins["dims"].data_ptr(),
                                          x.data_ptr(), k, prep._stream(x))
        assert rc == 0, lib.mtadgat_last_error()
        return {"x": x}
    ref, _ = watched_calls(monkeypatch, gpu_device, inputs, with_dims, f"inverse n={n} d={d} ld={ld} dims", layout=layout)
    want = prep.SeriesScaler(inputs["record"]).inverse(y[:, :k], dims=list(range(d - 1, d - 1 - k, -1)))
    assert torch.equal(ref["x"].view(torch.int32), want.view(torch.int32))


def _refusal_calls(lib, t, device):
    n, d = 3000, 3
    p = lambda a: a.data_ptr()                                                                                        # noqa: E731
    f32 = torch.float32
    stream = prep._stream(torch.empty(0, device=device))
    return {
        "prep_fit": (8, lib.mtadgat_prep_fit_scratch(n, d),
                     lambda s, b: lib.mtadgat_prep_fit(p(t("x", (n, d), f32, 0.5)), n, d, d, 0, s, b, p(t("record", (d, 6), f32)), stream)),
        "prep_transform": (8, lib.mtadgat_prep_transform_scratch(n, d, 2, 1),
                           lambda s, b: lib.mtadgat_prep_transform(p(t("x", (n, d), f32, 0.5)), n, d, d, p(t("record", (d, 6), f32, 1.0)), 2, 0, None,
                                                                   None, 0, s, b, p(t("y", (n, d), f32)), d, p(t("age", (n, d), torch.int32)),
                                                                   stream)),
    }


@pytest.mark.parametrize("entry", ["prep_fit", "prep_transform"])
def test_short_or_misaligned_scratch_is_refused_before_anything_launches(entry, gpu_device):
    """As tests/test_gpu_guard_bands_eval.py asks of the evaluation calls: 8 bytes short or 4 bytes past an 8-byte boundary gives -5
    and leaves the whole arena as it was."""
    refuse_scratch(prep._lib(), _refusal_calls, entry, gpu_device)
