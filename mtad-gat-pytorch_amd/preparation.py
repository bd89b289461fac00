"""Preparing raw telemetry: a per-column min-max scaler fitted and applied on the device, with the sensor gaps filled on the way.

The first step of the reference's pipeline -- utils.normalize_data: NaNs replaced, a MinMaxScaler fitted on the training series and
applied to train and test -- for series that already live on the GPU, and the same arithmetic as per-stream state for live rows:

    scaler = fit_scaler(train_raw, gaps="zero")                        # the reference's fit; gaps="ignore" is sklearn's own
    train = scaler.transform(train_raw, fill="zero")                   # MinMaxScaler's float32 bits
    test = scaler.transform(test_raw, fill="hold", lengths=[...])      # a gap repeats the last valid sample of its part
    torch.save(scaler.state_dict(), "scaler.pt")                       # beside the checkpoint
    prep = StreamPreparer(scaler, n_streams=256, fill="hold")          # or StreamScorer(..., prepare=(scaler, "hold"))
    rows = prep.push(raw_rows)

A gap is a sample that is not finite (NaN, +inf, -inf).  Per column the scaler holds lo, hi, scale = 1 / (hi - lo) (1 where hi - lo
< 10 eps32), offset = 0 - lo scale -- MinMaxScaler's scale_ and min_ bit for bit in float32 --, the mean of the valid samples and
their number, in one small device record the host reads only in read() / state_dict().  transform computes
fl(fl(v scale) + offset) with v the sample or its fill:
  fill="zero"   the raw value 0.0 (the reference's nan_to_num)
  fill="hold"   the raw value of the last valid sample of the column within the row's part (causal: what a live stream can do), the
                column's mean where the part has none yet
  fill=None     NaN
Three departures from the reference: +-inf is a gap, where nan_to_num makes it +-3.4e38 and the scaler then flattens the column;
the hold fill is ours; a column without any valid sample scales as a constant column (lo = hi = mean = 0, scale 1).

GPU tensors run the HIP kernels of csrc/mtadgat_prep.hip (include/mtadgat.h: mtadgat_prep_*); CPU tensors take a torch-op route
here for fit_scaler, transform and inverse (a scaler can be fitted where the data is loaded) whose bits are those of
tests/prep_refs.py, the specification.  StreamPreparer is GPU only.
"""
import math

import torch

import _native

_FILLS = {None: 0, "none": 0, "zero": 1, "hold": 2}
_GAPS = {"ignore": 0, "zero": 1}
_FIELDS = ("lo", "hi", "scale", "offset", "mean")
_TINY_RANGE = 10.0 * 1.1920929e-07          # sklearn's _handle_zeros_in_scale: 10 * eps of float32


_lib = _native.load_library           # (tests/pointer_proxy.py replaces it: every call below fetches the library through it)
_stream = _native._stream


def rows_per_block():
    """Rows per block of the fit's reductions and the fill's scan (mtadgat_prep_rows_per_block; tests place their edge cases by it)."""
    return int(_lib().mtadgat_prep_rows_per_block())


def _fail(rc, what):
    _native._fail(_lib(), rc, what)


def _scratch(nbytes, device):              # (never empty: at least one 8-byte word)
    return _native._scratch(nbytes, device, least=8)


def _rows2d(t, name):
    """A float32 (n, d) tensor whose rows are contiguous (a column slice keeps its row stride: no copy); 1-D is one column."""
    return _native._rows2d(t, name, max_columns=2048)


def _fill_code(fill):
    if fill not in _FILLS:
        raise ValueError(f"fill must be 'zero', 'hold' or None, got {fill!r}")
    return _FILLS[fill]


def _part_offsets(lengths, n):
    """Row offsets (P + 1 python ints) of parts of `lengths` rows each, which must add up to n."""
    ls = [int(v) for v in lengths]
    if len(ls) < 1 or any(v < 0 for v in ls) or any(int(v) != v for v in lengths):
        raise ValueError(f"lengths must be a non-empty sequence of integers >= 0, got {lengths!r}")
    if sum(ls) != n:
        raise ValueError(f"lengths add up to {sum(ls)} rows, the series has {n}")
    offs = [0]
    for v in ls:
        offs.append(offs[-1] + v)
    return offs


# ---- the torch-op route of CPU tensors ---------------------------------------------------------------------------------------
def _valid(x):
    return torch.isfinite(x)


def _fit_cpu(x, gaps):
    ok = _valid(x)
    if gaps == "zero":
        x = torch.where(ok, x, torch.zeros((), dtype=torch.float32))
        ok = torch.ones_like(ok)
    n_valid = ok.sum(dim=0).to(torch.int32)
    some = n_valid > 0
    zero = torch.zeros((), dtype=torch.float32)
    lo = torch.where(some, torch.where(ok, x, torch.full((), math.inf)).amin(dim=0), zero) + 0.0
    hi = torch.where(some, torch.where(ok, x, torch.full((), -math.inf)).amax(dim=0), zero) + 0.0
    rng = hi - lo
    scale = 1.0 / torch.where(rng < torch.tensor(_TINY_RANGE, dtype=torch.float32), torch.ones((), dtype=torch.float32), rng)
    offset = 0.0 - lo * scale
    # the mean: the exactly rounded float64 sum of the valid samples, divided once, rounded once to float32
    cols = torch.where(ok, x, zero).double().t().tolist()
    mean = torch.tensor([math.fsum(c) / k if k else 0.0 for c, k in zip(cols, n_valid.tolist())], dtype=torch.float64).float()
    rec = torch.empty((x.shape[1], 6), dtype=torch.float32)
    for j, v in enumerate((lo, hi, scale, offset, mean)):
        rec[:, j] = v
    rec.view(torch.int32)[:, 5] = n_valid
    return rec


def _transform_cpu(x, rec, fill, clip, offsets, want_age):
    n, d = x.shape
    ok = _valid(x)
    scale, offset, mean = rec[:, 2], rec[:, 3], rec[:, 4]
    age = None
    if fill == 2 or want_age:
        row = torch.arange(n, dtype=torch.int64)[:, None]
        part_start = torch.zeros(n, dtype=torch.int64)
        for s, e in zip(offsets[:-1], offsets[1:]):
            part_start[s:e] = s
        part_start = part_start[:, None]
        last = torch.where(ok, row, torch.full((), -1, dtype=torch.int64)).cummax(dim=0).values       # the last valid row at or before
        has = last >= part_start
        age = torch.where(has, row - last, row - part_start + 1).to(torch.int32)
        held = torch.where(has, torch.gather(x, 0, last.clamp(min=0)), mean[None, :].expand(n, d))
    if fill == 2:
        v = torch.where(ok, x, held)
    elif fill == 1:
        v = torch.where(ok, x, torch.zeros((), dtype=torch.float32))
    else:
        v = torch.where(ok, x, torch.full((), math.nan))
    y = v * scale
    y = y + offset
    if clip:
        y = torch.where(y < 0, torch.zeros((), dtype=torch.float32), torch.where(y > 1, torch.ones((), dtype=torch.float32), y))
    return y, (age if want_age else None)


# ---- the scaler ----------------------------------------------------------------------------------------------------------------
class SeriesScaler:
    """The fitted per-column scaler (fit_scaler): `record` is a (d, 6) float32 tensor on `device` -- lo, hi, scale, offset, mean and
    the bits of the int32 n_valid per column, the device record the kernels read (mtadgat_prep_column).  `gaps`: how it was fitted."""

    def __init__(self, record, gaps="ignore"):
        if not isinstance(record, torch.Tensor) or record.dtype != torch.float32 or record.ndim != 2 or record.shape[1] != 6:
            raise ValueError("record must be a (d, 6) float32 tensor")
        self.record = record.contiguous()
        self.gaps = gaps

    @property
    def device(self):
        return self.record.device

    @property
    def n_columns(self):
        return self.record.shape[0]

    def read(self):
        """The record on the host: a dict of (d,) numpy arrays lo, hi, scale, offset, mean (float32) and n_valid (int32)."""
        rec = self.record.cpu()
        out = {name: rec[:, j].numpy().copy() for j, name in enumerate(_FIELDS)}
        out["n_valid"] = rec.view(torch.int32)[:, 5].numpy().copy()
        return out

    def state_dict(self):
        """What to save beside a checkpoint (torch.save): the record as a CPU tensor and how it was fitted."""
        return {"record": self.record.cpu().clone(), "gaps": self.gaps}

    @classmethod
    def from_state(cls, state, device=None):
        scaler = cls(state["record"].clone(), state.get("gaps", "ignore"))
        return scaler if device is None else scaler.to(device)

    def to(self, device):
        device = torch.device(device)
        return self if device == self.record.device else SeriesScaler(self.record.to(device), self.gaps)

    def _same_device(self, t, name):
        if t.device != self.record.device:
            raise RuntimeError(f"{name} is on '{t.device}', the scaler on '{self.record.device}' (SeriesScaler.to)")

    def transform(self, series, fill="zero", clip=False, lengths=None, out=None, return_age=False):
        """The (n, d) series scaled, its gaps filled by `fill` ("zero", "hold" or None, see the module's text); clip: to [0, 1].
        lengths: the row counts of the parts the series is a concatenation of (they must add up to n; as score_parts takes them) --
        a hold fill and the age never cross a seam; None: one part.  out: a float32 (n, d) tensor on the same device that receives
        the result, possibly `series` itself (in place).  return_age: also the (n, d) int32 age -- 0 at a valid sample, k at the
        k-th consecutive gap row since the last valid one, counted from the part's first row where the part has none yet.
        Asynchronous on the GPU, bitwise reproducible."""
        code = _fill_code(fill)
        one_d = isinstance(series, torch.Tensor) and series.ndim == 1
        x = _rows2d(series, "series")
        self._same_device(x, "series")
        n, d = x.shape
        if d != self.n_columns:
            raise ValueError(f"the series has {d} columns, the scaler {self.n_columns}")
        offsets = _part_offsets([n] if lengths is None else lengths, n)
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != x.device or out.numel() != n * d:
                raise ValueError(f"out must be a float32 tensor of the series' shape on '{x.device}'")
            o = out.reshape(n, d) if out.ndim == 1 else out
            if tuple(o.shape) != (n, d) or o.stride(1) != 1 or (n > 1 and o.stride(0) < d):
                raise ValueError("out must have the series' shape and contiguous rows")
        if x.device.type != "cuda":
            y, age = _transform_cpu(x, self.record, code, clip, offsets, return_age)
            if out is not None:
                o.copy_(y)
                y = o
        else:
            y, age = self._transform_gpu(x, code, clip, offsets, None if out is None else o, return_age)
        if out is not None:
            y = out
        elif one_d:
            y = y.reshape(-1)
        if return_age:
            return y, (age.reshape(-1) if one_d else age)
        return y

    def _transform_gpu(self, x, code, clip, offsets, o, want_age):
        lib = _lib()
        n, d = x.shape
        if o is None:
            o = _native._empty((n, d), dtype=torch.float32, device=x.device)
        ld_out = o.stride(0) if n > 1 else d
        age = _native._empty((n, d), dtype=torch.int32, device=x.device) if want_age else None
        start = end = None
        count = 0
        if len(offsets) > 2:
            bounds = torch.tensor(offsets, dtype=torch.int64).to(x.device)
            start, end, count = bounds[:-1].contiguous(), bounds[1:].contiguous(), len(offsets) - 1
        need = lib.mtadgat_prep_transform_scratch(n, d, code, 1 if want_age else 0)
        scratch = _scratch(need, x.device) if need else None
        with torch.cuda.device(x.device):
            rc = lib.mtadgat_prep_transform(x.data_ptr(), n, d, x.stride(0), self.record.data_ptr(), code, 1 if clip else 0,
                                            start.data_ptr() if count else None, end.data_ptr() if count else None, count,
                                            scratch.data_ptr() if need else None, scratch.numel() * 8 if need else 0, o.data_ptr(), ld_out,
                                            age.data_ptr() if want_age else None, _stream(x))
        if rc != 0:
            _fail(rc, "prep_transform")
        return o, age

    def inverse(self, values, dims=None):
        """Scaled values back in raw units: fl(fl(y - offset) / scale).  values (n, k) (or (k,)-wide rows of predictions or
        reconstructions); dims: the scaler column of each of the k columns (the model's target_dims), None: columns 0 .. k - 1."""
        one_d = isinstance(values, torch.Tensor) and values.ndim == 1
        y = _rows2d(values, "values")
        self._same_device(y, "values")
        n, k = y.shape
        if dims is None:
            if k > self.n_columns:
                raise ValueError(f"values have {k} columns, the scaler {self.n_columns}: pass dims")
            cols = None
        else:
            cols = [int(dims)] if isinstance(dims, int) else [int(c) for c in dims]
            if len(cols) != k:
                raise ValueError(f"dims select {len(cols)} columns, values have {k}")
            if any(c < 0 or c >= self.n_columns for c in cols):
                raise ValueError(f"dims must lie in [0, {self.n_columns})")
        if y.device.type != "cuda":
            rec = self.record if cols is None else self.record[cols]
            x = (y - rec[:k, 3]) / rec[:k, 2]
        else:
            lib = _lib()
            x = _native._empty((n, k), dtype=torch.float32, device=y.device)
            dims_dev = None if cols is None else torch.tensor(cols, dtype=torch.int32).to(y.device)
            with torch.cuda.device(y.device):
                rc = lib.mtadgat_prep_inverse(y.data_ptr(), n, k, y.stride(0), self.record.data_ptr(), self.n_columns,
                                              dims_dev.data_ptr() if dims_dev is not None else None, x.data_ptr(), k, _stream(y))
            if rc != 0:
                _fail(rc, "prep_inverse")
        return x.reshape(-1) if one_d else x


def fit_scaler(train, gaps="ignore"):
    """Fit the per-column min-max scaler on the (n, d) training series, where it lives (GPU: two launches, nothing read back).
    gaps="ignore" leaves the gaps out (sklearn's MinMaxScaler on data with NaNs); gaps="zero" counts every gap as the sample 0.0
    (the reference: nan_to_num runs before its fit).  Returns a SeriesScaler."""
    if gaps not in _GAPS:
        raise ValueError(f"gaps must be 'ignore' or 'zero', got {gaps!r}")
    x = _rows2d(train, "train")
    n, d = x.shape
    if x.device.type != "cuda":
        return SeriesScaler(_fit_cpu(x, gaps), gaps)
    lib = _lib()
    need = lib.mtadgat_prep_fit_scratch(n, d)
    if need == 0:
        raise RuntimeError("mtadgat_prep_fit_scratch refused the sizes")
    scratch = _scratch(need, x.device)
    rec = _native._empty((d, 6), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.mtadgat_prep_fit(x.data_ptr(), n, d, x.stride(0), _GAPS[gaps], scratch.data_ptr(), scratch.numel() * 8, rec.data_ptr(),
                                  _stream(x))
    if rc != 0:
        _fail(rc, "prep_fit")
    return SeriesScaler(rec, gaps)


# ---- live rows -------------------------------------------------------------------------------------------------------------------
class StreamPreparer:
    """SeriesScaler.transform for rows that arrive a few at a time from `n_streams` independent sources (GPU only, like
    StreamScorer): per (stream, column) the last valid raw value and the age live in one device allocation the host never reads.
    What a stream's rows come out as does not depend on how they were cut into pushes: it is transform(all its rows so far,
    fill, clip) with the stream as one part."""

    def __init__(self, scaler, n_streams, fill="hold", clip=False):
        if not isinstance(scaler, SeriesScaler):
            raise TypeError("scaler must be a SeriesScaler (fit_scaler)")
        if scaler.device.type != "cuda":
            raise RuntimeError(f"the scaler is on '{scaler.device}': the streaming path is GPU only (SeriesScaler.to)")
        if int(n_streams) != n_streams or n_streams < 1:
            raise ValueError(f"n_streams must be a positive integer, got {n_streams!r}")
        self.scaler, self.n_streams, self.fill, self.clip = scaler, int(n_streams), fill, bool(clip)
        self._fill = _fill_code(fill)
        self.device = scaler.device
        lib = _lib()
        nbytes = lib.mtadgat_prep_stream_state_bytes(self.n_streams, scaler.n_columns)
        if nbytes == 0:
            raise RuntimeError("mtadgat_prep_stream_state_bytes refused the sizes")
        self._state = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = lib.mtadgat_prep_stream_init(self._state.data_ptr(), self.n_streams, scaler.n_columns, _stream(self._state))
        if rc != 0:
            _fail(rc, "prep_stream_init")

    def _select(self, streams, n=None):
        if streams is None:
            if n is not None and n != self.n_streams:
                raise ValueError(f"{n} rows for {self.n_streams} streams: pass `streams` to push a subset")
            return None, self.n_streams
        if not isinstance(streams, torch.Tensor) or streams.device != self.device or streams.dtype != torch.int64 or streams.dim() != 1:
            raise ValueError("streams must be a 1-D int64 tensor of distinct stream indices on the preparer's device")
        if n is not None and streams.numel() != n:
            raise ValueError(f"{streams.numel()} stream indices for {n} rows")
        if not 1 <= streams.numel() <= self.n_streams:
            raise ValueError(f"streams must select between 1 and {self.n_streams} streams")
        return streams.contiguous(), streams.numel()

    def push(self, rows, streams=None, return_age=False):
        """The next T raw rows of n streams: rows (n, T, d) or (n, d) float32 on the device; streams None (all, in order) or n
        distinct int64 stream indices on the device.  Returns the prepared rows in the shape given, with return_age also their
        int32 age (SeriesScaler.transform)."""
        d = self.scaler.n_columns
        if not isinstance(rows, torch.Tensor) or rows.dim() not in (2, 3) or rows.shape[-1] != d or rows.shape[0] < 1:
            raise ValueError(f"rows must be a tensor of shape (n, T, {d}) or (n, {d})")
        if rows.device != self.device:
            raise RuntimeError(f"rows are on '{rows.device}', the preparer on '{self.device}': the streaming path is GPU only")
        shape = rows.shape
        r = rows.detach().float().reshape(shape[0], -1, d).contiguous()
        n, T = r.shape[0], r.shape[1]
        if T < 1:
            raise ValueError("a push carries at least one row per stream")
        st, _ = self._select(streams, n)
        out = _native._empty((n, T, d), dtype=torch.float32, device=self.device)
        age = _native._empty((n, T, d), dtype=torch.int32, device=self.device) if return_age else None
        with torch.cuda.device(self.device):
            rc = _lib().mtadgat_prep_stream_push(self._state.data_ptr(), self.n_streams, d, r.data_ptr(), st.data_ptr() if st is not None else None,
                                                 n, T, self.scaler.record.data_ptr(), self._fill, 1 if self.clip else 0, out.data_ptr(),
                                                 age.data_ptr() if return_age else None, _stream(r))
        if rc != 0:
            _fail(rc, "prep_stream_push")
        out = out.reshape(shape)
        return (out, age.reshape(shape)) if return_age else out

    def reset(self, streams=None):
        """Return the selected streams (None: all) to "nothing heard yet"."""
        st, n = self._select(streams)
        with torch.cuda.device(self.device):
            rc = _lib().mtadgat_prep_stream_reset(self._state.data_ptr(), self.n_streams, self.scaler.n_columns,
                                                  st.data_ptr() if st is not None else None, n, _stream(self._state))
        if rc != 0:
            _fail(rc, "prep_stream_reset")
