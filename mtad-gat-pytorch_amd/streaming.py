"""Scoring live streams row by row, with the model's state kept on the GPU.

`StreamScorer` is the deployment side of `MTAD_GAT.anomaly_scores` + `evaluation.anomaly_events`: telemetry of many
independent sources arrives a row (or a few rows) at a time, and every new row gets its anomaly score, an alarm flag and -- when
an alarm ends -- the finished event, in the same score-index space (score i of a stream belongs to its row i + window_size).

    scorer = StreamScorer(model, n_streams=256, threshold=eps, smoothing_span=None, merge_gap=2, min_length=3)
    out = scorer.push(rows)                  # rows (256, F): one new row per stream
    out["flags"], out["scores"]              # (256, 1) alarms and scores of these rows, on the device
    out["closed_start"] >= 0                 # where an event became final at this row

Everything that carries over between pushes -- per stream its row counter, the last window_size + max_block - 1 rows, the
forecast pending for the next row, the moving-average state and the open event -- lives in one device allocation that the host
never reads (csrc/mtadgat_stream.hip).  A push is three launches around ONE `mtadgat_forward_series` call: stage the rows into
the histories, run the model on the windows that end at the new rows (forecast and last reconstruction step only), advance the
state machines.  The only host read of a push is the 8-byte weight fingerprint every `MTAD_GAT` entry point waits for
(`model._checked`); it sits between the forward and the state update, so a repeated forward (weights edited in place) never
advances a stream twice.

The threshold may adapt per stream: pass an `evaluation.SpotState` (spot_calibrate on training scores) as `threshold` and every
stream runs SPOT's step on its own (smoothed) score inside the same kernel -- its excesses, its generalized Pareto fit and its alarm
threshold live in a second device allocation, and `out["thresholds"]` reports what each row was compared against.
"""
import ctypes

import torch

import _native
from evaluation import SpotState

_lib = _native.load_library
_Outputs = _native._Outputs
_CLOSED = (("closed_start", torch.int64), ("closed_end", torch.int64), ("closed_peak", torch.int64),
           ("closed_peak_score", torch.float32), ("closed_mean", torch.float32))


def _host(t, ctype):
    """The typed host pointer of a CPU tensor (None: NULL)."""
    return None if t is None else ctypes.cast(t.data_ptr(), ctypes.POINTER(ctype))


def window_start(count, t, window_size, ring_rows):
    """The first slot, within a stream's 2 * ring_rows history slots, of the window ending at its row `count + t`: the index
    arithmetic of the stage kernel (mtadgat_stream_window_start), callable without a GPU."""
    return int(_lib().mtadgat_stream_window_start(int(count), int(t), int(window_size), int(ring_rows)))


class StreamScorer:
    """Row-by-row anomaly scoring of `n_streams` independent series with one trained `model` (on the GPU, in eval()).

    threshold       a float, or an (n_streams,) tensor of per-stream thresholds: flag = float64(score) > threshold (NaN and
                    equality are not flagged, as evaluation.flag_runs); or an evaluation.SpotState of one column (every stream
                    starts from it) or n_streams columns: the scorer clones it, each stream then runs SPOT's step on its score
                    (after the smoothing) -- push / update also return "thresholds", (n, T) float64, what each row was compared
                    against (NaN for the warm-up rows) --, reset() restores the calibrated state, spot_state() is the live one
    target_dims     as MTAD_GAT.anomaly_scores: None (all features), an int or a list of series columns, one per out_dim
    gamma           weight of the reconstruction error in the score
    smoothing_span  None, or the span (>= 1) of the moving average of the score (evaluation.moving_average, per stream)
    scale           None, or (center, spread) of (out_dim,) values: per-dimension scores become (a - center) / (1 + spread) --
                    the median and the inter-quartile range of training scores (evaluation.column_quantiles), held fixed
    merge_gap,      the event rules of evaluation.flag_runs: flagged runs at most merge_gap samples apart are one event, events
    min_length      shorter than min_length are dropped
    max_block       the most rows per stream one push may carry
    prepare         None: the rows are scored as they come (a row with a NaN has no score, and poisons a moving average for good);
                    or a preparation.StreamPreparer for n_streams streams, or a (scaler, fill) pair one is made from: push and
                    update run the raw rows through it first -- scaled, the gaps filled ("zero" or "hold": no NaN reaches the
                    history or the moving average) --, reset() resets its streams too
    """

    def __init__(self, model, n_streams, threshold, target_dims=None, gamma=1.0, smoothing_span=None, scale=None, merge_gap=0,
                 min_length=1, max_block=64, prepare=None):
        F, d = model.n_features, model.out_dim
        if int(n_streams) != n_streams or n_streams < 1:
            raise ValueError(f"n_streams must be a positive integer, got {n_streams!r}")
        if int(max_block) != max_block or not 1 <= max_block <= 65536:
            raise ValueError(f"max_block must be an integer in [1, 65536], got {max_block!r}")
        if smoothing_span is not None and not smoothing_span >= 1:
            raise ValueError(f"smoothing_span must be >= 1, got {smoothing_span!r}")
        if int(merge_gap) != merge_gap or merge_gap < 0 or int(min_length) != min_length or min_length < 1:
            raise ValueError(f"needs integers merge_gap >= 0 and min_length >= 1, got {merge_gap!r}, {min_length!r}")
        if gamma != gamma:
            raise ValueError("gamma is NaN")
        dims = list(range(F)) if target_dims is None else ([target_dims] if isinstance(target_dims, int) else [int(c) for c in target_dims])
        if len(dims) != d:
            raise ValueError(f"target_dims select {len(dims)} columns but the model has out_dim={d}")
        if any(c < 0 or c >= F for c in dims):
            raise ValueError(f"target_dims must lie in [0, {F})")
        center = spread = None
        if scale is not None:
            center, spread = (torch.as_tensor(v, dtype=torch.float32).detach().reshape(-1).cpu().contiguous() for v in scale)
            if center.numel() != d or spread.numel() != d:
                raise ValueError(f"scale must be a (center, spread) pair of ({d},) values")
        thr = None
        spot = threshold if isinstance(threshold, SpotState) else None
        if spot is not None:
            if spot.n_columns not in (1, n_streams):
                raise ValueError(f"a SpotState of {spot.n_columns} columns for {n_streams} streams: it needs one column or one per stream")
            threshold = 0.0
        elif isinstance(threshold, torch.Tensor) and threshold.dim() > 0:
            if threshold.numel() != n_streams:
                raise ValueError(f"{threshold.numel()} thresholds for {n_streams} streams")
            thr = threshold
        param = next(model.parameters())
        model._require_gpu(param, "StreamScorer")
        self.model, self.device = model, param.device
        self.n_streams, self.max_block = int(n_streams), int(max_block)
        self.window_size, self.n_features, self.out_dim = model.window_size, F, d
        self.ring_rows = model.window_size + self.max_block - 1
        self.threshold = float(threshold) if thr is None else 0.0
        self._thresholds = None if thr is None else thr.detach().to(device=self.device, dtype=torch.float64).reshape(-1).contiguous()
        self._init_args = (float(gamma), 0.0 if smoothing_span is None else 2.0 / (float(smoothing_span) + 1.0), int(merge_gap),
                           int(min_length), torch.tensor(dims, dtype=torch.int32), center, spread)
        self._state = None
        self._ws = None
        self._spot = self._spot_calibrated = None
        self._prepare = None
        if prepare is not None:
            from preparation import StreamPreparer
            if not isinstance(prepare, StreamPreparer):
                scaler, fill = prepare
                prepare = StreamPreparer(scaler.to(self.device), self.n_streams, fill=fill)
            if prepare.n_streams != self.n_streams or prepare.scaler.n_columns != F or prepare.device != self.device:
                raise ValueError(f"prepare must serve {self.n_streams} streams of {F} columns on '{self.device}'")
            self._prepare = prepare
        if spot is not None:
            if spot.device != self.device:
                raise ValueError(f"the SpotState is on '{spot.device}', the model on '{self.device}'")
            self._spot_calibrated = spot.clone()
            self._spot = spot.expand(self.n_streams) if spot.n_columns == 1 and self.n_streams != 1 else spot.clone()

    # -- plumbing ------------------------------------------------------------------------------------------------------------
    def _stream(self):
        return _native._stream(self.device)

    def _fail(self, rc, what):
        _native._fail(_lib(), rc, what)

    def _ensure_state(self, eng):
        """The device allocation, made and initialised at the first call (the sizes come from the model's native handle)."""
        if self._state is not None:
            return
        lib = _lib()
        nbytes = lib.mtadgat_stream_state_bytes(eng.handle, self.n_streams, self.max_block)
        if nbytes == 0:
            raise RuntimeError("mtadgat_stream_state_bytes refused the sizes")
        state = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)
        gamma, alpha, gap, min_length, dims, center, spread = self._init_args
        with torch.cuda.device(self.device):
            rc = lib.mtadgat_stream_init(eng.handle, state.data_ptr(), self.n_streams, self.max_block, gamma, alpha, gap, min_length,
                                         _host(dims, ctypes.c_int32), _host(center, ctypes.c_float), _host(spread, ctypes.c_float),
                                         self._stream())
        if rc != 0:
            self._fail(rc, "stream_init")
        self._state = state

    def _engine(self):
        """The model's native handle without a weight check: update / flush / reset run no model kernel."""
        eng = self.model._engine
        if eng is None or eng.device != self.device:
            eng = self.model._checked(self.device, False, lambda e: e)
        self._ensure_state(eng)
        return eng

    def _select(self, streams, n=None):
        """(pointer or None, n) of a stream selection; None selects all streams in order."""
        if streams is None:
            if n is not None and n != self.n_streams:
                raise ValueError(f"{n} rows for {self.n_streams} streams: pass `streams` to push a subset")
            return None, self.n_streams
        if not isinstance(streams, torch.Tensor) or streams.device != self.device or streams.dtype != torch.int64 or streams.dim() != 1:
            raise ValueError("streams must be a 1-D int64 tensor of distinct stream indices on the scorer's device")
        if n is not None and streams.numel() != n:
            raise ValueError(f"{streams.numel()} stream indices for {n} rows")
        if not 1 <= streams.numel() <= self.n_streams:
            raise ValueError(f"streams must select between 1 and {self.n_streams} streams")
        return streams.contiguous(), streams.numel()

    def _rows(self, rows):
        if not isinstance(rows, torch.Tensor) or rows.dim() not in (2, 3):
            raise ValueError("rows must be a tensor of shape (n, T, F) or (n, F)")
        if rows.shape[-1] != self.n_features:
            raise ValueError(f"rows have {rows.shape[-1]} features, the model {self.n_features}")
        if rows.dim() == 2:
            rows = rows[:, None, :]
        if not 1 <= rows.shape[1] <= self.max_block:
            raise ValueError(f"a push carries between 1 and max_block = {self.max_block} rows per stream, got {rows.shape[1]}")
        if rows.device != self.device:
            raise RuntimeError(f"rows are on '{rows.device}', the scorer on '{self.device}': the streaming path is GPU only")
        return rows.detach().float().contiguous()

    def _outputs(self, n, T):
        dev = self.device
        out = {"scores": _native._empty((n, T), dtype=torch.float32, device=dev),
               "flags": torch.empty((n, T), dtype=torch.uint8, device=dev),
               "per_dim": _native._empty((n, T, self.out_dim), dtype=torch.float32, device=dev)}
        for name, dtype in _CLOSED:
            out[name] = torch.empty((n, T), dtype=dtype, device=dev)
        return out, _Outputs(**{k: v.data_ptr() for k, v in out.items()})

    def spot_state(self):
        """The live SpotState the streams advance (None for a scorer with fixed thresholds)."""
        return self._spot

    def _thr_ptr(self):
        return self._thresholds.data_ptr() if self._thresholds is not None else None

    def _commit(self, eng, preds, last, rows, st, n, T, staged):
        out, c_out = self._outputs(n, T)
        with torch.cuda.device(self.device):
            if self._spot is not None:
                thr = _native._empty((n, T), dtype=torch.float64, device=self.device)
                rc = _lib().mtadgat_stream_update_spot(eng.handle, self._state.data_ptr(), self.n_streams, self.max_block, preds, last,
                                                       rows.data_ptr(), st.data_ptr() if st is not None else None, n, T, 1 if staged else 0,
                                                       self._spot.data_ptr(), self._spot.max_peaks, thr.data_ptr(), ctypes.byref(c_out),
                                                       self._stream())
                out["thresholds"] = thr
            else:
                rc = _lib().mtadgat_stream_update(eng.handle, self._state.data_ptr(), self.n_streams, self.max_block, preds, last,
                                                  rows.data_ptr(), st.data_ptr() if st is not None else None, n, T, 1 if staged else 0,
                                                  self.threshold, self._thr_ptr(), ctypes.byref(c_out), self._stream())
        if rc != 0:
            self._fail(rc, "stream_update")
        return out

    # -- the public calls ------------------------------------------------------------------------------------------------------
    def push(self, rows, streams=None):
        """The next T rows of n streams: rows (n, T, F) or (n, F) float32 on the device, T <= max_block; streams None (all, in order)
        or n distinct int64 stream indices on the device.  Returns a dict of device tensors: scores (n, T) float32 (NaN for a
        stream's first window_size rows), flags (n, T) uint8, per_dim (n, T, out_dim) float32, and the event that became final at
        each row: closed_start (-1: none), closed_end, closed_peak int64, closed_peak_score, closed_mean float32."""
        self.model._require_gpu(next(self.model.parameters()), "StreamScorer.push")
        rows = self._rows(rows)
        n, T = rows.shape[0], rows.shape[1]
        st, _ = self._select(streams, n)
        if self._prepare is not None:
            rows = self._prepare.push(rows, st)
        lib = _lib()
        windows = n * T

        def stage_and_forward(eng):
            self._ensure_state(eng)
            need = lib.mtadgat_stream_workspace_bytes(eng.handle, windows)
            if self._ws is None or self._ws.numel() * 4 < need:
                self._ws = None
                self._ws = _native._empty((need + 3) // 4, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                rc = lib.mtadgat_stream_push(eng.handle, self._state.data_ptr(), self.n_streams, self.max_block, rows.data_ptr(),
                                             st.data_ptr() if st is not None else None, n, T, self.threshold, self._thr_ptr(), None,
                                             self._ws.data_ptr(), self._ws.numel() * 4, self._stream())
            if rc != 0:
                self._fail(rc, "stream_push")
            return eng

        with torch.no_grad():
            eng = self.model._checked(self.device, self.model._use_bf16(rows), stage_and_forward)
            od = (windows * self.out_dim + 3) // 4 * 4                     # the workspace starts with preds, then recons_last
            base = self._ws.data_ptr()
            return self._commit(eng, base, base + 4 * od, rows, st, n, T, staged=True)

    def update(self, preds, recons_last, rows, streams=None):
        """push() with the model outputs supplied by the caller: preds and recons_last (n, T, out_dim) (or (n, out_dim) with rows
        (n, F)) are the forecast and the last reconstruction step of the windows ENDING at the new rows."""
        rows = self._rows(rows)
        n, T = rows.shape[0], rows.shape[1]
        st, _ = self._select(streams, n)
        given = []
        for name, t in (("preds", preds), ("recons_last", recons_last)):
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.numel() != n * T * self.out_dim or t.shape[0] != n:
                raise ValueError(f"{name} must be a ({n}, {T}, {self.out_dim}) tensor on the scorer's device")
            given.append(t.detach().float().contiguous())
        if self._prepare is not None:
            rows = self._prepare.push(rows, st)
        eng = self._engine()
        return self._commit(eng, given[0].data_ptr(), given[1].data_ptr(), rows, st, n, T, staged=False)

    def flush(self, streams=None, reset=False):
        """The still-open event of each selected stream, ending at its last flagged sample + 1: a dict of (n,) device tensors
        closed_start (-1: none, or shorter than min_length), closed_end, closed_peak, closed_peak_score, closed_mean.  The streams
        go on as they are -- a later flagged row still extends the event -- unless reset=True."""
        st, n = self._select(streams)
        eng = self._engine()
        out = {name: torch.empty((n,), dtype=dtype, device=self.device) for name, dtype in _CLOSED}
        c_out = _Outputs(**{k: v.data_ptr() for k, v in out.items()})
        with torch.cuda.device(self.device):
            rc = _lib().mtadgat_stream_flush(eng.handle, self._state.data_ptr(), self.n_streams, self.max_block,
                                             st.data_ptr() if st is not None else None, n, 1 if reset and self._spot is None else 0,
                                             ctypes.byref(c_out), self._stream())
        if rc != 0:
            self._fail(rc, "stream_flush")
        if reset and self._spot is not None:
            self.reset(streams)
        elif reset and self._prepare is not None:
            self._prepare.reset(st)
        return out

    def reset(self, streams=None):
        """Return the selected streams (None: all) to their initial state: no rows seen, no open event, and -- with a SpotState --
        the calibrated thresholds, counts and excesses."""
        st, n = self._select(streams)
        eng = self._engine()
        if self._prepare is not None:
            self._prepare.reset(st)
        sp = st.data_ptr() if st is not None else None
        with torch.cuda.device(self.device):
            if self._spot is not None:
                cal = self._spot_calibrated
                rc = _lib().mtadgat_stream_reset_spot(eng.handle, self._state.data_ptr(), self.n_streams, self.max_block, self._spot.data_ptr(),
                                                      cal.data_ptr(), cal.n_columns, cal.max_peaks, sp, n, self._stream())
            else:
                rc = _lib().mtadgat_stream_flush(eng.handle, self._state.data_ptr(), self.n_streams, self.max_block, sp, n, 1, None, self._stream())
        if rc != 0:
            self._fail(rc, "stream_flush")
