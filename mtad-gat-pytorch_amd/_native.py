"""ctypes binding of the C ABI in include/mtadgat.h (libmtadgat.so, gfx950 HIP kernels).

PyTorch is used for device memory and the current HIP stream only.  There is no
fallback: if the library is missing or the tensors are not on a HIP device the
calls raise.
"""
import ctypes
import os

import torch  # must be imported before the library: both bind libamdhip64.so.7, torch's copy wins

import _abi

# Debugging aid (tests/test_gpu_fuzz.py): every scratch buffer handed to the library (workspace, training tape) is
# filled with a large finite value before each call, so a kernel that USES scratch it did not write shows up in the outputs of a
# single call instead of depending on what the caching allocator left in the block (finite, inside the fp16 range: padding that
# is read and multiplied by zero weights is legitimate and stays harmless).
_POISON_SCRATCH = bool(os.environ.get("MTADGAT_POISON_SCRATCH"))
_POISON_VALUE = 7777.0


def _empty(*shape, **kw):
    """torch.empty, poisoned under MTADGAT_POISON_SCRATCH (outputs included: a kernel that accumulates into an output it was
    supposed to write, or leaves part of it unwritten, shows up the same way).  Every buffer this layer hands the library is
    allocated here or by _empty_like: tests/arena.py replaces both to hand out exactly sized, guard-banded buffers."""
    t = torch.empty(*shape, **kw)
    if _POISON_SCRATCH and t.is_floating_point() and t.device.type == "cuda":
        t.fill_(_POISON_VALUE)
    return t


def _empty_like(x):
    return _empty(x.shape, dtype=x.dtype, device=x.device)


def _stream(device=None):
    """The current HIP stream of `device` -- a tensor stands for its device, None for the current device -- as the void* the
    library takes."""
    if isinstance(device, torch.Tensor):
        device = device.device
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _scratch(nbytes, device, least=0):
    """Scratch of max(nbytes, least) bytes in 8-byte words from _empty (poisoned under MTADGAT_POISON_SCRATCH): exactly the
    header's minimum unless the caller asks for a floor."""
    return _empty((max(nbytes, least) + 7) // 8, dtype=torch.float64, device=device)


def _fail(lib, rc, what):
    raise RuntimeError(f"mtadgat {what} failed (status {rc}): {lib.mtadgat_last_error().decode('utf-8', 'replace')}")


def _rows2d(t, name, gpu_only=False, max_columns=None):
    """A float32 (n, d) tensor whose rows are contiguous (a column slice keeps its row stride: no copy); 1-D is one column.
    gpu_only: the evaluation kernels' check; max_columns: the preparation's limit."""
    if gpu_only and (not isinstance(t, torch.Tensor) or t.device.type != "cuda"):
        raise RuntimeError(f"{name} must be a tensor on the GPU (the evaluation kernels are HIP only)")
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    t = t.detach()
    if t.ndim == 1:
        t = t.reshape(-1, 1)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name} must have shape (n, d) with n, d >= 1, got {tuple(t.shape)}")
    if max_columns is not None and t.shape[1] > max_columns:
        raise ValueError(f"{name} has {t.shape[1]} columns, the preparation covers up to {max_columns}")
    if t.dtype != torch.float32:
        t = t.float()
    if t.shape[0] == 1:                    # a single row: any row stride is legal in torch, the kernels want ld >= d
        t = t.as_strided((1, t.shape[1]), (t.shape[1], 1)) if t.shape[1] == 1 or t.stride(1) == 1 else t.reshape(1, -1).clone()
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libmtadgat.so")
_HEADER = _abi.read()                  # include/mtadgat.h: the constants here, the Structures below and every declaration come from it
ABI_VERSION = _HEADER.defines["MTADGAT_ABI_VERSION"]
MAX_LAYERS = _HEADER.defines["MTADGAT_MAX_LAYERS"]
PROFILE_SLOTS = _HEADER.defines["MTADGAT_PROFILE_SLOTS"]
# mtadgat_gru_route: the integers it writes, the kernel codes (GruKernel) and operand builds (GruBuild) of csrc/mtadgat_host.h
GRU_ROUTE_FIELDS = ("first", "fallback", "build", "two", "hoist", "split_packs", "fc_rides", "small_stack")
GRU_KERNELS = ("none", "k_gru1", "k_gru16", "k_gru_split", "k_gru_split_x3", "k_gru_cm", "k_gru")
GRU_BUILDS = ("fp32", "bf16", "x3_hi", "x3_lo")
# mtadgat_train_route: the backward kernel codes (GruBwdKernel of csrc/mtadgat_host.h)
GRU_BWD_KERNELS = ("k_gru1_bwd", "k_gru16_bwd", "k_gru_bwd")
# mtadgat_front_route: the integers it writes (include/mtadgat.h) and the codes of csrc/mtadgat_host.h
FRONT_ROUTE_FIELDS = ("conv", "conv_build", "conv_split_pack", "range",
                      "temp_kernel", "temp_build", "temp_fp16", "temp_split_gemm", "temp_split_pack",
                      "feat_kernel", "feat_build", "feat_fp16", "feat_split_gemm", "feat_split_pack")
# mtadgat_wgrad_plan: the ten integers per weight-gradient site (include/mtadgat.h)
WGRAD_PLAN_FIELDS = ("R", "M", "N", "Mp", "Np", "nslab", "rows_per_slab", "bmode", "bshift", "x3")
FRONT_KINDS = ("forward", "forward_unfused", "train", "attention", "conv")
FRONT_SOURCES = ("windows", "windows_bf16", "series_unit", "series")
FRONT_CONVS = ("in_gath", "k_conv_win", "shared_rows", "launch_conv")
FRONT_LAYERS = ("none", "k_gat", "k_gath+k_gat", "rowgemm+k_gat_wide", "rowgemm+k_attend")
FRONT_BUILDS = ("fp32", "bf16", "x3")
# mtadgat_fit_prepare: the float64 fields of the step record and of a row of the log ring (include/mtadgat.h)
FIT_STATE_FIELDS = ("t", "calls", "clip", "step_size", "bc2s", "applied", "norm_sq", "norm")
FIT_LOG_FIELDS = ("rmse_forecast", "rmse_recon", "norm", "applied")
assert len(FIT_STATE_FIELDS) == _HEADER.defines["MTADGAT_FIT_STATE_FIELDS"]


class Config(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "n_features", "window_size", "out_dim", "kernel_size", "use_gatv2", "feat_embed", "time_embed",
        "gru_n_layers", "gru_hid_dim", "forecast_n_linear", "forecast_hid_dim", "recon_n_layers",
        "recon_hid_dim")] + [("alpha", ctypes.c_float)]


class Params(ctypes.Structure):
    _fields_ = (
        [(n, ctypes.c_void_p) for n in (
            "conv_weight", "conv_bias", "feat_lin_weight", "feat_lin_bias", "feat_a", "feat_bias",
            "temp_lin_weight", "temp_lin_bias", "temp_a", "temp_bias")]
        + [(n, ctypes.c_void_p * MAX_LAYERS) for n in (
            "gru_w_ih", "gru_w_hh", "gru_b_ih", "gru_b_hh", "fc_weight", "fc_bias",
            "rec_w_ih", "rec_w_hh", "rec_b_ih", "rec_b_hh")]
        + [("rec_fc_weight", ctypes.c_void_p), ("rec_fc_bias", ctypes.c_void_p)])


class _Outputs(ctypes.Structure):
    """mtadgat_stream_outputs (streaming.py fills it)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("scores", "flags", "per_dim", "closed_start", "closed_end", "closed_peak",
                                                "closed_peak_score", "closed_mean")]


_HEADER.register(mtadgat_config=Config, mtadgat_params=Params, mtadgat_stream_outputs=_Outputs)
_lib = None


def library_path():
    return _LIB_PATH


def load_library():
    """Load libmtadgat.so (raises with build instructions if it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"{_LIB_PATH} is missing: the MI355X HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`python mtad-gat-pytorch_amd/build.py`). There is no non-HIP implementation.")
    lib = _HEADER.bind(ctypes.CDLL(_LIB_PATH))
    if lib.mtadgat_abi_version() != ABI_VERSION:
        raise RuntimeError("libmtadgat.so ABI version mismatch")
    _lib = lib
    return lib


# mtadgat_split_steps: SplitStep::Op of csrc/mtadgat_host.h and the fields of a record
SPLIT_OPS = ("ZERO_SCALE", "ABSMAX", "SCALE_FROM_MAX", "SPLIT3", "SPLIT2H", "SPLIT2H_GATH", "SPLIT_X", "REORDER_XQ")
SPLIT_STEP_FIELDS = ("group", "op", "scale", "src", "dst", "n", "Qs", "Qd", "arg", "ord")


def split_steps(lib, handle):
    """mtadgat_split_steps of a handle as a list of dicts (needs no GPU: the host tests call it on a bare handle)."""
    n = lib.mtadgat_split_steps(handle, None, 0)
    buf = (ctypes.c_int64 * (10 * n))()
    n = lib.mtadgat_split_steps(handle, buf, n)
    steps = [dict(zip(SPLIT_STEP_FIELDS, (int(v) for v in buf[10 * i:10 * i + 10]))) for i in range(n)]
    for s in steps:
        s["op"] = SPLIT_OPS[s["op"]]
    return steps


def _check(rc, what):
    if rc != 0:
        msg = load_library().mtadgat_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"mtadgat {what} failed (status {rc}): {msg}")


def _dev_ptr(t, name, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(
            f"{name} is on '{t.device}': the MI355X HIP path needs tensors on the GPU "
            "('cuda' = HIP on PyTorch-ROCm); there is no CPU implementation")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


# -- the series trainer's kernels (csrc/mtadgat_fit.hip; tests/fit_refs.py is the specification) --------------
# Handle-free, asynchronous on the current stream of the tensors' device; none of them reads from the device.
def _typed(t, dtype, name, numel=None):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous {dtype} tensor on the GPU")
    if numel is not None and t.numel() != numel:
        raise RuntimeError(f"{name} holds {t.numel()} elements, expected {numel}")
    return ctypes.c_void_p(t.data_ptr())


def _series_rows(series):
    if (not isinstance(series, torch.Tensor) or series.device.type != "cuda" or series.dtype != torch.float32 or series.ndim != 2
            or series.shape[0] < 1 or series.shape[1] < 1 or series.stride(1) != 1 or series.stride(0) < series.shape[1]):
        raise RuntimeError("series must be a float32 (n_rows, F) tensor on the GPU whose rows are contiguous")
    return ctypes.c_void_p(series.data_ptr()), series.shape[0], series.shape[1], series.stride(0)


def fit_gather(series, starts, W, out=None):
    """x[w, t, :] = series[starts[w] + t] for t < W (mtadgat_fit_gather): (len(starts), W, F) float32.  starts: int64 on the
    GPU, every starts[w] in [0, n_rows - W] -- the caller's to check."""
    sp, n_rows, F, ld = _series_rows(series)
    b = starts.numel()
    if out is None:
        out = _empty((b, W, F), dtype=torch.float32, device=series.device)
    with torch.cuda.device(series.device):
        _check(load_library().mtadgat_fit_gather(sp, n_rows, F, ld, _typed(starts, torch.int64, "starts"), b, W,
                                                 _typed(out, torch.float32, "x", b * W * F), _stream(series)), "fit_gather")
    return out


def fit_loss_grad(preds, recons, series, starts, sums, dims=None, d_preds=None, d_recons=None, rmse=None):
    """(d_preds, d_recons, rmse (2,) float64) of loss = rmse_forecast + rmse_recon over one batch (mtadgat_fit_loss_grad).  sums:
    the batch's two squared-error sums on the device, mtadgat_eval_window_sse then mtadgat_eval_group_sums(group = batch).
    dims: int32 on the GPU or None."""
    sp, n_rows, F, ld = _series_rows(series)
    b, W, out = recons.shape
    dev = series.device
    d_preds = _empty((b, out), dtype=torch.float32, device=dev) if d_preds is None else d_preds
    d_recons = _empty((b, W, out), dtype=torch.float32, device=dev) if d_recons is None else d_recons
    rmse = _empty(2, dtype=torch.float64, device=dev) if rmse is None else rmse
    with torch.cuda.device(dev):
        _check(load_library().mtadgat_fit_loss_grad(
            _typed(preds, torch.float32, "preds", b * out), _typed(recons, torch.float32, "recons"), b, W, out, sp, n_rows, F, ld,
            _typed(starts, torch.int64, "starts", b), None if dims is None else _typed(dims, torch.int32, "dims", out),
            _typed(sums, torch.float64, "sums", 2), _typed(d_preds, torch.float32, "d_preds", b * out),
            _typed(d_recons, torch.float32, "d_recons", b * W * out), _typed(rmse, torch.float64, "rmse", 2), _stream(series)),
            "fit_loss_grad")
    return d_preds, d_recons, rmse


def fit_prepare(grads, rmse, state, log, lr, betas, max_grad_norm=None, skip_nonfinite=False, scratch=None):
    """The gradient norm and the step record (mtadgat_fit_prepare): state (8,) float64 -- FIT_STATE_FIELDS, zeroed before the first
    step --, log (capacity, 4) float64 -- FIT_LOG_FIELDS.  scratch: float64, mtadgat_fit_prepare_scratch(n) bytes."""
    lib = load_library()
    n = grads.numel()
    need = lib.mtadgat_fit_prepare_scratch(n)
    if scratch is None:
        scratch = _empty(max(1, (need + 7) // 8), dtype=torch.float64, device=grads.device)
    with torch.cuda.device(grads.device):
        _check(lib.mtadgat_fit_prepare(
            _typed(grads, torch.float32, "grads"), n, _typed(rmse, torch.float64, "rmse", 2), float(lr), float(betas[0]), float(betas[1]),
            -1.0 if max_grad_norm is None else float(max_grad_norm), int(bool(skip_nonfinite)),
            _typed(state, torch.float64, "state", len(FIT_STATE_FIELDS)), _typed(log, torch.float64, "log"), log.numel() // 4,
            _typed(scratch, torch.float64, "scratch"), scratch.numel() * 8, _stream(grads)), "fit_prepare")


def fit_adam(params, grads, exp_avg, exp_avg_sq, state, lr, betas, eps, weight_decay=0.0, decoupled=False):
    """Adam / AdamW over the flat float32 buffers, in place, from the record fit_prepare left in `state` (mtadgat_fit_adam)."""
    n = params.numel()
    with torch.cuda.device(params.device):
        _check(load_library().mtadgat_fit_adam(
            _typed(params, torch.float32, "params"), _typed(grads, torch.float32, "grads", n), _typed(exp_avg, torch.float32, "exp_avg", n),
            _typed(exp_avg_sq, torch.float32, "exp_avg_sq", n), n, _typed(state, torch.float64, "state", len(FIT_STATE_FIELDS)),
            float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(bool(decoupled)), _stream(params)),
            "fit_adam")


# -- training on gappy, concatenated series (csrc/mtadgat_fitwin.hip and the masked instances of _losses.hip / _fit.hip;
#    tests/fit_mask_refs.py is the specification) ----------------------------------------------------------------------------------
def _age_rows(age, n_rows, F, device):
    """age: the int32 (n_rows, F) tensor of SeriesScaler.transform(..., return_age=True) on `device`, rows contiguous."""
    if (not isinstance(age, torch.Tensor) or age.device != device or age.dtype != torch.int32 or age.ndim != 2
            or tuple(age.shape) != (n_rows, F) or (F > 1 and age.stride(1) != 1) or (n_rows > 1 and age.stride(0) < F)):
        raise RuntimeError(f"age must be an int32 ({n_rows}, {F}) tensor on {device} whose rows are contiguous "
                           "(a boolean mask m of observed samples is (~m).to(torch.int32))")
    return ctypes.c_void_p(age.data_ptr()), (age.stride(0) if n_rows > 1 else F)


def fit_windows(n_rows, W, F, device, age=None, max_age=0, dims=None, out_dim=None, offsets=None, min_count=0):
    """(starts, count) of mtadgat_fit_windows: starts int64 (n_rows - W,) on `device`, its first `count` entries the valid window
    starts in ascending order, count a one-element int64 device tensor -- nothing is read from the device.  dims: int32 on the device
    or None (then columns 0 .. out_dim - 1, out_dim defaulting to F); offsets: the P + 1 int64 part offsets on the device or None."""
    lib = load_library()
    device = torch.device(device)
    n_rows, W, F = int(n_rows), int(W), int(F)
    out_dim = (F if dims is None else dims.numel()) if out_dim is None else int(out_dim)
    need = lib.mtadgat_fit_windows_scratch(n_rows)
    if need == 0 or n_rows < W:
        raise ValueError(f"fit_windows: n_rows must lie in [W, 2^31 - 1], got {n_rows} (W = {W})")
    ap, ld = (None, 0) if age is None else _age_rows(age, n_rows, F, device)
    starts = _empty((max(n_rows - W, 1),), dtype=torch.int64, device=device)        # (one entry where there is no start: a pointer to pass)
    count = _empty((1,), dtype=torch.int64, device=device)
    scratch = _scratch(need, device)
    with torch.cuda.device(device):
        _check(lib.mtadgat_fit_windows(
            ap, ld, int(max_age), n_rows, F, W, None if dims is None else _typed(dims, torch.int32, "dims", out_dim), out_dim,
            None if offsets is None else _typed(offsets, torch.int64, "offsets"), 1 if offsets is None else offsets.numel() - 1,
            int(min_count), ctypes.c_void_p(starts.data_ptr()), _typed(count, torch.int64, "count", 1),
            _typed(scratch, torch.float64, "scratch"), scratch.numel() * 8, _stream(device)), "fit_windows")
    return starts[:n_rows - W], count


def fit_masked_sse(preds, recons, series, starts, age, max_age=0, dims=None, want_dims=True):
    """(window (b, 4) float64 = S_f, S_r, N_f, N_r per window, dim (4, out) float64 or None) of mtadgat_fit_masked_sse: the squared
    errors of mtadgat_eval_window_sse over the observed samples (age <= max_age) and their counts."""
    lib = load_library()
    sp, n_rows, F, ld = _series_rows(series)
    b, W, out = recons.shape
    dev = series.device
    ap, lda = _age_rows(age, n_rows, F, dev)
    window = _empty((b, 4), dtype=torch.float64, device=dev)
    dim = _empty((4, out), dtype=torch.float64, device=dev) if want_dims else None
    scratch = _scratch(lib.mtadgat_fit_masked_sse_scratch(b, out), dev)
    with torch.cuda.device(dev):
        _check(lib.mtadgat_fit_masked_sse(
            _typed(preds, torch.float32, "preds", b * out), _typed(recons, torch.float32, "recons"), b, W, out, sp, n_rows, F, ld,
            _typed(starts, torch.int64, "starts", b), 0, 0, None if dims is None else _typed(dims, torch.int32, "dims", out), ap, lda,
            int(max_age), 0, _typed(window, torch.float64, "window"), None if dim is None else _typed(dim, torch.float64, "dim"),
            _typed(scratch, torch.float64, "scratch"), scratch.numel() * 8, _stream(series)), "fit_masked_sse")
    return window, dim


def fit_masked_loss_grad(preds, recons, series, starts, age, sums, max_age=0, dims=None, d_preds=None, d_recons=None, rmse=None):
    """fit_loss_grad over observed samples (mtadgat_fit_masked_loss_grad).  sums: the batch's (S_f, S_r, N_f, N_r) on the device,
    fit_masked_sse then mtadgat_eval_group_sums(cols = 4, group = batch).  An unobserved entry's cotangent is +0.0."""
    sp, n_rows, F, ld = _series_rows(series)
    b, W, out = recons.shape
    dev = series.device
    ap, lda = _age_rows(age, n_rows, F, dev)
    d_preds = _empty((b, out), dtype=torch.float32, device=dev) if d_preds is None else d_preds
    d_recons = _empty((b, W, out), dtype=torch.float32, device=dev) if d_recons is None else d_recons
    rmse = _empty(2, dtype=torch.float64, device=dev) if rmse is None else rmse
    with torch.cuda.device(dev):
        _check(load_library().mtadgat_fit_masked_loss_grad(
            _typed(preds, torch.float32, "preds", b * out), _typed(recons, torch.float32, "recons"), b, W, out, sp, n_rows, F, ld,
            _typed(starts, torch.int64, "starts", b), None if dims is None else _typed(dims, torch.int32, "dims", out), ap, lda,
            int(max_age), _typed(sums, torch.float64, "sums", 4), _typed(d_preds, torch.float32, "d_preds", b * out),
            _typed(d_recons, torch.float32, "d_recons", b * W * out), _typed(rmse, torch.float64, "rmse", 2), _stream(series)),
            "fit_masked_loss_grad")
    return d_preds, d_recons, rmse


class Engine:
    """One model instance on the native side: packed weights + launch plans."""

    def __init__(self, cfg: dict, device):
        self.lib = load_library()
        self.cfg = Config(**cfg)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"the MI355X HIP engine lives on a GPU, not on '{device}'")
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):      # the library sizes its chunks from this device's memory
            _check(self.lib.mtadgat_create(ctypes.byref(self.cfg), ctypes.byref(self.handle)), "create")
        self._ws = None
        self._keep = None

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                self.lib.mtadgat_destroy(self.handle)
                self.handle = ctypes.c_void_p()
        except Exception:
            pass

    # -- training step ------------------------------------------------------------------------------
    def backward_supported(self):
        """True when the library has a HIP backward for this configuration (else why_not() says why)."""
        return bool(self.lib.mtadgat_backward_supported(self.handle))

    def why_not(self):
        self.lib.mtadgat_backward_supported(self.handle)
        return self.lib.mtadgat_last_error().decode("utf-8", "replace")

    def grad_layout(self):
        """[offsets] of the flat gradient buffer in the field order of mtadgat_params, total floats."""
        n = 10 + 4 * self.cfg.gru_n_layers + 2 * self.cfg.forecast_n_linear + 4 * self.cfg.recon_n_layers + 2
        offs = (ctypes.c_int64 * n)()
        got = self.lib.mtadgat_grad_offsets(self.handle, offs, n)
        if got != n:
            raise RuntimeError("mtadgat_grad_offsets: unexpected parameter count")
        return list(offs), int(self.lib.mtadgat_grad_floats(self.handle))

    TAPE_FIELDS = ("hcat", "xct", "att_f", "att_t", "hend", "gates_g", "seq_g", "gates_d", "seq_d", "xdec")
    WS_FIELDS = ("da", "dhcat", "dhdec", "dhend", "dz0", "dz1", "de_f", "de_t", "dv_f", "dv_t", "dlr_f", "dlr_t",
                 "dap_f", "dap_t", "dpre")

    def train_layout(self, batch):
        """Diagnostics: float offsets of the tape / backward-workspace regions for `batch` windows."""
        n = len(self.TAPE_FIELDS) + len(self.WS_FIELDS)
        offs = (ctypes.c_int64 * n)()
        if self.lib.mtadgat_train_layout(self.handle, batch, offs, n) != n:
            raise RuntimeError("mtadgat_train_layout failed")
        v = list(offs)
        return dict(zip(self.TAPE_FIELDS, v[:len(self.TAPE_FIELDS)])), dict(zip(self.WS_FIELDS, v[len(self.TAPE_FIELDS):]))

    def _buf(self, name, nbytes, device, fresh=True):
        cur = getattr(self, name, None)
        if cur is None or cur.device != device or cur.numel() * 4 < nbytes:
            setattr(self, name, None)
            cur = _empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
            setattr(self, name, cur)
        if _POISON_SCRATCH and fresh:
            cur.fill_(_POISON_VALUE)
        return cur

    def forward_train(self, x, p, seed, window0=0, tape=None):
        """Training forward of `x` (one chunk): (preds, recons, tape).  Dropout with probability p inside the kernels."""
        c = self.cfg
        b = x.shape[0]
        xp = _dev_ptr(x, "x", (b, c.window_size, c.n_features))
        preds = _empty((b, c.out_dim), dtype=torch.float32, device=x.device)
        recons = _empty((b, c.window_size, c.out_dim), dtype=torch.float32, device=x.device)
        if b == 0:
            return preds, recons, None
        need = self.lib.mtadgat_tape_bytes(self.handle, b)
        if tape is None or tape.numel() * 4 < need:
            tape = _empty((need + 3) // 4, dtype=torch.float32, device=x.device)
        if _POISON_SCRATCH:
            tape.fill_(_POISON_VALUE)
        self._call(self.lib.mtadgat_forward_train, "forward_train", x.device, xp, b, int(window0), float(p), int(seed),
                   _dev_ptr(preds, "preds"), _dev_ptr(recons, "recons"), _dev_ptr(tape, "tape"), need)
        return preds, recons, tape

    def backward(self, x, p, seed, d_preds, d_recons, tape, grads, window0=0):
        """Accumulates the parameter gradients of one chunk into the flat buffer `grads`."""
        c = self.cfg
        b = x.shape[0]
        if b == 0:
            return
        xp = _dev_ptr(x, "x", (b, c.window_size, c.n_features))
        need_t = self.lib.mtadgat_tape_bytes(self.handle, b)
        need_w = self.lib.mtadgat_backward_workspace_bytes(self.handle, b)
        ws = self._buf("_bws", need_w, x.device)
        self._call(self.lib.mtadgat_backward, "backward", x.device, xp, b, int(window0), float(p), int(seed),
                   _dev_ptr(d_preds, "d_preds", (b, c.out_dim)), _dev_ptr(d_recons, "d_recons", (b, c.window_size, c.out_dim)),
                   _dev_ptr(tape, "tape"), need_t, _dev_ptr(grads, "grads"), _dev_ptr(ws, "workspace"), need_w)

    def backward_input(self, x_like):
        """d loss / d x of the chunk mtadgat_backward just processed (same stream, same workspace): (b, W, F)."""
        c = self.cfg
        b = x_like.shape[0]
        dx = _empty((b, c.window_size, c.n_features), dtype=torch.float32, device=x_like.device)
        if b == 0:
            return dx
        need_w = self.lib.mtadgat_backward_workspace_bytes(self.handle, b)
        ws = self._buf("_bws", need_w, x_like.device, fresh=False)      # (mtadgat_backward's d pre-activations are read from it)
        self._call(self.lib.mtadgat_backward_input, "backward_input", x_like.device, b, _dev_ptr(ws, "workspace"), need_w, _dev_ptr(dx, "dx"))
        return dx

    def backward_data(self, x, p, seed, d_preds, d_recons, tape, window0=0):
        """The data-only backward of one chunk (mtadgat_backward_data): d loss / d x (b, W, F) from the tape of forward_train, with
        no weight gradient computed and no gradient buffer; bit-identical to backward() + backward_input() on the same chunk."""
        c = self.cfg
        b = x.shape[0]
        dx = _empty((b, c.window_size, c.n_features), dtype=torch.float32, device=x.device)
        if b == 0:
            return dx
        xp = _dev_ptr(x, "x", (b, c.window_size, c.n_features))
        need_t = self.lib.mtadgat_tape_bytes(self.handle, b)
        need_w = self.lib.mtadgat_backward_workspace_bytes(self.handle, b)
        ws = self._buf("_bws", need_w, x.device)
        self._call(self.lib.mtadgat_backward_data, "backward_data", x.device, xp, b, int(window0), float(p), int(seed),
                   _dev_ptr(d_preds, "d_preds", (b, c.out_dim)), _dev_ptr(d_recons, "d_recons", (b, c.window_size, c.out_dim)),
                   _dev_ptr(tape, "tape"), need_t, _dev_ptr(dx, "dx"), _dev_ptr(ws, "workspace"), need_w)
        return dx

    def score_attribution_workspace_bytes(self, count, steps):
        return int(self.lib.mtadgat_score_attribution_workspace_bytes(self.handle, int(count), int(steps)))

    def score_attribution(self, series, idx, dims, dim_w, gamma, steps, baseline=None):
        """Attribution of the anomaly scores at indices `idx` (int64, on the series' device) to the W + 1 rows each reads:
        (count, W + 1, F).  dims (out_dim) int32 series columns, dim_w (out_dim) float32 weights w_d, steps 0 = gradient, else
        Integrated Gradients with `steps` midpoint nodes from `baseline` (None = zeros, (F,) or (W + 1, F))."""
        c = self.cfg
        W, F = c.window_size, c.n_features
        dev = series.device
        sp = _dev_ptr(series, "series")
        if series.dim() != 2 or series.shape[1] != F:
            raise RuntimeError(f"series must have shape (n_rows, {F}), got {tuple(series.shape)}")
        for t, name, dt in ((idx, "indices", torch.int64), (dims, "dims", torch.int32)):
            if t.dtype != dt or t.device != dev or not t.is_contiguous() or t.dim() != 1:
                raise RuntimeError(f"{name} must be a contiguous 1-D {dt} tensor on the series' device")
        count = idx.shape[0]
        out = _empty((count, W + 1, F), dtype=torch.float32, device=dev)
        if count == 0:
            return out
        if not self.backward_supported():
            raise RuntimeError("score attribution needs the HIP backward, which this configuration lacks: " + self.why_not())
        kind, bp = 0, None
        if baseline is not None:
            kind = 1 if baseline.dim() == 1 else 2
            bp = _dev_ptr(baseline, "baseline", (F,) if kind == 1 else (W + 1, F))
        need = self.score_attribution_workspace_bytes(count, steps)
        ws = _empty((need + 3) // 4, dtype=torch.float32, device=dev)
        self._call(self.lib.mtadgat_score_attribution, "score_attribution", dev, sp, series.shape[0], ctypes.c_void_p(idx.data_ptr()),
                   count, ctypes.c_void_p(dims.data_ptr()), dims.shape[0], _dev_ptr(dim_w, "dim_w", (dims.shape[0],)), float(gamma),
                   int(steps), bp, kind, _dev_ptr(out, "out"), _dev_ptr(ws, "workspace"), need)
        return out

    def dropout_masks(self, batch, p, seed, device, window0=0):
        """The keep-masks the kernels apply: {"feat": (b,F,F), "temp": (b,W,W), "fc": [(b,hid)] * hidden layers}."""
        c = self.cfg
        mf = _empty((batch, c.n_features, c.n_features), dtype=torch.float32, device=device)
        mt = _empty((batch, c.window_size, c.window_size), dtype=torch.float32, device=device)
        nh = c.forecast_n_linear - 1
        mfc = _empty((max(nh, 1), batch, c.forecast_hid_dim), dtype=torch.float32, device=device)
        self._call(self.lib.mtadgat_dropout_masks, "dropout_masks", device, batch, int(window0), float(p), int(seed),
                   _dev_ptr(mf, "mask"), _dev_ptr(mt, "mask"), _dev_ptr(mfc, "mask"))
        out = {"feat": mf, "temp": mt, "fc": [mfc[i] for i in range(nh)]}
        lg, ld = c.gru_n_layers - 1, c.recon_n_layers - 1
        if lg > 0 or ld > 0:      # nn.GRU's dropout between stacked layers
            mg = _empty((max(lg, 1), batch, c.window_size, c.gru_hid_dim), dtype=torch.float32, device=device)
            mr = _empty((max(ld, 1), batch, c.window_size, c.recon_hid_dim), dtype=torch.float32, device=device)
            self._call(self.lib.mtadgat_dropout_masks_rnn, "dropout_masks_rnn", device, batch, int(window0), float(p), int(seed),
                       _dev_ptr(mg, "mask") if lg > 0 else None, _dev_ptr(mr, "mask") if ld > 0 else None)
            out["gru"] = [mg[i] for i in range(lg)]
            out["rec"] = [mr[i] for i in range(ld)]
        return out

    # -- weights ------------------------------------------------------------------------------
    def flat_keys(self):
        """state_dict keys in the field order of mtadgat_params (= the flat parameter / gradient buffer)."""
        names = ["conv.conv.weight", "conv.conv.bias"]
        for g in ("feature_gat", "temporal_gat"):
            names += [f"{g}.lin.weight", f"{g}.lin.bias", f"{g}.a", f"{g}.bias"]
        for l in range(self.cfg.gru_n_layers):
            names += [f"gru.gru.{k}_l{l}" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        for i in range(self.cfg.forecast_n_linear):
            names += [f"forecasting_model.layers.{i}.weight", f"forecasting_model.layers.{i}.bias"]
        for l in range(self.cfg.recon_n_layers):
            names += [f"recon_model.decoder.rnn.{k}_l{l}" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        return names + ["recon_model.fc.weight", "recon_model.fc.bias"]

    def update_weights_device(self, sd, device):
        """Re-pack from parameters that live on `device` without leaving it (after an optimizer step).  False when the
        library declines (no earlier host-side load, bf16 image, ...): the caller then uses load_weights."""
        if self._keep is None:
            return False
        flat = torch.cat([sd[k].detach().reshape(-1).to(torch.float32) for k in self.flat_keys()])
        if flat.device != device:
            return False
        with torch.cuda.device(device):
            rc = self.lib.mtadgat_update_weights_device(self.handle, ctypes.c_void_p(flat.data_ptr()), flat.numel(), _stream())
        if rc == -2:          # MTADGAT_ERR_UNSUPPORTED
            return False
        _check(rc, "update_weights_device")
        self._flat_dev = flat     # read by the kernels queued on the stream
        return True

    def fingerprint(self, params, device):
        """Bit-exact checksum of the parameter tensors (one kernel + one 8-byte read-back)."""
        n = len(params)
        cache = getattr(self, "_fp_cache", None)
        key = tuple(p.data_ptr() for p in params)
        if cache is None or cache[0] != key:
            ptrs = (ctypes.c_void_p * n)(*[p.data_ptr() for p in params])
            counts = (ctypes.c_int64 * n)(*[p.numel() for p in params])
            out = torch.zeros(1, dtype=torch.int64, device=device)
            cache = (key, ptrs, counts, out)
            self._fp_cache = cache
        _, ptrs, counts, out = cache
        with torch.cuda.device(device):
            _check(self.lib.mtadgat_params_fingerprint(ptrs, counts, n, ctypes.c_void_p(out.data_ptr()), _stream()), "fingerprint")
        return int(out.item())

    def fingerprint_async(self, params, device):
        """The same checksum without a host wait: the kernel and an 8-byte copy into pinned host memory are enqueued on a side
        stream that starts where the current stream is now; returns a function that waits for THAT copy (an event, not a
        stream: the caller's work keeps running) and returns the value."""
        n = len(params)
        cache = getattr(self, "_fp_cache", None)
        key = tuple(p.data_ptr() for p in params)
        if cache is None or cache[0] != key:
            ptrs = (ctypes.c_void_p * n)(*[p.data_ptr() for p in params])
            counts = (ctypes.c_int64 * n)(*[p.numel() for p in params])
            out = torch.zeros(1, dtype=torch.int64, device=device)
            cache = (key, ptrs, counts, out)
            self._fp_cache = cache
        _, ptrs, counts, out = cache
        ring = getattr(self, "_fp_ring", None)
        if ring is None:
            ring = self._fp_ring = [[torch.zeros(1, dtype=torch.int64).pin_memory(), torch.cuda.Event(), torch.cuda.Event()] for _ in range(4)]
            self._fp_slot = 0
            self._fp_stream = torch.cuda.Stream(device)
        self._fp_slot = (self._fp_slot + 1) % len(ring)
        pin, ev, ev0 = ring[self._fp_slot]
        # on a side stream that starts where the caller's stream is now: the check runs beside the call's first kernels instead of
        # in front of them.  (The caller waits for `ev` before it returns -- _finish_weight_check -- so nothing the caller enqueues
        # after this call can overtake the read of the parameters.)
        with torch.cuda.device(device):
            cur = torch.cuda.current_stream()
            ev0.record(cur)
            side = self._fp_stream
            side.wait_event(ev0)
            with torch.cuda.stream(side):
                _check(self.lib.mtadgat_params_fingerprint(ptrs, counts, n, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(side.cuda_stream)), "fingerprint")
                pin.copy_(out, non_blocking=True)
                ev.record(side)

        def wait():
            ev.synchronize()
            return int(pin[0])
        return wait

    def read_packed(self, device):
        """Diagnostic: the packed weight image as a CPU tensor."""
        n = self.lib.mtadgat_packed_floats(self.handle)
        out = _empty(n, dtype=torch.float32)
        with torch.cuda.device(device):
            dst = ctypes.cast(out.data_ptr(), ctypes.POINTER(ctypes.c_float))
            _check(self.lib.mtadgat_read_packed(self.handle, dst, n, _stream()), "read_packed")
        return out

    def derived_regions(self):
        """(offset, length) pairs in floats of the image regions derived on the device from other regions (split packs)."""
        n = self.lib.mtadgat_derived_regions(self.handle, None, 0)
        buf = (ctypes.c_int64 * (2 * n))()
        n = self.lib.mtadgat_derived_regions(self.handle, buf, n)
        return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n)]

    def split_steps(self):
        """The steps that derive the split packs (host only), in group then step order: dicts of the ten fields of
        mtadgat_split_steps (include/mtadgat.h), the op as its name (SPLIT_OPS)."""
        return split_steps(self.lib, self.handle)

    def split_n_infer(self):
        """Groups [0, n) of split_steps() are the ones an inference call may read; the rest are the training backward's."""
        return int(self.lib.mtadgat_split_n_infer(self.handle))

    def derive_split_packs(self, device):
        """Diagnostic: derive every split group, the backward's included, on the current stream (read_packed derives the
        inference groups only)."""
        with torch.cuda.device(device):
            _check(self.lib.mtadgat_derive_split_packs(self.handle, _stream()), "derive_split_packs")

    def gru_route(self, stack, layer, n, training=False, compute_units=256):
        """Which kernels run recurrence layer `layer` of the GRU stack (stack 0) or the decoder (1) at n windows, under the current
        precision and "gru_kernel" option (host only): dict of the eight integers of mtadgat_gru_route (include/mtadgat.h)."""
        buf = (ctypes.c_int * 8)()
        _check(self.lib.mtadgat_gru_route(self.handle, stack, layer, n, int(training), compute_units, buf), "mtadgat_gru_route")
        return dict(zip(GRU_ROUTE_FIELDS, (int(v) for v in buf)))

    def front_route(self, kind, source, n, facts=7):
        """Which kernels run the convolution and the two attention layers of a call of FRONT_KINDS[kind] on n windows from
        FRONT_SOURCES[source], under the current precision and options (host only): dict of the 14 integers of
        mtadgat_front_route (include/mtadgat.h)."""
        buf = (ctypes.c_int * 14)()
        _check(self.lib.mtadgat_front_route(self.handle, kind, source, n, facts, buf), "mtadgat_front_route")
        return dict(zip(FRONT_ROUTE_FIELDS, (int(v) for v in buf)))

    def forward_plan(self, batch):
        """How forward() walks a call of `batch` windows under the current chunk size, precision and "lanes" option (host only):
        dict of fork, lane_floats (2), total_floats and pieces [(first window, windows, lane)] -- mtadgat_forward_plan (include/mtadgat.h)."""
        n = 5 + 3 * min(int(batch), 64)
        while True:                                              # (no piece is empty: 5 + 3 * batch values always suffice)
            buf = (ctypes.c_int64 * n)()
            got = self.lib.mtadgat_forward_plan(self.handle, int(batch), buf, n)
            if got > 0 or n >= 5 + 3 * batch:
                break
            n = min(8 * n, 5 + 3 * int(batch))
        if got <= 0:
            _check(got, "mtadgat_forward_plan")
        v = [int(x) for x in buf[:got]]
        return dict(fork=bool(v[1]), lane_floats=(v[2], v[3]), total_floats=v[4], pieces=[tuple(v[i:i + 3]) for i in range(5, got, 3)])

    def train_route(self, n):
        """Which kernels run the recurrence and attention layers of a training step of n windows under the current precision and
        "gru_kernel" option (host only) -- mtadgat_train_route (include/mtadgat.h): dict of gru / rec [(forward kernel, backward
        kernel, x3) per layer], rec_fc_rides, feat / temp (wide, v1)."""
        lg, ld = self.cfg.gru_n_layers, self.cfg.recon_n_layers
        cap = 3 * (lg + ld) + 5
        buf = (ctypes.c_int * cap)()
        got = self.lib.mtadgat_train_route(self.handle, int(n), buf, cap)
        if got != cap:
            _check(got or -1, "mtadgat_train_route")
        v = [int(x) for x in buf]
        layers = [tuple(v[3 * i:3 * i + 3]) for i in range(lg + ld)]
        return dict(gru=layers[:lg], rec=layers[lg:], rec_fc_rides=v[-5], feat=tuple(v[-4:-2]), temp=tuple(v[-2:]))

    def wgrad_sites(self):
        """Names of the weight-gradient sites of a training step in mtadgat_wgrad_plan's order."""
        c = self.cfg
        names = ["conv"] + (["feat_lin", "temp_lin"] if c.use_gatv2 else [])
        for stack, layers in (("gru", c.gru_n_layers), ("rec", c.recon_n_layers)):
            for l in range(layers):
                names += [f"{stack}{l}_ih", f"{stack}{l}_hh"]
        return names + ["rec_fc"] + [f"fc{i}" for i in range(c.forecast_n_linear)]

    def wgrad_plan(self, n):
        """How the weight-gradient GEMMs of a backward of n windows (one chunk of the training step) are laid out under the
        current precision and "wgrad_kernel" option (host only) -- mtadgat_wgrad_plan (include/mtadgat.h): {site name: dict of
        WGRAD_PLAN_FIELDS}, sites in the library's order (wgrad_sites)."""
        names = self.wgrad_sites()
        k = len(WGRAD_PLAN_FIELDS)
        cap = k * len(names)
        buf = (ctypes.c_int64 * cap)()
        got = self.lib.mtadgat_wgrad_plan(self.handle, int(n), buf, cap)
        if got != cap:
            _check(got if got < 0 else -1, "mtadgat_wgrad_plan")
        return {name: dict(zip(WGRAD_PLAN_FIELDS, (int(v) for v in buf[k * i:k * i + k]))) for i, name in enumerate(names)}

    def load_weights(self, sd, device, allow_device_pack=True):
        """sd: reference-format state_dict (any device).  The first load packs on the host and uploads on the current
        stream; later ones (fp32 image, parameters on the GPU) re-pack on the device."""
        if allow_device_pack and self.update_weights_device(sd, device):
            return
        # one device-side concatenation + one transfer instead of a copy (and a sync) per tensor
        keys = list(sd.keys())
        flat = torch.cat([sd[k].detach().reshape(-1).to(torch.float32) for k in keys]).cpu()
        host, off = {}, 0
        for k in keys:
            n = sd[k].numel()
            host[k] = flat[off:off + n]
            off += n
        p = Params()

        def ptr(key):
            return ctypes.c_void_p(host[key].data_ptr())

        p.conv_weight, p.conv_bias = ptr("conv.conv.weight"), ptr("conv.conv.bias")
        p.feat_lin_weight, p.feat_lin_bias = ptr("feature_gat.lin.weight"), ptr("feature_gat.lin.bias")
        p.feat_a, p.feat_bias = ptr("feature_gat.a"), ptr("feature_gat.bias")
        p.temp_lin_weight, p.temp_lin_bias = ptr("temporal_gat.lin.weight"), ptr("temporal_gat.lin.bias")
        p.temp_a, p.temp_bias = ptr("temporal_gat.a"), ptr("temporal_gat.bias")
        for l in range(self.cfg.gru_n_layers):
            p.gru_w_ih[l], p.gru_w_hh[l] = ptr(f"gru.gru.weight_ih_l{l}").value, ptr(f"gru.gru.weight_hh_l{l}").value
            p.gru_b_ih[l], p.gru_b_hh[l] = ptr(f"gru.gru.bias_ih_l{l}").value, ptr(f"gru.gru.bias_hh_l{l}").value
        for i in range(self.cfg.forecast_n_linear):
            p.fc_weight[i] = ptr(f"forecasting_model.layers.{i}.weight").value
            p.fc_bias[i] = ptr(f"forecasting_model.layers.{i}.bias").value
        for l in range(self.cfg.recon_n_layers):
            pre = "recon_model.decoder.rnn."
            p.rec_w_ih[l], p.rec_w_hh[l] = ptr(f"{pre}weight_ih_l{l}").value, ptr(f"{pre}weight_hh_l{l}").value
            p.rec_b_ih[l], p.rec_b_hh[l] = ptr(f"{pre}bias_ih_l{l}").value, ptr(f"{pre}bias_hh_l{l}").value
        p.rec_fc_weight, p.rec_fc_bias = ptr("recon_model.fc.weight"), ptr("recon_model.fc.bias")
        with torch.cuda.device(device):
            _check(self.lib.mtadgat_load_weights(self.handle, ctypes.byref(p), _stream()), "load_weights")
        self._keep = flat

    # -- scratch ------------------------------------------------------------------------------
    def _workspace(self, batch, device):
        need = self.lib.mtadgat_workspace_bytes(self.handle, batch)
        ws = self._ws
        if ws is None or ws.device != device or ws.numel() * 4 < need:
            self._ws = None
            ws = _empty((need + 3) // 4, dtype=torch.float32, device=device)
            self._ws = ws
        if _POISON_SCRATCH:
            ws.fill_(_POISON_VALUE)
        return ws, need

    def set_precision(self, mode):
        """0 / False: fp32 MFMA operands (<= 1e-5 parity); 1 / True: bf16 MFMA operands, fp32 accumulation / state
        (<= 2e-2); 2: fp32-class results through split-bf16 operands on the large-batch kernels (<= 1e-5)."""
        _check(self.lib.mtadgat_set_precision(self.handle, int(mode)), "set_precision")

    def bf16_ready(self):
        return bool(self.lib.mtadgat_bf16_ready(self.handle))

    def set_option(self, name, value):
        """Testing / measurement hook (include/mtadgat.h): e.g. ("gru_kernel", 0 automatic | 1 tile-major | 2 chunk-major | 3 hidden-tile split on split operands)."""
        _check(self.lib.mtadgat_set_option(self.handle, name.encode(), int(value)), "set_option")

    def last_conv_max(self, batch, device):
        """Largest convolution output of the last forward of `batch` windows (range guard of the fp16 operand pieces);
        synchronises the current stream."""
        if self._ws is None:
            return 0.0
        out = ctypes.c_float(0.0)
        with torch.cuda.device(device):
            _check(self.lib.mtadgat_last_conv_max(self.handle, ctypes.c_void_p(self._ws.data_ptr()), int(batch), ctypes.byref(out), _stream()),
                   "last_conv_max")
        return float(out.value)

    def chunk_windows(self):
        return int(self.lib.mtadgat_chunk_windows(self.handle))

    def set_chunk_windows(self, n):
        _check(self.lib.mtadgat_set_chunk_windows(self.handle, int(n)), "set_chunk_windows")
        self._ws = None

    def _call(self, fn, what, device, *args):
        with torch.cuda.device(device):
            _check(fn(self.handle, *args, _stream()), what)

    # -- forward ------------------------------------------------------------------------------
    def forward(self, x, want_hend=False):
        c = self.cfg
        b = x.shape[0]
        fn = self.lib.mtadgat_forward
        if x.dtype == torch.bfloat16:       # read directly by the convolution: no fp32 copy of the batch
            if x.device.type != "cuda" or not x.is_contiguous() or tuple(x.shape) != (b, c.window_size, c.n_features):
                raise RuntimeError("bfloat16 input must be a contiguous (b, W, F) tensor on the GPU")
            xp, fn = ctypes.c_void_p(x.data_ptr()), self.lib.mtadgat_forward_xbf16
        else:
            xp = _dev_ptr(x, "x", (b, c.window_size, c.n_features))
        preds = _empty((b, c.out_dim), dtype=torch.float32, device=x.device)
        recons = _empty((b, c.window_size, c.out_dim), dtype=torch.float32, device=x.device)
        hend = _empty((b, c.gru_hid_dim), dtype=torch.float32, device=x.device) if want_hend else None
        ws, need = self._workspace(b, x.device)
        self._call(fn, "forward", x.device, xp, b, _dev_ptr(preds, "preds"),
                   _dev_ptr(recons, "recons"), _dev_ptr(hend, "hend") if want_hend else None,
                   _dev_ptr(ws, "workspace"), need)
        return (preds, recons, hend) if want_hend else (preds, recons)

    def _series_windows(self, series, starts, start0, stride, count):
        """(series pointer, n_rows, starts pointer or None, window count) of a series call, checked on the host."""
        c = self.cfg
        if series.dim() != 2 or series.shape[1] != c.n_features:
            raise RuntimeError(f"series must have shape (n_rows, {c.n_features}), got {tuple(series.shape)}")
        sp = _dev_ptr(series, "series")
        n_rows = series.shape[0]
        if starts is not None:
            if starts.dtype != torch.int64 or starts.device != series.device or not starts.is_contiguous() or starts.dim() != 1:
                raise RuntimeError("starts must be a contiguous 1-D int64 tensor on the series' device")
            b = starts.shape[0]
            if b and (int(starts.min()) < 0 or int(starts.max()) + c.window_size > n_rows):
                raise RuntimeError("a window does not lie inside the series")
            stp = ctypes.c_void_p(starts.data_ptr())
        else:
            b = count if count is not None else max(0, (n_rows - c.window_size - start0) // max(stride, 1) + 1)
            stp = None
        return sp, n_rows, stp, b

    def forward_series(self, series, starts=None, start0=0, stride=1, count=None, want_recons=True, want_last=False):
        """Windows gathered on the GPU from the device-resident series (n_rows, F); returns
        (preds, recons or None, recons[:, -1] or None)."""
        c = self.cfg
        sp, n_rows, stp, b = self._series_windows(series, starts, start0, stride, count)
        dev = series.device
        preds = _empty((b, c.out_dim), dtype=torch.float32, device=dev)
        recons = _empty((b, c.window_size, c.out_dim), dtype=torch.float32, device=dev) if want_recons else None
        last = _empty((b, c.out_dim), dtype=torch.float32, device=dev) if want_last else None
        ws, need = self._workspace(b, dev)
        self._call(self.lib.mtadgat_forward_series, "forward_series", dev, sp, n_rows, stp, int(start0), int(stride), b,
                   _dev_ptr(preds, "preds"), _dev_ptr(recons, "recons") if want_recons else None,
                   _dev_ptr(last, "recons_last") if want_last else None, _dev_ptr(ws, "workspace") if b else None, need)
        return preds, recons, last

    # -- attention maps (eval mode, fp32 in every precision mode) -----------------------------------------
    def _attention_ws(self, batch, reduce, device):
        """Scratch of an attention call: its own buffer (the forward's workspace is sized differently), poisoned like it."""
        need = self.lib.mtadgat_attention_workspace_bytes(self.handle, batch, 1 if reduce else 0)
        return _empty((need + 3) // 4, dtype=torch.float32, device=device), need

    def _attention_out(self, b, reduce, feat, temp, device):
        c = self.cfg
        lead = () if reduce else (b,)
        af = _empty(lead + (c.n_features, c.n_features), dtype=torch.float32, device=device) if feat else None
        at = _empty(lead + (c.window_size, c.window_size), dtype=torch.float32, device=device) if temp else None
        return af, at

    def attention(self, x, reduce=False, feat=True, temp=True):
        """Attention matrices of the windows x (b, W, F): per window ((b, F, F), (b, W, W)) or, reduce=True, their means
        ((F, F), (W, W)); a layer not asked for (feat / temp False) comes back as None."""
        c = self.cfg
        b = x.shape[0]
        xp = _dev_ptr(x, "x", (b, c.window_size, c.n_features))
        af, at = self._attention_out(b, reduce, feat, temp, x.device)
        if b == 0 and not reduce:
            return af, at
        ws, need = self._attention_ws(b, reduce, x.device)
        fn = self.lib.mtadgat_attention_mean if reduce else self.lib.mtadgat_attention
        self._call(fn, "attention", x.device, xp, b, _dev_ptr(af, "att_feat") if feat else None,
                   _dev_ptr(at, "att_temp") if temp else None, _dev_ptr(ws, "workspace"), need)
        return af, at

    def attention_series(self, series, starts=None, start0=0, stride=1, count=None, reduce=True, feat=True, temp=True):
        """attention() over the windows of forward_series(), gathered from the device-resident series."""
        sp, n_rows, stp, b = self._series_windows(series, starts, start0, stride, count)
        dev = series.device
        af, at = self._attention_out(b, reduce, feat, temp, dev)
        if b == 0 and not reduce:
            return af, at
        ws, need = self._attention_ws(b, reduce, dev)
        fn = self.lib.mtadgat_attention_series_mean if reduce else self.lib.mtadgat_attention_series
        self._call(fn, "attention_series", dev, sp, n_rows, stp, int(start0), int(stride), b,
                   _dev_ptr(af, "att_feat") if feat else None, _dev_ptr(at, "att_temp") if temp else None,
                   _dev_ptr(ws, "workspace") if b else None, need)
        return af, at

    # -- forecast / reconstruction errors of a series (Trainer.evaluate's reduction, chunk by chunk) -----------------------
    def series_losses_chunk(self):
        """Windows per chunk of series_losses (mtadgat_series_losses_chunk)."""
        return int(self.lib.mtadgat_series_losses_chunk(self.handle))

    def series_losses_workspace_bytes(self, batch):
        return int(self.lib.mtadgat_series_losses_workspace_bytes(self.handle, int(batch)))

    def series_losses(self, series, starts=None, start0=0, stride=1, count=None, dims=None, age=None, max_age=0):
        """Squared errors of the windows of forward_series() against the series itself, the (b, W, out) reconstructions never
        leaving the library's workspace: (window_sse (b, 2) float64 -- forecast against row s_w + W, reconstruction against rows
        s_w .. s_w + W - 1 --, dim_sse (2, out_dim) float64).  dims: int32 device tensor of the out_dim series columns compared
        with (None: 0 .. out_dim - 1).  count defaults to the windows whose target row exists.
        age (int32 (n_rows, F) on the series' device; observed iff age <= max_age): mtadgat_series_losses_masked, the results are
        (b, 4) = (S_f, S_r, N_f, N_r) per window and (4, out_dim) per dimension, sums and counts over the observed samples."""
        c = self.cfg
        W = c.window_size
        if starts is None and count is None:
            count = max(0, (series.shape[0] - 1 - W - start0) // max(stride, 1) + 1)
        sp, n_rows, stp, b = self._series_windows(series, starts, start0, stride, count)
        if b < 1:
            raise RuntimeError("series_losses needs at least one window with a target row")
        if starts is not None and int(starts.max()) + W > n_rows - 1:
            raise RuntimeError("a window's target row does not lie inside the series")
        dev = series.device
        if dims is not None:
            if dims.dtype != torch.int32 or dims.device != dev or not dims.is_contiguous() or tuple(dims.shape) != (c.out_dim,):
                raise RuntimeError(f"dims must be a contiguous int32 tensor of {c.out_dim} columns on the series' device")
        dp = ctypes.c_void_p(dims.data_ptr()) if dims is not None else None
        if age is None:
            wsse = _empty((b, 2), dtype=torch.float64, device=dev)
            dsse = _empty((2, c.out_dim), dtype=torch.float64, device=dev)
            need = self.series_losses_workspace_bytes(b)
            ws = _empty((need + 3) // 4, dtype=torch.float32, device=dev)
            self._call(self.lib.mtadgat_series_losses, "series_losses", dev, sp, n_rows, stp, int(start0), int(stride), b,
                       dp, ctypes.c_void_p(wsse.data_ptr()), ctypes.c_void_p(dsse.data_ptr()), _dev_ptr(ws, "workspace"), need)
            return wsse, dsse
        ap, lda = _age_rows(age, n_rows, c.n_features, dev)
        wsse = _empty((b, 4), dtype=torch.float64, device=dev)
        dsse = _empty((4, c.out_dim), dtype=torch.float64, device=dev)
        need = int(self.lib.mtadgat_series_losses_masked_workspace_bytes(self.handle, b))
        ws = _empty((need + 3) // 4, dtype=torch.float32, device=dev)
        self._call(self.lib.mtadgat_series_losses_masked, "series_losses", dev, sp, n_rows, stp, int(start0), int(stride), b,
                   dp, ap, lda, int(max_age), ctypes.c_void_p(wsse.data_ptr()), ctypes.c_void_p(dsse.data_ptr()), _dev_ptr(ws, "workspace"), need)
        return wsse, dsse

    def conv(self, x):
        c = self.cfg
        b = x.shape[0]
        xp = _dev_ptr(x, "x", (b, c.window_size, c.n_features))
        y = _empty_like(x)
        self._call(self.lib.mtadgat_conv, "conv", x.device, xp, b, _dev_ptr(y, "y"), None, 0)
        return y

    def gat(self, which, xc):
        c = self.cfg
        b = xc.shape[0]
        xp = _dev_ptr(xc, "x", (b, c.window_size, c.n_features))
        y = _empty_like(xc)
        ws, need = self._workspace(b, xc.device)
        self._call(self.lib.mtadgat_gat, "gat", xc.device, which, xp, b, _dev_ptr(y, "y"), _dev_ptr(ws, "workspace"), need)
        return y

    def gru(self, hcat):
        c = self.cfg
        b = hcat.shape[0]
        xp = _dev_ptr(hcat, "h_cat", (b, c.window_size, 3 * c.n_features))
        hend = _empty((b, c.gru_hid_dim), dtype=torch.float32, device=hcat.device)
        ws, need = self._workspace(b, hcat.device)
        self._call(self.lib.mtadgat_gru, "gru", hcat.device, xp, b, _dev_ptr(hend, "h_end"), _dev_ptr(ws, "workspace"), need)
        return hend

    def heads(self, hend, want_preds=True, want_recons=True):
        c = self.cfg
        b = hend.shape[0]
        hp = _dev_ptr(hend, "h_end", (b, c.gru_hid_dim))
        preds = _empty((b, c.out_dim), dtype=torch.float32, device=hend.device) if want_preds else None
        recons = _empty((b, c.window_size, c.out_dim), dtype=torch.float32, device=hend.device) if want_recons else None
        ws, need = self._workspace(b, hend.device)
        self._call(self.lib.mtadgat_heads, "heads", hend.device, hp, b,
                   _dev_ptr(preds, "preds") if want_preds else None,
                   _dev_ptr(recons, "recons") if want_recons else None, _dev_ptr(ws, "workspace"), need)
        return preds, recons

    # -- per-kernel timing (bench.py) ------------------------------------------------------------
    def profile_enable(self, on=True):
        _check(self.lib.mtadgat_profile_enable(self.handle, 1 if on else 0), "profile_enable")

    def profile_read(self):
        ms = (ctypes.c_double * PROFILE_SLOTS)()
        n = (ctypes.c_int64 * PROFILE_SLOTS)()
        _check(self.lib.mtadgat_profile_read(self.handle, ms, n), "profile_read")
        return {self.lib.mtadgat_profile_name(i).decode(): (ms[i], n[i]) for i in range(PROFILE_SLOTS)}
