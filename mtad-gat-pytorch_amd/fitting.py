"""Training from a series that lives on the GPU: `SeriesTrainer`, the training half of the loop whose validation half is
`MTAD_GAT.series_losses`.

The reference's `Trainer.fit` (training.py:100-130) feeds each batch from a CPU `SlidingWindowDataset` / `DataLoader`, copies it to
the device, forms the loss `sqrt(mse) + sqrt(mse)` with half a dozen torch kernels under autograd and steps `torch.optim.Adam`
tensor by tensor; the module then concatenates the ~30 parameter tensors to re-pack the kernels' weights.  Here a step is a fixed
sequence of the library's calls on one flat parameter buffer, fed by window starts into the device series:

    zero the flat gradients | mtadgat_fit_gather | mtadgat_forward_train | mtadgat_eval_window_sse, mtadgat_eval_group_sums |
    mtadgat_fit_loss_grad | mtadgat_backward | mtadgat_fit_prepare | mtadgat_fit_adam | mtadgat_update_weights_device

`step` returns nothing and reads nothing from the device; losses, gradient norms and skipped steps are appended to a ring on the
device that `losses()` / `fit()` copy once per epoch.  tests/fit_refs.py specifies the new kernels' arithmetic.

Three departures from the reference and torch, all deliberate:
  * Adam's arithmetic is float64 per element on float32 state, each result rounded once (torch rounds to float32 after every
    operation): parameters differ from torch.optim.Adam's in the last bits.
  * A head whose residuals are all zero (rmse == 0) contributes a zero gradient; autograd's sqrt gives 0 / 0 there.
  * A step takes at most one training chunk of windows (`_hipgrad._chunk_windows`, 8 192 unless the model is very wide); the
    existing route (`model(x)` + autograd) chunks larger batches.
Series that are several parts laid end to end and hold filled gaps: `training_windows` is the sampler -- the starts whose window and
target row lie in one part, with an observed target and enough observed samples --, and `step` / `fit` with `age` (the
preparation's `transform(..., return_age=True)`) count observed samples only: mtadgat_fit_masked_sse and
mtadgat_fit_masked_loss_grad take the places of mtadgat_eval_window_sse and mtadgat_fit_loss_grad.  tests/fit_mask_refs.py specifies
both.  Without those arguments the calls and the bits are the ones above.
(Not named training.py: the reference's train.py imports a module of that name and this package sits flat on sys.path.)"""
import ctypes
import math

import numpy as np
import torch

import _hipgrad
import _native
import evaluation

_MASK64 = (1 << 64) - 1


def _mix64(z):
    """splitmix64's output function."""
    z = (z + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def _min_count(min_observed, W, F):
    """ceil(min_observed W F), the observed samples a window must hold, formed on the host."""
    if not 0.0 <= float(min_observed) <= 1.0:
        raise ValueError(f"min_observed must lie in [0, 1], got {min_observed!r}")
    return int(math.ceil(float(min_observed) * W * F))


def training_windows(n_rows, window_size, n_features, lengths=None, age=None, max_age=0, min_observed=0.5, target_dims=None, device=None):
    """The window starts a trainer may draw from when the series is several parts laid end to end and has filled gaps: the int64
    device tensor, ascending, of the starts s in [0, n_rows - W) for which
      1. rows s .. s + W lie in one part (lengths: the parts' row counts, as SeriesScaler.transform(lengths=) and score_parts take
         them; None: one part),
      2. the target row s + W has an observed sample among the columns target_dims (None: all),
      3. rows s .. s + W - 1 hold at least ceil(min_observed W F) observed samples over all columns.
    age: int32 (n_rows, F) on the device as SeriesScaler.transform(..., return_age=True) returns it -- 0 for a real sample, k for the
    k-th consecutive filled row; a sample is observed iff age <= max_age.  A boolean mask m of observed samples is
    (~m).to(torch.int32).  None: every sample is observed.  One device call (mtadgat_fit_windows) and one 8-byte host read, of the
    count.  device: where the result lives when neither age nor a device is given, the current GPU."""
    import preparation
    n_rows, W, F = int(n_rows), int(window_size), int(n_features)
    min_count = _min_count(min_observed, W, F)
    if age is not None:
        if not isinstance(age, torch.Tensor) or age.device.type != "cuda":
            raise RuntimeError("age must be an int32 tensor on the GPU (the window sampler is HIP only)")
        asked = None if device is None else torch.device(device)
        if asked is not None and (asked.type != "cuda" or asked.index not in (None, age.device.index)):
            raise RuntimeError(f"age is on {age.device}, the windows were asked for on {device}")
        device = age.device
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if n_rows < W + 1:
        raise ValueError("the series is shorter than a window and its target row")
    dims = None
    if target_dims is not None:
        cols = [target_dims] if isinstance(target_dims, int) else [int(d) for d in target_dims]
        dims = torch.tensor(evaluation._target_dims(cols, len(cols), F), dtype=torch.int32, device=device)
    offsets = None
    if lengths is not None:
        offsets = torch.tensor(preparation._part_offsets(lengths, n_rows), dtype=torch.int64, device=device)
    starts, count = _native.fit_windows(n_rows, W, F, device, age=age, max_age=max_age, dims=dims, offsets=offsets, min_count=min_count)
    return starts[:int(count.item())]


class SeriesTrainer:
    """Adam / AdamW steps of an MTAD_GAT on windows of a device-resident series, on the HIP kernels throughout.

    model: on the GPU, float32 parameters that all require a gradient, a configuration with a HIP backward.  The trainer owns flat
    `params / grads / exp_avg / exp_avg_sq` buffers in the order of `Engine.grad_layout()`; every `nn.Parameter`'s `.data` becomes a
    view of `params`, so parameter identity, `model.state_dict()` and checkpoints keep working and `model(x)` sees each step.
    max_grad_norm: torch's `clip_grad_norm_` (L2 over all parameters) before the step, None for none.  decoupled: AdamW's decay.
    skip_nonfinite: a step whose gradient norm or loss is not finite changes nothing (it is logged with applied = 0).
    seed: of the dropout streams (`step_seed`) and of `fit`'s shuffling; None draws one from torch's CPU generator."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_grad_norm=None,
                 target_dims=None, seed=None, skip_nonfinite=False, log_capacity=4096):
        plist = list(model.parameters())
        if not plist or any(p.device.type != "cuda" for p in plist):
            raise RuntimeError("SeriesTrainer trains on the GPU (MI355X HIP kernels): move the model there first (.cuda() / .to('cuda'))")
        if any(p.dtype != torch.float32 for p in plist):
            raise RuntimeError("SeriesTrainer needs float32 parameters")
        if not all(p.requires_grad for p in plist):
            raise RuntimeError("SeriesTrainer updates every parameter: all of them must require a gradient")
        if not (lr >= 0.0 and math.isfinite(lr)) or not all(0.0 <= b < 1.0 for b in betas) or not eps >= 0.0 or not weight_decay >= 0.0:
            raise ValueError("SeriesTrainer: lr, eps, weight_decay must be finite and >= 0, betas in [0, 1)")
        if max_grad_norm is not None and not max_grad_norm >= 0.0:
            raise ValueError("SeriesTrainer: max_grad_norm must be >= 0 or None")
        if int(log_capacity) < 1:
            raise ValueError("SeriesTrainer: log_capacity must be >= 1")
        self.model = model
        self.device = plist[0].device
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.decoupled = float(weight_decay), bool(decoupled)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.target_dims = target_dims
        self._dims = evaluation._target_dims(target_dims, model.out_dim, model.n_features)
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        self._lib = evaluation._lib()
        eng = model._sync_engine(self.device)
        model._finish_weight_check()
        if not eng.backward_supported():
            raise RuntimeError("SeriesTrainer needs the HIP training step: " + eng.why_not())
        offs, total = eng.grad_layout()
        self._plist = _hipgrad.param_order(model)
        sizes = [p.numel() for p in self._plist]
        if len(offs) != len(sizes) or {id(p) for p in self._plist} != {id(p) for p in plist} or \
                any(o != sum(sizes[:i]) for i, o in enumerate(offs)) or total != sum(sizes):
            raise RuntimeError("SeriesTrainer: the flat gradient layout does not list the model's parameters densely")
        self._spans = list(zip(offs, sizes))
        dev = self.device
        self.params = torch.empty(total, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self.state = torch.zeros(len(_native.FIT_STATE_FIELDS), dtype=torch.float64, device=dev)      # the step record
        self.log = torch.zeros((int(log_capacity), 4), dtype=torch.float64, device=dev)
        self._dims_dev = None if target_dims is None else torch.tensor(self._dims, dtype=torch.int32, device=dev)
        self._generator = torch.Generator(device=dev)
        self._generator.manual_seed(self.seed)
        self._calls = 0                                     # steps taken, applied or not: the host's copy of the record's `calls`
        self._key = None
        self._eng = None
        self._bufs = {}
        self._tape = None
        self.last_preds = self.last_recons = None           # the last step's model outputs (the tests read them)
        self._adopt()

    # -- the flat parameter buffer and the packed weights --------------------------------------------------------------------------
    def _param_key(self):
        return tuple((p.data_ptr(), p._version) for p in self._plist)

    def _adopt(self):
        """Make every parameter a view of `params` (copying in what is not) and re-pack the kernels' weights from it."""
        with torch.no_grad():
            for p, (o, n) in zip(self._plist, self._spans):
                view = self.params[o:o + n].view(p.shape)
                if p.data_ptr() != view.data_ptr():
                    view.copy_(p.detach())
                    p.data = view
        model = self.model
        eng = model._sync_engine(self.device)               # an engine with one host-side load behind it
        model._finish_weight_check()
        self._eng = eng
        self._repack()
        self._key = self._param_key()

    def _repack(self):
        eng, n = self._eng, self.params.numel()
        eng.set_precision(0 if self.model.precision == "fp32_strict" else 2)
        with torch.cuda.device(self.device):
            stream = _native._stream()
            _native._check(self._lib.mtadgat_update_weights_device(eng.handle, ctypes.c_void_p(self.params.data_ptr()), n, stream),
                           "update_weights_device")
        # the module's own entry points re-pack from the parameters when one of them is called next
        object.__setattr__(self.model, "_weights_key", None)

    def _ready(self):
        """The engine with the flat buffer's weights packed.  Host checks only: a parameter that was re-allocated (.to(),
        a `p.data =`) or written in place through torch (load_state_dict: its version counter moved), another engine, or a call of the
        module's own entry points since the last step (it re-packed, perhaps for another arithmetic) make the trainer adopt again."""
        m = self.model
        if self._key != self._param_key() or m._engine is not self._eng or m._weights_key is not None:
            self._adopt()
        return self._eng

    def step_seed(self, k):
        """Seed of step k's dropout masks: a pure function of (seed, k), below 2^62."""
        return _mix64(_mix64(self.seed & _MASK64) ^ (int(k) & _MASK64)) >> 2

    def _buffers(self, b):
        c = self._bufs.get(b)
        if c is None:
            m, dev, e = self.model, self.device, _native._empty
            W, F, out = m.window_size, m.n_features, m.out_dim
            need_sse = self._lib.mtadgat_eval_window_sse_scratch(b, out)
            need_norm = self._lib.mtadgat_fit_prepare_scratch(self.params.numel())
            if need_sse == 0:
                raise ValueError(f"SeriesTrainer: sizes outside the loss kernels' limits (batch {b}, out_dim {out})")
            c = dict(x=e((b, W, F), dtype=torch.float32, device=dev), d_preds=e((b, out), dtype=torch.float32, device=dev),
                     d_recons=e((b, W, out), dtype=torch.float32, device=dev), wsse=e((b, 2), dtype=torch.float64, device=dev),
                     sums=e(2, dtype=torch.float64, device=dev), rmse=e(2, dtype=torch.float64, device=dev),
                     sse_scratch=e((need_sse + 7) // 8, dtype=torch.float64, device=dev),
                     wsse4=None, sums4=None, sse4_scratch=None,                     # the masked step's, made when one is taken
                     norm_scratch=e(max(1, (need_norm + 7) // 8), dtype=torch.float64, device=dev))
            if len(self._bufs) >= 4:                        # a full batch and a short last one, with room for a change of batch size
                self._bufs.pop(next(iter(self._bufs)))
            self._bufs[b] = c
        elif _native._POISON_SCRATCH:
            for t in c.values():
                if t is not None:
                    t.fill_(_native._POISON_VALUE)
        return c

    def _masked_buffers(self, c, b):
        if c["wsse4"] is None:
            dev, e, out = self.device, _native._empty, self.model.out_dim
            need = self._lib.mtadgat_fit_masked_sse_scratch(b, out)
            c["wsse4"] = e((b, 4), dtype=torch.float64, device=dev)
            c["sums4"] = e(4, dtype=torch.float64, device=dev)
            c["sse4_scratch"] = e((need + 7) // 8, dtype=torch.float64, device=dev)
        return c

    # -- one step --------------------------------------------------------------------------------------------------------------------
    def step(self, series, starts, age=None, max_age=0):
        """One optimisation step on the windows series[s : s + W], s in `starts`, each asked to forecast row s + W.
        series: (N, n_features) float32 on the model's GPU, rows contiguous (a column slice keeps its row stride).  starts: int64 on
        the same GPU, 1 .. one training chunk of them, every entry in [0, N - W - 1] -- not checked: that would read the device.
        age: int32 (N, n_features) on the same GPU, as SeriesScaler.transform(..., return_age=True) returns it (a boolean mask m of
        observed samples is (~m).to(torch.int32)): the loss is sqrt(S_f / N_f) + sqrt(S_r / N_r) over the observed samples only,
        age <= max_age -- a filled value is neither a target of the forecast nor of the reconstruction, and its cotangent is 0.
        The step runs mtadgat_fit_masked_sse, mtadgat_eval_group_sums(cols 4) and mtadgat_fit_masked_loss_grad in place of the
        three loss calls; a head without an observed sample in the batch logs rmse 0 and contributes no gradient.  Without age the
        calls and the bits are what they were."""
        m, lib = self.model, self._lib
        W, F, out = m.window_size, m.n_features, m.out_dim
        if not isinstance(series, torch.Tensor) or series.device != self.device or series.dtype != torch.float32 or series.ndim != 2 \
                or series.shape[1] != F or series.stride(1) != 1 or series.stride(0) < F:
            raise RuntimeError(f"series must be a float32 (N, {F}) tensor on {self.device} whose rows are contiguous")
        if series.shape[0] < W + 1:
            raise RuntimeError("the series is shorter than a window and its target row")
        if not isinstance(starts, torch.Tensor) or starts.device != self.device or starts.dtype != torch.int64 or starts.ndim != 1 \
                or not starts.is_contiguous():
            raise RuntimeError(f"starts must be a contiguous 1-D int64 tensor on {self.device}")
        agep = None
        if age is not None:
            agep, ld_age = _native._age_rows(age, series.shape[0], F, self.device)
        eng = self._ready()
        b = starts.numel()
        limit = _hipgrad._chunk_windows(eng, self.device)
        if b < 1 or b > limit:
            raise ValueError(f"a step takes 1 .. {limit} windows (one training chunk), got {b}")
        eng.set_precision(0 if m.precision == "fp32_strict" else 2)      # a bf16 request trains on the fp32 step
        p = float(m.dropout_p) if m.training else 0.0
        seed = self.step_seed(self._calls)
        c = self._buffers(b)
        n_rows, ld = series.shape[0], series.stride(0)
        vp = ctypes.c_void_p
        sp, stp = vp(series.data_ptr()), vp(starts.data_ptr())
        dims = None if self._dims_dev is None else vp(self._dims_dev.data_ptr())
        with torch.cuda.device(self.device):
            stream = _native._stream()
            self.grads.zero_()
            _native._check(lib.mtadgat_fit_gather(sp, n_rows, F, ld, stp, b, W, vp(c["x"].data_ptr()), stream), "fit_gather")
            preds, recons, self._tape = eng.forward_train(c["x"], p, seed, 0, tape=self._tape)
            if agep is not None:
                c = self._masked_buffers(c, b)
                _native._check(lib.mtadgat_fit_masked_sse(vp(preds.data_ptr()), vp(recons.data_ptr()), b, W, out, sp, n_rows, F, ld, stp, 0, 0,
                                                          dims, agep, ld_age, int(max_age), 0, vp(c["wsse4"].data_ptr()), None,
                                                          vp(c["sse4_scratch"].data_ptr()), c["sse4_scratch"].numel() * 8, stream),
                               "fit_masked_sse")
                _native._check(lib.mtadgat_eval_group_sums(vp(c["wsse4"].data_ptr()), b, 4, b, vp(c["sums4"].data_ptr()), stream),
                               "eval_group_sums")
                _native._check(lib.mtadgat_fit_masked_loss_grad(vp(preds.data_ptr()), vp(recons.data_ptr()), b, W, out, sp, n_rows, F, ld, stp,
                                                                dims, agep, ld_age, int(max_age), vp(c["sums4"].data_ptr()),
                                                                vp(c["d_preds"].data_ptr()), vp(c["d_recons"].data_ptr()),
                                                                vp(c["rmse"].data_ptr()), stream), "fit_masked_loss_grad")
            else:
                _native._check(lib.mtadgat_eval_window_sse(vp(preds.data_ptr()), vp(recons.data_ptr()), b, W, out, sp, n_rows, F, ld, stp, 0, 0,
                                                           dims, 0, vp(c["wsse"].data_ptr()), None, vp(c["sse_scratch"].data_ptr()),
                                                           c["sse_scratch"].numel() * 8, stream), "eval_window_sse")
                _native._check(lib.mtadgat_eval_group_sums(vp(c["wsse"].data_ptr()), b, 2, b, vp(c["sums"].data_ptr()), stream),
                               "eval_group_sums")
                _native._check(lib.mtadgat_fit_loss_grad(vp(preds.data_ptr()), vp(recons.data_ptr()), b, W, out, sp, n_rows, F, ld, stp, dims,
                                                         vp(c["sums"].data_ptr()), vp(c["d_preds"].data_ptr()), vp(c["d_recons"].data_ptr()),
                                                         vp(c["rmse"].data_ptr()), stream), "fit_loss_grad")
            eng.backward(c["x"], p, seed, c["d_preds"], c["d_recons"], self._tape, self.grads, 0)
            _native.fit_prepare(self.grads, c["rmse"], self.state, self.log, self.lr, self.betas, self.max_grad_norm, self.skip_nonfinite,
                                scratch=c["norm_scratch"])
            _native.fit_adam(self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.state, self.lr, self.betas, self.eps,
                             self.weight_decay, self.decoupled)
            _native._check(lib.mtadgat_update_weights_device(eng.handle, vp(self.params.data_ptr()), self.params.numel(), stream),
                           "update_weights_device")
        self._calls += 1
        self.last_preds, self.last_recons = preds, recons

    # -- epochs ----------------------------------------------------------------------------------------------------------------------
    def losses(self, last=None):
        """The log's rows of the last `last` steps (all it still holds when None), oldest first, as a numpy (k, 4) float64 array:
        _native.FIT_LOG_FIELDS = (rmse_forecast, rmse_recon, gradient norm, applied).  One device copy."""
        cap = self.log.shape[0]
        k = min(self._calls, cap) if last is None else int(last)
        if k < 0 or k > min(self._calls, cap):
            raise ValueError(f"the log holds the last {min(self._calls, cap)} steps, asked for {k}")
        log = self.log.cpu().numpy()
        return log[[(self._calls - k + i) % cap for i in range(k)]]

    def fit(self, train_series, val_series=None, epochs=1, batch_size=256, shuffle=True, lengths=None, age=None, val_lengths=None,
            val_age=None, max_age=0, min_observed=0.5):
        """The reference's Trainer.fit over a device series: per epoch the windows 0 .. N - W - 1 in consecutive batches of
        `batch_size` (the short last batch kept) of a device `torch.randperm` (shuffle) or in order.  The epoch's losses are the
        reference's sqrt(mean over the batches of rmse^2) per head, read from the log once per epoch; validation, when val_series is
        given, is model.series_losses(val_series, target_dims=, batch_size=).  Returns the dict of lists of Trainer.losses:
        train_forecast, train_recon, train_total, val_forecast, val_recon, val_total.
        lengths (the row counts of the parts laid end to end in train_series) and / or age (int32 (N, F), as
        SeriesScaler.transform(..., return_age=True) returns it; a boolean mask m of observed samples is (~m).to(torch.int32)): the
        windows are training_windows(N, W, F, lengths, age, max_age, min_observed, target_dims), found once per call -- none
        straddles two parts, asks for an unobserved target row or holds fewer than min_observed of its samples observed --, an
        epoch's order is windows[randperm(count)] or the windows in order, its step count follows their number, and every step
        takes `age`: filled samples count for nothing in either loss.  val_lengths / val_age: the same for val_series, whose losses
        are then model.series_losses(val_series, starts=<its windows>, age=val_age, max_age=)."""
        W = self.model.window_size
        batch_size = int(batch_size)
        windows = None
        if lengths is not None or age is not None:
            windows = training_windows(train_series.shape[0], W, self.model.n_features, lengths, age, max_age, min_observed,
                                       self.target_dims, self.device)
            n = windows.numel()
            if n < 1:
                raise ValueError("fit: no window lies in one part with an observed target row and enough observed samples")
        else:
            n = train_series.shape[0] - W
        if n < 1 or batch_size < 1:
            raise ValueError("fit needs at least one window with a target row and batch_size >= 1")
        val_windows = None
        if val_series is not None and (val_lengths is not None or val_age is not None):
            val_windows = training_windows(val_series.shape[0], W, self.model.n_features, val_lengths, val_age, max_age, min_observed,
                                           self.target_dims, self.device)
            if val_windows.numel() < 1:
                raise ValueError("fit: no validation window lies in one part with an observed target row and enough observed samples")
        steps = (n + batch_size - 1) // batch_size
        if steps > self.log.shape[0]:
            raise ValueError(f"an epoch of {steps} steps does not fit the log (log_capacity={self.log.shape[0]})")
        out = {k: [] for k in ("train_forecast", "train_recon", "train_total", "val_forecast", "val_recon", "val_total")}
        for _ in range(int(epochs)):
            if shuffle:
                order = torch.randperm(n, device=self.device, generator=self._generator)
            else:
                order = torch.arange(n, device=self.device)
            if windows is not None:
                order = windows[order]
            for lo in range(0, n, batch_size):
                if age is None:
                    self.step(train_series, order[lo:lo + batch_size])
                else:
                    self.step(train_series, order[lo:lo + batch_size], age=age, max_age=max_age)
            rows = self.losses(last=steps)
            with np.errstate(over="ignore", invalid="ignore"):
                f, r = (float(np.sqrt(np.mean(rows[:, j] ** 2))) for j in (0, 1))
            out["train_forecast"].append(f)
            out["train_recon"].append(r)
            out["train_total"].append(f + r)
            if val_series is not None:
                if val_windows is None:
                    vf, vr, vt = self.model.series_losses(val_series, target_dims=self.target_dims, batch_size=batch_size)
                else:
                    vf, vr, vt = self.model.series_losses(val_series, target_dims=self.target_dims, batch_size=batch_size,
                                                          starts=val_windows, age=val_age, max_age=max_age)
                out["val_forecast"].append(vf)
                out["val_recon"].append(vr)
                out["val_total"].append(vt)
        return out

    # -- checkpoints -----------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """The optimiser's side of a checkpoint (the parameters are the model's): with model.state_dict() a run resumes bit for bit."""
        return dict(exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(), state=self.state.clone(), log=self.log.clone(),
                    calls=self._calls, seed=self.seed, generator_state=self._generator.get_state(),
                    hyper=dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, decoupled=self.decoupled,
                               max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite, target_dims=self.target_dims))

    def load_state_dict(self, sd):
        if sd["exp_avg"].numel() != self.exp_avg.numel() or sd["log"].shape != self.log.shape:
            raise RuntimeError("SeriesTrainer.load_state_dict: the checkpoint is of another model or log capacity")
        h = sd["hyper"]
        dims = evaluation._target_dims(h["target_dims"], self.model.out_dim, self.model.n_features)
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.state.copy_(sd["state"])
        self.log.copy_(sd["log"])
        self._calls, self.seed = int(sd["calls"]), int(sd["seed"])
        self._generator.set_state(sd["generator_state"])
        self.lr, self.betas, self.eps = float(h["lr"]), (float(h["betas"][0]), float(h["betas"][1])), float(h["eps"])
        self.weight_decay, self.decoupled = float(h["weight_decay"]), bool(h["decoupled"])
        self.max_grad_norm, self.skip_nonfinite = h["max_grad_norm"], bool(h["skip_nonfinite"])
        self.target_dims, self._dims = h["target_dims"], dims
        self._dims_dev = None if self.target_dims is None else torch.tensor(dims, dtype=torch.int32, device=self.device)
