"""Drop-in `mtad_gat` module: `MTAD_GAT` with the reference's constructor, parameter
names and `forward(x) -> (predictions, recons)` contract (reference
`mtad_gat.py:14-79`), whose forward pass runs on hand-written HIP kernels for
MI355X (gfx950) through the C ABI in `include/mtadgat.h`.

Put this directory ahead of the reference on `sys.path` and the reference's own
`train.py` / `predict.py` pick it up through `from mtad_gat import MTAD_GAT`
(`train.py:7`, `predict.py:7`); see INTEGRATION.md.

The sub-modules below only *hold* the parameters -- under the reference's
attribute names, created in the reference's order with the reference's
initialisers, so `state_dict()` keys/shapes, strict `load_state_dict` of the
shipped checkpoints, `.cuda()`, optimisers and seeded initialisation behave
exactly as with the reference classes (`modules.py:5-311`).  Their `forward`
methods call the corresponding stage entry point of the native library.

Device contract.  Tensors on the GPU ('cuda' = HIP on PyTorch-ROCm) always run the
HIP kernels in inference (no grad) and raise if `libmtadgat.so` is missing: there is no
fallback for the inference forward of GPU tensors.  When gradients are wanted, the HIP
training step (forward that keeps a tape + HIP backward behind a `torch.autograd.Function`)
runs for every configuration the forward takes: GATv2 and GAT (v1) attention layers of up to
2048 nodes / features (fused kernels up to 128, the wide kernels of csrc/mtadgat_bwdw.hip above;
round 6: GAT v1 there too), any number of GRU and decoder layers (nn.GRU's inter-layer dropout
included); parameter gradients, and the input's when `x.requires_grad` (mtadgat_backward_input).
The forward takes up to 2048 features (window_size <= 512, hidden sizes <= 256); above 512 features
both attention layers run through a score matrix in memory (training too).  Should the library report a
configuration without a HIP training step (attention backward tiles that exceed the LDS), the call RAISES (`model.strict_hip_training`, default True): nothing on the GPU runs rocBLAS /
MIOpen behind the caller's back.  `model.strict_hip_training = False` opts into evaluating
such a step by torch ops on the GPU (`_torchpath.py`, autograd), with `model.grad_path`
naming the route and the reason and a RuntimeWarning once per reason.  A model and input left on the CPU (the reference's
`--use_cuda False` / no-GPU branch, predict.py:122, training.py:60; BASELINE config 1)
are evaluated by the package's own torch-op algebra (`_torchpath.py`), chosen by the
caller through the tensors' device.
"""
import torch
import torch.nn as nn

import _native


class _Stage(nn.Module):
    """Base of the parameter-holding sub-modules.  `_owner` (a weak reference to the MTAD_GAT that
    runs the stage) is not part of the pickled / deep-copied state; MTAD_GAT re-binds it."""

    def __getstate__(self):
        d = self.__dict__.copy()
        d.pop("_owner", None)
        return d

    def _run(self, name, x):
        owner = self.__dict__.get("_owner")
        owner = owner() if owner is not None else None
        if owner is None:
            raise RuntimeError(f"{type(self).__name__} is a stage of MTAD_GAT and cannot run detached from its model")
        return owner._stage(name, x)


class ConvLayer(_Stage):
    """Parameters of reference `ConvLayer` (`modules.py:12-16`): `conv.weight (F,F,k)`, `conv.bias (F)`."""

    def __init__(self, n_features, kernel_size=7):
        super().__init__()
        self.kernel_size = kernel_size
        self.conv = nn.Conv1d(in_channels=n_features, out_channels=n_features, kernel_size=kernel_size)

    def forward(self, x):
        return self._run("conv", x)


class _AttentionParams(_Stage):
    """Parameters shared by the two graph-attention layers (`modules.py:36-63`, `:137-164`)."""

    def __init__(self, num_nodes, node_dim, default_embed, dropout, alpha, embed_dim, use_gatv2, use_bias):
        super().__init__()
        self.dropout = dropout
        self.alpha = alpha
        self.use_gatv2 = use_gatv2
        self.use_bias = use_bias
        self.num_nodes = num_nodes
        self.embed_dim = embed_dim if embed_dim is not None else default_embed
        if use_gatv2:   # GATv2 applies `lin` to the concatenated pair, so both dims double
            self.embed_dim *= 2
            lin_in, a_in = 2 * node_dim, self.embed_dim
        else:
            lin_in, a_in = node_dim, 2 * self.embed_dim
        self.lin = nn.Linear(lin_in, self.embed_dim)
        self.a = nn.Parameter(torch.empty((a_in, 1)))
        nn.init.xavier_uniform_(self.a.data, gain=1.414)
        if use_bias:
            self.bias = nn.Parameter(torch.zeros(num_nodes, num_nodes))


class FeatureAttentionLayer(_AttentionParams):
    """Feature-oriented GAT/GATv2: nodes = features (reference `modules.py:25-122`)."""

    def __init__(self, n_features, window_size, dropout, alpha, embed_dim=None, use_gatv2=True, use_bias=True):
        super().__init__(n_features, window_size, window_size, dropout, alpha, embed_dim, use_gatv2, use_bias)
        self.n_features, self.window_size = n_features, window_size

    def forward(self, x):
        return self._run("feature_gat", x)


class TemporalAttentionLayer(_AttentionParams):
    """Time-oriented GAT/GATv2: nodes = time steps (reference `modules.py:125-217`)."""

    def __init__(self, n_features, window_size, dropout, alpha, embed_dim=None, use_gatv2=True, use_bias=True):
        super().__init__(window_size, n_features, n_features, dropout, alpha, embed_dim, use_gatv2, use_bias)
        self.n_features, self.window_size = n_features, window_size

    def forward(self, x):
        return self._run("temporal_gat", x)


class GRULayer(_Stage):
    """Parameters of reference `GRULayer` (`modules.py:228-233`); forward returns (None, h_end)."""

    def __init__(self, in_dim, hid_dim, n_layers, dropout):
        super().__init__()
        self.hid_dim, self.n_layers = hid_dim, n_layers
        self.dropout = 0.0 if n_layers == 1 else dropout
        self.gru = nn.GRU(in_dim, hid_dim, num_layers=n_layers, batch_first=True, dropout=self.dropout)

    def forward(self, x):
        # the reference also returns out[-1] (the last batch element's sequence, a batch_first
        # quirk, modules.py:237) which MTAD_GAT.forward discards (mtad_gat.py:73): not produced.
        return None, self._run("gru", x)


class RNNDecoder(nn.Module):
    """Parameters of reference `RNNDecoder` (`modules.py:249-253`)."""

    def __init__(self, in_dim, hid_dim, n_layers, dropout):
        super().__init__()
        self.in_dim = in_dim
        self.dropout = 0.0 if n_layers == 1 else dropout
        self.rnn = nn.GRU(in_dim, hid_dim, n_layers, batch_first=True, dropout=self.dropout)


class ReconstructionModel(_Stage):
    """Parameters of reference `ReconstructionModel` (`modules.py:260-262`)."""

    def __init__(self, window_size, in_dim, hid_dim, out_dim, n_layers, dropout):
        super().__init__()
        self.window_size = window_size
        self.decoder = RNNDecoder(in_dim, hid_dim, n_layers, dropout)
        self.fc = nn.Linear(hid_dim, out_dim)

    def forward(self, x):
        return self._run("recon", x)


class Forecasting_Model(_Stage):
    """Parameters of reference `Forecasting_Model` (`modules.py:295-305`): n_layers + 1 Linear."""

    def __init__(self, in_dim, hid_dim, out_dim, n_layers, dropout):
        super().__init__()
        layers = [nn.Linear(in_dim, hid_dim)]
        for _ in range(n_layers - 1):
            layers.append(nn.Linear(hid_dim, hid_dim))
        layers.append(nn.Linear(hid_dim, out_dim))
        self.layers = nn.ModuleList(layers)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x):
        return self._run("forecast", x)


class MTAD_GAT(nn.Module):
    """MTAD-GAT model, reference signature (`mtad_gat.py:37-54`).

    :param n_features: number of input features
    :param window_size: length of the input sequence
    :param out_dim: number of features to output
    :param kernel_size: size of kernel to use in the 1-D convolution (odd)
    :param feat_gat_embed_dim / time_gat_embed_dim: embedding dims of the two GAT layers
    :param use_gatv2: GATv2 attention instead of standard GAT
    :param gru_n_layers / gru_hid_dim: GRU layer
    :param forecast_n_layers / forecast_hid_dim: FC forecasting model
    :param recon_n_layers / recon_hid_dim: GRU reconstruction model
    :param dropout: dropout rate
    :param alpha: negative slope of the LeakyReLU
    """

    def __init__(
        self,
        n_features,
        window_size,
        out_dim,
        kernel_size=7,
        feat_gat_embed_dim=None,
        time_gat_embed_dim=None,
        use_gatv2=True,
        gru_n_layers=1,
        gru_hid_dim=150,
        forecast_n_layers=1,
        forecast_hid_dim=150,
        recon_n_layers=1,
        recon_hid_dim=150,
        dropout=0.2,
        alpha=0.2,
    ):
        super().__init__()
        if kernel_size % 2 == 0:
            raise ValueError("kernel_size must be odd: the reference's ConvLayer shortens the window otherwise")
        self.n_features, self.window_size, self.out_dim = n_features, window_size, out_dim
        self.alpha, self.dropout_p = alpha, dropout
        # same construction order as the reference (mtad_gat.py:56-62) => same RNG consumption
        self.conv = ConvLayer(n_features, kernel_size)
        self.feature_gat = FeatureAttentionLayer(n_features, window_size, dropout, alpha, feat_gat_embed_dim, use_gatv2)
        self.temporal_gat = TemporalAttentionLayer(n_features, window_size, dropout, alpha, time_gat_embed_dim, use_gatv2)
        self.gru = GRULayer(3 * n_features, gru_hid_dim, gru_n_layers, dropout)
        self.forecasting_model = Forecasting_Model(gru_hid_dim, forecast_hid_dim, out_dim, forecast_n_layers, dropout)
        self.recon_model = ReconstructionModel(window_size, gru_hid_dim, recon_hid_dim, out_dim, recon_n_layers, dropout)
        self._native_cfg = dict(
            n_features=n_features, window_size=window_size, out_dim=out_dim, kernel_size=kernel_size,
            use_gatv2=1 if use_gatv2 else 0, feat_embed=self.feature_gat.embed_dim,
            time_embed=self.temporal_gat.embed_dim, gru_n_layers=gru_n_layers, gru_hid_dim=gru_hid_dim,
            forecast_n_linear=forecast_n_layers + 1, forecast_hid_dim=forecast_hid_dim,
            recon_n_layers=recon_n_layers, recon_hid_dim=recon_hid_dim, alpha=float(alpha))
        self._bind()

    # -- instance plumbing: weak back-references, copy / pickle ----------------------------------------
    def _bind(self):
        """(Re-)attach the sub-modules to this instance and drop any native state (engine, packed-weight
        cache): used by __init__ and after unpickling / deepcopy, where the state belongs to the new object."""
        import weakref
        ref = weakref.ref(self)
        for mod in (self.conv, self.feature_gat, self.temporal_gat, self.gru, self.forecasting_model, self.recon_model):
            object.__setattr__(mod, "_owner", ref)
        object.__setattr__(self, "_engine", None)
        object.__setattr__(self, "_weights_key", None)
        object.__setattr__(self, "_fp_vec", None)
        object.__setattr__(self, "_fp_pending", None)
        object.__setattr__(self, "_fp_value", None)
        if "precision" not in self.__dict__:
            # arithmetic of GPU inference: "fp32" (<= 1e-5 of the reference: fp32 accumulation, state, gates and softmax
            # everywhere; the large-batch kernels form their products from split 16-bit operands on the 16-bit matrix pipe --
            # two fp16 pieces per operand where its range is bounded or recorded (recurrent state, attention outputs, the
            # convolution's outputs below 2^15, weights under a per-layer power of two), three bf16 pieces otherwise -- which
            # reproduces the fp32-MFMA result to ~2e-7: DESIGN.md section 4), "fp32_strict" (v_mfma_f32 / fp32 VALU only),
            # "bf16" (bf16 MFMA operands, fp32 accumulation / state / softmax, <= 2e-2; from 4 096 windows per call the convolution
            # and attention layers take the faster two-fp16-piece kernels of "fp32"), "auto" = bf16 exactly when the caller
            # hands over bfloat16 tensors (BASELINE "bf16 inference" configs), fp32 otherwise
            object.__setattr__(self, "precision", "auto")
        if "check_weight_contents" not in self.__dict__:
            # True: every GPU call fingerprints the parameter *contents* (one small reduction whose 8-byte result is read after
            # the call's kernels are enqueued: no stream synchronisation, see _sync_engine), so in-place edits that bypass
            # autograd's version counter (`p.data.mul_()`, `nn.init.*_(p.data)`) are seen.  False: trust (data_ptr, _version)
            # only; call refresh_weights() after such edits.  "eval_only": fingerprint in eval() mode, trust the version
            # counters in train() mode.  ("always" = True, kept for old callers.)
            object.__setattr__(self, "check_weight_contents", True)
        if "device_repack" not in self.__dict__:
            # True: after the first load, changed fp32 weights (an optimizer step) are re-packed on the GPU
            # (mtadgat_update_weights_device); False: every load goes through the host packer
            object.__setattr__(self, "device_repack", True)

    def __getstate__(self):
        d = self.__dict__.copy()
        for k in ("_engine", "_weights_key", "_fp_vec", "_fp_pending", "_fp_value"):
            d.pop(k, None)
        return d

    def __setstate__(self, state):
        super().__setstate__(state)
        self._bind()

    # -- native engine ----------------------------------------------------------------------------
    def _fingerprint(self, params):
        """Exact bit-level checksum of all parameters: sum over (int32 bits * fixed odd multipliers) mod 2^64."""
        flat = torch.cat([p.detach().reshape(-1) for p in params]).view(torch.int32).to(torch.int64)
        vec = self._fp_vec
        if vec is None or vec.device != flat.device or vec.numel() != flat.numel():
            g = torch.Generator().manual_seed(0x5EED)
            vec = (torch.randint(0, 2 ** 31, (flat.numel(),), generator=g, dtype=torch.int64) * 2 + 1).to(flat.device)
            object.__setattr__(self, "_fp_vec", vec)
        return int((flat * vec).sum())

    def refresh_weights(self):
        """Force the packed kernel weights to be rebuilt from the current parameters at the next GPU call.
        Only needed with `check_weight_contents = False` after edits autograd's version counter does not see."""
        object.__setattr__(self, "_weights_key", None)

    def _sync_engine(self, device, bf16=False):
        """Engine (on `device`) whose packed weights match the current parameters (repacked when any changed), with
        the requested arithmetic selected (the bf16 weight streams are packed on first use only).

        The content check is split in two: this half enqueues the fingerprint, `_finish_weight_check()` reads it once the
        call's kernels are enqueued (its `event.synchronize()` blocks the host until the side stream's 8-byte copy has landed --
        the main stream is not synchronised).  `_checked()` does both and repeats the call when the contents changed under
        unchanged version counters.  A caller that takes the engine from here directly (bench.py, profiles/, tests) leaves the
        check open: it is finished at the top of the next `_sync_engine`, i.e. such a caller sees a `p.data` edit one call late
        -- use `_checked` or set `check_weight_contents = False` and call `refresh_weights()`."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        params = list(self.parameters())
        for p in params:
            if p.device != device:
                raise RuntimeError(f"MTAD_GAT parameters are on '{p.device}' but the input is on '{device}': "
                                   "move the model with .to(device) / .cuda()")
        if self._engine is None or self._engine.device != device:
            object.__setattr__(self, "_engine", _native.Engine(self._native_cfg, device))
            object.__setattr__(self, "_weights_key", None)
        if getattr(self, "_fp_pending", None) is not None:
            self._finish_weight_check()                   # (a caller that took the engine directly left its check open)
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in params)
        # In-place edits that bypass autograd's version counters (`p.data.mul_()`, `nn.init.*_(p.data)`) are caught by a content
        # fingerprint, in train() and eval() mode alike ("eval_only": not while the model trains).  It does not hold the call up:
        # the kernel and an 8-byte copy to pinned memory are enqueued here, the call's kernels are enqueued behind them with the
        # weights as packed, and _finish_weight_check() reads the value afterwards -- waiting on the copy's event only -- and has
        # the call repeated with re-packed weights in the (rare) case that the contents changed under unchanged version counters.
        check = bool(self.check_weight_contents) and not (self.check_weight_contents == "eval_only" and self.training)
        pending = None
        if check:
            if all(p.dtype == torch.float32 and p.is_contiguous() for p in params):
                pending = self._engine.fingerprint_async(params, device)
            else:
                v = self._fingerprint(params)             # (odd parameter dtypes / layouts: torch ops, a host read)
                pending = lambda: v                       # noqa: E731
        mode = 1 if bf16 else (0 if self.precision == "fp32_strict" else 2)
        self._engine.set_precision(mode)
        repack = key != self._weights_key or (bf16 and not self._engine.bf16_ready())
        if check and getattr(self, "_fp_value", None) is None:
            # the contents the packed weights were built from are not on record (first call, or unchecked calls in between:
            # "eval_only" while training, the flag toggled): a `p.data` edit made meanwhile could not be seen by comparing, so
            # this call re-packs and records the fingerprint of what it packed
            repack = True
        if repack:
            self._engine.load_weights(self.state_dict(), device, allow_device_pack=self.device_repack)
            object.__setattr__(self, "_weights_key", key)
        object.__setattr__(self, "_fp_pending", (pending, repack) if pending is not None else None)
        if not check:
            object.__setattr__(self, "_fp_value", None)   # unknown from here on: the next checked call records, it cannot compare
        return self._engine

    def _finish_weight_check(self):
        """Second half of _sync_engine's content check, called once the call's kernels are enqueued: True when the parameters'
        contents differ from the ones the packed weights were built from although no version counter moved -- the packed
        weights are then marked stale and the caller repeats its launches."""
        pend = getattr(self, "_fp_pending", None)
        if pend is None:
            return False
        object.__setattr__(self, "_fp_pending", None)
        wait, repacked = pend
        value = wait()
        known = getattr(self, "_fp_value", None)
        object.__setattr__(self, "_fp_value", value)
        if repacked or known is None or known == value:
            return False
        object.__setattr__(self, "_weights_key", None)
        return True

    def _checked(self, device, bf16, fn):
        """fn(engine) with the packed weights matching the parameters: at most one repetition (see _sync_engine)."""
        out = fn(self._sync_engine(device, bf16))
        if self._finish_weight_check():
            out = fn(self._sync_engine(device, bf16))
            self._finish_weight_check()
        return out

    def _use_bf16(self, x):
        if self.precision not in ("auto", "fp32", "fp32_strict", "bf16"):
            raise ValueError("MTAD_GAT.precision must be 'auto', 'fp32', 'fp32_strict' or 'bf16'")
        return self.precision == "bf16" or (self.precision == "auto" and x.dtype == torch.bfloat16)

    def _wants_grad(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _stage(self, name, x):
        """One sub-module call (`model.conv(x)`, ...): eval-mode stage of the HIP library on the GPU,
        the torch-op stage on the CPU."""
        import _torchpath as tp
        if x.device.type != "cuda":
            x = x.float()
            fn = {"conv": tp.conv_stage, "feature_gat": tp.feature_gat_stage, "temporal_gat": tp.temporal_gat_stage,
                  "gru": tp.gru_stage, "forecast": tp.forecast_stage, "recon": tp.recon_stage}[name]
            if name in ("feature_gat", "temporal_gat", "forecast"):
                return fn(self, x, self.training)
            return fn(self, x)
        if self.training:
            raise NotImplementedError(
                "stage calls run the eval-mode HIP kernels; train-mode (dropout / gradients) is supported through "
                "MTAD_GAT.forward() -- call model.eval() for per-stage inference")
        x = x.detach().contiguous().float()
        call = {"conv": lambda eng: eng.conv(x), "feature_gat": lambda eng: eng.gat(0, x), "temporal_gat": lambda eng: eng.gat(1, x),
                "gru": lambda eng: eng.gru(x), "forecast": lambda eng: eng.heads(x, True, False)[0],
                "recon": lambda eng: eng.heads(x, False, True)[1]}[name]
        return self._checked(x.device, self._use_bf16(x), call)

    def _require_gpu(self, t, what):
        if t.device.type != "cuda":
            raise RuntimeError(
                f"MTAD_GAT.{what} is a GPU-side data path (MI355X HIP kernels) and got a tensor on '{t.device}': "
                "move the model and the series to the GPU (.cuda() / .to('cuda'))")
        if self.training:
            raise NotImplementedError(f"MTAD_GAT.{what} is an inference entry point: call model.eval() first")

    def forward(self, x):
        """x (b, window_size, n_features) -> (predictions (b, out_dim), recons (b, window_size, out_dim));
        reference `mtad_gat.py:64-79`.  x is not modified.  float32 (bf16 / fp16 inputs are answered in
        their own dtype)."""
        if x.dim() != 3 or x.shape[1] != self.window_size or x.shape[2] != self.n_features:
            raise RuntimeError(f"expected input of shape (b, {self.window_size}, {self.n_features}), got {tuple(x.shape)}")
        if x.device.type != "cuda":
            # the caller keeps model and data on the CPU (reference: `--use_cuda False` / no GPU)
            import _torchpath
            preds, recons = _torchpath.forward(self, x.float())
            return (preds.to(x.dtype), recons.to(x.dtype)) if x.dtype != torch.float32 else (preds, recons)
        grad_step = self.training or self._wants_grad(x)
        # a training step computes in fp32 whatever the request (BASELINE config 3's "bf16 train loop": the bf16 recurrence kernels
        # of rounds 2-5 were slower AND less accurate than the fp32 step at every batch size and were removed in round 6); bf16
        # tensors are still answered in bf16
        bf16 = self._use_bf16(x) and not grad_step
        if grad_step:
            # training step (Trainer.fit, training.py:100-130) or any call that will be differentiated:
            # HIP forward that keeps what the HIP backward needs, dropout in the kernels
            import _hipgrad
            stream = _hipgrad.draw_dropout_stream(self)   # once: a repetition by _checked must not consume the generator twice
            preds, recons = self._checked(x.device, bf16, lambda eng: _hipgrad.forward(self, eng, x, stream))
        else:
            with torch.no_grad():
                # bfloat16 batches go to the kernels as they are (the convolution converts while staging) when the
                # LDS-staged convolution applies; everything else is handed over as float32
                direct = x.dtype == torch.bfloat16 and self.n_features <= 64 and self.conv.kernel_size <= 31
                xin = x.contiguous() if direct else x.contiguous().float()
                preds, recons = self._checked(x.device, bf16, lambda eng: eng.forward(xin))
        if x.dtype in (torch.bfloat16, torch.float16):
            # reduced-precision I/O (BASELINE config "bf16 inference"): results in the caller's dtype
            return preds.to(x.dtype), recons.to(x.dtype)
        return preds, recons

    # -- beyond the reference's module API: the callers' data path on the GPU -------
    def forward_series(self, series, starts=None, start=0, stride=1, count=None):
        """forward() over sliding windows of a device-resident series (n_rows, F) without materialising
        them: window w = series[s_w : s_w + W], s_w = starts[w] or start + w*stride.  Equivalent to
        `SlidingWindowDataset` + default collate + `model(x)` (reference utils.py:107-120,
        prediction.py:43-55); consecutive windows share W-1 rows, so ~W times fewer input bytes are read.
        Returns (predictions (b, out_dim), recons (b, W, out_dim))."""
        self._require_gpu(series, "forward_series")
        with torch.no_grad():
            sf = series.contiguous().float()
            p, r, _ = self._checked(series.device, self._use_bf16(series), lambda eng: eng.forward_series(sf, starts, start, stride, count))
        return p, r

    # -- the attention maps behind a score (the two graph-attention layers' softmax matrices) ----------------------------------
    def attention_maps(self, x, reduce=None):
        """The post-softmax attention matrices of the two graph-attention layers for windows x (b, window_size, n_features):
        `attention` of the reference's FeatureAttentionLayer.forward (modules.py:85-89, nodes = features) and
        TemporalAttentionLayer.forward (modules.py:184-188, nodes = time steps); row i is the softmax over the keys j.
        Returns (att_feat (b, F, F), att_temp (b, W, W)), or with reduce="mean" their means over the windows ((F, F), (W, W)).

        The maps are always the EVAL-mode maps (no dropout), in train() and eval() alike: this method runs under
        torch.no_grad() and does not look at or change `self.training`.  x may be float32, bfloat16 or float16; the maps are
        float32.  GPU tensors run the HIP kernels (fp32 arithmetic whatever `self.precision` says; the mean is reduced on the
        device), CPU tensors the package's torch-op algebra (`_torchpath.py`)."""
        if x.dim() != 3 or x.shape[1] != self.window_size or x.shape[2] != self.n_features:
            raise RuntimeError(f"expected input of shape (b, {self.window_size}, {self.n_features}), got {tuple(x.shape)}")
        mean = self._attention_reduce(reduce)
        if mean and x.shape[0] == 0:
            raise RuntimeError("the mean attention map needs at least one window")
        with torch.no_grad():
            if x.device.type != "cuda":
                return self._attention_cpu(x.float(), mean)
            xin = x.detach().contiguous().float()
            return self._checked(x.device, False, lambda eng: eng.attention(xin, reduce=mean))

    def attention_series(self, series, starts=None, start=0, stride=1, count=None, reduce="mean"):
        """attention_maps() over sliding windows of a series (n_rows, F), with forward_series()'s window arguments: window
        w = series[s_w : s_w + W], s_w = starts[w] or start + w*stride (count windows; default: as many as fit).  By default
        the mean over the windows ((F, F), (W, W)); reduce=None gives the per-window maps.  On the GPU the windows are gathered
        from the device-resident series and, for the mean, the per-window maps never exist in full: they pass through the
        library's workspace a chunk at a time.  Eval-mode maps, under torch.no_grad(), `self.training` untouched."""
        mean = self._attention_reduce(reduce)
        W = self.window_size
        if series.dim() != 2 or series.shape[1] != self.n_features:
            raise RuntimeError(f"series must have shape (n_rows, {self.n_features}), got {tuple(series.shape)}")
        with torch.no_grad():
            if series.device.type != "cuda":
                if starts is None:
                    n = count if count is not None else max(0, (series.shape[0] - W - start) // max(stride, 1) + 1)
                    starts = start + torch.arange(n, dtype=torch.int64) * stride
                if starts.numel() and (int(starts.min()) < 0 or int(starts.max()) + W > series.shape[0]):
                    raise RuntimeError("a window does not lie inside the series")
                if mean and starts.numel() == 0:
                    raise RuntimeError("the mean attention map needs at least one window")
                x = series.float().unfold(0, W, 1)[starts.cpu()].permute(0, 2, 1)
                return self._attention_cpu(x, mean)
            sf = series.contiguous().float()
            return self._checked(series.device, False,
                                 lambda eng: eng.attention_series(sf, starts, start, stride, count, reduce=mean))

    @staticmethod
    def _attention_reduce(reduce):
        if reduce not in (None, "mean"):
            raise ValueError(f"reduce must be None or 'mean', got {reduce!r}")
        return reduce == "mean"

    def _attention_cpu(self, x, mean):
        import _torchpath
        att_f, att_t = _torchpath.attention_maps(self, x)
        if mean:
            return att_f.double().mean(0).float(), att_t.double().mean(0).float()
        return att_f, att_t

    def score_series(self, values):
        """The model evaluations of `Predictor.get_score` (reference prediction.py:51-63) for a whole
        series (N, F), fused: for every i in [0, N-W)
            y_hat_i  = forward(values[i : i+W])[0]                  (forecast of row i+W)
            recon_i  = forward(values[i+1 : i+W+1])[1][:, -1]       (reconstruction of row i+W)
        The reference runs two full forwards per window and throws half of each away; both outputs of
        window j are the forecast for i = j and the reconstruction for i = j-1, so ONE forward per window
        over windows 0..N-W is enough, and only the last reconstruction step is ever written.
        Returns (preds (N-W, out_dim), recons_last (N-W, out_dim))."""
        self._require_gpu(values, "score_series")
        n = values.shape[0] - self.window_size
        if n <= 0:
            raise RuntimeError("series shorter than window_size + 1")
        with torch.no_grad():
            vf = values.contiguous().float()
            p, _, last = self._checked(values.device, self._use_bf16(values),
                                       lambda eng: eng.forward_series(vf, None, 0, 1, n + 1, want_recons=False, want_last=True))
        return p[:n], last[1:n + 1]

    def anomaly_scores(self, values, target_dims=None, gamma=1.0, scale_scores=False, use_mov_av=False, smoothing_span=None, parts=None,
                       normalize_parts=True, age=None, max_age=0, min_observed=0.5, lengths=None):
        """The per-timestamp anomaly score of `Predictor.get_score` (reference prediction.py:65-103) for a
        whole series (N, F), computed on the device from `score_series`:
            a_i[d] = |y_hat_i[d] - x_{i+W}[d]| + gamma * |recon_i[d] - x_{i+W}[d]|
        (the reference writes sqrt((.)**2)), optionally (a - median) / (1 + IQR) per dimension
        (`scale_scores`; quantiles from evaluation.column_quantiles), then the mean over the target dimensions,
        optionally smoothed (`use_mov_av`: pandas' ewm(span).mean() of the global score, evaluation.moving_average;
        the span is `smoothing_span`, or the reference's int(256 * window_size * 0.05) -- its Predictor's
        hard-coded batch size of 256 -- and a span below 1 raises ValueError).  target_dims as in the reference
        (`utils.get_target_dims`): None = all features, an int or a list of column indices.
        `parts` (an evaluation.ScoreParts for this series and window, from evaluation.score_parts) treats the series as a
        concatenation of independent parts, the reference's adjust_anomaly_scores (utils.py:210-255): the global score is
        smoothed part by part when `use_mov_av` (evaluation.moving_average(parts=)), then the scores around every seam are
        set to 0 and, with `normalize_parts`, every part is min-max normalised on its own (evaluation.adjust_part_scores).
        The per-dimension scores are returned exactly as without `parts`, unless `scale_scores="per_part"`: then every part's
        per-dimension scores are scaled by the part's own median and IQR (evaluation.scale_scores(parts=); GPU only) before the
        mean over the dimensions, and the returned per-dimension scores are those per-part-scaled ones.  `scale_scores=True` keeps
        its meaning -- the quantiles of the whole series -- with or without `parts`; "per_part" without `parts`, and any other
        string, raise ValueError.
        Returns (scores (N-W,), per-dimension scores (N-W, out_dim)), both on the device; the per-dimension
        scores are never smoothed, as in the reference.
        `age` (GPU only) scores a series with filled gaps: the int32 (N, F) tensor SeriesScaler.transform(..., return_age=True)
        returns with the series -- 0 for a real sample, k for the k-th consecutive filled row; a sample is observed iff
        age <= max_age.  A score exists exactly where fitting.training_windows would have drawn a training window: score i
        belongs to window start i and target row i + W, and exists iff
          1. rows i .. i + W lie in one part (`lengths`: the parts' row counts, for a concatenated series, so that the windows over
             a seam are unscored; None: one part),
          2. the target row i + W has an observed sample among the columns target_dims (None: all),
          3. rows i .. i + W - 1 hold at least ceil(min_observed W F) observed samples over all columns
        (evaluation.scored_rows).  Everywhere else the score is NaN, and so is the per-dimension score of an unobserved target
        sample: a held value is not scored as if it had been measured.  The steps are those above with the missing entries
        left out: the masked score kernel (evaluation.anomaly_scores(age=, keep=)), scale_scores by the median and IQR of every
        column's existing entries, the mean over the row's existing entries, the moving average over the scored rows
        (evaluation.moving_average(skip_nan=True): an unscored row stays NaN).  `age` with `parts` or scale_scores="per_part", and
        `lengths` without `age`, raise ValueError."""
        if age is not None and (parts is not None or scale_scores == "per_part"):
            raise ValueError("age together with parts= or scale_scores='per_part' is not supported: per-part masked scoring is not covered")
        if lengths is not None and age is None:
            raise ValueError("lengths needs age (without age, parts= describes a concatenated series)")
        if isinstance(scale_scores, str) and scale_scores != "per_part":
            raise ValueError(f"scale_scores must be False, True or 'per_part', got {scale_scores!r}")
        if isinstance(scale_scores, str) and parts is None:
            raise ValueError("scale_scores='per_part' needs parts= (evaluation.score_parts)")
        span = None
        if use_mov_av:
            span = int(256 * self.window_size * 0.05) if smoothing_span is None else smoothing_span
            if not span >= 1:
                raise ValueError(f"the smoothing span must be >= 1, got {span!r}")
        preds, recons = self.score_series(values)
        if age is not None:
            import evaluation
            if values.device.type != "cuda":
                raise RuntimeError("anomaly_scores(age=) runs on the GPU only (the masked score kernels are HIP only)")
            keep = evaluation.scored_rows(values.shape[0], self.window_size, values.shape[1], age, max_age=max_age,
                                          min_observed=min_observed, target_dims=target_dims, lengths=lengths)
            scores, a, _ = evaluation.anomaly_scores(preds, recons, values, self.window_size, target_dims=target_dims, gamma=gamma,
                                                     age=age, max_age=max_age, keep=keep)
            if scale_scores:
                a = evaluation.scale_scores(a, skip_nan=True)
                scores = evaluation.row_means_valid(a)
            if use_mov_av:
                scores = evaluation.moving_average(scores, span, skip_nan=True)
            return scores, a
        actual = values[self.window_size:].float()
        if target_dims is not None:
            dims = [target_dims] if isinstance(target_dims, int) else list(target_dims)
            actual = actual[:, dims]
        if actual.shape[1] != preds.shape[1]:
            raise RuntimeError(f"target_dims select {actual.shape[1]} columns but the model has out_dim={preds.shape[1]}")
        a = (preds - actual).abs() + gamma * (recons - actual).abs()
        if scale_scores == "per_part":
            import evaluation
            a = evaluation.scale_scores(a, parts=parts)
        elif scale_scores:
            q = _column_quantiles(a, [0.25, 0.5, 0.75])
            a = (a - q[1]) / (1.0 + (q[2] - q[0]))
        scores = a.mean(dim=1)
        if use_mov_av:
            import evaluation
            scores = evaluation.moving_average(scores, span, parts=parts)
        if parts is not None:
            import evaluation
            scores = evaluation.adjust_part_scores(scores, parts, normalize=normalize_parts)
        return scores, a

    # -- which inputs pushed a score up: gradient attribution of anomaly_scores ---------------------------------------------------
    def score_attribution(self, values, indices, target_dims=None, gamma=1.0, scale_scores=False, method="gradient", steps=32,
                          baseline=None):
        """Attribution of the anomaly scores at `indices` to the input rows and channels they read: (len(indices), W+1, F) float32
        on values' device (a float64 series on the CPU, with a float64 model, is attributed in float64).

        For a series `values` (N, F), window W and score index i with 0 <= i < N - W (the index into anomaly_scores' output; the
        scored row is values[i+W]):
          slice S = values[i : i+W+1] (W+1 rows); window A = S[0:W], window B = S[1:W+1], target y = S[W, dims]
          a_i(S) = sum_d w_d * ( |yhat_A[d] - y[d]| + gamma * |r_B[W-1, d] - y[d]| ),  yhat_A = preds of A, r_B = recons of B
        which equals anomaly_scores(values, target_dims, gamma, scale_scores)[0][i] (reference prediction.py:65-91).
          w_d = 1/|dims|; with scale_scores=True w_d = 1/(|dims| (1 + IQR_d)), IQR_d from the whole series' per-dimension scores as
          anomaly_scores computes them, held constant (the median drops out of the gradient).  scale_scores="per_part" raises
          ValueError: the weights are one vector per call, not one per part.
        The model is the eval-mode function (no dropout) whatever self.training is; the arithmetic is fp32.
          method="gradient":   attr = d a_i / d S, shape (W+1, F), including the direct dependence through the target row
                               (sign(0) = 0, as torch's abs backward)
          method="integrated": attr = (S - b) * (1/m) sum_{k<m} d a_i / d S at b + alpha_k (S - b), alpha_k = (k + 1/2)/m, m = steps
        baseline b: None (zeros), an (F,) vector or a (W+1, F) slice; the interpolation covers the whole slice, target row included.

        GPU tensors run the HIP library (mtadgat_score_attribution: training forward without dropout and the data-only backward,
        chunked, under no_grad); self.training, the precision setting and every p.grad are left as they were.  CPU tensors go
        through the torch-op algebra with torch.autograd.grad with respect to the slices only."""
        W, F = self.window_size, self.n_features
        if isinstance(scale_scores, str):
            raise ValueError(f"score_attribution takes scale_scores=False or True, got {scale_scores!r}: per-part scaling "
                             "(anomaly_scores(scale_scores='per_part')) is not attributed yet, the weights are one vector per call")
        if values.dim() != 2 or values.shape[1] != F:
            raise RuntimeError(f"values must have shape (N, {F}), got {tuple(values.shape)}")
        if method not in ("gradient", "integrated"):
            raise ValueError(f"method must be 'gradient' or 'integrated', got {method!r}")
        m = 0
        if method == "integrated":
            m = int(steps)
            if m < 1 or m != steps:
                raise ValueError(f"steps must be a positive integer, got {steps!r}")
        n = values.shape[0] - W
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1).cpu()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise IndexError(f"score indices must lie in [0, {max(n, 0)}) for a series of {values.shape[0]} rows and window {W}")
        dims = list(range(F)) if target_dims is None else ([target_dims] if isinstance(target_dims, int) else [int(d) for d in target_dims])
        if len(dims) != self.out_dim:
            raise RuntimeError(f"target_dims select {len(dims)} columns but the model has out_dim={self.out_dim}")
        if any(d < 0 or d >= F for d in dims):
            raise IndexError(f"target_dims must lie in [0, {F})")
        dev = values.device
        gpu = dev.type == "cuda"
        dtype = values.dtype if (not gpu and values.dtype == torch.float64) else torch.float32
        if baseline is not None:
            baseline = torch.as_tensor(baseline)
            if tuple(baseline.shape) not in ((F,), (W + 1, F)):
                raise RuntimeError(f"baseline must have shape ({F},) or ({W + 1}, {F}), got {tuple(baseline.shape)}")
            baseline = baseline.to(device=dev, dtype=dtype).contiguous()
        if idx.numel() == 0:
            return torch.zeros((0, W + 1, F), dtype=torch.float32, device=dev)
        vf = values.detach().to(dtype).contiguous()
        dim_w = torch.full((len(dims),), 1.0 / len(dims), dtype=torch.float64)
        if scale_scores:
            if gpu:
                per_dim = self.anomaly_scores(vf, dims, gamma, False)[1]
            else:
                import _torchpath
                per_dim = _torchpath.per_dim_scores(self, vf, dims, gamma)
            q = _column_quantiles(per_dim, [0.25, 0.75])
            dim_w = dim_w / (1.0 + (q[1] - q[0]).double().cpu())
        if not gpu:
            import _torchpath
            return _torchpath.score_attribution(self, vf, idx.tolist(), dims, dim_w.to(dtype), gamma, m, baseline)
        with torch.no_grad():
            idx_d = idx.to(dev)
            dims_d = torch.tensor(dims, dtype=torch.int32, device=dev)
            w_d = dim_w.to(device=dev, dtype=torch.float32)
            return self._checked(dev, False, lambda eng: eng.score_attribution(vf, idx_d, dims_d, w_d, gamma, m, baseline))

    # -- the validation pass: forecast and reconstruction losses of a series ------------------------------------------------------
    def series_losses(self, values, target_dims=None, batch_size=None, starts=None, start=0, stride=1, count=None, age=None, max_age=0):
        """What the reference's `Trainer.evaluate` (training.py:188-228) computes over `SlidingWindowDataset(values, W)`, in one
        call on a series (N, F): window w = values[s_w : s_w + W] (s_w = starts[w] or start + w*stride; default the N - W windows
        0 .. N-W-1, the dataset's length) is run through the model, its forecast compared with row s_w + W and its reconstruction
        with the window itself, both on the columns `target_dims` (None = all, an int or a list, as in score_attribution).
        Returns a SeriesLosses:
          forecast_loss, recon_loss, total_loss   floats.  batch_size=None: the global RMSEs sqrt(sum SSE_f / (n out_dim)) and
                       sqrt(sum SSE_r / (n W out_dim)).  batch_size=b: the reference's epoch value for a loader of b windows
                       per batch, sqrt(mean over the batches of the batch's MSE) -- a short last batch weighs as much as a full one.
          window_sse   (n, 2) float64 on values' device: per window the squared forecast / reconstruction error
          dim_mse      (2, out_dim) float64: the global mean squared error per output dimension
          n_windows    n
        Every difference is one float32 subtraction, squared and summed in float64 (evaluation.window_sse).
        The model is the EVAL-mode function, under torch.no_grad(), whatever `self.training` is, which is left untouched: a
        validation pass in the middle of training does not have to flip modes.  GPU tensors run the HIP library
        (mtadgat_series_losses): the (n, W, out_dim) reconstructions pass through its workspace a chunk at a time and the group
        sums are formed on the device, one small host copy per call.  CPU tensors run the torch-op forward over batches of
        `batch_size` windows (256 when None) -- the calls the reference's loader would make.
        age (GPU tensors only; int32 (N, F) on values' device, as SeriesScaler.transform(..., return_age=True) returns it -- a
        boolean mask m of observed samples is (~m).to(torch.int32)): only observed samples, age <= max_age, are compared
        (mtadgat_series_losses_masked).  Per group of batch_size windows (all of them when None) mse = S_g / N_g over its observed
        terms; a group without any is left out of the mean, and no group left gives NaN.  window_sse holds the sums over the
        observed terms, window_count (n, 2) float64 their numbers (None without age), dim_mse is S / N per dimension, NaN where N == 0."""
        import evaluation
        W, F = self.window_size, self.n_features
        if values.dim() != 2 or values.shape[1] != F:
            raise RuntimeError(f"values must have shape (N, {F}), got {tuple(values.shape)}")
        if batch_size is not None and (int(batch_size) != batch_size or batch_size < 1):
            raise ValueError(f"batch_size must be a positive integer or None, got {batch_size!r}")
        dims = evaluation._target_dims(target_dims, self.out_dim, F)
        N = values.shape[0]
        dev = values.device
        if starts is not None:
            starts = torch.as_tensor(starts, dtype=torch.int64).reshape(-1)
            n = starts.numel()
            if n and (int(starts.min()) < 0 or int(starts.max()) + W > N - 1):
                raise RuntimeError("a window or its target row does not lie inside the series")
        else:
            if start < 0 or stride < 0:
                raise RuntimeError("start and stride must not be negative")
            n = int(count) if count is not None else max(0, (N - 1 - W - start) // max(stride, 1) + 1)
            if n > 0 and start + (n - 1) * stride + W > N - 1:
                raise RuntimeError("a window or its target row does not lie inside the series")
        if n < 1:
            raise RuntimeError("series_losses needs at least one window whose target row lies inside the series")
        group = n if batch_size is None else int(batch_size)
        if age is not None:
            return self._series_losses_masked(values, age, max_age, target_dims, dims, starts, start, stride, n, group)
        with torch.no_grad():
            if dev.type == "cuda":
                vf = values.detach().contiguous().float()
                dims_d = None if target_dims is None else torch.tensor(dims, dtype=torch.int32, device=dev)
                st = None if starts is None else starts.to(dev).contiguous()
                wsse, dsse = self._checked(dev, self._use_bf16(values), lambda eng: eng.series_losses(vf, st, start, stride, n, dims_d))
            else:
                wsse, dsse = self._series_losses_cpu(values.detach().float(), starts, start, stride, n, dims, min(group, n) if batch_size else 256)
            sums = evaluation.group_sums(wsse, group).cpu().numpy()
        f, r, t = evaluation.group_losses(sums, n, W, self.out_dim, batch_size)
        terms = torch.tensor([[n], [n * W]], dtype=torch.float64, device=dsse.device)
        return SeriesLosses(f, r, t, wsse, dsse / terms, n)

    def _series_losses_masked(self, values, age, max_age, target_dims, dims, starts, start, stride, n, group):
        """series_losses over observed samples: the device's (n, 4) sums and counts, their group sums, one small host copy."""
        import numpy as np
        import evaluation
        dev = values.device
        if dev.type != "cuda":
            raise RuntimeError("series_losses(age=) runs on the GPU only: the masked reduction is a HIP kernel, there is no CPU route")
        with torch.no_grad():
            vf = values.detach().contiguous().float()
            dims_d = None if target_dims is None else torch.tensor(dims, dtype=torch.int32, device=dev)
            st = None if starts is None else starts.to(dev).contiguous()
            w4, d4 = self._checked(dev, self._use_bf16(values),
                                   lambda eng: eng.series_losses(vf, st, start, stride, n, dims_d, age=age, max_age=max_age))
            sums = evaluation.group_sums(w4, group).cpu().numpy()
        with np.errstate(all="ignore"):
            losses = []
            for j in (0, 1):
                seen = sums[:, 2 + j] > 0
                losses.append(float(np.sqrt((sums[seen, j] / sums[seen, 2 + j]).mean())) if seen.any() else float("nan"))
        f, r = losses
        dim_mse = torch.where(d4[2:] > 0, d4[:2] / d4[2:], torch.full_like(d4[:2], float("nan")))
        return SeriesLosses(f, r, f + r, w4[:, :2], dim_mse, n, window_count=w4[:, 2:])

    def _series_losses_cpu(self, values, starts, start, stride, n, dims, batch):
        """(window_sse, dim_sse) from torch-op forwards over loader batches, with evaluation.window_sse's arithmetic in numpy."""
        import numpy as np
        import _torchpath
        W = self.window_size
        if starts is None:
            starts = start + torch.arange(n, dtype=torch.int64) * stride
        starts = starts.cpu()
        series = values.numpy()
        rows, dsse = [], np.zeros((2, self.out_dim), dtype=np.float64)
        with _torchpath._eval_mode(self):
            for lo in range(0, n, batch):
                st = starts[lo:lo + batch]
                x = values.unfold(0, W, 1)[st].permute(0, 2, 1).contiguous()
                preds, recons = _torchpath.forward(self, x)
                s = st.numpy()
                df = preds.numpy() - series[s + W][:, dims]
                dr = recons.numpy() - series[s[:, None] + np.arange(W)[None, :]][:, :, dims]
                with np.errstate(over="ignore", invalid="ignore"):
                    qf, qr = df.astype(np.float64) ** 2, dr.astype(np.float64) ** 2
                    rows.append(np.stack([qf.sum(axis=1), qr.reshape(len(s), -1).sum(axis=1)], axis=1))
                    dsse += np.stack([qf.sum(axis=0), qr.sum(axis=(0, 1))])
        return torch.from_numpy(np.concatenate(rows)), torch.from_numpy(dsse)


class SeriesLosses:
    """Result of MTAD_GAT.series_losses: Trainer.evaluate's three floats, and the per-window / per-dimension errors behind them."""
    __slots__ = ("forecast_loss", "recon_loss", "total_loss", "window_sse", "dim_mse", "n_windows", "window_count")

    def __init__(self, forecast_loss, recon_loss, total_loss, window_sse, dim_mse, n_windows, window_count=None):
        self.forecast_loss, self.recon_loss, self.total_loss = forecast_loss, recon_loss, total_loss
        self.window_sse, self.dim_mse, self.n_windows = window_sse, dim_mse, n_windows
        self.window_count = window_count          # (n, 2) float64: the observed terms behind window_sse; None for the unmasked call

    def __iter__(self):                   # forecast_loss, recon_loss, total_loss = model.series_losses(...): Trainer.evaluate's return
        return iter((self.forecast_loss, self.recon_loss, self.total_loss))

    def __repr__(self):
        return (f"SeriesLosses(forecast_loss={self.forecast_loss!r}, recon_loss={self.recon_loss!r}, total_loss={self.total_loss!r}, "
                f"n_windows={self.n_windows})")


def _column_quantiles(a, qs):
    """np.percentile's linear quantiles of a column (n,) -> (len(qs),), or of every column of (n, d) -> (len(qs), d).
    GPU tensors of any length go through evaluation.column_quantiles (one radix select over all columns);
    CPU tensors keep torch.quantile, a column at a time (it refuses more than 16 M elements per call)."""
    if a.device.type == "cuda":
        import evaluation
        q = evaluation.column_quantiles(a, qs.tolist() if isinstance(qs, torch.Tensor) else qs).to(a.dtype)
        return q[:, 0] if a.dim() == 1 else q
    qs = torch.as_tensor(qs, dtype=a.dtype)
    if a.dim() == 1:
        return torch.quantile(a, qs)
    return torch.stack([torch.quantile(a[:, d], qs) for d in range(a.shape[1])], dim=1)
