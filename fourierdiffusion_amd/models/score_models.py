"""ScoreModule on the HIP engine -- same surface as fdiff.models.score_models.ScoreModule
(reference: src/fdiff/models/score_models.py:22-166).

The network (Linear embed + learned positional table with max_norm + Gaussian-Fourier time
embedding -> L x post-LN transformer encoder layer (relu, dim_ff 2048) -> Linear unembed) lives in
ONE flat fp32 device buffer whose layout is defined by the engine (``fd_score_layout``); the
reference's state_dict keys are views into it, so checkpoints interchange, the optimizer is one
fused pass and the data-parallel gradient exchange is one flat RCCL all-reduce.

No autograd graph is built: ``forward`` in training mode keeps activations inside the engine and
``backward(dscore)`` accumulates into ``self.grads`` (same flat layout).

Extension (not in the reference): an exponential moving average of the weights lives next to them in a second flat buffer
(``ema_parameters``, filled by ``FusedAdamW(ema_decay=...)``); ``use_ema()`` runs every engine call on it.

Extension (not in the reference, which drops ``batch.y``): ``n_classes = K > 0`` makes the transformer model class-conditional.  One
more tensor, ``class_encoder.weight`` (K + 1, D), sits behind every other one in the flat buffer; row ``y_b`` of it is added to the time
embedding of series b inside the engine's time-embedding kernel, row K being the null (unconditional) token that a missing label
and, in training, a label dropped with probability ``label_dropout`` read.  ``DiffusionSampler.sample(y=, cfg_scale=)`` samples
with classifier-free guidance.  ``n_classes = 0`` is the reference's model bit for bit.

Extension (not in the reference): ``cond_dim = P > 0`` makes the transformer model covariate-conditional.  ``batch.y`` is then a float
tensor (B, P) of real-valued attributes; a two-layer encoder e(c) = W2 silu(W1 c + b1) + b2 of hidden width d_model -- five more
tensors ``cov_encoder.*`` behind every other one -- is added to the time embedding by the engine's k_cov_embed, and a learned null
vector ``cov_encoder.null`` takes its place where the covariates are absent or, in training, dropped with probability
``cond_dropout``.  ``DiffusionSampler.sample(y=c, cfg_scale=)`` guides on them.  Not together with ``n_classes``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from collections import OrderedDict
from typing import Any, Callable, Dict, Iterator, Optional, Tuple

import torch

from .. import _C, _rng
from ..schedulers.sde import SDE
from ..utils.dataclasses import DiffusableBatch
from ..utils.losses import get_sde_loss_fn

_PRECISIONS = {"fp32": _C.FD_MODE_F32, "bf16": _C.FD_MODE_BF16}


def _default_precision() -> str:
    return os.environ.get("FDIFF_PRECISION", "bf16")


class ScoreModule:
    # torch.nn.TransformerEncoderLayer defaults the reference relies on (score_models.py:57-59)
    dim_feedforward = 2048
    dropout = 0.1
    _backbone = _C.FD_BACKBONE_TRANSFORMER
    _d_mlp = 0

    def __init__(
        self,
        n_channels: int,
        max_len: int,
        noise_scheduler: SDE,
        fourier_noise_scaling: bool = True,
        d_model: int = 60,
        num_layers: int = 3,
        n_head: int = 12,
        num_training_steps: int = 1000,
        lr_max: float = 1e-3,
        likelihood_weighting: bool = False,
        n_classes: int = 0,
        label_dropout: float = 0.1,
        cond_dim: int = 0,
        cond_dropout: float = 0.1,
    ) -> None:
        self.n_classes = int(n_classes)
        self.label_dropout = float(label_dropout)
        self.cond_dim = int(cond_dim)
        self.cond_dropout = float(cond_dropout)
        if not 0 <= self.cond_dim <= 64:
            raise ValueError(f"cond_dim must lie in [0, 64] (0: no covariates), got {cond_dim}")
        if self.cond_dim > 0 and self._backbone != _C.FD_BACKBONE_TRANSFORMER:
            raise ValueError(f"{type(self).__name__}: cond_dim > 0 (covariate conditioning) exists for the transformer backbone only")
        if self.cond_dim > 0 and self.n_classes > 0:
            raise ValueError("cond_dim > 0 together with n_classes > 0 is not built: condition on covariates or on classes")
        if not 0.0 <= self.cond_dropout <= 1.0:
            raise ValueError(f"cond_dropout must lie in [0, 1], got {cond_dropout}")
        if self.n_classes < 0:
            raise ValueError(f"n_classes must be >= 0, got {n_classes}")
        if self.n_classes > 0 and self._backbone != _C.FD_BACKBONE_TRANSFORMER:
            raise ValueError(f"{type(self).__name__}: n_classes > 0 (class conditioning) exists for the transformer backbone only")
        if not 0.0 <= self.label_dropout <= 1.0:
            raise ValueError(f"label_dropout must lie in [0, 1], got {label_dropout}")
        self.max_len = int(max_len)
        self.n_channels = int(n_channels)
        self.noise_scheduler = noise_scheduler
        self.num_warmup_steps = num_training_steps // 10
        self.num_training_steps = num_training_steps
        self.lr_max = lr_max
        self.d_model = int(d_model)
        self.num_layers = int(num_layers)
        self.n_head = int(n_head)
        self.scale_noise = fourier_noise_scaling
        self.likelihood_weighting = likelihood_weighting
        self.training = True
        self.precision = _default_precision()      # eval/sampling arithmetic: "bf16" (MFMA) or "fp32" (parity)
        # training arithmetic (forward with dropout + backward): "bf16" = fused MFMA kernels with fp32 accumulation where they
        # are instantiated for the model's dims (else the exact-f32 kernels), "fp32" = exact-f32 kernels (parity anchor)
        self.train_precision = os.environ.get("FDIFF_TRAIN_PRECISION", "bf16")
        self._train_mode_set: Optional[str] = None
        self.hparams: Dict[str, Any] = dict(
            n_channels=n_channels, max_len=max_len, noise_scheduler=noise_scheduler,
            fourier_noise_scaling=fourier_noise_scaling, d_model=d_model, num_layers=num_layers, n_head=n_head,
            num_training_steps=num_training_steps, lr_max=lr_max, likelihood_weighting=likelihood_weighting)
        if self.n_classes > 0:      # (only then: a checkpoint of an unlabelled model stays readable by the reference's constructor)
            self.hparams.update(n_classes=self.n_classes, label_dropout=self.label_dropout)
        if self.cond_dim > 0:       # (only then, for the same reason)
            self.hparams.update(cond_dim=self.cond_dim, cond_dropout=self.cond_dropout)

        self.training_loss_fn, self.validation_loss_fn = self.set_loss_fn()

        if self.d_model % self.n_head != 0:
            raise AssertionError("embed_dim must be divisible by num_heads")
        self._dims = _C.model_dims(self.n_channels, self.max_len, self.d_model, self.n_head, self.num_layers,
                                   self.dim_feedforward)
        self._layout, self._nparams = _C.score_layout(self._dims, self._backbone, self._d_mlp, self.n_classes,
                                                       self.cond_dim)
        self._flat = torch.zeros(self._nparams, dtype=torch.float32)
        self._ema: Optional[torch.Tensor] = None              # averaged weights, same layout (enable_ema)
        self._ema_scope: Optional[torch.Tensor] = None        # inside use_ema(): the raw buffer that `_flat` stopped naming
        self._ema_meta: Optional[Dict[str, Any]] = None       # {"decay", "warmup", "num_updates"}, kept current by the optimizer
        self._other_dirty = True                              # `_dirty` of the buffer `_flat` does not name at the moment
        self._rebind = False                                  # the engine handle still points at the other buffer
        self._grads: Optional[torch.Tensor] = None
        self._zero_pending = False
        self._views: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        self._trainable: Dict[str, bool] = {}
        self._bind_views()
        self._init_parameters()
        self._handle: Optional[int] = None
        self._dirty = True

    # ------------------------------------------------------------------ parameters
    def _bind_views(self) -> None:
        self._views.clear()
        for name, off, numel, shape, trainable in self._layout:
            self._views[name] = self._flat[off:off + numel].view(*shape)
            self._trainable[name] = trainable

    def _named_copies(self, flat: torch.Tensor) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((name, flat[off:off + numel].view(*shape).detach().clone())
                           for name, off, numel, shape, _ in self._layout)

    def _init_parameters(self) -> None:
        """Same initialisers, drawn from torch's global generator in the same order as the reference's
        constructor (score_models.py:52-62), so that ``torch.manual_seed(s)`` gives the reference's weights:
        Embedding N(0,1); randn*30; Linear = kaiming_uniform(a=sqrt 5) + U(+-1/sqrt(fan_in)) bias;
        MHA: out_proj Linear init, then xavier_uniform in_proj, zero in_proj_bias / out_proj.bias;
        one encoder layer is drawn and copied into all L layers (nn.TransformerEncoder deep-copies)."""
        v = self._views
        init = torch.nn.init

        def linear(prefix: str) -> None:
            w, b = v[prefix + ".weight"], v[prefix + ".bias"]
            init.kaiming_uniform_(w, a=math.sqrt(5))
            bound = 1.0 / math.sqrt(w.shape[1]) if w.shape[1] > 0 else 0.0
            init.uniform_(b, -bound, bound)

        if "pos_encoder.embedding.weight" in v:
            init.normal_(v["pos_encoder.embedding.weight"])
        v["time_encoder.W"].copy_(torch.randn((self.d_model + 1) // 2) * 30.0)
        linear("time_encoder.dense")
        linear("embedder")
        linear("unembedder")
        self._init_backbone(v, linear)
        if "class_encoder.weight" in v:      # nn.Embedding's N(0, 1), drawn behind everything the reference's constructor draws
            init.normal_(v["class_encoder.weight"])
        if "cov_encoder.0.weight" in v:      # two nn.Linear layers, drawn behind everything else; the null vector starts at zero
            linear("cov_encoder.0")
            linear("cov_encoder.2")
            v["cov_encoder.null"].zero_()

    def _init_backbone(self, v, linear) -> None:
        init = torch.nn.init
        if self.num_layers > 0:
            p = "backbone.layers.0."
            linear(p + "self_attn.out_proj")
            init.xavier_uniform_(v[p + "self_attn.in_proj_weight"])
            v[p + "self_attn.in_proj_bias"].zero_()
            v[p + "self_attn.out_proj.bias"].zero_()
            linear(p + "linear1")
            linear(p + "linear2")
            for nm in ("norm1", "norm2"):
                v[p + nm + ".weight"].fill_(1.0)
                v[p + nm + ".bias"].zero_()
            for i in range(1, self.num_layers):
                q = f"backbone.layers.{i}."
                for k in list(v):
                    if k.startswith(p):
                        v[q + k[len(p):]].copy_(v[k])

    def parameters(self) -> Iterator[torch.Tensor]:
        return iter(self._views.values())

    def named_parameters(self) -> Iterator[Tuple[str, torch.Tensor]]:
        return iter(self._views.items())

    def trainable_mask(self) -> Dict[str, bool]:
        return dict(self._trainable)

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((k, t.detach().clone()) for k, t in self._views.items())

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True) -> None:
        missing = [k for k in self._views if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self._views]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing}, unexpected {unexpected}")
        for k, dst in self._views.items():
            if k in state_dict:
                src = state_dict[k]
                if tuple(src.shape) != tuple(dst.shape):
                    raise RuntimeError(f"size mismatch for {k}: {tuple(src.shape)} vs {tuple(dst.shape)}")
                dst.copy_(src.to(device=dst.device, dtype=torch.float32))
        self._dirty = True

    @property
    def flat_parameters(self) -> torch.Tensor:
        return self._flat

    def mark_parameters_changed(self) -> None:
        """Call after writing into ``flat_parameters`` / the views (e.g. an optimizer step)."""
        self._dirty = True

    # ------------------------------------------------------------------ averaged weights (EMA; not in the reference)
    @property
    def ema_parameters(self) -> Optional[torch.Tensor]:
        """The averaged weights: a flat fp32 buffer with the layout and device of ``flat_parameters``; None until ``enable_ema()``."""
        return self._ema

    def enable_ema(self) -> torch.Tensor:
        """Allocate the averaged weights as a copy of the current ones (idempotent); returns the buffer."""
        if self._ema is None:
            if self._ema_scope is not None:
                raise _C.FdError("enable_ema() inside use_ema()")
            self._ema = self._flat.detach().clone()
            self._other_dirty = True
        return self._ema

    def ema_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """The averaged weights under the names and shapes of ``state_dict()``."""
        if self._ema is None:
            raise _C.FdError("this model has no averaged weights: train with FusedAdamW(ema_decay=...) / Trainer(ema_decay=...), "
                             "call enable_ema(), or load a checkpoint that has an 'ema_state_dict'")
        return self._named_copies(self._ema)

    def load_ema_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True) -> None:
        missing = [k for k in self._views if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self._views]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading ema state_dict: missing {missing}, unexpected {unexpected}")
        ema = self.enable_ema()
        for name, off, numel, shape, _ in self._layout:
            if name in state_dict:
                src = state_dict[name]
                if tuple(src.shape) != tuple(shape):
                    raise RuntimeError(f"size mismatch for {name}: {tuple(src.shape)} vs {tuple(shape)}")
                ema[off:off + numel].view(*shape).copy_(src.to(device=ema.device, dtype=torch.float32))
        self.mark_ema_changed()

    def mark_ema_changed(self) -> None:
        """Call after writing into ``ema_parameters`` (the optimizer step does)."""
        if self._ema_scope is not None:
            self._dirty = True
        else:
            self._other_dirty = True

    @contextlib.contextmanager
    def use_ema(self):
        """Inside the scope every engine call (forward, the samplers, likelihood, impute) and ``state_dict()`` see the averaged
        weights; on exit -- also by exception -- the raw weights are back bit for bit.  No copy: ``flat_parameters`` names the
        other buffer and the views are rebound; the engine handle caches only the parameter pointer and the images derived from
        it, both of which the next engine call renews: through fd_score_prepare when the buffer changed since it was last
        prepared (which, as on the raw weights, renormalises the rows of the positional table above max_norm in place), else
        through fd_score_rebind, which leaves the buffer alone -- a second renormalisation would move the last bits of rows at
        the bound.  Not re-entrant; an optimizer step inside the scope raises."""
        if self._ema_scope is not None:
            raise _C.FdError("use_ema() is already active (the scope does not nest)")
        if self._ema is None:
            raise _C.FdError("use_ema(): this model has no averaged weights -- train with FusedAdamW(ema_decay=...) / "
                             "Trainer(ema_decay=...), or load a checkpoint that has an 'ema_state_dict'")
        self._ema_scope, self._flat = self._flat, self._ema
        self._swapped()
        try:
            yield self
        finally:
            self._flat, self._ema_scope = self._ema_scope, None
            self._swapped()

    def _swapped(self) -> None:
        self._bind_views()
        self._dirty, self._other_dirty = self._other_dirty, self._dirty
        self._rebind = not self._rebind        # (in and out again without an engine call in between: the handle never noticed)

    # ------------------------------------------------------------------ device / mode
    @property
    def device(self) -> torch.device:
        return self._flat.device

    def to(self, device=None, **kwargs) -> "ScoreModule":
        device = torch.device(device if device is not None else kwargs.get("device"))
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device != self._flat.device:
            if self._ema_scope is not None:
                raise _C.FdError("ScoreModule.to() inside use_ema()")
            self._release()
            self._flat = self._flat.to(device)
            if self._ema is not None:
                self._ema = self._ema.to(device)
                self._other_dirty = True
            self.grads = None
            self._bind_views()
            self._dirty = True
        return self

    def cuda(self) -> "ScoreModule":
        return self.to("cuda")

    def cpu(self) -> "ScoreModule":
        return self.to("cpu")

    def eval(self) -> "ScoreModule":
        self.training = False
        return self

    def train(self, mode: bool = True) -> "ScoreModule":
        self.training = bool(mode)
        return self

    def _release(self) -> None:
        if self._handle is not None:
            _C.lib().fd_score_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _engine(self) -> Tuple[int, int]:
        """(ctx, model handle); creates the engine object and refreshes derived weights when dirty."""
        if self._flat.device.type != "cuda":
            raise _C.FdError("ScoreModule is on the CPU: move it to the GPU with .to('cuda') -- the score network "
                             "runs only on the HIP engine (no CPU fallback)")
        ctx = _C.ctx(self._flat.device)
        if self._handle is None:
            h = C.c_void_p()
            if self.cond_dim > 0:
                rc = _C.lib().fd_score_create_cov(ctx, C.byref(self._dims), 0, self.cond_dim, C.byref(h))
                _C.check(rc, ctx)
                _C.check(_C.lib().fd_score_set_cov_dropout(h, self.cond_dropout), ctx)
            elif self.n_classes > 0:
                rc = _C.lib().fd_score_create_cond(ctx, C.byref(self._dims), self.n_classes, C.byref(h))
                _C.check(rc, ctx)
                _C.check(_C.lib().fd_score_set_label_dropout(h, self.label_dropout), ctx)
            else:
                rc = _C.lib().fd_score_create_ex(ctx, C.byref(self._dims), self._backbone, self._d_mlp, C.byref(h))
                _C.check(rc, ctx)
            self._handle = h
            self._dirty = self._other_dirty = True
            self._train_mode_set = None
        if self._dirty:
            rc = _C.lib().fd_score_prepare(self._handle, self._flat.data_ptr(), _C.stream_of(self._flat))
            _C.check(rc, ctx)
            self._dirty = self._rebind = False
        elif self._rebind:
            _C.check(_C.lib().fd_score_rebind(self._handle, self._flat.data_ptr()), ctx)
            self._rebind = False
        if self._train_mode_set != self.train_precision:
            rc = _C.lib().fd_score_set_train_mode(self._handle, _PRECISIONS[self.train_precision])
            if rc == -5 and self.train_precision == "bf16":       # FD_ERR_UNSUPPORTED: dims without bf16 training kernels
                rc = _C.lib().fd_score_set_train_mode(self._handle, _C.FD_MODE_F32)
                self.train_mode_effective = "fp32"
            else:
                self.train_mode_effective = self.train_precision
            _C.check(rc, ctx)
            self._train_mode_set = self.train_precision
        return ctx, self._handle

    @property
    def precision_effective(self) -> str:
        """The arithmetic eval / sampling really runs in: ``precision`` unless it asks for bf16 and this model's dimensions
        have no bf16 MFMA instantiation (fd_score_plan answers FD_ERR_UNSUPPORTED) -- then the exact-f32 kernels run, the same
        way ``train_mode_effective`` reports the training fallback.  The reference takes any d_model / n_head
        (score_models.py:23-65); a width the MFMA path does not cover must still sample."""
        if self.precision != "bf16":
            return self.precision
        ctx, h = self._engine()
        key = (int(h.value or 0), self.precision)
        if getattr(self, "_precision_probe", (None, None))[0] != key:
            buf = C.create_string_buffer(192)
            rc = _C.lib().fd_score_plan(h, 1, _C.FD_MODE_BF16, buf, None)
            if rc not in (0, -5):
                _C.check(rc, ctx)
            self._precision_probe = (key, "bf16" if rc == 0 else "fp32")
        return self._precision_probe[1]

    def plan(self, batch_size: int, precision: Optional[str] = None) -> Tuple[str, int]:
        """(description of the kernel path a batch of this size takes, series per workgroup) -- fd_score_plan."""
        ctx, h = self._engine()
        buf = C.create_string_buffer(192)
        spw = C.c_int(0)
        rc = _C.lib().fd_score_plan(h, int(batch_size), _PRECISIONS[precision or self.precision_effective], buf, C.byref(spw))
        _C.check(rc, ctx)
        return buf.value.decode(), spw.value

    def train_plan(self, batch_size: int) -> Tuple[str, int]:
        """(description of the training launch plan of a batch of this size, token splits of the weight-gradient kernel; 0 on
        the exact-f32 path) -- fd_score_train_plan."""
        ctx, h = self._engine()
        buf = C.create_string_buffer(192)
        ts = C.c_int(0)
        _C.check(_C.lib().fd_score_train_plan(h, int(batch_size), buf, C.byref(ts)), ctx)
        return buf.value.decode(), ts.value

    def train_cluster_xcds(self, batch_size: int) -> torch.Tensor:
        """(batch_size, ceil(max_len / 16)) int32 CPU tensor: the XCD that published each 16-token tile of each series in the last
        training forward, which must have been the persistent bf16 form at this batch size -- fd_score_train_cluster_xcds.  A row
        with one value is a cluster that exchanged its rows through that XCD's L2."""
        ctx, h = self._engine()
        B, KT = int(batch_size), (self.max_len + 15) // 16
        buf = (C.c_int * (max(B, 1) * KT))()
        _C.check(_C.lib().fd_score_train_cluster_xcds(h, B, buf, _C.stream_of(self._flat)), ctx)
        return torch.tensor(list(buf), dtype=torch.int32).view(B, KT)

    # ------------------------------------------------------------------ labels (class conditioning; not in the reference)
    def labels_on_device(self, y, batch_size: int, name: str = "y") -> Optional[torch.Tensor]:
        """``y`` validated and uploaded: an int32 device vector of ``batch_size`` labels, or None for ``y is None``.  y: an int
        (every row that class) or an integer tensor (batch_size,), every label in [0, n_classes] (n_classes itself is the null,
        unconditional token).  ValueError on an unlabelled model, a wrong length, dtype or range -- checked on the host (a device
        tensor is read back for it)."""
        if y is None:
            return None
        K = self.n_classes
        if K <= 0:
            raise ValueError(f"{name} was given, but the model is not class-conditional (n_classes = 0)")
        if isinstance(y, bool) or (not isinstance(y, (int, torch.Tensor))):
            raise ValueError(f"{name} must be an int or an integer tensor of shape ({batch_size},), got {type(y).__name__}")
        if isinstance(y, int):
            y = torch.full((batch_size,), y, dtype=torch.int64)
        if y.is_floating_point() or y.is_complex() or y.dtype == torch.bool:
            raise ValueError(f"{name} must hold integers, got {y.dtype}")
        if tuple(y.shape) != (batch_size,):
            raise ValueError(f"{name} must have shape ({batch_size},), got {tuple(y.shape)}")
        lo, hi = int(y.min()), int(y.max())
        if lo < 0 or hi > K:
            raise ValueError(f"{name} must lie in [0, {K}] ({K} = the null token), got values in [{lo}, {hi}]")
        return y.to(device=self.device, dtype=torch.int32).contiguous()

    @contextlib.contextmanager
    def _labels_bound(self, h, ctx, yd: Optional[torch.Tensor], restore: bool = False):
        """Binds the label vector for the engine calls of the scope (fd_score_set_labels) and clears it afterwards -- or, restore,
        puts the binding it found (fd_score_get_labels) back."""
        if yd is None:
            yield
            return
        # a covariate model binds its float (B, P) matrix the same way (fd_score_set_covariates / fd_score_get_covariates)
        get, put = ((_C.lib().fd_score_get_covariates, _C.lib().fd_score_set_covariates) if self.cond_dim > 0 else
                    (_C.lib().fd_score_get_labels, _C.lib().fd_score_set_labels))
        old_y, old_B = C.c_void_p(), C.c_int(0)
        if restore:
            _C.check(get(h, C.byref(old_y), C.byref(old_B)), ctx)
        _C.check(put(h, yd.data_ptr(), int(yd.shape[0])), ctx)
        try:
            yield
        finally:
            put(h, old_y, old_B.value)

    def effective_labels(self, y, batch_size: int, key: int, offset: int, p: Optional[float] = None) -> torch.Tensor:
        """The labels a training forward with the Philox stream (key, offset) uses for ``y`` (fd_label_dropout): int32 device vector,
        the null token ``n_classes`` where label dropout (p, default ``label_dropout``) struck or ``y`` is None."""
        if self.n_classes <= 0:
            raise ValueError("effective_labels: the model is not class-conditional (n_classes = 0)")
        yd = self.labels_on_device(y, batch_size)
        ctx = _C.ctx(self.device)
        out = torch.empty(batch_size, dtype=torch.int32, device=self.device)
        rc = _C.lib().fd_label_dropout(ctx, _C.ptr(yd), out.data_ptr(), int(batch_size), self.n_classes,
                                       float(self.label_dropout if p is None else p), int(key), int(offset), _C.stream_of(out))
        _C.check(rc, ctx)
        return out

    # ------------------------------------------------------------------ covariates (not in the reference)
    def covariates_on_device(self, c, batch_size: int, name: str = "y") -> Optional[torch.Tensor]:
        """``c`` validated and uploaded: a float32 device matrix (batch_size, cond_dim), or None for ``c is None``.  c: a floating
        tensor (batch_size, cond_dim), or (cond_dim,) to give every row the same covariates.  ValueError on a model without
        covariates, a wrong shape, an integer tensor or a non-finite value -- checked on the host (a device tensor is read back)."""
        if c is None:
            return None
        P = self.cond_dim
        if P <= 0:
            raise ValueError(f"{name} was given as covariates, but the model has none (cond_dim = 0)")
        if not isinstance(c, torch.Tensor) or not c.is_floating_point():
            what = c.dtype if isinstance(c, torch.Tensor) else type(c).__name__
            raise ValueError(f"{name} must be a floating tensor of shape ({batch_size}, {P}) or ({P},), got {what}")
        if c.dim() == 1 and c.shape[0] == P:
            c = c.unsqueeze(0).expand(batch_size, P)
        if tuple(c.shape) != (batch_size, P):
            raise ValueError(f"{name} must have shape ({batch_size}, {P}) or ({P},), got {tuple(c.shape)}")
        if not bool(torch.isfinite(c).all()):
            raise ValueError(f"{name} must be finite")
        return c.to(device=self.device, dtype=torch.float32).contiguous()

    def effective_keep(self, n: int, key: int, offset: int, p: Optional[float] = None) -> torch.Tensor:
        """The keep bytes of covariate dropout a training forward with the Philox stream (key, offset) draws for n rows
        (fd_cov_dropout): uint8 device vector, 0 where the row reads the null vector (p, default ``cond_dropout``)."""
        if self.cond_dim <= 0:
            raise ValueError("effective_keep: the model has no covariates (cond_dim = 0)")
        ctx = _C.ctx(self.device)
        out = torch.empty(int(n), dtype=torch.uint8, device=self.device)
        rc = _C.lib().fd_cov_dropout(ctx, out.data_ptr(), int(n), float(self.cond_dropout if p is None else p), int(key), int(offset),
                                     _C.stream_of(out))
        _C.check(rc, ctx)
        return out

    def cov_embedding(self, c, keep=None) -> torch.Tensor:
        """e (n, d_model) float32 on the device: the encoder's output for the rows of c (n, cond_dim), the null vector where
        ``keep`` (n, bool / uint8) is zero -- the engine's own kernel on the model's current weights (fd_cov_embed)."""
        if self.cond_dim <= 0:
            raise ValueError("cov_embedding: the model has no covariates (cond_dim = 0)")
        if not isinstance(c, torch.Tensor) or c.dim() != 2:
            raise ValueError(f"c must be a tensor (n, {self.cond_dim})")
        n = int(c.shape[0])
        cd = self.covariates_on_device(c, n, "c")
        kd = None if keep is None else torch.as_tensor(keep).to(device=self.device).ne(0).to(torch.uint8).contiguous()
        if kd is not None and tuple(kd.shape) != (n,):
            raise ValueError(f"keep must have shape ({n},), got {tuple(kd.shape)}")
        ctx = _C.ctx(self.device)
        v = {k: _C.dev_f32(t) for k, t in self._views.items() if k.startswith("cov_encoder.")}
        out = torch.empty(n, self.d_model, dtype=torch.float32, device=self.device)
        rc = _C.lib().fd_cov_embed(ctx, v["cov_encoder.0.weight"].data_ptr(), v["cov_encoder.0.bias"].data_ptr(),
                                   v["cov_encoder.2.weight"].data_ptr(), v["cov_encoder.2.bias"].data_ptr(),
                                   v["cov_encoder.null"].data_ptr(), cd.data_ptr(), _C.ptr(kd), out.data_ptr(), n, self.cond_dim,
                                   self.d_model, _C.stream_of(out))
        _C.check(rc, ctx)
        return out

    def _cond_on_device(self, y, batch_size: int, name: str = "y") -> Optional[torch.Tensor]:
        """What ``_labels_bound`` binds for ``y``: the covariates of a covariate model, the labels of a labelled one, else None."""
        if self.cond_dim > 0:
            return self.covariates_on_device(y, batch_size, name)
        return self.labels_on_device(y, batch_size, name) if self.n_classes > 0 else None

    # ------------------------------------------------------------------ forward / backward
    def forward(self, batch: DiffusableBatch) -> torch.Tensor:
        X = batch.X
        assert X.size()[1:] == (self.max_len, self.n_channels), (
            f"X has wrong shape, should be {(X.size(0), self.max_len, self.n_channels)}, but is {X.size()}")
        timesteps = batch.timesteps
        assert timesteps is not None and timesteps.size(0) == len(batch)
        ctx, h = self._engine()
        Xd = _C.dev_f32(X.to(self.device), "batch.X")
        td = _C.dev_f32(timesteps.to(self.device), "batch.timesteps")
        out = torch.empty_like(Xd)
        B = Xd.shape[0]
        # a labelled model reads batch.y (None: the null token on every row); an unlabelled one ignores it, as the reference does
        # (a covariate model reads it as its float (B, P) covariates, None: the null vector on every row)
        yd = self._cond_on_device(batch.y, B, "batch.y")
        if not self.training:
            mode = _PRECISIONS[self.precision_effective]
        with self._labels_bound(h, ctx, yd):
            if self.training:
                p = float(self.dropout)
                key, off = _rng.stream()
                rc = _C.lib().fd_score_forward_train(h, Xd.data_ptr(), td.data_ptr(), out.data_ptr(), B, p,
                                                     key, off, _C.stream_of(Xd))
                self._train_inputs = (Xd, td)       # the engine reads them again in backward
            else:
                rc = _C.lib().fd_score_forward(h, Xd.data_ptr(), td.data_ptr(), out.data_ptr(), B, mode,
                                               _C.stream_of(Xd))
        _C.check(rc, ctx)
        return out

    __call__ = forward

    def train_dsm(self, x_noisy: torch.Tensor, timesteps: torch.Tensor, target: torch.Tensor, std: torch.Tensor,
                  likelihood_weighting: bool = False, grad_weight: float = 1.0, y=None) -> Optional[torch.Tensor]:
        """Training forward + denoising score-matching loss + backward as one engine call (fd_score_train_dsm): the loss
        tensor, with the gradients ACCUMULATED into ``self.grads`` -- or None when this model has no fused step (exact-f32
        training, MLP / LSTM backbones, very wide C * d_model), in which case the caller runs forward -> fd_dsm_loss ->
        backward.  Same Philox stream use as ``forward`` in training mode (one key per call).  y: the batch's labels for a
        class-conditional model (as ``forward`` reads ``batch.y``; ignored by an unlabelled one)."""
        if not self.training or getattr(self, "_no_fused_dsm", False):     # (_no_fused_dsm: a manual switch, never latched here)
            return None
        ctx, h = self._engine()
        if self.train_mode_effective != "bf16":
            return None
        # capability per batch size, asked BEFORE a Philox key is drawn (an unsupported batch must not consume one: the trainer
        # counts keys per step to keep empty-slice ranks in step) and cached per B -- one oversized batch does not switch the
        # fused step off for later, smaller ones
        # (key: the engine handle the answer was given for, the batch size, and the one environment switch the C side reads per
        # call -- a recreated handle or a toggled FDIFF_TRAIN_DSM_UNFUSED must not meet a stale verdict)
        Bn = int(x_noisy.shape[0])
        cache = self.__dict__.setdefault("_fused_dsm_ok", {})
        ckey = (int(h.value) if hasattr(h, "value") else int(h), Bn, os.environ.get("FDIFF_TRAIN_DSM_UNFUSED"))
        ok = cache.get(ckey)
        if ok is None:
            ok = cache[ckey] = bool(_C.lib().fd_score_train_dsm_supported(h, Bn))
        if not ok:
            return None
        Xd = _C.dev_f32(x_noisy.to(self.device), "x_noisy")
        td = _C.dev_f32(timesteps.to(self.device), "timesteps")
        tg = _C.dev_f32(target, "target")
        sd = _C.dev_f32(std, "std")
        yd = self._cond_on_device(y, Bn)
        grads, acc = self._grads_for_backward()
        loss = torch.empty(1, device=self.device, dtype=torch.float32)
        key, off = _rng.stream()
        with self._labels_bound(h, ctx, yd):
            rc = _C.lib().fd_score_train_dsm(h, Xd.data_ptr(), td.data_ptr(), tg.data_ptr(), sd.data_ptr(),
                                             1 if likelihood_weighting else 0, float(grad_weight), Xd.shape[0], float(self.dropout),
                                             key, off, loss.data_ptr(), grads.data_ptr(), acc, _C.stream_of(Xd))
        _C.check(rc, ctx)
        self._train_inputs = (Xd, td, tg, sd)
        return loss[0]

    @property
    def grads(self) -> Optional[torch.Tensor]:
        """The flat gradient buffer (same layout as ``flat_parameters``).  ``zero_grad()`` is lazy: the next backward OVERWRITES the
        buffer (the engine's accumulate = 0 form, bit-identical to accumulating onto zeros: tests/test_gpu_train_bf16.py) instead of
        a 13 MB fill kernel in front of every step plus a read of it in every reduce; anyone who looks at the buffer before that
        backward gets the zeros here."""
        if self._zero_pending and self._grads is not None:
            self._grads.zero_()
        self._zero_pending = False
        return self._grads

    @grads.setter
    def grads(self, value: Optional[torch.Tensor]) -> None:
        self._grads = value
        self._zero_pending = False

    def _grads_for_backward(self) -> Tuple[torch.Tensor, int]:
        """(buffer, accumulate flag of the engine call) -- consumes a pending ``zero_grad()``."""
        if self._grads is None or self._grads.device != self.device:
            self._grads = torch.zeros_like(self._flat)
            self._zero_pending = False
        acc = 0 if self._zero_pending else 1
        self._zero_pending = False
        return self._grads, acc

    def zero_grad(self) -> None:
        if self._grads is not None:
            if os.environ.get("FDIFF_LAZY_ZERO_GRAD", "1") == "0":      # (A/B runs: the fill kernel of rounds 1-5)
                self._grads.zero_()
                self._zero_pending = False
            else:
                self._zero_pending = True

    def backward(self, dscore: torch.Tensor, accumulate: bool = True) -> torch.Tensor:
        """d loss / d params for the last training-mode forward; accumulates into ``self.grads``."""
        ctx, h = self._engine()
        grads, acc = self._grads_for_backward()
        d = _C.dev_f32(dscore, "dscore")
        rc = _C.lib().fd_score_backward(h, d.data_ptr(), grads.data_ptr(), acc if accumulate else 0, _C.stream_of(d))
        _C.check(rc, ctx)
        return grads

    def input_vjp(self, dscore: torch.Tensor) -> torch.Tensor:
        """d x = (d score / d x)^T dscore for the last training-mode forward (fd_score_input_vjp): a new device tensor shaped like
        the forward's input.  Consumes that forward as ``backward`` does; no parameter gradient is formed, ``grads`` and a pending
        ``zero_grad()`` are left as they are."""
        ctx, h = self._engine()
        d = _C.dev_f32(dscore, "dscore")
        dx = torch.empty_like(d)
        rc = _C.lib().fd_score_input_vjp(h, d.data_ptr(), dx.data_ptr(), _C.stream_of(d))
        _C.check(rc, ctx)
        return dx

    def grad_views(self) -> "OrderedDict[str, torch.Tensor]":
        assert self.grads is not None
        return OrderedDict((name, self.grads[off:off + numel].view(*shape))
                           for name, off, numel, shape, _ in self._layout)

    # ------------------------------------------------------------------ Lightning-style hooks
    def training_step(self, batch: DiffusableBatch, batch_idx: int = 0, dataloader_idx: int = 0,
                      grad_weight: float = 1.0) -> torch.Tensor:
        return self.training_loss_fn(self, batch, grad_weight=grad_weight)

    def validation_step(self, batch: DiffusableBatch, batch_idx: int = 0, dataloader_idx: int = 0) -> torch.Tensor:
        return self.validation_loss_fn(self, batch)

    def configure_optimizers(self):
        """AdamW(lr_max) + cosine schedule with warmup = num_training_steps // 10, stepped per batch
        (score_models.py:122-130)."""
        from ..optim import FusedAdamW, cosine_schedule_with_warmup
        opt = FusedAdamW(self, lr=self.lr_max)
        sched = cosine_schedule_with_warmup(self.num_warmup_steps, self.num_training_steps)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": sched, "interval": "step"}}

    def set_loss_fn(self) -> Tuple[Callable, Callable]:
        if isinstance(self.noise_scheduler, SDE):
            return (get_sde_loss_fn(self.noise_scheduler, train=True, likelihood_weighting=self.likelihood_weighting),
                    get_sde_loss_fn(self.noise_scheduler, train=False, likelihood_weighting=self.likelihood_weighting))
        raise NotImplementedError(
            f"Scheduler {self.noise_scheduler} not implemented yet, cannot set loss function.")

    # ------------------------------------------------------------------ checkpoints (Lightning layout)
    def save_checkpoint(self, path, **extra) -> None:
        # Lightning's layout (state_dict keys of the reference model, ctor hyper-parameters incl. the scheduler object) plus
        # the bookkeeping keys its load_from_checkpoint expects, so the reference can load checkpoints written here
        # ("state_dict" is always the RAW weights, also when written inside use_ema(); the averaged ones, when there are any, go
        #  under two extra keys the reference's loader ignores: tensors and plain numbers only, nothing it could not unpickle)
        raw = self._ema_scope if self._ema_scope is not None else self._flat
        ckpt = {"epoch": 0, "global_step": 0, "pytorch-lightning_version": "2.1.0",
                "state_dict": OrderedDict((k, t.cpu()) for k, t in self._named_copies(raw).items()),
                "hparams_name": "kwargs", "hyper_parameters": dict(self.hparams), "engine": "fourierdiffusion_amd"}
        if self._ema is not None:
            meta = self._ema_meta or {}
            ckpt["ema_state_dict"] = OrderedDict((k, t.cpu()) for k, t in self._named_copies(self._ema).items())
            ckpt["ema"] = {"decay": float(meta.get("decay", 0.0)), "warmup": bool(meta.get("warmup", False)),
                           "num_updates": int(meta.get("num_updates", 0))}
        ckpt.update(extra)
        torch.save(ckpt, path)

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, weights: str = "raw", **overrides) -> "ScoreModule":
        """weights: "raw" -- the trained weights, with the averaged ones attached (``ema_parameters``) when the file has them;
        "ema" -- the averaged weights AS the model's weights (a plain inference model; raises when the file has none);
        "auto" -- "ema" when the file has them, else "raw".  ``weights_loaded`` says which of the two the model runs."""
        if weights not in ("raw", "ema", "auto"):
            raise ValueError(f"load_from_checkpoint: weights must be 'raw', 'ema' or 'auto', got {weights!r}")
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        has_ema = "ema_state_dict" in ckpt
        if weights == "ema" and not has_ema:
            raise _C.FdError(f"{checkpoint_path} has no averaged weights ('ema_state_dict'): it was trained without ema_decay; "
                             "load it with weights='raw' or 'auto'")
        hp = dict(ckpt["hyper_parameters"])
        hp.update(overrides)
        model = cls(**hp)
        if weights != "raw" and has_ema:
            model.load_state_dict(ckpt["ema_state_dict"])
            model.weights_loaded = "ema"
        else:
            model.load_state_dict(ckpt["state_dict"])
            model.weights_loaded = "raw"
            if has_ema:
                model.load_ema_state_dict(ckpt["ema_state_dict"])
                model._ema_meta = dict(ckpt.get("ema") or {})
        if map_location is not None:
            model.to(map_location)
        return model


class MLPScoreModule(ScoreModule):
    """fdiff.models.score_models.MLPScoreModule (score_models.py:169-246) on the engine: the series is flattened to
    (B, T*C), Linear embed, + time embedding, num_layers x { h += torchvision.ops.MLP(d_model, [d_mlp, d_model], dropout 0.1)(h) },
    Linear unembed.  Exact-f32 kernels (csrc/fd_backbones.hip); state-dict keys backbone.{i}.0|3.weight|bias."""
    _backbone = _C.FD_BACKBONE_MLP

    def __init__(self, n_channels: int, max_len: int, noise_scheduler: SDE, fourier_noise_scaling: bool = True, d_model: int = 72,
                 d_mlp: int = 512, num_layers: int = 3, num_training_steps: int = 1000, lr_max: float = 1e-3,
                 likelihood_weighting: bool = False, n_classes: int = 0, cond_dim: int = 0) -> None:
        if n_classes:
            raise ValueError("MLPScoreModule: n_classes > 0 (class conditioning) exists for the transformer backbone only")
        if cond_dim:
            raise ValueError("MLPScoreModule: cond_dim > 0 (covariate conditioning) exists for the transformer backbone only")
        self._d_mlp = int(d_mlp)
        self.d_mlp = int(d_mlp)
        super().__init__(n_channels=n_channels, max_len=max_len, noise_scheduler=noise_scheduler,
                         fourier_noise_scaling=fourier_noise_scaling, d_model=d_model, num_layers=num_layers, n_head=1,
                         num_training_steps=num_training_steps, lr_max=lr_max, likelihood_weighting=likelihood_weighting)
        self.hparams = dict(n_channels=n_channels, max_len=max_len, noise_scheduler=noise_scheduler,
                            fourier_noise_scaling=fourier_noise_scaling, d_model=d_model, d_mlp=d_mlp, num_layers=num_layers,
                            num_training_steps=num_training_steps, lr_max=lr_max, likelihood_weighting=likelihood_weighting)
        self.precision = "fp32"
        self.train_precision = "fp32"

    def _init_backbone(self, v, linear) -> None:
        # nn.Linear default initialisation of every layer, drawn independently per block (a ModuleList of fresh MLPs)
        for i in range(self.num_layers):
            linear(f"backbone.{i}.0")
            linear(f"backbone.{i}.3")


class LSTMScoreModule(ScoreModule):
    """fdiff.models.score_models.LSTMScoreModule (score_models.py:249-317) on the engine: Linear embed, + time embedding,
    num_layers x { h += nn.LSTM(d_model, d_model, batch_first=True)(h)[0] }, Linear unembed.  Exact-f32 kernels; state-dict keys
    backbone.{i}.weight_ih_l0 | weight_hh_l0 | bias_ih_l0 | bias_hh_l0 (gate order i, f, g, o)."""
    _backbone = _C.FD_BACKBONE_LSTM

    def __init__(self, n_channels: int, max_len: int, noise_scheduler: SDE, fourier_noise_scaling: bool = True, d_model: int = 72,
                 num_layers: int = 3, num_training_steps: int = 1000, lr_max: float = 1e-3,
                 likelihood_weighting: bool = False, n_classes: int = 0, cond_dim: int = 0) -> None:
        if n_classes:
            raise ValueError("LSTMScoreModule: n_classes > 0 (class conditioning) exists for the transformer backbone only")
        if cond_dim:
            raise ValueError("LSTMScoreModule: cond_dim > 0 (covariate conditioning) exists for the transformer backbone only")
        super().__init__(n_channels=n_channels, max_len=max_len, noise_scheduler=noise_scheduler,
                         fourier_noise_scaling=fourier_noise_scaling, d_model=d_model, num_layers=num_layers, n_head=1,
                         num_training_steps=num_training_steps, lr_max=lr_max, likelihood_weighting=likelihood_weighting)
        self.hparams = dict(n_channels=n_channels, max_len=max_len, noise_scheduler=noise_scheduler,
                            fourier_noise_scaling=fourier_noise_scaling, d_model=d_model, num_layers=num_layers,
                            num_training_steps=num_training_steps, lr_max=lr_max, likelihood_weighting=likelihood_weighting)
        self.precision = "fp32"
        self.train_precision = "fp32"

    def _init_backbone(self, v, linear) -> None:
        # nn.LSTM.reset_parameters: every tensor U(-1/sqrt(hidden), 1/sqrt(hidden))
        k = 1.0 / math.sqrt(self.d_model)
        for i in range(self.num_layers):
            for nm in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                torch.nn.init.uniform_(v[f"backbone.{i}.{nm}"], -k, k)
