"""The optimizers the reference builds in embedding_net/utils.py:143-153 — `optimizers.Adam(lr)`,
`optimizers.RMSprop(lr)`, `keras_radam.RAdam(lr)`, else `optimizers.SGD(lr)` — with the Keras update rules and
defaults (Adam/RAdam b1 .9, b2 .999, eps 1e-7; RMSprop rho .9, eps 1e-7, no momentum; plain SGD).

torch.optim's Adam/RAdam fold epsilon into the bias-corrected denominator differently (eps/sqrt(1-b2^t) instead of
eps), so they are not the reference's rules; these are.  Each `step()` is ONE launch of `embnet_optimizer_step`
(csrc/optimizer.hip) over every parameter tensor: a device table of {w, g, slot1, slot2, n} descriptors plus a
static chunk list.  The table is re-uploaded only when a gradient pointer changed since the last step (with the
caching allocator they normally do not).  A parameter without a gradient is skipped, as Keras does.
The classes are torch.optim.Optimizer subclasses, so param_groups[...]['lr'] scheduling and state_dict() work
as usual.  GPU tensors only (the library has no CPU path).

Beyond the reference: parameter groups with a rate multiplier and a decoupled weight decay each, SGD momentum, and gradient
clipping by value or by global norm — what the proxy losses' papers train with (Proxy-Anchor: AdamW, the proxies at 100 x the
backbone's rate, clipped gradients; SoftTriple: centres at 1e-2 against 1e-4; ArcFace / CosFace: SGD, momentum 0.9, decay 5e-4).
An optimizer that uses any of them steps through `embnet_optimizer_step_groups` (still one launch; `global_clipnorm` puts
`embnet_optimizer_grad_norm` in front of it); one group with none of them issues the call it always issued.

The layer-wise adaptive rules 'lars' and 'lamb' (large-batch training; SupCon and SimCLR are LARS recipes) scale every tensor's
step by a trust ratio eta |w| / |u|: two launches per step, `embnet_optimizer_layerwise_norms` and
`embnet_optimizer_layerwise_step` (csrc/layerwise.hip), the norms in f64 on the device and bitwise reproducible.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import check
from . import layers as L
from .multi_tensor import chunk_list, f32_i32_word, pack_rows

RULE = {"sgd": 0, "rms_prop": 1, "adam": 2, "radam": 3}
MAX_GROUPS = 8               # EMBNET_OPT_MAX_GROUPS
MOMENTUM_RULE = 5            # EMBNET_OPT_MOMENTUM: 'sgd' with a momentum
LAYERWISE = {"lars": 0, "lamb": 1}       # EMBNET_LAYERWISE_*: entry points and codes of their own


class KerasOptimizer(torch.optim.Optimizer):
    """rule: 'sgd' | 'rms_prop' | 'adam' | 'radam' (the names utils.get_optimizer dispatches on) | 'lars' | 'lamb'.

    params: a parameter list, or torch-style groups (at most 8) with the keys
      lr            the group's base rate (default: `lr`); a schedule may overwrite it at any time
      lr_mult       default 1: the group steps at lr * lr_mult, so a schedule that writes one `lr` into every group keeps the ratio
      weight_decay  default 0: decoupled decay in Keras AdamW's form, variable -= variable * weight_decay * (lr * lr_mult), applied
                    before the rule (with 'adam' this is AdamW; it is not the l2 regulariser of set_l2, which joins the gradient)
    momentum, nesterov: Keras' SGD momentum (rule 'sgd' only): v = momentum v - lr g;  w += nesterov ? momentum v - lr g : v.
    clipvalue c: every gradient element is clamped to [-c, c].  global_clipnorm c: all gradients are scaled by
    c / max(norm, c), norm the 2-norm over every gradient of the step (TensorFlow's clip_by_global_norm); `grad_norm` then holds
    the norm before clipping.  The two are exclusive.  Both act on the gradient after the l2 regularisers' part joined it.
    Under data parallelism step() runs after the gradient all-reduce, so every rank holds the same gradients and computes the
    same norm in the same order: no extra collective, and the ranks' weights stay bitwise equal.

    'lars' (SimCLR's LARSOptimizer form; momentum 0.9 unless given, nesterov allowed) and 'lamb' (beta_1, beta_2, epsilon as
    'adam'; no momentum) take one more group key:
      trust_coefficient  eta (default: the constructor's `trust_coefficient`, which is 1e-3 for 'lars' and 1 for 'lamb'); the
                    group's tensors step at lr * lr_mult * r, r = eta |w| / |u| per tensor (1 where a norm is zero); 0 exempts the
                    group from adaptation (r = 1), as the papers exempt BatchNorm parameters and biases
    and under these two rules `weight_decay` is COUPLED: it joins the direction whose norm is taken, u = g' + weight_decay * w
    for 'lars' and u = m_hat / (sqrt(v_hat) + epsilon) + weight_decay * w for 'lamb' (with eta = 0: SGD with L2 decay, and AdamW).
    The clips act on the gradient in front, as above.  `trust_ratios` holds every tensor's r of the last step."""

    def __init__(self, params, rule, lr, beta_1=0.9, beta_2=0.999, rho=0.9, epsilon=1e-7, momentum=None, nesterov=False,
                 clipvalue=None, global_clipnorm=None, trust_coefficient=None):
        if rule not in RULE and rule not in LAYERWISE:
            raise KeyError(rule)
        self.layerwise = rule in LAYERWISE
        if momentum is None:
            momentum = 0.9 if rule == "lars" else 0.0
        if momentum < 0 or (clipvalue is not None and clipvalue < 0) or (global_clipnorm is not None and global_clipnorm < 0):
            raise ValueError("momentum, clipvalue and global_clipnorm must not be negative")
        if clipvalue and global_clipnorm:
            raise ValueError("clipvalue and global_clipnorm are exclusive")
        if nesterov and not momentum:
            raise ValueError("nesterov needs a momentum")
        if (momentum or nesterov) and rule not in ("sgd", "lars"):
            raise ValueError(f"momentum and nesterov belong to the rules 'sgd' and 'lars', not {rule!r}")
        if trust_coefficient is not None and not self.layerwise:
            raise ValueError(f"trust_coefficient belongs to the rules 'lars' and 'lamb', not {rule!r}")
        defaults = dict(lr=float(lr), lr_mult=1.0, weight_decay=0.0)
        if self.layerwise:
            defaults["trust_coefficient"] = float({"lars": 1e-3, "lamb": 1.0}[rule] if trust_coefficient is None else trust_coefficient)
        super().__init__(params, defaults)
        self.rule, self.b1, self.b2, self.rho, self.eps = rule, beta_1, beta_2, rho, epsilon
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        self.clipvalue = float(clipvalue) if clipvalue else 0.0
        self.global_clipnorm = float(global_clipnorm) if global_clipnorm else 0.0
        self.iterations = 0
        self._tensors = [p for g in self.param_groups for p in g["params"] if p.requires_grad]
        if not self._tensors:
            raise ValueError("optimizer got no trainable parameters")
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"{len(self.param_groups)} parameter groups: the update kernel takes at most {MAX_GROUPS}")
        for g in self.param_groups:
            if g["weight_decay"] < 0:
                raise ValueError("weight_decay must not be negative")
            if self.layerwise and not g["trust_coefficient"] >= 0:
                raise ValueError("trust_coefficient must not be negative")
        self._ptrs, self._table, self._chunks, self._host, self._copied = None, None, None, None, None
        self._l2 = {}                # parameter -> lambda of its kernel_regularizer (set_l2): 2*lambda*w joins the gradient in the kernel
        self.coef_dev = None         # device float[6] the kernel reads its scalars from (set by a graph-capturing trainer)
        self.group_coef_dev = None   # device float[groups][4] beside it (group_scalars): read only while coef_dev is set
        self._norm = None            # device f64 [4]: N2, norm, the clip scale (a float in the third word's first half), unused
        self._stats = None           # 'lars' / 'lamb': (device f64 [tensors][3] = W2, U2, {float r, 0}; the norms' workspace)

    @property
    def grouped(self):
        """Whether step() needs embnet_optimizer_step_groups: any group, decay, multiplier, momentum or clip beyond the reference's."""
        gs = self.param_groups
        return (self.layerwise or len(gs) != 1 or gs[0].get("weight_decay", 0.0) != 0 or gs[0].get("lr_mult", 1.0) != 1 or self.momentum != 0
                or self.clipvalue != 0 or self.global_clipnorm != 0)

    @property
    def grad_norm(self):
        """Device float64 scalar at a static address: the global gradient norm of the last step before clipping (0 before the
        first one).  Only written with `global_clipnorm`; valid under graph replay."""
        return self._norm_buffers()[0][1]

    def _norm_buffers(self):
        if self._norm is None:
            dev = self._tensors[0].device
            nbytes = _lib.lib().embnet_optimizer_grad_norm_workspace_bytes(self._chunk_list().shape[0])
            # the workspace's first 16 bytes are the arrival ticket: zero once, the kernel re-arms it
            self._norm = (torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(-(-nbytes // 8), dtype=torch.float64, device=dev))
        return self._norm

    def _layerwise_buffers(self):
        if self._stats is None:
            dev = self._tensors[0].device
            nbytes = _lib.lib().embnet_optimizer_layerwise_workspace_bytes(self._chunk_list().shape[0])
            # the workspace's first 16 bytes are the arrival ticket: zero once, the kernel re-arms it
            self._stats = (torch.zeros((len(self._tensors), 3), dtype=torch.float64, device=dev),
                           torch.zeros(-(-nbytes // 8), dtype=torch.float64, device=dev))
        return self._stats

    @property
    def trust_ratios(self):
        """Device float32 [tensors] at a static address (a view of the norms kernel's stats, in the order of the optimizer's
        trainable parameters): every tensor's trust ratio r of the last step — 1 for an exempt group, a tensor without a
        gradient or a zero norm; 0 before the first step.  Rules 'lars' and 'lamb' only; valid under graph replay."""
        if not self.layerwise:
            raise AttributeError(f"trust_ratios belong to the rules 'lars' and 'lamb', not {self.rule!r}")
        return self._layerwise_buffers()[0].view(torch.float32)[:, 4]

    @property
    def adapted(self):
        """Indices (into `trust_ratios`) of the tensors whose group has a trust coefficient above zero."""
        eta = {id(p): g["trust_coefficient"] for g in self.param_groups for p in g["params"]}
        return [i for i, p in enumerate(self._tensors) if eta[id(p)] > 0]

    # -- state ----------------------------------------------------------------------------
    def _slots(self, p):
        st = self.state[p]
        # sgd's and lars' slot1: the velocity (lars keeps it at momentum 0 too)
        n = {"sgd": 1 if self.momentum else 0, "rms_prop": 1, "adam": 2, "radam": 2, "lars": 1, "lamb": 2}[self.rule]
        for i in range(n):
            if f"slot{i + 1}" not in st:
                st[f"slot{i + 1}"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st.get("slot1"), st.get("slot2")

    def set_l2(self, kernels):
        """[(parameter, lambda)]: fold the gradient of kernel_regularizer=l2(lambda) — 2*lambda*w — into the update launch
        (the caller then adds only the regularisers' VALUE to the loss: layers.regularization_loss(..., with_grad=False))."""
        self._l2 = {id(p): float(lam) for p, lam in kernels}
        self._ptrs = None

    def state_dict(self):
        d = super().state_dict()
        d["iterations"] = self.iterations
        return d

    def load_state_dict(self, d):
        d = dict(d)
        self.iterations = int(d.pop("iterations", 0))
        super().load_state_dict(d)
        self._ptrs = None

    # -- one launch -----------------------------------------------------------------------
    def _coefficients(self, lr, t):
        """-> (kernel rule, b1, b2, c1, c2), scalars in double (oracle/optimizers.py states the rules)."""
        if self.rule == "sgd":
            return 0, 0.0, 0.0, 0.0, 0.0
        if self.rule == "rms_prop":
            return 1, self.rho, 0.0, 0.0, 0.0
        b1, b2 = self.b1, self.b2
        if self.rule == "adam":
            return 2, b1, b2, lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t), 0.0
        sma_inf = 2.0 / (1.0 - b2) - 1.0
        sma_t = sma_inf - 2.0 * t * b2 ** t / (1.0 - b2 ** t)
        if sma_t >= 5.0:
            r_t = math.sqrt((sma_t - 4.0) / (sma_inf - 4.0) * (sma_t - 2.0) / (sma_inf - 2.0) * sma_inf / sma_t)
            return 3, b1, b2, lr * r_t / (1.0 - b1 ** t), 1.0 / (1.0 - b2 ** t)
        return 4, b1, b2, lr / (1.0 - b1 ** t), 0.0

    def _chunk_list(self):
        """The static half of the launch (multi_tensor.py): parameters keep their sizes."""
        if self._chunks is None:
            sizes = [p.numel() for p in self._tensors]
            self._chunks = torch.from_numpy(chunk_list(sizes, _lib.lib().embnet_optimizer_chunk_elems())).to(self._tensors[0].device)
        return self._chunks

    def _build_table(self):
        dev = self._tensors[0].device
        rows, ptrs = [], []
        group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
        for p in self._tensors:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.EmbnetError("KerasOptimizer: parameters must be contiguous fp32 GPU tensors")
            g = p.grad
            if g is not None and (g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape):
                raise _lib.EmbnetError("KerasOptimizer: gradients must be dense contiguous fp32")
            s1, s2 = self._slots(p)
            gp = g.data_ptr() if g is not None else 0
            rows.append((p.data_ptr(), gp, s1.data_ptr() if s1 is not None else 0, s2.data_ptr() if s2 is not None else 0,
                         p.numel(), f32_i32_word(2.0 * self._l2.get(id(p), 0.0), group_of[id(p)])))     # {float l2x2; int32 group}
            ptrs.append(gp)
        self._chunk_list()
        rows = torch.from_numpy(pack_rows(rows))
        if torch.cuda.is_current_stream_capturing():
            # a captured step keeps a table (and its pinned source) of its own: replays re-run the upload node, and eager
            # steps in between must not rewrite what it copies from; no host wait is legal inside a capture either
            host = getattr(self, "_graph_host", None)     # pinned memory cannot be allocated while capturing: prepare_capture()
            if host is None or host.shape[0] != rows.shape[0]:
                raise _lib.EmbnetError("KerasOptimizer: call prepare_capture() before capturing a step")
            host.copy_(rows)
            self._table = torch.empty_like(rows, device=dev)
            self._table.copy_(host, non_blocking=True)
            self._ptrs = ptrs
            return
        # Autograd hands out fresh gradient buffers every step, so this runs every step: a ring of four staging / device
        # tables, so that the host never waits for the upload of the step before (one table + an event wait kept the host
        # at most one step ahead of the GPU: 5 ms of host time per ResNet18 step went into that wait)
        if not hasattr(self, "_ring"):
            self._ring = [[torch.empty_like(rows).pin_memory(), torch.empty_like(rows, device=dev), None] for _ in range(4)]
            self._ring_i = 0
        self._ring_i = (self._ring_i + 1) % len(self._ring)
        slot = self._ring[self._ring_i]
        if slot[2] is not None:
            slot[2].synchronize()                         # the upload issued four rebuilds ago
        slot[0].copy_(rows)
        slot[1].copy_(slot[0], non_blocking=True)
        slot[2] = torch.cuda.Event()
        slot[2].record()
        self._table = slot[1]
        self._ptrs = ptrs

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        cur = [p.grad.data_ptr() if p.grad is not None else 0 for p in self._tensors]
        if cur != self._ptrs:
            self._build_table()
        self.iterations += 1
        L.WEIGHT_EPOCH[0] += 1                             # cached bf16 planes of conv kernels are stale from here on
        if self.layerwise:
            self._step_layerwise()
        elif self.grouped:
            self._step_groups()
        else:
            lr = float(self.param_groups[0]["lr"])
            rule, b1, b2, c1, c2 = self._coefficients(lr, self.iterations)
            check(_lib.lib().embnet_optimizer_step(rule, self._table.data_ptr(), len(self._tensors), self._chunks.data_ptr(),
                                                   self._chunks.shape[0], lr, b1, b2, self.eps, c1, c2,
                                                   self.coef_dev.data_ptr() if self.coef_dev is not None else None,
                                                   _lib.stream()))
        # planes and ranges of the conv kernels among the parameters, current again in one launch each (layers.refresh_tensors)
        L.refresh_tensors(self._tensors, self)
        return loss

    def _group_rows(self, t):
        """-> (kernel rule, b1, b2, c2, [[lr_g, c1_g, d_g, 0]] per group) of step t: lr_g = lr * lr_mult, c1_g the rule's c1 at
        lr_g, d_g = (float)(lr_g * weight_decay) — all in double until the kernel's fp32."""
        rows = []
        for g in self.param_groups:
            lr = float(g["lr"]) * float(g.get("lr_mult", 1.0))
            rule, b1, b2, c1, c2 = self._coefficients(lr, t)
            rows.append([lr, c1, lr * float(g.get("weight_decay", 0.0)), 0.0])
        if self.momentum:
            rule, b1 = MOMENTUM_RULE, 0.0
        return rule, b1, b2, c2, rows

    def _step_groups(self):
        lib, stream = _lib.lib(), _lib.stream()
        table, n, chunks, n_chunks = self._table.data_ptr(), len(self._tensors), self._chunks.data_ptr(), self._chunks.shape[0]
        scale = None
        if self.global_clipnorm:
            norm, ws = self._norm_buffers()
            scale = norm.data_ptr() + 16
            check(lib.embnet_optimizer_grad_norm(table, n, chunks, n_chunks, self.global_clipnorm, ws.data_ptr(),
                                                 ws.numel() * 8, norm.data_ptr(), scale, stream))
        rule, b1, b2, c2, rows = self._group_rows(self.iterations)
        rows = np.asarray(rows, dtype=np.float32)
        on_dev = self.coef_dev is not None
        if on_dev and self.group_coef_dev is None:
            raise _lib.EmbnetError("KerasOptimizer: coef_dev without group_coef_dev (the groups' rows of group_scalars)")
        check(lib.embnet_optimizer_step_groups(rule, table, n, chunks, n_chunks, rows.ctypes.data, rows.shape[0], b1, b2, self.eps,
                                               c2, self.momentum, int(self.nesterov), self.clipvalue, scale,
                                               self.coef_dev.data_ptr() if on_dev else None,
                                               self.group_coef_dev.data_ptr() if on_dev else None, stream))

    def _layerwise_rows(self):
        """-> [[lr_g, 0, wd_g, eta_g]] per group: the rate, the decay ITSELF (it joins the direction) and the trust coefficient."""
        return [[float(g["lr"]) * float(g.get("lr_mult", 1.0)), 0.0, float(g.get("weight_decay", 0.0)), float(g["trust_coefficient"])]
                for g in self.param_groups]

    def _step_layerwise(self):
        lib, stream = _lib.lib(), _lib.stream()
        table, n, chunks, n_chunks = self._table.data_ptr(), len(self._tensors), self._chunks.data_ptr(), self._chunks.shape[0]
        scale = None
        if self.global_clipnorm:
            norm, ws = self._norm_buffers()
            scale = norm.data_ptr() + 16
            check(lib.embnet_optimizer_grad_norm(table, n, chunks, n_chunks, self.global_clipnorm, ws.data_ptr(),
                                                 ws.numel() * 8, norm.data_ptr(), scale, stream))
        stats, ws = self._layerwise_buffers()
        code, (_, b1, b2, eps, c1, c2) = self.scalars(self.iterations)
        rows = np.asarray(self._layerwise_rows(), dtype=np.float32)
        on_dev = self.coef_dev is not None
        if on_dev and self.group_coef_dev is None:
            raise _lib.EmbnetError("KerasOptimizer: coef_dev without group_coef_dev (the groups' rows of group_scalars)")
        coef_dev = self.coef_dev.data_ptr() if on_dev else None
        group_dev = self.group_coef_dev.data_ptr() if on_dev else None
        check(lib.embnet_optimizer_layerwise_norms(code, table, n, chunks, n_chunks, rows.ctypes.data, rows.shape[0], b1, b2, eps, c1, c2,
                                                   self.clipvalue, scale, coef_dev, group_dev, ws.data_ptr(), ws.numel() * 8,
                                                   stats.data_ptr(), stream))
        check(lib.embnet_optimizer_layerwise_step(code, table, n, chunks, n_chunks, rows.ctypes.data, rows.shape[0], b1, b2, eps, c1, c2,
                                                  self.momentum, int(self.nesterov), self.clipvalue, scale, coef_dev, group_dev,
                                                  stats.data_ptr(), stream))

    def prepare_capture(self):
        """Allocate what a captured step() needs that cannot be allocated during stream capture."""
        self._graph_host = torch.empty((len(self._tensors), 6), dtype=torch.int64).pin_memory()
        if self.global_clipnorm:
            self._norm_buffers()                           # grad_norm keeps its address outside the graph's pool
        if self.layerwise:
            self._layerwise_buffers()                      # so do trust_ratios
        self._ptrs = None                                  # the captured step builds (and keeps) its own table

    def scalars(self, t):
        """-> (kernel rule, [lr, b1, b2, eps, c1, c2]) of step t (1-based): what step() passes, for a caller that keeps
        them in device memory (`coef_dev`) across graph replays."""
        lr = float(self.param_groups[0]["lr"])
        if self.layerwise:                                 # LAMB's bias corrections; LARS has none
            if self.rule == "lars":
                return LAYERWISE["lars"], [lr, self.b1, self.b2, self.eps, 0.0, 0.0]
            # from the betas as the kernel holds them: its 1 - b2 is 1 - 0.999f, 1.3e-5 off 1e-3 in relative terms, and only
            # 1 / (1 - 0.999f^t) makes v c2 the weighted mean it stands for (likewise m c1)
            b1, b2 = float(np.float32(self.b1)), float(np.float32(self.b2))
            return LAYERWISE["lamb"], [lr, self.b1, self.b2, self.eps, 1.0 / (1.0 - b1 ** t), 1.0 / (1.0 - b2 ** t)]
        rule, b1, b2, c1, c2 = self._coefficients(lr, t)
        return rule, [lr, b1, b2, self.eps, c1, c2]

    def group_scalars(self, t):
        """-> the flat [lr_g, c1_g, d_g, 0] rows of step t, four floats per group: what a grouped step() passes, for
        `group_coef_dev` (beside `coef_dev`, whose b1, b2, eps and c2 a grouped step reads); [] when step() is not grouped."""
        if not self.grouped:
            return []
        if self.layerwise:                                 # [lr_g, 0, wd_g, eta_g]
            return [v for row in self._layerwise_rows() for v in row]
        return [v for row in self._group_rows(t)[4] for v in row]


def save_optimizer_state(path, opt, named_params, extra=None):
    """Optimizer slots keyed by the Keras weight names (backbones.keras_weights order), `iterations`, and `extra` scalars
    (e.g. the epoch) -> an .npz next to a weights checkpoint, so that --resume_from continues Adam / RAdam / RMSprop where
    they stopped (the reference's ModelCheckpoint saves the optimizer with the model)."""
    data = {"__iterations__": np.asarray(opt.iterations), "__rule__": np.asarray(opt.rule)}
    for k, v in (extra or {}).items():
        data[f"__extra__{k}"] = np.asarray(v)
    index = {id(p): name for name, p in named_params.items()}
    for p, st in opt.state.items():
        name = index.get(id(p))
        if name is None:
            continue
        for slot in ("slot1", "slot2"):
            if slot in st:
                data[f"{name}::{slot}"] = st[slot].detach().cpu().numpy()
    np.savez(path, **data)


def load_optimizer_state(path, opt, named_params):
    """Inverse of save_optimizer_state; returns the `extra` dict.  Slots of parameters the file does not hold stay zero."""
    d = np.load(path, allow_pickle=False)
    if str(d["__rule__"]) != opt.rule:
        raise _lib.EmbnetError(f"optimizer state is for '{d['__rule__']}', the config builds '{opt.rule}'")
    opt.iterations = int(d["__iterations__"])
    mine = {id(q) for g in opt.param_groups for q in g["params"]}
    for name, p in named_params.items():
        if id(p) not in mine:                   # frozen / foreign parameters: no slots, no keys in opt.state
            continue
        s1, s2 = opt._slots(p)
        for slot, t in (("slot1", s1), ("slot2", s2)):
            if t is not None and f"{name}::{slot}" in d:
                t.copy_(torch.as_tensor(d[f"{name}::{slot}"]).to(t.device).view_as(t))
    opt._ptrs = None
    return {k[len("__extra__"):]: d[k] for k in d.files if k.startswith("__extra__")}


def SGD(params, lr):
    return KerasOptimizer(params, "sgd", lr)


def Adam(params, lr):
    return KerasOptimizer(params, "adam", lr)


def RMSprop(params, lr):
    return KerasOptimizer(params, "rms_prop", lr)


def RAdam(params, lr):
    return KerasOptimizer(params, "radam", lr)
