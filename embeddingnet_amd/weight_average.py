"""Averaged weights: an exponential moving average (EMA) or a stochastic weight average (SWA: the equal mean of snapshots,
Izmailov et al. 2018) of every floating-point tensor of a model, kept by ONE launch per step (csrc/weight_average.hip,
`embnet_weight_average_update`) beside the one-launch optimizer, and put into the model for an evaluation by one launch that
exchanges the two copies (`embnet_weight_average_swap`).

Why not torch.optim.swa_utils: one `lerp_` per tensor is 62+ launches per ResNet18 step, the step no longer replays as one HIP
graph, and a raw copy into the weights does not reliably invalidate what the conv kernels cache of them (the fp16 / bf16 planes
and the range slots, keyed on layers.WEIGHT_EPOCH and the tensor version) — `applied()` and `copy_to()` refresh those.

Both rules are the same per-element step  avg += c (w - avg)  with a host-computed coefficient (`coefficient`); BatchNorm moving
statistics are averaged with the same coefficient (torch's use_buffers=True; there is no BN re-estimation pass).  In fp32 an
average stops moving once |c (w - avg)| falls below half an ulp of avg: a relative lag of about 2^-24 / c (6e-4 at decay 0.9999),
as for every fp32 EMA; a compensated sum is out of scope.
"""
import contextlib

import numpy as np
import torch

from . import _lib
from ._lib import check
from . import layers as L
from .multi_tensor import Plan

MODES = ("ema", "swa")


def coefficient(mode, t, u, decay=0.999, warmup=True, start_iteration=0, update_every=1):
    """The coefficient c of step t (1-based) when u updates have been made: avg += c (w - avg).  Computed in double, fp32 last.
    0: no update at this step (before start_iteration, or between two updates of an `update_every` grid).
    swa: 1 / (u + 1) — the first update copies, u snapshots average to their arithmetic mean.
    ema: 1 at the first update of an averager that starts late (start_iteration > 0: from the model as it is then), otherwise
    1 - min(decay, (1 + u) / (10 + u)) with warm-up (TensorFlow's ExponentialMovingAverage(num_updates)), 1 - decay without."""
    t, u = int(t), int(u)
    if t < start_iteration or (t - start_iteration) % update_every != 0:
        return 0.0
    if mode == "swa":
        c = 1.0 / (u + 1.0)
    elif u == 0 and start_iteration > 0:
        c = 1.0
    elif warmup:
        c = 1.0 - min(float(decay), (1.0 + u) / (10.0 + u))
    else:
        c = 1.0 - float(decay)
    return float(np.float32(c))


class WeightAverager:
    """modules: a module or a list of them (the base model and a proxies.ProxyHead, say).  Covers every floating-point parameter
    and buffer — contiguous fp32 GPU tensors only — and starts every average as a bit copy of its tensor.  The descriptor table
    and the chunk list are built once: parameters and buffers do not move.
    mode 'ema': decay in (0, 1), warmup (see `coefficient`);  mode 'swa': neither.  start_iteration: the first step (1-based)
    that may update;  update_every: an update every so many steps from there.
    `n_averaged` counts the updates made, `iterations` the last step seen."""

    def __init__(self, modules, mode="ema", decay=None, warmup=None, start_iteration=0, update_every=1):
        if mode not in MODES:
            raise ValueError(f"WeightAverager: unknown mode {mode!r} ({', '.join(MODES)})")
        if mode == "swa" and (decay is not None or warmup is not None):
            raise ValueError("WeightAverager: decay and warmup belong to mode 'ema', not 'swa'")
        decay = 0.999 if decay is None else float(decay)
        if mode == "ema" and not 0.0 < decay < 1.0:
            raise ValueError(f"WeightAverager: decay={decay} must lie inside (0, 1)")
        if int(update_every) != update_every or update_every < 1:
            raise ValueError(f"WeightAverager: update_every={update_every!r} must be a whole number >= 1")
        if int(start_iteration) != start_iteration or start_iteration < 0:
            raise ValueError(f"WeightAverager: start_iteration={start_iteration!r} must be a whole number >= 0")
        self.mode, self.decay, self.warmup = mode, decay, True if warmup is None else bool(warmup)
        self.start_iteration, self.update_every = int(start_iteration), int(update_every)
        self.modules = list(modules) if isinstance(modules, (list, tuple)) else [modules]
        self.n_averaged, self.iterations = 0, 0
        self._applied = False
        self._named = self._collect(self.modules)            # name -> the model's tensor
        if not self._named:
            raise ValueError("WeightAverager: the modules hold no floating-point tensors")
        for name, t in self._named.items():
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.EmbnetError(f"WeightAverager: {name} is not a contiguous fp32 GPU tensor ({t.dtype}, {t.device})")
        with torch.no_grad():
            self.averaged = {name: t.detach().clone(memory_format=torch.contiguous_format) for name, t in self._named.items()}
        live, avgs = list(self._named.values()), list(self.averaged.values())
        self._plan = self._rows(live, avgs)                   # { w, avg, n, 0 }
        self._plan_back = self._rows(avgs, live)              # the roles exchanged: copy_to() is an update with c = 1

    @staticmethod
    def _rows(ws, avgs):
        return Plan([(w.data_ptr(), a.data_ptr(), w.numel(), 0) for w, a in zip(ws, avgs)], [w.numel() for w in ws],
                    _lib.lib().embnet_optimizer_chunk_elems(), ws[0].device)

    @staticmethod
    def _collect(modules):
        from .backbones import keras_weights
        from .proxies import ProxyHead
        named, seen = {}, set()
        for m in modules:
            items = {"proxy_head/proxies": m.proxies} if isinstance(m, ProxyHead) else keras_weights(m)
            for name, t in items.items():
                if not t.is_floating_point() or t.numel() == 0 or id(t) in seen:
                    continue
                if name in named:
                    raise ValueError(f"WeightAverager: two tensors are named {name}")
                seen.add(id(t))
                named[name] = t
        return named

    # -- the schedule --------------------------------------------------------------------------
    def coefficient(self, t, u=None):
        """c of step t (1-based) with `u` updates made so far (default: n_averaged)."""
        return coefficient(self.mode, t, self.n_averaged if u is None else u, self.decay, self.warmup, self.start_iteration,
                           self.update_every)

    def counters(self):
        return self.iterations, self.n_averaged

    def set_counters(self, counters):
        self.iterations, self.n_averaged = int(counters[0]), int(counters[1])

    def advance(self, t=None):
        """What update() does to the counters, without a launch (a replayed graph holds the launch); -> c of the step."""
        t = self.iterations + 1 if t is None else int(t)
        c = self.coefficient(t)
        self.iterations = t
        if c > 0:
            self.n_averaged += 1
        return c

    # -- launches ------------------------------------------------------------------------------
    def update(self, t=None, c_dev=None):
        """One launch: the averages take step t (default: the step after the last one seen).  c_dev: a device float (tensor or
        address) the kernel reads the coefficient from instead — a captured step; the caller keeps coefficient(t) there."""
        if self._applied:
            raise _lib.EmbnetError("WeightAverager.update inside applied(): the model holds the averages")
        c = self.advance(t)
        if c_dev is None and not c > 0:
            return                                            # nothing to do, and nobody replays this call
        if torch.is_tensor(c_dev):
            c_dev = c_dev.data_ptr()
        check(_lib.lib().embnet_weight_average_update(*self._plan.args, c, c_dev, _lib.stream()))

    def _refresh(self):
        L.WEIGHT_EPOCH[0] += 1                                # every cached plane and range is stale from here on ...
        for m in self.modules:
            L.refresh_weight_planes(m)                        # ... and current again, eagerly: a replayed graph never asks

    def _swap(self):
        check(_lib.lib().embnet_weight_average_swap(*self._plan.args, _lib.stream()))
        self._refresh()

    @contextlib.contextmanager
    def applied(self):
        """Inside the context the model holds the averages (and `averaged` the live weights): one swap launch, then the kernels'
        planes and ranges follow; the same again on exit, unconditionally — a replayed graph never runs the lazy check of the
        Python side, and stale planes would silently train on the averaged kernels."""
        if torch.cuda.is_current_stream_capturing():
            raise _lib.EmbnetError("WeightAverager.applied cannot be entered during stream capture")
        if self._applied:
            raise _lib.EmbnetError("WeightAverager.applied does not nest")
        self._swap()
        self._applied = True
        try:
            yield self
        finally:
            self._applied = False
            self._swap()

    def copy_to(self):
        """One-way: the model's tensors become the averages (for export); the live weights are lost."""
        if self._applied:
            raise _lib.EmbnetError("WeightAverager.copy_to inside applied()")
        check(_lib.lib().embnet_weight_average_update(*self._plan_back.args, 1.0, None, _lib.stream()))
        self._refresh()

    def average_buffers(self, process_group=None):
        """Data parallel: parameters' averages are bitwise equal on every rank (the same coefficient, the same weights), buffers'
        are rank-local like the buffers themselves — their mean over the ranks, as parallel.average_buffers does for the model's
        (call it when a checkpoint is written)."""
        import torch.distributed as dist
        if not (dist.is_initialized() and dist.get_world_size(process_group) > 1):
            return
        bufs = [self.averaged[k] for k, t in self._named.items() if not isinstance(t, torch.nn.Parameter)]
        if not bufs:
            return
        flat = torch.cat([b.reshape(-1) for b in bufs])
        dist.all_reduce(flat, group=process_group)
        flat /= dist.get_world_size(process_group)
        off = 0
        for b in bufs:
            b.copy_(flat[off:off + b.numel()].view_as(b))
            off += b.numel()

    # -- state ---------------------------------------------------------------------------------
    def state_dict(self):
        return {"n_averaged": self.n_averaged, "iterations": self.iterations,
                "averaged": {k: v.detach().clone() for k, v in self.averaged.items()}}

    @torch.no_grad()
    def load_state_dict(self, state):
        """Refuses a state whose tensor names or shapes differ from this averager's."""
        self.load_averaged(state["averaged"])
        self.n_averaged = int(state["n_averaged"])
        self.iterations = int(state.get("iterations", self.iterations))

    @torch.no_grad()
    def load_averaged(self, tensors):
        """name -> array or tensor, e.g. a weights file of the averages: every name and shape must match."""
        if self._applied:
            raise _lib.EmbnetError("WeightAverager.load_averaged inside applied()")
        if set(tensors) != set(self.averaged):
            odd = sorted(set(tensors) ^ set(self.averaged))
            raise _lib.EmbnetError(f"WeightAverager: the state's tensor names differ from the model's ({', '.join(odd[:4])}"
                                   f"{', ...' if len(odd) > 4 else ''})")
        for k, a in self.averaged.items():
            if tuple(np.shape(tensors[k])) != tuple(a.shape):
                raise _lib.EmbnetError(f"WeightAverager: {k} has shape {tuple(np.shape(tensors[k]))} in the state, "
                                       f"{tuple(a.shape)} in the model")
        for k, a in self.averaged.items():
            a.copy_(torch.as_tensor(np.asarray(tensors[k]) if not torch.is_tensor(tensors[k]) else tensors[k]).to(a.device, a.dtype))
