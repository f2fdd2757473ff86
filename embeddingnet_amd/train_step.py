"""The fused metric-learning training step (BASELINE.json north_star).

One forward of the class-contiguous batch [P*K, H, W, 3] -> embeddings [N,E] ->
N x N distance matrix -> mine-and-select -> hinge on the mined triplets ->
backward -> (all-reduce) -> optimizer.  Everything between the image batch and
the optimizer is HIP kernels from libembnet_hip.so; torch provides the tape and
the optimizer.  No host synchronisation inside a step (the triplet count stays
on the device).

What this replaces in the reference, per step:
  datagenerators.py:211-215  P separate predict() calls           -> the one training forward
  datagenerators.py:219      sklearn pairwise_distances           -> ops.pairwise_distances
  datagenerators.py:225-250  Python mining loop                   -> ops.mine_triplets / ops.batch_hard
  models.py:181-185          3 forwards of the mined images       -> rows gathered from the same embeddings
  losses_and_accuracies.py:26-42 + Keras mean + regularisers      -> ops.triplet_gather_loss + layers.regularization_loss
Documented semantic difference (SURVEY §7 hard part f): the reference mines with inference-mode
embeddings and normalises the a/p/n branches as three separate BN batches; the fused step mines on
the training-mode embeddings of the one batch.
"""
import os

import torch

from . import layers as L
from . import ops


class TripletTrainer:
    """graph=True (or EMBNET_GRAPH=1): after GRAPH_WARMUP eager steps the whole step — forward, loss path, backward,
    optimizer — is captured once into a HIP graph and replayed: one launch call per step instead of ~600 (ResNet18) or
    ~200 (simple2), for the batch sizes where the host cannot keep up with the GPU.  The step-dependent scalars (the
    optimizer's bias corrections, the mining seed) live in device memory and are refreshed by a 32-byte copy before
    each replay (dropout layers add a device-side step counter to their seeds); results are bit-identical to eager steps.
    Needs: the KerasOptimizer and the fused loss path (or batch_all / multi_similarity / supcon / fast_ap / smooth_ap / circle / distance_weighted); anything else, or a failed capture, falls back to eager steps.
    With a gradient reducer (N > 1) the step is two graphs — forward + backward, optimizer — with the bucketed gradient
    all-reduce issued between them as ordinary collectives.  Steps taken while the kernel trace is on run eagerly.
    negatives_selection_mode: 'semihard' | 'hardest' | 'random_hard' (the reference's rules, ops.MINING_MODES), 'batch_hard'
    (Hermans: one triplet per anchor) or 'batch_all' (every valid triplet, mean over those with a positive hinge; there are
    no triplet rows, so last_triplets = (None, n_active)) or 'multi_similarity' (Wang et al.: the pair-based loss of
    ops.multi_similarity_loss with loss_params = dict(alpha, beta, base, epsilon), defaults 2, 50, 0.5, 0.1; `margin` is not
    used; last_triplets = (None, kept pairs [1]) and last_pair_counts = int32 [4]: kept positives, kept negatives, active
    anchors, kept pairs) or 'supcon' (the softmax / InfoNCE family of ops.supcon_loss with loss_params = dict(temperature,
    denominator), defaults 0.1 and 'all' = SupCon, 'negatives' = NT-Xent; `margin` is not used; last_triplets = (None, violating
    anchors [1]) and last_pair_counts = int32 [2]: positive pairs, violating anchors) or 'fast_ap' / 'smooth_ap' (the ranking
    family: ops.fast_ap_loss with loss_params = dict(bins), default 10, and ops.smooth_ap_loss with loss_params =
    dict(temperature), default 0.01; `margin` is not used; last_triplets and last_pair_counts as for 'supcon') or 'circle' (Sun et
    al.: ops.circle_loss with loss_params = dict(m, gamma), defaults 0.4 and 80; `margin` is not used; last_triplets = (None,
    violating anchors [1]) and last_pair_counts = int32 [3]: positive pairs, violating anchors, negatives that still carry
    gradient) or 'distance_weighted' (Wu et al.: distance-weighted sampling with the margin loss, ops.margin_loss with loss_params =
    dict(beta, alpha, cutoff, nonzero_loss_cutoff), defaults 1.2, 0.2, 0.5, 1.4; `margin` is not used; the draws are keyed by the
    step's seed, from device memory in a replayed step, as the fused path's; last_triplets = (the N (K-1) drawn triplets, active
    hinges A [1]) and last_pair_counts = int32 [3]: active positive hinges, active negative hinges, A).  Under data
    parallelism every mode mines and normalises per rank.
    averager: a weight_average.WeightAverager (every trainer takes one): its one update launch follows the optimizer's in every
    step, eager, captured or replayed; without one no branch of a step changes."""
    GRAPH_WARMUP = 8          # graph='auto' decides here: see _probe
    LOSS_PARAMS = {mode: keys for mode, (_, keys, _) in ops.PAIR_LOSS_MODES.items() if keys is not None}
    # (last_triplets / last_total are the replayed step's own buffers in graph mode: read them before the next step)

    def __init__(self, base_model, optimizer, k_classes, k_samples, margin=0.5,
                 negatives_selection_mode="semihard", seed=0, reducer=None, graph=None, loss_params=None, averager=None):
        self.p, self.k, self.margin, self.mode = int(k_classes), int(k_samples), float(margin), negatives_selection_mode
        if self.mode not in tuple(ops.MINING_MODES) + ("batch_hard",) + tuple(ops.PAIR_LOSS_MODES):
            raise KeyError(self.mode)
        if loss_params and self.mode not in self.LOSS_PARAMS:
            raise ValueError(f"loss_params belong to negatives_selection_mode='multi_similarity', 'supcon', 'fast_ap' or 'smooth_ap', "
                             f"not {self.mode!r}")
        self.loss_params = self._checked_loss_params(self.mode, loss_params)
        # one gradient per parameter and step: kernels write the reducer's flat buffer in place
        self._setup(base_model, optimizer, seed, reducer, graph, direct=True, averager=averager)
        # one launch for distance matrix + mining + hinge + mean when the batch fits the fused kernel (N <= 512)
        self.fused_loss = os.environ.get("EMBNET_FUSED_LOSS", "1") == "1"

    def _setup(self, model, optimizer, seed, reducer, graph, direct, averager=None):
        """What every trainer's constructor does behind its own argument checks.  direct: whether each parameter gets ONE
        gradient contribution per step, so that the kernels may write the reducer's flat buffer in place.
        averager: a weight_average.WeightAverager (or None): its one update launch follows the optimizer's in every step."""
        self.averager = averager
        env = os.environ.get("EMBNET_GRAPH", "0")
        self.graph_mode = ({"1": True, "auto": "auto"}.get(env, False)) if graph is None else (graph if graph == "auto" else bool(graph))
        self._graph, self._graph_failed = None, False
        self.model, self.opt = model, optimizer
        self.seed, self.step_no, self.reducer = int(seed), 0, reducer
        self.ctx = L.StepContext(f"{type(self).__name__}@{id(self):x}")    # this trainer's fused hand-overs (layers.StepContext)
        self.fused_loss = False
        from .optimizers import KerasOptimizer
        self._keras_opt = isinstance(optimizer, KerasOptimizer)
        if self._keras_opt:
            # the regularisers' gradient (2*lambda*w) joins g inside the one optimizer launch; the loss keeps their value
            optimizer.set_l2(L.regularized_kernels(model))
            if reducer is not None:
                reducer.direct(direct)

    def _checked_loss_params(self, mode, loss_params):
        params = dict(loss_params or {})
        unknown = set(params) - set(self.LOSS_PARAMS.get(mode, ()))
        if unknown:
            raise ValueError(f"loss_params: unknown keys {sorted(unknown)} for {mode!r} ({', '.join(self.LOSS_PARAMS[mode])})")
        return params

    def mine(self, emb):
        with torch.no_grad():
            dist = ops.pairwise_distances(emb)
            if self.mode == "batch_hard":
                trip, count = ops.batch_hard(dist, self.p, self.k)
            else:
                trip, count, _ = ops.mine_triplets(dist, self.p, self.k, self.margin, self.mode,
                                                   seed=(self.seed << 20) + self.step_no)
            self.last_triplets = (trip, count)      # device tensors; only the first count[0] rows are live
            return trip, count

    def loss(self, images):
        """-> (total loss incl. regularisers, triplet loss, live triplet count tensor)."""
        if images.shape[0] != self.p * self.k:
            raise ValueError(f"batch of {images.shape[0]} images != k_classes*k_samples = {self.p * self.k}")
        mean, count = self.batch_loss(self.model(images))
        reg = L.regularization_loss(self.model, with_grad=not self._keras_opt)
        return (mean if reg is None else mean + reg), mean, count

    def batch_loss(self, emb):
        """The mode's loss of the class-contiguous embeddings [P*K, E] of one batch -> (mean, live count tensor); sets
        last_triplets (and last_pair_counts).  XbmTrainer adds the memory's loss of the same embeddings to it."""
        if self.mode in ops.PAIR_LOSS_MODES:                # at every batch size and whatever EMBNET_FUSED_LOSS says
            fn, keys, at = ops.PAIR_LOSS_MODES[self.mode]
            kwargs = {"margin": self.margin} if keys is None else dict(self.loss_params)
            draws = self.mode == "distance_weighted"        # the one whole-batch loss that samples: the fused path's seed
            if draws:
                kwargs.update(seed=(self.seed << 20) + self.step_no,
                              seed_dev=self._state.data_ptr() + 24 if self._graph_state_live() else None)
            out = fn(emb, self.p, self.k, **kwargs)
            mean, counts = out[:2]
            count = counts if at is None else counts[at:at + 1]             # a slice view of the counts
            if at is not None:
                self.last_pair_counts = counts
            self.last_triplets = (out[2] if draws else None, count)
        elif self.fused_loss and ops.fused_loss_supported(self.p, self.k, emb.shape[1]):
            seed_dev = self._state.data_ptr() + 24 if self._graph_state_live() else None     # uint64 behind the 6 floats
            mean, _, trip, count = ops.fused_triplet_loss(emb, self.p, self.k, self.margin, self.mode,
                                                          seed=(self.seed << 20) + self.step_no, seed_dev=seed_dev)
            self.last_triplets = (trip, count)
        else:
            trip, count = self.mine(emb)
            mean, _ = ops.triplet_gather_loss(emb, trip, count, self.margin)
        return mean, count

    # ---- graph replay ---------------------------------------------------------------------------------------
    def _graph_state_live(self):
        return getattr(self, "_state", None) is not None and torch.cuda.is_current_stream_capturing()

    ANY_LOSS_CAPTURES = False       # this class: only the fused loss path and the pair losses run without the host

    def _graph_supported(self, images):
        if not self._keras_opt or not (self.ANY_LOSS_CAPTURES or self.fused_loss or self.mode in ops.PAIR_LOSS_MODES):
            return False
        return self.opt.rule != "radam" or self.opt.iterations >= 6      # RAdam switches kernels while it warms up

    def _push_state(self):
        """Scalars of the step about to run -> the next slot of a pinned ring -> device (stream-ordered before the replay)."""
        slot = self._ring_pos % self._ring.shape[0]
        if slot % 128 == 0:                                 # about to overwrite this half: its copies of the previous lap must be done
            ev = self._ring_events[(slot // 128) % 2]
            if ev is not None:
                ev.synchronize()
        _, coef = self.opt.scalars(self.opt.iterations + 1)
        self._ring_np[slot, :6] = coef
        if self._state.numel() > 12:                        # a grouped optimizer: four floats per group behind the fixed row
            self._ring_np[slot, 12:] = self.opt.group_scalars(self.opt.iterations + 1)
        self._ring_np[slot, 6:8].view("uint64")[0] = ((self.seed << 20) + self.step_no) & (2 ** 64 - 1)
        self._ring_np[slot, 8:10].view("uint64")[0] = self._since_capture
        if self.averager is not None:                       # float 10: the averager's coefficient of this step
            self._ring_np[slot, 10] = self.averager.coefficient(self.opt.iterations + 1)
        row = self._ring[slot]
        self._state.copy_(row, non_blocking=True)
        if slot % 128 == 127:                               # last copy out of this half: its event guards the half's next lap
            ev = torch.cuda.Event(); ev.record()
            self._ring_events[(slot // 128) % 2] = ev
        self._ring_pos += 1

    def _capture(self, images):
        dev = self._tuple(images)[0].device
        # lr, b1, b2, eps, c1, c2 | seed (uint64) | steps since capture (uint64) | averager's c, pad | lr_g, c1_g, d_g, 0 per group (KerasOptimizer.group_scalars)
        width = 12 + len(self.opt.group_scalars(self.opt.iterations + 1))
        self._state = torch.zeros(width, dtype=torch.float32, device=dev)
        self._ring = torch.zeros((256, width), dtype=torch.float32).pin_memory()
        self._since_capture = 0
        self._drops = [m for m in self.model.modules() if isinstance(m, (L.Dropout, L.DropConnect))]
        self._ring_np = self._ring.numpy()                                        # same memory
        self._ring_pos, self._ring_events = 0, [None, None]
        self._gx = self._inputs_like(images)
        self.opt.coef_dev = self._state
        self.opt.group_coef_dev = self._state[12:] if width > 12 else None
        self.opt.prepare_capture()
        it0, st0 = self.opt.iterations, self.step_no
        avg0 = self.averager.counters() if self.averager is not None else None
        drop_steps = [m._step for m in self._drops]
        try:
            self._inputs_copy(images)
            self.step_no += 1
            self._push_state()
            g = torch.cuda.CUDAGraph()
            L.GRAPH_TICK = self._state.data_ptr() + 32
            try:
                if self.reducer is None:
                    with torch.cuda.graph(g):
                        self._gout = self._eager_step(self._gx)
                    self._graph_opt = None
                else:
                    # data parallel: forward + backward is one graph (the reducer counts but launches nothing), the gradient
                    # all-reduce runs between the graphs as ordinary bucketed collectives, the optimizer is a second graph
                    self.reducer.hold(True)
                    with torch.cuda.graph(g):
                        self._gout = self._eager_step(self._gx, with_update=False)
                    g2 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g2, pool=g.pool()):
                        self._update()
                    self._graph_opt = g2
            finally:
                L.GRAPH_TICK = None
                if self.reducer is not None:
                    self.reducer.hold(False)
            self._g_last = (getattr(self, "last_triplets", None), self.last_total)     # the replayed step's (static) output tensors
            self._g_pair_counts = getattr(self, "last_pair_counts", None)
            self._graph = g
        except Exception as exc:                                                  # stay correct: eager from here on
            self._graph, self._graph_failed, self._state = None, True, None
            self._graph_error = f"{type(exc).__name__}: {exc}"
            self.opt.coef_dev = None
            self.opt._ptrs = self.opt._table = None                # they pointed into the failed capture's pool
            import warnings
            warnings.warn(f"TripletTrainer: graph capture failed ({type(exc).__name__}: {exc}); running eager steps")
        finally:
            # capturing ran the Python side once without executing anything: the counters advanced, the weights did not —
            # whether or not the capture succeeded
            self.opt.iterations, self.step_no = it0, st0
            if self.averager is not None:
                self.averager.set_counters(avg0)
            for m, st in zip(self._drops, drop_steps):
                m._step = st

    # the step's inputs, as `loss` takes them: one image batch here; SiameseTrainer packs (x1, x2, y), ProxyTrainer and XbmTrainer (images, labels)
    @staticmethod
    def _tuple(inputs):
        return tuple(inputs) if isinstance(inputs, (tuple, list)) else (inputs,)

    def _inputs_like(self, inputs):
        like = tuple(torch.empty_like(t) for t in self._tuple(inputs))
        return like if isinstance(inputs, (tuple, list)) else like[0]

    def _inputs_copy(self, inputs):
        for d, t in zip(self._tuple(self._gx), self._tuple(inputs)):
            d.copy_(t)

    def _inputs_match(self, inputs):
        new, held = self._tuple(inputs), self._tuple(self._gx)
        return len(new) == len(held) and all(a.shape == b.shape for a, b in zip(new, held))

    def _replay(self, images):
        self._inputs_copy(images)
        self.step_no += 1
        self._push_state()
        self.opt.iterations += 1
        if self.averager is not None:                       # the launch is in the graph and reads the row _push_state wrote
            self.averager.advance(self.opt.iterations)
        for m in self._drops:                               # what the layers' forward() does in an eager step
            if m.training and m.enabled and m.rate > 0:
                m._step += 1
        self._since_capture += 1
        if self._graph_opt is None:
            self._graph.replay()
        else:
            self.reducer.zero_counts()
            self._graph.replay()                                # zero the flat buffer, forward, backward
            self.reducer.reduce_all()                           # bucketed all-reduce, wait, average
            self._graph_opt.replay()
        self.last_triplets, self.last_total = self._g_last      # an eager step in between re-bound them
        if self._g_pair_counts is not None:
            self.last_pair_counts = self._g_pair_counts
        return self._gout.clone()                               # callers keep per-step losses; the graph's output is one buffer

    def _probe(self, images):
        """graph='auto': three eager steps timed on the host (enqueue only) and on the device.  A step whose launches the
        host enqueues in well under its device time gains nothing from a graph; otherwise the step is captured and three
        replays are timed against the eager steps — the graph stays only if it is not slower (the replayed step works in
        a memory pool of its own, and HBM-bound networks have measured up to 1.5x slower in an unlucky one)."""
        import time
        torch.cuda.synchronize()
        t0 = time.perf_counter(); host = 0.0
        for _ in range(3):
            h0 = time.perf_counter()
            self._plain_step(images)
            host += time.perf_counter() - h0
        torch.cuda.synchronize()
        eager = (time.perf_counter() - t0) / 3
        self.graph_probe = dict(eager_ms=1e3 * eager, host_ms=1e3 * host / 3)
        want = host / 3 >= 0.8 * eager and self._graph_supported(images)
        if self.reducer is not None:                             # every rank must take the same branch: the replays hold collectives
            want = self._agree(want, any_rank=True)
        if not want:
            self.graph_mode = False                              # GPU-bound as it is
            return
        self._capture(images)
        ok = self._graph is not None
        if self.reducer is not None:
            ok = self._agree(ok, any_rank=False)                 # a rank whose capture failed takes everyone back to eager steps
            if not ok:
                self._graph, self.graph_mode = None, False
                self.opt.coef_dev = None
        if not ok:
            return
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            self._replay(images)
        torch.cuda.synchronize()
        replay = (time.perf_counter() - t0) / 3
        self.graph_probe["replay_ms"] = 1e3 * replay
        keep = replay <= 0.97 * eager
        if self.reducer is not None:
            keep = self._agree(keep, any_rank=False)
        if not keep:                                             # no gain: stay eager
            self._graph, self.graph_mode = None, False
            self.opt.coef_dev = None

    def _agree(self, flag, any_rank):
        """One decision for all ranks: True if any rank (any_rank) / every rank says so."""
        import torch.distributed as dist
        if not (dist.is_initialized() and dist.get_world_size(self.reducer.group) > 1):
            return bool(flag)
        t = torch.tensor([1.0 if flag else 0.0], device=self.reducer.flat.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX if any_rank else dist.ReduceOp.MIN, group=self.reducer.group)
        return bool(t.item() > 0.5)

    def step(self, images):
        from . import _lib
        if self.graph_mode and not self._graph_failed and not _lib.trace_is_enabled():
            if self._graph is not None and self._inputs_match(images):
                return self._replay(images)
            if self._graph is None and self.step_no >= self.GRAPH_WARMUP:
                if self.graph_mode == "auto":
                    self._probe(images)
                else:
                    # graph=True: with a reducer every rank must take the same branch at every fork (a rank that steps
                    # eagerly issues its bucket all-reduces as the buckets close, a replaying rank in index order)
                    want = self._graph_supported(images)
                    if self.reducer is not None:
                        want = self._agree(want, any_rank=False)
                    if want:
                        self._capture(images)
                        if self.reducer is not None and not self._agree(self._graph is not None, any_rank=False):
                            self._graph, self.graph_mode = None, False     # somebody's capture failed: everyone eager
                            self.opt.coef_dev = None
                    elif self.reducer is not None:
                        self.graph_mode = False
                if self._graph is not None and self._inputs_match(images):
                    return self._replay(images)
        return self._plain_step(images)

    def _plain_step(self, images):
        has = hasattr(self.opt, "coef_dev")                   # eager steps pass their scalars by value
        saved = self.opt.coef_dev if has else None
        if has:
            self.opt.coef_dev = None
        try:
            return self._eager_step(images, count_step=True)
        finally:
            if has:
                self.opt.coef_dev = saved

    def _eager_step(self, images, count_step=False, with_update=True):
        """One step inside THIS trainer's step context (layers.StepContext): the fused hand-overs of its forward and backward
        never meet those of another model stepped or evaluated in the same process."""
        with L.step_context(self.ctx):
            return self._eager_step_body(images, count_step, with_update)

    def _eager_step_body(self, images, count_step=False, with_update=True):
        self.model.train()
        if count_step:
            self.step_no += 1
            if self._graph is not None:
                self._since_capture += 1
        if self.reducer is not None:
            self.reducer.zero()                 # one memset of the flat gradient buffer
        else:
            self.opt.zero_grad(set_to_none=True)
        total, mean, count = self.loss(images)
        self.last_total = total.detach()        # triplet mean + kernel regularisers (what Keras reports as `loss`)
        # weight-gradient slab sums: queued, one launch for all (layers.conv_wgrad).  Needs every dw to stay untouched until
        # the flush: a fresh .grad (zero_grad(set_to_none)) or the reducer's in-place sinks — not an AccumulateGrad add_
        # and ONE gradient contribution per parameter (the regularisers' gradient folded into the KerasOptimizer launch, not
        # added by autograd)
        L.SLAB_DEFER[0] = L.SLAB_DEFER_ENABLED[0] and self._keras_opt and (self.reducer is None or self.reducer._direct)
        try:
            total.backward()
        finally:
            L.SLAB_DEFER[0] = False
            L.flush_slab_reduces()              # (with a reducer: what its buckets have not flushed already)
        # what the backward left unclaimed (BatchNorm-backward sums whose gradient got a second contribution, gradient planes of a
        # consumer that fell back to the fp32 kernel) was dropped and counted when the backward ended (StepContext.end_of_backward)
        self.ctx.end_of_backward()
        L._BN_FWD_STATS.clear()
        if self.reducer is not None:
            self.reducer.finish()
        if with_update:
            self._update()
        return mean.detach()

    def _update(self):
        self.opt.step()
        L.refresh_weight_planes(self.model)     # bf16 planes of the patch convs' kernels, one launch (layers.py)
        if self.averager is not None:
            # one more launch: eager steps pass the coefficient by value, a captured step reads it from the state row
            t = self.opt.iterations if self._keras_opt else self.step_no
            self.averager.update(t, self._state[10:11] if self._graph_state_live() else None)


class SiameseTrainer(TripletTrainer):
    """The Siamese training step (reference models.py:192-236 + tools/train.py:108-119: `model.fit` of SiameseNet.model with
    contrastive_loss on the first output) with TripletTrainer's machinery: its own step context, the weight-gradient slab sums
    deferred to one launch per flush, the KerasOptimizer's one-launch update with the kernel planes / ranges refreshed behind it,
    and — graph=True / 'auto' — the whole step (two branch forwards, pair distance, loss, backward with the two branches' gradient
    accumulation, optimizer) captured once into a HIP graph and replayed: ResNet50 at 256 pairs is 900 launches per step that the
    host needs 79 ms to enqueue against 85-89 ms of kernels (profiles/r05_final_bench_c3_kernels.txt) — any faster kernel makes the
    eager step host-bound.  `graph_probe` (graph='auto') reports the eager step's host work like TripletTrainer's.

    siamese_model: SiameseNet.model ([x1, x2] -> [distance, cls1, cls2]); loss_fn(y_true, distance) -> scalar (contrastive_loss).
    step(x1, x2, y) -> the loss of the step (detached)."""

    ANY_LOSS_CAPTURES = True

    def __init__(self, siamese_model, optimizer, loss_fn=None, seed=0, reducer=None, graph=None, averager=None):
        # two gradient contributions per shared parameter: autograd accumulates, no in-place sinks
        self._setup(siamese_model, optimizer, seed, reducer, graph, direct=False, averager=averager)
        self.last_triplets = None
        if loss_fn is None:
            from .losses_and_accuracies import contrastive_loss as loss_fn
        self.loss_fn = loss_fn

    def loss(self, inputs):
        x1, x2, y = inputs
        mean = self.loss_fn(y, self.model([x1, x2])[0])
        reg = L.regularization_loss(self.model, with_grad=not self._keras_opt)
        return (mean if reg is None else mean + reg), mean, None

    def step(self, x1, x2, y):
        return super().step((x1, x2, y))


class ProxyTrainer(TripletTrainer):
    """The training step of the proxy / classification losses with TripletTrainer's machinery: its own step context, the
    weight-gradient slab sums deferred to one launch per flush, the KerasOptimizer's one-launch update — the proxies are one more
    tensor of its single group, or a group of their own with a rate multiplier and a decay (optimizers.KerasOptimizer) — and, graph=True / 'auto', the whole step captured once into a HIP graph and replayed, the labels
    copied into a static buffer beside the images.

    base_model: images -> embeddings [N, E];  head: a proxies.ProxyHead whose parameter the optimizer (and the reducer) must hold;
    loss_params: a dict out of the mode's keys below, unknown keys are refused.  step(images, labels) -> the loss of the step
    (detached); labels: int32 device tensor [N] of global class indices in any order (outside [0, C): unlabelled).

    One proxy per class (ops.PROXY_LOSS_MODES; head.centers_per_class must be 1):
      'proxy_anchor'   Proxy-Anchor, Kim et al. 2020; dict(alpha, delta), defaults 32 and 0.1.
      'proxy_softmax'  CosFace, Wang et al. 2018, with margin 0 NormSoftmax; dict(scale, margin), defaults 64 and 0.35.
      last_pair_counts = int32 [3]: anchors with a positive term, labelled samples, violating anchors (include/embnet.h);
      last_triplets = (None, violating anchors [1]);  last_reg = None.
    Several centres per class (ops.MULTI_PROXY_LOSS_MODES; `centers`, where given, must be head.centers_per_class):
      'soft_triple'    SoftTriple, Qian et al. 2019; dict(scale, margin, gamma, tau, centers), defaults 20, 0.01, 0.1, 0.2.
      'arcface'        sub-centre ArcFace, Deng et al. 2019 / 2020; dict(scale, margin, centers), defaults 64, 0.5.
      last_pair_counts = int32 [3]: labelled samples, violating samples, samples on ArcFace's guard branch (0 for SoftTriple);
      last_triplets = (None, violating samples [1]);  last_reg = SoftTriple's centre regulariser (a device scalar, part of the
      loss), None for ArcFace.

    Under data parallelism each rank's loss covers its own batch against ALL proxies; the proxies are replicated, so the mean of the
    ranks' gradients — what the reducer forms — is the gradient of the mean of the ranks' losses, for the proxies as for the
    backbone.  (Proxy-Anchor's 1/|C+| is each rank's own: the mean is over the ranks' losses, not the loss of the pooled batch.)"""
    LOSS_MODES = {**ops.PROXY_LOSS_MODES, **ops.MULTI_PROXY_LOSS_MODES}
    LOSS_PARAMS = {mode: keys for mode, (_, keys) in LOSS_MODES.items()}
    ANY_LOSS_CAPTURES = True

    def __init__(self, base_model, head, optimizer, loss="proxy_anchor", loss_params=None, seed=0, reducer=None, graph=None,
                 averager=None):
        if loss not in self.LOSS_MODES:
            raise KeyError(loss)
        self.loss_params = self._checked_loss_params(loss, loss_params)
        self.multi = loss in ops.MULTI_PROXY_LOSS_MODES
        kc = self.loss_params.pop("centers", head.centers_per_class) if self.multi else 1
        if kc != head.centers_per_class:
            raise ValueError(f"ProxyTrainer: {loss!r} with {kc} centre(s) per class on a head of centers_per_class="
                             f"{head.centers_per_class}")
        if not any(q is head.proxies for g in optimizer.param_groups for q in g["params"]):
            raise ValueError("ProxyTrainer: the optimizer does not hold head.proxies (build it over the backbone's parameters "
                             "and the head's)")
        self.head, self.mode = head, loss
        # one gradient per parameter and step, the proxies' included
        self._setup(base_model, optimizer, seed, reducer, graph, direct=True, averager=averager)
        self.last_triplets = self.last_reg = None

    def loss(self, inputs):
        images, labels = inputs
        emb = self.model(images)
        fn = self.LOSS_MODES[self.mode][0]
        if self.multi:                                      # violating samples are counts[1]; SoftTriple's loss carries its reg
            mean, counts, *reg = fn(emb, self.head.proxies, labels, self.head.n_classes, **self.loss_params)
            self.last_reg = reg[0] if reg else None
            count = counts[1:2]
        else:
            mean, counts = fn(emb, self.head.proxies, labels, **self.loss_params)
            count = counts[2:3]                             # a slice view of the counts
        self.last_pair_counts = counts
        self.last_triplets = (None, count)
        reg = L.regularization_loss(self.model, with_grad=not self._keras_opt)
        return (mean if reg is None else mean + reg), mean, count

    def step(self, images, labels):
        if labels.dtype != torch.int32 or labels.dim() != 1 or labels.shape[0] != images.shape[0]:
            raise ValueError(f"ProxyTrainer.step: labels must be int32 [{images.shape[0]}] (got {labels.dtype} {tuple(labels.shape)})")
        return super().step((images, labels))


class XbmTrainer(TripletTrainer):
    """TripletTrainer with a cross-batch memory (xbm.CrossBatchMemory; Wang et al., CVPR 2020): the loss of a step is the parent
    mode's in-batch loss — any negatives_selection_mode — plus `weight` times the loss of the SAME embeddings against the memory
    (ops.XBM_LOSS_MODES: 'contrastive', the XBM paper's criterion, xbm_params = dict(margin), default 0.5; 'multi_similarity',
    xbm_params = dict(alpha, beta, base, epsilon), defaults 2, 50, 0.5, 0.1; 'circle', xbm_params = dict(m, gamma), defaults 0.4
    and 80, whose first two counts are the pairs with a positive weight; unknown keys are refused).  The XBM recipe: the batch's
    detached embeddings are enqueued first, then the batch is scored against the whole ring with each sample's own slot excluded.
    The ring, its write position and the enqueue live on the device (include/embnet.h): no host synchronisation, and with
    graph=True / 'auto' the step — enqueue and memory loss included — is captured once and replayed like ProxyTrainer's, the labels
    copied into a static buffer beside the images; a replayed step is bit-identical to an eager one.

    step(images, labels): labels int32 device tensor [N] of global class indices, rows class-contiguous as for TripletTrainer.
    While step_no < start_iteration nothing of the memory runs — no enqueue, no memory loss: the step is TripletTrainer's, bit for
    bit, and runs eagerly (the capture waits until the memory is live).  last_pair_counts / last_triplets are the parent's;
    last_xbm_counts = int32 [4]: kept positives, kept negatives, active anchors, labelled memory slots (None before the memory is live).
    Under data parallelism each rank keeps a memory of its own batches: nothing is gathered, the reducer averages the ranks'
    gradients as it does the in-batch loss's.  The memory is not checkpointed: after a resume it refills."""

    def __init__(self, base_model, optimizer, k_classes, k_samples, margin=0.5, negatives_selection_mode="semihard", seed=0,
                 reducer=None, graph=None, loss_params=None, memory=None, xbm_loss="contrastive", xbm_params=None, weight=1.0,
                 start_iteration=0, averager=None):
        super().__init__(base_model, optimizer, k_classes, k_samples, margin, negatives_selection_mode, seed, reducer, graph,
                         loss_params, averager=averager)
        if xbm_loss not in ops.XBM_LOSS_MODES:
            raise KeyError(xbm_loss)
        keys = ops.XBM_LOSS_MODES[xbm_loss][1]
        unknown = set(xbm_params or {}) - set(keys)
        if unknown:
            raise ValueError(f"xbm_params: unknown keys {sorted(unknown)} for {xbm_loss!r} ({', '.join(keys)})")
        if memory is None or not hasattr(memory, "enqueue"):
            raise ValueError("XbmTrainer: memory must be an xbm.CrossBatchMemory")
        if memory.size < self.p * self.k:
            raise ValueError(f"XbmTrainer: a memory of {memory.size} slots is smaller than a batch of {self.p * self.k}")
        if int(start_iteration) < 0:
            raise ValueError(f"XbmTrainer: start_iteration={start_iteration} must not be negative")
        self.memory, self.xbm_loss, self.xbm_params = memory, xbm_loss, dict(xbm_params or {})
        self.weight, self.start_iteration = float(weight), int(start_iteration)
        self.last_xbm_counts, self._xbm_live, self._g_xbm_counts = None, False, None

    def loss(self, inputs):
        images, labels = inputs
        if images.shape[0] != self.p * self.k:
            raise ValueError(f"batch of {images.shape[0]} images != k_classes*k_samples = {self.p * self.k}")
        emb = self.model(images)
        if emb.shape[1] != self.memory.embedding_size:
            raise ValueError(f"XbmTrainer: embeddings of width {emb.shape[1]} do not match a memory of width "
                             f"{self.memory.embedding_size}")
        mean, count = self.batch_loss(emb)
        if self._xbm_live:
            slots = self.memory.enqueue(emb, labels)        # first the batch's own (detached) copies, then the whole ring
            xbm_mean, self.last_xbm_counts = ops.XBM_LOSS_MODES[self.xbm_loss][0](
                emb, labels, self.memory.feats, self.memory.labels, slots, **self.xbm_params)
            mean = mean + self.weight * xbm_mean
        reg = L.regularization_loss(self.model, with_grad=not self._keras_opt)
        return (mean if reg is None else mean + reg), mean, count

    def _graph_supported(self, inputs):
        return self.step_no >= self.start_iteration and super()._graph_supported(inputs)

    def _capture(self, inputs):
        super()._capture(inputs)
        self._g_xbm_counts = self.last_xbm_counts           # the replayed step's (static) output tensor

    def _replay(self, inputs):
        out = super()._replay(inputs)
        self.last_xbm_counts = self._g_xbm_counts           # an eager step in between re-bound it
        return out

    def step(self, images, labels):
        if labels.dtype != torch.int32 or labels.dim() != 1 or labels.shape[0] != images.shape[0]:
            raise ValueError(f"XbmTrainer.step: labels must be int32 [{images.shape[0]}] (got {labels.dtype} {tuple(labels.shape)})")
        self._xbm_live = self.step_no >= self.start_iteration
        if not self._xbm_live:
            return self._plain_step((images, labels))       # the parent's eager step; the capture waits for the memory
        return super().step((images, labels))
