"""Tensor-level entry points over the C ABI (include/embnet.h).

PyTorch is plumbing here: it owns device memory, the stream and the autograd
tape; every forward/backward below is one or two launches of hand-written HIP
kernels from libembnet_hip.so.  Nothing in this module computes on the CPU or
through torch's own operators.
"""
import ctypes

import torch

from . import _lib
from ._lib import check, f32, ptr, stream

MINING_MODES = {"semihard": 0, "hardest": 1, "random_hard": 2}


def _prep(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _new(shape, like, dtype=torch.float32):
    return torch.empty(shape, device=like.device, dtype=dtype)


# --------------------------------------------------------------------------- distances / mining
def pairwise_distances(x, squared=False):
    """[n,e] -> [n,n] Euclidean matrix with sklearn semantics (datagenerators.py:219)."""
    x = _prep(x.detach())
    n, e = x.shape
    lib = _lib.lib()
    ws = _new((max(lib.embnet_pairwise_workspace_bytes(n, e) // 4, 1),), x)
    d = _new((n, n), x)
    check(lib.embnet_pairwise_dist_f32(ptr(x), n, e, ptr(d), int(bool(squared)), ptr(ws),
                                       ws.numel() * 4, stream()))
    return d


def mine_triplets(dist, k_classes, k_samples, margin, mode, seed=0, with_candidates=False):
    """Online mining on a class-contiguous distance matrix (datagenerators.py:225-250).

    Returns (triplets [max_t,3] int32, count [1] int32, selected [pairs] int32[, cand_mask]).
    Only the first count[0] rows of `triplets` are live; nothing is copied to the host.
    """
    dist = _prep(dist)
    lib = _lib.lib()
    p, k = int(k_classes), int(k_samples)
    n = p * k
    if dist.shape != (n, n):
        raise _lib.EmbnetError(f"distance matrix {tuple(dist.shape)} != ({n},{n}) for {p}x{k}")
    max_t = lib.embnet_mine_max_triplets(p, k)
    trip = _new((max_t, 3), dist, torch.int32)
    count = _new((1,), dist, torch.int32)
    npairs = p * (k * (k - 1) // 2)
    sel = _new((max(npairs, 1),), dist, torch.int32)
    mask = _new((max(npairs, 1), (n - k + 31) // 32), dist, torch.int32) if with_candidates else None
    check(lib.embnet_mine_triplets(ptr(dist), p, k, f32(margin), MINING_MODES[mode],
                                   int(seed) & (2 ** 64 - 1), ptr(trip), ptr(count),
                                   ptr(sel), ptr(mask), stream()))
    return (trip, count, sel, mask) if with_candidates else (trip, count, sel)


def batch_hard(dist, k_classes, k_samples):
    """Hermans batch-hard (build-defined): [n,3] triplets, one per anchor, + count."""
    dist = _prep(dist)
    p, k = int(k_classes), int(k_samples)
    n = p * k
    trip = _new((n, 3), dist, torch.int32)
    count = _new((1,), dist, torch.int32)
    check(_lib.lib().embnet_batch_hard(ptr(dist), p, k, ptr(trip), ptr(count), stream()))
    return trip, count


# --------------------------------------------------------------------------- triplet hinge
class _TripletHinge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_pred, margin):
        y = _prep(y_pred)
        t, e3 = y.shape
        if e3 % 3:
            raise _lib.EmbnetError(f"triplet_loss: last dim {e3} is not 3*E")
        loss = _new((t,), y)
        check(_lib.lib().embnet_triplet_hinge_fwd(ptr(y), t, e3 // 3, f32(margin), ptr(loss), stream()))
        ctx.save_for_backward(y)
        ctx.margin = margin
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (y,) = ctx.saved_tensors
        t, e3 = y.shape
        dy = torch.empty_like(y)
        check(_lib.lib().embnet_triplet_hinge_bwd(ptr(y), ptr(_prep(dloss)), t, e3 // 3, f32(ctx.margin),
                                                  ptr(dy), stream()))
        return dy, None


def triplet_hinge(y_pred, margin):
    return _TripletHinge.apply(y_pred, float(margin))


class _TripletGatherLoss(torch.autograd.Function):
    """mean_t max(|a-p|^2 - |a-n|^2 + m, 0) over the live triplets, rows gathered from emb."""

    @staticmethod
    def forward(ctx, emb, triplets, count, margin):
        emb = _prep(emb)
        n, e = emb.shape
        max_t = triplets.shape[0]
        loss = _new((max_t,), emb)
        act = _new((max_t,), emb)
        mean = _new((), emb)
        check(_lib.lib().embnet_triplet_gather_fwd(ptr(emb), n, e, ptr(triplets), ptr(count), max_t,
                                                   f32(margin), ptr(loss), ptr(act), ptr(mean), stream()))
        ctx.save_for_backward(emb, triplets, count, act)
        ctx.mark_non_differentiable(loss)
        return mean, loss

    @staticmethod
    def backward(ctx, dmean, _dloss):
        emb, triplets, count, act = ctx.saved_tensors
        n, e = emb.shape
        demb = torch.empty_like(emb)
        up = _prep(dmean)
        check(_lib.lib().embnet_triplet_gather_bwd(ptr(emb), n, e, ptr(triplets), ptr(count),
                                                   triplets.shape[0], ptr(act), ptr(up), ptr(demb), stream()))
        return demb, None, None, None


def triplet_gather_loss(emb, triplets, count, margin):
    """-> (mean loss scalar [autograd], per-triplet losses [max_t])."""
    return _TripletGatherLoss.apply(emb, triplets, count, float(margin))


_FUSED_WS = {}


def _ticket_workspace(cache, where, shape, bytes_fn, dtype, device):
    """bytes_fn(*shape) bytes (32 where a shape is out of range and the call about to be refused), zero-filled on the first call
    under where + shape and kept: the kernels re-arm the arrival ticket in it."""
    if where + shape not in cache:
        cache[where + shape] = torch.zeros(max(bytes_fn(*shape), 32) // dtype.itemsize, dtype=dtype, device=device)
    return cache[where + shape]


def fused_loss_supported(k_classes, k_samples, e):
    return bool(_lib.lib().embnet_fused_loss_supported(int(k_classes), int(k_samples), int(e)))


class _FusedTripletLoss(torch.autograd.Function):
    """distance matrix + mining + gathered hinge + mean in one launch (embnet_fused_triplet_loss_fwd); the backward is
    the gather form's (embnet_triplet_gather_bwd), since the outputs are the same."""

    @staticmethod
    def forward(ctx, emb, p, k, margin, mode, seed, seed_dev=None):
        emb = _prep(emb)
        n, e = emb.shape
        lib = _lib.lib()
        code = 3 if mode == "batch_hard" else MINING_MODES[mode]
        rows = n if code == 3 else lib.embnet_mine_max_triplets(p, k)
        trip = _new((rows, 3), emb, torch.int32)
        count = _new((1,), emb, torch.int32)
        sel = _new((max(p * (k * (k - 1) // 2), 1),), emb, torch.int32)
        loss, act, mean = _new((rows,), emb), _new((rows,), emb), _new((), emb)
        ws = _ticket_workspace(_FUSED_WS, (emb.device.index, stream()), (p, k), lib.embnet_fused_loss_workspace_bytes, torch.float32,
                               emb.device)
        check(lib.embnet_fused_triplet_loss_fwd(ptr(emb), p, k, e, f32(margin), code, int(seed) & (2 ** 64 - 1),
                                                seed_dev, ptr(trip),
                                                ptr(count), ptr(sel), ptr(loss), ptr(act), ptr(mean), ptr(ws),
                                                ws.numel() * 4, stream()))
        ctx.save_for_backward(emb, trip, count, act)
        ctx.mark_non_differentiable(loss, trip, count)
        ctx.set_materialize_grads(False)                    # no zero tensors (three fill launches) for the outputs nobody differentiates
        return mean, loss, trip, count

    @staticmethod
    def backward(ctx, dmean, _dloss, _dtrip, _dcount):
        emb, trip, count, act = ctx.saved_tensors
        n, e = emb.shape
        demb = torch.empty_like(emb)
        check(_lib.lib().embnet_triplet_gather_bwd(ptr(emb), n, e, ptr(trip), ptr(count), trip.shape[0], ptr(act),
                                                   ptr(_prep(dmean)), ptr(demb), stream()))
        return demb, None, None, None, None, None, None


def fused_triplet_loss(emb, k_classes, k_samples, margin, mode, seed=0, seed_dev=None):
    """-> (mean loss [autograd], per-triplet losses, triplets [rows,3] int32, count [1] int32); one launch.
    seed_dev: device address of a uint64 seed that overrides `seed` (graph replays, see train_step.TripletTrainer)."""
    return _FusedTripletLoss.apply(emb, int(k_classes), int(k_samples), float(margin), mode, int(seed), seed_dev)


BATCH_ALL_PATHS = {"auto": 0, "per_class": 1, "distance_matrix": 2}
MS_PATHS = {"auto": 0, "per_class": 1, "similarity_matrix": 2}
SUPCON_PATHS = {"auto": 0, "per_class": 1, "similarity_matrix": 2}
SUPCON_DENOMINATORS = {"all": 1, "negatives": 2}
AP_PATHS = {"auto": 0, "per_class": 1, "similarity_matrix": 2}
CIRCLE_PATHS = {"auto": 0, "per_class": 1, "similarity_matrix": 2}


def _supcon_scalars(temperature, denominator):
    if denominator not in SUPCON_DENOMINATORS:
        raise _lib.EmbnetError(f"supcon_loss: denominator {denominator!r} is not one of {sorted(SUPCON_DENOMINATORS)}")
    return f32(temperature), SUPCON_DENOMINATORS[denominator]


# The losses over a class-contiguous block (csrc/pair_loss.h), by the name of their public function.  Every forward entry point
# takes (emb, p, k, e, *scalars, path, pair weights [N,N], *outputs, mean, workspace, bytes, stream); every backward
# (emb, n, e, pair weights, [outputs[0]], upstream, demb, stream).
#   name: (forward, workspace size, path table, Python scalars -> C arguments, outputs beside the mean as (shape, dtype),
#          backward, whether it takes outputs[0])
_PAIR_LOSSES = {
    "batch_all_triplet_loss": ("embnet_batch_all_loss_fwd", "embnet_batch_all_workspace_bytes", BATCH_ALL_PATHS,
                               lambda margin: (f32(margin),), (((1,), torch.int32), ((), torch.float32)),
                               "embnet_batch_all_loss_bwd", True),
    "multi_similarity_loss": ("embnet_ms_loss_fwd", "embnet_ms_loss_workspace_bytes", MS_PATHS,
                              lambda *abbe: tuple(map(f32, abbe)), (((4,), torch.int32),), "embnet_ms_loss_bwd", False),
    "supcon_loss": ("embnet_supcon_loss_fwd", "embnet_supcon_loss_workspace_bytes", SUPCON_PATHS, _supcon_scalars,
                    (((2,), torch.int32),), "embnet_ms_loss_bwd", False),     # demb = (g / N)(G + G^T) X is MS's backward
    "fast_ap_loss": ("embnet_fast_ap_loss_fwd", "embnet_fast_ap_loss_workspace_bytes", AP_PATHS, lambda bins: (bins,),
                     (((2,), torch.int32),), "embnet_ms_loss_bwd", False),
    "smooth_ap_loss": ("embnet_smooth_ap_loss_fwd", "embnet_smooth_ap_loss_workspace_bytes", AP_PATHS,
                       lambda temperature: (f32(temperature),), (((2,), torch.int32),), "embnet_ms_loss_bwd", False),
    "circle_loss": ("embnet_circle_loss_fwd", "embnet_circle_loss_workspace_bytes", CIRCLE_PATHS,
                    lambda m, gamma: (f32(m), f32(gamma)), (((3,), torch.int32),), "embnet_ms_loss_bwd", False),
}
_PAIR_WS = {}


class _PairLoss(torch.autograd.Function):
    """A loss of _PAIR_LOSSES (include/embnet.h): one forward launch on the per-class path, pair matrix + sweep above it; one
    backward launch.  The pair weights stay saved for the backward."""

    @staticmethod
    def forward(ctx, emb, loss, p, k, scalars, path):
        fwd, ws_bytes, paths, marshal, outputs, bwd, bwd_takes_output = _PAIR_LOSSES[loss]
        emb = _prep(emb)
        n, e = emb.shape
        if n != p * k:
            raise _lib.EmbnetError(f"{loss}: {n} rows != k_classes*k_samples = {p}*{k}")
        scalars = marshal(*scalars)
        lib = _lib.lib()
        g = _new((n, n), emb)
        outs = [_new(shape, emb, dtype) for shape, dtype in outputs]
        mean = _new((), emb)
        ws = _ticket_workspace(_PAIR_WS, (loss, emb.device.index, stream()), (p, k, e), getattr(lib, ws_bytes), torch.float32, emb.device)
        check(getattr(lib, fwd)(ptr(emb), p, k, e, *scalars, paths[path], ptr(g), *map(ptr, outs), ptr(mean), ptr(ws),
                                ws.numel() * 4, stream()))
        ctx.bwd = bwd
        ctx.save_for_backward(emb, g, *(outs[:1] if bwd_takes_output else ()))
        ctx.mark_non_differentiable(*outs, g)
        ctx.set_materialize_grads(False)                    # no zero tensors for the outputs nobody differentiates
        return (mean, *outs, g)

    @staticmethod
    def backward(ctx, dmean, *_):
        if dmean is None:
            return (None,) * 6
        emb, g, *output = ctx.saved_tensors
        n, e = emb.shape
        demb = torch.empty_like(emb)
        check(getattr(_lib.lib(), ctx.bwd)(ptr(emb), n, e, ptr(g), *map(ptr, output), ptr(_prep(dmean)), ptr(demb), stream()))
        return (demb,) + (None,) * 5


def batch_all_triplet_loss(emb, k_classes, k_samples, margin, path="auto", return_weights=False):
    """Batch-all triplet loss over a class-contiguous [P*K, E] block: the mean of b = d(a,p) - d(a,n) + margin over every
    valid triplet with b > 0 (d squared L2).  -> (mean [autograd], n_active int32 [1], frac_active []) on the device, no host
    synchronisation; return_weights adds the pair-weight matrix W [N,N] the backward uses.  path: 'auto', 'per_class' or
    'distance_matrix' (include/embnet.h)."""
    out = _PairLoss.apply(emb, "batch_all_triplet_loss", int(k_classes), int(k_samples), (float(margin),), path)
    return out if return_weights else out[:3]


def multi_similarity_loss(emb, k_classes, k_samples, alpha=2.0, beta=50.0, base=0.5, epsilon=0.1, path="auto",
                          return_weights=False):
    """Multi-similarity loss (Wang et al., CVPR 2019) over a class-contiguous [P*K, E] block, on the dot-product similarities
    S = X X^T: negatives with S_in + epsilon > min_p S_ip and positives with max_n S_in + epsilon > S_ip are kept, and
    l_i = log(1 + sum_p e^{-alpha (S_ip - base)}) / alpha + log(1 + sum_n e^{beta (S_in - base)}) / beta, mean over all N anchors
    (include/embnet.h has the rounding forms).  -> (mean [autograd], counts int32 [4] = kept positives, kept negatives, active
    anchors, kept pairs) on the device, no host synchronisation; return_weights adds the pair-weight matrix G [N,N] the
    backward uses.  path: 'auto', 'per_class' or 'similarity_matrix'."""
    out = _PairLoss.apply(emb, "multi_similarity_loss", int(k_classes), int(k_samples),
                          (float(alpha), float(beta), float(base), float(epsilon)), path)
    return out if return_weights else out[:2]


def supcon_loss(emb, k_classes, k_samples, temperature=0.1, denominator="all", path="auto", return_weights=False):
    """The softmax / InfoNCE family over a class-contiguous [P*K, E] block, on the logits t = S / temperature, S = X X^T.
    denominator 'all': SupCon (Khosla et al. 2020, L_out), l_i = lse_{a != i} t_ia - mean_p t_ip; 'negatives': NT-Xent as
    pytorch-metric-learning has it, l_i = mean_p (log(e^{t_ip} + sum_n e^{t_in}) - t_ip); mean over all N anchors (include/embnet.h
    has the rounding and the stable forms).  -> (mean [autograd], counts int32 [2] = positive pairs, violating anchors: those
    whose hardest negative is at least as similar as their hardest positive) on the device, no host synchronisation;
    return_weights adds the pair-weight matrix G [N,N] the backward uses.  path: 'auto', 'per_class' or 'similarity_matrix'."""
    out = _PairLoss.apply(emb, "supcon_loss", int(k_classes), int(k_samples), (float(temperature), denominator), path)
    return out if return_weights else out[:2]


def fast_ap_loss(emb, k_classes, k_samples, bins=10, path="auto", return_weights=False):
    """FastAP (Cakir et al., CVPR 2019) over a class-contiguous [P*K, E] block of L2-normalised rows: each anchor's distances
    d = 2 - 2 S, S = X X^T, are soft-binned into histograms h+ / h- over the bins + 1 centres l * 4 / bins (triangular pulse), and
    l_i = 1 - (1/(K-1)) sum_l h+_l H+_l / H_l with H+, H the running sums; mean over all N anchors (include/embnet.h has the
    rounding form and the pair weights).  bins: a whole number in [2, 64].  -> (mean [autograd], counts int32 [2] = positive
    pairs, violating anchors: those whose hardest negative is at least as similar as their hardest positive) on the device, no
    host synchronisation; return_weights adds the pair-weight matrix G [N,N] the backward uses.  path: 'auto', 'per_class' or
    'similarity_matrix'."""
    if isinstance(bins, bool) or int(bins) != bins:
        raise _lib.EmbnetError(f"fast_ap_loss: bins={bins!r} is not a whole number")
    out = _PairLoss.apply(emb, "fast_ap_loss", int(k_classes), int(k_samples), (int(bins),), path)
    return out if return_weights else out[:2]


def smooth_ap_loss(emb, k_classes, k_samples, temperature=0.01, path="auto", return_weights=False):
    """Smooth-AP (Brown et al., ECCV 2020) over a class-contiguous [P*K, E] block: the ranks in average precision with the step
    replaced by a sigmoid of temperature tau, l_i = 1 - (1/(K-1)) sum_p R_p / Q_p, R_p = 1 + sum_{q != p} sigma((S_iq - S_ip) / tau)
    over the other positives and Q_p the same sum over every other column; mean over all N anchors (include/embnet.h has the
    rounding form and the pair weights).  K <= 65.  -> (mean [autograd], counts int32 [2] = positive pairs, violating anchors) on
    the device, no host synchronisation; return_weights adds the pair-weight matrix G [N,N] the backward uses.  path: 'auto',
    'per_class' or 'similarity_matrix'."""
    out = _PairLoss.apply(emb, "smooth_ap_loss", int(k_classes), int(k_samples), (float(temperature),), path)
    return out if return_weights else out[:2]


def circle_loss(emb, k_classes, k_samples, m=0.4, gamma=80.0, path="auto", return_weights=False):
    """Circle loss (Sun et al., CVPR 2020; the pair-wise form) over a class-contiguous [P*K, E] block, on S = X X^T: every pair is
    weighted by its distance from its optimum, alpha+ = [1 + m - S_ip]+ and alpha- = [S_in + m]+ (constants of the backward), and
    l_i = softplus(lse_p(-gamma alpha+ (S_ip - (1 - m))) + lse_n(gamma alpha- (S_in - m))), mean over all N anchors
    (include/embnet.h has the rounding and the stable forms).  0 <= m <= 1, gamma > 0; the defaults are pytorch-metric-learning's,
    the paper's face setting is 0.25 / 256.  -> (mean [autograd], counts int32 [3] = positive pairs, violating anchors: those
    whose hardest negative is at least as similar as their hardest positive, negatives with alpha- > 0) on the device, no host
    synchronisation; return_weights adds the pair-weight matrix G [N,N] the backward uses.  path: 'auto', 'per_class' or
    'similarity_matrix'."""
    out = _PairLoss.apply(emb, "circle_loss", int(k_classes), int(k_samples), (float(m), float(gamma)), path)
    return out if return_weights else out[:2]


MARGIN_PATHS = {"auto": 0, "per_class": 1, "distance_matrix": 2}


class _MarginLoss(torch.autograd.Function):
    """embnet_margin_loss_fwd / _bwd (include/embnet.h): the sampler and the loss in one forward launch on the per-class path,
    distance matrix + sweep above it; one backward launch.  Beside _PairLoss because of the seed, the triplet rows and sample_w."""

    @staticmethod
    def forward(ctx, emb, p, k, scalars, seed, seed_dev, path, with_sample_w):
        emb = _prep(emb)
        n, e = emb.shape
        if n != p * k:
            raise _lib.EmbnetError(f"margin_loss: {n} rows != k_classes*k_samples = {p}*{k}")
        if path not in MARGIN_PATHS:
            raise _lib.EmbnetError(f"margin_loss: path {path!r} is not one of {sorted(MARGIN_PATHS)}")
        lib = _lib.lib()
        w = _new((n, n), emb)
        sample_w = _new((n, n), emb) if with_sample_w else None
        counts = _new((3,), emb, torch.int32)
        trip = _new((n * max(k - 1, 0), 3), emb, torch.int32)
        mean = _new((), emb)
        ws = _ticket_workspace(_PAIR_WS, ("margin_loss", emb.device.index, stream()), (p, k, e), lib.embnet_margin_loss_workspace_bytes,
                               torch.float32, emb.device)
        check(lib.embnet_margin_loss_fwd(ptr(emb), p, k, e, *map(f32, scalars), int(seed) & (2 ** 64 - 1), seed_dev, MARGIN_PATHS[path],
                                         ptr(w), ptr(counts), ptr(trip), ptr(sample_w), ptr(mean), ptr(ws), ws.numel() * 4, stream()))
        ctx.save_for_backward(emb, w, counts)
        outs = (counts, trip, w) + ((sample_w,) if with_sample_w else ())
        ctx.mark_non_differentiable(*outs)
        ctx.set_materialize_grads(False)                    # no zero tensors for the outputs nobody differentiates
        return (mean, *outs)

    @staticmethod
    def backward(ctx, dmean, *_):
        if dmean is None:
            return (None,) * 8
        emb, w, counts = ctx.saved_tensors
        n, e = emb.shape
        demb = torch.empty_like(emb)
        check(_lib.lib().embnet_margin_loss_bwd(ptr(emb), n, e, ptr(w), ptr(counts), ptr(_prep(dmean)), ptr(demb), stream()))
        return (demb,) + (None,) * 7


def margin_loss(emb, k_classes, k_samples, beta=1.2, alpha=0.2, cutoff=0.5, nonzero_loss_cutoff=1.4, seed=0, seed_dev=None,
                path="auto", return_weights=False):
    """Distance-weighted sampling with the margin loss (Wu et al., ICCV 2017) over a class-contiguous [P*K, E] block of unit rows:
    every anchor draws one negative per positive, with replacement, from the other-class rows at Euclidean distance D <
    nonzero_loss_cutoff with weight 1 / q(max(D, cutoff)), q the density of pairwise distances on the unit sphere, and pays
    [D_ap - beta + alpha]+ + [beta - D_an + alpha]+; the mean runs over the A positive hinges (include/embnet.h has the rounding
    form, the draws' keying and the sampler's summation order).  0 < cutoff < nonzero_loss_cutoff < 2, alpha >= 0; the defaults are
    the paper's.  seed: the draws' key; seed_dev: device address of a uint64 that overrides it (graph replays).
    -> (mean [autograd], counts int32 [3] = active positive hinges, active negative hinges, A, triplets int32 [N (K-1), 3] =
    (anchor, positive, drawn negative)) on the device, no host synchronisation; return_weights adds the pair-weight matrix W [N,N]
    the backward uses and the sampling weights [N,N] (a row of zeros: the anchor had no eligible negative and drew uniformly).
    path: 'auto', 'per_class' or 'distance_matrix'."""
    out = _MarginLoss.apply(emb, int(k_classes), int(k_samples),
                            (float(beta), float(alpha), float(cutoff), float(nonzero_loss_cutoff)), int(seed), seed_dev, path,
                            bool(return_weights))
    return out if return_weights else out[:3]


def distance_weighted_triplets(emb, k_classes, k_samples, cutoff=0.5, nonzero_loss_cutoff=1.4, seed=0):
    """The miner of margin_loss on its own: -> (triplets int32 [N (K-1), 3], count int32 [1] = N (K-1)), no gradient; the rows
    are fit for triplet_gather_loss.  The draws depend on the embeddings, the two cutoffs and the seed only, so they equal
    margin_loss's for the same seed."""
    with torch.no_grad():
        trip = margin_loss(emb.detach(), k_classes, k_samples, cutoff=cutoff, nonzero_loss_cutoff=nonzero_loss_cutoff, seed=seed)[2]
    return trip, torch.full((1,), trip.shape[0], dtype=torch.int32, device=trip.device)


# The training modes (TripletTrainer's negatives_selection_mode) whose loss is one of the above over the whole batch; they have no
# triplet rows ('distance_weighted' apart: its third result is the rows it drew, and it takes the step's seed), a device count stands
# where the triplet count does.
#   mode: (function, the loss_params it takes or None = it takes `margin`, the element of its counts that is that count or
#          None = the counts are the count; with an element the trainer keeps all of them as last_pair_counts)
PAIR_LOSS_MODES = {
    "batch_all": (batch_all_triplet_loss, None, None),                                          # n_active
    "multi_similarity": (multi_similarity_loss, ("alpha", "beta", "base", "epsilon"), 3),       # kept pairs
    "supcon": (supcon_loss, ("temperature", "denominator"), 1),                                 # violating anchors
    "fast_ap": (fast_ap_loss, ("bins",), 1),                                                    # violating anchors
    "smooth_ap": (smooth_ap_loss, ("temperature",), 1),                                         # violating anchors
    "circle": (circle_loss, ("m", "gamma"), 1),                                                 # violating anchors
    "distance_weighted": (margin_loss, ("beta", "alpha", "cutoff", "nonzero_loss_cutoff"), 2),  # active hinges A
}


# --------------------------------------------------------------------------- losses on learnable class proxies (csrc/proxy_loss.hip)
PROXY_PATHS = {"auto": 0, "small": 1, "matrix": 2}
PROXY_KINDS = {"proxy_anchor_loss": 1, "proxy_softmax_loss": 2}      # EMBNET_PROXY_ANCHOR, EMBNET_PROXY_SOFTMAX
_PROXY_WS = {}


def _int32_labels(who, name, labels, n):
    if not torch.is_tensor(labels) or labels.dtype != torch.int32 or tuple(labels.shape) != (n,):
        raise _lib.EmbnetError(f"{who}: {name} must be an int32 tensor of {n} entries")
    return labels.contiguous()


def _proxy_width(loss, name, w, e):                         # the first check of the losses on proxies and on centres ...
    if w.dim() != 2 or w.shape[1] != e:
        raise _lib.EmbnetError(f"{loss}: {name} {tuple(w.shape)} do not match embeddings of width {e}")


def _proxy_labels_and_path(loss, labels, n, path):          # ... and their last two -> the labels, contiguous
    labels = _int32_labels(loss, "labels", labels, n)
    if path not in PROXY_PATHS:
        raise _lib.EmbnetError(f"{loss}: path {path!r} is not one of {sorted(PROXY_PATHS)}")
    return labels


class _ProxyLoss(torch.autograd.Function):
    """embnet_proxy_loss_fwd / _bwd (include/embnet.h): a prep launch and one forward launch on the small path, prep + D + sweep
    above it; three backward launches.  G [c,n] (Proxy-Anchor) or [n,c] (CosFace) and q stay saved for the backward."""

    @staticmethod
    def forward(ctx, emb, proxies, labels, loss, a, b, path):
        emb, proxies = _prep(emb), _prep(proxies)
        n, e = emb.shape
        c = proxies.shape[0]
        _proxy_width(loss, "proxies", proxies, e)
        labels = _proxy_labels_and_path(loss, labels, n, path)
        kind = PROXY_KINDS[loss]
        lib = _lib.lib()
        g = _new((c, n) if kind == 1 else (n, c), emb)
        q, counts, mean = _new((c,), emb), _new((3,), emb, torch.int32), _new((), emb)
        ws = _ticket_workspace(_PROXY_WS, (emb.device.index, stream()), (n, c, e), lib.embnet_proxy_loss_workspace_bytes, torch.float64,
                               emb.device)
        check(lib.embnet_proxy_loss_fwd(ptr(emb), ptr(proxies), ptr(labels), n, c, e, kind, f32(a), f32(b), PROXY_PATHS[path],
                                        ptr(g), ptr(q), ptr(counts), ptr(mean), ptr(ws), ws.numel() * 8, stream()))
        ctx.kind, ctx.ws = kind, ws
        ctx.save_for_backward(emb, proxies, g, q)
        ctx.mark_non_differentiable(counts, g)
        ctx.set_materialize_grads(False)                    # no zero tensors for the outputs nobody differentiates
        return mean, counts, g

    @staticmethod
    def backward(ctx, dmean, *_):
        if dmean is None:
            return (None,) * 7
        emb, proxies, g, q = ctx.saved_tensors
        n, e = emb.shape
        c = proxies.shape[0]
        demb, dproxies = torch.empty_like(emb), torch.empty_like(proxies)
        check(_lib.lib().embnet_proxy_loss_bwd(ptr(emb), ptr(proxies), n, c, e, ctx.kind, ptr(g), ptr(q), ptr(_prep(dmean)),
                                               ptr(demb), ptr(dproxies), ptr(ctx.ws), ctx.ws.numel() * 8, stream()))
        return (demb, dproxies) + (None,) * 5


def proxy_anchor_loss(emb, proxies, labels, alpha=32.0, delta=0.1, path="auto", return_weights=False):
    """Proxy-Anchor loss (Kim et al., CVPR 2020) of embeddings [N,E] against learnable proxies [C,E], labels int32 [N] of global
    class indices in any order (outside [0, C): unlabelled, ignored).  S_ci = x_i . w_c / |w_c| (the embeddings as they are),
    loss = mean over the classes present of log(1 + sum_{i in c} e^{-alpha (S_ci - delta)}) + mean over all C classes of
    log(1 + sum_{i labelled, not in c} e^{alpha (S_ci + delta)}) (include/embnet.h has the rounding and the stable forms).
    -> (mean [autograd w.r.t. emb and proxies], counts int32 [3] = classes present, labelled samples, violating anchors: the
    present classes whose hardest negative is at least as similar as their hardest positive) on the device, no host
    synchronisation; return_weights adds G [C,N] = dloss/dS.  path: 'auto', 'small' or 'matrix'."""
    out = _ProxyLoss.apply(emb, proxies, labels, "proxy_anchor_loss", float(alpha), float(delta), path)
    return out if return_weights else out[:2]


def proxy_softmax_loss(emb, proxies, labels, scale=64.0, margin=0.35, path="auto", return_weights=False):
    """CosFace (Wang et al., CVPR 2018: the large-margin cosine loss) of embeddings [N,E] against learnable proxies [C,E], labels
    int32 [N] as in proxy_anchor_loss; margin = 0 is NormSoftmax (Zhai & Wu 2019).  t_ic = scale (S_ic - margin [c = y_i]),
    loss = mean over the labelled samples of lse_c t_ic - t_iy (include/embnet.h has the rounding and the stable forms).
    -> (mean [autograd w.r.t. emb and proxies], counts int32 [3] = labelled samples, labelled samples, violating anchors: the
    samples with another class's proxy at least as similar as their own) on the device, no host synchronisation; return_weights
    adds G [N,C] = dloss/dS.  path: 'auto', 'small' or 'matrix'."""
    out = _ProxyLoss.apply(emb, proxies, labels, "proxy_softmax_loss", float(scale), float(margin), path)
    return out if return_weights else out[:2]


# --------------------------------------------------------------------------- losses on several centres per class (csrc/multi_proxy_loss.hip)
MPROXY_KINDS = {"soft_triple_loss": 1, "arcface_loss": 2}            # EMBNET_MPROXY_SOFT_TRIPLE, EMBNET_MPROXY_ARCFACE
_MPROXY_WS = {}


class _MultiProxyLoss(torch.autograd.Function):
    """embnet_multi_proxy_loss_fwd / _bwd (include/embnet.h): a prep launch, the regulariser's where SoftTriple has one, and one
    forward launch on the small path, D + sweep above it; the proxy losses' backward launches, one more with the regulariser.
    G [n, c kc], q and the regulariser's H [c, kc, kc] stay saved for the backward."""

    @staticmethod
    def forward(ctx, emb, centres, labels, loss, n_classes, a, b, gamma, tau, path):
        emb, centres = _prep(emb), _prep(centres)
        n, e = emb.shape
        c = int(n_classes)
        _proxy_width(loss, "centres", centres, e)
        if c < 1 or centres.shape[0] % c:
            raise _lib.EmbnetError(f"{loss}: {centres.shape[0]} centres are not a whole number per class of n_classes={n_classes}")
        kc = centres.shape[0] // c
        labels = _proxy_labels_and_path(loss, labels, n, path)
        kind = MPROXY_KINDS[loss]
        lib = _lib.lib()
        g, q = _new((n, c * kc), emb), _new((c * kc,), emb)
        # H exists where the library launches the regulariser: it decides on tau as the float it receives
        h = _new((c, kc, kc), emb) if kind == 1 and kc > 1 and ctypes.c_float(tau).value > 0 else None
        counts, mean, reg = _new((3,), emb, torch.int32), _new((), emb), _new((), emb)
        ws = _ticket_workspace(_MPROXY_WS, (emb.device.index, stream()), (n, c, kc, e), lib.embnet_multi_proxy_loss_workspace_bytes,
                               torch.float64, emb.device)
        check(lib.embnet_multi_proxy_loss_fwd(ptr(emb), ptr(centres), ptr(labels), n, c, kc, e, kind, f32(a), f32(b), f32(gamma),
                                              f32(tau), PROXY_PATHS[path], ptr(g), ptr(q), ptr(h), ptr(counts), ptr(mean), ptr(reg),
                                              ptr(ws), ws.numel() * 8, stream()))
        ctx.shape, ctx.ws, ctx.has_h = (n, c, kc, e), ws, h is not None
        ctx.save_for_backward(*((emb, centres, g, q) + ((h,) if h is not None else ())))
        ctx.mark_non_differentiable(counts, g, reg)
        ctx.set_materialize_grads(False)
        return mean, counts, reg, g

    @staticmethod
    def backward(ctx, dmean, *_):
        if dmean is None:
            return (None,) * 10
        emb, centres, g, q = ctx.saved_tensors[:4]
        h = ctx.saved_tensors[4] if ctx.has_h else None
        n, c, kc, e = ctx.shape
        demb, dcentres = torch.empty_like(emb), torch.empty_like(centres)
        check(_lib.lib().embnet_multi_proxy_loss_bwd(ptr(emb), ptr(centres), n, c, kc, e, ptr(g), ptr(q), ptr(h), ptr(_prep(dmean)),
                                                     ptr(demb), ptr(dcentres), ptr(ctx.ws), ctx.ws.numel() * 8, stream()))
        return (demb, dcentres) + (None,) * 8


def soft_triple_loss(emb, centres, labels, n_classes, scale=20.0, margin=0.01, gamma=0.1, tau=0.2, path="auto", return_weights=False):
    """SoftTriple (Qian et al., ICCV 2019) of embeddings [N,E] against learnable centres [C*kc,E] (class-major: kc consecutive rows
    per class), labels int32 [N] as in proxy_anchor_loss.  S'_ic = sum_j softmax_j(S_icj / gamma) S_icj pools a class's kc
    similarities, t_ic = scale (S'_ic - margin [c = y_i]), loss = mean over the labelled samples of lse_c t_ic - t_iy, plus the
    centre regulariser reg = tau / (C kc (kc - 1)) sum_c sum_{s<t} sqrt(2 + 1e-5 - 2 cos(w_cs, w_ct)) (include/embnet.h has the
    rounding and the stable forms).  -> (loss [autograd w.r.t. emb and centres], counts int32 [3] = labelled samples, violating
    samples (another class pools at least as similar as the own), 0, reg) on the device, no host synchronisation; return_weights
    adds G [N, C*kc] = dloss/dS.  path: 'auto', 'small' or 'matrix'."""
    out = _MultiProxyLoss.apply(emb, centres, labels, "soft_triple_loss", n_classes, float(scale), float(margin), float(gamma),
                                float(tau), path)
    return out if return_weights else out[:3]


def arcface_loss(emb, centres, labels, n_classes, scale=64.0, margin=0.5, path="auto", return_weights=False):
    """Sub-centre ArcFace (Deng et al., CVPR 2019 / ECCV 2020) of embeddings [N,E] against learnable centres [C*kc,E] (class-major),
    labels int32 [N] as in proxy_anchor_loss; kc = 1 is ArcFace, margin = 0 NormSoftmax.  S'_ic = max_j S_icj,
    t_ic = scale cos(acos(S'_ic) + margin [c = y_i]) with the usual guard below cos(pi - margin), loss = mean over the labelled
    samples of lse_c t_ic - t_iy (include/embnet.h has the rounding and the stable forms).  -> (loss [autograd w.r.t. emb and centres],
    counts int32 [3] = labelled samples, violating samples, samples on the guard's branch) on the device, no host synchronisation;
    return_weights adds G [N, C*kc] = dloss/dS.  path: 'auto', 'small' or 'matrix'."""
    out = _MultiProxyLoss.apply(emb, centres, labels, "arcface_loss", n_classes, float(scale), float(margin), 1.0, 0.0, path)
    return (out[0], out[1], out[3]) if return_weights else out[:2]


# The training modes of train_step.ProxyTrainer:  mode: (function, the loss_params it takes)
PROXY_LOSS_MODES = {
    "proxy_anchor": (proxy_anchor_loss, ("alpha", "delta")),
    "proxy_softmax": (proxy_softmax_loss, ("scale", "margin")),
}
# ... and its modes on several centres per class, in a table of their own: the function takes the number of classes behind the
# labels, `centers` is no argument of it but must be the head's centers_per_class, and the violating samples are counts[1]
MULTI_PROXY_LOSS_MODES = {
    "soft_triple": (soft_triple_loss, ("scale", "margin", "gamma", "tau", "centers")),
    "arcface": (arcface_loss, ("scale", "margin", "centers")),
}


# --------------------------------------------------------------------------- cross-batch memory (csrc/xbm.hip)
XBM_KINDS = {"xbm_contrastive_loss": 1, "xbm_multi_similarity_loss": 2}      # EMBNET_XBM_CONTRASTIVE, EMBNET_XBM_MULTI_SIMILARITY
_XBM_WS = {}


def xbm_enqueue(emb, labels, memory):
    """The rows of emb [N,E] (detached) and their int32 labels [N] into the ring of `memory` (an xbm.CrossBatchMemory, or anything
    with feats [M,E], labels [M], cursor [1], slots and a 16-byte zeroed `ticket`): row i goes to slot (cursor + i) mod M and the
    cursor advances by N, all on the device (embnet_xbm_enqueue: one launch, the cursor read by the kernel, so a captured graph
    replays on the ring's current state).  -> slots int32 [N] (memory.slots[:N]), no host synchronisation."""
    emb = _prep(emb.detach())
    n, e = emb.shape
    m = memory.feats.shape[0]
    if memory.feats.shape[1] != e:
        raise _lib.EmbnetError(f"xbm_enqueue: embeddings of width {e} do not match a memory of width {memory.feats.shape[1]}")
    if n > memory.slots.shape[0]:
        raise _lib.EmbnetError(f"xbm_enqueue: a batch of {n} rows does not fit a memory of {m} slots")
    labels = _int32_labels("xbm_enqueue", "labels", labels, n)
    slots = memory.slots[:n]
    check(_lib.lib().embnet_xbm_enqueue(ptr(emb), ptr(labels), n, e, ptr(memory.feats), ptr(memory.labels), m, ptr(memory.cursor),
                                        ptr(slots), ptr(memory.ticket), stream()))
    return slots


class _XbmLoss(torch.autograd.Function):
    """embnet_xbm_loss_fwd (Circle loss: embnet_xbm_circle_loss_fwd) / _bwd (include/embnet.h): S + sweep forward, one or two backward
    launches.  G [n,m] and the bank stay saved for the backward; the bank is a constant."""

    @staticmethod
    def forward(ctx, emb, labels, mem, mem_labels, self_slots, loss, scalars):
        emb, mem = _prep(emb), _prep(mem.detach())
        n, e = emb.shape
        if mem.dim() != 2 or mem.shape[1] != e:
            raise _lib.EmbnetError(f"{loss}: a memory {tuple(mem.shape)} does not match embeddings of width {e}")
        m = mem.shape[0]
        labels = _int32_labels(loss, "labels", labels, n)
        mem_labels = _int32_labels(loss, "mem_labels", mem_labels, m)
        if self_slots is not None:
            self_slots = _int32_labels(loss, "self_slots", self_slots, n)
        lib = _lib.lib()
        g = _new((n, m), emb)
        counts, mean = _new((4,), emb, torch.int32), _new((), emb)
        ws = _ticket_workspace(_XBM_WS, (emb.device.index, stream()), (n, m, e), lib.embnet_xbm_loss_workspace_bytes, torch.float64,
                               emb.device)
        if loss == "xbm_circle_loss":                       # an entry point of its own: (m, gamma) where the kinds take a, b, c, d
            check(lib.embnet_xbm_circle_loss_fwd(ptr(emb), ptr(labels), ptr(mem), ptr(mem_labels), ptr(self_slots), n, m, e,
                                                 *map(f32, scalars), ptr(g), ptr(counts), ptr(mean), ptr(ws), ws.numel() * 8,
                                                 stream()))
        else:
            a, b, c, d = (tuple(map(f32, scalars)) + (0.0, 0.0, 0.0))[:4]
            check(lib.embnet_xbm_loss_fwd(ptr(emb), ptr(labels), ptr(mem), ptr(mem_labels), ptr(self_slots), n, m, e, XBM_KINDS[loss],
                                          a, b, c, d, ptr(g), ptr(counts), ptr(mean), ptr(ws), ws.numel() * 8, stream()))
        ctx.save_for_backward(mem, g)
        ctx.shape, ctx.ws = (n, m, e), ws                   # the backward's scratch: S is not needed any more
        ctx.mark_non_differentiable(counts, g)
        ctx.set_materialize_grads(False)                    # no zero tensors for the outputs nobody differentiates
        return mean, counts, g

    @staticmethod
    def backward(ctx, dmean, *_):
        if dmean is None:
            return (None,) * 7
        mem, g = ctx.saved_tensors
        n, m, e = ctx.shape
        demb = _new((n, e), g)
        check(_lib.lib().embnet_xbm_loss_bwd(ptr(mem), n, m, e, ptr(g), ptr(_prep(dmean)), ptr(demb), ptr(ctx.ws),
                                             ctx.ws.numel() * 8, stream()))
        return (demb,) + (None,) * 6


def xbm_contrastive_loss(emb, labels, mem, mem_labels, self_slots=None, margin=0.5, return_weights=False):
    """The XBM paper's contrastive loss (Wang et al., CVPR 2020) of embeddings [N,E] with int32 labels [N] against a DETACHED bank
    mem [M,E] with int32 mem_labels [M] (negative: an unlabelled row, an empty slot; they belong to no pair), on S = X mem^T:
    l_i = sum over the same-label slots with 1 - S > 0 of (1 - S) + sum over the other-label slots with S > margin of S, mean over
    all N rows; self_slots int32 [N] names each row's own copy in the bank (what xbm_enqueue returned), which is excluded.
    -> (mean [autograd w.r.t. emb only], counts int32 [4] = kept positives, kept negatives, active anchors, labelled bank slots) on
    the device, no host synchronisation; return_weights adds G [N,M] = dl_i/dS_ij (include/embnet.h)."""
    out = _XbmLoss.apply(emb, labels, mem, mem_labels, self_slots, "xbm_contrastive_loss", (float(margin),))
    return out if return_weights else out[:2]


def xbm_multi_similarity_loss(emb, labels, mem, mem_labels, self_slots=None, alpha=2.0, beta=50.0, base=0.5, epsilon=0.1,
                              return_weights=False):
    """The multi-similarity loss of multi_similarity_loss — its mining rule, rounding forms and stable logarithms — with anchor i's
    positives the same-label slots of a DETACHED bank and its negatives the other-label slots (arguments and results as
    xbm_contrastive_loss; an anchor without a positive or without a negative keeps nothing)."""
    out = _XbmLoss.apply(emb, labels, mem, mem_labels, self_slots, "xbm_multi_similarity_loss",
                         (float(alpha), float(beta), float(base), float(epsilon)))
    return out if return_weights else out[:2]


def xbm_circle_loss(emb, labels, mem, mem_labels, self_slots=None, m=0.4, gamma=80.0, return_weights=False):
    """The Circle loss of circle_loss — its weights, rounding forms and stable logarithms — with anchor i's positives the same-label
    slots of a DETACHED bank and its negatives the other-label slots (arguments and results as xbm_contrastive_loss; an anchor
    without a positive or without a negative has no loss).  counts int32 [4] = positives with alpha+ > 0, negatives with
    alpha- > 0, active anchors (a positive and a negative), labelled bank slots."""
    out = _XbmLoss.apply(emb, labels, mem, mem_labels, self_slots, "xbm_circle_loss", (float(m), float(gamma)))
    return out if return_weights else out[:2]


# The memory losses of train_step.XbmTrainer:  mode: (function, the xbm_params it takes)
XBM_LOSS_MODES = {
    "contrastive": (xbm_contrastive_loss, ("margin",)),
    "multi_similarity": (xbm_multi_similarity_loss, ("alpha", "beta", "base", "epsilon")),
    "circle": (xbm_circle_loss, ("m", "gamma")),
}


# --------------------------------------------------------------------------- contrastive / accuracy
class _Contrastive(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_true, dist):
        y = _prep(y_true).reshape(-1)
        d = _prep(dist).reshape(-1)
        if y.numel() != d.numel():
            raise _lib.EmbnetError("contrastive_loss: y_true and y_pred sizes differ")
        out = _new((), d)
        check(_lib.lib().embnet_contrastive_fwd(ptr(y), ptr(d), d.numel(), ptr(out), stream()))
        ctx.save_for_backward(y, d)
        ctx.shape = dist.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        y, d = ctx.saved_tensors
        dd = torch.empty_like(d)
        check(_lib.lib().embnet_contrastive_bwd(ptr(y), ptr(d), d.numel(), ptr(_prep(dout)), ptr(dd), stream()))
        return None, dd.reshape(ctx.shape)


def contrastive(y_true, dist):
    return _Contrastive.apply(y_true, dist)


def accuracy(y_true, dist):
    y = _prep(y_true.detach()).reshape(-1)
    d = _prep(dist.detach()).reshape(-1)
    out = _new((), d)
    check(_lib.lib().embnet_accuracy(ptr(y), ptr(d), d.numel(), ptr(out), stream()))
    return out


# --------------------------------------------------------------------------- embedding heads
class _L2Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _prep(x)
        n, e = x.shape
        y = torch.empty_like(x)
        rn = _new((n,), x)
        check(_lib.lib().embnet_l2norm_fwd(ptr(x), n, e, ptr(y), ptr(rn), stream()))
        ctx.save_for_backward(y, rn)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, rn = ctx.saved_tensors
        n, e = y.shape
        dx = torch.empty_like(y)
        check(_lib.lib().embnet_l2norm_bwd(ptr(y), ptr(rn), ptr(_prep(dy)), n, e, ptr(dx), stream()))
        return dx


def l2_normalize(x):
    return _L2Normalize.apply(x)


class _PairDistance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e1, e2):
        e1, e2 = _prep(e1), _prep(e2)
        b, e = e1.shape
        d = _new((b, 1), e1)
        check(_lib.lib().embnet_pair_distance_fwd(ptr(e1), ptr(e2), b, e, ptr(d), stream()))
        ctx.save_for_backward(e1, e2, d)
        return d

    @staticmethod
    def backward(ctx, dd):
        e1, e2, d = ctx.saved_tensors
        b, e = e1.shape
        de1, de2 = torch.empty_like(e1), torch.empty_like(e2)
        check(_lib.lib().embnet_pair_distance_bwd(ptr(e1), ptr(e2), ptr(d), ptr(_prep(dd)), b, e,
                                                  ptr(de1), ptr(de2), stream()))
        return de1, de2


def pair_distance(e1, e2):
    """models.py:225: sqrt(max(sum (e1-e2)^2, 1e-7)), keepdims -> [b,1]."""
    return _PairDistance.apply(e1, e2)


# --------------------------------------------------------------------------- evaluation: kNN on embeddings
def cross_distances(q, x, squared=False):
    """[nq,e] x [n,e] -> [nq,n] Euclidean distances (sklearn euclidean_distances(Q, X))."""
    q, x = _prep(q.detach()), _prep(x.detach())
    nq, e = q.shape
    n = x.shape[0]
    if x.shape[1] != e:
        raise _lib.EmbnetError(f"cross_distances: widths differ ({e} vs {x.shape[1]})")
    lib = _lib.lib()
    ws = _new((max(lib.embnet_cross_dist_workspace_bytes(nq, n) // 4, 1),), q)
    d = _new((nq, n), q)
    check(lib.embnet_cross_dist_f32(ptr(q), nq, ptr(x), n, e, ptr(d), int(bool(squared)), ptr(ws), ws.numel() * 4,
                                    stream()))
    return d


def topk_smallest(dist, k):
    """-> (values [rows,k], indices [rows,k] int32), ascending, ties to the smaller column; 0 < k <= min(64, n).
    A NaN entry counts as +inf and is reported as +inf: it follows every finite entry, and every index is in [0, n)."""
    dist = _prep(dist)
    rows, n = dist.shape
    idx = _new((rows, k), dist, torch.int32)
    val = _new((rows, k), dist)
    check(_lib.lib().embnet_topk_smallest(ptr(dist), rows, n, int(k), ptr(idx), ptr(val), stream()))
    return val, idx


def knn_vote(idx, labels):
    """Majority label of each row's neighbours (labels int32 [n]); ties to the smallest label."""
    idx = idx.contiguous()
    labels = labels.to(torch.int32).contiguous()
    pred = _new((idx.shape[0],), idx, torch.int32)
    check(_lib.lib().embnet_knn_vote(ptr(idx), ptr(labels), idx.shape[0], idx.shape[1], ptr(pred), stream()))
    return pred


# --------------------------------------------------------------------------- evaluation: retrieval (Recall@K, MRR)
def _retrieval_blocks(who, q, q_labels, x, x_labels):
    """The shared opening of the two retrieval primitives -> (q, ql, x, xl, self_exclude, nq, n, e): float32 blocks and int32
    labels, contiguous; x None: leave-one-out, the gallery IS the query block.  Errors name the caller `who`."""
    q = _prep(q.detach())
    ql = q_labels.to(torch.int32).contiguous()
    self_exclude = x is None
    if self_exclude:
        if x_labels is not None:
            raise _lib.EmbnetError(f"{who}: gallery labels without a gallery")
        x, xl = q, ql
    else:
        if x_labels is None:
            raise _lib.EmbnetError(f"{who}: a gallery needs its labels")
        x = _prep(x.detach())
        xl = x_labels.to(torch.int32).contiguous()
    if q.dim() != 2 or x.dim() != 2 or q.shape[0] == 0 or x.shape[0] == 0:
        raise _lib.EmbnetError(f"{who}: need non-empty [rows, e] blocks (got {tuple(q.shape)}, {tuple(x.shape)})")
    nq, e = q.shape
    n = x.shape[0]
    if x.shape[1] != e:
        raise _lib.EmbnetError(f"{who}: widths differ ({e} vs {x.shape[1]})")
    if tuple(ql.shape) != (nq,) or tuple(xl.shape) != (n,):
        raise _lib.EmbnetError(f"{who}: one label per row is needed")
    return q, ql, x, xl, self_exclude, nq, n, e


def retrieval_first_positive(q, q_labels, x=None, x_labels=None):
    """Rank of each query's nearest same-class gallery item, without the [nq,n] distance matrix (include/embnet.h).

    q [nq,e], q_labels [nq] (integers); x [n,e], x_labels [n] the gallery.  x is None: leave-one-out on q (column i is skipped
    for query i).  -> (rank int32 [nq]: 1 + negatives in front of the first positive in (d2, index) order, 0 without a positive;
    pos_index int32 [nq]: its gallery index or -1; pos_d2 float32 [nq]: its squared distance or +inf), on the device."""
    q, ql, x, xl, self_exclude, nq, n, e = _retrieval_blocks("retrieval_first_positive", q, q_labels, x, x_labels)
    lib = _lib.lib()
    ws = _new((max(lib.embnet_retrieval_workspace_bytes(nq, n) // 8, 1),), q, torch.float64)
    rank, pos = _new((nq,), q, torch.int32), _new((nq,), q, torch.int32)
    d2 = _new((nq,), q)
    check(lib.embnet_retrieval_first_positive(ptr(q), ptr(ql), nq, ptr(x), ptr(xl), n, e, int(self_exclude), ptr(rank), ptr(pos),
                                              ptr(d2), ptr(ws), ws.numel() * 8, stream()))
    return rank, pos, d2


def retrieval_reduce(rank, ks):
    """rank int32 [nq] (0 = no positive) and cut-offs ks -> (hits int32 [nk] = #{0 < rank <= K}, n_valid int32 [] = #{rank > 0},
    sum_inv_rank float64 [] = sum 1 / rank over rank > 0), on the device; fixed summation order.  ks: a sequence of integers >= 1
    (checked here), or an int32 device tensor whose entries the caller has checked."""
    rank = rank.to(torch.int32).contiguous()
    if torch.is_tensor(ks):
        kt = ks.to(device=rank.device, dtype=torch.int32).contiguous()
    else:
        ks = [int(k) for k in ks]
        if any(k < 1 for k in ks):
            raise _lib.EmbnetError(f"retrieval_reduce: every K must be >= 1 (got {ks})")
        kt = torch.tensor(ks, dtype=torch.int32, device=rank.device)
    if kt.numel() == 0 or rank.numel() == 0:
        raise _lib.EmbnetError("retrieval_reduce: empty ranks or empty ks")
    hits = _new((kt.numel(),), rank, torch.int32)
    n_valid = _new((), rank, torch.int32)
    s = _new((), rank, torch.float64)
    check(_lib.lib().embnet_retrieval_reduce(ptr(rank), rank.numel(), ptr(kt), kt.numel(), ptr(hits), ptr(n_valid), ptr(s),
                                             stream()))
    return hits, n_valid, s


# --------------------------------------------------------------------------- evaluation: k-nearest-neighbour search
KNN_K_MAX = 128                                            # EMBNET_KNN_K_MAX (include/embnet.h)
KNN_SELECT = {"all": 0, "same": 1, "other": 2}


def knn_search(q, x=None, k=1, q_labels=None, x_labels=None, select="all", squared=True):
    """The k nearest gallery items of every query, without the [nq,n] distance matrix (include/embnet.h, "k-nearest-neighbour
    search").

    q [nq,e]; x [n,e] the gallery, None: leave-one-out on q (column i is skipped for query i).  select: 'all' — every gallery
    item (labels may be omitted); 'same' / 'other' — only items with the query's label / with another label (q_labels, and
    x_labels with a gallery, are needed).  1 <= k <= KNN_K_MAX; k may exceed n.
    -> (dist float32 [nq,k], idx int32 [nq,k], found int32 [nq]), on the device: ascending in (d2, index); found = min(k, eligible
    items); entries from found on are idx = -1, dist = +inf.  squared=False: dist is the square root of the kernel's d2 (one
    elementwise pass on the way out)."""
    if select not in KNN_SELECT:
        raise _lib.EmbnetError(f"knn_search: select must be one of {sorted(KNN_SELECT)} (got {select!r})")
    k = int(k)
    if not 1 <= k <= KNN_K_MAX:
        raise _lib.EmbnetError(f"knn_search: k = {k} must be in [1, {KNN_K_MAX}]")
    if q_labels is None:
        if select != "all":
            raise _lib.EmbnetError(f"knn_search: select={select!r} needs labels")
        if x_labels is not None:
            raise _lib.EmbnetError("knn_search: gallery labels without query labels")
        q = _prep(q.detach())
        self_exclude = x is None
        x = q if self_exclude else _prep(x.detach())
        if q.dim() != 2 or x.dim() != 2 or q.shape[0] == 0 or x.shape[0] == 0:
            raise _lib.EmbnetError(f"knn_search: need non-empty [rows, e] blocks (got {tuple(q.shape)}, {tuple(x.shape)})")
        if x.shape[1] != q.shape[1]:
            raise _lib.EmbnetError(f"knn_search: widths differ ({q.shape[1]} vs {x.shape[1]})")
        ql = xl = None
        (nq, e), n = q.shape, x.shape[0]
    else:
        q, ql, x, xl, self_exclude, nq, n, e = _retrieval_blocks("knn_search", q, q_labels, x, x_labels)
    lib = _lib.lib()
    ws = _new((max(lib.embnet_knn_search_workspace_bytes(nq, n, k) // 8, 2),), q, torch.float64)
    idx, found = _new((nq, k), q, torch.int32), _new((nq,), q, torch.int32)
    d2 = _new((nq, k), q)
    check(lib.embnet_knn_search(ptr(q), ptr(ql), nq, ptr(x), ptr(xl), n, e, int(self_exclude), KNN_SELECT[select], k, ptr(idx),
                                ptr(d2), ptr(found), ptr(ws), ws.numel() * 8, stream()))
    return (d2 if squared else d2.sqrt_()), idx, found


# --------------------------------------------------------------------------- softmax pre-training head
class _SoftmaxXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        z, t = _prep(logits), _prep(targets)
        b, c = z.shape
        if t.shape != z.shape:
            raise _lib.EmbnetError(f"categorical_crossentropy: targets {tuple(t.shape)} vs logits {tuple(z.shape)}")
        prob, rows, corr = torch.empty_like(z), _new((b,), z), _new((b,), z)
        mean, acc = _new((), z), _new((), z)
        check(_lib.lib().embnet_softmax_xent_fwd(ptr(z), ptr(t), b, c, ptr(prob), ptr(rows), ptr(corr), ptr(mean),
                                                 ptr(acc), stream()))
        ctx.save_for_backward(prob, t)
        ctx.mark_non_differentiable(acc, prob)
        return mean, acc, prob

    @staticmethod
    def backward(ctx, dmean, _dacc, _dprob):
        prob, t = ctx.saved_tensors
        b, c = prob.shape
        dz = torch.empty_like(prob)
        check(_lib.lib().embnet_softmax_xent_bwd(ptr(prob), ptr(t), b, c, ptr(_prep(dmean)), ptr(dz), stream()))
        return dz, None


def softmax_cross_entropy(logits, targets):
    """Keras Dense(softmax) + 'categorical_crossentropy' + 'accuracy' from the logits:
    -> (mean loss [autograd], accuracy, probabilities)."""
    return _SoftmaxXent.apply(logits, targets)


# --------------------------------------------------------------------------- exact t-SNE (embeddingnet_amd/tsne.py drives these)
def tsne_workspace(n, like):
    """The [bytes/8] float64 workspace the three t-SNE entry points share for n points."""
    return _new((max(_lib.lib().embnet_tsne_workspace_bytes(int(n)) // 8, 1),), like, torch.float64)


def tsne_affinities(d2, perplexity, inplace=False, ws=None):
    """Squared distances [n,n] -> (P [n,n] joint probabilities, beta [n] precisions; sigma = sqrt(1 / (2 beta))): scikit-learn's
    _joint_probabilities.  inplace writes P over d2 (a float32 contiguous tensor)."""
    d2 = _prep(d2)
    n = d2.shape[0]
    if d2.shape != (n, n):
        raise _lib.EmbnetError(f"tsne_affinities: distance matrix {tuple(d2.shape)} is not square")
    ws = tsne_workspace(n, d2) if ws is None else ws
    p = d2 if inplace else torch.empty_like(d2)
    beta = _new((n,), d2)
    check(_lib.lib().embnet_tsne_affinities(ptr(d2), n, f32(perplexity), ptr(p), ptr(beta), ptr(ws), ws.numel() * 8, stream()))
    return p, beta


def tsne_iterate(p, y, update, gains, exaggeration, momentum, learning_rate, n_iter, ws=None):
    """n_iter gradient-descent iterations of exact t-SNE, in place on y, update, gains (float32 contiguous [n,2])."""
    n = p.shape[0]
    for t in (y, update, gains):
        if t.dtype != torch.float32 or tuple(t.shape) != (n, 2):
            raise _lib.EmbnetError(f"tsne_iterate: y, update and gains must be float32 [{n},2]")
    ws = tsne_workspace(n, p) if ws is None else ws
    check(_lib.lib().embnet_tsne_iterate(ptr(p), n, ptr(y), ptr(update), ptr(gains), f32(exaggeration), f32(momentum),
                                         f32(learning_rate), int(n_iter), ptr(ws), ws.numel() * 8, stream()))
    return y


def tsne_kl(p, y, return_grad=False, ws=None):
    """-> out [2] = (KL divergence, 2-norm of the gradient) at y, on the device[, gradient [n,2]]: scikit-learn's _kl_divergence."""
    n = p.shape[0]
    y = _prep(y)
    ws = tsne_workspace(n, p) if ws is None else ws
    out = _new((2,), p)
    grad = _new((n, 2), p) if return_grad else None
    check(_lib.lib().embnet_tsne_kl(ptr(p), n, ptr(y), out.data_ptr(), out.data_ptr() + 4, ptr(grad), ptr(ws), ws.numel() * 8,
                                    stream()))
    return (out, grad) if return_grad else out


# --------------------------------------------------------------------------- evaluation: retrieval (MAP@R, R-precision)
R_MAX = 4096                                                # EMBNET_RETRIEVAL_R_MAX (include/embnet.h)
_POSITIVE_RANKS_STATUS = {1: "the positives of all queries exceed `capacity`",
                          2: f"a query has more than R_MAX = {R_MAX} positives (a class that large is refused)",
                          3: "a label outside [0, num_classes)"}


def retrieval_positive_ranks(q, q_labels, x=None, x_labels=None, num_classes=None, capacity=None):
    """Position of EVERY same-class gallery item of each query, without the [nq,n] distance matrix (include/embnet.h).

    q [nq,e], q_labels [nq]: dense class ids in [0, num_classes); x [n,e], x_labels [n] the gallery, or x None: leave-one-out
    on q.  num_classes None: 1 + the largest label; capacity None: the number of positives of all queries — both then cost one
    host read of the labels.  -> (offset int64 [nq+1], pos_index int32 [total], pos_rank int32 [total]) with total = offset[-1]
    (with `capacity` given the two arrays keep that length): query r's positives are offset[r]:offset[r+1], in the order
    (d2, gallery index); pos_rank = 1-based position among all non-excluded gallery items, so pos_rank[offset[r]] is
    retrieval_first_positive's rank.  A condition the device finds in the labels raises EmbnetError naming it."""
    q, ql, x, xl, self_exclude, nq, n, e = _retrieval_blocks("retrieval_positive_ranks", q, q_labels, x, x_labels)
    if num_classes is None:
        num_classes = int(torch.maximum(ql.max(), xl.max()).item()) + 1
    num_classes = int(num_classes)
    if num_classes < 1:
        raise _lib.EmbnetError(f"retrieval_positive_ranks: num_classes = {num_classes} (labels are dense ids >= 0)")
    trim = capacity is None
    if trim:      # labels out of range are clamped here and reported by the device below
        sizes = torch.bincount(xl.long().clamp(0, num_classes - 1), minlength=num_classes)
        capacity = int((sizes[ql.long().clamp(0, num_classes - 1)] - int(self_exclude)).clamp(min=0).sum().item())
    capacity = max(int(capacity), 1)
    lib = _lib.lib()
    ws = _new((max(lib.embnet_retrieval_positive_ranks_workspace_bytes(nq, n, num_classes, capacity) // 8, 1),), q, torch.float64)
    offset = _new((nq + 1,), q, torch.int64)
    pos_index, pos_rank = _new((capacity,), q, torch.int32), _new((capacity,), q, torch.int32)
    status = _new((1,), q, torch.int32)
    check(lib.embnet_retrieval_positive_ranks(ptr(q), ptr(ql), nq, ptr(x), ptr(xl), n, e, int(self_exclude), num_classes, capacity,
                                              ptr(offset), ptr(pos_index), ptr(pos_rank), ptr(status), ptr(ws), ws.numel() * 8,
                                              stream()))
    st = int(status.item())
    if st != 0:
        raise _lib.EmbnetError(f"retrieval_positive_ranks: status {st}: {_POSITIVE_RANKS_STATUS.get(st, 'unknown')}")
    if trim:
        total = int(offset[-1].item())
        pos_index, pos_rank = pos_index[:total], pos_rank[:total]
    return offset, pos_index, pos_rank


def retrieval_map_reduce(offset, pos_rank):
    """CSR (offset int64 [nq+1], pos_rank int32) of retrieval_positive_ranks -> (ap_at_r, r_precision, ap: float64 [nq], NaN for a
    query without a positive; sums float64 [3] of the three over the valid queries; n_valid int32 []), on the device, fixed
    summation order.  map@r = sums[0] / n_valid, r_precision = sums[1] / n_valid, map = sums[2] / n_valid."""
    offset = offset.contiguous()
    pos_rank = pos_rank.contiguous()
    if offset.dtype != torch.int64 or pos_rank.dtype != torch.int32 or offset.dim() != 1 or offset.numel() < 2:
        raise _lib.EmbnetError("retrieval_map_reduce: offset int64 [nq+1] and pos_rank int32 are needed")
    nq = offset.numel() - 1
    if pos_rank.numel() == 0:                               # no positive anywhere: nothing is read through this pointer
        pos_rank = _new((1,), offset, torch.int32)
    per = [_new((nq,), offset, torch.float64) for _ in range(3)]
    sums = _new((3,), offset, torch.float64)
    n_valid = _new((), offset, torch.int32)
    check(_lib.lib().embnet_retrieval_map_reduce(ptr(offset), ptr(pos_rank), nq, ptr(per[0]), ptr(per[1]), ptr(per[2]), ptr(sums),
                                                 ptr(n_valid), stream()))
    return per[0], per[1], per[2], sums, n_valid


# --------------------------------------------------------------------------- k-means on encodings (csrc/kmeans.hip)
def _kmeans_block(who, t, name):
    """A block is taken as it is or refused: float32, contiguous, [rows, e] on the device.  (A silent copy would hide a cast
    of a whole encodings block per Lloyd pass.)"""
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise _lib.EmbnetError(f"{who}: {name} must be a float32 tensor (got {getattr(t, 'dtype', type(t))})")
    if t.dim() != 2:
        raise _lib.EmbnetError(f"{who}: {name} must be [rows, e] (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise _lib.EmbnetError(f"{who}: {name} must be contiguous")
    return t.detach()


def _kmeans_labels(who, labels, n):
    if not torch.is_tensor(labels) or labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or not labels.is_contiguous():
        raise _lib.EmbnetError(f"{who}: labels must be a contiguous int32 tensor of {n} entries")
    return labels


def _kmeans_shapes(who, x, centres):
    x, centres = _kmeans_block(who, x, "points"), _kmeans_block(who, centres, "centres")
    if x.shape[1] != centres.shape[1]:
        raise _lib.EmbnetError(f"{who}: widths differ (points e = {x.shape[1]}, centres e = {centres.shape[1]})")
    return x, centres, x.shape[0], centres.shape[0], x.shape[1]


def kmeans_workspace(n, k, e, like):
    """The workspace every k-means call of one (n, k, e) problem shares; it also carries the point norms from the first assign
    pass of a fit to the later ones.  A refused shape (k > n, a size <= 0) gets a token workspace: the call itself reports it."""
    nbytes = _lib.lib().embnet_kmeans_workspace_bytes(int(n), int(k), int(e))
    return _new((max(nbytes // 8, 2),), like, torch.float64)


def kmeans_assign(x, centres, prev_labels=None, ws=None, reuse_point_norms=False):
    """Nearest centre of every point, without the [n,k] distance matrix (include/embnet.h).

    x [n,e], centres [k,e] float32.  -> (labels int32 [n]: ties to the smaller centre index; d2 float32 [n]: the squared distance
    to that centre; changed int32 []: the labels that differ from prev_labels (n without them); inertia float64 []: sum d2),
    on the device.  ws: kmeans_workspace(n, k, e, x); reuse_point_norms: ws already went through an assign call on this x."""
    x, centres, n, k, e = _kmeans_shapes("kmeans_assign", x, centres)
    if prev_labels is not None:
        prev_labels = _kmeans_labels("kmeans_assign", prev_labels, n)
    if ws is None:
        ws, reuse_point_norms = kmeans_workspace(n, k, e, x), False
    labels, d2 = _new((n,), x, torch.int32), _new((n,), x)
    changed, inertia = _new((), x, torch.int32), _new((), x, torch.float64)
    check(_lib.lib().embnet_kmeans_assign(ptr(x), n, ptr(centres), k, e, int(bool(reuse_point_norms)), ptr(prev_labels), ptr(labels),
                                          ptr(d2), ptr(changed), ptr(inertia), ptr(ws), ws.numel() * 8, stream()))
    return labels, d2, changed, inertia


def kmeans_update(x, labels, centres, ws=None):
    """The mean of every cluster's points (include/embnet.h).  x [n,e], labels int32 [n], centres [k,e] the previous centres.
    -> (centres float32 [k,e]: an empty cluster keeps its previous centre; counts int32 [k]; shift float64 []: the sum of
    |new - old|^2; n_empty int32 []), on the device; the same bits for the same labels."""
    x, centres, n, k, e = _kmeans_shapes("kmeans_update", x, centres)
    labels = _kmeans_labels("kmeans_update", labels, n)
    if ws is None:
        ws = kmeans_workspace(n, k, e, x)
    out, counts = _new((k, e), x), _new((k,), x, torch.int32)
    shift, n_empty = _new((), x, torch.float64), _new((), x, torch.int32)
    check(_lib.lib().embnet_kmeans_update(ptr(x), ptr(labels), n, ptr(centres), k, e, ptr(out), ptr(counts), ptr(shift),
                                          ptr(n_empty), ptr(ws), ws.numel() * 8, stream()))
    return out, counts, shift, n_empty


def kmeans_pp_update(x, index, mind2=None):
    """k-means++ weights: mind2[i] = min(mind2[i], |x_i - x_c|^2) for the row c = index (int32 device tensor of one entry);
    mind2 None: the first call, which creates it.  -> mind2 float32 [n] (updated in place when given)."""
    x = _kmeans_block("kmeans_pp_update", x, "points")
    n, e = x.shape
    if not torch.is_tensor(index) or index.dtype != torch.int32 or index.numel() != 1:
        raise _lib.EmbnetError("kmeans_pp_update: index must be an int32 tensor of one entry")
    first = mind2 is None
    if first:
        mind2 = _new((n,), x)
    elif mind2.dtype != torch.float32 or tuple(mind2.shape) != (n,):
        raise _lib.EmbnetError(f"kmeans_pp_update: mind2 must be float32 [{n}]")
    check(_lib.lib().embnet_kmeans_pp_update(ptr(x), n, e, ptr(index), int(first), ptr(mind2), stream()))
    return mind2


def kmeans_pp_pick(mind2, seed, draw):
    """Draw `draw` of a k-means++ seeding keyed by `seed`: draw 0 is uniform over the n rows (only mind2's length and device are
    used); draw j >= 1 samples a row with probability mind2 / sum(mind2), never one of weight 0 while the sum is positive.
    -> (index int32 [1], u float64 []: the draw's uniform number, 0 for draw 0) on the device."""
    like = mind2
    if not torch.is_tensor(mind2) or mind2.dtype != torch.float32 or mind2.dim() != 1 or mind2.numel() == 0:
        raise _lib.EmbnetError("kmeans_pp_pick: mind2 must be a non-empty float32 [n] tensor")
    index, u = _new((1,), like, torch.int32), _new((), like, torch.float64)
    check(_lib.lib().embnet_kmeans_pp_pick(ptr(mind2), mind2.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw), ptr(index), ptr(u),
                                           stream()))
    return index, u


# --------------------------------------------------------------------------- verification histograms (csrc/verification.hip)
VERIFICATION_MAX_BINS = 4096


def verification_all_pairs(q, q_labels, x=None, x_labels=None, bins=4096, d2_max=4.0, flush_tiles=0):
    """Every (query, gallery) pair counted by its squared distance, without the [nq,n] matrix (include/embnet.h, "verification").

    q [nq,e], q_labels [nq]; x [n,e], x_labels [n] the gallery, or None: leave-one-out on q — pair (i, i) is skipped and every
    unordered pair is counted twice.  bins: a power of two in [2, 4096] over [0, d2_max), d2_max a power of two; a pair beyond
    the range (or with a NaN distance) sits in the last bin.  -> (hist_same, hist_other) int64 [bins] on the device, exact.
    flush_tiles: how often a workgroup empties its LDS counters (0: as rarely as is safe); the result does not depend on it."""
    q, ql, x, xl, self_exclude, nq, n, e = _retrieval_blocks("verification_all_pairs", q, q_labels, x, x_labels)
    lib = _lib.lib()
    ws = _new((max(lib.embnet_verification_all_pairs_workspace_bytes(nq, n) // 8, 2),), q, torch.float64)
    hist = _new((2, int(bins)) if int(bins) > 0 else (2, 1), q, torch.int64)
    check(lib.embnet_verification_all_pairs(ptr(q), ptr(ql), nq, None if self_exclude else ptr(x), None if self_exclude else ptr(xl),
                                            n, e, int(bins), f32(d2_max), int(flush_tiles), ptr(hist[0]), ptr(hist[1]),
                                            ptr(ws), ws.numel() * 8, stream()))
    return hist[0], hist[1]


def verification_values(values, same, lo=0.0, w=1.0, bins=4096):
    """Per-pair values (distances or scores) counted into a same-pair and an other-pair histogram of `bins` bins of width w (a
    power of two) from lo: bin = clamp(floor((v - lo) / w), 0, bins - 1), NaN to the last bin.  values [m] float32, same [m]
    (non-zero: a same-class pair); m = 0 yields zeros.  -> (hist_same, hist_other) int64 [bins] on the device, exact."""
    values = _prep(values.detach()).reshape(-1)
    same = same.to(device=values.device, dtype=torch.int32).contiguous().reshape(-1)
    if same.numel() != values.numel():
        raise _lib.EmbnetError(f"verification_values: {values.numel()} values but {same.numel()} flags")
    m = values.numel()
    hist = _new((2, int(bins)) if int(bins) > 0 else (2, 1), values, torch.int64)
    check(_lib.lib().embnet_verification_values(ptr(values) if m else None, ptr(same) if m else None, m, f32(lo), f32(w), int(bins),
                                                ptr(hist[0]), ptr(hist[1]), stream()))
    return hist[0], hist[1]
