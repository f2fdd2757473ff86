"""Drop-in for embedding_net/losses_and_accuracies.py (same names, arguments and
meaning), computing on the GPU through libembnet_hip.so.

  contrastive_loss(y_true, y_pred)          reference :4-11
  triplet_loss(margin)(y_true, y_pred)      reference :14-44  -> per-row [T] (caller means)
  accuracy(y_true, y_pred)                  reference :47-50
  batch_all_triplet_loss(P, K, margin)(y_true, y_pred)   build-defined (batch-all over a [P*K, E] block) -> scalar
  multi_similarity_loss(P, K, alpha, beta, base, epsilon)(y_true, y_pred)   build-defined (MS loss over a [P*K, E] block) -> scalar
  supcon_loss(P, K, temperature, denominator)(y_true, y_pred)   build-defined (SupCon / NT-Xent over a [P*K, E] block) -> scalar
  circle_loss(P, K, m, gamma)(y_true, y_pred)               build-defined (Circle loss over a [P*K, E] block) -> scalar
  margin_loss(P, K, beta, alpha, cutoff, nonzero_loss_cutoff, seed)(y_true, y_pred)   build-defined (distance-weighted sampling + margin loss) -> scalar
  fast_ap_loss(P, K, bins)(y_true, y_pred)                  build-defined (FastAP over a [P*K, E] block) -> scalar
  smooth_ap_loss(P, K, temperature)(y_true, y_pred)         build-defined (Smooth-AP over a [P*K, E] block) -> scalar
  proxy_anchor_loss(head, alpha, delta)(y_true, y_pred)     build-defined (Proxy-Anchor against a ProxyHead's proxies) -> scalar
  proxy_softmax_loss(head, scale, margin)(y_true, y_pred)   build-defined (CosFace / NormSoftmax against a ProxyHead's proxies) -> scalar
  soft_triple_loss(head, scale, margin, gamma, tau)(y_true, y_pred)   build-defined (SoftTriple against a ProxyHead's centres) -> scalar
  arcface_loss(head, scale, margin)(y_true, y_pred)         build-defined (sub-centre ArcFace against a ProxyHead's centres) -> scalar
  xbm_loss(memory, loss, **params)(y_true, y_pred)          build-defined (a batch against a cross-batch memory, xbm.py) -> scalar
Inputs are torch CUDA tensors; outputs carry autograd.
"""
from . import ops


def contrastive_loss(y_true, y_pred):
    '''Contrastive loss (Hadsell et al. 2006), margin fixed to 1, y_true 1 = same class.'''
    return ops.contrastive(y_true, y_pred)


def triplet_loss(margin=0.5):
    """Returns loss_function(y_true, y_pred); y_pred is [T, 3E] = concat(anchor,
    positive, negative) on the last axis, y_true is ignored (Keras signature)."""

    def loss_function(y_true, y_pred):
        return ops.triplet_hinge(y_pred, margin)

    return loss_function


def batch_all_triplet_loss(k_classes, k_samples, margin=0.5):
    """Returns loss_function(y_true, y_pred) -> scalar; y_pred is the class-contiguous [k_classes*k_samples, E] embedding
    block, y_true is ignored (Keras signature).  Batch-all (build-defined, not in the reference): the mean of
    d(a,p) - d(a,n) + margin over every valid triplet of the block where it is > 0 (d squared L2)."""

    def loss_function(y_true, y_pred):
        return ops.batch_all_triplet_loss(y_pred, k_classes, k_samples, margin)[0]

    return loss_function


def multi_similarity_loss(k_classes, k_samples, alpha=2.0, beta=50.0, base=0.5, epsilon=0.1):
    """Returns loss_function(y_true, y_pred) -> scalar; y_pred is the class-contiguous [k_classes*k_samples, E] embedding
    block, y_true is ignored (Keras signature).  Multi-similarity loss (Wang et al. 2019; build-defined, not in the
    reference): pairs mined with `epsilon` on the dot-product similarities, weighted through two log-sum-exps
    (include/embnet.h, embnet_ms_loss_fwd)."""

    def loss_function(y_true, y_pred):
        return ops.multi_similarity_loss(y_pred, k_classes, k_samples, alpha, beta, base, epsilon)[0]

    return loss_function


def supcon_loss(k_classes, k_samples, temperature=0.1, denominator="all"):
    """Returns loss_function(y_true, y_pred) -> scalar; y_pred is the class-contiguous [k_classes*k_samples, E] embedding
    block, y_true is ignored (Keras signature).  The softmax / InfoNCE family (build-defined, not in the reference):
    denominator 'all' is SupCon (Khosla et al. 2020, L_out), 'negatives' NT-Xent with the pair itself and the anchor's
    negatives in the denominator (include/embnet.h, embnet_supcon_loss_fwd)."""

    def loss_function(y_true, y_pred):
        return ops.supcon_loss(y_pred, k_classes, k_samples, temperature, denominator)[0]

    return loss_function


def circle_loss(k_classes, k_samples, m=0.4, gamma=80.0):
    """Returns loss_function(y_true, y_pred) -> scalar; y_pred is the class-contiguous [k_classes*k_samples, E] embedding
    block, y_true is ignored (Keras signature).  Circle loss (Sun et al. 2020, the pair-wise form; build-defined, not in the
    reference): every pair weighted by its distance from its optimum, relaxation m and scale gamma (include/embnet.h,
    embnet_circle_loss_fwd)."""

    def loss_function(y_true, y_pred):
        return ops.circle_loss(y_pred, k_classes, k_samples, m, gamma)[0]

    return loss_function


def margin_loss(k_classes, k_samples, beta=1.2, alpha=0.2, cutoff=0.5, nonzero_loss_cutoff=1.4, seed=0):
    """Returns loss_function(y_true, y_pred) -> scalar; y_pred is the class-contiguous [k_classes*k_samples, E] block of
    L2-normalised embeddings, y_true is ignored (Keras signature).  Distance-weighted sampling with the margin loss (Wu et al.
    2017; build-defined, not in the reference): one negative per positive drawn with the inverse of the unit sphere's distance
    density, two hinges around the boundary beta; the draws are keyed by `seed` (include/embnet.h, embnet_margin_loss_fwd)."""

    def loss_function(y_true, y_pred):
        return ops.margin_loss(y_pred, k_classes, k_samples, beta, alpha, cutoff, nonzero_loss_cutoff, seed=seed)[0]

    return loss_function


def fast_ap_loss(k_classes, k_samples, bins=10):
    """Returns loss_function(y_true, y_pred) -> scalar; y_pred is the class-contiguous [k_classes*k_samples, E] block of
    L2-normalised embeddings, y_true is ignored (Keras signature).  FastAP (Cakir et al. 2019; build-defined, not in the
    reference): average precision over each anchor's soft-binned distance histograms (include/embnet.h,
    embnet_fast_ap_loss_fwd)."""

    def loss_function(y_true, y_pred):
        return ops.fast_ap_loss(y_pred, k_classes, k_samples, bins)[0]

    return loss_function


def smooth_ap_loss(k_classes, k_samples, temperature=0.01):
    """Returns loss_function(y_true, y_pred) -> scalar; y_pred is the class-contiguous [k_classes*k_samples, E] embedding
    block, y_true is ignored (Keras signature).  Smooth-AP (Brown et al. 2020; build-defined, not in the reference): average
    precision with sigmoid ranks at a temperature (include/embnet.h, embnet_smooth_ap_loss_fwd)."""

    def loss_function(y_true, y_pred):
        return ops.smooth_ap_loss(y_pred, k_classes, k_samples, temperature)[0]

    return loss_function


def proxy_anchor_loss(head, alpha=32.0, delta=0.1):
    """Returns loss_function(y_true, y_pred) -> scalar; y_true is the int32 [N] tensor of global class indices (outside
    [0, C): unlabelled), y_pred the [N, E] embeddings, head a proxies.ProxyHead whose parameter receives a gradient.  Proxy-Anchor
    (Kim et al. 2020; build-defined, not in the reference; include/embnet.h, embnet_proxy_loss_fwd)."""

    def loss_function(y_true, y_pred):
        return ops.proxy_anchor_loss(y_pred, head.proxies, y_true, alpha, delta)[0]

    return loss_function


def proxy_softmax_loss(head, scale=64.0, margin=0.35):
    """Returns loss_function(y_true, y_pred) -> scalar; arguments as proxy_anchor_loss.  CosFace (Wang et al. 2018), with
    margin = 0 NormSoftmax (build-defined, not in the reference; include/embnet.h, embnet_proxy_loss_fwd)."""

    def loss_function(y_true, y_pred):
        return ops.proxy_softmax_loss(y_pred, head.proxies, y_true, scale, margin)[0]

    return loss_function


def soft_triple_loss(head, scale=20.0, margin=0.01, gamma=0.1, tau=0.2):
    """Returns loss_function(y_true, y_pred) -> scalar; arguments as proxy_anchor_loss, head a proxies.ProxyHead with
    centers_per_class centres per class.  SoftTriple (Qian et al. 2019), the centre regulariser included (build-defined, not in
    the reference; include/embnet.h, embnet_multi_proxy_loss_fwd)."""

    def loss_function(y_true, y_pred):
        return ops.soft_triple_loss(y_pred, head.proxies, y_true, head.n_classes, scale, margin, gamma, tau)[0]

    return loss_function


def arcface_loss(head, scale=64.0, margin=0.5):
    """Returns loss_function(y_true, y_pred) -> scalar; arguments as soft_triple_loss.  Sub-centre ArcFace (Deng et al. 2019 / 2020);
    centers_per_class = 1 is ArcFace, margin = 0 NormSoftmax (build-defined, not in the reference; include/embnet.h,
    embnet_multi_proxy_loss_fwd)."""

    def loss_function(y_true, y_pred):
        return ops.arcface_loss(y_pred, head.proxies, y_true, head.n_classes, scale, margin)[0]

    return loss_function


def xbm_loss(memory, loss="contrastive", **params):
    """Returns loss_function(y_true, y_pred) -> scalar; y_true is the int32 [N] tensor of class indices (negative: unlabelled),
    y_pred the [N, E] embeddings, memory an xbm.CrossBatchMemory.  Each call first enqueues the batch (detached) and then scores
    it against the whole memory with the rows' own slots excluded: the cross-batch memory loss of Wang et al. 2020 (build-defined,
    not in the reference; include/embnet.h, embnet_xbm_loss_fwd).  loss: 'contrastive' (params: margin) or 'multi_similarity'
    (alpha, beta, base, epsilon) or 'circle' (m, gamma; embnet_xbm_circle_loss_fwd); other parameters are refused."""
    if loss not in ops.XBM_LOSS_MODES:
        raise KeyError(loss)
    fn, keys = ops.XBM_LOSS_MODES[loss]
    if set(params) - set(keys):
        raise ValueError(f"xbm_loss: unknown parameters {sorted(set(params) - set(keys))} for {loss!r} ({', '.join(keys)})")

    def loss_function(y_true, y_pred):
        slots = memory.enqueue(y_pred, y_true)
        return fn(y_pred, y_true, memory.feats, memory.labels, slots, **params)[0]

    return loss_function


def accuracy(y_true, y_pred):
    '''Classification accuracy with a fixed 0.5 threshold on distances.'''
    return ops.accuracy(y_true, y_pred)
