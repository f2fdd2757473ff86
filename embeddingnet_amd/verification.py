"""Verification metrics on embeddings: ROC AUC, equal error rate, TAR@FAR and the best threshold, for any number of pairs.

Verification asks of two items whether they are the same class: they are accepted as "same" when their distance is below a
threshold.  TAR (true accept rate, TPR) is the share of same-class pairs accepted, FAR (false accept rate, FPR) the share of
other-class pairs accepted.  Every metric here is a function of two histograms of the pair distances, one over the same-class
pairs and one over the other-class pairs, with `bins` bins of width w from lo; the thresholds are the bin edges
t_j = lo + j * w, and a pair is accepted at t_j iff its bin is below j (include/embnet.h, "verification": the bin is an exact
function of the fp32 distance).  ops.verification_all_pairs counts ALL pairs of a set of encodings in one walk of the fp32 MFMA
distance GEMM whose epilogue bins d2 instead of storing it (csrc/verification.hip): no [n, n] matrix, no sort, O(bins) result,
exact integer counts.  ops.verification_values counts an explicit list of per-pair values (distances of a pair list, Siamese
scores).  The reduction from the histograms to the metrics (verification_from_histograms) is host arithmetic on at most 2 x 4096
integers, exact in Python integers up to the final divisions.

Out of scope: a query set that is a strict subset of its gallery (as for retrieval), more than 4096 bins, ROC plots, per-class
breakdowns, score normalisation, open-set identification.
"""
import math
from fractions import Fraction

import numpy as np
import torch

from . import ops
from .retrieval import _blocks, _unpack

DEFAULT_FARS = (1e-1, 1e-2, 1e-3)
NAN = float('nan')


def _counts(h):
    if torch.is_tensor(h):
        h = h.detach().cpu().numpy()
    out = [int(v) for v in np.asarray(h).reshape(-1).tolist()]
    if any(v < 0 for v in out):
        raise ValueError("verification_from_histograms: a negative count")
    return out


def _far_list(fars):
    fars = [f for f in fars]
    for f in fars:
        if isinstance(f, bool) or not isinstance(f, (int, float)) or not 0.0 < float(f) < 1.0:
            raise ValueError(f"verification: every far must lie in (0, 1) (got {f!r})")
    return [float(f) for f in fars]


def _check_bins(bins, who):
    if isinstance(bins, bool) or int(bins) != bins or not 2 <= int(bins) <= ops.VERIFICATION_MAX_BINS or int(bins) & (int(bins) - 1):
        raise ValueError(f"{who}: bins must be a power of two in [2, {ops.VERIFICATION_MAX_BINS}] (got {bins!r})")
    return int(bins)


def _pow2_at_least(v):
    """The smallest power of two >= v (v > 0, finite), as a float."""
    m, ex = math.frexp(v)                                   # v = m * 2**ex, 0.5 <= m < 1
    return math.ldexp(1.0, ex - 1 if m == 0.5 else ex)


def far_count(f, n_other):
    """floor(f * n_other) with f read as the decimal number that repr(f) prints (0.1 is one tenth, not the double below it)."""
    return int(Fraction(repr(float(f))) * n_other // 1)


def verification_from_histograms(hist_same, hist_other, lo, w, fars=DEFAULT_FARS, at=None, accept='below'):
    """P = hist_same, N = hist_other (equal length `bins`, non-negative integers) -> dict of metrics.

    accept='below' (distances): a pair is accepted as same at edge j iff its bin is below j, the edge is t_j = lo + j * w.
    accept='above' (scores, larger means same): both histograms are reversed first, the edge is t_j = lo + (bins - j) * w, and a
    pair is accepted iff its value is at least t_j.  With TP_j, FP_j the accepted same / other pairs at edge j (j = 0 .. bins):
      auc             the probability that a random same pair is in a lower bin than a random other pair, ties inside a bin half
      eer, eer_threshold   where FPR = 1 - TPR, linear between the two edges around the crossing
      tar@far=f, threshold@far=f   TPR and edge at the LARGEST j with FP_j <= floor(f * n_other): no interpolation, the
                      conservative reading (the key carries repr(f))
      best_accuracy, best_threshold   the edge with the most correct decisions (TP_j + n_other - FP_j), ties to the smaller j
      accuracy@T, accuracy_threshold@T   for each T in `at`: at the edge nearest to T, and that edge
      n_same, n_other, tpr, fpr, thresholds (float64 arrays of length bins + 1)
    With n_same == 0 or n_other == 0 every rate is NaN and the counts stand."""
    if accept not in ('below', 'above'):
        raise ValueError(f"verification_from_histograms: accept must be 'below' or 'above' (got {accept!r})")
    P, N = _counts(hist_same), _counts(hist_other)
    bins = len(P)
    if bins < 1 or len(N) != bins:
        raise ValueError(f"verification_from_histograms: two histograms of one length are needed (got {len(P)}, {len(N)})")
    fars = _far_list(fars)
    at = [float(t) for t in (at or ())]
    lo, w = float(lo), float(w)
    if not w > 0.0:
        raise ValueError(f"verification_from_histograms: w must be positive (got {w})")
    below = accept == 'below'
    if not below:
        P, N = P[::-1], N[::-1]
    edge = (lambda j: lo + j * w) if below else (lambda j: lo + (bins - j) * w)
    step = w if below else -w
    SP, SN = sum(P), sum(N)
    TP, FP = [0], [0]
    for b in range(bins):
        TP.append(TP[-1] + P[b])
        FP.append(FP[-1] + N[b])
    out = {'n_same': SP, 'n_other': SN, 'thresholds': np.asarray([edge(j) for j in range(bins + 1)], np.float64)}
    out['tpr'] = np.asarray([t / SP for t in TP], np.float64) if SP else np.full(bins + 1, np.nan)
    out['fpr'] = np.asarray([f / SN for f in FP], np.float64) if SN else np.full(bins + 1, np.nan)
    snap = {}
    for T in at:
        j = min(max(int(math.floor((T - lo) / w + 0.5)), 0), bins)
        snap[T] = j if below else bins - j
    if SP == 0 or SN == 0:
        for name in ('auc', 'eer', 'eer_threshold', 'best_accuracy', 'best_threshold'):
            out[name] = NAN
        for f in fars:
            out[f'tar@far={f!r}'] = out[f'threshold@far={f!r}'] = NAN
        for T in at:
            out[f'accuracy@{T!r}'] = NAN
            out[f'accuracy_threshold@{T!r}'] = edge(snap[T])
        return out

    # auc: twice the numerator in integers, one division
    num2 = 0
    for b in range(bins):
        if P[b]:
            num2 += P[b] * (2 * (SN - FP[b + 1]) + N[b])
    out['auc'] = num2 / (2 * SP * SN)

    # eer: the smallest j with FPR_j >= 1 - TPR_j, that is FP_j * SP >= (SP - TP_j) * SN; false at j = 0, true at j = bins
    j = next(j for j in range(1, bins + 1) if FP[j] * SP >= (SP - TP[j]) * SN)
    s = Fraction((SP - TP[j - 1]) * SN - FP[j - 1] * SP, (FP[j] - FP[j - 1]) * SP + (TP[j] - TP[j - 1]) * SN)
    out['eer'] = float(Fraction(FP[j - 1], SN) + s * Fraction(FP[j] - FP[j - 1], SN))
    out['eer_threshold'] = edge(j - 1) + float(s) * step

    for f in fars:
        allowed = far_count(f, SN)
        j = max(j for j in range(bins + 1) if FP[j] <= allowed)          # FP_0 = 0 always qualifies
        out[f'tar@far={f!r}'] = TP[j] / SP
        out[f'threshold@far={f!r}'] = edge(j)

    correct = [TP[j] + SN - FP[j] for j in range(bins + 1)]
    j = correct.index(max(correct))                         # the first of equal maxima
    out['best_accuracy'] = correct[j] / (SP + SN)
    out['best_threshold'] = edge(j)
    for T in at:
        out[f'accuracy@{T!r}'] = correct[snap[T]] / (SP + SN)
        out[f'accuracy_threshold@{T!r}'] = edge(snap[T])
    return out


def _with_distances(out):
    """Thresholds in d2 -> also as distances: <key>_distance = sqrt(threshold) for every threshold key."""
    for k in [k for k in out if 'threshold' in k and k != 'thresholds']:
        v = out[k]
        out[k + '_distance'] = math.sqrt(v) if v == v and v >= 0.0 else NAN
    return out


def _max_norm(t):
    """The largest finite row norm of a block (float64), 0.0 when there is none."""
    n = torch.linalg.vector_norm(t.double(), dim=1)
    n = n[torch.isfinite(n)]
    return float(n.max().item()) if n.numel() else 0.0


# a row "normalised" in float32 has a norm within a few ulp of 1: the range is chosen for the norms less this slack, so that
# unit rows get d2_max = 4 and not 8.  A pair beyond the range is still counted: the last bin takes it.
_NORM_SLACK = 1.0 - 2.0 ** -16


def _range_for(bound):
    return _pow2_at_least(bound * _NORM_SLACK) if bound > 0.0 and math.isfinite(bound) else 1.0


def verification_metrics(encodings, labels=None, gallery=None, gallery_labels=None, fars=DEFAULT_FARS, bins=4096, d2_max=None,
                         at=None, device=None):
    """ROC AUC, EER, TAR@FAR, best threshold over ALL pairs (query, gallery item): a pair is "same" when the labels agree.

    The inputs are retrieval_metrics': arrays, tensors or the encodings dict; gallery None = all unordered pairs within
    `encodings` (i < j, every pair once).  bins: a power of two in [2, 4096] over [0, d2_max) of the SQUARED distance;
    d2_max None: the smallest power of two >= (max |q| + max |x|)^2 * (1 - 2^-16), 4 for normalised encodings — the slack
    keeps rows whose float32 norm is a few ulp above 1 at 4 and not 8: a bound up to 1.5e-5 (relative) above a power of two
    is rounded DOWN to it, and the few pairs beyond the range are counted in the last bin.  Thresholds are in d2; every
    threshold also comes as a distance under <key>_distance.  at: thresholds in d2 for accuracy@T (the reference's `accuracy`,
    d < 0.5, is at=[0.25]).  -> verification_from_histograms' dict plus 'hist_same', 'hist_other' (int64 arrays), 'd2_max'."""
    encodings, labels, gallery, gallery_labels = _unpack(encodings, labels, gallery, gallery_labels)
    bins = _check_bins(bins, "verification_metrics")
    fars = _far_list(fars)
    q, ql, x, xl, _ = _blocks("verification_metrics", encodings, labels, gallery, gallery_labels, device)
    if d2_max is None:
        nq = _max_norm(q)
        d2_max = _range_for((nq + (nq if x is None else _max_norm(x))) ** 2)
    d2_max = float(d2_max)
    if not (d2_max > 0.0 and math.isfinite(d2_max) and math.frexp(d2_max)[0] == 0.5):
        raise ValueError(f"verification_metrics: d2_max must be a positive power of two (got {d2_max})")
    hs, ho = ops.verification_all_pairs(q, ql, x, xl, bins=bins, d2_max=d2_max)
    hs, ho = hs.cpu().numpy(), ho.cpu().numpy()
    if x is None:                                           # ordered pairs: (i, j) and (j, i) have the same bits of d2
        hs, ho = hs // 2, ho // 2
    out = verification_from_histograms(hs, ho, 0.0, d2_max / bins, fars=fars, at=at)
    out.update(hist_same=hs, hist_other=ho, d2_max=d2_max)
    return _with_distances(out)


def _pair_inputs(who, same, m, dev):
    if torch.is_tensor(same):
        same = same.detach().cpu().numpy()
    same = np.asarray(same).reshape(-1)
    if same.shape[0] != m:
        raise ValueError(f"{who}: {m} pairs but {same.shape[0]} flags")
    return torch.as_tensor((same != 0).astype(np.int32), device=dev)


def _device_of(t, device):
    if device is not None:
        return device
    if torch.is_tensor(t) and t.is_cuda:
        return t.device
    from .backbones import default_device
    return default_device()


def verification_pair_metrics(a, b, same, fars=DEFAULT_FARS, bins=4096, d_max=None, at=None, device=None):
    """The same metrics over an explicit pair list: a, b [m, e], same [m] (non-zero / True: a same-class pair).  The distances
    are ops.pair_distance's (the Siamese head's Euclidean distance); thresholds are in d over [0, d_max), d_max None: the smallest
    power of two >= (max |a| + max |b|) * (1 - 2^-16) (the slack of verification_metrics).  -> verification_from_histograms' dict plus 'hist_same', 'hist_other', 'd_max'."""
    bins = _check_bins(bins, "verification_pair_metrics")
    fars = _far_list(fars)
    dev = _device_of(a, device)
    a = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=dev, dtype=torch.float32).contiguous()
    b = torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b).to(device=dev, dtype=torch.float32).contiguous()
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"verification_pair_metrics: a and b must be [m, e] of one shape (got {tuple(a.shape)}, {tuple(b.shape)})")
    m = a.shape[0]
    flags = _pair_inputs("verification_pair_metrics", same, m, dev)
    if d_max is None:
        d_max = _range_for(_max_norm(a) + _max_norm(b)) if m else 1.0
    d_max = float(d_max)
    if not (d_max > 0.0 and math.isfinite(d_max) and math.frexp(d_max)[0] == 0.5):
        raise ValueError(f"verification_pair_metrics: d_max must be a positive power of two (got {d_max})")
    d = ops.pair_distance(a.detach(), b.detach()).reshape(-1) if m else torch.empty(0, device=dev)
    hs, ho = ops.verification_values(d, flags, lo=0.0, w=d_max / bins, bins=bins)
    hs, ho = hs.cpu().numpy(), ho.cpu().numpy()
    out = verification_from_histograms(hs, ho, 0.0, d_max / bins, fars=fars, at=at)
    out.update(hist_same=hs, hist_other=ho, d_max=d_max)
    return out


def verification_score_metrics(scores, same, fars=DEFAULT_FARS, bins=4096, at=None, device=None):
    """The same metrics over similarity scores in [0, 1] where LARGER means same (the Siamese 'l1' head's sigmoid): scores [m],
    same [m].  lo = 0, w = 1 / bins, accept='above': a pair is accepted at threshold t iff its score is at least t."""
    bins = _check_bins(bins, "verification_score_metrics")
    fars = _far_list(fars)
    dev = _device_of(scores, device)
    s = torch.as_tensor(np.asarray(scores) if not torch.is_tensor(scores) else scores)
    s = s.to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    flags = _pair_inputs("verification_score_metrics", same, s.numel(), dev)
    hs, ho = ops.verification_values(s, flags, lo=0.0, w=1.0 / bins, bins=bins)
    hs, ho = hs.cpu().numpy(), ho.cpu().numpy()
    out = verification_from_histograms(hs, ho, 0.0, 1.0 / bins, fars=fars, at=at, accept='above')
    out.update(hist_same=hs, hist_other=ho)
    return out
