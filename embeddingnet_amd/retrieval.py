"""Retrieval metrics on embeddings: Recall@K and mean reciprocal rank, for any K and any gallery size.

The rank of a query is the position of its nearest same-class gallery item among the gallery ordered by (squared Euclidean
distance, gallery index): 1 + the number of other-class items in front of it.  recall@K = the share of queries with rank <= K,
mrr = the mean of 1 / rank — both over the queries that have a same-class item at all (`n_valid`); a query without one has
rank 0 and is left out.  The ranks come from ops.retrieval_first_positive, two passes of the fp32 MFMA distance GEMM whose
epilogue keeps a minimum and a count instead of storing the [nq, n] matrix (csrc/retrieval.hip); the sums from
ops.retrieval_reduce.  Out of scope: MAP@R and R-precision (they need the rank of EVERY positive, not the first), and a query
set that is a strict subset of its gallery (leave-one-out needs queries and gallery to be the same rows in the same order).
"""
import numpy as np
import torch

from . import ops


def _as_block(a, dev):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    t = t.to(device=dev, dtype=torch.float32)
    if t.dim() != 2:
        raise ValueError(f"retrieval_metrics: encodings must be [rows, e] (got {tuple(t.shape)})")
    return t.contiguous()


def _label_list(labels):
    if torch.is_tensor(labels):
        labels = labels.detach().cpu().numpy()
    if isinstance(labels, np.ndarray):
        labels = labels.tolist()
    return list(labels)


def retrieval_metrics(encodings, labels=None, ks=(1, 5, 10), gallery=None, gallery_labels=None, device=None):
    """-> {'recall@K': float for K in ks, 'mrr': float, 'n_queries': int, 'n_valid': int, 'ranks': np.ndarray[int32]}.

    encodings: [nq, e] array or tensor, or the {'encodings', 'labels', ...} dict of EmbeddingNet.generate_encodings /
    load_encodings (then `labels` may be omitted).  labels: one hashable per row.  gallery / gallery_labels: the set searched;
    None = leave-one-out within `encodings` (every query skips itself).  ks: cut-offs >= 1, no upper limit.
    With no valid query the metric values are NaN and the counts 0."""
    if isinstance(encodings, dict):
        if labels is None:
            labels = encodings['labels']
        encodings = encodings['encodings']
    if isinstance(gallery, dict):
        if gallery_labels is None:
            gallery_labels = gallery['labels']
        gallery = gallery['encodings']
    ks = [k for k in ks]
    if len(ks) == 0:
        raise ValueError("retrieval_metrics: ks is empty")
    if any(int(k) != k or int(k) < 1 for k in ks):
        raise ValueError(f"retrieval_metrics: every K must be an integer >= 1 (got {ks})")
    ks = [int(k) for k in ks]
    if labels is None:
        raise ValueError("retrieval_metrics: labels are needed")
    if (gallery is None) != (gallery_labels is None):
        raise ValueError("retrieval_metrics: gallery and gallery_labels come together")
    if device is None:
        if torch.is_tensor(encodings) and encodings.is_cuda:
            device = encodings.device
        else:
            from .backbones import default_device
            device = default_device()
    labels = _label_list(labels)
    n_rows = encodings.shape[0] if hasattr(encodings, 'shape') else len(encodings)
    if len(labels) != n_rows:
        raise ValueError(f"retrieval_metrics: {n_rows} encodings but {len(labels)} labels")
    if n_rows == 0:
        raise ValueError("retrieval_metrics: no encodings")
    if gallery is not None:
        gallery_labels = _label_list(gallery_labels)
        g_rows = gallery.shape[0] if hasattr(gallery, 'shape') else len(gallery)
        if len(gallery_labels) != g_rows:
            raise ValueError(f"retrieval_metrics: {g_rows} gallery encodings but {len(gallery_labels)} gallery labels")
        if g_rows == 0:
            raise ValueError("retrieval_metrics: empty gallery")
    q = _as_block(encodings, device)
    x = None
    if gallery is not None:
        x = _as_block(gallery, device)
        if x.shape[1] != q.shape[1]:
            raise ValueError(f"retrieval_metrics: widths differ ({q.shape[1]} vs {x.shape[1]})")
    # one label -> int32 mapping for queries and gallery (as KNNClassifier.fit: position among the sorted distinct labels)
    classes = sorted(set(labels) | set(gallery_labels or ()))
    lookup = {c: i for i, c in enumerate(classes)}
    ql = torch.tensor([lookup[l] for l in labels], dtype=torch.int32, device=device)
    xl = None if x is None else torch.tensor([lookup[l] for l in gallery_labels], dtype=torch.int32, device=device)

    rank, _, _ = ops.retrieval_first_positive(q, ql, x, xl)
    hits, n_valid, sum_inv = ops.retrieval_reduce(rank, ks)
    hits, n_valid, sum_inv = hits.cpu().numpy(), int(n_valid.item()), float(sum_inv.item())
    out = {}
    for k, h in zip(ks, hits):
        out[f'recall@{k}'] = float(h) / n_valid if n_valid else float('nan')
    out['mrr'] = sum_inv / n_valid if n_valid else float('nan')
    out['n_queries'] = int(q.shape[0]) if n_valid else 0
    out['n_valid'] = n_valid
    out['ranks'] = rank.cpu().numpy().astype(np.int32, copy=False)
    return out
