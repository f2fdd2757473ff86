"""Retrieval metrics on embeddings: Recall@K and mean reciprocal rank, for any K and any gallery size.

The rank of a query is the position of its nearest same-class gallery item among the gallery ordered by (squared Euclidean
distance, gallery index): 1 + the number of other-class items in front of it.  recall@K = the share of queries with rank <= K,
mrr = the mean of 1 / rank — both over the queries that have a same-class item at all (`n_valid`); a query without one has
rank 0 and is left out.  The ranks come from ops.retrieval_first_positive, two passes of the fp32 MFMA distance GEMM whose
epilogue keeps a minimum and a count instead of storing the [nq, n] matrix (csrc/retrieval.hip); the sums from
ops.retrieval_reduce.

MAP@R and R-precision (Musgrave et al., "A Metric Learning Reality Check") look at EVERY same-class item: with R the number of
a query's positives and pos(p_j) the position of its j-th nearest positive among all gallery items, r_precision = the share of
the positives with pos <= R, ap@r = (1 / R) * the sum of j / pos(p_j) over those, ap the same sum over all positives
(retrieval_map_metrics; ops.retrieval_positive_ranks keeps every positive's key in pass 1 and counts the negatives in front of
each in pass 2, ops.retrieval_map_reduce sums).  Out of scope: a query set that is a strict subset of its gallery (leave-one-out
needs queries and gallery to be the same rows in the same order), and classes above ops.R_MAX = 4096 positives per query.

nearest_neighbors answers the other question — WHICH gallery items are nearest to a query: the k smallest (distance, index)
per query among all items, the same-class ones or the other-class ones, from one walk of the same GEMM whose epilogue keeps
each row's candidates in LDS (ops.knn_search, csrc/knn_search.hip).  No [nq, n] matrix is formed there either.
"""
import numpy as np
import torch

from . import ops


def _as_block(a, dev, who="retrieval_metrics"):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    t = t.to(device=dev, dtype=torch.float32)
    if t.dim() != 2:
        raise ValueError(f"{who}: encodings must be [rows, e] (got {tuple(t.shape)})")
    return t.contiguous()


def _label_list(labels):
    if torch.is_tensor(labels):
        labels = labels.detach().cpu().numpy()
    if isinstance(labels, np.ndarray):
        labels = labels.tolist()
    return list(labels)


def _unpack(encodings, labels, gallery, gallery_labels):
    """The {'encodings', 'labels', ...} dict form of either set -> arrays and labels."""
    if isinstance(encodings, dict):
        if labels is None:
            labels = encodings['labels']
        encodings = encodings['encodings']
    if isinstance(gallery, dict):
        if gallery_labels is None:
            gallery_labels = gallery['labels']
        gallery = gallery['encodings']
    return encodings, labels, gallery, gallery_labels


def _blocks(who, encodings, labels, gallery, gallery_labels, device):
    """The input conventions both metric functions share -> (q, ql, x, xl, classes): float32 blocks and int32 labels on the
    device (x, xl None: leave-one-out), classes[i] the label that id i stands for.  ValueError for what cannot be honoured."""
    if labels is None:
        raise ValueError(f"{who}: labels are needed")
    if (gallery is None) != (gallery_labels is None):
        raise ValueError(f"{who}: gallery and gallery_labels come together")
    if device is None:
        if torch.is_tensor(encodings) and encodings.is_cuda:
            device = encodings.device
        else:
            from .backbones import default_device
            device = default_device()
    labels = _label_list(labels)
    n_rows = encodings.shape[0] if hasattr(encodings, 'shape') else len(encodings)
    if len(labels) != n_rows:
        raise ValueError(f"{who}: {n_rows} encodings but {len(labels)} labels")
    if n_rows == 0:
        raise ValueError(f"{who}: no encodings")
    if gallery is not None:
        gallery_labels = _label_list(gallery_labels)
        g_rows = gallery.shape[0] if hasattr(gallery, 'shape') else len(gallery)
        if len(gallery_labels) != g_rows:
            raise ValueError(f"{who}: {g_rows} gallery encodings but {len(gallery_labels)} gallery labels")
        if g_rows == 0:
            raise ValueError(f"{who}: empty gallery")
    q = _as_block(encodings, device, who)
    x = None
    if gallery is not None:
        x = _as_block(gallery, device, who)
        if x.shape[1] != q.shape[1]:
            raise ValueError(f"{who}: widths differ ({q.shape[1]} vs {x.shape[1]})")
    # one label -> int32 mapping for queries and gallery (as KNNClassifier.fit: position among the sorted distinct labels)
    classes = sorted(set(labels) | set(gallery_labels or ()))
    lookup = {c: i for i, c in enumerate(classes)}
    ql = torch.tensor([lookup[l] for l in labels], dtype=torch.int32, device=device)
    xl = None if x is None else torch.tensor([lookup[l] for l in gallery_labels], dtype=torch.int32, device=device)
    return q, ql, x, xl, classes


def retrieval_metrics(encodings, labels=None, ks=(1, 5, 10), gallery=None, gallery_labels=None, device=None):
    """-> {'recall@K': float for K in ks, 'mrr': float, 'n_queries': int, 'n_valid': int, 'ranks': np.ndarray[int32]}.

    encodings: [nq, e] array or tensor, or the {'encodings', 'labels', ...} dict of EmbeddingNet.generate_encodings /
    load_encodings (then `labels` may be omitted).  labels: one hashable per row.  gallery / gallery_labels: the set searched;
    None = leave-one-out within `encodings` (every query skips itself).  ks: cut-offs >= 1, no upper limit.
    With no valid query the metric values are NaN and the counts 0."""
    encodings, labels, gallery, gallery_labels = _unpack(encodings, labels, gallery, gallery_labels)
    ks = [k for k in ks]
    if len(ks) == 0:
        raise ValueError("retrieval_metrics: ks is empty")
    if any(int(k) != k or int(k) < 1 for k in ks):
        raise ValueError(f"retrieval_metrics: every K must be an integer >= 1 (got {ks})")
    ks = [int(k) for k in ks]
    q, ql, x, xl, _ = _blocks("retrieval_metrics", encodings, labels, gallery, gallery_labels, device)

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


def retrieval_map_metrics(encodings, labels=None, gallery=None, gallery_labels=None, device=None):
    """-> {'map@r', 'r_precision', 'map': float, 'n_queries', 'n_valid': int, 'ap@r': np.ndarray[float64] (NaN for a query without
    a positive), 'r': np.ndarray[int32] (the number of positives of each query)}.

    The inputs are retrieval_metrics': arrays, tensors or the encodings dict; gallery None = leave-one-out.  The three values are
    means over the queries that have a positive (`n_valid`); with none they are NaN and the counts 0.  A class with more than
    ops.R_MAX positives per query is refused with a ValueError."""
    encodings, labels, gallery, gallery_labels = _unpack(encodings, labels, gallery, gallery_labels)
    q, ql, x, xl, classes = _blocks("retrieval_map_metrics", encodings, labels, gallery, gallery_labels, device)
    sizes = torch.bincount((ql if xl is None else xl).long(), minlength=len(classes))
    r = (sizes[ql.long()] - (1 if xl is None else 0)).clamp(min=0)
    worst = int(r.argmax().item())
    if int(r[worst].item()) > ops.R_MAX:
        c = int(ql[worst].item())
        raise ValueError(f"retrieval_map_metrics: label {classes[c]!r} has {int(sizes[c].item())} gallery items; more than "
                         f"{ops.R_MAX} positives per query are not supported")
    total = int(r.sum().item())
    offset, _, pos_rank = ops.retrieval_positive_ranks(q, ql, x, xl, num_classes=len(classes), capacity=max(total, 1))
    ap_at_r, _, _, sums, n_valid = ops.retrieval_map_reduce(offset, pos_rank)
    sums, n_valid = sums.cpu().numpy(), int(n_valid.item())
    out = {}
    for name, s in zip(('map@r', 'r_precision', 'map'), sums):
        out[name] = float(s) / n_valid if n_valid else float('nan')
    out['n_queries'] = int(q.shape[0]) if n_valid else 0
    out['n_valid'] = n_valid
    out['ap@r'] = ap_at_r.cpu().numpy()
    out['r'] = r.cpu().numpy().astype(np.int32, copy=False)
    return out


def nearest_neighbors(encodings, k, labels=None, gallery=None, gallery_labels=None, select='all', squared=False, device=None):
    """-> {'distances': np.ndarray[float32] [nq, k], 'indices': np.ndarray[int32] [nq, k], 'found': np.ndarray[int32] [nq]}: the k
    nearest gallery items of every query, nearest first, ties to the smaller gallery index.

    The inputs are retrieval_metrics': arrays, tensors or the encodings dict; labels any hashables; gallery None = leave-one-out
    within `encodings` (a query never returns itself).  select: 'all' — every gallery item (labels may be omitted); 'same' —
    only items with the query's label; 'other' — only items with another label.  found[r] = min(k, eligible items of query r);
    the entries of a row from found[r] on are index -1 and distance +inf.  1 <= k <= ops.KNN_K_MAX = 128.  The search runs on the
    streaming distance walk (ops.knn_search): no [nq, n] matrix is formed, so the gallery can be a whole training set.

    The k hardest negatives of every training sample, over the whole dataset:

        hard = nearest_neighbors(train_encodings, 10, labels=train_labels, select='other')
        hard['indices'][i]        # the 10 samples of other classes nearest to sample i, nearest first

    and its nearest positives (a class with fewer than k + 1 members gives found < k):

        pos = nearest_neighbors(train_encodings, 5, labels=train_labels, select='same')
        pos['indices'][i, :pos['found'][i]]
    """
    who = "nearest_neighbors"
    encodings, labels, gallery, gallery_labels = _unpack(encodings, labels, gallery, gallery_labels)
    if select not in ops.KNN_SELECT:
        raise ValueError(f"{who}: select must be one of {sorted(ops.KNN_SELECT)} (got {select!r})")
    if int(k) != k or not 1 <= int(k) <= ops.KNN_K_MAX:
        raise ValueError(f"{who}: k must be an integer in [1, {ops.KNN_K_MAX}] (got {k})")
    if select == 'all' and gallery is not None and gallery_labels is None:
        labels = None                                       # nothing to compare them with: the search reads no label
    if labels is None:
        if select != 'all':
            raise ValueError(f"{who}: select={select!r} needs labels")
        n_rows = encodings.shape[0] if hasattr(encodings, 'shape') else len(encodings)
        dummy = [0] * n_rows
        g_rows = 0 if gallery is None else (gallery.shape[0] if hasattr(gallery, 'shape') else len(gallery))
        q, _, x, _, _ = _blocks(who, encodings, dummy, gallery, None if gallery is None else [0] * g_rows, device)
        ql = xl = None
    else:
        q, ql, x, xl, _ = _blocks(who, encodings, labels, gallery, gallery_labels, device)
    dist, idx, found = ops.knn_search(q, x, int(k), ql, xl, select=select, squared=squared)
    return {'distances': dist.cpu().numpy(), 'indices': idx.cpu().numpy().astype(np.int32, copy=False),
            'found': found.cpu().numpy().astype(np.int32, copy=False)}
