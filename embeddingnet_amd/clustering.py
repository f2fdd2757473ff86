"""Clustering quality of encodings: NMI of a k-means clustering against the class labels, the third evaluation metric of the
metric-learning literature next to Recall@K and MAP@R (retrieval.py).

The clustering is kmeans.KMeans, on the device.  The scores work from the contingency table of two label vectors, after one
copy of the int32 cluster ids to the host: O(n) bookkeeping in float64 NumPy, with scikit-learn's definitions
(normalized_mutual_info_score, homogeneity_completeness_v_measure).  Adjusted mutual information is not offered: its
expected-MI term costs O(rows x columns x n).
"""
import numpy as np

_AVERAGES = {
    'min': min,
    'max': max,
    'arithmetic': lambda a, b: 0.5 * (a + b),
    'geometric': lambda a, b: float(np.sqrt(a * b)),
}


def _ids(labels):
    """Any sequence of hashables -> (dense ids int64 [n], number of distinct labels), ids in order of first appearance."""
    if hasattr(labels, 'detach'):
        labels = labels.detach().cpu().numpy()
    if isinstance(labels, np.ndarray):
        labels = labels.ravel().tolist()
    lookup = {}
    ids = np.fromiter((lookup.setdefault(l, len(lookup)) for l in labels), dtype=np.int64)
    return ids, len(lookup)


def contingency(labels_true, labels_pred):
    """-> int64 [classes, clusters]: how many items of each class fell into each cluster."""
    t, r = _ids(labels_true)
    p, c = _ids(labels_pred)
    if t.shape[0] != p.shape[0]:
        raise ValueError(f"clustering: {t.shape[0]} true labels but {p.shape[0]} predicted ones")
    return np.bincount(t * max(c, 1) + p, minlength=r * c).reshape(r, c)


def _entropy(counts):
    counts = counts[counts > 0].astype(np.float64)
    if counts.size <= 1:
        return 0.0
    total = counts.sum()
    return float(-np.sum((counts / total) * (np.log(counts) - np.log(total))))


def _mutual_information(table):
    n = float(table.sum())
    i, j = np.nonzero(table)
    nij = table[i, j].astype(np.float64)
    a = table.sum(axis=1).astype(np.float64)[i]
    b = table.sum(axis=0).astype(np.float64)[j]
    mi = np.sum((nij / n) * (np.log(nij) - np.log(n)) + (nij / n) * (2.0 * np.log(n) - np.log(a) - np.log(b)))
    return float(max(mi, 0.0))


def nmi(labels_true, labels_pred, average_method='arithmetic'):
    """scikit-learn's normalized_mutual_info_score: MI / average(H(true), H(pred)), natural logarithms.  Labels are any
    hashables.  Both sides a single cluster: 1.0; one side a single cluster (no information shared): 0.0."""
    if average_method not in _AVERAGES:
        raise ValueError(f"nmi: average_method must be one of {sorted(_AVERAGES)} (got {average_method!r})")
    table = contingency(labels_true, labels_pred)
    if table.shape[0] <= 1 and table.shape[1] <= 1:
        return 1.0
    mi = _mutual_information(table)
    if abs(mi) < np.finfo(np.float64).eps:
        return 0.0
    h_true, h_pred = _entropy(table.sum(axis=1)), _entropy(table.sum(axis=0))
    return float(mi / _AVERAGES[average_method](h_true, h_pred))


def homogeneity_completeness(labels_true, labels_pred):
    """-> (homogeneity = MI / H(true), completeness = MI / H(pred)); a side without entropy scores 1.0, as in scikit-learn."""
    table = contingency(labels_true, labels_pred)
    if table.size == 0:
        return 1.0, 1.0
    mi = _mutual_information(table)
    h_true, h_pred = _entropy(table.sum(axis=1)), _entropy(table.sum(axis=0))
    return (mi / h_true if h_true else 1.0), (mi / h_pred if h_pred else 1.0)


def purity(labels_true, labels_pred):
    """The share of items that belong to the majority class of their cluster."""
    table = contingency(labels_true, labels_pred)
    return float(table.max(axis=0).sum()) / float(table.sum()) if table.size else 1.0


def clustering_metrics(encodings, labels=None, n_clusters=None, seed=0, n_init=1, max_iter=300, device=None):
    """-> {'nmi', 'homogeneity', 'completeness', 'purity', 'inertia': float, 'n_iter', 'n_empty', 'n_clusters': int}.

    encodings: [n, e] array or tensor, or the {'encodings', 'labels', ...} dict of EmbeddingNet.generate_encodings (then
    `labels` may be omitted).  labels: one hashable per row.  The encodings are clustered by kmeans.KMeans(n_clusters,
    init='k-means++', seed=seed, n_init=n_init, max_iter=max_iter) — n_clusters None: the number of distinct labels — and the
    cluster ids are scored against the labels."""
    from .kmeans import KMeans
    if isinstance(encodings, dict):
        if labels is None:
            labels = encodings['labels']
        encodings = encodings['encodings']
    if labels is None:
        raise ValueError("clustering_metrics: labels are needed")
    n_rows = encodings.shape[0] if hasattr(encodings, 'shape') else len(encodings)
    if hasattr(encodings, 'reshape') and n_rows:
        encodings = encodings.reshape(n_rows, -1)
    ids, distinct = _ids(labels)
    if ids.shape[0] != n_rows:
        raise ValueError(f"clustering_metrics: {n_rows} encodings but {ids.shape[0]} labels")
    if n_rows == 0:
        raise ValueError("clustering_metrics: no encodings")
    k = distinct if n_clusters is None else int(n_clusters)
    km = KMeans(k, seed=seed, n_init=n_init, max_iter=max_iter, device=device).fit(encodings)
    hom, com = homogeneity_completeness(ids, km.labels_)
    return {'nmi': nmi(ids, km.labels_), 'homogeneity': hom, 'completeness': com, 'purity': purity(ids, km.labels_),
            'inertia': km.inertia_, 'n_iter': km.n_iter_, 'n_empty': km.n_empty_, 'n_clusters': k}
