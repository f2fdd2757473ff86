"""Oracle (test infrastructure): brute-force k-NN on embeddings, the arithmetic scikit-learn's
KNeighborsClassifier (reference models.py:15; third-party, unpinned, 1.7.2 here) performs for
algorithm='brute', metric Euclidean, uniform weights: euclidean_distances(Q, X) with f64 accumulation
for f32 input, the k smallest per row in ascending order, majority vote with ties to the smallest class.
Pinned by tests/golden/knn.npz (real sklearn output)."""
import numpy as np


def cross_distances(q, x):
    q64, x64 = np.asarray(q, np.float32).astype(np.float64), np.asarray(x, np.float32).astype(np.float64)
    d = -2.0 * (q64 @ x64.T) + (q64 * q64).sum(1)[:, None] + (x64 * x64).sum(1)[None, :]
    d = np.maximum(d.astype(np.float32), 0)
    return np.sqrt(d)


def cross_sqdist64(q, x):
    """The same formula kept in float64, unclamped and unrounded: the yardstick an fp32 distance kernel is measured by.
    -> (d2 [nq,n], |q|^2 [nq], |x|^2 [n])"""
    q64, x64 = np.asarray(q, np.float32).astype(np.float64), np.asarray(x, np.float32).astype(np.float64)
    qn, xn = (q64 * q64).sum(1), (x64 * x64).sum(1)
    d = q64 @ x64.T
    d *= -2.0
    d += qn[:, None]
    d += xn[None, :]
    return d, qn, xn


def topk_smallest(d, k):
    """The k smallest entries of each row of a given matrix, ascending, ties to the smaller column (a stable sort).
    NaN counts as +inf, in the order as in the reported value: it ties with +inf by column and never precedes a
    finite entry.  -> (values, indices)"""
    d = np.asarray(d)
    d = np.where(np.isnan(d), np.asarray(np.inf, d.dtype), d)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, idx, 1), idx


def kneighbors(q, x, k):
    return topk_smallest(cross_distances(q, x), k)


def vote(votes):
    """Majority of each row of integer class ids, ties to the smallest id (scipy.stats.mode, as sklearn's predict)."""
    return np.array([np.bincount(v).argmax() for v in np.asarray(votes)])


def predict(q, x, labels, k):
    """labels: integer class ids [n]."""
    _, idx = kneighbors(q, x, k)
    return vote(np.asarray(labels)[idx])
