"""Float64 restatement of the positive-ranks contract (include/embnet.h, "MAP@R, R-precision"), NumPy only.

Order: lexicographic on (d2, gallery index), NaN = +inf.  Positive of query r: a non-excluded column with the query's label.  With
R positives p_1 .. p_R in that order, pos(p_j) = the 1-based position of p_j among all non-excluded columns.  Per query
r_precision = #{pos <= R} / R, ap@r = (1 / R) sum_{pos(p_j) <= R} j / pos(p_j), ap = (1 / R) sum_j j / pos(p_j); NaN for R = 0; the
means run over the queries with R > 0.
"""
import math

import numpy as np

import retrieval_ref as RR


def positions_exact(d2, ql, xl, self_exclude, rows=None):
    """d2 [b, n] of the queries `rows` (default: row i is query i) -> CSR (offset int64 [b+1], pos_index int32, pos_rank int32) by a
    full sort of every row under the (d2, index) order."""
    d2 = np.array(d2, dtype=np.float64, copy=True)
    d2[np.isnan(d2)] = np.inf
    b, n = d2.shape
    rows = np.arange(b) if rows is None else np.asarray(rows)
    ql, xl = np.asarray(ql), np.asarray(xl)
    offset, idx, rank = [0], [], []
    for i, r in enumerate(rows):
        order = np.argsort(d2[i], kind='stable')                  # stable: equal d2 keep the index order
        if self_exclude:
            order = order[order != r]
        hit = np.flatnonzero(xl[order] == ql[r])
        idx.append(order[hit])
        rank.append(hit + 1)
        offset.append(offset[-1] + len(hit))
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return np.asarray(offset, np.int64), cat(idx), cat(rank)


def query_metrics(pos):
    """One query's (ap@r, r_precision, ap) from its positions in ascending order (exactly rounded sums); NaN without a positive."""
    R = len(pos)
    if R == 0:
        return float('nan'), float('nan'), float('nan')
    pos = np.asarray(pos, np.float64)
    term = np.arange(1, R + 1, dtype=np.float64) / pos
    inside = pos <= R
    return math.fsum(term[inside]) / R, float(inside.sum()) / R, math.fsum(term) / R


def metrics_from_positions(offset, pos_rank):
    """CSR positions -> {'ap@r', 'r_precision_q', 'ap' (float64 [nq], NaN where R = 0), 'r' (int32 [nq]), 'map@r', 'r_precision',
    'map' (means over R > 0; NaN without a valid query), 'n_valid', 'n_queries' (0 without a valid query)}."""
    offset = np.asarray(offset, np.int64)
    nq = len(offset) - 1
    per = np.array([query_metrics(pos_rank[offset[i]:offset[i + 1]]) for i in range(nq)], np.float64).reshape(nq, 3)
    r = np.diff(offset).astype(np.int32)
    valid = r > 0
    nv = int(valid.sum())
    mean = lambda col: math.fsum(per[valid, col]) / nv if nv else float('nan')
    return {'ap@r': per[:, 0], 'r_precision_q': per[:, 1], 'ap': per[:, 2], 'r': r, 'map@r': mean(0), 'r_precision': mean(1),
            'map': mean(2), 'n_valid': nv, 'n_queries': nq if nv else 0}


def position_interval(q, x, ql, xl, self_exclude, A, rows=None):
    """The positions any kernel may report whose distances satisfy |d2 - d2_f64| <= B, B[r, c] = A * (|q_r|^2 + |x_c|^2).  Per
    positive p of a query (the live columns are the non-excluded ones):
         lo = 1 + #{other live j : d_j + B_j <  d_p - B_p}
         hi = 1 + #{other live j : d_j - B_j <= d_p + B_p}
    -> CSR (offset int64 [b+1], pos_index int32, lo int64, hi int64): a query's positives in gallery-index order."""
    q64, x64 = np.asarray(q, np.float64), np.asarray(x, np.float64)
    ql, xl = np.asarray(ql), np.asarray(xl)
    qn, xn = (q64 * q64).sum(1), (x64 * x64).sum(1)
    rows = np.arange(len(q64)) if rows is None else np.asarray(rows)
    n = len(x64)
    col = np.arange(n)
    parts = {}
    for idx, d2 in RR.sqdist_blocks(q64, x64, rows=rows):
        B = A * (qn[idx][:, None] + xn[None, :])
        up, dn = d2 + B, d2 - B
        if self_exclude:                                          # the excluded column sorts behind everything and is never counted
            up[np.arange(len(idx)), idx] = np.inf
            dn[np.arange(len(idx)), idx] = np.inf
        up_sorted, dn_sorted = np.sort(up, axis=1), np.sort(dn, axis=1)
        for i, r in enumerate(idx):
            p = np.flatnonzero((xl == ql[r]) & ((col != r) if self_exclude else True))
            lo = 1 + np.searchsorted(up_sorted[i], d2[i, p] - B[i, p], side='left')
            hi = np.searchsorted(dn_sorted[i], d2[i, p] + B[i, p], side='right')      # counts p itself: 1 + (count - 1)
            parts[int(r)] = (p.astype(np.int32), lo.astype(np.int64), hi.astype(np.int64))
    offset = np.zeros(len(rows) + 1, np.int64)
    for i, r in enumerate(rows):
        offset[i + 1] = offset[i] + len(parts[int(r)][0])
    cat = lambda k, t: np.concatenate([parts[int(r)][k] for r in rows]).astype(t) if len(rows) else np.zeros(0, t)
    return offset, cat(0, np.int32), cat(1, np.int64), cat(2, np.int64)


def metric_bounds(offset, lo, hi):
    """All three per-query metrics are non-increasing in every position, so the sorted `hi` vector gives their lower bound and the
    sorted `lo` vector their upper bound -> (lower, upper), each a metrics_from_positions dict."""
    offset = np.asarray(offset, np.int64)
    srt = lambda v: np.concatenate([np.sort(v[offset[i]:offset[i + 1]]) for i in range(len(offset) - 1)]) if len(v) else v
    return metrics_from_positions(offset, srt(hi)), metrics_from_positions(offset, srt(lo))
