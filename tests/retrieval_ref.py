"""Float64 restatement of the retrieval contract (include/embnet.h, "retrieval evaluation"), NumPy only.

Order: lexicographic on (d2, gallery index).  Positive of query r: a non-excluded column with the query's label.  rank = 1 + the
number of non-excluded negatives in front of the first positive, 0 without a positive.  Metrics over the queries with rank > 0.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_CHUNK_ELEMS = 1 << 23                                   # float64 elements of one (rows x n x e) difference block: 64 MiB


def _sq_rows(qb, x):
    """[b, n] = sum_k (qb[r, k] - x[c, k])^2 in float64, a few rows at a time."""
    n, e = x.shape
    step = max(1, _CHUNK_ELEMS // max(n * e, 1))
    out = np.empty((len(qb), n), np.float64)
    for r0 in range(0, len(qb), step):
        d = qb[r0:r0 + step, None, :] - x[None, :, :]
        out[r0:r0 + step] = np.einsum('rnk,rnk->rn', d, d)
    return out


def sqdist_blocks(q, x, block=256, rows=None):
    """Yield (row indices, d2 [b, n] float64) over the queries (all, or the `rows` given) in blocks of <= `block` <= 256 rows."""
    assert 1 <= block <= 256
    q = np.asarray(q, np.float64)
    x = np.asarray(x, np.float64)
    rows = np.arange(len(q)) if rows is None else np.asarray(rows)
    parts = [rows[i:i + block] for i in range(0, len(rows), block)]
    with ThreadPoolExecutor(max_workers=8) as pool:
        # a window of blocks in flight: NumPy releases the GIL inside the subtraction and the einsum
        for w0 in range(0, len(parts), 8):
            window = parts[w0:w0 + 8]
            for idx, d2 in zip(window, pool.map(lambda idx: _sq_rows(q[idx], x), window)):
                yield idx, d2


def sqdist64(q, x, block=256):
    """[nq, n] float64 matrix of sum (q - x)^2 (only for sizes whose matrix fits; the other functions stream the blocks)."""
    out = np.empty((len(q), len(x)), np.float64)
    for idx, d2 in sqdist_blocks(q, x, block):
        out[idx] = d2
    return out


def _excluded(idx, n, self_exclude):
    ex = np.zeros((len(idx), n), bool)
    if self_exclude:
        ex[np.arange(len(idx)), idx] = True
    return ex


def ranks_exact(d2, ql, xl, self_exclude, rows=None):
    """d2 [b, n] (any float dtype; NaN counts as +inf) of the queries `rows` (default: row i is query i)
    -> (rank int32 [b], pos_index int32 [b], pos_d2 [b] in d2's dtype)."""
    d2 = np.array(d2, copy=True)
    d2[np.isnan(d2)] = np.inf
    b, n = d2.shape
    rows = np.arange(b) if rows is None else np.asarray(rows)
    ql, xl = np.asarray(ql), np.asarray(xl)
    ex = _excluded(rows, n, self_exclude)
    same = xl[None, :] == ql[rows][:, None]
    pos, neg = same & ~ex, ~same & ~ex
    has = pos.any(1)
    dpos = np.where(pos, d2, np.inf)
    # the first positive: smallest d2, then smallest index — argmin returns the first minimum; where that minimum is +inf every
    # positive sits at +inf (a masked column may too), and the first positive by index is the one
    p = dpos.argmin(1)
    p = np.where(np.isinf(dpos[np.arange(b), p]), pos.argmax(1), p)
    pd = d2[np.arange(b), p]
    before = neg & ((d2 < pd[:, None]) | ((d2 == pd[:, None]) & (np.arange(n)[None, :] < p[:, None])))
    rank = np.where(has, 1 + before.sum(1), 0).astype(np.int32)
    pos_index = np.where(has, p, -1).astype(np.int32)
    pos_d2 = np.where(has, pd, np.inf).astype(d2.dtype)
    return rank, pos_index, pos_d2


def rank_interval(q, x, ql, xl, self_exclude, A, rows=None, details=False, gap_ks=()):
    """The ranks any kernel may report whose distances satisfy |d2 - d2_f64| <= B, B[r, c] = A * (|q_r|^2 + |x_c|^2):
         r_lo = 1 + #{negatives j : d2_j + B_j <  min_p (d2_p - B_p)}
         r_hi = 1 + #{negatives j : d2_j - B_j <= min_p (d2_p + B_p)}
    (both 0 for a query without a positive).  A is the caller's A(e) — tests/test_eval_path_gpu.py::_A: 2e-6 up to e = 512,
    4e-6 * sqrt(e / 512) beyond, the project's derived bound for this GEMM engine and epilogue.
    details: also a dict with, per query, rank / pos_index / pos_d2 of the float64 order, pos_hi = min_p (d2_p + B_p),
    bmax = max_c B, and for each K of gap_ks the K-th and (K+1)-th smallest non-excluded d2 (kth [b, len(gap_ks), 2])."""
    q64, x64 = np.asarray(q, np.float64), np.asarray(x, np.float64)
    ql, xl = np.asarray(ql), np.asarray(xl)
    qn, xn = (q64 * q64).sum(1), (x64 * x64).sum(1)
    rows = np.arange(len(q64)) if rows is None else np.asarray(rows)
    n = len(x64)
    lo, hi = np.zeros(len(q64), np.int64), np.zeros(len(q64), np.int64)
    det = {k: np.zeros(len(q64), t) for k, t in (('rank', np.int32), ('pos_index', np.int32), ('pos_d2', np.float64),
                                                ('pos_hi', np.float64), ('bmax', np.float64))}
    det['kth'] = np.zeros((len(q64), len(gap_ks), 2))
    for idx, d2 in sqdist_blocks(q64, x64, rows=rows):
        B = A * (qn[idx][:, None] + xn[None, :])
        ex = _excluded(idx, n, self_exclude)
        same = xl[None, :] == ql[idx][:, None]
        pos, neg = same & ~ex, ~same & ~ex
        has = pos.any(1)
        p_lo = np.where(pos, d2 - B, np.inf).min(1)
        p_hi = np.where(pos, d2 + B, np.inf).min(1)
        lo[idx] = np.where(has, 1 + (neg & (d2 + B < p_lo[:, None])).sum(1), 0)
        hi[idx] = np.where(has, 1 + (neg & (d2 - B <= p_hi[:, None])).sum(1), 0)
        if details:
            det['rank'][idx], det['pos_index'][idx], det['pos_d2'][idx] = ranks_exact(d2, ql, xl, self_exclude, rows=idx)
            det['pos_hi'][idx], det['bmax'][idx] = p_hi, B.max(1)
            if len(gap_ks):
                live = np.where(ex, np.inf, d2)
                part = np.sort(live, axis=1)[:, :max(gap_ks) + 1]
                for i, k in enumerate(gap_ks):
                    det['kth'][idx, i, 0] = part[:, k - 1]
                    det['kth'][idx, i, 1] = part[:, k] if k < part.shape[1] else np.inf
    lo, hi = lo[rows], hi[rows]
    if details:
        return lo, hi, {k: v[rows] for k, v in det.items()}
    return lo, hi


def metrics(rank, ks):
    """The contract's metric arithmetic on a rank vector: recall@K and mrr over rank > 0; NaN values and zero counts without one."""
    rank = np.asarray(rank)
    valid = rank[rank > 0]
    nv = int(len(valid))
    out = {f'recall@{k}': (float((valid <= k).sum()) / nv if nv else float('nan')) for k in ks}
    out['mrr'] = float((1.0 / valid.astype(np.float64)).sum()) / nv if nv else float('nan')
    out['n_queries'] = int(len(rank)) if nv else 0
    out['n_valid'] = nv
    return out
