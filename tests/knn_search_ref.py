"""Float64 restatement of the k-nearest-neighbour search contract (include/embnet.h, "k-nearest-neighbour search"), NumPy only.

Key of gallery column c for query r: (d2[r, c], c), NaN counting as +inf; order: lexicographic.  Eligible columns: not the query's
own (leave-one-out), and by `select` 0 all / 1 the query's label / 2 another label.  The answer of a row: its min(k, eligible)
smallest keys, ascending, padded with index -1 and d2 = +inf; found = min(k, eligible).

check(): the answers a kernel may give whose distances satisfy |d2 - d2_f64| <= B, B[r, c] = A * (|q_r|^2 + |x_c|^2), A the
project's bound for this GEMM engine (tests/test_eval_path_gpu.py::_A).
"""
import numpy as np

import retrieval_ref as RR


def A(e):
    """tests/test_eval_path_gpu.py::_A"""
    return 2e-6 if e <= 512 else 4e-6 * (e / 512) ** 0.5


def eligible_mask(rows, n, ql, xl, self_exclude, select):
    """[b, n] bool: the columns query `rows[i]` may return."""
    ok = ~RR._excluded(np.asarray(rows), n, self_exclude)
    if select:
        same = np.asarray(xl)[None, :] == np.asarray(ql)[np.asarray(rows)][:, None]
        ok &= same if select == 1 else ~same
    return ok


def knn_exact(d2, k, ql=None, xl=None, self_exclude=False, select=0, rows=None):
    """d2 [b, n] (any float dtype; NaN counts as +inf) of the queries `rows` (default: row i is query i)
    -> (idx int32 [b, k], d2 [b, k] in d2's dtype, found int32 [b])."""
    d2 = np.array(d2, copy=True)
    d2[np.isnan(d2)] = np.inf
    b, n = d2.shape
    rows = np.arange(b) if rows is None else np.asarray(rows)
    ok = eligible_mask(rows, n, ql, xl, self_exclude, select)
    idx = np.full((b, k), -1, np.int32)
    val = np.full((b, k), np.inf, d2.dtype)
    found = np.minimum(ok.sum(1), k).astype(np.int32)
    cols = np.arange(n)
    for r in range(b):
        order = np.lexsort((cols, d2[r], ~ok[r]))          # eligible first, then by d2, then by index
        f = found[r]
        idx[r, :f] = order[:f]
        val[r, :f] = d2[r, order[:f]]
    return idx, val, found


def knn_ref(q, x, k, ql=None, xl=None, self_exclude=False, select=0):
    """The contract on float64 distances -> (idx int32 [nq, k], d2 float64 [nq, k], found int32 [nq])."""
    nq = len(q)
    idx, val, found = np.empty((nq, k), np.int32), np.empty((nq, k), np.float64), np.empty(nq, np.int32)
    for rows, d2 in RR.sqdist_blocks(q, x):
        idx[rows], val[rows], found[rows] = knn_exact(d2, k, ql, xl, self_exclude, select, rows=rows)
    return idx, val, found


def check(q, x, k, got_idx, got_d2, got_found, ql=None, xl=None, self_exclude=False, select=0, a=None):
    """-> a list of what is wrong with the answer (empty: accepted).  Accepted iff
      (a) found is exact; the first found indices of a row are distinct, eligible and in range; the rest is index -1, d2 +inf;
      (b) the returned d2 is ascending, index-ascending on equal d2, and within B of the float64 value (+inf where that is
          +inf or NaN);
      (c) for every returned j and every eligible unreturned c: d2_64[c] + B_c >= d2_64[j] - B_j."""
    q64, x64 = np.asarray(q, np.float64), np.asarray(x, np.float64)
    got_idx, got_d2, got_found = np.asarray(got_idx), np.asarray(got_d2), np.asarray(got_found)
    nq, n = len(q64), len(x64)
    a = A(q64.shape[1]) if a is None else a
    qn, xn = (q64 * q64).sum(1), (x64 * x64).sum(1)
    bad = []
    if got_idx.shape != (nq, k) or got_d2.shape != (nq, k) or got_found.shape != (nq,):
        return [f"shapes {got_idx.shape} {got_d2.shape} {got_found.shape}"]
    for rows, d2 in RR.sqdist_blocks(q64, x64):
        d2 = np.where(np.isnan(d2), np.inf, d2)
        B = a * (qn[rows][:, None] + xn[None, :])
        B = np.where(np.isfinite(B), B, 0.0)
        ok = eligible_mask(rows, n, ql, xl, self_exclude, select)
        for i, r in enumerate(rows):
            f = int(min(ok[i].sum(), k))
            if got_found[r] != f:
                bad.append(f"row {r}: found {got_found[r]} != {f}")
                continue
            j, dj = got_idx[r, :f].astype(np.int64), got_d2[r, :f].astype(np.float64)
            if np.any(got_idx[r, f:] != -1) or np.any(got_d2[r, f:] != np.inf):
                bad.append(f"row {r}: padding behind found = {f}")
            if np.any(j < 0) or np.any(j >= n):
                bad.append(f"row {r}: index out of range")
                continue
            if len(np.unique(j)) != f:
                bad.append(f"row {r}: repeated index")
            if not np.all(ok[i, j]):
                bad.append(f"row {r}: ineligible column {j[~ok[i, j]].tolist()}")
            if np.any(np.isnan(dj)) or np.any(np.diff(dj) < 0) or np.any((np.diff(dj) == 0) & (np.diff(j) <= 0)):
                bad.append(f"row {r}: not ascending in (d2, index)")
            want = d2[i, j]
            fin = np.isfinite(want)
            if np.any(dj[~fin] != np.inf) or np.any(np.abs(dj[fin] - want[fin]) > B[i, j][fin]):
                bad.append(f"row {r}: d2 off by {np.max(np.abs(dj[fin] - want[fin]) / np.maximum(B[i, j][fin], 1e-300), initial=0.0):.3g} B")
            rest = ok[i].copy()
            rest[j] = False
            if f and rest.any():
                lo_rest, hi_ret = (d2[i] + B[i])[rest].min(), (want - B[i, j]).max()
                if lo_rest < hi_ret:
                    bad.append(f"row {r}: an unreturned column at {lo_rest:.9g} (upper end) lies below a returned one at {hi_ret:.9g} (lower end)")
    return bad


def keys_u64(d2_f32, cols):
    """The kernel's key: (bits of the fp32 d2) << 32 | column."""
    return (np.asarray(d2_f32, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(cols, np.uint64)


def integer_rows(n, e, seed):
    """[n, e] float32 with integer entries in [-3, 3]: every d2 is an exact fp32 integer."""
    return np.random.default_rng(seed).integers(-3, 4, size=(n, e)).astype(np.float32)


def unit_rows(n, e, seed):
    g = np.random.default_rng(seed).standard_normal((n, e))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def unbalanced_labels(n, seed, classes=7):
    """`classes` classes of very different sizes in random order; class 0 has exactly ONE member."""
    rng = np.random.default_rng(seed)
    w = np.arange(1, classes, dtype=np.float64) ** 2
    lab = 1 + rng.choice(classes - 1, size=n, p=w / w.sum())
    lab[rng.integers(n)] = 0
    return lab.astype(np.int32)
