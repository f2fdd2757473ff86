"""Float64 restatement of the k-means kernels (csrc/kmeans.hip) and of the clustering scores, NumPy only, with the rules by
which a device result is accepted.  tests/golden/gen_kmeans_golden.py, tests/test_kmeans_ref_cpu.py and
tests/test_kmeans_gpu.py all read this file; nothing here imports the package under test.

DISTANCE BOUND.  The assign pass is the retrieval walk: d2 = max(|x|^2 + |c|^2 - 2 x.c, 0) with x.c from the k-ordered fp32 fma
chain of the MFMA and the norms from a lane-strided fp32 fma chain.  The project's bound for that engine and epilogue is
tests/test_eval_path_gpu.py::_A:  |d2_gpu[i, j] - d64[i, j]| <= B[i, j] = A(e) (|x_i|^2 + |c_j|^2), A = 2e-6 up to e = 512 and
4e-6 sqrt(e / 512) beyond.  A label a_i is ACCEPTED iff d64[i, a_i] - B[i, a_i] <= min_j (d64[i, j] + B[i, j]): some
perturbation of the distances within the bound makes a_i the argmin.  A point is UNAMBIGUOUS iff its two smallest d64 differ by
more than the sum of their bounds; there the accepted label is unique and is the float64 argmin.

UPDATE BOUND, from the kernel's summation order.  Element (j, col) of the new centre is the sum of the m = count[j] values
x[i, col] (exact fp32 inputs) accumulated in f64: four interleaved chains per chunk of 512 rows, folded, the chunks added in
order — m + m / 512 + 3 additions at most, each rounding by 2^-53 of a partial sum that is at most S = sum |x[i, col]|.  So
|sum_gpu - sum| <= (m + m / 512 + 4) 2^-53 S.  The f64 division adds 2^-53 and the one rounding to fp32 2^-24 of the
result (2^-149 below the normal range).  update64's own NumPy sum is within m 2^-53 S as well.  Hence, with the mean absolute
value M = S / m,
    |c_gpu[j, col] - c64[j, col]| <= 2^-24 |c64[j, col]| + 2^-149 + (2 m + 8) 2^-53 M = U[j, col].
The shift sum_j |new - old|^2 is computed in f64 from the fp32 centres: each term moves by at most 2 |t| U + U^2 with
t = c64_new - old, and the fixed-order f64 sum of k e terms adds k e 2^-53 shift.
"""
import numpy as np

def A(e):
    """tests/test_eval_path_gpu.py::_A."""
    return 2e-6 if e <= 512 else 4e-6 * (e / 512) ** 0.5


# ---------------------------------------------------------------------------------------------------------------- inputs
def blobs(n, e, k, noise, seed):
    """Unit-norm blobs: k centres N(0, I), n points = a centre plus N(0, noise^2 / e I), normalised.  Point i belongs to blob
    i mod k.  -> (x float32 [n, e], blob ids int64 [n])."""
    rs = np.random.RandomState(seed)
    centres = rs.randn(k, e)
    ids = np.arange(n) % k
    x = centres[ids] + noise * rs.randn(n, e)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x.astype(np.float32)), ids


def case_c():
    """Shape C: n = 6100, e = 20, k = 1000 — the 128x128 geometry, ragged on both sides.  Centres: rows of x."""
    x, _ = blobs(6100, 20, 1000, 0.5, 31)
    rows = np.random.RandomState(32).choice(6100, 1000, replace=False)
    return x, np.ascontiguousarray(x[rows])


def skewed_labels(n, k, seed=5):
    """One cluster (id 3) holds 90 % of the points, clusters 500 .. 999 one point each, the rest is spread over the others
    (some of which stay empty)."""
    rs = np.random.RandomState(seed)
    labels = np.full(n, 3, np.int32)
    order = rs.permutation(n)
    singles = order[:500]
    labels[singles] = 500 + np.arange(500)
    rest = order[500:500 + (n - int(0.9 * n) - 500)]
    labels[rest] = rs.randint(0, 400, rest.shape[0])
    return labels


# ---------------------------------------------------------------------------------------------------------------- Lloyd
def d64(x, c):
    """Squared Euclidean distances in float64, [n, k], from the differences (no cancellation); NaN counts as +inf."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    out = np.empty((x.shape[0], c.shape[0]))
    for j0 in range(0, c.shape[0], 64):
        with np.errstate(invalid="ignore", over="ignore"):
            d = x[:, None, :] - c[None, j0:j0 + 64, :]
            out[:, j0:j0 + 64] = np.einsum("nke,nke->nk", d, d)
    out[np.isnan(out)] = np.inf
    return out


def bound(x, c):
    """B[i, j] = A(e) (|x_i|^2 + |c_j|^2); a NaN / inf centre has an infinite bound (its distance is +inf anyway)."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        b = A(x.shape[1]) * ((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :])
    b[np.isnan(b)] = np.inf
    return b


def assign64(x, c, d=None):
    """-> (labels int32 [n]: the argmin, ties to the smaller index, label 0 without a finite distance; d2 float64 [n])."""
    d = d64(x, c) if d is None else d
    labels = np.argmin(d, axis=1).astype(np.int32)
    return labels, d[np.arange(d.shape[0]), labels]


def ambiguous(d, b):
    """bool [n]: the two smallest distances of the point are closer than the sum of their bounds (k = 1: never)."""
    if d.shape[1] == 1:
        return np.zeros(d.shape[0], bool)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    rows = np.arange(d.shape[0])
    d0, d1 = d[rows, order[:, 0]], d[rows, order[:, 1]]
    with np.errstate(invalid="ignore"):
        gap = d1 - d0
    gap[np.isnan(gap)] = 0.0                                 # inf - inf: no finite distance at all
    both = b[rows, order[:, 0]] + b[rows, order[:, 1]]
    return ~(gap > both) & np.isfinite(d0)


def labels_acceptable(d, b, labels):
    """bool [n]: the acceptance rule of the module docstring.  A point without a finite distance accepts label 0 only."""
    rows = np.arange(d.shape[0])
    with np.errstate(invalid="ignore"):
        lo = d[rows, labels] - b[rows, labels]
        hi = np.min(d + b, axis=1)
    none = ~np.isfinite(d).any(axis=1)
    ok = lo <= hi
    ok[none] = labels[none] == 0
    return ok


def update64(x, labels, centres):
    """-> (centres float64 [k, e]: the mean of each cluster, an empty cluster keeps its row of `centres`; counts int64 [k];
    U [k, e]: the per-element bound of the module docstring)."""
    x = np.asarray(x, np.float64)
    k = centres.shape[0]
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    sums = np.zeros((k, x.shape[1]))
    sabs = np.zeros((k, x.shape[1]))
    np.add.at(sums, labels, x)
    np.add.at(sabs, labels, np.abs(x))
    out = np.asarray(centres, np.float64).copy()
    live = counts > 0
    out[live] = sums[live] / counts[live, None]
    m = np.maximum(counts, 1)[:, None].astype(np.float64)
    u = 2.0 ** -24 * np.abs(out) + 2.0 ** -149 + (2.0 * m + 8.0) * 2.0 ** -53 * (sabs / m)
    u[~live] = 0.0
    return out, counts, u


def shift64(new, old, counts, u):
    """-> (shift, its bound) over the non-empty clusters."""
    t = (np.asarray(new, np.float64) - np.asarray(old, np.float64))[counts > 0]
    uu = u[counts > 0]
    shift = float((t * t).sum())
    return shift, float((2.0 * np.abs(t) * uu + uu * uu).sum() + t.size * 2.0 ** -53 * shift)


def lloyd64(x, init, max_iter=300, check=False):
    """Lloyd from `init` in float64 with the estimator's stopping rule (tol = 0): stop when an assign pass changes no label.
    -> dict(labels, centres, inertia, n_iter, n_empty_max, ambiguous_max: the largest share of ambiguous points of any pass at
    1.25 B: the device's centres are the fp32 roundings of its own means, within 2^-24 |c| of these, which moves a distance of
    unit-norm data by at most 2 |x - c| 2^-24 |c| < B / 4)."""
    x64 = np.asarray(x, np.float64)
    c = np.asarray(init, np.float64).copy()
    prev, n_iter, n_empty_max, amb_max = None, 0, 0, 0.0
    for it in range(1, max_iter + 1):
        d = d64(x64, c)
        labels, d2 = assign64(x64, c, d)
        n_iter = it
        if check:
            amb_max = max(amb_max, float(ambiguous(d, 1.25 * bound(x64, c)).mean()))
        if prev is not None and np.array_equal(prev, labels):
            break
        c, counts, _ = update64(x64, labels, c)
        n_empty_max = max(n_empty_max, int((counts == 0).sum()))
        prev = labels
    return dict(labels=labels, centres=c, inertia=float(d2.sum()), n_iter=n_iter, n_empty_max=n_empty_max,
                ambiguous_max=amb_max)


# ---------------------------------------------------------------------------------------------------------------- seeding
K_A = np.uint64(0xD6E8FEB86659FD93)


def mix64(z):
    """csrc/common.h mix64 (as tests/augment_ref.py::mix64)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def rng_u32(seed, a, b):
    with np.errstate(over="ignore"):
        key = mix64(np.uint64(seed) ^ (np.uint64(a) * K_A))
        return int(mix64(key + np.uint64(b)) >> np.uint64(32))


def first_row(seed, n):
    return rng_u32(seed, 0, 0) % n


def draw_u(seed, j):
    """u_j = (((rng(seed, j, 0) << 32) | rng(seed, j, 1)) >> 11) * 2^-53, exactly representable."""
    bits = (rng_u32(seed, j, 0) << 32) | rng_u32(seed, j, 1)
    return float(bits >> 11) * 2.0 ** -53


def pick64(w, u):
    """The first index whose inclusive float64 prefix sum of w exceeds u * total; total == 0: floor(u n).
    -> (index, margin): margin = the distance of u * total to the nearer end of the chosen interval, over total."""
    w = np.asarray(w, np.float64)
    w = np.where(np.isfinite(w) & (w > 0), w, 0.0)
    p = np.cumsum(w)
    total = p[-1]
    if total == 0.0:
        return int(u * w.shape[0]), 1.0
    t = u * total
    i = int(np.searchsorted(p, t, side="right"))
    i = min(i, w.shape[0] - 1)
    lo = p[i - 1] if i > 0 else 0.0
    return i, float(min(t - lo, p[i] - t) / total)


def pick_acceptable(w, u, index):
    """The interval rule: `index` has positive weight and u * total lies in its interval of the float64 prefix sums, widened
    by n 2^-53 total (what a reordered f64 summation can move a prefix by); total == 0: exactly floor(u n)."""
    w = np.asarray(w, np.float64)
    w = np.where(np.isfinite(w) & (w > 0), w, 0.0)
    p = np.cumsum(w)
    total = p[-1]
    if total == 0.0:
        return index == int(u * w.shape[0])
    if not (0 <= index < w.shape[0]) or w[index] <= 0.0:
        return False
    tol = w.shape[0] * 2.0 ** -53 * total
    lo = p[index - 1] if index > 0 else 0.0
    return lo - tol <= u * total <= p[index] + tol


def pp64(x, k, seed):
    """k-means++ by plain D^2 sampling with the keyed draws.  -> (rows int64 [k], margin): margin = the smallest relative
    distance of any u * total to a prefix-sum boundary, minus the relative weight the device's fp32 distances may move across
    that boundary (sum_i A(e) (|x_i|^2 + |x_c|^2) over total).  The device picks the same rows when margin > n 2^-53."""
    x64 = np.asarray(x, np.float64)
    n, e = x64.shape
    norms = (x64 * x64).sum(1)
    rows = [first_row(seed, n)]
    mind2, slack, margin = None, np.zeros(n), np.inf
    for j in range(1, k):
        c = rows[-1]
        d = ((x64 - x64[c]) ** 2).sum(1)
        b = A(e) * (norms + norms[c])
        b[c] = 0.0                                           # the row itself: an exact zero on the device too
        if mind2 is None:
            mind2, slack = d, b
        else:
            slack = np.where(d < mind2, b, slack)
            mind2 = np.minimum(mind2, d)
        i, m = pick64(mind2, draw_u(seed, j))
        margin = min(margin, m - float(slack.sum() / mind2.sum()))
        rows.append(i)
    return np.asarray(rows, np.int64), margin


# ---------------------------------------------------------------------------------------------------------------- scores
def _table(a, b):
    ua, ia = np.unique(np.asarray([repr(v) for v in a]), return_inverse=True)
    ub, ib = np.unique(np.asarray([repr(v) for v in b]), return_inverse=True)
    t = np.zeros((ua.shape[0], ub.shape[0]), np.int64)
    np.add.at(t, (ia, ib), 1)
    return t


def _h(counts):
    p = counts[counts > 0] / counts.sum()
    return float(-(p * np.log(p)).sum())


def _mi(t):
    n = t.sum()
    pij = t / n
    outer = np.outer(t.sum(1), t.sum(0)) / (n * n)
    nz = t > 0
    return float(max((pij[nz] * np.log(pij[nz] / outer[nz])).sum(), 0.0))


def nmi64(labels_true, labels_pred):
    """normalized_mutual_info_score, arithmetic mean of the entropies."""
    t = _table(labels_true, labels_pred)
    if t.shape[0] == 1 and t.shape[1] == 1:
        return 1.0
    mi = _mi(t)
    if mi < np.finfo(np.float64).eps:
        return 0.0
    return mi / (0.5 * (_h(t.sum(1)) + _h(t.sum(0))))


def hc64(labels_true, labels_pred):
    """(homogeneity, completeness)."""
    t = _table(labels_true, labels_pred)
    mi, ht, hp = _mi(t), _h(t.sum(1)), _h(t.sum(0))
    return (mi / ht if ht else 1.0), (mi / hp if hp else 1.0)
