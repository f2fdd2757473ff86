"""NumPy restatement of scikit-learn's exact t-SNE (TSNE(method='exact', n_components=2)): the specification the HIP kernels
of csrc/tsne.hip are tested against, next to the recorded scikit-learn results in tests/golden/tsne.npz.

float64 by default.  `dtype=np.float32` runs the descent state and arithmetic in float32 (the storage format of the device
path).  The sign test of the gains is done on signs, not on the product update * grad (see include/embnet.h).
"""
import numpy as np

EPS = 2.220446049250313e-16          # scikit-learn's MACHINE_EPSILON
TOL = 1e-5                           # _binary_search_perplexity: PERPLEXITY_TOLERANCE
N_STEPS = 100


def squared_distances(x):
    """float64 difference-form squared distances of the rows of x, rounded to float32 (what scikit-learn's affinities read)."""
    x = np.asarray(x, np.float64)
    g = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(g, 0.0)
    return g.astype(np.float32)


def _row_entropy(d, beta):
    p = np.exp(-d * beta)
    s = p.sum()
    if s == 0.0:
        s = 1e-8
    p = p / s
    return np.log(s) + beta * (d * p).sum(), p


def conditional_probabilities(d2, perplexity, extra=0):
    """Rows of p_j|i and beta_i: _binary_search_perplexity.  extra = -1 / +1 returns the row one bisection step before /
    after the step the stop rule accepts (the slack two correct implementations may differ by)."""
    d2 = np.asarray(d2, np.float64)
    n = d2.shape[0]
    want = np.log(perplexity)
    pc, betas = np.zeros((n, n)), np.zeros(n)
    for i in range(n):
        d = np.delete(d2[i], i)
        beta, lo, hi = 1.0, -np.inf, np.inf
        trail = []
        for _ in range(N_STEPS):
            h, p = _row_entropy(d, beta)
            trail.append((beta, p))
            diff = h - want
            if abs(diff) <= TOL and extra <= 0:
                break
            if diff > 0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
            if abs(diff) <= TOL:                                             # extra = +1: evaluate the next beta and stop
                h, p = _row_entropy(d, beta)
                trail.append((beta, p))
                break
        b, p = trail[-2] if (extra < 0 and len(trail) > 1) else trail[-1]
        betas[i] = b
        pc[i] = np.insert(p, i, 0.0)
    return pc, betas


def joint_probabilities(d2, perplexity, extra=0):
    """-> (P [n,n] float64: symmetric, sum 1, >= EPS off the diagonal, 0 on it; beta [n]): _joint_probabilities."""
    pc, betas = conditional_probabilities(d2, perplexity, extra)
    p = pc + pc.T
    p = np.maximum(p / max(p.sum(), EPS), EPS)
    np.fill_diagonal(p, 0.0)
    return p, betas


def perplexity_of(d2_row_without_self, beta):
    """exp(entropy) of one conditional row at beta, float64."""
    d = np.asarray(d2_row_without_self, np.float64)
    d = d - d.min()
    h, _ = _row_entropy(d, float(beta))
    return float(np.exp(h))


def kl_and_grad(p, y, alpha=1.0, dtype=np.float64):
    """-> kl, grad [n,2], kl_abs, grad_abs [n,2], z: _kl_divergence at Y with alpha * P in the gradient.  kl_abs and grad_abs
    are the float64 sums of the absolute values of the terms of kl and of each gradient component."""
    p = np.asarray(p, dtype)
    y = np.asarray(y, dtype)
    diff = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (diff ** 2).sum(-1))
    np.fill_diagonal(w, 0.0)
    z = w.sum(dtype=np.float64).astype(dtype) if dtype != np.float64 else w.sum()
    q = w / z
    off = ~np.eye(len(y), dtype=bool)
    terms = np.zeros_like(p)
    terms[off] = p[off] * np.log(np.maximum(p[off], EPS) / np.maximum(q[off], EPS))
    coef = ((dtype(alpha) * p - q) * w)[:, :, None] * diff
    grad = 4.0 * coef.sum(1)
    return (float(terms.sum()), grad.astype(dtype), float(np.abs(terms).astype(np.float64).sum()),
            4.0 * np.abs(coef).astype(np.float64).sum(1), float(z))


def update(y, upd, gains, grad, momentum, lr):
    """One _gradient_descent update, in place; arithmetic in the arrays' dtype."""
    inc = ((upd < 0) & (grad > 0)) | ((upd > 0) & (grad < 0))
    gains[inc] += 0.2
    gains[~inc] *= 0.8
    np.maximum(gains, 0.01, out=gains)
    upd[:] = momentum * upd - lr * (gains * grad)
    y += upd


def iterate(p, y, upd, gains, alpha, momentum, lr, n_iter, dtype=np.float64, track=None):
    """n_iter iterations in place.  track (a list) receives per step (grad, grad_abs, gains after the step)."""
    t = dtype
    for _ in range(n_iter):
        _, g, _, gabs, _ = kl_and_grad(p, y, alpha, dtype)
        update(y, upd, gains, g, t(momentum), t(lr))
        if track is not None:
            track.append((g.copy(), gabs, gains.copy()))


def pca_init(x):
    x = np.asarray(x, np.float64)
    xc = x - x.mean(0)
    _, _, vt = np.linalg.svd(xc, full_matrices=False)
    vt = vt[:2]
    for c in range(2):
        if vt[c, np.argmax(np.abs(vt[c]))] < 0:
            vt[c] = -vt[c]
    y = (xc @ vt.T).astype(np.float32)
    return (y / np.std(y[:, 0]) * 1e-4).astype(np.float32)


def fit(x, perplexity=30.0, early_exaggeration=12.0, max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7,
        y0=None, dtype=np.float64):
    """The full schedule of TSNE(method='exact', init='pca', learning_rate='auto') -> (Y, kl_divergence, n_iter)."""
    n = len(x)
    p, _ = joint_probabilities(squared_distances(x), perplexity)
    p = p.astype(dtype)
    lr = max(n / early_exaggeration / 4.0, 50.0)
    y = np.array(pca_init(x) if y0 is None else y0, dtype)
    upd, gains = np.zeros_like(y), np.ones_like(y)
    iterate(p, y, upd, gains, early_exaggeration, 0.5, lr, 250, dtype)
    best, best_iter, kl, i = np.finfo(np.float64).max, 250, np.nan, 249
    for i in range(250, max_iter):
        check = (i + 1) % 50 == 0
        k, g, _, _, _ = kl_and_grad(p, y, 1.0, dtype)
        update(y, upd, gains, g, dtype(0.8), dtype(lr))
        if check or i == max_iter - 1:
            kl = k
        if check:
            if k < best:
                best, best_iter = k, i
            elif i - best_iter > n_iter_without_progress:
                break
            if np.linalg.norm(g) <= min_grad_norm:
                break
    return y.astype(np.float32), float(kl), i


def trustworthiness(x, y, n_neighbors=5):
    """Venna & Kaski's trustworthiness of the embedding y of x (the quantity of sklearn.manifold.trustworthiness)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = len(x)
    dx = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    dy = ((y[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(dx, np.inf)
    np.fill_diagonal(dy, np.inf)
    rank_x = np.argsort(np.argsort(dx, axis=1, kind="stable"), axis=1, kind="stable")    # 0 = nearest
    near_y = np.argsort(dy, axis=1, kind="stable")[:, :n_neighbors]
    r = np.take_along_axis(rank_x, near_y, axis=1) + 1 - n_neighbors
    t = np.sum(r[r > 0])
    return float(1.0 - t * (2.0 / (n * n_neighbors * (2.0 * n - 3.0 * n_neighbors - 1.0))))
