"""Exact t-SNE on the device: the slice of scikit-learn's `sklearn.manifold.TSNE` that the reference's utils.py touches
(`TSNE().fit_transform(encodings)`, reference utils.py:39-40, :66-67) plus what a user would set.

Semantics are scikit-learn 1.7's with method='exact': joint probabilities from a per-row bisection on the perplexity, 250
iterations at `early_exaggeration` with momentum 0.5, then momentum 0.8 without exaggeration; the KL divergence and the
gradient norm are looked at every 50 iterations of the second phase (the first cannot stop: scikit-learn sets its patience
to the phase's length), which is the only host read — 8 bytes per 50 iterations.  All N^2 work (distances, affinities,
iterations, KL) is HIP kernels of libembnet_hip.so (csrc/tsne.hip, csrc/pairwise.hip); the PCA initialisation is an e x e
eigenproblem on the host.  Two deliberate differences from scikit-learn's default: the method is the exact one at every n
(scikit-learn defaults to the Barnes-Hut approximation), and the gradient norm tested against `min_grad_norm` is that of
the gradient itself (scikit-learn tests the gradient after it was scaled by the gains).  With max_iter = 250 there is no
second phase and `kl_divergence_` is the KL of the returned embedding (scikit-learn reports the exaggerated phase's error).
"""
import numpy as np
import torch

from . import ops

EXPLORATION_ITER = 250          # scikit-learn's _EXPLORATION_MAX_ITER
CHECK_EVERY = 50                # scikit-learn's _N_ITER_CHECK
MAX_N = 32768


def pca_init(x, scale=1e-4):
    """First two principal components of the rows of x (centred), float64 on the host, scaled so that column 0 has standard
    deviation `scale`.  Each component's sign makes its largest-magnitude loading positive (scikit-learn's svd_flip)."""
    x = np.asarray(x, dtype=np.float64)
    xc = x - x.mean(axis=0, keepdims=True)
    _, vecs = np.linalg.eigh(xc.T @ xc)
    if vecs.shape[1] < 2:
        vecs = np.concatenate([vecs, np.zeros_like(vecs)], axis=1)
    v = vecs[:, ::-1][:, :2].copy()
    for c in range(2):
        if v[np.argmax(np.abs(v[:, c])), c] < 0:
            v[:, c] = -v[:, c]
    y = (xc @ v).astype(np.float32)
    sd = np.std(y[:, 0])
    return (y / sd * scale).astype(np.float32) if sd > 0 else y


class TSNE:
    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, init='pca', random_state=None, device=None):
        if n_components != 2:
            raise ValueError(f"n_components={n_components!r} is not supported: the on-device exact method embeds into 2 dimensions")
        if not (isinstance(learning_rate, str) and learning_rate == 'auto') and not float(learning_rate) > 0:
            raise ValueError("The 'learning_rate' parameter of TSNE must be a str among {'auto'} or a float in the range "
                             f"(0.0, inf). Got {learning_rate!r} instead.")
        if not float(perplexity) > 0:
            raise ValueError(f"The 'perplexity' parameter of TSNE must be a float in the range (0.0, inf). Got {perplexity!r} instead.")
        if not float(early_exaggeration) >= 1:
            raise ValueError("The 'early_exaggeration' parameter of TSNE must be a float in the range [1.0, inf). "
                             f"Got {early_exaggeration!r} instead.")
        if int(max_iter) < EXPLORATION_ITER:
            raise ValueError(f"The 'max_iter' parameter of TSNE must be an int in the range [250, inf). Got {max_iter!r} instead.")
        if isinstance(init, str) and init not in ('pca', 'random'):
            raise ValueError(f"The 'init' parameter of TSNE must be a str among {{'pca', 'random'}} or an array. Got {init!r} instead.")
        self.n_components, self.perplexity, self.early_exaggeration = 2, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.max_iter = learning_rate, int(max_iter)
        self.n_iter_without_progress, self.min_grad_norm = int(n_iter_without_progress), float(min_grad_norm)
        self.init, self.random_state, self.device = init, random_state, device

    # ------------------------------------------------------------------ pieces (the tests drive them one by one)
    def _device(self):
        return torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())

    def _initial(self, x_host, n):
        if isinstance(self.init, str):
            if self.init == 'pca':
                return pca_init(x_host)
            rs = self.random_state if isinstance(self.random_state, np.random.RandomState) else np.random.RandomState(self.random_state)
            return (1e-4 * rs.standard_normal(size=(n, 2))).astype(np.float32)
        y = np.asarray(self.init.detach().cpu() if torch.is_tensor(self.init) else self.init, dtype=np.float32)
        if y.shape != (n, 2):
            raise ValueError(f"init must have shape ({n}, 2), got {y.shape}")
        return y.copy()

    def fit_transform(self, X, y=None):
        x = X.detach() if torch.is_tensor(X) else torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float32)))
        if x.dim() != 2:
            raise ValueError(f"Expected 2D array, got {x.dim()}D array instead")
        n = x.shape[0]
        if self.perplexity >= n:
            raise ValueError("perplexity must be less than n_samples")
        if n > MAX_N:
            raise ValueError(f"n_samples={n} > {MAX_N}: the exact method keeps a dense [n,n] float32 matrix on the device")
        dev = self._device()
        y0 = self._initial(x.cpu().numpy() if isinstance(self.init, str) and self.init == 'pca' else None, n)
        with torch.cuda.device(dev):
            x = x.to(dev, torch.float32)
            self.learning_rate_ = (max(n / self.early_exaggeration / 4.0, 50.0) if isinstance(self.learning_rate, str)
                                   else float(self.learning_rate))
            ws = ops.tsne_workspace(n, x)
            p, beta = ops.tsne_affinities(ops.pairwise_distances(x, squared=True), self.perplexity, inplace=True, ws=ws)
            self.beta_ = beta
            emb, kl, it = self._descend(p, torch.from_numpy(y0).to(dev), ws)
        self.embedding_ = emb.cpu().numpy()
        self.kl_divergence_, self.n_iter_ = kl, it
        return self.embedding_

    def _descend(self, p, y, ws):
        """scikit-learn's two _gradient_descent calls.  -> (Y, the last KL looked at, index of the last iteration run)."""
        update, gains = torch.zeros_like(y), torch.ones_like(y)
        lr = self.learning_rate_
        ops.tsne_iterate(p, y, update, gains, self.early_exaggeration, 0.5, lr, EXPLORATION_ITER, ws=ws)
        best, best_iter, kl, i = np.finfo(np.float64).max, EXPLORATION_ITER, float("nan"), EXPLORATION_ITER - 1
        done = EXPLORATION_ITER                 # iterations applied so far
        while done < self.max_iter:
            i = min((done // CHECK_EVERY + 1) * CHECK_EVERY, self.max_iter) - 1      # the next iteration that is looked at
            ops.tsne_iterate(p, y, update, gains, 1.0, 0.8, lr, i - done, ws=ws)
            out = ops.tsne_kl(p, y, ws=ws)                                           # at the Y iteration i starts from
            ops.tsne_iterate(p, y, update, gains, 1.0, 0.8, lr, 1, ws=ws)
            done = i + 1
            kl, grad_norm = (float(v) for v in out.cpu())
            if (i + 1) % CHECK_EVERY == 0:
                if kl < best:
                    best, best_iter = kl, i
                elif i - best_iter > self.n_iter_without_progress:
                    break
                if grad_norm <= self.min_grad_norm:
                    break
        if done == EXPLORATION_ITER:            # max_iter = 250: no second phase; report the KL of the embedding returned
            kl = float(ops.tsne_kl(p, y, ws=ws)[0])
        return y, kl, i

    def fit(self, X, y=None):
        self.fit_transform(X)
        return self
