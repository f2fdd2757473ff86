"""Lloyd's k-means on the device, for clustering encodings (clustering.clustering_metrics reports NMI from it).

Assignment is ops.kmeans_assign — the streaming fp32 MFMA distance GEMM of the retrieval metrics with an argmin epilogue, no
[n, k] matrix — and the centre update ops.kmeans_update, a fixed-order segmented sum (csrc/kmeans.hip).  Seeding is k-means++ by
plain D^2 sampling (ops.kmeans_pp_update / kmeans_pp_pick), one draw per centre from the library's counter-based generator, so a
seed names one clustering: two fits with the same arguments return the same bits.
"""
import numpy as np
import torch

from . import ops


class KMeans:
    """KMeans(n_clusters, init='k-means++' | ndarray[k, e], n_init=1, max_iter=300, tol=0.0, seed=0, device=None)

    fit / predict / fit_predict and scikit-learn's attribute names: cluster_centers_ [k, e] float32, labels_ [n] int32,
    inertia_ (the sum of squared distances to the assigned centres), n_iter_; and n_empty_, the clusters the last update found
    without a point.

    Lloyd alternates an assign pass and a centre update.  It stops when an assign pass changes no label, when the update moved
    the centres by shift = sum_j |c_j_new - c_j_old|^2 <= tol, or after max_iter assign passes.  `tol` is an ABSOLUTE threshold
    on that shift — not scikit-learn's tolerance, which scales with the variance of the data; tol=0 (the default) means "until no
    label changes".  n_iter_ counts the assign passes including the one that confirmed convergence, which is scikit-learn's count
    under strict convergence.  labels_ and inertia_ come from the last assign pass against cluster_centers_, so the three are
    consistent.  An empty cluster keeps its centre (scikit-learn relocates it): n_empty_ says when that happened.

    n_init > 1: run r is seeded with seed + r; the run with the smallest inertia is kept, ties going to the earlier run.  With
    an array init every run is the same, so n_init is taken as 1.  The fit reads four bytes per pass on the host (the number of
    changed labels), plus eight for the shift when tol > 0."""

    def __init__(self, n_clusters, init='k-means++', n_init=1, max_iter=300, tol=0.0, seed=0, device=None):
        if int(n_clusters) < 1:
            raise ValueError(f"KMeans: n_clusters must be >= 1 (got {n_clusters})")
        if isinstance(init, str) and init != 'k-means++':
            raise ValueError(f"KMeans: init must be 'k-means++' or an array [n_clusters, e] (got {init!r})")
        if int(n_init) < 1 or int(max_iter) < 1:
            raise ValueError("KMeans: n_init and max_iter must be >= 1")
        self.n_clusters, self.init, self.n_init = int(n_clusters), init, int(n_init)
        self.max_iter, self.tol, self.seed, self.device = int(max_iter), float(tol), int(seed), device

    # ---- inputs
    def _points(self, x):
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        device = self.device
        if device is None:
            if t.is_cuda:
                device = t.device
            else:
                from .backbones import default_device
                device = default_device()
        t = t.detach().to(device=device, dtype=torch.float32)
        if t.dim() != 2 or t.shape[0] == 0:
            raise ValueError(f"KMeans: points must be a non-empty [n, e] block (got {tuple(t.shape)})")
        return t.contiguous()

    def seed_rows(self, x, seed):
        """The k-means++ rows for `seed`: int32 [n_clusters] on the device (x: a float32 device block)."""
        rows = torch.empty(self.n_clusters, dtype=torch.int32, device=x.device)
        weights = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        mind2 = None
        for j in range(self.n_clusters):
            index, _ = ops.kmeans_pp_pick(weights if mind2 is None else mind2, seed, j)
            rows[j:j + 1] = index
            if j + 1 < self.n_clusters:
                mind2 = ops.kmeans_pp_update(x, index, mind2)
        return rows

    def _lloyd(self, x, centres, ws):
        prev, n_iter, n_empty = None, 0, None
        labels = inertia = None
        settled = False
        for it in range(1, self.max_iter + 1):
            labels, _, changed, inertia = ops.kmeans_assign(x, centres, prev, ws=ws, reuse_point_norms=it > 1)
            n_iter = it
            if prev is not None and int(changed.item()) == 0:
                settled = True
                break
            centres, _, shift, n_empty = ops.kmeans_update(x, labels, centres, ws=ws)
            prev = labels
            if self.tol > 0.0 and float(shift.item()) <= self.tol:
                break
        if not settled:                                     # the centres moved after the last assign pass
            labels, _, _, inertia = ops.kmeans_assign(x, centres, None, ws=ws, reuse_point_norms=True)
        return centres, labels, inertia, n_iter, n_empty

    def fit(self, x):
        x = self._points(x)
        n, e = x.shape
        k = self.n_clusters
        if k > n:
            raise ValueError(f"KMeans: n_clusters = {k} exceeds the number of points {n}")
        given = None
        if not isinstance(self.init, str):
            given = self._points(self.init)
            if tuple(given.shape) != (k, e):
                raise ValueError(f"KMeans: init must be [{k}, {e}] (got {tuple(given.shape)})")
        ws = ops.kmeans_workspace(n, k, e, x)
        best = None
        for r in range(1 if given is not None else self.n_init):
            if given is not None:
                centres, rows = given.clone(), None
            else:
                rows = self.seed_rows(x, self.seed + r)
                centres = x.index_select(0, rows.long()).contiguous()
            centres, labels, inertia, n_iter, n_empty = self._lloyd(x, centres, ws)
            if best is None or bool((inertia < best[2]).item()):
                best = (centres, labels, inertia, n_iter, n_empty, rows)
        centres, labels, inertia, n_iter, n_empty, rows = best
        self.cluster_centers_ = centres.cpu().numpy()
        self.labels_ = labels.cpu().numpy()
        self.inertia_ = float(inertia.item())
        self.n_iter_ = int(n_iter)
        self.n_empty_ = 0 if n_empty is None else int(n_empty.item())
        self.init_rows_ = None if rows is None else rows.cpu().numpy()
        self._centres = centres
        return self

    def predict(self, x):
        if not hasattr(self, '_centres'):
            raise ValueError("KMeans.predict: fit first")
        x = self._points(x).to(self._centres.device)
        if x.shape[1] != self._centres.shape[1]:
            raise ValueError(f"KMeans.predict: points have e = {x.shape[1]}, the centres {self._centres.shape[1]}")
        if x.shape[0] < self.n_clusters:                    # the assign pass wants k <= n: repeat the block's first row behind it
            pad = x[:1].expand(self.n_clusters - x.shape[0], -1)
            return ops.kmeans_assign(torch.cat([x, pad]).contiguous(), self._centres)[0][:x.shape[0]].cpu().numpy()
        return ops.kmeans_assign(x, self._centres)[0].cpu().numpy()

    def fit_predict(self, x):
        return self.fit(x).labels_
