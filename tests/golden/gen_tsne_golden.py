"""Writes tests/golden/tsne.npz: scikit-learn's exact t-SNE on small seeded inputs, for tests/test_tsne_cpu.py and
tests/test_tsne_gpu.py (which read only that file and tests/tsne_ref.py; scikit-learn is needed here alone).

    python tests/golden/gen_tsne_golden.py            (CPU, a few minutes; scikit-learn 1.7)

Per input k: x{k} (unit-norm clustered rows whose classes overlap: scikit-learn's final KL must be >= 0.25, checked below),
scikit-learn's joint probabilities p{k} (condensed, float32), the slack of the bisection's stop rule p_slack{k}, a fixed
yfix{k} with _kl_divergence's value and gradient there, the end of a full TSNE(method='exact', init='pca', random_state=0)
run, and the three end-of-run figures (KL, n_iter, trustworthiness) of scikit-learn with random_state=7 and of tsne_ref.fit
in float64 and float32.  Two descent cases: a one-step case on a far-spread Y whose gradient components are below 4e-9
with update = +-2e-38 (the fp32 product update * grad is 0: only a test on the signs takes the right gains branch), and a
ten-step case near scikit-learn's final embedding.  Both are checked here to have every |grad| component above twice its
fp32 error bound at every step, so the branch is defined.
"""
import os
import sys
import time

import numpy as np
from scipy.spatial.distance import squareform
from sklearn.manifold import TSNE, trustworthiness
from sklearn.manifold._t_sne import _joint_probabilities, _kl_divergence

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsne_ref as R  # noqa: E402

INPUTS = [(12, 25, 32, 1.6, 11), (20, 20, 64, 1.8, 12)]        # classes, per class, e, spread, seed
PERPLEXITY = 30.0
U = 2.0 ** -24


def clustered(classes, per, e, spread, seed):
    rs = np.random.RandomState(seed)
    c = rs.randn(classes, e)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = np.repeat(c, per, axis=0) + spread * rs.randn(classes * per, e) / np.sqrt(e)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def figures(x, y, kl, n_iter):
    return np.array([kl, n_iter, trustworthiness(x, y, n_neighbors=5)], np.float64)


def branch_defined(p, y, upd, gains, lr, steps):
    """every |grad| component above twice 16 * 2^-24 * (sum of |terms|) at each of `steps` float64 steps"""
    y, upd, gains = y.astype(np.float64), upd.astype(np.float64), gains.astype(np.float64)
    track = []
    R.iterate(p, y, upd, gains, 1.0, 0.8, lr, steps, track=track)
    return all(np.all(np.abs(g) > 2 * 16 * U * gabs) for g, gabs, _ in track), track


def main():
    out = {"perplexity": np.float64(PERPLEXITY), "n_inputs": np.int64(len(INPUTS))}
    for k, spec in enumerate(INPUTS):
        x = clustered(*spec)
        n = len(x)
        d2 = R.squared_distances(x)
        p = _joint_probabilities(d2, PERPLEXITY, 0)
        p32 = p.astype(np.float32)
        pd = squareform(p32.astype(np.float64))
        ref_p, _ = R.joint_probabilities(d2, PERPLEXITY)
        off = ~np.eye(n, dtype=bool)
        ref_err = np.abs(ref_p - squareform(p))[off].max()
        slack = max(np.abs(R.joint_probabilities(d2, PERPLEXITY, extra)[0] - squareform(p))[off].max() for extra in (-1, 1))
        print(f"input {k}: n={n} max P {p.max():.3e} restatement {ref_err:.2e} one step early/late {slack:.2e}", flush=True)
        rs = np.random.RandomState(100 + k)
        yfix = (2.0 * rs.randn(n, 2)).astype(np.float32)
        kl_fix, grad_fix = _kl_divergence(yfix.astype(np.float64).ravel(), squareform(pd, checks=False), 1.0, n, 2)

        runs = {}
        for seed in (0, 7):
            t = TSNE(method='exact', init='pca', random_state=seed, perplexity=PERPLEXITY)
            emb = t.fit_transform(x)
            runs[seed] = (emb, figures(x, emb, t.kl_divergence_, t.n_iter_))
            print(f"  sklearn seed {seed}: kl {t.kl_divergence_:.4f} n_iter {t.n_iter_} trust {runs[seed][1][2]:.4f}", flush=True)
        assert runs[0][1][0] >= 0.25, "end-to-end inputs must overlap: scikit-learn's final KL >= 0.25"
        ref = {}
        for name, dt in (("f64", np.float64), ("f32", np.float32)):
            y, kl, it = R.fit(x, PERPLEXITY, dtype=dt)
            ref[name] = figures(x, y, kl, it)
            print(f"  tsne_ref {name}: kl {kl:.4f} n_iter {it} trust {ref[name][2]:.4f}", flush=True)

        emb = runs[0][0]
        lr = max(n / 12.0 / 4.0, 50.0)
        # one step, far-spread Y: scale scikit-learn's embedding until every gradient component is below 4e-9
        scale = 1.0
        while np.abs(R.kl_and_grad(pd, (emb * np.float32(scale)).astype(np.float32), 1.0)[1]).max() >= 4e-9:
            scale *= 10.0
        y_far = (emb * np.float32(scale)).astype(np.float32)
        u_far = (np.where(rs.rand(n, 2) < 0.5, -1.0, 1.0) * 2e-38).astype(np.float32)
        ok, track = branch_defined(pd, y_far, u_far, np.ones((n, 2)), lr, 1)
        g_far = track[0][0]
        assert ok and np.abs(g_far).min() > 1.2e-38 and (np.abs(g_far) * 2e-38).max() < 1e-46, (scale, np.abs(g_far).max())
        print(f"  far case: scale {scale:g}, |g| in [{np.abs(g_far).min():.2e}, {np.abs(g_far).max():.2e}]", flush=True)
        # ten steps near scikit-learn's final embedding
        for attempt in range(50):
            rs2 = np.random.RandomState(1000 * k + attempt)
            y_near = (emb + 0.05 * emb.std() * rs2.randn(n, 2)).astype(np.float32)
            u_near = (0.01 * rs2.randn(n, 2)).astype(np.float32)
            ok, _ = branch_defined(pd, y_near, u_near, np.ones((n, 2)), lr, 10)
            if ok:
                break
        assert ok, "no ten-step case with a defined branch found"
        print(f"  near case: attempt {attempt}", flush=True)
        out.update({f"x{k}": x, f"p{k}": p32, f"p_ref_err{k}": np.float64(ref_err), f"p_slack{k}": np.float64(slack),
                    f"yfix{k}": yfix, f"kl_fix{k}": np.float64(kl_fix), f"grad_fix{k}": grad_fix.reshape(n, 2),
                    f"emb{k}": emb.astype(np.float32), f"sk0_{k}": runs[0][1], f"sk7_{k}": runs[7][1],
                    f"ref64_{k}": ref["f64"], f"ref32_{k}": ref["f32"], f"lr{k}": np.float64(lr),
                    f"y_far{k}": y_far, f"u_far{k}": u_far, f"y_near{k}": y_near, f"u_near{k}": u_near})

    # host times of scikit-learn at the reference's size (107 classes x 10 samples), e = 256: reported in DESIGN.md, not tested
    x = clustered(107, 10, 256, 0.9, 5)
    for method in ("exact", "barnes_hut"):
        t0 = time.perf_counter()
        t = TSNE(method=method, init='pca', random_state=0).fit(x)
        out[f"host_seconds_{method}_1070"] = np.float64(time.perf_counter() - t0)
        out[f"host_kl_{method}_1070"] = np.float64(t.kl_divergence_)
        print(f"scikit-learn {method} n=1070: {out[f'host_seconds_{method}_1070']:.1f} s, kl {t.kl_divergence_:.4f}", flush=True)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tsne.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
