"""Exact t-SNE on the device (csrc/tsne.hip, embeddingnet_amd/tsne.py) against scikit-learn's recorded results
(tests/golden/tsne.npz, written by tests/golden/gen_tsne_golden.py) and the float64 restatement tests/tsne_ref.py.

Tolerances are derived, not tuned:
  * affinities: both sides bisect to |dH| <= 1e-5 and may stop one step apart; the fixture records how far the restatement's P
    moves when it stops one step early / late, and the device gets twice that;
  * gradient / KL at a fixed Y: 16 * 2^-24 times the float64 sum of the absolute values of the terms of each sum (a term is a
    handful of fp32 operations, the accumulation is wide);
  * descent steps: gains within 1e-6 relative (a wrong branch is 20 % off); update and Y within lr * gains * (gradient bound)
    per step plus the spacings of the fp32 arrays they are stored in (_descent_case spells the two comparisons out);
  * end to end: the KL gap to scikit-learn within twice the largest gap among the restatement (float64, float32) and
    scikit-learn with another seed, all read from the fixture.
Every test prints the figure it measured before asserting."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
INPUTS = [0, 1]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne.npz"))


def _square(cond, n):
    p = np.zeros((n, n))
    p[np.triu_indices(n, 1)] = cond
    return p + p.T


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _golden_p(g, k):
    n = len(g[f"x{k}"])
    p64 = _square(g[f"p{k}"].astype(np.float64), n)
    return p64, _dev(p64)


@pytest.mark.parametrize("k", INPUTS)
def test_affinities_vs_sklearn(g, k):
    from embeddingnet_amd import ops
    x = g[f"x{k}"]
    n, perp = len(x), float(g["perplexity"])
    d2 = R.squared_distances(x)
    p, beta = ops.tsne_affinities(_dev(d2), perp)
    want, _ = _golden_p(g, k)
    got = p.cpu().numpy().astype(np.float64)
    err, tol = np.abs(got - want).max(), 2.0 * float(g[f"p_slack{k}"])
    print(f"input {k}: max |P - sklearn P| {err:.3e} (allowed {tol:.3e}, max P {want.max():.3e}); sum P - 1 = {got.sum() - 1:.2e}")
    assert err <= tol
    assert abs(got.sum() - 1.0) <= 1e-5
    assert torch.equal(p, p.t().contiguous())
    assert torch.all(torch.diagonal(p) == 0)
    off = ~np.eye(n, dtype=bool)
    assert got[off].min() >= 2.220446e-16
    b = beta.cpu().numpy()
    d64 = d2.astype(np.float64)
    rel = max(abs(R.perplexity_of(np.delete(d64[i], i), b[i]) / perp - 1.0) for i in range(n))
    print(f"input {k}: perplexity recomputed from beta: worst relative error {rel:.2e}; sigma in "
          f"[{np.sqrt(0.5 / b.max()):.3f}, {np.sqrt(0.5 / b.min()):.3f}]")
    assert rel <= 1e-4
    d2_dev = _dev(d2)
    p2, beta2 = ops.tsne_affinities(d2_dev, perp, inplace=True)
    assert p2.data_ptr() == d2_dev.data_ptr() and torch.equal(p2, p) and torch.equal(beta2, beta)


@pytest.mark.parametrize("k", INPUTS)
def test_gradient_and_kl_at_fixed_y_vs_sklearn(g, k):
    from embeddingnet_amd import ops
    p64, p = _golden_p(g, k)
    y = g[f"yfix{k}"]
    _, _, kl_abs, grad_abs, _ = R.kl_and_grad(p64, y.astype(np.float64))
    out, grad = ops.tsne_kl(p, _dev(y), return_grad=True)
    kl, gn = (float(v) for v in out.cpu())
    grad = grad.cpu().numpy().astype(np.float64)
    want_kl, want_grad = float(g[f"kl_fix{k}"]), g[f"grad_fix{k}"]
    gerr = np.abs(grad - want_grad)
    tol = 16 * U * grad_abs
    print(f"input {k}: KL {kl:.7f} vs {want_kl:.7f}: error {abs(kl - want_kl):.2e}, allowed {16 * U * kl_abs + U * abs(want_kl):.2e}; "
          f"gradient: worst error / allowed {np.max(gerr / tol):.3f}, max |g| {np.abs(want_grad).max():.3e}")
    assert np.all(gerr <= tol + U * np.abs(want_grad))                 # + the rounding of the fp32 result itself
    assert abs(kl - want_kl) <= 16 * U * kl_abs + U * abs(want_kl)
    want_gn = np.linalg.norm(want_grad)
    assert abs(gn - want_gn) <= np.linalg.norm(tol) + 2 * U * want_gn


def _spacing32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def _descent_case(g, k, y0, u0, steps):
    """`steps` iterations (alpha 1, momentum 0.8) on the device, checked two ways against the float64 restatement.

    Step by step: the restatement takes ONE step from the device's stored fp32 state; gains within 1e-6 relative, the update
    within lr * gains * (gradient bound) + one fp32 spacing of the update (it is stored in fp32 and formed from two rounded
    products), Y within that + half a spacing of the stored Y.  The call with n_iter = steps must then equal the chain of
    single calls bit for bit.
    So every step is within its share, and the shares sum over the steps.
    Free running: the restatement runs all steps in float64 from the same start; the gains (the branches taken) must agree
    within 1e-6 relative at the end.  Y is NOT asserted against the free-running trajectory: half a spacing of the stored fp32
    Y (1e-6 at |Y| = 20, already above lr * gains * bound for one step) enters the next gradient, which the momentum and the
    step (lr * dg/dy ~ 0.3 per step near close pairs) amplify; the issue calls this descent chaotic itself.  The figure is
    printed as `y_free`: the deviation over the recurrence e_u(k) = momentum e_u(k-1) + [share of step k],
    e_Y(k) = e_Y(k-1) + e_u(k) + half a spacing, which ignores dg/dy (measured after ten steps: 0.88 on input 0, 6.9 on input 1;
    against lr * gains * bound summed over the steps plus the spacings, without the momentum carry: 1.49 on input 0).
    -> worst measured / allowed ratios and the first step's float64 gradient."""
    from embeddingnet_amd import ops
    p64, p = _golden_p(g, k)
    lr, n = float(g[f"lr{k}"]), len(y0)
    y, u, gains = _dev(y0), _dev(u0), torch.ones(n, 2, device=DEV)
    worst = dict(gains=0.0, update=0.0, y_step=0.0)
    first_grad = None
    for _ in range(steps):
        ry, ru, rg = (t.cpu().numpy().astype(np.float64) for t in (y, u, gains))
        track = []
        R.iterate(p64, ry, ru, rg, 1.0, 0.8, lr, 1, track=track)
        grad, gabs, _ = track[0]
        first_grad = grad if first_grad is None else first_grad
        assert np.all(np.abs(grad) > 16 * U * gabs)                    # the branch is defined: |g| above its error bound
        ops.tsne_iterate(p, y, u, gains, 1.0, 0.8, lr, 1)
        dy, du, dg = (t.cpu().numpy().astype(np.float64) for t in (y, u, gains))
        tol_u = lr * rg * 16 * U * gabs + _spacing32(ru)
        worst["gains"] = max(worst["gains"], np.abs(dg / rg - 1.0).max())
        worst["update"] = max(worst["update"], np.max(np.abs(du - ru) / tol_u))
        worst["y_step"] = max(worst["y_step"], np.max(np.abs(dy - ry) / (tol_u + 0.5 * _spacing32(ry))))
    y2, u2, gains2 = _dev(y0), _dev(u0), torch.ones(n, 2, device=DEV)
    ops.tsne_iterate(p, y2, u2, gains2, 1.0, 0.8, lr, steps)
    assert torch.equal(y2, y) and torch.equal(u2, u) and torch.equal(gains2, gains)
    fy, fu, fg = y0.astype(np.float64), u0.astype(np.float64), np.ones((n, 2))
    e_u, e_y = np.zeros((n, 2)), np.zeros((n, 2))
    for _ in range(steps):
        track = []
        R.iterate(p64, fy, fu, fg, 1.0, 0.8, lr, 1, track=track)
        grad, gabs, _ = track[0]
        assert np.all(np.abs(grad) > 16 * U * gabs)
        e_u = 0.8 * e_u + lr * fg * 16 * U * gabs + _spacing32(fu)
        e_y = e_y + e_u + 0.5 * _spacing32(fy)
    worst["gains_free"] = np.abs(gains.cpu().numpy().astype(np.float64) / fg - 1.0).max()
    worst["y_free"] = np.max(np.abs(y.cpu().numpy().astype(np.float64) - fy) / e_y)
    return worst, first_grad, fg


@pytest.mark.parametrize("k", INPUTS)
def test_one_step_where_the_fp32_product_of_update_and_gradient_is_zero(g, k):
    y0, u0 = g[f"y_far{k}"], g[f"u_far{k}"]
    worst, grad, rg = _descent_case(g, k, y0, u0, 1)
    prod32 = u0 * grad.astype(np.float32)
    assert np.all(grad.astype(np.float32) != 0) and np.all(np.abs(grad) > 1.1754944e-38) and np.all(np.abs(u0) > 1.1754944e-38)
    assert np.abs(u0.astype(np.float64) * grad).max() < 1e-46 and np.all(prod32 == 0)
    n_inc = int(np.sum(np.isclose(rg, 1.2)))
    print(f"input {k}: |g| in [{np.abs(grad).min():.2e}, {np.abs(grad).max():.2e}], {n_inc} of {rg.size} gains take the +0.2 "
          f"branch; measured / allowed: {worst}")
    assert 0 < n_inc < rg.size
    assert worst["gains"] <= 1e-6 and worst["gains_free"] <= 1e-6
    assert worst["update"] <= 1.0 and worst["y_step"] <= 1.0 and worst["y_free"] <= 1.0     # one step: free running = step by step


@pytest.mark.parametrize("k", INPUTS)
@pytest.mark.parametrize("steps", [1, 10])
def test_iterations_vs_restatement(g, k, steps):
    worst, _, _ = _descent_case(g, k, g[f"y_near{k}"], g[f"u_near{k}"], steps)
    print(f"input {k}, {steps} step(s): measured / allowed: {worst}")
    assert worst["gains"] <= 1e-6 and worst["gains_free"] <= 1e-6
    assert worst["update"] <= 1.0 and worst["y_step"] <= 1.0
    if steps == 1:
        assert worst["y_free"] <= 1.0


@pytest.mark.parametrize("k", INPUTS)
def test_end_to_end_vs_sklearn(g, k):
    from embeddingnet_amd.tsne import TSNE
    x = g[f"x{k}"]
    sk0, others = g[f"sk0_{k}"], [g[f"ref64_{k}"], g[f"ref32_{k}"], g[f"sk7_{k}"]]
    t = TSNE(perplexity=float(g["perplexity"]), init='pca', random_state=0, device=DEV)
    emb = t.fit_transform(x)
    assert emb.shape == (len(x), 2) and emb.dtype == np.float32 and np.all(np.isfinite(emb))
    assert t.embedding_ is emb and t.learning_rate_ == float(g[f"lr{k}"])
    gap = abs(t.kl_divergence_ - sk0[0]) / sk0[0]
    allowed = 2.0 * max(abs(o[0] - sk0[0]) / sk0[0] for o in others)
    trust = R.trustworthiness(x, emb, 5)
    trusts = [sk0[2]] + [o[2] for o in others]
    floor = min(trusts) - (max(trusts) - min(trusts))
    print(f"input {k}: KL {t.kl_divergence_:.5f} vs scikit-learn {sk0[0]:.5f}: gap {100 * gap:.2f} % (allowed {100 * allowed:.2f} %); "
          f"n_iter {t.n_iter_} (scikit-learn {int(sk0[1])}); trustworthiness {trust:.4f} (floor {floor:.4f})")
    assert gap <= allowed
    assert trust >= floor
    assert t.n_iter_ <= 999


def test_fit_transform_is_bitwise_reproducible(g):
    from embeddingnet_amd.tsne import TSNE
    x = g["x0"]
    a = TSNE(device=DEV).fit_transform(x)
    b = TSNE(device=DEV).fit(torch.tensor(x, device=DEV)).embedding_
    assert np.array_equal(a, b)
    r1 = TSNE(init='random', random_state=3, max_iter=250, device=DEV).fit_transform(x)
    r2 = TSNE(init='random', random_state=3, max_iter=250, device=DEV).fit_transform(x)
    assert np.array_equal(r1, r2) and not np.array_equal(r1, a)
    y0 = np.random.RandomState(1).randn(len(x), 2).astype(np.float32) * 1e-4
    assert np.all(np.isfinite(TSNE(init=y0, max_iter=250, device=DEV).fit_transform(x)))


def test_size_8192_and_the_smallest_inputs():
    from embeddingnet_amd import ops
    from embeddingnet_amd.tsne import TSNE, pca_init
    n, e, classes = 8192, 256, 64
    gen = torch.Generator(device=DEV).manual_seed(5)
    centres = torch.randn(classes, e, device=DEV, generator=gen)
    x = centres.repeat_interleave(n // classes, 0) + 0.8 * torch.randn(n, e, device=DEV, generator=gen)
    x = x / x.norm(dim=1, keepdim=True)
    ws = ops.tsne_workspace(n, x)
    p, beta = ops.tsne_affinities(ops.pairwise_distances(x, squared=True), 30.0, inplace=True, ws=ws)
    total = float(p.sum(dtype=torch.float64))
    assert abs(total - 1.0) <= 1e-5 and bool(torch.all(beta > 0)) and bool(torch.all(torch.isfinite(beta)))
    y = torch.from_numpy(pca_init(x.cpu().numpy())).to(DEV)
    upd, gains = torch.zeros_like(y), torch.ones_like(y)
    lr = max(n / 12.0 / 4.0, 50.0)
    ops.tsne_iterate(p, y, upd, gains, 12.0, 0.5, lr, 250, ws=ws)
    kls = []
    for _ in range(3):                                                 # iterations 250..299, looked at every 25
        kls.append(float(ops.tsne_kl(p, y, ws=ws)[0]))
        ops.tsne_iterate(p, y, upd, gains, 1.0, 0.8, lr, 25 if len(kls) < 3 else 0, ws=ws)
    print(f"n = {n}: sum P - 1 = {total - 1:.2e}, KL after 250 / 275 / 300 iterations: {kls}")
    assert bool(torch.all(torch.isfinite(y))) and all(np.isfinite(kls))
    assert kls[0] > kls[1] > kls[2] > 0
    for m in (2, 3):
        xs = np.random.RandomState(m).randn(m, 4).astype(np.float32)
        t = TSNE(perplexity=1.0, max_iter=250, device=DEV)
        emb = t.fit_transform(xs)
        assert emb.shape == (m, 2) and np.all(np.isfinite(emb)) and np.isfinite(t.kl_divergence_)


def test_plot_tsne_writes_the_reference_file(tmp_path, monkeypatch):
    from embeddingnet_amd.datagenerators import SyntheticDataLoader
    from embeddingnet_amd.models import TripletNet
    import embedding_net.utils as ref_utils
    monkeypatch.delenv("DISPLAY", raising=False)
    monkeypatch.delenv("WAYLAND_DISPLAY", raising=False)
    dev = torch.device(DEV)
    params = {"model": dict(input_shape=[64, 64, 3], encodings_len=16, mode="triplet", distance_type="l2",
                            backbone_name="simple2", backbone_weights=None, freeze_backbone=False,
                            embeddings_normalization=True, device=dev, seed=0),
              "dataloader": {}, "generator": {}, "train": {}, "general": {"work_dir": str(tmp_path), "project_name": "p"}}
    data = SyntheticDataLoader(5, 8, (64, 64, 3), noise=0.2, validate=False, seed=3)
    net = TripletNet(params, training=True)
    enc = net.generate_encodings(data, max_n_samples=8, shuffle=False)
    net.save_encodings(enc, save_folder=str(tmp_path))
    n = len(enc["labels"])
    assert n == 40
    emb = ref_utils.plot_tsne(str(tmp_path / "encodings.pkl"), str(tmp_path) + os.sep, show=True)
    png = tmp_path / "tsne.png.png"
    assert png.exists() and png.stat().st_size > 1000 and png.read_bytes()[:4] == b"\x89PNG"
    assert emb.shape == (n, 2) and np.all(np.isfinite(emb))
    assert set(pickle.loads((tmp_path / "encodings.pkl").read_bytes())["labels"]) == set(enc["labels"])


def _kl_and_grad_chunked(p, y, rows=256):
    """tsne_ref.kl_and_grad for an n the [n,n,2] temporaries of the plain form would not suit: the same float64 terms, a block
    of rows at a time."""
    n = len(y)
    w_sum = 0.0
    for r0 in range(0, n, rows):
        d = y[r0:r0 + rows, None, :] - y[None, :, :]
        w = 1.0 / (1.0 + (d ** 2).sum(-1))
        w[np.arange(len(w)), np.arange(r0, r0 + len(w))] = 0.0
        w_sum += w.sum()
    kl = kl_abs = 0.0
    grad, grad_abs = np.zeros((n, 2)), np.zeros((n, 2))
    for r0 in range(0, n, rows):
        d = y[r0:r0 + rows, None, :] - y[None, :, :]
        w = 1.0 / (1.0 + (d ** 2).sum(-1))
        idx = (np.arange(len(w)), np.arange(r0, r0 + len(w)))
        w[idx] = 0.0
        q = w / w_sum
        pr = p[r0:r0 + rows]
        ratio = np.maximum(pr, R.EPS) / np.maximum(q, R.EPS)
        ratio[idx] = 1.0
        t = pr * np.log(ratio)
        kl, kl_abs = kl + t.sum(), kl_abs + np.abs(t).sum()
        c = ((pr - q) * w)[:, :, None] * d
        grad[r0:r0 + rows], grad_abs[r0:r0 + rows] = 4.0 * c.sum(1), 4.0 * np.abs(c).sum(1)
    return kl, grad, kl_abs, grad_abs


@pytest.mark.parametrize("n", [301, 4098, 4100])
def test_gradient_and_kl_on_every_launch_shape(n):
    """The row-sum kernel has four shapes: one or four rows per wave (n < 4096 or not), 16-byte loads or scalar ones (n % 4
    == 0 or not).  The golden inputs (n = 300, 400) use one of them; here the other three, on a seeded symmetric P and a
    seeded Y, against the same float64 terms and the same bound."""
    from embeddingnet_amd import ops
    rs = np.random.RandomState(n)
    a = rs.rand(n, n) ** 8
    p64 = a + a.T
    np.fill_diagonal(p64, 0.0)
    p64 = (p64 / p64.sum()).astype(np.float32).astype(np.float64)
    y = (3.0 * rs.randn(n, 2)).astype(np.float32)
    want_kl, want_grad, kl_abs, grad_abs = _kl_and_grad_chunked(p64, y.astype(np.float64))
    out, grad = ops.tsne_kl(_dev(p64), _dev(y), return_grad=True)
    kl, gn = (float(v) for v in out.cpu())
    gerr = np.abs(grad.cpu().numpy().astype(np.float64) - want_grad)
    tol = 16 * U * grad_abs
    print(f"n = {n}: KL error {abs(kl - want_kl):.2e} (allowed {16 * U * kl_abs + U * abs(want_kl):.2e}); gradient: worst error / "
          f"allowed {np.max(gerr / tol):.3f}")
    assert np.all(gerr <= tol + U * np.abs(want_grad))
    assert abs(kl - want_kl) <= 16 * U * kl_abs + U * abs(want_kl)
    assert abs(gn - np.linalg.norm(want_grad)) <= np.linalg.norm(tol) + 2 * U * np.linalg.norm(want_grad)


def test_affinities_on_streamed_rows():
    """n > 4096: the bisection streams its row instead of keeping it in LDS.  Every row's perplexity, recomputed in float64
    from the returned beta, is within 1e-4 relative of the request; P is symmetric bit for bit, sums to 1, has a zero diagonal."""
    from embeddingnet_amd import ops
    n, e, perp = 4101, 16, 50.0
    rs = np.random.RandomState(9)
    x = np.repeat(rs.randn(41, e), 101, axis=0)[:n] + 0.7 * rs.randn(n, e)
    d2 = ops.pairwise_distances(_dev(x), squared=True)
    d64 = d2.cpu().numpy().astype(np.float64)
    p, beta = ops.tsne_affinities(d2, perp)
    b = beta.cpu().numpy().astype(np.float64)
    np.fill_diagonal(d64, np.inf)
    d64 -= d64.min(axis=1, keepdims=True)
    w = np.exp(-d64 * b[:, None])
    s = w.sum(1)
    h = np.log(s) + b * (np.where(np.isfinite(d64), d64, 0.0) * w).sum(1) / s
    rel = np.abs(np.exp(h) / perp - 1.0).max()
    total = float(p.sum(dtype=torch.float64))
    print(f"n = {n}: worst relative perplexity error {rel:.2e}; sum P - 1 = {total - 1:.2e}")
    assert rel <= 1e-4
    assert abs(total - 1.0) <= 1e-5 and torch.equal(p, p.t().contiguous()) and bool(torch.all(torch.diagonal(p) == 0))
    assert float(p[~torch.eye(n, dtype=torch.bool, device=DEV)].min()) >= 2.220446e-16
