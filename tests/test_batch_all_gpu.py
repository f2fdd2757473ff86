"""Batch-all triplet loss (ops.batch_all_triplet_loss, csrc/batch_all.hip) against an f64 reference, the existing gathered
hinge, its own second forward path, and inside the training step (eager, graph-replayed, tools/train.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recipes as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP4 = 4.0 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- f64 reference
def ref_batch_all(x, p, k, margin):
    """-> dict(loss, A, T, frac, W [n,n], min_abs_b) in f64; d(i,j) = sum_c (x_ic - x_jc)^2, active iff b > 0."""
    x = np.asarray(x, np.float64)
    n = p * k
    sq = (x * x).sum(1)
    d = sq[:, None] + sq[None, :] - 2.0 * x @ x.T
    W = np.zeros((n, n))
    total, A, min_b = 0.0, 0, np.inf
    for c in range(p):
        lo = c * k
        neg = np.r_[0:lo, lo + k:n]
        dap = d[lo:lo + k, lo:lo + k]                           # [anchor, positive]
        dan = d[lo:lo + k][:, neg]                              # [anchor, negative]
        b = dap[:, :, None] - dan[:, None, :] + margin          # [anchor, positive, negative]
        valid = ~np.eye(k, dtype=bool)[:, :, None] & np.ones_like(b, dtype=bool)
        act = (b > 0) & valid
        min_b = min(min_b, np.abs(b[valid]).min())
        total += b[act].sum()
        A += int(act.sum())
        W[lo:lo + k, lo:lo + k] = act.sum(2)
        W[lo:lo + k, neg] = -act.sum(1)
    T = n * (k - 1) * (n - k)
    return dict(loss=total / max(A, 1), A=A, T=T, frac=A / T, W=W, min_abs_b=min_b)


def ref_grad(x, W, A, g=1.0, rows=None):
    """demb in f64 and the per-element bound 4 ulp * scale * sum_j |M_ij| |x_i - x_j| (M = W + W^T), for `rows`."""
    x = np.asarray(x, np.float64)
    M = W + W.T
    rows = np.arange(x.shape[0]) if rows is None else rows
    scale = 2.0 * g / max(A, 1)
    want = scale * (M[rows].sum(1)[:, None] * x[rows] - M[rows] @ x)
    bound = np.empty_like(want)
    for r0 in range(0, len(rows), 16):
        rr = rows[r0:r0 + 16]
        bound[r0:r0 + 16] = np.einsum("ij,ijc->ic", np.abs(M[rr]), np.abs(x[rr][:, None, :] - x[None, :, :]))
    return want, ULP4 * abs(scale) * bound + 1e-12


def grid_embeddings(seed, p, k, e, sigma=0.6):
    """R.clustered_embeddings scaled to O(1) components and rounded to multiples of 1/8: every squared distance is then a
    multiple of 1/64 and exact in fp32 in both the difference and the Gram form, so the active set cannot depend on the
    summation order.  With the margin half a step off that grid (grid_margin) every |b| >= 1/128."""
    x = R.clustered_embeddings(seed, p, k, e, sigma)
    return (np.round(x * np.sqrt(e) * 8.0) / 8.0).astype(np.float32)


def grid_margin(x, p, k, q=0.5):
    """a margin on the 1/64 grid plus 1/128, near the q-quantile of d(a,n) - d(a,p) (so some triplets are active, some not)."""
    x = x.astype(np.float64)
    rs = np.random.RandomState(1)
    n = p * k
    a = rs.randint(0, n, 4000)
    pp = (a // k) * k + (a % k + 1 + rs.randint(0, k - 1, 4000)) % k
    nn = (a // k * k + k + rs.randint(0, n - k, 4000)) % n
    gap = ((x[a] - x[nn]) ** 2).sum(1) - ((x[a] - x[pp]) ** 2).sum(1)
    return float(np.round(np.quantile(gap, q) * 64.0) / 64.0 + 1.0 / 128.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(x, p, k, margin, dev, path="auto", g=None):
    from embeddingnet_amd import ops
    xt = torch.tensor(x, device=dev, requires_grad=True)
    mean, n_act, frac, w = ops.batch_all_triplet_loss(xt, p, k, margin, path=path, return_weights=True)
    if g is None:
        mean.backward()
    else:
        mean.backward(torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), A=int(n_act.item()), frac=float(frac.item()), W=w.cpu().numpy(),
                grad=xt.grad.cpu().numpy(), mean_t=mean.detach().clone(), n_t=n_act.clone(), frac_t=frac.clone())


def _check_against_ref(got, ref, x, rows=None, g=1.0):
    assert got["A"] == ref["A"]
    assert got["frac"] == np.float32(ref["A"] / ref["T"])
    assert abs(got["loss"] - ref["loss"]) <= 1e-5 * max(abs(ref["loss"]), 1e-30)
    assert np.array_equal(got["W"], ref["W"].astype(np.float32))
    want, bound = ref_grad(x, ref["W"], ref["A"], g, rows)
    have = got["grad"] if rows is None else got["grad"][rows]
    err = np.abs(have - want)
    assert np.all(err <= bound), (err / bound).max()


# ---------------------------------------------------------------------------------------------------------------- 1. values
SHAPES = [(8, 4, 256), (32, 4, 256), (64, 4, 512), (3, 3, 64), (20, 3, 128), (16, 16, 128), (5, 7, 33), (4, 4, 4096),
          (256, 8, 128)]


@pytest.mark.parametrize("p,k,e", SHAPES, ids=lambda v: str(v))
def test_values_vs_f64_reference(dev, p, k, e):
    from embeddingnet_amd import _lib
    x = grid_embeddings(p * 1000 + k * 10 + e, p, k, e)
    margin = grid_margin(x, p, k)
    ref = ref_batch_all(x, p, k, margin)
    assert ref["min_abs_b"] >= 1.0 / 128.0 and 0 < ref["A"] < ref["T"]
    got = _run(x, p, k, margin, dev, g=0.75)
    n = p * k
    rows = None if n <= 512 else np.r_[0:96, n // 2:n // 2 + 32, n - 96:n]
    _check_against_ref(got, ref, x, rows, g=0.75)
    if n > 512 or e > 1024:
        assert _lib.lib().embnet_batch_all_path(p, k, e) == 2            # the distance-matrix path is covered here


def test_backward_precision_on_continuous_embeddings(dev):
    """Unquantised C2 embeddings: the gradient from the kernel's own W and A meets the per-element bound."""
    p, k, e = 32, 4, 256
    x = R.clustered_embeddings(11, p, k, e, 0.7)
    got = _run(x, p, k, 0.2, dev)
    assert 0 < got["A"]
    want, bound = ref_grad(x, got["W"].astype(np.float64), got["A"])
    err = np.abs(got["grad"] - want)
    assert np.all(err <= bound), (err / bound).max()


# ---------------------------------------------------------------------------------------------------------------- 2. vs gather
def test_matches_gathered_hinge_on_the_active_triplets(dev):
    from embeddingnet_amd import ops
    p, k, e = 8, 4, 256
    x = grid_embeddings(5, p, k, e)
    margin = grid_margin(x, p, k)
    ref = ref_batch_all(x, p, k, margin)
    n = p * k
    xd = x.astype(np.float64)
    d = ((xd[:, None, :] - xd[None, :, :]) ** 2).sum(-1)
    trip = [(a, q, m) for a in range(n) for q in range(a // k * k, a // k * k + k) if q != a
            for m in range(n) if m // k != a // k and d[a, q] - d[a, m] + margin > 0]
    assert len(trip) == ref["A"] > 0
    got = _run(x, p, k, margin, dev)
    xt = torch.tensor(x, device=dev, requires_grad=True)
    tt = torch.tensor(np.array(trip, np.int32), device=dev)
    cnt = torch.tensor([len(trip)], dtype=torch.int32, device=dev)
    mean, _ = ops.triplet_gather_loss(xt, tt, cnt, margin)
    mean.backward()
    gm = float(mean.item())
    assert abs(gm - got["loss"]) <= 1e-5 * abs(gm)
    _, bound = ref_grad(x, ref["W"], ref["A"])
    err = np.abs(xt.grad.cpu().numpy() - got["grad"])
    assert np.all(err <= bound), (err / bound).max()


# ---------------------------------------------------------------------------------------------------------------- 3. edges
def test_no_active_triplet_gives_zero_loss_and_zero_gradient(dev):
    p, k, e = 4, 3, 8
    x = np.zeros((p * k, e), np.float32)
    for c in range(p):
        x[c * k:(c + 1) * k, c] = 10.0
        x[c * k:(c + 1) * k, 4 + c % 4] = np.arange(k) * 0.125
    got = _run(x, p, k, 1e-3, dev)
    assert got["A"] == 0 and got["loss"] == 0.0 and got["frac"] == 0.0
    assert np.all(got["W"] == 0) and np.all(got["grad"] == 0) and np.isfinite(got["grad"]).all()


@pytest.mark.parametrize("path", ["per_class", "distance_matrix"])
def test_huge_margin_makes_every_triplet_active(dev, path):
    p, k, e = 6, 4, 64
    x = grid_embeddings(3, p, k, e)
    ref = ref_batch_all(x, p, k, 1e4)
    got = _run(x, p, k, 1e4, dev, path=path)
    assert got["A"] == ref["T"] == ref["A"] and got["frac"] == 1.0
    _check_against_ref(got, ref, x)


def test_every_triplet_active_at_the_int32_limit(dev):
    """32 x 128 rows: T = 4096 * 127 * 3968 = 2 064 121 856, the largest count the range rule admits at n = 4096, on the
    distance-matrix path (k > 16).  Every triplet is active, so the expected values have a closed form: W[a,p] = n - k,
    W[a,n] = -(k - 1), loss = margin + sum_a ((n - k) sum_p d(a,p) - (k - 1) sum_n d(a,n)) / T.  Coordinates are multiples of
    1/8, so every d and every b is a multiple of 1/64 below 2^14: exact in fp32 in either rounding form."""
    from embeddingnet_amd import _lib
    p, k, e, margin = 32, 128, 4, 1e4
    n = p * k
    T = n * (k - 1) * (n - k)
    assert T == 2064121856 < 2 ** 31 and _lib.lib().embnet_batch_all_path(p, k, e) == 2
    x = grid_embeddings(9, p, k, e)
    xd = x.astype(np.float64)
    sq = (xd * xd).sum(1)
    d = sq[:, None] + sq[None, :] - 2.0 * xd @ xd.T                  # exact: multiples of 1/64
    assert d.max() < margin and d.max() + margin < 2.0 ** 14
    same = np.kron(np.eye(p, dtype=bool), np.ones((k, k), dtype=bool))
    W = np.where(same, float(n - k), -float(k - 1))
    np.fill_diagonal(W, 0.0)
    loss = margin + ((n - k) * d[same].sum() - (k - 1) * d[~same].sum()) / T
    ref = dict(loss=loss, A=T, T=T, W=W)
    got = _run(x, p, k, margin, dev)
    assert got["A"] == T and got["frac"] == 1.0
    _check_against_ref(got, ref, x, rows=np.r_[0:96, n // 2:n // 2 + 32, n - 96:n])


def test_duplicate_rows(dev):
    p, k, e = 5, 4, 32
    x = grid_embeddings(8, p, k, e)
    x[1::k] = x[0::k]                                               # rows 0 and 1 of every class coincide: d(a,p) = 0
    margin = grid_margin(x, p, k)
    ref = ref_batch_all(x, p, k, margin)
    assert 0 < ref["A"] < ref["T"]
    _check_against_ref(_run(x, p, k, margin, dev), ref, x)


@pytest.mark.parametrize("p,k,e", [(1, 4, 16), (4, 1, 16), (2, 2049, 4), (4, 4, 4097), (4, 32, 16)])
def test_out_of_range_arguments_raise(dev, p, k, e):
    from embeddingnet_amd import _lib, ops
    x = torch.rand((p * k, e), device=dev)
    path = "per_class" if (p, k) == (4, 32) else "auto"
    with pytest.raises(_lib.EmbnetError):
        ops.batch_all_triplet_loss(x, p, k, 0.5, path=path)
    with pytest.raises(_lib.EmbnetError):
        ops.batch_all_triplet_loss(x, p + 1, k, 0.5)                # rows != p*k


# ---------------------------------------------------------------------------------------------------------------- 4. two paths
def test_forward_paths_agree(dev):
    p, k, e = 8, 4, 256
    for seed in range(40):                                          # continuous data: a seed with every |b| >= 1e-4
        x = R.clustered_embeddings(seed, p, k, e, 0.7)
        ref = ref_batch_all(x, p, k, 0.2)
        if ref["min_abs_b"] >= 1e-4:
            break
    assert ref["min_abs_b"] >= 1e-4 and 0 < ref["A"] < ref["T"]
    a = _run(x, p, k, 0.2, dev, path="per_class")
    b = _run(x, p, k, 0.2, dev, path="distance_matrix")
    assert a["A"] == b["A"] == ref["A"]
    assert abs(a["loss"] - b["loss"]) <= 1e-5 * abs(a["loss"])
    assert abs(a["loss"] - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert np.array_equal(a["W"], b["W"])


# ---------------------------------------------------------------------------------------------------------------- 5. reproducible
@pytest.mark.parametrize("p,k,e", [(32, 4, 256), (256, 8, 128)])
def test_bitwise_reproducible(dev, p, k, e):
    x = R.clustered_embeddings(4, p, k, e, 0.7)
    r1, r2 = _run(x, p, k, 0.2, dev), _run(x, p, k, 0.2, dev)
    for key in ("mean_t", "n_t", "frac_t"):
        assert torch.equal(r1[key], r2[key]), key
    assert np.array_equal(r1["W"], r2["W"]) and np.array_equal(r1["grad"], r2["grad"])


# ---------------------------------------------------------------------------------------------------------------- 6. training
def _trainer(dev, graph, seed=5):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=seed,
                             device=dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-3)
    return base, opt, TripletTrainer(base, opt, 8, 4, margin=0.5, negatives_selection_mode="batch_all", seed=3, graph=graph)


def _batches(dev, steps):
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((12, 64, 64, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(12, generator=torch.Generator().manual_seed(i))[:8].to(dev)
        x = protos[cls].repeat_interleave(4, 0) + 0.15 * torch.randn((32, 64, 64, 3), device=dev, generator=gen)
        yield x.clamp(0, 1)


def test_trainer_batch_all_learns(dev):
    _, _, tr = _trainer(dev, graph=False)
    losses = []
    for x in _batches(dev, 25):
        losses.append(float(tr.step(x).item()))
        trip, count = tr.last_triplets
        assert trip is None and count.dtype == torch.int32 and count.shape == (1,)
    assert np.all(np.isfinite(losses))
    assert min(losses[-5:]) < losses[0], losses


def test_trainer_batch_all_graph_replay_equals_eager(dev):
    from embeddingnet_amd import _lib
    runs = []
    for graph in (False, True):
        base, opt, tr = _trainer(dev, graph=graph)
        losses, counts = [], []
        for i, x in enumerate(_batches(dev, 14)):
            if graph and i == 11:
                _lib.trace_enable(True)                             # an eager step between replays
            losses.append(tr.step(x).clone())
            _lib.trace_enable(False)
            counts.append(tr.last_triplets[1].clone())
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        runs.append((torch.stack(losses), torch.stack(counts), torch.cat([q.detach().reshape(-1) for q in base.parameters()])))
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0] - runs[1][0]).abs().max()
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])


# ---------------------------------------------------------------------------------------------------------------- 7. CLI
@pytest.mark.parametrize("mode", ["batch_all", "batch_hard"])
def test_train_cli_step_only_modes(tmp_path, mode):
    cfg = open(os.path.join(ROOT, "configs", "simple2_synthetic.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert "negatives_selection_mode : 'semihard'" in cfg and "n_batches : 20" in cfg
    cfg = cfg.replace("negatives_selection_mode : 'semihard'", f"negatives_selection_mode : '{mode}'")
    cfg = cfg.replace("n_batches : 20", "n_batches : 4")
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(cfg)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path), "--synthetic", "10",
                          "--max_epochs", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch 2/2" in out.stdout and "saving model" in out.stdout
    assert any(f.startswith("epoch_") for f in os.listdir(tmp_path / "simple2_synthetic" / "weights"))
