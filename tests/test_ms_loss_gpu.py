"""Multi-similarity loss (ops.multi_similarity_loss, csrc/multi_similarity.hip) against the float64 reference and the a-priori bounds
of tests/ms_ref.py, its two forward paths against each other, and inside the training step (eager, graph-replayed, tools/train.py).

Every check prints its largest error / bound before it asserts ratio < 1.  Largest ratios observed on an MI355X, per group of
checks (the gradient's bound is one fp32 rounding of the result, which a nearest rounding all but reaches):
  grid               open_share 0  G 0.122  loss 0.0772  grad 0.999
  per_class          open_share 0  G 0.0622  loss 0.0125  grad 0.998
  similarity_matrix  open_share 0  G 0.0622  loss 0.0125  grad 0.998
  continuous         open_share 0.00391  G 0.0605  loss 0.0295  grad 0.999
  backward           grad 0.996
  eps=1e4            open_share 0  G 0.0804  loss 0.0175  grad 0.978
  duplicates         open_share 0  G 0.0701  loss 0.04  grad 0.955
  norm               open_share 0  G 1.31e-77  loss 0  grad 0
  offset             open_share 0  G 0.107  loss 0.0652  grad 0.992
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ms_ref as M
import recipes as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = 0.75


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(x, p, k, dev, path="auto", g=None, **params):
    from embeddingnet_amd import ops
    xt = x if torch.is_tensor(x) else torch.tensor(x, device=dev)
    xt = xt.detach().requires_grad_(True)
    mean, counts, gw = ops.multi_similarity_loss(xt, p, k, path=path, return_weights=True, **params)
    mean.backward(None if g is None else torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), counts=counts.cpu().numpy(), G=gw.cpu().numpy(), grad=xt.grad.cpu().numpy(),
                mean_t=mean.detach().clone(), counts_t=counts.clone(), G_t=gw, grad_t=xt.grad)


def _grad_rows(n):
    return None if n <= 512 else np.r_[0:96, n // 2:n // 2 + 32, n - 96:n]


def _check(got, x, p, k, gs, g=1.0, what="", underflow=False, unit=None, **params):
    """Everything the header promises about one forward + backward, for a device whose S is within gs A of the truth: counts,
    the zero pattern of G, every weight, the loss and (from the device's own G) every gradient element.  Anchors whose mining
    decision gs leaves open (at most 1 %) are judged with the device's own decision, which must lie between `sure` and `may`.
    -> {check: largest error / bound}."""
    n = p * k
    eps = params.get("epsilon", 0.1)
    assert gs > 0 or M.exact_in_any_order(x, unit)                         # gamma_S = 0 only where S is exact in any order
    pos, neg = M.class_masks(p, k)
    nz = got["G"] != 0
    assert np.isfinite(got["G"]).all() and np.isfinite(got["grad"]).all() and np.isfinite(got["loss"])
    assert not nz[~(pos | neg)].any()                                      # the diagonal
    assert np.all(got["G"][pos] <= 0) and np.all(got["G"][neg] >= 0)
    d = M.decisions(x, p, k, eps, gs)
    share = d["open"].mean()
    assert share <= 0.01, share
    ref = M.reference(x, p, k, **params)
    if underflow:                                                           # weights below 2^-126 may be flushed to zero
        big = np.abs(ref["G"]) >= 2.0 ** -120
        assert np.all(nz <= (ref["keep_pos"] | ref["keep_neg"])) and np.all(big <= nz)
    else:
        closed = ~d["open"]
        assert np.array_equal(nz[closed], (ref["keep_pos"] | ref["keep_neg"])[closed])
        if share:
            assert np.all((d["sure_pos"] | d["sure_neg"]) <= nz) and np.all(nz <= (d["may_pos"] | d["may_neg"]))
            ref = M.reference(x, p, k, keep=(nz & pos, nz & neg), **params)
        assert np.array_equal(got["counts"], ref["counts"].astype(np.int32)), (got["counts"], ref["counts"])
    bg, _, bl = M.bounds(x, ref, gs)
    kept = ref["keep_pos"] | ref["keep_neg"]
    ratios = dict(open_share=float(share))
    ratios["G"] = float((np.abs(got["G"] - ref["G"])[kept] / bg[kept]).max()) if kept.any() else 0.0
    ratios["loss"] = float(abs(got["loss"] - ref["loss"]) / bl) if bl > 0 else float(got["loss"] != 0)
    rows = _grad_rows(n)
    want, bound = M.grad(x, got["G"], g, rows)
    have = got["grad"] if rows is None else got["grad"][rows]
    ratios["grad"] = float((np.abs(have - want) / bound).max())
    print(f"ms_loss {what} p={p} k={k} e={x.shape[1]}: " + " ".join(f"{a}={b:.3g}" for a, b in ratios.items()))
    assert ratios["G"] < 1 and ratios["loss"] < 1 and ratios["grad"] < 1, ratios
    return ratios


def _grid(p, k, e, seed=None, sigma=M.SIGMA):
    """-> (x on the 1/q grid, epsilon half a step off the grid of S, unit = 1/q)."""
    x, eps, q = M.grid_inputs(R.clustered_embeddings(M.seed_of(p, k, e) if seed is None else seed, p, k, e, sigma))
    return x, eps, 1.0 / q


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("p,k,e", M.VALUE_SHAPES, ids=str)
def test_values_on_grid_inputs(dev, p, k, e):
    """S is exact in any order (test_ms_ref_cpu.py), so counts and the zero pattern are exact and gamma_S = 0 in the bounds."""
    from embeddingnet_amd import _lib
    x, eps, unit = _grid(p, k, e)
    got = _run(x, p, k, dev, g=UP, epsilon=eps)
    r = _check(got, x, p, k, 0.0, unit=unit, g=UP, what="grid", epsilon=eps)
    assert r["open_share"] == 0
    n = p * k
    assert 0 < got["counts"][0] and 0 < got["counts"][1] < n * (n - k) and got["counts"][3] == got["counts"][0] + got["counts"][1]
    assert _lib.lib().embnet_ms_loss_path(p, k, e) == (2 if (p, k, e) in M.VALUE_SHAPES[-2:] else 1)


def test_forward_paths_agree_on_a_grid_input(dev):
    p, k, e = 8, 4, 256
    x, eps, unit = _grid(p, k, e, seed=5)
    a = _run(x, p, k, dev, path="per_class", epsilon=eps)
    b = _run(x, p, k, dev, path="similarity_matrix", epsilon=eps)
    assert np.array_equal(a["counts"], b["counts"]) and a["counts"][2] > 0
    assert np.array_equal(a["G"] != 0, b["G"] != 0)
    _check(a, x, p, k, 0.0, unit=unit, what="per_class", epsilon=eps)
    _check(b, x, p, k, 0.0, unit=unit, what="similarity_matrix", epsilon=eps)


# ---------------------------------------------------------------------------------------------------------------- 2. continuous
@pytest.mark.parametrize("p,k,e", M.CONTINUOUS_SHAPES, ids=str)
def test_values_on_continuous_inputs(dev, p, k, e):
    x = R.clustered_embeddings(M.seed_of(p, k, e), p, k, e, M.SIGMA)
    got = _run(x, p, k, dev, g=UP)
    _check(got, x, p, k, M.gamma_s(M.auto_path(p, k, e), e), g=UP, what="continuous")
    assert got["counts"][2] > 0


def test_backward_precision_on_continuous_embeddings(dev):
    """Unquantised C2 embeddings: the gradient from the kernel's own G meets the per-element bound, at two upstream values."""
    p, k, e = 32, 4, 256
    x = R.clustered_embeddings(11, p, k, e, 0.7)
    for g in (None, -3.0):
        got = _run(x, p, k, dev, g=g)
        assert got["counts"][3] > 0 and np.abs(got["grad"]).max() > 0
        want, bound = M.grad(x, got["G"], 1.0 if g is None else g)
        ratio = (np.abs(got["grad"] - want) / bound).max()
        print(f"ms_loss backward g={g}: grad={ratio:.3g}")
        assert ratio < 1


# ---------------------------------------------------------------------------------------------------------------- 3. edges
def test_no_active_anchor_gives_zero_loss_and_zero_gradient(dev):
    p, k, e = 4, 3, 8
    x = np.zeros((p * k, e), np.float32)
    for c in range(p):
        x[c * k:(c + 1) * k, c] = 1.0
        x[c * k:(c + 1) * k, 4 + c] = np.arange(k) * 0.25
    for path in ("per_class", "similarity_matrix"):
        got = _run(x, p, k, dev, path=path)
        assert got["loss"] == 0.0 and not got["counts"].any()
        assert np.all(got["G"] == 0) and np.all(got["grad"] == 0) and np.isfinite(got["grad"]).all()


@pytest.mark.parametrize("path", ["per_class", "similarity_matrix"])
def test_huge_epsilon_keeps_every_pair(dev, path):
    p, k, e = 6, 4, 64
    x, _, unit = _grid(p, k, e, seed=3)
    got = _run(x, p, k, dev, path=path, epsilon=1e4)
    n = p * k
    assert list(got["counts"]) == [n * (k - 1), n * (n - k), n, n * (n - 1)]
    _check(got, x, p, k, 0.0, unit=unit, what="eps=1e4 " + path, epsilon=1e4)


def test_duplicate_rows(dev):
    p, k, e = 5, 4, 32
    x, eps, unit = _grid(p, k, e, seed=8)
    x[1::k] = x[0::k]                                               # rows 0 and 1 of every class coincide
    got = _run(x, p, k, dev, epsilon=eps)
    assert got["counts"][2] > 0
    _check(got, x, p, k, 0.0, unit=unit, what="duplicates", epsilon=eps)


@pytest.mark.parametrize("path", ["per_class", "similarity_matrix"])
def test_unnormalised_rows_of_norm_30_stay_finite_and_within_bounds(dev, path):
    """t- = 50 (S - 1/2) reaches 3e4: the plain formula overflows fp32 (and float64), the stable form does not."""
    p, k, e = 6, 4, 64
    x, eps, unit = _grid(p, k, e, seed=3)
    x = (x * np.float32(30.0)).astype(np.float32)                   # still exact: S q^2 / 900 is an integer below 2^24 / 900
    ref = M.reference(x, p, k, epsilon=eps)
    assert ref["counts"][2] > 0 and ref["sides"]["neg"]["m"].max() > 1e4 and np.isfinite(ref["loss"])
    got = _run(x, p, k, dev, path=path, epsilon=eps)
    assert np.array_equal(got["counts"], ref["counts"].astype(np.int32))
    _check(got, x, p, k, 0.0, unit=30.0 * unit, what="norm 30 " + path, underflow=True, epsilon=eps)


@pytest.mark.parametrize("p,k,e,path", [(4, 3, 1, "per_class"), (4, 3, 1, "similarity_matrix"), (5, 7, 33, "similarity_matrix"),
                                        (16, 2, 48, "per_class"), (16, 2, 48, "similarity_matrix"), (3, 16, 40, "per_class")],
                         ids=str)
def test_small_and_odd_shapes_from_an_offset_pointer(dev, p, k, e, path):
    """E = 1, E = 33, K = 2, K = 16, with the block one float behind a 16-byte boundary (the dense GEMM's scalar loader)."""
    x, eps, unit = _grid(p, k, e)
    buf = torch.zeros(p * k * e + 1, device=dev)
    xt = buf[1:].view(p * k, e)
    xt.copy_(torch.tensor(x))
    assert xt.data_ptr() % 16 == 4
    got = _run(xt, p, k, dev, path=path, g=UP, epsilon=eps)
    _check(got, x, p, k, 0.0, unit=unit, g=UP, what="offset " + path, epsilon=eps)


@pytest.mark.parametrize("p,k,e", [(1, 4, 16), (4, 1, 16), (2, 2049, 4), (4, 4, 4097), (4, 32, 16)])
def test_out_of_range_arguments_raise(dev, p, k, e):
    from embeddingnet_amd import _lib, ops
    x = torch.rand((p * k, e), device=dev)
    path = "per_class" if (p, k) == (4, 32) else "auto"
    with pytest.raises(_lib.EmbnetError):
        ops.multi_similarity_loss(x, p, k, path=path)
    with pytest.raises(_lib.EmbnetError):
        ops.multi_similarity_loss(x, p + 1, k)                      # rows != p*k
    with pytest.raises(_lib.EmbnetError):
        ops.multi_similarity_loss(torch.rand((8, 4), device=dev), 4, 2, alpha=0.0)
    with pytest.raises(_lib.EmbnetError):
        ops.multi_similarity_loss(torch.rand((8, 4), device=dev), 4, 2, epsilon=-0.1)


def _raw(xt, p, k, eps, path, pad, stream=None, fill_ff=False):
    """The C ABI directly on buffers with `pad` guard elements on either side.  -> (G, demb, counts, mean, ws) guarded tensors."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    n, e = xt.shape
    dev = xt.device
    wsn = lib.embnet_ms_loss_workspace_bytes(p, k, e) // 4
    gb = torch.full((2 * pad + n * n,), float("nan"), device=dev)
    if fill_ff:
        gb.view(torch.int32).fill_(-1)                              # 0xFF bytes
    db = torch.full((2 * pad + n * e,), float("nan"), device=dev)
    cb = torch.full((2 * pad + 4,), -12345, dtype=torch.int32, device=dev)
    mb = torch.full((2 * pad + 1,), float("nan"), device=dev)
    wb = torch.full((2 * pad + wsn,), float("nan"), device=dev)
    wb[pad:pad + wsn] = 0
    up = torch.tensor(UP, device=dev)
    torch.cuda.synchronize()
    s = _lib.stream() if stream is None else stream.cuda_stream
    sl = lambda t, m: t[pad:pad + m]
    _lib.check(lib.embnet_ms_loss_fwd(xt.data_ptr(), p, k, e, 2.0, 50.0, 0.5, eps, path, sl(gb, n * n).data_ptr(),
                                      sl(cb, 4).data_ptr(), sl(mb, 1).data_ptr(), sl(wb, wsn).data_ptr(), wsn * 4, s))
    _lib.check(lib.embnet_ms_loss_bwd(xt.data_ptr(), n, e, sl(gb, n * n).data_ptr(), up.data_ptr(), sl(db, n * e).data_ptr(), s))
    torch.cuda.synchronize()
    return gb, db, cb, mb, wb


@pytest.mark.parametrize("path", [1, 2])
def test_nothing_is_written_outside_the_outputs(dev, path):
    p, k, e, pad = 5, 7, 33, 64                                     # N = 35: ragged tiles in every kernel
    x, eps, unit = _grid(p, k, e)
    xt = torch.tensor(x, device=dev)
    gb, db, cb, mb, wb = _raw(xt, p, k, eps, path, pad)
    for t in (gb, db, mb, wb):
        assert torch.isnan(t[:pad]).all() and torch.isnan(t[-pad:]).all()
        assert torch.isfinite(t[pad:-pad]).all()
    assert (cb[:pad] == -12345).all() and (cb[-pad:] == -12345).all()
    assert wb[pad].view(torch.int32).item() == 0                    # the ticket is re-armed
    got = _run(x, p, k, dev, path={1: "per_class", 2: "similarity_matrix"}[path], g=UP, epsilon=eps)
    n = p * k
    assert np.array_equal(gb[pad:-pad].view(n, n).cpu().numpy(), got["G"])
    assert np.array_equal(db[pad:-pad].view(n, e).cpu().numpy(), got["grad"])
    assert np.array_equal(cb[pad:-pad].cpu().numpy(), got["counts"]) and mb[pad].item() == got["loss"]


# ---------------------------------------------------------------------------------------------------------------- 4. reproducible
@pytest.mark.parametrize("p,k,e", [(32, 4, 256), (256, 8, 128)], ids=str)
def test_bitwise_reproducible(dev, p, k, e):
    x = R.clustered_embeddings(4, p, k, e, 0.7)
    r1, r2 = _run(x, p, k, dev, g=UP), _run(x, p, k, dev, g=UP)
    for key in ("mean_t", "counts_t", "G_t", "grad_t"):
        assert torch.equal(r1[key], r2[key]), key
    assert r1["counts"][3] > 0
    # a second stream, its own workspace, a G buffer full of 0xFF bytes
    n = p * k
    s2 = torch.cuda.Stream(device=dev)
    gb, db, cb, mb, _ = _raw(torch.tensor(x, device=dev), p, k, 0.1, 0, 16, stream=s2, fill_ff=True)
    assert torch.equal(gb[16:-16].view(n, n), r1["G_t"]) and torch.equal(db[16:-16].view(n, e), r1["grad_t"])
    assert torch.equal(cb[16:-16], r1["counts_t"]) and torch.equal(mb[16], r1["mean_t"])


# ---------------------------------------------------------------------------------------------------------------- 5. training
def _trainer(dev, graph, seed=5):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=seed,
                             device=dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-3)
    return base, opt, TripletTrainer(base, opt, 8, 4, negatives_selection_mode="multi_similarity", seed=3, graph=graph)


def _batches(dev, steps):
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((12, 64, 64, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(12, generator=torch.Generator().manual_seed(i))[:8].to(dev)
        x = protos[cls].repeat_interleave(4, 0) + 0.15 * torch.randn((32, 64, 64, 3), device=dev, generator=gen)
        yield x.clamp(0, 1)


def test_trainer_multi_similarity_learns(dev):
    _, _, tr = _trainer(dev, graph=False)
    losses = []
    for x in _batches(dev, 25):
        losses.append(float(tr.step(x).item()))
        trip, count = tr.last_triplets
        assert trip is None and count.dtype == torch.int32 and count.shape == (1,)
        assert tr.last_pair_counts.shape == (4,) and int(tr.last_pair_counts[3]) == int(count)
    print("ms_loss trainer losses", [round(v, 4) for v in losses])
    assert np.all(np.isfinite(losses))
    assert max(losses[-5:]) < losses[0], losses


def test_trainer_multi_similarity_graph_replay_equals_eager(dev):
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
            assert tr.last_triplets[1].data_ptr() == tr.last_pair_counts.data_ptr() + 12
            counts.append(tr.last_pair_counts.clone())
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        runs.append((torch.stack(losses), torch.stack(counts), torch.cat([q.detach().reshape(-1) for q in base.parameters()])))
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0] - runs[1][0]).abs().max()
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])


# ---------------------------------------------------------------------------------------------------------------- 6. CLI
def _cli(tmp_path, edit):
    cfg = open(os.path.join(ROOT, "configs", "simple2_ms_synthetic.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert "negatives_selection_mode : 'multi_similarity'" in cfg and "n_batches : 20" in cfg and "ms_loss :" in cfg
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(edit(cfg.replace("n_batches : 20", "n_batches : 4")))
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path), "--synthetic", "10",
                           "--max_epochs", "2"], capture_output=True, text=True, timeout=600)


def test_train_cli_multi_similarity_config(tmp_path):
    out = _cli(tmp_path, lambda cfg: cfg)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch 2/2" in out.stdout and "saving model" in out.stdout
    assert any(f.startswith("epoch_") for f in os.listdir(tmp_path / "simple2_ms_synthetic" / "weights"))


def test_train_cli_refuses_ms_loss_with_another_mode(tmp_path):
    out = _cli(tmp_path, lambda cfg: cfg.replace("'multi_similarity'", "'semihard'"))
    assert out.returncode != 0
    assert "GENERATOR.ms_loss" in out.stderr and "multi_similarity" in out.stderr and "Epoch 1" not in out.stdout
