"""SupCon / NT-Xent (ops.supcon_loss, csrc/supcon.hip on csrc/pair_loss.h) against the float64 reference and the a-priori bounds of
tests/supcon_ref.py, its two forward paths against each other, and inside the training step (eager, graph-replayed, tools/train.py).

Every check prints its largest error / bound before it asserts ratio < 1.  Largest ratios observed on an MI355X, per group of
checks (the gradient's bound is one fp32 rounding of the result, which a nearest rounding all but reaches;
1 = above 0.9995 and below 1):
  grid               open_share 0  G 0.571  rowsum 0.0345  loss 0.0445  grad 1
  continuous         open_share 0  G 0.23  rowsum 0.00764  loss 0.01  grad 0.999
  per_class          open_share 0  G 0.147  rowsum 0.0264  loss 0.0212  grad 1
  similarity_matrix  open_share 0  G 0.147  rowsum 0.0264  loss 0.0212  grad 1
  backward           grad 0.997
  tau                open_share 0  G 0.398  rowsum 0.0776  loss 0.0875  grad 0.989
  norm 30            open_share 0  G 0.288  rowsum 2.95e-05  loss 0.000451  grad 0.96
  trap               open_share 0  G 0.0937  rowsum 0.000159  loss 0.00167  grad 0.795
  duplicates         open_share 0  G 0.112  rowsum 0.0175  loss 0.0115  grad 0.982
  offset             open_share 0  G 0.242  rowsum 0.0275  loss 0.026  grad 0.994
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ms_ref as M
import recipes as R
import supcon_ref as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = 0.75
DENOMS = list(C.DENOMINATORS)
SHAPES = M.PER_CLASS_SHAPES + C.MATRIX_SHAPES
PATHS = ["per_class", "similarity_matrix"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(x, p, k, dev, tau=0.1, denom="all", path="auto", g=None):
    from embeddingnet_amd import ops
    xt = x if torch.is_tensor(x) else torch.tensor(x, device=dev)
    xt = xt.detach().requires_grad_(True)
    mean, counts, gw = ops.supcon_loss(xt, p, k, tau, denom, path=path, return_weights=True)
    mean.backward(None if g is None else torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), counts=counts.cpu().numpy(), G=gw.cpu().numpy(), grad=xt.grad.cpu().numpy(),
                mean_t=mean.detach().clone(), counts_t=counts.clone(), G_t=gw, grad_t=xt.grad)


def _grad_rows(n):
    return None if n <= 512 else np.r_[0:96, n // 2:n // 2 + 32, n - 96:n]


@functools.lru_cache(maxsize=4)
def _continuous(p, k, e):
    return R.clustered_embeddings(M.seed_of(p, k, e), p, k, e, M.SIGMA)


@functools.lru_cache(maxsize=4)
def _grid(p, k, e, seed=None):
    """-> (x on the 1/q grid: S exact in any order, unit = 1/q)."""
    x, _, q = M.grid_inputs(R.clustered_embeddings(M.seed_of(p, k, e) if seed is None else seed, p, k, e, M.SIGMA))
    return x, 1.0 / q


def _check(got, x, p, k, gs, tau, denom, g=1.0, what="", unit=None, counter=True):
    """Everything the header promises about one forward + backward, for a device whose S is within gs A of the truth: both
    counters (the violating anchors between the sure and the possible count, at most 1 % of the anchors open), every entry of G,
    every row sum of G, the loss and (from the device's own G) every gradient element.  counter=False leaves the violating anchors
    to the caller (an input with exact ties, which any gs > 0 calls open).  -> {check: largest error / bound}."""
    n = p * k
    assert gs > 0 or M.exact_in_any_order(x, unit)                         # gamma_S = 0 only where S is exact in any order
    assert np.isfinite(got["G"]).all() and np.isfinite(got["grad"]).all() and np.isfinite(got["loss"])
    pos, neg = M.class_masks(p, k)
    assert not np.diag(got["G"]).any()
    if denom == "negatives":
        assert np.all(got["G"][pos] <= 0) and np.all(got["G"][neg] >= 0)
    assert got["counts"].dtype == np.int32 and got["counts"].shape == (2,) and got["counts"][0] == n * (k - 1)
    share = 0.0
    if counter:
        d = C.decisions(x, p, k, gs)
        share = d["open"].mean()
        assert share <= 0.01, share
        assert d["sure"].sum() <= got["counts"][1] <= d["may"].sum(), (got["counts"], d["sure"].sum(), d["may"].sum())
    ref = C.reference(x, p, k, tau, denom)
    bg, _, bl = C.bounds(x, ref, gs)
    off = pos | neg
    ratios = dict(open_share=float(share))
    ratios["G"] = float((np.abs(got["G"] - ref["G"])[off] / bg[off]).max())
    ratios["rowsum"] = float((np.abs(got["G"].astype(np.float64).sum(1)) / bg.sum(1)).max())     # the true rows sum to zero
    ratios["loss"] = float(abs(got["loss"] - ref["loss"]) / bl)
    rows = _grad_rows(n)
    want, bound = M.grad(x, got["G"], g, rows)
    have = got["grad"] if rows is None else got["grad"][rows]
    ratios["grad"] = float((np.abs(have - want) / bound).max())
    print(f"supcon {what} {denom} tau={tau} p={p} k={k} e={x.shape[1]} viol={got['counts'][1]}: "
          + " ".join(f"{a}={b:.3g}" for a, b in ratios.items()))
    assert ratios["G"] < 1 and ratios["rowsum"] < 1 and ratios["loss"] < 1 and ratios["grad"] < 1, ratios
    return ratios


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("denom", DENOMS)
@pytest.mark.parametrize("p,k,e", SHAPES, ids=str)
def test_values_on_grid_inputs(dev, p, k, e, denom):
    """S is exact in any order (test_supcon_ref_cpu.py), so the violating-anchor count is exact and gamma_S = 0 in the bounds."""
    from embeddingnet_amd import _lib
    x, unit = _grid(p, k, e)
    got = _run(x, p, k, dev, denom=denom, g=UP)
    r = _check(got, x, p, k, 0.0, 0.1, denom, unit=unit, g=UP, what="grid")
    assert r["open_share"] == 0
    assert _lib.lib().embnet_supcon_loss_path(p, k, e) == (2 if (p, k, e) in C.MATRIX_SHAPES else 1)


@pytest.mark.parametrize("denom", DENOMS)
@pytest.mark.parametrize("p,k,e", SHAPES, ids=str)
def test_values_on_continuous_inputs(dev, p, k, e, denom):
    """No anchor's decision is open at either path's gamma_S (test_supcon_ref_cpu.py): the counter is asserted exactly."""
    x = _continuous(p, k, e)
    got = _run(x, p, k, dev, denom=denom, g=UP)
    r = _check(got, x, p, k, M.gamma_s(M.auto_path(p, k, e), e), 0.1, denom, g=UP, what="continuous")
    assert r["open_share"] == 0 and got["counts"][1] == C.reference(x, p, k, 0.1, denom)["counts"][1]


@pytest.mark.parametrize("denom", DENOMS)
def test_forward_paths_agree_on_a_grid_input(dev, denom):
    """The two paths differ in how S is summed; on an exact S the per-anchor body sees the same bits."""
    p, k, e = 8, 4, 256
    x, unit = _grid(p, k, e, seed=5)
    a = _run(x, p, k, dev, denom=denom, path="per_class")
    b = _run(x, p, k, dev, denom=denom, path="similarity_matrix")
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["G"], b["G"]) and np.array_equal(a["grad"], b["grad"])
    _check(a, x, p, k, 0.0, 0.1, denom, unit=unit, what="per_class")
    _check(b, x, p, k, 0.0, 0.1, denom, unit=unit, what="similarity_matrix")


def test_backward_precision_on_continuous_embeddings(dev):
    """Unquantised C2 embeddings: the gradient from the kernel's own G meets the per-element bound, at two upstream values."""
    p, k, e = 32, 4, 256
    x = R.clustered_embeddings(11, p, k, e, 0.7)
    for denom in DENOMS:
        for g in (None, -3.0):
            got = _run(x, p, k, dev, denom=denom, g=g)
            assert np.abs(got["grad"]).max() > 0
            want, bound = M.grad(x, got["G"], 1.0 if g is None else g)
            ratio = (np.abs(got["grad"] - want) / bound).max()
            print(f"supcon backward {denom} g={g}: grad={ratio:.3g}")
            assert ratio < 1


@pytest.mark.parametrize("denom", DENOMS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("tau", [0.01, 0.1, 100.0])
def test_temperatures(dev, tau, path, denom):
    p, k, e = 5, 7, 33
    x = _continuous(p, k, e)
    got = _run(x, p, k, dev, tau=tau, denom=denom, path=path, g=UP)
    _check(got, x, p, k, M.gamma_s(path, e), tau, denom, g=UP, what="tau " + path)


# ---------------------------------------------------------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("denom", DENOMS)
@pytest.mark.parametrize("path", PATHS)
def test_unnormalised_rows_of_norm_30_stay_finite_and_within_bounds(dev, path, denom):
    """t = S / 0.1 reaches 7800 and spans 3400: e^t overflows fp32 above 88 and float64 above 709, so the plain formulas overflow
    and a maximum taken over the wrong set underflows; the stable forms do neither."""
    p, k, e = 6, 4, 64
    x, unit = _grid(p, k, e, seed=3)
    x = (x * np.float32(30.0)).astype(np.float32)                   # still exact: S q^2 / 900 is an integer below 2^24 / 900
    ref = C.reference(x, p, k, 0.1, denom)
    t = ref["t"][~np.eye(p * k, dtype=bool)]
    assert t.max() > 709 and np.ptp(t) > 709 and np.isfinite(ref["loss"])
    got = _run(x, p, k, dev, denom=denom, path=path)
    _check(got, x, p, k, 0.0, 0.1, denom, unit=30.0 * unit, what="norm 30 " + path)


@pytest.mark.parametrize("path", PATHS)
def test_negatives_takes_its_maximum_per_pair(dev, path):
    """supcon_ref.underflow_trap: logits 200 / 40 / 0.  One maximum per anchor underflows d of the pair (0, 2) to 0 and gives
    -inf; the loss must be finite and within bound ('all' runs on the same rows).  The counter by hand: every off-diagonal S is
    ONE product by 1 or by 0, exact on either path; the classes on (0,1) meet each other's rows at S = 1 = their own positives
    (>=: violating), the trap class's negatives are at 0 below its positives at 0.2 and 1."""
    x, p, k = C.underflow_trap()
    for denom in ("negatives", "all"):
        got = _run(x, p, k, dev, tau=C.TRAP_TAU, denom=denom, path=path, g=UP)
        assert np.isfinite(got["loss"]) and got["loss"] > 0
        _check(got, x, p, k, M.gamma_s(path, 2), C.TRAP_TAU, denom, g=UP, what="trap " + path, counter=False)
        assert got["counts"][1] == k * (p - 1)


@pytest.mark.parametrize("denom", DENOMS)
def test_duplicate_rows(dev, denom):
    p, k, e = 5, 4, 32
    x, unit = _grid(p, k, e, seed=8)
    x = x.copy()
    x[1::k] = x[0::k]                                               # rows 0 and 1 of every class coincide
    got = _run(x, p, k, dev, denom=denom)
    _check(got, x, p, k, 0.0, 0.1, denom, unit=unit, what="duplicates")
    assert got["counts"][1] > 0                                     # a twin is its twin's hardest positive, the others are not


@pytest.mark.parametrize("denom", DENOMS)
@pytest.mark.parametrize("p,k,e,path", [(4, 3, 1, "per_class"), (4, 3, 1, "similarity_matrix"), (5, 7, 33, "similarity_matrix"),
                                        (16, 2, 48, "per_class"), (16, 2, 48, "similarity_matrix"), (3, 16, 40, "per_class"),
                                        (2, 2, 5, "per_class"), (2, 2, 5, "similarity_matrix")], ids=str)
def test_small_and_odd_shapes_from_an_offset_pointer(dev, p, k, e, path, denom):
    """E = 1, E = 33, K = 2, K = 16, N = 4 (the backward's minimum), with the block one float behind a 16-byte boundary (the
    dense GEMM's scalar loader)."""
    x, unit = _grid(p, k, e)
    buf = torch.zeros(p * k * e + 1, device=dev)
    xt = buf[1:].view(p * k, e)
    xt.copy_(torch.tensor(x))
    assert xt.data_ptr() % 16 == 4
    got = _run(xt, p, k, dev, denom=denom, path=path, g=UP)
    _check(got, x, p, k, 0.0, 0.1, denom, unit=unit, g=UP, what="offset " + path)


@pytest.mark.parametrize("p,k,e", [(1, 4, 16), (4, 1, 16), (2, 2049, 4), (4, 4, 4097), (4, 32, 16)])
def test_out_of_range_arguments_raise(dev, p, k, e):
    from embeddingnet_amd import _lib, ops
    x = torch.rand((p * k, e), device=dev)
    path = "per_class" if (p, k) == (4, 32) else "auto"
    with pytest.raises(_lib.EmbnetError):
        ops.supcon_loss(x, p, k, path=path)
    with pytest.raises(_lib.EmbnetError):
        ops.supcon_loss(x, p + 1, k)                                # rows != p*k
    with pytest.raises(_lib.EmbnetError):
        ops.supcon_loss(torch.rand((8, 4), device=dev), 4, 2, temperature=0.0)
    with pytest.raises(_lib.EmbnetError):
        ops.supcon_loss(torch.rand((8, 4), device=dev), 4, 2, denominator="positives")


def _raw(xt, p, k, denom, path, pad, stream=None, fill_ff=False):
    """The C ABI directly on buffers with `pad` guard elements on either side.  -> (G, demb, counts, mean, ws) guarded tensors."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    n, e = xt.shape
    dev = xt.device
    wsn = lib.embnet_supcon_loss_workspace_bytes(p, k, e) // 4
    gb = torch.full((2 * pad + n * n,), float("nan"), device=dev)
    if fill_ff:
        gb.view(torch.int32).fill_(-1)                              # 0xFF bytes
    db = torch.full((2 * pad + n * e,), float("nan"), device=dev)
    cb = torch.full((2 * pad + 2,), -12345, dtype=torch.int32, device=dev)
    mb = torch.full((2 * pad + 1,), float("nan"), device=dev)
    wb = torch.full((2 * pad + wsn,), float("nan"), device=dev)
    wb[pad:pad + wsn] = 0
    up = torch.tensor(UP, device=dev)
    torch.cuda.synchronize()
    s = _lib.stream() if stream is None else stream.cuda_stream
    sl = lambda t, m: t[pad:pad + m]
    _lib.check(lib.embnet_supcon_loss_fwd(xt.data_ptr(), p, k, e, 0.1, {"all": 1, "negatives": 2}[denom], path,
                                          sl(gb, n * n).data_ptr(), sl(cb, 2).data_ptr(), sl(mb, 1).data_ptr(),
                                          sl(wb, wsn).data_ptr(), wsn * 4, s))
    _lib.check(lib.embnet_ms_loss_bwd(xt.data_ptr(), n, e, sl(gb, n * n).data_ptr(), up.data_ptr(), sl(db, n * e).data_ptr(), s))
    torch.cuda.synchronize()
    return gb, db, cb, mb, wb


@pytest.mark.parametrize("denom", DENOMS)
@pytest.mark.parametrize("path", [1, 2])
def test_nothing_is_written_outside_the_outputs(dev, path, denom):
    p, k, e, pad = 5, 7, 33, 64                                     # N = 35: ragged tiles in every kernel
    x, unit = _grid(p, k, e)
    xt = torch.tensor(x, device=dev)
    gb, db, cb, mb, wb = _raw(xt, p, k, denom, path, pad)
    for t in (gb, db, mb, wb):
        assert torch.isnan(t[:pad]).all() and torch.isnan(t[-pad:]).all()
        assert torch.isfinite(t[pad:-pad]).all()                    # all n*n entries of G are written
    assert (cb[:pad] == -12345).all() and (cb[-pad:] == -12345).all()
    assert wb[pad].view(torch.int32).item() == 0                    # the ticket is re-armed
    got = _run(x, p, k, dev, denom=denom, path=PATHS[path - 1], g=UP)
    n = p * k
    assert np.array_equal(gb[pad:-pad].view(n, n).cpu().numpy(), got["G"])
    assert np.array_equal(db[pad:-pad].view(n, e).cpu().numpy(), got["grad"])
    assert np.array_equal(cb[pad:-pad].cpu().numpy(), got["counts"]) and mb[pad].item() == got["loss"]


# ---------------------------------------------------------------------------------------------------------------- 3. reproducible
@pytest.mark.parametrize("denom", DENOMS)
@pytest.mark.parametrize("p,k,e", [(32, 4, 256), (256, 8, 128)], ids=str)
def test_bitwise_reproducible(dev, p, k, e, denom):
    x = R.clustered_embeddings(4, p, k, e, 0.7)
    r1, r2 = _run(x, p, k, dev, denom=denom, g=UP), _run(x, p, k, dev, denom=denom, g=UP)
    for key in ("mean_t", "counts_t", "G_t", "grad_t"):
        assert torch.equal(r1[key], r2[key]), key
    # a second stream, its own workspace, a G buffer full of 0xFF bytes
    n = p * k
    s2 = torch.cuda.Stream(device=dev)
    gb, db, cb, mb, _ = _raw(torch.tensor(x, device=dev), p, k, denom, 0, 16, stream=s2, fill_ff=True)
    assert torch.equal(gb[16:-16].view(n, n), r1["G_t"]) and torch.equal(db[16:-16].view(n, e), r1["grad_t"])
    assert torch.equal(cb[16:-16], r1["counts_t"]) and torch.equal(mb[16], r1["mean_t"])


# ---------------------------------------------------------------------------------------------------------------- 4. training
def _trainer(dev, graph, denom="all", seed=5):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=seed,
                             device=dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-3)
    return base, opt, TripletTrainer(base, opt, 8, 4, negatives_selection_mode="supcon", seed=3, graph=graph,
                                     loss_params=dict(denominator=denom))


def _batches(dev, steps):
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((12, 64, 64, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(12, generator=torch.Generator().manual_seed(i))[:8].to(dev)
        x = protos[cls].repeat_interleave(4, 0) + 0.15 * torch.randn((32, 64, 64, 3), device=dev, generator=gen)
        yield x.clamp(0, 1)


@pytest.mark.parametrize("denom", DENOMS)
def test_trainer_supcon_learns(dev, denom):
    _, _, tr = _trainer(dev, graph=False, denom=denom)
    losses, viol = [], []
    for x in _batches(dev, 25):
        losses.append(float(tr.step(x).item()))
        trip, count = tr.last_triplets
        assert trip is None and count.dtype == torch.int32 and count.shape == (1,)
        assert tr.last_pair_counts.shape == (2,) and int(tr.last_pair_counts[1]) == int(count)
        assert int(tr.last_pair_counts[0]) == 32 * 3
        viol.append(int(count))
    print(f"supcon trainer {denom} losses", [round(v, 4) for v in losses], "violating anchors", viol)
    assert np.all(np.isfinite(losses))
    assert max(losses[-5:]) < losses[0], losses


def test_trainer_supcon_graph_replay_equals_eager(dev):
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
            assert tr.last_triplets[1].data_ptr() == tr.last_pair_counts.data_ptr() + 4
            counts.append(tr.last_pair_counts.clone())
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        runs.append((torch.stack(losses), torch.stack(counts), torch.cat([q.detach().reshape(-1) for q in base.parameters()])))
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0] - runs[1][0]).abs().max()
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])


# ---------------------------------------------------------------------------------------------------------------- 5. CLI
def _cli(tmp_path, edit):
    cfg = open(os.path.join(ROOT, "configs", "simple2_supcon_synthetic.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert "negatives_selection_mode : 'supcon'" in cfg and "n_batches : 20" in cfg and "supcon_loss :" in cfg
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(edit(cfg.replace("n_batches : 20", "n_batches : 4")))
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path), "--synthetic", "10",
                           "--max_epochs", "2"], capture_output=True, text=True, timeout=600)


def test_train_cli_supcon_config(tmp_path):
    out = _cli(tmp_path, lambda cfg: cfg)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch 2/2" in out.stdout and "saving model" in out.stdout
    assert any(f.startswith("epoch_") for f in os.listdir(tmp_path / "simple2_supcon_synthetic" / "weights"))


def test_train_cli_refuses_supcon_loss_with_another_mode(tmp_path):
    out = _cli(tmp_path, lambda cfg: cfg.replace("'supcon'", "'semihard'"))
    assert out.returncode != 0
    assert "GENERATOR.supcon_loss" in out.stderr and "supcon" in out.stderr and "Epoch 1" not in out.stdout
