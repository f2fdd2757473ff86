"""FastAP and Smooth-AP (ops.fast_ap_loss / ops.smooth_ap_loss, csrc/ap_loss.hip on csrc/pair_loss.h) against the float64 reference
and the a-priori bounds of tests/ap_ref.py, their two forward paths against each other, and inside the training step (eager,
graph-replayed, tools/train.py).

Every check prints its largest error / bound before it asserts ratio < 1.  FastAP's open pairs (ap_ref.open_pairs: at most 1 % of
the off-diagonal pairs, tests/test_ap_ref_cpu.py) are left out of the entry-wise comparison of G and of nothing else.
Largest ratios observed on an MI355X, per group of checks and loss (the gradient's bound is one fp32 rounding of the result, which
a nearest rounding all but reaches):
  grid        fast_ap    open_share 0  G 0.0197  loss 0.0136  grad 0.998
  grid        smooth_ap  G 0.138  rowsum 0.0129  loss 0.0189  grad 0.999
  continuous  fast_ap    open_share 0.00403  G 0.0805  loss 0.00938  grad 0.998
  continuous  smooth_ap  G 0.137  rowsum 0.00134  loss 0.0202  grad 0.998
  negated     fast_ap    open_share 0  G 0.0549  loss 0.000811  grad 0.983
  scaled      fast_ap    open_share 0.00202  G 0.106  loss 0.0139  grad 0.998
  antipodal   fast_ap    open_share 0.00202  G 0.0961  loss 0.000418  grad 0.992
  tau         smooth_ap  G 0.0947  rowsum 0.00479  loss 0.00389  grad 0.979
  duplicates  fast_ap    open_share 0  G 0.0167  loss 0.00162  grad 0.949
  duplicates  smooth_ap  G 0.0848  rowsum 0.0114  loss 0.00107  grad 0.926
  offset      fast_ap    open_share 0  G 0.0197  loss 0.00644  grad 0.98
  offset      smooth_ap  G 0.138  rowsum 0.0118  loss 0.0189  grad 0.999
  k = 65      smooth_ap  G 0.0508  rowsum 0.00243  loss 0.00101  grad 0.953
  backward    fast_ap    grad 0.998
  backward    smooth_ap  grad 0.995
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ap_ref as A
import ms_ref as M
import recipes as R
import supcon_ref as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = 0.75
LOSSES = list(A.LOSSES)
DEFAULTS = dict(fast_ap=dict(bins=10), smooth_ap=dict(temperature=0.01))
PATHS = ["per_class", "similarity_matrix"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(x, p, k, dev, loss, path="auto", g=None, **params):
    from embeddingnet_amd import ops
    xt = x if torch.is_tensor(x) else torch.tensor(x, device=dev)
    xt = xt.detach().requires_grad_(True)
    fn = ops.fast_ap_loss if loss == "fast_ap" else ops.smooth_ap_loss
    mean, counts, gw = fn(xt, p, k, path=path, return_weights=True, **dict(DEFAULTS[loss], **params))
    mean.backward(None if g is None else torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), counts=counts.cpu().numpy(), G=gw.cpu().numpy(), grad=xt.grad.cpu().numpy(),
                mean_t=mean.detach().clone(), counts_t=counts.clone(), G_t=gw, grad_t=xt.grad)


def _grad_rows(n):
    return None if n <= 512 else np.r_[0:96, n // 2:n // 2 + 32, n - 96:n]


@functools.lru_cache(maxsize=8)
def _input(kind, p, k, e):
    return A.make_input(kind, p, k, e)


@functools.lru_cache(maxsize=8)
def _reference(kind, p, k, e, loss, value):
    """One float64 reference per (input, loss, parameter), shared by the paths that are checked against it."""
    x, _ = _input(kind, p, k, e)
    return A.reference(x, p, k, loss, **{("bins" if loss == "fast_ap" else "temperature"): value})


def _gs(path, p, k, e, unit):
    return 0.0 if unit is not None else M.gamma_s(M.auto_path(p, k, e) if path == "auto" else path, e)


def _check(got, x, ref, gs, loss, g=1.0, what="", unit=None, counter=True):
    """Everything the header promises about one forward + backward, for a device whose S is within gs A of the truth: both
    counters (the violating anchors between the sure and the possible count), every entry of G (FastAP: of the pairs that are not
    open, at most 1 % may be), Smooth-AP's row sums of G, the loss and (from the device's own G) every gradient element.
    counter=False leaves the violating anchors to the caller.  -> {check: largest error / bound}."""
    p, k = ref["p"], ref["k"]
    n = p * k
    assert gs > 0 or M.exact_in_any_order(x, unit)                         # gamma_S = 0 only where S is exact in any order
    assert np.isfinite(got["G"]).all() and np.isfinite(got["grad"]).all() and np.isfinite(got["loss"])
    pos, neg = M.class_masks(p, k)
    off = pos | neg
    assert not np.diag(got["G"]).any()
    assert got["counts"].dtype == np.int32 and got["counts"].shape == (2,) and got["counts"][0] == n * (k - 1)
    if counter:
        d = C.decisions(x, p, k, gs)
        assert d["sure"].sum() <= got["counts"][1] <= d["may"].sum(), (got["counts"], d["sure"].sum(), d["may"].sum())
    bg, _, bl, _ = A.bounds(x, ref, gs)
    ratios = {}
    keep = off
    if loss == "fast_ap":
        opened = A.open_pairs(x, p, k, ref["bins"], gs)
        ratios["open_share"] = float(opened.sum() / (n * (n - 1)))
        assert ratios["open_share"] <= A.OPEN_CAP
        keep = off & ~opened
    ratios["G"] = float((np.abs(got["G"] - ref["G"])[keep] / bg[keep]).max())
    if loss == "smooth_ap":
        ratios["rowsum"] = float((np.abs(got["G"].astype(np.float64).sum(1)) / bg.sum(1)).max())     # the true rows sum to zero
    ratios["loss"] = float(abs(got["loss"] - ref["loss"]) / bl)
    rows = _grad_rows(n)
    want, bound = M.grad(x, got["G"], g, rows)
    have = got["grad"] if rows is None else got["grad"][rows]
    ratios["grad"] = float((np.abs(have - want) / bound).max())
    par = f"L={ref['bins']}" if loss == "fast_ap" else f"tau={ref['tau']:.3g}"
    print(f"{loss} {what} {par} p={p} k={k} e={x.shape[1]} viol={got['counts'][1]} loss={got['loss']:.6g}: "
          + " ".join(f"{a}={b:.3g}" for a, b in ratios.items()))
    assert all(v < 1 for name, v in ratios.items() if name != "open_share"), ratios
    return ratios


def _value_case(dev, kind, p, k, e, loss, value, g=UP):
    x, unit = _input(kind, p, k, e)
    ref = _reference(kind, p, k, e, loss, value)
    key = "bins" if loss == "fast_ap" else "temperature"
    out = {}
    for path in A.paths_of(p, k, e):
        got = _run(x, p, k, dev, loss, path=path, g=g, **{key: value})
        _check(got, x, ref, _gs(path, p, k, e, unit), loss, g=g, unit=unit, what=f"{kind} {path}")
        out[path] = got
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("p,k,e", A.SHAPES, ids=str)
def test_values_on_grid_inputs(dev, p, k, e, loss):
    """S is exact in any order (test_ap_ref_cpu.py): gamma_S = 0, no FastAP pair is open, and the forward paths of a shape that
    has both see the same bits."""
    from embeddingnet_amd import _lib
    out = _value_case(dev, "grid", p, k, e, loss, DEFAULTS[loss][("bins" if loss == "fast_ap" else "temperature")])
    if len(out) == 2:
        a, b = out["per_class"], out["similarity_matrix"]
        assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["G"], b["G"]) and np.array_equal(a["grad"], b["grad"])
        assert a["loss"] == b["loss"]
    path_fn = getattr(_lib.lib(), f"embnet_{loss}_loss_path")
    assert path_fn(p, k, e) == (1 if M.auto_path(p, k, e) == "per_class" else 2)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("p,k,e", [s for s in A.SHAPES if s[2] > 1], ids=str)
def test_values_on_continuous_inputs(dev, p, k, e, loss):
    _value_case(dev, "continuous", p, k, e, loss, DEFAULTS[loss][("bins" if loss == "fast_ap" else "temperature")])


@pytest.mark.parametrize("bins", A.CONTINUOUS_BINS)
@pytest.mark.parametrize("p,k,e", A.RANGE_SHAPES, ids=str)
def test_fast_ap_bin_counts(dev, p, k, e, bins):
    """L = 2 (the minimum), 7, and the powers of two 16 and 64 (bin 64 lives in a lane's second slot), on continuous inputs."""
    _value_case(dev, "continuous", p, k, e, "fast_ap", bins)


@pytest.mark.parametrize("kind,bins", [("negated", 10), ("scaled", 10), ("antipodal", 64)])
@pytest.mark.parametrize("p,k,e", A.RANGE_SHAPES, ids=str)
def test_fast_ap_over_the_whole_range_of_distances(dev, p, k, e, kind, bins):
    """negated: the rows of every odd class are negated, d reaches 3.4 and beyond and the top bins of 10 fill.  scaled: every second
    row of norm 1.5 as well, some d below 0 and above 4: what falls outside the bins is dropped, everything stays finite and within bound.
    antipodal: a pair at d = 3.98, between the last two centres of L = 64 (bin 64 is the one bin in a lane's second slot)."""
    ref = _reference(kind, p, k, e, "fast_ap", bins)
    d = 2.0 - 2.0 * ref["S"][~np.eye(p * k, dtype=bool)]
    if kind == "negated":
        assert d.max() > 3.2 and ref["hn"][:, 8:].sum() > 0
    elif kind == "scaled":
        assert d.min() < 0 and d.max() > 4 and np.abs(ref["G"]).max() > 0.01
    else:
        assert (ref["hn"][:, 64] > 0.1).any()
    _value_case(dev, kind, p, k, e, "fast_ap", bins)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("tau", [0.01, 0.1, 10.0])
def test_smooth_ap_temperatures(dev, tau, path):
    """At tau = 0.01 |z| reaches 100 and beyond: e^{-|z|} underflows towards 0, sigma to 0 or 1, nothing overflows."""
    p, k, e = 5, 7, 33
    x, _ = _input("continuous", p, k, e)
    ref = _reference("continuous", p, k, e, "smooth_ap", tau)
    if tau == 0.01:
        assert np.abs(ref["S"][:, :, None] - ref["S"][:, None, :]).max() / A.tau32(tau) > 50
    got = _run(x, p, k, dev, "smooth_ap", path=path, g=UP, temperature=tau)
    _check(got, x, ref, M.gamma_s(path, e), "smooth_ap", g=UP, what="tau " + path)


# ---------------------------------------------------------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("loss", LOSSES)
def test_duplicate_rows(dev, loss):
    """Twins: z = 0 and sigma = 1/2 in Smooth-AP; d ~ 0 in bin 0 in FastAP."""
    p, k, e = A.DUPLICATE_SHAPE
    x, unit = _input("duplicates", p, k, e)
    ref = _reference("duplicates", p, k, e, loss, DEFAULTS[loss]["bins" if loss == "fast_ap" else "temperature"])
    got = _run(x, p, k, dev, loss)
    _check(got, x, ref, 0.0, loss, unit=unit, what="duplicates")
    assert got["counts"][1] > 0                                     # a twin is its twin's hardest positive, the others are not


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("p,k,e,path", [(4, 3, 1, "per_class"), (4, 3, 1, "similarity_matrix"), (5, 7, 33, "similarity_matrix"),
                                        (16, 2, 48, "per_class"), (16, 2, 48, "similarity_matrix"), (3, 16, 40, "per_class"),
                                        (2, 2, 5, "per_class"), (2, 2, 5, "similarity_matrix")], ids=str)
def test_small_and_odd_shapes_from_an_offset_pointer(dev, p, k, e, path, loss):
    """E = 1, E = 33, K = 2, K = 16, N = 4 (the backward's minimum), with the block one float behind a 16-byte boundary (the
    dense GEMM's scalar loader)."""
    x, unit = _input("grid", p, k, e)
    buf = torch.zeros(p * k * e + 1, device=dev)
    xt = buf[1:].view(p * k, e)
    xt.copy_(torch.tensor(x))
    assert xt.data_ptr() % 16 == 4
    got = _run(xt, p, k, dev, loss, path=path, g=UP)
    ref = _reference("grid", p, k, e, loss, DEFAULTS[loss]["bins" if loss == "fast_ap" else "temperature"])
    _check(got, x, ref, 0.0, loss, unit=unit, g=UP, what="offset " + path)


def test_smooth_ap_takes_65_samples_per_class_and_refuses_66(dev):
    from embeddingnet_amd import _lib, ops
    p, k, e = 2, 65, 8
    x, unit = _input("grid", p, k, e)
    got = _run(x, p, k, dev, "smooth_ap", g=UP)
    _check(got, x, _reference("grid", p, k, e, "smooth_ap", 0.01), 0.0, "smooth_ap", unit=unit, g=UP, what="k=65")
    with pytest.raises(_lib.EmbnetError, match="k=66 > 65"):
        ops.smooth_ap_loss(torch.rand((2 * 66, 8), device=dev), 2, 66)
    assert torch.isfinite(ops.fast_ap_loss(torch.rand((2 * 66, 8), device=dev), 2, 66)[0])      # FastAP has no such limit


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("p,k,e", [(1, 4, 16), (4, 1, 16), (2, 2049, 4), (4, 4, 4097), (4, 32, 16)])
def test_out_of_range_arguments_raise(dev, p, k, e, loss):
    from embeddingnet_amd import _lib, ops
    fn = ops.fast_ap_loss if loss == "fast_ap" else ops.smooth_ap_loss
    x = torch.rand((p * k, e), device=dev)
    path = "per_class" if (p, k) == (4, 32) else "auto"
    with pytest.raises(_lib.EmbnetError):
        fn(x, p, k, path=path)
    with pytest.raises(_lib.EmbnetError):
        fn(x, p + 1, k)                                             # rows != p*k
    small = torch.rand((8, 4), device=dev)
    if loss == "fast_ap":
        for bins in (1, 65, 10.5):
            with pytest.raises(_lib.EmbnetError):
                ops.fast_ap_loss(small, 4, 2, bins=bins)
    else:
        for tau in (0.0, -1.0, float("inf")):
            with pytest.raises(_lib.EmbnetError):
                ops.smooth_ap_loss(small, 4, 2, temperature=tau)


def _raw(xt, p, k, loss, path, pad, stream=None, fill_ff=False):
    """The C ABI directly on buffers with `pad` guard elements on either side.  -> (G, demb, counts, mean, ws) guarded tensors."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    n, e = xt.shape
    dev = xt.device
    wsn = getattr(lib, f"embnet_{loss}_loss_workspace_bytes")(p, k, e) // 4
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
    scalar = 10 if loss == "fast_ap" else 0.01
    _lib.check(getattr(lib, f"embnet_{loss}_loss_fwd")(xt.data_ptr(), p, k, e, scalar, path, sl(gb, n * n).data_ptr(),
                                                       sl(cb, 2).data_ptr(), sl(mb, 1).data_ptr(), sl(wb, wsn).data_ptr(), wsn * 4, s))
    _lib.check(lib.embnet_ms_loss_bwd(xt.data_ptr(), n, e, sl(gb, n * n).data_ptr(), up.data_ptr(), sl(db, n * e).data_ptr(), s))
    torch.cuda.synchronize()
    return gb, db, cb, mb, wb


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("path", [1, 2])
def test_nothing_is_written_outside_the_outputs(dev, path, loss):
    p, k, e, pad = 5, 7, 33, 64                                     # N = 35: ragged tiles in every kernel
    x, unit = _input("grid", p, k, e)
    xt = torch.tensor(x, device=dev)
    gb, db, cb, mb, wb = _raw(xt, p, k, loss, path, pad)
    for t in (gb, db, mb, wb):
        assert torch.isnan(t[:pad]).all() and torch.isnan(t[-pad:]).all()
        assert torch.isfinite(t[pad:-pad]).all()                    # all n*n entries of G are written
    assert (cb[:pad] == -12345).all() and (cb[-pad:] == -12345).all()
    assert wb[pad].view(torch.int32).item() == 0                    # the ticket is re-armed
    got = _run(x, p, k, dev, loss, path=PATHS[path - 1], g=UP)
    n = p * k
    assert np.array_equal(gb[pad:-pad].view(n, n).cpu().numpy(), got["G"])
    assert np.array_equal(db[pad:-pad].view(n, e).cpu().numpy(), got["grad"])
    assert np.array_equal(cb[pad:-pad].cpu().numpy(), got["counts"]) and mb[pad].item() == got["loss"]


def test_backward_precision_on_continuous_embeddings(dev):
    """Unquantised embeddings: the gradient from the kernel's own G meets the per-element bound, at two upstream values."""
    p, k, e = 32, 4, 256
    x = R.clustered_embeddings(11, p, k, e, 0.7)
    for loss in LOSSES:
        for g in (None, -3.0):
            got = _run(x, p, k, dev, loss, g=g)
            assert np.abs(got["grad"]).max() > 0
            want, bound = M.grad(x, got["G"], 1.0 if g is None else g)
            ratio = (np.abs(got["grad"] - want) / bound).max()
            print(f"{loss} backward g={g}: grad={ratio:.3g}")
            assert ratio < 1


# ---------------------------------------------------------------------------------------------------------------- 3. reproducible
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("p,k,e", [(32, 4, 256), (256, 8, 128)], ids=str)
def test_bitwise_reproducible(dev, p, k, e, loss):
    x = R.clustered_embeddings(4, p, k, e, 0.7)
    r1, r2 = _run(x, p, k, dev, loss, g=UP), _run(x, p, k, dev, loss, g=UP)
    for key in ("mean_t", "counts_t", "G_t", "grad_t"):
        assert torch.equal(r1[key], r2[key]), key
    # a second stream, its own workspace, a G buffer full of 0xFF bytes
    n = p * k
    s2 = torch.cuda.Stream(device=dev)
    gb, db, cb, mb, _ = _raw(torch.tensor(x, device=dev), p, k, loss, 0, 16, stream=s2, fill_ff=True)
    assert torch.equal(gb[16:-16].view(n, n), r1["G_t"]) and torch.equal(db[16:-16].view(n, e), r1["grad_t"])
    assert torch.equal(cb[16:-16], r1["counts_t"]) and torch.equal(mb[16], r1["mean_t"])


# ---------------------------------------------------------------------------------------------------------------- 4. training
def _trainer(dev, graph, loss, seed=5):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=seed,
                             device=dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-3)
    return base, opt, TripletTrainer(base, opt, 8, 4, negatives_selection_mode=loss, seed=3, graph=graph,
                                     loss_params=DEFAULTS[loss])


def _batches(dev, steps):
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((12, 64, 64, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(12, generator=torch.Generator().manual_seed(i))[:8].to(dev)
        x = protos[cls].repeat_interleave(4, 0) + 0.15 * torch.randn((32, 64, 64, 3), device=dev, generator=gen)
        yield x.clamp(0, 1)


@pytest.mark.parametrize("loss", LOSSES)
def test_trainer_learns(dev, loss):
    _, _, tr = _trainer(dev, graph=False, loss=loss)
    losses, viol = [], []
    for x in _batches(dev, 25):
        losses.append(float(tr.step(x).item()))
        trip, count = tr.last_triplets
        assert trip is None and count.dtype == torch.int32 and count.shape == (1,)
        assert tr.last_pair_counts.shape == (2,) and int(tr.last_pair_counts[1]) == int(count)
        assert int(tr.last_pair_counts[0]) == 32 * 3
        viol.append(int(count))
    print(f"{loss} trainer losses", [round(v, 4) for v in losses], "violating anchors", viol)
    assert np.all(np.isfinite(losses))
    assert max(losses[-5:]) < losses[0], losses


def test_trainer_refuses_parameters_of_another_loss(dev):
    from embeddingnet_amd.train_step import TripletTrainer
    base, opt, _ = _trainer(dev, graph=False, loss="fast_ap")
    with pytest.raises(ValueError):
        TripletTrainer(base, opt, 8, 4, negatives_selection_mode="fast_ap", loss_params=dict(temperature=0.1))
    with pytest.raises(ValueError, match="fast_ap"):
        TripletTrainer(base, opt, 8, 4, negatives_selection_mode="semihard", loss_params=dict(bins=10))


def test_trainer_fast_ap_graph_replay_equals_eager(dev):
    from embeddingnet_amd import _lib
    runs = []
    for graph in (False, True):
        base, opt, tr = _trainer(dev, graph=graph, loss="fast_ap")
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
def _cli(tmp_path, loss, edit):
    cfg = open(os.path.join(ROOT, "configs", f"simple2_{loss}_synthetic.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert f"negatives_selection_mode : '{loss}'" in cfg and "n_batches : 20" in cfg and "ap_loss :" in cfg
    assert "embeddings_normalization: True" in cfg
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(edit(cfg.replace("n_batches : 20", "n_batches : 4")))
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path), "--synthetic", "10",
                           "--max_epochs", "2"], capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("loss", LOSSES)
def test_train_cli_config(tmp_path, loss):
    out = _cli(tmp_path, loss, lambda cfg: cfg)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch 2/2" in out.stdout and "saving model" in out.stdout and " - violating " in out.stdout
    assert any(f.startswith("epoch_") for f in os.listdir(tmp_path / f"simple2_{loss}_synthetic" / "weights"))


def test_train_cli_refuses_ap_loss_with_another_mode(tmp_path):
    out = _cli(tmp_path, "fast_ap", lambda cfg: cfg.replace("'fast_ap'", "'semihard'"))
    assert out.returncode != 0
    assert "GENERATOR.ap_loss" in out.stderr and "fast_ap" in out.stderr and "Epoch 1" not in out.stdout


def test_train_cli_fast_ap_with_a_cross_batch_memory(tmp_path):
    out = _cli(tmp_path, "fast_ap", lambda cfg: cfg.replace("  ap_loss : {bins: 10}", "  ap_loss : {bins: 10}\n  xbm : {size: 64}"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch 2/2" in out.stdout and "xbm_filled" in out.stdout and " - violating " in out.stdout
