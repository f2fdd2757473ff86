"""Proxy-Anchor and CosFace / NormSoftmax (ops.proxy_anchor_loss, ops.proxy_softmax_loss, csrc/proxy_loss.hip) against the float64
reference and the a-priori bounds of tests/proxy_ref.py, the two forward paths against each other, and inside the training step
(train_step.ProxyTrainer: eager and graph-replayed), Feeder.next_labelled() on the file-backed input pipelines, and tools/train.py
(checkpoints, resume, refusals, two ranks).

Every check prints its largest error / bound before it asserts ratio < 1.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import proxy_ref as P
import recipes as R

pytestmark = pytest.mark.gpu
UP = 0.75
KINDS = list(P.KINDS)
KIND_CODE = {"anchor": 1, "softmax": 2}
PATH_CODE = {"auto": 0, "small": 1, "matrix": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _fn(kind):
    from embeddingnet_amd import ops
    return ops.proxy_anchor_loss if kind == "anchor" else ops.proxy_softmax_loss


def _run(kind, x, w, lab, dev, a=None, b=None, path="auto", g=None):
    a, b = P.params32(kind, a, b)
    xt = torch.tensor(x, device=dev).requires_grad_(True)
    wt = torch.tensor(w, device=dev).requires_grad_(True)
    mean, counts, gw = _fn(kind)(xt, wt, torch.tensor(lab, device=dev), a, b, path=path, return_weights=True)
    mean.backward(None if g is None else torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), counts=counts.cpu().numpy(), G=gw.cpu().numpy(), demb=xt.grad.cpu().numpy(),
                dw=wt.grad.cpu().numpy(), t=(mean.detach().clone(), counts.clone(), gw, xt.grad, wt.grad))


def _q(w, dev):
    """The device's q through the C ABI's forward (ops keeps it to itself)."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    c, e = w.shape
    n = 2
    wt, xt = torch.tensor(w, device=dev), torch.zeros((n, e), device=dev)
    lab = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = torch.zeros(lib.embnet_proxy_loss_workspace_bytes(n, c, e) // 8, dtype=torch.float64, device=dev)
    g, q = torch.empty(n * c, device=dev), torch.empty(c, device=dev)
    cnt, mean = torch.empty(3, dtype=torch.int32, device=dev), torch.empty((), device=dev)
    _lib.check(lib.embnet_proxy_loss_fwd(xt.data_ptr(), wt.data_ptr(), lab.data_ptr(), n, c, e, 1, 32.0, 0.1, 0, g.data_ptr(),
                                         q.data_ptr(), cnt.data_ptr(), mean.data_ptr(), ws.data_ptr(), ws.numel() * 8, _lib.stream()))
    torch.cuda.synchronize()
    return q.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(shape, grid):
    """-> (x, w, labels, unit or None), shared by the tests and left unchanged."""
    if shape == "ragged":
        e, c = P.RAGGED
        x, w, lab = P.ragged_inputs(R.clustered_embeddings(77, 5, 5, e, P.SIGMA), e, c, 77)
    else:
        p, k, e, c = shape
        x, w, lab = P.make_inputs(R.clustered_embeddings(P.seed_of(p, k, e), p, k, e, P.SIGMA), p, k, c, P.seed_of(p, k, e))
    unit = None
    if grid:
        x, w, unit = P.to_grid(x, w)
    for t in (x, w, lab):
        t.setflags(write=False)
    return x, w, lab, unit


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, grid):
    x, w, lab, _ = _inputs(shape, grid)
    return P.reference(kind, x, w, lab)


def _check(kind, got, x, w, lab, gs, a=None, b=None, g=1.0, what="", unit=None, ref=None, q_dev=None):
    """Everything the header promises about one forward + backward, for a device whose D is within gs A of the truth: the three
    counters (the violating anchors between the sure and the possible count, exact where nothing is open; at most 1 % open), every
    entry of G, the loss, and (from the device's own G and q) every element of demb and dproxies.  -> {check: largest error / bound}."""
    n, c = x.shape[0], w.shape[0]
    assert gs > 0 or P.exact_in_any_order(x, w, unit)                   # gamma_S = 0 only where D is exact in any order
    for key in ("G", "demb", "dw"):
        assert np.isfinite(got[key]).all(), key
    assert np.isfinite(got["loss"])
    ref = P.reference(kind, x, w, lab, a, b) if ref is None else ref
    assert got["G"].shape == ((c, n) if kind == "anchor" else (n, c))
    assert got["counts"].dtype == np.int32 and got["counts"].shape == (3,)
    assert got["counts"][0] == ref["counts"][0] and got["counts"][1] == ref["counts"][1], (got["counts"], ref["counts"])
    d = P.decisions(kind, x, w, lab, gs)
    share = float(d["open"].mean())
    assert share <= 0.01, share
    assert d["sure"].sum() <= got["counts"][2] <= d["may"].sum(), (got["counts"], d["sure"].sum(), d["may"].sum())
    if share == 0:
        assert got["counts"][2] == ref["counts"][2], (got["counts"], ref["counts"])
    bg, bl = P.bounds(ref, gs)
    zero = bg == 0                                                      # outside every set, unlabelled rows / columns
    assert not got["G"][zero].any()
    ratios = dict(open_share=share)
    ratios["G"] = float((np.abs(got["G"] - ref["G"])[~zero] / bg[~zero]).max()) if (~zero).any() else 0.0
    ratios["loss"] = float(abs(got["loss"] - ref["loss"]) / bl)
    q = ref["q"] if q_dev is None else q_dev
    demb, b_emb, dw, b_w = P.grads(kind, x, w, got["G"], q, g)
    ratios["demb"] = float((np.abs(got["demb"] - demb) / b_emb).max())
    ratios["dproxies"] = float((np.abs(got["dw"] - dw) / b_w).max())
    unl = ~ref["labelled"]
    assert not got["demb"][unl].any()                                   # an unlabelled sample receives no gradient
    assert not got["dw"][ref["q"] == 0].any()                           # a zero proxy neither
    print(f"proxy {what} {kind} n={n} c={c} e={x.shape[1]} counts={got['counts']}: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    assert all(ratios[k] < 1 for k in ("G", "loss", "demb", "dproxies")), ratios
    return ratios


def _n_of(shape):
    return 17 if shape == "ragged" else shape[0] * shape[1]


def _gs(shape, path="auto"):
    e, c = P.RAGGED if shape == "ragged" else shape[2:]
    return P.gamma_s(P.auto_path(_n_of(shape), c, e) if path == "auto" else path, e)


ALL_SHAPES = P.SHAPES + ["ragged"]


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_values_on_grid_inputs(dev, shape, kind):
    x, w, lab, unit = _inputs(shape, True)
    q = _q(w, dev)
    assert np.array_equal(q, P.q_of(w))                                 # q is reproduced bit for bit
    ref = _reference(kind, shape, True)
    for g in (None, UP):
        _check(kind, _run(kind, x, w, lab, dev, g=g), x, w, lab, 0.0, g=1.0 if g is None else g, what="grid", unit=unit, ref=ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_values_on_continuous_inputs(dev, shape, kind):
    x, w, lab, _ = _inputs(shape, False)
    q = _q(w, dev)
    assert np.array_equal(q, P.q_of(w))
    ref = _reference(kind, shape, False)
    for g in (None, UP):
        _check(kind, _run(kind, x, w, lab, dev, g=g), x, w, lab, _gs(shape), g=1.0 if g is None else g, what="continuous", ref=ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(32, 4, 256, 100), (5, 7, 33, 70), (4, 4, 64, 2), "ragged"], ids=str)
def test_forward_paths_agree_on_a_grid_input(dev, shape, kind):
    x, w, lab, unit = _inputs(shape, True)
    assert P.exact_in_any_order(x, w, unit)
    r1, r2 = _run(kind, x, w, lab, dev, path="small", g=UP), _run(kind, x, w, lab, dev, path="matrix", g=UP)
    for a, b in zip(r1["t"][1:], r2["t"][1:]):                          # counts, G, demb, dproxies: bit-equal
        assert torch.equal(a, b)
    assert r1["loss"] == r2["loss"]
    _check(kind, r2, x, w, lab, 0.0, g=UP, what="matrix path", unit=unit)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["small", "matrix"])
def test_both_paths_on_a_continuous_input(dev, path, kind):
    shape = (32, 4, 256, 100)
    x, w, lab, _ = _inputs(shape, False)
    _check(kind, _run(kind, x, w, lab, dev, path=path), x, w, lab, _gs(shape, path), what=path, ref=_reference(kind, shape, False))


# ---------------------------------------------------------------------------------------------------------------- 2. traps
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["small", "matrix"])
def test_unnormalised_rows_of_norm_30_stay_finite_and_within_bounds(dev, path, kind):
    shape = (8, 4, 256, 24)
    x, w, lab, _ = _inputs(shape, False)
    x = (30.0 * x).astype(np.float32)
    got = _run(kind, x, w, lab, dev, path=path, g=UP)
    assert np.isfinite(got["loss"])
    _check(kind, got, x, w, lab, _gs(shape, path), g=UP, what="norm 30 " + path)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["small", "matrix"])
def test_a_logit_spread_of_200_takes_no_log_of_zero(dev, path, kind):
    x, w, lab, a = P.underflow_trap()
    got = _run(kind, x, w, lab, dev, a=a, b=0.0, path=path)
    assert np.isfinite(got["loss"]) and got["loss"] > 0
    _check(kind, got, x, w, lab, P.gamma_s(path, 3), a=a, b=0.0, what="trap " + path)


@pytest.mark.parametrize("kind", KINDS)
def test_a_zero_proxy_has_zero_similarity_and_no_gradient(dev, kind):
    x, w, lab, unit = _inputs((8, 4, 256, 24), True)
    w = w.copy()
    w[int(lab[0])] = 0                                                  # a present class's proxy
    w[int(np.setdiff1d(np.arange(24), lab)[0])] = 0                     # and an absent one's
    assert (P.q_of(w) == 0).sum() == 2 and np.array_equal(_q(w, dev), P.q_of(w))
    got = _run(kind, x, w, lab, dev, g=UP)
    _check(kind, got, x, w, lab, 0.0, g=UP, what="zero proxy", unit=unit)
    assert not got["dw"][P.q_of(w) == 0].any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["small", "matrix"])
def test_all_unlabelled_gives_zero_loss_and_zero_weights(dev, path, kind):
    x, w, lab, unit = _inputs((8, 4, 256, 24), True)
    lab = np.where(np.arange(32) % 2 == 0, -1, 24).astype(np.int32)
    lab[3], lab[5] = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    got = _run(kind, x, w, lab, dev, path=path, g=UP)
    assert got["loss"] == 0.0 and not got["G"].any() and not got["demb"].any() and not got["dw"].any()
    assert got["counts"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("kind", KINDS)
def test_out_of_range_arguments_raise(dev, kind):
    from embeddingnet_amd._lib import EmbnetError
    x, w, lab = torch.rand((8, 4), device=dev), torch.rand((3, 4), device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(EmbnetError, match="proxy_loss_fwd"):
        _fn(kind)(x, w, lab, -1.0, 0.1)
    with pytest.raises(EmbnetError, match="proxy_loss_fwd"):
        _fn(kind)(x[:1], w, lab[:1])
    with pytest.raises(EmbnetError, match="labels"):
        _fn(kind)(x, w, lab.long())
    with pytest.raises(EmbnetError, match="path"):
        _fn(kind)(x, w, lab, path="per_class")
    with pytest.raises(EmbnetError, match="width"):
        _fn(kind)(x, torch.rand((3, 5), device=dev), lab)


# ---------------------------------------------------------------------------------------------------------------- 3. reproducible
def _raw(kind, x, w, lab, dev, path, pad, ws=None, fill_ff=False):
    """The C ABI directly on buffers with `pad` guard elements on either side.  -> (G, demb, dproxies, q, counts, mean, ws)."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    (n, e), c = x.shape, w.shape[0]
    xt, wt, lt = torch.tensor(x, device=dev), torch.tensor(w, device=dev), torch.tensor(lab, device=dev)
    wsn = lib.embnet_proxy_loss_workspace_bytes(n, c, e) // 4
    nan = float("nan")
    gb, db, pb = (torch.full((2 * pad + m,), nan, device=dev) for m in (n * c, n * e, c * e))
    qb, mb = torch.full((2 * pad + c,), nan, device=dev), torch.full((2 * pad + 1,), nan, device=dev)
    if fill_ff:
        gb.view(torch.int32).fill_(-1)                                  # 0xFF bytes
    cb = torch.full((2 * pad + 3,), -12345, dtype=torch.int32, device=dev)
    if ws is None:
        ws = torch.full((2 * pad + wsn,), nan, device=dev)
        ws[pad:pad + wsn] = 0
    up = torch.tensor(UP, device=dev)
    sl = lambda t, m: t[pad:pad + m].data_ptr()
    a, b = P.params32(kind)
    s = _lib.stream()
    _lib.check(lib.embnet_proxy_loss_fwd(xt.data_ptr(), wt.data_ptr(), lt.data_ptr(), n, c, e, KIND_CODE[kind], a, b, path,
                                         sl(gb, n * c), sl(qb, c), sl(cb, 3), sl(mb, 1), sl(ws, wsn), wsn * 4, s))
    _lib.check(lib.embnet_proxy_loss_bwd(xt.data_ptr(), wt.data_ptr(), n, c, e, KIND_CODE[kind], sl(gb, n * c), sl(qb, c),
                                         up.data_ptr(), sl(db, n * e), sl(pb, c * e), sl(ws, wsn), wsn * 4, s))
    torch.cuda.synchronize()
    return gb, db, pb, qb, cb, mb, ws


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", [1, 2])
def test_nothing_is_written_outside_the_outputs_and_the_ticket_is_rearmed(dev, path, kind):
    shape, pad = (5, 7, 33, 70), 64                                     # n = 35, c = 70, e = 33: ragged tiles in every kernel
    x, w, lab, _ = _inputs(shape, True)
    first = _raw(kind, x, w, lab, dev, path, pad)
    second = _raw(kind, x, w, lab, dev, path, pad, ws=first[-1])        # back to back on ONE workspace
    got = _run(kind, x, w, lab, dev, path=["small", "matrix"][path - 1], g=UP)
    for out in (first, second):
        gb, db, pb, qb, cb, mb, ws = out
        for t in (gb, db, pb, qb, mb, ws):
            assert torch.isnan(t[:pad]).all() and torch.isnan(t[-pad:]).all()
        for t in (gb, db, pb, qb, mb):
            assert torch.isfinite(t[pad:-pad]).all()                    # every entry is written
        assert (cb[:pad] == -12345).all() and (cb[-pad:] == -12345).all()
        assert ws[pad].view(torch.int32).item() == 0                    # the ticket is re-armed
        assert np.array_equal(gb[pad:-pad].cpu().numpy(), got["G"].reshape(-1))
        assert np.array_equal(db[pad:-pad].cpu().numpy(), got["demb"].reshape(-1))
        assert np.array_equal(pb[pad:-pad].cpu().numpy(), got["dw"].reshape(-1))
        assert np.array_equal(cb[pad:-pad].cpu().numpy(), got["counts"]) and mb[pad].item() == got["loss"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(32, 4, 256, 100), (128, 4, 257, 256)], ids=str)
def test_bitwise_reproducible(dev, shape, kind):
    x, w, lab, _ = _inputs(shape, False)
    r1, r2 = _run(kind, x, w, lab, dev, g=UP), _run(kind, x, w, lab, dev, g=UP)
    for a, b in zip(r1["t"], r2["t"]):
        assert torch.equal(a, b)
    gb, db, pb, _, cb, mb, _ = _raw(kind, x, w, lab, dev, 0, 16, fill_ff=True)     # its own workspace, a G buffer of 0xFF bytes
    assert torch.equal(gb[16:-16], r1["t"][2].reshape(-1)) and torch.equal(db[16:-16], r1["t"][3].reshape(-1))
    assert torch.equal(pb[16:-16], r1["t"][4].reshape(-1)) and torch.equal(cb[16:-16], r1["t"][1]) and torch.equal(mb[16], r1["t"][0])


# ---------------------------------------------------------------------------------------------------------------- 4. training
N_CLASSES = 12


def _trainer(dev, graph, loss, seed=5):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.proxies import ProxyHead
    from embeddingnet_amd.train_step import ProxyTrainer
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=seed,
                             device=dev)
    head = ProxyHead(N_CLASSES, 64, seed=1).to(dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad] + [head.proxies], "adam", 1e-3)
    return base, head, opt, ProxyTrainer(base, head, opt, loss=loss, seed=3, graph=graph)


def _batches(dev, steps, classes=N_CLASSES):
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((N_CLASSES, 64, 64, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(classes, generator=torch.Generator().manual_seed(i))[:8].to(dev)
        x = protos[cls].repeat_interleave(4, 0) + 0.15 * torch.randn((32, 64, 64, 3), device=dev, generator=gen)
        yield x.clamp(0, 1), cls.repeat_interleave(4).to(torch.int32)


@pytest.mark.parametrize("loss", ["proxy_anchor", "proxy_softmax"])
def test_trainer_learns(dev, loss):
    _, _, _, tr = _trainer(dev, graph=False, loss=loss)
    losses, viol = [], []
    for x, y in _batches(dev, 60):
        losses.append(float(tr.step(x, y).item()))
        trip, count = tr.last_triplets
        assert trip is None and count.dtype == torch.int32 and count.shape == (1,)
        assert tr.last_pair_counts.shape == (3,) and int(tr.last_pair_counts[2]) == int(count)
        assert int(tr.last_pair_counts[0]) == (8 if loss == "proxy_anchor" else 32) and int(tr.last_pair_counts[1]) == 32
        viol.append(int(count))
    print(f"{loss} trainer losses", [round(v, 4) for v in losses], "violating anchors", viol)
    assert np.all(np.isfinite(losses))
    assert max(losses[-5:]) < losses[0], losses
    assert min(viol) < viol[0], viol                                    # the violating anchors reach a lower value


@pytest.mark.parametrize("loss", ["proxy_anchor", "proxy_softmax"])
def test_trainer_graph_replay_equals_eager(dev, loss):
    from embeddingnet_amd import _lib
    runs = []
    for graph in (False, True):
        base, head, opt, tr = _trainer(dev, graph=graph, loss=loss)
        losses, counts = [], []
        for i, (x, y) in enumerate(_batches(dev, 14)):
            if graph and i == 11:
                _lib.trace_enable(True)                                 # an eager step between replays
            losses.append(tr.step(x, y).clone())
            _lib.trace_enable(False)
            assert tr.last_triplets[1].data_ptr() == tr.last_pair_counts.data_ptr() + 8
            counts.append(tr.last_pair_counts.clone())
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        runs.append((torch.stack(losses), torch.stack(counts), head.proxies.detach().clone(),
                     torch.cat([q.detach().reshape(-1) for q in base.parameters()])))
    for a, b in zip(*runs):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()


def test_the_proxies_move_and_an_absent_class_moves_by_the_negative_term_only(dev):
    """Plain SGD on an identity backbone, so that an update IS -lr times the loss's gradient on known embeddings: a present class's
    proxy moves; an absent class's row of G has no negative entry (no positive term), and its update is -lr dproxies of that row.
    Bound: proxy_ref.grads' for the gradient, times lr, plus the roundings of lr g and of w - lr g in fp32."""
    from embeddingnet_amd import ops
    from embeddingnet_amd.proxies import ProxyHead
    from embeddingnet_amd.train_step import ProxyTrainer
    head = ProxyHead(N_CLASSES, 64, seed=1).to(dev)
    lr = 0.05
    opt = torch.optim.SGD([head.proxies], lr=lr)
    tr = ProxyTrainer(torch.nn.Identity(), head, opt, loss="proxy_anchor", graph=False)
    x = torch.tensor(R.clustered_embeddings(11, 8, 4, 64, P.SIGMA), device=dev)
    y = torch.arange(8, dtype=torch.int32, device=dev).repeat_interleave(4)           # classes 8 .. 11 are absent
    w0 = head.proxies.detach().clone()
    _, counts, g = ops.proxy_anchor_loss(x, w0, y, return_weights=True)
    assert counts.tolist()[:2] == [8, 32]
    tr.step(x, y)
    dw = (head.proxies.detach().double() - w0.double()).cpu().numpy()
    gn, w0n = g.cpu().numpy(), w0.cpu().numpy()
    assert (np.linalg.norm(dw, axis=1) > 0).all()                       # every proxy moves, the present ones included
    assert (gn[8:] >= 0).all() and (gn[8:] > 0).any(1).all() and (gn[:8] < 0).any(1).all()
    _, _, want, bound = P.grads("anchor", x.cpu().numpy(), w0n, gn, P.q_of(w0n))
    tol = lr * bound + P.U * (2 * lr * np.abs(want) + np.abs(w0n) + np.abs(w0n - lr * want))
    ratio = float((np.abs(dw + lr * want) / tol).max())
    print("proxy update vs -lr dproxies: error / bound", ratio)
    assert ratio < 1


# ---------------------------------------------------------------------------------------------------------------- 4b. labelled batches
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """6 classes x 9 JPEG / PNG files of 40x33 random pixels (the tree of tests/test_input_pipeline_gpu.py)."""
    from PIL import Image
    root = tmp_path_factory.mktemp("images")
    rs = np.random.RandomState(0)
    for ci in range(6):
        os.makedirs(root / f"class{ci}")
        for i in range(9):
            arr = (rs.rand(33, 40, 3) * 255).astype(np.uint8)
            Image.fromarray(arr).save(str(root / f"class{ci}" / f"im{i}.{'jpg' if i % 3 else 'png'}"), quality=90)
    return root


@pytest.mark.parametrize("kind", ["store", "prefetch", "prefetch-threads"])
def test_feeder_next_labelled_on_the_file_kinds(dev, tree, kind, monkeypatch):
    """The HBM-resident store and the prefetcher (plans drawn `depth` batches ahead) deliver, with next() interleaved, the batches of
    the sequential sample_batch() and with each the class indices of ITS plan."""
    from embeddingnet_amd.datagenerators import ENDataLoader, TripletsDataGenerator
    dl = ENDataLoader(str(tree), validate=False)

    def gen():
        return TripletsDataGenerator(embedding_model=None, class_files_paths=dl.train_data, class_names=dl.class_names,
                                     input_shape=[24, 20, 3], k_classes=4, k_samples=3, margin=0.5,
                                     negatives_selection_mode="proxy_anchor")
    pattern = [True, False, True, True, False, True, False, False, True]
    g = gen()
    np.random.seed(3)
    plans = [g.sample_plan() for _ in range(len(pattern) + 5)]
    monkeypatch.setenv("EMBNET_IMAGE_STORE", "1" if kind == "store" else "0")
    monkeypatch.setenv("EMBNET_DECODE_PROCESSES", "0" if kind == "prefetch-threads" else "1")
    np.random.seed(3)
    g = gen()
    feeder = g.feeder(dev, depth=4, workers=3)
    assert feeder.kind.startswith(kind.split("-")[0])
    try:
        for labelled, plan in zip(pattern, plans):
            want = g.load_plan(plan)
            if labelled:
                got, labels = feeder.next_labelled()
                assert labels.dtype == torch.int32 and labels.is_cuda and labels.shape == (12,)
                assert labels.tolist() == [dl.class_names.index(cl) for cl in plan[0] for _ in range(3)]
            else:
                got = feeder.next()
            assert got.dtype == torch.float32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
        ahead = 0 if kind == "store" else len(feeder._plan_labels)
        assert (kind == "store" and len(feeder._plan_labels) == 0) or ahead >= 4       # the labels of the plans drawn ahead wait
    finally:
        feeder.close()


# ---------------------------------------------------------------------------------------------------------------- 5. CLI
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["proxy_anchor", "proxy_softmax"]


def _cli(tmp_path, mode, edit=lambda cfg: cfg, extra=(), env=None, launcher=()):
    cfg = open(os.path.join(ROOT, "configs", f"simple2_{mode}_synthetic.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert f"negatives_selection_mode : '{mode}'" in cfg and "n_batches : 20" in cfg and "proxy_loss :" in cfg
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(edit(cfg.replace("n_batches : 20", "n_batches : 6")))
    return subprocess.run([sys.executable, *launcher, os.path.join(ROOT, "tools", "train.py"), str(cfg_path), "--synthetic", "10",
                           "--max_epochs", "2", *extra], capture_output=True, text=True, timeout=600, env=env)


def _losses(stdout):
    return [float(v) for v in re.findall(r"Epoch \d+/\d+ - lr \S+ - loss (\S+)", stdout)]


@pytest.mark.parametrize("mode", MODES)
def test_train_cli_trains_checkpoints_and_resumes(tmp_path, mode):
    follow_loss = lambda cfg: cfg.replace("monitor : 'val_map@r'", "monitor : 'loss'")     # a checkpoint after every epoch that trains
    assert "monitor : 'loss'" in follow_loss(open(os.path.join(ROOT, "configs", f"simple2_{mode}_synthetic.yml")).read())
    out = _cli(tmp_path, mode, follow_loss)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch 2/2" in out.stdout and "saving model" in out.stdout
    project = tmp_path / f"simple2_{mode}_synthetic"
    saved = sorted(os.listdir(project / "weights"))
    assert saved and saved == sorted(os.listdir(project / "optimizer")) == sorted(os.listdir(project / "proxies"))
    ck = np.load(project / "proxies" / saved[-1])
    assert ck["proxies"].shape == (10, 256) and [str(v) for v in ck["class_names"]] == [f"class_{i:03d}" for i in range(10)]
    opt = np.load(project / "optimizer" / saved[-1])
    assert "proxy_head/proxies::slot1" in opt.files
    first = _losses(out.stdout)
    assert len(first) == 2
    assert saved[-1] == "epoch_002.npz", (saved, first)                   # the loss fell: the last epoch is checkpointed
    res = _cli(tmp_path, mode, follow_loss, extra=("--resume_from", str(project / "weights" / saved[-1])))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "resumed proxies from" in res.stdout and "resumed optimizer state" in res.stdout
    resumed = _losses(res.stdout)
    print(mode, "losses", first, "resumed", resumed)
    assert abs(resumed[0] - first[-1]) < abs(resumed[0] - first[0])       # it starts near the last loss, not near the initial one


@pytest.mark.parametrize("mode,edit,needle", [
    ("proxy_anchor", lambda c: c.replace("'proxy_anchor'", "'semihard'"), "GENERATOR.proxy_loss"),
    ("proxy_anchor", lambda c: c.replace("mode : 'triplet'", "mode : 'siamese'"), "Siamese"),
    ("proxy_anchor", lambda c: c.replace("{alpha: 32.0, delta: 0.1}", "{alpha: 32.0, margin: 0.1}"), "GENERATOR.proxy_loss"),
    ("proxy_anchor", lambda c: c.replace("alpha: 32.0", "alpha: 0.0"), "alpha must be positive"),
    ("proxy_softmax", lambda c: c.replace("scale: 64.0", "scale: -1"), "scale must be positive"),
    ("proxy_softmax", lambda c: c.replace("proxy_loss :", "supcon_loss : {temperature: 0.1}\n  proxy_loss :"), "GENERATOR.supcon_loss"),
    ("proxy_softmax", lambda c: c.replace("proxy_loss :", "ms_loss : {alpha: 2.0}\n  proxy_loss :"), "GENERATOR.ms_loss"),
], ids=["other mode", "siamese", "unknown key", "alpha 0", "scale -1", "supcon_loss", "ms_loss"])
def test_train_cli_refuses_a_bad_proxy_loss_before_training(tmp_path, mode, edit, needle):
    out = _cli(tmp_path, mode, edit)
    assert out.returncode != 0
    assert needle in out.stderr and "Epoch 1" not in out.stdout


def test_train_cli_refuses_proxies_of_other_classes(tmp_path):
    out = _cli(tmp_path, "proxy_anchor")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    project = tmp_path / "simple2_proxy_anchor_synthetic"
    name = sorted(os.listdir(project / "proxies"))[-1]
    ck = np.load(project / "proxies" / name)
    np.savez(project / "proxies" / name, proxies=ck["proxies"], class_names=ck["class_names"][::-1])
    res = _cli(tmp_path, "proxy_anchor", extra=("--resume_from", str(project / "weights" / name)))
    assert res.returncode != 0 and "class_names" in res.stderr and "Epoch 1" not in res.stdout


def test_train_cli_two_ranks_end_with_identical_proxies_and_weights(tmp_path):
    """Two ranks on one GPU over gloo (the pattern of tests/test_train_cli_gpu.py): the proxies are replicated, their gradients
    averaged like the backbone's: both ranks end with bit-identical proxies and backbone weights."""
    env = dict(os.environ, EMBNET_DIST_BACKEND="gloo", EMBNET_DUMP_FINAL_WEIGHTS=str(tmp_path / "final_rank"))
    out = _cli(tmp_path, "proxy_anchor", env=env,
               launcher=("-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", "29588"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "Epoch 2/2" in out.stdout
    p0, p1 = np.load(str(tmp_path / "final_rank") + "0_proxies.npz"), np.load(str(tmp_path / "final_rank") + "1_proxies.npz")
    assert np.array_equal(p0["proxies"], p1["proxies"]) and np.array_equal(p0["class_names"], p1["class_names"])
    w0, w1 = np.load(str(tmp_path / "final_rank") + "0.npz"), np.load(str(tmp_path / "final_rank") + "1.npz")
    assert set(w0.files) == set(w1.files) and len(w0.files) > 10
    for k in w0.files:
        if "moving_" in k:
            continue                                   # BatchNorm statistics are local to a rank (as the reference: no SyncBN)
        assert np.array_equal(w0[k], w1[k]), k
