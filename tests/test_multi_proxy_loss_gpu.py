"""SoftTriple and sub-centre ArcFace (ops.soft_triple_loss, ops.arcface_loss, csrc/multi_proxy_loss.hip) against the float64 reference
and the a-priori bounds of tests/multi_proxy_ref.py, the two forward paths against each other, the degenerate identities against the
proxy losses, and inside the training step (train_step.ProxyTrainer: eager and graph-replayed) and tools/train.py (checkpoints,
resume, refusals).

Every check prints its largest error / bound before it asserts ratio < 1.  Open decisions are a condition, not a tolerance: an ArcFace
argmax cell whose two largest similarities lie within 2 max dS of each other is compared by its class total only, and at most 1 % of a
case's cells may be such.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import multi_proxy_ref as M
import proxy_ref as P

pytestmark = pytest.mark.gpu
UP = 0.75
KINDS = list(M.KINDS)
KIND_CODE = {"soft_triple": 1, "arcface": 2}
PATH_CODE = {"auto": 0, "small": 1, "matrix": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(kind, x, w, lab, c, dev, a=None, b=None, gam=None, tau=None, path="auto", g=None):
    from embeddingnet_amd import ops
    pr = M.params32(kind, a, b, gam, tau)
    xt = torch.tensor(x, device=dev).requires_grad_(True)
    wt = torch.tensor(w, device=dev).requires_grad_(True)
    lt = torch.tensor(np.asarray(lab, np.int32), device=dev)
    if kind == "soft_triple":
        mean, counts, reg, gw = ops.soft_triple_loss(xt, wt, lt, c, pr["a"], pr["b"], pr["gamma"], pr["tau"], path=path, return_weights=True)
    else:
        mean, counts, gw = ops.arcface_loss(xt, wt, lt, c, pr["a"], pr["b"], path=path, return_weights=True)
        reg = torch.zeros((), device=dev)
    mean.backward(None if g is None else torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), reg=float(reg.item()), counts=counts.cpu().numpy(), G=gw.cpu().numpy(),
                demb=xt.grad.cpu().numpy(), dw=wt.grad.cpu().numpy(), t=(mean.detach().clone(), counts.clone(), gw, xt.grad, wt.grad))


def _raw(kind, x, w, lab, c, dev, path=0, pad=16, ws=None, fill_ff=False, tau=None, no_h=False):
    """The C ABI directly on buffers with `pad` guard elements on either side.  no_h: the backward without the regulariser's H.
    -> dict of the padded buffers."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    (n, e), nb = x.shape, w.shape[0]
    kc = nb // c
    pr = M.params32(kind, tau=tau)
    xt, wt = torch.tensor(x, device=dev), torch.tensor(w, device=dev)
    lt = torch.tensor(np.asarray(lab, np.int32), device=dev)
    wsn = lib.embnet_multi_proxy_loss_workspace_bytes(n, c, kc, e) // 4
    nan = float("nan")
    gb, db, pb, qb, hb, mb, rb = (torch.full((2 * pad + m,), nan, device=dev) for m in (n * nb, n * e, nb * e, nb, c * kc * kc, 1, 1))
    if fill_ff:
        gb.view(torch.int32).fill_(-1)                                  # 0xFF bytes
    cb = torch.full((2 * pad + 3,), -12345, dtype=torch.int32, device=dev)
    if ws is None:
        ws = torch.full((2 * pad + wsn,), nan, device=dev)
        ws[pad:pad + wsn] = 0
    up = torch.tensor(UP, device=dev)
    sl = lambda t, m: t[pad:pad + m].data_ptr()
    has_h = kind == "soft_triple" and kc > 1 and pr["tau"] > 0
    s = _lib.stream()
    _lib.check(lib.embnet_multi_proxy_loss_fwd(xt.data_ptr(), wt.data_ptr(), lt.data_ptr(), n, c, kc, e, KIND_CODE[kind], pr["a"], pr["b"],
                                               pr["gamma"], pr["tau"], path, sl(gb, n * nb), sl(qb, nb), sl(hb, c * kc * kc) if has_h else None,
                                               sl(cb, 3), sl(mb, 1), sl(rb, 1), sl(ws, wsn), wsn * 4, s))
    _lib.check(lib.embnet_multi_proxy_loss_bwd(xt.data_ptr(), wt.data_ptr(), n, c, kc, e, sl(gb, n * nb), sl(qb, nb),
                                               sl(hb, c * kc * kc) if has_h and not no_h else None, up.data_ptr(), sl(db, n * e),
                                               sl(pb, nb * e), sl(ws, wsn), wsn * 4, s))
    torch.cuda.synchronize()
    return dict(G=gb, demb=db, dw=pb, q=qb, H=hb, counts=cb, mean=mb, reg=rb, ws=ws, has_h=has_h, pad=pad)


def _qh(kind, w, c, dev, tau=None):
    """The device's q and H (None without a regulariser) through the C ABI's forward on a two-row batch (ops keeps them to itself)."""
    r = _raw(kind, np.zeros((2, w.shape[1]), np.float32), w, np.zeros(2, np.int32), c, dev, tau=tau)
    kc = w.shape[0] // c
    q = r["q"][16:-16].cpu().numpy()
    return q, (r["H"][16:-16].cpu().numpy().reshape(c, kc, kc) if r["has_h"] else None), float(r["reg"][16].item())


@functools.lru_cache(maxsize=None)
def _inputs(shape, grid):
    """-> (x, w, labels, c, kc, unit or None), shared by the tests and left unchanged."""
    out = M.case_inputs(shape, grid)
    for t in out[:3]:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, grid):
    x, w, lab, c, _, _ = _inputs(shape, grid)
    return M.reference(kind, x, w, lab, c)


def _check(kind, got, x, w, lab, c, gs, dev, a=None, b=None, gam=None, tau=None, g=1.0, what="", unit=None, ref=None):
    """Everything the header promises about one forward + backward, for a device whose D is within gs A of the truth: the counters
    (violating and lower-branch samples between the sure and the possible count, exact where nothing is open), every entry of G
    outside the open argmax cells and every class total, the loss, reg and H, and (from the device's own G, q and H) every element of
    demb and dcentres.  gs = 0 only where D is exact in any order: the argmax is then the reference's.  -> {check: error / bound}."""
    n, nb = x.shape[0], w.shape[0]
    kc = nb // c
    exact = gs == 0
    assert not exact or P.exact_in_any_order(x, w, unit)
    for key in ("G", "demb", "dw"):
        assert np.isfinite(got[key]).all(), key
    assert np.isfinite(got["loss"]) and np.isfinite(got["reg"])
    ref = M.reference(kind, x, w, lab, c, a, b, gam, tau) if ref is None else ref
    assert got["G"].shape == (n, nb) and got["counts"].dtype == np.int32 and got["counts"].shape == (3,)
    assert got["counts"][0] == ref["counts"][0], (got["counts"], ref["counts"])
    d = M.decisions(ref, gs)
    assert not d["branch_open"].any()
    assert d["sure"].sum() <= got["counts"][1] <= d["may"].sum(), (got["counts"], d["sure"].sum(), d["may"].sum())
    assert d["lower_sure"].sum() <= got["counts"][2] <= d["lower_may"].sum(), (got["counts"], d["lower_sure"].sum())
    if not d["open"].any():
        assert got["counts"][1] == ref["counts"][1], (got["counts"], ref["counts"])
    assert got["counts"][2] == ref["counts"][2]
    bd = M.bounds(ref, gs, exact_argmax=exact)
    opened = bd["open_cells"]
    share = float(opened.mean())
    assert share <= M.OPEN_CAP, share
    closed = np.repeat(~opened, kc, 1)
    err, bg = np.abs(got["G"] - ref["G"]), bd["G"]
    zero = closed & (bg == 0)                                           # unlabelled rows; ArcFace's sub-centres off the argmax
    assert not got["G"][zero].any()
    live = closed & (bg > 0)
    ratios = dict(open_share=share)
    ratios["G"] = float((err[live] / bg[live]).max()) if live.any() else 0.0
    if kind == "arcface":                                               # the class totals, open cells included: always bounded
        tot, want = got["G"].astype(np.float64).reshape(n, c, kc).sum(2), ref["G"].reshape(n, c, kc).sum(2)
        lv = bd["total"] > 0
        assert not tot[~lv].any()
        ratios["total"] = float((np.abs(tot - want)[lv] / bd["total"][lv]).max()) if lv.any() else 0.0
    ratios["loss"] = float(abs(got["loss"] - ref["loss"]) / bd["loss"])
    q_dev, h_dev, _ = _qh(kind, w, c, dev, tau=ref["pr"]["tau"])
    assert np.array_equal(q_dev, ref["q"])                              # q is reproduced bit for bit
    if h_dev is not None:
        ratios["reg"] = float(abs(got["reg"] - ref["reg"]["R"]) / bd["reg"])
        off = bd["H"] > 0
        ratios["H"] = float((np.abs(h_dev - ref["reg"]["H"])[off] / bd["H"][off]).max())
        assert not h_dev[~off].any()
    else:
        assert got["reg"] == 0.0 and ref["reg"]["R"] == 0.0
    demb, b_emb, dw, b_w = M.grads(x, w, got["G"], q_dev, c, h_dev, g)
    ratios["demb"] = float((np.abs(got["demb"] - demb) / b_emb).max())
    ratios["dcentres"] = float((np.abs(got["dw"] - dw) / b_w).max())
    assert not got["demb"][~ref["labelled"]].any()                      # an unlabelled sample receives no gradient
    assert not got["dw"][ref["q"] == 0].any()                           # a zero centre neither
    print(f"mproxy {what} {kind} n={n} c={c} kc={kc} e={x.shape[1]} counts={got['counts']}: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    assert all(v < 1 for k, v in ratios.items() if k != "open_share"), ratios
    return ratios


ALL_SHAPES = M.SHAPES + ["ragged"]
BOTH_PATHS = M.SMALL_SHAPES + ["ragged"]                              # every case that fits the small path runs on both


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_values_on_grid_inputs(dev, shape, kind):
    x, w, lab, c, _, unit = _inputs(shape, True)
    ref = _reference(kind, shape, True)
    for g in (None, UP):
        _check(kind, _run(kind, x, w, lab, c, dev, g=g), x, w, lab, c, 0.0, dev, g=1.0 if g is None else g, what="grid", unit=unit, ref=ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_values_on_continuous_inputs(dev, shape, kind):
    x, w, lab, c, _, _ = _inputs(shape, False)
    _check(kind, _run(kind, x, w, lab, c, dev, g=UP), x, w, lab, c, M.gamma_s_of(shape), dev, g=UP, what="continuous",
           ref=_reference(kind, shape, False))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", BOTH_PATHS, ids=str)
def test_forward_paths_agree_on_a_grid_input(dev, shape, kind):
    x, w, lab, c, _, unit = _inputs(shape, True)
    assert P.exact_in_any_order(x, w, unit)
    r1, r2 = _run(kind, x, w, lab, c, dev, path="small", g=UP), _run(kind, x, w, lab, c, dev, path="matrix", g=UP)
    for a, b in zip(r1["t"][1:], r2["t"][1:]):                          # counts, G, demb, dcentres: bit-equal
        assert torch.equal(a, b)
    assert r1["loss"] == r2["loss"] and r1["reg"] == r2["reg"]
    _check(kind, r2, x, w, lab, c, 0.0, dev, g=UP, what="matrix path", unit=unit, ref=_reference(kind, shape, True))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["small", "matrix"])
@pytest.mark.parametrize("shape", BOTH_PATHS, ids=str)
def test_both_paths_on_a_continuous_input(dev, shape, path, kind):
    x, w, lab, c, _, _ = _inputs(shape, False)
    _check(kind, _run(kind, x, w, lab, c, dev, path=path), x, w, lab, c, M.gamma_s_of(shape, path), dev, what=path,
           ref=_reference(kind, shape, False))


# ---------------------------------------------------------------------------------------------------------------- 2. identities
def _proxy_softmax(x, w, lab, dev, scale, margin, g=UP):
    from embeddingnet_amd import ops
    xt = torch.tensor(x, device=dev).requires_grad_(True)
    wt = torch.tensor(w, device=dev).requires_grad_(True)
    mean, counts, gw = ops.proxy_softmax_loss(xt, wt, torch.tensor(lab, device=dev), scale, margin, return_weights=True)
    mean.backward(torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), counts=counts.cpu().numpy(), G=gw.cpu().numpy(), demb=xt.grad.cpu().numpy(), dw=wt.grad.cpu().numpy())


def _same_within_both_bounds(what, got, other, x, w, q, c, bg, bl, bg2, bl2, g=UP):
    """Two runs of one mathematical loss: the losses and G's within the sum of their bounds, the gradients within the sum of their own
    bounds plus what the G's may differ by, carried through the (linear) backward."""
    dg = bg + bg2
    assert abs(got["loss"] - other["loss"]) <= bl + bl2
    assert (np.abs(got["G"] - other["G"]) <= dg).all()
    demb, b_emb, dw, b_w = M.grads(x, w, got["G"], q, c, None, g)
    demb2, b_emb2, dw2, b_w2 = M.grads(x, w, other["G"], q, c, None, g)
    assert (np.abs(got["demb"] - other["demb"]) <= b_emb + b_emb2 + np.abs(demb - demb2)).all()
    assert (np.abs(got["dw"] - other["dw"]) <= b_w + b_w2 + np.abs(dw - dw2)).all()
    xa, wa, qd = np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64)), q.astype(np.float64)
    # |G - G'| <= dg entrywise bounds what the two float64 gradients may differ by (the backward is linear in G)
    assert (np.abs(demb - demb2) <= abs(g) * (dg * qd[None, :]) @ wa * (1 + 1e-9) + 1e-300).all()
    ya = dg.T @ xa
    assert (np.abs(dw - dw2) <= abs(g) * qd[:, None] * (ya + (qd * qd * (ya * wa).sum(1))[:, None] * wa) * (1 + 1e-9) + 1e-300).all()
    print(f"mproxy identity {what}: loss {got['loss']} vs {other['loss']}, max |dG| {np.abs(got['G'] - other['G']).max():.3g}")


def test_soft_triple_with_one_centre_is_cosface(dev):
    shape = (16, 16, 40, 1, 128)
    x, w, lab, c, _, _ = _inputs(shape, False)
    gs = M.gamma_s_of(shape)
    got = _run("soft_triple", x, w, lab, c, dev, a=20.0, b=0.01, g=UP)
    cos = _proxy_softmax(x, w, lab, dev, 20.0, 0.01)
    ref = _reference("soft_triple", shape, False)
    bd = M.bounds(ref, gs)
    bg2, bl2 = P.bounds(P.reference("softmax", x, w, lab, 20.0, 0.01), P.gamma_s(P.auto_path(256, 40, 128), 128))
    _same_within_both_bounds("soft_triple kc=1 vs CosFace", got, cos, x, w, ref["q"], c, bd["G"], bd["loss"], bg2, bl2)
    assert got["counts"][1] == cos["counts"][2] and got["counts"][0] == cos["counts"][0] and got["reg"] == 0.0


def test_arcface_with_margin_zero_and_one_centre_is_normsoftmax(dev):
    shape = (16, 16, 40, 1, 128)
    x, w, lab, c, _, _ = _inputs(shape, False)
    gs = M.gamma_s_of(shape)
    got = _run("arcface", x, w, lab, c, dev, a=64.0, b=0.0, g=UP)
    nsm = _proxy_softmax(x, w, lab, dev, 64.0, 0.0)
    ref = M.reference("arcface", x, w, lab, c, b=0.0)
    bd = M.bounds(ref, gs)
    bg2, bl2 = P.bounds(P.reference("softmax", x, w, lab, 64.0, 0.0), P.gamma_s(P.auto_path(256, 40, 128), 128))
    _same_within_both_bounds("arcface m=0 kc=1 vs NormSoftmax", got, nsm, x, w, ref["q"], c, bd["G"], bd["loss"], bg2, bl2)
    assert got["counts"][1] == nsm["counts"][2] and got["counts"][2] == 0


def test_arcface_duplicated_sub_centres_put_the_whole_weight_on_the_first(dev):
    shape = (16, 16, 40, 1, 128)
    x, w, lab, c, _, _ = _inputs(shape, False)
    gs = M.gamma_s_of(shape)
    one = _run("arcface", x, w, lab, c, dev, g=UP)
    w3 = np.repeat(w, 3, 0)                                             # rows identical, kc = 3
    got = _run("arcface", x, w3, lab, c, dev, g=UP)
    assert not got["G"][:, 1::3].any() and not got["G"][:, 2::3].any()  # exactly 0 on the copies
    ref = _reference("arcface", shape, False)
    bd = M.bounds(ref, gs)
    assert abs(got["loss"] - one["loss"]) <= 2 * bd["loss"]
    assert (np.abs(got["G"][:, 0::3] - one["G"]) <= 2 * bd["G"]).all()
    demb, b_emb, _, _ = M.grads(x, w, one["G"], ref["q"], c, None, UP)
    demb3, b_emb3, _, _ = M.grads(x, w3, got["G"], np.repeat(ref["q"], 3), c, None, UP)
    assert (np.abs(got["demb"] - one["demb"]) <= b_emb + b_emb3 + np.abs(demb - demb3)).all()
    assert np.array_equal(got["counts"], one["counts"])
    assert not got["dw"][1::3].any() and not got["dw"][2::3].any()      # a copy that never wins receives no gradient


# ---------------------------------------------------------------------------------------------------------------- 3. ArcFace's branches
def _hand(dev):
    """e = 4, three classes of two centres, on the grid.  Sample 0 = e1 of class 0, whose centres are -2 e1 and -e1 (S = -1, -1: the
    guard's branch, the tie to j = 0); sample 1 = e2 of class 1 with centres 2 e2 (S' = 1 exactly, r = 0) and e3; sample 2 =
    (3, 4, 0, 0) / 5 of class 2 with centres e1 and e4; sample 3 = e3, unlabelled."""
    w = np.zeros((6, 4), np.float32)
    w[0, 0], w[1, 0], w[2, 1], w[3, 2], w[4, 0], w[5, 3] = -2, -1, 2, 1, 1, 1
    x = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0.625, 0.75, 0, 0], [0, 0, 1, 0]], np.float32)
    return x, w, np.array([0, 1, 2, -1], np.int32), 3


def test_arcface_branches_on_hand_cases(dev):
    x, w, lab, c = _hand(dev)
    assert P.exact_in_any_order(x, w, 1.0 / 8)
    got = _run("arcface", x, w, lab, c, dev, a=4.0, g=UP)               # scale 4: the own class keeps a weight well below 1
    ref = M.reference("arcface", x, w, lab, c, a=4.0)
    pr = ref["pr"]
    assert ref["sy"][0] == -1.0 <= pr["th"] - 0.01 and ref["sy"][1] == 1.0 and ref["r"][1] == 0.0
    assert got["counts"].tolist() == [3, 2, 1] == ref["counts"].tolist()            # samples 0 and 2 (0.75 >= 0.625) violate; one lower
    _check("arcface", got, x, w, lab, c, 0.0, dev, a=4.0, g=UP, what="hand", unit=1.0 / 8, ref=ref)
    assert got["G"][0, 0] != 0 and got["G"][0, 1] == 0                              # the tie goes to the smaller j
    assert ref["psi"][0] == 1.0                                                     # the guard's branch has slope 1
    # S' = 1: r = 0 and phi' = cos m, the contract's slope there: a finite weight (the unfloored slope is infinite)
    wy = ref["e"][1, 1] / ref["d"][1]
    want = 4.0 / 3.0 * (wy - 1.0) * pr["cm"]
    assert 0.5 < wy < 0.99 and ref["psi"][1] == pr["cm"]
    assert np.isfinite(got["G"][1]).all() and abs(got["G"][1, 2] - want) <= M.bounds(ref, 0.0, exact_argmax=True)["G"][1, 2]
    assert np.isfinite(got["demb"]).all() and np.isfinite(got["dw"]).all()


# ---------------------------------------------------------------------------------------------------------------- 4. traps
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["small", "matrix"])
def test_unnormalised_rows_of_norm_30_stay_finite_and_within_bounds(dev, path, kind):
    """S' reaches 25: SoftTriple's pooling exponents reach 250 at gamma 0.1, ArcFace's own class is past S' = 1 (phi = S' cos m)."""
    shape = (8, 4, 24, 3, 256)
    x, w, lab, c, _, _ = _inputs(shape, False)
    x = (30.0 * x).astype(np.float32)
    got = _run(kind, x, w, lab, c, dev, path=path, g=UP)
    ref = M.reference(kind, x, w, lab, c)
    assert ref["sy"][ref["labelled"]].min() > 1.0
    _check(kind, got, x, w, lab, c, M.gamma_s_of(shape, path), dev, g=UP, what="norm 30 " + path, ref=ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["small", "matrix"])
def test_a_logit_spread_of_200_takes_no_log_of_zero(dev, path, kind):
    """proxy_ref.underflow_trap with every centre twice (once at twice the length): class logits 200 / 40 / 0.  ArcFace takes the
    trap's own centres, the samples at half the length and twice the scale: the same logits, and S' = 0.5 instead of 1, away from
    the floor band of r."""
    x, w, lab, a = P.underflow_trap()
    w2 = (np.repeat(w, 2, 0) * np.tile([1.0, 2.0], 3)[:, None]).astype(np.float32)
    if kind == "arcface":                                               # (one centre per class: equal copies would tie in every cell)
        x, a, w2 = (0.5 * x).astype(np.float32), 2 * a, w
    got = _run(kind, x, w2, lab, 3, dev, a=a, b=0.0, path=path)
    assert np.isfinite(got["loss"]) and got["loss"] > 0
    ref = M.reference(kind, x, w2, lab, 3, a=a, b=0.0)
    assert np.allclose(ref["t"][0], [200.0, 40.0, 0.0])
    _check(kind, got, x, w2, lab, 3, P.gamma_s(path, 3), dev, a=a, b=0.0, what="trap " + path, ref=ref)


# ---------------------------------------------------------------------------------------------------------------- 5. the regulariser
def test_regulariser_off_leaves_no_trace(dev):
    shape = (8, 4, 24, 3, 256)
    x, w, lab, c, _, _ = _inputs(shape, False)
    on, off = _run("soft_triple", x, w, lab, c, dev, g=UP), _run("soft_triple", x, w, lab, c, dev, tau=0.0, g=UP)
    assert off["reg"] == 0.0 and on["reg"] > 0.0
    for i in (1, 2, 3):                                                 # counts, G, demb: the regulariser does not reach them
        assert torch.equal(on["t"][i], off["t"][i])
    assert not torch.equal(on["t"][4], off["t"][4])
    raw = _raw("soft_triple", x, w, lab, c, dev, no_h=True)             # the regularised forward, the backward without H
    assert torch.equal(raw["dw"][16:-16], off["t"][4].reshape(-1)) and torch.equal(raw["G"][16:-16], off["t"][2].reshape(-1))
    _check("soft_triple", off, x, w, lab, c, M.gamma_s_of(shape), dev, tau=0.0, g=UP, what="tau 0")
    # a positive tau that is 0 as the float the library receives: no regulariser, and no H for the backward to read
    from embeddingnet_amd import ops
    xt, wt = torch.tensor(x, device=dev).requires_grad_(True), torch.tensor(w, device=dev).requires_grad_(True)
    mean, _, reg = ops.soft_triple_loss(xt, wt, torch.tensor(lab, device=dev), c, tau=1e-46)
    mean.backward(torch.tensor(UP, device=dev))
    assert float(reg) == 0.0 and torch.equal(wt.grad, off["t"][4]) and torch.equal(xt.grad, off["t"][3])
    x1, w1, lab1, c1, _, _ = _inputs((16, 16, 40, 1, 128), False)       # one centre per class: no pairs
    a, b = _run("soft_triple", x1, w1, lab1, c1, dev, g=UP), _run("soft_triple", x1, w1, lab1, c1, dev, tau=0.0, g=UP)
    assert a["reg"] == 0.0 and a["loss"] == b["loss"]
    for u, v in zip(a["t"], b["t"]):
        assert torch.equal(u, v)


def test_identical_centres_have_a_finite_regulariser_gradient(dev):
    shape = (8, 4, 24, 3, 256)
    x, w, lab, c, kc, _ = _inputs(shape, False)
    ident = np.repeat(w[::kc], kc, 0)                                   # g = 1: the root's argument is 1e-5
    got = _run("soft_triple", x, ident, lab, c, dev, g=UP)
    assert np.isfinite(got["dw"]).all() and got["reg"] > 0
    _check("soft_triple", got, x, ident, lab, c, M.gamma_s_of(shape), dev, g=UP, what="identical centres")


def test_an_absent_class_moves_by_the_regulariser_and_the_negative_term_only(dev):
    """Plain SGD on an identity backbone: an update IS -lr times the loss's gradient.  An absent class's total weight is the softmax's
    (not negative), and its centres' update is -lr dcentres of its columns of G and its block of H."""
    from embeddingnet_amd import ops
    from embeddingnet_amd.proxies import ProxyHead
    from embeddingnet_amd.train_step import ProxyTrainer
    import recipes as R
    c, kc, e, lr = 12, 3, 64, 0.05
    head = ProxyHead(c, e, seed=1, centers_per_class=kc).to(dev)
    opt = torch.optim.SGD([head.proxies], lr=lr)
    tr = ProxyTrainer(torch.nn.Identity(), head, opt, loss="soft_triple", graph=False)
    x = torch.tensor(R.clustered_embeddings(11, 8, 4, e, M.SIGMA), device=dev)
    y = torch.arange(8, dtype=torch.int32, device=dev).repeat_interleave(4)           # classes 8 .. 11 are absent
    w0 = head.proxies.detach().clone()
    _, counts, reg, g = ops.soft_triple_loss(x, w0, y, c, return_weights=True)
    assert counts.tolist()[0] == 32 and float(reg) > 0
    tr.step(x, y)
    assert float(tr.last_reg) == float(reg)
    dw = (head.proxies.detach().double() - w0.double()).cpu().numpy()
    gn, w0n = g.cpu().numpy(), w0.cpu().numpy()
    assert (np.linalg.norm(dw, axis=1) > 0).all()
    tot = gn.astype(np.float64).reshape(32, c, kc).sum(2)
    ref = M.reference("soft_triple", x.cpu().numpy(), w0n, y.cpu().numpy(), c)
    bd = M.bounds(ref, P.gamma_s("small", e))
    assert (tot[:, 8:] >= -bd["G"].reshape(32, c, kc).sum(2)[:, 8:]).all() and (ref["base"][:, 8:] > 0).all()
    q, h, _ = _qh("soft_triple", w0n, c, dev)
    _, _, want, bound = M.grads(x.cpu().numpy(), w0n, gn, q, c, h)
    tol = lr * bound + P.U * (2 * lr * np.abs(want) + np.abs(w0n) + np.abs(w0n - lr * want))
    ratio = float((np.abs(dw + lr * want) / tol).max())
    _, _, no_reg, _ = M.grads(x.cpu().numpy(), w0n, gn, q, c, None)
    assert np.abs(want - no_reg)[8 * kc:].max() > 0                     # the regulariser does move the absent classes' centres
    print("centre update vs -lr dcentres: error / bound", ratio)
    assert ratio < 1


# ---------------------------------------------------------------------------------------------------------------- 6. robustness, hygiene
@pytest.mark.parametrize("kind", KINDS)
def test_a_zero_centre_has_zero_similarity_and_no_gradient(dev, kind):
    x, w, lab, c, kc, unit = _inputs((8, 4, 24, 3, 256), True)
    w = w.copy()
    w[int(lab[0]) * kc + 1] = 0                                         # a present class's centre
    w[int(np.setdiff1d(np.arange(c), lab)[0]) * kc] = 0                 # and an absent one's
    assert (P.q_of(w) == 0).sum() == 2
    got = _run(kind, x, w, lab, c, dev, g=UP)
    _check(kind, got, x, w, lab, c, 0.0, dev, g=UP, what="zero centre", unit=unit)
    assert not got["dw"][P.q_of(w) == 0].any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["small", "matrix"])
def test_all_unlabelled_gives_the_regulariser_alone_and_zero_weights(dev, path, kind):
    x, w, lab, c, _, _ = _inputs((8, 4, 24, 3, 256), True)
    lab = np.where(np.arange(32) % 2 == 0, -1, c).astype(np.int32)
    lab[3], lab[5] = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    got = _run(kind, x, w, lab, c, dev, path=path, g=UP)
    assert got["loss"] == got["reg"] and not got["G"].any() and not got["demb"].any()
    assert got["counts"].tolist() == [0, 0, 0]
    assert (got["reg"] > 0 and got["dw"].any()) if kind == "soft_triple" else (got["reg"] == 0.0 and not got["dw"].any())


def test_out_of_range_arguments_raise(dev):
    from embeddingnet_amd import ops
    from embeddingnet_amd._lib import EmbnetError
    x, lab = torch.rand((8, 4), device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    w = torch.rand((6, 4), device=dev)
    for fn in (ops.soft_triple_loss, ops.arcface_loss):
        with pytest.raises(EmbnetError, match="multi_proxy_loss_fwd"):
            fn(x, w, lab, 3, -1.0)
        with pytest.raises(EmbnetError, match="multi_proxy_loss_fwd"):
            fn(x[:1], w, lab[:1], 3)
        with pytest.raises(EmbnetError, match="labels"):
            fn(x, w, lab.long(), 3)
        with pytest.raises(EmbnetError, match="path"):
            fn(x, w, lab, 3, path="per_class")
        with pytest.raises(EmbnetError, match="width"):
            fn(x, torch.rand((6, 5), device=dev), lab, 3)
        with pytest.raises(EmbnetError, match="whole number per class"):
            fn(x, w, lab, 4)
        with pytest.raises(EmbnetError, match="kc=33"):
            fn(x, torch.rand((66, 4), device=dev), lab, 2)
        with pytest.raises(EmbnetError, match="c\\*kc=16386"):
            fn(x, torch.rand((16386, 4), device=dev), lab, 8193)
    for m in (float(np.pi / 2), 1.6, -0.1):
        with pytest.raises(EmbnetError, match="pi/2"):
            ops.arcface_loss(x, w, lab, 3, margin=m)
    with pytest.raises(EmbnetError, match="gamma"):
        ops.soft_triple_loss(x, w, lab, 3, gamma=0.0)
    with pytest.raises(EmbnetError, match="tau"):
        ops.soft_triple_loss(x, w, lab, 3, tau=-0.1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", [1, 2])
def test_nothing_is_written_outside_the_outputs_and_the_ticket_is_rearmed(dev, path, kind):
    shape, pad = (5, 5, 7, 2, 33), 64                                   # n = 25, c kc = 14, e = 33: ragged tiles in every kernel
    x, w, lab, c, kc, _ = _inputs(shape, True)
    first = _raw(kind, x, w, lab, c, dev, path, pad, fill_ff=True)
    second = _raw(kind, x, w, lab, c, dev, path, pad, ws=first["ws"])   # back to back on ONE workspace
    got = _run(kind, x, w, lab, c, dev, path=["small", "matrix"][path - 1], g=UP)
    for out in (first, second):
        outs = [out[k] for k in ("G", "demb", "dw", "q", "mean", "reg")] + ([out["H"]] if out["has_h"] else [])
        for t in outs + [out["ws"]]:
            assert torch.isnan(t[:pad]).all() and torch.isnan(t[-pad:]).all()
        for t in outs:
            assert torch.isfinite(t[pad:-pad]).all()                    # every entry is written
        if not out["has_h"]:
            assert torch.isnan(out["H"]).all()                          # no regulariser: H is not touched
        cb = out["counts"]
        assert (cb[:pad] == -12345).all() and (cb[-pad:] == -12345).all()
        assert out["ws"][pad].view(torch.int32).item() == 0             # the ticket is re-armed
        assert np.array_equal(out["G"][pad:-pad].cpu().numpy(), got["G"].reshape(-1))
        assert np.array_equal(out["demb"][pad:-pad].cpu().numpy(), got["demb"].reshape(-1))
        assert np.array_equal(out["dw"][pad:-pad].cpu().numpy(), got["dw"].reshape(-1))
        assert np.array_equal(cb[pad:-pad].cpu().numpy(), got["counts"]) and out["mean"][pad].item() == got["loss"]
        assert out["reg"][pad].item() == got["reg"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["small", "matrix"])
def test_bitwise_reproducible(dev, path, kind):
    x, w, lab, c, _, _ = _inputs((32, 4, 100, 3, 256), False)
    r1, r2 = _run(kind, x, w, lab, c, dev, path=path, g=UP), _run(kind, x, w, lab, c, dev, path=path, g=UP)
    for a, b in zip(r1["t"], r2["t"]):
        assert torch.equal(a, b)
    assert r1["reg"] == r2["reg"]
    raw = _raw(kind, x, w, lab, c, dev, PATH_CODE[path], 16, fill_ff=True)            # its own workspace, a G buffer of 0xFF bytes
    assert torch.equal(raw["G"][16:-16], r1["t"][2].reshape(-1)) and torch.equal(raw["demb"][16:-16], r1["t"][3].reshape(-1))
    assert torch.equal(raw["dw"][16:-16], r1["t"][4].reshape(-1)) and torch.equal(raw["counts"][16:-16], r1["t"][1])
    assert torch.equal(raw["mean"][16], r1["t"][0])


# ---------------------------------------------------------------------------------------------------------------- 7. training
N_CLASSES = 12
MODES = ["soft_triple", "arcface"]
CENTERS = {"soft_triple": 4, "arcface": 3}


def _trainer(dev, graph, loss, seed=5):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.proxies import ProxyHead
    from embeddingnet_amd.train_step import ProxyTrainer
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=seed, device=dev)
    head = ProxyHead(N_CLASSES, 64, seed=1, centers_per_class=CENTERS[loss]).to(dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad] + [head.proxies], "adam", 1e-3)
    return base, head, opt, ProxyTrainer(base, head, opt, loss=loss, loss_params=dict(centers=CENTERS[loss]), seed=3, graph=graph)


def _batches(dev, steps):
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((N_CLASSES, 64, 64, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(N_CLASSES, generator=torch.Generator().manual_seed(i))[:8].to(dev)
        x = protos[cls].repeat_interleave(4, 0) + 0.15 * torch.randn((32, 64, 64, 3), device=dev, generator=gen)
        yield x.clamp(0, 1), cls.repeat_interleave(4).to(torch.int32)


@pytest.mark.parametrize("loss", MODES)
def test_trainer_learns(dev, loss):
    _, _, _, tr = _trainer(dev, graph=False, loss=loss)
    losses, viol = [], []
    for x, y in _batches(dev, 60):
        losses.append(float(tr.step(x, y).item()))
        trip, count = tr.last_triplets
        assert trip is None and count.dtype == torch.int32 and count.shape == (1,)
        assert tr.last_pair_counts.shape == (3,) and int(tr.last_pair_counts[1]) == int(count)
        assert int(tr.last_pair_counts[0]) == 32 and int(tr.last_pair_counts[2]) == 0
        assert (tr.last_reg is None) == (loss == "arcface")
        viol.append(int(count))
    print(f"{loss} trainer losses", [round(v, 4) for v in losses], "violating samples", viol)
    assert np.all(np.isfinite(losses))
    assert max(losses[-5:]) < losses[0], losses
    assert np.mean(viol[-10:]) < np.mean(viol[:10]), viol               # the violating samples fall: the last ten steps against the first ten


@pytest.mark.parametrize("loss", MODES)
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
            assert tr.last_triplets[1].data_ptr() == tr.last_pair_counts.data_ptr() + 4
            counts.append(tr.last_pair_counts.clone())
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        runs.append((torch.stack(losses), torch.stack(counts), head.proxies.detach().clone(),
                     torch.cat([q.detach().reshape(-1) for q in base.parameters()])))
    for a, b in zip(*runs):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()


# ---------------------------------------------------------------------------------------------------------------- 8. CLI
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_CENTERS = {"soft_triple": 10, "arcface": 1}


def _cli(tmp_path, mode, edit=lambda cfg: cfg, extra=()):
    cfg = open(os.path.join(ROOT, "configs", f"simple2_{mode}_synthetic.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert f"negatives_selection_mode : '{mode}'" in cfg and "n_batches : 20" in cfg and "proxy_loss :" in cfg
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(edit(cfg.replace("n_batches : 20", "n_batches : 6")))
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path), "--synthetic", "10", "--max_epochs", "2",
                           *extra], capture_output=True, text=True, timeout=600)


def _losses(stdout):
    return [float(v) for v in re.findall(r"Epoch \d+/\d+ - lr \S+ - loss (\S+)", stdout)]


@pytest.mark.parametrize("mode", MODES)
def test_train_cli_trains_checkpoints_resumes_and_refuses_other_centres(tmp_path, mode):
    follow_loss = lambda cfg: cfg.replace("monitor : 'val_map@r'", "monitor : 'loss'")     # a checkpoint after every epoch that trains
    out = _cli(tmp_path, mode, follow_loss)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch 2/2" in out.stdout and "saving model" in out.stdout and " - violating " in out.stdout
    assert (" - reg " in out.stdout) == (mode == "soft_triple")
    project = tmp_path / f"simple2_{mode}_synthetic"
    saved = sorted(os.listdir(project / "weights"))
    assert saved and saved == sorted(os.listdir(project / "optimizer")) == sorted(os.listdir(project / "proxies"))
    ck = np.load(project / "proxies" / saved[-1])
    kc = CLI_CENTERS[mode]
    assert ck["proxies"].shape == (10 * kc, 256) and int(ck["centers_per_class"]) == kc
    first = _losses(out.stdout)
    assert len(first) == 2 and saved[-1] == "epoch_002.npz", (saved, first)
    res = _cli(tmp_path, mode, follow_loss, extra=("--resume_from", str(project / "weights" / saved[-1])))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "resumed proxies from" in res.stdout and "resumed optimizer state" in res.stdout
    resumed = _losses(res.stdout)
    print(mode, "losses", first, "resumed", resumed)
    assert abs(resumed[0] - first[-1]) < abs(resumed[0] - first[0])       # it starts near the last loss, not near the initial one
    other = _cli(tmp_path, mode, lambda cfg: follow_loss(cfg).replace(f"centers: {kc}", f"centers: {kc + 1}"),
                 extra=("--resume_from", str(project / "weights" / saved[-1])))
    assert other.returncode != 0 and "centers_per_class" in other.stderr and "Epoch 1" not in other.stdout


@pytest.mark.parametrize("mode,edit,needle", [
    ("soft_triple", lambda c: c.replace("gamma: 0.1", "beta: 0.1"), "GENERATOR.proxy_loss"),
    ("soft_triple", lambda c: c.replace("centers: 10", "centers: 33"), "GENERATOR.proxy_loss"),
    ("arcface", lambda c: c.replace("margin: 0.5,", "margin: 1.6,"), "GENERATOR.proxy_loss"),
    ("arcface", lambda c: c.replace("mode : 'triplet'", "mode : 'siamese'"), "Siamese"),
    ("soft_triple", lambda c: c.replace("proxy_loss :", "xbm : {size: 64}\n  proxy_loss :"), "GENERATOR.xbm"),
    ("arcface", lambda c: c.replace("proxy_loss :", "xbm : {size: 64}\n  proxy_loss :"), "GENERATOR.xbm"),
], ids=["unknown key", "centers 33", "margin 1.6", "siamese", "xbm soft_triple", "xbm arcface"])
def test_train_cli_refuses_a_bad_config_before_training(tmp_path, mode, edit, needle):
    out = _cli(tmp_path, mode, edit)
    assert out.returncode != 0
    assert needle in out.stderr and "Epoch 1" not in out.stdout


def test_a_proxy_anchor_checkpoint_without_the_key_still_resumes(tmp_path):
    """A proxies file as it was written before centers_per_class existed, built by hand."""
    cfg = open(os.path.join(ROOT, "configs", "simple2_proxy_anchor_synthetic.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(cfg.replace("n_batches : 20", "n_batches : 4").replace("monitor : 'val_map@r'", "monitor : 'loss'"))
    run = lambda *extra: subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path), "--synthetic", "10",
                                         "--max_epochs", "1", *extra], capture_output=True, text=True, timeout=600)
    out = run()
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    project = tmp_path / "simple2_proxy_anchor_synthetic"
    name = sorted(os.listdir(project / "proxies"))[-1]
    ck = np.load(project / "proxies" / name)
    assert int(ck["centers_per_class"]) == 1
    np.savez(project / "proxies" / name, proxies=ck["proxies"], class_names=ck["class_names"])       # the old file: two keys
    assert "centers_per_class" not in np.load(project / "proxies" / name).files
    res = run("--resume_from", str(project / "weights" / name))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "resumed proxies from" in res.stdout and "Epoch 1/1" in res.stdout
