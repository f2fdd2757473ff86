"""Circle loss (ops.circle_loss: csrc/circle_loss.hip on csrc/pair_loss.h; ops.xbm_circle_loss: csrc/xbm.hip) against the float64
reference and the a-priori bounds of tests/circle_ref.py: values through ops and through the C ABI, the two forward paths against each
other, the ring criterion against the in-batch one, and both inside the training step (eager, graph-replayed, tools/train.py).

Every check prints its largest error / bound before it asserts ratio < 1 (the gradient's bound is one fp32 rounding of the result,
which a nearest rounding all but reaches).  Largest ratios observed on an MI355X, per group of checks:
  batch (grid, continuous, parameters, saturated, duplicates, C ABI)   free_share 0  G 0.163  loss 0.247  grad 0.998
  batch, rows of norm 30                                               free_share 0  G 2e-23  loss 0.096  grad 0.984
  ring (six cases, self slots, C ABI, long bank)                       free_share 0  G 0.12   loss 0.053  demb 0.944
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import circle_ref as C
import ms_ref as M
import supcon_ref
import xbm_ref as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = 0.75
PATHS = ["per_class", "similarity_matrix"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(x, p, k, dev, m=0.4, gamma=80.0, path="auto", g=None):
    from embeddingnet_amd import ops
    xt = x if torch.is_tensor(x) else torch.tensor(x, device=dev)
    xt = xt.detach().requires_grad_(True)
    mean, counts, gw = ops.circle_loss(xt, p, k, m, gamma, path=path, return_weights=True)
    mean.backward(None if g is None else torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), counts=counts.cpu().numpy(), G=gw.cpu().numpy(), grad=xt.grad.cpu().numpy(),
                mean_t=mean.detach().clone(), counts_t=counts.clone(), G_t=gw, grad_t=xt.grad)


@functools.lru_cache(maxsize=None)
def _continuous(p, k, e):
    x = C.continuous(p, k, e)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _grid(p, k, e, seed=None):
    x, unit = C.grid(p, k, e, seed)
    x.setflags(write=False)
    return x, unit


def _paths(p, k, e):
    return PATHS if C.auto_path(p, k, e) == "per_class" else PATHS[1:]


def _check(got, x, p, k, gs, m=0.4, gamma=80.0, g=1.0, what="", unit=None, counter=True):
    """Everything the header promises about one forward + backward, for a device whose S is within gs A of the truth: the three
    counters (the violating anchors and the negatives with alpha- > 0 between the sure and the possible count, at most 1 % free),
    every entry of G with its sign, exact zeros where the reference's alpha is surely 0, the loss and (from the device's own G)
    every gradient element.  -> {check: largest error / bound}."""
    n = p * k
    assert gs > 0 or M.exact_in_any_order(x, unit)                         # gamma_S = 0 only where S is exact in any order
    assert np.isfinite(got["G"]).all() and np.isfinite(got["grad"]).all() and np.isfinite(got["loss"])
    pos, neg = M.class_masks(p, k)
    assert not np.diag(got["G"]).any() and np.all(got["G"][pos] <= 0) and np.all(got["G"][neg] >= 0)
    assert got["counts"].dtype == np.int32 and got["counts"].shape == (3,) and got["counts"][0] == n * (k - 1)
    ref = C.reference(x, p, k, m, gamma)
    d = C.decisions(ref, gs)
    assert d["share"] <= C.FREE_CAP, d["share"]
    assert d["sure_neg"].sum() <= got["counts"][2] <= d["may_neg"].sum(), (got["counts"], d["sure_neg"].sum(), d["may_neg"].sum())
    assert not got["G"][neg & ~d["may_neg"]].any() and not got["G"][pos & ~d["may_pos"]].any()      # alpha surely 0: exactly 0
    if counter:
        v = supcon_ref.decisions(x, p, k, gs)
        assert v["open"].mean() <= 0.01
        assert v["sure"].sum() <= got["counts"][1] <= v["may"].sum(), (got["counts"], v["sure"].sum(), v["may"].sum())
    if gs == 0:
        assert np.array_equal(got["counts"], ref["counts"].astype(np.int32)), (got["counts"], ref["counts"])
    bg, _, bl = C.bounds(ref, gs)
    off = pos | neg
    ratios = dict(free_share=d["share"])
    ratios["G"] = float((np.abs(got["G"] - ref["G"])[off] / bg[off]).max())
    ratios["loss"] = float(abs(got["loss"] - ref["loss"]) / bl)
    want, bound = M.grad(x, got["G"], g)
    ratios["grad"] = float((np.abs(got["grad"] - want) / bound).max())
    print(f"circle {what} m={m} gamma={gamma} p={p} k={k} e={x.shape[1]} counts={got['counts']}: "
          + " ".join(f"{a}={b:.3g}" for a, b in ratios.items()))
    assert ratios["G"] < 1 and ratios["loss"] < 1 and ratios["grad"] < 1, ratios
    return ratios


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("p,k,e", C.BATCH_SHAPES, ids=str)
def test_values_on_grid_inputs_on_every_path_from_an_offset_pointer(dev, p, k, e):
    """S is exact in any order (test_circle_ref_cpu.py): the counters are exact and gamma_S = 0 in the bounds.  The block sits one
    float behind a 16-byte boundary (the dense GEMM's scalar loader)."""
    from embeddingnet_amd import _lib
    x, unit = _grid(p, k, e)
    buf = torch.zeros(p * k * e + 1, device=dev)
    xt = buf[1:].view(p * k, e)
    xt.copy_(torch.tensor(x))
    assert xt.data_ptr() % 16 == 4
    assert _lib.lib().embnet_circle_loss_path(p, k, e) == PATHS.index(C.auto_path(p, k, e)) + 1
    for path in _paths(p, k, e):
        r = _check(_run(xt, p, k, dev, path=path, g=UP), x, p, k, 0.0, unit=unit, g=UP, what="grid " + path)
        assert r["free_share"] == 0


@pytest.mark.parametrize("p,k,e", C.BATCH_SHAPES, ids=str)
def test_values_on_continuous_inputs_on_every_path(dev, p, k, e):
    x = _continuous(p, k, e)
    for path in _paths(p, k, e):
        _check(_run(x, p, k, dev, path=path, g=UP), x, p, k, C.continuous_gs(x, path, e), g=UP, what="continuous " + path,
               unit=1.0)


def test_forward_paths_agree_on_a_grid_input(dev):
    """The two paths differ in how S is summed; on an exact S the row body sees the same bits."""
    p, k, e = 8, 4, 256
    x, unit = _grid(p, k, e, seed=5)
    a, b = _run(x, p, k, dev, path="per_class"), _run(x, p, k, dev, path="similarity_matrix")
    assert a["loss"] == b["loss"] and np.array_equal(a["counts"], b["counts"])
    assert np.array_equal(a["G"], b["G"]) and np.array_equal(a["grad"], b["grad"])
    _check(a, x, p, k, 0.0, unit=unit, what="paths")


@pytest.mark.parametrize("m,gamma", C.PARAMS)
@pytest.mark.parametrize("path", PATHS)
def test_parameters(dev, path, m, gamma):
    p, k, e = 5, 7, 33
    x = _continuous(p, k, e)
    _check(_run(x, p, k, dev, m, gamma, path=path, g=UP), x, p, k, M.gamma_s(path, e), m, gamma, g=UP, what="params " + path)


@pytest.mark.parametrize("m,gamma", C.PARAMS)
@pytest.mark.parametrize("path", PATHS)
def test_unnormalised_rows_of_norm_30_stay_finite_and_within_bounds(dev, path, m, gamma):
    """S reaches 900 and a logit 10^8: e^a overflows fp32 and float64 alike, the stable forms do not."""
    p, k, e = 6, 4, 64
    x, unit = _grid(p, k, e, seed=3)
    x = (x * np.float32(30.0)).astype(np.float32)                   # still exact: S q^2 / 900 is an integer below 2^24 / 900
    ref = C.reference(x, p, k, m, gamma)
    assert np.abs(ref["logit"]).max() > 709 and np.isfinite(ref["loss"])
    _check(_run(x, p, k, dev, m, gamma, path=path), x, p, k, 0.0, m, gamma, unit=30.0 * unit, what="norm 30 " + path)


# ---------------------------------------------------------------------------------------------------------------- 2. edges
def _saturated():
    """Class 0 on (1, 0), every other row on (-1, 0) or (-0.6, 0.8): every negative of class 0's anchors has S <= -0.6 <= -m.
    (test_circle_ref_cpu.py works the reference's side of it by hand.)"""
    return np.array([[1, 0], [1, 0], [-1, 0], [-0.6, 0.8], [-0.6, 0.8], [-1, 0]], np.float32), 3, 2


@pytest.mark.parametrize("path", PATHS)
def test_a_saturated_side_has_exact_zeros_and_the_stated_loss(dev, path):
    x, p, k = _saturated()
    gs = M.gamma_s(path, 2)
    ref = C.reference(x, p, k)
    assert not C.decisions(ref, gs)["free"].any()                   # -0.6 and -1 are far from -0.4 at either path's gamma_S
    got = _run(x, p, k, dev, path=path, g=UP)
    _check(got, x, p, k, gs, g=UP, what="saturated " + path, counter=False)      # S = 1 twice: ties, which any gs > 0 calls open
    assert not got["G"][:2, 2:].any() and (got["G"][[0, 1], [1, 0]] < 0).all()
    assert got["counts"][2] == ref["counts"][2] == ref["count_neg"][2:].sum()
    # all of class 0's negatives saturated, every other anchor's too (their negatives are class 0 at S <= -0.6 or each other at
    # S >= 0.6): the counter holds only the latter
    assert not ref["count_neg"][:2].any()


def test_duplicate_rows(dev):
    p, k, e = 5, 4, 32
    x, unit = _grid(p, k, e, seed=8)
    x = x.copy()
    x[1::k] = x[0::k]                                               # rows 0 and 1 of every class coincide
    _check(_run(x, p, k, dev), x, p, k, 0.0, unit=unit, what="duplicates")


@pytest.mark.parametrize("p,k,e", [(1, 4, 16), (4, 1, 16), (2, 2049, 4), (4, 4, 4097), (4, 32, 16)])
def test_out_of_range_shapes_raise(dev, p, k, e):
    from embeddingnet_amd import _lib, ops
    x = torch.rand((p * k, e), device=dev)
    with pytest.raises(_lib.EmbnetError):
        ops.circle_loss(x, p, k, path="per_class" if (p, k) == (4, 32) else "auto")
    with pytest.raises(_lib.EmbnetError):
        ops.circle_loss(x, p + 1, k)                                # rows != p*k


@pytest.mark.parametrize("m,gamma", [(-0.1, 80.0), (1.5, 80.0), (0.4, 0.0), (float("nan"), 80.0), (0.4, float("nan")),
                                     (0.4, float("inf"))])
def test_out_of_range_parameters_raise_before_a_launch(dev, m, gamma):
    from embeddingnet_amd import _lib, ops
    x = torch.rand((8, 4), device=dev)
    lab = torch.arange(4, device=dev, dtype=torch.int32).repeat_interleave(2)
    _lib.trace_reset()
    _lib.trace_enable(True)
    try:
        with pytest.raises(_lib.EmbnetError, match="circle_loss_fwd"):
            ops.circle_loss(x, 4, 2, m, gamma)
        with pytest.raises(_lib.EmbnetError, match="xbm_circle_loss_fwd"):
            ops.xbm_circle_loss(x, lab, x.clone(), lab.clone(), None, m, gamma)
        assert _lib.trace_records() == []                           # no kernel was launched
    finally:
        _lib.trace_enable(False)


def _raw(xt, p, k, path, pad, m=0.4, gamma=80.0, stream=None, fill_ff=False):
    """The C ABI directly on buffers with `pad` guard elements on either side.  -> (G, demb, counts, mean, ws) guarded tensors."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    n, e = xt.shape
    dev = xt.device
    wsn = lib.embnet_circle_loss_workspace_bytes(p, k, e) // 4
    gb = torch.full((2 * pad + n * n,), float("nan"), device=dev)
    if fill_ff:
        gb.view(torch.int32).fill_(-1)                              # 0xFF bytes
    db = torch.full((2 * pad + n * e,), float("nan"), device=dev)
    cb = torch.full((2 * pad + 3,), -12345, dtype=torch.int32, device=dev)
    mb = torch.full((2 * pad + 1,), float("nan"), device=dev)
    wb = torch.full((2 * pad + wsn,), float("nan"), device=dev)
    wb[pad:pad + wsn] = 0
    up = torch.tensor(UP, device=dev)
    torch.cuda.synchronize()
    s = _lib.stream() if stream is None else stream.cuda_stream
    sl = lambda t, cnt: t[pad:pad + cnt]
    _lib.check(lib.embnet_circle_loss_fwd(xt.data_ptr(), p, k, e, m, gamma, path, sl(gb, n * n).data_ptr(), sl(cb, 3).data_ptr(),
                                          sl(mb, 1).data_ptr(), sl(wb, wsn).data_ptr(), wsn * 4, s))
    _lib.check(lib.embnet_ms_loss_bwd(xt.data_ptr(), n, e, sl(gb, n * n).data_ptr(), up.data_ptr(), sl(db, n * e).data_ptr(), s))
    torch.cuda.synchronize()
    return gb, db, cb, mb, wb


@pytest.mark.parametrize("path", [1, 2])
def test_the_c_abi_gives_the_same_values_and_writes_nothing_outside_the_outputs(dev, path):
    p, k, e, pad = 5, 7, 33, 64                                     # N = 35: ragged tiles in every kernel
    x, unit = _grid(p, k, e)
    gb, db, cb, mb, wb = _raw(torch.tensor(x, device=dev), p, k, path, pad)
    for t in (gb, db, mb, wb):
        assert torch.isnan(t[:pad]).all() and torch.isnan(t[-pad:]).all()
        assert torch.isfinite(t[pad:-pad]).all()                    # all n*n entries of G are written
    assert (cb[:pad] == -12345).all() and (cb[-pad:] == -12345).all()
    assert wb[pad].view(torch.int32).item() == 0                    # the ticket is re-armed
    n = p * k
    raw = dict(loss=mb[pad].item(), counts=cb[pad:-pad].cpu().numpy(), G=gb[pad:-pad].view(n, n).cpu().numpy(),
               grad=db[pad:-pad].view(n, e).cpu().numpy())
    _check(raw, x, p, k, 0.0, g=UP, unit=unit, what=f"C ABI path {path}")
    got = _run(x, p, k, dev, path=PATHS[path - 1], g=UP)
    assert np.array_equal(raw["G"], got["G"]) and np.array_equal(raw["grad"], got["grad"])
    assert np.array_equal(raw["counts"], got["counts"]) and raw["loss"] == got["loss"]


# ---------------------------------------------------------------------------------------------------------------- 3. reproducible
@pytest.mark.parametrize("p,k,e", [(32, 4, 256), (256, 8, 128)], ids=str)
def test_bitwise_reproducible(dev, p, k, e):
    from recipes import clustered_embeddings
    x = clustered_embeddings(4, p, k, e, 0.7)
    r1, r2 = _run(x, p, k, dev, g=UP), _run(x, p, k, dev, g=UP)
    for key in ("mean_t", "counts_t", "G_t", "grad_t"):
        assert torch.equal(r1[key], r2[key]), key
    assert np.isfinite(r1["loss"]) and r1["loss"] > 0 and np.abs(r1["grad"]).max() > 0
    # a second stream, its own workspace, a G buffer full of 0xFF bytes
    n = p * k
    s2 = torch.cuda.Stream(device=dev)
    gb, db, cb, mb, _ = _raw(torch.tensor(x, device=dev), p, k, 0, 16, stream=s2, fill_ff=True)
    assert torch.equal(gb[16:-16].view(n, n), r1["G_t"]) and torch.equal(db[16:-16].view(n, e), r1["grad_t"])
    assert torch.equal(cb[16:-16], r1["counts_t"]) and torch.equal(mb[16], r1["mean_t"])


# ---------------------------------------------------------------------------------------------------------------- 4. the ring
@functools.lru_cache(maxsize=None)
def _case(name):
    return C.ring_case(name)


def _xrun(c, dev, m=0.4, gamma=80.0, g=None):
    from embeddingnet_amd import ops
    t = lambda a: None if a is None else torch.tensor(a, device=dev)
    xt = t(c["x"]).requires_grad_(True)
    mean, counts, gw = ops.xbm_circle_loss(xt, t(c["labels"]), t(c["mem"]), t(c["mem_labels"]), t(c["self_slots"]), m, gamma,
                                           return_weights=True)
    mean.backward(None if g is None else torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), counts=counts.cpu().numpy(), G=gw.cpu().numpy(), demb=xt.grad.cpu().numpy(),
                t=(mean.detach().clone(), counts.clone(), gw, xt.grad))


def _xcheck(got, c, gs, m=0.4, gamma=80.0, g=1.0, what=""):
    """The ring criterion's promises: zero G outside every set and on inactive anchors, signs, exact zeros where alpha is surely 0,
    the four counters (the two alpha > 0 counts between sure and possible), every entry of G, the loss, and from the device's own
    G every element of demb; no gradient on unlabelled or inactive rows."""
    x, lab, mem, mlab, slots = c["x"], c["labels"], c["mem"], c["mem_labels"], c["self_slots"]
    n, slots_n = x.shape[0], mem.shape[0]
    assert gs > 0 or X.exact_in_any_order(x, mem, c["unit"])
    assert got["G"].shape == (n, slots_n) and got["counts"].dtype == np.int32 and got["counts"].shape == (4,)
    assert np.isfinite(got["G"]).all() and np.isfinite(got["demb"]).all() and np.isfinite(got["loss"])
    ref = C.xbm_reference(x, lab, mem, mlab, slots, m, gamma)
    pos, neg = ref["pos"], ref["neg"]                               # restricted to the active anchors
    assert not got["G"][~(pos | neg)].any() and np.all(got["G"][pos] <= 0) and np.all(got["G"][neg] >= 0)
    d = C.decisions(ref, gs)
    assert d["share"] <= C.FREE_CAP, d["share"]
    assert d["sure_pos"].sum() <= got["counts"][0] <= d["may_pos"].sum() and d["sure_neg"].sum() <= got["counts"][1] <= d["may_neg"].sum()
    assert got["counts"][2:].tolist() == ref["counts"][2:].tolist(), (got["counts"], ref["counts"])
    assert not got["G"][neg & ~d["may_neg"]].any() and not got["G"][pos & ~d["may_pos"]].any()
    if not d["free"].any():
        assert np.array_equal(got["counts"], ref["counts"].astype(np.int32)), (got["counts"], ref["counts"])
    bg, _, bl = C.bounds(ref, gs)
    pair = pos | neg
    ratios = dict(free_share=d["share"])
    ratios["G"] = float((np.abs(got["G"] - ref["G"])[pair] / bg[pair]).max()) if pair.any() else 0.0
    ratios["loss"] = float(abs(got["loss"] - ref["loss"]) / bl) if bl > 0 else float(got["loss"] != 0)
    want, bound = X.grad(mem, got["G"], g)
    ratios["demb"] = float((np.abs(got["demb"] - want) / bound).max())
    assert not got["demb"][~ref["active"]].any()
    print(f"xbm circle {what} m={m} gamma={gamma} n={n} slots={slots_n} e={x.shape[1]} counts={got['counts']}: "
          + " ".join(f"{a}={b:.3g}" for a, b in ratios.items()))
    assert ratios["G"] < 1 and ratios["loss"] < 1 and ratios["demb"] < 1, ratios
    return ratios


@pytest.mark.parametrize("m,gamma", C.PARAMS[:2])
@pytest.mark.parametrize("name", C.RING_CASES)
def test_ring_values(dev, name, m, gamma):
    c = _case(name)
    gs = X.gamma_s(c["x"].shape[1], c["unit"] is not None)
    first = _xrun(c, dev, m, gamma)
    _xcheck(first, c, gs, m, gamma, what=name)
    second = _xrun(c, dev, m, gamma, g=UP)                          # upstream != 1, and two runs bitwise equal
    _xcheck(second, c, gs, m, gamma, g=UP, what=name + " upstream")
    for a, b in zip(first["t"][:3], second["t"][:3]):
        assert torch.equal(a, b)
    assert torch.equal(second["t"][3], _xrun(c, dev, m, gamma, g=UP)["t"][3])


def test_a_bank_that_is_the_batch_agrees_with_the_in_batch_circle_loss(dev):
    c = _case("bank_is_batch")
    n, _, e = X.SHAPES["bank_is_batch"]
    got = _xrun(c, dev)
    mine = _run(c["x"], 4, 2, dev)
    ref, want = C.xbm_reference(c["x"], c["labels"], c["mem"], c["mem_labels"], c["self_slots"]), C.reference(c["x"], 4, 2)
    gs_in = M.gamma_s(C.auto_path(4, 2, e), e)
    assert not C.decisions(want, gs_in)["free"].any() and not C.decisions(ref, X.gamma_s(e))["free"].any()
    assert got["counts"][1] == mine["counts"][2] and got["counts"][2:].tolist() == [n, n]
    bound = C.bounds(ref, X.gamma_s(e))[2] + C.bounds(want, gs_in)[2]
    err = abs(got["loss"] - mine["loss"])
    print("xbm circle vs in-batch circle: |difference| / (sum of both bounds)", err / bound)
    assert err < bound
    bg = C.bounds(ref, X.gamma_s(e))[0] + C.bounds(want, gs_in)[0]
    off = ~np.eye(n, dtype=bool)
    assert (np.abs(got["G"] - mine["G"])[off] < bg[off]).all()


def test_no_self_slots_and_out_of_range_self_slots_exclude_nothing(dev):
    c = dict(_case("ragged"))
    for slots in (None, np.full(12, -1, np.int32), np.array([40, 41, 1 << 30, -5] * 3, np.int32)):
        c["self_slots"] = slots
        _xcheck(_xrun(c, dev, g=UP), c, X.gamma_s(5), g=UP, what="self_slots " + ("None" if slots is None else str(slots[:4])))


def test_all_unlabelled_gives_zero_loss_and_zero_weights(dev):
    c = dict(_case("ragged"))
    lab = np.full(12, -1, np.int32)
    lab[3], lab[5] = np.iinfo(np.int32).min, -2
    c["labels"] = lab
    got = _xrun(c, dev, g=UP)
    assert got["loss"] == 0.0 and not got["G"].any() and not got["demb"].any()
    assert got["counts"].tolist() == [0, 0, 0, int((c["mem_labels"] >= 0).sum())]


def test_ring_c_abi_writes_nothing_outside_the_outputs_and_rearms_its_ticket(dev):
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    c = _case("long")
    (n, e), slots_n, pad = c["x"].shape, c["mem"].shape[0], 64
    t = lambda a, dt=None: torch.tensor(a, device=dev, dtype=dt)
    x, lab, mem, mlab, own = t(c["x"]), t(c["labels"]), t(c["mem"]), t(c["mem_labels"]), t(c["self_slots"])
    wsn = lib.embnet_xbm_loss_workspace_bytes(n, slots_n, e) // 4
    gb = torch.full((2 * pad + n * slots_n,), float("nan"), device=dev)
    db = torch.full((2 * pad + n * e,), float("nan"), device=dev)
    cb = torch.full((2 * pad + 4,), -12345, dtype=torch.int32, device=dev)
    mb = torch.full((2 * pad + 1,), float("nan"), device=dev)
    wb = torch.full((2 * pad + wsn,), float("nan"), device=dev)
    wb[pad:pad + wsn] = 0
    up = torch.tensor(UP, device=dev)
    torch.cuda.synchronize()
    sl = lambda v, cnt: v[pad:pad + cnt].data_ptr()
    _lib.check(lib.embnet_xbm_circle_loss_fwd(x.data_ptr(), lab.data_ptr(), mem.data_ptr(), mlab.data_ptr(), own.data_ptr(), n, slots_n, e,
                                              0.4, 80.0, sl(gb, n * slots_n), sl(cb, 4), sl(mb, 1), sl(wb, wsn), wsn * 4, _lib.stream()))
    torch.cuda.synchronize()
    assert wb[pad].view(torch.int32).item() == 0                    # before the backward takes the workspace as scratch
    _lib.check(lib.embnet_xbm_loss_bwd(mem.data_ptr(), n, slots_n, e, sl(gb, n * slots_n), up.data_ptr(), sl(db, n * e), sl(wb, wsn),
                                       wsn * 4, _lib.stream()))
    torch.cuda.synchronize()
    for v in (gb, db, mb, wb):
        assert torch.isnan(v[:pad]).all() and torch.isnan(v[-pad:]).all()
    assert torch.isfinite(gb[pad:-pad]).all() and torch.isfinite(db[pad:-pad]).all()
    assert (cb[:pad] == -12345).all() and (cb[-pad:] == -12345).all()
    raw = dict(loss=mb[pad].item(), counts=cb[pad:-pad].cpu().numpy(), G=gb[pad:-pad].view(n, slots_n).cpu().numpy(),
               demb=db[pad:-pad].view(n, e).cpu().numpy())
    _xcheck(raw, c, X.gamma_s(e), g=UP, what="C ABI")
    got = _xrun(c, dev, g=UP)
    assert np.array_equal(raw["G"], got["G"]) and np.array_equal(raw["demb"], got["demb"]) and raw["loss"] == got["loss"]


def test_the_long_bank_backward_takes_two_launches_at_512_slots(dev):
    """512 slots is the least the backward splits (two slices of 256): its kernels' names in the trace, the values as ever."""
    from embeddingnet_amd import _lib
    n, slots_n, e = 4, 512, 8
    x, lab, mem, mlab, own = X._split(5120, 2, 2, slots_n, e, cursor=500, empty=3)
    c = dict(x=x, labels=lab, mem=mem, mem_labels=mlab, self_slots=own, unit=None)
    _lib.trace_reset()
    _lib.trace_enable(True)
    try:
        got = _xrun(c, dev, g=UP)
        names = [r[0] for r in _lib.trace_records()]
    finally:
        _lib.trace_enable(False)
    assert any("xbm_circle_sweep_kernel" in s for s in names), names
    assert any("xbm_bwd_part_kernel" in s for s in names) and any("xbm_bwd_sum_kernel" in s for s in names), names
    _xcheck(got, c, X.gamma_s(e), g=UP, what="long bank")


# ---------------------------------------------------------------------------------------------------------------- 5. training
def _trainer(dev, graph, cls="triplet", seed=5, **kw):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer, XbmTrainer
    from embeddingnet_amd.xbm import CrossBatchMemory
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=seed, device=dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-3)
    if cls == "triplet":
        return base, None, TripletTrainer(base, opt, 8, 4, negatives_selection_mode="circle", seed=3, graph=graph, **kw)
    memory = CrossBatchMemory(96, 64, dev)
    return base, memory, XbmTrainer(base, opt, 8, 4, negatives_selection_mode="circle", seed=3, graph=graph, memory=memory,
                                    xbm_loss="circle", **kw)


def _batches(dev, steps):
    """Class prototypes plus noise: 8 of 12 classes x 4 samples, class-contiguous, with their labels."""
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((12, 64, 64, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(12, generator=torch.Generator().manual_seed(i))[:8].to(dev)
        x = protos[cls].repeat_interleave(4, 0) + 0.15 * torch.randn((32, 64, 64, 3), device=dev, generator=gen)
        yield x.clamp(0, 1), cls.repeat_interleave(4).to(torch.int32)


def _weights(base):
    return torch.cat([q.detach().reshape(-1) for q in base.parameters()])


def test_trainer_circle_learns(dev):
    """30 steps on the backbone's raw embeddings (unit rows are not required).  The thresholds are the run's own start: the loss of
    the last five steps stays below the first, and the violating anchors of the last five steps below those of the first five."""
    _, _, tr = _trainer(dev, graph=False)
    losses, viol = [], []
    for x, _ in _batches(dev, 30):
        losses.append(float(tr.step(x).item()))
        trip, count = tr.last_triplets
        assert trip is None and count.dtype == torch.int32 and count.shape == (1,)
        assert tr.last_pair_counts.shape == (3,) and int(tr.last_pair_counts[1]) == int(count)
        assert int(tr.last_pair_counts[0]) == 32 * 3
        viol.append(int(count))
    print("circle trainer losses", [round(v, 4) for v in losses], "violating anchors", viol)
    assert np.all(np.isfinite(losses))
    assert max(losses[-5:]) < losses[0], losses
    assert sum(viol[-5:]) < sum(viol[:5]), viol


def test_trainer_circle_graph_replay_equals_eager(dev):
    from embeddingnet_amd import _lib
    runs = []
    for graph in (False, True):
        base, _, tr = _trainer(dev, graph=graph, loss_params=dict(m=0.25, gamma=64.0))
        losses, counts = [], []
        for i, (x, _) in enumerate(_batches(dev, 14)):
            if graph and i == 11:
                _lib.trace_enable(True)                             # an eager step between replays
            losses.append(tr.step(x).clone())
            _lib.trace_enable(False)
            assert tr.last_triplets[1].data_ptr() == tr.last_pair_counts.data_ptr() + 4
            counts.append(tr.last_pair_counts.clone())
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        runs.append((torch.stack(losses), torch.stack(counts), _weights(base)))
    for a, b in zip(*runs):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()


def test_xbm_trainer_circle_graph_replay_equals_eager(dev):
    from embeddingnet_amd import _lib
    from embeddingnet_amd.train_step import TripletTrainer
    steps = TripletTrainer.GRAPH_WARMUP + 8
    runs = []
    for graph in (False, True):
        base, memory, tr = _trainer(dev, graph=graph, cls="xbm", start_iteration=2, xbm_params=dict(m=0.25))
        losses, counts = [], []
        for i, (x, y) in enumerate(_batches(dev, steps)):
            if graph and i == steps - 3:
                _lib.trace_enable(True)                             # an eager step between replays
            losses.append(tr.step(x, y).clone())
            _lib.trace_enable(False)
            if i < 2:
                assert tr.last_xbm_counts is None and tr._graph is None
            else:
                counts.append(tr.last_xbm_counts.clone())
                assert int(tr.last_xbm_counts[3]) == min(96, 32 * (i - 1))       # the ring fills, then stays full (it wraps)
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        runs.append((torch.stack(losses), torch.stack(counts), _weights(base), memory.feats.clone(), memory.labels.clone(),
                     memory.cursor.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()
    assert runs[0][1][:, 2].max() > 0                               # the memory had active anchors


def test_before_start_iteration_the_xbm_step_is_the_parents(dev):
    runs = []
    for cls in ("triplet", "xbm"):
        base, memory, tr = _trainer(dev, graph=False, cls=cls, **(dict(start_iteration=1000) if cls == "xbm" else {}))
        losses = [(tr.step(x) if cls == "triplet" else tr.step(x, y)).clone() for x, y in _batches(dev, 5)]
        runs.append((torch.stack(losses), _weights(base)))
        if memory is not None:
            assert memory.filled() == 0 and memory.cursor.item() == 0 and tr.last_xbm_counts is None
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 6. CLI
def _cli(tmp_path, name, edit=lambda cfg: cfg, classes=10):
    cfg = open(os.path.join(ROOT, "configs", name + ".yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert "negatives_selection_mode : 'circle'" in cfg and "n_batches : 20" in cfg and "circle_loss :" in cfg
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(edit(cfg.replace("n_batches : 20", "n_batches : 4")))
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path), "--synthetic", str(classes),
                           "--max_epochs", "2"], capture_output=True, text=True, timeout=600)


def test_train_cli_circle_config(tmp_path):
    out = _cli(tmp_path, "simple2_circle_synthetic")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch 2/2" in out.stdout and "saving model" in out.stdout and "violating" in out.stdout
    assert any(f.startswith("epoch_") for f in os.listdir(tmp_path / "simple2_circle_synthetic" / "weights"))


def test_train_cli_xbm_circle_config(tmp_path):
    """4 batches of 32 per epoch, the memory live from step 2: 2 batches after the first epoch, 6 after the second."""
    out = _cli(tmp_path, "simple2_xbm_circle_synthetic", lambda cfg: cfg.replace("start_iteration: 20", "start_iteration: 2"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    filled = [int(v) for v in re.findall(r"xbm_filled (\d+)", out.stdout)]
    assert filled == [64, 192] and "xbm_kept" in out.stdout and "Epoch 2/2" in out.stdout, out.stdout[-2000:]


def test_train_cli_refuses_circle_loss_with_another_mode(tmp_path):
    out = _cli(tmp_path, "simple2_circle_synthetic", lambda cfg: cfg.replace("'circle'", "'semihard'"))
    assert out.returncode != 0
    assert "GENERATOR.circle_loss" in out.stderr and "circle" in out.stderr and "Epoch 1" not in out.stdout
