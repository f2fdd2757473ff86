"""Distance-weighted sampling and the margin loss (ops.margin_loss: csrc/margin_loss.hip on csrc/pair_loss.h) against the float64
reference and the a-priori bounds of tests/margin_ref.py: the picks by the interval rule on the device's OWN weights, the weights
against float64 relative to the device's own maximal column, loss / counts / pair weights / gradient given the device's picks,
through ops and through the C ABI, the two forward paths against each other, and the mode inside the training step (eager,
graph-replayed, tools/train.py).

Every check prints its largest error / bound before it asserts ratio <= 1 (the gradient's bound is one fp32 rounding of the result,
which a nearest rounding all but reaches).  Largest ratios observed on an MI355X, per group of checks:
  sampling weights (11 shapes, both paths)                      0.129; 100 weights underflowed to 0 at E = 512, inside their bound
  values (signed, grid, parameter sets, edges, C ABI)           loss 0.073  W 0.369  grad 0.998; no open hinge, counters exact
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import margin_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = 0.75
SEED = 20171
PARAM_SETS = dict(test=R.TEST_PARAMS, defaults=R.DEFAULTS, alpha0=dict(R.TEST_PARAMS, alpha=0.0))
CASES = [(s, path) for s in R.SHAPES for path in R.paths(*s)]
WEIGHT_CASES = CASES + [(s, path) for s in R.WEIGHT_SHAPES for path in R.paths(*s)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(x, p, k, dev, params=R.TEST_PARAMS, seed=SEED, path="auto", g=None, seed_dev=None):
    from embeddingnet_amd import ops
    xt = x if torch.is_tensor(x) else torch.tensor(x, device=dev)
    xt = xt.detach().requires_grad_(True)
    mean, counts, trip, w, sw = ops.margin_loss(xt, p, k, **params, seed=seed, seed_dev=seed_dev, path=path, return_weights=True)
    mean.backward(None if g is None else torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), counts=counts.cpu().numpy(), trip=trip.cpu().numpy(), W=w.cpu().numpy(), SW=sw.cpu().numpy(),
                grad=xt.grad.cpu().numpy(), mean_t=mean.detach().clone(), counts_t=counts.clone(), trip_t=trip, W_t=w, SW_t=sw,
                grad_t=xt.grad)


@functools.lru_cache(maxsize=None)
def _signed(p, k, e):
    x = R.weight_input(p, k, e) if (p, k, e) in R.WEIGHT_SHAPES else R.signed(p, k, e)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _grid(p, k, e):
    x, unit = R.grid(p, k, e)
    x.setflags(write=False)
    return x, unit


@functools.lru_cache(maxsize=None)
def _dist(p, k, e, path, grid=False):
    """The float64 distances and their admissible interval on `path`, computed once per case and shared."""
    x, unit = _grid(p, k, e) if grid else (_signed(p, k, e), None)
    return R.distances(x, R.error_class(x, path, unit))


@functools.lru_cache(maxsize=None)
def _device(p, k, e, path, grid=False, params="test"):
    """One device run per case, shared by the tests that read it (the GPU is not handed to lru_cache: the module's one device)."""
    x = _grid(p, k, e)[0] if grid else _signed(p, k, e)
    return _run(x, p, k, torch.device("cuda:0"), PARAM_SETS[params], path=path, g=UP)


# ---------------------------------------------------------------------------------------------------------------- 1. picks
def _check_picks(got, p, k, seed, what):
    n = p * k
    trip, sw = got["trip"], got["SW"]
    assert trip.shape == (n * (k - 1), 3) and trip.dtype == np.int32
    rows = trip.reshape(n, k - 1, 3)
    fallback = 0
    for i in range(n):
        assert rows[i, :, 0].tolist() == [i] * (k - 1) and rows[i, :, 1].tolist() == R.positives(i, k), (what, i)
        total = sw[i].astype(np.float64).sum()
        for j in range(k - 1):
            u, pick = R.draw_u(seed, i, j), int(rows[i, j, 2])
            assert 0 <= pick < n and pick // k != i // k, (what, i, j, pick)
            if total == 0.0:
                fallback += 1
                assert pick == R.fallback_pick(u, i, n, k), (what, i, j, pick)
            else:
                assert R.pick_acceptable(sw[i], u, pick), (what, i, j, pick, u)
    return fallback


@pytest.mark.parametrize("shape,path", CASES, ids=str)
def test_picks_follow_the_interval_rule_on_the_devices_own_weights(dev, shape, path):
    p, k, e = shape
    fallback = _check_picks(_device(p, k, e, path), p, k, SEED, (shape, path))
    dist = _dist(p, k, e, path)
    if dist["exact"]:                                        # rows of +-1: an anchor with every negative at D = 2 falls back
        _, elig = R.weights64(dist, p, k, e, R.params32(**R.TEST_PARAMS))
        assert fallback == int((~elig.any(1)).sum()) * (k - 1)


# ---------------------------------------------------------------------------------------------------------------- 2. weights
def _check_weights(got, dist, p, k, e, par, what):
    dec = R.decisions(dist, p, k, par)
    sw = got["SW"].astype(np.float64)
    n = p * k
    assert not sw[~dec["elig_may"]].any(), what             # own class, the anchor, sure-ineligible columns: exactly 0
    assert np.isfinite(sw).all() and sw.min() >= 0 and sw.max() <= 1
    live = sw.max(1) > 0
    assert live[dec["elig_sure"].any(1)].all() and not live[~dec["elig_may"].any(1)].any(), what
    assert (sw.max(1)[live] == 1.0).all(), what              # the row's maximum is exactly 1
    top = sw.argmax(1)
    w64, bound = R.weight_bound(dist, e, par, top)
    err = np.abs(sw - w64)
    sure = dec["elig_sure"] & live[:, None]
    open_ = dec["elig_may"] & ~dec["elig_sure"] & live[:, None]
    ratio = float((err[sure] / bound[sure]).max()) if sure.any() else 0.0
    under = int((sure & (sw == 0)).sum())
    print(f"margin weights {what}: err/bound {ratio:.3g}, open {int(open_.sum())}, underflowed to 0: {under}, fall-back rows {int((~live).sum())}")
    assert ratio <= 1.0, what
    assert ((sw[open_] == 0) | (err[open_] <= bound[open_])).all(), what
    return under


@pytest.mark.parametrize("shape,path", WEIGHT_CASES, ids=str)
def test_sampling_weights(dev, shape, path):
    p, k, e = shape
    under = _check_weights(_device(p, k, e, path), _dist(p, k, e, path), p, k, e, R.params32(**R.TEST_PARAMS), (shape, path))
    if e == 512:
        assert under > 0                                     # weights underflow there, and an underflowed weight is within its bound
    _check_picks(_device(p, k, e, path), p, k, SEED, (shape, path))


# ---------------------------------------------------------------------------------------------------------------- 3. values
def _check_values(got, x, dist, p, k, par, what, g=UP, grad=None):
    n = p * k
    dec = R.decisions(dist, p, k, par)
    ref = R.reference(dist, p, k, par, got["trip"])
    cp, cn, a = (int(v) for v in got["counts"])
    draws = ref["draws"]
    assert int(dec["pos_sure"].sum()) <= cp <= int(dec["pos_may"].sum()), what
    assert int((draws * dec["neg_sure"]).sum()) <= cn <= int((draws * dec["neg_may"]).sum()), what
    assert a == cp + cn, what
    loss, bl = R.loss_and_bound(ref, a)
    r_loss = abs(got["loss"] - loss) / bl
    w = got["W"].astype(np.float64)
    assert np.isfinite(w).all() and not w[np.eye(n, dtype=bool)].any(), what
    pair = dec["pos"] | (draws > 0)
    assert not w[~pair].any(), what                          # everything else is 0
    sure = (dec["pos"] & dec["pos_sure"]) | ((draws > 0) & dec["neg_sure"])
    may = (dec["pos"] & dec["pos_may"]) | ((draws > 0) & dec["neg_may"])
    assert not w[pair & ~may].any(), what                    # a surely inactive hinge weighs exactly 0
    zero = dist["Dhi"] == 0                                  # coincident rows on an exact d2: no direction
    assert not w[zero].any(), what
    free = (dist["Dlo"] <= 0) & ~zero                        # D may round to 0 or to anything small (Gram form): finite, no bound
    judged = sure & ~zero & ~free
    err = np.abs(w - ref["W_on"])
    r_w = float((err[judged] / ref["bound_W"][judged]).max()) if judged.any() else 0.0
    open_ = pair & may & ~sure & ~zero & ~free
    assert ((w[open_] == 0) | (err[open_] <= ref["bound_W"][open_])).all(), what
    want, bd = R.demb(x, w, a, g)
    grad = got["grad"] if grad is None else grad
    assert np.isfinite(grad).all(), what
    r_g = float((np.abs(grad - want) / bd).max())
    print(f"margin values {what}: loss {r_loss:.3g} W {r_w:.3g} grad {r_g:.3g}; counts {cp}+{cn}, open hinges {int(open_.sum())}")
    assert r_loss <= 1 and r_w <= 1 and r_g <= 1, what
    return ref


@pytest.mark.parametrize("shape,path", CASES, ids=str)
def test_values_given_the_devices_picks(dev, shape, path):
    p, k, e = shape
    _check_values(_device(p, k, e, path), _signed(p, k, e), _dist(p, k, e, path), p, k, R.params32(**R.TEST_PARAMS), (shape, path))


@pytest.mark.parametrize("params", ["defaults", "alpha0"])
@pytest.mark.parametrize("shape", [(9, 8, 40), (4, 32, 16), (32, 4, 256)], ids=str)
def test_values_at_the_default_parameters_and_at_alpha_zero(dev, shape, params):
    p, k, e = shape
    for path in R.paths(p, k, e):
        got = _device(p, k, e, path, params=params)
        _check_values(got, _signed(p, k, e), _dist(p, k, e, path), p, k, R.params32(**PARAM_SETS[params]), (shape, path, params))
        _check_picks(got, p, k, SEED, (shape, path, params))


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_grid_inputs_are_exact_and_the_two_paths_agree_bit_for_bit(dev, shape):
    p, k, e = shape
    x, _ = _grid(p, k, e)
    runs = [_device(p, k, e, path, grid=True) for path in R.paths(p, k, e)]
    par = R.params32(**R.TEST_PARAMS)
    for path, got in zip(R.paths(p, k, e), runs):
        dist = _dist(p, k, e, path, grid=True)
        assert dist["exact"] and R.decisions(dist, p, k, par)["share"] <= R.OPEN_CAP      # (sqrtf's own rounding can still open one)
        _check_picks(got, p, k, SEED, (shape, path, "grid"))
        _check_values(got, x, dist, p, k, par, (shape, path, "grid"))
    for other in runs[1:]:
        for key in ("trip", "counts", "W", "SW"):
            assert np.array_equal(runs[0][key], other[key]), key


# ---------------------------------------------------------------------------------------------------------------- 4. edges
@pytest.mark.parametrize("path", ["per_class", "distance_matrix"])
def test_duplicate_rows_weigh_nothing_are_counted_and_stay_finite(dev, path):
    p, k, e = 5, 7, 33
    x = _grid(p, k, e)[0].copy()
    x[1] = x[0]                                              # a coincident positive
    x[k] = x[0]                                              # a coincident negative: eligible, at the clamp's weight
    x[2 * k:3 * k] = x[2 * k]                                # a class of one point
    unit = _grid(p, k, e)[1]
    dist = R.distances(x, R.error_class(x, path, unit))
    assert dist["exact"] and dist["D"][0, 1] == 0 and dist["D"][0, k] == 0
    par = R.params32(beta=0.3, alpha=0.4, cutoff=0.5, nonzero_loss_cutoff=1.4)       # D = 0 pays beta - 0 + alpha > 0, and 0 - beta + alpha > 0
    got = _run(x, p, k, dev, dict(beta=0.3, alpha=0.4, cutoff=0.5, nonzero_loss_cutoff=1.4), path=path, g=UP)
    ref = _check_values(got, x, dist, p, k, par, ("duplicates", path))
    _check_picks(got, p, k, SEED, ("duplicates", path))
    assert got["SW"][0, k] > 0 and got["W"][0, 1] == 0 and got["W"][0, k] == 0 and got["W"][1, 0] == 0
    assert ref["lp"][0, 1] > 0 and int(got["counts"][0]) == ref["cp"] and int(got["counts"][1]) == ref["cn"]      # counted all the same
    assert not got["W"][2 * k:3 * k, 2 * k:3 * k].any() and np.isfinite(got["grad"]).all() and np.isfinite(got["loss"])


@pytest.mark.parametrize("path", ["per_class", "distance_matrix"])
def test_two_antipodal_classes_fall_back_to_uniform_draws(dev, path):
    """Class 0 around +v, class 1 around -v: every negative lies at D >= c_hi, for every anchor."""
    p, k, e = 2, 6, 4
    r = np.random.RandomState(5)
    x = np.zeros((p * k, e))
    x[:, 0] = np.repeat([1.0, -1.0], k)
    x[:, 1:] = np.round(r.randn(p * k, e - 1) * 4) / 64
    x = x.astype(np.float32)
    dist = R.distances(x, R.error_class(x, path, 1.0 / 64))
    assert dist["exact"] and dist["D"][:k, k:].min() >= 1.9
    got = _run(x, p, k, dev, path=path, g=UP)
    assert not got["SW"].any()
    assert _check_picks(got, p, k, SEED, ("antipodal", path)) == p * k * (k - 1)
    _check_values(got, x, dist, p, k, R.params32(**R.TEST_PARAMS), ("antipodal", path))
    assert got["counts"][1] == 0                             # beta - D + alpha < 0 at D ~ 2


@pytest.mark.parametrize("path", ["per_class", "distance_matrix"])
def test_a_nan_row_is_never_eligible_and_indices_stay_in_range(dev, path):
    p, k, e = 5, 7, 33
    n = p * k
    x = _signed(p, k, e).copy()
    bad = 9
    x[bad] = np.nan
    got = _run(x, p, k, dev, path=path)
    trip = got["trip"]
    assert trip.min() >= 0 and trip.max() < n and (trip[:, 2] // k != trip[:, 0] // k).all()
    assert not got["SW"][:, bad].any() and not got["SW"][bad].any()          # never eligible; the NaN anchor itself falls back
    assert not (trip[trip[:, 0] != bad][:, 2] == bad).any()                   # and so never drawn by an anchor with eligible columns
    rows = trip.reshape(n, k - 1, 3)
    assert [int(v) for v in rows[bad, :, 2]] == [R.fallback_pick(R.draw_u(SEED, bad, j), bad, n, k) for j in range(k - 1)]
    assert np.isfinite(got["W"]).all() and not got["W"][bad].any() and not got["W"][:, bad].any()
    assert np.isfinite(got["loss"]) and (got["counts"] >= 0).all() and got["counts"][2] == got["counts"][0] + got["counts"][1]
    clean = _run(_signed(p, k, e), p, k, dev, path=path)   # rows whose maximum was elsewhere keep their weights bit for bit
    keep = (np.arange(n) != bad) & (clean["SW"].argmax(1) != bad)
    cols = np.arange(n) != bad
    assert keep.sum() > n // 2 and np.array_equal(got["SW"][keep][:, cols], clean["SW"][keep][:, cols])


@pytest.mark.parametrize("kw", [dict(cutoff=1.4), dict(cutoff=1.5), dict(nonzero_loss_cutoff=2.0), dict(cutoff=0.0), dict(cutoff=-1.0),
                                dict(alpha=-0.1), dict(beta=float("nan")), dict(alpha=float("nan")), dict(cutoff=float("nan")),
                                dict(nonzero_loss_cutoff=float("nan"))], ids=str)
def test_out_of_range_parameters_raise_before_a_launch(dev, kw):
    from embeddingnet_amd import _lib, ops
    x = torch.tensor(_signed(5, 7, 33), device=dev)
    _lib.trace_enable(True)
    _lib.trace_reset()                                       # (records of an earlier test's traced step may still be there)
    try:
        with pytest.raises(_lib.EmbnetError, match="margin_loss_fwd"):
            ops.margin_loss(x, 5, 7, **dict(R.DEFAULTS, **kw))
        assert _lib.trace_records() == []                    # no kernel was launched
    finally:
        _lib.trace_enable(False)
    with pytest.raises(_lib.EmbnetError, match="margin_loss"):
        ops.margin_loss(x, 5, 7, path="similarity_matrix")
    with pytest.raises(_lib.EmbnetError, match="margin_loss"):
        ops.margin_loss(x, 7, 7)


def _raw(xt, p, k, path, pad, params=R.TEST_PARAMS, seed=SEED, stream=None):
    """The C ABI directly on buffers with `pad` guard elements on either side.  -> dict of guarded tensors."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    n, e = xt.shape
    dev = xt.device
    wsn = lib.embnet_margin_loss_workspace_bytes(p, k, e) // 4
    rows = n * (k - 1)
    nan = float("nan")
    b = dict(W=torch.full((2 * pad + n * n,), nan, device=dev), SW=torch.full((2 * pad + n * n,), nan, device=dev),
             demb=torch.full((2 * pad + n * e,), nan, device=dev), mean=torch.full((2 * pad + 1,), nan, device=dev),
             ws=torch.full((2 * pad + wsn,), nan, device=dev), counts=torch.full((2 * pad + 3,), -12345, dtype=torch.int32, device=dev),
             trip=torch.full((2 * pad + rows * 3,), -12345, dtype=torch.int32, device=dev))
    b["ws"][pad:pad + wsn] = 0
    up = torch.tensor(UP, device=dev)
    torch.cuda.synchronize()
    s = _lib.stream() if stream is None else stream.cuda_stream
    at = lambda name: b[name][pad:].data_ptr()
    par = [params[key] for key in ("beta", "alpha", "cutoff", "nonzero_loss_cutoff")]
    _lib.check(lib.embnet_margin_loss_fwd(xt.data_ptr(), p, k, e, *par, seed, None, path, at("W"), at("counts"), at("trip"), at("SW"),
                                          at("mean"), at("ws"), wsn * 4, s))
    _lib.check(lib.embnet_margin_loss_bwd(xt.data_ptr(), n, e, at("W"), at("counts"), up.data_ptr(), at("demb"), s))
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize("path", [1, 2])
def test_the_c_abi_gives_the_same_values_and_writes_nothing_outside_the_outputs(dev, path):
    p, k, e, pad = 5, 7, 33, 64                              # N = 35: ragged tiles in every kernel; pad * 4 bytes keeps 16-byte alignment
    n = p * k
    x = _signed(p, k, e)
    b = _raw(torch.tensor(x, device=dev), p, k, path, pad)
    for name in ("W", "SW", "demb", "mean", "ws"):
        assert torch.isnan(b[name][:pad]).all() and torch.isnan(b[name][-pad:]).all(), name
        assert torch.isfinite(b[name][pad:-pad]).all(), name  # every entry of W, sample_w and demb is written
    for name in ("counts", "trip"):
        assert (b[name][:pad] == -12345).all() and (b[name][-pad:] == -12345).all() and (b[name][pad:-pad] >= 0).all(), name
    assert b["ws"][pad].view(torch.int32).item() == 0       # the ticket is re-armed
    name = ["per_class", "distance_matrix"][path - 1]
    got = _run(x, p, k, dev, path=name, g=UP)
    raw = dict(loss=b["mean"][pad].item(), counts=b["counts"][pad:-pad].cpu().numpy(), trip=b["trip"][pad:-pad].view(-1, 3).cpu().numpy(),
               W=b["W"][pad:-pad].view(n, n).cpu().numpy(), SW=b["SW"][pad:-pad].view(n, n).cpu().numpy(),
               grad=b["demb"][pad:-pad].view(n, e).cpu().numpy())
    for key in ("trip", "counts", "W", "SW", "grad"):
        assert np.array_equal(raw[key], got[key]), key
    assert raw["loss"] == got["loss"]
    _check_values(raw, x, _dist(p, k, e, name), p, k, R.params32(**R.TEST_PARAMS), ("C ABI", name))
    # sample_w = NULL skips that output and changes nothing else
    from embeddingnet_amd import ops
    m2, c2, t2 = ops.margin_loss(torch.tensor(x, device=dev), p, k, **R.TEST_PARAMS, seed=SEED, path=name)
    assert torch.equal(t2, got["trip_t"]) and torch.equal(c2, got["counts_t"]) and torch.equal(m2, got["mean_t"])


# ---------------------------------------------------------------------------------------------------------------- 5. reproducible
@pytest.mark.parametrize("p,k,e", [(32, 4, 256), (256, 8, 128)], ids=str)
def test_bitwise_reproducible_and_keyed_by_the_seed(dev, p, k, e):
    x = R.signed(p, k, e, seed=4)
    r1, r2 = _run(x, p, k, dev, g=UP), _run(x, p, k, dev, g=UP)
    for key in ("mean_t", "counts_t", "trip_t", "W_t", "SW_t", "grad_t"):
        assert torch.equal(r1[key], r2[key]), key
    assert np.isfinite(r1["loss"]) and r1["loss"] > 0 and np.abs(r1["grad"]).max() > 0
    other = _run(x, p, k, dev, seed=SEED + 1, g=UP)
    assert torch.equal(other["SW_t"], r1["SW_t"])            # the weights do not depend on the seed
    assert (other["trip"][:, 2] != r1["trip"][:, 2]).any() and np.array_equal(other["trip"][:, :2], r1["trip"][:, :2])
    word = torch.tensor([SEED + 1], dtype=torch.int64, device=dev)                  # seed_dev overrides seed
    over = _run(x, p, k, dev, seed=SEED, seed_dev=word.data_ptr(), g=UP)
    for key in ("mean_t", "counts_t", "trip_t", "W_t", "grad_t"):
        assert torch.equal(over[key], other[key]), key
    if (p, k, e) == (256, 8, 128):                           # a second stream, its own workspace
        s2 = torch.cuda.Stream(device=dev)
        b = _raw(torch.tensor(x, device=dev), p, k, 0, 16, stream=s2)
        n = p * k
        assert torch.equal(b["W"][16:-16].view(n, n), r1["W_t"]) and torch.equal(b["trip"][16:-16].view(-1, 3), r1["trip_t"])
        assert torch.equal(b["demb"][16:-16].view(n, e), r1["grad_t"]) and torch.equal(b["mean"][16], r1["mean_t"])


def test_the_miner_alone_draws_the_same_triplets_and_feeds_the_gather_loss(dev):
    from embeddingnet_amd import ops
    p, k, e = 9, 8, 40
    x = torch.tensor(_signed(p, k, e), device=dev)
    trip, count = ops.distance_weighted_triplets(x, p, k, 0.5, 1.4, SEED)
    got = _device(p, k, e, "per_class")
    assert torch.equal(trip, got["trip_t"]) and count.dtype == torch.int32 and count.tolist() == [p * k * (k - 1)]
    assert not trip.requires_grad
    xt = x.clone().requires_grad_(True)
    mean, losses = ops.triplet_gather_loss(xt, trip, count, 0.2)
    mean.backward()
    x64 = x.double().cpu().numpy()
    t = trip.cpu().numpy()
    hinge = np.maximum(((x64[t[:, 0]] - x64[t[:, 1]]) ** 2).sum(1) - ((x64[t[:, 0]] - x64[t[:, 2]]) ** 2).sum(1) + 0.2, 0.0)
    assert abs(mean.item() - hinge.mean()) < 1e-5 and losses.shape == (t.shape[0],) and torch.isfinite(xt.grad).all()


# ---------------------------------------------------------------------------------------------------------------- 6. training
def _trainer(dev, graph, cls="triplet", seed=5, **kw):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer, XbmTrainer
    from embeddingnet_amd.xbm import CrossBatchMemory
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=seed, device=dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-3)
    if cls == "triplet":
        return base, None, TripletTrainer(base, opt, 8, 4, negatives_selection_mode="distance_weighted", seed=3, graph=graph, **kw)
    memory = CrossBatchMemory(96, 64, dev)
    return base, memory, XbmTrainer(base, opt, 8, 4, negatives_selection_mode="distance_weighted", seed=3, graph=graph, memory=memory,
                                    **kw)


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


def test_trainer_distance_weighted_learns(dev):
    """30 steps on the backbone's unit embeddings.  The threshold is the run's own start: the hinge sum (loss x active pairs) of the
    last five steps stays below that of the first five."""
    _, _, tr = _trainer(dev, graph=False)
    sums, active = [], []
    for x, _ in _batches(dev, 30):
        loss = float(tr.step(x).item())
        trip, count = tr.last_triplets
        assert trip.shape == (32 * 3, 3) and trip.dtype == torch.int32 and count.dtype == torch.int32 and count.shape == (1,)
        c = tr.last_pair_counts
        assert c.shape == (3,) and int(c[2]) == int(count) == int(c[0]) + int(c[1])
        assert int(trip.min()) >= 0 and int(trip.max()) < 32
        active.append(int(count))
        sums.append(loss * max(int(count), 1))
    print("distance_weighted trainer hinge sums", [round(v, 3) for v in sums], "active pairs", active)
    assert np.all(np.isfinite(sums))
    assert sum(sums[-5:]) < sum(sums[:5]), sums


def test_trainer_graph_replay_equals_eager_and_redraws_every_step(dev):
    from embeddingnet_amd import _lib
    runs = []
    for graph in (False, True):
        base, _, tr = _trainer(dev, graph=graph, loss_params=dict(beta=1.0, alpha=0.1))
        losses, counts, trips = [], [], []
        for i, (x, _) in enumerate(_batches(dev, 14)):
            if graph and i == 11:
                _lib.trace_enable(True)                      # an eager step between replays
            losses.append(tr.step(x).clone())
            _lib.trace_enable(False)
            assert tr.last_triplets[1].data_ptr() == tr.last_pair_counts.data_ptr() + 8
            counts.append(tr.last_pair_counts.clone())
            trips.append(tr.last_triplets[0].clone())        # (a replayed step's rows are one buffer)
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        runs.append((torch.stack(losses), torch.stack(counts), torch.stack(trips), _weights(base)))
    for a, b in zip(*runs):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()
    trips = runs[1][2]
    for i in range(1, trips.shape[0]):
        assert not torch.equal(trips[i, :, 2], trips[i - 1, :, 2]), i             # the replay draws new negatives


def test_xbm_trainer_graph_replay_equals_eager(dev):
    from embeddingnet_amd import _lib
    from embeddingnet_amd.train_step import TripletTrainer
    steps = TripletTrainer.GRAPH_WARMUP + 8
    runs = []
    for graph in (False, True):
        base, memory, tr = _trainer(dev, graph=graph, cls="xbm", start_iteration=2)
        losses, trips = [], []
        for i, (x, y) in enumerate(_batches(dev, steps)):
            if graph and i == steps - 3:
                _lib.trace_enable(True)                      # an eager step between replays
            losses.append(tr.step(x, y).clone())
            _lib.trace_enable(False)
            trips.append(tr.last_triplets[0].clone())
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        runs.append((torch.stack(losses), torch.stack(trips), _weights(base), memory.feats.clone(), memory.labels.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()


# ---------------------------------------------------------------------------------------------------------------- 7. CLI
def _cli(tmp_path, edit=lambda cfg: cfg, classes=10):
    cfg = open(os.path.join(ROOT, "configs", "simple2_margin_synthetic.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert "negatives_selection_mode : 'distance_weighted'" in cfg and "n_batches : 20" in cfg and "margin_loss :" in cfg
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(edit(cfg.replace("n_batches : 20", "n_batches : 4")))
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path), "--synthetic", str(classes),
                           "--max_epochs", "2"], capture_output=True, text=True, timeout=600)


def test_train_cli_margin_config(tmp_path):
    out = _cli(tmp_path)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Epoch 2/2" in out.stdout and "saving model" in out.stdout and "active_pairs" in out.stdout
    assert any(f.startswith("epoch_") for f in os.listdir(tmp_path / "simple2_margin_synthetic" / "weights"))


def test_train_cli_refuses_margin_loss_with_another_mode(tmp_path):
    out = _cli(tmp_path, lambda cfg: cfg.replace("'distance_weighted'", "'semihard'"))
    assert out.returncode != 0
    assert "GENERATOR.margin_loss" in out.stderr and "distance_weighted" in out.stderr and "Epoch 1" not in out.stdout
