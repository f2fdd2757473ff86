"""Distance-weighted sampling and the margin loss, host side (no GPU): the C ABI is declared and exported and refuses arguments outside
its range before any launch; the float64 restatement in tests/margin_ref.py agrees with torch autograd (picks held fixed) and with
cases worked by hand; the Python layers and tools/train.py know the mode; and the inputs of tests/test_margin_loss_gpu.py are fit
for what that test asserts on them."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import margin_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_margin_loss_path", "embnet_margin_loss_workspace_bytes", "embnet_margin_loss_fwd", "embnet_margin_loss_bwd")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced
KEYS = ("beta", "alpha", "cutoff", "nonzero_loss_cutoff")


# ---------------------------------------------------------------------------------------------------------------- 1. the ABI
def _lib():
    from embeddingnet_amd import _lib
    return _lib.lib()


def test_header_declares_and_library_exports_margin_loss():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported and exported == set(protos)
    assert _lib.lib().embnet_abi_version() == 22


def _fwd(p, k, e, beta=1.2, alpha=0.2, c_lo=0.5, c_hi=1.4, ws_bytes=1 << 31, path=0):
    l = _lib()
    rc = l.embnet_margin_loss_fwd(FAKE, p, k, e, beta, alpha, c_lo, c_hi, 7, None, path, FAKE, FAKE, FAKE, None, FAKE, FAKE, ws_bytes, None)
    return rc, l.embnet_last_error().decode()


@pytest.mark.parametrize("p,k,e,what", [(1, 4, 64, "p >= 2"), (4, 1, 64, "k >= 2"), (2, 2049, 16, "n = p*k = 4098"),
                                        (8, 4, 0, "e=0"), (8, 4, 4097, "e=4097")])
def test_fwd_refuses_out_of_range_shapes(p, k, e, what):
    rc, msg = _fwd(p, k, e)
    assert rc == -1 and what in msg and msg.startswith("margin_loss_fwd"), msg
    assert _lib().embnet_margin_loss_path(p, k, e) == 0 and _lib().embnet_margin_loss_workspace_bytes(p, k, e) == 0


@pytest.mark.parametrize("kw,what", [(dict(c_lo=1.4, c_hi=1.4), "cutoff"), (dict(c_lo=1.5, c_hi=1.4), "cutoff"), (dict(c_hi=2.0), "cutoff"),
                                     (dict(c_hi=2.5), "cutoff"), (dict(c_lo=0.0), "cutoff"), (dict(c_lo=-0.5), "cutoff"),
                                     (dict(alpha=-0.1), "alpha="), (dict(beta=math.nan), "beta="), (dict(alpha=math.nan), "alpha="),
                                     (dict(c_lo=math.nan), "cutoff"), (dict(c_hi=math.nan), "cutoff"), (dict(beta=math.inf), "beta="),
                                     (dict(alpha=math.inf), "alpha=")])
def test_fwd_refuses_parameters_outside_their_range(kw, what):
    rc, msg = _fwd(8, 4, 64, **kw)
    assert rc == -1 and what in msg and msg.startswith("margin_loss_fwd"), msg


def test_null_pointers_are_refused_and_sample_w_may_be_null():
    l = _lib()
    rc = l.embnet_margin_loss_fwd(FAKE, 8, 4, 64, 1.2, 0.2, 0.5, 1.4, 7, None, 0, FAKE, FAKE, None, None, FAKE, FAKE, 1 << 31, None)
    assert rc == -1 and "margin_loss_fwd: null pointer" in l.embnet_last_error().decode()
    rc = l.embnet_margin_loss_bwd(FAKE, 32, 64, FAKE, None, None, FAKE, None)
    assert rc == -1 and "margin_loss_bwd: null pointer" in l.embnet_last_error().decode()
    rc = l.embnet_margin_loss_bwd(FAKE, 3, 64, FAKE, FAKE, None, FAKE, None)
    assert rc == -1 and "margin_loss_bwd: n=3" in l.embnet_last_error().decode()
    rc, msg = _fwd(8, 4, 64, ws_bytes=16)                    # sample_w NULL passes the pointer check: the next refusal is the workspace's
    assert rc == -3 and "workspace" in msg


def test_path_and_workspace_rules_equal_batch_alls():
    l = _lib()
    need = l.embnet_margin_loss_workspace_bytes(8, 4, 256)
    rc, msg = _fwd(8, 4, 256, ws_bytes=need - 16)
    assert rc == -3 and "workspace" in msg
    rc, msg = _fwd(8, 4, 256, path=3)
    assert rc == -1 and "unknown path" in msg
    rc, msg = _fwd(4, 32, 16, path=1)                       # k > 16: only the distance-matrix path
    assert rc == -1 and "per-class path" in msg
    for p, k, e in R.SHAPES + R.WEIGHT_SHAPES + [(256, 8, 128), (4, 4, 4081), (64, 4, 512)]:
        want = {"per_class": 1, "distance_matrix": 2}[R.auto_path(p, k, e)]
        assert l.embnet_margin_loss_path(p, k, e) == want == l.embnet_batch_all_path(p, k, e), (p, k, e)
        assert l.embnet_margin_loss_workspace_bytes(p, k, e) == l.embnet_batch_all_workspace_bytes(p, k, e)
    assert [R.auto_path(*s) for s in R.SHAPES[5:7]] == ["distance_matrix"] * 2


# ---------------------------------------------------------------------------------------------------------------- 2. the layers
def _cfg(mode, model_mode="triplet", **gen):
    return dict(generator=dict(negatives_selection_mode=mode, k_classes=8, k_samples=4, **gen), model=dict(mode=model_mode))


def _train():
    import importlib.util
    spec = importlib.util.spec_from_file_location("embnet_tools_train", os.path.join(ROOT, "tools", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    return train


def test_table_rows_and_python_layers_know_the_mode():
    import inspect
    from embeddingnet_amd import losses_and_accuracies, ops
    from embeddingnet_amd.datagenerators import TripletsDataGenerator
    from embeddingnet_amd.train_step import TripletTrainer, XbmTrainer
    assert ops.PAIR_LOSS_MODES["distance_weighted"] == (ops.margin_loss, KEYS, 2)
    assert ops.MARGIN_PATHS == dict(auto=0, per_class=1, distance_matrix=2)
    sig = inspect.signature(ops.margin_loss)
    assert list(sig.parameters) == ["emb", "k_classes", "k_samples", *KEYS, "seed", "seed_dev", "path", "return_weights"]
    assert {n: sig.parameters[n].default for n in KEYS} == R.DEFAULTS
    assert list(inspect.signature(ops.distance_weighted_triplets).parameters) == ["emb", "k_classes", "k_samples", "cutoff",
                                                                                  "nonzero_loss_cutoff", "seed"]
    assert callable(losses_and_accuracies.margin_loss(8, 4, beta=1.0, alpha=0.1))
    assert "distance_weighted" in TripletsDataGenerator.STEP_ONLY_MODES and TripletTrainer.LOSS_PARAMS["distance_weighted"] == KEYS
    assert XbmTrainer.LOSS_PARAMS["distance_weighted"] == KEYS
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    tr = TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="distance_weighted", loss_params=dict(beta=1.0, alpha=0.1))
    assert tr.loss_params == dict(beta=1.0, alpha=0.1)
    assert TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="distance_weighted").loss_params == {}
    with pytest.raises(ValueError, match="unknown keys"):
        TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="distance_weighted", loss_params=dict(margin=0.1))
    with pytest.raises(ValueError, match="unknown keys"):
        TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="circle", loss_params=dict(beta=1.0))


def test_train_config_validator_accepts_and_refuses_the_key():
    train = _train()
    assert train.MARGIN_LOSS_KEYS == KEYS and "margin_loss" not in train.LOSS_CONFIGS
    cfg = train.margin_loss_config
    assert cfg(_cfg("distance_weighted")) is None
    assert cfg(_cfg("distance_weighted", margin_loss=dict(beta=1, alpha=0.1, cutoff=0.4, nonzero_loss_cutoff=1.5))) == \
        dict(beta=1.0, alpha=0.1, cutoff=0.4, nonzero_loss_cutoff=1.5)
    assert cfg(_cfg("distance_weighted", margin_loss=dict(alpha=0))) == dict(alpha=0.0)
    assert cfg(_cfg("distance_weighted", margin_loss=dict(beta=-1))) == dict(beta=-1.0)
    for mode in ("semihard", "multi_similarity", "circle", "batch_all"):
        with pytest.raises(ValueError, match="GENERATOR.margin_loss sets the parameters of negatives_selection_mode 'distance_weighted'"):
            cfg(_cfg(mode, margin_loss=dict(beta=1.0)))
    with pytest.raises(ValueError, match="Siamese"):
        cfg(_cfg("distance_weighted", model_mode="siamese", margin_loss=dict(beta=1.0)))
    for other, fn in (("ms_loss", train.ms_loss_config), ("circle_loss", train.circle_loss_config)):
        with pytest.raises(ValueError, match="GENERATOR." + other):                 # the other keys stay refused with this mode
            fn(_cfg("distance_weighted", **{other: dict()}))
    for bad, text in ((dict(cutoff=1.4), "0 < cutoff < nonzero_loss_cutoff < 2"), (dict(nonzero_loss_cutoff=0.5), "0 < cutoff < nonzero"),
                      (dict(cutoff=1.5, nonzero_loss_cutoff=1.4), "0 < cutoff < nonzero"), (dict(nonzero_loss_cutoff=2), "< 2"),
                      (dict(nonzero_loss_cutoff=2.5), "< 2"), (dict(cutoff=0), "cutoff must be positive"),
                      (dict(cutoff=-0.5), "cutoff must be positive"), (dict(alpha=-0.1), "alpha must not be negative"),
                      (dict(margin=0.5), "a mapping with keys out of"), (dict(beta="wide"), "every value must be a number"),
                      (dict(beta=True), "every value must be a number"), ([1.2], "a mapping with keys out of")):
        with pytest.raises(ValueError, match="GENERATOR.margin_loss.*" + text):
            cfg(_cfg("distance_weighted", margin_loss=bad))
    assert "distance_weighted" in train.XBM_MODES
    assert train.xbm_config(_cfg("distance_weighted", xbm=dict(size=64)))["loss"] == "contrastive"


def test_the_example_config_passes_the_validator():
    import yaml
    with open(os.path.join(ROOT, "configs", "simple2_margin_synthetic.yml")) as f:
        raw = yaml.safe_load(f)
    assert raw["MODEL"]["embeddings_normalization"] is True and raw["GENERATOR"]["negatives_selection_mode"] == "distance_weighted"
    cfg = dict(generator=raw["GENERATOR"], model=raw["MODEL"])
    assert _train().margin_loss_config(cfg) == R.DEFAULTS


# ---------------------------------------------------------------------------------------------------------------- 3. the reference
def test_draws_are_the_53_bit_form_of_the_kmeans_pick():
    import kmeans_ref
    assert R.draw_u(5, 3, 0) == float(((kmeans_ref.rng_u32(5, 3, 0) << 32 | kmeans_ref.rng_u32(5, 3, 1)) >> 11)) * 2.0 ** -53
    us = np.array([R.draw_u(11, i, j) for i in range(40) for j in range(25)])
    assert 0.0 <= us.min() and us.max() < 1.0 and len(set(us.tolist())) == us.size and abs(us.mean() - 0.5) < 0.05
    assert R.positives(5, 4) == [4, 6, 7] and R.positives(0, 3) == [1, 2]
    assert [R.fallback_pick(u, 5, 12, 4) for u in (0.0, 0.49, 0.5, 0.999)] == [0, 3, 8, 11]


def test_log_weight_is_the_inverse_sphere_density_and_flat_where_the_paper_says():
    """q(d) ~ d^{e-2} (1 - d^2/4)^{(e-3)/2}: at e = 2 the first exponent vanishes, at e = 3 the second; lw is -log q."""
    d = np.array([[0.3, 0.7, 1.0, 1.3]])
    dist = dict(D=d, dD=np.zeros_like(d))
    par = R.params32(cutoff=0.1, nonzero_loss_cutoff=1.9)
    for e in (2, 3, 16):
        lw, elw = R.log_weights(dist, e, par)
        want = -((e - 2) * np.log(d) + 0.5 * (e - 3) * np.log(1 - d * d / 4))
        assert np.abs(lw - want).max() < 1e-12 and (elw < 1e-4).all()
    par = R.params32()
    lw, _ = R.log_weights(dict(D=np.array([[0.2, 0.5]]), dD=np.zeros((1, 2))), 8, par)
    assert lw[0, 0] == lw[0, 1]                               # below the cutoff the weight is the cutoff's


def test_p2_k2_by_hand():
    """Rows (1,0), (c,s) | (0,1), (-s,c) at 30 degrees.  Anchor 0: positive at D = 2 sin 15, negatives at sqrt(2) and 2 sin 60:
    with c_hi = 1.5 only row 2 is eligible, so every draw of anchor 0 takes it whatever u is."""
    c, s_ = math.cos(math.pi / 6), math.sin(math.pi / 6)
    x = np.array([[1, 0], [c, s_], [0, 1], [-s_, c]], np.float32)
    par = R.params32(1.0, 0.1, 0.5, 1.5)
    dist = R.distances(x, "exact")
    w, elig = R.weights64(dist, 2, 2, 2, par)
    assert elig[0].tolist() == [False, False, True, False] and w[0].tolist() == [0, 0, 1, 0]
    trip = R.sample64(x, 2, 2, par, seed=3)
    assert trip.shape == (4, 3) and trip[0].tolist() == [0, 1, 2] and trip[:, 1].tolist() == [1, 0, 3, 2]
    ref = R.reference(dist, 2, 2, par, trip)
    dp, dn = 2 * math.sin(math.pi / 12), math.sqrt(2.0)
    assert abs(dist["D"][0, 1] - dp) < 1e-7 and abs(dist["D"][0, 2] - dn) < 1e-7
    assert ref["lp"][0, 1] == 0 and ref["W"][0, 1] == 0         # D+ = 0.52 < beta - alpha: the positive is inactive
    assert ref["ln"][0, 2] == 0 and ref["W"][0, 2] == 0         # D- = 1.41 > beta + alpha: so is the drawn negative
    par = R.params32(0.4, 0.2, 0.5, 1.5)                       # beta inside: the positive pays 0.52 - 0.4 + 0.2
    ref = R.reference(dist, 2, 2, par, trip)
    assert abs(ref["lp"][0, 1] - (dist["D"][0, 1] - par["beta"] + par["alpha"])) < 1e-15 and abs(ref["W"][0, 1] - 1 / dist["D"][0, 1]) < 1e-15
    assert ref["cp"] == 4 and ref["A"] == ref["cp"] + ref["cn"]


def test_fallback_when_nothing_is_eligible_and_duplicates_weigh_nothing():
    x = np.array([[1], [1], [-1], [-1], [1], [-1]], np.float32)          # classes (1,1) (-1,-1) (1,-1): D is 0 or 2
    par = R.params32(**R.TEST_PARAMS)
    dist = R.distances(x, "exact")
    w, _ = R.weights64(dist, 3, 2, 1, par)
    assert not w[2].any() or w[2, 5] == 1                       # row 2 = -1: its only eligible negatives are the -1 of class 2
    assert not w[0, 2:4].any() and w[0, 4] == 1 and w[0, 5] == 0
    x2 = np.array([[1], [1], [-1], [-1]], np.float32)
    d2 = R.distances(x2, "exact")
    w2, _ = R.weights64(d2, 2, 2, 1, par)
    assert not w2.any()                                         # every negative at D = 2: all four anchors fall back
    trip = R.sample64(x2, 2, 2, par, seed=9)
    for i, pc, n in trip.tolist():
        assert n == R.fallback_pick(R.draw_u(9, i, 0), i, 4, 2) and (n // 2) != (i // 2)
    ref = R.reference(dist, 3, 2, par, np.array([[0, 1, 4], [1, 0, 4], [2, 3, 5], [3, 2, 5], [4, 5, 0], [5, 4, 2]]))
    assert ref["ln"][0, 4] > 0 and ref["W"][0, 4] == 0 and ref["cn"] == 6     # D = 0: counted, no direction
    want, bound = R.demb(x, ref["W"], ref["A"])
    assert np.isfinite(want).all() and np.isfinite(bound).all()


def _torch_loss(x, p, k, par, trip, a):
    pos, _ = R.class_masks(p, k)
    d = torch.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1) + torch.eye(p * k, dtype=torch.float64))     # (the diagonal is unused)
    lp = torch.clamp(d - par["beta"] + par["alpha"], min=0)[torch.tensor(pos)].sum()
    t = torch.tensor(np.asarray(trip, np.int64))
    ln = torch.clamp(par["beta"] - d[t[:, 0], t[:, 2]] + par["alpha"], min=0).sum()
    return (lp + ln) / max(a, 1)


@pytest.mark.parametrize("p,k,e", [(5, 7, 33), (9, 8, 40), (4, 32, 16), (32, 4, 256)], ids=str)
@pytest.mark.parametrize("params", [R.TEST_PARAMS, R.DEFAULTS, dict(R.TEST_PARAMS, alpha=0.0)], ids=["test", "defaults", "alpha0"])
def test_reference_gradient_agrees_with_autograd_picks_held_fixed(p, k, e, params):
    x = R.signed(p, k, e)
    par = R.params32(**params)
    trip = R.sample64(x, p, k, par, seed=17)
    dist = R.distances(x, "exact")
    ref = R.reference(dist, p, k, par, trip)
    assert trip.shape == (p * k * (k - 1), 3) and (ref["A"] > 0 or (params["alpha"] == 0 and e == 256))
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    loss = _torch_loss(xt, p, k, par, trip, ref["A"])
    (0.75 * loss).backward()
    want, _ = R.demb(x, ref["W"], ref["A"], 0.75)
    assert abs(loss.item() - ref["loss_sum"] / max(ref["A"], 1)) < 1e-12
    assert np.abs(want - xt.grad.numpy()).max() < 1e-12
    assert np.isfinite(R.loss_and_bound(ref, ref["A"])[1])


def test_sampler_restatement_spreads_draws_and_never_takes_a_zero_weight():
    p, k, e = 9, 8, 40
    x, par = R.signed(p, k, e), R.params32(**R.TEST_PARAMS)
    w, elig = R.weights64(R.distances(x, "exact"), p, k, e, par)
    trips = np.concatenate([R.sample64(x, p, k, par, seed=s) for s in range(4)])
    assert (w[trips[:, 0], trips[:, 2]] > 0).all() and w.max(1).tolist() == [1.0] * (p * k)
    assert len({tuple(t) for t in trips.tolist()}) > trips.shape[0] // 3
    assert R.pick_acceptable(w[3], R.draw_u(0, 3, 2), int(R.sample64(x, p, k, par, seed=0)[3 * (k - 1) + 2, 2]))


# ---------------------------------------------------------------------------------------------------------------- 4. fitness
@pytest.mark.parametrize("p,k,e", R.SHAPES, ids=str)
def test_gpu_inputs_are_fit(p, k, e):
    """Grid inputs: d2 exact in any order and form.  Signed inputs: unit rows, and on every path the GPU test runs at most OPEN_CAP of
    the decisions (eligibility, clamp, hinge signs) are open, for both parameter sets the GPU test runs."""
    xg, unit = R.grid(p, k, e)
    assert R.d2_is_exact(xg, unit) and R.error_class(xg, "per_class", unit) == "exact"
    x = R.signed(p, k, e)
    assert np.allclose(np.linalg.norm(x.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (R.error_class(x, "distance_matrix") == "exact") == (e == 1)
    for path in R.paths(p, k, e):
        dist = R.distances(x, R.error_class(x, path))
        for params in (R.TEST_PARAMS, R.DEFAULTS, dict(R.TEST_PARAMS, alpha=0.0)):
            dec = R.decisions(dist, p, k, R.params32(**params))
            assert dec["share"] <= R.OPEN_CAP, (path, params, dec["share"])


@pytest.mark.parametrize("p,k,e", R.WEIGHT_SHAPES, ids=str)
def test_weight_inputs_are_fit(p, k, e):
    x = R.weight_input(p, k, e)
    for path in R.paths(p, k, e):
        assert R.decisions(R.distances(x, path), p, k, R.params32(**R.TEST_PARAMS))["share"] <= R.OPEN_CAP
    if e == 512:                                                # some weight underflows in fp32: lw - M < log 2^-149
        dist = R.distances(x, "exact")
        w, elig = R.weights64(dist, p, k, e, R.params32(**R.TEST_PARAMS))
        assert (elig & (w < 2.0 ** -149)).any()


def test_every_case_the_gpu_test_names_occurs_in_some_shape():
    seen = dict(fallback=False, ineligible=False, pos_on=False, pos_off=False, neg_on=False, neg_off=False, clamped=False)
    par = R.params32(**R.TEST_PARAMS)
    for p, k, e in R.SHAPES:
        x = R.signed(p, k, e)
        dist = R.distances(x, "exact")
        w, elig = R.weights64(dist, p, k, e, par)
        pos, neg = R.class_masks(p, k)
        seen["fallback"] |= bool((~elig.any(1)).any())
        seen["ineligible"] |= bool((neg & ~elig).any() and elig.any())
        seen["clamped"] |= bool((elig & (dist["D"] < par["c_lo"])).any())
        ref = R.reference(dist, p, k, par, R.sample64(x, p, k, par, seed=1))
        seen["pos_on"] |= bool((ref["lp"][pos] > 0).any())
        seen["pos_off"] |= bool((ref["lp"][pos] == 0).any())
        drawn = ref["draws"] > 0
        seen["neg_on"] |= bool((ref["ln"][drawn] > 0).any())
        seen["neg_off"] |= bool((ref["ln"][drawn] == 0).any())
    assert all(seen.values()), seen
    # with the defaults every eligible negative is active by construction (c_hi = beta + alpha): the tests must not use them alone
    d = R.params32(**R.DEFAULTS)
    assert abs(d["beta"] + d["alpha"] - d["c_hi"]) < 1e-6
