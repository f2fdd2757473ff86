"""Circle loss, host side (no GPU): the C ABI is declared and exported and refuses arguments outside its range before any launch;
the float64 restatement in tests/circle_ref.py agrees with torch autograd (alpha detached) in the batch and against a bank and with
cases worked by hand; an fp32 emulation of the header's rounding form stays within the a-priori bounds; the Python layers and
tools/train.py know the mode; and the inputs of tests/test_circle_loss_gpu.py are fit for what that test asserts on them."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import circle_ref as C
import ms_ref as M
import xbm_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_circle_loss_path", "embnet_circle_loss_workspace_bytes", "embnet_circle_loss_fwd", "embnet_xbm_circle_loss_fwd")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced


# ---------------------------------------------------------------------------------------------------------------- 1. the ABI
def _lib():
    from embeddingnet_amd import _lib
    return _lib.lib()


def test_header_declares_and_library_exports_circle_loss():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported and exported == set(protos)
    assert _lib.lib().embnet_abi_version() == 22


def _fwd(p, k, e, m=0.4, gamma=80.0, ws_bytes=1 << 31, path=0):
    l = _lib()
    rc = l.embnet_circle_loss_fwd(FAKE, p, k, e, m, gamma, path, FAKE, FAKE, FAKE, FAKE, ws_bytes, None)
    return rc, l.embnet_last_error().decode()


def _xbm_fwd(n, slots, e, m=0.4, gamma=80.0, ws_bytes=1 << 31):
    l = _lib()
    rc = l.embnet_xbm_circle_loss_fwd(FAKE, FAKE, FAKE, FAKE, None, n, slots, e, m, gamma, FAKE, FAKE, FAKE, FAKE, ws_bytes, None)
    return rc, l.embnet_last_error().decode()


@pytest.mark.parametrize("p,k,e,what", [(1, 4, 64, "p >= 2"), (4, 1, 64, "k >= 2"), (2, 2049, 16, "n = p*k = 4098"),
                                        (8, 4, 0, "e=0"), (8, 4, 4097, "e=4097")])
def test_fwd_refuses_out_of_range_shapes(p, k, e, what):
    rc, msg = _fwd(p, k, e)
    assert rc == -1 and what in msg and msg.startswith("circle_loss_fwd"), msg
    assert _lib().embnet_circle_loss_path(p, k, e) == 0 and _lib().embnet_circle_loss_workspace_bytes(p, k, e) == 0


@pytest.mark.parametrize("m,gamma,what", [(-0.1, 80.0, "m="), (1.5, 80.0, "m="), (math.nan, 80.0, "m="), (math.inf, 80.0, "m="),
                                          (0.4, 0.0, "gamma="), (0.4, -1.0, "gamma="), (0.4, math.nan, "gamma="),
                                          (0.4, math.inf, "gamma=")])
def test_both_entry_points_refuse_parameters_outside_their_range(m, gamma, what):
    for rc, msg in (_fwd(8, 4, 64, m=m, gamma=gamma), _xbm_fwd(8, 16, 4, m=m, gamma=gamma)):
        assert rc == -1 and what in msg and "circle_loss_fwd" in msg, msg


def test_fwd_refuses_bad_workspace_and_path_and_follows_the_multi_similarity_fit_rule():
    l = _lib()
    need = l.embnet_circle_loss_workspace_bytes(8, 4, 256)
    rc, msg = _fwd(8, 4, 256, ws_bytes=need - 16)
    assert rc == -3 and "workspace" in msg
    rc, msg = _fwd(8, 4, 256, path=3)
    assert rc == -1 and "unknown path" in msg
    rc, msg = _fwd(4, 32, 16, path=1)                       # k > 16: only the similarity-matrix path
    assert rc == -1 and "per-class path" in msg
    for p, k, e in C.BATCH_SHAPES + [(32, 4, 256), (256, 8, 128), (4, 4, 4081), (2, 2048, 4096)]:
        want = {"per_class": 1, "similarity_matrix": 2}[C.auto_path(p, k, e)]
        assert l.embnet_circle_loss_path(p, k, e) == want == l.embnet_ms_loss_path(p, k, e), (p, k, e)
        assert l.embnet_circle_loss_workspace_bytes(p, k, e) == l.embnet_ms_loss_workspace_bytes(p, k, e)
    assert [C.auto_path(*s) for s in C.BATCH_SHAPES[-2:]] == ["similarity_matrix"] * 2


@pytest.mark.parametrize("n,slots,e,what", [(1, 8, 4, "n=1"), (4097, 8192, 4, "n=4097"), (8, 7, 4, "m=7"), (8, 65537, 4, "m=65537"),
                                            (4096, 32768, 4, "2^26"), (8, 16, 0, "e=0"), (8, 16, 4097, "e=4097")])
def test_xbm_fwd_refuses_out_of_range_shapes(n, slots, e, what):
    rc, msg = _xbm_fwd(n, slots, e)
    assert rc == -1 and what in msg and msg.startswith("xbm_circle_loss_fwd"), msg


def test_xbm_fwd_refuses_a_short_workspace_and_the_kinds_stay_two():
    need = _lib().embnet_xbm_loss_workspace_bytes(8, 16, 4)
    rc, msg = _xbm_fwd(8, 16, 4, ws_bytes=need - 16)
    assert rc == -3 and "workspace" in msg
    rc = _lib().embnet_xbm_loss_fwd(FAKE, FAKE, FAKE, FAKE, None, 8, 16, 4, 3, 0.4, 80.0, 0.0, 0.0, FAKE, FAKE, FAKE, FAKE, 1 << 31, None)
    assert rc == -1 and "unknown kind 3" in _lib().embnet_last_error().decode()


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
    from embeddingnet_amd import losses_and_accuracies, ops
    from embeddingnet_amd.datagenerators import TripletsDataGenerator
    from embeddingnet_amd.train_step import TripletTrainer
    assert ops.PAIR_LOSS_MODES["circle"] == (ops.circle_loss, ("m", "gamma"), 1)
    assert ops.XBM_LOSS_MODES["circle"] == (ops.xbm_circle_loss, ("m", "gamma"))
    assert ops.CIRCLE_PATHS == dict(auto=0, per_class=1, similarity_matrix=2)
    assert callable(losses_and_accuracies.circle_loss(8, 4, 0.25, 256.0))
    assert callable(losses_and_accuracies.xbm_loss(object(), "circle", m=0.25, gamma=64.0))
    with pytest.raises(ValueError, match="unknown parameters"):
        losses_and_accuracies.xbm_loss(object(), "circle", margin=0.5)
    assert "circle" in TripletsDataGenerator.STEP_ONLY_MODES and TripletTrainer.LOSS_PARAMS["circle"] == ("m", "gamma")
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    tr = TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="circle", loss_params=dict(m=0.25, gamma=256.0))
    assert tr.loss_params == dict(m=0.25, gamma=256.0)
    assert TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="circle").loss_params == {}
    with pytest.raises(ValueError, match="unknown keys"):
        TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="circle", loss_params=dict(temperature=0.1))
    with pytest.raises(ValueError, match="unknown keys"):
        TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="supcon", loss_params=dict(gamma=80.0))


def test_train_config_validator_accepts_and_refuses_the_key():
    train = _train()
    assert train.CIRCLE_LOSS_KEYS == ("m", "gamma")
    assert train.circle_loss_config(_cfg("circle")) is None
    assert train.circle_loss_config(_cfg("circle", circle_loss=dict(m=0.25, gamma=256))) == dict(m=0.25, gamma=256.0)
    assert train.circle_loss_config(_cfg("circle", circle_loss=dict(gamma=64))) == dict(gamma=64.0)
    assert train.circle_loss_config(_cfg("circle", circle_loss=dict(m=0))) == dict(m=0.0)
    for mode in ("semihard", "multi_similarity", "supcon", "batch_all"):
        with pytest.raises(ValueError, match="GENERATOR.circle_loss sets the parameters of negatives_selection_mode 'circle'"):
            train.circle_loss_config(_cfg(mode, circle_loss=dict(m=0.4)))
    with pytest.raises(ValueError, match="Siamese"):
        train.circle_loss_config(_cfg("circle", model_mode="siamese", circle_loss=dict(m=0.4)))
    for other, fn in (("ms_loss", train.ms_loss_config), ("supcon_loss", train.supcon_loss_config)):
        with pytest.raises(ValueError, match="GENERATOR." + other):                 # the other keys stay refused with circle
            fn(_cfg("circle", **{other: dict()}))
    for bad in (dict(margin=0.5), dict(m="wide"), dict(m=True), dict(m=-0.1), dict(m=1.5), dict(gamma=0.0), dict(gamma=-2), [0.4]):
        with pytest.raises(ValueError, match="GENERATOR.circle_loss"):
            train.circle_loss_config(_cfg("circle", circle_loss=bad))
    assert "circle" in train.XBM_MODES
    got = train.xbm_config(_cfg("circle", xbm=dict(size=64, loss="circle", m=0.25, gamma=128)))
    assert got["loss"] == "circle" and got["params"] == dict(m=0.25, gamma=128.0)
    assert train.xbm_config(_cfg("semihard", xbm=dict(size=64, loss="circle")))["params"] == {}
    for bad in (dict(size=64, loss="circle", margin=0.5), dict(size=64, loss="circle", m=2.0), dict(size=64, loss="circle", gamma=0),
                dict(size=64, loss="contrastive", gamma=80.0)):
        with pytest.raises(ValueError, match="GENERATOR.xbm"):
            train.xbm_config(_cfg("circle", xbm=bad))


# ---------------------------------------------------------------------------------------------------------------- 3. the reference
def _torch_circle(s, pos, neg, par):
    """The header's plain formulas on a torch float64 S with alpha detached.  -> (sum_i l_i, active)."""
    pos, neg = torch.tensor(pos), torch.tensor(neg)
    active = pos.any(1) & neg.any(1)
    ninf = torch.tensor(-math.inf, dtype=torch.float64)
    ap = torch.clamp(par["op"] - s, min=0).detach()
    an = torch.clamp(s - par["on"], min=0).detach()
    lp = torch.logsumexp(torch.where(pos, -par["gamma"] * ap * (s - par["dp"]), ninf)[active], 1)
    ln = torch.logsumexp(torch.where(neg, par["gamma"] * an * (s - par["dn"]), ninf)[active], 1)
    z = lp + ln                                             # (torch's softplus is linear above 20: logaddexp is the function itself)
    return torch.logaddexp(z, torch.zeros_like(z)).sum(), active


@pytest.mark.parametrize("m,gamma", C.PARAMS)
@pytest.mark.parametrize("p,k,e,scale", [(8, 4, 64, 1.0), (5, 7, 33, 1.0), (2, 2, 1, 1.0), (6, 4, 16, 3.0)])
def test_reference_equals_autograd_with_alpha_detached(p, k, e, scale, m, gamma):
    x = (C.continuous(p, k, e) * np.float32(scale)).astype(np.float32)
    ref = C.reference(x, p, k, m, gamma)
    s = torch.tensor(ref["S"], requires_grad=True)
    total, active = _torch_circle(s, *M.class_masks(p, k), ref["par"])
    total.backward()
    assert active.all() and ref["active"].all()
    assert abs(float(total) / (p * k) - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
    assert np.abs(s.grad.numpy() - ref["G"]).max() <= 1e-11 * max(1.0, np.abs(ref["G"]).max())
    assert not np.diag(ref["G"]).any()


@pytest.mark.parametrize("m,gamma", C.PARAMS[:2])
@pytest.mark.parametrize("name", C.RING_CASES)
def test_ring_reference_equals_autograd_with_alpha_detached(name, m, gamma):
    c = C.ring_case(name)
    ref = C.xbm_reference(c["x"], c["labels"], c["mem"], c["mem_labels"], c["self_slots"], m, gamma)
    s = torch.tensor(ref["S"], requires_grad=True)
    total, active = _torch_circle(s, *X.sets(c["labels"], c["mem_labels"], c["self_slots"]), ref["par"])
    total.backward()
    assert np.array_equal(active.numpy(), ref["active"])
    assert abs(float(total) / len(c["x"]) - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
    assert np.abs(s.grad.numpy() - ref["G"]).max() <= 1e-11 * max(1.0, np.abs(ref["G"]).max())
    assert not ref["G"][~ref["active"]].any() and not ref["ell"][~ref["active"]].any()
    assert ref["counts"][2] == ref["active"].sum() and ref["counts"][3] == (c["mem_labels"] >= 0).sum()


def test_ring_cases_hold_what_the_gpu_test_needs_of_them():
    """Negative labels on both sides, a wrapping batch, an anchor with no positive, one with no negative, self slots out of range,
    more than one lane trip with a tail; no case larger than the two envelopes."""
    seen = dict(no_pos=False, no_neg=False)
    for name in C.RING_CASES:
        c = C.ring_case(name)
        n, slots, e = C.RING_SHAPES[name]
        assert (n <= 5 and slots <= 70 and e <= 33) or (n <= 12 and slots <= 129 and e <= 5), name
        pos, neg = X.sets(c["labels"], c["mem_labels"], c["self_slots"])
        lab = c["labels"] >= 0
        seen["no_pos"] |= bool((lab & ~pos.any(1) & neg.any(1)).any())
        seen["no_neg"] |= bool((lab & pos.any(1) & ~neg.any(1)).any())
    assert all(seen.values()), seen
    for name in ("ragged", "wide", "long"):
        c = C.ring_case(name)
        assert (c["labels"] < 0).any() and (c["mem_labels"] < 0).any()
    assert (C.ring_case("long")["self_slots"] < 0).any() and C.RING_SHAPES["wide"][1] % 64 == 6 and C.RING_SHAPES["long"][1] % 64 == 1


# ---------------------------------------------------------------------------------------------------------------- 4. by hand
def test_p2_k2_in_closed_form():
    """Rows (1,0), (c,s) | (0,1), (-s,c) at angle 30 degrees: every anchor has ONE positive at S = c and two negatives at 0 and
    -+s, so each lse has one or two terms and the loss is a few logarithms."""
    c, s_ = math.cos(math.pi / 6), math.sin(math.pi / 6)
    x = np.array([[1, 0], [c, s_], [0, 1], [-s_, c]], np.float32)
    m, g = 0.25, 8.0
    ref = C.reference(x, 2, 2, m, g)
    xs = x.astype(np.float64)
    par = ref["par"]

    def logit_p(v):
        return -g * max(par["op"] - v, 0.0) * (v - par["dp"])

    def logit_n(v):
        return g * max(v - par["on"], 0.0) * (v - par["dn"])

    for i, (pi, ns) in enumerate([(1, (2, 3)), (0, (2, 3)), (3, (0, 1)), (2, (0, 1))]):
        sp = float(xs[i] @ xs[pi])
        z = logit_p(sp) + math.log(sum(math.exp(logit_n(float(xs[i] @ xs[j]))) for j in ns))
        assert abs(ref["ell"][i] - math.log1p(math.exp(z))) < 1e-13
        sig = 1.0 / (1.0 + math.exp(-z))
        assert abs(ref["G"][i, pi] + sig * g * max(par["op"] - sp, 0.0)) < 1e-13           # the one positive's softmax weight is 1
    assert ref["counts"].tolist() == [4, 0, int(ref["count_neg"].sum())]
    # -s = -0.5 < -m: that negative has alpha- = 0, logit 0 and no gradient, and is not counted; the one at +0.5 is
    assert ref["alpha"][0, 3] == 0 and ref["G"][0, 3] == 0 and ref["logit"][0, 3] == 0 and not ref["count_neg"][0, 3]
    assert ref["count_neg"][1, 3] and ref["G"][1, 3] > 0


def saturated_batch():
    """Class 0 on (1, 0), every other row on (-1, 0) or (-0.6, 0.8): every negative of class 0's anchors has S <= -0.6 <= -m."""
    x = np.array([[1, 0], [1, 0], [-1, 0], [-0.6, 0.8], [-0.6, 0.8], [-1, 0]], np.float32)
    return x, 3, 2


def test_a_side_with_every_alpha_zero():
    x, p, k = saturated_batch()
    ref = C.reference(x, p, k, 0.4, 80.0)
    for i in (0, 1):
        assert not ref["alpha"][i, 2:].any() and not ref["G"][i, 2:].any() and not ref["count_neg"][i].any()
        # L- = log 4 (four logits of 0), L+ = the one positive's logit -80 (1.4 - 1)(1 - 0.6) with the fp32 constants
        lp = -ref["par"]["gamma"] * (ref["par"]["op"] - 1.0) * (1.0 - ref["par"]["dp"])
        assert abs(ref["ell"][i] - math.log1p(math.exp(lp + math.log(4.0)))) < 1e-12
        assert ref["G"][i, 1 - i] < 0                         # the positive still pulls: alpha+ = 0.4
    assert ref["counts"][2] == ref["count_neg"][2:].sum() > 0


def test_an_anchor_without_positives_against_the_ring_has_no_loss():
    x = np.array([[1, 0], [0, 1]], np.float32)
    mem = np.array([[1, 0], [0.6, 0.8], [0, 1], [0.8, 0.6]], np.float32)
    ref = C.xbm_reference(x, np.array([5, 7], np.int32), mem, np.array([7, 7, -1, 9], np.int32), None, 0.4, 80.0)
    assert ref["active"].tolist() == [False, True]            # label 5 has no slot; label 7 has two and one negative
    assert ref["ell"][0] == 0 and not ref["G"][0].any() and not ref["G"][:, 2].any()
    assert ref["counts"].tolist() == [2, 1, 1, 3]
    assert abs(ref["loss"] - ref["ell"][1] / 2) < 1e-15 and ref["ell"][1] > 0


# ---------------------------------------------------------------------------------------------------------------- 5. the bounds
@pytest.mark.parametrize("m,gamma", C.PARAMS)
@pytest.mark.parametrize("p,k,e,scale", [(5, 7, 33, 1.0), (9, 8, 40, 1.0), (6, 4, 16, 30.0), (2, 2, 1, 1.0)])
def test_an_fp32_emulation_of_the_rounding_form_stays_within_the_bounds(p, k, e, scale, m, gamma):
    """S~ = float32(S): one rounding, gamma_S = u.  circle_ref.emulate32 then runs the header's operations in numpy fp32."""
    x = (C.continuous(p, k, e) * np.float32(scale)).astype(np.float32)
    ref = C.reference(x, p, k, m, gamma)
    bg, bl, _ = C.bounds(ref, M.U)
    ell, g = C.emulate32(ref["S"].astype(np.float32), *M.class_masks(p, k), m, gamma)
    assert np.isfinite(ell).all() and np.isfinite(g).all()
    pair = ref["pos"] | ref["neg"]
    r_g, r_l = (np.abs(g - ref["G"])[pair] / bg[pair]).max(), (np.abs(ell - ref["ell"]) / bl).max()
    print(f"circle emulation p={p} k={k} e={e} scale={scale} m={m} gamma={gamma}: G={r_g:.3g} ell={r_l:.3g}")
    assert r_g < 1 and r_l < 1
    assert not g[~pair].any()


def test_the_saturated_side_emulates_to_exact_zeros():
    x, p, k = saturated_batch()
    ref = C.reference(x, p, k, 0.4, 80.0)
    ell, g = C.emulate32(ref["S"].astype(np.float32), *M.class_masks(p, k), 0.4, 80.0)
    assert not g[:2, 2:].any() and (np.abs(ell - ref["ell"]) <= C.bounds(ref, 0.0)[1]).all()


# ---------------------------------------------------------------------------------------------------------------- 6. fitness
@pytest.mark.parametrize("p,k,e", C.BATCH_SHAPES, ids=str)
def test_gpu_inputs_are_fit(p, k, e):
    """Grid inputs: S exact in any order.  Continuous inputs: at either path's gamma_S at most FREE_CAP of the pairs lie within dS of
    a counter threshold, for every parameter pair the GPU test runs, and at most 1 % of the anchors' violating tests are open."""
    import supcon_ref
    x, unit = C.grid(p, k, e)
    assert M.exact_in_any_order(x, unit)
    x = C.continuous(p, k, e)
    assert np.allclose(np.linalg.norm(x.astype(np.float64), axis=1), 1.0, atol=1e-6)
    for path in {C.auto_path(p, k, e), "similarity_matrix"}:
        gs = C.continuous_gs(x, path, e)
        assert (gs == 0) == (e == 1)
        assert supcon_ref.decisions(x, p, k, gs)["open"].mean() <= 0.01
        for m, gamma in C.PARAMS:
            assert C.decisions(C.reference(x, p, k, m, gamma), gs)["share"] <= C.FREE_CAP, (path, m, gamma)


@pytest.mark.parametrize("name", C.RING_CASES)
def test_ring_inputs_are_fit(name):
    c = C.ring_case(name)
    e = c["x"].shape[1]
    if c["unit"] is not None:
        assert X.exact_in_any_order(c["x"], c["mem"], c["unit"])
    for m, gamma in C.PARAMS:
        ref = C.xbm_reference(c["x"], c["labels"], c["mem"], c["mem_labels"], c["self_slots"], m, gamma)
        assert C.decisions(ref, X.gamma_s(e, c["unit"] is not None))["share"] <= C.FREE_CAP, (m, gamma)
