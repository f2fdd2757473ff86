"""CPU tests of the layer-wise adaptive optimizers 'lars' and 'lamb': tests/layerwise_ref.py (the float64 restatement of the
contract of `embnet_optimizer_layerwise_norms` / `embnet_optimizer_layerwise_step`, include/embnet.h) against torch.optim and the
rules' own properties, and the host side — what KerasOptimizer, check_optimizer_params, OptimizerSpec and the two C entry points
refuse before anything is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import layerwise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 3, 4, 2), (7,), (50,), (1,)]


def _problem(seed, steps=7):
    rs = np.random.RandomState(seed)
    w0 = [rs.randn(*s) for s in SHAPES]
    grads = [[rs.randn(*s) * 10.0 ** rs.randint(-4, 1) for s in SHAPES] for _ in range(steps)]
    return w0, grads


def _rel(a, b):
    return max(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300) for x, y in zip(a, b))


def _torch_params(w0):
    return [torch.nn.Parameter(torch.tensor(w, dtype=torch.float64)) for w in w0]


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("nesterov", [False, True])
def test_ref_lars_without_adaptation_is_torch_sgd_at_a_constant_rate(nesterov):
    """eta = 0 everywhere: v = momentum v + lr (g + wd w) is lr times torch's buffer, at a constant rate and only then."""
    w0, grads = _problem(1)
    ref = R.RefLayerwise("lars", 1e-2, [dict(tensors=[0, 1, 2, 3], weight_decay=1e-2, trust_coefficient=0.0)], momentum=0.9,
                         nesterov=nesterov)
    wn, wt = [w.copy() for w in w0], _torch_params(w0)
    opt = torch.optim.SGD(wt, lr=1e-2, momentum=0.9, weight_decay=1e-2, nesterov=nesterov)
    for gs in grads:
        ref.step(wn, gs)
        for p, g in zip(wt, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        assert _rel(wn, [p.detach().numpy() for p in wt]) < 1e-12
        assert all(ref.stats[i][2] == 1.0 for i in range(4))


@pytest.mark.parametrize("eps", [1e-12, 1e-8, 1e-6])
def test_ref_lamb_without_adaptation_is_torch_adamw(eps):
    """eta = 0 everywhere: w - lr (u_hat + wd w) is AdamW's step, and sqrt(v c2) + eps is torch's sqrt(v) / sqrt(1 - b2^t) + eps."""
    w0, grads = _problem(2)
    groups = [dict(tensors=[0, 2], weight_decay=1e-2, trust_coefficient=0.0),
              dict(tensors=[1, 3], weight_decay=0.0, lr_mult=4.0, trust_coefficient=0.0)]
    ref = R.RefLayerwise("lamb", 1e-2, groups, epsilon=eps)
    wn, wt = [w.copy() for w in w0], _torch_params(w0)
    opt = torch.optim.AdamW([dict(params=[wt[0], wt[2]], weight_decay=1e-2), dict(params=[wt[1], wt[3]], weight_decay=0.0, lr=4e-2)],
                            lr=1e-2, betas=(0.9, 0.999), eps=eps)
    for gs in grads:
        ref.step(wn, gs)
        for p, g in zip(wt, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        assert _rel(wn, [p.detach().numpy() for p in wt]) < 1e-12


@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_ref_update_does_not_see_the_gradients_scale(rule):
    """At wd = 0, momentum 0 and on LAMB's first step u is proportional to g (LAMB: g / |g|, its epsilon taken out of the way),
    and r u is not: a gradient 1e3 times larger moves the tensor by the same vector."""
    w0, grads = _problem(3, steps=1)
    out = []
    for scale in (1.0, 1e3):
        ref = R.RefLayerwise(rule, 1e-2, [dict(tensors=[0, 1, 2, 3], trust_coefficient=0.5)], momentum=0.0, epsilon=1e-300)
        wn = [w.copy() for w in w0]
        gs = list(grads[0])
        gs[2] = gs[2] * scale
        ref.step(wn, gs)
        out.append([a - b for a, b in zip(wn, w0)])
    assert np.abs(out[0][2]).max() > 0
    assert _rel(out[1], out[0]) < 1e-12


@pytest.mark.parametrize("rule,wd", [("lars", 0.0), ("lars", 0.1), ("lamb", 0.0), ("lamb", 0.1)])
def test_ref_step_norm_is_lr_eta_weight_norm(rule, wd):
    w0, grads = _problem(4, steps=3)
    ref = R.RefLayerwise(rule, 1e-2, [dict(tensors=[0, 2], weight_decay=wd, trust_coefficient=0.25),
                                      dict(tensors=[1, 3], weight_decay=wd, lr_mult=4.0, trust_coefficient=2.0)], momentum=0.0)
    wn = [w.copy() for w in w0]
    for gs in grads:
        old = [w.copy() for w in wn]
        ref.step(wn, gs)
        for i, (lr, eta) in enumerate([(1e-2, 0.25), (4e-2, 2.0), (1e-2, 0.25), (4e-2, 2.0)]):
            step, norm = np.sqrt(np.sum((wn[i] - old[i]) ** 2)), np.sqrt(np.sum(old[i] ** 2))
            assert abs(step - lr * eta * norm) <= 1e-12 * lr * eta * norm, (rule, i)
            assert abs(ref.stats[i][0] - norm * norm) <= 1e-12 * norm * norm


@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_ref_zero_norms_give_a_ratio_of_one(rule):
    w0, grads = _problem(5, steps=1)
    ref = R.RefLayerwise(rule, 1e-2, [dict(tensors=[0, 1, 2, 3], trust_coefficient=0.5)], momentum=0.0)
    wn = [w.copy() for w in w0]
    wn[0][...] = 0.0                                                 # |w| = 0
    gs = list(grads[0])
    gs[2] = np.zeros_like(gs[2])                                     # |u| = 0 (no decay)
    gs[3] = None
    before = wn[2].copy()
    ref.step(wn, gs)
    assert ref.stats[0][0] == 0.0 and ref.stats[0][1] > 0 and ref.stats[0][2] == 1.0
    assert ref.stats[2][0] > 0 and ref.stats[2][1] == 0.0 and ref.stats[2][2] == 1.0
    assert np.array_equal(wn[2], before)
    assert ref.stats[3] == (0.0, 0.0, 1.0) and np.array_equal(wn[3], w0[3])
    assert ref.stats[1][2] != 1.0 and np.isfinite(ref.stats[1][2])
    assert np.abs(wn[0]).max() > 0                                   # a zero tensor still moves, at the plain rate


def test_ref_fp32_emulation_stays_close_to_the_contract():
    """The emulation the GPU test takes its bound from is the same rule: a few fp32 roundings away after three steps."""
    for rule in ("lars", "lamb"):
        w0, grads = _problem(6, steps=3)
        w0 = [w.astype(np.float32).astype(np.float64) for w in w0]
        grads = [[g.astype(np.float32).astype(np.float64) for g in gs] for gs in grads]
        groups = [dict(tensors=[0, 1, 2, 3], weight_decay=1e-2, trust_coefficient=0.1)]
        a, b = R.RefLayerwise(rule, 1e-2, groups), R.RefLayerwise(rule, 1e-2, groups, fp32=True)
        wa, wb = [w.copy() for w in w0], [w.copy() for w in w0]
        for gs in grads:
            a.step(wa, gs)
            b.step(wb, gs)
        assert 0 < _rel(wb, wa) < 1e-5
        assert all(np.array_equal(w, w.astype(np.float32)) for w in wb)


# ------------------------------------------------------------------------------------------------ the host side
def _cpu_params(n=2):
    return [torch.nn.Parameter(torch.zeros(3, 3)) for _ in range(n)]


def test_constructor_defaults_and_refusals():
    from embeddingnet_amd.optimizers import KerasOptimizer
    ps = _cpu_params(3)
    lars = KerasOptimizer(ps, "lars", 0.3)
    assert lars.layerwise and lars.grouped and lars.momentum == 0.9 and lars.param_groups[0]["trust_coefficient"] == 1e-3
    lamb = KerasOptimizer([dict(params=ps[:2], weight_decay=1e-2), dict(params=ps[2:], trust_coefficient=0.0, lr_mult=4.0)], "lamb", 1e-3)
    assert lamb.layerwise and lamb.grouped and lamb.momentum == 0.0
    assert [g["trust_coefficient"] for g in lamb.param_groups] == [1.0, 0.0] and lamb.adapted == [0, 1]
    assert KerasOptimizer(ps, "lars", 0.3, momentum=0.0, trust_coefficient=0.02).param_groups[0]["trust_coefficient"] == 0.02
    assert KerasOptimizer(ps, "lars", 0.3, nesterov=True).nesterov
    # slots: lars always keeps the velocity, lamb both moments
    assert [s is not None for s in KerasOptimizer(ps, "lars", 0.3, momentum=0.0)._slots(ps[0])] == [True, False]
    assert [s is not None for s in lamb._slots(ps[0])] == [True, True]
    # the rows the kernels read: the decay itself, not lr * wd; LAMB's bias corrections in c1 and c2
    assert lamb.group_scalars(3) == [1e-3, 0.0, 1e-2, 1.0, 4e-3, 0.0, 0.0, 0.0]
    code, coef = lamb.scalars(3)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))       # the corrections belong to the betas the kernel holds
    assert code == 1 and coef == [1e-3, 0.9, 0.999, 1e-7, 1.0 / (1.0 - b1 ** 3), 1.0 / (1.0 - b2 ** 3)]
    code, coef = lars.scalars(3)
    assert code == 0 and coef[0] == 0.3 and coef[4:] == [0.0, 0.0]
    assert lars.group_scalars(1) == [0.3, 0.0, 0.0, 1e-3]
    with pytest.raises(ValueError, match="trust_coefficient must not be negative"):
        KerasOptimizer(ps, "lars", 0.3, trust_coefficient=-1e-3)
    with pytest.raises(ValueError, match="trust_coefficient must not be negative"):
        KerasOptimizer([dict(params=ps, trust_coefficient=-1.0)], "lamb", 1e-3)
    with pytest.raises(ValueError, match="momentum and nesterov belong"):
        KerasOptimizer(ps, "lamb", 1e-3, momentum=0.9)
    with pytest.raises(ValueError, match="nesterov"):
        KerasOptimizer(ps, "lamb", 1e-3, nesterov=True)
    with pytest.raises(ValueError, match="trust_coefficient belongs"):
        KerasOptimizer(ps, "adam", 1e-3, trust_coefficient=1.0)
    with pytest.raises(ValueError, match="exclusive"):
        KerasOptimizer(ps, "lars", 0.3, clipvalue=1.0, global_clipnorm=1.0)
    with pytest.raises(ValueError, match="at most 8"):
        KerasOptimizer([dict(params=[p]) for p in _cpu_params(9)], "lamb", 1e-3)
    with pytest.raises(AttributeError, match="trust_ratios"):
        KerasOptimizer(ps, "adam", 1e-3).trust_ratios
    with pytest.raises(KeyError):
        KerasOptimizer(ps, "lans", 1e-3)


def test_slots_in_state_files(tmp_path):
    from embeddingnet_amd.optimizers import KerasOptimizer, load_optimizer_state, save_optimizer_state
    a, b = _cpu_params(2)
    opt = KerasOptimizer([a, b], "lamb", 1e-3)
    for p in (a, b):
        for s in opt._slots(p):
            s.copy_(torch.randn(3, 3))
    opt.iterations = 5
    save_optimizer_state(str(tmp_path / "l.npz"), opt, {"a": a, "b": b})
    a2, b2 = _cpu_params(2)
    opt2 = KerasOptimizer([a2, b2], "lamb", 1e-3)
    load_optimizer_state(str(tmp_path / "l.npz"), opt2, {"a": a2, "b": b2})
    assert opt2.iterations == 5
    for k in ("slot1", "slot2"):
        assert torch.equal(opt2.state[a2][k], opt.state[a][k]) and torch.equal(opt2.state[b2][k], opt.state[b][k])
    from embeddingnet_amd._lib import EmbnetError
    with pytest.raises(EmbnetError, match="optimizer state is for 'lamb'"):
        load_optimizer_state(str(tmp_path / "l.npz"), KerasOptimizer([a2, b2], "lars", 0.3), {"a": a2, "b": b2})


def test_optimizer_params_and_spec(tmp_path):
    from embeddingnet_amd.utils import OptimizerSpec, check_optimizer_params, parse_params
    assert check_optimizer_params({"trust_coefficient": 0.001}) == {"trust_coefficient": 0.001}
    for bad in (-1e-3, "0.001", True, float("nan")):
        with pytest.raises(ValueError, match="trust_coefficient must be a number >= 0"):
            check_optimizer_params({"trust_coefficient": bad})
    with pytest.raises(ValueError, match="unknown keys.*trust_coef"):
        check_optimizer_params({"trust_coef": 1e-3})
    kernel, bias, gem_p, proxies = (torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(3)),
                                    torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(5, 3)))
    assert OptimizerSpec("lamb", 1e-3).rule == "lamb" and OptimizerSpec("lars", 0.3).rule == "lars"
    assert OptimizerSpec("whatever", 1e-2).rule == "sgd" and OptimizerSpec("LAMB", 1e-2).rule == "sgd"
    # three groups, with or without optimizer_params; 'other' neither decayed nor adapted
    opt = OptimizerSpec("lamb", 1e-3).build([kernel, bias, gem_p], proxies=[proxies])
    assert opt.rule == "lamb" and opt.group_names == ["kernels", "other", "proxies"]
    assert [g["trust_coefficient"] for g in opt.param_groups] == [1.0, 0.0, 1.0]
    assert opt.param_groups[1]["params"] == [bias, gem_p] and opt.param_groups[1]["weight_decay"] == 0.0
    spec = OptimizerSpec("lamb", 1e-3, {"weight_decay": 1e-2, "proxy_lr_mult": 10, "proxy_weight_decay": 1e-3, "trust_coefficient": 0.5,
                                        "global_clipnorm": 10})
    opt = spec.build([kernel, bias], proxies=[proxies])
    assert [(g["lr_mult"], g["weight_decay"], g["trust_coefficient"]) for g in opt.param_groups] == \
        [(1.0, 1e-2, 0.5), (1.0, 0.0, 0.0), (10.0, 1e-3, 0.5)]
    assert opt.global_clipnorm == 10.0 and opt.adapted == [0, 2]
    opt = OptimizerSpec("lars", 0.3, {"momentum": 0.8, "nesterov": True, "weight_decay": 1e-6}).build([kernel, bias])
    assert opt.rule == "lars" and opt.group_names == ["kernels", "other"] and opt.momentum == 0.8 and opt.nesterov
    assert [g["trust_coefficient"] for g in opt.param_groups] == [1e-3, 0.0]
    assert OptimizerSpec("lars", 0.3).build([kernel, bias]).momentum == 0.9
    with pytest.raises(ValueError, match="proxy modes"):
        OptimizerSpec("lamb", 1e-3, {"proxy_lr_mult": 10}).build([kernel, bias])
    with pytest.raises(ValueError, match="trust_coefficient belongs"):
        OptimizerSpec("adam", 1e-3, {"trust_coefficient": 1.0}).build([kernel, bias])
    with pytest.raises(ValueError, match="momentum and nesterov belong"):
        OptimizerSpec("lamb", 1e-3, {"momentum": 0.9}).build([kernel, bias])
    for name, rule in (("simple2_supcon_lars_synthetic", "lars"), ("simple2_proxy_anchor_lamb_synthetic", "lamb")):
        spec = parse_params(os.path.join(ROOT, "configs", name + ".yml"))["train"]["optimizer"]
        assert spec.rule == rule and isinstance(spec.params["weight_decay"], float)
    # the other rules are dispatched as before: without the key one group, the proxies one more tensor of it
    plain = OptimizerSpec("adam", 1e-3).build([kernel, bias], proxies=[proxies])
    assert not plain.grouped and not plain.layerwise and len(plain.param_groups) == 1
    assert "trust_coefficient" not in plain.param_groups[0]


def test_new_exports_have_prototypes():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("embnet_optimizer_layerwise_norms", "embnet_optimizer_layerwise_step", "embnet_optimizer_layerwise_workspace_bytes"):
        assert name in protos and hasattr(lib, name), name
    assert len(protos["embnet_optimizer_layerwise_norms"][1]) == 20 and len(protos["embnet_optimizer_layerwise_step"][1]) == 20
    bound = _lib.lib()
    assert bound.embnet_optimizer_layerwise_workspace_bytes(100) == 16 + 16 * 100
    assert bound.embnet_optimizer_layerwise_workspace_bytes(0) == 0
    header = open(_lib.HEADER_PATH).read()
    assert "enum { EMBNET_LAYERWISE_LARS = 0, EMBNET_LAYERWISE_LAMB = 1 };" in header
    assert "consecutive and ascending" in header                      # the chunk list's new precondition is stated


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """Validation happens before any launch (the pointers are dummies and never dereferenced, except the host rows)."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    p = 4096                                                         # non-null, 16-byte aligned
    rows = np.zeros((9, 4), dtype=np.float32)
    rows[:, 0] = 1e-3

    def norms(rule=1, table=p, chunks=p, n_tensors=1, n_chunks=3, coef=rows.ctypes.data, n_groups=1, clipvalue=0.0, scale=None, ws=p,
              ws_bytes=16 + 16 * 3, stats=p):
        return lib.embnet_optimizer_layerwise_norms(rule, table, n_tensors, chunks, n_chunks, coef, n_groups, 0.9, 0.999, 1e-7, 1.0, 1.0,
                                                    clipvalue, scale, None, None, ws, ws_bytes, stats, None)

    def step(rule=1, table=p, chunks=p, n_tensors=1, n_chunks=3, coef=rows.ctypes.data, n_groups=1, momentum=0.0, nesterov=0,
             clipvalue=0.0, scale=None, stats=p):
        return lib.embnet_optimizer_layerwise_step(rule, table, n_tensors, chunks, n_chunks, coef, n_groups, 0.9, 0.999, 1e-7, 1.0, 1.0,
                                                   momentum, nesterov, clipvalue, scale, None, None, stats, None)

    both = [(dict(table=None), -1, b"null pointer"), (dict(chunks=None), -1, b"null pointer"), (dict(coef=None), -1, b"null pointer"),
            (dict(stats=None), -1, b"null pointer"), (dict(n_tensors=0), -1, b"empty table"), (dict(n_chunks=0), -1, b"empty table"),
            (dict(rule=2), -1, b"unknown rule 2"), (dict(rule=-1), -1, b"unknown rule -1"), (dict(rule=6), -1, b"unknown rule 6"),
            (dict(n_groups=0), -1, b"0 groups"), (dict(n_groups=9), -1, b"9 groups"), (dict(clipvalue=-1.0), -1, b"negative clipvalue"),
            (dict(clipvalue=1.0, scale=p), -1, b"exclusive"), (dict(stats=p + 4), -1, b"8-byte aligned")]
    only_norms = [(dict(ws=None), -1, b"null pointer"), (dict(ws=p + 8), -1, b"16-byte aligned"),
                  (dict(ws_bytes=16 + 16 * 3 - 1), -3, b"workspace")]
    only_step = [(dict(nesterov=1), -1, b"belong to LARS"), (dict(momentum=0.9), -1, b"belong to LARS"),
                 (dict(rule=0, momentum=-0.5), -1, b"negative momentum")]
    for fn, name, cases in ((norms, b"optimizer_layerwise_norms", both + only_norms), (step, b"optimizer_layerwise_step", both + only_step)):
        for kw, rc, msg in cases:
            lib.embnet_pairwise_dist_f32(None, 4, 4, None, 0, None, 0, None)          # leaves another message behind
            assert fn(**kw) == rc and msg in lib.embnet_last_error() and name in lib.embnet_last_error(), (kw, lib.embnet_last_error())
    # and the old grouped entry point goes on refusing what lies past its own rules
    assert lib.embnet_optimizer_step_groups(6, p, 1, p, 1, rows.ctypes.data, 1, 0.9, 0.999, 1e-7, 0.0, 0.0, 0, 0.0, None, None, None,
                                            None) == -1 and b"unknown rule 6" in lib.embnet_last_error()
