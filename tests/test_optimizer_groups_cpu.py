"""CPU tests of the grouped optimizer: tests/optimizer_ref.py (the float64 restatement of the per-element contract of
`embnet_optimizer_step_groups`, include/embnet.h) against torch.optim and NumPy, and the host side — what KerasOptimizer,
parse_params and the C entry points refuse before anything is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import optimizer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 3, 4, 2), (7,), (50,), (1,)]


def _problem(seed, steps=7):
    rs = np.random.RandomState(seed)
    w0 = [rs.randn(*s) for s in SHAPES]
    grads = [[rs.randn(*s) * 10.0 ** rs.randint(-4, 1) for s in SHAPES] for _ in range(steps)]
    return w0, grads


def _rel(a, b):
    return max(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("nesterov", [False, True])
def test_ref_momentum_is_torch_sgd_at_a_constant_rate(nesterov):
    """Keras keeps v = -lr * (torch's buffer): the two forms coincide at a constant rate, and only then."""
    w0, grads = _problem(1)
    ref = R.RefOptimizer("sgd", 1e-2, [dict(tensors=[0, 1, 2, 3])], momentum=0.9, nesterov=nesterov)
    wn = [w.copy() for w in w0]
    wt = [torch.nn.Parameter(torch.tensor(w, dtype=torch.float64)) for w in w0]
    opt = torch.optim.SGD(wt, lr=1e-2, momentum=0.9, nesterov=nesterov)
    for gs in grads:
        ref.step(wn, gs)
        for p, g in zip(wt, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        assert _rel(wn, [p.detach().numpy() for p in wt]) < 1e-12


def test_ref_adam_with_decay_is_torch_adamw():
    """torch puts epsilon inside the bias correction; at 1e-300 it vanishes from both forms."""
    w0, grads = _problem(2)
    groups = [dict(tensors=[0, 2], weight_decay=1e-2), dict(tensors=[1, 3], weight_decay=0.0, lr_mult=4.0)]
    ref = R.RefOptimizer("adam", 1e-2, groups, epsilon=1e-300)
    wn = [w.copy() for w in w0]
    wt = [torch.nn.Parameter(torch.tensor(w, dtype=torch.float64)) for w in w0]
    opt = torch.optim.AdamW([dict(params=[wt[0], wt[2]], weight_decay=1e-2), dict(params=[wt[1], wt[3]], weight_decay=0.0, lr=4e-2)],
                            lr=1e-2, betas=(0.9, 0.999), eps=1e-300)
    for gs in grads:
        ref.step(wn, gs)
        for p, g in zip(wt, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        assert _rel(wn, [p.detach().numpy() for p in wt]) < 1e-12


@pytest.mark.parametrize("c", [1e-3, 1.0, 1e6])
def test_ref_global_clipnorm_keeps_the_direction(c):
    _, grads = _problem(3, steps=1)
    gs = grads[0][:3] + [None]                                       # a tensor without a gradient is not in the norm
    flat = np.concatenate([g.ravel() for g in gs if g is not None])
    norm = np.sqrt(np.sum(flat * flat))
    out, n2 = R.clip_gradients(gs, global_clipnorm=c)
    assert out[3] is None and abs(n2 - norm * norm) <= 1e-12 * n2
    oflat = np.concatenate([g.ravel() for g in out if g is not None])
    onorm = np.sqrt(np.sum(oflat * oflat))
    assert abs(onorm - min(norm, c)) <= 1e-12 * min(norm, c)
    assert np.abs(oflat / onorm - flat / norm).max() <= 1e-12        # the same unit vector


def test_ref_clipvalue_is_np_clip():
    _, grads = _problem(4, steps=1)
    out, n2 = R.clip_gradients(grads[0], clipvalue=0.05)
    for o, g in zip(out, grads[0]):
        assert np.array_equal(o, np.clip(g, -0.05, 0.05))
    assert n2 == sum(np.sum(g * g) for g in grads[0])                 # the norm is the one before clipping


def test_ref_skips_a_tensor_without_a_gradient_entirely():
    w0, grads = _problem(5, steps=2)
    ref = R.RefOptimizer("adam", 1e-2, [dict(tensors=[0, 1, 2, 3], weight_decay=0.1)], global_clipnorm=1.0, l2={1: 1e-3})
    wn = [w.copy() for w in w0]
    ref.step(wn, grads[0])
    before = (wn[1].copy(), ref.slots[(1, "slot1")].copy(), ref.slots[(1, "slot2")].copy())
    gs = list(grads[1])
    gs[1] = None
    ref.step(wn, gs)
    assert np.array_equal(wn[1], before[0])                           # no decay either
    assert np.array_equal(ref.slots[(1, "slot1")], before[1]) and np.array_equal(ref.slots[(1, "slot2")], before[2])
    assert ref.n2 == sum(np.sum(g * g) for g in gs if g is not None)


# ------------------------------------------------------------------------------------------------ the host side
def _cpu_params(n=2):
    return [torch.nn.Parameter(torch.zeros(3, 3)) for _ in range(n)]


def test_constructor_refusals():
    from embeddingnet_amd.optimizers import KerasOptimizer
    ps = _cpu_params(9)
    with pytest.raises(ValueError, match="at most 8"):
        KerasOptimizer([dict(params=[p]) for p in ps], "adam", 1e-3)
    with pytest.raises(ValueError, match="exclusive"):
        KerasOptimizer(ps, "adam", 1e-3, clipvalue=1.0, global_clipnorm=1.0)
    for kw in (dict(clipvalue=-1.0), dict(global_clipnorm=-1.0), dict(momentum=-0.1)):
        with pytest.raises(ValueError, match="negative"):
            KerasOptimizer(ps, "sgd", 1e-3, **kw)
    with pytest.raises(ValueError, match="negative"):
        KerasOptimizer([dict(params=ps, weight_decay=-1e-4)], "adam", 1e-3)
    with pytest.raises(ValueError, match="nesterov"):
        KerasOptimizer(ps, "sgd", 1e-3, nesterov=True)
    with pytest.raises(ValueError, match="momentum"):
        KerasOptimizer(ps, "adam", 1e-3, momentum=0.9)


def test_groups_and_the_plain_optimizer():
    """Eight groups are accepted; one group without options is the plain optimizer (step() then issues the call it always did)."""
    from embeddingnet_amd.optimizers import KerasOptimizer
    ps = _cpu_params(8)
    opt = KerasOptimizer([dict(params=[p], lr_mult=float(i + 1)) for i, p in enumerate(ps)], "adam", 1e-3)
    assert opt.grouped and len(opt.param_groups) == 8
    assert [g["lr"] * g["lr_mult"] for g in opt.param_groups] == [1e-3 * (i + 1) for i in range(8)]
    for g in opt.param_groups:
        g["lr"] = 5e-4                                               # a schedule writes one rate into every group ...
    rows = opt._group_rows(1)[4]
    assert [r[0] for r in rows] == [5e-4 * (i + 1) for i in range(8)]   # ... and the ratios stay
    plain = KerasOptimizer(ps, "adam", 1e-3)
    assert not plain.grouped and plain.group_scalars(1) == []
    assert not KerasOptimizer([dict(params=ps)], "sgd", 1e-3).grouped
    for kw in (dict(momentum=0.9), dict(clipvalue=1.0), dict(global_clipnorm=1.0)):
        assert KerasOptimizer(ps, "sgd", 1e-3, **kw).grouped
    assert KerasOptimizer([dict(params=ps, weight_decay=1e-4)], "adam", 1e-3).grouped
    # d_g = lr_g * wd_g, c1 at the group's own rate
    opt = KerasOptimizer([dict(params=ps[:1], weight_decay=1e-2), dict(params=ps[1:], lr_mult=4.0)], "adam", 1e-2)
    rule, b1, b2, c2, rows = opt._group_rows(3)
    assert rule == 2 and rows[0][2] == 1e-2 * 1e-2 and rows[1][2] == 0.0
    assert rows[1][0] == 4e-2 and abs(rows[1][1] / rows[0][1] - 4.0) < 1e-15
    assert KerasOptimizer(ps, "sgd", 1e-2, momentum=0.9)._group_rows(1)[0] == 5


def test_momentum_slot_in_state_files(tmp_path):
    """The velocity is slot1: it is saved by name, and a file without it loads with the slot at zero."""
    from embeddingnet_amd.optimizers import KerasOptimizer, load_optimizer_state, save_optimizer_state
    a, b = _cpu_params(2)
    opt = KerasOptimizer([a, b], "sgd", 1e-2, momentum=0.9)
    for p in (a, b):
        s1, s2 = opt._slots(p)
        assert s2 is None
        s1.copy_(torch.randn(3, 3))
    opt.iterations = 4
    save_optimizer_state(str(tmp_path / "m.npz"), opt, {"a": a, "b": b})
    a2, b2 = _cpu_params(2)
    opt2 = KerasOptimizer([a2, b2], "sgd", 1e-2, momentum=0.9)
    load_optimizer_state(str(tmp_path / "m.npz"), opt2, {"a": a2, "b": b2})
    assert opt2.iterations == 4
    assert torch.equal(opt2.state[a2]["slot1"], opt.state[a]["slot1"]) and torch.equal(opt2.state[b2]["slot1"], opt.state[b]["slot1"])
    sd = opt.state_dict()
    opt3 = KerasOptimizer(_cpu_params(2), "sgd", 1e-2, momentum=0.9)
    opt3.load_state_dict(sd)
    assert torch.equal(opt3.state[opt3.param_groups[0]["params"][0]]["slot1"], opt.state[a]["slot1"])
    plain = KerasOptimizer([a, b], "sgd", 1e-2)                        # plain SGD: no slot in the file
    save_optimizer_state(str(tmp_path / "p.npz"), plain, {"a": a, "b": b})
    opt4 = KerasOptimizer([a2, b2], "sgd", 1e-2, momentum=0.9)
    load_optimizer_state(str(tmp_path / "p.npz"), opt4, {"a": a2, "b": b2})
    assert float(opt4.state[a2]["slot1"].abs().max()) == 0.0


def _config(tmp_path, optimizer_params):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "simple2_proxy_anchor_synthetic.yml")))
    cfg["TRAIN"]["optimizer"] = "adam"
    cfg["TRAIN"]["optimizer_params"] = optimizer_params
    path = tmp_path / "c.yml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def test_parse_params_and_optimizer_spec(tmp_path):
    from embeddingnet_amd.utils import OptimizerSpec, parse_params
    with pytest.raises(ValueError, match="unknown keys.*weight_decy"):
        parse_params(_config(tmp_path, {"weight_decy": 1e-4}))
    spec = parse_params(_config(tmp_path, {"weight_decay": 1e-4, "proxy_lr_mult": 100, "clipvalue": 10}))["train"]["optimizer"]
    assert isinstance(spec, OptimizerSpec) and spec.params == {"weight_decay": 1e-4, "proxy_lr_mult": 100, "clipvalue": 10}
    kernel, bias, proxies = (torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(3)),
                             torch.nn.Parameter(torch.zeros(5, 3)))
    opt = spec.build([kernel, bias], proxies=[proxies])
    assert opt.rule == "adam" and opt.group_names == ["kernels", "other", "proxies"] and opt.clipvalue == 10.0
    assert [(g["lr_mult"], g["weight_decay"]) for g in opt.param_groups] == [(1.0, 1e-4), (1.0, 0.0), (100.0, 0.0)]
    assert opt.param_groups[0]["params"] == [kernel] and opt.param_groups[1]["params"] == [bias]
    with pytest.raises(ValueError, match="proxy modes"):
        spec.build([kernel, bias])                                   # the proxy_* keys outside the proxy modes
    # sgd plus momentum; names are dispatched as before (unknown -> sgd)
    opt = OptimizerSpec("whatever", 1e-2, {"momentum": 0.9, "nesterov": True, "weight_decay": 5e-4}).build([kernel, bias])
    assert opt.rule == "sgd" and opt.momentum == 0.9 and opt.nesterov and opt.group_names == ["kernels", "other"]
    # without the key: today's optimizer, the proxies one more tensor of its single group
    plain = parse_params(os.path.join(ROOT, "configs", "simple2_proxy_anchor_synthetic.yml"))["train"]["optimizer"]
    opt = plain.build([kernel, bias], proxies=[proxies])
    assert not opt.grouped and len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == 3
    for name in ("simple2_proxy_anchor_adamw_synthetic", "simple2_proxy_anchor_clipnorm_synthetic"):
        spec = parse_params(os.path.join(ROOT, "configs", name + ".yml"))["train"]["optimizer"]
        assert spec.rule == "adam" and spec.params["weight_decay"] == 1e-4 and spec.params["proxy_lr_mult"] == 100


def test_new_exports_have_prototypes():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("embnet_optimizer_step_groups", "embnet_optimizer_grad_norm", "embnet_optimizer_grad_norm_workspace_bytes"):
        assert name in protos and hasattr(lib, name), name
    assert len(protos["embnet_optimizer_step_groups"][1]) == 18 and len(protos["embnet_optimizer_grad_norm"][1]) == 10
    bound = _lib.lib()
    assert bound.embnet_abi_version() == 22
    assert bound.embnet_optimizer_grad_norm_workspace_bytes(100) == 16 + 8 * 100
    assert bound.embnet_optimizer_grad_norm_workspace_bytes(0) == 0
    assert "#define EMBNET_OPT_MAX_GROUPS 8" in open(_lib.HEADER_PATH).read()


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """Validation happens before any launch (the pointers are dummies and never dereferenced, except the host rows)."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    p = 4096                                                         # non-null, 16-byte aligned
    rows = np.zeros((9, 4), dtype=np.float32)
    rows[:, 0] = 1e-3

    def step(rule=2, table=p, n_groups=1, momentum=0.0, nesterov=0, clipvalue=0.0, scale=None, coef=rows.ctypes.data):
        return lib.embnet_optimizer_step_groups(rule, table, 1, p, 1, coef, n_groups, 0.9, 0.999, 1e-7, 0.0, momentum, nesterov,
                                                clipvalue, scale, None, None, None)

    cases = [(dict(table=None), b"null pointer"), (dict(coef=None), b"null pointer"), (dict(n_groups=0), b"0 groups"),
             (dict(n_groups=9), b"9 groups"), (dict(rule=6), b"unknown rule 6"), (dict(rule=-1), b"unknown rule -1"),
             (dict(clipvalue=-1.0), b"negative clipvalue"), (dict(clipvalue=1.0, scale=p), b"exclusive"),
             (dict(rule=5, momentum=-0.5), b"negative momentum"), (dict(momentum=0.9), b"momentum belongs"),
             (dict(nesterov=1), b"momentum belongs")]
    for kw, msg in cases:
        lib.embnet_pairwise_dist_f32(None, 4, 4, None, 0, None, 0, None)          # leaves another message behind
        assert step(**kw) == -1 and msg in lib.embnet_last_error(), (kw, lib.embnet_last_error())

    def norm(table=p, clipnorm=1.0, ws=p, ws_bytes=16 + 8 * 3, n_chunks=3, out=p):
        return lib.embnet_optimizer_grad_norm(table, 1, p, n_chunks, clipnorm, ws, ws_bytes, out, out, None)

    for kw, rc, msg in [(dict(table=None), -1, b"null pointer"), (dict(out=None), -1, b"null pointer"),
                        (dict(clipnorm=-1.0), -1, b"must be positive"), (dict(clipnorm=0.0), -1, b"must be positive"),
                        (dict(n_chunks=0), -1, b"empty table"), (dict(ws=p + 8), -1, b"16-byte aligned"),
                        (dict(ws_bytes=16 + 8 * 3 - 1), -3, b"workspace")]:
        lib.embnet_pairwise_dist_f32(None, 4, 4, None, 0, None, 0, None)
        assert norm(**kw) == rc and msg in lib.embnet_last_error(), (kw, lib.embnet_last_error())
