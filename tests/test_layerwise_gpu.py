"""GPU tests of the layer-wise adaptive optimizers — `embnet_optimizer_layerwise_norms` and `embnet_optimizer_layerwise_step` as
KerasOptimizer('lars' / 'lamb') launches them — against tests/layerwise_ref.py (float64), bit for bit against themselves, under
graph replay and through tools/train.py.

The shapes, the three groups and the l2 table are test_optimizer_groups_gpu.py's: a scalar tail, a one-element tensor, more than
one chunk; tensor 3 has no gradient on even steps; the second group is exempt from adaptation (trust coefficient 0).  The metric of
the parity test is that test's, per tensor and step: max|got - ref| / max(max|ref_new|, max|ref_old|).

The bound comes from an fp32 NumPy emulation of the contract (layerwise_ref.RefLayerwise(fp32=True): every kernel rounding, the
norms in f64) on exactly these inputs, 9 steps, run on the CPU.  Its worst error against the float64 reference per combination:
    lars  none 1.86e-7   decay 1.85e-7   clipvalue 1.80e-7   clipnorm 1.86e-7   decay+clipnorm 1.92e-7
    lamb  none 1.62e-7   decay 1.75e-7   clipvalue 1.68e-7   clipnorm 2.02e-7   decay+clipnorm 1.69e-7
(worst_emulated() below computes them again).  Times 6, the headroom f-19 gave its own emulation's 5e-7: 1.15e-6 for lars and
1.21e-6 for lamb, each rule held to its own; both lie inside f-19's 3e-6.  (With LAMB's bias corrections computed from the
float64 betas the emulation reached 7.2e-7: the kernel's 1 - b2 is 1 - 0.999f, 1.3e-5 off 1e-3 in relative terms, which
sqrt(v c2) carries into every step of the exempt group at its fourfold rate.  KerasOptimizer.scalars therefore computes c1 and
c2 from the betas as fp32 holds them, and v c2 is the weighted mean it stands for.)"""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import layerwise_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(3, 3, 16, 8), (7,), (5000,), (1,), (4096 + 13,), (64, 64)]
GROUPS = [([0, 2], 1.0, 1e-2), ([1, 3], 4.0, 0.0), ([4, 5], 0.25, 2e-2)]          # tensors, lr_mult, weight_decay
ETA = {"lars": [1e-2, 0.0, 2e-2], "lamb": [1.0, 0.0, 0.5]}                          # per group; the second one is exempt
LR = {"lars": 0.1, "lamb": 1e-2}
L2 = {0: 2e-4, 5: 1e-3}
OPTIONS = {"none": (False, {}), "decay": (True, {}), "clipvalue": (False, dict(clipvalue=0.05)),
           "clipnorm": (False, dict(global_clipnorm=1.0)), "decay+clipnorm": (True, dict(global_clipnorm=1.0))}
BOUND = {"lars": 6 * 1.92e-7, "lamb": 6 * 2.02e-7}                                  # six times the emulation's worst (docstring)
EPS24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def g(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _inputs(seed, steps=9):
    """-> (initial weights, per step the gradients; tensor 3 has none on even steps), all fp32 values held in float64."""
    rs = np.random.RandomState(seed)
    w0 = [f32(rs.randn(*s)) for s in SHAPES]
    grads = []
    for step in range(1, steps + 1):
        gs = [f32(rs.randn(*s) * 10.0 ** rs.randint(-4, 1)) for s in SHAPES]
        if step % 2 == 0:
            gs[3] = None
        grads.append(gs)
    return w0, grads


def _ref(rule, decay, kw, l2=L2, fp32=False):
    groups = [dict(tensors=idx, lr_mult=m, weight_decay=wd if decay else 0.0, trust_coefficient=eta)
              for (idx, m, wd), eta in zip(GROUPS, ETA[rule])]
    return R.RefLayerwise(rule, LR[rule], groups, l2=l2, fp32=fp32, **kw)


def _pair(dev, w0, rule, decay, kw, l2=L2):
    """The device optimizer over three groups and its float64 reference."""
    from embeddingnet_amd.optimizers import KerasOptimizer
    ws = [torch.nn.Parameter(g(w, dev)) for w in w0]
    opt = KerasOptimizer([dict(params=[ws[i] for i in idx], lr_mult=m, weight_decay=wd if decay else 0.0, trust_coefficient=eta)
                          for (idx, m, wd), eta in zip(GROUPS, ETA[rule])], rule, LR[rule], **kw)
    opt.set_l2([(ws[i], lam) for i, lam in l2.items()])
    return ws, opt, _ref(rule, decay, kw, l2)


def _metric(got, new, was):
    return np.abs(got - new).max() / max(np.abs(new).max(), np.abs(was).max())


def worst_emulated(seed=5):
    """The docstring's table: the fp32 emulation against the float64 reference on the parity test's inputs (CPU only)."""
    out = {}
    for rule in ("lars", "lamb"):
        for name, (decay, kw) in OPTIONS.items():
            w0, grads = _inputs(seed)
            a, b = _ref(rule, decay, kw), _ref(rule, decay, kw, fp32=True)
            wa, wb = [w.copy() for w in w0], [w.copy() for w in w0]
            worst = 0.0
            for step, gs in enumerate(grads, 1):
                if step == 6:
                    a.lr = b.lr = LR[rule] / 2
                old = [w.copy() for w in wa]
                a.step(wa, gs)
                b.step(wb, gs)
                worst = max(worst, max(_metric(y, x, o) for x, y, o in zip(wa, wb, old)))
            out[rule, name] = worst
    return out


def _set_grads(ws, gs, dev):
    for w, gr in zip(ws, gs):
        w.grad = None if gr is None else g(gr, dev)


def _stats(opt, ws):
    """-> (W2, U2, r) float64 arrays per tensor of `ws` (the stats' rows are in the order of the optimizer's groups), r read from
    the float view the trainers log."""
    s = opt._stats[0].cpu().numpy()
    r = opt.trust_ratios.cpu().numpy().astype(np.float64)
    assert np.array_equal(s[:, 2:3].copy().view(np.float32)[:, 0], r.astype(np.float32))
    assert np.all(s[:, 2:3].copy().view(np.float32)[:, 1] == 0.0)                  # the pad word
    rows = [next(j for j, q in enumerate(opt._tensors) if q is w) for w in ws]
    return s[rows, 0], s[rows, 1], r[rows]


def _state(ws, opt):
    out = [w.detach().clone() for w in ws]
    for w in ws:
        for k in ("slot1", "slot2"):
            if k in opt.state[w]:
                out.append(opt.state[w][k].clone())
    return out


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("options", list(OPTIONS))
@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_layerwise_steps_vs_reference(dev, rule, options):
    decay, kw = OPTIONS[options]
    w0, grads = _inputs(5)
    ws, opt, ref = _pair(dev, w0, rule, decay, kw)
    assert opt.grouped and opt.layerwise
    wn = [w.copy() for w in w0]
    worst = 0.0
    for step, gs in enumerate(grads, 1):
        if step == 6:                                                # the schedule writes one rate into every group
            ref.lr = LR[rule] / 2
            for grp in opt.param_groups:
                grp["lr"] = LR[rule] / 2
        old = [w.copy() for w in wn]
        _set_grads(ws, gs, dev)
        opt.step()
        ref.step(wn, gs)
        _, _, r = _stats(opt, ws)
        for i, (w, new, was) in enumerate(zip(ws, wn, old)):
            err = _metric(w.detach().cpu().double().numpy(), new, was)
            worst = max(worst, err)
            assert err < BOUND[rule], f"{rule} {options} step {step} tensor {i}: {err:.2e}"
            assert abs(r[i] - ref.stats[i][2]) <= 1e-5 * ref.stats[i][2]
        assert r[1] == 1.0 and r[3] == 1.0                           # the exempt group: exactly one
    print(f"{rule} {options}: worst error {worst:.2e} (bound {BOUND[rule]:.2e})")
    assert opt.iterations == 9


# ------------------------------------------------------------------------------------------------ 2. the stats
def _lars_u2_bound(ws_np, gs, l2x2, wd):
    """u = fma(wd, w, g'), g' = fma(l2x2, w, g): |dg'| <= 2^-24 (|g| + |l2x2 w|), |du| <= 2^-24 |u| + |dg'| <= 2^-23 A with
    A = |g| + |l2x2 w| + |wd w| >= |u|, so |d(u^2)| <= 2 |u| |du| + du^2 <= 2^-22 A^2 (1 + 2^-22) per element."""
    return [None if gr is None else 2.0 ** -22 * 1.001 * np.sum((np.abs(gr) + np.abs(l2x2.get(i, 0.0) * w) + np.abs(wd[i] * w)) ** 2)
            for i, (w, gr) in enumerate(zip(ws_np, gs))]


@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_stats_are_the_norms_of_what_is_applied(dev, rule):
    """W2 is an exact sum of exact squares up to the f64 additions; U2 within the fp32 roundings of u; r the f64 quotient rounded
    to fp32 once.  All against the device's own weights and slots before the step, with the kernel's fp32 coefficients.
    lamb (no l2, no clip: g' = g exactly), per element with e = 2^-24:  m' = fma(1-b1, g, b1 m) is off by <= 2 e M,
    M = |b1 m| + (1-b1)|g|;  N = m' c1 by <= 3 e c1 M;  v' >= 0 term by term, off by <= 2 e v' (1 + e), so D = sqrt(v' c2) + eps by
    <= 3.5 e D;  q = N / D by <= 7.5 e Q, Q = c1 M / D >= |q|;  u = fma(wd, w, q) by <= e (|wd w| + Q) + 7.5 e Q <= 8.5 e A,
    A = |wd w| + Q >= |u|;  so |d(u^2)| <= 17 e A^2 (1 + 9 e)."""
    w0, grads = _inputs(6, steps=4)
    ws, opt, ref = _pair(dev, w0, rule, True, {}, l2=L2 if rule == "lars" else {})
    eta = {i: float(np.float32(e)) for (idx, _, _), e in zip(GROUPS, ETA[rule]) for i in idx}
    wd = {i: float(np.float32(d)) for (idx, _, d) in GROUPS for i in idx}
    b1, b2, eps = (float(np.float32(x)) for x in (0.9, 0.999, 1e-7))
    for t, gs in enumerate(grads, 1):
        held = [w.detach().cpu().double().numpy() for w in ws]
        _set_grads(ws, gs, dev)
        if rule == "lars":
            want = [None if gr is None else np.sum((wd[i] * w + (gr + ref.l2x2.get(i, 0.0) * w)) ** 2) for i, (w, gr) in enumerate(zip(held, gs))]
            bound = _lars_u2_bound(held, gs, ref.l2x2, wd)
        else:
            c1, c2 = float(np.float32(1.0 / (1.0 - b1 ** t))), float(np.float32(1.0 / (1.0 - b2 ** t)))
            want, bound = [], []
            for i, (w, gr) in enumerate(zip(held, gs)):
                if gr is None:
                    want.append(None), bound.append(None)
                    continue
                m, v = (opt._slots(ws[i])[j].cpu().double().numpy() for j in (0, 1))
                m1, v1 = (1.0 - b1) * gr + b1 * m, (1.0 - b2) * gr * gr + b2 * v
                d = np.sqrt(v1 * c2) + eps
                want.append(np.sum((wd[i] * w + m1 * c1 / d) ** 2))
                bound.append(17 * EPS24 * 1.001 * np.sum((np.abs(wd[i] * w) + c1 * (np.abs(b1 * m) + (1.0 - b1) * np.abs(gr)) / d) ** 2))
        opt.step()
        w2, u2, r = _stats(opt, ws)
        for i, w in enumerate(held):
            if gs[i] is None:
                assert (w2[i], u2[i], r[i]) == (0.0, 0.0, 1.0)
                continue
            exact = float(np.sum(w * w))
            print(f"{rule} step {t} tensor {i}: W2 rel {abs(w2[i] - exact) / exact:.1e}  U2 error / bound "
                  f"{abs(u2[i] - want[i]) / bound[i]:.3f}  r {r[i]:.4g}")
            assert abs(w2[i] - exact) <= 1e-12 * exact
            assert abs(u2[i] - want[i]) <= bound[i] + 1e-12 * want[i]
            formula = eta[i] * np.sqrt(w2[i]) / np.sqrt(u2[i]) if eta[i] > 0 else 1.0
            assert abs(r[i] - formula) <= (EPS24 + 1e-12) * formula
    assert opt.trust_ratios.dtype == torch.float32 and opt.trust_ratios.data_ptr() == opt._stats[0].data_ptr() + 16     # a static address


# ------------------------------------------------------------------------------------------------ 3. where the kernels can go wrong
@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_more_chunks_than_the_norm_grid_and_a_tail(dev, rule):
    """513 whole chunks and 77 elements: the norm kernel's 512 workgroups take a second chunk, the last workgroup's wave adds
    514 partials (nine per lane and a rest); a 300-element neighbour on either side keeps its own sums."""
    from embeddingnet_amd import _lib
    from embeddingnet_amd.optimizers import KerasOptimizer
    n = 513 * _lib.lib().embnet_optimizer_chunk_elems() + 77
    rs = np.random.RandomState(21)
    w0 = [f32(rs.randn(300)), f32(rs.randn(n)), f32(rs.randn(300))]
    ws = [torch.nn.Parameter(g(w, dev)) for w in w0]
    eta = ETA[rule][0]
    opt = KerasOptimizer([dict(params=ws, weight_decay=1e-2, trust_coefficient=eta)], rule, LR[rule])
    ref = R.RefLayerwise(rule, LR[rule], [dict(tensors=[0, 1, 2], weight_decay=1e-2, trust_coefficient=eta)])
    wn = [w.copy() for w in w0]
    for step in range(2):
        gs = [f32(rs.randn(*w.shape) * 0.1) for w in w0]
        old = [w.copy() for w in wn]
        exact = [float(np.sum(w.detach().cpu().double().numpy() ** 2)) for w in ws]
        _set_grads(ws, gs, dev)
        opt.step()
        ref.step(wn, gs)
        w2, u2, r = _stats(opt, ws)
        for i in range(3):
            assert abs(w2[i] - exact[i]) <= 1e-12 * exact[i]
            assert abs(u2[i] - ref.stats[i][1]) <= 1e-5 * ref.stats[i][1] and abs(r[i] - ref.stats[i][2]) <= 1e-5 * ref.stats[i][2]
            err = _metric(ws[i].detach().cpu().double().numpy(), wn[i], old[i])
            assert err < BOUND[rule], (step, i, err)
    assert opt._chunks.shape[0] == 514 + 2


@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_an_unaligned_parameter_takes_the_scalar_path_to_the_same_bits(dev, rule):
    """A parameter one float into a larger buffer is not 16-byte aligned: element by element in the norms and in the update, to
    the bits of the aligned one — weights, slots and stats."""
    from embeddingnet_amd.optimizers import KerasOptimizer
    rs = np.random.RandomState(12)
    n = 2 * 4096 + 13
    w0, other = f32(rs.randn(n)), f32(rs.randn(300))
    runs = []
    for shifted in (False, True):
        buf = torch.zeros(n + 8, device=dev)
        w = torch.nn.Parameter(buf[1:n + 1] if shifted else buf[4:n + 4])
        assert (w.data_ptr() % 16 != 0) == shifted and w.is_contiguous()
        with torch.no_grad():
            w.copy_(g(w0, dev))
        v = torch.nn.Parameter(g(other, dev))
        opt = KerasOptimizer([dict(params=[w], weight_decay=1e-2, trust_coefficient=ETA[rule][0]), dict(params=[v], lr_mult=4.0)],
                             rule, LR[rule], global_clipnorm=1.0, **(dict(nesterov=True) if rule == "lars" else {}))
        opt.set_l2([(w, 1e-3)])
        rs2, stats = np.random.RandomState(13), []
        for _ in range(3):
            w.grad, v.grad = g(rs2.randn(n) * 0.1, dev), g(rs2.randn(300), dev)
            opt.step()
            stats.append(opt._stats[0].clone())
        runs.append(_state([w, v], opt) + stats)
    for a, b in zip(*runs):
        assert _same_bits(a, b)


@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_zero_tensors_and_missing_gradients(dev, rule):
    """A zero weight tensor and a zero gradient without decay have r = 1 (the first still moves, at the plain rate; the second
    stays where it is under lars without momentum); a tensor without a gradient keeps its weight, both slots and stats {0, 0, 1}."""
    from embeddingnet_amd.optimizers import KerasOptimizer
    rs = np.random.RandomState(31)
    shapes = [(5000,), (33,), (4096,), (9,)]
    w0 = [f32(rs.randn(*s)) for s in shapes]
    w0[0][...] = 0.0
    ws = [torch.nn.Parameter(g(w, dev)) for w in w0]
    kw = dict(momentum=0.0) if rule == "lars" else {}
    opt = KerasOptimizer([dict(params=ws, trust_coefficient=0.5)], rule, 1e-2, **kw)
    ref = R.RefLayerwise(rule, 1e-2, [dict(tensors=[0, 1, 2, 3], trust_coefficient=0.5)], **kw)
    wn = [w.copy() for w in w0]
    gs = [f32(rs.randn(*s)) for s in shapes]
    _set_grads(ws, gs, dev)
    opt.step()                                                       # every tensor has slots and a history now
    ref.step(wn, gs)
    assert _stats(opt, ws)[2][0] == 1.0 and float(ws[0].detach().abs().max()) > 0
    gs = [f32(rs.randn(*s)) for s in shapes]
    gs[2] = np.zeros_like(gs[2])
    gs[3] = None
    before = {i: [ws[i].detach().clone()] + [s.clone() for s in opt._slots(ws[i]) if s is not None] for i in (2, 3)}
    old = [w.copy() for w in wn]
    _set_grads(ws, gs, dev)
    opt.step()
    ref.step(wn, gs)
    w2, u2, r = _stats(opt, ws)
    assert (w2[3], u2[3], r[3]) == (0.0, 0.0, 1.0)
    for a, b in zip(before[3], [ws[3].detach()] + [s for s in opt._slots(ws[3]) if s is not None]):
        assert _same_bits(a, b)
    if rule == "lars":                                               # u = g = 0: no norm, no step (the velocity is now zero)
        assert u2[2] == 0.0 and r[2] == 1.0 and w2[2] > 0
        assert _same_bits(before[2][0], ws[2].detach()) and float(opt._slots(ws[2])[0].abs().max()) == 0.0
    for i in range(4):
        assert _metric(ws[i].detach().cpu().double().numpy(), wn[i], old[i]) < BOUND[rule]


@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_the_same_inputs_give_the_same_bits(dev, rule):
    w0, grads = _inputs(8, steps=7)
    runs = []
    for _ in range(2):
        ws, opt, _ = _pair(dev, w0, rule, True, dict(global_clipnorm=1.0))
        stats = []
        for gs in grads:
            _set_grads(ws, gs, dev)
            opt.step()
            stats.append(opt._stats[0].clone())
        runs.append(_state(ws, opt) + stats)
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ 4. state
@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_state_round_trips(dev, rule, tmp_path):
    from embeddingnet_amd.optimizers import load_optimizer_state, save_optimizer_state
    w0, grads = _inputs(15, steps=4)
    kw = dict(clipvalue=0.05)
    ws, opt, _ = _pair(dev, w0, rule, True, kw)
    for gs in grads[:3]:
        _set_grads(ws, gs, dev)
        opt.step()
    save_optimizer_state(str(tmp_path / "o.npz"), opt, {f"t{i}": w for i, w in enumerate(ws)})
    files = np.load(str(tmp_path / "o.npz")).files
    assert "t2::slot1" in files and ("t2::slot2" in files) == (rule == "lamb")
    sd = copy.deepcopy(opt.state_dict())                              # (state_dict() hands out the live slots)
    now = [w.detach().clone() for w in ws]
    _set_grads(ws, grads[3], dev)
    opt.step()
    want = _state(ws, opt)
    for how in ("file", "state_dict"):
        ws2, opt2, _ = _pair(dev, [w.cpu().double().numpy() for w in now], rule, True, kw)
        if how == "file":
            load_optimizer_state(str(tmp_path / "o.npz"), opt2, {f"t{i}": w for i, w in enumerate(ws2)})
        else:
            opt2.load_state_dict(sd)
        assert opt2.iterations == 3 and float(opt2.state[ws2[2]]["slot1"].abs().max()) > 0
        assert [grp["trust_coefficient"] for grp in opt2.param_groups] == ETA[rule]
        _set_grads(ws2, grads[3], dev)
        opt2.step()
        for a, b in zip(want, _state(ws2, opt2)):
            assert torch.equal(a, b), how


# ------------------------------------------------------------------------------------------------ 5. replay
N_CLASSES = 12


def _groups(base, rule, proxies=None):
    from embeddingnet_amd.utils import OptimizerSpec
    params = {"weight_decay": 1e-2, "global_clipnorm": 0.5}
    if proxies is not None:
        params.update(proxy_lr_mult=10.0, proxy_weight_decay=1e-3)
    return OptimizerSpec(rule, LR[rule], params).build([q for q in base.parameters() if q.requires_grad], proxies=proxies)


def _trainer(dev, rule, graph):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.proxies import ProxyHead
    from embeddingnet_amd.train_step import ProxyTrainer, TripletTrainer
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=5, device=dev)
    if rule == "lamb":
        head = ProxyHead(N_CLASSES, 64, seed=1).to(dev)
        opt = _groups(base, rule, [head.proxies])
        return base, head, opt, ProxyTrainer(base, head, opt, loss="proxy_anchor", seed=3, graph=graph)
    opt = _groups(base, rule)
    return base, None, opt, TripletTrainer(base, opt, 4, 4, negatives_selection_mode="supcon", seed=3, graph=graph)


def _batches(dev, steps):
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((N_CLASSES, 64, 64, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(N_CLASSES, generator=torch.Generator().manual_seed(i))[:4].to(dev)
        x = protos[cls].repeat_interleave(4, 0) + 0.15 * torch.randn((16, 64, 64, 3), device=dev, generator=gen)
        yield x.clamp(0, 1), cls.repeat_interleave(4).to(torch.int32)


@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_captured_step_replays_with_current_rates_and_ratios(dev, rule):
    """A captured ProxyTrainer step with 'lamb' (three groups) and a captured TripletTrainer(supcon) step with 'lars' (two)
    against eager steps from the same state: loss, weights, slots, grad_norm and the trust ratios equal bit for bit after every
    step, across a change of the rate and an eager step in between."""
    from embeddingnet_amd import _lib
    runs = []
    for graph in (False, True):
        base, head, opt, tr = _trainer(dev, rule, graph)
        assert opt.group_names == (["kernels", "other", "proxies"] if head is not None else ["kernels", "other"])
        seen = []
        for i, (x, y) in enumerate(_batches(dev, 14)):              # (the capture follows eight eager steps)
            if i == 10:
                for grp in opt.param_groups:
                    grp["lr"] = 0.4 * LR[rule]
            if graph and i == 12:
                _lib.trace_enable(True)                               # an eager step between replays
            loss = (tr.step(x, y) if head is not None else tr.step(x)).clone()
            _lib.trace_enable(False)
            slots = [s.reshape(-1) for q in opt._tensors for s in opt._slots(q) if s is not None]
            seen.append([loss, opt.grad_norm.clone(), opt.trust_ratios.clone(),
                         torch.cat([q.detach().reshape(-1) for q in opt._tensors]), torch.cat(slots)])
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
            assert tr._state.numel() == 12 + 4 * len(opt.param_groups)
        runs.append(seen)
    ratios = runs[0][-1][2].cpu().numpy()
    adapted = np.zeros(len(ratios), dtype=bool)
    adapted[opt.adapted] = True
    print(f"{rule}: trust ratios of the adapted tensors {ratios[adapted].min():.3g}..{ratios[adapted].max():.3g}")
    assert np.all(ratios[~adapted] == 1.0) and np.all(np.isfinite(ratios)) and np.all(ratios[adapted] > 0) and np.any(ratios[adapted] != 1.0)
    assert not torch.equal(runs[0][0][3], runs[0][-1][3])            # the weights moved
    for i, (a, b) in enumerate(zip(*runs)):
        for j, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), (i, ["loss", "grad_norm", "trust_ratios", "weights", "slots"][j])


# ------------------------------------------------------------------------------------------------ 6. CLI
def _cli(tmp_path, name, extra=()):
    cfg = open(os.path.join(ROOT, "configs", f"{name}.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert "optimizer_params" in cfg and "n_batches : 20" in cfg and "monitor : 'val_map@r'" in cfg
    cfg = cfg.replace("n_batches : 20", "n_batches : 6").replace("monitor : 'val_map@r'", "monitor : 'loss'")
    path = tmp_path / "cfg.yml"
    path.write_text(cfg)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(path), "--synthetic", "10", "--max_epochs", "2",
                           *extra], capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("name,slots", [("simple2_supcon_lars_synthetic", 1), ("simple2_proxy_anchor_lamb_synthetic", 2)])
def test_train_cli_logs_trust_ratios_and_resumes(tmp_path, name, slots):
    out = _cli(tmp_path, name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"Epoch \d+/\d+ - lr \S+ - loss (\S+)", out.stdout)]
    trust = [(float(a), float(b)) for a, b in re.findall(r" - trust ([0-9.e+-]+)\.\.([0-9.e+-]+)", out.stdout)]
    print("losses", losses, "trust", trust)
    assert len(losses) == 2 and all(np.isfinite(losses))
    assert len(trust) == 2 and all(0 < a <= b and np.isfinite(b) for a, b in trust)
    saved = sorted(os.listdir(tmp_path / name / "weights"))
    assert saved and saved == sorted(os.listdir(tmp_path / name / "optimizer"))
    with np.load(tmp_path / name / "optimizer" / saved[-1]) as state:         # (the resumed run writes the file again)
        assert str(state["__rule__"]) == name.split("_")[2 if slots == 1 else 3]
        assert sum(k.endswith("::slot1") for k in state.files) > 0
        assert (sum(k.endswith("::slot2") for k in state.files) > 0) == (slots == 2)
        iterations = int(state["__iterations__"])
    res = _cli(tmp_path, name, extra=("--resume_from", str(tmp_path / name / "weights" / saved[-1])))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    found = re.search(r"resumed optimizer state from \S+ \(iterations (\d+),", res.stdout)
    assert found and int(found.group(1)) == iterations > 0
    assert len(re.findall(r" - trust \S+\.\.\S+", res.stdout)) == 2
