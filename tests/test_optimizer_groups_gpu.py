"""GPU tests of the grouped optimizer — `embnet_optimizer_step_groups` and `embnet_optimizer_grad_norm` as KerasOptimizer launches
them — against tests/optimizer_ref.py (float64), and bit for bit against themselves, against `embnet_optimizer_step`, under graph
replay and through tools/train.py.

The shapes are test_step_parity_gpu.py's optimizer test's: a scalar tail, more than one chunk, a one-element tensor.  The metric of
the parity test is, per tensor and step, max|got - ref| / max(max|ref_new|, max|ref_old|) < 3e-6 (that test's tolerance; the old
value is in the denominator so that a one-element tensor passing through zero cannot fail by cancellation).  An fp32 NumPy
emulation of these rules on exactly these inputs stays at or below 5e-7 for every combination, so the reference's own fp32 form
has about 6x headroom; with a multiplier of 64 and momentum the emulation left the bound (1.3e-5), hence multipliers 4 and 0.25."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import optimizer_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(3, 3, 16, 8), (7,), (5000,), (1,), (4096 + 13,), (64, 64)]
GROUPS = [([0, 2], 1.0, 1e-2), ([1, 3], 4.0, 0.0), ([4, 5], 0.25, 2e-2)]          # tensors, lr_mult, weight_decay
L2 = {0: 2e-4, 5: 1e-3}
RULES = {"sgd": ("sgd", {}), "momentum": ("sgd", dict(momentum=0.9)), "nesterov": ("sgd", dict(momentum=0.9, nesterov=True)),
         "rms_prop": ("rms_prop", {}), "adam": ("adam", {}), "radam": ("radam", {})}
OPTIONS = {"none": (False, {}), "decay": (True, {}), "clipvalue": (False, dict(clipvalue=0.05)),
           "clipnorm": (False, dict(global_clipnorm=1.0)), "decay+clipnorm": (True, dict(global_clipnorm=1.0)),
           "decay+clipvalue": (True, dict(clipvalue=0.05))}


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


def _pair(dev, w0, rule, decay, kw, l2=L2, lr=1e-2):
    """The device optimizer over three groups and its float64 reference."""
    from embeddingnet_amd.optimizers import KerasOptimizer
    ws = [torch.nn.Parameter(g(w, dev)) for w in w0]
    opt = KerasOptimizer([dict(params=[ws[i] for i in idx], lr_mult=m, weight_decay=wd if decay else 0.0) for idx, m, wd in GROUPS],
                         rule, lr, **kw)
    opt.set_l2([(ws[i], lam) for i, lam in l2.items()])
    ref = R.RefOptimizer(rule, lr, [dict(tensors=idx, lr_mult=m, weight_decay=wd if decay else 0.0) for idx, m, wd in GROUPS],
                         l2=l2, **kw)
    return ws, opt, ref


def _n2_bound(gs, l2x2, wn):
    """g' = fma(l2x2, w, g) is rounded to fp32 once, |g'_fp32 - g'| <= 2^-24 (|g| + |l2x2 w|), and the square of it twice over:
    |dN2| <= 2^-22 sum (|g| + |l2x2 w|)^2 (plus the f64 additions' 1e-12)."""
    return 2.0 ** -22 * sum(np.sum((np.abs(gr) + np.abs(l2x2.get(i, 0.0) * wn[i])) ** 2) for i, gr in enumerate(gs) if gr is not None)


def _set_grads(ws, gs, dev):
    for w, gr in zip(ws, gs):
        w.grad = None if gr is None else g(gr, dev)


def _state(ws, opt):
    out = [w.detach().clone() for w in ws]
    for w in ws:
        for k in ("slot1", "slot2"):
            if k in opt.state[w]:
                out.append(opt.state[w][k].clone())
    return out


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("options", list(OPTIONS))
@pytest.mark.parametrize("rule", list(RULES))
def test_grouped_steps_vs_reference(dev, rule, options):
    name, kw = RULES[rule]
    decay, okw = OPTIONS[options]
    w0, grads = _inputs(5)
    ws, opt, ref = _pair(dev, w0, name, decay, {**kw, **okw})
    assert opt.grouped
    wn = [w.copy() for w in w0]
    worst = 0.0
    for step, gs in enumerate(grads, 1):
        if step == 6:                                                # the schedule writes one rate into every group
            ref.lr = 5e-3
            for grp in opt.param_groups:
                grp["lr"] = 5e-3
        old = [w.copy() for w in wn]
        _set_grads(ws, gs, dev)
        opt.step()
        ref.step(wn, gs)
        for i, (w, new, was) in enumerate(zip(ws, wn, old)):
            got = w.detach().cpu().double().numpy()
            err = np.abs(got - new).max() / max(np.abs(new).max(), np.abs(was).max())
            worst = max(worst, err)
            assert err < 3e-6, f"{rule} {options} step {step} tensor {i}: {err:.2e}"
    print(f"{rule} {options}: worst error {worst:.2e}")
    assert opt.iterations == 9


# ------------------------------------------------------------------------------------------------ 2. the norm
def test_grad_norm_without_l2_is_an_exact_sum(dev):
    """Squares of fp32 values are exact in f64; what is left is the rounding of the f64 additions."""
    w0, grads = _inputs(6, steps=4)
    ws, opt, ref = _pair(dev, w0, "adam", True, dict(global_clipnorm=1.0), l2={})
    wn = [w.copy() for w in w0]
    for gs in grads:
        _set_grads(ws, gs, dev)
        opt.step()
        ref.step(wn, gs)
        n2, norm = float(opt._norm[0][0].item()), float(opt.grad_norm.item())
        print("N2", n2, "reference", ref.n2, "relative error", abs(n2 - ref.n2) / ref.n2)
        assert abs(n2 - ref.n2) <= 1e-12 * ref.n2
        assert abs(norm * norm - ref.n2) <= 1e-12 * ref.n2
        scale = float(opt._norm[0][2:3].view(torch.float32)[0].item())
        assert abs(scale - 1.0 / max(np.sqrt(n2), 1.0)) <= (2.0 ** -24 + 1e-12) * scale      # the f64 quotient, rounded to fp32 once
    assert opt.grad_norm.dtype == torch.float64 and opt.grad_norm.data_ptr() == opt._norm[0].data_ptr() + 8      # a static address


def test_grad_norm_with_l2_within_one_rounding_per_element(dev):
    """|dN2| <= 2^-22 sum (|g| + |l2x2 w|)^2 (_n2_bound)."""
    w0, grads = _inputs(7, steps=3)
    ws, opt, ref = _pair(dev, w0, "sgd", False, dict(global_clipnorm=1.0))
    for gs in grads:
        wn = [w.detach().cpu().double().numpy() for w in ws]         # the device's own weights: the bound is about one step
        bound = _n2_bound(gs, ref.l2x2, wn)
        _set_grads(ws, gs, dev)
        opt.step()
        ref.step(wn, gs)
        n2 = float(opt._norm[0][0].item())
        print("N2", n2, "reference", ref.n2, "error / bound", abs(n2 - ref.n2) / bound)
        assert abs(n2 - ref.n2) <= bound


# ------------------------------------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("rule", ["nesterov", "radam"])
def test_the_same_inputs_give_the_same_bits(dev, rule):
    name, kw = RULES[rule]
    w0, grads = _inputs(8, steps=7)
    runs = []
    for _ in range(2):
        ws, opt, _ = _pair(dev, w0, name, True, dict(global_clipnorm=1.0, **kw))
        norms = []
        for gs in grads:
            _set_grads(ws, gs, dev)
            opt.step()
            norms.append(opt._norm[0].clone())
        runs.append(_state(ws, opt) + norms)
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _raw_problem(dev, seed, n_slots, misalign=False):
    """Tensors, a descriptor table and the chunk list built by hand: what a caller of the C ABI passes."""
    from embeddingnet_amd import _lib
    rs = np.random.RandomState(seed)
    ce = _lib.lib().embnet_optimizer_chunk_elems()
    keep, rows, chunks = [], [], []
    for i, s in enumerate(SHAPES):
        n = int(np.prod(s))
        t = [g(rs.randn(n), dev), g(rs.randn(n) * 0.1, dev)] + [g(np.abs(rs.randn(n)) * 0.01, dev) for _ in range(n_slots)]
        keep.append(t)
        l2x2 = int(np.float32(2.0 * L2.get(i, 0.0)).view(np.uint32))
        rows.append([t[0].data_ptr(), t[1].data_ptr()] + [x.data_ptr() for x in t[2:]] + [0] * (2 - n_slots) + [n, l2x2])
        chunks += [(i, c) for c in range(-(-n // ce))]
    table = torch.tensor(np.asarray(rows, dtype=np.uint64).view(np.int64), device=dev)
    return keep, table, torch.tensor(chunks, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("code", [0, 1, 2, 3, 4])
def test_one_group_without_options_is_the_old_entry_point(dev, code):
    """Through ctypes: embnet_optimizer_step_groups with one group, no decay and no clip == embnet_optimizer_step, bit for bit."""
    from embeddingnet_amd import _lib
    from embeddingnet_amd._lib import check
    lib = _lib.lib()
    n_slots = [0, 1, 2, 2, 2][code]
    lr, b1, b2, eps, c1, c2 = 1e-2, 0.9, 0.999, 1e-7, 0.0123, 1.7
    out = []
    for grouped in (False, True):
        keep, table, chunks = _raw_problem(dev, 11, n_slots)
        if grouped:
            rows = np.asarray([[lr, c1, 0.0, 0.0]], dtype=np.float32)
            check(lib.embnet_optimizer_step_groups(code, table.data_ptr(), len(keep), chunks.data_ptr(), chunks.shape[0],
                                                   rows.ctypes.data, 1, b1, b2, eps, c2, 0.0, 0, 0.0, None, None, None, _lib.stream()))
        else:
            check(lib.embnet_optimizer_step(code, table.data_ptr(), len(keep), chunks.data_ptr(), chunks.shape[0], lr, b1, b2, eps,
                                            c1, c2, None, _lib.stream()))
        torch.cuda.synchronize()
        out.append(keep)
    for ta, tb in zip(*out):
        for a, b in zip(ta, tb):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    start, _, _ = _raw_problem(dev, 11, n_slots)
    assert all(not torch.equal(t0[0], t1[0]) for t0, t1 in zip(start, out[1]))      # (the step did run, on every tensor)


@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_three_groups_are_three_single_group_optimizers(dev, rule):
    """lr_mult 1, 4, 0.25 in one launch == three plain optimizers at those rates (which go through embnet_optimizer_step)."""
    from embeddingnet_amd.optimizers import KerasOptimizer
    w0, grads = _inputs(9, steps=4)
    ws, opt, _ = _pair(dev, w0, rule, False, {})
    ws1 = [torch.nn.Parameter(g(w, dev)) for w in w0]
    singles = [KerasOptimizer([ws1[i] for i in idx], rule, 1e-2 * m) for idx, m, _ in GROUPS]
    for o in singles:
        assert not o.grouped
        o.set_l2([(ws1[i], lam) for i, lam in L2.items() if any(ws1[i] is q for q in o._tensors)])
    for step, gs in enumerate(grads, 1):
        if step == 3:
            for grp in opt.param_groups:
                grp["lr"] = 5e-3
            for o, (_, m, _) in zip(singles, GROUPS):
                o.param_groups[0]["lr"] = 5e-3 * m
        _set_grads(ws, gs, dev)
        _set_grads(ws1, gs, dev)
        opt.step()
        for o in singles:
            if any(q.grad is not None for q in o._tensors):
                o.step()
        for i, (a, b) in enumerate(zip(ws, ws1)):
            assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), (step, i)
    for a, b in zip(ws, ws1):
        for k in opt.state[a]:
            o = next(o for o in singles if any(b is q for q in o._tensors))
            assert torch.equal(opt.state[a][k], o.state[b][k])


@pytest.mark.parametrize("rule", ["adam", "nesterov"])
def test_an_unaligned_parameter_takes_the_scalar_path_to_the_same_bits(dev, rule):
    """A parameter one float into a larger buffer is not 16-byte aligned: element by element, in the update and in the norm.
    With decay, l2 and the norm clip every rounding is pinned and the same on both paths (include/embnet.h).  (A tensor that no
    option touches goes through embnet_optimizer_step's own code instead, whose two paths round the slot updates of rms_prop / adam /
    radam differently: that is the old entry point's behaviour, kept bit for bit.)"""
    name, kw = RULES[rule]
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
        opt = KerasOptimizer([dict(params=[w], weight_decay=1e-2), dict(params=[v], lr_mult=4.0)], name, 1e-2, global_clipnorm=1.0, **kw)
        opt.set_l2([(w, 1e-3)])
        rs2, norms = np.random.RandomState(13), []
        for _ in range(3):
            w.grad, v.grad = g(rs2.randn(n) * 0.1, dev), g(rs2.randn(300), dev)
            opt.step()
            norms.append(opt._norm[0].clone())
        runs.append(_state([w, v], opt) + norms)
    for a, b in zip(*runs):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 4. no gradient
def test_a_tensor_without_a_gradient_is_left_alone(dev):
    w0, _ = _inputs(14, steps=1)
    rs = np.random.RandomState(14)
    grads = [[f32(rs.randn(*s)) for s in SHAPES]]                    # every tensor weighs in the norm by its size
    ws, opt, ref = _pair(dev, w0, "adam", True, dict(global_clipnorm=1.0))
    wn = [w.copy() for w in w0]
    _set_grads(ws, grads[0], dev)
    opt.step()
    ref.step(wn, grads[0])
    gs = list(grads[0])
    gs[0] = gs[3] = None                                             # tensor 0: decayed group, l2; tensor 3: one element
    before = {i: [ws[i].detach().clone()] + [opt.state[ws[i]][k].clone() for k in ("slot1", "slot2")] for i in (0, 3)}
    moved = ws[2].detach().clone()
    _set_grads(ws, gs, dev)
    held = [w.detach().cpu().double().numpy() for w in ws]           # the device's own weights: the bound is about this step
    bound = _n2_bound(gs, ref.l2x2, held)
    opt.step()
    ref.step(held, gs)
    for i, (w, s1, s2) in before.items():
        assert torch.equal(ws[i].detach(), w) and torch.equal(opt.state[ws[i]]["slot1"], s1) and torch.equal(opt.state[ws[i]]["slot2"], s2)
    assert not torch.equal(ws[2].detach(), moved)
    n2 = float(opt._norm[0][0].item())
    with_them = ref.n2 + sum(np.sum((grads[0][i] + ref.l2x2.get(i, 0.0) * wn[i]) ** 2) for i in (0, 3))
    assert abs(n2 - ref.n2) <= bound + 1e-12 * ref.n2 and with_them > 1.05 * ref.n2       # they are absent from the norm


# ------------------------------------------------------------------------------------------------ 5. state
def test_state_round_trips_carry_the_velocity(dev, tmp_path):
    from embeddingnet_amd.optimizers import load_optimizer_state, save_optimizer_state
    name, kw = RULES["nesterov"]
    w0, grads = _inputs(15, steps=4)
    ws, opt, _ = _pair(dev, w0, name, True, dict(clipvalue=0.05, **kw))
    for gs in grads[:3]:
        _set_grads(ws, gs, dev)
        opt.step()
    names = {f"t{i}": w for i, w in enumerate(ws)}
    save_optimizer_state(str(tmp_path / "o.npz"), opt, names)
    assert "t2::slot1" in np.load(str(tmp_path / "o.npz")).files
    sd = copy.deepcopy(opt.state_dict())                              # (state_dict() hands out the live slots)
    now = [w.detach().clone() for w in ws]
    _set_grads(ws, grads[3], dev)
    opt.step()
    want = _state(ws, opt)
    for how in ("file", "state_dict"):
        ws2, opt2, _ = _pair(dev, [w.cpu().double().numpy() for w in now], name, True, dict(clipvalue=0.05, **kw))
        if how == "file":
            load_optimizer_state(str(tmp_path / "o.npz"), opt2, {f"t{i}": w for i, w in enumerate(ws2)})
        else:
            opt2.load_state_dict(sd)
        assert opt2.iterations == 3 and float(opt2.state[ws2[2]]["slot1"].abs().max()) > 0
        _set_grads(ws2, grads[3], dev)
        opt2.step()
        for a, b in zip(want, _state(ws2, opt2)):
            assert torch.equal(a, b), how


# ------------------------------------------------------------------------------------------------ 6. replay
N_CLASSES = 12


def _proxy_trainer(dev, graph):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.proxies import ProxyHead
    from embeddingnet_amd.train_step import ProxyTrainer
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=5, device=dev)
    head = ProxyHead(N_CLASSES, 64, seed=1).to(dev)
    ps = [q for q in base.parameters() if q.requires_grad]
    opt = KerasOptimizer([dict(params=[q for q in ps if q.dim() >= 2], weight_decay=1e-2), dict(params=[q for q in ps if q.dim() < 2]),
                          dict(params=[head.proxies], lr_mult=10.0, weight_decay=1e-3)], "adam", 1e-3, global_clipnorm=0.5)
    return base, head, opt, ProxyTrainer(base, head, opt, loss="proxy_anchor", seed=3, graph=graph)


def _batches(dev, steps):
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((N_CLASSES, 64, 64, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(N_CLASSES, generator=torch.Generator().manual_seed(i))[:4].to(dev)
        x = protos[cls].repeat_interleave(4, 0) + 0.15 * torch.randn((16, 64, 64, 3), device=dev, generator=gen)
        yield x.clamp(0, 1), cls.repeat_interleave(4).to(torch.int32)


def test_captured_step_replays_with_every_groups_coefficients(dev):
    """A captured ProxyTrainer step (three groups, AdamW, global_clipnorm) against eager steps from the same state: weights,
    proxies, slots and grad_norm equal bit for bit after every step, across a change of the rate and an eager step in between."""
    from embeddingnet_amd import _lib
    runs = []
    for graph in (False, True):
        base, head, opt, tr = _proxy_trainer(dev, graph)
        seen = []
        for i, (x, y) in enumerate(_batches(dev, 14)):              # (the capture follows eight eager steps)
            if i == 10:
                for grp in opt.param_groups:
                    grp["lr"] = 4e-4
            if graph and i == 12:
                _lib.trace_enable(True)                               # an eager step between replays
            loss = tr.step(x, y).clone()
            _lib.trace_enable(False)
            seen.append([loss, opt.grad_norm.clone(), head.proxies.detach().clone(),
                         torch.cat([q.detach().reshape(-1) for q in base.parameters()]),
                         torch.cat([opt.state[q][k].reshape(-1) for q in opt._tensors for k in ("slot1", "slot2")])])
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
            assert tr._state.numel() == 12 + 4 * 3
        runs.append(seen)
    norms = [float(s[1].item()) for s in runs[0]]
    print("grad norms", norms)
    assert all(np.isfinite(norms)) and max(norms) > 0.5               # the clip was active
    for i, (a, b) in enumerate(zip(*runs)):
        for j, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), (i, ["loss", "grad_norm", "proxies", "weights", "slots"][j])


# ------------------------------------------------------------------------------------------------ 6b. the launches beside the update
def test_step_leaves_planes_and_ranges_current_through_cached_plans(dev, monkeypatch):
    """After KerasOptimizer.step() on BatchNorm -> 3x3 conv 16 -> 32 (patch kernel: kernel planes) -> BatchNorm -> 1x1 conv 32 -> 16
    (gather kernel on three products: a kernel range), 8x8 images: the optimizer's chunk list is the hand-written one, both side
    entries are current, asking again launches nothing, the next step makes one call per kind from the plans cached on the
    optimizer, and the regularisers' value is their float64 sum (2e-6 relative, test_round3_gpu.py's tolerance)."""
    from embeddingnet_amd import _lib
    from embeddingnet_amd import layers as L
    from embeddingnet_amd.optimizers import KerasOptimizer
    lib = _lib.lib()
    torch.manual_seed(3)
    net = torch.nn.Sequential()
    net.bn0, net.c3 = L.BatchNormalization(16), L.Conv2D(16, 32, 3, padding="same", use_bias=False, l2=2e-4)
    net.bn1, net.c1 = L.BatchNormalization(32), L.Conv2D(32, 16, 1, l2=1e-3)
    net.c1.f16 = True
    net.to(dev).train()
    opt = KerasOptimizer(net.parameters(), "sgd", 0.05)
    x = torch.randn(4, 8, 8, 16, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        net.c1(net.bn1(net.c3(net.bn0(x, planes_for=net.c3)))).square().sum().backward()
        opt.step()

    step()
    ce = lib.embnet_optimizer_chunk_elems()
    assert net.c3.kernel.numel() > ce                                            # more than one chunk
    assert opt._chunks.dtype == torch.int32 and opt._chunks.device == x.device
    assert opt._chunks.cpu().tolist() == [[i, c] for i, p in enumerate(opt._tensors) for c in range(-(-p.numel() // ce))]
    planes, rng = net.c3.kernel._embnet_wplanes, net.c1.kernel._embnet_wrange

    def current():
        return all(e["epoch"] == L.WEIGHT_EPOCH[0] and e["version"] == w._version
                   for e, w in ((planes, net.c3.kernel), (rng, net.c1.kernel)))

    assert current()
    assert rng["slot"].cpu().view(torch.int32).item() == net.c1.kernel.detach().abs().max().cpu().view(torch.int32).item()
    calls = {"embnet_conv_weight_planes": 0, "embnet_range_multi": 0}

    def counted(name, fn):
        def call(*args):
            calls[name] += 1
            return fn(*args)
        return call

    for name in calls:
        monkeypatch.setattr(lib, name, counted(name, getattr(lib, name)))
    L.refresh_tensors(opt._tensors, opt)
    L.refresh_weight_planes(net)
    assert calls == {"embnet_conv_weight_planes": 0, "embnet_range_multi": 0}
    cached = opt._wplanes_plan, opt._wrange_plan
    step()
    assert calls == {"embnet_conv_weight_planes": 1, "embnet_range_multi": 1} and current()
    assert opt._wplanes_plan is cached[0] and opt._wrange_plan is cached[1]
    assert rng["slot"].cpu().view(torch.int32).item() == net.c1.kernel.detach().abs().max().cpu().view(torch.int32).item()
    want = sum(lam * float((w.detach().double() ** 2).sum()) for w, lam in ((net.c3.kernel, 2e-4), (net.c1.kernel, 1e-3)))
    val = L.regularization_loss(net, with_grad=False)
    assert abs(val.item() - want) <= 2e-6 * want


# ------------------------------------------------------------------------------------------------ 7. CLI
def _cli(tmp_path, name, extra=()):
    cfg = open(os.path.join(ROOT, "configs", f"{name}.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert "optimizer_params" in cfg and "n_batches : 20" in cfg and "monitor : 'val_map@r'" in cfg
    cfg = cfg.replace("n_batches : 20", "n_batches : 6").replace("monitor : 'val_map@r'", "monitor : 'loss'")
    path = tmp_path / "cfg.yml"
    path.write_text(cfg)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(path), "--synthetic", "10", "--max_epochs", "2",
                           *extra], capture_output=True, text=True, timeout=600)


def test_train_cli_adamw_recipe(tmp_path):
    out = _cli(tmp_path, "simple2_proxy_anchor_adamw_synthetic")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"Epoch \d+/\d+ - lr \S+ - loss (\S+)", out.stdout)]
    print("losses", losses)
    assert len(losses) == 2 and all(np.isfinite(losses)) and "grad_norm" not in out.stdout


def test_train_cli_clipnorm_logs_the_norm_and_resumes(tmp_path):
    name = "simple2_proxy_anchor_clipnorm_synthetic"
    out = _cli(tmp_path, name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    norms = [float(v) for v in re.findall(r" - grad_norm (\S+)", out.stdout)]
    print("grad_norm per epoch", norms)
    assert len(norms) == 2 and all(np.isfinite(norms)) and min(norms) > 0
    saved = sorted(os.listdir(tmp_path / name / "weights"))
    assert saved and saved == sorted(os.listdir(tmp_path / name / "optimizer"))
    with np.load(tmp_path / name / "optimizer" / saved[-1]) as state:         # (the resumed run writes the file again)
        assert "proxy_head/proxies::slot1" in state.files and "proxy_head/proxies::slot2" in state.files
        iterations = int(state["__iterations__"])
    res = _cli(tmp_path, name, extra=("--resume_from", str(tmp_path / name / "weights" / saved[-1])))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    found = re.search(r"resumed optimizer state from \S+ \(iterations (\d+),", res.stdout)
    assert found and int(found.group(1)) == iterations > 0
    assert len(re.findall(r" - grad_norm (\S+)", res.stdout)) == 2
