"""GPU tests of weight averaging — `embnet_weight_average_update` / `embnet_weight_average_swap` through the C ABI, bit for bit
against tests/weight_average_ref.py (NumPy float32 restates the contract's three roundings exactly, so there is no tolerance), the
float64 trajectory inside the bound derived there, WeightAverager in the trainers (eager, captured, replayed), `applied()` on a model
whose convs read cached planes, and tools/train.py.

Shapes: test_optimizer_groups_gpu.py's — a scalar tail, more than one chunk, a one-element tensor — plus a view that is 4-byte but
not 16-byte aligned beside an aligned tensor of the same values."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import weight_average_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(3, 3, 16, 8), (7,), (5000,), (1,), (4096 + 13,), (64, 64)]
N_VIEW = 4096 * 2 + 5
SPECIAL = np.array([0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, np.nan, 1.5e-38], dtype=np.float32)     # +-0, subnormals, +-inf, NaN
PAYLOADS = np.array([0x7FC01234, 0xFFC00001, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32)                 # NaNs: quiet, signalling


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1)


def _values(rs, n, specials):
    v = (rs.randn(n) * 10.0 ** rs.randint(-3, 2, size=n)).astype(np.float32)
    if specials and n >= 64:                         # every pair of special values meets once: w by rows, avg by columns
        v[:64] = np.repeat(SPECIAL, 8) if specials == "w" else np.tile(SPECIAL, 8)
    return v


class Problem:
    """Tensors, a descriptor table and the chunk list built by hand: what a caller of the C ABI passes.  The last two tensors hold
    the same values: a view one float into a larger buffer (not 16-byte aligned) and an aligned one."""

    def __init__(self, dev, seed, specials=True):
        from embeddingnet_amd import _lib
        self.lib, self.dev = _lib.lib(), dev
        rs = np.random.RandomState(seed)
        sizes = [int(np.prod(s)) for s in SHAPES] + [N_VIEW, N_VIEW]
        self.w_host = [_values(rs, n, "w" if specials else None) for n in sizes[:-1]]
        self.a_host = [_values(rs, n, "avg" if specials else None) for n in sizes[:-1]]
        self.w_host.append(self.w_host[-1].copy())
        self.a_host.append(self.a_host[-1].copy())
        self._bufs = [torch.zeros(N_VIEW + 8, device=dev) for _ in range(2)]
        self.w = [torch.empty(n, device=dev) for n in sizes[:-2]] + [self._bufs[0][1:N_VIEW + 1], torch.empty(N_VIEW, device=dev)]
        self.a = [torch.empty(n, device=dev) for n in sizes[:-2]] + [self._bufs[1][1:N_VIEW + 1], torch.empty(N_VIEW, device=dev)]
        assert self.w[-2].data_ptr() % 16 == 4 and self.a[-2].data_ptr() % 16 == 4 and self.w[-1].data_ptr() % 16 == 0
        self.put(self.w, self.w_host)
        self.put(self.a, self.a_host)
        ce = self.lib.embnet_optimizer_chunk_elems()
        rows = [(w.data_ptr(), a.data_ptr(), w.numel(), 0) for w, a in zip(self.w, self.a)]
        self.table = torch.tensor(np.asarray(rows, dtype=np.uint64).view(np.int64), device=dev)
        self.chunks = torch.tensor([(i, c) for i, n in enumerate(sizes) for c in range(-(-n // ce))], dtype=torch.int32, device=dev)
        assert self.table.shape == (len(sizes), 4) and self.chunks.shape[0] > len(sizes)

    def put(self, tensors, host):
        for t, h in zip(tensors, host):
            t.copy_(torch.from_numpy(h.view(np.int32)).to(self.dev).view(torch.float32))          # the bits, NaN payloads included

    def update(self, c, c_dev=None):
        from embeddingnet_amd import _lib
        _lib.check(self.lib.embnet_weight_average_update(self.table.data_ptr(), len(self.w), self.chunks.data_ptr(), self.chunks.shape[0],
                                                         c, None if c_dev is None else c_dev.data_ptr(), _lib.stream()))

    def swap(self):
        from embeddingnet_amd import _lib
        _lib.check(self.lib.embnet_weight_average_swap(self.table.data_ptr(), len(self.w), self.chunks.data_ptr(), self.chunks.shape[0],
                                                       _lib.stream()))


def _same_bits_or_both_nan(got, want, what):
    got_f, want_f = got.view(np.float32), want.view(np.float32)
    nan = np.isnan(want_f)
    assert np.array_equal(np.isnan(got_f), nan), what
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first {bad[:4]}: {got_f[bad[:4]]} != {want_f[bad[:4]]}"


# ------------------------------------------------------------------------------------------------ 1. bits of update
@pytest.mark.parametrize("c", [1e-4, 1e-3, 0.1, 0.5])
def test_update_bits_equal_the_float32_reference(dev, c):
    p = Problem(dev, 21)
    c = float(np.float32(c))
    ref = [a.copy() for a in p.a_host]
    rs = np.random.RandomState(22)
    for step in range(5):
        if step:                                     # the weights move; the special values stay where they are
            for w in p.w_host[:-1]:
                lo = 64 if w.size >= 64 else 0
                w[lo:] = (w[lo:] + 0.1 * rs.randn(w.size - lo) * np.abs(w[lo:])).astype(np.float32)
            p.w_host[-1] = p.w_host[-2].copy()
            p.put(p.w, p.w_host)
        p.update(c)
        ref = [R.update_f32(a, w, c) for a, w in zip(ref, p.w_host)]
        for i, (a, want) in enumerate(zip(p.a, ref)):
            _same_bits_or_both_nan(bits(a), want.view(np.uint32), f"c {c} step {step} tensor {i}")
        for w, want in zip(p.w, p.w_host):
            _same_bits_or_both_nan(bits(w), want.view(np.uint32), "w is only read")
        assert np.array_equal(bits(p.a[-2]), bits(p.a[-1]))              # element by element == float4, NaN payloads included
    assert float(p._bufs[1][0]) == 0.0 and float(p._bufs[1][N_VIEW + 1:].abs().max()) == 0.0      # nothing beside the view
    moved = [not np.array_equal(a.view(np.uint32), a0.view(np.uint32)) for a, a0 in zip(ref, p.a_host)]
    assert all(moved)                                # (the updates did run, on every tensor)


# ------------------------------------------------------------------------------------------------ 2. special branches
def test_no_update_copy_and_the_device_coefficient(dev):
    p = Problem(dev, 23)
    for t, h in ((p.a, p.a_host), (p.w, p.w_host)):                      # arbitrary NaN payloads on both sides
        for i in (0, 2, 4, 6, 7):
            h[i].view(np.uint32)[8:12] = PAYLOADS if t is p.a else PAYLOADS[::-1]
        p.put(t, h)
    a0, w0 = [bits(a) for a in p.a], [bits(w) for w in p.w]
    for i in (0, 2, 4, 6, 7):
        assert np.array_equal(a0[i][8:12], PAYLOADS)                     # (the upload kept them)
    c_dev = torch.zeros(1, device=dev)
    for value in (None, 0.0, -1.0, float("nan"), -float("inf")):         # by value 0; from the device 0, negative, NaN
        if value is None:
            p.update(0.0)
        else:
            c_dev.fill_(value)
            p.update(0.5, c_dev)                                         # the argument is not read
        assert all(np.array_equal(bits(a), b) for a, b in zip(p.a, a0)), value
        assert all(np.array_equal(bits(w), b) for w, b in zip(p.w, w0)), value
    # the device coefficient == the same coefficient by value
    q = Problem(dev, 23)
    for t, h in ((q.a, p.a_host), (q.w, p.w_host)):
        q.put(t, h)
    c_dev.fill_(0.1)
    p.update(0.9, c_dev)
    q.update(float(np.float32(0.1)))
    for i, (x, y) in enumerate(zip(p.a, q.a)):
        assert np.array_equal(bits(x), bits(y)), i
    assert not np.array_equal(bits(p.a[2]), a0[2])
    # c = 1, by value and from the device (and anything above): avg takes w's bits
    for how in ("value", "device", "device 2.5"):
        p.put(p.a, p.a_host)
        if how == "value":
            p.update(1.0)
        else:
            c_dev.fill_(1.0 if how == "device" else 2.5)
            p.update(0.0, c_dev)
        assert all(np.array_equal(bits(a), b) for a, b in zip(p.a, w0)), how
        assert all(np.array_equal(bits(w), b) for w, b in zip(p.w, w0)), how


# ------------------------------------------------------------------------------------------------ 3. swap
def test_swap_exchanges_the_bits_and_twice_is_the_identity(dev):
    p = Problem(dev, 24)
    for h in (p.a_host, p.w_host):
        for i in (0, 2, 4, 6, 7):
            h[i].view(np.uint32)[8:12] = PAYLOADS
            if h is p.w_host:
                h[i].view(np.uint32)[12:16] = PAYLOADS[::-1]
    p.put(p.a, p.a_host)
    p.put(p.w, p.w_host)
    a0, w0 = [bits(a) for a in p.a], [bits(w) for w in p.w]
    assert any(not np.array_equal(x, y) for x, y in zip(a0, w0))
    p.swap()
    assert all(np.array_equal(bits(a), b) for a, b in zip(p.a, w0)) and all(np.array_equal(bits(w), b) for w, b in zip(p.w, a0))
    assert float(p._bufs[0][0]) == 0.0 and float(p._bufs[0][N_VIEW + 1:].abs().max()) == 0.0
    p.swap()
    assert all(np.array_equal(bits(a), b) for a, b in zip(p.a, a0)) and all(np.array_equal(bits(w), b) for w, b in zip(p.w, w0))


# ------------------------------------------------------------------------------------------------ 4. trajectory
@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_trajectory_stays_inside_the_derived_bound(dev, decay):
    """200 updates against the float64 recurrence: per tensor max |avg - ideal| <= B of weight_average_ref.py (steady state
    1.01 * 2^-24 (max|avg| + 2 c max|w - avg|) / c); the float32 reference, whose bits the kernel has, uses less than half of it
    on these inputs (tests/test_weight_average_cpu.py shows the same on the CPU)."""
    p = Problem(dev, 25, specials=False)
    c = R.coefficient("ema", 1, 0, decay=decay, warmup=False)
    rs = np.random.RandomState(26)
    a32, a64, bound = [a.copy() for a in p.a_host], [a.astype(np.float64) for a in p.a_host], [0.0] * len(p.a_host)
    for _ in range(200):
        for w in p.w_host[:-1]:
            w += (0.05 * rs.randn(w.size) * np.abs(w)).astype(np.float32)
        p.w_host[-1] = p.w_host[-2].copy()
        p.put(p.w, p.w_host)
        p.update(float(c))
        new = [R.ideal_f64(a, w, c) for a, w in zip(a64, p.w_host)]
        bound = [R.error_bound(b, c, a, w.astype(np.float64), n) for b, a, w, n in zip(bound, a64, p.w_host, new)]
        a32, a64 = [R.update_f32(a, w, c) for a, w in zip(a32, p.w_host)], new
    for i, (a, ref32, ref64, b) in enumerate(zip(p.a, a32, a64, bound)):
        got = a.detach().cpu().numpy().reshape(-1)
        assert np.array_equal(got.view(np.uint32), ref32.view(np.uint32)), i
        err, err32 = np.abs(got.astype(np.float64) - ref64).max(), np.abs(ref32.astype(np.float64) - ref64).max()
        print(f"decay {decay} tensor {i}: error {err:.3e}, float32 reference {err32:.3e}, bound {b:.3e}")
        assert err <= b and err32 <= 0.5 * b
        assert b <= 1.02 * 2.0 ** -24 * (np.abs(ref64).max() * 3.0) * min(200.0, 1.0 / float(c)) * 1.5       # of the stated order


# ------------------------------------------------------------------------------------------------ 5. TripletTrainer, eager
def _simple2(dev, seed=5, enc=64):
    from embeddingnet_amd import backbones as B
    base, _ = B.get_backbone((64, 64, 3), encodings_len=enc, backbone_name="simple2", backbone_weights=None, seed=seed, device=dev)
    return base


def _batches(dev, steps, p=4, k=4, n_classes=12, size=64):
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((n_classes, size, size, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(n_classes, generator=torch.Generator().manual_seed(i))[:p].to(dev)
        x = protos[cls].repeat_interleave(k, 0) + 0.15 * torch.randn((p * k, size, size, 3), device=dev, generator=gen)
        yield x.clamp(0, 1), cls.repeat_interleave(k).to(torch.int32)


def _named(module):
    from embeddingnet_amd.backbones import keras_weights
    return {k: v.detach().cpu().numpy().copy() for k, v in keras_weights(module).items()}


def test_triplet_trainer_keeps_the_reference_average_and_leaves_the_weights_alone(dev):
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer
    from embeddingnet_amd.weight_average import WeightAverager
    base, twin = _simple2(dev), _simple2(dev)
    avg = WeightAverager(base, mode="ema", decay=0.9)
    assert any("moving_mean" in k for k in avg.averaged) and any("moving_variance" in k for k in avg.averaged)
    assert set(avg.averaged) == set(_named(base)) and all(v.dtype == torch.float32 for v in avg.averaged.values())
    ref = _named(base)
    for k, v in avg.averaged.items():                                    # at construction: a bit copy
        assert np.array_equal(bits(v), ref[k].reshape(-1).view(np.uint32)), k
    tr = TripletTrainer(base, KerasOptimizer([q for q in base.parameters()], "adam", 1e-3), 4, 4, seed=3, averager=avg)
    tw = TripletTrainer(twin, KerasOptimizer([q for q in twin.parameters()], "adam", 1e-3), 4, 4, seed=3)
    for t, (x, _) in enumerate(_batches(dev, 12), 1):
        la, lb = tr.step(x), tw.step(x)
        assert torch.equal(la, lb)
        snap = _named(base)
        c = R.coefficient("ema", t, t - 1, decay=0.9)
        assert 0 < c < 1 and avg.coefficient(t, t - 1) == float(c)
        ref = {k: R.update_f32(ref[k], snap[k], c) for k in ref}
        assert avg.n_averaged == t and avg.iterations == t
        for k, v in avg.averaged.items():
            assert np.array_equal(bits(v), ref[k].reshape(-1).view(np.uint32)), (t, k)
        other = _named(twin)
        for k in snap:
            assert np.array_equal(snap[k].view(np.uint32), other[k].view(np.uint32)), (t, k)
    moved = [k for k in ref if not np.array_equal(ref[k], snap[k])]
    assert any("moving_mean" in k for k in moved) and any("kernel" in k for k in moved)          # the average lags the model


# ------------------------------------------------------------------------------------------------ 6. graph
N_CLASSES = 12


def _graph_trainer(dev, cls, mode, graph):
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.proxies import ProxyHead
    from embeddingnet_amd.train_step import ProxyTrainer, TripletTrainer, XbmTrainer
    from embeddingnet_amd.weight_average import WeightAverager
    from embeddingnet_amd.xbm import CrossBatchMemory
    base = _simple2(dev)
    kw = dict(decay=0.9) if mode == "ema" else {}
    params = [q for q in base.parameters() if q.requires_grad]
    if cls == "proxy":
        head = ProxyHead(N_CLASSES, 64, seed=1).to(dev)
        avg = WeightAverager([base, head], mode=mode, update_every=3, start_iteration=2, **kw)
        assert "proxy_head/proxies" in avg.averaged
        tr = ProxyTrainer(base, head, KerasOptimizer(params + [head.proxies], "adam", 1e-3), loss="proxy_anchor", seed=3, graph=graph,
                          averager=avg)
        return base, avg, tr
    avg = WeightAverager(base, mode=mode, update_every=3, start_iteration=2, **kw)
    opt = KerasOptimizer(params, "adam", 1e-3)
    if cls == "triplet":
        return base, avg, TripletTrainer(base, opt, 4, 4, seed=3, graph=graph, averager=avg)
    memory = CrossBatchMemory(48, 64, dev)
    return base, avg, XbmTrainer(base, opt, 4, 4, seed=3, graph=graph, memory=memory, averager=avg)


def _step(tr, cls, x, y):
    return tr.step(x) if cls == "triplet" else tr.step(x, y)


@pytest.mark.parametrize("mode", ["ema", "swa"])
@pytest.mark.parametrize("cls", ["triplet", "proxy", "xbm"])
def test_replayed_steps_average_like_eager_ones(dev, cls, mode):
    """16 steps, the ones past GRAPH_WARMUP replayed, updates at steps 2, 5, 8, ...: the replays in between run the launch with
    c = 0 from the state row.  Averages, weights and counters equal an eager twin's after every step."""
    runs = []
    for graph in (False, True):
        base, avg, tr = _graph_trainer(dev, cls, mode, graph)
        seen = []
        for t, (x, y) in enumerate(_batches(dev, 16), 1):
            loss = _step(tr, cls, x, y).clone()
            assert avg.iterations == t and avg.n_averaged == len([s for s in range(2, t + 1, 3)]), (t, avg.counters())
            seen.append([loss, torch.cat([q.detach().reshape(-1) for q in base.parameters()]),
                         torch.cat([v.reshape(-1) for v in avg.averaged.values()])])
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
            assert tr._since_capture >= 7
        runs.append(seen)
    for t, (a, b) in enumerate(zip(*runs), 1):
        for j, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (t, ["loss", "weights", "averages"][j])
    eager = runs[0]
    assert torch.equal(eager[2][2], eager[3][2]) and not torch.equal(eager[3][2], eager[4][2])     # steps 3, 4: c = 0; step 5 updates


def test_a_failed_or_discarded_capture_leaves_the_counters(dev):
    base, avg, tr = _graph_trainer(dev, "triplet", "ema", False)
    batches = list(_batches(dev, 6))
    for x, _ in batches[:4]:
        tr.step(x)
    before = (avg.counters(), tr.opt.iterations, tr.step_no)
    assert before[0] == (4, 1)
    kept = torch.cat([v.reshape(-1) for v in avg.averaged.values()]).clone()
    tr._capture(batches[4][0])                                           # step 5 would update: the dry run advances, then restores
    assert tr._graph is not None, getattr(tr, "_graph_error", "")
    assert (avg.counters(), tr.opt.iterations, tr.step_no) == before
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([v.reshape(-1) for v in avg.averaged.values()]), kept)          # nothing ran
    tr._graph, tr._state = None, None                                    # discarded
    tr.opt.coef_dev = tr.opt._ptrs = tr.opt._table = None
    real = avg.update

    def failing(t=None, c_dev=None):
        real(t, c_dev)
        raise RuntimeError("no capture today")
    avg.update = failing
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tr._capture(batches[4][0])
    avg.update = real
    assert tr._graph is None and tr._graph_failed and any("graph capture failed" in str(w.message) for w in caught)
    assert (avg.counters(), tr.opt.iterations, tr.step_no) == before
    tr.step(batches[4][0])                                               # eager from here on, and it counts
    assert avg.counters() == (5, 2) and not torch.equal(torch.cat([v.reshape(-1) for v in avg.averaged.values()]), kept)


# ------------------------------------------------------------------------------------------------ 7. applied() on a model with planes
def _resnet(dev, seed):
    from embeddingnet_amd import backbones as B
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="resnet18", backbone_weights=None, seed=seed, device=dev)
    return base


def _encode(base, x):
    was = base.training
    base.eval()
    with torch.no_grad():
        out = base(x).clone()
    base.train(was)
    return out


@pytest.mark.parametrize("graph", [False, True])
def test_applied_puts_the_averages_into_a_model_with_planes(dev, graph):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd import _lib
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer
    from embeddingnet_amd.weight_average import WeightAverager
    steps, more = (10, 4) if graph else (4, 3)
    batches = list(_batches(dev, steps + more, p=4, k=2))
    probe = batches[-1][0]
    runs = []
    for enters in (True, False):
        base = _resnet(dev, 7)
        avg = WeightAverager(base, mode="ema", decay=0.9)
        tr = TripletTrainer(base, KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-3), 4, 2, seed=3,
                            graph=graph, averager=avg)
        for x, _ in batches[:steps]:
            tr.step(x)
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        if enters:
            assert any(hasattr(m.kernel, "_embnet_wplanes") or hasattr(m.kernel, "_embnet_wrange") for m in base.modules()
                       if hasattr(m, "kernel")), "no conv of this model caches planes or a range: the test would show nothing"
            held = {k: v.detach().cpu().numpy().copy() for k, v in avg.averaged.items()}
            live = _encode(base, probe)
            with avg.applied():
                inside = _encode(base, probe)
                with pytest.raises(_lib.EmbnetError, match="does not nest"):
                    with avg.applied():
                        pass
                with pytest.raises(_lib.EmbnetError, match="inside applied"):
                    avg.update()
            fresh = _resnet(dev, 99)
            B.load_keras_weights(fresh, held)
            want = _encode(fresh, probe)
            assert torch.equal(inside.view(torch.int32), want.view(torch.int32)), (inside - want).abs().max()
            assert not torch.equal(inside, live)
            assert torch.equal(_encode(base, probe).view(torch.int32), live.view(torch.int32))
            for k, v in avg.averaged.items():
                assert np.array_equal(bits(v), held[k].reshape(-1).view(np.uint32)), k
        for x, _ in batches[steps:]:
            tr.step(x)
        runs.append((torch.cat([q.detach().reshape(-1) for q in base.parameters()]), torch.cat([b.reshape(-1) for b in base.buffers()]),
                     torch.cat([v.reshape(-1) for v in avg.averaged.values()]), avg.counters()))
    for j, (u, v) in enumerate(zip(*runs)):
        same = u == v if j == 3 else torch.equal(u.view(torch.int32), v.view(torch.int32))
        assert same, ["weights", "buffers", "averages", "counters"][j]


def test_applied_refuses_stream_capture_and_copy_to_is_one_way(dev, monkeypatch):
    from embeddingnet_amd import _lib
    from embeddingnet_amd.weight_average import WeightAverager
    base = _simple2(dev)
    avg = WeightAverager(base, mode="swa")
    with torch.no_grad():
        for q in base.parameters():
            q.add_(1.0)
    held = torch.cat([v.reshape(-1) for v in avg.averaged.values()]).clone()
    with monkeypatch.context() as m:                                     # (what a capturing stream answers)
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(_lib.EmbnetError, match="stream capture"):
            with avg.applied():
                pass
    assert not avg._applied
    state = avg.state_dict()
    avg.copy_to()
    now = torch.cat([v.detach().reshape(-1) for v in _named_tensors(base, avg)])
    assert torch.equal(now, held) and torch.equal(torch.cat([v.reshape(-1) for v in avg.averaged.values()]), held)
    other = WeightAverager(_simple2(dev, seed=9), mode="swa")
    other.load_state_dict(state)
    assert torch.equal(torch.cat([v.reshape(-1) for v in other.averaged.values()]), held) and other.n_averaged == 0
    bad = dict(state, averaged={k: v for k, v in list(state["averaged"].items())[1:]})
    with pytest.raises(_lib.EmbnetError, match="names differ"):
        other.load_state_dict(bad)
    first = next(iter(state["averaged"]))
    bad = dict(state, averaged=dict(state["averaged"], **{first: torch.zeros(3, device=dev)}))
    with pytest.raises(_lib.EmbnetError, match="has shape"):
        other.load_state_dict(bad)


def _named_tensors(base, avg):
    from embeddingnet_amd.backbones import keras_weights
    named = keras_weights(base)
    return [named[k] for k in avg.averaged]


# ------------------------------------------------------------------------------------------------ 8. CLI
def _cli(tmp_path, name, averaging="keep", extra=(), epochs=3):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", f"{name}.yml")))
    assert "weight_averaging" in cfg["TRAIN"]
    cfg["GENERAL"]["work_dir"] = str(tmp_path) + "/"
    cfg["GENERATOR"]["n_batches"] = 6
    if averaging is None:
        del cfg["TRAIN"]["weight_averaging"]
    elif averaging != "keep":
        cfg["TRAIN"]["weight_averaging"].update(averaging)
    path = tmp_path / "cfg.yml"
    path.write_text(yaml.safe_dump(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(path), "--synthetic", "10", "--max_epochs",
                          str(epochs), *extra], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout, str(path)


def _checkpoints(tmp_path, name):
    saved = sorted(os.listdir(tmp_path / name / "weights"))
    assert saved and saved == sorted(os.listdir(tmp_path / name / "averaged")) == sorted(os.listdir(tmp_path / name / "optimizer"))
    return saved


@pytest.mark.parametrize("mode", ["ema", "swa"])
def test_train_cli_averages_saves_and_loads(dev, tmp_path, mode):
    from embeddingnet_amd.models import TripletNet
    from embeddingnet_amd.utils import parse_params
    name = f"simple2_{mode}_synthetic"
    out, cfg_path = _cli(tmp_path, name)
    counts = [int(v) for v in re.findall(r" - averaged (\d+)", out)]
    print(out)
    assert counts == ([6, 12, 18] if mode == "ema" else [1, 2, 3])       # 6 steps per epoch; swa: one snapshot per epoch from epoch 1
    saved = _checkpoints(tmp_path, name)
    for f in saved:
        with np.load(tmp_path / name / "weights" / f) as live, np.load(tmp_path / name / "averaged" / f) as avg, \
                np.load(tmp_path / name / "optimizer" / f) as state:
            n = int(state["__extra__n_averaged"])
            assert n == counts[int(state["__extra__epoch"]) - 1]
            assert set(avg.files) == set(live.files)
            differ = [k for k in live.files if not np.array_equal(live[k], avg[k])]
            # swa's first snapshot is a copy of the model; every later average, and every ema, lags it
            assert (not differ) if (mode == "swa" and n == 1) else any("kernel" in k for k in differ), (f, n, differ[:3])
    cfg = parse_params(cfg_path)
    cfg["model"]["device"], cfg["model"]["seed"] = dev, 99
    net = TripletNet(cfg, training=True)
    net.load_model(str(tmp_path / name / "averaged" / saved[-1]))        # the averaged file serves inference as a weights file does
    with np.load(tmp_path / name / "averaged" / saved[-1]) as avg:
        for k, v in _named(net.base_model).items():
            assert np.array_equal(v, avg[k]), k


def test_train_cli_resumes_the_averages(tmp_path):
    import shutil
    name = "simple2_ema_synthetic"
    _cli(tmp_path, name, epochs=1)
    saved = _checkpoints(tmp_path, name)
    for kind in ("weights", "averaged", "optimizer"):                    # (a resumed run writes its own epoch_001 over the first run's)
        os.makedirs(tmp_path / "kept" / kind)
        shutil.copy(tmp_path / name / kind / saved[-1], tmp_path / "kept" / kind / "last.npz")
    last = tmp_path / "kept" / "weights" / "last.npz"
    with np.load(tmp_path / "kept" / "optimizer" / "last.npz") as state:
        n, it = int(state["__extra__n_averaged"]), int(state["__iterations__"])
    assert n == it > 0
    out, _ = _cli(tmp_path, name, extra=("--resume_from", str(last)), epochs=1)
    found = re.search(r"resumed averaged weights from \S+ \(averaged (\d+)\)", out)
    assert found and int(found.group(1)) == n, out[-1500:]
    assert [int(v) for v in re.findall(r" - averaged (\d+)", out)] == [n + 6]
    # without the sibling the averages start from the resumed model, and the run says so
    shutil.rmtree(tmp_path / "kept" / "averaged")
    out, _ = _cli(tmp_path, name, extra=("--resume_from", str(last)), epochs=1)
    assert "the averages start from the resumed model" in out and [int(v) for v in re.findall(r" - averaged (\d+)", out)] == [6]


def test_train_cli_evaluate_model_is_a_run_without_the_key(tmp_path):
    name = "simple2_ema_synthetic"
    vals = []
    for averaging in ({"evaluate": "model"}, None):
        work = tmp_path / str(len(vals))
        work.mkdir()
        out, _ = _cli(work, name, averaging=averaging, epochs=2)
        vals.append((re.findall(r" - loss (\S+)", out), re.findall(r" - val_loss (\S+)", out)))
        assert (" - averaged " in out) == (averaging is not None)
    print(vals)
    assert len(vals[0][1]) == 2 and vals[0] == vals[1]                   # the same training, the same validation values
