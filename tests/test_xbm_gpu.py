"""The cross-batch memory (csrc/xbm.hip: ops.xbm_enqueue, ops.xbm_contrastive_loss, ops.xbm_multi_similarity_loss) against the float64
reference and the a-priori bounds of tests/xbm_ref.py, the ring against the NumPy ring (eager and replayed from a captured graph),
the refusals through the C ABI, and inside the training step (train_step.XbmTrainer: eager and graph-replayed) and tools/train.py.

Every check prints its largest error / bound before it asserts ratio < 1.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ms_ref as M
import xbm_ref as X

pytestmark = pytest.mark.gpu
UP = 0.75
KIND_CODE = {"contrastive": 1, "multi_similarity": 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs of a case, shared by the tests and left unchanged (read-only arrays)."""
    return X.case_inputs(name)


@functools.lru_cache(maxsize=None)
def _reference(kind, name):
    c = _case(name)
    return X.reference(kind, c["x"], c["labels"], c["mem"], c["mem_labels"], c["self_slots"], **c["params"][kind])


def _fn(kind):
    from embeddingnet_amd import ops
    return ops.xbm_contrastive_loss if kind == "contrastive" else ops.xbm_multi_similarity_loss


def _run(kind, c, dev, g=None, **override):
    params = dict(c["params"][kind], **override)
    t = lambda a: None if a is None else torch.tensor(a, device=dev)
    xt = t(c["x"]).requires_grad_(True)
    mean, counts, gw = _fn(kind)(xt, t(c["labels"]), t(c["mem"]), t(c["mem_labels"]), t(c["self_slots"]), return_weights=True, **params)
    mean.backward(None if g is None else torch.tensor(g, device=dev))
    torch.cuda.synchronize()
    return dict(loss=float(mean.item()), counts=counts.cpu().numpy(), G=gw.cpu().numpy(), demb=xt.grad.cpu().numpy(),
                t=(mean.detach().clone(), counts.clone(), gw, xt.grad))


def _check(kind, got, c, gs, g=1.0, what="", ref=None):
    """Everything the header promises about one forward + backward, for a device whose S is within gs A of the truth: zero G outside
    every set, the kept sets (between `sure` and `may`; at most 1 % of the decisions open, and those judged with the device's own
    decision), the four counters, every entry of G (contrastive: exactly -1 / +1 / 0), the loss, and, from the device's own G, every
    element of demb; no gradient on unlabelled rows.  -> {check: largest error / bound}."""
    x, lab, mem, mlab, slots = c["x"], c["labels"], c["mem"], c["mem_labels"], c["self_slots"]
    n, m = x.shape[0], mem.shape[0]
    params = c["params"][kind]
    assert gs > 0 or X.exact_in_any_order(x, mem, c["unit"])              # gamma_S = 0 only where S is exact in any order
    assert got["G"].shape == (n, m) and got["counts"].dtype == np.int32 and got["counts"].shape == (4,)
    assert np.isfinite(got["G"]).all() and np.isfinite(got["demb"]).all() and np.isfinite(got["loss"])
    pos, neg = X.sets(lab, mlab, slots)
    nz = got["G"] != 0
    assert not nz[~(pos | neg)].any()                                      # unlabelled rows, empty slots, the own copies
    assert np.all(got["G"][pos] <= 0) and np.all(got["G"][neg] >= 0)
    d = X.decisions(kind, x, lab, mem, mlab, slots, gs, **params)
    assert d["share"] <= 0.01, d["share"]
    ref = X.reference(kind, x, lab, mem, mlab, slots, **params) if ref is None else ref
    closed = ~d["open"]
    assert np.array_equal(nz[closed], (ref["keep_pos"] | ref["keep_neg"])[closed])
    assert np.all((d["sure_pos"] | d["sure_neg"]) <= nz) and np.all(nz <= (d["may_pos"] | d["may_neg"]))
    if d["open"].any():
        ref = X.reference(kind, x, lab, mem, mlab, slots, keep=(nz & pos, nz & neg), **params)
    assert np.array_equal(got["counts"], ref["counts"].astype(np.int32)), (got["counts"], ref["counts"])
    bg, _, bl = X.bounds(ref, gs)
    kept = ref["keep_pos"] | ref["keep_neg"]
    ratios = dict(open_share=d["share"])
    if kind == "contrastive":
        assert np.array_equal(got["G"], ref["G"].astype(np.float32))       # -1, +1 or 0: exact
        ratios["G"] = 0.0
    else:
        ratios["G"] = float((np.abs(got["G"] - ref["G"])[kept] / bg[kept]).max()) if kept.any() else 0.0
    ratios["loss"] = float(abs(got["loss"] - ref["loss"]) / bl) if bl > 0 else float(got["loss"] != 0)
    want, bound = X.grad(mem, got["G"], g)
    ratios["demb"] = float((np.abs(got["demb"] - want) / bound).max())
    assert not got["demb"][lab < 0].any()                                  # an unlabelled row receives no gradient
    print(f"xbm {what} {kind} n={n} m={m} e={x.shape[1]} counts={got['counts']}: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    assert ratios["G"] < 1 and ratios["loss"] < 1 and ratios["demb"] < 1, ratios
    return ratios


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("name", X.CASES)
def test_values(dev, name, kind):
    c = _case(name)
    e = c["x"].shape[1]
    gs = X.gamma_s(e, c["unit"] is not None)
    first = _run(kind, c, dev)
    r = _check(kind, first, c, gs, what=name, ref=_reference(kind, name))
    if c["unit"] is not None:
        assert r["open_share"] == 0                                        # grid inputs: counters and G's support checked exactly
    second = _run(kind, c, dev, g=UP)                                      # upstream != 1, and two runs bitwise equal
    _check(kind, second, c, gs, g=UP, what=name + " upstream", ref=_reference(kind, name))
    for a, b in zip(first["t"][:3], second["t"][:3]):
        assert torch.equal(a, b)
    third = _run(kind, c, dev, g=UP)
    assert torch.equal(second["t"][3], third["t"][3])


def test_a_bank_that_is_the_batch_agrees_with_the_in_batch_multi_similarity_loss(dev):
    from embeddingnet_amd import ops
    c = _case("bank_is_batch")
    n, m, e = X.SHAPES["bank_is_batch"]
    got = _run("multi_similarity", c, dev)
    mean, counts = ops.multi_similarity_loss(torch.tensor(c["x"], device=dev), 4, 2)
    ref, want = _reference("multi_similarity", "bank_is_batch"), M.reference(c["x"], 4, 2)
    gs_ms = M.gamma_s(M.auto_path(4, 2, e), e)
    assert not M.decisions(c["x"], 4, 2, 0.1, gs_ms)["open"].any()         # both kernels' decisions are sure on this input
    assert not X.decisions("multi_similarity", c["x"], c["labels"], c["mem"], c["mem_labels"], c["self_slots"], X.gamma_s(e))["open"].any()
    assert got["counts"][:3].tolist() == counts.cpu().numpy()[:3].tolist() and got["counts"][3] == n
    bound = X.bounds(ref, X.gamma_s(e))[2] + M.bounds(c["x"], want, gs_ms)[2]
    err = abs(got["loss"] - float(mean.item()))
    print("xbm vs in-batch multi-similarity: |difference| / (sum of both bounds)", err / bound)
    assert err < bound


@pytest.mark.parametrize("kind", X.KINDS)
def test_no_self_slots_and_out_of_range_self_slots_exclude_nothing(dev, kind):
    c = dict(_case("ragged"))
    # rows of norm 0.9: without its exclusion an own copy is a positive at S = 0.81, a sure decision (at norm 1 it sits on 1 - S = 0)
    c["x"], c["mem"] = (np.float32(0.9) * c["x"]), (np.float32(0.9) * c["mem"])
    for slots in (None, np.full(12, -1, np.int32), np.array([40, 41, 1 << 30, -5] * 3, np.int32)):
        c["self_slots"] = slots
        got = _run(kind, c, dev, g=UP)
        _check(kind, got, c, X.gamma_s(5), g=UP, what="self_slots " + ("None" if slots is None else str(slots[:4])))


@pytest.mark.parametrize("kind", X.KINDS)
def test_all_unlabelled_gives_zero_loss_and_zero_weights(dev, kind):
    c = dict(_case("ragged"))
    lab = np.full(12, -1, np.int32)
    lab[3], lab[5] = np.iinfo(np.int32).min, -2
    c["labels"] = lab
    got = _run(kind, c, dev, g=UP)
    assert got["loss"] == 0.0 and not got["G"].any() and not got["demb"].any()
    assert got["counts"].tolist() == [0, 0, 0, int((c["mem_labels"] >= 0).sum())]


# ---------------------------------------------------------------------------------------------------------------- 2. refusals
def _abi(dev, n=8, m=16, e=4):
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    wsn = max(lib.embnet_xbm_loss_workspace_bytes(n, m, e), 64)
    t = dict(x=torch.rand((n, e), device=dev), lab=torch.zeros(n, dtype=torch.int32, device=dev), mem=torch.rand((m, e), device=dev),
             mlab=torch.ones(m, dtype=torch.int32, device=dev), slots=torch.full((n,), -1, dtype=torch.int32, device=dev),
             g=torch.full((n * m,), float("nan"), device=dev), counts=torch.full((4,), -12345, dtype=torch.int32, device=dev),
             mean=torch.full((1,), float("nan"), device=dev), ws=torch.zeros(wsn // 4 + 4, device=dev))
    return lib, _lib, t, wsn


def _fwd(lib, _lib, t, wsn, n=8, m=16, e=4, kind=1, a=0.5, b=50.0, c=0.5, d=0.1, null=(), ws_off=0, ws_bytes=None):
    p = {k: (None if k in null else v.data_ptr()) for k, v in t.items()}
    return lib.embnet_xbm_loss_fwd(p["x"], p["lab"], p["mem"], p["mlab"], p["slots"], n, m, e, kind, a, b, c, d, p["g"], p["counts"],
                                   p["mean"], None if "ws" in null else p["ws"] + ws_off, wsn if ws_bytes is None else ws_bytes,
                                   _lib.stream())


def test_out_of_range_calls_are_refused_before_a_launch(dev):
    lib, _lib, t, wsn = _abi(dev)
    EINVAL, EWORKSPACE = -1, -3
    nan, inf = float("nan"), float("inf")
    bad = [dict(n=17), dict(n=1), dict(m=65537), dict(n=2048, m=65536), dict(e=0), dict(e=4097), dict(kind=0), dict(kind=3),
           dict(a=nan), dict(a=inf), dict(kind=2, a=0.0), dict(kind=2, a=2.0, b=-1.0), dict(kind=2, a=2.0, c=nan),
           dict(kind=2, a=2.0, d=-0.1), dict(kind=2, a=2.0, d=inf), dict(ws_off=4),
           *(dict(null=(k,)) for k in ("x", "lab", "mem", "mlab", "g", "counts", "mean", "ws"))]
    for kw in bad:
        assert _fwd(lib, _lib, t, wsn, **kw) == EINVAL, kw
        assert lib.embnet_last_error().decode().startswith("xbm_loss_fwd"), kw
    assert _fwd(lib, _lib, t, wsn, ws_bytes=wsn - 16) == EWORKSPACE and _fwd(lib, _lib, t, wsn, ws_bytes=0) == EWORKSPACE
    for shape in ((17, 16, 4), (1, 16, 4), (8, 65537, 4), (2048, 65536, 4), (8, 16, 0)):
        assert lib.embnet_xbm_loss_workspace_bytes(*shape) == 0 and lib.embnet_xbm_loss_path(*shape) == 0
    assert lib.embnet_xbm_loss_path(8, 16, 4) == 1 and wsn == X.workspace_bytes(8, 16, 4)
    demb, up = torch.full((8 * 4,), nan, device=dev), torch.ones(1, device=dev)
    for n, m, e, null in ((17, 16, 4, ()), (8, 65537, 4, ()), (2048, 65536, 4, ()), (8, 16, 4097, ()), (8, 16, 4, ("mem",)),
                          (8, 16, 4, ("g",)), (8, 16, 4, ("demb",)), (8, 16, 4, ("ws",)), (8, 16, 4, ("misaligned",)), (8, 16, 4, ("short",))):
        rc = lib.embnet_xbm_loss_bwd(None if "mem" in null else t["mem"].data_ptr(), n, m, e, None if "g" in null else t["g"].data_ptr(),
                                     up.data_ptr(), None if "demb" in null else demb.data_ptr(),
                                     None if "ws" in null else t["ws"].data_ptr() + (4 if "misaligned" in null else 0),
                                     wsn - 16 if "short" in null else wsn, _lib.stream())
        assert rc == (EWORKSPACE if "short" in null else EINVAL), (n, m, e, null)
    ring = dict(cursor=torch.zeros(1, dtype=torch.int32, device=dev), out=torch.full((16,), -7, dtype=torch.int32, device=dev))
    for n, m, e, null in ((17, 16, 4, ()), (0, 16, 4, ()), (8, 65537, 4, ()), (8, 16, 0, ()), (8, 16, 4, ("cursor",)), (8, 16, 4, ("ws",))):
        rc = lib.embnet_xbm_enqueue(t["x"].data_ptr(), t["lab"].data_ptr(), n, e, t["mem"].data_ptr(), t["mlab"].data_ptr(), m,
                                    None if "cursor" in null else ring["cursor"].data_ptr(), ring["out"].data_ptr(),
                                    None if "ws" in null else t["ws"].data_ptr(), _lib.stream())
        assert rc == EINVAL, (n, m, e, null)
    torch.cuda.synchronize()
    # nothing ran: every output is as it was
    assert torch.isnan(t["g"]).all() and torch.isnan(t["mean"]).all() and (t["counts"] == -12345).all() and torch.isnan(demb).all()
    assert (ring["out"] == -7).all() and ring["cursor"].item() == 0 and (t["mlab"] == 1).all() and not t["ws"].any()
    assert _fwd(lib, _lib, t, wsn) == 0                                     # and the same buffers serve a good call
    torch.cuda.synchronize()
    assert torch.isfinite(t["g"]).all() and t["counts"][3].item() == 16 and t["ws"][:4].view(torch.int32)[0].item() == 0


def test_python_refusals(dev):
    from embeddingnet_amd import ops
    from embeddingnet_amd._lib import EmbnetError
    from embeddingnet_amd.xbm import CrossBatchMemory
    x, lab = torch.rand((8, 4), device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    mem, mlab = torch.rand((16, 4), device=dev), torch.zeros(16, dtype=torch.int32, device=dev)
    with pytest.raises(EmbnetError, match="labels"):
        ops.xbm_contrastive_loss(x, lab.long(), mem, mlab)
    with pytest.raises(EmbnetError, match="mem_labels"):
        ops.xbm_contrastive_loss(x, lab, mem, mlab[:8])
    with pytest.raises(EmbnetError, match="self_slots"):
        ops.xbm_multi_similarity_loss(x, lab, mem, mlab, lab[:4])
    with pytest.raises(EmbnetError, match="width"):
        ops.xbm_contrastive_loss(x, lab, torch.rand((16, 5), device=dev), mlab)
    with pytest.raises(EmbnetError, match="xbm_loss_fwd"):
        ops.xbm_contrastive_loss(x, lab, mem[:4], mlab[:4])                 # n > m
    with pytest.raises(EmbnetError, match="xbm_loss_fwd"):
        ops.xbm_multi_similarity_loss(x, lab, mem, mlab, alpha=-1.0)
    memory = CrossBatchMemory(6, 4, dev)
    with pytest.raises(EmbnetError, match="fit"):
        memory.enqueue(x, lab)
    with pytest.raises(EmbnetError, match="width"):
        CrossBatchMemory(16, 5, dev).enqueue(x, lab)
    assert memory.filled() == 0


# ---------------------------------------------------------------------------------------------------------------- 3. the ring
def _ring_batches(n, e, count):
    rs = np.random.RandomState(11)
    return [(rs.rand(n, e).astype(np.float32), rs.randint(0, 50, n).astype(np.int32)) for _ in range(count)]


def _same(memory, ring, slots, want_slots):
    assert np.array_equal(memory.feats.cpu().numpy(), ring.feats) and np.array_equal(memory.labels.cpu().numpy(), ring.labels)
    assert np.array_equal(slots.cpu().numpy(), want_slots) and memory.cursor.item() == ring.cursor
    assert memory.ticket[0].item() == 0 and memory.filled() == int((ring.labels >= 0).sum())


@pytest.mark.parametrize("n,m,e", [(12, 40, 5), (40, 40, 5), (3, 7, 130)])
def test_enqueue_follows_the_numpy_ring(dev, n, m, e):
    from embeddingnet_amd.xbm import CrossBatchMemory
    memory, ring = CrossBatchMemory(m, e, dev), X.Ring(m, e)
    for emb, lab in _ring_batches(n, e, 7):
        xt = torch.tensor(emb, device=dev).requires_grad_(True)
        slots = memory.enqueue(xt, torch.tensor(lab, device=dev))
        assert slots.dtype == torch.int32 and slots.shape == (n,) and not memory.feats.requires_grad
        _same(memory, ring, slots, ring.enqueue(emb, lab))
    memory.reset()
    assert memory.filled() == 0 and memory.cursor.item() == 0 and not memory.feats.any()


def test_a_captured_enqueue_replays_on_the_current_cursor(dev):
    """Seven enqueues of 12 rows into 40 slots from ONE captured launch: the cursor is device state the kernel reads, so the
    replays walk round the ring as eager calls do (a cursor baked into the launch would write the same 12 slots seven times)."""
    from embeddingnet_amd.xbm import CrossBatchMemory
    n, m, e = 12, 40, 5
    CrossBatchMemory(m, e, dev).enqueue(torch.zeros((n, e), device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    memory, ring = CrossBatchMemory(m, e, dev), X.Ring(m, e)
    sx, sl = torch.zeros((n, e), device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        slots = memory.enqueue(sx, sl)
    torch.cuda.synchronize()
    assert memory.filled() == 0 and memory.cursor.item() == 0               # capturing ran nothing
    for emb, lab in _ring_batches(n, e, 7):
        sx.copy_(torch.tensor(emb, device=dev))
        sl.copy_(torch.tensor(lab, device=dev))
        graph.replay()
        torch.cuda.synchronize()
        _same(memory, ring, slots, ring.enqueue(emb, lab))


# ---------------------------------------------------------------------------------------------------------------- 4. training
P_CLASSES, K_SAMPLES, BANK, N_CLASSES = 4, 2, 24, 12


def _trainer(dev, graph, cls="xbm", mode="multi_similarity", seed=5, **kw):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer, XbmTrainer
    from embeddingnet_amd.xbm import CrossBatchMemory
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=seed, device=dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-3)
    if cls == "triplet":
        return base, None, TripletTrainer(base, opt, P_CLASSES, K_SAMPLES, negatives_selection_mode=mode, seed=3, graph=graph)
    memory = CrossBatchMemory(BANK, 64, dev)
    return base, memory, XbmTrainer(base, opt, P_CLASSES, K_SAMPLES, negatives_selection_mode=mode, seed=3, graph=graph,
                                    memory=memory, **kw)


def _batches(dev, steps):
    """Class prototypes plus noise (the batches of tests/test_proxy_loss_gpu.py): 4 of 12 classes x 2 samples, class-contiguous."""
    gen = torch.Generator(device=dev).manual_seed(2)
    protos = torch.rand((N_CLASSES, 64, 64, 3), device=dev, generator=gen)
    for i in range(steps):
        cls = torch.randperm(N_CLASSES, generator=torch.Generator().manual_seed(i))[:P_CLASSES].to(dev)
        x = protos[cls].repeat_interleave(K_SAMPLES, 0) + 0.15 * torch.randn((P_CLASSES * K_SAMPLES, 64, 64, 3), device=dev, generator=gen)
        yield x.clamp(0, 1), cls.repeat_interleave(K_SAMPLES).to(torch.int32)


def _weights(base):
    return torch.cat([q.detach().reshape(-1) for q in base.parameters()])


@pytest.mark.parametrize("mode", ["multi_similarity", "semihard"])
def test_before_start_iteration_the_step_is_the_parents(dev, mode):
    runs = []
    for cls in ("triplet", "xbm"):
        base, memory, tr = _trainer(dev, graph=False, cls=cls, mode=mode, start_iteration=1000)
        losses = [(tr.step(x) if cls == "triplet" else tr.step(x, y)).clone() for x, y in _batches(dev, 6)]
        runs.append((torch.stack(losses), _weights(base)))
        if memory is not None:
            assert memory.filled() == 0 and memory.cursor.item() == 0 and tr.last_xbm_counts is None
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("xbm_loss", ["contrastive", "multi_similarity"])
def test_trainer_graph_replay_equals_eager(dev, xbm_loss):
    from embeddingnet_amd import _lib
    from embeddingnet_amd.train_step import TripletTrainer
    steps = TripletTrainer.GRAPH_WARMUP + 13
    runs = []
    for graph in (False, True):
        base, memory, tr = _trainer(dev, graph=graph, xbm_loss=xbm_loss, start_iteration=2)
        losses, counts = [], []
        for i, (x, y) in enumerate(_batches(dev, steps)):
            if graph and i == steps - 3:
                _lib.trace_enable(True)                                 # an eager step between replays
            losses.append(tr.step(x, y).clone())
            _lib.trace_enable(False)
            if i < 2:
                assert tr.last_xbm_counts is None and tr._graph is None
            else:
                counts.append(tr.last_xbm_counts.clone())
                assert int(tr.last_xbm_counts[3]) == min(BANK, 8 * (i - 1))      # the ring fills, then stays full (it wraps)
        if graph:
            assert tr._graph is not None, f"not captured: {getattr(tr, '_graph_error', '')}"
        runs.append((torch.stack(losses), torch.stack(counts), _weights(base), memory.feats.clone(), memory.labels.clone(),
                     memory.cursor.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()


def test_trainer_learns(dev):
    """40 steps, multi-similarity in the batch plus the contrastive memory.  As for ProxyTrainer's learning test the thresholds are
    the run's own start: the loss of the last five steps stays below the first loss taken against a FULL ring (step 3; the
    memory loss is a sum over the ring's pairs, so it grows while the ring fills), and the memory's kept negatives, which are the
    violations of the contrastive criterion, reach a lower value than at that step."""
    _, memory, tr = _trainer(dev, graph=False, xbm_loss="contrastive")
    losses, kept = [], []
    for x, y in _batches(dev, 40):
        losses.append(float(tr.step(x, y).item()))
        assert tr.last_pair_counts.shape == (4,) and tr.last_xbm_counts.shape == (4,) and tr.last_triplets[0] is None
        kept.append(int(tr.last_xbm_counts[1]))
    print("xbm trainer losses", [round(v, 3) for v in losses], "kept memory negatives", kept)
    assert np.all(np.isfinite(losses)) and memory.filled() == BANK
    assert max(losses[-5:]) < losses[3], losses
    assert min(kept[4:]) < kept[3], kept


def test_trainer_refusals(dev):
    from embeddingnet_amd.xbm import CrossBatchMemory
    with pytest.raises(ValueError, match="unknown keys"):
        _trainer(dev, graph=False, xbm_loss="contrastive", xbm_params=dict(alpha=2.0))
    with pytest.raises(KeyError):
        _trainer(dev, graph=False, xbm_loss="triplet")
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import XbmTrainer
    base, _ = B.get_backbone((64, 64, 3), encodings_len=64, backbone_name="simple2", backbone_weights=None, seed=1, device=dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-3)
    with pytest.raises(ValueError, match="smaller than a batch"):
        XbmTrainer(base, opt, 4, 2, negatives_selection_mode="multi_similarity", memory=CrossBatchMemory(7, 64, dev))
    with pytest.raises(ValueError, match="memory"):
        XbmTrainer(base, opt, 4, 2, negatives_selection_mode="multi_similarity")
    tr = XbmTrainer(base, opt, 4, 2, negatives_selection_mode="multi_similarity", memory=CrossBatchMemory(24, 32, dev), graph=False)
    x, y = next(_batches(dev, 1))
    with pytest.raises(ValueError, match="width"):
        tr.step(x, y)
    with pytest.raises(ValueError, match="int32"):
        tr.step(x, y.long())


# ---------------------------------------------------------------------------------------------------------------- 5. CLI
def _cli(tmp_path, edit=lambda cfg: cfg):
    cfg = open(os.path.join(ROOT, "configs", "simple2_xbm_synthetic.yml")).read().replace("work_dirs/", str(tmp_path) + "/")
    assert "negatives_selection_mode : 'multi_similarity'" in cfg and "xbm :" in cfg and "n_batches : 20" in cfg
    cfg_path = tmp_path / "cfg.yml"
    assert "k_classes: 8" in cfg                            # three synthetic classes: batches of 3 x 4
    cfg_path.write_text(edit(cfg.replace("n_batches : 20", "n_batches : 15").replace("k_classes: 8", "k_classes: 3")))
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path), "--synthetic", "3", "--max_epochs", "3"],
                          capture_output=True, text=True, timeout=600)


def test_train_cli_fills_the_memory(tmp_path):
    out = _cli(tmp_path)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    filled = [int(v) for v in re.findall(r"xbm_filled (\d+)", out.stdout)]
    print("xbm_filled per epoch", filled)
    # 15 batches of 12 per epoch, the memory live from step 20: empty after the first epoch, 10 batches after the second, 25 after the third
    assert filled == [0, 120, 300] and "xbm_kept" in out.stdout and "Epoch 3/3" in out.stdout


@pytest.mark.parametrize("edit,needle", [
    (lambda c: c.replace("'multi_similarity'", "'proxy_anchor'").replace("ms_loss :", "proxy_loss : {alpha: 32.0}\n  #"), "GENERATOR.xbm"),
    (lambda c: c.replace("mode : 'triplet'", "mode : 'siamese'").replace("ms_loss :", "#"), "GENERATOR.xbm"),
    (lambda c: c.replace("size: 1024", "size: 1024, alpha: 2.0"), "GENERATOR.xbm"),
    (lambda c: c.replace("size: 1024", "size: 8"), "smaller than a batch"),
], ids=["proxy mode", "siamese", "unknown key", "small memory"])
def test_train_cli_refuses_a_bad_xbm_key_before_training(tmp_path, edit, needle):
    out = _cli(tmp_path, edit)
    assert out.returncode != 0
    assert needle in out.stderr and "Epoch 1" not in out.stdout
