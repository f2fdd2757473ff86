#!/usr/bin/env python3
"""Loss path of the fused training step at the BASELINE config sizes: launches and microseconds, fused vs separate.

  python tools/losspath_bench.py [--json profiles/r02_losspath.json]          (GPU box)

For C1 (8x4 = 32 rows, E = 256, semihard), C2 (32x4 = 128, E = 256, hardest), C2 batch-hard and C5 (64x4 = 256, E = 512,
semihard) the forward + backward of the loss path is run both ways on the same clustered embeddings (the *_batch_all cases
run ops.batch_all_triplet_loss beside the fused `hardest` path at the same shape instead, the *_multi_similarity cases
ops.multi_similarity_loss beside the fused `hardest` path and beside batch-all, the *_supcon cases ops.supcon_loss with either
denominator beside ops.multi_similarity_loss, the *_fast_ap / *_smooth_ap cases (`--only _ap`) ops.fast_ap_loss / ops.smooth_ap_loss at
their defaults beside ops.supcon_loss('all'), the *_circle cases (`--only circle`, which also takes the xbm_circle cases) ops.circle_loss
at its defaults beside ops.supcon_loss('all'), the *_distance_weighted cases (`--only distance_weighted`) ops.margin_loss at its defaults
beside ops.batch_all_triplet_loss and ops.circle_loss; the *_proxy_anchor / *_proxy_softmax cases are described at proxy_cases(), the
xbm_* cases (the cross-batch memory) at xbm_cases(), `--xbm-step` at xbm_step_time(), the mproxy_* cases (SoftTriple and sub-centre
ArcFace on several centres per class; `--only mproxy_`) at mproxy_cases()):
  separate: ops.pairwise_distances -> ops.mine_triplets / ops.batch_hard -> ops.triplet_gather_loss -> backward
  fused:    ops.fused_triplet_loss (one forward launch) -> backward
Reported per variant: library launches per pass and the sum of their device times (embnet_trace_*: HIP events on the
launch stream), and the wall time per pass of back-to-back passes (launch overheads overlap with the device work).
SURVEY.md §8d asks for microseconds and launch counts at these sizes: the path is latency-bound, not bandwidth-bound.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from embeddingnet_amd import _lib, ops  # noqa: E402

CASES = [("c1", 8, 4, 256, "semihard"), ("c2", 32, 4, 256, "hardest"), ("c2_batch_hard", 32, 4, 256, "batch_hard"),
         ("c5", 64, 4, 512, "semihard"),
         ("c1_batch_all", 8, 4, 256, "batch_all"), ("c2_batch_all", 32, 4, 256, "batch_all"),
         ("c5_batch_all", 64, 4, 512, "batch_all"),
         ("c1_multi_similarity", 8, 4, 256, "multi_similarity"), ("c2_multi_similarity", 32, 4, 256, "multi_similarity"),
         ("c5_multi_similarity", 64, 4, 512, "multi_similarity"),
         ("c1_supcon", 8, 4, 256, "supcon"), ("c2_supcon", 32, 4, 256, "supcon"), ("c5_supcon", 64, 4, 512, "supcon")] + \
        [(f"{cfg}_{mode}", p, k, e, mode) for mode in ("fast_ap", "smooth_ap", "circle", "distance_weighted")
         for cfg, p, k, e in (("c1", 8, 4, 256), ("c2", 32, 4, 256), ("c5", 64, 4, 512))]


# the losses on class proxies: (name, p, k, e, classes, mode)
PROXY_CASES = [(f"{cfg}_{mode}", p, k, e, 100, mode) for mode in ("proxy_anchor", "proxy_softmax")
               for cfg, p, k, e in (("c1", 8, 4, 256), ("c2", 32, 4, 256), ("c5", 64, 4, 512))] + \
              [("c2_proxy_anchor_c4096", 32, 4, 256, 4096, "proxy_anchor"), ("c2_proxy_softmax_c4096", 32, 4, 256, 4096, "proxy_softmax")]


def measure(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    _lib.trace_enable(True); _lib.trace_reset()
    fn()
    torch.cuda.synchronize()
    rec = _lib.trace_records()
    _lib.trace_enable(False)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / iters
    return dict(launches=len(rec), device_us=round(1e3 * sum(r[1] for r in rec), 1), wall_us_per_pass=round(1e6 * wall, 1),
                kernels={r[0].replace("embnet::", ""): round(1e3 * r[1], 1) for r in rec})


def torch_proxy_loss(mode, x, w, labels, a, b):
    """The same loss composed from torch ops (matmul, logsumexp, autograd): the yardstick of the proxy cases."""
    c = w.shape[0]
    s = (x @ w.T) * torch.rsqrt((w * w).sum(1))
    pos = labels[:, None] == torch.arange(c, device=x.device)[None, :]
    if mode == "proxy_softmax":
        t = a * (s - b * pos)
        return (torch.logsumexp(t, 1) - (t * pos).sum(1)).mean()       # (no boolean gather: the leg is captured in a graph)
    ninf = torch.full((), -float("inf"), device=x.device)
    z = torch.zeros((c, 1), device=x.device)
    lp = torch.logsumexp(torch.cat([z, torch.where(pos, -a * (s - b), ninf).T], 1), 1)
    ln = torch.logsumexp(torch.cat([z, torch.where(pos, ninf, a * (s + b)).T], 1), 1)
    present = pos.any(0)
    return (lp * present).sum() / present.sum() + ln.sum() / c


def graph_rounds(legs, rounds, reps):
    """Each leg (a forward + backward) captured once into a graph; `rounds` alternating rounds of `reps` replays timed with events.
    -> {leg: median device microseconds per pass}.  Replays leave the host out: this is device time for library and torch legs alike."""
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in legs.items():
        with torch.cuda.stream(side):                        # warm-up off the default stream, as capture wants it
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphs[name] = g
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, g in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g.replay()
            t0.record()
            for _ in range(reps):
                g.replay()
            t1.record()
            t1.synchronize()
            times[name].append(1e3 * t0.elapsed_time(t1) / reps)
    return {name: round(sorted(v)[len(v) // 2], 2) for name, v in times.items()}


def proxy_cases(a, dev, out):
    """ops.proxy_anchor_loss / ops.proxy_softmax_loss (forward + backward w.r.t. embeddings and proxies) beside two other legs in the
    same process, alternating: the same loss composed from torch ops, and ops.multi_similarity_loss at the same N and E.  Device
    microseconds are medians of alternating rounds of graph replays; launches and per-kernel times of the library leg come from the
    library's trace."""
    for name, p, k, e, c, mode in PROXY_CASES:
        if a.only and a.only not in name:
            continue
        n = p * k
        g = torch.Generator(device=dev).manual_seed(7)
        cen = torch.rand((p, e), device=dev, generator=g)
        x = (cen.repeat_interleave(k, 0) + 0.25 * torch.randn((n, e), device=dev, generator=g)).abs()
        x = (x / x.norm(dim=1, keepdim=True)).requires_grad_(True)
        w = (torch.randn((c, e), device=dev, generator=g) * (2.0 / c) ** 0.5).requires_grad_(True)
        labels = torch.randperm(c, device=dev, generator=g)[:p].repeat_interleave(k).to(torch.int32)
        fn = ops.PROXY_LOSS_MODES[mode][0]
        sa, sb = (32.0, 0.1) if mode == "proxy_anchor" else (64.0, 0.35)
        lab64 = labels.long()

        def hip():
            x.grad = w.grad = None
            fn(x, w, labels, sa, sb)[0].backward()

        def composed():
            x.grad = w.grad = None
            torch_proxy_loss(mode, x, w, lab64, sa, sb).backward()

        def multi_similarity():
            x.grad = None
            ops.multi_similarity_loss(x, p, k)[0].backward()

        def hip_fwd():
            fn(x, w, labels, sa, sb)

        def composed_fwd():
            torch_proxy_loss(mode, x, w, lab64, sa, sb)

        trace = measure(hip, a.iters)
        med = graph_rounds(dict(hip=hip, torch_composed=composed, multi_similarity=multi_similarity, hip_forward=hip_fwd,
                                torch_composed_forward=composed_fwd), rounds=15, reps=20)
        row = dict(config=name, N=n, E=e, C=c, mining=mode, path={1: "small", 2: "matrix"}[_lib.lib().embnet_proxy_loss_path(n, c, e)],
                   hip=trace, device_us_median=med,
                   device_ratio_vs_torch_composed=round(med["hip"] / med["torch_composed"], 3),
                   device_ratio_vs_multi_similarity=round(med["hip"] / med["multi_similarity"], 3))
        out.append(row)
        print(json.dumps(row), flush=True)


# the losses on several centres per class: (name, p, k, e, classes, centres per class, mode), at the proxy cases' shapes with 1, 3 and
# 10 centres (4096 classes with 10 centres are past the 16384 rows of the range)
MPROXY_CASES = [(f"mproxy_{cfg}_{mode}_kc{kc}", p, k, e, 100, kc, mode) for mode in ("soft_triple", "arcface") for kc in (1, 3, 10)
                for cfg, p, k, e in (("c1", 8, 4, 256), ("c2", 32, 4, 256), ("c5", 64, 4, 512))] + \
               [(f"mproxy_c2_{mode}_c4096_kc3", 32, 4, 256, 4096, 3, mode) for mode in ("soft_triple", "arcface")]


def torch_mproxy_loss(mode, x, w, labels, c, kc):
    """The same loss composed from torch ops (matmul, softmax / max, logsumexp, autograd) at the layers' default parameters: the
    yardstick of the mproxy cases."""
    wn = w * torch.rsqrt((w * w).sum(1, keepdim=True))
    s = (x @ wn.T).reshape(x.shape[0], c, kc)
    pos = labels[:, None] == torch.arange(c, device=x.device)[None, :]
    if mode == "soft_triple":
        sp = (torch.softmax(s / 0.1, 2) * s).sum(2)
        t = 20.0 * (sp - 0.01 * pos)
        if kc == 1:                                         # no pairs of centres: no regulariser
            return (torch.logsumexp(t, 1) - (t * pos).sum(1)).mean()
        gram = wn.reshape(c, kc, -1) @ wn.reshape(c, kc, -1).transpose(1, 2)
        iu = torch.triu_indices(kc, kc, 1, device=x.device)                # (no boolean gather: the leg is captured in a graph)
        reg = 0.2 / (c * kc * (kc - 1)) * torch.sqrt(2.0 + 1e-5 - 2.0 * gram[:, iu[0], iu[1]]).sum()
    else:
        sp = s.max(2).values
        m, th = 0.5, -0.8775825619
        phi = torch.where(sp > th, sp * 0.8775825619 - torch.sqrt(torch.clamp(1.0 - sp * sp, min=1e-12)) * 0.4794255386, sp - 0.4794255386 * m)
        t = 64.0 * torch.where(pos, phi, sp)
        reg = 0.0
    return (torch.logsumexp(t, 1) - (t * pos).sum(1)).mean() + reg


def mproxy_cases(a, dev, out):
    """ops.soft_triple_loss / ops.arcface_loss (forward + backward w.r.t. embeddings and centres, default parameters) beside the same
    loss composed from torch ops and, where the shape fits both, beside the forward path that `auto` does not take, in one process,
    alternating; measured as proxy_cases() measures.  Only with `--only mproxy...` or without `--only`."""
    for name, p, k, e, c, kc, mode in MPROXY_CASES:
        if a.only and not (a.only.startswith("mproxy") and a.only in name):
            continue
        n = p * k
        g = torch.Generator(device=dev).manual_seed(7)
        cen = torch.rand((p, e), device=dev, generator=g)
        x = (cen.repeat_interleave(k, 0) + 0.25 * torch.randn((n, e), device=dev, generator=g)).abs()
        x = (x / x.norm(dim=1, keepdim=True)).requires_grad_(True)
        w = (torch.randn((c * kc, e), device=dev, generator=g) * (2.0 / (c * kc)) ** 0.5).requires_grad_(True)
        labels = torch.randperm(c, device=dev, generator=g)[:p].repeat_interleave(k).to(torch.int32)
        fn = ops.MULTI_PROXY_LOSS_MODES[mode][0]
        lab64 = labels.long()

        def hip():
            x.grad = w.grad = None
            fn(x, w, labels, c)[0].backward()

        def composed():
            x.grad = w.grad = None
            torch_mproxy_loss(mode, x, w, lab64, c, kc).backward()

        def hip_fwd():
            fn(x, w, labels, c)

        def composed_fwd():
            torch_mproxy_loss(mode, x, w, lab64, c, kc)

        def hip_other():
            x.grad = w.grad = None
            fn(x, w, labels, c, path=other)[0].backward()

        def hip_other_fwd():
            fn(x, w, labels, c, path=other)

        path = {1: "small", 2: "matrix"}[_lib.lib().embnet_multi_proxy_loss_path(n, c, kc, e)]
        other = "small" if path == "matrix" else "matrix"
        legs = dict(hip=hip, torch_composed=composed, hip_forward=hip_fwd, torch_composed_forward=composed_fwd)
        if other == "matrix" or (e + c * kc <= 4096 and n * c * kc * e <= 2 ** 25):          # the path `auto` does not take, where the shape allows it: the crossover's evidence
            legs.update({f"hip_{other}": hip_other, f"hip_{other}_forward": hip_other_fwd})
        trace = measure(hip, a.iters)
        med = graph_rounds(legs, rounds=15, reps=20)
        row = dict(config=name, N=n, E=e, C=c, KC=kc, mining=mode, path=path, hip=trace, device_us_median=med,
                   device_ratio_vs_torch_composed=round(med["hip"] / med["torch_composed"], 3))
        out.append(row)
        print(json.dumps(row), flush=True)


# the cross-batch memory: (name, n, e, m, kind)
XBM_CASES = [(f"xbm_{kind}_e{e}_m{m}", 128, e, m, kind) for kind in ("contrastive", "multi_similarity", "circle") for e in (128, 256)
             for m in (1024, 8192, 65536)]


def torch_xbm_step(kind, x, labels, mem, mem_labels, cursor, params):
    """Enqueue and loss composed from torch ops (index_copy_, matmul, where, logsumexp, autograd), everything on the device: the
    yardstick of the xbm cases."""
    n, m = x.shape[0], mem.shape[0]
    slots = (cursor + torch.arange(n, device=x.device)) % m
    mem.index_copy_(0, slots, x.detach())
    mem_labels.index_copy_(0, slots, labels)
    cursor.add_(n).remainder_(m)
    s = x @ mem.T
    ok = (labels >= 0)[:, None] & (mem_labels >= 0)[None, :] & (torch.arange(m, device=x.device)[None, :] != slots[:, None])
    same = labels[:, None] == mem_labels[None, :]
    pos, neg = ok & same, ok & ~same
    zero = torch.zeros((), device=x.device)
    if kind == "contrastive":
        return (torch.where(pos & (1.0 - s > 0), 1.0 - s, zero).sum(1) + torch.where(neg & (s > params["margin"]), s, zero).sum(1)).mean()
    inf = torch.full((), float("inf"), device=x.device)
    if kind == "circle":
        mr, ga = params["m"], params["gamma"]
        lp = torch.logsumexp(torch.where(pos, -ga * (1.0 + mr - s).clamp(min=0).detach() * (s - (1.0 - mr)), -inf), 1)
        ln = torch.logsumexp(torch.where(neg, ga * (s + mr).clamp(min=0).detach() * (s - mr), -inf), 1)
        return torch.where(pos.any(1) & neg.any(1), torch.nn.functional.softplus(lp + ln), zero).mean()
    al, be, ba, eps = params["alpha"], params["beta"], params["base"], params["epsilon"]
    mn, mx = torch.where(pos, s, inf).min(1).values, torch.where(neg, s, -inf).max(1).values
    kp, kn = pos & ((mx + eps)[:, None] > s), neg & ((s + eps) > mn[:, None])
    z = torch.zeros((n, 1), device=x.device)
    lp = torch.logsumexp(torch.cat([z, torch.where(kp, -al * (s - ba), -inf)], 1), 1) / al
    ln = torch.logsumexp(torch.cat([z, torch.where(kn, be * (s - ba), -inf)], 1), 1) / be
    return torch.where(kn.any(1), lp + ln, zero).mean()


def xbm_cases(a, dev, out):
    """ops.xbm_enqueue + ops.xbm_contrastive_loss / ops.xbm_multi_similarity_loss / ops.xbm_circle_loss + backward at N = 128 against a full memory of M
    slots, beside the same step composed from torch ops, in one process, alternating: device microseconds are medians of
    alternating rounds of graph replays; launches and per-kernel times of the library leg come from the library's trace."""
    from embeddingnet_amd.xbm import CrossBatchMemory
    for name, n, e, m, kind in XBM_CASES:
        if a.only and a.only not in name:
            continue
        g = torch.Generator(device=dev).manual_seed(7)
        classes = 256
        cen = torch.rand((classes, e), device=dev, generator=g)

        def rows(lab):
            r = (cen[lab.long()] + 0.25 * torch.randn((lab.shape[0], e), device=dev, generator=g)).abs()
            return r / r.norm(dim=1, keepdim=True)
        labels = torch.randperm(classes, device=dev, generator=g)[:n // 4].repeat_interleave(4).to(torch.int32)
        x = rows(labels).requires_grad_(True)
        bank_labels = torch.randint(0, classes, (m,), device=dev, generator=g).to(torch.int32)
        memory = CrossBatchMemory(m, e, dev)
        memory.feats.copy_(rows(bank_labels)); memory.labels.copy_(bank_labels)
        t_mem, t_lab, t_cur = memory.feats.clone(), bank_labels.long(), torch.zeros(1, dtype=torch.long, device=dev)
        fn, keys = ops.XBM_LOSS_MODES[kind]
        params = dict(contrastive=dict(margin=0.5), multi_similarity=dict(alpha=2.0, beta=50.0, base=0.5, epsilon=0.1),
                      circle=dict(m=0.4, gamma=80.0))[kind]
        lab64 = labels.long()

        def hip():
            x.grad = None
            fn(x, labels, memory.feats, memory.labels, memory.enqueue(x, labels), **params)[0].backward()

        def composed():
            x.grad = None
            torch_xbm_step(kind, x, lab64, t_mem, t_lab, t_cur, params).backward()

        trace = measure(hip, a.iters)
        med = graph_rounds(dict(hip=hip, torch_composed=composed), rounds=15, reps=20)
        row = dict(config=name, N=n, E=e, M=m, kind=kind, hip=trace, device_us_median=med,
                   device_ratio_vs_torch_composed=round(med["hip"] / med["torch_composed"], 3))
        out.append(row)
        print(json.dumps(row), flush=True)


def xbm_step_time(config, m, rounds=7, steps=10):
    """One process, one leg: the training step of `config` ('simple2': simple2 64 x 64, 8 x 4, semihard; 'c2': ResNet18 224 x 224,
    32 x 4, hardest; E = 256, graph-replayed) with a contrastive cross-batch memory of m slots (XbmTrainer) or, m = 0, without
    (TripletTrainer), on eight resident random batches taken in turn, so that the in-batch loss stays live in both legs (a step
    whose loss has died propagates zero gradients, and the backbone's backward kernels run measurably faster on zeros).
    -> median, min and max milliseconds per step over `rounds` rounds of `steps` steps timed with events, and the live count."""
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer, XbmTrainer
    from embeddingnet_amd.xbm import CrossBatchMemory
    dev = torch.device("cuda:0")
    backbone, image, p, k, mining = dict(simple2=("simple2", 64, 8, 4, "semihard"), c2=("resnet18", 224, 32, 4, "hardest"))[config]
    g = torch.Generator(device=dev).manual_seed(3)
    pool = [torch.rand((p * k, image, image, 3), device=dev, generator=g) for _ in range(8)]
    y = torch.arange(p, dtype=torch.int32, device=dev).repeat_interleave(k)
    tick = [0]

    def x():
        tick[0] += 1
        return pool[tick[0] % 8]
    base, _ = B.get_backbone((image, image, 3), encodings_len=256, backbone_name=backbone, backbone_weights=None, seed=1, device=dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-4)
    if m:
        tr = XbmTrainer(base, opt, p, k, negatives_selection_mode=mining, graph=True, memory=CrossBatchMemory(m, 256, dev))
        step = lambda: tr.step(x(), y)
    else:
        tr = TripletTrainer(base, opt, p, k, negatives_selection_mode=mining, graph=True)
        step = lambda: tr.step(x())
    for _ in range(TripletTrainer.GRAPH_WARMUP + 6 + (m // (p * k) if config == "simple2" else 0)):     # captured; simple2: a full memory
        step()
    torch.cuda.synchronize()
    times, live = [], []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            step()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) / steps)
        live.append(int(tr.last_triplets[1].sum().item()))
    row = dict(config=f"xbm_step_{config}", M=m, live_triplets_min=min(live), graph=tr._graph is not None, step_ms_median=round(sorted(times)[len(times) // 2], 4),
               step_ms_min_max=[round(min(times), 4), round(max(times), 4)],
               filled=None if not m else tr.memory.filled())
    print(json.dumps(row), flush=True)
    return row


def step_times(out, rounds=9, steps=10):
    """The simple2 64 x 64 training step, 8 x 4 batches, in proxy_anchor mode (ProxyTrainer, 100 classes) beside supcon mode
    (TripletTrainer), eager steps, alternating rounds of `steps` steps timed with events: median milliseconds per step."""
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.proxies import ProxyHead
    from embeddingnet_amd.train_step import ProxyTrainer, TripletTrainer
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.rand((32, 64, 64, 3), device=dev, generator=g)
    y = torch.arange(8, dtype=torch.int32, device=dev).repeat_interleave(4)
    legs = {}
    for mode in ("proxy_anchor", "supcon"):
        base, _ = B.get_backbone((64, 64, 3), encodings_len=256, backbone_name="simple2", backbone_weights=None, seed=1, device=dev)
        params = [q for q in base.parameters() if q.requires_grad]
        if mode == "supcon":
            tr = TripletTrainer(base, KerasOptimizer(params, "adam", 1e-3), 8, 4, negatives_selection_mode="supcon", graph=False)
            legs[mode] = lambda tr=tr: tr.step(x)
        else:
            head = ProxyHead(100, 256).to(dev)
            tr = ProxyTrainer(base, head, KerasOptimizer(params + [head.proxies], "adam", 1e-3), loss=mode, graph=False)
            legs[mode] = lambda tr=tr: tr.step(x, y)
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / steps)
    row = dict(config="simple2_step_8x4_64px", step_ms_median={k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()},
               step_ms_min_max={k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()})
    out.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, help="run only the cases whose name contains this")
    ap.add_argument("--xbm-step", default=None, choices=["simple2", "c2"], help="time one training step leg (xbm_step_time) and exit")
    ap.add_argument("--xbm-memory", type=int, default=0, help="--xbm-step: slots of the cross-batch memory, 0 = none")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.xbm_step:
        row = xbm_step_time(a.xbm_step, a.xbm_memory)
        if a.json:
            json.dump([row], open(a.json, "w"), indent=1)
        return
    out = []
    for name, p, k, e, mode in CASES:
        if a.only and a.only not in name:
            continue
        n = p * k
        g = torch.Generator(device=dev).manual_seed(7)
        c = torch.rand((p, e), device=dev, generator=g)
        x = (c.repeat_interleave(k, 0) + 0.25 * torch.randn((n, e), device=dev, generator=g)).abs()
        x = (x / x.norm(dim=1, keepdim=True)).requires_grad_(True)

        def separate():
            x.grad = None
            with torch.no_grad():
                d = ops.pairwise_distances(x)
                if mode == "batch_hard":
                    trip, count = ops.batch_hard(d, p, k)
                else:
                    trip, count, _ = ops.mine_triplets(d, p, k, 0.5, mode, seed=1)
            ops.triplet_gather_loss(x, trip, count, 0.5)[0].backward()

        def fused():
            x.grad = None
            ops.fused_triplet_loss(x, p, k, 0.5, mode, seed=1)[0].backward()

        def batch_all():
            x.grad = None
            ops.batch_all_triplet_loss(x, p, k, 0.5)[0].backward()

        def hardest_fused():
            x.grad = None
            ops.fused_triplet_loss(x, p, k, 0.5, "hardest", seed=1)[0].backward()

        def multi_similarity():
            x.grad = None
            ops.multi_similarity_loss(x, p, k)[0].backward()

        def supcon(denominator):
            def leg():
                x.grad = None
                ops.supcon_loss(x, p, k, 0.1, denominator)[0].backward()
            return leg

        def ap_loss():
            x.grad = None
            dict(fast_ap=ops.fast_ap_loss, smooth_ap=ops.smooth_ap_loss, circle=ops.circle_loss)[mode](x, p, k)[0].backward()

        if mode in ("fast_ap", "smooth_ap", "circle"):                # the two legs alternate in one process, at one shape, twice over
            row = dict(config=name, N=n, E=e, mining=mode)
            for rnd in (1, 2):
                row[f"{mode}_{rnd}"] = measure(ap_loss, a.iters)
                row[f"supcon_all_{rnd}"] = measure(supcon("all"), a.iters)
            row[f"device_ratio_{mode}_vs_supcon_all"] = round(min(row[f"{mode}_1"]["device_us"], row[f"{mode}_2"]["device_us"])
                                                              / min(row["supcon_all_1"]["device_us"], row["supcon_all_2"]["device_us"]), 3)
            out.append(row)
            print(json.dumps(row), flush=True)
            continue
        if mode == "distance_weighted":                     # beside batch-all and Circle loss: the same skeleton, so the rest is the sampler
            def margin():
                x.grad = None
                ops.margin_loss(x, p, k, seed=1)[0].backward()

            def circle():
                x.grad = None
                ops.circle_loss(x, p, k)[0].backward()

            row = dict(config=name, N=n, E=e, mining=mode)
            for rnd in (1, 2):                              # the three legs alternate in one process, at one shape, twice over
                row[f"distance_weighted_{rnd}"] = measure(margin, a.iters)
                row[f"batch_all_{rnd}"] = measure(batch_all, a.iters)
                row[f"circle_{rnd}"] = measure(circle, a.iters)
            best = {leg: min(row[f"{leg}_1"]["device_us"], row[f"{leg}_2"]["device_us"]) for leg in ("distance_weighted", "batch_all", "circle")}
            row["device_ratio_vs_batch_all"] = round(best["distance_weighted"] / best["batch_all"], 3)
            row["device_ratio_vs_circle"] = round(best["distance_weighted"] / best["circle"], 3)
            out.append(row)
            print(json.dumps(row), flush=True)
            continue
        if mode == "supcon":                                # the three legs alternate in one process, at one shape
            row = dict(config=name, N=n, E=e, mining=mode, supcon_all=measure(supcon("all"), a.iters),
                       supcon_negatives=measure(supcon("negatives"), a.iters),
                       multi_similarity=measure(multi_similarity, a.iters))
            for leg in ("supcon_all", "supcon_negatives"):
                row[f"device_ratio_{leg}_vs_multi_similarity"] = round(row[leg]["device_us"] / row["multi_similarity"]["device_us"], 3)
            out.append(row)
            print(json.dumps(row), flush=True)
            continue
        if mode == "multi_similarity":                      # the three legs alternate in one process, at one shape
            row = dict(config=name, N=n, E=e, mining=mode, multi_similarity=measure(multi_similarity, a.iters),
                       hardest_fused=measure(hardest_fused, a.iters), batch_all=measure(batch_all, a.iters))
            row["device_ratio_vs_hardest"] = round(row["multi_similarity"]["device_us"] / row["hardest_fused"]["device_us"], 3)
            row["device_ratio_vs_batch_all"] = round(row["multi_similarity"]["device_us"] / row["batch_all"]["device_us"], 3)
            out.append(row)
            print(json.dumps(row), flush=True)
            continue
        if mode == "batch_all":                             # batch-all beside the fused `hardest` path, same shape and process
            row = dict(config=name, N=n, E=e, mining=mode, batch_all=measure(batch_all, a.iters),
                       hardest_fused=measure(hardest_fused, a.iters))
            row["device_ratio_vs_hardest"] = round(row["batch_all"]["device_us"] / row["hardest_fused"]["device_us"], 3)
            out.append(row)
            print(json.dumps(row), flush=True)
            continue
        row = dict(config=name, N=n, E=e, mining=mode, separate=measure(separate, a.iters))
        if ops.fused_loss_supported(p, k, e):
            row["fused"] = measure(fused, a.iters)
        out.append(row)
        print(json.dumps(row), flush=True)
    proxy_cases(a, dev, out)
    mproxy_cases(a, dev, out)
    xbm_cases(a, dev, out)
    if a.only and a.only in "proxy_step_time":
        step_times(out)
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
