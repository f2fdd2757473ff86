#!/usr/bin/env python3
"""What generalised-mean pooling (embnet_gem_fwd / embnet_gem_bwd, layers.GeM) costs beside average pooling (embnet_gap_fwd /
embnet_gap_bwd), kernels of both in one process.

  python tools/pooling_bench.py [--rounds 9] [--reps 200] [--step] [--json out.json]          (GPU box)

Kernels, at the head's shapes [128, 7, 7, 512], [128, 7, 7, 1280] and [128, 7, 7, 2048] (ResNet18/34, EfficientNet, ResNet50+): the
legs gap_fwd, gem_fwd (no dy/dp), gem_fwd_dydp, gap_bwd, gem_bwd (dx only) and gem_bwd_dp (dx + the exponent's gradient) alternate
in rounds; a round is `reps` back-to-back calls on one stream between two device events.  Reported per leg: the median, minimum
and maximum over the rounds in microseconds per call (launch gaps included: what a stream of such calls pays), the median of the
kernels' own durations from the library's trace (embnet_trace_*: events around every launch, taken in a separate pass), the
bytes the operation must move (forward 4 B, backward 8 B per element) over that kernel time, and the ratio to the GAP leg.
--step: a ResNet18 224 x 224 32x4 TripletTrainer step with pooling='gem' against the default head, two trainers alternating rounds
of eager steps timed on the host around a device synchronisation; the difference of the medians is the step delta."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SHAPES = ((128, 7, 7, 512), (128, 7, 7, 1280), (128, 7, 7, 2048))


def stats(v):
    v = sorted(v)
    return dict(us_median=round(v[len(v) // 2], 2), us_min=round(v[0], 2), us_max=round(v[-1], 2))


def kernel_legs(dev, shape):
    from embeddingnet_amd import _lib
    from embeddingnet_amd._lib import check, stream
    lib = _lib.lib()
    n, h, w, c = shape
    hw = h * w
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(shape, device=dev, generator=gen).sub_(0.4).clamp_(min=0)          # a ReLU's output: exact zeros among the values
    dy = torch.randn((n, c), device=dev, generator=gen)
    p = torch.full((1,), 3.0, device=dev)
    y, dydp, dx, dp = torch.empty_like(dy), torch.empty_like(dy), torch.empty_like(x), torch.empty_like(p)
    ws = torch.zeros(lib.embnet_gem_bwd_workspace_bytes(c) // 8 + 1, dtype=torch.float64, device=dev)
    P = lambda t: t.data_ptr()  # noqa: E731
    check(lib.embnet_gem_fwd(P(x), n, hw, c, P(p), 0, 1e-6, P(y), P(dydp), stream()))
    elems = n * hw * c
    return {
        "gap_fwd": (lambda: lib.embnet_gap_fwd(P(x), n, hw, c, P(y), stream()), 4 * elems),
        "gem_fwd": (lambda: lib.embnet_gem_fwd(P(x), n, hw, c, P(p), 0, 1e-6, P(y), None, stream()), 4 * elems),
        "gem_fwd_dydp": (lambda: lib.embnet_gem_fwd(P(x), n, hw, c, P(p), 0, 1e-6, P(y), P(dydp), stream()), 4 * elems),
        "gap_bwd": (lambda: lib.embnet_gap_bwd(P(dy), n, hw, c, None, P(dx), stream()), 4 * elems),
        "gem_bwd": (lambda: lib.embnet_gem_bwd(P(dy), P(x), P(y), P(p), 0, 1e-6, n, hw, c, P(dx), None, None, None, 0, stream()), 8 * elems),
        "gem_bwd_dp": (lambda: lib.embnet_gem_bwd(P(dy), P(x), P(y), P(p), 0, 1e-6, n, hw, c, P(dx), P(dydp), P(dp), P(ws), ws.numel() * 8,
                                                  stream()), 8 * elems),
    }, (x, dy, p, y, dydp, dx, dp, ws)


def bench_kernels(dev, rounds, reps):
    from embeddingnet_amd import _lib
    out = {}
    for shape in SHAPES:
        legs, keep = kernel_legs(dev, shape)
        for fn, _ in legs.values():                           # warm-up: code objects loaded, clocks up
            for _ in range(20):
                assert fn() == 0
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for _ in range(rounds):
            for name, (fn, _) in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(1e3 * e0.elapsed_time(e1) / reps)
        case = {}
        for name, (fn, nbytes) in legs.items():               # the kernels' own durations, a pass of their own
            _lib.trace_reset(); _lib.trace_enable(True)
            try:
                for _ in range(50):
                    fn()
                torch.cuda.synchronize()
                per_call = {}
                for kname, ms, *_ in _lib.trace_records():
                    per_call.setdefault(kname, []).append(1e3 * ms)
            finally:
                _lib.trace_enable(False)
            kernel_us = sum(sorted(v)[len(v) // 2] for v in per_call.values())         # (gem_bwd_dp: two kernels per call)
            case[name] = dict(stats(times[name]), kernel_us=round(kernel_us, 2), kernels=sorted(per_call), bytes=nbytes,
                              gb_per_s=round(nbytes / kernel_us / 1e3, 1))
        for name, base in (("gem_fwd", "gap_fwd"), ("gem_fwd_dydp", "gap_fwd"), ("gem_bwd", "gap_bwd"), ("gem_bwd_dp", "gap_bwd")):
            case[name]["ratio_to_gap"] = round(case[name]["us_median"] / case[base]["us_median"], 2)
            case[name]["kernel_ratio_to_gap"] = round(case[name]["kernel_us"] / case[base]["kernel_us"], 2)
        out["x".join(map(str, shape))] = case
        del keep
    return out


def bench_step(dev, rounds, reps):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer
    p, k, size = 32, 4, 224

    def trainer(pooling):
        base, _ = B.get_backbone((size, size, 3), encodings_len=256, backbone_name="resnet18", backbone_weights=None, seed=0, device=dev,
                                 pooling=pooling)
        opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-4)
        return TripletTrainer(base, opt, p, k, seed=1, graph=False)
    gen = torch.Generator(device=dev).manual_seed(0)
    protos = torch.rand((p, size, size, 3), device=dev, generator=gen)
    x = (protos.repeat_interleave(k, 0) + 0.15 * torch.randn((p * k, size, size, 3), device=dev, generator=gen)).clamp(0, 1)
    legs = {"avg": trainer(None), "gem": trainer("gem")}
    times = {name: [] for name in legs}
    for tr in legs.values():
        for _ in range(5):
            tr.step(x)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, tr in legs.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                tr.step(x)
            torch.cuda.synchronize()
            times[name].append(1e6 * (time.perf_counter() - t0) / reps)
    case = {name: stats(v) for name, v in times.items()}
    case["difference_us"] = round(case["gem"]["us_median"] - case["avg"]["us_median"], 1)
    case["gem_p"] = round(float(legs["gem"].model.net.head.gem.p.detach()), 5)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", action="store_true", help="also time the ResNet18 training step with and without GeM")
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pooling_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    out = dict(rounds=a.rounds, reps=a.reps, kernels=bench_kernels(dev, a.rounds, a.reps))
    if a.step:
        out["resnet18_224_32x4_step"] = dict(reps=a.step_reps, **bench_step(dev, a.rounds, a.step_reps))
    print(json.dumps(out))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
