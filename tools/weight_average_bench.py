#!/usr/bin/env python3
"""What an averaged copy of the weights costs in the training step: TripletTrainer steps with and without a WeightAverager
(embeddingnet_amd/weight_average.py, 'ema', one update per step), two trainers of the same model in one process, alternating rounds
of `reps` eager steps timed on the host around a device synchronisation.

  python tools/weight_average_bench.py [--rounds 9] [--reps 20] [--json out.json]          (GPU box)

Two cases: simple2 at 64x64, batch 8x4, and ResNet18 at 224x224, batch 32x4 (bench.py's step).  Reported per case and leg: the
median, minimum and maximum over the rounds in microseconds per step, and the difference of the medians.  By bytes the update is
12 B per averaged element (ResNet18: 11.3 M floats, about 20 us beside a step of several ms)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def trainer(dev, backbone, size, p, k, averaged):
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer
    from embeddingnet_amd.weight_average import WeightAverager
    base, _ = B.get_backbone((size, size, 3), encodings_len=256, backbone_name=backbone, backbone_weights=None, seed=0, device=dev)
    opt = KerasOptimizer([q for q in base.parameters() if q.requires_grad], "adam", 1e-4)
    avg = WeightAverager(base, mode="ema", decay=0.999) if averaged else None
    return TripletTrainer(base, opt, p, k, seed=1, graph=False, averager=avg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = dict(rounds=a.rounds, reps=a.reps, cases={})
    for backbone, size, p, k in (("simple2", 64, 8, 4), ("resnet18", 224, 32, 4)):
        gen = torch.Generator(device=dev).manual_seed(0)
        protos = torch.rand((p, size, size, 3), device=dev, generator=gen)
        x = (protos.repeat_interleave(k, 0) + 0.15 * torch.randn((p * k, size, size, 3), device=dev, generator=gen)).clamp(0, 1)
        legs = {"plain": trainer(dev, backbone, size, p, k, False), "averaged": trainer(dev, backbone, size, p, k, True)}
        times = {name: [] for name in legs}
        for tr in legs.values():
            for _ in range(5):
                tr.step(x)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, tr in legs.items():
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    tr.step(x)
                torch.cuda.synchronize()
                times[name].append(1e6 * (time.perf_counter() - t0) / a.reps)
        case = {}
        for name, v in times.items():
            case[name] = dict(us_median=round(sorted(v)[len(v) // 2], 1), us_min=round(min(v), 1), us_max=round(max(v), 1))
        case["difference_us"] = round(case["averaged"]["us_median"] - case["plain"]["us_median"], 1)
        case["averaged_elements"] = sum(v.numel() for v in legs["averaged"].averager.averaged.values())
        out["cases"][f"{backbone}_{size}_{p}x{k}"] = case
    print(json.dumps(out))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
