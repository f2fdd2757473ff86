#!/usr/bin/env python3
"""Loss path of the fused training step at the BASELINE config sizes: launches and microseconds, fused vs separate.

  python tools/losspath_bench.py [--json profiles/r02_losspath.json]          (GPU box)

For C1 (8x4 = 32 rows, E = 256, semihard), C2 (32x4 = 128, E = 256, hardest), C2 batch-hard and C5 (64x4 = 256, E = 512,
semihard) the forward + backward of the loss path is run both ways on the same clustered embeddings (the *_batch_all cases
run ops.batch_all_triplet_loss beside the fused `hardest` path at the same shape instead, the *_multi_similarity cases
ops.multi_similarity_loss beside the fused `hardest` path and beside batch-all, the *_supcon cases ops.supcon_loss with either
denominator beside ops.multi_similarity_loss):
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
         ("c1_supcon", 8, 4, 256, "supcon"), ("c2_supcon", 32, 4, 256, "supcon"), ("c5_supcon", 64, 4, 512, "supcon")]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, help="run only the cases whose name contains this")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
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
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
