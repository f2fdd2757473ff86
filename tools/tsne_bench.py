#!/usr/bin/env python3
"""Exact on-device t-SNE (embeddingnet_amd/tsne.py, csrc/tsne.hip): time of one `TSNE().fit_transform` per size.

For each n in `--sizes` (default 1070 = the reference's 107 classes x 10 samples, 8192, 16384) at e = `--dim`, on clustered
unit-norm rows generated from a seed on the device:
  fit_transform_s       device events around the whole call (upload, PCA on the host, every kernel, the host reads), after one
                        untimed warm-up fit at a small size and one at the size itself; median of `--rounds`
  *_kernel_us           per-kernel DEVICE time from the library's event trace, in a separate traced fit (tracing slows the
                        host: the whole-call time above is taken with it off): the median over the kernel's launches, and how
                        many launches the fit made
  rows_bytes_per_iter   the algorithmic bytes of one launch of tsne_rows_kernel (4 n^2 of P + 56 n of Y and row sums)
  rows_tb_per_s         those bytes over the kernel's median time; `rows_share_of_copy_rate` = that over the 6.29 TB/s measured
                        copy rate where P (4 n^2 bytes) exceeds the 256 MiB Infinity Cache, "cache-resident" where it does not
Prints one JSON line per size."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_RATE = 6.29e12
INFINITY_CACHE = 256 << 20


def clustered(n, e, dev, seed=0, classes=107):
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.randn(classes, e, device=dev, generator=g)
    x = centres[torch.arange(n, device=dev) % classes] + 0.8 * torch.randn(n, e, device=dev, generator=g)
    return x / x.norm(dim=1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1070, 8192, 16384])
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=1000)
    args = ap.parse_args()
    from embeddingnet_amd import _lib
    from embeddingnet_amd.tsne import TSNE
    dev = torch.device("cuda:0")
    TSNE(max_iter=250, device=dev).fit(clustered(256, args.dim, dev))          # code objects, torch's allocator
    for n in args.sizes:
        x = clustered(n, args.dim, dev)
        TSNE(max_iter=250, device=dev).fit(x)
        secs, t = [], None
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = TSNE(max_iter=args.max_iter, device=dev)
            a.record()
            t.fit(x)
            b.record()
            b.synchronize()
            secs.append(1e-3 * a.elapsed_time(b))
        _lib.trace_enable(True)
        _lib.trace_reset()
        TSNE(max_iter=args.max_iter, device=dev).fit(x)
        torch.cuda.synchronize()
        per = {}
        for name, ms, _, _, _ in _lib.trace_records():
            per.setdefault(name.split("::")[-1], []).append(1e3 * ms)
        _lib.trace_enable(False)
        _lib.trace_reset()
        rows_bytes = 4.0 * n * n + 56.0 * n
        rows_us = float(np.median(per["tsne_rows_kernel"]))
        res = {"n": n, "e": args.dim, "max_iter": args.max_iter, "n_iter": t.n_iter_ + 1, "kl_divergence": round(t.kl_divergence_, 5),
               "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
               "fit_transform_s": round(float(np.median(secs)), 4), "fit_transform_s_min_max": [round(min(secs), 4), round(max(secs), 4)],
               "kernel_us_median": {k: round(float(np.median(v)), 2) for k, v in per.items()},
               "kernel_launches": {k: len(v) for k, v in per.items()},
               "kernel_total_s": round(sum(sum(v) for v in per.values()) * 1e-6, 4),
               "rows_bytes_per_iter": rows_bytes, "rows_kernel_us": round(rows_us, 2),
               "rows_tb_per_s": round(rows_bytes / (rows_us * 1e-6) / 1e12, 3),
               "rows_share_of_copy_rate": (round(rows_bytes / (rows_us * 1e-6) / COPY_RATE, 3) if 4 * n * n > INFINITY_CACHE
                                           else "cache-resident")}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
