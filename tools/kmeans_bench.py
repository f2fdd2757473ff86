#!/usr/bin/env python3
"""k-means on encodings (embeddingnet_amd/kmeans.py, csrc/kmeans.hip): time of one assign pass, one centre update and a whole
fit, on clustered unit-norm rows generated from a seed on the device (default n = 65 536, e = 512, k = 1 024).

  assign_ms / update_ms   device events around ops.kmeans_assign / ops.kmeans_update with a workspace held by the caller, as a
                          fit does; one untimed warm-up, median and minimum of `--rounds`
  assign_kernel_us        device time of kmeans_assign_kernel from the library's event trace, next to
  counting_kernel_us      that of retrieval_walk_kernel<2> inside ops.retrieval_first_positive at the same nq, gallery size and e
                          — the same walk of the distance GEMM with an integer count where the assign pass keeps a 64-bit
                          minimum.  The two legs alternate round by round in one process; `assign_over_counting` is the
                          ratio of the medians
  assign_tflops           2 n k e / kernel time, and its share of the 157.3 TFLOP/s fp32 MFMA peak
  update_gbs              4 n e bytes (one read of x) / update time
  fit_ms, fit_n_iter      KMeans(k, init=<rows of x>, max_iter=--max-iter).fit wall time including its host reads
  sklearn_fit_ms          scikit-learn KMeans(algorithm='lloyd', tol=0, the same init and max_iter) on the host's cores, when
                          scikit-learn is installed (null otherwise) — recorded, not compared against a threshold
Prints one JSON line; `--out` also writes it to a file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK = 157.3e12


def clustered(n, e, k, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.randn(k, e, device=dev, generator=g)
    ids = torch.arange(n, device=dev) % k
    x = centres[ids] + 0.8 * torch.randn(n, e, device=dev, generator=g)
    return torch.nn.functional.normalize(x, dim=1).contiguous(), ids.to(torch.int32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def traced(fn, kernel):
    from embeddingnet_amd import _lib
    _lib.trace_reset()
    _lib.trace_enable(True)
    fn()
    torch.cuda.synchronize()
    rec = _lib.trace_records()
    _lib.trace_enable(False)
    return sum(ms for name, ms, *_ in rec if name == kernel) * 1e3


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--e", type=int, default=512)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from embeddingnet_amd import ops
    from embeddingnet_amd.kmeans import KMeans
    dev = torch.device("cuda:0")
    n, e, k = args.n, args.e, args.k
    x, ids = clustered(n, e, k, dev)
    init = x[torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:k]].contiguous()
    ws = ops.kmeans_workspace(n, k, e, x)
    labels = ops.kmeans_assign(x, init, ws=ws)[0]
    ops.kmeans_update(x, labels, init, ws=ws)
    ops.retrieval_first_positive(x, ids, init, ids[:k].contiguous())
    torch.cuda.synchronize()
    assign_ms, update_ms, assign_us, counting_us = [], [], [], []
    for _ in range(max(args.rounds, 3)):
        assign_ms.append(timed(lambda: ops.kmeans_assign(x, init, labels, ws=ws, reuse_point_norms=True))[0])
        update_ms.append(timed(lambda: ops.kmeans_update(x, labels, init, ws=ws))[0])
        assign_us.append(traced(lambda: ops.kmeans_assign(x, init, labels, ws=ws, reuse_point_norms=True),
                                "embnet::kmeans_assign_kernel"))
        counting_us.append(traced(lambda: ops.retrieval_first_positive(x, ids, init, ids[:k].contiguous()),
                                  "embnet::retrieval_walk_kernel<2>"))
    t0 = time.perf_counter()
    km = KMeans(k, init=init, max_iter=args.max_iter, device=dev).fit(x)
    torch.cuda.synchronize()
    fit_ms = (time.perf_counter() - t0) * 1e3
    out = {"n": n, "e": e, "k": k, "rounds": max(args.rounds, 3),
           "assign_ms": stats(assign_ms), "update_ms": stats(update_ms),
           "assign_kernel_us": stats(assign_us), "counting_kernel_us": stats(counting_us),
           "assign_over_counting": round(float(np.median(assign_us) / np.median(counting_us)), 4),
           "assign_tflops": round(2.0 * n * k * e / (np.median(assign_us) * 1e-6) / 1e12, 2),
           "assign_share_of_fp32_mfma_peak": round(2.0 * n * k * e / (np.median(assign_us) * 1e-6) / PEAK, 4),
           "update_gbs": round(4.0 * n * e / (np.median(update_ms) * 1e-3) / 1e9, 1),
           "fit_ms": round(fit_ms, 2), "fit_n_iter": km.n_iter_, "fit_inertia": km.inertia_, "fit_n_empty": km.n_empty_,
           "sklearn_fit_ms": None, "sklearn_n_iter": None, "sklearn_inertia": None}
    if not args.no_sklearn:
        try:
            from sklearn.cluster import KMeans as SK
        except ImportError:
            SK = None
        if SK is not None:
            xh, ih = x.cpu().numpy(), init.cpu().numpy()
            t0 = time.perf_counter()
            sk = SK(k, init=ih, n_init=1, algorithm="lloyd", tol=0, max_iter=args.max_iter).fit(xh)
            out.update(sklearn_fit_ms=round((time.perf_counter() - t0) * 1e3, 1), sklearn_n_iter=int(sk.n_iter_),
                       sklearn_inertia=float(sk.inertia_), host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or None)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
