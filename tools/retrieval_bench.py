#!/usr/bin/env python3
"""Retrieval evaluation (embeddingnet_amd/retrieval.py, csrc/retrieval.hip): time of the fused rank computation per size, next
to the materialising path where its matrix fits.

For each (n, e) in `--sizes` x `--dims` (default 6 100, 32 768, 131 072, 262 144 x 256, 512), on clustered unit-norm rows
generated from a seed on the device, leave-one-out:
  fused_ms            device events around ops.retrieval_first_positive (norms + reset, two walks of the distance GEMM, finish)
                      + ops.retrieval_reduce; workspace and outputs allocated inside, as a caller would; one untimed warm-up,
                      median of `--rounds` (>= 3)
  materialised_ms     ops.cross_distances(squared) + ops.topk_smallest(k = 10) at the sizes where the [n, n] fp32 matrix is at
                      most `--max-matrix-gib` (6 100 and 32 768), in the same process, the two paths alternating round by round
  *_tflops            2 n^2 e / t — the ALGORITHMIC work of one distance matrix over the path's time, and its share of the
                      157.3 TFLOP/s fp32 MFMA peak
  fused_gemm_passes   how many times the fused path executes that GEMM: 1 (the counting pass, every tile) + the share of tile
                      pairs whose label filters overlap, which is all that the nearest-positive pass visits — counted here
                      from the labels with the library's filter (1 024 bits per tile, bit = label * 2654435761 >> 22)
  fused_kernel_us     per-kernel device time from the library's event trace, in a separate traced call
Every size runs with the labels grouped by class (how encodings are produced: the nearest-positive pass is a sliver) and in
shuffled order (nothing can be skipped: two full passes).
Prints one JSON line per case; `--out` also writes the list to a file.

`--map`: the same table for ops.retrieval_positive_ranks + ops.retrieval_map_reduce (MAP@R / R-precision: the position of every
positive), for classes of `--per-class` members (default 20 and 512), next to
  (a) first_ms          ops.retrieval_first_positive + ops.retrieval_reduce at the same size — the same two GEMM walks without the
                        key stores, the sort, the binary searches and the histogram atomics: the floor
  (b) materialised_ms   ops.cross_distances(squared) + torch.sort(dim=1) + a gather of the labels, where the matrix fits
the three alternating round by round in one process; `pass2_over_counting` = device time of map_walk_kernel<2> over that of
retrieval_walk_kernel<2> from the library's event trace — what counting EVERY positive's negatives costs over counting the
first's."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK = 157.3e12


def gemm_passes(labels, n):
    """1 + the share of (query tile, gallery tile) pairs that pass 1 visits, from the library's tile choice and label filter."""
    tile = 128 if ((n + 127) // 128) ** 2 >= 384 else 64
    tiles = (n + tile - 1) // tile
    bit = ((labels.to(torch.int64) & 0xffffffff) * 2654435761 & 0xffffffff) >> 22
    f = torch.zeros(tiles, 1024, dtype=torch.float16, device=labels.device)
    f[torch.arange(n, device=labels.device) // tile, bit] = 1
    live = 0
    for i in range(0, tiles, 512):                         # [512, tiles] blocks of the tile-pair overlap matrix
        live += int(((f[i:i + 512] @ f.T) > 0).sum().item())
    return round(1.0 + live / float(tiles * tiles), 3)


def clustered(n, e, dev, order="grouped", per_class=16, seed=0):
    """Non-negative unit rows around class centres (the recipe of the tests' galleries, sigma 1.2), 16 per class.  order
    'grouped': class by class, as encodings are produced; 'shuffled': rows in random order."""
    g = torch.Generator(device=dev).manual_seed(seed)
    classes = max(n // per_class, 1)
    centres = torch.randn(classes, e, device=dev, generator=g).abs()
    labels = torch.clamp(torch.arange(n, device=dev) // per_class, max=classes - 1)
    if order == "shuffled":
        labels = labels[torch.randperm(n, device=dev, generator=g)]
    x = (centres[labels] + 1.2 * torch.randn(n, e, device=dev, generator=g)).abs()
    return (x / x.norm(dim=1, keepdim=True)).contiguous(), labels.to(torch.int32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def map_mode(args):
    from embeddingnet_amd import _lib, ops
    dev = torch.device("cuda:0")
    ks = torch.tensor([1, 10, 100, 1000], dtype=torch.int32, device=dev)

    def positions(x, labels, classes, capacity):
        offset, _, pos_rank = ops.retrieval_positive_ranks(x, labels, num_classes=classes, capacity=capacity)
        return ops.retrieval_map_reduce(offset, pos_rank)

    def first(x, labels):
        rank, _, _ = ops.retrieval_first_positive(x, labels)
        return ops.retrieval_reduce(rank, ks)

    def materialised(x, labels):
        d = ops.cross_distances(x, x, squared=True)
        d.fill_diagonal_(float("inf"))
        order = torch.sort(d, dim=1).indices
        del d
        return (labels[order] == labels[:, None]).nonzero()

    def traced(fn, kernel):
        _lib.trace_enable(True)
        _lib.trace_reset()
        fn()
        torch.cuda.synchronize()
        per = {}
        for name, ms, _, _, _ in _lib.trace_records():
            per[name.split("::")[-1]] = round(1e3 * ms, 1)
        _lib.trace_enable(False)
        _lib.trace_reset()
        return per, per[kernel]

    warm, wl = clustered(512, 64, dev)
    positions(warm, wl, 32, 512 * 15), first(warm, wl), materialised(warm, wl)
    results = []
    for e in args.dims:
        for n, per_class, order in [(n, c, o) for n in args.sizes for c in args.per_class for o in ("grouped", "shuffled")]:
            x, labels = clustered(n, e, dev, order, per_class=per_class)
            classes = max(n // per_class, 1)
            capacity = int((torch.bincount(labels.long(), minlength=classes)[labels.long()] - 1).sum().item())
            both = 4.0 * n * n <= args.max_matrix_gib * 2 ** 30           # (the sort adds a copy and 8-byte indices: 4x that)
            run_p, run_f, run_m = (lambda: positions(x, labels, classes, capacity)), (lambda: first(x, labels)), (lambda: materialised(x, labels))
            run_p(), run_f()
            if both:
                run_m()
            t_p, t_f, t_m, out = [], [], [], None
            for _ in range(args.rounds):
                ms, out = timed(run_p)
                t_p.append(ms)
                t_f.append(timed(run_f)[0])
                if both:
                    t_m.append(timed(run_m)[0])
                    torch.cuda.empty_cache()
            per, walk2 = traced(run_p, "map_walk_kernel<2>")
            _, count2 = traced(run_f, "retrieval_walk_kernel<2>")
            sums, n_valid = out[3].cpu().numpy(), int(out[4].item())
            p_ms, f_ms = float(np.median(t_p)), float(np.median(t_f))
            res = {"mode": "map", "n": n, "e": e, "per_class": per_class, "label_order": order, "positives": capacity,
                   "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "leave_one_out": True,
                   "map_ms": round(p_ms, 3), "map_ms_min_max": [round(min(t_p), 3), round(max(t_p), 3)],
                   "first_ms": round(f_ms, 3), "first_ms_min_max": [round(min(t_f), 3), round(max(t_f), 3)],
                   "map_over_first": round(p_ms / f_ms, 3), "pass2_over_counting": round(walk2 / count2, 3),
                   "map_kernel_us": per, "map_at_r": round(float(sums[0]) / n_valid, 4), "r_precision": round(float(sums[1]) / n_valid, 4)}
            if both:
                m_ms = float(np.median(t_m))
                res.update({"materialised_ms": round(m_ms, 3), "materialised_ms_min_max": [round(min(t_m), 3), round(max(t_m), 3)],
                            "map_over_materialised": round(p_ms / m_ms, 3)})
            print(json.dumps(res), flush=True)
            results.append(res)
            del x, labels
            torch.cuda.empty_cache()
    return results


def write_out(args, results):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[6100, 32768, 131072, 262144])
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-matrix-gib", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--map", action="store_true", help="time the MAP@R primitive (see the module docstring)")
    ap.add_argument("--per-class", type=int, nargs="+", default=[20, 512], help="--map: members per class")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if args.map:
        if args.sizes == ap.get_default("sizes"):
            args.sizes = [6100, 32768, 131072]
        return write_out(args, map_mode(args))
    from embeddingnet_amd import _lib, ops
    dev = torch.device("cuda:0")
    ks = torch.tensor([1, 10, 100, 1000], dtype=torch.int32, device=dev)

    def fused(x, labels):
        rank, _, _ = ops.retrieval_first_positive(x, labels)
        return ops.retrieval_reduce(rank, ks)

    def materialised(x):
        d = ops.cross_distances(x, x, squared=True)
        return ops.topk_smallest(d, 10)

    warm, wl = clustered(512, 64, dev)
    fused(warm, wl), materialised(warm)                    # code objects, torch's allocator
    results = []
    for e in args.dims:
        for n, order in [(n, o) for n in args.sizes for o in ("grouped", "shuffled")]:
            x, labels = clustered(n, e, dev, order)
            both = 4.0 * n * n <= args.max_matrix_gib * 2 ** 30
            fused(x, labels)
            if both:
                materialised(x)
            t_f, t_m, hits = [], [], None
            for _ in range(args.rounds):
                ms, (hits, n_valid, _) = timed(lambda: fused(x, labels))
                t_f.append(ms)
                if both:
                    t_m.append(timed(lambda: materialised(x))[0])
            _lib.trace_enable(True)
            _lib.trace_reset()
            fused(x, labels)
            torch.cuda.synchronize()
            per = {}
            for name, ms, _, _, _ in _lib.trace_records():
                per[name.split("::")[-1]] = round(1e3 * ms, 1)
            _lib.trace_enable(False)
            _lib.trace_reset()
            flop = 2.0 * n * n * e
            f_ms = float(np.median(t_f))
            res = {"n": n, "e": e, "label_order": order, "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "leave_one_out": True,
                   "fused_ms": round(f_ms, 3), "fused_ms_min_max": [round(min(t_f), 3), round(max(t_f), 3)],
                   "fused_gemm_passes": gemm_passes(labels, n), "fused_tflops": round(flop / (f_ms * 1e-3) / 1e12, 2),
                   "fused_share_of_peak": round(flop / (f_ms * 1e-3) / PEAK, 3),
                   "fused_kernel_us": per, "recall_at_1_10_100_1000": [round(float(h) / int(n_valid), 4) for h in hits.cpu()],
                   "matrix_gib_avoided": round(4.0 * n * n / 2 ** 30, 2)}
            if both:
                m_ms = float(np.median(t_m))
                res.update({"materialised_ms": round(m_ms, 3), "materialised_ms_min_max": [round(min(t_m), 3), round(max(t_m), 3)],
                            "materialised_gemm_passes": 1, "materialised_tflops": round(flop / (m_ms * 1e-3) / 1e12, 2),
                            "materialised_share_of_peak": round(flop / (m_ms * 1e-3) / PEAK, 3),
                            "fused_over_materialised": round(f_ms / m_ms, 3)})
            print(json.dumps(res), flush=True)
            results.append(res)
            del x, labels
            torch.cuda.empty_cache()
    write_out(args, results)


if __name__ == "__main__":
    main()
