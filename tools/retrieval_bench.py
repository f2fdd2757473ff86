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
first's.

`--verification`: device time of the verification histogram walk (ops.verification_all_pairs, bins 1024 and 4096) next to the two
walks of ops.retrieval_first_positive at the same shape (the same GEMM under a minimum epilogue; `--floor-lib` names another
build of the library to take them from) and to ops.cross_distances + torch.histc where the matrix fits: verification_mode.
`--verification --contention`: the epilogue's terms priced one by one — a collapsed input whose pairs all share one bin, 64 / 1024 /
4096 bins at equal atomics, one flush per tile against one per walk: verification_contention_mode.

`--knn`: the streaming k-nearest-neighbour search (ops.knn_search) at the nq,n,e,k of `--knn-cases`, next to the matrix path
(ops.cross_distances + ops.topk_smallest) where its matrix fits and to one plain walk of the same shape: knn_mode."""
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


def _bind(path):
    """A second copy of the library (another build) next to the one the package loaded: every symbol the header declares and
    this build has, with its own event trace."""
    import ctypes
    from embeddingnet_amd import _lib
    l = ctypes.CDLL(path)
    for name, (res, argtypes) in _lib.parse_header().items():
        if hasattr(l, name):
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, argtypes
    return l


def _trace_us(l, fn):
    """{kernel: device microseconds} of one call of fn under library l's event trace."""
    import ctypes
    l.embnet_trace_enable(1)
    l.embnet_trace_reset()
    fn()
    torch.cuda.synchronize()
    name = ctypes.create_string_buffer(160)
    ms, work, unit, nbytes = ctypes.c_float(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
    per = {}
    for i in range(l.embnet_trace_count()):
        l.embnet_trace_get(i, ctypes.addressof(name), 160, ctypes.addressof(ms), ctypes.addressof(work), ctypes.addressof(unit),
                           ctypes.addressof(nbytes))
        per[name.value.decode().split("::")[-1]] = round(1e3 * ms.value, 1)
    l.embnet_trace_enable(0)
    l.embnet_trace_reset()
    return per


def verification_mode(args):
    """ops.verification_all_pairs (bins 1024 and 4096, leave-one-out, shuffled labels: nothing for a label filter to skip) next to
      (a) the two walks of embnet_retrieval_first_positive at the same shape — the same GEMM under a minimum epilogue (pass 1: a
          64-bit minimum per row, pass 2: a count per row) — from `--floor-lib` (a build of another commit) when given, else
          from the loaded library; per-kernel device time from that library's event trace
      (b) ops.cross_distances(squared) + torch.histc per label class, where the [n, n] matrix fits: wall time between events
    the legs alternating round by round in one process; the medians of `--rounds` traced calls."""
    from embeddingnet_amd import _lib, ops
    from embeddingnet_amd._lib import ptr, stream
    dev = torch.device("cuda:0")
    cur = _lib.lib()
    floor = _bind(args.floor_lib) if args.floor_lib else cur

    def first(x, labels, ws, outs):
        n, e = x.shape
        rc = floor.embnet_retrieval_first_positive(ptr(x), ptr(labels), n, ptr(x), ptr(labels), n, e, 1, ptr(outs[0]), ptr(outs[1]),
                                                   ptr(outs[2]), ptr(ws), ws.numel() * 8, stream())
        assert rc == 0, floor.embnet_last_error()

    def composed(x, labels, bins):
        d = ops.cross_distances(x, x, squared=True)
        same = labels[:, None] == labels[None, :]
        hs = torch.histc(d[same], bins=bins, min=0.0, max=4.0)
        ho = torch.histc(d[~same], bins=bins, min=0.0, max=4.0)
        return hs, ho

    warm, wl = clustered(512, 64, dev, "shuffled")
    ops.verification_all_pairs(warm, wl, bins=1024), composed(warm, wl, 1024)
    results = []
    for e in args.dims:
        for n in args.sizes:
            x, labels = clustered(n, e, dev, "shuffled")
            ws = torch.empty(max(floor.embnet_retrieval_workspace_bytes(n, n) // 8, 2), dtype=torch.float64, device=dev)
            outs = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                    torch.empty(n, device=dev))
            both = 4.0 * n * n <= args.max_matrix_gib * 2 ** 30 / 3      # the two masked copies besides the matrix
            run_v = {b: (lambda b=b: ops.verification_all_pairs(x, labels, bins=b, d2_max=4.0)) for b in (1024, 4096)}
            run_f = lambda: first(x, labels, ws, outs)
            run_f(), [r() for r in run_v.values()]
            t_v, t_f1, t_f2, t_c, t_prep = {1024: [], 4096: []}, [], [], {1024: [], 4096: []}, []
            for _ in range(args.rounds):
                for b in (1024, 4096):
                    per = _trace_us(cur, run_v[b])
                    t_v[b].append(per["verif_walk_kernel"])
                    t_prep.append(per["verif_prep_kernel"])
                    per = _trace_us(floor, run_f)
                    t_f1.append(per["retrieval_walk_kernel<1>"])
                    t_f2.append(per["retrieval_walk_kernel<2>"])
                    if both:
                        t_c[b].append(1e3 * timed(lambda: composed(x, labels, b))[0])
                        torch.cuda.empty_cache()
            hs, ho = run_v[4096]()
            f1, f2 = float(np.median(t_f1)), float(np.median(t_f2))
            tile = 128 if ((n + 127) // 128) ** 2 >= 384 else 64
            res = {"mode": "verification", "n": n, "e": e, "tile": tile, "label_order": "shuffled", "leave_one_out": True,
                   "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "floor_lib": args.floor_lib or "loaded library",
                   "floor_pass1_us": round(f1, 1), "floor_pass1_us_min_max": [min(t_f1), max(t_f1)],
                   "floor_pass2_us": round(f2, 1), "floor_pass2_us_min_max": [min(t_f2), max(t_f2)],
                   "prep_us": round(float(np.median(t_prep)), 1), "pairs": int((hs.sum() + ho.sum()).item()),
                   "same_pairs": int(hs.sum().item())}
            for b in (1024, 4096):
                v = float(np.median(t_v[b]))
                res.update({f"walk_us_{b}": round(v, 1), f"walk_us_{b}_min_max": [min(t_v[b]), max(t_v[b])],
                            f"walk_{b}_over_pass1": round(v / f1, 3), f"walk_{b}_over_pass2": round(v / f2, 3),
                            f"walk_{b}_tflops": round(2.0 * n * n * e / (v * 1e-6) / 1e12, 2)})
                if both:
                    c = float(np.median(t_c[b]))
                    res.update({f"composed_us_{b}": round(c, 1), f"walk_{b}_over_composed": round(v / c, 4)})
            print(json.dumps(res), flush=True)
            results.append(res)
            del x, labels, ws, outs
            torch.cuda.empty_cache()
    return results


def verification_contention_mode(args):
    """What the histogram epilogue costs beyond the walk, term by term (device µs of verif_walk_kernel, median of `--rounds`):
      collapsed   every row the same unit vector up to 1e-4 of noise: all d2 fall into bin 0, so the 64 LDS atomics of a wave
                  instruction aim at one address (two with mixed labels) — the worst case for same-address LDS atomics; next to
                  the clustered input of the same shape, whose d2 spreads over many bins
      bins        64 / 1024 / 4096 on the clustered input: the same atomics, a growing clear + scan + flush per workgroup
      flush       flush_tiles = 1 against 0 (one flush per walk): the price of one flush per gallery tile, divided by the number
                  of extra flushes a workgroup does (tiles_per_split - 1, from the library's plan)"""
    from embeddingnet_amd import _lib, ops
    dev = torch.device("cuda:0")
    cur = _lib.lib()

    def walk_us(x, labels, bins, flush_tiles=0):
        run = lambda: ops.verification_all_pairs(x, labels, bins=bins, d2_max=4.0, flush_tiles=flush_tiles)
        run()
        t = [_trace_us(cur, run)["verif_walk_kernel"] for _ in range(args.rounds)]
        return round(float(np.median(t)), 1), [min(t), max(t)]

    def plan(n):
        big = ((n + 127) // 128) ** 2 >= 384
        b = 128 if big else 64
        tiles = (n + b - 1) // b
        want = min(-(-512 // tiles), tiles)
        return b, -(-tiles // want)

    results = []
    for e in args.dims:
        for n in args.sizes:
            x, labels = clustered(n, e, dev, "shuffled")
            g = torch.Generator(device=dev).manual_seed(1)
            c = torch.randn(1, e, device=dev, generator=g) + 1e-4 * torch.randn(n, e, device=dev, generator=g)
            c = (c / c.norm(dim=1, keepdim=True)).contiguous()
            tile, tps = plan(n)
            res = {"mode": "verification_contention", "n": n, "e": e, "tile": tile, "tiles_per_split": tps,
                   "device": torch.cuda.get_device_name(dev), "rounds": args.rounds}
            hs, ho = ops.verification_all_pairs(c, labels, bins=4096, d2_max=4.0)
            res["collapsed_share_in_bin0"] = round(float((hs[0] + ho[0]).item()) / float((hs.sum() + ho.sum()).item()), 4)
            for bins in (64, 1024, 4096):
                res[f"clustered_us_{bins}"], res[f"clustered_us_{bins}_min_max"] = walk_us(x, labels, bins)
                res[f"collapsed_us_{bins}"], res[f"collapsed_us_{bins}_min_max"] = walk_us(c, labels, bins)
                res[f"collapsed_over_clustered_{bins}"] = round(res[f"collapsed_us_{bins}"] / res[f"clustered_us_{bins}"], 3)
            for bins in (1024, 4096):
                every, _ = walk_us(x, labels, bins, flush_tiles=1)
                res[f"flush_every_tile_us_{bins}"] = every
                if tps > 1:
                    res[f"us_per_extra_flush_{bins}"] = round((every - res[f"clustered_us_{bins}"]) / (tps - 1), 3)
            print(json.dumps(res), flush=True)
            results.append(res)
            del x, labels, c
            torch.cuda.empty_cache()
    return results


def knn_mode(args):
    """ops.knn_search (the top-k epilogue on the distance walk, select 'all') at each nq,n,e,k of `--knn-cases`, next to
      (a) matrix_ms   ops.cross_distances(squared) + ops.topk_smallest(k) — what KNNClassifier(algorithm='matrix') runs — where
                      k <= 64 and the [nq, n] fp32 matrix is at most `--max-matrix-gib`: wall time between events
      (b) floor_us    ONE plain walk at the same shape: the counting pass of ops.retrieval_first_positive
                      (retrieval_walk_kernel<2>: every tile, an integer count per row) on shuffled labels — the floor of what any
                      epilogue on this walk can reach; it runs on the plan's own tiles (128x128 where they fill the chip), the
                      search on 64x64: `floor_tile`
    the legs alternating round by round in one process; medians of `--rounds`.  stream_ms: wall time between events around the
    whole call (norms, walk, merge; workspace and outputs allocated inside); walk_us / merge_us / floor_us: device time of the
    kernels from the library's event trace."""
    from embeddingnet_amd import _lib, ops
    dev = torch.device("cuda:0")
    cur = _lib.lib()
    warm, wl = clustered(512, 64, dev, "shuffled")
    ops.knn_search(warm, warm, 10), ops.topk_smallest(ops.cross_distances(warm, warm, squared=True), 10)
    ops.retrieval_first_positive(warm, wl, warm, wl)
    results = []
    for nq, n, e, k in args.knn_cases:
        x, xl = clustered(n, e, dev, "shuffled")
        q, ql = clustered(nq, e, dev, "shuffled", seed=1)
        both = k <= 64 and 4.0 * nq * n <= args.max_matrix_gib * 2 ** 30
        run_s = lambda: ops.knn_search(q, x, k)
        run_m = lambda: ops.topk_smallest(ops.cross_distances(q, x, squared=True), k)
        run_f = lambda: ops.retrieval_first_positive(q, ql, x, xl)
        run_s(), run_f()
        if both:
            run_m()
            torch.cuda.empty_cache()
        t_s, t_m, t_w, t_g, t_f = [], [], [], [], []
        for _ in range(args.rounds):
            t_s.append(timed(run_s)[0])
            if both:
                t_m.append(timed(run_m)[0])
                torch.cuda.empty_cache()
            per = _trace_us(cur, run_s)
            t_w.append(per["knn_walk_kernel"])
            t_g.append(per["knn_merge_kernel"])
            t_f.append(_trace_us(cur, run_f)["retrieval_walk_kernel<2>"])
        s_ms, w_us, f_us = float(np.median(t_s)), float(np.median(t_w)), float(np.median(t_f))
        flop = 2.0 * nq * n * e
        tiles_m = -(-nq // 64)
        want = min(-(-512 // tiles_m), -(-n // 64))
        tps = -(-(-(-n // 64)) // want)
        res = {"mode": "knn", "nq": nq, "n": n, "e": e, "k": k, "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
               "splits": -(-(-(-n // 64)) // tps), "tiles_per_split": tps,
               "stream_ms": round(s_ms, 3), "stream_ms_min_max": [round(min(t_s), 3), round(max(t_s), 3)],
               "walk_us": round(w_us, 1), "walk_us_min_max": [min(t_w), max(t_w)], "merge_us": round(float(np.median(t_g)), 1),
               "walk_tflops": round(flop / (w_us * 1e-6) / 1e12, 2), "walk_share_of_peak": round(flop / (w_us * 1e-6) / PEAK, 3),
               "floor_us": round(f_us, 1), "floor_us_min_max": [min(t_f), max(t_f)],
               "floor_tile": 128 if (-(-nq // 128)) * (-(-n // 128)) >= 384 else 64, "walk_over_floor": round(w_us / f_us, 3),
               "matrix_gib": round(4.0 * nq * n / 2 ** 30, 2)}
        if both:
            m_ms = float(np.median(t_m))
            res.update({"matrix_ms": round(m_ms, 3), "matrix_ms_min_max": [round(min(t_m), 3), round(max(t_m), 3)],
                        "stream_over_matrix": round(s_ms / m_ms, 3)})
        print(json.dumps(res), flush=True)
        results.append(res)
        del x, xl, q, ql
        torch.cuda.empty_cache()
    return results


def _knn_case(text):
    nq, n, e, k = (int(v) for v in text.split(","))
    return nq, n, e, k


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
    ap.add_argument("--verification", action="store_true", help="time the verification histogram walk (see verification_mode)")
    ap.add_argument("--contention", action="store_true",
                    help="--verification: price the epilogue's terms instead (see verification_contention_mode)")
    ap.add_argument("--floor-lib", default=None, help="--verification: another build of libembnet_hip.so for the floor leg")
    ap.add_argument("--knn", action="store_true", help="time the streaming k-nearest-neighbour search (see knn_mode)")
    ap.add_argument("--knn-cases", type=_knn_case, nargs="+", metavar="NQ,N,E,K",
                    default=[(2048, 32768, 256, 10), (2048, 32768, 256, 64), (2048, 32768, 256, 128), (32768, 32768, 256, 10),
                             (8192, 262144, 512, 10), (8192, 262144, 512, 128), (50000, 262144, 512, 10)])
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    if args.knn:
        return write_out(args, knn_mode(args))
    if args.verification:
        return write_out(args, verification_contention_mode(args) if args.contention else verification_mode(args))
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
