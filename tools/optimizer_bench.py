#!/usr/bin/env python3
"""The optimizer update as a hot path of its own: device time of one step over ResNet18's parameter list (62 tensors, 11.3 M
floats, the kernels with their l2 regulariser) plus a [1000, 256] proxy tensor, rule 'adam', four legs through the C ABI:

  opt_parent      embnet_optimizer_step                       (the one-group update: the yardstick)
  opt_groups      embnet_optimizer_step_groups, three groups (kernels / other / proxies at 100 x the rate), no option
  opt_clipvalue   the same with clipvalue
  opt_clipnorm    embnet_optimizer_grad_norm + the same with the norm's scale        (two launches)

and three for the averaged weights (csrc/weight_average.hip) over the same tensors and the same chunk list:

  opt_sgd         embnet_optimizer_step, rule 'sgd'           (12 B per element: the yardstick of the next leg)
  average_update  embnet_weight_average_update, c = 1e-3      (12 B per element)
  average_swap    embnet_weight_average_swap                  (16 B per element)

and the layer-wise adaptive rules (csrc/layerwise.hip), three groups, 'other' exempt, two launches per step, each also alone:

  lars, lamb                embnet_optimizer_layerwise_norms + embnet_optimizer_layerwise_step   (8 + 20 and 24 + 16 B per element)
  lars_norms, lamb_norms    the norms launch alone (its last workgroup adds every tensor's partials)
  lars_step, lamb_step      the update alone, at the trust ratios the last norms launch left

  python tools/optimizer_bench.py [--rounds 15] [--reps 20] [--json out.json]          (GPU box)

All legs run in one process on the same table, in alternating rounds of `reps` back-to-back steps timed with events (a step is
~100 us of device time against a few us of launch cost, so the device is the limiter); reported per leg: the median, minimum and
maximum over the rounds in microseconds, and the algorithmic bytes (28 B per element for 'adam'; the norm pass adds 4 B per
element, 8 B where a tensor has l2) over the median as TB/s.  The spread of the parent's rounds is the margin a leg is read
against."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from embeddingnet_amd import _lib  # noqa: E402
from embeddingnet_amd._lib import check  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd import layers as L
    from embeddingnet_amd.optimizers import KerasOptimizer
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    base, _ = B.get_backbone((224, 224, 3), encodings_len=256, backbone_name="resnet18", backbone_weights=None, seed=0, device=dev)
    ps = [p for p in base.parameters() if p.requires_grad]
    proxies = torch.nn.Parameter(torch.randn(1000, 256, device=dev))
    opt = KerasOptimizer([dict(params=[p for p in ps if p.dim() >= 2]), dict(params=[p for p in ps if p.dim() < 2]),
                          dict(params=[proxies], lr_mult=100.0)], "adam", 1e-4)
    l2 = L.regularized_kernels(base)
    opt.set_l2(l2)
    gen = torch.Generator(device=dev).manual_seed(0)
    for p in opt._tensors:
        p.grad = 1e-2 * torch.randn(p.shape, device=dev, generator=gen)
    opt._build_table()
    norm, ws = opt._norm_buffers()
    n_elem = sum(p.numel() for p in opt._tensors)
    n_l2 = sum(p.numel() for p, _ in l2)
    table, n, chunks, n_chunks = opt._table.data_ptr(), len(opt._tensors), opt._chunks.data_ptr(), opt._chunks.shape[0]
    lr, b1, b2, eps = 1e-4, 0.9, 0.999, 1e-7
    c1 = lr * np.sqrt(1 - b2 ** 10) / (1 - b1 ** 10)
    rows = np.asarray([[lr, c1, 0, 0], [lr, c1, 0, 0], [100 * lr, 100 * c1, 0, 0]], dtype=np.float32)
    stream = _lib.stream()

    def groups(clipvalue=0.0, scale=None):
        check(lib.embnet_optimizer_step_groups(2, table, n, chunks, n_chunks, rows.ctypes.data, 3, b1, b2, eps, 0.0, 0.0, 0, clipvalue,
                                               scale, None, None, stream))

    def clipnorm():
        check(lib.embnet_optimizer_grad_norm(table, n, chunks, n_chunks, 10.0, ws.data_ptr(), ws.numel() * 8, norm.data_ptr(),
                                             norm.data_ptr() + 16, stream))
        groups(scale=norm.data_ptr() + 16)

    legs = {"opt_parent": lambda: check(lib.embnet_optimizer_step(2, table, n, chunks, n_chunks, lr, b1, b2, eps, c1, 0.0, None, stream)),
            "opt_groups": groups, "opt_clipvalue": lambda: groups(clipvalue=10.0), "opt_clipnorm": clipnorm}
    nbytes = {k: 28.0 * n_elem for k in legs}
    nbytes["opt_clipnorm"] += 4.0 * n_elem + 4.0 * n_l2
    # the averaged copies of the same tensors: { w, avg, n, 0 } rows over the optimizer's chunk list
    averages = [p.detach().clone() for p in opt._tensors]
    avg_rows = [(p.data_ptr(), v.data_ptr(), p.numel(), 0) for p, v in zip(opt._tensors, averages)]
    avg_table = torch.from_numpy(np.asarray(avg_rows, dtype=np.uint64).view(np.int64)).to(dev)
    legs["opt_sgd"] = lambda: check(lib.embnet_optimizer_step(0, table, n, chunks, n_chunks, lr, 0.0, 0.0, eps, 0.0, 0.0, None, stream))
    legs["average_update"] = lambda: check(lib.embnet_weight_average_update(avg_table.data_ptr(), n, chunks, n_chunks, 1e-3, None, stream))
    legs["average_swap"] = lambda: check(lib.embnet_weight_average_swap(avg_table.data_ptr(), n, chunks, n_chunks, stream))
    nbytes.update(opt_sgd=12.0 * n_elem, average_update=12.0 * n_elem, average_swap=16.0 * n_elem)
    # the layer-wise rules over the same table and groups ('other' exempt): the norms launch, then the update
    lw_rows = np.asarray([[lr, 0, 1e-4, 1e-3], [lr, 0, 0, 0], [100 * lr, 0, 0, 1e-3]], dtype=np.float32)
    stats = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    lw_bytes = lib.embnet_optimizer_layerwise_workspace_bytes(n_chunks)
    lw_ws = torch.zeros(-(-lw_bytes // 8), dtype=torch.float64, device=dev)          # (the ticket in front: zero once)

    def layerwise(code, momentum, norms=True, step=True):
        if norms:
            check(lib.embnet_optimizer_layerwise_norms(code, table, n, chunks, n_chunks, lw_rows.ctypes.data, 3, b1, b2, eps, 1.5, 1.01,
                                                       0.0, None, None, None, lw_ws.data_ptr(), lw_ws.numel() * 8, stats.data_ptr(), stream))
        if step:
            check(lib.embnet_optimizer_layerwise_step(code, table, n, chunks, n_chunks, lw_rows.ctypes.data, 3, b1, b2, eps, 1.5, 1.01,
                                                      momentum, 0, 0.0, None, None, None, stats.data_ptr(), stream))

    legs.update(lars=lambda: layerwise(0, 0.9), lars_norms=lambda: layerwise(0, 0.9, step=False),
                lars_step=lambda: layerwise(0, 0.9, norms=False), lamb=lambda: layerwise(1, 0.0),
                lamb_norms=lambda: layerwise(1, 0.0, step=False), lamb_step=lambda: layerwise(1, 0.0, norms=False))
    nbytes.update(lars=28.0 * n_elem, lars_norms=8.0 * n_elem, lars_step=20.0 * n_elem, lamb=40.0 * n_elem, lamb_norms=24.0 * n_elem,
                  lamb_step=16.0 * n_elem)
    times = {k: [] for k in legs}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            t0.record()
            for _ in range(a.reps):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(1e3 * t0.elapsed_time(t1) / a.reps)
    out = dict(tensors=n, elements=n_elem, l2_elements=n_l2, chunks=n_chunks, rounds=a.rounds, reps=a.reps, legs={})
    for name, v in times.items():
        med = sorted(v)[len(v) // 2]
        out["legs"][name] = dict(us_median=round(med, 2), us_min=round(min(v), 2), us_max=round(max(v), 2),
                                 tb_per_s=round(nbytes[name] / med * 1e-6, 3))
    print(json.dumps(out))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
