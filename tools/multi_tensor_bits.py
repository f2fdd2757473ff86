#!/usr/bin/env python3
"""Bits of the multi-tensor launches (csrc/multi_tensor.h): fixed-seed inputs through the six entry points that take a descriptor
table and a chunk list, one SHA-256 per output tensor on stdout.  The tables and lists are built by hand here, as a caller of the
C ABI would (include/embnet.h), so the same file runs on any commit of ABI 22: two builds compute the same iff the listings are equal.

  python tools/multi_tensor_bits.py [--out listing.txt]          (GPU box, seconds)

Tensors of 1, 7, 4095, 4096, 4097 and 2*4096+13 elements (a tail, a whole chunk, a chunk and an element, two chunks and a tail),
one more placed one float into a larger buffer (not 16-byte aligned: the element-wise path), and for the optimizer entry points
one with a null gradient; for the planes a [3,3,16,32] and a [1,1,32,16] kernel, flip 0 and 1, in the build's plane format."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from embeddingnet_amd import _lib  # noqa: E402
from embeddingnet_amd._lib import check  # noqa: E402

SIZES = [1, 7, 4095, 4096, 4097, 2 * 4096 + 13, 4096 + 5]      # the last one sits one float into its buffer
UNALIGNED, NO_GRAD = 6, 2                                       # indices into SIZES
LINES = []


def emit(name, t):
    torch.cuda.synchronize()
    LINES.append(f"{hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}  {name}")


def u64(rows, dev):
    return torch.from_numpy(np.asarray(rows, dtype=np.uint64).view(np.int64)).to(dev)


def f32_word(f, hi=0):
    return int(np.float32(f).view(np.uint32)) | (hi << 32)


class Tensors:
    """One set of fp32 tensors of SIZES from a seeded generator; `again()` gives a bit copy of the set as first drawn."""

    def __init__(self, seed, dev, scale=1.0):
        g = torch.Generator().manual_seed(seed)
        self.host = [scale * torch.randn(n + 8, generator=g) for n in SIZES]
        self.dev = dev
        self.again()

    def again(self):
        self.bufs = [h.to(self.dev) for h in self.host]
        self.t = [b[1:1 + n] if i == UNALIGNED else b[:n] for i, (b, n) in enumerate(zip(self.bufs, SIZES))]
        assert self.t[UNALIGNED].data_ptr() % 16 == 4 and all(t.data_ptr() % 16 == 0 for t in self.t[:UNALIGNED])
        return self


def chunk_list(sizes, ce, dev):
    return torch.tensor([(i, c) for i, n in enumerate(sizes) for c in range(-(-n // ce))], dtype=torch.int32, device=dev)


def optimizer(lib, dev):
    ce = lib.embnet_optimizer_chunk_elems()
    chunks = chunk_list(SIZES, ce, dev)
    w, g, s1, s2 = Tensors(1, dev), Tensors(2, dev, 1e-2), Tensors(3, dev, 1e-2), Tensors(4, dev, 1e-4)
    for s in s2.host:
        s.abs_()                                               # the second-moment slot is never negative
    lr, b1, b2, eps, c1, c2 = 1e-3, 0.9, 0.999, 1e-7, 2.5e-3, 1.0 / (1.0 - 0.999 ** 7)
    coef = torch.tensor([lr, b1, b2, eps, c1, c2], dtype=torch.float32, device=dev)
    group_rows = np.asarray([[lr, c1, lr * 5e-4, 0], [100 * lr, 100 * c1, 0, 0], [3 * lr, 3 * c1, 3 * lr * 1e-2, 0]], dtype=np.float32)
    group_dev = torch.from_numpy(group_rows).to(dev)

    def table():
        for x in (w, g, s1, s2):
            x.again()
        rows = [(w.t[i].data_ptr(), 0 if i == NO_GRAD else g.t[i].data_ptr(), s1.t[i].data_ptr(), s2.t[i].data_ptr(), n,
                 f32_word(2 * 2e-4 if i % 2 else 0.0, i % 3)) for i, n in enumerate(SIZES)]
        return u64(rows, dev)

    def state(name):
        for k, x in (("w", w), ("slot1", s1), ("slot2", s2)):
            emit(f"{name} {k}", torch.cat(x.bufs))               # the whole buffers: a write outside a tensor shows too

    for rule in range(5):
        for on_dev in (0, 1):
            t = table()
            k = (0.0,) * 6 if on_dev else (lr, b1, b2, eps, c1, c2)
            check(lib.embnet_optimizer_step(rule, t.data_ptr(), len(SIZES), chunks.data_ptr(), chunks.shape[0], *k,
                                            coef.data_ptr() if on_dev else None, None))
            state(f"optimizer_step rule={rule} coef_dev={on_dev}")
    scale = torch.tensor([0.37], dtype=torch.float32, device=dev)
    for rule, nesterov in [(r, 0) for r in range(6)] + [(5, 1)]:
        momentum = 0.9 if rule == 5 else 0.0
        for opts in ("none", "decay+l2+clip_scale", "decay+l2+clipvalue", "group_dev"):
            t = table()
            rows = group_rows.copy()
            if opts == "none":
                rows[:, 2] = 0
            on_dev = opts == "group_dev"
            check(lib.embnet_optimizer_step_groups(rule, t.data_ptr(), len(SIZES), chunks.data_ptr(), chunks.shape[0], rows.ctypes.data, 3,
                                                   b1, b2, eps, c2, momentum, nesterov, 0.02 if opts == "decay+l2+clipvalue" else 0.0,
                                                   scale.data_ptr() if opts == "decay+l2+clip_scale" else None,
                                                   coef.data_ptr() if on_dev else None, group_dev.data_ptr() if on_dev else None, None))
            state(f"optimizer_step_groups rule={rule} nesterov={nesterov} options={opts}")
    t = table()
    nbytes = lib.embnet_optimizer_grad_norm_workspace_bytes(chunks.shape[0])
    ws = torch.zeros(-(-nbytes // 8), dtype=torch.float64, device=dev)
    norm = torch.zeros(4, dtype=torch.float64, device=dev)
    for clipnorm in (0.05, 1e3):
        for rep in range(2):                                     # the second launch finds the ticket as the first left it
            check(lib.embnet_optimizer_grad_norm(t.data_ptr(), len(SIZES), chunks.data_ptr(), chunks.shape[0], clipnorm, ws.data_ptr(),
                                                 ws.numel() * 8, norm.data_ptr(), norm.data_ptr() + 16, None))
            emit(f"optimizer_grad_norm clipnorm={clipnorm} launch={rep} norm words and scale", norm)
    emit("optimizer_grad_norm weights untouched", torch.cat(w.bufs))


def weight_average(lib, dev):
    ce = lib.embnet_optimizer_chunk_elems()
    chunks = chunk_list(SIZES, ce, dev)
    w, a = Tensors(5, dev), Tensors(6, dev)
    c_dev = torch.tensor([1e-3], dtype=torch.float32, device=dev)

    def table():
        w.again(), a.again()
        return u64([(w.t[i].data_ptr(), a.t[i].data_ptr(), n, 0) for i, n in enumerate(SIZES)], dev)

    for c, on_dev in ((0.0, 0), (1e-3, 0), (1.0, 0), (0.0, 1)):
        t = table()
        check(lib.embnet_weight_average_update(t.data_ptr(), len(SIZES), chunks.data_ptr(), chunks.shape[0], c,
                                               c_dev.data_ptr() if on_dev else None, None))
        emit(f"weight_average_update c={c} c_dev={on_dev} avg", torch.cat(a.bufs))
        emit(f"weight_average_update c={c} c_dev={on_dev} w", torch.cat(w.bufs))
    t = table()
    check(lib.embnet_weight_average_swap(t.data_ptr(), len(SIZES), chunks.data_ptr(), chunks.shape[0], None))
    emit("weight_average_swap avg", torch.cat(a.bufs))
    emit("weight_average_swap w", torch.cat(w.bufs))


def sumsq_and_range(lib, dev):
    x = Tensors(7, dev)
    chunks = chunk_list(SIZES, lib.embnet_sumsq_chunk_elems(), dev)
    t = u64([(x.t[i].data_ptr(), n, f32_word(1e-4 * (i + 1))) for i, n in enumerate(SIZES)], dev)
    out = torch.zeros(1, dtype=torch.float32, device=dev)
    ws = torch.zeros(chunks.shape[0], dtype=torch.float32, device=dev)
    check(lib.embnet_sumsq_multi(t.data_ptr(), len(SIZES), chunks.data_ptr(), chunks.shape[0], out.data_ptr(), ws.data_ptr(),
                                 ws.numel() * 4, None))
    emit("sumsq_multi out", out)
    emit("sumsq_multi partials", ws)
    chunks = chunk_list(SIZES, lib.embnet_range_chunk_elems(), dev)
    slots = torch.full((len(SIZES),), -1, dtype=torch.int32, device=dev)
    t = u64([(x.t[i].data_ptr(), n, slots.data_ptr() + 4 * i) for i, n in enumerate(SIZES)], dev)
    check(lib.embnet_range_multi(t.data_ptr(), len(SIZES), chunks.data_ptr(), chunks.shape[0], None))
    emit("range_multi slots", slots)


def weight_planes(lib, dev):
    g = torch.Generator().manual_seed(8)
    ce = lib.embnet_conv_weight_planes_chunk_elems()
    kernels = [torch.randn(3, 3, 16, 32, generator=g).to(dev), (0.05 * torch.randn(1, 1, 32, 16, generator=g)).to(dev)]
    rows, outs, sizes = [], [], []
    for w in kernels:
        r, s, c, k = w.shape
        for flip in (0, 1):
            outs.append(torch.zeros(3 * w.numel(), dtype=torch.int16, device=dev))
            rows.append((w.data_ptr(), outs[-1].data_ptr(), r | (s << 32), c | (k << 32), flip))
            sizes.append(w.numel())
    t, chunks = u64(rows, dev), chunk_list(sizes, ce, dev)
    check(lib.embnet_conv_weight_planes(t.data_ptr(), len(rows), chunks.data_ptr(), chunks.shape[0], None))
    for (w, flip), o in zip([(w, f) for w in kernels for f in (0, 1)], outs):
        emit(f"conv_weight_planes {list(w.shape)} flip={flip} terms={lib.embnet_conv_planes_mfma_terms()}", o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    for part in (optimizer, weight_average, sumsq_and_range, weight_planes):
        part(lib, dev)
    text = "\n".join(LINES) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
