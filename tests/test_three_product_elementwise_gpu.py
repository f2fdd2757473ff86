"""Every kernel of the default conv arithmetic — two fp16 pieces per operand, three products (include/embnet.h PRECISION) — held
against an independent NumPy model of that arithmetic (tests/split_ref.py), ELEMENT BY ELEMENT.

The neighbouring accuracy tests divide the largest error by the largest result of the whole tensor; that metric cannot see the
elements where this format goes wrong: a quiet channel beside a loud one, a dark image in a batch, a dead ReLU channel — elements
more than 2^17 below the tensor's bound sit on fp16's subnormal floor, and the bound itself may be 2^6 loose.  Two things can hide
there: the format's own floor (documented; measured per element in tests/test_split_ref_cpu.py and DESIGN.md 3.14 (9)) and a kernel
that does not compute the format (a flushed subnormal h2, a piece in the wrong slot, a wrong scale, a K-split fix-up or tail tile
that differs).  This file pins the second, through the C ABI:

  (a) the splitters ARE the format, bit for bit: the planes embnet_planes_from_f32, embnet_conv_weight_planes (flip 0 and 1) and
      embnet_affine_act_planes_ex write equal split_ref.split of the fp32 tensor, both pieces as uint16, at s = scale_of(bound used);
  (b) each kernel computes the model: |kernel - model| / sum|a||b| <= max(2 E32, 5e-7) for EVERY element, E32 the largest
      |float32 CPU convolution - float64| / sum|a||b| on the same operands (the criterion of
      tests/test_backbone_gpu.py::test_conv2d_products_are_fp32_accurate: only fp32 accumulation lies between kernel and model);
      where sum|a||b| = 0 the kernel's value is exactly 0.  The model's pieces are what the kernel reads: decoded planes for the
      planes kernels, split_ref.split at scale_of(range slot) for the in-kernel splitters (gather _ex, stem, DMA 1x1);
  (c) printed, not asserted: |kernel - float64| / sum|a||b| per bin of depth below the bound (split_ref.depth).

Input families (split_ref.operands) x activation bound 1x / 8x / 64x the true maximum (kernels and gradients keep their exact
maxima, as in the network) x the kernels and passes of CASES.

Measured on an MI355X — (b): the largest |kernel - model| / sum|a||b| over all elements, geometries and bound loosenesses, as a
multiple of the float32 CPU convolution's E32 on the same operands (the assertion allows 2; nobody had measured it: the
six-term kernels measured 0.75 - 1.6 under the same criterion); q_ = quiet_, filt = filters:

  kernel pass              even  spread10  spread17  spread20 q_image17 q_image20  q_filt17  q_filt20      zero      relu
  dma1x1 dgrad             0.56      0.44      0.53      0.55      0.50      0.66      0.64      0.64      1.02      0.60
  dma1x1 fwd               0.47      0.29      0.36      0.44      0.41      0.45      0.44      0.42      0.35      0.64
  gather dgrad             0.96      0.61      0.83      0.84      0.70      0.73      0.72      0.94      0.74      0.77
  gather fwd               0.18      0.24      0.21      0.31      0.24      0.17      0.25      0.19      0.20      0.26
  gather wgrad             1.18      1.15      1.15      1.25      0.88      0.80      1.32      0.90      0.90      1.24
  patch dgrad              0.88      0.59      0.67      0.58      0.59      0.63      0.81      0.77      1.17      0.66
  patch fwd                0.39      0.43      0.54      0.36      0.56      0.25      0.25      0.33      0.42      0.55
  planes1x1 dgrad          0.56      0.44      0.53      0.55      0.50      0.66      0.64      0.64      1.02      0.60
  planes1x1 fwd            0.47      0.29      0.36      0.44      0.41      0.45      0.44      0.42      0.35      0.64
  stem fwd                 0.76      0.85      0.83      0.77      0.86      0.83      0.69      0.81      1.05      1.28
  wgrad_planes wgrad       0.97      0.96      0.83      0.83      1.04      0.98      0.76      1.01      1.03      0.79

  largest ratio 1.32 (gather weight gradient, quiet filters 2^-17); largest |kernel - model| / sum|a||b| 1.0e-6.  Every splitter's
  planes are the emulator's bit for bit, up to the sign of a zero piece (assert_pieces has the finding).

(c): the largest |kernel - float64| / sum|a||b| by depth (binades below the bound, split_ref.depth) — the format's envelope of
tests/test_split_ref_cpu.py plus fp32 accumulation, i.e. what (b) and the CPU bound together imply:

  |kernel-f64|/mag        0..4     4..8    8..12   12..16   16..20   20..24   24..28   28..32   32..36
  dma1x1 dgrad               -  4.2e-07  5.3e-07  4.0e-07        -        -  1.2e-05  5.9e-05        -
  dma1x1 fwd           1.9e-07  3.1e-07  3.1e-07  2.1e-07  4.4e-07  4.2e-06  8.1e-05  2.1e-04        -
  gather dgrad         4.1e-07  9.2e-07  1.0e-06  7.3e-07  6.3e-07  5.6e-06  9.0e-05  6.1e-04  2.9e-04
  gather fwd           7.6e-08  1.8e-07  1.8e-07  1.3e-07  1.7e-07  1.5e-06  1.1e-05  8.1e-05        -
  gather wgrad         4.4e-07  7.0e-07  8.0e-07  6.8e-07  1.2e-06  2.1e-05  3.0e-04  3.7e-03        -
  patch dgrad                -  3.3e-07  5.3e-07  1.6e-07        -        -  1.7e-05  1.8e-04        -
  patch fwd            1.5e-07  3.3e-07  3.3e-07  1.2e-07  3.3e-07  1.9e-06  3.7e-05  1.3e-04        -
  planes1x1 dgrad            -  4.2e-07  5.3e-07  4.0e-07        -        -  1.2e-05  5.9e-05        -
  planes1x1 fwd        1.9e-07  3.1e-07  3.1e-07  2.1e-07  4.4e-07  4.2e-06  8.1e-05  2.1e-04        -
  stem fwd             3.7e-07  3.7e-07  3.7e-07        -  4.7e-07  3.3e-06  7.4e-05  2.4e-04        -
  wgrad_planes wgrad         -  5.7e-07  5.6e-07  4.4e-07  8.8e-07  1.3e-05  1.4e-04  4.3e-04        -
  all kernels          4.4e-07  9.2e-07  1.0e-06  7.3e-07  1.2e-06  2.1e-05  3.0e-04  3.7e-03  2.9e-04

A model made wrong on purpose (EMBNET_TEST_WRONG_MODEL=drop: without h2 h1'; =flush: subnormal h2 flushed to zero) fails (b): see
model_terms().
"""
import os
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd import layers as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as SR  # noqa: E402
import test_conv_ranges_gpu as CR  # noqa: E402   (conv_fwd / conv_dgrad / conv_wgrad / range_of: the gather _ex launchers)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    if _lib.lib().embnet_conv_planes_mfma_terms() != 3:
        pytest.skip("the two-piece fp16 planes format is off (EMBNET_PLANES_F16=0)")
    return torch.device("cuda", 0)


# ---- operands on the device, in the form each kernel reads ------------------------------------------------------------------------------
def f32max(t):
    return np.float32(np.abs(np.asarray(t)).max())


def slot_of(value, dev):
    """A range slot holding the bit pattern of float32 `value`."""
    return torch.from_numpy(np.array([value], dtype=np.float32).view(np.int32).copy()).to(dev)


def planes_from(t):
    """embnet_planes_from_f32 of an NHWC (or [m, c]) tensor."""
    c = t.shape[-1]
    p = torch.zeros(3 * t.numel(), dtype=torch.int16, device=t.device)
    _lib.check(_lib.lib().embnet_planes_from_f32(t.data_ptr(), t.numel() // c, c, p.data_ptr(), _lib.stream()))
    return p


def act_planes(t, bound, scale=None, shift=None, act=0):
    """embnet_affine_act_planes_ex of t (viewed [m, c]) with a per-channel bound vector -> (y fp32, planes, range slot).
    scale / shift None: the identity (y = fma(t, 1, 0) = t exactly)."""
    c = t.shape[-1]
    m = t.numel() // c
    dev = t.device
    sc = torch.ones(c, device=dev) if scale is None else scale
    sh = torch.zeros(c, device=dev) if shift is None else shift
    yb = torch.from_numpy(np.broadcast_to(np.asarray(bound, dtype=np.float32), (c,)).copy()).to(dev)
    y = torch.full((m, c), float("nan"), device=dev)
    p = torch.zeros(3 * m * c, dtype=torch.int16, device=dev)
    rng = torch.full((1,), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().embnet_affine_act_planes_ex(t.data_ptr(), m, c, sc.data_ptr(), sh.data_ptr(), act, y.data_ptr(), p.data_ptr(),
                                                      yb.data_ptr(), rng.data_ptr(), _lib.stream()))
    return y, p, rng


def assert_pieces(got, want, what):
    """Both pieces equal as uint16 — up to the SIGN OF A ZERO piece.  Finding (embnet_conv_weight_planes, x = -0.0): the compiler
    contracts split4h's `x s - h1` into fused multiply-adds (v_fma_mixlo_f16 v, s, 0 recomputes h1 as fma(x, s, +0) = +0 for
    x = -0.0, and the rest fma(x, s, -(+0)) comes out as -0 where IEEE's (-0) - (-0) is +0).  A zero piece of either sign adds
    nothing to any product sum, so 0x8000 and 0x0000 are the same piece here; every other bit pattern must match exactly."""
    for i, (g, w) in enumerate(zip(got, want)):
        gb, wb = np.ascontiguousarray(g).view(np.uint16).copy(), np.ascontiguousarray(w).view(np.uint16).copy()
        gb[gb == 0x8000] = 0
        wb[wb == 0x8000] = 0
        bad = gb != wb
        if bad.any():
            pairs = ", ".join("%04x != %04x" % (a, b) for a, b in zip(gb[bad][:6], wb[bad][:6]))
            raise AssertionError("%s: piece %d differs in %d of %d elements (kernel != split_ref): %s" % (what, i + 1, bad.sum(), bad.size, pairs))


def x_planes(xd, x, loose):
    """Planes of activation x at a bound loose x its maximum, through embnet_affine_act_planes_ex; (a) is asserted on the way."""
    bound = np.float32(f32max(x) * np.float32(loose))
    y, p, rng = act_planes(xd, bound)
    c = x.shape[-1]
    h1, h2, s = SR.decode_planes(p.cpu().numpy(), x.size // c, c)
    assert s == SR.scale_of(bound), (s, bound)
    assert int(rng.item()) == int(np.array([bound]).view(np.int32)[0])
    assert np.array_equal(y.cpu().numpy().reshape(x.shape), x)
    assert_pieces((h1, h2), [q.reshape(-1, c) for q in SR.split(x, s)], "affine_act_planes_ex")
    return p, (h1.reshape(x.shape), h2.reshape(x.shape)), s, float(bound)


def t_planes(td, t):
    """embnet_planes_from_f32 (a gradient: its own abs-max pass)."""
    p = planes_from(td)
    c = t.shape[-1]
    h1, h2, s = SR.decode_planes(p.cpu().numpy(), t.size // c, c)
    assert s == SR.scale_of(f32max(t)), (s, f32max(t))
    assert_pieces((h1, h2), [q.reshape(-1, c) for q in SR.split(t, s)], "planes_from_f32")
    return p, (h1.reshape(t.shape), h2.reshape(t.shape)), s


def w_planes(wd, w, flip):
    p = L.weight_planes(wd, flip)
    h1, h2, s = SR.decode_weight_planes(p.cpu().numpy(), w.shape, flip)
    assert s == SR.scale_of(f32max(w)), (s, f32max(w))
    assert_pieces((h1, h2), SR.split(w, s), "conv_weight_planes flip %d" % flip)
    return p, (h1, h2), s


def in_kernel(t, bound):
    s = SR.scale_of(bound)
    return SR.split(t, s), s


# ---- the launchers: (x, kern, dy numpy; loose) -> (result, a pieces, b pieces, s_a, s_b, bound_a, bound_b) --------------------------------
def out_hw(h, w, ks, stride, pad):
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def run_gather(kind, geo, x, kern, dy, loose, dev):
    n, h, w, c, k, ks, stride, pad = geo
    oh, ow = out_hw(h, w, ks, stride, pad)
    g = (stride, pad, pad, oh, ow)
    xd, wd, dyd = (torch.from_numpy(t).to(dev) for t in (x, kern, dy))
    bx, bw, bdy = np.float32(f32max(x) * np.float32(loose)), f32max(kern), f32max(dy)
    rx, rw, rdy = slot_of(bx, dev), CR.range_of(wd), CR.range_of(dyd)
    assert CR.bits(rw) == int(np.array([bw]).view(np.uint32)[0]) and CR.bits(rdy) == int(np.array([bdy]).view(np.uint32)[0])
    if kind == "fwd":
        got, (a, ba), (b, bb) = CR.conv_fwd(xd, wd, g, (rx, rw)), (x, bx), (kern, bw)
    elif kind == "dgrad":
        got, (a, ba), (b, bb) = CR.conv_dgrad(dyd, wd, tuple(x.shape), g, (rdy, rw)), (dy, bdy), (kern, bw)
    else:
        got, (a, ba), (b, bb) = CR.conv_wgrad(xd, dyd, tuple(kern.shape), g, (rx, rdy)), (x, bx), (dy, bdy)
    pa, sa = in_kernel(a, ba)
    pb, sb = in_kernel(b, bb)
    return got, pa, pb, sa, sb, float(ba), float(bb)


def run_patch(kind, geo, x, kern, dy, loose, dev):
    lib = _lib.lib()
    n, h, w, c, k, ks, stride, pad = geo
    xd, wd, dyd = (torch.from_numpy(t).to(dev) for t in (x, kern, dy))
    if kind == "fwd":
        assert lib.embnet_conv2d_patch_supported(n, c, 3, 3, k, 1, h, w) == 1
        ap, pa, sa, ba = x_planes(xd, x, loose)
        bp, pb, sb = w_planes(wd, kern, 0)
        y = torch.full((n, h, w, k), float("nan"), device=dev)
        ws = torch.empty(max(lib.embnet_conv2d_patch_workspace_bytes(n, c, 3, 3, k, h, w), 4) // 4, device=dev)
        _lib.check(lib.embnet_conv2d_patch_f32(ap.data_ptr(), bp.data_ptr(), None, y.data_ptr(), n, h, w, c, 3, 3, k, 1, 1, h, w, 0, None, None,
                                               ws.data_ptr(), ws.numel() * 4, _lib.stream()))
        return y, pa, pb, sa, sb, ba, float(f32max(kern))
    assert lib.embnet_conv2d_patch_supported(n, k, 3, 3, c, 1, h, w) == 1
    ap, pa, sa = t_planes(dyd, dy)
    bp, pb, sb = w_planes(wd, kern, 1)
    dx = torch.full((n, h, w, c), float("nan"), device=dev)
    ws = torch.empty(max(lib.embnet_conv2d_patch_workspace_bytes(n, k, 3, 3, c, h, w), 4) // 4, device=dev)
    _lib.check(lib.embnet_conv2d_patch_f32(ap.data_ptr(), bp.data_ptr(), None, dx.data_ptr(), n, h, w, k, 3, 3, c, 1, 1, h, w, 0, None, None,
                                           ws.data_ptr(), ws.numel() * 4, _lib.stream()))
    return dx, pa, pb, sa, sb, float(f32max(dy)), float(f32max(kern))


def run_wgrad_planes(kind, geo, x, kern, dy, loose, dev):
    lib = _lib.lib()
    n, h, w, c, k, ks, stride, pad = geo
    assert lib.embnet_conv2d_wgrad_planes_supported(n, h, w, c, 3, 3, k, 1, 1, 1, h, w) == 1
    xd, dyd = torch.from_numpy(x).to(dev), torch.from_numpy(dy).to(dev)
    ap, pa, sa, ba = x_planes(xd, x, loose)
    bp, pb, sb = t_planes(dyd, dy)
    dw = torch.full((3, 3, c, k), float("nan"), device=dev)
    ws = torch.empty(max(lib.embnet_conv2d_wgrad_planes_workspace_bytes(n, h, w, c, k) // 4, 4), device=dev)
    _lib.check(lib.embnet_conv2d_wgrad_planes_f32(ap.data_ptr(), bp.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel() * 4, n, h, w, c, k, 1,
                                                  _lib.stream()))
    return dw, pa, pb, sa, sb, ba, float(f32max(dy))


def run_stem(kind, geo, x, kern, dy, loose, dev):
    lib = _lib.lib()
    n, h, w, c, k, ks, stride, pad = geo
    oh, ow = out_hw(h, w, 7, 2, pad)
    assert lib.embnet_conv2d_stem_supported(n, h, w, 4, 7, 7, 64, 2, pad, pad, oh, ow) == 1
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(kern).to(dev)
    bx, bw = np.float32(f32max(x) * np.float32(loose)), f32max(kern)
    rx, rw = slot_of(bx, dev), slot_of(bw, dev)
    y = torch.full((n, oh, ow, 64), float("nan"), device=dev)
    _lib.check(lib.embnet_conv2d_stem_f32(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), n, h, w, pad, pad, oh, ow, None, rx.data_ptr(),
                                          rw.data_ptr(), _lib.stream()))
    pa, sa = in_kernel(x, bx)
    pb, sb = in_kernel(kern, bw)
    return y, pa, pb, sa, sb, float(bx), float(bw)


def run_1x1(kernel, kind, geo, x, kern, dy, loose, dev):
    """planes1x1 / dma1x1, forward (stride 1 or 2) and stride-1 data gradient (flip-1 kernel planes, channel roles swapped)."""
    lib = _lib.lib()
    n, h, w, c, k, ks, stride, pad = geo
    oh, ow = out_hw(h, w, 1, stride, 0)
    wd = torch.from_numpy(kern).to(dev)
    if kind == "fwd":
        src, srcd, red, cols, flip, oh_, ow_, ih, iw = x, torch.from_numpy(x).to(dev), c, k, 0, oh, ow, h, w
    else:
        assert stride == 1
        src, srcd, red, cols, flip, oh_, ow_, ih, iw = dy, torch.from_numpy(dy).to(dev), k, c, 1, h, w, oh, ow
    bp, pb, sb = w_planes(wd, kern, flip)
    out = torch.full((n, oh_, ow_, cols), float("nan"), device=dev)
    ws = torch.empty(max(lib.embnet_conv2d_patch_workspace_bytes(n, red, 1, 1, cols, oh_, ow_), 4) // 4, device=dev)
    if kernel == "planes1x1":
        assert lib.embnet_conv2d_patch_supported(n, red, 1, 1, cols, stride, oh_, ow_) == 1
        if kind == "fwd":
            ap, pa, sa, ba = x_planes(srcd, src, loose)
        else:
            ap, pa, sa = t_planes(srcd, src)
            ba = float(f32max(src))
        _lib.check(lib.embnet_conv2d_planes1x1_f32(ap.data_ptr(), bp.data_ptr(), None, out.data_ptr(), n, ih, iw, red, cols, stride, oh_, ow_, 0,
                                                   None, None, ws.data_ptr(), ws.numel() * 4, _lib.stream()))
    else:
        assert lib.embnet_conv2d_dma1x1_supported(n, ih, iw, red, cols, stride, oh_, ow_) == 1
        ba = np.float32(f32max(src) * np.float32(loose if kind == "fwd" else 1.0))
        rng = slot_of(ba, dev)
        _lib.check(lib.embnet_conv2d_dma1x1_f32(srcd.data_ptr(), bp.data_ptr(), None, out.data_ptr(), n, ih, iw, red, cols, stride, oh_, ow_, 0,
                                                None, None, rng.data_ptr(), ws.data_ptr(), ws.numel() * 4, _lib.stream()))
        pa, sa = in_kernel(src, ba)
        ba = float(ba)
    return out, pa, pb, sa, sb, ba, float(f32max(kern))


RUNNERS = {
    "gather": run_gather, "patch": run_patch, "wgrad_planes": run_wgrad_planes, "stem": run_stem,
    "planes1x1": lambda *a: run_1x1("planes1x1", *a), "dma1x1": lambda *a: run_1x1("dma1x1", *a),
}
TRACE_NAME = {
    ("gather", "fwd"): "conv_fwd_h_kernel", ("gather", "dgrad"): "conv_dgrad_h_kernel", ("gather", "wgrad"): "conv_wgrad_h_kernel",
    ("patch", "fwd"): "conv_patch_kernel", ("patch", "dgrad"): "conv_patch_kernel", ("wgrad_planes", "wgrad"): "conv_wgrad_planes_kernel",
    ("stem", "fwd"): "conv_stem_kernel", ("planes1x1", "fwd"): "conv1x1_planes_kernel", ("planes1x1", "dgrad"): "conv1x1_planes_kernel",
    ("dma1x1", "fwd"): "conv1x1_a32_kernel", ("dma1x1", "dgrad"): "conv1x1_a32_kernel",
}

# geometry: n, h, w, c, k, kernel size, stride, pad — from the LAYERS / GEOMS lists of the neighbouring files (batch cut where the
# float64 reference would cost more than a fraction of a second)
G_K4608 = (2, 12, 12, 512, 64, 3, 2, 1)        # test_conv_ranges_gpu.py's worst-case geometry: K = 4608, forward K-split workspace
G_S2 = (4, 28, 28, 64, 128, 3, 2, 1)           # LAYERS: stride-2 3x3; the weight gradient's split + workspace
G_RAGGED1 = (2, 9, 7, 512, 128, 1, 1, 0)       # LAYERS: ragged map, long 1x1 reduction
P_K4608 = (4, 7, 7, 512, 512, 3, 1, 1)         # patch GEOMS (32 -> 4 images): K = 4608, few tiles: reduction split + fix-up workspace
P_RAGGED = (3, 13, 9, 32, 96, 3, 1, 1)         # patch GEOMS: ragged rows, K not a multiple of the tile
W_LONG = (4, 56, 56, 64, 64, 3, 1, 1)          # wgrad-planes GEOMS: 12 544 positions in the reduction, 82 splits
W_RAGGED = (3, 13, 9, 64, 192, 3, 1, 1)        # wgrad-planes GEOMS: positions not a multiple of the stage
S_64 = (3, 64, 64, 4, 64, 7, 2, 3)             # stem: the suite's small image size
S_RAGGED = (2, 75, 61, 4, 64, 7, 2, 3)         # stem: outputs not a multiple of the 16 x 16 tile
O_LONG = (2, 7, 7, 2048, 512, 1, 1, 0)         # 1x1 GEOMS (8 -> 2 images): few tiles, long reduction: split over workgroups + fix-up
O_S2 = (3, 15, 13, 64, 96, 1, 2, 0)            # 1x1 GEOMS: stride 2, ragged
O_DG = (2, 7, 7, 512, 2048, 1, 1, 0)           # its data gradient: reduction over k = 2048

CASES = [
    ("gather", "fwd", G_K4608), ("gather", "dgrad", G_K4608), ("gather", "wgrad", G_K4608),
    ("gather", "fwd", G_S2), ("gather", "dgrad", G_S2), ("gather", "wgrad", G_S2),
    ("gather", "fwd", G_RAGGED1), ("gather", "dgrad", G_RAGGED1), ("gather", "wgrad", G_RAGGED1),
    ("patch", "fwd", P_K4608), ("patch", "dgrad", P_K4608), ("patch", "fwd", P_RAGGED), ("patch", "dgrad", P_RAGGED),
    ("wgrad_planes", "wgrad", W_LONG), ("wgrad_planes", "wgrad", W_RAGGED),
    ("stem", "fwd", S_64), ("stem", "fwd", S_RAGGED),
    ("planes1x1", "fwd", O_LONG), ("planes1x1", "fwd", O_S2), ("planes1x1", "dgrad", O_DG),
    ("dma1x1", "fwd", O_LONG), ("dma1x1", "fwd", O_S2), ("dma1x1", "dgrad", O_DG),
]


def case_id(case):
    return "%s-%s-%s" % (case[0], case[1], "x".join(map(str, case[2])))


def test_the_cases_take_the_k_split_paths(dev):
    """The geometries chosen for the reduction-split / fix-up paths do have a workspace (host-side plan queries)."""
    lib = _lib.lib()
    n, h, w, c, k, ks, stride, pad = G_K4608
    oh, ow = out_hw(h, w, ks, stride, pad)
    assert ks * ks * c >= 4608 and lib.embnet_conv2d_fwd_workspace_bytes(n, c, ks, ks, k, oh, ow) > 0
    n, h, w, c, k, ks, stride, pad = G_S2
    oh, ow = out_hw(h, w, ks, stride, pad)
    assert lib.embnet_conv2d_wgrad_workspace_bytes(n, c, ks, ks, k, oh, ow) > 0
    n, h, w, c, k = P_K4608[:5]
    assert 9 * c >= 4608 and lib.embnet_conv2d_patch_workspace_bytes(n, c, 3, 3, k, h, w) > 0
    n, h, w, c, k = W_LONG[:5]
    assert n * h * w >= 4608 and lib.embnet_conv2d_wgrad_planes_splits(n, h, w, c, k) > 1
    n, h, w, c, k = O_LONG[:5]
    assert lib.embnet_conv2d_patch_workspace_bytes(n, c, 1, 1, k, h, w) > 0


# ---- (b) and (c) -----------------------------------------------------------------------------------------------------------------------
def model_terms():
    """EMBNET_TEST_WRONG_MODEL = drop | flush makes the MODEL wrong on purpose (run by hand, once: (b) must then fail on the quiet
    families while the per-tensor tests, which do not know the model, stay green)."""
    mode = os.environ.get("EMBNET_TEST_WRONG_MODEL", "")
    assert mode in ("", "drop", "flush"), mode
    return dict(terms=(True, True, mode != "drop"), flush_h2=(mode == "flush"))


@pytest.mark.parametrize("family", SR.FAMILIES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_computes_the_model_per_element(dev, case, family):
    kernel, kind, geo = case
    n, h, w, c, k, ks, stride, pad = geo
    x, kern, dy = SR.operands(family, n, h, w, c, k, ks, stride, pad, seed=sum(geo), pad_channel=(kernel == "stem"))
    a, b, out_shape = SR.pass_operands(kind, x, kern, dy)
    geom = SR.Geometry(kind, stride, pad, out_shape)
    truth = SR.conv(a, b, geom)
    m = SR.mag(a, b, geom)
    live = m > 0
    e32 = float((np.abs(SR.conv(a, b, geom, dtype=torch.float32) - truth)[live] / m[live]).max())
    allowed = max(2 * e32, 5e-7)
    reach = SR.reach(a, b, geom)
    activation_first = kind != "dgrad"                       # (the data gradient has no activation operand: nothing is loose)
    for loose in (SR.LOOSE if activation_first else [1.0]):
        _lib.trace_reset(); _lib.trace_enable(True)
        try:
            got, pa, pb, sa, sb, ba, bb = RUNNERS[kernel](kind, geo, x, kern, dy, loose, dev)
            torch.cuda.synchronize()
            names = [r[0] for r in _lib.trace_records()]
        finally:
            _lib.trace_enable(False)
        assert any(TRACE_NAME[(kernel, kind)] in s for s in names), names
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == truth.shape and np.isfinite(got).all()
        model = SR.model_conv(pa, pb, sa, sb, geom, **model_terms())
        # where nothing contributes the result is exactly zero
        assert (got[~live] == 0).all(), (family, loose, int((got[~live] != 0).sum()))
        err = np.abs(got - model)[live] / m[live]
        ratio = float(err.max()) / e32
        env = SR.envelope(np.abs(got - truth), m, SR.depth_from(reach, ba, bb, m))
        print("ELEMENTWISE %s %s loose %g: |kernel - model| / mag %.2e = %.2f x float32 CPU conv (%.2e); |kernel - float64| / mag by depth %s"
              % (case_id(case), family, loose, err.max(), ratio, e32, " ".join("%d:%.1e" % (SR.BIN * bn, v) for bn, v in sorted(env.items()))))
        assert err.max() <= allowed, (family, loose, float(err.max()), e32, int(np.argmax(err)))


# ---- (a) the splitters, on their own: amplitudes and dynamic ranges the convolution cases do not reach ------------------------------------
def deep(shape, amp, binades, g):
    """Values spread over `binades` binades below amp, both signs, with exact zeros, a negative zero and the largest element."""
    v = torch.randn(shape, generator=g) * amp * torch.exp2(-binades * torch.rand(shape, generator=g))
    flat = v.view(-1)
    flat[0], flat[1], flat[2] = 0.0, -0.0, amp * 4.5
    return v.numpy().copy()


@pytest.mark.parametrize("amp", [1e-4, 1.7, 1e5, 1e-30, 1e30])
@pytest.mark.parametrize("m,c", [(3 * 13 * 9, 48), (4 * 7 * 7, 512), (1, 16)])
def test_planes_from_f32_is_the_split_bit_for_bit(dev, m, c, amp):
    g = torch.Generator().manual_seed(m + c)
    x = deep((m, c), amp, 44, g)
    t_planes(torch.from_numpy(x).to(dev), x)


@pytest.mark.parametrize("amp", [1e-3, 0.05, 300.0])
@pytest.mark.parametrize("shape", [(3, 3, 32, 96), (1, 1, 64, 96), (3, 3, 512, 64), (7, 7, 16, 64)])
def test_weight_planes_are_the_split_bit_for_bit_in_both_layouts(dev, shape, amp):
    g = torch.Generator().manual_seed(sum(shape))
    w = deep(shape, amp, 44, g)
    wd = torch.from_numpy(w).to(dev)
    for flip in (0, 1):
        w_planes(wd, w, flip)


@pytest.mark.parametrize("loose", SR.LOOSE)
@pytest.mark.parametrize("amp", [1e-4, 1.7, 3e4])
@pytest.mark.parametrize("act", [0, 1])
def test_affine_act_planes_are_the_split_of_the_fp32_output_bit_for_bit(dev, act, amp, loose):
    """A BatchNormalization's apply pass with per-channel scales spread over 2^20, per-channel bounds as bn_finalize leaves them
    (each channel's own maximum x loose): planes = split(the fp32 y the same call writes) at s = scale_of(max_c bound_c)."""
    g = torch.Generator().manual_seed(int(amp * 10) + act)
    m, c = 4 * 13 * 9, 64
    x = torch.randn(m, c, generator=g)
    scale = (torch.rand(c, generator=g) + 0.5) * amp * torch.exp2(-20 * torch.rand(c, generator=g))
    scale[3] = amp
    shift = torch.randn(c, generator=g) * 0.3 * scale
    xd, sc, sh = x.to(dev), scale.to(dev), shift.to(dev)
    y0 = torch.nn.functional.relu(xd * sc + sh) if act else xd * sc + sh
    chan = (y0.abs().amax(0) * 1.001 * loose).cpu().numpy().astype(np.float32)          # sound per-channel bounds
    y, p, rng = act_planes(xd, chan, sc, sh, act)
    yn = y.cpu().numpy()
    assert np.isfinite(yn).all() and (np.abs(yn).max(0) <= chan).all()
    h1, h2, s = SR.decode_planes(p.cpu().numpy(), m, c)
    bound = chan.max()
    assert s == SR.scale_of(bound) and int(rng.item()) == int(np.array([bound]).view(np.int32)[0])
    assert_pieces((h1, h2), SR.split(yn, s), "affine_act_planes_ex")


# ---- in the network: how deep below their tensor's bound do the shipped nets' channels lie? ------------------------------------------------
def bn_bound_survey(dev, name, steps_before):
    """One training step of `name` at 64 x 64 after `steps_before` optimizer steps: every training BatchNormalization's per-channel
    bound row (embnet_bn_train_fwd_ex `bound`, stats[4]) -> per layer (channels, channels more than 2^14 / 2^17 / 2^20 below the
    tensor's bound max_c bound_c)."""
    from embeddingnet_amd.backbones import get_backbone
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer
    torch.manual_seed(0)
    base, _ = get_backbone((64, 64, 3), encodings_len=64, backbone_name=name, backbone_weights=None, seed=4, device=dev)
    base.train()
    tr = TripletTrainer(base, KerasOptimizer(base.parameters(), "adam", 1e-3), k_classes=4, k_samples=4, margin=0.5,
                        negatives_selection_mode="hardest", graph=False)
    g = torch.Generator().manual_seed(9)
    for _ in range(steps_before):
        tr.step(torch.rand(16, 64, 64, 3, generator=g).to(dev))
    seen = []
    inner = L._bn_stats

    def recording(*args, **kw):
        stats, st = inner(*args, **kw)
        training = args[9] if len(args) > 9 else kw.get("training")
        if training and stats.shape[0] >= 6:
            seen.append(stats)
        return stats, st

    L._bn_stats = recording
    try:
        tr.step(torch.rand(16, 64, 64, 3, generator=g).to(dev))
        torch.cuda.synchronize()
    finally:
        L._bn_stats = inner
    rows = []
    for stats in seen:
        b = stats[4].detach().cpu().numpy().astype(np.float64)
        assert np.isfinite(b).all() and (b >= 0).all()
        top = b.max()
        nz = b[b > 0]                                      # (a channel whose bound is 0 is exactly zero: the image's pad channel)
        rows.append((b.size, int((nz < top * 2.0 ** -14).sum()), int((nz < top * 2.0 ** -17).sum()), int((nz < top * 2.0 ** -20).sum()),
                     float(np.log2(top / nz.min())) if nz.size else 0.0, int((b == 0).sum())))
    return rows


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_bn_channel_bounds_survey_in_the_shipped_resnets(dev, name):
    """Recorded for DESIGN.md 3.14 (9), asserted only to exist and be finite: whether the per-element floor of the format is
    reachable in the shipped nets — channels whose BOUND is more than 2^14 / 2^17 / 2^20 below their tensor's."""
    for label, steps in (("fresh", 0), ("after 4 steps", 4)):
        rows = bn_bound_survey(dev, name, steps)
        assert rows, "no training BatchNormalization left a bound row"
        tot = np.array([r[:4] for r in rows]).sum(0)
        deepest = max(r[4] for r in rows)
        print("SURVEY %s %s: %d BatchNormalizations, %d channels; below the tensor's bound by more than 2^14: %d, 2^17: %d, 2^20: %d "
              "channels (all-zero bounds: %d); deepest non-zero channel 2^-%.1f; layers with any channel beyond 2^14: %d"
              % (name, label, len(rows), tot[0], tot[1], tot[2], tot[3], sum(r[5] for r in rows), deepest, sum(r[1] > 0 for r in rows)))
        assert np.isfinite(deepest) and tot[0] > 0
