"""The streaming kernels of the EfficientNet configurations — the depthwise kernels of csrc/mbconv_kernels.hip and csrc/dwconv_tile.hip,
the thin 1x1 kernels of csrc/conv_thin.hip — through the C ABI against float64 (tests/stream_ref.py), PER ELEMENT and PER CHANNEL.

Every output of these kernels feeds a BatchNormalization that rescales each channel by that channel's own standard deviation, and
the per-channel partial sums they emit replace that layer's reduction pass: an error matters relative to the channel it lands in.
The neighbouring tests divide the largest error by the largest value of the whole tensor, on inputs whose channels share one scale;
with per-channel amplitudes spread over 2^17 a third of the channels lies below what that metric can see
(test_the_old_metric_is_blind_to_a_quiet_channel).  These kernels do exact fp32 FMA arithmetic, so the tolerance needs no
measurement: it is the textbook rounding bound, gamma(n) = n u / (1 - n u), u = 2^-24.

  per element   |kernel - float64| <= gamma(n) sum|a||b|, n = products of the element (+ 2 for bias and residual): k k for the
                depthwise forward / data gradient, R (+ 2) for the thin ones, the output pixels M for the weight gradients (any
                summation order, slabs included); where sum|a||b| = 0 the kernel's value is exactly 0;
  statistics    on the kernel's OWN fp32 output: |S1 - sum y| <= gamma(M) sum|y|, |S2 - sum y^2| <= gamma(M + 1) sum y^2 per channel,
                S the float64 sum of the partial rows; every (channel, row) written; the output bit-identical to the plain launch;
  BN sums       on the kernel's own dx: |S1 - sum dz| <= gamma(M) sum|dz| + 4 E32 + B, |S2 - sum dz ehat| <= gamma(M + 3) sum|dz ehat|
                + 4 E32' + B' per channel; E32 = sum |term in float32 on the CPU - term in float64| (against the reference, never
                the kernel; 4 = the margin for the device's exp being another fp32 implementation), B / B' = sum |dx| / |dx ehat|
                over the channel's ReLU-borderline elements (ReLU only; at most 0.1 % of a channel);
  memory        every output and partials buffer sits inside a larger buffer with a 4 KB sentinel margin on both sides: no
                sentinel left inside, the margins untouched.

Families (stream_ref.GPU_FAMILIES): even, spread17, quiet_image17, zero, relu.  Which kernel ran is asserted from the kernel trace;
the trace names every row kernel dwconv_row4_kernel, and for those the geometry rules of launch_dw_rows decide (dw_wide / rows2
below mirror them; the statistics' row count, which follows from them, is asserted).

Dispatch findings, from reading the host code:
  * (2,1,9,16,3,1), listed for the one-row kernel, has C % 16 == 0 on a map under 32 x 32: it runs on the LDS-tile kernel (a
    one-row image there: every window row but one masked); (2,1,9,24,3,1) is added and reaches dwconv_row4_kernel's one-row form at
    stride 1, (2,2,9,16,3,2) at stride 2.
  * thin_wgrad_applies needs thin/4 + wide/4 <= 256 (eight pixels per 32 KB tile), so the widest weight gradient on
    thin_wgrad_kernel is 1016 (thin 4 or 8), not 1024: the wide cases here are 1016; 1024 runs on the MFMA kernels, which the
    three-product file covers.

MEASURED ON AN MI355X — every assertion holds, no kernel needed a change.  Largest |kernel - float64| / (gamma(n) sum|a||b|) over
all elements and geometries (printed, not asserted beyond < 1; the float32 CPU evaluation measures 0.13 - 0.43,
tests/test_stream_ref_cpu.py; the ratios are largest where n is small: half an ulp of a one-product element is 0.5):

  kernel, pass                              even       spread17  quiet_image17           zero           relu
  row kernels forward                      0.390          0.450          0.430          0.422          0.348
  row kernels data gradient (stride 1)     0.563          0.589          0.547          0.551              -
  dwconv_dgrad4_s2_row data gradient       0.361          0.325          0.326          0.375              -
  tile kernel forward                      0.174          0.197          0.172          0.178          0.142
  tile kernel data gradient                0.317          0.322          0.328          0.288              -
  generic fallbacks forward                0.228          0.250          0.203          0.152          0.179
  generic fallbacks data gradient          0.299          0.317          0.326          0.334              -
  dwconv_wgrad4_wave weight gradient       0.243          0.163          0.279          0.152          0.149
  dw_tile_wgrad weight gradient            0.087          0.076          0.059          0.108          0.147
  dwconv_wgrad4 weight gradient            0.022          0.027          0.028          0.031          0.024
  dwconv_wgrad1 weight gradient            0.029          0.018          0.029          0.020          0.019
  thin_gemm forward                        0.635          0.706          0.607          0.536          0.538
  thin_gemm forward, bias + ReLU + res.    0.497          0.572          0.424          0.423          0.447
  thin_gemm data gradient                  0.376          0.426          0.336          0.363              -
  thin_wgrad, x thin                       0.041          0.032          0.046          0.033          0.038
  thin_wgrad, dy thin                      0.025          0.030          0.033          0.035          0.038

Statistics: largest |S - sum| / bound per channel.  BatchNorm-backward sums: largest |S - reference| / (gamma mag + E32) per
channel — the assertion allows gamma mag + 4 E32 + B; nobody had measured it: the device's __expf-based swish gradient stays
far inside ONE E32, the factor 4 is not needed by any kernel:

  kernel, quantity                          even       spread17  quiet_image17           zero           relu
  row kernels forward S1                   0.065          0.058          0.075          0.077          0.076
  row kernels forward S2                   0.095          0.073          0.118          0.128          0.104
  tile kernel forward S1                   0.068          0.036          0.044          0.027          0.076
  tile kernel forward S2                   0.071          0.075          0.081          0.066          0.106
  thin_gemm S1                             0.012          0.012          0.029          0.021          0.043
  thin_gemm S2                             0.477          0.470          0.445          0.057          0.463
  thin_gemm, epilogue, S1                  0.027          0.048          0.079          0.027          0.035
  thin_gemm, epilogue, S2                  0.457          0.468          0.475          0.468          0.483
  row kernels sum dz, ReLU / swish         0.005 / 0.007  0.007 / 0.004  0.010 / 0.024  0.006 / 0.006      -
  row kernels sum dz ehat                  0.011 / 0.007  0.009 / 0.005  0.010 / 0.010  0.008 / 0.013      -
  dwconv_dgrad4_s2_row sum dz              0.025 / 0.037  0.052 / 0.031  0.032 / 0.061  0.034 / 0.065      -
  dwconv_dgrad4_s2_row sum dz ehat         0.037 / 0.060  0.029 / 0.027  0.030 / 0.047  0.033 / 0.075      -
  tile kernel sum dz                       0.057 / 0.076  0.057 / 0.070  0.047 / 0.127  0.036 / 0.055      -
  tile kernel sum dz ehat                  0.063 / 0.086  0.046 / 0.063  0.034 / 0.068  0.058 / 0.110      -

  (thin_gemm's S2 of 0.48 is the single-pixel case: M = 1, the one square's own rounding against gamma(2).)

The guard (test_the_old_metric_is_blind_to_a_quiet_channel), spread17 on (2,9,9,24,3,1): the quietest channel lies at 1.4e-7 of the
loudest, 38 % of the channels below 1e-5 of it.  A reference without one border tap there: the old metric reads 9.1e-8 (passes
1e-5), the per-element ratio 3.1e5 (fails 1).  One partial row counted twice: the old sums criterion passes, the per-channel one
fails.  The whole file (61 tests) costs 6 s on the GPU.
"""
import os
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd._lib import check, stream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_ref as ST  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = ST.GPU_FAMILIES
MARGIN = 1024                                              # floats: 4 KB on both sides
PATTERN = 0x7FC0BEEF                                       # a NaN no arithmetic produces
ELEM = {}                                                  # (kernel, pass, family) -> largest |kernel - float64| / (gamma(n) mag)
SUMS = {}                                                  # (kernel, what, family) -> largest |S - ref| / bound  /  / (gamma mag + E32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def guarded(shape, dev):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * MARGIN,), PATTERN, dtype=torch.int32, device=dev)
    return big, big[MARGIN:MARGIN + n].view(torch.float32).view(*shape)


def assert_guard(big, out, what):
    assert not bool(torch.isnan(out).any()), what + ": an element was not written (or is NaN)"
    assert bool((big[:MARGIN] == PATTERN).all()) and bool((big[-MARGIN:] == PATTERN).all()), what + ": wrote outside its buffer"


def traced(fn):
    _lib.trace_reset(); _lib.trace_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in _lib.trace_records()]
    finally:
        _lib.trace_enable(False)


def up(a, dev, reps=1):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.repeat(reps, *([1] * (t.dim() - 1))).contiguous() if reps > 1 else t


def note(table, key, value):
    table[key] = max(table.get(key, 0.0), float(value))


def first_bad(bad, what, err, bound):
    idx = tuple(int(v) for v in torch.nonzero(bad)[0])
    return "%s: %d of %d elements outside the bound, first at %s: error %.3e, bound %.3e" % (
        what, int(bad.sum()), bad.numel(), idx, float(err[idx]), float(bound[idx]))


def elements_ok(got, ref, mag, nprod):
    """(ok, largest ratio, message) of the per-element criterion; got may hold `reps` copies of the reference's batch."""
    g = got.double().to(ref.device).reshape(-1, *ref.shape)
    err = (g - ref).abs()
    bound = (ST.gamma(nprod) * mag).expand_as(err)
    zero = bound == 0
    if bool((g[zero] != 0).any()):
        return False, float("inf"), "an element with sum|a||b| = 0 is not exactly 0"
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    bad = err > bound
    return not bool(bad.any()), ratio, first_bad(bad, "per element", err, bound) if bool(bad.any()) else ""


def check_elements(got, ref, mag, nprod, key):
    ok, ratio, msg = elements_ok(got, ref, mag, nprod)
    note(ELEM, key, ratio)
    assert ok, "%s: %s" % (key, msg)


def stats_ok(s, y):
    """(ok, r1, r2, message): s [2, c] float64 sums of the partial rows against the kernel's own output y [..., c]."""
    c = y.shape[-1]
    y64 = y.double().reshape(-1, c)
    m = y64.shape[0]
    sq = y64 * y64
    e1, e2 = (s[0] - y64.sum(0)).abs(), (s[1] - sq.sum(0)).abs()
    b1, b2 = ST.gamma(m) * y64.abs().sum(0), ST.gamma(m + 1) * sq.sum(0)
    r = [float((e[b > 0] / b[b > 0]).max()) if bool((b > 0).any()) else 0.0 for e, b in ((e1, b1), (e2, b2))]
    bad1, bad2 = e1 > b1, e2 > b2
    msg = ""
    if bool(bad1.any()):
        msg = first_bad(bad1, "S1 per channel", e1, b1)
    elif bool(bad2.any()):
        msg = first_bad(bad2, "S2 per channel", e2, b2)
    return not msg, r[0], r[1], msg


def check_stats(stats, y, key):
    ok, r1, r2, msg = stats_ok(stats.double().sum(-1), y)
    note(SUMS, (key[0], "S1", key[2]), r1)
    note(SUMS, (key[0], "S2", key[2]), r2)
    assert ok, "%s: %s" % (key, msg)


def check_bnsums(part, dx, bn_np, bn_dev, act, key, reps):
    """The BatchNorm-backward partial rows against stream_ref.bn_sums of the kernel's own dx."""
    e, scale, shift, mean, rstd = bn_dev
    ref = ST.bn_sums(dx, e, scale, shift, mean, rstd, act)
    n0 = dx.shape[0] // reps
    if reps > 1:                                           # the copies of the batch are computed alike: E32 of one copy, reps times
        assert torch.equal(dx.reshape(reps, n0, *dx.shape[1:]), dx[:n0].unsqueeze(0).expand(reps, n0, *dx.shape[1:])), key
    dxc = dx[:n0].cpu()
    d64, t64 = ST.bn_terms(dxc, *bn_np, act)
    d32, t32 = ST.bn_terms(dxc, *bn_np, act, dtype=torch.float32)
    e32 = [reps * (a.double() - b).abs().sum((0, 1, 2)).to(dx.device) for a, b in ((d32, d64), (t32, t64))]
    m = dx.numel() // dx.shape[-1]
    assert float(ref.border.double().mean((0, 1, 2)).max()) <= 1e-3, key
    s = part.double().sum(-1)
    bb = (ref.b1, ref.b2) if act == 1 else (torch.zeros_like(ref.b1), torch.zeros_like(ref.b2))
    for i, (want, g, mg) in enumerate(((ref.s1, ST.gamma(m), ref.m1), (ref.s2, ST.gamma(m + 3), ref.m2))):
        err = (s[i] - want).abs()
        bound = g * mg + 4 * e32[i] + bb[i]
        den = g * mg + e32[i]
        assert bool((err[den == 0] == 0).all()), key
        if bool((den > 0).any()):
            note(SUMS, (key[0], "bn%d act%d" % (i + 1, act), key[2]), (err[den > 0] / den[den > 0]).max())
        bad = err > bound
        assert not bool(bad.any()), "%s: %s" % (key, first_bad(bad, "BN sum %d per channel" % (i + 1), err, bound))


def cdiv(a, b):
    return -(-a // b)


# ---- depthwise --------------------------------------------------------------------------------------------------------------------------
ROW, TILE, S2 = "embnet::dwconv_row4_kernel", "embnet::dwt::dw_tile_kernel", "embnet::dwconv_dgrad4_s2_row_kernel"


def dw_wide(ow):
    return ow >= 7 and cdiv(ow, 8) * 8 <= cdiv(ow, 4) * 4 + ow // 8


def stats_rows_of(units):
    """rows of partials of a statistics variant that walks `units` thread units (dw_stats_chunks, dw_block_accumulate) -> (rows, L)."""
    grid = cdiv(units, 256)
    chunks = cdiv(grid, 2048) if grid > 2048 else 1
    return cdiv(grid, chunks), chunks


# (n, h, w, c, r, s, stride, pads or None = Keras 'same', reps, forward / data-gradient kernel at stride 1 or None = generic fallback,
#  weight-gradient kernel)
WAVE, TWG, WG4, WG1 = "embnet::dwconv_wgrad4_wave_kernel", "embnet::dwt::dw_tile_wgrad_kernel", "embnet::dwconv_wgrad4_kernel", "embnet::dwconv_wgrad1_kernel"
DW_CASES = [
    (2, 9, 9, 24, 3, 3, 1, None, 1, ROW, WAVE), (2, 10, 13, 40, 5, 5, 1, None, 1, ROW, WAVE),                 # row4x2, four columns
    (2, 15, 15, 24, 5, 5, 1, None, 1, ROW, WAVE), (2, 34, 34, 16, 3, 3, 1, None, 1, ROW, WAVE),               # row4x2, eight columns
    (3, 15, 17, 96, 3, 3, 2, None, 1, ROW, WAVE), (2, 14, 14, 240, 5, 5, 2, None, 1, ROW, WAVE),              # stride 2, odd pad_l
    (2, 16, 16, 32, 3, 3, 2, None, 1, ROW, WAVE), (2, 15, 15, 32, 5, 5, 2, None, 1, ROW, WAVE),               # stride 2, even pad_l
    (2, 1, 9, 16, 3, 3, 1, None, 1, TILE, TWG), (2, 1, 9, 24, 3, 3, 1, None, 1, ROW, WAVE), (2, 2, 9, 16, 3, 3, 2, None, 1, ROW, WAVE),   # OH == 1
    (2, 6, 6, 1040, 3, 3, 2, None, 1, ROW, WAVE), (2, 34, 34, 1040, 5, 5, 1, None, 1, ROW, WAVE),            # c / 4 > 256
    (5, 14, 14, 64, 5, 5, 1, None, 1, TILE, TWG), (6, 7, 7, 96, 5, 5, 1, None, 1, TILE, TWG),                 # tile kernels
    (3, 28, 28, 48, 5, 5, 1, None, 1, TILE, TWG), (2, 30, 30, 48, 5, 5, 1, None, 1, TILE, WAVE),
    (3, 14, 14, 32, 5, 5, 1, (1, 3), 1, TILE, TWG), (3, 14, 14, 24, 5, 5, 1, (1, 3), 1, ROW, WAVE),           # asymmetric pads
    (2, 9, 9, 6, 3, 3, 1, None, 1, None, WG1), (2, 9, 9, 8, 3, 5, 1, None, 1, None, WG4), (2, 9, 9, 8, 7, 7, 1, None, 1, None, WG4),   # fallbacks
    # more than 2048 * 256 thread units: L > 1 in dw_block_accumulate (row4x2 STATS 1 and 2; the stride-2 data gradient's STATS 2);
    # the batch is `reps` copies of eight images, so the references are those of eight
    (8, 12, 12, 1044, 3, 3, 1, None, 14, ROW, WAVE), (8, 12, 12, 1044, 3, 3, 2, None, 7, ROW, WAVE),
]


def dw_id(case):
    n, h, w, c, r, s, st, pads, reps = case[:9]
    return "%dx%dx%dx%d_k%dx%d_s%d%s" % (n * reps, h, w, c, r, s, st, "" if pads is None else "_p%d%d" % pads)


@pytest.mark.parametrize("case", DW_CASES, ids=dw_id)
def test_depthwise_kernels_per_element_and_per_channel(dev, case):
    lib = _lib.lib()
    n0, h, w, c, r, s, st, pads, reps, kfwd, kwg = case
    n = n0 * reps
    oh, pt = ST.same_pads(h, r, st)
    ow, pl = ST.same_pads(w, s, st)
    if pads is not None:
        pt, pl = pads
    big_case = reps > 1
    rdev = dev if n0 * h * w * c > (1 << 18) else torch.device("cpu")
    rows_path = kfwd is not None
    fwd_name = kfwd or "embnet::dwconv_fwd_kernel"
    dgrad_name = (S2 if st == 2 else kfwd) if rows_path else "embnet::dwconv_dgrad_kernel"
    for family in FAMILIES:
        x_np, w_np, dy_np = ST.dw_operands(family, n0, h, w, c, r, s, oh, ow, seed=h * 100 + c)
        bn_np = ST.bn_operands(family, n0, h, w, c, seed=h * 100 + c)
        x, dy = up(x_np, dev, reps), up(dy_np, dev, reps)
        wt = up(w_np, dev)
        xr, wr, dyr = (torch.from_numpy(a).to(rdev) for a in (x_np, w_np, dy_np))
        tag = "tile" if kfwd == TILE else ("row" if rows_path else "generic")

        # ---- forward, and forward with the statistics
        yb, y = guarded((n, oh, ow, c), dev)
        names = traced(lambda: check(lib.embnet_dwconv2d_fwd_f32(x.data_ptr(), wt.data_ptr(), y.data_ptr(), n, h, w, c, r, s, st, pt, pl, oh, ow, stream())))
        assert names == [fwd_name], names
        assert_guard(yb, y, "forward")
        check_elements(y, ST.dw_fwd(xr, wr, st, pt, pl, oh, ow), ST.dw_fwd_mag(xr, wr, st, pt, pl, oh, ow), r * s, (tag + " fwd", "fwd", family))
        rows = lib.embnet_dwconv2d_fwd_stats_rows(n, c, r, s, st, oh, ow)
        if rows_path and kfwd == ROW:
            want_rows, chunks = stats_rows_of(n * cdiv(oh, 2) * cdiv(ow, 8 if dw_wide(ow) else 4) * (c // 4)) if oh >= 2 else (0, 1)
            assert rows == want_rows, (rows, want_rows)
            assert not (big_case and st == 1) or chunks > 1
        assert rows > 0 or not rows_path or oh < 2, rows
        if rows > 0:
            sb, stats = guarded((2, c, rows), dev)
            y2b, y2 = guarded((n, oh, ow, c), dev)
            names = traced(lambda: check(lib.embnet_dwconv2d_fwd_stats_f32(x.data_ptr(), wt.data_ptr(), y2.data_ptr(), n, h, w, c, r, s, st, pt, pl, oh, ow,
                                                                           stats.data_ptr(), stream())))
            assert names == [fwd_name], names
            assert_guard(y2b, y2, "forward with statistics"); assert_guard(sb, stats, "statistics partials")
            assert torch.equal(y2, y), "the output with statistics differs from the output without"
            check_stats(stats, y, (tag + " fwd stats", "stats", family))
            del y2b, y2
        del yb, y

        # ---- weight gradient (twice: bit-identical)
        ws = None if big_case else torch.empty(max(lib.embnet_dwconv2d_wgrad_workspace_bytes(n, c, r, s, oh, ow) // 4, 4), device=dev)
        outs = []
        for _ in range(0 if big_case else 2):
            wb, dw = guarded((r, s, c, 1), dev)
            names = traced(lambda: check(lib.embnet_dwconv2d_wgrad_f32(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                                                       n, h, w, c, r, s, st, pt, pl, oh, ow, stream())))
            assert names == [kwg, "embnet::dw_slab_sum_kernel"], names
            assert_guard(wb, dw, "weight gradient")
            outs.append(dw)
        if outs:
            assert torch.equal(outs[0], outs[1])
            check_elements(outs[0], ST.dw_wgrad(xr, dyr, r, s, st, pt, pl), ST.dw_wgrad_mag(xr, dyr, r, s, st, pt, pl), n * oh * ow,
                           (kwg.split("::")[-1].replace("_kernel", ""), "wgrad", family))

        if family == "relu":                               # the forward input's family only
            continue
        # ---- data gradient, and data gradient with the BatchNorm-backward sums
        dxb, dx = guarded((n, h, w, c), dev)
        names = traced(lambda: check(lib.embnet_dwconv2d_dgrad_f32(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), n, h, w, c, r, s, st, pt, pl, oh, ow, stream())))
        assert names == [dgrad_name], names
        assert_guard(dxb, dx, "data gradient")
        dtag = "s2row" if (rows_path and st == 2) else tag
        check_elements(dx, ST.dw_dgrad(dyr, wr, (n0, h, w, c), st, pt, pl), ST.dw_dgrad_mag(dyr, wr, (n0, h, w, c), st, pt, pl), r * s,
                       (dtag + " dgrad", "dgrad", family))
        brows = lib.embnet_dwconv2d_dgrad_bnsums_rows(n, h, w, c, r, s, st)
        if rows_path and st == 2:
            want_rows, chunks = stats_rows_of(n * h * cdiv(w, 4) * (c // 4))
            assert brows == want_rows and (not big_case or chunks > 1), (brows, want_rows, chunks)
        elif rows_path and kfwd == ROW:
            want_rows, chunks = stats_rows_of(n * cdiv(h, 2) * cdiv(w, 8 if dw_wide(w) else 4) * (c // 4)) if h >= 2 else (0, 1)
            assert brows == want_rows and (not big_case or chunks > 1), (brows, want_rows, chunks)
        if brows > 0:
            bn_dev = tuple(up(a, dev, reps if i == 0 else 1) for i, a in enumerate(bn_np))
            for act in (1, 2):
                pb, part = guarded((2, c, brows), dev)
                d2b, dx2 = guarded((n, h, w, c), dev)
                names = traced(lambda: check(lib.embnet_dwconv2d_dgrad_bnsums_f32(
                    dy.data_ptr(), wt.data_ptr(), dx2.data_ptr(), n, h, w, c, r, s, st, pt, pl, oh, ow, bn_dev[0].data_ptr(), bn_dev[1].data_ptr(),
                    bn_dev[2].data_ptr(), bn_dev[3].data_ptr(), bn_dev[4].data_ptr(), act, part.data_ptr(), brows, stream())))
                assert names == [dgrad_name], names
                assert_guard(d2b, dx2, "data gradient with sums"); assert_guard(pb, part, "BatchNorm-backward partials")
                assert torch.equal(dx2, dx), "the data gradient with sums differs from the one without"
                check_bnsums(part, dx, bn_np, bn_dev, act, (dtag + " dgrad sums", "bn", family), reps)
                del d2b, dx2
        del dxb, dx


# ---- thin 1x1 ---------------------------------------------------------------------------------------------------------------------------
def thin_rdev(dev, n, h, w, k):
    return dev if n * h * w * k > (1 << 18) else torch.device("cpu")


THIN_FWD = [(3, 17, 15, 16, 96, 1), (2, 9, 11, 24, 144, 1), (5, 7, 7, 40, 240, 1), (2, 5, 5, 4, 1024, 1), (2, 5, 5, 4, 8, 1), (1, 1, 1, 16, 96, 1),
            (5, 112, 112, 16, 96, 1), (3, 13, 10, 12, 40, 2)]


@pytest.mark.parametrize("n,h,w,cin,cout,st", THIN_FWD)
def test_thin_forward_per_element_and_per_channel(dev, n, h, w, cin, cout, st):
    lib = _lib.lib()
    oh, ow = cdiv(h, st), cdiv(w, st)
    rdev = thin_rdev(dev, n, oh, ow, cout)
    rows = lib.embnet_conv2d_fwd_stats_rows(n, cin, 1, 1, cout, oh, ow)
    assert lib.embnet_conv1x1_thin_supported(cin, cout) == 1 and rows > 0
    for family in FAMILIES:
        ops = ST.thin_operands(family, n, h, w, cin, cout, st, seed=h + cin)
        x, wt, _, bias, res = (up(a, dev) for a in ops)
        xr, wr, _, br, rr = (torch.from_numpy(a).to(rdev) for a in ops)
        plain = None
        for variant in ("plain", "stats", "epilogue"):
            ep = variant == "epilogue"
            yb, y = guarded((n, oh, ow, cout), dev)
            sb, stats = guarded((2, cout, rows), dev) if variant != "plain" else (None, None)
            names = traced(lambda: check(lib.embnet_conv2d_fwd_f32_ex(
                x.data_ptr(), wt.data_ptr(), bias.data_ptr() if ep else None, y.data_ptr(), n, h, w, cin, 1, 1, cout, st, 0, 0, oh, ow, 1 if ep else 0,
                res.data_ptr() if ep else None, None, None, 0, None if stats is None else stats.data_ptr(), None, 0, None, None, stream())))
            assert names == ["embnet::thin::thin_gemm_kernel"], names
            assert_guard(yb, y, "thin forward " + variant)
            if ep:
                ref, mag, npr = ST.thin_fwd(xr, wr, br, True, rr, st), ST.thin_fwd_mag(xr, wr, br, True, rr, st), cin + 2
            else:
                ref, mag, npr = ST.thin_fwd(xr, wr, stride=st), ST.thin_fwd_mag(xr, wr, stride=st), cin
            check_elements(y, ref, mag, npr, ("thin_gemm fwd" + (" epilogue" if ep else ""), "fwd", family))
            if variant == "plain":
                plain = y
            elif variant == "stats":
                assert torch.equal(y, plain), "the output with statistics differs from the output without"
            if stats is not None:
                assert_guard(sb, stats, "thin statistics partials")
                check_stats(stats, y, ("thin_gemm fwd stats" + (" epilogue" if ep else ""), "stats", family))


@pytest.mark.parametrize("n,h,w,c,k", [(3, 17, 15, 96, 16), (2, 9, 11, 144, 24), (5, 7, 7, 240, 40)])
def test_thin_data_gradient_per_element(dev, n, h, w, c, k):
    lib = _lib.lib()
    for family in FAMILIES[:4]:
        ops = ST.thin_operands(family, n, h, w, c, k, 1, seed=h + k)
        _, wt, dy = (up(a, dev) for a in ops[:3])
        dxb, dx = guarded((n, h, w, c), dev)
        names = traced(lambda: check(lib.embnet_conv2d_dgrad_f32_ex(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), n, h, w, c, 1, 1, k, 1, 0, 0, h, w, 0, None,
                                                                    None, 0, None, None, stream())))
        assert names == ["embnet::thin::thin_gemm_kernel"], names
        assert_guard(dxb, dx, "thin data gradient")
        wr, dyr = torch.from_numpy(ops[1]), torch.from_numpy(ops[2])
        check_elements(dx, ST.thin_dgrad(dyr, wr, (n, h, w, c)), ST.thin_dgrad_mag(dyr, wr, (n, h, w, c)), k, ("thin_gemm dgrad", "dgrad", family))


# every thin_wgrad_kernel<RQ> in both orientations (x thin, dy thin): thin sides 4 .. 20 (one row group) and 24, 32, 40 (two); wide side 8
# (slots clamped to the tile) and 1016 (the widest the kernel takes: see the docstring); stride 2; several workgroups with a ragged last tile
THIN_WGRAD = ([(2, 9, 11, t, 96, 1) for t in (4, 8, 12, 16, 20, 24, 32, 40)] + [(2, 9, 11, 96, t, 1) for t in (4, 8, 12, 16, 20, 24, 32, 40)] +
              [(2, 9, 11, 4, 8, 1), (2, 9, 11, 8, 4, 1), (2, 9, 11, 8, 1016, 1), (2, 9, 11, 1016, 8, 1), (2, 9, 11, 4, 1016, 1),
               (3, 13, 10, 12, 40, 2), (3, 13, 10, 40, 12, 2), (130, 14, 14, 24, 144, 1)])


@pytest.mark.parametrize("n,h,w,c,k,st", THIN_WGRAD)
def test_thin_weight_gradient_per_element(dev, n, h, w, c, k, st):
    lib = _lib.lib()
    oh, ow = cdiv(h, st), cdiv(w, st)
    ws = torch.empty(max(lib.embnet_conv2d_wgrad_workspace_bytes(n, c, 1, 1, k, oh, ow) // 4, 4), device=dev)
    if (n, c, k) == (130, 24, 144):
        assert lib.embnet_conv2d_wgrad_splits(n, c, 1, 1, k, oh, ow) > 1
    for family in FAMILIES:
        ops = ST.thin_operands(family, n, h, w, c, k, st, seed=c + k)
        x, _, dy = (up(a, dev) for a in ops[:3])
        outs = []
        for _ in range(2):
            wb, dw = guarded((1, 1, c, k), dev)
            names = traced(lambda: check(lib.embnet_conv2d_wgrad_f32_ex(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel() * 4, n, h, w, c,
                                                                        1, 1, k, st, 0, 0, oh, ow, None, None, 0, None, None, stream())))
            assert names and names[0] == "embnet::thinw::thin_wgrad_kernel", names
            assert_guard(wb, dw, "thin weight gradient")
            outs.append(dw)
        assert torch.equal(outs[0], outs[1])
        xr, dyr = torch.from_numpy(ops[0]), torch.from_numpy(ops[2])
        check_elements(outs[0], ST.thin_wgrad(xr, dyr, st), ST.thin_wgrad_mag(xr, dyr, st), n * oh * ow,
                       ("thin_wgrad " + ("x thin" if c < k else "dy thin"), "wgrad", family))


# ---- the guard --------------------------------------------------------------------------------------------------------------------------
def test_the_old_metric_is_blind_to_a_quiet_channel(dev):
    """A reference made WRONG on purpose — one border tap dropped in the quietest channel; one partial row counted twice — passes
    the neighbouring tests' metric (max error / max |reference| < 1e-5; sums within 1e-5 of the largest channel) against the correct
    kernel, and fails this file's per-element and per-channel criteria; the right reference passes both."""
    lib = _lib.lib()
    n, h, w, c, k = 2, 9, 9, 24, 3
    x_np, w_np, _ = ST.dw_operands("spread17", n, h, w, c, k, k, h, w, seed=h * 100 + c)
    x, wt = up(x_np, dev), up(w_np, dev)
    y = torch.empty(n, h, w, c, device=dev)
    rows = lib.embnet_dwconv2d_fwd_stats_rows(n, c, k, k, 1, h, w)
    stats = torch.empty(2, c, rows, device=dev)
    check(lib.embnet_dwconv2d_fwd_stats_f32(x.data_ptr(), wt.data_ptr(), y.data_ptr(), n, h, w, c, k, k, 1, 1, 1, h, w, stats.data_ptr(), stream()))
    torch.cuda.synchronize()
    xr, wr = torch.from_numpy(x_np), torch.from_numpy(w_np)
    ref, mag = ST.dw_fwd(xr, wr, 1, 1, 1, h, w), ST.dw_fwd_mag(xr, wr, 1, 1, 1, h, w)
    amp = ref.abs().amax((0, 1, 2))
    quiet = int(torch.where(amp > 0, amp, torch.full_like(amp, float("inf"))).argmin())
    assert float(amp[quiet] / amp.max()) < 1e-5
    quiet_share = float((amp < 1e-5 * amp.max()).double().mean())
    # the dropped tap: kernel row 1 (the image's own first row), column 2 (input column 1), at every output of row 0, column 0
    wrong = ref.clone()
    wrong[:, 0, 0, quiet] -= xr[:, 0, 1, quiet].double() * wr[1, 2, quiet, 0].double()
    old = lambda got, want: float((got.double().cpu() - want).abs().max() / want.abs().max())      # noqa: E731
    assert old(y, ref) < 1e-5 and old(y, wrong) < 1e-5
    assert elements_ok(y, ref, mag, k * k)[0]
    ok, ratio, msg = elements_ok(y, wrong, mag, k * k)
    assert not ok and ratio > 1e3, (ok, ratio)
    # one partial row of the quietest channel counted twice
    s = stats.double().sum(-1)
    twice = s.clone()
    live = int(stats[0, quiet].abs().argmax())
    twice[:, quiet] += stats[:, quiet, live].double()
    y64 = y.double()
    s1, a1, s2 = y64.sum((0, 1, 2)), y64.abs().sum((0, 1, 2)), (y64 * y64).sum((0, 1, 2))
    old_sums = lambda t: (float((t[0] - s1).abs().max()) <= 1e-5 * float(a1.max()) and float((t[1] - s2).abs().max()) <= 1e-5 * float(s2.max()))      # noqa: E731
    assert old_sums(s) and old_sums(twice)
    assert stats_ok(s, y)[0] and not stats_ok(twice, y)[0]
    print("\nblind-metric guard: quietest channel %d at %.1e of the loudest (%.0f %% of the channels below 1e-5); dropped tap: old metric %.1e, "
          "per-element ratio %.1e; row counted twice: old metric passes, per-channel fails" % (quiet, float(amp[quiet] / amp.max()), 100 * quiet_share,
                                                                                               old(y, wrong), ratio))


def test_zz_print_the_measured_tables():
    """Not an assertion of its own: prints what the tests above measured (pytest -s), for the docstring."""
    def table(data, title):
        rowsk = sorted({k[:2] for k in data})
        lines = [title, "  %-34s" % "kernel / quantity" + "".join("%15s" % f for f in FAMILIES)]
        for rk in rowsk:
            cells = ["%15s" % ("%.3f" % data[rk + (f,)] if rk + (f,) in data else "-") for f in FAMILIES]
            lines.append("  %-34s" % " ".join(rk) + "".join(cells))
        return "\n".join(lines)
    print("\n" + table(ELEM, "largest |kernel - float64| / (gamma(n) sum|a||b|)"))
    print("\n" + table(SUMS, "largest |S - reference| / bound (S1, S2) and / (gamma mag + E32) (bn1, bn2)"))
