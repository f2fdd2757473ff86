"""tests/stream_ref.py against torch, on the CPU:

  (a) every reference equals float64 torch autograd of F.conv2d / matmul to 1e-12 (k 3 and 5, stride 1 and 2, odd and even sizes,
      Keras-'same' and asymmetric pads, r != s), and every *_mag twin is the same operation on absolute values;
  (b) the FLOAT32 CPU evaluation of each operation stays inside every bound tests/test_stream_kernels_elementwise_gpu.py asserts of
      the kernels, for every input family: the bounds are not tight for a correct fp32 implementation.  Printed (pytest -s), largest
      |float32 - float64| over the bound, all families:
        depthwise 5x5 stride 2 forward / gamma(25) mag   0.13        thin 16 -> 96 forward / gamma(16) mag      0.43
        depthwise data gradient / gamma(25) mag          0.19        thin forward + bias, residual / gamma(18)  0.37
        depthwise weight gradient / gamma(M) mag         0.015       thin data gradient / gamma(96) mag         0.13
        per-channel S1 / gamma(M) sum|y|                 0.005       thin weight gradient / gamma(M) mag        0.017
        per-channel S2 / gamma(M + 1) sum y^2            0.012       BatchNorm-backward sums / their bound      0.005
        elements with mag == 0                           exactly 0
  (c) the ReLU-borderline mask of stream_ref.bn_sums selects at most 0.1 % of the elements of any channel, for every family and both
      activations (the cap the GPU test asserts as well).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_ref as ST  # noqa: E402

T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()      # noqa: E731


def _close(got, want, what):
    err = float((got - want).abs().max())
    assert err <= 1e-12 * max(float(want.abs().max()), 1e-300), (what, err)


def _conv_dw(x, w, stride, pad_t, pad_l, oh, ow):
    """F.conv2d depthwise with explicit top / left pads and output size (enough zeros below / right, then cropped)."""
    n, h, wd, c = x.shape
    r, s = w.shape[0], w.shape[1]
    pb = max((oh - 1) * stride + r - pad_t - h, 0)
    pr = max((ow - 1) * stride + s - pad_l - wd, 0)
    xt = F.pad(x.permute(0, 3, 1, 2), (pad_l, pr, pad_t, pb))
    y = F.conv2d(xt, w.reshape(r, s, c).permute(2, 0, 1).unsqueeze(1), stride=stride, groups=c)
    return y[:, :, :oh, :ow].permute(0, 2, 3, 1)


# (h, w, r, s, stride, pad_t, pad_l) — None pads: Keras 'same'
DW_GEOMS = [(9, 9, 3, 3, 1, None, None), (10, 13, 5, 5, 1, None, None), (15, 17, 3, 3, 2, None, None), (14, 14, 5, 5, 2, None, None),
            (16, 16, 3, 3, 2, None, None), (15, 15, 5, 5, 2, None, None), (14, 14, 5, 5, 1, 1, 3), (9, 11, 3, 3, 2, 2, 0),
            (9, 9, 3, 5, 1, None, None), (1, 9, 3, 3, 1, None, None), (2, 9, 3, 3, 2, None, None), (9, 9, 7, 7, 1, None, None)]


@pytest.mark.parametrize("h,w,r,s,stride,pad_t,pad_l", DW_GEOMS)
def test_depthwise_references_equal_conv2d_autograd(h, w, r, s, stride, pad_t, pad_l):
    n, c = 2, 6
    oh, pt = ST.same_pads(h, r, stride)
    ow, pl = ST.same_pads(w, s, stride)
    if pad_t is not None:
        pt, pl = pad_t, pad_l
    x, kern, dy = (T(a) for a in ST.dw_operands("spread10", n, h, w, c, r, s, oh, ow, seed=3))
    xr, wr = x.clone().requires_grad_(True), kern.clone().requires_grad_(True)
    y = _conv_dw(xr, wr, stride, pt, pl, oh, ow)
    y.backward(dy)
    _close(ST.dw_fwd(x, kern, stride, pt, pl, oh, ow), y.detach(), "fwd")
    _close(ST.dw_dgrad(dy, kern, x.shape, stride, pt, pl), xr.grad, "dgrad")
    _close(ST.dw_wgrad(x, dy, r, s, stride, pt, pl), wr.grad, "wgrad")
    xa, wa = x.abs().requires_grad_(True), kern.abs().requires_grad_(True)
    ya = _conv_dw(xa, wa, stride, pt, pl, oh, ow)
    _close(ST.dw_fwd_mag(x, kern, stride, pt, pl, oh, ow), ya.detach(), "fwd mag")
    gx, _ = torch.autograd.grad(ya, (xa, wa), dy.abs(), retain_graph=True)
    _close(ST.dw_dgrad_mag(dy, kern, x.shape, stride, pt, pl), gx, "dgrad mag")
    _close(ST.dw_wgrad_mag(x, dy, r, s, stride, pt, pl), torch.autograd.grad(ya, wa, dy.abs())[0], "wgrad mag")


@pytest.mark.parametrize("h,w,cin,cout,stride", [(17, 15, 16, 96, 1), (9, 11, 24, 12, 1), (13, 10, 12, 40, 2), (1, 1, 16, 8, 1)])
def test_thin_references_equal_conv2d_autograd(h, w, cin, cout, stride):
    x, kern, dy, bias, res = (T(a) for a in ST.thin_operands("spread10", 2, h, w, cin, cout, stride, seed=4))
    wt = lambda k: k.reshape(cin, cout).t().reshape(cout, cin, 1, 1)      # noqa: E731
    conv = lambda xx, kk: F.conv2d(xx.permute(0, 3, 1, 2), wt(kk), stride=stride).permute(0, 2, 3, 1)      # noqa: E731
    xr, wr = x.clone().requires_grad_(True), kern.clone().requires_grad_(True)
    y = conv(xr, wr)
    y.backward(dy)
    _close(ST.thin_fwd(x, kern, stride=stride), y.detach(), "fwd")
    _close(ST.thin_fwd(x, kern, bias, True, res, stride), torch.relu(y.detach() + bias) + res, "fwd epilogue")
    _close(ST.thin_dgrad(dy, kern, x.shape, stride), xr.grad, "dgrad")
    _close(ST.thin_wgrad(x, dy, stride), wr.grad, "wgrad")
    xa, wa = x.abs().requires_grad_(True), kern.abs().requires_grad_(True)
    ya = conv(xa, wa)
    _close(ST.thin_fwd_mag(x, kern, bias, True, res, stride), ya.detach() + bias.abs() + res.abs(), "fwd mag")
    gx, gw = torch.autograd.grad(ya, (xa, wa), dy.abs())
    _close(ST.thin_dgrad_mag(dy, kern, x.shape, stride), gx, "dgrad mag")
    _close(ST.thin_wgrad_mag(x, dy, stride), gw, "wgrad mag")


@pytest.mark.parametrize("act", [0, 1, 2])
def test_bn_sums_equal_autograd(act):
    """sum dz and sum dz ehat are the gradients of beta and gamma of z = gamma ehat + beta (= scale e + shift)."""
    n, h, w, c = 3, 7, 5, 8
    e, scale, shift, mean, rstd = (T(a) for a in ST.bn_operands("spread10", n, h, w, c, seed=5))
    dx = T(ST.dw_operands("spread10", n, h, w, c, 3, 3, h, w, seed=5)[2])
    gam = (scale / rstd).requires_grad_(True)
    beta = (shift + mean * scale).requires_grad_(True)
    z = gam * ((e - mean) * rstd) + beta
    a = torch.relu(z) if act == 1 else (z * torch.sigmoid(z) if act == 2 else z)
    (a * dx).sum().backward()
    got = ST.bn_sums(dx, e, scale, shift, mean, rstd, act)
    _close(got.s1, beta.grad, "sum dz")
    _close(got.s2, gam.grad, "sum dz ehat")
    dz, t2 = ST.bn_terms(dx, e, scale, shift, mean, rstd, act)
    _close(got.m1, dz.abs().sum((0, 1, 2)), "sum |dz|")
    _close(got.m2, t2.abs().sum((0, 1, 2)), "sum |dz ehat|")
    _close(got.mdx, dx.abs().sum((0, 1, 2)), "sum |dx|")
    assert ST.gamma(1) == 2.0 ** -24 / (1 - 2.0 ** -24) and abs(ST.gamma(25) / (25 * 2.0 ** -24) - 1) < 1e-5


# ---- (b): float32 on the CPU inside the bounds the kernels are held to ------------------------------------------------------------------
WORST = {}


def _ratio(name, got32, ref, mag, nprod):
    """largest |float32 - float64| / (gamma(n) mag); elements with mag == 0 must be exactly 0."""
    got = got32.double()
    zero = mag == 0
    assert bool((got[zero] == 0).all()), name
    r = float(((got - ref).abs()[~zero] / (ST.gamma(nprod) * mag[~zero])).max()) if bool((~zero).any()) else 0.0
    WORST[name] = max(WORST.get(name, 0.0), r)
    return r


def _stats_ratio(name, y32):
    """the per-channel sum and sum of squares of a float32 tensor, added in float32, against float64 sums of the same values."""
    c = y32.shape[-1]
    y = y32.reshape(-1, c)
    m = y.shape[0]
    y64 = y.double()
    s1, s2 = y.sum(0).double(), (y * y).sum(0).double()
    b1, b2 = ST.gamma(m) * y64.abs().sum(0), ST.gamma(m + 1) * (y64 * y64).sum(0)
    e1, e2 = (s1 - y64.sum(0)).abs(), (s2 - (y64 * y64).sum(0)).abs()
    assert bool((e1[b1 == 0] == 0).all()) and bool((e2[b2 == 0] == 0).all()), name
    r1 = float((e1[b1 > 0] / b1[b1 > 0]).max())
    r2 = float((e2[b2 > 0] / b2[b2 > 0]).max())
    WORST[name + " S1"] = max(WORST.get(name + " S1", 0.0), r1)
    WORST[name + " S2"] = max(WORST.get(name + " S2", 0.0), r2)
    return r1, r2


@pytest.mark.parametrize("family", ST.FAMILIES)
def test_float32_cpu_stays_inside_the_kernel_bounds(family):
    f32 = torch.float32
    # depthwise 5x5 stride 2
    n, h, w, c, k, st = 4, 14, 14, 24, 5, 2
    oh, pt = ST.same_pads(h, k, st)
    ow, pl = ST.same_pads(w, k, st)
    x, kern, dy = ST.dw_operands(family, n, h, w, c, k, k, oh, ow, seed=1)
    y32 = ST.dw_fwd(x, kern, st, pt, pl, oh, ow, dtype=f32)
    rs = [_ratio("dw fwd", y32, ST.dw_fwd(x, kern, st, pt, pl, oh, ow), ST.dw_fwd_mag(x, kern, st, pt, pl, oh, ow), k * k),
          _ratio("dw dgrad", ST.dw_dgrad(dy, kern, x.shape, st, pt, pl, dtype=f32), ST.dw_dgrad(dy, kern, x.shape, st, pt, pl),
                 ST.dw_dgrad_mag(dy, kern, x.shape, st, pt, pl), k * k),
          _ratio("dw wgrad", ST.dw_wgrad(x, dy, k, k, st, pt, pl, dtype=f32), ST.dw_wgrad(x, dy, k, k, st, pt, pl),
                 ST.dw_wgrad_mag(x, dy, k, k, st, pt, pl), n * oh * ow)]
    rs += list(_stats_ratio("dw", y32))
    # thin 16 -> 96 and its data gradient (a 96 -> 16 project conv's)
    x, kern, dy, bias, res = ST.thin_operands(family, 3, 17, 15, 16, 96, 1, seed=2)
    t32 = ST.thin_fwd(x, kern, dtype=f32)
    rs += [_ratio("thin fwd", t32, ST.thin_fwd(x, kern), ST.thin_fwd_mag(x, kern), 16),
           _ratio("thin fwd epilogue", ST.thin_fwd(x, kern, bias, True, res, dtype=f32), ST.thin_fwd(x, kern, bias, True, res),
                  ST.thin_fwd_mag(x, kern, bias, True, res), 18),
           _ratio("thin dgrad", ST.thin_dgrad(dy, kern, x.shape, dtype=f32), ST.thin_dgrad(dy, kern, x.shape),
                  ST.thin_dgrad_mag(dy, kern, x.shape), 96),
           _ratio("thin wgrad", ST.thin_wgrad(x, dy, dtype=f32), ST.thin_wgrad(x, dy), ST.thin_wgrad_mag(x, dy), 3 * 17 * 15)]
    rs += list(_stats_ratio("thin", t32))
    # the BatchNorm-backward sums: float32 terms added in float32, against the bound with E32 of those very terms
    n, h, w, c = 4, 14, 14, 24
    e, scale, shift, mean, rstd = ST.bn_operands(family, n, h, w, c, seed=1)
    dx = ST.dw_operands(family, n, h, w, c, 3, 3, h, w, seed=6)[2]
    m = n * h * w
    for act in (1, 2):
        ref = ST.bn_sums(dx, e, scale, shift, mean, rstd, act)
        d64, t64 = ST.bn_terms(dx, e, scale, shift, mean, rstd, act)
        d32, t32b = ST.bn_terms(dx, e, scale, shift, mean, rstd, act, dtype=f32)
        e1, e2 = (d32.double() - d64).abs().sum((0, 1, 2)), (t32b.double() - t64).abs().sum((0, 1, 2))
        bb = (ref.b1, ref.b2) if act == 1 else (0.0, 0.0)
        for s32, s64, g, mg, ee, b in ((d32.sum((0, 1, 2)), ref.s1, ST.gamma(m), ref.m1, e1, bb[0]),
                                       (t32b.sum((0, 1, 2)), ref.s2, ST.gamma(m + 3), ref.m2, e2, bb[1])):
            bound = g * mg + 4 * ee + b
            err = (s32.double() - s64).abs()
            assert bool((err[bound == 0] == 0).all())
            r = float((err[bound > 0] / bound[bound > 0]).max())
            WORST["bn sums"] = max(WORST.get("bn sums", 0.0), r)
            rs.append(r)
    print("\n%-16s float32 CPU / bound: " % family + " ".join("%.3f" % r for r in rs))
    assert max(rs) < 1.0, rs


def test_print_the_largest_float32_ratios():
    print("\nlargest float32 CPU / bound over the families run: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert all(v < 1.0 for v in WORST.values())


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ST.FAMILIES)
@pytest.mark.parametrize("act", [1, 2])
def test_relu_borderline_mask_is_rare(family, act):
    for (n, h, w, c) in [(2, 9, 9, 24), (4, 14, 14, 24), (2, 34, 34, 16)]:
        e, scale, shift, mean, rstd = ST.bn_operands(family, n, h, w, c, seed=0)
        dx = ST.dw_operands(family, n, h, w, c, 3, 3, h, w, seed=0)[2]
        frac = ST.bn_sums(dx, e, scale, shift, mean, rstd, act).border.double().mean((0, 1, 2))
        assert float(frac.max()) <= 1e-3, (family, act, (n, h, w, c), float(frac.max()))
