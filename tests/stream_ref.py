"""float64 references of the STREAMING kernels — depthwise convolution (csrc/mbconv_kernels.hip, csrc/dwconv_tile.hip) and the thin
1x1 convolution (csrc/conv_thin.hip) — written with shifted slices and einsum, NOT with F.conv2d, so that they share nothing with the
references of the neighbouring tests (tests/test_stream_ref_cpu.py holds them against torch autograd once).  No kernel code.

Tensors are torch tensors (or NumPy arrays) in the library's layouts, on the CPU or — for the one or two large cases — on the GPU:
activations / gradients NHWC, depthwise kernels [r,s,c,1], 1x1 kernels [1,1,c,k].  Geometry as the C ABI takes it: explicit top /
left pads and output size.  Every function takes `dtype` (float64; float32 = the same operation evaluated in fp32, the yardstick
for 'a correct fp32 implementation') and has a `*_mag` twin: sum |a||b| of every output element (+ |bias| + |residual| where they
enter), the quantity the textbook bound gamma(n) * mag is written in (Higham, Accuracy and Stability, 3.1: any order of n
products / additions).

The second half makes the INPUT FAMILIES (split_ref.operands and, for depthwise layers, per-channel amplitudes in the kernel and
the gradient as well) and the BatchNormalization in front of a depthwise layer.
"""
import os
import sys
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as SR  # noqa: E402

U = 2.0 ** -24                                             # unit roundoff of fp32


def gamma(n):
    return n * U / (1.0 - n * U)


def _t(a, dtype, like=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if like is not None:
        t = t.to(like.device)
    return t.to(dtype)


# ---- depthwise ------------------------------------------------------------------------------------------------------------------------
def _canvas(h, w, r, s, stride, pad_t, pad_l, oh, ow):
    """Size of the zero-padded image that holds every tap of every output: rows pad_t .. pad_t + h - 1 are the image."""
    return max(pad_t + h, (oh - 1) * stride + r), max(pad_l + w, (ow - 1) * stride + s)


def _window(t, a, b, stride, oh, ow):
    return t[:, a:a + (oh - 1) * stride + 1:stride, b:b + (ow - 1) * stride + 1:stride, :]


def dw_fwd(x, w, stride, pad_t, pad_l, oh, ow, dtype=torch.float64):
    """y[n,oh,ow,c] = sum_{r,s} x[n, oh st + r - pad_t, ow st + s - pad_l, c] w[r,s,c]  (taps outside the image are zero)."""
    x = _t(x, dtype)
    w = _t(w, dtype, x)
    n, h, wd, c = x.shape
    r, s = w.shape[0], w.shape[1]
    w = w.reshape(r, s, c)
    hp, wp = _canvas(h, wd, r, s, stride, pad_t, pad_l, oh, ow)
    xp = torch.zeros(n, hp, wp, c, dtype=dtype, device=x.device)
    xp[:, pad_t:pad_t + h, pad_l:pad_l + wd] = x
    y = torch.zeros(n, oh, ow, c, dtype=dtype, device=x.device)
    for a in range(r):
        for b in range(s):
            y += _window(xp, a, b, stride, oh, ow) * w[a, b]
    return y


def dw_dgrad(dy, w, xshape, stride, pad_t, pad_l, dtype=torch.float64):
    """dx[n,ih,iw,c] = sum over (r,s,oh,ow) with oh st + r - pad_t = ih, ow st + s - pad_l = iw of dy[n,oh,ow,c] w[r,s,c]."""
    dy = _t(dy, dtype)
    w = _t(w, dtype, dy)
    n, h, wd, c = xshape
    oh, ow = dy.shape[1], dy.shape[2]
    r, s = w.shape[0], w.shape[1]
    w = w.reshape(r, s, c)
    hp, wp = _canvas(h, wd, r, s, stride, pad_t, pad_l, oh, ow)
    dxp = torch.zeros(n, hp, wp, c, dtype=dtype, device=dy.device)
    for a in range(r):
        for b in range(s):
            _window(dxp, a, b, stride, oh, ow).add_(dy * w[a, b])
    return dxp[:, pad_t:pad_t + h, pad_l:pad_l + wd].contiguous()


def dw_wgrad(x, dy, r, s, stride, pad_t, pad_l, dtype=torch.float64):
    """dw[r,s,c,1] = sum_{n,oh,ow} x[n, oh st + r - pad_t, ow st + s - pad_l, c] dy[n,oh,ow,c]."""
    x = _t(x, dtype)
    dy = _t(dy, dtype, x)
    n, h, wd, c = x.shape
    oh, ow = dy.shape[1], dy.shape[2]
    hp, wp = _canvas(h, wd, r, s, stride, pad_t, pad_l, oh, ow)
    xp = torch.zeros(n, hp, wp, c, dtype=dtype, device=x.device)
    xp[:, pad_t:pad_t + h, pad_l:pad_l + wd] = x
    dw = torch.zeros(r, s, c, 1, dtype=dtype, device=x.device)
    for a in range(r):
        for b in range(s):
            dw[a, b, :, 0] = (_window(xp, a, b, stride, oh, ow) * dy).sum((0, 1, 2))
    return dw


def _abs(a):
    return np.abs(a) if isinstance(a, np.ndarray) else a.abs()


def dw_fwd_mag(x, w, stride, pad_t, pad_l, oh, ow):
    return dw_fwd(_abs(x), _abs(w), stride, pad_t, pad_l, oh, ow)


def dw_dgrad_mag(dy, w, xshape, stride, pad_t, pad_l):
    return dw_dgrad(_abs(dy), _abs(w), xshape, stride, pad_t, pad_l)


def dw_wgrad_mag(x, dy, r, s, stride, pad_t, pad_l):
    return dw_wgrad(_abs(x), _abs(dy), r, s, stride, pad_t, pad_l)


# ---- thin 1x1 -----------------------------------------------------------------------------------------------------------------------
def thin_fwd(x, w, bias=None, relu=False, residual=None, stride=1, dtype=torch.float64):
    """relu(x . W + b) + residual, the composition csrc/conv_thin.hip documents; output pixel (oh, ow) reads input (oh st, ow st)."""
    x = _t(x, dtype)
    w = _t(w, dtype, x).reshape(x.shape[-1], -1)
    y = torch.einsum("nhwc,ck->nhwk", x[:, ::stride, ::stride], w)
    if bias is not None:
        y = y + _t(bias, dtype, x)
    if relu:
        y = torch.clamp_min(y, 0)
    if residual is not None:
        y = y + _t(residual, dtype, x)
    return y


def thin_fwd_mag(x, w, bias=None, relu=False, residual=None, stride=1):
    """sum |x||W| + |b| + |residual|  (|relu(a) - relu(b)| <= |a - b|: the ReLU adds nothing)."""
    return thin_fwd(_abs(x), _abs(w), None if bias is None else _abs(bias), False, None if residual is None else _abs(residual), stride)


def thin_dgrad(dy, w, xshape, stride=1, dtype=torch.float64):
    """dx[n, oh st, ow st, c] = sum_k dy[n,oh,ow,k] W[c,k]; input pixels no output reads get zero."""
    dy = _t(dy, dtype)
    n, h, wd, c = xshape
    w = _t(w, dtype, dy).reshape(c, -1)
    dx = torch.zeros(n, h, wd, c, dtype=dtype, device=dy.device)
    dx[:, ::stride, ::stride] = torch.einsum("nhwk,ck->nhwc", dy, w)
    return dx


def thin_dgrad_mag(dy, w, xshape, stride=1):
    return thin_dgrad(_abs(dy), _abs(w), xshape, stride)


def thin_wgrad(x, dy, stride=1, dtype=torch.float64):
    """dw[1,1,c,k] = sum_{n,oh,ow} x[n, oh st, ow st, c] dy[n,oh,ow,k]."""
    x = _t(x, dtype)
    dy = _t(dy, dtype, x)
    return torch.einsum("nhwc,nhwk->ck", x[:, ::stride, ::stride], dy).reshape(1, 1, x.shape[-1], dy.shape[-1])


def thin_wgrad_mag(x, dy, stride=1):
    return thin_wgrad(_abs(x), _abs(dy), stride)


# ---- the BatchNorm-backward sums a data-gradient kernel emits ---------------------------------------------------------------------------
def bn_terms(dx, e, scale, shift, mean, rstd, act, dtype=torch.float64):
    """(dz, dz * ehat) per element in `dtype`: dz = dx * act'(scale e + shift), ehat = (e - mean) rstd; act 0 none, 1 ReLU, 2 swish."""
    dx = _t(dx, dtype)
    e, scale, shift, mean, rstd = (_t(v, dtype, dx) for v in (e, scale, shift, mean, rstd))
    z = e * scale + shift
    if act == 1:
        dz = torch.where(z > 0, dx, torch.zeros_like(dx))
    elif act == 2:
        sg = torch.sigmoid(z)
        dz = dx * (sg + z * sg * (1 - sg))
    else:
        dz = dx
    return dz, dz * ((e - mean) * rstd)


BnSums = namedtuple("BnSums", "s1 s2 m1 m2 mdx border b1 b2")


def bn_sums(dx, e, scale, shift, mean, rstd, act):
    """Per channel, float64: s1 = sum dz, s2 = sum dz ehat; their magnitudes m1 = sum |dz|, m2 = sum |dz ehat|, mdx = sum |dx|;
    border: the elements whose ReLU decision fp32 may take the other way, |z| <= 4u (|e scale| + |shift|); b1 / b2: sum |dx| and
    sum |dx ehat| over them (what a flipped decision moves)."""
    f = torch.float64
    dx = _t(dx, f)
    e, scale, shift, mean, rstd = (_t(v, f, dx) for v in (e, scale, shift, mean, rstd))
    dz, t2 = bn_terms(dx, e, scale, shift, mean, rstd, act)
    red = tuple(range(dx.dim() - 1))
    border = (e * scale + shift).abs() <= 4 * U * ((e * scale).abs() + shift.abs())
    ehat = (e - mean) * rstd
    zero = torch.zeros_like(dx)
    return BnSums(dz.sum(red), t2.sum(red), dz.abs().sum(red), t2.abs().sum(red), dx.abs().sum(red), border,
                  torch.where(border, dx.abs(), zero).sum(red), torch.where(border, (dx * ehat).abs(), zero).sum(red))


# ---- operand families -------------------------------------------------------------------------------------------------------------------
FAMILIES = SR.FAMILIES
GPU_FAMILIES = ["even", "spread17", "quiet_image17", "zero", "relu"]


def same_pads(size, k, stride):
    """(output size, leading pad) of Keras padding='same'."""
    out = -(-size // stride)
    return out, max((out - 1) * stride + k - size, 0) // 2


def _channel_amplitude(g, c, spread):
    u = torch.rand(c, generator=g)
    u[int(torch.randint(0, c, (1,), generator=g))] = 0.0
    return torch.exp2(-float(spread) * u)


def _gradient(family, g, shape, gmag=1e-3):
    """split_ref.operands' log-normal gradient with the family's treatment PER CHANNEL (the last axis plays the filters' part);
    the spread families, which leave dy alone there, spread it over the channels here as well."""
    dy = torch.randn(*shape, generator=g) * gmag * torch.exp(2 * torch.randn(*shape, generator=g))
    c = shape[-1]
    if family.startswith("spread"):
        dy = dy * _channel_amplitude(g, c, family[6:])
    elif family.startswith("quiet_image"):
        dy[-1] *= 2.0 ** -float(family[11:])
    elif family.startswith("quiet_filters"):
        dy = dy * _channel_amplitude(g, c, family[13:])
    elif family == "zero":
        dy[0] = 0.0
        dy[..., c // 3] = 0.0
    return dy


def dw_operands(family, n, h, w, c, r, s, oh, ow, seed=0):
    """(x [n,h,w,c], kern [r,s,c,1], dy [n,oh,ow,c]) float32 NumPy: x is split_ref.operands' x of the family; the kernel has a
    per-channel amplitude 2^(-12 u_c) of its own (one channel at full amplitude), so quiet channels exist in w as well as in x."""
    x = SR.operands(family, n, h, w, c, 1, 1, 1, 0, seed=seed)[0]
    g = torch.Generator().manual_seed(seed * 7919 + 31 * FAMILIES.index(family) + 5)
    kern = torch.randn(r, s, c, 1, generator=g) * (2.0 / (r * s)) ** 0.5 * _channel_amplitude(g, c, 12).reshape(1, 1, c, 1)
    dy = _gradient(family, g, (n, oh, ow, c))
    return x, kern.numpy().copy(), dy.numpy().copy()


def thin_operands(family, n, h, w, cin, cout, stride=1, seed=0):
    """(x, kern [1,1,cin,cout], dy, bias [cout], residual [n,oh,ow,cout]) float32 NumPy: split_ref.operands plus a bias and a
    residual (the spread families give the residual per-channel amplitudes, so the statistics of the sum have quiet channels)."""
    x, kern, dy = SR.operands(family, n, h, w, cin, cout, 1, stride, 0, seed=seed)
    g = torch.Generator().manual_seed(seed * 7919 + 31 * FAMILIES.index(family) + 11)
    bias = torch.randn(cout, generator=g) * 0.1
    res = torch.randn(*dy.shape, generator=g)
    if family.startswith("spread"):
        amp = _channel_amplitude(g, cout, family[6:])
        res, bias = res * amp, bias * amp
    elif family.startswith("quiet_image"):
        res[-1] *= 2.0 ** -float(family[11:])
    elif family == "zero":
        res[0] = 0.0
        res[..., cout // 3] = 0.0
        bias[cout // 3] = 0.0
    return x, kern, dy, bias.numpy().copy(), res.numpy().copy()


def bn_operands(family, n, h, w, c, seed=0):
    """The BatchNormalization in front of a depthwise layer, float32 NumPy: its input e (the family's x of another seed), its own
    batch mean / rstd of e (eps 1e-3), gamma in [0.5, 1.5], beta in [-0.3, 0.31] (never exactly 0: a dead channel's z = beta) and
    the folded scale = gamma rstd, shift = beta - mean scale the kernels read."""
    e = SR.operands(family, n, h, w, c, 1, 1, 1, 0, seed=seed + 101)[0]
    e64 = e.astype(np.float64).reshape(-1, c)
    mean = e64.mean(0)
    rstd = 1.0 / np.sqrt(e64.var(0) + 1e-3)
    gam, beta = np.linspace(0.5, 1.5, c), np.linspace(-0.3, 0.31, c)
    scale = gam * rstd
    shift = beta - mean * scale
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)      # noqa: E731
    return e, f(scale), f(shift), f(mean), f(rstd)
