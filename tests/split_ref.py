"""NumPy restatement of the two-piece fp16 format of the conv kernels (include/embnet.h, PRECISION; csrc/gemm_engine.h).  No kernel
code: this file is the header's paragraph, written down a second time, so that a kernel can be held against it element by element.

  x = (h1 + h2) / s,  s a power of two per tensor that puts a bound B >= max |x| into [2^14, 2^15);
  h1 = fp16(x s), h2 = fp16(x s - h1), both rounded to nearest even, subnormals kept;
  a product keeps h1 h1' + h1 h2' + h2 h1' and is multiplied by 1 / s and 1 / s'.

Tensors are NumPy arrays in the library's layouts: activations / gradients NHWC, kernels RSCK.  A GEOMETRY names the pass and says
which two tensors are the operands, in the order of the C entry points:

  fwd    (x [n,h,w,c],    w [r,s,c,k])   -> y  [n,oh,ow,k]
  dgrad  (dy [n,oh,ow,k], w [r,s,c,k])   -> dx [n,h,w,c]        (out_shape = x's shape)
  wgrad  (x [n,h,w,c],    dy [n,oh,ow,k]) -> dw [r,s,c,k]       (out_shape = w's shape)

The second half of the file makes the INPUT FAMILIES the CPU and the GPU test share (tests/test_split_ref_cpu.py,
tests/test_three_product_elementwise_gpu.py) and the amplitude-binned envelope both print.
"""
from collections import namedtuple

import numpy as np
import torch

Geometry = namedtuple("Geometry", "kind stride pad out_shape")          # pad: zero padding on every side; out_shape: see above


# ---- the scale ---------------------------------------------------------------------------------------------------------------------
def scale_exponent(bound):
    """k with s = 2^k: bound * s lands in [2^14, 2^15).  0 for a zero, infinite or NaN bound; |k| <= 126 (s and 1 / s stay normal)."""
    b = abs(float(np.float32(bound)))
    if b == 0.0 or not np.isfinite(b):
        return 0
    _, e = np.frexp(b)                                  # b = m 2^e, m in [0.5, 1): b in [2^(e-1), 2^e)
    return int(min(max(15 - int(e), -126), 126))


def scale_of(bound):
    return float(np.ldexp(1.0, scale_exponent(bound)))


# ---- the split ---------------------------------------------------------------------------------------------------------------------
def split(x, s):
    """(h1, h2) as np.float16: the two pieces of float32(x) * float32(s)."""
    with np.errstate(over="ignore", invalid="ignore"):
        xs = np.asarray(x, dtype=np.float32) * np.float32(s)
        h1 = xs.astype(np.float16)
        h2 = (xs - h1.astype(np.float32)).astype(np.float16)
    return h1, h2


# ---- float64 (or float32) convolutions of the three passes ------------------------------------------------------------------------------
def conv(a, b, geom, dtype=torch.float64):
    """The pass `geom` names on operands (a, b), computed by torch on the CPU in `dtype`; returns float64 NumPy."""
    ta = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).permute(0, 3, 1, 2)
    if geom.kind == "fwd":
        tb = torch.from_numpy(np.ascontiguousarray(b)).to(dtype).permute(3, 2, 0, 1)
        out = torch.nn.functional.conv2d(ta, tb, stride=geom.stride, padding=geom.pad).permute(0, 2, 3, 1)
    elif geom.kind == "dgrad":
        tb = torch.from_numpy(np.ascontiguousarray(b)).to(dtype).permute(3, 2, 0, 1)
        n, h, w, c = geom.out_shape
        out = torch.nn.grad.conv2d_input((n, c, h, w), tb, ta, stride=geom.stride, padding=geom.pad).permute(0, 2, 3, 1)
    elif geom.kind == "wgrad":
        tb = torch.from_numpy(np.ascontiguousarray(b)).to(dtype).permute(0, 3, 1, 2)
        r, s, c, k = geom.out_shape
        out = torch.nn.grad.conv2d_weight(ta, (k, c, r, s), tb, stride=geom.stride, padding=geom.pad).permute(2, 3, 1, 0)
    else:
        raise ValueError(geom.kind)
    return out.double().numpy()


def model_conv(a_pieces, b_pieces, s_a, s_b, geom, terms=(True, True, True), flush_h2=False):
    """float64 sum of exactly the kept products h1 h1' + h1 h2' + h2 h1', times 1 / (s_a s_b).
    `terms` / `flush_h2` exist for ONE purpose: to make the model wrong on purpose (drop a term; flush subnormal h2 to zero) and
    see the per-element test fail where the per-tensor tests stay green."""
    a1, a2 = (np.asarray(p, dtype=np.float16).astype(np.float64) for p in a_pieces)
    b1, b2 = (np.asarray(p, dtype=np.float16).astype(np.float64) for p in b_pieces)
    if flush_h2:
        tiny = 2.0 ** -14
        a2 = np.where(np.abs(a2) < tiny, 0.0, a2)
        b2 = np.where(np.abs(b2) < tiny, 0.0, b2)
    acc = 0.0
    for on, (pa, pb) in zip(terms, ((a1, b1), (a1, b2), (a2, b1))):
        if on:
            acc = acc + conv(pa, pb, geom)
    return acc * (1.0 / float(s_a)) * (1.0 / float(s_b))


def mag(a, b, geom):
    """sum |a| |b| of every output element."""
    return conv(np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64)), geom)


def operand_error(x, s):
    """eps(x) = max(2^-22 |x|, 2^-25 / s): what PRECISION allows one operand element."""
    return np.maximum(np.abs(np.asarray(x, np.float64)) * 2.0 ** -22, 2.0 ** -25 / float(s))


def format_bound(a, b, s_a, s_b, geom):
    """Per-element error the header allows the FORMAT (not a kernel: no accumulation error):
    conv(eps_a, |b|) + conv(|a|, eps_b) + conv(eps_a, eps_b) + conv(|h2_a|, |h2_b|) / (s_a s_b)."""
    a64, b64 = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    ea, eb = operand_error(a, s_a), operand_error(b, s_b)
    h2a = np.abs(split(a, s_a)[1].astype(np.float64))
    h2b = np.abs(split(b, s_b)[1].astype(np.float64))
    dropped = conv(h2a, h2b, geom) * (1.0 / float(s_a)) * (1.0 / float(s_b))
    return conv(ea, b64, geom) + conv(a64, eb, geom) + conv(ea, eb, geom) + dropped


# ---- the amplitude-binned envelope ---------------------------------------------------------------------------------------------------
def depth(a, b, bound_a, bound_b, geom, magv=None):
    """Per output element: how many binades the operand elements that contribute to it lie below their tensor's bound — the
    weighted mean over the element's own products, log2(bound_a sum |b| / sum |a||b|) for the first operand and likewise for the
    second, the deeper of the two.  This is the quantity the format's floor scales with: an operand element on the subnormal floor
    carries 2^-39 bound absolute, so the element's floor error / sum |a||b| is 2^(depth - 39).  (The loudest element of a slice says
    less: log-normal gradients put most elements of a loud image far below its maximum.)  inf where sum |a||b| = 0."""
    m = mag(a, b, geom) if magv is None else magv
    return depth_from(reach(a, b, geom), bound_a, bound_b, m)


def reach(a, b, geom):
    """(sum |b|, sum |a|) over each output element's products: what depth() needs beside the bounds (independent of them)."""
    a64, b64 = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    return conv(np.ones_like(a64), b64, geom), conv(a64, np.ones_like(b64), geom)


def depth_from(reach_ab, bound_a, bound_b, m):
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.maximum(np.log2(float(bound_a) * reach_ab[0] / m), np.log2(float(bound_b) * reach_ab[1] / m))
    return np.where(m > 0, d, np.inf)


BIN = 4                                                   # binades per bin


def envelope(err, magv, dep, into=None):
    """{bin: max err / mag over the elements whose depth is in [4 bin, 4 bin + 4)}; mag == 0 elements are left out.  `into`: merge."""
    out = {} if into is None else into
    dep = np.broadcast_to(dep, magv.shape)
    ok = (magv > 0) & np.isfinite(dep)
    if ok.any():
        ratio = err[ok] / magv[ok]
        bins = np.floor(np.maximum(dep[ok], 0) / BIN).astype(np.int64)
        for bn in np.unique(bins):
            out[int(bn)] = max(out.get(int(bn), 0.0), float(ratio[bins == bn].max()))
    return out


def format_envelope_rows(rows):
    """rows: {label: {bin: value}} -> text table, one line per bin."""
    labels = list(rows)
    bins = sorted({b for r in rows.values() for b in r})
    lines = ["binades below the bound | " + " | ".join(labels)]
    for b in bins:
        cells = [("%.1e" % rows[l][b]) if b in rows[l] else "-" for l in labels]
        lines.append(("%3d .. %3d" % (BIN * b, BIN * b + BIN)).ljust(23) + " | " + " | ".join(cells))
    return "\n".join(lines)


# ---- the input families ------------------------------------------------------------------------------------------------------------
FAMILIES = ["even", "spread10", "spread17", "spread20", "quiet_image17", "quiet_image20", "quiet_filters17", "quiet_filters20",
            "zero", "relu"]
LOOSE = [1.0, 8.0, 64.0]                                  # activation bound / true maximum


def operands(family, n, h, w, c, k, ks, stride, pad, gmag=1e-3, seed=0, pad_channel=False):
    """(x [n,h,w,c], kern [ks,ks,c,k], dy [n,oh,ow,k]) float32 of one family (n >= 2).
    even            randn activations, He-scaled kernel, log-normal gradients of magnitude gmag (what the neighbouring tests use);
    spreadS         per-channel amplitude 2^(-S u_c) on x, u_c uniform in [0, 1], one channel at full amplitude;
    quiet_imageS    the last image of the batch 2^-S below the others, in x and in dy;
    quiet_filtersS  per-filter amplitude 2^(-S u_k) on dy, one filter at full amplitude;
    zero            one channel and one image of x exactly zero, one image and one filter of dy exactly zero (a dead ReLU channel);
    relu            x = relu(randn): half zeros throughout.
    pad_channel: the last input channel is the zero pad of a widened image (the stem)."""
    g = torch.Generator().manual_seed(seed * 1009 + FAMILIES.index(family))
    oh, ow = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    x = torch.randn(n, h, w, c, generator=g)
    kern = torch.randn(ks, ks, c, k, generator=g) * (2.0 / (ks * ks * c)) ** 0.5
    dy = torch.randn(n, oh, ow, k, generator=g) * gmag * torch.exp(2 * torch.randn(n, oh, ow, k, generator=g))
    live = c - 1 if pad_channel else c
    if family.startswith("spread"):
        u = torch.rand(c, generator=g)
        u[int(torch.randint(0, live, (1,), generator=g))] = 0.0
        x = x * torch.exp2(-float(family[6:]) * u)
    elif family.startswith("quiet_image"):
        sp = float(family[11:])
        x[-1] *= 2.0 ** -sp
        dy[-1] *= 2.0 ** -sp
    elif family.startswith("quiet_filters"):
        u = torch.rand(k, generator=g)
        u[int(torch.randint(0, k, (1,), generator=g))] = 0.0
        dy = dy * torch.exp2(-float(family[13:]) * u)
    elif family == "zero":
        x[..., live // 2] = 0.0
        x[0] = 0.0
        dy[0] = 0.0
        dy[..., k // 3] = 0.0
    elif family == "relu":
        x = torch.relu(x)
    if pad_channel:
        x[..., -1] = 0.0
        kern[:, :, -1, :] = 0.0
    return x.numpy().copy(), kern.numpy().copy(), dy.numpy().copy()


def pass_operands(kind, x, kern, dy):
    """(a, b, out_shape) of a pass, in the entry points' operand order."""
    if kind == "fwd":
        return x, kern, None
    if kind == "dgrad":
        return dy, kern, x.shape
    return x, dy, kern.shape


# ---- decoding the planes buffers (include/embnet.h, FORMAT OF THE PLANES) ------------------------------------------------------------
def _planes_and_scale(raw16):
    flat = np.asarray(raw16).view(np.uint16).reshape(3, -1)
    s, inv = flat[2][:4].view(np.float32)[:2]
    assert s > 0 and s * inv == 1.0 and np.log2(s) == np.round(np.log2(s)), (s, inv)
    return flat[0].view(np.float16), flat[1].view(np.float16), float(s)


def decode_planes(raw16, m, c):
    """planes of an activation / gradient, 16-bit [3][c/16][m][16] -> (h1 [m, c], h2 [m, c] as np.float16, s)."""
    p1, p2, s = _planes_and_scale(raw16)
    back = lambda p: p.reshape(c // 16, m, 16).transpose(1, 0, 2).reshape(m, c)       # noqa: E731
    return back(p1), back(p2), s


def decode_weight_planes(raw16, shape, flip):
    """planes of a kernel w [r,s,c,k], 16-bit [3][r][red/16][s][rows][16] -> (h1, h2 as np.float16 in w's own [r,s,c,k] order, s).
    flip 0: rows = k, reduction = c; flip 1: rows = c, reduction = k, taps flipped."""
    r, s_, c, k = shape
    p1, p2, s = _planes_and_scale(raw16)

    def back(p):
        if flip:
            q = p.reshape(r, k // 16, s_, c, 16)                     # [r'][kc][s'][c][j] = w[r-1-r', s-1-s', c, 16 kc + j]
            return q.transpose(0, 2, 3, 1, 4).reshape(r, s_, c, k)[::-1, ::-1]
        q = p.reshape(r, c // 16, s_, k, 16)                         # [r][cc][s][k][j] = w[r, s, 16 cc + j, k]
        return q.transpose(0, 2, 1, 4, 3).reshape(r, s_, c, k)
    return back(p1), back(p2), s
