"""float64 references and textbook rounding bounds of the layers BETWEEN the convolutions (csrc/nn_kernels.hip): BatchNormalization
forward / backward / inference, max pooling, the fused BN -> act -> pad -> pool stem, global average pooling.  Plain torch float64 on
the CPU, no kernel code; tests/test_nn_ref_cpu.py holds the float32 CPU evaluation of every formula against every bound, and
tests/test_nn_kernels_elementwise_gpu.py the kernels.  Both call the SAME check_* functions below: a check takes the operands and
the outputs (the kernel's, or the float32 stand-in's), raises AssertionError at the first element or channel outside its bound and
returns {quantity: largest error / bound}.

Bounds.  u = 2^-24, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability, 3.1: n roundings on the path of a term, any order).
Nothing is measured; the rounding counts are read off nn_kernels.hip.

  statistics, per channel, reduction length M (bn_stats*_kernel: one add per element for S1, one fma per element for S2, fp32
  partials added in double by bn_finalize_kernel — every order of M fp32 additions obeys the same bound):
      |S1 - sum x| <= gamma(M) sum|x|,  |S2 - sum x^2| <= gamma(M + 1) sum x^2
      |mean_k - mean| <= gamma(M) sum|x| / M + u |mean| =: Em                       (the division is in double; u: the cast to fp32)
      |var_k - var|  <= gamma(M + 1) E[x^2] + 2 |mean| gamma(M) E|x| + Em^2 + u var =: Ev        (var_k = S2 / M - (S1 / M)^2, cast)
      |rstd_k - rstd| <= rstd Ev / (2 (var + eps - Ev)) + u rstd =: Er.   With v = var + eps, f(v) = v^-1/2:
          f(v - E) - f(v) = E / ((sqrt v + sqrt(v - E)) sqrt v sqrt(v - E)) <= f(v) E / (2 (v - E)), and the other side is smaller.
          CONDITION Ev <= (var + eps) / 4: on the inputs, asserted for every family, shape and eps on the CPU and on the GPU.
      moving_mean: (1 - mom) Em + gamma(2) (|mom old| + |(1 - mom) mean|); moving_var likewise with Ev   (a product and the sum
          on each term's path; 1 - mom is exact for mom = 0.99f).  With mom = 0 the update returns (float)var_k itself: the GPU
          test makes that call too and asserts |var_k - var| <= Ev directly.
  scale, shift against float64 of the kernel's OWN fp32 save_mean / save_rstd:
      |scale - gamma rstd_k| <= u |.|,   |shift - (beta - mean_k scale)| <= 2 u (|beta| + |mean_k scale|)
  inference (bn_infer_prepare_kernel: fp32 add, the hardware's 1-ulp = 2 u reciprocal square root, a product: 0.5 u + 2 u + u):
      |scale - gamma (mv + eps)^-1/2| <= gamma(4) |.|, shift as above from the kernel's own scale
  y per element against float64 of the kernel's own scale / shift, z = x scale + shift (ONE fma):
      identity, ReLU   |y - act(z)| <= u |z|     (|relu(a) - relu(b)| <= |a - b|: a borderline z may take either side)
      swish            + 4 E32, E32 = kappa |z|, kappa = the largest |float32 CPU evaluation - float64| / |z| over the tensor.
          (The per-element |float32 - float64| is 0 by luck on some elements and so cannot bound ANOTHER fp32 implementation there;
          the tensor's largest relative figure can.  Every error of a swish scales with |z|: |swish(z)| <= |z|, |swish'| <= 1.1.
          Always measured against the reference, never against the kernel; 4 = the margin for the device's exp.)
  dbeta, dgamma per channel against stream_ref.bn_sums of (dy, x) and the kernel's own scale, shift, mean, rstd — the 'BN sums' form
  of tests/test_stream_kernels_elementwise_gpu.py:
      |dbeta_k - sum dz| <= gamma(M) sum|dz| + 4 E32 + B,  |dgamma_k - sum dz xhat| <= gamma(M + 3) sum|dz xhat| + 4 E32' + B'
      E32 = sum over the channel of |term in float32 on the CPU - term in float64| (swish; 0 otherwise); B, B' = sum |dy|, |dy xhat|
      over the channel's ReLU-borderline elements |z| <= 4 u (|x scale| + |shift|), at most 0.1 % of any channel (asserted).
      ((x - mean) 1, rstd 2, the product with dz and the add: one fma in bn_sums4, a product and an add in pool_bn_bwd_reduce4: 3.)
  dx per element against float64 of the kernel's own dbeta, dgamma, save_mean, save_rstd, scale:
      |dx_k - dx| <= gamma(7) |scale| (|dz| + |dbeta| / M + |xhat| |dgamma| / M)       bn_dx4: the longest path is xhat dgamma / M:
          x - mean (1), rstd (2), dgamma (3), the rounding of inv_m = 1.f / M itself (4), the product with it (5), the subtraction (6),
          scale (7); dz's path has 3, dbeta's 5.  Frozen statistics: dx = scale dz, ONE rounding.
      swish: + 4 |scale| kappa' |dy|, kappa' = the largest |float32 CPU act'(z) - float64| over the tensor (act' is O(1))
      ReLU-borderline elements may take either side; dx_add: the sum's rounding, u (|dx| + |dx_add|), on top.
      in-ReLU form (embnet_bn_bwd_inrelu): dz_out = dx [x > 0], same bound; dbias against the kernel's own dz_out: gamma(M) sum|dz_out|.
  pools: y bit-identical, argmax equal (the rule below); dx <= gamma(w - 1) sum|dy terms| over the w windows routed to the pixel:
      exactly equal for w <= 1, exactly 0 for w = 0.  embnet_maxpool_relu_bwd_colsum: dz = dx [y_in > 0], dbias as above.
  fused stem backward: the pooled gradient is routed by the forward's own argmax (w - 1 additions), then the BN formulas: the sums
      run over the M' = n oh ow POOLED elements, dx uses inv_m = 1 / (n h w): gamma(7 + max(w - 1, 0)) on the dx bound.
  GAP: forward gamma(hw + 1) mean|x| per (image, channel) (hw - 1 additions, inv = 1.f / hw and the product); backward two
      roundings: gamma(2) |dy| / hw; with dx_add gamma(3) |dy| / hw + u |dx_add|.
  zero channels: every bound above is a multiple of a magnitude sum; where that is 0 the value must be exactly 0.

The max-pool rule (nn_kernels.hip pool_scan4 / maxpool_fwd_kernel): taps outside the image compete as the VALUE 0 (ZeroPadding2D
in front of the pool), strict `>` from -inf, the first winner in row-major window order stays, tap byte dy k + dx, or 255 when a
padding zero won (it carries no gradient).  test_nn_ref_cpu.py pins it to oracle.backbones.maxpool (F.pad + max_pool2d + autograd).
"""
import os
import sys
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_ref as ST  # noqa: E402

U, gamma = ST.U, ST.gamma
F64, F32 = torch.float64, torch.float32
EPS_VALUES = (1e-3, 2e-5)                                  # Keras' default and the zoo ResNet's
MOMENTUM = 0.99


def f32(v):
    """The float a C `float` argument holds."""
    return float(np.float32(v))


def _t(a, dtype=F64):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.detach().cpu().to(dtype)


# ---- geometry of the column reductions (nn_kernels.hip col_geom) ------------------------------------------------------------------
ColGeom = namedtuple("ColGeom", "cl rl blocks rows_per_block")


def col_geom(m, c):
    """Mirror of col_geom(m, c): c = the channel count for the scalar kernels, the QUAD count c / 4 for the four-channel ones."""
    cl = 1
    while cl < c and cl < 256:
        cl <<= 1
    rl = 256 // cl
    blocks = -(-m // (rl * 16))
    if blocks < 512:
        blocks = min(-(-m // (rl * 4)), 512)
    blocks = max(min(blocks, 2048), 1)
    return ColGeom(cl, rl, blocks, -(-m // blocks))


def reduce_geom(m, c):
    """The geometry a BatchNorm reduction over [m, c] runs on and what it reaches: (ColGeom, the four-channel kernels, the LDS branch
    of col_reduce2_v4p (cl = 64 and up: no butterfly), trips of the column loop, rows of the last block)."""
    quad = c % 4 == 0
    cols = c // 4 if quad else c
    g = col_geom(m, cols)
    return g, quad, quad and g.cl >= 64, -(-cols // g.cl), m - (g.blocks - 1) * g.rows_per_block


# ---- operand families -----------------------------------------------------------------------------------------------------------------
BN_FAMILIES = ["even", "spread17", "zero", "relu", "offset8", "const"]
BnCase = namedtuple("BnCase", "x dy gamma beta mm mv")
CONST_VALUE = 0.06                                         # not a power of two: its partial sums round
OFFSET8_AMP = 0.25                                         # loudest channel of offset8: keeps Ev <= (var + eps) / 4 at m = 1, eps = 2e-5


def bn_case(family, m, c, seed=0):
    """Float32 torch tensors of one family over [m, c]:
    even      randn;                           spread17  randn x per-channel amplitudes over 2^17 (one channel at full amplitude);
    zero      channels 1, 5, 9, .. all zero;    relu      relu(randn);
    offset8   per-channel mean = 8 std, the sign alternating by channel, on spread17 amplitudes (x OFFSET8_AMP);
    const     channels 2, 6, 10, .. constant (var = 0, rstd = eps^-1/2), the others randn.
    dy is stream_ref._gradient of the family (per-channel amplitudes for the spread families; zero: row 0 and channel c // 3 zero);
    gamma in +-[0.5, 1.5] with every third entry negative, beta = 0.3 randn, moving statistics of the layer before the step."""
    g = torch.Generator().manual_seed(seed * 7919 + 131 * BN_FAMILIES.index(family) + 17 * m + c)
    x = torch.randn(m, c, generator=g)
    if family in ("spread17", "offset8"):
        amp = ST._channel_amplitude(g, c, 17)
        if family == "offset8":
            sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(c)])
            x = (x + 8.0 * sign) * (amp * OFFSET8_AMP)
        else:
            x = x * amp
    elif family == "zero":
        x[:, 1::4] = 0.0
    elif family == "relu":
        x = torch.relu(x)
    elif family == "const":
        x[:, 2::4] = CONST_VALUE
    dy = ST._gradient("spread17" if family == "offset8" else family, g, (m, c))
    gam = 0.5 + torch.rand(c, generator=g)
    gam[2::3] *= -1.0
    beta = 0.3 * torch.randn(c, generator=g)
    mm = 0.1 * torch.randn(c, generator=g)
    mv = 0.5 + torch.rand(c, generator=g)
    return BnCase(x.contiguous(), dy.contiguous(), gam, beta, mm, mv)


def affine(x, scale, shift, dtype):
    """z = x scale + shift: float64, or the ONE-rounding fp32 fma the kernels use (product and sum in double, then rounded: a
    24 x 24-bit product is exact there)."""
    z = _t(x) * _t(scale) + _t(shift)
    return z if dtype == F64 else z.to(F32)


# ---- checks ---------------------------------------------------------------------------------------------------------------------------
def within(err, bound, what):
    """Largest err / bound; AssertionError at the first element with err > bound (bound == 0: the value must be exact)."""
    err, bound = torch.broadcast_tensors(err, bound)
    assert bool(torch.isfinite(err).all()), what + ": not finite"
    bad = err > bound
    if bool(bad.any()):
        idx = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError("%s: %d of %d outside the bound, first at %s: error %.3e, bound %.3e" % (
            what, int(bad.sum()), bad.numel(), idx, float(err[idx]), float(bound[idx])))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def act_fwd(z, act, exp_form=False):
    if act == 1:
        return torch.clamp_min(z, 0)
    if act == 2:
        return z / (1 + torch.exp(-z)) if exp_form else z * torch.sigmoid(z)
    return z


def act_der(z, act, exp_form=False):
    if act == 1:
        return (z > 0).to(z.dtype)
    if act == 2:
        sg = 1 / (1 + torch.exp(-z)) if exp_form else torch.sigmoid(z)
        return sg + z * sg * (1 - sg)
    return torch.ones_like(z)


# ---- BatchNorm forward ---------------------------------------------------------------------------------------------------------------
BnStats = namedtuple("BnStats", "s1 a1 s2 mean var rstd Em Ev Er ok")


def bn_stats(x, eps):
    """Per channel, float64: sum x, sum |x|, sum x^2, mean, biased variance (two-pass), rstd and the bounds Em, Ev, Er of the
    module docstring; ok: the condition Ev <= (var + eps) / 4 per channel."""
    x = _t(x)
    m = x.shape[0]
    s1, a1, s2 = x.sum(0), x.abs().sum(0), (x * x).sum(0)
    mean = s1 / m
    var = ((x - mean) ** 2).sum(0) / m
    Em = gamma(m) * a1 / m + U * mean.abs()
    Ev = gamma(m + 1) * s2 / m + 2 * mean.abs() * gamma(m) * a1 / m + Em * Em + U * var
    v = var + eps
    rstd = v ** -0.5
    ok = Ev <= v / 4
    Er = rstd * Ev / (2 * (v - Ev).clamp_min(1e-300)) + U * rstd
    return BnStats(s1, a1, s2, mean, var, rstd, Em, Ev, Er, ok)


def bn_forward(case, eps, act, momentum=MOMENTUM, dtype=F64, stats_rows=None):
    """dict of save_mean, save_rstd, scale, shift, moving_mean, moving_var, y.  float64: the exact layer.  float32: the stand-in for a
    correct fp32 implementation, in the kernel's arithmetic: fp32 sums (stats_rows: that many row bands summed one by one, the
    by-channel partials of a conv epilogue), the finalize in double, fp32 results."""
    x = _t(case.x, dtype)
    m = x.shape[0]
    gam, beta, mm, mv = (_t(v, dtype) for v in (case.gamma, case.beta, case.mm, case.mv))
    if dtype == F64:
        st = bn_stats(x, eps)
        mean, var = st.mean, st.var
    else:
        p = partials(case.x, stats_rows or 1)
        mean = p[0].double().sum(-1) / m
        var = (p[1].double().sum(-1) / m - mean * mean).clamp_min(0)
    rstd = ((var + eps) ** -0.5).to(dtype)
    scale = gam * rstd
    shift = beta - mean.to(dtype) * scale
    mom = torch.tensor(f32(momentum), dtype=dtype)
    out = dict(save_mean=mean.to(dtype), save_rstd=rstd, scale=scale, shift=shift, moving_mean=mom * mm + (1 - mom) * mean.to(dtype),
               moving_var=mom * mv + (1 - mom) * var.to(dtype), y=act_fwd(affine(case.x, scale, shift, dtype), act, exp_form=dtype == F32))
    return out


def partials(x, rows):
    """[2][c][rows] float32: sum and sum of squares of `rows` bands of x's rows, each added in fp32 (the layout partial_in takes)."""
    x = _t(x, F32)
    bands = torch.tensor_split(x, rows, dim=0)
    return torch.stack([torch.stack([b.sum(0) for b in bands], -1), torch.stack([(b * b).sum(0) for b in bands], -1)]).contiguous()


def kappa_fwd(x, scale, shift, act):
    """Largest |float32 CPU act(z) - float64| / |z| over the tensor (0 unless swish); scale / shift: the fp32 values both use."""
    if act != 2:
        return 0.0
    z, z32 = affine(x, scale, shift, F64), affine(x, scale, shift, F32)
    err = (act_fwd(z32, 2).double() - act_fwd(z, 2)).abs()
    nz = z != 0
    return float((err[nz] / z[nz].abs()).max()) if bool(nz.any()) else 0.0


def kappa_der(x, scale, shift, act):
    """Largest |float32 CPU act'(z) - float64| over the tensor (0 unless swish)."""
    if act != 2:
        return 0.0
    z, z32 = affine(x, scale, shift, F64), affine(x, scale, shift, F32)
    return float((act_der(z32, 2).double() - act_der(z, 2)).abs().max())


def check_y(x, scale, shift, act, y, what):
    """y per element against float64 of the fp32 scale / shift it was formed from."""
    x, sc, sh, y = _t(x), _t(scale), _t(shift), _t(y)
    z = x * sc + sh
    bound = (U + 4 * kappa_fwd(x, scale, shift, act)) * z.abs()
    exact = ((x * sc).abs() + sh.abs()) == 0
    assert bool((y[exact.expand_as(y)] == 0).all()), what + ": an element with |x scale| + |shift| = 0 is not exactly 0"
    return within((y - act_fwd(z, act)).abs(), bound, what)


def check_bn_forward(case, eps, act, out, momentum=MOMENTUM, what="bn fwd"):
    """Every output of embnet_bn_train_fwd (a dict as bn_forward's; y may be missing) -> {quantity: largest error / bound}."""
    st = bn_stats(case.x, eps)
    assert bool(st.ok.all()), what + ": Ev <= (var + eps) / 4 does not hold for these inputs"
    o = {k: _t(v) for k, v in out.items()}
    gam, beta, mm, mv = (_t(v) for v in (case.gamma, case.beta, case.mm, case.mv))
    mom = f32(momentum)
    r = {}
    r["mean"] = within((o["save_mean"] - st.mean).abs(), st.Em, what + " mean")
    r["rstd"] = within((o["save_rstd"] - st.rstd).abs(), st.Er, what + " rstd")
    assert bool((o["save_mean"][st.a1 == 0] == 0).all()), what + ": the mean of an all-zero channel is not exactly 0"
    if "moving_mean" in o:
        r["moving_mean"] = within((o["moving_mean"] - (mom * mm + (1 - mom) * st.mean)).abs(),
                                  (1 - mom) * st.Em + gamma(2) * ((mom * mm).abs() + ((1 - mom) * st.mean).abs()), what + " moving_mean")
        r["moving_var"] = within((o["moving_var"] - (mom * mv + (1 - mom) * st.var)).abs(),
                                 (1 - mom) * st.Ev + gamma(2) * ((mom * mv).abs() + (1 - mom) * st.var), what + " moving_var")
    ref = gam * o["save_rstd"]
    r["scale"] = within((o["scale"] - ref).abs(), U * ref.abs(), what + " scale")
    ms = o["save_mean"] * o["scale"]
    r["shift"] = within((o["shift"] - (beta - ms)).abs(), 2 * U * (beta.abs() + ms.abs()), what + " shift")
    if "y" in o:
        r["y act%d" % act] = check_y(case.x, out["scale"], out["shift"], act, out["y"], what + " y")
    return r


def bn_infer(case, eps, act, dtype=F64):
    x, gam, beta, mm, mv = (_t(v, dtype) for v in (case.x, case.gamma, case.beta, case.mm, case.mv))
    scale = gam * ((mv + torch.tensor(eps, dtype=dtype)) ** -0.5)
    shift = beta - mm * scale
    return dict(scale=scale, shift=shift, y=act_fwd(affine(x, scale, shift, dtype), act, exp_form=dtype == F32))


def check_bn_infer(case, eps, act, out, what="bn infer"):
    o = {k: _t(v) for k, v in out.items()}
    gam, beta, mm, mv = (_t(v) for v in (case.gamma, case.beta, case.mm, case.mv))
    ref = gam * (mv + eps) ** -0.5
    r = {"infer scale": within((o["scale"] - ref).abs(), gamma(4) * ref.abs(), what + " scale")}
    ms = mm * o["scale"]
    r["infer shift"] = within((o["shift"] - (beta - ms)).abs(), 2 * U * (beta.abs() + ms.abs()), what + " shift")
    r["infer y act%d" % act] = check_y(case.x, out["scale"], out["shift"], act, out["y"], what + " y")
    return r


# ---- BatchNorm backward --------------------------------------------------------------------------------------------------------------
BORDER_CAP = 1e-3


def bn_backward(x, dy, state, act, training, dx_add=None, inrelu=False, inv_m=None, dtype=F64):
    """dict of dbeta, dgamma, dx (inrelu: dz = dx [x > 0] and dbias = its column sum) from the saved forward state
    (save_mean, save_rstd, scale, shift); float32: the stand-in, every product and sum rounded."""
    x, dy = _t(x, dtype), _t(dy, dtype)
    mean, rstd, sc, sh = (_t(state[k], dtype) for k in ("save_mean", "save_rstd", "scale", "shift"))
    m = x.shape[0]
    inv_m = torch.tensor(1.0 / m if inv_m is None else inv_m, dtype=dtype)
    dz = dy * act_der(affine(x, sc, sh, dtype), act, exp_form=dtype == F32) if act else dy
    xhat = (x - mean) * rstd
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    dx = sc * (dz - dbeta * inv_m - xhat * dgamma * inv_m) if training else sc * dz
    if dx_add is not None:
        dx = dx + _t(dx_add, dtype)
    out = dict(dbeta=dbeta, dgamma=dgamma, dx=dx)
    if inrelu:
        out["dx"] = torch.where(x > 0, dx, torch.zeros_like(dx))
        out["dbias"] = out["dx"].sum(0)
    return out


def check_bn_sums(x, dy, state, act, dbeta, dgamma, what, nround=3):
    """dbeta / dgamma per channel against stream_ref.bn_sums: the 'BN sums' form of the module docstring."""
    args = tuple(_t(state[k], F32) for k in ("scale", "shift", "save_mean", "save_rstd"))
    x, dy = _t(x, F32), _t(dy, F32)
    m = x.shape[0]
    ref = ST.bn_sums(dy, x, *args, act)
    assert float(ref.border.double().mean(0).max()) <= BORDER_CAP or act != 1, what + ": more than 0.1 % of a channel is ReLU-borderline"
    e32 = [torch.zeros_like(ref.s1)] * 2
    if act == 2:
        t64, t32 = ST.bn_terms(dy, x, *args, act), ST.bn_terms(dy, x, *args, act, dtype=F32)
        e32 = [(a.double() - b).abs().sum(0) for a, b in zip(t32, t64)]
    bb = (ref.b1, ref.b2) if act == 1 else (0.0, 0.0)
    r = {}
    for i, (name, got, want, g, mag) in enumerate((("dbeta", dbeta, ref.s1, gamma(m), ref.m1), ("dgamma", dgamma, ref.s2, gamma(m + nround), ref.m2))):
        r["%s act%d" % (name, act)] = within((_t(got) - want).abs(), g * mag + 4 * e32[i] + bb[i], "%s %s" % (what, name))
    return r


def check_dx(x, dz_in, dz_mag, state, act, training, dbeta, dgamma, dx, what, m=None, nround=7, dx_add=None, mask=None):
    """dx per element against float64 of the kernel's own dbeta / dgamma and saved state.  dz_in: the gradient in front of the
    activation's derivative (dy, or the routed pooled gradients), dz_mag: sum |terms| of it; m: the inv_m divisor; mask: in-ReLU."""
    x, dz_in, dz_mag, dx = _t(x), _t(dz_in), _t(dz_mag), _t(dx)
    mean, rstd, sc, sh = (_t(state[k]) for k in ("save_mean", "save_rstd", "scale", "shift"))
    db, dg = _t(dbeta), _t(dgamma)
    m = x.shape[0] if m is None else m
    z = x * sc + sh
    xhat = (x - mean) * rstd
    kd = kappa_der(x, state["scale"], state["shift"], act)

    def side(der):
        dz, mag = dz_in * der, dz_mag * der.abs()
        if training:
            ref = sc * (dz - db / m - xhat * dg / m)
            bound = gamma(nround) * sc.abs() * (mag + db.abs() / m + xhat.abs() * dg.abs() / m)
        else:
            ref, bound = sc * dz, gamma(max(nround - 6, 1)) * sc.abs() * mag
        bound = bound + 4 * kd * sc.abs() * dz_mag
        if dx_add is not None:
            a = _t(dx_add)
            ref, bound = ref + a, bound * (1 + U) + U * (ref.abs() + a.abs())
        if mask is not None:
            ref, bound = torch.where(mask, ref, torch.zeros_like(ref)), torch.where(mask, bound, torch.zeros_like(bound))
        return (dx - ref).abs(), bound

    err, bound = side(act_der(z, act))
    if act == 1:                                           # a borderline element may take either side
        border = z.abs() <= 4 * U * ((x * sc).abs() + sh.abs())
        e0, b0 = side(torch.zeros_like(z))
        e1, b1 = side(torch.ones_like(z))
        other = border & (err > bound)
        pick0 = other & (e0 <= b0)
        err, bound = torch.where(pick0, e0, torch.where(other, e1, err)), torch.where(pick0, b0, torch.where(other, b1, bound))
    return within(err, bound, what)


def check_bn_backward(case, state, act, training, out, dx_add=None, inrelu=False, what="bn bwd"):
    """Every output of embnet_bn_bwd / embnet_bn_bwd_inrelu -> {quantity: largest error / bound}."""
    r = check_bn_sums(case.x, case.dy, state, act, out["dbeta"], out["dgamma"], what)
    mask = _t(case.x) > 0 if inrelu else None
    key = "%s act%d" % (("dz inrelu" if inrelu else "dx") + ("" if training else " frozen") + (" +add" if dx_add is not None else ""), act)
    dy = _t(case.dy)
    r[key] = check_dx(case.x, dy, dy.abs(), state, act, training, out["dbeta"], out["dgamma"], out["dx"], what + " dx",
                      dx_add=dx_add, mask=mask)
    if inrelu:
        own = _t(out["dx"])
        r["dbias"] = within((_t(out["dbias"]) - own.sum(0)).abs(), gamma(own.shape[0]) * own.abs().sum(0), what + " dbias")
    return r


# ---- max pooling ----------------------------------------------------------------------------------------------------------------------
def pool_out(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


def _taps(h, w, k, stride, pad):
    """For every tap (dy, dx): (tap byte, input rows of the output rows, their validity, columns, validity)."""
    oh, ow = pool_out(h, k, stride, pad), pool_out(w, k, stride, pad)
    for a in range(k):
        for b in range(k):
            ih, iw = np.arange(oh) * stride + a - pad, np.arange(ow) * stride + b - pad
            yield a * k + b, ih, (ih >= 0) & (ih < h), iw, (iw >= 0) & (iw < w)


def maxpool_fwd(x, k, stride, pad):
    """(y [n,oh,ow,c] in x's dtype, argmax uint8) by the kernels' rule, one window tap after the other."""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x)
    n, h, w, c = x.shape
    oh, ow = pool_out(h, k, stride, pad), pool_out(w, k, stride, pad)
    y = np.full((n, oh, ow, c), -np.inf, dtype=x.dtype)
    am = np.full((n, oh, ow, c), 255, dtype=np.uint8)
    for tap, ih, vh, iw, vw in _taps(h, w, k, stride, pad):
        v = np.zeros((n, oh, ow, c), dtype=x.dtype)
        v[np.ix_(range(n), np.nonzero(vh)[0], np.nonzero(vw)[0])] = x[np.ix_(range(n), ih[vh], iw[vw])]
        inside = (vh[:, None] & vw[None, :])[None, :, :, None]
        better = v > y
        y = np.where(better, v, y)
        am = np.where(better, np.where(inside, np.uint8(tap), np.uint8(255)), am).astype(np.uint8)
    return torch.from_numpy(y), torch.from_numpy(am)


def maxpool_route(dy, argmax, xshape, k, stride, pad):
    """(dx, sum |dy terms|, w) float64 / int per input pixel: the pooled gradients of the windows whose arg-max names the pixel."""
    dy, am = _t(dy).numpy(), _t(argmax, torch.uint8).numpy()
    n, h, w, c = xshape
    dx, mag, cnt = np.zeros(xshape), np.zeros(xshape), np.zeros(xshape, dtype=np.int64)
    for tap, ih, vh, iw, vw in _taps(h, w, k, stride, pad):
        src = np.ix_(range(n), np.nonzero(vh)[0], np.nonzero(vw)[0])
        dst = np.ix_(range(n), ih[vh], iw[vw])                # one window per pixel and tap: no index repeats
        hit = am[src] == tap
        dx[dst] += np.where(hit, dy[src], 0.0)
        mag[dst] += np.where(hit, np.abs(dy[src]), 0.0)
        cnt[dst] += hit
    return torch.from_numpy(dx), torch.from_numpy(mag), torch.from_numpy(cnt)


def maxpool_gather(x, argmax, k, stride, pad):
    """x at each window's winning tap (0 where a padding zero won): what the fused forward leaves in xwin."""
    x, am = _t(x, F32).numpy(), _t(argmax, torch.uint8).numpy()
    n, h, w, c = x.shape
    out = np.zeros(am.shape, dtype=np.float32)
    for tap, ih, vh, iw, vw in _taps(h, w, k, stride, pad):
        src = np.ix_(range(n), np.nonzero(vh)[0], np.nonzero(vw)[0])
        out[src] = np.where(am[src] == tap, x[np.ix_(range(n), ih[vh], iw[vw])], out[src])
    return torch.from_numpy(out)


def check_maxpool(x, dy, k, stride, pad, y, argmax, dx, what="maxpool"):
    """y bit-identical, argmax equal, dx inside gamma(w - 1) sum|dy terms| (exact for w <= 1)."""
    yr, ar = maxpool_fwd(_t(x, F32), k, stride, pad)
    assert torch.equal(_t(y, F32), yr), what + ": y is not bit-identical"
    assert torch.equal(_t(argmax, torch.uint8), ar), what + ": argmax differs"
    ref, mag, cnt = maxpool_route(dy, ar, tuple(x.shape), k, stride, pad)
    dx = _t(dx)
    assert bool((dx[cnt == 0] == 0).all()), what + ": a pixel no window routes to is not exactly 0"
    adds = (cnt - 1).clamp_min(0).double()
    return {"pool dx": within((dx - ref).abs(), adds * U / (1 - adds * U) * mag, what + " dx")}, int(cnt.max())


def check_relu_colsum(y_in, dx_ref_own, dz, dbias, what="maxpool_relu_bwd_colsum"):
    """embnet_maxpool_relu_bwd_colsum: dz = (the pool's dx) [y_in > 0] bit for bit, dbias against the column sum of dz."""
    dz = _t(dz)
    want = torch.where(_t(y_in) > 0, _t(dx_ref_own), torch.zeros_like(dz))
    assert torch.equal(dz, want), what + ": dz is not the masked pool gradient"
    flat = dz.reshape(-1, dz.shape[-1])
    return {"pool dbias": within((_t(dbias) - flat.sum(0)).abs(), gamma(flat.shape[0]) * flat.abs().sum(0), what + " dbias")}


# ---- fused BN -> act -> pad -> pool -------------------------------------------------------------------------------------------------
def fused_forward(x, scale, shift, act, k, stride, pad, dtype=F64):
    """(y, argmax, xwin): the pool of act(x scale + shift), as the composition of the above."""
    a = act_fwd(affine(x, scale, shift, dtype), act, exp_form=dtype == F32)
    y, am = maxpool_fwd(a, k, stride, pad)
    return y, am, maxpool_gather(x, am, k, stride, pad)


def fused_backward(x, dy, argmax, state, act, training, k, stride, pad, dtype=F64):
    """dict of dbeta, dgamma (sums over the pooled elements), dx (inv_m = 1 / (n h w)): pool backward, then bn_backward."""
    n, h, w, c = x.shape
    xw = maxpool_gather(x, argmax, k, stride, pad).reshape(-1, c)
    on = (_t(argmax, torch.uint8) != 255).reshape(-1, c)
    dyp = torch.where(on, _t(dy, dtype).reshape(-1, c), torch.zeros(1, dtype=dtype))
    sums = bn_backward(xw, dyp, state, act, 1, dtype=dtype)
    routed = maxpool_route(_t(dy, dtype), argmax, (n, h, w, c), k, stride, pad)[0].to(dtype).reshape(-1, c)
    xs = _t(x, dtype).reshape(-1, c)
    mean, rstd, sc, sh = (_t(state[key], dtype) for key in ("save_mean", "save_rstd", "scale", "shift"))
    dz = routed * act_der(affine(xs, sc, sh, dtype), act, exp_form=dtype == F32)
    inv_m = torch.tensor(1.0 / (n * h * w), dtype=dtype)
    dx = sc * (dz - sums["dbeta"] * inv_m - (xs - mean) * rstd * sums["dgamma"] * inv_m) if training else sc * dz
    return dict(dbeta=sums["dbeta"], dgamma=sums["dgamma"], dx=dx.reshape(n, h, w, c))


def check_fused_backward(x, dy, argmax, state, act, training, k, stride, pad, out, what="fused bwd"):
    n, h, w, c = x.shape
    xw = maxpool_gather(x, argmax, k, stride, pad).reshape(-1, c)
    on = (_t(argmax, torch.uint8) != 255).reshape(-1, c)
    dyp = torch.where(on, _t(dy, F32).reshape(-1, c), torch.zeros(1))
    r = check_bn_sums(xw, dyp, state, act, out["dbeta"], out["dgamma"], what)
    routed, mag, cnt = maxpool_route(dy, argmax, (n, h, w, c), k, stride, pad)
    key = "fused dx%s act%d" % ("" if training else " frozen", act)
    r[key] = check_dx(_t(x).reshape(-1, c), routed.reshape(-1, c), mag.reshape(-1, c), state, act, training, out["dbeta"], out["dgamma"],
                      _t(out["dx"]).reshape(-1, c), what + " dx", m=n * h * w, nround=7 + max(int(cnt.max()) - 1, 0))
    return r


# ---- global average pooling ------------------------------------------------------------------------------------------------------------
def gap_forward(x, dtype=F64):
    return _t(x, dtype).mean(1)                            # x [n, hw, c]


def gap_backward(dy, hw, dx_add=None, dtype=F64):
    dx = (_t(dy, dtype) / hw).unsqueeze(1).expand(-1, hw, -1)
    return dx + _t(dx_add, dtype) if dx_add is not None else dx.contiguous()


def check_gap_forward(x, y, what="gap fwd"):
    x = _t(x)
    hw = x.shape[1]
    return {"gap fwd": within((_t(y) - x.mean(1)).abs(), gamma(hw + 1) * x.abs().mean(1), what)}


def check_gap_backward(dy, hw, dx, dx_add=None, what="gap bwd"):
    t = (_t(dy) / hw).unsqueeze(1)
    if dx_add is None:
        return {"gap bwd": within((_t(dx) - t).abs(), gamma(2) * t.abs(), what)}
    a = _t(dx_add)
    return {"gap bwd +add": within((_t(dx) - (t + a)).abs(), gamma(3) * t.abs() + U * a.abs(), what)}


def check_affine_act_gap(x, scale, shift, act, y, gap, what="affine_act_gap"):
    """y per element as a BatchNorm's; gap against the float64 mean of the kernel's own y (y given), or of act(z) with the
    elements' own bounds added (y = NULL)."""
    n, hw, c = x.shape
    r = {}
    if y is not None:
        r["gap y act%d" % act] = check_y(x.reshape(-1, c), scale, shift, act, _t(y, F32).reshape(-1, c), what + " y")
        own = _t(y)
        r["gap mean act%d" % act] = within((_t(gap) - own.mean(1)).abs(), gamma(hw + 1) * own.abs().mean(1), what + " gap")
    else:
        z = _t(x) * _t(scale) + _t(shift)
        a = act_fwd(z, act)
        eb = ((U + 4 * kappa_fwd(x.reshape(-1, c), scale, shift, act)) * z.abs()).mean(1)
        r["gap mean (y NULL) act%d" % act] = within((_t(gap) - a.mean(1)).abs(), gamma(hw + 1) * (a.abs().mean(1) + eb) + eb, what + " gap")
    return r


def old_close(got, want, tol=1e-5):
    """The neighbouring tests' metric: the largest error over the largest value of the whole tensor."""
    got, want = _t(got), _t(want)
    return float((got - want).abs().max()) <= tol * max(float(want.abs().max()), 1e-30)


# ---- the cases both test files run ---------------------------------------------------------------------------------------------------
# (m, c): each the smallest shape that reaches its branch of the reductions (reduce_geom; test_nn_ref_cpu.py holds the table)
BN_SHAPES = [(1, 4), (37, 4), (2500, 4), (297, 48), (297, 256), (37, 1028), (98, 3), (297, 6), (37, 258)]
POOL_GEOMS = [(2, 2, 0, 12, 12), (2, 2, 0, 13, 11), (3, 2, 1, 15, 17), (3, 2, 1, 16, 16), (3, 1, 1, 7, 9), (3, 3, 0, 9, 9), (3, 2, 1, 1, 1)]   # k, stride, pad, h, w
POOL_CHANNELS = (8, 20, 6)
POOL_INPUTS = ("postrelu", "quantised", "negative")
POOL_N = 2
FUSED_GEOMS = [(3, 2, 1, 15, 17), (2, 2, 0, 12, 10), (3, 1, 1, 7, 9)]
FUSED_CHANNELS = (8, 64)
# (n, hw, c); (1, 1025, 8) runs affine_act_gap4_kernel on 1024 threads = 512 pixel lanes, where the four-pixel loop needs hw > 1536:
# it reaches the tail loop alone, so (1, 2051, 8) is added for the loop plus its tail there ((2, 196, 68) has both on 256 threads)
GAP_CASES = [(2, 1, 4), (3, 49, 48), (2, 196, 68), (2, 49, 6), (1, 1025, 8), (1, 2051, 8)]


def pool_input(kind, n, h, w, c, seed=0):
    """(x, dy-generator) float32: postrelu = relu(randn), many zero ties; quantised = multiples of 1/4, ties among positive maxima;
    negative = -(|randn| + 0.01): padding zeros win where pad > 0, the true negative maximum where pad = 0."""
    g = torch.Generator().manual_seed(seed * 7919 + 31 * POOL_INPUTS.index(kind) + 1000 * h + 10 * w + c)
    x = torch.randn(n, h, w, c, generator=g)
    if kind == "postrelu":
        x = torch.relu(x)
    elif kind == "quantised":
        x = torch.round(x * 4) / 4
    else:
        x = -(x.abs() + 0.01)
    return x.contiguous(), g
