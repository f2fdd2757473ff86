"""float64 references and textbook rounding bounds of everything BETWEEN an MBConv block's depthwise BatchNormalization and its
residual add: the squeeze-and-excite multiply (csrc/mbconv_kernels.hip chscale_*), the stand-alone activations, |a - b| and the
per-sample drop-connect of the same file, the fused passes of csrc/nn_kernels.hip (affine_act_scale4, affine_drop_add4, se_bn_sums4,
se_bn_finalize, bn_bwd_reduce4_gap / bn_bwd_apply4_gap) and the squeeze-and-excite MLP of csrc/se_mlp.hip.  Plain torch / NumPy on
the CPU, no kernel code.  tests/test_se_ref_cpu.py holds the float32 CPU evaluation of every formula against every check below,
tests/test_se_kernels_elementwise_gpu.py the kernels; both call the SAME check_* functions: a check takes the operands and the
outputs, raises AssertionError at the first element outside its bound and returns {quantity: largest error / bound}.  gamma, U,
within, act_fwd, act_der, kappa_fwd, kappa_der, check_dx, check_y, bn_case, BORDER_CAP, GAP_CASES and col_geom are nn_ref's.

Every quantity here is scaled per (image, channel): the gate s[n,c] is a sigmoid, the sums are [n][5][c], drop-connect zeroes whole
images.  So every bound is per element or per (image, channel), u = 2^-24, gamma(k) = k u / (1 - k u) for k roundings on the path of
a term (any order of the additions; an addition of an exact zero does not round, so a sum of hw terms has at most hw - 1 rounding
additions on any path however the lanes, butterflies and waves are laid out).  The counts, read off the source:

  embnet_channel_scale_fwd   y = x s, one product:                    |y - x s| <= u |x s|
  embnet_channel_scale_bwd   dx = dy s: one product.  ds[n,c] = sum_p dy x: chscale_bwd_kernel is a chain of hw fmas;
      chscale_bwd4_kernel has ceil(hw / 16) fmas per pixel lane and then the <= min(hw, 16) - 1 rounding additions of the 16 lanes,
      never more than hw on a path:                                   |ds - sum_p dy x| <= gamma(hw) sum_p |dy x|
  embnet_channel_scale_dgate bit-identical to chscale_bwd4_kernel's ds (the same lanes, the same order).
  embnet_activation_fwd / _bwd (kind 0 sigmoid, 1 swish), 1 / (1 + __expf(-v)):  the E32 form of nn_ref's swish — 4 x (the largest
      relative figure of the float32 CPU evaluation over the tensor) x the element's own scale:
          swish      4 kappa |v|                 kappa  = max |swish32 - swish64| / |v|                      (nn_ref.kappa_fwd)
          sigmoid    4 kappa_s s (1 + |v|)       kappa_s = max |sigmoid32 - sigmoid64| / (s (1 + |v|))  — exp's ARGUMENT is rounded
                     (v log2 e on the device): a relative error of |v| u in exp(-v), so the scale grows with |v|
          dx         4 kappa' |dy| + u |dy act'| kappa' = max |act'32 - act'64| (act' is O(1); the product with dy rounds once).
      4 = the project's margin for the device's exp (nn_ref).  dy = 0 gives a bound of 0: dx must be exactly 0.
  embnet_absdiff_fwd / _bwd  exact: y is the bits of fl(|a - b|) (never -0), da = +dy / -dy / 0 by the sign of fl(a - b), db = -da;
      a == b (as values: +0 and -0 too) gives 0 in both (db's zero carries a sign bit: compared as a value).
  embnet_sample_dropout and embnet_affine_drop_add's factor: image i is kept iff augment_ref.rng_u32(seed, i, 2) >=
      uint32(double(rate) 2^32); survivors are the bits of fl(x fl(1 / (1 - rate))); rate = 0 is the identity.
  embnet_affine_act_scale    z = x scale + shift by ONE fma, act, one product with the gate:
          |y - act(z) s| <= (1 + u) B_y |s| + u |act(z) s|,  B_y = check_y's (u + 4 kappa) |z|;  |x scale| + |shift| = 0 or s = 0: exactly 0
  embnet_affine_drop_add     fma, product with the factor f, sum with skip: three roundings on z f's path, one on skip's:
          |y - (z f + skip)| <= gamma(3) |z f| + u |skip|;  a dropped image (f = 0): y is skip exactly
  embnet_se_bn_sums          per (image, channel) against float64 of the given scale / shift / mean / rstd:
          |T - sum_p term| <= gamma(hw + k) sum_p |term| + 4 E32 + B,   k = the roundings of one() in front of the accumulating
          add / fma:      T0 = dg a      S1 = a' dg   S2 = a'   S3 = a' dg xhat   S4 = a' xhat
            act 0, 1      1 (z)          0            0         2 (xhat)          2
            act 2         2 (z, z sg)    1 (a' dg)    0         3                 2          (the sigmoid itself is in E32)
          E32 (swish; 0 otherwise) in nn_ref's KAPPA form: sum_p kappa |z| |dg| for T0, sum_p kappa' |the factors of a'| for
          S1..S4, kappa / kappa' the tensor's largest float32-CPU figures (nn_ref.kappa_fwd / kappa_der).  (The plain sum over
          the pixels of |term in float32 - term in float64| is never larger, and at hw = 1 .. a few pixels it is 0 or tiny BY
          LUCK on some (image, channel) — (2, 1, 64): the float32 stand-in itself missed it by 1.5x — so it cannot bound
          another fp32 implementation there; the tensor's largest relative figure can, nn_ref's argument for y.)
          B = the ReLU-borderline mass: what the elements |z| <= 4 u (|x scale| + |shift|) can move if fp32 takes the other
          side.  S2 of act 0 / 1 is a count and exact.
          T0 against embnet_channel_scale_dgate on embnet_affine_act's OWN output a_k: within the sum of both bounds,
          T0's + gamma(hw) sum |dg a_k| + sum |dg| |a_k - a| (not bitwise: z / (1 + e) there, z rcp(1 + e) here).
  embnet_bn_bwd_gap_sums     dz = a' (dg s + dpool / hw).  dbeta / dgamma per channel, M = n hw:
          (a) against the kernel's OWN sums: sum_n (s S1 + q S2), q = dpool / hw, is formed in double: the rounding of 1.f / hw,
              the product with it and the cast: gamma(3) sum_n (|s S1| + |q S2|)           (S3, S4 for dgamma)
          (b) against float64 of dz, the nn_ref.check_bn_sums form on the two products: gamma(M + 3) sum (|a' dg s| + |a' q|)
              + 4 E32 + B for dbeta (S1's hw, then (a)'s 3), gamma(M + 6) with |xhat| for dgamma (k = 3 more); E32 = kappa' x
              the same magnitude sums
          dx per element by nn_ref.check_dx on dz_in = dy s + dpool / hw in float64 with dz_mag = |dy s| + |dpool / hw| and the
          kernel's own dbeta / dgamma: the gate's product, 1.f / hw and its product (or the contracted fma) stay inside the seven
          roundings of check_dx's longest path (dpool's: 1 / hw, product, sum, act', the two subtractions, scale = 7).
  embnet_bn_bwd_gap          the same (b) and dx checks for gate NULL, gate given and the drop-connect form (gate = factor,
          dpool = 0); its sums agree with embnet_bn_bwd_gap_sums' within the sum of the two (b) bounds, its dx within the two dx
          bounds plus |scale| (|dbeta_1 - dbeta_2| + |xhat| |dgamma_1 - dgamma_2|) / M.
  embnet_se_mlp_fwd          z1 = pooled W1 + b1: ceil(C / 16) fmas per channel lane, then b1 and the <= min(C, 16) lane sums:
          |z1 - ref| <= gamma(C + 1) (sum |p| |w1| + |b1|)
          gate against float64 from the kernel's OWN z1, h = swish(z1), a = h W2 + b2 (ceil(S / G) fmas per unit group, G + 1 adds):
          |gate - s| <= e^Ea s (1 - s) Ea + 4 kappa_s s (1 + |a|),  Ea = gamma(S + 1) (sum |h| |w2| + |b2|) + sum |w2| 4 kappa |z1|
  embnet_se_mlp_bwd          each quantity from the kernel's own upstream outputs (gate, z1, dz1):
          dz2 = dgate g (1 - g): three roundings.  dh = dz2 W2^T: four-term fma groups, row slices, 16 slice sums, at most C.
          dz1 = dh swish'(z1):  gamma(C + 4) |swish'| sum |dz2| |w2| + 4 kappa' sum |dz2| |w2|     (+ 1: the last product)
          dpooled = dz1 W1^T: gamma(S) sum |dz1| |w1|;  dW1, db1: gamma(n) sum_n |pooled| |dz1|, gamma(n) sum_n |dz1|
          dW2, db2: gamma(n + 3) sum_n |h| |dz2| + 4 E32 (E32 = sum_n kappa |z1| |dz2|, the kappa form), gamma(n + 3) sum_n |dz2|
  zero rule: every bound is a multiple of a magnitude sum; where that is 0 the value must be exactly 0 (within()).

ReLU-borderline cap — a CONDITION on the inputs, asserted by both test files: at most BORDER_CAP = 0.1 % of any channel and, per
(image, channel) group of fewer than 1000 pixels, none (0.1 % of a larger group).  se_case walks the seeds from the one it is given
until the inputs meet it (the seed it settled on is in the case).
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as AR  # noqa: E402
import nn_ref as N  # noqa: E402
import stream_ref as ST  # noqa: E402
from nn_ref import BORDER_CAP, GAP_CASES, U, act_der, act_fwd, bn_case, check_dx, check_y, col_geom, gamma, kappa_der, kappa_fwd, within  # noqa: E402,F401

F64, F32 = torch.float64, torch.float32
_t = N._t
STATE = ("save_mean", "save_rstd", "scale", "shift")
ONE, ZERO = torch.ones(()), torch.zeros(())


# ---- geometry mirrors -----------------------------------------------------------------------------------------------------------------
PixGeom = namedtuple("PixGeom", "cls xblocks threads lanes")
EW_CAP = 4096


def pix_geom(n, hw, c4):
    """nn_kernels.hip pix_geom (se_bn_sums4_kernel, affine_act_gap4_kernel): channel-quad lanes, channel blocks, threads, pixel lanes."""
    lg = 4
    while lg > 0 and (1 << (lg - 1)) >= c4:
        lg -= 1
    cls = 1 << lg
    xblocks = (c4 + cls - 1) >> lg
    threads = 1024 if (xblocks * n < 2048 and hw >= 256) else 256
    return PixGeom(cls, xblocks, threads, threads // cls)


def pix_paths(n, hw, c4):
    """What se_bn_sums4_kernel's pixel loop reaches: (the two-pixel loop runs, a lane has a tail pixel behind it or alone)."""
    g = pix_geom(n, hw, c4)
    loop = tail = False
    for pl in range(min(g.lanes, hw + 1)):
        p = pl
        while p + g.lanes < hw:
            loop, p = True, p + 2 * g.lanes
        tail = tail or p < hw
    return loop, tail


def ew_blocks(total):
    return max(min((total + 255) // 256, EW_CAP), 1)


def ew_blocks_c4(total4, c4):
    b = ew_blocks(total4)
    unit = c4 // int(np.gcd(c4, 256))
    if unit > 1:
        b = unit if b < unit else b // unit * unit
    return b


def quad_groups(c4, S):
    g = max(min(1024 // c4, S), 1)
    return g, -(-S // g)


def jp_of(S):
    return (S + 63) // 64 * 64


WL_FLOATS = 16384


def se_mlp_supported(n, c, s):
    if n <= 0 or c <= 0 or s <= 0 or s > 160 or c % 4 or c // 4 > 1024:
        return False
    lds_a = (2 * c + 2 * jp_of(s) + 16 * 64 + 1024 * 17) * 4
    lds_b = (2 * 16 + 2 * s) * 68 * 4
    return lds_a <= 150 * 1024 and lds_b <= 150 * 1024


def mlp_paths(n, c, S):
    """dict of the branches of se_mlp.hip a shape reaches."""
    return dict(umax=3 if S <= 48 else 10, jp=jp_of(S), tiles=-(-n // 64), odd_n=n % 2 == 1, ragged_c=c % 16 != 0,
                G=quad_groups(c // 4, S)[0], w1_chunks=-(-c // (WL_FLOATS // (S | 1))), workgroups_b=-(-c // 16))


# ---- families -------------------------------------------------------------------------------------------------------------------------
FAMILIES = ["even", "spread17", "quiet_image17", "zero", "relu"]
GATE_FAMILIES = ["unit", "spread17", "dropped"]
GATE_OF = {"even": "spread17", "spread17": "spread17", "quiet_image17": "unit", "zero": "dropped", "relu": "spread17"}
DROP_RATE = 0.2
QUIET = 2.0 ** -17
SeCase = namedtuple("SeCase", "x dy skip dpool gate state seed")


def keep_scale(rate):
    """fl(1 / (1 - rate)) as the kernels form it."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def drop_keep(n, rate, seed):
    """bool [n]: image i survives iff rng_u32(seed, i, 2) >= uint32(double(rate) 2^32)."""
    thr = np.uint32(int(float(np.float32(rate)) * 4294967296.0))
    return AR.rng_u32(int(seed) % (1 << 64), np.arange(n, dtype=np.uint64), 2) >= thr


def drop_factor(n, c, rate, seed):
    """embnet_affine_drop_add's factor [n, c] float32."""
    keep = drop_keep(n, rate, seed) if rate > 0 else np.ones(n, dtype=bool)
    return torch.from_numpy(np.where(keep, keep_scale(rate), np.float32(0.0)).astype(np.float32))[:, None].expand(n, c).contiguous()


def se_gate(kind, n, c, g, rate=DROP_RATE):
    """unit: ones; spread17: log-uniform over [2^-17, 1], independent per image and channel; dropped: rows 0, 2, .. zero, the rest
    fl(1 / (1 - rate))."""
    if kind == "unit":
        return torch.ones(n, c)
    if kind == "spread17":
        return torch.exp2(-17.0 * torch.rand(n, c, generator=g)).contiguous()
    s = torch.full((n, c), float(keep_scale(rate)))
    s[0::2] = 0.0
    return s


def border(x, scale, shift):
    x, sc, sh = _t(x), _t(scale), _t(shift)
    return (x * sc + sh).abs() <= 4 * U * ((x * sc).abs() + sh.abs())


def border_ok(x, scale, shift):
    """The ReLU-borderline cap on [n, hw, c] inputs (module docstring)."""
    b = border(x, scale, shift)
    n, hw, c = b.shape
    allowed = int(BORDER_CAP * hw) if hw >= 1000 else 0
    return float(b.reshape(-1, c).double().mean(0).max()) <= BORDER_CAP and int(b.sum(1).max()) <= allowed


def _make(family, n, hw, c, seed):
    base = "even" if family == "quiet_image17" else family
    bc = bn_case(base, n * hw, c, seed=seed + 11)
    x, dy = bc.x.reshape(n, hw, c).clone(), bc.dy.reshape(n, hw, c).clone()
    g = torch.Generator().manual_seed(seed * 7919 + 977 * FAMILIES.index(family) + 31 * n + 7 * hw + c)
    skip = torch.randn(n, hw, c, generator=g)
    dpool = ST._gradient(base, g, (n, c)) * float(hw)      # dpool / hw is of dy's size
    if family == "spread17":
        skip = skip * ST._channel_amplitude(g, c, 17)
    elif family == "zero":
        skip[:, :, 1::4] = 0.0
    elif family == "quiet_image17":
        for t in (x, dy, skip, dpool):
            t[-1] *= QUIET
    gate = se_gate(GATE_OF[family], n, c, g)
    st = N.bn_forward(bc._replace(x=x.reshape(-1, c)), N.f32(1e-3), 0, dtype=F32)
    return SeCase(x.contiguous(), dy.contiguous(), skip.contiguous(), dpool.contiguous(), gate, {k: st[k].contiguous() for k in STATE}, seed)


@functools.lru_cache(maxsize=512)
def se_case(family, n, hw, c, seed=0):
    """Float32 tensors of one family over [n, hw, c] (nn_ref.bn_case's x / dy / gamma / beta of the family; quiet_image17: the last
    image, its gradients and its skip at 2^-17 of the others), a skip tensor, a pooled gradient, the gate of GATE_OF[family] and the
    BatchNormalization state (batch statistics of x, eps 1e-3) as fp32 save_mean / save_rstd / scale / shift.  The first seed from
    `seed` on whose inputs meet the ReLU-borderline cap."""
    for s in range(seed, seed + 64):
        case = _make(family, n, hw, c, s)
        if border_ok(case.x, case.state["scale"], case.state["shift"]):
            return case
    raise AssertionError("no seed meets the ReLU-borderline cap")


def logits30(total, seed=0):
    """Activation inputs over [-30, 30], where the sigmoid's relative error has not been measured before."""
    g = torch.Generator().manual_seed(991 + seed + total)
    return ((torch.rand(total, generator=g) * 2 - 1) * 30.0).contiguous()


# ---- squeeze-and-excite multiply ----------------------------------------------------------------------------------------------------
def _bc(s):
    return _t(s).unsqueeze(1)                              # [n, c] -> [n, 1, c]


def check_channel_scale_fwd(x, s, y, what="channel_scale_fwd"):
    ref = _t(x) * _bc(s)
    return {"chscale y": within((_t(y) - ref).abs(), U * ref.abs(), what)}


def check_channel_scale_bwd(x, s, dy, dx, ds, what="channel_scale_bwd"):
    x, dy = _t(x), _t(dy)
    hw = x.shape[1]
    ref, t = dy * _bc(s), dy * x
    return {"chscale dx": within((_t(dx) - ref).abs(), U * ref.abs(), what + " dx"),
            "chscale ds": within((_t(ds) - t.sum(1)).abs(), gamma(hw) * t.abs().sum(1), what + " ds")}


def lane_fma_sum(a, b, lanes=16):
    """sum_p a b over axis 1 in fp32 in chscale_bwd4_kernel's order: pixel lane l takes pixels l, l + lanes, .. by fma, the lanes
    are then added in lane order.  (The fma: product and sum in double, rounded once.)"""
    a, b = _t(a, F32), _t(b, F32)
    n, hw, c = a.shape
    acc = torch.zeros(n, lanes, c)
    for p0 in range(0, hw, lanes):
        k = min(lanes, hw - p0)
        acc[:, :k] = (acc[:, :k].double() + a[:, p0:p0 + k].double() * b[:, p0:p0 + k].double()).float()
    out = acc[:, 0].clone()
    for lane in range(1, lanes):
        out = out + acc[:, lane]
    return out


# ---- activations, |a - b|, drop-connect ---------------------------------------------------------------------------------------------
def sigmoid_kappa(v):
    """Largest |float32 CPU sigmoid - float64| / (s (1 + |v|)) over the tensor."""
    v64 = _t(v)
    s = torch.sigmoid(v64)
    err = (torch.sigmoid(_t(v, F32)).double() - s).abs()
    return float((err / (s * (1 + v64.abs()))).max())


def act_kind(v, kind, dtype=F64, exp_form=False):
    v = _t(v, dtype)
    sg = 1 / (1 + torch.exp(-v)) if exp_form else torch.sigmoid(v)
    return v * sg if kind else sg


def act_kind_der(v, kind, dtype=F64, exp_form=False):
    v = _t(v, dtype)
    sg = 1 / (1 + torch.exp(-v)) if exp_form else torch.sigmoid(v)
    return sg + v * sg * (1 - sg) if kind else sg * (1 - sg)


def check_activation_fwd(x, kind, y, what="activation_fwd"):
    v = _t(x).reshape(-1)
    if kind:
        bound = 4 * kappa_fwd(v.reshape(-1, 1), ONE, ZERO, 2) * v.abs()
    else:
        bound = 4 * sigmoid_kappa(v) * torch.sigmoid(v) * (1 + v.abs())
    return {"act fwd %s" % ("swish" if kind else "sigmoid"): within((_t(y).reshape(-1) - act_kind(v, kind)).abs(), bound, what)}


def check_activation_bwd(x, dy, kind, dx, what="activation_bwd"):
    v, dy = _t(x).reshape(-1), _t(dy).reshape(-1)
    der = act_kind_der(v, kind)
    kd = float((act_kind_der(v, kind, F32).double() - der).abs().max())
    ref = dy * der
    return {"act bwd %s" % ("swish" if kind else "sigmoid"): within((_t(dx).reshape(-1) - ref).abs(), 4 * kd * dy.abs() + U * ref.abs(), what)}


def _bits(t):
    return _t(t, F32).contiguous().view(torch.int32)


def bit_identical(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape and bool((a == b).all()), "%s: %d of %d elements differ in their bits" % (what, int((a != b).sum()), a.numel())


def absdiff(a, b, dy):
    """(y, da, db) float32 as the kernels define them."""
    d = _t(a, F32) - _t(b, F32)
    dy = _t(dy, F32)
    da = torch.where(d > 0, dy, torch.where(d < 0, -dy, torch.zeros_like(dy)))
    return d.abs(), da, -da


def check_absdiff(a, b, dy, y, da, db, what="absdiff"):
    yr, dar, dbr = absdiff(a, b, dy)
    bit_identical(y, yr, what + " y")
    assert not bool((_bits(y) < 0).any()), what + ": y carries a sign bit"
    tie = (_t(a, F32) - _t(b, F32)) == 0
    da, db = _t(da, F32), _t(db, F32)
    assert bool((da[tie] == 0).all()) and bool((db[tie] == 0).all()), what + ": a == b must give gradient 0"
    bit_identical(da[~tie], dar[~tie], what + " da")
    bit_identical(db[~tie], dbr[~tie], what + " db")
    return {"absdiff (exact)": 0.0}


def sample_dropout(x, per_sample, rate, seed):
    """embnet_sample_dropout in float32, bit for bit."""
    x = _t(x, F32).reshape(-1)
    total = x.numel()
    img = np.arange(total, dtype=np.int64) // per_sample
    keep = torch.from_numpy(drop_keep(int(img[-1]) + 1, rate, seed)[img])
    return torch.where(keep, x * torch.tensor(float(keep_scale(rate))), torch.zeros(()))


# ---- the fused BatchNorm-apply passes ------------------------------------------------------------------------------------------------
def _z(x, state):
    return _t(x) * _t(state["scale"]) + _t(state["shift"])


def affine_act_scale(x, state, act, gate, dtype=F64):
    a = act_fwd(N.affine(x, state["scale"], state["shift"], dtype), act, exp_form=dtype == F32)
    return a * _t(gate, dtype).unsqueeze(1)


def check_affine_act_scale(x, state, act, gate, y, what="affine_act_scale"):
    x64, y, s = _t(x), _t(y), _bc(gate)
    n, hw, c = x64.shape
    z = _z(x, state)
    ref = act_fwd(z, act) * s
    by = (U + 4 * kappa_fwd(x64.reshape(-1, c), state["scale"], state["shift"], act)) * z.abs() * s.abs()
    exact = (((x64 * _t(state["scale"])).abs() + _t(state["shift"]).abs()) == 0) | (s == 0)
    assert bool((y[exact.expand_as(y)] == 0).all()), what + ": an element with |x scale| + |shift| = 0 or a zero gate is not exactly 0"
    return {"act_scale y act%d" % act: within((y - ref).abs(), (1 + U) * by + U * ref.abs(), what)}


def affine_drop_add(x, state, factor, skip, dtype=F64):
    return N.affine(x, state["scale"], state["shift"], dtype) * _t(factor, dtype).unsqueeze(1) + _t(skip, dtype)


def check_affine_drop_add(x, state, factor, skip, y, what="affine_drop_add"):
    f, k = _bc(factor), _t(skip)
    zf = _z(x, state) * f
    bound = gamma(3) * zf.abs() + U * k.abs() * (f != 0)
    return {"drop_add y": within((_t(y) - (zf + k)).abs(), bound, what)}


# ---- the [n][5][c] sums -----------------------------------------------------------------------------------------------------------------
SUMS = ("T0", "S1", "S2", "S3", "S4")
SUMS_K = {0: (1, 0, 0, 2, 2), 1: (1, 0, 0, 2, 2), 2: (2, 1, 0, 3, 2)}


def se_sums_terms(dg, x, state, act, dtype=F64, exp_form=False):
    """The five per-element terms of se_bn_sums4_kernel's one()."""
    dg, x = _t(dg, dtype), _t(x, dtype)
    mu, rs = _t(state["save_mean"], dtype), _t(state["save_rstd"], dtype)
    z = N.affine(x, state["scale"], state["shift"], dtype)
    a, ad = act_fwd(z, act, exp_form), act_der(z, act, exp_form)
    xh = (x - mu) * rs
    adg = ad * dg
    return [dg * a, adg, ad + torch.zeros_like(x), adg * xh, ad * xh]


def se_sums(dg, x, state, act, dtype=F64):
    """[n, 5, c]; float32: the stand-in (the exp form of the sigmoid, torch's own summation order)."""
    return torch.stack([t.sum(1) for t in se_sums_terms(dg, x, state, act, dtype, exp_form=dtype == F32)], 1)


def _e32_sums(dg, x, state):
    """E32 of the five swish terms, per (image, channel), in the kappa form of the module docstring."""
    c = x.shape[-1]
    kf, kd = kappa_fwd(x.reshape(-1, c), state["scale"], state["shift"], 2), kappa_der(x.reshape(-1, c), state["scale"], state["shift"], 2)
    dg64, xh, z = _t(dg).abs(), ((_t(x) - _t(state["save_mean"])) * _t(state["save_rstd"])).abs(), _z(x, state).abs()
    return [kf * (dg64 * z).sum(1), kd * dg64.sum(1), kd * torch.ones_like(z).sum(1), kd * (dg64 * xh).sum(1), kd * xh.sum(1)]


def se_sums_bounds(dg, x, state, act):
    """(reference [n,5,c], bound [n,5,c]) of the module docstring."""
    hw = x.shape[1]
    t64 = se_sums_terms(dg, x, state, act)
    zero = torch.zeros_like(t64[0][:, 0])
    e32 = [zero] * 5
    if act == 2:
        e32 = _e32_sums(dg, x, state)
    bm = [zero] * 5
    if act == 1:
        bd = border(x, state["scale"], state["shift"]).double()
        dg64, xh, z = _t(dg), (_t(x) - _t(state["save_mean"])) * _t(state["save_rstd"]), _z(x, state)
        bm = [(v.abs() * bd).sum(1) for v in (dg64 * z, dg64, torch.ones_like(z), dg64 * xh, xh)]
    ref = torch.stack([t.sum(1) for t in t64], 1)
    bound = torch.stack([gamma(hw + SUMS_K[act][q]) * t64[q].abs().sum(1) + 4 * e32[q] + bm[q] for q in range(5)], 1)
    return ref, bound


def check_se_sums(dg, x, state, act, sums, what="se_bn_sums"):
    ref, bound = se_sums_bounds(dg, x, state, act)
    got = _t(sums)
    return {"sums %s act%d" % (SUMS[q], act): within((got[:, q] - ref[:, q]).abs(), bound[:, q], "%s %s" % (what, SUMS[q])) for q in range(5)}


def check_t0_vs_dgate(dg, x, state, act, sums, a_k, dgate, what="se_bn_sums T0 vs channel_scale_dgate"):
    """Row 0 against embnet_channel_scale_dgate on embnet_affine_act's own output a_k: the sum of both bounds."""
    hw = x.shape[1]
    _, bound = se_sums_bounds(dg, x, state, act)
    dg64, ak = _t(dg), _t(a_k)
    a = act_fwd(_z(x, state), act)
    other = gamma(hw) * (dg64 * ak).abs().sum(1) + (dg64.abs() * (ak - a).abs()).sum(1)
    return {"T0 - dgate act%d" % act: within((_t(sums)[:, 0] - _t(dgate)).abs(), bound[:, 0] + other, what)}


# ---- BatchNorm backward on dy gate + dpool / hw -----------------------------------------------------------------------------------------
def _gap_terms(dy, dpool, gate, x, state, act, dtype, exp_form=False):
    x, dy = _t(x, dtype), _t(dy, dtype)
    hw = x.shape[1]
    s = torch.ones((), dtype=dtype) if gate is None else _t(gate, dtype).unsqueeze(1)
    q = (_t(dpool, dtype) * torch.tensor(1.0 / hw, dtype=dtype)).unsqueeze(1)
    ad = act_der(N.affine(x, state["scale"], state["shift"], dtype), act, exp_form)
    xh = (x - _t(state["save_mean"], dtype)) * _t(state["save_rstd"], dtype)
    return ad * (dy * s), ad * q, xh


def gap_backward(dy, dpool, gate, x, state, act, dtype=F64):
    """dict of dbeta, dgamma, dx of embnet_bn_bwd_gap / _gap_sums; float32: the stand-in."""
    n, hw, c = x.shape
    t1, t2, xh = _gap_terms(dy, dpool, gate, x, state, act, dtype, exp_form=dtype == F32)
    dz = t1 + t2
    db, dg = dz.sum((0, 1)), (dz * xh).sum((0, 1))
    inv_m = torch.tensor(1.0 / (n * hw), dtype=dtype)
    return dict(dbeta=db, dgamma=dg, dx=_t(state["scale"], dtype) * (dz - db * inv_m - xh * dg * inv_m))


def gap_sum_bounds(dy, dpool, gate, x, state, act):
    """((dbeta, dgamma) references, (their bounds)) per channel: form (b) of the module docstring."""
    n, hw, c = x.shape
    m = n * hw
    t1, t2, xh = _gap_terms(dy, dpool, gate, x, state, act, F64)
    dz, mag = t1 + t2, t1.abs() + t2.abs()
    eb = eg = bb = bg = torch.zeros(c, dtype=F64)
    if act == 2:                                           # E32 in the kappa form, on the magnitudes in front of a'
        o1, o2, _ = _gap_terms(dy, dpool, gate, x, state, 0, F64)
        kd = kappa_der(x.reshape(-1, c), state["scale"], state["shift"], 2)
        eb, eg = kd * (o1.abs() + o2.abs()).sum((0, 1)), kd * ((o1.abs() + o2.abs()) * xh.abs()).sum((0, 1))
    if act == 1:
        bd = border(x, state["scale"], state["shift"]).double()
        o1, o2, _ = _gap_terms(dy, dpool, gate, x, state, 0, F64)
        bb, bg = ((o1.abs() + o2.abs()) * bd).sum((0, 1)), ((o1.abs() + o2.abs()) * xh.abs() * bd).sum((0, 1))
    return (dz.sum((0, 1)), (dz * xh).sum((0, 1))), (gamma(m + 3) * mag.sum((0, 1)) + 4 * eb + bb, gamma(m + 6) * (mag * xh.abs()).sum((0, 1)) + 4 * eg + bg)


def check_gap_backward(dy, dpool, gate, x, state, act, out, key, what="bn_bwd_gap"):
    """dbeta / dgamma per channel (form (b)) and dx per element of one embnet_bn_bwd_gap / _gap_sums call."""
    n, hw, c = x.shape
    (rb, rg), (bb, bg) = gap_sum_bounds(dy, dpool, gate, x, state, act)
    r = {"%s dbeta act%d" % (key, act): within((_t(out["dbeta"]) - rb).abs(), bb, what + " dbeta"),
         "%s dgamma act%d" % (key, act): within((_t(out["dgamma"]) - rg).abs(), bg, what + " dgamma")}
    s = torch.ones((), dtype=F64) if gate is None else _bc(gate)
    t1, t2 = _t(dy) * s, (_t(dpool) / hw).unsqueeze(1).expand(n, hw, c)
    r["%s dx act%d" % (key, act)] = check_dx(x.reshape(-1, c), (t1 + t2).reshape(-1, c), (t1.abs() + t2.abs()).reshape(-1, c), state, act, 1,
                                            out["dbeta"], out["dgamma"], _t(out["dx"]).reshape(-1, c), what + " dx")
    return r


def check_gap_finalize(sums, gate, dpool, hw, dbeta, dgamma, what="bn_bwd_gap_sums finalize"):
    """Form (a): dbeta / dgamma against the double-precision combination of the kernel's own [n][5][c] sums."""
    S, s, q = _t(sums), _t(gate), _t(dpool) / hw
    n = S.shape[0]
    g3 = gamma(3) + n * 2.0 ** -52
    r = {}
    for name, got, i in (("dbeta", dbeta, 1), ("dgamma", dgamma, 3)):
        ref, mag = (s * S[:, i] + q * S[:, i + 1]).sum(0), ((s * S[:, i]).abs() + (q * S[:, i + 1]).abs()).sum(0)
        r["finalize " + name] = within((_t(got) - ref).abs(), g3 * mag, "%s %s" % (what, name))
    return r


def check_gap_agree(dy, dpool, gate, x, state, act, o1, o2, what="bn_bwd_gap vs bn_bwd_gap_sums"):
    """The reduction-pass and the sums forms of the same backward: the sum of the two bounds."""
    n, hw, c = x.shape
    m = n * hw
    _, (bb, bg) = gap_sum_bounds(dy, dpool, gate, x, state, act)
    ddb, ddg = (_t(o1["dbeta"]) - _t(o2["dbeta"])).abs(), (_t(o1["dgamma"]) - _t(o2["dgamma"])).abs()
    r = {"agree dbeta": within(ddb, 2 * bb, what + " dbeta"), "agree dgamma": within(ddg, 2 * bg, what + " dgamma")}
    sc = _t(state["scale"]).abs()
    xh = ((_t(x) - _t(state["save_mean"])) * _t(state["save_rstd"])).abs()
    mag = (_t(dy) * _bc(gate)).abs() + (_t(dpool) / hw).abs().unsqueeze(1)
    kd = kappa_der(x.reshape(-1, c), state["scale"], state["shift"], act)
    sums = (_t(o1["dbeta"]).abs() + _t(o2["dbeta"]).abs()) / m + xh * (_t(o1["dgamma"]).abs() + _t(o2["dgamma"]).abs()) / m
    bound = gamma(7) * sc * (2 * mag + sums) + 8 * kd * sc * mag + sc * (ddb + xh * ddg) / m
    r["agree dx"] = within((_t(o1["dx"]) - _t(o2["dx"])).abs(), bound, what + " dx")
    return r


# ---- the squeeze-and-excite MLP -----------------------------------------------------------------------------------------------------------
MLP_FAMILIES = FAMILIES + ["saturated"]
MlpCase = namedtuple("MlpCase", "pooled w1 b1 w2 b2 dgate")


@functools.lru_cache(maxsize=256)
def mlp_case(family, n, c, S, seed=0):
    """pooled [n, c] (nn_ref.bn_case's x of the family over [n, c]; quiet_image17: the last sample at 2^-17), He-scaled W1 [c, S] and
    W2 [S, c], biases 0.1 randn, dgate the family's gradient.  saturated: b2 a permutation of linspace(-30, 30, c): logits over +-30."""
    base = family if family in ("even", "spread17", "zero", "relu") else "even"
    bc = bn_case(base, n, c, seed=seed + 23)
    g = torch.Generator().manual_seed(seed * 7919 + 389 * MLP_FAMILIES.index(family) + 131 * n + 17 * c + S)
    pooled, dgate = bc.x.clone(), bc.dy.clone()
    if family == "quiet_image17":
        pooled[-1] *= QUIET
        dgate[-1] *= QUIET
    w1 = torch.randn(c, S, generator=g) * (2.0 / c) ** 0.5
    w2 = torch.randn(S, c, generator=g) * (2.0 / S) ** 0.5
    b1, b2 = 0.1 * torch.randn(S, generator=g), 0.1 * torch.randn(c, generator=g)
    if family == "saturated":
        b2 = torch.linspace(-30.0, 30.0, c)[torch.randperm(c, generator=g)]
    return MlpCase(*(t.contiguous() for t in (pooled, w1, b1, w2, b2, dgate)))


def mlp_forward(case, dtype=F64):
    """(z1, gate); float32: the stand-in, both sigmoids through exp."""
    p, w1, b1, w2, b2 = (_t(v, dtype) for v in case[:5])
    z1 = p @ w1 + b1
    a = act_kind(z1, 1, dtype, exp_form=dtype == F32) @ w2 + b2
    return z1, act_kind(a, 0, dtype, exp_form=dtype == F32)


def mlp_backward(case, gate, z1, dtype=F64):
    p, w1, _, w2, _, dgate = (_t(v, dtype) for v in case)
    g, z = _t(gate, dtype), _t(z1, dtype)
    dz2 = dgate * g * (1 - g)
    dz1 = (dz2 @ w2.T) * act_kind_der(z, 1, dtype, exp_form=dtype == F32)
    h = act_kind(z, 1, dtype, exp_form=dtype == F32)
    return dict(dz1=dz1, dpooled=dz1 @ w1.T, dw1=p.T @ dz1, db1=dz1.sum(0), dw2=h.T @ dz2, db2=dz2.sum(0))


def mlp_logits(case, z1):
    """float64 logits a = swish(z1) W2 + b2 from the given (the kernel's own) z1."""
    return act_kind(z1, 1) @ _t(case.w2) + _t(case.b2)


def check_mlp_fwd(case, z1, gate, what="se_mlp_fwd"):
    p, w1, b1, w2, b2 = (_t(v) for v in case[:5])
    c, S = w1.shape
    r = {"mlp z1": within((_t(z1) - (p @ w1 + b1)).abs(), gamma(c + 1) * (p.abs() @ w1.abs() + b1.abs()), what + " z1")}
    z = _t(z1)
    h = act_kind(z, 1)
    a = h @ w2 + b2
    ea = gamma(S + 1) * (h.abs() @ w2.abs() + b2.abs()) + (4 * kappa_fwd(z.reshape(-1, 1), ONE, ZERO, 2) * z.abs()) @ w2.abs()
    s = torch.sigmoid(a)
    bound = torch.exp(ea) * s * (1 - s) * ea + 4 * sigmoid_kappa(a) * s * (1 + a.abs())
    r["mlp gate"] = within((_t(gate) - s).abs(), bound, what + " gate")
    return r


def check_mlp_bwd(case, gate, z1, out, what="se_mlp_bwd"):
    p, w1, _, w2, _, dgate = (_t(v) for v in case)
    n, c = p.shape
    S = w1.shape[1]
    g, z = _t(gate), _t(z1)
    dz2 = dgate * g * (1 - g)
    m = dz2.abs() @ w2.abs().T
    swd = act_kind_der(z, 1)
    kd = float((act_kind_der(z, 1, F32).double() - swd).abs().max())
    r = {"mlp dz1": within((_t(out["dz1"]) - (dz2 @ w2.T) * swd).abs(), gamma(c + 4) * swd.abs() * m + 4 * kd * m, what + " dz1")}
    own = _t(out["dz1"])
    r["mlp dpooled"] = within((_t(out["dpooled"]) - own @ w1.T).abs(), gamma(S) * own.abs() @ w1.abs().T, what + " dpooled")
    r["mlp dW1"] = within((_t(out["dw1"]) - p.T @ own).abs(), gamma(n) * p.abs().T @ own.abs(), what + " dW1")
    r["mlp db1"] = within((_t(out["db1"]) - own.sum(0)).abs(), gamma(n) * own.abs().sum(0), what + " db1")
    h = act_kind(z, 1)
    e32 = (kappa_fwd(z.reshape(-1, 1), ONE, ZERO, 2) * z.abs()).T @ dz2.abs()
    r["mlp dW2"] = within((_t(out["dw2"]) - h.T @ dz2).abs(), gamma(n + 3) * h.abs().T @ dz2.abs() + 4 * e32, what + " dW2")
    r["mlp db2"] = within((_t(out["db2"]) - dz2.sum(0)).abs(), gamma(n + 3) * dz2.abs().sum(0), what + " db2")
    return r


old_close = N.old_close

# ---- the cases both test files run ---------------------------------------------------------------------------------------------------
# (n, hw, c) of the per-(image, channel) kernels; what each reaches is tabulated (and asserted) in test_se_ref_cpu.py
QUAD_SHAPES = [s for s in GAP_CASES if s[2] % 4 == 0] + [(3, 9, 12), (2, 33, 32), (2, 196, 80), (1, 257, 8), (2, 1, 64), (70, 4, 16), (65, 3, 68),
                                                         (1, 37, 1028), (4, 625, 4), (3, 99, 48), (3, 99, 256)]
SCALAR_SHAPES = [s for s in GAP_CASES if s[2] % 4] + [(2, 17, 6), (2, 5, 258)]
BIG_SHAPE = (5, 1024, 1028)                                # total4 = 1 315 840 > 4096 * 256: the second trip of every grid-stride loop
EW_TOTALS = [1, 255, 257, 1048577]                         # activation / absdiff / dropout; 4096 * 256 + 1: one element on the second trip
DROP_PER_SAMPLE = (1, 37, 4099)                            # 37 and 4099 divide neither 256 nor a grid stride
MLP_SHAPES = [(1, 4, 1), (3, 20, 1), (2, 40, 10), (5, 56, 14), (65, 96, 16), (64, 96, 17), (7, 240, 48), (7, 240, 49), (3, 64, 64), (3, 64, 65),
              (9, 640, 160), (3, 1028, 17), (2, 4096, 8), (130, 36, 9)]
