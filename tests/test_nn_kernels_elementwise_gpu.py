"""The kernels BETWEEN the convolutions — BatchNormalization, max pooling, the fused BN -> act -> pad -> pool stem and global average
pooling of csrc/nn_kernels.hip — through the C ABI against float64 (tests/nn_ref.py), PER ELEMENT and PER CHANNEL.

BatchNorm is the one layer whose whole job is to treat every channel by that channel's own scale, and every activation of every
backbone passes through these kernels twice per step; the neighbouring tests (test_backbone_gpu.py, test_bn_backward_forms_gpu.py,
the fused forms of test_round4_gpu.py) compare through layers.py at 1e-5 of the largest value of the whole tensor, on inputs whose
channels share one scale, at channel counts that reach a fraction of the reduction geometry, on the pool's fast path only.  Here
every bound is the textbook one, derived in tests/nn_ref.py's docstring from the rounding counts of the kernel source (u = 2^-24,
gamma(n)); only `error <= bound` is asserted, the ratios are printed (pytest -s).  tests/test_nn_ref_cpu.py holds the float32 CPU
evaluation against the same check functions.

  families   even, spread17 (per-channel amplitudes over 2^17), zero (every fourth channel all zero), relu, offset8 (per-channel
             mean = 8 std, alternating sign, on spread17 amplitudes), const (one channel per quad constant: var = 0); every third
             gamma negative, beta = 0.3 randn, eps 1e-3 and 2e-5;
  BatchNorm  embnet_bn_train_fwd (+ momentum 0: var_k itself; y = NULL; by-channel partial_in at 8 and 7 rows), embnet_bn_bwd with
             training 1 and 0 (+ dx_add), embnet_bn_bwd_inrelu, embnet_bn_infer_fwd, act 0 / 1 / 2, at the (m, c) of nn_ref.BN_SHAPES:
             each the smallest shape that reaches its branch of the reductions by the col_geom mirror (all nine of the issue's shapes
             do; the table is in test_nn_ref_cpu.py);
  pools      embnet_maxpool_fwd / _bwd / _relu_bwd_colsum, n = 2, c 8, 20 and 6 (the scalar pair; the colsum form needs c % 4 == 0),
             seven geometries x post-ReLU / quantised / all-negative inputs;
  fused stem embnet_bn_act_maxpool_fwd / _bwd, c 8 and 64, act 0 / 1 / 2, training 1 / 0, xwin given and NULL (bit-identical),
             forward bit-identical to embnet_affine_act + embnet_maxpool_fwd; pool_bn_bwd_apply4_kernel's path is not in the trace:
             k <= 2 stride is the four-candidate fast path ((3,2,1,15,17), (2,2,0,12,10)), (3,1,1,7,9) the general one;
  GAP        embnet_gap_fwd, embnet_gap_bwd (+ dx_add), embnet_affine_act_gap (y given and NULL) at nn_ref.GAP_CASES.  Finding:
             (1, 1025, 8) runs affine_act_gap4_kernel on 1024 threads (512 pixel lanes), where the four-pixel loop needs hw > 1536:
             it reaches the tail loop only; (1, 2051, 8) is added and runs the loop plus its tail there;
  memory     every output — argmax and xwin too — sits in a larger buffer with a 4 KB sentinel margin on both sides: no sentinel left
             inside, the margins untouched; the workspace is exactly embnet_bn_workspace_bytes /
             embnet_bn_act_maxpool_bwd_workspace_bytes long, between margins;
  selection  which kernel ran is asserted from the kernel trace (embnet_trace_*) at every call.

MEASURED ON AN MI355X — every assertion holds, no kernel needed a change.  Largest error / bound per quantity and family over all
shapes, both eps (printed by the last test, not asserted beyond <= 1); `cpu` = the float32 CPU evaluation's largest figure over all
families (tests/test_nn_ref_cpu.py).  act 0 / 1 / 2 where three figures stand:

  quantity                       even            spread17        zero            relu            offset8         const           cpu
  mean                           0.017           0.018           0.018           0.048           0.042           0.105           0.090
  var_k (momentum 0)             0.176           0.061           0.144           0.028           0.182           0.209           -
  rstd                           0.176           0.571           0.323           0.323           0.569           0.208           0.571
  moving_mean / moving_var       0.42 / 0.71     0.88 / 0.90     0.47 / 0.73     0.59 / 0.76     0.90 / 0.78     0.74 / 0.72     0.90 / 0.90
  scale / shift                  0.97 / 0.49     0.98 / 0.47     0.98 / 0.47     0.98 / 0.49     0.99 / 0.49     0.98 / 0.50     0.99 / 0.86
  y                              1.00 1.00 0.24  1.00 1.00 0.22  1.00 1.00 0.24  1.00 1.00 0.24  1.00 1.00 0.28  1.00 1.00 0.29  1.00 1.00 0.26
  y, statistics from partial_in  0.993           0.992           0.996           0.993           0.996           0.999           -
  inference scale / shift        0.54 / 0.48     0.54 / 0.48     0.53 / 0.49     0.56 / 0.48     0.54 / 0.49     0.56 / 0.49     0.61 / 0.80
  dbeta                          .049 .048 .144  .045 .060 .188  .055 .052 .075  .053 .049 .539  .042 .049 .224  .051 .047 .218  .110 .097 .224
  dgamma                         .060 .078 .143  .064 .071 .066  .054 .058 .100  .062 .067 .095  .079 .055 .069  .054 .071 .081  .121 .121 .114
  dx                             0.51 0.51 0.50  0.53 0.51 0.41  0.55 0.48 0.43  0.52 0.45 0.46  0.43 0.43 0.42  0.46 0.48 0.47  0.55 0.64 0.55
  dx, frozen statistics          1.00 1.00 0.44  1.00 1.00 0.35  1.00 1.00 0.30  1.00 1.00 0.62  1.00 1.00 0.39  1.00 1.00 0.31  1.00 1.00 0.53
  dx + dx_add                    0.45 0.83 0.68  0.99 0.98 0.98  0.47 0.86 0.63  0.50 0.68 0.60  0.97 0.99 0.96  0.64 0.78 0.54  0.98 0.98 0.98
  in-ReLU dz                     0.51 0.50 0.50  0.53 0.46 0.48  0.46 0.48 0.48  0.53 0.45 0.49  0.48 0.47 0.48  0.46 0.47 0.47  0.50 0.53 0.55
  in-ReLU dbias                  0.048           0.057           0.046           0.048           0.052           0.050           0.119
  fused stem dx                  0.50 0.50 0.49  0.45 0.46 0.56  0.45 0.49 0.47  0.50 0.46 0.48  0.44 0.47 0.50  0.53 0.46 0.51  0.56 0.53 0.62
  fused stem dx, frozen          0.99 1.00 0.31  0.98 0.97 0.26  0.99 0.99 0.29  0.99 0.99 0.24  0.99 0.99 0.30  0.99 0.98 0.24  0.99 1.00 0.31
  GAP forward                    0.019           0.028           0.020           0.057           0.099           0.208           0.056
  GAP backward / + dx_add        0.64 / 1.00     0.66 / 1.00     0.63 / 0.99     0.65 / 0.99     0.66 / 0.99     0.62 / 1.00     0.49 / 1.00
  affine_act_gap mean, y / NULL  0.04 / 0.19     0.05 / 0.26     0.05 / 0.30     0.05 / 0.22     0.06 / 0.19     0.05 / 0.19     0.09 / 0.30

  max pool                       post-ReLU       quantised       all-negative    cpu
  dx                             0.992           0.999           0.987           0.999
  maxpool_relu_bwd_colsum dbias  0.354           0.289           0 (all masked)  0.354

(1.00 stands for 0.99..: ONE rounding against u |value| — y by one fma, the frozen dx, a sum of two terms; such a bound cannot be
missed by a correct kernel and leaves no slack for a wrong one.  The dx figures near 0.5 come from m = 1, where dz - dbeta / m
cancels.  The swish sums need at most 0.54 of gamma mag + 4 E32 — relu's dbeta, the device's __expf against torch.sigmoid.)

offset8, the cancellation in var = E[x^2] - mean^2 at |mean| = 8 std, from the momentum-0 call: largest |var_k - var| / var per shape
(eps does not enter), always inside Ev (0.18 of it at most) — the figure a change to the variance formula is judged against:
  (37, 4) 7.6e-6   (2500, 4) 8.3e-6   (297, 48) 6.3e-6   (297, 256) 4.0e-6   (37, 1028) 1.0e-5   (98, 3) 7.8e-6   (297, 6) 9.3e-6
  (37, 258) 6.0e-6   ((1, 4): var = 0 and var_k = 0 exactly) — about 100 u: E[x^2] / var = 65 times the rounding of the two sums.
The whole file (101 tests) costs 7 s on the GPU.
"""
import os
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd._lib import check, stream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref as N  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 1024                                              # 32-bit words: 4 KB on both sides
PATTERN = 0x7FC0BEEF                                       # a NaN no arithmetic produces; none of its bytes is a tap index
RATIOS = {}                                                # (quantity, family) -> largest error / bound
VARREL = {}                                                # (m, c, eps) -> largest |var_k - var| / var of offset8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
class Guard:
    """A tensor of `shape` between two 4 KB margins of PATTERN words."""

    def __init__(self, shape, dev, dtype=torch.float32, init=None):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        words = -(-self.nbytes // 4)
        self.big = torch.full((words + 2 * MARGIN,), PATTERN, dtype=torch.int32, device=dev)
        self.bytes = self.big.view(torch.uint8)
        self.t = self.bytes[4 * MARGIN:4 * MARGIN + self.nbytes].view(dtype).view(*shape)
        if init is not None:
            self.t.copy_(init)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what, written=True):
        """Margins untouched; written: no sentinel left inside (None: the inside is a workspace; False: it must be untouched)."""
        lo, hi = 4 * MARGIN, 4 * MARGIN + self.nbytes
        pat = torch.full_like(self.big, PATTERN).view(torch.uint8)
        assert torch.equal(self.bytes[:lo], pat[:lo]) and torch.equal(self.bytes[hi:], pat[hi:]), what + ": wrote outside its buffer"
        if written is False:
            assert torch.equal(self.bytes[lo:hi], pat[lo:hi]), what + ": the buffer was written"
        elif written:
            if self.t.dtype == torch.uint8:
                left = (self.t == 0xEF) | (self.t == 0xBE) | (self.t == 0xC0) | (self.t == 0x7F)
            else:
                left = torch.isnan(self.t)
            assert not bool(left.any()), what + ": an element was not written (or is NaN)"
        return self.t


def traced(fn):
    _lib.trace_reset(); _lib.trace_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in _lib.trace_records()]
    finally:
        _lib.trace_enable(False)


def note(r, family):
    for k, v in r.items():
        assert v <= 1.0, (k, family, v)
        RATIOS[(k, family)] = max(RATIOS.get((k, family), 0.0), v)


def workspace(nbytes, dev):
    return Guard((max(nbytes, 4) // 4,), dev)


STATS4, STATS, FINAL, AFFINE = "embnet::bn_stats4_kernel", "embnet::bn_stats_kernel", "embnet::bn_finalize_kernel", "embnet::affine_act_kernel"
RED4, RED, APPLY4, APPLY = ("embnet::bn_bwd_reduce4_kernel", "embnet::bn_bwd_reduce_kernel", "void embnet::bn_bwd_apply4_kernel<0>",
                            "embnet::bn_bwd_apply_kernel")
INRELU = "embnet::bn_bwd_apply_inrelu4_kernel"
STATE = ("save_mean", "save_rstd", "scale", "shift")


def train_fwd(dev, x, case, eps, act, momentum=N.MOMENTUM, with_y=True, partial=None):
    """embnet_bn_train_fwd on guarded buffers -> (outputs on the device, outputs on the CPU, kernel names)."""
    lib = _lib.lib()
    m, c = x.shape
    g = {k: Guard((c,), dev) for k in STATE}
    g["moving_mean"], g["moving_var"] = Guard((c,), dev, init=case.mm), Guard((c,), dev, init=case.mv)
    g["y"] = Guard((m, c), dev)
    gam, beta = case.gamma.to(dev), case.beta.to(dev)
    nbytes = lib.embnet_bn_workspace_bytes(m, c)
    ws = workspace(nbytes, dev)
    rows = 0 if partial is None else partial.shape[-1]
    names = traced(lambda: check(lib.embnet_bn_train_fwd(
        x.data_ptr(), m, c, gam.data_ptr(), beta.data_ptr(), eps, momentum, act, g["y"].ptr() if with_y else None, g["save_mean"].ptr(),
        g["save_rstd"].ptr(), g["scale"].ptr(), g["shift"].ptr(), g["moving_mean"].ptr(), g["moving_var"].ptr(),
        None if partial is None else partial.data_ptr(), rows, ws.ptr(), nbytes, stream())))
    ws.check("bn_train_fwd workspace", written=None)
    out = {k: v.check("bn_train_fwd " + k, written=with_y or k != "y") for k, v in g.items()}
    if not with_y:
        del out["y"]
    return out, {k: v.cpu() for k, v in out.items()}, names


def bn_bwd(dev, x, dy, state, act, training, dx_add=None, inrelu=False):
    lib = _lib.lib()
    m, c = x.shape
    g = {"dx": Guard((m, c), dev), "dgamma": Guard((c,), dev), "dbeta": Guard((c,), dev)}
    nbytes = lib.embnet_bn_workspace_bytes(m, c)
    ws = workspace(nbytes, dev)
    st = [state[k].data_ptr() for k in STATE]
    if inrelu:
        g["dbias"] = Guard((c,), dev)
        names = traced(lambda: check(lib.embnet_bn_bwd_inrelu(dy.data_ptr(), x.data_ptr(), m, c, *st, act, training, g["dx"].ptr(), g["dgamma"].ptr(),
                                                              g["dbeta"].ptr(), g["dbias"].ptr(), ws.ptr(), nbytes, stream())))
    else:
        names = traced(lambda: check(lib.embnet_bn_bwd(dy.data_ptr(), x.data_ptr(), m, c, *st, act, training, None if dx_add is None else dx_add.data_ptr(),
                                                       g["dx"].ptr(), g["dgamma"].ptr(), g["dbeta"].ptr(), None, ws.ptr(), nbytes, stream())))
    ws.check("bn_bwd workspace", written=None)
    return {k: v.check("bn_bwd " + k).cpu() for k, v in g.items()}, names


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,c", N.BN_SHAPES)
@pytest.mark.parametrize("family", N.BN_FAMILIES)
def test_batchnorm_per_element_and_per_channel(dev, family, m, c):
    lib = _lib.lib()
    case = N.bn_case(family, m, c)
    x, dy = case.x.to(dev), case.dy.to(dev)
    quad = c % 4 == 0
    assert N.reduce_geom(m, c)[1] == quad
    fwd_names = [STATS4 if quad else STATS, FINAL, AFFINE]
    bwd_names = [RED4, APPLY4] if quad else [RED, APPLY]
    for eps in N.EPS_VALUES:
        eps = N.f32(eps)
        st = N.bn_stats(case.x, eps)
        # momentum 0: the moving statistics come back as (float)mean_k and (float)var_k themselves
        _, o0, names = train_fwd(dev, x, case, eps, 0, momentum=0.0)
        assert names == fwd_names, names
        note({"var": N.within((o0["moving_var"].double() - st.var).abs(), st.Ev, "var_k")}, family)
        assert torch.equal(o0["moving_mean"], o0["save_mean"])
        if family == "offset8":
            live = st.var > 0
            VARREL[(m, c, eps)] = float(((o0["moving_var"].double() - st.var).abs()[live] / st.var[live]).max()) if bool(live.any()) else 0.0
        for act in (0, 1, 2):
            sd, out, names = train_fwd(dev, x, case, eps, act)
            assert names == fwd_names, names
            note(N.check_bn_forward(case, eps, act, out), family)
            for training in (1, 0):
                got, names = bn_bwd(dev, x, dy, sd, act, training)
                assert names == bwd_names, names
                note(N.check_bn_backward(case, out, act, training, got), family)
                if quad:
                    got, names = bn_bwd(dev, x, dy, sd, act, training, inrelu=True)
                    assert names == [RED4, INRELU], names
                    note(N.check_bn_backward(case, out, act, training, got, inrelu=True), family)
            if (m, c) == (297, 48):
                add = (torch.randn(m, c, generator=torch.Generator().manual_seed(5)) * 1e-3)
                got, names = bn_bwd(dev, x, dy, sd, act, 1, dx_add=add.to(dev))
                assert names == bwd_names, names
                note(N.check_bn_backward(case, out, act, 1, got, dx_add=add), family)
            # inference, from the moving statistics of the case
            gi = {k: Guard((c,), dev) for k in ("scale", "shift")}
            gi["y"] = Guard((m, c), dev)
            gam, beta, mm, mv = (v.to(dev) for v in (case.gamma, case.beta, case.mm, case.mv))
            names = traced(lambda: check(lib.embnet_bn_infer_fwd(x.data_ptr(), m, c, gam.data_ptr(), beta.data_ptr(), mm.data_ptr(), mv.data_ptr(), eps, act,
                                                                 gi["y"].ptr(), gi["scale"].ptr(), gi["shift"].ptr(), stream())))
            assert names == [AFFINE], names
            note(N.check_bn_infer(case, eps, act, {k: v.check("bn_infer " + k).cpu() for k, v in gi.items()}), family)
        # statistics only: y = NULL writes no y and launches no apply pass
        _, out, names = train_fwd(dev, x, case, eps, 1, with_y=False)
        assert names == fwd_names[:2], names
        note(N.check_bn_forward(case, eps, 1, out), family)
        if (m, c) == (297, 48):
            # by-channel partials [2][c][rows] of a conv epilogue, formed in float32 on the CPU: 8 rows take block_partial_sums'
            # 16-byte loads, 7 the scalar ones; no statistics kernel runs
            for rows in (8, 7):
                part = Guard((2, c, rows), dev, init=N.partials(case.x, rows))
                assert part.ptr() % 16 == 0
                _, out, names = train_fwd(dev, x, case, eps, 0, partial=part.t)
                assert names == [FINAL, AFFINE], names
                note({k + " partial_in": v for k, v in N.check_bn_forward(case, eps, 0, out).items()}, family)


# ---- max pooling ------------------------------------------------------------------------------------------------------------------------
POOL4, POOL1 = ["embnet::maxpool_fwd4_kernel", "embnet::maxpool_bwd4_kernel"], ["embnet::maxpool_fwd_kernel", "embnet::maxpool_bwd_kernel"]
COLSUM = "embnet::maxpool_relu_bwd_colsum4_kernel"


@pytest.mark.parametrize("kind", N.POOL_INPUTS)
@pytest.mark.parametrize("k,stride,pad,h,w", N.POOL_GEOMS)
def test_maxpool_bit_identical_forward_and_bounded_backward(dev, k, stride, pad, h, w, kind):
    lib = _lib.lib()
    n = N.POOL_N
    oh, ow = N.pool_out(h, k, stride, pad), N.pool_out(w, k, stride, pad)
    for c in N.POOL_CHANNELS:
        xc, g = N.pool_input(kind, n, h, w, c)
        dyc = N.ST._gradient("even", g, (n, oh, ow, c))
        x, dy = xc.to(dev), dyc.to(dev)
        fwd_name, bwd_name = POOL4 if c % 4 == 0 else POOL1
        y, am, dx = Guard((n, oh, ow, c), dev), Guard((n, oh, ow, c), dev, torch.uint8), Guard((n, h, w, c), dev)
        names = traced(lambda: check(lib.embnet_maxpool_fwd(x.data_ptr(), n, h, w, c, k, stride, pad, oh, ow, y.ptr(), am.ptr(), stream())))
        assert names == [fwd_name], names
        am.check("maxpool argmax")
        names = traced(lambda: check(lib.embnet_maxpool_bwd(dy.data_ptr(), am.ptr(), n, h, w, c, k, stride, pad, oh, ow, dx.ptr(), stream())))
        assert names == [bwd_name], names
        r, _ = N.check_maxpool(xc, dyc, k, stride, pad, y.check("maxpool y").cpu(), am.t.cpu(), dx.check("maxpool dx").cpu())
        note(r, kind)
        if kind == "negative":
            assert bool((am.t == 255).any()) == (pad > 0)
        if c % 4 == 0:
            dz, db = Guard((n, h, w, c), dev), Guard((c,), dev)
            nbytes = lib.embnet_bn_workspace_bytes(n * h * w, c)
            ws = workspace(nbytes, dev)
            names = traced(lambda: check(lib.embnet_maxpool_relu_bwd_colsum(dy.data_ptr(), am.ptr(), x.data_ptr(), n, h, w, c, k, stride, pad, oh, ow,
                                                                            dz.ptr(), db.ptr(), ws.ptr(), nbytes, stream())))
            assert names == [COLSUM], names
            ws.check("colsum workspace", written=None)
            note(N.check_relu_colsum(xc, dx.t.cpu(), dz.check("colsum dz").cpu(), db.check("colsum dbias").cpu()), kind)


# ---- fused BN -> act -> pad -> pool -----------------------------------------------------------------------------------------------------
FUSED_FWD, FUSED_BWD = "embnet::affine_act_maxpool_fwd4_kernel", ["embnet::pool_bn_bwd_reduce4_kernel", "embnet::pool_bn_bwd_apply4_kernel"]


def apply_path(k, stride):
    """The branch of pool_bn_bwd_apply4_kernel (the trace does not name it): four unconditional candidates, or pool_taps_grad4."""
    return "fast" if k <= 2 * stride else "general"


@pytest.mark.parametrize("k,stride,pad,h,w", N.FUSED_GEOMS)
@pytest.mark.parametrize("family", N.BN_FAMILIES)
def test_fused_stem_per_element_and_per_channel(dev, family, k, stride, pad, h, w):
    lib = _lib.lib()
    n, eps = N.POOL_N, N.f32(1e-3)
    oh, ow = N.pool_out(h, k, stride, pad), N.pool_out(w, k, stride, pad)
    assert apply_path(k, stride) == ("general" if (k, stride) == (3, 1) else "fast")
    for c in N.FUSED_CHANNELS:
        case = N.bn_case(family, n * h * w, c, seed=1)
        x = case.x.to(dev)
        xc = case.x.reshape(n, h, w, c)
        sd, st, _ = train_fwd(dev, x, case, eps, 0, with_y=False)
        assert bool((st["scale"] < 0).any())                 # negative gammas reach the kernels
        sp = [sd[key].data_ptr() for key in STATE]
        for act in (0, 1, 2):
            dyc = N.ST._gradient("even", torch.Generator().manual_seed(c + act), (n, oh, ow, c))
            dy = dyc.to(dev)
            fw = {}
            for with_xwin in (True, False):
                y, am, xw = Guard((n, oh, ow, c), dev), Guard((n, oh, ow, c), dev, torch.uint8), Guard((n, oh, ow, c), dev)
                names = traced(lambda: check(lib.embnet_bn_act_maxpool_fwd(x.data_ptr(), n, h, w, c, sp[2], sp[3], act, k, stride, pad, oh, ow, y.ptr(), am.ptr(),
                                                                           xw.ptr() if with_xwin else None, stream())))
                assert names == [FUSED_FWD], names
                fw[with_xwin] = (y.check("fused y"), am.check("fused argmax"), xw.check("fused xwin", written=with_xwin))
            assert torch.equal(fw[True][0], fw[False][0]) and torch.equal(fw[True][1], fw[False][1])
            y, am, xw = fw[True]
            # the unfused chain, bit for bit; and the pool rule on the chain's fp32 activations
            a, y2, am2 = Guard((n, h, w, c), dev), Guard((n, oh, ow, c), dev), Guard((n, oh, ow, c), dev, torch.uint8)
            check(lib.embnet_affine_act(x.data_ptr(), n * h * w, c, sp[2], sp[3], act, a.ptr(), stream()))
            check(lib.embnet_maxpool_fwd(a.ptr(), n, h, w, c, k, stride, pad, oh, ow, y2.ptr(), am2.ptr(), stream()))
            torch.cuda.synchronize()
            assert torch.equal(y, y2.check("unfused y")) and torch.equal(am, am2.check("unfused argmax"))
            note({"fused a act%d" % act: N.check_y(case.x, st["scale"], st["shift"], act, a.check("affine_act y").cpu().reshape(-1, c), "affine_act")}, family)
            yr, ar = N.maxpool_fwd(a.t.cpu(), k, stride, pad)
            amc = am.cpu()
            assert torch.equal(y.cpu(), yr) and torch.equal(amc, ar)
            assert torch.equal(xw.cpu(), N.maxpool_gather(xc, amc, k, stride, pad))
            for training in (1, 0):
                res = {}
                for with_xwin in (True, False):
                    g = {"dx": Guard((n, h, w, c), dev), "dgamma": Guard((c,), dev), "dbeta": Guard((c,), dev)}
                    nbytes = lib.embnet_bn_act_maxpool_bwd_workspace_bytes(n, oh, ow, c)
                    ws = workspace(nbytes, dev)
                    names = traced(lambda: check(lib.embnet_bn_act_maxpool_bwd(
                        dy.data_ptr(), am.data_ptr(), x.data_ptr(), n, h, w, c, k, stride, pad, oh, ow, *sp, act, training, xw.data_ptr() if with_xwin else None,
                        g["dx"].ptr(), g["dgamma"].ptr(), g["dbeta"].ptr(), ws.ptr(), nbytes, stream())))
                    assert names == FUSED_BWD, names
                    ws.check("fused bwd workspace", written=None)
                    res[with_xwin] = {key: v.check("fused bwd " + key).cpu() for key, v in g.items()}
                for key in ("dx", "dgamma", "dbeta"):
                    assert torch.equal(res[True][key], res[False][key]), key + ": xwin given and NULL differ"
                note(N.check_fused_backward(xc, dyc, amc, st, act, training, k, stride, pad, res[True]), family)


# ---- global average pooling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,c", N.GAP_CASES)
def test_gap_per_element(dev, n, hw, c):
    lib = _lib.lib()
    quad = c % 4 == 0
    for family in N.BN_FAMILIES:
        case = N.bn_case(family, n * hw, c, seed=2)
        xc = case.x.reshape(n, hw, c)
        dyc, addc = case.dy[:n].contiguous(), case.dy.reshape(n, hw, c)
        x, dy, add = xc.to(dev), dyc.to(dev), addc.to(dev)
        y = Guard((n, c), dev)
        names = traced(lambda: check(lib.embnet_gap_fwd(x.data_ptr(), n, hw, c, y.ptr(), stream())))
        assert names == ["embnet::gap_fwd4_kernel" if quad else "embnet::gap_fwd_kernel"], names
        note(N.check_gap_forward(xc, y.check("gap y").cpu()), family)
        for with_add in ((False, True) if quad else (False,)):
            dx = Guard((n, hw, c), dev)
            names = traced(lambda: check(lib.embnet_gap_bwd(dy.data_ptr(), n, hw, c, add.data_ptr() if with_add else None, dx.ptr(), stream())))
            assert names == ["embnet::gap_bwd_add4_kernel" if quad else "embnet::gap_bwd_kernel"], names
            note(N.check_gap_backward(dyc, hw, dx.check("gap dx").cpu(), addc if with_add else None), family)
        if not quad:
            continue
        sc, sh = case.gamma.to(dev), case.beta.to(dev)
        for act in (0, 1, 2):
            gaps = {}
            for with_y in (True, False):
                ya, gp = Guard((n, hw, c), dev), Guard((n, c), dev)
                names = traced(lambda: check(lib.embnet_affine_act_gap(x.data_ptr(), n, hw, c, sc.data_ptr(), sh.data_ptr(), act, ya.ptr() if with_y else None,
                                                                       gp.ptr(), stream())))
                assert names == ["embnet::affine_act_gap4_kernel"], names
                yt = ya.check("affine_act_gap y", written=with_y)
                yk = yt.cpu() if with_y else None
                gaps[with_y] = gp.check("affine_act_gap gap").cpu()
                note(N.check_affine_act_gap(xc, case.gamma, case.beta, act, yk, gaps[with_y]), family)
            assert torch.equal(gaps[True], gaps[False]), "the pooled means with y = NULL differ from those with y"


def test_every_kernel_and_branch_named_is_reached_by_a_case():
    """The tables above against the list of kernels and branches this file exists for: each is asserted from the trace (or, inside
    pool_bn_bwd_apply4_kernel, from k <= 2 stride) by at least one case."""
    geoms = {mc: N.reduce_geom(*mc) for mc in N.BN_SHAPES}
    assert any(q and lds and trips == 1 for _, q, lds, trips, _ in geoms.values())                       # the LDS branch
    assert any(q and trips == 2 for _, q, _, trips, _ in geoms.values())                                 # the quad column loop's second trip
    assert any(q and g.cl == 1 for g, q, _, _, _ in geoms.values())                                      # c = 4: one butterfly
    assert any(not q and trips == 2 for _, q, _, trips, _ in geoms.values())                             # the scalar loop's second trip
    assert any(m < g.rl for (m, _), (g, _, _, _, _) in geoms.items()) and (1, 4) in geoms               # fewer rows than row lanes; m = 1
    assert any(g.blocks > 1 and last < g.rows_per_block for g, _, _, _, last in geoms.values())          # a ragged last row block
    assert {c % 4 == 0 for _, c in N.BN_SHAPES} == {True, False}                                         # bn_stats4 / bn_stats, the reduce / apply pairs
    assert {c % 4 == 0 for c in N.POOL_CHANNELS} == {True, False} and {c % 4 == 0 for _, _, c in N.GAP_CASES} == {True, False}
    assert {apply_path(k, s) for k, s, _, _, _ in N.FUSED_GEOMS} == {"fast", "general"}


def test_zz_print_the_measured_tables():
    """Not an assertion of its own: prints what the tests above measured (pytest -s), for the docstring."""
    fams = N.BN_FAMILIES + list(N.POOL_INPUTS)
    print("\nlargest error / bound\n  %-30s" % "quantity" + "".join("%10s" % f for f in fams))
    for q in sorted({k[0] for k in RATIOS}):
        print("  %-30s" % q + "".join("%10s" % ("%.3f" % RATIOS[(q, f)] if (q, f) in RATIOS else "-") for f in fams))
    print("\noffset8, largest |var_k - var| / var per (m, c, eps):")
    for key in sorted(VARREL):
        print("  m %5d c %5d eps %.0e   %.3e" % (key + (VARREL[key],)))
