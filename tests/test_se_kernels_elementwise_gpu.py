"""Everything between an MBConv block's depthwise BatchNormalization and its residual add — the squeeze-and-excite multiply, the
stand-alone activations, |a - b| and drop-connect of csrc/mbconv_kernels.hip, the fused passes of csrc/nn_kernels.hip
(affine_act_scale4, affine_drop_add4, se_bn_sums4 + se_bn_finalize, bn_bwd_reduce4_gap / bn_bwd_apply4_gap) and the squeeze-and-excite
MLP of csrc/se_mlp.hip — through the C ABI against float64 (tests/se_ref.py), PER ELEMENT and PER (IMAGE, CHANNEL).

Both EfficientNet configs run through these kernels once per block per step, and every quantity in them is scaled per (image,
channel): the gate is a sigmoid that saturates toward 0 for whole (image, channel) pairs, the [n][5][c] sums replace a BatchNorm
reduction pass, drop-connect zeroes whole images.  The neighbouring tests (test_fused_kernels_vs_oracle_gpu.py, test_round4_gpu.py,
test_se_mlp_gpu.py, test_mbconv_siamese_gpu.py) assert 1e-5 of the largest value of the whole tensor, or compare two forms that
share their helpers.  Here every bound is the textbook one of tests/se_ref.py's docstring (u = 2^-24, gamma(k), rounding counts read
off the source); only `error <= bound` is asserted, the ratios are printed by the last test (pytest -s).  tests/test_se_ref_cpu.py
holds the float32 CPU evaluation against the same check functions, the table of which shape reaches which branch, and the guard.

  families   even, spread17 (per-channel amplitudes over 2^17), quiet_image17 (the last image at 2^-17), zero (every fourth channel
             all zero), relu; gates: spread17 (log-uniform over [2^-17, 1] per image and channel; with even, spread17, relu), unit
             (quiet_image17), dropped (rows 0, 2, .. zero, the rest 1 / (1 - rate); with zero), and embnet_affine_drop_add's own factor;
  shapes     se_ref.QUAD_SHAPES (n, hw, c): nn_ref.GAP_CASES and the issue's list, every kernel, act 0 / 1 / 2; SCALAR_SHAPES: the scalar
             chscale_fwd / chscale_bwd kernels; BIG_SHAPE (5, 1024, 1028), even: the second trip of the grid-stride loops;
             EW_TOTALS 1, 255, 257, 1 048 577 x {randn, uniform over +-30}: the activations, |a - b|, drop-connect at per_sample 1, 37,
             4099; MLP_SHAPES (n, c, S) x the five families + saturated (b2 over +-30);
  bitwise    embnet_channel_scale_dgate = chscale_bwd4_kernel's ds;  embnet_affine_act_scale = embnet_affine_act ->
             embnet_channel_scale_fwd;  embnet_affine_drop_add = embnet_affine_act -> embnet_sample_dropout -> embnet_add, and its
             factor = the mask of augment_ref.rng_u32;  (seed, seed_add_dev = a) = (seed + a, NULL);  rate 0 = the identity;
  memory     every output sits in a larger buffer with a 4 KB sentinel margin on both sides: no sentinel left inside, the margins
             untouched; embnet_bn_bwd_gap's workspace is exactly embnet_bn_workspace_bytes long, between margins;
  selection  which kernel ran is asserted from the kernel trace (embnet_trace_*) at every call.

DISPATCH FINDINGS (asserted by the geometry mirrors in test_se_ref_cpu.py):
  * (1, 257, 8) and (4, 625, 4), listed for the 1024-thread form of se_bn_sums4_kernel, do run on 1024 threads but have fewer pixels
    than its 512 / 1024 pixel lanes: they reach the tail statement only.  nn_ref.GAP_CASES' (1, 1025, 8) and (1, 2051, 8) run the
    two-pixel loop plus the tail there, at cls = 2 < 16 (the 'pixel_lane_sums on 1024 threads at cls < 16' candidate); all four stay.
  * ew_blocks_c4 rounds the grid DOWN to a multiple of unit = c4 / gcd(c4, 256): small tensors with unit > 1 — (3, 49, 48) 7 -> 6
    blocks, (3, 99, 48) 14 -> 12, (2, 196, 68) 27 -> 17, (2, 196, 80) 31 -> 30 — already take a second trip of the grid-stride
    loop; BIG_SHAPE takes it at the 4096-block cap (3855 blocks).  (1, 37, 1028): 38 blocks of work, 257 launched (b < unit).
  * The `!fixed` path of affine_act_scale4_kernel / affine_drop_add4_kernel is UNREACHABLE through the host wrappers: ew_blocks_c4
    returns a multiple of unit, so the stride b * 256 = k unit 256 = k c4 (256 / gcd) is always a multiple of c4
    (test_ew_blocks_c4_always_gives_a_stride_that_is_a_multiple_of_c4 walks c4 = 1 .. 1099).  It is left in place.
  * The trace names se_mlp_bwd_b_kernel without its template argument: the S <= 48 / > 48 switch is taken from the mirror.
  * Every shape of MLP_SHAPES is supported by embnet_se_mlp_supported (the mirror agrees with the library): none is skipped.
  * E32 of the swish sums is taken in nn_ref's kappa form (se_ref docstring): the per-pixel |float32 - float64| summed over hw = 1
    pixel is 0 by luck on some (image, channel), and the float32 stand-in itself missed that form at (2, 1, 64).

MEASURED ON AN MI355X — every assertion holds, no kernel needed a change (the three candidates of the issue — se_mlp_bwd_b_kernel's
last workgroup at c % 16 != 0, the 1024-thread pixel_lane_sums at cls < 16, sigmoidf at large negative arguments — are all inside
their bounds).  Largest error / bound per quantity and family over all shapes (printed by the last test, not asserted beyond <= 1);
`cpu` = the float32 CPU evaluation's largest figure over all families (tests/test_se_ref_cpu.py).  act 0 / 1 / 2 where three figures
stand; `logits30` = inputs uniform over +-30, `saturated` = the MLP with b2 over +-30; `big` = BIG_SHAPE; `scalar` = c % 4 != 0:

  quantity                          even      spread17 quiet_image17          zero          relu     saturated      logits30           cpu
  T0 - dgate                 .21 .22 .20   .21 .21 .15   .21 .21 .17   .23 .21 .19   .22 .20 .20             -             -   .17 .12 .07
  absdiff (exact)                  0.000             -             -             -             -             -             -         0.000
  act bwd sigmoid                  0.268             -             -             -             -             -         0.250         0.268
  act bwd swish                    0.264             -             -             -             -             -         0.257         0.264
  act fwd sigmoid                  0.259             -             -             -             -             -         0.339         0.271
  act fwd swish                    0.250             -             -             -             -             -         0.250         0.250
  act_scale y                .97 .95 .24   .96 .96 .26   .50 .50 .22   .89 .89 .24   .98 .98 .26             -             -   .98 .98 .26
  act_scale y act2 big             0.222             -             -             -             -             -             -         0.257
  agree dbeta                      0.189         0.186         0.196         0.190         0.196             -             -         0.196
  agree dgamma                     0.118         0.123         0.177         0.116         0.116             -             -         0.177
  agree dx                         0.796         0.932         0.912         0.967         0.764             -             -             -
  chscale ds                       0.835         0.845         0.835         0.808         0.949             -             -         0.949
  chscale ds scalar                0.493         0.597         0.493         0.438         0.474             -             -         0.949
  chscale dx                       0.998         1.000         0.000         1.000         1.000             -             -         1.000
  chscale dx scalar                0.993         0.977         0.000         0.994         0.980             -             -         1.000
  chscale y                        0.998         0.999         0.000         1.000         0.995             -             -         1.000
  drop_add y                       0.971         0.954         0.974         0.963         0.971             -             -         0.974
  drop_add y big                   0.982             -             -             -             -             -             -         0.974
  finalize dbeta                   0.703         0.666         0.604         0.472         0.684             -             -         0.703
  finalize dgamma                  0.677         0.604         0.483         0.486         0.719             -             -         0.719
  gap dbeta                  .31 .18 .15   .23 .18 .24   .35 .20 .25   .20 .20 .20   .33 .16 .21             -             -   .35 .20 .25
  gap dgamma                 .24 .21 .15   .20 .26 .17   .27 .23 .23   .23 .23 .20   .20 .16 .23             -             -   .32 .26 .26
  gap drop dbeta             .33 .20 .22   .24 .16 .14   .30 .17 .25   .18 .15 .26   .23 .23 .24             -             -   .33 .23 .25
  gap drop dgamma            .31 .30 .28   .28 .24 .20   .29 .27 .17   .30 .27 .16   .26 .21 .19             -             -   .31 .30 .28
  gap drop dx                .51 .46 .49   .48 .47 .41   .49 .52 .43   .46 .47 .46   .45 .46 .56             -             -   .59 .54 .63
  gap dx                     .47 .49 .39   .43 .47 .40   .48 .43 .43   .44 .43 .38   .50 .47 .38             -             -   .56 .54 .54
  gap gated dbeta            .25 .17 .24   .27 .23 .15   .35 .20 .25   .22 .22 .26   .24 .18 .21             -             -   .35 .23 .25
  gap gated dgamma           .22 .27 .18   .32 .19 .13   .27 .23 .23   .34 .34 .13   .19 .19 .19             -             -   .34 .34 .23
  gap gated dx               .54 .48 .38   .50 .46 .40   .48 .43 .43   .52 .54 .47   .46 .44 .43             -             -   .53 .63 .55
  gap sums dbeta             .17 .16 .19   .18 .18 .18   .16 .20 .13   .18 .17 .16   .16 .18 .15             -             -             -
  gap sums dbeta act0 big          0.000             -             -             -             -             -             -             -
  gap sums dgamma            .21 .20 .18   .20 .19 .17   .17 .20 .23   .21 .21 .13   .14 .16 .13             -             -             -
  gap sums dgamma act0 big         0.000             -             -             -             -             -             -             -
  gap sums dx                .53 .48 .37   .44 .47 .40   .45 .45 .42   .53 .54 .46   .46 .55 .42             -             -             -
  gap sums dx act0 big             0.596             -             -             -             -             -             -             -
  mlp dW1                          0.909         0.836         0.827         0.606         0.688         0.911             -         0.939
  mlp dW2                          0.537         0.443         0.449         0.424         0.377         0.384             -         0.500
  mlp db1                          0.544         0.470         0.621         0.414         0.473         0.455             -         0.544
  mlp db2                          0.609         0.599         0.566         0.514         0.575         0.477             -         0.629
  mlp dpooled                      0.972         0.842         0.905         0.931         0.873         0.962             -         0.972
  mlp dz1                          0.209         0.088         0.088         0.071         0.072         0.103             -         0.160
  mlp gate                         0.230         0.245         0.246         0.314         0.238         0.335             -         0.331
  mlp z1                           0.080         0.102         0.224         0.049         0.050         0.244             -         0.151
  sums S1                    .61 .52 .30   .55 .54 .29   .61 .50 .26   .59 .59 .27   .59 .48 .26             -             -   .61 .59 .27
  sums S2                    .00 .00 .27   .00 .00 .28   .00 .00 .25   .00 .00 .54   .00 .00 .23             -             -   .00 .00 .24
  sums S3                    .68 .68 .28   .64 .59 .29   .66 .59 .29   .56 .58 .25   .59 .57 .25             -             -   .68 .68 .32
  sums S4                    .45 .45 .29   .49 .49 .34   .52 .51 .23   .50 .44 .25   .41 .40 .29             -             -   .52 .51 .29
  sums T0                    .72 .72 .24   .84 .84 .22   .75 .75 .22   .71 .58 .19   .83 .83 .20             -             -   .84 .84 .23

(1.000 stands for 0.99..: ONE rounding against u |value|, which a correct kernel cannot miss and which leaves no slack for a wrong
one; 0.000 under quiet_image17 is the unit gate: x * 1 is exact.  S2 of act 0 / 1 is a count and exact.)
NEW FIGURES.  Sigmoid at |v| up to 30 (embnet_activation_fwd kind 0, 1 / (1 + __expf(-v))): 0.339 of 4 kappa_s s (1 + |v|) against
0.259 on randn inputs and 0.271 / 0.250 for the float32 CPU form — the relative error of a gate near 0 does grow with |v|, inside
the scale s (1 + |v|).  se_mlp: z1 <= 0.24, gate <= 0.34 (saturated), dz1 <= 0.21, dpooled <= 0.97 and dW1 <= 0.91 (plain gamma(S) /
gamma(n) chains), db1 <= 0.62, dW2 <= 0.54, db2 <= 0.61.
THE GUARD (test_se_ref_cpu.py::test_the_old_metric_is_blind_to_a_quiet_image_channel, (3, 99, 48)): the gate of the quietest (image,
channel) wrong by 2x is an error of 2.5e-7 of max|ref|; the quiet image's S1 row counted twice 8.2e-8 of max|ref|: both pass the
1e-5-of-max|ref| metric and fail the per-(image, channel) checks (error / bound >> 1).
The whole file (40 tests) costs 6.5 s on the GPU.
"""
import os
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd._lib import check, stream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import se_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 1024                                              # 32-bit words: 4 KB on both sides
PATTERN = 0x7FC0BEEF                                       # a NaN no arithmetic produces
RATIOS = {}                                                # (quantity, family) -> largest error / bound


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
class Guard:
    """A float32 tensor of `shape` between two 4 KB margins of PATTERN words."""

    def __init__(self, shape, dev):
        self.n = int(np.prod(shape))
        self.big = torch.full((self.n + 2 * MARGIN,), PATTERN, dtype=torch.int32, device=dev)
        self.t = self.big[MARGIN:MARGIN + self.n].view(torch.float32).view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what, written=True):
        """Margins untouched; written: no sentinel left inside (None: the inside is a workspace)."""
        assert bool((self.big[:MARGIN] == PATTERN).all()) and bool((self.big[MARGIN + self.n:] == PATTERN).all()), what + ": wrote outside its buffer"
        if written:
            assert not bool(torch.isnan(self.t).any()), what + ": an element was not written (or is NaN)"
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


K = "embnet::"
CH_FWD, CH_BWD4, CH_BWD, CH_DGATE = K + "chscale_fwd_kernel", K + "chscale_bwd4_kernel", K + "chscale_bwd_kernel", K + "chscale_dgate4_kernel"
AFFINE, ACT_SCALE, DROP_ADD, DROPOUT, ADD = (K + "affine_act_kernel", K + "affine_act_scale4_kernel", K + "affine_drop_add4_kernel",
                                             K + "sample_dropout_kernel", K + "add_kernel")
SUMS, GAP_RED, GAP_APPLY = K + "se_bn_sums4_kernel", K + "bn_bwd_reduce4_gap_kernel", K + "bn_bwd_apply4_gap_kernel"
MLP_FWD, MLP_A, MLP_B = K + "semlp::se_mlp_fwd_kernel", K + "semlp::se_mlp_bwd_a_kernel", K + "semlp::se_mlp_bwd_b_kernel"


def run(names, fn, *args):
    got = traced(lambda: check(fn(*args, stream())))
    assert got == names, (got, names)


def p(t):
    return None if t is None else t.data_ptr()


class Ops:
    """The C ABI calls of this file on guarded outputs; every method returns the checked device tensors."""

    def __init__(self, dev):
        self.dev, self.lib = dev, _lib.lib()

    def affine_act(self, x, st, act):
        n, hw, c = x.shape
        y = Guard((n, hw, c), self.dev)
        run([AFFINE], self.lib.embnet_affine_act, p(x), n * hw, c, p(st["scale"]), p(st["shift"]), act, y.ptr())
        return y.check("affine_act")

    def chscale_fwd(self, x, s):
        n, hw, c = x.shape
        y = Guard((n, hw, c), self.dev)
        run([CH_FWD], self.lib.embnet_channel_scale_fwd, p(x), p(s), n, hw, c, y.ptr())
        return y.check("channel_scale_fwd")

    def chscale_bwd(self, x, s, dy):
        n, hw, c = x.shape
        dx, ds = Guard((n, hw, c), self.dev), Guard((n, c), self.dev)
        run([CH_BWD if c % 4 else CH_BWD4], self.lib.embnet_channel_scale_bwd, p(x), p(s), p(dy), n, hw, c, dx.ptr(), ds.ptr())
        return dx.check("channel_scale_bwd dx"), ds.check("channel_scale_bwd ds")

    def dgate(self, x, dy):
        n, hw, c = x.shape
        ds = Guard((n, c), self.dev)
        run([CH_DGATE], self.lib.embnet_channel_scale_dgate, p(x), p(dy), n, hw, c, ds.ptr())
        return ds.check("channel_scale_dgate")

    def act_scale(self, x, st, act, gate):
        n, hw, c = x.shape
        y = Guard((n, hw, c), self.dev)
        run([ACT_SCALE], self.lib.embnet_affine_act_scale, p(x), n, hw, c, p(st["scale"]), p(st["shift"]), act, p(gate), y.ptr())
        return y.check("affine_act_scale")

    def drop_add(self, x, st, rate, seed, seed_add, skip):
        n, hw, c = x.shape
        y, f = Guard((n, hw, c), self.dev), Guard((n, c), self.dev)
        run([DROP_ADD], self.lib.embnet_affine_drop_add, p(x), n, hw, c, p(st["scale"]), p(st["shift"]), rate, seed, p(seed_add), p(skip), y.ptr(), f.ptr())
        return y.check("affine_drop_add y"), f.check("affine_drop_add factor")

    def dropout(self, x, per_sample, rate, seed, seed_add=None):
        y = Guard(tuple(x.shape), self.dev)
        run([DROPOUT], self.lib.embnet_sample_dropout, p(x), x.numel(), per_sample, rate, seed, p(seed_add), y.ptr())
        return y.check("sample_dropout")

    def add(self, a, b):
        y = Guard(tuple(a.shape), self.dev)
        run([ADD], self.lib.embnet_add, p(a), p(b), a.numel(), y.ptr())
        return y.check("add")

    def se_sums(self, dg, x, st, act):
        n, hw, c = x.shape
        s = Guard((n, 5, c), self.dev)
        run([SUMS], self.lib.embnet_se_bn_sums, p(dg), p(x), n, hw, c, p(st["save_mean"]), p(st["save_rstd"]), p(st["scale"]), p(st["shift"]), act, s.ptr())
        return s.check("se_bn_sums")

    def gap_sums(self, dy, dpool, gate, sums, x, st, act):
        n, hw, c = x.shape
        g = {"dx": Guard((n, hw, c), self.dev), "dgamma": Guard((c,), self.dev), "dbeta": Guard((c,), self.dev)}
        run([GAP_APPLY], self.lib.embnet_bn_bwd_gap_sums, p(dy), p(dpool), p(gate), p(sums), n, hw, p(x), c, p(st["save_mean"]), p(st["save_rstd"]),
            p(st["scale"]), p(st["shift"]), act, g["dx"].ptr(), g["dgamma"].ptr(), g["dbeta"].ptr())
        return {k: v.check("bn_bwd_gap_sums " + k).cpu() for k, v in g.items()}

    def gap(self, dy, dpool, gate, x, st, act):
        n, hw, c = x.shape
        g = {"dx": Guard((n, hw, c), self.dev), "dgamma": Guard((c,), self.dev), "dbeta": Guard((c,), self.dev)}
        nbytes = self.lib.embnet_bn_workspace_bytes(n * hw, c)
        assert nbytes % 4 == 0 and nbytes > 0
        ws = Guard((nbytes // 4,), self.dev)
        run([GAP_RED, GAP_APPLY], self.lib.embnet_bn_bwd_gap, p(dy), p(dpool), p(gate), n, hw, p(x), c, p(st["save_mean"]), p(st["save_rstd"]),
            p(st["scale"]), p(st["shift"]), act, g["dx"].ptr(), g["dgamma"].ptr(), g["dbeta"].ptr(), ws.ptr(), nbytes)
        ws.check("bn_bwd_gap workspace", written=None)
        return {k: v.check("bn_bwd_gap " + k).cpu() for k, v in g.items()}


def to_dev(case, dev):
    return (case.x.to(dev), case.dy.to(dev), case.skip.to(dev), case.dpool.to(dev), case.gate.to(dev), {k: v.to(dev) for k, v in case.state.items()})


def seed_word(a, dev):
    return torch.tensor([a], dtype=torch.int64, device=dev)


# ---- the per-(image, channel) kernels -----------------------------------------------------------------------------------------------------
def drop_add_checks(ops, k, d, family, rate, seed):
    """embnet_affine_drop_add: the factor, the three-launch chain bit for bit, float64 per element, seed_add_dev; returns the factor."""
    x, _, skip, _, _, st = d
    n, hw, c = k.x.shape
    y, f = ops.drop_add(x, st, rate, seed, None, skip)
    R.bit_identical(f.cpu(), R.drop_factor(n, c, rate, seed), "affine_drop_add factor against the mask of rng_u32")
    chain = ops.add(ops.dropout(ops.affine_act(x, st, 0), hw * c, rate, seed), skip)
    R.bit_identical(y.cpu(), chain.cpu(), "affine_drop_add against affine_act -> sample_dropout -> add")
    note(R.check_affine_drop_add(k.x, k.state, f.cpu(), k.skip, y.cpu()), family)
    y2, f2 = ops.drop_add(x, st, rate, seed - 7, seed_word(7, ops.dev), skip)
    assert torch.equal(y2, y) and torch.equal(f2, f), "(seed - 7, seed_add_dev = 7) differs from (seed, NULL)"
    return f


@pytest.mark.parametrize("n,hw,c", R.QUAD_SHAPES)
def test_per_image_channel_kernels(dev, n, hw, c):
    ops = Ops(dev)
    zeros = torch.zeros(n, c, device=dev)
    for family in R.FAMILIES:
        k = R.se_case(family, n, hw, c)
        assert R.border_ok(k.x, k.state["scale"], k.state["shift"]), "the ReLU-borderline cap"
        d = to_dev(k, dev)
        x, dy, skip, dpool, gate, st = d
        note(R.check_channel_scale_fwd(k.x, k.gate, ops.chscale_fwd(x, gate).cpu()), family)
        dx, ds = ops.chscale_bwd(x, gate, dy)
        note(R.check_channel_scale_bwd(k.x, k.gate, k.dy, dx.cpu(), ds.cpu()), family)
        R.bit_identical(ops.dgate(x, dy).cpu(), ds.cpu(), "channel_scale_dgate against channel_scale_bwd's ds")
        fac = drop_add_checks(ops, k, d, family, R.DROP_RATE, 1234 + n)
        one = drop_add_checks(ops, k, d, family, 0.0, 5)
        assert bool((one == 1).all())
        for act in (0, 1, 2):
            a_k = ops.affine_act(x, st, act)
            y = ops.act_scale(x, st, act, gate)
            R.bit_identical(y.cpu(), ops.chscale_fwd(a_k, gate).cpu(), "affine_act_scale against affine_act -> channel_scale_fwd")
            note(R.check_affine_act_scale(k.x, k.state, act, k.gate, y.cpu()), family)
            sums = ops.se_sums(dy, x, st, act)
            sc = sums.cpu()
            note(R.check_se_sums(k.dy, k.x, k.state, act, sc), family)
            note(R.check_t0_vs_dgate(k.dy, k.x, k.state, act, sc, a_k.cpu(), ops.dgate(a_k, dy).cpu()), family)
            o_sums = ops.gap_sums(dy, dpool, gate, sums, x, st, act)
            note(R.check_gap_backward(k.dy, k.dpool, k.gate, k.x, k.state, act, o_sums, "gap sums"), family)
            note(R.check_gap_finalize(sc, k.gate, k.dpool, hw, o_sums["dbeta"], o_sums["dgamma"]), family)
            o_gate = ops.gap(dy, dpool, gate, x, st, act)
            note(R.check_gap_backward(k.dy, k.dpool, k.gate, k.x, k.state, act, o_gate, "gap gated"), family)
            note(R.check_gap_agree(k.dy, k.dpool, k.gate, k.x, k.state, act, o_gate, o_sums), family)
            note(R.check_gap_backward(k.dy, k.dpool, None, k.x, k.state, act, ops.gap(dy, dpool, None, x, st, act), "gap"), family)
            note(R.check_gap_backward(k.dy, zeros.cpu(), fac.cpu(), k.x, k.state, act, ops.gap(dy, zeros, fac, x, st, act), "gap drop"), family)


@pytest.mark.parametrize("n,hw,c", R.SCALAR_SHAPES)
def test_scalar_channel_scale_kernels(dev, n, hw, c):
    ops = Ops(dev)
    for family in R.FAMILIES:
        k = R.se_case(family, n, hw, c)
        x, dy, gate = k.x.to(dev), k.dy.to(dev), k.gate.to(dev)
        note(R.check_channel_scale_fwd(k.x, k.gate, ops.chscale_fwd(x, gate).cpu()), family)
        dx, ds = ops.chscale_bwd(x, gate, dy)
        note({q + " scalar": v for q, v in R.check_channel_scale_bwd(k.x, k.gate, k.dy, dx.cpu(), ds.cpu()).items()}, family)


def test_big_case_second_trip_of_the_grid_stride_loops(dev):
    """(5, 1024, 1028), even: total4 = 1 315 840 quads on 3855 workgroups (affine_act_scale4, affine_drop_add4, bn_bwd_apply4_gap) and
    5 263 360 elements on 4096 (chscale_fwd, affine_act, sample_dropout, add)."""
    ops = Ops(dev)
    n, hw, c = R.BIG_SHAPE
    k = R.se_case("even", n, hw, c)
    assert R.border_ok(k.x, k.state["scale"], k.state["shift"])
    d = to_dev(k, dev)
    x, dy, skip, dpool, gate, st = d
    a_k = ops.affine_act(x, st, 2)
    y = ops.act_scale(x, st, 2, gate)
    R.bit_identical(y.cpu(), ops.chscale_fwd(a_k, gate).cpu(), "affine_act_scale against affine_act -> channel_scale_fwd")
    note({q + " big": v for q, v in R.check_affine_act_scale(k.x, k.state, 2, k.gate, y.cpu()).items()}, "even")
    y, f = ops.drop_add(x, st, R.DROP_RATE, 4330, None, skip)
    R.bit_identical(f.cpu(), R.drop_factor(n, c, R.DROP_RATE, 4330), "affine_drop_add factor")
    assert 0 < int((f[:, 0] == 0).sum()) < n                 # a dropped and a kept image
    chain = ops.add(ops.dropout(ops.affine_act(x, st, 0), hw * c, R.DROP_RATE, 4330), skip)
    R.bit_identical(y.cpu(), chain.cpu(), "affine_drop_add against affine_act -> sample_dropout -> add")
    note({q + " big": v for q, v in R.check_affine_drop_add(k.x, k.state, f.cpu(), k.skip, y.cpu()).items()}, "even")
    sums = ops.se_sums(dy, x, st, 0)
    o = ops.gap_sums(dy, dpool, gate, sums, x, st, 0)
    note({q + " big": v for q, v in R.check_gap_backward(k.dy, k.dpool, k.gate, k.x, k.state, 0, o, "gap sums").items()}, "even")


# ---- activations, |a - b|, drop-connect -------------------------------------------------------------------------------------------------------
def ew_inputs(total):
    g = torch.Generator().manual_seed(total)
    return {"even": torch.randn(total, generator=g), "logits30": R.logits30(total)}


def absdiff_inputs(total):
    g = torch.Generator().manual_seed(total + 5)
    a, b = torch.randn(total, generator=g), torch.randn(total, generator=g)
    b[::3] = a[::3]                                        # ties
    a[::6], b[::6] = 0.0, -0.0                             # +0 against -0
    a[1::12], b[1::12] = -0.0, -0.0
    return a, b, R.ST._gradient("even", g, (total,))


@pytest.mark.parametrize("total", R.EW_TOTALS)
def test_activations_absdiff_dropout(dev, total):
    lib, ops = _lib.lib(), Ops(dev)
    for name, v in ew_inputs(total).items():
        dyc = R.ST._gradient("even", torch.Generator().manual_seed(3), (total,))
        dyc[::5] = 0.0
        x, dy = v.to(dev), dyc.to(dev)
        for kind in (0, 1):
            y, dx = Guard((total,), dev), Guard((total,), dev)
            run([K + "act_fwd_kernel"], lib.embnet_activation_fwd, p(x), total, kind, y.ptr())
            run([K + "act_bwd_kernel"], lib.embnet_activation_bwd, p(x), p(dy), total, kind, dx.ptr())
            r = R.check_activation_fwd(v, kind, y.check("activation_fwd").cpu())
            r.update(R.check_activation_bwd(v, dyc, kind, dx.check("activation_bwd").cpu()))
            note(r, name)
    ac, bc, dyc = absdiff_inputs(total)
    a, b, dy = ac.to(dev), bc.to(dev), dyc.to(dev)
    y, da, db = Guard((total,), dev), Guard((total,), dev), Guard((total,), dev)
    run([K + "absdiff_fwd_kernel"], lib.embnet_absdiff_fwd, p(a), p(b), total, y.ptr())
    run([K + "absdiff_bwd_kernel"], lib.embnet_absdiff_bwd, p(a), p(b), p(dy), total, da.ptr(), db.ptr())
    note(R.check_absdiff(ac, bc, dyc, y.check("absdiff y").cpu(), da.check("absdiff da").cpu(), db.check("absdiff db").cpu()), "even")
    for per in R.DROP_PER_SAMPLE:
        y = ops.dropout(a, per, R.DROP_RATE, 77)
        R.bit_identical(y.cpu(), R.sample_dropout(ac, per, R.DROP_RATE, 77), "sample_dropout per_sample %d" % per)
        assert torch.equal(ops.dropout(a, per, R.DROP_RATE, 70, seed_word(7, dev)), y), "(70, seed_add_dev = 7) differs from (77, NULL)"
        R.bit_identical(ops.dropout(a, per, 0.0, 77).cpu(), ac, "sample_dropout: rate 0 is the identity")


# ---- the squeeze-and-excite MLP ----------------------------------------------------------------------------------------------------------------
def mlp_id(s):
    return "%d-%d-%d%s" % (s + ("" if R.se_mlp_supported(*s) else "-refused by embnet_se_mlp_supported",))


@pytest.mark.parametrize("shape", R.MLP_SHAPES, ids=mlp_id)
def test_se_mlp_per_element(dev, shape):
    lib = _lib.lib()
    n, c, S = shape
    assert bool(lib.embnet_se_mlp_supported(n, c, S)) == R.se_mlp_supported(n, c, S)
    if not R.se_mlp_supported(n, c, S):
        pytest.skip("refused by embnet_se_mlp_supported")
    for family in R.MLP_FAMILIES:
        case = R.mlp_case(family, n, c, S)
        pooled, w1, b1, w2, b2, dgate = (t.to(dev) for t in case)
        z1, gate = Guard((n, S), dev), Guard((n, c), dev)
        run([MLP_FWD], lib.embnet_se_mlp_fwd, p(pooled), p(w1), p(b1), p(w2), p(b2), n, c, S, z1.ptr(), gate.ptr())
        z1c, gc = z1.check("se_mlp_fwd z1").cpu(), gate.check("se_mlp_fwd gate").cpu()
        note(R.check_mlp_fwd(case, z1c, gc), family)
        g = {q: Guard(s, dev) for q, s in (("dz1", (n, S)), ("dpooled", (n, c)), ("dw1", (c, S)), ("db1", (S,)), ("dw2", (S, c)), ("db2", (c,)))}
        run([MLP_A, MLP_B], lib.embnet_se_mlp_bwd, p(dgate), gate.ptr(), z1.ptr(), p(pooled), p(w1), p(w2), n, c, S,
            *(g[q].ptr() for q in ("dz1", "dpooled", "dw1", "db1", "dw2", "db2")))
        note(R.check_mlp_bwd(case, gc, z1c, {q: v.check("se_mlp_bwd " + q).cpu() for q, v in g.items()}), family)


def test_se_mlp_supported_is_the_mirror(dev):
    lib = _lib.lib()
    for s in R.MLP_SHAPES + [(9, 640, 161), (2, 4100, 8), (2, 4096, 160), (2, 6, 2), (0, 8, 2)]:
        assert bool(lib.embnet_se_mlp_supported(*s)) == R.se_mlp_supported(*s), s


def test_zz_print_the_measured_tables():
    """Not an assertion of its own: prints what the tests above measured (pytest -s), for the docstring."""
    fams = R.MLP_FAMILIES + ["logits30"]
    print("\nlargest error / bound\n  %-28s" % "quantity" + "".join("%15s" % f for f in fams))
    for q in sorted({k[0] for k in RATIOS}):
        print("  %-28s" % q + "".join("%15s" % ("%.3f" % RATIOS[(q, f)] if (q, f) in RATIOS else "-") for f in fams))
