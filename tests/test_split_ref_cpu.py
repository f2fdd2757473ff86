"""The NumPy restatement of the two-piece fp16 format (tests/split_ref.py) against hand-computed vectors, and the FORMAT against the
truth: for every input family of tests/test_three_product_elementwise_gpu.py the three kept products of the split operands differ
from the float64 convolution of the fp32 operands by no more than include/embnet.h's PRECISION paragraph allows, element by
element.  No kernel runs here; a failure of the second part means the header is wrong.

format_envelope() is the table of DESIGN.md 3.14 (9): the largest |model - float64| / sum|a||b| per bin of depth — how many binades
the operand elements behind an output element lie below their tensor's bound (split_ref.depth: the weighted mean over the
element's own products, the deeper operand) — beside a float32 CPU convolution's.  Measured (pytest -s prints it), all families,
passes and bound loosenesses 1x / 8x / 64x together; |model - float64| reached 0.86 of the header's bound at most:

  binades below the bound | three products | float32 CPU convolution
    0 ..   4              | 2.4e-07 | 3.8e-07
    4 ..   8              | 3.4e-07 | 6.9e-07
    8 ..  12              | 3.4e-07 | 8.1e-07
   12 ..  16              | 3.1e-07 | 3.5e-07
   16 ..  20              | 1.1e-06 | 2.5e-07
   20 ..  24              | 1.8e-05 | 3.2e-07
   24 ..  28              | 1.9e-04 | 6.2e-07
   28 ..  32              | 5.2e-04 | 2.0e-07

i.e. fp32-class down to 2^16 below the bound, then 2^(depth - 39): the subnormal floor of h2, 2^-39 of the bound, absolute.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as SR  # noqa: E402


# ---- the scale ---------------------------------------------------------------------------------------------------------------------
SCALE_VECTORS = [  # bound, exponent of s
    (0.0, 0), (-0.0, 0), (float("inf"), 0), (float("nan"), 0),
    (1e-40, 126),                                        # an fp32 subnormal: 15 + 133 clamps to 126
    (2.0 ** -149, 126), (2.0 ** -120, 126), (2.0 ** -112, 126), (2.0 ** -111, 125),
    (1.0, 14), (2.0, 13), (0.5, 15), (2.0 ** 14, 0), (2.0 ** 15, -1),
    (float(np.nextafter(np.float32(1), np.float32(0))), 15), (float(np.nextafter(np.float32(1), np.float32(2))), 14),
    (0.99999999, 14),                                    # rounds to 1.0f: the slot holds a float
    (1.7, 14), (1e-4, 28), (3e4, 0), (1e5, -2),
    (65504.0, -1), (3e38, -113), (float(np.finfo(np.float32).max), -113), (-3.0, 13),
]


@pytest.mark.parametrize("bound,k", SCALE_VECTORS)
def test_scale_hand_vectors(bound, k):
    assert SR.scale_exponent(bound) == k
    assert SR.scale_of(bound) == 2.0 ** k


def test_scale_puts_the_bound_into_its_binade():
    rs = np.random.RandomState(1)
    for b in np.concatenate([10.0 ** rs.uniform(-30, 38, 2000), 2.0 ** np.arange(-100, 120)]).astype(np.float32):
        s = SR.scale_of(b)
        assert 2.0 ** 14 <= float(b) * s < 2.0 ** 15, (b, s)
        assert np.float32(s) * np.float32(1.0 / s) == 1.0 and np.isfinite(np.float32(1.0 / s))


# ---- the split ---------------------------------------------------------------------------------------------------------------------
def bits(h):
    return int(np.asarray(h, dtype=np.float16).view(np.uint16))


S14 = 2.0 ** 14
SPLIT_VECTORS = [  # x, s, h1 (value, bits), h2 (value, bits)
    # normal h2: x s = 2^14 + 4, fp16's step at 2^14 is 16
    (1.0 + 2.0 ** -12, S14, 16384.0, 0x7400, 4.0, 0x4400),
    # x = 0.3f = 0.300000011920928955078125: x s = 4915.2001953125, step 4 -> 4916, rest -1638 / 2048
    (0.3, S14, 4916.0, 0x6CCD, -0.7998046875, 0xBA66),
    # subnormal h2: x s = 2^-6 + 3.25 x 2^-24 -> h1 = 2^-6 (step 2^-16), h2 = 3 x 2^-24
    (2.0 ** -20 + 3 * 2.0 ** -38 + 2.0 ** -40, S14, 2.0 ** -6, 0x2400, 3 * 2.0 ** -24, 0x0003),
    # ... a tie goes to the even subnormal: 2.5 x 2^-24 -> 2 x 2^-24
    (2.0 ** -20 + 2.0 ** -37 + 2.0 ** -39, S14, 2.0 ** -6, 0x2400, 2 * 2.0 ** -24, 0x0002),
    # h1 itself subnormal: x s = 5.25 x 2^-24 -> h1 = 5 x 2^-24, the rest (2^-26) is below half a step: h2 = 0
    (5.25 * 2.0 ** -38, S14, 5 * 2.0 ** -24, 0x0005, 0.0, 0x0000),
    # ... 5.5 x 2^-24 ties to the even 6 x 2^-24; the rest -2^-25 ties to (minus) zero
    (5.5 * 2.0 ** -38, S14, 6 * 2.0 ** -24, 0x0006, -0.0, 0x8000),
    # the top of the range: a bound of 1 - 2^-24 takes s = 2^15 and lands one fp16 step below 2^15 after rounding UP to 32768
    (1.0 - 2.0 ** -24, 2.0 ** 15, 32768.0, 0x7800, -2.0 ** -9, 0x9800),
    # a negative value that is an fp16 after scaling: the rest is +0
    (-3.0, 2.0 ** 13, -24576.0, 0xF600, 0.0, 0x0000),
    # a scale below one (bound 1e5 -> s = 2^-2): 99999 s = 24999.75 -> 25008 | 24992 (step 16): 24992 is nearer, rest 7.75
    (99999.0, 2.0 ** -2, 24992.0, 0x761A, 7.75, 0x47C0),
    (0.0, S14, 0.0, 0x0000, 0.0, 0x0000),
]


@pytest.mark.parametrize("x,s,h1,b1,h2,b2", SPLIT_VECTORS)
def test_split_hand_vectors(x, s, h1, b1, h2, b2):
    g1, g2 = SR.split(np.float32(x), s)
    assert float(g1) == h1 and float(g2) == h2, (float(g1), float(g2))
    assert bits(g1) == b1 and bits(g2) == b2, (hex(bits(g1)), hex(bits(g2)))


def test_split_keeps_what_precision_states():
    """|x - (h1 + h2) / s| <= max(2^-22 |x|, 2^-25 / s) for every element, at any amplitude below the bound."""
    rs = np.random.RandomState(3)
    for bound in (1.0, 1e-4, 3e4, 7.3):
        x = (rs.uniform(-1, 1, 200000) * bound * 2.0 ** -rs.uniform(0, 40, 200000)).astype(np.float32)
        s = SR.scale_of(bound)
        h1, h2 = SR.split(x, s)
        back = (h1.astype(np.float64) + h2.astype(np.float64)) / s
        assert (np.abs(back - x.astype(np.float64)) <= SR.operand_error(x, s)).all()
        assert np.isfinite(h1).all()


# ---- the format against the truth ------------------------------------------------------------------------------------------------------
SMALL = dict(n=2, h=8, w=8, c=32, k=32, ks=3, stride=1, pad=1)      # one small geometry; the three passes
SMALL_S2 = dict(n=2, h=9, w=9, c=16, k=16, ks=3, stride=2, pad=1)


def _bound_of(t, loose=1.0):
    return float(np.float32(np.abs(t).max()) * np.float32(loose))


def _case(family, kind, loose, geo):
    x, kern, dy = SR.operands(family, seed=7, **geo)
    a, b, out_shape = SR.pass_operands(kind, x, kern, dy)
    geom = SR.Geometry(kind, geo["stride"], geo["pad"], out_shape)
    ba = _bound_of(a, loose if a is x else 1.0)
    bb = _bound_of(b)
    return a, b, geom, ba, bb


def format_envelope(verbose=True):
    """Runs every family x pass x looseness on the small geometries, asserts the header's bound per element and returns
    {"three products": {bin: max |model - float64| / mag}, "float32 CPU convolution": {bin: ...}, "share of bound": float}."""
    env3, env32, share = {}, {}, 0.0
    for geo in (SMALL, SMALL_S2):
        for family in SR.FAMILIES:
            for kind in ("fwd", "dgrad", "wgrad"):
                for loose in (SR.LOOSE if kind != "dgrad" else [1.0]):
                    a, b, geom, ba, bb = _case(family, kind, loose, geo)
                    sa, sb = SR.scale_of(ba), SR.scale_of(bb)
                    truth = SR.conv(a, b, geom)
                    model = SR.model_conv(SR.split(a, sa), SR.split(b, sb), sa, sb, geom)
                    allowed = SR.format_bound(a, b, sa, sb, geom)
                    err = np.abs(model - truth)
                    # (the float64 sums themselves: 2^-50 of sum |a||b|)
                    m = SR.mag(a, b, geom)
                    bad = err > allowed + m * 2.0 ** -50
                    assert not bad.any(), (family, kind, loose, float((err / np.maximum(allowed, 1e-300)).max()))
                    assert (model[m == 0] == 0).all()
                    if (allowed > 0).any():
                        share = max(share, float((err[allowed > 0] / allowed[allowed > 0]).max()))
                    dep = SR.depth(a, b, ba, bb, geom, m)
                    SR.envelope(err, m, dep, env3)
                    SR.envelope(np.abs(SR.conv(a, b, geom, dtype=__import__("torch").float32) - truth), m, dep, env32)
    out = {"three products": env3, "float32 CPU convolution": env32, "share of bound": share}
    if verbose:
        print()
        print(SR.format_envelope_rows({k: v for k, v in out.items() if isinstance(v, dict)}))
        print("largest |model - float64| / format_bound: %.2f" % share)
    return out


def test_format_stays_inside_the_headers_bound_for_every_family():
    env = format_envelope()
    e3, e32 = env["three products"], env["float32 CPU convolution"]
    assert 0 < env["share of bound"] <= 1.0
    assert all(np.isfinite(v) for v in e3.values()) and all(np.isfinite(v) for v in e32.values())
    # the control: elements within 2^16 of their tensor's bound are fp32-class — no worse than twice the float32 convolution's
    # worst (all bins), the criterion of tests/test_backbone_gpu.py::test_conv2d_products_are_fp32_accurate
    worst32 = max(e32.values())
    for b in range(0, 16 // SR.BIN):
        if b in e3:
            assert e3[b] <= max(2 * worst32, 5e-7), (b, e3[b], worst32)


def test_a_wrong_model_is_not_the_model():
    """model_conv's sabotage switches: a dropped term is 2^-11 of every element; subnormal h2 flushed to zero changes the quiet
    elements by far more than fp32 rounding and nothing a per-tensor metric sees."""
    a, b, geom, ba, bb = _case("quiet_image20", "fwd", 64.0, SMALL)
    sa, sb = SR.scale_of(ba), SR.scale_of(bb)
    pa, pb = SR.split(a, sa), SR.split(b, sb)
    good = SR.model_conv(pa, pb, sa, sb, geom)
    m = SR.mag(a, b, geom)

    def both(wrong):
        return np.abs(wrong - good).max() / np.abs(good).max(), (np.abs(wrong - good)[m > 0] / m[m > 0]).max()

    per_tensor, per_element = both(SR.model_conv(pa, pb, sa, sb, geom, terms=(True, True, False)))
    assert per_element > 1e-5, per_element
    per_tensor, per_element = both(SR.model_conv(pa, pb, sa, sb, geom, flush_h2=True))
    assert per_tensor < 1.5e-6 and per_element > 1e-5, (per_tensor, per_element)
