"""tests/se_ref.py on the CPU, for every family and shape tests/test_se_kernels_elementwise_gpu.py runs:

  (a) the FLOAT32 CPU evaluation of every formula (the kernels' arithmetic: one fma for z, fp32 products and sums — the pixel sums
      of the gate's gradient in chscale_bwd4_kernel's lane order, se_ref.lane_fma_sum — the sigmoids through exp where the bounds'
      E32 / kappa are measured through torch.sigmoid, so the stand-in is ANOTHER fp32 implementation, as the device is) stays inside
      every bound.  Printed (pytest -s) by the last test; these are the `cpu` column of the GPU file's docstring.  Largest error /
      bound over all families and shapes (act 0 / 1 / 2 where three figures stand):
        chscale y 1.00, dx 1.00, ds 0.95   act_scale y 0.98 / 0.98 / 0.26   drop_add y 0.97   sigmoid fwd 0.27, bwd 0.27   swish fwd
        0.25, bwd 0.26 (the same on inputs over +-30: 0.25)   T0 .84 .84 .23   S1 .61 .59 .27   S2 0 0 .24   S3 .68 .68 .32   S4 .52 .51 .29
        T0 - dgate .17 .12 .07   gap dbeta .35 .23 .25, dgamma .34 .34 .28, dx .59 .63 .63   finalize dbeta 0.70, dgamma 0.72
        mlp z1 0.15, gate 0.33, dz1 0.16, dpooled 0.97, dW1 0.94, db1 0.54, dW2 0.50, db2 0.63
      (1.00, printed for 0.999..: one rounding against u |value|);
  (b) the condition of the bounds: the ReLU-borderline cap (at most 0.1 % of a channel, none in an (image, channel) group of fewer
      than 1000 pixels) holds for every family and shape at the seed se_case settled on;
  (c) the table: every listed shape reaches the branch it is listed for, by the geometry mirrors (pix_geom, ew_blocks_c4,
      quad_groups, jp_of, nn_ref.col_geom);
  (d) ew_blocks_c4 returns a grid whose stride is a multiple of c4 for EVERY (total4, c4): the `!fixed` path of
      affine_act_scale4_kernel / affine_drop_add4_kernel cannot be reached through the host wrappers;
  (e) the guard: test_the_old_metric_is_blind_to_a_quiet_image_channel — a gate wrong by 2x in the quietest (image, channel) is
      2.5e-7 of max|ref|, the quiet image's S1 row counted twice 8.2e-8: 1e-5 of max|ref| passes both, the per-(image, channel)
      checks fail both.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import se_ref as R  # noqa: E402
from nn_ref import col_geom  # noqa: E402

F32 = torch.float32
RATIOS = {}
GUARD = {}


def note(r):
    for k, v in r.items():
        assert v <= 1.0, (k, v)
        RATIOS[k] = max(RATIOS.get(k, 0.0), v)


# ---- (a), (b): the per-(image, channel) kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,c", R.QUAD_SHAPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_float32_per_image_channel_formulas_stay_inside_every_bound(family, n, hw, c):
    k = R.se_case(family, n, hw, c)
    st = k.state
    assert R.border_ok(k.x, st["scale"], st["shift"]), "the ReLU-borderline cap"
    x, dy, g = k.x, k.dy, k.gate
    note(R.check_channel_scale_fwd(x, g, x * g.unsqueeze(1)))
    note(R.check_channel_scale_bwd(x, g, dy, dy * g.unsqueeze(1), R.lane_fma_sum(dy, x)))
    f = R.drop_factor(n, c, R.DROP_RATE, 1234 + n)
    for factor in (f, torch.ones(n, c)):
        note(R.check_affine_drop_add(x, st, factor, k.skip, R.affine_drop_add(x, st, factor, k.skip, F32)))
    for act in (0, 1, 2):
        note(R.check_affine_act_scale(x, st, act, g, R.affine_act_scale(x, st, act, g, F32)))
        sums = R.se_sums(dy, x, st, act, F32)
        note(R.check_se_sums(dy, x, st, act, sums))
        a_k = R.act_fwd(R.N.affine(x, st["scale"], st["shift"], F32), act, exp_form=True)
        note(R.check_t0_vs_dgate(dy, x, st, act, sums, a_k, R.lane_fma_sum(dy, a_k)))
        outs = {}
        for key, gate, dpool in (("gap", None, k.dpool), ("gap gated", g, k.dpool), ("gap drop", f, torch.zeros(n, c))):
            outs[key] = R.gap_backward(dy, dpool, gate, x, st, act, F32)
            note(R.check_gap_backward(dy, dpool, gate, x, st, act, outs[key], key))
        # the sums form: dbeta / dgamma combined in double from the float32 sums, as se_bn_finalize_kernel does
        s64, q = sums.double(), (k.dpool * torch.tensor(1.0 / hw)).double()
        own = dict(dbeta=(g.double() * s64[:, 1] + q * s64[:, 2]).sum(0).float(), dgamma=(g.double() * s64[:, 3] + q * s64[:, 4]).sum(0).float())
        note(R.check_gap_finalize(sums, g, k.dpool, hw, own["dbeta"], own["dgamma"]))
        own["dx"] = outs["gap gated"]["dx"]
        note(R.check_gap_agree(dy, k.dpool, g, x, st, act, outs["gap gated"], own))


@pytest.mark.parametrize("n,hw,c", R.SCALAR_SHAPES)
def test_float32_scalar_channel_scale(n, hw, c):
    for family in R.FAMILIES:
        k = R.se_case(family, n, hw, c)
        note(R.check_channel_scale_fwd(k.x, k.gate, k.x * k.gate.unsqueeze(1)))
        note(R.check_channel_scale_bwd(k.x, k.gate, k.dy, k.dy * k.gate.unsqueeze(1), R.lane_fma_sum(k.dy, k.x, lanes=1)))


def test_float32_big_case_meets_the_border_cap_and_the_elementwise_bounds():
    n, hw, c = R.BIG_SHAPE
    k = R.se_case("even", n, hw, c)
    assert R.border_ok(k.x, k.state["scale"], k.state["shift"])
    note(R.check_affine_act_scale(k.x, k.state, 2, k.gate, R.affine_act_scale(k.x, k.state, 2, k.gate, F32)))


# ---- activations, |a - b|, drop-connect -------------------------------------------------------------------------------------------------------
def ew_inputs(total):
    g = torch.Generator().manual_seed(total)
    return {"even": torch.randn(total, generator=g), "logits30": R.logits30(total)}


@pytest.mark.parametrize("total", R.EW_TOTALS)
def test_float32_activations_absdiff_dropout(total):
    for name, v in ew_inputs(total).items():
        dy = R.ST._gradient("even", torch.Generator().manual_seed(3), (total,))
        dy[::5] = 0.0
        for kind in (0, 1):
            r = R.check_activation_fwd(v, kind, R.act_kind(v, kind, F32, exp_form=True))
            r.update(R.check_activation_bwd(v, dy, kind, dy * R.act_kind_der(v, kind, F32, exp_form=True)))
            note({"%s (%s)" % (q, name): val for q, val in r.items()})
    a, b, dy = absdiff_inputs(total)
    note(R.check_absdiff(a, b, dy, *R.absdiff(a, b, dy)))
    for per in R.DROP_PER_SAMPLE:
        y = R.sample_dropout(a, per, R.DROP_RATE, 77)
        assert bool(((y == 0) | (y == a * float(R.keep_scale(R.DROP_RATE)))).all())
        R.bit_identical(R.sample_dropout(a, per, 0.0, 77), a, "rate 0 is the identity")


def absdiff_inputs(total):
    g = torch.Generator().manual_seed(total + 5)
    a, b = torch.randn(total, generator=g), torch.randn(total, generator=g)
    b[::3] = a[::3]                                        # ties
    a[::6], b[::6] = 0.0, -0.0                             # +0 against -0
    a[1::12], b[1::12] = -0.0, -0.0
    return a, b, R.ST._gradient("even", g, (total,))


def test_drop_mask_and_factor_follow_the_rng_of_augment_ref():
    keep = R.drop_keep(4096, R.DROP_RATE, 99)
    assert abs(float(keep.mean()) - (1 - R.DROP_RATE)) < 0.03
    assert bool(R.drop_keep(64, 0.0, 5).all())
    assert float(R.keep_scale(R.DROP_RATE)) == float(np.float32(1) / np.float32(np.float32(1) - np.float32(0.2)))
    f = R.drop_factor(64, 8, R.DROP_RATE, 99)
    assert set(f.unique().tolist()) == {0.0, float(R.keep_scale(R.DROP_RATE))}


# ---- the squeeze-and-excite MLP ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c,S", R.MLP_SHAPES)
def test_float32_se_mlp_stays_inside_every_bound(n, c, S):
    assert R.se_mlp_supported(n, c, S)
    for family in R.MLP_FAMILIES:
        case = R.mlp_case(family, n, c, S)
        z1, gate = R.mlp_forward(case, F32)
        note(R.check_mlp_fwd(case, z1, gate))
        if family == "saturated":
            a = R.mlp_logits(case, z1)
            assert float(a.min()) < -25 and float(a.max()) > 25 or c < 8
        note(R.check_mlp_bwd(case, gate, z1, R.mlp_backward(case, gate, z1, F32)))


# ---- (c): the shape tables --------------------------------------------------------------------------------------------------------------------
def test_every_listed_shape_reaches_the_branch_it_is_listed_for():
    pg = {s: R.pix_geom(s[0], s[1], s[2] // 4) for s in R.QUAD_SHAPES}
    paths = {s: R.pix_paths(s[0], s[1], s[2] // 4) for s in R.QUAD_SHAPES}
    assert [pg[s].cls for s in ((2, 1, 4), (1, 257, 8), (3, 9, 12), (2, 33, 32))] == [1, 2, 4, 8]           # cls 1, 2, 4, 8 (c = 4, 8, 12, 32)
    assert pg[(2, 196, 80)][:2] == (16, 2) and 80 // 4 % 16 == 4                                          # a ragged second channel block
    assert pg[(3, 9, 12)].lanes > 9 and pg[(2, 1, 64)].lanes > 1                                          # hw < pixel lanes; hw = 1
    assert paths[(2, 33, 32)] == (True, True) and paths[(2, 196, 80)] == (True, True)                     # the two-pixel loop and its tail
    assert paths[(2, 1, 64)] == (False, True)
    # the 1024-thread form: (1, 257, 8) and (4, 625, 4) have fewer pixels than its 512 / 1024 pixel lanes and reach the tail alone;
    # nn_ref.GAP_CASES' (1, 1025, 8) and (1, 2051, 8) run the two-pixel loop there, at cls = 2 < 16
    for s in ((1, 257, 8), (4, 625, 4), (1, 1025, 8), (1, 2051, 8)):
        assert pg[s].threads == 1024
    assert paths[(1, 257, 8)] == (False, True) and paths[(4, 625, 4)] == (False, True)
    assert paths[(1, 1025, 8)] == (True, True) and paths[(1, 2051, 8)] == (True, True) and pg[(1, 2051, 8)].cls == 2
    assert all(pg[s].threads == 256 for s in R.QUAD_SHAPES if s[1] < 256)
    assert {s[0] > 64 for s in R.QUAD_SHAPES} == {True, False} and (70, 4, 16) in pg and (65, 3, 68) in pg  # se_bn_finalize: lanes stride the images
    assert {s[2] // 4 for s in R.QUAD_SHAPES} >= {16, 17}                                                  # chscale_bwd4_kernel across c4 = 16 / 17
    assert any(c % 4 and c > 256 for _, _, c in R.SCALAR_SHAPES) and any(c % 4 and c < 256 for _, _, c in R.SCALAR_SHAPES)   # chscale_bwd_kernel: 2 column blocks
    # grid-stride kernels: ew_blocks_c4 with b < unit (c4 = 257 on a small tensor: 38 blocks of work, 257 launched), and a second trip
    n, hw, c = (1, 37, 1028)
    assert R.ew_blocks(n * hw * c // 4) == 38 and R.ew_blocks_c4(n * hw * c // 4, c // 4) == 257
    n, hw, c = R.BIG_SHAPE
    t4 = n * hw * c // 4
    assert t4 > R.EW_CAP * 256 and R.ew_blocks_c4(t4, c // 4) * 256 < t4 and R.ew_blocks(n * hw * c) * 256 < n * hw * c
    # ew_blocks_c4 rounds DOWN to a multiple of unit = c4 / gcd(c4, 256), so small tensors with unit > 1 take a second trip as well:
    # (3, 99, 48) has 14 blocks of work on 12 (unit 3), (2, 196, 68) 27 on 17; the shapes with unit = 1 take one trip
    two = {s for s in R.QUAD_SHAPES if R.ew_blocks_c4(s[0] * s[1] * s[2] // 4, s[2] // 4) * 256 < s[0] * s[1] * s[2] // 4}
    assert (3, 99, 48) in two and R.ew_blocks_c4(3 * 99 * 12, 12) == 12 and R.ew_blocks(3 * 99 * 12) == 14
    assert all(256 % (s[2] // 4) for s in two) and (3, 99, 256) not in two and (4, 625, 4) not in two
    assert R.EW_TOTALS[-1] > R.EW_CAP * 256 and all(t <= R.EW_CAP * 256 for t in R.EW_TOTALS[:-1])
    assert all(256 % p or p == 1 for p in R.DROP_PER_SAMPLE) and 1 in R.DROP_PER_SAMPLE
    # bn_bwd_reduce4_gap_kernel's column reduction (nn_ref.col_geom on the quads): one butterfly, the LDS branch, a second column trip
    geoms = {s: col_geom(s[0] * s[1], s[2] // 4) for s in R.QUAD_SHAPES}
    assert geoms[(4, 625, 4)].cl == 1 and geoms[(3, 99, 256)].cl == 64 and geoms[(1, 37, 1028)].cl == 256 and 1028 // 4 > 256
    assert any(g.blocks > 1 and s[0] * s[1] % g.rows_per_block for s, g in geoms.items())
    # se_mlp.hip
    mp = {s: R.mlp_paths(*s) for s in R.MLP_SHAPES}
    assert all(R.se_mlp_supported(*s) for s in R.MLP_SHAPES)                                               # none is skipped
    assert [mp[s]["umax"] for s in ((7, 240, 48), (7, 240, 49))] == [3, 10]                                # the template switch at 48 / 49
    assert [mp[s]["jp"] for s in ((3, 64, 64), (3, 64, 65))] == [64, 128]                                  # jp_of at 64 / 65
    assert (9, 640, 160) in mp and not R.se_mlp_supported(9, 640, 161)                                     # the upper limit of S
    assert mp[(1, 4, 1)]["odd_n"] and mp[(3, 20, 1)]["odd_n"] and not mp[(2, 40, 10)]["odd_n"]             # n = 1, odd n: half a workgroup
    assert [mp[s]["tiles"] for s in ((64, 96, 17), (65, 96, 16), (130, 36, 9))] == [1, 2, 3]               # NT = 64
    assert all(mp[s]["ragged_c"] for s in ((3, 20, 1), (2, 40, 10), (5, 56, 14), (3, 1028, 17), (130, 36, 9)))   # c % 16 != 0
    assert mp[(2, 4096, 8)]["G"] == 1 and mp[(1, 4, 1)]["G"] == 1 and mp[(7, 240, 48)]["G"] == 17 and mp[(3, 1028, 17)]["G"] == 3
    assert mp[(3, 1028, 17)]["w1_chunks"] == 2 and mp[(9, 640, 160)]["w1_chunks"] > 2 and mp[(7, 240, 48)]["w1_chunks"] == 1


# ---- (d): the `!fixed` path --------------------------------------------------------------------------------------------------------------------
def test_ew_blocks_c4_always_gives_a_stride_that_is_a_multiple_of_c4():
    """b is a multiple of unit = c4 / gcd(c4, 256), so b * 256 = k unit 256 = k c4 (256 / gcd): `fixed` is always true."""
    for c4 in list(range(1, 1100)) + [2048, 4097, 65535]:
        for total4 in (1, c4, 255 * c4 + 1, 4096 * 256, 4096 * 256 + c4, 10 ** 8):
            assert R.ew_blocks_c4(total4, c4) * 256 % c4 == 0 and R.ew_blocks_c4(total4, c4) >= 1


# ---- (e): the guard ----------------------------------------------------------------------------------------------------------------------------
def test_the_old_metric_is_blind_to_a_quiet_image_channel():
    """(3, 99, 48).  (1) spread17: act(BN(x)) * gate with the gate of the quietest (image, channel) wrong by 2x; (2) quiet_image17:
    the [n][5][c] sums with the quiet image's S1 row counted twice.  1e-5 of max|ref| over the whole tensor passes both, the
    per-(image, channel) checks fail both."""
    n, hw, c = 3, 99, 48
    k = R.se_case("spread17", n, hw, c)
    ref = R.affine_act_scale(k.x, k.state, 2, k.gate)
    level = ref.abs().amax(1)
    i, j = divmod(int(torch.argmin(torch.where(level > 0, level, torch.full_like(level, 1e30)))), c)
    bad_gate = k.gate.clone()
    bad_gate[i, j] *= 2.0
    wrong = R.affine_act_scale(k.x, k.state, 2, bad_gate, F32)
    GUARD["gate x2: error / max|ref|"] = float((wrong.double() - ref).abs().max() / ref.abs().max())
    GUARD["gate x2: error / own level"] = float((wrong.double() - ref)[i, :, j].abs().max() / level[i, j])
    assert R.old_close(wrong, ref)
    with pytest.raises(AssertionError):
        R.check_affine_act_scale(k.x, k.state, 2, k.gate, wrong)
    k = R.se_case("quiet_image17", n, hw, c)
    sums = R.se_sums(k.dy, k.x, k.state, 2)
    twice = R.se_sums(k.dy, k.x, k.state, 2, F32)
    twice[-1, 1] *= 2.0                                    # the quiet image's S1 row, all channels
    GUARD["row twice: error / max|ref|"] = float((twice.double() - sums).abs().max() / sums.abs().max())
    assert R.old_close(twice, sums)
    with pytest.raises(AssertionError):
        R.check_se_sums(k.dy, k.x, k.state, 2, twice)
    R.check_se_sums(k.dy, k.x, k.state, 2, R.se_sums(k.dy, k.x, k.state, 2, F32))


def test_zz_print_the_float32_ratios():
    """Not an assertion of its own: the `cpu` column of the GPU file's docstring (pytest -s)."""
    print("\nfloat32 CPU evaluation, largest error / bound")
    for q in sorted(RATIOS):
        print("  %-40s %.3f" % (q, RATIOS[q]))
    for q, v in GUARD.items():
        print("  guard  %-32s %.3e" % (q, v))
