"""tests/nn_ref.py on the CPU, for every family, shape and geometry tests/test_nn_kernels_elementwise_gpu.py runs:

  (a) the FLOAT32 CPU evaluation of every formula (the kernel's arithmetic: fp32 sums, the finalize in double; the swish through
      exp where the bounds' E32 is measured through torch.sigmoid, so the stand-in is ANOTHER fp32 implementation, as the device
      is) stays inside every bound, ratio < 1 — the bounds are not too tight for a correct fp32 implementation.  Printed (pytest -s);
      largest error / bound over all families, shapes, both eps:
        mean 0.090   rstd 0.57   moving_mean 0.90   moving_var 0.90   scale 0.99   shift 0.86   y 1.00 / 1.00 / 0.26 (act 0 / 1 / 2)
        dbeta 0.11 / 0.10 / 0.22   dgamma 0.12 / 0.12 / 0.11   dx 0.55 / 0.64 / 0.55   frozen dx 1.00 / 1.00 / 0.53   dx + add 0.98
        in-ReLU dz 0.50 / 0.53 / 0.55, dbias 0.12   inference scale 0.61, shift 0.80, y as above
        pool dx 1.00, dbias 0.35   fused dx 0.56 / 0.53 / 0.62, frozen 0.99 / 1.00 / 0.31
        GAP forward 0.056, backward 0.49, + add 1.00, affine_act_gap mean 0.09 (y given), 0.30 (y NULL)
      (1.00, printed for 0.999..: one rounding to nearest against u |value| — the bound of a single operation cannot be missed and
      leaves no slack; the larger dx figures are m = 1, where dz - dbeta / m cancels and only the last roundings remain);
  (b) the conditions of the bounds: Ev <= (var + eps) / 4 (largest Ev / (var + eps): 0.080 — offset8's loudest channel sits at
      amplitude 1/4, which keeps the m = 1 case at eps = 2e-5 inside) and at most 0.1 % ReLU-borderline elements per channel;
  (c) the max-pool rule equals oracle.backbones.maxpool's (F.pad + max_pool2d + autograd): y and dx on the same inputs;
  (d) the col_geom mirror against a hand-worked table;
  (e) the guard: spread17 at (297, 48), a reference whose quietest channel's mean is off by 1 % of that channel's std passes the
      neighbouring tests' metric and fails the per-channel bound.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref as N  # noqa: E402
from oracle import backbones as OB  # noqa: E402

RATIOS = {}


def note(r):
    for k, v in r.items():
        assert v < 1.0, (k, v)
        RATIOS[k] = max(RATIOS.get(k, 0.0), v)


@pytest.mark.parametrize("m,c", N.BN_SHAPES)
@pytest.mark.parametrize("family", N.BN_FAMILIES)
def test_float32_batchnorm_stays_inside_every_bound(family, m, c):
    case = N.bn_case(family, m, c)
    for eps in N.EPS_VALUES:
        eps = N.f32(eps)
        st = N.bn_stats(case.x, eps)
        assert bool(st.ok.all()), "Ev <= (var + eps) / 4"
        RATIOS["Ev / (var + eps)"] = max(RATIOS.get("Ev / (var + eps)", 0.0), float((st.Ev / (st.var + eps)).max()))
        for act in (0, 1, 2):
            out = N.bn_forward(case, eps, act, dtype=N.F32)
            note(N.check_bn_forward(case, eps, act, out))
            note(N.check_bn_infer(case, eps, act, N.bn_infer(case, eps, act, dtype=N.F32)))
            for training in (1, 0):
                note(N.check_bn_backward(case, out, act, training, N.bn_backward(case.x, case.dy, out, act, training, dtype=N.F32)))
                if c % 4 == 0:
                    note(N.check_bn_backward(case, out, act, training, N.bn_backward(case.x, case.dy, out, act, training, inrelu=True, dtype=N.F32),
                                             inrelu=True))
            if (m, c) == (297, 48):
                add = torch.randn(m, c, generator=torch.Generator().manual_seed(5)) * 1e-3
                note(N.check_bn_backward(case, out, act, 1, N.bn_backward(case.x, case.dy, out, act, 1, dx_add=add, dtype=N.F32), dx_add=add))
        if (m, c) == (297, 48):                           # statistics from by-channel partials: 8 and 7 row bands
            for rows in (8, 7):
                note(N.check_bn_forward(case, eps, 0, N.bn_forward(case, eps, 0, dtype=N.F32, stats_rows=rows)))


def _dy(g, shape):
    return N.ST._gradient("even", g, shape)


@pytest.mark.parametrize("k,stride,pad,h,w", N.POOL_GEOMS)
def test_maxpool_rule_is_the_oracles_and_float32_stays_inside(k, stride, pad, h, w):
    for c in N.POOL_CHANNELS:
        for kind in N.POOL_INPUTS:
            x, g = N.pool_input(kind, N.POOL_N, h, w, c)
            y, am = N.maxpool_fwd(x, k, stride, pad)
            dy = _dy(g, tuple(y.shape))
            dx, mag, cnt = N.maxpool_route(dy, am, tuple(x.shape), k, stride, pad)
            xo = x.double().requires_grad_(True)
            yo = OB.maxpool(xo, k, stride, zero_pad=pad)
            yo.backward(dy.double())
            assert torch.equal(yo.detach(), y.double()), (kind, c)
            assert torch.equal(xo.grad, dx), (kind, c)
            if kind == "negative":                         # padding zeros win exactly where a window touches the padding
                assert bool(((am == 255) == (y == 0)).all()) and bool((am == 255).any()) == (pad > 0)
            r, wmax = N.check_maxpool(x, dy, k, stride, pad, y, am, dx.float())
            note(r)
            assert wmax <= (-(-k // stride)) ** 2
            if c % 4 == 0:
                note(N.check_relu_colsum(x, dx.float(), torch.where(x > 0, dx.float(), torch.zeros(1)),
                                         torch.where(x > 0, dx.float(), torch.zeros(1)).reshape(-1, c).sum(0)))
    if (k, stride, pad, h, w) == (2, 2, 0, 13, 11):
        assert bool((cnt[:, 12] == 0).all()) and bool((cnt[:, :, 10] == 0).all())      # the uncovered last row and column
    if (k, stride, pad, h, w) == (3, 1, 1, 7, 9):
        assert wmax > 4                                    # more windows per pixel than the fast path's four candidates


@pytest.mark.parametrize("k,stride,pad,h,w", N.FUSED_GEOMS)
@pytest.mark.parametrize("family", N.BN_FAMILIES)
def test_float32_fused_stem_stays_inside_every_bound(family, k, stride, pad, h, w):
    n, eps = N.POOL_N, N.f32(1e-3)
    for c in N.FUSED_CHANNELS:
        case = N.bn_case(family, n * h * w, c, seed=1)
        x = case.x.reshape(n, h, w, c)
        for act in (0, 1, 2):
            st = N.bn_forward(case, eps, act, dtype=N.F32)
            y, am, xwin = N.fused_forward(x, st["scale"], st["shift"], act, k, stride, pad, dtype=N.F32)
            y2, am2 = N.maxpool_fwd(st["y"].reshape(n, h, w, c), k, stride, pad)
            assert torch.equal(y, y2) and torch.equal(am, am2)
            dy = _dy(torch.Generator().manual_seed(c + act), tuple(y.shape))
            for training in (1, 0):
                note(N.check_fused_backward(x, dy, am, st, act, training, k, stride, pad,
                                            N.fused_backward(x, dy, am, st, act, training, k, stride, pad, dtype=N.F32)))


@pytest.mark.parametrize("n,hw,c", N.GAP_CASES)
def test_float32_gap_stays_inside_every_bound(n, hw, c):
    for family in N.BN_FAMILIES:
        case = N.bn_case(family, n * hw, c, seed=2)
        x = case.x.reshape(n, hw, c)
        note(N.check_gap_forward(x, N.gap_forward(x, N.F32)))
        dy, add = case.dy[:n], case.dy.reshape(n, hw, c)
        note(N.check_gap_backward(dy, hw, N.gap_backward(dy, hw, dtype=N.F32)))
        note(N.check_gap_backward(dy, hw, N.gap_backward(dy, hw, add, dtype=N.F32), add))
        for act in (0, 1, 2):
            y = N.act_fwd(N.affine(x, case.gamma, case.beta, N.F32), act, exp_form=True)
            note(N.check_affine_act_gap(x, case.gamma, case.beta, act, y, y.mean(1)))
            note(N.check_affine_act_gap(x, case.gamma, case.beta, act, None, y.mean(1)))


def test_col_geom_mirror_against_a_hand_worked_table():
    """cl = the power of two >= columns (<= 256), rl = 256 / cl, blocks = ceil(m / (4 rl)) under 512 blocks, rows = ceil(m / blocks)."""
    table = {  # (m, c): ((cl, rl, blocks, rows per block), quad kernels, LDS branch, column trips, rows of the last block)
        (1, 4): ((1, 256, 1, 1), True, False, 1, 1),               # m = 1
        (37, 4): ((1, 256, 1, 37), True, False, 1, 37),            # one quad, 256 row lanes for 37 rows
        (2500, 4): ((1, 256, 3, 834), True, False, 1, 832),        # three row blocks, the last ragged
        (297, 48): ((16, 16, 5, 60), True, False, 1, 57),          # 12 quads in 16 lanes
        (297, 256): ((64, 4, 19, 16), True, True, 1, 9),           # the LDS branch, 19 blocks, ragged
        (37, 1028): ((256, 1, 10, 4), True, True, 2, 1),           # 257 quads: the second trip has one live lane
        (98, 3): ((4, 64, 1, 98), False, False, 1, 98),            # scalar kernels
        (297, 6): ((8, 32, 3, 99), False, False, 1, 99),
        (37, 258): ((256, 1, 10, 4), False, False, 2, 1),          # the scalar column loop's second trip
    }
    assert sorted(table) == sorted(N.BN_SHAPES)
    for (m, c), want in table.items():
        g, quad, lds, trips, last = N.reduce_geom(m, c)
        assert (tuple(g), quad, lds, trips, last) == want, (m, c)
    assert N.col_geom(132 * 1000, 33).cl == 64 and N.col_geom(1, 32).cl == 32      # c >= 132 is the LDS branch
    assert N.col_geom(300000, 16) == N.ColGeom(16, 16, 1172, 256)                  # 16 rows per lane once that fills 512 blocks
    assert N.col_geom(10 ** 8, 16).blocks == 2048


def test_the_old_metric_is_blind_to_a_quiet_channels_mean():
    """spread17 at (297, 48): the quietest channel's mean moved by 1 % of that channel's own standard deviation.  The neighbouring
    tests' metric (error <= 1e-5 of the largest value of the tensor) accepts it, the per-channel bound Em rejects it."""
    case, eps = N.bn_case("spread17", 297, 48), N.f32(1e-3)
    out = N.bn_forward(case, eps, 0, dtype=N.F32)
    st = N.bn_stats(case.x, eps)
    std = st.var.sqrt()
    quiet = int(std.argmin())
    assert float(std[quiet] / std.max()) < 1e-4
    wrong = st.mean.clone()
    wrong[quiet] += 0.01 * std[quiet]
    assert N.old_close(out["save_mean"], st.mean) and N.old_close(out["save_mean"], wrong)
    assert N.within((out["save_mean"].double() - st.mean).abs(), st.Em, "mean") < 1
    with pytest.raises(AssertionError):
        N.within((out["save_mean"].double() - wrong).abs(), st.Em, "mean")
    ratio = float(((out["save_mean"].double() - wrong).abs() / st.Em)[quiet])
    assert ratio > 100
    print("\nblind-metric guard: quietest channel %d at %.1e of the loudest std; mean off by 1 %% of its std: old metric passes, "
          "per-channel error / Em = %.0f" % (quiet, float(std[quiet] / std.max()), ratio))


def test_zz_print_the_float32_ratios():
    """Not an assertion of its own: prints what the tests above measured (pytest -s), for the docstrings."""
    print("\nfloat32 CPU evaluation, largest error / bound:")
    for k in sorted(RATIOS):
        print("  %-28s %.3f" % (k, RATIOS[k]))
