"""The dx pass of the stem's fused BN + activation + max-pool backward on row bands (embnet_bn_act_maxpool_bwd_band_ex): a workgroup
owns one 256-quad segment of the input row over a band of consecutive rows, so the pooled rows that neighbouring input rows share
are re-read by one CU.  Checked: dx, dgamma, dbeta and the range word bit for bit between band heights 0 (one thread per quad: the
kernel of embnet_bn_act_maxpool_bwd_ex), 8 and 5 — heights that do not divide the row count, so the last band is ragged — and
against the float64 reference at the bounds of the per-element suite (nn_ref.check_fused_backward); the range word is max |dx|.

Shapes: 3x3 / 2 pad 1 and 2x2 / 2 pad 0 (plus 3x3 / 1 pad 1: the general k > 2 stride path), c = 4 and 64, n = 2 at 9x9 and 10x7, and
two larger shapes per geometry (odd sizes; rows wider than one 256-quad segment at c = 64, so a row has a ragged last segment).
Inputs are quantised to quarter steps, so windows hold exact ties; one image region is all negative, so under ReLU whole windows
are zero (the first tap wins; at the border that is the padding, arg-max 255, which routes no gradient).
"""
import os
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd._lib import check, ptr, stream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref as N  # noqa: E402

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = N.f32(2e-5), N.f32(0.99)
BASE_SHAPES = [(2, 9, 9), (2, 10, 7)]
# (geometry, c) -> larger shapes: more than one workgroup per row and per band
LARGER_SHAPES = {(3, 2, 1, 4): [(3, 25, 53), (3, 25, 57)], (3, 2, 1, 64): [(3, 25, 53), (2, 7, 33)],
                 (2, 2, 0, 4): [(3, 26, 54), (3, 26, 58)], (2, 2, 0, 64): [(3, 26, 54), (2, 8, 34)]}
GEOMS = [(3, 2, 1), (2, 2, 0)]
CASES = [(k, s, p, c, shape) for (k, s, p) in GEOMS for c in (4, 64) for shape in BASE_SHAPES + LARGER_SHAPES[(k, s, p, c)]]
BANDS = (8, 5)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return int(t.detach().reshape(-1)[:1].view(torch.int32).item()) & 0xFFFFFFFF


def fbits(v):
    return int(np.float32(v).view(np.uint32))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def make_input(n, h, w, c, seed):
    """x in quarter steps (ties), image 0's top-left quadrant strictly negative; gamma of both signs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.round(torch.randn(n, h, w, c, generator=g) * 4.0) / 4.0
    x[0, : (h + 1) // 2, : (w + 1) // 2, :] = -0.25 - x[0, : (h + 1) // 2, : (w + 1) // 2, :].abs()
    gamma = torch.tensor([1.0, -0.5, 2.0, 1.0])[torch.arange(c) % 4].contiguous()
    beta = (torch.arange(c) % 3).float() * 0.25 - 0.25
    return x.contiguous(), gamma, beta


def bn_state(dev, x2d, gamma, beta):
    """embnet_bn_train_fwd_ex with y = NULL -> stats [4, c]: rows mean, rstd, scale, shift."""
    lib = _lib.lib()
    m, c = x2d.shape
    stats = torch.zeros((4, c), device=dev)
    nbytes = lib.embnet_bn_workspace_bytes(m, c)
    ws = torch.zeros((nbytes + 3) // 4, device=dev)
    row = [stats[i].data_ptr() for i in range(4)]
    check(lib.embnet_bn_train_fwd_ex(ptr(x2d), m, c, ptr(gamma), ptr(beta), EPS, MOMENTUM, 1, None, row[0], row[1], row[2], row[3],
                                     None, None, None, 0, ptr(ws), nbytes, None, None, None, stream()))
    torch.cuda.synchronize()
    return stats


def pool_forward(dev, x, stats, act, k, s, p):
    lib = _lib.lib()
    n, h, w, c = x.shape
    oh, ow = N.pool_out(h, k, s, p), N.pool_out(w, k, s, p)
    y = torch.full((n, oh, ow, c), 7.0, device=dev)
    am = torch.full((n, oh, ow, c), 77, device=dev, dtype=torch.uint8)
    xw = torch.full((n, oh, ow, c), 7.0, device=dev)
    check(lib.embnet_bn_act_maxpool_fwd(ptr(x), n, h, w, c, stats[2].data_ptr(), stats[3].data_ptr(), act, k, s, p, oh, ow,
                                        ptr(y), ptr(am), ptr(xw), stream()))
    torch.cuda.synchronize()
    return y, am, xw


_FWD = {}


def forward_case(dev, k, s, p, c, shape, act):
    """One forward per case: (x on the host, x, stats, y, argmax, xwin)."""
    key = (k, s, p, c, shape, act)
    if key not in _FWD:
        n, h, w = shape
        xc, gamma, beta = make_input(n, h, w, c, seed=3 * c + h)
        x, gd, bd = xc.to(dev), gamma.to(dev), beta.to(dev)
        stats = bn_state(dev, x.reshape(-1, c), gd, bd)
        y, am, xw = pool_forward(dev, x, stats, act, k, s, p)
        _FWD[key] = (xc, x, stats, y, am, xw)
    return _FWD[key]


def backward_run(dev, x, stats, am, xw, dy, k, s, p, act, training, band):
    lib = _lib.lib()
    n, h, w, c = x.shape
    oh, ow = am.shape[1], am.shape[2]
    dx = torch.full((n, h, w, c), 7.0, device=dev)
    dg, db = torch.full((c,), 7.0, device=dev), torch.full((c,), 7.0, device=dev)
    slot = torch.full((lib.embnet_range_slot_words(),), -1, dtype=torch.int32, device=dev)
    nbytes = lib.embnet_bn_act_maxpool_bwd_workspace_bytes(n, oh, ow, c)
    ws = torch.zeros((nbytes + 3) // 4, device=dev)
    check(lib.embnet_bn_act_maxpool_bwd_band_ex(ptr(dy), ptr(am), ptr(x), n, h, w, c, k, s, p, oh, ow, stats[0].data_ptr(), stats[1].data_ptr(),
                                                stats[2].data_ptr(), stats[3].data_ptr(), act, training, ptr(xw), ptr(dx), ptr(dg), ptr(db),
                                                ptr(ws), nbytes, ptr(slot), band, stream()))
    torch.cuda.synchronize()
    return dx, dg, db, slot


@pytest.mark.parametrize("k,s,p,c,shape", CASES + [(3, 1, 1, 64, (2, 9, 9)), (3, 1, 1, 4, (2, 10, 7))])
def test_pool_backward_on_row_bands(dev, k, s, p, c, shape):
    n, h, w = shape
    assert any((n * h) % band for band in BANDS), "every band height divides the row count: no ragged last band"
    act = 1
    xc, x, stats, y, am, xw = forward_case(dev, k, s, p, c, shape, act)
    assert bool((am == 255).any()) == (p > 0), "no window is won by the padding"
    assert float(y[0, 0, 0, 0]) == 0.0, "no all-negative window under ReLU"      # channel 0 (gamma > 0, beta < 0) of image 0's negative corner
    g = torch.Generator().manual_seed(11 * c + w)
    dyc = (torch.round(torch.randn(tuple(y.shape), generator=g) * 8.0) / 8.0).contiguous()
    dy = dyc.to(dev)
    st = {name: stats[i].cpu() for i, name in enumerate(("save_mean", "save_rstd", "scale", "shift"))}
    for training in (1, 0):
        base = backward_run(dev, x, stats, am, xw, dy, k, s, p, act, training, 0)
        for band in BANDS:
            got = backward_run(dev, x, stats, am, xw, dy, k, s, p, act, training, band)
            for a, b, name in zip(base, got, ("dx", "dgamma", "dbeta", "range slot")):
                if name == "range slot":
                    assert bits(a) == bits(b), "band %d: the range word differs" % band
                else:
                    assert same_bits(a, b), "band %d: %s differs" % (band, name)
        dx, dg, db, slot = got
        assert bits(slot) == fbits(float(dx.abs().max())), "the range word is not max |dx|"
        N.check_fused_backward(xc, dyc, am.cpu(), st, act, training, k, s, p, {"dx": dx.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()})
