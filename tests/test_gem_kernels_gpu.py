"""embnet_gem_fwd / embnet_gem_bwd through the C ABI, per element and per channel against tests/gem_ref.py within its bounds.

Shapes (n, hw, c): (2, 1, 4) one pixel; (2, 17, 68) a pixel count that is no multiple of the 16 pixel lanes and a channel quad past
one 64-channel workgroup; (3, 49, 64) the head's 7 x 7; (2, 49, 6) the scalar kernels; (1, 150, 8) past the 144 pixels whose
second sweep comes from registers.  p in {1, 3, 6.5}, one exponent or one per channel.  Inputs: positive; with zeros and negatives
(the clamp: dx exactly 0 below eps); one value exactly eps (it passes gradient); amplitudes 1e-4 and 1e5; one constant channel
(s = 1, t = 0: y is the constant and dy/dp is 0, exactly).  Also: which kernel ran (by trace), no reduction launch without dp, the
same bits from two runs, no write outside the outputs, and the argument errors.

Largest error / bound over all of the above, as measured on an MI355X (the assertion is the bound):
  y 0.200   dy/dp 0.088   dx 0.205   dp 0.066
(the bounds hold log2f / exp2f to the 3 ulp OpenCL guarantees; the device library's are nearer the 1 ulp of HIP's table).
"""
import os
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd._lib import stream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gem_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.float32(1e-6)
SHAPES = [(2, 1, 4), (2, 17, 68), (3, 49, 64), (2, 49, 6), (1, 150, 8)]
FAMILIES = ("positive", "clamped", "at_eps", "amp1e-4", "amp1e5", "constant")
EINVAL, EWORKSPACE = -1, -3
MARGIN = 256                                                  # floats on both sides of every output
RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_x(family, shape, rs):
    n, hw, c = shape
    x = (rs.rand(n, hw, c) * 2.0 + 0.1).astype(np.float32)
    if family == "clamped":
        x = rs.randn(n, hw, c).astype(np.float32)
        x.reshape(-1)[::7] = 0.0
        x[:, 0, :] = np.abs(x[:, 0, :]) + np.float32(0.25)       # (a positive value per channel, so that y is not eps everywhere)
    elif family == "at_eps":
        x[0, hw // 2, 1] = EPS
        x[-1, 0, c - 1] = np.float32(EPS * np.float32(0.5))      # and one just below it
    elif family == "amp1e-4":
        x *= np.float32(1e-4)
    elif family == "amp1e5":
        x *= np.float32(1e5)
    elif family == "constant":
        x[:, :, 0] = np.float32(0.75)
    return x


def make_p(p0, per_channel, c):
    if not per_channel:
        return np.full(1, p0, np.float32)
    return (np.float32(p0) + (np.arange(c) % 5).astype(np.float32) * np.float32(0.375)).astype(np.float32)


class Out:
    """A float32 output of `shape` between two margins of NaN."""

    def __init__(self, shape, dev):
        self.size = int(np.prod(shape))
        self.big = torch.full((self.size + 2 * MARGIN,), float("nan"), dtype=torch.float32, device=dev)
        self.t = self.big[MARGIN:MARGIN + self.size].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def get(self, what):
        assert bool(torch.isnan(self.big[:MARGIN]).all()) and bool(torch.isnan(self.big[MARGIN + self.size:]).all()), \
            what + ": wrote outside its buffer"
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


def note(name, got, want, bound):
    got = got.detach().cpu().double().numpy().reshape(want.shape)
    ratio = float(np.max(np.abs(got - want) / bound))
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    return ratio


def run(dev, x, p, dy, with_dp=True):
    """One forward and one backward on guarded outputs -> (y, dydp, dx, dp, forward kernels, backward kernels)."""
    lib = _lib.lib()
    n, hw, c = x.shape
    xd, pd, dyd = torch.tensor(x, device=dev), torch.tensor(p, device=dev), torch.tensor(dy, device=dev)
    stride = int(p.size > 1)
    y, dx = Out((n, c), dev), Out((n, hw, c), dev)
    dydp = Out((n, c), dev) if with_dp else None
    dp = Out((p.size,), dev) if with_dp else None
    ws = torch.zeros(lib.embnet_gem_bwd_workspace_bytes(c) // 8 + 1, dtype=torch.float64, device=dev)
    fwd = traced(lambda: _lib.check(lib.embnet_gem_fwd(xd.data_ptr(), n, hw, c, pd.data_ptr(), stride, float(EPS), y.ptr(),
                                                       dydp.ptr() if with_dp else None, stream())))
    bwd = traced(lambda: _lib.check(lib.embnet_gem_bwd(dyd.data_ptr(), xd.data_ptr(), y.ptr(), pd.data_ptr(), stride, float(EPS), n, hw,
                                                       c, dx.ptr(), dydp.ptr() if with_dp else None, dp.ptr() if with_dp else None,
                                                       ws.data_ptr() if with_dp else None, ws.numel() * 8 if with_dp else 0, stream())))
    if with_dp:                                               # the ticket re-armed itself: the second launch on the same workspace
        dp2 = Out((p.size,), dev)
        _lib.check(lib.embnet_gem_bwd(dyd.data_ptr(), xd.data_ptr(), y.ptr(), pd.data_ptr(), stride, float(EPS), n, hw, c, dx.ptr(),
                                      dydp.ptr(), dp2.ptr(), ws.data_ptr(), ws.numel() * 8, stream()))
        assert torch.equal(dp2.get("dp, second launch"), dp.get("dp"))
    return (y.get("y"), dydp.get("dydp") if with_dp else None, dx.get("dx"), dp.get("dp") if with_dp else None, fwd, bwd)


@pytest.mark.parametrize("per_channel", [False, True], ids=["scalar_p", "channel_p"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gem_kernels_against_reference(dev, shape, per_channel):
    n, hw, c = shape
    quad = c % 4 == 0
    rs = np.random.RandomState(1000 * hw + c)
    for p0 in (1.0, 3.0, 6.5):
        p = make_p(p0, per_channel, c)
        for family in FAMILIES:
            x, dy = make_x(family, shape, rs), rs.randn(n, c).astype(np.float32)
            ref = G.gem(x, p, EPS, dy)
            y, dydp, dx, dp, fwd, bwd = run(dev, x, p, dy)
            assert fwd == ["embnet::gem_fwd4_kernel" if quad else "embnet::gem_fwd_kernel"], fwd
            assert bwd == ["embnet::gem_bwd4_kernel" if quad else "embnet::gem_bwd_kernel", "embnet::gem_dp_kernel"], bwd
            tag = (shape, p0, per_channel, family)
            r = {"y": note("y", y, ref["y"], ref["b_y"]), "dydp": note("dydp", dydp, ref["dydp"], ref["b_dydp"])}
            # dx against the reference's own y: the bound carries the forward's rho_y for the y~ the kernel was given
            r["dx"] = note("dx", dx, ref["dx"], np.where(ref["live"], ref["b_dx"], 1.0))
            r["dp"] = note("dp", dp, ref["dp"], ref["b_dp"])
            print("gem", tag, " ".join(f"{k} {v:.3f}" for k, v in r.items()))
            assert all(v <= 1.0 for v in r.values()), (tag, r)
            dxc = dx.cpu().numpy()
            assert np.all(dxc[x < EPS] == 0.0), tag               # the clamp passes no gradient, exactly
            if family == "at_eps" and hw > 1:
                assert x[0, hw // 2, 1] == EPS and dxc[0, hw // 2, 1] != 0.0 and dxc[-1, 0, c - 1] == 0.0
            if family == "constant" or hw == 1:
                ch = slice(0, 1) if hw > 1 else slice(None)
                assert torch.equal(y[:, ch].cpu(), torch.tensor(np.maximum(x, EPS).max(axis=1)[:, ch])), tag
                assert bool((dydp[:, ch] == 0).all()), tag
            if p0 == 1.0 and not per_channel:                     # p - 1 = 0: dx = dy / hw, one rounding
                want = np.where(x >= EPS, (dy / np.float32(hw))[:, None, :], np.float32(0.0)).astype(np.float32)
                assert np.array_equal(dxc, want), tag
            # without dydp / dp: no reduction launch, the same y and dx
            y2, _, dx2, _, fwd2, bwd2 = run(dev, x, p, dy, with_dp=False)
            assert fwd2 == fwd and bwd2 == bwd[:1], (fwd2, bwd2)
            assert note("y", y2, ref["y"], ref["b_y"]) <= 1.0 and torch.equal(dx2, dx) and torch.equal(y2, y)
            # a second run: the same bits
            y3, dydp3, dx3, dp3, _, _ = run(dev, x, p, dy)
            assert torch.equal(y3, y) and torch.equal(dydp3, dydp) and torch.equal(dx3, dx) and torch.equal(dp3, dp), tag


def test_gem_bad_arguments(dev):
    lib = _lib.lib()
    n, hw, c = 2, 5, 8
    x, dy = torch.rand(n, hw, c, device=dev) + 0.1, torch.rand(n, c, device=dev)
    p, y, dydp, dx, dp = (torch.full((c,), 3.0, device=dev), torch.zeros(n, c, device=dev), torch.zeros(n, c, device=dev),
                          torch.zeros(n, hw, c, device=dev), torch.zeros(c, device=dev))
    ws = torch.zeros(lib.embnet_gem_bwd_workspace_bytes(c) // 8 + 1, dtype=torch.float64, device=dev)
    P = lambda t: t.data_ptr()  # noqa: E731

    def fwd(x=P(x), n=n, hw=hw, c=c, p=P(p), stride=1, eps=1e-6, y=P(y), dydp=P(dydp)):
        return lib.embnet_gem_fwd(x, n, hw, c, p, stride, eps, y, dydp, stream())

    def bwd(dy=P(dy), x=P(x), y=P(y), p=P(p), stride=1, eps=1e-6, n=n, hw=hw, c=c, dx=P(dx), dydp=P(dydp), dp=P(dp), ws=P(ws),
            ws_bytes=ws.numel() * 8):
        return lib.embnet_gem_bwd(dy, x, y, p, stride, eps, n, hw, c, dx, dydp, dp, ws, ws_bytes, stream())

    assert fwd() == 0 and bwd() == 0
    assert traced(lambda: bwd(dydp=None, dp=None, ws=None, ws_bytes=0)) == ["embnet::gem_bwd4_kernel"]
    for call in (lambda: fwd(x=None), lambda: fwd(p=None), lambda: fwd(y=None), lambda: fwd(n=0), lambda: fwd(hw=0),
                 lambda: fwd(c=-4), lambda: fwd(stride=2), lambda: fwd(eps=0.0), lambda: fwd(eps=float("nan")),
                 lambda: fwd(n=70000), lambda: fwd(p=P(p) + 4), lambda: fwd(y=P(y) + 4),
                 lambda: bwd(dy=None), lambda: bwd(dx=None), lambda: bwd(y=None), lambda: bwd(n=0), lambda: bwd(stride=-1),
                 lambda: bwd(eps=-1.0), lambda: bwd(dydp=None), lambda: bwd(ws=None), lambda: bwd(ws=P(ws) + 8),
                 lambda: bwd(x=P(x) + 4)):
        assert call() == EINVAL
        assert lib.embnet_last_error().decode().startswith(("gem_fwd:", "gem_bwd:"))
    assert bwd(ws_bytes=16) == EWORKSPACE
    torch.cuda.synchronize()
    assert lib.embnet_gem_bwd_workspace_bytes(c) == 16 + 8 and lib.embnet_gem_bwd_workspace_bytes(17) == 16 + 16


def test_gem_error_ratios_are_reported(dev):
    """The largest error / bound of this file's cases (the docstring's figures): printed, and asserted only against 1."""
    print("gem: largest error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(RATIOS.items())))
    assert RATIOS and all(v <= 1.0 for v in RATIOS.values())
