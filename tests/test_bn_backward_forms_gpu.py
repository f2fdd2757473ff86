"""The pooled-gradient BatchNorm backward is the plain one with another source of dz.

embnet_bn_bwd_gap runs the arithmetic of embnet_bn_bwd (the shared quad helpers of nn_kernels.hip) on dz = dy * gate + dpool / hw.
So, through the C ABI, bit for bit:
  gate = NULL, dpool = 0:  dx, dgamma, dbeta of embnet_bn_bwd on dy (dy + 0 may turn a -0 of dy into +0: floats compare with ==);
  gate = NULL, dpool != 0: those of embnet_bn_bwd on dy_total = rn(dpool * (1 / hw) + dy), the broadcast-add formed with ONE rounding.
n = 2, hw = 49, c in {4, 48} (one channel quad / a quad count that divides no power of two), act in {0, 1, 2}.

Finding: the two-launch chain embnet_gap_bwd(dpool, dx_add = dy) -> embnet_bn_bwd does NOT reproduce embnet_bn_bwd_gap to the last
bit.  HIP's __fmul_rn / __fadd_rn are plain `*` and `+` to the compiler, so add_pool4's product and sum contract into one fma inside
the fused kernels, while gap_bwd_add4_kernel's result is the two-rounding sum rn(rn(dpool / hw) + dy) (DESIGN 3.2 has the figures).
The second relation is therefore asserted against the one-rounding sum.  The reference forms it in float64, where the product is
exact, and casts to float32: a sum that needs more than 53 bits is rounded twice, which differs from the fma only if the float64
value lands exactly on a float32 midpoint (about 2^-29 per element; the seeds are fixed, so the outcome does not vary between runs).
"""
import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd._lib import check, ptr, stream

pytestmark = pytest.mark.gpu

N, HW = 2, 49


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _layer(dev, c):
    """x, dy, dpool and the saved forward state of a training-mode BatchNorm over [N * HW, c]."""
    lib = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(100 + c)
    m = N * HW
    x = torch.randn((m, c), device=dev, generator=g) * 1.5 + 0.25
    dy = torch.randn((m, c), device=dev, generator=g)
    dpool = torch.randn((N, c), device=dev, generator=g) * 3.0
    gamma = torch.rand((c,), device=dev, generator=g) + 0.5
    beta = torch.randn((c,), device=dev, generator=g) * 0.3
    mean, rstd, scale, shift = (torch.empty((c,), device=dev) for _ in range(4))
    ws = torch.empty((lib.embnet_bn_workspace_bytes(m, c) // 4 + 4,), device=dev)
    check(lib.embnet_bn_train_fwd(ptr(x), m, c, ptr(gamma), ptr(beta), 1e-3, 0.99, 0, None, ptr(mean), ptr(rstd), ptr(scale),
                                  ptr(shift), None, None, None, 0, ptr(ws), ws.numel() * 4, stream()))
    return x, dy, dpool, (mean, rstd, scale, shift), ws


def _bn_bwd(dy, x, c, state, act, ws):
    lib = _lib.lib()
    mean, rstd, scale, shift = state
    dx, dgamma, dbeta = torch.empty_like(x), torch.empty((c,), device=x.device), torch.empty((c,), device=x.device)
    check(lib.embnet_bn_bwd(ptr(dy), ptr(x), N * HW, c, ptr(mean), ptr(rstd), ptr(scale), ptr(shift), act, 1, None, ptr(dx),
                            ptr(dgamma), ptr(dbeta), None, ptr(ws), ws.numel() * 4, stream()))
    return dx, dgamma, dbeta


def _bn_bwd_gap(dy, dpool, x, c, state, act, ws):
    lib = _lib.lib()
    mean, rstd, scale, shift = state
    dx, dgamma, dbeta = torch.empty_like(x), torch.empty((c,), device=x.device), torch.empty((c,), device=x.device)
    check(lib.embnet_bn_bwd_gap(ptr(dy), ptr(dpool), None, N, HW, ptr(x), c, ptr(mean), ptr(rstd), ptr(scale), ptr(shift), act,
                                ptr(dx), ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel() * 4, stream()))
    return dx, dgamma, dbeta


def _same(got, want):
    for name, a, b in zip(("dx", "dgamma", "dbeta"), got, want):
        assert bool(torch.isfinite(b).all()), name
        assert bool((a == b).all()), f"{name}: {int((a != b).sum())} of {a.numel()} elements differ, max |diff| {float((a - b).abs().max())}"


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("c", [4, 48])
def test_gap_form_with_nothing_pooled_is_the_plain_backward(dev, c, act):
    x, dy, dpool, state, ws = _layer(dev, c)
    _same(_bn_bwd_gap(dy, torch.zeros_like(dpool), x, c, state, act, ws), _bn_bwd(dy, x, c, state, act, ws))


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("c", [4, 48])
def test_gap_form_is_the_fused_broadcast_add_then_the_plain_backward(dev, c, act):
    x, dy, dpool, state, ws = _layer(dev, c)
    inv_hw = float(np.float32(1.0) / np.float32(HW))                  # the float the library passes to its kernels
    dy_total = (dpool.double().repeat_interleave(HW, dim=0) * inv_hw + dy.double()).float().contiguous()
    assert not torch.equal(dy_total, dy)
    _same(_bn_bwd_gap(dy, dpool, x, c, state, act, ws), _bn_bwd(dy_total, x, c, state, act, ws))
