"""GPU parity of the backbone layers, the backbones and the fused step against the
oracle (oracle/backbones.py on PyTorch-CPU, float64 where cheap).  Tolerances stated per test;
they are fp32-accumulation bounds, the oracle being the same arithmetic in a different order."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recipes as R
from oracle import backbones as OB
from oracle import losses as olosses
from oracle import mining as omining
from oracle import pairwise as opair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def g(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)


def close(got, want, rtol, what=""):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = want.detach().double().numpy() if torch.is_tensor(want) else np.asarray(want, np.float64)
    scale = max(np.abs(want).max(), 1e-30)
    err = np.abs(got - want).max() / scale
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert err <= rtol, f"{what}: max err / max|ref| = {err:.3e} > {rtol:.1e}"


CONV_CASES = [
    # n, h, w, cin, cout, k, stride, padding, bias, relu
    (2, 20, 20, 3, 64, 7, 2, 3, False, False),        # resnet conv0 (C=3 scalar gather)
    (2, 16, 16, 64, 64, 3, 1, 1, False, False),       # resnet 3x3
    (3, 15, 17, 64, 128, 3, 2, 1, False, False),      # stride-2 3x3, odd sizes
    (2, 14, 14, 64, 128, 1, 2, "valid", False, False),  # projection shortcut
    (2, 30, 30, 32, 32, 5, 2, "same", True, True),    # simple2 'same' stride 2 (asymmetric pad)
    (2, 31, 29, 32, 64, 5, 2, "same", True, True),
    (1, 24, 24, 3, 64, 10, 1, "valid", True, True),   # simple conv1
    (2, 12, 12, 20, 24, 3, 1, "valid", True, False),  # channels not multiples of 32
    (2, 9, 9, 6, 10, 2, 1, "valid", True, True),      # non-vector channel counts
    (4, 7, 7, 512, 512, 3, 1, 1, False, False),       # deep K (4608)
    (2, 8, 8, 256, 64, 1, 1, "valid", False, False),  # bottleneck 1x1
    (8, 40, 40, 256, 128, 3, 1, 1, True, True),       # 400 tiles of 64x64, fused bias + ReLU
    (5, 61, 59, 128, 64, 3, 1, 1, False, False),      # 282 tiles of 64x64 with a ragged last row tile
    (10, 60, 60, 64, 64, 3, 1, 1, True, True),        # 563 tiles of 64x64: the 51 left over after a round of 512 are split along K (fwd + dgrad)
    (5, 60, 60, 128, 128, 3, 1, 1, False, False),     # 564 tiles (two column tiles): 52 left-over tiles split along K
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv2d_fwd_bwd(dev, case):
    from embeddingnet_amd import layers as L
    n, h, w, cin, cout, k, stride, padding, bias, relu = case
    import zlib
    rs = np.random.RandomState(zlib.crc32(repr(case).encode()) % 2 ** 31)
    layer = L.Conv2D(cin, cout, k, strides=stride, padding=padding, use_bias=bias,
                     activation="relu" if relu else None).to(dev)
    x = rs.randn(n, h, w, cin).astype(np.float32)
    kern = (rs.randn(k, k, cin, cout) / np.sqrt(k * k * cin)).astype(np.float32)
    b = rs.randn(cout).astype(np.float32) * 0.1
    with torch.no_grad():
        layer.kernel.copy_(g(kern, dev))
        if bias:
            layer.bias.copy_(g(b, dev))
    xt = g(x, dev).requires_grad_(True)
    y = layer(xt)
    # oracle in float64
    ctx = OB.Ctx({"c/kernel": torch.tensor(kern, dtype=torch.float64, requires_grad=True),
                  "c/bias": torch.tensor(b, dtype=torch.float64, requires_grad=True)})
    xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yr = OB.conv2d(ctx, "c", xr, cout, k, stride=stride, padding=padding, bias=bias, relu=relu)
    close(y, yr, 2e-5, "fwd")
    dy = rs.randn(*yr.shape).astype(np.float32)
    y.backward(g(dy, dev))
    yr.backward(torch.tensor(dy, dtype=torch.float64))
    close(xt.grad, xr.grad, 2e-5, "dgrad")
    close(layer.kernel.grad, ctx.params["c/kernel"].grad, 2e-5, "wgrad")
    if bias:
        close(layer.bias.grad, ctx.params["c/bias"].grad, 2e-5, "bias grad")


@pytest.mark.parametrize("shape", [(4, 14, 14, 64, 64, 3), (2, 8, 8, 512, 128, 3), (4, 12, 12, 256, 256, 1)])
def test_conv2d_products_are_fp32_accurate(dev, shape):
    """The conv kernels form each fp32 product from bf16 matrix-instruction terms of an exact three-way operand split
    (include/embnet.h).  This pins that the result is fp32-class, not bf16- or tf32-class: on operands spread over six
    decades, every output / gradient element is as close to the float64 result (relative to sum|a||b|) as a float32
    convolution on the CPU is, within a factor 2 (measured: 0.75-1.6 x; three terms instead of six would be 5-10 x off,
    one term 1000 x), and on small integers, where every partial sum is representable, it is exact."""
    n, h, w, cin, cout, k = shape
    rs = np.random.RandomState(7)
    x = (rs.randn(n, h, w, cin) * 10.0 ** rs.uniform(-3, 3, (n, h, w, cin))).astype(np.float32)
    kern = (rs.randn(k, k, cin, cout) * 10.0 ** rs.uniform(-3, 3, (k, k, cin, cout))).astype(np.float32)
    dy = (rs.randn(n, h, w, cout) * 10.0 ** rs.uniform(-3, 3, (n, h, w, cout))).astype(np.float32)

    def run64(x_, k_, dy_, dt=torch.float64):
        xr = torch.tensor(x_, dtype=dt, requires_grad=True)
        kr = torch.tensor(k_, dtype=dt, requires_grad=True)
        yr = torch.nn.functional.conv2d(xr.permute(0, 3, 1, 2), kr.permute(3, 2, 0, 1), padding=k // 2).permute(0, 2, 3, 1)
        yr.backward(torch.tensor(dy_, dtype=dt))
        return yr.detach().double().numpy(), xr.grad.double().numpy(), kr.grad.double().numpy()

    from embeddingnet_amd import layers as L
    layer = L.Conv2D(cin, cout, k, padding=k // 2, use_bias=False).to(dev)

    def run_gpu(x_, k_, dy_):
        with torch.no_grad():
            layer.kernel.copy_(g(k_, dev))
        layer.kernel.grad = None
        xt = g(x_, dev).requires_grad_(True)
        y = layer(xt)
        y.backward(g(dy_, dev))
        return [t.detach().cpu().double().numpy() for t in (y, xt.grad, layer.kernel.grad)]

    want = run64(x, kern, dy)
    mag = run64(np.abs(x), np.abs(kern), np.abs(dy))           # sum |a||b| of every output / gradient element
    cpu32 = run64(x, kern, dy, torch.float32)
    for name, got, c32, ref, m in zip(("fwd", "dgrad", "wgrad"), run_gpu(x, kern, dy), cpu32, want, mag):
        err, err32 = (np.abs(got - ref) / m).max(), (np.abs(c32 - ref) / m).max()
        assert err <= max(2 * err32, 5e-7), f"{name}: max |err| / sum|a||b| = {err:.2e}, float32 CPU conv {err32:.2e}"
    xi = rs.randint(-60, 61, x.shape).astype(np.float32)
    ki = rs.randint(-3, 4, kern.shape).astype(np.float32)
    di = rs.randint(-2, 3, dy.shape).astype(np.float32)
    for name, got, ref in zip(("fwd", "dgrad", "wgrad"), run_gpu(xi, ki, di), run64(xi, ki, di)):
        assert np.array_equal(got, ref), f"{name}: integer operands must come out exact"


@pytest.mark.parametrize("shape", [(2, 16, 16, 64, 64), (8, 40, 40, 256, 128), (10, 60, 60, 64, 64), (2, 9, 9, 6, 10)])
def test_conv2d_residual_epilogue(dev, shape):
    """Conv2D(x, residual=r) == Conv2D(x) + r bit for bit (whole tiles, K-split left-over tiles and the scalar
    path), and the Add's gradient reaches r unchanged."""
    from embeddingnet_amd import layers as L
    n, h, w, cin, cout = shape
    gen = torch.Generator().manual_seed(5)
    conv = L.Conv2D(cin, cout, 3, padding=1, use_bias=False, gen=gen).to(dev)
    x = torch.randn((n, h, w, cin), device=dev)
    r = torch.randn((n, h, w, cout), device=dev, requires_grad=True)
    y0 = conv(x)
    y1 = conv(x, residual=r)
    assert torch.equal(y1, y0 + r)
    dy = torch.randn_like(y1)
    y1.backward(dy)
    assert torch.equal(r.grad, dy)
    with pytest.raises(Exception):
        conv(x, residual=r[:, 1:])


@pytest.mark.parametrize("shape,k,stride,act", [((2, 16, 16, 64, 64), 3, 1, "relu"), ((8, 40, 40, 256, 128), 3, 1, "relu"),
                                                ((3, 15, 17, 64, 128), 3, 2, "relu"), ((2, 14, 14, 64, 128), 1, 2, None),
                                                ((2, 12, 12, 32, 48), 3, 1, "swish")])
def test_deferred_batchnorm_into_conv(dev, shape, k, stride, act):
    """bn(x, defer=True) -> Conv2D applies the BN affine + activation while gathering (forward and wgrad):
    outputs and every gradient equal the materialised BN -> conv path bit for bit (same operands, same order)."""
    from embeddingnet_amd import layers as L
    n, h, w, cin, cout = shape
    x = torch.randn((n, h, w, cin), device=dev) * 1.5 + 0.3
    res = {}
    # (the materialised path's BatchNorm-backward sums by the BatchNorm's own reduction pass, as the deferred path computes
    # them: with layers.FUSE_BN_SUMS the conv's data gradient would produce them in another summation order)
    with L.switches(FUSE_BN_SUMS=False):
        for defer in (False, True):
            gen = torch.Generator().manual_seed(11)
            bn = L.BatchNormalization(cin, epsilon=2e-5, activation=act).to(dev).train()
            conv = L.Conv2D(cin, cout, k, strides=stride, padding=k // 2, use_bias=False, gen=gen).to(dev)
            with torch.no_grad():
                bn.gamma.copy_(torch.linspace(-1.0, 1.5, cin)); bn.beta.copy_(torch.linspace(0.4, -0.4, cin))
            xt = x.clone().requires_grad_(True)
            a = bn(xt, defer=defer)
            assert isinstance(a, L.Deferred) == defer
            y = conv(a)
            y.backward(torch.cos(y.detach() * 3))
            res[defer] = (y.detach(), xt.grad, conv.kernel.grad, bn.gamma.grad, bn.beta.grad, bn.moving_mean.clone())
            if defer:                                   # a consumer that cannot fuse gets the materialised tensor
                bn2 = L.BatchNormalization(cin, epsilon=2e-5, activation=act).to(dev).train()
                with torch.no_grad():
                    bn2.gamma.copy_(bn.gamma); bn2.beta.copy_(bn.beta)
                assert torch.equal(bn(x, defer=True).materialize(), bn2(x))
    for got, want, what in zip(res[True], res[False], ("y", "dx", "dW", "dgamma", "dbeta", "moving_mean")):
        assert torch.equal(got, want), what


@pytest.mark.parametrize("shape,k,stride", [((2, 16, 16, 64, 64), 3, 1), ((8, 40, 40, 256, 128), 3, 1),
                                            ((5, 61, 59, 128, 64), 3, 1), ((3, 15, 17, 64, 128), 3, 2),
                                            ((2, 9, 9, 8, 32), 1, 1), ((10, 60, 60, 64, 64), 3, 1)])
def test_conv_epilogue_statistics_feed_batchnorm(dev, shape, k, stride):
    """Conv2D(emit_stats=True) hands the next BatchNormalization its per-channel sums from the conv epilogue
    (whole tiles and K-split left-over tiles, with a residual): same BN output, moving statistics and gradients
    as the BN that reads its input again (fp32 summation order differs)."""
    from embeddingnet_amd import layers as L
    n, h, w, cin, cout = shape
    x = torch.randn((n, h, w, cin), device=dev)
    res = {}
    for emit in (False, True):
        gen = torch.Generator().manual_seed(3)
        conv = L.Conv2D(cin, cout, k, strides=stride, padding=k // 2, use_bias=False, gen=gen).to(dev)
        bn = L.BatchNormalization(cout, epsilon=2e-5, relu=True).to(dev).train()
        xt = x.clone().requires_grad_(True)
        y = conv(xt, emit_stats=emit)
        r = torch.sin(y.detach() * 2)                        # a residual, so the statistics are of conv + residual
        y = conv(xt, residual=r, emit_stats=emit)
        assert (getattr(y, "_bn_partials", None) is not None) == emit
        if emit:
            m = y.numel() // cout
            p = y._bn_partials.double().sum(2)
            close(p[0] / m, y.double().mean((0, 1, 2)).cpu(), 1e-5, "epilogue sum")
            close(p[1] / m, (y.double() ** 2).mean((0, 1, 2)).cpu(), 1e-5, "epilogue sum of squares")
        z = bn(y)
        z.backward(torch.cos(z.detach()))
        res[emit] = (z.detach(), bn.moving_mean.clone(), bn.moving_variance.clone(), xt.grad, bn.gamma.grad, bn.beta.grad)
    for got, want, what in zip(res[True], res[False], ("bn out", "moving mean", "moving var", "dx", "dgamma", "dbeta")):
        close(got, want.double().cpu(), 2e-5, what)


@pytest.mark.parametrize("c", [64, 6])
def test_batchnorm_with_skip_folds_the_shortcut_gradient(dev, c):
    """bn(x, with_skip=True) -> (bn(x), x): the gradient arriving through the pass-through copy is added inside the
    BN backward kernel; same result as letting autograd accumulate the two gradients of x."""
    from embeddingnet_amd import layers as L
    x = torch.randn((3, 10, 11, c), device=dev)
    w1, w2 = torch.randn_like(x), torch.randn_like(x)
    res = []
    for fold in (False, True):
        bn = L.BatchNormalization(c, epsilon=2e-5, relu=True).to(dev).train()
        xt = x.clone().requires_grad_(True)
        if fold:
            a, skip = bn(xt, with_skip=True)
        else:
            a, skip = bn(xt), xt
        ((a * w1).sum() + (skip * w2).sum()).backward()
        res.append((a.detach(), xt.grad, bn.gamma.grad, bn.beta.grad))
    assert torch.equal(res[0][0], res[1][0])
    for got, want, what in zip(res[1][1:], res[0][1:], ("dx", "dgamma", "dbeta")):
        close(got, want.double().cpu(), 1e-6, what)


@pytest.mark.parametrize("shape,stride", [((2, 16, 16, 64, 64), 1), ((3, 15, 17, 64, 128), 2), ((8, 40, 40, 256, 128), 1),
                                          ((2, 9, 9, 6, 10), 2), ((10, 60, 60, 64, 64), 1)])
def test_conv_pair_accumulates_the_input_gradient(dev, shape, stride):
    """conv_pair(x, 3x3, 1x1 projection): one node whose backward lets the second dgrad add into the first one's
    output (skipping pixels a strided 1x1 never touches) — same values as two separate convs + autograd's add."""
    from embeddingnet_amd import layers as L
    n, h, w, cin, cout = shape
    x = torch.randn((n, h, w, cin), device=dev)
    res = []
    for fused in (False, True):
        gen = torch.Generator().manual_seed(9)
        c1 = L.Conv2D(cin, cout, 3, strides=stride, padding=1, use_bias=False, gen=gen).to(dev)
        c2 = L.Conv2D(cin, cout, 1, strides=stride, padding="valid", use_bias=False, gen=gen).to(dev)
        xt = x.clone().requires_grad_(True)
        y1, y2 = L.conv_pair(xt, c1, c2) if fused else (c1(xt), c2(xt))
        (y1 * torch.cos(y1.detach()) + 0.5 * y2 * torch.sin(y2.detach() * 2)).sum().backward()
        res.append((y1.detach(), y2.detach(), xt.grad, c1.kernel.grad, c2.kernel.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for got, want, what in zip(res[1][2:], res[0][2:], ("dx", "dW1", "dW2")):
        close(got, want.double().cpu(), 1e-6, what)


@pytest.mark.parametrize("shape,k,stride", [((2, 16, 16, 64, 64), 1, 1), ((8, 40, 40, 256, 128), 3, 1), ((2, 9, 9, 6, 10), 3, 1),
                                            ((3, 15, 17, 64, 128), 3, 2), ((10, 60, 60, 64, 64), 3, 1)])
def test_conv_with_skip_folds_the_skip_gradient(dev, shape, k, stride):
    """conv(x, with_skip=True) -> (conv(x), x): the gradient of the pass-through copy is added in the data-gradient
    epilogue (whole tiles, K-split tiles, scalar path, strided classes); same as autograd's own accumulation."""
    from embeddingnet_amd import layers as L
    n, h, w, cin, cout = shape
    x = torch.randn((n, h, w, cin), device=dev)
    w2 = torch.randn_like(x)
    res = []
    for fold in (False, True):
        gen = torch.Generator().manual_seed(13)
        conv = L.Conv2D(cin, cout, k, strides=stride, padding=k // 2, use_bias=False, gen=gen).to(dev)
        xt = x.clone().requires_grad_(True)
        y, skip = conv(xt, with_skip=True) if fold else (conv(xt), xt)
        ((y * torch.cos(y.detach())).sum() + (skip * w2).sum()).backward()
        res.append((y.detach(), xt.grad, conv.kernel.grad))
    assert torch.equal(res[0][0], res[1][0])
    close(res[1][1], res[0][1].double().cpu(), 1e-6, "dx")
    close(res[1][2], res[0][2].double().cpu(), 1e-6, "dW")


def test_conv_tail_split_is_planned_for_the_test_shapes():
    """The two big CONV_CASES must really take the remainder-split path (host-side plan, no launch)."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    assert lib.embnet_conv2d_fwd_workspace_bytes(10, 64, 3, 3, 64, 60, 60) > 0
    assert lib.embnet_conv2d_dgrad_workspace_bytes(10, 60, 60, 64, 3, 3, 64, 1) > 0
    assert lib.embnet_conv2d_fwd_workspace_bytes(5, 128, 3, 3, 128, 60, 60) > 0
    # a launch below one round (8 tiles here) cuts EVERY tile's K range over several workgroups (round 4: plan_tail's small-launch
    # split): parts x tiles x 64 x 64 x 4 bytes, parts <= kt / 3 = 6
    small = lib.embnet_conv2d_fwd_workspace_bytes(2, 64, 3, 3, 64, 16, 16)
    assert small > 0 and small % (8 * 64 * 64 * 4) == 0 and 2 <= small // (8 * 64 * 64 * 4) <= 6
    assert lib.embnet_conv2d_fwd_workspace_bytes(1, 8, 1, 1, 8, 4, 4) == 0            # one K tile: nothing to cut


def test_conv2d_wgrad_splitk_large(dev):
    """Enough output pixels to force many split-K slabs (stage-0 shape at a small batch)."""
    from embeddingnet_amd import layers as L
    rs = np.random.RandomState(3)
    layer = L.Conv2D(64, 64, 3, padding=1, use_bias=False).to(dev)
    x = rs.randn(8, 56, 56, 64).astype(np.float32)
    dy = rs.randn(8, 56, 56, 64).astype(np.float32)
    xt = g(x, dev)
    layer(xt).backward(g(dy, dev))
    xr = torch.tensor(x).permute(0, 3, 1, 2).double()
    dyr = torch.tensor(dy).permute(0, 3, 1, 2).double()
    wr = torch.nn.grad.conv2d_weight(xr, (64, 64, 3, 3), dyr, padding=1).permute(2, 3, 1, 0)
    close(layer.kernel.grad, wr, 2e-5, "wgrad split-K")


@pytest.mark.parametrize("c,relu,scale", [(64, True, True), (3, False, False), (32, False, True), (100, True, True)])
def test_batchnorm_train(dev, c, relu, scale):
    from embeddingnet_amd import layers as L
    rs = np.random.RandomState(c)
    x = (rs.randn(4, 9, 11, c) * 2 + 0.5).astype(np.float32)
    bn = L.BatchNormalization(c, epsilon=2e-5, scale=scale, relu=relu).to(dev).train()
    gam = rs.rand(c).astype(np.float32) + 0.5
    bet = rs.randn(c).astype(np.float32) * 0.3
    with torch.no_grad():
        if scale:
            bn.gamma.copy_(g(gam, dev))
        bn.beta.copy_(g(bet, dev))
    xt = g(x, dev).requires_grad_(True)
    y = bn(xt)
    P = {"b/beta": torch.tensor(bet, dtype=torch.float64, requires_grad=True)}
    if scale:
        P["b/gamma"] = torch.tensor(gam, dtype=torch.float64, requires_grad=True)
    P["b/moving_mean"] = torch.zeros(c, dtype=torch.float64)
    P["b/moving_variance"] = torch.ones(c, dtype=torch.float64)
    ctx = OB.Ctx(P, training=True)
    xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yr = OB.batchnorm(ctx, "b", xr, eps=2e-5, scale=scale)
    if relu:
        yr = torch.relu(yr)
    close(y, yr, 1e-5, "bn fwd")
    close(bn.moving_mean, ctx.new_stats["b/moving_mean"], 1e-5, "moving mean")
    close(bn.moving_variance, ctx.new_stats["b/moving_variance"], 1e-5, "moving var")
    dy = rs.randn(*x.shape).astype(np.float32)
    y.backward(g(dy, dev))
    yr.backward(torch.tensor(dy, dtype=torch.float64))
    close(xt.grad, xr.grad, 2e-5, "bn dx")
    close(bn.beta.grad, P["b/beta"].grad, 2e-5, "dbeta")
    if scale:
        close(bn.gamma.grad, P["b/gamma"].grad, 2e-5, "dgamma")
    # inference mode uses the moving statistics
    bn.eval()
    yi = bn(g(x, dev))
    ctx2 = OB.Ctx({k: (ctx.new_stats[k] if k in ctx.new_stats else v.detach()) for k, v in P.items()}, training=False)
    yri = OB.batchnorm(ctx2, "b", torch.tensor(x, dtype=torch.float64), eps=2e-5, scale=scale)
    close(yi, torch.relu(yri) if relu else yri, 1e-5, "bn infer")


@pytest.mark.parametrize("k,s,pad,h,w", [(2, 2, 0, 12, 12), (2, 2, 0, 13, 11), (3, 2, 1, 16, 16), (3, 2, 1, 15, 17)])
def test_maxpool(dev, k, s, pad, h, w):
    from embeddingnet_amd import layers as L
    rs = np.random.RandomState(k * 100 + h)
    x = np.maximum(rs.randn(3, h, w, 20), 0).astype(np.float32)       # post-ReLU: many exact-zero ties
    xt = g(x, dev).requires_grad_(True)
    y = L.MaxPool2D(k, s, zero_pad=pad)(xt)
    xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yr = OB.maxpool(xr, k, s, zero_pad=pad)
    assert torch.equal(y.detach().cpu().double(), yr.detach())
    dy = rs.randn(*yr.shape).astype(np.float32)
    y.backward(g(dy, dev))
    yr.backward(torch.tensor(dy, dtype=torch.float64))
    close(xt.grad, xr.grad, 1e-6, "maxpool dx")


@pytest.mark.parametrize("c,act,k,s,pad,h,w", [(64, "relu", 3, 2, 1, 16, 16), (8, "relu", 3, 2, 1, 15, 17),
                                               (16, None, 2, 2, 0, 12, 10), (12, "swish", 3, 2, 1, 9, 9)])
def test_bn_act_maxpool_fused(dev, c, act, k, s, pad, h, w):
    """The fused stem (bn -> act -> ZeroPadding2D -> MaxPool in one pass, backward from the pooled gradient)
    against the oracle's three separate layers, training and inference statistics."""
    from embeddingnet_amd import layers as L
    rs = np.random.RandomState(c + h)
    x = (rs.randn(3, h, w, c) * 1.5 + 0.2).astype(np.float32)
    bn = L.BatchNormalization(c, epsilon=2e-5, activation=act).to(dev).train()
    pool = L.MaxPool2D(k, s, zero_pad=pad)
    gam, bet = rs.rand(c).astype(np.float32) + 0.5, rs.randn(c).astype(np.float32) * 0.3
    gam[::3] *= -1                                       # negative scales: max does not commute with the affine
    with torch.no_grad():
        bn.gamma.copy_(g(gam, dev)); bn.beta.copy_(g(bet, dev))
    P = {"b/beta": torch.tensor(bet, dtype=torch.float64, requires_grad=True),
         "b/gamma": torch.tensor(gam, dtype=torch.float64, requires_grad=True),
         "b/moving_mean": torch.zeros(c, dtype=torch.float64), "b/moving_variance": torch.ones(c, dtype=torch.float64)}

    def ref(ctx, xr):
        z = OB.batchnorm(ctx, "b", xr, eps=2e-5)
        z = torch.relu(z) if act == "relu" else (z * torch.sigmoid(z) if act == "swish" else z)
        return OB.maxpool(z, k, s, zero_pad=pad)

    xt = g(x, dev).requires_grad_(True)
    y = L.bn_act_maxpool(xt, bn, pool)
    ctx = OB.Ctx(P, training=True)
    xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yr = ref(ctx, xr)
    close(y, yr, 1e-5, "fused stem fwd")
    close(bn.moving_mean, ctx.new_stats["b/moving_mean"], 1e-5, "moving mean")
    dy = rs.randn(*yr.shape).astype(np.float32)
    y.backward(g(dy, dev))
    yr.backward(torch.tensor(dy, dtype=torch.float64))
    close(xt.grad, xr.grad, 2e-5, "fused stem dx")
    close(bn.beta.grad, P["b/beta"].grad, 2e-5, "fused stem dbeta")
    close(bn.gamma.grad, P["b/gamma"].grad, 2e-5, "fused stem dgamma")
    # identical to our own unfused layers up to summation order
    bn2 = L.BatchNormalization(c, epsilon=2e-5, activation=act).to(dev).train()
    with torch.no_grad():
        bn2.gamma.copy_(g(gam, dev)); bn2.beta.copy_(g(bet, dev))
    x2 = g(x, dev).requires_grad_(True)
    y2 = pool(bn2(x2))
    assert torch.equal(y2, y)
    y2.backward(g(dy, dev))
    close(xt.grad, x2.grad.double().cpu(), 2e-6, "fused vs unfused dx")
    # inference statistics, with a gradient through the frozen affine
    bn.eval()
    xe = g(x, dev).requires_grad_(True)
    ye = L.bn_act_maxpool(xe, bn, pool)
    ctx2 = OB.Ctx({kk: (ctx.new_stats[kk] if kk in ctx.new_stats else v.detach()) for kk, v in P.items()}, training=False)
    xre = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yre = ref(ctx2, xre)
    close(ye, yre, 1e-5, "fused stem infer")
    ye.backward(g(dy, dev)); yre.backward(torch.tensor(dy, dtype=torch.float64))
    close(xe.grad, xre.grad, 2e-5, "fused stem infer dx")


def test_dense_gap_add_l2(dev):
    from embeddingnet_amd import layers as L
    rs = np.random.RandomState(4)
    for m, i, o, relu in [(32, 9216, 256, True), (8, 512, 128, True), (5, 70, 33, False), (128, 12800, 512, True)]:
        d = L.Dense(i, o, activation="relu" if relu else None, gen=torch.Generator().manual_seed(i + o)).to(dev)
        with torch.no_grad():
            d.bias.copy_(g(0.5 * rs.randn(o), dev))           # (the layer starts at zero: a bias read from the wrong column would pass)
        x = rs.randn(m, i).astype(np.float32)
        tol = 2e-5 * max(1.0, (i / 2048) ** 0.5)            # k-ordered f32 chains of length `in` vs f64
        xt = g(x, dev).requires_grad_(True)
        y = d(xt)
        wr = d.kernel.detach().cpu().double().requires_grad_(True)
        br = d.bias.detach().cpu().double().requires_grad_(True)
        xr = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        yr = xr @ wr + br
        if relu:
            yr = torch.relu(yr)
        close(y, yr, tol, "dense fwd")
        dy = rs.randn(m, o).astype(np.float32)
        y.backward(g(dy, dev))
        yr.backward(torch.tensor(dy, dtype=torch.float64))
        close(xt.grad, xr.grad, tol, "dense dx")
        close(d.kernel.grad, wr.grad, tol, "dense dw")
        close(d.bias.grad, br.grad, tol, "dense db")
    x = rs.randn(4, 7, 7, 96).astype(np.float32)
    xt = g(x, dev).requires_grad_(True)
    y = L.GlobalAveragePooling2D()(xt)
    close(y, torch.tensor(x).double().mean(dim=(1, 2)), 1e-6, "gap")
    y.sum().backward()
    close(xt.grad, torch.full(x.shape, 1 / 49.0, dtype=torch.float64), 1e-6, "gap dx")
    a, b = rs.randn(1000).astype(np.float32), rs.randn(1000).astype(np.float32)
    assert np.array_equal(L.add(g(a, dev), g(b, dev)).cpu().numpy(), a + b)
    w = g(rs.randn(3, 3, 16, 8), dev).requires_grad_(True)
    pen = L.l2_penalty(w, 2e-4)
    close(pen, 2e-4 * (w.detach().cpu().double() ** 2).sum(), 1e-6, "l2 penalty")
    (pen * 2).backward()
    close(w.grad, 2 * 2 * 2e-4 * w.detach().cpu().double(), 1e-6, "l2 grad")


def _oracle_from(model, training, dtype=torch.float64):
    from embeddingnet_amd.backbones import keras_weights
    params = {k: v.detach().cpu().to(dtype).requires_grad_(v.requires_grad) for k, v in keras_weights(model).items()}
    return OB.Ctx(params, training=training)


@pytest.mark.parametrize("name,shape,enc,batch", [("simple", (73, 73, 3), 64, 6), ("simple2", (64, 64, 3), 64, 8),
                                                   ("resnet18", (64, 64, 3), 64, 8), ("resnet50", (128, 128, 3), 32, 6)])
def test_backbone_forward_backward_vs_oracle(dev, name, shape, enc, batch):
    from embeddingnet_amd import backbones as B

    def one_input(seed):
        base, backbone = B.get_backbone(shape, encodings_len=enc, backbone_name=name, backbone_weights=None, seed=1,
                                        device=dev)
        for m in base.modules():
            if hasattr(m, "enabled"):
                m.enabled = False                         # dropout off for parity
        rs = np.random.RandomState(seed)
        x = rs.rand(batch, *shape).astype(np.float32)
        base.train()
        emb = base(g(x, dev))
        ctx = _oracle_from(base, training=True)
        embr = OB.base_model(ctx, torch.tensor(x, dtype=torch.float64), backbone_name=name, encodings_len=enc)
        close(emb, embr, 2e-4, f"{name} embeddings (train mode)")
        wgt = rs.randn(batch, enc).astype(np.float32)
        (emb * g(wgt, dev)).sum().backward()
        (embr * torch.tensor(wgt, dtype=torch.float64)).sum().backward()
        got = B.keras_weights(base)
        # fp32 noise floor of this very network: the same oracle run in float32 vs float64.  Max-pool
        # arg-max and ReLU decisions that flip between precisions move a few gradients by ~1e-2 in ANY
        # fp32 implementation (tests/diag_backbone.py prints both columns), so the bound is relative to it.
        ctx32 = _oracle_from(base, training=True, dtype=torch.float32)
        emb32 = OB.base_model(ctx32, torch.tensor(x), backbone_name=name, encodings_len=enc)
        (emb32 * torch.tensor(wgt)).sum().backward()
        bad, num, den, total = {}, 0.0, 0.0, 0
        for k, p in ctx.params.items():
            if p.grad is None:
                continue
            total += 1
            diff = got[k].grad.detach().cpu().double() - p.grad
            scale = max(p.grad.abs().max().item(), 1e-12)
            err = diff.abs().max().item() / scale
            floor = (ctx32.params[k].grad.double() - p.grad).abs().max().item() / scale
            num += (diff ** 2).sum().item()
            den += (p.grad ** 2).sum().item()
            assert err < 0.3, f"{name}: grad {k} rel err {err:.2e}"
            if err >= 5 * floor + 1e-4:
                bad[k] = f"{k}: {err:.2e} (floor {floor:.2e})"
        assert (num / den) ** 0.5 < 2e-2, f"{name}: global gradient rel-L2 error {(num / den) ** 0.5:.2e}"
        return base, x, bad, total

    # Every parameter gradient within 5x the float32 oracle's own deviation (+ 1e-4) of the float64 oracle for at least 97.5 % of
    # the tensors; the rest are printed and stay within the loose bounds above.  What pushes a tensor out is a ReLU / arg-max
    # decision that fell the other way than in the float32 oracle run: ONE such flip early in the net (an element of stage 1's
    # BatchNorm output within 1e-6 of zero) moves every gradient tensor upstream of it by 1e-4 ... 1e-2 — half a dozen at once, on
    # about one input in three for any arithmetic whose rounding differs from the oracle's (tools/exp/debug_stem_grads.py).  So a
    # tensor counts as off only if it is off on BOTH of two inputs: a wiring error is there every time, a flip chain is not.
    # The per-STAGE gradient check (tests/test_round3_gpu.py::test_stage_gradients_vs_oracle) is the one that localises a wiring error.
    base, x, bad, total = one_input(0)
    if len(bad) > max(total // 40, 1):
        print(f"{name}: {len(bad)} of {total} gradient tensors beyond 5x the float32 floor on the first input: {list(bad.values())}")
        _, _, bad2, _ = one_input(1)
        bad = {k: v + " | " + bad2[k] for k, v in bad.items() if k in bad2}
    elif bad:
        print(f"{name}: {len(bad)} of {total} gradient tensors beyond 5x the float32 floor: {list(bad.values())}")
    assert len(bad) <= max(total // 40, 1), f"{name}: {len(bad)} of {total} tensors off: {list(bad.values())}"
    # inference path (moving stats) through Model.predict
    pred = base.predict(x)
    ctx_i = _oracle_from(base, training=False)
    embi = OB.base_model(ctx_i, torch.tensor(x, dtype=torch.float64), backbone_name=name, encodings_len=enc)
    close(pred, embi, 2e-4, f"{name} predict()")


def test_fused_step_loss_and_grads_vs_oracle(dev):
    """simple2 @64x64, P=8,K=4, hardest mining: total loss (triplet mean + regularisers) and all
    parameter gradients vs the oracle composition embeddings -> sklearn-style matrix -> mining -> hinge."""
    from embeddingnet_amd import backbones as B
    from embeddingnet_amd.train_step import TripletTrainer
    p, k, enc, m = 8, 4, 64, 0.5
    base, _ = B.get_backbone((64, 64, 3), encodings_len=enc, backbone_name="simple2", backbone_weights=None,
                             seed=2, device=dev)
    for mod in base.modules():
        if hasattr(mod, "enabled"):
            mod.enabled = False
    rs = np.random.RandomState(1)
    cls = rs.rand(p, 64, 64, 3)
    x = np.clip(np.repeat(cls, k, axis=0) + 0.15 * rs.randn(p * k, 64, 64, 3), 0, 1).astype(np.float32)
    tr = TripletTrainer(base, None, p, k, margin=m, negatives_selection_mode="hardest")
    base.train()
    total, mean, count = tr.loss(g(x, dev))
    total.backward()
    ctx = _oracle_from(base, training=True)
    embr = OB.base_model(ctx, torch.tensor(x, dtype=torch.float64), backbone_name="simple2", encodings_len=enc)
    mined = omining.mine_from_embeddings(embr.detach().numpy().astype(np.float32), p, k, m, "hardest")
    t = mined["triplets"]
    assert int(count.item()) == len(t)
    # The GPU mined on ITS fp32 embeddings.  Where its pick differs from the oracle's, the two candidate
    # negatives must be an fp32-borderline tie of the reference's loss values (then the loss barely moves
    # but the gradient is routed to another row); the gradient comparison below uses the GPU's triplets.
    with torch.no_grad():
        t_gpu = tr.mine(base(g(x, dev)))[0].cpu().numpy()[: len(t)]
    assert np.array_equal(t_gpu[:, :2], t[:, :2])
    d_or = opair.pairwise_distances(embr.detach().numpy().astype(np.float32))
    for (a, pp, n_gpu), n_or in zip(t_gpu, t[:, 2]):
        assert n_gpu == n_or or abs(d_or[a, n_gpu] - d_or[a, n_or]) < 1e-5, (a, pp, n_gpu, n_or)
    t = t_gpu
    yr = torch.cat([embr[t[:, 0]], embr[t[:, 1]], embr[t[:, 2]]], dim=1)
    e = enc
    pos = ((yr[:, :e] - yr[:, e:2 * e]) ** 2).sum(1)
    neg = ((yr[:, :e] - yr[:, 2 * e:]) ** 2).sum(1)
    rows = torch.clamp(pos - neg + m, min=0)
    np.testing.assert_allclose(rows.detach().numpy(), olosses.triplet_loss(m)(None, yr.detach().numpy()), rtol=1e-12)
    total_r = rows.mean() + OB.regularisation(ctx)
    # north_star: loss values within 1e-4 relative
    assert abs(total.item() - total_r.item()) <= 1e-4 * abs(total_r.item()), (total.item(), total_r.item())
    assert abs(mean.item() - rows.mean().item()) <= 1e-4 * abs(rows.mean().item())
    total_r.backward()
    # fp32 noise floor of this step: the same oracle composition in float32 (same mined triplets)
    ctx32 = _oracle_from(base, training=True, dtype=torch.float32)
    e32 = OB.base_model(ctx32, torch.tensor(x), backbone_name="simple2", encodings_len=enc)
    y32 = torch.cat([e32[t[:, 0]], e32[t[:, 1]], e32[t[:, 2]]], dim=1)
    rows32 = torch.clamp(((y32[:, :e] - y32[:, e:2 * e]) ** 2).sum(1) - ((y32[:, :e] - y32[:, 2 * e:]) ** 2).sum(1) + m, min=0)
    (rows32.mean() + OB.regularisation(ctx32)).backward()
    got = B.keras_weights(base)
    # A ReLU pre-activation within ~1e-6 of zero can land on the other side in a different fp32 summation
    # order (measured: one conv6 unit flips between two of our own BN reduction orders), which moves a
    # 5x5xC patch of gradients by O(1e-3) of the max while every tensor still agrees to ~1e-6 before it.
    # So: element-wise bound where the fp32 oracle itself is tight, and an L2 bound per tensor everywhere.
    num = den = 0.0
    for kname, pr in ctx.params.items():
        if pr.grad is None:
            continue
        diff = got[kname].grad.detach().cpu().double() - pr.grad
        scale = max(pr.grad.abs().max().item(), 1e-12)
        err = diff.abs().max().item() / scale
        l2 = (diff.norm() / max(pr.grad.norm().item(), 1e-30)).item()
        num += (diff ** 2).sum().item()
        den += (pr.grad ** 2).sum().item()
        assert err < 2e-2 and l2 < 5e-3, f"grad {kname}: max-rel {err:.2e}, rel-L2 {l2:.2e}"
    assert (num / den) ** 0.5 < 2e-3, f"global gradient rel-L2 error {(num / den) ** 0.5:.2e}"


def test_stem_beta_gradient_from_border_strips(dev):
    """bn_data's beta gradient through conv0 (layers.input_bn_conv): with zero_sum_dy (conv0's only consumer is a
    training-mode BatchNormalization, whose data gradient sums to zero per channel) the per-tap sums of dy come from the
    border strips alone (embnet_tap_border_sums); same gradient as the full per-tap sums, and as the float64 autograd
    of the plain layers."""
    from embeddingnet_amd import layers as L
    gen = torch.Generator().manual_seed(3)
    n, h, w = 6, 40, 36
    bn_data = L.BatchNormalization(3, epsilon=2e-5, scale=False).to(dev)
    conv0 = L.Conv2D(3, 64, 7, strides=2, padding=3, use_bias=False, gen=gen).to(dev)
    bn0 = L.BatchNormalization(64, epsilon=2e-5, relu=True).to(dev)
    x = torch.rand((n, h, w, 3), device=dev)
    up = torch.randn((n, 20, 18, 64), device=dev)
    grads = {}
    for flag in (False, True):
        for m in (bn_data, conv0, bn0):
            m.zero_grad(set_to_none=True)
        y = bn0(L.input_bn_conv(x, bn_data, conv0, zero_sum_dy=flag))
        (y * up).sum().backward()
        grads[flag] = (bn_data.beta.grad.clone(), conv0.kernel.grad.clone())
    scale = grads[False][0].abs().max().item()
    assert (grads[True][0] - grads[False][0]).abs().max().item() <= 2e-5 * max(scale, 1e-6) + 1e-6
    assert torch.equal(grads[True][1], grads[False][1])
    # float64 reference of the same three layers
    xr = x.detach().cpu().double()
    beta = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    xm = xr.mean((0, 1, 2)); xv = xr.var((0, 1, 2), unbiased=False)
    a = (xr - xm) / torch.sqrt(xv + 2e-5) + beta
    kr = conv0.kernel.detach().cpu().double()
    yr = F.conv2d(a.permute(0, 3, 1, 2), kr.permute(3, 2, 0, 1), stride=2, padding=3).permute(0, 2, 3, 1)
    ym = yr.mean((0, 1, 2)); yv = yr.var((0, 1, 2), unbiased=False)
    out = torch.relu((yr - ym) / torch.sqrt(yv + 2e-5) * bn0.gamma.detach().cpu().double() + bn0.beta.detach().cpu().double())
    (out * up.cpu().double()).sum().backward()
    close(grads[True][0], beta.grad, 2e-4, "beta gradient vs float64")


@pytest.mark.parametrize("geom", [(3, 9, 11, 8, 3, 3, 1, 1, 1, 9, 11),          # n, oh, ow, k, r, s, stride, pad_t, pad_l, h, w
                                  (2, 10, 7, 68, 7, 7, 2, 3, 3, 20, 14),        # the stem's 7x7/2, pad 3
                                  (2, 6, 6, 5, 5, 5, 2, 1, 2, 12, 11),          # Keras 'same' with asymmetric padding
                                  (2, 8, 8, 4, 1, 1, 1, 0, 0, 8, 8), (1, 4, 5, 3, 3, 3, 1, 0, 0, 6, 7)])   # no padding
def test_tap_border_sums_against_brute_force(dev, geom):
    """embnet_tap_border_sums: taps[r,s,k] = - sum of dy over the pixels whose tap (r,s) falls into the padding (row
    sums + column sums - corners of the border strips), for any stride / asymmetric padding / channel count; without
    padding every entry is zero."""
    from embeddingnet_amd import _lib
    from embeddingnet_amd.layers import workspace
    n, oh, ow, k, r, s, stride, pt, pl, h, w = geom
    rs = np.random.RandomState(4)
    dy = rs.randn(n, oh, ow, k).astype(np.float32)
    want = np.zeros((r, s, k))
    for rr in range(r):
        for ss in range(s):
            for y in range(oh):
                for x in range(ow):
                    ih, iw = y * stride + rr - pt, x * stride + ss - pl
                    if not (0 <= ih < h and 0 <= iw < w):
                        want[rr, ss] -= dy[:, y, x, :].astype(np.float64).sum(0)
    lib = _lib.lib()
    d = g(dy, dev)
    taps = torch.full((r, s, k), 7.0, device=dev)
    ws = workspace(max(lib.embnet_tap_border_sums_workspace_bytes(n, oh, ow, k, r, s, stride, pt, pl, h, w), 16), dev)
    _lib.check(lib.embnet_tap_border_sums(_lib.ptr(d), n, oh, ow, k, r, s, stride, pt, pl, h, w, _lib.ptr(taps), _lib.ptr(ws),
                                          ws.numel() * 4, _lib.stream()))
    got = taps.cpu().double().numpy()
    assert np.abs(got - want).max() <= 1e-5 * max(np.abs(want).max(), 1.0), (got - want)


def test_conv2d_split_arithmetic_extreme_magnitudes(dev):
    """The bf16 pieces of the conv kernels' operand split keep fp32's exponent range: activations around 1e-30 and
    weights around 1e+25 (products around 1e-5), and the reverse, come out as accurately as ordinary magnitudes; zeros
    and negative zeros stay exact.  (An infinite operand gives NaN, not inf: inf - inf in the split — documented.)"""
    from embeddingnet_amd import layers as L
    rs = np.random.RandomState(9)
    layer = L.Conv2D(64, 64, 3, padding=1, use_bias=False).to(dev)
    for sx, sw in ((1e-30, 1e25), (1e25, 1e-30), (1.0, 1.0)):
        x = (rs.randn(2, 10, 10, 64) * sx).astype(np.float32)
        x[0, :3] = 0.0
        x[1, 5] = -0.0
        w = (rs.randn(3, 3, 64, 64) * sw).astype(np.float32)
        with torch.no_grad():
            layer.kernel.copy_(g(w, dev))
        y = layer(g(x, dev)).detach().cpu().double().numpy()
        ref = F.conv2d(torch.tensor(x, dtype=torch.float64).permute(0, 3, 1, 2), torch.tensor(w, dtype=torch.float64).permute(3, 2, 0, 1),
                       padding=1).permute(0, 2, 3, 1).numpy()
        mag = F.conv2d(torch.tensor(np.abs(x), dtype=torch.float64).permute(0, 3, 1, 2),
                       torch.tensor(np.abs(w), dtype=torch.float64).permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1).numpy()
        assert np.isfinite(y).all()
        assert (np.abs(y - ref) / np.maximum(mag, 1e-300)).max() <= 1e-6, (sx, sw)
    with torch.no_grad():
        layer.kernel.zero_()
    assert torch.count_nonzero(layer(g(x, dev))) == 0
