"""The opt-in for more than 64 KB of dynamic LDS holds per (kernel, device) (csrc/common.h allow_big_lds): after a process has run
a kernel family on device 0, the same call on device 1 opts that kernel in there too.  One supported geometry through every family
whose launch asks for more than 64 KB — patch 3x3, planes 1x1, DMA 1x1, the stem, the planes weight gradient, the depthwise tile
forward and weight gradient, the SE MLP forward and backward — through the C ABI, first on device 0, then on device 1, from the same
host operands: bitwise equal results.  A launch without the opt-in does not run: embnet's check_launch reports it as an error code,
which _lib.check raises.

Dynamic LDS of the geometries below (bytes; the default launch limit is 65 536): patch 3x3 at 128 output channels >= 73 728 of
kernel slots alone; both 1x1 kernels 147 456; stem and planes weight gradient fixed at ~155 KB; depthwise 5x5 on 28x28x48 runs in
14-row bands, 2 x 32 768 of tile + the taps; SE MLP forward / backward A 73 728 + 8 (c + JP), backward B (32 + 2 s) x 272 = 78 336
at s = 128.
"""
import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd import layers as L

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs in one process")]


def slot_for(t):
    return t.detach().abs().max().reshape(1).float().view(torch.int32).clone()


def planes_of(x):
    c = x.shape[-1]
    p = torch.zeros(3 * x.numel(), device=x.device, dtype=torch.int16)
    _lib.check(_lib.lib().embnet_planes_from_f32(x.data_ptr(), x.numel() // c, c, p.data_ptr(), _lib.stream()))
    return p


def run_families(dev):
    """Every family once on `dev` (the current device while it runs) -> {family: results on the host}."""
    lib = _lib.lib()
    rs = np.random.RandomState(11)
    t = lambda *shape, s=1.0: torch.from_numpy((rs.standard_normal(shape) * s).astype(np.float32)).to(dev)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    ws_of = lambda nbytes: torch.empty(max(nbytes // 4, 4), device=dev)
    out = {}
    with torch.cuda.device(dev):
        # patch 3x3 (stride 1, pad 1) and the two 1x1 kernels
        n, h, c, k = 4, 28, 64, 128
        x, w3, w1 = t(n, h, h, c), t(3, 3, c, k, s=0.05), t(1, 1, c, k, s=0.1)
        xp = planes_of(x)
        assert lib.embnet_conv2d_patch_supported(n, c, 3, 3, k, 1, h, h) == 1
        y, ws = nan(n, h, h, k), ws_of(lib.embnet_conv2d_patch_workspace_bytes(n, c, 3, 3, k, h, h))
        _lib.check(lib.embnet_conv2d_patch_f32(xp.data_ptr(), L.weight_planes(w3, 0).data_ptr(), None, y.data_ptr(), n, h, h, c, 3, 3, k, 1, 1,
                                               h, h, 0, None, None, ws.data_ptr(), ws.numel() * 4, _lib.stream()))
        out["patch 3x3"] = [y]
        assert lib.embnet_conv2d_patch_supported(n, c, 1, 1, k, 1, h, h) == 1 and lib.embnet_conv2d_dma1x1_supported(n, h, h, c, k, 1, h, h) == 1
        y1, y2, ws = nan(n, h, h, k), nan(n, h, h, k), ws_of(lib.embnet_conv2d_patch_workspace_bytes(n, c, 1, 1, k, h, h))
        _lib.check(lib.embnet_conv2d_planes1x1_f32(xp.data_ptr(), L.weight_planes(w1, 0).data_ptr(), None, y1.data_ptr(), n, h, h, c, k, 1, h, h,
                                                   0, None, None, ws.data_ptr(), ws.numel() * 4, _lib.stream()))
        out["planes 1x1"] = [y1]
        rng = slot_for(x)
        _lib.check(lib.embnet_conv2d_dma1x1_f32(x.data_ptr(), L.weight_planes(w1, 0).data_ptr(), None, y2.data_ptr(), n, h, h, c, k, 1, h, h,
                                                0, None, None, rng.data_ptr(), ws.data_ptr(), ws.numel() * 4, _lib.stream()))
        out["DMA 1x1"] = [y2]

        # stem: 7x7 stride 2 on the image padded to four channels
        n, h, pad = 3, 64, 3
        oh = (h + 2 * pad - 7) // 2 + 1
        xs, wst = t(n, h, h, 4), t(7, 7, 4, 64, s=0.08)
        xs[..., 3] = 0
        wst[:, :, 3, :] = 0
        assert lib.embnet_conv2d_stem_supported(n, h, h, 4, 7, 7, 64, 2, pad, pad, oh, oh) == 1
        ys, rx, rw = nan(n, oh, oh, 64), slot_for(xs), slot_for(wst)
        _lib.check(lib.embnet_conv2d_stem_f32(xs.data_ptr(), wst.data_ptr(), ys.data_ptr(), n, h, h, pad, pad, oh, oh, None, rx.data_ptr(),
                                              rw.data_ptr(), _lib.stream()))
        out["stem"] = [ys]

        # planes weight gradient of a 3x3 stride-1 conv
        n, h, c, k = 4, 28, 128, 128
        assert lib.embnet_conv2d_wgrad_planes_supported(n, h, h, c, 3, 3, k, 1, 1, 1, h, h) == 1
        xg, dyg = planes_of(t(n, h, h, c)), planes_of(t(n, h, h, k, s=1e-3))
        dw, ws = nan(3, 3, c, k), ws_of(lib.embnet_conv2d_wgrad_planes_workspace_bytes(n, h, h, c, k))
        _lib.check(lib.embnet_conv2d_wgrad_planes_f32(xg.data_ptr(), dyg.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel() * 4, n, h, h, c, k,
                                                      1, _lib.stream()))
        out["planes weight gradient"] = [dw]

        # depthwise 5x5 on the LDS tile: forward and weight gradient
        n, h, c, ks = 3, 28, 48, 5
        xd, wd, dyd = t(n, h, h, c), t(ks, ks, c, 1, s=0.3), t(n, h, h, c)
        yd, dwd = nan(n, h, h, c), nan(ks, ks, c, 1)
        traced = dev.index == 0                     # (the trace's event pool belongs to the device that filled it: device 0 only)
        _lib.trace_reset(); _lib.trace_enable(traced)
        try:
            _lib.check(lib.embnet_dwconv2d_fwd_f32(xd.data_ptr(), wd.data_ptr(), yd.data_ptr(), n, h, h, c, ks, ks, 1, 2, 2, h, h, _lib.stream()))
            ws = ws_of(lib.embnet_dwconv2d_wgrad_workspace_bytes(n, c, ks, ks, h, h))
            _lib.check(lib.embnet_dwconv2d_wgrad_f32(xd.data_ptr(), dyd.data_ptr(), dwd.data_ptr(), ws.data_ptr(), ws.numel() * 4, n, h, h, c,
                                                     ks, ks, 1, 2, 2, h, h, _lib.stream()))
            torch.cuda.synchronize()
            names = [r[0] for r in _lib.trace_records()]
        finally:
            _lib.trace_enable(False)
        if traced:                                  # the tile kernels ran, not the row kernels (the plan is the same on every device)
            assert names[0] == "embnet::dwt::dw_tile_kernel" and "dw_tile_wgrad" in names[1], names
        out["depthwise tile forward"], out["depthwise tile weight gradient"] = [yd], [dwd]

        # SE MLP: forward, and the two backward launches
        n, c, s = 9, 2048, 128
        assert lib.embnet_se_mlp_supported(n, c, s)
        pooled, w1s, b1, w2s, b2 = t(n, c), t(c, s, s=0.02), t(s, s=0.1), t(s, c, s=0.1), t(c, s=0.1)
        z1, gate = nan(n, s), nan(n, c)
        _lib.check(lib.embnet_se_mlp_fwd(pooled.data_ptr(), w1s.data_ptr(), b1.data_ptr(), w2s.data_ptr(), b2.data_ptr(), n, c, s, z1.data_ptr(),
                                         gate.data_ptr(), _lib.stream()))
        out["SE MLP forward"] = [z1, gate]
        dgate = t(n, c)
        dz1, dpooled, dw1, db1, dw2, db2 = nan(n, s), nan(n, c), nan(c, s), nan(s), nan(s, c), nan(c)
        _lib.check(lib.embnet_se_mlp_bwd(dgate.data_ptr(), gate.data_ptr(), z1.data_ptr(), pooled.data_ptr(), w1s.data_ptr(), w2s.data_ptr(), n, c,
                                         s, dz1.data_ptr(), dpooled.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(),
                                         _lib.stream()))
        out["SE MLP backward"] = [dpooled, dw1, db1, dw2, db2]
        torch.cuda.synchronize()
        return {name: [r.cpu() for r in res] for name, res in out.items()}


def test_every_big_lds_family_on_a_second_device_after_the_first():
    if _lib.lib().embnet_conv_planes_mfma_terms() != 3:
        pytest.skip("built for the two-piece fp16 planes format")
    first = run_families(torch.device("cuda", 0))
    second = run_families(torch.device("cuda", 1))
    assert list(first) == list(second) and len(first) == 9
    for name in first:
        for a, b in zip(first[name], second[name]):
            assert torch.isfinite(a).all(), name
            assert torch.equal(a, b), name
