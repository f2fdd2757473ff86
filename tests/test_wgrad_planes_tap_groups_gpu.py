"""Addressing of the planes weight gradient's wave roles (csrc/conv_wgrad_planes.hip), through the C ABI.

A wave of the kernel owns one 32-channel block, BOTH 32-filter blocks of the 64 x 64 tile, one half of the stage's positions
and one tap GROUP (taps 0-4 or 5-8); its half sums meet the other half's in LDS.  Every one of these indices selects an
address — of a fragment, of an accumulator's place in the half-sum buffer, of an output row — so each is tested by itself:

  * one-hot operands: one non-zero pixel and channel of x, one non-zero pixel and filter of dy, a tap (r, s) apart: exactly ONE
    element of dW is non-zero and it is their product — for all nine taps, a channel of each 32-block, a filter of each 32-block
    of every 64-wide tile;
  * small-integer operands (|v| <= 3: products and sums are exact in fp32 and in both plane formats), equal to a float64
    gradient: two channel tiles; >= 9 stages per split (the x ring wraps); a halo of four blocks with slabs — the library's
    slab sum and the slabs summed in order on the host;
  * the same call twice gives the same bits.

The process runs one plane format (two fp16 pieces by default); the last test runs this file's one-hot and small-integer
cases in a child process on the other (three bf16 pieces), whose kernel is an instantiation of its own.

Reference behaviour being matched: the kernel gradient of keras Conv2D(3x3, padding 1 after ZeroPadding2D) inside
image-classifiers' ResNet (reference embedding_net/backbones.py:99-104).
"""
import os
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_wgrad_planes_gpu import wgrad_planes  # noqa: E402   (planes of both operands, workspace, the C ABI call)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    return torch.device("cuda", 0)


def splits_of(n, h, w, c, k):
    return _lib.lib().embnet_conv2d_wgrad_planes_splits(n, h, w, c, k)


def wgrad64_dev(x, dy):
    """float64 dW[r,s,c,k] = sum_{n,oh,ow} x[n, oh+r-1, ow+s-1, c] dy[n, oh, ow, k] (zero padding): nine matrix products on the
    device.  Exact for the small-integer operands of this file in any summation order (every partial sum is an integer < 2^53)."""
    n, h, w, c = x.shape
    xp = torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1))
    d = dy.double().reshape(n * h * w, -1)
    out = torch.empty(3, 3, c, d.shape[1], dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            out[r, s] = xp[:, r:r + h, s:s + w, :].reshape(n * h * w, c).t() @ d
    return out


# ---- one-hot addressing ---------------------------------------------------------------------------------------------------------

ONE_HOT_SHAPES = [(1, 3, 3, 64, 64),       # one stage; every tap's window touches the padding
                  (2, 5, 7, 64, 128)]      # two filter tiles, a non-square pitch, three stages


@pytest.mark.parametrize("tap", range(9))
@pytest.mark.parametrize("n,h,w,c,k", ONE_HOT_SHAPES)
def test_one_hot_operands_address_one_element(dev, n, h, w, c, k, tap):
    r, s = divmod(tap, 3)
    assert splits_of(n, h, w, c, k) == 1
    img = n - 1
    oy, ox = (1, 1) if h == 3 else (1 + (r + s) % 3, 1 + (2 * r + s) % 5)      # the dy pixel; x's lies (r - 1, s - 1) from it
    iy, ix = oy + r - 1, ox + s - 1
    assert 0 <= iy < h and 0 <= ix < w
    for ch in (5, 37):                                         # a channel of each 32-block
        for f in [t + o for t in range(0, k, 64) for o in (3, 35)]:            # a filter of each 32-block of every tile
            x = torch.zeros(n, h, w, c, device=dev)
            dy = torch.zeros(n, h, w, k, device=dev)
            x[img, iy, ix, ch] = 1.5
            dy[img, oy, ox, f] = -2.5
            dw, _ = wgrad_planes(x, dy)
            nz = torch.nonzero(dw).cpu().tolist()
            assert nz == [[r, s, ch, f]], (tap, ch, f, nz[:8])
            assert dw[r, s, ch, f].item() == -3.75


# ---- small integers: exact sums ----------------------------------------------------------------------------------------------------

INT_GEOMS = [  # n, h, w, c, k, splits
    (3, 8, 8, 128, 64, 2),        # two channel tiles
    (8, 14, 14, 512, 512, 4),     # 57 stages in splits of 15: the ring of 8 blocks wraps
    (4, 56, 56, 256, 256, 16),    # a halo of four blocks (the ring exactly full), 16 slabs
]


@pytest.mark.parametrize("n,h,w,c,k,splits", INT_GEOMS)
def test_small_integer_operands_are_exact(dev, n, h, w, c, k, splits):
    assert splits_of(n, h, w, c, k) == splits
    g = torch.Generator(device=dev).manual_seed(100 * n + h)
    x = torch.randint(-3, 4, (n, h, w, c), device=dev, generator=g).float()
    dy = torch.randint(-3, 4, (n, h, w, k), device=dev, generator=g).float()
    ref = wgrad64_dev(x, dy)
    assert ref.abs().max().item() > 0
    dw, _ = wgrad_planes(x, dy, reduce=1)                      # the library's fixed-order slab sum
    assert torch.equal(dw.double(), ref)
    raw, ws = wgrad_planes(x, dy, reduce=0)                    # the slabs, summed in order on the host
    assert torch.isnan(raw).all()                              # dw untouched
    slabs = ws[: splits * 9 * c * k].cpu().numpy().reshape(splits, 3, 3, c, k)
    total = slabs[0].copy()
    for i in range(1, splits):
        total += slabs[i]
    assert np.array_equal(total.astype(np.float64), ref.cpu().numpy())


# ---- determinism -----------------------------------------------------------------------------------------------------------------

def test_same_call_twice_same_bits(dev):
    n, h, w, c, k = 6, 14, 14, 128, 128
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(n, h, w, c, device=dev, generator=g)
    dy = torch.randn(n, h, w, k, device=dev, generator=g)
    assert splits_of(n, h, w, c, k) > 1
    a, wa = wgrad_planes(x, dy, reduce=1)
    b, wb = wgrad_planes(x, dy, reduce=1)
    assert torch.isfinite(a).all()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(wa.view(torch.int32), wb.view(torch.int32))            # slab by slab as well


# ---- the other plane format ------------------------------------------------------------------------------------------------------

def test_other_plane_format_in_a_child_process(dev):
    """The planes' format is read once per process: the one-hot and small-integer cases again with the other format's kernel."""
    import subprocess
    other = "0" if os.environ.get("EMBNET_PLANES_F16", "1") != "0" else "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "tests/test_wgrad_planes_tap_groups_gpu.py",
                        "-k", "one_hot or small_integer"], cwd=root, env=dict(os.environ, EMBNET_PLANES_F16=other),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "21 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]
