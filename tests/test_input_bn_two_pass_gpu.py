"""embnet_bn_train_fwd_pad_ex: the BatchNormalization of a c-channel image batch (c % 4 != 0) written as cp = 4 ceil(c / 4) channels in
two passes over the image, against the four passes it replaces — embnet_pad_channels, then embnet_bn_train_fwd_ex on the padded copy
(statistics, finalize, apply).  Bit for bit: the output a, every statistics row (mean, rstd, scale, shift, bound, xhat), the range
word of a, and the moving statistics.  c = 3 and 1; n = 2 at 7x5 (m < 256: fewer rows than row lanes), 33x17, and 64x41
(m > 16 * 256: six row blocks, the last one ragged); the stem's own case (no gamma, no activation) and gamma + ReLU.
"""
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd._lib import check, ptr, stream

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 2e-5, 0.99


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run(dev, x, cp, gamma, beta, act, two_pass):
    lib = _lib.lib()
    n, h, w, c = x.shape
    m = n * h * w
    stats = torch.full((7, cp), 7.0, device=dev)
    mm, mv = torch.zeros(cp, device=dev), torch.ones(cp, device=dev)
    mm[:c], mv[:c] = 0.125, 0.75
    a = torch.full((n, h, w, cp), 7.0, device=dev)
    nbytes = lib.embnet_bn_workspace_bytes(m, cp)
    ws = torch.zeros((nbytes + 3) // 4, device=dev)
    row = [stats[i].data_ptr() for i in range(7)]
    if two_pass:
        check(lib.embnet_bn_train_fwd_pad_ex(ptr(x), m, c, cp, ptr(gamma), ptr(beta), EPS, MOMENTUM, act, ptr(a), row[0], row[1], row[2], row[3],
                                             ptr(mm), ptr(mv), ptr(ws), nbytes, row[4], row[5], row[6], stream()))
    else:
        xp = torch.full((n, h, w, cp), 7.0, device=dev)
        check(lib.embnet_pad_channels(ptr(x), m, c, cp, ptr(xp), stream()))
        check(lib.embnet_bn_train_fwd_ex(ptr(xp), m, cp, ptr(gamma), ptr(beta), EPS, MOMENTUM, act, ptr(a), row[0], row[1], row[2], row[3],
                                         ptr(mm), ptr(mv), None, 0, ptr(ws), nbytes, row[4], row[5], row[6], stream()))
    torch.cuda.synchronize()
    return a, stats, mm, mv


@pytest.mark.parametrize("with_gamma_relu", [False, True])
@pytest.mark.parametrize("h,w", [(7, 5), (33, 17), (64, 41)])
@pytest.mark.parametrize("c", [3, 1])
def test_two_passes_equal_pad_then_batchnorm(dev, c, h, w, with_gamma_relu):
    n, cp = 2, 4
    m = n * h * w
    assert (m < 256) == ((h, w) == (7, 5)) and (m > 16 * 256) == ((h, w) == (64, 41))
    g = torch.Generator(device=dev).manual_seed(100 * c + h)
    x = torch.rand((n, h, w, c), device=dev, generator=g) * torch.tensor([1.0, 0.5, 2.0][:c], device=dev) - 0.2
    beta = torch.zeros(cp, device=dev)
    beta[:c] = torch.tensor([0.3, -0.2, 0.1][:c], device=dev)
    gamma = None
    if with_gamma_relu:
        gamma = torch.ones(cp, device=dev)
        gamma[:c] = torch.tensor([1.5, -0.7, 0.9][:c], device=dev)
    act = 1 if with_gamma_relu else 0
    want = run(dev, x, cp, gamma, beta, act, two_pass=False)
    got = run(dev, x, cp, gamma, beta, act, two_pass=True)
    assert same_bits(want[0], got[0]), "a"
    assert bool((got[0][..., c:] == 0).all()), "a pad channel is not exactly 0"
    for i, name in enumerate(("mean", "rstd", "scale", "shift", "bound", "range", "xhat")):
        a, b = (want[1][i][:1], got[1][i][:1]) if name == "range" else (want[1][i], got[1][i])
        assert same_bits(a, b), name
    assert float(got[1][5][0]) >= float(got[0].abs().max()), "the range word is below max |a|"
    assert same_bits(want[2], got[2]) and same_bits(want[3], got[3]), "moving statistics"


def test_rejects_a_channel_count_that_needs_no_padding(dev):
    lib = _lib.lib()
    x = torch.zeros((2, 4), device=dev)
    s = torch.zeros((4, 4), device=dev)
    ws = torch.zeros(4096, device=dev)
    rc = lib.embnet_bn_train_fwd_pad_ex(ptr(x), 2, 4, 4, None, None, EPS, MOMENTUM, 0, ptr(x), s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(),
                                        s[3].data_ptr(), None, None, ptr(ws), ws.numel() * 4, None, None, None, stream())
    assert rc != 0
