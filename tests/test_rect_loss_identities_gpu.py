"""An identity of the margin-softmax rows of CosFace (ops.proxy_softmax_loss, csrc/proxy_loss.hip), SoftTriple (ops.soft_triple_loss)
and sub-centre ArcFace (ops.arcface_loss; both csrc/multi_proxy_loss.hip), pinned bit for bit: at one centre per class SoftTriple's
pooling is the identity and its logit is CosFace's, and at margin 0 ArcFace's phi(s) = fl(fl(s 1) - fl(r 0)) = s with phi' = 1, so
the three entry points must return the same loss, G, demb and proxy gradient on both forward paths.  Continuous inputs (nothing is
exact in any order): the identity is one of rounding order, not of exact sums.  Whoever merges the two row bodies can rely on it;
whoever changes one of them learns here that the other has to follow.

Nothing here is a tolerance: every comparison is torch.equal.
"""
import functools

import pytest
import torch

import proxy_ref as P
import recipes as R

pytestmark = pytest.mark.gpu
UP = 0.75
SCALE, MARGIN = 64.0, 0.35
# (proxy_ref shape, path): the ragged batch (17 rows, e = 64, c = 40, labels -1 and c among them), c = 70 > 64 (a lane owns two
# classes) with e = 33 (a tail), and c = 4000 on `matrix` only (15 class slices: demb's split product under both entry points)
CASES = [("ragged", "small"), ("ragged", "matrix"), ((5, 7, 33, 70), "small"), ((5, 7, 33, 70), "matrix"),
         ((4, 4, 96, 4000), "matrix")]
IDS = [f"{s if isinstance(s, str) else 'x'.join(map(str, s))}-{p}" for s, p in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    if shape == "ragged":
        e, c = P.RAGGED
        x, w, lab = P.ragged_inputs(R.clustered_embeddings(77, 5, 5, e, P.SIGMA), e, c, 77)
    else:
        p, k, e, c = shape
        x, w, lab = P.make_inputs(R.clustered_embeddings(P.seed_of(p, k, e), p, k, e, P.SIGMA), p, k, c, P.seed_of(p, k, e))
    for t in (x, w, lab):
        t.setflags(write=False)
    return x, w, lab


@functools.lru_cache(maxsize=None)
def _run(loss, shape, path, margin):
    """One forward + backward (upstream gradient 0.75) -> dict of device tensors; computed once per case, left unchanged."""
    from embeddingnet_amd import ops
    dev = torch.device("cuda:0")
    x, w, lab = _inputs(shape)
    c = w.shape[0]
    xt = torch.tensor(x, device=dev).requires_grad_(True)
    wt = torch.tensor(w, device=dev).requires_grad_(True)
    lt = torch.tensor(lab, device=dev)
    reg = None
    if loss == "cosface":
        mean, counts, g = ops.proxy_softmax_loss(xt, wt, lt, SCALE, margin, path=path, return_weights=True)
    elif loss == "soft_triple":
        mean, counts, reg, g = ops.soft_triple_loss(xt, wt, lt, c, SCALE, margin, gamma=0.1, tau=0.0, path=path, return_weights=True)
    else:
        mean, counts, g = ops.arcface_loss(xt, wt, lt, c, SCALE, margin, path=path, return_weights=True)
    mean.backward(torch.tensor(UP, device=dev))
    torch.cuda.synchronize()
    return dict(loss=mean.detach(), counts=counts, reg=reg, G=g, demb=xt.grad, dw=wt.grad)


def _same(a, b, what):
    for key in ("loss", "G", "demb", "dw"):
        assert a[key].shape == b[key].shape, (what, key)
        assert torch.isfinite(a[key]).all(), (what, key)
        assert torch.equal(a[key], b[key]), (what, key, float((a[key] - b[key]).abs().max()))


@pytest.mark.parametrize("shape,path", CASES, ids=IDS)
def test_cosface_is_soft_triple_at_one_centre(dev, shape, path):
    cf = _run("cosface", shape, path, MARGIN)
    st = _run("soft_triple", shape, path, MARGIN)
    _same(cf, st, "cosface / soft_triple")
    assert bool(cf["G"].any()) and bool(cf["demb"].any()) and bool(cf["dw"].any())
    cc, sc = cf["counts"].cpu().tolist(), st["counts"].cpu().tolist()
    print(f"{shape} {path}: loss {float(cf['loss']):.9g}, counts cosface {cc} soft_triple {sc}")
    assert cc[0] == sc[0] and cc[0] > 0                                  # labelled samples
    assert cc[2] == sc[1]                                                # violating samples
    assert float(st["reg"]) == 0.0 and not torch.signbit(st["reg"])      # no regulariser at one centre: exactly +0


@pytest.mark.parametrize("shape,path", CASES, ids=IDS)
def test_three_way_identity_at_margin_zero(dev, shape, path):
    cf = _run("cosface", shape, path, 0.0)
    st = _run("soft_triple", shape, path, 0.0)
    af = _run("arcface", shape, path, 0.0)
    _same(cf, st, "cosface / soft_triple")
    _same(cf, af, "cosface / arcface")
    assert bool(cf["G"].any())
    print(f"{shape} {path}: loss {float(cf['loss']):.9g}")
