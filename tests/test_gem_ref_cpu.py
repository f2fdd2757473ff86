"""GeM pooling without a GPU: the float64 reference (tests/gem_ref.py) against torch autograd of the textbook formula, the
maximum-normalised form against the naive one, the header, and the MODEL.pooling surface of get_backbone / parse_params."""
import os
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib
from embeddingnet_amd import backbones as B
from embeddingnet_amd import layers as L
from embeddingnet_amd.utils import check_pooling, parse_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gem_ref as G  # noqa: E402

EPS = 1e-6
CPU = torch.device("cpu")


def inputs(n=3, hw=11, c=6, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, hw, c).astype(np.float32)                 # zeros and negatives: the clamp is live
    x[0, 3, 1] = 0.0
    return x, rs.randn(n, c).astype(np.float32)


def torch_naive(x, p, dy):
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    pt = torch.tensor(np.asarray(p, np.float32), dtype=torch.float64, requires_grad=True)
    y = xt.clamp(min=float(np.float32(EPS))).pow(pt).mean(dim=1).pow(1.0 / pt)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    return y.detach().numpy(), xt.grad.numpy(), pt.grad.numpy()


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("p0", [1.0, 3.0, 6.5])
def test_reference_matches_torch_autograd(p0, per_channel):
    x, dy = inputs()
    p = np.float32(p0) + (np.arange(6, dtype=np.float32) * np.float32(0.25) if per_channel else np.zeros(1, np.float32))
    ref = G.gem(x, p, EPS, dy)
    y, dx, dp = torch_naive(x, p, dy)
    np.testing.assert_allclose(ref["y"], y, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref["dx"], dx, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(ref["dp"], dp, rtol=1e-9, atol=1e-15)
    assert ref["dp"].shape == (6 if per_channel else 1,)
    assert np.all(ref["dx"][x < np.float32(EPS)] == 0.0)
    for k in ("b_y", "b_dydp", "b_dx", "b_dp"):
        assert np.all(np.isfinite(ref[k])) and np.all(ref[k] >= 0)
    assert np.all(ref["b_y"] <= 1e-4 * ref["y"])              # the bound is a few hundred u at most, not vacuous


def test_p_one_is_the_mean():
    x = np.abs(inputs(seed=1)[0]) + np.float32(0.5)
    ref = G.gem(x, np.ones(1, np.float32), EPS)
    np.testing.assert_allclose(ref["y"], x.astype(np.float64).mean(axis=1), rtol=1e-14)


def test_constant_channel_has_no_exponent_gradient():
    x = np.full((2, 9, 4), 0.75, np.float32)
    ref = G.gem(x, np.full(1, 3.0, np.float32), EPS)
    assert np.all(ref["s"] == 1.0) and np.all(ref["t"] == 0.0) and np.all(ref["dydp"] == 0.0)
    np.testing.assert_allclose(ref["y"], 0.75, rtol=1e-15)


@pytest.mark.parametrize("amp", [1e-4, 1.0, 1e5])
def test_normalised_form_equals_naive_where_finite(amp):
    x = (np.abs(inputs(seed=2)[0]) * np.float32(amp)).astype(np.float32)
    for p0 in (1.0, 3.0, 6.5, 10.0):
        p = np.full(1, p0, np.float32)
        want = G.naive(x, p, EPS)
        assert np.all(np.isfinite(want))                      # float64 holds 1e5^10
        np.testing.assert_allclose(G.gem(x, p, EPS)["y"], want, rtol=1e-12)


def test_normalised_form_is_finite_where_naive_float32_overflows():
    x = (np.abs(inputs(seed=3)[0]) * np.float32(1e5) + np.float32(1e4)).astype(np.float32)
    p = np.full(1, 10.0, np.float32)
    assert not np.all(np.isfinite(G.naive(x, p, EPS, dtype=np.float32)))      # (1e5)^10 = 1e50 > 3.4e38
    ref = G.gem(x, p, EPS, np.ones((3, 6), np.float32))
    for k in ("y", "dydp", "dx", "dp", "b_y", "b_dydp", "b_dx", "b_dp"):
        assert np.all(np.isfinite(ref[k])), k
    # every intermediate of the normalised form is an fp32 number: r, e in (0, 1], y within [eps, max]
    assert np.all(ref["y"] <= x.max(axis=1)) and np.all(ref["y"] >= x.max(axis=1) * (1.0 / 11) ** 0.1 * (1 - 1e-12))


def test_header_declares_gem_and_abi_is_22():
    protos = _lib.parse_header()
    for name, nargs in (("embnet_gem_fwd", 10), ("embnet_gem_bwd", 15), ("embnet_gem_bwd_workspace_bytes", 1)):
        assert name in protos and len(protos[name][1]) == nargs, name
    assert "#define EMBNET_ABI_VERSION 22" in open(_lib.HEADER_PATH).read()


@pytest.mark.parametrize("bad, key", [
    ("max", "type"), ({"type": "mac"}, "type"), ({"p": 3.0}, "type"), ({"type": "gem", "power": 3}, "power"),
    ({"type": "gem", "p": "3"}, "p"), ({"type": "gem", "p": 0}, "p"), ({"type": "gem", "p": True}, "p"),
    ({"type": "gem", "eps": -1.0}, "eps"), ({"type": "gem", "learnable": 1}, "learnable"),
    ({"type": "gem", "per_channel": "yes"}, "per_channel"), ({"type": "avg", "p": 3.0}, "p"), (3.0, "pooling")])
def test_pooling_is_refused_by_key(bad, key):
    with pytest.raises(ValueError, match=key):
        check_pooling(bad, "resnet18")
    with pytest.raises(ValueError, match=key):
        B.get_backbone((64, 64, 3), encodings_len=32, backbone_name="resnet18", backbone_weights=None, device=CPU, pooling=bad)


@pytest.mark.parametrize("backbone", ["simple", "simple2"])
def test_gem_is_refused_where_the_head_does_not_pool(backbone, tmp_path):
    with pytest.raises(ValueError, match=backbone):
        B.get_backbone((64, 64, 3), encodings_len=32, backbone_name=backbone, backbone_weights=None, device=CPU, pooling="gem")
    assert check_pooling("avg", backbone) is None and check_pooling({"type": "avg"}, backbone) is None
    B.get_backbone((64, 64, 3), encodings_len=32, backbone_name="simple2", backbone_weights=None, device=CPU, pooling="avg")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "configs", "simple2_synthetic.yml")).read()
    assert "backbone_name : 'simple2'" in text or "backbone_name: 'simple2'" in text
    cfg = tmp_path / "bad.yml"
    cfg.write_text(text.replace("MODEL:\n", "MODEL:\n  pooling : 'gem'\n", 1))
    with pytest.raises(ValueError, match="simple2"):
        parse_params(str(cfg))
    cfg.write_text(text.replace("MODEL:\n", "MODEL:\n  pooling : {type: gem, exponent: 3}\n", 1))
    with pytest.raises(ValueError, match="exponent"):
        parse_params(str(cfg))


def test_shipped_gem_config_parses():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    params = parse_params(os.path.join(root, "configs", "resnet18_gem_synthetic.yml"))
    assert params["model"]["pooling"] == "gem" and params["model"]["backbone_name"] == "resnet18"
    plain = parse_params(os.path.join(root, "configs", "resnet18_synthetic.yml"))
    params["model"].pop("pooling")
    assert params["model"] == plain["model"] and params["generator"] == plain["generator"]


def test_avg_is_the_default_head_and_gem_replaces_one_layer():
    kw = dict(encodings_len=32, backbone_name="resnet18", backbone_weights=None, device=CPU, seed=3)
    default, _ = B.get_backbone((64, 64, 3), **kw)
    avg, _ = B.get_backbone((64, 64, 3), pooling="avg", **kw)
    assert [k for k, _ in default.named_modules()] == [k for k, _ in avg.named_modules()]
    wd, wa = B.keras_weights(default), B.keras_weights(avg)
    assert list(wd) == list(wa) and all(torch.equal(wd[k], wa[k]) for k in wd)
    assert isinstance(default.net.head.gap, L.GlobalAveragePooling2D) and default.net.head._order[0] == "gap"

    gem, _ = B.get_backbone((64, 64, 3), pooling="gem", **kw)
    wg = B.keras_weights(gem)
    assert set(wg) - set(wd) == {"gem/p"} and set(wd) <= set(wg)
    assert all(torch.equal(wd[k], wg[k]) for k in wd)         # the same initial weights everywhere else
    layer = gem.net.head.gem
    assert gem.net.head._order[:3] == ["gem", "dense1", "dense2"] and not hasattr(gem.net.head, "gap")
    assert isinstance(layer.p, torch.nn.Parameter) and layer.p.shape == (1,) and float(layer.p.detach()) == 3.0 and layer.eps == 1e-6
    spec = {"type": "gem", "p": 4.5, "eps": 1e-5, "learnable": False, "per_channel": True}
    frozen, _ = B.get_backbone((64, 64, 3), pooling=spec, **kw)
    layer = frozen.net.head.gem
    assert layer.p.shape == (512,) and not isinstance(layer.p, torch.nn.Parameter) and float(layer.p[7]) == 4.5
    assert "gem/p" in B.keras_weights(frozen) and all(q is not layer.p for q in frozen.parameters())
    with pytest.raises(KeyError, match="gem/p"):              # a file of the average-pooling model lacks the exponent
        B.load_keras_weights(gem, {k: v.detach().numpy() for k, v in wd.items()}, strict=True)


def test_layer_refuses_bad_arguments():
    for kw in (dict(p=0.0), dict(p=-1.0), dict(p="3"), dict(eps=0.0), dict(per_channel=True), dict(per_channel=True, channels=0)):
        with pytest.raises(ValueError):
            L.GeM(**kw)
    assert L.GeM(per_channel=True, channels=8).p.shape == (8,)
