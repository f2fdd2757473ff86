"""SoftTriple and sub-centre ArcFace, host side (no GPU): the C ABI is declared and exported and refuses arguments outside its range
before any launch; the path rule and the workspace size are restated; the float64 restatement in tests/multi_proxy_ref.py agrees with
torch autograd of the textbook formulas, with central differences and with cases worked by hand; the Python layers know the modes;
and the inputs of tests/test_multi_proxy_loss_gpu.py are fit for what that test asserts on them (the caps on open decisions)."""
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import multi_proxy_ref as M
import proxy_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_multi_proxy_loss_path", "embnet_multi_proxy_loss_workspace_bytes", "embnet_multi_proxy_loss_fwd",
       "embnet_multi_proxy_loss_bwd")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced
KINDS = list(M.KINDS)
CODE = {"soft_triple": 1, "arcface": 2}


def _lib():
    from embeddingnet_amd import _lib
    return _lib.lib()


def _train():
    spec = importlib.util.spec_from_file_location("embnet_tools_train", os.path.join(ROOT, "tools", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    return train


# ---------------------------------------------------------------------------------------------------------------- 1. the ABI
def test_header_declares_and_library_exports_the_entries():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    for name in NEW:
        assert name in protos and name in exported, name
    assert len(protos["embnet_multi_proxy_loss_fwd"][1]) == 22 and len(protos["embnet_multi_proxy_loss_bwd"][1]) == 15
    assert _lib.lib().embnet_abi_version() == 22


FWD_PTRS = ["emb", "centres", "labels", "g", "q", "counts", "mean", "reg", "ws"]
BWD_PTRS = ["emb", "centres", "g", "q", "demb", "dcentres", "ws"]


def _fwd(n, c, kc, e, kind=1, a=20.0, b=0.01, gam=0.1, tau=0.2, ws=FAKE, ws_bytes=1 << 40, path=0, null=None, h=FAKE):
    l = _lib()
    p = {k: FAKE for k in FWD_PTRS}
    p["ws"] = ws
    if null:
        p[null] = None
    rc = l.embnet_multi_proxy_loss_fwd(p["emb"], p["centres"], p["labels"], n, c, kc, e, kind, a, b, gam, tau, path, p["g"], p["q"], h,
                                       p["counts"], p["mean"], p["reg"], p["ws"], ws_bytes, None)
    return rc, l.embnet_last_error().decode()


def _bwd(n, c, kc, e, ws=FAKE, ws_bytes=1 << 40, null=None):
    l = _lib()
    p = {k: FAKE for k in BWD_PTRS}
    p["ws"] = ws
    if null:
        p[null] = None
    rc = l.embnet_multi_proxy_loss_bwd(p["emb"], p["centres"], n, c, kc, e, p["g"], p["q"], None, None, p["demb"], p["dcentres"],
                                       p["ws"], ws_bytes, None)
    return rc, l.embnet_last_error().decode()


@pytest.mark.parametrize("null", FWD_PTRS)
def test_fwd_rejects_null_pointers(null):
    rc, msg = _fwd(32, 24, 3, 256, null=null)
    assert rc == -1 and "multi_proxy_loss_fwd: null pointer" in msg
    rc, msg = _fwd(32, 24, 3, 256, h=None)                   # the regulariser's H where there is a regulariser
    assert rc == -1 and "null pointer (reg_h" in msg


@pytest.mark.parametrize("null", BWD_PTRS)
def test_bwd_rejects_null_pointers(null):
    rc, msg = _bwd(32, 24, 3, 256, null=null)
    assert rc == -1 and "multi_proxy_loss_bwd: null pointer" in msg


@pytest.mark.parametrize("n,c,kc,e,what", [(1, 24, 3, 64, "n=1"), (4097, 24, 3, 64, "n=4097"), (32, 1, 3, 64, "c=1"),
                                           (32, 24, 0, 64, "kc=0"), (32, 24, 33, 64, "kc=33"), (32, 8193, 2, 64, "c*kc=16386"),
                                           (32, 16385, 1, 64, "c*kc=16385"), (32, 24, 3, 0, "e=0"), (32, 24, 3, 4097, "e=4097"),
                                           (-5, 24, 3, 64, "n=-5"), (32, 2 ** 30, 4, 64, "c*kc=4294967296")])
def test_both_reject_out_of_range_shapes(n, c, kc, e, what):
    for call, name in ((_fwd, "multi_proxy_loss_fwd"), (_bwd, "multi_proxy_loss_bwd")):
        rc, msg = call(n, c, kc, e)
        assert rc == -1 and what in msg and msg.startswith(name), msg
    assert _lib().embnet_multi_proxy_loss_path(n, c, kc, e) == 0 and _lib().embnet_multi_proxy_loss_workspace_bytes(n, c, kc, e) == 0
    assert M.auto_path(n, c, kc, e) is None and M.workspace_bytes(n, c, kc, e) == 0


def test_fwd_rejects_bad_scalars_kinds_paths_and_workspaces():
    bad = [math.nan, math.inf, -math.inf]
    for kind in (0, 3, -1):
        assert "unknown kind" in _fwd(32, 24, 3, 256, kind=kind)[1]
    for kind in (1, 2):
        for a in [0.0, -1.0] + bad:
            rc, msg = _fwd(32, 24, 3, 256, kind=kind, a=a)
            assert rc == -1 and "scale" in msg, msg
        for b in bad:
            rc, msg = _fwd(32, 24, 3, 256, kind=kind, b=b)
            assert rc == -1 and "margin" in msg, msg
    for g in [0.0, -0.1] + bad:
        assert "gamma" in _fwd(32, 24, 3, 256, gam=g)[1]
    for t in [-0.1] + bad:
        assert "tau" in _fwd(32, 24, 3, 256, tau=t)[1]
    assert _fwd(32, 24, 3, 256, tau=0.0, h=None, null="emb")[1].endswith("null pointer")      # tau = 0: in range, no H needed
    assert _fwd(32, 24, 3, 256, b=-0.5, null="emb")[1].endswith("null pointer")               # SoftTriple: a negative delta is in range
    for m in (-0.01, math.pi / 2, float(np.float32(math.pi / 2)), 2.0):
        rc, msg = _fwd(32, 24, 3, 256, kind=2, b=m)
        assert rc == -1 and "margin" in msg and "pi/2" in msg, msg
    assert _fwd(32, 24, 3, 256, kind=2, b=1.5, gam=math.nan, tau=-1.0, h=None, null="emb")[1].endswith("null pointer")  # ArcFace ignores both
    need = _lib().embnet_multi_proxy_loss_workspace_bytes(32, 24, 3, 256)
    for call, name in ((_fwd, "multi_proxy_loss_fwd"), (_bwd, "multi_proxy_loss_bwd")):
        rc, msg = call(32, 24, 3, 256, ws_bytes=need - 16)
        assert rc == -3 and "workspace" in msg and msg.startswith(name)
        rc, msg = call(32, 24, 3, 256, ws=FAKE + 4)
        assert rc == -1 and "16-byte aligned" in msg and msg.startswith(name)
    for path in (3, -1):
        assert "unknown path" in _fwd(32, 24, 3, 256, path=path)[1]
    rc, msg = _fwd(16, 1367, 3, 96, path=1)                  # e + c kc = 4197: only the matrix path
    assert rc == -1 and "small path" in msg


def test_path_rule_and_workspace_size_restated():
    l = _lib()
    shapes = [(p * k, c, kc, e) for p, k, c, kc, e in M.SHAPES] + [(17, M.RAGGED[1], M.RAGGED[2], M.RAGGED[0]), (2, 2, 1, 1),
                                                                   (4096, 512, 32, 4096), (4096, 2, 1, 1), (2, 1365, 3, 1),
                                                                   (2, 4095, 1, 1), (2, 4096, 1, 1), (512, 100, 10, 256), (32, 100, 10, 512),
                                                                   (128, 1024, 4, 128)]
    for n, c, kc, e in shapes:
        assert l.embnet_multi_proxy_loss_path(n, c, kc, e) == {"small": 1, "matrix": 2}[M.auto_path(n, c, kc, e)], (n, c, kc, e)
        assert l.embnet_multi_proxy_loss_workspace_bytes(n, c, kc, e) == M.workspace_bytes(n, c, kc, e) >= 4 * n * c * kc + 8 * c * kc * e
    for p, k, c, kc, e in M.SMALL_SHAPES:                    # they fit the small path; `auto` takes it below 100 centres
        assert M.fits_small(p * k, c, kc, e) and l.embnet_multi_proxy_loss_path(p * k, c, kc, e) == (1 if c * kc < 100 else 2)
        assert not _fwd(p * k, c, kc, e, path=1, null="emb")[1].endswith("small path")
    for p, k, c, kc, e in M.MATRIX_SHAPES:
        assert not M.fits_small(p * k, c, kc, e) and l.embnet_multi_proxy_loss_path(p * k, c, kc, e) == 2
        assert _fwd(p * k, c, kc, e, path=1)[1].endswith("small path")
    assert [M.auto_path(32, 33, 3, 256), M.auto_path(32, 50, 2, 256), M.auto_path(32, 99, 1, 256)] == ["small", "matrix", "small"]


# ---------------------------------------------------------------------------------------------------------------- 2. the layers
def test_python_layers_know_the_modes():
    from embeddingnet_amd import losses_and_accuracies, ops
    from embeddingnet_amd.datagenerators import TripletsDataGenerator
    from embeddingnet_amd.proxies import ProxyHead
    from embeddingnet_amd.train_step import ProxyTrainer
    assert ops.MULTI_PROXY_LOSS_MODES["soft_triple"] == (ops.soft_triple_loss, ("scale", "margin", "gamma", "tau", "centers"))
    assert ops.MULTI_PROXY_LOSS_MODES["arcface"] == (ops.arcface_loss, ("scale", "margin", "centers"))
    for mode in ops.MULTI_PROXY_LOSS_MODES:
        assert mode in TripletsDataGenerator.STEP_ONLY_MODES and mode in ProxyTrainer.LOSS_PARAMS
    head = ProxyHead(6, 16, seed=3, centers_per_class=4)
    assert head.proxies.shape == (24, 16) and head.n_classes == 6 and head.centers_per_class == 4
    one = ProxyHead(6, 16, seed=3)
    assert one.centers_per_class == 1 and one.n_classes == 6
    gen = torch.Generator(device="cpu").manual_seed(3)       # centers_per_class = 1 draws what it always drew
    assert torch.equal(one.proxies.detach(), torch.randn(6, 16, generator=gen, dtype=torch.float32) * math.sqrt(2.0 / 6))
    assert torch.equal(ProxyHead(6, 16, seed=3, centers_per_class=1).proxies, one.proxies)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="centers_per_class"):
            ProxyHead(6, 16, centers_per_class=bad)
    assert callable(losses_and_accuracies.soft_triple_loss(head, 20.0, 0.01, 0.1, 0.2))
    assert callable(losses_and_accuracies.arcface_loss(head, 64.0, 0.5))
    opt = torch.optim.SGD([head.proxies], lr=0.1)
    ident = torch.nn.Identity()
    tr = ProxyTrainer(ident, head, opt, loss="soft_triple", loss_params=dict(scale=10.0, centers=4))
    assert tr.mode == "soft_triple" and tr.loss_params == dict(scale=10.0)
    assert ProxyTrainer(ident, head, opt, loss="arcface").loss_params == {}
    with pytest.raises(ValueError, match="centers_per_class"):
        ProxyTrainer(ident, head, opt, loss="arcface", loss_params=dict(centers=3))
    with pytest.raises(ValueError, match="unknown keys"):
        ProxyTrainer(ident, head, opt, loss="arcface", loss_params=dict(gamma=0.1))
    with pytest.raises(ValueError, match="unknown keys"):
        ProxyTrainer(ident, head, opt, loss="proxy_softmax", loss_params=dict(centers=4))
    with pytest.raises(ValueError, match="centers_per_class"):                 # the one-proxy losses on a multi-centre head
        ProxyTrainer(ident, head, opt, loss="proxy_softmax")


def _cfg(mode, model_mode="triplet", **gen):
    return dict(generator=dict(negatives_selection_mode=mode, k_classes=8, k_samples=4, **gen), model=dict(mode=model_mode))


def test_train_config_accepts_and_refuses_the_key():
    train = _train()
    assert train.proxy_loss_config(_cfg("soft_triple")) is None and train.proxy_loss_config(_cfg("arcface")) is None
    assert train.proxy_loss_config(_cfg("soft_triple", proxy_loss=dict(scale=10, centers=5, tau=0))) == dict(scale=10.0, tau=0.0, centers=5)
    assert train.proxy_loss_config(_cfg("arcface", proxy_loss=dict(margin=0.3, centers=3))) == dict(margin=0.3, centers=3)
    assert tuple(train.MULTI_PROXY_LOSS_CONFIGS["soft_triple"]) == ("scale", "margin", "gamma", "tau", "centers")
    assert tuple(train.MULTI_PROXY_LOSS_CONFIGS["arcface"]) == ("scale", "margin", "centers")
    assert train.MULTI_PROXY_DEFAULT_CENTERS == dict(soft_triple=10, arcface=1)
    for mode, bads in (("soft_triple", (dict(alpha=2.0), dict(scale=0), dict(gamma=0.0), dict(gamma=-1), dict(tau=-0.1), dict(centers=0),
                                        dict(centers=2.5), dict(centers=33), dict(scale="big"), dict(tau=True), [20.0])),
                       ("arcface", (dict(gamma=0.1), dict(tau=0.2), dict(margin=1.6), dict(margin=-0.1), dict(scale=-64.0), dict(centers=64),
                                    "arc"))):
        for bad in bads:
            with pytest.raises(ValueError, match="GENERATOR.proxy_loss"):
                train.proxy_loss_config(_cfg(mode, proxy_loss=bad))
    for mode in M.KINDS:
        with pytest.raises(ValueError, match="Siamese"):
            train.proxy_loss_config(_cfg(mode, model_mode="siamese", proxy_loss=dict(scale=32.0)))
        with pytest.raises(ValueError, match="GENERATOR.xbm"):                 # the memory goes with TripletTrainer's modes only
            train.xbm_config(_cfg(mode, xbm=dict(size=64)))
        with pytest.raises(ValueError, match="GENERATOR.ms_loss"):
            train.ms_loss_config(_cfg(mode, ms_loss=dict(alpha=2.0)))
    for mode in ("semihard", "supcon"):                                        # the key stays refused with the other modes
        with pytest.raises(ValueError, match="GENERATOR.proxy_loss"):
            train.proxy_loss_config(_cfg(mode, proxy_loss=dict(centers=3)))
    from embeddingnet_amd.utils import parse_params
    for mode in M.KINDS:
        cfg = parse_params(os.path.join(ROOT, "configs", f"simple2_{mode}_synthetic.yml"))
        assert cfg["generator"]["negatives_selection_mode"] == mode
        got = train.proxy_loss_config(cfg)
        assert tuple(got) == tuple(train.MULTI_PROXY_LOSS_CONFIGS[mode])
        d = M.DEFAULTS[mode]
        assert got["scale"] == d["a"] and got["margin"] == d["b"] and got["centers"] == train.MULTI_PROXY_DEFAULT_CENTERS[mode]
        if mode == "soft_triple":
            assert got["gamma"] == d["gamma"] and got["tau"] == d["tau"]


def test_checkpoints_keep_the_centres_per_class(tmp_path):
    from embeddingnet_amd.proxies import ProxyHead
    train = _train()
    names = [f"class_{i}" for i in range(5)]
    head = ProxyHead(5, 8, seed=1, centers_per_class=3)
    train.save_proxies(str(tmp_path / "p.npz"), head, names)
    assert int(np.load(tmp_path / "p.npz")["centers_per_class"]) == 3
    other = ProxyHead(5, 8, seed=2, centers_per_class=3)
    train.load_proxies(str(tmp_path / "p.npz"), other, names)
    assert torch.equal(other.proxies, head.proxies)
    with pytest.raises(ValueError, match="centers_per_class"):
        train.load_proxies(str(tmp_path / "p.npz"), ProxyHead(15, 8, seed=2), [f"c{i}" for i in range(15)])
    with pytest.raises(ValueError, match="centers_per_class"):
        train.load_proxies(str(tmp_path / "p.npz"), ProxyHead(5, 8, centers_per_class=2), names)
    one = ProxyHead(5, 8, seed=4)                              # a file from before the key: one centre per class
    np.savez(tmp_path / "old.npz", proxies=one.proxies.detach().numpy(), class_names=np.asarray(names, dtype=str))
    back = ProxyHead(5, 8, seed=5)
    train.load_proxies(str(tmp_path / "old.npz"), back, names)
    assert torch.equal(back.proxies, one.proxies)
    with pytest.raises(ValueError, match="centers_per_class"):
        train.load_proxies(str(tmp_path / "old.npz"), ProxyHead(5, 8, centers_per_class=2), names)


# ---------------------------------------------------------------------------------------------------------------- 3. the restatement
def _torch_loss(kind, xt, wt, lab, c, kc, pr, q=None, textbook=False, s=None):
    """The loss composed from torch ops in float64 from the textbook formulas: cross-entropy over the pooled, margined logits plus the
    authors' regulariser.  q: the fp32 q as constants; None: the exact normalisation.  textbook: ArcFace's own-class logit as
    cos(acos(S') + m) with float64 m (needs |S'| < 1 and S' > cos(pi - m)), not the product form on the fp32 constants."""
    n = xt.shape[0]
    qq = (wt * wt).sum(1) ** -0.5 if q is None else q
    s3 = ((xt @ wt.T) * qq if s is None else s).reshape(n, c, kc)            # s: S itself, to differentiate by it
    labels = torch.as_tensor(lab, dtype=torch.int64)
    labelled = (labels >= 0) & (labels < c)
    pos = (labels[:, None] == torch.arange(c)[None, :]) & labelled[:, None]
    if kind == "arcface":
        sp = s3.max(2).values
        if textbook:
            own = torch.cos(torch.acos(sp) + pr["b"])
        else:
            r = torch.sqrt(torch.clamp(1.0 - sp * sp, min=0.0))
            own = torch.where(sp > pr["th"], sp * pr["cm"] - r * pr["sm"], sp - pr["mm"])
        t = pr["a"] * torch.where(pos, own, sp)
        reg = 0.0
    else:
        sp = (torch.softmax(s3 / pr["gamma"], 2) * s3).sum(2)
        t = pr["a"] * (sp - pr["b"] * pos)
        reg = 0.0
        if kc > 1 and pr["tau"] > 0:
            wn = (wt * qq[:, None]).reshape(c, kc, -1)
            gram = wn @ wn.transpose(1, 2)
            up = torch.triu(torch.ones(kc, kc, dtype=torch.bool), 1)
            reg = pr["tau"] / (c * kc * (kc - 1)) * torch.sqrt(2.0 + 1e-5 - 2.0 * gram[:, up]).sum()
    ell = torch.logsumexp(t, 1) - torch.where(pos, t, torch.zeros((), dtype=torch.float64)).sum(1)
    return (ell[labelled].sum() / labelled.sum() if labelled.any() else ell.sum() * 0.0) + reg


CASES = [(3, 3, 5, 2, 64), (5, 5, 7, 2, 33), (8, 4, 24, 3, 256), (4, 4, 6, 32, 16), (16, 16, 40, 1, 128), "ragged"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CASES, ids=str)
def test_restatement_against_torch_autograd(shape, kind):
    """Loss, reg, G = dloss/dS, H, demb and dcentres.  With the SAME q as constants the loss and G are autograd's to float64 rounding;
    with the exact normalisation the relative difference 2^-24 of q moves S by u |S| and the rest accordingly."""
    x, w, lab, c, kc, _ = M.case_inputs(shape)
    ref = M.reference(kind, x, w, lab, c)
    pr = ref["pr"]
    if kind == "arcface":                                    # away from the branch point and the floor band
        sy = ref["sy"][ref["labelled"]]
        assert (sy > pr["th"] + 0.05).all() and (ref["r"][ref["labelled"]] > 0.01).all()
        assert ref["counts"][2] == 0
    q = torch.tensor(ref["q"].astype(np.float64))
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    wt = torch.tensor(w.astype(np.float64))
    s = torch.tensor(ref["S"], requires_grad=True)
    n = x.shape[0]
    # G against autograd's derivative by S: the loss as a function of S alone (the regulariser does not depend on it)
    labels = torch.as_tensor(lab, dtype=torch.int64)
    l2 = _torch_loss(kind, xt, wt, lab, c, kc, pr, q=q, s=s)
    l2.backward()
    assert abs(float(l2.detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    assert np.abs(ref["G"] - s.grad.numpy()).max() <= 1e-11 * max(np.abs(ref["G"]).max(), 1.0)
    # the gradients with the exact normalisation
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    wt = torch.tensor(w.astype(np.float64), requires_grad=True)
    loss = _torch_loss(kind, xt, wt, lab, c, kc, pr)
    loss.backward()
    slack = pr["a"] * P.U * np.abs(ref["S"]).max() * (1.0 + 2.0 / pr["gamma"] if kind == "soft_triple" else 1.0)
    assert abs(float(loss.detach()) - ref["loss"]) <= 4 * slack * max(1.0, abs(ref["loss"]))
    demb, _, dw, _ = M.grads(x, w, ref["G"], ref["q"], c, ref["reg"]["H"])
    for got, want in ((demb, xt.grad.numpy()), (dw, wt.grad.numpy())):
        assert np.abs(got - want).max() <= 64 * slack * max(np.abs(want).max(), 1e-30), np.abs(got - want).max() / np.abs(want).max()
    if kind == "arcface":                                    # the product form IS cos(acos(S') + m), to the fp32 constants' rounding
        tb = _torch_loss(kind, xt.detach(), wt.detach(), lab, c, kc, pr, textbook=True)
        assert abs(float(tb) - ref["loss"]) <= 8 * pr["a"] * P.U * max(1.0, abs(ref["loss"]))
    assert n == len(labels)


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_against_central_differences(kind):
    x, w, lab, c, kc, _ = M.case_inputs((3, 3, 5, 2, 64))
    ref = M.reference(kind, x, w, lab, c, a=8.0)
    demb, _, dw, _ = M.grads(x, w, ref["G"], ref["q"], c, ref["reg"]["H"])
    x64, w64 = x.astype(np.float64), w.astype(np.float64)

    def f(xx, ww):
        return float(_torch_loss(kind, torch.tensor(xx), torch.tensor(ww), lab, c, kc, ref["pr"]))
    h = 1e-6
    r = np.random.RandomState(0)
    for _ in range(12):
        i, k = r.randint(x.shape[0]), r.randint(x.shape[1])
        d = np.zeros_like(x64); d[i, k] = h
        assert abs((f(x64 + d, w64) - f(x64 - d, w64)) / (2 * h) - demb[i, k]) <= 1e-5 * max(1.0, abs(demb[i, k]))
        cc, k = r.randint(w.shape[0]), r.randint(w.shape[1])
        d = np.zeros_like(w64); d[cc, k] = h
        assert abs((f(x64, w64 + d) - f(x64, w64 - d)) / (2 * h) - dw[cc, k]) <= 1e-5 * max(1.0, abs(dw[cc, k]))


def test_cases_worked_by_hand():
    """Two classes with two unit centres each, e = 2: class 0 has (1, 0) and (0, 1), class 1 has (-1, 0) twice.  The sample (3, 4) / 5
    of class 0 has S = 0.6, 0.8 | -0.6, -0.6."""
    w = np.array([[1, 0], [0, 1], [-1, 0], [-1, 0]], np.float32)
    x = np.array([[0.6, 0.8]], np.float32).repeat(2, 0)
    lab = np.array([0, 1])
    s = np.float32([0.6, 0.8]).astype(np.float64)
    arc = M.reference("arcface", x, w, lab, 2, a=4.0, b=0.5)
    pr = arc["pr"]
    assert np.array_equal(arc["q"], np.ones(4, np.float32)) and np.array_equal(arc["arg"], [[1, 0], [1, 0]])     # the tie goes to j = 0
    phi0 = s[1] * pr["cm"] - math.sqrt(1 - s[1] ** 2) * pr["sm"]
    assert abs(phi0 - math.cos(math.acos(s[1]) + 0.5)) < 1e-7
    l0 = math.log(math.exp(4 * phi0) + math.exp(4 * -s[0])) - 4 * phi0
    # sample 1 is labelled with the class whose centres are its negation's side: S'_y = -0.6 > th = cos(pi - 0.5) = -0.8776: upper branch
    phi1 = -s[0] * pr["cm"] - math.sqrt(1 - s[0] ** 2) * pr["sm"]
    l1 = math.log(math.exp(4 * phi1) + math.exp(4 * s[1])) - 4 * phi1
    assert abs(arc["loss"] - (l0 + l1) / 2) < 1e-14
    assert arc["counts"].tolist() == [2, 1, 0]               # sample 1: the other class pools 0.8 >= -0.6
    assert not arc["G"][:, [0, 3]].any() and arc["reg"]["R"] == 0.0
    psi0 = pr["cm"] + s[1] * pr["sm"] / math.sqrt(1 - s[1] ** 2)
    w0 = math.exp(4 * phi0) / (math.exp(4 * phi0) + math.exp(4 * -s[0]))
    assert abs(arc["G"][0, 1] - 4.0 / 2 * (w0 - 1) * psi0) < 1e-14
    low = M.reference("arcface", -x, w, np.array([0, 0]), 2, a=4.0, b=0.5)       # S'_y = max(-0.6, -0.8) = -0.6 ... still upper
    assert low["counts"][2] == 0
    low = M.reference("arcface", x, w, np.array([1, 1]), 2, a=4.0, b=1.2)        # th = cos(pi - 1.2) = -0.362 >= -0.6: the guard's branch
    assert low["counts"].tolist() == [2, 2, 2] and abs(low["t"][0, 1] - 4.0 * (-s[0] - low["pr"]["mm"])) < 1e-14
    assert np.all(low["psi"] == 1.0)
    st = M.reference("soft_triple", x, w, lab, 2, a=4.0, b=0.25, gam=0.5, tau=0.3)
    p1 = 1.0 / (1.0 + math.exp((s[0] - s[1]) / 0.5))
    sp0 = (1 - p1) * s[0] + p1 * s[1]
    t0 = [4 * (sp0 - 0.25), 4 * -s[0]]
    t1 = [4 * sp0, 4 * (-s[0] - 0.25)]
    tau = float(np.float32(0.3))                             # the C ABI takes floats
    reg = tau / (2 * 2 * 1) * (math.sqrt(2 + 1e-5) + math.sqrt(2 + 1e-5 - 2.0))    # (2 + 1e-5 is rounded before the 2 leaves)
    ce = lambda t, y: math.log(sum(math.exp(v) for v in t)) - t[y]
    assert abs(st["reg"]["R"] - reg) < 1e-15 and abs(st["loss"] - ((ce(t0, 0) + ce(t1, 1)) / 2 + reg)) < 1e-14
    assert abs(st["reg"]["H"][1, 0, 1] + tau / 4 / math.sqrt(2 + 1e-5 - 2.0)) < 1e-12 and st["reg"]["H"][0, 0, 0] == 0
    assert st["counts"].tolist() == [2, 1, 0]
    # kc = 1: both kinds pool nothing; SoftTriple is CosFace, ArcFace with m = 0 NormSoftmax
    x1, w1, lab1, c1, _, _ = M.case_inputs((16, 16, 40, 1, 128))
    cos = P.reference("softmax", x1, w1, lab1, 20.0, 0.01)
    one = M.reference("soft_triple", x1, w1, lab1, c1)
    assert one["loss"] == cos["loss"] and np.array_equal(one["G"], cos["G"]) and one["counts"][1] == cos["counts"][2]
    nsm = P.reference("softmax", x1, w1, lab1, 64.0, 0.0)
    a0 = M.reference("arcface", x1, w1, lab1, c1, b=0.0)
    assert abs(a0["loss"] - nsm["loss"]) <= 1e-12 * nsm["loss"] and np.abs(a0["G"] - nsm["G"]).max() <= 1e-12 * np.abs(nsm["G"]).max()


def test_edge_rows_and_stable_forms():
    x, w, lab, c, kc, _ = M.case_inputs((8, 4, 24, 3, 256))
    for kind in KINDS:
        lab1 = lab.copy()
        lab1[1:4] = [-1, c, 10 ** 6]
        r1 = M.reference(kind, x, w, lab1, c)
        assert r1["counts"][0] == 29 and not r1["G"][1:4].any()
        demb, _, dw, _ = M.grads(x, w, r1["G"], r1["q"], c, r1["reg"]["H"])
        assert not demb[1:4].any() and np.isfinite(r1["loss"])
        w0 = w.copy()
        w0[int(lab[0]) * kc + 1] = 0                         # a zero centre: S = 0, no gradient row, not even the regulariser's
        r0 = M.reference(kind, x, w0, lab, c)
        assert r0["q"][int(lab[0]) * kc + 1] == 0 and not r0["S"][:, int(lab[0]) * kc + 1].any()
        _, _, dw, _ = M.grads(x, w0, r0["G"], r0["q"], c, r0["reg"]["H"])
        assert not dw[int(lab[0]) * kc + 1].any() and np.isfinite(dw).all()
        ru = M.reference(kind, x, w, np.full(32, -1), c)
        assert ru["loss"] == ru["reg"]["R"] and not ru["G"].any() and ru["counts"].tolist() == [0, 0, 0]
        big = M.reference(kind, 30.0 * x, w, lab, c)         # rows of norm 30: gamma 0.1 and scale 64 stay finite
        assert np.isfinite(big["loss"]) and np.isfinite(big["G"]).all()
        b = M.bounds(big, P.gamma_s("small", 256))
        assert np.isfinite(b["G"]).all() and np.isfinite(b["loss"])
    ident = np.repeat(w[::kc], kc, 0)                        # identical centres: g = 1, H finite
    rg = M.regulariser(ident, c, kc, 0.2)
    # q is an fp32 number: g = q^2 ss lies within (1 + u)^2 of 1, the root's argument within 4.1 u of 1e-5, the root within half that
    ideal = float(np.float32(0.2)) / (c * kc * (kc - 1)) * c * 3 * math.sqrt(1e-5)
    assert np.isfinite(rg["H"]).all() and abs(rg["R"] - ideal) <= ideal * 2.1 * P.U / 1e-5
    assert M.regulariser(w, c, kc, 0.0)["R"] == 0.0 and M.regulariser(w[::kc], c, 1, 0.2)["R"] == 0.0


# ---------------------------------------------------------------------------------------------------------------- 4. fitness
@pytest.mark.parametrize("shape", M.SHAPES + ["ragged"], ids=str)
def test_gpu_test_inputs_are_fit(shape):
    """On every shape of the GPU test, at the gamma_S of the path `auto` takes (and of both where both run): at most 1 % of the
    (sample, class) cells have an open argmax, no ArcFace branch is open, the own-class similarity stays out of the floor band, no
    violating-sample decision is open, and the bounds are finite and small; the grid inputs are exact in any order."""
    x, w, lab, c, kc, _ = M.case_inputs(shape)
    xg, wg, _, _, _, unit = M.case_inputs(shape, grid=True)
    assert P.exact_in_any_order(xg, wg, unit)
    assert (P.q_of(w) > 0).all() and (P.q_of(wg) > 0).all()
    n, e = x.shape
    gss = {M.gamma_s_of(shape), P.gamma_s("matrix", e)}
    if M.fits_small(n, c, kc, e):
        gss.add(P.gamma_s("small", e))
    for kind in KINDS:
        for xx, ww, gs, exact in [(x, w, g, False) for g in sorted(gss)] + [(xg, wg, 0.0, True)]:
            ref = M.reference(kind, xx, ww, lab, c)
            d = M.decisions(ref, gs)
            share = float(d["open_cells"].mean())
            assert share <= M.OPEN_CAP, (kind, shape, share)
            assert not d["branch_open"].any() and not d["open"].any(), (kind, shape)
            assert d["sure"].sum() == ref["counts"][1] == d["may"].sum() and d["lower_sure"].sum() == ref["counts"][2] == 0
            if kind == "arcface":
                assert (ref["sy"][ref["labelled"]] > 0.5).all()              # against th = -0.88: far above the branch point
            b = M.bounds(ref, gs, exact_argmax=exact)
            assert np.isfinite(b["G"]).all() and np.isfinite(b["total"]).all()
            assert 0 < b["loss"] < 1e-2 * abs(ref["loss"]), (kind, shape, b["loss"], ref["loss"])
            assert np.array_equal(b["open_cells"], d["open_cells"] & (not exact))
