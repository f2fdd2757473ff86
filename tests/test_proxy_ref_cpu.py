"""Proxy-Anchor and CosFace / NormSoftmax, host side (no GPU): the C ABI is declared and exported and refuses arguments outside its
range before any launch; the path rule and the workspace size are restated; the float64 restatement in tests/proxy_ref.py agrees with
torch autograd, with central differences, with a scalar restatement and with cases worked by hand; the Python layers know the modes;
the Feeder's label FIFO follows the plans; and the inputs of tests/test_proxy_loss_gpu.py are fit for what that test asserts on them."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import proxy_ref as P
import recipes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_proxy_loss_path", "embnet_proxy_loss_workspace_bytes", "embnet_proxy_loss_fwd", "embnet_proxy_loss_bwd")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced
KINDS = list(P.KINDS)


# ---------------------------------------------------------------------------------------------------------------- 1. the ABI
def _lib():
    from embeddingnet_amd import _lib
    return _lib.lib()


def test_header_declares_and_library_exports_the_proxy_losses():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported
    assert exported == set(protos)
    assert _lib.lib().embnet_abi_version() == 22


FWD_PTRS = ["emb", "proxies", "labels", "g", "q", "counts", "mean", "ws"]
BWD_PTRS = ["emb", "proxies", "g", "q", "demb", "dproxies", "ws"]


def _fwd(n, c, e, kind=1, a=32.0, b=0.1, ws=FAKE, ws_bytes=1 << 40, path=0, null=None):
    l = _lib()
    p = {k: FAKE for k in FWD_PTRS}
    p["ws"] = ws
    if null:
        p[null] = None
    rc = l.embnet_proxy_loss_fwd(p["emb"], p["proxies"], p["labels"], n, c, e, kind, a, b, path, p["g"], p["q"], p["counts"],
                                 p["mean"], p["ws"], ws_bytes, None)
    return rc, l.embnet_last_error().decode()


def _bwd(n, c, e, kind=1, ws=FAKE, ws_bytes=1 << 40, null=None):
    l = _lib()
    p = {k: FAKE for k in BWD_PTRS}
    p["ws"] = ws
    if null:
        p[null] = None
    rc = l.embnet_proxy_loss_bwd(p["emb"], p["proxies"], n, c, e, kind, p["g"], p["q"], None, p["demb"], p["dproxies"], p["ws"],
                                 ws_bytes, None)
    return rc, l.embnet_last_error().decode()


@pytest.mark.parametrize("null", FWD_PTRS)
def test_fwd_rejects_null_pointers(null):
    rc, msg = _fwd(32, 24, 256, null=null)
    assert rc == -1 and "proxy_loss_fwd: null pointer" in msg


@pytest.mark.parametrize("null", BWD_PTRS)
def test_bwd_rejects_null_pointers(null):
    rc, msg = _bwd(32, 24, 256, null=null)
    assert rc == -1 and "proxy_loss_bwd: null pointer" in msg


@pytest.mark.parametrize("n,c,e,what", [(1, 24, 64, "n=1"), (4097, 24, 64, "n=4097"), (32, 1, 64, "c=1"), (32, 16385, 64, "c=16385"),
                                        (32, 24, 0, "e=0"), (32, 24, 4097, "e=4097"), (-5, 24, 64, "n=-5")])
def test_both_reject_out_of_range_shapes(n, c, e, what):
    for call, name in ((_fwd, "proxy_loss_fwd"), (_bwd, "proxy_loss_bwd")):
        rc, msg = call(n, c, e)
        assert rc == -1 and what in msg and msg.startswith(name), msg
    assert _lib().embnet_proxy_loss_path(n, c, e) == 0 and _lib().embnet_proxy_loss_workspace_bytes(n, c, e) == 0
    assert P.auto_path(n, c, e) is None and P.workspace_bytes(n, c, e) == 0


@pytest.mark.parametrize("kind", [0, 3, -1])
def test_both_reject_an_unknown_kind(kind):
    for call, name in ((_fwd, "proxy_loss_fwd"), (_bwd, "proxy_loss_bwd")):
        rc, msg = call(32, 24, 256, kind=kind)
        assert rc == -1 and "unknown kind" in msg and msg.startswith(name), msg


@pytest.mark.parametrize("kind,name", [(1, "alpha"), (2, "scale")])
@pytest.mark.parametrize("a", [0.0, -1.0, math.nan, math.inf, -math.inf])
def test_fwd_rejects_a_first_scalar_that_is_not_positive_and_finite(a, kind, name):
    rc, msg = _fwd(32, 24, 256, kind=kind, a=a)
    assert rc == -1 and msg.startswith("proxy_loss_fwd") and name in msg, msg


@pytest.mark.parametrize("kind,name", [(1, "delta"), (2, "margin")])
@pytest.mark.parametrize("b", [math.nan, math.inf, -math.inf])
def test_fwd_rejects_a_second_scalar_that_is_not_finite(b, kind, name):
    rc, msg = _fwd(32, 24, 256, kind=kind, b=b)
    assert rc == -1 and msg.startswith("proxy_loss_fwd") and name in msg, msg
    assert _fwd(32, 24, 256, kind=kind, b=-0.5, null="emb")[1].endswith("null pointer")       # a negative one is in range


def test_both_reject_bad_workspace_and_path():
    need = _lib().embnet_proxy_loss_workspace_bytes(32, 24, 256)
    for kind in (1, 2):
        for call, name in ((_fwd, "proxy_loss_fwd"), (_bwd, "proxy_loss_bwd")):
            rc, msg = call(32, 24, 256, kind=kind, ws_bytes=need - 16)
            assert rc == -3 and "workspace" in msg and msg.startswith(name)
            rc, msg = call(32, 24, 256, kind=kind, ws=FAKE + 4)
            assert rc == -1 and "16-byte aligned" in msg and msg.startswith(name)
        for path in (3, -1):
            rc, msg = _fwd(32, 24, 256, kind=kind, path=path)
            assert rc == -1 and "proxy_loss_fwd: unknown path" in msg
        rc, msg = _fwd(16, 4001, 96, kind=kind, path=1)     # e + c = 4097: only the matrix path
        assert rc == -1 and "small path" in msg and msg.startswith("proxy_loss_fwd")


def test_path_rule_and_workspace_size_restated():
    l = _lib()
    shapes = [(p * k, c, e) for p, k, e, c in P.SHAPES] + [(17, P.RAGGED[1], P.RAGGED[0]), (2, 2, 1), (4096, 16384, 4096), (4096, 2, 1),
                                                           (2, 4095, 1), (2, 4096, 1), (4095, 2, 1), (512, 100, 256), (128, 4096, 128)]
    for n, c, e in shapes:
        assert l.embnet_proxy_loss_path(n, c, e) == {"small": 1, "matrix": 2}[P.auto_path(n, c, e)], (n, c, e)
        assert l.embnet_proxy_loss_workspace_bytes(n, c, e) == P.workspace_bytes(n, c, e) >= 4 * n * c + 8 * c * e, (n, c, e)
    for p, k, e, c in P.SMALL_SHAPES:
        assert l.embnet_proxy_loss_path(p * k, c, e) == 1
    for p, k, e, c in P.MATRIX_SHAPES:
        assert l.embnet_proxy_loss_path(p * k, c, e) == 2
    assert l.embnet_proxy_loss_path(512, 100, 256) == 1     # the project's own batches take the small path
    assert P.workspace_bytes(4096, 16384, 4096) < 2 ** 30


# ---------------------------------------------------------------------------------------------------------------- 2. the layers
def test_python_layers_know_the_modes():
    from embeddingnet_amd import losses_and_accuracies, ops
    from embeddingnet_amd.datagenerators import SyntheticDataLoader, TripletsDataGenerator
    from embeddingnet_amd.proxies import ProxyHead
    from embeddingnet_amd.train_step import ProxyTrainer, TripletTrainer
    import embedding_net.proxies
    assert embedding_net.proxies.ProxyHead is ProxyHead
    assert set(ops.PROXY_LOSS_MODES) == {"proxy_anchor", "proxy_softmax"}
    assert ops.PROXY_LOSS_MODES["proxy_anchor"] == (ops.proxy_anchor_loss, ("alpha", "delta"))
    assert ops.PROXY_LOSS_MODES["proxy_softmax"] == (ops.proxy_softmax_loss, ("scale", "margin"))
    assert ops.PROXY_PATHS == dict(auto=0, small=1, matrix=2)
    for mode in ops.PROXY_LOSS_MODES:
        assert mode in TripletsDataGenerator.STEP_ONLY_MODES
    head = ProxyHead(6, 16, seed=3)
    assert callable(losses_and_accuracies.proxy_anchor_loss(head, 16.0, 0.2))
    assert callable(losses_and_accuracies.proxy_softmax_loss(head, 30.0, 0.0))
    data = SyntheticDataLoader(6, 4, (8, 8, 3), validate=False)
    for mode in ops.PROXY_LOSS_MODES:
        gen = TripletsDataGenerator(embedding_model=None, class_files_paths=data.train_data, class_names=data.class_names,
                                    n_batches=2, input_shape=[8, 8, 3], k_classes=3, k_samples=2, negatives_selection_mode=mode)
        with pytest.raises(ValueError, match="fused step"):
            gen.mine_batch(gen.sample_batch())
    opt = torch.optim.SGD([head.proxies], lr=0.1)
    ident = torch.nn.Identity()
    assert issubclass(ProxyTrainer, TripletTrainer)
    assert ProxyTrainer(ident, head, opt).mode == "proxy_anchor" and ProxyTrainer(ident, head, opt).loss_params == {}
    assert ProxyTrainer(ident, head, opt, loss="proxy_anchor", loss_params=dict(alpha=16.0, delta=0.2)).loss_params == dict(alpha=16.0, delta=0.2)
    assert ProxyTrainer(ident, head, opt, loss="proxy_softmax", loss_params=dict(scale=30.0)).loss_params == dict(scale=30.0)
    with pytest.raises(ValueError, match="unknown keys"):                      # per mode: the other loss's keys are unknown
        ProxyTrainer(ident, head, opt, loss="proxy_anchor", loss_params=dict(scale=30.0))
    with pytest.raises(ValueError, match="unknown keys"):
        ProxyTrainer(ident, head, opt, loss="proxy_softmax", loss_params=dict(alpha=2.0, margin=0.1))
    with pytest.raises(KeyError):
        ProxyTrainer(ident, head, opt, loss="supcon")
    with pytest.raises(ValueError, match="head.proxies"):
        ProxyTrainer(ident, head, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1))
    with pytest.raises(ValueError, match="int32"):
        ProxyTrainer(ident, head, opt).step(torch.zeros(4, 16), torch.zeros(4, dtype=torch.int64))


def _cfg(mode, model_mode="triplet", **gen):
    return dict(generator=dict(negatives_selection_mode=mode, **gen), model=dict(mode=model_mode))


def test_train_config_function_accepts_and_refuses_the_key():
    import importlib.util
    spec = importlib.util.spec_from_file_location("embnet_tools_train", os.path.join(ROOT, "tools", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    assert train.proxy_loss_config(_cfg("proxy_anchor")) is None and train.proxy_loss_config(_cfg("semihard")) is None
    assert train.proxy_loss_config(_cfg("proxy_anchor", proxy_loss=dict(alpha=16, delta=0.2))) == dict(alpha=16.0, delta=0.2)
    assert train.proxy_loss_config(_cfg("proxy_softmax", proxy_loss=dict(scale=30))) == dict(scale=30.0)
    assert train.proxy_loss_config(_cfg("proxy_softmax", proxy_loss=dict(margin=0.0))) == dict(margin=0.0)
    for mode in ("semihard", "multi_similarity", "supcon", "batch_all"):
        with pytest.raises(ValueError, match="GENERATOR.proxy_loss"):
            train.proxy_loss_config(_cfg(mode, proxy_loss=dict(alpha=32.0)))
    with pytest.raises(ValueError, match="Siamese"):
        train.proxy_loss_config(_cfg("proxy_anchor", model_mode="siamese", proxy_loss=dict(alpha=32.0)))
    for mode in ("proxy_anchor", "proxy_softmax"):                             # the other losses' keys stay refused with these modes
        with pytest.raises(ValueError, match="GENERATOR.ms_loss"):
            train.ms_loss_config(_cfg(mode, ms_loss=dict(alpha=2.0)))
        with pytest.raises(ValueError, match="GENERATOR.supcon_loss"):
            train.supcon_loss_config(_cfg(mode, supcon_loss=dict(temperature=0.1)))
    for mode, bads in (("proxy_anchor", (dict(scale=64.0), dict(alpha="big"), dict(alpha=True), dict(alpha=0.0), dict(alpha=-1.0), [32.0])),
                       ("proxy_softmax", (dict(alpha=32.0), dict(scale=0), dict(scale=-64.0), dict(margin=None), "cosface"))):
        for bad in bads:
            with pytest.raises(ValueError, match="GENERATOR.proxy_loss"):
                train.proxy_loss_config(_cfg(mode, proxy_loss=bad))
    for name in ("simple2_proxy_anchor_synthetic.yml", "simple2_proxy_softmax_synthetic.yml"):
        from embeddingnet_amd.utils import parse_params
        cfg = parse_params(os.path.join(ROOT, "configs", name))
        assert cfg["generator"]["negatives_selection_mode"] in train.PROXY_LOSS_KEYS
        assert set(train.proxy_loss_config(cfg)) == set(train.PROXY_LOSS_KEYS[cfg["generator"]["negatives_selection_mode"]])
        assert cfg["generator"]["k_classes"] == 8 and cfg["generator"]["k_samples"] == 4 and cfg["generator"]["n_batches"] == 20


def test_loss_config_table_names_the_trainers_parameters_and_keeps_the_messages():
    """tools/train.py's one table-driven validator: every mode's parameters are the ones its trainer takes, in its order, and
    each kind of refusal keeps the text the three separate validators had."""
    import importlib.util
    from embeddingnet_amd.train_step import ProxyTrainer, TripletTrainer
    spec = importlib.util.spec_from_file_location("embnet_tools_train", os.path.join(ROOT, "tools", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    assert set(train.LOSS_CONFIGS) == {"ms_loss", "supcon_loss", "proxy_loss"}
    for table in train.LOSS_CONFIGS.values():
        for mode, checks in table.items():
            trainer = ProxyTrainer if mode in ProxyTrainer.LOSS_PARAMS else TripletTrainer
            assert tuple(checks) == tuple(trainer.LOSS_PARAMS[mode])
    assert train.MS_LOSS_KEYS == ("alpha", "beta", "base", "epsilon") and train.SUPCON_LOSS_KEYS == ("temperature", "denominator")
    assert train.PROXY_LOSS_KEYS == {"proxy_anchor": ("alpha", "delta"), "proxy_softmax": ("scale", "margin")}
    texts = [
        (train.ms_loss_config, _cfg("semihard", ms_loss=dict(alpha=2.0)),
         "GENERATOR.ms_loss sets the parameters of negatives_selection_mode 'multi_similarity'; this config trains with 'semihard': "
         "drop the key or change the mode"),
        (train.proxy_loss_config, _cfg("proxy_anchor", model_mode="siamese", proxy_loss=dict(alpha=2.0)),
         "GENERATOR.proxy_loss sets the parameters of negatives_selection_mode 'proxy_anchor' or 'proxy_softmax'; this config trains "
         "with the Siamese contrastive loss: drop the key or change the mode"),
        (train.ms_loss_config, _cfg("multi_similarity", ms_loss=dict(gamma=1.0)),
         "GENERATOR.ms_loss: a mapping with keys out of ('alpha', 'beta', 'base', 'epsilon') (got {'gamma': 1.0})"),
        (train.proxy_loss_config, _cfg("proxy_softmax", proxy_loss=dict(alpha=1.0)),
         "GENERATOR.proxy_loss: a mapping with keys out of ('scale', 'margin') for 'proxy_softmax' (got {'alpha': 1.0})"),
        (train.ms_loss_config, _cfg("multi_similarity", ms_loss=dict(alpha=True)),
         "GENERATOR.ms_loss: every value must be a number (got {'alpha': True})"),
        (train.proxy_loss_config, _cfg("proxy_anchor", proxy_loss=dict(alpha=-1.0, delta="x")),
         "GENERATOR.proxy_loss: every value must be a number (got {'alpha': -1.0, 'delta': 'x'})"),
        (train.proxy_loss_config, _cfg("proxy_anchor", proxy_loss=dict(delta=0.1, alpha=0)),
         "GENERATOR.proxy_loss: alpha must be positive (got 0)"),
        (train.supcon_loss_config, _cfg("supcon", supcon_loss=dict(temperature="hot", denominator="none")),
         "GENERATOR.supcon_loss: temperature must be a positive number (got 'hot')"),
        (train.supcon_loss_config, _cfg("supcon", supcon_loss=dict(denominator="none")),
         "GENERATOR.supcon_loss: denominator must be 'all' or 'negatives' (got 'none')"),
    ]
    for fn, cfg, text in texts:
        with pytest.raises(ValueError) as err:
            fn(cfg)
        assert str(err.value) == text
    assert train.ms_loss_config(_cfg("multi_similarity", ms_loss=dict(beta=40, alpha=1))) == dict(alpha=1.0, beta=40.0)
    assert train.proxy_loss_config(_cfg("proxy_anchor", proxy_loss=dict(delta=-0.5))) == dict(delta=-0.5)


def test_proxy_checkpoints_round_trip_and_refuse_other_classes(tmp_path):
    import importlib.util
    from embeddingnet_amd.proxies import ProxyHead
    spec = importlib.util.spec_from_file_location("embnet_tools_train", os.path.join(ROOT, "tools", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    names = [f"class_{i:03d}" for i in range(5)]
    a, b = ProxyHead(5, 8, seed=1), ProxyHead(5, 8, seed=2)
    path = train._proxies_path(str(tmp_path / "weights" / "epoch_003.npz"))
    assert path == str(tmp_path / "proxies" / "epoch_003.npz")
    train.save_proxies(path, a, names)
    train.load_proxies(path, b, names)
    assert torch.equal(a.proxies, b.proxies)
    with pytest.raises(ValueError, match="class_names"):
        train.load_proxies(path, b, names[::-1])
    with pytest.raises(ValueError, match="class_names"):
        train.load_proxies(path, ProxyHead(4, 8), names[:4])


def test_proxy_head_is_seeded_on_the_cpu_and_kaiming_fan_out():
    from embeddingnet_amd.proxies import ProxyHead
    a, b, c = ProxyHead(200, 64, seed=7), ProxyHead(200, 64, seed=7), ProxyHead(200, 64, seed=8)
    assert [n for n, _ in a.named_parameters()] == ["proxies"] and a.proxies.shape == (200, 64) and a.proxies.dtype == torch.float32
    assert torch.equal(a.proxies, b.proxies) and not torch.equal(a.proxies, c.proxies)
    torch.manual_seed(123)                                  # the global generator plays no part
    assert torch.equal(ProxyHead(200, 64, seed=7).proxies, a.proxies)
    want = torch.empty(200, 64)
    torch.nn.init.kaiming_normal_(want, mode="fan_out", generator=torch.Generator().manual_seed(7))
    assert torch.equal(a.proxies.detach(), want)            # torch's own initialiser, the same draw
    assert abs(float(a.proxies.detach().std()) - math.sqrt(2.0 / 200)) < 0.05 * math.sqrt(2.0 / 200)
    with pytest.raises(ValueError):
        ProxyHead(1, 64)


def test_feeder_label_fifo_follows_the_plans():
    """In-memory dataset: next_labelled()'s labels are the class indices of the plans a fresh generator draws from the same seed, with
    next() interleaved, and the images are next()'s."""
    from embeddingnet_amd.datagenerators import SyntheticDataLoader, TripletsDataGenerator
    from embeddingnet_amd.input_pipeline import Feeder
    data = SyntheticDataLoader(7, 5, (8, 8, 3), validate=False)

    def gen():
        return TripletsDataGenerator(embedding_model=None, class_files_paths=data.train_data, class_names=data.class_names,
                                     n_batches=2, input_shape=[8, 8, 3], k_classes=3, k_samples=2,
                                     negatives_selection_mode="proxy_anchor")
    pattern = [True, True, False, True, False, False, True, True]
    np.random.seed(5)
    g = gen()
    plans = [g.sample_plan() for _ in pattern]
    after = np.random.rand()
    np.random.seed(5)
    g = gen()
    feeder = Feeder(g, "cpu")
    assert feeder.kind == "memory"
    for labelled, plan in zip(pattern, plans):
        want_images = g.load_plan(plan)
        if labelled:
            images, labels = feeder.next_labelled()
            assert labels.dtype == torch.int32 and labels.shape == (6,)
            assert labels.tolist() == [data.class_names.index(cl) for cl in plan[0] for _ in range(2)]
        else:
            images = feeder.next()
        assert np.array_equal(images.numpy(), want_images)
    assert np.random.rand() == after                        # the np.random stream is where the plans alone leave it
    assert len(feeder._plan_labels) == 0


def test_feeder_label_fifo_with_plans_drawn_ahead():
    """The prefetch kind draws its plans `depth` batches ahead through Feeder._plan: the FIFO hands the OLDEST labels out, next() drops
    them.  (The prefetcher itself needs a GPU; its plan function is driven by hand here.)"""
    from embeddingnet_amd.datagenerators import SyntheticDataLoader, TripletsDataGenerator
    from embeddingnet_amd.input_pipeline import Feeder
    data = SyntheticDataLoader(7, 5, (8, 8, 3), validate=False)
    g = TripletsDataGenerator(embedding_model=None, class_files_paths=data.train_data, class_names=data.class_names, n_batches=2,
                              input_shape=[8, 8, 3], k_classes=3, k_samples=2, negatives_selection_mode="proxy_softmax")
    feeder = Feeder(g, "cpu")
    np.random.seed(9)
    plans = [feeder._plan() for _ in range(4)]
    assert len(feeder._plan_labels) == 4
    for plan in plans:
        lab = feeder._plan_labels.popleft()
        assert lab.dtype == np.int32 and lab.tolist() == [data.class_names.index(cl) for cl in plan[0] for _ in range(2)]


# ---------------------------------------------------------------------------------------------------------------- 3. the restatement
def _case(shape, grid=False):
    if shape == "ragged":
        e, c = P.RAGGED
        x, w, lab = P.ragged_inputs(R.clustered_embeddings(77, 5, 5, e, P.SIGMA), e, c, 77)
    else:
        p, k, e, c = shape
        x, w, lab = P.make_inputs(R.clustered_embeddings(P.seed_of(p, k, e), p, k, e, P.SIGMA), p, k, c, P.seed_of(p, k, e))
    if grid:
        x, w, unit = P.to_grid(x, w)
        return x, w, lab, unit
    return x, w, lab, None


def _torch_loss(kind, xt, wt, lab, a, b, q=None):
    """The loss composed from torch ops, float64, plain forms.  q: the fp32 q as constants times the exact normalisation's gradient is
    NOT what the header differentiates, so q is recomputed from wt (exact) unless given."""
    c = wt.shape[0]
    s = (xt @ wt.T) * ((wt * wt).sum(1) ** -0.5 if q is None else q)
    labels = torch.as_tensor(lab, dtype=torch.int64)
    labelled = (labels >= 0) & (labels < c)
    pos = (labels[:, None] == torch.arange(c)[None, :]) & labelled[:, None]
    ninf = torch.tensor(-float("inf"), dtype=torch.float64)
    if kind == "anchor":
        neg = ~pos & labelled[:, None]
        z = torch.zeros(c, 1, dtype=torch.float64)
        lp = torch.logsumexp(torch.cat([z, torch.where(pos, -a * (s - b), ninf).T], 1), 1)
        ln = torch.logsumexp(torch.cat([z, torch.where(neg, a * (s + b), ninf).T], 1), 1)
        present = pos.any(0)
        return (lp[present].sum() / present.sum() if present.any() else 0.0) + ln.sum() / c
    t = a * (s - b * pos)
    ell = torch.logsumexp(t, 1) - torch.where(pos, t, torch.zeros((), dtype=torch.float64)).sum(1)
    return ell[labelled].sum() / labelled.sum() if labelled.any() else ell.sum() * 0.0


CASES = [(8, 4, 256, 24), (3, 3, 64, 5), (5, 7, 33, 70), (16, 16, 128, 16), (4, 4, 64, 2), "ragged"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CASES, ids=str)
def test_restatement_against_torch_autograd(shape, kind):
    """Loss, G = dloss/dS, demb and dproxies.  The restatement holds q as the fp32 number the device has; autograd normalises exactly:
    the relative difference 2^-24 of q moves S by u |S|, a logit by a u |S| and the loss and G accordingly — the tolerances below."""
    x, w, lab, _ = _case(shape)
    ref = P.reference(kind, x, w, lab)
    a, b = ref["a"], ref["b"]
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    wt = torch.tensor(w.astype(np.float64), requires_grad=True)
    loss = _torch_loss(kind, xt, wt, lab, a, b)
    loss.backward()
    slack = a * P.U * np.abs(ref["S"]).max()                # one logit's shift
    assert abs(float(loss.detach()) - ref["loss"]) <= 4 * slack * max(1.0, abs(ref["loss"]))
    demb, _, dw, _ = P.grads(kind, x, w, ref["G"], ref["q"])
    for got, want in ((demb, xt.grad.numpy()), (dw, wt.grad.numpy())):
        assert np.abs(got - want).max() <= 16 * slack * max(np.abs(want).max(), 1e-30), np.abs(got - want).max()
    # with the SAME q (as constants) G itself is autograd's derivative by S to float64 rounding
    s = torch.tensor(ref["S"], requires_grad=True)
    labels = torch.as_tensor(lab, dtype=torch.int64)
    c = w.shape[0]
    labelled = (labels >= 0) & (labels < c)
    pos = (labels[:, None] == torch.arange(c)[None, :]) & labelled[:, None]
    ninf = torch.tensor(-float("inf"), dtype=torch.float64)
    if kind == "anchor":
        neg = ~pos & labelled[:, None]
        z = torch.zeros(c, 1, dtype=torch.float64)
        l2 = (torch.logsumexp(torch.cat([z, torch.where(pos, -a * (s - b), ninf).T], 1), 1)[pos.any(0)].sum() / pos.any(0).sum()
              + torch.logsumexp(torch.cat([z, torch.where(neg, a * (s + b), ninf).T], 1), 1).sum() / c)
    else:
        t = a * (s - b * pos)
        l2 = ((torch.logsumexp(t, 1) - torch.where(pos, t, torch.zeros((), dtype=torch.float64)).sum(1))[labelled]).sum() / labelled.sum()
    l2.backward()
    gs = s.grad.numpy()
    g = ref["G"].T if kind == "anchor" else ref["G"]
    assert abs(float(l2.detach()) - ref["loss"]) <= 1e-13 * abs(ref["loss"])
    assert np.abs(g - gs).max() <= 1e-13 * max(np.abs(gs).max(), 1.0)


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_against_central_differences(kind):
    x, w, lab, _ = _case((3, 3, 64, 5))
    ref = P.reference(kind, x, w, lab, 8.0, 0.1)
    demb, _, dw, _ = P.grads(kind, x, w, ref["G"], ref["q"])
    x64, w64 = x.astype(np.float64), w.astype(np.float64)

    def f(xx, ww):
        return float(_torch_loss(kind, torch.tensor(xx), torch.tensor(ww), lab, ref["a"], ref["b"]))
    h = 1e-6
    r = np.random.RandomState(0)
    for _ in range(12):
        i, k = r.randint(x.shape[0]), r.randint(x.shape[1])
        d = np.zeros_like(x64); d[i, k] = h
        assert abs((f(x64 + d, w64) - f(x64 - d, w64)) / (2 * h) - demb[i, k]) <= 1e-5 * max(1.0, abs(demb[i, k]))
        cc, k = r.randint(w.shape[0]), r.randint(w.shape[1])
        d = np.zeros_like(w64); d[cc, k] = h
        assert abs((f(x64, w64 + d) - f(x64, w64 - d)) / (2 * h) - dw[cc, k]) <= 1e-5 * max(1.0, abs(dw[cc, k]))


def _scalar(kind, x, w, lab, a, b):
    """One anchor at a time, plain Python floats, the PLAIN forms (no maximum is subtracted): shares no code with proxy_ref."""
    n, e = x.shape
    c = w.shape[0]
    q = []
    for cl in range(c):
        ss = 0.0
        for k in range(e):
            ss += float(w[cl, k]) * float(w[cl, k])
        q.append(float(np.float32(1.0 / math.sqrt(ss))) if ss > 0 else 0.0)
    s = [[sum(float(x[i, k]) * float(w[cl, k]) for k in range(e)) * q[cl] for cl in range(c)] for i in range(n)]
    lab = [int(v) for v in lab]
    ok = [0 <= v < c for v in lab]
    g = [[0.0] * c for _ in range(n)]
    if kind == "anchor":
        present = [cl for cl in range(c) if any(ok[i] and lab[i] == cl for i in range(n))]
        loss = 0.0
        for cl in range(c):
            sp = sum(math.exp(-a * (s[i][cl] - b)) for i in range(n) if ok[i] and lab[i] == cl)
            sn = sum(math.exp(a * (s[i][cl] + b)) for i in range(n) if ok[i] and lab[i] != cl)
            if cl in present:
                loss += math.log1p(sp) / len(present)
            loss += math.log1p(sn) / c
            for i in range(n):
                if ok[i] and lab[i] == cl:
                    g[i][cl] = -a * math.exp(-a * (s[i][cl] - b)) / (1.0 + sp) / len(present)
                elif ok[i]:
                    g[i][cl] = a * math.exp(a * (s[i][cl] + b)) / (1.0 + sn) / c
        return loss, np.array(g).T
    nl = sum(ok)
    loss = 0.0
    for i in range(n):
        if not ok[i]:
            continue
        t = [a * (s[i][cl] - (b if cl == lab[i] else 0.0)) for cl in range(c)]
        z = sum(math.exp(v) for v in t)
        loss += (math.log(z) - t[lab[i]]) / nl
        for cl in range(c):
            g[i][cl] = a * (math.exp(t[cl]) / z - (1.0 if cl == lab[i] else 0.0)) / nl
    return loss, np.array(g)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(3, 3, 64, 5), (4, 4, 64, 2), "ragged"], ids=str)
def test_restatement_against_a_scalar_restatement(shape, kind):
    x, w, lab, _ = _case(shape)
    a, b = (8.0, 0.1) if kind == "anchor" else (16.0, 0.35)          # the plain forms stay inside float64 at these scales
    ref = P.reference(kind, x, w, lab, a, b)
    loss, g = _scalar(kind, x, w, lab, ref["a"], ref["b"])
    assert abs(loss - ref["loss"]) <= 1e-12 * abs(loss)
    assert np.abs(g - ref["G"]).max() <= 1e-12 * np.abs(g).max()


def test_cases_worked_by_hand():
    """Two unit proxies on the axes, e = 2.  Samples: (1, 0) of class 0, (0, 1) of class 1, and (3, 4) / 5 of class 0."""
    w = np.eye(2, dtype=np.float32)
    x = np.array([[1.0, 0.0], [0.0, 1.0], [0.6, 0.8]], np.float32)
    lab = np.array([0, 1, 0])
    s = x.astype(np.float64)                                 # S_ic = x_ic
    a, d = 2.0, 0.25
    ref = P.reference("anchor", x, w, lab, a, d)
    assert np.array_equal(ref["q"], np.ones(2, np.float32))
    lp0 = math.log(1 + math.exp(-a * (1 - d)) + math.exp(-a * (s[2, 0] - d)))
    lp1 = math.log(1 + math.exp(-a * (1 - d)))
    ln0 = math.log(1 + math.exp(a * (0 + d)))
    ln1 = math.log(1 + math.exp(a * (0 + d)) + math.exp(a * (s[2, 1] + d)))
    assert abs(ref["loss"] - ((lp0 + lp1) / 2 + (ln0 + ln1) / 2)) < 1e-15
    assert ref["counts"].tolist() == [2, 3, 0]               # class 1: its negative (3,4)/5 at 0.8 < its positive at 1; class 0: 0 < 0.6
    sm = P.reference("softmax", x, w, lab, 4.0, 0.5)
    t2 = [4.0 * (s[2, 0] - 0.5), 4.0 * s[2, 1]]
    l2 = math.log(math.exp(t2[0]) + math.exp(t2[1])) - t2[0]
    l0 = math.log(math.exp(2.0) + 1.0) - 2.0
    assert abs(sm["loss"] - (l0 + l0 + l2) / 3) < 1e-15
    assert sm["counts"].tolist() == [3, 3, 1]                # (3,4)/5 is closer to the other class's proxy
    assert abs(sm["G"][2, 1] - 4.0 / 3 * math.exp(t2[1]) / (math.exp(t2[0]) + math.exp(t2[1]))) < 1e-15


@pytest.mark.parametrize("kind", KINDS)
def test_absent_single_unlabelled_zero_proxy_and_one_class(kind):
    x, w, lab, _ = _case((8, 4, 256, 24))
    c = 24
    # an absent class: no positive term, a row of non-negative weights (anchor); a column that only ever loses (softmax)
    ref = P.reference(kind, x, w, lab)
    absent = np.setdiff1d(np.arange(c), lab)
    assert len(absent) == 16
    if kind == "anchor":
        assert ref["counts"][0] == 8 and (ref["G"][absent] >= 0).all() and (ref["G"][lab[0], lab == lab[0]] < 0).all()
    else:
        assert ref["counts"][0] == 32 and (ref["G"][:, absent] >= 0).all()
        assert np.abs(ref["G"].sum(1)).max() < 1e-15         # a softmax row sums to zero
    # a class with one sample, an unlabelled sample
    lab1 = lab.copy()
    lab1[1:4] = [-1, c, 10 ** 6]
    r1 = P.reference(kind, x, w, lab1)
    assert r1["counts"][1] == 29 and r1["counts"][0] == (8 if kind == "anchor" else 29)
    assert not (r1["G"][:, 1:4] if kind == "anchor" else r1["G"][1:4]).any()
    demb, _, dw, _ = P.grads(kind, x, w, r1["G"], r1["q"])
    assert not demb[1:4].any() and np.isfinite(r1["loss"])
    # a zero proxy: S = 0, no gradient row
    w0 = w.copy()
    w0[lab[0]] = 0
    r0 = P.reference(kind, x, w0, lab)
    assert r0["q"][lab[0]] == 0 and not r0["S"][:, lab[0]].any()
    demb, _, dw, _ = P.grads(kind, x, w0, r0["G"], r0["q"])
    assert not dw[lab[0]].any() and np.isfinite(dw).all() and np.isfinite(r0["loss"])
    # all samples of one class; all unlabelled
    same = np.full(32, 5)
    rs = P.reference(kind, x, w, same)
    assert rs["counts"][:2].tolist() == ([1, 32] if kind == "anchor" else [32, 32]) and np.isfinite(rs["loss"])
    if kind == "anchor":
        assert rs["counts"][2] == 0 and (rs["G"][np.arange(c) != 5] >= 0).all()          # N_5 is empty: no violation
    ru = P.reference(kind, x, w, np.full(32, -1))
    assert ru["loss"] == 0.0 and not ru["G"].any() and ru["counts"].tolist() == [0, 0, 0]


def test_stable_forms_hold_where_the_plain_ones_overflow():
    x, w, lab, _ = _case((8, 4, 256, 24))
    for kind in KINDS:
        ref = P.reference(kind, 30.0 * x, w, lab)
        assert np.isfinite(ref["loss"]) and np.isfinite(ref["G"]).all()
        bg, bl = P.bounds(ref, P.gamma_s("small", 256))
        assert np.isfinite(bg).all() and np.isfinite(bl)
    x, w, lab, a = P.underflow_trap()
    for kind in KINDS:
        ref = P.reference(kind, x, w, lab, a, 0.0)
        assert np.isfinite(ref["loss"]) and ref["loss"] > 0
    assert np.allclose(P.reference("softmax", x, w, lab, a, 0.0)["t"][0], [200.0, 40.0, 0.0])


def test_q_of_is_the_k_ordered_float64_chain():
    r = np.random.RandomState(1)
    w = (r.randn(5, 300) * r.uniform(1e-3, 1e3, size=(5, 1))).astype(np.float32)
    w[2] = 0
    q = P.q_of(w)
    for cl in range(5):
        ss = 0.0
        for k in range(300):
            ss += float(w[cl, k]) * float(w[cl, k])
        assert q[cl] == (np.float32(1.0 / math.sqrt(ss)) if ss > 0 else 0)
    assert q.dtype == np.float32 and q[2] == 0


# ---------------------------------------------------------------------------------------------------------------- 4. fitness
@pytest.mark.parametrize("shape", P.SHAPES + ["ragged"], ids=str)
def test_gpu_test_inputs_are_fit(shape):
    """On every shape of the GPU test, at the gamma_S of the path `auto` takes, no anchor's counter decision is open, the bounds are
    finite and small against the quantities they bound; the grid inputs are exact in any order and leave nothing open either."""
    x, w, lab, _ = _case(shape)
    n, c, e = x.shape[0], w.shape[0], x.shape[1]
    gs = P.gamma_s(P.auto_path(n, c, e), e)
    xg, wg, _, unit = _case(shape, grid=True)
    assert P.exact_in_any_order(xg, wg, unit)
    assert (P.q_of(w) > 0).all() and (P.q_of(wg) > 0).all()
    for kind in KINDS:
        for xx, ww, g in ((x, w, gs), (xg, wg, 0.0), (x, w, P.gamma_s("small", e) if P.auto_path(n, c, e) == "small" else gs)):
            d = P.decisions(kind, xx, ww, lab, g)
            assert not d["open"].any(), (kind, shape, int(d["open"].sum()))
            ref = P.reference(kind, xx, ww, lab)
            assert d["sure"].sum() == ref["counts"][2] == d["may"].sum()
            bg, bl = P.bounds(ref, g)
            assert np.isfinite(bg).all() and 0 < bl < 1e-2 * abs(ref["loss"])
    for kind in KINDS:                                       # the path-agreement shapes are judged at either path's gamma_S
        if shape in [(32, 4, 256, 100)]:
            for path in ("small", "matrix"):
                assert not P.decisions(kind, x, w, lab, P.gamma_s(path, e))["open"].any()
