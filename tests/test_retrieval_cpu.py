"""Retrieval evaluation, host side (no GPU): the C ABI is declared and exported, arguments are refused before any launch, the
float64 restatement (tests/retrieval_ref.py) gives the known answers on hand-made cases, the inputs of the GPU interval test are
fit for it (few queries whose rank the error bound leaves open), and the Python surface is there."""
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import recipes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_retrieval_workspace_bytes", "embnet_retrieval_first_positive", "embnet_retrieval_reduce")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_ref as RR  # noqa: E402


def _A(e):
    """tests/test_eval_path_gpu.py::_A, verbatim: the project's bound on |d2_gpu - d2_f64| / (|q|^2 + |x|^2)."""
    return 2e-6 if e <= 512 else 4e-6 * (e / 512) ** 0.5


def _l():
    from embeddingnet_amd import _lib
    return _lib.lib()


def _err():
    return _l().embnet_last_error().decode()


# ---- 1. header and exports ----------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_retrieval():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported
    assert exported == set(protos)
    assert _l().embnet_abi_version() == 22


# ---- 2. argument refusal --------------------------------------------------------------------------------------------------
def _fp(nq=100, n=100, e=8, self_exclude=0, ws_bytes=None, **null):
    l = _l()
    a = dict(q=FAKE, ql=FAKE, x=FAKE, xl=FAKE, rank=FAKE, pos=FAKE, d2=FAKE, ws=FAKE)
    a.update(null)
    ws_bytes = l.embnet_retrieval_workspace_bytes(nq, n) if ws_bytes is None else ws_bytes
    return l.embnet_retrieval_first_positive(a["q"], a["ql"], nq, a["x"], a["xl"], n, e, self_exclude, a["rank"], a["pos"],
                                             a["d2"], a["ws"], ws_bytes, None)


def _red(nq=100, nk=3, **null):
    a = dict(rank=FAKE, ks=FAKE, hits=FAKE, nv=FAKE, s=FAKE)
    a.update(null)
    return _l().embnet_retrieval_reduce(a["rank"], nq, a["ks"], nk, a["hits"], a["nv"], a["s"], None)


@pytest.mark.parametrize("fn,names", [(_fp, ("q", "ql", "x", "xl", "rank", "pos", "d2", "ws")),
                                      (_red, ("rank", "ks", "hits", "nv", "s"))])
def test_rejects_null_pointers(fn, names):
    for name in names:
        assert fn(**{name: None}) == -1 and "null pointer" in _err(), (fn.__name__, name)


def test_rejects_sizes_self_exclude_and_workspace():
    for kw in (dict(nq=0), dict(nq=-3), dict(n=0), dict(n=-1), dict(e=0), dict(e=-8)):
        assert _fp(ws_bytes=1 << 30, **kw) == -1 and "must be positive" in _err(), kw
    assert _fp(nq=100, n=101, self_exclude=1) == -1 and "self_exclude" in _err()
    assert _fp(nq=100, n=101, self_exclude=0, e=-1) == -1
    need = _l().embnet_retrieval_workspace_bytes(100, 100)
    assert need >= 100 * (8 + 4 + 4) + 100 * 4
    assert _fp(ws_bytes=need - 8) == -3 and "workspace" in _err()
    assert _fp(ws=FAKE + 4) == -1 and "aligned" in _err()
    assert _fp(nq=1 << 20, n=16, e=1024) == -1 and "2 GiB" in _err()
    assert _fp(nq=16, n=1 << 20, e=1024) == -1 and "2 GiB" in _err()
    for kw in (dict(nq=0), dict(nq=-1), dict(nk=0), dict(nk=-2)):
        assert _red(**kw) == -1 and "must be positive" in _err(), kw


def test_workspace_bytes():
    l = _l()
    assert l.embnet_retrieval_workspace_bytes(0, 1000) == 0 and l.embnet_retrieval_workspace_bytes(1000, 0) == 0
    assert l.embnet_retrieval_workspace_bytes(-1, 5) == 0
    n = 1 << 20                                             # O(nq + n): norms, a 64-bit key and a counter per query, 2 bytes per
    assert 20 * n <= l.embnet_retrieval_workspace_bytes(n, n) <= 24 * n + 64          # row of label filters
    assert l.embnet_retrieval_workspace_bytes(n, n) % 16 == 0


def test_ks_below_one_is_refused_before_the_library_is_reached():
    """ks lives in device memory, so the C entry cannot read it: the Python wrapper refuses K < 1 (before it touches its
    tensor arguments, so a CPU-only machine can check it)."""
    import torch
    from embeddingnet_amd import _lib, ops
    rank = torch.tensor([1, 2, 0], dtype=torch.int32)
    for ks in ((1, 0), (-1,), (5, 0, 10)):
        with pytest.raises(_lib.EmbnetError, match="K must be >= 1"):
            ops.retrieval_reduce(rank, ks)


# ---- 3. the restatement on cases with known answers ---------------------------------------------------------------------------
def test_restatement_line_of_six():
    # labels a a b a b b on a line: every query's nearest same-class point and the other-class points in front of it, by hand
    x = np.array([[0.], [1.], [2.], [4.], [7.], [11.]])
    lab = np.array([0, 0, 1, 0, 1, 1])
    rank, pos, d2 = RR.ranks_exact(RR.sqdist64(x, x), lab, lab, True)
    assert rank.tolist() == [1, 1, 4, 2, 2, 1]
    assert pos.tolist() == [1, 0, 4, 1, 5, 4]
    assert d2.tolist() == [1., 1., 25., 9., 16., 16.]
    m = RR.metrics(rank, (1, 2, 1000))
    assert m["recall@1"] == 3 / 6 and m["recall@2"] == 5 / 6 and m["recall@1000"] == 1.0
    assert abs(m["mrr"] - (1 + 1 + 0.25 + 0.5 + 0.5 + 1) / 6) < 1e-15 and m["n_valid"] == 6 and m["n_queries"] == 6


def test_restatement_ties_go_to_the_smaller_index():
    # four copies of one point: d2 = 0 everywhere, the order is the index order
    x = np.zeros((4, 3))
    rank, pos, d2 = RR.ranks_exact(RR.sqdist64(x, x), [0, 1, 1, 0], [0, 1, 1, 0], True)
    assert rank.tolist() == [3, 2, 2, 1] and pos.tolist() == [3, 2, 1, 0] and d2.tolist() == [0., 0., 0., 0.]
    # without exclusion every query finds itself or an earlier copy
    rank, pos, _ = RR.ranks_exact(RR.sqdist64(x, x), [0, 1, 1, 0], [0, 1, 1, 0], False)
    assert rank.tolist() == [1, 2, 2, 1] and pos.tolist() == [0, 1, 1, 0]


def test_restatement_class_of_one_and_separate_gallery():
    x = np.array([[0.], [1.], [5.]])
    rank, pos, d2 = RR.ranks_exact(RR.sqdist64(x, x), [0, 0, 7], [0, 0, 7], True)
    assert rank.tolist() == [1, 1, 0] and pos.tolist() == [1, 0, -1] and d2[2] == np.inf
    m = RR.metrics(rank, (1,))
    assert m["n_valid"] == 2 and m["n_queries"] == 3 and m["recall@1"] == 1.0 and m["mrr"] == 1.0
    # a separate gallery: nothing excluded, a label the gallery lacks gives rank 0
    q = np.array([[0.9], [4.], [4.]])
    rank, pos, d2 = RR.ranks_exact(RR.sqdist64(q, x), [7, 0, 3], [0, 0, 7], False)
    assert rank.tolist() == [3, 2, 0] and pos.tolist() == [2, 1, -1]
    e = RR.metrics(np.zeros(4, np.int32), (1, 5))
    assert math.isnan(e["recall@1"]) and math.isnan(e["mrr"]) and e["n_valid"] == 0 and e["n_queries"] == 0


def test_restatement_nan_counts_as_inf_and_interval_brackets_the_exact_rank():
    d2 = np.array([[np.nan, 1.0, 2.0], [np.nan, np.nan, np.nan]])
    rank, pos, pd = RR.ranks_exact(d2, [0, 1], [0, 1, 1], False)
    assert rank.tolist() == [3, 2] and pos.tolist() == [0, 1] and np.isinf(pd).all()   # (inf, 0) precedes (inf, 1)
    g, gl, _, _ = R.knn_data(12, 6, 16, 1.2, 4, 3)
    lo, hi, det = RR.rank_interval(g, g, gl, gl, True, _A(16), details=True)
    assert np.all(lo <= det["rank"]) and np.all(det["rank"] <= hi)
    lo0, hi0 = RR.rank_interval(g, g, gl, gl, True, 0.0)
    assert np.array_equal(lo0, det["rank"]) and np.array_equal(hi0, det["rank"])


# ---- 4. input fitness ----------------------------------------------------------------------------------------------------------
FITNESS_SEEDS = (5, 77)


@pytest.mark.parametrize("seed", FITNESS_SEEDS)
def test_interval_inputs_are_fit(seed):
    """The GPU interval test is only as sharp as its intervals: on its inputs nearly every query must have r_lo == r_hi."""
    g, gl, _, _ = R.knn_data(305, 20, 256, 1.2, 10, seed)
    assert g.shape == (6100, 256)
    lo, hi, det = RR.rank_interval(g, g, gl, gl, True, _A(256), details=True)
    share, width = float(np.mean(lo != hi)), int((hi - lo).max())
    m = RR.metrics(det["rank"], (1, 10, 100))
    print(f"seed {seed}: ambiguous share {share:.4%}, width {width}, R@1 {m['recall@1']:.3f}, R@10 {m['recall@10']:.3f}, "
          f"R@100 {m['recall@100']:.3f}, max rank {det['rank'].max()}")
    assert share <= 0.01 and width <= 2
    assert 0.3 < m["recall@1"] < 0.9
    assert det["rank"].max() > 64


def test_separable_sanity_case():
    g, gl, _, _ = R.knn_data(40, 10, 64, 0.3, 10, 5)
    rank, _, _ = RR.ranks_exact(RR.sqdist64(g, g), gl, gl, True)
    assert RR.metrics(rank, (1,))["recall@1"] == 1.0


# ---- 5. Python surface ---------------------------------------------------------------------------------------------------------
def test_alias_and_signature():
    import embedding_net.retrieval
    import embeddingnet_amd.retrieval as M
    import embedding_net
    assert embedding_net.retrieval is M
    assert embedding_net.retrieval.retrieval_metrics is M.retrieval_metrics
    sig = inspect.signature(M.retrieval_metrics)
    assert list(sig.parameters) == ["encodings", "labels", "ks", "gallery", "gallery_labels", "device"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["labels"] is None and d["ks"] == (1, 5, 10) and d["gallery"] is None and d["gallery_labels"] is None
    assert d["device"] is None
    from embeddingnet_amd import ops
    assert list(inspect.signature(ops.retrieval_first_positive).parameters)[:4] == ["q", "q_labels", "x", "x_labels"]
    assert list(inspect.signature(ops.retrieval_reduce).parameters) == ["rank", "ks"]


def test_retrieval_metrics_value_errors():
    from embeddingnet_amd.retrieval import retrieval_metrics
    x = np.zeros((4, 3), np.float32)
    lab = ["a", "b", "a", "b"]
    with pytest.raises(ValueError, match="ks is empty"):
        retrieval_metrics(x, lab, ks=())
    with pytest.raises(ValueError, match=">= 1"):
        retrieval_metrics(x, lab, ks=(1, 0))
    with pytest.raises(ValueError, match=">= 1"):
        retrieval_metrics({"encodings": x, "labels": lab}, ks=(-5,))
    with pytest.raises(ValueError, match="labels"):
        retrieval_metrics(x, lab[:3])
    with pytest.raises(ValueError, match="labels are needed"):
        retrieval_metrics(x)
    with pytest.raises(ValueError, match="gallery labels"):
        retrieval_metrics(x, lab, gallery=x, gallery_labels=lab[:2])
    with pytest.raises(ValueError, match="come together"):
        retrieval_metrics(x, lab, gallery=x)
    with pytest.raises(ValueError, match="widths differ"):
        retrieval_metrics(x, lab, gallery=np.zeros((4, 5), np.float32), gallery_labels=lab, device="cpu")
    with pytest.raises(ValueError, match=r"\[rows, e\]"):
        retrieval_metrics(np.zeros(4, np.float32), lab, device="cpu")


def test_model_method_signature():
    from embeddingnet_amd.models import EmbeddingNet
    sig = inspect.signature(EmbeddingNet.calculate_retrieval_metrics)
    assert list(sig.parameters) == ["self", "data_loader", "ks", "gallery", "batch_size"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["ks"] == (1, 5, 10) and d["gallery"] == "val" and d["batch_size"] == 256


def test_train_cli_lets_the_keys_through_and_checks_them(tmp_path):
    import yaml
    from embeddingnet_amd.utils import parse_params
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "simple2_retrieval_synthetic.yml")))
    stock = yaml.safe_load(open(os.path.join(ROOT, "configs", "simple2_synthetic.yml")))
    assert cfg["TRAIN"]["retrieval_ks"] == [1, 5, 10] and cfg["TRAIN"]["monitor"] == "val_recall@1"
    rest = {k: v for k, v in cfg["TRAIN"].items() if k not in ("retrieval_ks", "monitor")}
    assert rest == stock["TRAIN"]
    assert cfg["GENERAL"]["project_name"] == "simple2_retrieval_synthetic"
    for section in stock:
        if section not in ("TRAIN", "GENERAL"):
            assert cfg[section] == stock[section], section
    params = parse_params(os.path.join(ROOT, "configs", "simple2_retrieval_synthetic.yml"))
    assert params["train"]["retrieval_ks"] == [1, 5, 10] and params["train"]["monitor"] == "val_recall@1"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train as T
    assert T.monitor_config({"retrieval_ks": [1, 5], "monitor": "val_recall@5"}, True) == ([1, 5], "val_recall@5")
    assert T.monitor_config({}, True) == ([], "val_loss") and T.monitor_config({}, False) == ([], "loss")
    with pytest.raises(ValueError, match="retrieval_ks"):
        T.monitor_config({"retrieval_ks": [1, 5], "monitor": "val_recall@10"}, True)
    with pytest.raises(ValueError, match="validation"):
        T.monitor_config({"retrieval_ks": [1], "monitor": "val_recall@1"}, False)
    with pytest.raises(ValueError, match="monitor"):
        T.monitor_config({"monitor": "val_banana"}, True)
    with pytest.raises(ValueError, match=">= 1"):
        T.monitor_config({"retrieval_ks": [0]}, True)
