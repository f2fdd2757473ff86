"""MAP@R / R-precision, host side (no GPU): the C ABI is declared and exported, arguments are refused before any launch, the
workspace size behaves, the float64 restatement (tests/retrieval_map_ref.py) gives the known answers on hand-made cases and agrees
with tests/retrieval_ref.py on the first positive, the inputs of the GPU interval test are fit for it, and the Python surface
(retrieval_map_metrics, calculate_map_at_r, TRAIN.retrieval_map) is there."""
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
NEW = ("embnet_retrieval_positive_ranks_workspace_bytes", "embnet_retrieval_positive_ranks", "embnet_retrieval_map_reduce")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_map_ref as MR  # noqa: E402
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
def test_header_declares_and_library_exports_positive_ranks():
    from embeddingnet_amd import _lib, ops
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported
    assert exported == set(protos)
    assert _l().embnet_abi_version() == 22
    header = open(os.path.join(ROOT, "include", "embnet.h")).read()
    assert "#define EMBNET_RETRIEVAL_R_MAX 4096" in header and ops.R_MAX == 4096
    for word in ("No [nq, n] buffer", "O(nq + n + num_classes + capacity)", "exact integer", "bitwise reproducible",
                 "no initialisation", "64x64, 128x128", "scalar for unaligned"):
        assert word in header, word


# ---- 2. argument refusal --------------------------------------------------------------------------------------------------
def _pr(nq=100, n=100, e=8, self_exclude=0, num_classes=10, capacity=1000, ws_bytes=None, **null):
    l = _l()
    a = dict(q=FAKE, ql=FAKE, x=FAKE, xl=FAKE, offset=FAKE, idx=FAKE, rank=FAKE, status=FAKE, ws=FAKE)
    a.update(null)
    ws_bytes = l.embnet_retrieval_positive_ranks_workspace_bytes(nq, n, num_classes, capacity) if ws_bytes is None else ws_bytes
    return l.embnet_retrieval_positive_ranks(a["q"], a["ql"], nq, a["x"], a["xl"], n, e, self_exclude, num_classes, capacity,
                                             a["offset"], a["idx"], a["rank"], a["status"], a["ws"], ws_bytes, None)


def _red(nq=100, **null):
    a = dict(offset=FAKE, rank=FAKE, a=FAKE, r=FAKE, ap=FAKE, sums=FAKE, nv=FAKE)
    a.update(null)
    return _l().embnet_retrieval_map_reduce(a["offset"], a["rank"], nq, a["a"], a["r"], a["ap"], a["sums"], a["nv"], None)


@pytest.mark.parametrize("fn,names", [(_pr, ("q", "ql", "x", "xl", "offset", "idx", "rank", "status", "ws")),
                                      (_red, ("offset", "rank", "a", "r", "ap", "sums", "nv"))])
def test_rejects_null_pointers(fn, names):
    for name in names:
        assert fn(**{name: None}) == -1 and "null pointer" in _err(), (fn.__name__, name)


def test_rejects_sizes_self_exclude_and_workspace():
    for kw in (dict(nq=0), dict(nq=-3), dict(n=0), dict(n=-1), dict(e=0), dict(e=-8), dict(num_classes=0), dict(num_classes=-2),
               dict(capacity=0), dict(capacity=-5)):
        assert _pr(ws_bytes=1 << 30, **kw) == -1 and "must be positive" in _err(), kw
    assert _pr(nq=100, n=101, self_exclude=1) == -1 and "self_exclude" in _err()
    need = _l().embnet_retrieval_positive_ranks_workspace_bytes(100, 100, 10, 1000)
    assert _pr(ws_bytes=need - 8) == -3 and "workspace" in _err()
    assert _pr(ws=FAKE + 4) == -1 and "aligned" in _err()
    assert _pr(offset=FAKE + 4) == -1 and "aligned" in _err()
    assert _pr(nq=1 << 20, n=16, e=1024) == -1 and "2 GiB" in _err()
    assert _pr(nq=16, n=1 << 20, e=1024) == -1 and "2 GiB" in _err()
    for kw in (dict(nq=0), dict(nq=-1)):
        assert _red(**kw) == -1 and "must be positive" in _err(), kw
    assert _red(sums=FAKE + 4) == -1 and "aligned" in _err()


def test_workspace_bytes():
    f = _l().embnet_retrieval_positive_ranks_workspace_bytes
    for args in ((0, 10, 10, 10), (10, 0, 10, 10), (10, 10, 0, 10), (10, 10, 10, 0), (-1, 10, 10, 10), (10, 10, 10, -4)):
        assert f(*args) == 0, args
    sizes = [f(1000, 2000, 50, c) for c in (1, 2, 100, 1000, 19000, 1 << 20)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert all(s % 16 == 0 for s in sizes)
    n, c = 1 << 20, 1 << 22                                 # O(nq + n + num_classes + capacity): 12 bytes per unit of capacity, 4 per
    assert 12 * c <= f(n, n, n, c) <= 12 * c + 24 * n + 256   # class, norms + slots + 2 bytes of label filter per row
    assert f(n, n, 1, c) < f(n, n, n, c)


# ---- 3. the restatement on cases with known answers ---------------------------------------------------------------------------
def _case(x, lab, self_exclude=True, q=None, ql=None):
    x = np.asarray(x, np.float64)
    q = x if q is None else np.asarray(q, np.float64)
    ql = lab if ql is None else ql
    off, idx, pos = MR.positions_exact(RR.sqdist64(q, x), ql, lab, self_exclude)
    return off, idx, pos, MR.metrics_from_positions(off, pos)


def test_restatement_perfect_ranking():
    x = [[0.], [1.], [2.], [100.], [101.], [102.]]
    off, idx, pos, m = _case(x, np.array([0, 0, 0, 1, 1, 1]))
    assert off.tolist() == [0, 2, 4, 6, 8, 10, 12] and pos.tolist() == [1, 2] * 6
    assert m["map@r"] == 1.0 and m["r_precision"] == 1.0 and m["map"] == 1.0 and m["n_valid"] == 6 and m["n_queries"] == 6
    assert np.all(m["ap@r"] == 1.0) and m["r"].tolist() == [2] * 6


def test_restatement_line_of_six():
    # labels a a b a b b on a line (test_retrieval_cpu.py's example): every positive's position, by hand
    x = [[0.], [1.], [2.], [4.], [7.], [11.]]
    off, idx, pos, m = _case(x, np.array([0, 0, 1, 0, 1, 1]))
    assert off.tolist() == [0, 2, 4, 6, 8, 10, 12]
    assert idx.tolist() == [1, 3, 0, 3, 4, 5, 1, 0, 5, 2, 4, 2]
    assert pos.tolist() == [1, 3, 1, 3, 4, 5, 2, 4, 2, 3, 1, 3]
    want_apr = [(1 / 1) / 2, (1 / 1) / 2, 0.0, (1 / 2) / 2, (1 / 2) / 2, (1 / 1) / 2]
    want_ap = [(1 + 2 / 3) / 2, (1 + 2 / 3) / 2, (1 / 4 + 2 / 5) / 2, (1 / 2 + 2 / 4) / 2, (1 / 2 + 2 / 3) / 2, (1 + 2 / 3) / 2]
    assert np.allclose(m["ap@r"], want_apr, rtol=0, atol=1e-15) and np.allclose(m["ap"], want_ap, rtol=0, atol=1e-15)
    assert m["r_precision_q"].tolist() == [0.5, 0.5, 0.0, 0.5, 0.5, 0.5]
    assert abs(m["map@r"] - sum(want_apr) / 6) < 1e-15 and abs(m["r_precision"] - 2.5 / 6) < 1e-15
    assert abs(m["map"] - sum(want_ap) / 6) < 1e-15
    # query 2 (label b at 2.): its first positive sits at position 4 > R = 2 -> ap@r 0 but ap > 0
    assert m["ap@r"][2] == 0.0 and m["ap"][2] > 0 and m["r_precision_q"][2] == 0.0


def test_restatement_ties_go_to_the_smaller_index():
    x = np.zeros((5, 3))                                    # five copies of one point: the order is the index order
    off, idx, pos, m = _case(x, np.array([0, 1, 1, 0, 1]))
    assert idx.tolist() == [3, 2, 4, 1, 4, 0, 1, 2] and pos.tolist() == [3, 2, 4, 2, 4, 1, 2, 3]
    assert m["ap@r"].tolist() == [0.0, 0.25, 0.25, 1.0, 0.25] and m["ap"][0] == 1 / 3
    off, idx, pos, _ = _case(x, np.array([0, 1, 1, 0, 1]), self_exclude=False)
    assert idx.tolist() == [0, 3, 1, 2, 4, 1, 2, 4, 0, 3, 1, 2, 4] and pos.tolist() == [1, 4, 2, 3, 5, 2, 3, 5, 1, 4, 2, 3, 5]


def test_restatement_queries_without_a_positive_and_nan():
    x = [[0.], [1.], [5.]]
    off, idx, pos, m = _case(x, np.array([0, 0, 7]))
    assert off.tolist() == [0, 1, 2, 2] and math.isnan(m["ap@r"][2]) and math.isnan(m["ap"][2]) and math.isnan(m["r_precision_q"][2])
    assert m["n_valid"] == 2 and m["n_queries"] == 3 and m["map@r"] == 1.0 and m["r"].tolist() == [1, 1, 0]
    off, idx, pos, m = _case(x, np.array([0, 0, 7]), self_exclude=False, q=[[0.9], [4.]], ql=np.array([7, 3]))
    assert off.tolist() == [0, 1, 1] and idx.tolist() == [2] and pos.tolist() == [3] and m["ap@r"][0] == 0.0 and m["ap"][0] == 1 / 3
    e = MR.metrics_from_positions(np.zeros(4, np.int64), np.zeros(0, np.int32))
    assert math.isnan(e["map@r"]) and math.isnan(e["r_precision"]) and math.isnan(e["map"]) and e["n_valid"] == 0 and e["n_queries"] == 0
    d2 = np.array([[np.nan, 1.0, 2.0], [np.nan, np.nan, np.nan]])      # NaN counts as +inf, ties by index
    off, idx, pos = MR.positions_exact(d2, [0, 1], [0, 1, 1], False)
    assert idx.tolist() == [0, 1, 2] and pos.tolist() == [3, 2, 3]


def test_first_position_is_the_rank_of_the_existing_restatement():
    rs = np.random.RandomState(3)
    for self_exclude in (True, False):
        x = rs.randint(0, 4, size=(90, 6)).astype(np.float64)              # integer rows: many equal distances
        lab = rs.randint(0, 12, size=90)
        q, ql = (x, lab) if self_exclude else (rs.randint(0, 4, size=(40, 6)).astype(np.float64), rs.randint(0, 14, size=40))
        d2 = RR.sqdist64(q, x)
        off, idx, pos = MR.positions_exact(d2, ql, lab, self_exclude)
        rank, first, _ = RR.ranks_exact(d2, ql, lab, self_exclude)
        has = np.diff(off) > 0
        assert np.array_equal(has, rank > 0)
        assert np.array_equal(pos[off[:-1][has]], rank[has]) and np.array_equal(idx[off[:-1][has]], first[has])
        for i in range(len(q)):
            assert np.all(np.diff(pos[off[i]:off[i + 1]]) > 0)
    g, gl, _, _ = R.knn_data(12, 6, 16, 1.2, 4, 3)
    off, idx, lo, hi = MR.position_interval(g, g, gl, gl, True, _A(16))
    eo, eidx, epos = MR.positions_exact(RR.sqdist64(g, g), gl, gl, True)
    o0, i0, lo0, hi0 = MR.position_interval(g, g, gl, gl, True, 0.0)
    assert np.array_equal(off, eo) and np.array_equal(o0, eo) and np.array_equal(lo0, hi0)
    for i in range(len(g)):                                                # index order there, position order here
        seg = slice(off[i], off[i + 1])
        by_index = np.argsort(eidx[seg])
        assert np.array_equal(idx[seg], eidx[seg][by_index]) and np.array_equal(lo0[seg], epos[seg][by_index])
        assert np.all(lo[seg] <= epos[seg][by_index]) and np.all(epos[seg][by_index] <= hi[seg])
    lower, upper = MR.metric_bounds(off, lo, hi)
    exact = MR.metrics_from_positions(eo, epos)
    for key in ("map@r", "r_precision", "map"):
        assert lower[key] <= exact[key] <= upper[key], key


# ---- 4. input fitness ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (5, 77))
def test_interval_inputs_are_fit(seed):
    """The GPU interval test is only as sharp as its intervals.  Measured in float64 with A = 2e-6: 14.2 % / 14.1 % of the 115 900
    positives have an interval wider than one position, the largest width is 6 / 5, MAP@R lies in [0.16299, 0.16313] /
    [0.16617, 0.16631]."""
    g, gl, _, _ = R.knn_data(305, 20, 256, 1.2, 10, seed)
    assert g.shape == (6100, 256)
    off, idx, lo, hi = MR.position_interval(g, g, gl, gl, True, _A(256))
    assert len(idx) == 115900 and off[-1] == 115900
    lower, upper = MR.metric_bounds(off, lo, hi)
    share, width = float(np.mean(hi > lo)), int((hi - lo).max())
    print(f"seed {seed}: open share {share:.4%}, max width {width}, map@r in [{lower['map@r']:.5f}, {upper['map@r']:.5f}], "
          f"r_precision in [{lower['r_precision']:.5f}, {upper['r_precision']:.5f}], map in [{lower['map']:.5f}, {upper['map']:.5f}]")
    assert share <= 0.16 and width <= 8
    for key in ("map@r", "r_precision", "map"):
        assert 0 <= upper[key] - lower[key] < 3e-4, key
    assert 0.05 < lower["map@r"] < 0.9


# ---- 5. Python surface ---------------------------------------------------------------------------------------------------------
def test_alias_and_signatures():
    import embedding_net.retrieval
    import embeddingnet_amd.retrieval as M
    assert embedding_net.retrieval.retrieval_map_metrics is M.retrieval_map_metrics
    sig = inspect.signature(M.retrieval_map_metrics)
    assert list(sig.parameters) == ["encodings", "labels", "gallery", "gallery_labels", "device"]
    assert all(p.default is None for name, p in sig.parameters.items() if name != "encodings")
    from embeddingnet_amd import ops
    sig = inspect.signature(ops.retrieval_positive_ranks)
    assert list(sig.parameters) == ["q", "q_labels", "x", "x_labels", "num_classes", "capacity"]
    assert all(p.default is None for name, p in sig.parameters.items() if name not in ("q", "q_labels"))
    assert list(inspect.signature(ops.retrieval_map_reduce).parameters) == ["offset", "pos_rank"]
    from embeddingnet_amd.models import EmbeddingNet
    sig = inspect.signature(EmbeddingNet.calculate_map_at_r)
    assert list(sig.parameters) == ["self", "data_loader", "gallery", "batch_size"]
    assert sig.parameters["gallery"].default == "val" and sig.parameters["batch_size"].default == 256


def test_retrieval_map_metrics_value_errors():
    from embeddingnet_amd.retrieval import retrieval_map_metrics
    x = np.zeros((4, 3), np.float32)
    lab = ["a", "b", "a", "b"]
    with pytest.raises(ValueError, match="labels"):
        retrieval_map_metrics(x, lab[:3])
    with pytest.raises(ValueError, match="labels are needed"):
        retrieval_map_metrics(x)
    with pytest.raises(ValueError, match="gallery labels"):
        retrieval_map_metrics(x, lab, gallery=x, gallery_labels=lab[:2])
    with pytest.raises(ValueError, match="come together"):
        retrieval_map_metrics(x, lab, gallery=x)
    with pytest.raises(ValueError, match="widths differ"):
        retrieval_map_metrics(x, lab, gallery=np.zeros((4, 5), np.float32), gallery_labels=lab, device="cpu")
    with pytest.raises(ValueError, match=r"\[rows, e\]"):
        retrieval_map_metrics(np.zeros(4, np.float32), lab, device="cpu")
    with pytest.raises(ValueError, match="retrieval_map_metrics"):
        retrieval_map_metrics({"encodings": x, "labels": lab[:1]})
    # a class above R_MAX is refused by name and size before the library is reached
    big = np.zeros((4098, 2), np.float32)
    with pytest.raises(ValueError, match=r"'crowd' has 4098 gallery items"):
        retrieval_map_metrics(big, ["crowd"] * 4098, device="cpu")


def test_train_cli_lets_the_key_through_and_checks_it():
    import yaml
    from embeddingnet_amd.utils import parse_params
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "simple2_map_synthetic.yml")))
    stock = yaml.safe_load(open(os.path.join(ROOT, "configs", "simple2_synthetic.yml")))
    assert cfg["TRAIN"]["retrieval_map"] is True and cfg["TRAIN"]["monitor"] == "val_map@r"
    rest = {k: v for k, v in cfg["TRAIN"].items() if k not in ("retrieval_map", "monitor")}
    assert rest == stock["TRAIN"]
    assert cfg["GENERAL"]["project_name"] == "simple2_map_synthetic"
    for section in stock:
        if section not in ("TRAIN", "GENERAL"):
            assert cfg[section] == stock[section], section
    params = parse_params(os.path.join(ROOT, "configs", "simple2_map_synthetic.yml"))
    assert params["train"]["retrieval_map"] is True and params["train"]["monitor"] == "val_map@r"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train as T
    assert T.retrieval_map_config({"retrieval_map": True}, True) is True
    assert T.retrieval_map_config({}, True) is False and T.retrieval_map_config({"retrieval_map": False}, False) is False
    assert T.monitor_config({"retrieval_map": True, "monitor": "val_map@r"}, True) == ([], "val_map@r")
    assert T.monitor_config({"retrieval_map": True, "monitor": "val_r_precision", "retrieval_ks": [1]}, True) == ([1], "val_r_precision")
    assert T.monitor_config({"retrieval_map": True}, True) == ([], "val_loss")
    for name in ("val_map@r", "val_r_precision"):
        with pytest.raises(ValueError, match="retrieval_map"):
            T.monitor_config({"monitor": name}, True)
        with pytest.raises(ValueError, match="retrieval_map"):
            T.monitor_config({"monitor": name, "retrieval_ks": [1, 5]}, True)
        with pytest.raises(ValueError, match="validation"):
            T.monitor_config({"retrieval_map": True, "monitor": name}, False)
    with pytest.raises(ValueError, match="validation"):
        T.retrieval_map_config({"retrieval_map": True}, False)
    with pytest.raises(ValueError, match="true or false"):
        T.retrieval_map_config({"retrieval_map": "yes"}, True)
