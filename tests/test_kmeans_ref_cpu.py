"""k-means and the clustering scores, host side (no GPU): the C ABI is declared and exported, arguments are refused before any
launch, the workspace size behaves, the float64 restatement (tests/kmeans_ref.py) gives the known answers on hand-made cases and
scikit-learn's recorded ones (tests/golden/kmeans.npz), the inputs of the GPU tests are fit for their assertions, the scores of
embeddingnet_amd.clustering equal scikit-learn's recorded values, and the Python surface (KMeans, clustering_metrics,
calculate_clustering_metrics, TRAIN.clustering_nmi) is there."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_kmeans_workspace_bytes", "embnet_kmeans_assign", "embnet_kmeans_update", "embnet_kmeans_pp_update",
       "embnet_kmeans_pp_pick")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_ref as KR  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "kmeans.npz"))


def _l():
    from embeddingnet_amd import _lib
    return _lib.lib()


def _err():
    return _l().embnet_last_error().decode()


# ---- 1. header and exports ----------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_kmeans():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported
    assert exported == set(protos)
    assert _l().embnet_abi_version() == 22
    header = open(os.path.join(ROOT, "include", "embnet.h")).read()
    for word in ("ties go to the smaller index, exactly", "No [n,k] matrix", "keeps its centre bit for bit", "plain D^2 sampling",
                 "the same bits"):
        assert word in header, word


# ---- 2. argument refusal --------------------------------------------------------------------------------------------------
def _assign(n=100, k=10, e=8, ws_bytes=None, **over):
    l = _l()
    a = dict(x=FAKE, c=FAKE, prev=None, labels=FAKE, d2=FAKE, changed=FAKE, inertia=FAKE, ws=FAKE)
    a.update(over)
    ws_bytes = l.embnet_kmeans_workspace_bytes(n, k, e) if ws_bytes is None else ws_bytes
    return l.embnet_kmeans_assign(a["x"], n, a["c"], k, e, 0, a["prev"], a["labels"], a["d2"], a["changed"], a["inertia"], a["ws"],
                                  ws_bytes, None)


def _update(n=100, k=10, e=8, ws_bytes=None, **over):
    l = _l()
    a = dict(x=FAKE, labels=FAKE, c=FAKE, out=FAKE, count=FAKE, shift=FAKE, empty=FAKE, ws=FAKE)
    a.update(over)
    ws_bytes = l.embnet_kmeans_workspace_bytes(n, k, e) if ws_bytes is None else ws_bytes
    return l.embnet_kmeans_update(a["x"], a["labels"], n, a["c"], k, e, a["out"], a["count"], a["shift"], a["empty"], a["ws"],
                                  ws_bytes, None)


def _pp_update(n=100, e=8, **over):
    a = dict(x=FAKE, index=FAKE, mind2=FAKE)
    a.update(over)
    return _l().embnet_kmeans_pp_update(a["x"], n, e, a["index"], 1, a["mind2"], None)


def _pp_pick(n=100, draw=1, **over):
    a = dict(mind2=FAKE, index=FAKE, u=FAKE)
    a.update(over)
    return _l().embnet_kmeans_pp_pick(a["mind2"], n, 7, draw, a["index"], a["u"], None)


@pytest.mark.parametrize("fn,names", [(_assign, ("x", "c", "labels", "d2", "changed", "inertia", "ws")),
                                      (_update, ("x", "labels", "c", "out", "count", "shift", "empty", "ws")),
                                      (_pp_update, ("x", "index", "mind2")),
                                      (_pp_pick, ("mind2", "index", "u"))])
def test_rejects_null_pointers(fn, names):
    for name in names:
        assert fn(**{name: None}) == -1 and "null pointer" in _err(), (fn.__name__, name)


@pytest.mark.parametrize("fn", [_assign, _update])
def test_rejects_sizes_and_workspace(fn):
    for kw in (dict(n=0), dict(n=-3), dict(k=0), dict(k=-1), dict(e=0), dict(e=-8)):
        assert fn(ws_bytes=1 << 30, **kw) == -1 and "must be positive" in _err(), kw
    assert fn(n=10, k=11, ws_bytes=1 << 30) == -1 and "k=11 exceeds n=10" in _err()
    need = _l().embnet_kmeans_workspace_bytes(100, 10, 8)
    assert fn(ws_bytes=need - 8) == -3 and "workspace" in _err()
    assert fn(ws=FAKE + 4) == -1 and "aligned" in _err()
    assert fn(n=1 << 20, k=16, e=1024) == -1 and "2 GiB" in _err()
    assert fn(n=1 << 21, k=1 << 20, e=512) == -1 and "2 GiB" in _err()


def test_rejects_the_rest():
    assert _assign(inertia=FAKE + 4) == -1 and "aligned" in _err()
    assert _update(shift=FAKE + 4) == -1 and "aligned" in _err()
    for kw in (dict(n=0), dict(e=0), dict(n=-2)):
        assert _pp_update(**kw) == -1 and "must be positive" in _err(), kw
    assert _pp_update(n=1 << 20, e=1024) == -1 and "2 GiB" in _err()
    assert _pp_pick(n=0) == -1 and "positive" in _err()
    assert _pp_pick(draw=-1) == -1 and "non-negative" in _err()
    assert _pp_pick(u=FAKE + 4) == -1 and "aligned" in _err()


def test_workspace_bytes():
    f = _l().embnet_kmeans_workspace_bytes
    for args in ((0, 1, 8), (10, 0, 8), (10, 5, 0), (-1, 1, 8), (10, 11, 8)):
        assert f(*args) == 0, args
    sizes = [f(100000, k, 64) for k in (1, 10, 1000, 100000)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert all(s % 16 == 0 for s in sizes)
    n, k, e = 1 << 18, 4096, 512                             # O(n + (n / 512 + k) e): the f64 chunk partials dominate
    assert 8 * (n // 512 + k) * e <= f(n, k, e) <= 8 * (n // 512 + k) * e + 32 * n + 64 * k + 4096


# ---- 3. the restatement on cases with known answers -------------------------------------------------------------------------
def test_assign64_ties_nan_and_update64():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [4.0, 0.0], [5.0, 0.0]], np.float32)
    c = np.array([[0.5, 0.0], [0.5, 0.0], [np.nan, 0.0], [4.5, 0.0]], np.float32)
    labels, d2 = KR.assign64(x, c)
    assert labels.tolist() == [0, 0, 3, 3] and np.allclose(d2, 0.25)         # equal rows: the smaller index; NaN never chosen
    assert KR.assign64(x, np.full((2, 2), np.nan, np.float32))[0].tolist() == [0, 0, 0, 0]
    new, counts, u = KR.update64(x, labels, c)
    assert counts.tolist() == [2, 0, 0, 2]
    assert np.array_equal(new[0], [0.5, 0.0]) and np.array_equal(new[3], [4.5, 0.0])
    assert np.array_equal(new[1], c[1].astype(np.float64)) and np.isnan(new[2, 0])      # empty clusters keep their row
    assert (u[1] == 0).all() and (u[0] > 0).all()
    d = KR.d64(x, c[[0, 3]])
    b = KR.bound(x, c[[0, 3]])
    assert not KR.ambiguous(d, b).any()
    assert KR.labels_acceptable(d, b, np.array([0, 0, 1, 1])).all()
    assert not KR.labels_acceptable(d, b, np.array([1, 0, 1, 1]))[0]
    mid = np.array([[2.5, 0.0]], np.float32)                                  # equidistant: ambiguous, both labels accepted
    dm, bm = KR.d64(mid, c[[0, 3]]), KR.bound(mid, c[[0, 3]])
    assert KR.ambiguous(dm, bm).all() and KR.labels_acceptable(dm, bm, np.array([1])).all()


def test_lloyd64_two_obvious_clusters():
    x = np.array([[0, 0], [0, 1], [10, 0], [10, 1], [0, 2]], np.float32)
    r = KR.lloyd64(x, x[[0, 2]], check=True)
    assert r["labels"].tolist() == [0, 0, 1, 1, 0] and r["n_empty_max"] == 0
    assert np.allclose(r["centres"], [[0, 1], [10, 0.5]]) and np.isclose(r["inertia"], 2.5)
    assert r["n_iter"] == 2                                                  # the pass that assigns and the one that confirms


def test_draws_and_pick64():
    assert KR.rng_u32(0, 0, 0) == KR.rng_u32(0, 0, 0) != KR.rng_u32(1, 0, 0)
    us = [KR.draw_u(5, j) for j in range(1, 200)]
    assert all(0.0 <= u < 1.0 for u in us) and len(set(us)) == 199 and 0.35 < np.mean(us) < 0.65
    assert all((u * 2.0 ** 53) == int(u * 2.0 ** 53) for u in us)
    w = np.array([0, 0, 3, 0, 1, 0], np.float32)
    assert [KR.pick64(w, u)[0] for u in (0.0, 0.5, 0.74, 0.75, 0.99)] == [2, 2, 2, 4, 4]      # zero weights are never drawn
    assert KR.pick64(np.zeros(10, np.float32), 0.57)[0] == 5
    assert KR.pick_acceptable(w, 0.74, 2) and not KR.pick_acceptable(w, 0.74, 4) and not KR.pick_acceptable(w, 0.74, 3)
    assert KR.pick_acceptable(w, 0.75, 4) and KR.pick_acceptable(w, 0.75, 2)    # on the boundary itself both sides are within n 2^-53
    assert KR.pick_acceptable(np.zeros(10), 0.57, 5) and not KR.pick_acceptable(np.zeros(10), 0.57, 4)
    one = np.zeros(100, np.float32); one[63] = 2.5
    assert all(KR.pick64(one, u)[0] == 63 for u in (0.0, 0.3, 0.999999))


# ---- 4. scikit-learn's recorded answers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_lloyd64_is_scikit_learn_on_the_golden_inputs(gold, name):
    x, init = gold[f"{name}_x"], gold[f"{name}_init"]
    r = KR.lloyd64(x, init, check=True)
    assert np.array_equal(r["labels"], gold[f"{name}_labels"]) and r["n_iter"] == int(gold[f"{name}_n_iter"])
    assert np.abs(r["centres"] - gold[f"{name}_centres"]).max() <= 1e-12
    assert abs(r["inertia"] - float(gold[f"{name}_inertia"])) <= 1e-9 * r["inertia"]
    assert r["n_empty_max"] == 0 and r["ambiguous_max"] == 0.0               # fit for an exact comparison on the device


def test_pp_case_is_fit(gold):
    x, seed = gold["A_x"], int(gold["pp_seed"])
    for r in range(3):
        rows, margin = KR.pp64(x, 7, seed + r)
        assert np.array_equal(rows, gold["pp_rows"][r]) and margin > x.shape[0] * 2.0 ** -53
        ref = KR.lloyd64(x, x[rows], check=True)
        assert np.array_equal(ref["labels"], gold["pp_labels"][r]) and ref["n_iter"] == int(gold["pp_n_iter"][r])
        assert ref["n_empty_max"] == 0 and ref["ambiguous_max"] == 0.0
    best = np.sort(gold["pp_inertia"])
    assert best[1] - best[0] > 1e-4 * best[0] and int(np.argmin(gold["pp_inertia"])) != 0      # n_init has something to choose


def test_ambiguous_share_of_the_gpu_cases_is_below_the_cap(gold):
    """The cap of the GPU assign test, a condition on its inputs: at most 1 % of a case's points may be ambiguous."""
    xc, cc = KR.case_c()
    for name, x, c in (("A", gold["A_x"], gold["A_init"]), ("B", gold["B_x"], gold["B_init"]), ("C", xc, cc)):
        share = float(KR.ambiguous(KR.d64(x, c), KR.bound(x, c)).mean())
        assert share <= 0.01, (name, share)
    labels = KR.skewed_labels(6100, 1000)
    counts = np.bincount(labels, minlength=1000)
    assert counts[3] >= 0.9 * 6100 - 1 and (counts[500:] == 1).all() and (counts[:500] == 0).any()


def test_scores_equal_scikit_learn(gold):
    from embeddingnet_amd import clustering
    for name in gold["pair_names"]:
        t, p = gold[f"pair_{name}_true"], gold[f"pair_{name}_pred"]
        want = gold[f"pair_{name}_scores"]
        assert abs(KR.nmi64(t, p) - want[0]) <= 1e-12, name
        assert np.abs(np.asarray(KR.hc64(t, p)) - want[1:]).max() <= 1e-12, name
        assert abs(clustering.nmi(t, p) - want[0]) <= 1e-12, name
        assert abs(clustering.nmi(t.tolist(), p.tolist()) - want[0]) <= 1e-12, name
        assert np.abs(np.asarray(clustering.homogeneity_completeness(t, p)) - want[1:]).max() <= 1e-12, name
    assert float(gold["pair_both_one_cluster_scores"][0]) == 1.0 and clustering.nmi([0, 0, 0], ["a", "a", "a"]) == 1.0
    assert float(gold["pair_true_one_cluster_scores"][0]) == 0.0 and clustering.nmi([0, 0, 0, 0], [1, 2, 1, 2]) == 0.0
    assert clustering.nmi([(1, 2), (1, 2), "x", None], [0, 0, 1, 2]) == pytest.approx(KR.nmi64([0, 0, 1, 2], [0, 0, 1, 2]))
    assert clustering.purity([0, 0, 1, 1, 2], [5, 5, 5, 7, 7]) == pytest.approx(3 / 5)
    for method, f in (("min", min), ("max", max), ("geometric", lambda a, b: (a * b) ** 0.5)):
        t, p = gold["pair_random_unequal_counts_true"], gold["pair_random_unequal_counts_pred"]
        h = [KR._h(np.bincount(t)), KR._h(np.bincount(p))]
        assert clustering.nmi(t, p, average_method=method) == pytest.approx(KR._mi(KR._table(t, p)) / f(*h), rel=1e-12)
    with pytest.raises(ValueError):
        clustering.nmi([0, 1], [0, 1], average_method="harmonic")
    with pytest.raises(ValueError):
        clustering.nmi([0, 1], [0, 1, 2])


# ---- 5. the Python surface -----------------------------------------------------------------------------------------------------
def test_python_surface():
    import embedding_net
    from embeddingnet_amd import clustering, kmeans, ops
    from embeddingnet_amd.models import EmbeddingNet
    assert embedding_net.clustering is clustering and embedding_net.kmeans is kmeans
    for name in ("kmeans_workspace", "kmeans_assign", "kmeans_update", "kmeans_pp_update", "kmeans_pp_pick"):
        assert callable(getattr(ops, name)), name
    sig = inspect.signature(kmeans.KMeans.__init__).parameters
    assert [p for p in sig][1:] == ["n_clusters", "init", "n_init", "max_iter", "tol", "seed", "device"]
    assert (sig["init"].default, sig["n_init"].default, sig["max_iter"].default, sig["tol"].default, sig["seed"].default) == \
        ("k-means++", 1, 300, 0.0, 0)
    assert "not scikit-learn's tolerance" in kmeans.KMeans.__doc__
    sig = inspect.signature(clustering.clustering_metrics).parameters
    assert list(sig) == ["encodings", "labels", "n_clusters", "seed", "n_init", "max_iter", "device"]
    sig = inspect.signature(EmbeddingNet.calculate_clustering_metrics).parameters
    assert list(sig) == ["self", "data_loader", "n_clusters", "seed", "n_init", "batch_size"]
    for bad in (dict(n_clusters=0), dict(n_clusters=3, init="random"), dict(n_clusters=3, n_init=0), dict(n_clusters=3, max_iter=0)):
        with pytest.raises(ValueError):
            kmeans.KMeans(**bad)


def test_train_config_keys():
    import yaml
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train as T
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "simple2_nmi_synthetic.yml")))
    assert cfg["TRAIN"]["clustering_nmi"] is True and cfg["TRAIN"]["monitor"] == "val_nmi"
    assert cfg["GENERAL"]["project_name"] == "simple2_nmi_synthetic"
    assert T.monitor_config({"clustering_nmi": True, "monitor": "val_nmi"}, True) == ([], "val_nmi")
    assert T.monitor_config({"clustering_nmi": True}, True) == ([], "val_loss")
    assert T.clustering_nmi_config({}, True) is False and T.clustering_nmi_config({"clustering_nmi": True}, True) is True
    with pytest.raises(ValueError, match="needs TRAIN.clustering_nmi"):
        T.monitor_config({"monitor": "val_nmi"}, True)
    with pytest.raises(ValueError, match="needs TRAIN.clustering_nmi"):
        T.monitor_config({"monitor": "val_nmi", "retrieval_ks": [1], "retrieval_map": True}, True)
    with pytest.raises(ValueError, match="validation is off"):
        T.monitor_config({"clustering_nmi": True, "monitor": "val_nmi"}, False)
    with pytest.raises(ValueError, match="validation is off"):
        T.clustering_nmi_config({"clustering_nmi": True}, False)
    with pytest.raises(ValueError, match="true or false"):
        T.clustering_nmi_config({"clustering_nmi": "yes"}, True)
    with pytest.raises(ValueError, match="val_nmi"):
        T.monitor_config({"monitor": "val_banana"}, True)
