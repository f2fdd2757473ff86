"""GPU: the k-means kernels (csrc/kmeans.hip) element by element against the float64 restatement tests/kmeans_ref.py, the
estimator against scikit-learn's recorded answers (tests/golden/kmeans.npz), the clustering scores on top of it.

The bounds are kmeans_ref's (module docstring there): B = A(e) (|x|^2 + |c|^2) for every distance, U for every element of an
updated centre.  Shapes: A (777, 33, 7: scalar loader, ragged 64x64 tiles), B (1000, 64, 200: vector loader, four centre tiles in
four gallery splits merged by the 64-bit atomicMin), C (6100, 20, 1000: the 128x128 geometry, ragged on both sides) and the edge
cases of test_assign_edge_cases.

Measured on an MI355X, the largest error / bound of each check (every check asserts <= 1):
    assign d2 vs d64             A 0.109    B 0.162    C 0.119    edge cases <= 0.159
    assign inertia               A 0.0009   B 0.0075   C 0.0012   edge cases <= 0.019      ambiguous points: none in A, B, C (cap 1 %)
    update element vs update64   A 0.952    C 0.9993   C skewed 0.963   C blocks 0.818   A with an empty cluster 0.990
                                 (the bound is half an fp32 ulp at the top of a binade: a correctly rounded mean reaches it)
    update shift                 A 0.059    C 0.0032   C skewed 0.0001  C blocks 0.119   A with an empty cluster 0.025
    pp_update vs float64         A 0.069    B 0.077
    fit vs scikit-learn          centres A 0.958, B 0.9999; inertia A 0.0011, B 0.0019; labels and n_iter_ equal
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_ref as KR  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "kmeans.npz"))


@pytest.fixture(scope="module")
def cases(gold):
    """name -> (x, centres, d64, B): computed once, read by every test that needs them."""
    xc, cc = KR.case_c()
    out = {}
    for name, x, c in (("A", gold["A_x"], gold["A_init"]), ("B", gold["B_x"], gold["B_init"]), ("C", xc, cc)):
        out[name] = (x, c, KR.d64(x, c), KR.bound(x, c))
    return out


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint64 if t.dtype == torch.float64 else np.int32)


def _check_assign(name, x, c, d, b, dev, cap=0.01):
    """One assign pass against the float64 distances d and their bounds b; -> the device labels."""
    from embeddingnet_amd import ops
    n, k = d.shape
    prev = np.random.RandomState(3).randint(0, k, n).astype(np.int32)
    xt, ct = _t(x, dev), _t(c, dev)
    labels, d2, changed, inertia = ops.kmeans_assign(xt, ct, _t(prev, dev, torch.int32))
    again = ops.kmeans_assign(xt, ct, _t(prev, dev, torch.int32))
    for a, g in zip((labels, d2, changed, inertia), again):
        assert np.array_equal(_bits(a), _bits(g)), f"{name}: two calls differ"
    got, gd2 = labels.cpu().numpy(), d2.cpu().numpy().astype(np.float64)
    assert got.dtype == np.int32 and got.min() >= 0 and got.max() < k
    amb = KR.ambiguous(d, b)
    print(f"{name}: ambiguous {amb.mean():.5f}")
    assert amb.mean() <= cap, f"{name}: the case is not fit for the test ({amb.mean()} ambiguous)"
    ok = KR.labels_acceptable(d, b, got)
    assert ok.all(), f"{name}: {np.flatnonzero(~ok)[:5]} took labels {got[~ok][:5]}"
    want, _ = KR.assign64(x, c, d)
    assert np.array_equal(got[~amb], want[~amb]), f"{name}: an unambiguous point is off the float64 argmin"
    rows = np.arange(n)
    dsel, bsel = d[rows, got], b[rows, got]
    fin = np.isfinite(dsel)
    assert np.array_equal(np.isinf(gd2), ~fin)
    ratio = float((np.abs(gd2[fin] - dsel[fin]) / bsel[fin]).max()) if fin.any() else 0.0
    print(f"{name}: d2 error / bound {ratio:.4f}")
    assert ratio <= 1.0
    assert int(changed.item()) == int((got != prev).sum())
    assert int(ops.kmeans_assign(xt, ct)[2].item()) == n                      # without previous labels every label is new
    if fin.all():
        total = float(dsel.sum())
        lim = float(bsel.sum()) + n * 2.0 ** -53 * total
        print(f"{name}: inertia error / bound {abs(float(inertia.item()) - total) / lim:.4f}")
        assert abs(float(inertia.item()) - total) <= lim
    else:
        assert np.isinf(float(inertia.item()))
    return got


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_assign(cases, dev, name):
    x, c, d, b = cases[name]
    _check_assign(name, x, c, d, b, dev)


def test_assign_edge_cases(dev):
    rs = np.random.RandomState(17)

    def run(name, x, c, cap=0.01):
        x, c = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(c, np.float32)
        return _check_assign(name, x, c, KR.d64(x, c), KR.bound(x, c), dev, cap)

    x = rs.randn(70, 5).astype(np.float32)
    assert (run("k=1", x, x[:1]) == 0).all()
    x = rs.randn(64, 12).astype(np.float32)
    assert np.array_equal(run("k=n=64", x, x), np.arange(64))                # every point is its own centre, d2 = 0 < the rest
    # two bitwise identical centre rows: the distances to them are the same bits, and the smaller index wins exactly
    x, _ = KR.blobs(300, 16, 6, 0.5, 4)
    c = x[[0, 1, 2, 3, 4, 5, 2]].copy()                                      # row 6 repeats row 2
    got = run("duplicate centre", x, c, cap=1.0)                             # (every point near rows 2 / 6 is ambiguous by design)
    assert (got != 6).all() and (got == 2).any()
    # duplicate points take the same label and the same distance bits; a zero-norm point is served like any other
    x = rs.randn(130, 9).astype(np.float32)
    x[100:130] = x[10:40]
    x[7] = 0.0
    c = x[rs.choice(100, 11, replace=False)]
    from embeddingnet_amd import ops
    got = run("duplicate points", x, c)
    d2 = ops.kmeans_assign(_t(x, dev), _t(c, dev))[1]
    assert np.array_equal(got[100:130], got[10:40]) and np.array_equal(_bits(d2)[100:130], _bits(d2)[10:40])
    # a centre row of NaN is never chosen; with nothing but NaN rows every point takes label 0 at d2 = +inf
    c2 = c.copy()
    c2[0] = np.nan
    assert (run("NaN centre", x, c2) != 0).all()
    lab, d2, _, inertia = ops.kmeans_assign(_t(x, dev), _t(np.full((3, 9), np.nan, np.float32), dev))
    assert (lab == 0).all().item() and torch.isinf(d2).all().item() and np.isinf(float(inertia.item()))
    x = np.sort(rs.randn(200, 1).astype(np.float32), axis=0)
    run("e=1", x, x[[5, 60, 120, 199]])


def _check_update(name, x, labels, centres, dev, labels_t=None):
    from embeddingnet_amd import ops
    xt, ct = _t(x, dev), _t(centres, dev)
    lt = _t(labels, dev, torch.int32) if labels_t is None else labels_t
    new, counts, shift, n_empty = ops.kmeans_update(xt, lt, ct)
    again = ops.kmeans_update(xt, lt.clone(), ct)
    for a, g in zip((new, counts, shift, n_empty), again):
        assert np.array_equal(_bits(a), _bits(g)), f"{name}: two calls differ"
    want, wcounts, u = KR.update64(x, labels, centres)
    assert np.array_equal(counts.cpu().numpy(), wcounts.astype(np.int32)), f"{name}: counts"
    got = new.cpu().numpy()
    empty = wcounts == 0
    assert int(n_empty.item()) == int(empty.sum())
    assert np.array_equal(got[empty].view(np.uint32), np.asarray(centres, np.float32)[empty].view(np.uint32)), f"{name}: an empty cluster moved"
    live = ~empty
    ratio = float((np.abs(got[live].astype(np.float64) - want[live]) / u[live]).max())
    print(f"{name}: centre error / bound {ratio:.4f}")
    assert ratio <= 1.0
    s64, sb = KR.shift64(want, centres, wcounts, u)
    print(f"{name}: shift error / bound {abs(float(shift.item()) - s64) / sb:.4f}")
    assert abs(float(shift.item()) - s64) <= sb
    return new


def test_update(cases, dev):
    from embeddingnet_amd import ops
    for name in ("A", "C"):
        x, c, d, _ = cases[name]
        xt, ct = _t(x, dev), _t(c, dev)
        labels_t = ops.kmeans_assign(xt, ct)[0]
        labels = labels_t.cpu().numpy()
        from_device = _check_update(name, x, labels, c, dev, labels_t=labels_t)
        from_host = _check_update(name + " (labels from the host)", x, labels, c, dev)
        assert np.array_equal(_bits(from_device), _bits(from_host)), f"{name}: the route of the labels shows in the centres"
    x, c, _, _ = cases["C"]
    _check_update("C skewed", x, KR.skewed_labels(6100, 1000), c, dev)       # 90 % in one cluster (11 chunks), 500 singletons, empties
    _check_update("C blocks", x, (np.arange(6100) % 4).astype(np.int32) * 7, c, dev)   # four interleaved clusters of 1525: the LDS sort, 3 chunks
    x, c, _, _ = cases["A"]
    labels = (np.arange(777) % 6).astype(np.int32)                           # cluster 6 stays empty
    _check_update("A with an empty cluster", x, labels, c, dev)


def test_update_in_place_and_out_of_range_labels(cases, dev):
    """centres_out may be centres; a label outside [0, k) belongs to no cluster."""
    from embeddingnet_amd import _lib, ops
    from embeddingnet_amd._lib import ptr, stream
    x, c, _, _ = cases["A"]
    labels = (np.arange(777) % 7).astype(np.int32)
    xt, lt, ct = _t(x, dev), _t(labels, dev, torch.int32), _t(c, dev)
    want = ops.kmeans_update(xt, lt, ct)[0]
    ws = ops.kmeans_workspace(777, 7, 33, xt)
    counts, shift, n_empty = torch.empty(7, dtype=torch.int32, device=dev), torch.empty((), dtype=torch.float64, device=dev), \
        torch.empty((), dtype=torch.int32, device=dev)
    inplace = ct.clone()
    _lib.check(_lib.lib().embnet_kmeans_update(ptr(xt), ptr(lt), 777, ptr(inplace), 7, 33, ptr(inplace), ptr(counts), ptr(shift),
                                               ptr(n_empty), ptr(ws), ws.numel() * 8, stream()))
    assert np.array_equal(_bits(inplace), _bits(want))
    bad = labels.copy()
    bad[::10] = np.where(np.arange(0, 777, 10) % 20 == 0, -1, 7)
    got, counts, _, _ = ops.kmeans_update(xt, _t(bad, dev, torch.int32), ct)
    keep = (bad >= 0) & (bad < 7)
    ref, wcounts, u = KR.update64(x[keep], bad[keep], c)
    assert np.array_equal(counts.cpu().numpy(), wcounts) and (np.abs(got.cpu().numpy() - ref) <= u).all()


def test_pp_update(cases, dev):
    from embeddingnet_amd import ops
    for name in ("A", "B"):
        x = cases[name][0]
        x64 = x.astype(np.float64)
        n, e = x.shape
        xt = _t(x, dev)
        norms = (x64 * x64).sum(1)
        mind2, want, worst = None, None, 0.0
        for c in (5, n - 1, 300):
            mind2 = ops.kmeans_pp_update(xt, torch.tensor([c], dtype=torch.int32, device=dev), mind2)
            d = ((x64 - x64[c]) ** 2).sum(1)
            # the minimum of two values each within its bound is within the larger of the two bounds
            bnd = KR.A(e) * (norms + norms[c]) if want is None else np.maximum(bnd, KR.A(e) * (norms + norms[c]))
            want = d if want is None else np.minimum(want, d)
            got = mind2.cpu().numpy().astype(np.float64)
            assert got[c] == 0.0
            worst = max(worst, float((np.abs(got - want) / bnd).max()))
        print(f"{name}: pp_update error / bound {worst:.4f}")
        assert worst <= 1.0


def test_pp_pick(dev):
    from embeddingnet_amd import ops
    rs = np.random.RandomState(23)
    big = rs.rand(5000).astype(np.float32) * (rs.rand(5000) < 0.6)           # 40 % zeros; five rows per thread of the scan
    one = np.zeros(3000, np.float32)
    one[1777] = 0.37
    vectors = {"zeros and weights": np.array([0, 0, 3, 0, 1, 0, 0, 2.5, 0], np.float32), "one non-zero": one,
               "all zero": np.zeros(777, np.float32), "random": big, "single row": np.array([2.0], np.float32),
               "non-finite weigh nothing": np.array([np.nan, 1.0, np.inf, -3.0, 2.0], np.float32)}
    for name, w in vectors.items():
        wt = _t(w, dev)
        for seed in (0, 8, 12345678901):
            for draw in range(1, 9):
                index, u = ops.kmeans_pp_pick(wt, seed, draw)
                uu, i = float(u.item()), int(index.item())
                assert uu == KR.draw_u(seed, draw), (name, seed, draw)          # the same 53 bits
                assert KR.pick_acceptable(w, uu, i), (name, seed, draw, uu, i, KR.pick64(w, uu))
                if name != "all zero":
                    assert w[i] > 0 and np.isfinite(w[i])
        index, u = ops.kmeans_pp_pick(wt, 8, 0)
        assert int(index.item()) == KR.first_row(8, w.shape[0]) and float(u.item()) == 0.0
        again = ops.kmeans_pp_pick(wt, 8, 3)
        assert int(again[0].item()) == int(ops.kmeans_pp_pick(wt, 8, 3)[0].item())


def test_seed_rows_follow_the_seed(gold, dev):
    from embeddingnet_amd.kmeans import KMeans
    x = _t(gold["A_x"], dev)
    km = KMeans(7)
    a, b, c = km.seed_rows(x, 8).cpu().numpy(), km.seed_rows(x, 8).cpu().numpy(), km.seed_rows(x, 9).cpu().numpy()
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, gold["pp_rows"][0]) and np.array_equal(c, gold["pp_rows"][1])


@pytest.mark.parametrize("name", ["A", "B"])
def test_fit_from_given_init_is_scikit_learn(gold, dev, name):
    from embeddingnet_amd.kmeans import KMeans
    x, init = gold[f"{name}_x"], gold[f"{name}_init"]
    k = init.shape[0]
    km = KMeans(k, init=init, n_init=5, device=dev).fit(x)
    assert np.array_equal(km.labels_, gold[f"{name}_labels"]) and km.labels_.dtype == np.int32
    assert km.n_iter_ == int(gold[f"{name}_n_iter"]) and km.n_empty_ == 0
    # the centres are the means of the golden labels: the last update's bound.  (The device's previous centres, from which the
    # bound's labels came, play no part: the labels are equal.)
    _, _, u = KR.update64(x, gold[f"{name}_labels"], init)
    ratio = float((np.abs(km.cluster_centers_.astype(np.float64) - gold[f"{name}_centres"]) / u).max())
    print(f"{name}: fitted centres error / bound {ratio:.4f}")
    assert km.cluster_centers_.dtype == np.float32 and ratio <= 1.0
    b = KR.bound(x, gold[f"{name}_centres"])[np.arange(x.shape[0]), km.labels_]
    lim = float(b.sum()) + x.shape[0] * 2.0 ** -53 * float(gold[f"{name}_inertia"])
    print(f"{name}: fitted inertia error / bound {abs(km.inertia_ - float(gold[f'{name}_inertia'])) / lim:.4f}")
    assert abs(km.inertia_ - float(gold[f"{name}_inertia"])) <= lim
    assert np.array_equal(km.predict(x), km.labels_)
    assert np.array_equal(KMeans(k, init=init, device=dev).fit_predict(torch.as_tensor(x)), km.labels_)


def test_fit_kmeans_pp_is_the_restatement(gold, dev):
    from embeddingnet_amd.kmeans import KMeans
    x, seed = gold["A_x"], int(gold["pp_seed"])
    for r in range(3):
        km = KMeans(7, seed=seed + r, device=dev).fit(x)
        assert np.array_equal(km.init_rows_, gold["pp_rows"][r]), r
        assert np.array_equal(km.labels_, gold["pp_labels"][r]) and km.n_iter_ == int(gold["pp_n_iter"][r]), r
        # unit-norm points and centres inside the unit ball: B <= 2 A(e) per point
        assert abs(km.inertia_ - float(gold["pp_inertia"][r])) <= 2 * KR.A(33) * 777 + 777 * 2.0 ** -53 * km.inertia_
        assert np.array_equal(km.predict(x), km.labels_)
    best = int(np.argmin(gold["pp_inertia"]))
    km = KMeans(7, n_init=3, seed=seed, device=dev).fit(x)
    assert np.array_equal(km.init_rows_, gold["pp_rows"][best]) and np.array_equal(km.labels_, gold["pp_labels"][best])
    assert km.n_iter_ == int(gold["pp_n_iter"][best])
    again = KMeans(7, n_init=3, seed=seed, device=dev).fit(x)
    assert np.array_equal(again.cluster_centers_.view(np.uint32), km.cluster_centers_.view(np.uint32)) and again.inertia_ == km.inertia_
    few = KMeans(7, seed=seed, max_iter=2, device=dev).fit(x)                # stopped early: labels still belong to the centres
    assert few.n_iter_ == 2 and np.array_equal(few.predict(x), few.labels_)
    loose = KMeans(7, seed=seed, tol=1e9, device=dev).fit(x)                 # any shift is below this tolerance: one pass
    assert loose.n_iter_ == 1 and np.array_equal(loose.predict(x), loose.labels_)


def test_clustering_metrics(gold, dev):
    from embeddingnet_amd import clustering
    from embeddingnet_amd.kmeans import KMeans
    x = gold["A_x"]
    truth = [f"class {i % 7}" for i in range(x.shape[0])]                    # kmeans_ref.blobs: point i belongs to blob i mod k
    seed = int(gold["pp_seed"])
    m = clustering.clustering_metrics(x, truth, seed=seed, n_init=3, device=dev)
    km = KMeans(7, seed=seed, n_init=3, device=dev).fit(x)
    assert abs(m["nmi"] - KR.nmi64(truth, km.labels_)) <= 1e-12
    h, c = KR.hc64(truth, km.labels_)
    assert abs(m["homogeneity"] - h) <= 1e-12 and abs(m["completeness"] - c) <= 1e-12
    assert m["n_clusters"] == 7 and m["n_iter"] == km.n_iter_ and m["n_empty"] == 0 and m["inertia"] == km.inertia_
    assert 0.0 < m["nmi"] <= 1.0 and 1.0 / 7 < m["purity"] <= 1.0
    m3 = clustering.clustering_metrics({"encodings": x, "labels": truth}, n_clusters=3, seed=1, device=dev)
    assert m3["n_clusters"] == 3 and 0.0 <= m3["nmi"] <= 1.0
    for name in gold["pair_names"]:
        t, p = gold[f"pair_{name}_true"], gold[f"pair_{name}_pred"]
        assert abs(clustering.nmi(t, p) - gold[f"pair_{name}_scores"][0]) <= 1e-12, name


def test_refusals(gold, dev):
    from embeddingnet_amd import ops
    from embeddingnet_amd._lib import EmbnetError
    from embeddingnet_amd.kmeans import KMeans
    x = _t(gold["A_x"], dev)
    labels = torch.zeros(777, dtype=torch.int32, device=dev)
    with pytest.raises(EmbnetError, match="k=778 exceeds n=777"):
        ops.kmeans_assign(x, torch.zeros(778, 33, device=dev))
    with pytest.raises(EmbnetError, match="k=778 exceeds n=777"):
        ops.kmeans_update(x, labels, torch.zeros(778, 33, device=dev))
    with pytest.raises(EmbnetError, match="widths differ"):
        ops.kmeans_assign(x, torch.zeros(7, 32, device=dev))
    with pytest.raises(EmbnetError, match="widths differ"):
        ops.kmeans_update(x, labels, torch.zeros(7, 34, device=dev))
    with pytest.raises(EmbnetError, match="contiguous"):
        ops.kmeans_assign(torch.zeros(33, 777, device=dev).t(), x[:7].contiguous())
    with pytest.raises(EmbnetError, match="contiguous"):
        ops.kmeans_assign(x, torch.zeros(7, 66, device=dev)[:, ::2])
    with pytest.raises(EmbnetError, match="float32"):
        ops.kmeans_assign(x.double(), x[:7].contiguous())
    with pytest.raises(EmbnetError, match="float32"):
        ops.kmeans_update(x, labels, x[:7].half())
    with pytest.raises(EmbnetError, match="int32"):
        ops.kmeans_update(x, labels.long(), x[:7].contiguous())
    with pytest.raises(EmbnetError, match="float32"):
        ops.kmeans_pp_update(x.double(), torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="exceeds the number of points"):
        KMeans(800, device=dev).fit(gold["A_x"])
    with pytest.raises(ValueError, match="init must be"):
        KMeans(7, init=np.zeros((7, 32), np.float32), device=dev).fit(gold["A_x"])
