"""GPU: the streaming k-nearest-neighbour search (csrc/knn_search.hip) through the C ABI, ops.knn_search, knn.KNNClassifier,
retrieval.nearest_neighbors and EmbeddingNet.fit_knn, against the float64 restatement tests/knn_search_ref.py.  Where the fp32 d2
is exact (integer embeddings) every output is compared bit for bit; on continuous inputs the answer has to be one that the
project's distance error bound allows (knn_search_ref.check)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_search_ref as KR  # noqa: E402

GUARD = 64                                                  # sentinel words on both sides of each output
SELECT = {0: "all", 1: "same", 2: "other"}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(a, dev, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.array(a, order="C"), dtype=dtype, device=dev)   # a copy: shared inputs are read-only


def _search(q, x, k, dev, ql=None, xl=None, select=0, qt=None, xt=None):
    """ops.knn_search (squared) as NumPy (idx, d2, found); x None: leave-one-out."""
    from embeddingnet_amd import ops
    qt = _t(q, dev) if qt is None else qt
    xt = (None if x is None else _t(x, dev)) if xt is None else xt
    d2, idx, found = ops.knn_search(qt, xt, k, _t(ql, dev, torch.int32), None if x is None else _t(xl, dev, torch.int32),
                                    select=SELECT[select])
    assert d2.dtype == torch.float32 and idx.dtype == found.dtype == torch.int32
    assert d2.shape == idx.shape == (len(q), k) and found.shape == (len(q),)
    return idx.cpu().numpy(), d2.cpu().numpy(), found.cpu().numpy()


def _raw(qt, qlt, xt, xlt, self_exclude, select, k, ws=None, ws_bytes=None):
    """The C entry on guarded outputs -> (rc, idx, d2, found, guards untouched)."""
    from embeddingnet_amd import _lib
    from embeddingnet_amd._lib import ptr, stream
    lib = _lib.lib()
    nq, e = qt.shape
    n = xt.shape[0]
    kk = max(k, 1)
    if ws is None:
        ws = torch.empty(max(lib.embnet_knn_search_workspace_bytes(nq, n, k) // 8, 2), dtype=torch.float64, device=qt.device)
    bi = torch.full((nq * kk + 2 * GUARD,), -7, dtype=torch.int32, device=qt.device)
    bd = torch.full((nq * kk + 2 * GUARD,), -7.0, dtype=torch.float32, device=qt.device)
    bf = torch.full((nq + 2 * GUARD,), -7, dtype=torch.int32, device=qt.device)
    rc = lib.embnet_knn_search(ptr(qt), ptr(qlt), nq, ptr(xt), ptr(xlt), n, e, self_exclude, select, k,
                               bi[GUARD:].data_ptr(), bd[GUARD:].data_ptr(), bf[GUARD:].data_ptr(), ptr(ws),
                               ws.numel() * 8 if ws_bytes is None else ws_bytes, stream())
    torch.cuda.synchronize()
    i, d, f = bi.cpu().numpy(), bd.cpu().numpy(), bf.cpu().numpy()
    clean = all(np.all(a[:GUARD] == -7) and np.all(a[GUARD + m:] == -7) for a, m in ((i, nq * kk), (d, nq * kk), (f, nq)))
    return rc, i[GUARD:GUARD + nq * kk].reshape(nq, kk), d[GUARD:GUARD + nq * kk].reshape(nq, kk), f[GUARD:GUARD + nq], clean


def _matrix_indices(q, x, k, dev):
    """What the matrix path selects: ops.topk_smallest on ops.cross_distances (k <= 64)."""
    from embeddingnet_amd import ops
    return ops.topk_smallest(ops.cross_distances(_t(q, dev), _t(x, dev), squared=True), k)[1].cpu().numpy()


def _same_bits(got, want):
    idx, d2, found = got
    widx, wd2, wfound = want
    assert np.array_equal(found, wfound)
    assert np.array_equal(idx, widx)
    assert np.array_equal(d2.view(np.uint32), wd2.astype(np.float32).view(np.uint32))


# ---- 1. exact cases: integer embeddings, every d2 an exact fp32 integer ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tie_case():
    """(70, 389, 3): tiny e gives masses of ties; nq and n off the tile; 7 unbalanced classes, class 0 with ONE gallery member."""
    q, x = KR.integer_rows(70, 3, 1), KR.integer_rows(389, 3, 2)
    ql, xl = KR.unbalanced_labels(70, 3), KR.unbalanced_labels(389, 4)
    for a in (q, x, ql, xl):
        a.setflags(write=False)
    return q, x, ql, xl


@pytest.mark.parametrize("k", [1, 5, 64, 128])
def test_ties_off_the_tile_are_exact(dev, k):
    q, x, ql, xl = _tie_case()
    got = _search(q, x, k, dev)
    _same_bits(got, KR.knn_ref(q, x, k))
    if k <= 64:                                             # the matrix path orders the same exact distances the same way
        assert np.array_equal(got[0], _matrix_indices(q, x, k, dev))


@pytest.mark.parametrize("k", [5, 128])
@pytest.mark.parametrize("select", [1, 2])
def test_select_on_unbalanced_classes_is_exact(dev, select, k):
    q, x, ql, xl = _tie_case()
    got = _search(q, x, k, dev, ql, xl, select)
    _same_bits(got, KR.knn_ref(q, x, k, ql, xl, False, select))
    live = got[0] >= 0
    agree = xl[got[0][live]] == np.broadcast_to(ql[:, None], got[0].shape)[live]
    assert live.any() and (np.all(agree) if select == 1 else not np.any(agree))


@pytest.mark.parametrize("k", [1, 5, 64, 128])
@pytest.mark.parametrize("select", [0, 1, 2])
def test_leave_one_out_is_exact(dev, select, k):
    _, x, _, xl = _tie_case()
    got = _search(x, None, k, dev, xl if select else None, None, select)
    _same_bits(got, KR.knn_ref(x, x, k, xl, xl, True, select))
    assert not np.any(got[0] == np.arange(389)[:, None])
    if select == 1:                                         # the class of one: nothing eligible, a fully padded row
        single = int(np.flatnonzero(xl == 0)[0])
        assert got[2][single] == 0 and np.all(got[0][single] == -1) and np.all(np.isposinf(got[1][single]))
    if select == 0 and k <= 64:
        from embeddingnet_amd import ops
        d = ops.cross_distances(_t(x, dev), _t(x, dev), squared=True)
        d.fill_diagonal_(float("inf"))
        assert np.array_equal(got[0], ops.topk_smallest(d, k)[1].cpu().numpy())


def test_k_above_n_pads(dev):
    q, x = KR.integer_rows(9, 8, 5), KR.integer_rows(5, 8, 6)
    got = _search(q, x, 8, dev)
    _same_bits(got, KR.knn_ref(q, x, 8))
    assert np.all(got[2] == 5) and np.all(got[0][:, 5:] == -1) and np.all(np.isposinf(got[1][:, 5:]))
    assert np.array_equal(got[0][:, :5], _matrix_indices(q, x, 5, dev))
    got = _search(x, None, 8, dev)
    _same_bits(got, KR.knn_ref(x, x, 8, self_exclude=True))
    assert np.all(got[2] == 4)


@pytest.mark.parametrize("k", [3, 128])
def test_many_splits_meet_in_the_merge_kernel(dev, k):
    """nq = 7 against n = 2 000: one query tile, 32 gallery splits of one tile each."""
    q, x = KR.integer_rows(7, 16, 7), KR.integer_rows(2000, 16, 8)
    got = _search(q, x, k, dev)
    _same_bits(got, KR.knn_ref(q, x, k))
    if k <= 64:
        assert np.array_equal(got[0], _matrix_indices(q, x, k, dev))


def test_many_tiles_in_one_walk(dev):
    """600 queries against 3 000: 10 query tiles, so a workgroup walks several gallery tiles with its thresholds standing."""
    q, x = KR.integer_rows(600, 16, 9), KR.integer_rows(3000, 16, 10)
    for k in (10, 100):
        _same_bits(_search(q, x, k, dev), KR.knn_ref(q, x, k))


def test_gallery_sorted_by_descending_distance(dev):
    """One query direction, the gallery from the farthest to the nearest: every tile displaces the whole list, every row is
    compacted behind every tile."""
    n, k = 389, 8
    q = np.zeros((70, 4), np.float32); q[:, 0] = 1 + np.arange(70) % 3
    x = np.zeros((n, 4), np.float32); x[:, 0] = -(n - np.arange(n))
    want = KR.knn_ref(q, x, k)
    assert np.array_equal(want[0], np.broadcast_to(np.arange(n - 1, n - 1 - k, -1), (70, k)))
    got = _search(q, x, k, dev)
    _same_bits(got, want)
    assert np.array_equal(got[0], _matrix_indices(q, x, k, dev))
    qq = np.repeat(q, 4, axis=0)[:250]                      # four query tiles: one split walks all seven gallery tiles
    _same_bits(_search(qq, x, k, dev), KR.knn_ref(qq, x, k))


def test_unaligned_view_takes_the_scalar_loader(dev):
    q, x = KR.integer_rows(70, 13, 11), KR.integer_rows(389, 13, 12)
    bq, bx = torch.zeros(70 * 13 + 1, device=dev), torch.zeros(389 * 13 + 1, device=dev)
    qt, xt = bq[1:].view(70, 13), bx[1:].view(389, 13)
    qt.copy_(_t(q, dev)); xt.copy_(_t(x, dev))
    assert qt.data_ptr() % 16 == 4 and qt.is_contiguous()
    for k in (5, 128):
        got = _search(q, x, k, dev, qt=qt, xt=xt)
        _same_bits(got, KR.knn_ref(q, x, k))
        if k <= 64:
            assert np.array_equal(got[0], _matrix_indices(q, x, k, dev))
    q, x = KR.integer_rows(70, 64, 13), KR.integer_rows(389, 64, 14)     # e % 4 == 0, 4 bytes off a 16-byte boundary
    bq, bx = torch.zeros(70 * 64 + 1, device=dev), torch.zeros(389 * 64 + 1, device=dev)
    qt, xt = bq[1:].view(70, 64), bx[1:].view(389, 64)
    qt.copy_(_t(q, dev)); xt.copy_(_t(x, dev))
    _same_bits(_search(q, x, 5, dev, qt=qt, xt=xt), KR.knn_ref(q, x, 5))


# ---- 2. float cases: through the interval checker ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float_case(nq, n, e):
    q, x = KR.unit_rows(nq, e, 100 + e), KR.unit_rows(n, e, 200 + e)
    ql, xl = KR.unbalanced_labels(nq, 300 + e), KR.unbalanced_labels(n, 400 + e)
    for a in (q, x, ql, xl):
        a.setflags(write=False)
    return q, x, ql, xl


@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("select", [0, 1, 2])
@pytest.mark.parametrize("shape", [(300, 1000, 128), (64, 700, 517)])
def test_unit_rows_within_the_distance_bound(dev, shape, select, k):
    q, x, ql, xl = _float_case(*shape)
    idx, d2, found = _search(q, x, k, dev, ql, xl, select)
    assert KR.check(q, x, k, idx, d2, found, ql, xl, False, select) == []


def test_a_nan_row_comes_back_last(dev):
    """A gallery row of NaN is a real entry: d2 = +inf with a valid index, behind every finite one."""
    q, x = KR.unit_rows(64, 128, 21), KR.unit_rows(100, 128, 22).copy()
    x[37] = np.nan
    idx, d2, found = _search(q, x, 128, dev)
    assert np.all(found == 100) and np.all(idx[:, 99] == 37) and np.all(np.isposinf(d2[:, 99])) and np.all(np.isfinite(d2[:, :99]))
    assert KR.check(q, x, 128, idx, d2, found) == []
    x2 = KR.unit_rows(1000, 128, 23).copy()
    x2[[5, 900]] = np.nan                                   # far from the front: the finite answer is untouched
    idx, d2, found = _search(q, x2, 10, dev)
    assert KR.check(q, x2, 10, idx, d2, found) == [] and np.all(np.isfinite(d2))


# ---- 3. the contract -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(dev):
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.embnet_last_error().decode()
    q, x, ql, xl = _tie_case()
    qt, xt, qlt, xlt = _t(q, dev), _t(x, dev), _t(ql, dev, torch.int32), _t(xl, dev, torch.int32)
    big = torch.empty(lib.embnet_knn_search_workspace_bytes(70, 389, 128) // 8, dtype=torch.float64, device=dev)

    def refused(rc_want, word, *a, **kw):
        rc, idx, d2, found, clean = _raw(*a, **kw)
        assert rc == rc_want and word in err() and clean
        assert np.all(idx == -7) and np.all(d2 == -7.0) and np.all(found == -7)

    refused(-1, "k=0", qt, None, xt, None, 0, 0, 0, ws=big)
    refused(-1, "k=129", qt, None, xt, None, 0, 0, 129, ws=big)
    refused(-1, "needs q_labels", qt, None, xt, None, 0, 1, 5)
    refused(-1, "needs q_labels", qt, qlt, xt, None, 0, 2, 5)
    refused(-1, "select=3", qt, qlt, xt, xlt, 0, 3, 5)
    refused(-1, "self_exclude", qt, None, xt, None, 1, 0, 5)
    need = lib.embnet_knn_search_workspace_bytes(70, 389, 5)
    refused(-3, "workspace", qt, None, xt, None, 0, 0, 5, ws=big, ws_bytes=need - 16)
    rc, idx, d2, found, clean = _raw(qt, None, xt, None, 0, 0, 5, ws=big, ws_bytes=need)
    assert rc == 0 and clean
    _same_bits((idx, d2, found), KR.knn_ref(q, x, 5))
    assert lib.embnet_knn_search_workspace_bytes(70, 389, 0) == 0 and lib.embnet_knn_search_workspace_bytes(70, 389, 129) == 0
    assert lib.embnet_knn_search_workspace_bytes(0, 389, 5) == 0


def test_workspace_holds_no_matrix():
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    assert 0 < lib.embnet_knn_search_workspace_bytes(1 << 20, 1 << 20, 10) < 1 << 30
    assert 0 < lib.embnet_knn_search_workspace_bytes(50000, 262144, 128) < 1 << 30


def test_streams_and_graph_replay_give_the_same_bits(dev):
    from embeddingnet_amd import ops
    q, x, ql, xl = _float_case(300, 1000, 128)
    qt, xt, qlt, xlt = _t(q, dev), _t(x, dev), _t(ql, dev, torch.int32), _t(xl, dev, torch.int32)
    run = lambda: ops.knn_search(qt, xt, 20, qlt, xlt, select="other")
    first = run()
    outs = []
    for _ in range(2):                                      # two runs on two streams of their own
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            outs.append(run())
        s.synchronize()
    for o in outs:
        for a, b in zip(first, o):
            assert torch.equal(a, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run()
    for seed in (31, 32):                                   # replayed on changed inputs: thresholds and counters start afresh
        qt.copy_(_t(KR.unit_rows(300, 128, seed), dev)); xt.copy_(_t(KR.unit_rows(1000, 128, seed + 10), dev))
        for t in cap:
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in cap]
        for a, b in zip(got, run()):
            assert torch.equal(a, b)
        assert not torch.equal(got[1], first[1])


# ---- 4. the Python surface -----------------------------------------------------------------------------------------------------------
def test_classifier_stream_equals_matrix(dev):
    from embeddingnet_amd.knn import KNNClassifier
    x, q = KR.integer_rows(389, 16, 41), KR.integer_rows(70, 16, 42)
    names = [f"class-{c}" for c in KR.unbalanced_labels(389, 43)]
    for k in (1, 5, 64):
        a = KNNClassifier(n_neighbors=k, device=dev).fit(x, names)
        b = KNNClassifier(n_neighbors=k, device=dev, algorithm="stream").fit(x, names)
        assert a.algorithm == "matrix" and np.array_equal(a.predict(q), b.predict(q))
        (da, ia), (db, ib) = a.kneighbors(q), b.kneighbors(q)
        assert ia.dtype == ib.dtype == np.int64 and np.array_equal(ia, ib)
        assert da.dtype == db.dtype and np.array_equal(da.view(np.uint32), db.view(np.uint32))
        assert np.array_equal(b.kneighbors(q, return_distance=False), ia)
    d, i = b.kneighbors(q, n_neighbors=100)                 # beyond the matrix path's 64
    want = KR.knn_ref(q, x, 100)
    assert np.array_equal(i, want[0]) and np.array_equal(d, np.sqrt(want[1].astype(np.float32)))
    with pytest.raises(Exception):
        b.kneighbors(q, n_neighbors=390)                    # more neighbours than fitted samples
    with pytest.raises(ValueError):
        KNNClassifier(algorithm="kd_tree")


def test_nearest_neighbors_with_string_labels(dev):
    from embeddingnet_amd import ops
    from embedding_net.retrieval import nearest_neighbors
    x = KR.unit_rows(300, 32, 51)
    lab = KR.unbalanced_labels(300, 52)
    names = [f"n{c}" for c in lab]
    out = nearest_neighbors(x, 10, labels=names, select="other", device=dev)
    assert set(out) == {"distances", "indices", "found"} and out["indices"].shape == (300, 10) and np.all(out["found"] == 10)
    assert not np.any(lab[out["indices"]] == lab[:, None])
    d2, idx, found = ops.knn_search(_t(x, dev), None, 10, _t(lab, dev, torch.int32), select="other")
    assert np.array_equal(out["indices"], idx.cpu().numpy()) and np.array_equal(out["found"], found.cpu().numpy())
    assert np.array_equal(out["distances"], torch.sqrt(d2).cpu().numpy())
    pos = nearest_neighbors({"encodings": x, "labels": names}, 5, select="same", device=dev)
    single = int(np.flatnonzero(lab == 0)[0])
    assert pos["found"][single] == 0 and np.all(lab[pos["indices"][pos["indices"] >= 0]] == np.broadcast_to(lab[:, None], (300, 5))[pos["indices"] >= 0])
    plain = nearest_neighbors(x[:40], 3, gallery=x, squared=True, device=dev)
    assert np.array_equal(plain["indices"][:, 0], np.arange(40)) and KR.check(x[:40], x, 3, plain["indices"], plain["distances"], plain["found"]) == []
    with pytest.raises(ValueError):
        nearest_neighbors(x, 10, select="other", device=dev)
    with pytest.raises(ValueError):
        nearest_neighbors(x, 129, device=dev)


def test_fit_knn_passes_the_algorithm_through(dev, tmp_path):
    import pickle
    from embeddingnet_amd import models
    x, q = KR.integer_rows(120, 8, 61), KR.integer_rows(30, 8, 62)
    params = {s: {} for s in models.PARAM_SECTIONS}
    params["general"] = {"work_dir": str(tmp_path), "project_name": "p"}
    net = models.EmbeddingNet(params)
    net.save_encodings({"encodings": x, "labels": [f"c{c}" for c in KR.unbalanced_labels(120, 63)]}, save_folder=str(tmp_path))
    with open(tmp_path / "encodings.pkl", "rb") as f:
        data = pickle.load(f)
    stream = net.fit_knn(knn_k=3, encoded_training_data=dict(data), algorithm="stream")
    assert stream.algorithm == "stream" and net.encoded_training_data["knn_classifier"] is stream
    default = net.fit_knn(knn_k=3, encoded_training_data=dict(data))
    assert default.algorithm == "matrix" and np.array_equal(default.predict(q), stream.predict(q))
