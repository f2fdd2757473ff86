"""GPU: retrieval evaluation (ops.retrieval_first_positive / retrieval_reduce, retrieval.retrieval_metrics,
EmbeddingNet.calculate_retrieval_metrics, tools/train.py TRAIN.retrieval_ks / TRAIN.monitor) against the float64 restatement
tests/retrieval_ref.py.  Exact where the fp32 arithmetic is exact (small integer embeddings), inside the rank interval that the
project's distance error bound allows everywhere else; every query is judged."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recipes as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_ref as RR  # noqa: E402

KS = (1, 10, 100, 1000)


def _A(e):
    """tests/test_eval_path_gpu.py::_A, verbatim: the project's bound on |d2_gpu - d2_f64| / (|q|^2 + |x|^2)."""
    return 2e-6 if e <= 512 else 4e-6 * (e / 512) ** 0.5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)


def _run(q, ql, x, xl, dev):
    """(rank, pos_index, pos_d2) as NumPy; x is None: leave-one-out."""
    from embeddingnet_amd import ops
    out = ops.retrieval_first_positive(_t(q, dev), _t(ql, dev, torch.int32), None if x is None else _t(x, dev),
                                       None if x is None else _t(xl, dev, torch.int32))
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.int32 and out[2].dtype == torch.float32
    return tuple(o.cpu().numpy() for o in out)


# ---- 6. exact, with ties ------------------------------------------------------------------------------------------------------
def _integer_case(rs, nq, n, e, self_exclude):
    """Entries in 0..3: every product and partial sum is a small integer, so the fp32 d2 is exact.  Rows are duplicated across
    classes (equal-distance positive / negative pairs decide by index), some classes have one member, labels are shuffled, and
    one query's label is absent from the gallery."""
    x = rs.randint(0, 4, size=(n, e)).astype(np.float32)
    n_classes = max(2, n // 5)
    xl = rs.randint(0, n_classes, size=n).astype(np.int32) * 3 - 7          # arbitrary, negative values included
    for _ in range(max(1, n // 4)):                                        # duplicates, usually across classes
        a, b = rs.randint(0, n, 2)
        x[a] = x[b]
    if n >= 4:
        xl[rs.randint(0, n)] = 1000001                                      # classes of one member
        xl[rs.randint(0, n)] = 1000002
    if self_exclude:
        return x, xl, x, xl
    q = rs.randint(0, 4, size=(nq, e)).astype(np.float32)
    ql = xl[rs.randint(0, n, size=nq)].copy()
    for _ in range(max(1, nq // 3)):                                       # queries that ARE gallery rows: d2 = 0 ties
        q[rs.randint(0, nq)] = x[rs.randint(0, n)]
    ql[rs.randint(0, nq)] = -123456                                         # a label the gallery does not have
    return q, ql, x, xl


# The last three reach the walk shapes that the smaller ones do not (retrieval_plan in csrc/retrieval.hip): 1500 leave-one-out
# is 24 x 24 tiles of 64 with two gallery tiles per workgroup and a ragged last tile; 4000 leave-one-out takes the 128-row
# tiles, 32 x 32 of them in 16 splits of two, the own column excluded across tiles; 300 x 16400 is 3 x 129 tiles of 128, one
# tile per split, ragged in both dimensions.
EXACT_SHAPES = [(1, 5, 0), (3, 7, 0), (65, 130, 0), (130, 257, 0), (257, 1000, 0), (2, 2, 1), (64, 64, 1), (65, 65, 1), (1000, 1000, 1),
                (1500, 1500, 1), (4000, 4000, 1), (300, 16400, 0)]


@pytest.mark.parametrize("e", [5, 33, 64])
def test_exact_with_ties(dev, e):
    rs = np.random.RandomState(100 + e)
    for nq, n, self_exclude in EXACT_SHAPES:
        q, ql, x, xl = _integer_case(rs, nq, n, e, bool(self_exclude))
        want = RR.ranks_exact(RR.sqdist64(q, x), ql, xl, bool(self_exclude))
        got = _run(q, ql, None if self_exclude else x, None if self_exclude else xl, dev)
        tag = f"e={e} nq={nq} n={n} self_exclude={self_exclude}"
        assert np.array_equal(got[0], want[0]), (tag, np.flatnonzero(got[0] != want[0])[:8])
        assert np.array_equal(got[1], want[1]), (tag, np.flatnonzero(got[1] != want[1])[:8])
        assert np.array_equal(got[2], want[2].astype(np.float32)), tag
        ties = int(np.sum(want[2] == 0))
        print(f"{tag}: {int((want[0] == 0).sum())} queries without a positive, {ties} first positives at d2 = 0, max rank {want[0].max()}")
    assert (want[0] == 0).any() and want[0].max() > 64


# ---- 7. float64 interval at scale -----------------------------------------------------------------------------------------------
def _judge(tag, got, q, x, ql, xl, self_exclude, A, lo, hi, det, rows=None):
    """Every query: r_lo <= rank <= r_hi, pos_d2 within B of the float64 d2 of the reported pos_index, and pos_index a positive
    that the bound allows to be the nearest one."""
    rank, pos, pd = got
    rows = np.arange(len(q)) if rows is None else rows
    rank, pos, pd = rank[rows], pos[rows], pd[rows]
    q64, x64 = np.asarray(q, np.float64)[rows], np.asarray(x, np.float64)
    has = lo > 0
    assert np.array_equal(rank > 0, has) and np.all(pos[~has] == -1) and np.all(np.isinf(pd[~has]))
    assert np.all((pos[has] >= 0) & (pos[has] < len(x)))
    xp = x64[pos[has]]
    d_ref = ((q64[has] - xp) ** 2).sum(1)
    B = A * ((q64[has] ** 2).sum(1) + (xp ** 2).sum(1))
    worst = float((np.abs(pd[has] - d_ref) / B).max())
    width = hi - lo
    print(f"{tag}: {len(rows)} queries, worst |pos_d2 - ref| / B = {worst:.3f}, ambiguous share {np.mean(width != 0):.4%}, "
          f"max interval width {int(width.max())}, {int(np.sum(rank != det['rank']))} ranks differ from the float64 order, "
          f"max rank {int(rank.max())}")
    assert np.all(lo <= rank) and np.all(rank <= hi), np.flatnonzero((rank < lo) | (rank > hi))[:8]
    assert worst <= 1.0
    assert np.all(np.asarray(xl)[pos[has]] == np.asarray(ql)[rows][has])
    if self_exclude:
        assert np.all(pos[has] != rows[has])
    assert np.all(d_ref - B <= det['pos_hi'][has])
    return lo, hi


def _judge_metrics(tag, rank, lo, hi, dev):
    from embeddingnet_amd import ops
    hits, nv, s = ops.retrieval_reduce(_t(rank, dev, torch.int32), KS)
    hits, nv, s = hits.cpu().numpy(), int(nv.item()), float(s.item())
    v = lo > 0
    assert nv == int(v.sum()) and nv > 0
    for k, h in zip(KS, hits):
        rec = h / nv
        print(f"{tag}: recall@{k} = {rec:.4f} in [{np.mean(hi[v] <= k):.4f}, {np.mean(lo[v] <= k):.4f}]")
        assert np.mean(hi[v] <= k) <= rec <= np.mean(lo[v] <= k)
        assert h == int(np.sum((rank > 0) & (rank <= k)))
    mrr = s / nv
    print(f"{tag}: mrr = {mrr:.6f} in [{np.mean(1.0 / hi[v]):.6f}, {np.mean(1.0 / lo[v]):.6f}]")
    assert np.mean(1.0 / hi[v]) - 1e-6 <= mrr <= np.mean(1.0 / lo[v]) + 1e-6


@functools.lru_cache(maxsize=None)
def _fit_input(seed):
    """The inputs test_retrieval_cpu.py::test_interval_inputs_are_fit checks, with their float64 intervals (computed once)."""
    g, gl, _, _ = R.knn_data(305, 20, 256, 1.2, 10, seed)
    lo, hi, det = RR.rank_interval(g, g, gl, gl, True, _A(256), details=True, gap_ks=(1, 5, 64))
    return g, gl.astype(np.int32), lo, hi, det


@pytest.mark.parametrize("seed", [5, 77])
def test_interval_leave_one_out_6100(dev, seed):
    g, gl, lo, hi, det = _fit_input(seed)
    got = _run(g, gl, None, None, dev)
    _judge(f"leave-one-out n=6100 e=256 seed {seed}", got, g, g, gl, gl, True, _A(256), lo, hi, det)
    _judge_metrics(f"seed {seed}", got[0], lo, hi, dev)


@pytest.mark.parametrize("name,args,shuffle", [("queries vs gallery 512 x 6100 x 256", (305, 20, 256, 1.2, 512, 5), True),
                                               ("e=4096 64 x 350", (50, 7, 4096, 1.2, 64, 9), True),
                                               ("ragged e=70 130 x 1000", (100, 10, 70, 1.2, 130, 11), False)])
def test_interval_separate_queries(dev, name, args, shuffle):
    g, gl, q, ql = R.knn_data(*args)
    if shuffle:                                            # labels in no particular order
        perm = np.random.RandomState(1).permutation(len(g))
        g, gl = g[perm], gl[perm]
    e = args[2]
    lo, hi, det = RR.rank_interval(q, g, ql, gl, False, _A(e), details=True)
    got = _run(q, ql, g, gl, dev)
    _judge(name, got, q, g, ql, gl, False, _A(e), lo, hi, det)
    _judge_metrics(name, got[0], lo, hi, dev)
    # and the same gallery leave-one-out
    lo, hi, det = RR.rank_interval(g, g, gl, gl, True, _A(e), details=True) if len(g) <= 1000 else (None, None, None)
    if lo is not None:
        got = _run(g, gl, None, None, dev)
        _judge(name + " (gallery, leave-one-out)", got, g, g, gl, gl, True, _A(e), lo, hi, det)


# ---- 8. beyond what can be materialised or selected ------------------------------------------------------------------------------
def test_gallery_of_131072_without_the_matrix(dev):
    from embeddingnet_amd import ops
    n, e = 131072, 64
    g = R.clustered_embeddings(21, 4096, 32, e, 0.6)
    gl = np.repeat(np.arange(4096), 32).astype(np.int32)
    perm = np.random.RandomState(2).permutation(n)
    g, gl = np.ascontiguousarray(g[perm]), gl[perm]
    gt, lt = _t(g, dev), _t(gl, dev, torch.int32)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    rank, pos, pd = ops.retrieval_first_positive(gt, lt)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"n = {n}: peak device memory over the call {peak / 2 ** 20:.1f} MiB beyond the operands (the matrix would be 64 GiB)")
    assert peak < 64 << 20
    rows = np.arange(0, n, n // 512)
    assert len(rows) == 512
    lo, hi, det = RR.rank_interval(g, g, gl, gl, True, _A(e), rows=rows, details=True)
    got = (rank.cpu().numpy(), pos.cpu().numpy(), pd.cpu().numpy())
    assert got[0].shape == (n,) and got[0].min() >= 0 and got[0].max() <= n
    _judge(f"n={n} e={e}, 512 queries at stride {n // 512}", got, g, g, gl, gl, True, _A(e), lo, hi, det, rows=rows)
    m = RR.metrics(got[0], (1, 100, 1000))
    print(f"n = {n}: recall@1 {m['recall@1']:.4f} recall@100 {m['recall@100']:.4f} recall@1000 {m['recall@1000']:.4f} mrr {m['mrr']:.4f}")


# ---- 9. agreement with the materialising path -----------------------------------------------------------------------------------
def test_agrees_with_cross_distances_and_topk(dev):
    from embeddingnet_amd import ops
    g, gl, lo, hi, det = _fit_input(5)
    n = len(g)
    gt = _t(g, dev)
    rank = _run(g, gl, None, None, dev)[0]
    d = ops.cross_distances(gt, gt, squared=True)
    d[torch.arange(n, device=dev), torch.arange(n, device=dev)] = float("inf")
    for i, k in enumerate((1, 5, 64)):
        _, idx = ops.topk_smallest(d, k)
        found = (gl[idx.cpu().numpy()] == gl[:, None]).any(1)
        kth = det["kth"][:, i]
        judged = (lo == hi) & (kth[:, 1] - kth[:, 0] > 2 * det["bmax"])
        print(f"K = {k}: {int(judged.sum())} of {n} queries judged ({judged.mean():.2%}), "
              f"{int(np.sum(found[judged] != ((rank > 0) & (rank <= k))[judged]))} disagree")
        assert judged.mean() >= 0.95
        assert np.array_equal(found[judged], ((rank > 0) & (rank <= k))[judged])


# ---- 10. reproducibility, other streams, graph replay ----------------------------------------------------------------------------
def test_reproducible_on_streams_and_under_graph_replay(dev):
    from embeddingnet_amd import ops
    from embeddingnet_amd.retrieval import retrieval_metrics
    g, gl, _, _ = R.knn_data(60, 12, 96, 1.2, 10, 4)
    gt, lt = _t(g, dev), _t(gl, dev, torch.int32)
    kt = _t(np.array(KS), dev, torch.int32)
    first = ops.retrieval_first_positive(gt, lt)
    red = ops.retrieval_reduce(first[0], kt)
    again = ops.retrieval_first_positive(gt, lt)
    for a, b in zip(first + red, again + ops.retrieval_reduce(again[0], kt)):
        assert torch.equal(a, b)
    # other label values (other bits in the tiles' label filters, so other tiles skipped by the nearest-positive pass) and a
    # gallery large enough for 128-row tiles: the same answer
    relabelled = ops.retrieval_first_positive(gt, lt * 7919 - 100003)
    assert all(torch.equal(a, b) for a, b in zip(first, relabelled))
    big, bl = R.knn_data(640, 4, 32, 1.2, 10, 8)[:2]
    bt, blt = _t(big, dev), _t(bl, dev, torch.int32)
    perm = torch.randperm(640, generator=torch.Generator().manual_seed(3)).to(dev).to(torch.int32)
    assert all(torch.equal(a, b) for a, b in zip(ops.retrieval_first_positive(bt, blt), ops.retrieval_first_positive(bt, perm[blt.long()])))
    m0, m1 = retrieval_metrics(g, gl, ks=KS, device=dev), retrieval_metrics(g, gl, ks=KS, device=dev)
    assert m0.keys() == m1.keys() and all(np.array_equal(m0[k], m1[k]) for k in m0)
    assert np.array_equal(m0["ranks"], first[0].cpu().numpy())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.retrieval_first_positive(gt, lt)
        red_side = ops.retrieval_reduce(on_side[0], kt)
    side.synchronize()
    for a, b in zip(first + red, on_side + red_side):
        assert torch.equal(a, b)
    # capture the new launches only; the counters and keys are re-zeroed by the library's own kernel on every replay
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = ops.retrieval_first_positive(gt, lt)
        cap_red = ops.retrieval_reduce(cap[0], kt)
    for _ in range(2):
        for t in cap + cap_red:
            t.fill_(-1) if t.dtype != torch.float64 else t.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first + red, cap + cap_red):
            assert torch.equal(a, b)


# ---- 11. unaligned pointers, NaN rows ---------------------------------------------------------------------------------------------
def test_unaligned_pointers_and_nan_query_row(dev):
    from embeddingnet_amd import ops
    g, gl, q, ql = R.knn_data(16, 8, 64, 1.2, 64, 62)
    qs, xs = torch.empty(q.size + 1, device=dev), torch.empty(g.size + 1, device=dev)
    qt, xt = qs[1:].view(q.shape), xs[1:].view(g.shape)
    qt.copy_(_t(q, dev))
    xt.copy_(_t(g, dev))
    assert qt.data_ptr() % 16 == 4 and xt.data_ptr() % 16 == 4 and qt.is_contiguous() and xt.is_contiguous()
    out = ops.retrieval_first_positive(qt, _t(ql, dev, torch.int32), xt, _t(gl, dev, torch.int32))
    got = tuple(o.cpu().numpy() for o in out)
    lo, hi, det = RR.rank_interval(q, g, ql, gl, False, _A(64), details=True)
    _judge("unaligned 64 x 128 x 64", got, q, g, ql, gl, False, _A(64), lo, hi, det)
    aligned = _run(q, ql, g, gl, dev)
    assert all(np.array_equal(a, b) for a, b in zip(got, aligned))          # the scalar loader feeds the same arithmetic
    # a NaN query row: every d2 of that row is NaN = +inf, the order is the index order; nothing faults, the other rows are untouched
    qn = q.copy()
    qn[3, 5] = np.nan
    rank, pos, pd = _run(qn, ql, g, gl, dev)
    n = len(g)
    assert 0 <= rank.min() and rank.max() <= n
    positives = np.flatnonzero(gl == ql[3])
    assert pos[3] == positives[0] and rank[3] == 1 + int(np.sum(gl[:positives[0]] != ql[3])) and np.isinf(pd[3])
    keep = np.arange(len(q)) != 3
    assert all(np.array_equal(a[keep], b[keep]) for a, b in zip((rank, pos, pd), aligned))
    # leave-one-out with a NaN row in the gallery as well
    gn = g.copy()
    gn[7] = np.nan
    rank, pos, _ = _run(gn, gl, None, None, dev)
    assert 0 <= rank.min() and rank.max() <= n and np.all((pos >= -1) & (pos < n)) and pos[7] != 7
    assert np.all(gl[pos[pos >= 0]] == gl[pos >= 0])


# ---- 12. model level ------------------------------------------------------------------------------------------------------------
def test_model_level_metrics(tmp_path, dev):
    from embeddingnet_amd.datagenerators import SyntheticDataLoader
    from embeddingnet_amd.models import TripletNet
    from embeddingnet_amd.retrieval import retrieval_metrics
    params = {"model": dict(input_shape=[64, 64, 3], encodings_len=64, mode="triplet", distance_type="l2",
                            backbone_name="simple2", backbone_weights=None, freeze_backbone=False,
                            embeddings_normalization=True, device=dev, seed=0),
              "dataloader": {}, "generator": {}, "train": {}, "general": {"work_dir": str(tmp_path), "project_name": "p"}}
    data = SyntheticDataLoader(6, 16, (64, 64, 3), noise=0.2, validate=True, val_ratio=0.25, seed=3)
    net = TripletNet(params, training=True)
    got = net.calculate_retrieval_metrics(data, ks=(1, 3, 100))
    enc = np.concatenate([net.base_model.predict(data.val_data[c]) for c in data.val_data])
    labels = [c for c in data.val_data for _ in range(len(data.val_data[c]))]
    want = retrieval_metrics(enc, labels, ks=(1, 3, 100), device=dev)
    assert set(got) == {"recall@1", "recall@3", "recall@100", "mrr", "n_queries", "n_valid", "ranks"}
    assert got["n_queries"] == got["n_valid"] == len(labels) == 24 and got["ranks"].dtype == np.int32
    assert all(np.array_equal(got[k], want[k]) for k in want)
    assert 0 <= got["recall@1"] <= got["recall@3"] <= got["recall@100"] == 1.0
    # the dict form, and small batches, change nothing
    assert all(np.array_equal(want[k], v) for k, v in retrieval_metrics({"encodings": enc, "labels": labels}, ks=(1, 3, 100), device=dev).items())
    small = net.calculate_retrieval_metrics(data, ks=(1, 3, 100), batch_size=32)
    assert np.array_equal(small["ranks"], got["ranks"])
    with pytest.raises(ValueError, match="encoded_training_data"):
        net.calculate_retrieval_metrics(data, gallery="train")
    net.encoded_training_data = net.generate_encodings(data, max_n_samples=10, shuffle=False)
    tr = net.calculate_retrieval_metrics(data, ks=(1, 5), gallery="train")
    ref = retrieval_metrics(enc, labels, ks=(1, 5), gallery=net.encoded_training_data["encodings"],
                            gallery_labels=net.encoded_training_data["labels"], device=dev)
    assert all(np.array_equal(tr[k], ref[k]) for k in ref) and tr["n_valid"] == 24


# ---- 13. CLI ----------------------------------------------------------------------------------------------------------------------
def _start(tmp_path, name, text):
    """tools/train.py on `text` in a fresh child process under its own time limit: 2 epochs, 10 synthetic classes."""
    wd = tmp_path / name
    cfg_path = tmp_path / f"{name}.yml"
    cfg_path.write_text(text.replace("work_dirs/", str(wd) + "/"))
    project = [l.split("'")[1] for l in text.splitlines() if "project_name" in l][0]
    proc = subprocess.Popen(["timeout", "-k", "10", "500", sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path),
                             "--synthetic", "10", "--max_epochs", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return proc, wd / project / "plots" / "history.npz"


def _finish(started):
    proc, hist = started
    out, err = proc.communicate(timeout=600)
    assert proc.returncode == 0, out[-2000:] + err[-2000:]
    return out, np.load(hist)


def test_train_cli_logs_and_monitors_recall(tmp_path):
    text = open(os.path.join(ROOT, "configs", "simple2_retrieval_synthetic.yml")).read()
    stock = open(os.path.join(ROOT, "configs", "simple2_synthetic.yml")).read()
    removed = "\n".join(l for l in text.splitlines() if "retrieval_ks" not in l and "monitor :" not in l) + "\n"
    assert "retrieval_ks" not in removed and "monitor" not in removed.split("TRAIN:")[1]
    runs = [_start(tmp_path, name, t) for name, t in (("with", text), ("removed", removed), ("stock", stock))]   # side by side
    (out, hist), (_, h_removed), (out_stock, h_stock) = [_finish(r) for r in runs]
    for key in ("val_recall@1", "val_recall@5", "val_recall@10", "val_mrr"):
        assert hist[key].shape == (2,) and np.all((hist[key] >= 0) & (hist[key] <= 1)), key
        assert f" - {key} " in out
    assert np.all(hist["val_recall@1"] <= hist["val_recall@5"]) and np.all(hist["val_recall@5"] <= hist["val_recall@10"])
    improved = [l for l in out.splitlines() if "improved to" in l]
    assert improved and all(l.startswith("val_recall@1 improved to ") for l in improved)
    assert float(improved[0].split("improved to ")[1].split(",")[0]) == pytest.approx(hist["val_recall@1"][0], abs=1e-5)
    # the keys removed: the run of the stock config, bit for bit
    assert np.array_equal(h_removed["loss"], h_stock["loss"]) and np.array_equal(h_removed["val_loss"], h_stock["val_loss"])
    assert np.array_equal(hist["loss"], h_stock["loss"])           # the evaluation does not disturb training either
    assert set(h_stock.files) == {"loss", "val_loss"} and "val_loss improved to" in out_stock
