"""GPU: MAP@R / R-precision (ops.retrieval_positive_ranks / retrieval_map_reduce, retrieval.retrieval_map_metrics,
EmbeddingNet.calculate_map_at_r, tools/train.py TRAIN.retrieval_map) against the float64 restatement tests/retrieval_map_ref.py.
Exact where the fp32 arithmetic is exact (small integer embeddings), bitwise equal to ops.retrieval_first_positive on the first
positive, inside the position interval that the project's distance error bound allows everywhere else; every positive is judged."""
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
import retrieval_map_ref as MR  # noqa: E402
import retrieval_ref as RR  # noqa: E402

R_MAX = 4096


def _A(e):
    """tests/test_eval_path_gpu.py::_A, verbatim: the project's bound on |d2_gpu - d2_f64| / (|q|^2 + |x|^2)."""
    return 2e-6 if e <= 512 else 4e-6 * (e / 512) ** 0.5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)


def _run(q, ql, x, xl, dev, **kw):
    """(offset, pos_index, pos_rank) as NumPy; x is None: leave-one-out."""
    from embeddingnet_amd import ops
    out = ops.retrieval_positive_ranks(_t(q, dev), _t(ql, dev, torch.int32), None if x is None else _t(x, dev),
                                       None if x is None else _t(xl, dev, torch.int32), **kw)
    assert out[0].dtype == torch.int64 and out[1].dtype == torch.int32 and out[2].dtype == torch.int32
    return tuple(o.cpu().numpy() for o in out)


def _reduce(offset, pos_rank, dev):
    """ops.retrieval_map_reduce -> the dict layout of MR.metrics_from_positions."""
    from embeddingnet_amd import ops
    a, r, ap, sums, nv = ops.retrieval_map_reduce(_t(offset, dev, torch.int64), _t(pos_rank, dev, torch.int32))
    assert a.dtype == r.dtype == ap.dtype == sums.dtype == torch.float64 and nv.dtype == torch.int32
    sums, nv = sums.cpu().numpy(), int(nv.item())
    mean = lambda s: float(s) / nv if nv else float("nan")
    return {"ap@r": a.cpu().numpy(), "r_precision_q": r.cpu().numpy(), "ap": ap.cpu().numpy(), "map@r": mean(sums[0]),
            "r_precision": mean(sums[1]), "map": mean(sums[2]), "n_valid": nv}


def _raw(qt, qlt, xt, xlt, num_classes, capacity, ws=None, out=None, alloc=None):
    """The C entries on the caller's buffers (no host read, so a graph can capture it): -> (offset, pos_index, pos_rank, status,
    ap_at_r, r_precision, ap, sums, n_valid).  alloc: the length of pos_index / pos_rank when it is not `capacity`."""
    from embeddingnet_amd import _lib
    from embeddingnet_amd._lib import check, ptr, stream
    lib = _lib.lib()
    self_exclude = xt is None
    if self_exclude:
        xt, xlt = qt, qlt
    nq, e = qt.shape
    n = xt.shape[0]
    d = qt.device
    if ws is None:
        ws = torch.empty(lib.embnet_retrieval_positive_ranks_workspace_bytes(nq, n, num_classes, capacity), dtype=torch.uint8, device=d)
    if out is None:
        out = (torch.empty(nq + 1, dtype=torch.int64, device=d), torch.empty(alloc or capacity, dtype=torch.int32, device=d),
               torch.empty(alloc or capacity, dtype=torch.int32, device=d), torch.empty(1, dtype=torch.int32, device=d)) + \
              tuple(torch.empty(nq, dtype=torch.float64, device=d) for _ in range(3)) + \
              (torch.empty(3, dtype=torch.float64, device=d), torch.empty((), dtype=torch.int32, device=d))
    offset, idx, rank, status, a, r, ap, sums, nv = out
    check(lib.embnet_retrieval_positive_ranks(ptr(qt), ptr(qlt), nq, ptr(xt), ptr(xlt), n, e, int(self_exclude), num_classes, capacity,
                                              ptr(offset), ptr(idx), ptr(rank), ptr(status), ptr(ws), ws.numel(), stream()))
    return out


def _raw_reduce(out):
    from embeddingnet_amd import _lib
    from embeddingnet_amd._lib import check, ptr, stream
    offset, idx, rank, status, a, r, ap, sums, nv = out
    check(_lib.lib().embnet_retrieval_map_reduce(ptr(offset), ptr(rank), offset.numel() - 1, ptr(a), ptr(r), ptr(ap), ptr(sums), ptr(nv),
                                                 stream()))


def _same_metrics(tag, got, want):
    """Per-query values: NaN in the same places, equal up to the few ulp a different summation order allows."""
    for key in ("ap@r", "r_precision_q", "ap"):
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), (tag, key)
        assert np.allclose(got[key], want[key], rtol=1e-14, atol=0, equal_nan=True), (tag, key)
    assert got["n_valid"] == want["n_valid"], tag
    for key in ("map@r", "r_precision", "map"):
        assert (np.isnan(want[key]) and np.isnan(got[key])) or abs(got[key] - want[key]) <= 1e-13 * abs(want[key]), (tag, key)


# ---- 1. exact, with ties ------------------------------------------------------------------------------------------------------
FORCED_SIZES = (1, 2, 3, 64, 65, 66, 129, 1030)             # the wave-sort / LDS-sort boundaries, multi-step bitonic stages


def _integer_case(rs, nq, n, e, self_exclude, forced):
    """Entries in 0..3: every product and partial sum is a small integer, so the fp32 d2 is exact.  Rows are duplicated across
    classes (equal-distance positive / negative pairs decide by index), labels are dense ids in shuffled order, classes of forced
    sizes where asked for, and (separate queries) one query's label has no gallery member."""
    x = rs.randint(0, 4, size=(n, e)).astype(np.float32)
    if forced:
        xl = np.concatenate([np.full(s, c) for c, s in enumerate(FORCED_SIZES)])
        rest = n - len(xl)
        assert rest > 0
        xl = np.concatenate([xl, len(FORCED_SIZES) + rs.randint(0, max(2, rest // 5), size=rest)])
    else:
        xl = rs.randint(0, max(2, n // 5), size=n)
    xl = xl[rs.permutation(n)].astype(np.int32)
    for _ in range(max(1, n // 4)):                                        # duplicates, usually across classes
        a, b = rs.randint(0, n, 2)
        x[a] = x[b]
    num_classes = int(xl.max()) + 2                                        # the last id has no gallery member
    if self_exclude:
        return x, xl, x, xl, num_classes
    q = rs.randint(0, 4, size=(nq, e)).astype(np.float32)
    ql = xl[rs.randint(0, n, size=nq)].copy()
    if forced:
        ql[:len(FORCED_SIZES)] = np.arange(len(FORCED_SIZES))              # a query of every forced class
    for _ in range(max(1, nq // 3)):                                       # queries that ARE gallery rows: d2 = 0 ties
        q[rs.randint(0, nq)] = x[rs.randint(0, n)]
    ql[rs.randint(len(FORCED_SIZES) if forced else 0, nq)] = num_classes - 1
    return q, ql, x, xl, num_classes


# test_retrieval_gpu.py's EXACT_SHAPES, the last small one of each mode with n raised to hold the forced class sizes; the last
# two are its 128-row-tile shapes (two gallery tiles per workgroup; one tile per split, ragged in both dimensions)
EXACT_SHAPES = [(1, 5, 0, 0), (3, 7, 0, 0), (65, 130, 0, 0), (130, 257, 0, 0), (257, 1500, 0, 1), (2, 2, 1, 0), (64, 64, 1, 0),
                (65, 65, 1, 0), (1500, 1500, 1, 1), (4000, 4000, 1, 0), (300, 16400, 0, 0)]


@pytest.mark.parametrize("e", [5, 33, 64])
def test_exact_with_ties(dev, e):
    rs = np.random.RandomState(200 + e)
    seen = set()
    for nq, n, self_exclude, forced in EXACT_SHAPES:
        q, ql, x, xl, num_classes = _integer_case(rs, nq, n, e, bool(self_exclude), bool(forced))
        want = MR.positions_exact(RR.sqdist64(q, x), ql, xl, bool(self_exclude))
        got = _run(q, ql, None if self_exclude else x, None if self_exclude else xl, dev, num_classes=num_classes)
        tag = f"e={e} nq={nq} n={n} self_exclude={self_exclude}"
        for g, w, name in zip(got, want, ("offset", "pos_index", "pos_rank")):
            assert g.shape == w.shape and np.array_equal(g, w), (tag, name, np.flatnonzero(g != w)[:8])
        _same_metrics(tag, _reduce(got[0], got[2], dev), MR.metrics_from_positions(*want[::2]))
        seen |= set(np.diff(want[0]).tolist())
        print(f"{tag}: {len(want[1])} positives, {int(np.sum(np.diff(want[0]) == 0))} queries without one, largest R {np.diff(want[0]).max()}")
    assert {0, 1, 2, 3, 63, 64, 65, 66, 128, 129, 1029, 1030} <= seen


# ---- 2. the first positive is ops.retrieval_first_positive's, bit for bit -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit_input(seed):
    """The inputs test_retrieval_map_cpu.py::test_interval_inputs_are_fit checks, with their float64 intervals (computed once)."""
    g, gl, _, _ = R.knn_data(305, 20, 256, 1.2, 10, seed)
    off, idx, lo, hi = MR.position_interval(g, g, gl, gl, True, _A(256))
    return g, gl.astype(np.int32), off, idx, lo, hi


def _first_matches(tag, got, first):
    off, idx, pos = got
    rank, fidx, _ = (t.cpu().numpy() for t in first)
    has = rank > 0
    assert np.array_equal(np.diff(off) > 0, has), tag
    assert np.array_equal(pos[off[:-1][has]], rank[has]) and np.array_equal(idx[off[:-1][has]], fidx[has]), tag
    print(f"{tag}: {int(has.sum())} first positives agree bit for bit")


def test_first_positive_identity(dev):
    from embeddingnet_amd import ops
    g, gl, _, _, _, _ = _fit_input(5)
    gt, lt = _t(g, dev), _t(gl, dev, torch.int32)
    got = tuple(o.cpu().numpy() for o in ops.retrieval_positive_ranks(gt, lt))
    _first_matches("leave-one-out n=6100 e=256", got, ops.retrieval_first_positive(gt, lt))
    # ragged e = 70 through the scalar loader, from an unaligned base pointer, queries against a gallery
    x, xl, q, ql = R.knn_data(100, 10, 70, 1.2, 130, 11)
    qs, xs = torch.empty(q.size + 1, device=dev), torch.empty(x.size + 1, device=dev)
    qt, xt = qs[1:].view(q.shape), xs[1:].view(x.shape)
    qt.copy_(_t(q, dev))
    xt.copy_(_t(x, dev))
    assert qt.data_ptr() % 16 == 4 and xt.data_ptr() % 16 == 4
    qlt, xlt = _t(ql, dev, torch.int32), _t(xl, dev, torch.int32)
    got = tuple(o.cpu().numpy() for o in ops.retrieval_positive_ranks(qt, qlt, xt, xlt))
    _first_matches("ragged e=70 130 x 1000, unaligned", got, ops.retrieval_first_positive(qt, qlt, xt, xlt))
    aligned = _run(q, ql, x, xl, dev)
    assert all(np.array_equal(a, b) for a, b in zip(got, aligned))          # the scalar loader feeds the same arithmetic


# ---- 3. float64 interval ------------------------------------------------------------------------------------------------------
def _judge(tag, got, ref, dev):
    """Every positive: lo <= pos_rank <= hi; per query pos_rank strictly increasing and pos_index exactly the query's positives;
    the three means inside the bounds of the intervals (1e-12 slack)."""
    off, idx, pos = got
    roff, ridx, lo, hi = ref
    assert np.array_equal(off, roff), tag
    row = np.repeat(np.arange(len(off) - 1), np.diff(off))
    inner = np.ones(len(pos), bool)
    inner[off[:-1][np.diff(off) > 0]] = False
    assert np.all(np.diff(pos)[inner[1:]] > 0), tag                        # strictly increasing within a query
    by_index = np.lexsort((idx, row))                                      # the restatement lists a query's positives by index
    assert np.array_equal(idx[by_index], ridx), tag
    p = pos[by_index]
    bad = np.flatnonzero((p < lo) | (p > hi))
    print(f"{tag}: {len(pos)} positives of {len(off) - 1} queries, open share {np.mean(hi > lo):.4%}, max width {int((hi - lo).max())}, "
          f"{len(bad)} outside")
    assert len(bad) == 0, (tag, bad[:8], p[bad[:8]], lo[bad[:8]], hi[bad[:8]])
    lower, upper = MR.metric_bounds(roff, lo, hi)
    m = _reduce(off, pos, dev)
    for key in ("map@r", "r_precision", "map"):
        print(f"{tag}: {key} = {m[key]:.6f} in [{lower[key]:.6f}, {upper[key]:.6f}]")
        assert lower[key] - 1e-12 <= m[key] <= upper[key] + 1e-12, (tag, key)
    assert m["n_valid"] == lower["n_valid"]
    return m


@pytest.mark.parametrize("seed", [5, 77])
def test_interval_leave_one_out_6100(dev, seed):
    from embeddingnet_amd.retrieval import retrieval_map_metrics
    g, gl, off, idx, lo, hi = _fit_input(seed)
    got = _run(g, gl, None, None, dev)
    m = _judge(f"leave-one-out n=6100 e=256 seed {seed}", got, (off, idx, lo, hi), dev)
    top = retrieval_map_metrics(g, gl, device=dev)                           # the public function: the same numbers
    assert set(top) == {"map@r", "r_precision", "map", "n_queries", "n_valid", "ap@r", "r"}
    assert all(top[k] == m[k] for k in ("map@r", "r_precision", "map", "n_valid")) and top["n_queries"] == 6100
    assert np.array_equal(top["ap@r"], m["ap@r"]) and top["ap@r"].dtype == np.float64
    assert top["r"].dtype == np.int32 and np.array_equal(top["r"], np.diff(off))


# ---- 4. queries against a large gallery -------------------------------------------------------------------------------------------
def test_queries_against_a_gallery_of_131072(dev):
    g, gl, q, ql = R.knn_data(1024, 128, 64, 0.6, 512, 23)
    assert g.shape == (131072, 64) and q.shape == (512, 64)
    perm = np.random.RandomState(2).permutation(len(g))                     # shuffled labels: pass 1 skips nothing
    g, gl = np.ascontiguousarray(g[perm]), gl[perm]
    got = _run(q, ql, g, gl, dev)
    ref = MR.position_interval(q, g, ql, gl, False, _A(64))
    assert np.all(np.diff(ref[0]) == 128)
    _judge("512 x 131072 x 64, classes of 128", got, ref, dev)


# ---- 5. reproducibility, other streams, graph replay ----------------------------------------------------------------------------
def test_reproducible_on_streams_and_under_graph_replay(dev):
    from embeddingnet_amd import _lib
    g, gl, q, ql = R.knn_data(60, 12, 96, 1.2, 90, 4)
    perm = np.random.RandomState(5).permutation(len(g))
    xt, xlt = _t(g[perm], dev), _t(gl[perm], dev, torch.int32)
    qt, qlt = _t(q, dev), _t(ql, dev, torch.int32)
    for a, al, b, bl, total in ((xt, xlt, None, None, 720 * 11), (qt, qlt, xt, xlt, 90 * 12)):
        nq, n = a.shape[0], (a if b is None else b).shape[0]
        need = _lib.lib().embnet_retrieval_positive_ranks_workspace_bytes(nq, n, 60, total)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)       # nothing relies on an initialised workspace
        first = _raw(a, al, b, bl, 60, total, ws=ws)
        _raw_reduce(first)
        assert int(first[3].item()) == 0 and int(first[0][-1].item()) == total
        again = _raw(a, al, b, bl, 60, total, ws=ws)                        # the same workspace, now holding the last run's state
        _raw_reduce(again)
        fresh = _raw(a, al, b, bl, 60, total)
        _raw_reduce(fresh)
        for x, y, z in zip(first, again, fresh):
            assert torch.equal(x, y) and torch.equal(x, z)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = _raw(a, al, b, bl, 60, total, ws=ws)
            _raw_reduce(on_side)
        side.synchronize()
        for x, y in zip(first, on_side):
            assert torch.equal(x, y)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        cap = tuple(torch.empty_like(t) for t in first)
        with torch.cuda.graph(graph):
            _raw(a, al, b, bl, 60, total, ws=ws, out=cap)
            _raw_reduce(cap)
        for _ in range(3):                                                  # counters, histogram and status are zeroed by the
            for t in cap:                                                   # library's own kernels on every replay
                t.fill_(-1) if t.dtype != torch.float64 else t.fill_(-1.0)
            graph.replay()
            torch.cuda.synchronize()
            for x, y in zip(first, cap):
                assert torch.equal(x, y)
        want = MR.positions_exact(RR.sqdist64(a.cpu().numpy(), (a if b is None else b).cpu().numpy()), al.cpu().numpy(),
                                  (al if b is None else bl).cpu().numpy(), b is None)
        assert np.array_equal(first[0].cpu().numpy(), want[0])              # and it is the right CSR shape


# ---- 6. limits ----------------------------------------------------------------------------------------------------------------
def _crowd(members, others, rs):
    """Integer rows, e = 5: one class of `members` rows (id 0) and `others` rows of ids 1..3, shuffled."""
    n = members + others
    x = rs.randint(0, 4, size=(n, 5)).astype(np.float32)
    lab = np.concatenate([np.zeros(members, np.int32), 1 + rs.randint(0, 3, size=others).astype(np.int32)])
    perm = rs.permutation(n)
    return x, lab[perm]


def test_r_max_is_reached_and_not_exceeded(dev):
    from embeddingnet_amd import _lib
    from embeddingnet_amd.retrieval import retrieval_map_metrics
    rs = np.random.RandomState(7)
    x, lab = _crowd(R_MAX + 1, 13, rs)                                      # leave-one-out: R = 4096 for the members
    want = MR.positions_exact(RR.sqdist64(x, x), lab, lab, True)
    assert np.diff(want[0]).max() == R_MAX
    got = _run(x, lab, None, None, dev, num_classes=4)
    for g, w, name in zip(got, want, ("offset", "pos_index", "pos_rank")):
        assert np.array_equal(g, w), name
    members = np.flatnonzero(lab == 0)[:64]                                 # 64 of the 4097 long sums, the 13 short ones
    rows = np.concatenate([members, np.flatnonzero(lab != 0)])
    m = _reduce(got[0], got[2], dev)
    for r in rows:
        a, rp, ap = MR.query_metrics(want[2][want[0][r]:want[0][r + 1]])
        assert np.allclose([m["ap@r"][r], m["r_precision_q"][r], m["ap"][r]], [a, rp, ap], rtol=1e-14, atol=0, equal_nan=True), r
    x, lab = _crowd(R_MAX + 2, 5, rs)                                       # R = 4097
    with pytest.raises(_lib.EmbnetError, match="status 2.*R_MAX"):
        _run(x, lab, None, None, dev, num_classes=4)
    with pytest.raises(ValueError, match=r"label 0 has 4098 gallery items"):
        retrieval_map_metrics(x, lab.tolist(), device=dev)


def test_status_for_labels_and_capacity(dev):
    from embeddingnet_amd import _lib
    rs = np.random.RandomState(8)
    x = rs.randint(0, 4, size=(300, 8)).astype(np.float32)
    lab = rs.randint(0, 10, size=300).astype(np.int32)
    bad = lab.copy()
    bad[17] = 10                                                            # id == num_classes
    with pytest.raises(_lib.EmbnetError, match="status 3.*label"):
        _run(x, bad, None, None, dev, num_classes=10)
    with pytest.raises(_lib.EmbnetError, match="status 3.*label"):
        _run(x[:40], np.where(np.arange(40) == 3, -1, lab[:40]).astype(np.int32), x, lab, dev, num_classes=10)
    # a capacity below the number of positives while the buffers have the full size: status 1 and nothing written behind offset —
    # the guard, not a stray write that happened to land in allocated memory
    xt, lt = _t(x, dev), _t(lab, dev, torch.int32)
    full = _raw(xt, lt, None, None, 10, 300 * 300)
    total = int(full[0][-1].item())
    assert int(full[3].item()) == 0 and total == int(sum(c * (c - 1) for c in np.bincount(lab)))
    for capacity in (total - 1, total // 2, 1):
        out = _raw(xt, lt, None, None, 10, capacity, alloc=total)
        out[1].fill_(-7)
        out[2].fill_(-7)
        out = _raw(xt, lt, None, None, 10, capacity, out=out)
        assert int(out[3].item()) == 1, capacity
        assert torch.equal(out[0], full[0])                                  # offset is written in full whatever the status
        assert bool((out[1] == -7).all()) and bool((out[2] == -7).all()), capacity
    exact = _raw(xt, lt, None, None, 10, total)
    assert int(exact[3].item()) == 0 and torch.equal(exact[1], full[1][:total]) and torch.equal(exact[2], full[2][:total])


def test_nan_query_row(dev):
    rs = np.random.RandomState(9)
    x = rs.randint(0, 4, size=(200, 16)).astype(np.float32)
    xl = rs.randint(0, 12, size=200).astype(np.int32)
    q = rs.randint(0, 4, size=(70, 16)).astype(np.float32)
    ql = rs.randint(0, 12, size=70).astype(np.int32)
    q[3, 5] = np.nan                                                        # every d2 of row 3 is NaN = +inf: index order
    want = MR.positions_exact(RR.sqdist64(q, x), ql, xl, False)
    got = _run(q, ql, x, xl, dev, num_classes=12)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    seg = slice(want[0][3], want[0][4])
    positives = np.flatnonzero(xl == ql[3])
    assert np.array_equal(got[1][seg], positives) and np.array_equal(got[2][seg], positives + 1)
    xn = x.copy()
    xn[7] = np.nan                                                          # leave-one-out with a NaN row in the gallery as well
    want = MR.positions_exact(RR.sqdist64(xn, xn), xl, xl, True)
    got = _run(xn, xl, None, None, dev, num_classes=12)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- 7. model and CLI -------------------------------------------------------------------------------------------------------------
def test_model_level_map_at_r(tmp_path, dev):
    from embeddingnet_amd.datagenerators import SyntheticDataLoader
    from embeddingnet_amd.models import TripletNet
    from embeddingnet_amd.retrieval import retrieval_map_metrics
    params = {"model": dict(input_shape=[64, 64, 3], encodings_len=64, mode="triplet", distance_type="l2",
                            backbone_name="simple2", backbone_weights=None, freeze_backbone=False,
                            embeddings_normalization=True, device=dev, seed=0),
              "dataloader": {}, "generator": {}, "train": {}, "general": {"work_dir": str(tmp_path), "project_name": "p"}}
    data = SyntheticDataLoader(6, 16, (64, 64, 3), noise=0.2, validate=True, val_ratio=0.25, seed=3)
    net = TripletNet(params, training=True)
    got = net.calculate_map_at_r(data)
    enc = np.concatenate([net.base_model.predict(data.val_data[c]) for c in data.val_data])
    labels = [c for c in data.val_data for _ in range(len(data.val_data[c]))]
    want = retrieval_map_metrics(enc, labels, device=dev)
    assert set(got) == {"map@r", "r_precision", "map", "n_queries", "n_valid", "ap@r", "r"}
    assert got["n_queries"] == got["n_valid"] == len(labels) == 24 and np.all(got["r"] == 3)
    assert all(np.array_equal(got[k], want[k]) for k in want)
    assert 0 <= got["map@r"] <= got["r_precision"] <= 1 and got["map@r"] <= got["map"] <= 1
    assert all(np.array_equal(want[k], v) for k, v in retrieval_map_metrics({"encodings": enc, "labels": labels}, device=dev).items())
    small = net.calculate_map_at_r(data, batch_size=32)
    assert np.array_equal(small["ap@r"], got["ap@r"])
    with pytest.raises(ValueError, match="encoded_training_data"):
        net.calculate_map_at_r(data, gallery="train")
    net.encoded_training_data = net.generate_encodings(data, max_n_samples=10, shuffle=False)
    tr = net.calculate_map_at_r(data, gallery="train")
    ref = retrieval_map_metrics(enc, labels, gallery=net.encoded_training_data["encodings"],
                                gallery_labels=net.encoded_training_data["labels"], device=dev)
    assert all(np.array_equal(tr[k], ref[k]) for k in ref) and tr["n_valid"] == 24


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


def test_train_cli_logs_and_monitors_map_at_r(tmp_path):
    text = open(os.path.join(ROOT, "configs", "simple2_map_synthetic.yml")).read()
    stock = open(os.path.join(ROOT, "configs", "simple2_synthetic.yml")).read()
    runs = [_start(tmp_path, name, t) for name, t in (("with", text), ("stock", stock))]   # side by side
    (out, hist), (out_stock, h_stock) = [_finish(r) for r in runs]
    for key in ("val_map@r", "val_r_precision"):
        assert hist[key].shape == (2,) and np.all((hist[key] >= 0) & (hist[key] <= 1)), key
        assert f" - {key} " in out
    assert set(hist.files) == {"loss", "val_loss", "val_map@r", "val_r_precision"}
    assert np.all(hist["val_map@r"] <= hist["val_r_precision"])
    improved = [l for l in out.splitlines() if "improved to" in l]
    assert improved and all(l.startswith("val_map@r improved to ") for l in improved)
    assert float(improved[0].split("improved to ")[1].split(",")[0]) == pytest.approx(hist["val_map@r"][0], abs=1e-5)
    assert len(improved) == 1 + int(1.0 - hist["val_map@r"][1] < 1.0 - hist["val_map@r"][0])   # larger is better
    # the stock config writes the history it always wrote, and the evaluation does not disturb training
    assert set(h_stock.files) == {"loss", "val_loss"} and "val_loss improved to" in out_stock
    assert np.array_equal(hist["loss"], h_stock["loss"]) and np.array_equal(hist["val_loss"], h_stock["val_loss"])
