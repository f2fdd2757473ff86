"""GPU parity of the kernels behind every number a user finally reads (kNN accuracy, predict_knn's label, the softmax
pre-training loss and accuracy) at gallery scale, on ragged shapes and on ties: cross_dist / topk_smallest / knn_vote
(csrc/pairwise.hip), softmax_xent / l2norm (csrc/losses.hip), through ops, knn.KNNClassifier and the C ABI.

References are float64, computed here on the host (oracle/knn.py, oracle/losses.py, oracle/pairwise.py).  Every
comparison is element-wise.  Tolerances are derived where they are used; each test prints the figures it judges."""
import numpy as np
import pytest
import torch

import recipes as R
from oracle import knn as oknn
from oracle import losses as olosses
from oracle import pairwise as opair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)


# ---------------------------------------------------------------- 1. cross distances vs float64
def _A(e):
    """test_pairwise_golden's bound on |d2 - d2_ref| for unit rows on this GEMM engine and epilogue."""
    return 2e-6 if e <= 512 else 4e-6 * (e / 512) ** 0.5


def _check_cross(ops, q, x, dev, label, qt=None, xt=None):
    """Both outputs of ops.cross_distances against the float64 formula, element by element, at

        B[r, c] = A(E) * (|q_r|^2 + |x_c|^2).

    A(E) is the bound test_pairwise_golden derives for unit rows (2e-6 up to E = 512, 4e-6 * sqrt(E / 512) beyond): the
    MFMA result is a k-ordered fp32 fmaf chain whose error random-walks as sqrt(E) * 2^-24.  Every term of
    |q|^2 + |x|^2 - 2 q.x carries an error proportional to its own size and |q.x| <= (|q|^2 + |x|^2) / 2, so the bound
    scales with (|q_r|^2 + |x_c|^2) / 2.  A(E) was stated for matrices of about a million elements; the maximum is taken
    here over 6 to 100 million, where a strictly k-ordered float32 chain of the same formula, evaluated on the host,
    reaches 0.87 A at E = 256 and 1.2 A at E = 508 / 510 (1000 x 6100 clustered unit rows) and 0.12 - 0.35 A on the small
    shapes at every scale.  Hence the factor 2 on unit rows: 1.7 over the worst the float32 chain itself does.
    The square-rooted output is judged through |d_gpu^2 - d_ref^2| at the same bound, never through an absolute
    tolerance on d (which would let an error of 1e-3 in a unit-norm distance through)."""
    nq, e = q.shape
    n = x.shape[0]
    qt = _t(q, dev) if qt is None else qt
    xt = _t(x, dev) if xt is None else xt
    a = _A(e)
    for squared in (True, False):
        d = ops.cross_distances(qt, xt, squared=squared)
        assert d.shape == (nq, n) and d.dtype == torch.float32
        d = d.cpu().numpy()
        worst = 0.0
        for r0 in range(0, nq, 256):                              # 256 x 50 000 float64 at a time
            ref, qn, xn = oknn.cross_sqdist64(q[r0:r0 + 256], x)
            np.maximum(ref, 0, out=ref)
            got = d[r0:r0 + 256].astype(np.float64)
            assert np.all(np.isfinite(got)) and np.all(got >= 0), f"{label}: negative or non-finite distance"
            if not squared:
                got *= got
            err = np.abs(got - ref)
            err /= a * (qn[:, None] + xn[None, :])
            if err.max() > 1:
                r, c = np.unravel_index(err.argmax(), err.shape)
                raise AssertionError(f"{label} squared={squared}: |d2 - d2_ref| = {err[r, c]:.2f} B at "
                                     f"[{r0 + r}, {c}] (got {got[r, c]!r}, f64 {ref[r, c]!r}, B = A({e}) (|q|^2 + |x|^2))")
            worst = max(worst, err.max())
        print(f"cross {label} squared={squared}: worst |d2 - d2_ref| = {worst:.3f} B")
    return d


@pytest.mark.parametrize("case", R.EVAL_CROSS_CASES, ids=lambda c: c[0])
def test_cross_distances_clustered_vs_float64(dev, case):
    """The project's clustered unit embeddings at the shapes of predict_knn (one query), of the scalar loader, of the
    first size on the 128x128 tiles and of a gallery of real size; query 0 is bit-identical to a gallery row, whose
    distance must come out >= 0, finite and within the bound of 0 (the fmaxf(..., 0) clamp).  Bound: _check_cross."""
    from embeddingnet_amd import ops
    name, nc, per, e, nq, seed = case
    x, _, q, _ = R.knn_data(nc, per, e, 0.3, nq, seed)
    assert q.shape == (nq, e) and x.shape == (nc * per, e)
    twin = x.shape[0] // 2
    q[0] = x[twin]
    d = _check_cross(ops, q, x, dev, name)                        # the square-rooted output is the one returned
    b = _A(e) * 2 * float((x[twin].astype(np.float64) ** 2).sum())
    assert 0 <= d[0, twin] ** 2 <= b, (d[0, twin], b)


@pytest.mark.parametrize("scale", R.EVAL_CROSS_SCALES)
@pytest.mark.parametrize("shape", R.EVAL_CROSS_RAGGED, ids=lambda s: "x".join(map(str, s)))
def test_cross_distances_unnormalised_vs_float64(dev, shape, scale):
    """embeddings_normalization: False is a legal config: raw randn rows of amplitude 1e-2, 1 and 30 on the ragged
    scalar-loader shapes.  The bound scales with the row norms (_check_cross)."""
    from embeddingnet_amd import ops
    nq, n, e = shape
    q, x = R.randn_rows(61 + e, nq, n, e, scale)
    _check_cross(ops, q, x, dev, f"randn*{scale:g} {nq}x{n}x{e}")


def test_cross_distances_unaligned_pointer(dev):
    """An aligned shape (64, 128, 64) whose q / x start 4 bytes into their storage: the vector loader must not be
    chosen (it would fault or read shifted rows); the scalar loader gives the same distances."""
    from embeddingnet_amd import ops
    x, _, q, _ = R.knn_data(16, 8, 64, 0.3, 64, 62)
    qs, xs = torch.empty(q.size + 1, device=dev), torch.empty(x.size + 1, device=dev)
    qt, xt = qs[1:].view(q.shape), xs[1:].view(x.shape)
    qt.copy_(_t(q, dev))
    xt.copy_(_t(x, dev))
    assert qt.data_ptr() % 16 == 4 and xt.data_ptr() % 16 == 4 and qt.is_contiguous() and xt.is_contiguous()
    _check_cross(ops, q, x, dev, "unaligned 64x128x64", qt=qt, xt=xt)


# ---------------------------------------------------------------- 2. selection and vote: exact integer work
TOPK_ROWS = (1, 2, 3, 5, 130)
TOPK_N = (1, 5, 63, 64, 65, 200, 6100)
TOPK_K = (1, 2, 5, 63, 64)


def _topk_equal(ops, dm, k, dev, label):
    val, idx = ops.topk_smallest(_t(dm, dev), k)
    ref_val, ref_idx = oknn.topk_smallest(dm, k)
    assert idx.dtype == torch.int32 and idx.shape == (dm.shape[0], k) and val.shape == (dm.shape[0], k)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx, err_msg=label)
    np.testing.assert_array_equal(val.cpu().numpy(), ref_val, err_msg=label)


@pytest.mark.parametrize("n", TOPK_N)
@pytest.mark.parametrize("rows", TOPK_ROWS)
def test_topk_smallest_ties_exact(dev, rows, n):
    """Integer-valued matrices with values 0..7, built on the host: every round of the selection meets ties, so the
    rule 'ties to the smaller column' and the taken-column bookkeeping decide every index.  k up to 64 and k = n,
    n below, at and off the wave width, rows off the 4 rows of a workgroup.  idx and val equal a stable argsort's."""
    from embeddingnet_amd import ops
    dm = R.tied_matrix(71 + rows + n, rows, n)
    for k in TOPK_K:
        if k <= n:
            _topk_equal(ops, dm, k, dev, f"rows={rows} n={n} k={k}")


@pytest.mark.parametrize("n", (5, 63, 64, 65, 200, 642, 6100))
def test_topk_smallest_special_rows(dev, n):
    """A constant row, a row whose minimum sits in the last column, rows holding +inf (one or two finite entries, or
    none: fewer than k finite entries for every k > 2), a descending row, and a row whose n % 64 last columns are
    chosen from round 30 on, among tied rows; 9 rows, so the last workgroup is ragged.

    The last two are the regression test of a selection bug this file found: the column loop ran per lane
    (c = lane; c < n; c += 64), so in its last trip only the lanes below n % 64 were left, and the shuffle that asks
    lane j for the column taken in round j got nothing from a lane that had left: a column past the last multiple of 64
    taken in a round >= n % 64 was chosen again in every later round (n = 65: index 64 repeated to the end of the row).
    It showed wherever k > n % 64 and such a column was among the k nearest."""
    from embeddingnet_amd import ops
    dm = R.tied_matrix(72 + n, 9, n) + 1
    dm[0] = 3.0
    dm[1, -1] = 0.0
    dm[2, ::3] = np.inf
    dm[3] = np.inf
    dm[3, n // 2] = 2.0
    dm[4] = np.inf
    dm[4, -1] = 5.0
    dm[4, 0] = 5.0
    dm[5] = np.inf
    dm[6] = np.arange(n)[::-1]
    tail = n % 64 if n > 64 and n % 64 else min(n, 8)
    dm[7] = 1000.0
    dm[7, :30] = np.arange(30)[:n]
    dm[7, n - tail:] = 50 + np.arange(tail)[::-1]
    for k in TOPK_K:
        if k <= n:
            _topk_equal(ops, dm, k, dev, f"special n={n} k={k}")


def test_topk_smallest_refuses_bad_k(dev):
    """k = 0, k > 64 and k > n are refused by the library before anything is launched."""
    from embeddingnet_amd import ops
    from embeddingnet_amd._lib import EmbnetError
    for n, k in [(200, 65), (5, 6), (64, 65), (200, 0), (1, 2)]:
        with pytest.raises(EmbnetError):
            ops.topk_smallest(_t(R.tied_matrix(73, 3, n), dev), k)


def test_topk_smallest_nan_is_plus_inf(dev):
    """The defined behaviour for NaN (kernel comment, ops.topk_smallest): it counts as +inf.  Before, no column of a row
    with fewer than k non-NaN entries compared smaller than the initial best, and 0x7fffffff came out as a neighbour index.
    Asserted through ops.topk_smallest alone: indices in [0, n), distinct per row, NaN columns after all finite ones,
    and the whole result equal to the oracle's rule (NaN ties with +inf by column, reported as +inf)."""
    from embeddingnet_amd import ops
    for n in (5, 64, 65, 200):
        dm = R.tied_matrix(74 + n, 6, n)
        dm[0, 0] = np.nan                                          # one NaN, in the first column
        dm[1, ::2] = np.nan                                        # half the row
        dm[2] = np.nan                                             # the whole row
        dm[3] = np.nan
        dm[3, -1] = 1.0                                            # one finite entry, last column
        dm[4, 1::4] = np.nan
        dm[4, 2::4] = np.inf                                       # NaN and +inf interleaved
        for k in (1, 2, 5, 63, 64, n):
            if k > min(n, 64):
                continue
            val, idx = ops.topk_smallest(_t(dm, dev), k)
            val, idx = val.cpu().numpy(), idx.cpu().numpy()
            assert idx.min() >= 0 and idx.max() < n, (n, k, idx.min(), idx.max())
            for r in range(dm.shape[0]):
                assert len(set(idx[r])) == k, (n, k, r, idx[r])
                picked = dm[r, idx[r]]
                nans = np.flatnonzero(np.isnan(picked))
                if nans.size:                                       # a NaN is taken only once every finite entry is
                    assert not np.isfinite(picked[nans[0]:]).any(), (n, k, r)
                    assert np.isfinite(picked).sum() == np.isfinite(dm[r]).sum(), (n, k, r)
            ref_val, ref_idx = oknn.topk_smallest(dm, k)
            np.testing.assert_array_equal(idx, ref_idx)
            np.testing.assert_array_equal(val, ref_val)


def test_predict_with_nan_query_returns_a_gallery_class(dev):
    """With the NaN rule in place, whatever the distance kernel makes of a query holding a NaN (NaN, or 0 through its
    fmaxf(..., 0)), the selection returns k rows of the gallery, and predict answers with one of the gallery's classes
    instead of reading labels out of range.  Run once, on the fixed selection only."""
    from embeddingnet_amd.knn import KNNClassifier
    x, y, q, _ = R.knn_data(10, 20, 64, 0.35, 2, 41)
    q[1, 7] = np.nan
    clf = KNNClassifier(n_neighbors=5, device=dev).fit(x, list(y))
    pred = clf.predict(q)
    assert pred.shape == (2,) and pred[0] in clf.classes_ and pred[1] in clf.classes_


def _vote_equal(ops, idx, labels, dev, label):
    pred = ops.knn_vote(_t(idx, dev, torch.int32), _t(labels, dev, torch.int32))
    assert pred.dtype == torch.int32
    np.testing.assert_array_equal(pred.cpu().numpy(), oknn.vote(labels[idx]), err_msg=label)


@pytest.mark.parametrize("rows", (1, 255, 256, 257))
def test_knn_vote_ties_exact(dev, rows):
    """knn_vote on hand-built neighbour lists: label ids up to 999 over a gallery of 3 000, k from 1 to 64 (random lists:
    at k = 2 nearly every row is a 1-1 tie, at k = 10 most are ties between pairs), then constructed 2-2-1, 1-1-1-1-1 and
    32-32 ties with the larger label met first.  Rows around the 256 threads of a workgroup.  Equal to bincount.argmax."""
    from embeddingnet_amd import ops
    rs = np.random.RandomState(75 + rows)
    labels = rs.permutation(np.concatenate([np.arange(1000), rs.randint(0, 1000, size=2000)]))    # every id is held
    for k in (1, 2, 5, 10, 64):
        _vote_equal(ops, rs.randint(0, 3000, size=(rows, k)), labels, dev, f"random rows={rows} k={k}")
        few = rs.randint(0, 3000, size=(rows, 1 + k // 4))          # few distinct neighbours: large tied counts
        _vote_equal(ops, np.take_along_axis(few, rs.randint(0, few.shape[1], size=(rows, k)), 1), labels, dev,
                    f"repeats rows={rows} k={k}")
    by_label = [np.flatnonzero(labels == c) for c in range(1000)]
    assert all(len(m) for m in by_label)

    def rows_of(pattern):
        """pattern: counts per distinct label; labels drawn per row, listed in DESCENDING label order, shuffled or not"""
        out = np.empty((rows, sum(pattern)), np.int64)
        for r in range(rows):
            cls = np.sort(rs.choice(1000, len(pattern), replace=False))[::-1]
            row = np.concatenate([rs.choice(by_label[c], cnt) for c, cnt in zip(cls, pattern)])
            out[r] = row if r % 2 == 0 else rs.permutation(row)
        return out
    for pattern in [(2, 2, 1), (1, 2, 2), (1, 1, 1, 1, 1), (32, 32), (5, 5), (3, 3, 3, 1)]:
        idx = rows_of(pattern)
        _vote_equal(ops, idx, labels, dev, f"pattern {pattern} rows={rows}")
        top = max(pattern)
        want = np.array([min(c for c in set(v) if list(v).count(c) == top) for v in labels[idx]])   # the rule, restated
        np.testing.assert_array_equal(oknn.vote(labels[idx]), want)


# ---------------------------------------------------------------- 3. the classifier end to end, at gallery size
def _host_vote(y_idx, neighbours):
    return oknn.vote(y_idx[neighbours])


@pytest.mark.parametrize("names", ("int", "str"))
@pytest.mark.parametrize("case", R.EVAL_KNN_CASES, ids=lambda c: c[0])
def test_knn_classifier_at_gallery_size(dev, case, names):
    """KNNClassifier on 1000 queries x 6100 gallery rows x 256 (305 classes; the distance kernel's large tiles), separable
    (sigma 0.3) and overlapping (sigma 1.2: float64 top-1 0.63, k = 5 vote 0.71 - 0.74, so the vote decides), with int
    and string class names.

    fp32 distances may swap neighbours that float64 holds nearly tied, so neighbour identity gets an excuse with a cap:
      * a position where idx_gpu != idx_ref is accepted only if the float64 squared distances of the two gallery rows to
        that query differ by at most 2 B = 4 A(E) = 8e-6 (both off by B = 2 A(E), unit rows; _check_cross); every
        row's indices are distinct and its distances ascending in any case;
      * at most 2 % of positions may use it.  One float64 gap below 4 A(E) can displace two positions, so the test first
        asserts ON THE REFERENCE ALONE that such gaps among the first k + 1 neighbours are at most 1 % of positions
        (0.0 % - 0.49 % for these recipes), and only then looks at the GPU's answer;
      * predictions get no excuse: predict(q) equals the host's majority vote (ties to the smallest class) over the
        labels of the GPU's own kneighbors(q, k); agreement with the float64 oracle's predictions is then at least
        1 - (share of rows holding an excused position), which is asserted too."""
    from embeddingnet_amd.knn import KNNClassifier
    _, sigma, seed = case
    e = 256
    x, y, q, _ = R.knn_data(305, 20, e, sigma, 1000, seed)
    nq = q.shape[0]
    if names == "str":                                            # sorted order differs from the order of the ids
        class_names = np.array([f"{(c * 7919) % 1000:03d}-sign" for c in range(305)])
        assert len(set(class_names)) == 305
        labels = list(class_names[y])
    else:
        labels = [int(c) for c in y]
    classes, y_idx = np.unique(np.array(labels), return_inverse=True)
    d2, qn, xn = oknn.cross_sqdist64(q, x)
    order = np.argsort(d2, axis=1, kind="stable")[:, :11]
    gaps = np.diff(np.take_along_axis(d2, order, 1), axis=1)
    tie = 4 * _A(e)
    rows = np.arange(nq)[:, None]
    for k in (1, 5, 10):
        near = float((gaps[:, :k] < tie).mean())
        assert near <= 0.01, f"the recipe's float64 near-tie share {near} would turn the 2 % cap into a loophole"
        clf = KNNClassifier(n_neighbors=k, device=dev).fit(x, labels)
        assert np.array_equal(clf.classes_, classes)
        dist, idx = clf.kneighbors(q)
        assert dist.shape == (nq, k) and idx.shape == (nq, k) and idx.min() >= 0 and idx.max() < x.shape[0]
        assert np.all(np.diff(dist, axis=1) >= 0) and all(len(set(r)) == k for r in idx)
        ref_idx = order[:, :k]
        differs = idx != ref_idx
        excess = np.abs(d2[rows, idx] - d2[rows, ref_idx])
        assert np.all(excess[differs] <= tie), f"k={k}: a neighbour {excess[differs].max()} farther than the reference's"
        assert np.all(np.abs(dist.astype(np.float64) ** 2 - d2[rows, idx]) <= _A(e) * (qn[:, None] + xn[idx]))      # B
        used = float(differs.mean())
        print(f"knn {case[0]} {names} k={k}: float64 near-tie share {near:.4f}, excused positions {used:.4f}")
        assert used <= 0.02, f"k={k}: {used} of the positions differ from the float64 neighbours"
        pred = clf.predict(q)
        assert pred.shape == (nq,)
        np.testing.assert_array_equal(pred, classes[_host_vote(y_idx, idx)])
        agree = float(np.mean(pred == classes[_host_vote(y_idx, ref_idx)]))
        assert agree >= 1 - float(differs.any(axis=1).mean()), (k, agree)
    # one query shaped (E,), as predict_knn passes it
    dist1, idx1 = clf.kneighbors(q[3])
    assert dist1.shape == (1, 10) and idx1.shape == (1, 10) and len(set(idx1[0])) == 10 and np.all(np.diff(dist1[0]) >= 0)
    assert np.all(np.abs(dist1[0].astype(np.float64) ** 2 - d2[3, idx1[0]]) <= _A(e) * (qn[3] + xn[idx1[0]]))
    assert np.all(np.abs(d2[3, idx1[0]] - d2[3, order[3, :10]]) <= tie)
    one = clf.predict(q[3])
    assert one.shape == (1,) and one[0] == classes[_host_vote(y_idx, idx1)[0]]


def test_kneighbors_refuses_k_above_gallery(dev):
    from embeddingnet_amd._lib import EmbnetError
    from embeddingnet_amd.knn import KNNClassifier
    x, y, q, _ = R.knn_data(3, 1, 64, 0.3, 4, 76)
    clf = KNNClassifier(n_neighbors=1, device=dev).fit(x, list(y))
    with pytest.raises(EmbnetError) as err:
        clf.kneighbors(q, n_neighbors=5)
    assert "k=5" in str(err.value) and "n=3" in str(err.value)
    assert clf.kneighbors(q, n_neighbors=3)[1].shape == (4, 3)


# ---------------------------------------------------------------- 4. softmax cross-entropy and L2 normalisation
XENT_SHAPES = [(1, 3), (5, 3), (33, 107), (300, 5000), (257, 1000), (7, 64), (7, 65)]
U = 2.0 ** -24


def _xent_check(dev, z, t, label):
    """ops.softmax_cross_entropy (mean loss, accuracy, probabilities, dlogits through (loss * 2).backward()) and the row
    losses of embnet_softmax_xent_fwd against the float64 oracle.

    Yardstick: the same formula in plain float32 on the host (torch.log_softmax).  Its row-loss error on these inputs
    is about 2^-24 * max|z| (0.2 - 1.4 of that), its probabilities are within 2e-7.  The kernel sums in another order
    and uses the hardware exp / log, so it gets a factor 4 over max(yardstick's error on the same input, 2^-24 * max|z|)
    for the row losses and their mean, and over max(yardstick's error, 2^-24) for the probabilities and for dlogits * b:
    4 covers reordering, not a systematically worse function, and the floor keeps a lucky yardstick from making the
    test flaky.  Accuracy is compared exactly (argmax = first maximum on both sides).

    Measured on an MI355X, in floors (kernel / yardstick on the same input), worst over s in {3, 30, 100} and over
    one-hot and soft targets:
        (b, c)        row losses    mean        probabilities   dlogits * b
        (1, 3)        0.78 / 0.78   0.78/0.78   0.65 / 1.35     1.30 / 2.70
        (5, 3)        0.84 / 0.84   0.17/0.17   1.04 / 0.99     2.48 / 2.48
        (33, 107)     1.74 / 2.08   1.19/0.93   1.71 / 2.76     4.87 / 5.58
        (300, 5000)   1.88 / 1.88   0.94/0.63   3.73 / 9.58     7.63 / 19.35
        (257, 1000)   1.71 / 1.96   0.67/1.43   4.26 / 5.00     9.33 / 10.22
        (7, 64)       1.56 / 1.56   1.08/2.01   1.92 / 1.21     5.23 / 5.23
        (7, 65)       2.50 / 2.50   0.86/0.86   1.62 / 1.62     6.24 / 6.24
    so the kernel, with the hardware exp / log, is as good as the yardstick and __expf / __logf stay.  It was not before
    this test: it formed lse = max + log(sum) first and took z - lse, which costs every log-probability half an ulp of
    the maximum logit; the probabilities were off by 40 - 65 floors at s = 30 and 49 - 255 floors (1.5e-5) at s = 100,
    dlogits * b by twice that, where the yardstick stays below 10.  The kernel now takes (z - max) - log(sum)."""
    from embeddingnet_amd import _lib, ops
    b, c = z.shape
    rl, ra, rp, rg = olosses.softmax_cross_entropy_rows(z, t)
    zy = torch.tensor(z, requires_grad=True)
    ty = torch.tensor(t)
    logp = torch.log_softmax(zy, 1)
    yl = -(ty * logp).sum(1)
    (yl.mean() * 2).backward()
    zmax = float(np.abs(z).max())
    floor_l = U * zmax
    y_rows = float(np.abs(yl.detach().numpy().astype(np.float64) - rl).max())
    y_mean = abs(float(yl.mean().item()) - rl.mean())
    y_prob = float(np.abs(logp.detach().exp().numpy().astype(np.float64) - rp).max())
    y_grad = float(np.abs(zy.grad.numpy().astype(np.float64) * b - 2 * rg * b).max())

    zt = _t(z, dev).requires_grad_(True)
    tt = _t(t, dev)
    loss, acc, prob = ops.softmax_cross_entropy(zt, tt)
    (loss * 2).backward()
    p2, rows, corr = torch.empty_like(tt), torch.empty(b, device=dev), torch.empty(b, device=dev)
    mean, acc2 = torch.empty((), device=dev), torch.empty((), device=dev)
    _lib.check(_lib.lib().embnet_softmax_xent_fwd(_lib.ptr(zt.detach()), _lib.ptr(tt), b, c, _lib.ptr(p2), _lib.ptr(rows),
                                                  _lib.ptr(corr), _lib.ptr(mean), _lib.ptr(acc2), _lib.stream()))
    rows, corr, prob, grad = rows.cpu().numpy(), corr.cpu().numpy(), prob.detach().cpu().numpy(), zt.grad.cpu().numpy()
    k_rows = float(np.abs(rows.astype(np.float64) - rl).max())
    k_mean = abs(float(loss.item()) - rl.mean())
    k_prob = float(np.abs(prob.astype(np.float64) - rp).max())
    k_grad = float(np.abs(grad.astype(np.float64) * b - 2 * rg * b).max())
    print(f"xent {label} b={b} c={c} max|z|={zmax:.1f}: rows {k_rows / floor_l:.2f}/{y_rows / floor_l:.2f}  "
          f"mean {k_mean / floor_l:.2f}/{y_mean / floor_l:.2f}  prob {k_prob / U:.2f}/{y_prob / U:.2f}  "
          f"dlogits*b {k_grad / U:.2f}/{y_grad / U:.2f}  (kernel/yardstick, in floors)")
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(prob)) and np.all(np.isfinite(grad))
    np.testing.assert_allclose(rows, rl, rtol=0, atol=4 * max(y_rows, floor_l), err_msg=f"{label}: row losses")
    np.testing.assert_allclose(loss.item(), rl.mean(), rtol=0, atol=4 * max(y_mean, floor_l), err_msg=f"{label}: mean")
    assert mean.item() == loss.item() and torch.equal(p2.cpu(), torch.from_numpy(prob))
    np.testing.assert_allclose(prob, rp, rtol=0, atol=4 * max(y_prob, U), err_msg=f"{label}: probabilities")
    np.testing.assert_allclose(grad * np.float64(b), 2 * rg * b, rtol=0, atol=4 * max(y_grad, U),
                               err_msg=f"{label}: dlogits * b")
    np.testing.assert_array_equal(corr, (z.argmax(1) == t.argmax(1)).astype(np.float32), err_msg=f"{label}: correct")
    assert acc.item() == np.float32(corr.sum()) / np.float32(b) == np.float32(ra) and acc2.item() == acc.item(), label
    return rows


@pytest.mark.parametrize("s", (3, 30, 100))
@pytest.mark.parametrize("shape", XENT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_softmax_cross_entropy_vs_float64(dev, shape, s):
    """Logit spreads of a confident classifier (s * randn, s up to 100), up to 5000 classes, b = 1 and b > 256 (the
    single-workgroup mean walks more than one element per thread), c at and off the wave width; one-hot targets.
    Bound and yardstick: _xent_check."""
    b, c = shape
    rs = np.random.RandomState(81 + b + c + s)
    z = (s * rs.randn(b, c)).astype(np.float32)
    t = np.eye(c, dtype=np.float32)[rs.randint(0, c, b)]
    _xent_check(dev, z, t, f"one-hot s={s}")


@pytest.mark.parametrize("s", (3, 30, 100))
@pytest.mark.parametrize("total", (1.0, 0.9))
@pytest.mark.parametrize("shape", [(33, 107), (257, 1000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_softmax_cross_entropy_soft_targets(dev, shape, total, s):
    """Soft targets: rows summing to 1 (label smoothing, mixup) and to 0.9 (dlogits = prob * sum t - t keeps the sum)."""
    b, c = shape
    rs = np.random.RandomState(82 + b + s)
    z = (s * rs.randn(b, c)).astype(np.float32)
    t = rs.rand(b, c) ** 8                                          # a few large entries per row
    t = (total * t / t.sum(1, keepdims=True)).astype(np.float32)
    _xent_check(dev, z, t, f"soft sum={total} s={s}")


def test_softmax_cross_entropy_tied_maximum(dev):
    """Rows whose maximum logit is held by two or three classes (in the same lane of the row's wave: columns 64 apart; in
    different lanes; the last column), and targets tied the same way: accuracy follows argmax = the first maximum."""
    b, c = 12, 200
    rs = np.random.RandomState(83)
    z = (3 * rs.randn(b, c)).astype(np.float32)
    t = np.eye(c, dtype=np.float32)[rs.randint(0, c, b)]
    ties = [(5, 69), (69, 133, 197), (0, 199), (198, 199), (7, 8), (130, 2), (64, 0), (63, 64), (3, 67), (10, 20, 30),
            (199, 100), (1, 65, 129)]
    for r, cols in enumerate(ties):
        z[r, list(cols)] = 20.0
        t[r] = 0
        t[r, min(cols) if r % 3 else max(cols)] = 1.0                # right on two rows of three, wrong on the third
    t[9] = 0
    t[9, [10, 30]] = 0.5                                            # a tied target maximum: its first column counts
    t[11] = 0
    t[11, [65, 129]] = 0.5                                          # first target maximum 65 != first logit maximum 1
    want = np.array([max(cols) != min(cols) and r % 3 != 0 for r, cols in enumerate(ties)], np.float32)
    want[9], want[11] = 1.0, 0.0
    assert np.array_equal((z.argmax(1) == t.argmax(1)).astype(np.float32), want) and 0 < want.sum() < b
    _xent_check(dev, z, t, "tied maximum")


def test_softmax_cross_entropy_vanishing_target_probability(dev):
    """A row whose target class has probability below 1e-30 (e^-150: not representable in float32): the loss is about
    150 and finite, because it is taken from the log-softmax and never from log(prob)."""
    b, c = 5, 107
    rs = np.random.RandomState(84)
    z = rs.randn(b, c).astype(np.float32)
    t = np.eye(c, dtype=np.float32)[[3, 50, 106, 0, 64]]
    z[0, 3], z[0, 70] = -75.0, 75.0
    z[2, 106], z[2, 0] = -60.0, 95.0
    rows = _xent_check(dev, z, t, "vanishing target")
    assert 149 < rows[0] < 151 and 154 < rows[2] < 156 and np.all(np.isfinite(rows))
    assert olosses.softmax_cross_entropy_rows(z, t)[2][0, 3] < 1e-30


L2_SHAPES = [(1, 1), (5, 3), (37, 300), (130, 4096), (3, 64)]
L2_KINDS = ("ordinary", "zero", "below", "above", "large")


def _l2_row(rs, e, kind):
    v = rs.randn(e)
    v[np.abs(v) < 0.1] = 0.5                                        # (1, 1): keep the only element away from 0
    if kind == "zero":
        return np.zeros(e)
    if kind == "below":                                             # sum x^2 = 1e-13: >= 4 below 1e-12
        return v * (1e-13 / (v * v).sum()) ** 0.5
    if kind == "above":                                             # sum x^2 = 1e-11: >= 4 above
        return v * (1e-11 / (v * v).sum()) ** 0.5
    if kind == "large":
        return v * 1e4
    return v


def _l2_check(dev, x, label):
    """Forward and backward of ops.l2_normalize against float64 autograd of x * rsqrt(clamp(sum x^2, min=1e-12)), the
    clamped rows included (expected gradient dy * 1e6), at the tolerances of test_l2_normalize_and_pair_distance:
    rtol 1e-5 / atol 1e-7 forward, rtol 2e-4 / atol 2e-5 backward, the absolute part of the latter scaled by the row's
    1 / |x| (as clamped: rsqrt(max(sum x^2, 1e-12))) where that exceeds 1, since dx is dy scaled by it."""
    from embeddingnet_amd import ops
    n, e = x.shape
    rs = np.random.RandomState(85 + n)
    w = rs.randn(n, e)
    yr, gr = olosses.l2_normalize(x, w)
    ss = (x.astype(np.float64) ** 2).sum(1)
    assert not np.any((ss > 2.5e-13) & (ss < 4e-12)), "a row too close to the clamp: float32 may take the other branch"
    xt = _t(x, dev).requires_grad_(True)
    y = ops.l2_normalize(xt)
    (y * _t(w, dev)).sum().backward()
    y, g = y.detach().cpu().numpy(), xt.grad.cpu().numpy()
    w32 = w.astype(np.float32).astype(np.float64)
    scale = np.maximum(1.0, 1.0 / np.sqrt(np.maximum(ss, 1e-12)))[:, None]
    for r in range(n):
        np.testing.assert_allclose(y[r], yr[r], rtol=1e-5, atol=1e-7, err_msg=f"{label}: forward row {r}")
        np.testing.assert_allclose(g[r], gr[r], rtol=2e-4, atol=2e-5 * scale[r, 0], err_msg=f"{label}: backward row {r}")
        if ss[r] < 1e-12:                                          # stated outright: a plain scale by 1e6
            np.testing.assert_allclose(g[r], w32[r] * 1e6, rtol=2e-4, atol=0, err_msg=f"{label}: clamped row {r}")
            np.testing.assert_allclose(y[r], x[r].astype(np.float64) * 1e6, rtol=1e-5, atol=0)


@pytest.mark.parametrize("shape", L2_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_l2_normalize_vs_float64_with_clamped_rows(dev, shape):
    """Rows of ordinary size, an all-zero row, rows with sum x^2 a factor >= 4 below and above the 1e-12 clamp (float32
    and float64 take the same branch) and a row of amplitude 1e4, in one matrix where it has 5 rows or more, one kind
    per row position otherwise.  E from 1 to 4096 (64 elements per lane), n off the 4 rows of a workgroup."""
    n, e = shape
    rs = np.random.RandomState(86 + n + e)
    if n >= len(L2_KINDS):
        x = np.stack([_l2_row(rs, e, L2_KINDS[r % len(L2_KINDS)] if r < 2 * len(L2_KINDS) else "ordinary")
                      for r in range(n)]).astype(np.float32)
        _l2_check(dev, x, f"{n}x{e}")
        return
    for first in range(len(L2_KINDS)):
        x = np.stack([_l2_row(rs, e, L2_KINDS[(first + r) % len(L2_KINDS)]) for r in range(n)]).astype(np.float32)
        _l2_check(dev, x, f"{n}x{e} from {L2_KINDS[first]}")


# ---------------------------------------------------------------- 5. pairwise distances: large tiles, ragged edges
@pytest.mark.parametrize("n", (2500, 2502))
def test_pairwise_large_tiles_ragged(dev, n):
    """20 x 20 = 400 tiles of 128x128 with a ragged last row and column of tiles: N = 2500 takes the float4 store path
    (N % 4 == 0), N = 2502 the scalar one.  Unit non-negative rows, E = 64, squared output against the float64 oracle at
    test_pairwise_golden's bound (2e-6 for E <= 512), plus exact symmetry and an exactly zero diagonal."""
    from embeddingnet_amd import ops
    x = R.unit_nonneg_rows(np.random.RandomState(87 + n), n, 64)
    d2 = ops.pairwise_distances(_t(x, dev), squared=True)
    assert torch.equal(d2, d2.t()) and torch.all(torch.diagonal(d2) == 0) and torch.all(d2 >= 0)
    np.testing.assert_allclose(d2.cpu().numpy(), opair.pairwise_sqdist(x), rtol=0, atol=2e-6)
