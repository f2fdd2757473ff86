"""CPU: the float64 restatement of the k-nearest-neighbour search contract and its interval checker (tests/knn_search_ref.py),
which the GPU tests (tests/test_knn_search_gpu.py) compare the kernel with."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_search_ref as KR  # noqa: E402
import retrieval_ref as RR  # noqa: E402


def _by_sorted_keys(d2_f32, k, ok):
    """The contract said the kernel's way: a stable sort of the eligible columns' 64-bit keys."""
    b, n = d2_f32.shape
    idx, val, found = np.full((b, k), -1, np.int32), np.full((b, k), np.inf, np.float32), np.zeros(b, np.int32)
    for r in range(b):
        cols = np.flatnonzero(ok[r])
        keys = KR.keys_u64(d2_f32[r, cols], cols)
        keys = keys[np.argsort(keys, kind="stable")][:k]
        f = len(keys)
        found[r] = f
        idx[r, :f] = (keys & np.uint64(0xffffffff)).astype(np.int32)
        val[r, :f] = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, val, found


@pytest.mark.parametrize("kind", ["random", "tied"])
@pytest.mark.parametrize("select,loo", [(0, False), (0, True), (1, True), (2, True), (1, False), (2, False)])
@pytest.mark.parametrize("k", [1, 5, 40])
def test_restatement_is_a_stable_sort_of_the_keys(kind, select, loo, k):
    n = 33
    x = KR.unit_rows(n, 8, 1) if kind == "random" else KR.integer_rows(n, 2, 1)
    q = x if loo else (KR.unit_rows(9, 8, 2) if kind == "random" else KR.integer_rows(9, 2, 2))
    xl = KR.unbalanced_labels(n, 3)
    ql = xl if loo else KR.unbalanced_labels(len(q), 4)
    d2 = RR.sqdist64(q, x).astype(np.float32)
    if kind == "random":
        d2[0, 5] = np.nan                                   # counts as +inf, keeps its index
    if kind == "tied":
        assert len(np.unique(d2)) < d2.size // 4            # masses of ties
    got = KR.knn_exact(d2, k, ql, xl, loo, select)
    ok = KR.eligible_mask(np.arange(len(q)), n, ql, xl, loo, select)
    want = _by_sorted_keys(np.where(np.isnan(d2), np.float32(np.inf), d2), k, ok)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    if select == 1 and loo:
        single = int(np.flatnonzero(xl == 0)[0])            # the class of one: nothing eligible, a fully padded row
        assert got[2][single] == 0 and np.all(got[0][single] == -1) and np.all(np.isinf(got[1][single]))
    if k > n:
        assert np.all(got[2] <= n) and np.all(got[0][:, n:] == -1)


def _float_case(e=24):
    q, x = KR.unit_rows(20, e, 5), KR.unit_rows(150, e, 6)
    return q, x, KR.unbalanced_labels(20, 7), KR.unbalanced_labels(150, 8)


def _f32_answer(q, x, k, ql, xl, loo, select):
    """What a float32 implementation of d2 = rn + cn - 2 q.x gives."""
    q, x = np.asarray(q, np.float32), np.asarray(x, np.float32)
    d2 = np.maximum((q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - np.float32(2) * (q @ x.T), np.float32(0))
    assert d2.dtype == np.float32
    return KR.knn_exact(d2, k, ql, xl, loo, select)


@pytest.mark.parametrize("select", [0, 1, 2])
@pytest.mark.parametrize("k", [3, 160])
def test_checker_accepts_the_float64_and_a_float32_answer(select, k):
    q, x, ql, xl = _float_case()
    idx, val, found = KR.knn_ref(q, x, k, ql, xl, False, select)
    assert KR.check(q, x, k, idx, val, found, ql, xl, False, select) == []
    idx, val, found = _f32_answer(q, x, k, ql, xl, False, select)
    assert KR.check(q, x, k, idx, val, found, ql, xl, False, select) == []
    idx, val, found = _f32_answer(x, x, k, xl, xl, True, select)
    assert KR.check(x, x, k, idx, val, found, xl, xl, True, select) == []


def test_checker_accepts_either_order_inside_the_bound_only():
    """Two columns closer than 2 B may come back in either order; two that are farther apart may not."""
    q = np.array([[1.0, 0.0]], np.float32)
    x = np.array([[0.0, 1.0], [1e-7, 1.0], [0.0, -1.0], [-1.0, 0.0]], np.float32)
    idx, val, found = KR.knn_ref(q, x, 2)
    assert KR.check(q, x, 2, idx, val, found) == []
    swapped = idx[:, ::-1].copy()
    assert idx[0].tolist() == [1, 0] and KR.check(q, x, 2, swapped, np.sort(val[:, ::-1].copy()), found) == []
    far = np.array([[1, 3]], np.int32)
    assert any("unreturned" in m for m in KR.check(q, x, 2, far, np.array([[val[0, 0], 4.0]]), found))


def test_checker_rejects_the_mutations():
    q, x, ql, xl = _float_case()
    k = 6
    idx, val, found = KR.knn_ref(q, x, k)
    d2 = RR.sqdist64(q, x)
    # one neighbour swapped for a clearly farther one (kept in order, with its own correct distance)
    i2, v2 = idx.copy(), val.copy()
    far = int(d2[3].argmax())
    i2[3, -1], v2[3, -1] = far, d2[3, far]
    assert any(m.startswith("row 3:") and "unreturned" in m for m in KR.check(q, x, k, i2, v2, found))
    # a wrong found
    f2 = found.copy(); f2[4] -= 1
    assert any(m.startswith("row 4: found") for m in KR.check(q, x, k, idx, val, f2))
    # an excluded column returned: leave-one-out, the query itself in front
    li, lv, lf = KR.knn_ref(x, x, k, self_exclude=True)
    assert KR.check(x, x, k, li, lv, lf, self_exclude=True) == []
    i3, v3 = li.copy(), lv.copy()
    i3[7, 1:], v3[7, 1:] = li[7, :-1], lv[7, :-1]
    i3[7, 0], v3[7, 0] = 7, 0.0
    assert any(m.startswith("row 7: ineligible") for m in KR.check(x, x, k, i3, v3, lf, self_exclude=True))
    # ... and a column of the wrong label under select
    si, sv, sf = KR.knn_ref(q, x, k, ql, xl, False, 2)
    assert KR.check(q, x, k, si, sv, sf, ql, xl, False, 2) == []
    same = np.flatnonzero(xl == ql[0])
    i4, v4 = si.copy(), sv.copy()
    i4[0, -1], v4[0, -1] = same[d2[0, same].argmax()], d2[0, same].max()
    assert any(m.startswith("row 0: ineligible") for m in KR.check(q, x, k, i4, np.sort(v4), sf, ql, xl, False, 2))
    # a d2 outside the bound
    v5 = val.copy(); v5[2, 0] += 1e-4
    assert any(m.startswith("row 2: d2 off") for m in KR.check(q, x, k, idx, v5, found))
    # a padded row that is not padded
    pi, pv, pf = KR.knn_ref(x, x, k, xl, xl, True, 1)
    single = int(np.flatnonzero(xl == 0)[0])
    assert pf[single] == 0
    i6 = pi.copy(); i6[single, 0] = 0
    assert any(m.startswith(f"row {single}: padding") for m in KR.check(x, x, k, i6, pv, pf, xl, xl, True, 1))


def test_checker_rejects_a_dropped_tie_rule():
    q, x = KR.integer_rows(6, 2, 11), KR.integer_rows(60, 2, 12)
    k = 10
    idx, val, found = KR.knn_ref(q, x, k)
    assert KR.check(q, x, k, idx, val, found) == []
    r, j = np.argwhere(np.diff(val, axis=1) == 0)[0]        # two equal distances side by side
    i2 = idx.copy()
    i2[r, j], i2[r, j + 1] = idx[r, j + 1], idx[r, j]
    assert any(m.startswith(f"row {r}: not ascending") for m in KR.check(q, x, k, i2, val, found))
