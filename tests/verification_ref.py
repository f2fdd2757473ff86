"""Float64 restatement of the verification contract (include/embnet.h, "verification"), NumPy and Python integers only.

Histograms: every (query, gallery) pair — ordered pairs, the query's own column skipped under leave-one-out, as the kernel counts
them — goes to bin clamp(floor((v - lo) / w), 0, bins - 1) of the same-class or the other-class histogram; NaN goes to the last
bin.  With float64 d2 from retrieval_ref.sqdist_blocks that is the exact answer wherever the fp32 d2 is exact (grid inputs).
Elsewhere the kernel's d2 differs from the float64 one by at most B = A(e) * (|q|^2 + |x|^2), so a pair within B of an edge may
sit on either side of it: `brackets` gives, per edge, the fewest and the most pairs that can lie below it.
Metrics: `brute_metrics` restates every metric from the two lists of pair values directly — counts by comparison against each
edge, AUC by comparing every same pair with every other pair — in exact rationals, independent of the histogram reduction of
embeddingnet_amd/verification.py.
"""
import functools
import math
from decimal import Decimal
from fractions import Fraction

import numpy as np

import retrieval_ref as RR


def A(e):
    """tests/test_eval_path_gpu.py::_A, verbatim: the project's bound on |d2_gpu - d2_f64| / (|q|^2 + |x|^2)."""
    return 2e-6 if e <= 512 else 4e-6 * (e / 512) ** 0.5


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def grid_rows(n, e, classes, seed):
    """Rows with entries k / 4, |k| <= 8 (e <= 128): every norm, product and partial sum is exact in fp32 in any order, so the
    kernel's d2 is exact.  -> (x float32 [n, e], labels int32 [n])."""
    assert e <= 128
    rs = np.random.RandomState(seed)
    return (rs.randint(-8, 9, size=(n, e)) / 4.0).astype(np.float32), rs.randint(0, classes, size=n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def clustered_unit_rows(n, e, classes=10, spread=0.35, seed=0):
    """Unit rows (normalised in float64, rounded to float32 once) scattered around `classes` unit centres.  Cached: the callers
    share one copy and leave it unchanged."""
    rs = np.random.RandomState(seed)
    centres = rs.randn(classes, e)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    labels = rs.randint(0, classes, size=n).astype(np.int32)
    x = centres[labels] + spread * rs.randn(n, e) / math.sqrt(e)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = x.astype(np.float32)
    x.setflags(write=False)
    labels.setflags(write=False)
    return x, labels


# ---- histograms ---------------------------------------------------------------------------------------------------------------
def bin_of(v, lo, w, bins):
    """The bin contract in float64 on float64 values: exact whenever v - lo and the product are (they are for fp32 inputs and
    power-of-two w)."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid='ignore'):
        t = np.floor((v - lo) / w)
        b = np.where(np.isnan(v), bins - 1, np.clip(np.nan_to_num(t, nan=0.0, posinf=bins - 1, neginf=0.0), 0, bins - 1))
    return b.astype(np.int64)


def bin_of_f32(v, lo, w, bins):
    """The same contract in float32 arithmetic, as the values kernel computes it: (v - lo) rounded to float32, times 1 / w."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        t = np.floor((v - np.float32(lo)) * np.float32(1.0 / w))
        b = np.where(np.isnan(v), bins - 1, np.clip(np.nan_to_num(t, nan=0.0, posinf=bins - 1, neginf=0.0), 0, bins - 1))
    return b.astype(np.int64)


def _pairs(q, ql, x, xl):
    """Yield (d2 [b, n] float64, same [b, n] bool, live [b, n] bool) over blocks of queries; x None: leave-one-out."""
    loo = x is None
    if loo:
        x, xl = q, ql
    ql, xl = np.asarray(ql), np.asarray(xl)
    for idx, d2 in RR.sqdist_blocks(q, x):
        live = np.ones(d2.shape, bool)
        if loo:
            live[np.arange(len(idx)), idx] = False
        yield idx, d2, ql[idx][:, None] == xl[None, :], live


def exact_histograms(q, ql, x, xl, bins, d2_max):
    """-> (hist_same, hist_other) int64 [bins] over the ordered pairs, from float64 d2."""
    hs, ho = np.zeros(bins, np.int64), np.zeros(bins, np.int64)
    for _, d2, same, live in _pairs(q, ql, x, xl):
        b = bin_of(d2, 0.0, d2_max / bins, bins)
        hs += np.bincount(b[same & live], minlength=bins)
        ho += np.bincount(b[~same & live], minlength=bins)
    return hs, ho


def brackets(q, ql, x, xl, bins, d2_max, a):
    """Per edge t_j = j * w, j = 0 .. bins, for same and other pairs separately: lo_j = #{d2 < t_j - B}, hi_j = #{d2 < t_j + B} with
    B = a * (|q|^2 + |x|^2) per pair, in float64.  The last edge closes the range: everything beyond it is clamped into the last
    bin, so lo = hi = the total there.  -> {'same': (lo, hi), 'other': (lo, hi), 'open_share': the share of pairs with an edge
    inside (d2 - B, d2 + B], 'n_same', 'n_other'}; finite inputs only."""
    w = d2_max / bins
    q64 = np.asarray(q, np.float64)
    x64 = q64 if x is None else np.asarray(x, np.float64)
    qn, xn = (q64 * q64).sum(1), (x64 * x64).sum(1)
    first = {k: np.zeros(bins + 2, np.int64) for k in ('same_lo', 'same_hi', 'other_lo', 'other_hi')}
    open_pairs = total = 0
    for idx, d2, same, live in _pairs(q, ql, x, xl):
        B = a * (qn[idx][:, None] + xn[None, :])
        # the first edge j that has the pair below it: d2 -+ B < j * w  <=>  j >= floor((d2 -+ B) / w) + 1
        j_hi = np.clip(np.floor((d2 - B) / w) + 1, 0, bins + 1).astype(np.int64)      # counted by hi_j from here on
        j_lo = np.clip(np.floor((d2 + B) / w) + 1, 0, bins + 1).astype(np.int64)      # counted by lo_j from here on
        for name, sel in (('same', same & live), ('other', ~same & live)):
            first[name + '_hi'] += np.bincount(j_hi[sel], minlength=bins + 2)
            first[name + '_lo'] += np.bincount(j_lo[sel], minlength=bins + 2)
        open_pairs += int(((j_hi != j_lo) & live).sum())
        total += int(live.sum())
    out = {'open_share': open_pairs / max(total, 1)}
    for name in ('same', 'other'):
        lo, hi = np.cumsum(first[name + '_lo'])[:bins + 1], np.cumsum(first[name + '_hi'])[:bins + 1]
        n = int(first[name + '_hi'].sum())
        lo[bins] = hi[bins] = n
        out[name] = (lo, hi)
        out['n_' + name] = n
    return out


def pair_lists(q, ql, x, xl):
    """-> (same_values, other_values): float64 d2 of every UNORDERED pair under leave-one-out (x None), of every (query, gallery)
    pair otherwise."""
    s, o = [], []
    for idx, d2, same, live in _pairs(q, ql, x, xl):
        if x is None:
            live = live & (np.arange(d2.shape[1])[None, :] > idx[:, None])
        s.append(d2[same & live])
        o.append(d2[~same & live])
    return np.concatenate(s), np.concatenate(o)


# ---- metrics from the pair lists ------------------------------------------------------------------------------------------------
def brute_metrics(same_values, other_values, lo, w, bins, fars=(), at=(), accept='below'):
    """Every metric of verification_from_histograms restated on the two lists of pair values.  A pair is accepted as same at
    edge j iff its bin is below j ('below'), or iff its bin is at least bins - j ('above': larger values mean same)."""
    sb = np.sort(bin_of(same_values, lo, w, bins))
    ob = np.sort(bin_of(other_values, lo, w, bins))
    if accept == 'above':
        sb, ob = np.sort(bins - 1 - sb), np.sort(bins - 1 - ob)
        edge = lambda j: lo + (bins - j) * w
        step = -w
    else:
        edge = lambda j: lo + j * w
        step = w
    S, O = len(sb), len(ob)
    TP = [int(np.searchsorted(sb, j, side='left')) for j in range(bins + 1)]       # bins below j
    FP = [int(np.searchsorted(ob, j, side='left')) for j in range(bins + 1)]
    out = {'n_same': S, 'n_other': O}
    if S == 0 or O == 0:
        return out
    tpr = [Fraction(t, S) for t in TP]
    fpr = [Fraction(f, O) for f in FP]
    above = O - np.searchsorted(ob, sb, side='right')                               # other pairs in a higher bin, per same pair
    equal = np.searchsorted(ob, sb, side='right') - np.searchsorted(ob, sb, side='left')
    out['auc'] = float(Fraction(2 * int(above.sum()) + int(equal.sum()), 2 * S * O))
    j = min(j for j in range(bins + 1) if fpr[j] >= 1 - tpr[j])
    assert j >= 1
    s = ((1 - tpr[j - 1]) - fpr[j - 1]) / ((fpr[j] - fpr[j - 1]) + (tpr[j] - tpr[j - 1]))
    out['eer'] = float(fpr[j - 1] + s * (fpr[j] - fpr[j - 1]))
    out['eer_threshold'] = edge(j - 1) + float(s) * step
    for f in fars:
        allowed = int((Decimal(repr(float(f))) * O).to_integral_value(rounding='ROUND_FLOOR'))
        j = max(j for j in range(bins + 1) if FP[j] <= allowed)
        out[f'tar@far={f!r}'] = float(tpr[j])
        out[f'threshold@far={f!r}'] = edge(j)
    acc = [Fraction(TP[j] + O - FP[j], S + O) for j in range(bins + 1)]
    most = max(acc)
    j = min(j for j in range(bins + 1) if acc[j] == most)
    out['best_accuracy'] = float(acc[j])
    out['best_threshold'] = edge(j)
    for T in at:
        T = float(T)
        j = min(range(bins + 1), key=lambda j: (abs((lo + j * w) - T), -j))            # the nearest edge, a tie to the upper one
        j = j if accept == 'below' else bins - j
        out[f'accuracy@{T!r}'] = float(acc[j])
        out[f'accuracy_threshold@{T!r}'] = edge(j)
    return out


def same_metrics(got, want, tol=1e-12):
    """Every key of `want` is in `got` with the same value (integers exactly, floats within tol)."""
    for k, v in want.items():
        assert k in got, k
        if isinstance(v, int):
            assert got[k] == v, (k, got[k], v)
        else:
            assert abs(got[k] - v) <= tol, (k, got[k], v)
