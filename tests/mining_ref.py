"""The triplet loss path restated in NumPy, vectorised over pairs: mining on a distance matrix (the three selection rules of
csrc/mining.hip with their counter RNG and rank-select, the fallback triplet), batch-hard with its non-finite rule, the gather-form
hinge with its mean and gradient (once in the kernels' float32 order, once in float64), and the inputs the tests run on.

The lattice: every embedding entry is a small integer times STEP = 1/8.  Every product, partial sum, squared norm, Gram entry,
d^2, hinge sum and gradient sum is then a multiple of 1/64 far below 2^24 units, i.e. exactly representable in float32 IN ANY
SUMMATION ORDER, so a kernel's result must equal this file's bit for bit (lattice_units_max checks the premise).  No device code.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from augment_ref import rng_u32  # noqa: E402

f32 = np.float32
STEP = 0.125
MODES = ("semihard", "hardest", "random_hard")
MODE_ID = {"semihard": 0, "hardest": 1, "random_hard": 2, "batch_hard": 3}          # include/embnet.h EMBNET_MINE_*
SPECIAL_COLUMNS = (0, 31, 32, 63, 64, 255, 256)                                     # + nneg - 1: ballot-block and trip edges


# ---- index helpers ---------------------------------------------------------------------------------------------------------------
def pair_index(p, k):
    """-> (i, j, lo) of every positive pair, class by class, combinations() order inside a class."""
    ii, jj = np.triu_indices(k, 1)
    lo = np.repeat(np.arange(p) * k, len(ii))
    return lo + np.tile(ii, p), lo + np.tile(jj, p), lo


def negative_columns(p, k):
    """[pairs, n-k]: the out-of-class columns of each pair, ascending."""
    _, _, lo = pair_index(p, k)
    q = np.arange(p * k - k)[None, :]
    return np.where(q < lo[:, None], q, q + k)


def loss_values(D, p, k, margin):
    """(D[i,j] - D[i,neg]) + float32(margin), two float32 roundings."""
    D = np.asarray(D, f32)
    i, j, _ = pair_index(p, k)
    cols = negative_columns(p, k)
    with np.errstate(invalid="ignore"):
        lv = (D[i, j][:, None] - D[i[:, None], cols]).astype(f32) + f32(margin)
    return lv.astype(f32)


def candidate_sets(lv, margin, mode):
    """bool [pairs, n-k].  NaN is never a candidate and never the arg-max; -inf never wins."""
    with np.errstate(invalid="ignore"):
        if mode == "random_hard":
            return lv > 0
        if mode == "semihard":
            return (lv > 0) & (lv < f32(margin))
        if mode != "hardest":
            raise KeyError(mode)
        v = np.where(lv > -np.inf, lv, -np.inf).astype(f32)                         # NaN -> -inf: neither compares
        best = np.argmax(v, axis=1)                                                 # first maximum
        out = np.zeros(lv.shape, bool)
        rows = np.arange(len(lv))
        out[rows, best] = v[rows, best] > 0
        return out


def ranked_pick(cand, want):
    """Column (in candidate order) of the want-th candidate of every row; -1 where the row has none."""
    cum = np.cumsum(cand, axis=1)
    hit = cand & (cum == (want[:, None] + 1))
    return np.where(cand.any(1), np.argmax(hit, axis=1), -1)


def mine(D, p, k, margin, mode, seed, lv=None, pick=None):
    """embnet_mine_triplets restated.  -> dict(selected [pairs] (row index or -1), candidates [pairs, n-k] bool, triplets [T,3],
    count, fallback, loss_values).  lv: loss_values(D, ...) computed before (it does not depend on mode or seed).
    pick: replaces ranked_pick (the tests' deliberately wrong variants)."""
    n = p * k
    lv = loss_values(D, p, k, margin) if lv is None else lv
    cand = candidate_sets(lv, margin, mode)
    total = cand.sum(1).astype(np.uint64)
    if mode == "hardest":
        want = np.zeros(len(cand), np.int64)
    else:
        u = rng_u32(seed, np.arange(len(cand), dtype=np.uint64), np.uint64(0)).astype(np.uint64)
        want = ((u * total) >> np.uint64(32)).astype(np.int64)
    q = (pick or ranked_pick)(cand, want)
    i, j, lo = pair_index(p, k)
    selected = np.where(q < 0, -1, np.where(q < lo, q, q + k)).astype(np.int32)
    act = selected >= 0
    trip = np.stack([i[act], j[act], selected[act]], axis=1).astype(np.int32)
    fallback = len(trip) == 0
    if fallback:
        trip = np.array([[n - 2, n - 1, 0]], np.int32)
    return dict(selected=selected, candidates=cand, triplets=trip, count=len(trip), fallback=fallback, loss_values=lv)


def pack_mask(cand):
    """candidates -> the uint32 words of embnet_mine_triplets' cand_mask: bit (q & 31) of word (q >> 5)."""
    pairs, nneg = cand.shape
    words = (nneg + 31) // 32
    bits = np.zeros((pairs, words * 32), np.uint64)
    bits[:, :nneg] = cand
    return (bits.reshape(pairs, words, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def batch_hard(D, p, k):
    """embnet_batch_hard restated: per anchor the farthest same-class and the closest other-class row under the kernels'
    comparisons (v > best from -inf, v < best from +inf: a NaN never compares), the first index on ties; where no column of a set
    compares, the set's first column.  -> [n, 3] int32."""
    D = np.asarray(D, f32)
    n = p * k
    a = np.arange(n)
    lo = (a // k) * k
    col = np.arange(n)[None, :]
    same = (col >= lo[:, None]) & (col < lo[:, None] + k)
    with np.errstate(invalid="ignore"):
        okp = same & (col != a[:, None]) & (D > -np.inf)
        okn = ~same & (D < np.inf)
    ip = np.where(okp.any(1), np.argmax(np.where(okp, D, -np.inf), axis=1), np.where(a == lo, lo + 1, lo))
    in_ = np.where(okn.any(1), np.argmin(np.where(okn, D, np.inf), axis=1), np.where(lo > 0, 0, lo + k))
    return np.stack([a, ip, in_], axis=1).astype(np.int32)


# ---- the gather-form hinge ---------------------------------------------------------------------------------------------------------
def gather_loss(emb, triplets, count, margin, upstream=None, dtype=f32, active=None):
    """embnet_triplet_gather_fwd / _bwd restated on the first `count` triplets.
    dtype float32: the kernels' order of roundings — b = (pos - neg) + margin, g = 2 * up / float32(count), demb = g * sum —
    exact on lattice inputs, where the sums themselves are exact in any order.  dtype float64: the same in float64.
    active: the flags the gradient uses instead of b >= 0 (a kernel's own, where b sits within rounding of the corner).
    -> dict(rows, active, mean, demb, sq [T] = pos + neg, mag [n, e] = |g| * sum of the absolute terms, matches [n], g, acc [n, e] = the
    unscaled gradient sums)."""
    x = np.asarray(emb, dtype)
    t = np.asarray(triplets)[:count]
    a, p, n = x[t[:, 0]], x[t[:, 1]], x[t[:, 2]]
    pos = ((a - p) ** 2).sum(1, dtype=dtype)
    neg = ((a - n) ** 2).sum(1, dtype=dtype)
    b = (pos - neg) + dtype(margin)
    rows = np.maximum(b, dtype(0))
    active = b >= 0 if active is None else np.asarray(active, bool)
    mean = rows.sum(dtype=dtype) / dtype(count)
    up = dtype(1 if upstream is None else upstream)
    g = dtype(2) * up / dtype(count)
    acc = np.zeros_like(x)
    mag = np.zeros_like(x)
    matches = np.zeros(len(x), np.int64)
    ta = t[active]
    a, p, n = x[ta[:, 0]], x[ta[:, 1]], x[ta[:, 2]]
    for idx, d in ((ta[:, 0], n - p), (ta[:, 1], p - a), (ta[:, 2], a - n)):
        np.add.at(acc, idx, d)
        np.add.at(mag, idx, np.abs(d))
        np.add.at(matches, idx, 1)
    return dict(rows=rows, active=active.astype(dtype), mean=mean, demb=(g * acc).astype(dtype), sq=pos + neg,
                mag=np.abs(g) * mag, matches=matches, g=g, acc=acc)


def hinge_concat(y, margin, dloss, dtype=f32):
    """embnet_triplet_hinge_fwd / _bwd on y[t, 3e] = concat(a, p, n) -> (loss [t], dy [t, 3e])."""
    y = np.asarray(y, dtype)
    e = y.shape[1] // 3
    a, p, n = y[:, :e], y[:, e:2 * e], y[:, 2 * e:]
    b = (((a - p) ** 2).sum(1, dtype=dtype) - ((a - n) ** 2).sum(1, dtype=dtype)) + dtype(margin)
    g = np.where(b >= 0, dtype(2) * np.asarray(dloss, dtype), dtype(0))[:, None]
    return np.maximum(b, dtype(0)), np.concatenate([g * (n - p), g * (p - a), g * (a - n)], axis=1).astype(dtype)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def lattice(seed, p, k, e, nonzero=6, moved=2, centre_amp=6, move_amp=2, dense=False):
    """-> (rows int64 [p*k, e], STEP); the embedding is rows * STEP.  A class centre has `nonzero` non-zero coordinates in
    [-centre_amp, centre_amp] (dense: every coordinate); a sample moves `moved` coordinates by [-move_amp, move_amp].  Classes come in
    groups of four: two ISOLATED ones (far from everything: their pairs are inactive), a base class and its SIBLING, the base's
    centre moved by one step in one coordinate (their members interleave: pairs are active, the candidate sets of the two random
    rules differ, loss values hit the margin exactly: D[a,p] == D[a,n]).  Every other group also plants one loss value of exactly 0: the
    base class's second sample copies its first (D[a,p] = 0) and the sibling's first sample is the base's first moved by four
    steps in one coordinate (D[a,n] = 0.5 = the margin of the tests)."""
    rs = np.random.RandomState(seed)
    cen = np.zeros((p, e), np.int64)
    for c in range(p):
        if c % 4 == 3:
            cen[c] = cen[c - 1]
            cen[c, rs.randint(e)] += rs.choice([-1, 1])
        elif dense:
            cen[c] = rs.randint(-centre_amp, centre_amp + 1, size=e)
        else:
            at = rs.choice(e, size=min(nonzero, e), replace=False)
            cen[c, at] = rs.randint(-centre_amp, centre_amp + 1, size=len(at))
    rows = np.repeat(cen, k, axis=0)
    for r in range(p * k):
        at = rs.choice(e, size=min(moved, e), replace=False)
        rows[r, at] += rs.randint(-move_amp, move_amp + 1, size=len(at))
    for c in range(3, p, 8):
        b = (c - 1) * k
        rows[b + 1] = rows[b]
        rows[c * k] = rows[b]
        rows[c * k, rs.randint(e)] += 4
    return rows, STEP


def fused_lattice(p, k, e, seed=9):
    """The lattice of the fused-kernel tests: dense centres and e / 8 moved coordinates, so that every 64-column step and every
    512-column sweep of a long row carries weight in the distances and in the hinge sums."""
    return lattice(seed, p, k, e, dense=True, moved=max(2, e // 8))[0]


def lattice_sqdist(rows):
    """Exact integer d^2 in units of STEP^2."""
    g = rows @ rows.T
    nn = np.diag(g)
    return nn[:, None] + nn[None, :] - 2 * g


def lattice_units_max(rows):
    """The largest partial sum any kernel can form on these rows, in units of STEP^2 (the exactness premise: < 2^24):
    sum |x_i y_i| bounds every partial Gram sum, 4 max|x|^2 bounds |x|^2 + |y|^2 + 2|x.y| and every (a-p)^2 + (a-n)^2 sum."""
    a = np.abs(rows)
    return int(4 * (a * a).sum(1).max())


def lattice_dist(rows):
    """float32 D = sqrt of the exact d^2 (correctly rounded, as the device's sqrtf is)."""
    return np.sqrt((lattice_sqdist(rows).astype(np.float64) * STEP * STEP).astype(f32)).astype(f32)


def _symmetric(rs, n, draw):
    d = np.triu(draw((n, n)), 1)
    return (d + d.T).astype(f32)


def quantised(seed, p, k):
    """D in multiples of 1/8: in-class distances in [0, 1], the others in [0, 2].  With margin 0.5 every loss value is a
    multiple of 1/8: exact 0 and exact margin hits, massive ties."""
    rs = np.random.RandomState(seed)
    n = p * k
    d = _symmetric(rs, n, lambda s: rs.randint(0, 17, size=s) / 8.0)
    cls = np.arange(n) // k
    inclass = _symmetric(rs, n, lambda s: rs.randint(0, 9, size=s) / 8.0)
    return np.where(cls[:, None] == cls[None, :], inclass, d).astype(f32)


def planted(seed, p, k):
    """Per anchor row, candidates only at a random non-empty subset of SPECIAL_COLUMNS + (nneg - 1) (negative order): in-class
    distances 1 + |j - i| / 64, the planted negatives at 1.25 or 1.125 (loss 0.25.. / 0.375..: a candidate of every rule, with
    ties for the arg-max) or at 1 + 1/64 (the distance of the neighbouring positive: that pair's loss EQUALS the margin, a
    candidate of random_hard only; the farther positives' exceed it), every other negative at 3 (loss < 0)."""
    rs = np.random.RandomState(seed)
    n, nneg = p * k, p * k - k
    special = np.array(sorted({c for c in SPECIAL_COLUMNS if c < nneg} | {nneg - 1}))
    d = np.full((n, n), 3.0, f32)
    for a in range(n):
        lo = (a // k) * k
        for j in range(lo, lo + k):
            d[a, j] = 0.0 if j == a else 1.0 + abs(j - a) / 64.0
        keep = special[rs.rand(len(special)) < 0.6]
        if len(keep) == 0:
            keep = special[rs.randint(len(special)):][:1]
        cols = np.where(keep < lo, keep, keep + k)
        d[a, cols] = rs.choice([1.25, 1.125, 1.0 + 1.0 / 64], size=len(cols), p=[0.4, 0.4, 0.2])
    return d


def none_qualifies(p, k):
    """In-class distance 1, every other 3: no pair has a candidate -> the fallback triplet."""
    n = p * k
    cls = np.arange(n) // k
    d = np.where(cls[:, None] == cls[None, :], 1.0, 3.0).astype(f32)
    np.fill_diagonal(d, 0)
    return d


def all_qualify(seed, p, k):
    """In-class distance 1, every other in {1.125, 1.25, 1.375}: every column of every pair is a candidate of every rule."""
    rs = np.random.RandomState(seed)
    n = p * k
    cls = np.arange(n) // k
    d = np.where(cls[:, None] == cls[None, :], 1.0, rs.choice([1.125, 1.25, 1.375], size=(n, n))).astype(f32)
    np.fill_diagonal(d, 0)
    return d


def nonfinite(seed, p, k):
    """quantised with NaN and +inf entries sprinkled in (about 3 % each) and whole NaN rows (about one in 16, at least one)."""
    rs = np.random.RandomState(seed + 1)
    d = quantised(seed, p, k)
    n = p * k
    r = rs.rand(n, n)
    d[r < 0.03] = np.nan
    d[(r >= 0.03) & (r < 0.06)] = np.inf
    rows = np.where(rs.rand(n) < 1.0 / 16)[0]
    d[rows if len(rows) else [rs.randint(n)]] = np.nan
    return d


FAMILIES = ("lattice", "quantised", "planted", "none", "all", "nonfinite")
FINITE_FAMILIES = FAMILIES[:-1]


def distance_family(family, seed, p, k, e=40):
    if family == "lattice":
        return lattice_dist(lattice(seed, p, k, e)[0])
    if family == "quantised":
        return quantised(seed, p, k)
    if family == "planted":
        return planted(seed, p, k)
    if family == "none":
        return none_qualifies(p, k)
    if family == "all":
        return all_qualify(seed, p, k)
    if family == "nonfinite":
        return nonfinite(seed, p, k)
    raise KeyError(family)


# ---- error bounds of the off-lattice families ----------------------------------------------------------------------------------------
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def sqdist_bound(x):
    """-> (d2 float64 [n,n], B2 [n,n]): |d2_kernel - d2| <= B2 = gamma(e + 3) (|x|^2 + |y|^2 + 2 sum |x_i y_i|)."""
    x = np.asarray(x, np.float64)
    nn = (x * x).sum(1)
    d2 = np.maximum(nn[:, None] + nn[None, :] - 2 * (x @ x.T), 0)
    np.fill_diagonal(d2, 0)
    mag = nn[:, None] + nn[None, :] + 2 * (np.abs(x) @ np.abs(x).T)
    return d2, gamma(x.shape[1] + 3) * mag


def dist_bound(x):
    """-> (D float64, delta, bad): |D_kernel - D| <= delta = B2 / D + u D; bad where D^2 <= 2 B2 (no bound on D there)."""
    d2, b2 = sqdist_bound(x)
    D = np.sqrt(d2)
    bad = d2 <= 2 * b2
    np.fill_diagonal(bad, False)                                                    # the kernels write an exact 0 there
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.where(bad, np.inf, b2 / D + U * D)
    np.fill_diagonal(delta, 0)
    return D, delta, bad


def decisions(x, p, k, margin, mode, seed):
    """What the float64 matrix decides and how firmly.  -> dict(lv [pairs, n-k] float64 loss values, slack [pairs, n-k] the summed
    delta of each value plus the two float32 roundings of the loss arithmetic, decided [pairs] bool, selected [pairs]: the pick of a
    decided pair (-1 = none)).  A pair is decided when every comparison its rule makes holds by more than the slack:
      hardest       the arg-max beats every other column by more than both slacks, and its value clears 0 by its slack;
      random rules  every column is inside or outside the candidate set by more than its slack (then the pick is the want-th)."""
    D, delta, _ = dist_bound(x)
    i, j, lo = pair_index(p, k)
    cols = negative_columns(p, k)
    lv = (D[i, j][:, None] - D[i[:, None], cols]) + margin
    mag = D[i, j][:, None] + D[i[:, None], cols] + margin
    slack = delta[i, j][:, None] + delta[i[:, None], cols] + 2 * U * mag + 2 * U * delta[i, j][:, None]
    pairs = len(lv)
    rows = np.arange(pairs)
    if mode == "hardest":
        best = np.argmax(lv, axis=1)
        bv, bs = lv[rows, best], slack[rows, best]
        gap = (bv[:, None] - lv) - (bs[:, None] + slack)
        gap[rows, best] = np.inf
        decided = (gap > 0).all(1) & (np.abs(bv) > bs)
        sel = np.where(bv > 0, best, -1)
    else:
        edge = np.abs(lv) > slack
        if mode == "semihard":
            edge &= np.abs(lv - margin) > slack
            cand = (lv > 0) & (lv < margin)
        else:
            cand = lv > 0
        decided = edge.all(1)
        total = cand.sum(1).astype(np.uint64)
        u = rng_u32(seed, np.arange(pairs, dtype=np.uint64), np.uint64(0)).astype(np.uint64)
        sel = ranked_pick(cand, ((u * total) >> np.uint64(32)).astype(np.int64))
    sel = np.where(sel < 0, -1, np.where(sel < lo, sel, sel + k))
    return dict(lv=lv, slack=slack, decided=decided & np.isfinite(slack).all(1), selected=sel.astype(np.int32))


def spread_rows(seed, p, k, e, sigma=0.3):
    """Unnormalised clustered rows whose norms spread over 2^10 within one batch (row r scaled by 2^(10 r' / (n-1)), r' a
    permutation, so that classes mix scales)."""
    rs = np.random.RandomState(seed)
    c = rs.randn(p, e)
    x = np.repeat(c, k, axis=0) + sigma * rs.randn(p * k, e)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    scale = 2.0 ** (10.0 * rs.permutation(p * k) / max(p * k - 1, 1))
    return (x * scale[:, None]).astype(f32)


# ---- the cases both test files run ---------------------------------------------------------------------------------------------------
# lattice (p, k, e): tests/test_mining_ref_cpu.py asserts on each that enough pairs are active, inactive, tied, multi-candidate
LATTICE_CASES = [(8, 4, 64), (64, 4, 128), (16, 16, 48), (512, 2, 32), (128, 8, 40)]
# (p, k) of the given-D mining tests: both routes of embnet_mine_triplets, ballot-block and trip edges (see the GPU file's table)
MINING_SHAPES = [(2, 2), (3, 3), (13, 5), (9, 8), (65, 4), (66, 4), (20, 16), (255, 4), (512, 2), (256, 4), (171, 6), (128, 8), (114, 9)]
MINING_SEED, MINING_E = 7, 40                             # distance_family(family, MINING_SEED, p, k, MINING_E) is what they run on
# off-lattice (family, p, k, e), inside the fused kernel's range.  The d^2 bound grows with e and the number of near-ties with the
# number of negatives, so a decision is only firmly testable at short rows and few columns: these are the shapes at which the bound
# leaves at most 2 % of the pairs undecided (asserted on the CPU; (8, 4, 256) leaves 17 %).  K = 16 has more pairs than the fused
# kernel has waves, K = 5 and 3 are odd, no E is a multiple of 64 but one that crosses it.  Long rows are the lattice's job.
OFF_LATTICE_CASES = [(f, p, k, e) for f in ("unit", "spread") for p, k, e in [(8, 4, 65), (6, 5, 24), (12, 3, 48), (5, 16, 40)]]


def off_lattice_rows(family, p, k, e):
    """unit: tests/golden/recipes.clustered_embeddings (unit-norm clustered rows); spread: spread_rows."""
    if family == "unit":
        import recipes
        return recipes.clustered_embeddings(11, p, k, e, 0.25)
    return spread_rows(11, p, k, e)
