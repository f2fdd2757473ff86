"""float64 restatement of distance-weighted sampling and the margin loss (include/embnet.h, embnet_margin_loss_fwd / _bwd;
csrc/margin_loss.hip) and the a-priori rounding bounds the kernels are held to.  NumPy only, no kernel code.
tests/test_margin_ref_cpu.py checks the restatement and the fitness of the GPU test's inputs; tests/test_margin_loss_gpu.py checks
the kernels against it.

Semantics (the header's).  beta, alpha, c_lo = cutoff, c_hi = nonzero_loss_cutoff ROUNDED TO fp32 (the C ABI takes floats).
D_ij = |x_i - x_j|.  For anchor i an other-class column n is eligible iff D_in < c_hi;  D~ = max(D, c_lo),
lw = (2 - e) log D~ - ((e - 3) / 2) log(1 - D~^2 / 4),  w = e^{lw - M} on eligible columns (M their largest lw), 0 elsewhere.
Draw j of anchor i (one per positive, ascending):  u_ij from two keyed words (draw_u), the pick = the first column of positive
weight whose inclusive prefix sum of w exceeds u total;  no eligible column: the floor(u (n-k))-th other-class column.
l+ = [D_ip - beta + alpha]+,  l- = [beta - D_in + alpha]+ per draw;  A = #{l+ > 0} + #{l- > 0};  loss = (sum l+ + sum l-) / max(A, 1).
W[i,p] = [l+ > 0] / D_ip,  W[i,n] = -#{active draws of i that picked n} / D_in,  0 where D = 0;
demb_i = (g / max(A,1)) sum_j (W_ij + W_ji)(x_i - x_j).

The smallest relative distance of u total to a prefix boundary is about 1e-8 on the test inputs, far below the fp32 rounding of
the weights, so the reference NEVER guesses a draw: picks are judged by kmeans_ref.pick_acceptable on the device's own weights, and
loss, W, counts and demb are computed from a GIVEN pick table.

Bounds.  u = 2^-24, gamma(n) = n u / (1 - n u).  Nothing is measured; the rounding counts are read off the header's form.
logf / expf are held to 3 ulp = 6 u (ms_ref.ULP_EXP_LOG), sqrtf and the division to 1 ulp = 2 u.  TINY = 2^-125 covers a flushed result.
  d2.  per_class (difference form): each difference one rounding, a lane's fma chain of ceil(e/64) squares, six butterfly additions,
      all terms non-negative:  |d2~ - d2| <= gamma(ceil(e/64) + 9) d2.  distance_matrix (Gram form n_i + n_j - 2 g): the norms a
      lane-strided chain, g ANY order of e products, three more operations:  |d2~ - d2| <= gamma(e + 8) (|x_i|^2 + |x_j|^2 + 2 A_ij),
      A_ij = sum_c |x_ic x_jc|.  exact (grid inputs, rows of +-1): 0.
  D.  D~ = sqrtf(max(d2~, 0)) lies in [Dlo, Dhi] = [sqrt(max(d2 - dd, 0)) (1 - 2u), sqrt(d2 + dd) (1 + 2u)];  dD = max(Dhi - D, D - Dlo).
  Decisions.  Eligibility (D~ < c_hi), the clamp (D~ < c_lo) and a hinge's sign are OPEN when [Dlo, Dhi] straddles them: the device
      may fall either way.  Values need no escape at the clamp and at a hinge (both continuous); eligibility and the 1/D of an open
      hinge do, and the tests give it.
  lw.  D~ -> Dt = max(D~, c_lo), a contraction: |Dt~ - Dt| <= dD.  L1~ = logf(Dt~): E1 = r1 + 6u (|log Dt| + r1), r1 = dD / (Dt - dD).
      t~ = fl(1 - fl(0.25 fl(Dt~ Dt~))): dt = 0.25 (2 Dt dD + dD^2)(1 + 2u) + 0.25 u Dt^2 (1 + u) + u (|t| + ...) , written out below.
      L2~ = logf(t~): E2 = r2 + 6u (|log t| + r2), r2 = dt / (t - dt).   lw~ = fl(fl(a1 L1~) - fl(a2 L2~)):
      Elw = (|a1| E1 + |a2| E2)(1 + u) + u (|a1 log Dt| + |a2 log t|) + u (|lw| + everything before) + TINY.
  w.  Relative to the DEVICE's own maximal column m (an open column may move the maximum): x = lw_n - lw_m,
      x~ = fl(lw~_n - lw~_m): Ex = (Elw_n + Elw_m)(1 + u) + u |x|;  w~ = expf(x~):  |w~ - e^x| <= e^x (expm1(Ex) + 6u e^Ex) + TINY.
      An underflowed weight (e = 512) is 0 <= its bound.
  hinge.  l~ = max(fl(fl(D~ - beta) + alpha), 0), a contraction of its argument:  El = dD + u (|D - beta| + dD) + u (|D - beta + alpha| + 2 dD).
  loss.  f64 sums; with the device's own A:  |loss~ - loss| <= sum El / max(A,1) + (u + 2^-40) |loss|.
  W.  Active, D > 0:  fl(m / D~), m <= k - 1 exact:  |W~ - m / D| <= m (dD / (D (D - dD)) + 2u / (D - dD)).  Dlo = 0: no bound but finiteness
      on a rounded d2 (the Gram form of coincident rows); on an exact d2 = 0 the weight is exactly 0.
  demb.  Against float64 of the DEVICE's own W and A (one fp32 rounding of an f64 sum):
      |demb~ - demb| <= u |demb| + (n + 8) 2^-53 (|g| / max(A,1)) (sum_j |M_ij| (|x_i| + |x_j|)) + 2^-149.
"""
import numpy as np

from kmeans_ref import pick_acceptable, rng_u32  # noqa: F401  (pick_acceptable re-exported for the tests)
from ms_ref import TINY, U, ULP_EXP_LOG, class_masks, exact_in_any_order, gamma, grid_inputs

OPEN_CAP = 0.01           # fitness of a continuous input: at most this share of its decisions open (multi_proxy_ref.OPEN_CAP)
SIGMA = 0.8
TEST_PARAMS = dict(beta=1.0, alpha=0.1, cutoff=0.5, nonzero_loss_cutoff=1.4)
DEFAULTS = dict(beta=1.2, alpha=0.2, cutoff=0.5, nonzero_loss_cutoff=1.4)
SHAPES = [(2, 2, 1), (4, 3, 1), (5, 7, 33), (9, 8, 40), (16, 16, 128), (4, 32, 16), (33, 16, 8), (32, 4, 256)]
WEIGHT_SHAPES = [(5, 4, 2), (5, 4, 3), (6, 4, 512)]      # an exponent vanishes at e = 2 and at e = 3; weights underflow at e = 512


def params32(beta=1.2, alpha=0.2, cutoff=0.5, nonzero_loss_cutoff=1.4):
    """The four parameters as the device has them: fp32 numbers."""
    return dict(beta=float(np.float32(beta)), alpha=float(np.float32(alpha)), c_lo=float(np.float32(cutoff)),
                c_hi=float(np.float32(nonzero_loss_cutoff)))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def seed_of(p, k, e):
    return 9000 + p * 1000 + k * 10 + e


def auto_path(p, k, e):
    """embnet_margin_loss_path restated: the per-class path's fit rule (embnet_batch_all_path's)."""
    n = p * k
    return "per_class" if k <= 16 and n <= 512 and k * (e + n) <= 16 * 1024 else "distance_matrix"


def paths(p, k, e):
    """Both forced paths where the per-class path fits."""
    return ["per_class", "distance_matrix"] if auto_path(p, k, e) == "per_class" else ["distance_matrix"]


def signed(p, k, e, seed=None):
    """recipes.clustered_embeddings without its two abs: P centres N(0, I), K members each at sigma = 0.8, unit rows of either sign, so
    that the distances reach beyond sqrt(2) (the recipe's non-negative rows never do)."""
    r = np.random.RandomState(seed_of(p, k, e) if seed is None else seed)
    c = r.randn(p, e)
    x = np.repeat(c, k, axis=0) + SIGMA * r.randn(p * k, e)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def weight_input(p, k, e):
    """The input of the weight tests: signed rows; at e = 512 the signed rows of length 8 padded with zeros, since 512 random
    directions are all but equidistant and only a spread of distances drives lw - M below log 2^-149."""
    if e < 512:
        return signed(p, k, e)
    x = np.zeros((p * k, e), np.float32)
    x[:, :8] = signed(p, k, 8, seed_of(p, k, e))
    return x


def grid(p, k, e, seed=None):
    """The signed rows on ms_ref's 1/q grid -> (x, the grid step 1/q)."""
    x, _, q = grid_inputs(signed(p, k, e, seed))
    return x, 1.0 / q


def d2_is_exact(x, unit):
    """True iff every x is a multiple of `unit` and 2 (|x_i|^2 + |x_j|^2) <= 2^24 unit^2 for every pair: every difference, square,
    product and partial sum of d2, in the difference form or the Gram form, in any order, with or without fma, is then a multiple
    of unit^2 below 2^24: exact in fp32."""
    m = np.asarray(x, np.float64) / unit
    return bool(np.array_equal(m, np.round(m)) and exact_in_any_order(x, unit) and 4.0 * (m * m).sum(1).max() <= 2 ** 24)


def error_class(x, path, unit=None):
    """The error class of d2 for `distances`: 'exact' for grid inputs (unit given) and for rows of +-1, else the forward path."""
    if unit is None and x.shape[1] == 1 and np.all(np.abs(x) == 1):
        unit = 1.0
    return "exact" if unit is not None and d2_is_exact(x, unit) else path


# ---- distances and decisions ------------------------------------------------------------------------------------------------------------
def distances(x, path):
    """-> dict(D, Dlo, Dhi, dD [n,n]) for a device on `path` ('per_class' | 'distance_matrix' | 'exact')."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n, e = x.shape
    d2 = np.zeros((n, n))
    for i0 in range(0, n, 64):
        d = x[i0:i0 + 64, None, :] - x[None, :, :]
        d2[i0:i0 + 64] = np.einsum("ijc,ijc->ij", d, d)
    if path == "exact":
        dd = np.zeros_like(d2)
    elif path == "per_class":
        dd = float(gamma(-(-e // 64) + 9)) * d2
    else:
        assert path == "distance_matrix", path
        nn = (x * x).sum(1)
        dd = float(gamma(e + 8)) * (nn[:, None] + nn[None, :] + 2.0 * (np.abs(x) @ np.abs(x).T))
    dist = np.sqrt(d2)
    lo = np.sqrt(np.maximum(d2 - dd, 0.0)) * (1.0 - 2.0 * U)
    hi = np.sqrt(d2 + dd) * (1.0 + 2.0 * U)
    return dict(D=dist, Dlo=lo, Dhi=hi, dD=np.maximum(hi - dist, dist - lo), exact=path == "exact")


def _down(v):
    v32 = np.asarray(v, np.float64).astype(np.float32)
    return np.where(v32.astype(np.float64) > v, np.nextafter(v32, np.float32(-np.inf)), v32)


def _up(v):
    v32 = np.asarray(v, np.float64).astype(np.float32)
    return np.where(v32.astype(np.float64) < v, np.nextafter(v32, np.float32(np.inf)), v32)


def hinge32(d32, par, side):
    """The header's hinge on fp32 distances, in fp32 arithmetic: side +1 the positives', -1 the drawn negatives'."""
    d32, b, a = np.asarray(d32, np.float32), np.float32(par["beta"]), np.float32(par["alpha"])
    v = ((d32 - b).astype(np.float32) + a) if side > 0 else ((b - d32).astype(np.float32) + a)
    return np.maximum(v.astype(np.float32), np.float32(0))


def decisions(dist, p, k, par):
    """For D~ anywhere in [Dlo, Dhi]: -> dict(sure / may for eligibility, the positives' hinge and a negative column's hinge, the open
    masks, share: open decisions over all decisions: eligibility, clamp and hinge per negative pair, hinge per positive pair)."""
    pos, neg = class_masks(p, k)
    lo, hi = dist["Dlo"], dist["Dhi"]
    elig_sure, elig_may = neg & (hi < par["c_hi"]), neg & (lo < par["c_hi"])
    clamp_open = neg & (lo < par["c_lo"]) & (par["c_lo"] < hi)
    lo32, hi32 = _down(lo), _up(hi)
    pos_sure, pos_may = pos & (hinge32(lo32, par, +1) > 0), pos & (hinge32(hi32, par, +1) > 0)
    neg_sure, neg_may = neg & (hinge32(hi32, par, -1) > 0), neg & (hinge32(lo32, par, -1) > 0)
    n_open = (elig_sure != elig_may).sum() + clamp_open.sum() + (pos_sure != pos_may).sum() + (neg_sure != neg_may).sum()
    return dict(pos=pos, neg=neg, elig_sure=elig_sure, elig_may=elig_may, clamp_open=clamp_open, pos_sure=pos_sure, pos_may=pos_may,
                neg_sure=neg_sure, neg_may=neg_may, share=float(n_open) / float(3 * neg.sum() + pos.sum()))


# ---- the sampler --------------------------------------------------------------------------------------------------------------------------
def draw_u(seed, i, j):
    """u_ij = (((rng(seed, i, 2j) << 32) | rng(seed, i, 2j+1)) >> 11) 2^-53, exactly representable."""
    bits = (rng_u32(seed, i, 2 * j) << 32) | rng_u32(seed, i, 2 * j + 1)
    return float(bits >> 11) * 2.0 ** -53


def positives(i, k):
    """The anchor's positives in ascending column order: ordinal j -> column."""
    lo = (i // k) * k
    return [c for c in range(lo, lo + k) if c != i]


def fallback_pick(u, i, n, k):
    """The floor(u (n-k))-th other-class column in ascending order."""
    lo, idx = (i // k) * k, int(u * (n - k))
    return idx if idx < lo else idx + k


def log_weights(dist, e, par):
    """f64 lw [n,n] (every column, as if eligible) and its bound Elw (module docstring)."""
    d, dd = dist["D"], dist["dD"]
    a1, a2 = float(2 - e), 0.5 * float(e - 3)
    dt = np.maximum(d, par["c_lo"])
    ok = dt < 2.0
    dt = np.where(ok, dt, 1.0)
    t = 1.0 - 0.25 * dt * dt
    l1, l2 = np.log(dt), np.log(t)
    lw = a1 * l1 - a2 * l2
    with np.errstate(divide="ignore", invalid="ignore"):
        r1 = dd / (dt - dd)
        e1 = r1 + ULP_EXP_LOG * (np.abs(l1) + r1)
        et = 0.25 * (2.0 * dt * dd + dd * dd) * (1.0 + 2.0 * U) + 0.25 * U * dt * dt * (1.0 + U)
        et = et + U * (np.abs(t) + et)
        r2 = np.where(et < t, et / (t - et), np.inf)
        e2 = r2 + ULP_EXP_LOG * (np.abs(l2) + r2)
        first = (abs(a1) * e1 + abs(a2) * e2) * (1.0 + U) + U * (np.abs(a1 * l1) + np.abs(a2 * l2))
        elw = first + U * (np.abs(lw) + first) + TINY
    return np.where(ok, lw, -np.inf), np.where(ok, elw, np.inf)


def weights64(dist, p, k, e, par):
    """The f64 sampling weights [n,n] (0 on own-class and ineligible columns; a row of zeros: a fall-back anchor)."""
    _, neg = class_masks(p, k)
    elig = neg & (dist["D"] < par["c_hi"])
    lw, _ = log_weights(dist, e, par)
    big = np.where(elig, lw, -np.inf).max(1)
    with np.errstate(invalid="ignore"):
        return np.where(elig, np.exp(np.where(elig, lw - big[:, None], 0.0)), 0.0), elig


def weight_bound(dist, e, par, top):
    """Against the device's own maximal column top[i] of each row: -> (w64 [n,n] = e^{lw_n - lw_top}, bound [n,n])."""
    lw, elw = log_weights(dist, e, par)
    rows = np.arange(lw.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        x = lw - lw[rows, top][:, None]
        ex = (elw + elw[rows, top][:, None]) * (1.0 + U) + U * np.abs(x)
        w = np.exp(x)
        return w, w * (np.expm1(ex) + ULP_EXP_LOG * np.exp(ex)) + TINY


def sample64(x, p, k, par, seed):
    """The whole sampler in f64 on f64 weights: -> triplets int32 [n (k-1), 3].  For CPU-side tests of the restatement; a device's
    picks are judged on ITS weights (pick_acceptable), never against these."""
    n, e = x.shape
    w, _ = weights64(distances(x, "exact"), p, k, e, par)
    out = []
    for i in range(n):
        prefix, total = np.cumsum(w[i]), w[i].sum()
        for j, pc in enumerate(positives(i, k)):
            u = draw_u(seed, i, j)
            if total == 0.0:
                pick = fallback_pick(u, i, n, k)
            else:
                hit = np.nonzero((w[i] > 0) & (prefix > u * total))[0]
                pick = int(hit[0]) if hit.size else int(np.nonzero(w[i] > 0)[0][-1])
            out.append((i, pc, pick))
    return np.asarray(out, np.int32)


# ---- the loss given a pick table ------------------------------------------------------------------------------------------------------------
def reference(dist, p, k, par, trip):
    """float64 hinge sums, W as if every hinge with a positive f64 value were active, and what the tests need to judge a device:
    -> dict(loss_sum, El_sum, cp, cn, A, W [n,n], draws [n,n] = how often i drew n, lp [n,n], ln [n,n] = the hinge of a column)."""
    d, dd = dist["D"], dist["dD"]
    pos, neg = class_masks(p, k)
    n = d.shape[0]
    beta, alpha = par["beta"], par["alpha"]
    trip = np.asarray(trip, np.int64)
    draws = np.zeros((n, n), np.int64)
    np.add.at(draws, (trip[:, 0], trip[:, 2]), 1)
    lp = np.where(pos, np.maximum(d - beta + alpha, 0.0), 0.0)
    ln = np.where(neg, np.maximum(beta - d + alpha, 0.0), 0.0)
    el = dd + U * (np.abs(d - beta) + dd) + U * (np.abs(np.where(pos, d - beta, beta - d) + alpha) + 2.0 * dd)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(d > 0, 1.0 / d, 0.0)
        bw = np.where(d > dd, dd / (d * (d - dd)) + 2.0 * U / (d - dd), np.inf)
    w = np.where(lp > 0, inv, 0.0) - np.where(ln > 0, draws * inv, 0.0)
    cp, cn = int((lp > 0).sum()), int((draws * (ln > 0)).sum())
    return dict(loss_sum=float(lp.sum() + (draws * ln).sum()), El_sum=float((el * pos).sum() + (el * draws).sum()), cp=cp, cn=cn,
                A=cp + cn, W=w, draws=draws, lp=lp, ln=ln, W_on=np.where(pos, inv, -draws * inv),
                bound_W=np.where(pos, bw, np.where(draws > 0, draws * np.where(draws > 0, bw, 0.0), 0.0)), pos=pos, neg=neg)


def loss_and_bound(ref, a_dev):
    """The loss with the device's own A and its bound."""
    a = max(int(a_dev), 1)
    loss = ref["loss_sum"] / a
    return loss, ref["El_sum"] / a + (U + 2.0 ** -40) * abs(loss) + TINY


def demb(x, w, a, upstream=1.0):
    """float64 demb = (g / max(A,1)) (s x - M X), M = W + W^T, from a given W and A, and its bound (module docstring)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    w = np.asarray(w, np.float64)
    m = w + w.T
    scale = float(np.float32(upstream)) / max(int(a), 1)
    want = scale * (m.sum(1)[:, None] * x - m @ x)
    mag = np.abs(m).sum(1)[:, None] * np.abs(x) + np.abs(m) @ np.abs(x)
    return want, U * np.abs(want) + (x.shape[0] + 8) * 2.0 ** -53 * abs(scale) * mag + 2.0 ** -149
