"""float64 restatement of the multi-similarity loss (include/embnet.h, csrc/multi_similarity.hip) and the a-priori rounding bounds
its kernels are held to.  NumPy only, no kernel code.  tests/test_ms_ref_cpu.py checks the restatement (autograd, differences,
hand cases) and the fitness of the GPU test's inputs; tests/test_ms_loss_gpu.py checks the kernels against it.

Semantics (the header's).  X [N, E] fp32, N = P K, rows c K .. c K + K - 1 are class c; S = X X^T.  With alpha, beta, base,
epsilon ROUNDED TO fp32 (the C ABI takes floats):
    negative n of anchor i kept iff fl(S_in + epsilon) > min_p S_ip;   positive p kept iff fl(max_n S_in + epsilon) > S_ip,
    evaluated on the fp32-rounded S with one fp32 addition (fl);
    t+_p = -alpha (S_ip - base), t-_n = beta (S_in - base), m = max(0, max kept t) per side, d = e^-m + sum_kept e^(t - m),
    l_i = (m+ + log d+) / alpha + (m- + log d-) / beta  (0 for an anchor that keeps nothing),  loss = sum_i l_i / N,
    G[i,p] = -e^(t+_p - m+) / d+,  G[i,n] = +e^(t-_n - m-) / d-,  0 elsewhere;  demb = (g / N) (G + G^T) X.

Bounds.  u = 2^-24, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability, 3.1).  Nothing is measured; the rounding counts are
read off multi_similarity.hip.

  S.  |S~_ij - S_ij| <= dS_ij = gamma_S A_ij, A_ij = sum_c |x_ic x_jc|.
      per-class path: lane l owns the columns l, l + 64, ...: a chain of ceil(E / 64) fma (one rounding each), then six
      additions of the wave butterfly: ceil(E / 64) + 6 roundings on the longest path; gamma_S = gamma(ceil(E / 64) + 7) leaves one
      to spare.  similarity-matrix path: embnet_dense_dgrad_f32's k-ordered chain, a rounded product and a rounded addition per k:
      gamma_S = gamma(E + 1), what tests/dense_ref.py allows that kernel.
      On the grid inputs (grid_inputs) every product is a multiple of 1 / q^2 and every partial sum is below 2^24 / q^2, so S~ = S
      in ANY order: gamma_S = 0 (test_ms_ref_cpu.py asserts the premise).
  t.  t~ = fl(c fl(S~ - base)) = c (S~ - base)(1 + e1)(1 + e2), c = alpha or beta:
      |t~ - t| <= Dt = c dS (1 + gamma(2)) + gamma(2) |t|.
  m.  m~ = max(0, t~ of the hardest pair); |max_j a_j - max_j b_j| <= max_j |a_j - b_j| over the kept pairs, and max(0, .) is a
      contraction:  |m~ - m| <= Dm = max over the anchor's kept pairs of Dt.
  z = t - m.  z~ = fl(t~ - m~):  |z~ - z| <= Dz = Dt + Dm + u (|z| + Dt + Dm).     (exp's input error is ABSOLUTE in t)
  e = exp(z).  The device's expf and logf are the ROCm device library's; OpenCL's full profile, which that library implements,
      guarantees 3 ulp = 6 u for both (HIP's own table says 1 ulp).  e~ = e exp(z~ - z)(1 + 6u'):
      relative error rho = expm1(Dz) + 6 u exp(Dz);  e0 = exp(-m): rho0 = expm1(Dm) + 6 u exp(Dm).
      fp32 underflow: d >= 1 (the hardest pair contributes e^0 when m > 0, e^-m = 1 otherwise), so e and G below the smallest
      normal number 2^-126 may be flushed: an absolute 2^-125 joins the weight's bound.
  d = e0 + sum e.  All terms positive; a lane adds at most ceil(cols / 64) of them (cols = K for the positives, N for the
      negatives), the butterfly adds six times, e0 joins with one more: L = ceil(cols / 64) + 7 roundings,
      rho_d = (sum_j rho_j e_j + rho0 e0) / d (1 + gamma(L)) + gamma(L).
  G = fl(e / d):  |G~ - G| <= |G| ((rho + rho_d) / (1 - rho_d) (1 + u) + u) + 2^-125.
  l side = fl(fl(m + logf(d)) / c):  |log d~ - log d| <= lam = -log(1 - rho_d); logf: 6 u (|log d| + lam); the addition and the
      division round relative to their own results:
      |side~ - side| <= (Dm + lam + 6 u (|log d| + lam)) (1 + gamma(2)) / c + gamma(2) |side|.
  l_i = fl(side+ + side-): + u (|l_i| + both side bounds).  The sum over anchors and the division by N are float64 on the device;
      the final cast adds u |loss|:   |loss~ - loss| <= mean_i bound(l_i) + u |loss| + 2^-40 |loss|.
  backward, against float64 of the DEVICE's own G:  M = G + G^T is one float64 addition, the products join a float64 fma chain of N
      terms, the scale g / N is two more float64 roundings, the store rounds once to fp32:
      |demb~ - demb| <= u |demb| + (N + 8) 2^-53 (|g| / N) sum_j |M_ij| |x_jc| + 2^-149.

Open decisions (continuous inputs).  The device's S~ is SOME fp32 number in [S - dS, S + dS]; fl is monotone, so a pair is surely
kept / surely dropped when the predicate gives the same answer at both ends of every interval involved (an fp32 number >= S - dS
is >= float32(S - dS) whichever way that rounds).  An anchor with a pair that is neither is OPEN: either answer is correct there.
"""
import numpy as np

U = 2.0 ** -24
ULP_EXP_LOG = 6.0 * U                                     # 3 ulp
TINY = 2.0 ** -125


def gamma(n):
    n = np.asarray(n, np.float64) * U
    assert np.all(n < 0.5)
    return n / (1.0 - n)


def gamma_s(path, e):
    """gamma_S of the forward path ('per_class' | 'similarity_matrix') at embedding length e; 0 for 'exact' (grid inputs)."""
    if path == "exact":
        return 0.0
    if path == "per_class":
        return float(gamma(-(-e // 64) + 7))
    assert path == "similarity_matrix", path
    return float(gamma(e + 1))


def params32(alpha=2.0, beta=50.0, base=0.5, epsilon=0.1):
    """The four parameters as the C ABI sees them: rounded to fp32."""
    return tuple(np.float32(v) for v in (alpha, beta, base, epsilon))


def class_masks(p, k):
    """-> (pos [N,N]: same class, not the diagonal; neg [N,N]: other classes)."""
    cls = np.repeat(np.arange(p), k)
    same = cls[:, None] == cls[None, :]
    return same & ~np.eye(p * k, dtype=bool), ~same


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def grid_q(e):
    """The power of two >= 4 sqrt(E), at least 16."""
    q = 16
    while q < 4.0 * np.sqrt(e):
        q *= 2
    return q


def grid_inputs(x):
    """x (unit rows, e.g. recipes.clustered_embeddings) rounded to multiples of 1/q, and epsilon = 13/128 + 1/(2 q^2): every S is a
    multiple of 1/q^2 and exact in fp32 in any summation order, S + epsilon is exact, and no mining decision is closer than half a
    grid step 1/(2 q^2).  -> (x fp32, epsilon, q)."""
    q = grid_q(x.shape[1])
    return (np.round(np.asarray(x, np.float64) * q) / q).astype(np.float32), 13.0 / 128.0 + 1.0 / (2.0 * q * q), q


def exact_in_any_order(x, unit):
    """True iff every x is an integer multiple of `unit` and sum_c |x_ic x_jc| <= 2^24 unit^2 for every pair: every product and
    every partial sum of S, in any order and with or without fma, is then an integer multiple of unit^2 below 2^24: exact in fp32."""
    x = np.asarray(x, np.float64)
    m = x / unit
    return bool(np.array_equal(m, np.round(m)) and (np.abs(m) @ np.abs(m).T).max() <= 2 ** 24)


# ---- mining -----------------------------------------------------------------------------------------------------------------------
def _row_min(v, mask):
    return np.where(mask, v, np.float32(np.inf)).min(1)


def _row_max(v, mask):
    return np.where(mask, v, np.float32(-np.inf)).max(1)


def mine(s32, p, k, eps32):
    """The header's predicates on an fp32 similarity matrix, in fp32 arithmetic.  -> (keep_pos, keep_neg) bool [N,N]."""
    s32 = np.asarray(s32, np.float32)
    eps32 = np.float32(eps32)
    pos, neg = class_masks(p, k)
    mn, mx = _row_min(s32, pos), _row_max(s32, neg)
    keep_neg = neg & ((s32 + eps32) > mn[:, None])
    keep_pos = pos & ((mx + eps32)[:, None] > s32)
    return keep_pos, keep_neg


def decisions(x, p, k, eps32, gs):
    """For S~ anywhere in [S - gs A, S + gs A]: -> dict(sure_pos, may_pos, sure_neg, may_neg [N,N], open [N]): pairs kept at every
    admissible S~, pairs kept at some, and the anchors where the two differ."""
    x = np.asarray(x, np.float64)
    eps32 = np.float32(eps32)
    s, a = x @ x.T, np.abs(x) @ np.abs(x).T
    lo, hi = (s - gs * a).astype(np.float32), (s + gs * a).astype(np.float32)
    pos, neg = class_masks(p, k)
    mn_lo, mn_hi = _row_min(lo, pos), _row_min(hi, pos)
    mx_lo, mx_hi = _row_max(lo, neg), _row_max(hi, neg)
    sure_neg = neg & ((lo + eps32) > mn_hi[:, None])
    may_neg = neg & ((hi + eps32) > mn_lo[:, None])
    sure_pos = pos & ((mx_lo + eps32)[:, None] > hi)
    may_pos = pos & ((mx_hi + eps32)[:, None] > lo)
    return dict(sure_pos=sure_pos, may_pos=may_pos, sure_neg=sure_neg, may_neg=may_neg,
                open=(sure_neg != may_neg).any(1) | (sure_pos != may_pos).any(1))


# ---- the loss -----------------------------------------------------------------------------------------------------------------------
def _side(t, keep):
    """Stable log-sum-exp of one side.  -> (m [N], e [N,N] = exp(t - m) on the kept pairs, e0 [N] = exp(-m), d [N])."""
    m = np.maximum(np.where(keep, t, -np.inf).max(1), 0.0)
    e = np.where(keep, np.exp(np.where(keep, t - m[:, None], 0.0)), 0.0)
    e0 = np.exp(-m)
    return m, e, e0, e0 + e.sum(1)


def reference(x, p, k, alpha=2.0, beta=50.0, base=0.5, epsilon=0.1, keep=None):
    """float64 loss, per-anchor losses, G and counts of an fp32 block x.  keep = (keep_pos, keep_neg) overrides the mining (the
    kept sets are constants of the loss: autograd checks, and open anchors judged with the device's own decision)."""
    a32, b32, l32, e32 = params32(alpha, beta, base, epsilon)
    al, be, ba = float(a32), float(b32), float(l32)
    x = np.asarray(x, np.float32).astype(np.float64)
    n = p * k
    assert x.shape[0] == n
    s = x @ x.T
    keep_pos, keep_neg = mine(s.astype(np.float32), p, k, e32) if keep is None else keep
    tp, tn = -al * (s - ba), be * (s - ba)
    mp, ep, e0p, dp = _side(tp, keep_pos)
    mg, en, e0n, dn = _side(tn, keep_neg)
    active = keep_neg.any(1)
    side_p = np.where(active, (mp + np.log(dp)) / al, 0.0)
    side_n = np.where(active, (mg + np.log(dn)) / be, 0.0)
    ell = side_p + side_n
    g = en / dn[:, None] - ep / dp[:, None]
    counts = np.array([keep_pos.sum(), keep_neg.sum(), active.sum(), keep_pos.sum() + keep_neg.sum()], np.int64)
    return dict(loss=ell.sum() / n, ell=ell, G=g, keep_pos=keep_pos, keep_neg=keep_neg, counts=counts, active=active, S=s,
                sides=dict(pos=dict(c=al, t=tp, m=mp, e=ep, e0=e0p, d=dp, side=side_p, cols=k),
                           neg=dict(c=be, t=tn, m=mg, e=en, e0=e0n, d=dn, side=side_n, cols=n)))


def grad(x, g, upstream=1.0, rows=None):
    """float64 demb = (upstream / N) (G + G^T) X for `rows`, and its bound (module docstring), from a given G."""
    x = np.asarray(x, np.float32).astype(np.float64)
    g = np.asarray(g, np.float64)
    n = x.shape[0]
    rows = np.arange(n) if rows is None else rows
    m = g[rows] + g.T[rows]
    up = float(np.float32(upstream))
    want = (up / n) * (m @ x)
    bound = U * np.abs(want) + (n + 8) * 2.0 ** -53 * (abs(up) / n) * (np.abs(m) @ np.abs(x)) + 2.0 ** -149
    return want, bound


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def bounds(x, ref, gs):
    """-> (bound_G [N,N], bound_ell [N], bound_loss) for a device whose S is within gs A of the truth (module docstring)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    ds = gs * (np.abs(x) @ np.abs(x).T)
    n = x.shape[0]
    g2 = float(gamma(2))
    bound_g = np.zeros((n, n))
    bound_ell = np.zeros(n)
    for name, keep in (("pos", ref["keep_pos"]), ("neg", ref["keep_neg"])):
        sd = ref["sides"][name]
        c, t, m, e, e0, d = sd["c"], sd["t"], sd["m"], sd["e"], sd["e0"], sd["d"]
        dt = np.where(keep, c * ds * (1.0 + g2) + g2 * np.abs(t), 0.0)
        dm = dt.max(1)
        z = np.where(keep, t - m[:, None], 0.0)
        dz = dt + dm[:, None] + U * (np.abs(z) + dt + dm[:, None])
        rho = np.where(keep, np.expm1(dz) + ULP_EXP_LOG * np.exp(dz), 0.0)
        rho0 = np.expm1(dm) + ULP_EXP_LOG * np.exp(dm)
        gl = float(gamma(-(-sd["cols"] // 64) + 7))
        rho_d = ((rho * e).sum(1) + rho0 * e0) / d * (1.0 + gl) + gl
        assert np.all(rho_d < 0.5), "the similarity error is too large for a meaningful bound"
        w = e / d[:, None]
        bound_g += np.where(keep, w * ((rho + rho_d[:, None]) / (1.0 - rho_d[:, None]) * (1.0 + U) + U) + TINY, 0.0)
        lam = -np.log1p(-rho_d)
        b_side = (dm + lam + ULP_EXP_LOG * (np.abs(np.log(d)) + lam)) * (1.0 + g2) / c + g2 * np.abs(sd["side"])
        bound_ell += np.where(ref["active"], b_side, 0.0)
    bound_ell = bound_ell + U * (np.abs(ref["ell"]) + bound_ell)
    bound_loss = bound_ell.sum() / n + (U + 2.0 ** -40) * abs(ref["loss"])
    return bound_g, bound_ell, bound_loss


# ---- the cases the CPU and the GPU test share -------------------------------------------------------------------------------------
PER_CLASS_SHAPES = [(8, 4, 256), (32, 4, 256), (64, 4, 512), (3, 3, 64), (20, 3, 128), (16, 16, 128), (5, 7, 33)]
VALUE_SHAPES = PER_CLASS_SHAPES + [(4, 4, 4096), (256, 8, 128)]          # grid inputs; the last two take the matrix path
CONTINUOUS_SHAPES = PER_CLASS_SHAPES + [(4, 32, 64), (4, 4, 4096)]        # (256,8,128), (64,8,128): 6 - 27 % open anchors
SIGMA = 0.8


def seed_of(p, k, e):
    return p * 1000 + k * 10 + e


def auto_path(p, k, e):
    """embnet_ms_loss_path restated: the per-class path's fit rule."""
    n = p * k
    return "per_class" if k <= 16 and n <= 512 and k * (e + n) <= 16 * 1024 else "similarity_matrix"
