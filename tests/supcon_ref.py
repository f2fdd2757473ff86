"""float64 restatement of the SupCon / NT-Xent loss (include/embnet.h, csrc/supcon.hip) and the a-priori rounding bounds its
kernels are held to.  NumPy only, no kernel code.  tests/test_supcon_ref_cpu.py checks the restatement (autograd, differences, a
scalar restatement, hand cases) and the fitness of the GPU test's inputs; tests/test_supcon_gpu.py checks the kernels against it.

Semantics (the header's).  X [N, E] fp32, N = P K, rows c K .. c K + K - 1 are class c; S = X X^T; tau ROUNDED TO fp32 (the C ABI
takes a float); t_ij = S_ij / tau.  P_i: the other rows of i's class, N_i: the rows of other classes.
    'all'        l_i = lse_{a != i} t_ia - (1/(K-1)) sum_p t_ip;   G_ij = (1/tau)(softmax_{a != i}(t_i.)_j - [j in P_i]/(K-1)), G_ii = 0
    'negatives'  d_ip = e^{t_ip} + sum_n e^{t_in};  l_i = (1/(K-1)) sum_p (log d_ip - t_ip);
                 G_ip = (1/tau)(1/(K-1))(e^{t_ip}/d_ip - 1),  G_in = (1/tau)(1/(K-1)) e^{t_in} sum_p 1/d_ip,  G_ii = 0
    loss = sum_i l_i / N;  demb = (g / N)(G + G^T) X;  counts = {N (K-1), anchors with max_n S_in >= min_p S_ip on the fp32 S}.
The restatement uses the header's stable forms (the plain ones overflow float64 at rows of norm 30).

Bounds.  u = 2^-24, gamma(n) = n u / (1 - n u) (ms_ref.gamma).  Nothing is measured; the rounding counts are read off supcon.hip
and pair_loss.h.  "flush": a result below 2^-126 may become 0, an absolute 2^-125 = TINY.

  S.  |S~ - S| <= dS = gamma_S A, A_ij = sum_c |x_ic x_jc|, gamma_S = ms_ref.gamma_s(path, E): the staging is pair_loss.h's, the
      one multi_similarity.hip runs on (per-class: gamma(ceil(E/64) + 7); similarity matrix: gamma(E + 1); grid inputs: 0).
  t.  r~ = fl(1 / tau) = (1/tau)(1 + d1);  t~ = fl(S~ r~) = S~ (1/tau)(1 + d1)(1 + d2):
      |t~ - t| <= Dt = (dS / tau)(1 + gamma(2)) + gamma(2) |t|.
  maxima.  fl(. r~) is monotone, so the device's maximum of a set IS the t~ of some member: |M~ - M| <= DM = max over the set of Dt.
  z = t - M (an exponent's argument), z~ = fl(t~ - M~):  |z~ - z| <= Dz = Dt + DM + u (|z| + Dt + DM)      (ABSOLUTE in t)
  e = exp(z):  expf and logf are held to 3 ulp = 6 u (ms_ref.ULP_EXP_LOG):  relative rho = expm1(Dz) + 6 u exp(Dz), + flush.
  sums of non-negative terms: a lane adds at most ceil(cols / 64) of them, the butterfly six times: gamma(ceil(cols / 64) + 7)
      (one to spare, as ms_ref), cols = N for sums over columns, K for sums over the positives.

  'all'.  d = sum_{a != i} e_a >= 1:  rho_d = sum_a rho_a e_a / d (1 + gamma_N) + gamma_N + N 2^-126.
      w = fl(e / d):  |w~ - w| <= Bw = w ((rho + rho_d) / (1 - rho_d)(1 + u) + u) + TINY.
      v = w - [pos] ck, ck~ = fl(1 / (K-1)) = ck (1 + d):  |v~ - v| <= Bv = Bw + u ck + u (|v| + Bw + u ck)   (positives; Bw else)
      G = fl(r~ v~):  |G~ - G| <= (1/tau)((1 + gamma(2)) Bv + gamma(2) |v|) + TINY.       ABSOLUTE: w - ck cancels.
      l_i = fl(logf(d~) + fl(sum_p fl(M~ - t~_p) / (K-1))):  h_p = M - t_p >= 0 with |h~ - h| <= Dz_p; the sum of the h~ (all >= 0):
      B_sum = sum Dz_p (1 + gamma_K) + gamma_K sum h;  the division: B_pm = B_sum / (K-1) (1 + u) + u pm;
      the logarithm: lam = -log(1 - rho_d), B_log = lam + 6 u (log d + lam);   B_l = (B_log + B_pm)(1 + u) + u l_i.
  'negatives'.  Mn = max_n t_n, e_n = exp(t_n - Mn), En = sum_n e_n >= 1: rho_n, rho_E as above.  Per positive p:
      m = max(t_p, Mn): |m~ - m| <= Dm = max(Dt_p, DMn);  a = exp(t_p - m), b = exp(Mn - m) with their Dz and rho_a, rho_b;
      bE = fl(b~ En~): rho_bE = (1 + rho_b)(1 + rho_E)(1 + u) - 1;  D = fl(a~ + bE~) >= 1:
      rho_D = (rho_a a + rho_bE bE) / D (1 + u) + u + 3 TINY;
      l_p = fl(fl(m~ - t~_p) + logf(D~)):  B_lp = (Dh + lamD + 6 u (log D + lamD))(1 + u) + u l_p, Dh the Dz form of m - t_p;
      l_i = fl(sum_p l_p / (K-1)):  B_l = (sum B_lp (1 + gamma_K) + gamma_K sum l_p) / (K-1) (1 + u) + u l_i.
      q_p = fl(b~ / D~): rho_q = (rho_b + rho_D) / (1 - rho_D)(1 + u) + u, + flush;  Q = sum_p q_p:
      B_Q = sum rho_q q (1 + gamma_K) + gamma_K Q + K TINY.
      rck~ = fl(r~ ck~) = (ck / tau)(1 + gamma(3)), so one more product leaves (1 + gamma(4)):
      G_in = fl(rck~ fl(e~_n Q~)):  B = e_n B_Q + rho_n e_n (Q + B_Q) + TINY (Q + B_Q + 1) and
          |G~ - G| <= (ck / tau)((1 + gamma(4))(B (1 + u) + u e_n Q) + gamma(4) e_n Q) + TINY;
      G_ip = fl(rck~ fl(fl(a~ / D~) - 1)):  y = a / D, By = y ((rho_a + rho_D) / (1 - rho_D)(1 + u) + u) + TINY, v = y - 1,
          Bv = By + u (|v| + By),  |G~ - G| <= (ck / tau)((1 + gamma(4)) Bv + gamma(4) |v|) + TINY.
  loss.  The sum over anchors and the division by N are float64 on the device; the final cast adds u |loss|:
      |loss~ - loss| <= mean_i B_l + (u + 2^-40) |loss|.
  backward.  ms_ref.grad: float64 of the DEVICE's own G, u |demb| + (N + 8) 2^-53 (|g| / N) sum_j |M_ij| |x_jc| + 2^-149.

Violating anchors.  The device's S~ is SOME fp32 number in [S - dS, S + dS] (ms_ref's argument): an anchor surely violates when
max_n float32(S - dS) >= min_p float32(S + dS), possibly when max_n float32(S + dS) >= min_p float32(S - dS); it is OPEN when the
two differ, and the device's count must lie between the sure and the possible count.
"""
import numpy as np

from ms_ref import TINY, U, ULP_EXP_LOG, class_masks, gamma

DENOMINATORS = ("all", "negatives")


def tau32(temperature):
    """The temperature as the C ABI sees it."""
    return float(np.float32(temperature))


def _rmax(v, mask):
    return np.where(mask, v, -np.inf).max(1)


def _rmin(v, mask):
    return np.where(mask, v, np.inf).min(1)


# ---- the counter ------------------------------------------------------------------------------------------------------------------
def violating(s32, p, k):
    """Anchors with max_n S_in >= min_p S_ip on an fp32 similarity matrix.  -> bool [N]."""
    s32 = np.asarray(s32, np.float32)
    pos, neg = class_masks(p, k)
    return _rmax(s32, neg) >= _rmin(s32, pos)


def decisions(x, p, k, gs):
    """For S~ anywhere in [S - gs A, S + gs A]: -> dict(sure, may, open bool [N])."""
    x = np.asarray(x, np.float32).astype(np.float64)
    s, a = x @ x.T, np.abs(x) @ np.abs(x).T
    lo, hi = (s - gs * a).astype(np.float32), (s + gs * a).astype(np.float32)
    pos, neg = class_masks(p, k)
    sure = _rmax(lo, neg) >= _rmin(hi, pos)
    may = _rmax(hi, neg) >= _rmin(lo, pos)
    return dict(sure=sure, may=may, open=sure != may)


# ---- the loss -----------------------------------------------------------------------------------------------------------------------
def reference(x, p, k, temperature=0.1, denominator="all"):
    """float64 loss, per-anchor losses, G and counts of an fp32 block x, with the intermediates bounds() reads."""
    assert denominator in DENOMINATORS, denominator
    tau = tau32(temperature)
    x = np.asarray(x, np.float32).astype(np.float64)
    n = p * k
    assert x.shape[0] == n and p >= 2 and k >= 2
    s = x @ x.T
    t = s / tau
    pos, neg = class_masks(p, k)
    off = ~np.eye(n, dtype=bool)
    kf = float(k - 1)
    out = dict(p=p, k=k, tau=tau, denominator=denominator, S=s, t=t,
               counts=np.array([n * (k - 1), violating(s.astype(np.float32), p, k).sum()], np.int64))
    if denominator == "all":
        m = _rmax(t, off)
        e = np.where(off, np.exp(np.where(off, t - m[:, None], 0.0)), 0.0)
        d = e.sum(1)
        ell = np.log(d) + np.where(pos, m[:, None] - t, 0.0).sum(1) / kf
        g = (e / d[:, None] - pos / kf) / tau
        out.update(M=m, e=e, d=d)
    else:
        mn = _rmax(t, neg)
        en = np.where(neg, np.exp(np.where(neg, t - mn[:, None], 0.0)), 0.0)
        big_e = en.sum(1)
        m = np.maximum(t, mn[:, None])
        a = np.where(pos, np.exp(np.where(pos, t - m, 0.0)), 0.0)
        b = np.where(pos, np.exp(np.where(pos, mn[:, None] - m, 0.0)), 0.0)
        dd = np.where(pos, a + b * big_e[:, None], 1.0)
        lp = np.where(pos, (m - t) + np.log(dd), 0.0)
        ell = lp.sum(1) / kf
        q = (b / dd).sum(1)
        g = (np.where(pos, a / dd - 1.0, 0.0) + en * q[:, None]) / (kf * tau)
        out.update(Mn=mn, en=en, En=big_e, m=m, a=a, b=b, D=dd, lp=lp, Q=q)
    out.update(ell=ell, loss=ell.sum() / n, G=g)
    return out


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def _rho(dz):
    return np.expm1(dz) + ULP_EXP_LOG * np.exp(dz)


def bounds(x, ref, gs):
    """-> (bound_G [N,N], bound_ell [N], bound_loss) for a device whose S is within gs A of the truth (module docstring)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    p, k, tau, t = ref["p"], ref["k"], ref["tau"], ref["t"]
    n = p * k
    it, kf = 1.0 / tau, float(k - 1)
    ck = 1.0 / kf
    pos, neg = class_masks(p, k)
    off = ~np.eye(n, dtype=bool)
    g2, g4 = float(gamma(2)), float(gamma(4))
    gn, gk = float(gamma(-(-n // 64) + 7)), float(gamma(-(-k // 64) + 7))
    dt = gs * (np.abs(x) @ np.abs(x).T) * it * (1.0 + g2) + g2 * np.abs(t)

    def dz_of(z, d1, d2):
        return d1 + d2 + U * (np.abs(z) + d1 + d2)

    if ref["denominator"] == "all":
        m, e, d = ref["M"], ref["e"], ref["d"]
        dm = np.where(off, dt, 0.0).max(1)[:, None]
        dz = dz_of(np.where(off, t - m[:, None], 0.0), dt, dm)
        rho = np.where(off, _rho(dz), 0.0)
        rho_d = ((rho * e).sum(1) / d * (1.0 + gn) + gn + n * 2.0 ** -126)[:, None]
        assert np.all(rho_d < 0.5), "the similarity error is too large for a meaningful bound"
        w = e / d[:, None]
        bw = w * ((rho + rho_d) / (1.0 - rho_d) * (1.0 + U) + U) + TINY
        v = w - ck * pos
        bv = np.where(pos, bw + U * ck + U * (np.abs(v) + bw + U * ck), bw)
        bound_g = np.where(off, it * ((1.0 + g2) * bv + g2 * np.abs(v)) + TINY, 0.0)
        h = np.where(pos, m[:, None] - t, 0.0)
        b_sum = np.where(pos, dz, 0.0).sum(1) * (1.0 + gk) + gk * h.sum(1)
        pm = h.sum(1) / kf
        b_pm = b_sum / kf * (1.0 + U) + U * pm
        lam = -np.log1p(-rho_d[:, 0])
        b_log = lam + ULP_EXP_LOG * (np.log(d) + lam)
        bound_ell = (b_log + b_pm) * (1.0 + U) + U * np.abs(ref["ell"])
    else:
        mn, en, big_e, m, a, b, dd, lp, q = (ref[key] for key in ("Mn", "en", "En", "m", "a", "b", "D", "lp", "Q"))
        dmn = np.where(neg, dt, 0.0).max(1)[:, None]
        rho_n = np.where(neg, _rho(dz_of(np.where(neg, t - mn[:, None], 0.0), dt, dmn)), 0.0)
        rho_e = ((rho_n * en).sum(1) / big_e * (1.0 + gn) + gn + n * 2.0 ** -126)[:, None]
        dm = np.maximum(dt, dmn)
        rho_a = _rho(dz_of(t - m, dt, dm))
        rho_b = _rho(dz_of(mn[:, None] - m, dmn, dm))
        be = b * big_e[:, None]
        rho_be = (1.0 + rho_b) * (1.0 + rho_e) * (1.0 + U) - 1.0
        rho_dd = np.where(pos, (rho_a * a + rho_be * be) / dd * (1.0 + U) + U + 3.0 * TINY, 0.0)
        assert np.all(rho_dd < 0.5), "the similarity error is too large for a meaningful bound"
        dh = dz_of(m - t, dm, dt)
        lam = -np.log1p(-rho_dd)
        b_lp = np.where(pos, (dh + lam + ULP_EXP_LOG * (np.log(dd) + lam)) * (1.0 + U) + U * lp, 0.0)
        bound_ell = (b_lp.sum(1) * (1.0 + gk) + gk * lp.sum(1)) / kf * (1.0 + U) + U * np.abs(ref["ell"])
        qv = np.where(pos, b / dd, 0.0)
        rho_q = (rho_b + rho_dd) / (1.0 - rho_dd) * (1.0 + U) + U
        b_q = ((np.where(pos, rho_q, 0.0) * qv).sum(1) * (1.0 + gk) + gk * q + k * TINY)[:, None]
        qq = q[:, None]
        b_neg = en * b_q + rho_n * en * (qq + b_q) + TINY * (qq + b_q + 1.0)
        bg_neg = ck * it * ((1.0 + g4) * (b_neg * (1.0 + U) + U * en * qq) + g4 * en * qq) + TINY
        y = np.where(pos, a / dd, 0.0)
        by = y * ((rho_a + rho_dd) / (1.0 - rho_dd) * (1.0 + U) + U) + TINY
        v = y - 1.0
        bv = by + U * (np.abs(v) + by)
        bg_pos = ck * it * ((1.0 + g4) * bv + g4 * np.abs(v)) + TINY
        bound_g = np.where(pos, bg_pos, np.where(neg, bg_neg, 0.0))
    bound_loss = bound_ell.sum() / n + (U + 2.0 ** -40) * abs(ref["loss"])
    return bound_g, bound_ell, bound_loss


# ---- the cases the CPU and the GPU test share -------------------------------------------------------------------------------------
MATRIX_SHAPES = [(4, 32, 64), (4, 4, 4096), (256, 8, 128)]
TRAP_TAU = 0.005


def underflow_trap(p=3):
    """One class with rows (1,0), (1,0), (0.2,0), the other classes on (0,1); with tau = 0.005 the logits of anchor 0 are 200 / 40 /
    0: under ONE maximum per anchor e^(40 - 200) and every e^(0 - 200) underflow in fp32 and the pair (0, 2) takes log 0.
    -> (x fp32 [3 p, 2], p, k)."""
    x = np.zeros((3 * p, 2), np.float32)
    x[:, 1] = 1.0
    x[:3] = [[1.0, 0.0], [1.0, 0.0], [0.2, 0.0]]
    return x, p, 3
