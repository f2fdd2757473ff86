"""float64 restatement of the FastAP and Smooth-AP losses (include/embnet.h, csrc/ap_loss.hip) and the a-priori rounding bounds their
kernels are held to.  NumPy only, no kernel code.  tests/test_ap_ref_cpu.py checks the restatement (autograd, a float32 emulation of
the rounding forms, hand cases) and the fitness of the GPU test's inputs; tests/test_ap_loss_gpu.py checks the kernels against it.

Semantics (the header's).  X [N, E] fp32, N = P K, rows c K .. c K + K - 1 are class c; S = X X^T.  P_i: the other rows of i's class,
N_i: the rows of other classes.  loss = sum_i l_i / N;  demb = (g / N)(G + G^T) X;  counts = {N (K-1), anchors with
max_n S_in >= min_p S_ip on the fp32 S}.
    'fast_ap'    bins = L, inv = L / 4;  u_ij = (2 - 2 S_ij) inv, l0 = floor(u), f = u - l0: 1 - f to bin l0, f to bin l0 + 1 of h+
                 (j in P_i) or h- (j in N_i), bins 0 .. L, anything else dropped.  Hp, Hn running sums, H = Hp + Hn.
                 F_i = sum_{H_l > 0} h+_l Hp_l / H_l,  l_i = 1 - F_i / (K-1);  b_l = h+_l Hp_l / H_l^2,  c_l = h+_l Hn_l / H_l^2,
                 A-_m = -sum_{l >= m} b_l,  A+_m = Hp_m / H_m + sum_{l >= m} c_l  (0 where H = 0 and outside 0 .. L),
                 G_ij = (2 inv / (K-1)) (A^c_{l0+1} - A^c_{l0}),  G_ii = 0.
    'smooth_ap'  tau ROUNDED TO fp32 (the C ABI takes a float); per positive p and column j not in {i, p}: z = (S_ij - S_ip) / tau,
                 s = sigma(z), s' = sigma'(z) / tau;  R_p = 1 + sum_{q in P_i} s_pq, Nn_p = sum_{n in N_i} s_pn, Q_p = R_p + Nn_p,
                 U_p, Tn_p the same sums of s';  l_i = 1 - (1/(K-1)) sum_p R_p / Q_p;
                 G_ij = (1/(K-1)) [sum_{p != j} s'_pj (j in P_i ? -Nn_p : R_p) / Q_p^2 + [j in P_i] (U_j Nn_j - R_j Tn_j) / Q_j^2].

Bounds.  u = 2^-24 (written UR below where u is taken), gamma(n) = n UR / (1 - n UR) (ms_ref.gamma).  Nothing is measured; the
rounding counts are read off ap_loss.hip and pair_loss.h.  TINY = 2^-125: a result below 2^-126 may be flushed.  Every function
below takes `unit` (the unit roundoff) so that the same bounds hold the float64 restatement itself to autograd at 2^-53.

  S.  |S~ - S| <= dS = gamma_S A, A_ij = sum_c |x_ic x_jc|, gamma_S = ms_ref.gamma_s(path, E) (pair_loss.h's staging; 0 on grid
      inputs).

  FastAP.
  u.  d~ = fl(2 - 2 S~) (2 S~ is exact), u~ = fl(d~ inv):  |u~ - u| <= Du = inv (2 dS + UR (|d| + 2 dS)) (1 + UR) + UR |u|;
      Du = 0 where gamma_S = 0 and both d and u are fp32 numbers (a rounding of a representable result is exact; on the grid
      inputs that is every pair).
  h.  A pair's weight in bin l is the pulse w_l(u) = max(0, 1 - |u - l|): continuous and 1-Lipschitz in u, whichever interval the
      device puts u~ in; fl(1 - f) adds UR.  So a pair moves each bin it can reach by at most e = Du + UR, and it can reach l0,
      l0 + 1, and l0 - 1 / l0 + 2 when f < Du / 1 - f < Du.  A bin is a chain of at most N additions in column order:
      Eh_l = sum_{pairs reaching l} e + gamma(N) (h_l + sum e).                                   [chain length N per bin]
  Hp, Hn.  chains of at most L + 1 additions:  EHp_l = sum_{m <= l} Eh+_m + gamma(L + 1) (Hp_l + sum Eh+);  H = fl(Hp + Hn):
      EH = EHp + EHn + UR (H + EHp + EHn).
  quotients x / H with H - EH > 0:  |x~/H~ - x/H| <= (Ex + (x/H) EH) / (H - EH), then one rounding.  rp = Hp/H, a = h+/H and
      rn = Hn/H lie in [0, 1] on the device as well (h+~ <= Hp~ <= H~ by monotone rounding of non-negative chains), so each
      error is capped at 1 (+ UR): this is the bound where H - EH <= 0 (the row's nearest pair sits within Du below a centre), the
      device's H~ may then be 0 with every quotient 0, which the cap covers.
      b = fl(a rp), c = fl(a rn), the bin's term of F = fl(h+ rp): products of bounded factors, E_xy = x Ey + y Ex + Ex Ey + UR (..);
      b, c capped at 1, the term of F at h+ + Eh+.
  A.  suffix chains of at most L + 1 additions: E_Sb_m = sum_{l >= m} Eb_l + gamma(L + 1)(Sb_m + sum Eb);  A- = -Sb;
      A+ = fl(rp_m + Sc_m): E = Erp_m + ESc_m + UR (A+ + Erp + ESc).
  G.  For a pair that is not OPEN the device's l0 is the reference's.  v = A_{l0+1} - A_{l0}: Ev = EA1 + EA0 + UR (|v| + EA1 + EA0);
      coef~ = fl(2 inv / (K-1)) = coef (1 + d):  |G~ - G| <= coef ((1 + gamma(2)) Ev + gamma(2) |v|) + TINY.    ABSOLUTE: A1 - A0 cancels.
      The amplification is coef = 2 inv / (K-1) = (2 / Delta) / (K-1).
  l.  F = butterfly sum of the 65 terms (one addition joins a lane's two bins, six more): gamma(8):
      EF = sum Ef (1 + gamma(8)) + gamma(8) F;  l = fl(1 - fl(F / (K-1))):  El = (EF / (K-1))(1 + UR) + UR F / (K-1) + UR |l|.
  open pairs.  Du > 0 and |u - round(u)| <= Du: the device may put u~ on the other side of the centre; the pair's own G_ij is then one of two
      values (open_pairs).  The histogram, the loss and every other pair's G stay within the bounds above.

  Smooth-AP.
  z.  r~ = fl(1 / tau), z~ = fl(fl(S~_ij - S~_ip) r~):  |z~ - z| <= Dz = ((dS_ij + dS_ip) / tau)(1 + gamma(3)) + gamma(3) |z|.
  t = e^{-|z|}: expf held to 3 ulp (ms_ref.ULP_EXP_LOG):  rho_t = expm1(Dz) + 6 UR e^{Dz}.
  iv = fl(1 / fl(1 + t~)):  rho_den = rho_t phi (1 + UR) + UR, phi = t / (1 + t) (phi = 1 where |z| <= Dz: the device may take the
      other branch, which is the same function e^z / (1 + e^z) of z~);  rho_iv = rho_den / (1 - rho_den)(1 + UR) + UR.
  w = fl(t~ iv~):  rho_w = (1 + rho_t)(1 + rho_iv)(1 + UR) - 1, + TINY.  s = iv or w:  rho_s = rho_w (the larger of the two).
  s' = fl(fl(r~ w~) iv~):  rho_s' = (1 + UR)(1 + rho_w)(1 + rho_iv)(1 + UR)^2 - 1, + (1/tau + 1) TINY.
  sums of non-negative terms over the columns: a lane adds at most ceil(N / 64) of them, the butterfly six times:
      gamma(ceil(N / 64) + 7) (ms_ref's count, one to spare):  E_sum = sum rho v (1 + g) + g sum v + N (flush).  [chain length N per rank]
  R = fl(1 + .), Q = fl(R + Nn) >= 1, iq = fl(1 / Q): rho_iq = (EQ / Q) / (1 - EQ / Q)(1 + UR) + UR.
  rq = fl(R iq);  wneg = fl(rq iq);  wpos = -fl(fl(Nn iq) iq);  own = fl(fl(fl(fl(U Nn) - fl(R Tn)) iq) iq): products and one
      difference, bounded as written in _smooth_bounds.
  G.  acc = a chain of K - 1 fma over the positives + one addition + one division:  with terms T_p = s'_pj w_p,
      E_T = s' Ew + |w| s' rho_s' + rho_s' s' Ew + (flush) and
      |G~ - G| <= (sum E_T + Eown + gamma(K + 1)(sum |T| + |own| + sum E_T + Eown)) / (K-1) (1 + UR) + TINY.  [chain length K-1]
      The amplification is 1 / tau, inside s'.  The true rows sum to zero: |sum_j G~_ij| <= sum_j bound_ij.
  l.  ap = butterfly sum of the rq: gamma(7);  l = fl(1 - fl(ap / (K-1))):  El = (Eap / (K-1))(1 + UR) + UR ap / (K-1) + UR |l|.
  loss (both).  The sum over anchors and the division by N are float64 on the device; the final cast adds UR |loss|:
      |loss~ - loss| <= mean_i El_i + (UR + 2^-40) |loss|.
  backward.  ms_ref.grad, from the DEVICE's own G.
"""
import numpy as np

from ms_ref import TINY, U, ULP_EXP_LOG, class_masks

LOSSES = ("fast_ap", "smooth_ap")
MAX_BINS = 64
SMOOTH_MAX_K = 65
OPEN_CAP = 0.01                                           # the share of off-diagonal pairs that may be open


def gamma(n, unit=U):
    n = np.asarray(n, np.float64) * unit
    assert np.all(n < 0.5)
    return n / (1.0 - n)


def tau32(temperature):
    """The temperature as the C ABI sees it."""
    return float(np.float32(temperature))


def violating(s32, p, k):
    """Anchors with max_n S_in >= min_p S_ip on an fp32 similarity matrix.  -> bool [N]."""
    s32 = np.asarray(s32, np.float32)
    pos, neg = class_masks(p, k)
    return np.where(neg, s32, -np.inf).max(1) >= np.where(pos, s32, np.inf).min(1)


# ---- FastAP -----------------------------------------------------------------------------------------------------------------------
def _scatter(n, nb, rows_ok, idx, w):
    """sum of w into [n, nb] at (row, idx) where rows_ok and 0 <= idx < nb."""
    ok = rows_ok & (idx >= 0) & (idx < nb)
    r = np.nonzero(ok)[0]
    return np.bincount(r * nb + idx[ok].astype(np.int64), weights=w[ok], minlength=n * nb).reshape(n, nb)


def _pad_lookup(a, idx):
    """a [N, L+1] = A_0 .. A_L, idx int [N, N] -> A_idx with 0 outside 0 .. L."""
    nb = a.shape[1]
    ok = (idx >= 0) & (idx < nb)
    return np.where(ok, np.take_along_axis(a, np.clip(idx, 0, nb - 1), 1), 0.0)


def _fast_ap(s, p, k, bins):
    n = p * k
    assert isinstance(bins, (int, np.integer)) and 2 <= bins <= MAX_BINS, bins
    nb = bins + 1
    inv = bins / 4.0
    pos, neg = class_masks(p, k)
    u = (2.0 - 2.0 * s) * inv
    l0f = np.floor(u)
    f = u - l0f
    l0 = np.clip(l0f, -3, nb + 2).astype(np.int64)
    hp = _scatter(n, nb, pos, l0, 1.0 - f) + _scatter(n, nb, pos, l0 + 1, f)
    hn = _scatter(n, nb, neg, l0, 1.0 - f) + _scatter(n, nb, neg, l0 + 1, f)
    cp, cn = np.cumsum(hp, 1), np.cumsum(hn, 1)
    h = cp + cn
    ok = h > 0
    hs = np.where(ok, h, 1.0)
    rp, rn, a = np.where(ok, cp / hs, 0.0), np.where(ok, cn / hs, 0.0), np.where(ok, hp / hs, 0.0)
    b, c, ft = a * rp, a * rn, hp * rp
    sb, sc = np.cumsum(b[:, ::-1], 1)[:, ::-1], np.cumsum(c[:, ::-1], 1)[:, ::-1]
    a_neg, a_pos = -sb, rp + sc
    big_f = ft.sum(1)
    kf = float(k - 1)
    ell = 1.0 - big_f / kf
    coef = 2.0 * inv / kf
    v_pos = _pad_lookup(a_pos, l0 + 1) - _pad_lookup(a_pos, l0)
    v_neg = _pad_lookup(a_neg, l0 + 1) - _pad_lookup(a_neg, l0)
    v = np.where(pos, v_pos, np.where(neg, v_neg, 0.0))
    return dict(bins=bins, inv=inv, u=u, l0=l0, f=f, hp=hp, hn=hn, Hp=cp, Hn=cn, H=h, rp=rp, rn=rn, a=a, b=b, c=c, ft=ft, Sb=sb, Sc=sc,
                A_pos=a_pos, A_neg=a_neg, F=big_f, v=v, coef=coef, ell=ell, G=coef * v)


# ---- Smooth-AP --------------------------------------------------------------------------------------------------------------------
def _members(p, k):
    """For class member m: -> (valid [N]: m is not the anchor itself, jp [N]: the member's column) per m."""
    n = p * k
    rows = np.arange(n)
    lo, ai = rows // k * k, rows % k
    for m in range(k):
        yield m, ai != m, lo + m


def _sigmoid(z, it):
    """-> (t, sigma(z), sigma'(z) / tau) without 1 - sigma."""
    t = np.exp(-np.abs(z))
    den = 1.0 + t
    return t, np.where(z >= 0, 1.0 / den, t / den), it * t / (den * den)


def _smooth_ap(s, p, k, tau):
    n = p * k
    assert k <= SMOOTH_MAX_K
    it, kf = 1.0 / tau, float(k - 1)
    pos, neg = class_masks(p, k)
    rows = np.arange(n)
    shape = (n, k)
    big_r, big_n, big_u, big_t = np.ones(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for m, valid, jp in _members(p, k):
        z = (s - s[rows, jp][:, None]) * it
        _, sg, dsg = _sigmoid(z, it)
        keep = np.ones((n, n), bool)
        keep[rows, jp] = False
        kp, kn = pos & keep, neg
        big_r[:, m] = 1.0 + np.where(kp, sg, 0.0).sum(1)
        big_n[:, m] = np.where(kn, sg, 0.0).sum(1)
        big_u[:, m] = np.where(kp, dsg, 0.0).sum(1)
        big_t[:, m] = np.where(kn, dsg, 0.0).sum(1)
    q = big_r + big_n
    is_pos = np.arange(k)[None, :] != (rows % k)[:, None]              # [N, K]: member m is a positive of anchor i
    rq = np.where(is_pos, big_r / q, 0.0)
    wneg = np.where(is_pos, big_r / q ** 2, 0.0)
    wpos = np.where(is_pos, -big_n / q ** 2, 0.0)
    own = np.where(is_pos, (big_u * big_n - big_r * big_t) / q ** 2, 0.0)
    acc, mag = np.zeros((n, n)), np.zeros((n, n))
    for m, valid, jp in _members(p, k):
        z = (s - s[rows, jp][:, None]) * it
        _, _, dsg = _sigmoid(z, it)
        w = np.where(pos, wpos[:, m][:, None], np.where(neg, wneg[:, m][:, None], 0.0))
        w[rows, jp] = 0.0
        w[~valid] = 0.0
        acc += dsg * w
        mag += np.abs(dsg * w)
        acc[rows[valid], jp[valid]] += own[valid, m]
        mag[rows[valid], jp[valid]] += np.abs(own[valid, m])
    ell = 1.0 - rq.sum(1) / kf
    return dict(tau=tau, R=big_r, Nn=big_n, U=big_u, Tn=big_t, Q=q, is_pos=is_pos, rq=rq, wneg=wneg, wpos=wpos, own=own, acc=acc, mag=mag,
                ell=ell, G=acc / kf)


def reference(x, p, k, loss, **params):
    """float64 loss, per-anchor losses (ell), G and counts of an fp32 block x, with the intermediates bounds() reads; for 'fast_ap'
    (bins=10) the u of every pair as well; 'smooth_ap' takes temperature=0.01."""
    assert loss in LOSSES, loss
    x = np.asarray(x, np.float32).astype(np.float64)
    n = p * k
    assert x.shape[0] == n and p >= 2 and k >= 2
    s = x @ x.T
    if loss == "fast_ap":
        out = _fast_ap(s, p, k, params.pop("bins", 10))
    else:
        out = _smooth_ap(s, p, k, tau32(params.pop("temperature", 0.01)))
    assert not params, params
    out.update(p=p, k=k, kind=loss, S=s, loss=out["ell"].sum() / n,
               counts=np.array([n * (k - 1), violating(s.astype(np.float32), p, k).sum()], np.int64))
    return out


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def _du(x, ref, gs, unit):
    ds = gs * (np.abs(x) @ np.abs(x).T)
    d = 2.0 - 2.0 * ref["S"]
    du = ref["inv"] * (2.0 * ds + unit * (np.abs(d) + 2.0 * ds)) * (1.0 + unit) + unit * np.abs(ref["u"])
    if gs == 0.0 and unit == U:                           # S~ = S: a rounding whose exact result is an fp32 number commits no error
        with np.errstate(over="ignore"):
            exact = (d.astype(np.float32).astype(np.float64) == d) & (ref["u"].astype(np.float32).astype(np.float64) == ref["u"])
        du = np.where(exact, 0.0, du)
    return du


def open_pairs(x, p, k, bins, gs, unit=U):
    """FastAP's pairs whose u lies within Du of a whole number: the device may put them in the neighbouring interval.
    -> bool [N, N] (the diagonal False)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    ref = dict(S=x @ x.T, inv=bins / 4.0)
    ref["u"] = (2.0 - 2.0 * ref["S"]) * ref["inv"]
    du = _du(x, ref, gs, unit)
    return (du > 0) & (np.abs(ref["u"] - np.round(ref["u"])) <= du) & ~np.eye(p * k, dtype=bool)


def _quot(xv, ex, h, eh, unit):
    """|fl(x~ / H~) - x / H| for 0 <= x <= H, both quotients in [0, 1]: first order where H - EH > 0, capped at 1."""
    safe = h - eh > 0
    den = np.where(safe, h - eh, 1.0)
    q = np.where(h > 0, xv / np.where(h > 0, h, 1.0), 0.0)
    first = (ex + q * eh) / den
    capped = np.where(safe, np.minimum(first + unit * (q + first), 1.0 + unit), 1.0 + unit)
    return np.where((h == 0) & (eh == 0), 0.0, capped)     # a bin nothing can reach is empty on the device too


def _prod(a, ea, b, eb, unit):
    e = a * eb + b * ea + ea * eb
    return e + unit * (a * b + e)


def _fast_bounds(x, ref, gs, unit):
    p, k, nb = ref["p"], ref["k"], ref["bins"] + 1
    n = p * k
    pos, neg = class_masks(p, k)
    du = _du(x, ref, gs, unit)
    e = du + unit
    l0, f = ref["l0"], ref["f"]
    g_n, g_l, g2, g8 = (float(gamma(v, unit)) for v in (n, nb, 2, 8))

    def reach(mask):
        tot = _scatter(n, nb, mask, l0, e) + _scatter(n, nb, mask, l0 + 1, e)
        tot += _scatter(n, nb, mask & (f < du), l0 - 1, e) + _scatter(n, nb, mask & (1.0 - f < du), l0 + 2, e)
        return tot

    ehp, ehn = reach(pos), reach(neg)
    ehp, ehn = ehp + g_n * (ref["hp"] + ehp), ehn + g_n * (ref["hn"] + ehn)
    chp, chn = np.cumsum(ehp, 1), np.cumsum(ehn, 1)
    e_hp, e_hn = chp + g_l * (ref["Hp"] + chp), chn + g_l * (ref["Hn"] + chn)
    h = ref["H"]
    e_h = e_hp + e_hn + unit * (h + e_hp + e_hn)
    e_rp = _quot(ref["Hp"], e_hp, h, e_h, unit)
    e_rn = _quot(ref["Hn"], e_hn, h, e_h, unit)
    e_a = _quot(ref["hp"], ehp, h, e_h, unit)
    e_b = np.minimum(_prod(ref["a"], e_a, ref["rp"], e_rp, unit), 1.0 + 3.0 * unit)
    e_c = np.minimum(_prod(ref["a"], e_a, ref["rn"], e_rn, unit), 1.0 + 3.0 * unit)
    e_ft = np.minimum(_prod(ref["hp"], ehp, ref["rp"], e_rp, unit), (ref["hp"] + ehp) * (1.0 + 3.0 * unit))

    def suffix(v):
        return np.cumsum(v[:, ::-1], 1)[:, ::-1]

    e_sb, e_sc = suffix(e_b), suffix(e_c)
    e_an = e_sb + g_l * (ref["Sb"] + e_sb)
    e_sc = e_sc + g_l * (ref["Sc"] + e_sc)
    e_ap = e_rp + e_sc + unit * (ref["A_pos"] + e_rp + e_sc)
    ea = np.where(pos, _pad_lookup(e_ap, l0 + 1) + _pad_lookup(e_ap, l0), _pad_lookup(e_an, l0 + 1) + _pad_lookup(e_an, l0))
    v = np.abs(ref["v"])
    ev = ea + unit * (v + ea)
    bound_g = np.where(pos | neg, ref["coef"] * ((1.0 + g2) * ev + g2 * v) + TINY, 0.0)
    kf = float(k - 1)
    e_f = e_ft.sum(1) * (1.0 + g8) + g8 * ref["F"]
    bound_ell = e_f / kf * (1.0 + unit) + unit * ref["F"] / kf + unit * np.abs(ref["ell"])
    return bound_g, bound_ell, dict(Du=du, Eh_pos=ehp, Eh_neg=ehn, EH=e_h)


def _smooth_bounds(x, ref, gs, unit):
    p, k, tau, s = ref["p"], ref["k"], ref["tau"], ref["S"]
    n = p * k
    it, kf = 1.0 / tau, float(k - 1)
    pos, neg = class_masks(p, k)
    rows = np.arange(n)
    ds = gs * (np.abs(x) @ np.abs(x).T)
    ulp = ULP_EXP_LOG * unit / U
    g3, g7, gn, gk = (float(gamma(v, unit)) for v in (3, 7, -(-n // 64) + 7, k + 1))
    flush = TINY if unit == U else 0.0

    def pieces(jp):
        z = (s - s[rows, jp][:, None]) * it
        dz = (ds + ds[rows, jp][:, None]) * it * (1.0 + g3) + g3 * np.abs(z)
        t, sg, dsg = _sigmoid(z, it)
        rho_t = np.expm1(dz) + ulp * np.exp(dz)
        phi = np.where(np.abs(z) <= dz, 1.0, t / (1.0 + t))
        rho_den = rho_t * phi * (1.0 + unit) + unit
        assert np.all(rho_den < 0.5), "the similarity error is too large for a meaningful bound"
        rho_iv = rho_den / (1.0 - rho_den) * (1.0 + unit) + unit
        rho_w = (1.0 + rho_t) * (1.0 + rho_iv) * (1.0 + unit) - 1.0
        rho_d = (1.0 + unit) ** 3 * (1.0 + rho_w) * (1.0 + rho_iv) - 1.0
        return sg, dsg, rho_w, rho_d

    shape = (n, k)
    e_r, e_n, e_u, e_t = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for m, valid, jp in _members(p, k):
        sg, dsg, rho_w, rho_d = pieces(jp)
        keep = np.ones((n, n), bool)
        keep[rows, jp] = False
        kp = pos & keep

        def esum(mask, v, rho, fl):
            tot = np.where(mask, v, 0.0).sum(1)
            return np.where(mask, rho * v, 0.0).sum(1) * (1.0 + gn) + gn * tot + n * fl

        e_r[:, m] = esum(kp, sg, rho_w, flush)
        e_n[:, m] = esum(neg, sg, rho_w, flush)
        e_u[:, m] = esum(kp, dsg, rho_d, (it + 1.0) * flush)
        e_t[:, m] = esum(neg, dsg, rho_d, (it + 1.0) * flush)
    big_r, big_n, big_u, big_t, q = ref["R"], ref["Nn"], ref["U"], ref["Tn"], ref["Q"]
    e_r = e_r + unit * (big_r + e_r)                                  # R = fl(1 + .)
    e_q = e_r + e_n + unit * (q + e_r + e_n)
    assert np.all(e_q / q < 0.5)
    rho_iq = (e_q / q) / (1.0 - e_q / q) * (1.0 + unit) + unit
    iq = 1.0 / q
    e_iq = iq * rho_iq
    e_rq = _prod(big_r, e_r, iq, e_iq, unit)
    e_wneg = _prod(big_r * iq, e_rq, iq, e_iq, unit) + flush
    e_niq = _prod(big_n, e_n, iq, e_iq, unit) + flush
    e_wpos = _prod(big_n * iq, e_niq, iq, e_iq, unit) + flush
    e_un = _prod(big_u, e_u, big_n, e_n, unit) + flush
    e_rt = _prod(big_r, e_r, big_t, e_t, unit) + flush
    diff = np.abs(big_u * big_n - big_r * big_t)
    e_diff = e_un + e_rt + unit * (diff + e_un + e_rt)
    e_d1 = _prod(diff, e_diff, iq, e_iq, unit) + flush
    e_own = _prod(diff * iq, e_d1, iq, e_iq, unit) + flush
    is_pos = ref["is_pos"]
    e_rq, e_wneg, e_wpos, e_own = (np.where(is_pos, v, 0.0) for v in (e_rq, e_wneg, e_wpos, e_own))
    e_acc = np.zeros((n, n))
    for m, valid, jp in _members(p, k):
        _, dsg, _, rho_d = pieces(jp)
        w = np.where(pos, np.abs(ref["wpos"][:, m])[:, None], np.where(neg, ref["wneg"][:, m][:, None], 0.0))
        ew = np.where(pos, e_wpos[:, m][:, None], np.where(neg, e_wneg[:, m][:, None], 0.0))
        et = dsg * ew + w * dsg * rho_d + rho_d * dsg * ew + (it + 1.0) * flush * (w + ew) + flush
        et[rows, jp] = 0.0
        et[~valid] = 0.0
        e_acc += et
        e_acc[rows[valid], jp[valid]] += e_own[valid, m]
    bound_g = np.where(pos | neg, (e_acc + gk * (ref["mag"] + e_acc)) / kf * (1.0 + unit) + flush, 0.0)
    ap = ref["rq"].sum(1)
    e_ap = e_rq.sum(1) * (1.0 + g7) + g7 * ap
    bound_ell = e_ap / kf * (1.0 + unit) + unit * ap / kf + unit * np.abs(ref["ell"])
    return bound_g, bound_ell, dict(EQ=e_q, ER=e_r)


def bounds(x, ref, gamma_s, unit=U):
    """-> (bound_G [N,N], bound_ell [N], bound_loss, extras) for a device whose S is within gamma_s A of the truth and whose unit
    roundoff is `unit` (module docstring).  For 'fast_ap' bound_G holds for the pairs that are not open (open_pairs), and extras
    has the histogram-propagated bounds Eh_pos / Eh_neg [N, L+1], EH and Du; for 'smooth_ap' sum_j bound_G[i, j] bounds |sum_j G~_ij|."""
    x = np.asarray(x, np.float32).astype(np.float64)
    fn = _fast_bounds if ref["kind"] == "fast_ap" else _smooth_bounds
    bound_g, bound_ell, extras = fn(x, ref, gamma_s, unit)
    bound_loss = bound_ell.sum() / ref["ell"].size + (unit + 2.0 ** -40 * unit / U) * abs(ref["loss"])
    return bound_g, bound_ell, bound_loss, extras


# ---- the inputs the CPU and the GPU test share ------------------------------------------------------------------------------------
def negated_odd_classes(x, k):
    """x with the rows of every odd class negated: d = 2 - 2 S spans to about 3.8 and FastAP's top bins fill."""
    x = np.array(x, np.float32)
    cls = np.arange(x.shape[0]) // k
    x[cls % 2 == 1] *= np.float32(-1.0)
    return x


def antipodal_rows(x, k):
    """x with the first row of every odd class replaced by the unit row along 0.05 (itself) - (the first row of the class before):
    that pair has S about -0.99 and d about 3.98, which at L = 64 lies between the centres 63 and 64: the last bin fills."""
    x = np.array(x, np.float64)
    for lo in range(k, x.shape[0], 2 * k):
        v = 0.05 * x[lo] - x[lo - k]
        x[lo] = v / np.linalg.norm(v)
    return x.astype(np.float32)


def scaled_rows(x, k, norm=1.5):
    """x with the rows of every odd class negated and every second row brought to `norm` times its length: for unit rows the
    pairs of two long rows of a class have d = 2 - 2 S below 0, those of long rows of opposite classes d above 4, and the rest
    stays inside, so the histograms are neither empty nor complete."""
    x = negated_odd_classes(x, k)
    x[1::2] *= np.float32(norm)
    return x


# FastAP's inputs by kind, for both test files: -> (x fp32 [N, E], the grid's unit or None).  The clustered rows of
# recipes.clustered_embeddings are non-negative unit rows: d lies in about [0.2, 1.2].
SIGMA = 0.8
SHAPES = [(2, 2, 5), (4, 3, 1), (5, 7, 33), (16, 2, 48), (3, 16, 40), (8, 4, 256), (4, 32, 64), (64, 4, 512), (256, 8, 128)]
RANGE_SHAPES = [(5, 7, 33), (8, 4, 256)]
CONTINUOUS_BINS = (2, 7, 16, 64)                          # with 10: a dyadic spacing meets the dyadic grid, so not on grid inputs
DUPLICATE_SHAPE = (5, 4, 32)


def make_input(kind, p, k, e):
    import ms_ref
    import recipes
    seed = ms_ref.seed_of(p, k, e)
    if kind == "duplicates":
        x, _, q = ms_ref.grid_inputs(recipes.clustered_embeddings(8, p, k, e, SIGMA))
        x = x.copy()
        x[1::k] = x[0::k]                                 # rows 0 and 1 of every class coincide
        return x, 1.0 / q
    x = recipes.clustered_embeddings(seed, p, k, e, SIGMA)
    if kind == "grid":
        x, _, q = ms_ref.grid_inputs(x)
        return x, 1.0 / q
    if kind == "negated":
        return negated_odd_classes(x, k), None
    if kind == "scaled":
        return scaled_rows(x, k), None
    if kind == "antipodal":
        return antipodal_rows(x, k), None
    assert kind == "continuous", kind
    return x, None


def fast_ap_cases():
    """(kind, (p, k, e), bins) of every FastAP value check of tests/test_ap_loss_gpu.py."""
    out = [("grid", s, 10) for s in SHAPES]
    out += [("continuous", s, 10) for s in SHAPES if s[2] > 1]         # E = 1: every row is (1), every pair on the centre 0
    out += [("continuous", s, b) for s in RANGE_SHAPES for b in CONTINUOUS_BINS]
    out += [(kind, s, 10) for kind in ("negated", "scaled") for s in RANGE_SHAPES]
    out += [("antipodal", s, 64) for s in RANGE_SHAPES]
    out += [("duplicates", DUPLICATE_SHAPE, 10)]
    return out


def paths_of(p, k, e):
    """The forward paths a shape is run on: both where the per-class path fits a small shape, `auto` otherwise."""
    import ms_ref
    if ms_ref.auto_path(p, k, e) != "per_class":
        return ["similarity_matrix"]
    return ["per_class", "similarity_matrix"] if p * k <= 64 else ["auto"]
