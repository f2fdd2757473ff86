"""float64 restatement of SoftTriple and sub-centre ArcFace (include/embnet.h, csrc/multi_proxy_loss.hip) and the a-priori rounding
bounds their kernels are held to.  NumPy only, no kernel code.  tests/test_multi_proxy_ref_cpu.py checks the restatement (autograd,
differences, hand cases) and the fitness of the GPU test's inputs; tests/test_multi_proxy_loss_gpu.py checks the kernels against it.

Semantics (the header's).  X [n, e], W [c kc, e] fp32 class-major, y [n] labels (outside [0, c): unlabelled).  q, D, S = D q as in
proxy_ref over the nb = c kc rows.  The scalar parameters ROUNDED TO fp32.
    pooling    'arcface': S' = max_j S_j, the weight on the FIRST j that attains it;  'soft_triple': p = softmax_j(S_j / gamma),
               S' = sum_j p_j S_j, dS'/dS_j = p_j (1 + (S_j - S') / gamma);  kc = 1: S' = S.
    logits     'soft_triple': t = lambda (S' - delta [c' = y]);  'arcface': t = s S' off the own class and s phi(S'_y) on it, with
               cm, sm, th = cos(pi - m), mm = sin(pi - m) m computed in float64 and rounded to fp32;  S' > th: r = sqrt(max(0, 1 - S'^2)),
               phi = S' cm - r sm, phi' = cm + S' sm / max(r, 2^-10) (cm where r = 0);  S' <= th: phi = S' - mm, phi' = 1.
    loss       M = max t, d = sum e^(t - M), l_i = log d + (M - t_y), loss = sum l_i / n_l + R;
               G [n, c kc] = (scale / n_l)(e^(t - M) / d - [c' = y]) psi dS'/dS_j, psi = phi' on ArcFace's own class, 1 elsewhere.
    reg        g_st = q_s q_t w_s . w_t;  coef = tau / (c kc (kc - 1));  R = coef sum_c' sum_{s<t} sqrt(max(0, 2 + 1e-5 - 2 g_st));
               H_st = H_ts = -coef / sqrt(2 + 1e-5 - 2 g_st);  'soft_triple' with kc > 1 and tau > 0 only.
    counts     = {n_l, violating samples max_{c' != y} S' >= S'_y, own-class lower-branch samples S'_y <= th} on the fp32 values.
    Q = q G;  demb = g Q W;  Y_r = sum_i G_ir x_i + sum_{t != r, same class} H_rt q_t w_t;  dW_r = g q_r (Y_r - q_r^2 (Y_r . w_r) w_r).

Bounds.  u = 2^-24, gamma(n) = n u / (1 - n u), ULP_EXP_LOG = 6 u for expf / logf, TINY = 2^-125 for a flushed result (ms_ref,
proxy_ref).  Nothing is measured; the rounding counts are read off multi_proxy_loss.hip.

  q, S.  proxy_ref's: q is reproduced bit for bit, |S~ - S| <= dS = gamma_S A q (1 + u) + u |S|, gamma_S by the path.
  S'.  'arcface': the maximum is 1-Lipschitz and the device's maximum is some member's S~:  dS' = max_j dS_j.
       'soft_triple': z~ = fl(S~ / gamma): dz = dS / gamma (1 + u) + u |z|;  zm: dzm = max_j dz_j;  v = z - zm:
       dv = dz + dzm + u (|v| + dz + dzm);  x = exp(v): E_j = x_j (expm1(dv) + 6 u exp(dv)) + TINY absolute;  den: kc additions,
       gk = gamma(kc + 1): d_den = sum E (1 + gk) + gk den;  num: a chain of kc fma over x~ S~.  With theta, theta' <= gk the chains'
       relative errors,  num~ / den~ - S' = [sum x~_j (S_j - S') + sum x~_j (S~_j - S_j) + sum x~_j S~_j theta_j - S' sum x~_j theta'_j] / den~,
       and sum x_j (S_j - S') = 0: the errors of x weigh the DEVIATIONS S_j - S', not |S_j| (rows of norm 30 stay bounded):
       d_num = sum [E_j |S_j - S'| + (x_j + E_j) dS_j + gk (x_j + E_j)(|S_j| + dS_j)] + gk |S'| sum (x_j + E_j);  S' = fl(num / den):
       dS' = d_num / (den - d_den) (1 + u) + u |S'| + TINY  (den >= 1).        kc = 1: dS' = dS.
  phi.  S' > th surely (S' - dS' > th):  A = 1 - S'^2, A~ = fl(1 - fl(S~'^2)): dA = (2 |S'| dS' + dS'^2)(1 + 2u) + u (S'^2 + |A|) + u dA;
       r~ is the correctly rounded root of max(0, A~): both r and r~ lie in [r_lo, r_hi (1 + u)], r_lo / r_hi = sqrt(max(0, A -/+ dA)):
       dr = r_hi - r_lo + u r_hi.  phi~ = fl(fl(S~' cm) - fl(r~ sm)):
       dphi = (cm dS' + sm dr)(1 + 2 u) + u (|S' cm| + r sm) + u |phi|: the slope |phi'| at the unfavourable end of the interval
       is what r_hi - r_lo amounts to.  S' <= th surely:  dphi = dS' (1 + u) + u |phi|.  Neither: the branch is OPEN.
  psi.  A + dA <= 0: r~ = r = 0, psi = cm exactly.  r_lo > 2^-10:  the quotient S' sm / r over the interval:
       dpsi = (sm dS'(1 + u) + u |S' sm|) / r_lo + |S' sm| (1 / r_lo - 1 / (r_hi (1 + u))) + 2 u |psi|.  Anything else is the floor band:
       the contract's phi' jumps at r = 0 and bends at the floor, no bound is stated there (bounds() refuses such inputs).
  t.  Dt = a dS' (1 + gamma(2)) + gamma(2) |t|; on ArcFace's own class a dphi (1 + u) + u |t|.  M, z, e, d, w = e / d, v = w - [c' = y],
      l_i: proxy_ref's CosFace bounds with c columns (L = ceil(c / 64) + 7).
  base = fl(k~ v~), k~ = fl(a / n_l):  B = (a / n_l)((1 + gamma(2)) Bv + gamma(2) |v|) + TINY;  times psi~ on ArcFace's own class:
      B' = B (|psi| + dpsi) + |base| dpsi + u |base psi| + TINY.
  G.  'arcface': base on the argmax, EXACTLY 0 on the others: bound B' there, 0 elsewhere.  The argmax is the device's own where the
      two largest S of the class are more than 2 max_j dS_j apart; otherwise the cell is OPEN and only sum_j G_j is compared (bound B').
      'soft_triple': p_j = fl(x~_j / den~): dp = p ((E_j / x_j + rd) / (1 - rd)(1 + u) + u) + TINY, rd = d_den / den;
      h = 1 + (S_j - S') / gamma: dh = ((dS_j + dS')(1 + gamma(3)) / gamma + gamma(2) |h - 1|)(1 + u) + u |h|;  F = fl(p h):
      dF = dp (|h| + dh) + p dh + u |F| + TINY;  G = fl(base F): dG = B (|F| + dF) + |base| dF + u |G| + TINY.
  loss.  |loss~ - loss| <= sum B_l / n_l + dR + (2 u + 2^-40) |loss|.
  reg.  float64 throughout on exact products: g = q q acc: dg = (e + 4) 2^-53 q_s q_t sum_k |w_sk w_tk|;  arg = 2 + 1e-5 - 2 g:
      darg = 2 dg + 2^-51;  a term: dterm = darg / (2 sqrt(arg - darg)) + 2^-52 term;  R: the sums add (pairs + c + 8) 2^-53 relative,
      the cast u:  dR = coef sum dterm + ((pairs + c + 8) 2^-53 + u) R + 2^-149.   H: dH = |H| (darg / (2 (arg - darg)) + 2^-51 + u) + 2^-149.
  backward, against float64 of the DEVICE's own G, q and H:  proxy_ref.grads' bounds with c := c kc, the regulariser's kc more terms
      in Y's chain and sum_t |H_rt| q_t |w_t| in Ya.

Decisions.  The device's S'~ lies in [S' - dS', S' + dS']: a sample surely violates when it does at the unfavourable ends, possibly
when it does at the favourable ends, OPEN when the two differ; likewise the lower branch against th.
"""
import math

import numpy as np

import proxy_ref as P
from ms_ref import TINY, U, ULP_EXP_LOG, gamma

KINDS = ("soft_triple", "arcface")
DEFAULTS = {"soft_triple": dict(a=20.0, b=0.01, gamma=0.1, tau=0.2), "arcface": dict(a=64.0, b=0.5, gamma=1.0, tau=0.0)}
MAX_N, MAX_NB, MAX_E, MAX_KC = 4096, 16384, 4096, 32
R_FLOOR = 2.0 ** -10
REG_EPS = 1e-5


# ---- path rule, workspace (embnet_multi_proxy_loss_path / _workspace_bytes restated) ------------------------------------------------
def in_range(n, c, kc, e):
    return 2 <= n <= MAX_N and 2 <= c and 1 <= kc <= MAX_KC and c * kc <= MAX_NB and 1 <= e <= MAX_E


def fits_small(n, c, kc, e):
    """Whether the small path may be forced."""
    return in_range(n, c, kc, e) and e + c * kc <= 4096 and n * c * kc * e <= 2 ** 25


def auto_path(n, c, kc, e):
    """'small' | 'matrix'; None outside the range.  `auto` takes the small path where it fits and there are fewer than 100 centres."""
    if not in_range(n, c, kc, e):
        return None
    return "small" if fits_small(n, c, kc, e) and c * kc < 100 else "matrix"


def workspace_bytes(n, c, kc, e):
    if not in_range(n, c, kc, e):
        return 0
    a16 = lambda b: (b + 15) // 16 * 16
    return 16 + a16(8 * n) + 16 * n + a16(8 * c) + a16(4 * c * kc * n) + a16(8 * c * kc * e)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(x, p, k, c, kc, seed, centre_sigma=0.5):
    """A class-contiguous block x [p k, e] -> (x, w fp32 [c kc, e], labels int32 [p k]): labels as proxy_ref.make_inputs; each present
    class's kc centres are its members' normalised mean plus centre_sigma randn / sqrt(e) per centre, the others |randn|; every row is
    rescaled by a factor in [0.5, 3]."""
    e = x.shape[1]
    _, _, labels = P.make_inputs(x, p, k, c, seed)
    r = np.random.RandomState(seed + 7)
    w = np.abs(r.randn(c, kc, e))
    x64 = x.astype(np.float64)
    for cl in np.unique(labels):
        cent = x64[labels == cl].mean(0)
        w[cl] = cent / np.linalg.norm(cent) + centre_sigma * r.randn(kc, e) / np.sqrt(e)
    w *= r.uniform(0.5, 3.0, size=(c, kc, 1))
    return x, w.reshape(c * kc, e).astype(np.float32), labels


def ragged_inputs(x5, e, c, kc, seed):
    """proxy_ref.ragged_inputs' 17 rows and labels, with kc centres per class (a present class's around its members' mean)."""
    x, _, lab = P.ragged_inputs(x5, e, c, seed)
    r = np.random.RandomState(seed + 9)
    w = np.abs(r.randn(c, kc, e))
    for cl in np.unique(lab[(lab >= 0) & (lab < c)]):
        cent = x[lab == cl].astype(np.float64).mean(0)
        w[cl] = cent / np.linalg.norm(cent) + 0.5 * r.randn(kc, e) / np.sqrt(e)
    w *= r.uniform(0.5, 3.0, size=(c, kc, 1))
    return x, w.reshape(c * kc, e).astype(np.float32), lab


# ---- parameters -----------------------------------------------------------------------------------------------------------------------
def params32(kind, a=None, b=None, gam=None, tau=None):
    """-> dict(a, b, gamma, tau) rounded to fp32, and for 'arcface' cm, sm, th, mm as the host computes them."""
    d = DEFAULTS[kind]
    f = lambda v, dv: float(np.float32(dv if v is None else v))
    out = dict(a=f(a, d["a"]), b=f(b, d["b"]), gamma=f(gam, d["gamma"]), tau=f(tau, d["tau"]))
    if kind == "arcface":
        m = out["b"]
        out.update(cm=float(np.float32(math.cos(m))), sm=float(np.float32(math.sin(m))), th=float(np.float32(math.cos(math.pi - m))),
                   mm=float(np.float32(math.sin(math.pi - m) * m)))
    return out


def phi_of(sp, pr):
    """-> (phi, phi', r, upper) of the own-class pooled similarity; the branch on the fp32 rounding of sp."""
    sp = np.asarray(sp, np.float64)
    upper = sp.astype(np.float32) > np.float32(pr["th"])
    r = np.sqrt(np.maximum(0.0, 1.0 - sp * sp))
    phi = np.where(upper, sp * pr["cm"] - r * pr["sm"], sp - pr["mm"])
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = np.where(r == 0, pr["cm"], pr["cm"] + sp * pr["sm"] / np.maximum(r, R_FLOOR))
    return phi, np.where(upper, slope, 1.0), r, upper


# ---- the regulariser --------------------------------------------------------------------------------------------------------------------
def regulariser(w, c, kc, tau, q=None):
    """-> dict(R, H [c, kc, kc], dR, dH) (module docstring); zeros without a regulariser."""
    w = np.asarray(w, np.float32).astype(np.float64)
    e = w.shape[1]
    q = (P.q_of(w) if q is None else np.asarray(q, np.float32)).astype(np.float64)
    h = np.zeros((c, kc, kc))
    if kc == 1 or tau == 0:
        return dict(R=0.0, H=h, dR=0.0, dH=np.zeros_like(h))
    coef = tau / (c * kc * (kc - 1))
    w3, q3 = w.reshape(c, kc, e), q.reshape(c, kc)
    qq = q3[:, :, None] * q3[:, None, :]
    g = qq * np.einsum("cse,cte->cst", w3, w3)
    dg = (e + 4) * 2.0 ** -53 * qq * np.einsum("cse,cte->cst", np.abs(w3), np.abs(w3))
    arg = 2.0 + REG_EPS - 2.0 * g
    darg = 2.0 * dg + 2.0 ** -51
    assert np.all(arg - darg > 0)
    up = np.triu(np.ones((kc, kc), bool), 1)[None]
    term = np.where(up, np.sqrt(np.maximum(arg, 0.0)), 0.0)
    dterm = np.where(up, darg / (2.0 * np.sqrt(arg - darg)) + 2.0 ** -52 * term, 0.0)
    off = ~np.eye(kc, dtype=bool)[None]
    h = np.where(off, -coef / np.sqrt(arg), 0.0)
    reg = coef * term.sum()
    pairs = kc * (kc - 1) // 2
    d_r = coef * dterm.sum() + ((pairs + c + 8) * 2.0 ** -53 + U) * reg + 2.0 ** -149
    d_h = np.where(off, np.abs(h) * (darg / (2.0 * (arg - darg)) + 2.0 ** -51 + U) + 2.0 ** -149, 0.0)
    return dict(R=reg, H=h, dR=d_r, dH=d_h)


# ---- the losses -----------------------------------------------------------------------------------------------------------------------
def reference(kind, x, w, labels, c, a=None, b=None, gam=None, tau=None, q=None):
    """float64 loss, reg, G [n, c kc] and counts, with the intermediates bounds() reads."""
    assert kind in KINDS, kind
    pr = params32(kind, a, b, gam, tau)
    s, aq, q = P.similarity(x, w, q)
    n, nb = s.shape
    kc = nb // c
    assert nb == c * kc
    pos, labelled = P.masks(labels, c)
    nl = int(labelled.sum())
    s3 = s.reshape(n, c, kc)
    s32 = s3.astype(np.float32)
    if kind == "arcface" or kc == 1:
        arg = s32.argmax(2)                                 # the first maximum of the fp32 values
        sp = np.take_along_axis(s3, arg[:, :, None], 2)[:, :, 0]
        dsds = (np.arange(kc)[None, None, :] == arg[:, :, None]).astype(np.float64)
        pool = dict(arg=arg)
    else:
        z = s3 / pr["gamma"]
        zm = z.max(2, keepdims=True)
        xx = np.exp(z - zm)
        den = xx.sum(2, keepdims=True)
        pj = xx / den
        sp = (pj * s3).sum(2)
        dsds = pj * (1.0 + (s3 - sp[:, :, None]) / pr["gamma"])
        pool = dict(z=z, zm=zm, x=xx, den=den[:, :, 0], p=pj)
    a_ = pr["a"]
    sy = np.where(pos, sp, 0.0).sum(1)                      # own-class pooled similarity (0 for an unlabelled row)
    psi = np.ones(n)
    if kind == "arcface":
        phi, slope, r, upper = phi_of(sy, pr)
        t = a_ * np.where(pos, phi[:, None], sp)
        psi = np.where(labelled, slope, 1.0)
        lower = labelled & ~upper
        pool.update(phi=phi, r=r, upper=upper)
    else:
        t = a_ * (sp - pr["b"] * pos)
        lower = np.zeros(n, bool)
    big_m = t.max(1)
    ex = np.exp(t - big_m[:, None])
    d = ex.sum(1)
    ty = np.where(pos, t, 0.0).sum(1)
    ell = np.where(labelled, np.log(d) + (big_m - ty), 0.0)
    rg = regulariser(w, c, kc, pr["tau"] if kind == "soft_triple" else 0.0, q)
    loss = (ell.sum() / nl if nl else 0.0) + rg["R"]
    v = ex / d[:, None] - pos
    base = np.where(labelled[:, None], (a_ / max(nl, 1)) * v, 0.0)
    basep = base * np.where(pos, psi[:, None], 1.0)
    g = (basep[:, :, None] * dsds).reshape(n, nb)
    sp32 = sp.astype(np.float32)
    mxo = np.where(~pos, sp32, -np.inf).max(1)
    viol = labelled & (mxo >= np.where(pos, sp32, np.inf).min(1))
    out = dict(kind=kind, pr=pr, S=s, Aq=aq, q=q, pos=pos, labelled=labelled, n=n, c=c, kc=kc, nl=nl, Sp=sp, dsds=dsds, t=t, M=big_m,
               e=ex, d=d, ell=ell, loss=loss, reg=rg, G=g, v=v, base=base, basep=basep, psi=psi, sy=sy,
               counts=np.array([nl, int(viol.sum()), int(lower.sum())], np.int64))
    out.update(pool)
    return out


def pooled_bound(ref, gs):
    """-> (dS [n, c, kc], dS' [n, c]) and, for 'soft_triple' with kc > 1, what the bound on G reads (E, rd)."""
    s, kc, n, c = ref["S"], ref["kc"], ref["n"], ref["c"]
    ds = (gs * ref["Aq"] * (1.0 + U) + U * np.abs(s)).reshape(n, c, kc)
    if kc == 1:
        return ds, ds[:, :, 0], None
    if ref["kind"] == "arcface":
        return ds, ds.max(2), None
    gm, s3 = ref["pr"]["gamma"], s.reshape(n, c, kc)
    z, x, den, sp = ref["z"], ref["x"], ref["den"], ref["Sp"]
    dz = ds / gm * (1.0 + U) + U * np.abs(z)
    dzm = dz.max(2, keepdims=True)
    vv = z - ref["zm"]
    dv = dz + dzm + U * (np.abs(vv) + dz + dzm)
    big_e = x * (np.expm1(dv) + ULP_EXP_LOG * np.exp(dv)) + TINY
    gk = float(gamma(kc + 1))
    d_den = big_e.sum(2) * (1.0 + gk) + gk * den
    xe = x + big_e
    d_num = (big_e * np.abs(s3 - sp[:, :, None]) + xe * ds + gk * xe * (np.abs(s3) + ds)).sum(2) + gk * np.abs(sp) * xe.sum(2)
    assert np.all(d_den < 0.5)
    dsp = d_num / (den - d_den) * (1.0 + U) + U * np.abs(sp) + TINY
    return ds, dsp, dict(E=big_e, rd=d_den / den)


def decisions(ref, gs):
    """-> dict(sure, may, open [n]: violating samples; lower_sure, lower_may [n]; open_cells [n, c]: ArcFace argmax cells whose two
    largest similarities lie within 2 max dS of each other; branch_open [n])."""
    ds, dsp, _ = pooled_bound(ref, gs)
    sp, pos, lab, n, c, kc = ref["Sp"], ref["pos"], ref["labelled"], ref["n"], ref["c"], ref["kc"]
    lo, hi = (sp - dsp).astype(np.float32), (sp + dsp).astype(np.float32)

    def viol(others, own):
        return lab & (np.where(~pos, others, -np.inf).max(1) >= np.where(pos, own, np.inf).min(1))
    sure, may = viol(lo, hi), viol(hi, lo)
    out = dict(sure=sure, may=may, open=sure != may, open_cells=np.zeros((n, c), bool), lower_sure=np.zeros(n, bool),
               lower_may=np.zeros(n, bool), branch_open=np.zeros(n, bool))
    if ref["kind"] == "arcface":
        th = np.float32(ref["pr"]["th"])
        own_lo, own_hi = np.where(pos, lo, 0).sum(1), np.where(pos, hi, 0).sum(1)
        out["lower_sure"], out["lower_may"] = lab & (own_hi <= th), lab & (own_lo <= th)
        out["branch_open"] = out["lower_sure"] != out["lower_may"]
        if kc > 1:
            srt = np.sort(ref["S"].reshape(n, c, kc), 2)
            out["open_cells"] = (srt[:, :, -1] - srt[:, :, -2]) <= 2.0 * ds.max(2)
    return out


def _rho(dz):
    return np.expm1(dz) + ULP_EXP_LOG * np.exp(dz)


def bounds(ref, gs, exact_argmax=False):
    """-> dict(G [n, c kc] per-entry bound, total [n, c] bound on a class's sum_j G_j, open_cells [n, c], loss, reg, H) for a device
    whose D is within gs A of the truth (module docstring).  exact_argmax: the inputs are exact in any order (gs = 0), so the device's
    S~ is the fp32 rounding of S and its argmax is the reference's: no cell is open."""
    kind, pr, n, c, kc = ref["kind"], ref["pr"], ref["n"], ref["c"], ref["kc"]
    a, pos, lab, nl = pr["a"], ref["pos"], ref["labelled"], max(ref["nl"], 1)
    g2, g3 = float(gamma(2)), float(gamma(3))
    ds, dsp, st = pooled_bound(ref, gs)
    sp, t = ref["Sp"], ref["t"]
    dt = a * dsp * (1.0 + g2) + g2 * np.abs(t)
    dpsi = np.zeros(n)
    if kind == "arcface":
        sy, dsy = ref["sy"], np.where(pos, dsp, 0.0).sum(1)
        th, cm, sm = pr["th"], pr["cm"], pr["sm"]
        up_sure, low_sure = sy - dsy > th, sy + dsy <= th
        assert np.all(up_sure[lab] | low_sure[lab]), "an own-class similarity within dS' of cos(pi - m): the branch is open"
        big_a = 1.0 - sy * sy
        d_a = ((2.0 * np.abs(sy) * dsy + dsy * dsy) * (1.0 + 2 * U) + U * (sy * sy + np.abs(big_a))) / (1.0 - U)
        r_lo, r_hi = np.sqrt(np.maximum(0.0, big_a - d_a)), np.sqrt(np.maximum(0.0, big_a + d_a))
        dr = r_hi - r_lo + U * r_hi
        phi, r = ref["phi"], ref["r"]
        dphi = np.where(up_sure, (cm * dsy + sm * dr) * (1.0 + 2 * U) + U * (np.abs(sy * cm) + r * sm) + U * np.abs(phi),
                        dsy * (1.0 + U) + U * np.abs(phi))
        dty = a * dphi * (1.0 + U) + U * np.abs(np.where(pos, t, 0.0).sum(1))
        dt = np.where(pos, dty[:, None], dt)
        zero_r = up_sure & (big_a + d_a <= 0)
        band = lab & up_sure & ~zero_r & ~(r_lo > R_FLOOR)
        if exact_argmax:                                    # S'~ is the fp32 rounding of S': A~ is reproduced where A is 0
            band &= ~(sy.astype(np.float32).astype(np.float64) ** 2 == 1.0)
        assert not band.any(), "an own-class similarity in the floor band of r: no bound is stated there"
        with np.errstate(divide="ignore", invalid="ignore"):
            reg_psi = (sm * dsy * (1.0 + U) + U * np.abs(sy * sm)) / r_lo + np.abs(sy * sm) * (1.0 / r_lo - 1.0 / (r_hi * (1.0 + U))) \
                + 2 * U * np.abs(ref["psi"])
        dpsi = np.where(lab & up_sure & (r_lo > R_FLOOR), reg_psi, 0.0)
    gl = float(gamma(-(-c // 64) + 7))
    dm = dt.max(1)[:, None]
    z = t - ref["M"][:, None]
    dz = dt + dm + U * (np.abs(z) + dt + dm)
    rho = _rho(dz)
    e, d = ref["e"], ref["d"]
    rho_d = ((rho * e).sum(1) / d * (1.0 + gl) + gl + c * 2.0 ** -126)[:, None]
    assert np.all(rho_d[lab] < 0.5), "the similarity error is too large for a meaningful bound"
    rho_d = np.minimum(rho_d, 0.5)
    wgt = e / d[:, None]
    bw = wgt * ((rho + rho_d) / (1.0 - rho_d) * (1.0 + U) + U) + TINY
    v = ref["v"]
    bv = np.where(pos, bw + U * (np.abs(v) + bw), bw)
    b_base = (a / nl) * ((1.0 + g2) * bv + g2 * np.abs(v)) + TINY
    base, basep = ref["base"], ref["basep"]
    if kind == "arcface":
        own = b_base * (np.abs(ref["psi"]) + dpsi)[:, None] + np.abs(base) * dpsi[:, None] + U * np.abs(basep) + TINY
        b_base = np.where(pos, own, b_base)
    b_base = np.where(lab[:, None], b_base, 0.0)
    open_cells = np.zeros((n, c), bool)
    if kc == 1:
        b_g = b_base[:, :, None]
    elif kind == "arcface":
        b_g = b_base[:, :, None] * ref["dsds"]
        if not exact_argmax:
            srt = np.sort(ref["S"].reshape(n, c, kc), 2)
            open_cells = (srt[:, :, -1] - srt[:, :, -2]) <= 2.0 * ds.max(2)
    else:
        gm, s3, pj = pr["gamma"], ref["S"].reshape(n, c, kc), ref["p"]
        rd = st["rd"][:, :, None]
        dp = pj * ((st["E"] / ref["x"] + rd) / (1.0 - rd) * (1.0 + U) + U) + TINY
        h = 1.0 + (s3 - sp[:, :, None]) / gm
        dh = ((ds + dsp[:, :, None]) * (1.0 + g3) / gm + g2 * np.abs(h - 1.0)) * (1.0 + U) + U * np.abs(h)
        big_f = ref["dsds"]
        d_f = dp * (np.abs(h) + dh) + pj * dh + U * np.abs(big_f) + TINY
        gg = basep[:, :, None] * big_f
        b_g = b_base[:, :, None] * (np.abs(big_f) + d_f) + np.abs(basep)[:, :, None] * d_f + U * np.abs(gg) + TINY
        b_g = np.where(lab[:, None, None], b_g, 0.0)
    lam = -np.log1p(-rho_d[:, 0])
    dzy = np.where(pos, dz, 0.0).sum(1)
    b_l = np.where(lab, (lam + ULP_EXP_LOG * (np.log(d) + lam) + dzy) * (1.0 + U) + U * np.abs(ref["ell"]), 0.0)
    rg = ref["reg"]
    b_loss = b_l.sum() / nl + rg["dR"] + (2 * U + 2.0 ** -40) * abs(ref["loss"])
    return dict(G=b_g.reshape(n, c * kc), total=b_base, open_cells=open_cells, loss=b_loss, reg=rg["dR"], H=rg["dH"])


def grads(x, w, g, q, c, h=None, upstream=1.0):
    """float64 (demb, dcentres) and their bounds (module docstring) from a given G [n, c kc], q and H [c, kc, kc] (None: none)."""
    x, w = np.asarray(x, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    gt, qd = np.asarray(g, np.float64).T, np.asarray(q, np.float32).astype(np.float64)                  # [nb, n]
    n, e = x.shape
    nb = w.shape[0]
    kc = nb // c
    up = float(np.float32(upstream))
    qg = gt * qd[:, None]
    demb = up * (qg.T @ w)
    b_emb = U * np.abs(demb) + (nb + 8) * 2.0 ** -53 * abs(up) * (np.abs(qg).T @ np.abs(w)) + 2.0 ** -149
    y, ya = gt @ x, np.abs(gt) @ np.abs(x)
    if h is not None and kc > 1:
        h = np.asarray(h, np.float64).reshape(c, kc, kc)
        qw = (qd[:, None] * w).reshape(c, kc, e)
        y = y + np.einsum("cst,cte->cse", h, qw).reshape(nb, e)
        ya = ya + np.einsum("cst,cte->cse", np.abs(h), np.abs(qw)).reshape(nb, e)
    t = (y * w).sum(1)
    dw = up * qd[:, None] * (y - (qd * qd * t)[:, None] * w)
    ta = (ya * np.abs(w)).sum(1)
    b_w = (U * np.abs(dw) + (n + kc + -(-e // 64) + 16) * 2.0 ** -53 * abs(up) * qd[:, None] * (ya + (qd * qd * ta)[:, None] * np.abs(w))
           + 2.0 ** -149)
    return demb, b_emb, dw, b_w


# ---- the cases the CPU and the GPU test share (p, k, c, kc, e): n = p k samples of p of the c classes ---------------------------------
SIGMA = 0.8
SMALL_SHAPES = [(3, 3, 5, 2, 64),                           # (these fit the small path; `auto` takes it below 100 centres)
                (5, 5, 7, 2, 33), (8, 4, 24, 3, 256), (32, 4, 100, 3, 256), (4, 4, 6, 32, 16), (16, 16, 40, 1, 128),
                (8, 4, 70, 10, 64)]
MATRIX_SHAPES = [(4, 4, 1367, 3, 96),                      # e + c kc = 4197
                 (2, 2, 512, 32, 8)]                       # c kc = 16384
SHAPES = SMALL_SHAPES + MATRIX_SHAPES
RAGGED = (64, 40, 3)                                        # (e, c, kc) of the ragged general-label batch
OPEN_CAP = 0.01                                             # at most 1 % of a case's (sample, class) cells may be open


def seed_of(p, k, c, kc, e):
    return p * 1000 + k * 10 + e + 7 * kc


def case_inputs(shape, grid=False):
    """The inputs of one shared case ('ragged' or (p, k, c, kc, e)) -> (x, w, labels, c, kc, unit or None); grid: x and w on
    proxy_ref.to_grid's grid (exact in any order)."""
    import recipes as R
    if shape == "ragged":
        e, c, kc = RAGGED
        x, w, lab = ragged_inputs(R.clustered_embeddings(77, 5, 5, e, SIGMA), e, c, kc, 77)
    else:
        p, k, c, kc, e = shape
        seed = seed_of(p, k, c, kc, e)
        x, w, lab = make_inputs(R.clustered_embeddings(seed, p, k, e, SIGMA), p, k, c, kc, seed)
    unit = None
    if grid:
        x, w, unit = P.to_grid(x, w)
    return x, w, lab, c, kc, unit


def gamma_s_of(shape, path="auto"):
    if shape == "ragged":
        (e, c, kc), n = RAGGED, 17
    else:
        p, k, c, kc, e = shape
        n = p * k
    return P.gamma_s(auto_path(n, c, kc, e) if path == "auto" else path, e)
