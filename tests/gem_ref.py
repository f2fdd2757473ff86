"""Float64 restatement of generalised-mean pooling (embnet_gem_fwd / embnet_gem_bwd, include/embnet.h) and the error bounds of the
fp32 kernels, derived from the contract's operation list.

The operation.  x[n,hw,c], p[1] or p[c] (> 0), eps > 0, per (sample, channel):
    z_i = max(x_i, eps)     M = max_i z_i     r_i = z_i / M     l_i = log2 r_i     e_i = 2^(p l_i) = r_i^p
    S = sum_i e_i           s = S / hw        y = M s^(1/p)                                    (>= 1 <= hw: the largest e_i is 1)
    g_i = e_i ln r_i        T = sum_i g_i     t = T / hw      dydp = y (t / (p s) - ln s / p^2)                  (M cancels)
    dx_i = (dy / hw) (z_i / y)^(p - 1) [x_i >= eps]           dp = sum dy dydp over (n, c) or, per channel, over n
`naive` is the textbook form x.clamp(min=eps).pow(p).mean().pow(1/p); the two agree wherever the naive one is finite.

Bounds.  u = 2^-24; a correctly rounded fp32 operation (+, *, /, and the conversions) has relative error u.  log2f and exp2f are
the ROCm device library's: HIP's table gives 1 ulp for both, OpenCL's full profile, which the library implements, guarantees
3 ulp = 6 u (ms_ref.ULP_EXP_LOG, as for expf / logf in the loss references): E = 6 u.  gamma(k) = k u / (1 - k u).  TINY = 2^-125
stands for a result flushed below the smallest normal number.  Premise: eps / M >= 2^-126 (r is a normal number).
  r~ = r (1 + d), |d| <= u.
  l~ = log2f(r~):       |l~ - l| <= Dl = E |l| + (1 + E) u / ln2 / (1 - u)         (log2's own error; log2(1 + d) of the input's)
  q~ = fl(p l~):        |q~ - p l| <= Dq = p Dl + u (|p l| + p Dl)
  e~ = exp2f(q~):       relative rho_e = expm1(ln2 Dq) + E exp(ln2 Dq);   De = e rho_e + TINY
  S~:  positive terms; the longest path of additions is L = ceil(hw / 16) + 15 (c % 4 == 0: a lane's chain, then the 15 lane
       additions) or hw (c % 4 != 0: one chain):   DS = (sum De) (1 + gamma(L)) + gamma(L) S
  s~ = fl(S~ / hw):     rho_s = DS / S (1 + u) + u;   lam = -log1p(-rho_s) bounds |ln(s~ / s)|
  ls~ = log2f(s~):      Dls = lam / ln2 + E (|log2 s| + lam / ln2)
  a~ = fl(ls~ / p):     Da = Dls / p + u (|log2 s| / p + Dls / p)
  w~ = exp2f(a~):       rho_w = expm1(ln2 Da) + E exp(ln2 Da)
  y~ = fl(M w~):        rho_y = rho_w (1 + u) + u;   Dy = y rho_y
  dydp:  ln r~ = fl(l~ LN2), LN2 = fl(ln 2):  Dlam_i = ln2 Dl (1 + gamma(2)) + gamma(2) |ln r|
         g~ = fl(e~ ln r~):  Dg = (De (|ln r| + Dlam) + e Dlam) (1 + u) + u |g| + TINY
         DT = (sum Dg) (1 + gamma(L)) + gamma(L) sum |g|;   t~ = fl(T~ / hw):  Dt = DT / hw (1 + u) + u |t|
         A = t / (p s):  fl(p s~) has relative error rho_ps = rho_s (1 + u) + u;  DA = (Dt / (p s) + |A| rho_ps) / (1 - rho_ps) (1 + u) + u |A|
         B = ln s / p^2:  fl(ls~ LN2): Dn = ln2 Dls (1 + gamma(2)) + gamma(2) |ln s|;  fl(p p): u;  DB = (Dn / p^2 + |B| u) / (1 - u) (1 + u) + u |B|
         C = A - B:  DC = DA + DB + u (|C| + DA + DB);    dydp~ = fl(y~ C~):  Ddydp = (Dy (|C| + DC) + y DC) (1 + u) + u |dydp| + TINY
  dx (from the fp32 y~ the forward wrote, rho_y off y):
         fl(dy / hw): u;   fl(p - 1): Dm = u |p - 1|;   v~ = fl(x / y~): rho_v = rho_y / (1 - rho_y) (1 + u) + u,  lamv = -log1p(-rho_v)
         log2f(v~):  Dlv = lamv / ln2 + E (|log2 v| + lamv / ln2);   the product with fl(p - 1):
         Dqv = (|p - 1| Dlv + Dm (|log2 v| + Dlv)) (1 + u) + u |(p - 1) log2 v|;   exp2f: rho = expm1(ln2 Dqv) + E exp(ln2 Dqv)
         dx~ = fl(fl(dy / hw) exp2f(.)):  Ddx = |dx| (rho (1 + gamma(2)) + gamma(2)) + TINY;   x < eps: dx~ = 0 exactly.
  dp:    float64 on the device: the products are exact, the sum of k terms adds (k + 8) 2^-53 sum |dy dydp|, the store rounds once:
         Ddp = sum |dy| Ddydp + u |dp| + (k + 8) 2^-53 sum |dy dydp| + 2^-149.
"""
import numpy as np

from ms_ref import TINY, U, ULP_EXP_LOG as E, gamma

LN2 = float(np.log(2.0))


def _p_row(p, c):
    p = np.asarray(p, np.float32).astype(np.float64).reshape(-1)
    assert p.size in (1, c) and np.all(p > 0), p
    return np.broadcast_to(p, (c,)) if p.size == 1 else p


def naive(x, p, eps, dtype=np.float64):
    """(mean_hw max(x, eps)^p)^(1/p) as written, in `dtype` (float32: overflows where the maximum-normalised form does not)."""
    x = np.asarray(x, np.float32).astype(dtype)
    pr = _p_row(p, x.shape[2]).astype(dtype)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        z = np.maximum(x, dtype(np.float32(eps)))
        return (z ** pr).mean(axis=1, dtype=dtype) ** (dtype(1) / pr)


def gem(x, p, eps, dy=None):
    """x[n,hw,c], p[1] | p[c], eps as the C ABI sees them (rounded to fp32), dy[n,c] optional.  -> dict of float64 arrays:
    y, dydp [n,c] and their bounds b_y, b_dydp, rho_y; with dy: dx [n,hw,c], dp [1] | [c] and b_dx, b_dp."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n, hw, c = x.shape
    scalar_p = np.asarray(p).size == 1
    pr = _p_row(p, c)[None, :]                                # [1,c]
    eps = float(np.float32(eps))
    z = np.maximum(x, eps)
    m = z.max(axis=1)                                         # [n,c]
    assert eps / m.max() >= 2.0 ** -126
    r = z / m[:, None, :]
    l = np.log2(r)
    pe = pr[:, None, :]                                       # [1,1,c]
    e = np.exp2(pe * l)
    big_s = e.sum(axis=1)
    s = big_s / hw
    y = m * s ** (1.0 / pr)
    lnr = l * LN2
    g = e * lnr
    t = g.sum(axis=1) / hw
    a_term, b_term = t / (pr * s), np.log(s) / (pr * pr)
    cc = a_term - b_term
    dydp = y * cc
    out = dict(y=y, dydp=dydp, s=s, t=t, m=m)

    # ---- forward bounds
    chain = -(-hw // 16) + 15 if c % 4 == 0 else hw
    gl, g2 = float(gamma(chain)), float(gamma(2))
    d_l = E * np.abs(l) + (1.0 + E) * U / LN2 / (1.0 - U)
    d_q = pe * d_l + U * (np.abs(pe * l) + pe * d_l)
    rho_e = np.expm1(LN2 * d_q) + E * np.exp(LN2 * d_q)
    d_e = e * rho_e + TINY
    d_s = d_e.sum(axis=1) * (1.0 + gl) + gl * big_s
    rho_s = d_s / big_s * (1.0 + U) + U
    lam = -np.log1p(-rho_s)
    ls = np.log2(s)
    d_ls = lam / LN2 + E * (np.abs(ls) + lam / LN2)
    d_a = d_ls / pr + U * (np.abs(ls) / pr + d_ls / pr)
    rho_w = np.expm1(LN2 * d_a) + E * np.exp(LN2 * d_a)
    rho_y = rho_w * (1.0 + U) + U
    d_y = y * rho_y
    d_lam = LN2 * d_l * (1.0 + g2) + g2 * np.abs(lnr)
    d_g = (d_e * (np.abs(lnr) + d_lam) + e * d_lam) * (1.0 + U) + U * np.abs(g) + TINY
    d_t = (d_g.sum(axis=1) * (1.0 + gl) + gl * np.abs(g).sum(axis=1)) / hw * (1.0 + U) + U * np.abs(t)
    rho_ps = rho_s * (1.0 + U) + U
    d_a_term = (d_t / (pr * s) + np.abs(a_term) * rho_ps) / (1.0 - rho_ps) * (1.0 + U) + U * np.abs(a_term)
    d_n = LN2 * d_ls * (1.0 + g2) + g2 * np.abs(np.log(s))
    d_b_term = (d_n / (pr * pr) + np.abs(b_term) * U) / (1.0 - U) * (1.0 + U) + U * np.abs(b_term)
    d_c = d_a_term + d_b_term + U * (np.abs(cc) + d_a_term + d_b_term)
    b_dydp = (d_y * (np.abs(cc) + d_c) + y * d_c) * (1.0 + U) + U * np.abs(dydp) + TINY
    out.update(b_y=d_y, rho_y=rho_y, b_dydp=b_dydp)
    if dy is None:
        return out

    # ---- backward
    dy = np.asarray(dy, np.float32).astype(np.float64)
    live = x >= eps
    v = z / y[:, None, :]
    lv = np.log2(v)
    dx = np.where(live, dy[:, None, :] / hw * np.exp2((pe - 1.0) * lv), 0.0)
    prod = dy * dydp
    dp = np.array([prod.sum()]) if scalar_p else prod.sum(axis=0)
    pm1 = np.abs(pe - 1.0)
    rho_v = (rho_y / (1.0 - rho_y) * (1.0 + U) + U)[:, None, :]
    lamv = -np.log1p(-rho_v)
    d_lv = lamv / LN2 + E * (np.abs(lv) + lamv / LN2)
    d_qv = (pm1 * d_lv + U * pm1 * (np.abs(lv) + d_lv)) * (1.0 + U) + U * np.abs(pm1 * lv)
    rho = np.expm1(LN2 * d_qv) + E * np.exp(LN2 * d_qv)
    b_dx = np.where(live, np.abs(dx) * (rho * (1.0 + g2) + g2) + TINY, 0.0)
    k = n * c if scalar_p else n
    spread = np.abs(dy) * b_dydp
    mag = np.abs(prod)
    if scalar_p:
        spread, mag = np.array([spread.sum()]), np.array([mag.sum()])
    else:
        spread, mag = spread.sum(axis=0), mag.sum(axis=0)
    b_dp = spread + U * np.abs(dp) + (k + 8) * 2.0 ** -53 * mag + 2.0 ** -149
    out.update(dx=dx, dp=dp, b_dx=b_dx, b_dp=b_dp, live=live)
    return out
