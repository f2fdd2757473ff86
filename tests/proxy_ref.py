"""float64 restatement of the Proxy-Anchor and CosFace / NormSoftmax losses (include/embnet.h, csrc/proxy_loss.hip) and the a-priori
rounding bounds their kernels are held to.  NumPy only, no kernel code.  tests/test_proxy_ref_cpu.py checks the restatement (autograd,
differences, a scalar restatement, hand cases) and the fitness of the GPU test's inputs; tests/test_proxy_loss_gpu.py checks the
kernels against it.

Semantics (the header's).  X [n, e], W [c, e] fp32, y [n] integer labels (outside [0, c): unlabelled).  q_c = float32(1 / sqrt(ss_c)),
ss_c = sum_k w_ck^2 in float64 in k order (0 -> q_c = 0);  S_ic = D_ic q_c, D = X W^T.  The scalar parameters ROUNDED TO fp32.
    'anchor'   P_c = {i: y_i = c}, N_c = the labelled i with y_i != c, C+ = {c: P_c not empty};  t+ = -alpha (S - delta),
               t- = alpha (S + delta);  per side m = max(0, max t), d = e^-m + sum e^(t - m), side = m + log d;
               loss = sum_{C+} side+ / |C+| + sum_c side- / c;  G [c, n] = -(alpha / |C+|) e^(t+ - m+) / d+ on P_c,
               +(alpha / c) e^(t- - m-) / d- on N_c, 0 elsewhere.
    'softmax'  labelled i of class y:  t_ic = sigma (S_ic - mu [c = y]),  M = max_c t,  d = sum_c e^(t - M),
               l_i = log d + (M - t_iy);  loss = sum l_i / n_l;  G [n, c] = (sigma / n_l)(e^(t - M) / d - [c = y]), unlabelled rows 0.
    counts = {|C+| or n_l, labelled samples, violating anchors on the fp32 S}.
    Q = q_c G;  demb = g Q^T W ('anchor') or g Q W ('softmax');  Y_c = sum_i G_ci x_i;  dW_c = g q_c (Y_c - q_c^2 (Y_c . w_c) w_c).

Bounds.  u = 2^-24, gamma(n) = n u / (1 - n u) (ms_ref.gamma).  Nothing is measured; the rounding counts are read off proxy_loss.hip.
"flush": a result below 2^-126 may become 0, an absolute 2^-125 = TINY.

  q.  The squares of fp32 numbers are exact in float64, so the k-ordered float64 chain is the same fused or not; sqrt and the division
      are correctly rounded float64 operations and the cast rounds once: q is REPRODUCED by q_of(), bit for bit.
  S.  S~ = fl(D~ q), |D~ - D| <= gamma_S A, A_ic = sum_k |x_ik w_ck|:  |S~ - S| <= dS = gamma_S A q (1 + u) + u |S|.
      gamma_S = gamma_s(path, e): small path: lane l owns the columns l, l + 64, ...: ceil(e / 64) fma and the six additions of the wave
      butterfly, gamma(ceil(e / 64) + 7) with one to spare (ms_ref's per-class staging); matrix path: embnet_dense_dgrad_f32's k-ordered
      chain, gamma(e + 1); grid inputs (x and w multiples of 1 / qg, A qg^2 <= 2^24): D~ = D in any order, gamma_S = 0, so S~ is the
      fp32 rounding of S: the counters are exact.
  t.  t~ = fl(c fl(S~ + o)), o = -+delta or -mu or nothing:  |t~ - t| <= Dt = c dS (1 + gamma(2)) + gamma(2) |t|.
  m / M.  fl is monotone, the device's maximum of a set is the t~ of some member, max(0, .) is a contraction: Dm = max over the set of Dt.
  z = t - m:  |z~ - z| <= Dz = Dt + Dm + u (|z| + Dt + Dm).       e = exp(z): rho = expm1(Dz) + 6 u exp(Dz) (expf, logf: 3 ulp,
      ms_ref.ULP_EXP_LOG);  e0 = exp(-m): rho0 = expm1(Dm) + 6 u exp(Dm).
  d: positive terms; a lane adds at most ceil(cols / 64), the butterfly six times, e0 joins with one more: L = ceil(cols / 64) + 7,
      rho_d = (sum rho e + rho0 e0) / d (1 + gamma(L)) + gamma(L) + cols 2^-126  (d >= 1 on both losses).
  w = fl(e / d):  Bw = w ((rho + rho_d) / (1 - rho_d)(1 + u) + u) + TINY.
  'anchor'.   G~ = fl(k~ w~), k~ = fl(alpha / N) = (alpha / N)(1 + d1), N = |C+| or c exact in fp32:
      |G~ - G| <= (alpha / N)((1 + gamma(2)) Bw + gamma(2) w) + TINY.
      side~ = fl(m~ + logf(d~)):  lam = -log(1 - rho_d);  B_side = (Dm + lam + 6 u (|log d| + lam))(1 + u) + u |side|.
      loss: both sums and both divisions are float64 on the device, then one cast:
      |loss~ - loss| <= sum_{C+} B_side+ / |C+| + sum_c B_side- / c + (u + 2^-40) |loss|.
  'softmax'.  v = w - [c = y]: Bv = Bw + u (|v| + Bw) at c = y, Bw elsewhere;  G~ = fl(k~ v~), k~ = fl(sigma / n_l):
      |G~ - G| <= (sigma / n_l)((1 + gamma(2)) Bv + gamma(2) |v|) + TINY.       ABSOLUTE: w - 1 cancels.
      l~ = fl(logf(d~) + fl(M~ - t~_y)):  h = M - t_y >= 0, |h~ - h| <= Dz_y;  B_l = (lam + 6 u (log d + lam) + Dz_y)(1 + u) + u l.
      |loss~ - loss| <= sum B_l / n_l + (u + 2^-40) |loss|.
  backward, against float64 of the DEVICE's own G and q.  q G is an exact float64 product; a float64 fma chain of J terms, the scale
      by g, one fp32 rounding:  |demb~ - demb| <= u |demb| + (c + 8) 2^-53 |g| sum_c |Q_ci| |w_ck| + 2^-149.
      Y: a chain of n terms; t_c = Y_c . w_c: lane chains of ceil(e / 64) and the butterfly; the expression adds a handful of float64
      operations:  |dW~ - dW| <= u |dW| + (n + ceil(e / 64) + 16) 2^-53 |g| q_c (Ya_ck + q_c^2 (Ya_c . |w_c|) |w_ck|) + 2^-149,
      Ya = |G| |X|.

Violating anchors.  The device's S~ is SOME fp32 number in [fl((D - gamma_S A) q), fl((D + gamma_S A) q)] (fl is monotone): an anchor
surely violates when it does at the unfavourable ends, possibly when it does at the favourable ends; it is OPEN when the two differ.
"""
import numpy as np

from ms_ref import TINY, U, ULP_EXP_LOG, gamma, grid_q

KINDS = ("anchor", "softmax")
DEFAULTS = {"anchor": (32.0, 0.1), "softmax": (64.0, 0.35)}
MAX_N, MAX_C, MAX_E = 4096, 16384, 4096


# ---- path rule, workspace (embnet_proxy_loss_path / _workspace_bytes restated) -------------------------------------------------------
def in_range(n, c, e):
    return 2 <= n <= MAX_N and 2 <= c <= MAX_C and 1 <= e <= MAX_E


def auto_path(n, c, e):
    """'small' | 'matrix'; None outside the range."""
    if not in_range(n, c, e):
        return None
    return "small" if 4 * (e + max(n, c)) <= 16 * 1024 and n * c * e <= 2 ** 25 else "matrix"


def workspace_bytes(n, c, e):
    if not in_range(n, c, e):
        return 0
    a16 = lambda b: (b + 15) // 16 * 16
    return 16 + a16(4 * c) + 32 * max(n, c) + a16(4 * c * n) + a16(8 * c * e)


def gamma_s(path, e):
    if path == "exact":
        return 0.0
    if path == "small":
        return float(gamma(-(-e // 64) + 7))
    assert path == "matrix", path
    return float(gamma(e + 1))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(x, p, k, c, seed, proxy_sigma=0.5):
    """A class-contiguous block x [p k, e] (recipes.clustered_embeddings) -> (x, w fp32 [c, e], labels int32 [p k]): the p classes
    get distinct global indices out of c (p > c: cluster j is class j mod c); the proxy of a present class is its members' normalised mean plus proxy_sigma randn / sqrt(e),
    the others are |randn|; every proxy row is rescaled by a factor in [0.5, 3]."""
    e = x.shape[1]
    r = np.random.RandomState(seed + 1)
    cls = r.permutation(c)[:p] if p <= c else np.arange(p) % c          # more clusters than classes: several clusters per class
    labels = np.repeat(cls, k).astype(np.int32)
    w = np.abs(r.randn(c, e))
    x64 = x.astype(np.float64)
    for cl in np.unique(cls):
        cent = x64[labels == cl].mean(0)
        w[cl] = cent / np.linalg.norm(cent) + proxy_sigma * r.randn(e) / np.sqrt(e)
    w *= r.uniform(0.5, 3.0, size=(c, 1))
    return x, w.astype(np.float32), labels


def ragged_inputs(x5, e, c, seed):
    """From a class-contiguous 5 x 5 block: class j keeps j + 1 rows (sizes 1 .. 5), two more rows are unlabelled (labels -1 and c),
    the rows are shuffled.  -> (x [17, e], w [c, e], labels int32 [17])."""
    assert x5.shape == (25, e) and c >= 5
    r = np.random.RandomState(seed + 2)
    keep = np.concatenate([np.arange(5 * j, 5 * j + j + 1) for j in range(5)])
    cls = r.permutation(c)[:5]
    lab = np.concatenate([np.repeat(cls, np.arange(1, 6)), [-1, c]]).astype(np.int32)
    extra = np.abs(r.randn(2, e))
    extra /= np.linalg.norm(extra, axis=1, keepdims=True)
    x = np.concatenate([x5[keep], extra.astype(np.float32)])
    w = np.abs(r.randn(c, e))
    for j in range(5):
        cent = x5[5 * j:5 * j + j + 1].astype(np.float64).mean(0)
        w[cls[j]] = cent / np.linalg.norm(cent) + 0.5 * r.randn(e) / np.sqrt(e)
    w *= r.uniform(0.5, 3.0, size=(c, 1))
    order = r.permutation(17)
    return x[order], w.astype(np.float32), lab[order]


def to_grid(x, w):
    """x and w rounded to multiples of 1 / qg.  -> (x, w fp32, unit = 1 / qg)."""
    qg = grid_q(x.shape[1])
    rnd = lambda a: (np.round(np.asarray(a, np.float64) * qg) / qg).astype(np.float32)
    return rnd(x), rnd(w), 1.0 / qg


def exact_in_any_order(x, w, unit):
    """True iff x and w are integer multiples of `unit` and sum_k |x_ik w_ck| <= 2^24 unit^2 everywhere: every product and partial
    sum of D, in any order and with or without fma, is exact in fp32 (and every ss_c in float64)."""
    mx, mw = np.asarray(x, np.float64) / unit, np.asarray(w, np.float64) / unit
    return bool(np.array_equal(mx, np.round(mx)) and np.array_equal(mw, np.round(mw)) and (np.abs(mx) @ np.abs(mw).T).max() <= 2 ** 24)


# ---- similarity -----------------------------------------------------------------------------------------------------------------------
def q_of(w):
    """The header's q, bit for bit: a float64 chain over k in order, one float64 sqrt, one float64 division, one cast."""
    w = np.asarray(w, np.float32).astype(np.float64)
    ss = np.zeros(w.shape[0])
    for k in range(w.shape[1]):
        ss = ss + w[:, k] * w[:, k]
    with np.errstate(divide="ignore"):
        return np.where(ss > 0, (1.0 / np.sqrt(ss)).astype(np.float32), np.float32(0)).astype(np.float32)


def similarity(x, w, q=None):
    """-> (S [n, c] float64 = D q, A q [n, c], q fp32 [c])."""
    x, w = np.asarray(x, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    q = q_of(w) if q is None else np.asarray(q, np.float32)
    qd = q.astype(np.float64)
    return (x @ w.T) * qd, (np.abs(x) @ np.abs(w).T) * qd, q


def masks(labels, c):
    """-> (pos [n, c]: y_i = c, labelled [n])."""
    labels = np.asarray(labels, np.int64)
    labelled = (labels >= 0) & (labels < c)
    return (labels[:, None] == np.arange(c)[None, :]) & labelled[:, None], labelled


# ---- the counter ----------------------------------------------------------------------------------------------------------------------
def _viol(kind, neg_s, pos_s, pos, labelled):
    neg = ~pos & labelled[:, None]
    if kind == "anchor":                                    # per class (column): N_c not empty, P_c not empty
        mx = np.where(neg, neg_s, -np.inf).max(0)
        mn = np.where(pos, pos_s, np.inf).min(0)
        return pos.any(0) & neg.any(0) & (mx >= mn)
    mx = np.where(neg, neg_s, -np.inf).max(1)               # per sample (row): the other classes against its own
    sy = np.where(pos, pos_s, np.inf).min(1)
    return labelled & (mx >= sy)


def violating(kind, s32, labels):
    """On an fp32 S [n, c] -> bool per anchor ([c] for 'anchor', [n] for 'softmax')."""
    s32 = np.asarray(s32, np.float32)
    pos, labelled = masks(labels, s32.shape[1])
    return _viol(kind, s32, s32, pos, labelled)


def decisions(kind, x, w, labels, gs, q=None):
    """For D~ anywhere in [D - gs A, D + gs A]: -> dict(sure, may, open) bool per anchor."""
    s, aq, _ = similarity(x, w, q)
    lo, hi = (s - gs * aq).astype(np.float32), (s + gs * aq).astype(np.float32)
    pos, labelled = masks(labels, s.shape[1])
    sure = _viol(kind, lo, hi, pos, labelled)
    may = _viol(kind, hi, lo, pos, labelled)
    return dict(sure=sure, may=may, open=sure != may)


# ---- the losses -----------------------------------------------------------------------------------------------------------------------
def params32(kind, a=None, b=None):
    da, db = DEFAULTS[kind]
    return float(np.float32(da if a is None else a)), float(np.float32(db if b is None else b))


def _side(t, keep):
    """Stable log(1 + sum exp) over the rows of t [anchors, others].  -> (m, e, e0, d)."""
    m = np.maximum(np.where(keep, t, -np.inf).max(1), 0.0)
    e = np.where(keep, np.exp(np.where(keep, t - m[:, None], 0.0)), 0.0)
    e0 = np.exp(-m)
    return m, e, e0, e0 + e.sum(1)


def reference(kind, x, w, labels, a=None, b=None, q=None):
    """float64 loss, G (in the header's layout) and counts, with the intermediates bounds() reads."""
    assert kind in KINDS, kind
    a, b = params32(kind, a, b)
    s, aq, q = similarity(x, w, q)
    n, c = s.shape
    pos, labelled = masks(labels, c)
    nl = int(labelled.sum())
    viol = int(violating(kind, s.astype(np.float32), labels).sum())
    out = dict(kind=kind, a=a, b=b, S=s, Aq=aq, q=q, pos=pos, labelled=labelled, n=n, c=c)
    if kind == "anchor":
        st, post = s.T, pos.T                               # [c, n]
        negt = ~post & labelled[None, :]
        tp, tn = -a * (st - b), a * (st + b)
        mp, ep, e0p, dp = _side(tp, post)
        mg, en, e0n, dn = _side(tn, negt)
        sp, sn = mp + np.log(dp), mg + np.log(dn)
        present = post.any(1)
        ncp = int(present.sum())
        loss = (sp[present].sum() / ncp if ncp else 0.0) + sn.sum() / c
        g = -(a / max(ncp, 1)) * ep / dp[:, None] + (a / c) * en / dn[:, None]
        out.update(loss=loss, G=g, counts=np.array([ncp, nl, viol], np.int64), present=present, ncp=ncp,
                   sides=dict(pos=dict(keep=post, t=tp, m=mp, e=ep, e0=e0p, d=dp, side=sp, norm=max(ncp, 1)),
                              neg=dict(keep=negt, t=tn, m=mg, e=en, e0=e0n, d=dn, side=sn, norm=c)))
    else:
        t = a * (s - b * pos)
        big_m = t.max(1)
        e = np.exp(t - big_m[:, None])
        d = e.sum(1)
        ty = np.where(pos, t, 0.0).sum(1)
        ell = np.where(labelled, np.log(d) + (big_m - ty), 0.0)
        loss = ell.sum() / nl if nl else 0.0
        g = np.where(labelled[:, None], (a / max(nl, 1)) * (e / d[:, None] - pos), 0.0)
        out.update(loss=loss, G=g, counts=np.array([nl, nl, viol], np.int64), t=t, M=big_m, e=e, d=d, ell=ell, nl=nl)
    return out


def grads(kind, x, w, g, q, upstream=1.0):
    """float64 (demb, dproxies) and their bounds (module docstring) from a given G (the header's layout) and q."""
    x, w = np.asarray(x, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    g, qd = np.asarray(g, np.float64), np.asarray(q, np.float32).astype(np.float64)
    gcn = g if kind == "anchor" else g.T                    # [c, n]
    n, e = x.shape
    c = w.shape[0]
    up = float(np.float32(upstream))
    qg = gcn * qd[:, None]
    demb = up * (qg.T @ w)
    b_emb = U * np.abs(demb) + (c + 8) * 2.0 ** -53 * abs(up) * (np.abs(qg).T @ np.abs(w)) + 2.0 ** -149
    y = gcn @ x
    t = (y * w).sum(1)
    dw = up * qd[:, None] * (y - (qd * qd * t)[:, None] * w)
    ya = np.abs(gcn) @ np.abs(x)
    ta = (ya * np.abs(w)).sum(1)
    b_w = (U * np.abs(dw) + (n + -(-e // 64) + 16) * 2.0 ** -53 * abs(up) * qd[:, None] * (ya + (qd * qd * ta)[:, None] * np.abs(w))
           + 2.0 ** -149)
    return demb, b_emb, dw, b_w


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def _rho(dz):
    return np.expm1(dz) + ULP_EXP_LOG * np.exp(dz)


def bounds(ref, gs):
    """-> (bound_G in G's layout, bound_loss) for a device whose D is within gs A of the truth (module docstring)."""
    kind, a, s, n, c = ref["kind"], ref["a"], ref["S"], ref["n"], ref["c"]
    g2 = float(gamma(2))
    ds = gs * ref["Aq"] * (1.0 + U) + U * np.abs(s)        # [n, c]
    if kind == "anchor":
        bound_g = np.zeros((c, n))
        bound_loss = 0.0
        gl = float(gamma(-(-n // 64) + 7))
        for name in ("pos", "neg"):
            sd = ref["sides"][name]
            keep, t, m, e, e0, d = sd["keep"], sd["t"], sd["m"], sd["e"], sd["e0"], sd["d"]
            dt = np.where(keep, a * ds.T * (1.0 + g2) + g2 * np.abs(t), 0.0)
            dm = dt.max(1)
            z = np.where(keep, t - m[:, None], 0.0)
            dz = dt + dm[:, None] + U * (np.abs(z) + dt + dm[:, None])
            rho = np.where(keep, _rho(dz), 0.0)
            rho0 = _rho(dm)
            rho_d = ((rho * e).sum(1) + rho0 * e0) / d * (1.0 + gl) + gl + n * 2.0 ** -126
            assert np.all(rho_d < 0.5), "the similarity error is too large for a meaningful bound"
            wgt = e / d[:, None]
            bw = wgt * ((rho + rho_d[:, None]) / (1.0 - rho_d[:, None]) * (1.0 + U) + U) + TINY
            kk = a / sd["norm"]
            bound_g += np.where(keep, kk * ((1.0 + g2) * bw + g2 * wgt) + TINY, 0.0)
            lam = -np.log1p(-rho_d)
            b_side = (dm + lam + ULP_EXP_LOG * (np.abs(np.log(d)) + lam)) * (1.0 + U) + U * np.abs(sd["side"])
            if name == "pos":
                bound_loss += b_side[ref["present"]].sum() / max(ref["ncp"], 1)
            else:
                bound_loss += b_side.sum() / c
        return bound_g, bound_loss + (U + 2.0 ** -40) * abs(ref["loss"])
    t, big_m, e, d, pos, lab, nl = ref["t"], ref["M"], ref["e"], ref["d"], ref["pos"], ref["labelled"], max(ref["nl"], 1)
    gl = float(gamma(-(-c // 64) + 7))
    dt = a * ds * (1.0 + g2) + g2 * np.abs(t)
    dm = dt.max(1)[:, None]
    z = t - big_m[:, None]
    dz = dt + dm + U * (np.abs(z) + dt + dm)
    rho = _rho(dz)
    rho_d = ((rho * e).sum(1) / d * (1.0 + gl) + gl + c * 2.0 ** -126)[:, None]
    assert np.all(rho_d[lab] < 0.5), "the similarity error is too large for a meaningful bound"
    rho_d = np.minimum(rho_d, 0.5)
    wgt = e / d[:, None]
    bw = wgt * ((rho + rho_d) / (1.0 - rho_d) * (1.0 + U) + U) + TINY
    v = wgt - pos
    bv = np.where(pos, bw + U * (np.abs(v) + bw), bw)
    kk = a / nl
    bound_g = np.where(lab[:, None], kk * ((1.0 + g2) * bv + g2 * np.abs(v)) + TINY, 0.0)
    lam = -np.log1p(-rho_d[:, 0])
    dzy = np.where(pos, dz, 0.0).sum(1)
    b_l = np.where(lab, (lam + ULP_EXP_LOG * (np.log(d) + lam) + dzy) * (1.0 + U) + U * np.abs(ref["ell"]), 0.0)
    return bound_g, b_l.sum() / nl + (U + 2.0 ** -40) * abs(ref["loss"])


# ---- the cases the CPU and the GPU test share (p, k, e, c): n = p k samples of p of the c classes -------------------------------------
SIGMA = 0.8
SMALL_SHAPES = [(8, 4, 256, 24), (32, 4, 256, 100), (3, 3, 64, 5), (5, 7, 33, 70), (16, 16, 128, 16), (4, 4, 64, 2),
                (4, 4, 96, 4000),                           # e + c = 4096: the last c of the small path at this e
                (128, 4, 256, 256),                         # n c e = 2^25: the last product of the small path
                (4, 4, 16, 511), (4, 4, 16, 512)]           # the backward splits demb's class sum from c = 512 on (few samples)
MATRIX_SHAPES = [(4, 4, 96, 4001),                          # e + c = 4097
                 (128, 4, 257, 256),                        # n c e just above 2^25
                 (512, 8, 32, 600),                         # n = 4096
                 (4, 4, 64, 4100),
                 (4, 4, 8, 16384)]                          # the largest c
SHAPES = SMALL_SHAPES + MATRIX_SHAPES
RAGGED = (64, 40)                                           # (e, c) of the ragged general-label batch


def seed_of(p, k, e):
    return p * 1000 + k * 10 + e


def underflow_trap():
    """Logit spreads of 200 / 40 / 0 (alpha = scale = 200 on S = 1, 0.2, 0): under a maximum that is not the set's own, e^(40 - 200)
    and e^(0 - 200) underflow in fp32 and a logarithm is taken of 0.  Three unit proxies on the axes; sample 0 = (1, 0.2, 0) has the
    CosFace logits 200 / 40 / 0, class 0's members have S = 1, 0.2, 0.  -> (x [5, 3], w [3, 3], labels, a = 200)."""
    x = np.array([[1.0, 0.2, 0.0], [0.2, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.2, 1.0]], np.float32)
    return x, np.eye(3, dtype=np.float32), np.array([0, 0, 0, 1, 2], np.int32), 200.0
