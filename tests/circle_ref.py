"""float64 restatement of Circle loss (include/embnet.h; csrc/circle_loss.hip in the batch, csrc/xbm.hip against the memory ring, both on
csrc/pair_loss.h's circle_row) and the a-priori rounding bounds its kernels are held to.  NumPy only, no kernel code.
tests/test_circle_ref_cpu.py checks the restatement (autograd with alpha detached, an fp32 emulation of the rounding form, hand cases)
and the fitness of the GPU test's inputs; tests/test_circle_loss_gpu.py checks the kernels against it.

Semantics (the header's).  m and gamma ROUNDED TO fp32 (the C ABI takes floats), and from them IN fp32  O+ = fl(1 + m), O- = -m,
D+ = fl(1 - m), D- = m.  S = X X^T over a class-contiguous P x K batch (P_i the other rows of i's class, N_i the other classes) or
S = X Mem^T against a bank (P_i, N_i by label value, negative labels and self_slots: xbm_ref.sets).  With [.]+ = max(., 0):
    alpha+_p = [O+ - S_ip]+,  a+_p = -gamma alpha+_p (S_ip - D+);    alpha-_n = [S_in - O-]+,  a-_n = gamma alpha-_n (S_in - D-);
    L+ = lse_p a+_p,  L- = lse_n a-_n,  z = L+ + L-,  l_i = softplus(z),  sigma = sigmoid(z);   alpha is a CONSTANT of the backward:
    G_ip = -sigma gamma alpha+_p e^{a+_p - L+},  G_in = +sigma gamma alpha-_n e^{a-_n - L-},  0 elsewhere.
    An anchor with an empty P_i or N_i (the ring only; also an unlabelled row) has l_i = 0 and a zero row of G.  loss = sum_i l_i / n.
    counts, on the fp32 S: batch {n (k-1), anchors with max_n S_in >= min_p S_ip, negatives with alpha- > 0}; ring {positives with
    alpha+ > 0, negatives with alpha- > 0 (both over the active anchors), active anchors, labelled bank slots}.  alpha~ > 0 exactly
    when the fp32 S~ differs from the fp32 threshold on the right side: S~ < O+, S~ > O-.

Bounds.  u = 2^-24, gamma(n) = n u / (1 - n u) (ms_ref.gamma).  Nothing is measured; the rounding counts are read off circle_row.
expf / logf are held to 3 ulp = 6 u (ms_ref.ULP_EXP_LOG).  "flush": a result below 2^-126 may become 0, an absolute TINY = 2^-125.
The constants O, D are the reference's own fp32 numbers: they carry no error.

  S.  |S~ - S| <= dS = gamma_S A, A_ij = sum_c |x_ic y_jc|.  Batch: ms_ref.gamma_s(path, E), the staging is pair_loss.h's (per-class:
      gamma(ceil(E/64) + 7); similarity matrix: gamma(E + 1)); ring: xbm_ref.gamma_s(E) = gamma(E + 1); grid inputs: 0.
  alpha.  alpha~ = [fl(O - S~)]+ (the positives; fl(S~ - O) the negatives); [.]+ is a contraction, so the clamp needs no case of its own:
      |alpha~ - alpha| <= Da = dS + u (|O - S| + dS).
  b = S - D.  b~ = fl(S~ - D):  |b~ - b| <= Db = dS + u (|b| + dS).
  q = alpha b, continuous at the clamp.  q~ = fl(alpha~ b~):  |alpha~ b~ - q| <= Dq' = alpha Db + |b| Da + Da Db,
      |q~ - q| <= Dq = Dq' (1 + u) + u |q| + TINY.
  a = -+gamma q.  a~ = fl(gamma q~):  |a~ - a| <= Dl = gamma Dq (1 + u) + u |a| + TINY.   To first order Dl = gamma (alpha + |b|) dS
      + 3 u |a|: the similarity error is amplified by gamma (alpha + |S - D|), up to 2 gamma (1 + m) on unit rows.
  lse.  The logits are NOT monotone in S, so the device takes its maxima over the logits themselves: M~ = max a~ EXACTLY.  What it
      then computes is the log-sum-exp and the softmax OF THE PERTURBED LOGITS a~, up to the roundings behind them.  Both are
      1-Lipschitz in the largest perturbation DM = max Dl over the side:  |lse(a~) - lse(a)| <= DM, and for sm_j = e^{a_j - L}
      sm(a~)_j = sm(a)_j e^{+-(Dl_j + DM)}.  (At rows of norm 30 a logit is 10^8 and Dl itself is above 1: the bounds stay finite and
      true, and say how little fp32 then knows.)
  x^ = a~ - M~ <= 0, |x^| <= X = |a - M| + Dl + DM.  x~ = fl(x^), |x~ - x^| <= u X;  e~ = expf(x~) = e^{x^} (1 + rho_B),
      rho_B = expm1(u X) + 6 u exp(u X), + flush.
  sum~ of the e~, all >= 0, the largest exactly 1.  A lane adds at most ceil(cols / 64) terms of a side (cols = the row's length: N
      in the batch, the slots of the ring), the butterfly adds six times: g_L = gamma(ceil(cols / 64) + 7), one to spare as in ms_ref.
      Term j's share of the perturbed sum is at most min(1, sm_j e^{Dl_j + DM}):
      rho_s = sum_j rho_B,j min(1, sm_j e^{Dl_j + DM}) (1 + g_L) + g_L + cols 2^-126      (must stay below 1/2).
  L = lse(a).  L~ = fl(M~ + logf(sum~)), 0 <= log sum <= log cols:  lam = -log(1 - rho_s),
      DL = DM + (lam + 6 u (log cols + lam)) (1 + u) + u (|L| + DM).
  z = L+ + L-.  z~ = fl(L+~ + L-~):  Dz = (DL+ + DL-) (1 + u) + u |z|.
  softplus is 1-Lipschitz: |softplus(z~) - softplus(z)| <= Dz.  The device forms it from t~ = expf(-|z~|) <= 1 (6 u),
      d1~ = fl(1 + t~) (relative 7 u to 1 + t^: below gamma(8)), logf(d1~) <= log 2 (6 u) and one addition:
      |l~ - l| <= Bl = Dz + (-log(1 - gamma(8)) + 6 u log 2) (1 + u) + u (l + Dz) + TINY.
  sigma.  The device forms sigmoid(z~) from t~: 1 / d1~ for z~ >= 0, t~ / d1~ otherwise.  Either form IS sigmoid(z~) up to its own
      roundings (expf 6 u, the addition u, the division u: below gamma(16) with room), whichever sign z has, and
      d log sigmoid / dz = 1 - sigmoid <= 1:  relative rho_g = e^{Dz} (1 + gamma(16)) - 1, + flush of t~.
  G = -+sigma gamma alpha sm.  G~ = fl(fl(fl(sigma~ gamma) / sum~) fl(alpha~ e~)): four roundings (gamma(4)) around
      sigma~ gamma alpha~ e~ / sum~, and e~ / sum~ = sm(a~)_j (1 + rho_B,j) / (1 + rho_s'):  with
      R_j = (1 + rho_g) e^{Dl_j + DM} (1 + rho_B,j) / (1 - rho_s) (1 + gamma(4)),   alpha's error ABSOLUTE (alpha may be 0 where
      alpha~ is not):
      |G~ - G| <= gamma sigma sm_j R_j Da + |G| (R_j - 1) + TINY (1 + gamma (1 + alpha + Da)).
      A pair with alpha = 0 has G = 0 and a bound gamma sigma sm Da: a few ulp of S times the pair's weight.
  loss.  The sum over the anchors and the division by n are float64 on the device; the final cast adds u |loss|:
      |loss~ - loss| <= mean_i Bl + (u + 2^-40) |loss|.
  backward.  Against float64 of the DEVICE's own G: ms_ref.grad in the batch, xbm_ref.grad against the ring.

Counters.  The device's S~ is SOME fp32 number in [S - dS, S + dS] (ms_ref's argument).  The violating anchors: supcon_ref.decisions.
The two alpha > 0 counters: a pair surely counts when float32(S - dS) and float32(S + dS) are both on the counting side of the fp32
threshold, possibly when one of them is; a pair within dS of its threshold is FREE to fall either way, and the device's count must
lie between the sure and the possible count.  Values need no such escape: alpha (S - D) is continuous at the clamp and Da covers it.
"""
import numpy as np

from ms_ref import TINY, U, ULP_EXP_LOG, class_masks, gamma, gamma_s, grad, grid_inputs  # noqa: F401  (re-exported for the tests)
import supcon_ref
import xbm_ref
from xbm_ref import case_inputs  # noqa: F401  (the ring cases the GPU test shares with xbm_ref's)

FREE_CAP = 0.01          # fitness of a continuous input: at most this share of its pairs within dS of a counter threshold
PARAMS = [(0.4, 80.0), (0.25, 256.0), (0.0, 1.0), (1.0, 80.0)]
BATCH_SHAPES = [(2, 2, 1), (4, 3, 1), (5, 7, 33), (9, 8, 40), (16, 16, 128), (4, 32, 16), (33, 16, 8)]
RING_CASES = ("bank_is_batch", "ragged", "ragged_one_class", "low_end", "wide", "long")


def params32(m=0.4, gamma_=80.0):
    """m, gamma and the four derived constants as the device has them: fp32 numbers, the derived ones by ONE fp32 operation."""
    m32, one = np.float32(m), np.float32(1)
    return dict(m=float(m32), gamma=float(np.float32(gamma_)), op=float(one + m32), on=-float(m32), dp=float(one - m32), dn=float(m32))


# ---- the loss on a rectangle of similarities ------------------------------------------------------------------------------------------
def _core(s, a, pos, neg, par):
    """S [n, cols] float64 with A = sum |x y|, the pair sets -> the loss, G and every intermediate bounds() reads."""
    n, cols = s.shape
    g = par["gamma"]
    active = pos.any(1) & neg.any(1)
    pos, neg = pos & active[:, None], neg & active[:, None]
    alpha = np.where(pos, np.maximum(par["op"] - s, 0.0), 0.0) + np.where(neg, np.maximum(s - par["on"], 0.0), 0.0)
    b = np.where(pos, s - par["dp"], 0.0) + np.where(neg, s - par["dn"], 0.0)
    logit = np.where(pos, -g * alpha * b, np.where(neg, g * alpha * b, 0.0))
    sides = {}
    for name, mask in (("pos", pos), ("neg", neg)):
        big = np.where(active, np.where(mask, logit, -np.inf).max(1, initial=-np.inf), 0.0)
        e = np.where(mask, np.exp(np.where(mask, logit - big[:, None], 0.0)), 0.0)
        d = np.where(active, e.sum(1), 1.0)
        sides[name] = dict(mask=mask, M=big, e=e, d=d, L=big + np.log(d))
    z = sides["pos"]["L"] + sides["neg"]["L"]
    t = np.exp(-np.abs(z))
    ell = np.where(active, np.maximum(z, 0.0) + np.log1p(t), 0.0)
    sigma = np.where(z >= 0, 1.0 / (1.0 + t), t / (1.0 + t))
    w = {k: sigma * g / sides[k]["d"] for k in sides}
    gm = alpha * (w["neg"][:, None] * sides["neg"]["e"] - w["pos"][:, None] * sides["pos"]["e"])
    s32 = s.astype(np.float32)
    return dict(par=par, S=s, A=a, pos=pos, neg=neg, active=active, n=n, cols=cols, alpha=alpha, b=b, logit=logit, sides=sides, z=z,
                t=t, sigma=sigma, w=w, ell=ell, loss=ell.sum() / n, G=np.where(active[:, None], gm, 0.0),
                count_pos=pos & (s32 < np.float32(par["op"])), count_neg=neg & (s32 > np.float32(par["on"])))


def reference(x, p, k, m=0.4, gamma_=80.0):
    """In-batch: float64 loss, per-anchor losses, G [N, N] and counts [3] of an fp32 block x."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = p * k
    assert x.shape[0] == n and p >= 2 and k >= 2
    pos, neg = class_masks(p, k)
    out = _core(x @ x.T, np.abs(x) @ np.abs(x).T, pos, neg, params32(m, gamma_))
    viol = supcon_ref.violating(out["S"].astype(np.float32), p, k)
    out.update(p=p, k=k, counts=np.array([n * (k - 1), viol.sum(), out["count_neg"].sum()], np.int64))
    return out


def xbm_reference(x, labels, mem, mem_labels, self_slots=None, m=0.4, gamma_=80.0):
    """Against a bank: float64 loss, per-anchor losses, G [n, slots] and counts [4]."""
    s, a = xbm_ref.similarity(x, mem)
    pos, neg = xbm_ref.sets(labels, mem_labels, self_slots)
    out = _core(s, a, pos, neg, params32(m, gamma_))
    out.update(counts=np.array([out["count_pos"].sum(), out["count_neg"].sum(), out["active"].sum(),
                                (np.asarray(mem_labels) >= 0).sum()], np.int64))
    return out


# ---- the counters' free pairs -----------------------------------------------------------------------------------------------------------
def decisions(ref, gs):
    """For S~ anywhere in [S - gs A, S + gs A]: -> dict(sure_pos, may_pos, sure_neg, may_neg, free [n, cols], share): the pairs that
    count at every admissible S~, at some, the pairs where the two differ and their share of all the pairs in a set."""
    s, a, par = ref["S"], ref["A"], ref["par"]
    lo, hi = (s - gs * a).astype(np.float32), (s + gs * a).astype(np.float32)
    op, on = np.float32(par["op"]), np.float32(par["on"])
    sure_pos, may_pos = ref["pos"] & (hi < op), ref["pos"] & (lo < op)
    sure_neg, may_neg = ref["neg"] & (lo > on), ref["neg"] & (hi > on)
    free = (sure_pos != may_pos) | (sure_neg != may_neg)
    return dict(sure_pos=sure_pos, may_pos=may_pos, sure_neg=sure_neg, may_neg=may_neg, free=free,
                share=float(free.sum()) / max(int((ref["pos"] | ref["neg"]).sum()), 1))


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------
def _rho(dx):
    return np.expm1(dx) + ULP_EXP_LOG * np.exp(dx)


def bounds(ref, gs):
    """-> (bound_G [n, cols], bound_ell [n], bound_loss) for a device whose S is within gs A of the truth (module docstring)."""
    par, s, n, cols = ref["par"], ref["S"], ref["n"], ref["cols"]
    g, active = par["gamma"], ref["active"]
    ds = gs * ref["A"]
    gl, g16 = float(gamma(-(-cols // 64) + 7)), float(gamma(16))
    alpha, b, logit = ref["alpha"], ref["b"], ref["logit"]
    pair = ref["pos"] | ref["neg"]
    thr = np.where(ref["pos"], par["op"] - s, s - par["on"])
    da = ds + U * (np.abs(thr) + ds)
    db = ds + U * (np.abs(b) + ds)
    dq = (alpha * db + np.abs(b) * da + da * db) * (1.0 + U) + U * np.abs(alpha * b) + TINY
    dl = np.where(pair, g * dq * (1.0 + U) + U * np.abs(logit) + TINY, 0.0)
    g4, g8 = float(gamma(4)), float(gamma(8))
    side = {}
    for name in ("pos", "neg"):
        sd = ref["sides"][name]
        mask, e, d = sd["mask"], sd["e"], sd["d"]
        dm = np.where(mask, dl, 0.0).max(1)[:, None]
        xh = np.where(mask, np.abs(logit - sd["M"][:, None]) + dl + dm, 0.0)
        rho_b = np.where(mask, np.expm1(U * xh) + ULP_EXP_LOG * np.exp(U * xh), 0.0)
        with np.errstate(over="ignore"):
            grow = np.where(mask, np.exp(np.minimum(dl + dm, 700.0)), 0.0)             # e^{Dl_j + DM}
        sm = e / d[:, None]
        rho_s = (rho_b * np.minimum(1.0, sm * grow)).sum(1) * (1.0 + gl) + gl + cols * 2.0 ** -126
        assert np.all(rho_s < 0.5), "the sums' own rounding is too large for a meaningful bound"
        lam = -np.log1p(-rho_s)
        d_l = dm[:, 0] + (lam + ULP_EXP_LOG * (np.log(cols) + lam)) * (1.0 + U) + U * (np.abs(sd["L"]) + dm[:, 0])
        side[name] = dict(rho_b=rho_b, rho_s=rho_s, DL=d_l, grow=grow, sm=sm)
    dz = (side["pos"]["DL"] + side["neg"]["DL"]) * (1.0 + U) + U * np.abs(ref["z"])
    bound_ell = np.where(active, dz + (-np.log1p(-g8) + ULP_EXP_LOG * np.log(2.0)) * (1.0 + U) + U * (ref["ell"] + dz) + TINY, 0.0)
    with np.errstate(over="ignore"):
        rho_g1 = np.exp(np.minimum(dz, 700.0)) * (1.0 + g16)                             # 1 + rho_g
    bound_g = np.zeros((n, cols))
    for name in ("pos", "neg"):
        sd, b_ = ref["sides"][name], side[name]
        big_r = rho_g1[:, None] * b_["grow"] * (1.0 + b_["rho_b"]) / (1.0 - b_["rho_s"][:, None]) * (1.0 + g4)
        bg = g * ref["sigma"][:, None] * b_["sm"] * big_r * da + np.abs(ref["G"]) * (big_r - 1.0) + TINY * (1.0 + g * (1.0 + alpha + da))
        bound_g += np.where(sd["mask"], bg, 0.0)
    bound_loss = bound_ell.sum() / n + (U + 2.0 ** -40) * abs(ref["loss"])
    return bound_g, bound_ell, bound_loss


# ---- the device's rounding form in numpy fp32 (tests/test_circle_ref_cpu.py holds it to the bounds) -----------------------------------
def _wave(v, op):
    """A wave's reduction of lane values v [n, 64]: the xor butterfly 32, 16, .. 1, in v's own precision."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, lanes ^ o])
    return v[:, 0]


def emulate32(s32, pos, neg, m=0.4, gamma_=80.0):
    """circle_row restated operation by operation in numpy fp32 on an fp32 S [n, cols]: the header's rounding form, the lane-strided
    sums in column order and the butterflies.  np.exp / np.log stand in for expf / logf.  -> (ell [n], G [n, cols]) fp32."""
    f = np.float32
    par = {k: f(v) for k, v in params32(m, gamma_).items()}
    s32 = np.asarray(s32, f)
    n, cols = s32.shape
    active = pos.any(1) & neg.any(1)
    pos, neg = pos & active[:, None], neg & active[:, None]
    alpha = np.where(pos, np.maximum(par["op"] - s32, f(0)), np.where(neg, np.maximum(s32 - par["on"], f(0)), f(0))).astype(f)
    b = np.where(pos, s32 - par["dp"], s32 - par["dn"]).astype(f)
    q = (alpha * b).astype(f)
    logit = np.where(pos, -par["gamma"] * q, par["gamma"] * q).astype(f)
    trips = -(-cols // 64)

    def lanes_of(v, fill):                                   # [n, cols] -> [n, trips, 64], column j in lane j % 64
        out = np.full((n, trips * 64), fill, f)
        out[:, :cols] = v
        return out.reshape(n, trips, 64)

    big, e, d = {}, {}, {}
    for name, mask in (("pos", pos), ("neg", neg)):
        big[name] = _wave(lanes_of(np.where(mask, logit, f(-np.inf)), f(-np.inf)).max(1), np.maximum)
        with np.errstate(invalid="ignore"):
            e[name] = np.where(mask, np.exp((logit - big[name][:, None]).astype(f)), f(0)).astype(f)
        acc = np.zeros((n, 64), f)
        for trip in range(trips):                            # a lane's chain in column order; skipped columns add an exact 0
            acc = (acc + lanes_of(e[name], f(0))[:, trip]).astype(f)
        d[name] = _wave(acc, lambda x, y: (x + y).astype(f))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = ((big["pos"] + np.log(d["pos"]).astype(f)).astype(f) + (big["neg"] + np.log(d["neg"]).astype(f)).astype(f)).astype(f)
        t = np.exp(-np.abs(z)).astype(f)
        d1 = (f(1) + t).astype(f)
        ell = (np.maximum(z, f(0)) + np.log(d1).astype(f)).astype(f)
        sg = ((np.where(z >= 0, f(1), t) / d1).astype(f) * par["gamma"]).astype(f)
        wp, wn = (sg / d["pos"]).astype(f), (sg / d["neg"]).astype(f)
    gm = np.where(pos, -(wp[:, None] * (alpha * e["pos"]).astype(f)).astype(f), (wn[:, None] * (alpha * e["neg"]).astype(f)).astype(f))
    gm = np.where((pos | neg), gm, f(0)).astype(f)
    return np.where(active, ell, f(0)).astype(f), gm


# ---- the inputs the CPU and the GPU test share ------------------------------------------------------------------------------------------
SIGMA = 0.8
RING_SHAPES = dict(xbm_ref.SHAPES, wide=(5, 70, 33), long=(12, 129, 5))


def seed_of(p, k, e):
    return 7000 + p * 1000 + k * 10 + e


def auto_path(p, k, e):
    """embnet_circle_loss_path restated: the per-class path's fit rule (ms_ref.auto_path's)."""
    n = p * k
    return "per_class" if k <= 16 and n <= 512 and k * (e + n) <= 16 * 1024 else "similarity_matrix"


def continuous(p, k, e, seed=None):
    """L2-normalised clustered rows (recipes.clustered_embeddings)."""
    from recipes import clustered_embeddings
    return clustered_embeddings(seed_of(p, k, e) if seed is None else seed, p, k, e, SIGMA)


def continuous_gs(x, path, e):
    """gamma_S of a continuous input on a forward path.  Unit rows of length 1 are +-1: their S is one exact product, gamma_S = 0."""
    from ms_ref import exact_in_any_order
    return 0.0 if e == 1 and exact_in_any_order(x, 1.0) else gamma_s(path, e)


def grid(p, k, e, seed=None):
    """-> (x on the 1/q grid: S exact in fp32 in any order, the grid step 1/q)."""
    x, _, q = grid_inputs(continuous(p, k, e, seed))
    return x, 1.0 / q


def ring_case(name):
    """xbm_ref's small cases and two of this file's: 'wide' (5 anchors of 5 classes, 70 slots: a second lane trip with a tail of 6,
    e = 33) and 'long' (4 x 3 anchors, 129 slots: a third trip of one column), both with empty slots, a wrapping batch, unlabelled
    rows on both sides and one class that only the batch has (no positive but the own copy: an inactive anchor); 'long' has a self
    slot of -1.  xbm_ref's 'ragged_one_class' has the anchor whose class fills the bank (no negative)."""
    if name not in ("wide", "long"):
        return case_inputs(name)
    n, m, e = RING_SHAPES[name]
    p, k = (5, 1) if name == "wide" else (4, 3)
    x, lab, mem, mlab, slots = xbm_ref._split(9100 + n, p, k, m, e, cursor=m - 3, empty=4)
    x, lab, mem, mlab, slots = x.copy(), lab.copy(), mem.copy(), mlab.copy(), slots.copy()
    lab[1] = -3                                              # an unlabelled row; its copy in the bank is unlabelled too
    mlab[slots[1]] = -3
    own = np.zeros(m, bool)
    own[slots] = True
    only, other = int(lab[0]), int(lab[-1])
    mlab[(mlab == only) & ~own] = other                      # anchor 0's class lives in the batch only: no positive in the ring
    if name == "long":
        slots[2] = -1                                        # a self slot that excludes nothing: the own copy is a positive at S = |x|^2
    out = dict(x=np.ascontiguousarray(x, np.float32), labels=np.ascontiguousarray(lab, np.int32),
               mem=np.ascontiguousarray(mem, np.float32), mem_labels=np.ascontiguousarray(mlab, np.int32),
               self_slots=np.ascontiguousarray(slots, np.int32))
    assert out["x"].shape == (n, e) and out["mem"].shape == (m, e)
    for v in out.values():
        v.setflags(write=False)
    out.update(unit=None, params={})
    return out
