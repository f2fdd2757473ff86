"""float64 restatement of the cross-batch memory (include/embnet.h, csrc/xbm.hip): the ring, the two losses of a batch against a detached
bank, their gradient and counters, and the a-priori rounding bounds the kernels are held to.  NumPy only, no kernel code.
tests/test_xbm_ref_cpu.py checks the restatement (autograd, a scalar triple loop, ms_ref on a bank that is the batch, hand cases, the
ring against a Python list) and the fitness of the GPU test's inputs; tests/test_xbm_gpu.py checks the kernels against it.

Semantics (the header's).  X [n, e] fp32 with labels y [n], bank Y [m, e] fp32 with labels z [m] (negative: no pair set), self [n] or
None (a column in [0, m) that anchor i leaves out).  S = X Y^T.  For y_i >= 0:  P_i = {j: z_j = y_i, j != self_i},
N_i = {j: z_j >= 0, z_j != y_i}.  The scalar parameters ROUNDED TO fp32.
    'contrastive'       p kept iff fl(1 - S_ip) > 0, term fl(1 - S_ip), G = -1;  n kept iff S_in > margin, term S_in, G = +1;
                        l_i = the sum of the kept terms.
    'multi_similarity'  ms_ref's mining rule, t, stable sides, l_i and G, over P_i and N_i.
    loss = sum_i l_i / n (n counts every row);  demb = (g / n) G Y;  counts = {kept positives, kept negatives, anchors that keep a
    pair, labelled bank slots}.
The ring (Ring): row i of a batch goes to slot (cursor + i) mod m, the cursor advances by the batch.

Bounds.  u = 2^-24, gamma(n) = n u / (1 - n u) (ms_ref.gamma).  Nothing is measured; the rounding counts are read off xbm.hip.
  S.  embnet_dense_dgrad_f32's k-ordered chain, a rounded product and a rounded addition per k:  |S~ - S| <= dS = gamma(e + 1) A,
      A_ij = sum_k |x_ik y_jk|.  Grid inputs (x and y multiples of 1 / q, A q^2 <= 2^24): S~ = S in any order, gamma_S = 0.
  'contrastive'.  A kept positive's term is t~ = fl(1 - S~): |t~ - (1 - S)| <= dS + u (|1 - S| + dS); a kept negative's term is S~
      itself: dS.  The terms are fp32 numbers; a lane adds at most ceil(m / 64) of them in float64, the butterfly adds six times:
      |l~_i - l_i| <= sum_kept (term bounds) + (ceil(m / 64) + 7) 2^-53 T_i (1 + ...), T_i = sum_kept |term| + term bounds.
      G is -1, +1 or 0: exact wherever the decision is sure.
  'multi_similarity'.  ms_ref's chain of bounds (t, m, z, e, d, G, side, l_i) on the rectangle: the lane chains of BOTH sides run
      over the m columns, L = ceil(m / 64) + 7.
  loss.  The sum over the anchors and the division by n are float64 on the device, the cast rounds once:
      |loss~ - loss| <= mean_i bound(l_i) + u |loss| + 2^-40 mean_i T_i.
  backward, against float64 of the DEVICE's own G: a float64 fma chain of m terms, the scale g / n, one fp32 rounding:
      |demb~ - demb| <= u |demb| + (m + 8) 2^-53 (|g| / n) sum_j |G_ij| |y_jk| + 2^-149.

Open decisions.  The device's S~ is SOME fp32 number in [S - dS, S + dS]; fl is monotone, so a pair is surely kept / surely dropped
when its comparison (S > margin, fl(1 - S) > 0, and multi-similarity's two mining tests) gives the same answer at both ends of
every interval involved.  A pair that is neither is OPEN: either answer is correct there, and the anchor is judged with the device's
own decision.
"""
import numpy as np

from ms_ref import TINY, U, ULP_EXP_LOG, gamma, grid_q

KINDS = ("contrastive", "multi_similarity")
DEFAULTS = {"contrastive": dict(margin=0.5), "multi_similarity": dict(alpha=2.0, beta=50.0, base=0.5, epsilon=0.1)}
MAX_N, MAX_M, MAX_E, MAX_PAIRS = 4096, 65536, 4096, 2 ** 26


def in_range(n, m, e):
    return 2 <= n <= MAX_N and n <= m <= MAX_M and n * m <= MAX_PAIRS and 1 <= e <= MAX_E


def workspace_bytes(n, m, e):
    """embnet_xbm_loss_workspace_bytes restated."""
    if not in_range(n, m, e):
        return 0
    a16 = lambda b: (b + 15) // 16 * 16
    return 16 + a16(8 * n) + 16 * n + a16(4 * n * m)


def gamma_s(e, exact=False):
    return 0.0 if exact else float(gamma(e + 1))


def params32(kind, **params):
    """The kind's parameters, defaults filled in, as the C ABI sees them: rounded to fp32 (returned as Python floats)."""
    assert kind in KINDS and set(params) <= set(DEFAULTS[kind]), (kind, params)
    return {k: float(np.float32(params.get(k, v))) for k, v in DEFAULTS[kind].items()}


# ---- the ring -------------------------------------------------------------------------------------------------------------------------
class Ring:
    """The header's ring on the host: feats [m, e] zeros, labels [m] -1, cursor 0."""

    def __init__(self, m, e):
        self.feats, self.labels, self.cursor = np.zeros((m, e), np.float32), np.full(m, -1, np.int32), 0

    def enqueue(self, emb, labels):
        m = self.feats.shape[0]
        assert 1 <= len(emb) <= m
        slots = ((self.cursor + np.arange(len(emb))) % m).astype(np.int32)
        self.feats[slots], self.labels[slots] = emb, labels
        self.cursor = int((self.cursor + len(emb)) % m)
        return slots


# ---- pair sets, similarity --------------------------------------------------------------------------------------------------------------
def sets(labels, mem_labels, self_slots=None):
    """-> (pos [n, m], neg [n, m]) bool."""
    y, z = np.asarray(labels, np.int64), np.asarray(mem_labels, np.int64)
    ok = (y >= 0)[:, None] & (z >= 0)[None, :]
    same = y[:, None] == z[None, :]
    pos, neg = ok & same, ok & ~same
    if self_slots is not None:
        own = np.asarray(self_slots, np.int64)[:, None] == np.arange(len(z))[None, :]      # a slot outside [0, m) matches nothing
        pos, neg = pos & ~own, neg & ~own
    return pos, neg


def similarity(x, mem):
    """-> (S [n, m], A [n, m]) float64."""
    x, mem = np.asarray(x, np.float32).astype(np.float64), np.asarray(mem, np.float32).astype(np.float64)
    return x @ mem.T, np.abs(x) @ np.abs(mem).T


def exact_in_any_order(x, mem, unit):
    """True iff x and mem are integer multiples of `unit` and sum_k |x_ik y_jk| <= 2^24 unit^2 everywhere: S is exact in fp32 in any
    order, with or without fma."""
    mx, my = np.asarray(x, np.float64) / unit, np.asarray(mem, np.float64) / unit
    return bool(np.array_equal(mx, np.round(mx)) and np.array_equal(my, np.round(my)) and (np.abs(mx) @ np.abs(my).T).max() <= 2 ** 24)


# ---- decisions --------------------------------------------------------------------------------------------------------------------------
def _row_min(v, mask):
    return np.where(mask, v, np.float32(np.inf)).min(1)


def _row_max(v, mask):
    return np.where(mask, v, np.float32(-np.inf)).max(1)


def _keep(kind, pos_s, neg_s, mn_s, mx_s, pos, neg, par):
    """The header's comparisons in fp32 arithmetic.  pos_s / neg_s: the fp32 S a positive's / a negative's own test reads; mn_s / mx_s:
    the fp32 S the minimum over the positives / the maximum over the negatives is taken of (multi-similarity)."""
    if kind == "contrastive":
        return pos & ((np.float32(1) - pos_s) > 0), neg & (neg_s > np.float32(par["margin"]))
    eps = np.float32(par["epsilon"])
    mn, mx = _row_min(mn_s, pos), _row_max(mx_s, neg)
    return pos & ((mx + eps)[:, None] > pos_s), neg & ((neg_s + eps) > mn[:, None])


def keep_sets(kind, s32, pos, neg, par):
    """-> (keep_pos, keep_neg) bool [n, m] on an fp32 S."""
    s32 = np.asarray(s32, np.float32)
    return _keep(kind, s32, s32, s32, s32, pos, neg, par)


def decisions(kind, x, labels, mem, mem_labels, self_slots, gs, **params):
    """For S~ anywhere in [S - gs A, S + gs A]: -> dict(sure_pos, may_pos, sure_neg, may_neg, open [n, m], share): pairs kept at every
    admissible S~, pairs kept at some, the pairs where the two differ and their share of all the pairs in a set."""
    par = params32(kind, **params)
    s, a = similarity(x, mem)
    lo, hi = (s - gs * a).astype(np.float32), (s + gs * a).astype(np.float32)
    pos, neg = sets(labels, mem_labels, self_slots)
    # a positive is kept the more readily the SMALLER its S and the larger the negatives' maximum; a negative the LARGER its S and
    # the smaller the positives' minimum
    sure_pos, sure_neg = _keep(kind, hi, lo, hi, lo, pos, neg, par)
    may_pos, may_neg = _keep(kind, lo, hi, lo, hi, pos, neg, par)
    opened = (sure_pos != may_pos) | (sure_neg != may_neg)
    return dict(sure_pos=sure_pos, may_pos=may_pos, sure_neg=sure_neg, may_neg=may_neg, open=opened,
                share=float(opened.sum()) / max(int((pos | neg).sum()), 1))


# ---- the losses -------------------------------------------------------------------------------------------------------------------------
def _side(t, keep):
    """Stable log-sum-exp of one side (ms_ref._side).  -> (m [n], e [n, m] = exp(t - m) on the kept pairs, e0 [n], d [n])."""
    m = np.maximum(np.where(keep, t, -np.inf).max(1), 0.0)
    e = np.where(keep, np.exp(np.where(keep, t - m[:, None], 0.0)), 0.0)
    e0 = np.exp(-m)
    return m, e, e0, e0 + e.sum(1)


def reference(kind, x, labels, mem, mem_labels, self_slots=None, keep=None, **params):
    """float64 loss, per-anchor losses, G [n, m] and counts.  keep = (keep_pos, keep_neg) overrides the decisions (they are constants
    of the loss: autograd checks, and open pairs judged with the device's own decision)."""
    par = params32(kind, **params)
    s, a = similarity(x, mem)
    n, m = s.shape
    pos, neg = sets(labels, mem_labels, self_slots)
    keep_pos, keep_neg = keep_sets(kind, s.astype(np.float32), pos, neg, par) if keep is None else keep
    assert not (keep_pos & ~pos).any() and not (keep_neg & ~neg).any()
    out = dict(kind=kind, par=par, S=s, A=a, pos=pos, neg=neg, keep_pos=keep_pos, keep_neg=keep_neg, n=n, m=m)
    if kind == "contrastive":
        terms = np.where(keep_pos, 1.0 - s, 0.0) + np.where(keep_neg, s, 0.0)
        ell = terms.sum(1)
        g = keep_neg.astype(np.float64) - keep_pos.astype(np.float64)
        active = (keep_pos | keep_neg).any(1)
        out.update(terms=terms)
    else:
        al, be, ba = par["alpha"], par["beta"], par["base"]
        tp, tn = -al * (s - ba), be * (s - ba)
        mp, ep, e0p, dp = _side(tp, keep_pos)
        mg, en, e0n, dn = _side(tn, keep_neg)
        active = keep_neg.any(1)
        assert np.array_equal(active, keep_pos.any(1)) or keep is not None
        side_p = np.where(active, (mp + np.log(dp)) / al, 0.0)
        side_n = np.where(active, (mg + np.log(dn)) / be, 0.0)
        ell = side_p + side_n
        g = np.where(active[:, None], en / dn[:, None] - ep / dp[:, None], 0.0)
        out.update(sides=dict(pos=dict(c=al, t=tp, m=mp, e=ep, e0=e0p, d=dp, side=side_p, keep=keep_pos),
                              neg=dict(c=be, t=tn, m=mg, e=en, e0=e0n, d=dn, side=side_n, keep=keep_neg)))
    counts = np.array([keep_pos.sum(), keep_neg.sum(), active.sum(), (np.asarray(mem_labels) >= 0).sum()], np.int64)
    out.update(loss=ell.sum() / n, ell=ell, G=g, counts=counts, active=active)
    return out


def scalar_reference(kind, x, labels, mem, mem_labels, self_slots=None, **params):
    """The same by a triple loop over anchors, slots and components, nothing vectorised.  -> (loss, G, counts)."""
    par = params32(kind, **params)
    x, mem = np.asarray(x, np.float32), np.asarray(mem, np.float32)
    n, m, e = len(x), len(mem), x.shape[1]
    g = np.zeros((n, m))
    total, cp, cn, act = 0.0, 0, 0, 0
    for i in range(n):
        if labels[i] < 0:
            continue
        sim, role = [0.0] * m, [0] * m
        for j in range(m):
            acc = 0.0
            for k in range(e):
                acc += float(x[i, k]) * float(mem[j, k])
            sim[j] = acc
            if mem_labels[j] >= 0 and not (self_slots is not None and self_slots[i] == j):
                role[j] = 1 if mem_labels[j] == labels[i] else -1
        s32 = [np.float32(v) for v in sim]
        if kind == "contrastive":
            kept = 0
            for j in range(m):
                if role[j] > 0 and np.float32(1) - s32[j] > 0:
                    total += 1.0 - sim[j]; g[i, j] = -1.0; cp += 1; kept += 1
                elif role[j] < 0 and s32[j] > np.float32(par["margin"]):
                    total += sim[j]; g[i, j] = 1.0; cn += 1; kept += 1
            act += kept > 0
            continue
        ps, ns = [j for j in range(m) if role[j] > 0], [j for j in range(m) if role[j] < 0]
        if not ps or not ns:
            continue
        eps = np.float32(par["epsilon"])
        mn, mx = min(s32[j] for j in ps), max(s32[j] for j in ns)
        kp = [j for j in ps if mx + eps > s32[j]]
        kn = [j for j in ns if s32[j] + eps > mn]
        if not kn:
            continue
        al, be, ba = par["alpha"], par["beta"], par["base"]
        zp = 1.0 + sum(np.exp(-al * (sim[j] - ba)) for j in kp)
        zn = 1.0 + sum(np.exp(be * (sim[j] - ba)) for j in kn)
        total += np.log(zp) / al + np.log(zn) / be
        for j in kp:
            g[i, j] = -np.exp(-al * (sim[j] - ba)) / zp
        for j in kn:
            g[i, j] = np.exp(be * (sim[j] - ba)) / zn
        cp += len(kp); cn += len(kn); act += 1
    return total / n, g, np.array([cp, cn, act, sum(1 for v in mem_labels if v >= 0)], np.int64)


def grad(mem, g, upstream=1.0):
    """float64 demb = (upstream / n) G Y and its bound (module docstring), from a given G [n, m]."""
    mem, g = np.asarray(mem, np.float32).astype(np.float64), np.asarray(g, np.float64)
    n, m = g.shape
    up = float(np.float32(upstream))
    want = (up / n) * (g @ mem)
    bound = U * np.abs(want) + (m + 8) * 2.0 ** -53 * (abs(up) / n) * (np.abs(g) @ np.abs(mem)) + 2.0 ** -149
    return want, bound


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------
def bounds(ref, gs):
    """-> (bound_G [n, m], bound_ell [n], bound_loss) for a device whose S is within gs A of the truth (module docstring)."""
    n, m = ref["n"], ref["m"]
    ds = gs * ref["A"]
    lanes = -(-m // 64)
    if ref["kind"] == "contrastive":
        b_term = np.where(ref["keep_pos"], ds + U * (np.abs(1.0 - ref["S"]) + ds), 0.0) + np.where(ref["keep_neg"], ds, 0.0)
        t_abs = np.abs(ref["terms"]).sum(1) + b_term.sum(1)
        bound_ell = b_term.sum(1) + (lanes + 7) * 2.0 ** -53 * t_abs
        bound_loss = bound_ell.sum() / n + U * abs(ref["loss"]) + 2.0 ** -40 * t_abs.sum() / n
        return np.zeros((n, m)), bound_ell, bound_loss
    g2 = float(gamma(2))
    gl = float(gamma(lanes + 7))
    bound_g, bound_ell = np.zeros((n, m)), np.zeros(n)
    for name in ("pos", "neg"):
        sd = ref["sides"][name]
        keep, c, t, mm, e, e0, d = sd["keep"], sd["c"], sd["t"], sd["m"], sd["e"], sd["e0"], sd["d"]
        dt = np.where(keep, c * ds * (1.0 + g2) + g2 * np.abs(t), 0.0)
        dm = dt.max(1)
        z = np.where(keep, t - mm[:, None], 0.0)
        dz = dt + dm[:, None] + U * (np.abs(z) + dt + dm[:, None])
        rho = np.where(keep, np.expm1(dz) + ULP_EXP_LOG * np.exp(dz), 0.0)
        rho0 = np.expm1(dm) + ULP_EXP_LOG * np.exp(dm)
        rho_d = ((rho * e).sum(1) + rho0 * e0) / d * (1.0 + gl) + gl
        assert np.all(rho_d < 0.5), "the similarity error is too large for a meaningful bound"
        w = e / d[:, None]
        bound_g += np.where(keep, w * ((rho + rho_d[:, None]) / (1.0 - rho_d[:, None]) * (1.0 + U) + U) + TINY, 0.0)
        lam = -np.log1p(-rho_d)
        b_side = (dm + lam + ULP_EXP_LOG * (np.abs(np.log(d)) + lam)) * (1.0 + g2) / c + g2 * np.abs(sd["side"])
        bound_ell += np.where(ref["active"], b_side, 0.0)
    bound_ell = bound_ell + U * (np.abs(ref["ell"]) + bound_ell)
    return bound_g, bound_ell, bound_ell.sum() / n + (U + 2.0 ** -40) * abs(ref["loss"])


# ---- the inputs the CPU and the GPU test share ----------------------------------------------------------------------------------------
SIGMA = 0.8
CASES = ("bank_is_batch", "ragged", "ragged_one_class", "trips", "edge", "low_end", "grid")
SHAPES = dict(bank_is_batch=(8, 8, 4), ragged=(12, 40, 5), ragged_one_class=(12, 40, 5), trips=(20, 4160, 130), edge=(8, 65536, 16),
              low_end=(4, 4, 1), grid=(128, 1024, 128))


def _clustered(seed, p, k, e, sigma=SIGMA):
    from recipes import clustered_embeddings
    return clustered_embeddings(seed, p, k, e, sigma)


def _split(seed, p, k, m, e, cursor, empty=0):
    """p classes with global indices out of 100: k rows each form the class-contiguous batch, the others the shuffled bank of m
    slots (`empty` of them empty: zero rows, label -1); the batch is then enqueued at `cursor`, wrapping.
    -> (x, labels, mem, mem_labels, self_slots)."""
    per = -(-m // p)
    full = _clustered(seed, p, k + per, e).reshape(p, k + per, e)
    r = np.random.RandomState(seed + 1)
    cls = r.permutation(100)[:p].astype(np.int32)
    x, lab = full[:, :k].reshape(p * k, e), np.repeat(cls, k)
    rest, rlab = full[:, k:].reshape(p * per, e), np.repeat(cls, per)
    order = r.permutation(p * per)[:m]
    ring = Ring(m, e)
    ring.feats[:], ring.labels[:] = rest[order], rlab[order]
    gone = (cursor + p * k + np.arange(empty)) % m            # right behind where the batch will land
    ring.feats[gone], ring.labels[gone] = 0, -1
    ring.cursor = cursor
    slots = ring.enqueue(x, lab)
    return x, lab.astype(np.int32), ring.feats, ring.labels, slots


def case_inputs(name):
    """-> dict(x, labels, mem, mem_labels, self_slots, unit (grid inputs: the grid step, else None), params per kind)."""
    n, m, e = SHAPES[name]
    unit, params = None, {k: {} for k in KINDS}
    if name == "bank_is_batch":                             # the class-contiguous 4 x 2 batch is the whole bank
        x = _clustered(842, 4, 2, e)
        lab = np.repeat(np.arange(4), 2).astype(np.int32)
        mem, mlab, slots = x.copy(), lab.copy(), np.arange(n, dtype=np.int32)
    elif name in ("ragged", "ragged_one_class"):
        # 4 classes x 3; slots 6 .. 10 are empty; the batch lands on slots 34 .. 39, 0 .. 5 (it wraps the ring's end)
        x, lab, mem, mlab, slots = _split(1240, 4, 3, m, e, cursor=34, empty=5)
        r = np.random.RandomState(5)
        x, lab, slots = x.copy(), lab.copy(), slots.copy()
        lab[[4, 9]] = (-1, -7)                              # two unlabelled rows (their copies in the bank are unlabelled too)
        mlab[slots[[4, 9]]] = (-1, -7)
        order = r.permutation(n)                            # ragged, shuffled labels
        x, lab, slots = x[order], lab[order], slots[order]
        only = int(lab[lab >= 0][0])                        # one class present only in the batch: its bank rows change class
        other = int(lab[(lab >= 0) & (lab != only)][0])
        own = np.zeros(m, bool)
        own[slots] = True
        mlab[(mlab == only) & ~own] = other
        row = int(np.flatnonzero(lab == other)[0])          # one self slot = -1: that row's slot holds another class's sample
        mem[slots[row]], mlab[slots[row]] = _clustered(77, 1, 1, e)[0], 100
        slots[row] = -1
        if name == "ragged_one_class":                      # one anchor's class fills the whole (labelled) bank
            mlab[mlab >= 0] = other
    elif name == "trips":                                   # 65 lane trips and a tail of 0; e over one 128 chunk
        x, lab, mem, mlab, slots = _split(4160, 5, 4, m, e, cursor=4150, empty=3)
    elif name == "edge":
        x, lab, mem, mlab, slots = _split(655, 4, 2, m, e, cursor=65532, empty=100)
    elif name == "low_end":
        x = np.array([[0.5], [0.75], [1.0], [0.25]], np.float32)
        lab = np.array([3, 3, 9, 9], np.int32)
        mem, mlab, slots = np.array([[1.0], [0.5], [0.75], [0.25]], np.float32), np.array([3, 9, 3, 9], np.int32), np.array([2, 0, 1, 3], np.int32)
        mem[slots] = x
        mlab[slots] = lab
        unit = 0.25                                         # every product is exact: S = 1/2 meets the margin exactly, and is dropped
    else:
        assert name == "grid", name
        x, lab, mem, mlab, slots = _split(128, 32, 4, m, e, cursor=1000, empty=0)
        q = grid_q(e)
        rnd = lambda a: (np.round(np.asarray(a, np.float64) * q) / q).astype(np.float32)
        x, mem, unit = rnd(x), rnd(mem), 1.0 / q
        mem[slots] = x
        params["multi_similarity"] = dict(epsilon=13.0 / 128.0 + 1.0 / (2.0 * q * q))       # ms_ref.grid_inputs: half a step off S's grid
    out = dict(x=np.ascontiguousarray(x, np.float32), labels=np.ascontiguousarray(lab, np.int32),
               mem=np.ascontiguousarray(mem, np.float32), mem_labels=np.ascontiguousarray(mlab, np.int32),
               self_slots=np.ascontiguousarray(slots, np.int32))
    assert out["x"].shape == (n, e) and out["mem"].shape == (m, e)
    for v in out.values():
        v.setflags(write=False)
    out.update(unit=unit, params=params)
    return out
