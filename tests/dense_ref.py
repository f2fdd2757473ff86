"""NumPy restatement of the Dense layer (csrc/dense.hip): Y = act(X W + b), dX = dY W^T, dW = X^T dY, with X [m, in], W [in, out]
(Keras layout), Y [m, out].  No kernel code: float64 products, the per-element magnitude sum |a||b| they are judged against, the
k-ordered float32 chain that is the project's yardstick for "only fp32 accumulation lies in between"
(tests/test_backbone_gpu.py::test_conv2d_products_are_fp32_accurate, tests/test_three_product_elementwise_gpu.py), the two operand
families the CPU and the GPU test share (tests/test_dense_ref_cpu.py, tests/test_dense_elementwise_gpu.py), and the comparator.

Every pass is one matrix product a [M, K] x b [K, N]:

  fwd    a = x,    b = w     (K = in)   + bias per column, ReLU
  dgrad  a = dy,   b = w^T   (K = out)
  wgrad  a = x^T,  b = dy    (K = batch)
"""
import numpy as np

U = 2.0 ** -24                                            # unit roundoff of float32
FACTOR, FLOOR = 2.0, 5e-7                                 # allowed |got - f64| / mag = max(FACTOR E32, FLOOR)


def _f64(t):
    return np.asarray(t, dtype=np.float64)


# ---- float64 results and magnitudes ------------------------------------------------------------------------------------------------
def fwd64(x, w, bias=None, relu=False):
    y = _f64(x) @ _f64(w)
    if bias is not None:
        y = y + _f64(bias)[None, :]
    return np.maximum(y, 0.0) if relu else y


def dgrad64(dy, w):
    return _f64(dy) @ _f64(w).T


def wgrad64(x, dy):
    return _f64(x).T @ _f64(dy)


def mag_fwd(x, w, bias=None):
    """sum_k |x||w| (+ |bias|) of every output element."""
    m = np.abs(_f64(x)) @ np.abs(_f64(w))
    return m + np.abs(_f64(bias))[None, :] if bias is not None else m


def mag_dgrad(dy, w):
    return np.abs(_f64(dy)) @ np.abs(_f64(w)).T


def mag_wgrad(x, dy):
    return np.abs(_f64(x)).T @ np.abs(_f64(dy))


# ---- the float32 chain -----------------------------------------------------------------------------------------------------------------
def chain32(a, b, k0=0, k1=None):
    """a [M, K] x b [K, N] as the k-ordered float32 chain acc = float32(acc + float32(a_k b_k)), k = k0 .. k1 - 1: vectorised over the
    output, a loop over k.  Returns float32 [M, N]."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32).T)           # [K, M]: a_k is a contiguous row
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
    k1 = a.shape[0] if k1 is None else k1
    acc = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32)
    prod = np.empty_like(acc)
    for k in range(k0, k1):
        np.multiply(a[k][:, None], b[k][None, :], out=prod)
        np.add(acc, prod, out=acc)
    return acc


def epilogue32(acc, bias=None, relu=False):
    """The forward's epilogue on a float32 accumulator: one float32 bias add, then ReLU."""
    y = np.asarray(acc, dtype=np.float32)
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float32)[None, :]
    return np.maximum(y, np.float32(0)) if relu else y


def e32_of(chain, f64, mag):
    """E32 = max |chain32 - f64| / mag over the elements with mag > 0 (0 if there are none)."""
    live = mag > 0
    if not live.any():
        return 0.0
    return float((np.abs(_f64(chain) - f64)[live] / mag[live]).max())


# ---- the operand families ------------------------------------------------------------------------------------------------------------
FAMILIES = ["ints", "reals"]


def ints(seed, shape, k):
    """Integers in [-3, 3] as float32.  k: the length of the reduction they go into — with 9 k + 3 < 2^24 every product, every partial
    sum in ANY order, and the sum plus a bias in [-3, 3] is an integer below 2^24, i.e. exact in float32: a kernel must be bit-exact."""
    assert 9 * k + 3 < 2 ** 24, k
    return np.random.RandomState(seed).randint(-3, 4, size=shape).astype(np.float32)


def int_bias(seed, n):
    """Integers in [-3, 3], no two adjacent columns equal: the cycle (col % 7) - 3 entered at a seeded point, then a seeded
    shuffle of every other pair of columns that keeps neighbours different."""
    rs = np.random.RandomState(seed)
    b = (np.arange(n) + rs.randint(0, 7)) % 7 - 3
    for c in range(1, n - 1):
        cand = int(rs.randint(-3, 4))
        if cand != b[c - 1] and cand != b[c + 1]:
            b[c] = cand
    assert n < 2 or (b[1:] != b[:-1]).all()
    return b.astype(np.float32)


def reals(seed, shape):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


BIAS_AMPLITUDE = 2.0 ** -16                               # of the `reals` bias: see operands()


def operands(family, seed, m, i, o):
    """(x [m, i], w [i, o], bias [o], dy [m, o]) float32, and a dict of the special rows / columns.

    ints   x, w, dy integers in [-3, 3] (exact in any order, see ints()), bias int_bias().
    reals  randn, and — where a dimension has at least 4 entries —
             w and dy: column c multiplied by 2^(-12 u_c), u uniform, u = 0 for one column and u = 1 for the QUIET one;
             x and dy: one row multiplied by 2^-12 (the quiet row);
             one column of w / dy and one row of x / dy exactly zero;
             one row of x and one column of w non-negative (a ReLU output on positive weights: no cancellation at that element);
           bias: randn 2^-16 — small against the loud columns, as a trained head's bias is against 12 800 products, large against
           the quiet ones: the whole-tensor metric cannot see its column, the per-element one can."""
    rs = np.random.RandomState(seed)
    if family == "ints":
        x, w, dy = ints(seed + 1, (m, i), i), ints(seed + 2, (i, o), max(i, o)), ints(seed + 3, (m, o), max(m, o))
        return x, w, int_bias(seed + 4, o), dy, {}
    assert family == "reals", family
    x, w, dy = reals(seed + 1, (m, i)), reals(seed + 2, (i, o)), reals(seed + 3, (m, o))
    bias = (reals(seed + 4, (o,)) * np.float32(BIAS_AMPLITUDE)).astype(np.float32)
    marks = {}
    if o >= 4:
        u = rs.rand(o)
        loud, quiet, zero, pos = rs.permutation(o)[:4]
        u[loud], u[quiet] = 0.0, 1.0
        scale = np.exp2(-12.0 * u).astype(np.float32)
        w, dy = w * scale[None, :], dy * scale[None, :]
        w[:, pos] = np.abs(w[:, pos])
        w[:, zero] = 0.0
        dy[:, zero] = 0.0
        marks.update(quiet_col=int(quiet), zero_col=int(zero), pos_col=int(pos))
    if m >= 4:
        quiet, zero, pos = rs.permutation(m)[:3]
        x[quiet] *= np.float32(2.0 ** -12)
        dy[quiet] *= np.float32(2.0 ** -12)
        x[pos] = np.abs(x[pos])
        x[zero] = 0.0
        dy[zero] = 0.0
        marks.update(quiet_row=int(quiet), zero_row=int(zero), pos_row=int(pos))
    return x, w, bias, dy, marks


def pass_problem(kind, x, w, bias, dy, with_bias=False, relu=False):
    """(a [M, K], b [K, N], f64 [M, N], mag [M, N], K) of a pass: chain32(a, b) is its float32 chain (before the epilogue)."""
    if kind == "fwd":
        bb = bias if with_bias else None
        return x, w, fwd64(x, w, bb, relu), mag_fwd(x, w, bb), x.shape[1]
    if kind == "dgrad":
        return dy, np.ascontiguousarray(w.T), dgrad64(dy, w), mag_dgrad(dy, w), w.shape[1]
    assert kind == "wgrad", kind
    return np.ascontiguousarray(x.T), dy, wgrad64(x, dy), mag_wgrad(x, dy), x.shape[0]


# ---- the comparator ------------------------------------------------------------------------------------------------------------------
def apriori_bound(mag, k, extra_roundings):
    """(K + extra) u / (1 - (K + extra) u) x mag: what ANY order of float32 accumulation of K rounded products, `extra_roundings`
    further float32 additions (slab adds, the bias add) included, can be off by (Higham, Accuracy and Stability, 3.1 / 3.5)."""
    n = (k + extra_roundings) * U
    assert n < 1
    return n / (1.0 - n) * mag


def check_elementwise(got, f64, mag, k, extra_roundings, e32, what=""):
    """Assert for EVERY element: (1) |got - f64| <= apriori_bound; (2) |got - f64| / mag <= max(2 E32, 5e-7); (3) got == 0 exactly
    where mag == 0.  Returns max |got - f64| / mag as a multiple of E32 (inf if E32 == 0 and there is an error; 0 if neither)."""
    got = _f64(got)
    assert got.shape == f64.shape == mag.shape, (what, got.shape, f64.shape, mag.shape)
    assert np.isfinite(got).all(), "%s: %d non-finite elements" % (what, int((~np.isfinite(got)).sum()))
    live = mag > 0
    dead = got[~live]
    assert (dead == 0).all(), "%s: %d elements with sum |a||b| = 0 are not exactly 0" % (what, int((dead != 0).sum()))
    err = np.abs(got - f64)
    over = err > apriori_bound(mag, k, extra_roundings)
    if over.any():
        at = np.unravel_index(int(np.argmax(np.where(over, err, 0))), err.shape)
        raise AssertionError("%s: %d elements beyond the a-priori fp32 bound (K = %d + %d roundings), worst at %s: |err| %.3e, "
                             "bound %.3e" % (what, int(over.sum()), k, extra_roundings, at, err[at],
                                             apriori_bound(mag, k, extra_roundings)[at]))
    if not live.any():
        return 0.0
    rel = np.where(live, err / np.where(live, mag, 1.0), 0.0)
    allowed = max(FACTOR * e32, FLOOR)
    worst = float(rel.max())
    if worst > allowed:
        at = np.unravel_index(int(np.argmax(rel)), rel.shape)
        raise AssertionError("%s: %d elements with |err| / mag above max(%g E32, %g) = %.3e (E32 %.3e), worst %.3e at %s"
                             % (what, int((rel > allowed).sum()), FACTOR, FLOOR, allowed, e32, worst, at))
    if e32 == 0.0:
        return float("inf") if worst > 0 else 0.0
    return worst / e32


# ---- the metric this file replaces (tests/test_backbone_gpu.py::test_dense_gap_add_l2) ------------------------------------------------
def old_metric(got, f64):
    """max |err| / max |ref| over the whole tensor."""
    return float(np.abs(_f64(got) - f64).max() / max(np.abs(f64).max(), 1e-30))


def old_tolerance(i):
    return 2e-5 * max(1.0, (i / 2048) ** 0.5)


# ---- outputs made wrong on purpose (the forward pass) -----------------------------------------------------------------------------------
def bf16x2(t):
    """t kept to two bf16 pieces by truncation (top 16 bits of t, top 16 bits of the rest: the first two pieces of the engine's
    three-way split): what an operand is after a silent move to a reduced split."""
    t = np.asarray(t, dtype=np.float32)
    hi = (t.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    rest = t - hi
    return hi + (rest.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


WRONG = ["bias_rolled", "last_k_dropped", "slab_left_out", "last_row_repeats", "bf16x2", "quiet_column_last_k"]


def wrong_forward(name, x, w, bias, marks, slabs=8):
    """The forward (bias, no ReLU) computed wrongly in one way, by the float32 chain; None where the shape has no room for the error."""
    m, i = x.shape
    o = w.shape[1]
    if name == "bias_rolled":                               # every column gets its left neighbour's bias
        return epilogue32(chain32(x, w), np.roll(bias, 1)) if o >= 2 else None
    if name == "last_k_dropped":                            # a K tail read one element short
        return epilogue32(chain32(x, w, 0, i - 1), bias)
    if name == "slab_left_out":                             # a K split whose finish kernel skips one slab
        per = -(-i // slabs)
        if per >= i:
            return None
        acc = np.zeros((m, o), dtype=np.float32)
        for s in range(slabs):
            if s != slabs // 2 and s * per < i:
                acc = acc + chain32(x, w, s * per, min(i, (s + 1) * per))
        return epilogue32(acc, bias)
    if name == "last_row_repeats":                          # a tail tile that writes row m - 2 into row m - 1
        if m < 2:
            return None
        y = epilogue32(chain32(x, w), bias)
        y[m - 1] = y[m - 2]
        return y
    if name == "bf16x2":
        return epilogue32(chain32(bf16x2(x), bf16x2(w)), bias)
    assert name == "quiet_column_last_k", name               # the K tail error in ONE column, the quiet one
    if "quiet_col" not in marks:
        return None
    y = epilogue32(chain32(x, w), bias)
    c = marks["quiet_col"]
    y[:, c] = epilogue32(chain32(x, w[:, c:c + 1], 0, i - 1), bias[c:c + 1])[:, 0]
    return y


# ---- the shapes (m, in, out) both test files use; the path each one takes is stated in tests/test_dense_elementwise_gpu.py ----------------
G64_SHAPES = [(1, 1, 1), (3, 33, 5), (67, 31, 66), (64, 32, 64), (65, 36, 68), (5, 70, 33)]
MISALIGNED_SHAPE = (8, 64, 64)
SPLITK_SHAPES = [((8, 2048, 128), 16), ((5, 2050, 33), 13), ((6, 2116, 36), 14), ((960, 2048, 256), 8), ((200, 2052, 800), 9)]
G128_CASES = [("fwd", (1925, 36, 1923)), ("fwd", (1928, 36, 1924)), ("dgrad", (1925, 1923, 36)), ("dgrad", (1928, 1924, 36)),
              ("wgrad", (36, 1925, 1923)), ("wgrad", (36, 1928, 1924))]
BELOW_G128 = (1920, 36, 1920)
HEAD_SHAPE, HEAD_SLABS = (4, 12800, 512), 58


def seed_of(shape):
    m, i, o = shape
    return 1000 * m + 10 * i + o
