"""Reference of the weight-averaging contract (include/embnet.h, `embnet_weight_average_update`), independent of the library:

  update_f32   NumPy float32 arithmetic, the contract's three roundings and its two special branches: the kernel's bits;
  ideal_f64    the same recurrence in float64: what the averages would be without fp32 rounding;
  coefficient  the schedule of weight_average.py, restated;
  error_bound  how far an fp32 trajectory may be from the float64 one.

The bound.  Hats are the fp32 values, e = a^ - a.  One update computes
    a^' = fl(a^ + fl(c fl(w - a^))) = ((1 - c) a^ + c w + c (w - a^) eta) (1 + e3),   |eta| <= 2u + u^2, |e3| <= u = 2^-24,
(c is the same fp32 value on both sides, and the inputs of the test are far from the subnormal range), so
    |e'| <= (1 - c) |e| + u (2 c |w - a^| + |a^'|) (1 + O(u)).
With A = max |a'| and D = max |w - a| over a tensor (ideal values; |w - a^| <= D + |e| and |a^'| <= A + |e'| add terms of order
u |e| <= u^2 A / c, below 1 % of u A while c >> 2^-24 / 0.01 = 6e-6) the per-tensor recursion
    B' = (1 - c) B + 1.01 u (2 c D + A)
bounds max |e|.  In the steady state B -> 1.01 u (A + 2 c D) / c: of order 2^-24 max|avg| / c, the fp32 EMA's known lag.  It is a
worst case (every rounding at half an ulp, all of one sign); roundings of random sign add up to about its square root.
"""
import numpy as np

U = 2.0 ** -24


def coefficient(mode, t, u, decay=0.999, warmup=True, start_iteration=0, update_every=1):
    """c of step t (1-based) after u updates, as an fp32 value (0: no update)."""
    if t < start_iteration or (t - start_iteration) % update_every:
        return np.float32(0.0)
    if mode == "swa":
        return np.float32(1.0 / (u + 1))
    if mode != "ema":
        raise KeyError(mode)
    if u == 0 and start_iteration > 0:
        return np.float32(1.0)
    beta = min(decay, (1.0 + u) / (10.0 + u)) if warmup else decay
    return np.float32(1.0 - beta)


def update_f32(avg, w, c):
    """One update of float32 arrays -> the new average (float32).  !(c > 0): unchanged; c >= 1: w's bits; otherwise three
    separately rounded float32 operations."""
    avg, w, c = np.asarray(avg, dtype=np.float32), np.asarray(w, dtype=np.float32), np.float32(c)
    if not c > 0:
        return avg.copy()
    if c >= 1:
        return w.copy()
    with np.errstate(all="ignore"):
        d = (w - avg).astype(np.float32)
        p = (c * d).astype(np.float32)
        return (avg + p).astype(np.float32)


def ideal_f64(avg, w, c):
    """The same step without fp32 rounding (c is the fp32 coefficient's value)."""
    avg, w, c = np.asarray(avg, dtype=np.float64), np.asarray(w, dtype=np.float64), float(np.float32(c))
    if not c > 0:
        return avg.copy()
    if c >= 1:
        return w.copy()
    return avg + c * (w - avg)


def error_bound(bound, c, avg_old, w, avg_new):
    """B' of the module docstring for one tensor: the ideal float64 values before and after the step."""
    c = float(np.float32(c))
    if not c > 0:
        return bound
    if c >= 1:
        return 0.0
    return (1.0 - c) * bound + 1.01 * U * (2.0 * c * float(np.abs(w - avg_old).max()) + float(np.abs(avg_new).max()))
