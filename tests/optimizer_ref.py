"""The per-element contract of `embnet_optimizer_step_groups` / `embnet_optimizer_grad_norm` (include/embnet.h) restated in NumPy
float64 — test infrastructure, shared by test_optimizer_groups_cpu.py (which checks it against torch.optim and NumPy) and
test_optimizer_groups_gpu.py (which checks the kernels against it).

Per tensor with a gradient, in this order:
    g' = g + l2x2 * w                                  (l2x2 = 2 * lambda of the tensor's l2 regulariser)
    clipvalue c > 0:        g' = clip(g', -c, c)
    global_clipnorm c > 0:  g' = g' * c / max(sqrt(N2), c),   N2 = sum over every tensor with a gradient of g'^2
    weight_decay:           w  = w - (lr_g * wd_g) * w        (Keras AdamW: before the rule)
    the rule at lr_g = lr * lr_mult_g                  (sgd, sgd with momentum / Nesterov, rms_prop, adam, radam: Keras' forms)
A tensor without a gradient is skipped entirely and is not in N2.  t counts from 1.
"""
import numpy as np


def folded_gradients(params, grads, l2x2):
    """g' = g + l2x2 w per tensor (None stays None)."""
    return [None if g is None else np.asarray(g, np.float64) + l2x2.get(i, 0.0) * params[i] for i, g in enumerate(grads)]


def clip_gradients(grads, clipvalue=0.0, global_clipnorm=0.0):
    """-> (clipped gradients, N2): N2 = the sum of squares over every gradient BEFORE clipping (what grad_norm reports)."""
    n2 = float(sum(np.sum(g * g) for g in grads if g is not None))
    if clipvalue and global_clipnorm:
        raise ValueError("exclusive")
    if clipvalue:
        grads = [None if g is None else np.clip(g, -clipvalue, clipvalue) for g in grads]
    if global_clipnorm:
        s = global_clipnorm / max(np.sqrt(n2), global_clipnorm)
        grads = [None if g is None else g * s for g in grads]
    return grads, n2


class RefOptimizer:
    """groups: [dict(tensors=[indices], lr_mult=1, weight_decay=0)]; `lr` may be changed between steps.  l2: {tensor: lambda}."""

    def __init__(self, rule, lr, groups, beta_1=0.9, beta_2=0.999, rho=0.9, epsilon=1e-7, momentum=0.0, nesterov=False,
                 clipvalue=0.0, global_clipnorm=0.0, l2=None):
        assert rule in ("sgd", "rms_prop", "adam", "radam")
        self.rule, self.lr, self.groups = rule, float(lr), groups
        self.b1, self.b2, self.rho, self.eps = beta_1, beta_2, rho, epsilon
        self.momentum, self.nesterov, self.clipvalue, self.global_clipnorm = momentum, nesterov, clipvalue, global_clipnorm
        self.l2x2 = {i: float(np.float32(2.0 * lam)) for i, lam in (l2 or {}).items()}     # the descriptor holds it in fp32
        self.t, self.slots, self.n2 = 0, {}, 0.0

    def slot(self, i, name, like):
        return self.slots.setdefault((i, name), np.zeros_like(like, dtype=np.float64))

    def step(self, params, grads):
        """params: float64 arrays, updated in place; grads: arrays or None."""
        self.t += 1
        t = self.t
        gs, self.n2 = clip_gradients(folded_gradients(params, grads, self.l2x2), self.clipvalue, self.global_clipnorm)
        for grp in self.groups:
            lr = self.lr * grp.get("lr_mult", 1.0)
            wd = grp.get("weight_decay", 0.0)
            for i in grp["tensors"]:
                g, w = gs[i], params[i]
                if g is None:
                    continue
                if wd:
                    w -= lr * wd * w
                if self.rule == "sgd":
                    if self.momentum:
                        v = self.slot(i, "slot1", w)
                        v[...] = self.momentum * v - lr * g
                        w += self.momentum * v - lr * g if self.nesterov else v
                    else:
                        w -= lr * g
                elif self.rule == "rms_prop":
                    rms = self.slot(i, "slot1", w)
                    rms[...] = self.rho * rms + (1 - self.rho) * g * g
                    w -= lr * g / (np.sqrt(rms) + self.eps)
                else:
                    m, v = self.slot(i, "slot1", w), self.slot(i, "slot2", w)
                    m[...] = self.b1 * m + (1 - self.b1) * g
                    v[...] = self.b2 * v + (1 - self.b2) * g * g
                    if self.rule == "adam":
                        w -= lr * np.sqrt(1 - self.b2 ** t) / (1 - self.b1 ** t) * m / (np.sqrt(v) + self.eps)
                        continue
                    m_hat = m / (1 - self.b1 ** t)
                    sma_inf = 2.0 / (1 - self.b2) - 1.0
                    sma_t = sma_inf - 2.0 * t * self.b2 ** t / (1 - self.b2 ** t)
                    if sma_t >= 5:
                        r_t = np.sqrt((sma_t - 4) / (sma_inf - 4) * (sma_t - 2) / (sma_inf - 2) * sma_inf / sma_t)
                        w -= lr * r_t * m_hat / (np.sqrt(v / (1 - self.b2 ** t)) + self.eps)
                    else:
                        w -= lr * m_hat
