"""The contract of `embnet_optimizer_layerwise_norms` / `embnet_optimizer_layerwise_step` (include/embnet.h) restated in NumPy —
test infrastructure, shared by test_layerwise_ref_cpu.py (which checks it against torch.optim and the rules' own properties) and
test_layerwise_gpu.py (which checks the kernels against it).

Per tensor with a gradient, in this order (optimizer_ref.py forms and clips the gradient):
    g' = g + l2x2 * w;   clipvalue c > 0: g' = clip(g', -c, c);   global_clipnorm c > 0: g' = g' * c / max(sqrt(N2), c)
    lars   u = g' + wd_g * w
    lamb   m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  u = (m c1) / (sqrt(v c2) + eps) + wd_g * w,  c1 = 1 / (1 - b1^t), c2 = 1 / (1 - b2^t)
    W2 = sum w^2,  U2 = sum u^2,  r = eta_g sqrt(W2) / sqrt(U2) if eta_g > 0 and W2 > 0 and U2 > 0 else 1
    lars   s = lr_g r;  v = momentum v + s u;  w -= momentum v + s u if nesterov else v          (SimCLR's LARSOptimizer)
    lamb   w -= lr_g r u
A tensor without a gradient is skipped entirely; its stats are (0, 0, 1).  t counts from 1.

`fp32=True` rounds every intermediate to float32 where the kernels do (a fused multiply-add once, everything else per
operation; the two norms stay float64 sums, as on the device): the emulation the GPU test takes its bound from.
"""
import numpy as np

from optimizer_ref import clip_gradients, folded_gradients


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


class RefLayerwise:
    """groups: [dict(tensors=[indices], lr_mult=1, weight_decay=0, trust_coefficient=<the rule's default>)]; `lr` may be changed
    between steps.  l2: {tensor: lambda}.  After a step `stats[i]` = (W2, U2, r) of tensor i."""

    def __init__(self, rule, lr, groups, beta_1=0.9, beta_2=0.999, epsilon=1e-7, momentum=None, nesterov=False, clipvalue=0.0,
                 global_clipnorm=0.0, l2=None, fp32=False):
        assert rule in ("lars", "lamb")
        self.rule, self.lr, self.groups, self.fp32 = rule, float(lr), groups, fp32
        self.b1, self.b2, self.eps = beta_1, beta_2, epsilon
        self.momentum = (0.9 if rule == "lars" else 0.0) if momentum is None else momentum
        self.nesterov, self.clipvalue, self.global_clipnorm = nesterov, clipvalue, global_clipnorm
        self.l2x2 = {i: float(np.float32(2.0 * lam)) for i, lam in (l2 or {}).items()}     # the descriptor holds it in fp32
        self.t, self.slots, self.n2, self.stats = 0, {}, 0.0, {}

    def slot(self, i, name, like):
        return self.slots.setdefault((i, name), np.zeros_like(like, dtype=np.float64))

    def _gradients(self, params, grads):
        R = _f32 if self.fp32 else (lambda x: x)
        gs = [None if g is None else R(g) for g in folded_gradients(params, grads, self.l2x2)]
        if not (self.fp32 and self.global_clipnorm):
            gs, self.n2 = clip_gradients(gs, self.clipvalue, self.global_clipnorm)
            return [None if g is None else R(g) for g in gs]
        _, self.n2 = clip_gradients(gs)                                     # the device rounds the scale to fp32, then multiplies
        s = float(np.float32(self.global_clipnorm / max(np.sqrt(self.n2), self.global_clipnorm)))
        return [None if g is None else R(g * s) for g in gs]

    def step(self, params, grads):
        """params: float64 arrays, updated in place; grads: arrays or None."""
        R = _f32 if self.fp32 else (lambda x: x)
        self.t += 1
        t = self.t
        gs = self._gradients(params, grads)
        b1, b2, eps, mom = (float(R(x)) for x in (self.b1, self.b2, self.eps, self.momentum))
        c1, c2 = float(R(1.0 / (1.0 - b1 ** t))), float(R(1.0 / (1.0 - b2 ** t)))      # (fp32: from the betas the kernel holds)
        for grp in self.groups:
            lr = float(R(self.lr * grp.get("lr_mult", 1.0)))
            wd = float(R(grp.get("weight_decay", 0.0)))
            eta = float(R(grp.get("trust_coefficient", 1e-3 if self.rule == "lars" else 1.0)))
            for i in grp["tensors"]:
                g, w = gs[i], params[i]
                if g is None:
                    self.stats[i] = (0.0, 0.0, 1.0)
                    continue
                if self.rule == "lars":
                    u = R(wd * w + g)
                else:
                    m, v = self.slot(i, "slot1", w), self.slot(i, "slot2", w)
                    m[...] = R(R(1.0 - b1) * g + R(b1 * m))
                    v[...] = R(R(R(1.0 - b2) * g) * g + R(b2 * v))
                    u = R(wd * w + R(R(m * c1) / R(R(np.sqrt(R(v * c2))) + eps)))
                w2, u2 = float(np.sum(w * w)), float(np.sum(u * u))
                r = float(R(eta * np.sqrt(w2) / np.sqrt(u2))) if eta > 0 and w2 > 0 and u2 > 0 else 1.0
                self.stats[i] = (w2, u2, r)
                s = float(R(lr * r))
                if self.rule == "lars":
                    vel = self.slot(i, "slot1", w)
                    su = R(s * u)
                    vel[...] = R(mom * vel + su)
                    w[...] = R(w - (R(mom * vel + su) if self.nesterov else vel))
                else:
                    w[...] = R(w - s * u)
