"""The learnable class proxies of the proxy / classification losses (ops.proxy_anchor_loss, ops.proxy_softmax_loss: one vector per
class; ops.soft_triple_loss, ops.arcface_loss: centers_per_class vectors per class), trained beside the backbone by
train_step.ProxyTrainer."""
import math

import torch


class ProxyHead(torch.nn.Module):
    """One parameter `proxies` [n_classes * centers_per_class, embedding_size], class-major: rows c kc .. c kc + kc - 1 are the
    centres of class c (kc = centers_per_class; 1, the default, is one proxy per class).  Kaiming-normal, mode fan_out, as the
    Proxy-Anchor authors' code initialises them: std = sqrt(2 / rows).  The values are drawn on the CPU from a generator seeded by
    `seed`, so every rank of a data-parallel run starts from the same proxies whatever its device's generator has drawn before."""

    def __init__(self, n_classes, embedding_size, seed=0, centers_per_class=1):
        super().__init__()
        n_classes, embedding_size, kc = int(n_classes), int(embedding_size), int(centers_per_class)
        if n_classes < 2 or embedding_size < 1:
            raise ValueError(f"ProxyHead: need n_classes >= 2 and embedding_size >= 1 (got {n_classes}, {embedding_size})")
        if kc < 1 or kc != centers_per_class:
            raise ValueError(f"ProxyHead: centers_per_class must be a whole number >= 1 (got {centers_per_class!r})")
        gen = torch.Generator(device="cpu").manual_seed(int(seed))
        rows = n_classes * kc
        w = torch.randn(rows, embedding_size, generator=gen, dtype=torch.float32) * math.sqrt(2.0 / rows)
        self.proxies = torch.nn.Parameter(w)
        self._centers_per_class = kc

    @property
    def n_classes(self):
        return self.proxies.shape[0] // self._centers_per_class

    @property
    def centers_per_class(self):
        return self._centers_per_class

    def forward(self):
        return self.proxies
