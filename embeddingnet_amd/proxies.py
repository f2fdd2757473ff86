"""The learnable class proxies of the proxy / classification losses (ops.proxy_anchor_loss, ops.proxy_softmax_loss): one vector
per class, trained beside the backbone by train_step.ProxyTrainer."""
import math

import torch


class ProxyHead(torch.nn.Module):
    """One parameter `proxies` [n_classes, embedding_size].  Kaiming-normal, mode fan_out, as the Proxy-Anchor authors' code
    initialises them: std = sqrt(2 / n_classes).  The values are drawn on the CPU from a generator seeded by `seed`, so every rank
    of a data-parallel run starts from the same proxies whatever its device's generator has drawn before."""

    def __init__(self, n_classes, embedding_size, seed=0):
        super().__init__()
        n_classes, embedding_size = int(n_classes), int(embedding_size)
        if n_classes < 2 or embedding_size < 1:
            raise ValueError(f"ProxyHead: need n_classes >= 2 and embedding_size >= 1 (got {n_classes}, {embedding_size})")
        gen = torch.Generator(device="cpu").manual_seed(int(seed))
        w = torch.randn(n_classes, embedding_size, generator=gen, dtype=torch.float32) * math.sqrt(2.0 / n_classes)
        self.proxies = torch.nn.Parameter(w)

    @property
    def n_classes(self):
        return self.proxies.shape[0]

    def forward(self):
        return self.proxies
