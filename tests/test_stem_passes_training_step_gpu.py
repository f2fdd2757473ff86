"""One ResNet18 training step at 64x64, batch 8, taken twice from the same seed: the loss, every parameter and the moving statistics
are bit-identical.  The step runs the stem's two-pass input BatchNormalization and the banded pool backward; neither holds an atomic
sum or a launch-dependent order, so a repeat that differs in one bit is a race or an uninitialised read in one of them.
"""
import pytest
import torch

from embeddingnet_amd import backbones as B

pytestmark = pytest.mark.gpu


def one_step(dev):
    """-> (loss bits, [parameter and buffer tensors]) after one TripletTrainer step of a freshly seeded resnet18."""
    from embeddingnet_amd.optimizers import KerasOptimizer
    from embeddingnet_amd.train_step import TripletTrainer
    base, _ = B.get_backbone(input_shape=(64, 64, 3), encodings_len=64, backbone_name="resnet18", embeddings_normalization=True,
                             backbone_weights=None, seed=5)
    base.to(dev)
    tr = TripletTrainer(base, KerasOptimizer(base.parameters(), "adam", 1e-3), k_classes=4, k_samples=2, margin=0.5, graph=False)
    imgs = torch.rand(8, 64, 64, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    loss = tr.step(imgs)
    torch.cuda.synchronize()
    state = [p.detach().clone() for p in base.parameters()] + [b.detach().clone() for b in base.buffers()]
    return loss.detach().reshape(-1)[:1].clone().view(torch.int32).item(), state


def same_state(a, b):
    return a[0] == b[0] and len(a[1]) == len(b[1]) and all(torch.equal(u, v) for u, v in zip(a[1], b[1]))


def test_resnet18_step_repeats_bit_for_bit():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    first, second = one_step(dev), one_step(dev)
    assert any(float(p.abs().max()) > 0 for p in first[1])
    assert same_state(first, second)
