"""Cross-Batch Memory (Wang et al., CVPR 2020, "XBM"): the detached embeddings of the last `size` samples and their labels in a
ring that lives on the device.  Build-defined: the reference has no memory.

Embeddings drift slowly, so a batch can be scored against the embeddings of the last few thousand samples as if they were current:
ops.xbm_contrastive_loss / ops.xbm_multi_similarity_loss take the ring as their bank, train_step.XbmTrainer adds that loss to the
in-batch one.  The write position is a device int32 that the enqueue kernel reads and advances itself (include/embnet.h,
embnet_xbm_enqueue): nothing here waits for the GPU, and a training step captured into a HIP graph replays on the ring's current
state.  The ring is a constant of the loss: it receives no gradient.  It is not part of a checkpoint: after --resume_from it
refills from the first steps.  Under data parallelism every rank keeps a ring of its own batches; nothing is gathered.
"""
import torch

from . import ops


class CrossBatchMemory:
    """feats [size, embedding_size] fp32 (zeros), labels [size] int32 (-1: an empty slot, which belongs to no pair), cursor [1]
    int32 (the next slot to write), slots [size] int32 (its first N entries: where the last enqueue put its N rows)."""

    def __init__(self, size, embedding_size, device):
        self.size, self.embedding_size = int(size), int(embedding_size)
        if self.size < 1 or self.embedding_size < 1:
            raise ValueError(f"CrossBatchMemory: size={size} and embedding_size={embedding_size} must be positive")
        device = torch.device(device)
        self.feats = torch.zeros((self.size, self.embedding_size), dtype=torch.float32, device=device)
        self.labels = torch.full((self.size,), -1, dtype=torch.int32, device=device)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=device)
        self.slots = torch.zeros(self.size, dtype=torch.int32, device=device)
        self.ticket = torch.zeros(4, dtype=torch.int32, device=device)      # the enqueue kernel's arrival counter (re-armed by it)

    def enqueue(self, emb, labels):
        """The rows of emb [N, E], detached, and their int32 labels [N] into the next N slots (wrapping).  -> slots int32 [N], a view
        of self.slots: the rows' own copies, for the losses' self_slots.  No host synchronisation."""
        return ops.xbm_enqueue(emb, labels, self)

    def reset(self):
        """An empty ring again (in place: a captured step keeps pointing at the same tensors)."""
        self.feats.zero_()
        self.labels.fill_(-1)
        self.cursor.zero_()

    def filled(self):
        """The number of labelled slots.  Waits for the device: the only method that does."""
        return int((self.labels >= 0).sum().item())
