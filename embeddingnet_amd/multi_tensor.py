"""The two arrays of a multi-tensor launch (csrc/multi_tensor.h): a device table of per-tensor descriptors and a device list
of int32 (tensor index, chunk index) pairs, one workgroup per pair.  The array builders are host-only NumPy; `Plan` puts a
pair of them on a device."""
import numpy as np
import torch


def chunk_list(sizes, chunk_elems):
    """int32 [n_chunks, 2]: (tensor index, chunk index) for every chunk of `chunk_elems` elements, tensor by tensor."""
    counts = [-(-int(n) // int(chunk_elems)) for n in sizes]
    if sum(counts) <= 0:
        raise ValueError("multi-tensor launch over no elements: the library refuses an empty chunk list")
    return np.asarray([(i, c) for i, k in enumerate(counts) for c in range(k)], dtype=np.int32)


def pack_rows(rows):
    """int64 [n, words] of descriptor rows given as 64-bit words; a word may be any int in [0, 2^64) — a device address with
    the top bit set keeps its bits."""
    return np.asarray(rows, dtype=np.uint64).view(np.int64).reshape(len(rows), -1)


def f32_i32_word(f, i=0):
    """The descriptor word { float f; int32 i; }."""
    return int(np.float32(f).view(np.uint32)) | ((int(i) & 0xFFFFFFFF) << 32)


class Plan:
    """Table and chunk list of one launch on `device`: rows[i] describes a tensor of sizes[i] elements."""

    def __init__(self, rows, sizes, chunk_elems, device):
        if len(rows) != len(sizes):
            raise ValueError(f"{len(rows)} descriptor rows for {len(sizes)} tensors")
        self.chunks = torch.from_numpy(chunk_list(sizes, chunk_elems)).to(device)
        self.table = torch.from_numpy(pack_rows(rows)).to(device)
        self.n = len(rows)

    @property
    def args(self):
        """(table, n_tensors, chunks, n_chunks) as the entry points take them."""
        return self.table.data_ptr(), self.n, self.chunks.data_ptr(), self.chunks.shape[0]
