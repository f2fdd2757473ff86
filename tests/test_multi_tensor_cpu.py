"""The host side of a multi-tensor launch (embeddingnet_amd/multi_tensor.py): the chunk list, the packed descriptor rows and the
{float; int32} word against what a caller of the C ABI writes by hand (include/embnet.h), without a GPU."""
import numpy as np
import pytest
import torch

from embeddingnet_amd import multi_tensor as MT

CE = 4096
SIZES = [1, 4095, 4096, 4097, 2 * 4096 + 13]


def test_chunk_list_is_the_hand_written_comprehension():
    got = MT.chunk_list(SIZES, CE)
    want = [(i, c) for i, n in enumerate(SIZES) for c in range(-(-n // CE))]
    assert got.dtype == np.int32 and got.shape == (len(want), 2) == (8, 2)
    assert got.tolist() == [list(r) for r in want]
    assert got[:, 0].tolist() == sorted(got[:, 0].tolist())                     # tensor-major
    assert got.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [4, 0], [4, 1], [4, 2]]


def test_pack_rows_keeps_a_pointer_with_the_top_bit_set():
    p = (1 << 63) | 0x7F12_3456_789A_BCD0
    got = MT.pack_rows([(p, 5), ((1 << 64) - 1, 0)])
    assert got.dtype == np.int64 and got.shape == (2, 2)
    assert got.view(np.uint64).tolist() == [[p, 5], [(1 << 64) - 1, 0]]
    assert got.tobytes()[:8] == p.to_bytes(8, "little")


def test_f32_i32_word_is_what_the_optimizer_packed():
    lam, group = 2e-4, 3
    assert MT.f32_i32_word(2.0 * lam, group) == int(np.float32(2.0 * lam).view(np.uint32)) | (group << 32)
    assert MT.f32_i32_word(lam) == int(np.float32(lam).view(np.uint32))
    word = np.asarray([MT.f32_i32_word(2.0 * lam, group)], dtype=np.uint64)
    assert word.view(np.float32)[0] == np.float32(2.0 * lam) and word.view(np.int32)[1] == group


def test_rows_have_the_strides_the_library_asserts():
    """sizeof(OptTensor) == 48 (csrc/optimizer.hip), sizeof(SumsqTensor) == 24 (csrc/nn_kernels.hip)."""
    opt = MT.pack_rows([(0x1000, 0x2000, 0x3000, 0, 4097, MT.f32_i32_word(4e-4, 1))] * 3)
    assert opt.strides == (48, 8) and opt.flags["C_CONTIGUOUS"]
    sumsq = MT.pack_rows([(0x1000, 7, MT.f32_i32_word(1e-4))] * 2)
    assert sumsq.strides == (24, 8) and sumsq.flags["C_CONTIGUOUS"]
    plan = MT.Plan([(0x1000, 7, MT.f32_i32_word(1e-4))] * 2, [7, 4097], CE, torch.device("cpu"))
    assert plan.table.stride() == (3, 1) and plan.table.dtype == torch.int64 and plan.chunks.dtype == torch.int32
    assert plan.args == (plan.table.data_ptr(), 2, plan.chunks.data_ptr(), 3)


def test_an_empty_launch_is_refused_in_python():
    with pytest.raises(ValueError, match="no elements"):
        MT.chunk_list([], CE)
    with pytest.raises(ValueError, match="no elements"):
        MT.Plan([], [], CE, torch.device("cpu"))
    with pytest.raises(ValueError, match="rows for"):
        MT.Plan([(1, 2, 3)], [7, 7], CE, torch.device("cpu"))
