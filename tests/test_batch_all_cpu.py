"""Batch-all triplet loss, host side (no GPU): the C ABI is declared and exported, arguments outside the supported range are
refused before any launch, and TripletsDataGenerator accepts the two fused-step-only rules."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_batch_all_path", "embnet_batch_all_workspace_bytes", "embnet_batch_all_loss_fwd", "embnet_batch_all_loss_bwd")


def test_header_declares_and_library_exports_batch_all():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported
    assert exported == set(protos)
    assert _lib.lib().embnet_abi_version() == 22


FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced


def _fwd(p, k, e, ws_bytes=None, null=None, path=0):
    l = __import__("embeddingnet_amd._lib", fromlist=["lib"]).lib()
    args = dict(emb=FAKE, w=FAKE, n=FAKE, frac=FAKE, mean=FAKE, ws=FAKE)
    if null:
        args[null] = None
    if ws_bytes is None:
        ws_bytes = l.embnet_batch_all_workspace_bytes(p, k, e)
    rc = l.embnet_batch_all_loss_fwd(args["emb"], p, k, e, 0.5, path, args["w"], args["n"], args["frac"], args["mean"],
                                     args["ws"], ws_bytes, None)
    return rc, l.embnet_last_error().decode()


@pytest.mark.parametrize("null", ["emb", "w", "n", "frac", "mean", "ws"])
def test_fwd_rejects_null_pointers(null):
    rc, msg = _fwd(8, 4, 256, null=null)
    assert rc == -1 and "null pointer" in msg


@pytest.mark.parametrize("p,k,e,what", [(1, 4, 64, "p >= 2"), (4, 1, 64, "k >= 2"), (2, 2049, 16, "n = p*k = 4098"),
                                        (1025, 4, 16, "n = p*k = 4100"), (8, 4, 4097, "e=4097"), (8, 4, 0, "e=0"),
                                        (2, 2048, 16, "2^31-1 triplets")])
def test_fwd_rejects_out_of_range_shapes(p, k, e, what):
    rc, msg = _fwd(p, k, e, ws_bytes=1 << 30)
    assert rc == -1 and what in msg, msg


def test_fwd_rejects_short_workspace_and_bad_path():
    from embeddingnet_amd import _lib
    need = _lib.lib().embnet_batch_all_workspace_bytes(8, 4, 256)
    assert need > 0
    rc, msg = _fwd(8, 4, 256, ws_bytes=need - 16)
    assert rc == -3 and "workspace" in msg
    rc, msg = _fwd(8, 4, 256, path=3)
    assert rc == -1 and "unknown path" in msg
    rc, msg = _fwd(4, 32, 64, path=1)                       # k > 16: only the distance-matrix path
    assert rc == -1 and "per-class path" in msg


def test_bwd_rejects_bad_arguments():
    from embeddingnet_amd import _lib
    l = _lib.lib()
    assert l.embnet_batch_all_loss_bwd(None, 32, 256, FAKE, FAKE, None, FAKE, None) == -1
    assert "null pointer" in l.embnet_last_error().decode()
    assert l.embnet_batch_all_loss_bwd(FAKE, 4097, 256, FAKE, FAKE, None, FAKE, None) == -1
    assert l.embnet_batch_all_loss_bwd(FAKE, 32, 4097, FAKE, FAKE, None, FAKE, None) == -1


def test_paths_and_workspace_sizes():
    from embeddingnet_amd import _lib
    l = _lib.lib()
    for p, k, e in [(8, 4, 256), (32, 4, 256), (64, 4, 512), (3, 3, 64), (20, 3, 128), (16, 16, 128), (5, 7, 33)]:
        assert l.embnet_batch_all_path(p, k, e) == 1, (p, k, e)
    for p, k, e in [(4, 4, 4096), (256, 8, 128), (4, 32, 64), (64, 64, 64)]:
        assert l.embnet_batch_all_path(p, k, e) == 2, (p, k, e)
        n = p * k
        assert l.embnet_batch_all_workspace_bytes(p, k, e) >= n * n * 4
    assert l.embnet_batch_all_path(1, 4, 64) == 0 and l.embnet_batch_all_workspace_bytes(1, 4, 64) == 0


def test_triplets_generator_accepts_the_step_only_modes():
    from embeddingnet_amd.datagenerators import SyntheticDataLoader, TripletsDataGenerator
    data = SyntheticDataLoader(6, 4, (8, 8, 3), validate=False)
    for mode in ("batch_all", "batch_hard"):
        gen = TripletsDataGenerator(embedding_model=None, class_files_paths=data.train_data, class_names=data.class_names,
                                    n_batches=2, input_shape=[8, 8, 3], k_classes=3, k_samples=2,
                                    negatives_selection_mode=mode)
        assert gen.sample_batch().shape == (6, 8, 8, 3)
        with pytest.raises(ValueError, match="TripletTrainer"):
            gen.mine_batch(gen.sample_batch())
    with pytest.raises(KeyError):
        TripletsDataGenerator(embedding_model=None, class_files_paths=data.train_data, class_names=data.class_names,
                              input_shape=[8, 8, 3], negatives_selection_mode="nope")
