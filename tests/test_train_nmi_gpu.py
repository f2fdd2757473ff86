"""TRAIN.clustering_nmi end to end: EmbeddingNet.calculate_clustering_metrics, and tools/train.py logging val_nmi per epoch and
following it with plateau / early stop / best checkpoint.  The configuration half (no GPU) refuses what cannot be honoured."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_monitor_config_refuses_val_nmi_without_its_key_or_without_validation():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train as T
    assert T.monitor_config({"clustering_nmi": True, "monitor": "val_nmi"}, True) == ([], "val_nmi")
    with pytest.raises(ValueError, match="'val_nmi' needs TRAIN.clustering_nmi"):
        T.monitor_config({"monitor": "val_nmi"}, True)
    with pytest.raises(ValueError, match="'val_nmi' needs TRAIN.clustering_nmi"):
        T.monitor_config({"monitor": "val_nmi", "clustering_nmi": False}, True)
    with pytest.raises(ValueError, match="validation is off"):
        T.monitor_config({"monitor": "val_nmi", "clustering_nmi": True}, False)
    assert T.monitor_config({}, True) == ([], "val_loss")      # without the key nothing changes


@pytest.mark.gpu
def test_model_level_clustering_metrics(tmp_path):
    from embeddingnet_amd.clustering import clustering_metrics
    from embeddingnet_amd.datagenerators import SyntheticDataLoader
    from embeddingnet_amd.models import TripletNet
    dev = torch.device("cuda:0")
    params = {"model": dict(input_shape=[64, 64, 3], encodings_len=64, mode="triplet", distance_type="l2",
                            backbone_name="simple2", backbone_weights=None, freeze_backbone=False,
                            embeddings_normalization=True, device=dev, seed=0),
              "dataloader": {}, "generator": {}, "train": {}, "general": {"work_dir": str(tmp_path), "project_name": "p"}}
    data = SyntheticDataLoader(6, 16, (64, 64, 3), noise=0.2, validate=True, val_ratio=0.25, seed=3)
    net = TripletNet(params, training=True)
    got = net.calculate_clustering_metrics(data)
    enc = np.concatenate([net.base_model.predict(data.val_data[c]) for c in data.val_data])
    labels = [c for c in data.val_data for _ in range(len(data.val_data[c]))]
    want = clustering_metrics(enc, labels, device=dev)
    assert set(got) == {"nmi", "homogeneity", "completeness", "purity", "inertia", "n_iter", "n_empty", "n_clusters"}
    assert got == want and got["n_clusters"] == 6 and 0.0 <= got["nmi"] <= 1.0
    assert net.calculate_clustering_metrics(data, batch_size=32) == got
    assert net.calculate_clustering_metrics(data, n_clusters=3, seed=4, n_init=2)["n_clusters"] == 3


def _start(tmp_path, name, text):
    """tools/train.py on `text` in a fresh child process under its own time limit: 2 epochs, 10 synthetic classes."""
    wd = tmp_path / name
    cfg_path = tmp_path / f"{name}.yml"
    cfg_path.write_text(text.replace("work_dirs/", str(wd) + "/"))
    project = [l.split("'")[1] for l in text.splitlines() if "project_name" in l][0]
    proc = subprocess.Popen(["timeout", "-k", "10", "500", sys.executable, os.path.join(ROOT, "tools", "train.py"), str(cfg_path),
                             "--synthetic", "10", "--max_epochs", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return proc, wd / project / "plots" / "history.npz"


def _finish(started):
    proc, hist = started
    out, err = proc.communicate(timeout=600)
    assert proc.returncode == 0, out[-2000:] + err[-2000:]
    return out, np.load(hist)


@pytest.mark.gpu
def test_train_cli_logs_and_monitors_val_nmi(tmp_path):
    text = open(os.path.join(ROOT, "configs", "simple2_nmi_synthetic.yml")).read()
    stock = open(os.path.join(ROOT, "configs", "simple2_synthetic.yml")).read()
    runs = [_start(tmp_path, name, t) for name, t in (("with", text), ("stock", stock))]   # side by side
    (out, hist), (out_stock, h_stock) = [_finish(r) for r in runs]
    assert hist["val_nmi"].shape == (2,) and np.all((hist["val_nmi"] >= 0) & (hist["val_nmi"] <= 1))
    assert " - val_nmi " in out and set(hist.files) == {"loss", "val_loss", "val_nmi"}
    improved = [l for l in out.splitlines() if "improved to" in l]
    assert improved and all(l.startswith("val_nmi improved to ") for l in improved)
    assert float(improved[0].split("improved to ")[1].split(",")[0]) == pytest.approx(hist["val_nmi"][0], abs=1e-5)
    assert len(improved) == 1 + int(1.0 - hist["val_nmi"][1] < 1.0 - hist["val_nmi"][0])   # larger is better
    # the stock config writes the history it always wrote, and the evaluation does not disturb training
    assert set(h_stock.files) == {"loss", "val_loss"} and "val_loss improved to" in out_stock
    assert np.array_equal(hist["loss"], h_stock["loss"]) and np.array_equal(hist["val_loss"], h_stock["val_loss"])
