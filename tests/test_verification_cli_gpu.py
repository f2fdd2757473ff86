"""GPU: tools/train.py with TRAIN.verification — the new values join the history and the log, and TRAIN.monitor: val_eer is
followed downwards (it is the first monitored evaluation value where lower is better)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_train_cli_logs_verification_and_monitors_val_eer(tmp_path):
    text = open(os.path.join(ROOT, "configs", "simple2_verification_synthetic.yml")).read()
    stock = open(os.path.join(ROOT, "configs", "simple2_synthetic.yml")).read()
    runs = [_start(tmp_path, name, t) for name, t in (("with", text), ("stock", stock))]   # side by side
    (out, hist), (out_stock, h_stock) = [_finish(r) for r in runs]
    keys = ("val_auc", "val_eer", "val_tar@far=0.1", "val_tar@far=0.01")
    for key in keys:
        assert hist[key].shape == (2,) and np.all((hist[key] >= 0) & (hist[key] <= 1)), key
        assert f" - {key} " in out
    assert set(hist.files) == {"loss", "val_loss"} | set(keys)
    assert np.all(hist["val_tar@far=0.01"] <= hist["val_tar@far=0.1"]) and np.all(hist["val_auc"] >= 0.5)
    improved = [l for l in out.splitlines() if "improved to" in l]
    assert improved and all(l.startswith("val_eer improved to ") for l in improved)
    assert float(improved[0].split("improved to ")[1].split(",")[0]) == pytest.approx(hist["val_eer"][0], abs=1e-5)
    assert len(improved) == 1 + int(hist["val_eer"][1] < hist["val_eer"][0])              # LOWER is better: no 1 - value flip
    # the stock config writes the history it always wrote, and the evaluation does not disturb training
    assert set(h_stock.files) == {"loss", "val_loss"} and "val_loss improved to" in out_stock
    assert np.array_equal(hist["loss"], h_stock["loss"]) and np.array_equal(hist["val_loss"], h_stock["val_loss"])
