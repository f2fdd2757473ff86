"""Verification metrics, host side (no GPU): the C ABI is declared and exported, arguments are refused before any launch, the
reduction from histograms to metrics (embeddingnet_amd/verification.py) agrees with the brute-force restatement
(tests/verification_ref.py) on hand cases and with scikit-learn where every distinct value has a bin of its own, the
conservative TAR@FAR rule and the EER interpolation give the answers worked by hand, the inputs of the GPU bracket test are fit
for it, and the Python surface (TRAIN.verification, TRAIN.monitor, calculate_verification_metrics) is there."""
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_verification_all_pairs_workspace_bytes", "embnet_verification_all_pairs", "embnet_verification_values")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import verification_ref as VR  # noqa: E402


def _l():
    from embeddingnet_amd import _lib
    return _lib.lib()


def _err():
    return _l().embnet_last_error().decode()


# ---- 1. header and exports ----------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_verification():
    from embeddingnet_amd import _lib, ops
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported and exported == set(protos)
    assert _l().embnet_abi_version() == 22
    header = open(os.path.join(ROOT, "include", "embnet.h")).read()
    assert "#define EMBNET_ABI_VERSION 22" in header
    assert "#define EMBNET_VERIFICATION_MAX_BINS 4096" in header and ops.VERIFICATION_MAX_BINS == 4096
    flat = " ".join(header.replace("*", " ").split())      # the comment's line breaks and margins do not matter
    for word in ("the product is exact", "EXACT function of the fp32 value", "bin(NaN) = bins - 1", "not a memset node",
                 "counted TWICE", "bitwise reproducible"):
        assert word in flat, word


def test_python_surface_is_there():
    import embedding_net
    import embedding_net.verification as alias
    from embeddingnet_amd import models, ops, verification
    assert alias is verification and embedding_net.verification is verification
    for name in ("verification_from_histograms", "verification_metrics", "verification_pair_metrics", "verification_score_metrics"):
        assert callable(getattr(verification, name)), name
    assert callable(ops.verification_all_pairs) and callable(ops.verification_values)
    sig = inspect.signature(models.EmbeddingNet.calculate_verification_metrics)
    assert list(sig.parameters) == ["self", "data_loader", "fars", "bins", "gallery", "batch_size"]
    assert sig.parameters["bins"].default == 4096 and sig.parameters["gallery"].default == "val"
    assert sig.parameters["batch_size"].default == 256 and tuple(sig.parameters["fars"].default) == (1e-1, 1e-2, 1e-3)


# ---- 2. argument refusal --------------------------------------------------------------------------------------------------
def _ap(nq=100, n=100, e=8, bins=64, d2_max=4.0, flush_tiles=0, ws_bytes=None, **ptrs):
    l = _l()
    a = dict(q=FAKE, ql=FAKE, x=FAKE, xl=FAKE, hs=FAKE, ho=FAKE, ws=FAKE)
    a.update(ptrs)
    ws_bytes = l.embnet_verification_all_pairs_workspace_bytes(nq, n) if ws_bytes is None else ws_bytes
    return l.embnet_verification_all_pairs(a["q"], a["ql"], nq, a["x"], a["xl"], n, e, bins, d2_max, flush_tiles, a["hs"], a["ho"],
                                           a["ws"], ws_bytes, None)


def _vv(m=10, lo=0.0, w=0.25, bins=64, **ptrs):
    a = dict(v=FAKE, same=FAKE, hs=FAKE, ho=FAKE)
    a.update(ptrs)
    return _l().embnet_verification_values(a["v"], a["same"], m, lo, w, bins, a["hs"], a["ho"], None)


def test_all_pairs_refusals():
    for name in ("q", "ql", "hs", "ho", "ws"):
        assert _ap(**{name: None}) == -1 and "null pointer" in _err(), name
    assert _ap(x=None) == -1 and "come together" in _err()
    assert _ap(xl=None) == -1 and "come together" in _err()
    assert _ap(x=None, xl=None, nq=100, n=101, ws_bytes=1 << 20) == -1 and "leave-one-out" in _err()
    for kw in (dict(nq=0), dict(nq=-3), dict(n=0), dict(e=0), dict(e=-8)):
        assert _ap(ws_bytes=1 << 30, **kw) == -1 and "must be positive" in _err(), kw
    for bins in (0, 1, 3, 48, 100, 4095, 8192, -64):
        assert _ap(bins=bins) == -1 and "bins=" in _err() and "power of two" in _err(), bins
    for d2_max in (0.0, -4.0, 3.0, 4.5, float("inf"), float("nan"), 1e-45):
        assert _ap(d2_max=d2_max) == -1 and "d2_max" in _err(), d2_max
    need = _l().embnet_verification_all_pairs_workspace_bytes(100, 100)
    assert _ap(ws_bytes=need - 8) == -3 and "workspace" in _err()
    assert _ap(ws=FAKE + 4) == -1 and "aligned" in _err()
    assert _ap(hs=FAKE + 4) == -1 and "aligned" in _err()
    assert _ap(nq=1 << 20, n=16, e=1024) == -1 and "2 GiB" in _err()
    assert _ap(nq=16, n=1 << 20, e=1024) == -1 and "2 GiB" in _err()
    # the largest safe interval: (2^32 - 1) / (64 * 64) on the 64x64 tile, (2^32 - 1) / (128 * 128) on the 128x128 one
    assert _ap(flush_tiles=-1) == -1 and "flush_tiles" in _err()
    assert _ap(nq=100, n=100, flush_tiles=(2 ** 32 - 1) // 4096 + 1) == -1 and "overflow" in _err()
    big = dict(nq=2560, n=2560, e=16)
    assert _ap(flush_tiles=(2 ** 32 - 1) // 16384 + 1, **big) == -1 and "overflow" in _err() and "128x128" in _err()


def test_values_refusals():
    for name in ("v", "same", "hs", "ho"):
        assert _vv(**{name: None}) == -1 and "null pointer" in _err(), name
    assert _vv(m=-1) == -1 and "negative" in _err()
    for bins in (0, 1, 3, 100, 8192):
        assert _vv(bins=bins) == -1 and "power of two" in _err(), bins
    for w in (0.0, -0.25, 0.3, float("inf"), float("nan")):
        assert _vv(w=w) == -1 and "w=" in _err(), w
    assert _vv(lo=float("nan")) == -1 and "lo" in _err()
    assert _vv(hs=FAKE + 4) == -1 and "aligned" in _err()


def test_workspace_bytes():
    f = _l().embnet_verification_all_pairs_workspace_bytes
    for args in ((0, 10), (10, 0), (-1, 10), (10, -4)):
        assert f(*args) == 0, args
    assert all(f(a, b) % 16 == 0 for a, b in ((1, 1), (63, 517), (50000, 50000)))
    assert 4 * 100000 <= f(50000, 50000) <= 4 * 100000 + 64          # O(nq + n): the two norm vectors


# ---- 3. the host reduction against the restatement ---------------------------------------------------------------------------
FARS = (0.25, 0.1, 0.01)


def _hist(values, lo, w, bins):
    return np.bincount(VR.bin_of(values, lo, w, bins), minlength=bins)


def _both(same, other, lo=0.0, w=0.25, bins=16, accept="below", at=(), fars=FARS):
    from embeddingnet_amd.verification import verification_from_histograms
    got = verification_from_histograms(_hist(same, lo, w, bins), _hist(other, lo, w, bins), lo, w, fars=fars, at=at, accept=accept)
    want = VR.brute_metrics(same, other, lo, w, bins, fars=fars, at=at, accept=accept)
    VR.same_metrics(got, want)
    assert len(got["tpr"]) == len(got["fpr"]) == len(got["thresholds"]) == bins + 1
    return got


def test_perfectly_separated_sets():
    got = _both([0.1, 0.3, 0.6, 0.6], [2.1, 2.6, 3.9, 3.2, 2.1])
    assert got["auc"] == 1.0 and got["eer"] == 0.0 and got["best_accuracy"] == 1.0
    assert got["best_threshold"] == 0.75                    # the first edge with every same pair below it
    assert all(got[f"tar@far={f!r}"] == 1.0 for f in FARS) and got["threshold@far=0.01"] == 2.0   # the last edge with FP = 0


def test_fully_overlapping_sets():
    v = [0.1, 0.6, 0.6, 1.3, 2.2, 3.9]
    got = _both(v, v)
    assert got["auc"] == 0.5 and got["eer"] == pytest.approx(0.5, abs=1e-15)
    assert got["best_accuracy"] == 0.5 and got["best_threshold"] == 0.0      # ties go to the smaller j


def test_all_pairs_in_one_bin():
    got = _both([1.1, 1.2, 1.15], [1.05, 1.24], at=(1.0, 1.3, 1.12, 1.13))
    assert got["auc"] == 0.5 and got["eer"] == pytest.approx(0.5, abs=1e-15) and got["eer_threshold"] == pytest.approx(1.125)
    assert got["tar@far=0.25"] == 0.0 and got["threshold@far=0.25"] == 1.0
    assert got["accuracy@1.0"] == 0.4 and got["accuracy@1.3"] == 0.6
    assert got["accuracy_threshold@1.12"] == 1.0 and got["accuracy_threshold@1.13"] == 1.25      # snapped to the nearest edge


def test_single_same_pair():
    got = _both([0.7], [0.1, 0.9, 1.7, 2.6])
    assert got["n_same"] == 1 and got["n_other"] == 4 and got["auc"] == 0.75
    assert got["tar@far=0.25"] == 1.0 and got["threshold@far=0.25"] == 0.75    # one false accept allowed: up to the edge before 0.9
    assert _both([0.8], [0.1, 0.9, 1.7, 2.6])["auc"] == 0.625                  # 0.8 and 0.9 share a bin: that pair counts half


def test_no_same_pair_and_no_other_pair():
    from embeddingnet_amd.verification import verification_from_histograms
    for P, N in (([0, 0, 0, 0], [1, 2, 0, 3]), ([1, 2, 0, 3], [0, 0, 0, 0])):
        got = verification_from_histograms(P, N, 0.0, 0.5, fars=FARS, at=[1.0])
        assert got["n_same"] == sum(P) and got["n_other"] == sum(N)
        for key in ("auc", "eer", "eer_threshold", "best_accuracy", "best_threshold", "tar@far=0.1", "threshold@far=0.1",
                    "accuracy@1.0"):
            assert math.isnan(got[key]), key
        assert np.all(np.isnan(got["tpr" if sum(P) == 0 else "fpr"])) and got["accuracy_threshold@1.0"] == 1.0
        assert np.array_equal(got["thresholds"], [0.0, 0.5, 1.0, 1.5, 2.0])


def test_accept_above_for_scores():
    same = [(k + 0.5) / 16 for k in (14, 12, 15, 6)]        # bin centres: 1 - score is the centre of the mirrored bin
    other = [(k + 0.5) / 16 for k in (1, 3, 13, 4, 0)]
    got = _both(same, other, lo=0.0, w=1 / 16, bins=16, accept="above", at=(0.5,))
    flipped = _both([1 - v for v in same], [1 - v for v in other], lo=0.0, w=1 / 16, bins=16, at=(0.5,))
    assert got["auc"] == flipped["auc"] == 0.9 and got["eer"] == flipped["eer"]      # 18 of the 20 (same, other) pairs in order
    assert got["best_threshold"] == 1.0 - flipped["best_threshold"] and got["best_accuracy"] == flipped["best_accuracy"]
    assert np.array_equal(got["thresholds"], np.arange(16, -1, -1) / 16)
    assert got["accuracy@0.5"] == 7 / 9                      # accepted: scores >= 0.5 -> 3 of 4 same right, 4 of 5 other right


def test_random_cases_agree_with_the_restatement():
    rs = np.random.RandomState(5)
    for bins, w in ((2, 2.0), (8, 0.5), (64, 1 / 16), (256, 1 / 64)):
        same = rs.gamma(2.0, 0.4, size=57)
        other = rs.gamma(5.0, 0.5, size=143)
        _both(same, other, w=w, bins=bins, at=(0.25, 1.0, 7.5), fars=(0.5, 0.1, 0.07, 0.001))
        _both(np.clip(1 - same / 4, 0, 0.999), np.clip(1 - other / 4, 0, 0.999), w=1.0 / bins, bins=bins, accept="above", at=(0.5,))


def test_against_sklearn_where_every_value_has_its_own_bin():
    from sklearn.metrics import roc_auc_score, roc_curve
    from embeddingnet_amd.verification import verification_from_histograms
    rs = np.random.RandomState(11)
    bins, w = 256, 1 / 64
    for trial in range(3):
        ks = rs.randint(0, bins, size=400)                  # repeated values (ties) included; the value of bin k is its centre
        y = rs.rand(400) < (0.75 - 0.5 * ks / bins)         # same pairs lean to small distances
        d = (ks + 0.5) * w
        got = verification_from_histograms(np.bincount(ks[y], minlength=bins), np.bincount(ks[~y], minlength=bins), 0.0, w)
        assert abs(got["auc"] - roc_auc_score(y, -d)) <= 1e-12
        fpr, tpr, _ = roc_curve(y, -d, drop_intermediate=False)
        ours = np.unique(np.round(np.stack([got["fpr"], got["tpr"]], 1), 12), axis=0)
        theirs = np.unique(np.round(np.stack([fpr, tpr], 1), 12), axis=0)
        assert ours.shape == theirs.shape and np.allclose(ours, theirs, atol=1e-12, rtol=0)


def test_tar_at_far_is_conservative():
    from embeddingnet_amd.verification import far_count, verification_from_histograms
    # f * n_other just below an integer: 0.1 * 19 = 1.9 allows one false accept; at an integer: 0.1 * 20 = 2.0 allows two.
    # (0.1 is read as one tenth: 0.1 * 30 is 3, although the double 0.1 times 30 rounds to 3.0000000000000004 and
    # 0.07 * 100 to 7.000000000000001; 0.29 * 100 rounds to 28.999999999999996 and is still 29.)
    assert far_count(0.1, 19) == 1 and far_count(0.1, 20) == 2 and far_count(0.1, 30) == 3
    assert far_count(0.07, 100) == 7 and far_count(0.29, 100) == 29 and far_count(1e-3, 999) == 0 and far_count(1e-3, 1000) == 1
    P = [5, 5, 5, 5]
    for n_last, tar, thr in ((16, 0.5, 1.0), (17, 0.75, 1.5)):          # N = [1, 1, 1, n_last]: FP_j = 0, 1, 2, 3, 3 + n_last
        got = verification_from_histograms(P, [1, 1, 1, n_last], 0.0, 0.5, fars=(0.1,))
        # n_other = 19: floor(1.9) = 1 -> the largest j with FP_j <= 1 is 1?  FP = [0, 1, 2, 3, 19]: j = 1; n_other = 20: FP_j <= 2: j = 2
        assert got["n_other"] == 3 + n_last
        assert (got["tar@far=0.1"], got["threshold@far=0.1"]) == ((0.25, 0.5) if n_last == 16 else (0.5, 1.0))
    # never interpolated, never above the bound: the reported point has FPR <= f
    got = verification_from_histograms([3, 0, 1], [0, 7, 3], 0.0, 1.0, fars=(0.5, 0.69, 0.7))
    assert got["tar@far=0.5"] == 0.75 and got["threshold@far=0.5"] == 1.0
    assert got["tar@far=0.69"] == 0.75 and got["tar@far=0.7"] == 0.75 and got["threshold@far=0.7"] == 2.0


def test_eer_interpolation_by_hand():
    from embeddingnet_amd.verification import verification_from_histograms
    # two bins, P = [3, 1], N = [1, 3]: edges j = 0, 1, 2 have (FPR, 1 - TPR) = (0, 1), (1/4, 1/4), (1, 0): they meet AT edge 1
    got = verification_from_histograms([3, 1], [1, 3], 0.0, 2.0, fars=(0.5,))
    assert got["eer"] == 0.25 and got["eer_threshold"] == 2.0
    # P = [4, 0], N = [1, 3]: (0, 1), (1/4, 0), (1, 0): the crossing lies between edges 0 and 1, s = (1 - 0) / (1/4 + 1) = 4/5,
    # eer = 0 + 4/5 * 1/4 = 1/5 at threshold 0 + 4/5 * 2
    got = verification_from_histograms([4, 0], [1, 3], 0.0, 2.0, fars=(0.5,))
    assert got["eer"] == pytest.approx(0.2, abs=1e-15) and got["eer_threshold"] == pytest.approx(1.6, abs=1e-15)
    # P = [1, 3], N = [0, 4]: (0, 1), (0, 3/4), (1, 0): between edges 1 and 2, s = (3/4 - 0) / (1 + 3/4) = 3/7, eer = 3/7
    got = verification_from_histograms([1, 3], [0, 4], 0.0, 2.0, fars=(0.5,))
    assert got["eer"] == pytest.approx(3 / 7, abs=1e-15) and got["eer_threshold"] == pytest.approx(2.0 + 6 / 7, abs=1e-15)


def test_bad_arguments_are_value_errors():
    from embeddingnet_amd import verification as V
    with pytest.raises(ValueError, match="accept"):
        V.verification_from_histograms([1], [1], 0.0, 1.0, accept="between")
    with pytest.raises(ValueError, match="one length"):
        V.verification_from_histograms([1, 2], [1], 0.0, 1.0)
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        V.verification_from_histograms([1, 2], [1, 2], 0.0, 1.0, fars=(1.0,))
    with pytest.raises(ValueError, match="negative"):
        V.verification_from_histograms([1, -2], [1, 2], 0.0, 1.0)
    for bins in (0, 3, 8192, 2.5):
        with pytest.raises(ValueError, match="power of two"):
            V.verification_metrics(np.zeros((4, 2), np.float32), [0, 0, 1, 1], bins=bins)


# ---- 4. the inputs of the GPU bracket test -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,e", [(300, 64), (517, 96), (1000, 128)])
def test_open_share_of_the_continuous_gpu_inputs(n, e):
    """The brackets of the GPU test leave a pair undecided only when an edge lies within B of its float64 d2.  For them to
    bind, that share has to be small: at most 0.5 % for every (input, bins) the GPU file uses.  At 4096 bins the same inputs
    are past it (an edge every 2^-10, B = 4e-6 on both sides: 0.8 %), which is why the 4096-bin GPU cases use grid inputs."""
    x, labels = VR.clustered_unit_rows(n, e)
    assert np.allclose(np.linalg.norm(x.astype(np.float64), axis=1), 1.0, atol=1e-6)
    for bins in (64, 1024):
        br = VR.brackets(x, labels, None, None, bins, 4.0, VR.A(e))
        assert br["open_share"] <= 0.005, (bins, br["open_share"])
        assert br["n_same"] + br["n_other"] == n * (n - 1) and br["n_same"] > 0
        hs, ho = VR.exact_histograms(x, labels, None, None, bins, 4.0)
        for name, h in (("same", hs), ("other", ho)):
            lo, hi = br[name]
            cum = np.concatenate([[0], np.cumsum(h)])
            assert np.all(lo <= cum) and np.all(cum <= hi), name
    assert VR.brackets(x, labels, None, None, 4096, 4.0, VR.A(e))["open_share"] > 0.005


# ---- 5. tools/train.py: TRAIN.verification and TRAIN.monitor -------------------------------------------------------------------------
def test_verification_config():
    import train as T
    assert T.verification_config({}, True) is None and T.verification_config({"verification": False}, False) is None
    assert T.verification_config({"verification": True}, True) == {"fars": [0.1, 0.01, 0.001], "bins": 4096}
    assert T.verification_config({"verification": {"fars": [0.05], "bins": 256}}, True) == {"fars": [0.05], "bins": 256}
    assert T.verification_config({"verification": {"bins": 2}}, True)["bins"] == 2
    with pytest.raises(ValueError, match="DATALOADER.validate"):
        T.verification_config({"verification": True}, False)
    for bins in (0, 1, 3, 1000, 8192, 64.0, "64", True):
        with pytest.raises(ValueError, match="power of two"):
            T.verification_config({"verification": {"bins": bins}}, True)
    for fars in ([0.0], [1.0], [-0.1], [0.1, 2], ["0.1"], [], [True]):
        with pytest.raises(ValueError, match="far"):
            T.verification_config({"verification": {"fars": fars}}, True)
    with pytest.raises(ValueError, match="unknown keys"):
        T.verification_config({"verification": {"far": [0.1]}}, True)
    with pytest.raises(ValueError, match="mapping"):
        T.verification_config({"verification": "yes"}, True)


def test_monitor_rules():
    import train as T
    on = {"verification": {"fars": [0.1, 0.01], "bins": 64}}
    for name in ("val_auc", "val_eer", "val_tar@far=0.1", "val_tar@far=0.01"):
        assert T.monitor_config(dict(on, monitor=name), True) == ([], name)
        with pytest.raises(ValueError, match="needs TRAIN.verification"):
            T.monitor_config({"monitor": name}, True)
        with pytest.raises(ValueError, match="DATALOADER.validate"):
            T.monitor_config(dict(on, monitor=name), False)
    with pytest.raises(ValueError, match="names a far"):
        T.monitor_config(dict(on, monitor="val_tar@far=0.001"), True)
    with pytest.raises(ValueError, match="val_auc, val_eer, val_tar@far=f"):
        T.monitor_config(dict(on, monitor="val_roc"), True)
    assert T.monitor_config({}, True) == ([], "val_loss") and T.monitor_config({}, False) == ([], "loss")
    assert T.verification_names({"fars": [0.1, 0.001], "bins": 64}) == ["auc", "eer", "tar@far=0.1", "tar@far=0.001"]
    assert T.verification_names(None) == []


def test_monitored_value_does_not_flip_val_eer():
    import train as T
    history = {"loss": [0.9], "val_loss": [0.7], "val_eer": [0.2], "val_auc": [0.9], "val_tar@far=0.1": [0.6], "val_mrr": [0.75]}
    assert T.monitored_value("loss", history, 0.9) == 0.9 and T.monitored_value("val_loss", history, 0.9) == 0.7
    assert T.monitored_value("val_eer", history, 0.9) == 0.2            # lower is better: taken as it is
    assert T.monitored_value("val_auc", history, 0.9) == pytest.approx(0.1)
    assert T.monitored_value("val_tar@far=0.1", history, 0.9) == pytest.approx(0.4)
    assert T.monitored_value("val_mrr", history, 0.9) == 0.25


def test_config_file():
    import yaml
    import train as T
    from embeddingnet_amd.utils import parse_params
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "simple2_verification_synthetic.yml")))
    stock = yaml.safe_load(open(os.path.join(ROOT, "configs", "simple2_synthetic.yml")))
    assert cfg["TRAIN"]["verification"] == {"fars": [0.1, 0.01], "bins": 4096} and cfg["TRAIN"]["monitor"] == "val_eer"
    assert cfg["GENERAL"]["project_name"] == "simple2_verification_synthetic"
    for section in ("MODEL", "DATALOADER", "GENERATOR"):
        assert cfg[section] == stock[section], section
    params = parse_params(os.path.join(ROOT, "configs", "simple2_verification_synthetic.yml"))
    assert T.verification_config(params["train"], True) == {"fars": [0.1, 0.01], "bins": 4096}
    assert T.monitor_config(params["train"], True) == ([], "val_eer")
