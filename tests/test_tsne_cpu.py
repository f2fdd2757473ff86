"""Exact t-SNE, host side (no GPU): the C ABI is declared and exported, arguments are refused before any launch, the NumPy
restatement (tests/tsne_ref.py) agrees with the recorded scikit-learn results (tests/golden/tsne.npz), and the Python surface
(`embeddingnet_amd.tsne.TSNE`, `embedding_net.utils.plot_tsne` ...) is there with the reference's parameter names."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tsne.npz")
NEW = ("embnet_tsne_workspace_bytes", "embnet_tsne_affinities", "embnet_tsne_iterate", "embnet_tsne_kl")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_ref as R  # noqa: E402


def _l():
    from embeddingnet_amd import _lib
    return _lib.lib()


def _err():
    return _l().embnet_last_error().decode()


def test_header_declares_and_library_exports_tsne():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported
    assert exported == set(protos)
    assert _l().embnet_abi_version() == 22


def test_workspace_bytes_range():
    l = _l()
    assert l.embnet_tsne_workspace_bytes(1) == 0 and l.embnet_tsne_workspace_bytes(32769) == 0
    assert l.embnet_tsne_workspace_bytes(2) > 0
    assert l.embnet_tsne_workspace_bytes(32768) >= 32768 * 48


def _aff(n=100, perp=30.0, ws_bytes=None, **null):
    l = _l()
    a = dict(d2=FAKE, p=FAKE, beta=FAKE, ws=FAKE)
    a.update(null)
    ws_bytes = l.embnet_tsne_workspace_bytes(n) if ws_bytes is None else ws_bytes
    return l.embnet_tsne_affinities(a["d2"], n, perp, a["p"], a["beta"], a["ws"], ws_bytes, None)


def _it(n=100, n_iter=1, ws_bytes=None, **null):
    l = _l()
    a = dict(p=FAKE, y=FAKE, u=FAKE, g=FAKE, ws=FAKE)
    a.update(null)
    ws_bytes = l.embnet_tsne_workspace_bytes(n) if ws_bytes is None else ws_bytes
    return l.embnet_tsne_iterate(a["p"], n, a["y"], a["u"], a["g"], 1.0, 0.8, 50.0, n_iter, a["ws"], ws_bytes, None)


def _kl(n=100, ws_bytes=None, **null):
    l = _l()
    a = dict(p=FAKE, y=FAKE, kl=FAKE, gn=FAKE, ws=FAKE)
    a.update(null)
    ws_bytes = l.embnet_tsne_workspace_bytes(n) if ws_bytes is None else ws_bytes
    return l.embnet_tsne_kl(a["p"], n, a["y"], a["kl"], a["gn"], None, a["ws"], ws_bytes, None)


@pytest.mark.parametrize("fn,names", [(_aff, ("d2", "p", "beta", "ws")), (_it, ("p", "y", "u", "g", "ws")),
                                      (_kl, ("p", "y", "kl", "gn", "ws"))])
def test_rejects_null_pointers(fn, names):
    for name in names:
        assert fn(**{name: None}) == -1 and "null pointer" in _err(), (fn.__name__, name)


@pytest.mark.parametrize("fn", [_aff, _it, _kl])
def test_rejects_n_out_of_range_short_and_misaligned_workspace(fn):
    for n in (1, 0, -5, 32769):
        assert fn(n=n, ws_bytes=1 << 30) == -1 and f"n={n}" in _err()
    need = _l().embnet_tsne_workspace_bytes(100)
    assert fn(ws_bytes=need - 8) == -3 and "workspace" in _err()
    assert fn(ws=FAKE + 4) == -1 and "aligned" in _err()


def test_rejects_perplexity_and_n_iter():
    for perp in (0.5, 100.0, 250.0, float("nan")):
        assert _aff(n=100, perp=perp) == -1 and "perplexity" in _err(), perp
    assert _it(n_iter=-1) == -1 and "n_iter" in _err()


# ---- the restatement against scikit-learn's recorded results -----------------------------------------------------------
def _golden():
    return np.load(GOLDEN)


def _square(cond, n):
    p = np.zeros((n, n))
    p[np.triu_indices(n, 1)] = cond
    return p + p.T


@pytest.mark.parametrize("k", [0, 1])
def test_restatement_joint_probabilities_match_sklearn(k):
    g = _golden()
    x = g[f"x{k}"]
    n = len(x)
    want = _square(g[f"p{k}"].astype(np.float64), n)
    p, beta = R.joint_probabilities(R.squared_distances(x), float(g["perplexity"]))
    err = np.abs(p - want).max()
    print(f"input {k}: max |P - sklearn P| = {err:.3e} = {err / want.max():.2e} of max P")
    assert err <= 1e-6 * want.max()
    assert np.array_equal(p, p.T) and np.all(np.diag(p) == 0) and abs(p.sum() - 1) < 1e-12
    d2 = R.squared_distances(x).astype(np.float64)
    for i in (0, n // 2, n - 1):
        assert abs(R.perplexity_of(np.delete(d2[i], i), beta[i]) / float(g["perplexity"]) - 1) < 2e-5


@pytest.mark.parametrize("k", [0, 1])
def test_restatement_kl_and_gradient_match_sklearn(k):
    g = _golden()
    n = len(g[f"x{k}"])
    p = _square(g[f"p{k}"].astype(np.float64), n)
    kl, grad, kl_abs, grad_abs, _ = R.kl_and_grad(p, g[f"yfix{k}"].astype(np.float64))
    assert abs(kl - float(g[f"kl_fix{k}"])) <= 1e-10 * abs(float(g[f"kl_fix{k}"]))
    want = g[f"grad_fix{k}"]
    assert np.abs(grad - want).max() <= 1e-10 * np.abs(want).max()
    assert kl_abs >= abs(kl) and np.all(grad_abs >= np.abs(grad))


def test_restatement_sign_test_survives_fp32_underflow():
    y = np.zeros((2, 2), np.float32)
    upd = np.array([[2e-38, -2e-38], [2e-38, -2e-38]], np.float32)
    grad = np.array([[-1e-9, -1e-9], [1e-9, 1e-9]], np.float32)
    assert np.all(upd * grad == 0)                          # what a product test would see
    gains = np.ones((2, 2), np.float32)
    R.update(y, upd, gains, grad, np.float32(0.8), np.float32(50.0))
    assert np.allclose(gains, [[1.2, 0.8], [0.8, 1.2]])


def test_fixture_inputs_are_fit_for_the_end_to_end_check():
    g = _golden()
    assert os.path.getsize(GOLDEN) < 1 << 20
    for k in range(int(g["n_inputs"])):
        assert g[f"sk0_{k}"][0] >= 0.25                     # overlapping classes: a relative KL gap means something
        assert g[f"p_slack{k}"] > 0


# ---- Python surface -----------------------------------------------------------------------------------------------------
def test_tsne_constructor_and_errors():
    from embeddingnet_amd.tsne import TSNE
    t = TSNE()
    assert (t.n_components, t.perplexity, t.early_exaggeration, t.learning_rate, t.max_iter) == (2, 30.0, 12.0, 'auto', 1000)
    assert (t.n_iter_without_progress, t.min_grad_norm, t.init, t.random_state) == (300, 1e-7, 'pca', None)
    assert list(inspect.signature(TSNE.__init__).parameters)[1:] == [
        "n_components", "perplexity", "early_exaggeration", "learning_rate", "max_iter", "n_iter_without_progress",
        "min_grad_norm", "init", "random_state", "device"]
    with pytest.raises(ValueError, match="n_components"):
        TSNE(n_components=3)
    with pytest.raises(ValueError, match="learning_rate"):
        TSNE(learning_rate=-1.0)
    with pytest.raises(ValueError, match="max_iter"):
        TSNE(max_iter=100)
    with pytest.raises(ValueError, match="init"):
        TSNE(init="spectral")
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
        TSNE(perplexity=30.0).fit_transform(np.zeros((20, 4), np.float32))


def test_pca_init_matches_the_restatement_up_to_sign():
    from embeddingnet_amd.tsne import pca_init
    x = _golden()["x0"]
    a, b = pca_init(x), R.pca_init(x)
    assert a.dtype == np.float32 and a.shape == (len(x), 2)
    assert abs(np.std(a[:, 0]) - 1e-4) < 1e-9
    for c in range(2):
        assert min(np.abs(a[:, c] - b[:, c]).max(), np.abs(a[:, c] + b[:, c]).max()) < 1e-8


def test_utils_exposes_the_reference_plot_functions():
    import embedding_net.utils
    import embeddingnet_amd.utils as U
    from embedding_net.utils import load_encodings, plot_tsne, plot_tsne_interactive  # noqa: F401
    assert list(inspect.signature(U.load_encodings).parameters) == ["path_to_encodings"]
    assert list(inspect.signature(U.plot_tsne).parameters) == ["encodings_path", "save_plot_dir", "show"]
    assert inspect.signature(U.plot_tsne).parameters["show"].default is True
    assert list(inspect.signature(U.plot_tsne_interactive).parameters) == ["encodings"]
    assert embedding_net.utils.plot_tsne is U.plot_tsne
    assert embedding_net.utils.plot_tsne_interactive is U.plot_tsne_interactive


def test_load_encodings_round_trip(tmp_path):
    import pickle
    from embeddingnet_amd.utils import load_encodings
    enc = {"encodings": np.arange(6, dtype=np.float32).reshape(3, 2), "labels": ["a", "b", "a"]}
    path = tmp_path / "encodings.pkl"
    path.write_bytes(pickle.dumps(enc))
    got = load_encodings(str(path))
    assert got["labels"] == enc["labels"] and np.array_equal(got["encodings"], enc["encodings"])
