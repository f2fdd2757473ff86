"""SupCon / NT-Xent, host side (no GPU): the C ABI is declared and exported and refuses arguments outside its range before any
launch; the float64 restatement in tests/supcon_ref.py agrees with torch.logsumexp under autograd, with central differences, with a
scalar restatement and with cases worked by hand; the Python layers know the mode; and the inputs of tests/test_supcon_gpu.py are
fit for what that test asserts on them."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import ms_ref as M
import recipes as R
import supcon_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_supcon_loss_path", "embnet_supcon_loss_workspace_bytes", "embnet_supcon_loss_fwd")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced
DENOMS = list(C.DENOMINATORS)


# ---------------------------------------------------------------------------------------------------------------- 1. the ABI
def _lib():
    from embeddingnet_amd import _lib
    return _lib.lib()


def test_header_declares_and_library_exports_supcon_loss():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported
    assert exported == set(protos)
    assert _lib.lib().embnet_abi_version() == 22


def _fwd(p, k, e, tau=0.1, denom=1, ws=FAKE, ws_bytes=1 << 31, path=0, null=None):
    l = _lib()
    a = dict(emb=FAKE, g=FAKE, counts=FAKE, mean=FAKE, ws=ws)
    if null:
        a[null] = None
    rc = l.embnet_supcon_loss_fwd(a["emb"], p, k, e, tau, denom, path, a["g"], a["counts"], a["mean"], a["ws"], ws_bytes, None)
    return rc, l.embnet_last_error().decode()


@pytest.mark.parametrize("null", ["emb", "g", "counts", "mean", "ws"])
def test_fwd_rejects_null_pointers(null):
    rc, msg = _fwd(8, 4, 256, null=null)
    assert rc == -1 and "supcon_loss_fwd: null pointer" in msg


@pytest.mark.parametrize("p,k,e,what", [(1, 4, 64, "p >= 2"), (4, 1, 64, "k >= 2"), (2, 2049, 16, "n = p*k = 4098"),
                                        (8, 4, 0, "e=0"), (8, 4, 4097, "e=4097")])
def test_fwd_rejects_out_of_range_shapes(p, k, e, what):
    rc, msg = _fwd(p, k, e)
    assert rc == -1 and what in msg and msg.startswith("supcon_loss_fwd"), msg
    assert _lib().embnet_supcon_loss_path(p, k, e) == 0 and _lib().embnet_supcon_loss_workspace_bytes(p, k, e) == 0


@pytest.mark.parametrize("tau", [0.0, -0.1, math.nan, math.inf, -math.inf])
def test_fwd_rejects_a_temperature_that_is_not_positive_and_finite(tau):
    rc, msg = _fwd(8, 4, 256, tau=tau)
    assert rc == -1 and "temperature" in msg, msg


@pytest.mark.parametrize("denom", [0, 3, -1])
def test_fwd_rejects_an_unknown_denominator(denom):
    rc, msg = _fwd(8, 4, 256, denom=denom)
    assert rc == -1 and "unknown denominator" in msg, msg


def test_fwd_rejects_bad_workspace_and_path():
    need = _lib().embnet_supcon_loss_workspace_bytes(8, 4, 256)
    assert need >= 16 + 32 * 8 + 32 * 16 + 32 * 32 * 4
    for denom in (1, 2):
        rc, msg = _fwd(8, 4, 256, denom=denom, ws_bytes=need - 16)
        assert rc == -3 and "workspace" in msg
        rc, msg = _fwd(8, 4, 256, denom=denom, ws=FAKE + 4)
        assert rc == -1 and "16-byte aligned" in msg
        rc, msg = _fwd(8, 4, 256, denom=denom, path=3)
        assert rc == -1 and "unknown path" in msg
        rc, msg = _fwd(4, 32, 64, denom=denom, path=1)      # k > 16: only the similarity-matrix path
        assert rc == -1 and "per-class path" in msg


def test_paths_and_workspace_follow_the_multi_similarity_fit_rule():
    l = _lib()
    shapes = M.PER_CLASS_SHAPES + C.MATRIX_SHAPES + [(32, 16, 16), (33, 16, 16), (2, 17, 8), (4, 4, 4080), (4, 4, 4081), (2, 2, 1),
                                                     (2, 2048, 4096)]
    for p, k, e in shapes:
        want = {"per_class": 1, "similarity_matrix": 2}[M.auto_path(p, k, e)]
        assert l.embnet_supcon_loss_path(p, k, e) == want == l.embnet_ms_loss_path(p, k, e), (p, k, e)
        assert l.embnet_supcon_loss_workspace_bytes(p, k, e) == l.embnet_ms_loss_workspace_bytes(p, k, e) >= (p * k) ** 2 * 4
    for p, k, e in M.PER_CLASS_SHAPES:
        assert l.embnet_supcon_loss_path(p, k, e) == 1
    for p, k, e in C.MATRIX_SHAPES:
        assert l.embnet_supcon_loss_path(p, k, e) == 2


# ---------------------------------------------------------------------------------------------------------------- 2. the layers
def _cfg(mode, model_mode="triplet", **gen):
    return dict(generator=dict(negatives_selection_mode=mode, **gen), model=dict(mode=model_mode))


def test_python_layers_know_the_mode():
    from embeddingnet_amd import losses_and_accuracies, ops
    from embeddingnet_amd.datagenerators import SyntheticDataLoader, TripletsDataGenerator
    from embeddingnet_amd.train_step import TripletTrainer
    assert callable(losses_and_accuracies.supcon_loss(8, 4, 0.2, "negatives"))
    assert ops.SUPCON_PATHS["similarity_matrix"] == 2 and ops.SUPCON_DENOMINATORS == dict(all=1, negatives=2)
    assert "supcon" in TripletsDataGenerator.STEP_ONLY_MODES
    data = SyntheticDataLoader(6, 4, (8, 8, 3), validate=False)
    gen = TripletsDataGenerator(embedding_model=None, class_files_paths=data.train_data, class_names=data.class_names,
                                n_batches=2, input_shape=[8, 8, 3], k_classes=3, k_samples=2, negatives_selection_mode="supcon")
    with pytest.raises(ValueError, match="TripletTrainer"):
        gen.mine_batch(gen.sample_batch())
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    tr = TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="supcon",
                        loss_params=dict(temperature=0.5, denominator="negatives"))
    assert tr.loss_params == dict(temperature=0.5, denominator="negatives")
    assert TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="supcon").loss_params == {}
    with pytest.raises(ValueError, match="multi_similarity"):
        TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="semihard", loss_params=dict(temperature=1.0))
    with pytest.raises(ValueError, match="unknown keys"):                      # per mode: the other loss's keys are unknown
        TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="supcon", loss_params=dict(alpha=1.0))
    with pytest.raises(ValueError, match="unknown keys"):
        TripletTrainer(torch.nn.Identity(), opt, 3, 2, negatives_selection_mode="multi_similarity",
                       loss_params=dict(temperature=1.0))


def test_train_config_function_accepts_and_refuses_the_key():
    import importlib.util
    spec = importlib.util.spec_from_file_location("embnet_tools_train", os.path.join(ROOT, "tools", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    assert train.supcon_loss_config(_cfg("supcon")) is None
    assert train.supcon_loss_config(_cfg("supcon", supcon_loss=dict(temperature=1, denominator="negatives"))) == \
        dict(temperature=1.0, denominator="negatives")
    assert train.supcon_loss_config(_cfg("supcon", supcon_loss=dict(temperature=0.07))) == dict(temperature=0.07)
    for mode in ("semihard", "multi_similarity", "batch_all"):
        with pytest.raises(ValueError, match="GENERATOR.supcon_loss"):
            train.supcon_loss_config(_cfg(mode, supcon_loss=dict(temperature=0.1)))
    with pytest.raises(ValueError, match="Siamese"):
        train.supcon_loss_config(_cfg("supcon", model_mode="siamese", supcon_loss=dict(temperature=0.1)))
    with pytest.raises(ValueError, match="GENERATOR.ms_loss"):                 # ms_loss stays refused with supcon
        train.ms_loss_config(_cfg("supcon", ms_loss=dict(alpha=2.0)))
    for bad in (dict(alpha=2.0), dict(temperature="hot"), dict(temperature=True), dict(temperature=0.0),
                dict(denominator="some"), [0.1]):
        with pytest.raises(ValueError, match="GENERATOR.supcon_loss"):
            train.supcon_loss_config(_cfg("supcon", supcon_loss=bad))


# ---------------------------------------------------------------------------------------------------------------- 3. the reference
def _torch_total(s, p, k, tau, denom):
    """The header's plain formulas on a torch float64 S through torch.logsumexp.  -> sum_i l_i."""
    pos, neg = (torch.tensor(m) for m in M.class_masks(p, k))
    n = p * k
    t = s / tau
    ninf = torch.tensor(-math.inf, dtype=torch.float64)
    if denom == "all":
        off = ~torch.eye(n, dtype=torch.bool)
        return (torch.logsumexp(torch.where(off, t, ninf), 1) - (t * pos).sum(1) / (k - 1)).sum()
    lse_n = torch.logsumexp(torch.where(neg, t, ninf), 1)
    lp = torch.logaddexp(t, lse_n[:, None]) - t
    return ((lp * pos).sum(1) / (k - 1)).sum()


@pytest.mark.parametrize("denom", DENOMS)
@pytest.mark.parametrize("p,k,e,tau,scale", [(8, 4, 64, 0.1, 1.0), (5, 7, 33, 0.05, 1.0), (3, 2, 1, 0.5, 1.0), (6, 4, 64, 0.1, 30.0),
                                             (4, 2, 16, 100.0, 1.0)])
def test_reference_equals_autograd_of_torch_logsumexp(denom, p, k, e, tau, scale):
    x = (R.clustered_embeddings(3 + e, p, k, e, 0.8) * np.float32(scale)).astype(np.float32)
    ref = C.reference(x, p, k, tau, denom)
    tau = C.tau32(tau)
    s = torch.tensor(ref["S"], requires_grad=True)
    total = _torch_total(s, p, k, tau, denom)
    total.backward()
    assert abs(float(total.detach()) / (p * k) - ref["loss"]) <= 1e-13 * abs(ref["loss"])
    gmax = np.abs(ref["G"]).max()
    np.testing.assert_allclose(ref["G"], s.grad.numpy(), rtol=1e-10, atol=1e-13 * gmax)
    assert np.all(np.abs(ref["G"].sum(1)) <= 1e-12 * gmax) and not np.diag(ref["G"]).any()     # every row of G sums to zero
    # and the embedding gradient: demb = (1/N) (G + G^T) X is autograd's of loss(X X^T)
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    (_torch_total(xt @ xt.T, p, k, tau, denom) / (p * k)).backward()
    want, _ = M.grad(x, ref["G"])
    scale = (np.abs(ref["G"] + ref["G"].T) @ np.abs(x.astype(np.float64))).max() / (p * k)      # rows of G sum to zero: it cancels
    np.testing.assert_allclose(want, xt.grad.numpy(), rtol=1e-9, atol=1e-12 * scale)


def _scalar(x, p, k, tau, denom):
    """The header's sentences one anchor and one pair at a time (Python floats): shares nothing with supcon_ref.reference but the
    text.  The plain formulas: fine for unit rows at moderate temperatures."""
    tau = C.tau32(tau)
    x = np.asarray(x, np.float32).astype(np.float64)
    n = p * k
    s = [[float(np.dot(x[i], x[j])) for j in range(n)] for i in range(n)]
    g = np.zeros((n, n))
    ell = np.zeros(n)
    viol = 0
    for i in range(n):
        pos = [j for j in range(n) if j // k == i // k and j != i]
        neg = [j for j in range(n) if j // k != i // k]
        viol += max(np.float32(s[i][j]) for j in neg) >= min(np.float32(s[i][j]) for j in pos)
        ex = {j: math.exp(s[i][j] / tau) for j in pos + neg}
        if denom == "all":
            tot = sum(ex.values())
            ell[i] = math.log(tot) - sum(s[i][j] / tau for j in pos) / (k - 1)
            for j in pos + neg:
                g[i, j] = (ex[j] / tot - (1.0 / (k - 1) if j in pos else 0.0)) / tau
        else:
            sn = sum(ex[j] for j in neg)
            ell[i] = sum(math.log(ex[j] + sn) - s[i][j] / tau for j in pos) / (k - 1)
            for j in pos:
                g[i, j] = (ex[j] / (ex[j] + sn) - 1.0) / (tau * (k - 1))
            for j in neg:
                g[i, j] = ex[j] * sum(1.0 / (ex[q] + sn) for q in pos) / (tau * (k - 1))
    return ell.sum() / n, ell, g, [n * (k - 1), viol]


@pytest.mark.parametrize("denom", DENOMS)
@pytest.mark.parametrize("p,k,e,tau", [(3, 3, 8, 0.1), (5, 2, 16, 0.05), (2, 6, 4, 0.3), (4, 4, 33, 1.0), (3, 2, 1, 0.5)])
def test_reference_equals_the_scalar_restatement(denom, p, k, e, tau):
    x = R.clustered_embeddings(17 + p, p, k, e, 0.8)
    ref = C.reference(x, p, k, tau, denom)
    loss, ell, g, counts = _scalar(x, p, k, tau, denom)
    assert list(ref["counts"]) == counts
    np.testing.assert_allclose(ref["ell"], ell, rtol=1e-12)
    np.testing.assert_allclose(ref["G"], g, rtol=1e-11, atol=1e-13 * np.abs(g).max())
    assert abs(ref["loss"] - loss) <= 1e-13 * abs(loss)


@pytest.mark.parametrize("denom", DENOMS)
def test_central_differences_in_s(denom):
    p, k, e, tau = 6, 4, 32, 0.1
    x = R.clustered_embeddings(9, p, k, e, 0.8)
    ref = C.reference(x, p, k, tau, denom)
    s = ref["S"]

    def total(sm):
        return float(_torch_total(torch.tensor(sm), p, k, C.tau32(tau), denom))

    rs = np.random.RandomState(0)
    h = 1e-5                                                # truncation: h^2 / (6 tau^2) = 2e-9 relative to 1/tau
    noise = 16 * 2.0 ** -52 * abs(total(s)) / h             # rounding of the two float64 totals under the division by 2 h
    for _ in range(60):
        i, j = rs.randint(0, p * k, 2)
        sp, sm = s.copy(), s.copy()
        sp[i, j] += h
        sm[i, j] -= h
        fd = (total(sp) - total(sm)) / (2 * h)
        assert abs(fd - ref["G"][i, j]) <= 1e-6 / C.tau32(tau) + noise, (i, j, fd, ref["G"][i, j])


@pytest.mark.parametrize("p,k,e,tau", [(4, 3, 5, 0.1), (3, 2, 1, 0.07), (2, 5, 7, 2.0)])
def test_all_rows_equal_worked_by_hand(p, k, e, tau):
    """Every logit is the same: 'all' l = log(n - 1), 'negatives' l = log(1 + n - k); G = (1/tau)(1/(n-1) - [pos]/(k-1)) and
    (1/tau)(1/(k-1))(1/(1+n-k) - 1) on positives, (1/tau)(1/(1+n-k)) on negatives."""
    n = p * k
    x = np.tile(np.linspace(0.25, 1.0, e, dtype=np.float32), (n, 1))
    pos, neg = M.class_masks(p, k)
    t = C.tau32(tau)
    ref = C.reference(x, p, k, tau, "all")
    np.testing.assert_allclose(ref["ell"], math.log(n - 1), rtol=1e-14)
    np.testing.assert_allclose(ref["G"], (1.0 / (n - 1) * (pos | neg) - pos / (k - 1.0)) / t, rtol=1e-13, atol=1e-15 / t)
    ref = C.reference(x, p, k, tau, "negatives")
    np.testing.assert_allclose(ref["ell"], math.log(1 + n - k), rtol=1e-14)
    want = (pos * (1.0 / (1 + n - k) - 1.0) / (k - 1.0) + neg * 1.0 / (1 + n - k)) / t
    np.testing.assert_allclose(ref["G"], want, rtol=1e-13, atol=1e-15 / t)
    assert list(ref["counts"]) == [n * (k - 1), n]         # max_n S = min_p S: every anchor violates (>=)


@pytest.mark.parametrize("p,k,tau", [(4, 3, 0.1), (3, 2, 0.5), (5, 4, 0.02)])
def test_one_hot_class_rows_worked_by_hand(p, k, tau):
    """Row = its class's unit vector: S = 1 within a class, 0 across.  'all': l = log((k-1) e^{1/tau} + n - k) - 1/tau;
    'negatives': l = log(e^{1/tau} + n - k) - 1/tau.  (tau = 0.02: e^50, the stable form's business.)"""
    n = p * k
    x = np.repeat(np.eye(p, dtype=np.float32), k, axis=0)
    t = C.tau32(tau)
    ref = C.reference(x, p, k, tau, "all")
    np.testing.assert_allclose(ref["ell"], math.log((k - 1) * math.exp(1 / t) + n - k) - 1 / t, rtol=1e-12, atol=16 * 2.0 ** -53 / t)
    ref = C.reference(x, p, k, tau, "negatives")
    np.testing.assert_allclose(ref["ell"], math.log(math.exp(1 / t) + n - k) - 1 / t, rtol=1e-12, atol=16 * 2.0 ** -53 / t)
    assert list(ref["counts"]) == [n * (k - 1), 0]
    assert np.all(np.abs(ref["G"].sum(1)) <= 1e-13 / t)


def test_smallest_batch_of_one_dimensional_embeddings():
    """3 x 2, e = 1, k = 2 (one positive per anchor): both denominators against the scalar restatement and torch."""
    x = np.array([[1.0], [0.5], [-1.0], [-0.75], [0.25], [2.0]], np.float32)
    for denom in DENOMS:
        ref = C.reference(x, 3, 2, 0.5, denom)
        loss, ell, g, counts = _scalar(x, 3, 2, 0.5, denom)
        np.testing.assert_allclose(ref["G"], g, rtol=1e-12, atol=1e-15)
        assert abs(ref["loss"] - loss) <= 1e-14 * abs(loss) and list(ref["counts"]) == counts
        assert np.all(np.abs(ref["G"].sum(1)) <= 1e-14)
        total = _torch_total(torch.tensor(ref["S"]), 3, 2, 0.5, denom)
        assert abs(float(total) / 6 - ref["loss"]) <= 1e-14 * abs(ref["loss"])


def test_underflow_trap_is_what_it_claims():
    """float32 arithmetic under ONE maximum per anchor gives log 0 on the trap; the reference's per-pair maximum does not."""
    x, p, k = C.underflow_trap()
    ref = C.reference(x, p, k, C.TRAP_TAU, "negatives")
    assert np.isfinite(ref["loss"]) and np.isfinite(ref["G"]).all()
    t = (ref["S"][0] / C.tau32(C.TRAP_TAU)).astype(np.float32)
    assert abs(t[1] - 200) < 1e-3 and abs(t[2] - 40) < 1e-3 and not t[3:].any()
    single = t[1:].max()
    d02 = np.exp(t[2] - single, dtype=np.float32) + np.exp(t[3:] - single, dtype=np.float32).sum(dtype=np.float32)
    assert d02 == 0.0                                       # what the per-anchor maximum would hand to the logarithm
    assert abs(ref["lp"][0, 2] - math.log1p((3 * p - 3) * math.exp(-40.0))) < 1e-12
    bg, bell, bl = C.bounds(x, ref, M.gamma_s("similarity_matrix", 2))
    assert bl < 1e-3 * ref["loss"] and np.isfinite(bg).all()   # logits of 200 cost 200 u each: still far from telling nothing


# ---------------------------------------------------------------------------------------------------------------- 4. the GPU inputs
ALL_SHAPES = sorted(set(M.VALUE_SHAPES) | set(M.CONTINUOUS_SHAPES))


@pytest.mark.parametrize("p,k,e", ALL_SHAPES, ids=str)
def test_continuous_inputs_leave_no_anchor_open(p, k, e):
    """The violating-anchor counter is asserted exactly only where no decision is open: at gamma(E + 1), the wider of the two
    paths' gamma_S, every shape has none, and the counts reach both ends."""
    x = R.clustered_embeddings(M.seed_of(p, k, e), p, k, e, M.SIGMA)
    d = C.decisions(x, p, k, M.gamma_s("similarity_matrix", e))
    assert not d["open"].any()
    assert M.gamma_s("per_class", e) <= M.gamma_s("similarity_matrix", e)
    viol = int(C.reference(x, p, k)["counts"][1])
    assert viol == d["sure"].sum()
    print(f"violating anchors {viol} of {p * k}")


def test_violating_counts_reach_both_ends():
    got = {s: int(C.reference(R.clustered_embeddings(M.seed_of(*s), *s, M.SIGMA), s[0], s[1])["counts"][1]) for s in ALL_SHAPES}
    assert min(got.values()) == 0 and got[(256, 8, 128)] == 1853, got


@pytest.mark.parametrize("p,k,e", M.VALUE_SHAPES + [(4, 32, 64)], ids=str)
def test_grid_inputs_are_exact_and_their_bounds_tight(p, k, e):
    x, _, q = M.grid_inputs(R.clustered_embeddings(M.seed_of(p, k, e), p, k, e, M.SIGMA))
    assert M.exact_in_any_order(x, 1.0 / q)
    assert not C.decisions(x, p, k, 0.0)["open"].any()
    for denom in DENOMS:
        ref = C.reference(x, p, k, 0.1, denom)
        bg, bell, bl = C.bounds(x, ref, 0.0)
        assert bl < 1e-5 * ref["loss"] and bg.max() < 1e-4 * np.abs(ref["G"]).max()
