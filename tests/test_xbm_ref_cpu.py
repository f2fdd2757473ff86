"""tests/xbm_ref.py, the float64 restatement the cross-batch-memory kernels are tested against (tests/test_xbm_gpu.py), checked without
a GPU: against torch float64 autograd of the plain formulas, against a scalar triple loop, against ms_ref when the bank is the
class-contiguous batch itself, on hand cases, the ring against a Python list; and the fitness of every input of the GPU test.
"""
import functools

import numpy as np
import pytest
import torch

import ms_ref as M
import xbm_ref as X

SMALL = ("bank_is_batch", "ragged", "ragged_one_class", "low_end")


@functools.lru_cache(maxsize=None)
def _case(name):
    return X.case_inputs(name)


def _args(c):
    return c["x"], c["labels"], c["mem"], c["mem_labels"], c["self_slots"]


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _torch_loss(kind, x, mem, ref):
    """The plain formulas (log(1 + sum exp), no stable form) in torch float64, the kept sets as constants."""
    s = x @ mem.T
    kp, kn = torch.tensor(ref["keep_pos"]), torch.tensor(ref["keep_neg"])
    zero = torch.zeros((), dtype=torch.float64)
    if kind == "contrastive":
        ell = torch.where(kp, 1.0 - s, zero).sum(1) + torch.where(kn, s, zero).sum(1)
    else:
        par = ref["par"]
        ell = (torch.log1p(torch.where(kp, torch.exp(-par["alpha"] * (s - par["base"])), zero).sum(1)) / par["alpha"]
               + torch.log1p(torch.where(kn, torch.exp(par["beta"] * (s - par["base"])), zero).sum(1)) / par["beta"])
        ell = torch.where(torch.tensor(ref["active"]), ell, zero)
    return ell.sum() / x.shape[0], s


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("name", SMALL + ("trips",))
def test_reference_against_float64_autograd(name, kind):
    c = _case(name)
    ref = X.reference(kind, *_args(c), **c["params"][kind])
    x = torch.tensor(c["x"].astype(np.float64), requires_grad=True)
    mem = torch.tensor(c["mem"].astype(np.float64), requires_grad=True)
    loss, s = _torch_loss(kind, x, mem, ref)
    s.retain_grad()
    (0.75 * loss).backward()
    n = x.shape[0]
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
    assert np.allclose(s.grad.numpy() * n / 0.75, ref["G"], rtol=1e-10, atol=1e-300)
    want, _ = X.grad(c["mem"], ref["G"], 0.75)
    assert np.allclose(x.grad.numpy(), want, rtol=1e-10, atol=1e-18)
    unl = c["labels"] < 0
    assert not ref["G"][unl].any() and not want[unl].any() and not ref["G"][:, c["mem_labels"] < 0].any()


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("name", SMALL)
def test_reference_against_a_scalar_triple_loop(name, kind):
    c = _case(name)
    ref = X.reference(kind, *_args(c), **c["params"][kind])
    loss, g, counts = X.scalar_reference(kind, *_args(c), **c["params"][kind])
    assert abs(loss - ref["loss"]) <= 1e-12 * max(1.0, abs(loss))
    assert np.array_equal(g != 0, ref["G"] != 0) and np.allclose(g, ref["G"], rtol=1e-11, atol=0)
    assert np.array_equal(counts, ref["counts"])


@pytest.mark.parametrize("p,k,e", [(4, 2, 4), (5, 7, 33), (8, 4, 64)])
def test_multi_similarity_on_a_bank_that_is_the_batch_is_ms_ref(p, k, e):
    import recipes as R
    x = R.clustered_embeddings(M.seed_of(p, k, e), p, k, e, M.SIGMA)
    lab = np.repeat(np.arange(p), k).astype(np.int32)
    ref = X.reference("multi_similarity", x, lab, x, lab, np.arange(p * k, dtype=np.int32))
    want = M.reference(x, p, k)
    assert ref["loss"] == pytest.approx(want["loss"], rel=1e-13)
    assert np.array_equal(ref["keep_pos"], want["keep_pos"]) and np.array_equal(ref["keep_neg"], want["keep_neg"])
    assert np.allclose(ref["G"], want["G"], rtol=1e-13, atol=0)
    assert np.array_equal(ref["counts"][:3], want["counts"][:3]) and ref["counts"][3] == p * k
    bg, _, bl = X.bounds(ref, X.gamma_s(e))                 # the same chain of bounds; here both sides' lane chains cover m columns
    wg, _, wl = M.bounds(x, want, M.gamma_s("similarity_matrix", e))
    assert np.all(bg >= wg * (1 - 1e-12)) and bl >= wl * (1 - 1e-12)


# ---------------------------------------------------------------------------------------------------------------- hand cases
def _hand(kind, x, lab, mem, mlab, slots=None, **params):
    return X.reference(kind, np.asarray(x, np.float32), np.asarray(lab, np.int32), np.asarray(mem, np.float32),
                       np.asarray(mlab, np.int32), None if slots is None else np.asarray(slots, np.int32), **params)


def test_hand_contrastive_values():
    # anchor (1, 0) of class 0: a positive at S = 0.5, a negative above the margin (S = 0.75), one below (0.25), one at S = 0
    ref = _hand("contrastive", [[1, 0], [0, 1]], [0, 1], [[0.5, 0], [0.75, 0], [0.25, 0], [0, 1]], [0, 1, 1, 1])
    assert ref["G"][0].tolist() == [-1, 1, 0, 0] and ref["ell"][0] == 0.5 + 0.75
    # anchor (0, 1) of class 1: two positives at S = 0 (term 1 each) and one at S = 1, where fl(1 - S) = 0 is not > 0
    assert ref["G"][1].tolist() == [0, -1, -1, 0] and ref["ell"][1] == 2
    assert ref["loss"] == 3.25 / 2 and ref["counts"].tolist() == [3, 1, 2, 4]


@pytest.mark.parametrize("kind", X.KINDS)
def test_hand_an_anchor_without_positives_or_without_negatives(kind):
    mem, mlab = [[0.9, 0.1], [0.8, 0.3], [0.2, 0.9]], [0, 0, 0]
    ref = _hand(kind, [[1, 0], [0.6, 0.6]], [0, 5], mem, mlab)
    # anchor 0: no negatives; anchor 1: no positives (its class is absent)
    assert not ref["neg"][0].any() and ref["pos"][0].all() and not ref["pos"][1].any() and ref["neg"][1].all()
    if kind == "multi_similarity":                          # either side empty: nothing kept
        assert not ref["G"].any() and ref["loss"] == 0 and ref["counts"].tolist() == [0, 0, 0, 3]
    else:                                                   # the sides are independent
        assert ref["G"][0].tolist() == [-1, -1, -1] and ref["G"][1].tolist() == [1, 1, 1]
        assert ref["counts"].tolist() == [3, 3, 2, 3]


@pytest.mark.parametrize("kind", X.KINDS)
def test_hand_unlabelled_rows_empty_slots_and_self_slots(kind):
    x = [[0.8, 0.2], [0.7, 0.4], [0.1, 0.9], [0.3, 0.8]]
    mem = [[0.8, 0.2], [0.7, 0.4], [0.1, 0.9], [0.3, 0.8], [0, 0], [0.5, 0.5]]
    mlab = [0, 0, 1, 1, -1, -3]                             # an empty slot and an unlabelled one
    base = _hand(kind, x, [0, 0, 1, 1], mem, mlab, [0, 1, 2, 3])
    assert not base["G"][:, 4:].any() and base["counts"][3] == 4
    assert not np.diag(base["G"][:, :4]).any()              # the own copies are left out
    unl = _hand(kind, x, [0, -1, 1, -2], mem, mlab, [0, 1, 2, 3])
    assert not unl["G"][[1, 3]].any() and unl["ell"][1] == 0 and unl["ell"][3] == 0
    assert unl["loss"] == pytest.approx((unl["ell"][0] + unl["ell"][2]) / 4)      # n counts every row
    assert np.array_equal(unl["G"][[0, 2]], base["G"][[0, 2]])
    # a self slot outside [0, m) excludes nothing: the same as no self slots at all
    out = _hand(kind, x, [0, 0, 1, 1], mem, mlab, [-1, 6, 1 << 20, -5])
    none = _hand(kind, x, [0, 0, 1, 1], mem, mlab, None)
    assert np.array_equal(out["G"], none["G"]) and out["loss"] == none["loss"]
    assert out["pos"][0, 0] and not base["pos"][0, 0]


# ---------------------------------------------------------------------------------------------------------------- the ring
@pytest.mark.parametrize("m,sizes", [(40, [12] * 7), (5, [5, 5, 5]), (7, [3, 1, 7, 2, 6, 4]), (1, [1, 1])])
def test_ring_against_a_python_list(m, sizes):
    rs = np.random.RandomState(m)
    ring, feats, labels, cursor, stamp = X.Ring(m, 3), [None] * m, [-1] * m, 0, 0
    for n in sizes:
        emb = rs.rand(n, 3).astype(np.float32)
        lab = np.arange(stamp, stamp + n, dtype=np.int32)
        stamp += n
        slots = ring.enqueue(emb, lab)
        for i in range(n):
            assert slots[i] == cursor
            feats[cursor], labels[cursor] = emb[i], int(lab[i])
            cursor = cursor + 1 if cursor + 1 < m else 0
        assert ring.cursor == cursor and ring.labels.tolist() == labels
        for j in range(m):
            assert np.array_equal(ring.feats[j], np.zeros(3, np.float32) if feats[j] is None else feats[j])
    with pytest.raises(AssertionError):
        ring.enqueue(np.zeros((m + 1, 3), np.float32), np.zeros(m + 1, np.int32))


# ---------------------------------------------------------------------------------------------------------------- the GPU test's inputs
def test_range_and_workspace():
    assert X.in_range(4, 4, 1) and X.in_range(8, 65536, 16) and X.in_range(1024, 65536, 4096) and X.in_range(4096, 16384, 1)
    assert not X.in_range(1, 4, 4) and not X.in_range(8, 4, 4) and not X.in_range(8, 65537, 4) and not X.in_range(2048, 65536, 4)
    assert X.workspace_bytes(8, 4, 4) == 0 and X.workspace_bytes(12, 40, 5) == 16 + 96 + 192 + 1920
    assert all(X.in_range(*shape) for shape in X.SHAPES.values())


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("name", X.CASES)
def test_gpu_inputs_are_fit(name, kind):
    """At most 1 % of an input's keep / drop decisions may be open under the bound on S (a condition on the input: a miss is mended
    by its seed or spread).  Grid inputs: S is exact in any order, nothing is open."""
    c = _case(name)
    n, m, e = X.SHAPES[name]
    exact = c["unit"] is not None
    if exact:
        assert X.exact_in_any_order(c["x"], c["mem"], c["unit"])
    assert exact == (name in ("grid", "low_end"))
    d = X.decisions(kind, *_args(c), X.gamma_s(e, exact), **c["params"][kind])
    print(name, kind, "open pairs", int(d["open"].sum()), "share", d["share"])
    assert d["share"] <= 0.01
    if exact:
        assert not d["open"].any()
    assert np.all(d["sure_pos"] <= d["may_pos"]) and np.all(d["sure_neg"] <= d["may_neg"])
    ref = X.reference(kind, *_args(c), **c["params"][kind])
    assert np.all(d["sure_pos"] <= ref["keep_pos"]) and np.all(ref["keep_pos"] <= d["may_pos"])
    assert np.all(d["sure_neg"] <= ref["keep_neg"]) and np.all(ref["keep_neg"] <= d["may_neg"])
    bg, bell, bl = X.bounds(ref, X.gamma_s(e, exact))
    assert np.isfinite(bl) and np.isfinite(bg).all()
    # what each case is there for
    lab, mlab, slots = c["labels"], c["mem_labels"], c["self_slots"]
    if name == "ragged":
        assert (lab < 0).sum() == 2 and (mlab < 0).sum() >= 5 and (slots < 0).sum() == 1
        assert (slots >= 34).any() and ((slots >= 0) & (slots <= 5)).any()           # the self slots wrap the ring's end
        own = np.zeros(m, bool)
        own[slots[slots >= 0]] = True
        assert any(not (mlab[~own] == cl).any() for cl in set(lab[lab >= 0].tolist()))     # a class present only in the batch
        assert 0 < ref["counts"][0] and 0 < ref["counts"][1] and ref["counts"][2] == 10
    if name == "ragged_one_class":
        assert len(set(mlab[mlab >= 0].tolist())) == 1
        full = lab == mlab[mlab >= 0][0]
        assert full.any() and not ref["neg"][full].any() and ref["pos"][full].any()
    if name == "bank_is_batch":
        assert np.array_equal(c["mem"], c["x"]) and slots.tolist() == list(range(n))
    if name in ("trips", "edge", "grid"):
        assert ref["counts"][2] == n and slots.min() == 0 and slots.max() == m - 1
