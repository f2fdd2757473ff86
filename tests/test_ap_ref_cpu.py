"""tests/ap_ref.py on the CPU: the float64 restatement of FastAP and Smooth-AP against torch autograd of the plain formulas, a
float32 NumPy emulation of the header's rounding forms inside the a-priori bounds, hand cases, the fitness of the inputs
tests/test_ap_loss_gpu.py uses (the open-pair cap), tools/train.py's GENERATOR.ap_loss validator, and the new exports."""
import os
import sys

import numpy as np
import pytest
import torch

import ap_ref as A
import ms_ref as M
import recipes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
AUTOGRAD_CASES = [(4, 3, 8), (5, 4, 16)]


def _off(n):
    return ~np.eye(n, dtype=bool)


# ---------------------------------------------------------------------------------------------------------------- 1. autograd
def _plain_fast_ap(s, p, k, bins):
    """The paper's formula: triangular pulses on the centres l * 4 / L, AP of the binned ranking.  s [N,N] float64 leaf."""
    n = p * k
    pos, neg = (torch.tensor(m) for m in M.class_masks(p, k))
    delta = 4.0 / bins
    centres = torch.arange(bins + 1, dtype=torch.float64) * delta
    pulse = torch.relu(1.0 - (2.0 - 2.0 * s)[:, :, None].sub(centres).abs() / delta)
    hp = (pulse * pos[:, :, None]).sum(1)
    hn = (pulse * neg[:, :, None]).sum(1)
    cp, c = hp.cumsum(1), (hp + hn).cumsum(1)
    f = torch.where(c > 0, hp * cp / torch.where(c > 0, c, torch.ones_like(c)), torch.zeros_like(c)).sum(1)
    return (1.0 - f / (k - 1)).sum() / n


def _plain_smooth_ap(s, p, k, tau):
    """The paper's formula: ranks as 1 + sums of sigmoids of similarity differences."""
    n = p * k
    pos, _ = M.class_masks(p, k)
    total = 0.0
    for i in range(n):
        ap = 0.0
        for q in np.nonzero(pos[i])[0]:
            # sigma as exp(log sigma): torch.sigmoid's own derivative is s (1 - s), whose 1 - s loses every digit of a small s'
            sg = torch.nn.functional.logsigmoid((s[i] - s[i, q]) / tau).exp()
            others = torch.ones(n, dtype=torch.bool)
            others[i] = others[q] = False
            # rank among the positives / rank among all = R / (R + Nn), written 1 / (1 + Nn / R): autograd of R / Q forms
            # s'/Q - R s'/Q^2 for a positive column, which cancels to nothing where the negatives' share Nn is small
            rank_pos = 1.0 + sg[others & torch.tensor(pos[i])].sum()
            ap = ap + 1.0 / (1.0 + sg[others & ~torch.tensor(pos[i])].sum() / rank_pos)
        total = total + 1.0 - ap / (k - 1)
    return total / n


@pytest.mark.parametrize("p,k,e", AUTOGRAD_CASES, ids=str)
@pytest.mark.parametrize("loss,params", [("fast_ap", dict(bins=10)), ("fast_ap", dict(bins=7)), ("smooth_ap", dict(temperature=0.01)),
                                         ("smooth_ap", dict(temperature=0.1))], ids=str)
def test_reference_matches_autograd(p, k, e, loss, params):
    x = R.clustered_embeddings(M.seed_of(p, k, e), p, k, e, A.SIGMA)
    ref = A.reference(x, p, k, loss, **params)
    n = p * k
    s = torch.tensor(ref["S"], requires_grad=True)
    if loss == "fast_ap":
        value = _plain_fast_ap(s, p, k, params["bins"])
        assert not A.open_pairs(x, p, k, params["bins"], 0.0, U64).any()         # no pair on a kink of the pulse
    else:
        value = _plain_smooth_ap(s, p, k, A.tau32(params["temperature"]))
    value.backward()
    g = s.grad.numpy() * n
    bg, _, bl, _ = A.bounds(x, ref, 0.0, unit=U64)
    off = _off(n)
    ratio_g = (np.abs(g - ref["G"])[off] / bg[off]).max()
    ratio_l = abs(float(value.detach()) - ref["loss"]) / bl
    print(f"{loss} {params} p={p} k={k} e={e}: G {np.abs(g - ref['G']).max():.3g} ratio {ratio_g:.3g}  loss ratio {ratio_l:.3g}")
    assert np.abs(ref["G"]).max() > 1e-3 and not np.diag(ref["G"]).any()
    assert ratio_g < 1 and ratio_l < 1


@pytest.mark.parametrize("tau", [0.01, 0.1, 10.0])
def test_smooth_ap_reference_rows_sum_to_zero(tau):
    p, k, e = 5, 7, 33
    x = R.clustered_embeddings(M.seed_of(p, k, e), p, k, e, A.SIGMA)
    ref = A.reference(x, p, k, "smooth_ap", temperature=tau)
    bg = A.bounds(x, ref, 0.0, unit=U64)[0]
    ratio = (np.abs(ref["G"].sum(1)) / bg.sum(1)).max()
    print(f"smooth_ap tau={tau}: row sums {np.abs(ref['G'].sum(1)).max():.3g} ratio {ratio:.3g}")
    assert ratio < 1 and np.abs(ref["G"]).max() > 1e-6


# ---------------------------------------------------------------------------------------------------------------- 2. hand cases
def test_fast_ap_by_hand():
    """Two classes of two on the axes of the plane, L = 4 (Delta = 1, u = d).  Anchor (1,0): its positive (0,1) at d = 2, the
    negatives (-1,0) at d = 4 and (0,-1) at d = 2; a d on a centre goes to the interval on its right with f = 0.
    h+ = [0,0,1,0,0], h- = [0,0,1,0,1]; Hp = [0,0,1,1,1], H = [0,0,2,2,3]; F = 1 * 1 / 2, l = 1/2.
    b_2 = c_2 = 1/4: A- = [-1/4,-1/4,-1/4,0,0], A+ = [1/4, 1/4, 3/4, 1/2, 1/3]; coef = 2 inv / (K-1) = 2:
    G(positive, l0 = 2) = 2 (1/2 - 3/4) = -1/2, G(negative at 2) = 2 (0 + 1/4) = 1/2, G(negative at 4) = 2 (0 - 0) = 0.
    Every anchor sees the same picture."""
    x = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], np.float32)
    ref = A.reference(x, 2, 2, "fast_ap", bins=4)
    assert np.array_equal(ref["hp"], np.tile([0, 0, 1, 0, 0], (4, 1))) and np.array_equal(ref["hn"], np.tile([0, 0, 1, 0, 1], (4, 1)))
    assert np.array_equal(ref["ell"], np.full(4, 0.5)) and ref["loss"] == 0.5
    assert np.allclose(ref["A_pos"][0], [0.25, 0.25, 0.75, 0.5, 1 / 3], atol=1e-15)
    assert np.array_equal(ref["A_neg"][0], [-0.25, -0.25, -0.25, 0, 0])
    want = np.array([[0, -.5, 0, .5], [-.5, 0, .5, 0], [0, .5, 0, -.5], [.5, 0, -.5, 0]])
    assert np.allclose(ref["G"], want, atol=1e-15)
    assert np.array_equal(ref["counts"], [4, 4])                        # S_in = 0 = S_ip: every anchor violates
    assert not A.open_pairs(x, 2, 2, 4, 0.0).any()                      # every d and u is an fp32 number: nothing is open


def test_fast_ap_drops_what_falls_outside_the_bins():
    """Rows of norm 1.5: the twin at S = 2.25 has d = -2.5 (u = -6.25 at L = 10: no bin), the opposite row d = 6.5 (u = 16.25)."""
    x = np.array([[1.5, 0], [1.5, 0], [-1.5, 0], [0, 1.5]], np.float32)
    ref = A.reference(x, 2, 2, "fast_ap", bins=10)
    assert ref["hp"][0].sum() == 0 and ref["hn"][0].sum() == 1          # only (0, 1.5) at d = 2 is counted
    assert ref["ell"][0] == 1.0 and not ref["G"][0].any() and np.isfinite(ref["G"]).all()


def test_smooth_ap_by_hand():
    """K = 2: one positive.  R = 1, Q = 1 + sum_n sigma((S_in - S_ip) / tau), l = 1 - 1 / Q."""
    x = R.clustered_embeddings(3, 3, 2, 4, A.SIGMA)
    ref = A.reference(x, 3, 2, "smooth_ap", temperature=0.1)
    s, tau = ref["S"], A.tau32(0.1)
    neg = M.class_masks(3, 2)[1]
    for i in range(6):
        q = 1.0 + sum(1.0 / (1.0 + np.exp(-(s[i, j] - s[i, i ^ 1]) / tau)) for j in np.nonzero(neg[i])[0])
        assert abs(ref["ell"][i] - (1.0 - 1.0 / q)) < 1e-14


def test_twins_meet_at_one_half():
    x, _ = A.make_input("duplicates", *A.DUPLICATE_SHAPE)
    p, k, _ = A.DUPLICATE_SHAPE
    ref = A.reference(x, p, k, "smooth_ap", temperature=0.01)
    assert np.isfinite(ref["G"]).all() and ref["counts"][1] > 0
    fa = A.reference(x, p, k, "fast_ap", bins=10)
    assert (fa["l0"][0, 1] in (-1, 0)) and np.isfinite(fa["G"]).all()       # d ~ 0: bin 0


# ---------------------------------------------------------------------------------------------------------------- 3. float32 emulation
F = np.float32


def _wave_sum32(v):
    """[..., M] float32 -> the lane-strided chain (64 lanes, column order) and then the six butterfly steps."""
    m = v.shape[-1]
    lanes = np.zeros(v.shape[:-1] + (64,), F)
    for c in range(0, m, 64):
        part = v[..., c:c + 64]
        lanes[..., :part.shape[-1]] = lanes[..., :part.shape[-1]] + part
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., np.arange(64) ^ o]
    return lanes[..., 0]


def _emulate_fast_ap(s, p, k, bins):
    """csrc/ap_loss.hip's FastAP body in float32 NumPy, from a float32 S."""
    n, nb = p * k, bins + 1
    pos, neg = M.class_masks(p, k)
    inv = F(bins / 4.0)
    u = (F(2) - F(2) * s) * inv
    l0 = np.floor(u)
    f = u - l0
    g = F(1) - f
    lbin = np.arange(nb, dtype=F)
    hp, hn = np.zeros((n, nb), F), np.zeros((n, nb), F)
    for j in range(n):                                                   # the chain in column order
        w = np.where(l0[:, j, None] == lbin, g[:, j, None], np.where(l0[:, j, None] + F(1) == lbin, f[:, j, None], F(0))).astype(F)
        hp += np.where(pos[:, j, None], w, F(0))
        hn += np.where(neg[:, j, None], w, F(0))
    cp, cn = np.cumsum(hp, 1, dtype=F), np.cumsum(hn, 1, dtype=F)
    h = cp + cn
    ok = h > 0
    hs = np.where(ok, h, F(1))
    a, rp, rn = (np.where(ok, v / hs, F(0)).astype(F) for v in (hp, cp, cn))
    b, c, ft = a * rp, a * rn, hp * rp
    sb = np.cumsum(b[:, ::-1], 1, dtype=F)[:, ::-1]
    sc = np.cumsum(c[:, ::-1], 1, dtype=F)[:, ::-1]
    a_neg, a_pos = -sb, rp + sc
    ftp = np.pad(ft, ((0, 0), (0, 128 - nb)))                            # lane l holds the bins l and l + 64
    big_f = _wave_sum32(ftp[:, :64] + ftp[:, 64:])
    kf = F(k - 1)
    coef = F(2) * inv / kf
    i0 = np.clip(l0, -2, 66).astype(np.int64)
    look = lambda t, idx: A._pad_lookup(t.astype(np.float64), idx).astype(F)
    v = np.where(pos, look(a_pos, i0 + 1) - look(a_pos, i0), look(a_neg, i0 + 1) - look(a_neg, i0)).astype(F)
    gm = np.where(pos | neg, coef * v, F(0)).astype(F)
    return dict(hp=hp, hn=hn, G=gm, ell=(F(1) - big_f / kf).astype(F))


def _emulate_smooth_ap(s, p, k, tau):
    """csrc/ap_loss.hip's Smooth-AP body in float32 NumPy, from a float32 S."""
    n = p * k
    pos, neg = M.class_masks(p, k)
    r = F(1) / F(tau)
    kf = F(k - 1)
    rows = np.arange(n)

    def sigmoid(jp):
        z = (s - s[rows, jp][:, None]) * r
        t = np.exp(-np.abs(z)).astype(F)
        iv = F(1) / (F(1) + t)
        w = t * iv
        return np.where(z >= 0, iv, w).astype(F), ((r * w) * iv).astype(F)

    acc = np.zeros((n, n), F)
    ap = np.zeros((n, 64), F)
    stats = []
    for lane, (m, valid, jp) in enumerate(A._members(p, k)):
        sg, dsg = sigmoid(jp)
        keep = np.ones((n, n), bool)
        keep[rows, jp] = False
        kp = pos & keep
        big_r = F(1) + _wave_sum32(np.where(kp, sg, F(0)))
        nn, uu, tn = (_wave_sum32(np.where(msk, v, F(0))) for msk, v in ((neg, sg), (kp, dsg), (neg, dsg)))
        iq = F(1) / (big_r + nn)
        rq = big_r * iq
        stats.append((valid, jp, dsg, rq * iq, -((nn * iq) * iq), ((uu * nn - big_r * tn) * iq) * iq))
        ap[:, m % 64] += np.where(valid, rq, F(0))                       # (K <= 64 here: one member per lane)
    for valid, jp, dsg, wneg, wpos, own in stats:                       # the chain over the positives, in member order
        w = np.where(pos, wpos[:, None], wneg[:, None]).astype(F)
        term = (dsg.astype(np.float64) * w.astype(np.float64) + acc.astype(np.float64)).astype(F)      # fma: one rounding
        use = valid[:, None] & (pos | neg)
        use[rows, jp] = False
        acc = np.where(use, term, acc)
    for valid, jp, dsg, wneg, wpos, own in stats:
        acc[rows[valid], jp[valid]] = acc[rows[valid], jp[valid]] + own[valid]
    return dict(G=np.where(pos | neg, acc / kf, F(0)).astype(F), ell=(F(1) - _wave_sum32(ap) / kf).astype(F))


EMULATION_SHAPES = [(2, 2, 5), (5, 7, 33), (3, 16, 40), (8, 4, 64)]


def _s32(x):
    """A float32 S as some device might sum it, and its gamma_S: any order of E products and E - 1 additions."""
    return (x.astype(F) @ x.astype(F).T).astype(F), float(M.gamma(x.shape[1] + 1))


@pytest.mark.parametrize("kind", ["continuous", "grid", "negated", "scaled", "antipodal"])
@pytest.mark.parametrize("bins", [2, 7, 10, 16, 64])
@pytest.mark.parametrize("p,k,e", EMULATION_SHAPES, ids=str)
def test_float32_emulation_of_fast_ap_is_inside_the_bounds(p, k, e, bins, kind):
    x, _ = A.make_input(kind, p, k, e)
    s, gs = _s32(x)
    ref = A.reference(x, p, k, "fast_ap", bins=bins)
    bg, bell, _, extra = A.bounds(x, ref, gs)
    emu = _emulate_fast_ap(s, p, k, bins)
    keep = _off(p * k) & ~A.open_pairs(x, p, k, bins, gs)
    assert np.isfinite(emu["G"]).all()
    ratios = dict(G=(np.abs(emu["G"] - ref["G"])[keep] / bg[keep]).max() if keep.any() else 0.0,
                  ell=(np.abs(emu["ell"] - ref["ell"]) / bell).max(),
                  hp=(np.abs(emu["hp"] - ref["hp"]) / np.maximum(extra["Eh_pos"], 1e-300)).max(),
                  hn=(np.abs(emu["hn"] - ref["hn"]) / np.maximum(extra["Eh_neg"], 1e-300)).max())
    print(f"fast_ap emulation {kind} L={bins} p={p} k={k} e={e}: " + " ".join(f"{a}={b:.3g}" for a, b in ratios.items()))
    assert all(v < 1 for v in ratios.values()), ratios


@pytest.mark.parametrize("kind", ["continuous", "grid"])
@pytest.mark.parametrize("tau", [0.01, 0.1, 10.0])
@pytest.mark.parametrize("p,k,e", EMULATION_SHAPES, ids=str)
def test_float32_emulation_of_smooth_ap_is_inside_the_bounds(p, k, e, tau, kind):
    x, _ = A.make_input(kind, p, k, e)
    s, gs = _s32(x)
    ref = A.reference(x, p, k, "smooth_ap", temperature=tau)
    bg, bell, _, _ = A.bounds(x, ref, gs)
    emu = _emulate_smooth_ap(s, p, k, A.tau32(tau))
    off = _off(p * k)
    ratios = dict(G=(np.abs(emu["G"] - ref["G"])[off] / bg[off]).max(), ell=(np.abs(emu["ell"] - ref["ell"]) / bell).max(),
                  rowsum=(np.abs(emu["G"].astype(np.float64).sum(1)) / bg.sum(1)).max())
    print(f"smooth_ap emulation {kind} tau={tau} p={p} k={k} e={e}: " + " ".join(f"{a}={b:.3g}" for a, b in ratios.items()))
    assert np.isfinite(emu["G"]).all() and all(v < 1 for v in ratios.values()), ratios


# ---------------------------------------------------------------------------------------------------------------- 4. the GPU test's inputs
@pytest.mark.parametrize("kind,shape,bins", A.fast_ap_cases(), ids=str)
def test_open_pair_cap_holds_for_the_gpu_tests_inputs(kind, shape, bins):
    p, k, e = shape
    x, unit = A.make_input(kind, p, k, e)
    n = p * k
    if unit is not None:
        assert M.exact_in_any_order(x, unit)                            # gamma_S = 0 is claimed for these
    gammas = [0.0] if unit is not None else [M.gamma_s("similarity_matrix" if path == "auto" and M.auto_path(p, k, e) != "per_class"
                                                        else ("per_class" if path == "auto" else path), e) for path in A.paths_of(p, k, e)]
    for gs in gammas:
        share = A.open_pairs(x, p, k, bins, gs).sum() / (n * (n - 1))
        print(f"{kind} {shape} L={bins} gamma_S={gs:.3g}: open share {share:.3g}")
        assert share <= A.OPEN_CAP
    if kind == "grid":
        assert not A.open_pairs(x, p, k, bins, 0.0).any()               # S, d and u are exact: the device's intervals are the reference's
    if kind == "negated":
        assert (2.0 - 2.0 * A.reference(x, p, k, "fast_ap", bins=bins)["S"]).max() > 3.2                  # bins 8 and above of 10
    if kind == "antipodal":
        assert (A.reference(x, p, k, "fast_ap", bins=bins)["hn"][:, 64] > 0.1).any()
    if kind == "scaled":
        ref = A.reference(x, p, k, "fast_ap", bins=bins)
        d = 2.0 - 2.0 * ref["S"][_off(n)]
        assert d.min() < 0 and d.max() > 4 and 0 < ref["hp"].sum() < n * (k - 1) and 0.01 < ref["loss"] < 0.99


def test_case_table_covers_every_bin_count_and_path():
    cases = A.fast_ap_cases()
    assert {b for _, _, b in cases} == {2, 7, 10, 16, 64}
    assert all(b == 10 for kind, _, b in cases if kind in ("grid", "duplicates"))
    assert {(4, 32, 64), (64, 4, 512), (256, 8, 128), (2, 2, 5), (3, 16, 40)} <= {s for _, s, _ in cases}
    assert A.paths_of(8, 4, 256) == ["per_class", "similarity_matrix"] and A.paths_of(4, 32, 64) == ["similarity_matrix"]
    assert A.paths_of(64, 4, 512) == ["auto"]


# ---------------------------------------------------------------------------------------------------------------- 5. CLI validator, exports
def _train():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train
    finally:
        sys.path.pop(0)
    return train


def _cfg(mode, value, model_mode="triplet"):
    return {"generator": {"negatives_selection_mode": mode, "ap_loss": value}, "model": {"mode": model_mode}}


def test_ap_loss_validator():
    train = _train()
    assert train.ap_loss_config(_cfg("fast_ap", {"bins": 10})) == {"bins": 10}
    assert isinstance(train.ap_loss_config(_cfg("fast_ap", {"bins": 16.0}))["bins"], int)
    assert train.ap_loss_config(_cfg("fast_ap", {})) == {}
    assert train.ap_loss_config(_cfg("smooth_ap", {"temperature": 0.05})) == {"temperature": 0.05}
    assert train.ap_loss_config({"generator": {"negatives_selection_mode": "fast_ap"}, "model": {"mode": "triplet"}}) is None
    for mode, value in [("fast_ap", {"bins": 1}), ("fast_ap", {"bins": 65}), ("fast_ap", {"bins": 2.5}), ("fast_ap", {"bins": True}),
                        ("fast_ap", {"bins": "10"}), ("fast_ap", {"temperature": 0.1}), ("smooth_ap", {"bins": 10}),
                        ("smooth_ap", {"temperature": 0}), ("smooth_ap", {"temperature": -1.0}), ("smooth_ap", {"temperature": "x"}),
                        ("fast_ap", [10]), ("semihard", {"bins": 10}), ("supcon", {"temperature": 0.1})]:
        with pytest.raises(ValueError, match="GENERATOR.ap_loss"):
            train.ap_loss_config(_cfg(mode, value))
    with pytest.raises(ValueError, match="GENERATOR.ap_loss"):
        train.ap_loss_config(_cfg("fast_ap", {"bins": 10}, model_mode="siamese"))
    assert {"fast_ap", "smooth_ap"} <= set(train.XBM_MODES)


def test_exports_and_abi():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in ("fast_ap", "smooth_ap"):
        for suffix in ("loss_fwd", "loss_path", "loss_workspace_bytes"):
            assert f"embnet_{name}_{suffix}" in protos
    assert len(protos["embnet_fast_ap_loss_fwd"][1]) == 12 and len(protos["embnet_smooth_ap_loss_fwd"][1]) == 12
    header = open(_lib.HEADER_PATH).read()
    assert "EMBNET_AP_PER_CLASS = 1, EMBNET_AP_SIMILARITY_MATRIX = 2" in header and "#define EMBNET_ABI_VERSION 22" in header
    source = open(os.path.join(ROOT, "embeddingnet_amd", "csrc", "ap_loss.hip")).read()
    for kernel in ("fast_ap_class_fwd_kernel", "fast_ap_sweep_kernel", "smooth_ap_class_fwd_kernel", "smooth_ap_sweep_kernel"):
        assert f'"embnet::{kernel}"' in source


def test_python_layers_know_the_modes():
    from embeddingnet_amd import losses_and_accuracies as LA
    from embeddingnet_amd import ops
    from embeddingnet_amd.train_step import TripletTrainer
    assert ops.PAIR_LOSS_MODES["fast_ap"] == (ops.fast_ap_loss, ("bins",), 1)
    assert ops.PAIR_LOSS_MODES["smooth_ap"] == (ops.smooth_ap_loss, ("temperature",), 1)
    assert ops.AP_PATHS == {"auto": 0, "per_class": 1, "similarity_matrix": 2}
    assert ops._PAIR_LOSSES["fast_ap_loss"][5:] == ("embnet_ms_loss_bwd", False)
    assert ops._PAIR_LOSSES["smooth_ap_loss"][5:] == ("embnet_ms_loss_bwd", False)
    assert TripletTrainer.LOSS_PARAMS["fast_ap"] == ("bins",) and TripletTrainer.LOSS_PARAMS["smooth_ap"] == ("temperature",)
    assert callable(LA.fast_ap_loss(8, 4, 10)) and callable(LA.smooth_ap_loss(8, 4, 0.01))
