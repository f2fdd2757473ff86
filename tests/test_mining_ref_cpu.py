"""tests/mining_ref.py on the CPU: the restatement against oracle/mining.py, the uniformity of its pick, the CONDITIONS on the inputs
that tests/test_loss_path_exact_gpu.py runs on (so that no GPU test passes vacuously), and three restatements made wrong on purpose,
each of which must fail the exact comparison on the `planted` and the lattice families."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mining_ref as M  # noqa: E402
import recipes as R  # noqa: E402
from oracle import mining as omining  # noqa: E402

MARGIN = 0.5
LATTICE_CASES = M.LATTICE_CASES
OFF_LATTICE_CASES = M.OFF_LATTICE_CASES
off_lattice_rows = M.off_lattice_rows


def lattice_D(p, k, e):
    rows, _ = M.lattice(M.MINING_SEED, p, k, e)
    return rows, M.lattice_dist(rows)


# ---- against the oracle ------------------------------------------------------------------------------------------------------------
def check_against_oracle(D, p, k):
    for mode in M.MODES:
        o = omining.mine_triplets(D, p, k, MARGIN, mode, rng=np.random.RandomState(0))
        r = M.mine(D, p, k, MARGIN, mode, seed=3)
        assert np.array_equal(r["loss_values"], o["loss_values"])
        assert np.array_equal(r["candidates"], o["candidates"])
        assert r["fallback"] == o["fallback"]
        if mode == "hardest" or o["fallback"]:
            assert np.array_equal(r["triplets"], o["triplets"])
        else:
            assert np.array_equal(r["triplets"][:, :2], o["triplets"][:, :2])       # same active pairs in the same order


@pytest.mark.parametrize("case", R.MINING_CASES, ids=lambda c: c[0])
def test_mine_equals_oracle_on_golden(golden, case):
    name, p, k = case[0], case[1], case[2]
    check_against_oracle(golden("mining")[f"{name}/D"], p, k)


@pytest.mark.parametrize("family", M.FINITE_FAMILIES)
@pytest.mark.parametrize("p,k", [(3, 3), (13, 5), (9, 8), (66, 4)])
def test_mine_equals_oracle_on_families(family, p, k):
    check_against_oracle(M.distance_family(family, 5, p, k), p, k)


def test_batch_hard_equals_oracle_on_finite_and_is_in_range_on_nonfinite():
    for family in M.FINITE_FAMILIES:
        D = M.distance_family(family, 5, 13, 5)
        assert np.array_equal(M.batch_hard(D, 13, 5), omining.batch_hard(D, 13, 5))
    for p, k in [(2, 2), (13, 5), (66, 4)]:
        D = M.nonfinite(5, p, k)
        t = M.batch_hard(D, p, k)
        n = p * k
        assert t.min() >= 0 and t.max() < n
        assert np.all(t[:, 1] // k == t[:, 0] // k) and np.all(t[:, 1] != t[:, 0]) and np.all(t[:, 2] // k != t[:, 0] // k)
        nanrow = np.isnan(D).all(1)
        assert nanrow.any()
        a = np.where(nanrow)[0]
        lo = (a // k) * k
        assert np.array_equal(t[a, 1], np.where(a == lo, lo + 1, lo)) and np.array_equal(t[a, 2], np.where(lo > 0, 0, k))


def test_pack_mask_layout():
    cand = np.zeros((2, 70), bool)
    cand[0, [0, 31, 32, 69]] = True
    cand[1, 33] = True
    assert np.array_equal(M.pack_mask(cand), np.array([[0x80000001, 1, 1 << 5], [0, 2, 0]], np.uint32))


# ---- uniformity of the pick: a property of the RNG, shown here once -------------------------------------------------------------------
def test_pick_is_uniform_over_seeds():
    from scipy.stats import chi2
    p, k = 4, 2
    D = M.none_qualifies(p, k)
    cols = [2, 3, 5, 6, 7]                                                          # five candidates of pair 0 (rows 0, 1)
    D[0, cols] = 1.25
    seeds = 3000
    counts = dict.fromkeys(cols, 0)
    lv = M.loss_values(D, p, k, MARGIN)
    for seed in range(seeds):
        r = M.mine(D, p, k, MARGIN, "semihard", seed, lv=lv)
        assert r["candidates"][0].sum() == 5
        counts[int(r["selected"][0])] += 1
    exp = seeds / 5
    stat = sum((c - exp) ** 2 / exp for c in counts.values())
    assert stat < chi2.ppf(0.999, 4), (stat, counts)


# ---- conditions on the lattice inputs ---------------------------------------------------------------------------------------------------
# the issue's five cases, and every lattice matrix of the GPU mining tests that has pairs enough for a share to mean something
# ((2, 2) and (3, 3) have 2 and 9 pairs: their job is the smallest grid, not the statistics)
MINED_LATTICES = [(p, k, M.MINING_E) for p, k in M.MINING_SHAPES if p * k * (k - 1) // 2 >= 100 and (p, k, M.MINING_E) not in LATTICE_CASES]


@pytest.mark.parametrize("p,k,e", LATTICE_CASES + MINED_LATTICES)
def test_lattice_inputs_exercise_every_decision(p, k, e):
    rows, D = lattice_D(p, k, e)
    assert np.array_equal(D, M.distance_family("lattice", M.MINING_SEED, p, k, e))
    assert M.lattice_units_max(rows) < 2 ** 24
    assert np.isfinite(D).all()
    lv = M.loss_values(D, p, k, MARGIN)
    assert (lv == 0).any() and (lv == np.float32(MARGIN)).any()
    sets = {m: M.candidate_sets(lv, MARGIN, m) for m in M.MODES}
    pairs = len(lv)
    for m in M.MODES:
        active = sets[m].any(1).mean()
        assert active >= 0.15 and 1 - active >= 0.10, (m, active)
    for m in ("semihard", "random_hard"):
        assert (sets[m].sum(1) >= 2).mean() >= 0.20, m
    tied = ((lv == lv.max(1, keepdims=True)).sum(1) >= 2).mean()
    assert tied >= 0.05, tied
    assert (sets["semihard"] != sets["random_hard"]).any(1).mean() >= 0.10
    assert pairs == p * k * (k - 1) // 2


@pytest.mark.parametrize("p,k,e", LATTICE_CASES[:3])
def test_gather_loss_forms_agree_exactly_on_lattice(p, k, e):
    rows, D = lattice_D(p, k, e)
    x = (rows * M.STEP).astype(np.float32)
    for mode in M.MODES:
        r = M.mine(D, p, k, MARGIN, mode, seed=1234)
        for up in (None, 0.37):
            a = M.gather_loss(x, r["triplets"], r["count"], MARGIN, up, np.float32)
            b = M.gather_loss(x, r["triplets"], r["count"], MARGIN, up, np.float64)
            for key in ("rows", "active", "acc", "sq"):                             # every sum is exact in both formats
                assert np.array_equal(a[key].astype(np.float64), b[key]), key
            # the two scalings round once each in float32 (sum / count, g = 2 up / count, g * sum): redo them from the float64 sums
            assert a["mean"] == np.float32(b["rows"].sum()) / np.float32(r["count"])
            assert np.array_equal(a["demb"], (np.float64(a["g"]) * b["acc"]).astype(np.float32))
            assert abs(float(a["g"]) - float(b["g"])) <= 2.0 ** -23 * float(b["g"])


# ---- the off-lattice families: few pairs are left undecided ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OFF_LATTICE_CASES, ids=lambda c: "%s-%dx%dx%d" % c)
def test_off_lattice_undecided_share(case):
    family, p, k, e = case
    x = off_lattice_rows(family, p, k, e)
    if family == "spread":
        nn = np.linalg.norm(x.astype(np.float64), axis=1)
        assert nn.max() / nn.min() >= 2 ** 10 * 0.99
    for mode in M.MODES:
        d = M.decisions(x, p, k, MARGIN, mode, seed=1234)
        share = 1 - d["decided"].mean()
        assert share <= 0.02, (mode, share)
        assert d["decided"].any() and (d["selected"][d["decided"]] >= 0).any()


# ---- restatements made wrong on purpose must fail the exact comparisons ----------------------------------------------------------------------
def first_of_block_pick(cand, want):
    """WRONG: the first candidate of the right 64-column ballot block instead of the want-th candidate."""
    q = M.ranked_pick(cand, want)
    block = (np.arange(cand.shape[1])[None, :] // 64) == (np.maximum(q, 0)[:, None] // 64)
    return np.where(q < 0, -1, np.argmax(cand & block, axis=1))


def mine_margin_le(D, p, k, margin, mode, seed):
    """WRONG: `<=` in place of `<` at the margin."""
    lv = M.loss_values(D, p, k, margin)
    lv = np.where(lv == np.float32(margin), np.nextafter(np.float32(margin), np.float32(0)), lv).astype(np.float32)
    return M.mine(D, p, k, margin, mode, seed, lv=lv)


def mine_last_argmax(D, p, k, margin, mode, seed):
    """WRONG: the last arg-max on ties."""
    lv = M.loss_values(D, p, k, margin)
    r = M.mine(D[:, ::-1], p, k, margin, mode, seed, lv=lv[:, ::-1])
    nneg = lv.shape[1]
    _, _, lo = M.pair_index(p, k)
    q = np.where(r["candidates"].any(1), nneg - 1 - np.argmax(r["candidates"], axis=1), -1)
    return dict(selected=np.where(q < 0, -1, np.where(q < lo, q, q + k)).astype(np.int32))


WRONGINGS = [
    ("first_of_block", ("semihard", "random_hard"), lambda D, p, k, mode, seed: M.mine(D, p, k, MARGIN, mode, seed, pick=first_of_block_pick)),
    ("margin_le", ("semihard",), lambda D, p, k, mode, seed: mine_margin_le(D, p, k, MARGIN, mode, seed)),
    ("last_argmax", ("hardest",), lambda D, p, k, mode, seed: mine_last_argmax(D, p, k, MARGIN, mode, seed)),
]


@pytest.mark.parametrize("wrong", WRONGINGS, ids=lambda w: w[0])
@pytest.mark.parametrize("family", ["planted", "lattice"])
def test_wrong_restatements_fail_the_exact_comparison(family, wrong):
    name, modes, fn = wrong
    p, k = 66, 4
    D = M.distance_family(family, 7, p, k)
    for mode in modes:
        differs = False
        for seed in (0, 1234, 2 ** 63 + 5):
            true = M.mine(D, p, k, MARGIN, mode, seed)
            differs |= not np.array_equal(fn(D, p, k, mode, seed)["selected"], true["selected"])
        assert differs, (name, family, mode)


def test_fused_lattice_inputs_are_exact_and_mixed():
    """The shapes of the fused-kernel test: the exactness premise, and pairs of both kinds wherever a sibling class exists."""
    for p, k, e in [(2, 2, 1), (3, 3, 63), (8, 4, 65), (7, 5, 300), (32, 16, 48), (256, 2, 32), (32, 4, 600), (128, 4, 3584), (32, 16, 512)]:
        rows = M.fused_lattice(p, k, e)
        assert M.lattice_units_max(rows) < 2 ** 24
        lv = M.loss_values(M.lattice_dist(rows), p, k, MARGIN)
        for mode in M.MODES:
            active = M.candidate_sets(lv, MARGIN, mode).any(1).mean()
            if p >= 4:
                assert 0.15 <= active <= 0.9, (p, k, e, mode, active)
            elif p == 3:
                assert active == 0                                                  # three isolated classes: the fallback triplet
