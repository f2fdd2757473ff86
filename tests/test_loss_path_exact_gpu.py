"""The loss path (csrc/pairwise.hip, mining.hip, losses.hip, fused_loss.hip) through the C ABI against tests/mining_ref.py:
all-pairs distances, online triplet mining with its random pick, batch-hard, the gather-form and the concat-form hinge with their
backward, and the one-launch fused kernel.

EXACT assertions (array_equal, no tolerance), on lattice inputs (every embedding entry a small integer over 8: every sum any kernel
forms is exactly representable in fp32 in any order) and on given distance matrices:
  * mining on a given D: selected, candidate mask words, triplets and count equal mining_ref.mine for the three rules, three seeds,
    six matrix families, thirteen shapes on both routes (per pair, per anchor <1> <3> <7>); embnet_batch_hard equals
    mining_ref.batch_hard on the same matrices, the non-finite family included, every index in [0, n);
  * pairwise: d^2 equals the integer d^2 bit for bit on every route of the plan (64 and 128 tiles, K-split slabs + finish, scalar
    and vector loader, scalar and vector epilogue, unaligned x); d equals sqrt of the kernel's own d^2 through the device's sqrtf;
  * fused kernel, launched twice: selected / triplets / count / loss rows / active / mean are the bits of pairwise + mining (or
    batch-hard) + gather forward on the same rows and seed, and the bits of the restatement; four modes, seed and seed_dev, nine
    shapes up to both LDS limits; embnet_fused_loss_supported is 0 one step beyond each limit;
  * gather forward / backward and the concat-form hinge equal the float32 restatement: E in {1 .. 4100} (the blockIdx.y walk past
    4096), live counts {1, 255, 256, 257, 700}, a hub row that is the negative of every triplet, rows with pos - neg + margin == 0
    exactly (loss 0, active 1, gradient passes), upstream 0.37 and NULL.
Every output sits between sentinel margins that must stay untouched; triplets rows at and beyond count keep the sentinel, loss and
active there are 0; the kernel that ran is read from the launch trace.

BOUNDED assertions, on off-lattice rows (unit-norm clustered rows; unnormalised rows whose norms spread over 2^10), u = 2^-24,
gamma(n) = n u / (1 - n u), nothing tuned against the kernels:
  * pairwise per element   |d2 - d2_f64| <= gamma(e + 3) (|x|^2 + |y|^2 + 2 sum |x_i y_i|)
  * gather forward per row |loss - loss_f64| <= gamma(e + 2) (pos + neg + margin)
  * mean                   |mean - mean_f64 of the kernel's rows| <= gamma(T + 1) sum loss / T
  * backward per element   |demb - demb_f64| <= gamma(2 m_r + 4) |g| sum |terms of the m_r matches|
  * decisions per pair     a pair whose float64 decision (activity, arg-max, candidate-set membership of every column) holds by more
                           than the summed distance bounds must be decided as the restatement decides, with the want-th pick; only
                           the other pairs are excused, each on its own margin (their share is capped at 2 % per case by
                           tests/test_mining_ref_cpu.py).

Measured on an MI355X: the largest error / bound per kernel and family, and the largest undecided share:

  kernel                    unit rows   spread rows
  pairwise d^2 / element       0.062        0.091
  gather forward / row         0.032        0.065
  mean                         0.031        0.056
  gather backward / element    0.385        0.359
  undecided pairs, fused       1.50 %       0.83 %      (largest case: (5, 16, 40); 0 in the other six)
  undecided pairs, separate    1.50 %       0.83 %
  Every exact assertion held bit for bit, the device's sqrtf and the divisions by count included; no decided pair was decided
  otherwise by either path.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mining_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 0.5
GUARD = 64                                                # elements of sentinel on each side of every output (256 bytes)
SENT = -77777                                             # int sentinel; float outputs use NaN
NAN = float("nan")
SEEDS = (0, 1234, 2 ** 63 + 5)
RATIOS = {}                                               # (kernel, family) -> largest error / bound seen
UNDECIDED = {}                                            # (path, family) -> largest undecided share seen


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    yield torch.device("cuda", 0)
    for (kernel, family), r in sorted(RATIOS.items()):
        print("LOSSPATH RATIO  %-22s %-7s %.3f" % (kernel, family, r))
    for (path, family), s in sorted(UNDECIDED.items()):
        print("LOSSPATH UNDECIDED  %-10s %-7s %.4f" % (path, family, s))


def note_ratio(kernel, family, err, bound):
    """err <= bound everywhere (exactly 0 where the bound is 0); records the largest ratio."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert np.all(err[bound == 0] == 0), kernel
    r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    RATIOS[(kernel, family)] = max(RATIOS.get((kernel, family), 0.0), r)
    print("ratio %s %s %.3f" % (kernel, family, r))
    assert r < 1, (kernel, family, r)


# ---- buffers -------------------------------------------------------------------------------------------------------------------------
class Out:
    """An output of n elements between two sentinel margins."""

    def __init__(self, n, dev, dtype):
        self.n, self.fill = n, (NAN if dtype == torch.float32 else SENT)
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=dev)
        self.view = self.buf[GUARD:GUARD + n]
        assert self.view.data_ptr() % 16 == 0

    def ptr(self):
        return self.view.data_ptr()

    def get(self, what):
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        edge = np.concatenate([host[:GUARD], host[GUARD + self.n:]])
        assert (np.isnan(edge).all() if self.fill != SENT else (edge == SENT).all()), "%s wrote outside its output" % what
        return host[GUARD:GUARD + self.n].copy()


def fout(n, dev):
    return Out(n, dev, torch.float32)


def iout(n, dev):
    return Out(n, dev, torch.int32)


def place(a, dev, shift=0):
    """float32 array on the device; shift: floats by which its first element is off a 16-byte boundary."""
    a = np.array(a, dtype=np.float32, order="C")             # a copy: the cached inputs are read-only
    buf = torch.full((a.size + 8 + shift,), NAN, device=dev)
    view = buf[4 + shift:4 + shift + a.size]
    view.copy_(torch.from_numpy(a.reshape(-1)))
    assert view.data_ptr() % 16 == 4 * shift
    return view


def traced(call):
    _lib.trace_reset(); _lib.trace_enable(True)
    try:
        call()
        torch.cuda.synchronize()
        return [r[0].replace("embnet::", "") for r in _lib.trace_records()]
    finally:
        _lib.trace_enable(False)


def check_live_rows(trip, count, what):
    """triplets [max_t, 3] as written: rows >= count keep the sentinel."""
    assert (trip[count:] == SENT).all(), "%s wrote triplet rows beyond count" % what
    return trip[:count]


# ---- entry points ---------------------------------------------------------------------------------------------------------------------
def run_pairwise(dev, x, squared, shift=0):
    """-> (matrix [n, n] on the device (inside its guarded buffer, checked), kernel names)."""
    lib = _lib.lib()
    n, e = x.shape
    xd = place(x, dev, shift)
    out = fout(n * n, dev)
    nws = lib.embnet_pairwise_workspace_bytes(n, e)
    ws = torch.full((nws // 4 + 4,), NAN, device=dev)
    names = traced(lambda: _lib.check(lib.embnet_pairwise_dist_f32(xd.data_ptr(), n, e, out.ptr(), int(squared), ws.data_ptr(), nws,
                                                                  _lib.stream())))
    assert "pairwise_kernel" in names, names
    out.get("pairwise")
    return out.view.reshape(n, n), names


def mining_route(p, k, mode):
    n = p * k
    if int(os.environ.get("EMBNET_MINE_BY_ANCHOR", "1")) and k - 1 <= 7 and n >= 1024:
        return "mine_hardest_anchor_kernel" if mode == "hardest" else "mine_random_anchor_kernel"
    return "mine_select_kernel"


def run_mine(dev, Dd, p, k, mode, seed):
    """embnet_mine_triplets -> dict(selected, mask [pairs, words] uint32, triplets [count, 3], count)."""
    lib = _lib.lib()
    n, pairs = p * k, p * k * (k - 1) // 2
    words, max_t = (n - k + 31) // 32, lib.embnet_mine_max_triplets(p, k)
    trip, count, sel, mask = iout(3 * max_t, dev), iout(1, dev), iout(pairs, dev), iout(pairs * words, dev)
    names = traced(lambda: _lib.check(lib.embnet_mine_triplets(Dd.data_ptr(), p, k, MARGIN, M.MODE_ID[mode], seed, trip.ptr(),
                                                              count.ptr(), sel.ptr(), mask.ptr(), _lib.stream())))
    assert mining_route(p, k, mode) in names and "mine_compact_kernel" in names, names
    c = int(count.get("mine count")[0])
    assert 1 <= c <= max_t
    return dict(selected=sel.get("mine selected"), mask=mask.get("mine mask").view(np.uint32).reshape(pairs, words),
                triplets=check_live_rows(trip.get("mine triplets").reshape(max_t, 3), c, "mine"), count=c,
                dev=(trip, count, max_t))


def run_batch_hard(dev, Dd, p, k):
    lib = _lib.lib()
    n = p * k
    trip, count = iout(3 * n, dev), iout(1, dev)
    names = traced(lambda: _lib.check(lib.embnet_batch_hard(Dd.data_ptr(), p, k, trip.ptr(), count.ptr(), _lib.stream())))
    assert names == ["batch_hard_kernel"], names
    assert int(count.get("batch_hard count")[0]) == n
    return dict(triplets=trip.get("batch_hard").reshape(n, 3), count=n, dev=(trip, count, n))


def run_gather_fwd(dev, xd, n, e, trip_ptr, count_ptr, max_t):
    lib = _lib.lib()
    loss, act, mean = fout(max_t, dev), fout(max_t, dev), fout(1, dev)
    names = traced(lambda: _lib.check(lib.embnet_triplet_gather_fwd(xd.data_ptr(), n, e, trip_ptr, count_ptr, max_t, MARGIN, loss.ptr(),
                                                                   act.ptr(), mean.ptr(), _lib.stream())))
    assert names == ["triplet_gather_fwd_kernel", "mean_first_kernel"], names
    return loss.get("gather_fwd loss"), act.get("gather_fwd active"), mean.get("gather_fwd mean")[0], act


def run_gather_bwd(dev, xd, n, e, trip_ptr, count_ptr, max_t, act_out, upstream):
    lib = _lib.lib()
    demb = fout(n * e, dev)
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=dev)
    names = traced(lambda: _lib.check(lib.embnet_triplet_gather_bwd(xd.data_ptr(), n, e, trip_ptr, count_ptr, max_t, act_out.ptr(),
                                                                   up.data_ptr() if up is not None else None, demb.ptr(),
                                                                   _lib.stream())))
    assert names == ["triplet_gather_bwd_kernel"], names
    return demb.get("gather_bwd").reshape(n, e)


def run_fused(dev, xd, p, k, e, mode, seed, seed_dev=None, launches=2):
    """embnet_fused_triplet_loss_fwd, `launches` times on one workspace (zeroed once: every launch re-arms its ticket), each into
    fresh sentinel buffers -> the last launch's outputs."""
    lib = _lib.lib()
    n, pairs = p * k, p * k * (k - 1) // 2
    max_t = n if mode == "batch_hard" else lib.embnet_mine_max_triplets(p, k)
    assert lib.embnet_fused_loss_supported(p, k, e) == 1
    nws = lib.embnet_fused_loss_workspace_bytes(p, k)
    ws = torch.zeros((nws // 4,), dtype=torch.int32, device=dev)
    sd = None
    if seed_dev is not None:
        sd = torch.from_numpy(np.array([seed_dev], np.uint64).view(np.int64)).to(dev)
    res = []
    for _ in range(launches):
        trip, count, sel = iout(3 * max_t, dev), iout(1, dev), iout(pairs, dev)
        loss, act, mean = fout(max_t, dev), fout(max_t, dev), fout(1, dev)
        names = traced(lambda: _lib.check(lib.embnet_fused_triplet_loss_fwd(
            xd.data_ptr(), p, k, e, MARGIN, M.MODE_ID[mode], seed, sd.data_ptr() if sd is not None else None, trip.ptr(), count.ptr(),
            sel.ptr(), loss.ptr(), act.ptr(), mean.ptr(), ws.data_ptr(), nws, _lib.stream())))
        assert names == ["fused_triplet_loss_fwd_kernel"], names
        c = int(count.get("fused count")[0])
        assert 1 <= c <= max_t
        res.append(dict(selected=sel.get("fused selected"), count=c,
                        triplets=check_live_rows(trip.get("fused triplets").reshape(max_t, 3), c, "fused"),
                        loss=loss.get("fused loss"), active=act.get("fused active"), mean=mean.get("fused mean")[0]))
        assert int(ws[0].item()) == 0, "the arrival ticket was not re-armed"
    for key in res[0]:
        assert np.array_equal(res[0][key], res[-1][key]), "two launches differ in %s" % key
    return res[-1]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, "%s: %d elements differ, first at %d: %r != %r" % (what, bad.size, bad[0], got.reshape(-1)[bad[0]],
                                                                            want.reshape(-1)[bad[0]])


# ---- mining on a given D ------------------------------------------------------------------------------------------------------------------
MINING_SHAPES = M.MINING_SHAPES


@functools.lru_cache(maxsize=8)
def given_D(family, p, k):
    d = M.distance_family(family, M.MINING_SEED, p, k, M.MINING_E)
    d.setflags(write=False)
    return d


@pytest.mark.parametrize("p,k", MINING_SHAPES, ids=lambda v: str(v))
def test_mining_on_a_given_matrix_is_the_restatement(dev, p, k):
    for family in M.FAMILIES:
        D = given_D(family, p, k)
        Dd = place(D, dev)
        lv = M.loss_values(D, p, k, MARGIN)
        for mode in M.MODES:
            for seed in (SEEDS if mode != "hardest" else SEEDS[1:2]):
                what = "%s %s seed %d" % (family, mode, seed)
                want = M.mine(D, p, k, MARGIN, mode, seed, lv=lv)
                got = run_mine(dev, Dd, p, k, mode, seed)
                assert np.array_equal(got["mask"], M.pack_mask(want["candidates"])), what
                assert np.array_equal(got["selected"], want["selected"]), what
                assert got["count"] == want["count"] and np.array_equal(got["triplets"], want["triplets"]), what
                if family == "none":
                    assert want["fallback"] and np.array_equal(got["triplets"], [[p * k - 2, p * k - 1, 0]])
                if family == "all":
                    assert want["candidates"].all() or mode == "hardest"


@pytest.mark.parametrize("p,k", MINING_SHAPES, ids=lambda v: str(v))
def test_batch_hard_on_a_given_matrix_is_the_restatement(dev, p, k):
    """The non-finite family goes through embnet_batch_hard ALONE: it only writes indices.  No other entry point sees such rows."""
    n = p * k
    for family in M.FAMILIES:
        D = given_D(family, p, k)
        got = run_batch_hard(dev, place(D, dev), p, k)["triplets"]
        assert got.min() >= 0 and got.max() < n, family
        assert np.array_equal(got, M.batch_hard(D, p, k)), family


# ---- pairwise, lattice -------------------------------------------------------------------------------------------------------------------
def dense_rows(n, e, seed=3):
    rows, _ = M.lattice(seed, n, 1, e, dense=True, moved=max(2, e // 8))
    assert M.lattice_units_max(rows) < 2 ** 24
    return rows


# (n, e, shift of x off 16 bytes, kernels the trace must show besides pairwise_kernel)
PAIRWISE_CASES = [(1, 3, 0, ()), (7, 5, 0, ()), (64, 64, 0, ()), (64, 64, 1, ()), (65, 33, 0, ()), (130, 70, 0, ()), (130, 72, 3, ()),
                  (256, 4096, 0, ("pairwise_finish_kernel",)), (512, 256, 0, ()), (1024, 64, 0, ()), (2560, 24, 0, ()), (2562, 7, 0, ())]


@pytest.mark.parametrize("n,e,shift,also", PAIRWISE_CASES, ids=lambda v: str(v))
def test_pairwise_lattice_is_exact(dev, n, e, shift, also):
    rows = dense_rows(n, e)
    x = (rows * M.STEP).astype(np.float32)
    want = (M.lattice_sqdist(rows) * (M.STEP * M.STEP)).astype(np.float32)
    d2, names = run_pairwise(dev, x, True, shift)
    for kern in also:
        assert kern in names, names
    same_bits(d2.cpu().numpy(), want, "d^2")
    d, _ = run_pairwise(dev, x, False, shift)
    assert torch.equal(d.view(torch.int32), torch.sqrt(d2).view(torch.int32)), "d is not sqrtf of the kernel's d^2"


# ---- fused against separate, lattice --------------------------------------------------------------------------------------------------------
FUSED_SHAPES = [(2, 2, 1), (3, 3, 63), (8, 4, 65), (7, 5, 300), (32, 16, 48), (256, 2, 32), (32, 4, 600), (128, 4, 3584), (32, 16, 512)]


@pytest.mark.parametrize("p,k,e", FUSED_SHAPES, ids=lambda v: str(v))
def test_fused_equals_separate_kernels_and_the_restatement(dev, p, k, e):
    n = p * k
    rows = M.fused_lattice(p, k, e)
    x = (rows * M.STEP).astype(np.float32)
    xd = place(x, dev)
    Dd, _ = run_pairwise(dev, x, False)
    D = Dd.cpu().numpy()
    d2, _ = run_pairwise(dev, x, True)
    same_bits(d2.cpu().numpy(), (M.lattice_sqdist(rows) * (M.STEP * M.STEP)).astype(np.float32), "d^2")
    lv = M.loss_values(D, p, k, MARGIN)
    for mode in M.MODES + ("batch_hard",):
        for seed, seed_dev in ((1234, None), (999, SEEDS[2])):
            what = "%s seed %s" % (mode, seed_dev if seed_dev is not None else seed)
            fused = run_fused(dev, xd, p, k, e, mode, seed, seed_dev)
            live = seed_dev if seed_dev is not None else seed
            if mode == "batch_hard":
                sep = run_batch_hard(dev, Dd, p, k)
                want = dict(triplets=M.batch_hard(D, p, k), count=n)
            else:
                sep = run_mine(dev, Dd, p, k, mode, live)
                want = M.mine(D, p, k, MARGIN, mode, live, lv=lv)
                assert np.array_equal(fused["selected"], sep["selected"]) and np.array_equal(sep["selected"], want["selected"]), what
            trip, count, max_t = sep["dev"]
            loss, act, mean, _ = run_gather_fwd(dev, xd, n, e, trip.ptr(), count.ptr(), max_t)
            ref = M.gather_loss(x, want["triplets"], want["count"], MARGIN)
            assert ref["rows"].sum(dtype=np.float64) / M.STEP ** 2 < 2 ** 24
            assert fused["count"] == sep["count"] == want["count"], what
            assert np.array_equal(fused["triplets"], sep["triplets"]) and np.array_equal(sep["triplets"], want["triplets"]), what
            c = want["count"]
            for got in (fused, dict(loss=loss, active=act, mean=mean)):
                same_bits(got["loss"][:c], ref["rows"], what + " loss rows")
                same_bits(got["active"][:c], ref["active"], what + " active")
                assert (got["loss"][c:] == 0).all() and (got["active"][c:] == 0).all(), what
                same_bits(got["mean"], ref["mean"], what + " mean")


def test_fused_loss_supported_stops_one_step_beyond_each_limit(dev):
    lib = _lib.lib()
    for p, k, e in FUSED_SHAPES:
        assert lib.embnet_fused_loss_supported(p, k, e) == 1
    for p, k, e in [(128, 4, 3585), (32, 16, 513), (129, 4, 8), (257, 2, 8), (2, 17, 8), (30, 17, 8), (1, 4, 8), (4, 1, 8), (4, 4, 0),
                    (33, 16, 496)]:
        assert lib.embnet_fused_loss_supported(p, k, e) == 0, (p, k, e)


# ---- gather loss, lattice --------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 255, 256, 257, 700)


def corner_rows(e):
    """Three rows (a, p, n) with pos - neg + margin == 0 exactly: a = 0, p = 2 steps, n = 6 steps in the first coordinate
    (4/64 - 36/64 + 1/2)."""
    r = np.zeros((3, e), np.int64)
    r[1, 0], r[2, 0] = 2, 6
    return r


@functools.lru_cache(maxsize=4)
def gather_case(e, count, hub):
    """-> (x float32 [n, e], triplets int32 [max_t, 3] (rows >= count valid but dead), max_t)."""
    rs = np.random.RandomState(1000 * e + count)
    p, k = (2, 2) if e >= 1024 else (6, 4)
    amp = 2 if e >= 1024 else 6                                                      # keeps the 700-row loss sum below 2^24 units
    rows = np.concatenate([M.lattice(5, p, k, e, dense=True, moved=max(2, e // 8), centre_amp=amp)[0], corner_rows(e)])
    assert M.lattice_units_max(rows) < 2 ** 24
    n, base = len(rows), p * k
    max_t = count + 37
    t = np.zeros((max_t, 3), np.int32)
    for i in range(max_t):
        t[i] = rs.choice(base, size=3, replace=False)
    if hub:
        t[:, 2] = base - 1                                                           # one row is the negative of every triplet
        clash = (t[:, 0] == base - 1) | (t[:, 1] == base - 1) | (t[:, 0] == t[:, 1])
        t[clash, 0], t[clash, 1] = 0, 1
    else:
        t[rs.rand(max_t) < 0.1] = (base, base + 1, base + 2)                         # the b == 0 corner
        t[count - 1] = (base, base + 1, base + 2)
    x = (rows * M.STEP).astype(np.float32)
    x.setflags(write=False); t.setflags(write=False)
    return x, t, max_t


def check_gather_exact(dev, e, count, hub, upstreams):
    x, t, max_t = gather_case(e, count, hub)
    n = len(x)
    xd = place(x, dev)
    td = torch.from_numpy(np.array(t)).to(dev)
    cd = torch.tensor([count], dtype=torch.int32, device=dev)
    loss, act, mean, act_out = run_gather_fwd(dev, xd, n, e, td.data_ptr(), cd.data_ptr(), max_t)
    what = "e %d count %d" % (e, count)
    for up in upstreams:
        ref = M.gather_loss(x, t, count, MARGIN, up)
        assert ref["rows"].sum(dtype=np.float64) / M.STEP ** 2 < 2 ** 24              # the premise, for the mean's sum too
        same_bits(loss[:count], ref["rows"], what + " loss rows")
        same_bits(act[:count], ref["active"], what + " active")
        assert (loss[count:] == 0).all() and (act[count:] == 0).all(), what
        same_bits(mean, ref["mean"], what + " mean")
        if not hub:
            corner = np.all(t[:count] == t[count - 1], axis=1)
            assert corner.any() and (loss[:count][corner] == 0).all() and (act[:count][corner] == 1).all()
            assert np.abs(ref["demb"][-3:]).max() > 0                                # the gradient passes at b == 0
        else:
            assert ref["matches"][t[0, 2]] == int(ref["active"].sum()) >= count // 8   # hundreds of matches on one row
        same_bits(run_gather_bwd(dev, xd, n, e, td.data_ptr(), cd.data_ptr(), max_t, act_out, up), ref["demb"], what + " demb up %s" % up)


@pytest.mark.parametrize("e", [1, 3, 63, 64, 65, 300, 4096, 4097, 4100])
def test_gather_loss_lattice_is_exact(dev, e):
    for count in COUNTS:
        check_gather_exact(dev, e, count, False, (0.37, None) if count in (1, 257) else (0.37,))


def test_gather_loss_hub_row_is_exact(dev):
    for e, count in ((65, 700), (3, 257), (4097, 256)):
        check_gather_exact(dev, e, count, True, (0.37, None))


@pytest.mark.parametrize("e", [1, 3, 63, 64, 65, 300])
def test_hinge_concat_lattice_is_exact(dev, e):
    lib = _lib.lib()
    for t in (1, 5, 258):
        x, trip, _ = gather_case(e, 257, False)
        trip = trip[:t] if t > 1 else trip[256:257]                                  # t == 1: the b == 0 corner alone
        y = np.concatenate([x[trip[:, 0]], x[trip[:, 1]], x[trip[:, 2]]], axis=1)
        dloss = np.linspace(0.25, 1.75, t).astype(np.float32)
        yd, dd = place(y, dev), place(dloss, dev)
        loss, dy = fout(t, dev), fout(t * 3 * e, dev)
        names = traced(lambda: (_lib.check(lib.embnet_triplet_hinge_fwd(yd.data_ptr(), t, e, MARGIN, loss.ptr(), _lib.stream())),
                                _lib.check(lib.embnet_triplet_hinge_bwd(yd.data_ptr(), dd.data_ptr(), t, e, MARGIN, dy.ptr(),
                                                                       _lib.stream()))))
        assert names == ["triplet_hinge_fwd_kernel", "triplet_hinge_bwd_kernel"], names
        want_loss, want_dy = M.hinge_concat(y, MARGIN, dloss)
        same_bits(loss.get("hinge_fwd"), want_loss, "hinge loss e %d t %d" % (e, t))
        same_bits(dy.get("hinge_bwd").reshape(t, 3 * e), want_dy, "hinge dy e %d t %d" % (e, t))
        if t == 1:
            assert want_loss[0] == 0 and np.abs(want_dy).max() > 0


# ---- off-lattice families: bounded -----------------------------------------------------------------------------------------------------------
def check_decisions(got_selected, dec, path, family, what):
    ok = dec["decided"]
    share = 1 - ok.mean()
    UNDECIDED[(path, family)] = max(UNDECIDED.get((path, family), 0.0), share)
    print("undecided %s %s %.4f" % (path, what, share))
    bad = np.flatnonzero(ok & (got_selected != dec["selected"]))
    assert bad.size == 0, "%s %s: decided pairs %s picked %s, the restatement %s" % (path, what, bad[:8], got_selected[bad[:8]],
                                                                                 dec["selected"][bad[:8]])


@pytest.mark.parametrize("case", M.OFF_LATTICE_CASES, ids=lambda c: "%s-%dx%dx%d" % c)
def test_off_lattice_rows_within_the_textbook_bounds(dev, case):
    family, p, k, e = case
    n = p * k
    x = M.off_lattice_rows(family, p, k, e)
    x64 = x.astype(np.float64)
    xd = place(x, dev)
    # pairwise, per element
    d2_64, b2 = M.sqdist_bound(x)
    d2, _ = run_pairwise(dev, x, True)
    note_ratio("pairwise", family, np.abs(d2.cpu().numpy().astype(np.float64) - d2_64), b2)
    Dd, _ = run_pairwise(dev, x, False)
    for mode in M.MODES:
        dec = M.decisions(x, p, k, MARGIN, mode, 1234)
        what = "%s %s" % ("%s-%dx%dx%d" % case, mode)
        fused = run_fused(dev, xd, p, k, e, mode, 1234, launches=1)
        check_decisions(fused["selected"], dec, "fused", family, what)
        sep = run_mine(dev, Dd, p, k, mode, 1234)
        check_decisions(sep["selected"], dec, "separate", family, what)
        # gather forward on the triplets the separate path mined, per row; activity where the float64 value clears the bound
        trip, count, max_t = sep["dev"]
        c, t = sep["count"], sep["triplets"]
        loss, act, mean, act_out = run_gather_fwd(dev, xd, n, e, trip.ptr(), count.ptr(), max_t)
        a, pp, nn = x64[t[:, 0]], x64[t[:, 1]], x64[t[:, 2]]
        pos, neg = ((a - pp) ** 2).sum(1), ((a - nn) ** 2).sum(1)
        b64 = pos - neg + MARGIN
        bound = M.gamma(e + 2) * (pos + neg + MARGIN)
        note_ratio("gather_fwd", family, np.abs(loss[:c] - np.maximum(b64, 0)), bound)
        firm = np.abs(b64) > bound
        assert np.array_equal(act[:c][firm], (b64 >= 0)[firm].astype(np.float32)) and (loss[c:] == 0).all() and (act[c:] == 0).all()
        rows64 = loss[:c].astype(np.float64)
        note_ratio("mean", family, [abs(float(mean) - rows64.sum() / c)], [M.gamma(c + 1) * rows64.sum() / c])
        # backward, per element, on the kernel's own activity flags
        for up in (0.37, None):
            ref = M.gather_loss(x, t, c, MARGIN, None if up is None else float(np.float32(up)), np.float64, active=act[:c] != 0)
            demb = run_gather_bwd(dev, xd, n, e, trip.ptr(), count.ptr(), max_t, act_out, up)
            gam = np.array([M.gamma(2 * m + 4) for m in ref["matches"]])[:, None]
            note_ratio("gather_bwd", family, np.abs(demb - ref["demb"]), gam * ref["mag"])
