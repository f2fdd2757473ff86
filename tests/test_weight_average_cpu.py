"""CPU tests of weight averaging: the schedule of embeddingnet_amd/weight_average.py and tests/weight_average_ref.py against
closed forms and against torch.optim.swa_utils (float64), and the host side — what WeightAverager, parse_params and the two C entry
points refuse before anything is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import weight_average_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 3, 4, 2), (7,), (50,), (1,)]


def _snapshots(seed, steps):
    rs = np.random.RandomState(seed)
    return [[rs.randn(*s) for s in SHAPES] for _ in range(steps + 1)]            # [0]: the model at construction


def _run(snaps, mode, **kw):
    """The ideal float64 trajectory under the module's schedule -> (averages, updates made, the coefficients used)."""
    from embeddingnet_amd.weight_average import coefficient
    avg, u, cs = [w.copy() for w in snaps[0]], 0, []
    for t, ws in enumerate(snaps[1:], 1):
        c = coefficient(mode, t, u, **kw)
        assert c == float(R.coefficient(mode, t, u, **kw))                      # the restatement agrees, as fp32 values
        assert c == float(np.float32(c)) and 0.0 <= c <= 1.0
        cs.append(c)
        avg = [R.ideal_f64(a, w, c) for a, w in zip(avg, ws)]
        u += c > 0
    return avg, u, cs


# ------------------------------------------------------------------------------------------------ the schedule
def test_swa_is_the_arithmetic_mean_of_its_snapshots():
    snaps = _snapshots(1, 24)
    avg, u, cs = _run(snaps, "swa", start_iteration=6, update_every=4)
    taken = [t for t in range(1, 25) if t >= 6 and (t - 6) % 4 == 0]
    assert u == len(taken) == 5 and [t for t, c in enumerate(cs, 1) if c > 0] == taken and cs[5] == 1.0
    for i in range(len(SHAPES)):
        mean = np.mean([snaps[t][i] for t in taken], axis=0)
        assert np.abs(avg[i] - mean).max() <= 1e-7 * np.abs(mean).max()          # c is an fp32 value: 1/3 is off by 2^-25 relative


def test_ema_without_warmup_is_the_geometric_sum():
    snaps = _snapshots(2, 30)
    avg, u, cs = _run(snaps, "ema", decay=0.75, warmup=False)                    # 0.25 is exact in fp32: the closed form is too
    assert u == 30 and set(cs) == {0.25}
    for i in range(len(SHAPES)):
        want = 0.75 ** 30 * snaps[0][i] + sum(0.25 * 0.75 ** k * snaps[30 - k][i] for k in range(30))
        assert np.abs(avg[i] - want).max() <= 1e-13 * np.abs(want).max()


def test_ema_schedule_warmup_late_start_and_stride():
    from embeddingnet_amd.weight_average import coefficient
    # TensorFlow's num_updates warm-up: decay_t = min(decay, (1 + u) / (10 + u))
    assert [coefficient("ema", t, t - 1, decay=0.999) for t in (1, 2, 91)] == [float(np.float32(1 - v)) for v in (0.1, 2 / 11, 91 / 100)]
    assert coefficient("ema", 10 ** 6, 10 ** 6 - 1, decay=0.999) == float(np.float32(1 - 0.999))
    # a late start copies the model as it is then, warm-up or not; before it, and off the grid, nothing
    for warm in (True, False):
        kw = dict(decay=0.9, warmup=warm, start_iteration=5, update_every=3)
        assert [coefficient("ema", t, 0, **kw) for t in (1, 4, 5)] == [0.0, 0.0, 1.0]
        assert [coefficient("ema", t, 1, **kw) for t in (6, 7)] == [0.0, 0.0] and 0.0 < coefficient("ema", 8, 1, **kw) < 1.0
    assert coefficient("ema", 1, 0, decay=0.9, warmup=False) == float(np.float32(1 - 0.9))        # start 0: no copy step
    assert coefficient("swa", 7, 3) == float(np.float32(0.25)) and coefficient("swa", 1, 0) == 1.0


# ------------------------------------------------------------------------------------------------ against torch.optim.swa_utils
class _Net(torch.nn.Module):
    def __init__(self, ws):
        super().__init__()
        self.ws = torch.nn.ParameterList([torch.nn.Parameter(torch.tensor(w, dtype=torch.float64)) for w in ws])


def _set(net, ws):
    with torch.no_grad():
        for p, w in zip(net.ws, ws):
            p.copy_(torch.tensor(w, dtype=torch.float64))


def test_ema_against_torch_averaged_model():
    """torch's EMA: the first update_parameters copies, then avg = lerp(avg, w, 1 - decay): a late-starting averager without
    warm-up.  The decay is the fp32 coefficient's own, so that the two differ by float64 rounding only."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    snaps = _snapshots(3, 20)
    avg, u, cs = _run(snaps, "ema", decay=0.9, warmup=False, start_iteration=1)
    assert u == 20 and cs[0] == 1.0
    net = _Net(snaps[0])
    am = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(1.0 - cs[1]))
    for ws in snaps[1:]:
        _set(net, ws)
        am.update_parameters(net)
    for a, p in zip(avg, am.module.ws):
        assert np.abs(a - p.detach().numpy()).max() <= 1e-13 * np.abs(a).max()


def test_swa_against_torch_averaged_model():
    from torch.optim.swa_utils import AveragedModel, get_swa_multi_avg_fn
    snaps = _snapshots(4, 12)
    avg, u, cs = _run(snaps, "swa", start_iteration=2, update_every=2)
    net = _Net(snaps[0])
    am = AveragedModel(net, multi_avg_fn=get_swa_multi_avg_fn())
    for t, ws in enumerate(snaps[1:], 1):
        if cs[t - 1] > 0:
            _set(net, ws)
            am.update_parameters(net)
    assert int(am.n_averaged) == u == 6
    for a, p in zip(avg, am.module.ws):
        assert np.abs(a - p.detach().numpy()).max() <= 1e-7 * np.abs(a).max()    # 1/3, 1/5, 1/6 as fp32 values


# ------------------------------------------------------------------------------------------------ the fp32 reference
def test_update_f32_branches_and_roundings():
    rs = np.random.RandomState(5)
    a, w = rs.randn(1000).astype(np.float32), rs.randn(1000).astype(np.float32)
    a[:4] = np.array([0x7FC01234, 0xFFC00001, 0x7F800000, 0x80000000], dtype=np.uint32).view(np.float32)
    for c in (0.0, -1.0, float("nan")):
        assert np.array_equal(R.update_f32(a, w, c).view(np.uint32), a.view(np.uint32))
    assert np.array_equal(R.update_f32(a, w, 1.0).view(np.uint32), w.view(np.uint32))
    got = R.update_f32(a[4:], w[4:], 0.1)
    exact = a[4:].astype(np.float64) + float(np.float32(0.1)) * (w[4:].astype(np.float64) - a[4:].astype(np.float64))
    assert np.abs(got - exact).max() <= 3 * 2.0 ** -24 * np.abs(exact).max() + 2.0 ** -24 * 0.1 * 8
    # why c >= 1 has a branch of its own: a + 1 (w - a) is not w in fp32
    d = (w[4:] - a[4:]).astype(np.float32)
    assert np.mean((a[4:] + d).astype(np.float32) == w[4:]) < 0.9


def test_error_bound_holds_for_the_fp32_reference_with_headroom():
    """200 updates of random-walk weights: update_f32 stays inside the bound derived in weight_average_ref.py."""
    for decay in (0.9, 0.999):
        rs = np.random.RandomState(6)
        w = rs.randn(5000).astype(np.float32)
        a32, a64, bound, c = w.copy(), w.astype(np.float64), 0.0, R.coefficient("ema", 1, 0, decay=decay, warmup=False)
        for _ in range(200):
            w = (w + 0.05 * rs.randn(5000)).astype(np.float32)
            new = R.ideal_f64(a64, w, c)
            bound = R.error_bound(bound, c, a64, w.astype(np.float64), new)
            a32, a64 = R.update_f32(a32, w, c), new
        err = np.abs(a32 - a64).max()
        print(f"decay {decay}: error {err:.3e}, bound {bound:.3e}")
        assert err <= 0.5 * bound and bound <= 1.02 * 2.0 ** -24 * (np.abs(a64).max() * 1.1 + 1.0) * min(200, 1 / float(c))


# ------------------------------------------------------------------------------------------------ the host side
def test_constructor_refusals():
    from embeddingnet_amd.weight_average import WeightAverager
    net = torch.nn.Linear(3, 2)
    for kw, msg in [(dict(mode="mean"), "unknown mode"), (dict(decay=0.0), "inside"), (dict(decay=1.0), "inside"),
                    (dict(decay=-0.1), "inside"), (dict(mode="swa", decay=0.9), "belong to mode 'ema'"),
                    (dict(mode="swa", warmup=False), "belong to mode 'ema'"), (dict(update_every=0), "update_every"),
                    (dict(update_every=1.5), "update_every"), (dict(start_iteration=-1), "start_iteration")]:
        with pytest.raises(ValueError, match=msg):
            WeightAverager(net, **kw)
    with pytest.raises(ValueError, match="no floating-point tensors"):
        WeightAverager(torch.nn.ReLU())
    from embeddingnet_amd._lib import EmbnetError
    with pytest.raises(EmbnetError, match="contiguous fp32 GPU tensor"):
        WeightAverager(net)                                          # CPU tensors: the library has no CPU path
    with pytest.raises(EmbnetError, match="contiguous fp32 GPU tensor"):
        WeightAverager([net.double()])


def _config(tmp_path, averaging, name="simple2_ema_synthetic"):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name + ".yml")))
    cfg["TRAIN"]["weight_averaging"] = averaging
    path = tmp_path / "c.yml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def test_parse_params_checks_the_key(tmp_path):
    from embeddingnet_amd.utils import parse_params
    ema = parse_params(os.path.join(ROOT, "configs", "simple2_ema_synthetic.yml"))["train"]["weight_averaging"]
    assert ema == dict(mode="ema", decay=0.99, warmup=True, start_epoch=0, update_every=1, evaluate="averaged")
    swa = parse_params(os.path.join(ROOT, "configs", "simple2_swa_synthetic.yml"))["train"]["weight_averaging"]
    assert swa == dict(mode="swa", start_epoch=1, update_every="epoch", evaluate="averaged")
    assert "weight_averaging" not in parse_params(os.path.join(ROOT, "configs", "simple2_synthetic.yml"))["train"]
    got = parse_params(_config(tmp_path, {"mode": "ema"}))["train"]["weight_averaging"]
    assert got == dict(mode="ema", decay=0.999, warmup=True, start_epoch=0, update_every=1, evaluate="averaged")
    got = parse_params(_config(tmp_path, {"mode": "swa", "update_every": 5, "evaluate": "model"}))["train"]["weight_averaging"]
    assert got == dict(mode="swa", start_epoch=0, update_every=5, evaluate="model")
    for bad, msg in [({"mode": "ema", "decy": 0.9}, "unknown keys.*decy"), ({"decay": 0.9}, "mode must be"),
                     ({"mode": "mean"}, "mode must be"), ({"mode": "ema", "decay": 1.0}, "decay must be"),
                     ({"mode": "ema", "decay": "0.9"}, "decay must be"), ({"mode": "ema", "decay": True}, "decay must be"),
                     ({"mode": "ema", "warmup": 1}, "warmup must be"), ({"mode": "swa", "decay": 0.9}, "belongs to mode 'ema'"),
                     ({"mode": "swa", "warmup": True}, "belongs to mode 'ema'"), ({"mode": "ema", "start_epoch": -1}, "start_epoch"),
                     ({"mode": "ema", "start_epoch": 1.5}, "start_epoch"), ({"mode": "ema", "update_every": 0}, "update_every"),
                     ({"mode": "ema", "update_every": "step"}, "update_every"), ({"mode": "ema", "update_every": 2.0}, "update_every"),
                     ({"mode": "ema", "evaluate": "both"}, "evaluate must be"), ("ema", "a mapping")]:
        with pytest.raises(ValueError, match=msg):
            parse_params(_config(tmp_path, bad))


def test_new_exports_have_prototypes():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (("embnet_weight_average_update", 7), ("embnet_weight_average_swap", 5)):
        assert name in protos and hasattr(raw, name), name
        assert protos[name][0] is ctypes.c_int and len(protos[name][1]) == n_args
    assert protos["embnet_weight_average_update"][1][4] is ctypes.c_float
    assert _lib.lib().embnet_abi_version() == 22
    assert "#define EMBNET_ABI_VERSION 22" in open(_lib.HEADER_PATH).read()


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """Validation happens before any launch: the pointers are dummies and never dereferenced."""
    from embeddingnet_amd import _lib
    lib = _lib.lib()
    p = 4096                                                         # non-null, 16-byte aligned

    def update(table=p, n=1, chunks=p, n_chunks=1, c=0.5, c_dev=None):
        return lib.embnet_weight_average_update(table, n, chunks, n_chunks, c, c_dev, None)

    def swap(table=p, n=1, chunks=p, n_chunks=1):
        return lib.embnet_weight_average_swap(table, n, chunks, n_chunks, None)

    cases = [(update, dict(table=None), b"null pointer"), (update, dict(chunks=None), b"null pointer"),
             (update, dict(n=0), b"empty table"), (update, dict(n_chunks=0), b"empty table"),
             (update, dict(c=-0.25), b"outside [0, 1]"), (update, dict(c=1.5), b"outside [0, 1]"),
             (update, dict(c=float("nan")), b"outside [0, 1]"),
             (swap, dict(table=None), b"null pointer"), (swap, dict(chunks=None), b"null pointer"),
             (swap, dict(n=0), b"empty table"), (swap, dict(n_chunks=0), b"empty table")]
    for fn, kw, msg in cases:
        lib.embnet_pairwise_dist_f32(None, 4, 4, None, 0, None, 0, None)          # leaves another message behind
        assert fn(**kw) == -1 and msg in lib.embnet_last_error(), (kw, lib.embnet_last_error())
        assert (b"weight_average_update" if fn is update else b"weight_average_swap") in lib.embnet_last_error()
