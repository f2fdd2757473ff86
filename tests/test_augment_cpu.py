"""Device augmentation, host side (no GPU): the C ABI is declared and exported, presets expand exactly, invalid pipelines and
configs are refused before anything runs, parse_params is unchanged, and the NumPy mirror of the RNG and of the parameter
draws gives known values."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_augment_param_floats", "embnet_augment_params", "embnet_augment_apply")

import augment_ref as R  # noqa: E402


def test_header_declares_and_library_exports_augment():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported and exported == set(protos)
    assert _lib.lib().embnet_augment_param_floats() == R.F == 48
    assert _lib.lib().embnet_abi_version() == 22


def test_presets_expand_exactly():
    from embeddingnet_amd.augment import DeviceAugment
    a = DeviceAugment.from_config("crop_flip", [224, 224, 3])
    assert a.records[:2].tolist() == np.float32([[1, 1, 0.16, 1, 3 / 4, 4 / 3, 0, 0], [3, 0.5, 0, 0, 0, 0, 0, 0]]).tolist()
    a = DeviceAugment.from_config("default", [64, 64, 3])
    assert a.records.tolist() == np.float32([[6, .4, .2, .2, 0, 0, 0, 0], [7, .4, 80, 120, 0, 0, 0, 0], [8, .4, 20, 30, 30, 0, 0, 0],
                                             [9, .3, 3, 0, 0, 0, 0, 0], [10, .3, 50, 80, 0, 0, 0, 0]]).tolist()
    a = DeviceAugment.from_config("deepfake", [64, 48, 3])
    assert a.records.tolist() == np.float32([[3, .5, 0, 0, 0, 0, 0, 0]]).tolist()
    a = DeviceAugment.from_config("plates2", [96, 96, 3])
    assert [n for n, _ in a.ops] == ["horizontal_flip", "vertical_flip", "brightness_contrast", "brightness_contrast",
                                     "random_rotate90", "hue_saturation_value", "gauss_noise", "center_crop"]
    assert a.records[2].tolist() == np.float32([6, .3, .2, 0, 0, 0, 0, 0]).tolist()
    assert a.records[3].tolist() == np.float32([6, .3, 0, .2, 0, 0, 0, 0]).tolist()
    assert a.records[5].tolist() == np.float32([8, .5, 50, 15, 15, 0, 0, 0]).tolist()
    assert a.records[7].tolist() == np.float32([2, 1, 2 / 3, 0, 0, 0, 0, 0]).tolist()
    assert DeviceAugment.from_config("none", [64, 64, 3]) is None and DeviceAugment.from_config(None, [64, 64, 3]) is None
    a = DeviceAugment.from_config([{"gamma": {"p": 1, "gamma_limit": [90, 110]}}, {"blur": None}], [64, 64, 3])
    assert a.records.tolist() == np.float32([[7, 1, 90, 110, 0, 0, 0, 0], [9, .5, 7, 0, 0, 0, 0, 0]]).tolist()


@pytest.mark.parametrize("value,shape,what", [
    ("plates", [64, 64, 3], "RandomCrop"),
    ("nope", [64, 64, 3], "unknown device augmentation preset"),
    ([{"sharpen": {}}], [64, 64, 3], "unknown op"),
    ([{"random_rotate90": {}}], [64, 48, 3], "square"),
    ("plates2", [64, 48, 3], "square"),
    ([{"blur": {"blur_limit": 9}}], [64, 64, 3], "blur_limit"),
    ([{"gamma": {"p": 1.5}}], [64, 64, 3], "p=1.5"),
    ([{"horizontal_flip": {}}] * 9, [64, 64, 3], "at most 8"),
    ([{"gamma": {"limit": 3}}], [64, 64, 3], "no parameter"),
])
def test_invalid_pipelines_are_refused(value, shape, what):
    from embeddingnet_amd.augment import DeviceAugment
    with pytest.raises(ValueError, match=what):
        DeviceAugment.from_config(value, shape)


FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced


def _params(recs, n_ops=None, n=4, h=16, w=16, table=FAKE):
    from embeddingnet_amd import _lib
    recs = np.ascontiguousarray(np.asarray(recs, np.float32).reshape(-1, 8))
    rc = _lib.lib().embnet_augment_params(recs.ctypes.data, len(recs) if n_ops is None else n_ops, 0, 0, n, h, w, table, None)
    return rc, _lib.lib().embnet_last_error().decode()


@pytest.mark.parametrize("recs,kw,what", [
    ([[3, .5, 0, 0, 0, 0, 0, 0]], dict(n=0), "n=0"),
    ([[11, .5, 0, 0, 0, 0, 0, 0]], {}, "unknown opcode"),
    ([[3, .5, 0, 0, 0, 0, 0, 0]] * 9, {}, "n_ops=9"),
    ([[5, .5, 0, 0, 0, 0, 0, 0]], dict(h=16, w=20), "square"),
    ([[9, .5, 8, 0, 0, 0, 0, 0]], {}, "blur_limit=8"),
    ([[3, 1.5, 0, 0, 0, 0, 0, 0]], {}, "p=1.5"),
    ([[3, -0.1, 0, 0, 0, 0, 0, 0]], {}, "p=-0.1"),
    ([[3, .5, 0, 0, 0, 0, 0, 0]], dict(table=None), "null pointer"),
    ([[3, .5, 0, 0, 0, 0, 0, 0], [3, .5, 0, 0, 0, 0, 0, 0]], {}, "appears twice"),
    ([[1, 1, .5, .2, .75, 1.3, 0, 0]], {}, "random_resized_crop"),
])
def test_params_entry_point_rejects_before_any_launch(recs, kw, what):
    rc, msg = _params(recs, **kw)
    assert rc == -1 and what in msg, msg


@pytest.mark.parametrize("kw,what", [(dict(src=None), "null pointer"), (dict(table=None), "null pointer"),
                                     (dict(dst=None), "null pointer"), (dict(n=0), "n=0"), (dict(c_in=5, c_out=5), "c_in=5"),
                                     (dict(c_out=2), "c_out=2"), (dict(c_out=17), "c_out=17"), (dict(h=3), "h=3")])
def test_apply_entry_point_rejects_before_any_launch(kw, what):
    from embeddingnet_amd import _lib
    a = dict(src=FAKE, index=None, n=4, h=16, w=16, c_in=3, c_out=3, table=FAKE, dst=FAKE)
    a.update(kw)
    rc = _lib.lib().embnet_augment_apply(a["src"], a["index"], a["n"], a["h"], a["w"], a["c_in"], a["c_out"], a["table"], 0, 0,
                                         a["dst"], None)
    msg = _lib.lib().embnet_last_error().decode()
    assert rc == -1 and what in msg, msg


def test_parse_params_of_every_shipped_config_is_unchanged():
    """The new key passes through GENERATOR untouched; no shipped config sets it, so nothing else changes."""
    from embeddingnet_amd.utils import parse_params
    import yaml
    for name in sorted(os.listdir(os.path.join(ROOT, "configs"))):
        path = os.path.join(ROOT, "configs", name)
        raw = yaml.safe_load(open(path))
        p = parse_params(path)
        assert "device_augmentations" not in p["generator"]
        assert p["generator"] == dict(raw["GENERATOR"], input_shape=raw["MODEL"]["input_shape"], augmentations=None)
        assert p["model"] == raw["MODEL"] and p["dataloader"] == raw["DATALOADER"]


def _train_module():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import importlib
    return importlib.import_module("train")


def _cfg(mode="triplet", value="crop_flip", shape=(64, 64, 3)):
    return {"generator": {"device_augmentations": value, "augment_seed": 7}, "model": {"mode": mode, "input_shape": list(shape)}}


def test_train_refuses_the_key_with_synthetic_data_or_siamese_mode():
    train = _train_module()
    with pytest.raises(ValueError, match="synthetic"):
        train.device_augmentations(_cfg(), synthetic=10)
    with pytest.raises(ValueError, match="Siamese"):
        train.device_augmentations(_cfg(mode="siamese"))
    assert train.device_augmentations(_cfg(value="none"), synthetic=10) is None
    assert train.device_augmentations(_cfg(mode="siamese", value="none")) is None
    a0, a1 = train.device_augmentations(_cfg(), rank=0), train.device_augmentations(_cfg(), rank=1)
    assert a0.seed == 7 and a1.seed != 7
    with pytest.raises(ValueError, match="RandomCrop"):
        train.device_augmentations(_cfg(value="plates"))


def test_generator_refuses_host_and_device_augmentation_together_and_float_datasets():
    from embeddingnet_amd.augment import DeviceAugment
    from embeddingnet_amd.datagenerators import SyntheticDataLoader, TripletsDataGenerator
    aug = DeviceAugment.from_config("deepfake", [16, 16, 3])
    files = {"a": ["x.jpg"], "b": ["y.jpg"]}
    with pytest.raises(ValueError, match="not both"):
        TripletsDataGenerator(None, files, ["a", "b"], input_shape=[16, 16, 3], augmentations=lambda image: {"image": image},
                              device_augmentations=aug)
    dl = SyntheticDataLoader(3, 4, [16, 16, 3], validate=False)
    with pytest.raises(ValueError, match="synthetic"):
        TripletsDataGenerator(None, dl.train_data, dl.class_names, input_shape=[16, 16, 3], device_augmentations=aug)
    g = TripletsDataGenerator(None, files, ["a", "b"], input_shape=[16, 16, 3], device_augmentations=aug)
    assert g.device_augmentations is aug and g.augmentations is None


# rng_u32(seed, a, b) of csrc/common.h, computed by the C implementation
RNG_KNOWN = [(0, 0, 0, 2802244911), (0, 1, 0, 409945657), (1, 0, 1, 2262236565), (12345, 458755, 31, 755745299),
             (3735928559, 65536127, 4294967306, 3671988110)]


def test_numpy_mirror_of_rng_u32_gives_known_values():
    for seed, a, b, want in RNG_KNOWN:
        assert int(R.rng_u32(seed, a, b)) == want


def test_numpy_mirror_of_the_parameter_draws_gives_known_values():
    """Fields follow include/embnet.h's table layout: flips, rot90 and noise re-derived from rng_u32 for seed 3, batch 2;
    the crop_flip boxes pinned to what the C implementation of the row draws (compiled for the host) gives."""
    from embeddingnet_amd.augment import DeviceAugment
    a = DeviceAugment([("horizontal_flip", {"p": 0.5}), ("random_rotate90", {"p": 1.0}), ("gauss_noise", {"p": 1.0})], seed=3)
    t = R.params(a.records, len(a.ops), 3, 2, 6, 32, 32)
    rows = np.arange(6, dtype=np.uint64) + np.uint64(2 * 65536)
    u0 = (R.rng_u32(3, rows, 0) >> np.uint32(8)).astype(np.float64) / 2 ** 24
    assert np.array_equal(t[:, 4], (u0 < 0.5).astype(np.float32))
    assert np.array_equal(t[:, 16], np.where(u0 < 0.5, 3, 0).astype(np.float32))
    k = ((R.rng_u32(3, rows, 33) >> np.uint32(8)).astype(np.uint64) * 4) >> np.uint64(24)
    assert np.array_equal(t[:, 6], k.astype(np.float32)) and np.array_equal(t[:, 21], k.astype(np.float32))
    var = np.float32(10) + np.float32(40) * ((R.rng_u32(3, rows, 65) >> np.uint32(8)).astype(np.float32) * np.float32(2 ** -24))
    assert np.array_equal(t[:, 26], var) and np.array_equal(t[:, 8], np.sqrt(var)) and (t[:, 9] == 1).all()
    assert np.array_equal(t[:, :4], np.tile(np.float32([0, 0, 32, 32]), (6, 1)))
    assert np.array_equal(t[:, 10], 2 + t[:, 4])
    # a row's draws do not depend on n
    assert np.array_equal(R.params(a.records, 3, 3, 2, 2, 32, 32), t[:2])
    # pinned values of a crop draw
    c = DeviceAugment.from_config("crop_flip", [224, 224, 3], seed=0)
    t = R.params(c.records, 2, 0, 0, 4, 224, 224)
    assert t[:, :4].tolist() == [[43, 62, 123, 122], [65, 44, 119, 158], [11, 2, 201, 219], [41, 12, 172, 210]]
    assert t[:, 16:20].tolist() == [[1, 123, 122, 1], [1, 119, 158, 1], [1, 201, 219, 3], [1, 172, 210, 1]]
    assert t[:, 20].tolist() == [0, 3, 0, 0]
