"""CLAHE in the device augmentation, host side (no GPU): the entry points are declared and exported with the ABI still 22, the
CLAHE presets are `default` / `plates2` plus the reference's CLAHE record, invalid CLAHE pipelines are refused in DeviceAugment
and in the C entry points before anything runs, and the NumPy mirror gives hand-worked values (table fields, a flat tile, the
clip-and-remainder redistribution, OpenCV's padding quirk)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "embeddingnet_amd", "libembnet_hip.so")
NEW = ("embnet_augment_params_clahe", "embnet_augment_clahe_lut_bytes", "embnet_augment_clahe_luts", "embnet_augment_apply_clahe")
FAKE = 4096                                                 # a non-null, 16-byte aligned address: never dereferenced

import augment_ref as R  # noqa: E402
import clahe_ref as C  # noqa: E402


def test_header_declares_and_library_exports_clahe():
    from embeddingnet_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if " T embnet_" in ln}
    assert set(NEW) <= exported and exported == set(protos)
    assert _lib.lib().embnet_abi_version() == 22
    assert _lib.lib().embnet_augment_clahe_lut_bytes(128, 8, 8) == 128 * 8 * 8 * 256
    assert _lib.lib().embnet_augment_clahe_lut_bytes(3, 4, 6) == 3 * 6 * 4 * 256


def test_clahe_presets_are_the_reference_pipelines():
    from embeddingnet_amd.augment import DeviceAugment
    base, full = DeviceAugment.from_config("default", [64, 64, 3]), DeviceAugment.from_config("default_clahe", [64, 64, 3])
    assert base.clahe is None and full.records.tolist() == base.records.tolist() and full.n_ops == 5
    assert full.clahe.tolist() == np.float32([11, .4, 1, 4, 8, 8, 0, 0]).tolist() and full.clahe_pos == 3
    assert [n for n, _ in full.ops] == ["brightness_contrast", "gamma", "hue_saturation_value", "clahe", "blur", "gauss_noise"]
    base, full = DeviceAugment.from_config("plates2", [96, 96, 3]), DeviceAugment.from_config("plates2_clahe", [96, 96, 3])
    assert full.records.tolist() == base.records.tolist() and full.n_ops == 8
    assert full.clahe.tolist() == np.float32([11, .3, 1, 4, 8, 8, 0, 0]).tolist() and full.clahe_pos == 0
    # defaults, a scalar clip limit (albumentations: (1, c)), a list position, 9 entries = 8 ops + clahe
    a = DeviceAugment([{"gamma": {"p": 1}}, {"clahe": {"clip_limit": 2.5, "tile_grid_size": [4, 6]}}, {"blur": None}])
    assert a.clahe.tolist() == np.float32([11, .5, 1, 2.5, 4, 6, 0, 0]).tolist() and a.clahe_pos == 1 and a.grid == (4, 6)
    assert a.records.tolist() == DeviceAugment([{"gamma": {"p": 1}}, {"blur": None}]).records.tolist()
    assert DeviceAugment([("clahe", {})]).clahe.tolist() == np.float32([11, .5, 1, 4, 8, 8, 0, 0]).tolist()
    nine = DeviceAugment([{"horizontal_flip": {}}] + [{"gamma": {}}] * 7 + [{"clahe": {}}])
    assert nine.n_ops == 8 and nine.clahe_pos == 8


@pytest.mark.parametrize("value,shape,what", [
    ([{"clahe": {}}, {"clahe": {}}], [64, 64, 3], "at most one"),
    ([{"clahe": {"clip_limit": (4, 1)}}], [64, 64, 3], "clip_limit"),
    ([{"clahe": {"clip_limit": 0}}], [64, 64, 3], "clip_limit"),
    ([{"clahe": {"tile_grid_size": (0, 8)}}], [64, 64, 3], "tile_grid_size"),
    ([{"clahe": {"tile_grid_size": (8, 17)}}], [64, 64, 3], "tile_grid_size"),
    ([{"clahe": {"tile_grid_size": (8, 8)}}], [15, 64, 3], "too large"),
    ([{"clahe": {"tile_grid_size": (4, 9)}}], [64, 17, 3], "too large"),
    ([{"clahe": {}}], [64, 64, 2], "1-channel or 3-channel"),
    ([{"clahe": {}}], [64, 64, 4], "1-channel or 3-channel"),
    ([{"clahe": {"p": 1.5}}], [64, 64, 3], "p=1.5"),
    ([{"clahe": {"limit": 3}}], [64, 64, 3], "no parameter"),
    ([{"horizontal_flip": {}}] * 9 + [{"clahe": {}}], [64, 64, 3], "at most 8"),
])
def test_invalid_clahe_pipelines_are_refused(value, shape, what):
    from embeddingnet_amd.augment import DeviceAugment
    with pytest.raises(ValueError, match=what):
        DeviceAugment.from_config(value, shape)


def _params_clahe(clahe, pos=0, recs=((3, .5, 0, 0, 0, 0, 0, 0),), n=4, h=32, w=32, table=FAKE):
    from embeddingnet_amd import _lib
    recs = np.ascontiguousarray(np.asarray(recs, np.float32).reshape(-1, 8))
    c = None if clahe is None else np.ascontiguousarray(np.asarray(clahe, np.float32))
    rc = _lib.lib().embnet_augment_params_clahe(recs.ctypes.data, len(recs), None if c is None else c.ctypes.data, pos, 0, 0, n, h,
                                                w, table, None)
    return rc, _lib.lib().embnet_last_error().decode()


OK_REC = [11, .5, 1, 4, 8, 8, 0, 0]


@pytest.mark.parametrize("clahe,kw,what", [
    ([10, .5, 1, 4, 8, 8, 0, 0], {}, "opcode"),
    ([11, 1.5, 1, 4, 8, 8, 0, 0], {}, "p=1.5"),
    ([11, .5, 4, 1, 8, 8, 0, 0], {}, "clip_limit"),
    ([11, .5, 0, 4, 8, 8, 0, 0], {}, "clip_limit"),
    ([11, .5, 1, 4, 0, 8, 0, 0], {}, "tile_grid_size"),
    ([11, .5, 1, 4, 8, 17, 0, 0], {}, "tile_grid_size"),
    ([11, .5, 1, 4, 2.5, 8, 0, 0], {}, "tile_grid_size"),
    (OK_REC, dict(h=15), "too large"),
    (OK_REC, dict(w=15), "too large"),
    (OK_REC, dict(pos=2), "pos=2"),
    (OK_REC, dict(pos=-1), "pos=-1"),
    (OK_REC, dict(table=None), "null pointer"),
    (OK_REC, dict(recs=[[11, .5, 1, 4, 8, 8, 0, 0]]), "unknown opcode"),
])
def test_params_clahe_entry_point_rejects_before_any_launch(clahe, kw, what):
    rc, msg = _params_clahe(clahe, **kw)
    assert rc == -1 and what in msg, msg


def test_params_clahe_without_a_record_is_the_plain_entry_point():
    rc, msg = _params_clahe(None, recs=[[11, .5, 0, 0, 0, 0, 0, 0]])
    assert rc == -1 and "unknown opcode" in msg, msg


@pytest.mark.parametrize("entry", ["luts", "apply"])
@pytest.mark.parametrize("kw,what", [(dict(c_in=2, c_out=2), "c_in=2"), (dict(c_in=4, c_out=4), "c_in=4"),
                                     (dict(gx=0), "tile_grid_size"), (dict(gy=17), "tile_grid_size"), (dict(h=15), "too large"),
                                     (dict(luts=None), "null pointer"), (dict(src=None), "null pointer"), (dict(n=0), "n=0")])
def test_lut_and_apply_entry_points_reject_before_any_launch(entry, kw, what):
    from embeddingnet_amd import _lib
    a = dict(src=FAKE, n=4, h=32, w=32, c_in=3, c_out=3, gx=8, gy=8, luts=FAKE)
    a.update(kw)
    l = _lib.lib()
    if entry == "luts":
        rc = l.embnet_augment_clahe_luts(a["src"], None, a["n"], a["h"], a["w"], a["c_in"], a["gx"], a["gy"], FAKE, a["luts"], None)
    else:
        rc = l.embnet_augment_apply_clahe(a["src"], None, a["n"], a["h"], a["w"], a["c_in"], a["c_out"], FAKE, a["luts"], a["gx"],
                                          a["gy"], 0, 0, FAKE, None)
    msg = l.embnet_last_error().decode()
    assert rc == -1 and what in msg, msg


def test_train_accepts_clahe_presets_and_lists():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import importlib
    train = importlib.import_module("train")
    cfg = {"generator": {"device_augmentations": "default_clahe", "augment_seed": 7},
           "model": {"mode": "triplet", "input_shape": [64, 64, 3]}}
    assert train.device_augmentations(cfg).clahe_pos == 3
    cfg["generator"]["device_augmentations"] = [{"horizontal_flip": {"p": .5}},
                                                {"clahe": {"clip_limit": [1, 3], "tile_grid_size": [4, 4]}}]
    a = train.device_augmentations(cfg)
    assert a.clahe.tolist() == np.float32([11, .5, 1, 3, 4, 4, 0, 0]).tolist() and a.clahe_pos == 1 and a.n_ops == 1


def test_mirror_table_fields_10_to_14():
    """CLAHE's fields re-derived from rng_u32 (seed 5, batch 3, b = 256 / 257); rows where it did not fire are augment_ref's row
    of the list without it, bit for bit."""
    recs = np.float32([[3, .5, 0, 0, 0, 0, 0, 0], [7, .7, 80, 120, 0, 0, 0, 0]])
    clahe = np.float32([11, .5, 2, 3, 4, 6, 0, 0])
    t = C.params(recs, 2, clahe, 1, 5, 3, 64, 32, 32)
    plain = R.params(recs, 2, 5, 3, 64, 32, 32)
    rows = np.arange(64, dtype=np.uint64) + np.uint64(3 * 65536)
    fire = (R.rng_u32(5, rows, 256) >> np.uint32(8)).astype(np.float64) / 2 ** 24 < 0.5
    assert 10 < fire.sum() < 54
    clip = np.float32(2) + np.float32(1) * ((R.rng_u32(5, rows, 257) >> np.uint32(8)).astype(np.float32) * np.float32(2 ** -24))
    assert np.array_equal(t[fire, 11], clip[fire]) and ((t[fire, 11] >= 2) & (t[fire, 11] < 3)).all()
    assert (t[fire, 12] == 1).all() and (t[fire, 13] == 4).all() and (t[fire, 14] == 6).all()
    assert np.array_equal(t[fire, 10], plain[fire, 10] + 1)
    assert np.array_equal(t[~fire], plain[~fire]) and (t[~fire, 11:15] == 0).all()
    t[fire, 10] -= 1
    t[fire, 11:15] = 0
    assert np.array_equal(t, plain)                     # nothing else moves
    # every row fires at p = 1: the clip draws of rows 0..2 of seed 0, batch 0
    t = C.params(recs, 2, np.float32([11, 1, 1, 4, 8, 8, 0, 0]), 2, 0, 0, 3, 32, 32)
    assert t[:, 12:15].tolist() == [[2, 8, 8]] * 3
    u = (R.rng_u32(0, np.arange(3, dtype=np.uint64), 257) >> np.uint32(8)).astype(np.float32) * np.float32(2 ** -24)
    assert t[:, 11].tolist() == (np.float32(1) + np.float32(3) * u).tolist()


def test_mirror_flat_tile():
    """An 8x8 tile of one value v = 100: clip = max(1, int(4 * 64 / 256)) = 1, excess 63 -> 0 per bin plus 1 to bins 0, 4, ...,
    248 (step 256 // 63 = 4); scale 255 / 64 = 3.984375."""
    hist = np.zeros(256, np.int64)
    hist[100] = 64
    assert C.clip_limit(np.float32(4), 64) == 1
    r = C.redistribute(hist, 1)
    want = np.zeros(256, np.int64)
    want[0:249:4] = 1
    want[100] += 1
    assert np.array_equal(r, want) and r.sum() == 64
    lut = C.lut(hist, 1, 64)
    assert [int(lut[i]) for i in (0, 3, 4, 99, 100, 247, 248, 255)] == [4, 4, 8, 100, 108, 251, 255, 255]
    img = np.full((16, 16), 100, np.uint8)              # 2 x 2 tiles of 8 x 8, all flat: every LUT is that one
    luts, out = C.gray(img, 2, 2, np.float32(4))
    assert (luts == lut).all() and (out == np.float32(108) / np.float32(255)).all()


def test_mirror_clip_and_remainder_redistribution():
    # batch > 0: 1024 pixels, clip = int(1 * 1024 / 256) = 4; excess 596 + 6 * 66 = 992 = 3 * 256 + 224 -> +3 everywhere, +1 to 0..223
    hist = np.zeros(256, np.int64)
    hist[10], hist[100:106], hist[200] = 600, 70, 4
    assert C.clip_limit(np.float32(1), 1024) == 4
    r = C.redistribute(hist, 4)
    want = np.full(256, 3, np.int64) + (np.arange(256) < 224)
    want[[10, 100, 101, 102, 103, 104, 105, 200]] += 4
    assert np.array_equal(r, want) and r.sum() == 1024
    # a small remainder: excess 3 -> step 85, bins 0, 85, 170
    hist = np.zeros(256, np.int64)
    hist[50], hist[100:162], hist[170] = 7, 4, 1
    r = C.redistribute(hist, 4)
    want = np.minimum(hist, 4)
    want[[0, 85, 170]] += 1
    assert np.array_equal(r, want) and r.sum() == 256
    lut = C.lut(hist, 4, 256)                            # scale 255 / 256 = 0.99609375
    assert [int(lut[i]) for i in (0, 49, 50, 99, 100, 170, 255)] == [1, 1, 5, 6, 10, 255, 255]
    # clip_f32 -> int(double(clip) * total / 256) truncates: 3.99 * 64 / 256 = 0.9975 -> max(1, 0) = 1; 2.5 * 841 / 256 = 8.21 -> 8
    assert C.clip_limit(np.float32(3.99), 64) == 1 and C.clip_limit(np.float32(2.5), 841) == 8


def test_mirror_padding_quirk():
    """h divisible, w not: BOTH axes pad (the divisible one by a full g); padded pixels count in their tiles."""
    assert C.tile_size(112, 105, 8, 8) == (14, 15) and C.tile_size(224, 224, 8, 8) == (28, 28)
    assert C.tile_size(105, 105, 8, 8) == (14, 14) and C.tile_size(37, 53, 4, 6) == (14, 7)
    img = np.zeros((16, 13), np.uint8)                   # grid (2, 2): padded 18 x 14, tiles 7 wide x 9 high
    img[14] = 255
    p = C.pad_image(img, 2, 2)
    assert p.shape == (18, 14) and np.array_equal(p[16], p[14]) and np.array_equal(p[17], p[13])
    assert np.array_equal(p[:, 13], p[:, 11])
    hist = C.tile_histograms(img.astype(np.int64), 2, 2)
    assert hist[1, 1, 255] == 14 and hist[1, 1, 0] == 63 - 14          # row 14 and its reflection row 16, 7 columns each
    assert hist[1, 0, 255] == 14 and hist[0, 0, 255] == 0 and hist.sum() == 18 * 14


def test_mirror_lab_pair():
    l8, a, b = C.bgr_to_lab(np.float64([[255, 255, 255], [0, 0, 0], [0, 0, 255]]))
    assert np.allclose(l8[:2], [255, 0], atol=1e-3) and np.allclose(a[:2], 0, atol=1e-3) and np.allclose(b[:2], 0, atol=1e-3)
    assert abs(l8[2] / 2.55 - 53.24) < 0.05 and a[2] > 70                # sRGB red
    rs = np.random.RandomState(0)
    v = rs.rand(500, 3) * 255
    l8, a, b = C.bgr_to_lab(v)
    assert np.abs(C.lab_to_bgr(l8 * 100 / 255, a, b) - v).max() < 0.05   # OpenCV's two matrices are 6-digit inverses
