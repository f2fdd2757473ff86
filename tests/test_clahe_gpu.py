"""CLAHE in the device augmentation on the GPU (csrc/augment.hip): where CLAHE does not fire, the output is the pipeline without it
bit for bit; gray LUTs equal the NumPy mirror's byte for byte and the output is within 1e-6; the BGR presets match a float64
reference fed the dumped table and LUTs; runs are reproducible, the store and prefetch feeders agree, and tools/train.py trains
with `default_clahe` and with a list holding a clahe op."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_ref as C  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bgr(dev, n, h, w, seed=0):
    """Smooth colour waves with noise and a flat block: narrow and one-bin tile histograms, so that the clip matters."""
    rs = np.random.RandomState(seed + 31 * h + w)
    y, x = np.mgrid[0:h, 0:w]
    img = np.zeros((n, h, w, 3))
    for i in range(n):
        for ch in range(3):
            img[i, ..., ch] = 60 + 40 * np.sin((x * (ch + 1) + y * (i + 1)) / 9.0) + 12 * rs.randn(h, w)
        img[i, h // 4:h // 2, w // 3:w // 2] = rs.randint(0, 256, 3)
    src = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return src, torch.from_numpy(src).to(dev)


def _gray(n, h, w):
    rs = np.random.RandomState(h * w)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([90 + 50 * np.sin(x / (5.0 + i)) * np.cos(y / 7.0) + (4 + 6 * i) * rs.randn(h, w) for i in range(n)])
    img[:, :h // 3, :w // 3] = (30 + 40 * np.arange(n))[:, None, None]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)[..., None]


BASE = [("random_resized_crop", {"p": .5, "scale": (.3, 1)}), ("horizontal_flip", {"p": .5}), ("brightness_contrast", {"p": .5}),
        ("gamma", {"p": .5}), ("hue_saturation_value", {"p": .5}), ("blur", {"p": .4, "blur_limit": 5}), ("gauss_noise", {"p": .4})]


@pytest.mark.parametrize("pad", [None, 4])
def test_rows_where_clahe_did_not_fire_are_the_pipeline_without_it(dev, pad):
    from embeddingnet_amd.augment import DeviceAugment
    n, h, w = 24, 48, 40
    src, d = _bgr(dev, n + 4, h, w)
    idx = torch.from_numpy(np.random.RandomState(2).permutation(n + 4)[:n].astype(np.int32)).to(dev)
    want = DeviceAugment(BASE, seed=9).apply(d, idx, n, batch_no=5, pad_to=pad)
    for pos, p in ((0, 0.0), (4, 0.0), (3, 0.5), (7, 0.5)):
        aug = DeviceAugment(BASE[:pos] + [("clahe", {"p": p, "tile_grid_size": (4, 3)})] + BASE[pos:], seed=9)
        got = aug.apply(d, idx, n, batch_no=5, pad_to=pad)
        fired = torch.from_numpy(aug.params(n, 5, (h, w)).cpu().numpy()[:, 11] != 0).to(dev)
        assert int(fired.sum()) == 0 if p == 0 else 0 < int(fired.sum()) < n
        assert torch.equal(got[~fired], want[~fired]), (pos, p)
        assert all(not torch.equal(got[i], want[i]) for i in torch.nonzero(fired).flatten().tolist())
    base = DeviceAugment.from_config("default", [w, h, 3], seed=4)
    full = DeviceAugment.from_config("default_clahe", [w, h, 3], seed=4)
    for b in (0, 1):
        tb, tf = base.params(n, b).cpu().numpy(), full.params(n, b).cpu().numpy()
        fired = tf[:, 11] != 0
        assert fired.any() and not fired.all()
        assert np.array_equal(tf[~fired], tb[~fired]) and np.array_equal(np.delete(tf, [10, 11, 12, 13, 14], 1),
                                                                         np.delete(tb, [10, 11, 12, 13, 14], 1))
        got, ref = full.apply(d, idx, n, batch_no=b, pad_to=pad), base.apply(d, idx, n, batch_no=b, pad_to=pad)
        keep = torch.from_numpy(~fired).to(dev)
        assert torch.equal(got[keep], ref[keep])


@pytest.mark.parametrize("h,w", [(224, 224), (105, 105), (112, 105), (37, 53)])
def test_gray_luts_equal_the_mirror_and_output_is_within_1e_6(dev, h, w):
    from embeddingnet_amd.augment import DeviceAugment
    n = 3
    src = _gray(n, h, w)
    d = torch.from_numpy(src).to(dev)
    for gx, gy in ((8, 8), (4, 6), (1, 1)):
        aug = DeviceAugment([("clahe", {"p": 1, "clip_limit": (1, 4), "tile_grid_size": (gx, gy)})], seed=h + gx)
        t = aug.params(n, 2, (h, w)).cpu().numpy()
        luts = aug.clahe_luts(d, None, n, 2).cpu().numpy()
        out = aug.apply(d, None, n, batch_no=2).cpu().numpy()
        assert luts.shape == (n, gy, gx, 256) and out.shape == (n, h, w, 1)
        for i in range(n):
            want_luts, want_out = C.gray(src[i, ..., 0], gx, gy, t[i, 11])
            assert np.array_equal(luts[i], want_luts), (h, w, gx, gy, i, np.argwhere(luts[i] != want_luts)[:5])
            err = np.abs(out[i, ..., 0].astype(np.float64) - want_out).max()
            assert err <= 1e-6, (h, w, gx, gy, i, err)


def _tiles_any(mask, gx, gy):
    """bool [gy, gx]: any True in each tile of the padded mask."""
    h, w = mask.shape
    tw, th = C.tile_size(h, w, gx, gy)
    return C.pad_image(mask, gx, gy).reshape(gy, th, gx, tw).any(axis=(1, 3))


@pytest.mark.parametrize("preset,h,w", [("default_clahe", 64, 64), ("default_clahe", 37, 53), ("plates2_clahe", 64, 64),
                                        ("plates2_clahe", 40, 40)])
def test_bgr_presets_match_the_float64_reference(dev, preset, h, w):
    """Every p = 1 except gauss_noise (0): crops, flips, rot90, the pixel ops around CLAHE and a blur over CLAHE'd halos.  A
    pixel whose reference L8 lies within 1e-2 of a .5 boundary may take the other bin in float32: those pixels (and the blur
    windows that hold one) are left out of the output check, and the tiles that hold one out of the LUT check."""
    from embeddingnet_amd.augment import PRESETS, DeviceAugment
    ops = [(name, dict(kw, p=0.0 if name == "gauss_noise" else 1.0)) for name, kw in PRESETS[preset]]
    n, rows = 3, [3, 0, 2]
    src, d = _bgr(dev, n + 1, h, w)
    idx = torch.tensor(rows, dtype=torch.int32, device=dev)
    aug = DeviceAugment(ops, seed=h * w)
    t = aug.params(n, 6, (h, w)).cpu().numpy()
    luts = aug.clahe_luts(d, idx, n, 6).cpu().numpy()
    out = aug.apply(d, idx, n, batch_no=6).cpu().numpy()
    gx, gy = aug.grid
    checked = 0
    for i, j in enumerate(rows):
        assert t[i, 11] != 0 and (preset != "default_clahe" or t[i, 7] == 3)
        want_luts, l8 = C.luts(src[j], t[i])
        near = C.near_half(l8)
        ok = ~_tiles_any(near, gx, gy)
        assert np.array_equal(luts[i][ok], want_luts[ok]), (preset, h, w, i)
        checked += int(ok.sum())
        ref = C.apply_image(src[j], t[i], luts[i])
        rad = int(t[i, 7]) // 2
        if rad:
            p = np.pad(near, rad, mode="reflect")
            near = np.any([p[dy:dy + h, dx:dx + w] for dy in range(2 * rad + 1) for dx in range(2 * rad + 1)], axis=0)
        assert near.mean() < 0.25
        err = np.abs(out[i].astype(np.float64) - ref)[~near].max()
        assert err <= 1e-4, (preset, h, w, i, err)
    assert checked >= 6, checked


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """6 classes x 8 JPEG files of 40x33 smooth colour images."""
    from PIL import Image
    root = tmp_path_factory.mktemp("clahe_images")
    rs = np.random.RandomState(0)
    y, x = np.mgrid[0:33, 0:40]
    for ci in range(6):
        os.makedirs(root / f"class{ci}")
        for i in range(8):
            arr = 120 + 60 * np.sin((x * (ci + 1) + y * (i + 1))[..., None] / np.float64([7, 9, 11])) + 20 * rs.randn(33, 40, 3)
            Image.fromarray(np.clip(arr, 0, 255).astype(np.uint8)).save(str(root / f"class{ci}" / f"im{i}.jpg"), quality=90)
    return root


def test_runs_are_reproducible_and_the_feeders_agree(dev, tree, monkeypatch):
    from embeddingnet_amd.augment import DeviceAugment
    from embeddingnet_amd.datagenerators import ENDataLoader, TripletsDataGenerator
    src, d = _bgr(dev, 16, 40, 48)
    aug = DeviceAugment.from_config("default_clahe", [48, 40, 3], seed=3)
    l1, o1 = aug.clahe_luts(d, None, 16, 1).clone(), aug.apply(d, None, 16, batch_no=1).clone()
    l2, o2 = aug.clahe_luts(d, None, 16, 1), aug.apply(d, None, 16, batch_no=1)
    assert torch.equal(l1, l2) and torch.equal(o1, o2) and l1.any()
    dl = ENDataLoader(str(tree), validate=False)
    out = {}
    for kind in ("store", "prefetch"):
        monkeypatch.setenv("EMBNET_IMAGE_STORE", "1" if kind == "store" else "0")
        gen = TripletsDataGenerator(None, dl.train_data, dl.class_names, input_shape=[32, 32, 3], k_classes=4, k_samples=3,
                                    negatives_selection_mode="semihard",
                                    device_augmentations=DeviceAugment.from_config("default_clahe", [32, 32, 3], seed=5))
        np.random.seed(7)
        feeder = gen.feeder(dev, depth=3, workers=2)
        try:
            assert feeder.kind.startswith(kind)
            out[kind] = [feeder.next().cpu().numpy() for _ in range(6)]
        finally:
            feeder.close()
    for a, b in zip(out["store"], out["prefetch"]):
        assert a.shape == (12, 32, 32, 3) and np.array_equal(a, b)
    aug = DeviceAugment.from_config("default_clahe", [32, 32, 3], seed=5)
    assert any((aug.params(12, b).cpu().numpy()[:, 11] != 0).any() for b in range(6))      # CLAHE took part


CFG = """
MODEL:
  input_shape : [32, 32, 3]
  encodings_len: 32
  mode : 'triplet'
  distance_type : 'l2'
  backbone_name : 'simple2'
  backbone_weights : null
  freeze_backbone : False
  embeddings_normalization: True
DATALOADER:
  dataset_path : '{tree}'
  validate : False
  val_ratio : 0.2
GENERATOR:
  negatives_selection_mode : 'hardest'
  k_classes: 4
  k_samples: 3
  margin: 0.5
  batch_size : 8
  n_batches : 3
  augmentations : 'none'
  augment_seed : 3
{extra}
TRAIN:
  optimizer : 'adam'
  learning_rate : 0.001
  decay_factor : 0.5
  step_size : 1
  n_epochs : 1
  plot_history : False
ENCODINGS:
  save_encodings : False
GENERAL:
  project_name : 'clahe_tree'
  work_dir : '{work}/'
"""


def test_train_cli_with_clahe(dev, tree, tmp_path):
    """The preset and a list holding a clahe op both train to a finite loss (the two runs go concurrently)."""
    runs = {"preset": "  device_augmentations : 'default_clahe'",
            "list": "  device_augmentations :\n    - horizontal_flip: {p: 0.5}\n"
                    "    - clahe: {p: 1.0, clip_limit: [1, 3], tile_grid_size: [4, 4]}"}
    procs = {}
    for name, extra in runs.items():
        d = tmp_path / name
        d.mkdir()
        (d / "cfg.yml").write_text(CFG.format(tree=tree, extra=extra, work=d / "work"))
        procs[name] = subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(d / "cfg.yml")],
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=str(d))
    outs = {name: p.communicate(timeout=600) for name, p in procs.items()}
    for name, p in procs.items():
        assert p.returncode == 0, (name, outs[name][1][-3000:])
        lines = [l for l in outs[name][0].splitlines() if l.startswith("Epoch ")]
        assert "input pipeline: store" in outs[name][0]
        assert len(lines) == 1 and "nan" not in lines[0] and "inf" not in lines[0].split("loss")[1], (name, lines)
