"""Device augmentation on the GPU (csrc/augment.hip): no op fired is embnet_u8_to_f32 bit for bit, the parameter table is the
NumPy mirror's, flips and rot90 are exact permutations, every op matches a float64 reference fed the dumped table, noise has
the drawn variance and is reproducible, the store and prefetch feeders agree, and tools/train.py trains with the key."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from embeddingnet_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _src(dev, n, h, w, seed=0):
    rs = np.random.RandomState(seed + h * 7 + w)
    src = rs.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    src.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return src, torch.from_numpy(src).to(dev)


ALL_P0 = [("random_resized_crop", {"p": 0}), ("center_crop", {"p": 0}), ("horizontal_flip", {"p": 0}), ("vertical_flip", {"p": 0}),
          ("brightness_contrast", {"p": 0}), ("gamma", {"p": 0}), ("hue_saturation_value", {"p": 0}), ("blur", {"p": 0})]


@pytest.mark.parametrize("ops", [[], ALL_P0, [("gauss_noise", {"p": 0}), ("random_rotate90", {"p": 0})]])
@pytest.mark.parametrize("h,w,pad,indexed", [(24, 32, None, False), (24, 32, 4, True), (37, 53, None, True), (37, 53, 4, False)])
def test_nothing_fired_is_u8_to_f32_bit_for_bit(dev, ops, h, w, pad, indexed):
    from embeddingnet_amd.augment import DeviceAugment
    from embeddingnet_amd.input_pipeline import u8_to_f32
    if h != w:
        ops = [o for o in ops if o[0] != "random_rotate90"]
    src, d = _src(dev, 9, h, w)
    idx = torch.from_numpy(np.random.RandomState(1).permutation(9)[:6].astype(np.int32)).to(dev) if indexed else None
    want = u8_to_f32(d, idx, 6, pad_to=pad)
    got = DeviceAugment(ops, seed=11).apply(d, idx, 6, pad_to=pad)
    assert got.shape == want.shape and torch.equal(got, want)


P1 = [("random_resized_crop", {"p": .7}), ("center_crop", {"p": .6, "frac": .8}), ("horizontal_flip", {"p": .5}),
      ("vertical_flip", {"p": .3}), ("random_rotate90", {"p": .4}), ("brightness_contrast", {"p": .5}), ("gamma", {"p": .6}),
      ("hue_saturation_value", {"p": .45})]
P2 = [("blur", {"p": .35, "blur_limit": 7}), ("gauss_noise", {"p": .55, "var_limit": (10, 50)}),
      ("brightness_contrast", {"p": .25, "brightness_limit": .3, "contrast_limit": 0})]
INT_FIELDS = list(range(0, 8)) + [9, 10]


@pytest.mark.parametrize("ops", [P1, P2])
def test_parameter_table_is_the_numpy_mirror(dev, ops):
    from embeddingnet_amd.augment import DeviceAugment
    aug = DeviceAugment(ops, seed=12345)
    n = 4096
    for bno in (0, 77):
        got = aug.params(n, bno, (64, 64)).cpu().numpy()
        want = R.params(aug.records, len(ops), aug.seed, bno, n, 64, 64)
        ints = INT_FIELDS + [R.SLOTS + 4 * i for i in range(len(ops))]
        for i, (name, _) in enumerate(ops):
            if name in ("random_resized_crop", "center_crop", "random_rotate90", "blur"):
                ints += [R.SLOTS + 4 * i + 1, R.SLOTS + 4 * i + 2, R.SLOTS + 4 * i + 3]
        assert np.array_equal(got[:, ints], want[:, ints])
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, np.argwhere(ulps > 1)[:5]
        for i, (name, kw) in enumerate(ops):
            fired = got[:, R.SLOTS + 4 * i] != 0
            p = kw["p"]
            assert abs(fired.mean() - p) <= 5 * np.sqrt(p * (1 - p) / n), (name, fired.mean())
            s = got[fired, R.SLOTS + 4 * i + 1: R.SLOTS + 4 * i + 4]
            if name == "brightness_contrast":
                assert (np.abs(s[:, 0] - 1) <= 0.2 + 1e-6).all() and (np.abs(s[:, 1]) <= kw.get("brightness_limit", .2) + 1e-6).all()
            elif name == "gamma":
                assert ((s[:, 0] >= 0.8) & (s[:, 0] <= 1.2)).all()
            elif name == "hue_saturation_value":
                assert (np.abs(s) <= np.float32([20, 30, 20]) + 1e-4).all()
            elif name == "random_rotate90":
                assert set(np.unique(s[:, 0])) == {0, 1, 2, 3}
            elif name == "blur":
                assert set(np.unique(s[:, 0])) == {3, 5, 7}
            elif name == "gauss_noise":
                assert ((s[:, 1] >= 10) & (s[:, 1] <= 50)).all() and np.allclose(s[:, 0] ** 2, s[:, 1], rtol=1e-6)
            elif name == "random_resized_crop":
                area = s[:, 0] * s[:, 1] / (64 * 64)
                att = s[:, 2] > 0
                assert ((area[att] >= 0.08 * 0.9) & (area[att] <= 1.0)).all() and att.mean() > 0.9
        box = got[:, :4]
        assert ((box[:, 0] >= 0) & (box[:, 1] >= 0) & (box[:, 0] + box[:, 2] <= 64) & (box[:, 1] + box[:, 3] <= 64)).all()


def test_flips_and_rot90_are_exact_permutations(dev):
    from embeddingnet_amd.augment import DeviceAugment
    from embeddingnet_amd.input_pipeline import u8_to_f32
    src, d = _src(dev, 16, 40, 40)
    base = u8_to_f32(d, None, 16).cpu().numpy()
    for ops in ([("horizontal_flip", {"p": 1})], [("vertical_flip", {"p": 1})], [("random_rotate90", {"p": 1})],
                [("horizontal_flip", {"p": .5}), ("vertical_flip", {"p": .5}), ("random_rotate90", {"p": 1})]):
        aug = DeviceAugment(ops, seed=3)
        t = aug.params(16, 4, (40, 40)).cpu().numpy()
        got = aug.apply(d, None, 16, batch_no=4).cpu().numpy()
        for i in range(16):
            want = np.rot90(base[i], int(t[i, 6]))
            if t[i, 4]:
                want = want[:, ::-1]
            if t[i, 5]:
                want = want[::-1]
            assert np.array_equal(got[i], want), (ops, i)


SINGLE = [("random_resized_crop", {"p": 1}), ("center_crop", {"p": 1, "frac": 0.7}), ("horizontal_flip", {"p": 1}),
          ("vertical_flip", {"p": 1}), ("random_rotate90", {"p": 1}),
          ("brightness_contrast", {"p": 1, "brightness_limit": .3, "contrast_limit": .4}), ("gamma", {"p": 1}),
          ("hue_saturation_value", {"p": 1, "hue_shift_limit": 50, "sat_shift_limit": 40, "val_shift_limit": 40}),
          ("blur", {"p": 1, "blur_limit": 7})]


@pytest.mark.parametrize("h,w", [(64, 64), (105, 105), (224, 224), (37, 53)])
def test_ops_match_the_float64_reference(dev, h, w):
    from embeddingnet_amd.augment import DeviceAugment
    n = 3
    src, d = _src(dev, n + 2, h, w)
    idx = torch.tensor([4, 0, 2], dtype=torch.int32, device=dev)
    pipelines = [[op] for op in SINGLE] + [[o for o in SINGLE if o[0] != "center_crop"]]
    for ops in pipelines:
        if h != w:
            ops = [o for o in ops if o[0] != "random_rotate90"]
            if not ops:
                continue
        aug = DeviceAugment(ops, seed=h + w)
        t = aug.params(n, 9, (h, w)).cpu().numpy()
        got = aug.apply(d, idx, n, batch_no=9).cpu().numpy()
        for i, j in enumerate([4, 0, 2]):
            want = R.apply_image(src[j], t[i])
            err = np.abs(got[i].astype(np.float64) - want).max()
            assert err <= 1e-5, ([o[0] for o in ops], h, w, i, err, t[i, :11])


def test_noise_statistics_and_reproducibility(dev):
    from embeddingnet_amd.augment import DeviceAugment
    n, h, w = 8, 64, 64
    d = torch.full((n, h, w, 3), 128, dtype=torch.uint8, device=dev)
    aug = DeviceAugment([("gauss_noise", {"p": 1, "var_limit": (10, 50)})], seed=21)
    t = aug.params(n, 3, (h, w)).cpu().numpy()
    x = aug.apply(d, None, n, batch_no=3).cpu().numpy().astype(np.float64) * 255 - 128
    for i in range(n):
        var = x[i].var()
        sig2 = float(t[i, 8]) ** 2
        assert abs(var / sig2 - 1) <= 0.05, (i, var, sig2)
        assert abs(x[i].mean()) <= 5 * np.sqrt(sig2 / x[i].size), (i, x[i].mean())
    again = aug.apply(d, None, n, batch_no=3)
    assert np.array_equal(again.cpu().numpy().astype(np.float64) * 255 - 128, x)
    other = aug.apply(d, None, n, batch_no=4).cpu().numpy()
    assert all(not np.array_equal(other[i], again[i].cpu().numpy()) for i in range(n))
    few = aug.apply(d, None, 3, batch_no=3)
    assert torch.equal(few, again[:3])
    # the counter: calls without batch_no take 0, 1, 2, ...
    fresh = DeviceAugment([("gauss_noise", {"p": 1, "var_limit": (10, 50)})], seed=21)
    seq = [fresh.apply(d, None, n) for _ in range(4)]
    assert torch.equal(seq[3], again) and fresh.batch_no == 4


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """6 classes x 8 JPEG files of 40x33 random pixels."""
    from PIL import Image
    root = tmp_path_factory.mktemp("aug_images")
    rs = np.random.RandomState(0)
    for ci in range(6):
        os.makedirs(root / f"class{ci}")
        for i in range(8):
            arr = (rs.rand(33, 40, 3) * 255).astype(np.uint8)
            Image.fromarray(arr).save(str(root / f"class{ci}" / f"im{i}.jpg"), quality=90)
    return root


FEED_OPS = [("random_resized_crop", {"p": 1, "scale": (0.16, 1)}), ("horizontal_flip", {"p": .5}),
            ("brightness_contrast", {"p": .4}), ("gamma", {"p": .4}), ("hue_saturation_value", {"p": .4}),
            ("blur", {"p": .3, "blur_limit": 5}), ("gauss_noise", {"p": .3, "var_limit": (50, 80)})]


def test_feeder_store_and_prefetch_agree_with_device_augmentation(dev, tree, monkeypatch):
    from embeddingnet_amd.augment import DeviceAugment
    from embeddingnet_amd.datagenerators import ENDataLoader, TripletsDataGenerator
    dl = ENDataLoader(str(tree), validate=False)
    out = {}
    for kind in ("store", "prefetch"):
        monkeypatch.setenv("EMBNET_IMAGE_STORE", "1" if kind == "store" else "0")
        gen = TripletsDataGenerator(None, dl.train_data, dl.class_names, input_shape=[32, 32, 3], k_classes=4, k_samples=3,
                                    negatives_selection_mode="semihard", device_augmentations=DeviceAugment(FEED_OPS, seed=5))
        np.random.seed(7)
        feeder = gen.feeder(dev, depth=3, workers=2)
        try:
            assert feeder.kind.startswith(kind)
            out[kind] = [feeder.next().cpu().numpy() for _ in range(6)]
        finally:
            feeder.close()
    for a, b in zip(out["store"], out["prefetch"]):
        assert a.shape == (12, 32, 32, 3) and np.array_equal(a, b)
    assert not np.array_equal(out["store"][0], out["store"][1])


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
  project_name : 'aug_tree'
  work_dir : '{work}/'
"""


def test_train_cli_with_device_augmentations(dev, tree, tmp_path):
    """crop_flip trains to a finite loss; `none` dumps final weights bit-identical to the run without the key.  (The three
    runs go concurrently.)"""
    runs = {"crop_flip": "  device_augmentations : 'crop_flip'\n  augment_seed : 3", "none": "  device_augmentations : 'none'",
            "absent": ""}
    procs = {}
    for name, extra in runs.items():
        d = tmp_path / name
        d.mkdir()
        (d / "cfg.yml").write_text(CFG.format(tree=tree, extra=extra, work=d / "work"))
        env = dict(os.environ, EMBNET_DUMP_FINAL_WEIGHTS=str(d / "final_"))
        procs[name] = subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "train.py"), str(d / "cfg.yml")],
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=str(d), env=env)
    outs = {name: p.communicate(timeout=600) for name, p in procs.items()}
    for name, p in procs.items():
        assert p.returncode == 0, (name, outs[name][1][-3000:])
    lines = [l for l in outs["crop_flip"][0].splitlines() if l.startswith("Epoch ")]
    assert "input pipeline: store" in outs["crop_flip"][0]
    assert len(lines) == 1 and "nan" not in lines[0] and "inf" not in lines[0].split("loss")[1], lines
    a, b = np.load(tmp_path / "none" / "final_0.npz"), np.load(tmp_path / "absent" / "final_0.npz")
    assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files)
    c = np.load(tmp_path / "crop_flip" / "final_0.npz")
    assert any(not np.array_equal(a[k], c[k]) for k in a.files)


def test_invalid_calls_launch_nothing(dev):
    l = _lib.lib()
    table = torch.full((4, 48), 7.0, device=dev)
    dst = torch.full((4, 16, 16, 3), 7.0, device=dev)
    src = torch.zeros((4, 16, 16, 3), dtype=torch.uint8, device=dev)
    bad = np.float32([[11, .5, 0, 0, 0, 0, 0, 0]])
    assert l.embnet_augment_params(bad.ctypes.data, 1, 0, 0, 4, 16, 16, table.data_ptr(), _lib.stream()) != 0
    assert b"unknown opcode" in l.embnet_last_error()
    rot = np.float32([[5, .5, 0, 0, 0, 0, 0, 0]])
    assert l.embnet_augment_params(rot.ctypes.data, 1, 0, 0, 4, 16, 20, table.data_ptr(), _lib.stream()) != 0
    assert l.embnet_augment_apply(src.data_ptr(), None, 4, 16, 16, 5, 5, table.data_ptr(), 0, 0, dst.data_ptr(), _lib.stream()) != 0
    assert l.embnet_augment_apply(src.data_ptr(), None, 0, 16, 16, 3, 3, table.data_ptr(), 0, 0, dst.data_ptr(), _lib.stream()) != 0
    torch.cuda.synchronize()
    assert (table == 7).all() and (dst == 7).all()
