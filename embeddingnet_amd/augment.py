"""Seeded on-device image augmentation for triplet training batches (csrc/augment.hip, include/embnet.h "Device augmentation").

The reference lists four albumentations pipelines (embedding_net/augmentations.py: default, plates, deepfake, plates2) but,
through a misspelt config key (utils.py:160), never builds them.  Here a pipeline is a short list of ops that one HIP kernel
applies while it gathers and converts a uint8 batch — the HBM-resident DeviceImageStore keeps its one-kernel-per-batch path —
with every draw taken from the counter RNG keyed by (seed, batch number, row): an augmented run is reproducible whatever the
number of decode workers.

    aug = DeviceAugment.from_config("crop_flip", input_shape=[224, 224, 3], seed=0)
    x = aug.apply(store_u8, index, n)              # float32 [n, H, W, 3] in [0, 1]; the batch counter advances by one

Ops (name: parameters, defaults):
    random_resized_crop   p=1, scale=(0.08, 1), ratio=(3/4, 4/3)      torchvision's rule (10 attempts, centre fallback)
    center_crop           p=1, frac=2/3                               the centre frac of the image, resized back
    horizontal_flip       p=0.5
    vertical_flip         p=0.5
    random_rotate90       p=0.5                                       k in 0..3; square images only
    brightness_contrast   p=0.5, brightness_limit=0.2, contrast_limit=0.2
    gamma                 p=0.5, gamma_limit=(80, 120)
    hue_saturation_value  p=0.5, hue_shift_limit=20, sat_shift_limit=30, val_shift_limit=20   (3-channel BGR images)
    blur                  p=0.5, blur_limit=7                         box, odd k in [3, max(3, blur_limit)], blur_limit <= 7
    gauss_noise           p=0.5, var_limit=(10, 50)
Geometry runs first, then the pixel ops in list order, then blur, then noise (include/embnet.h has the exact rules).

Presets mirror the reference's pipelines.  CLAHE (in `default` and `plates2`) is not implemented and is left out of both;
`plates` is refused: its RandomCrop returns 2/3-size images, which cannot form a batch of input_shape.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

OPCODES = {"random_resized_crop": 1, "center_crop": 2, "horizontal_flip": 3, "vertical_flip": 4, "random_rotate90": 5,
           "brightness_contrast": 6, "gamma": 7, "hue_saturation_value": 8, "blur": 9, "gauss_noise": 10}
# op -> (default p, [(parameter, default)]); a tuple-valued parameter fills two record fields
_PARAMS = {
    "random_resized_crop": (1.0, [("scale", (0.08, 1.0)), ("ratio", (3 / 4, 4 / 3))]),
    "center_crop": (1.0, [("frac", 2 / 3)]),
    "horizontal_flip": (0.5, []),
    "vertical_flip": (0.5, []),
    "random_rotate90": (0.5, []),
    "brightness_contrast": (0.5, [("brightness_limit", 0.2), ("contrast_limit", 0.2)]),
    "gamma": (0.5, [("gamma_limit", (80.0, 120.0))]),
    "hue_saturation_value": (0.5, [("hue_shift_limit", 20.0), ("sat_shift_limit", 30.0), ("val_shift_limit", 20.0)]),
    "blur": (0.5, [("blur_limit", 7)]),
    "gauss_noise": (0.5, [("var_limit", (10.0, 50.0))]),
}
GEOMETRY = ("random_resized_crop", "center_crop", "horizontal_flip", "vertical_flip", "random_rotate90")
MAX_OPS, RECORD = 8, 8

PRESETS = {
    "deepfake": [("horizontal_flip", {"p": 0.5})],
    # the reference's Blur(blur_limit=1) is albumentations' minimum kernel, 3; its CLAHE(p=0.4) is left out
    "default": [("brightness_contrast", {"p": 0.4, "brightness_limit": 0.2, "contrast_limit": 0.2}),
                ("gamma", {"p": 0.4, "gamma_limit": (80, 120)}),
                ("hue_saturation_value", {"p": 0.4, "hue_shift_limit": 20, "sat_shift_limit": 30, "val_shift_limit": 30}),
                ("blur", {"p": 0.3, "blur_limit": 3}),
                ("gauss_noise", {"p": 0.3, "var_limit": (50, 80)})],
    # CLAHE(p=0.3) left out; RandomBrightness / RandomContrast are brightness_contrast with the other limit 0; the CenterCrop
    # (+ Resize back) is geometry, so it is applied first
    "plates2": [("horizontal_flip", {"p": 0.5}),
                ("vertical_flip", {"p": 0.5}),
                ("brightness_contrast", {"p": 0.3, "brightness_limit": 0.2, "contrast_limit": 0.0}),
                ("brightness_contrast", {"p": 0.3, "brightness_limit": 0.0, "contrast_limit": 0.2}),
                ("random_rotate90", {"p": 0.3}),
                ("hue_saturation_value", {"p": 0.5, "hue_shift_limit": 50, "sat_shift_limit": 15, "val_shift_limit": 15}),
                ("gauss_noise", {"p": 0.3, "var_limit": (10, 50)}),
                ("center_crop", {"p": 1.0, "frac": 2 / 3})],
    # the usual metric-learning recipe
    "crop_flip": [("random_resized_crop", {"p": 1.0, "scale": (0.16, 1.0), "ratio": (3 / 4, 4 / 3)}),
                  ("horizontal_flip", {"p": 0.5})],
}


def _normalise(ops):
    """[(name, {params})] or [{name: {params}}] -> [(name, {every parameter})], checked on the host."""
    out = []
    for item in ops:
        if isinstance(item, dict):
            if len(item) != 1:
                raise ValueError(f"device augmentation: an op is a one-key mapping {{op: {{params}}}}, got {item!r}")
            (name, kw), = item.items()
        else:
            name, kw = item
        kw = dict(kw or {})
        if name not in _PARAMS:
            raise ValueError(f"device augmentation: unknown op {name!r} (known: {', '.join(_PARAMS)})")
        p0, spec = _PARAMS[name]
        full = {"p": float(kw.pop("p", p0))}
        for key, dflt in spec:
            full[key] = kw.pop(key, dflt)
        if kw:
            raise ValueError(f"device augmentation: {name} has no parameter(s) {sorted(kw)}")
        out.append((name, full))
    return out


def _record(name, kw):
    rec = [float(OPCODES[name]), float(kw["p"])]
    for key, _ in _PARAMS[name][1]:
        v = kw[key]
        rec += [float(x) for x in v] if isinstance(v, (tuple, list)) else [float(v)]
    return rec + [0.0] * (RECORD - len(rec))


class DeviceAugment:
    """A seeded augmentation pipeline run by the HIP kernels of csrc/augment.hip.  `ops`: [(name, {params})] or
    [{name: {params}}] (module docstring).  Host-side checks here; the library repeats them (and rejects anything else) before
    any launch."""

    def __init__(self, ops, seed=0):
        self.ops = _normalise(ops)
        if len(self.ops) > MAX_OPS:
            raise ValueError(f"device augmentation: {len(self.ops)} ops (at most {MAX_OPS})")
        for name, kw in self.ops:
            if not 0.0 <= kw["p"] <= 1.0:
                raise ValueError(f"device augmentation: {name} p={kw['p']} outside [0, 1]")
            if name == "blur" and not 1 <= kw["blur_limit"] <= 7:
                raise ValueError(f"device augmentation: blur_limit={kw['blur_limit']} (1..7; the box filter is at most 7x7)")
        self.records = np.zeros((max(1, len(self.ops)), RECORD), np.float32)
        for i, (name, kw) in enumerate(self.ops):
            self.records[i] = _record(name, kw)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.batch_no = 0
        self.hw = None
        self._table = None

    @classmethod
    def from_config(cls, value, input_shape, seed=0):
        """GENERATOR.device_augmentations -> a DeviceAugment, or None for None / 'none' (training unchanged).  `value`: a
        preset name (PRESETS) or a list of {op: {params}} mappings; input_shape = MODEL.input_shape [W, H, C]."""
        if value is None or (isinstance(value, str) and value.lower() == "none"):
            return None
        if isinstance(value, str):
            if value == "plates":
                raise ValueError("device augmentation preset 'plates' is not supported: its RandomCrop returns 2/3-size "
                                 "images, which cannot form a batch of input_shape (use 'plates2')")
            if value not in PRESETS:
                raise ValueError(f"unknown device augmentation preset {value!r} (known: {', '.join(PRESETS)}, none)")
            value = PRESETS[value]
        aug = cls(value, seed=seed)
        aug.check_shape(int(input_shape[1]), int(input_shape[0]), int(input_shape[2]) if len(input_shape) > 2 else 3)
        return aug

    def check_shape(self, h, w, c=3):
        names = [n for n, _ in self.ops]
        if "random_rotate90" in names and h != w:
            raise ValueError(f"device augmentation: random_rotate90 needs square images (got {h}x{w})")
        if "hue_saturation_value" in names and c != 3:
            raise ValueError(f"device augmentation: hue_saturation_value needs 3-channel BGR images (got {c} channels)")
        self.hw = (h, w)

    def params(self, n, batch_no, hw=None):
        """The parameter table [n, embnet_augment_param_floats()] of batch `batch_no` on the current device (tests, debugging)."""
        h, w = hw or self.hw
        f = int(_lib.lib().embnet_augment_param_floats())
        if self._table is None or self._table.shape[0] < n or self._table.device != torch.device("cuda", torch.cuda.current_device()):
            self._table = torch.empty((max(n, 128), f), device="cuda", dtype=torch.float32)
        table = self._table[:n]
        check(_lib.lib().embnet_augment_params(self.records.ctypes.data, len(self.ops), self.seed, int(batch_no), n, h, w,
                                               ptr(table), stream()))
        return table

    def apply(self, src_u8, index, n, batch_no=None, out=None, pad_to=None):
        """float32 [n, H, W, C'] = augment(src_u8[index or :n]) / 255 on the device.  Batch `batch_no`, or the next of this
        object's counter (which advances by one per call that does not name one)."""
        _, h, w, c = src_u8.shape
        if batch_no is None:
            batch_no = self.batch_no
            self.batch_no += 1
        if self.hw != (h, w):
            self.check_shape(h, w, c)
        c_out = pad_to or c
        if out is None:
            out = torch.empty((n, h, w, c_out), device=src_u8.device, dtype=torch.float32)
        table = self.params(n, batch_no, (h, w))
        check(_lib.lib().embnet_augment_apply(ptr(src_u8), ptr(index), n, h, w, c, c_out, ptr(table), self.seed, int(batch_no),
                                              ptr(out), stream()))
        return out

    def __repr__(self):
        return f"DeviceAugment({self.ops!r}, seed={self.seed})"


def rank_seed(seed, rank):
    """The augmentation seed of a data-parallel rank: `seed` on rank 0, distinct streams on the others."""
    return (int(seed) ^ (int(rank) * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF
