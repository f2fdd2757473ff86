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
    clahe                 p=0.5, clip_limit=(1, 4), tile_grid_size=(8, 8)   OpenCV's CLAHE on the gray value or on L* of the BGR
                                                                            pixel; a scalar clip_limit c is (1, c); grid
                                                                            (columns, rows), each in 1..16; at most one clahe
Geometry runs first, then the pixel ops in list order (clahe among them, where it is listed), then blur, then noise
(include/embnet.h has the exact rules).  CLAHE needs every tile's histogram first, so a pipeline with it runs three kernels
(parameters, LUTs, apply) instead of two; it keeps out of the 8 op slots, so every other op draws the same with or without it.

Presets mirror the reference's pipelines.  `default` and `plates2` leave the reference's CLAHE out (runs and tests pin them);
`default_clahe` and `plates2_clahe` are the reference's full pipelines.  `plates` is refused: its RandomCrop returns 2/3-size
images, which cannot form a batch of input_shape.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

OPCODES = {"random_resized_crop": 1, "center_crop": 2, "horizontal_flip": 3, "vertical_flip": 4, "random_rotate90": 5,
           "brightness_contrast": 6, "gamma": 7, "hue_saturation_value": 8, "blur": 9, "gauss_noise": 10, "clahe": 11}
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
    "clahe": (0.5, [("clip_limit", (1.0, 4.0)), ("tile_grid_size", (8, 8))]),
}
GEOMETRY = ("random_resized_crop", "center_crop", "horizontal_flip", "vertical_flip", "random_rotate90")
MAX_OPS, RECORD = 8, 8
MAX_CLAHE_GRID = 16

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
# the reference's full pipelines: `default` with its CLAHE(p=0.4) after HSV, `plates2` with its CLAHE(clip_limit=(1, 4), p=0.3)
# first among the pixel ops (after the geometry, which runs first anyway)
PRESETS["default_clahe"] = PRESETS["default"][:3] + [("clahe", {"p": 0.4, "clip_limit": (1, 4), "tile_grid_size": (8, 8)})] + \
    PRESETS["default"][3:]
PRESETS["plates2_clahe"] = [("clahe", {"p": 0.3, "clip_limit": (1, 4), "tile_grid_size": (8, 8)})] + PRESETS["plates2"]


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


def _clip_limit(v):
    """clahe's clip_limit: a scalar c is (1, c) as in albumentations (sorted), a pair (lo, hi) needs 0 < lo <= hi."""
    lo, hi = (min(1.0, float(v)), max(1.0, float(v))) if np.isscalar(v) else (float(v[0]), float(v[1]))
    if not (0 < lo <= hi < float("inf")):
        raise ValueError(f"device augmentation: clahe clip_limit={v!r} (0 < lo <= hi)")
    return (lo, hi)


def _grid(v):
    """clahe's tile_grid_size (columns, rows): integers in 1..16."""
    try:
        gx, gy = v
    except (TypeError, ValueError):
        raise ValueError(f"device augmentation: clahe tile_grid_size={v!r} (a pair (columns, rows))") from None
    if not all(float(g) == int(g) and 1 <= int(g) <= MAX_CLAHE_GRID for g in (gx, gy)):
        raise ValueError(f"device augmentation: clahe tile_grid_size={v!r} (integers in 1..{MAX_CLAHE_GRID})")
    return (int(gx), int(gy))


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
        names = [n for n, _ in self.ops]
        if names.count("clahe") > 1:
            raise ValueError(f"device augmentation: {names.count('clahe')} clahe ops (at most one)")
        # CLAHE keeps out of the op slots: its record and position (the number of other ops before it) are kept apart, and
        # `records` is what the list without it gives
        self.clahe, self.clahe_pos = None, 0
        if "clahe" in names:
            self.clahe_pos = names.index("clahe")
            kw = self.ops[self.clahe_pos][1]
            kw["clip_limit"] = _clip_limit(kw["clip_limit"])
            kw["tile_grid_size"] = _grid(kw["tile_grid_size"])
            self.clahe = np.float32(_record("clahe", kw))
        base = [(n, kw) for n, kw in self.ops if n != "clahe"]
        if len(base) > MAX_OPS:
            raise ValueError(f"device augmentation: {len(base)} ops (at most {MAX_OPS}, plus one clahe)")
        for name, kw in self.ops:
            if not 0.0 <= kw["p"] <= 1.0:
                raise ValueError(f"device augmentation: {name} p={kw['p']} outside [0, 1]")
            if name == "blur" and not 1 <= kw["blur_limit"] <= 7:
                raise ValueError(f"device augmentation: blur_limit={kw['blur_limit']} (1..7; the box filter is at most 7x7)")
        self.n_ops = len(base)
        self.records = np.zeros((max(1, len(base)), RECORD), np.float32)
        for i, (name, kw) in enumerate(base):
            self.records[i] = _record(name, kw)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.batch_no = 0
        self.hw = None
        self._table = None
        self._luts = None

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
        if self.clahe is not None:
            if c not in (1, 3):
                raise ValueError(f"device augmentation: clahe needs 1-channel or 3-channel BGR images (got {c} channels)")
            gx, gy = self.grid
            if 2 * gx > w or 2 * gy > h:
                raise ValueError(f"device augmentation: clahe tile_grid_size=({gx}, {gy}) too large for {h}x{w} images "
                                 f"(2 * columns <= width, 2 * rows <= height)")
        self.hw = (h, w)

    @property
    def grid(self):
        """CLAHE's tile grid (columns, rows), or None without clahe."""
        return None if self.clahe is None else (int(self.clahe[4]), int(self.clahe[5]))

    def params(self, n, batch_no, hw=None):
        """The parameter table [n, embnet_augment_param_floats()] of batch `batch_no` on the current device (tests, debugging)."""
        h, w = hw or self.hw
        f = int(_lib.lib().embnet_augment_param_floats())
        if self._table is None or self._table.shape[0] < n or self._table.device != torch.device("cuda", torch.cuda.current_device()):
            self._table = torch.empty((max(n, 128), f), device="cuda", dtype=torch.float32)
        table = self._table[:n]
        if self.clahe is None:
            check(_lib.lib().embnet_augment_params(self.records.ctypes.data, self.n_ops, self.seed, int(batch_no), n, h, w,
                                                   ptr(table), stream()))
        else:
            check(_lib.lib().embnet_augment_params_clahe(self.records.ctypes.data, self.n_ops, self.clahe.ctypes.data,
                                                         self.clahe_pos, self.seed, int(batch_no), n, h, w, ptr(table), stream()))
        return table

    def _lut_buffer(self, n, device):
        """CLAHE's LUTs uint8 [n, gy, gx, 256]: a buffer kept like the parameter table (reused call after call on the current
        stream; kernels on one stream run in order, so a call's LUTs are read before the next call writes them)."""
        gx, gy = self.grid
        if self._luts is None or self._luts.shape[0] < n or self._luts.device != device:
            self._luts = torch.empty((max(n, 128), gy, gx, 256), device=device, dtype=torch.uint8)
        return self._luts[:n]

    def _clahe_luts(self, src_u8, index, n, table):
        _, h, w, c = src_u8.shape
        gx, gy = self.grid
        luts = self._lut_buffer(n, src_u8.device)
        check(_lib.lib().embnet_augment_clahe_luts(ptr(src_u8), ptr(index), n, h, w, c, gx, gy, ptr(table), ptr(luts), stream()))
        return luts

    def clahe_luts(self, src_u8, index, n, batch_no):
        """CLAHE's LUTs uint8 [n, gy, gx, 256] of batch `batch_no` (tests, debugging): zeros for the rows where CLAHE did not
        fire.  A view of the buffer the next call overwrites."""
        if self.clahe is None:
            raise ValueError("device augmentation: clahe_luts() needs a pipeline with clahe")
        _, h, w, c = src_u8.shape
        if self.hw != (h, w):
            self.check_shape(h, w, c)
        table = self.params(n, batch_no, (h, w))
        self._lut_buffer(n, src_u8.device).zero_()
        return self._clahe_luts(src_u8, index, n, table)

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
        if self.clahe is None:
            check(_lib.lib().embnet_augment_apply(ptr(src_u8), ptr(index), n, h, w, c, c_out, ptr(table), self.seed,
                                                  int(batch_no), ptr(out), stream()))
        else:
            luts = self._clahe_luts(src_u8, index, n, table)
            gx, gy = self.grid
            check(_lib.lib().embnet_augment_apply_clahe(ptr(src_u8), ptr(index), n, h, w, c, c_out, ptr(table), ptr(luts), gx, gy,
                                                        self.seed, int(batch_no), ptr(out), stream()))
        return out

    def __repr__(self):
        return f"DeviceAugment({self.ops!r}, seed={self.seed})"


def rank_seed(seed, rank):
    """The augmentation seed of a data-parallel rank: `seed` on rank 0, distinct streams on the others."""
    return (int(seed) ^ (int(rank) * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF
