#!/usr/bin/env python3
"""Device augmentation against the plain conversion it replaces (csrc/augment.hip vs embnet_u8_to_f32).

A batch of `--batch` images of `--image`^2 x 3 is gathered by index out of a uint8 store of `--store` random images resident in
HBM and converted to float32, by:
  u8_to_f32      embnet_u8_to_f32 (one kernel)
  default        DeviceAugment('default'): parameter kernel + apply kernel
  default_p1     the same ops with every probability forced to 1 (blur and noise on every image: the costliest per-pixel path)
  crop_flip      DeviceAugment('crop_flip'): random resized crop (bilinear) + horizontal flip
  default_clahe  DeviceAugment('default_clahe'): the reference's full pipeline, CLAHE included (parameter, LUT and apply kernels)
  default_clahe_p1  the same with every probability forced to 1 (CLAHE on every image)
  params_only    the parameter kernel alone (default_p1)
Legs alternate round by round after a warm-up; each timing is device events around `--reps` back-to-back calls.  Reported: the
median microseconds per batch, and achieved bytes/s against the algorithmic bytes (n*H*W*3 read + n*H*W*3*4 written).  A call
from Python costs host time too (two launches for an augmenting leg, three with CLAHE), so the per-kernel DEVICE times are also reported, from the
library's event trace (`*_kernel_us`: median over `--reps` traced calls, per kernel).
Prints one JSON object."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--store", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from embeddingnet_amd.augment import PRESETS, DeviceAugment
    from embeddingnet_amd.input_pipeline import u8_to_f32
    dev = torch.device("cuda:0")
    n, s = args.batch, args.image
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    store = torch.randint(0, 256, (args.store, s, s, 3), dtype=torch.uint8, device=dev, generator=g)
    index = torch.from_numpy(np.random.RandomState(0).choice(args.store, n, replace=False).astype(np.int32)).to(dev)
    out = torch.empty((n, s, s, 3), device=dev, dtype=torch.float32)
    p1 = [(name, dict(kw, p=1.0)) for name, kw in PRESETS["default"]]
    clahe_p1 = [(name, dict(kw, p=1.0)) for name, kw in PRESETS["default_clahe"]]
    augs = {"default": DeviceAugment.from_config("default", [s, s, 3]), "default_p1": DeviceAugment(p1),
            "crop_flip": DeviceAugment.from_config("crop_flip", [s, s, 3]),
            "default_clahe": DeviceAugment.from_config("default_clahe", [s, s, 3]), "default_clahe_p1": DeviceAugment(clahe_p1)}
    params_aug = augs["default_p1"]
    params_aug.check_shape(s, s)
    legs = {"u8_to_f32": lambda: u8_to_f32(store, index, n, out=out),
            "default": lambda: augs["default"].apply(store, index, n, out=out),
            "default_p1": lambda: augs["default_p1"].apply(store, index, n, out=out),
            "crop_flip": lambda: augs["crop_flip"].apply(store, index, n, out=out),
            "default_clahe": lambda: augs["default_clahe"].apply(store, index, n, out=out),
            "default_clahe_p1": lambda: augs["default_clahe_p1"].apply(store, index, n, out=out),
            "params_only": lambda: params_aug.params(n, 0)}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / args.reps

    for _ in range(args.warmup):
        for fn in legs.values():
            timed(fn)
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    nbytes = n * s * s * 3 * (1 + 4)
    res = {"batch": n, "image": s, "store_images": args.store, "rounds": args.rounds, "reps": args.reps,
           "algorithmic_bytes": nbytes, "device": torch.cuda.get_device_name(dev)}
    for k, v in times.items():
        med = float(np.median(v))
        res[f"{k}_us"] = round(med, 2)
        res[f"{k}_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        if k != "params_only":
            res[f"{k}_tb_per_s"] = round(nbytes / (med * 1e-6) / 1e12, 3)
    augmented = ("default", "default_p1", "crop_flip", "default_clahe", "default_clahe_p1")
    for k in augmented:
        res[f"{k}_over_u8_to_f32"] = round(res[f"{k}_us"] / res["u8_to_f32_us"], 3)
    from embeddingnet_amd import _lib
    for k, fn in legs.items():
        _lib.trace_enable(True)
        _lib.trace_reset()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        per = {}
        for name, ms, _, _, _ in _lib.trace_records():
            per.setdefault(name.split("::")[-1], []).append(1e3 * ms)
        _lib.trace_enable(False)
        res[f"{k}_kernel_us"] = {name: round(float(np.median(v)), 2) for name, v in per.items()}
    dev_us = {k: sum(res[f"{k}_kernel_us"].values()) for k in legs}
    for k in augmented:
        apply_us = res[f"{k}_kernel_us"].get("augment_apply_kernel", res[f"{k}_kernel_us"].get("augment_apply_clahe_kernel"))
        res[f"{k}_kernel_over_u8_to_f32"] = round(dev_us[k] / dev_us["u8_to_f32"], 3)
        res[f"{k}_apply_kernel_over_u8_to_f32"] = round(apply_us / dev_us["u8_to_f32"], 3)
    # CLAHE's LUT kernel against the apply kernel of default_p1 (the issue's target: at most that)
    for k in ("default_clahe", "default_clahe_p1"):
        res[f"{k}_lut_kernel_us"] = res[f"{k}_kernel_us"].get("augment_clahe_lut_kernel")
    res["clahe_p1_lut_over_default_p1_apply"] = round(res["default_clahe_p1_lut_kernel_us"] /
                                                      res["default_p1_kernel_us"]["augment_apply_kernel"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
