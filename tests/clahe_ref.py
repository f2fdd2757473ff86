"""NumPy mirror of CLAHE in csrc/augment.hip (include/embnet.h, "CLAHE"): the CLAHE draws of the parameter table, OpenCV's tile
histograms, clip, redistribution and LUTs (integers, and float32 where the kernel uses float32: the clip draw, lutScale, 1/tw and
the blend weights), the bilinear LUT blend, and a float64 pair of OpenCV's float Lab conversions for BGR images.  The ops before
and after CLAHE are augment_ref's."""
import numpy as np

import augment_ref as R

T_FIRED, T_CLIP, T_POS, T_GX, T_GY = 10, 11, 12, 13, 14
CLAHE_OP = 8                       # RNG op index of the CLAHE draws: b = 256 (fires), 257 (clip limit)
F32 = np.float32


def params(records, n_ops, clahe_rec, pos, seed, batch_no, n, h, w):
    """The table embnet_augment_params_clahe writes: augment_ref's table, then fields 10-14 of the rows where CLAHE fires."""
    t = R.params(records, n_ops, seed, batch_no, n, h, w)
    if clahe_rec is None:
        return t
    rec = np.asarray(clahe_rec, np.float32)
    a = np.uint64(batch_no) * np.uint64(65536) + np.arange(n, dtype=np.uint64)
    fire = R.unit24(R.rng_u32(seed, a, np.uint64(32 * CLAHE_OP))) < rec[1]
    clip = rec[2] + (rec[3] - rec[2]) * R.unit24(R.rng_u32(seed, a, np.uint64(32 * CLAHE_OP + 1)))
    t[fire, T_FIRED] += 1
    t[fire, T_CLIP] = clip[fire]
    t[fire, T_POS], t[fire, T_GX], t[fire, T_GY] = pos, rec[4], rec[5]
    return t


def tile_size(h, w, gx, gy):
    """(tw, th): both axes padded by g - size % g when either does not divide (OpenCV's quirk)."""
    pad = w % gx != 0 or h % gy != 0
    return (w + gx - w % gx if pad else w) // gx, (h + gy - h % gy if pad else h) // gy


def pad_image(a, gx, gy):
    """a [h, w, ...] padded at the bottom / right to the tile grid, reflect-101 (numpy's 'reflect')."""
    h, w = a.shape[:2]
    tw, th = tile_size(h, w, gx, gy)
    return np.pad(a, [(0, gy * th - h), (0, gx * tw - w)] + [(0, 0)] * (a.ndim - 2), mode="reflect")


def bins(l8):
    return np.rint(np.clip(l8, 0, 255)).astype(np.int64)


def tile_histograms(b, gx, gy):
    """int64 [gy, gx, 256]: the bins b [h, w] of the padded image counted per tile."""
    h, w = b.shape
    tw, th = tile_size(h, w, gx, gy)
    bp = pad_image(b, gx, gy)
    out = np.zeros((gy, gx, 256), np.int64)
    for ty in range(gy):
        for tx in range(gx):
            out[ty, tx] = np.bincount(bp[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256)
    return out


def clip_limit(clip_f32, total):
    return max(1, int(float(np.float32(clip_f32)) * total / 256))


def redistribute(hist, clip):
    """OpenCV: clip every bin at `clip`, add excess // 256 to every bin, then 1 to bins 0, step, 2 step, ... while the remainder
    lasts (step = max(256 // remainder, 1))."""
    hist = np.asarray(hist, np.int64)
    excess = int(np.maximum(hist - clip, 0).sum())
    out = np.minimum(hist, clip) + excess // 256
    resid = excess % 256
    if resid:
        step = max(256 // resid, 1)
        out[np.arange(0, 256, step)[:resid]] += 1
    return out


def lut(hist, clip, total):
    """uint8 [256]: saturate(rint(float32(cumsum) * (255.f / total))), round half even."""
    cum = np.cumsum(redistribute(hist, clip)).astype(np.float32)
    return np.clip(np.rint(cum * (F32(255) / F32(total))), 0, 255).astype(np.uint8)


def luts_from_bins(b, gx, gy, clip_f32):
    """uint8 [gy, gx, 256]: every tile's LUT from the bins b [h, w] of the image CLAHE sees."""
    h, w = b.shape
    tw, th = tile_size(h, w, gx, gy)
    hist = tile_histograms(b, gx, gy)
    c = clip_limit(clip_f32, tw * th)
    return np.stack([np.stack([lut(hist[ty, tx], c, tw * th) for tx in range(gx)]) for ty in range(gy)])


def blend(luts, b, dtype=np.float32):
    """[h, w]: OpenCV's bilinear blend of the four nearest tiles' LUTs at bins b [h, w], coordinates and weights in float32 (as the
    kernel), the blend itself in `dtype`."""
    gy, gx = luts.shape[:2]
    h, w = b.shape
    tw, th = tile_size(h, w, gx, gy)

    def axis(n, t, g):
        f = np.arange(n).astype(F32) * (F32(1) / F32(t)) - F32(0.5)
        i1 = np.floor(f).astype(np.int64)
        a = f - i1.astype(F32)
        return np.maximum(i1, 0), np.minimum(i1 + 1, g - 1), a.astype(dtype), (F32(1) - a).astype(dtype)

    tx1, tx2, xa, xa1 = axis(w, tw, gx)
    ty1, ty2, ya, ya1 = axis(h, th, gy)

    def at(ty, tx):
        return luts[ty[:, None], tx[None, :], b].astype(dtype)

    return ((at(ty1, tx1) * xa1[None] + at(ty1, tx2) * xa[None]) * ya1[:, None] +
            (at(ty2, tx1) * xa1[None] + at(ty2, tx2) * xa[None]) * ya[:, None])


# OpenCV's float Lab, D65, with the sRGB companding formula (float64 here)
M_XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
M_RGB = np.array([[3.240479, -1.53715, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])
XN, ZN = 0.950456, 1.088754


def _f(t):
    return np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16 / 116)


def bgr_to_lab(v):
    """float64 [..., 3] BGR on 0..255 -> (L* 255 / 100, a*, b*)."""
    c = np.asarray(v, np.float64)[..., ::-1] / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    xyz = lin @ M_XYZ.T
    x, y, z = xyz[..., 0] / XN, xyz[..., 1], xyz[..., 2] / ZN
    L = np.where(y > 0.008856, 116 * _f(y) - 16, 903.3 * y)
    return L * 255 / 100, 500 * (_f(x) - _f(y)), 200 * (_f(y) - _f(z))


def lab_to_bgr(L, a, b):
    """float64 L* (0..100), a*, b* -> BGR on 0..255 (linear clipped to [0, 1] before the companding, then clipped)."""
    low = L <= 0.008856 * 903.3
    y = np.where(low, L / 903.3, ((L + 16) / 116) ** 3)
    fy = np.where(low, 7.787 * (L / 903.3) + 16 / 116, (L + 16) / 116)

    def finv(f):
        return np.where(f <= 7.787 * 0.008856 + 16 / 116, (f - 16 / 116) / 7.787, f ** 3)

    rgb = np.clip(np.stack([finv(a / 500 + fy) * XN, y, finv(fy - b / 200) * ZN], -1) @ M_RGB.T, 0, 1)
    s = np.where(rgb <= 0.0031308, 12.92 * rgb, 1.055 * rgb ** (1 / 2.4) - 0.055)
    return np.clip(255 * s[..., ::-1], 0, 255)


def value(v):
    """What CLAHE equalises (0..255) of float64 pixels v [h, w, c]: the gray value, or L* 255 / 100 of the BGR pixel."""
    return v[..., 0] if v.shape[-1] == 1 else bgr_to_lab(v)[0]


def pixel_ops(v, t, i0, i1):
    """augment_ref's per-pixel ops of slots [i0, i1) of table row t on float64 pixels v [h, w, c] (0..255)."""
    c = v.shape[-1]
    for i in range(i0, i1):
        code, a0, a1, a2 = (float(x) for x in t[R.SLOTS + 4 * i: R.SLOTS + 4 * i + 4])
        if code == 6:
            v = np.clip(v * a0 + a1 * 255, 0, 255)
        elif code == 7:
            v = np.clip(255 * (v / 255) ** a0, 0, 255)
        elif code == 8 and c == 3:
            v = np.stack(R._hsv_shift(v[..., 0], v[..., 1], v[..., 2], a0, a1, a2), -1)
    return v


def before_clahe(img, t):
    """float64 [h, w, c] on 0..255: uint8 img through the geometry and the pixel ops before CLAHE (slots < pos) of row t."""
    g = np.array(t, np.float32)
    g[R.SLOTS:] = 0
    g[7] = 0
    v = R.apply_image(img, g) * 255.0          # augment_ref's geometry alone (v / 255 * 255: within an ulp)
    return pixel_ops(v, t, 0, int(t[T_POS]))


def luts(img, t):
    """uint8 [gy, gx, 256]: the LUTs of one image and table row t where CLAHE fired; also L8 [h, w] of the image it sees."""
    gx, gy = int(t[T_GX]), int(t[T_GY])
    l8 = value(before_clahe(img, t))
    return luts_from_bins(bins(l8), gx, gy, t[T_CLIP]), l8


def near_half(l8, window=1e-2):
    """bool [h, w]: L8 within `window` of a .5 bin boundary, where float32 and float64 may bin differently."""
    x = np.clip(l8, 0, 255)
    return np.abs(x - np.floor(x) - 0.5) < window


def apply_image(img, t, lut_bytes):
    """float64 [h, w, c] in [0, 1]: steps 1-3 of row t (no noise) with CLAHE from the given LUTs [gy, gx, 256] (the dumped ones)."""
    if t[T_CLIP] == 0:
        return R.apply_image(img, t)
    h, w, c = img.shape
    pos = int(t[T_POS])
    v = before_clahe(img, t)
    if c == 1:
        v = blend(lut_bytes, bins(v[..., 0]), np.float64)[..., None]
    else:
        l8, la, lb = bgr_to_lab(v)
        v = lab_to_bgr(blend(lut_bytes, bins(l8), np.float64) * 100 / 255, la, lb)
    v = pixel_ops(v, t, pos, 8)
    kb = int(t[7])
    if kb:
        rad = kb // 2
        pad = np.pad(v, ((rad, rad), (rad, rad), (0, 0)), mode="reflect")
        acc = np.zeros_like(v)
        for dy in range(kb):
            for dx in range(kb):
                acc += pad[dy:dy + h, dx:dx + w]
        v = np.clip(acc / (kb * kb), 0, 255)
    return v / 255.0


def gray(img, gx, gy, clip_f32):
    """CLAHE alone on a uint8 gray image [h, w] as the kernels compute it: (LUTs, float32 output in [0, 1])."""
    b = img.astype(np.int64)
    lut_bytes = luts_from_bins(b, gx, gy, clip_f32)
    return lut_bytes, blend(lut_bytes, b) / F32(255)
