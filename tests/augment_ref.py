"""NumPy mirror of csrc/augment.hip for the device-augmentation tests: the counter RNG, the parameter table (float32 and
integer fields reproduced operation for operation, the crop boxes in float64 as the kernel computes them) and a float64
reference of the apply kernel's steps 1-3 fed a dumped table (noise is checked statistically)."""
import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
F = 48
SLOTS = 16
K_A = np.uint64(0xD6E8FEB86659FD93)


def mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def rng_u32(seed, a, b):
    """csrc/common.h rng_u32: (mix64(mix64(seed ^ a * K) + b) >> 32), vectorised over a and b."""
    a = np.asarray(a, np.uint64)
    b = np.asarray(b, np.uint64)
    with np.errstate(over="ignore"):
        key = mix64(np.uint64(seed) ^ (a * K_A))
        return (mix64(key + b) >> np.uint64(32)).astype(np.uint32)


def unit24(r):
    return ((np.asarray(r, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def uniform_int(r, m):
    r = (np.asarray(r, np.uint32) >> np.uint32(8)).astype(np.uint64)
    return ((r * np.asarray(m, np.uint64)) >> np.uint64(24)).astype(np.int64)


def params(records, n_ops, seed, batch_no, n, h, w):
    """The table embnet_augment_params writes: float32 [n, 48]."""
    f32 = np.float32
    rows = np.arange(n, dtype=np.uint64)
    a = np.uint64(batch_no) * np.uint64(65536) + rows

    def draw(i, j):
        return rng_u32(seed, a, np.uint64(32 * i + j))

    t = np.zeros((n, F), np.float32)
    x0 = np.zeros(n, np.int64); y0 = np.zeros(n, np.int64)
    cw = np.full(n, w, np.int64); ch = np.full(n, h, np.int64)
    fired = np.zeros(n, np.int64)
    for i in range(n_ops):
        r = np.asarray(records[i], np.float32)
        code = int(r[0])
        fire = unit24(draw(i, 0)) < r[1]
        fired += fire
        s0 = np.zeros(n, np.float32); s1 = np.zeros(n, np.float32); s2 = np.zeros(n, np.float32)
        if code == 1:
            area = cw.astype(np.float64) * ch.astype(np.float64)
            slo, shi = np.float64(r[2]), np.float64(r[3])
            lrlo, lrhi = np.log(np.float64(r[4])), np.log(np.float64(r[5]))
            cw2 = np.zeros(n, np.int64); ch2 = np.zeros(n, np.int64); att = np.zeros(n, np.int64)
            for k in range(10):
                ua = (draw(i, 1 + 2 * k) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
                ur = (draw(i, 2 + 2 * k) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
                target = area * (slo + (shi - slo) * ua)
                aspect = np.exp(lrlo + (lrhi - lrlo) * ur)
                ww = np.rint(np.sqrt(target * aspect)).astype(np.int64)
                hh = np.rint(np.sqrt(target / aspect)).astype(np.int64)
                ok = (att == 0) & (ww > 0) & (ww <= cw) & (hh > 0) & (hh <= ch)
                cw2 = np.where(ok, ww, cw2); ch2 = np.where(ok, hh, ch2); att = np.where(ok, k + 1, att)
            oy = uniform_int(draw(i, 21), np.maximum(ch - ch2 + 1, 0))
            ox = uniform_int(draw(i, 22), np.maximum(cw - cw2 + 1, 0))
            in_ratio = cw.astype(np.float64) / ch.astype(np.float64)
            fb_w = np.where(in_ratio < np.float64(r[4]), cw, np.where(in_ratio > np.float64(r[5]),
                                                                     np.rint(ch * np.float64(r[5])).astype(np.int64), cw))
            fb_h = np.where(in_ratio < np.float64(r[4]), np.rint(cw / np.float64(r[4])).astype(np.int64), ch)
            fb = att == 0
            cw2 = np.where(fb, fb_w, cw2); ch2 = np.where(fb, fb_h, ch2)
            oy = np.where(fb, (ch - ch2) // 2, oy); ox = np.where(fb, (cw - cw2) // 2, ox)
            x0 = np.where(fire, x0 + ox, x0); y0 = np.where(fire, y0 + oy, y0)
            cw = np.where(fire, cw2, cw); ch = np.where(fire, ch2, ch)
            s0, s1, s2 = cw2.astype(f32), ch2.astype(f32), att.astype(f32)
        elif code == 2:
            cw2 = np.maximum(1, np.rint(cw * np.float64(r[2])).astype(np.int64))
            ch2 = np.maximum(1, np.rint(ch * np.float64(r[2])).astype(np.int64))
            x0 = np.where(fire, x0 + (cw - cw2) // 2, x0); y0 = np.where(fire, y0 + (ch - ch2) // 2, y0)
            cw = np.where(fire, cw2, cw); ch = np.where(fire, ch2, ch)
            s0, s1 = cw2.astype(f32), ch2.astype(f32)
        elif code == 3:
            t[:, 4] = np.where(fire, 1, t[:, 4])
        elif code == 4:
            t[:, 5] = np.where(fire, 1, t[:, 5])
        elif code == 5:
            s0 = uniform_int(draw(i, 1), 4).astype(f32)
            t[:, 6] = np.where(fire, s0, t[:, 6])
        elif code == 6:
            s0 = f32(1) + (-r[3] + f32(2) * r[3] * unit24(draw(i, 1)))
            s1 = -r[2] + f32(2) * r[2] * unit24(draw(i, 2))
        elif code == 7:
            s0 = (r[2] + (r[3] - r[2]) * unit24(draw(i, 1))) / f32(100)
        elif code == 8:
            s0 = -r[2] + f32(2) * r[2] * unit24(draw(i, 1))
            s1 = -r[3] + f32(2) * r[3] * unit24(draw(i, 2))
            s2 = -r[4] + f32(2) * r[4] * unit24(draw(i, 3))
        elif code == 9:
            kmax = max(3, (int(r[2]) - 1) // 2 * 2 + 1)
            s0 = (3 + 2 * uniform_int(draw(i, 1), (kmax - 3) // 2 + 1)).astype(f32)
            t[:, 7] = np.where(fire, s0, t[:, 7])
        elif code == 10:
            s1 = r[2] + (r[3] - r[2]) * unit24(draw(i, 1))
            s0 = np.sqrt(s1)
            t[:, 8] = np.where(fire, s0, t[:, 8])
            t[:, 9] = np.where(fire, 1, t[:, 9])
        slot = np.stack([np.full(n, code, f32), s0.astype(f32), s1.astype(f32), s2.astype(f32)], 1)
        t[:, SLOTS + 4 * i: SLOTS + 4 * i + 4] = np.where(fire[:, None], slot, 0)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = x0, y0, cw, ch
    t[:, 10] = fired
    return t


def _hsv_shift(b, g, r, dh, ds, dv):
    v = np.maximum(np.maximum(b, g), r)
    mn = np.minimum(np.minimum(b, g), r)
    d = v - mn
    s = np.where(v > 0, 255.0 * d / np.where(v > 0, v, 1), 0.0)
    dd = np.where(d > 0, d, 1)
    hh = np.where(v == r, 60 * (g - b) / dd, np.where(v == g, 120 + 60 * (b - r) / dd, 240 + 60 * (r - g) / dd))
    hh = np.where(d > 0, hh, 0.0)
    hh = np.where(hh < 0, hh + 360, hh)
    hh = hh * 0.5 + dh
    hh = hh - 180 * np.floor(hh / 180)
    hh = np.where(hh >= 180, hh - 180, hh)
    s = np.clip(s + ds, 0, 255)
    val = np.clip(v + dv, 0, 255)
    sf = s / 255
    h6 = hh / 30
    sec = np.floor(h6)
    f = h6 - sec
    p, q, u = val * (1 - sf), val * (1 - sf * f), val * (1 - sf * (1 - f))
    k = sec.astype(np.int64)
    rr = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [val, q, p, p, u], val)
    gg = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [u, val, val, q, p], p)
    bb = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [p, p, u, val, val], q)
    return np.clip(bb, 0, 255), np.clip(gg, 0, 255), np.clip(rr, 0, 255)


def apply_image(img, t):
    """float64 [h, w, c] in [0, 1]: one uint8 image [h, w, c] through steps 1-3 of the table row t (no noise)."""
    h, w, c = img.shape
    f32 = np.float32
    oy, ox = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    r = np.where(t[5] != 0, h - 1 - oy, oy)
    cc = np.where(t[4] != 0, w - 1 - ox, ox)
    k = int(t[6])
    if k == 1:
        r, cc = cc, w - 1 - r
    elif k == 2:
        r, cc = h - 1 - r, w - 1 - cc
    elif k == 3:
        r, cc = h - 1 - cc, r
    src = img.astype(np.float64)
    if t[0] == 0 and t[1] == 0 and t[2] == w and t[3] == h:
        v = src[r, cc]
    else:
        sx = (f32(t[0]) + (2 * cc + 1).astype(f32) * f32(t[2]) / f32(2 * w)) - f32(0.5)
        sy = (f32(t[1]) + (2 * r + 1).astype(f32) * f32(t[3]) / f32(2 * h)) - f32(0.5)
        fx0, fy0 = np.floor(sx), np.floor(sy)
        fx, fy = (sx - fx0).astype(np.float64)[..., None], (sy - fy0).astype(np.float64)[..., None]
        xa, xb = np.clip(fx0.astype(np.int64), 0, w - 1), np.clip(fx0.astype(np.int64) + 1, 0, w - 1)
        ya, yb = np.clip(fy0.astype(np.int64), 0, h - 1), np.clip(fy0.astype(np.int64) + 1, 0, h - 1)
        top = src[ya, xa] + fx * (src[ya, xb] - src[ya, xa])
        bot = src[yb, xa] + fx * (src[yb, xb] - src[yb, xa])
        v = np.clip(top + fy * (bot - top), 0, 255)
    for i in range(8):
        code, a0, a1, a2 = (float(x) for x in t[SLOTS + 4 * i: SLOTS + 4 * i + 4])
        if code == 6:
            v = np.clip(v * a0 + a1 * 255, 0, 255)
        elif code == 7:
            v = np.clip(255 * (v / 255) ** a0, 0, 255)
        elif code == 8 and c == 3:
            b, g, rr = _hsv_shift(v[..., 0], v[..., 1], v[..., 2], a0, a1, a2)
            v = np.stack([b, g, rr], -1)
    kb = int(t[7])
    if kb:
        rad = kb // 2
        pad = np.pad(v, ((rad, rad), (rad, rad), (0, 0)), mode="reflect")     # numpy 'reflect' = OpenCV reflect-101
        acc = np.zeros_like(v)
        for dy in range(kb):
            for dx in range(kb):
                acc += pad[dy:dy + h, dx:dx + w]
        v = np.clip(acc / (kb * kb), 0, 255)
    return v / 255.0
