// Seeded on-device image augmentation for triplet training batches: the augmenting form of embnet_u8_to_f32 (image_input.hip).
// The reference's pipelines are albumentations Compose lists applied on the host per image (embedding_net/augmentations.py);
// here a batch is augmented where it already lives — in the uint8 HBM store or a staged uint8 batch — in the one pass that
// gathers and converts it, so the store path stays one read of 1 byte and one write of 4 bytes per value.
//
// Two kernels:
//   augment_params_kernel  one thread per image: draws every op's "does it fire" and parameters into table[n][AUG_F] from the
//                          counter RNG rng_u32(seed, a, b) (common.h), a = batch_no * 65536 + row, b = 32 * op + draw.  A row's
//                          draws depend on (seed, batch_no, row) only — not on n, nor on which thread issued the batch.
//   augment_apply_kernel   one workgroup per 32 x 32 output tile of one image (every per-image branch is workgroup-uniform):
//                          geometry (one output -> source map, bilinear), the per-pixel ops in list order, an optional k x k box
//                          blur over an LDS tile with its halo, Gaussian noise, then v / 255.f.  Float32 on the 0..255 scale,
//                          clipped to [0, 255] after every op, no rounding between ops.
// CLAHE (OpenCV's contrast-limited adaptive histogram equalisation) needs the histogram of every tile of the image as it stands
// before it, so it adds a kernel and keeps out of the 8 op slots:
//   augment_params_clahe_kernel  the parameter row above, then the CLAHE draws (RNG op index 8) into fields 10-14
//   augment_clahe_lut_kernel     one workgroup per (tile, image): recomputes geometry + the pixel ops before CLAHE for the
//                                tile's pixels, counts their bins in per-wave LDS histograms, and one wave turns the histogram
//                                into the tile's 256 LUT bytes
//   augment_apply_kernel<..., CLAHE = true>  (traced as augment_apply_clahe_kernel) the apply kernel with the CLAHE stage
//                                between the pixel ops before and after it
// The table layout, the op records and the RNG counters are documented in include/embnet.h ("Device augmentation").
#include "common.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr int AUG_F = 48;            // floats per image in the parameter table
constexpr int AUG_MAX_OPS = 8;
constexpr int AUG_REC = 8;           // floats per op record: opcode, p, four parameters, two unused
constexpr int AUG_TILE = 32;         // output tile edge
constexpr int AUG_HALO = 3;          // blur k <= 7
constexpr int AUG_LT = AUG_TILE + 2 * AUG_HALO;   // 38: LDS tile edge with the halo
constexpr uint64_t AUG_NOISE_B0 = 1ull << 32;     // first RNG counter `b` of the noise draws (parameter draws use b < 258)
constexpr int AUG_CLAHE_OP = AUG_MAX_OPS;         // RNG op index of the CLAHE draws (b = 256, 257): no slot uses it
constexpr int AUG_CLAHE_MAX_GRID = 16;

enum : int {
  AUG_RRC = 1, AUG_CENTER_CROP = 2, AUG_HFLIP = 3, AUG_VFLIP = 4, AUG_ROT90 = 5,
  AUG_BRIGHTNESS_CONTRAST = 6, AUG_GAMMA = 7, AUG_HSV = 8, AUG_BLUR = 9, AUG_GAUSS_NOISE = 10, AUG_CLAHE = 11,
};
// table fields
enum : int {
  T_X0 = 0, T_Y0 = 1, T_CW = 2, T_CH = 3, T_HFLIP = 4, T_VFLIP = 5, T_ROT = 6, T_BLUR_K = 7, T_NOISE_SIGMA = 8,
  T_NOISE_ON = 9, T_FIRED = 10, T_CLAHE_CLIP = 11, T_CLAHE_POS = 12, T_CLAHE_GX = 13, T_CLAHE_GY = 14, T_SLOTS = 16,
};

struct AugOps {
  float rec[AUG_MAX_OPS * AUG_REC];
  int n_ops;
};

// the top 24 bits of one draw as a float in [0, 1): exact
__host__ __device__ __forceinline__ float unit24(uint32_t r) { return (float)(r >> 8) * 5.9604644775390625e-8f; }
// an integer uniform in [0, m): exact (the top 24 bits scaled in 64-bit integer arithmetic)
__host__ __device__ __forceinline__ int uniform_int(uint32_t r, int m) { return (int)(((uint64_t)(r >> 8) * (uint64_t)m) >> 24); }

// One row of the table (host and device: the same code checks on the CPU what the kernel draws).
__host__ __device__ inline void augment_params_row(const AugOps& ops, uint64_t seed, uint64_t batch_no, int row, int h, int w,
                                                   float* __restrict__ table) {
#pragma clang fp contract(off)
  const uint64_t a = batch_no * 65536ull + (uint64_t)row;
  const uint64_t key = mix64(seed ^ (a * 0xD6E8FEB86659FD93ull));       // rng_u32(seed, a, b) = mix64(key + b) >> 32
  auto draw = [&](int op, int j) { return (uint32_t)(mix64(key + (uint64_t)(32 * op + j)) >> 32); };
  float* trow = table + (long)row * AUG_F;
  float hflip = 0.f, vflip = 0.f, rot = 0.f, blur_k = 0.f, sigma = 0.f, noise_on = 0.f;
  int x0 = 0, y0 = 0, cw = w, ch = h, fired = 0;
  for (int i = 0; i < ops.n_ops; ++i) {
    const float* r = ops.rec + i * AUG_REC;
    const int code = (int)r[0];
    if (!(unit24(draw(i, 0)) < r[1])) {
      reinterpret_cast<float4*>(trow)[T_SLOTS / 4 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    ++fired;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (code == AUG_RRC) {
      // torchvision RandomResizedCrop.get_params inside the current box, in double as torchvision's Python floats:
      // 10 attempts of (area fraction, log aspect ratio), then the centre-crop fallback
      const double area = (double)cw * (double)ch, slo = r[2], shi = r[3], lrlo = log((double)r[4]), lrhi = log((double)r[5]);
      int cw2 = 0, ch2 = 0, attempt = 0;
      for (int k = 0; k < 10 && !attempt; ++k) {
        const double ua = (double)(draw(i, 1 + 2 * k) >> 8) * 5.9604644775390625e-8;
        const double ur = (double)(draw(i, 2 + 2 * k) >> 8) * 5.9604644775390625e-8;
        const double target = area * (slo + (shi - slo) * ua);
        const double aspect = exp(lrlo + (lrhi - lrlo) * ur);
        const int ww = (int)rint(sqrt(target * aspect)), hh = (int)rint(sqrt(target / aspect));
        if (ww > 0 && ww <= cw && hh > 0 && hh <= ch) { cw2 = ww; ch2 = hh; attempt = k + 1; }
      }
      int oy, ox;
      if (attempt) {
        oy = uniform_int(draw(i, 21), ch - ch2 + 1);
        ox = uniform_int(draw(i, 22), cw - cw2 + 1);
      } else {
        const double in_ratio = (double)cw / (double)ch;
        if (in_ratio < (double)r[4]) { cw2 = cw; ch2 = (int)rint((double)cw2 / (double)r[4]); }
        else if (in_ratio > (double)r[5]) { ch2 = ch; cw2 = (int)rint((double)ch2 * (double)r[5]); }
        else { cw2 = cw; ch2 = ch; }
        oy = (ch - ch2) / 2;
        ox = (cw - cw2) / 2;
      }
      x0 += ox; y0 += oy; cw = cw2; ch = ch2;
      s0 = (float)cw2; s1 = (float)ch2; s2 = (float)attempt;
    } else if (code == AUG_CENTER_CROP) {
      int cw2 = (int)rint((double)cw * (double)r[2]), ch2 = (int)rint((double)ch * (double)r[2]);
      cw2 = cw2 < 1 ? 1 : cw2;
      ch2 = ch2 < 1 ? 1 : ch2;
      x0 += (cw - cw2) / 2; y0 += (ch - ch2) / 2; cw = cw2; ch = ch2;
      s0 = (float)cw2; s1 = (float)ch2;
    } else if (code == AUG_HFLIP) {
      hflip = 1.f;
    } else if (code == AUG_VFLIP) {
      vflip = 1.f;
    } else if (code == AUG_ROT90) {
      s0 = (float)uniform_int(draw(i, 1), 4);
      rot = s0;
    } else if (code == AUG_BRIGHTNESS_CONTRAST) {      // alpha = 1 + U(-c, c), beta = U(-b, b)
      s0 = 1.f + (-r[3] + 2.f * r[3] * unit24(draw(i, 1)));
      s1 = -r[2] + 2.f * r[2] * unit24(draw(i, 2));
    } else if (code == AUG_GAMMA) {                    // gamma = U(lo, hi) / 100
      s0 = (r[2] + (r[3] - r[2]) * unit24(draw(i, 1))) / 100.f;
    } else if (code == AUG_HSV) {                      // hue, saturation, value shifts U(-limit, limit)
      s0 = -r[2] + 2.f * r[2] * unit24(draw(i, 1));
      s1 = -r[3] + 2.f * r[3] * unit24(draw(i, 2));
      s2 = -r[4] + 2.f * r[4] * unit24(draw(i, 3));
    } else if (code == AUG_BLUR) {                     // odd k uniform in [3, max(3, blur_limit)]
      const int kodd = ((int)r[2] - 1) / 2 * 2 + 1, kmax = kodd < 3 ? 3 : kodd;
      s0 = (float)(3 + 2 * uniform_int(draw(i, 1), (kmax - 3) / 2 + 1));
      blur_k = s0;
    } else if (code == AUG_GAUSS_NOISE) {              // sigma = sqrt(U(var_lo, var_hi))
      s1 = r[2] + (r[3] - r[2]) * unit24(draw(i, 1));
      s0 = sqrtf(s1);
      sigma = s0;
      noise_on = 1.f;
    }
    reinterpret_cast<float4*>(trow)[T_SLOTS / 4 + i] = make_float4((float)code, s0, s1, s2);
  }
  float4* t4 = reinterpret_cast<float4*>(trow);
  t4[0] = make_float4((float)x0, (float)y0, (float)cw, (float)ch);
  t4[1] = make_float4(hflip, vflip, rot, blur_k);
  t4[2] = make_float4(sigma, noise_on, (float)fired, 0.f);
  t4[3] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = ops.n_ops; i < AUG_MAX_OPS; ++i) t4[T_SLOTS / 4 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(256) void augment_params_kernel(AugOps ops, uint64_t seed, uint64_t batch_no, int n, int h, int w,
                                                             float* __restrict__ table) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row < n) augment_params_row(ops, seed, batch_no, row, h, w, table);
}

// The CLAHE record { AUG_CLAHE, p, clip lo, clip hi, gx, gy, 0, 0 } (checked on the host) and pos, the number of other ops
// listed before it.
struct AugClahe {
  float p, lo, hi;
  int gx, gy, pos;
};

// CLAHE's draws for a row that augment_params_row has written (host and device).  Fields 10-14 change only when it fires, so a
// row where it did not is, bit for bit, the row of the list without it.
__host__ __device__ inline void augment_clahe_row(const AugClahe& c, uint64_t seed, uint64_t batch_no, int row,
                                                  float* __restrict__ table) {
#pragma clang fp contract(off)
  const uint64_t a = batch_no * 65536ull + (uint64_t)row;
  const uint64_t key = mix64(seed ^ (a * 0xD6E8FEB86659FD93ull));
  auto draw = [&](int j) { return (uint32_t)(mix64(key + (uint64_t)(32 * AUG_CLAHE_OP + j)) >> 32); };
  if (!(unit24(draw(0)) < c.p)) return;
  float* trow = table + (long)row * AUG_F;
  trow[T_FIRED] += 1.f;
  trow[T_CLAHE_CLIP] = c.lo + (c.hi - c.lo) * unit24(draw(1));
  trow[T_CLAHE_POS] = (float)c.pos;
  trow[T_CLAHE_GX] = (float)c.gx;
  trow[T_CLAHE_GY] = (float)c.gy;
}

__global__ __launch_bounds__(256) void augment_params_clahe_kernel(AugOps ops, AugClahe clahe, uint64_t seed, uint64_t batch_no,
                                                                   int n, int h, int w, float* __restrict__ table) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row < n) {
    augment_params_row(ops, seed, batch_no, row, h, w, table);
    augment_clahe_row(clahe, seed, batch_no, row, table);
  }
}

__device__ __forceinline__ float clip255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

// OpenCV's float HSV with 8-bit ranges (H in [0, 180), S and V in [0, 255]) on a BGR pixel, shifted, and back
__device__ __forceinline__ void hsv_shift(float& b, float& g, float& r, float dh, float ds, float dv) {
  const float v = fmaxf(fmaxf(b, g), r), mn = fminf(fminf(b, g), r), d = v - mn;
  float s = v > 0.f ? 255.f * d / v : 0.f;
  float hh = 0.f;
  if (d > 0.f) {
    hh = v == r ? 60.f * (g - b) / d : (v == g ? 120.f + 60.f * (b - r) / d : 240.f + 60.f * (r - g) / d);
    if (hh < 0.f) hh += 360.f;
  }
  hh = hh * 0.5f + dh;
  hh = hh - 180.f * floorf(hh / 180.f);
  if (hh >= 180.f) hh -= 180.f;
  s = clip255(s + ds);
  const float val = clip255(v + dv);
  const float sf = s / 255.f, h6 = hh / 30.f;
  const float sec = floorf(h6), f = h6 - sec;
  const float p = val * (1.f - sf), q = val * (1.f - sf * f), u = val * (1.f - sf * (1.f - f));
  const int k = (int)sec;
  float rr, gg, bb;
  if (k == 0) { rr = val; gg = u; bb = p; }
  else if (k == 1) { rr = q; gg = val; bb = p; }
  else if (k == 2) { rr = p; gg = val; bb = u; }
  else if (k == 3) { rr = p; gg = q; bb = val; }
  else if (k == 4) { rr = u; gg = p; bb = val; }
  else { rr = val; gg = p; bb = q; }
  b = clip255(bb); g = clip255(gg); r = clip255(rr);
}

// OpenCV's float Lab (D65 white Xn = 0.950456, Zn = 1.088754) of a BGR pixel on the 0..255 scale, with the sRGB companding
// formula: l8 = L* 255 / 100, la = a*, lb = b*.  (OpenCV's float path interpolates the companding from a table; the formula is
// the definition here.)
constexpr float LAB_T = 0.008856f, LAB_K = 7.787f, LAB_B = 16.f / 116.f, LAB_KAPPA = 903.3f;
__device__ __forceinline__ float srgb_to_linear(float c) { return c <= 0.04045f ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f); }
__device__ __forceinline__ float linear_to_srgb(float c) { return c <= 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.f / 2.4f) - 0.055f; }
__device__ __forceinline__ float lab_f(float t) { return t > LAB_T ? cbrtf(t) : LAB_K * t + LAB_B; }
__device__ __forceinline__ float lab_f_inv(float f) { return f <= LAB_K * LAB_T + LAB_B ? (f - LAB_B) / LAB_K : f * f * f; }

__device__ __forceinline__ void bgr_to_lab(const float* v, float& l8, float& la, float& lb) {
#pragma clang fp contract(off)
  const float b = srgb_to_linear(v[0] / 255.f), g = srgb_to_linear(v[1] / 255.f), r = srgb_to_linear(v[2] / 255.f);
  const float x = (float)(0.412453 / 0.950456) * r + (float)(0.357580 / 0.950456) * g + (float)(0.180423 / 0.950456) * b;
  const float y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
  const float z = (float)(0.019334 / 1.088754) * r + (float)(0.119193 / 1.088754) * g + (float)(0.950227 / 1.088754) * b;
  const float fx = lab_f(x), fy = lab_f(y), fz = lab_f(z);
  l8 = (y > LAB_T ? 116.f * fy - 16.f : LAB_KAPPA * y) * (255.f / 100.f);
  la = 500.f * (fx - fy);
  lb = 200.f * (fy - fz);
}

// ... and back: L* (0..100), a*, b* -> BGR on the 0..255 scale (linear values clipped to [0, 1] before the companding)
__device__ __forceinline__ void lab_to_bgr(float l, float la, float lb, float* v) {
#pragma clang fp contract(off)
  float y, fy;
  if (l <= LAB_T * LAB_KAPPA) { y = l / LAB_KAPPA; fy = LAB_K * y + LAB_B; }
  else { fy = (l + 16.f) / 116.f; y = fy * fy * fy; }
  const float x = lab_f_inv(la / 500.f + fy) * 0.950456f, z = lab_f_inv(fy - lb / 200.f) * 1.088754f;
  const float r = 3.240479f * x - 1.53715f * y - 0.498535f * z;
  const float g = -0.969256f * x + 1.875991f * y + 0.041556f * z;
  const float b = 0.055648f * x - 0.204043f * y + 1.057311f * z;
  v[0] = clip255(255.f * linear_to_srgb(fminf(fmaxf(b, 0.f), 1.f)));
  v[1] = clip255(255.f * linear_to_srgb(fminf(fmaxf(g, 0.f), 1.f)));
  v[2] = clip255(255.f * linear_to_srgb(fminf(fmaxf(r, 0.f), 1.f)));
}

// The value CLAHE equalises, on the 0..255 scale: the gray value, or L* 255 / 100 of the BGR pixel (la, lb: its a*, b*)
template <int CI>
__device__ __forceinline__ float clahe_value(const float* v, float& la, float& lb) {
  if (CI == 3) {
    float l8;
    bgr_to_lab(v, l8, la, lb);
    return l8;
  }
  la = lb = 0.f;
  return v[0];
}
__device__ __forceinline__ int clahe_bin(float l8) { return (int)rintf(fminf(fmaxf(l8, 0.f), 255.f)); }

// OpenCV pads an image whose w % gx or h % gy is non-zero on BOTH axes (bottom / right, reflect-101) by g - size % g pixels, so
// an axis that divides evenly gains a full g; the tiles are then padded_w / gx x padded_h / gy.
__host__ __device__ __forceinline__ void clahe_tile(int h, int w, int gx, int gy, int& tw, int& th) {
  const bool pad = w % gx != 0 || h % gy != 0;
  tw = (pad ? w + gx - w % gx : w) / gx;
  th = (pad ? h + gy - h % gy : h) / gy;
}

// Per-image constants of the CLAHE stage (one image per workgroup)
struct AugClaheImage {
  const unsigned char* lut;          // this image's LUTs [gy][gx][256]
  int on, pos, gx, gy;
  float inv_tw, inv_th;
};

// The CLAHE stage on one pixel at output (y, x): OpenCV's bilinear blend of the four nearest tiles' LUTs at the pixel's bin,
// kept as a float; for BGR put back as L* with the pixel's own a*, b*.
template <int CI>
__device__ __forceinline__ void aug_clahe(const AugClaheImage& c, int y, int x, float* v) {
#pragma clang fp contract(off)
  float la, lb;
  const int bin = clahe_bin(clahe_value<CI>(v, la, lb));
  const float txf = (float)x * c.inv_tw - 0.5f, tyf = (float)y * c.inv_th - 0.5f;
  int tx1 = (int)floorf(txf), ty1 = (int)floorf(tyf);
  const float xa = txf - (float)tx1, ya = tyf - (float)ty1;
  const int tx2 = min(tx1 + 1, c.gx - 1), ty2 = min(ty1 + 1, c.gy - 1);
  tx1 = min(max(tx1, 0), c.gx - 1);            // (the upper clamp only matters for the unwritten pixels past the image)
  ty1 = min(max(ty1, 0), c.gy - 1);
  const unsigned char* l1 = c.lut + ty1 * c.gx * 256 + bin;
  const unsigned char* l2 = c.lut + ty2 * c.gx * 256 + bin;
  const float xa1 = 1.f - xa, ya1 = 1.f - ya;
  const float res = ((float)l1[tx1 * 256] * xa1 + (float)l1[tx2 * 256] * xa) * ya1 +
                    ((float)l2[tx1 * 256] * xa1 + (float)l2[tx2 * 256] * xa) * ya;
  if (CI == 3) lab_to_bgr(res * (100.f / 255.f), la, lb, v);
  else v[0] = res;
}

// Per-image constants of the apply kernel, read once from the table row (scalar loads: one image per workgroup).
struct AugImage {
  float x0, y0, cw, ch;
  int hflip, vflip, rot, blur_k, noise_on, crop;
  float sigma;
};

// Step 1 for output pixel (oy, ox): v[] = its CI channels on the 0..255 scale.
template <int CI>
__device__ __forceinline__ void aug_geometry(const unsigned char* __restrict__ s, const AugImage& g, int h, int w, int oy, int ox,
                                             float* v) {
  // undo the flips, then the rotation (square images): (r, c) in the resized crop
  int r = g.vflip ? h - 1 - oy : oy, c = g.hflip ? w - 1 - ox : ox;
  if (g.rot == 1) { const int t = r; r = c; c = w - 1 - t; }              // np.rot90(img, 1)[i, j] = img[j, S-1-i]
  else if (g.rot == 2) { r = h - 1 - r; c = w - 1 - c; }
  else if (g.rot == 3) { const int t = r; r = h - 1 - c; c = t; }          // np.rot90(img, 3)[i, j] = img[S-1-j, i]
  if (!g.crop) {                                                           // an integer map: one texel, exactly
    const unsigned char* p = s + ((long)r * w + c) * CI;
#pragma unroll
    for (int j = 0; j < CI; ++j) v[j] = (float)p[j];
  } else {
    // half-pixel centres: source x = x0 + (2c + 1) cw / (2W) - 0.5, clamped bilinear
    float sx, sy;
    {
#pragma clang fp contract(off)
      sx = g.x0 + (float)(2 * c + 1) * g.cw / (float)(2 * w) - 0.5f;
      sy = g.y0 + (float)(2 * r + 1) * g.ch / (float)(2 * h) - 0.5f;
    }
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    const float fx = sx - fx0, fy = sy - fy0;
    const int xa = min(max((int)fx0, 0), w - 1), xb = min(max((int)fx0 + 1, 0), w - 1);
    const int ya = min(max((int)fy0, 0), h - 1), yb = min(max((int)fy0 + 1, 0), h - 1);
    const unsigned char* p00 = s + ((long)ya * w + xa) * CI;
    const unsigned char* p01 = s + ((long)ya * w + xb) * CI;
    const unsigned char* p10 = s + ((long)yb * w + xa) * CI;
    const unsigned char* p11 = s + ((long)yb * w + xb) * CI;
#pragma unroll
    for (int j = 0; j < CI; ++j) {
      const float top = (float)p00[j] + fx * ((float)p01[j] - (float)p00[j]);
      const float bot = (float)p10[j] + fx * ((float)p11[j] - (float)p10[j]);
      v[j] = clip255(top + fy * (bot - top));
    }
  }
}

// Step 2 on NP pixels: the per-pixel ops of the table's slots [i0, i1) in list order (slot opcode 0: did not fire / not a pixel
// op).  CLAHE splits the slots at its position.
template <int CI, int NP>
__device__ __forceinline__ void aug_pixel_ops(const float* __restrict__ tp, float (&v)[NP][CI], int i0 = 0, int i1 = AUG_MAX_OPS) {
  for (int i = i0; i < i1; ++i) {
    const int code = (int)tp[T_SLOTS + 4 * i];
    const float a0 = tp[T_SLOTS + 4 * i + 1], a1 = tp[T_SLOTS + 4 * i + 2], a2 = tp[T_SLOTS + 4 * i + 3];
    if (code == AUG_BRIGHTNESS_CONTRAST) {
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int j = 0; j < CI; ++j) v[p][j] = clip255(v[p][j] * a0 + a1 * 255.f);
    } else if (code == AUG_GAMMA) {
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int j = 0; j < CI; ++j) v[p][j] = clip255(255.f * __powf(v[p][j] / 255.f, a0));
    } else if (code == AUG_HSV) {
      if (CI == 3) {
#pragma unroll
        for (int p = 0; p < NP; ++p) hsv_shift(v[p][0], v[p][1], v[p][CI - 1], a0, a1, a2);
      }
    }
  }
}

// Gaussian noise on element e = (oy * W + ox) * CI + j of an image: a Box-Muller pair per even/odd element pair,
//   u1 = (top 24 bits of rng_u32(seed, a, AUG_NOISE_B0 + e_even) + 1) / 2^24 in (0, 1],
//   u2 = top 24 bits of rng_u32(seed, a, AUG_NOISE_B0 + e_even + 1) / 2^24,
//   z(e_even) = sqrt(-2 ln u1) cos(2 pi u2),  z(e_even + 1) = sqrt(-2 ln u1) sin(2 pi u2)
// (a = batch_no * 65536 + row, key = mix64(seed ^ a * K): the first half of rng_u32, per image).
__device__ __forceinline__ void noise_pair(uint64_t key, uint64_t e_even, float& z0, float& z1) {
  const uint32_t r1 = (uint32_t)(mix64(key + AUG_NOISE_B0 + e_even) >> 32);
  const uint32_t r2 = (uint32_t)(mix64(key + AUG_NOISE_B0 + e_even + 1) >> 32);
  const float u1 = (float)((r1 >> 8) + 1u) * 5.9604644775390625e-8f, u2 = unit24(r2);
  const float rad = sqrtf(-2.f * __logf(u1));
  float sn, cs;
  __sincosf(6.28318530717958647692f * u2, &sn, &cs);
  z0 = rad * cs;
  z1 = rad * sn;
}

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// The per-image constants for the CLAHE LUT kernel: the same loads as augment_apply_kernel's, which keeps its own inline copy so
// that its instantiations without CLAHE compile to the code they compiled to before CLAHE was added.
__device__ __forceinline__ AugImage aug_image(const float* __restrict__ tp, int h, int w) {
  AugImage g;
  g.x0 = tp[T_X0]; g.y0 = tp[T_Y0]; g.cw = tp[T_CW]; g.ch = tp[T_CH];
  g.hflip = tp[T_HFLIP] != 0.f; g.vflip = tp[T_VFLIP] != 0.f; g.rot = h == w ? ((int)tp[T_ROT] & 3) : 0;   // (never off the image)
  g.blur_k = (int)tp[T_BLUR_K]; g.noise_on = tp[T_NOISE_ON] != 0.f; g.sigma = tp[T_NOISE_SIGMA];
  g.crop = !(g.x0 == 0.f && g.y0 == 0.f && g.cw == (float)w && g.ch == (float)h);
  return g;
}

// Step 2 with the CLAHE stage at the pixels' output coordinates (c.on: CLAHE fired for this image)
template <int CI, int NP>
__device__ __forceinline__ void aug_pixel_stage(const float* __restrict__ tp, const AugClaheImage& c, const int (&ys)[NP],
                                                const int (&xs)[NP], float (&v)[NP][CI]) {
  if (c.on) {
    aug_pixel_ops<CI, NP>(tp, v, 0, c.pos);
#pragma unroll
    for (int p = 0; p < NP; ++p) aug_clahe<CI>(c, ys[p], xs[p], v[p]);
    aug_pixel_ops<CI, NP>(tp, v, c.pos, AUG_MAX_OPS);
  } else {
    aug_pixel_ops<CI, NP>(tp, v);
  }
}

// One workgroup of 256 threads per 32 x 32 output tile; thread t owns the 4 pixels (ty + t / 8, tx + 4 (t % 8) + 0..3).
// VEC: W % 4 == 0 and 16-byte aligned dst: the 4 pixels' CO channels leave as CO float4 stores.  CLAHE: the CLAHE stage is
// compiled in (embnet_augment_apply_clahe, traced as augment_apply_clahe_kernel); without it luts, gx and gy are unused and the
// kernel is the one embnet_augment_apply has always launched.
template <int CI, int CO, bool VEC, bool CLAHE>
__global__ __launch_bounds__(256) void augment_apply_kernel(const unsigned char* __restrict__ src, const int* __restrict__ index,
                                                            int h, int w, int c_out_rt, const float* __restrict__ table,
                                                            uint64_t seed, uint64_t batch_no, float* __restrict__ dst,
                                                            const unsigned char* __restrict__ luts, int gx, int gy) {
  __shared__ float lds[CI][AUG_LT][AUG_LT + 1];
  const int img = blockIdx.y;
  const int tiles_x = (w + AUG_TILE - 1) / AUG_TILE;
  const int tx0 = (blockIdx.x % tiles_x) * AUG_TILE, ty0 = (blockIdx.x / tiles_x) * AUG_TILE;
  const float* tp = table + (long)img * AUG_F;
  AugImage g;
  g.x0 = tp[T_X0]; g.y0 = tp[T_Y0]; g.cw = tp[T_CW]; g.ch = tp[T_CH];
  g.hflip = tp[T_HFLIP] != 0.f; g.vflip = tp[T_VFLIP] != 0.f; g.rot = h == w ? ((int)tp[T_ROT] & 3) : 0;   // (never off the image)
  g.blur_k = (int)tp[T_BLUR_K]; g.noise_on = tp[T_NOISE_ON] != 0.f; g.sigma = tp[T_NOISE_SIGMA];
  g.crop = !(g.x0 == 0.f && g.y0 == 0.f && g.cw == (float)w && g.ch == (float)h);
  AugClaheImage c{};
  if constexpr (CLAHE) {
    c.on = tp[T_CLAHE_CLIP] != 0.f;
    c.pos = min(max((int)tp[T_CLAHE_POS], 0), AUG_MAX_OPS);
    c.gx = gx;
    c.gy = gy;
    int tw, th;
    clahe_tile(h, w, gx, gy, tw, th);
    c.inv_tw = 1.f / (float)tw;
    c.inv_th = 1.f / (float)th;
    c.lut = luts + (long)img * gy * gx * 256;
  }
  const unsigned char* s = src + (index ? (long)index[img] : (long)img) * h * w * CI;
  const int c_out = CO > 0 ? CO : c_out_rt;
  float* d = dst + (long)img * h * w * c_out;
  const int oy = ty0 + (int)threadIdx.x / 8, ox0 = tx0 + 4 * ((int)threadIdx.x % 8);

  float v[4][CI];
  if (g.blur_k) {
    // steps 1-2 over the tile and its halo (reflect-101 at the image border), then the k x k box from LDS
    for (int q = threadIdx.x; q < AUG_LT * AUG_LT; q += 256) {
      const int ly = q / AUG_LT, lx = q % AUG_LT;
      const int yy = reflect101(ty0 - AUG_HALO + ly, h), xx = reflect101(tx0 - AUG_HALO + lx, w);
      float u[1][CI];
      if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
        aug_geometry<CI>(s, g, h, w, yy, xx, u[0]);
        if constexpr (CLAHE) aug_pixel_stage<CI, 1>(tp, c, {yy}, {xx}, u);   // (a halo pixel gets CLAHE at its reflected coordinates)
        else aug_pixel_ops<CI, 1>(tp, u);
      } else {                                   // beyond the reflection (only past a partial tile's far edge): never read
#pragma unroll
        for (int j = 0; j < CI; ++j) u[0][j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < CI; ++j) lds[j][ly][lx] = u[0][j];
    }
    __syncthreads();
    const int k = g.blur_k, r = k / 2;
    const float inv = 1.f / (float)(k * k);
    const int ly = oy - ty0 + AUG_HALO, lx = ox0 - tx0 + AUG_HALO;
#pragma unroll
    for (int j = 0; j < CI; ++j) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int dy = -r; dy <= r; ++dy) {
        const float* row = &lds[j][ly + dy][lx - r];
        float win = 0.f;
        for (int dx = 0; dx < k; ++dx) win += row[dx];
        acc[0] += win;
#pragma unroll
        for (int p = 1; p < 4; ++p) { win += row[k - 1 + p] - row[p - 1]; acc[p] += win; }
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) v[p][j] = clip255(acc[p] * inv);
    }
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (oy < h && ox0 + p < w) aug_geometry<CI>(s, g, h, w, oy, ox0 + p, v[p]);
      else {
#pragma unroll
        for (int j = 0; j < CI; ++j) v[p][j] = 0.f;
      }
    }
    if constexpr (CLAHE) aug_pixel_stage<CI, 4>(tp, c, {oy, oy, oy, oy}, {ox0, ox0 + 1, ox0 + 2, ox0 + 3}, v);
    else aug_pixel_ops<CI, 4>(tp, v);
  }
  if (oy >= h) return;
  if (g.noise_on) {
    const uint64_t a = batch_no * 65536ull + (uint64_t)img;
    const uint64_t key = mix64(seed ^ (a * 0xD6E8FEB86659FD93ull));
    const uint64_t e0 = ((uint64_t)oy * w + ox0) * CI;
#pragma unroll
    for (int e = 0; e < 4 * CI; e += 2) {                  // (4 CI is even and e0 is even: the pairs stay in this thread)
      float z0, z1;
      noise_pair(key, e0 + e, z0, z1);
      v[e / CI][e % CI] = clip255(v[e / CI][e % CI] + g.sigma * z0);
      v[(e + 1) / CI][(e + 1) % CI] = clip255(v[(e + 1) / CI][(e + 1) % CI] + g.sigma * z1);
    }
  }
  if (VEC) {                                               // 4 pixels x CO channels = CO float4, 16-byte aligned
    float4* o = reinterpret_cast<float4*>(d + ((long)oy * w + ox0) * CO);
    if (ox0 < w) {
#pragma unroll
      for (int q = 0; q < CO; ++q) {
        float f[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int el = 4 * q + e, p = el / CO, j = el % CO;
          f[e] = j < CI ? v[p][j < CI ? j : 0] / 255.f : 0.f;
        }
        o[q] = make_float4(f[0], f[1], f[2], f[3]);
      }
    }
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (ox0 + p >= w) break;
      float* o = d + ((long)oy * w + ox0 + p) * c_out;
#pragma unroll
      for (int j = 0; j < CI; ++j) o[j] = v[p][j] / 255.f;
      for (int j = CI; j < c_out; ++j) o[j] = 0.f;
    }
  }
}

// One workgroup of 256 threads (4 waves) per (tile, image): the tile's pixels of the padded image through geometry and the pixel
// ops before CLAHE (the apply kernel's device code), their bins counted in one LDS histogram per wave (integer adds: the same
// counts every run; per wave, so a flat tile's pixels do not all queue on one address), then wave 0 sums the four, clips,
// redistributes, scans and writes the tile's 256 LUT bytes, one 32-bit word per lane.  OpenCV's CLAHE_CalcLut_Body.
template <int CI>
__global__ __launch_bounds__(256) void augment_clahe_lut_kernel(const unsigned char* __restrict__ src, const int* __restrict__ index,
                                                                int h, int w, int gx, int gy, const float* __restrict__ table,
                                                                unsigned char* __restrict__ luts) {
  __shared__ int hist[4][256];
  const int img = blockIdx.y, tx = (int)blockIdx.x % gx, ty = (int)blockIdx.x / gx;
  const float* tp = table + (long)img * AUG_F;
  const float clip_f = tp[T_CLAHE_CLIP];
  if (clip_f == 0.f) return;                         // CLAHE did not fire for this image (uniform over the workgroup)
  for (int i = threadIdx.x; i < 4 * 256; i += 256) (&hist[0][0])[i] = 0;
  __syncthreads();
  const AugImage g = aug_image(tp, h, w);
  const int pos = min(max((int)tp[T_CLAHE_POS], 0), AUG_MAX_OPS);
  const unsigned char* s = src + (index ? (long)index[img] : (long)img) * h * w * CI;
  int tw, th;
  clahe_tile(h, w, gx, gy, tw, th);
  int* my = hist[threadIdx.x / 64];
  for (int q = threadIdx.x; q < tw * th; q += 256) {
    const int py = ty * th + q / tw, px = tx * tw + q % tw;
    const int yy = py < h ? py : 2 * h - 2 - py, xx = px < w ? px : 2 * w - 2 - px;     // the reflect-101 pad (< h, w)
    float u[1][CI], la, lb;
    aug_geometry<CI>(s, g, h, w, yy, xx, u[0]);
    aug_pixel_ops<CI, 1>(tp, u, 0, pos);
    atomicAdd(&my[clahe_bin(clahe_value<CI>(u[0], la, lb))], 1);
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, total = tw * th;
  int hb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) hb[k] = hist[0][4 * lane + k] + hist[1][4 * lane + k] + hist[2][4 * lane + k] + hist[3][4 * lane + k];
  const int clip = max((int)((double)clip_f * (double)total / 256.0), 1);
  int excess = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (hb[k] > clip) { excess += hb[k] - clip; hb[k] = clip; }
  }
  for (int o = 32; o > 0; o >>= 1) excess += __shfl_xor(excess, o, 64);
  // excess / 256 to every bin, then one more to bins 0, step, 2 step, ... until the remainder is used up
  const int batch = excess / 256, resid = excess % 256, step = resid ? max(256 / resid, 1) : 1;
  int cum[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = 4 * lane + k;
    cum[k] = (k ? cum[k - 1] : 0) + hb[k] + batch + (resid != 0 && i % step == 0 && i / step < resid ? 1 : 0);
  }
  int run = cum[3];                                  // inclusive scan of the lanes' sums
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(run, o, 64);
    if (lane >= o) run += t;
  }
  const int base = run - cum[3];
  const float scale = 255.f / (float)total;
  uint32_t word = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) word |= (uint32_t)min(max((int)rintf((float)(base + cum[k]) * scale), 0), 255) << (8 * k);
  reinterpret_cast<uint32_t*>(luts + (((long)img * gy + ty) * gx + tx) * 256)[lane] = word;
}

// host-side validation of an op list (before any launch)
static int check_ops(const float* ops, int n_ops, int h, int w, AugOps& out) {
  EMBNET_CHECK_ARG(n_ops >= 0 && n_ops <= AUG_MAX_OPS, "augment: n_ops=%d (0..%d ops)", n_ops, AUG_MAX_OPS);
  EMBNET_CHECK_ARG(n_ops == 0 || ops, "augment: null pointer (ops)");
  int seen[16] = {0};
  for (int i = 0; i < AUG_MAX_OPS * AUG_REC; ++i) out.rec[i] = 0.f;
  out.n_ops = n_ops;
  for (int i = 0; i < n_ops; ++i) {
    const float* r = ops + i * AUG_REC;
    const float c = r[0], p = r[1];
    const int code = (int)c;
    EMBNET_CHECK_ARG(c == (float)code && code >= AUG_RRC && code <= AUG_GAUSS_NOISE, "augment: op %d: unknown opcode %g", i, c);
    EMBNET_CHECK_ARG(p >= 0.f && p <= 1.f, "augment: op %d: p=%g outside [0, 1]", i, p);
    const bool pixel_op = code == AUG_BRIGHTNESS_CONTRAST || code == AUG_GAMMA || code == AUG_HSV;
    EMBNET_CHECK_ARG(pixel_op || !seen[code], "augment: op %d: opcode %d appears twice (only per-pixel ops may repeat)", i, code);
    seen[code] = 1;
    switch (code) {
      case AUG_RRC:
        EMBNET_CHECK_ARG(r[2] > 0.f && r[2] <= r[3] && r[3] <= 1.f && r[4] > 0.f && r[4] <= r[5],
                         "augment: op %d: random_resized_crop scale=(%g, %g) ratio=(%g, %g) (0 < lo <= hi <= 1; 0 < lo <= hi)",
                         i, r[2], r[3], r[4], r[5]);
        break;
      case AUG_CENTER_CROP:
        EMBNET_CHECK_ARG(r[2] > 0.f && r[2] <= 1.f, "augment: op %d: center_crop frac=%g outside (0, 1]", i, r[2]);
        break;
      case AUG_ROT90:
        EMBNET_CHECK_ARG(h == w, "augment: op %d: random_rotate90 needs square images (h=%d w=%d)", i, h, w);
        break;
      case AUG_BRIGHTNESS_CONTRAST:
        EMBNET_CHECK_ARG(r[2] >= 0.f && r[3] >= 0.f, "augment: op %d: brightness_contrast limits (%g, %g) < 0", i, r[2], r[3]);
        break;
      case AUG_GAMMA:
        EMBNET_CHECK_ARG(r[2] > 0.f && r[2] <= r[3], "augment: op %d: gamma_limit=(%g, %g) (0 < lo <= hi)", i, r[2], r[3]);
        break;
      case AUG_HSV:
        EMBNET_CHECK_ARG(r[2] >= 0.f && r[3] >= 0.f && r[4] >= 0.f, "augment: op %d: hue_saturation_value limits < 0", i);
        break;
      case AUG_BLUR:
        EMBNET_CHECK_ARG(r[2] >= 1.f && r[2] <= 7.f && r[2] == (float)(int)r[2],
                         "augment: op %d: blur_limit=%g (an integer in 1..7)", i, r[2]);
        break;
      case AUG_GAUSS_NOISE:
        EMBNET_CHECK_ARG(r[2] >= 0.f && r[2] <= r[3], "augment: op %d: var_limit=(%g, %g) (0 <= lo <= hi)", i, r[2], r[3]);
        break;
      default: break;
    }
    for (int j = 0; j < AUG_REC; ++j) out.rec[i * AUG_REC + j] = r[j];
  }
  return EMBNET_OK;
}

// host-side validation of a CLAHE grid against the image size (the pad, at most g, stays below the image size)
static int check_clahe_grid(const char* what, int gx, int gy, int h, int w) {
  EMBNET_CHECK_ARG(gx >= 1 && gx <= AUG_CLAHE_MAX_GRID && gy >= 1 && gy <= AUG_CLAHE_MAX_GRID,
                   "%s: clahe tile_grid_size=(%d, %d) (1..%d each)", what, gx, gy, AUG_CLAHE_MAX_GRID);
  EMBNET_CHECK_ARG(2 * gx <= w && 2 * gy <= h, "%s: clahe tile_grid_size=(%d, %d) too large for %dx%d images (2 gx <= w, 2 gy <= h)",
                   what, gx, gy, h, w);
  return EMBNET_OK;
}

// host-side validation of a CLAHE record and its position in an op list of n_ops other ops (before any launch)
static int check_clahe(const float* r, int pos, int n_ops, int h, int w, AugClahe& out) {
  EMBNET_CHECK_ARG(r[0] == (float)AUG_CLAHE, "augment: clahe record: opcode %g (expected %d)", r[0], AUG_CLAHE);
  EMBNET_CHECK_ARG(r[1] >= 0.f && r[1] <= 1.f, "augment: clahe p=%g outside [0, 1]", r[1]);
  EMBNET_CHECK_ARG(r[2] > 0.f && r[2] <= r[3] && r[3] <= 3.0e38f, "augment: clahe clip_limit=(%g, %g) (0 < lo <= hi)", r[2], r[3]);
  EMBNET_CHECK_ARG(r[4] >= 1.f && r[4] <= (float)AUG_CLAHE_MAX_GRID && r[4] == (float)(int)r[4] && r[5] >= 1.f &&
                   r[5] <= (float)AUG_CLAHE_MAX_GRID && r[5] == (float)(int)r[5],
                   "augment: clahe tile_grid_size=(%g, %g) (integers in 1..%d)", r[4], r[5], AUG_CLAHE_MAX_GRID);
  const int rc = check_clahe_grid("augment", (int)r[4], (int)r[5], h, w);
  if (rc != EMBNET_OK) return rc;
  EMBNET_CHECK_ARG(pos >= 0 && pos <= n_ops, "augment: clahe pos=%d outside [0, n_ops=%d]", pos, n_ops);
  out = AugClahe{r[1], r[2], r[3], (int)r[4], (int)r[5], pos};
  return EMBNET_OK;
}

}  // namespace embnet

using namespace embnet;

extern "C" size_t embnet_augment_param_floats(void) { return AUG_F; }

extern "C" int embnet_augment_params(const float* ops, int n_ops, uint64_t seed, uint64_t batch_no, int n, int h, int w,
                                     float* table, void* stream) {
  EMBNET_CHECK_ARG(table, "augment_params: null pointer (table)");
  EMBNET_CHECK_ARG(n > 0 && n <= 65535 && h >= 4 && w >= 4 && h <= 16384 && w <= 16384,
                   "augment_params: n=%d h=%d w=%d (1 <= n <= 65535, 4 <= h, w <= 16384)", n, h, w);
  EMBNET_CHECK_ARG(((uintptr_t)table & 15) == 0, "augment_params: table not 16-byte aligned");
  AugOps rec;
  const int rc = check_ops(ops, n_ops, h, w, rec);
  if (rc != EMBNET_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  EMBNET_TRACE("embnet::augment_params_kernel", TRACE_BYTES, (double)n * AUG_F * 4.0, st);
  augment_params_kernel<<<cdiv(n, 256), 256, 0, st>>>(rec, seed, batch_no, n, h, w, table);
  return check_launch("augment_params");
}

extern "C" int embnet_augment_params_clahe(const float* ops, int n_ops, const float* clahe_rec, int clahe_pos, uint64_t seed,
                                           uint64_t batch_no, int n, int h, int w, float* table, void* stream) {
  if (!clahe_rec) return embnet_augment_params(ops, n_ops, seed, batch_no, n, h, w, table, stream);
  EMBNET_CHECK_ARG(table, "augment_params_clahe: null pointer (table)");
  EMBNET_CHECK_ARG(n > 0 && n <= 65535 && h >= 4 && w >= 4 && h <= 16384 && w <= 16384,
                   "augment_params_clahe: n=%d h=%d w=%d (1 <= n <= 65535, 4 <= h, w <= 16384)", n, h, w);
  EMBNET_CHECK_ARG(((uintptr_t)table & 15) == 0, "augment_params_clahe: table not 16-byte aligned");
  AugOps rec;
  int rc = check_ops(ops, n_ops, h, w, rec);
  if (rc != EMBNET_OK) return rc;
  AugClahe clahe;
  rc = check_clahe(clahe_rec, clahe_pos, n_ops, h, w, clahe);
  if (rc != EMBNET_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  EMBNET_TRACE("embnet::augment_params_clahe_kernel", TRACE_BYTES, (double)n * AUG_F * 4.0, st);
  augment_params_clahe_kernel<<<cdiv(n, 256), 256, 0, st>>>(rec, clahe, seed, batch_no, n, h, w, table);
  return check_launch("augment_params_clahe");
}

extern "C" size_t embnet_augment_clahe_lut_bytes(int n, int gx, int gy) {
  return n > 0 && gx > 0 && gy > 0 ? (size_t)n * (size_t)gy * (size_t)gx * 256u : 0;
}

extern "C" int embnet_augment_clahe_luts(const void* src, const int32_t* index, int n, int h, int w, int c_in, int gx, int gy,
                                         const float* table, void* luts, void* stream) {
  EMBNET_CHECK_ARG(src && table && luts, "augment_clahe_luts: null pointer");
  EMBNET_CHECK_ARG(n > 0 && n <= 65535 && h >= 4 && w >= 4 && h <= 16384 && w <= 16384,
                   "augment_clahe_luts: n=%d h=%d w=%d (1 <= n <= 65535, 4 <= h, w <= 16384)", n, h, w);
  EMBNET_CHECK_ARG(c_in == 1 || c_in == 3, "augment_clahe_luts: c_in=%d (clahe takes 1-channel or 3-channel BGR images)", c_in);
  const int rc = check_clahe_grid("augment_clahe_luts", gx, gy, h, w);
  if (rc != EMBNET_OK) return rc;
  EMBNET_CHECK_ARG(((uintptr_t)luts & 3) == 0, "augment_clahe_luts: luts not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int tw, th;
  clahe_tile(h, w, gx, gy, tw, th);
  EMBNET_TRACE("embnet::augment_clahe_lut_kernel", TRACE_BYTES, (double)n * ((double)gx * tw * gy * th * c_in + gx * gy * 256.0), st);
  const dim3 grid((unsigned)(gx * gy), (unsigned)n);
  const unsigned char* s = (const unsigned char*)src;
  unsigned char* l = (unsigned char*)luts;
  if (c_in == 3) augment_clahe_lut_kernel<3><<<grid, 256, 0, st>>>(s, index, h, w, gx, gy, table, l);
  else augment_clahe_lut_kernel<1><<<grid, 256, 0, st>>>(s, index, h, w, gx, gy, table, l);
  return check_launch("augment_clahe_luts");
}

extern "C" int embnet_augment_apply(const void* src, const int32_t* index, int n, int h, int w, int c_in, int c_out,
                                    const float* table, uint64_t seed, uint64_t batch_no, float* dst, void* stream) {
  EMBNET_CHECK_ARG(src && table && dst, "augment_apply: null pointer");
  EMBNET_CHECK_ARG(n > 0 && n <= 65535 && h >= 4 && w >= 4 && h <= 16384 && w <= 16384,
                   "augment_apply: n=%d h=%d w=%d (1 <= n <= 65535, 4 <= h, w <= 16384)", n, h, w);
  EMBNET_CHECK_ARG(c_in >= 1 && c_in <= 4 && c_out >= c_in && c_out <= 16,
                   "augment_apply: c_in=%d c_out=%d (1 <= c_in <= 4, c_in <= c_out <= 16)", c_in, c_out);
  hipStream_t st = (hipStream_t)stream;
  const long pixels = (long)h * w;
  EMBNET_TRACE("embnet::augment_apply_kernel", TRACE_BYTES, (double)n * pixels * (c_in + 4.0 * c_out), st);
  const dim3 grid((unsigned)(cdiv(w, AUG_TILE) * cdiv(h, AUG_TILE)), (unsigned)n);
  const unsigned char* s = (const unsigned char*)src;
  const bool vec = (w & 3) == 0 && ((uintptr_t)dst & 15) == 0;
#define AUG_LAUNCH(CI, CO, V) \
  augment_apply_kernel<CI, CO, V, false><<<grid, 256, 0, st>>>(s, index, h, w, c_out, table, seed, batch_no, dst, nullptr, 0, 0)
  if (vec && c_in == 3 && c_out == 3) AUG_LAUNCH(3, 3, true);
  else if (vec && c_in == 3 && c_out == 4) AUG_LAUNCH(3, 4, true);
  else if (vec && c_in == 4 && c_out == 4) AUG_LAUNCH(4, 4, true);
  else if (vec && c_in == 1 && c_out == 1) AUG_LAUNCH(1, 1, true);
  else if (c_in == 1) AUG_LAUNCH(1, 0, false);
  else if (c_in == 2) AUG_LAUNCH(2, 0, false);
  else if (c_in == 3) AUG_LAUNCH(3, 0, false);
  else AUG_LAUNCH(4, 0, false);
#undef AUG_LAUNCH
  return check_launch("augment_apply");
}

extern "C" int embnet_augment_apply_clahe(const void* src, const int32_t* index, int n, int h, int w, int c_in, int c_out,
                                          const float* table, const void* luts, int gx, int gy, uint64_t seed, uint64_t batch_no,
                                          float* dst, void* stream) {
  EMBNET_CHECK_ARG(src && table && luts && dst, "augment_apply_clahe: null pointer");
  EMBNET_CHECK_ARG(n > 0 && n <= 65535 && h >= 4 && w >= 4 && h <= 16384 && w <= 16384,
                   "augment_apply_clahe: n=%d h=%d w=%d (1 <= n <= 65535, 4 <= h, w <= 16384)", n, h, w);
  EMBNET_CHECK_ARG((c_in == 1 || c_in == 3) && c_out >= c_in && c_out <= 16,
                   "augment_apply_clahe: c_in=%d c_out=%d (c_in 1 or 3: clahe takes gray or BGR images; c_in <= c_out <= 16)",
                   c_in, c_out);
  const int rc = check_clahe_grid("augment_apply_clahe", gx, gy, h, w);
  if (rc != EMBNET_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const long pixels = (long)h * w;
  EMBNET_TRACE("embnet::augment_apply_clahe_kernel", TRACE_BYTES, (double)n * pixels * (c_in + 4.0 * c_out), st);
  const dim3 grid((unsigned)(cdiv(w, AUG_TILE) * cdiv(h, AUG_TILE)), (unsigned)n);
  const unsigned char* s = (const unsigned char*)src;
  const unsigned char* l = (const unsigned char*)luts;
  const bool vec = (w & 3) == 0 && ((uintptr_t)dst & 15) == 0;
#define AUG_LAUNCH(CI, CO, V) \
  augment_apply_kernel<CI, CO, V, true><<<grid, 256, 0, st>>>(s, index, h, w, c_out, table, seed, batch_no, dst, l, gx, gy)
  if (vec && c_in == 3 && c_out == 3) AUG_LAUNCH(3, 3, true);
  else if (vec && c_in == 3 && c_out == 4) AUG_LAUNCH(3, 4, true);
  else if (vec && c_in == 1 && c_out == 1) AUG_LAUNCH(1, 1, true);
  else if (c_in == 1) AUG_LAUNCH(1, 0, false);
  else AUG_LAUNCH(3, 0, false);
#undef AUG_LAUNCH
  return check_launch("augment_apply_clahe");
}
