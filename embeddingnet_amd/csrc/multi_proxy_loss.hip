// SoftTriple (Qian et al., ICCV 2019) and sub-centre ArcFace (Deng et al., CVPR 2019 / ECCV 2020): the losses that score a batch against
// kc learnable centres per class.  Build-defined: the reference has no such loss.  Semantics: include/embnet.h.
//
//   X [n, e] fp32 embeddings, W [c kc, e] fp32 centres, class-major (row c' kc + j is centre j of class c'), y [n] int32 labels (any
//   order; outside [0, c) = unlabelled).  q_r = (float)(1 / sqrt(sum_k w_rk^2)), D = fp32 dot products, S = fl(D q_r) over the
//   nb = c kc rows.  One wave owns one sample's row of D.  The row is TWO-LEVEL: a lane owns the classes lane, lane + 64, ... and
//   walks each class's kc columns itself, so pooling S_ic'j -> S'_ic' needs no cross-lane traffic; the margin softmax over the c
//   pooled similarities is three passes (extrema, sum, weights), each of which pools again: a row may reach 16384 floats.  At kc = 1
//   (and, for ArcFace, margin 0) the row gives CosFace's bits: tests/test_rect_loss_identities_gpu.py.
//   prep launch (a wave per centre): q.   regulariser launch (SoftTriple with kc > 1 and tau > 0 only; a workgroup per class): the
//     class's pairs in f64, H, a per-class partial, and the last workgroup to arrive adds the partials up to *reg.
//   forward: the small kernel or D + sweep (rect_loss.h's rect_launch), partials, ticket and fixed-order f64 reduction as in
//     proxy_loss.hip.  The small path fits where e + c kc <= 4096 and n c kc e <= 2^25; `auto` takes it below 100 centres only: at
//     100, 300 and 1000 centres the matrix path's forward measured 1.6 to 9 times faster.
//   backward: the proxies' launches (rect_loss.h declares them) with c := c kc, and between Y and the projection one launch that adds
//     the regulariser's term  sum_t H_rt q_t w_t  to Y in f64.
// A label is compared, and used as an index (the sample's own class) only behind the range check that makes it a class index.  Nothing
// is atomic in floating point, every reduction has a fixed order: bitwise reproducible.  No host synchronisation, no allocation.
#include <math.h>
#include "rect_loss.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr int MPROXY_MAX_KC = 32;
constexpr int MPROXY_MAX_PAIRS = MPROXY_MAX_KC * (MPROXY_MAX_KC - 1) / 2;
constexpr int MPROXY_AUTO_MATRIX_FROM = 100;             // c kc from which `auto` takes the matrix path (measured; below: inherited)
constexpr float MPROXY_R_FLOOR = 0x1p-10f;               // ArcFace: the floor under r = sqrt(1 - S'^2) in phi'
constexpr double MPROXY_REG_EPS = 1e-5;                  // SoftTriple's regulariser: sqrt(2 + 1e-5 - 2 g)
static_assert(EMBNET_MPROXY_SMALL == 1 && EMBNET_MPROXY_MATRIX == 2, "path constants");

struct MProxyParams {
  const float* emb;                                      // [n][e]
  const float* centres;                                  // [c kc][e]
  const int32_t* labels;                                 // [n]
  const float* q;                                        // [c kc]
  int n, c, kc, e, kind;
  float a, b, gamma;                                     // lambda, delta, gamma | scale, margin, -
  float cosm, sinm, th, mm;                              // ArcFace: cos m, sin m, cos(pi - m), sin(pi - m) m (host, f64, rounded)
  float* g; int32_t* counts; float* mean; float* reg;
  int has_reg;                                           // the regulariser's launch has written *reg
  int* ticket; double* part_loss; int4* part_cnt;        // workspace: arrival counter (zero between launches), partials
  const float* d;                                        // matrix path: D [n][c kc]
};

struct MProxyPool { float s, zm, den; };                 // S', and SoftTriple's pooling maximum and denominator

// ---- prep: q; one wave per centre -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RECT_THREADS) void mproxy_prep_kernel(const float* __restrict__ w, int nb, int e, float* __restrict__ q) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * RECT_WG_ANCHORS + (threadIdx.x >> 6);
  if (r >= nb) return;                                   // wave-uniform
  const float qr = proxy_row_q(w + (long)r * e, e, lane);
  if (lane == 0) q[r] = qr;
}

// ---- SoftTriple's regulariser: one workgroup per class ------------------------------------------------------------------------------
// g_st = q_s q_t sum_k w_sk w_tk: the products of fp32 numbers are exact in f64, the thread that owns the pair adds them in k order
// (the class's rows pass through LDS 64 columns at a time, zeros past the row's end).  term = sqrt(max(0, 2 + 1e-5 - 2 g)),
// H_st = H_ts = -coef / sqrt(2 + 1e-5 - 2 g), coef = tau / (c kc (kc - 1)); |g| <= (1 + 2^-24)^2, so the root's argument stays above
// 9e-6.  Thread 0 adds the class's terms in pair order (s, t lexicographic); the last workgroup to arrive adds the classes' partials
// (thread-strided, butterfly, waves in order) and writes *reg = (float)(coef total).
__global__ __launch_bounds__(RECT_THREADS) void mproxy_reg_kernel(const float* __restrict__ w, const float* __restrict__ q, int c, int kc,
                                                                   int e, float tau, float* __restrict__ h, double* __restrict__ part,
                                                                   int* ticket, float* __restrict__ reg) {
  __shared__ float tile[MPROXY_MAX_KC][65];
  __shared__ double term[MPROXY_MAX_PAIRS];
  __shared__ double wsum[RECT_THREADS / 64];
  const int tid = threadIdx.x, cl = blockIdx.x, r0 = cl * kc;
  const int pairs = kc * (kc - 1) / 2;
  int ps[2], pt[2];
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int u = 0; u < 2; ++u) {                          // pair tid + 256 u -> (s, t), s < t
    int p = tid + RECT_THREADS * u, s = 0;
    ps[u] = pt[u] = -1;
    if (p < pairs) {
      while (p >= kc - 1 - s) { p -= kc - 1 - s; ++s; }
      ps[u] = s; pt[u] = s + 1 + p;
    }
  }
  for (int k0 = 0; k0 < e; k0 += 64) {
    for (int i = tid; i < kc * 64; i += RECT_THREADS) {
      const int r = i >> 6, kk = i & 63;
      tile[r][kk] = k0 + kk < e ? w[(long)(r0 + r) * e + k0 + kk] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (ps[u] >= 0) {
        for (int kk = 0; kk < 64; ++kk) acc[u] = fma((double)tile[ps[u]][kk], (double)tile[pt[u]][kk], acc[u]);
      }
    }
    __syncthreads();
  }
  const double coef = (double)tau / ((double)c * (double)kc * (double)(kc - 1));
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (ps[u] >= 0) {
      const double g = (double)q[r0 + ps[u]] * (double)q[r0 + pt[u]] * acc[u];
      const double arg = 2.0 + MPROXY_REG_EPS - 2.0 * g;
      term[tid + RECT_THREADS * u] = sqrt(fmax(0.0, arg));
      const float hv = (float)(-coef / sqrt(arg));
      h[((long)r0 + ps[u]) * kc + pt[u]] = hv;
      h[((long)r0 + pt[u]) * kc + ps[u]] = hv;
    }
  }
  if (tid < kc) h[((long)r0 + tid) * kc + tid] = 0.f;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int p = 0; p < pairs; ++p) s += term[p];
    part[cl] = s;
  }
  if (!last_workgroup_to_arrive(ticket)) return;
  double s = 0.0;
  for (int i = tid; i < c; i += RECT_THREADS) s += __hip_atomic_load(&part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  s = wave_sum(s);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int wv = 0; wv < RECT_THREADS / 64; ++wv) t += wsum[wv];
    *reg = (float)(coef * t);
  }
}

// backward: Y_r += sum_{t != r, same class} H_rt q_t w_t, in f64, t in order; a thread per element of Y
__global__ __launch_bounds__(256) void mproxy_bwd_reg_kernel(const float* __restrict__ h, const float* __restrict__ q,
                                                             const float* __restrict__ w, int kc, int e, double* __restrict__ y) {
  const int k = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (k >= e) return;
  const int r0 = (r / kc) * kc;
  double s = 0.0;
  for (int t = 0; t < kc; ++t) {
    if (r0 + t == r) continue;
    s = fma((double)h[(long)r * kc + t] * (double)q[r0 + t], (double)w[(long)(r0 + t) * e + k], s);
  }
  y[(long)r * e + k] += s;
}

// ---- the row body -----------------------------------------------------------------------------------------------------------------------
// labelled samples, the same in every thread of the workgroup
__device__ __forceinline__ int mproxy_labelled(const int32_t* __restrict__ labels, int n, int c) {
  int l = 0;
  for (int i = threadIdx.x; i < n; i += RECT_THREADS) l += (unsigned)labels[i] < (unsigned)c;
  return block_total256(l);
}

// One class's kc similarities pooled into S' (one thread).  ArcFace: the maximum.  SoftTriple: z_j = fl(S_j / gamma), zm = max z,
// x_j = expf(fl(z_j - zm)), den = the x_j added in j order (>= 1), num = the chain fma(x_j, S_j, num) in j order, S' = fl(num / den).
// kc = 1: S' = S.
__device__ __forceinline__ MProxyPool mproxy_pool(const float* drow, const MProxyParams& P, int cl) {
  const int kc = P.kc, r0 = cl * kc;
  const float s0 = __fmul_rn(drow[r0], P.q[r0]);
  if (kc == 1) return MProxyPool{s0, 0.f, 1.f};
  if (P.kind == EMBNET_MPROXY_ARCFACE) {
    float m = s0;
    for (int j = 1; j < kc; ++j) m = fmaxf(m, __fmul_rn(drow[r0 + j], P.q[r0 + j]));
    return MProxyPool{m, 0.f, 1.f};
  }
  float zm = __fdiv_rn(s0, P.gamma);
  for (int j = 1; j < kc; ++j) zm = fmaxf(zm, __fdiv_rn(__fmul_rn(drow[r0 + j], P.q[r0 + j]), P.gamma));
  float num = 0.f, den = 0.f;
  for (int j = 0; j < kc; ++j) {
    const float s = __fmul_rn(drow[r0 + j], P.q[r0 + j]);
    const float x = expf(__fsub_rn(__fdiv_rn(s, P.gamma), zm));
    den = __fadd_rn(den, x);
    num = fmaf(x, s, num);
  }
  return MProxyPool{__fdiv_rn(num, den), zm, den};
}

// ArcFace's phi on the own class: above th = cos(pi - m)  fl(fl(S' cos m) - fl(r sin m)), r = sqrt(max(0, fl(1 - fl(S'^2))));
// at or below it  fl(S' - mm)
__device__ __forceinline__ float mproxy_r(float s) { return __fsqrt_rn(fmaxf(0.f, __fsub_rn(1.f, __fmul_rn(s, s)))); }
__device__ __forceinline__ float mproxy_phi(const MProxyParams& P, float s) {
  if (!(s > P.th)) return __fsub_rn(s, P.mm);
  return __fsub_rn(__fmul_rn(s, P.cosm), __fmul_rn(mproxy_r(s), P.sinm));
}
// phi': fl(cos m + fl(fl(S' sin m) / max(r, 2^-10))) above th, cos m where r = 0, 1 at or below th
__device__ __forceinline__ float mproxy_dphi(const MProxyParams& P, float s) {
  if (!(s > P.th)) return 1.f;
  const float r = mproxy_r(s);
  if (r == 0.f) return P.cosm;
  return __fadd_rn(P.cosm, __fdiv_rn(__fmul_rn(s, P.sinm), fmaxf(r, MPROXY_R_FLOOR)));
}

// the logit of a pooled similarity: one rounding form per case
__device__ __forceinline__ float mproxy_logit(const MProxyParams& P, float s, bool own) {
  if (!own) return __fmul_rn(P.a, s);
  if (P.kind == EMBNET_MPROXY_SOFT_TRIPLE) return __fmul_rn(P.a, __fsub_rn(s, P.b));
  return __fmul_rn(P.a, mproxy_phi(P, s));
}

// One wave, sample ai: its row drow[c kc] of D over the centres.  Writes all c kc entries of the row of G.
__device__ __forceinline__ void mproxy_row(const float* drow, const MProxyParams& P, int ai, int nl, int lane) {
  const int c = P.c, kc = P.kc;
  float* grow = P.g + (long)ai * c * kc;
  const int y = P.labels[ai];
  if ((unsigned)y >= (unsigned)c) {                      // unlabelled (wave-uniform): a zero row, no loss
    for (int col = lane; col < c * kc; col += 64) grow[col] = 0.f;
    if (lane == 0) { P.part_loss[ai] = 0.0; P.part_cnt[ai] = make_int4(0, 0, 0, 0); }
    return;
  }
  const bool arc = P.kind == EMBNET_MPROXY_ARCFACE;
  float M = -INFINITY, mxo = -INFINITY;
  for (int cl = lane; cl < c; cl += 64) {
    const float s = mproxy_pool(drow, P, cl).s;
    if (cl != y) mxo = fmaxf(mxo, s);
    M = fmaxf(M, mproxy_logit(P, s, cl == y));
  }
  M = wave_max(M);
  mxo = wave_max(mxo);
  const float sy = mproxy_pool(drow, P, y).s;            // every lane: the same value
  const float ty = mproxy_logit(P, sy, true);
  float se = 0.f;
  for (int cl = lane; cl < c; cl += 64)                  // lane-strided, class order
    se += expf(__fsub_rn(mproxy_logit(P, mproxy_pool(drow, P, cl).s, cl == y), M));
  const float d = wave_sum(se);                          // >= 1: the largest logit gives e^0
  const float cs = __fdiv_rn(P.a, (float)max(nl, 1));    // the normaliser 1/n_l joins the scale
  const float psi = arc ? mproxy_dphi(P, sy) : 1.f;
  for (int cl = lane; cl < c; cl += 64) {
    const MProxyPool pl = mproxy_pool(drow, P, cl);
    const float w = __fdiv_rn(expf(__fsub_rn(mproxy_logit(P, pl.s, cl == y), M)), d);
    float base = __fmul_rn(cs, cl == y ? __fsub_rn(w, 1.f) : w);
    if (arc && cl == y) base = __fmul_rn(base, psi);
    const int r0 = cl * kc;
    if (kc == 1) {
      grow[r0] = base;
    } else if (arc) {                                    // the whole weight on the first sub-centre that attains the maximum
      bool found = false;
      for (int j = 0; j < kc; ++j) {
        const bool hit = !found && __fmul_rn(drow[r0 + j], P.q[r0 + j]) == pl.s;
        grow[r0 + j] = hit ? base : 0.f;
        found = found || hit;
      }
    } else {                                             // dS'/dS_j = p_j (1 + (S_j - S') / gamma), p_j = fl(x_j / den)
      for (int j = 0; j < kc; ++j) {
        const float s = __fmul_rn(drow[r0 + j], P.q[r0 + j]);
        const float p = __fdiv_rn(expf(__fsub_rn(__fdiv_rn(s, P.gamma), pl.zm)), pl.den);
        grow[r0 + j] = __fmul_rn(base, __fmul_rn(p, __fadd_rn(1.f, __fdiv_rn(__fsub_rn(s, pl.s), P.gamma))));
      }
    }
  }
  if (lane == 0) {
    P.part_loss[ai] = (double)__fadd_rn(logf(d), __fsub_rn(M, ty));
    P.part_cnt[ai] = make_int4(1, mxo >= sy, arc && !(sy > P.th), 0);
  }
}

// The last workgroup to arrive reduces the n partials in index order: loss = sum l / n_l + R, one cast of the f64 expression.
__device__ __forceinline__ void mproxy_finish(const MProxyParams& P) {
  if (!last_workgroup_to_arrive(P.ticket)) return;
  double ts[1];
  int tc[3];
  if (reduce_partials<RECT_THREADS>(P.part_loss, P.part_cnt, P.n, ts, tc)) {
    P.counts[0] = tc[0];                                 // labelled samples: at most 4096
    P.counts[1] = tc[1];
    P.counts[2] = tc[2];
    double r = 0.0;
    if (P.has_reg) r = (double)*P.reg;
    else *P.reg = 0.f;
    *P.mean = (float)((tc[0] > 0 ? ts[0] / (double)tc[0] : 0.0) + r);
  }
}

// ---- forward, small path: grid = ceil(n / 4) workgroups -----------------------------------------------------------------------------
__global__ __launch_bounds__(RECT_THREADS) void mproxy_small_fwd_kernel(MProxyParams P) {
  __shared__ __attribute__((aligned(16))) float lds[RECT_LDS_FLOATS];
  const int n = P.n, nb = P.c * P.kc, e = P.e;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a0 = blockIdx.x * RECT_WG_ANCHORS;
  const int nl = mproxy_labelled(P.labels, n, P.c);
  float* A = lds;                                        // [4][e] the workgroup's samples (zero rows past n)
  float* D = lds + RECT_WG_ANCHORS * e;                 // [4][nb] their rows of D
  for (int i = tid; i < RECT_WG_ANCHORS * e; i += RECT_THREADS) A[i] = a0 + i / e < n ? P.emb[(long)a0 * e + i] : 0.f;
  __syncthreads();
  anchor_dots<RECT_WG_ANCHORS, RECT_WG_ANCHORS, PairDotBody>(A, RECT_WG_ANCHORS, P.centres, nb, e, D);
  __syncthreads();
  if (a0 + wave < n) mproxy_row(D + wave * nb, P, a0 + wave, nl, lane);
  mproxy_finish(P);
}

// ---- forward, matrix path: grid = ceil(n / 4) workgroups, one wave walks one row of D from L2 ---------------------------------------
__global__ __launch_bounds__(RECT_THREADS) void mproxy_sweep_kernel(MProxyParams P) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = blockIdx.x * RECT_WG_ANCHORS + wave;
  const int nl = mproxy_labelled(P.labels, P.n, P.c);
  if (a < P.n) mproxy_row(P.d + (long)a * P.c * P.kc, P, a, nl, lane);
  mproxy_finish(P);
}

// ---- host side: range, path rule, workspace layout ------------------------------------------------------------------------------------
inline bool mproxy_range_ok(int n, int c, int kc, int e) {
  return n >= 2 && n <= PROXY_MAX_N && c >= 2 && kc >= 1 && kc <= MPROXY_MAX_KC && (long)c * kc <= PROXY_MAX_C && e >= 1 &&
         e <= PROXY_MAX_E;
}

inline bool mproxy_small_fits(int n, int c, int kc, int e) {
  return rect_small_fits(n, (long)c * kc, e);
}

// [16 B ticket][n f64 partial losses][n int4 partial counts][c f64 regulariser partials][n*nb f32 D][nb*e f64 Y], nb = c kc
struct MProxyWorkspace {
  size_t part_loss, part_cnt, part_reg, d, y, bytes;
  MProxyWorkspace(int n, int c, int kc, int e) {
    const size_t nb = (size_t)c * kc;
    part_loss = 16;
    part_cnt = part_loss + pair_align16((size_t)n * 8);
    part_reg = part_cnt + (size_t)n * 16;
    d = part_reg + pair_align16((size_t)c * 8);
    y = d + pair_align16(nb * n * 4);
    bytes = y + pair_align16(nb * e * 8);
  }
};

inline int mproxy_check_common(const char* what, bool pointers, int n, int c, int kc, int e, const void* workspace,
                               size_t workspace_bytes) {
  EMBNET_CHECK_ARG(pointers, "%s: null pointer", what);
  EMBNET_CHECK_ARG(n >= 2 && n <= PROXY_MAX_N, "%s: n=%d outside [2, %d]", what, n, PROXY_MAX_N);
  EMBNET_CHECK_ARG(c >= 2, "%s: c=%d below 2", what, c);
  EMBNET_CHECK_ARG(kc >= 1 && kc <= MPROXY_MAX_KC, "%s: kc=%d outside [1, %d]", what, kc, MPROXY_MAX_KC);
  EMBNET_CHECK_ARG((long)c * kc <= PROXY_MAX_C, "%s: c*kc=%ld above %d", what, (long)c * kc, PROXY_MAX_C);
  EMBNET_CHECK_ARG(e >= 1 && e <= PROXY_MAX_E, "%s: e=%d outside [1, %d]", what, e, PROXY_MAX_E);
  return check_workspace(what, workspace, workspace_bytes, MProxyWorkspace(n, c, kc, e).bytes);
}

}  // namespace embnet

using namespace embnet;

extern "C" size_t embnet_multi_proxy_loss_workspace_bytes(int n, int c, int kc, int e) {
  return mproxy_range_ok(n, c, kc, e) ? MProxyWorkspace(n, c, kc, e).bytes : 0;
}

extern "C" int embnet_multi_proxy_loss_path(int n, int c, int kc, int e) {
  if (!mproxy_range_ok(n, c, kc, e)) return 0;
  return mproxy_small_fits(n, c, kc, e) && c * kc < MPROXY_AUTO_MATRIX_FROM ? EMBNET_MPROXY_SMALL : EMBNET_MPROXY_MATRIX;
}

extern "C" int embnet_multi_proxy_loss_fwd(const float* emb, const float* centres, const int32_t* labels, int n, int c, int kc, int e,
                                           int kind, float a, float b, float gamma, float tau, int path, float* pair_g, float* q,
                                           float* reg_h, int32_t* counts, float* mean_loss, float* reg, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  const char* what = "multi_proxy_loss_fwd";
  const bool st = kind == EMBNET_MPROXY_SOFT_TRIPLE;
  EMBNET_CHECK_ARG(st || kind == EMBNET_MPROXY_ARCFACE, "%s: unknown kind %d", what, kind);
  EMBNET_CHECK_ARG(path >= 0 && path <= EMBNET_MPROXY_MATRIX, "%s: unknown path %d", what, path);
  EMBNET_CHECK_ARG(isfinite(a) && a > 0.f, "%s: scale=%g must be finite and positive", what, (double)a);
  if (st) {
    EMBNET_CHECK_ARG(isfinite(b), "%s: margin=%g must be finite", what, (double)b);
    EMBNET_CHECK_ARG(isfinite(gamma) && gamma > 0.f, "%s: gamma=%g must be finite and positive", what, (double)gamma);
    EMBNET_CHECK_ARG(isfinite(tau) && tau >= 0.f, "%s: tau=%g must be finite and not negative", what, (double)tau);
  } else {
    EMBNET_CHECK_ARG(isfinite(b) && b >= 0.f && (double)b < M_PI / 2, "%s: margin=%g outside [0, pi/2)", what, (double)b);
  }
  const int rc = mproxy_check_common(what, emb && centres && labels && pair_g && q && counts && mean_loss && reg && workspace, n, c, kc, e,
                                     workspace, workspace_bytes);
  if (rc != EMBNET_OK) return rc;
  const bool has_reg = st && kc > 1 && tau > 0.f;
  EMBNET_CHECK_ARG(!has_reg || reg_h, "%s: null pointer (reg_h, with kc > 1 and tau > 0)", what);
  EMBNET_CHECK_ARG(path != EMBNET_MPROXY_SMALL || mproxy_small_fits(n, c, kc, e), "%s: n=%d c=%d kc=%d e=%d does not fit the small path",
                   what, n, c, kc, e);
  if (path == 0) path = embnet_multi_proxy_loss_path(n, c, kc, e);
  const MProxyWorkspace L(n, c, kc, e);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int nb = c * kc;
  float* d = (float*)(ws + L.d);
  MProxyParams P{};
  P.emb = emb; P.centres = centres; P.labels = labels; P.q = q;
  P.n = n; P.c = c; P.kc = kc; P.e = e; P.kind = kind;
  P.a = a; P.b = b; P.gamma = st ? gamma : 1.f;
  if (!st) {                                             // once, in f64, rounded to fp32
    const double m = (double)b;
    P.cosm = (float)cos(m); P.sinm = (float)sin(m); P.th = (float)cos(M_PI - m); P.mm = (float)(sin(M_PI - m) * m);
  }
  P.g = pair_g; P.counts = counts; P.mean = mean_loss; P.reg = reg; P.has_reg = has_reg;
  P.ticket = (int*)ws; P.part_loss = (double*)(ws + L.part_loss); P.part_cnt = (int4*)(ws + L.part_cnt); P.d = d;
  {
    EMBNET_TRACE("embnet::mproxy_prep_kernel", TRACE_BYTES, 4.0 * nb * e + 4.0 * nb, stream);
    mproxy_prep_kernel<<<cdiv(nb, RECT_WG_ANCHORS), RECT_THREADS, 0, s>>>(centres, nb, e, q);
  }
  if (has_reg) {
    EMBNET_TRACE_FLOP("embnet::mproxy_reg_kernel", 1.0 * c * kc * (kc - 1) * e, 4.0 * nb * e + 4.0 * nb * kc, stream);
    mproxy_reg_kernel<<<c, RECT_THREADS, 0, s>>>(centres, q, c, kc, e, tau, reg_h, (double*)(ws + L.part_reg), (int*)ws, reg);
  }
  return rect_launch(what, mproxy_small_fwd_kernel, "embnet::mproxy_small_fwd_kernel", mproxy_sweep_kernel,
                     "embnet::mproxy_sweep_kernel", path == EMBNET_MPROXY_SMALL, P, emb, centres, d, n, nb, e, stream);
}

extern "C" int embnet_multi_proxy_loss_bwd(const float* emb, const float* centres, int n, int c, int kc, int e, const float* pair_g,
                                           const float* q, const float* reg_h, const float* upstream, float* demb, float* dcentres,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "multi_proxy_loss_bwd";
  const int rc = mproxy_check_common(what, emb && centres && pair_g && q && demb && dcentres && workspace, n, c, kc, e, workspace,
                                     workspace_bytes);
  if (rc != EMBNET_OK) return rc;
  const int nb = c * kc;
  double* y = (double*)((char*)workspace + MProxyWorkspace(n, c, kc, e).y);
  proxy_bwd_products(emb, centres, n, nb, e, false, pair_g, q, upstream, demb, y, stream);
  if (reg_h && kc > 1) {
    EMBNET_TRACE("embnet::mproxy_bwd_reg_kernel", TRACE_BYTES, 4.0 * nb * e + 16.0 * nb * e, stream);
    mproxy_bwd_reg_kernel<<<dim3(cdiv(e, 256), nb), 256, 0, (hipStream_t)stream>>>(reg_h, q, centres, kc, e, y);
  }
  proxy_bwd_project(y, centres, q, nb, e, upstream, dcentres, stream);
  return check_launch(what);
}
