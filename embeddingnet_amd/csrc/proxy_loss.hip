// Proxy-Anchor (Kim et al., CVPR 2020) and CosFace / NormSoftmax (Wang et al., CVPR 2018; Zhai & Wu 2019): the losses that score a
// batch against one learnable vector per class.  Build-defined: the reference has no such loss.  Semantics: include/embnet.h.
//
//   X [n, e] fp32 embeddings, W [c, e] fp32 proxies, y [n] int32 labels (any order; outside [0, c) = unlabelled).
//   q_c = (float)(1 / sqrt(sum_k w_ck^2)) (f64, k order; 0 for a zero proxy),  D = fp32 dot products,  S = fl(D q_c).
//   Both losses are ONE rectangle seen from its two sides: anchors A [na, e] meet others B [nb, e], one wave owns one anchor's row.
//     Proxy-Anchor: the anchors are the proxies (na = c, nb = n), G is [c][n];  a row's positives are the samples of its class.
//     CosFace:      the anchors are the samples (na = n, nb = c), G is [n][c];  a row's positive is the sample's own class.
//   prep launch (a wave per class): q, the class sizes cnt[c] (every workgroup of the forward adds them up to |C+| and n_l).
//   small path (e + max(n, c) <= 4096 and n c e <= 2^25), ONE more launch: a workgroup holds four anchors and their four rows of D
//     in LDS (pair_loss.h's anchor_dots); matrix path, TWO more (rect_loss.h's rect_launch): D into the workspace, then a sweep from
//     L2 (a CosFace row reaches 16384 floats: not staged).  One wave per anchor runs the body in three passes (extrema, sums, weights).
//   per-anchor partials, the arrival ticket, pair_loss.h's fixed-order f64 reduction by the last workgroup.
//   backward, three launches (four with demb's class sum split, rect_loss.h's split product) on the f64 matrix instructions:
//     demb = g Q^(T) W, Y = G^(T) X in f64 into the workspace, then a wave per class: dproxies_c = g q_c (Y_c - q_c^2 (Y_c . w_c) w_c),
//     every output one fp32 rounding of an f64 expression.
// A label is compared, and used as an index (CosFace: the sample's own column) only behind the range check that makes it a class
// index; an unlabelled value addresses nothing.  Nothing is atomic in floating point, every reduction has a fixed order: bitwise
// reproducible.  No host synchronisation, no allocation: capturable in a graph.
#include <math.h>
#include "rect_loss.h"
#include "../../include/embnet.h"

namespace embnet {

static_assert(EMBNET_PROXY_SMALL == 1 && EMBNET_PROXY_MATRIX == 2, "path constants");

struct ProxyParams {
  const float* anchors;                                  // [na][e]
  const float* others;                                   // [nb][e]
  const int32_t* labels;                                 // [n]
  const float* q;                                        // [c]
  const int32_t* cnt;                                    // [c] class sizes (prep)
  int na, nb, e, n, c, kind;
  float a, b;                                            // alpha, delta | scale, margin
  float* g; int32_t* counts; float* mean;
  int* ticket; double2* part_loss; int4* part_cnt;       // workspace: arrival counter (zero between launches), partials
  const float* d;                                        // matrix path: D [na][nb]
};

struct ProxyAnchorOut { float lp, ln; int has, viol; };

// ---- prep: q (rect_loss.h's proxy_row_q) and the class sizes; one wave per class; the labels are counted lane-strided (integers) --
__global__ __launch_bounds__(RECT_THREADS) void proxy_prep_kernel(const float* __restrict__ w, const int32_t* __restrict__ labels,
                                                                   int n, int c, int e, float* __restrict__ q,
                                                                   int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int cl = blockIdx.x * RECT_WG_ANCHORS + (threadIdx.x >> 6);
  if (cl >= c) return;                                   // wave-uniform
  const float qc = proxy_row_q(w + (long)cl * e, e, lane);
  int m = 0;
  for (int i = lane; i < n; i += 64) m += labels[i] == cl;
  m = wave_sum(m);
  if (lane == 0) {
    q[cl] = qc;
    cnt[cl] = m;
  }
}

// (classes with a sample, labelled samples), the same in every thread of the workgroup
__device__ __forceinline__ int2 proxy_totals(const int32_t* __restrict__ cnt, int c) {
  int p = 0, l = 0;                                      // both from one pass over the class sizes
  for (int i = threadIdx.x; i < c; i += RECT_THREADS) { const int v = cnt[i]; p += v > 0; l += v; }
  int t[2] = {p, l};
  block_total256(t);
  return make_int2(t[0], t[1]);
}

// one rounding order: t = fl(c fl(s + o)); monotone in s for either sign of c
__device__ __forceinline__ float proxy_t(float c, float s, float o) { return __fmul_rn(c, __fadd_rn(s, o)); }

// Proxy-Anchor, one wave, anchor = class ai: its row drow[n] of D over the samples.  Writes all n entries of the row of G.
__device__ __forceinline__ ProxyAnchorOut proxy_anchor_row(const float* drow, const ProxyParams& P, int ai, int2 tot, float* grow,
                                                           int lane) {
  const int n = P.nb, c = P.c;
  const float alpha = P.a, delta = P.b, qa = P.q[ai];
  float mn = INFINITY, mx = -INFINITY;
  for (int col = lane; col < n; col += 64) {
    const int y = P.labels[col];
    if ((unsigned)y >= (unsigned)c) continue;
    const float s = __fmul_rn(drow[col], qa);
    if (y == ai) mn = fminf(mn, s); else mx = fmaxf(mx, s);
  }
  mn = wave_min(mn);                                     // min over the positives (+inf: none)
  mx = wave_max(mx);                                     // max over the negatives (-inf: none)
  // t is monotone in s: the largest exponent of a side belongs to its hardest pair; an empty side has t = -inf and m = 0
  const float mp = fmaxf(0.f, proxy_t(-alpha, mn, -delta));
  const float mg = fmaxf(0.f, proxy_t(alpha, mx, delta));
  float sp = 0.f, sn = 0.f;
  for (int col = lane; col < n; col += 64) {             // lane-strided, column order
    const int y = P.labels[col];
    if ((unsigned)y >= (unsigned)c) continue;
    const float s = __fmul_rn(drow[col], qa);
    if (y == ai) sp += expf(__fsub_rn(proxy_t(-alpha, s, -delta), mp));
    else sn += expf(__fsub_rn(proxy_t(alpha, s, delta), mg));
  }
  const float dp = __fadd_rn(expf(-mp), wave_sum(sp));   // e^{-m} + sum e^{t - m} >= 1
  const float dn = __fadd_rn(expf(-mg), wave_sum(sn));
  const float cp = __fdiv_rn(alpha, (float)max(tot.x, 1));           // the normalisers 1/|C+| and 1/c join alpha
  const float cn = __fdiv_rn(alpha, (float)c);
  for (int col = lane; col < n; col += 64) {
    const int y = P.labels[col];
    float g = 0.f;
    if ((unsigned)y < (unsigned)c) {
      const float s = __fmul_rn(drow[col], qa);
      if (y == ai) g = -__fmul_rn(cp, __fdiv_rn(expf(__fsub_rn(proxy_t(-alpha, s, -delta), mp)), dp));
      else g = __fmul_rn(cn, __fdiv_rn(expf(__fsub_rn(proxy_t(alpha, s, delta), mg)), dn));
    }
    grow[col] = g;
  }
  const int npos = P.cnt[ai];
  const int has = npos > 0;
  return ProxyAnchorOut{__fadd_rn(mp, logf(dp)), __fadd_rn(mg, logf(dn)), has, has && tot.y - npos > 0 && mx >= mn};
}

// CosFace, one wave, anchor = sample ai: its row drow[c] of D over the classes.  Writes all c entries of the row of G.
__device__ __forceinline__ ProxyAnchorOut proxy_softmax_row(const float* drow, const ProxyParams& P, int ai, int2 tot, float* grow,
                                                            int lane) {
  const int c = P.nb;
  const int y = P.labels[ai];
  if ((unsigned)y >= (unsigned)c) {                      // unlabelled (wave-uniform): a zero row, no loss
    for (int col = lane; col < c; col += 64) grow[col] = 0.f;
    return ProxyAnchorOut{0.f, 0.f, 0, 0};
  }
  const float sigma = P.a, mu = P.b;
  float M = -INFINITY, mxo = -INFINITY;
  for (int col = lane; col < c; col += 64) {
    const float s = __fmul_rn(drow[col], P.q[col]);
    if (col != y) mxo = fmaxf(mxo, s);
    M = fmaxf(M, __fmul_rn(sigma, col == y ? __fsub_rn(s, mu) : s));
  }
  M = wave_max(M);
  mxo = wave_max(mxo);
  const float sy = __fmul_rn(drow[y], P.q[y]);
  const float ty = __fmul_rn(sigma, __fsub_rn(sy, mu));
  float se = 0.f;
  for (int col = lane; col < c; col += 64) {             // lane-strided, column order
    const float s = __fmul_rn(drow[col], P.q[col]);
    se += expf(__fsub_rn(__fmul_rn(sigma, col == y ? __fsub_rn(s, mu) : s), M));
  }
  const float d = wave_sum(se);                          // >= 1: the largest logit gives e^0
  const float cs = __fdiv_rn(sigma, (float)max(tot.y, 1));           // the normaliser 1/n_l joins sigma
  for (int col = lane; col < c; col += 64) {
    const float s = __fmul_rn(drow[col], P.q[col]);
    const float w = __fdiv_rn(expf(__fsub_rn(__fmul_rn(sigma, col == y ? __fsub_rn(s, mu) : s), M)), d);
    grow[col] = __fmul_rn(cs, col == y ? __fsub_rn(w, 1.f) : w);
  }
  return ProxyAnchorOut{__fadd_rn(logf(d), __fsub_rn(M, ty)), 0.f, 1, mxo >= sy};
}

__device__ __forceinline__ void proxy_row(const float* drow, const ProxyParams& P, int a, int2 tot, int lane) {
  float* grow = P.g + (long)a * P.nb;
  const ProxyAnchorOut o = P.kind == EMBNET_PROXY_ANCHOR ? proxy_anchor_row(drow, P, a, tot, grow, lane)
                                                         : proxy_softmax_row(drow, P, a, tot, grow, lane);
  if (lane == 0) {
    P.part_loss[a] = make_double2((double)o.lp, (double)o.ln);
    P.part_cnt[a] = make_int4(o.has, o.viol, 0, 0);
  }
}

// The last workgroup to arrive reduces the na partials (two loss sums, two counters) in index order.
// loss = sum lp / (anchors with a positive term) + sum ln / c  (the second sum is zero for CosFace).
__device__ __forceinline__ void proxy_finish(const ProxyParams& P, int2 tot) {
  if (!last_workgroup_to_arrive(P.ticket)) return;
  double ts[2];
  int tc[2];
  if (reduce_partials<RECT_THREADS>((const double*)P.part_loss, P.part_cnt, P.na, ts, tc)) {
    P.counts[0] = tc[0];                                 // |C+| or n_l: at most 16384
    P.counts[1] = tot.y;                                 // labelled samples: at most 4096
    P.counts[2] = tc[1];
    *P.mean = (float)((tc[0] > 0 ? ts[0] / (double)tc[0] : 0.0) + ts[1] / (double)P.c);
  }
}

// ---- forward, small path: grid = ceil(na / 4) workgroups -------------------------------------------------------------------------
__global__ __launch_bounds__(RECT_THREADS) void proxy_small_fwd_kernel(ProxyParams P) {
  __shared__ __attribute__((aligned(16))) float lds[RECT_LDS_FLOATS];
  const int na = P.na, nb = P.nb, e = P.e;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a0 = blockIdx.x * RECT_WG_ANCHORS;
  const int2 tot = proxy_totals(P.cnt, P.c);
  float* A = lds;                                        // [4][e] the workgroup's anchors (zero rows past na)
  float* D = lds + RECT_WG_ANCHORS * e;                 // [4][nb] their rows of D
  for (int i = tid; i < RECT_WG_ANCHORS * e; i += RECT_THREADS) A[i] = a0 + i / e < na ? P.anchors[(long)a0 * e + i] : 0.f;
  __syncthreads();
  anchor_dots<RECT_WG_ANCHORS, RECT_WG_ANCHORS, PairDotBody>(A, RECT_WG_ANCHORS, P.others, nb, e, D);   // rows past na are zero
  __syncthreads();
  if (a0 + wave < na) proxy_row(D + wave * nb, P, a0 + wave, tot, lane);
  proxy_finish(P, tot);
}

// ---- forward, matrix path: grid = ceil(na / 4) workgroups, one wave walks one row of D from L2 -----------------------------------
__global__ __launch_bounds__(RECT_THREADS) void proxy_sweep_kernel(ProxyParams P) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = blockIdx.x * RECT_WG_ANCHORS + wave;
  const int2 tot = proxy_totals(P.cnt, P.c);
  if (a < P.na) proxy_row(P.d + (long)a * P.nb, P, a, tot, lane);
  proxy_finish(P, tot);
}

// ---- backward: rectangular products on pair_loss.h's mm_f64_tile ------------------------------------------------------------------
// The left operand is G[r][j] or, TRANS, G[j][r]; demb's is scaled by q[j].  demb = (float)(g sum), g = *upstream (NULL = 1).
template <bool TRANS>
__global__ __launch_bounds__(256) void proxy_bwd_emb_kernel(const float* __restrict__ G, const float* __restrict__ q,
                                                            const float* __restrict__ proxies, int n, int c, int e,
                                                            const float* __restrict__ upstream, float* __restrict__ demb) {
  mm_f64_tile<TRANS ? MM_TRANS : MM_DIRECT, true>(G, q, proxies, n, c, e, 0, c, RectScaledOut<false>{upstream, n, demb});
}

// Few samples against many classes leave the grid above ceil(n/32) ceil(e/32) workgroups with c / 32 serial rounds each: the
// classes are then split (rect_loss.h's split product).
template <bool TRANS>
__global__ __launch_bounds__(256) void proxy_bwd_emb_part_kernel(const float* __restrict__ G, const float* __restrict__ q,
                                                                 const float* __restrict__ proxies, int n, int c, int e, int jchunk,
                                                                 double* __restrict__ part) {
  rect_mm_part<TRANS ? MM_TRANS : MM_DIRECT, true>(G, q, proxies, n, c, e, jchunk, part);
}

__global__ __launch_bounds__(256) void proxy_bwd_emb_sum_kernel(const double* __restrict__ part, int splits, long ne,
                                                                const float* __restrict__ upstream, float* __restrict__ demb) {
  rect_mm_sum<false>(part, splits, ne, 1, upstream, demb);
}

template <bool TRANS>
__global__ __launch_bounds__(256) void proxy_bwd_y_kernel(const float* __restrict__ G, const float* __restrict__ emb, int n, int c,
                                                          int e, double* __restrict__ y) {
  mm_f64_tile<TRANS ? MM_TRANS : MM_DIRECT, false>(G, nullptr, emb, c, n, e, 0, n, RectF64Out{y});
}

// a wave per class: t = Y_c . w_c (lane-strided f64 chains + butterfly), dproxies_c = g q (Y_c - q^2 t w_c)
__global__ __launch_bounds__(RECT_THREADS) void proxy_bwd_proxies_kernel(const double* __restrict__ y, const float* __restrict__ proxies,
                                                                         const float* __restrict__ q, int c, int e,
                                                                         const float* __restrict__ upstream,
                                                                         float* __restrict__ dproxies) {
  const int lane = threadIdx.x & 63;
  const int cl = blockIdx.x * RECT_WG_ANCHORS + (threadIdx.x >> 6);
  if (cl >= c) return;                                   // wave-uniform
  const double* yr = y + (long)cl * e;
  const float* wr = proxies + (long)cl * e;
  double t = 0.0;
  for (int k = lane; k < e; k += 64) t = fma(yr[k], (double)wr[k], t);
  t = wave_sum(t);
  const double qc = (double)q[cl];
  const double gq = (upstream ? (double)*upstream : 1.0) * qc;
  const double f = qc * qc * t;
  for (int k = lane; k < e; k += 64) dproxies[(long)cl * e + k] = (float)(gq * (yr[k] - f * (double)wr[k]));
}

// ---- host side: range, path rule, workspace layout ---------------------------------------------------------------------------------
inline bool proxy_range_ok(int n, int c, int e) {
  return n >= 2 && n <= PROXY_MAX_N && c >= 2 && c <= PROXY_MAX_C && e >= 1 && e <= PROXY_MAX_E;
}

inline bool proxy_small_fits(int n, int c, int e) {       // either side of the rectangle as the anchors
  return rect_small_fits(n < c ? n : c, n > c ? n : c, e);
}

// [16 B ticket][c int32 class sizes][m double2 partial losses][m int4 partial counts][c*n f32 D][c*e f64 Y], m = max(n, c)
struct ProxyWorkspace {
  size_t cnt, part_loss, part_cnt, d, y, bytes;
  ProxyWorkspace(int n, int c, int e) {
    const size_t m = (size_t)(n > c ? n : c);
    cnt = 16;
    part_loss = cnt + pair_align16((size_t)c * 4);
    part_cnt = part_loss + m * 16;
    d = part_cnt + m * 16;
    y = d + pair_align16((size_t)c * n * 4);
    bytes = y + pair_align16((size_t)c * e * 8);
  }
};

// The backward's launches on checked arguments, in two steps so that multi_proxy_loss.hip (the CosFace case over c kc rows) can add its
// regulariser's term to Y between them.  products: demb, and Y = G^(T) X in f64 into y [c][e].  pa: G is [c][n] (transposed for
// demb's rows, direct for Y's), else [n][c].  demb's class sum is split towards 1024 workgroups; the slices' f64 sums (splits n e
// doubles) live where Y is written afterwards (c e doubles), so splits n <= c.
void proxy_bwd_products(const float* emb, const float* proxies, int n, int c, int e, bool pa, const float* pair_g, const float* q,
                        const float* upstream, float* demb, double* y, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const double flop = 2.0 * n * c * e, gbytes = 4.0 * n * c, ebytes = gbytes + 4.0 * e * (c + n);
  int splits, jchunk;
  rect_mm_split(n, c, e, 1024, c / n, splits, jchunk);
  rect_mm_launch({"embnet::proxy_bwd_emb_kernel", "embnet::proxy_bwd_emb_part_kernel", "embnet::proxy_bwd_emb_sum_kernel"}, flop, ebytes,
                 ebytes, n, e, splits, stream,
                 [&](dim3 grid) {
                   if (pa) proxy_bwd_emb_kernel<true><<<grid, 256, 0, s>>>(pair_g, q, proxies, n, c, e, upstream, demb);
                   else proxy_bwd_emb_kernel<false><<<grid, 256, 0, s>>>(pair_g, q, proxies, n, c, e, upstream, demb);
                 },
                 [&](dim3 grid) {
                   if (pa) proxy_bwd_emb_part_kernel<true><<<grid, 256, 0, s>>>(pair_g, q, proxies, n, c, e, jchunk, y);
                   else proxy_bwd_emb_part_kernel<false><<<grid, 256, 0, s>>>(pair_g, q, proxies, n, c, e, jchunk, y);
                 },
                 [&](int grid) { proxy_bwd_emb_sum_kernel<<<grid, 256, 0, s>>>(y, splits, (long)n * e, upstream, demb); });
  EMBNET_TRACE_FLOP("embnet::proxy_bwd_y_kernel", flop, gbytes + 4.0 * e * n + 8.0 * e * c, stream);
  const dim3 gy(cdiv(c, 32), cdiv(e, 32));
  if (pa) proxy_bwd_y_kernel<false><<<gy, 256, 0, s>>>(pair_g, emb, n, c, e, y);
  else proxy_bwd_y_kernel<true><<<gy, 256, 0, s>>>(pair_g, emb, n, c, e, y);
}

// project: dproxies_c = g q_c (Y_c - q_c^2 (Y_c . w_c) w_c)
void proxy_bwd_project(const double* y, const float* proxies, const float* q, int c, int e, const float* upstream, float* dproxies,
                       void* stream) {
  EMBNET_TRACE("embnet::proxy_bwd_proxies_kernel", TRACE_BYTES, 16.0 * c * e, stream);
  proxy_bwd_proxies_kernel<<<cdiv(c, RECT_WG_ANCHORS), RECT_THREADS, 0, (hipStream_t)stream>>>(y, proxies, q, c, e, upstream, dproxies);
}

inline int proxy_check_common(const char* what, bool pointers, int n, int c, int e, int kind, const void* workspace,
                              size_t workspace_bytes) {
  EMBNET_CHECK_ARG(pointers, "%s: null pointer", what);
  EMBNET_CHECK_ARG(n >= 2 && n <= PROXY_MAX_N, "%s: n=%d outside [2, %d]", what, n, PROXY_MAX_N);
  EMBNET_CHECK_ARG(c >= 2 && c <= PROXY_MAX_C, "%s: c=%d outside [2, %d]", what, c, PROXY_MAX_C);
  EMBNET_CHECK_ARG(e >= 1 && e <= PROXY_MAX_E, "%s: e=%d outside [1, %d]", what, e, PROXY_MAX_E);
  EMBNET_CHECK_ARG(kind == EMBNET_PROXY_ANCHOR || kind == EMBNET_PROXY_SOFTMAX, "%s: unknown kind %d", what, kind);
  return check_workspace(what, workspace, workspace_bytes, ProxyWorkspace(n, c, e).bytes);
}

}  // namespace embnet

using namespace embnet;

extern "C" size_t embnet_proxy_loss_workspace_bytes(int n, int c, int e) {
  return proxy_range_ok(n, c, e) ? ProxyWorkspace(n, c, e).bytes : 0;
}

extern "C" int embnet_proxy_loss_path(int n, int c, int e) {
  if (!proxy_range_ok(n, c, e)) return 0;
  return proxy_small_fits(n, c, e) ? EMBNET_PROXY_SMALL : EMBNET_PROXY_MATRIX;
}

extern "C" int embnet_proxy_loss_fwd(const float* emb, const float* proxies, const int32_t* labels, int n, int c, int e, int kind,
                                     float a, float b, int path, float* pair_g, float* q, int32_t* counts, float* mean_loss,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "proxy_loss_fwd";
  EMBNET_CHECK_ARG(path >= 0 && path <= EMBNET_PROXY_MATRIX, "%s: unknown path %d", what, path);
  EMBNET_CHECK_ARG(isfinite(a) && a > 0.f, "%s: %s=%g must be finite and positive", what, kind == EMBNET_PROXY_SOFTMAX ? "scale" : "alpha",
                   (double)a);
  EMBNET_CHECK_ARG(isfinite(b), "%s: %s=%g must be finite", what, kind == EMBNET_PROXY_SOFTMAX ? "margin" : "delta", (double)b);
  const int rc = proxy_check_common(what, emb && proxies && labels && pair_g && q && counts && mean_loss && workspace, n, c, e, kind,
                                    workspace, workspace_bytes);
  if (rc != EMBNET_OK) return rc;
  EMBNET_CHECK_ARG(path != EMBNET_PROXY_SMALL || proxy_small_fits(n, c, e), "%s: n=%d c=%d e=%d does not fit the small path", what, n,
                   c, e);
  if (path == 0) path = embnet_proxy_loss_path(n, c, e);
  const ProxyWorkspace L(n, c, e);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  float* d = (float*)(ws + L.d);
  const bool pa = kind == EMBNET_PROXY_ANCHOR;
  const int na = pa ? c : n, nb = pa ? n : c;
  ProxyParams P{pa ? proxies : emb, pa ? emb : proxies, labels, q, cnt, na, nb, e, n, c, kind, a, b, pair_g, counts, mean_loss,
                (int*)ws, (double2*)(ws + L.part_loss), (int4*)(ws + L.part_cnt), d};
  {
    EMBNET_TRACE("embnet::proxy_prep_kernel", TRACE_BYTES, 4.0 * c * e + 4.0 * n + 8.0 * c, stream);
    proxy_prep_kernel<<<cdiv(c, RECT_WG_ANCHORS), RECT_THREADS, 0, s>>>(proxies, labels, n, c, e, q, cnt);
  }
  return rect_launch(what, proxy_small_fwd_kernel, "embnet::proxy_small_fwd_kernel", proxy_sweep_kernel, "embnet::proxy_sweep_kernel",
                     path == EMBNET_PROXY_SMALL, P, P.anchors, P.others, d, na, nb, e, stream);
}

extern "C" int embnet_proxy_loss_bwd(const float* emb, const float* proxies, int n, int c, int e, int kind, const float* pair_g,
                                     const float* q, const float* upstream, float* demb, float* dproxies, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  const char* what = "proxy_loss_bwd";
  const int rc = proxy_check_common(what, emb && proxies && pair_g && q && demb && dproxies && workspace, n, c, e, kind, workspace,
                                    workspace_bytes);
  if (rc != EMBNET_OK) return rc;
  double* y = (double*)((char*)workspace + ProxyWorkspace(n, c, e).y);
  proxy_bwd_products(emb, proxies, n, c, e, kind == EMBNET_PROXY_ANCHOR, pair_g, q, upstream, demb, y, stream);
  proxy_bwd_project(y, proxies, q, c, e, upstream, dproxies, stream);
  return check_launch(what);
}
