// What proxy_loss.hip (one vector per class) and multi_proxy_loss.hip (kc centres per class: the CosFace rectangle over c kc rows)
// share: the limits and the path constants, a row's q, and the backward's launches (defined in proxy_loss.hip).
#pragma once
#include <math.h>
#include "common.h"

namespace embnet {

constexpr int PROXY_MAX_N = 4096;
constexpr int PROXY_MAX_C = 16384;
constexpr int PROXY_MAX_E = 4096;
constexpr int PROXY_THREADS = 256;                       // 4 waves: one anchor each
constexpr int PROXY_WG_ANCHORS = PROXY_THREADS / 64;
constexpr int PROXY_LDS_FLOATS = 16 * 1024;              // small path: 4 (e + nb) floats
constexpr long PROXY_SMALL_MACS = 1L << 25;              // small path: n c e, every workgroup re-reads all of B from L2

// q = (float)(1 / sqrt(sum_k r_k^2)), 0 for a zero row, by the calling wave (the same in every lane).  The wave reads 64 consecutive
// elements of the row at a time (coalesced) and squares them in f64, which is exact; the chain over k is contractual, so every lane
// then adds the 64 squares in lane order, taken from the other lanes one by one: the same f64 additions in the same order as a
// serial loop, and past the row's end exact zeros.
__device__ __forceinline__ float proxy_row_q(const float* __restrict__ r, int e, int lane) {
  double ss = 0.0;
  for (int k0 = 0; k0 < e; k0 += 64) {
    const double v = k0 + lane < e ? (double)r[k0 + lane] : 0.0;
    const double v2 = v * v;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) ss += __shfl(v2, j, 64);
  }
  return ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f;
}

// The backward on checked arguments (proxy_loss.hip), in two steps: demb and Y = G^(T) X in f64 into y [c][e], then
// dproxies_c = g q_c (Y_c - q_c^2 (Y_c . w_c) w_c).  pa: G is [c][n], else [n][c].  y holds c e doubles.
void proxy_bwd_products(const float* emb, const float* proxies, int n, int c, int e, bool pa, const float* pair_g, const float* q,
                        const float* upstream, float* demb, double* y, void* stream);
void proxy_bwd_project(const double* y, const float* proxies, const float* q, int c, int e, const float* upstream, float* dproxies,
                       void* stream);

}  // namespace embnet
