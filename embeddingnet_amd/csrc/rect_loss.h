// What the losses over a RECTANGLE share, a batch against something else (proxy_loss.hip: class proxies; multi_proxy_loss.hip: kc
// centres per class; xbm.hip: the memory bank), na anchors against nb others, one wave per anchor's row of D [na][nb]:
//   the forward's launches on checked arguments (rect_launch, rect_sweep_launch): the small kernel, or D and then the sweep;
//   the backward's split product on pair_loss.h's mm_f64_tile: where few rows meet a long j the sum is split over blockIdx.z into
//     f64 slices and a second launch adds the slices in slice order, scales and rounds once;
//   what the proxies' two files share: the limits, a row's q, the backward's launches (defined in proxy_loss.hip).
// The row bodies and the forward kernels' scaffold stay in the loss's own file: written over one Body they measured 1 - 3 % slower
// (DESIGN.md f-13b).  The integer workgroup total (block_total256) and check_workspace are common.h's.
#pragma once
#include <math.h>
#include "common.h"
#include "pair_loss.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr int PROXY_MAX_N = 4096;
constexpr int PROXY_MAX_C = 16384;
constexpr int PROXY_MAX_E = 4096;
constexpr int RECT_THREADS = 256;                        // 4 waves: one anchor each
constexpr int RECT_WG_ANCHORS = RECT_THREADS / 64;
constexpr int RECT_LDS_FLOATS = 16 * 1024;               // small path: 4 (e + nb) floats
constexpr long RECT_SMALL_MACS = 1L << 25;               // small path: na nb e, every workgroup re-reads all of B from L2

inline bool rect_small_fits(long na, long nb, int e) {
  return RECT_WG_ANCHORS * (e + nb) <= RECT_LDS_FLOATS && na * nb * e <= RECT_SMALL_MACS;
}

// The forward's launches on checked arguments: D = anchors others^T into d, then the sweep under the caller's trace entry ...
template <class Body>
inline int rect_sweep_launch(const char* what, void (*sweep)(Body), const char* sweep_name, double sweep_bytes, const Body& b,
                             const float* anchors, const float* others, float* d, int na, int nb, int e, void* stream) {
  const int rg = embnet_dense_dgrad_f32(anchors, others, d, na, nb, e, stream);
  if (rg != EMBNET_OK) return rg;
  EMBNET_TRACE(sweep_name, TRACE_BYTES, sweep_bytes, stream);
  sweep<<<cdiv(na, RECT_WG_ANCHORS), RECT_THREADS, 0, (hipStream_t)stream>>>(b);
  return check_launch(what);
}

// ... or, where the caller says so, the small kernel alone.  The kernels go under the names their trace entries carry.
template <class Body>
inline int rect_launch(const char* what, void (*small_fwd)(Body), const char* small_name, void (*sweep)(Body), const char* sweep_name,
                       bool small, const Body& b, const float* anchors, const float* others, float* d, int na, int nb, int e,
                       void* stream) {
  if (!small) return rect_sweep_launch(what, sweep, sweep_name, 16.0 * na * nb, b, anchors, others, d, na, nb, e, stream);
  const int grid = cdiv(na, RECT_WG_ANCHORS);
  EMBNET_TRACE_FLOP(small_name, 2.0 * na * nb * e, 4.0 * e * (na + (double)grid * nb) + 4.0 * na * nb, stream);
  small_fwd<<<grid, RECT_THREADS, 0, (hipStream_t)stream>>>(b);
  return check_launch(what);
}

// ---- backward: the split product --------------------------------------------------------------------------------------------------------
// mm_f64_tile's Outs of a rectangle: the f64 sums as they are (a slice, or a result that stays f64) ...
struct RectF64Out {
  static constexpr bool ROW_SUM = false;
  double* out;
  __device__ double begin() const { return 0.0; }
  __device__ void put(double, long at, double y, double) const { out[at] = y; }
};

// ... or scaled and rounded once: (float)(g y), MEAN: (float)(g / n y); g = *upstream, NULL = 1
template <bool MEAN>
struct RectScaledOut {
  static constexpr bool ROW_SUM = false;
  const float* upstream; int n; float* out;
  __device__ double begin() const {
    const double g = upstream ? (double)*upstream : 1.0;
    if constexpr (MEAN) return g / (double)n;
    else return g;
  }
  __device__ void put(double scale, long at, double y, double) const { out[at] = (float)(scale * y); }
};

// slice blockIdx.z sums j in [z jchunk, (z + 1) jchunk) into part[z][R][e] ...
template <int LEFT, bool SCALE>
__device__ __forceinline__ void rect_mm_part(const float* __restrict__ G, const float* __restrict__ qv, const float* __restrict__ B,
                                             int R, int J, int e, int jchunk, double* __restrict__ part) {
  const int jb = blockIdx.z * jchunk;
  mm_f64_tile<LEFT, SCALE>(G, qv, B, R, J, e, jb, min(J, jb + jchunk), RectF64Out{part + (long)blockIdx.z * R * e});
}

// ... and the slices are added in slice order, scaled and rounded once: a thread per element, 256 threads
template <bool MEAN>
__device__ __forceinline__ void rect_mm_sum(const double* __restrict__ part, int splits, long ne, int n,
                                            const float* __restrict__ upstream, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= ne) return;
  double s = 0.0;
  for (int z = 0; z < splits; ++z) s += part[z * ne + i];
  const RectScaledOut<MEAN> o{upstream, n, out};
  o.put(o.begin(), i, s, 0.0);
}

// The split rule of a product of r rows over j: none while a slice would hold fewer than 256 of j; otherwise towards `target`
// workgroups, at most `cap` slices (the caller's scratch holds splits r e doubles).  -> (splits, jchunk), jchunk a multiple of 32
inline void rect_mm_split(int r, int j, int e, int target, int cap, int& splits, int& jchunk) {
  int s = cdiv(target, (long)cdiv(r, 32) * cdiv(e, 32));
  if (s > j / 256) s = j / 256;
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  jchunk = cdiv(cdiv(j, s), 32) * 32;
  splits = cdiv(j, jchunk);
}

// The product's launches, r rows and e columns: unsplit (whole(grid)), or part(grid with splits in z) and then sum(grid) over the
// caller's scratch.  names: the three kernels' trace entries; the callers' byte counts differ, the sum's does not.
template <class Whole, class Part, class Sum>
inline void rect_mm_launch(const char* const (&names)[3], double flop, double whole_bytes, double part_bytes, int r, int e, int splits,
                           void* stream, Whole whole, Part part, Sum sum) {
  const dim3 grid(cdiv(r, 32), cdiv(e, 32));
  if (splits == 1) {
    EMBNET_TRACE_FLOP(names[0], flop, whole_bytes, stream);
    whole(grid);
    return;
  }
  {
    EMBNET_TRACE_FLOP(names[1], flop, part_bytes, stream);
    part(dim3(grid.x, grid.y, splits));
  }
  EMBNET_TRACE(names[2], TRACE_BYTES, 8.0 * splits * r * e + 4.0 * r * e, stream);
  sum(cdiv((long)r * e, 256));
}

// ---- what the proxies' two files share ----------------------------------------------------------------------------------------------------
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

// The backward on checked arguments, in two steps (proxy_loss.hip says what they do).  y holds c e doubles.
void proxy_bwd_products(const float* emb, const float* proxies, int n, int c, int e, bool pa, const float* pair_g, const float* q,
                        const float* upstream, float* demb, double* y, void* stream);
void proxy_bwd_project(const double* y, const float* proxies, const float* q, int c, int e, const float* upstream, float* dproxies,
                       void* stream);

}  // namespace embnet
