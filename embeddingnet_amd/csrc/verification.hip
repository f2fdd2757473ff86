// Verification evaluation (ROC AUC, EER, TAR@FAR) without the distance matrix and without a sort: every pair counted into a
// same-class and an other-class histogram of its distance (include/embnet.h, "verification").
//
// all_pairs is ONE walk of retrieval_walk (retrieval_walk.h): the distance, the NaN rule, the exclusion of the query's own
// column, the tile and split plan and the loaders are embnet_retrieval_first_positive's.  Its epilogue CountPairs turns d2 into
// a bin — (int)(d2 * (1 / w)) with 1 / w a power of two, so the product is exact and the bin an exact function of the fp32
// d2 — and adds 1 to a workgroup-private LDS histogram [same | other] with a 32-bit LDS atomic: one atomic per element, whichever
// label it has.  Every `flush_tiles` gallery tiles, and behind the walk, the workgroup adds its non-zero bins to the global u64
// histograms with 64-bit atomics and clears them; a 32-bit counter takes at most flush_tiles * BM * BN <= 2^32 - 1 counts between
// two flushes.  Integer sums commute: the result is independent of scheduling, bitwise reproducible.
// LDS: the walk holds 18.9 KB (64x64) or 37.9 KB (128x128) statically; 2 x 4096 counters are 32 KB of dynamic LDS on top.
// 64x64: 51.7 KB, inside the 64 KB a launch gets by default.  128x128: 70.7 KB, beyond it: every launch goes through
// allow_big_lds (common.h), which asks for the CU's LDS less the kernel's static part.  Two 128x128 workgroups (141 KB) still
// share a CU's 160 KB, as their launch bounds ask.
// values: the same bin function and flush over a vector of per-pair values (pair lists, similarity scores).
// Roofline: all_pairs MFMA f32, 2*nq*n*e FLOP, one LDS atomic per pair; values HBM, 8 bytes per pair.
#include "retrieval_walk.h"
#include <math.h>

namespace embnet {

constexpr int VERIF_MAX_BINS = EMBNET_VERIFICATION_MAX_BINS;

// the workgroup's counters join the global histograms: hist[0 .. bins) same, [bins .. 2 bins) other.  Every thread calls.
__device__ __forceinline__ void verif_flush(unsigned* s_hist, int bins, unsigned long long* __restrict__ hist_same,
                                            unsigned long long* __restrict__ hist_other) {
  __syncthreads();                                         // every wave's counts of the tiles so far are in
  for (int i = threadIdx.x; i < 2 * bins; i += NTHREADS) {
    const unsigned c = s_hist[i];
    if (c != 0u) {
      atomicAdd(i < bins ? &hist_same[i] : &hist_other[i - bins], (unsigned long long)c);
      s_hist[i] = 0u;
    }
  }
  __syncthreads();                                         // cleared before the next tile counts
}

struct CountPairs : WalkEpilogue {
  unsigned* s_hist; unsigned long long* hist_same; unsigned long long* hist_other;
  float inv_w; int bins, flush_tiles, rows;                // rows: the tile's rows below nq (the walk visits the padding rows too)
  __device__ __forceinline__ int visit(int c, int rt, int, int, unsigned long long k, bool live, bool same) const {
    if (live && rt < rows) {
      // d2 >= 0 or +inf (the walk's NaN rule), so truncation is floorf; +inf and everything past the range: the last bin
      const float d2 = __uint_as_float((unsigned)(k >> 32));
      const int b = (int)fminf(d2 * inv_w, (float)(bins - 1));
      atomicAdd(&s_hist[(same ? 0 : bins) + b], 1u);
    }
    return c;
  }
  __device__ static __forceinline__ int half_wave(int c) { return c; }      // nothing is kept per row
  __device__ __forceinline__ void tile_done(int count) const {
    if (count % flush_tiles == 0) verif_flush(s_hist, bins, hist_same, hist_other);    // the same answer in every thread
  }
};

struct VerifParams {
  WalkParams w;
  unsigned long long* hist_same; unsigned long long* hist_other;
  float inv_w; int bins, flush_tiles;
};

// one wave per row: the squared norms of queries and gallery (row_sqnorm, as retrieval_prep_kernel); the grid also zeroes the
// two output histograms — by this kernel, not a memset node, so a replayed graph starts from a clean state
__global__ __launch_bounds__(256) void verif_prep_kernel(const float* __restrict__ q, int nq, const float* __restrict__ x, int n,
                                                         int e, float* qn, float* xn, int bins,
                                                         unsigned long long* __restrict__ hist_same,
                                                         unsigned long long* __restrict__ hist_other) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < bins; i += gridDim.x * 256) { hist_same[i] = 0ull; hist_other[i] = 0ull; }
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row < nq) {
    const float s = row_sqnorm(q + (long)row * e, e);
    if (lane == 0) qn[row] = s;
  }
  if (xn != qn && row < n) {                               // leave-one-out: the host hands qn as xn, the walk reads one vector
                                                           // (a caller's own gallery gets its norms even when it is the query block)
    const float s = row_sqnorm(x + (long)row * e, e);
    if (lane == 0) xn[row] = s;
  }
}

// grid = (query tiles, gallery splits).  Dynamic LDS: 2 * bins counters.
template <class G, bool VEC>
__global__ __launch_bounds__(256, VEC ? 2 : 1) void verif_walk_kernel(VerifParams p) {
  extern __shared__ unsigned s_hist[];
  prio_hi();
  for (int i = threadIdx.x; i < 2 * p.bins; i += NTHREADS) s_hist[i] = 0u;   // published by the walk's first barrier
  retrieval_walk<G, VEC>(p.w, CountPairs{{}, s_hist, p.hist_same, p.hist_other, p.inv_w, p.bins, p.flush_tiles,
                                         p.w.nq - (int)blockIdx.x * G::BM});
  verif_flush(s_hist, p.bins, p.hist_same, p.hist_other);
}

__global__ __launch_bounds__(256) void verif_zero_kernel(int bins, unsigned long long* __restrict__ hist_same,
                                                         unsigned long long* __restrict__ hist_other) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < bins) { hist_same[i] = 0ull; hist_other[i] = 0ull; }
}

// grid-stride over the values; a workgroup sees fewer than 2^31 of them, so its 32-bit counters cannot overflow
__global__ __launch_bounds__(256) void verif_values_kernel(const float* __restrict__ values, const int32_t* __restrict__ same,
                                                           int m, float lo, float inv_w, int bins,
                                                           unsigned long long* __restrict__ hist_same,
                                                           unsigned long long* __restrict__ hist_other) {
  extern __shared__ unsigned s_hist[];
  for (int i = threadIdx.x; i < 2 * bins; i += 256) s_hist[i] = 0u;
  __syncthreads();
  const float top = (float)(bins - 1);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long)gridDim.x * 256) {
    const float v = values[i];
    const float t = floorf((v - lo) * inv_w);
    const int b = v != v ? bins - 1 : (int)fminf(fmaxf(t, 0.f), top);
    atomicAdd(&s_hist[(same[i] != 0 ? 0 : bins) + b], 1u);
  }
  verif_flush(s_hist, bins, hist_same, hist_other);
}

}  // namespace embnet

using namespace embnet;

// a positive power of two that is a normal float, and whose reciprocal is one too
static bool verif_pow2(float v) {
  int ex = 0;
  return v > 0.f && isfinite(v) && frexpf(v, &ex) == 0.5f && ex >= -124 && ex <= 126;
}
static bool verif_bins_ok(int bins) { return bins >= 2 && bins <= VERIF_MAX_BINS && (bins & (bins - 1)) == 0; }

struct VerifWorkspace {
  float* qn; float* xn; size_t bytes;
  VerifWorkspace(void* base, int nq, int n) {
    Bump b{(char*)base};
    qn = b.take<float>(nq); xn = b.take<float>(n);
    bytes = b.used;
  }
};
extern "C" size_t embnet_verification_all_pairs_workspace_bytes(int nq, int n) {
  return nq <= 0 || n <= 0 ? 0 : VerifWorkspace(nullptr, nq, n).bytes;
}

// the largest flush interval that cannot overflow a 32-bit counter of a workgroup with tile x tile elements per gallery tile
static int verif_max_flush_tiles(int tile) { return (int)(0xffffffffull / ((unsigned long long)tile * tile)); }

extern "C" int embnet_verification_all_pairs(const float* q, const int32_t* q_labels, int nq,
                                             const float* x, const int32_t* x_labels, int n, int e, int bins, float d2_max,
                                             int flush_tiles, uint64_t* hist_same, uint64_t* hist_other,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  EMBNET_CHECK_ARG(q && q_labels && hist_same && hist_other && workspace, "verification_all_pairs: null pointer");
  EMBNET_CHECK_ARG((x == nullptr) == (x_labels == nullptr), "verification_all_pairs: x and x_labels come together");
  EMBNET_CHECK_ARG(nq > 0 && n > 0 && e > 0, "verification_all_pairs: nq=%d n=%d e=%d must be positive", nq, n, e);
  const bool loo = x == nullptr;
  EMBNET_CHECK_ARG(!loo || nq == n, "verification_all_pairs: leave-one-out (x == NULL) needs nq == n (nq=%d n=%d)", nq, n);
  EMBNET_CHECK_ARG((size_t)nq * e * 4 <= MAX_OPERAND_BYTES && (size_t)n * e * 4 <= MAX_OPERAND_BYTES,
                   "verification_all_pairs: an embedding block exceeds 2 GiB");
  EMBNET_CHECK_ARG(verif_bins_ok(bins), "verification_all_pairs: bins=%d must be a power of two in [2, %d]", bins, VERIF_MAX_BINS);
  EMBNET_CHECK_ARG(verif_pow2(d2_max) && verif_pow2(d2_max / (float)bins),
                   "verification_all_pairs: d2_max=%g must be a positive power of two", (double)d2_max);
  EMBNET_CHECK_ARG(flush_tiles >= 0, "verification_all_pairs: flush_tiles=%d must not be negative", flush_tiles);
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "verification_all_pairs: workspace must be 16-byte aligned");
  EMBNET_CHECK_ARG(((reinterpret_cast<uintptr_t>(hist_same) | reinterpret_cast<uintptr_t>(hist_other)) & 7) == 0,
                   "verification_all_pairs: the histograms must be 8-byte aligned");
  if (loo) { x = q; x_labels = q_labels; }
  const VerifWorkspace w(workspace, nq, n);
  if (workspace_bytes < w.bytes)
    return fail(EMBNET_EWORKSPACE, "verification_all_pairs: workspace %zu < %zu bytes", workspace_bytes, w.bytes);

  WalkSetup su{{q, x, w.qn, loo ? w.qn : w.xn, q_labels, x_labels, nullptr, nullptr, nq, n, e, loo ? 1 : 0, 0}};
  int splits;
  retrieval_plan(nq, n, su.big, splits, su.w.tiles_per_split);
  const int tile = su.big ? 128 : 64, most = verif_max_flush_tiles(tile);
  EMBNET_CHECK_ARG(flush_tiles <= most, "verification_all_pairs: flush_tiles=%d above %d would overflow a 32-bit counter of a %dx%d tile",
                   flush_tiles, most, tile, tile);
  su.vec = (e & 3) == 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
  su.grid = dim3(cdiv(nq, tile), splits);

  hipStream_t s = (hipStream_t)stream;
  unsigned long long* hs = (unsigned long long*)hist_same;
  unsigned long long* ho = (unsigned long long*)hist_other;
  {
    EMBNET_TRACE("embnet::verif_prep_kernel", TRACE_BYTES, 4.0 * ((double)nq * e + (loo ? 0.0 : (double)n * e)) + 16.0 * bins, s);
    verif_prep_kernel<<<cdiv(nq > n ? nq : n, 4), 256, 0, s>>>(q, nq, x, n, e, w.qn, loo ? w.qn : w.xn, bins, hs, ho);
  }
  const VerifParams p{su.w, hs, ho, (float)bins / d2_max, bins, flush_tiles > 0 ? flush_tiles : most};
  const size_t lds = (size_t)2 * bins * sizeof(unsigned);
  auto launch = [&](auto g, auto vec, auto) {
    using G = decltype(g);
    constexpr auto kernel = verif_walk_kernel<G, decltype(vec)::value>;
    // the walk's own LDS (operand tiles, the rows' norms and labels) is static: the opt-in covers the dynamic rest of the CU's
    allow_big_lds<kernel, (MAIN_FLOATS<TileKC<G::BM>, TileKC<G::BN>> + 2 * G::BM) * 4>();
    kernel<<<su.grid, 256, lds, s>>>(p);
  };
  walk_dispatch(su, 1, "embnet::verif_walk_kernel", 8.0 * ((double)nq + n) + 16.0 * bins, s, launch);
  return check_launch("verification_all_pairs");
}

extern "C" int embnet_verification_values(const float* values, const int32_t* same, int m, float lo, float w, int bins,
                                          uint64_t* hist_same, uint64_t* hist_other, void* stream) {
  EMBNET_CHECK_ARG(hist_same && hist_other && (m == 0 || (values && same)), "verification_values: null pointer");
  EMBNET_CHECK_ARG(m >= 0, "verification_values: m=%d must not be negative", m);
  EMBNET_CHECK_ARG(verif_bins_ok(bins), "verification_values: bins=%d must be a power of two in [2, %d]", bins, VERIF_MAX_BINS);
  EMBNET_CHECK_ARG(verif_pow2(w), "verification_values: w=%g must be a positive power of two", (double)w);
  EMBNET_CHECK_ARG(isfinite(lo), "verification_values: lo must be finite");
  EMBNET_CHECK_ARG(((reinterpret_cast<uintptr_t>(hist_same) | reinterpret_cast<uintptr_t>(hist_other)) & 7) == 0,
                   "verification_values: the histograms must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* hs = (unsigned long long*)hist_same;
  unsigned long long* ho = (unsigned long long*)hist_other;
  {
    EMBNET_TRACE("embnet::verif_zero_kernel", TRACE_BYTES, 16.0 * bins, s);
    verif_zero_kernel<<<cdiv(bins, 256), 256, 0, s>>>(bins, hs, ho);
  }
  if (m > 0) {
    const int grid = cdiv(m, 256) < 512 ? cdiv(m, 256) : 512;
    EMBNET_TRACE("embnet::verif_values_kernel", TRACE_BYTES, 8.0 * m + 16.0 * bins, s);
    verif_values_kernel<<<grid, 256, (size_t)2 * bins * sizeof(unsigned), s>>>(values, same, m, lo, 1.f / w, bins, hs, ho);
  }
  return check_launch("verification_values");
}
