// Batch-all triplet loss (Moindrot; Hermans et al. name it next to batch-hard): every valid triplet of a class-contiguous
// P x K batch takes part, the loss is the mean over the triplets that violate the margin.  Build-defined: the reference
// cites both batch strategies (README [2], [4]) and implements neither.
//
//   X [N, E] fp32, N = P*K, rows c*K .. c*K+K-1 are class c.  d(i,j) = sum_c (x_ic - x_jc)^2 (the squared-L2 quantity of
//   triplet_gather_fwd).  Valid (a,p,n): p in a's class, p != a, n in another class; T = N (K-1) (N-K) of them.
//   b = (d(a,p) - d(a,n)) + margin; a triplet is ACTIVE iff b > 0 (strict: the selection rules' `active` flags use b >= 0).
//   A = #active;  loss = sum_active b / max(A, 1);  frac_active = A / T.
//   W[a,p] = #{n : (a,p,n) active},  W[a,n] = -#{p : (a,p,n) active},  0 elsewhere (small integers, exact in fp32).
//   backward, A held constant:  demb_i = (2 g / max(A,1)) * sum_j M_ij (x_i - x_j),  M = W + W^T
//                                      = (2 g / max(A,1)) * (s_i x_i - (M X)_i),   s_i = sum_j M_ij.
//
// Forward, per-class path (N <= 512, K <= 16, K (E + N) floats in 64 KiB of LDS: C1, C2, C5 and the shipped configs), ONE
// launch: a workgroup per class holds its K rows and their K x N distance rows (difference form) in LDS, one wave per anchor
// sweeps (K-1) positives x (N-K) negatives and writes the anchor's row of W (rows belong to their anchor: no atomics), the
// workgroup writes a per-class partial (f64 sum of b, count), and the last workgroup to arrive (agent-scope ticket, the
// hand-off of fused_loss.hip) reduces the partials in class order.
// Forward, distance-matrix path (everything else up to N = 4096, E = 4096): the per-class block would re-read all N rows per
// class (N^2 E / K bytes from L2), so the squared distances come from embnet_pairwise_dist_f32(squared = 1) into the
// workspace (the Gram form: its rounding differs from the difference form) and a sweep kernel takes one anchor row per wave,
// with the same partial / ticket / fixed-order reduction over anchors.
// Backward, one launch: Y = M X on the f64 matrix instructions (v_mfma_f64_16x16x4_f64) with the epilogue
// demb = (2g/A)(s x - Y).  Not the f32 ones: an f32 chain over j rounds relative to sum_j |M_ij| |x_j|, while the gradient is
// a sum of differences (x_i - x_j) whose size can be far below that (same-class rows are close); M is integer and x fp32, so
// every f64 product is exact and the result carries one fp32 rounding relative to sum_j |M_ij| |x_i - x_j|.
// Nothing is atomic in floating point, every reduction has a fixed order: bitwise reproducible.  No host synchronisation, no
// allocation: capturable in a graph.
// The skeleton (pair-matrix staging, row copy, ticket, reduction, workspace, fit rule, the backward's product) is pair_loss.h's,
// shared with multi_similarity.hip and supcon.hip; this file holds the per-anchor body, the epilogue and the kernels' names.
#include "common.h"
#include "pair_loss.h"
#include "../../include/embnet.h"

namespace embnet {

static_assert(EMBNET_BATCH_ALL_PER_CLASS == PAIR_PER_CLASS && EMBNET_BATCH_ALL_DISTANCE_MATRIX == PAIR_MATRIX, "path constants");

__device__ __forceinline__ float ba_b(float dap, float dan, float margin) {   // one rounding order everywhere
  return __fadd_rn(__fsub_rn(dap, dan), margin);
}

// Counts: ba_range_ok admits only T <= 2^31 - 1, and every partial count and every running sum of them is non-negative and at
// most T, so the skeleton's int counters are exact.
struct BatchAllBody {
  struct Args { float margin; float* frac; long long t_total; };
  using Sum = double;
  static constexpr int CLASS_TRACE_UNIT = TRACE_BYTES;

  static __device__ float term(float a, float y, float acc) { const float d = a - y; return fmaf(d, d, acc); }   // difference form
  static int matrix(const float* emb, int n, int e, float* dist, void* extra, void* stream) {
    return embnet_pairwise_dist_f32(emb, n, e, dist, 1, extra, pair_align16(embnet_pairwise_workspace_bytes(n, e)), stream);
  }
  static size_t matrix_extra_bytes(int n, int e) { return embnet_pairwise_workspace_bytes(n, e); }

  // One wave, one anchor (local index ai of class [lo, lo+k)), its squared-distance row drow[n] (LDS).  Writes the anchor's
  // row of W and returns the wave's f64 sum of active b (fixed order) and its active count.
  static __device__ PairAnchorOut<double> anchor(const float* drow, int n, int k, int lo, int ai, const Args& a, float* wrow,
                                                 int lane) {
    const float margin = a.margin;
    double s = 0.0;
    int c = 0;
    for (int col = lane; col < n; col += 64) {             // negatives: W[a,n] = -#{p : active}
      if (col >= lo && col < lo + k) continue;
      const float dan = drow[col];
      int cn = 0;
      for (int j = 0; j < k; ++j) {
        if (j == ai) continue;
        const float b = ba_b(drow[lo + j], dan, margin);
        if (b > 0.f) { ++cn; s += (double)b; }
      }
      wrow[col] = -(float)cn;
      c += cn;
    }
    for (int j = 0; j < k; ++j) {                          // positives: W[a,p] = #{n : active}; W[a,a] = 0
      int cp = 0;
      if (j != ai) {
        const float dap = drow[lo + j];
        for (int col = lane; col < n; col += 64)
          if ((col < lo || col >= lo + k) && ba_b(dap, drow[col], margin) > 0.f) ++cp;
      }
      cp = wave_sum(cp);
      if (lane == 0) wrow[lo + j] = (float)cp;
    }
    const double sum = wave_sum(s);
    return PairAnchorOut<double>{sum, wave_sum(c), 0};     // count <= (K-1)(N-K) < 2^23
  }
  static __device__ int third(const PairAnchorOut<double>&) { return 0; }
  static __device__ void finish(const PairParams<BatchAllBody>& q, double total, int active, int, int) {
    *q.counts = active;
    *q.a.frac = (float)((double)active / (double)q.a.t_total);
    *q.mean = (float)(total / (double)(active > 0 ? active : 1));
  }
};
using BatchAllParams = PairParams<BatchAllBody>;

__global__ __launch_bounds__(PAIR_CLASS_THREADS) void batch_all_class_fwd_kernel(BatchAllParams q) { pair_class_fwd<BatchAllBody>(q); }
__global__ __launch_bounds__(PAIR_SWEEP_THREADS) void batch_all_sweep_kernel(BatchAllParams q) { pair_sweep_fwd<BatchAllBody>(q); }

// ---- backward: demb = (2g / max(A,1)) (s x - M X), M = W + W^T; M is integer, so s and every f64 product are exact -----------
struct BatchAllEpilogue {
  static constexpr bool ROW_SUM = true;
  const int32_t* n_active; const float* upstream;
  __device__ double scale(int) const {
    const int cnt = *n_active;
    const double g = upstream ? (double)*upstream : 1.0;
    return 2.0 * g / (double)(cnt > 0 ? cnt : 1);
  }
  __device__ double value(double scale, double y, double s, const float* x) const { return scale * (s * (double)*x - y); }
};

__global__ __launch_bounds__(256) void batch_all_bwd_kernel(const float* __restrict__ emb, int n, int e,
                                                           const float* __restrict__ w, const int32_t* __restrict__ n_active,
                                                           const float* __restrict__ upstream, float* __restrict__ demb) {
  pair_bwd(emb, n, e, w, BatchAllEpilogue{n_active, upstream}, demb);
}

static bool ba_range_ok(int p, int k, int e) {           // the pair range, and T = N (K-1) (N-K) an int32
  const long long n = (long long)p * k;
  return pair_range_ok(p, k, e) && n * (k - 1) * (n - k) <= 0x7fffffffLL;
}

}  // namespace embnet

using namespace embnet;

// workspace: pair_loss.h's layout, the squared distances as the pair matrix, embnet_pairwise_dist_f32's workspace behind them
extern "C" size_t embnet_batch_all_workspace_bytes(int p, int k, int e) {
  return ba_range_ok(p, k, e) ? pair_workspace_bytes<BatchAllBody>(p, k, e) : 0;
}

extern "C" int embnet_batch_all_path(int p, int k, int e) { return ba_range_ok(p, k, e) ? pair_path(p, k, e) : 0; }

extern "C" int embnet_batch_all_loss_fwd(const float* emb, int p, int k, int e, float margin, int path, float* pair_w,
                                         int32_t* n_active, float* frac_active, float* mean_loss, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  int rc = pair_check_common("batch_all_loss_fwd", emb && pair_w && n_active && frac_active && mean_loss && workspace, p, k, e);
  if (rc != EMBNET_OK) return rc;
  EMBNET_CHECK_ARG(ba_range_ok(p, k, e), "batch_all_loss_fwd: p=%d k=%d has more than 2^31-1 triplets", p, k);
  rc = pair_check_path_and_workspace("batch_all_loss_fwd", p, k, e, path, workspace, workspace_bytes,
                                     embnet_batch_all_workspace_bytes(p, k, e));
  if (rc != EMBNET_OK) return rc;
  const long long n = (long long)p * k;
  static const PairKernels<BatchAllBody> kernels{batch_all_class_fwd_kernel, "embnet::batch_all_class_fwd_kernel",
                                                 batch_all_sweep_kernel, "embnet::batch_all_sweep_kernel"};
  return pair_launch<BatchAllBody>("batch_all_loss_fwd", kernels, emb, p, k, e, {margin, frac_active, n * (k - 1) * (n - k)}, path,
                                   pair_w, n_active, mean_loss, workspace, stream);
}

extern "C" int embnet_batch_all_loss_bwd(const float* emb, int n, int e, const float* pair_w, const int32_t* n_active,
                                         const float* upstream, float* demb, void* stream) {
  const int rc = pair_check_bwd("batch_all_loss_bwd", emb && pair_w && n_active && demb, n, e);
  if (rc != EMBNET_OK) return rc;
  EMBNET_TRACE_FLOP("embnet::batch_all_bwd_kernel", 2.0 * n * n * e, 4.0 * (2.0 * n * n + 2.0 * n * e), stream);
  batch_all_bwd_kernel<<<dim3(cdiv(n, 32), cdiv(e, 32)), 256, 0, (hipStream_t)stream>>>(emb, n, e, pair_w, n_active,
                                                                                           upstream, demb);
  return check_launch("batch_all_loss_bwd");
}
