// Multi-similarity loss (Wang et al., CVPR 2019; the pair-based baseline of "A Metric Learning Reality Check") over a
// class-contiguous P x K batch.  Build-defined: the reference has no pair-based loss.  Semantics: include/embnet.h.
//
//   X [N, E] fp32, N = P*K, rows c*K .. c*K+K-1 are class c.  S_ij = sum_c x_ic x_jc (cosine similarity of unit rows; unit rows
//   are not required).  Anchor i: positives P_i = the other rows of its class, negatives N_i = the rows of other classes.
//   Mining, one rounding form: n kept iff fl(S_in + eps) > min_p S_ip;  p kept iff fl(max_n S_in + eps) > S_ip.  fl is
//   monotone, so an anchor keeps a positive AND a negative (it is ACTIVE) or nothing.
//   t+_p = -alpha (S_ip - base), t-_n = beta (S_in - base);  m = max(0, max t) per side;
//   l_i = (m+ + log(e^{-m+} + sum_p e^{t+_p - m+})) / alpha + (m- + log(e^{-m-} + sum_n e^{t-_n - m-})) / beta   (0 if inactive)
//   loss = (1/N) sum_i l_i;   G[i,p] = -e^{t+_p - m+} / (e^{-m+} + sum),  G[i,n] = +e^{t-_n - m-} / (e^{-m-} + sum), 0 elsewhere.
//   backward, kept sets held constant:  demb_i = (g / N) sum_j (G_ij + G_ji) x_j.
//   counts = {kept positives, kept negatives, active anchors, kept positives + kept negatives}, exact.
//
// The skeleton (similarity staging, row copy, ticket, reduction, workspace, fit rule, the backward's product) is pair_loss.h's,
// shared with batch_all.hip and supcon.hip; this file holds the per-anchor body, the epilogue and the kernels' names.
// Forward, per-class path (N <= 512, K <= 16, K (E + N) floats in 64 KiB of LDS), ONE launch: a
// workgroup per class holds its K rows and their K x N similarity rows in LDS (per-lane fmaf chain over the columns + wave sum),
// one wave per anchor mines, sums and writes the anchor's row of G (rows belong to their anchor: no atomics), the workgroup writes
// a per-class partial and the last workgroup to arrive (agent-scope ticket, the hand-off of fused_loss.hip) reduces the partials
// in class order.
// Forward, similarity-matrix path (everything else up to N = E = 4096): S = X X^T through embnet_dense_dgrad_f32 (the exact-fp32
// matrix-instruction GEMM, a k-ordered chain per element) into the workspace, then a sweep kernel takes one anchor row per wave
// from an LDS copy of its row of S; per-anchor partials, the same ticket and fixed-order reduction.
// Backward, one launch: Y = (G + G^T) X on the f64 matrix instructions (v_mfma_f64_16x16x4_f64), demb = (g/N) Y.  G + G^T is formed
// in f64 while staging; the result carries one fp32 rounding of an f64 sum, because the L2-normalisation backward that follows
// projects out the radial part and what remains can be far below sum_j |M_ij| |x_j|.
// Nothing is atomic in floating point, every reduction has a fixed order: bitwise reproducible.  No host synchronisation, no
// allocation: capturable in a graph.
#include <math.h>
#include "common.h"
#include "pair_loss.h"
#include "../../include/embnet.h"

namespace embnet {

static_assert(EMBNET_MS_PER_CLASS == PAIR_PER_CLASS && EMBNET_MS_SIMILARITY_MATRIX == PAIR_MATRIX, "path constants");

// (ms_t, ms_term and ms_side are pair_loss.h's: xbm.hip applies them to pair sets given by labels)
struct MsBody : PairDotBody {
  struct Args { float alpha, beta, base, eps; };
  using Sum = float;

  // One wave, one anchor (local index ai of class [lo, lo+k)), its similarity row srow[n] (LDS).  Writes all n entries of the
  // anchor's row of G and returns (the same in every lane) the anchor's loss and its kept counts (positives, negatives).
  static __device__ PairAnchorOut<float> anchor(const float* srow, int n, int k, int lo, int ai, const Args& a, float* grow, int lane) {
    const float alpha = a.alpha, beta = a.beta, base = a.base, eps = a.eps;
    float mn = INFINITY, mx = -INFINITY;
    for (int j = lane; j < k; j += 64)
      if (j != ai) mn = fminf(mn, srow[lo + j]);
    for (int col = lane; col < n; col += 64)
      if (col < lo || col >= lo + k) mx = fmaxf(mx, srow[col]);
    mn = wave_min(mn);                                     // min over the positives
    mx = wave_max(mx);                                     // max over the negatives
    const float mxe = __fadd_rn(mx, eps);
    if (!(mxe > mn)) {                                     // inactive (wave-uniform): nothing kept on either side
      for (int col = lane; col < n; col += 64) grow[col] = 0.f;
      return PairAnchorOut<float>{0.f, 0, 0};
    }
    // t is monotone in s, so the largest exponent of each side belongs to the hardest kept pair, which is kept whenever any is
    const float mp = fmaxf(0.f, ms_t(-alpha, mn, base));
    const float mg = fmaxf(0.f, ms_t(beta, mx, base));
    float sp = 0.f, sn = 0.f;
    int cp = 0, cn = 0;
    for (int j = lane; j < k; j += 64) {                   // lane-strided, column order
      const float s = srow[lo + j];
      if (j != ai && mxe > s) { sp += ms_term(-alpha, s, base, mp); ++cp; }
    }
    for (int col = lane; col < n; col += 64) {
      if (col >= lo && col < lo + k) continue;
      const float s = srow[col];
      if (__fadd_rn(s, eps) > mn) { sn += ms_term(beta, s, base, mg); ++cn; }
    }
    const float dp = __fadd_rn(expf(-mp), wave_sum(sp));   // e^{-m} + sum e^{t - m}
    const float dn = __fadd_rn(expf(-mg), wave_sum(sn));
    for (int col = lane; col < n; col += 64) {
      const float s = srow[col];
      float g = 0.f;
      if (col >= lo && col < lo + k) {
        if (col - lo != ai && mxe > s) g = -__fdiv_rn(ms_term(-alpha, s, base, mp), dp);
      } else if (__fadd_rn(s, eps) > mn) {
        g = __fdiv_rn(ms_term(beta, s, base, mg), dn);
      }
      grow[col] = g;
    }
    const float lp = ms_side(mp, dp, alpha);
    const float ln = ms_side(mg, dn, beta);
    return PairAnchorOut<float>{__fadd_rn(lp, ln), wave_sum(cp), wave_sum(cn)};
  }
  static __device__ int third(const PairAnchorOut<float>& o) { return o.c1 > 0; }   // active: it keeps a negative
  static __device__ void finish(const PairParams<MsBody>& q, double total, int c0, int c1, int c2) {
    q.counts[0] = c0;                                      // <= N (K-1)
    q.counts[1] = c1;                                      // <= N (N-K) < 2^24
    q.counts[2] = c2;
    q.counts[3] = c0 + c1;
    *q.mean = (float)(total / (double)q.n);
  }
};
using MsParams = PairParams<MsBody>;

// The shared skeleton (pair_loss.h) around MsBody.
__global__ __launch_bounds__(PAIR_CLASS_THREADS) void ms_class_fwd_kernel(MsParams q) { pair_class_fwd<MsBody>(q); }
__global__ __launch_bounds__(PAIR_SWEEP_THREADS) void ms_sweep_kernel(MsParams q) { pair_sweep_fwd<MsBody>(q); }

// ---- backward: demb = (g / N) (G + G^T) X ------------------------------------------------------------------------------
struct MsEpilogue {
  static constexpr bool ROW_SUM = false;
  const float* upstream;
  __device__ double scale(int n) const { return (upstream ? (double)*upstream : 1.0) / (double)n; }
  __device__ double value(double scale, double y, double, const float*) const { return scale * y; }
};

__global__ __launch_bounds__(256) void ms_bwd_kernel(const float* __restrict__ emb, int n, int e, const float* __restrict__ gw,
                                                     const float* __restrict__ upstream, float* __restrict__ demb) {
  pair_bwd(emb, n, e, gw, MsEpilogue{upstream}, demb);
}

}  // namespace embnet

using namespace embnet;

extern "C" size_t embnet_ms_loss_workspace_bytes(int p, int k, int e) { return pair_workspace_bytes<MsBody>(p, k, e); }

extern "C" int embnet_ms_loss_path(int p, int k, int e) { return pair_path(p, k, e); }

extern "C" int embnet_ms_loss_fwd(const float* emb, int p, int k, int e, float alpha, float beta, float base, float epsilon,
                                  int path, float* pair_g, int32_t* counts, float* mean_loss, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  int rc = pair_check_common("ms_loss_fwd", emb && pair_g && counts && mean_loss && workspace, p, k, e);
  if (rc != EMBNET_OK) return rc;
  EMBNET_CHECK_ARG(isfinite(alpha) && alpha > 0.f, "ms_loss_fwd: alpha=%g must be finite and positive", (double)alpha);
  EMBNET_CHECK_ARG(isfinite(beta) && beta > 0.f, "ms_loss_fwd: beta=%g must be finite and positive", (double)beta);
  EMBNET_CHECK_ARG(isfinite(base), "ms_loss_fwd: base=%g must be finite", (double)base);
  EMBNET_CHECK_ARG(isfinite(epsilon) && epsilon >= 0.f, "ms_loss_fwd: epsilon=%g must be finite and non-negative",
                   (double)epsilon);
  rc = pair_check_path_and_workspace("ms_loss_fwd", p, k, e, path, workspace, workspace_bytes,
                                     embnet_ms_loss_workspace_bytes(p, k, e));
  if (rc != EMBNET_OK) return rc;
  static const PairKernels<MsBody> kernels{ms_class_fwd_kernel, "embnet::ms_class_fwd_kernel", ms_sweep_kernel,
                                           "embnet::ms_sweep_kernel"};
  return pair_launch<MsBody>("ms_loss_fwd", kernels, emb, p, k, e, {alpha, beta, base, epsilon}, path, pair_g, counts, mean_loss,
                             workspace, stream);
}

extern "C" int embnet_ms_loss_bwd(const float* emb, int n, int e, const float* pair_g, const float* upstream, float* demb,
                                  void* stream) {
  const int rc = pair_check_bwd("ms_loss_bwd", emb && pair_g && demb, n, e);
  if (rc != EMBNET_OK) return rc;
  EMBNET_TRACE_FLOP("embnet::ms_bwd_kernel", 2.0 * n * n * e, 4.0 * (2.0 * n * n + 2.0 * n * e), stream);
  ms_bwd_kernel<<<dim3(cdiv(n, 32), cdiv(e, 32)), 256, 0, (hipStream_t)stream>>>(emb, n, e, pair_g, upstream, demb);
  return check_launch("ms_loss_bwd");
}
